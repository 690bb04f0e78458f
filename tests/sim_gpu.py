"""What the GPU tests of the batched drivers (``relax``, ``run_md``, ``phonons``) share, each once: the small comparisons, the
random ``ALIGNNAtomWise`` and its crystals, the periodic spring crystals as device ``forces_fn``s, and the reference's loop
batched by hand - one host-side evaluation of the model under the calculator's rules and one loop each over the restated
integrators and over the restated FIRE.  The evaluation is the tests' own statement of what ``alignn_amd/_structures.py`` does
for the drivers and takes nothing from it.  Imported by GPU test modules only."""

import numpy as np
import torch

from alignn_amd import ALIGNNAtomWise, ALIGNNAtomWiseConfig, neighbors
from alignn_amd.synthetic import make_crystal
from tests.relax_ref import DEFAULTS, FireRef, converged
from tests.springs_ref import spring_list

DEV = "cuda"


def _t(x, dtype=torch.float64):
    return torch.tensor(np.ascontiguousarray(x), dtype=dtype, device=DEV)


def _rel(got, want):
    return np.abs(got - want).max() / max(1.0, np.abs(want).max())


def _relmax(got, want):
    return np.abs(got - want).max() / np.abs(want).max()


def _close(got, want, rel=1e-12):
    return np.abs(got - want).max() <= rel * max(1.0, np.abs(want).max())


# --- a random-initialised ALIGNNAtomWise and its crystals ----------------------------------------------------------------------
def _model(**kw):
    torch.manual_seed(0)
    cfg = dict(name="alignn_atomwise", alignn_layers=2, gcn_layers=2, hidden_features=128, embedding_features=64,
               atom_input_features=92, calculate_gradient=True, stresswise_weight=0.05)
    cfg.update(kw)
    return ALIGNNAtomWise(ALIGNNAtomWiseConfig(**cfg)).to(DEV).eval()


def _crystals(B=8, n=24):
    lats, pos, feats = [], [], []
    g = torch.Generator().manual_seed(3)
    for i in range(B):
        lat, frac, _ = make_crystal(n + 2 * i, 900 + i)
        lats.append(lat)
        pos.append(frac @ lat)
        feats.append(torch.randn(n + 2 * i, 92, generator=g))
    return lats, pos, feats


def _md_crystals(B=6, n=24):
    """``_crystals`` with masses, and the batch of six that the MD tests use."""
    lats, pos, feats = _crystals(B, n)
    return lats, pos, feats, [np.random.default_rng(i).uniform(1.0, 100.0, n + 2 * i) for i in range(B)]


# --- periodic spring crystals (forces_fn) -----------------------------------------------------------------------------------
class Springs:
    """Each atom tied to its 8 nearest neighbours of the start structure (springs_ref.spring_list), at rest there.  The
    forces gather every atom's springs through a fixed table and sum them in a fixed order (no atomics): the same bits for a
    structure whatever else is evaluated beside it."""

    def __init__(self, lats, fracs):
        self.tabs = []
        for lat, frac in zip(lats, fracs):
            I, J, img, d0, k = spring_list(lat, frac, nnb=8)
            n = len(frac)
            rows = [[] for _ in range(n)]
            for e, (i, j) in enumerate(zip(I, J)):
                rows[i].append((e, 1.0))
                rows[j].append((e, -1.0))
            deg = max(len(r) for r in rows)
            idx, sgn = np.zeros((n, deg), dtype=np.int64), np.zeros((n, deg))
            for i, r in enumerate(rows):
                for c, (e, sg) in enumerate(r):
                    idx[i, c], sgn[i, c] = e, sg
            shift = img[:, 0:1] * lat[0] + img[:, 1:2] * lat[1] + img[:, 2:3] * lat[2]
            self.tabs.append(tuple(_t(x) if x.dtype != np.int64 else _t(x, torch.int64) for x in (I, J, shift, d0, k, idx, sgn)))

    def __call__(self, lats, poss):
        es, fs = [], []
        for (I, J, shift, d0, k, idx, sgn), pos in zip(self.tabs, poss):
            d = pos[J] - pos[I] + shift
            r = torch.sqrt((d * d).sum(1))
            fv = (k * (r - d0) / r)[:, None] * d
            fs.append((fv[idx] * sgn[..., None]).sum(1))
            es.append(0.5 * (k * (r - d0) ** 2).sum())
        return torch.stack(es), torch.cat(fs)

    def subset(self, which):
        out = Springs.__new__(Springs)
        out.tabs = [self.tabs[s] for s in which]
        return out


def _spring_crystals(sizes, seed0):
    lats, fracs = [], []
    for i, n in enumerate(sizes):
        lat, frac, _ = make_crystal(n, seed0 + i)
        lats.append(lat)
        fracs.append(frac)
    return lats, [f @ l for f, l in zip(fracs, lats)], Springs(lats, fracs)


def _second_half_mean(res):
    T = res.temperature.cpu().numpy()
    return T[T.shape[0] // 2:].mean(0)


# --- periodic spring crystals with stresses ------------------------------------------------------------------------------------
def _det3(m):
    return (m[0, 0] * (m[1, 1] * m[2, 2] - m[1, 2] * m[2, 1]) - m[0, 1] * (m[1, 0] * m[2, 2] - m[1, 2] * m[2, 0])
            + m[0, 2] * (m[1, 0] * m[2, 1] - m[1, 1] * m[2, 0]))


def springs_torch(cases, record=None):
    """springs_efs on the device with reductions of a fixed order only (no atomics, no BLAS): the same bits for a structure
    whatever else is evaluated beside it."""
    tabs = {}
    for c in cases:
        I, J, img, d0, k = c[4]
        n = len(c[3])
        inc = np.zeros((n, len(I)))  # +1 at the spring's first atom, -1 at its second (0 for a spring to an own image)
        np.add.at(inc, (I, np.arange(len(I))), 1.0)
        np.add.at(inc, (J, np.arange(len(I))), -1.0)
        tabs[n] = tuple(torch.tensor(x, device=DEV) for x in (I, J, img, d0, k, inc))

    def fn(lats, poss):
        es, fs, ss = [], [], []
        for lat, pos in zip(lats, poss):
            n = pos.shape[0]
            I, J, img, d0, k, inc = tabs[n]
            d = pos[J] - pos[I] + (img[:, 0:1] * lat[0] + img[:, 1:2] * lat[1] + img[:, 2:3] * lat[2])
            r = torch.sqrt((d * d).sum(1))
            dphi = k * (r - d0)
            fv = (dphi / r)[:, None] * d
            fs.append((inc[:, :, None] * fv[None, :, :]).sum(1))
            ss.append((fv[:, :, None] * d[:, None, :]).sum(0) / _det3(lat).abs())
            es.append(0.5 * (k * (r - d0) ** 2).sum())
            if record is not None:
                record.setdefault(n, []).append((lat.clone(), pos.clone()))
        return torch.stack(es), torch.cat(fs), torch.stack(ss)

    return fn


def _stress_springs(sizes, seed0, nnb=14):
    """Crystals of distinct sizes at rest in their springs (springs_ref.spring_list) -> lattices, positions, the numpy
    spring lists and the device ``forces_fn`` with stresses (springs_torch, fixed-order sums)."""
    assert len(set(sizes)) == len(sizes), sizes  # (springs_torch finds a structure's table by its atom count)
    lats, pos, sls, cases = [], [], [], []
    for i, n in enumerate(sizes):
        lat, frac, _ = make_crystal(n, seed0 + i)
        sl = spring_list(lat, frac, nnb=nnb)
        lats.append(lat)
        pos.append(frac @ lat)
        sls.append(sl)
        cases.append((lat, frac, lat, frac @ lat, sl))
    return lats, pos, sls, springs_torch(cases)


def _no_stress(fn):
    return lambda lats, poss: fn(lats, poss)[:2]


# --- the reference's loop, batched by hand --------------------------------------------------------------------------------------
def host_evaluate(model, cells, positions, feats, stress_weight=None, frac_cells=None):
    """model(crystal_batch(...)) on the device for the structures ``(cells[s], positions[s])``, the fractions wrapped into [0, 1)
    (those of ``positions[s]`` in ``frac_cells[s]`` where given: the filter's X_a are Cartesian in the original cell), and the
    calculator's rules: the energy is out * n in float32, the forces are grad, the stress (``stress_weight`` not None) is the
    symmetrised one * stress_weight / 160.21766208 (eV/A^3) in float32.  -> (e [B], [forces [n, 3]], stress [B, 3, 3] or None),
    float64 numpy."""
    fr = []
    for s, r in enumerate(positions):
        f = r @ np.linalg.inv((frac_cells or cells)[s])
        f = f - np.floor(f)
        fr.append(torch.tensor(np.where(f < 1.0, f, 0.0), device=DEV))
    out = model(neighbors.crystal_batch([torch.tensor(c, device=DEV) for c in cells], fr, atom_features=feats, device=DEV))
    ptr = np.concatenate([[0], np.cumsum([len(r) for r in positions])])
    n_t = torch.tensor([len(r) for r in positions], dtype=torch.float32, device=DEV)
    e = (out["out"].detach().reshape(-1).float() * n_t).double().cpu().numpy()
    F = out["grad"].detach().reshape(-1, 3).double().cpu().numpy()
    st = None
    if stress_weight is not None:
        st = out["stresses"].detach().reshape(-1, 3, 3).float()
        st = ((st + st.transpose(1, 2)) / 2 * stress_weight / 160.21766208).double().cpu().numpy()
    return e, [F[ptr[s]:ptr[s + 1]] for s in range(len(positions))], st


def host_md_loop(model, refs, lats, feats, steps, stress="", observe=None):
    """``steps`` steps of the restated integrators ``refs`` (``begin`` / ``finish``; md_ref.py, md_npt_ref.py,
    md_nose_hoover_ref.py) around host_evaluate, in the cell ``o.cell`` of an integrator that has one and in ``lats[s]``
    otherwise.  ``stress``: "" (none evaluated), "begin" (``begin`` takes it) or "both" (``begin`` and ``finish`` do).
    -> (e_pot [steps + 1, B], ``observe(o, e, stress)`` of every structure after every evaluation [steps + 1, B])."""

    def evaluate():
        cells = [getattr(o, "cell", lats[s]) for s, o in enumerate(refs)]
        return host_evaluate(model, cells, [o.r for o in refs], feats, 1.0 if stress else None)

    def seen(e, st):
        return [observe(o, e[s], st[s] if stress else None) for s, o in enumerate(refs)] if observe else None

    e, F, st = evaluate()
    epot, obs = [e], [seen(e, st)]
    for _ in range(steps):
        for s, o in enumerate(refs):
            o.begin(F[s], st[s]) if stress else o.begin(F[s])
        e, F, st = evaluate()
        for s, o in enumerate(refs):
            o.finish(F[s], st[s]) if stress == "both" else o.finish(F[s])
            o.nsteps += 1
        epot.append(e)
        obs.append(seen(e, st))
    return np.array(epot), np.array(obs)


def host_relax_loop(model, lats, pos, feats, fmax, steps, filts=None, stress_weight=1.0):
    """``Optimizer.run(fmax, steps)`` of the restated FIRE (relax_ref.py) for every structure around host_evaluate of those still
    running, at fixed cell or through the cell filters ``filts`` (fresh lattice tensors every step).
    -> (the FireRefs, last energies [B], steps taken, the cell-force branches met)."""
    n = [len(p) for p in pos]
    opts = [FireRef(p if filts is None else filts[s].initial(p), **DEFAULTS) for s, p in enumerate(pos)]
    taken, energies, branches = [0] * len(pos), [None] * len(pos), set()
    active = list(range(len(pos)))
    while active:
        cells = [lats[s] if filts is None else filts[s].atoms(opts[s].r)[0] for s in active]
        e, F, st = host_evaluate(model, cells, [opts[s].r[:n[s]] for s in active], [feats[s] for s in active],
                                 None if filts is None else stress_weight, [lats[s] for s in active])
        nxt = []
        for k, s in enumerate(active):
            energies[s] = e[k]
            g = F[k]
            if filts is not None:
                g = filts[s].forces(opts[s].r, F[k], st[k])
                branches.add(filts[s].branch)
            if converged(g, fmax) or taken[s] >= steps:
                continue
            opts[s].step(g)
            taken[s] += 1
            nxt.append(s)
        active = nxt
    return opts, np.array(energies), taken, branches
