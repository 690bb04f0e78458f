"""Batched FIRE relaxation on the device (csrc/relax.hip, alignn_amd/relax.py) against the float64 restatement of ASE's FIRE and
Optimizer.run in relax_ref.py: (a) the kernel alone, step by step; (b) the relaxer on harmonic springs (convergence, step
counts, and bit-identical trajectories alone vs. in a batch whose other members retire earlier); (c) the relaxer with an
ALIGNNAtomWise against a host loop over the same model; (d) run-to-run bit identity."""

import ctypes

import numpy as np
import pytest
import torch

from alignn_amd import _lib
from alignn_amd.relax import relax
from alignn_amd.synthetic import make_crystal
from tests.relax_ref import DEFAULTS, FireRef, converged, run_ref
from tests.sim_gpu import DEV, _crystals, _model, host_relax_loop

pytestmark = pytest.mark.gpu


def _fire_step(lib, forces, energy, force_ptr, active, atom_ptr, inv, S, fmax, steps, p=DEFAULTS):
    args = _lib.FireArgs(
        forces=forces.data_ptr(), energy=energy.data_ptr(), force_ptr=force_ptr.data_ptr(), active=active.data_ptr(),
        atom_ptr=atom_ptr.data_ptr(), inv_lattice=inv.data_ptr(), positions=S["pos"].data_ptr(), velocities=S["vel"].data_ptr(),
        frac=S["frac"].data_ptr(), state=S["state"].data_ptr(), istate=S["istate"].data_ptr(), forces_out=S["F"].data_ptr(),
        energy_out=S["E"].data_ptr(), fmax_out=S["fmax"].data_ptr(), status=S["status"].data_ptr(), n_active=active.numel(),
        steps=steps, nmin=p["Nmin"], fmax=fmax, maxstep=p["maxstep"], dtmax=p["dtmax"], finc=p["finc"], fdec=p["fdec"],
        astart=p["astart"], fa=p["fa"])
    _lib.check(lib.alignn_fire_step(ctypes.byref(args), _lib.stream()), "fire_step")


def test_kernel_matches_the_restatement_step_by_step():
    lib = _lib.load()
    rng = np.random.default_rng(7)
    ns = [1, 5, 60, 300, 4]  # the last structure feels no force: it retires at the first check
    B = len(ns)
    lats = [make_crystal(max(n, 2), 40 + i)[0] for i, n in enumerate(ns)]
    pos0 = [rng.normal(0.0, 3.0, (n, 3)) for n in ns]
    ptr = np.concatenate([[0], np.cumsum(ns)]).astype(np.int32)
    inv = torch.linalg.inv(torch.tensor(np.stack(lats), device=DEV)).contiguous()
    N = int(ptr[-1])
    S = dict(pos=torch.tensor(np.concatenate(pos0), device=DEV), vel=torch.zeros(N, 3, dtype=torch.float64, device=DEV),
             frac=torch.full((N, 3), -1.0, dtype=torch.float64, device=DEV), F=torch.zeros(N, 3, dtype=torch.float64, device=DEV),
             E=torch.zeros(B, dtype=torch.float64, device=DEV),
             state=torch.tensor([[DEFAULTS["dt"], DEFAULTS["a"]]] * B, dtype=torch.float64, device=DEV),
             istate=torch.zeros(B, 2, dtype=torch.int32, device=DEV), fmax=torch.zeros(B, dtype=torch.float64, device=DEV),
             status=torch.empty(1 + B, dtype=torch.int32, device=DEV))
    refs = [FireRef(p, **DEFAULTS) for p in pos0]
    base = [rng.normal(0.0, 1.0, (n, 3)) for n in ns]
    fmax, steps = 1e-9, 12
    active = list(range(B))
    branches = set()
    n_taken = [0] * B
    for t in range(steps + 1):
        # structures 0 and 2 see slowly varying forces (downhill: mixing, dt growth after Nmin), 1 and 3 fresh random ones
        # (uphill resets); structure 3 moves far enough to hit maxstep
        fs = [base[s] + (0.05 if s in (0, 2) else 3.0) * rng.normal(0.0, 1.0, base[s].shape) for s in range(B)]
        fs[4] = np.zeros((ns[4], 3))
        f_act = np.concatenate([fs[s] for s in active])
        e_act = rng.normal(size=len(active))
        fp = np.concatenate([[0], np.cumsum([ns[s] for s in active])]).astype(np.int32)
        _fire_step(lib, torch.tensor(f_act, device=DEV), torch.tensor(e_act, device=DEV), torch.tensor(fp, device=DEV),
                   torch.tensor(active, dtype=torch.int32, device=DEV), torch.tensor(ptr, device=DEV), inv, S, fmax, steps)
        st = S["status"][:1 + len(active)].cpu().numpy()
        want = []
        for k, s in enumerate(active):
            conv = converged(fs[s], fmax)
            want.append(1 if conv else (2 if t >= steps else 0))
            if not want[-1]:
                o = refs[s]
                if o.v is not None:
                    P = np.vdot(fs[s], o.v)
                    branches.add("mix" if P > 0 else "reset")
                    if P > 0 and o.Nsteps > o.Nmin:
                        branches.add("grow")
                r_before = o.r.copy()
                o.step(fs[s])
                n_taken[s] += 1
                if np.linalg.norm(o.r - r_before) > o.maxstep * (1 - 1e-12):
                    branches.add("clip")
            assert S["E"][s].item() == e_act[k]
            np.testing.assert_array_equal(S["F"][ptr[s]:ptr[s + 1]].cpu().numpy(), fs[s])
            assert S["fmax"][s].item() == pytest.approx(np.sqrt((fs[s] ** 2).sum(1).max()), rel=1e-14, abs=1e-300)
        assert st[1:].tolist() == want and st[0] == want.count(0), (t, st, want)
        for s in range(B):
            o = refs[s]
            a, b = ptr[s], ptr[s + 1]
            pos = S["pos"][a:b].cpu().numpy()
            assert np.abs(pos - o.r).max() <= 1e-12 * max(1.0, np.abs(o.r).max()), (t, s)
            if o.v is not None:
                vel = S["vel"][a:b].cpu().numpy()
                assert np.abs(vel - o.v).max() <= 1e-12 * max(1.0, np.abs(o.v).max()), (t, s)
            dt, aa = S["state"][s].tolist()
            nst, taken = S["istate"][s].tolist()
            assert dt == pytest.approx(o.dt, rel=1e-12) and aa == pytest.approx(o.a, rel=1e-12) and nst == o.Nsteps, (t, s)
            assert taken == n_taken[s]
            if s != 4 and t < steps:  # every stepped structure has its wrapped fractional coordinates
                fr = S["frac"][a:b].cpu().numpy()
                assert (fr >= 0.0).all() and (fr < 1.0).all()
                want_fr = o.r @ np.linalg.inv(lats[s])
                d = fr - want_fr
                assert np.abs(d - np.round(d)).max() < 1e-9
        active = [s for s, w in zip(active, want) if w == 0]
        if not active:
            break
    assert S["istate"][:, 1].tolist() == [steps, steps, steps, steps, 0]
    assert {"mix", "reset", "grow", "clip"} <= branches, branches


# --- (b) harmonic springs: every structure has its minimum at fractional targets (fixed per atom count) of its own cell ---------
def _targets(n):
    return np.random.default_rng(1000 + n).uniform(0.0, 1.0, (n, 3))


def _k(n):
    return 0.5 + 2.0 * ((np.arange(n) * 7) % 5) / 4.0


def _minimum(lat, t):  # fixed elementwise order: the same bits from numpy and from torch
    return t[:, 0:1] * lat[0] + t[:, 1:2] * lat[1] + t[:, 2:3] * lat[2]


def springs_torch(record=None):
    def fn(lats, poss):
        es, fs = [], []
        for lat, pos in zip(lats, poss):
            n = pos.shape[0]
            d = pos - _minimum(lat, torch.tensor(_targets(n), device=pos.device))
            k = torch.tensor(_k(n), device=pos.device)
            fs.append(-k[:, None] * d)
            es.append(0.5 * (k * (d * d).sum(1)).sum())
            if record is not None:
                record.setdefault(lat.cpu().numpy().tobytes(), []).append(pos.clone())
        return torch.stack(es), torch.cat(fs)

    return fn


def springs_numpy(lat, n):
    m, k = _minimum(lat, _targets(n)), _k(n)

    def ef(r):
        d = r - m
        return 0.5 * float((k * (d * d).sum(1)).sum()), -k[:, None] * d

    return ef


def _spring_cases():
    sizes = [1, 2, 3, 5, 8, 13, 21, 34, 40, 4, 6, 9, 12, 17, 25, 30]
    lats, pos = [], []
    for i, n in enumerate(sizes):
        lat = make_crystal(max(n, 2), 500 + i)[0]
        rng = np.random.default_rng(i)
        lats.append(lat)
        pos.append(_minimum(lat, _targets(n)) + rng.normal(0.0, 0.3 + 0.1 * (i % 4), (n, 3)))
    return lats, pos


def test_relax_springs_converge_like_the_restatement_alone_or_batched():
    lats, pos = _spring_cases()
    fmax, steps = 1e-3, 500
    rec_b = {}
    res = relax(None, lats, pos, fmax=fmax, steps=steps, forces_fn=springs_torch(rec_b), device=DEV)
    want_steps = []
    for s, (lat, p) in enumerate(zip(lats, pos)):
        ref = run_ref(p, springs_numpy(lat, len(p)), fmax=fmax, steps=steps)
        assert ref["converged"]
        want_steps.append(ref["n_steps"])
        got = res.positions[s].cpu().numpy()
        assert np.abs(got - ref["r"]).max() <= 1e-10 * max(1.0, np.abs(ref["r"]).max()), s
        assert np.abs(got - _minimum(lat, _targets(len(p)))).max() < fmax / 0.5  # at the minimum within fmax / k_min
        assert res.energies[s].item() == pytest.approx(ref["e"], rel=1e-9, abs=1e-12)
        assert np.abs(res.forces[s].cpu().numpy() - ref["f"]).max() <= 1e-10
        assert res.fmax[s].item() < fmax
    assert res.converged.all().item()
    assert res.n_steps.tolist() == want_steps
    assert len(set(want_steps)) > 4  # structures retire at different steps: the batch shrinks
    assert res.n_evals == max(want_steps) + 1
    # each structure alone: the same trajectory, bit for bit, as inside the shrinking batch of 16
    for s, (lat, p) in enumerate(zip(lats, pos)):
        rec_a = {}
        alone = relax(None, [lat], [p], fmax=fmax, steps=steps, forces_fn=springs_torch(rec_a), device=DEV)
        key = torch.tensor(lat, device=DEV).cpu().numpy().tobytes()
        ta, tb = rec_a[key], rec_b[key]
        assert len(ta) == len(tb) == want_steps[s] + 1, s
        assert all(torch.equal(x, y) for x, y in zip(ta, tb)), s
        assert torch.equal(alone.positions[0], res.positions[s]) and alone.n_steps.item() == want_steps[s]


# --- (c), (d) a random-initialised ALIGNNAtomWise --------------------------------------------------------------------------
def _host_loop(model, lats, pos, feats, fmax, steps):
    """The reference's loop, batched by hand (sim_gpu.host_relax_loop): model(crystal_batch(active)) on the device, FIRE as the
    numpy restatement."""
    opts, energies, taken, _ = host_relax_loop(model, lats, pos, feats, fmax, steps)
    return [o.r for o in opts], energies, taken


def test_relax_model_matches_a_host_loop():
    model = _model()
    lats, pos, feats = _crystals()
    res = relax(model, lats, pos, feats, fmax=0.0, steps=10)
    r_host, e_host, taken = _host_loop(model, lats, pos, feats, 0.0, 10)
    assert res.n_steps.tolist() == taken == [10] * 8 and res.n_evals == 11 and not res.converged.any()
    dpos = max(np.abs(res.positions[s].cpu().numpy() - r_host[s]).max() for s in range(8))
    de = np.abs(res.energies.cpu().numpy() - e_host).max() / np.abs(e_host).max()
    moved = max(np.abs(r_host[s] - pos[s]).max() for s in range(8))
    print(f"relax vs host loop after 10 steps: max |dpos| {dpos:.3e} A (atoms moved up to {moved:.3e} A), energy rel {de:.3e}")
    assert moved > 1e-3
    # measured on an MI355X: max |dpos| 8.9e-16 A (the kernel's fused multiply-adds and reduction order against numpy's), energies
    # bit-equal (0.0).  Tolerances 3x that; for the energies 3x one float32 rounding, as 3 x 0 bounds nothing.
    assert dpos <= 3 * 8.9e-16 and de <= 3 * 2.0 ** -24, (dpos, de)


def test_relax_model_is_bit_reproducible():
    model = _model()
    lats, pos, feats = _crystals(4)
    a = relax(model, lats, pos, feats, fmax=0.05, steps=6)
    b = relax(model, lats, pos, feats, fmax=0.05, steps=6)
    for x, y in zip(a.positions + a.forces, b.positions + b.forces):
        assert torch.equal(x, y)
    assert torch.equal(a.energies, b.energies) and torch.equal(a.fmax, b.fmax) and torch.equal(a.n_steps, b.n_steps)


def test_relax_validates_its_inputs():
    model = _model()
    lats, pos, feats = _crystals(2)
    with pytest.raises(ValueError):
        relax(model.train(), lats, pos, feats)
    model.eval()
    with pytest.raises(ValueError):
        relax(model, lats, pos, [feats[0], feats[0]])
    with pytest.raises(ValueError):
        relax(model, lats, pos)
    with pytest.raises(ValueError):
        relax(model, lats[:1], pos, feats)
