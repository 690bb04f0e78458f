"""Batched FIRE with ASE's ExpCellFilter on the device (csrc/relax.hip ``alignn_fire_step`` with the filter's state,
``relax(optimize_lattice=True)``) against the float64 restatement in relax_ref.py: (a) the kernel alone, step by step, with injected forces and stresses,
naive and exact cell-force branches; (b) the relaxer on harmonic spring crystals (agreement with the restatement, cells at the
analytic minimum, bit-identical trajectories alone vs. in a shrinking batch); (c) the relaxer with an ALIGNNAtomWise against a
host loop over the same model; (d) run-to-run bit identity; (e) invalid input."""

import ctypes

import numpy as np
import pytest
import torch
from scipy.linalg import logm

from alignn_amd import _lib
from alignn_amd.relax import relax
from alignn_amd.synthetic import make_crystal
from tests.relax_ref import DEFAULTS, ExpCellFilterRef, FireRef, _case, exact_branch_state, run_cell_ref, sym_strain
from tests.sim_gpu import DEV, _close, _crystals, _model, _t, host_relax_loop, springs_torch
from tests.springs_ref import spring_list, springs_efs

pytestmark = pytest.mark.gpu


def _cell_step(lib, forces, energy, stress, force_ptr, active, atom_ptr, S, fmax, steps, p=DEFAULTS):
    args = _lib.FireArgs(
        forces=forces.data_ptr(), energy=energy.data_ptr(), stress=stress.data_ptr(), force_ptr=force_ptr.data_ptr(),
        active=active.data_ptr(), atom_ptr=atom_ptr.data_ptr(), inv_lattice=S["inv0"].data_ptr(), lattice0=S["lat0"].data_ptr(),
        positions=S["pos"].data_ptr(), velocities=S["vel"].data_ptr(), frac=S["frac"].data_ptr(), state=S["state"].data_ptr(),
        istate=S["istate"].data_ptr(), xa=S["xa"].data_ptr(), xc=S["xc"].data_ptr(), cell_velocities=S["cvel"].data_ptr(),
        defgrad=S["defgrad"].data_ptr(), lattice=S["lat"].data_ptr(), forces_out=S["F"].data_ptr(), energy_out=S["E"].data_ptr(),
        fmax_out=S["fmax"].data_ptr(), stress_out=S["stress"].data_ptr(), status=S["status"].data_ptr(),
        n_active=active.numel(), steps=steps, nmin=p["Nmin"], fmax=fmax, maxstep=p["maxstep"], dtmax=p["dtmax"], finc=p["finc"],
        fdec=p["fdec"], astart=p["astart"], fa=p["fa"])
    _lib.check(lib.alignn_fire_step(ctypes.byref(args), _lib.stream()), "fire_step")


def test_kernel_matches_the_restatement_step_by_step():
    lib = _lib.load()
    rng = np.random.default_rng(17)
    ns = [1, 5, 60, 300, 7]
    B = len(ns)
    C0s = [make_crystal(max(n, 2), 60 + i)[0] for i, n in enumerate(ns)]
    filts = [ExpCellFilterRef(C0s[s], n) for s, n in enumerate(ns)]
    # structures 1 and 3 start at a large log-strain L with a skewed virial: the exact cell force; the others at F = I
    # (0, 2: naive) or a ~5 % shear (4)
    Lx, Wx = exact_branch_state(5)
    X0 = []
    for s, n in enumerate(ns):
        Xa = rng.normal(0.0, 3.0, (n, 3))
        if s in (1, 3):
            Xc = n * Lx
        elif s == 4:
            Xc = n * np.real(logm(sym_strain(rng, 0.05)))
        else:
            Xc = np.zeros((3, 3))
        X0.append(np.vstack([Xa, Xc]))
    refs = [FireRef(X, **DEFAULTS) for X in X0]
    ptr = np.concatenate([[0], np.cumsum(ns)]).astype(np.int32)
    N = int(ptr[-1])
    cells = [f.atoms(X) for f, X in zip(filts, X0)]
    S = dict(lat0=_t(np.stack(C0s)), inv0=_t(np.linalg.inv(np.stack(C0s))),
             xa=_t(np.concatenate([X[:n] for X, n in zip(X0, ns)])), pos=_t(np.concatenate([c[1] for c in cells])),
             vel=torch.zeros(N, 3, dtype=torch.float64, device=DEV), frac=torch.full((N, 3), -1.0, dtype=torch.float64, device=DEV),
             xc=_t(np.stack([X[n:] for X, n in zip(X0, ns)])), cvel=torch.zeros(B, 3, 3, dtype=torch.float64, device=DEV),
             defgrad=_t(np.stack([c[2] for c in cells])), lat=_t(np.stack([c[0] for c in cells])),
             F=torch.zeros(N, 3, dtype=torch.float64, device=DEV), E=torch.zeros(B, dtype=torch.float64, device=DEV),
             stress=torch.zeros(B, 3, 3, dtype=torch.float64, device=DEV),
             state=_t([[DEFAULTS["dt"], DEFAULTS["a"]]] * B), istate=torch.zeros(B, 2, dtype=torch.int32, device=DEV),
             fmax=torch.zeros(B, dtype=torch.float64, device=DEV), status=torch.empty(1 + B, dtype=torch.int32, device=DEV))
    base_f = [rng.normal(0.0, 1.0, (n, 3)) for n in ns]
    base_s = [rng.normal(0.0, 0.01, (3, 3)) for _ in ns]
    fmax, steps = 1e-12, 24
    branches = {"naive": 0, "exact": 0}
    fire_br = set()
    for t in range(steps + 1):
        fs, ss = [], []
        for s, n in enumerate(ns):
            C = filts[s].atoms(refs[s].r)[0]
            V = abs(np.linalg.det(C))
            if s in (1, 3):  # the skewed virial, slowly varying
                st = -Wx / V * (1.0 + 0.02 * rng.normal()) + 1e-3 * rng.normal(0.0, 1.0, (3, 3))
            else:  # not symmetric: the kernel symmetrises
                st = base_s[s] + (0.002 if s in (0, 2) else 0.05) * rng.normal(0.0, 1.0, (3, 3))
            fs.append(base_f[s] + (0.05 if s in (0, 2) else 2.0) * rng.normal(0.0, 1.0, (n, 3)))
            ss.append(st)
        e = rng.normal(size=B)
        active = torch.arange(B, dtype=torch.int32, device=DEV)
        _cell_step(lib, _t(np.concatenate(fs)), _t(e), _t(np.stack(ss)), _t(ptr, torch.int32), active, _t(ptr, torch.int32), S,
                   fmax, steps)
        st = S["status"].cpu().numpy()
        want = [0 if t < steps else 2] * B
        assert st[1:].tolist() == want and st[0] == want.count(0), (t, st)
        for s, n in enumerate(ns):
            o, filt = refs[s], filts[s]
            g = filt.forces(o.r, fs[s], ss[s])
            branches[filt.branch] += 1
            assert S["fmax"][s].item() == pytest.approx(np.sqrt((g ** 2).sum(1).max()), rel=1e-12), (t, s)
            np.testing.assert_array_equal(S["F"][ptr[s]:ptr[s + 1]].cpu().numpy(), fs[s])
            assert _close(S["stress"][s].cpu().numpy(), (ss[s] + ss[s].T) / 2, 1e-15)
            assert S["E"][s].item() == e[s]
            if t == steps:
                continue
            if o.v is not None:
                P = np.vdot(g, o.v)
                fire_br.add("mix" if P > 0 else "reset")
            r0 = o.r.copy()
            o.step(g)
            if np.linalg.norm(o.r - r0) > o.maxstep * (1 - 1e-12):
                fire_br.add("clip")
        for s, n in enumerate(ns):
            o, filt = refs[s], filts[s]
            a, b = ptr[s], ptr[s + 1]
            C, pos, F = filt.atoms(o.r)
            assert _close(S["xa"][a:b].cpu().numpy(), o.r[:n]), (t, s)
            assert _close(S["xc"][s].cpu().numpy(), o.r[n:]), (t, s)
            assert _close(S["pos"][a:b].cpu().numpy(), pos), (t, s)
            assert _close(S["lat"][s].cpu().numpy(), C), (t, s)
            assert _close(S["defgrad"][s].cpu().numpy(), F), (t, s)
            if o.v is not None:
                assert _close(S["vel"][a:b].cpu().numpy(), o.v[:n]), (t, s)
                assert _close(S["cvel"][s].cpu().numpy(), o.v[n:]), (t, s)
            dt, aa = S["state"][s].tolist()
            nst, taken = S["istate"][s].tolist()
            assert dt == pytest.approx(o.dt, rel=1e-12) and aa == pytest.approx(o.a, rel=1e-12) and nst == o.Nsteps, (t, s)
            assert taken == min(t + 1, steps)
            fr = S["frac"][a:b].cpu().numpy()
            assert (fr >= 0.0).all() and (fr < 1.0).all()
            d = fr - o.r[:n] @ np.linalg.inv(C0s[s])
            assert np.abs(d - np.round(d)).max() < 1e-9
    print("cell-force branches over the run:", branches, "FIRE branches:", fire_br)
    assert branches["exact"] >= steps + 1 and branches["naive"] >= 3 * (steps + 1)
    assert {"mix", "reset", "clip"} <= fire_br, fire_br


# --- (b) harmonic spring crystals through forces_fn --------------------------------------------------------------------------
SIZES = [1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 16, 20]


def _spring_cases():
    cases = []
    for i, n in enumerate(SIZES):
        lat_t, frac_t, C0, pos0 = _case(20 + i, n, 0.02 + 0.01 * (i % 5))
        cases.append((lat_t, frac_t, C0, pos0, spring_list(lat_t, frac_t, nnb=14)))
    return cases


def test_relax_cell_springs_match_the_restatement_alone_or_batched():
    cases = _spring_cases()
    fmax, steps = 1e-6, 4000
    rec_b = {}
    res = relax(None, [c[2] for c in cases], [c[3] for c in cases], fmax=fmax, steps=steps,
                forces_fn=springs_torch(cases, rec_b), device=DEV, optimize_lattice=True)
    want_steps = []
    for s, (lat_t, frac_t, C0, pos0, sl) in enumerate(cases):
        ref = run_cell_ref(C0, pos0, springs_efs(*sl), fmax=fmax, steps=steps)
        assert ref["converged"], s
        want_steps.append(ref["n_steps"])
        got_p, got_c = res.positions[s].cpu().numpy(), res.lattices[s].cpu().numpy()
        assert np.abs(got_p - ref["pos"]).max() <= 1e-9 * max(1.0, np.abs(ref["pos"]).max()), s
        assert np.abs(got_c - ref["C"]).max() <= 1e-9 * np.abs(ref["C"]).max(), s
        assert res.energies[s].item() == pytest.approx(ref["e"], rel=1e-6, abs=1e-12)
        assert np.abs(res.stresses[s].cpu().numpy() - (ref["s"] + ref["s"].T) / 2).max() <= 1e-9
        assert np.abs(res.forces[s].cpu().numpy() - ref["f"]).max() <= 1e-9
        assert res.fmax[s].item() < fmax
        # the analytic minimum: the target cell (F symmetric admits no rotation), atoms at the target up to a translation
        np.testing.assert_allclose(got_c, lat_t, atol=1e-4 * np.abs(lat_t).max())
        rel = got_p - got_p[0]
        np.testing.assert_allclose(rel, frac_t @ lat_t - frac_t[0] @ lat_t, atol=1e-4 * np.abs(lat_t).max())
    assert res.converged.all().item()
    assert res.n_steps.tolist() == want_steps
    assert len(set(want_steps)) > 4  # the batch shrinks
    assert res.n_evals == max(want_steps) + 1
    for s, c in enumerate(cases):
        rec_a = {}
        alone = relax(None, [c[2]], [c[3]], fmax=fmax, steps=steps, forces_fn=springs_torch(cases, rec_a), device=DEV,
                      optimize_lattice=True)
        n = SIZES[s]
        ta, tb = rec_a[n], rec_b[n]
        assert len(ta) == len(tb) == want_steps[s] + 1, s
        assert all(torch.equal(x[0], y[0]) and torch.equal(x[1], y[1]) for x, y in zip(ta, tb)), s
        assert torch.equal(alone.positions[0], res.positions[s]) and torch.equal(alone.lattices[0], res.lattices[s])
        assert alone.n_steps.item() == want_steps[s]


# --- (c), (d), (e) a random-initialised ALIGNNAtomWise ---------------------------------------------------------------------
def _host_loop(model, lats, pos, feats, fmax, steps, stress_weight=1.0):
    """The reference's loop, batched by hand (sim_gpu.host_relax_loop): model(crystal_batch(active)) on the device with fresh
    lattice tensors every step, the calculator's rules, ExpCellFilter and FIRE as the numpy restatement."""
    filts = [ExpCellFilterRef(l, len(p)) for l, p in zip(lats, pos)]
    opts, _, taken, branches = host_relax_loop(model, lats, pos, feats, fmax, steps, filts, stress_weight)
    res = [f.atoms(o.r) for f, o in zip(filts, opts)]
    return [r[1] for r in res], [r[0] for r in res], taken, branches


def test_relax_cell_model_matches_a_host_loop():
    model = _model()
    lats, pos, feats = _crystals()
    res = relax(model, lats, pos, feats, fmax=0.0, steps=10, optimize_lattice=True)
    p_host, c_host, taken, _ = _host_loop(model, lats, pos, feats, 0.0, 10)
    assert res.n_steps.tolist() == taken == [10] * 8 and res.n_evals == 11 and not res.converged.any()
    dpos = max(np.abs(res.positions[s].cpu().numpy() - p_host[s]).max() for s in range(8))
    dlat = max(np.abs(res.lattices[s].cpu().numpy() - c_host[s]).max() for s in range(8))
    moved = max(np.abs(c_host[s] - lats[s]).max() for s in range(8))
    print(f"relax(optimize_lattice) vs host loop after 10 steps: max |dpos| {dpos:.3e} A, max |dlat| {dlat:.3e} A "
          f"(cells moved up to {moved:.3e} A)")
    assert moved > 1e-3
    # measured on an MI355X: max |dpos| 1.8e-15 A, max |dlat| 1.1e-16 A (fused multiply-adds and reduction order against
    # numpy and scipy; the model sees the same float32 graphs).  Tolerances 3x the larger.
    assert dpos <= 3 * 1.8e-15 and dlat <= 3 * 1.8e-15, (dpos, dlat)


def test_relax_cell_model_is_bit_reproducible():
    model = _model()
    lats, pos, feats = _crystals(4)
    a = relax(model, lats, pos, feats, fmax=0.05, steps=6, optimize_lattice=True)
    b = relax(model, lats, pos, feats, fmax=0.05, steps=6, optimize_lattice=True)
    for x, y in zip(a.positions + a.forces, b.positions + b.forces):
        assert torch.equal(x, y)
    assert torch.equal(a.lattices, b.lattices) and torch.equal(a.stresses, b.stresses)
    assert torch.equal(a.energies, b.energies) and torch.equal(a.fmax, b.fmax) and torch.equal(a.n_steps, b.n_steps)


def test_relax_cell_validates_its_inputs():
    lats, pos, feats = _crystals(2)
    with pytest.raises(ValueError, match="stress"):
        relax(_model(stresswise_weight=0.0), lats, pos, feats, optimize_lattice=True)
    with pytest.raises(ValueError, match="stress"):
        relax(_model(batch_stress=False), lats, pos, feats, optimize_lattice=True)
    cases = _spring_cases()[:2]
    fn = springs_torch(cases)
    with pytest.raises(ValueError, match="forces_fn"):
        relax(None, [c[2] for c in cases], [c[3] for c in cases], forces_fn=lambda l, p: fn(l, p)[:2], device=DEV,
              optimize_lattice=True)
    with pytest.raises(ValueError):
        relax(None, [c[2] for c in cases], [c[3] for c in cases], device=DEV, optimize_lattice=True,
              forces_fn=lambda l, p: (*fn(l, p)[:2], torch.zeros(1, 3, 3, device=DEV)))
