"""The constraints of the batched FIRE relaxer on the device (csrc/relax.hip: ``fixed``, ``cell_mask``, ``scalar_pressure``,
``hydrostatic_strain``, ``constant_volume`` and ``enthalpy_out`` of ``alignn_fire_args``; ``relax(fixed=, cell_mask=, ...)``)
against the float64 restatement in relax_ref.py.  Three structures of 1, 2 and 7 atoms in one launch: one atom
per workgroup, fewer atoms than lanes, a ragged batch.  (1) the kernel alone, step by step, forces and stresses of the spring
potential from the host, each option alone and all together; (2) the relaxer on spring crystals, alone and batched; (3) the
options passed but off give the bits of a call without them; (4) a fixed atom at fixed cell; (5) the relaxer with an
ALIGNNAtomWise against a host loop over the same model."""

import ctypes

import numpy as np
import pytest
import torch
from scipy.linalg import expm

from alignn_amd import _lib
from alignn_amd.relax import relax
from alignn_amd.synthetic import make_crystal
from tests.relax_ref import (DEFAULTS, SLAB, ConstrainedFilterRef, FireRef, _case, run_constrained_ref, run_fixed_ref, sym_strain,
                             voigt_mask)
from tests.sim_gpu import DEV, _close, _crystals, _model, _t, host_relax_loop, springs_torch
from tests.springs_ref import spring_list, springs_efs

pytestmark = pytest.mark.gpu
NS = [1, 2, 7]
FIXED = [np.array([False]), np.array([False, True]), np.array([False, False, False, True, False, False, False])]
TWO_FIXED = np.array([False, False, False, True, False, True, False])
DIAG = [1, 1, 1, 0, 0, 0]


# --- (1) the kernel, step by step --------------------------------------------------------------------------------------------
def kernel_cases(masks):
    """Per structure (C0, X0, efs): the 1-atom one at F = I, the 7-atom one at a ~5 % log-strain, the 2-atom one at a large
    log-strain L with the cell C0 expm(L)^T a 10 % strain of the springs' rest cell that has nothing to do with L: there the
    exact cell force points away from the naive one (cosine 0.5).  Every L is laid inside its structure's mask."""
    out = []
    for s, n in enumerate(NS):
        m = voigt_mask(masks[s])
        if s == 1:
            rng = np.random.default_rng(3)
            lat_t, frac_t, _ = make_crystal(2, 803)
            A = rng.normal(size=(3, 3))
            L = np.where(m == 1, 0.6 * (A + A.T), 0.0)
            C0 = lat_t @ sym_strain(rng, 0.1) @ np.linalg.inv(expm(L)).T
            pos0 = frac_t @ C0
        else:
            lat_t, frac_t, C0, pos0 = _case(40 + s, n, 0.04)
            rng = np.random.default_rng(50 + s)
            A = rng.normal(0.0, 0.05, (3, 3))
            L = np.where(m == 1, (A + A.T) / 2, 0.0) if s == 2 else np.zeros((3, 3))
        out.append((C0, np.vstack([pos0, n * L]), springs_efs(*spring_list(lat_t, frac_t))))
    return out


OPTION_RUNS = {
    "fixed": dict(fixed=FIXED),
    "mask": dict(mask=[SLAB, SLAB, DIAG]),
    "pressure": dict(scalar_pressure=[0.01, 0.02, -0.005]),
    "hydrostatic": dict(hydrostatic_strain=True),
    "constant_volume": dict(constant_volume=True),
    "all": dict(fixed=FIXED, mask=[SLAB, SLAB, DIAG], scalar_pressure=[0.01, 0.02, -0.005], hydrostatic_strain=True,
                constant_volume=True),
}


def _filters(cases, opts):
    B = len(cases)
    per = lambda key, default: opts.get(key, [default] * B)  # noqa: E731
    return [ConstrainedFilterRef(cases[s][0], NS[s], mask=per("mask", None)[s], fixed=per("fixed", None)[s],
                                 scalar_pressure=per("scalar_pressure", 0.0)[s],
                                 hydrostatic_strain=opts.get("hydrostatic_strain", False),
                                 constant_volume=opts.get("constant_volume", False)) for s in range(B)]


@pytest.mark.parametrize("name", list(OPTION_RUNS))
def test_kernel_matches_the_restatement_step_by_step(name):
    """hydrostatic_strain makes the virial a multiple of I (times a block mask), which commutes with L: the exact force is
    then the naive one whatever L is, so the runs with it stay on the naive branch; every other run takes both."""
    lib = _lib.load()
    opts = OPTION_RUNS[name]
    B = len(NS)
    masks = opts.get("mask", [np.ones((3, 3))] * B)
    cases = kernel_cases(masks)
    filts = _filters(cases, opts)
    X0 = [c[1] for c in cases]
    refs = [FireRef(X, **DEFAULTS) for X in X0]
    ptr = np.concatenate([[0], np.cumsum(NS)]).astype(np.int32)
    N = int(ptr[-1])
    cells = [f.atoms(X) for f, X in zip(filts, X0)]
    C0s = np.stack([c[0] for c in cases])
    xa0 = np.concatenate([X[:n] for X, n in zip(X0, NS)])
    fr0 = np.concatenate([X[:n] @ np.linalg.inv(c[0]) for X, n, c in zip(X0, NS, cases)])
    fr0 = fr0 - np.floor(fr0)
    S = dict(lat0=_t(C0s), inv0=_t(np.linalg.inv(C0s)), xa=_t(xa0), pos=_t(np.concatenate([c[1] for c in cells])),
             vel=torch.zeros(N, 3, dtype=torch.float64, device=DEV), frac=_t(fr0),
             xc=_t(np.stack([X[n:] for X, n in zip(X0, NS)])), cvel=torch.zeros(B, 3, 3, dtype=torch.float64, device=DEV),
             defgrad=_t(np.stack([c[2] for c in cells])), lat=_t(np.stack([c[0] for c in cells])),
             F=torch.zeros(N, 3, dtype=torch.float64, device=DEV), E=torch.zeros(B, dtype=torch.float64, device=DEV),
             H=torch.zeros(B, dtype=torch.float64, device=DEV), stress=torch.zeros(B, 3, 3, dtype=torch.float64, device=DEV),
             state=_t([[DEFAULTS["dt"], DEFAULTS["a"]]] * B), istate=torch.zeros(B, 2, dtype=torch.int32, device=DEV),
             fmax=torch.zeros(B, dtype=torch.float64, device=DEV), status=torch.empty(1 + B, dtype=torch.int32, device=DEV))
    fixed_all = np.concatenate(opts.get("fixed", [np.zeros(n, dtype=bool) for n in NS]))
    fixed_t = _t(fixed_all.astype(np.uint8), torch.uint8) if "fixed" in opts else None
    mask_t = _t(np.stack([voigt_mask(m) for m in masks])) if "mask" in opts else None
    press_t = _t(opts["scalar_pressure"]) if "scalar_pressure" in opts else None
    xc_start = S["xc"].cpu().numpy().copy()
    # the components of X_c that never move: the masked ones - but constant_volume comes after the mask in ASE's order and
    # hands every diagonal component, masked or not, its share of the trace: with it only the masked off-diagonal ones stay
    held = [(voigt_mask(m) == 0) & ~(np.eye(3, dtype=bool) & bool(opts.get("constant_volume"))) for m in masks]
    p, fmax, steps = DEFAULTS, 1e-12, 12
    active = torch.arange(B, dtype=torch.int32, device=DEV)
    ptr_t = _t(ptr, torch.int32)
    branches = []
    for t in range(steps + 1):
        fs, ss, es = [], [], []
        for s in range(B):
            C, pos, _ = filts[s].atoms(refs[s].r)
            e, f, st = cases[s][2](C, pos)
            es.append(e)
            fs.append(f)
            ss.append(st)
        forces, energy, stress = _t(np.concatenate(fs)), _t(es), _t(np.stack(ss))
        args = _lib.FireArgs(
            forces=forces.data_ptr(), energy=energy.data_ptr(), stress=stress.data_ptr(), force_ptr=ptr_t.data_ptr(),
            active=active.data_ptr(), atom_ptr=ptr_t.data_ptr(), inv_lattice=S["inv0"].data_ptr(), lattice0=S["lat0"].data_ptr(),
            positions=S["pos"].data_ptr(), velocities=S["vel"].data_ptr(), frac=S["frac"].data_ptr(),
            state=S["state"].data_ptr(), istate=S["istate"].data_ptr(), xa=S["xa"].data_ptr(), xc=S["xc"].data_ptr(),
            cell_velocities=S["cvel"].data_ptr(), defgrad=S["defgrad"].data_ptr(), lattice=S["lat"].data_ptr(),
            forces_out=S["F"].data_ptr(), energy_out=S["E"].data_ptr(), fmax_out=S["fmax"].data_ptr(),
            stress_out=S["stress"].data_ptr(), status=S["status"].data_ptr(), n_active=B, steps=steps, nmin=p["Nmin"],
            fmax=fmax, maxstep=p["maxstep"], dtmax=p["dtmax"], finc=p["finc"], fdec=p["fdec"], astart=p["astart"], fa=p["fa"],
            fixed=_lib.ptr(fixed_t), cell_mask=_lib.ptr(mask_t), scalar_pressure=_lib.ptr(press_t),
            hydrostatic_strain=int(opts.get("hydrostatic_strain", False)), constant_volume=int(opts.get("constant_volume", False)),
            enthalpy_out=S["H"].data_ptr())
        _lib.check(lib.alignn_fire_step(ctypes.byref(args), _lib.stream()), "fire_step")
        st = S["status"].cpu().numpy()
        want = [0 if t < steps else 2] * B
        assert st[1:].tolist() == want and st[0] == want.count(0), (t, st)
        for s, n in enumerate(NS):
            o, filt = refs[s], filts[s]
            g = filt.forces(o.r, fs[s], ss[s])
            branches.append(filt.branch)
            assert S["fmax"][s].item() == pytest.approx(np.sqrt((g ** 2).sum(1).max()), rel=1e-12), (t, s)
            np.testing.assert_array_equal(S["F"][ptr[s]:ptr[s + 1]].cpu().numpy(), fs[s])  # the force as evaluated
            assert S["E"][s].item() == es[s]
            assert S["H"][s].item() == pytest.approx(filt.enthalpy(o.r, es[s]), rel=1e-12, abs=1e-12), (t, s)
            if t < steps:
                o.step(g)
        for s, n in enumerate(NS):
            o, filt = refs[s], filts[s]
            a, b = ptr[s], ptr[s + 1]
            C, pos, F = filt.atoms(o.r)
            assert _close(S["xa"][a:b].cpu().numpy(), o.r[:n]), (t, s)
            assert _close(S["xc"][s].cpu().numpy(), o.r[n:]), (t, s)
            assert _close(S["pos"][a:b].cpu().numpy(), pos), (t, s)
            assert _close(S["lat"][s].cpu().numpy(), C), (t, s)
            assert _close(S["defgrad"][s].cpu().numpy(), F), (t, s)
            assert _close(S["vel"][a:b].cpu().numpy(), o.v[:n]), (t, s)
            assert _close(S["cvel"][s].cpu().numpy(), o.v[n:]), (t, s)
            dt, aa = S["state"][s].tolist()
            nst, taken = S["istate"][s].tolist()
            assert dt == pytest.approx(o.dt, rel=1e-12) and aa == pytest.approx(o.a, rel=1e-12) and nst == o.Nsteps, (t, s)
            assert taken == min(t + 1, steps)
            fr = S["frac"][a:b].cpu().numpy()
            assert (fr >= 0.0).all() and (fr < 1.0).all()
            d = fr - o.r[:n] @ np.linalg.inv(cases[s][0])
            assert np.abs(d - np.round(d)).max() < 1e-9
        # what is held is held exactly: the fixed atoms' rows X_a (and their frac), the masked components of X_c
        xa, fr, xc = S["xa"].cpu().numpy(), S["frac"].cpu().numpy(), S["xc"].cpu().numpy()
        assert xa[fixed_all].tobytes() == xa0[fixed_all].tobytes() and fr[fixed_all].tobytes() == fr0[fixed_all].tobytes()
        assert not S["vel"].cpu().numpy()[fixed_all].any()
        for s in range(B):
            assert np.array_equal(xc[s][held[s]], xc_start[s][held[s]]), (t, s)
    assert np.abs(S["xc"].cpu().numpy() - xc_start).max() > 1e-3  # (the cells did move)
    print(name, "cell-force branches:", {b: branches.count(b) for b in set(branches)})
    assert set(branches) == ({"naive"} if opts.get("hydrostatic_strain") else {"naive", "exact"})


# --- (2) the relaxer on spring crystals --------------------------------------------------------------------------------------
def _spring_cases():
    cases = []
    for i, n in enumerate(NS):
        lat_t, frac_t, C0, pos0 = _case(SPRING_SEEDS[i], n, 0.03)
        cases.append((lat_t, frac_t, C0, pos0, spring_list(lat_t, frac_t, nnb=14)))
    return cases


SPRING_SEEDS = [20, 21, 26]  # (seeds whose float64 restatement converges within the cap under every option set below)
RELAX_RUNS = {
    "pressure": dict(scalar_pressure=[0.01, 0.0, 0.004]),
    "hydrostatic": dict(hydrostatic_strain=True),
    "constant_volume": dict(constant_volume=True),
    "slab": dict(fixed=FIXED, cell_mask=[SLAB, np.ones((3, 3)), SLAB], scalar_pressure=0.005),
}


def _ref_options(kw, s):
    o = dict(hydrostatic_strain=kw.get("hydrostatic_strain", False), constant_volume=kw.get("constant_volume", False))
    if "fixed" in kw:
        o["fixed"] = kw["fixed"][s]
    if "cell_mask" in kw:
        o["mask"] = kw["cell_mask"][s]
    o["scalar_pressure"] = float(np.broadcast_to(kw.get("scalar_pressure", 0.0), (len(NS),))[s])
    return o


@pytest.mark.parametrize("name", list(RELAX_RUNS))
def test_relax_springs_match_the_restatement_alone_or_batched(name):
    kw = RELAX_RUNS[name]
    cases = _spring_cases()
    fmax, steps = 1e-6, 4000
    fn = springs_torch(cases)
    res = relax(None, [c[2] for c in cases], [c[3] for c in cases], fmax=fmax, steps=steps, forces_fn=fn, device=DEV,
                optimize_lattice=True, **kw)
    assert res.converged.all().item()
    for s, (lat_t, frac_t, C0, pos0, sl) in enumerate(cases):
        opt = _ref_options(kw, s)
        ref = run_constrained_ref(C0, pos0, springs_efs(*sl), fmax=fmax, steps=steps, **opt)
        assert ref["converged"] and ref["n_steps"] > 5, s
        got_p, got_c = res.positions[s].cpu().numpy(), res.lattices[s].cpu().numpy()
        scale = np.abs(ref["C"]).max()
        np.testing.assert_allclose(got_c, ref["C"], rtol=0, atol=1e-4 * scale)
        np.testing.assert_allclose(got_p, ref["pos"], rtol=0, atol=1e-4 * scale)
        assert res.energies[s].item() == pytest.approx(ref["e"], rel=1e-6, abs=1e-12)
        assert res.fmax[s].item() < fmax
        V = abs(np.linalg.det(got_c))
        assert res.enthalpies[s].item() == pytest.approx(res.energies[s].item() + opt["scalar_pressure"] * V, rel=1e-12, abs=1e-12)
        assert res.enthalpies[s].item() == pytest.approx(ref["h"], rel=1e-6, abs=1e-12)
        # alone: the same bits
        one = {k: ([v[s]] if isinstance(v, list) else v) for k, v in kw.items()}
        alone = relax(None, [C0], [pos0], fmax=fmax, steps=steps, forces_fn=fn, device=DEV, optimize_lattice=True, **one)
        assert torch.equal(alone.positions[0], res.positions[s]) and torch.equal(alone.lattices[0], res.lattices[s])
        assert torch.equal(alone.enthalpies[0], res.enthalpies[s]) and alone.n_steps.item() == res.n_steps[s].item()
        assert torch.equal(alone.fmax[0], res.fmax[s]) and torch.equal(alone.forces[0], res.forces[s])
    # the physics of the option at the end point
    c_end = res.lattices.cpu().numpy()
    for s, c in enumerate(cases):
        V0, V = abs(np.linalg.det(c[2])), abs(np.linalg.det(c_end[s]))
        if name == "constant_volume":
            assert abs(V - V0) <= 1e-12 * V0
        if name == "hydrostatic":
            assert np.abs(c_end[s] - (V / V0) ** (1 / 3) * c[2]).max() <= 1e-12 * np.abs(c[2]).max()
        if name == "pressure":
            p = kw["scalar_pressure"][s]
            assert abs(-np.trace(res.stresses[s].cpu().numpy()) / 3 - p) <= fmax * NS[s] / V
        if name == "slab":
            fx = FIXED[s]
            if voigt_mask(kw["cell_mask"][s])[2, 2] == 0:  # the frozen axis: no cell vector changes its z component
                assert np.array_equal(c_end[s][:, 2], c[2][:, 2])
            xa = res.positions[s].cpu().numpy() @ np.linalg.inv(c_end[s]) @ c[2]  # back to the starting cell: X_a
            assert np.abs(xa[fx] - c[3][fx]).max(initial=0.0) <= 1e-12 * np.abs(c[2]).max()


# --- (3) options passed but off ----------------------------------------------------------------------------------------------
def _same(a, b):
    ok = all(torch.equal(x, y) for x, y in zip(a.positions + a.forces, b.positions + b.forces))
    ok = ok and torch.equal(a.energies, b.energies) and torch.equal(a.fmax, b.fmax) and torch.equal(a.n_steps, b.n_steps)
    if a.lattices is not None:
        ok = ok and torch.equal(a.lattices, b.lattices) and torch.equal(a.stresses, b.stresses)
    return ok and torch.equal(a.converged, b.converged) and a.n_evals == b.n_evals


def test_options_that_are_off_take_the_old_path():
    cases = _spring_cases()
    fn = springs_torch(cases)
    lats, pos = [c[2] for c in cases], [c[3] for c in cases]
    off = dict(fixed=[np.zeros(n, dtype=bool) for n in NS], hydrostatic_strain=False, constant_volume=False)
    plain = relax(None, lats, pos, fmax=1e-3, steps=40, forces_fn=fn, device=DEV, optimize_lattice=True)
    same = relax(None, lats, pos, fmax=1e-3, steps=40, forces_fn=fn, device=DEV, optimize_lattice=True,
                 cell_mask=np.ones((3, 6)), scalar_pressure=[0.0, 0.0, 0.0], **off)
    assert plain.n_steps.max().item() == 40 and _same(plain, same)
    assert torch.equal(same.enthalpies, same.energies) and plain.enthalpies is not None
    fn2 = lambda l, p: fn(l, p)[:2]  # noqa: E731
    plain = relax(None, lats, pos, fmax=1e-3, steps=40, forces_fn=fn2, device=DEV)
    same = relax(None, lats, pos, fmax=1e-3, steps=40, forces_fn=fn2, device=DEV, scalar_pressure=0.0, **off)
    assert plain.n_steps.max().item() == 40 and _same(plain, same) and same.enthalpies is None and same.lattices is None


# --- (4) a fixed atom at fixed cell ------------------------------------------------------------------------------------------
def test_fixed_atoms_at_fixed_cell_stay_where_they_are():
    cases = _spring_cases()
    fn = springs_torch(cases)
    fn2 = lambda l, p: fn(l, p)[:2]  # noqa: E731
    lats, pos = [c[2] for c in cases], [c[3] for c in cases]
    # the 1-atom structure: everything held, converged at step 0; the 7-atom one: two atoms held, against each other too
    fixed = [np.array([True]), FIXED[1], TWO_FIXED]
    fmax = 1e-6
    # the forces of a spring crystal add up to zero, so one held atom's force goes to zero with the free atoms' as the run
    # converges: a short run shows it against the restatement, and the converged one where two atoms are held
    for steps in (6, 4000):
        res = relax(None, lats, pos, fmax=fmax, steps=steps, forces_fn=fn2, device=DEV, fixed=fixed)
        assert res.n_steps[0].item() == 0 and res.converged[0].item() and res.n_evals == res.n_steps.max().item() + 1
        assert res.converged.tolist() == [True, steps > 6, steps > 6] and res.enthalpies is None
        for s, c in enumerate(cases):
            fx = fixed[s]
            ef = springs_efs(*c[4])
            ref = run_fixed_ref(c[3], lambda r: ef(c[2], r)[:2], fx, fmax=fmax, steps=steps)
            assert ref["converged"] == res.converged[s].item()
            got = res.positions[s].cpu().numpy()
            assert got[fx].tobytes() == np.asarray(c[3])[fx].tobytes()  # the input's bits
            np.testing.assert_allclose(got, ref["r"], rtol=0, atol=1e-4 * np.abs(c[2]).max())
            f = res.forces[s].cpu().numpy()
            free = np.sqrt((f[~fx] ** 2).sum(1)).max(initial=0.0)
            assert res.fmax[s].item() == pytest.approx(free, rel=1e-12, abs=1e-300)  # fmax does not see the held rows
            np.testing.assert_allclose(f, ref["f"], rtol=0, atol=1e-6)
            if steps == 6:
                assert res.n_steps[s].item() == ref["n_steps"] == (0 if s == 0 else 6)
                assert _close(got, ref["r"], 1e-9) and _close(f, ref["f"], 1e-9)
            else:
                assert free < fmax
            if s > 0 and (steps == 6 or s == 2):  # held against a force: the result keeps it
                assert np.sqrt((f[fx] ** 2).sum(1)).min() > 1e3 * fmax
    # the kernel itself: a fixed atom's position and frac are not written (a sentinel survives), its velocity stays zero
    lib = _lib.load()
    n = 7
    rng = np.random.default_rng(5)
    x0 = rng.normal(0.0, 2.0, (n, 3))
    fx = FIXED[2]
    S = dict(pos=_t(x0), vel=torch.zeros(n, 3, dtype=torch.float64, device=DEV), frac=_t(np.full((n, 3), -7.0)),
             inv=_t(np.linalg.inv(cases[2][2])[None]), state=_t([[DEFAULTS["dt"], DEFAULTS["a"]]]),
             istate=torch.zeros(1, 2, dtype=torch.int32, device=DEV), F=torch.zeros(n, 3, dtype=torch.float64, device=DEV),
             E=torch.zeros(1, dtype=torch.float64, device=DEV), fmax=torch.zeros(1, dtype=torch.float64, device=DEV),
             status=torch.empty(2, dtype=torch.int32, device=DEV))
    ptr_t, act, fixed_t = _t([0, n], torch.int32), _t([0], torch.int32), _t(fx.astype(np.uint8), torch.uint8)
    ref, p = FireRef(x0, **DEFAULTS), DEFAULTS
    for t in range(4):
        f = rng.normal(0.0, 1.0, (n, 3))
        forces, energy = _t(f), _t([0.5])
        args = _lib.FireArgs(forces=forces.data_ptr(), energy=energy.data_ptr(), force_ptr=ptr_t.data_ptr(), active=act.data_ptr(),
                             atom_ptr=ptr_t.data_ptr(), inv_lattice=S["inv"].data_ptr(), positions=S["pos"].data_ptr(),
                             velocities=S["vel"].data_ptr(), frac=S["frac"].data_ptr(), state=S["state"].data_ptr(),
                             istate=S["istate"].data_ptr(), forces_out=S["F"].data_ptr(), energy_out=S["E"].data_ptr(),
                             fmax_out=S["fmax"].data_ptr(), status=S["status"].data_ptr(), n_active=1, steps=10, nmin=p["Nmin"],
                             fmax=1e-12, maxstep=p["maxstep"], dtmax=p["dtmax"], finc=p["finc"], fdec=p["fdec"],
                             astart=p["astart"], fa=p["fa"], fixed=fixed_t.data_ptr())
        _lib.check(lib.alignn_fire_step(ctypes.byref(args), _lib.stream()), "fire_step")
        g = f.copy()
        g[fx] = 0.0
        ref.step(g)
        assert S["fmax"].item() == pytest.approx(np.sqrt((g ** 2).sum(1).max()), rel=1e-12)
        np.testing.assert_array_equal(S["F"].cpu().numpy(), f)
        got, fr = S["pos"].cpu().numpy(), S["frac"].cpu().numpy()
        assert _close(got, ref.r) and _close(S["vel"].cpu().numpy(), ref.v)
        assert got[fx].tobytes() == x0[fx].tobytes() and (fr[fx] == -7.0).all() and not S["vel"].cpu().numpy()[fx].any()
        assert (fr[~fx] >= 0.0).all() and (fr[~fx] < 1.0).all()
    # the filter's options without the filter's state are refused
    args.constant_volume = 1
    assert lib.alignn_fire_step(ctypes.byref(args), _lib.stream()) != 0


# --- (5) with the model ------------------------------------------------------------------------------------------------------
def _host_loop(model, lats, pos, feats, fmax, steps, options):
    """test_gpu_relax_cell._host_loop with the constrained filter: model(crystal_batch) on the device, the calculator's rules,
    the filter and FIRE as the numpy restatement (sim_gpu.host_relax_loop)."""
    filts = [ConstrainedFilterRef(l, len(p), **o) for l, p, o in zip(lats, pos, options)]
    opts, energy, taken, _ = host_relax_loop(model, lats, pos, feats, fmax, steps, filts)
    res = [f.atoms(o.r) for f, o in zip(filts, opts)]
    return [r[1] for r in res], [r[0] for r in res], taken, [f.enthalpy(o.r, e) for f, o, e in zip(filts, opts, energy)]


def test_relax_model_with_constraints_matches_a_host_loop():
    model = _model()
    lats, pos, feats = _crystals(1)
    n = len(pos[0])
    fixed = np.zeros(n, dtype=bool)
    fixed[:6] = True
    p = 0.05
    kw = dict(fixed=[fixed], cell_mask=SLAB, scalar_pressure=p)
    res = relax(model, lats, pos, feats, fmax=0.0, steps=10, optimize_lattice=True, **kw)
    p_host, c_host, taken, h_host = _host_loop(model, lats, pos, feats, 0.0, 10, [dict(fixed=fixed, mask=SLAB, scalar_pressure=p)])
    assert res.n_steps.tolist() == taken == [10] and res.n_evals == 11
    lat0 = np.asarray(lats[0], dtype=np.float64)
    got_p, got_c = res.positions[0].cpu().numpy(), res.lattices[0].cpu().numpy()
    dpos, dlat = np.abs(got_p - p_host[0]).max(), np.abs(got_c - c_host[0]).max()
    moved = np.abs(c_host[0] - lat0).max()
    print(f"relax(fixed, cell_mask, scalar_pressure) vs host loop after 10 steps: max |dpos| {dpos:.3e} A, max |dlat| "
          f"{dlat:.3e} A (cell moved {moved:.3e} A)")
    assert moved > 1e-3
    # the tolerance of test_gpu_relax_cell.test_relax_cell_model_matches_a_host_loop
    assert dpos <= 3 * 1.8e-15 and dlat <= 3 * 1.8e-15, (dpos, dlat)
    assert np.array_equal(got_c[:, 2], lat0[:, 2])  # the frozen axis
    xa = got_p @ np.linalg.inv(got_c) @ lat0
    assert np.abs(xa[fixed] - np.asarray(pos[0], dtype=np.float64)[fixed]).max() <= 1e-12 * np.abs(lat0).max()
    V = abs(np.linalg.det(got_c))
    assert res.enthalpies[0].item() == pytest.approx(res.energies[0].item() + p * V, rel=1e-12)
    assert res.enthalpies[0].item() == pytest.approx(h_host[0], rel=1e-6)
    f = res.forces[0].cpu().numpy()
    assert np.abs(f[fixed]).max() > 0.0  # the forces as evaluated
    again = relax(model, lats, pos, feats, fmax=0.0, steps=10, optimize_lattice=True, **kw)
    assert all(torch.equal(x, y) for x, y in zip(res.positions + res.forces, again.positions + again.forces))
    assert torch.equal(res.lattices, again.lattices) and torch.equal(res.enthalpies, again.enthalpies)
    assert torch.equal(res.fmax, again.fmax) and torch.equal(res.energies, again.energies)
