"""Batched MD on the device (csrc/dynamics.hip, alignn_amd/dynamics.py) against the float64 restatement of ASE's integrators in
md_ref.py: (1) the kernel alone, step by step, for the three ensembles, the exported random numbers against the numpy
stream; (2) NVE on periodic spring crystals: second-order energy error, time reversal; (3) the Langevin and Berendsen
thermostats and the Maxwell-Boltzmann start; (4) a structure alone vs. in a batch, bit for bit; (5) run_md with an
ALIGNNAtomWise against a host loop over the same model; (6) replay and run-to-run bit identity."""

import ctypes

import numpy as np
import pytest
import torch

from alignn_amd import _lib
from alignn_amd.dynamics import ENSEMBLES, FS, KB, berendsen_taut, run_md
from alignn_amd.synthetic import make_crystal
from tests.md_ref import (BerendsenRef, LangevinRef, VerletRef, kinetic_energy, maxwell_boltzmann, normals, stream_words,
                          temperature)
from tests.sim_gpu import DEV, _md_crystals as _crystals, _model, _rel, _second_half_mean, _spring_crystals, _t, host_md_loop

pytestmark = pytest.mark.gpu


# --- (1) the kernel against the restatement, step by step -----------------------------------------------------------------
@pytest.mark.parametrize("ensemble", ["nve", "nvt_langevin", "nvt_berendsen"])
def test_kernel_matches_the_restatement_step_by_step(ensemble):
    lib = _lib.load()
    rng = np.random.default_rng(11)
    ns = [1, 5, 60, 300]
    B, N = len(ns), sum(ns)
    ptr = np.concatenate([[0], np.cumsum(ns)]).astype(np.int32)
    lats = [make_crystal(max(n, 2), 70 + i)[0] for i, n in enumerate(ns)]
    ms = [rng.uniform(1.0, 200.0, n) for n in ns]
    r0 = [rng.normal(0.0, 3.0, (n, 3)) for n in ns]
    p0 = [rng.normal(0.0, 1.0, (n, 3)) * np.sqrt(m * KB * 300.0)[:, None] for n, m in zip(ns, ms)]
    p0[0][:] = 0.0  # T = 0 at the first Berendsen scaling: the factor is 1.1, no NaN
    t0 = [150.0, 300.0, 600.0, 1200.0]
    seeds = [3, 2 ** 40 + 7, 2 ** 63 + 5, 0xFFFFFFFFFFFFFFFF]
    dt, fr, fixcm = 1.0 * FS, 0.05, True
    taut = dt if ensemble == "nvt_berendsen" else 100 * dt  # taut = dt: the scaling clips for most T0 / T
    steps, interval = 6, 2
    ens = ENSEMBLES[ensemble]
    nf = steps // interval + 1
    S = dict(ptr=_t(ptr, torch.int32), m=_t(np.concatenate(ms)), inv=torch.linalg.inv(_t(np.stack(lats))).contiguous(),
             p=_t(np.concatenate(p0)), r=_t(np.concatenate(r0)), frac=torch.full((N, 3), -1.0, dtype=torch.float64, device=DEV),
             v=torch.zeros(N, 3, dtype=torch.float64, device=DEV), rv=torch.zeros(N, 3, dtype=torch.float64, device=DEV),
             t0=_t(t0), seed=_t([s - 2 ** 64 if s >= 2 ** 63 else s for s in seeds], torch.int64),
             epot=torch.zeros(nf, B, dtype=torch.float64, device=DEV), ekin=torch.zeros(nf, B, dtype=torch.float64, device=DEV),
             temp=torch.zeros(nf, B, dtype=torch.float64, device=DEV), tp=torch.zeros(nf, N, 3, dtype=torch.float64, device=DEV),
             tm=torch.zeros(nf, N, 3, dtype=torch.float64, device=DEV), status=torch.zeros(1, dtype=torch.int32, device=DEV))
    noise = torch.full((N, 18), np.nan, dtype=torch.float64, device=DEV)
    if ensemble == "nve":
        refs = [VerletRef(r0[s], p0[s], ms[s], dt) for s in range(B)]
    elif ensemble == "nvt_berendsen":
        refs = [BerendsenRef(r0[s], p0[s], ms[s], dt, t0[s], taut, fixcm) for s in range(B)]
    else:
        refs = [LangevinRef(r0[s], p0[s], ms[s], dt, t0[s], fr, fixcm, seeds[s]) for s in range(B)]
    args = _lib.MdArgs(
        atom_ptr=S["ptr"].data_ptr(), masses=S["m"].data_ptr(), t0_kelvin=S["t0"].data_ptr(), seeds=S["seed"].data_ptr(),
        inv_lattice=S["inv"].data_ptr(), momenta=S["p"].data_ptr(), positions=S["r"].data_ptr(), frac=S["frac"].data_ptr(),
        velocities=S["v"].data_ptr(), scratch=S["rv"].data_ptr(), status=S["status"].data_ptr(), epot=S["epot"].data_ptr(),
        ekin=S["ekin"].data_ptr(), temperature=S["temp"].data_ptr(), traj_positions=S["tp"].data_ptr(),
        traj_momenta=S["tm"].data_ptr(), noise_out=noise.data_ptr(), n_structures=B, interval=interval, steps=steps,
        ensemble=ens, fixcm=int(fixcm), dt=dt, friction=fr, taut=taut, kB=KB)
    scales = set()
    for t in range(steps + 1):
        fs = [rng.normal(0.0, 1.0, (n, 3)) for n in ns]
        es = rng.normal(size=B)
        f_d, e_d = _t(np.concatenate(fs)), _t(es)
        args.forces, args.energy, args.n_rows, args.t = f_d.data_ptr(), e_d.data_ptr(), N, t
        _lib.check(lib.alignn_md_step(ctypes.byref(args), _lib.stream()), "md_step")
        nz = noise.cpu().numpy()
        for s, o in enumerate(refs):
            a, b = ptr[s], ptr[s + 1]
            if t > 0:
                o.finish(fs[s])
            if t % interval == 0:
                k = t // interval
                ke = kinetic_energy(o.p, o.m)
                assert S["epot"][k, s].item() == es[s]
                assert S["ekin"][k, s].item() == pytest.approx(ke, rel=1e-12, abs=1e-300), (t, s)
                assert S["temp"][k, s].item() == pytest.approx(temperature(o.p, o.m), rel=1e-12, abs=1e-300)
                assert _rel(S["tm"][k, a:b].cpu().numpy(), o.p) <= 1e-12 and _rel(S["tp"][k, a:b].cpu().numpy(), o.r) <= 1e-12
            if t < steps:
                if ensemble == "nvt_langevin":
                    w = stream_words(seeds[s], ns[s], t, 0, 3)
                    assert np.array_equal(nz[a:b, 6:].reshape(ns[s], 3, 4), w.astype(np.float64)), (t, s)
                    g = normals(seeds[s], ns[s], t, 0, 3)
                    assert np.abs(nz[a:b, :6] - g).max() <= 1e-14 * max(1.0, np.abs(g).max()), (t, s)
                    o.begin(fs[s], nz[a:b, 0:3], nz[a:b, 3:6])
                else:
                    if ensemble == "nvt_berendsen":
                        T = temperature(o.p, o.m)
                        scales.add("zero" if T == 0 else ("clip" if abs(np.sqrt(1 + (t0[s] / T - 1)) - 1) > 0.1 else "free"))
                    o.begin(fs[s])
        p_d, r_d = S["p"].cpu().numpy(), S["r"].cpu().numpy()
        for s, o in enumerate(refs):
            a, b = ptr[s], ptr[s + 1]
            assert _rel(p_d[a:b], o.p) <= 1e-12 and _rel(r_d[a:b], o.r) <= 1e-12, (t, s)
            if ensemble == "nvt_langevin" and t < steps:  # (v between the halves: after finish the kernel keeps only p)
                assert _rel(S["v"][a:b].cpu().numpy(), o.v) <= 1e-12, (t, s)
            if t < steps:
                fr_d = S["frac"][a:b].cpu().numpy()
                assert (fr_d >= 0.0).all() and (fr_d < 1.0).all()
                d = fr_d - o.r @ np.linalg.inv(lats[s])
                assert np.abs(d - np.round(d)).max() < 1e-9
    assert S["status"].item() == 0
    if ensemble == "nvt_berendsen":
        assert scales == {"zero", "clip", "free"}, scales
    # a force array of another row count than the batch: status -1, nothing written
    before = S["p"].clone()
    f_d, e_d = torch.zeros(N - 1, 3, dtype=torch.float64, device=DEV), _t(np.zeros(B))
    args.forces, args.energy, args.n_rows = f_d.data_ptr(), e_d.data_ptr(), N - 1
    args.traj_positions = args.traj_momenta = args.noise_out = None
    args.t, args.interval, args.steps, args.fixcm = 1, 1, 3, 1
    _lib.check(lib.alignn_md_step(ctypes.byref(args), _lib.stream()), "md_step")
    assert S["status"].item() == -1 and torch.equal(S["p"], before)


def test_initial_momenta_match_the_restatement():
    ns = [1, 7, 300]
    ms = [np.random.default_rng(n).uniform(1.0, 200.0, n) for n in ns]
    seeds, tk = [5, 2 ** 33 + 1, 2 ** 64 - 2], [10.0, 300.0, 2000.0]
    lats = [np.eye(3) * 10.0] * 3
    res = run_md(None, lats, [np.zeros((n, 3)) for n in ns], None, ms, steps=0, initial_temperature_K=tk, seed=seeds,
                 forces_fn=lambda l, p: (torch.zeros(3, device=DEV), torch.zeros(sum(ns), 3, dtype=torch.float64, device=DEV)))
    for s in range(3):
        want = maxwell_boltzmann(seeds[s], ms[s], tk[s])
        assert _rel(res.momenta[s].cpu().numpy(), want) <= 1e-14


# --- periodic spring crystals (forces_fn: sim_gpu.Springs) -------------------------------------------------------------------
def test_nve_springs_second_order_energy_and_time_reversal():
    sizes = [16, 24, 32, 20]
    lats, pos, ff = _spring_crystals(sizes, 300)
    ms = [np.full(n, 28.0) for n in sizes]
    a = run_md(None, lats, pos, None, ms, timestep=1.0, steps=2000, initial_temperature_K=300.0, seed=[1, 2, 3, 4],
               trajectory=False, forces_fn=ff, device=DEV)
    b = run_md(None, lats, pos, None, ms, timestep=0.5, steps=4000, interval=2, initial_temperature_K=300.0, seed=[1, 2, 3, 4],
               trajectory=False, forces_fn=ff, device=DEV)
    ea, eb = (a.epot + a.ekin).cpu().numpy(), (b.epot + b.ekin).cpu().numpy()
    ke = a.ekin.mean(0).cpu().numpy()
    spread_a, spread_b = ea.max(0) - ea.min(0), eb.max(0) - eb.min(0)
    drift = np.abs(ea - ea[0]).max(0)
    print("NVE springs: spread / <KE> at 1 fs", spread_a / ke, "ratio 1 fs / 0.5 fs", spread_a / spread_b)
    assert a.n_evals == 2001 and a.epot.shape == (2001, 4) and b.epot.shape == (2001, 4)
    assert (drift < 5e-3 * ke).all(), drift / ke
    assert ((spread_a / spread_b > 3.0) & (spread_a / spread_b < 5.0)).all(), spread_a / spread_b
    # flip the momenta and run the same steps back: the start again
    back = run_md(None, lats, a.positions, None, ms, timestep=1.0, steps=2000, momenta=[-p for p in a.momenta],
                  trajectory=False, forces_fn=ff, device=DEV)
    p_start = run_md(None, lats, pos, None, ms, steps=0, initial_temperature_K=300.0, seed=[1, 2, 3, 4], forces_fn=ff,
                     device=DEV).momenta
    for s in range(4):
        moved = np.abs(a.positions[s].cpu().numpy() - pos[s]).max()
        err_r = np.abs(back.positions[s].cpu().numpy() - pos[s]).max()
        err_p = np.abs(back.momenta[s].cpu().numpy() + p_start[s].cpu().numpy()).max()
        print(f"time reversal {s}: moved {moved:.3e} A, back to {err_r:.3e} A, momenta {err_p:.3e}")
        assert moved > 0.05 and err_r < 1e-9 and err_p < 1e-9 * np.abs(p_start[s].cpu().numpy()).max()


def test_thermostats_reach_their_temperature_ladder():
    sizes = [64, 64, 64, 64]
    lats, pos, ff = _spring_crystals(sizes, 600)
    ms = [np.random.default_rng(s).uniform(10.0, 60.0, n) for s, n in enumerate(sizes)]
    ladder = np.array([100.0, 300.0, 600.0, 1200.0])
    # Langevin from rest.  fixcm takes the centre-of-mass momentum out of the thermalised degrees of freedom: <T> over 3N is
    # T0 (N - 1) / N.  Instantaneous T has a relative spread of sqrt(2 / 3N) = 0.10; the friction (0.05 / ASE time unit,
    # ~200 steps) and the spring periods (~100-200 steps) leave >= 10 independent samples in the 2000 steps averaged, so the
    # standard error is <= 0.032 of T0; the bound 0.12 is ~4 of them.
    lv = run_md(None, lats, pos, None, ms, ensemble="nvt_langevin", timestep=1.0, steps=4000, interval=4, temperature_K=ladder,
                friction=0.05, seed=[7, 8, 9, 10], trajectory=False, forces_fn=ff, device=DEV)
    got = _second_half_mean(lv)
    want = ladder * (1 - 1 / np.array(sizes))
    print("Langevin <T> / T0(N-1)/N:", got / want)
    assert (np.abs(got / want - 1.0) < 0.12).all(), got / want
    # Berendsen from a Maxwell-Boltzmann start at half the target: scaling drives the measured T (3N) itself to T0; its
    # fluctuations are smaller than canonical ones, the same bound holds
    bd = run_md(None, lats, pos, None, ms, ensemble="nvt_berendsen", timestep=1.0, steps=4000, interval=4, temperature_K=ladder,
                initial_temperature_K=ladder / 2, seed=[1, 2, 3, 4], trajectory=False, forces_fn=ff, device=DEV)
    got = _second_half_mean(bd)
    print("Berendsen <T> / T0:", got / ladder)
    assert (np.abs(got / ladder - 1.0) < 0.12).all(), got / ladder


def test_maxwell_boltzmann_kinetic_energy():
    ns = [25000] * 4
    ms = [np.random.default_rng(s).uniform(1.0, 200.0, n) for s, n in enumerate(ns)]
    tk = np.array([50.0, 300.0, 1000.0, 3000.0])
    N = sum(ns)
    res = run_md(None, [np.eye(3) * 60.0] * 4, [np.zeros((n, 3)) for n in ns], None, ms, steps=0, initial_temperature_K=tk,
                 seed=[100, 101, 102, 103], trajectory=False,
                 forces_fn=lambda l, p: (torch.zeros(4, device=DEV), torch.zeros(N, 3, dtype=torch.float64, device=DEV)),
                 device=DEV)
    ke = res.ekin[0].cpu().numpy()
    want = 1.5 * np.array(ns) * KB * tk
    se = np.sqrt(1.5 * np.array(ns)) * KB * tk  # KE / kT is Gamma(3N / 2): variance 3N / 2
    print("MB KE / (3/2 N kB T) - 1:", ke / want - 1, "in standard errors:", (ke - want) / se)
    assert (np.abs(ke - want) < 5 * se).all()
    assert res.temperature[0].cpu().numpy() == pytest.approx(2 * ke / (3 * np.array(ns) * KB), rel=1e-15)


# --- (4) alone vs. batched --------------------------------------------------------------------------------------------------
def test_langevin_structure_alone_equals_its_slice_of_the_batch():
    sizes = [5, 16, 33, 12]
    lats, pos, ff = _spring_crystals(sizes, 900)
    ms = [np.random.default_rng(s).uniform(1.0, 100.0, n) for s, n in enumerate(sizes)]
    seeds, t0 = [11, 22, 2 ** 63 + 33, 44], [200.0, 400.0, 800.0, 1600.0]
    kw = dict(ensemble="nvt_langevin", timestep=2.0, steps=60, interval=3, friction=0.02, device=DEV)
    both = run_md(None, lats, pos, None, ms, temperature_K=t0, initial_temperature_K=t0, seed=seeds, forces_fn=ff, **kw)
    ptr = np.concatenate([[0], np.cumsum(sizes)])
    for s in range(4):
        one = run_md(None, lats[s:s + 1], pos[s:s + 1], None, ms[s:s + 1], temperature_K=t0[s], initial_temperature_K=t0[s],
                     seed=seeds[s], forces_fn=ff.subset([s]), **kw)
        a, b = ptr[s], ptr[s + 1]
        assert torch.equal(one.traj_positions[:, :, :], both.traj_positions[:, a:b]), s
        assert torch.equal(one.traj_momenta, both.traj_momenta[:, a:b]), s
        for k in ("epot", "ekin", "temperature"):
            assert torch.equal(getattr(one, k)[:, 0], getattr(both, k)[:, s]), (s, k)
        assert torch.equal(one.positions[0], both.positions[s]) and torch.equal(one.momenta[0], both.momenta[s])
    assert both.traj_positions.shape == (21, sum(sizes), 3)
    assert (both.traj_momenta[-1] != both.traj_momenta[0]).any()


# --- (5), (6) a random-initialised ALIGNNAtomWise -------------------------------------------------------------------------
def _host_loop(model, lats, pos, feats, ms, ensemble, steps, dt, t0, fr, seeds, t_init):
    """The reference's loop, batched by hand (sim_gpu.host_md_loop): model(crystal_batch(...)) on the device, the integrators as
    the restatement."""
    B = len(pos)
    p0 = [maxwell_boltzmann(seeds[s], ms[s], t_init) for s in range(B)]
    if ensemble == "nve":
        refs = [VerletRef(pos[s], p0[s], ms[s], dt) for s in range(B)]
    else:
        refs = [LangevinRef(pos[s], p0[s], ms[s], dt, t0, fr, True, seeds[s]) for s in range(B)]
    return refs, host_md_loop(model, refs, lats, feats, steps)[0]


@pytest.mark.parametrize("ensemble", ["nve", "nvt_langevin"])
def test_run_md_model_matches_a_host_loop(ensemble):
    model = _model()
    lats, pos, feats, ms = _crystals()
    seeds, steps = [5, 6, 7, 8, 9, 10], 5
    res = run_md(model, lats, pos, feats, ms, ensemble=ensemble, timestep=2.0, steps=steps, temperature_K=500.0,
                 friction=0.05, initial_temperature_K=500.0, seed=seeds)
    refs, epot = _host_loop(model, lats, pos, feats, ms, ensemble, steps, 2.0 * FS, 500.0, 0.05, seeds, 500.0)
    assert res.n_evals == steps + 1 and res.epot.shape == (steps + 1, 6)
    dpos = max(np.abs(res.positions[s].cpu().numpy() - refs[s].r).max() for s in range(6))
    dmom = max(_rel(res.momenta[s].cpu().numpy(), refs[s].p) for s in range(6))
    de = np.abs(res.epot.cpu().numpy() - epot).max() / np.abs(epot).max()
    moved = max(np.abs(refs[s].r - pos[s]).max() for s in range(6))
    print(f"run_md {ensemble} vs host loop after {steps} steps: max |dpos| {dpos:.3e} A (atoms moved up to {moved:.3e} A), "
          f"momenta rel {dmom:.3e}, energy rel {de:.3e}")
    assert moved > 1e-3
    # measured on an MI355X: NVE max |dpos| 0.0 A, momenta rel 1.7e-16, energies bit-equal; Langevin 3.6e-15 A, 5.2e-14, bit-equal
    # (the kernel's fused multiply-adds and reduction order, and its log / cos / sin against numpy's).  Tolerances 3x the larger;
    # for the energies 3x one float32 rounding, as 3 x 0 bounds nothing.
    assert dpos <= 3 * 3.6e-15 and dmom <= 3 * 5.2e-14 and de <= 3 * 2.0 ** -24, (dpos, dmom, de)


def test_replay_gives_the_same_bits_and_runs_repeat():
    model = _model()
    lats, pos, feats, ms = _crystals(4)
    kw = dict(ensemble="nvt_langevin", timestep=2.0, steps=20, temperature_K=400.0, friction=0.05, initial_temperature_K=400.0,
              seed=[1, 2, 3, 4])
    a = run_md(model, lats, pos, feats, ms, replay=False, **kw)
    b = run_md(model, lats, pos, feats, ms, replay=True, **kw)
    c = run_md(model, lats, pos, feats, ms, replay=False, **kw)
    for x in (b, c):
        assert torch.equal(a.traj_positions, x.traj_positions) and torch.equal(a.traj_momenta, x.traj_momenta)
        assert torch.equal(a.epot, x.epot) and torch.equal(a.ekin, x.ekin)
        for u, v in zip(a.forces, x.forces):
            assert torch.equal(u, v)
    assert (a.traj_positions[-1] != a.traj_positions[0]).any()


def test_run_md_validates_its_model_inputs():
    model = _model()
    lats, pos, feats, ms = _crystals(2)
    with pytest.raises(ValueError):
        run_md(model.train(), lats, pos, feats, ms, steps=1)
    model.eval()
    with pytest.raises(ValueError):
        run_md(model, lats, pos, None, ms, steps=1)
    with pytest.raises(ValueError):
        run_md(model, lats, pos, [feats[0], feats[0]], ms, steps=1)
    with pytest.raises(ValueError):  # forces_fn returning the wrong row count
        run_md(None, lats, pos, None, ms, steps=1, device=DEV,
               forces_fn=lambda l, p: (torch.zeros(2, device=DEV), torch.zeros(3, 3, device=DEV)))
    assert berendsen_taut(None, 2.0) == 200.0 * FS
