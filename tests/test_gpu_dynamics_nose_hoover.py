"""Nose-Hoover chain NVT and isotropic MTK NPT on the device (csrc/dynamics.hip ``alignn_md_step``, ensembles 5 and 6,
alignn_amd/dynamics.py) against the float64 restatement in md_nose_hoover_ref.py: (1) the kernel alone, step by step;
(2) the limits, bit for bit; (3) the conserved quantity at second order and the drift; (4) the temperature and the pressure
ladder; (5) a structure alone vs. in a batch; (6) run_md with an ALIGNNAtomWise against a host loop; (7) replay and run-to-run
bit identity; (8) what the entry point refuses."""

import ctypes

import numpy as np
import pytest
import torch

from alignn_amd import _lib
from alignn_amd.dynamics import BAR, ENSEMBLES, FS, KB, run_md
from alignn_amd.synthetic import make_crystal
from tests.md_nose_hoover_ref import (BARO, BARO_SEED, BARO_SIZES, LADDER_BAR, MTKRef, NoseHooverChainRef, barostat_ref,
                                      barostat_residuals)
from tests.md_npt_ref import pressure_of
from tests.md_ref import kinetic_energy, maxwell_boltzmann, temperature
from tests.sim_gpu import (DEV, _md_crystals as _crystals, _model, _no_stress, _rel, _relmax, _second_half_mean, _spring_crystals,
                           _stress_springs, _t, host_md_loop)

pytestmark = pytest.mark.gpu
INVALID = 1  # hipErrorInvalidValue


def _args(S, f_d, e_d, st_d, n_rows, t, interval, steps, ens, dt, **kw):
    a = dict(forces=f_d.data_ptr(), energy=e_d.data_ptr(), stress=_lib.ptr(st_d), n_rows=n_rows, atom_ptr=S["ptr"].data_ptr(),
             masses=S["m"].data_ptr(), t0_kelvin=S["t0"].data_ptr(), pressure=S["ptarget"].data_ptr(), lattice=S["lat"].data_ptr(),
             inv_lattice=S["inv"].data_ptr(), momenta=S["p"].data_ptr(), positions=S["r"].data_ptr(), frac=S["frac"].data_ptr(),
             status=S["status"].data_ptr(), epot=S["epot"].data_ptr(), ekin=S["ekin"].data_ptr(), temperature=S["temp"].data_ptr(),
             pressure_out=S["pout"].data_ptr(), volume_out=S["vout"].data_ptr(), traj_positions=S["tp"].data_ptr(),
             traj_momenta=S["tm"].data_ptr(), traj_lattice=S["tl"].data_ptr(), n_structures=S["t0"].numel(), t=t, interval=interval,
             steps=steps, ensemble=ens, fixcm=0, dt=dt, kB=KB, nhc_state=S["nhc"].data_ptr(), conserved_out=S["cons"].data_ptr())
    a.update(kw)
    return _lib.MdArgs(**a)


def _state(ns, rng, nf):
    B, N = len(ns), sum(ns)
    ptr = np.concatenate([[0], np.cumsum(ns)]).astype(np.int32)
    lats = [make_crystal(max(n, 2), 70 + i)[0] for i, n in enumerate(ns)]
    ms = [rng.uniform(1.0, 200.0, n) for n in ns]
    r0 = [rng.normal(0.0, 3.0, (n, 3)) for n in ns]
    p0 = [rng.normal(0.0, 1.0, (n, 3)) * np.sqrt(m * KB * 300.0)[:, None] for n, m in zip(ns, ms)]
    z = lambda *sh: torch.zeros(*sh, dtype=torch.float64, device=DEV)  # noqa: E731
    S = dict(ptr=_t(ptr, torch.int32), m=_t(np.concatenate(ms)), lat=_t(np.stack(lats)),
             inv=torch.linalg.inv(_t(np.stack(lats))).contiguous(), r=_t(np.concatenate(r0)),
             frac=torch.full((N, 3), -1.0, dtype=torch.float64, device=DEV), epot=z(nf, B), ekin=z(nf, B), temp=z(nf, B),
             pout=z(nf, B), vout=z(nf, B), cons=z(nf, B), tp=z(nf, N, 3), tm=z(nf, N, 3), tl=z(nf, B, 3, 3), nhc=z(B, 34),
             status=torch.zeros(1, dtype=torch.int32, device=DEV))
    return S, ptr, lats, ms, r0, p0


# --- (1) the kernel against the restatement, step by step -----------------------------------------------------------------
CASES = [("nvt_nose_hoover", 1, 1, 1, True, False), ("nvt_nose_hoover", 3, 3, 2, True, False),
         ("npt_nose_hoover", 3, 3, 1, True, True), ("npt_nose_hoover", 1, 5, 2, True, True),
         ("npt_nose_hoover", 3, 5, 1, False, True), ("npt_nose_hoover", 2, 1, 1, True, False)]


@pytest.mark.parametrize("ensemble,chain,order,loops,thermo,baro", CASES)
def test_nose_hoover_kernel_matches_the_restatement_step_by_step(ensemble, chain, order, loops, thermo, baro):
    lib = _lib.load()
    rng = np.random.default_rng(12)
    ns = [1, 5, 60, 300]
    B, N = len(ns), sum(ns)
    steps, interval = 6, 2
    nf = steps // interval + 1
    S, ptr, lats, ms, r0, p0 = _state(ns, rng, nf)
    p0[1][:] = 0.0  # one structure starts at rest; the single atom moves (fixcm, which would stop it, is off where chain = 1)
    t0 = [150.0, 300.0, 600.0, 1200.0]
    ptarget = [-0.01, 0.0, 0.005, 0.02]  # eV/A^3
    dt = 1.0 * FS
    ttime, ptime = 20 * dt, 100 * dt
    S.update(p=_t(np.concatenate(p0)), t0=_t(t0), ptarget=_t(ptarget))
    npt = ensemble == "npt_nose_hoover"
    fixcm = chain != 1
    kw = dict(chain=chain, loops=loops, order=order, fixcm=fixcm)
    if npt:
        refs = [MTKRef(r0[s], p0[s], ms[s], dt, t0[s], ttime if thermo else None, ptime if baro else None, lats[s], ptarget[s], **kw)
                for s in range(B)]
    else:
        refs = [NoseHooverChainRef(r0[s], p0[s], ms[s], dt, t0[s], ttime, **kw) for s in range(B)]
    cells = [np.array(l) for l in lats]
    worst = {}

    def close(name, got, want, rel=_rel):
        d = rel(np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64))
        worst[name] = max(worst.get(name, 0.0), d)
        assert d <= 1e-12, (name, d)

    for t in range(steps + 1):
        fs = [rng.normal(0.0, 1.0, (n, 3)) for n in ns]
        es = rng.normal(size=B)
        sa = rng.normal(0.0, 0.01, (B, 3, 3))
        st = (sa + sa.transpose(0, 2, 1)) / 2
        args = _args(S, _t(np.concatenate(fs)), _t(es), _t(st) if npt else None, N, t, interval, steps, ENSEMBLES[ensemble], dt,
                     fixcm=int(fixcm), chain=chain, nhc_loops=loops, nhc_order=order, ttime=ttime if thermo else 0.0,
                     ptime=ptime if baro else 0.0)
        _lib.check(lib.alignn_md_step(ctypes.byref(args), _lib.stream()), "md_step")
        for s, o in enumerate(refs):
            a, b = ptr[s], ptr[s + 1]
            if t > 0:
                o.finish(fs[s], st[s])
                o.nsteps += 1
            if t % interval == 0:
                k = t // interval
                assert S["epot"][k, s].item() == es[s]
                assert S["ekin"][k, s].item() == pytest.approx(kinetic_energy(o.p, o.m), rel=1e-12, abs=1e-300), (t, s)
                assert S["temp"][k, s].item() == pytest.approx(temperature(o.p, o.m), rel=1e-12, abs=1e-300)
                close("conserved", S["cons"][k, s].item(), o.conserved(es[s]))
                close("traj_momenta", S["tm"][k, a:b].cpu().numpy(), o.p)
                close("traj_positions", S["tp"][k, a:b].cpu().numpy(), o.r)
                if npt:
                    assert S["vout"][k, s].item() == pytest.approx(abs(np.linalg.det(cells[s])), rel=1e-12)
                    close("traj_lattice", S["tl"][k, s].cpu().numpy(), cells[s], _relmax)
                    assert S["pout"][k, s].item() == pytest.approx(pressure_of(o.p, o.m, st[s], cells[s]), rel=1e-12), (t, s)
            if t < steps:
                o.begin(fs[s], st[s])
                if npt:
                    cells[s] = o.cell
        p_d, r_d, nhc_d = S["p"].cpu().numpy(), S["r"].cpu().numpy(), S["nhc"].cpu().numpy()
        lat_d, inv_d = S["lat"].cpu().numpy(), S["inv"].cpu().numpy()
        for s, o in enumerate(refs):
            a, b = ptr[s], ptr[s + 1]
            close("positions", r_d[a:b], o.r)
            close("momenta", p_d[a:b], o.p)
            close("state", nhc_d[s], o.state())
            if npt:
                close("cell", lat_d[s], cells[s], _relmax)
                close("inverse cell", inv_d[s], np.linalg.inv(cells[s]), _relmax)
            if not baro:
                assert np.array_equal(lat_d[s], lats[s])
            if t < steps:
                fr_d = S["frac"][a:b].cpu().numpy()
                assert (fr_d >= 0.0).all() and (fr_d < 1.0).all()
                d = fr_d - o.r @ np.linalg.inv(cells[s])
                assert np.abs(d - np.round(d)).max() < 1e-9
    print(f"{ensemble} chain {chain} order {order} loops {loops}: worst relative differences {worst}")
    assert S["status"].item() == 0
    if thermo:
        assert (np.abs(S["nhc"][:, 8].cpu().numpy()) > 1e-6).all()  # (every chain moved)
    if baro:
        assert (np.abs(S["nhc"][:, 33].cpu().numpy()) > 1e-6).all() and (S["lat"].cpu().numpy() != np.stack(lats)).any()


# --- (8) what the entry point refuses --------------------------------------------------------------------------------------
def test_entry_point_refuses_bad_nose_hoover_arguments():
    lib = _lib.load()
    rng = np.random.default_rng(2)
    ns = [3, 40]
    S, ptr, lats, ms, r0, p0 = _state(ns, rng, 2)
    S.update(p=_t(np.concatenate(p0)), t0=_t([300.0, 400.0]), ptarget=_t([0.0, 0.01]))
    f, e, st = _t(rng.normal(size=(43, 3))), _t(np.zeros(2)), _t(np.zeros((2, 3, 3)))
    good = dict(chain=3, nhc_loops=1, nhc_order=3, ttime=2.0, ptime=10.0)
    bad = [(6, dict(nhc_state=None)), (5, dict(nhc_state=None)), (5, dict(chain=0)), (5, dict(chain=9)), (6, dict(nhc_order=2)),
           (5, dict(nhc_order=0)), (5, dict(nhc_order=7)), (5, dict(nhc_loops=0)), (6, dict(nhc_loops=17)), (6, dict(stress=None)),
           (6, dict(pressure=None)), (6, dict(lattice=None)), (6, dict(inv_lattice=None)), (7, {}), (-1, {})]
    before = {k: v.clone() for k, v in S.items()}
    for ens, kw in bad:
        args = _args(S, f, e, st, 43, 0, 1, 1, ens, 0.1, **{**good, **kw})
        assert lib.alignn_md_step(ctypes.byref(args), _lib.stream()) == INVALID, (ens, kw)
    torch.cuda.synchronize()
    assert all(torch.equal(S[k], v) for k, v in before.items())
    # the barostat off needs neither stress nor pressure; the good block runs
    for ens, kw in [(6, dict(ptime=0.0, stress=None, pressure=None)), (6, {}), (5, dict(stress=None, pressure=None, lattice=None))]:
        args = _args(S, f, e, st if kw.get("stress", 1) else None, 43, 0, 1, 1, ens, 0.1, **{**good, **kw})
        assert lib.alignn_md_step(ctypes.byref(args), _lib.stream()) == 0, (ens, kw)
    assert S["status"].item() == 0 and not torch.equal(S["r"], before["r"])


# --- (2) the limits, bit for bit ----------------------------------------------------------------------------------------------
def test_limits_bit_for_bit():
    sizes = [16, 24, 32, 20]
    lats, pos, _, ff3 = _stress_springs(sizes, 300, nnb=8)
    ff = _no_stress(ff3)
    ms = [np.random.default_rng(s).uniform(10.0, 60.0, n) for s, n in enumerate(sizes)]
    kw = dict(timestep=1.0, steps=60, interval=3, initial_temperature_K=300.0, seed=[1, 2, 3, 4], forces_fn=ff, device=DEV)
    off = run_md(None, lats, pos, None, ms, ensemble="npt_nose_hoover", fixcm=False, **kw)
    nve = run_md(None, lats, pos, None, ms, ensemble="nve", fixcm=False, **kw)
    for k in ("traj_positions", "traj_momenta", "epot", "ekin"):
        assert torch.equal(getattr(off, k), getattr(nve, k)), k
    for s in range(4):
        assert torch.equal(off.positions[s], nve.positions[s]) and torch.equal(off.momenta[s], nve.momenta[s])
    assert torch.equal(off.lattices.cpu(), torch.tensor(np.stack(lats))) and torch.equal(off.traj_lattices[-1], off.lattices)
    assert torch.equal(off.conserved, off.epot + off.ekin) and nve.conserved is None and nve.lattices is None
    assert off.volume[-1].cpu().numpy() == pytest.approx(np.abs(np.linalg.det(np.stack(lats))), rel=1e-12)
    assert (off.traj_positions[-1] != off.traj_positions[0]).any()
    nh = dict(temperature_K=[100.0, 300.0, 600.0, 1200.0], ttime=25.0, chain=3, nhc_loops=2, nhc_order=5)
    a = run_md(None, lats, pos, None, ms, ensemble="npt_nose_hoover", **nh, **kw)
    b = run_md(None, lats, pos, None, ms, ensemble="nvt_nose_hoover", **nh, **kw)
    for k in ("traj_positions", "traj_momenta", "epot", "ekin", "temperature", "conserved"):
        assert torch.equal(getattr(a, k), getattr(b, k)), k
    assert b.lattices is None and b.volume is None and a.pressure is None and torch.equal(a.lattices.cpu(), torch.tensor(np.stack(lats)))
    assert not torch.equal(a.traj_momenta, nve.traj_momenta)
    # fixcm: the centre-of-mass momentum is taken out of the start momenta and stays out (the spring forces sum to zero)
    ptot = torch.stack([p.sum(0) for p in b.momenta]).abs().max().item()
    assert ptot <= 1e-12 * max(p.abs().max().item() for p in b.momenta)


# --- (3) the conserved quantity -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ensemble", ["nvt_nose_hoover", "npt_nose_hoover"])
def test_conserved_quantity_second_order_and_drift(ensemble):
    sizes = [16, 24, 32, 20]
    lats, pos, _, ff3 = _stress_springs(sizes, 300, nnb=8)
    npt = ensemble == "npt_nose_hoover"
    ms = [np.full(n, 28.0) for n in sizes]
    kw = dict(ensemble=ensemble, temperature_K=300.0, ttime=25.0, initial_temperature_K=300.0, seed=[1, 2, 3, 4], trajectory=False,
              forces_fn=ff3 if npt else _no_stress(ff3), device=DEV, **(dict(ptime=250.0, pressure=1000.0) if npt else {}))
    a = run_md(None, lats, pos, None, ms, timestep=1.0, steps=1000, **kw)
    b = run_md(None, lats, pos, None, ms, timestep=0.5, steps=2000, interval=2, **kw)
    ha, hb = a.conserved.cpu().numpy(), b.conserved.cpu().numpy()
    ke = a.ekin.mean(0).cpu().numpy()
    spread_a, spread_b = ha.max(0) - ha.min(0), hb.max(0) - hb.min(0)
    drift = np.abs(ha - ha[0]).max(0)
    print(f"{ensemble}: H' spread / <KE> at 1 fs", spread_a / ke, "ratio 1 fs / 0.5 fs", spread_a / spread_b)
    assert a.conserved.shape == (1001, 4) and b.conserved.shape == (1001, 4)
    assert (drift < 5e-3 * ke).all(), drift / ke
    assert ((spread_a / spread_b > 3.0) & (spread_a / spread_b < 5.0)).all(), spread_a / spread_b
    e = (a.epot + a.ekin).cpu().numpy()
    assert ((e.max(0) - e.min(0)) > 3 * spread_a).all()  # (the thermostat does exchange energy: H' is not E)
    if npt:
        v = a.volume.cpu().numpy()
        assert ((v.max(0) - v.min(0)) / v[0] > 1e-4).all()


# --- (4) the temperature ladder -------------------------------------------------------------------------------------------------
def test_nose_hoover_reaches_its_temperature_ladder():
    sizes = [64, 64, 64, 64]
    lats, pos, ff = _spring_crystals(sizes, 600)
    ms = [np.random.default_rng(s).uniform(10.0, 60.0, n) for s, n in enumerate(sizes)]
    ladder = np.array([100.0, 300.0, 600.0, 1200.0])
    # The protocol and the bound of test_gpu_dynamics.test_thermostats_reach_their_temperature_ladder's Berendsen half: a
    # Maxwell-Boltzmann start at half the target.  The chain drives the 3N-temperature itself to T0 (G_0 = 0 at sum p^2/m =
    # 3N kT, whatever fixcm removed); ttime = 50 fs is below the spring periods (~100-200 fs), so the 2000 steps averaged hold
    # >= 10 thermostat periods.  The restatement alone meets the bound with these crystals, masses and ttime:
    # test_md_nose_hoover_ref.test_thermostat_reaches_its_temperature_ladder (<T> / T0 = 1.005, 1.028, 0.999, 0.985).
    res = run_md(None, lats, pos, None, ms, ensemble="nvt_nose_hoover", timestep=1.0, steps=4000, interval=4, temperature_K=ladder,
                 ttime=50.0, initial_temperature_K=ladder / 2, seed=[1, 2, 3, 4], fixcm=True, trajectory=False, forces_fn=ff,
                 device=DEV)
    got = _second_half_mean(res)
    print("Nose-Hoover <T> / T0:", got / ladder)
    assert (np.abs(got / ladder - 1.0) < 0.12).all(), got / ladder
    h = res.conserved.cpu().numpy()
    assert (np.abs(h - h[0]).max(0) < 5e-3 * res.ekin.mean(0).cpu().numpy()).all()


def test_mtk_barostat_reaches_its_pressure_ladder():
    # The crystals, the 3 % start, chain = 1 and the time constants of test_md_nose_hoover_ref's ladder (the reasons are there),
    # and its bound, which is that of test_gpu_dynamics_npt's Berendsen ladder.
    lats, pos, _, ff = _stress_springs(list(BARO_SIZES), BARO_SEED)
    ms = [np.full(n, 28.0) for n in BARO_SIZES]
    cells = [BARO["strain"] * lat for lat in lats]
    res = run_md(None, cells, [BARO["strain"] * r for r in pos], None, ms, ensemble="npt_nose_hoover", timestep=1.0,
                 steps=BARO["steps"], interval=BARO["interval"], temperature_K=BARO["T0"], ttime=BARO["ttime"], ptime=BARO["ptime"],
                 chain=BARO["chain"], pressure=LADDER_BAR, trajectory=False, forces_fn=ff, device=DEV)
    P, V = res.pressure.cpu().numpy(), res.volume.cpu().numpy()
    assert P.shape == (BARO["steps"] // BARO["interval"] + 1, 4)
    for s in range(4):
        resid, peak, ratio = barostat_residuals(P[:, s], V[:, s], abs(np.linalg.det(lats[s])), s)
        want = barostat_ref(s)
        print(f"barostat {s}: second-half |mean P - P_target| / rung spacing {resid:.3e} (restatement {want[0]:.3e}), "
              f"max |P - P_target| {peak:.3e}, mean V / V_rest {ratio:.6f} (restatement {want[2]:.6f})")
        assert (ratio > 1.004) if LADDER_BAR[s] < 0 else (ratio < 0.996)  # (the cell went past rest, the right way)
        assert resid < 1e-3


# --- (5) alone vs. batched ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ensemble", ["nvt_nose_hoover", "npt_nose_hoover"])
def test_nose_hoover_structure_alone_equals_its_slice_of_the_batch(ensemble):
    sizes = [5, 16, 33, 12]
    lats, pos, _, ff3 = _stress_springs(sizes, 900, nnb=8)
    npt = ensemble == "npt_nose_hoover"
    ff = ff3 if npt else _no_stress(ff3)
    ms = [np.random.default_rng(s).uniform(1.0, 100.0, n) for s, n in enumerate(sizes)]
    seeds, t0, press = [11, 22, 2 ** 63 + 33, 44], [200.0, 400.0, 800.0, 1600.0], [-1e4, 0.0, 5e3, 2e4]
    kw = dict(ensemble=ensemble, timestep=2.0, steps=60, interval=3, ttime=40.0, forces_fn=ff, device=DEV)

    def more(sl):
        return dict(pressure=press[sl], ptime=300.0) if npt else {}

    both = run_md(None, lats, pos, None, ms, temperature_K=t0, initial_temperature_K=t0, seed=seeds, **more(slice(None)), **kw)
    ptr = np.concatenate([[0], np.cumsum(sizes)])
    for s in range(4):
        one = run_md(None, lats[s:s + 1], pos[s:s + 1], None, ms[s:s + 1], temperature_K=t0[s], initial_temperature_K=t0[s],
                     seed=seeds[s], **more(s), **kw)
        a, b = ptr[s], ptr[s + 1]
        assert torch.equal(one.traj_positions, both.traj_positions[:, a:b]), s
        assert torch.equal(one.traj_momenta, both.traj_momenta[:, a:b]), s
        for k in ("epot", "ekin", "temperature", "conserved") + (("pressure", "volume") if npt else ()):
            assert torch.equal(getattr(one, k)[:, 0], getattr(both, k)[:, s]), (s, k)
        assert torch.equal(one.positions[0], both.positions[s]) and torch.equal(one.momenta[0], both.momenta[s])
        if npt:
            assert torch.equal(one.traj_lattices[:, 0], both.traj_lattices[:, s]) and torch.equal(one.lattices[0], both.lattices[s])
    assert (both.traj_momenta[-1] != both.traj_momenta[0]).any()
    if npt:
        assert (both.traj_lattices[-1] != both.traj_lattices[0]).any()


# --- (6), (7) a random-initialised ALIGNNAtomWise -------------------------------------------------------------------------
NH_KW = dict(ttime=20.0, ptime=200.0, pressure=0.0)


def _host_loop(model, lats, pos, feats, ms, ensemble, steps, dt, t0, seeds, t_init):
    """test_gpu_dynamics_npt._host_loop with the restatement of this feature."""
    B = len(pos)
    npt = ensemble == "npt_nose_hoover"
    p0 = [maxwell_boltzmann(seeds[s], ms[s], t_init) for s in range(B)]
    if npt:
        refs = [MTKRef(pos[s], p0[s], ms[s], dt, t0, NH_KW["ttime"] * FS, NH_KW["ptime"] * FS, lats[s], NH_KW["pressure"] * BAR,
                       fixcm=True) for s in range(B)]
    else:
        refs = [NoseHooverChainRef(pos[s], p0[s], ms[s], dt, t0, NH_KW["ttime"] * FS, fixcm=True) for s in range(B)]
    epot, cons = host_md_loop(model, refs, lats, feats, steps, "both", lambda o, e, st: o.conserved(e))
    return refs, epot, cons


@pytest.mark.parametrize("ensemble", ["nvt_nose_hoover", "npt_nose_hoover"])
def test_run_md_nose_hoover_model_matches_a_host_loop(ensemble):
    model = _model()
    lats, pos, feats, ms = _crystals()
    seeds, steps = [5, 6, 7, 8, 9, 10], 5
    npt = ensemble == "npt_nose_hoover"
    kw = NH_KW if npt else dict(ttime=NH_KW["ttime"])
    res = run_md(model, lats, pos, feats, ms, ensemble=ensemble, timestep=2.0, steps=steps, temperature_K=500.0,
                 initial_temperature_K=500.0, seed=seeds, **kw)
    refs, epot, cons = _host_loop(model, lats, pos, feats, ms, ensemble, steps, 2.0 * FS, 500.0, seeds, 500.0)
    dpos = max(np.abs(res.positions[s].cpu().numpy() - refs[s].r).max() for s in range(6))
    dmom = max(_rel(res.momenta[s].cpu().numpy(), refs[s].p) for s in range(6))
    de = np.abs(res.epot.cpu().numpy() - epot).max() / np.abs(epot).max()
    dc = np.abs(res.conserved.cpu().numpy() - cons).max() / np.abs(cons).max()
    moved = max(np.abs(refs[s].r - pos[s]).max() for s in range(6))
    print(f"run_md {ensemble} vs host loop after {steps} steps: max |dpos| {dpos:.3e} A (atoms moved up to {moved:.3e} A), "
          f"momenta rel {dmom:.3e}, energy rel {de:.3e}, conserved rel {dc:.3e}")
    assert moved > 1e-3 and res.n_evals == steps + 1
    # the tolerances of test_gpu_dynamics.test_run_md_model_matches_a_host_loop; the conserved energy holds the model's
    # float32 energy and is held to the energies' bound
    assert dpos <= 3 * 3.6e-15 and dmom <= 3 * 5.2e-14 and de <= 3 * 2.0 ** -24 and dc <= 3 * 2.0 ** -24, (dpos, dmom, de, dc)
    if npt:
        dcell = max(_relmax(res.lattices[s].cpu().numpy(), refs[s].cell) for s in range(6))
        dvol = np.array([abs(np.linalg.det(refs[s].cell)) / abs(np.linalg.det(lats[s])) - 1.0 for s in range(6)])
        print(f"    volumes changed by {dvol}, cell rel {dcell:.3e}")
        assert (np.abs(dvol) > 1e-7).all() and dcell <= 3 * 2.0 ** -24


@pytest.mark.parametrize("ensemble", ["nvt_nose_hoover", "npt_nose_hoover"])
def test_nose_hoover_replay_gives_the_same_bits_and_runs_repeat(ensemble):
    model = _model()
    lats, pos, feats, ms = _crystals(4)
    npt = ensemble == "npt_nose_hoover"
    kw = dict(ensemble=ensemble, timestep=2.0, steps=20, temperature_K=400.0, initial_temperature_K=400.0, seed=[1, 2, 3, 4],
              **(NH_KW if npt else dict(ttime=NH_KW["ttime"])))
    a = run_md(model, lats, pos, feats, ms, replay=False, **kw)
    b = run_md(model, lats, pos, feats, ms, replay=True, **kw)
    c = run_md(model, lats, pos, feats, ms, replay=False, **kw)
    for x in (b, c):
        assert torch.equal(a.traj_positions, x.traj_positions) and torch.equal(a.traj_momenta, x.traj_momenta)
        assert torch.equal(a.epot, x.epot) and torch.equal(a.ekin, x.ekin) and torch.equal(a.conserved, x.conserved)
        for u, v in zip(a.forces, x.forces):
            assert torch.equal(u, v)
        if npt:
            assert torch.equal(a.traj_lattices, x.traj_lattices) and torch.equal(a.pressure, x.pressure)
            assert torch.equal(a.volume, x.volume) and torch.equal(a.lattices, x.lattices)
    assert (a.traj_positions[-1] != a.traj_positions[0]).any()
    if npt:
        assert (a.traj_lattices[-1] != a.traj_lattices[0]).any()
