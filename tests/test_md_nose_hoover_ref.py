"""Checks of tests/md_nose_hoover_ref.py, the float64 numpy restatement of Nose-Hoover chains and of the isotropic MTK barostat
that specifies the ``nvt_nose_hoover`` and ``npt_nose_hoover`` ensembles of ``alignn_amd.run_md`` (csrc/dynamics.hip,
``alignn_md_step`` with ensembles 5 and 6).  They pin the restatement by what does not come from the kernel: second-order
conservation of H', time reversal, a step by hand, its limits and the thermostat's and barostat's targets; and what the entry
point refuses before it touches a device.  The GPU tests (test_gpu_dynamics_nose_hoover.py) hold the kernel and ``run_md`` to the
restatement."""

import ctypes

import numpy as np
import pytest

from alignn_amd import _lib, dynamics
from alignn_amd.dynamics import BAR, FS, KB, MDResult, run_md
from alignn_amd.synthetic import make_crystal
from tests.md_nose_hoover_ref import (LADDER_BAR, MTKRef, NoseHooverChainRef, barostat_ref, nhc_half, remove_com, run_nh_ref,
                                      sinhc, spring_case, sy_weights)
from tests.md_ref import VerletRef, kinetic_energy, maxwell_boltzmann, temperature
from tests.springs_ref import spring_list, springs_efs


KINDS = {"nvt": dict(ttime=25.0, ptime=None), "npt": dict(ttime=25.0, ptime=100.0), "nph": dict(ttime=None, ptime=100.0)}


def _integ(kind, dt_fs, case, **kw):
    cell, r, p, m, _ = case
    tt, pt = KINDS[kind]["ttime"], KINDS[kind]["ptime"]
    as_mtk = kw.pop("as_mtk", False)
    if kind == "nvt" and not as_mtk:
        return NoseHooverChainRef(r, p, m, dt_fs * FS, 300.0, tt * FS, **kw)
    return MTKRef(r, p, m, dt_fs * FS, 300.0, None if tt is None else tt * FS, None if pt is None else pt * FS, cell,
                  1000.0 * BAR, **kw)


# ---- the checks -----------------------------------------------------------------------------------------------------------
def test_suzuki_yoshida_weights_and_sinhc():
    for order in (1, 3, 5):
        w = sy_weights(order)
        assert len(w) == order and abs(sum(w) - 1.0) <= 1e-15 and w == w[::-1]
    # the cube roots as the kernel spells them
    assert 2.0 ** (1.0 / 3.0) == 1.2599210498948732 and 4.0 ** (1.0 / 3.0) == 1.5874010519681994
    assert sinhc(0.0) == 1.0
    for x in (1e-3, -5e-3, 9.99e-3, 1e-2, 0.3, -2.0):
        assert sinhc(x) == pytest.approx(float(np.sinh(np.longdouble(x)) / np.longdouble(x)), rel=4e-16)


def test_nhc_half_identity_at_equilibrium():
    for M in (1, 3, 8):
        for order in (1, 3, 5):
            kT, dof = 0.025, 21.0
            Q = np.full(M, kT * 4.0)
            Q[0] *= dof
            v, eta = np.zeros(M), np.zeros(M)
            # K2 = dof kT: G_0 = 0, link 0 stays at rest and the momenta are untouched, exactly.  The links above it are driven
            # by Q_{k-1} v_{k-1}^2 - kT = -kT and do move; a chain of one link is a fixed point altogether.
            s = nhc_half(dof * kT, dof, kT, Q, v, eta, 0.1, 2, order)
            assert s == 1.0 and v[0] == 0.0 and eta[0] == 0.0
            if M == 1:
                assert (v == 0.0).all() and (eta == 0.0).all()
            else:
                assert (v[1:] < 0.0).all()


def test_nhc_half_orders_agree_and_converge():
    kT, dof, M = 0.03, 12.0, 3
    Q = np.full(M, kT * 6.0)
    Q[0] *= dof

    def run(dt, order, loops):
        v, eta = np.array([0.05, -0.02, 0.01]), np.zeros(M)
        s = nhc_half(1.7 * dof * kT, dof, kT, Q, v, eta, dt, loops, order)
        return np.concatenate([[s], v, eta])

    for order in (3, 5):
        d1 = np.abs(run(0.4, order, 16) - run(0.4, 1, 16)).max()
        d2 = np.abs(run(0.2, order, 16) - run(0.2, 1, 16)).max()
        assert d1 < 1e-5 and d2 < d1 / 4, (order, d1, d2)  # (order 1 is second order in h: its error falls 8-fold per halving)


def test_nose_hoover_by_hand():
    # one atom, one link, order 1, one loop; the force is -k x along x
    m, dt, T0, tau, k = 2.0, 0.1, 100.0, 0.5, 3.0
    kT, g = KB * T0, 3.0
    Q = g * kT * tau * tau
    x, p = 1.0, 0.3
    ref = NoseHooverChainRef(np.array([[x, 0.0, 0.0]]), np.array([[p, 0.0, 0.0]]), np.array([m]), dt, T0, tau, chain=1, order=1)
    ref.begin(np.array([[-k * x, 0.0, 0.0]]))
    h = 1.0 * (0.5 * dt) / 1
    K2 = p * p / m
    v0 = 0.0 + 0.5 * h * ((K2 * 1.0 * 1.0 - g * kT) / Q)
    s = 1.0 * np.exp(-h * v0)
    eta0 = 0.0 + h * v0
    v0 = v0 + 0.5 * h * ((K2 * s * s - g * kT) / Q)
    p = s * p
    p = p + 0.5 * dt * (-k * x)
    x = x + dt * p / m
    assert ref.p[0, 0] == p and ref.r[0, 0] == x and ref.v[0] == v0 and ref.eta[0] == eta0
    ref.finish(np.array([[-k * x, 0.0, 0.0]]))
    p = p + 0.5 * dt * (-k * x)
    K2 = p * p / m
    v0 = v0 + 0.5 * h * ((K2 * 1.0 * 1.0 - g * kT) / Q)
    s = 1.0 * np.exp(-h * v0)
    eta0 = eta0 + h * v0
    v0 = v0 + 0.5 * h * ((K2 * s * s - g * kT) / Q)
    p = s * p
    assert ref.p[0, 0] == p and ref.v[0] == v0 and ref.eta[0] == eta0
    assert (ref.p[0, 1:] == 0).all() and (ref.r[0, 1:] == 0).all()
    assert ref.conserved(0.5 * k * x * x) == (0.5 * (p * p / m) + 0.5 * k * x * x) + (0.5 * (Q * v0 * v0) + g * kT * eta0 + kT * 0.0)


def test_limits_bit_for_bit():
    rng = np.random.default_rng(3)
    case = spring_case()
    cell, r, p, m, efs = case
    dt = 1.0 * FS
    off = MTKRef(r, p, m, dt, 300.0, None, None, cell)
    vv = VerletRef(r, p, m, dt)
    nvt = NoseHooverChainRef(r, p, m, dt, 300.0, 25.0 * FS, chain=3, loops=2, order=5, fixcm=True)
    mtk = MTKRef(r, p, m, dt, 300.0, 25.0 * FS, None, cell, chain=3, loops=2, order=5, fixcm=True)
    for _ in range(4):
        f = rng.normal(0.0, 1.0, r.shape)
        for o in (off, vv, nvt, mtk):
            o.begin(f)
        f = rng.normal(0.0, 1.0, r.shape)
        for o in (off, vv, nvt, mtk):
            o.finish(f)
        assert np.array_equal(off.r, vv.r) and np.array_equal(off.p, vv.p) and np.array_equal(off.cell, cell)
        assert np.array_equal(mtk.r, nvt.r) and np.array_equal(mtk.p, nvt.p) and np.array_equal(mtk.state(), nvt.state())
        assert mtk.conserved(0.25) == nvt.conserved(0.25) and np.array_equal(mtk.cell, cell)
    assert off.conserved(0.5) == kinetic_energy(vv.p, m) + 0.5 and (off.state() == 0.0).all()
    assert not np.array_equal(nvt.p, vv.p) and (nvt.state()[:3] != 0.0).all()
    assert np.abs(remove_com(p, m).sum(axis=0)).max() <= 1e-14 * np.abs(p).max()


@pytest.mark.parametrize("kind", ["nvt", "npt", "nph"])
def test_conserved_quantity_is_second_order(kind):
    case = spring_case()
    efs = case[4]

    def spread(dt_fs, steps):
        H = np.array([fr[8] for fr in run_nh_ref(_integ(kind, dt_fs, case), efs, steps, cell=case[0])["frames"]])
        return np.abs(H - H[0]).max()

    a, b = spread(1.0, 300), spread(0.5, 600)
    ke = kinetic_energy(case[2], case[3])
    print(f"{kind}: max |H' - H'(0)| at 1 fs {a:.3e} eV, at 0.5 fs {b:.3e} eV (KE {ke:.3e} eV), ratio {a / b:.3f}")
    assert a < 5e-3 * ke and 3.0 < a / b < 5.0, (a, b)


# the return error of the restatement as it stands, measured here (max over positions in A, momenta relative to the largest,
# cell relative, chain state absolute): nvt 1.1e-13, npt 6.0e-14, nph 3.3e-14.  100x that is asserted; a factorisation that is not
# symmetric (second_exp=False) misses the start by ~1 A.
REVERSAL = {"nvt": 1.1e-13, "npt": 6.0e-14, "nph": 3.3e-14}


def _reversal_error(kind, steps=200, **kw):
    case = spring_case()
    cell, r, p, m, efs = case
    integ = _integ(kind, 1.0, case, as_mtk=True, **kw)
    run_nh_ref(integ, efs, steps)
    moved = np.abs(integ.r - r).max()
    integ.reverse()
    run_nh_ref(integ, efs, steps)
    err = max(np.abs(integ.r - r).max(), np.abs(integ.p + p).max() / np.abs(p).max(), np.abs(integ.cell - cell).max() / np.abs(cell).max(),
              np.abs(integ.state()[[0, 1, 2, 16, 17, 18, 32]]).max())
    return moved, err


@pytest.mark.parametrize("kind", ["nvt", "npt", "nph"])
def test_time_reversal(kind):
    moved, err = _reversal_error(kind)
    print(f"{kind}: moved {moved:.3e} A, back to {err:.3e}")
    assert moved > 0.05 and err <= 100 * REVERSAL[kind], (moved, err)
    if kind != "nph":  # (nph runs no chain)
        _, bad = _reversal_error(kind, second_exp=False)
        print(f"{kind} without the second exp factor: back to {bad:.3e}")
        assert bad > 1e4 * REVERSAL[kind]


def test_barostat_reaches_its_pressure_ladder():
    res = [barostat_ref(s) for s in range(4)]
    for s, (resid, peak, ratio) in enumerate(res):
        print(f"barostat {s}: second-half |mean P - P_target| / rung spacing {resid:.3e}, max |P - P_target| {peak:.3e}, "
              f"mean V / V_rest {ratio:.6f}")
    for s, (resid, peak, ratio) in enumerate(res):
        assert (ratio > 1.004) if LADDER_BAR[s] < 0 else (ratio < 0.996)  # (the cell went past rest, the right way)
        assert resid < 1e-3  # (the bound of test_gpu_dynamics_npt's Berendsen ladder)


# The thermostat: the crystals, masses, ladder, protocol (a Maxwell-Boltzmann start at half the target, the centre of mass
# taken out once) and bound of test_gpu_dynamics.test_thermostats_reach_their_temperature_ladder, with the ttime that
# test_gpu_dynamics_nose_hoover's ladder uses.  Instantaneous T has a relative spread of sqrt(2 / 3N) = 0.10; ttime = 50 fs is
# below the spring periods (~100-200 fs), so the 2000 steps averaged hold >= 10 thermostat periods: 0.12 is ~4 standard errors.
T_LADDER = np.array([100.0, 300.0, 600.0, 1200.0])
THERMO = dict(ttime=50.0, n=64, seed0=600, steps=4000, interval=4)


@pytest.mark.parametrize("s", range(4))
def test_thermostat_reaches_its_temperature_ladder(s):
    n, T0 = THERMO["n"], T_LADDER[s]
    lat, frac, _ = make_crystal(n, THERMO["seed0"] + s)
    efs = springs_efs(*spring_list(lat, frac, nnb=8))
    m = np.random.default_rng(s).uniform(10.0, 60.0, n)
    integ = NoseHooverChainRef(frac @ lat, maxwell_boltzmann(s + 1, m, T0 / 2), m, 1.0 * FS, T0, THERMO["ttime"] * FS, fixcm=True)
    fr = run_nh_ref(integ, efs, THERMO["steps"], THERMO["interval"], cell=lat)["frames"]
    T = np.array([temperature(f[2], m) for f in fr])
    H, ke = np.array([f[8] for f in fr]), np.mean([f[4] for f in fr])
    got, drift = T[len(T) // 2:].mean() / T0, np.abs(H - H[0]).max() / ke
    print(f"thermostat {s}: second-half <T> / T0 {got:.4f}, max |H' - H'(0)| / <KE> {drift:.2e}")
    assert abs(got - 1.0) < 0.12
    assert drift < 5e-3


def test_mtk_begin_by_hand():
    # one atom, no thermostat: v_eps += dt/2 G_eps, the scaled half-kick, the scaled drift, the cell
    m, dt, T0, taup, pext = 2.0, 0.1, 100.0, 0.7, 0.01
    kT, g = KB * T0, 3.0
    alpha, W = 1.0 + 3.0 / g, (g + 3.0) * kT * taup * taup
    x, p, F = 1.0, 0.3, -3.0
    stress = np.diag([-0.01, -0.02, -0.03])
    ref = MTKRef(np.array([[x, 0.0, 0.0]]), np.array([[p, 0.0, 0.0]]), np.array([m]), dt, T0, None, taup, 2.0 * np.eye(3), pext)
    ref.begin(np.array([[F, 0.0, 0.0]]), stress)
    veps = 0.0 + 0.5 * dt * ((alpha * (p * p / m) + 3.0 * 8.0 * (0.02 - pext)) / W)
    assert alpha == 2.0 and ref.veps == pytest.approx(veps, rel=1e-15)
    xk = alpha * veps * 0.25 * dt
    p = p * np.exp(-alpha * veps * (0.5 * dt)) + 0.5 * dt * F * (np.exp(-xk) * (np.sinh(xk) / xk))
    y = veps * (0.5 * dt)
    x = x * np.exp(veps * dt) + dt * (p / m) * (np.exp(y) * (np.sinh(y) / y))
    assert abs(xk) > 1e-2 and ref.p[0, 0] == pytest.approx(p, rel=1e-15) and ref.r[0, 0] == pytest.approx(x, rel=1e-15)
    assert np.allclose(ref.cell, 2.0 * np.exp(veps * dt) * np.eye(3), rtol=1e-15, atol=0) and ref.eps == veps * dt
    assert ref.conserved(0.5) == pytest.approx(0.5 * p * p / m + 0.5 + pext * 8.0 * np.exp(3.0 * veps * dt) + 0.5 * W * veps * veps,
                                               rel=1e-14)
    assert (ref.state()[:32] == 0.0).all()  # (no thermostat: a barostat alone runs no chain)


# ---- the interface ---------------------------------------------------------------------------------------------------------
def test_run_md_validates_the_nose_hoover_arguments_before_touching_a_device():
    assert dynamics.ENSEMBLES["nvt_nose_hoover"] == 5 and dynamics.ENSEMBLES["npt_nose_hoover"] == 6
    res = MDResult(1, 2, 3, 4, 5, 6, 7, 8, 9)
    assert res.n_evals == 9 and res.conserved is None and res.traj_lattices is None
    assert list(MDResult.__dataclass_fields__)[-2:] == ["traj_lattices", "conserved"]
    names = [f[0] for f in _lib.MdArgs._fields_]
    assert names[-7:] == ["nhc_state", "conserved_out", "chain", "nhc_loops", "nhc_order", "ttime", "ptime"]
    assert names[-8] == "kB"
    empty = _lib.MdArgs(ensemble=2)  # (a block filled by name: the new fields default to NULL / 0)
    assert empty.nhc_state is None and empty.conserved_out is None and empty.chain == 0 and empty.ttime == 0.0
    from alignn_amd.build import build

    build()
    assert _lib.load().alignn_md_args_sizeof() == ctypes.sizeof(_lib.MdArgs)
    lat, pos, m = [np.eye(3) * 5, np.eye(3) * 6], [np.zeros((2, 3)), np.ones((3, 3))], [np.ones(2), np.ones(3)]
    ff = lambda lat, pos: None  # noqa: E731
    nvt = dict(ensemble="nvt_nose_hoover", ttime=25.0)
    npt = dict(ensemble="npt_nose_hoover", ttime=25.0, ptime=250.0, pressure=1.0)
    bad = [
        dict(ensemble="npt"),
        dict(ensemble="nvt_nose_hoover"),  # no ttime
        dict(nvt, ttime=0.001),  # below the timestep (0.01 fs)
        dict(nvt, ttime=float("inf")),
        dict(nvt, ttime=float("nan")),
        dict(nvt, temperature_K=0.0),
        dict(nvt, temperature_K=[300.0, 0.0]),
        dict(nvt, chain=0),
        dict(nvt, chain=9),
        dict(nvt, chain=2.5),
        dict(nvt, nhc_loops=0),
        dict(nvt, nhc_loops=17),
        dict(nvt, nhc_order=2),
        dict(nvt, nhc_order=7),
        dict(npt, ptime=0.001),
        dict(npt, ptime=float("inf")),
        dict(npt, pressure=None),
        dict(npt, pressure=float("nan")),
        dict(npt, pressure=[1.0, 2.0, 3.0]),
        dict(npt, temperature_K=0.0),
        dict(npt, ttime=None, temperature_K=0.0),  # the barostat's mass divides by kT too
        dict(npt, stress_weight=float("nan")),
        dict(npt, chain=0),
        dict(npt, nhc_order=4),
    ]
    for kw in bad:
        with pytest.raises(ValueError):
            run_md(None, lat, pos, None, m, forces_fn=ff, **kw)
    # valid arguments get as far as the device: a CPU device is a TypeError, raised after every ValueError check
    good = [nvt, npt, dict(npt, pressure=[-5.0, 5.0]), dict(npt, ttime=None), dict(npt, ptime=None, pressure=None),
            dict(ensemble="npt_nose_hoover", temperature_K=0.0), dict(nvt, chain=8, nhc_loops=16, nhc_order=5),
            dict(nvt, chain=1, nhc_order=1)]
    for kw in good:
        with pytest.raises(TypeError):
            run_md(None, lat, pos, None, m, forces_fn=ff, device="cpu", **kw)
