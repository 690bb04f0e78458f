"""Checks of tests/md_npt_ref.py, the float64 numpy restatement of ASE 3.22.1's ``Andersen`` and ``NPTBerendsen`` that specifies
the ``nvt_andersen`` and ``npt_berendsen`` ensembles of ``alignn_amd.run_md`` (csrc/dynamics.hip, ``alignn_md_step`` with
ensembles 3 and 4): steps computed by hand, the identities and limits of the two integrators, the draws against the project's
random stream, and what the entry point refuses before it touches a device.  The GPU tests (test_gpu_dynamics_npt.py) hold the
kernel and ``run_md`` to the restatement."""

import ctypes
import os

import numpy as np
import pytest

from alignn_amd import _lib, dynamics
from alignn_amd.dynamics import FS, KB, MDResult, run_md
from tests.md_npt_ref import PURPOSE_ANDERSEN, AndersenRef, NPTBerendsenRef, andersen_draws, pressure_of, run_npt_ref
from tests.md_ref import (BerendsenRef, VerletRef, berendsen_scale, box_muller, normals, stream_words, temperature,
                          unit_interval)


# ---- the checks -----------------------------------------------------------------------------------------------------------
def test_bar_and_taup_default():
    from alignn_amd.dynamics import BAR, barostat_taup

    assert BAR == 1e-4 / 160.21766208
    assert BAR == pytest.approx(1e5 / (1.6021766208e-19 * 1e30), rel=1e-15)  # 1 bar = 1e5 Pa; eV/A^3 = e J / 1e-30 m^3
    assert barostat_taup(None) == 1000.0 * FS == pytest.approx(98.22694788464063, rel=1e-15)  # ff.py's NPTBerendsen taup
    assert barostat_taup(250.0) == 250.0 * FS


def _hand_case(fixcm=False):
    m, dt, taut = np.array([2.0]), 0.1, 10.0
    p0 = np.array([[0.3, 0.0, 0.0]])
    T = 2 * (0.5 * 0.09 / 2.0) / (3 * KB)
    # KE after the scaling: 0.0225 * 1.03 = 0.023175; V = 8; P = 0.02 + 2 * 0.023175 / 24 = 0.02193125; target 0.01 below
    return NPTBerendsenRef(np.array([[1.0, 0.0, 0.0]]), p0, m, dt, T0=4 * T, taut=taut, cell=2.0 * np.eye(3), taup=1.0,
                           pressure=0.01193125, compressibility=3.0, fixcm=fixcm)


def test_npt_berendsen_by_hand():
    b = _hand_case()
    stress = np.diag([-0.01, -0.02, -0.03])
    b.begin(np.array([[-1.0, 0.0, 0.0]]), stress)
    assert b.P == pytest.approx(0.02193125, rel=1e-14)
    assert b.mu == pytest.approx(1.001, rel=1e-14)  # 1 - 0.1 / 1 * 3 / 3 * (-0.01)
    assert np.allclose(b.cell, 2.002 * np.eye(3), rtol=1e-14, atol=0)
    p = 0.3 * np.sqrt(1.03) - 0.05  # the scaling, then p += 0.05 * -1
    assert b.p[0, 0] == pytest.approx(p, rel=1e-15)
    assert b.r[0, 0] == pytest.approx(1.001 + 0.05 * p, rel=1e-14)  # mu x, then x += 0.1 p / 2
    assert (b.p[0, 1:] == 0).all() and (b.r[0, 1:] == 0).all()
    b.finish(np.array([[-0.5, 0.25, 0.0]]))
    assert b.p[0, 0] == pytest.approx(p - 0.025, rel=1e-15) and b.p[0, 1] == pytest.approx(0.0125, rel=1e-15)
    # two atoms, fixcm: the plain mean of the momenta after the half-kick goes, at T0 = 0 and zero stress
    two = NPTBerendsenRef(np.array([[1.0, 0, 0], [0.0, 2.0, 0]]), np.array([[1.0, 0, 0], [0.0, 0, 0]]), np.array([1.0, 3.0]),
                          0.1, T0=0.0, taut=10.0, cell=4.0 * np.eye(3), taup=2.0, pressure=0.0, compressibility=6.0)
    two.begin(np.array([[0.0, 2.0, 0.0], [0.0, 0.0, 0.0]]), np.zeros((3, 3)))
    s2 = 1.0 - 0.01  # the squared scaling factor
    P = 2 * (0.5 * s2) / (3 * 64.0)
    mu = 1.0 - 0.1 / 2.0 * 6.0 / 3.0 * (0.0 - P)
    assert two.P == pytest.approx(P, rel=1e-14) and two.mu == pytest.approx(mu, rel=1e-15)
    want = np.array([[np.sqrt(s2), 0.1, 0.0], [0.0, 0.0, 0.0]])
    want -= want.mean(axis=0)
    assert np.allclose(two.p, want, rtol=0, atol=1e-15)
    assert np.allclose(two.r, mu * np.array([[1.0, 0, 0], [0.0, 2.0, 0]]) + 0.1 * want / np.array([[1.0], [3.0]]), rtol=0,
                       atol=1e-15)


def _random_state(rng, n):
    cell = 6.0 * np.eye(3) + rng.normal(0.0, 0.4, (3, 3))
    m = rng.uniform(1.0, 100.0, n)
    r = rng.uniform(0.0, 1.0, (n, 3)) @ cell
    p = rng.normal(0.0, 1.0, (n, 3)) * np.sqrt(m * KB * 300.0)[:, None]
    a = rng.normal(0.0, 0.01, (3, 3))
    return cell, m, r, p, (a + a.T) / 2


def test_npt_berendsen_identities():
    rng = np.random.default_rng(4)
    dt, taut, taup = 1.0 * FS, 50.0 * FS, 200.0 * FS
    for n in (1, 7, 40):
        cell, m, r, p, stress = _random_state(rng, n)
        # compressibility 0: NVTBerendsen, bit for bit, and the cell stays
        a = NPTBerendsenRef(r, p, m, dt, 500.0, taut, cell, taup, 0.003, 0.0)
        b = BerendsenRef(r, p, m, dt, 500.0, taut)
        for _ in range(4):
            f = rng.normal(0.0, 1.0, (n, 3))
            a.begin(f, stress)
            b.begin(f)
            assert a.mu == 1.0 and np.array_equal(a.r, b.r) and np.array_equal(a.p, b.p) and np.array_equal(a.cell, cell)
            f = rng.normal(0.0, 1.0, (n, 3))
            a.finish(f)
            b.finish(f)
            assert np.array_equal(a.p, b.p)
        # the scaling keeps the fractional coordinates and changes the volume by mu^3 (zero forces and momenta: no drift)
        c = NPTBerendsenRef(r, np.zeros_like(p), m, dt, 0.0, taut, cell, taup, 0.02, 40.0, fixcm=False)
        frac0, v0 = r @ np.linalg.inv(cell), abs(np.linalg.det(cell))
        c.begin(np.zeros((n, 3)), stress)
        assert c.mu != 1.0 and abs(c.mu - 1.0) < 0.1
        assert np.abs(c.r @ np.linalg.inv(c.cell) - frac0).max() <= 1e-15 * max(1.0, np.abs(frac0).max())
        assert abs(np.linalg.det(c.cell)) == pytest.approx(c.mu ** 3 * v0, rel=1e-14)
        # at the target pressure nothing is scaled
        d = NPTBerendsenRef(r, p, m, dt, 500.0, taut, cell, taup, 0.0, 40.0)
        d.p = berendsen_scale(500.0, temperature(p, m), dt, taut) * d.p
        d.pressure = pressure_of(d.p, m, stress, cell)
        d.p = np.array(p)
        d.begin(np.zeros((n, 3)), stress)
        assert d.P == d.pressure and d.mu == 1.0 and np.array_equal(d.cell, cell)


def test_run_npt_ref_schedule_and_barostat_direction():
    # a cubic one-atom "crystal" whose stress is that of springs to its own images: S = k (a - a0) a^2 / a^3 on the diagonal
    k, a0 = 2.0, 3.0

    def efs(cell, r):
        a = cell[0, 0]
        return 1.5 * k * (a - a0) ** 2, np.zeros_like(r), np.eye(3) * k * (a - a0) / a

    for target in (-0.05, 0.0, 0.05):
        integ = NPTBerendsenRef(np.zeros((1, 3)), np.zeros((1, 3)), np.array([10.0]), 1.0, 0.0, 100.0, a0 * np.eye(3), 20.0,
                                target, 1.0, fixcm=False)
        res = run_npt_ref(integ, efs, 600, interval=100)
        assert [fr[0] for fr in res["frames"]] == list(range(0, 601, 100)) and res["n_evals"] == 601
        a = integ.cell[0, 0]
        assert res["frames"][-1][6] == pytest.approx(target, abs=1e-6)  # P relaxes to the target
        assert a == pytest.approx(a0 / (1.0 + target / k), rel=1e-4)  # -k (a - a0) / a = target
        assert res["frames"][-1][7] == pytest.approx(a ** 3, rel=1e-14)


def test_andersen_by_hand():
    dt, T0 = 0.1, 0.5 / KB  # kB T = 0.5 eV
    m = np.array([1.0, 2.0])
    r0 = np.array([[0.0, 0.0, 0.0], [1.0, 1.0, 1.0]])
    p0 = np.array([[0.2, 0.0, 0.0], [0.0, -0.4, 0.0]])
    f = np.array([[1.0, 0.0, 0.0], [0.0, 0.0, 2.0]])
    g = np.array([[0.5, 9.0, 9.0], [9.0, -1.0, 9.0]])
    u = np.array([[0.05, 0.5, 0.11], [0.9, 0.1, 1.0]])  # replaced: atom 0 x (0.05) and atom 1 y (0.1 <= 0.1), no other
    a = AndersenRef(r0, p0, m, dt, T0, 0.1, fixcm=False)
    a.begin(f, None, g, u)
    # atom 0: v = (0.2 + 0.05, 0, 0), x replaced by 0.5 sqrt(0.5 / 1); atom 1: v = (0, -0.2, 0.05), y by -sqrt(0.5 / 2) = -0.5
    want = np.array([[0.5 * np.sqrt(0.5), 0.0, 0.0], [0.0, -0.5, 0.05]])
    assert np.allclose(a.v_replaced, want, rtol=1e-15, atol=0)
    assert np.allclose(a.r, r0 + 0.1 * want, rtol=1e-15, atol=0) and np.allclose(a.v, want, rtol=0, atol=1e-14)
    a.finish(np.array([[0.0, 1.0, 0.0], [4.0, 0.0, 0.0]]))
    want2 = a.v_drift + np.array([[0.0, 0.05, 0.0], [0.1, 0.0, 0.0]])
    assert np.allclose(a.p, m[:, None] * want2, rtol=0, atol=1e-14)
    # fixcm: every atom first gets the same random velocity com sqrt(kB T / sum m)
    b = AndersenRef(r0, p0, m, dt, T0, 0.0, fixcm=True)
    b.begin(np.zeros((2, 3)), np.array([1.0, -2.0, 0.0]), g, u)
    w = np.sqrt(0.5 / 3.0)
    assert np.allclose(b.v_replaced, p0 / m[:, None] + np.array([w, -2.0 * w, 0.0]), rtol=1e-15, atol=0)


def test_andersen_limits():
    rng = np.random.default_rng(8)
    dt = 1.0 * FS
    for n in (1, 6, 50):
        _, m, r, p, _ = _random_state(rng, n)
        # probability 0 without fixcm: velocity Verlet.  The positions agree to 1e-15 relative.  The momenta cannot: beside
        # the rounding of p / m * m, v = (r - x) / dt divides the rounding of r (1e-16 |r|) by dt, so they agree to
        # 1e-15 |r| m / dt (here 1e-13 of |p|), which is what is asserted
        a, v = AndersenRef(r, p, m, dt, 300.0, 0.0, fixcm=False, seed=n), VerletRef(r, p, m, dt)
        for _ in range(3):
            f = rng.normal(0.0, 1.0, (n, 3))
            a.begin(f)
            v.begin(f)
            assert np.abs(a.r - v.r).max() <= 1e-15 * np.abs(v.r).max()
            f = rng.normal(0.0, 1.0, (n, 3))
            a.finish(f)
            v.finish(f)
            a.nsteps += 1
            assert np.abs(a.p - v.p).max() <= 1e-15 * np.abs(v.r).max() / dt * m.max()
        # probability 1: exactly the drawn velocities before the drift
        for fixcm in (False, True):
            b = AndersenRef(r, p, m, dt, 700.0, 1.0, fixcm=fixcm, seed=3)
            b.begin(rng.normal(0.0, 1.0, (n, 3)))
            _, g, u = andersen_draws(3, n, 0)
            assert (u <= 1.0).all() and np.array_equal(b.v_replaced, g * np.sqrt(KB * 700.0 / m[:, None]))
        # fixcm: no mass-weighted mean velocity after the correction, the centre of mass stays through the drift
        c = AndersenRef(r, p, m, dt, 700.0, 0.3, fixcm=True, seed=5)
        for _ in range(3):
            com0 = (m[:, None] * c.r).sum(0) / m.sum()
            c.begin(rng.normal(0.0, 1.0, (n, 3)))
            scale = max(np.abs(c.v_replaced).max(), 1e-300)
            assert np.abs((m[:, None] * c.v_drift).sum(0) / m.sum()).max() <= 1e-14 * scale
            assert np.abs((m[:, None] * c.r).sum(0) / m.sum() - com0).max() <= 1e-14 * max(1.0, np.abs(c.r).max())
            c.finish(rng.normal(0.0, 1.0, (n, 3)))
            c.nsteps += 1


def test_andersen_draws_against_the_stream():
    seed = 0xA4093822 | (0x299F31D0 << 32)
    n, t = 5, 7
    com, g, u = andersen_draws(seed, n, t)
    w = stream_words(seed, n, t, PURPOSE_ANDERSEN, 4)
    assert w.shape == (n, 4, 4)
    from tests.md_ref import philox4x32_10

    assert w[3, 2].tolist() == philox4x32_10(np.array([3, 7, 2, 2], dtype=np.uint32), (0xA4093822, 0x299F31D0)).tolist()
    assert np.array_equal(g, normals(seed, n, t, PURPOSE_ANDERSEN, 2)[:, :3])
    assert u[3, 0] == unit_interval(w[3, 2, 0], w[3, 2, 1]) and u[3, 1] == unit_interval(w[3, 2, 2], w[3, 2, 3])
    assert u[3, 2] == unit_interval(w[3, 3, 0], w[3, 3, 1])
    wc = philox4x32_10(np.array([[0, 7, 0, 3], [0, 7, 1, 3]], dtype=np.uint32), (0xA4093822, 0x299F31D0))
    assert np.array_equal(com, box_muller(wc).reshape(4)[:3])
    # the new purposes collide with neither each other nor purposes 0 and 1
    blocks = [stream_words(seed, n, t, purpose, 4) for purpose in (0, 1, 2, 3)]
    for i in range(4):
        for j in range(i + 1, 4):
            assert not (blocks[i] == blocks[j]).all(axis=-1).any()
    # a large sample: the uniforms fill (0, 1], the comparison at the ends of [0, 1]
    _, g, u = andersen_draws(11, 20000, 3)
    assert (u > 0.0).all() and (u <= 1.0).all() and not (u <= 0.0).any() and (u <= 1.0).all()
    assert abs(u.mean() - 0.5) < 5 / np.sqrt(12 * u.size) and abs((u <= 0.1).mean() - 0.1) < 5 * np.sqrt(0.09 / u.size)
    assert abs(g.mean()) < 5 / np.sqrt(g.size) and abs(g.var() - 1.0) < 5 * np.sqrt(2.0 / g.size)
    assert unit_interval(0, 0) > 0.0 and unit_interval(0xFFFFFFFF, 0xFFFFFFFF) <= 1.0  # prob 0: never; prob 1: always


def test_run_md_validates_the_new_arguments_before_touching_a_device():
    assert dynamics.ENSEMBLES["nvt_andersen"] == 3 and dynamics.ENSEMBLES["npt_berendsen"] == 4
    assert {"lattices", "pressure", "volume", "traj_lattices"} <= set(MDResult.__dataclass_fields__)
    res = MDResult(1, 2, 3, 4, 5, 6, 7, 8, 9)  # (the nine fields of the fixed-cell ensembles, positionally)
    assert res.n_evals == 9 and res.lattices is None and res.pressure is None and res.volume is None
    assert res.traj_lattices is None
    assert "alignn_md_step" in _lib.SIGNATURES and "alignn_md_args_sizeof" in _lib.SIGNATURES
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "alignn_hip.h")).read()
    assert "alignn_md_step(" in header and "alignn_md_args_sizeof(" in header
    from alignn_amd.build import build

    build()
    lib = _lib.load()  # (host-only queries: the binding's two argument blocks are the library's)
    assert lib.alignn_md_args_sizeof() == ctypes.sizeof(_lib.MdArgs)
    assert lib.alignn_fire_args_sizeof() == ctypes.sizeof(_lib.FireArgs)
    lat, pos, m = [np.eye(3) * 5, np.eye(3) * 6], [np.zeros((2, 3)), np.ones((3, 3))], [np.ones(2), np.ones(3)]
    ff = lambda lat, pos: None  # noqa: E731
    npt = dict(ensemble="npt_berendsen", pressure=1.0, compressibility=1e-6)
    bad = [
        dict(ensemble="nvt_andersen", andersen_prob=-0.1),
        dict(ensemble="nvt_andersen", andersen_prob=1.5),
        dict(ensemble="nvt_andersen", andersen_prob=float("nan")),
        dict(ensemble="npt"),
        dict(npt, taup=0.001),
        dict(npt, taut=0.001),
        dict(npt, pressure=None),
        dict(npt, compressibility=None),
        dict(npt, pressure=float("inf")),
        dict(npt, pressure=[1.0, 2.0, 3.0]),
        dict(npt, compressibility=-1e-6),
        dict(npt, compressibility=float("nan")),
        dict(npt, compressibility=[1e-6]),
        dict(npt, stress_weight=float("nan")),
    ]
    for kw in bad:
        with pytest.raises(ValueError):
            run_md(None, lat, pos, None, m, forces_fn=ff, **kw)
    # valid arguments get as far as the device: a CPU device is a TypeError, raised after every ValueError check
    for kw in (npt, dict(npt, pressure=[-5.0, 5.0], compressibility=[0.0, 1e-6]), dict(ensemble="nvt_andersen", andersen_prob=0)):
        with pytest.raises(TypeError):
            run_md(None, lat, pos, None, m, forces_fn=ff, device="cpu", **kw)
