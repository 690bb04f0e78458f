"""Checks of tests/md_ref.py, the float64 numpy restatement of ASE 3.22.1's ``VelocityVerlet``, ``Langevin``, ``NVTBerendsen``,
``MaxwellBoltzmannDistribution`` and run loop that specifies ``alignn_amd.run_md`` (csrc/dynamics.hip), and of the project's
counter-based random stream: steps computed by hand on a 1-D harmonic oscillator, known answers of Philox4x32-10, and what the
entry point refuses before it touches a device.  The GPU tests (test_gpu_dynamics.py) hold the kernel and ``run_md`` to the
restatement."""

import numpy as np
import pytest

from alignn_amd import dynamics
from alignn_amd.dynamics import FS, KB, MDResult, berendsen_taut, run_md  # the batched integrator the restatement specifies
from tests.md_ref import (PURPOSE_LANGEVIN, PURPOSE_MOMENTA, BerendsenRef, LangevinRef, VerletRef, berendsen_scale,
                          kinetic_energy, langevin_noise, maxwell_boltzmann, normals, philox4x32_10, run_ref, stream_words, temperature,
                          unit_interval)


def oscillator(k):
    """1-D harmonic oscillator along x: E = k x^2 / 2, F = -k x."""

    def ef(r):
        f = np.zeros_like(r)
        f[:, 0] = -k * r[:, 0]
        return 0.5 * k * float(r[:, 0] @ r[:, 0]), f

    return ef


X0 = np.array([[1.0, 0.0, 0.0]])


# ---- the checks -----------------------------------------------------------------------------------------------------------
def test_units_and_taut_default():
    assert FS == 0.09822694788464063 and KB == 8.617330337217213e-05
    # CODATA 2014: e = 1.6021766208e-19 C, amu = 1.660539040e-27 kg, k = 1.38064852e-23 J/K
    e, amu = 1.6021766208e-19, 1.660539040e-27
    assert FS == pytest.approx(1e-15 * np.sqrt(e / amu) * 1e10, rel=1e-15)
    assert KB == pytest.approx(1.38064852e-23 / e, rel=1e-15)
    assert 500 * FS == pytest.approx(49.11347394232032, rel=1e-15)  # ff.py's NPTBerendsen taut
    assert 1.0 / (1e9 / (e * 1e30)) == pytest.approx(160.21766208, rel=1e-15)  # relax.py's eV/A^3 per GPa
    assert berendsen_taut(None, 0.5) == 100 * 0.5 * FS and berendsen_taut(500.0, 0.5) == 500.0 * FS


def test_velocity_verlet_by_hand():
    m = np.array([2.0])
    vv = VerletRef(X0, np.zeros((1, 3)), m, 0.1)
    ef = oscillator(1.0)
    vv.begin(ef(vv.r)[1])  # F = -1: p = -0.05, x = 1 + 0.1 (-0.05) / 2 = 0.9975
    assert vv.p[0, 0] == pytest.approx(-0.05, abs=1e-16) and vv.r[0, 0] == pytest.approx(0.9975, abs=1e-16)
    vv.finish(ef(vv.r)[1])  # F = -0.9975: p = -0.05 - 0.049875
    assert vv.p[0, 0] == pytest.approx(-0.099875, abs=1e-16)
    assert (vv.p[0, 1:] == 0).all() and (vv.r[0, 1:] == 0).all()
    # the step form gives the same and counts
    vv2 = VerletRef(X0, np.zeros((1, 3)), m, 0.1)
    e, f = vv2.step(ef(vv2.r)[1], ef)
    assert vv2.nsteps == 1 and np.array_equal(vv2.p, vv.p) and f[0, 0] == -vv2.r[0, 0] and e == 0.5 * vv2.r[0, 0] ** 2


def test_nve_conserves_energy_at_second_order():
    ef, m = oscillator(1.0), np.array([1.0])

    def spread(dt, steps):
        res = run_ref(VerletRef(X0, np.zeros((1, 3)), m, dt), ef, steps)
        etot = np.array([fr[3] + fr[4] for fr in res["frames"]])
        return etot.max() - etot.min()

    a, b = spread(0.1, 200), spread(0.05, 400)
    assert a < 2e-3 and 3.9 < a / b < 4.1


def test_frame_schedule():
    ef = oscillator(1.0)
    for steps, interval in [(7, 3), (6, 3), (0, 1), (5, 1), (4, 10)]:
        res = run_ref(VerletRef(X0, np.zeros((1, 3)), np.array([1.0]), 0.1), ef, steps, interval)
        assert len(res["frames"]) == 1 + steps // interval and res["n_evals"] == steps + 1
        assert [fr[0] for fr in res["frames"]] == list(range(0, steps + 1, interval))


def test_berendsen_scale_and_clip():
    T = 300.0
    assert berendsen_scale(4 * T, T, 0.01, 1.0) == pytest.approx(np.sqrt(1.03), rel=1e-15)
    assert berendsen_scale(100 * T, T, 1.0, 1.0) == 1.1  # sqrt(100) clips to the upper bound
    assert berendsen_scale(0.0, T, 0.5, 1.0) == 0.9  # sqrt(0.5) clips to the lower bound
    assert berendsen_scale(300.0, 0.0, 0.01, 1.0) == 1.1 and berendsen_scale(0.0, 0.0, 0.01, 1.0) == 1.1


def test_berendsen_by_hand():
    m, dt, taut = np.array([2.0]), 0.1, 10.0
    p0 = np.array([[0.3, 0.0, 0.0]])
    T = 2 * (0.5 * 0.09 / 2.0) / (3 * KB)
    assert temperature(p0, m) == pytest.approx(T, rel=1e-15)
    b = BerendsenRef(X0, p0, m, dt, T0=4 * T, taut=taut, fixcm=False)
    ef = oscillator(1.0)
    b.begin(ef(b.r)[1])  # scale sqrt(1 + 3 * 0.01), then p += 0.05 * -1, x += 0.1 p / 2
    p = 0.3 * np.sqrt(1.03) - 0.05
    assert b.p[0, 0] == pytest.approx(p, rel=1e-15) and b.r[0, 0] == pytest.approx(1.0 + 0.05 * p, rel=1e-15)
    b.finish(ef(b.r)[1])
    assert b.p[0, 0] == pytest.approx(p - 0.05 * (1.0 + 0.05 * p), rel=1e-15)
    # fixcm: the plain (not mass-weighted) mean of the momenta after the half-kick is removed
    two = BerendsenRef(np.zeros((2, 3)), np.array([[1.0, 0, 0], [0.0, 0, 0]]), np.array([1.0, 3.0]), dt, T0=0.0, taut=taut)
    two.begin(np.array([[0.0, 2.0, 0.0], [0.0, 0.0, 0.0]]))
    s = np.sqrt(1.0 - 0.01)
    want = np.array([[s, 0.1, 0.0], [0.0, 0.0, 0.0]])
    want -= want.mean(axis=0)
    assert np.allclose(two.p, want, rtol=0, atol=1e-15) and np.allclose(two.p.sum(axis=0), 0.0, atol=1e-16)
    assert np.allclose(two.r, dt * want / np.array([[1.0], [3.0]]), rtol=0, atol=1e-16)


def test_langevin_by_hand():
    dt, fr, T0 = 0.1, 0.2, 0.5 / KB  # kB T = 0.5 eV, m = 1: sigma = sqrt(0.2)
    lv = LangevinRef(X0, np.zeros((1, 3)), np.array([1.0]), dt, T0, fr, fixcm=False)
    c1, c2 = 0.05 - 0.01 * 0.2 / 8, 0.01 - 0.01 * 0.04 / 8  # 0.04975, 0.00995
    c5 = np.sqrt(0.001 * 0.2 / 12.0)
    c3 = np.sqrt(0.02) * (0.5 - 0.2 * 0.1 / 8)
    c4 = 0.1 * c5
    assert (lv.c1, lv.c2) == pytest.approx((c1, c2), rel=1e-14)
    assert lv.c3[0, 0] == pytest.approx(c3, rel=1e-14) and lv.c5[0, 0] == pytest.approx(c5, rel=1e-14)
    assert lv.c4[0, 0] == pytest.approx(c4, rel=1e-14)
    xi, eta = np.array([[0.5, 0.0, 0.0]]), np.array([[-1.0, 0.0, 0.0]])
    ef = oscillator(1.0)
    lv.begin(ef(lv.r)[1], xi, eta)
    rnd_pos, rnd_vel = -c5, 0.5 * c3 + c4
    v = -c1 + rnd_vel  # v0 = 0, F = -1
    x1 = 1.0 + dt * v + rnd_pos
    assert lv.r[0, 0] == pytest.approx(x1, rel=1e-15) and lv.v[0, 0] == pytest.approx(v, rel=1e-12)
    lv.finish(ef(lv.r)[1])
    assert lv.p[0, 0] == pytest.approx(v + (-c1 * x1 - c2 * v + rnd_vel), rel=1e-12)
    assert (lv.p[0, 1:] == 0).all()
    # the next step starts from v = p / m and draws its own noise
    lv.begin(ef(lv.r)[1], np.zeros((1, 3)), np.zeros((1, 3)))
    assert lv.rnd_vel[0, 0] == 0.0


def test_langevin_fixcm_keeps_the_momentum_sum():
    m = np.array([1.0, 4.0, 12.0, 7.0])
    lv = LangevinRef(np.zeros((4, 3)), np.zeros((4, 3)), m, 0.1, 1000.0, 0.3, fixcm=True, seed=5)
    zero = np.zeros((4, 3))
    for _ in range(5):
        lv.begin(zero)
        assert np.abs((lv.rnd_vel * m[:, None]).sum(axis=0)).max() < 1e-15
        assert np.abs(lv.rnd_pos.sum(axis=0)).max() < 1e-15
        lv.finish(zero)
        lv.nsteps += 1
        assert np.abs(lv.p.sum(axis=0)).max() < 1e-14
    assert np.abs(lv.p).max() > 1e-3  # (the noise did act)


def test_philox_known_answers():
    kat = [((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
           ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
           ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0),
            (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1))]
    for ctr, key, want in kat:
        assert philox4x32_10(np.array(ctr, dtype=np.uint32), key).tolist() == list(want)
    # the stream: key = (seed low word, seed high word), counter (atom, t, block, purpose)
    seed = 0xA4093822 | (0x299F31D0 << 32)
    w = stream_words(seed, 3, 7, PURPOSE_LANGEVIN, 3)
    assert w[2, 1].tolist() == philox4x32_10(np.array([2, 7, 1, 0], dtype=np.uint32), (0xA4093822, 0x299F31D0)).tolist()


def test_unit_interval_and_normals():
    assert unit_interval(0, 0) == 0.5 * 2.0 ** -53 > 0.0
    assert unit_interval(0xFFFFFFFF, 0xFFFFFFFF) <= 1.0
    assert unit_interval(0x80000000, 0) == 0.5
    g = normals(123, 20000, 0, PURPOSE_LANGEVIN, 3)
    assert g.shape == (20000, 6) and np.isfinite(g).all()
    assert abs(g.mean()) < 5 / np.sqrt(g.size) and abs(g.var() - 1.0) < 5 * np.sqrt(2.0 / g.size)
    xi, eta = langevin_noise(123, 20000, 0)
    assert np.array_equal(xi, g[:, :3]) and np.array_equal(eta, g[:, 3:])
    # streams of different seeds, steps and purposes differ
    assert not np.array_equal(normals(124, 4, 0, 0, 1), normals(123, 4, 0, 0, 1))
    assert not np.array_equal(normals(123, 4, 1, 0, 1), normals(123, 4, 0, 0, 1))
    assert not np.array_equal(normals(123, 4, 0, 1, 1), normals(123, 4, 0, 0, 1))


def test_maxwell_boltzmann():
    m = np.full(30000, 12.0)
    p = maxwell_boltzmann(9, m, 500.0)
    ke, want = kinetic_energy(p, m), 1.5 * len(m) * KB * 500.0
    assert abs(ke - want) < 5 * np.sqrt(1.5 * len(m)) * KB * 500.0
    xi = normals(9, 30000, 0, PURPOSE_MOMENTA, 2)[:, :3]
    assert np.array_equal(p, xi * np.sqrt(m * (KB * 500.0))[:, None])


def test_run_md_validates_before_touching_a_device():
    import alignn_amd

    assert alignn_amd.run_md is run_md and dynamics.run_md is run_md
    assert set(MDResult.__dataclass_fields__) >= {"epot", "ekin", "temperature", "traj_positions", "traj_momenta", "positions",
                                                  "momenta", "forces", "n_evals"}
    lat, pos, m = [np.eye(3) * 5], [np.zeros((2, 3))], [np.ones(2)]
    ff = lambda lat, pos: None  # noqa: E731
    bad = [
        dict(lattices=lat, positions=pos + pos, masses=m),
        dict(masses=[np.ones(3)]),
        dict(masses=[np.array([1.0, 0.0])]),
        dict(masses=[np.array([1.0, np.nan])]),
        dict(positions=[np.zeros((2, 2))]),
        dict(ensemble="npt"),
        dict(timestep=0.0),
        dict(steps=-1),
        dict(interval=0),
        dict(temperature_K=[300.0, 300.0]),
        dict(temperature_K=-1.0),
        dict(friction=-1.0),
        dict(ensemble="nvt_berendsen", taut=0.001),
        dict(initial_temperature_K=300.0, momenta=[np.zeros((2, 3))]),
        dict(momenta=[np.zeros((3, 3))]),
        dict(seed=-1),
        dict(seed=[1, 2]),
        dict(seed=2 ** 64),
    ]
    for kw in bad:
        args = dict(lattices=lat, positions=pos, masses=m)
        args.update(kw)
        with pytest.raises(ValueError):
            run_md(None, args.pop("lattices"), args.pop("positions"), None, args.pop("masses"), forces_fn=ff, **args)
    with pytest.raises(TypeError):
        run_md(object(), lat, pos, [np.zeros((2, 92))], m)
