"""The executable specification of ``alignn_amd.run_md`` (csrc/dynamics.hip): a float64 numpy restatement of ASE 3.22.1's
``VelocityVerlet``, ``Langevin``, ``NVTBerendsen``, ``MaxwellBoltzmannDistribution`` and of the run loop
(``Dynamics.irun`` with observers every ``interval`` steps), as the reference's ``ForceField.run_nve_velocity_verlet`` /
``run_nvt_langevin`` / ``run_nvt_berendsen`` / ``set_momentum_maxwell_boltzmann`` drive them (alignn/ff/ff.py:360-550).
ASE is not a dependency of this project; the restatement follows the published ase/md/{verlet,langevin,nvtberendsen,
velocitydistribution,md}.py and ase/optimize/optimize.py, and the checks below pin it to steps computed by hand on a 1-D
harmonic oscillator.  Where a detail of ASE was in doubt when this was written, the project's own statement rules:

- NVTBerendsen compares the target ``T0`` with the current temperature ``T`` both in kelvin;
- Langevin's ``fixcm`` correction removes the plain mean of ``rnd_pos`` and the mass-weighted mean of ``rnd_vel``
  (``(rnd_vel * m).sum(0) / (m * n)``), NVTBerendsen's the plain mean of the momenta.

ASE's numpy random streams are not reproduced.  The random numbers are the project's counter-based stream (``philox4x32_10``,
``normals``), which the kernel draws alike; the GPU tests (test_gpu_dynamics.py) hold the kernel and ``run_md`` to this file."""

import numpy as np
import pytest

from alignn_amd import dynamics
from alignn_amd.dynamics import FS, KB, MDResult, berendsen_taut, run_md  # the batched integrator this file specifies

# ---- the project's random stream -----------------------------------------------------------------------------------------
M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
PURPOSE_LANGEVIN, PURPOSE_MOMENTA = 0, 1
MASK = np.uint64(0xFFFFFFFF)


def philox4x32_10(ctr, key):
    """Philox4x32-10 of counters ``ctr`` [..., 4] under ``key`` (k0, k1) (each uint32 or an array broadcasting against ctr's
    leading shape) -> [..., 4] uint32 words."""
    c = [np.asarray(ctr, dtype=np.uint64)[..., i] for i in range(4)]
    k0 = np.asarray(key[0], dtype=np.uint64) & MASK
    k1 = np.asarray(key[1], dtype=np.uint64) & MASK
    for r in range(10):
        if r:
            k0 = (k0 + np.uint64(W0)) & MASK
            k1 = (k1 + np.uint64(W1)) & MASK
        p0 = np.uint64(M0) * c[0]
        p1 = np.uint64(M1) * c[2]
        c = [((p1 >> np.uint64(32)) ^ c[1] ^ k0) & MASK, p1 & MASK, ((p0 >> np.uint64(32)) ^ c[3] ^ k1) & MASK, p0 & MASK]
    return np.stack(c, axis=-1).astype(np.uint32)


def unit_interval(a, b):
    """53 bits of two words as a double in (0, 1]: ((a >> 5) 2^26 + (b >> 6) + 0.5) 2^-53, evaluated left to right."""
    a = (np.asarray(a, dtype=np.uint64) >> np.uint64(5)).astype(np.float64)
    b = (np.asarray(b, dtype=np.uint64) >> np.uint64(6)).astype(np.float64)
    return (a * 67108864.0 + b + 0.5) * 2.0 ** -53


def box_muller(words):
    """[..., 4] words -> [..., 2] normals: sqrt(-2 ln u1) (cos, sin)(2 pi u2)."""
    u1, u2 = unit_interval(words[..., 0], words[..., 1]), unit_interval(words[..., 2], words[..., 3])
    rad, th = np.sqrt(-2.0 * np.log(u1)), 2.0 * np.pi * u2
    return np.stack([rad * np.cos(th), rad * np.sin(th)], axis=-1)


def stream_words(seed, n, t, purpose, blocks):
    """The Philox words of atoms 0..n-1 at counter (atom, t, j, purpose), j < blocks -> [n, blocks, 4]."""
    i = np.arange(n, dtype=np.uint64)[:, None]
    j = np.arange(blocks, dtype=np.uint64)[None, :]
    ctr = np.stack(np.broadcast_arrays(i, np.uint64(t), j, np.uint64(purpose)), axis=-1)
    return philox4x32_10(ctr, (seed & 0xFFFFFFFF, seed >> 32))


def normals(seed, n, t, purpose, blocks):
    """[n, 2 * blocks] normals, in block order, cos before sin within a block."""
    return box_muller(stream_words(seed, n, t, purpose, blocks)).reshape(n, 2 * blocks)


def langevin_noise(seed, n, t):
    """xi, eta [n, 3] of the Langevin step that starts at iteration t."""
    g = normals(seed, n, t, PURPOSE_LANGEVIN, 3)
    return g[:, :3], g[:, 3:]


def maxwell_boltzmann(seed, m, temperature_K):
    """MaxwellBoltzmannDistribution(temperature_K), no Stationary: p = xi sqrt(m kB T)."""
    xi = normals(seed, len(m), 0, PURPOSE_MOMENTA, 2)[:, :3]
    return xi * np.sqrt(np.asarray(m, dtype=np.float64) * (KB * temperature_K))[:, None]


# ---- the integrators ------------------------------------------------------------------------------------------------------
def kinetic_energy(p, m):
    return 0.5 * float((p * p / m[:, None]).sum())


def temperature(p, m):
    """Atoms.get_temperature: 3N degrees of freedom, nothing removed for fixcm."""
    return 2.0 * kinetic_energy(p, m) / (3 * len(m) * KB)


class VerletRef:
    """ase/md/verlet.py VelocityVerlet.step.  ``dt`` in ASE time units.  ``begin(f)``: first half-kick and drift; ``finish(f)``:
    the second half-kick with the forces of the new positions (the two halves are kept apart, not folded into one kick)."""

    def __init__(self, r, p, m, dt):
        self.r, self.p = np.array(r, dtype=np.float64), np.array(p, dtype=np.float64)
        self.m, self.dt, self.nsteps = np.asarray(m, dtype=np.float64), dt, 0

    def begin(self, f):
        self.p = self.p + 0.5 * self.dt * f
        self.r = self.r + self.dt * self.p / self.m[:, None]

    def finish(self, f):
        self.p = self.p + 0.5 * self.dt * f

    def step(self, f, ef):
        """One ASE step from forces ``f`` of the current positions -> (e, f) of the new ones."""
        self.begin(f)
        e, f = ef(self.r)
        self.finish(f)
        self.nsteps += 1
        return e, f


def berendsen_scale(T0, T, dt, taut):
    """NVTBerendsen.scale_velocities' factor, T0 and T in kelvin.  T == 0 gives 1.1 (T0 / T = +inf) and no NaN."""
    if T == 0.0:
        return 1.1
    return float(np.clip(np.sqrt(1.0 + (T0 / T - 1.0) * dt / taut), 0.9, 1.1))


class BerendsenRef(VerletRef):
    """ase/md/nvtberendsen.py NVTBerendsen.step: the velocity scaling, the first half-kick, fixcm (the plain mean of the momenta),
    the drift; the second half-kick after the evaluation."""

    def __init__(self, r, p, m, dt, T0, taut, fixcm=True):
        super().__init__(r, p, m, dt)
        self.T0, self.taut, self.fixcm = T0, taut, fixcm

    def begin(self, f):
        self.p = berendsen_scale(self.T0, temperature(self.p, self.m), self.dt, self.taut) * self.p
        p = self.p + 0.5 * self.dt * f
        if self.fixcm:
            p = p - p.sum(axis=0) / float(len(p))
        self.r = self.r + self.dt * p / self.m[:, None]
        self.p = p


class LangevinRef(VerletRef):
    """ase/md/langevin.py Langevin (updatevars / step); ``T`` = kB T0 in eV, ``fr`` the friction.  The noise of the step that
    starts at iteration t = ``nsteps`` comes from ``langevin_noise(seed, n, t)`` unless ``begin`` gets it."""

    def __init__(self, r, p, m, dt, T0, friction, fixcm=True, seed=0):
        super().__init__(r, p, m, dt)
        self.fixcm, self.seed, self.fr = fixcm, seed, friction
        T, fr = KB * T0, friction
        sigma = np.sqrt(2 * T * fr / self.m)[:, None]
        self.c1 = dt / 2.0 - dt * dt * fr / 8.0
        self.c2 = dt * fr / 2 - dt * dt * fr * fr / 8.0
        self.c3 = np.sqrt(dt) * sigma / 2.0 - dt ** 1.5 * fr * sigma / 8.0
        self.c5 = dt ** 1.5 * sigma / (2 * np.sqrt(3))
        self.c4 = fr / 2.0 * self.c5
        self.v = self.rnd_vel = None

    def begin(self, f, xi=None, eta=None):
        n, m = len(self.m), self.m[:, None]
        if xi is None:
            xi, eta = langevin_noise(self.seed, n, self.nsteps)
        self.v = self.p / m
        self.rnd_pos = self.c5 * eta
        self.rnd_vel = self.c3 * xi - self.c4 * eta
        if self.fixcm:
            self.rnd_pos = self.rnd_pos - self.rnd_pos.sum(axis=0) / n
            self.rnd_vel = self.rnd_vel - (self.rnd_vel * m).sum(axis=0) / (m * n)
        self.v = self.v + (self.c1 * f / m - self.c2 * self.v + self.rnd_vel)
        x = self.r
        self.r = x + self.dt * self.v + self.rnd_pos
        self.v = (self.r - x - self.rnd_pos) / self.dt

    def finish(self, f):
        m = self.m[:, None]
        self.v = self.v + (self.c1 * f / m - self.c2 * self.v + self.rnd_vel)
        self.p = self.v * m


def run_ref(integ, ef, steps, interval=1):
    """Dynamics.irun(steps) with one observer every ``interval`` steps: evaluate, record frame 0, then step and record after
    step k when k % interval == 0.  ``ef(r) -> (e, f)``.  -> dict(frames: [(step, r, p, e_pot, e_kin)], n_evals, f)."""
    e, f = ef(integ.r)
    n_evals = 1
    frames = [(0, integ.r.copy(), integ.p.copy(), e, kinetic_energy(integ.p, integ.m))]
    for k in range(1, steps + 1):
        e, f = integ.step(f, ef)
        n_evals += 1
        if k % interval == 0:
            frames.append((k, integ.r.copy(), integ.p.copy(), e, kinetic_energy(integ.p, integ.m)))
    return dict(frames=frames, n_evals=n_evals, f=f)


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
