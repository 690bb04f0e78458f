"""The executable specification of ``alignn_amd.run_md`` (csrc/dynamics.hip): a float64 numpy restatement of ASE 3.22.1's
``VelocityVerlet``, ``Langevin``, ``NVTBerendsen``, ``MaxwellBoltzmannDistribution`` and of the run loop
(``Dynamics.irun`` with observers every ``interval`` steps), as the reference's ``ForceField.run_nve_velocity_verlet`` /
``run_nvt_langevin`` / ``run_nvt_berendsen`` / ``set_momentum_maxwell_boltzmann`` drive them (alignn/ff/ff.py:360-550).
ASE is not a dependency of this project; the restatement follows the published ase/md/{verlet,langevin,nvtberendsen,
velocitydistribution,md}.py and ase/optimize/optimize.py, and tests/test_md_ref.py pins it to steps computed by hand on a 1-D
harmonic oscillator.  Where a detail of ASE was in doubt when this was written, the project's own statement rules:

- NVTBerendsen compares the target ``T0`` with the current temperature ``T`` both in kelvin;
- Langevin's ``fixcm`` correction removes the plain mean of ``rnd_pos`` and the mass-weighted mean of ``rnd_vel``
  (``(rnd_vel * m).sum(0) / (m * n)``), NVTBerendsen's the plain mean of the momenta.

ASE's numpy random streams are not reproduced.  The random numbers are the project's counter-based stream (``philox4x32_10``,
``normals``), which the kernel draws alike; the GPU tests (test_gpu_dynamics.py) hold the kernel and ``run_md`` to this file."""

import numpy as np

from alignn_amd.dynamics import KB


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
