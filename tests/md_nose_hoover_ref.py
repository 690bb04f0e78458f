"""The executable specification of the ``nvt_nose_hoover`` and ``npt_nose_hoover`` ensembles of ``alignn_amd.run_md``
(csrc/dynamics.hip, ``alignn_md_step`` with ensembles 5 and 6): a float64 numpy restatement of Nose-Hoover chains and of the
isotropic MTK barostat in the explicit reversible form of Martyna, Tuckerman, Tobias and Klein (Mol. Phys. 87, 1117, 1996), the
barostat measure-preserving (Tuckerman et al., J. Phys. A 39, 5629, 2006).  This is not ASE's ``NPT``: the reference's
``run_npt_nose_hoover`` calls that class with neither ``ttime`` nor ``pfactor``, which is ``ttime=None, ptime=None`` here - plain
velocity Verlet.

Per structure, in ASE units: ``kT = kB T0``, ``g = 3N``, ``Q_0 = g kT tau^2``, ``Q_k = kT tau^2``, ``W = (g + 3) kT tau_p^2``, the
barostat's own chain ``Q'_k = kT tau_p^2`` with one degree of freedom, ``alpha = 1 + 3 / g``.  One step, T = thermostat on,
B = barostat on:

1. B and T: ``v_eps *= nhc_half(W v_eps^2, 1, Q', v', eta')``; T: ``p *= nhc_half(sum p^2/m, g, Q, v, eta)``
2. B: ``v_eps += dt/2 G_eps``, ``G_eps = (alpha sum p^2/m + 3 V (P_vir - P_ext)) / W``, ``P_vir = -tr(stress) / 3``
3. B: ``p = p exp(-alpha v_eps dt/2) + dt/2 F exp(-alpha v_eps dt/4) sinhc(alpha v_eps dt/4)``; else ``p += dt/2 F``
4. B: ``r = r exp(v_eps dt) + dt p/m exp(v_eps dt/2) sinhc(v_eps dt/2)``, ``cell *= exp(v_eps dt)``; else ``r += dt p/m``
5. evaluate; 6. = 3. with the new forces; 7. = 2. with the new momenta, cell and stress; 8. = 1. in the opposite order.

``begin`` is 1-4, ``finish`` 6-8, as the kernel's launches split a step.  tests/test_md_nose_hoover_ref.py pins the restatement
by what does not come from the kernel: second-order conservation of H', time reversal, a step by hand, its limits and the
barostat's targets.  The GPU tests (test_gpu_dynamics_nose_hoover.py) hold the kernel and ``run_md`` to this file."""

import numpy as np

from alignn_amd.dynamics import BAR, FS, KB
from alignn_amd.synthetic import make_crystal
from tests.md_npt_ref import pressure_of
from tests.md_ref import VerletRef, kinetic_energy, maxwell_boltzmann
from tests.springs_ref import spring_list, springs_efs


# ---- the integrators ------------------------------------------------------------------------------------------------------
def sy_weights(order):
    """The Suzuki-Yoshida weights of order 1, 3 or 5."""
    if order == 1:
        return [1.0]
    if order == 3:
        w = 1.0 / (2.0 - 2.0 ** (1.0 / 3.0))
        return [w, 1.0 - 2.0 * w, w]
    if order == 5:
        w = 1.0 / (4.0 - 4.0 ** (1.0 / 3.0))
        return [w, w, 1.0 - 4.0 * w, w, w]
    raise ValueError(order)


def sinhc(x):
    """sinh(x) / x, by its series below |x| = 1e-2."""
    x2 = x * x
    if abs(x) < 1e-2:
        return 1.0 + x2 / 6.0 + x2 * x2 / 120.0 + x2 * x2 * x2 / 5040.0 + x2 * x2 * x2 * x2 / 362880.0
    return np.sinh(x) / x


def nhc_half(K2, dof, kT, Q, v, eta, dt, loops=1, order=3, second_exp=True):
    """A chain (masses ``Q``, velocities ``v``, positions ``eta``, all [M], the last two updated in place) by ``dt / 2``; ``K2`` is
    ``sum p^2 / m`` of what it thermostats.  -> the factor on those momenta.  (``second_exp=False`` is the unsymmetric
    factorisation that the reversal check below tells apart.)"""
    M, s = len(Q), 1.0

    def G(k):
        return (K2 * s * s - dof * kT) / Q[0] if k == 0 else (Q[k - 1] * v[k - 1] * v[k - 1] - kT) / Q[k]

    def link(k, h):
        e = np.exp(-0.25 * h * v[k + 1])
        v[k] *= e
        v[k] += 0.5 * h * G(k)
        if second_exp:
            v[k] *= e

    for _ in range(loops):
        for w in sy_weights(order):
            h = w * (0.5 * dt) / loops
            v[M - 1] += 0.5 * h * G(M - 1)
            for k in range(M - 2, -1, -1):
                link(k, h)
            s *= np.exp(-h * v[0])
            eta += h * v
            for k in range(M - 1):
                link(k, h)
            v[M - 1] += 0.5 * h * G(M - 1)
    return s


def sum_p2_over_m(p, m):
    return float((p * p / m[:, None]).sum())


def remove_com(p, m):
    """``fixcm`` of the two ensembles, once, on the start momenta: p_i -= m_i sum p / sum m."""
    return p - m[:, None] * p.sum(axis=0) / m.sum()


class NoseHooverChainRef(VerletRef):
    """NVT: velocity Verlet between two half steps of the particles' chain.  ``dt`` and ``ttime`` in ASE time units."""

    def __init__(self, r, p, m, dt, T0, ttime, chain=3, loops=1, order=3, fixcm=False):
        super().__init__(r, p, m, dt)
        if fixcm:
            self.p = remove_com(self.p, self.m)
        self.kT, self.g, self.loops, self.order = KB * T0, 3.0 * len(self.m), loops, order
        self.Q = np.full(chain, self.kT * ttime * ttime)
        self.Q[0] = self.g * self.kT * ttime * ttime
        self.v, self.eta = np.zeros(chain), np.zeros(chain)

    def thermostat(self):
        s = nhc_half(sum_p2_over_m(self.p, self.m), self.g, self.kT, self.Q, self.v, self.eta, self.dt, self.loops, self.order)
        self.p = s * self.p

    def begin(self, f, stress=None):
        self.thermostat()
        super().begin(f)

    def finish(self, f, stress=None):
        super().finish(f)
        self.thermostat()

    def conserved(self, e):
        H = kinetic_energy(self.p, self.m) + e
        H += 0.5 * float((self.Q * self.v * self.v).sum()) + self.g * self.kT * self.eta[0] + self.kT * float(self.eta[1:].sum())
        return H

    def state(self):
        """The 34 doubles of ``alignn_md_args.nhc_state``."""
        out = np.zeros(34)
        out[:len(self.eta)], out[8:8 + len(self.v)] = self.eta, self.v
        return out


class MTKRef(VerletRef):
    """Isotropic MTK NPT.  ``ttime`` / ``ptime`` None: no thermostat / no barostat.  ``pressure`` in eV/A^3; ``begin`` and
    ``finish`` take the forces and the stress of the last evaluation (``second_exp=False``: the factorisation that the
    reversal check tells apart)."""

    def __init__(self, r, p, m, dt, T0, ttime, ptime, cell, pressure=0.0, chain=3, loops=1, order=3, fixcm=False,
                 second_exp=True):
        super().__init__(r, p, m, dt)
        if fixcm:
            self.p = remove_com(self.p, self.m)
        self.T, self.B = ttime is not None, ptime is not None
        self.kT, self.g, self.loops, self.order, self.second_exp = KB * T0, 3.0 * len(self.m), loops, order, second_exp
        self.alpha = 1.0 + 3.0 / self.g
        self.cell, self.pressure = np.array(cell, dtype=np.float64), pressure
        self.v, self.eta, self.vb, self.etab = (np.zeros(chain) for _ in range(4))
        self.eps = self.veps = 0.0
        if self.T:
            self.Q = np.full(chain, self.kT * ttime * ttime)
            self.Q[0] = self.g * self.kT * ttime * ttime
        if self.B:
            self.W = (self.g + 3.0) * self.kT * ptime * ptime
            self.Qb = np.full(chain, self.kT * ptime * ptime)

    def volume(self):
        return abs(np.linalg.det(self.cell))

    def chain_particles(self):
        s = nhc_half(sum_p2_over_m(self.p, self.m), self.g, self.kT, self.Q, self.v, self.eta, self.dt, self.loops, self.order,
                     self.second_exp)
        self.p = s * self.p

    def chain_barostat(self):
        self.veps *= nhc_half(self.W * self.veps * self.veps, 1.0, self.kT, self.Qb, self.vb, self.etab, self.dt, self.loops,
                              self.order, self.second_exp)

    def kick_eps(self, stress):
        virial = -(stress[0, 0] + stress[1, 1] + stress[2, 2]) / 3.0
        G = (self.alpha * sum_p2_over_m(self.p, self.m) + 3.0 * self.volume() * (virial - self.pressure)) / self.W
        self.veps += 0.5 * self.dt * G

    def kick(self, f):
        if self.B:
            x = self.alpha * self.veps * 0.25 * self.dt
            self.p = self.p * np.exp(-self.alpha * self.veps * (0.5 * self.dt)) + 0.5 * self.dt * f * (np.exp(-x) * sinhc(x))
        else:
            self.p = self.p + 0.5 * self.dt * f

    def begin(self, f, stress=None):
        if self.T:
            if self.B:
                self.chain_barostat()
            self.chain_particles()
        if self.B:
            self.kick_eps(stress)
        self.kick(f)
        if self.B:
            y = self.veps * (0.5 * self.dt)
            er = np.exp(self.veps * self.dt)
            self.r = self.r * er + self.dt * (self.p / self.m[:, None]) * (np.exp(y) * sinhc(y))
            self.cell = er * self.cell
            self.eps += self.veps * self.dt
        else:
            self.r = self.r + self.dt * self.p / self.m[:, None]

    def finish(self, f, stress=None):
        self.kick(f)
        if self.B:
            self.kick_eps(stress)
        if self.T:
            self.chain_particles()
            if self.B:
                self.chain_barostat()

    def conserved(self, e):
        H = kinetic_energy(self.p, self.m) + e
        if self.T:
            H += 0.5 * float((self.Q * self.v * self.v).sum()) + self.g * self.kT * self.eta[0] + self.kT * float(self.eta[1:].sum())
        if self.B:
            H += self.pressure * self.volume() + 0.5 * self.W * self.veps * self.veps
        if self.B and self.T:
            H += 0.5 * float((self.Qb * self.vb * self.vb).sum()) + self.kT * float(self.etab.sum())
        return H

    def state(self):
        out = np.zeros(34)
        M = len(self.eta)
        out[:M], out[8:8 + M], out[16:16 + M], out[24:24 + M], out[32], out[33] = self.eta, self.v, self.etab, self.vb, self.eps, self.veps
        return out

    def reverse(self):
        """Time reversal: every velocity of the extended system changes sign."""
        self.p, self.v, self.vb, self.veps = -self.p, -self.v, -self.vb, -self.veps


def run_nh_ref(integ, efs, steps, interval=1, cell=None):
    """md_ref.run_ref for the two classes above: ``efs(cell, r) -> (e, f, stress)``; frames (step, r, p, e_pot, e_kin, cell,
    P, V, H') with P = -tr(stress) / 3 + 2 KE / (3 V) of the recorded state."""

    def cell_now():
        return integ.cell if hasattr(integ, "cell") else cell

    def frame(k, e, stress):
        c = cell_now()
        return (k, integ.r.copy(), integ.p.copy(), e, kinetic_energy(integ.p, integ.m), np.array(c),
                pressure_of(integ.p, integ.m, stress, c), abs(np.linalg.det(c)), integ.conserved(e))

    e, f, stress = efs(cell_now(), integ.r)
    frames = [frame(0, e, stress)]
    for k in range(1, steps + 1):
        integ.begin(f, stress)
        e, f, stress = efs(cell_now(), integ.r)
        integ.finish(f, stress)
        integ.nsteps += 1
        if k % interval == 0:
            frames.append(frame(k, e, stress))
    return dict(frames=frames, n_evals=steps + 1, f=f, stress=stress)


# ---- spring crystals -------------------------------------------------------------------------------------------------------
def spring_case(n=8, seed=40, T=300.0, strain=1.0, nnb=8):
    """A crystal at rest in its springs, its cell and positions scaled by ``strain``, Maxwell-Boltzmann momenta at ``T``."""
    lat, frac, _ = make_crystal(n, seed)
    efs = springs_efs(*spring_list(lat, frac, nnb=nnb))
    m = np.random.default_rng(seed).uniform(10.0, 60.0, n)
    return strain * lat, frac @ (strain * lat), maxwell_boltzmann(seed, m, T), m, efs


# The barostat.  An MTK piston is an oscillator, and what damps it is its own thermostat: dv'_0/dt = (W v_eps^2 - kT) / Q'_0 =
# (g + 3) v_eps^2 - 1 / ptime^2, so the friction v'_0 grows with the piston's kinetic energy, and the amplitude falls as
# exp(-c t^2).  Two choices make that fast enough for a short run.  chain = 1: a second link holds Q' v'_0^2 near kT, which is
# v'_0 ~ 1 / ptime, no friction to speak of.  A start 3 % off in length: the crystals at rest in their springs (bulk modulus
# ~2e6 bar) are only ~1 % off the volumes that the targets ask for, and from there v_eps is so small that the friction needs
# ~800 steps for its first e-fold; 9 % in volume gives ~9 times the v_eps.  The piston's mass W = (g + 3) kT ptime^2 is set by
# kT: at T0 = 0.1 K, ptime = 8000 fs gives the period (~20 fs) that ptime ~ 150 fs gives at 300 K, and the thermal breathing
# that is left, W v_eps^2 ~ kT, is sqrt(kT B / V) ~ 0.05 rungs at the most.  -tr(stress) / 3 + 2 KE / (3 V) differs from what
# the barostat balances, alpha 2 KE / (3 V) - tr(stress) / 3, by 2 KE / (g V) = kB T / V, ~0.1 bar at T0.
# Measured on this restatement: second-half |mean P - P_target| / rung spacing 1.4e-5, 1.1e-8, 3.6e-6, 3.1e-6, and at most
# 2.3e-4 over ptime sqrt(T0) = 2000 ... 3000 fs K^1/2, T0 = 0.01 ... 1 K, a start 2 % off or 3 % the other way.
LADDER_BAR = np.array([-20000.0, -10000.0, 10000.0, 20000.0])
BARO = dict(ttime=100.0, ptime=8000.0, T0=0.1, chain=1, strain=0.97, steps=800, interval=10)
BARO_SIZES, BARO_SEED = (6, 8, 10, 12), 1200


def barostat_residuals(pressures, volumes, rest_volume, s):
    """Frames of P and V of rung ``s`` -> (second-half |mean P - P_target| and max |P - P_target|, in rungs; mean V / V_rest)."""
    half = pressures[len(pressures) // 2:] - LADDER_BAR[s] * BAR
    return abs(half.mean()) / (10000.0 * BAR), np.abs(half).max() / (10000.0 * BAR), volumes[len(volumes) // 2:].mean() / rest_volume


def barostat_ref(s):
    n = BARO_SIZES[s]
    lat, frac, _ = make_crystal(n, BARO_SEED + s)
    efs = springs_efs(*spring_list(lat, frac, nnb=14))
    cell = BARO["strain"] * lat
    integ = MTKRef(frac @ cell, np.zeros((n, 3)), np.full(n, 28.0), 1.0 * FS, BARO["T0"], BARO["ttime"] * FS, BARO["ptime"] * FS,
                   cell, LADDER_BAR[s] * BAR, chain=BARO["chain"])
    fr = run_nh_ref(integ, efs, BARO["steps"], BARO["interval"])["frames"]
    return barostat_residuals(np.array([f[6] for f in fr]), np.array([f[7] for f in fr]), abs(np.linalg.det(lat)), s)
