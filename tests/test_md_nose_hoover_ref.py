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

``begin`` is 1-4, ``finish`` 6-8, as the kernel's launches split a step.  The checks pin the restatement by what does not come
from the kernel: second-order conservation of H', time reversal, a step by hand, its limits and the barostat's targets.  The
GPU tests (test_gpu_dynamics_nose_hoover.py) hold the kernel and ``run_md`` to this file."""

import ctypes

import numpy as np
import pytest

from alignn_amd import _lib, dynamics
from alignn_amd.dynamics import BAR, FS, KB, MDResult, run_md
from alignn_amd.synthetic import make_crystal
from tests.test_md_npt_ref import pressure_of
from tests.test_md_ref import VerletRef, kinetic_energy, maxwell_boltzmann, temperature
from tests.test_relax_cell import spring_list, springs_efs


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
    """test_md_ref.run_ref for the two classes above: ``efs(cell, r) -> (e, f, stress)``; frames (step, r, p, e_pot, e_kin, cell,
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
