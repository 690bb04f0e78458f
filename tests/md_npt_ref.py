"""The executable specification of the ``nvt_andersen`` and ``npt_berendsen`` ensembles of ``alignn_amd.run_md``
(csrc/dynamics.hip, ``alignn_md_step`` with ensembles 3 and 4): a float64 numpy restatement of ASE 3.22.1's ``Andersen`` and
``NPTBerendsen`` as the reference's ``ForceField.run_nvt_andersen`` / ``run_npt_berendsen`` drive them (alignn/ff/ff.py:477-600), on top of
the base classes and the random stream of md_ref.py.  ASE is not a dependency of this project; the restatement follows
the published ase/md/andersen.py and ase/md/nptberendsen.py, and tests/test_md_npt_ref.py pins it to steps computed by hand.
Where a detail of ASE was in doubt when this was written, the project's own statement rules:

- NPTBerendsen takes one evaluation per step: the pressure of a step comes from the stress of the last evaluation (the state
  before the cell is scaled) and the first half-kick uses the forces of that same evaluation, although the cell and the
  positions have been scaled in between;
- the pressure carries the ideal-gas term of the momenta after the velocity scaling: ``P = -tr(S) / 3 + 2 KE / (3 V)``,
  ``V = |det cell|``;
- ``set_cell(scale_atoms=True)`` with an isotropic factor is ``cell <- mu cell``, ``positions <- mu positions``; the momenta
  stay; ``mu`` is not clipped; only the isotropic form exists here;
- ``pressure`` and ``compressibility`` enter the integrator in eV/A^3 and A^3/eV; ``run_md`` takes bar and 1/bar and converts
  with ``BAR`` (ASE's ``1e5 * units.Pascal``, CODATA 2014);
- Andersen's ``fixcm`` removes the mass-weighted mean velocity and, after the drift, moves all atoms by the difference of the
  old and the new centre of mass (``set_center_of_mass``); the velocity is then recomputed from the positions;
- Andersen's kicks are ``0.5 * f / m * dt`` evaluated left to right.

ASE's numpy random streams are not reproduced.  Andersen draws from the project's stream (md_ref.py), purposes 2 and 3,
so that no draw of purposes 0 (Langevin) and 1 (Maxwell-Boltzmann) moves: at counter (atom, t, j, 2) blocks j = 0, 1 give the
normals g0..g3 (replacement velocity ``(g0, g1, g2) sqrt(kB T0 / m)``), blocks j = 2, 3 the uniforms ``unit(w0, w1)``,
``unit(w2, w3)`` (u0, u1 of block 2, u2 of block 3; component c is replaced when ``u_c <= andersen_prob``); at counter
(0, t, j, 3), j = 0, 1, the three centre-of-mass normals of the structure.  ``unit_interval`` lies in (0, 1]: probability 0
never replaces, 1 always.  The GPU tests (test_gpu_dynamics_npt.py) hold the kernel and ``run_md`` to this file."""

import numpy as np

from alignn_amd.dynamics import KB
from tests.md_ref import (BerendsenRef, VerletRef, berendsen_scale, box_muller, kinetic_energy, stream_words, temperature,
                          unit_interval)


PURPOSE_ANDERSEN, PURPOSE_ANDERSEN_COM = 2, 3


# ---- the draws ------------------------------------------------------------------------------------------------------------
def andersen_draws(seed, n, t):
    """(com [3], g [n, 3], u [n, 3]) of the Andersen step that starts at iteration t: the centre-of-mass normals, the
    replacement normals and the uniforms of every velocity component."""
    w = stream_words(seed, n, t, PURPOSE_ANDERSEN, 4)
    g = box_muller(w[:, :2]).reshape(n, 4)
    u = np.stack([unit_interval(w[:, 2, 0], w[:, 2, 1]), unit_interval(w[:, 2, 2], w[:, 2, 3]),
                  unit_interval(w[:, 3, 0], w[:, 3, 1])], axis=1)
    com = box_muller(stream_words(seed, 1, t, PURPOSE_ANDERSEN_COM, 2)).reshape(4)
    return com[:3], g[:, :3], u


# ---- the integrators ------------------------------------------------------------------------------------------------------
def pressure_of(p, m, stress, cell):
    """-tr(stress) / 3 plus the ideal-gas term 2 KE / (3 V) (``get_stress(include_ideal_gas=True)``)."""
    return -(stress[0, 0] + stress[1, 1] + stress[2, 2]) / 3.0 + 2.0 * kinetic_energy(p, m) / (3.0 * abs(np.linalg.det(cell)))


class NPTBerendsenRef(BerendsenRef):
    """ase/md/nptberendsen.py NPTBerendsen.step: NVTBerendsen's velocity scaling, the isotropic scaling of cell and positions,
    then NVTBerendsen's half-kick, fixcm and drift.  ``pressure`` in eV/A^3, ``compressibility`` in A^3/eV, ``dt`` / ``taut`` /
    ``taup`` in ASE time units.  ``begin(f, stress)`` takes the forces and the stress of the current state."""

    def __init__(self, r, p, m, dt, T0, taut, cell, taup, pressure, compressibility, fixcm=True):
        super().__init__(r, p, m, dt, T0, taut, fixcm)
        self.cell, self.taup = np.array(cell, dtype=np.float64), taup
        self.pressure, self.compressibility = pressure, compressibility
        self.mu = self.P = None

    def begin(self, f, stress):
        self.p = berendsen_scale(self.T0, temperature(self.p, self.m), self.dt, self.taut) * self.p
        self.P = pressure_of(self.p, self.m, stress, self.cell)
        self.mu = 1.0 - self.dt / self.taup * self.compressibility / 3.0 * (self.pressure - self.P)
        self.cell = self.mu * self.cell
        self.r = self.mu * self.r
        p = self.p + 0.5 * self.dt * f
        if self.fixcm:
            p = p - p.sum(axis=0) / float(len(p))
        self.r = self.r + self.dt * p / self.m[:, None]
        self.p = p

    def step(self, f, stress, efs):
        """One step from forces and stress of the current state -> (e, f, stress) of the new one; ``efs(cell, r)``."""
        self.begin(f, stress)
        e, f, stress = efs(self.cell, self.r)
        self.finish(f)
        self.nsteps += 1
        return e, f, stress


class AndersenRef(VerletRef):
    """ase/md/andersen.py Andersen.step.  The draws of the step that starts at iteration t = ``nsteps`` come from
    ``andersen_draws(seed, n, t)`` unless ``begin`` gets them.  ``v_replaced``: the velocities right after the replacement."""

    def __init__(self, r, p, m, dt, T0, andersen_prob, fixcm=True, seed=0):
        super().__init__(r, p, m, dt)
        self.temp, self.prob, self.fixcm, self.seed = KB * T0, andersen_prob, fixcm, seed
        self.v = self.v_replaced = None

    def begin(self, f, com=None, g=None, u=None):
        m = self.m[:, None]
        if g is None:
            com, g, u = andersen_draws(self.seed, len(self.m), self.nsteps)
        v = self.p / m
        if self.fixcm:
            v = v + np.asarray(com) * np.sqrt(self.temp / self.m.sum())
        v = v + 0.5 * f / m * self.dt
        v = np.where(np.asarray(u) <= self.prob, np.asarray(g) * np.sqrt(self.temp / m), v)
        self.v_replaced = v.copy()
        x = self.r
        if self.fixcm:
            old_com = (m * x).sum(axis=0) / self.m.sum()
            v = v - (m * v).sum(axis=0) / self.m.sum()
        self.v_drift = v
        r = x + v * self.dt
        if self.fixcm:
            r = r + (old_com - (m * r).sum(axis=0) / self.m.sum())
        self.r = r
        self.v = (r - x) / self.dt

    def finish(self, f):
        m = self.m[:, None]
        self.v = self.v + 0.5 * f / m * self.dt
        self.p = m * self.v


def run_npt_ref(integ, efs, steps, interval=1):
    """md_ref.run_ref for NPTBerendsenRef: frames (step, r, p, e_pot, e_kin, cell, P, V), P with the ideal-gas term from
    the recorded momenta and the stress of the evaluation at the recorded state."""

    def frame(k, e, stress):
        return (k, integ.r.copy(), integ.p.copy(), e, kinetic_energy(integ.p, integ.m), integ.cell.copy(),
                pressure_of(integ.p, integ.m, stress, integ.cell), abs(np.linalg.det(integ.cell)))

    e, f, stress = efs(integ.cell, integ.r)
    frames = [frame(0, e, stress)]
    for k in range(1, steps + 1):
        e, f, stress = integ.step(f, stress, efs)
        if k % interval == 0:
            frames.append(frame(k, e, stress))
    return dict(frames=frames, n_evals=steps + 1, f=f, stress=stress)
