"""Batched molecular dynamics at fixed cell or constant pressure, integrator state on the device.

The reference runs MD one structure at a time: ``ForceField.run_nve_velocity_verlet`` / ``run_nvt_langevin`` /
``run_nvt_berendsen`` / ``run_nvt_andersen`` / ``run_npt_berendsen`` (alignn/ff/ff.py:419-600) wrap ASE's ``VelocityVerlet`` /
``Langevin`` / ``NVTBerendsen`` / ``Andersen`` / ``NPTBerendsen`` around ``AlignnAtomwiseCalculator``, one host round trip and
one host-side graph build per step.  ``run_md`` integrates B independent crystals together:

1. build the graph batch of all B structures on the device (``neighbors.crystal_batch``);
2. evaluate energies and forces (NPT: and stresses) with ``model(batch)``, or replay that evaluation
   (``md.GraphedForceField``, ``replay=True``);
3. one ``alignn_md_step`` launch (csrc/dynamics.hip; its argument block ``alignn_md_args`` is filled once, a step sets the
   evaluation's pointers and ``t``): finish step t with the new forces, record frame t, begin step t + 1 - under NPT the
   pressure, the scaled cell, its inverse and the scaled positions too.

No structure retires, so nothing is read back per step beyond what the neighbour search reads.  The semantics are ASE 3.22.1's
(``environment.yml``), restated in numpy in tests/md_ref.py and tests/md_npt_ref.py.  The random numbers are the
project's own counter-based stream (Philox4x32-10 per structure, csrc/dynamics.hip): a structure's trajectory is the same bits
alone or in a batch.
"""

from __future__ import annotations

import ctypes as C
import numbers
from dataclasses import dataclass
from typing import Callable, List, Optional, Sequence

import numpy as np
import torch

from . import _lib
from ._structures import EV_A3_TO_GPA, ForceEvaluator, check_inputs, gpu_device, pack, shape_of

__all__ = ["run_md", "MDResult", "FS", "KB", "BAR"]

# ASE's units (CODATA 2014, its default): the femtosecond in ASE time units (A sqrt(amu / eV)) and Boltzmann's constant (eV/K)
FS = 0.09822694788464063
KB = 8.617330337217213e-05
BAR = 1e-4 / EV_A3_TO_GPA  # eV/A^3 (160.21766208 eV/A^3 per GPa, the constant of _structures.ForceEvaluator)

ENSEMBLES = {"nve": 0, "nvt_langevin": 1, "nvt_berendsen": 2, "nvt_andersen": 3, "npt_berendsen": 4, "nvt_nose_hoover": 5,
             "npt_nose_hoover": 6}
NHC_MAX, NHC_STATE = 8, 34  # links per chain at the most; the doubles of a structure's chain state (alignn_md_args.nhc_state)


@dataclass
class MDResult:
    """Frame k = 0 .. steps // interval is the state after step k * interval (frame 0: the start).  ``epot`` (eV), ``ekin``
    (eV) and ``temperature`` (K, 3N degrees of freedom) are [n_frames, B]; ``traj_positions`` / ``traj_momenta`` [n_frames,
    sum n_i, 3] (``trajectory=True``, else None).  ``positions`` (Cartesian, unwrapped), ``momenta`` (amu A / ASE time) and
    ``forces`` (eV/A) are those of the final state, per structure in the input order.  ``n_evals`` counts batched force
    evaluations (``steps + 1``).  ``npt_berendsen`` only (else None): ``lattices`` [B, 3, 3] the final cells (``positions`` are
    Cartesian and unwrapped in them), ``pressure`` (eV/A^3, ``-tr(stress) / 3 + 2 KE / (3 V)``; divide by ``BAR`` for bar) and
    ``volume`` (A^3) [n_frames, B], ``traj_lattices`` [n_frames, B, 3, 3] (``trajectory=True``).  ``npt_nose_hoover`` fills them
    too (``pressure`` only with the barostat on: without it no stress is evaluated).  ``conserved`` [n_frames, B] (eV;
    ``nvt_nose_hoover`` / ``npt_nose_hoover`` only): the extended system's conserved energy H'."""

    epot: torch.Tensor
    ekin: torch.Tensor
    temperature: torch.Tensor
    traj_positions: Optional[torch.Tensor]
    traj_momenta: Optional[torch.Tensor]
    positions: List[torch.Tensor]
    momenta: List[torch.Tensor]
    forces: List[torch.Tensor]
    n_evals: int
    lattices: Optional[torch.Tensor] = None
    pressure: Optional[torch.Tensor] = None
    volume: Optional[torch.Tensor] = None
    traj_lattices: Optional[torch.Tensor] = None
    conserved: Optional[torch.Tensor] = None


def berendsen_taut(taut: Optional[float], timestep: float) -> float:
    """Berendsen's time constant in ASE time units: ``taut`` fs, or ``100 * timestep`` fs when None (ff.py:529)."""
    return (100.0 * timestep if taut is None else float(taut)) * FS


def barostat_taup(taup: Optional[float]) -> float:
    """NPTBerendsen's pressure time constant in ASE time units: ``taup`` fs, or ASE's default 1000 fs when None."""
    return (1000.0 if taup is None else float(taup)) * FS


def _per_structure(x, B: int, what: str, signed: bool = False) -> List[float]:
    if isinstance(x, numbers.Real):
        vals = [float(x)] * B
    else:
        vals = [float(v) for v in np.asarray(x, dtype=np.float64).reshape(-1)]
        if len(vals) != B:
            raise ValueError(f"run_md: {what} must be a number or one per structure ({B}), got {len(vals)}")
    if not all(np.isfinite(v) and (signed or v >= 0.0) for v in vals):
        raise ValueError(f"run_md: {what} must be finite" + ("" if signed else " and >= 0"))
    return vals


def _seeds(seed, B: int) -> List[int]:
    vals = [seed] * B if isinstance(seed, numbers.Integral) else list(seed)
    if len(vals) != B or not all(isinstance(s, numbers.Integral) for s in vals):
        raise ValueError(f"run_md: seed must be an int or {B} ints")
    if not all(0 <= int(s) < 2 ** 64 for s in vals):
        raise ValueError("run_md: seeds must lie in [0, 2^64)")
    return [int(s) - 2 ** 64 if int(s) >= 2 ** 63 else int(s) for s in vals]  # (the uint64 bits as an int64 tensor)


def run_md(model, lattices: Sequence, positions: Sequence, atom_features: Optional[Sequence], masses: Sequence, *,
           ensemble: str = "nve", timestep: float = 0.01, steps: int = 1000, interval: int = 1, temperature_K=300.0,
           friction: float = 1e-4, taut: Optional[float] = None, andersen_prob: float = 0.1, taup: Optional[float] = None,
           pressure=None, compressibility=None, ttime: Optional[float] = None, ptime: Optional[float] = None, chain: int = 3,
           nhc_loops: int = 1, nhc_order: int = 3, stress_weight: float = 1.0, initial_temperature_K=None,
           momenta: Optional[Sequence] = None, fixcm: bool = True, seed=0, trajectory: bool = True, replay: bool = False, cutoff: float = 8.0,
           max_neighbors: int = 12, neighbor_strategy: str = "k-nearest", intensive: bool = True, force_multiplier: float = 1.0,
           forces_fn: Optional[Callable] = None, device=None) -> MDResult:
    """Run ``steps`` steps of MD on B crystals; ASE's ``Dynamics.run(steps)`` with observers every ``interval``
    steps, for each structure.

    The structures, ``masses``, the model (or ``forces_fn``), ``cutoff`` ... ``force_multiplier`` and the device:
    alignn_amd/_structures.py.

    ``ensemble``: ``"nve"`` (VelocityVerlet), ``"nvt_langevin"`` (Langevin: ``temperature_K``, ``friction`` in ASE inverse
    time units), ``"nvt_berendsen"`` (NVTBerendsen: ``temperature_K``, ``taut`` in fs, ``100 * timestep`` when None, at least
    ``timestep``), ``"nvt_andersen"`` (Andersen: ``temperature_K``, ``andersen_prob`` in [0, 1], the chance per step and
    velocity component of a fresh Maxwell-Boltzmann draw; the uniform draws lie in (0, 1], so 0 never replaces and 1 always
    does), ``"npt_berendsen"`` (NPTBerendsen, isotropic: ``temperature_K``, ``taut`` as above, ``taup`` in fs, 1000 when None,
    at least ``timestep``; ``pressure`` in bar and ``compressibility`` in 1/bar, each a number or one per structure, both
    required; the cell and the positions are scaled every step, ``MDResult.lattices`` are the final cells).  NPT needs
    stresses: the model must predict per-crystal stresses, scaled by ``stress_weight`` as in ``relax``, and ``forces_fn`` must
    return ``(energy, forces, stress)``; the cells it gets change from step to step.  ``"nvt_nose_hoover"`` / ``"npt_nose_hoover"``
    are not ASE's: Nose-Hoover chains and the isotropic MTK barostat in the explicit reversible form of Martyna, Tuckerman,
    Tobias and Klein (Mol. Phys. 87, 1117, 1996; tests/md_nose_hoover_ref.py restates it): ``temperature_K`` (> 0),
    ``ttime`` / ``ptime`` the thermostat's / barostat's time constants in fs, at least ``timestep`` (chain masses
    ``Q_0 = 3N kT ttime^2``, ``Q_k = kT ttime^2``, barostat mass ``(3N + 3) kT ptime^2``), ``chain`` links (1..8), ``nhc_loops``
    (1..16) loops of the Suzuki-Yoshida weights of ``nhc_order`` (1, 3 or 5), ``pressure`` in bar.  ``nvt_nose_hoover`` needs
    ``ttime``; ``npt_nose_hoover`` takes None for either: ``ttime=None`` is no thermostat, ``ptime=None`` no barostat (then no
    ``pressure`` and no stresses are needed), both None constant cell and energy - what the reference's
    ``run_npt_nose_hoover`` runs.  ``MDResult.conserved`` is their conserved energy.  ``timestep`` in fs.  ``temperature_K`` and ``initial_temperature_K`` are a number or one per structure.
    The start momenta: Maxwell-Boltzmann at ``initial_temperature_K`` when given, else ``momenta`` (B [n_i, 3]), else zero.
    ``fixcm``: the centre-of-mass correction of Langevin, NVTBerendsen / NPTBerendsen and Andersen; for the Nose-Hoover
    ensembles the centre-of-mass velocity is removed from the start momenta, once.  ``seed``: an int or B ints in [0, 2^64), the key of
    each structure's random stream.  ``replay``: evaluate through ``md.GraphedForceField`` (the same bits)."""
    if ensemble not in ENSEMBLES:
        raise ValueError(f"run_md: ensemble must be one of {sorted(ENSEMBLES)}, got {ensemble!r}")
    andersen, nose = ensemble == "nvt_andersen", ensemble in ("nvt_nose_hoover", "npt_nose_hoover")
    if nose:
        if ensemble == "nvt_nose_hoover" and ttime is None:
            raise ValueError("run_md: nvt_nose_hoover needs ttime (fs)")
        for name, val in (("ttime", ttime),) + ((("ptime", ptime),) if ensemble == "npt_nose_hoover" else ()):
            if val is not None and not (isinstance(val, numbers.Real) and np.isfinite(val) and val >= timestep):
                raise ValueError(f"run_md: {name} must be finite and at least the timestep")
        if not (isinstance(chain, numbers.Integral) and 1 <= chain <= NHC_MAX):
            raise ValueError(f"run_md: chain must be an integer in 1..{NHC_MAX}")
        if not (isinstance(nhc_loops, numbers.Integral) and 1 <= nhc_loops <= 16):
            raise ValueError("run_md: nhc_loops must be an integer in 1..16")
        if nhc_order not in (1, 3, 5):
            raise ValueError("run_md: nhc_order must be 1, 3 or 5")
    baro = ensemble == "npt_nose_hoover" and ptime is not None  # the MTK barostat is on
    cell = ensemble in ("npt_berendsen", "npt_nose_hoover")  # the NPT outputs are filled
    npt = ensemble == "npt_berendsen" or baro  # stresses are needed
    ns = check_inputs("run_md", model, lattices, positions, atom_features, masses, forces_fn=forces_fn, stress=npt)
    B = len(ns)
    if not (isinstance(steps, numbers.Integral) and isinstance(interval, numbers.Integral)) or steps < 0 or interval < 1:
        raise ValueError("run_md: need integer steps >= 0 and interval >= 1")
    if steps >= 2 ** 31 - 1:
        raise ValueError("run_md: steps must be below 2^31 - 1")
    if not (timestep > 0 and np.isfinite(timestep)):
        raise ValueError("run_md: timestep must be > 0")
    if not (friction >= 0 and np.isfinite(friction)):
        raise ValueError("run_md: friction must be >= 0")
    t0 = _per_structure(temperature_K, B, "temperature_K")
    tau = berendsen_taut(taut, timestep)
    if ensemble in ("nvt_berendsen", "npt_berendsen") and not (tau >= timestep * FS and np.isfinite(tau)):
        raise ValueError("run_md: taut must be at least the timestep")
    if not (isinstance(andersen_prob, numbers.Real) and 0.0 <= andersen_prob <= 1.0):
        raise ValueError("run_md: andersen_prob must lie in [0, 1]")
    taup_ase = barostat_taup(taup)
    p_target = comp = None
    if nose and (ttime is not None or baro) and not all(v > 0.0 for v in t0):
        raise ValueError("run_md: a Nose-Hoover thermostat or barostat needs temperature_K > 0")
    if baro:
        if pressure is None:
            raise ValueError("run_md: npt_nose_hoover with ptime needs pressure (bar)")
        p_target = [v * BAR for v in _per_structure(pressure, B, "pressure", signed=True)]
    elif npt:
        if not (taup_ase >= timestep * FS and np.isfinite(taup_ase)):
            raise ValueError("run_md: taup must be at least the timestep")
        if pressure is None or compressibility is None:
            raise ValueError("run_md: npt_berendsen needs pressure (bar) and compressibility (1/bar)")
        p_target = [v * BAR for v in _per_structure(pressure, B, "pressure", signed=True)]
        comp = [v / BAR for v in _per_structure(compressibility, B, "compressibility")]
    if npt:
        if not (isinstance(stress_weight, numbers.Real) and np.isfinite(stress_weight)):
            raise ValueError("run_md: stress_weight must be a finite number")
    t_init = None if initial_temperature_K is None else _per_structure(initial_temperature_K, B, "initial_temperature_K")
    if t_init is not None and momenta is not None:
        raise ValueError("run_md: give initial_temperature_K or momenta, not both")
    seeds = _seeds(seed, B)
    if momenta is not None:
        if len(momenta) != B or any(shape_of(p) != (ns[i], 3) for i, p in enumerate(momenta)):
            raise ValueError("run_md: momenta must be B arrays [n_i, 3]")
    dev = gpu_device("run_md", model, forces_fn, device)
    lib = _lib.load()
    ens = ENSEMBLES[ensemble]
    dt = timestep * FS

    with _lib.device_guard(torch.empty(0, device=dev)):
        packed = pack(lattices, positions, ns, dev, masses)
        pos, inv, frac, mass, atom_ptr = packed.pos, packed.inv, packed.frac, packed.mass, packed.atom_ptr
        N = packed.ptr[-1]
        t0_t = torch.tensor(t0, dtype=torch.float64, device=dev)
        seed_t = torch.tensor(seeds, dtype=torch.int64, device=dev)
        if t_init is not None:
            mom = torch.empty(N, 3, dtype=torch.float64, device=dev)
            t_init_t = torch.tensor(t_init, dtype=torch.float64, device=dev)
            _lib.check(lib.alignn_md_init_momenta(atom_ptr.data_ptr(), B, mass.data_ptr(), t_init_t.data_ptr(), seed_t.data_ptr(),
                                                  mom.data_ptr(), KB, _lib.stream()), "md_init_momenta")
        elif momenta is not None:
            mom = torch.cat([torch.as_tensor(p).to(dev, torch.float64) for p in momenta]).contiguous()
        else:
            mom = torch.zeros(N, 3, dtype=torch.float64, device=dev)
        vel = scratch = None
        if ensemble == "nvt_langevin" or andersen:  # v between the halves; Langevin's noise, Andersen's positions before the drift
            vel, scratch = torch.zeros(N, 3, dtype=torch.float64, device=dev), torch.zeros(N, 3, dtype=torch.float64, device=dev)
        n_frames = steps // interval + 1
        epot, ekin, temp = (torch.zeros(n_frames, B, dtype=torch.float64, device=dev) for _ in range(3))
        traj_p = torch.zeros(n_frames, N, 3, dtype=torch.float64, device=dev) if trajectory else None
        traj_m = torch.zeros(n_frames, N, 3, dtype=torch.float64, device=dev) if trajectory else None
        status = torch.zeros(1, dtype=torch.int32, device=dev)
        lat_cur = p_out = v_out = traj_l = p_target_t = comp_t = nhc = conserved = None
        if cell:
            lat_cur = packed.lat.clone()  # the kernel rewrites it and ``inv``
            v_out = torch.zeros(n_frames, B, dtype=torch.float64, device=dev)
            traj_l = torch.zeros(n_frames, B, 3, 3, dtype=torch.float64, device=dev) if trajectory else None
        if npt:
            p_target_t = torch.tensor(p_target, dtype=torch.float64, device=dev)
            comp_t = None if comp is None else torch.tensor(comp, dtype=torch.float64, device=dev)
            p_out = torch.zeros(n_frames, B, dtype=torch.float64, device=dev)
        if nose:
            nhc = torch.zeros(B, NHC_STATE, dtype=torch.float64, device=dev)
            conserved = torch.zeros(n_frames, B, dtype=torch.float64, device=dev)
        # fixed per-structure views: the same lattice tensors every step keep neighbors' lattice tables cached
        lat_v = [packed.lat[s] for s in range(B)]
        pos_v, frac_v = packed.rows(pos), packed.rows(frac)
        evaluate = ForceEvaluator("run_md", model, forces_fn, atom_features, ns, dev, cutoff=cutoff, max_neighbors=max_neighbors,
                                  neighbor_strategy=neighbor_strategy, intensive=intensive, force_multiplier=force_multiplier,
                                  stress_weight=float(stress_weight) if npt else None, replay=replay)
        every = list(range(B))
        args = _lib.MdArgs(
            atom_ptr=atom_ptr.data_ptr(), masses=mass.data_ptr(), t0_kelvin=t0_t.data_ptr(), seeds=seed_t.data_ptr(),
            pressure=_lib.ptr(p_target_t), compressibility=_lib.ptr(comp_t),
            lattice=(lat_cur if cell else packed.lat).data_ptr() if cell or andersen else None, inv_lattice=inv.data_ptr(),
            momenta=mom.data_ptr(), positions=pos.data_ptr(), frac=frac.data_ptr(), velocities=_lib.ptr(vel),
            scratch=_lib.ptr(scratch), status=status.data_ptr(), epot=epot.data_ptr(), ekin=ekin.data_ptr(),
            temperature=temp.data_ptr(), pressure_out=_lib.ptr(p_out), volume_out=_lib.ptr(v_out),
            traj_positions=_lib.ptr(traj_p), traj_momenta=_lib.ptr(traj_m), traj_lattice=_lib.ptr(traj_l),
            n_structures=B, interval=int(interval), steps=int(steps), ensemble=ens, fixcm=int(bool(fixcm)), dt=dt,
            friction=float(friction), andersen_prob=float(andersen_prob), taut=tau, taup=taup_ase, kB=KB,
            nhc_state=_lib.ptr(nhc), conserved_out=_lib.ptr(conserved), chain=int(chain) if nose else 0,
            nhc_loops=int(nhc_loops) if nose else 0, nhc_order=int(nhc_order) if nose else 0,
            ttime=float(ttime) * FS if nose and ttime is not None else 0.0, ptime=float(ptime) * FS if baro else 0.0)

        for t in range(steps + 1):
            if npt:
                # fresh tensors every step: the kernel writes lat_cur through a raw pointer (no version bump), which the
                # lattice-table cache of neighbors would not see
                lat_now = lat_cur.clone()
                lat_v = [lat_now[s] for s in range(B)]
            energy, forces, stress = evaluate(every, lat_v, frac_v, pos_v)
            args.forces, args.energy, args.stress = forces.data_ptr(), energy.data_ptr(), _lib.ptr(stress)
            args.n_rows, args.t = forces.shape[0], t
            _lib.check(lib.alignn_md_step(C.byref(args), _lib.stream()), "md_step")
        if status.item() != 0:
            raise RuntimeError("run_md: md_step found force rows that do not match the batch's atom count")

        return MDResult(epot=epot, ekin=ekin, temperature=temp, traj_positions=traj_p, traj_momenta=traj_m,
                        positions=[p.clone() for p in pos_v], momenta=[p.clone() for p in packed.rows(mom)],
                        forces=[f.clone() for f in packed.rows(forces)], n_evals=steps + 1, lattices=lat_cur, pressure=p_out,
                        volume=v_out, traj_lattices=traj_l, conserved=conserved)
