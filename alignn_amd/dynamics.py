"""Batched molecular dynamics at fixed cell, integrator state on the device.

The reference runs MD one structure at a time: ``ForceField.run_nve_velocity_verlet`` / ``run_nvt_langevin`` /
``run_nvt_berendsen`` (alignn/ff/ff.py:419-550) wrap ASE's ``VelocityVerlet`` / ``Langevin`` / ``NVTBerendsen`` around
``AlignnAtomwiseCalculator``, one host round trip and one host-side graph build per step.  ``run_md`` integrates B independent
crystals together:

1. build the graph batch of all B structures on the device (``neighbors.crystal_batch``);
2. evaluate energies and forces with ``model(batch)``, or replay that evaluation (``md.GraphedForceField``, ``replay=True``);
3. one ``alignn_md_step`` launch (csrc/dynamics.hip): finish step t with the new forces, record frame t, begin step t + 1.

No structure retires, so nothing is read back per step beyond what the neighbour search reads.  The semantics are ASE 3.22.1's
(``environment.yml``), restated in numpy in tests/test_md_ref.py.  The random numbers are the project's own counter-based
stream (Philox4x32-10 per structure, csrc/dynamics.hip): a structure's trajectory is the same bits alone or in a batch.
"""

from __future__ import annotations

import numbers
from dataclasses import dataclass
from typing import Callable, List, Optional, Sequence

import numpy as np
import torch

from . import _lib, neighbors

__all__ = ["run_md", "MDResult", "FS", "KB"]

# ASE's units (CODATA 2014, its default): the femtosecond in ASE time units (A sqrt(amu / eV)) and Boltzmann's constant (eV/K)
FS = 0.09822694788464063
KB = 8.617330337217213e-05

ENSEMBLES = {"nve": 0, "nvt_langevin": 1, "nvt_berendsen": 2}


@dataclass
class MDResult:
    """Frame k = 0 .. steps // interval is the state after step k * interval (frame 0: the start).  ``epot`` (eV), ``ekin``
    (eV) and ``temperature`` (K, 3N degrees of freedom) are [n_frames, B]; ``traj_positions`` / ``traj_momenta`` [n_frames,
    sum n_i, 3] (``trajectory=True``, else None).  ``positions`` (Cartesian, unwrapped), ``momenta`` (amu A / ASE time) and
    ``forces`` (eV/A) are those of the final state, per structure in the input order.  ``n_evals`` counts batched force
    evaluations (``steps + 1``)."""

    epot: torch.Tensor
    ekin: torch.Tensor
    temperature: torch.Tensor
    traj_positions: Optional[torch.Tensor]
    traj_momenta: Optional[torch.Tensor]
    positions: List[torch.Tensor]
    momenta: List[torch.Tensor]
    forces: List[torch.Tensor]
    n_evals: int


def berendsen_taut(taut: Optional[float], timestep: float) -> float:
    """Berendsen's time constant in ASE time units: ``taut`` fs, or ``100 * timestep`` fs when None (ff.py:529)."""
    return (100.0 * timestep if taut is None else float(taut)) * FS


def _per_structure(x, B: int, what: str) -> List[float]:
    if isinstance(x, numbers.Real):
        vals = [float(x)] * B
    else:
        vals = [float(v) for v in np.asarray(x, dtype=np.float64).reshape(-1)]
        if len(vals) != B:
            raise ValueError(f"run_md: {what} must be a number or one per structure ({B}), got {len(vals)}")
    if not all(np.isfinite(v) and v >= 0.0 for v in vals):
        raise ValueError(f"run_md: {what} must be finite and >= 0")
    return vals


def _seeds(seed, B: int) -> List[int]:
    vals = [seed] * B if isinstance(seed, numbers.Integral) else list(seed)
    if len(vals) != B or not all(isinstance(s, numbers.Integral) for s in vals):
        raise ValueError(f"run_md: seed must be an int or {B} ints")
    if not all(0 <= int(s) < 2 ** 64 for s in vals):
        raise ValueError("run_md: seeds must lie in [0, 2^64)")
    return [int(s) - 2 ** 64 if int(s) >= 2 ** 63 else int(s) for s in vals]  # (the uint64 bits as an int64 tensor)


def _shape(x):
    return tuple(x.shape) if hasattr(x, "shape") else np.shape(x)


def run_md(model, lattices: Sequence, positions: Sequence, atom_features: Optional[Sequence], masses: Sequence, *,
           ensemble: str = "nve", timestep: float = 0.01, steps: int = 1000, interval: int = 1, temperature_K=300.0,
           friction: float = 1e-4, taut: Optional[float] = None, initial_temperature_K=None, momenta: Optional[Sequence] = None,
           fixcm: bool = True, seed=0, trajectory: bool = True, replay: bool = False, cutoff: float = 8.0,
           max_neighbors: int = 12, neighbor_strategy: str = "k-nearest", intensive: bool = True, force_multiplier: float = 1.0,
           forces_fn: Optional[Callable] = None, device=None) -> MDResult:
    """Run ``steps`` steps of MD on B crystals at fixed cell; ASE's ``Dynamics.run(steps)`` with observers every ``interval``
    steps, for each structure.

    ``lattices``: B cells [3, 3] (rows a, b, c); ``positions``: B Cartesian [n_i, 3]; ``atom_features``: B [n_i, F] (the model's
    ``atom_input_features``); ``masses``: B [n_i] in amu.  ``model``: an ``ALIGNNAtomWise`` with ``calculate_gradient=True``
    in eval mode; energies are ``out * n_i`` when ``intensive``, forces ``grad * force_multiplier``.  ``cutoff``,
    ``max_neighbors``, ``neighbor_strategy``: the graph construction.  ``forces_fn(lattices, positions) -> (energy [B],
    forces [sum n_i, 3])`` replaces the model (it gets device tensors it must not modify).

    ``ensemble``: ``"nve"`` (VelocityVerlet), ``"nvt_langevin"`` (Langevin: ``temperature_K``, ``friction`` in ASE inverse
    time units), ``"nvt_berendsen"`` (NVTBerendsen: ``temperature_K``, ``taut`` in fs, ``100 * timestep`` when None, at least
    ``timestep``).  ``timestep`` in fs.  ``temperature_K`` and ``initial_temperature_K`` are a number or one per structure.
    The start momenta: Maxwell-Boltzmann at ``initial_temperature_K`` when given, else ``momenta`` (B [n_i, 3]), else zero.
    ``fixcm``: Langevin's and NVTBerendsen's centre-of-mass correction.  ``seed``: an int or B ints in [0, 2^64), the key of
    each structure's random stream.  ``replay``: evaluate through ``md.GraphedForceField`` (the same bits).  Runs on the GPU
    (the model's device, else ``device``, else the current one)."""
    B = len(positions)
    if B == 0 or len(lattices) != B or len(masses) != B:
        raise ValueError(f"run_md: {len(lattices)} lattices, {B} position arrays, {len(masses)} mass arrays (need the same "
                         "number, at least one)")
    if ensemble not in ENSEMBLES:
        raise ValueError(f"run_md: ensemble must be one of {sorted(ENSEMBLES)}, got {ensemble!r}")
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
    if ensemble == "nvt_berendsen" and not (tau >= timestep * FS and np.isfinite(tau)):
        raise ValueError("run_md: taut must be at least the timestep")
    t_init = None if initial_temperature_K is None else _per_structure(initial_temperature_K, B, "initial_temperature_K")
    if t_init is not None and momenta is not None:
        raise ValueError("run_md: give initial_temperature_K or momenta, not both")
    seeds = _seeds(seed, B)
    ns = []
    for i, p in enumerate(positions):
        sh = _shape(p)
        if len(sh) != 2 or sh[1] != 3 or sh[0] < 1:
            raise ValueError(f"run_md: positions[{i}] is {sh}, need [n_i, 3] with n_i >= 1")
        ns.append(int(sh[0]))
    for i, m in enumerate(masses):
        if _shape(m) != (ns[i],):
            raise ValueError(f"run_md: masses[{i}] is {_shape(m)}, need [{ns[i]}]")
    if momenta is not None:
        if len(momenta) != B or any(_shape(p) != (ns[i], 3) for i, p in enumerate(momenta)):
            raise ValueError("run_md: momenta must be B arrays [n_i, 3]")
    if forces_fn is None:
        from .alignn_atomwise import ALIGNNAtomWise

        if not isinstance(model, ALIGNNAtomWise):
            raise TypeError(f"run_md: the model must be an ALIGNNAtomWise, got {type(model).__name__} (or pass forces_fn)")
        if not model.config.calculate_gradient:
            raise ValueError("run_md: the model has calculate_gradient=False and predicts no forces")
        if model.training:
            raise ValueError("run_md: the model is in training mode; call model.eval() first")
        if atom_features is None or len(atom_features) != B:
            raise ValueError("run_md: the model needs atom_features, one [n_i, F] array per structure")
        F_in = model.config.atom_input_features
        for i, f in enumerate(atom_features):
            if _shape(f) != (ns[i], F_in):
                raise ValueError(f"run_md: atom_features[{i}] is {_shape(f)}, need [{ns[i]}, {F_in}]")
        dev = model.fc.weight.device
    else:
        dev = torch.device(device) if device is not None else None
    mass_h = torch.cat([torch.as_tensor(m).detach().to("cpu", torch.float64).reshape(-1) for m in masses])
    if not bool(torch.isfinite(mass_h).all()) or not bool((mass_h > 0).all()):
        raise ValueError("run_md: masses must be finite and > 0")
    if dev is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    if dev.type != "cuda":
        raise TypeError(f"run_md runs on the GPU (csrc/dynamics.hip), got device {dev}")
    lib = _lib.load()
    ens = ENSEMBLES[ensemble]
    dt = timestep * FS

    with _lib.device_guard(torch.empty(0, device=dev)):
        lat = torch.stack([torch.as_tensor(x).to(dev, torch.float64) for x in lattices])
        if lat.shape != (B, 3, 3):
            raise ValueError(f"run_md: lattices must be B x [3, 3], got {tuple(lat.shape)}")
        ptr_h = [0]
        for n in ns:
            ptr_h.append(ptr_h[-1] + n)
        N = ptr_h[-1]
        atom_ptr = torch.tensor(ptr_h, dtype=torch.int32, device=dev)
        inv = torch.linalg.inv(lat).contiguous()
        pos = torch.cat([torch.as_tensor(p).to(dev, torch.float64) for p in positions]).contiguous()
        site = torch.repeat_interleave(torch.arange(B, device=dev), torch.tensor(ns, device=dev))
        frac = torch.bmm(pos.unsqueeze(1), inv[site]).squeeze(1)
        frac = frac - torch.floor(frac)
        frac = torch.where(frac < 1.0, frac, torch.zeros_like(frac)).contiguous()
        mass = mass_h.to(dev)
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
        vel = rnd_vel = None
        if ensemble == "nvt_langevin":
            vel, rnd_vel = torch.zeros(N, 3, dtype=torch.float64, device=dev), torch.zeros(N, 3, dtype=torch.float64, device=dev)
        n_frames = steps // interval + 1
        epot, ekin, temp = (torch.zeros(n_frames, B, dtype=torch.float64, device=dev) for _ in range(3))
        traj_p = torch.zeros(n_frames, N, 3, dtype=torch.float64, device=dev) if trajectory else None
        traj_m = torch.zeros(n_frames, N, 3, dtype=torch.float64, device=dev) if trajectory else None
        status = torch.zeros(1, dtype=torch.int32, device=dev)
        # fixed per-structure views: the same lattice tensors every step keep neighbors' lattice tables cached
        lat_v = [lat[s] for s in range(B)]
        pos_v = [pos[ptr_h[s]:ptr_h[s + 1]] for s in range(B)]
        frac_v = [frac[ptr_h[s]:ptr_h[s + 1]] for s in range(B)]
        if forces_fn is None:
            feats = [torch.as_tensor(f).to(dev, torch.float32) for f in atom_features]
            line_graph = len(model.alignn_layers) > 0
            n_t = torch.tensor(ns, dtype=torch.float32, device=dev)
            if replay:
                from .md import GraphedForceField

                evaluate = GraphedForceField(model)
            else:
                evaluate = model

        for t in range(steps + 1):
            if forces_fn is None:
                batch = neighbors.crystal_batch(lat_v, frac_v, atom_features=feats, device=dev, cutoff=cutoff,
                                                max_neighbors=max_neighbors, line_graph=line_graph,
                                                neighbor_strategy=neighbor_strategy)
                with torch.enable_grad():  # (the force head differentiates the energy)
                    res = evaluate(batch)
                out = res["out"].detach().reshape(-1).float()
                energy = ((out * n_t) if intensive else out).double()
                forces = (res["grad"].detach().reshape(-1, 3) * force_multiplier).double()
            else:
                energy, forces = forces_fn(lat_v, pos_v)
                energy = torch.as_tensor(energy).to(dev, torch.float64).reshape(-1)
                forces = torch.as_tensor(forces).to(dev, torch.float64).reshape(-1, 3)
            if energy.numel() != B or forces.shape[0] != N:
                raise ValueError(f"run_md: evaluation returned {energy.numel()} energies / {forces.shape[0]} force rows for "
                                 f"{B} structures / {N} atoms")
            energy, forces = energy.contiguous(), forces.contiguous()
            _lib.check(lib.alignn_md_step(
                forces.data_ptr(), energy.data_ptr(), forces.shape[0], atom_ptr.data_ptr(), B, mass.data_ptr(), inv.data_ptr(),
                mom.data_ptr(), pos.data_ptr(), frac.data_ptr(), _lib.ptr(vel), _lib.ptr(rnd_vel), t0_t.data_ptr(),
                seed_t.data_ptr(), epot.data_ptr(), ekin.data_ptr(), temp.data_ptr(), _lib.ptr(traj_p), _lib.ptr(traj_m), None,
                status.data_ptr(), t, int(interval), int(steps), ens, dt, float(friction), tau, int(bool(fixcm)), KB,
                _lib.stream()), "md_step")
        if status.item() != 0:
            raise RuntimeError("run_md: md_step found force rows that do not match the batch's atom count")

        return MDResult(epot=epot, ekin=ekin, temperature=temp, traj_positions=traj_p, traj_momenta=traj_m,
                        positions=[p.clone() for p in pos_v], momenta=[mom[ptr_h[s]:ptr_h[s + 1]].clone() for s in range(B)],
                        forces=[forces[ptr_h[s]:ptr_h[s + 1]].clone() for s in range(B)], n_evals=steps + 1)
