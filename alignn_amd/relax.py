"""Batched fixed-cell structure relaxation with FIRE, optimiser state on the device.

The reference relaxes one structure at a time: ``ForceField.optimize_atoms`` (alignn/ff/ff.py:373-415) wraps ASE's ``FIRE``
around ``AlignnAtomwiseCalculator`` (alignn/ff/calculators.py:280-370), one host round trip per step, and its callers
(``ev_curve``, ``vacancy_formation``, ``surface_energy``, ``get_interface_energy``: ff.py:762-1070) loop over structures.
``relax`` runs the same optimiser (``optimize_lattice=False``, ``downhill_check=False``) for a whole batch:

1. build the graph batch of the ACTIVE structures on the device (``neighbors.crystal_batch``, the line graph only when the
   model has ALIGNN layers);
2. evaluate energies and forces with ``model(batch)`` (the fused ``alignn_ff_eval`` path wherever it applies);
3. one ``alignn_fire_step`` launch (csrc/relax.hip): convergence test of ``Optimizer.run`` (max_i |F_i|^2 < fmax^2), then
   the FIRE update of every unconverged structure, wrapped fractional coordinates for the next neighbour search;
4. read the number of structures still active and their retire flags (one small host read), drop the retired ones.

Positions, velocities, ``dt``, ``a`` and ``Nsteps`` of every structure stay on the device in float64.  A structure's step
depends only on its own forces and state (fixed-order reductions): its trajectory is the same bits whether it is relaxed
alone or beside others.

``optimize_lattice=True`` relaxes the cells too, as ``optimize_atoms``' default does: ASE's ``ExpCellFilter`` around the atoms,
its n + 3 generalised rows per structure (atom rows in the starting cell, cell rows ``n logm(F)`` of the deformation gradient
``F``) driven by the same FIRE in ``alignn_fire_cell_step``.  The model's per-crystal stresses enter as the calculator gives
them (``stress * stress_weight / 160.21766208``, eV/A^3).
"""

from __future__ import annotations

from dataclasses import dataclass
from typing import Callable, List, Optional, Sequence

import torch

from . import _lib, neighbors

__all__ = ["relax", "RelaxResult"]


@dataclass
class RelaxResult:
    """Per structure, in the input order.  ``energies`` / ``forces`` / ``fmax`` are those of the final positions (the last
    evaluation); ``n_steps`` counts FIRE steps taken; ``n_evals`` counts batched force evaluations (model calls).  With
    ``optimize_lattice``, ``fmax`` is the largest of the n + 3 filter rows, ``forces`` stay the atoms' Cartesian forces, and
    ``lattices`` / ``stresses`` are the final cells and the stresses of the last evaluation."""

    positions: List[torch.Tensor]  # [n_i, 3] float64, Cartesian, not wrapped into the cell
    energies: torch.Tensor  # [B] float64
    forces: List[torch.Tensor]  # [n_i, 3] float64
    fmax: torch.Tensor  # [B] float64: max_i |F_i|
    converged: torch.Tensor  # [B] bool
    n_steps: torch.Tensor  # [B] int64
    n_evals: int
    lattices: Optional[torch.Tensor] = None  # [B, 3, 3] float64: the final cells (optimize_lattice only)
    stresses: Optional[torch.Tensor] = None  # [B, 3, 3] float64, eV/A^3, ASE's sign, symmetrised (optimize_lattice only)


def _wrap(frac: torch.Tensor) -> torch.Tensor:
    frac = frac - torch.floor(frac)
    return torch.where(frac < 1.0, frac, torch.zeros_like(frac))


def relax(model, lattices: Sequence, positions: Sequence, atom_features: Optional[Sequence] = None, *, fmax: float = 0.1,
          steps: int = 100, dt: float = 0.1, maxstep: float = 0.2, dtmax: float = 1.0, Nmin: int = 5, finc: float = 1.1,
          fdec: float = 0.5, astart: float = 0.1, fa: float = 0.99, a: float = 0.1, cutoff: float = 8.0, max_neighbors: int = 12,
          neighbor_strategy: str = "k-nearest", intensive: bool = True, force_multiplier: float = 1.0,
          forces_fn: Optional[Callable] = None, device=None, optimize_lattice: bool = False,
          stress_weight: float = 1.0) -> RelaxResult:
    """Relax the atomic positions of B crystals with FIRE until max_i |F_i| < ``fmax`` or ``steps`` steps; at fixed cell, or
    with the cells too when ``optimize_lattice``.

    ``lattices``: B cells [3, 3] (rows a, b, c); ``positions``: B Cartesian [n_i, 3]; ``atom_features``: B [n_i, F] (the
    model's ``atom_input_features``).  ``model``: an ``ALIGNNAtomWise`` with ``calculate_gradient=True`` in eval mode; energies
    are ``out * n_i`` when ``intensive`` (the calculator's rule), forces ``grad * force_multiplier``.  ``cutoff``,
    ``max_neighbors``, ``neighbor_strategy``: the graph construction (``neighbors.crystal_batch``).

    ``forces_fn(lattices, positions) -> (energy [B'], forces [sum n_i, 3])`` replaces the model: it gets the active
    structures' cells and Cartesian positions (lists of device tensors, not to be modified) and returns their energies and
    concatenated forces as they are to be used (no multiplier applied).

    ``dt`` ... ``a``: FIRE's parameters, ASE's defaults (ase/optimize/fire.py).  Runs on the GPU (the model's device, else
    ``device``, else the current one).

    ``optimize_lattice``: relax the cells as well, through ASE's ``ExpCellFilter`` (default arguments).  The reference's
    ``optimize_atoms`` defaults to ``optimize_lattice=True``; here the default stays ``False``.  The model must then predict
    per-crystal stresses (``stresswise_weight != 0``, ``batch_stress=True``), used as ``stress * stress_weight /
    160.21766208`` (the calculator's ``stress_wt``, 1.0 in ``ForceField``); ``forces_fn`` must return ``(energy, forces,
    stress [B', 3, 3])`` with the stress in eV/A^3 and ASE's sign (d E / d strain / volume), used as given.  The cells and
    positions it gets change from step to step."""
    B = len(positions)
    if B == 0 or len(lattices) != B:
        raise ValueError(f"relax: {len(lattices)} lattices for {B} position arrays (need the same number, at least one)")
    if steps < 0 or fmax < 0 or maxstep <= 0 or dt <= 0:
        raise ValueError("relax: need steps >= 0, fmax >= 0, maxstep > 0, dt > 0")
    if forces_fn is None:
        from .alignn_atomwise import ALIGNNAtomWise

        if not isinstance(model, ALIGNNAtomWise):
            raise TypeError(f"relax: the model must be an ALIGNNAtomWise, got {type(model).__name__} (or pass forces_fn)")
        if not model.config.calculate_gradient:
            raise ValueError("relax: the model has calculate_gradient=False and predicts no forces")
        if model.training:
            raise ValueError("relax: the model is in training mode; call model.eval() first")
        if atom_features is None or len(atom_features) != B:
            raise ValueError("relax: the model needs atom_features, one [n_i, F] array per structure")
        if optimize_lattice and (model.config.stresswise_weight == 0 or not model.config.batch_stress):
            raise ValueError("relax: optimize_lattice needs per-crystal stresses: a model with stresswise_weight != 0 and "
                             "batch_stress=True")
        dev = model.fc.weight.device
    else:
        dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    if dev.type != "cuda":
        raise TypeError(f"relax runs on the GPU (csrc/relax.hip), got device {dev}")
    lib = _lib.load()

    with _lib.device_guard(torch.empty(0, device=dev)):
        lat = torch.stack([torch.as_tensor(x).to(dev, torch.float64) for x in lattices])
        if lat.shape != (B, 3, 3):
            raise ValueError(f"relax: lattices must be B x [3, 3], got {tuple(lat.shape)}")
        pos_in = [torch.as_tensor(p).to(dev, torch.float64) for p in positions]
        ns = [int(p.shape[0]) for p in pos_in]
        if any(p.dim() != 2 or p.shape[1] != 3 or p.shape[0] < 1 for p in pos_in):
            raise ValueError("relax: every position array must be [n_i, 3] with n_i >= 1")
        feats = None
        if forces_fn is None:
            feats = [torch.as_tensor(f).to(dev, torch.float32) for f in atom_features]
            F_in = model.config.atom_input_features
            for i, f in enumerate(feats):
                if f.dim() != 2 or f.shape[0] != ns[i] or f.shape[1] != F_in:
                    raise ValueError(f"relax: atom_features[{i}] is {tuple(f.shape)}, need [{ns[i]}, {F_in}]")
        ptr_h = [0]
        for n in ns:
            ptr_h.append(ptr_h[-1] + n)
        atom_ptr = torch.tensor(ptr_h, dtype=torch.int32, device=dev)
        inv = torch.linalg.inv(lat).contiguous()
        pos = torch.cat(pos_in).contiguous()
        site = torch.repeat_interleave(torch.arange(B, device=dev), torch.tensor(ns, device=dev))
        frac = _wrap(torch.bmm(pos.unsqueeze(1), inv[site]).squeeze(1)).contiguous()
        vel = torch.zeros_like(pos)
        forces_all = torch.zeros_like(pos)
        energy_all = torch.zeros(B, dtype=torch.float64, device=dev)
        fmax_all = torch.zeros(B, dtype=torch.float64, device=dev)
        state = torch.tensor([[float(dt), float(a)]] * B, dtype=torch.float64, device=dev)  # dt, a
        istate = torch.zeros(B, 2, dtype=torch.int32, device=dev)  # Nsteps, steps taken
        status = torch.empty(1 + B, dtype=torch.int32, device=dev)
        if optimize_lattice:  # ExpCellFilter's state: X_a, X_c = n logm(F), cell velocities, F, the current cell
            xa = pos.clone()
            xc = torch.zeros(B, 3, 3, dtype=torch.float64, device=dev)
            cvel = torch.zeros_like(xc)
            defgrad = torch.eye(3, dtype=torch.float64, device=dev).repeat(B, 1, 1).contiguous()
            lat_cur = lat.clone()
            stress_all = torch.zeros_like(xc)
        # fixed per-structure views: the same lattice tensors every step keep neighbors' lattice tables cached
        lat_v = [lat[s] for s in range(B)]
        pos_v = [pos[ptr_h[s]:ptr_h[s + 1]] for s in range(B)]
        frac_v = [frac[ptr_h[s]:ptr_h[s + 1]] for s in range(B)]
        line_graph = forces_fn is None and len(model.alignn_layers) > 0

        flag = [0] * B
        active = list(range(B))
        n_evals = 0
        changed = True
        while active:
            Ba = len(active)
            if changed:
                n_act = [ns[s] for s in active]
                act_t = torch.tensor(active, dtype=torch.int32, device=dev)
                fp = [0]
                for n in n_act:
                    fp.append(fp[-1] + n)
                force_ptr = torch.tensor(fp, dtype=torch.int32, device=dev)
                n_act_t = torch.tensor(n_act, dtype=torch.float32, device=dev)
                changed = False
            if optimize_lattice:
                # fresh tensors every step: the kernel writes lat_cur through a raw pointer (no version bump), which the
                # lattice-table cache of neighbors would not see
                lat_now = lat_cur.clone()
                lat_act = [lat_now[s] for s in active]
            else:
                lat_act = [lat_v[s] for s in active]
            if forces_fn is None:
                batch = neighbors.crystal_batch(lat_act, [frac_v[s] for s in active],
                                                atom_features=[feats[s] for s in active], device=dev, cutoff=cutoff,
                                                max_neighbors=max_neighbors, line_graph=line_graph,
                                                neighbor_strategy=neighbor_strategy)
                with torch.enable_grad():  # (the force head differentiates the energy)
                    res = model(batch)
                out = res["out"].detach().reshape(-1).float()
                energy = ((out * n_act_t) if intensive else out).double()
                forces = (res["grad"].detach().reshape(-1, 3) * force_multiplier).double()
                if optimize_lattice:  # the calculator: voigt (symmetrised) stress * stress_wt / 160.21766208, float32
                    st = res["stresses"].detach().reshape(-1, 3, 3).float()
                    stress = ((st + st.transpose(1, 2)) / 2 * stress_weight / 160.21766208).double()
            elif optimize_lattice:
                out = forces_fn(lat_act, [pos_v[s] for s in active])
                if not isinstance(out, (tuple, list)) or len(out) != 3:
                    raise ValueError("relax: with optimize_lattice, forces_fn must return (energy, forces, stress)")
                energy, forces, stress = out
                energy = torch.as_tensor(energy).to(dev, torch.float64).reshape(-1)
                forces = torch.as_tensor(forces).to(dev, torch.float64).reshape(-1, 3)
                stress = torch.as_tensor(stress).to(dev, torch.float64)
            else:
                energy, forces = forces_fn(lat_act, [pos_v[s] for s in active])
                energy = torch.as_tensor(energy).to(dev, torch.float64).reshape(-1)
                forces = torch.as_tensor(forces).to(dev, torch.float64).reshape(-1, 3)
            if energy.numel() != Ba or forces.shape[0] != fp[-1]:
                raise ValueError(f"relax: evaluation returned {energy.numel()} energies / {forces.shape[0]} force rows for "
                                 f"{Ba} structures / {fp[-1]} atoms")
            energy, forces = energy.contiguous(), forces.contiguous()
            n_evals += 1
            if optimize_lattice:
                if stress.shape != (Ba, 3, 3):
                    raise ValueError(f"relax: evaluation returned stresses of shape {tuple(stress.shape)} for {Ba} structures")
                stress = stress.contiguous()
                _lib.check(lib.alignn_fire_cell_step(
                    forces.data_ptr(), energy.data_ptr(), stress.data_ptr(), force_ptr.data_ptr(), act_t.data_ptr(), Ba,
                    atom_ptr.data_ptr(), lat.data_ptr(), inv.data_ptr(), xa.data_ptr(), pos.data_ptr(), vel.data_ptr(),
                    frac.data_ptr(), xc.data_ptr(), cvel.data_ptr(), defgrad.data_ptr(), lat_cur.data_ptr(), forces_all.data_ptr(),
                    energy_all.data_ptr(), stress_all.data_ptr(), state.data_ptr(), istate.data_ptr(), fmax_all.data_ptr(),
                    status.data_ptr(), float(fmax), int(steps), float(maxstep), float(dtmax), int(Nmin), float(finc), float(fdec),
                    float(astart), float(fa), _lib.stream()), "fire_cell_step")
            else:
                _lib.check(lib.alignn_fire_step(forces.data_ptr(), energy.data_ptr(), force_ptr.data_ptr(), act_t.data_ptr(), Ba,
                                                atom_ptr.data_ptr(), inv.data_ptr(), pos.data_ptr(), vel.data_ptr(), frac.data_ptr(),
                                                forces_all.data_ptr(), energy_all.data_ptr(), state.data_ptr(), istate.data_ptr(),
                                                fmax_all.data_ptr(), status.data_ptr(), float(fmax), int(steps), float(maxstep),
                                                float(dtmax), int(Nmin), float(finc), float(fdec), float(astart), float(fa),
                                                _lib.stream()), "fire_step")
            st = status[:1 + Ba].tolist()  # the one host read of a step
            if st[0] == Ba:
                continue
            if min(st[1:]) < 0:
                raise RuntimeError("relax: fire_step found force rows that do not match a structure's atom count")
            for s, f in zip(active, st[1:]):
                flag[s] = f
            active = [s for s, f in zip(active, st[1:]) if f == 0]
            changed = True

        return RelaxResult(positions=[p.clone() for p in pos_v], energies=energy_all,
                           forces=[forces_all[ptr_h[s]:ptr_h[s + 1]].clone() for s in range(B)], fmax=fmax_all,
                           converged=torch.tensor([f == 1 for f in flag], device=dev), n_steps=istate[:, 1].long(),
                           n_evals=n_evals, lattices=lat_cur.clone() if optimize_lattice else None,
                           stresses=stress_all if optimize_lattice else None)
