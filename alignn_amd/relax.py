"""Batched fixed-cell structure relaxation with FIRE, optimiser state on the device.

The reference relaxes one structure at a time: ``ForceField.optimize_atoms`` (alignn/ff/ff.py:373-415) wraps ASE's ``FIRE``
around ``AlignnAtomwiseCalculator`` (alignn/ff/calculators.py:280-370), one host round trip per step, and its callers
(``ev_curve``, ``vacancy_formation``, ``surface_energy``, ``get_interface_energy``: ff.py:762-1070) loop over structures.
``relax`` runs the same optimiser (``optimize_lattice=False``, ``downhill_check=False``) for a whole batch:

1. build the graph batch of the ACTIVE structures on the device (``neighbors.crystal_batch``, the line graph only when the
   model has ALIGNN layers);
2. evaluate energies and forces with ``model(batch)`` (the fused ``alignn_ff_eval`` path wherever it applies);
3. one ``alignn_fire_step`` launch (csrc/relax.hip; its argument block ``alignn_fire_args`` is filled once, a step sets the
   evaluation's pointers and, when structures have retired, the active list): convergence test of ``Optimizer.run`` (max_i |F_i|^2 < fmax^2), then
   the FIRE update of every unconverged structure, wrapped fractional coordinates for the next neighbour search;
4. read the number of structures still active and their retire flags (one small host read), drop the retired ones.

Positions, velocities, ``dt``, ``a`` and ``Nsteps`` of every structure stay on the device in float64.  A structure's step
depends only on its own forces and state (fixed-order reductions): its trajectory is the same bits whether it is relaxed
alone or beside others.

``optimize_lattice=True`` relaxes the cells too, as ``optimize_atoms``' default does: ASE's ``ExpCellFilter`` around the atoms,
its n + 3 generalised rows per structure (atom rows in the starting cell, cell rows ``n logm(F)`` of the deformation gradient
``F``) driven by the same FIRE in the same ``alignn_fire_step`` (the filter's state in its argument block selects it).  The
model's per-crystal stresses enter as the calculator gives them (``stress * stress_weight / 160.21766208``, eV/A^3).

Constraints, as ASE states them: ``fixed`` is ``FixAtoms`` (those atoms' force rows are zero to the optimiser and to the
convergence test; at fixed cell they stay where they are, under the filter they ride with the cell), and ``cell_mask``,
``hydrostatic_strain``, ``constant_volume`` and ``scalar_pressure`` are ``ExpCellFilter``'s arguments.  They are fields of the
same argument block, passed only when they are on: the same kernel, and without them the same bits as before.
"""

from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Callable, List, Optional, Sequence

import numpy as np
import torch

from . import _lib
from ._structures import ForceEvaluator, check_inputs, gpu_device, host, pack

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
    enthalpies: Optional[torch.Tensor] = None  # [B] float64: energy + scalar_pressure * volume (optimize_lattice only)


def _full_mask(m, what: str) -> np.ndarray:
    """One cell mask, six Voigt flags (xx, yy, zz, yz, xz, xy) or [3, 3], as the full 3 x 3 of 0.0 / 1.0 (ASE's
    voigt_6_to_full_3x3_stress for the Voigt form)."""
    m = host(m)
    if m.shape == (6,):
        xx, yy, zz, yz, xz, xy = m
        m = np.array([[xx, xy, xz], [xy, yy, yz], [xz, yz, zz]])
    elif m.shape != (3, 3):
        raise ValueError(f"relax: {what} is {m.shape}, need six Voigt flags or [3, 3]")
    if m.dtype == object or not np.isin(m, (0, 1)).all():
        raise ValueError(f"relax: {what} must hold 0 / 1 only")
    return m.astype(np.float64)


def _constraints(ns: List[int], fixed, cell_mask, hydrostatic_strain, constant_volume, scalar_pressure, optimize_lattice):
    """The host-side checks of the constraint arguments -> (fixed [N] bool or None, masks [B, 3, 3] or None, pressures [B] or
    None), None where the option is off (no atom fixed, every mask all ones, every pressure zero)."""
    B = len(ns)
    for name, v in (("hydrostatic_strain", hydrostatic_strain), ("constant_volume", constant_volume)):
        if not isinstance(v, (bool, np.bool_)):
            raise ValueError(f"relax: {name} is one bool for the whole call, got {type(v).__name__}")
    fix = None
    if fixed is not None:
        if isinstance(fixed, (torch.Tensor, np.ndarray)) and fixed.ndim != 2 or len(fixed) != B:
            raise ValueError(f"relax: fixed needs one boolean [n_i] array (or None) per structure, {B} of them")
        rows = []
        for i, f in enumerate(fixed):
            f = np.zeros(ns[i], dtype=bool) if f is None else host(f)
            if f.shape != (ns[i],) or f.dtype != np.bool_:
                raise ValueError(f"relax: fixed[{i}] is {f.dtype} {f.shape}, need bool [{ns[i]}]")
            rows.append(f)
        fix = np.concatenate(rows)
        fix = fix if fix.any() else None
    masks = None
    if cell_mask is not None:
        shape = None
        try:
            shape = host(cell_mask).shape
        except (ValueError, TypeError):  # a ragged list: Voigt and [3, 3] masks mixed
            pass
        if shape in ((6,), (3, 3)):  # one mask for every structure
            masks = np.stack([_full_mask(cell_mask, "cell_mask")] * B)
        elif shape is not None and len(shape) < 2 or len(cell_mask) != B:
            raise ValueError(f"relax: cell_mask needs one mask (six Voigt flags or [3, 3]) or {B} of them")
        else:
            masks = np.stack([_full_mask(m, f"cell_mask[{i}]") for i, m in enumerate(cell_mask)])
    press = host(scalar_pressure)
    if press.dtype.kind not in "iuf" or press.shape not in ((), (B,)):
        raise ValueError(f"relax: scalar_pressure needs one number or {B} of them (eV/A^3)")
    press = np.broadcast_to(press.astype(np.float64), (B,)).copy()
    if not np.isfinite(press).all():
        raise ValueError("relax: scalar_pressure must be finite")
    if not optimize_lattice and (masks is not None or hydrostatic_strain or constant_volume or press.any()):
        raise ValueError("relax: cell_mask, hydrostatic_strain, constant_volume and a non-zero scalar_pressure need "
                         "optimize_lattice=True")
    return fix, None if masks is None or (masks == 1.0).all() else masks, press if press.any() else None


def relax(model, lattices: Sequence, positions: Sequence, atom_features: Optional[Sequence] = None, *, fmax: float = 0.1,
          steps: int = 100, dt: float = 0.1, maxstep: float = 0.2, dtmax: float = 1.0, Nmin: int = 5, finc: float = 1.1,
          fdec: float = 0.5, astart: float = 0.1, fa: float = 0.99, a: float = 0.1, cutoff: float = 8.0, max_neighbors: int = 12,
          neighbor_strategy: str = "k-nearest", intensive: bool = True, force_multiplier: float = 1.0,
          forces_fn: Optional[Callable] = None, device=None, optimize_lattice: bool = False,
          stress_weight: float = 1.0, fixed: Optional[Sequence] = None, cell_mask=None, hydrostatic_strain: bool = False,
          constant_volume: bool = False, scalar_pressure=0.0, evaluator: Optional[Callable] = None) -> RelaxResult:
    """Relax the atomic positions of B crystals with FIRE until max_i |F_i| < ``fmax`` or ``steps`` steps; at fixed cell, or
    with the cells too when ``optimize_lattice``.

    The structures, the model (or ``forces_fn``), ``cutoff`` ... ``force_multiplier`` and the device: alignn_amd/_structures.py.
    ``forces_fn`` gets the active structures.  ``dt`` ... ``a``: FIRE's parameters, ASE's defaults (ase/optimize/fire.py).

    ``optimize_lattice``: relax the cells as well, through ASE's ``ExpCellFilter`` (default arguments).  The reference's
    ``optimize_atoms`` defaults to ``optimize_lattice=True``; here the default stays ``False``.  The model must then predict
    per-crystal stresses, scaled by ``stress_weight``; ``forces_fn`` must return ``(energy, forces, stress)``.  The cells and
    positions it gets change from step to step.

    ``fixed``: ASE's ``FixAtoms``, B boolean arrays [n_i] (``None`` for a structure: none of its atoms), with or without
    ``optimize_lattice``.  The optimiser and the convergence test see zero force rows for these atoms (``fmax`` of the result
    too; ``forces`` stay the forces as evaluated).  At fixed cell a fixed atom does not move; under the filter it keeps its
    place in the cell and moves with it.

    ``cell_mask``, ``hydrostatic_strain``, ``constant_volume``, ``scalar_pressure``: ``ExpCellFilter``'s arguments of these
    names (``cell_mask`` its ``mask``); they need ``optimize_lattice``.  ``cell_mask``: which cell components may relax, six
    Voigt flags (xx, yy, zz, yz, xz, xy) or a [3, 3] array of 0 / 1, one for all structures or B of them (a [3, 3] array is
    always one mask).  ``scalar_pressure``: the target pressure in eV/A^3, ASE's unit (``dynamics.BAR`` converts from bar),
    one number or B; the run then minimises the enthalpy ``E + scalar_pressure * V``, returned as ``enthalpies``.

    ``evaluator``: an object called exactly as ``ForceEvaluator`` is, ``(which, lattices, frac, cart) -> (energy, forces,
    stress)`` with ``which`` the active structures' indices, ``frac`` the wrapped fractional coordinates the step kernel wrote
    and ``cart`` views of the packed position array; it replaces the evaluator built from the model or ``forces_fn``, and
    ``model`` may then be ``None`` (``alignn_amd.neb`` turns the forces of a band's images into NEB forces this way)."""
    if evaluator is not None:
        forces_fn = evaluator  # (to the checks below: no model needed, the device is ``device`` or the current one)
    ns = check_inputs("relax", model, lattices, positions, atom_features, forces_fn=forces_fn, stress=optimize_lattice)
    if steps < 0 or fmax < 0 or maxstep <= 0 or dt <= 0:
        raise ValueError("relax: need steps >= 0, fmax >= 0, maxstep > 0, dt > 0")
    fix, masks, press = _constraints(ns, fixed, cell_mask, hydrostatic_strain, constant_volume, scalar_pressure,
                                     optimize_lattice)
    dev = gpu_device("relax", model, forces_fn, device)
    lib = _lib.load()
    B = len(ns)

    with _lib.device_guard(torch.empty(0, device=dev)):
        packed = pack(lattices, positions, ns, dev)
        lat, pos, inv, frac, atom_ptr = packed.lat, packed.pos, packed.inv, packed.frac, packed.atom_ptr
        evaluate = evaluator if evaluator is not None else ForceEvaluator(
            "relax", model, forces_fn, atom_features, ns, dev, cutoff=cutoff, max_neighbors=max_neighbors,
            neighbor_strategy=neighbor_strategy, intensive=intensive, force_multiplier=force_multiplier,
            stress_weight=stress_weight if optimize_lattice else None)
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
            enthalpy_all = torch.zeros(B, dtype=torch.float64, device=dev)
        # the constraints that are on (None: a NULL field)
        fix_t = None if fix is None else torch.tensor(fix.astype(np.uint8), device=dev)
        mask_t = None if masks is None else torch.tensor(masks, dtype=torch.float64, device=dev)
        press_t = None if press is None else torch.tensor(press, dtype=torch.float64, device=dev)
        # fixed per-structure views: the same lattice tensors every step keep neighbors' lattice tables cached
        lat_v = [lat[s] for s in range(B)]
        pos_v, frac_v = packed.rows(pos), packed.rows(frac)

        args = _lib.FireArgs(
            atom_ptr=atom_ptr.data_ptr(), inv_lattice=inv.data_ptr(), positions=pos.data_ptr(), velocities=vel.data_ptr(),
            frac=frac.data_ptr(), state=state.data_ptr(), istate=istate.data_ptr(), forces_out=forces_all.data_ptr(),
            energy_out=energy_all.data_ptr(), fmax_out=fmax_all.data_ptr(), status=status.data_ptr(), steps=int(steps),
            nmin=int(Nmin), fmax=float(fmax), maxstep=float(maxstep), dtmax=float(dtmax), finc=float(finc), fdec=float(fdec),
            astart=float(astart), fa=float(fa), fixed=_lib.ptr(fix_t), cell_mask=_lib.ptr(mask_t),
            scalar_pressure=_lib.ptr(press_t), hydrostatic_strain=int(hydrostatic_strain), constant_volume=int(constant_volume))
        if optimize_lattice:
            args.enthalpy_out = enthalpy_all.data_ptr()
            args.lattice0, args.xa, args.xc, args.cell_velocities = lat.data_ptr(), xa.data_ptr(), xc.data_ptr(), cvel.data_ptr()
            args.defgrad, args.lattice, args.stress_out = defgrad.data_ptr(), lat_cur.data_ptr(), stress_all.data_ptr()

        flag = [0] * B
        active = list(range(B))
        n_evals = 0
        changed = True
        while active:
            Ba = len(active)
            if changed:
                act_t = torch.tensor(active, dtype=torch.int32, device=dev)
                fp = [0]
                for s in active:
                    fp.append(fp[-1] + ns[s])
                force_ptr = torch.tensor(fp, dtype=torch.int32, device=dev)
                args.active, args.n_active, args.force_ptr = act_t.data_ptr(), Ba, force_ptr.data_ptr()
                changed = False
            if optimize_lattice:
                # fresh tensors every step: the kernel writes lat_cur through a raw pointer (no version bump), which the
                # lattice-table cache of neighbors would not see
                lat_now = lat_cur.clone()
                lat_act = [lat_now[s] for s in active]
            else:
                lat_act = [lat_v[s] for s in active]
            energy, forces, stress = evaluate(active, lat_act, [frac_v[s] for s in active], [pos_v[s] for s in active])
            n_evals += 1
            args.forces, args.energy, args.stress = forces.data_ptr(), energy.data_ptr(), _lib.ptr(stress)
            _lib.check(lib.alignn_fire_step(C.byref(args), _lib.stream()), "fire_step")
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
                           forces=[f.clone() for f in packed.rows(forces_all)], fmax=fmax_all,
                           converged=torch.tensor([f == 1 for f in flag], device=dev), n_steps=istate[:, 1].long(),
                           n_evals=n_evals, lattices=lat_cur.clone() if optimize_lattice else None,
                           stresses=stress_all if optimize_lattice else None,
                           enthalpies=enthalpy_all if optimize_lattice else None)
