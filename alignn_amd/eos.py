"""Batched energy-volume curves with the equation-of-state fit on the device.

The reference's ``ev_curve`` (alignn/ff/ff.py:762-805) takes one crystal: per strain ``dx`` it builds ``atoms.strain_atoms(dx)``
(jarvis-tools), loads a new ``ForceField`` and evaluates it, then fits ASE's ``EquationOfState(vol, e, eos="murnaghan")`` - two
``scipy.optimize.curve_fit`` calls on the host - and reports the bulk modulus in GPa.  Here, for B parent crystals and K strains
together:

1. ``alignn_strain_build`` (csrc/eos.hip) writes the cells, Cartesian positions and volumes of all B K strained structures in
   one launch; job (s, k) is parent s at ``dx[k]``, a parent's jobs consecutive;
2. ``relax(..., steps=0)`` evaluates them, in groups of whole jobs of at most ``max_atoms_per_call`` atoms (the grouping of
   alignn_amd/_jobs.py); a job's atom features are its parent's;
3. ``alignn_eos_fit`` fits every parent's curve in one launch, one wavefront per parent: ASE's parabola start, then
   Levenberg-Marquardt with the analytic Jacobian.  Volumes, energies and fit results stay on the device until the result is
   assembled (one copy of each array).

The kernels are float64 with fixed-order sums and ``relax`` keeps a structure's bits independent of its batch, so a parent's
numbers are the same whatever else is in the call.  tests/eos_ref.py restates the builder and the fit in numpy.

The strained structure is the parent with its cell and positions multiplied by F = (1 + dx) I: the fractional coordinates stay,
the volume is (1 + dx)^3 V.  For cells whose matrix is diagonal this is jarvis-tools' ``Atoms.strain_atoms(dx)``; jarvis-tools
is not a dependency of this project and was not available to compare against, so nothing is claimed for other cells.  The
builder itself takes a general F (shear included).
"""

from __future__ import annotations

from dataclasses import dataclass
from typing import Callable, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib
from ._jobs import (EVALUATION, MAX_ATOMS_PER_CALL, check_max_atoms, evaluation_options, features, prepare_parents,
                    relax_jobs, strain_jobs)
from ._structures import EV_A3_TO_GPA, check_inputs, gpu_device

__all__ = ["ev_curve", "eos_fit", "EVResult", "EOS_FORMS", "EV_A3_TO_GPA"]

EOS_FORMS = {"murnaghan": 0, "birchmurnaghan": 1}  # ase/eos.py's names -> the kernel's ``form``
MIN_POINTS, MAX_POINTS = 4, 64  # four parameters; one lane of a wavefront per point


@dataclass
class EVResult:
    """Per parent s, in the input order.  ``volumes[s, k]`` (A^3) and ``energies[s, k]`` (eV) are those of the parent strained
    by ``dx[k]``; ``e0`` (eV), ``b0`` (eV/A^3), ``bp`` and ``v0`` (A^3) the fitted parameters, ``bulk_modulus_GPa = b0 *
    160.21766208``; ``rms`` the root mean square residual of the fit (eV), ``n_iter`` its steps, ``status`` 0 (converged), 1
    (stopped after 100 steps, the parameters as they stood) or 2 (no fit: the least-squares parabola through the points has no
    minimum, or a value is not finite; the fit fields are NaN).  ``lattices`` / ``positions`` are the parents the curve was
    taken on (the relaxed ones with ``on_relaxed_struct``), ``n_eval_calls`` the number of batched evaluation calls."""

    dx: np.ndarray  # [K]
    volumes: np.ndarray  # [B, K]
    energies: np.ndarray  # [B, K]
    e0: np.ndarray  # [B]
    b0: np.ndarray
    bp: np.ndarray
    v0: np.ndarray
    bulk_modulus_GPa: np.ndarray
    rms: np.ndarray
    n_iter: np.ndarray  # [B] int
    status: np.ndarray  # [B] int
    lattices: torch.Tensor  # [B, 3, 3] float64
    positions: List[torch.Tensor]  # [n_s, 3] float64
    n_eval_calls: int


def eos_fit(volumes: torch.Tensor, energies: torch.Tensor, eos: str = "murnaghan",
            n_points: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """The fit launch alone: ``volumes`` / ``energies`` [B, K] float64 on the GPU (4 <= K <= 64; structure s uses its first
    ``n_points[s]`` points where given, int32 [B]) -> (params [B, 4] = (E0, B0, BP, V0), rms [B], n_iter [B], status [B]) on
    the device, as ``EVResult`` describes them."""
    if eos not in EOS_FORMS:
        raise ValueError(f"eos_fit: eos must be one of {sorted(EOS_FORMS)}, got {eos!r}")
    if volumes.ndim != 2 or volumes.shape != energies.shape or not MIN_POINTS <= volumes.shape[1] <= MAX_POINTS:
        raise ValueError(f"eos_fit: volumes and energies must both be [B, K] with {MIN_POINTS} <= K <= {MAX_POINTS}, got "
                         f"{tuple(volumes.shape)} and {tuple(energies.shape)}")
    for name, t in (("volumes", volumes), ("energies", energies)):
        if t.dtype != torch.float64 or not t.is_cuda:
            raise TypeError(f"eos_fit: {name} must be a float64 tensor on the GPU, got {t.dtype} on {t.device}")
    B, K = volumes.shape
    if n_points is not None and (n_points.dtype != torch.int32 or n_points.shape != (B,) or n_points.device != volumes.device):
        raise ValueError(f"eos_fit: n_points must be int32 [{B}] on {volumes.device}")
    dev = volumes.device
    lib = _lib.load()
    with _lib.device_guard(volumes):
        volumes, energies = volumes.contiguous(), energies.contiguous()
        params = torch.empty(B, 4, dtype=torch.float64, device=dev)
        rms = torch.empty(B, dtype=torch.float64, device=dev)
        n_iter = torch.empty(B, dtype=torch.int32, device=dev)
        status = torch.empty(B, dtype=torch.int32, device=dev)
        _lib.check(lib.alignn_eos_fit(volumes.data_ptr(), energies.data_ptr(), _lib.ptr(n_points), B, K, EOS_FORMS[eos],
                                      params.data_ptr(), rms.data_ptr(), n_iter.data_ptr(), status.data_ptr(), _lib.stream()),
                   "eos_fit")
    return params, rms, n_iter, status


def _check_dx(who: str, dx) -> np.ndarray:
    try:
        d = np.asarray(dx, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError(f"{who}: dx must be a 1-D array of strains, got {dx!r}") from None
    if d.ndim != 1:
        raise ValueError(f"{who}: dx must be 1-D, got shape {d.shape}")
    if not MIN_POINTS <= len(d) <= MAX_POINTS:
        raise ValueError(f"{who}: dx needs {MIN_POINTS} to {MAX_POINTS} strains (four fit parameters, one lane per point), got "
                         f"{len(d)}")
    if not np.isfinite(d).all():
        raise ValueError(f"{who}: dx must be finite")
    if (d <= -1.0).any():
        raise ValueError(f"{who}: every dx must be > -1 (the cell is scaled by 1 + dx)")
    if len(np.unique(d)) != len(d):
        raise ValueError(f"{who}: the strains of dx must be distinct")
    return d


def ev_curve(model, lattices: Sequence, positions: Sequence, atom_features: Optional[Sequence] = None, *,
             dx=np.arange(-0.05, 0.05, 0.01), eos: str = "murnaghan", on_relaxed_struct: bool = False,
             max_atoms_per_call: int = MAX_ATOMS_PER_CALL, forces_fn: Optional[Callable] = None, device=None,
             **relax_kwargs) -> EVResult:
    """Energy-volume curves and equation-of-state fits of B crystals, the reference's ``ev_curve`` (ff.py:762) for each: the
    parent strained isotropically by every ``dx[k]`` (cell and positions times 1 + dx), all B K structures evaluated together,
    every curve fitted on the device.

    The structures, the model (or ``forces_fn``) and the device: alignn_amd/_structures.py.  ``dx``: K distinct strains > -1, 4
    <= K <= 64; the default is the reference's ten.  ``eos``: "murnaghan" (the reference's) or "birchmurnaghan", as ase/eos.py
    states them.  ``max_atoms_per_call``: atoms per evaluation call (whole jobs).

    ``on_relaxed_struct``: first one ``relax`` call on the B parents, with ``relax_kwargs`` and the defaults ``steps=100``,
    ``fmax=0.1``, ``optimize_lattice=True`` of the reference's ``optimize_atoms()`` (the model, or ``forces_fn``, must then
    give stresses, and the evaluations of the curve ask for them as well, so that a ``forces_fn`` has one form of result
    throughout; they are not used); the curve is taken on the relaxed cells and positions.  Without it ``relax_kwargs`` may
    only hold the evaluation options ``cutoff``, ``max_neighbors``, ``neighbor_strategy``, ``intensive`` and
    ``force_multiplier``, which reach every evaluation in both cases.

    A curve need not have a minimum inside the strains (``status``, ``EVResult``); its volumes and energies are returned
    whatever the fit says."""
    who = "ev_curve"
    if not isinstance(on_relaxed_struct, (bool, np.bool_)):
        raise ValueError(f"{who}: on_relaxed_struct is one bool, got {type(on_relaxed_struct).__name__}")
    optimize_lattice = bool(on_relaxed_struct) and bool(relax_kwargs.get("optimize_lattice", True))
    ns = check_inputs(who, model, lattices, positions, atom_features, forces_fn=forces_fn, stress=optimize_lattice)
    B = len(ns)
    d = _check_dx(who, dx)
    K = len(d)
    if eos not in EOS_FORMS:
        raise ValueError(f"{who}: eos must be one of {sorted(EOS_FORMS)}, got {eos!r}")
    check_max_atoms(who, max_atoms_per_call)
    evaluation = evaluation_options(who, relax_kwargs, EVALUATION, on_relaxed_struct)
    dev = gpu_device(who, model, forces_fn, device)

    with _lib.device_guard(torch.empty(0, device=dev)):
        packed, lat_out, pos_out = prepare_parents(model, lattices, positions, atom_features, ns, on_relaxed_struct, relax_kwargs,
                                                   forces_fn, dev)
        scale = torch.tensor(1.0 + d, dtype=torch.float64, device=dev)  # (1 + dx in float64, as the restatement takes it)
        cells, cart, volumes, src, counts = strain_jobs(
            packed, ns, scale[:, None, None] * torch.eye(3, dtype=torch.float64, device=dev), dev)
        r = relax_jobs(model, cells, cart, src, counts, features(atom_features, forces_fn, dev), max_atoms_per_call, False,
                       dict(evaluation, optimize_lattice=optimize_lattice), forces_fn, dev)
        volumes, energies = volumes.reshape(B, K), r.energies.reshape(B, K).contiguous()
        params, rms, n_iter, status = eos_fit(volumes, energies, eos)
        params_h = params.cpu().numpy()
    return EVResult(dx=d, volumes=volumes.cpu().numpy(), energies=energies.cpu().numpy(), e0=params_h[:, 0].copy(),
                    b0=params_h[:, 1].copy(), bp=params_h[:, 2].copy(), v0=params_h[:, 3].copy(),
                    bulk_modulus_GPa=params_h[:, 1] * EV_A3_TO_GPA, rms=rms.cpu().numpy(),
                    n_iter=n_iter.cpu().numpy().astype(np.int64), status=status.cpu().numpy().astype(np.int64), lattices=lat_out,
                    positions=pos_out, n_eval_calls=r.n_calls)
