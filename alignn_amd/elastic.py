"""Batched elastic tensors: the strained cells built and evaluated together, the stress-strain fit on the device.

The reference has ``ev_curve`` (alignn/ff/ff.py:762-805) for the bulk modulus and no elastic-tensor function; a user would loop
over a few dozen strained copies of a crystal on the host and fit the stresses with numpy.  Here, for B parent crystals and P
strain points together:

1. ``alignn_strain_build`` (csrc/eos.hip) writes the cells and Cartesian positions of all B P strained structures in one
   launch; job (s, p) is parent s under F = I + eps(p), a parent's jobs consecutive;
2. ``relax(..., optimize_lattice=True)`` evaluates them, in groups of whole jobs of at most ``max_atoms_per_call`` atoms (the
   grouping of alignn_amd/_jobs.py): ``steps=0`` for clamped ions, or FIRE at a fixed cell (``cell_mask`` all zero) with
   ``relax_ions``; either way it returns every structure's symmetrised stress;
3. ``alignn_elastic_fit`` (csrc/elastic.hip) fits sigma_i = sigma0_i + sum_j C_ij eps_j for every parent in one launch, one
   wavefront per parent, and derives the compliance and the Voigt-Reuss-Hill moduli.  Strains, stresses and fit results stay
   on the device until the result is assembled (one copy of each array).

Conventions: Voigt order xx, yy, zz, yz, xz, xy; shear strains are engineering shears (gamma = 2 eps); stresses are ASE's sign
(positive under tension) in eV/A^3, ``*_GPa`` fields that times ``EV_A3_TO_GPA``.  The kernels are float64 with fixed-order sums
and ``relax`` keeps a structure's bits independent of its batch, so a parent's numbers are the same whatever else is in the
call.  tests/elastic_ref.py restates the strain set, the deformation and the fit in numpy.
"""

from __future__ import annotations

from dataclasses import dataclass
from typing import Callable, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib
from ._jobs import (EVALUATION, MAX_ATOMS_PER_CALL, check_max_atoms, check_steps_fmax, evaluation_options, features, prepare_parents,
                    relax_jobs, strain_jobs)
from ._structures import EV_A3_TO_GPA, check_inputs, gpu_device

__all__ = ["elastic_tensor", "elastic_fit", "ElasticResult", "MODULI", "DEFAULT_STRAINS"]

MIN_POINTS, MAX_POINTS = 7, 64  # seven unknowns per stress component; one lane of a wavefront per point
MAX_STRAIN = 0.2  # |strain| below this: the fit is linear in the strain
MODULI = ("k_voigt", "k_reuss", "k_hill", "g_voigt", "g_reuss", "g_hill", "youngs_modulus", "poisson_ratio",
          "universal_anisotropy")  # the columns of the kernel's ``moduli``
_EVALUATION = EVALUATION + ("stress_weight",)
_ION_RELAXATION = ("steps", "fmax")
DEFAULT_STRAINS = (-0.01, -0.005, 0.005, 0.01)


@dataclass
class ElasticResult:
    """Per parent s, in the input order.  ``strains[p]`` is the applied strain of point p (Voigt, engineering shear) and
    ``stresses[s, p]`` the Voigt stress (eV/A^3) of parent s under it.  ``c_raw`` is the fitted slope d sigma_i / d eps_j, ``c``
    its symmetric part, ``c_GPa = c * 160.21766208``, ``compliance = c^-1`` (A^3/eV), ``sigma0`` the fitted stress at zero
    strain.  ``k_*`` / ``g_*`` are the bulk and shear moduli in the Voigt, Reuss and Hill averages, ``youngs_modulus`` and
    ``poisson_ratio`` those of the Hill averages, ``universal_anisotropy = 5 G_V / G_R + K_V / K_R - 6``; the moduli are in
    eV/A^3 with ``*_GPa`` twins.  ``rms`` is the root mean square residual of the 6 P stress values (eV/A^3), ``asymmetry`` =
    max |c_raw - c_raw^T| / max |c_raw|.  ``status`` 0: fitted and ``c`` positive definite (Born stable); 1: fitted, ``c`` not
    positive definite (unstable): ``compliance`` and every modulus but ``k_voigt`` and ``g_voigt`` are NaN; 2: no fit (a
    non-finite stress, a rank-deficient strain set): every fit field is NaN.  ``converged`` / ``n_steps`` are those of the
    ion relaxation of every strained structure (``relax_ions``).  ``lattices`` / ``positions`` are the parents the tensor was
    taken on (the relaxed ones with ``on_relaxed_struct``), ``n_eval_calls`` the number of batched evaluation calls."""

    strains: np.ndarray  # [P, 6]
    stresses: np.ndarray  # [B, P, 6]
    c: np.ndarray  # [B, 6, 6]
    c_raw: np.ndarray
    compliance: np.ndarray
    c_GPa: np.ndarray
    sigma0: np.ndarray  # [B, 6]
    k_voigt: np.ndarray  # [B]
    k_reuss: np.ndarray
    k_hill: np.ndarray
    g_voigt: np.ndarray
    g_reuss: np.ndarray
    g_hill: np.ndarray
    youngs_modulus: np.ndarray
    poisson_ratio: np.ndarray
    universal_anisotropy: np.ndarray
    k_voigt_GPa: np.ndarray
    k_reuss_GPa: np.ndarray
    k_hill_GPa: np.ndarray
    g_voigt_GPa: np.ndarray
    g_reuss_GPa: np.ndarray
    g_hill_GPa: np.ndarray
    youngs_modulus_GPa: np.ndarray
    rms: np.ndarray
    asymmetry: np.ndarray
    status: np.ndarray  # [B] int
    converged: np.ndarray  # [B, P] bool
    n_steps: np.ndarray  # [B, P] int
    lattices: torch.Tensor  # [B, 3, 3] float64
    positions: List[torch.Tensor]  # [n_s, 3] float64
    n_eval_calls: int


def elastic_fit(strains: torch.Tensor, stresses: torch.Tensor, n_points: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, ...]:
    """The fit launch alone: ``strains`` [B, P, 6] (Voigt, engineering shear) and ``stresses`` [B, P, 3, 3] float64 on the GPU
    (7 <= P <= 64; crystal s uses its first ``n_points[s]`` points where given, int32 [B]) -> (c_raw [B, 6, 6], c [B, 6, 6],
    compliance [B, 6, 6], sigma0 [B, 6], moduli [B, 9] in the order of ``MODULI``, rms [B], asymmetry [B], status [B] int32) on
    the device, as ``ElasticResult`` describes them."""
    if strains.ndim != 3 or strains.shape[2] != 6 or stresses.shape != strains.shape[:2] + (3, 3) or \
            not MIN_POINTS <= strains.shape[1] <= MAX_POINTS:
        raise ValueError(f"elastic_fit: strains must be [B, P, 6] and stresses [B, P, 3, 3] with {MIN_POINTS} <= P <= "
                         f"{MAX_POINTS}, got {tuple(strains.shape)} and {tuple(stresses.shape)}")
    for name, t in (("strains", strains), ("stresses", stresses)):
        if t.dtype != torch.float64 or not t.is_cuda:
            raise TypeError(f"elastic_fit: {name} must be a float64 tensor on the GPU, got {t.dtype} on {t.device}")
    B, P = strains.shape[:2]
    if n_points is not None and (n_points.dtype != torch.int32 or n_points.shape != (B,) or n_points.device != strains.device):
        raise ValueError(f"elastic_fit: n_points must be int32 [{B}] on {strains.device}")
    dev = strains.device
    lib = _lib.load()
    with _lib.device_guard(strains):
        strains, stresses = strains.contiguous(), stresses.contiguous()
        new = lambda *shape: torch.empty(B, *shape, dtype=torch.float64, device=dev)
        c_raw, c, compliance, sigma0, moduli, rms, asymmetry = new(6, 6), new(6, 6), new(6, 6), new(6), new(9), new(), new()
        status = torch.empty(B, dtype=torch.int32, device=dev)
        _lib.check(lib.alignn_elastic_fit(strains.data_ptr(), stresses.data_ptr(), _lib.ptr(n_points), B, P, c_raw.data_ptr(),
                                          c.data_ptr(), compliance.data_ptr(), sigma0.data_ptr(), moduli.data_ptr(),
                                          rms.data_ptr(), asymmetry.data_ptr(), status.data_ptr(), _lib.stream()), "elastic_fit")
    return c_raw, c, compliance, sigma0, moduli, rms, asymmetry, status


def _strain_points(who: str, strains, strain_set) -> np.ndarray:
    """The [P, 6] Voigt strain points: ``strain_set`` as given, else the six single-component modes, each at every magnitude of
    ``strains`` (mode after mode)."""
    if strain_set is not None:
        if strains is not DEFAULT_STRAINS:
            raise ValueError(f"{who}: give strains (magnitudes of the six single-component modes) or strain_set, not both")
        try:
            e = np.asarray(strain_set, dtype=np.float64)
        except (TypeError, ValueError):
            raise ValueError(f"{who}: strain_set must be a [P, 6] array of Voigt strains, got {strain_set!r}") from None
        if e.ndim != 2 or e.shape[1] != 6 or not MIN_POINTS <= e.shape[0] <= MAX_POINTS:
            raise ValueError(f"{who}: strain_set must be [P, 6] with {MIN_POINTS} <= P <= {MAX_POINTS} (seven unknowns per "
                             f"stress component, one lane per point), got shape {e.shape}")
        if not (np.abs(e) < MAX_STRAIN).all():  # (a NaN fails it too)
            raise ValueError(f"{who}: every strain of strain_set must be finite with |strain| < {MAX_STRAIN}")
        return e.copy()
    try:
        m = np.asarray(strains, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError(f"{who}: strains must be a 1-D array of magnitudes, got {strains!r}") from None
    if m.ndim != 1:
        raise ValueError(f"{who}: strains must be 1-D, got shape {m.shape}")
    if not MIN_POINTS <= 6 * len(m) <= MAX_POINTS:
        raise ValueError(f"{who}: strains needs 2 to {MAX_POINTS // 6} magnitudes (six modes each, {MIN_POINTS} to {MAX_POINTS} "
                         f"points), got {len(m)}")
    if not (np.abs(m) < MAX_STRAIN).all() or (m == 0.0).any():
        raise ValueError(f"{who}: every magnitude of strains must be finite, non-zero and below {MAX_STRAIN}")
    if len(np.unique(m)) != len(m):
        raise ValueError(f"{who}: the magnitudes of strains must be distinct")
    e = np.zeros((6 * len(m), 6))
    for j in range(6):
        e[j * len(m):(j + 1) * len(m), j] = m
    return e


def _defgrad(e: np.ndarray) -> np.ndarray:
    """F = I + eps [P, 3, 3] of the Voigt strains e [P, 6]: eps_yz = gamma_yz / 2 and so on.  F is symmetric."""
    F = np.zeros((len(e), 3, 3))
    for i in range(3):
        F[:, i, i] = 1.0 + e[:, i]
    for k, (i, j) in ((3, (1, 2)), (4, (0, 2)), (5, (0, 1))):
        F[:, i, j] = F[:, j, i] = 0.5 * e[:, k]
    return F


def _voigt(stress: torch.Tensor) -> torch.Tensor:
    """[..., 3, 3] -> [..., 6], the off-diagonals the mean of the two stored halves (as the kernel takes them)."""
    s = stress
    return torch.stack([s[..., 0, 0], s[..., 1, 1], s[..., 2, 2], (s[..., 1, 2] + s[..., 2, 1]) * 0.5,
                        (s[..., 0, 2] + s[..., 2, 0]) * 0.5, (s[..., 0, 1] + s[..., 1, 0]) * 0.5], dim=-1)


def elastic_tensor(model, lattices: Sequence, positions: Sequence, atom_features: Optional[Sequence] = None, *,
                   strains=DEFAULT_STRAINS, strain_set=None, relax_ions: bool = False, on_relaxed_struct: bool = False,
                   max_atoms_per_call: int = MAX_ATOMS_PER_CALL, forces_fn: Optional[Callable] = None, device=None,
                   **relax_kwargs) -> ElasticResult:
    """Elastic tensors of B crystals from finite strains: every parent under each of P small strains, all B P structures
    evaluated together, sigma_i = sigma0_i + sum_j C_ij eps_j fitted per parent on the device.

    The structures, the model (or ``forces_fn``) and the device: alignn_amd/_structures.py.  The model, or ``forces_fn``, must
    give stresses.  ``strains``: the magnitudes (finite, non-zero, distinct, below 0.2) at which each of the six
    single-component Voigt modes is applied, for the shear modes the engineering shear gamma; the default (-0.01, -0.005,
    0.005, 0.01) gives P = 24 points.  ``strain_set``: a [P, 6] array of Voigt strains instead, 7 <= P <= 64, the same set for
    every parent.  The strained structure is the parent with cell and positions multiplied by the symmetric F = I + eps.
    ``max_atoms_per_call``: atoms per evaluation call (whole jobs).

    ``relax_ions``: relax the atoms of every strained structure at its fixed cell (FIRE under the cell filter with an
    all-zero ``cell_mask``; ``steps`` and ``fmax`` from ``relax_kwargs``, ``relax``'s defaults otherwise) and fit the stresses
    of the relaxed structures: the relaxed-ion tensor.  Without it the ions are clamped (they follow the strain affinely),
    which is the whole tensor only where every atom is an inversion centre.  ``converged`` tells which relaxations reached
    ``fmax``.

    ``on_relaxed_struct``: first one ``relax`` call on the B parents, with ``relax_kwargs`` and the defaults ``steps=100``,
    ``fmax=0.1``, ``optimize_lattice=True``; the tensor is taken on the relaxed cells and positions.  Without it and without
    ``relax_ions``, ``relax_kwargs`` may only hold the evaluation options ``cutoff``, ``max_neighbors``,
    ``neighbor_strategy``, ``intensive``, ``force_multiplier`` and ``stress_weight``, which reach every evaluation in all
    cases.

    C is the slope of the Cauchy stress against small strain at the parent's own state.  For a parent under residual stress
    (see ``sigma0``) these are stress-strain coefficients, which differ from second derivatives of the energy by terms of order
    sigma0; ``on_relaxed_struct=True`` is the way to the usual constants.  The model path's stresses are float32, so C
    carries a relative noise of about 1e-7 / |eps|.  ``status`` and the fit's quality: ``ElasticResult``; the stresses are
    returned whatever the fit says."""
    who = "elastic_tensor"
    for name, v in (("on_relaxed_struct", on_relaxed_struct), ("relax_ions", relax_ions)):
        if not isinstance(v, (bool, np.bool_)):
            raise ValueError(f"{who}: {name} is one bool, got {type(v).__name__}")
    ns = check_inputs(who, model, lattices, positions, atom_features, forces_fn=forces_fn, stress=True)
    B = len(ns)
    e = _strain_points(who, strains, strain_set)
    P = len(e)
    check_max_atoms(who, max_atoms_per_call)
    job_kw = evaluation_options(who, relax_kwargs, _EVALUATION, on_relaxed_struct, _ION_RELAXATION if relax_ions else ())
    check_steps_fmax(who, relax_kwargs)
    job_kw["optimize_lattice"] = True
    if relax_ions:
        job_kw.update({k: v for k, v in relax_kwargs.items() if k in _ION_RELAXATION})
        job_kw["cell_mask"] = np.zeros(6)
    dev = gpu_device(who, model, forces_fn, device)

    with _lib.device_guard(torch.empty(0, device=dev)):
        packed, lat_out, pos_out = prepare_parents(model, lattices, positions, atom_features, ns, on_relaxed_struct, relax_kwargs,
                                                   forces_fn, dev)
        e_d = torch.tensor(e, dtype=torch.float64, device=dev)
        cells, cart, _, src, counts = strain_jobs(packed, ns, torch.tensor(_defgrad(e), dtype=torch.float64, device=dev), dev)
        r = relax_jobs(model, cells, cart, src, counts, features(atom_features, forces_fn, dev), max_atoms_per_call,
                       bool(relax_ions), job_kw, forces_fn, dev)
        stress = r.stresses.reshape(B, P, 3, 3).contiguous()
        c_raw, c, compliance, sigma0, moduli, rms, asymmetry, status = elastic_fit(e_d.expand(B, P, 6), stress)
        c_h, moduli_h = c.cpu().numpy(), moduli.cpu().numpy()
    named = {name: moduli_h[:, k].copy() for k, name in enumerate(MODULI)}
    named.update({name + "_GPa": named[name] * EV_A3_TO_GPA for name in MODULI[:7]})
    return ElasticResult(strains=e, stresses=_voigt(stress).cpu().numpy(), c=c_h, c_raw=c_raw.cpu().numpy(),
                         compliance=compliance.cpu().numpy(), c_GPa=c_h * EV_A3_TO_GPA, sigma0=sigma0.cpu().numpy(),
                         rms=rms.cpu().numpy(), asymmetry=asymmetry.cpu().numpy(), status=status.cpu().numpy().astype(np.int64),
                         converged=r.converged.cpu().numpy().reshape(B, P),
                         n_steps=r.n_steps.cpu().numpy().astype(np.int64).reshape(B, P), lattices=lat_out, positions=pos_out,
                         n_eval_calls=r.n_calls, **named)
