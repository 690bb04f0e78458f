"""IDPP band initialisation for the batched nudged elastic band: ASE's ``NEB.interpolate(method="idpp")`` for B bands together.

The straight line between two minima squeezes bonds when the moving atoms turn instead of translate, and the first model
evaluations of ``neb`` then land on structures the force field has never seen.  The image dependent pair potential (IDPP, ASE
3.22 ``ase/neb.py``: class ``IDPP`` and ``NEB.idpp_interpolate``) asks instead that every pair distance go linearly from its value
in the first image to its value in the last.  For image m of a band of M images, atom a and every b != a:

    D_ab = mic(R_a - R_b)      d_ab = |D_ab|
    t_ab(m) = d1_ab + m (d2_ab - d1_ab) / (M - 1)      d1, d2: d_ab in image 0 and in image M - 1
    delta = d_ab - t_ab(m)
    E_m = 1/2 sum_a sum_{b != a} delta^2 / d_ab^4
    F_a = -2 sum_{b != a} delta (1 - 2 delta / d_ab) / d_ab^5 D_ab

with ``mic`` the plain wrap of alignn_amd/neb.py (not ASE's Minkowski-reduced ``find_mic``).  ``alignn_idpp_forces``
(csrc/idpp.hip) evaluates it for the interior images of all active bands: one wavefront per (image, atom), float64 with fixed-order
sums, the results laid out as ``alignn_neb_forces`` reads an evaluation.

The IDPP pass is the band's own NEB run on this objective: ``neb``'s band evaluator with the model call replaced by that one
launch (endpoint energies 0, no climbing image), driven by ``relax``'s FIRE from the straight path.  ASE's default optimiser
for this pass is ``MDMin``, which this package does not have: FIRE is the stated difference, so the path at a given ``fmax`` is
not ASE's step for step.  Coinciding atoms (d = 0) get what the arithmetic gives, and a pair at exactly half a cell vector takes
the image ``rint`` gives: the cusp of the wrap, as in ASE.

tests/idpp_ref.py restates the formulas and the pass in numpy.  The entry point is declared in include/alignn_idpp.h, read here
with the reader of alignn_amd/_abi.py.
"""

from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import List, Optional, Sequence

import numpy as np
import torch

from . import _abi, _lib
from ._structures import gpu_device
from .neb import (MAX_IMAGES, _BandEvaluator, _band_results, _check, _inv3_cof, _linear_path, _prefix, _run_band)

__all__ = ["idpp_forces", "idpp_interpolate", "IDPPResult"]

H = _abi.header("alignn_idpp.h")
HEADER, STRUCTS, SIGNATURES = H.path, H.structs, H.signatures  # the argument block alignn_idpp_args; entry point -> (restype, argtypes)
IdppArgs = STRUCTS["alignn_idpp_args"]


def _load():
    return _lib.bind(H)


@dataclass
class IDPPResult:
    """Per band, in the input order; M = n_images + 2.  ``positions[b]`` [M, n, 3]: the band, endpoints included, Cartesian and
    not wrapped into the cell (``positions[b][1:-1]`` is what ``neb`` takes as ``start``).  ``energies[b]`` [M]: the IDPP
    objective of the band's last evaluation, zero at the endpoints.  ``fmax[b]``: the largest NEB force on the objective over
    the rows FIRE moves; ``n_steps`` FIRE steps taken; ``n_evals`` evaluations of the bands."""

    positions: List[torch.Tensor]  # [M, n, 3] float64
    energies: List[np.ndarray]  # [M] float64
    fmax: torch.Tensor  # [B] float64
    converged: torch.Tensor  # [B] bool
    n_steps: torch.Tensor  # [B] int64
    n_evals: int


# --- the launch --------------------------------------------------------------------------------------------------------------------
def idpp_forces(lattices: torch.Tensor, initial: torch.Tensor, final: torch.Tensor, positions: torch.Tensor, ns: Sequence[int],
                images: Sequence[int]):
    """The ``alignn_idpp_forces`` launch alone, on float64 tensors on the GPU: ``lattices`` [B, 3, 3], ``initial`` / ``final``
    [sum n_b, 3] the packed endpoints, ``positions`` [sum (M_b - 2) n_b, 3] the interior rows of all bands (band after band,
    image 1 first, as ``neb_interpolate`` gives them), ``ns`` the atom counts n_b and ``images`` the image counts M_b (endpoints
    included, 3 .. 64) -> (the objective of every interior image [sum (M_b - 2)], its forces [sum (M_b - 2) n_b, 3])."""
    who = "idpp_forces"
    ns, images = [int(n) for n in ns], [int(m) for m in images]
    B = len(ns)
    if B < 1 or B > 65535 or len(images) != B or min(ns) < 1 or min(images) < 3 or max(images) > MAX_IMAGES:
        raise ValueError(f"{who}: need 1 .. 65535 bands of n_b >= 1 atoms and 3 .. {MAX_IMAGES} images each")
    N = sum(ns)
    rows = [(m - 2) * n for m, n in zip(images, ns)]
    if sum(rows) >= 2 ** 31:
        raise ValueError(f"{who}: {sum(rows)} rows; a call takes fewer than 2^31")
    for name, t, shape in (("lattices", lattices, (B, 3, 3)), ("initial", initial, (N, 3)), ("final", final, (N, 3)),
                           ("positions", positions, (sum(rows), 3))):
        if tuple(t.shape) != shape:
            raise ValueError(f"{who}: {name} must be {list(shape)}, got {tuple(t.shape)}")
        if t.dtype != torch.float64 or not t.is_cuda or t.device != lattices.device:
            raise TypeError(f"{who}: {name} must be a float64 tensor on the GPU, got {t.dtype} on {t.device}")
    dev = lattices.device
    lib = _load()
    with _lib.device_guard(lattices):
        lattices, initial, final, positions = lattices.contiguous(), initial.contiguous(), final.contiguous(), positions.contiguous()
        inv = torch.tensor(np.stack([_inv3_cof(c) for c in lattices.cpu().numpy()]), dtype=torch.float64, device=dev)
        row_ptr, end_ptr, energy_ptr = _prefix(rows, dev), _prefix(ns, dev), _prefix([m - 2 for m in images], dev)
        active = torch.arange(B, dtype=torch.int32, device=dev)
        forces = torch.empty(sum(rows), 3, dtype=torch.float64, device=dev)
        energy = torch.empty(sum(images) - 2 * B, dtype=torch.float64, device=dev)
        row_energy = torch.empty(sum(rows), dtype=torch.float64, device=dev)
        status = torch.empty(B, dtype=torch.int32, device=dev)
        args = IdppArgs(force_ptr=row_ptr.data_ptr(), energy_ptr=energy_ptr.data_ptr(), active=active.data_ptr(),
                        row_ptr=row_ptr.data_ptr(), end_ptr=end_ptr.data_ptr(), lattice=lattices.data_ptr(),
                        inv_lattice=inv.data_ptr(), initial=initial.data_ptr(), final=final.data_ptr(),
                        positions=positions.data_ptr(), forces=forces.data_ptr(), energy=energy.data_ptr(),
                        row_energy=row_energy.data_ptr(), status=status.data_ptr(), n_active=B, max_images=max(images),
                        max_atoms=max(ns))
        _lib.check(lib.alignn_idpp_forces(C.byref(args), _lib.stream()), "idpp_forces")
    return energy, forces


# --- the pass ----------------------------------------------------------------------------------------------------------------------
def _no_model(*args, **kwargs):
    raise RuntimeError("idpp: the IDPP pass evaluates no model")


_NO_MODEL = dict(cutoff=0.0, max_neighbors=0, neighbor_strategy="none", intensive=False, force_multiplier=1.0)


class _IdppEvaluator(_BandEvaluator):
    """``neb``'s band evaluator on the IDPP objective: the evaluation of the interior images is one ``alignn_idpp_forces`` launch
    on the bands' own rows; the endpoint energies stay 0 and no image climbs."""

    def __init__(self, who, ns, M, ks, lat, inv, ends, fixed_t, method, dev):
        super().__init__(who, None, _no_model, None, ns, M, ks, lat, inv, ends, fixed_t, method, False, None, dev, _NO_MODEL)
        a = self.args
        self.idpp = IdppArgs(row_ptr=a.row_ptr, end_ptr=a.end_ptr, lattice=a.lattice, inv_lattice=a.inv_lattice,
                             initial=a.initial, final=a.final)
        self._sized = None

    def interior(self, which, lattices, frac, cart):
        ns, M, g = self.ns, self.M, self.idpp
        if self._sized is not self._which:  # (bands have retired: the launch's index arrays are the band evaluator's)
            self._sized = self._which
            self._rows = sum((int(M[b]) - 2) * ns[b] for b in which)
            self._n_images = sum(int(M[b]) - 2 for b in which)
            self._status = torch.empty(len(which), dtype=torch.int32, device=self.dev)
            g.force_ptr, g.energy_ptr, g.active = self._force_ptr.data_ptr(), self._energy_ptr.data_ptr(), self._active.data_ptr()
            g.status, g.n_active = self._status.data_ptr(), len(which)
            g.max_images, g.max_atoms = max(int(M[b]) for b in which), max(ns[b] for b in which)
        forces = torch.empty(self._rows, 3, dtype=torch.float64, device=self.dev)
        energy = torch.empty(self._n_images, dtype=torch.float64, device=self.dev)
        row_energy = torch.empty(self._rows, dtype=torch.float64, device=self.dev)
        g.positions = self.args.positions  # (relax's packed position array, set by the band evaluator)
        g.forces, g.energy, g.row_energy = forces.data_ptr(), energy.data_ptr(), row_energy.data_ptr()
        _lib.check(_load().alignn_idpp_forces(C.byref(g), _lib.stream()), "idpp_forces")
        return energy, forces


def idpp_pass(who, ns, M, ks, tiled, lat, inv, ends, fixed_t, method, rows, fmax, steps, dev, fire):
    """FIRE on the IDPP objective from the interior rows ``rows`` of the bands ``_linear_path`` set up -> (``relax``'s result,
    the evaluator)."""
    evaluate = _IdppEvaluator(who, ns, M, ks, lat, inv, ends, fixed_t, method, dev)
    return _run_band(evaluate, [lat[b] for b in range(len(ns))], rows, ns, M, tiled, fmax, steps, dev, fire), evaluate


def idpp_interpolate(lattices: Sequence, initial: Sequence, final: Sequence, *, n_images=3, k=0.1, method: str = "aseneb",
                     fmax: float = 0.1, steps: int = 100, fixed: Optional[Sequence] = None, device=None, **fire) -> IDPPResult:
    """The IDPP path between ``initial[b]`` and ``final[b]`` ([n_b, 3] Cartesian, the same atoms in the same order) in the cell
    ``lattices[b]``, for B bands together: ASE's ``NEB(images, k=k, method=method).interpolate(method="idpp", mic=True)``
    with ``idpp_interpolate(fmax=fmax, steps=steps)``, the optimiser FIRE where ASE's default is ``MDMin``.  No model is used.

    ``n_images``, ``k``, ``method``, ``fixed`` and ``**fire`` (FIRE's parameters) as in ``neb``, with the same checks;
    ``fmax`` and ``steps``: a band stops when its largest NEB force on the objective is below ``fmax``, or after ``steps`` steps
    (ASE's defaults).  ``device``: the GPU to run on (default: the current one).

    ``neb(..., interpolation="idpp", idpp_fmax=fmax, idpp_steps=steps)`` runs this pass and continues with the model;
    ``neb(..., start=[p[1:-1] for p in result.positions])`` continues from a path computed here."""
    who = "idpp_interpolate"
    ns, M, ks, tiled = _check(who, None, lattices, initial, final, None, n_images, k, False, method, fmax, steps, fixed, _no_model,
                              None, fire)
    dev = gpu_device(who, None, _no_model, device)
    with _lib.device_guard(torch.empty(0, device=dev)):
        ends, lat, rows, inv, fixed_t = _linear_path(lattices, initial, final, ns, M, tiled, dev)
        r, evaluate = idpp_pass(who, ns, M, ks, tiled, lat, inv, ends, fixed_t, method, rows, fmax, steps, dev, fire)
        energies = evaluate.energies_all.cpu().numpy()
    E, positions = _band_results(energies, r, ends, ns, M)
    return IDPPResult(positions=positions, energies=E, fmax=r.fmax, converged=r.converged, n_steps=r.n_steps, n_evals=r.n_evals)
