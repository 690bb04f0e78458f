"""Batched nudged elastic band (NEB): migration barriers between two minima, for B bands together.

The reference's ``alignn/ff/ff.py`` has no transition-path calculation; its users run ASE's ``NEB`` around the calculator, one
image and one host round trip at a time.  ``neb`` does for B bands what ``NEB(images, k, climb, method)``,
``interpolate(mic=True)`` and ``FIRE(neb).run(fmax, steps)`` do for one (the formulas of ``ase/neb.py`` 3.22 for
``method="aseneb"`` and ``"improvedtangent"``):

1. the endpoints are evaluated once, for their energies;
2. ``alignn_neb_interpolate`` (csrc/neb.hip) builds the interior images of all bands in one launch;
3. ``relax`` runs FIRE on every band as ONE structure of (M - 2) n rows - so FIRE's state, its ``maxstep`` clip and the
   convergence test (the largest NEB force over all image rows below ``fmax``) are per band, as in ASE - through its
   ``evaluator`` hook: an evaluation splits the active bands into images, evaluates all of them in one model call (or in
   whole-image chunks of at most ``max_atoms_per_eval`` atoms), and one ``alignn_neb_forces`` launch turns the raw forces into
   NEB forces (tangent, projection, springs, climbing image).

The minimum image convention is the plain wrap of the fractional difference (``f -= rint(f)``), not ASE's Minkowski-reduced
``find_mic``: for strongly skewed cells the two can differ.  The kernels are float64 with fixed-order sums over an image's own
rows, and ``relax`` keeps a structure's bits independent of its batch, so a band's numbers are the same whatever else is in the
call.  tests/neb_ref.py restates the formulas in numpy.  The entry points are declared in include/alignn_neb.h, read here with
the reader of alignn_amd/_abi.py.

A band starts from the straight line, from the IDPP path (``interpolation="idpp"``: alignn_amd/idpp.py runs the same evaluator
on the image dependent pair potential, csrc/idpp.hip, in place of the model) or from images handed in (``start``).

Not here: the ``eb`` / ``spline`` / ``string`` methods, a list of spring constants along a band, variable-cell NEB, dynamic
relaxation of images, and the relaxation of the endpoints (relax them with ``relax`` first).
"""

from __future__ import annotations

import ctypes as C
import numbers
from dataclasses import dataclass
from typing import Callable, List, Optional, Sequence

import numpy as np
import torch

from . import _abi, _lib
from ._structures import ForceEvaluator, check_inputs, gpu_device, host, pack, shape_of
from .relax import relax

__all__ = ["neb", "neb_interpolate", "NEBResult", "METHODS", "MAX_IMAGES"]

H = _abi.header("alignn_neb.h")
HEADER, STRUCTS, SIGNATURES = H.path, H.structs, H.signatures  # the argument block alignn_neb_args; entry point -> (restype, argtypes)
NebArgs = STRUCTS["alignn_neb_args"]
METHODS = {"aseneb": 0, "improvedtangent": 1}
MAX_IMAGES = H.defines["ALIGNN_NEB_MAX_IMAGES"]  # images per band, the endpoints included
_FIRE = ("dt", "maxstep", "dtmax", "Nmin", "finc", "fdec", "astart", "fa", "a")


def _load():
    return _lib.bind(H)


@dataclass
class NEBResult:
    """Per band, in the input order; M = n_images + 2.  ``positions[b]`` [M, n, 3]: the band, endpoints included, Cartesian and
    not wrapped into the cell.  ``energies[b]`` [M] (eV) and ``forces[b]`` [M - 2, n, 3] (the NEB forces of the interior images;
    a fixed atom's row is the projection's, FIRE reads it as zero) are those of the band's last evaluation.  ``imax[b]``: the
    interior image of largest energy.  ``barrier = max(E) - E[0]`` and ``delta_e = E[-1] - E[0]``: ASE's
    ``NEBTools.get_barrier(fit=False)``.  ``fmax[b]``: the largest NEB force over the rows FIRE moves; ``n_steps`` FIRE steps
    taken; ``n_evals`` batched evaluations of the bands (the one of the endpoints not counted)."""

    positions: List[torch.Tensor]  # [M, n, 3] float64
    energies: List[np.ndarray]  # [M] float64
    forces: List[torch.Tensor]  # [M - 2, n, 3] float64
    imax: np.ndarray  # [B] int
    barrier: np.ndarray  # [B] float64
    delta_e: np.ndarray  # [B] float64
    fmax: torch.Tensor  # [B] float64
    converged: torch.Tensor  # [B] bool
    n_steps: torch.Tensor  # [B] int64
    n_evals: int


# --- checks (host) -----------------------------------------------------------------------------------------------------------------
def _inv3_cof(a: np.ndarray) -> np.ndarray:
    """csrc/cell3.h's inverse by cofactors, on the host."""
    a = [float(v) for v in np.asarray(a, dtype=np.float64).reshape(-1)]
    c00, c01, c02 = a[4] * a[8] - a[5] * a[7], a[3] * a[8] - a[5] * a[6], a[3] * a[7] - a[4] * a[6]
    det = (a[0] * c00 - a[1] * c01) + a[2] * c02
    return np.array([c00 / det, (a[2] * a[7] - a[1] * a[8]) / det, (a[1] * a[5] - a[2] * a[4]) / det,
                     -c01 / det, (a[0] * a[8] - a[2] * a[6]) / det, (a[2] * a[3] - a[0] * a[5]) / det,
                     c02 / det, (a[1] * a[6] - a[0] * a[7]) / det, (a[0] * a[4] - a[1] * a[3]) / det]).reshape(3, 3)


def _mic_host(d: np.ndarray, cell: np.ndarray) -> np.ndarray:
    """The kernels' minimum image convention on the host (the check of coinciding endpoints)."""
    dot = lambda x, m: (x[:, 0:1] * m[0] + x[:, 1:2] * m[1]) + x[:, 2:3] * m[2]
    f = dot(d, _inv3_cof(cell))
    return dot(f - np.round(f), cell)


def _per_band(who: str, name: str, v, B: int, integer: bool) -> np.ndarray:
    x = host(v)
    ok = x.dtype.kind in ("iu" if integer else "iuf") and x.shape in ((), (B,))
    if not ok or (integer and isinstance(v, (bool, np.bool_))):
        raise ValueError(f"{who}: {name} needs one {'int' if integer else 'number'} or {B} of them, got {v!r}")
    return np.broadcast_to(x.astype(np.int64 if integer else np.float64), (B,)).copy()


def _check(who, model, lattices, initial, final, atom_features, n_images, k, climb, method, fmax, steps, fixed, forces_fn,
           max_atoms_per_eval, fire):
    """Every ``ValueError`` check of ``neb`` -> (ns, M [B], k [B], fixed per band row or None)."""
    ns = check_inputs(who, model, lattices, initial, atom_features, forces_fn=forces_fn)
    B = len(ns)
    if len(final) != B:
        raise ValueError(f"{who}: {B} initial and {len(final)} final structures (need the same number)")
    for i in range(B):
        if shape_of(final[i]) != (ns[i], 3):
            raise ValueError(f"{who}: final[{i}] is {shape_of(final[i])}, initial[{i}] is [{ns[i]}, 3]: the endpoints of a band "
                             "have the same atoms")
    n_im = _per_band(who, "n_images", n_images, B, integer=True)
    if (n_im < 1).any() or (n_im > MAX_IMAGES - 2).any():
        raise ValueError(f"{who}: n_images (the interior images) must be 1 .. {MAX_IMAGES - 2}, got {n_images!r}")
    ks = _per_band(who, "k", k, B, integer=False)
    if not (np.isfinite(ks).all() and (ks > 0).all()):
        raise ValueError(f"{who}: k must be finite and > 0 (one spring constant per band: a list along a band is not supported), "
                         f"got {k!r}")
    if method not in METHODS:
        raise ValueError(f"{who}: method must be one of {sorted(METHODS)}, got {method!r}")
    if not isinstance(climb, (bool, np.bool_)):
        raise ValueError(f"{who}: climb is one bool, got {type(climb).__name__}")
    if not (isinstance(steps, numbers.Integral) and steps >= 0 and isinstance(fmax, numbers.Real) and fmax >= 0):
        raise ValueError(f"{who}: need steps >= 0 and fmax >= 0")
    if max_atoms_per_eval is not None and not (isinstance(max_atoms_per_eval, numbers.Integral) and max_atoms_per_eval >= 1):
        raise ValueError(f"{who}: max_atoms_per_eval must be an int >= 1 or None, got {max_atoms_per_eval!r}")
    unknown = sorted(set(fire) - set(_FIRE))
    if unknown:
        raise ValueError(f"{who}: unknown option(s) {unknown}; FIRE's are {list(_FIRE)}")
    if fire.get("maxstep", 1.0) <= 0 or fire.get("dt", 1.0) <= 0:
        raise ValueError(f"{who}: need maxstep > 0, dt > 0")
    tiled = None
    if fixed is not None:
        if isinstance(fixed, (torch.Tensor, np.ndarray)) and fixed.ndim != 2 or len(fixed) != B:
            raise ValueError(f"{who}: fixed needs one boolean [n_i] array (or None) per band, {B} of them")
        tiled = []
        for i, f in enumerate(fixed):
            f = np.zeros(ns[i], dtype=bool) if f is None else host(f)
            if f.shape != (ns[i],) or f.dtype != np.bool_:
                raise ValueError(f"{who}: fixed[{i}] is {f.dtype} {f.shape}, need bool [{ns[i]}]")
            tiled.append(np.tile(f, int(n_im[i])))
    for i in range(B):
        d = host(final[i]).astype(np.float64) - host(initial[i]).astype(np.float64)
        if not np.isfinite(d).all():
            raise ValueError(f"{who}: the endpoints of band {i} must be finite")
        if not _mic_host(d, host(lattices[i]).astype(np.float64)).any():
            raise ValueError(f"{who}: the endpoints of band {i} coincide (to the minimum image convention): there is no path")
    return ns, n_im + 2, ks, tiled


# --- the launches ------------------------------------------------------------------------------------------------------------------
def _prefix(counts, dev) -> torch.Tensor:
    return torch.tensor(np.concatenate([[0], np.cumsum(counts)]), dtype=torch.int32, device=dev)


def neb_interpolate(lattices: torch.Tensor, initial: torch.Tensor, final: torch.Tensor, ns: Sequence[int], images: Sequence[int]):
    """The interpolation launch alone, on float64 tensors on the GPU: ``lattices`` [B, 3, 3], ``initial`` / ``final`` [sum n_b, 3]
    the packed endpoints, ``ns`` the atom counts n_b and ``images`` the image counts M_b (endpoints included, 3 .. 64) ->
    (the interior rows of all bands [sum (M_b - 2) n_b, 3], band after band and image 1 first; the inverse cells [B, 3, 3] as
    ``alignn_neb_forces`` takes them)."""
    who = "neb_interpolate"
    ns, images = [int(n) for n in ns], [int(m) for m in images]
    B = len(ns)
    if B < 1 or len(images) != B or min(ns) < 1 or min(images) < 3 or max(images) > MAX_IMAGES:
        raise ValueError(f"{who}: need B >= 1 bands of n_b >= 1 atoms and 3 .. {MAX_IMAGES} images each")
    N = sum(ns)
    for name, t, shape in (("lattices", lattices, (B, 3, 3)), ("initial", initial, (N, 3)), ("final", final, (N, 3))):
        if tuple(t.shape) != shape:
            raise ValueError(f"{who}: {name} must be {list(shape)}, got {tuple(t.shape)}")
        if t.dtype != torch.float64 or not t.is_cuda or t.device != lattices.device:
            raise TypeError(f"{who}: {name} must be a float64 tensor on the GPU, got {t.dtype} on {t.device}")
    rows = [(m - 2) * n for m, n in zip(images, ns)]
    if sum(rows) >= 2 ** 31:
        raise ValueError(f"{who}: {sum(rows)} rows; a call takes fewer than 2^31")
    dev = lattices.device
    lib = _load()
    with _lib.device_guard(lattices):
        lattices, initial, final = lattices.contiguous(), initial.contiguous(), final.contiguous()
        end_ptr, row_ptr = _prefix(ns, dev), _prefix(rows, dev)
        out = torch.empty(sum(rows), 3, dtype=torch.float64, device=dev)
        inv = torch.empty(B, 3, 3, dtype=torch.float64, device=dev)
        _lib.check(lib.alignn_neb_interpolate(initial.data_ptr(), final.data_ptr(), end_ptr.data_ptr(), lattices.data_ptr(),
                                              row_ptr.data_ptr(), B, sum(rows), out.data_ptr(), inv.data_ptr(), _lib.stream()),
                   "neb_interpolate")
    return out, inv


class _BandEvaluator:
    """``relax``'s evaluator for bands: called as ``ForceEvaluator`` is, with band indices.  It evaluates the images of the
    active bands through an inner ``ForceEvaluator`` whose structures are the images (interior image j of band b is structure
    ``img0[b] + j``, the 2 B endpoints follow), launches ``alignn_neb_forces`` and returns (E[imax] per band, the NEB forces,
    None)."""

    def __init__(self, who, model, forces_fn, atom_features, ns, M, ks, lat, inv, ends, fixed_t, method, climb, max_atoms, dev,
                 evaluation):
        B = len(ns)
        self.ns, self.M, self.dev, self.max_atoms, self.B = ns, M, dev, max_atoms, B
        inner = [int(m) - 2 for m in M]
        self.img0 = np.concatenate([[0], np.cumsum(inner)]).astype(np.int64)  # first interior-image structure of a band
        self.n_interior = int(self.img0[-1])
        counts = [ns[b] for b in range(B) for _ in range(inner[b])] + [ns[b] for b in range(B)] * 2
        feats = None
        if forces_fn is None:
            per_band = [torch.as_tensor(f).to(dev, torch.float32) for f in atom_features]
            feats = [per_band[b] for b in range(B) for _ in range(inner[b])] + per_band * 2
        self.inner = ForceEvaluator(who, model, forces_fn, feats, counts, dev, **evaluation)
        self.counts = counts
        self.energies_all = torch.zeros(int(np.sum(M)), dtype=torch.float64, device=dev)
        self.end_energy = torch.zeros(B, 2, dtype=torch.float64, device=dev)
        self.ends, self.keep = ends, (lat, inv, fixed_t)  # (the argument block holds raw pointers)
        self.spring = torch.tensor(ks, dtype=torch.float64, device=dev)
        self.image_ptr, self.end_ptr = _prefix(M, dev), _prefix(ns, dev)
        rows = [inner[b] * ns[b] for b in range(B)]
        self.row0 = np.concatenate([[0], np.cumsum(rows)]).astype(np.int64)  # a band's first row: relax's atom_ptr
        self.row_ptr = _prefix(rows, dev)
        self.args = NebArgs(row_ptr=self.row_ptr.data_ptr(), image_ptr=self.image_ptr.data_ptr(),
                            end_ptr=self.end_ptr.data_ptr(), lattice=lat.data_ptr(), inv_lattice=inv.data_ptr(), spring=self.spring.data_ptr(), initial=ends.pos[:ends.ptr[B]].data_ptr(),
                            final=ends.pos[ends.ptr[B]:].data_ptr(), end_energy=self.end_energy.data_ptr(),
                            fixed=_lib.ptr(fixed_t), energies_out=self.energies_all.data_ptr(), method=METHODS[method],
                            climb=int(bool(climb)))
        self._which = None
        self.n_model_calls = 0

    def images(self, which, lattices, frac, cart):
        """(energy, forces) of the image structures ``which``, in one call or in whole-image chunks of at most ``max_atoms``."""
        chunks, cur, atoms = [], [], 0
        for j, w in enumerate(which):
            if cur and self.max_atoms is not None and atoms + self.counts[w] > self.max_atoms:
                chunks.append(cur)
                cur, atoms = [], 0
            cur.append(j)
            atoms += self.counts[w]
        chunks.append(cur)
        es, fs = [], []
        for ch in chunks:
            e, f, _ = self.inner([which[j] for j in ch], [lattices[j] for j in ch], [frac[j] for j in ch],
                                 None if cart is None else [cart[j] for j in ch])
            self.n_model_calls += 1
            es.append(e)
            fs.append(f)
        return (es[0], fs[0]) if len(chunks) == 1 else (torch.cat(es), torch.cat(fs))

    def endpoints(self, lat_v):
        """The energies of the 2 B endpoints, once."""
        ends = self.ends
        which = list(range(self.n_interior, self.n_interior + 2 * self.B))
        e, _ = self.images(which, lat_v * 2, ends.rows(ends.frac), ends.rows(ends.pos))
        self.end_energy.copy_(e.view(2, self.B).t())

    def interior(self, which, lattices, frac, cart):
        """(energy, forces) of the interior images of the active bands ``which``, in evaluation order: the one place the band
        meets what it is relaxed on (alignn_amd/idpp.py puts the IDPP objective here)."""
        ns, M = self.ns, self.M
        split = lambda ts: [t[j * ns[b]:(j + 1) * ns[b]] for b, t in zip(which, ts) for j in range(int(M[b]) - 2)]
        lat_img = [lat for b, lat in zip(which, lattices) for _ in range(int(M[b]) - 2)]
        return self.images(self._structures, lat_img, split(frac), split(cart))

    def __call__(self, which, lattices, frac, cart):
        ns, M, dev = self.ns, self.M, self.dev
        if list(which) != self._which:  # (bands have retired: the launch's index arrays)
            self._which = list(which)
            self._structures = [int(self.img0[b]) + j for b in which for j in range(int(M[b]) - 2)]
            self._force_ptr = _prefix([(int(M[b]) - 2) * ns[b] for b in which], dev)
            self._energy_ptr = _prefix([int(M[b]) - 2 for b in which], dev)
            self._active = torch.tensor(self._which, dtype=torch.int32, device=dev)
            self._imax = torch.empty(len(which), dtype=torch.int32, device=dev)
            self._emax = torch.empty(len(which), dtype=torch.float64, device=dev)
            a = self.args
            a.force_ptr, a.energy_ptr, a.active = self._force_ptr.data_ptr(), self._energy_ptr.data_ptr(), self._active.data_ptr()
            a.imax, a.emax, a.n_active = self._imax.data_ptr(), self._emax.data_ptr(), len(which)
            a.max_images = max(int(M[b]) for b in which)
        # relax hands over views of its position array, a band's rows at its place in the packed batch: the kernel reads the
        # neighbouring images (and the fixed flags) by row index from the array's start
        base = cart[0].data_ptr() - 24 * int(self.row0[which[0]])
        if any(t.data_ptr() != base + 24 * int(self.row0[b]) or not t.is_contiguous() for b, t in zip(which, cart)):
            raise RuntimeError("neb: the bands' rows are not views of one packed position array")
        self.args.positions = base
        energy, forces = self.interior(which, lattices, frac, cart)
        out = torch.empty_like(forces)
        self.args.forces, self.args.energy, self.args.forces_out = forces.data_ptr(), energy.data_ptr(), out.data_ptr()
        _lib.check(_load().alignn_neb_forces(C.byref(self.args), _lib.stream()), "neb_forces")
        return self._emax, out, None


# --- the driver --------------------------------------------------------------------------------------------------------------------
INTERPOLATIONS = ("linear", "idpp")


def _check_start(who, interpolation, idpp_fmax, idpp_steps, start, ns, M):
    """The ``ValueError`` checks of where a band starts: ``interpolation``, the IDPP pass's limits and the shapes of ``start``."""
    if interpolation not in INTERPOLATIONS:
        raise ValueError(f"{who}: interpolation must be one of {list(INTERPOLATIONS)}, got {interpolation!r}")
    if not (isinstance(idpp_steps, numbers.Integral) and idpp_steps >= 0 and isinstance(idpp_fmax, numbers.Real) and idpp_fmax >= 0):
        raise ValueError(f"{who}: need idpp_steps >= 0 and idpp_fmax >= 0")
    if start is None:
        return
    if interpolation == "idpp":
        raise ValueError(f"{who}: start gives the interior images as they are; it cannot be combined with interpolation='idpp'")
    if isinstance(start, (torch.Tensor, np.ndarray)) and start.ndim != 4 or len(start) != len(ns):
        raise ValueError(f"{who}: start needs one [n_images, n, 3] array of interior images per band, {len(ns)} of them")
    for i, s in enumerate(start):
        want = (int(M[i]) - 2, ns[i], 3)
        if shape_of(s) != want:
            raise ValueError(f"{who}: start[{i}] is {shape_of(s)}, need {list(want)}: the interior images of band {i}")
        if not np.isfinite(host(s).astype(np.float64)).all():
            raise ValueError(f"{who}: start[{i}] must be finite")


def _linear_path(lattices, initial, final, ns, M, tiled, dev):
    """The bands on the device -> (the 2 B endpoints as one packed batch, the initial structures and then the final ones; the
    cells [B, 3, 3]; the interior rows of the straight path and the inverse cells, as ``neb_interpolate`` gives them; the fixed
    flags per interior row, or None)."""
    B = len(ns)
    ends = pack(list(lattices) * 2, list(initial) + list(final), ns * 2, dev)
    lat = ends.lat[:B].contiguous()
    rows, inv = neb_interpolate(lat, ends.pos[:ends.ptr[B]], ends.pos[ends.ptr[B]:], ns, M)
    fixed_t = None
    if tiled is not None and any(t.any() for t in tiled):
        fixed_t = torch.tensor(np.concatenate(tiled).astype(np.uint8), device=dev)
    return ends, lat, rows, inv, fixed_t


def _run_band(evaluate, lat_v, rows, ns, M, tiled, fmax, steps, dev, fire):
    """FIRE on every band as one structure of its interior rows ``rows``, through ``relax`` and the band evaluator."""
    counts = [(int(M[b]) - 2) * ns[b] for b in range(len(ns))]
    bands = list(torch.split(rows, counts))
    return relax(None, lat_v, bands, None, evaluator=evaluate, fixed=tiled, optimize_lattice=False, fmax=fmax,
                 steps=steps, device=dev, **fire)


def _band_results(energies, r, ends, ns, M):
    """Per band: the M energies of the last evaluation and the band [M, n, 3], endpoints included."""
    B = len(ns)
    ptr = np.concatenate([[0], np.cumsum(M)])
    E = [energies[ptr[b]:ptr[b + 1]].copy() for b in range(B)]
    positions = [torch.cat([ends.rows(ends.pos)[b][None], r.positions[b].view(int(M[b]) - 2, ns[b], 3),
                            ends.rows(ends.pos)[B + b][None]]) for b in range(B)]
    return E, positions


def neb(model, lattices: Sequence, initial: Sequence, final: Sequence, atom_features: Optional[Sequence] = None, *,
        n_images=3, k=0.1, climb: bool = False, method: str = "aseneb", fmax: float = 0.05, steps: int = 100,
        fixed: Optional[Sequence] = None, forces_fn: Optional[Callable] = None, device=None,
        max_atoms_per_eval: Optional[int] = None, cutoff: float = 8.0, max_neighbors: int = 12,
        neighbor_strategy: str = "k-nearest", intensive: bool = True, force_multiplier: float = 1.0,
        interpolation: str = "linear", idpp_fmax: float = 0.1, idpp_steps: int = 100, start: Optional[Sequence] = None,
        **fire) -> NEBResult:
    """Nudged elastic band between ``initial[b]`` and ``final[b]`` ([n_b, 3] Cartesian, the same atoms in the same order) in the
    cell ``lattices[b]``, for B bands together: ASE's ``NEB(images, k=k, climb=climb, method=method)`` with
    ``interpolate(mic=True)`` and ``FIRE(neb).run(fmax, steps)``.

    The structures, the model (or ``forces_fn``), ``cutoff`` ... ``force_multiplier`` and the device: alignn_amd/_structures.py.
    ``forces_fn`` gets the images of one evaluation, each with its band's cell.

    ``n_images``: the interior images of a band, one int or B of them, 1 .. 62 (a band has ``n_images + 2`` images).  ``k``: the
    spring constant (eV/A^2), one number or B of them, finite and > 0.  ``method``: "aseneb" or "improvedtangent".  ``climb``:
    the interior image of largest energy climbs (no springs, the force along the tangent reversed).  ``fmax`` (eV/A) and
    ``steps``: FIRE stops a band when its largest NEB force over all image rows is below ``fmax``, or after ``steps`` steps.
    ``fixed``: ASE's ``FixAtoms``, B boolean arrays [n_b] (``None`` for a band: none), the same atoms in every image; their raw
    forces are zero ahead of the projection and FIRE does not move them.  ``max_atoms_per_eval``: evaluate the images in chunks
    of whole images of at most this many atoms (an image larger than it goes alone); the results are the same bits.  ``**fire``:
    FIRE's ``dt``, ``maxstep``, ``dtmax``, ``Nmin``, ``finc``, ``fdec``, ``astart``, ``fa``, ``a`` with ``relax``'s defaults.

    Where the bands start.  ``interpolation="linear"`` (the default): the straight line between the endpoints,
    ``interpolate(mic=True)``.  ``"idpp"``: ASE's ``interpolate(method="idpp")`` - from the straight line, the band's own NEB
    (its ``k``, its ``method``, no climbing image, the same ``fixed`` rows, the same ``**fire``) is first run on the image
    dependent pair potential of alignn_amd/idpp.py instead of the model, until its largest force is below ``idpp_fmax`` or for
    ``idpp_steps`` steps (ASE's defaults), with FIRE where ASE's default is ``MDMin``; the model then starts from that path.
    ``start``: B arrays [n_images_b, n_b, 3], the interior images as they are to be used, instead of an interpolation (not
    together with ``"idpp"``); ``idpp_interpolate`` gives such images.

    The endpoints are used as given: relax them with ``relax`` first.  Displacements between neighbouring images take the
    minimum image convention of the plain wrap (``f -= rint(f)`` on the fractional difference), not ASE's Minkowski-reduced
    ``find_mic``: for strongly skewed cells the two can differ.  A band whose endpoints coincide is refused.

    Not supported: the ``eb`` / ``spline`` / ``string`` methods, a list of spring constants along a band, variable-cell NEB,
    dynamic relaxation of images, endpoint relaxation inside the call."""
    who = "neb"
    ns, M, ks, tiled = _check(who, model, lattices, initial, final, atom_features, n_images, k, climb, method, fmax, steps, fixed,
                              forces_fn, max_atoms_per_eval, fire)
    _check_start(who, interpolation, idpp_fmax, idpp_steps, start, ns, M)
    dev = gpu_device(who, model, forces_fn, device)
    B = len(ns)
    evaluation = dict(cutoff=cutoff, max_neighbors=max_neighbors, neighbor_strategy=neighbor_strategy, intensive=intensive,
                      force_multiplier=force_multiplier)

    with _lib.device_guard(torch.empty(0, device=dev)):
        ends, lat, rows, inv, fixed_t = _linear_path(lattices, initial, final, ns, M, tiled, dev)
        if start is not None:
            rows = torch.cat([torch.as_tensor(s).to(dev, torch.float64).reshape(-1, 3) for s in start]).contiguous()
        elif interpolation == "idpp":
            from .idpp import idpp_pass

            rows = torch.cat(idpp_pass(who, ns, M, ks, tiled, lat, inv, ends, fixed_t, method, rows, idpp_fmax, idpp_steps, dev,
                                       fire)[0].positions)
        evaluate = _BandEvaluator(who, model, forces_fn, atom_features, ns, M, ks, lat, inv, ends, fixed_t, method, climb,
                                  max_atoms_per_eval, dev, evaluation)
        lat_v = [lat[b] for b in range(B)]
        evaluate.endpoints(lat_v)
        r = _run_band(evaluate, lat_v, rows, ns, M, tiled, fmax, steps, dev, fire)
        energies = evaluate.energies_all.cpu().numpy()
    E, positions = _band_results(energies, r, ends, ns, M)
    return NEBResult(positions=positions, energies=E, forces=[f.view(int(M[b]) - 2, ns[b], 3) for b, f in enumerate(r.forces)],
                     imax=np.array([1 + int(np.argmax(e[1:-1])) for e in E]), barrier=np.array([e.max() - e[0] for e in E]),
                     delta_e=np.array([e[-1] - e[0] for e in E]), fmax=r.fmax, converged=r.converged, n_steps=r.n_steps,
                     n_evals=r.n_evals)
