"""Batched time-dependent pair correlations of MD trajectories on the device: the self and the distinct part of the van Hove
function, the non-Gaussian parameter and the intermediate scattering functions, for the B structures of a ``run_md`` call together.

``alignn_amd.trajectory`` and ``alignn_amd.order`` give the static structure (g(r), S(q)) and the single-particle averages (MSD,
VACF); the functions here say how the structure decays in time, on the same tensors (``MDResult.traj_positions`` [n_frames,
sum n_i, 3]) where they are:

* ``van_hove_self``: G_s(r, t), the distribution of the displacement of an atom over a lag - as a histogram that loses no term,
  as the radial density 4 pi r^2 G_s and as G_s - with <r^2>, <r^4>, the non-Gaussian parameter alpha_2(t) and, for given |q|,
  the isotropic self intermediate scattering function F_s(q, t);
* ``van_hove_distinct``: G_d(r, t), the distribution of the distance from where an atom was to where the OTHER atoms are a lag
  later, per species pair, normalised as g(r) (which it is at lag 0);
* ``intermediate_scattering``: the coherent F(q, t) on the reciprocal lattice of the (fixed) cell, total and Ashcroft-Langreth
  partials, per vector and in shells of |q| (which is S(q) at lag 0).

Conventions.  Frames (``start`` / ``stop`` / ``step``), groups (0 every atom, 1 .. S the species in ascending atomic number, at
most 8) and the pair rows (``trajectory.pair_row``) are those of ``alignn_amd.trajectory``, checked by the functions of
alignn_amd/_trajectory_inputs.py.  Lags count the frames used: ``lags`` is a strictly ascending sequence of ints in 0 .. F_used -
1 (at most 1024), or ``max_lag=K`` for 0 .. K; the origins of a lag k are t = 0, ``origin_stride``, 2 ``origin_stride``, ... with
t + k inside the selection, as in ``msd``.  ``remove_com``: the mass-weighted centre of mass of each structure and frame
(``alignn_traj_com``, the one ``msd`` uses) is taken off every position.  The kernels (csrc/vanhove.hip) are float64 without
contraction, the histograms are summed with integer atomics (exact), every floating-point sum has a fixed order over the
structure's own rows, frames and vectors: a structure's numbers are the same bits alone, in a batch and at any place of it.
tests/vanhove_ref.py restates the formulas in numpy; the entry points are declared in include/alignn_vanhove.h, read here with the
reader of alignn_amd/_abi.py.

Not here: the dynamic structure factor S(q, omega) (a window and a transform of F(q, t) away), F_s on single lattice vectors
(``fs`` is the powder average), per-frame cells for G_d and F(q, t) (a difference between two frames has no single cell), and
accumulation inside ``run_md`` without a stored trajectory.
"""

from __future__ import annotations

import ctypes as C
import numbers
from dataclasses import dataclass
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _abi, _lib, order, trajectory
from ._trajectory_inputs import _frames, _groups, _masses, _positive, _traj, bins, inputs

__all__ = ["van_hove_self", "van_hove_distinct", "intermediate_scattering", "VanHoveSelfResult", "VanHoveDistinctResult",
           "FqtResult", "MAX_LAGS", "MAX_Q", "MAX_BINS", "MAX_Q_BINS", "MAX_IMAGE_RANGE"]

H = _abi.header("alignn_vanhove.h")
HEADER, STRUCTS, SIGNATURES = H.path, H.structs, H.signatures  # the argument blocks; entry point -> (restype, argtypes)
SelfArgs, DistinctArgs, FqtArgs = STRUCTS["alignn_vh_self_args"], STRUCTS["alignn_vh_distinct_args"], STRUCTS["alignn_vh_fqt_args"]
MAX_SPECIES = H.defines["ALIGNN_VH_MAX_SPECIES"]
MAX_BINS = H.defines["ALIGNN_VH_MAX_BINS"]
MAX_IMAGE_RANGE = H.defines["ALIGNN_VH_MAX_IMAGE_RANGE"]
MAX_LAGS = H.defines["ALIGNN_VH_MAX_LAGS"]
MAX_Q = H.defines["ALIGNN_VH_MAX_Q"]
MAX_Q_BINS = H.defines["ALIGNN_VH_MAX_Q_BINS"]
STATUS_IMAGES = H.defines["ALIGNN_VH_STATUS_IMAGES"]


def _load():
    return _lib.bind(H)


# --- results -----------------------------------------------------------------------------------------------------------------------
@dataclass
class VanHoveSelfResult:
    """``r`` [n_bins]: the bin centres (A).  ``lags`` [L] and ``n_origins`` [L]: the lags (in frames used) and the time origins
    averaged at each.  ``counts`` [B, S + 1, L, n_bins] int64: the displacements (origin, atom) per bin of their length, per group
    (0: every atom, the sum of the species rows); ``overflow`` [B, S + 1, L] int64: those of r_max and beyond, so that
    ``counts.sum(-1) + overflow`` is n_origins N_a exactly.  ``p`` = counts / (n_origins N_a dr): the radial density 4 pi r^2
    G_s(r, t), which integrates to 1 less the overflow's share.  ``gs`` = counts / (n_origins N_a shell volume): G_s(r, t).
    ``moments`` [B, S + 1, L, 2]: <r^2> and <r^4> over origins and members; ``alpha2`` [B, S + 1, L] = 3 <r^4> / (5 <r^2>^2) - 1,
    0 where <r^2> is 0.  ``fs`` [B, S + 1, L, n_q] (None without ``q``): the mean of j0(q r), ``q`` [n_q] in 1/A.
    ``species[b]``: the atomic numbers of structure b's groups 1 .. S_b."""

    r: torch.Tensor
    lags: np.ndarray
    n_origins: np.ndarray
    counts: torch.Tensor
    overflow: torch.Tensor
    p: torch.Tensor
    gs: torch.Tensor
    moments: torch.Tensor
    alpha2: torch.Tensor
    fs: Optional[torch.Tensor]
    q: Optional[torch.Tensor]
    species: List[List[int]]
    origin_stride: int
    remove_com: bool
    r_max: float


@dataclass
class VanHoveDistinctResult:
    """``r`` [n_bins]: the bin centres (A).  ``lags`` [L], ``n_origins`` [L].  ``counts`` [B, P, L, n_bins] int64: the ordered
    (origin, i, j, image) per bin of the distance from i at the origin to j a lag later, the atom's own displaced image left out;
    P = 1 + S (S + 1) / 2, the rows as ``trajectory.pair_row`` numbers them, row 0 the sum of the others.  ``g`` [B, P, L,
    n_bins]: counts V / (n_origins N_a N_b w shell), G_d(r, t) / rho normalised as ``rdf`` normalises g(r) - it tends to 1 at
    large r and at long times, and is g(r) at lag 0.  ``volume`` [B]: V = |det C|."""

    r: torch.Tensor
    lags: np.ndarray
    n_origins: np.ndarray
    counts: torch.Tensor
    g: torch.Tensor
    volume: torch.Tensor
    species: List[List[int]]
    origin_stride: int
    remove_com: bool
    r_max: float


@dataclass
class FqtResult:
    """``q`` [n_bins] (1/A): the centres of the shells of width q_max / n_bins.  ``lags`` [L], ``n_origins`` [L].  ``f`` [B, P, L,
    n_bins]: the mean of ``f_vectors`` over the vectors of each shell, zero where a shell has none; ``n_vectors`` [B, n_bins]
    int64: how many it has.  Rows as ``trajectory.pair_row`` numbers them: row 0 the total ``<Re(rho(t + k) rho(t)*)> / N``, row
    (a, b) the Ashcroft-Langreth partial ``<Re(rho_a(t + k) rho_b(t)*) + Re(rho_b(t + k) rho_a(t)*)> / (2 sqrt(N_a N_b))`` with
    ``rho_a(q, t) = sum_{i in a} exp(i q . r_i(t))``, < > the mean over the origins.  ``hkl[b]`` [V_b, 3] int32 and
    ``f_vectors[b]`` [P, L, V_b]: the reciprocal vectors of structure b inside q_max, as ``structure_factor`` lists them, and F at
    each of them.  At lag 0 (and ``origin_stride`` 1) F is S(q)."""

    q: torch.Tensor
    lags: np.ndarray
    n_origins: np.ndarray
    f: torch.Tensor
    n_vectors: torch.Tensor
    hkl: List[torch.Tensor]
    f_vectors: List[torch.Tensor]
    species: List[List[int]]
    origin_stride: int
    q_max: float


# --- what the functions share ----------------------------------------------------------------------------------------------------------
def _is_int(v) -> bool:
    return isinstance(v, numbers.Integral) and not isinstance(v, (bool, np.bool_))


def _lags(who: str, lags, max_lag, used: int) -> np.ndarray:
    """``lags`` or 0 .. ``max_lag`` -> the lags as int32 [L], checked against the ``used`` frames."""
    if lags is not None and max_lag is not None:
        raise ValueError(f"{who}: give lags or max_lag, not both")
    if lags is None:
        if max_lag is None:
            max_lag = min(used - 1, MAX_LAGS - 1)
        if not _is_int(max_lag) or not 0 <= max_lag <= used - 1:
            raise ValueError(f"{who}: max_lag must be 0 .. {used - 1} (the frames used less one), got {max_lag!r}")
        lags = range(int(max_lag) + 1)
    elif isinstance(lags, (str, bytes)) or not hasattr(lags, "__iter__"):
        raise TypeError(f"{who}: lags must be a sequence of ints, got {type(lags).__name__}")
    lags = list(lags)
    if not all(_is_int(k) for k in lags):
        raise TypeError(f"{who}: lags must be ints, got {lags!r}")
    if not 1 <= len(lags) <= MAX_LAGS:
        raise ValueError(f"{who}: {len(lags)} lags; a call takes 1 .. {MAX_LAGS}")
    if lags[0] < 0 or lags[-1] > used - 1 or any(b <= a for a, b in zip(lags, lags[1:])):
        raise ValueError(f"{who}: lags must be strictly ascending ints in 0 .. {used - 1} (the frames used less one), got "
                         f"{lags if len(lags) <= 16 else lags[:16] + ['...']}")
    return np.asarray(lags, dtype=np.int32)


def _options(who: str, origin_stride, remove_com, masses):
    if not _is_int(origin_stride) or origin_stride < 1:
        raise ValueError(f"{who}: origin_stride must be an int >= 1, got {origin_stride!r}")
    if not isinstance(remove_com, (bool, np.bool_)):
        raise ValueError(f"{who}: remove_com is one bool, got {type(remove_com).__name__}")
    if remove_com and masses is None:
        raise ValueError(f"{who}: remove_com=True needs the masses")
    return int(origin_stride), bool(remove_com)


def _sized(who: str, name: str, *shape) -> Tuple[int, ...]:
    if int(np.prod([int(s) for s in shape], dtype=object)) >= 2 ** 31:
        raise ValueError(f"{who}: {name} would be {list(shape)}, 2^31 elements or more: take fewer lags or bins per call")
    return shape


def _com(who: str, traj, masses, ns, ptr, S, frame0, fstep, used) -> torch.Tensor:
    """The centres of mass [used, B, 3] of the frames used, by ``alignn_traj_com`` through the argument block of
    include/alignn_traj.h."""
    B, dev = len(ns), traj.device
    mass = _masses(who, masses, ns, dev)
    com = torch.empty(used, B, 3, dtype=torch.float64, device=dev)
    args = trajectory.CorrArgs(traj=traj.data_ptr(), masses=mass.data_ptr(), atom_ptr=ptr.data_ptr(), com=com.data_ptr(),
                               n_structs=B, n_atoms=sum(ns), n_species=S, n_total_frames=traj.shape[0], frame0=frame0,
                               frame_step=fstep, n_frames=used, max_lag=0, origin_stride=1, mode=0)
    _lib.check(_lib.bind(trajectory.H).alignn_traj_com(C.byref(args), _lib.stream()), "traj_com")
    return com


def _n_origins(used: int, lags: np.ndarray, stride: int) -> np.ndarray:
    return (used - 1 - lags.astype(np.int64)) // stride + 1


# --- the functions -----------------------------------------------------------------------------------------------------------------
def van_hove_self(traj: torch.Tensor, ns: Sequence[int], species: Optional[Sequence] = None, masses: Optional[Sequence] = None, *,
                  r_max: float, n_bins: int = 200, lags: Optional[Sequence[int]] = None, max_lag: Optional[int] = None,
                  origin_stride: int = 1, remove_com: bool = True, q: Optional[Sequence[float]] = None,
                  start: Optional[int] = None, stop: Optional[int] = None, step: Optional[int] = None) -> VanHoveSelfResult:
    """The self part of the van Hove function of B structures over the frames ``start:stop:step`` of ``traj`` [F, sum ns, 3]
    (float64 on the GPU, Cartesian, not wrapped).  For every structure, lag k, origin t and atom i
    ``d = (r_i(t + k) - r_i(t)) - (c(t + k) - c(t))`` and ``r = sqrt((dx dx + dy dy) + dz dz)`` falls into bin
    ``floor(r (n_bins / r_max))``, or into ``overflow`` from r_max on; see ``VanHoveSelfResult``.  ``lags`` / ``max_lag``,
    ``origin_stride`` and ``remove_com`` (needs ``masses``, B arrays [n_i]) as the module says; without either, every lag up to
    1023.  ``n_bins``: 1 .. 4096.

    ``q``: 1 to 16 magnitudes > 0 in 1/A, for ``fs``, the mean of ``j0(q r) = sin(q r) / (q r)``.  That is the POWDER AVERAGE of
    the self intermediate scattering function ``<exp(i q . d)>``: exact for an isotropic system (a liquid, a glass, a
    polycrystal), and not the value on one lattice vector of a single crystal, where the displacements are anisotropic.

    An empty frame selection is a ``ValueError``, as in ``msd``."""
    who = "van_hove_self"
    r_max, n_bins = _positive(who, "r_max", r_max), bins(who, n_bins, MAX_BINS)
    stride, remove_com = _options(who, origin_stride, remove_com, masses)
    traj, ns = _traj(who, "traj", traj, ns)
    B, N, F, dev = len(ns), sum(ns), traj.shape[0], traj.device
    frame0, fstep, used = _frames(who, F, start, stop, step)
    if used < 1:
        raise ValueError(f"{who}: the frame selection is empty")
    lag = _lags(who, lags, max_lag, used)
    L = len(lag)
    if q is not None:
        qs = [_positive(who, f"q[{u}]", v) for u, v in enumerate(q)] if hasattr(q, "__len__") else None
        if qs is None or not 1 <= len(qs) <= MAX_Q:
            raise ValueError(f"{who}: q must be 1 .. {MAX_Q} magnitudes > 0 (1/A), got {q!r}")
    nq = 0 if q is None else len(qs)
    lib = _load()
    f64 = lambda *shape: torch.empty(*shape, dtype=torch.float64, device=dev)
    i64 = lambda *shape: torch.zeros(*shape, dtype=torch.int64, device=dev)
    with _lib.device_guard(traj):
        ptr, group, count, S, lists = _groups(who, ns, species, dev)
        G = S + 1
        _sized(who, "counts", B, G, L, n_bins)
        com = _com(who, traj, masses, ns, ptr, S, frame0, fstep, used) if remove_com else None
        lag_dev = torch.tensor(lag, dtype=torch.int32, device=dev)
        q_dev = torch.tensor(qs, dtype=torch.float64, device=dev) if nq else None
        counts, overflow = i64(B, G, L, n_bins), i64(B, G, L)
        sums, fs_sum = f64(B, G, L, 2), (f64(B, G, L, nq) if nq else None)
        moments, alpha2, p, gs = f64(B, G, L, 2), f64(B, G, L), f64(B, G, L, n_bins), f64(B, G, L, n_bins)
        fs, centres = (f64(B, G, L, nq) if nq else None), f64(n_bins)
        args = SelfArgs(traj=traj.data_ptr(), atom_ptr=ptr.data_ptr(), group=group.data_ptr(), group_count=count.data_ptr(),
                        com=_lib.ptr(com), lags=lag_dev.data_ptr(), lags_host=lag.ctypes.data, q=_lib.ptr(q_dev),
                        counts=counts.data_ptr(), overflow=overflow.data_ptr(), sums=sums.data_ptr(), fs_sum=_lib.ptr(fs_sum),
                        moments=moments.data_ptr(), alpha2=alpha2.data_ptr(), p=p.data_ptr(), gs=gs.data_ptr(), fs=_lib.ptr(fs),
                        centres=centres.data_ptr(), r_max=r_max, n_structs=B, n_atoms=N, n_species=S, n_bins=n_bins,
                        n_total_frames=F, frame0=frame0, frame_step=fstep, n_frames=used, n_lags=L, origin_stride=stride, n_q=nq)
        _lib.check(lib.alignn_vh_self(C.byref(args), _lib.stream()), "vh_self")
        _lib.check(lib.alignn_vh_self_finish(C.byref(args), _lib.stream()), "vh_self_finish")
    return VanHoveSelfResult(r=centres, lags=lag.astype(np.int64), n_origins=_n_origins(used, lag, stride), counts=counts,
                             overflow=overflow, p=p, gs=gs, moments=moments, alpha2=alpha2, fs=fs, q=q_dev, species=lists,
                             origin_stride=stride, remove_com=remove_com, r_max=r_max)


def van_hove_distinct(traj: torch.Tensor, lattice: torch.Tensor, ns: Sequence[int], species: Optional[Sequence] = None,
                      masses: Optional[Sequence] = None, *, r_max: float, n_bins: int = 200,
                      lags: Optional[Sequence[int]] = None, max_lag: Optional[int] = None, origin_stride: int = 1,
                      remove_com: bool = False, start: Optional[int] = None, stop: Optional[int] = None,
                      step: Optional[int] = None) -> VanHoveDistinctResult:
    """The distinct part of the van Hove function of B structures in fixed cells ``lattice`` [B, 3, 3] over the frames
    ``start:stop:step`` of ``traj``.  For every lag k, origin t and ordered (i, j, image m)
    ``D = (r_j(t + k) - c(t + k)) - (r_i(t) - c(t))`` is wrapped as ``rdf`` wraps a difference - ``df = D Cinv``, ``n =
    rint(df)``, ``df -= n``, ``d0 = df C`` - and moved to the images |m_k| <= floor(r_max / h_k + 1/2) (a range above 8 is a
    ``ValueError``), r >= r_max is dropped.  For j = i the image m = n is left out: ``d0 + n C = D`` is the atom's own unwrapped
    displacement, which belongs to ``van_hove_self`` - also for an atom that moved by more than half a cell, whose wrapped
    displacement (m = 0) is then the image that entered from the next cell and counts; every other image of the atom counts, as
    ``rdf`` counts an atom's own images.  At lag 0 that is exactly ``rdf``'s pairs.  See ``VanHoveDistinctResult``.

    A per-frame lattice [F, B, 3, 3] is a ``ValueError``: a difference between two frames has no single cell.  An empty frame
    selection is a ``ValueError``, as in ``msd``."""
    who = "van_hove_distinct"
    r_max, n_bins = _positive(who, "r_max", r_max), bins(who, n_bins, MAX_BINS)
    stride, remove_com = _options(who, origin_stride, remove_com, masses)
    if isinstance(lattice, torch.Tensor) and lattice.ndim == 4:
        raise ValueError(f"{who}: a per-frame lattice {tuple(lattice.shape)} is not supported: a difference between two frames "
                         f"has no single cell; give one fixed cell per structure, [{len(ns)}, 3, 3]")
    sel = inputs(who, traj, lattice, ns, start, stop, step, per_frame=False, atom_limit=False)
    B, used, dev = len(sel.ns), sel.n_frames, sel.traj.device
    if used < 1:
        raise ValueError(f"{who}: the frame selection is empty")
    lag = _lags(who, lags, max_lag, used)
    L = len(lag)
    lib = _load()
    with _lib.device_guard(sel.traj):
        S, lists = sel.groups(species)
        P = 1 + S * (S + 1) // 2
        _sized(who, "counts", B, P, L, n_bins)
        com = _com(who, sel.traj, masses, sel.ns, sel.atom_ptr, S, sel.frame0, sel.frame_step, used) if remove_com else None
        lag_dev = torch.tensor(lag, dtype=torch.int32, device=dev)
        counts = torch.zeros(B, P, L, n_bins, dtype=torch.int64, device=dev)
        g = torch.empty(B, P, L, n_bins, dtype=torch.float64, device=dev)
        volume, centres = torch.empty(B, dtype=torch.float64, device=dev), torch.empty(n_bins, dtype=torch.float64, device=dev)
        status = torch.zeros(1, dtype=torch.int32, device=dev)
        args = DistinctArgs(com=_lib.ptr(com), lags=lag_dev.data_ptr(), lags_host=lag.ctypes.data, counts=counts.data_ptr(),
                            g=g.data_ptr(), volume=volume.data_ptr(), centres=centres.data_ptr(), r_max=r_max, n_bins=n_bins,
                            n_lags=L, origin_stride=stride, **sel.fields(DistinctArgs, status))
        _lib.check(lib.alignn_vh_distinct(C.byref(args), _lib.stream()), "vh_distinct")
        _lib.check(lib.alignn_vh_distinct_finish(C.byref(args), _lib.stream()), "vh_distinct_finish")
        if int(status.item()) & STATUS_IMAGES:
            raise ValueError(f"{who}: r_max = {r_max} needs periodic images beyond +-{MAX_IMAGE_RANGE} cells along an axis of some "
                             "cell (or a cell is singular): lower r_max or analyse a supercell")
    return VanHoveDistinctResult(r=centres, lags=lag.astype(np.int64), n_origins=_n_origins(used, lag, stride), counts=counts, g=g,
                                 volume=volume, species=lists, origin_stride=stride, remove_com=remove_com, r_max=r_max)


def intermediate_scattering(traj: torch.Tensor, lattice: torch.Tensor, ns: Sequence[int], species: Optional[Sequence] = None, *,
                            q_max: float, n_bins: int = 200, lags: Optional[Sequence[int]] = None, max_lag: Optional[int] = None,
                            origin_stride: int = 1, max_workspace_bytes: int = 2 ** 32, start: Optional[int] = None,
                            stop: Optional[int] = None, step: Optional[int] = None) -> FqtResult:
    """The coherent intermediate scattering function of B structures in fixed cells ``lattice`` [B, 3, 3] over the frames
    ``start:stop:step`` of ``traj``, on the reciprocal-lattice vectors of ``structure_factor`` (``order.reciprocal_vectors``:
    the half space, the order, |h_k| <= 32, |q| < ``q_max`` in 1/A, ``n_bins`` 1 .. 1024 shells).  Three launches: the density
    modes ``rho_a(q, t)`` of every species, frame used and vector into a workspace [F_used, S, V, 2] (formed as ``structure_factor``
    forms them); per vector, pair row and lag the sum over the origins in order; the mean over the vectors of each shell.  See
    ``FqtResult``.  The workspace takes 16 F_used S V bytes: more than ``max_workspace_bytes`` is a ``ValueError`` - take fewer
    frames (``step``), a smaller q_max, or fewer structures per call.

    A per-frame lattice [F, B, 3, 3] is a ``ValueError``: the vectors would move with the frame.  An empty frame selection is a
    ``ValueError``, as in ``msd``."""
    who = "intermediate_scattering"
    q_max, n_bins = _positive(who, "q_max", q_max), bins(who, n_bins, MAX_Q_BINS)
    stride, _ = _options(who, origin_stride, False, None)
    if not _is_int(max_workspace_bytes) or max_workspace_bytes < 0:
        raise ValueError(f"{who}: max_workspace_bytes must be an int >= 0, got {max_workspace_bytes!r}")
    if isinstance(lattice, torch.Tensor) and lattice.ndim == 4:
        raise ValueError(f"{who}: a per-frame lattice {tuple(lattice.shape)} is not supported: F(q, t) is taken on the reciprocal "
                         f"lattice of one fixed cell per structure, [{len(ns)}, 3, 3]")
    sel = inputs(who, traj, lattice, ns, start, stop, step, per_frame=False, atom_limit=False)
    B, used, dev = len(sel.ns), sel.n_frames, sel.traj.device
    if used < 1:
        raise ValueError(f"{who}: the frame selection is empty")
    lag = _lags(who, lags, max_lag, used)
    L = len(lag)
    lib = _load()
    f64 = lambda *shape: torch.zeros(*shape, dtype=torch.float64, device=dev)
    with _lib.device_guard(sel.traj):
        S, lists = sel.groups(species)
        P = 1 + S * (S + 1) // 2
        vec = order.reciprocal_vectors(who, sel, q_max, n_bins)
        V, offsets = vec.n_vectors, vec.offsets
        workspace = 16 * used * S * V
        if workspace > max_workspace_bytes:
            raise ValueError(f"{who}: the workspace of the density modes, [{used}, {S}, {V}, 2] float64, takes {workspace} bytes, "
                             f"more than max_workspace_bytes = {max_workspace_bytes}: take fewer frames, a smaller q_max or fewer "
                             "structures per call")
        _sized(who, "f", B, P, L, n_bins)
        _sized(who, "f_vectors", P, L, max(V, 1))
        modes = torch.empty(used, S, max(V, 1), 2, dtype=torch.float64, device=dev)
        f_vec, f = f64(P, L, max(V, 1)), f64(B, P, L, n_bins)
        n_vectors, centres = torch.zeros(B, n_bins, dtype=torch.int64, device=dev), f64(n_bins)
        lag_dev = torch.tensor(lag, dtype=torch.int32, device=dev)
        args = FqtArgs(vec_ptr=vec.vec_ptr.data_ptr(), hkl=vec.hkl.data_ptr(), vbin=vec.vbin.data_ptr(), lags=lag_dev.data_ptr(),
                       lags_host=lag.ctypes.data, modes=modes.data_ptr(), f_vec=f_vec.data_ptr(), f=f.data_ptr(),
                       n_vectors_bin=n_vectors.data_ptr(), centres=centres.data_ptr(), q_max=q_max, n_bins=n_bins, n_lags=L,
                       origin_stride=stride, n_vectors=V, max_vectors=vec.max_vectors, **sel.fields(FqtArgs, vec.status))
        if V > 0:
            _lib.check(lib.alignn_vh_fqt_modes(C.byref(args), _lib.stream()), "vh_fqt_modes")
            _lib.check(lib.alignn_vh_fqt_correlate(C.byref(args), _lib.stream()), "vh_fqt_correlate")
        _lib.check(lib.alignn_vh_fqt_bin(C.byref(args), _lib.stream()), "vh_fqt_bin")
    spans = [(int(offsets[b]), int(offsets[b + 1])) for b in range(B)]
    return FqtResult(q=centres, lags=lag.astype(np.int64), n_origins=_n_origins(used, lag, stride), f=f, n_vectors=n_vectors,
                     hkl=[vec.hkl[lo:hi] for lo, hi in spans], f_vectors=[f_vec[:, :, lo:hi] for lo, hi in spans], species=lists,
                     origin_stride=stride, q_max=q_max)
