"""Batched structural order of MD trajectories on the device: bond-angle distributions, Steinhardt bond-orientational order
parameters and the static structure factor, for the B structures of a ``run_md`` call together.

``alignn_amd.trajectory`` answers "how far apart" and "how fast"; the functions here answer the next three questions, on the same
tensors (``MDResult.traj_positions`` [n_frames, sum n_i, 3], ``traj_lattices`` under NPT) where they are:

* ``adf``: which bond angles are there - the distribution of the angle j-i-k over the pairs of neighbours of every atom i, per
  species of the centre and per species pair of the neighbours;
* ``steinhardt``: is it still crystalline, and where - q_l per atom and frame, by the addition theorem (no spherical harmonics),
  with the per-frame means per species;
* ``structure_factor``: what a diffraction experiment would see - S(q) on the reciprocal lattice of the (fixed) cell, total and
  Ashcroft-Langreth partials, per vector and in shells of |q|.

Conventions.  Frames (``start`` / ``stop`` / ``step``), groups (0 every atom, 1 .. S the species in ascending atomic number, at
most 8), ``lattices`` ([B, 3, 3] or [F, B, 3, 3]) and the pair rows (``pair_row``) are those of ``alignn_amd.trajectory``, checked
by the functions of alignn_amd/_trajectory_inputs.py that all three modules share; so is the pair geometry: the fractional
difference wrapped by ``rint``, the images |m_k| <= floor(r_cut / h_k + 1/2) of each frame's own cell, an atom's own images
included.  The neighbours of an atom are the (j, image) with r < ``r_cut``, at most 64.  The kernels (csrc/order.hip) are float64 without contraction, the angle histogram is summed with integer atomics (exact), every
floating-point sum has a fixed order over the structure's own rows, frames and vectors: a structure's numbers are the same bits
alone, in a batch and at any place of it.  Read back from the device: the status word of each call and, for
``structure_factor``, the number of reciprocal vectors of every structure (it sizes the lists).  tests/order_ref.py restates the
formulas in numpy; the entry points are declared in include/alignn_order.h, read here with the reader of alignn_amd/_abi.py.

Not here: per-frame cells for S(q), cutoffs per species pair, form-factor weighting.  (The averaged q_l of Lechner and Dellago,
the w_l invariants and common-neighbour analysis are in ``alignn_amd.local_order``.)
"""

from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _abi, _lib
from ._trajectory_inputs import _cutoffs, _positive, _raise_status, bins, degrees, inputs
from .trajectory import pair_row  # noqa: F401  (pair_row numbers the rows of the results)

__all__ = ["adf", "steinhardt", "structure_factor", "reciprocal_vectors", "ReciprocalVectors", "ADFResult", "SteinhardtResult", "SQResult", "MAX_NEIGHBORS", "MAX_L",
           "MAX_HKL", "MAX_BINS", "MAX_IMAGE_RANGE"]

H = _abi.header("alignn_order.h")
HEADER, STRUCTS, SIGNATURES = H.path, H.structs, H.signatures  # the argument blocks; entry point -> (restype, argtypes)
AngleArgs, SqArgs = STRUCTS["alignn_order_angle_args"], STRUCTS["alignn_order_sq_args"]
MAX_SPECIES = H.defines["ALIGNN_ORDER_MAX_SPECIES"]
MAX_IMAGE_RANGE = H.defines["ALIGNN_ORDER_MAX_IMAGE_RANGE"]
MAX_NEIGHBORS = H.defines["ALIGNN_ORDER_MAX_NEIGHBORS"]
MAX_BINS = H.defines["ALIGNN_ORDER_MAX_BINS"]
MAX_L = H.defines["ALIGNN_ORDER_MAX_L"]
MAX_LS = H.defines["ALIGNN_ORDER_MAX_LS"]
MAX_HKL = H.defines["ALIGNN_ORDER_MAX_HKL"]
SQ_FRAME_CHUNK = H.defines["ALIGNN_ORDER_SQ_FRAME_CHUNK"]
STATUS_IMAGES = H.defines["ALIGNN_ORDER_STATUS_IMAGES"]
STATUS_NEIGHBORS = H.defines["ALIGNN_ORDER_STATUS_NEIGHBORS"]
STATUS_HKL = H.defines["ALIGNN_ORDER_STATUS_HKL"]


def _load():
    return _lib.bind(H)


# --- results -----------------------------------------------------------------------------------------------------------------------
@dataclass
class ADFResult:
    """``theta`` [n_bins]: the bin centres in degrees, bins of 180 / n_bins degrees over [0, 180].  ``counts`` [B, S + 1, P,
    n_bins] int64: the triplets (i; j, k), j and k an unordered pair of distinct neighbours of the centre i, per bin of the angle
    at i, summed over the frames used.  First index: the centre's group (0: any).  Second index: ``pair_row`` of the two
    neighbours' groups, P = 1 + S (S + 1) / 2 (0: any pair); neither depends on the S of the call, and every row with a 0 is the
    sum of its specific rows.  ``adf`` [B, S + 1, P, n_bins]: counts / (the row's total x the bin width in degrees), a density
    per degree that integrates to 1 over a row; a row without counts is zeros.  ``species[b]``: the atomic numbers of structure
    b's groups 1 .. S_b.  ``r_cut`` [B] (A): the neighbour cutoff used.  ``n_frames``: frames used."""

    theta: torch.Tensor
    counts: torch.Tensor
    adf: torch.Tensor
    species: List[List[int]]
    r_cut: torch.Tensor
    n_frames: int


@dataclass
class SteinhardtResult:
    """``q`` [F_used, N, L]: q_l of every atom in every frame used, ``q_l(i)^2 = (4 pi / (2l + 1)) sum_m |mean_j Y_lm(r_ij)|^2``
    over the atom's Nb neighbours, evaluated as ``(Nb + 2 sum_{j<k} P_l(cos theta_jk)) / Nb^2``; in [0, 1], 0 for an atom
    without neighbours, 1 with one.  The last axis follows ``ls``.  ``n_neighbors`` [F_used, N] int32: Nb.  ``mean`` [B, S + 1,
    F_used, L]: the mean of q over each group's atoms (0: every atom) per frame; a group without members is zeros.
    ``species[b]``: the atomic numbers of structure b's groups.  ``r_cut`` [B] (A)."""

    q: torch.Tensor
    n_neighbors: torch.Tensor
    mean: torch.Tensor
    ls: Tuple[int, ...]
    species: List[List[int]]
    r_cut: torch.Tensor
    n_frames: int


@dataclass
class SQResult:
    """``q`` [n_bins] (1/A): the centres of the shells of width q_max / n_bins.  ``s`` [B, P, n_bins]: the mean of ``s_vectors``
    over the vectors of each shell, zero where a shell has none; ``n_vectors`` [B, n_bins] int64: how many it has.  Rows as
    ``pair_row`` numbers them: row 0 the total ``<|rho|^2> / N``, row (a, b) the Ashcroft-Langreth partial ``<Re(rho_a
    rho_b*)> / sqrt(N_a N_b)`` with ``rho_a(q) = sum_{i in a} exp(i q . r_i)``, < > the mean over the frames used - S_aa tends
    to 1 and S_ab (a != b) to 0 at large q, and the total is sum_ab sqrt(c_a c_b) S_ab with every a != b counted twice.
    ``hkl[b]`` [V_b, 3] int32 and ``s_vectors[b]`` [P, V_b]: the reciprocal vectors ``q = 2 pi (h0, h1, h2) C^-T`` of structure b
    inside q_max - one of each pair +-q, in lexicographic order - and S at each of them, so that Bragg peaks and anisotropy are
    not lost in the shells.  q = 0 is left out."""

    q: torch.Tensor
    s: torch.Tensor
    n_vectors: torch.Tensor
    hkl: List[torch.Tensor]
    s_vectors: List[torch.Tensor]
    species: List[List[int]]
    n_frames: int
    q_max: float


# --- the reciprocal vectors of fixed cells ---------------------------------------------------------------------------------------------
@dataclass
class ReciprocalVectors:
    """The reciprocal-lattice vectors of B fixed cells inside ``q_max``, as ``alignn_order_sq_vectors`` lists them: ``hkl``
    [V, 3] int32, ``qnorm`` [V] and ``vbin`` [V] int32 (the shell of ``n_bins`` over [0, q_max)) on the device, structure b's at
    ``offsets[b] .. offsets[b + 1]`` (``vec_ptr`` [B + 1] int32: the same on the device); ``n_vectors`` = V, ``max_vectors`` the
    most of one structure.  With V = 0 the three arrays hold one unused element.  ``status`` [1] int32: the word of the call."""

    vec_ptr: torch.Tensor
    hkl: torch.Tensor
    qnorm: torch.Tensor
    vbin: torch.Tensor
    offsets: np.ndarray
    n_vectors: int
    max_vectors: int
    status: torch.Tensor


def reciprocal_vectors(who: str, sel, q_max: float, n_bins: int) -> ReciprocalVectors:
    """The two calls of ``alignn_order_sq_vectors`` - count, read back, list - for the cells of ``sel`` (an ``Inputs`` of
    alignn_amd/_trajectory_inputs.py whose ``groups`` have been set), under the caller's device guard: what ``structure_factor``
    and ``vanhove.intermediate_scattering`` evaluate their sums on.  The half space h0 > 0, or h0 = 0 and h1 > 0, or h0 = h1 = 0
    and h2 > 0, |h_k| <= floor(q_max |C_k| / 2 pi) <= 32, |q| < q_max, in lexicographic order; a ``ValueError`` beyond 32."""
    B, dev = len(sel.ns), sel.traj.device
    lib = _load()
    words = torch.zeros(B + 1, dtype=torch.int32, device=dev)  # the vectors of every structure, then the status word: one copy back
    args = SqArgs(n_vec=words.data_ptr(), q_max=q_max, n_bins=n_bins, **sel.fields(SqArgs, words[B:]))
    _lib.check(lib.alignn_order_sq_vectors(C.byref(args), _lib.stream()), "order_sq_vectors")
    host = words.cpu().numpy()
    if int(host[B]) & STATUS_HKL:
        raise ValueError(f"{who}: q_max = {q_max} needs reciprocal vectors beyond |h| = {MAX_HKL} along an axis of some cell "
                         "(or a cell is singular): lower q_max or analyse a smaller cell")
    n_vec = host[:B].astype(np.int64)
    offsets = np.concatenate([[0], np.cumsum(n_vec)])
    V = int(offsets[-1])
    if V >= 2 ** 31:
        raise ValueError(f"{who}: {V} reciprocal vectors; a call takes fewer than 2^31")
    vec_ptr = torch.tensor(offsets, dtype=torch.int32, device=dev)
    hkl = torch.zeros(max(V, 1), 3, dtype=torch.int32, device=dev)
    qnorm = torch.zeros(max(V, 1), dtype=torch.float64, device=dev)
    vbin = torch.zeros(max(V, 1), dtype=torch.int32, device=dev)
    if V > 0:
        args.vec_ptr, args.hkl, args.qnorm, args.vbin = vec_ptr.data_ptr(), hkl.data_ptr(), qnorm.data_ptr(), vbin.data_ptr()
        args.n_vectors, args.max_vectors = V, int(n_vec.max())
        _lib.check(lib.alignn_order_sq_vectors(C.byref(args), _lib.stream()), "order_sq_vectors")
    return ReciprocalVectors(vec_ptr=vec_ptr, hkl=hkl, qnorm=qnorm, vbin=vbin, offsets=offsets, n_vectors=V,
                             max_vectors=int(n_vec.max()), status=words[B:])


# --- the call of the angle functions  ----------------------------------------------------------------------------------------------
def _angles(who, traj, lattices, ns, species, r_cut, n_bins, ls, start, stop, step):
    """The call of ``alignn_order_angles`` both public functions share: ``n_bins`` given -> the histogram, ``ls`` given -> q."""
    sel = inputs(who, traj, lattices, ns, start, stop, step)
    B, N, used, dev = len(sel.ns), sum(sel.ns), sel.n_frames, sel.traj.device
    lib = _load()
    out = {}
    with _lib.device_guard(sel.traj):
        cut = _cutoffs(who, r_cut, B, dev)
        S, lists = sel.groups(species)
        P = 1 + S * (S + 1) // 2
        status = torch.zeros(1, dtype=torch.int32, device=dev)
        args = AngleArgs(r_cut=cut.data_ptr(), n_bins=1, **sel.fields(AngleArgs, status))
        if n_bins is not None:
            out["counts"] = torch.zeros(B, S + 1, P, n_bins, dtype=torch.int64, device=dev)
            out["adf"] = torch.empty(B, S + 1, P, n_bins, dtype=torch.float64, device=dev)
            out["theta"] = torch.empty(n_bins, dtype=torch.float64, device=dev)
            args.counts, args.adf, args.theta, args.n_bins = out["counts"].data_ptr(), out["adf"].data_ptr(), out["theta"].data_ptr(), n_bins
        if ls is not None:
            L = len(ls)
            out["q"] = torch.zeros(used, N, L, dtype=torch.float64, device=dev)
            out["n_neighbors"] = torch.zeros(used, N, dtype=torch.int32, device=dev)
            out["mean"] = torch.zeros(B, S + 1, used, L, dtype=torch.float64, device=dev)
            args.q, args.n_neighbors, args.mean, args.n_ls = out["q"].data_ptr(), out["n_neighbors"].data_ptr(), out["mean"].data_ptr(), L
            for u, l in enumerate(ls):
                setattr(args, f"l{u}", l)
        _lib.check(lib.alignn_order_angles(C.byref(args), _lib.stream()), "order_angles")
        if n_bins is not None:
            _lib.check(lib.alignn_order_adf_finish(C.byref(args), _lib.stream()), "order_adf_finish")
        if ls is not None:
            _lib.check(lib.alignn_order_steinhardt_mean(C.byref(args), _lib.stream()), "order_steinhardt_mean")
        _raise_status(who, int(status.item()))
    return out, lists, cut, used


# --- the functions -----------------------------------------------------------------------------------------------------------------
def adf(traj: torch.Tensor, lattices: torch.Tensor, ns: Sequence[int], species: Optional[Sequence] = None, *, r_cut,
        n_bins: int = 180, start: Optional[int] = None, stop: Optional[int] = None, step: Optional[int] = None) -> ADFResult:
    """The bond-angle distributions of B structures over the frames ``start:stop:step`` of ``traj`` [F, sum ns, 3] (float64 on the
    GPU, Cartesian, not wrapped).  ``lattices``: [B, 3, 3] for a fixed cell or [F, B, 3, 3] per frame.  ``species``: B integer
    arrays of atomic numbers, or None for one group.  ``r_cut`` (A): one number, or one per structure (a sequence, or a float64
    tensor [B] on the device) - the end of the first neighbour shell.

    For every atom i of every frame and every unordered pair j < k of its neighbours (the (j, image) with r < r_cut, (i, 0) left
    out, at most 64): ``c = ((dxj dxk + dyj dyk) + dzj dzk) / (rj rk)`` clamped to [-1, 1], and theta = acos(c) falls into bin
    ``min(floor(theta n_bins / pi), n_bins - 1)``.  ``n_bins``: 1 .. 1024.  A ``ValueError`` when r_cut needs more than 8 images
    along an axis of some cell, or gives some atom more than 64 neighbours."""
    who = "adf"
    n_bins = bins(who, n_bins, MAX_BINS)
    out, lists, cut, used = _angles(who, traj, lattices, ns, species, r_cut, n_bins, None, start, stop, step)
    return ADFResult(theta=out["theta"], counts=out["counts"], adf=out["adf"], species=lists, r_cut=cut, n_frames=used)


def steinhardt(traj: torch.Tensor, lattices: torch.Tensor, ns: Sequence[int], species: Optional[Sequence] = None, *, r_cut,
               ls: Sequence[int] = (4, 6), start: Optional[int] = None, stop: Optional[int] = None,
               step: Optional[int] = None) -> SteinhardtResult:
    """Steinhardt's bond-orientational order parameters q_l of every atom in every frame used; arguments and neighbours as for
    ``adf``.  ``ls``: 1 to 4 distinct degrees in 1 .. 12.  By the addition theorem
    ``q_l(i)^2 = (Nb + 2 sum_{j<k} P_l(c_jk)) / Nb^2`` with c_jk the cosine of the angle between two neighbours as in ``adf``
    and P_l by the recurrence ``P_{n+1} = ((2n + 1) c P_n - n P_{n-1}) / (n + 1)``; a negative rounding result is clamped to 0
    before the square root.  Perfect first shells: fcc q4 0.19094 q6 0.57452, hcp 0.09722 0.48476, bcc (8 neighbours) 0.50918
    0.62854, simple cubic 0.76376 0.35355."""
    who = "steinhardt"
    ls = degrees(who, ls, MAX_LS, MAX_L)
    out, lists, cut, used = _angles(who, traj, lattices, ns, species, r_cut, None, ls, start, stop, step)
    return SteinhardtResult(q=out["q"], n_neighbors=out["n_neighbors"], mean=out["mean"], ls=ls, species=lists, r_cut=cut,
                            n_frames=used)


def structure_factor(traj: torch.Tensor, lattice: torch.Tensor, ns: Sequence[int], species: Optional[Sequence] = None, *,
                     q_max: float, n_bins: int = 200, start: Optional[int] = None, stop: Optional[int] = None,
                     step: Optional[int] = None) -> SQResult:
    """The static structure factor of B structures in fixed cells ``lattice`` [B, 3, 3] over the frames ``start:stop:step`` of
    ``traj``, on every reciprocal-lattice vector with |q| < ``q_max`` (1/A): the integer triples h of the half space h0 > 0, or
    h0 = 0 and h1 > 0, or h0 = h1 = 0 and h2 > 0, with |h_k| <= floor(q_max |C_k| / 2 pi) <= 32, in lexicographic order.  Per
    frame ``rho_a(q) = sum_{i in a} exp(2 pi i h . f_i)``, f the fractional coordinates; see ``SQResult`` for the rows.  The
    frames are summed in chunks of 64 and the chunks in order, so the bits do not depend on the launch.  ``n_bins``: 1 .. 1024
    shells over [0, q_max).  A per-frame lattice [F, B, 3, 3] is a ``ValueError``: the vectors would move with the frame."""
    who = "structure_factor"
    q_max, n_bins = _positive(who, "q_max", q_max), bins(who, n_bins, MAX_BINS)
    sel = inputs(who, traj, lattice, ns, start, stop, step, per_frame=False, atom_limit=False)
    B, used, dev = len(sel.ns), sel.n_frames, sel.traj.device
    lib = _load()
    f64 = lambda *shape: torch.zeros(*shape, dtype=torch.float64, device=dev)
    with _lib.device_guard(sel.traj):
        S, lists = sel.groups(species)
        P = 1 + S * (S + 1) // 2
        vec = reciprocal_vectors(who, sel, q_max, n_bins)
        offsets, V, hkl = vec.offsets, vec.n_vectors, vec.hkl
        chunks = max(1, -(-used // SQ_FRAME_CHUNK))
        partial, s_vec = f64(chunks, P, max(V, 1)), f64(P, max(V, 1))
        s, n_vectors, centres = f64(B, P, n_bins), torch.zeros(B, n_bins, dtype=torch.int64, device=dev), f64(n_bins)
        args = SqArgs(vec_ptr=vec.vec_ptr.data_ptr(), hkl=hkl.data_ptr(), qnorm=vec.qnorm.data_ptr(), vbin=vec.vbin.data_ptr(),
                      partial=partial.data_ptr(), s_vec=s_vec.data_ptr(), s=s.data_ptr(), n_vectors_bin=n_vectors.data_ptr(),
                      centres=centres.data_ptr(), q_max=q_max, n_bins=n_bins, n_vectors=V, max_vectors=vec.max_vectors,
                      **sel.fields(SqArgs, vec.status))
        if V > 0:
            _lib.check(lib.alignn_order_sq_accumulate(C.byref(args), _lib.stream()), "order_sq_accumulate")
        _lib.check(lib.alignn_order_sq_bin(C.byref(args), _lib.stream()), "order_sq_bin")
    spans = [(int(offsets[b]), int(offsets[b + 1])) for b in range(B)]
    return SQResult(q=centres, s=s, n_vectors=n_vectors, hkl=[hkl[lo:hi] for lo, hi in spans],
                    s_vectors=[s_vec[:, lo:hi] for lo, hi in spans], species=lists, n_frames=used, q_max=q_max)
