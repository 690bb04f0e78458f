"""Batched local structure of MD trajectories on the device: common-neighbour analysis and the bond-orientational order
parameters q_l, w_l with their averaged forms, for the B structures of a ``run_md`` call together.

``alignn_amd.order`` answers "is it still crystalline"; the functions here answer "which crystal, atom by atom", on the same
tensors (``MDResult.traj_positions`` [n_frames, sum n_i, 3], ``traj_lattices`` under NPT) where they are:

* ``cna``: every atom of every frame as fcc, hcp, bcc, icosahedral or none of these, from the signatures (n_cn, n_b, n_lcb) of
  its bonds (Honeycutt and Andersen; Faken and Jonsson), with a fixed cutoff or with the cutoff taken from the atom's own 12 or
  14 nearest neighbours (after Stukowski's adaptive CNA), and the atoms per class, species and frame;
* ``bond_order``: q_l and w_l of Steinhardt, Nelson and Ronchetti from the complex q_lm, and the averaged q_l, w_l of Lechner and
  Dellago, which separate fcc, hcp, bcc and the liquid at finite temperature where q_l alone does not, with the per-frame means per
  species.

Conventions.  Frames (``start`` / ``stop`` / ``step``), groups (0 every atom, 1 .. S the species in ascending atomic number, at
most 8), ``lattices`` ([B, 3, 3] or [F, B, 3, 3]) and the neighbour list of an atom - the (j, image) with r < ``r_cut``, (i, 0)
left out, its own images included, at most 64, in the order j ascending, then the image lexicographic - are those of
``alignn_amd.order``: the inputs are checked by alignn_amd/_trajectory_inputs.py and the list is built by csrc/neighbor_list.h,
for both.  All geometry is in the centre atom's frame, on the displacements of its list entries, so a cell smaller than the
cutoff is analysed through its own images.  The kernels (csrc/local_order.hip) are float64 without contraction, without
floating-point atomics, every sum in a fixed order over the atom's own list: a structure's numbers are the same bits alone, in a
batch and at any place of it.  Read back from the device: the status word of each call.  tests/local_ref.py restates the rules
in numpy; the entry points and every formula are in include/alignn_local.h, read here with the reader of alignn_amd/_abi.py.

Not here: polyhedral template matching, the diamond signatures of CNA, cutoffs per species pair, solid-angle neighbours.  The
Voronoi tessellation - atomic volumes, neighbours without a cutoff, the Voronoi index - is ``alignn_amd.voronoi``, on the same
neighbour list; its neighbours are not fed into ``cna`` or ``bond_order``.
"""

from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass
from fractions import Fraction
from functools import lru_cache
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _abi, _lib, order
from ._trajectory_inputs import _cutoffs, _raise_status, degrees, inputs

__all__ = ["cna", "bond_order", "CNAResult", "BondOrderResult", "CLASSES", "SIGNATURES_COUNTED", "wigner_3j_table", "ylm_norms"]

H = _abi.header("alignn_local.h")
HEADER, STRUCTS, SIGNATURES = H.path, H.structs, H.signatures  # the argument blocks; entry point -> (restype, argtypes)
CnaArgs, BondArgs = STRUCTS["alignn_local_cna_args"], STRUCTS["alignn_local_bond_args"]
MAX_NEIGHBORS = H.defines["ALIGNN_LOCAL_MAX_NEIGHBORS"]
MAX_L = H.defines["ALIGNN_LOCAL_MAX_L"]
MAX_LS = H.defines["ALIGNN_LOCAL_MAX_LS"]
N_CLASSES = H.defines["ALIGNN_LOCAL_CLASSES"]
N_SIGNATURES = H.defines["ALIGNN_LOCAL_SIGNATURES"]
M_STRIDE = H.defines["ALIGNN_LOCAL_M_STRIDE"]
W3J_STRIDE = H.defines["ALIGNN_LOCAL_W3J_STRIDE"]
CLASSES = ("OTHER", "FCC", "HCP", "BCC", "ICO")  # the values of ``CNAResult.structure``
SIGNATURES_COUNTED = ((4, 2, 1), (4, 2, 2), (4, 4, 4), (5, 5, 5), (6, 6, 6))  # the last axis of ``signature_counts``
# the q_lm of one chunk of frames are kept between the two passes of ``bond_order``: at most this many bytes (a chunk is at least
# one frame, so a frame of more than 64 MiB / (L x 13 x 16 B) = 80 000 atoms at L = 4 takes what it needs)
QLM_SCRATCH_BYTES = 64 << 20
for _mine, _theirs in ((H.defines["ALIGNN_LOCAL_MAX_SPECIES"], order.MAX_SPECIES), (MAX_NEIGHBORS, order.MAX_NEIGHBORS),
                       (H.defines["ALIGNN_LOCAL_MAX_IMAGE_RANGE"], order.MAX_IMAGE_RANGE), (MAX_L, order.MAX_L), (MAX_LS, order.MAX_LS),
                       (H.defines["ALIGNN_LOCAL_STATUS_IMAGES"], order.STATUS_IMAGES),
                       (H.defines["ALIGNN_LOCAL_STATUS_NEIGHBORS"], order.STATUS_NEIGHBORS)):
    if _mine != _theirs:  # (the limits and status bits are alignn_order.h's, by value)
        raise RuntimeError("include/alignn_local.h and include/alignn_order.h disagree on a limit or a status bit")


def _load():
    return _lib.bind(H)


# --- results -----------------------------------------------------------------------------------------------------------------------
@dataclass
class CNAResult:
    """``structure`` [F_used, N] int32: 0 OTHER, 1 FCC, 2 HCP, 3 BCC, 4 ICO (``CLASSES``).  ``signature_counts`` [F_used, N, 5]
    int32: the atom's bonds with the signature (4,2,1), (4,2,2), (4,4,4), (5,5,5), (6,6,6); with ``adaptive`` those of the stage
    that gave the class, else those of the 14 nearest, zeros with fewer than 14.  ``n_neighbors`` [F_used, N] int32: the entries
    inside ``r_cut``.  ``counts`` [B, S + 1, F_used, 5] int64: atoms per group (0: every atom), frame and class; ``fraction``:
    counts / the group's atoms, zeros for a group without members.  ``species[b]``: the atomic numbers of structure b's groups
    1 .. S_b.  ``r_cut`` [B] (A): the cutoff, or with ``adaptive`` the search radius."""

    structure: torch.Tensor
    signature_counts: torch.Tensor
    n_neighbors: torch.Tensor
    counts: torch.Tensor
    fraction: torch.Tensor
    species: List[List[int]]
    r_cut: torch.Tensor
    n_frames: int
    adaptive: bool


@dataclass
class BondOrderResult:
    """``q``, ``w`` [F_used, N, L]: q_l = sqrt(4 pi / (2l + 1) s_l) and w_l = t_l / s_l^(3/2) of every atom, with
    ``s_l = sum_m |q_lm|^2`` and ``t_l = sum_{m1 + m2 + m3 = 0} (l l l; m1 m2 m3) q_lm1 q_lm2 q_lm3`` of
    ``q_lm(i) = mean over the atom's Nb list entries of Y_lm``; ``q_avg``, ``w_avg``: the same of
    ``qbar_lm(i) = (q_lm(i) + sum over the entries (j, image) of i of q_lm(j)) / (Nb + 1)`` (None with ``average=False``).
    ``s``, ``t``, ``s_avg``, ``t_avg``: the sums themselves, of order one, where q and w magnify roundings without limit as s
    tends to 0 (w is 0 where s is).  The last axis follows ``ls``.  ``n_neighbors`` [F_used, N] int32: Nb.  ``mean`` [B, S + 1,
    F_used, 4, L]: the mean of q, q_avg, w, w_avg (in that order; zeros for those that are None) over each group's atoms (0: every
    atom) per frame, a group without members zeros.  ``species[b]``: the atomic numbers of structure b's groups.  ``r_cut`` [B]."""

    q: torch.Tensor
    w: torch.Tensor
    q_avg: Optional[torch.Tensor]
    w_avg: Optional[torch.Tensor]
    s: torch.Tensor
    t: torch.Tensor
    s_avg: Optional[torch.Tensor]
    t_avg: Optional[torch.Tensor]
    n_neighbors: torch.Tensor
    mean: torch.Tensor
    ls: Tuple[int, ...]
    species: List[List[int]]
    r_cut: torch.Tensor
    n_frames: int


# --- the tables of the harmonics (host) --------------------------------------------------------------------------------------------
@lru_cache(maxsize=None)
def wigner_3j_table(l: int) -> np.ndarray:
    """The Wigner 3j symbols (l l l; m1 m2 m3) [2l + 1, 2l + 1] at [m1 + l, m2 + l], m3 = -(m1 + m2), zero where |m3| > l: Racah's
    formula in integers - with D = (l!)^3 / (3l + 1)!, p = the product of (l + m_k)! (l - m_k)! and the integer
    A = l!^3 sum_k (-1)^k C(l, k) C(l, l - m1 - k) C(l, l + m2 - k), the symbol is (-1)^m3 sign(A) sqrt(D p A^2 / l!^6) - and
    one square root of the correctly rounded quotient in float64."""
    fact = [math.factorial(k) for k in range(3 * l + 2)]
    out = np.zeros((2 * l + 1, 2 * l + 1))
    for m1 in range(-l, l + 1):
        for m2 in range(-l, l + 1):
            m3 = -(m1 + m2)
            if abs(m3) > l:
                continue
            total = 0  # sum_k (-1)^k l!^3 / (k! (l - k)! (l - m1 - k)! (m1 + k)! (l + m2 - k)! (k - m2)!), an integer
            for k in range(max(0, -m1, m2), min(l, l - m1, l + m2) + 1):
                total += (-1) ** k * math.comb(l, k) * math.comb(l, l - m1 - k) * math.comb(l, l + m2 - k)
            prod = 1
            for m in (m1, m2, m3):
                prod *= fact[l + m] * fact[l - m]
            square = Fraction(prod * total * total, fact[3 * l + 1] * fact[l] ** 3)  # D p A^2 / l!^6
            sign = (-1) ** (m3 % 2) * (1 if total >= 0 else -1)
            out[m1 + l, m2 + l] = sign * math.sqrt(float(square))
    out.setflags(write=False)
    return out


@lru_cache(maxsize=None)
def ylm_norms() -> np.ndarray:
    """[MAX_L + 1, M_STRIDE]: sqrt(((2l + 1) (l - m)! / (l + m)!) / (4 pi)) at [l, m], m <= l, the quotient of integers correctly
    rounded first."""
    out = np.zeros((MAX_L + 1, M_STRIDE))
    for l in range(MAX_L + 1):
        for m in range(l + 1):
            out[l, m] = math.sqrt(float(Fraction((2 * l + 1) * math.factorial(l - m), math.factorial(l + m))) / (4.0 * math.pi))
    out.setflags(write=False)
    return out


# --- the functions -----------------------------------------------------------------------------------------------------------------
def cna(traj: torch.Tensor, lattices: torch.Tensor, ns: Sequence[int], species: Optional[Sequence] = None, *, r_cut,
        adaptive: bool = False, start: Optional[int] = None, stop: Optional[int] = None, step: Optional[int] = None) -> CNAResult:
    """Common-neighbour analysis of B structures over the frames ``start:stop:step`` of ``traj`` [F, sum ns, 3] (float64 on the
    GPU, Cartesian, not wrapped).  ``lattices``: [B, 3, 3] for a fixed cell or [F, B, 3, 3] per frame.  ``species``: B integer
    arrays of atomic numbers, or None for one group (they only sort the counts: every atom is a neighbour of every other).
    ``r_cut`` (A): one number, or one per structure (a sequence, or a float64 tensor [B] on the device).

    With d_a the displacement of list entry a from the centre, two entries are bonded iff |d_a - d_b| < r_c.  The signature of
    entry a: n_cn, the entries bonded to it (the neighbours it has in common with the centre); n_b, the bonded pairs among them;
    n_lcb, the bonds of the largest connected component of those bonds.  12 entries, all (4,2,1): FCC; 6 x (4,2,1) and 6 x
    (4,2,2): HCP; 14 entries, 6 x (4,4,4) and 8 x (6,6,6): BCC; 12 x (5,5,5): ICO; anything else OTHER.

    ``adaptive=False``: every entry counts and r_c = r_cut - for fcc and hcp between the first and the second shell, for bcc
    between the second and the third.  ``adaptive=True``: r_cut is only the search radius (it must reach the 14 nearest and give
    no atom more than 64).  The entries are sorted by distance, ties by list order; the 12 nearest with
    ``r_c = (1 + sqrt 2) / 2 x their mean distance`` are tested for FCC, HCP and ICO, then the 14 nearest with
    ``r_c = (1 + sqrt 2) / 2 x ((2 / sqrt 3) (r_1 + .. + r_8) + (r_9 + .. + r_14)) / 14`` for BCC; a stage with fewer entries than
    it needs does not match.  The rule follows Stukowski's adaptive CNA in spirit and is stated here as this package's own.

    A ``ValueError`` when r_cut needs more than 8 images along an axis of some cell, or gives some atom more than 64 entries."""
    who = "cna"
    if not isinstance(adaptive, (bool, np.bool_)):
        raise ValueError(f"{who}: adaptive is one bool, got {adaptive!r}")
    sel = inputs(who, traj, lattices, ns, start, stop, step)
    B, N, used, dev = len(sel.ns), sum(sel.ns), sel.n_frames, sel.traj.device
    lib = _load()
    with _lib.device_guard(sel.traj):
        cut = _cutoffs(who, r_cut, B, dev)
        S, lists = sel.groups(species)
        structure = torch.zeros(used, N, dtype=torch.int32, device=dev)
        signatures = torch.zeros(used, N, N_SIGNATURES, dtype=torch.int32, device=dev)
        n_neighbors = torch.zeros(used, N, dtype=torch.int32, device=dev)
        counts = torch.zeros(B, S + 1, used, N_CLASSES, dtype=torch.int64, device=dev)
        fraction = torch.zeros(B, S + 1, used, N_CLASSES, dtype=torch.float64, device=dev)
        status = torch.zeros(1, dtype=torch.int32, device=dev)
        args = CnaArgs(r_cut=cut.data_ptr(), structure=structure.data_ptr(), signature_counts=signatures.data_ptr(),
                       n_neighbors=n_neighbors.data_ptr(), counts=counts.data_ptr(), fraction=fraction.data_ptr(),
                       adaptive=int(adaptive), **sel.fields(CnaArgs, status))
        _lib.check(lib.alignn_local_cna(C.byref(args), _lib.stream()), "local_cna")
        _lib.check(lib.alignn_local_cna_counts(C.byref(args), _lib.stream()), "local_cna_counts")
        _raise_status(who, int(status.item()))
    return CNAResult(structure=structure, signature_counts=signatures, n_neighbors=n_neighbors, counts=counts, fraction=fraction,
                     species=lists, r_cut=cut, n_frames=used, adaptive=bool(adaptive))


def bond_order(traj: torch.Tensor, lattices: torch.Tensor, ns: Sequence[int], species: Optional[Sequence] = None, *, r_cut,
               ls: Sequence[int] = (4, 6), average: bool = True, start: Optional[int] = None, stop: Optional[int] = None,
               step: Optional[int] = None) -> BondOrderResult:
    """The bond-orientational order parameters of every atom in every frame used; arguments and neighbours as for ``cna``.
    ``ls``: 1 to 4 distinct degrees in 1 .. 12.  See ``BondOrderResult`` for the definitions; the harmonics are evaluated as a
    polynomial in z times a power of (x + i y), only m >= 0 is kept (q_{l,-m} = (-1)^m conj(q_lm)), and the 3j symbols come from
    ``wigner_3j_table``.  In the averaged forms every list entry counts once: the same j through several images, and the atom
    through its own images.  Perfect crystals (q4, q6, w4, w6): fcc 0.190941 0.574524 -0.159317 -0.013161, hcp 0.097222 0.484762
    +0.134097 -0.012442, bcc with 14 neighbours 0.036370 0.510688 +0.159317 +0.013161, icosahedron q6 0.663325 w6 -0.169754.

    Two passes over chunks of frames: the first writes the q_lm of the chunk, the second builds the same lists again and gathers
    them; no list is stored, and the q_lm of at most ``QLM_SCRATCH_BYTES`` (a whole frame at the least) at a time."""
    who = "bond_order"
    ls = degrees(who, ls, MAX_LS, MAX_L)
    if not isinstance(average, (bool, np.bool_)):
        raise ValueError(f"{who}: average is one bool, got {average!r}")
    sel = inputs(who, traj, lattices, ns, start, stop, step)
    B, N, used, dev, L = len(sel.ns), sum(sel.ns), sel.n_frames, sel.traj.device, len(ls)
    lib = _load()
    with _lib.device_guard(sel.traj):
        cut = _cutoffs(who, r_cut, B, dev)
        S, lists = sel.groups(species)
        f64 = lambda: torch.zeros(used, N, L, dtype=torch.float64, device=dev)
        out = {k: f64() for k in ("s", "t", "q", "w")}
        if average:
            out.update({k: f64() for k in ("s_avg", "t_avg", "q_avg", "w_avg")})
        n_neighbors = torch.zeros(used, N, dtype=torch.int32, device=dev)
        status = torch.zeros(1, dtype=torch.int32, device=dev)
        table = np.zeros((L, W3J_STRIDE))
        for u, l in enumerate(ls):
            table[u, :(2 * l + 1) ** 2] = wigner_3j_table(l).reshape(-1)
        w3j, ynorm = torch.tensor(table, device=dev), torch.tensor(np.array(ylm_norms()), device=dev)
        per_frame = N * L * M_STRIDE * 16  # the bytes of a frame's q_lm
        chunk = max(1, min(used, QLM_SCRATCH_BYTES // per_frame))
        qlm = torch.empty(chunk, N, L, M_STRIDE, 2, dtype=torch.float64, device=dev)
        degree = {f"l{u}": l for u, l in enumerate(ls)}
        args = BondArgs(r_cut=cut.data_ptr(), ynorm=ynorm.data_ptr(), w3j=w3j.data_ptr(), qlm=qlm.data_ptr(),
                        n_neighbors=n_neighbors.data_ptr(), average=int(average), n_ls=L, **{k: v.data_ptr() for k, v in out.items()},
                        **degree, **sel.fields(BondArgs, status))
        for chunk0 in range(0, used, chunk):
            args.chunk0, args.chunk_frames = chunk0, min(chunk, used - chunk0)
            _lib.check(lib.alignn_local_bond_qlm(C.byref(args), _lib.stream()), "local_bond_qlm")
            _lib.check(lib.alignn_local_bond_finish(C.byref(args), _lib.stream()), "local_bond_finish")
        # the group means, in the summation order of alignn_order_steinhardt_mean: that entry point on each array
        mean = torch.zeros(B, S + 1, used, 4, L, dtype=torch.float64, device=dev)
        olib = order._load()
        for k, name in enumerate(("q", "q_avg", "w", "w_avg")):
            if name not in out:
                continue
            one = torch.zeros(B, S + 1, used, L, dtype=torch.float64, device=dev)
            margs = order.AngleArgs(q=out[name].data_ptr(), mean=one.data_ptr(), n_bins=1, n_ls=L, **degree,
                                    **sel.fields(order.AngleArgs, status))
            _lib.check(olib.alignn_order_steinhardt_mean(C.byref(margs), _lib.stream()), "order_steinhardt_mean")
            mean[:, :, :, k] = one
        _raise_status(who, int(status.item()))
    return BondOrderResult(q=out["q"], w=out["w"], q_avg=out.get("q_avg"), w_avg=out.get("w_avg"), s=out["s"], t=out["t"],
                           s_avg=out.get("s_avg"), t_avg=out.get("t_avg"), n_neighbors=n_neighbors, mean=mean, ls=ls, species=lists,
                           r_cut=cut, n_frames=used)
