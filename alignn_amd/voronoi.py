"""Batched Voronoi analysis of MD trajectories on the device: the Voronoi cell of every atom of every frame - atomic volume,
surface, coordination without a bond cutoff and the Voronoi index <n3, n4, n5, n6, ...> - for the B structures of a ``run_md``
call together.

``alignn_amd.local_order`` names an atom's crystal (``cna``, ``bond_order``) and returns OTHER for a glass, a liquid or a melt;
the Voronoi index is what those are classified by.  On the same tensors (``MDResult.traj_positions`` [n_frames, sum n_i, 3],
``traj_lattices`` under NPT) where they are:

* ``voronoi``: per atom and frame the cell's ``volume``, ``area``, the number of its faces ``n_faces`` and ``index`` (the faces
  with 3, 4, ... 10 edges), after thresholds on small faces and short edges; ``complete``, the certificate that no atom beyond
  ``r_cut`` can cut the cell; the per-frame means per species; with ``faces=True`` the faces themselves (neighbour, displacement,
  area, edges);
* ``voronoi_census``: the most frequent index tuples of one structure and group over all frames.

Conventions.  Frames (``start`` / ``stop`` / ``step``), groups (0 every atom, 1 .. S the species in ascending atomic number, at
most 8), ``lattices`` ([B, 3, 3] or [F, B, 3, 3]) and the neighbour list of an atom - the (j, image) with r < ``r_cut``, (i, 0)
left out, its own images included, at most 64, in the order j ascending, then the image lexicographic - are those of
``alignn_amd.local_order``: the inputs are checked by alignn_amd/_trajectory_inputs.py and the list is built by
csrc/neighbor_list.h.  The cell is cut from the list entries alone, in the centre atom's frame, so a cell smaller than the cutoff
is tessellated through its own images.  The kernels (csrc/voronoi.hip) are float64 without contraction, without floating-point
atomics, every sum in a fixed order over the atom's own list: a structure's numbers are the same bits alone, in a batch and at any
place of it.  Read back from the device: the status word and, with ``strict``, whether every cell is complete.
tests/voronoi_ref.py restates the rules in numpy; the entry points and every formula are in include/alignn_voronoi.h, read here
with the reader of alignn_amd/_abi.py.

Not here: the radical (Laguerre) tessellation with atomic radii, cutoffs per species pair, Voronoi-weighted Steinhardt parameters
or Voronoi neighbours fed into ``cna`` / ``bond_order``, and accumulation inside ``run_md`` without a stored trajectory.
"""

from __future__ import annotations

import ctypes as C
import numbers
from dataclasses import dataclass
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _abi, _lib, order
from ._trajectory_inputs import _cutoffs, _raise_status, inputs

__all__ = ["voronoi", "voronoi_census", "VoronoiResult", "MAX_POLYGON", "MAX_FACES", "N_INDEX"]

H = _abi.header("alignn_voronoi.h")
HEADER, STRUCTS, SIGNATURES = H.path, H.structs, H.signatures  # the argument block; entry point -> (restype, argtypes)
VoroArgs = STRUCTS["alignn_voro_args"]
MAX_NEIGHBORS = H.defines["ALIGNN_VORO_MAX_NEIGHBORS"]
MAX_POLYGON = H.defines["ALIGNN_VORO_MAX_POLYGON"]
MAX_FACES = H.defines["ALIGNN_VORO_MAX_FACES"]
N_INDEX = H.defines["ALIGNN_VORO_INDEX"]  # the last axis of ``index``: faces of 3 .. 10 edges
STATUS_POLYGON = H.defines["ALIGNN_VORO_STATUS_POLYGON"]
STATUS_FACES = H.defines["ALIGNN_VORO_STATUS_FACES"]
for _mine, _theirs in ((H.defines["ALIGNN_VORO_MAX_SPECIES"], order.MAX_SPECIES), (MAX_NEIGHBORS, order.MAX_NEIGHBORS),
                       (H.defines["ALIGNN_VORO_MAX_IMAGE_RANGE"], order.MAX_IMAGE_RANGE),
                       (H.defines["ALIGNN_VORO_STATUS_IMAGES"], order.STATUS_IMAGES),
                       (H.defines["ALIGNN_VORO_STATUS_NEIGHBORS"], order.STATUS_NEIGHBORS)):
    if _mine != _theirs:  # (the limits and the first two status bits are alignn_order.h's, by value)
        raise RuntimeError("include/alignn_voronoi.h and include/alignn_order.h disagree on a limit or a status bit")


def _load():
    return _lib.bind(H)


@dataclass
class VoronoiResult:
    """``volume`` (A^3), ``area`` (A^2), ``r_max`` (A) [F_used, N]: the cell's volume sum_a A_a h_a / 3 and surface sum_a A_a over
    all its faces (A_a the area of the face of list entry a, h_a = |d_a| / 2 its distance from the atom), and the distance of its
    farthest vertex (infinite for an atom without a neighbour inside ``r_cut``).  ``n_faces`` [F_used, N] int32: the counted
    faces - those of an area above ``face_threshold`` and above ``relative_face_threshold`` x ``area`` that have at least 3 edges
    longer than ``edge_threshold``.  ``index`` [F_used, N, 8] int32: the counted faces with 3, 4, .. 10 such edges (one with more
    is in ``n_faces`` only).  ``complete`` [F_used, N] bool: r_max <= r_cut / 2, which no atom outside the list can undo.
    ``mean`` [B, S + 1, F_used, 3]: the mean volume, area and n_faces of each group's complete atoms (0: every atom) per frame,
    zeros for a group with none; ``n_complete`` [B, S + 1, F_used] int64: how many those are.  With ``faces=True`` (else None),
    the counted faces in list order, at most 32: ``face_j`` [F_used, N, 32] int32 the neighbour's index within the structure (-1
    beyond ``n_faces``), ``face_d`` [.., 32, 3] its displacement from the atom, which carries the image, ``face_area`` [.., 32],
    ``face_edges`` [.., 32] int32 (zeros beyond).  ``species[b]``: the atomic numbers of structure b's groups 1 .. S_b;
    ``group`` [N] int32: the group 1 .. S_b of every atom; ``ns``: the atoms per structure.  ``r_cut`` [B] (A)."""

    volume: torch.Tensor
    area: torch.Tensor
    r_max: torch.Tensor
    n_faces: torch.Tensor
    index: torch.Tensor
    complete: torch.Tensor
    mean: torch.Tensor
    n_complete: torch.Tensor
    face_j: Optional[torch.Tensor]
    face_d: Optional[torch.Tensor]
    face_area: Optional[torch.Tensor]
    face_edges: Optional[torch.Tensor]
    species: List[List[int]]
    group: torch.Tensor
    r_cut: torch.Tensor
    ns: List[int]
    n_frames: int
    face_threshold: float
    relative_face_threshold: float
    edge_threshold: float


def _threshold(who: str, name: str, v) -> float:
    if not isinstance(v, numbers.Real) or isinstance(v, (bool, np.bool_)) or not np.isfinite(v) or v < 0:
        raise ValueError(f"{who}: {name} must be a finite number >= 0, got {v!r}")
    return float(v)


def voronoi(traj: torch.Tensor, lattices: torch.Tensor, ns: Sequence[int], species: Optional[Sequence] = None, *, r_cut,
            face_threshold: float = 0.0, relative_face_threshold: float = 0.0, edge_threshold: float = 0.0, faces: bool = False,
            strict: bool = True, start: Optional[int] = None, stop: Optional[int] = None, step: Optional[int] = None) -> VoronoiResult:
    """The Voronoi cells of B structures over the frames ``start:stop:step`` of ``traj`` [F, sum ns, 3] (float64 on the GPU,
    Cartesian, not wrapped).  ``lattices``: [B, 3, 3] for a fixed cell or [F, B, 3, 3] per frame.  ``species``: B integer arrays of
    atomic numbers, or None for one group (they only sort the averages: every atom is a neighbour of every other).  ``r_cut`` (A):
    one number, or one per structure (a sequence, or a float64 tensor [B] on the device) - the radius inside which an atom's
    neighbours are looked for; it has to be at least twice the distance of the farthest vertex of every cell (about twice the
    nearest-neighbour distance of a dense structure) and may give no atom more than 64 entries.

    Entry a of an atom's list, at the displacement d_a, gives the half-space d_a . x <= |d_a|^2 / 2; the cell is their
    intersection and the face of entry a is its plane clipped by every other entry's half-space.  See ``VoronoiResult`` for what
    is taken from the faces.  ``face_threshold`` (A^2), ``relative_face_threshold`` (of the cell's area) and ``edge_threshold``
    (A) leave small faces and short edges out of ``n_faces`` and ``index`` - never out of ``volume`` and ``area``.  In a perfect
    crystal several planes meet in one vertex and roundings open faces of 1e-30 A^2 there: with thresholds of 0 the raw counts of
    such cells depend on rounding (12, 13 or 14 faces for fcc), with ``face_threshold=1e-8, edge_threshold=1e-6`` fcc and ideal
    hcp are <0,12,0,0>, bcc <0,6,0,8>, diamond <12,0,0,4> (its 12 triangles are real, if small) and simple cubic <0,6,0,0>.

    A cell is ``complete`` iff its farthest vertex is within r_cut / 2: a plane of an atom beyond r_cut lies farther out.  Every
    face starts from a square of half-side 4 r_cut, so an unbounded cell - a slab's surface atom next to vacuum, or an r_cut
    that is too small - fails that test by itself.  ``strict=True``: an incomplete cell is a ``ValueError``; ``strict=False``
    (slabs): it keeps ``complete=False`` and its numbers as computed, and is left out of ``mean``.

    A ``ValueError`` too when r_cut needs more than 8 images along an axis of some cell, gives some atom more than 64 entries,
    when a face polygon passes 32 vertices while it is clipped, or, with ``faces=True``, an atom has more than 32 counted faces."""
    who = "voronoi"
    for name, flag in (("faces", faces), ("strict", strict)):
        if not isinstance(flag, (bool, np.bool_)):
            raise ValueError(f"{who}: {name} is one bool, got {flag!r}")
    thresholds = [_threshold(who, name, v) for name, v in (("face_threshold", face_threshold), (
        "relative_face_threshold", relative_face_threshold), ("edge_threshold", edge_threshold))]
    sel = inputs(who, traj, lattices, ns, start, stop, step)
    if sel.n_frames == 0:
        raise ValueError(f"{who}: start / stop / step select no frame of {sel.traj.shape[0]}")
    B, N, used, dev = len(sel.ns), sum(sel.ns), sel.n_frames, sel.traj.device
    lib = _load()
    with _lib.device_guard(sel.traj):
        cut = _cutoffs(who, r_cut, B, dev)
        S, lists = sel.groups(species)
        f64 = lambda *shape: torch.zeros(used, N, *shape, dtype=torch.float64, device=dev)
        i32 = lambda *shape: torch.zeros(used, N, *shape, dtype=torch.int32, device=dev)
        volume, area, r_max, n_faces, index, flag = f64(), f64(), f64(), i32(), i32(N_INDEX), i32()
        mean = torch.zeros(B, S + 1, used, 3, dtype=torch.float64, device=dev)
        n_complete = torch.zeros(B, S + 1, used, dtype=torch.int64, device=dev)
        status = torch.zeros(1, dtype=torch.int32, device=dev)
        stored = {}
        if faces:
            stored = dict(face_j=torch.full((used, N, MAX_FACES), -1, dtype=torch.int32, device=dev), face_d=f64(MAX_FACES, 3),
                          face_area=f64(MAX_FACES), face_edges=i32(MAX_FACES))
        args = VoroArgs(r_cut=cut.data_ptr(), volume=volume.data_ptr(), area=area.data_ptr(), r_max=r_max.data_ptr(),
                        n_faces=n_faces.data_ptr(), index=index.data_ptr(), complete=flag.data_ptr(), mean=mean.data_ptr(),
                        n_complete=n_complete.data_ptr(), face_threshold=thresholds[0], relative_face_threshold=thresholds[1],
                        edge_threshold=thresholds[2], faces=int(faces), **{k: v.data_ptr() for k, v in stored.items()},
                        **sel.fields(VoroArgs, status))
        _lib.check(lib.alignn_voro_cells(C.byref(args), _lib.stream()), "voro_cells")
        _lib.check(lib.alignn_voro_means(C.byref(args), _lib.stream()), "voro_means")
        word = int(status.item())
        _raise_status(who, word)
        if word & STATUS_POLYGON:
            raise ValueError(f"{who}: a face polygon passed {MAX_POLYGON} vertices while it was clipped")
        if word & STATUS_FACES:
            raise ValueError(f"{who}: an atom has more than {MAX_FACES} counted faces, which faces=True cannot store: raise the "
                             "thresholds or pass faces=False")
        complete = flag != 0
        if strict and not bool(complete.all()):
            finite = r_max[torch.isfinite(r_max)]
            reach = f"{float(finite.max()):.6g} A" if finite.numel() else "none"
            raise ValueError(f"{who}: {int((~complete).sum())} cells are not complete inside r_cut (the largest finite r_max is {reach}, "
                             f"r_cut / 2 is at least {float(cut.min()) / 2.0:.6g} A): raise r_cut above twice that r_max, or pass "
                             "strict=False for slabs, whose surface cells are open")
    return VoronoiResult(volume=volume, area=area, r_max=r_max, n_faces=n_faces, index=index, complete=complete, mean=mean,
                         n_complete=n_complete, face_j=stored.get("face_j"), face_d=stored.get("face_d"),
                         face_area=stored.get("face_area"), face_edges=stored.get("face_edges"), species=lists, group=sel.group,
                         r_cut=cut, ns=list(sel.ns), n_frames=used, face_threshold=thresholds[0], relative_face_threshold=thresholds[1],
                         edge_threshold=thresholds[2])


def voronoi_census(result: VoronoiResult, b: int, group: int = 0, top: int = 10) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """The ``top`` most frequent index tuples of structure ``b`` and one group (0: every atom, g: the species
    ``result.species[b][g - 1]``) over all frames and atoms, complete or not -> (``tuples`` [K, 8] int32, ``counts`` [K] int64,
    ``fraction`` [K] = counts / the (frame, atom) pairs of the group), K <= top, the most frequent first, equal counts in ascending
    order of the tuple.  Plain torch on the result."""
    who = "voronoi_census"

    def integer(name, v, low, high):
        if not isinstance(v, numbers.Integral) or isinstance(v, (bool, np.bool_)) or v < low or (high is not None and v > high):
            raise ValueError(f"{who}: {name} must be an int in {low} .. {'' if high is None else high}, got {v!r}")
        return int(v)

    b = integer("b", b, 0, len(result.ns) - 1)
    group = integer("group", group, 0, len(result.species[b]))
    top = integer("top", top, 1, None)
    beg = sum(result.ns[:b])
    rows = result.index[:, beg:beg + result.ns[b]]
    if group:
        rows = rows[:, result.group[beg:beg + result.ns[b]] == group]
    rows = rows.reshape(-1, N_INDEX)
    if rows.shape[0] == 0:
        return rows.new_zeros(0, N_INDEX), torch.zeros(0, dtype=torch.int64, device=rows.device), torch.zeros(
            0, dtype=torch.float64, device=rows.device)
    tuples, counts = torch.unique(rows, dim=0, return_counts=True)  # (sorted ascending by the tuple)
    keep = torch.sort(counts, descending=True, stable=True).indices[:top]
    pairs = torch.full_like(counts[keep], rows.shape[0], dtype=torch.float64)  # (a tensor: the quotient is rounded once)
    return tuples[keep], counts[keep], counts[keep].to(torch.float64) / pairs
