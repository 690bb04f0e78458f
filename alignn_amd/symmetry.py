"""Batched crystal symmetry on the device: the space-group operations of B crystals found together, the atom permutations and
orbits that follow from them, and the projection of forces, stresses and positions onto the symmetric subspace.

The reference gets its symmetry from spglib through jarvis' ``Spacegroup3D``, one structure at a time on the host.  Here:

* ``find_symmetry``: every operation {W | t} of every structure (centring and supercell translations included), with the atom
  map and the lattice shift of each, the orbits, the counts and the crystal system;
* ``symmetrize_forces`` / ``symmetrize_stress`` / ``symmetrize_positions``: one launch each for the whole batch;
* ``distinct_miller_indices``: the symmetry-distinct surfaces up to an index, for ``surface_energy(miller_indices=...)``;
  ``vacancy_formation(site_labels="auto")`` uses the orbits as its classes of sites.

An operation acts on fractional column coordinates as x' = W x + t (the cell's rows are the lattice vectors), W an integer
matrix with det +-1 in the basis of the cell AS GIVEN - the search reduces or standardises no cell, entries of W may exceed +-1;
``primitive_cell`` and ``conventional_cell`` of alignn_amd/cells.py take the step from these operations to cells - and t in
[0, 1).  ``symprec`` is a length in A: lattice vectors keep their lengths and the lengths of their differences within it, and
every atom's image lies within it of an atom of its species.  The definitions are stated in include/alignn_sym.h (read here with
the reader of alignn_amd/_abi.py) and restated in numpy by tests/sym_ref.py.  The kernels (csrc/symmetry.hip) are float64 without
contraction and without floating-point atomics, every sum in a fixed order: a structure's results are the same bits alone, in a
batch and at any place of it.  One array of B x 8 integers (counts, crystal system, status) is read back between the search and
the launch that fills the results; nothing else.

Not here: space-group numbers and symbols, Wyckoff letters, symmetrising the lattice itself (primitive and conventional cells:
alignn_amd/cells.py; rotations of a supercell's crystal that do not keep the supercell are not among its operations), symmetry-reduced strains and q-meshes, a symmetry constraint inside ``relax``, magnetic or site-property-aware
symmetry.  (Symmetry-reduced displacements: ``phonons(displacements="symmetry", symmetry=...)``, alignn_amd/phonons.py.)
"""

from __future__ import annotations

import ctypes as C
import itertools
import numbers
from dataclasses import dataclass, field
from math import gcd
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _abi, _lib
from ._structures import host, shape_of

__all__ = ["find_symmetry", "symmetrize_forces", "symmetrize_stress", "symmetrize_positions", "distinct_miller_indices",
           "SymmetryResult", "CRYSTAL_SYSTEMS", "MAX_ATOMS", "MAX_IMAGE_RANGE"]

H = _abi.header("alignn_sym.h")
HEADER, STRUCTS, SIGNATURES = H.path, H.structs, H.signatures  # the argument blocks; entry point -> (restype, argtypes)
FindArgs, ApplyArgs = STRUCTS["alignn_sym_find_args"], STRUCTS["alignn_sym_apply_args"]
MAX_ATOMS = H.defines["ALIGNN_SYM_MAX_ATOMS"]
MAX_IMAGE_RANGE = H.defines["ALIGNN_SYM_MAX_IMAGE_RANGE"]
MAX_CANDIDATES = H.defines["ALIGNN_SYM_MAX_CANDIDATES"]
MAX_LATTICE_OPS = H.defines["ALIGNN_SYM_MAX_LATTICE_OPS"]
INFO = H.defines["ALIGNN_SYM_INFO"]
STATUS_IMAGES = H.defines["ALIGNN_SYM_STATUS_IMAGES"]
STATUS_OVERFLOW = H.defines["ALIGNN_SYM_STATUS_OVERFLOW"]
STATUS_INPUT = H.defines["ALIGNN_SYM_STATUS_INPUT"]
CRYSTAL_SYSTEMS = ("triclinic", "monoclinic", "orthorhombic", "tetragonal", "trigonal", "hexagonal", "cubic")


def _load():
    return _lib.bind(H)


@dataclass
class SymmetryResult:
    """Per structure b (lists of B entries; the tensors are views of packed device arrays):

    ``rotations[b]`` [G, 3, 3] int32 and ``translations[b]`` [G, 3]: the operations x' = W x + t, sorted by the nine entries of W
    row-major, then by the atom the pivot atom is sent to.  ``atom_map[b]`` [G, n] int32: operation g sends atom i onto atom
    ``atom_map[b][g, i]`` of the structure, and ``shifts[b]`` [G, n, 3] int32 is the lattice vector in between:
    W x_i + t = x_map + shift (to within symprec).  ``orbits[b]`` [n] int32: the lowest atom that atom i is equivalent to.
    ``n_ops[b]`` = G; ``n_translations[b]``: the operations with W = I (1 for a primitive cell); ``point_group_order[b]``: the
    distinct W; ``crystal_system[b]``: one of ``CRYSTAL_SYSTEMS``.  ``ns``: the atom counts; ``symprec``: as searched."""

    rotations: List[torch.Tensor]
    translations: List[torch.Tensor]
    atom_map: List[torch.Tensor]
    shifts: List[torch.Tensor]
    orbits: List[torch.Tensor]
    n_ops: List[int]
    n_translations: List[int]
    point_group_order: List[int]
    crystal_system: List[str]
    ns: List[int]
    symprec: float
    packed: dict = field(default_factory=dict, repr=False)  # the packed device arrays the symmetrisers take


def _stack_lattices(who: str, lattices, B: int, dev) -> torch.Tensor:
    if isinstance(lattices, torch.Tensor):
        lat = lattices.to(dev, torch.float64)
    else:
        lat = torch.stack([torch.as_tensor(host(x), dtype=torch.float64) for x in lattices]).to(dev)
    if tuple(lat.shape) != (B, 3, 3):
        raise ValueError(f"{who}: lattices must be {B} cells [3, 3], got {tuple(lat.shape)}")
    return lat.contiguous()


def _sorting(who: str, ns: List[int], species):
    """Per structure the stable sort of its atoms by species: -> (order, seg_lo, seg_hi [N], pivot_lo, pivot_hi [B])."""
    B = len(ns)
    if species is not None and len(species) != B:
        raise ValueError(f"{who}: species needs one integer array per structure ({B}) or None, got {len(species)}")
    order, lo, hi, plo, phi = [], [], [], [], []
    for b, n in enumerate(ns):
        z = np.zeros(n, dtype=np.int64) if species is None else host(species[b])
        if z.shape != (n,) or z.dtype.kind not in "iu":
            raise ValueError(f"{who}: species[{b}] is {z.dtype} {z.shape}, need integers [{n}]")
        o = np.argsort(z, kind="stable")
        kinds, first, count = np.unique(z[o], return_index=True, return_counts=True)
        which = np.repeat(np.arange(len(kinds)), count)
        order.append(o)
        lo.append(first[which])
        hi.append((first + count)[which])
        pivot = int(np.argmin(count))  # (the first minimum: the lowest species number among equals)
        plo.append(first[pivot])
        phi.append(first[pivot] + count[pivot])
    cat = lambda xs: np.concatenate(xs).astype(np.int32)
    return cat(order), cat(lo), cat(hi), np.array(plo, dtype=np.int32), np.array(phi, dtype=np.int32)


def find_symmetry(lattices: Sequence, positions: Sequence, species: Optional[Sequence] = None, *, symprec: float = 1e-3,
                  device=None) -> SymmetryResult:
    """The space-group operations of B crystals.  ``lattices``: B cells [3, 3] (rows are lattice vectors) or a [B, 3, 3] tensor;
    ``positions``: B Cartesian [n_s, 3] arrays; ``species``: B integer arrays [n_s], None: all atoms alike; ``symprec``: a
    length in A, > 0.  Runs on ``device`` (default: the current GPU).

    The lattice operations are searched among the lattice vectors n A with |n_k| <= floor((max_i |a_i| + symprec) / h_k), h_k the
    cell's heights; a structure that needs more than 8 on an axis (a very skewed or flat cell) raises ``ValueError`` naming it,
    as does one with more than 1024 atoms.  The error carries the results of the other structures as its ``result`` attribute.

    A limit: every operation is accepted or rejected on its own, so with per-atom noise near ``symprec`` the accepted set need
    not be a group.  The 2x2x2 supercell of fluorite (96 atoms, 1536 operations) with one draw of uniform noise of 2e-4 A has,
    at ``symprec`` 1e-3, 1534 of them, the closest decision 0.8 % of symprec from the threshold; with 4e-4 A, 14 operations
    with 12 distinct rotations and 2 pure translations, so that ``n_ops != point_group_order * n_translations`` and products of
    operations are missing.  This is not changed here.  What the tests pin holds where no comparison falls
    within 5 % of ``symprec``; keep the noise of a structure well below it, or ``symprec`` well above the noise."""
    who = "find_symmetry"
    B = len(positions)
    if B == 0 or len(lattices) != B:
        raise ValueError(f"{who}: {len(lattices)} lattices, {B} position arrays (need the same number, at least one)")
    if B > 65535:
        raise ValueError(f"{who}: {B} structures; a call takes at most 65535")
    ns = []
    for i, p in enumerate(positions):
        sh = shape_of(p)
        if len(sh) != 2 or sh[1] != 3 or sh[0] < 1:
            raise ValueError(f"{who}: positions[{i}] is {sh}, need [n_i, 3] with n_i >= 1")
        if sh[0] > MAX_ATOMS:
            raise ValueError(f"{who}: structure {i} has {sh[0]} atoms; at most {MAX_ATOMS} are supported")
        ns.append(int(sh[0]))
    if not isinstance(symprec, numbers.Real) or isinstance(symprec, (bool, np.bool_)) or not np.isfinite(symprec) or symprec <= 0:
        raise ValueError(f"{who}: symprec must be a finite length > 0, got {symprec!r}")
    order, lo, hi, plo, phi = _sorting(who, ns, species)
    dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    if dev.type != "cuda":
        raise TypeError(f"{who} runs on the GPU (its launches are HIP only), got device {dev}")
    lib = _load()
    N = sum(ns)
    ptr = np.concatenate([[0], np.cumsum(ns)])
    with _lib.device_guard(torch.empty(0, device=dev)):
        lat = _stack_lattices(who, lattices, B, dev)
        pos = torch.cat([torch.as_tensor(p).to(dev, torch.float64) for p in positions]).contiguous()
        i32 = lambda x: torch.tensor(np.ascontiguousarray(x), dtype=torch.int32, device=dev)
        i64 = lambda x: torch.tensor(np.ascontiguousarray(x), dtype=torch.int64, device=dev)
        atom_ptr, order_d, lo_d, hi_d, plo_d, phi_d = i32(ptr), i32(order), i32(lo), i32(hi), i32(plo), i32(phi)
        frac = torch.empty(N, 3, dtype=torch.float64, device=dev)
        lattice_ops = torch.zeros(B, MAX_LATTICE_OPS, 9, dtype=torch.int32, device=dev)
        accepted = torch.zeros(MAX_LATTICE_OPS * N, dtype=torch.uint8, device=dev)
        op_count = torch.zeros(B, MAX_LATTICE_OPS, dtype=torch.int32, device=dev)
        info = torch.zeros(B, INFO, dtype=torch.int32, device=dev)
        orbits = torch.empty(N, dtype=torch.int32, device=dev)
        args = FindArgs(lattice=lat.data_ptr(), pos=pos.data_ptr(), atom_ptr=atom_ptr.data_ptr(), order=order_d.data_ptr(),
                        seg_lo=lo_d.data_ptr(), seg_hi=hi_d.data_ptr(), pivot_lo=plo_d.data_ptr(), pivot_hi=phi_d.data_ptr(),
                        frac=frac.data_ptr(), lattice_ops=lattice_ops.data_ptr(), accepted=accepted.data_ptr(),
                        op_count=op_count.data_ptr(), info=info.data_ptr(), symprec=float(symprec), n_structs=B, n_atoms=N,
                        max_atoms=max(ns))
        _lib.check(lib.alignn_sym_search(C.byref(args), _lib.stream()), "sym_search")
        got = info.cpu().numpy()  # the one read-back: counts, crystal system and status of every structure
        n_ops = [int(v) for v in got[:, 0]]
        op_ptr = np.concatenate([[0], np.cumsum(n_ops)]).astype(np.int64)
        map_ptr = np.concatenate([[0], np.cumsum([g * n for g, n in zip(n_ops, ns)])]).astype(np.int64)
        G, Mt = int(op_ptr[-1]), int(map_ptr[-1])
        op_ptr_d, map_ptr_d = i64(op_ptr), i64(map_ptr)
        rotations = torch.empty(G, 3, 3, dtype=torch.int32, device=dev)
        translations = torch.empty(G, 3, dtype=torch.float64, device=dev)
        atom_map = torch.empty(Mt, dtype=torch.int32, device=dev)
        shifts = torch.empty(Mt, 3, dtype=torch.int32, device=dev)
        args.op_ptr, args.map_ptr, args.n_ops_total, args.n_map_total = op_ptr_d.data_ptr(), map_ptr_d.data_ptr(), G, Mt
        args.rotations, args.translations = _lib.ptr(rotations) if G else None, _lib.ptr(translations) if G else None
        args.atom_map, args.shifts, args.orbits = _lib.ptr(atom_map) if Mt else None, _lib.ptr(shifts) if Mt else None, orbits.data_ptr()
        _lib.check(lib.alignn_sym_fill(C.byref(args), _lib.stream()), "sym_fill")
    res = SymmetryResult(
        rotations=[rotations[op_ptr[b]:op_ptr[b + 1]] for b in range(B)],
        translations=[translations[op_ptr[b]:op_ptr[b + 1]] for b in range(B)],
        atom_map=[atom_map[map_ptr[b]:map_ptr[b + 1]].view(n_ops[b], ns[b]) for b in range(B)],
        shifts=[shifts[map_ptr[b]:map_ptr[b + 1]].view(n_ops[b], ns[b], 3) for b in range(B)],
        orbits=[orbits[ptr[b]:ptr[b + 1]] for b in range(B)], n_ops=n_ops, n_translations=[int(v) for v in got[:, 1]],
        point_group_order=[int(v) for v in got[:, 2]], crystal_system=[CRYSTAL_SYSTEMS[int(v)] for v in got[:, 3]], ns=ns,
        symprec=float(symprec),
        packed=dict(atom_ptr=atom_ptr, op_ptr=op_ptr_d, map_ptr=map_ptr_d, rotations=rotations, translations=translations,
                    atom_map=atom_map, shifts=shifts, n_ops_total=G, n_map_total=Mt, device=dev))
    bad = [(b, int(s)) for b, s in enumerate(got[:, 4]) if s]
    if bad:
        why = []
        for b, s in bad:
            if s & STATUS_IMAGES:
                why.append(f"structure {b}: the cell needs lattice vectors beyond +-{MAX_IMAGE_RANGE} along an axis (or is singular)")
            if s & STATUS_OVERFLOW:
                why.append(f"structure {b}: more than {MAX_CANDIDATES} candidate images of a lattice vector or {MAX_LATTICE_OPS} "
                           f"lattice operations: symprec = {symprec} is not small against the cell")
            if s & STATUS_INPUT:
                why.append(f"structure {b}: its rows do not fit the arrays")
        err = ValueError(f"{who}: " + "; ".join(why) + " (the other structures' results: this error's .result)")
        err.result = res
        raise err
    return res


def _apply(who: str, entry: str, sym: SymmetryResult, lattices, values, per_atom: bool):
    if not isinstance(sym, SymmetryResult) or not sym.packed:
        raise TypeError(f"{who}: sym must be the SymmetryResult of find_symmetry")
    pk, B, N = sym.packed, len(sym.ns), sum(sym.ns)
    dev = pk["device"]
    as_list = not isinstance(values, torch.Tensor)
    if as_list:
        if len(values) != B:
            raise ValueError(f"{who}: need one array per structure ({B}), got {len(values)}")
        for b, v in enumerate(values):
            want = (sym.ns[b], 3) if per_atom else (3, 3)
            if shape_of(v) != want:
                raise ValueError(f"{who}: entry {b} is {shape_of(v)}, need {list(want)}")
        parts = [torch.as_tensor(host(v) if not isinstance(v, torch.Tensor) else v).to(dev, torch.float64) for v in values]
        x = torch.cat(parts) if per_atom else torch.stack(parts)
    else:
        x = values.to(dev, torch.float64)
    want = (N, 3) if per_atom else (B, 3, 3)
    if tuple(x.shape) != want:
        raise ValueError(f"{who}: need {list(want)} values, got {tuple(x.shape)}")
    x = x.contiguous()
    lib = _load()
    with _lib.device_guard(x):
        lat = _stack_lattices(who, lattices, B, dev)
        out = torch.empty_like(x)
        args = ApplyArgs(lattice=lat.data_ptr(), in_=x.data_ptr(), out=out.data_ptr(), atom_ptr=pk["atom_ptr"].data_ptr(), op_ptr=pk["op_ptr"].data_ptr(),
                         map_ptr=pk["map_ptr"].data_ptr(), rotations=_lib.ptr(pk["rotations"]) if pk["n_ops_total"] else None,
                         translations=_lib.ptr(pk["translations"]) if pk["n_ops_total"] else None,
                         atom_map=_lib.ptr(pk["atom_map"]) if pk["n_map_total"] else None,
                         shifts=_lib.ptr(pk["shifts"]) if pk["n_map_total"] else None, n_ops_total=pk["n_ops_total"],
                         n_map_total=pk["n_map_total"], n_structs=B, n_atoms=N)
        _lib.check(getattr(lib, entry)(C.byref(args), _lib.stream()), entry[len("alignn_"):])
    if as_list:
        ptr = np.concatenate([[0], np.cumsum(sym.ns)])
        return [out[ptr[b]:ptr[b + 1]] for b in range(B)] if per_atom else [out[b] for b in range(B)]
    return out


def symmetrize_forces(sym: SymmetryResult, lattices, forces):
    """``F'_i = (1/G) sum_g Q_g^T F_map[g][i]``, Q_g = A^T W_g A^-T the Cartesian rotation in the cell ``lattices[b]``: the
    projection of the forces onto those the symmetry allows.  ``forces``: a packed [sum n, 3] tensor or B arrays [n, 3]; the
    result has the same form, float64 on the GPU.  One launch."""
    return _apply("symmetrize_forces", "alignn_sym_forces", sym, lattices, forces, True)


def symmetrize_stress(sym: SymmetryResult, lattices, stress):
    """``s' = (1/G) sum_g Q_g^T s Q_g`` for a [B, 3, 3] tensor (or B arrays [3, 3]).  One launch."""
    return _apply("symmetrize_stress", "alignn_sym_stress", sym, lattices, stress, False)


def symmetrize_positions(sym: SymmetryResult, lattices, positions):
    """In fractional coordinates ``x'_i = (1/G) sum_g W_g^-1 (x_map[g][i] + shift[g][i] - t_g)``, returned Cartesian in the
    cell ``lattices[b]``: every atom moves to the mean of where the operations say it is (by less than symprec for the
    structure that was searched).  ``positions`` as ``forces`` above.  One launch."""
    return _apply("symmetrize_positions", "alignn_sym_positions", sym, lattices, positions, True)


def _orbits_of_indices(rotations: np.ndarray, max_index: int, merge_opposite: bool) -> List[Tuple[int, int, int]]:
    Ws = np.unique(rotations.reshape(-1, 9), axis=0).reshape(-1, 3, 3).astype(np.int64)
    r = range(-max_index, max_index + 1)
    todo = {h for h in itertools.product(r, r, r) if any(h) and gcd(gcd(abs(h[0]), abs(h[1])), abs(h[2])) == 1}
    reps = []
    while todo:
        orbit, new = set(), {next(iter(todo))}
        while new:  # (the rotations found within a tolerance need not close: grow the class until nothing is added)
            orbit |= new
            grown = {tuple(int(v) for v in row) for row in (np.array(sorted(new), dtype=np.int64) @ Ws).reshape(-1, 3)}
            if merge_opposite:
                grown |= {(-h[0], -h[1], -h[2]) for h in grown | new}
            new = grown - orbit
        reps.append(max(orbit))
        todo -= orbit
    return sorted(reps, key=lambda h: (h[0] * h[0] + h[1] * h[1] + h[2] * h[2], (-h[0], -h[1], -h[2])))


def distinct_miller_indices(sym: SymmetryResult, max_index: int, merge_opposite: bool = True) -> List[List[Tuple[int, int, int]]]:
    """Per structure the symmetry-distinct Miller indices (h, k, l) != 0 with every |.| <= ``max_index`` and gcd 1: the classes
    under hkl -> hkl W (a row vector times W) over the structure's distinct rotations, merged with their negatives when
    ``merge_opposite`` (a slab has both faces).  A class is represented by its lexicographically largest member; the classes
    are ordered by h^2 + k^2 + l^2, then descending lexicographically.  The indices refer to the cell as given, as those of
    ``surface_energy(miller_indices=...)`` do.  Host logic: the rotations are copied from the device."""
    who = "distinct_miller_indices"
    if not isinstance(max_index, numbers.Integral) or isinstance(max_index, (bool, np.bool_)) or max_index < 1:
        raise ValueError(f"{who}: max_index must be an int >= 1, got {max_index!r}")
    if not isinstance(merge_opposite, (bool, np.bool_)):
        raise ValueError(f"{who}: merge_opposite is one bool, got {type(merge_opposite).__name__}")
    out = []
    for b, W in enumerate(sym.rotations):
        W = host(W).reshape(-1, 3, 3)
        if len(W) == 0:
            raise ValueError(f"{who}: structure {b} has no operations")
        out.append(_orbits_of_indices(W, int(max_index), bool(merge_opposite)))
    return out
