"""Batched primitive and conventional cells on the device: from the operations ``find_symmetry`` finds for B crystals, the reduced
primitive cell or the conventional cell of each, with its atoms.

The reference takes its conventional cells from spglib through jarvis' ``Spacegroup3D(atoms).conventional_standard_structure``,
one structure at a time on the host (``vacancy_formation(on_conventional_cell=True)``, ``surface_energy(on_conventional_cell=
True)``, ``get_interface_energy(from_conventional_structure=True)``, ``ase_phonon(use_cvn=True)``).  Here:

* ``primitive_cell``: the lattice of the pure translations in Hermite normal form, reduced to its successive minima, with one
  atom per orbit of the pure translations;
* ``conventional_cell``: the cell along the axes of the crystal's own rotations (not the lattice's holohedry), per crystal
  system, with its multiplicity and centring letter and the primitive atoms repeated at the lattice points inside it.

The new cell's rows are integer combinations of the given ones over ``n_translations``, exactly: nothing is idealised, a strained
cubic cell keeps its 89.99 degrees.  The definitions, with every tie rule, are stated in include/alignn_cells.h (read here with the
reader of alignn_amd/_abi.py) and restated in numpy by tests/cells_ref.py.  The kernels (csrc/cells.hip) do the lattice geometry in
int64; float64 without contraction enters where two lengths are compared - a vector is preferred to another only when it is
shorter by more than ``symprec`` - and no floating-point atomics are used: a structure's results are the same bits alone, in a
batch and at any place of it.  One array of B x 8 integers (atom counts, multiplicity, centring, status) is read back between the
launch that finds the cells and the one that writes the atoms; nothing else.

A supercell (``n_translations`` > 1) has, among the operations ``find_symmetry`` reports, only the rotations that keep the cell as
given.  ``conventional_cell`` therefore takes such a structure to its reduced primitive cell first, searches the symmetry of that
cell - every rotation of the crystal keeps it - and finds the conventional cell from there: for these structures the two launches
and the search run a second time, and the transformations and source atoms of the two rounds are composed.  Which way a structure
goes depends on that structure alone.

Not here: space-group numbers and symbols, Wyckoff letters, origin shifts and spglib's setting conventions (a monoclinic cell may
come out A-, C- or I-centred; orthorhombic axes are ordered by length), idealised lattices or positions.
"""

from __future__ import annotations

import ctypes as C
import numbers
from dataclasses import dataclass, field
from typing import List, Optional, Sequence

import numpy as np
import torch

from . import _abi, _lib
from ._structures import host, shape_of
from .symmetry import CRYSTAL_SYSTEMS, SymmetryResult, _stack_lattices, find_symmetry

__all__ = ["primitive_cell", "conventional_cell", "CellResult", "CENTRINGS"]

H = _abi.header("alignn_cells.h")
HEADER, STRUCTS, SIGNATURES = H.path, H.structs, H.signatures
CellsArgs = STRUCTS["alignn_cells_args"]
MAX_ATOMS = H.defines["ALIGNN_CELLS_MAX_ATOMS"]
MAX_IMAGE_RANGE = H.defines["ALIGNN_CELLS_MAX_IMAGE_RANGE"]
INFO = H.defines["ALIGNN_CELLS_INFO"]
STATUS_SYMMETRY = H.defines["ALIGNN_CELLS_STATUS_SYMMETRY"]
STATUS_TRANSLATIONS = H.defines["ALIGNN_CELLS_STATUS_TRANSLATIONS"]
STATUS_RANGE = H.defines["ALIGNN_CELLS_STATUS_RANGE"]
STATUS_REDUCE = H.defines["ALIGNN_CELLS_STATUS_REDUCE"]
STATUS_ATOMS = H.defines["ALIGNN_CELLS_STATUS_ATOMS"]
CENTRINGS = "PIFABCR"


def _load():
    return _lib.bind(H)


@dataclass
class CellResult:
    """Per structure b (lists of B entries; the tensors are views of packed device arrays):

    ``lattices`` [B, 3, 3]: the new cells, rows are lattice vectors.  ``positions[b]`` [m_b, 3]: Cartesian, the fractional
    coordinates wrapped into [0, 1).  ``source_atom[b]`` [m_b] int32: the input atom each output atom is a copy of (species and
    ``atom_features`` rows are taken through it).  ``transform_num[b]`` [3, 3] int64 and ``transform_den[b]``: the new cell's rows
    are ``transform_num / transform_den`` times the input cell's rows, exactly (``transform_den`` = ``n_translations``, not
    reduced).  ``multiplicity[b]``: lattice points per cell, 1 for a primitive cell; ``centring[b]``: one of ``P I F A B C R``;
    ``crystal_system[b]``: one of ``CRYSTAL_SYSTEMS``; ``n_translations[b]`` of the input; ``ns``: the output atom counts.  A
    structure that raised has zeros and no atoms."""

    lattices: torch.Tensor
    positions: List[torch.Tensor]
    source_atom: List[torch.Tensor]
    transform_num: List[torch.Tensor]
    transform_den: List[int]
    multiplicity: List[int]
    centring: List[str]
    crystal_system: List[str]
    n_translations: List[int]
    ns: List[int]
    symprec: float
    packed: dict = field(default_factory=dict, repr=False)


def _check(who: str, lattices, positions, species, symprec, sym) -> List[int]:
    """The checks that need no device: -> the atom counts."""
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
    if not isinstance(lattices, torch.Tensor):
        for i, lat in enumerate(lattices):
            if shape_of(lat) != (3, 3):
                raise ValueError(f"{who}: lattices[{i}] is {shape_of(lat)}, need [3, 3]")
    if species is not None:
        if len(species) != B:
            raise ValueError(f"{who}: species needs one integer array per structure ({B}) or None, got {len(species)}")
        for i, z in enumerate(species):
            if shape_of(z) != (ns[i],):
                raise ValueError(f"{who}: species[{i}] is {shape_of(z)}, need [{ns[i]}]")
    if not isinstance(symprec, numbers.Real) or isinstance(symprec, (bool, np.bool_)) or not np.isfinite(symprec) or symprec <= 0:
        raise ValueError(f"{who}: symprec must be a finite length > 0, got {symprec!r}")
    if sym is not None:
        if not isinstance(sym, SymmetryResult) or not sym.packed:
            raise ValueError(f"{who}: sym must be the SymmetryResult of find_symmetry for these structures")
        if list(sym.ns) != ns:
            raise ValueError(f"{who}: sym was found for structures of {list(sym.ns)} atoms, these have {ns}")
    return ns


def _pass(conventional: bool, lat: torch.Tensor, positions, ns: List[int], sym: SymmetryResult, symprec: float) -> dict:
    """The two launches over the structures of ``sym``, with the read-back of ``info`` in between."""
    pk = sym.packed
    dev, B, N = pk["device"], len(ns), sum(ns)
    lib = _load()
    pos = torch.cat([torch.as_tensor(p).to(dev, torch.float64) for p in positions]).contiguous()
    info = torch.zeros(B, INFO, dtype=torch.int32, device=dev)
    num = torch.zeros(B, 3, 3, dtype=torch.int64, device=dev)
    den = torch.zeros(B, dtype=torch.int64, device=dev)
    cells = torch.zeros(B, 3, 3, dtype=torch.float64, device=dev)
    points = torch.zeros(B, 4, 3, dtype=torch.int64, device=dev)
    reps = torch.zeros(N, dtype=torch.int32, device=dev)
    G, Mt = pk["n_ops_total"], pk["n_map_total"]
    args = CellsArgs(lattice=lat.data_ptr(), pos=pos.data_ptr(), atom_ptr=pk["atom_ptr"].data_ptr(), op_ptr=pk["op_ptr"].data_ptr(),
                     map_ptr=pk["map_ptr"].data_ptr(), rotations=_lib.ptr(pk["rotations"]) if G else None,
                     translations=_lib.ptr(pk["translations"]) if G else None, atom_map=_lib.ptr(pk["atom_map"]) if Mt else None,
                     info=info.data_ptr(), transform_num=num.data_ptr(), transform_den=den.data_ptr(), cells=cells.data_ptr(),
                     points=points.data_ptr(), reps=reps.data_ptr(), symprec=float(symprec), n_ops_total=G, n_map_total=Mt,
                     n_structs=B, n_atoms=N, conventional=1 if conventional else 0)
    _lib.check(lib.alignn_cells_reduce(C.byref(args), _lib.stream()), "cells_reduce")
    got = info.cpu().numpy()  # the one read-back: output atom counts, multiplicity, centring, system and status
    n_out = [int(v) for v in got[:, 0]]
    out_ptr = np.concatenate([[0], np.cumsum(n_out)]).astype(np.int64)
    total = int(out_ptr[-1])
    out_ptr_d = torch.tensor(out_ptr, dtype=torch.int64, device=dev)
    out_pos = torch.empty(total, 3, dtype=torch.float64, device=dev)
    source = torch.empty(total, dtype=torch.int32, device=dev)
    args.out_ptr, args.n_out_total, args.max_out = out_ptr_d.data_ptr(), total, max(n_out)
    args.out_pos, args.source_atom = _lib.ptr(out_pos) if total else None, _lib.ptr(source) if total else None
    _lib.check(lib.alignn_cells_fill(C.byref(args), _lib.stream()), "cells_fill")
    return dict(info=got, n_out=n_out, out_ptr=out_ptr, num=num, cells=cells, pos=out_pos, source=source)


def _find(lattices, positions, species, symprec, device):
    """``find_symmetry``; a structure without operations does not stop the others -> (sym, its message or None)."""
    try:
        return find_symmetry(lattices, positions, species, symprec=symprec, device=device), None
    except ValueError as e:
        if not isinstance(getattr(e, "result", None), SymmetryResult):
            raise
        return e.result, str(e)


def _cells(who: str, conventional: bool, lattices, positions, species, symprec, sym, device) -> CellResult:
    ns = _check(who, lattices, positions, species, symprec, sym)
    B = len(ns)
    sym_error = None
    if sym is None:
        sym, sym_error = _find(lattices, positions, species, symprec, device)
    dev = sym.packed["device"]
    if device is not None and torch.device(device).index not in (None, dev.index):
        raise ValueError(f"{who}: sym lives on {dev}, device is {device}")
    with _lib.device_guard(torch.empty(0, device=dev)):
        lat = _stack_lattices(who, lattices, B, dev)
        one = _pass(conventional, lat, positions, ns, sym, symprec)
        status = [int(v) for v in one["info"][:, 4]]
        info, cells, num = one["info"].copy(), one["cells"], one["num"]
        pos_of = [one["pos"][one["out_ptr"][b]:one["out_ptr"][b + 1]] for b in range(B)]
        src_of = [one["source"][one["out_ptr"][b]:one["out_ptr"][b + 1]] for b in range(B)]
        # supercells: what came back is the reduced primitive cell; its own operations give the conventional cell
        again = [b for b in range(B) if one["info"][b, 7] and not status[b]]
        if again:
            idx = torch.tensor(again, dtype=torch.int64, device=dev)
            z2 = None
            if species is not None:
                z2 = [torch.as_tensor(host(species[b])).to(dev)[src_of[b].long()] for b in again]
            sym2, err2 = _find(cells[idx], [pos_of[b] for b in again], z2, symprec, dev)
            sym_error = sym_error or err2
            two = _pass(True, cells[idx].contiguous(), [pos_of[b] for b in again], [len(pos_of[b]) for b in again], sym2, symprec)
            cells, num = cells.clone(), num.clone()
            cells[idx] = two["cells"]
            num[idx] = (two["num"][:, :, :, None] * num[idx][:, None, :, :]).sum(2)  # the product of the two transformations
            for k, b in enumerate(again):
                lo, hi = two["out_ptr"][k], two["out_ptr"][k + 1]
                status[b] = int(two["info"][k, 4]) | (STATUS_TRANSLATIONS if two["info"][k, 7] else 0)
                src_of[b], pos_of[b] = src_of[b][two["source"][lo:hi].long()], two["pos"][lo:hi]
                info[b, :4] = two["info"][k, :4] if not status[b] else 0
            out_pos, source = torch.cat(pos_of), torch.cat(src_of)  # (one packed array again)
            ptr = np.concatenate([[0], np.cumsum([len(p) for p in pos_of])])
            pos_of, src_of = [out_pos[ptr[b]:ptr[b + 1]] for b in range(B)], [source[ptr[b]:ptr[b + 1]] for b in range(B)]
        else:
            out_pos, source = one["pos"], one["source"]
    for b in range(B):
        if status[b]:
            info[b, :4], info[b, 5] = 0, 0
    res = CellResult(
        lattices=cells, positions=pos_of, source_atom=src_of, transform_num=[num[b] for b in range(B)],
        transform_den=[int(v) for v in info[:, 5]], multiplicity=[int(v) for v in info[:, 1]],
        centring=[CENTRINGS[int(v)] for v in info[:, 2]], crystal_system=[CRYSTAL_SYSTEMS[int(v)] for v in info[:, 3]],
        n_translations=[int(v) for v in info[:, 5]], ns=[len(p) for p in pos_of], symprec=float(symprec),
        packed=dict(positions=out_pos, source_atom=source, transform_num=num, device=dev))
    bad = [(b, s) for b, s in enumerate(status) if s]
    if bad:
        why = []
        for b, s in bad:
            if s & STATUS_SYMMETRY:
                why.append(f"structure {b}: no symmetry operations to work from" + (f" ({sym_error})" if sym_error else
                           " (sym does not describe it)"))
            if s & STATUS_TRANSLATIONS:
                why.append(f"structure {b}: its pure translations form no lattice within symprec = {symprec}")
            if s & STATUS_RANGE:
                why.append(f"structure {b}: the cell needs lattice vectors beyond +-{MAX_IMAGE_RANGE} along an axis (or is singular)")
            if s & STATUS_REDUCE:
                why.append(f"structure {b}: its operations give no cell: symprec = {symprec} is not small against the cell")
            if s & STATUS_ATOMS:
                why.append(f"structure {b}: the new cell has more than {MAX_ATOMS} atoms")
        err = ValueError(f"{who}: " + "; ".join(why) + " (the other structures' results: this error's .result)")
        err.result = res
        raise err
    return res


def primitive_cell(lattices: Sequence, positions: Sequence, species: Optional[Sequence] = None, *, symprec: float = 1e-3,
                   sym: Optional[SymmetryResult] = None, device=None) -> CellResult:
    """The reduced primitive cells of B crystals: the lattice of the pure translations, its basis the successive minima (the
    shortest vector, the shortest not collinear with it, the shortest that completes a basis), with the handedness of the input;
    one atom per orbit of the pure translations, the lowest input index of the orbit.

    ``lattices``, ``positions``, ``species``, ``symprec``, ``device``: as ``find_symmetry``; ``sym``: the ``SymmetryResult`` of
    these structures, searched here when None.  ``find_symmetry``'s limits hold.  A structure the method cannot handle (no
    operations, a cell that needs lattice vectors beyond +-8 of a basis, more than 1024 output atoms) raises ``ValueError``
    naming it and the reason; the error carries the results of the other structures as its ``result`` attribute."""
    return _cells("primitive_cell", False, lattices, positions, species, symprec, sym, device)


def conventional_cell(lattices: Sequence, positions: Sequence, species: Optional[Sequence] = None, *, symprec: float = 1e-3,
                      sym: Optional[SymmetryResult] = None, device=None) -> CellResult:
    """The conventional cells of B crystals, from the axes of each crystal's own rotations: cubic along the fourfold (or the
    three twofold) axes; tetragonal, trigonal and hexagonal with c the main axis and a the shortest lattice vector perpendicular
    to it (gamma = 120 degrees, rhombohedral lattices in the obverse setting); orthorhombic along the twofold axes with
    |a| <= |b| <= |c|; monoclinic with b the twofold axis, |a| <= |c| and beta >= 90 degrees; triclinic the reduced primitive
    cell.  The atoms are the primitive atoms repeated at the lattice points inside the cell, ordered by source atom.

    Arguments, limits and errors: as ``primitive_cell``."""
    return _cells("conventional_cell", True, lattices, positions, species, symprec, sym, device)
