"""What the trajectory analyses (``alignn_amd.trajectory``, ``order``, ``local_order``) share on the host: the conventions of their
inputs and the checks of them, in one place.

* frames: ``start`` / ``stop`` / ``step`` select as a slice selects (``_frames``);
* the trajectory: one float64 tensor [n_frames, sum n_i, 3] on the GPU for the B structures of ``ns`` (``_traj``), the cells
  [B, 3, 3] or one set per frame [F, B, 3, 3] (``_cells``);
* groups: 0 every atom, 1 .. S the species of a structure in ascending atomic number (``_groups``);
* the options more than one function takes: a positive number, the cutoffs, the bins, the degrees l, the masses;
* ``inputs``: the prologue of every function that reads cells - these checks in one order - and ``Inputs``, the record it
  returns, which fills the fields the argument blocks of the three headers have in common (``Inputs.fields``);
* ``_raise_status``: the status bits of include/alignn_order.h, which alignn_local.h repeats by value.

Nothing here touches the device but ``_groups``, ``_cutoffs`` and ``_masses``, which put their results there.
"""

from __future__ import annotations

import numbers
from dataclasses import dataclass
from typing import List, Optional, Tuple

import numpy as np
import torch

from . import _abi
from ._structures import host

MAX_SPECIES = _abi.header("alignn_traj.h").defines["ALIGNN_TRAJ_MAX_SPECIES"]
_ORDER = _abi.header("alignn_order.h").defines
MAX_ATOMS = 65535  # per structure, where a launch takes a workgroup or a wavefront per atom


def _frames(who: str, F: int, start, stop, step) -> Tuple[int, int, int]:
    """The slice ``start:stop:step`` of F frames -> (first frame, step, frames used)."""
    for name, v in (("start", start), ("stop", stop), ("step", step)):
        if v is not None and (not isinstance(v, numbers.Integral) or isinstance(v, (bool, np.bool_))):
            raise ValueError(f"{who}: {name} must be an int or None, got {v!r}")
    if step is not None and step < 1:
        raise ValueError(f"{who}: step must be >= 1, got {step}")
    r = range(F)[slice(start, stop, step)]
    return (r.start if len(r) else 0), r.step, len(r)


def _traj(who: str, name: str, traj, ns) -> Tuple[torch.Tensor, List[int]]:
    ns = [int(n) for n in ns]
    if not ns or min(ns) < 1:
        raise ValueError(f"{who}: ns needs the atom count (>= 1) of at least one structure, got {ns}")
    if len(ns) > 65535:
        raise ValueError(f"{who}: {len(ns)} structures; a call takes at most 65535")
    if not isinstance(traj, torch.Tensor) or traj.dtype != torch.float64 or not traj.is_cuda:
        raise TypeError(f"{who}: {name} must be a float64 tensor on the GPU (what run_md records)")
    if traj.ndim != 3 or tuple(traj.shape[1:]) != (sum(ns), 3):
        raise ValueError(f"{who}: {name} must be [n_frames, {sum(ns)}, 3], got {tuple(traj.shape)}")
    if traj.shape[0] >= 2 ** 31 or traj.shape[1] >= 2 ** 31 // 3:
        raise ValueError(f"{who}: {name} has {traj.shape[0]} frames of {traj.shape[1]} rows; a call takes fewer than 2^31 of each")
    return traj.contiguous(), ns


def _groups(who: str, ns: List[int], species, dev):
    """-> (atom_ptr [B + 1], group [N] 1-based rank of the row's species in its structure, group_count [B, S + 1], S, the
    species lists)."""
    B = len(ns)
    if species is None:
        ranks, lists = [np.ones(n, dtype=np.int32) for n in ns], [[0]] * B
    else:
        if len(species) != B:
            raise ValueError(f"{who}: species needs one array of atomic numbers per structure ({B}) or None, got {len(species)}")
        ranks, lists = [], []
        for b, z in enumerate(species):
            z = host(z)
            if z.shape != (ns[b],) or z.dtype.kind not in "iu":
                raise ValueError(f"{who}: species[{b}] is {z.dtype} {z.shape}, need integers [{ns[b]}]")
            uniq, inverse = np.unique(z, return_inverse=True)
            if len(uniq) > MAX_SPECIES:
                raise ValueError(f"{who}: structure {b} has {len(uniq)} species; at most {MAX_SPECIES} are supported")
            ranks.append((inverse.reshape(-1) + 1).astype(np.int32))
            lists.append([int(u) for u in uniq])
    S = max(len(l) for l in lists)
    count = np.zeros((B, S + 1), dtype=np.int32)
    for b in range(B):
        count[b, 0] = ns[b]
        count[b, 1:1 + len(lists[b])] = np.bincount(ranks[b], minlength=len(lists[b]) + 1)[1:]
    ptr = np.concatenate([[0], np.cumsum(ns)]).astype(np.int32)
    dev_i32 = lambda x: torch.tensor(np.ascontiguousarray(x), dtype=torch.int32, device=dev)
    return dev_i32(ptr), dev_i32(np.concatenate(ranks)), dev_i32(count), S, [list(l) for l in lists]


def _masses(who: str, masses, ns, dev) -> torch.Tensor:
    if len(masses) != len(ns):
        raise ValueError(f"{who}: masses needs one array per structure ({len(ns)}), got {len(masses)}")
    for b, x in enumerate(masses):
        if host(x).shape != (ns[b],):
            raise ValueError(f"{who}: masses[{b}] is {host(x).shape}, need [{ns[b]}]")
    m = torch.cat([torch.as_tensor(host(x)).to(torch.float64) for x in masses])
    if not bool(torch.isfinite(m).all() and (m > 0).all()):
        raise ValueError(f"{who}: masses must be finite and > 0")
    return m.to(dev)


def _positive(who: str, name: str, v) -> float:
    if not isinstance(v, numbers.Real) or isinstance(v, (bool, np.bool_)) or not np.isfinite(v) or v <= 0:
        raise ValueError(f"{who}: {name} must be a finite number > 0, got {v!r}")
    return float(v)


def bins(who: str, n_bins, max_bins: int, bool_ok: bool = False):
    """``n_bins`` in 1 .. ``max_bins``, as an int.  ``bool_ok``: what ``rdf`` has always let through - a bool is an Integral - and
    hands on as it came."""
    if not isinstance(n_bins, numbers.Integral) or not 1 <= n_bins <= max_bins or (
            not bool_ok and isinstance(n_bins, (bool, np.bool_))):
        raise ValueError(f"{who}: n_bins must be 1 .. {max_bins}, got {n_bins!r}")
    return n_bins if bool_ok else int(n_bins)


def degrees(who: str, ls, max_ls: int, max_l: int) -> Tuple[int, ...]:
    ok = isinstance(ls, (tuple, list)) and 1 <= len(ls) <= max_ls and all(
        isinstance(l, numbers.Integral) and not isinstance(l, (bool, np.bool_)) and 1 <= l <= max_l for l in ls)
    if not ok or len(set(int(l) for l in ls)) != len(ls):
        raise ValueError(f"{who}: ls must be 1 to {max_ls} distinct integers in 1 .. {max_l}, got {ls!r}")
    return tuple(int(l) for l in ls)


def _cutoffs(who: str, r_cut, B: int, dev) -> torch.Tensor:
    """One number, B numbers, or a float64 tensor [B] on the device -> [B] on the device."""
    if isinstance(r_cut, torch.Tensor):
        if r_cut.dtype != torch.float64 or r_cut.device != dev or tuple(r_cut.shape) != (B,):
            raise ValueError(f"{who}: r_cut as a tensor must be float64 [{B}] on the trajectory's device, got {r_cut.dtype} "
                             f"{tuple(r_cut.shape)} on {r_cut.device}")
        return r_cut.contiguous()
    if isinstance(r_cut, (list, tuple, np.ndarray)):
        if len(r_cut) != B:
            raise ValueError(f"{who}: r_cut needs one number or one per structure ({B}), got {len(r_cut)}")
        values = [_positive(who, f"r_cut[{b}]", v) for b, v in enumerate(r_cut)]
    else:
        values = [_positive(who, "r_cut", r_cut)] * B
    return torch.tensor(values, dtype=torch.float64, device=dev)


def _cells(who: str, lattices, traj, shapes) -> torch.Tensor:
    if not isinstance(lattices, torch.Tensor) or lattices.dtype != torch.float64 or lattices.device != traj.device:
        raise TypeError(f"{who}: lattices must be a float64 tensor on the trajectory's device")
    if tuple(lattices.shape) not in shapes:
        raise ValueError(f"{who}: lattices must be " + " or ".join(str(list(s)) for s in shapes) + f", got {tuple(lattices.shape)}")
    return lattices.contiguous()


def _raise_status(who: str, word: int):
    if word & _ORDER["ALIGNN_ORDER_STATUS_IMAGES"]:
        raise ValueError(f"{who}: r_cut needs periodic images beyond +-{_ORDER['ALIGNN_ORDER_MAX_IMAGE_RANGE']} cells along an axis of "
                         "some frame's cell (or a cell is singular, or an r_cut is not a finite number > 0): lower r_cut or analyse a "
                         "supercell")
    if word & _ORDER["ALIGNN_ORDER_STATUS_NEIGHBORS"]:
        raise ValueError(f"{who}: an atom has more than {_ORDER['ALIGNN_ORDER_MAX_NEIGHBORS']} neighbours inside r_cut: lower r_cut (it "
                         "is meant to end between the first and the second shell)")


@dataclass
class Inputs:
    """The checked inputs of one call: ``traj`` and ``lattices`` contiguous, ``ns`` a list, the frames used ``frame0``,
    ``frame0 + frame_step``, ... (``n_frames`` of them); after ``groups`` also what ``_groups`` returns."""

    who: str
    traj: torch.Tensor
    ns: List[int]
    lattices: torch.Tensor
    frame0: int
    frame_step: int
    n_frames: int
    atom_ptr: Optional[torch.Tensor] = None
    group: Optional[torch.Tensor] = None
    group_count: Optional[torch.Tensor] = None
    n_species: int = 0
    species: Optional[List[List[int]]] = None

    def groups(self, species) -> Tuple[int, List[List[int]]]:
        """``_groups`` on the trajectory's device (call it under the device guard) -> (S, the species lists)."""
        self.atom_ptr, self.group, self.group_count, self.n_species, self.species = _groups(self.who, self.ns, species, self.traj.device)
        return self.n_species, self.species

    def fields(self, Args, status: torch.Tensor) -> dict:
        """The fields the argument blocks share, those of them that the block ``Args`` declares."""
        shared = dict(traj=self.traj.data_ptr(), lattice=self.lattices.data_ptr(), atom_ptr=self.atom_ptr.data_ptr(),
                      group=self.group.data_ptr(), group_count=self.group_count.data_ptr(), status=status.data_ptr(),
                      n_structs=len(self.ns), n_atoms=sum(self.ns), max_atoms=max(self.ns), n_species=self.n_species,
                      n_total_frames=self.traj.shape[0], frame0=self.frame0, frame_step=self.frame_step, n_frames=self.n_frames,
                      lattice_per_frame=int(self.lattices.ndim == 4))
        declared = {f[0] for f in Args._fields_}
        return {k: v for k, v in shared.items() if k in declared}


def inputs(who: str, traj, lattices, ns, start, stop, step, *, per_frame: bool = True, atom_limit: bool = True) -> Inputs:
    """The prologue of ``rdf``, ``adf`` / ``steinhardt``, ``structure_factor``, ``cna`` and ``bond_order``: the trajectory, the
    atoms per structure (``atom_limit``), the cells (``per_frame``: [F, B, 3, 3] is taken too) and the frame selection."""
    traj, ns = _traj(who, "traj", traj, ns)
    B, F = len(ns), traj.shape[0]
    if atom_limit and max(ns) > MAX_ATOMS:
        raise ValueError(f"{who}: a structure of {max(ns)} atoms; a call takes at most {MAX_ATOMS} per structure")
    if not per_frame and isinstance(lattices, torch.Tensor) and lattices.ndim == 4:
        raise ValueError(f"{who}: a per-frame lattice {tuple(lattices.shape)} is not supported: S(q) is taken on the reciprocal "
                         f"lattice of one fixed cell per structure, [{B}, 3, 3]")
    lattices = _cells(who, lattices, traj, ((B, 3, 3), (F, B, 3, 3)) if per_frame else ((B, 3, 3),))
    return Inputs(who, traj, ns, lattices, *_frames(who, F, start, stop, step))
