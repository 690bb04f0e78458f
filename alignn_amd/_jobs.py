"""What the derived-structure drivers (``vacancy_formation``, ``surface_energy``, ``ev_curve``, ``elastic_tensor``,
``interface_energy``) share: the checks of their options, the parent preparation and the builders more than one of them uses,
and the job runner.

A job is one structure derived from the caller's parents on the device - a supercell, a slab, a strained copy, a stacked
interface - given as its cell, its rows of one Cartesian array and ``src``, the parent atom of every row (one gather gives
the atom features).  A driver builds its jobs, hands them to ``relax`` in groups of whole jobs of at most
``max_atoms_per_call`` atoms (``relax`` keeps a structure's bits independent of its batch, so the grouping does not show in the
numbers) and reduces the results.
"""

from __future__ import annotations

import numbers
from dataclasses import dataclass
from typing import List, Optional, Sequence

import numpy as np
import torch

from . import _lib
from ._structures import Packed, host, pack
from .relax import relax

MAX_ATOMS_PER_CALL = 32768
RELAX_DEFAULTS = dict(steps=100, fmax=0.1, optimize_lattice=True)  # the reference's ``optimize_atoms()``
EVALUATION = ("cutoff", "max_neighbors", "neighbor_strategy", "intensive", "force_multiplier")
_PER_STRUCTURE = ("fixed",)  # relax options given per structure: the jobs are not the caller's structures


# --- checks (host) -----------------------------------------------------------------------------------------------------------------
def positive(who, name, v, zero_ok=False) -> float:
    if not (isinstance(v, numbers.Real) and np.isfinite(v) and (v >= 0 if zero_ok else v > 0)):
        raise ValueError(f"{who}: {name} must be a finite number {'>= 0' if zero_ok else '> 0'}, got {v!r}")
    return float(v)


def check_max_atoms(who: str, max_atoms_per_call):
    if not (isinstance(max_atoms_per_call, numbers.Integral) and max_atoms_per_call >= 1):
        raise ValueError(f"{who}: max_atoms_per_call must be an int >= 1")


def check_steps_fmax(who: str, relax_kwargs: dict):
    for name in ("steps", "fmax"):
        if name in relax_kwargs and not (isinstance(relax_kwargs[name], numbers.Real) and relax_kwargs[name] >= 0):
            raise ValueError(f"{who}: {name} must be a number >= 0")


def check_job_options(who: str, max_atoms_per_call, relax_kwargs: dict):
    """The checks of a driver whose ``relax_kwargs`` go to the jobs' ``relax`` calls as whole-call options."""
    check_max_atoms(who, max_atoms_per_call)
    for name in _PER_STRUCTURE:
        if relax_kwargs.get(name) is not None:
            raise ValueError(f"{who}: relax's {name}= is given per structure; the jobs here are derived structures")
    check_steps_fmax(who, relax_kwargs)
    if "cell_mask" in relax_kwargs and relax_kwargs["cell_mask"] is not None:
        if host(relax_kwargs["cell_mask"]).shape not in ((6,), (3, 3)):
            raise ValueError(f"{who}: cell_mask is one mask for every job (six Voigt flags or [3, 3])")
    if np.ndim(relax_kwargs.get("scalar_pressure", 0.0)) != 0:
        raise ValueError(f"{who}: scalar_pressure is one number for every job")


def evaluation_options(who: str, relax_kwargs: dict, evaluation: Sequence[str], on_relaxed_struct, ion_relaxation=()) -> dict:
    """The options of ``relax_kwargs`` that reach every evaluation of a strained parent.  Without ``on_relaxed_struct`` nothing
    else may be given, but for ``ion_relaxation``, the options of a driver that relaxes the ions of its jobs."""
    if not on_relaxed_struct:
        extra = sorted(k for k in relax_kwargs if k not in tuple(evaluation) + tuple(ion_relaxation))
        if extra:
            raise ValueError(f"{who}: {', '.join(extra)} are options of the relaxation; without on_relaxed_struct only the "
                             f"evaluation options {', '.join(evaluation)} are taken" +
                             (f" (and {', '.join(ion_relaxation)} of the ion relaxation)" if ion_relaxation else ""))
    return {k: v for k, v in relax_kwargs.items() if k in evaluation}


def slab_layers(who: str, what: str, where: str, lat: np.ndarray, basis: np.ndarray, hkl, thickness: float, n_atoms: int) -> int:
    """``max(1, int(thickness / h3))`` layers of the cell ``lat`` oriented by ``basis`` (``miller_basis`` of ``hkl``), h3 the
    spacing of its (hkl) planes.  ``what`` names the lattice and ``where`` the slab in the caller's messages."""
    C = basis.astype(np.float64) @ lat
    nu = np.cross(C[0], C[1])
    with np.errstate(all="ignore"):
        h3 = abs(np.dot(C[2], nu)) / np.sqrt(np.dot(nu, nu))
    if not (np.isfinite(h3) and h3 > 0):
        raise ValueError(f"{who}: {what} has no volume")
    if thickness / h3 * n_atoms > np.iinfo(np.int32).max:
        raise ValueError(f"{who}: thickness {thickness} gives too many layers of {hkl} for {where}")
    return max(1, int(thickness / h3))


def offsets(counts) -> np.ndarray:
    """The first row of every job, and the number of rows."""
    return np.concatenate([[0], np.cumsum(counts)])


def group_jobs(counts: Sequence[int], max_atoms_per_call: int) -> List[List[int]]:
    """The jobs in order, in groups of whole jobs of at most ``max_atoms_per_call`` atoms (a job larger than that is a group
    alone): a group is closed when the next job does not fit."""
    groups, cur, atoms = [], [], 0
    for j, n in enumerate(counts):
        if cur and atoms + n > max_atoms_per_call:
            groups.append(cur)
            cur, atoms = [], 0
        cur.append(j)
        atoms += n
    groups.append(cur)
    return groups


def split(x, job_ptr):
    return [x[job_ptr[s]:job_ptr[s + 1]] for s in range(len(job_ptr) - 1)]


# --- on the device -----------------------------------------------------------------------------------------------------------------
def features(atom_features, forces_fn, dev) -> Optional[torch.Tensor]:
    """The parents' atom features, one row per packed atom (``src`` indexes them); None with ``forces_fn``."""
    if forces_fn is not None or atom_features is None:
        return None
    return torch.cat([torch.as_tensor(f).to(dev, torch.float32) for f in atom_features])


def prepare_parents(model, lattices, positions, atom_features, ns, on_relaxed_struct, relax_kwargs, forces_fn, dev):
    """The parents a strain driver works on: as given, or with ``on_relaxed_struct`` after one ``relax`` call on them with
    ``relax_kwargs`` over ``RELAX_DEFAULTS`` -> (packed, their lattices [B, 3, 3] and [positions] as the result returns them)."""
    if on_relaxed_struct:
        kw = dict(RELAX_DEFAULTS, **relax_kwargs)
        res = relax(model, lattices, positions, atom_features, forces_fn=forces_fn, device=dev, **kw)
        lattices = res.lattices if res.lattices is not None else lattices
        positions = res.positions
    packed = pack(lattices, positions, ns, dev, frac=False)
    return packed, packed.lat.clone(), [p.clone() for p in packed.rows(packed.pos)]


def strain_jobs(packed: Packed, ns: List[int], F: torch.Tensor, dev):
    """``alignn_strain_build`` for the B packed parents under each of the deformation gradients ``F`` [P, 3, 3] (float64, on
    the device): job s P + p is parent s with cell and positions times F[p] -> (cells [B P, 3, 3], cart [rows, 3], volumes
    [B P], src [rows] int32, counts)."""
    B, P = len(ns), len(F)
    J = B * P
    counts = [n for n in ns for _ in range(P)]
    off = offsets(counts)
    jobs_d = torch.arange(B, dtype=torch.int32, device=dev).repeat_interleave(P)
    F = F.repeat(B, 1, 1).contiguous()
    off_d = torch.tensor(off, dtype=torch.int64, device=dev)
    cells = torch.empty(J, 3, 3, dtype=torch.float64, device=dev)
    cart = torch.empty(int(off[-1]), 3, dtype=torch.float64, device=dev)
    volumes = torch.empty(J, dtype=torch.float64, device=dev)
    _lib.check(_lib.load().alignn_strain_build(
        packed.pos.data_ptr(), packed.atom_ptr.data_ptr(), packed.lat.data_ptr(), B, jobs_d.data_ptr(), F.data_ptr(),
        off_d.data_ptr(), J, cells.data_ptr(), cart.data_ptr(), volumes.data_ptr(), _lib.stream()), "strain_build")
    # row j of a job is atom j of its parent
    src = torch.cat([torch.arange(packed.ptr[s], packed.ptr[s + 1], dtype=torch.int32, device=dev).repeat(P) for s in range(B)])
    return cells, cart, volumes, src, counts


def build_slabs(packed: Packed, slab_jobs: List[List[int]], slab_counts: List[int], vacuum: float, dev):
    """``alignn_slab_build`` for the jobs [parent, the nine of its ``miller_basis``, layers] with ``vacuum`` (A) above every
    slab -> (cells [S, 3, 3], cart [rows, 3], src [rows] int32, the jobs' row offsets [S + 1] int64 on the device)."""
    S, rows = len(slab_jobs), int(sum(slab_counts))
    jobs_d = torch.tensor(slab_jobs, dtype=torch.int32, device=dev)
    vac_d = torch.full((S,), float(vacuum), dtype=torch.float64, device=dev)
    off_d = torch.tensor(offsets(slab_counts), dtype=torch.int64, device=dev)
    cells = torch.empty(S, 3, 3, dtype=torch.float64, device=dev)
    cart = torch.empty(rows, 3, dtype=torch.float64, device=dev)
    frac = torch.empty(rows, 3, dtype=torch.float64, device=dev)
    src = torch.empty(rows, dtype=torch.int32, device=dev)
    _lib.check(_lib.load().alignn_slab_build(
        packed.pos.data_ptr(), packed.atom_ptr.data_ptr(), packed.lat.data_ptr(), len(packed.ptr) - 1, jobs_d.data_ptr(),
        vac_d.data_ptr(), off_d.data_ptr(), S, cells.data_ptr(), cart.data_ptr(), frac.data_ptr(), src.data_ptr(), _lib.stream()),
        "slab_build")
    return cells, cart, src, off_d


@dataclass
class JobResults:
    """``relax`` over J jobs, the arrays on the device."""

    energies: torch.Tensor  # [J] float64
    lattices: torch.Tensor  # [J, 3, 3] float64
    positions: List[torch.Tensor]  # [n_job, 3] float64
    converged: torch.Tensor  # [J] bool
    n_steps: torch.Tensor  # [J] int64
    stresses: Optional[torch.Tensor]  # [J, 3, 3] float64, None without ``optimize_lattice``
    n_calls: int


def relax_jobs(model, cells, cart, src, counts, feats_all, max_atoms_per_call, relax_structures, relax_kwargs, forces_fn, dev,
               masks=None) -> JobResults:
    """``relax`` over the jobs (cells [J, 3, 3], rows of cart / src split by ``counts``), one call per group of ``group_jobs``,
    with ``relax_kwargs`` over ``RELAX_DEFAULTS``; ``steps=0`` without ``relax_structures``.  ``masks``: one cell mask per job."""
    off = offsets(counts)
    groups = group_jobs(counts, max_atoms_per_call)
    kw = dict(RELAX_DEFAULTS, **relax_kwargs)
    if not relax_structures:
        kw["steps"] = 0
    energies, lattices, positions, conv, nsteps, stresses = [], [], [], [], [], []
    for g in groups:
        rows = [slice(int(off[j]), int(off[j + 1])) for j in g]
        feats = None if feats_all is None else [feats_all[src[r].long()] for r in rows]
        if masks is not None:
            kw["cell_mask"] = [masks[j] for j in g]
        res = relax(model, [cells[j] for j in g], [cart[r] for r in rows], feats, forces_fn=forces_fn, device=dev, **kw)
        energies.append(res.energies)
        lattices.append(res.lattices if res.lattices is not None else cells[g[0]:g[-1] + 1].clone())
        positions += res.positions
        conv.append(res.converged)
        nsteps.append(res.n_steps)
        stresses.append(res.stresses)
    return JobResults(energies=torch.cat(energies), lattices=torch.cat(lattices), positions=positions, converged=torch.cat(conv),
                      n_steps=torch.cat(nsteps), stresses=None if stresses[0] is None else torch.cat(stresses),
                      n_calls=len(groups))
