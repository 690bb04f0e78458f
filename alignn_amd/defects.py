"""Batched vacancy formation energies and surface energies: the derived structures built on the device, all of them relaxed by
one ``relax`` call.

The reference's ``vacancy_formation`` (alignn/ff/ff.py:808-897) and ``surface_energy`` (ff.py:900-981) build a few dozen derived
structures from one crystal on the host - jarvis-tools' ``Vacancy.generate_defects`` (a supercell, and the supercell minus one
atom per inequivalent site) and ``Surface.make_surface`` (one slab per Miller index, a port of ASE's
``ase/build/general_surface.py``) - and relax each one alone through a new ``ForceField``.  Here, for B parent crystals together:

1. the job list (host, integers): supercell sizes and removed atoms, or ``miller_basis`` and layer counts;
2. ``alignn_defect_supercells`` / ``alignn_slab_build`` (csrc/defects.hip) write every job's cell, Cartesian positions, wrapped
   fractions and ``src``, the parent atom of every row (one gather gives the atom features);
3. ``relax`` on the jobs, in groups of whole jobs of at most ``max_atoms_per_call`` atoms (alignn_amd/_jobs.py);
4. the energies reduced to formation / surface energies.

The builders are float64 with fixed-order sums and ``relax`` keeps a structure's bits independent of its batch, so a parent's
numbers are the same whatever else is in the call.  tests/defects_ref.py restates the builders and the formulas in numpy.
"""

from __future__ import annotations

import math
import numbers
from dataclasses import dataclass
from typing import Callable, List, Optional, Sequence

import numpy as np
import torch

from . import _lib
from ._jobs import (MAX_ATOMS_PER_CALL, build_slabs, check_job_options, features, offsets, positive, relax_jobs, slab_layers,
                    split)
from ._structures import check_inputs, gpu_device, host, pack

__all__ = ["vacancy_formation", "surface_energy", "VacancyResult", "SurfaceResult", "miller_basis", "EV_A2_TO_J_M2"]

EV_A2_TO_J_M2 = 16.02176634  # eV/A^2 -> J/m^2 (the elementary charge, CODATA 2018, x 1e20 / 1e19)


def _ext_gcd(a: int, b: int):
    """ase/build/general_surface.py ext_gcd: (x, y) with a x + b y = gcd(a, b), Python's floor division and modulo."""
    if b == 0:
        return 1, 0
    if a % b == 0:
        return 0, 1
    x, y = _ext_gcd(b, a % b)
    return y, x - y * (a // b)


def _det3i(m) -> int:
    return (m[0][0] * (m[1][1] * m[2][2] - m[1][2] * m[2][1]) - m[0][1] * (m[1][0] * m[2][2] - m[1][2] * m[2][0])
            + m[0][2] * (m[1][0] * m[2][1] - m[1][1] * m[2][0]))


def miller_basis(lattice, hkl) -> np.ndarray:
    """The integer basis (rows c1, c2, c3) of ASE's ``surface(lattice, indices)``: c1 and c2 span the (hkl) plane of the cell
    ``lattice`` [3, 3] (rows a1, a2, a3), chosen as close to orthogonal as the construction allows, and c3 completes a unimodular
    basis.  ``hkl`` is reduced by its gcd.  Where ASE's basis has det -1, c2 is negated: it lies in the plane, so the surface is
    the same and the slab's cell stays right-handed.  -> int64 [3, 3], det +1."""
    idx = np.asarray(hkl)
    if idx.shape != (3,) or not all(isinstance(v, numbers.Integral) or float(v).is_integer() for v in idx):
        raise ValueError(f"miller_basis: hkl must be three integers, got {hkl!r}")
    h, k, l = (int(v) for v in idx)
    g = math.gcd(math.gcd(h, k), l)
    if g == 0:
        raise ValueError("miller_basis: hkl = (0, 0, 0) is no plane")
    h, k, l = h // g, k // g, l // g
    lat = np.asarray(lattice.detach().cpu() if isinstance(lattice, torch.Tensor) else lattice, dtype=np.float64)
    if lat.shape != (3, 3):
        raise ValueError(f"miller_basis: lattice is {lat.shape}, need [3, 3]")
    if (h == 0) + (k == 0) + (l == 0) == 2:
        if h != 0:
            c1, c2, c3 = (0, 1, 0), (0, 0, 1), (1, 0, 0)
        elif k != 0:
            c1, c2, c3 = (0, 0, 1), (1, 0, 0), (0, 1, 0)
        else:
            c1, c2, c3 = (1, 0, 0), (0, 1, 0), (0, 0, 1)
    else:
        p, q = _ext_gcd(k, l)
        a1, a2, a3 = lat
        # dot(c1, c2) = k1 + i k2 for the integer shear i of the in-plane basis
        k1 = np.dot(p * (k * a1 - h * a2) + q * (l * a1 - h * a3), l * a2 - k * a3)
        k2 = np.dot(l * (k * a1 - h * a2) - k * (l * a1 - h * a3), l * a2 - k * a3)
        if abs(k2) > 1e-10:
            i = -int(round(k1 / k2))
            p, q = p + i * l, q - i * k
        a, b = _ext_gcd(p * k + q * l, h)
        c1 = (p * k + q * l, -p * h, -q * h)
        d = abs(math.gcd(l, k))
        c2 = (0, l // d, -k // d)
        c3 = (b, a * p, a * q)
    basis = [list(c1), list(c2), list(c3)]
    det = _det3i(basis)
    if det == -1:
        basis[1] = [-v for v in basis[1]]
    elif det != 1:
        raise ValueError(f"miller_basis: the basis of hkl = {(h, k, l)} has det {det}, not +-1")
    return np.array(basis, dtype=np.int64)


@dataclass
class VacancyResult:
    """Per parent s, in the input order; the per-class arrays in the order of ``labels[s]`` (the distinct site labels, ascending).
    ``formation_energy[s][c] = e_defect[s][c] - (n_defect + 1) e_bulk[s] / n_bulk[s] + mu`` (eV) with n_defect = n_bulk - 1.
    Job 0 of a parent is its pristine supercell, job 1 + c the defect of class c: ``lattices[s]`` [1 + C, 3, 3] and
    ``positions[s]`` (a list of [n_job, 3]) are the structures after ``relax``, ``converged[s]`` / ``n_steps[s]`` its flags and
    step counts, ``src[s]`` the parent atom of every row of a job."""

    supercell: List[tuple]
    n_bulk: List[int]
    labels: List[np.ndarray]
    multiplicity: List[np.ndarray]  # the class's count in the parent cell
    removed_atom: List[np.ndarray]  # the supercell (= parent) atom taken out: the class's lowest index, image 0
    e_bulk: np.ndarray  # [B] eV, the whole supercell
    e_defect: List[np.ndarray]
    formation_energy: List[np.ndarray]
    lattices: List[torch.Tensor]
    positions: List[List[torch.Tensor]]
    src: List[List[torch.Tensor]]
    converged: List[np.ndarray]
    n_steps: List[np.ndarray]
    n_relax_calls: int


@dataclass
class SurfaceResult:
    """Per parent s, in the input order; the per-slab arrays in the order of its Miller indices.  ``surf_en[s][m] =
    (e_slab - epa[s] n_slab) / (2 area)`` in eV/A^2, ``surf_en_J_m2`` that times ``EV_A2_TO_J_M2``.  ``area`` is |C0 x C1| of the
    slab as built, ``epa`` the relaxed parent's energy per atom.  Job 0 of a parent is the parent itself, job 1 + m slab m:
    ``lattices`` ... ``n_steps`` as in ``VacancyResult``."""

    miller_indices: List[np.ndarray]
    basis: List[np.ndarray]  # [M, 3, 3] int
    layers: List[np.ndarray]
    n_slab: List[np.ndarray]
    area: List[np.ndarray]
    epa: np.ndarray  # [B] eV / atom
    e_slab: List[np.ndarray]
    surf_en: List[np.ndarray]
    surf_en_J_m2: List[np.ndarray]
    lattices: List[torch.Tensor]
    positions: List[List[torch.Tensor]]
    src: List[List[torch.Tensor]]
    converged: List[np.ndarray]
    n_steps: List[np.ndarray]
    n_relax_calls: int


def _supercell_dims(who, supercell, lattices, enforce_c_size, extend, B) -> List[tuple]:
    if supercell is None:
        if not (isinstance(enforce_c_size, numbers.Real) and np.isfinite(enforce_c_size) and enforce_c_size >= 0):
            raise ValueError(f"{who}: enforce_c_size must be a finite number >= 0")
        if not (isinstance(extend, numbers.Integral) and extend >= 0):
            raise ValueError(f"{who}: extend must be an int >= 0")
        out = []
        for lat in lattices:
            lengths = np.sqrt((host(lat).astype(np.float64) ** 2).sum(1))
            if not (np.isfinite(lengths).all() and (lengths > 0).all()):
                raise ValueError(f"{who}: a lattice vector has no length")
            out.append(tuple(int(enforce_c_size / x) + int(extend) for x in lengths))
    else:
        sc = np.asarray(supercell)
        if sc.shape == (3,):
            sc = np.broadcast_to(sc, (B, 3))
        if sc.shape != (B, 3) or not all(isinstance(v, numbers.Integral) or float(v).is_integer() for v in sc.reshape(-1)):
            raise ValueError(f"{who}: supercell must be (N1, N2, N3) or one per structure ({B}), got {supercell!r}")
        out = [tuple(int(v) for v in row) for row in sc]
    if any(v < 1 for row in out for v in row):
        raise ValueError(f"{who}: supercell sizes must be >= 1, got {out!r}")
    return out


def _on_conventional_cell(who, flag, model, lattices, positions, atom_features, forces_fn, stress, species, symprec, device,
                          site_labels=None):
    """``on_conventional_cell``: False leaves the parents as given; True replaces them by ``conventional_cell`` of them, with
    ``atom_features``, ``species`` and the ``site_labels`` arrays taken through ``source_atom``.
    -> (lattices, positions, atom_features, species, site_labels)."""
    if not isinstance(flag, (bool, np.bool_)):
        raise ValueError(f"{who}: on_conventional_cell is one bool, got {type(flag).__name__}")
    if not flag:
        return lattices, positions, atom_features, species, site_labels
    from .cells import conventional_cell

    ns = check_inputs(who, model, lattices, positions, atom_features, forces_fn=forces_fn, stress=stress)
    arrays = site_labels is not None and not isinstance(site_labels, str)
    for name, rows in (("species", species), ("site_labels", site_labels if arrays else None)):
        if rows is None:
            continue
        if len(rows) != len(ns):
            raise ValueError(f"{who}: {name} needs one integer [n_i] array per structure, {len(ns)} of them")
        for s, r in enumerate(rows):
            if host(r).shape != (ns[s],):
                raise ValueError(f"{who}: {name}[{s}] is {host(r).shape}, need [{ns[s]}]")
    cell = conventional_cell(lattices, positions, species, symprec=symprec, device=gpu_device(who, model, forces_fn, device))
    src = host(cell.packed["source_atom"]).astype(np.int64)  # (one copy: the rows of every host array are taken through it)
    ptr = np.concatenate([[0], np.cumsum(cell.ns)])
    src = [src[ptr[s]:ptr[s + 1]] for s in range(len(ns))]

    def through(rows):
        if rows is None:
            return None
        return [r[torch.as_tensor(i, device=r.device)] if isinstance(r, torch.Tensor) else np.asarray(r)[i] for r, i in zip(rows, src)]

    return ([cell.lattices[s] for s in range(len(ns))], cell.positions, through(atom_features), through(species),
            through(site_labels) if arrays else site_labels)


def vacancy_formation(model, lattices: Sequence, positions: Sequence, atom_features: Optional[Sequence] = None, *,
                      site_labels: Optional[Sequence] = None, supercell=None, enforce_c_size: float = 15.0, extend: int = 1,
                      chemical_potentials: Optional[Sequence] = None, relax_structures: bool = True,
                      max_atoms_per_call: int = MAX_ATOMS_PER_CALL, forces_fn: Optional[Callable] = None, device=None,
                      species: Optional[Sequence] = None, symprec: float = 1e-3, on_conventional_cell: bool = False,
                      **relax_kwargs) -> VacancyResult:
    """Vacancy formation energies of B crystals, the reference's ``vacancy_formation`` (ff.py:808) for each: per parent one
    pristine supercell and one supercell with an atom removed per class of sites, all relaxed together.

    The structures, the model (or ``forces_fn``) and the device: alignn_amd/_structures.py.  ``supercell``: (N1, N2, N3) for all
    or one per structure; by default jarvis-tools' rule, ``int(enforce_c_size / |a_k|) + extend`` along axis k.
    ``site_labels``: B integer arrays [n_s], one class per distinct label (e.g. the Wyckoff classes of spglib, the reference's
    ``using_wyckoffs``); default: every atom its own class; ``"auto"``: the orbits of ``find_symmetry(lattices, positions,
    species, symprec=symprec)``, the atoms the crystal's own symmetry makes equivalent (``species``: B integer arrays, None: all
    atoms alike; both are used by ``"auto"`` and ``on_conventional_cell`` only).  The atom removed is the class's lowest-index atom, in image 0.
    ``chemical_potentials``: B arrays with one value (eV) per class in ascending label order, added to the formation energy;
    default 0 (the reference reads jarvis' unary-energy table).  ``on_conventional_cell=True`` (the reference's default; here
    False, the parents as given) first replaces the parents by ``conventional_cell(lattices, positions, species,
    symprec=symprec)`` of them (alignn_amd/cells.py): the rows of ``atom_features``, ``species`` and the ``site_labels`` arrays
    are taken through its ``source_atom``, ``"auto"`` is evaluated on the new cell, and ``supercell`` / ``enforce_c_size`` refer
    to it.

    ``relax_structures=False`` evaluates the structures as built (``steps=0``).  ``relax_kwargs`` go to ``relax`` as whole-call
    options; ``steps=100``, ``fmax=0.1`` and ``optimize_lattice=True`` are the defaults here, as in the reference's
    ``optimize_atoms()`` (the model, or ``forces_fn``, must then give stresses).  ``max_atoms_per_call``: atoms per ``relax``
    call (whole jobs).  The reference relaxes the same pristine supercell once per defect; here once per parent."""
    who = "vacancy_formation"
    optimize_lattice = bool(relax_kwargs.get("optimize_lattice", True))
    lattices, positions, atom_features, species, site_labels = _on_conventional_cell(
        who, on_conventional_cell, model, lattices, positions, atom_features, forces_fn, optimize_lattice, species, symprec, device,
        site_labels)
    ns = check_inputs(who, model, lattices, positions, atom_features, forces_fn=forces_fn, stress=optimize_lattice)
    B = len(ns)
    check_job_options(who, max_atoms_per_call, relax_kwargs)
    dims = _supercell_dims(who, supercell, lattices, enforce_c_size, extend, B)
    n_bulk = [n * d[0] * d[1] * d[2] for n, d in zip(ns, dims)]
    for s, n in enumerate(n_bulk):
        if n < 2:
            raise ValueError(f"{who}: the supercell of structure {s} has one atom; without it nothing is left")
    auto = isinstance(site_labels, str)
    if auto and site_labels != "auto":
        raise ValueError(f"{who}: site_labels is B integer arrays, None or \"auto\", got {site_labels!r}")
    if site_labels is not None and not auto and len(site_labels) != B:
        raise ValueError(f"{who}: site_labels needs one integer [n_i] array per structure, {B} of them")
    if auto:
        from .symmetry import find_symmetry

        site_labels = find_symmetry(lattices, positions, species, symprec=symprec,
                                    device=gpu_device(who, model, forces_fn, device)).orbits
    labels, mult, removed = [], [], []
    for s in range(B):
        lab = np.arange(ns[s]) if site_labels is None else host(site_labels[s])
        if lab.shape != (ns[s],) or lab.dtype.kind not in "iu":
            raise ValueError(f"{who}: site_labels[{s}] is {lab.dtype} {lab.shape}, need integers [{ns[s]}]")
        u, first, count = np.unique(lab, return_index=True, return_counts=True)
        labels.append(u)
        removed.append(first.astype(np.int64))
        mult.append(count.astype(np.int64))
    if chemical_potentials is not None and len(chemical_potentials) != B:
        raise ValueError(f"{who}: chemical_potentials needs one array per structure, {B} of them")
    mus = []
    for s in range(B):
        mu = np.zeros(len(labels[s])) if chemical_potentials is None else host(chemical_potentials[s]).astype(np.float64)
        if mu.shape != (len(labels[s]),) or not np.isfinite(mu).all():
            raise ValueError(f"{who}: chemical_potentials[{s}] needs {len(labels[s])} finite values, one per class")
        mus.append(mu)
    dev = gpu_device(who, model, forces_fn, device)
    lib = _lib.load()

    jobs, counts, job_ptr = [], [], [0]
    for s in range(B):
        jobs.append((s, -1))
        counts.append(n_bulk[s])
        for a in removed[s]:
            jobs.append((s, int(a)))
            counts.append(n_bulk[s] - 1)
        job_ptr.append(len(jobs))
    J, rows = len(jobs), int(sum(counts))
    with _lib.device_guard(torch.empty(0, device=dev)):
        packed = pack(lattices, positions, ns, dev, frac=False)
        dims_d = torch.tensor(dims, dtype=torch.int32, device=dev)
        jobs_d = torch.tensor(jobs, dtype=torch.int32, device=dev)
        off = offsets(counts)
        off_d = torch.tensor(off, dtype=torch.int64, device=dev)
        cells = torch.empty(J, 3, 3, dtype=torch.float64, device=dev)
        cart = torch.empty(rows, 3, dtype=torch.float64, device=dev)
        frac = torch.empty(rows, 3, dtype=torch.float64, device=dev)
        src = torch.empty(rows, dtype=torch.int32, device=dev)
        _lib.check(lib.alignn_defect_supercells(
            packed.pos.data_ptr(), packed.atom_ptr.data_ptr(), packed.lat.data_ptr(), dims_d.data_ptr(), B, jobs_d.data_ptr(),
            off_d.data_ptr(), J, cells.data_ptr(), cart.data_ptr(), frac.data_ptr(), src.data_ptr(), _lib.stream()),
            "defect_supercells")
        r = relax_jobs(model, cells, cart, src, counts, features(atom_features, forces_fn, dev), max_atoms_per_call,
                       relax_structures, relax_kwargs, forces_fn, dev)
        e, conv, nsteps = r.energies.cpu().numpy(), r.converged.cpu().numpy(), r.n_steps.cpu().numpy()
        src_jobs = [src[off[j]:off[j + 1]] for j in range(J)]
    e_bulk = np.array([e[job_ptr[s]] for s in range(B)])
    e_def = [e[job_ptr[s] + 1:job_ptr[s + 1]] for s in range(B)]
    form = [e_def[s] - (n_bulk[s] - 1 + 1) * e_bulk[s] / n_bulk[s] + mus[s] for s in range(B)]
    return VacancyResult(supercell=dims, n_bulk=n_bulk, labels=labels, multiplicity=mult, removed_atom=removed, e_bulk=e_bulk,
                         e_defect=e_def, formation_energy=form, lattices=split(r.lattices, job_ptr),
                         positions=split(r.positions, job_ptr), src=split(src_jobs, job_ptr), converged=split(conv, job_ptr),
                         n_steps=split(nsteps, job_ptr), n_relax_calls=r.n_calls)


def _miller_lists(who, miller_indices, B) -> List[np.ndarray]:
    try:
        arr = np.asarray(miller_indices)
    except ValueError:  # ragged: B lists of different lengths
        arr = None
    if arr is not None and arr.dtype != object and arr.ndim == 2:
        lists = [arr] * B
    elif len(miller_indices) == B:
        lists = [np.asarray(m) for m in miller_indices]
    else:
        raise ValueError(f"{who}: miller_indices is one list of hkl for all structures, or {B} lists")
    for m in lists:
        if m.ndim != 2 or m.shape[1] != 3 or m.shape[0] < 1 or m.dtype.kind not in "iu":
            raise ValueError(f"{who}: every list of Miller indices needs integer [M, 3] with M >= 1")
    return lists


def surface_energy(model, lattices: Sequence, positions: Sequence, atom_features: Optional[Sequence] = None, *,
                   miller_indices, thickness: float = 25.0, vacuum: float = 18.0, relax_structures: bool = True,
                   max_atoms_per_call: int = MAX_ATOMS_PER_CALL, forces_fn: Optional[Callable] = None, device=None,
                   on_conventional_cell: bool = False, species: Optional[Sequence] = None, symprec: float = 1e-3,
                   **relax_kwargs) -> SurfaceResult:
    """Surface energies of B crystals, the reference's ``surface_energy`` (ff.py:900) for each: per parent the parent itself
    (its energy per atom) and one slab per Miller index, all relaxed together.

    The structures, the model (or ``forces_fn``) and the device: alignn_amd/_structures.py.  ``miller_indices``: one list of
    (h, k, l) for all parents, or B lists.  A slab is ASE's general surface construction on ``miller_basis``: ``layers = max(1,
    int(thickness / h3))`` repeats of the parent in the oriented cell, h3 the spacing of its (hkl) planes, ``vacuum`` (A) added
    above the slab.  ``on_conventional_cell=True`` (the reference's default; here False, the parents as given) first replaces the
    parents by ``conventional_cell(lattices, positions, species, symprec=symprec)`` of them (alignn_amd/cells.py), the rows of
    ``atom_features`` taken through its ``source_atom``: Miller indices and thickness then refer to the conventional cell.
    ``species`` (B integer arrays, None: all atoms alike) and ``symprec`` are used by that option only.

    ``surf_en = (E_slab - epa n_slab) / (2 area)`` in eV/A^2; ``surf_en_J_m2`` is that times ``EV_A2_TO_J_M2`` = 16.02176634.
    The reference multiplies by 16 instead, so its figures are 0.14 % lower.

    ``relax_structures``, ``relax_kwargs``, ``max_atoms_per_call``: as in ``vacancy_formation``; ``optimize_lattice=True`` is the
    default, as in the reference.  For slabs ``cell_mask=[1, 1, 0, 0, 0, 1]`` is recommended: the in-plane cell relaxes and the
    vacuum axis stays (with every component free the filter shrinks the vacuum)."""
    who = "surface_energy"
    optimize_lattice = bool(relax_kwargs.get("optimize_lattice", True))
    lattices, positions, atom_features, _, _ = _on_conventional_cell(
        who, on_conventional_cell, model, lattices, positions, atom_features, forces_fn, optimize_lattice, species, symprec, device)
    ns = check_inputs(who, model, lattices, positions, atom_features, forces_fn=forces_fn, stress=optimize_lattice)
    B = len(ns)
    check_job_options(who, max_atoms_per_call, relax_kwargs)
    positive(who, "thickness", thickness)
    positive(who, "vacuum", vacuum, zero_ok=True)
    hkls = _miller_lists(who, miller_indices, B)
    bases, layers = [], []
    for s in range(B):
        lat = host(lattices[s]).astype(np.float64)
        bs, ls = [], []
        for hkl in hkls[s]:
            bs.append(miller_basis(lat, hkl))
            ls.append(slab_layers(who, f"lattices[{s}]", f"structure {s}", lat, bs[-1], hkl, thickness, ns[s]))
        bases.append(np.stack(bs))
        layers.append(np.array(ls, dtype=np.int64))
    dev = gpu_device(who, model, forces_fn, device)

    slab_jobs, slab_counts = [], []
    for s in range(B):
        for bm, nl in zip(bases[s], layers[s]):
            slab_jobs.append([s] + [int(v) for v in bm.reshape(-1)] + [int(nl)])
            slab_counts.append(ns[s] * int(nl))
    with _lib.device_guard(torch.empty(0, device=dev)):
        packed = pack(lattices, positions, ns, dev, frac=False)
        cells, cart, src, _ = build_slabs(packed, slab_jobs, slab_counts, vacuum, dev)
        # the job list of relax: per parent the parent itself, then its slabs
        slab_off = offsets(slab_counts)
        order_cells, order_cart, order_src, counts, job_ptr, k = [], [], [], [], [0], 0
        for s in range(B):
            a, b = packed.ptr[s], packed.ptr[s + 1]
            order_cells.append(packed.lat[s:s + 1])
            order_cart.append(packed.pos[a:b])
            order_src.append(torch.arange(a, b, dtype=torch.int32, device=dev))
            counts.append(ns[s])
            for _ in range(len(layers[s])):
                order_cells.append(cells[k:k + 1])
                order_cart.append(cart[slab_off[k]:slab_off[k + 1]])
                order_src.append(src[slab_off[k]:slab_off[k + 1]])
                counts.append(slab_counts[k])
                k += 1
            job_ptr.append(len(counts))
        all_cells, all_cart, all_src = torch.cat(order_cells), torch.cat(order_cart), torch.cat(order_src)
        r = relax_jobs(model, all_cells, all_cart, all_src, counts, features(atom_features, forces_fn, dev), max_atoms_per_call,
                       relax_structures, relax_kwargs, forces_fn, dev)
        e, conv, nsteps = r.energies.cpu().numpy(), r.converged.cpu().numpy(), r.n_steps.cpu().numpy()
        cells_h = cells.cpu().numpy()
        off = offsets(counts)
        src_jobs = [all_src[off[j]:off[j + 1]] for j in range(len(counts))]
    epa = np.array([e[job_ptr[s]] / ns[s] for s in range(B)])
    e_slab, n_slab, area, surf, k = [], [], [], [], 0
    for s in range(B):
        M = len(layers[s])
        e_slab.append(e[job_ptr[s] + 1:job_ptr[s + 1]])
        n_slab.append(ns[s] * layers[s])
        nu = np.cross(cells_h[k:k + M, 0], cells_h[k:k + M, 1])
        area.append(np.sqrt((nu * nu).sum(1)))
        surf.append((e_slab[s] - epa[s] * n_slab[s]) / (2 * area[s]))
        k += M
    return SurfaceResult(miller_indices=hkls, basis=bases, layers=layers, n_slab=n_slab, area=area, epa=epa, e_slab=e_slab,
                         surf_en=surf, surf_en_J_m2=[x * EV_A2_TO_J_M2 for x in surf], lattices=split(r.lattices, job_ptr),
                         positions=split(r.positions, job_ptr), src=split(src_jobs, job_ptr), converged=split(conv, job_ptr),
                         n_steps=split(nsteps, job_ptr), n_relax_calls=r.n_calls)
