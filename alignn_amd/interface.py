"""Batched interface energies (the work of adhesion of a film on a substrate): the coincidence lattices found on the device, the
interfaces built on the device, every structure relaxed by ``relax`` in groups.

The reference's ``get_interface_energy`` (alignn/ff/ff.py:984-1116) hands one film / substrate pair to jarvis-tools'
``make_interface`` - two surfaces, a Zur-McGill search over the super-lattices of the two surface cells, the film strained onto
the substrate and stacked - and relaxes the substrate slab, the film slab and the interface one after the other.  Here, for P
pairs of B_f film and B_s substrate crystals together:

1. ``alignn_slab_build`` (csrc/defects.hip) cuts every (crystal, Miller index, thickness) once, without vacuum;
2. ``alignn_zsl_match`` (csrc/interface.hip) finds every pair's coincidence lattice: ``match_lattices`` is this step alone;
3. ``alignn_interface_build`` writes, per matched pair and in one common cell, the substrate, the film and the interface;
4. ``relax`` on the 3 jobs per pair, in groups of whole jobs of at most ``max_atoms_per_call`` atoms (alignn_amd/_jobs.py): the
   two slabs with an all-zero ``cell_mask`` (the reference's ``optimize_lattice=False``), the interface with
   ``interface_cell_mask``;
5. ``w_ad = -(E_interface - E_substrate - E_film) / area``.

jarvis-tools, pymatgen and ASE are not dependencies of this project: the match is the one specified in INTEGRATION.md and
restated in tests/interface_ref.py, not "whatever jarvis-tools returns".  It is float64 with a total order on the candidates and
``relax`` keeps a structure's bits independent of its batch, so a pair's numbers are the same whatever else is in the call.
"""

from __future__ import annotations

import math
import numbers
from dataclasses import dataclass
from typing import Callable, List, Optional, Sequence

import numpy as np
import torch

from . import _lib
from ._jobs import MAX_ATOMS_PER_CALL, build_slabs, check_job_options, features, offsets, positive, relax_jobs, slab_layers
from ._structures import check_inputs, gpu_device, host, pack
from .defects import EV_A2_TO_J_M2, miller_basis
from .relax import _full_mask

__all__ = ["interface_energy", "match_lattices", "InterfaceResult", "MatchResult", "MAX_MULTIPLE"]

MAX_MULTIPLE = 256  # the largest super-lattice multiple of a side (csrc/interface.hip ZSL_MAX_N)
_MAX_TABLE_ROWS = 1 << 21  # substrate table rows per launch (192 bytes each)
_TABLES: dict = {}


@dataclass
class MatchResult:
    """Per pair.  ``status``: 0 matched, 1 no coincidence within ``max_area``, 2 a degenerate surface cell (not finite, or v1 x
    v2 not > 0).  ``film_matrix`` / ``subs_matrix`` [P, 2, 2]: the super-cell vectors (rows u, w) in units of the surface cell's
    rows, with determinants ``film_multiple`` and ``subs_multiple``.  ``mismatch_u = | |u_s| / |u_f| - 1 |``, ``mismatch_w``
    likewise, ``mismatch_sin`` the sine of the difference of the two super-cells' angles, ``score`` the largest of the three
    magnitudes.  Where ``status != 0`` the integers are 0 and the floats NaN."""

    status: np.ndarray
    film_multiple: np.ndarray
    subs_multiple: np.ndarray
    film_matrix: np.ndarray
    subs_matrix: np.ndarray
    mismatch_u: np.ndarray
    mismatch_w: np.ndarray
    mismatch_sin: np.ndarray
    score: np.ndarray


@dataclass
class InterfaceResult(MatchResult):
    """``MatchResult`` and, per pair: ``area`` (A^2) of the common cell, the energies (eV) of the film, the substrate and the
    interface in it, ``w_ad = -(e_interface - e_subs - e_film) / area`` (eV/A^2) and ``w_ad_J_m2 = w_ad * EV_A2_TO_J_M2``.  Jobs
    0, 1, 2 of a pair are the substrate, the film and the interface: ``lattices[p]`` [3, 3, 3] and ``positions[p]`` (three
    [n_job, 3]) are the structures after ``relax``, ``converged[p]`` / ``n_steps[p]`` its flags and step counts, ``src[p]`` the
    parent atom of every row (film parents first, then the substrate parents, rows as packed) and ``part[p]`` 0 for a substrate
    row, 1 for a film row.  A pair with ``status != 0`` has NaN energies and ``None`` in the per-job lists."""

    area: np.ndarray = None
    e_film: np.ndarray = None
    e_subs: np.ndarray = None
    e_interface: np.ndarray = None
    w_ad: np.ndarray = None
    w_ad_J_m2: np.ndarray = None
    lattices: List[Optional[torch.Tensor]] = None
    positions: List[Optional[List[torch.Tensor]]] = None
    src: List[Optional[List[torch.Tensor]]] = None
    part: List[Optional[List[torch.Tensor]]] = None
    converged: List[Optional[np.ndarray]] = None
    n_steps: List[Optional[np.ndarray]] = None
    n_relax_calls: int = 0


# --- the match ---------------------------------------------------------------------------------------------------------------------
def _hnf_tables():
    """(hnf int32 [E, 3] = (n, a, b) of every Hermite normal form [[a, b], [0, n / a]], n <= MAX_MULTIPLE, in the order (n, a, b);
    prefix int32 [MAX_MULTIPLE + 2]: the first entry of multiple n)."""
    rows, prefix = [], [0, 0]
    for n in range(1, MAX_MULTIPLE + 1):
        rows += [(n, a, b) for a in range(1, n + 1) if n % a == 0 for b in range(n // a)]
        prefix.append(len(rows))
    return np.array(rows, dtype=np.int32), np.array(prefix, dtype=np.int32)


def _device_tables(dev):
    key = (dev.type, dev.index if dev.index is not None else torch.cuda.current_device())
    if key not in _TABLES:
        hnf, prefix = _hnf_tables()
        _TABLES[key] = (torch.tensor(hnf, device=dev), torch.tensor(prefix, device=dev), prefix)
    return _TABLES[key]


def _largest_multiple(area: float, max_area: float) -> int:
    """The largest n with n area <= max_area, in the kernel's arithmetic."""
    n = int(max_area / area)
    while (n + 1) * area <= max_area:
        n += 1
    while n > 0 and n * area > max_area:
        n -= 1
    return n


def _match_checks(who, max_area, max_area_ratio_tol, ltol, atol):
    positive(who, "max_area", max_area)
    positive(who, "max_area_ratio_tol", max_area_ratio_tol, zero_ok=True)
    positive(who, "ltol", ltol, zero_ok=True)
    if positive(who, "atol", atol, zero_ok=True) > 90.0:
        raise ValueError(f"{who}: atol is an angle in degrees, at most 90, got {atol!r}")


def _match_device(who, film, subs, max_area, max_area_ratio_tol, ltol, atol, dev) -> MatchResult:
    """``alignn_zsl_match`` on checked arguments: ``film`` / ``subs`` float64 numpy [P, 2, 2]."""
    P = len(film)
    cross = lambda c: c[:, 0, 0] * c[:, 1, 1] - c[:, 0, 1] * c[:, 1, 0]  # noqa: E731
    with np.errstate(all="ignore"):
        af, as_ = cross(film), cross(subs)
        valid = (np.isfinite(film).all((1, 2)) & np.isfinite(subs).all((1, 2)) & (af > 0) & np.isfinite(af) & (as_ > 0)
                 & np.isfinite(as_))
    nmax = np.zeros((P, 2), dtype=np.int32)
    for p in np.nonzero(valid)[0]:
        for side, a in enumerate((af[p], as_[p])):
            n = MAX_MULTIPLE + 1 if max_area / a > 2 * MAX_MULTIPLE else _largest_multiple(float(a), float(max_area))
            if n > MAX_MULTIPLE:
                raise ValueError(f"{who}: pair {p}: max_area {max_area} allows multiples above {MAX_MULTIPLE} of the "
                                 f"{('film', 'substrate')[side]} surface cell (area {a:.4g} A^2)")
            nmax[p, side] = n
    lib = _lib.load()
    status = torch.full((P,), -1, dtype=torch.int32, device=dev)
    mult = torch.zeros(P, 2, dtype=torch.int32, device=dev)
    fmat = torch.zeros(P, 2, 2, dtype=torch.int32, device=dev)
    smat = torch.zeros(P, 2, 2, dtype=torch.int32, device=dev)
    mis = torch.full((P, 4), float("nan"), dtype=torch.float64, device=dev)
    with _lib.device_guard(status):
        hnf_d, prefix_d, prefix = _device_tables(dev)
        rows = prefix[nmax + 1].astype(np.int64)  # [P, 2]
        film_d, subs_d = torch.tensor(film, device=dev), torch.tensor(subs, device=dev)
        nmax_d = torch.tensor(nmax, device=dev)
        beg = 0
        while beg < P:  # chunks of pairs whose tables fit the workspace
            end, used = beg + 1, int(rows[beg].max())
            while end < P and end - beg < 16384 and used + int(rows[end].max()) <= _MAX_TABLE_ROWS:
                used += int(rows[end].max())
                end += 1
            n = end - beg
            off = np.concatenate([[[0, 0]], np.cumsum(rows[beg:end], axis=0)])
            f_rows, s_rows = int(off[-1, 0]), int(off[-1, 1])
            max_f, max_s = int(nmax[beg:end, 0].max()), int(nmax[beg:end, 1].max())
            foff = torch.tensor(off[:-1, 0], dtype=torch.int64, device=dev)
            soff = torch.tensor(off[:-1, 1], dtype=torch.int64, device=dev)
            ftab = torch.empty(max(f_rows, 1), 4, dtype=torch.float64, device=dev)
            fint = torch.empty(max(f_rows, 1), 4, dtype=torch.int32, device=dev)
            stab = torch.empty(max(s_rows, 1), 6, 4, dtype=torch.float64, device=dev)
            sint = torch.empty(max(s_rows, 1), 4, dtype=torch.int32, device=dev)
            best_s = torch.empty(n * max(max_f, 1), dtype=torch.float64, device=dev)
            best_t = torch.empty(n * max(max_f, 1), dtype=torch.int64, device=dev)
            nf_d, ns_d = nmax_d[beg:end, 0].contiguous(), nmax_d[beg:end, 1].contiguous()
            _lib.check(lib.alignn_zsl_match(
                film_d[beg:end].data_ptr(), subs_d[beg:end].data_ptr(), n, nf_d.data_ptr(), ns_d.data_ptr(), max_f, max_s,
                hnf_d.data_ptr(), prefix_d.data_ptr(), foff.data_ptr(), soff.data_ptr(), f_rows, s_rows, ftab.data_ptr(),
                fint.data_ptr(), stab.data_ptr(), sint.data_ptr(), best_s.data_ptr(), best_t.data_ptr(),
                float(max_area_ratio_tol), float(ltol), math.cos(math.radians(float(atol))), status[beg:end].data_ptr(),
                mult[beg:end].data_ptr(), fmat[beg:end].data_ptr(), smat[beg:end].data_ptr(), mis[beg:end].data_ptr(),
                _lib.stream()), "zsl_match")
            beg = end
        st, mult_h, mis_h = status.cpu().numpy(), mult.cpu().numpy().astype(np.int64), mis.cpu().numpy()
        fmat_h, smat_h = fmat.cpu().numpy().astype(np.int64), smat.cpu().numpy().astype(np.int64)
    return MatchResult(status=st, film_multiple=mult_h[:, 0], subs_multiple=mult_h[:, 1], film_matrix=fmat_h, subs_matrix=smat_h,
                       mismatch_u=mis_h[:, 0], mismatch_w=mis_h[:, 1], mismatch_sin=mis_h[:, 2], score=mis_h[:, 3])


def _cells_2d(who, name, cells) -> np.ndarray:
    c = host(cells)
    if c.ndim != 3 or c.shape[1:] != (2, 2) or c.shape[0] < 1 or c.dtype.kind not in "iuf":
        raise ValueError(f"{who}: {name} must be numbers [P, 2, 2] with P >= 1, got {c.dtype} {c.shape}")
    return np.ascontiguousarray(c, dtype=np.float64)


def match_lattices(film_cells_2d, subs_cells_2d, *, max_area: float = 500.0, max_area_ratio_tol: float = 1.0, ltol: float = 0.05,
                   atol: float = 1.0, device=None) -> MatchResult:
    """The coincidence lattices of P pairs of surface cells [P, 2, 2] (rows v1, v2 in the plane, right-handed: v1 x v2 > 0), the
    Zur-McGill search of the reference's ``make_interface`` as INTEGRATION.md specifies it.

    Of every super-lattice of the film cell of multiple i (i area_f <= ``max_area``) and of the substrate cell of multiple j
    whose areas agree within ``max_area_ratio_tol``, reduced to their shortest bases, the pair is taken whose vectors' lengths
    agree within ``ltol`` (relative) and whose angles agree within ``atol`` (degrees), with the smallest i, then the smallest
    mismatch.  Rotations of a cell do not matter; a cell and its mirror image are different.  ``max_area`` must not allow
    multiples above ``MAX_MULTIPLE`` = 256 of a cell."""
    who = "match_lattices"
    film, subs = _cells_2d(who, "film_cells_2d", film_cells_2d), _cells_2d(who, "subs_cells_2d", subs_cells_2d)
    if len(film) != len(subs):
        raise ValueError(f"{who}: {len(film)} film cells, {len(subs)} substrate cells (need one of each per pair)")
    _match_checks(who, max_area, max_area_ratio_tol, ltol, atol)
    dev = gpu_device(who, None, True, device)
    return _match_device(who, film, subs, max_area, max_area_ratio_tol, ltol, atol, dev)


# --- the driver --------------------------------------------------------------------------------------------------------------------
def _plane_cell(C) -> np.ndarray:
    """The 2 x 2 cell of a slab cell's first two rows in their plane, x along row 0 (interface.hip plane_cell)."""
    C = [[float(x) for x in row] for row in C]
    l0 = math.sqrt((C[0][0] * C[0][0] + C[0][1] * C[0][1]) + C[0][2] * C[0][2])
    x1 = ((C[0][0] * C[1][0] + C[0][1] * C[1][1]) + C[0][2] * C[1][2]) / l0
    n0, n1, n2 = (C[0][1] * C[1][2] - C[0][2] * C[1][1], C[0][2] * C[1][0] - C[0][0] * C[1][2], C[0][0] * C[1][1] - C[0][1] * C[1][0])
    return np.array([[l0, 0.0], [x1, math.sqrt((n0 * n0 + n1 * n1) + n2 * n2) / l0]])


def _side_inputs(who, name, side):
    if not isinstance(side, (tuple, list)) or len(side) not in (2, 3):
        raise ValueError(f"{who}: {name} must be (lattices, positions, atom_features)")
    return side[0], side[1], side[2] if len(side) == 3 else None


def interface_energy(model, film, substrate, pairs: Sequence, *, film_thickness: float = 25.0, subs_thickness: float = 25.0,
                     separation: float = 3.0, vacuum: float = 8.0, max_area: float = 500.0, max_area_ratio_tol: float = 1.0,
                     ltol: float = 0.05, atol: float = 1.0, interface_cell_mask=(1, 1, 0, 0, 0, 1), relax_structures: bool = True,
                     max_atoms_per_call: int = MAX_ATOMS_PER_CALL, forces_fn: Optional[Callable] = None, device=None,
                     **relax_kwargs) -> InterfaceResult:
    """The work of adhesion of P film / substrate pairs, the reference's ``get_interface_energy`` (ff.py:984) for each.

    ``film`` and ``substrate``: ``(lattices, positions, atom_features)`` of B_f and B_s crystals (alignn_amd/_structures.py; the
    features may be left out with ``forces_fn``), taken as given.  ``pairs``: P tuples ``(film index, film hkl, substrate
    index, substrate hkl)``.  A surface is ``surface_energy``'s slab: ``max(1, int(thickness / h3))`` layers of the crystal in
    ``miller_basis``.  The two surface cells are matched as in ``match_lattices`` (``max_area`` ... ``atol``, the reference's
    defaults), the film is always strained onto the substrate's super-cell (the reference's ``apply_strain``, off by default
    there: nothing else is periodic) and laid
    ``separation`` (A) above the substrate's top atom, with ``vacuum`` (A) above the film's; ``vacuum`` should exceed the
    model's cutoff, or the film sees the substrate's underside.

    Per matched pair three structures in the same cell go to ``relax``: the substrate and the film, each alone, with an
    all-zero ``cell_mask`` (the reference relaxes them with ``optimize_lattice=False``), and the interface with
    ``interface_cell_mask`` (its ``optimize_lattice=True``; six Voigt flags or [3, 3]).  The default keeps the vacuum axis and
    the out-of-plane shears; the reference lets every component go, which shrinks the vacuum.  ``relax_structures``,
    ``relax_kwargs`` (``cell_mask`` and ``fixed`` are refused), ``max_atoms_per_call``: as in ``vacancy_formation``; with
    ``optimize_lattice=False`` no cell moves and the masks are not used.

    ``w_ad = -(E_interface - E_substrate - E_film) / area`` in eV/A^2, ``w_ad_J_m2`` that times ``EV_A2_TO_J_M2`` = 16.02176634
    (the reference multiplies by 16: 0.14 % lower).  A pair without a coincidence lattice within ``max_area`` has ``status`` 1,
    NaN energies and no structures; the other pairs are not affected."""
    who = "interface_energy"
    optimize_lattice = bool(relax_kwargs.get("optimize_lattice", True))
    lat_f, pos_f, feat_f = _side_inputs(who, "film", film)
    lat_s, pos_s, feat_s = _side_inputs(who, "substrate", substrate)
    ns_f = check_inputs(who + " (film)", model, lat_f, pos_f, feat_f, forces_fn=forces_fn, stress=optimize_lattice)
    ns_s = check_inputs(who + " (substrate)", model, lat_s, pos_s, feat_s, forces_fn=forces_fn, stress=optimize_lattice)
    Bf, ns = len(ns_f), ns_f + ns_s
    if relax_kwargs.get("cell_mask") is not None:
        raise ValueError(f"{who}: the cell masks are set per job; use interface_cell_mask")
    check_job_options(who, max_atoms_per_call, relax_kwargs)
    thickness = (positive(who, "film_thickness", film_thickness), positive(who, "subs_thickness", subs_thickness))
    positive(who, "separation", separation)
    positive(who, "vacuum", vacuum, zero_ok=True)
    _match_checks(who, max_area, max_area_ratio_tol, ltol, atol)
    try:
        mask_if = _full_mask(interface_cell_mask, "interface_cell_mask")
    except ValueError as e:
        raise ValueError(f"{who}: {e}") from None
    if not isinstance(pairs, (list, tuple)) or len(pairs) < 1:
        raise ValueError(f"{who}: pairs must be a list of (film index, film hkl, substrate index, substrate hkl)")
    lattices = [host(x).astype(np.float64) for x in list(lat_f) + list(lat_s)]
    slab_of, slab_jobs, slab_counts, pair_slabs = {}, [], [], []
    for p, pr in enumerate(pairs):
        if not isinstance(pr, (list, tuple)) or len(pr) != 4:
            raise ValueError(f"{who}: pairs[{p}] must be (film index, film hkl, substrate index, substrate hkl)")
        ids = []
        for side, (idx, hkl) in enumerate(((pr[0], pr[1]), (pr[2], pr[3]))):
            n_side = len(ns_s) if side else Bf
            if not (isinstance(idx, numbers.Integral) and 0 <= idx < n_side):
                raise ValueError(f"{who}: pairs[{p}] names {('film', 'substrate')[side]} {idx!r} of {n_side}")
            s = int(idx) + (Bf if side else 0)
            bm = miller_basis(lattices[s], hkl)  # (checks hkl)
            key = (s, tuple(int(v) for v in bm.reshape(-1)))
            if key not in slab_of:
                layers = slab_layers(who, f"the {('film', 'substrate')[side]} lattice {idx}", f"pairs[{p}]", lattices[s], bm, hkl,
                                     thickness[side], ns[s])
                slab_of[key] = len(slab_jobs)
                slab_jobs.append([s] + list(key[1]) + [layers])
                slab_counts.append(ns[s] * layers)
            ids.append(slab_of[key])
        pair_slabs.append(ids)
    dev = gpu_device(who, model, forces_fn, device)
    lib = _lib.load()
    P, S = len(pairs), len(slab_jobs)
    nan = np.full(P, np.nan)
    out = dict(area=nan.copy(), e_film=nan.copy(), e_subs=nan.copy(), e_interface=nan.copy(), lattices=[None] * P,
               positions=[None] * P, src=[None] * P, part=[None] * P, converged=[None] * P, n_steps=[None] * P, n_relax_calls=0)

    with _lib.device_guard(torch.empty(0, device=dev)):
        packed = pack(lattices, list(pos_f) + list(pos_s), ns, dev, frac=False)
        s_cells, s_cart, s_src, slab_off_d = build_slabs(packed, slab_jobs, slab_counts, 0.0, dev)  # (without vacuum)
        planes = [_plane_cell(c) for c in s_cells.cpu().numpy()]
        m = _match_device(who, np.stack([planes[f] for f, _ in pair_slabs]), np.stack([planes[s] for _, s in pair_slabs]),
                          max_area, max_area_ratio_tol, ltol, atol, dev)
        matched = [int(p) for p in np.nonzero(m.status == 0)[0]]
        if matched:
            K = len(matched)
            jobs, counts = [], []
            for p in matched:
                f, s = pair_slabs[p]
                jobs.append([f, s] + [int(v) for v in m.film_matrix[p].reshape(-1)] + [int(v) for v in m.subs_matrix[p].reshape(-1)])
                n_s, n_f = int(m.subs_multiple[p]) * slab_counts[s], int(m.film_multiple[p]) * slab_counts[f]
                counts += [n_s, n_f, n_s + n_f]
            off = offsets(counts)
            rows = int(off[-1])
            if rows > np.iinfo(np.int32).max:
                raise ValueError(f"{who}: the interfaces have {rows} atoms in all; split the pairs over several calls")
            cells = torch.empty(3 * K, 3, 3, dtype=torch.float64, device=dev)
            cart = torch.empty(rows, 3, dtype=torch.float64, device=dev)
            frac = torch.empty_like(cart)
            src = torch.empty(rows, dtype=torch.int32, device=dev)
            part = torch.empty(rows, dtype=torch.int32, device=dev)
            area = torch.empty(K, dtype=torch.float64, device=dev)
            pair_jobs_d = torch.tensor(jobs, dtype=torch.int32, device=dev)
            sep_d = torch.full((K,), float(separation), dtype=torch.float64, device=dev)
            vac_d = torch.full((K,), float(vacuum), dtype=torch.float64, device=dev)
            off_d = torch.tensor(off, device=dev)
            _lib.check(lib.alignn_interface_build(
                s_cells.data_ptr(), s_cart.data_ptr(), slab_off_d.data_ptr(), s_src.data_ptr(), S, pair_jobs_d.data_ptr(),
                sep_d.data_ptr(), vac_d.data_ptr(), off_d.data_ptr(), K, cells.data_ptr(), cart.data_ptr(), frac.data_ptr(),
                src.data_ptr(), part.data_ptr(), area.data_ptr(), _lib.stream()), "interface_build")
            feats = None
            if forces_fn is None:
                feats = features(list(feat_f) + list(feat_s), forces_fn, dev)
            masks = [np.zeros((3, 3)), np.zeros((3, 3)), mask_if] * K if optimize_lattice else None
            r = relax_jobs(model, cells, cart, src, counts, feats, max_atoms_per_call, relax_structures, relax_kwargs, forces_fn,
                           dev, masks)
            e, conv, nsteps = r.energies.cpu().numpy(), r.converged.cpu().numpy(), r.n_steps.cpu().numpy()
            area_h = area.cpu().numpy()
            out["n_relax_calls"] = r.n_calls
            for k, p in enumerate(matched):
                j = 3 * k
                out["area"][p], out["e_subs"][p], out["e_film"][p], out["e_interface"][p] = area_h[k], e[j], e[j + 1], e[j + 2]
                out["lattices"][p] = r.lattices[j:j + 3]
                out["positions"][p] = r.positions[j:j + 3]
                out["src"][p] = [src[off[j + q]:off[j + q + 1]] for q in range(3)]
                out["part"][p] = [part[off[j + q]:off[j + q + 1]] for q in range(3)]
                out["converged"][p], out["n_steps"][p] = conv[j:j + 3], nsteps[j:j + 3]
    w_ad = -(out["e_interface"] - out["e_subs"] - out["e_film"]) / out["area"]
    return InterfaceResult(status=m.status, film_multiple=m.film_multiple, subs_multiple=m.subs_multiple, film_matrix=m.film_matrix,
                           subs_matrix=m.subs_matrix, mismatch_u=m.mismatch_u, mismatch_w=m.mismatch_w,
                           mismatch_sin=m.mismatch_sin, score=m.score, w_ad=w_ad, w_ad_J_m2=w_ad * EV_A2_TO_J_M2, **out)
