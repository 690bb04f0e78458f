"""Batched finite-displacement phonons: force constants, frequencies at q-points and the DOS, on the device.

The reference computes phonons one structure and one displaced supercell at a time: ``ase_phonon`` (alignn/ff/ff.py:1337)
runs ASE's ``Phonons`` (an N x N x N supercell, every atom displaced by +-delta along x, y, z, one ``AlignnAtomwiseCalculator``
call per displaced supercell), reads the force constants, and diagonalises the dynamical matrix on the host, q-point after
q-point, for a band path and a 20 x 20 x 20 DOS mesh.  ``phonons`` does this for B structures together:

1. ``alignn_phonon_displace`` (csrc/phonon.hip) writes the displaced supercells of a chunk - several whole -/+ pairs of all
   B structures - straight into the fractional-coordinate array ``neighbors.crystal_batch`` takes;
2. one ``model(batch)`` per chunk (``max_atoms_per_eval`` supercell atoms), or ``forces_fn``;
3. ``alignn_phonon_fc_rows`` turns the chunk's forces into force-constant rows; after the last chunk ``_symmetrize``,
   ``_acoustic`` and ``_mass_weight`` finish C_R and D_R, all on the device;
4. ``alignn_phonon_eigh``: D(q) and its eigenvalues (and eigenvectors) in one workgroup per (structure, q), parallel cyclic
   Jacobi in LDS; ``alignn_phonon_dos``: the Gaussian-smeared DOS over a Monkhorst-Pack mesh.

The semantics are ASE 3.22.1's ``Phonons`` (``environment.yml``), restated in numpy in tests/phonons_ref.py.

``displacements="symmetry"`` (with the ``SymmetryResult`` of ``find_symmetry``) evaluates only the symmetry-inequivalent
displacements, as the reference's ``phonons()`` does through phonopy (alignn/ff/ff.py:1119): the operations that map the supercell
onto itself pick one representative atom per class and as few directions per representative as its site group allows
(``alignn_phsym_plan``), ``alignn_phsym_displace`` / ``alignn_phsym_rows`` take the place of steps 1 and 3 for those directions
alone, and ``alignn_phsym_solve`` / ``alignn_phsym_distribute`` (csrc/phonon_sym.hip) solve for the representatives' force
constants and rotate them onto the other atoms; everything after that is shared.  The rules are stated in
include/alignn_phsym.h and restated in numpy in tests/phonons_sym_ref.py; phonopy's own direction lists are not reproduced.
"""

from __future__ import annotations

import ctypes as C
import numbers
from dataclasses import dataclass, field
from typing import Callable, List, Optional, Sequence

import numpy as np
import torch

from . import _abi, _lib
from ._structures import ForceEvaluator, check_inputs, gpu_device, host, pack
from .symmetry import SymmetryResult

__all__ = ["phonons", "PhononResult", "EV_TO_THZ", "EV_TO_CM1", "MAX_DIM", "monkhorst_pack", "lattice_points", "repeat_symmetry"]

# CODATA 2014 (ASE's default units): hbar (J s), the elementary charge (C), the atomic mass unit (kg), h (J s), c (m/s)
_HBAR, _E, _AMU, _H, _C = 1.054571800e-34, 1.6021766208e-19, 1.660539040e-27, 6.626070040e-34, 299792458.0
# sqrt(eV / A^2 / amu) -> eV (ASE's band_structure), and eV -> THz / cm^-1 for plots in the reference's units
FREQ_SCALE = _HBAR * 1e10 / np.sqrt(_E * _AMU)
EV_TO_THZ = _E / _H / 1e12
EV_TO_CM1 = _E / (_H * _C * 100.0)
MAX_DIM = 96  # 3n limit of the eigen launch (csrc/phonon.hip PH_MAX_M: the matrix of D(q) in LDS)
DRIFTS = {None: 0, "frederiksen": 1, "mean": 2}
# Supercell atoms per model evaluation by default.  Measured on an MI355X with the tools/phonon_time.py model: see
# INTEGRATION.md, "Phonons".
MAX_ATOMS_PER_EVAL = 32768
DISPLACEMENTS = ("all", "symmetry")

# the entry points of the symmetry-reduced path: include/alignn_phsym.h
PHSYM = _abi.header("alignn_phsym.h")
PHSYM_HEADER, PHSYM_STRUCTS, PHSYM_SIGNATURES = PHSYM.path, PHSYM.structs, PHSYM.signatures
PlanArgs, DisplaceArgs = PHSYM_STRUCTS["alignn_phsym_plan_args"], PHSYM_STRUCTS["alignn_phsym_displace_args"]
RowsArgs, FcArgs = PHSYM_STRUCTS["alignn_phsym_rows_args"], PHSYM_STRUCTS["alignn_phsym_fc_args"]
PHSYM_MAX_ATOMS = PHSYM.defines["ALIGNN_PHSYM_MAX_ATOMS"]
PHSYM_MAX_SITE_OPS = PHSYM.defines["ALIGNN_PHSYM_MAX_SITE_OPS"]


def _load_phsym():
    return _lib.bind(PHSYM)


def monkhorst_pack(kpts) -> np.ndarray:
    """ASE's monkhorst_pack: [(i, j, k) + 0.5] / kpts - 0.5 over np.indices(kpts) in C order -> [prod(kpts), 3]."""
    kpts = np.asarray(kpts, dtype=np.int64)
    return (np.indices(kpts).transpose((1, 2, 3, 0)).reshape((-1, 3)) + 0.5) / kpts - 0.5


def lattice_points(supercell) -> np.ndarray:
    """ASE's Phonons.lattice_vectors() with offset 0, as rows: cell (m0 N1 + m1) N2 + m2 -> R = ((m + N // 2) % N) - N // 2."""
    N = np.asarray(supercell, dtype=np.int64)[:, None]
    R = np.indices(tuple(int(x) for x in N[:, 0])).reshape(3, -1)
    return (((R + N // 2) % N) - N // 2).T.copy()


@dataclass
class PhononResult:
    """Per structure, in the input order: ``force_constants`` [Ncell, 3n, 3n] (eV/A^2, after the drift correction,
    ``symmetrize`` and ``acoustic``) belonging to ``lattice_points`` [Ncell, 3] (the centred cell offsets R);
    ``frequencies`` [K, 3n] (eV, ascending per q, imaginary modes negative) at ``qpoints``; ``modes`` [K, 3n, 3n] complex,
    column r the unit eigenvector of D(q) of frequency r (``modes=True``; ASE's ``band_structure(modes=True)`` returns these
    columns transposed and scaled by m^-1/2); ``dos_energies`` / ``dos_weights`` [dos_npts].  Unrequested outputs are None.
    ``n_evals``: model (or ``forces_fn``) calls; ``n_supercells``: displaced supercells evaluated (6n per structure; with
    ``displacements="symmetry"`` 2 D_b, and then ``displaced_atoms`` [D_b] int32 is the displaced atom of each direction,
    ascending, and ``directions`` [D_b, 3] its unit Cartesian direction - both None with ``displacements="all"``)."""

    force_constants: List[torch.Tensor]
    lattice_points: List[torch.Tensor]
    frequencies: Optional[List[torch.Tensor]]
    modes: Optional[List[torch.Tensor]]
    dos_energies: Optional[List[torch.Tensor]]
    dos_weights: Optional[List[torch.Tensor]]
    n_evals: int
    n_supercells: int
    _dyn: Optional[dict] = field(default=None, repr=False)
    displaced_atoms: Optional[List[torch.Tensor]] = None
    directions: Optional[List[torch.Tensor]] = None

    def frequencies_at(self, q, modes: bool = False):
        """Frequencies [K, 3n] per structure at more q-points ([K, 3] fractional), from the stored dynamical matrices (no
        evaluation); with ``modes``, (frequencies, modes)."""
        freqs, vecs = _eigh(self._dyn, _qpoints(q), modes)
        return (freqs, vecs) if modes else freqs


def _qpoints(q) -> np.ndarray:
    q = np.asarray(q.detach().cpu() if isinstance(q, torch.Tensor) else q, dtype=np.float64)
    if q.ndim != 2 or q.shape[1] != 3 or not np.all(np.isfinite(q)):
        raise ValueError(f"phonons: q-points must be a finite [K, 3] array, got shape {q.shape}")
    return q


def _eigh(dyn: dict, q: np.ndarray, modes: bool):
    """Frequencies (and modes) of the structures of ``dyn`` at q-points q [K, 3]: one alignn_phonon_eigh launch."""
    lib = _lib.load()
    dev, ms, B, K = dyn["device"], dyn["m"], len(dyn["m"]), q.shape[0]
    with _lib.device_guard(torch.empty(0, device=dev)):
        freq_off = np.concatenate([[0], np.cumsum([K * m for m in ms])]).astype(np.int64)
        mode_off = 2 * np.concatenate([[0], np.cumsum([K * m * m for m in ms])]).astype(np.int64)
        freqs = torch.empty(int(freq_off[-1]), dtype=torch.float64, device=dev)
        vecs = torch.empty(int(mode_off[-1]) // 2, dtype=torch.complex128, device=dev) if modes else None
        if K:
            q_d = torch.tensor(q, dtype=torch.float64, device=dev)
            fo = torch.tensor(freq_off, device=dev)
            mo = torch.tensor(mode_off, device=dev)
            status = torch.zeros(1, dtype=torch.int32, device=dev)
            _lib.check(lib.alignn_phonon_eigh(
                dyn["dyn"].data_ptr(), dyn["off"].data_ptr(), dyn["R"].data_ptr(), dyn["cell_ptr"].data_ptr(),
                dyn["dims"].data_ptr(), B, max(ms), q_d.data_ptr(), K, FREQ_SCALE, freqs.data_ptr(), fo.data_ptr(), None,
                None if vecs is None else torch.view_as_real(vecs).data_ptr(), mo.data_ptr(), status.data_ptr(), _lib.stream()),
                "phonon_eigh")
            if status.item() != 0:
                raise RuntimeError("phonons: the Jacobi eigensolver hit its sweep cap without converging")
        f_list = [freqs[freq_off[s]:freq_off[s + 1]].view(K, ms[s]) for s in range(B)]
        v_list = None
        if vecs is not None:
            v_list = [vecs[mode_off[s] // 2:mode_off[s + 1] // 2].view(K, ms[s], ms[s]) for s in range(B)]
    return f_list, v_list


def _supercells(supercell, B: int) -> List[tuple]:
    sc = np.asarray(supercell)
    if sc.shape == (3,):
        sc = np.broadcast_to(sc, (B, 3))
    if sc.shape != (B, 3) or not all(isinstance(v, numbers.Integral) or float(v).is_integer() for v in sc.reshape(-1)):
        raise ValueError(f"phonons: supercell must be (N1, N2, N3) or one per structure ({B}), got {supercell!r}")
    out = [tuple(int(v) for v in row) for row in sc]
    if any(v < 1 for row in out for v in row):
        raise ValueError(f"phonons: supercell sizes must be >= 1, got {supercell!r}")
    return out


def _plan(lib, sym: SymmetryResult, lat, dims, atom_ptr, ns: List[int], n_sc: List[int], dev) -> dict:
    """alignn_phsym_plan for the batch, and the one read-back (the directions per atom) that sizes the jobs: -> the plan's device
    arrays, ``slots`` [(structure, atom, direction)] in the order of the displaced pairs, ``slot_rows`` (the first row in g of
    each slot, and the total), ``reps`` / ``others`` [(structure, atom)]."""
    pk, N = sym.packed, sum(ns)
    G = pk["n_ops_total"]
    i32 = lambda *shape: torch.zeros(*shape, dtype=torch.int32, device=dev)
    f64 = lambda *shape: torch.zeros(*shape, dtype=torch.float64, device=dev)
    plan = dict(usable=i32(G), rot=f64(G, 9), rep=i32(N), n_site=i32(N), site_ops=i32(N, PHSYM_MAX_SITE_OPS), n_dir=i32(N),
                dirs=f64(N, 9), minv=f64(N, 9), dist_op=i32(N))
    args = PlanArgs(lattice=lat.data_ptr(), supercell=dims.data_ptr(), atom_ptr=atom_ptr.data_ptr(), op_ptr=pk["op_ptr"].data_ptr(),
                    map_ptr=pk["map_ptr"].data_ptr(), rotations=pk["rotations"].data_ptr(), atom_map=pk["atom_map"].data_ptr(),
                    n_ops_total=G, n_map_total=pk["n_map_total"], n_structs=len(ns), n_atoms=N,
                    **{k: v.data_ptr() for k, v in plan.items()})
    _lib.check(lib.alignn_phsym_plan(C.byref(args), _lib.stream()), "phsym_plan")
    n_dir = plan["n_dir"].cpu().numpy()
    ptr = np.concatenate([[0], np.cumsum(ns)])
    bad = [b for b in range(len(ns)) if (n_dir[ptr[b]:ptr[b + 1]] < 0).any()]
    if bad:
        raise ValueError(f"phonons: symmetry= does not describe structure(s) {bad}: no usable operation fixes a representative, "
                         f"a site group has more than {PHSYM_MAX_SITE_OPS} operations, or its arrays do not fit the structure")
    slots, rows, reps, others, r = [], [], [], [], 0
    for b, n in enumerate(ns):
        for a in range(n):
            k = int(n_dir[ptr[b] + a])
            (reps if k else others).append((b, a))
            for m in range(k):
                slots.append((b, a, m))
                rows.append(r)
                r += n_sc[b]
    plan.update(slots=slots, slot_rows=rows + [r], reps=reps, others=others)
    return plan


def _solve(lib, plan: dict, sym: SymmetryResult, g_rows, fc, fc_off, atom_ptr, dims, B: int, max_sc: int, dev) -> None:
    """alignn_phsym_solve for the representatives, then alignn_phsym_distribute for the other atoms."""
    pk = sym.packed
    first = {(b, a): plan["slot_rows"][x] for x, (b, a, m) in enumerate(plan["slots"]) if m == 0}
    reps_d = torch.tensor(plan["reps"], dtype=torch.int32, device=dev)
    rows_d = torch.tensor([first[r] for r in plan["reps"]], dtype=torch.int64, device=dev)
    common = dict(fc=fc.data_ptr(), fc_off=fc_off.data_ptr(), atom_ptr=atom_ptr.data_ptr(), supercell=dims.data_ptr(),
                  op_ptr=pk["op_ptr"].data_ptr(), map_ptr=pk["map_ptr"].data_ptr(), rotations=pk["rotations"].data_ptr(),
                  atom_map=pk["atom_map"].data_ptr(), shifts=pk["shifts"].data_ptr(), n_ops_total=pk["n_ops_total"],
                  n_map_total=pk["n_map_total"], n_structs=B, max_supercell_atoms=max_sc,
                  **{k: plan[k].data_ptr() for k in ("rot", "rep", "n_site", "site_ops", "n_dir", "dirs", "minv", "dist_op")})
    args = FcArgs(items=reps_d.data_ptr(), g_rows=rows_d.data_ptr(), g=g_rows.data_ptr(), n_items=len(plan["reps"]), **common)
    _lib.check(lib.alignn_phsym_solve(C.byref(args), _lib.stream()), "phsym_solve")
    if plan["others"]:
        others_d = torch.tensor(plan["others"], dtype=torch.int32, device=dev)
        args = FcArgs(items=others_d.data_ptr(), n_items=len(plan["others"]), **common)
        _lib.check(lib.alignn_phsym_distribute(C.byref(args), _lib.stream()), "phsym_distribute")


def repeat_symmetry(sym: SymmetryResult, P: int) -> SymmetryResult:
    """The SymmetryResult of every structure of ``sym`` P times in a row (entry s P + p holds the operations of structure s):
    for the P copies of each parent that differ by an isotropic strain, which changes no W, atom map, lattice shift or Cartesian
    rotation (``thermo.qha``)."""
    if not isinstance(sym, SymmetryResult) or not sym.packed:
        raise ValueError(f"repeat_symmetry: need the SymmetryResult of find_symmetry, got {type(sym).__name__}")
    idx = [s for s in range(len(sym.ns)) for _ in range(P)]
    dev = sym.packed["device"]
    ns, n_ops = [sym.ns[s] for s in idx], [sym.n_ops[s] for s in idx]
    rotations = torch.cat([sym.rotations[s] for s in idx]).contiguous()
    translations = torch.cat([sym.translations[s] for s in idx]).contiguous()
    atom_map = torch.cat([sym.atom_map[s].reshape(-1) for s in idx]).contiguous()
    shifts = torch.cat([sym.shifts[s].reshape(-1, 3) for s in idx]).contiguous()
    orbits = torch.cat([sym.orbits[s] for s in idx]).contiguous()
    ptr = np.concatenate([[0], np.cumsum(ns)])
    op_ptr = np.concatenate([[0], np.cumsum(n_ops)]).astype(np.int64)
    map_ptr = np.concatenate([[0], np.cumsum([g * n for g, n in zip(n_ops, ns)])]).astype(np.int64)
    B = len(idx)
    return SymmetryResult(
        rotations=[rotations[op_ptr[b]:op_ptr[b + 1]] for b in range(B)],
        translations=[translations[op_ptr[b]:op_ptr[b + 1]] for b in range(B)],
        atom_map=[atom_map[map_ptr[b]:map_ptr[b + 1]].view(n_ops[b], ns[b]) for b in range(B)],
        shifts=[shifts[map_ptr[b]:map_ptr[b + 1]].view(n_ops[b], ns[b], 3) for b in range(B)],
        orbits=[orbits[ptr[b]:ptr[b + 1]] for b in range(B)], n_ops=n_ops, n_translations=[sym.n_translations[s] for s in idx],
        point_group_order=[sym.point_group_order[s] for s in idx], crystal_system=[sym.crystal_system[s] for s in idx], ns=ns,
        symprec=sym.symprec,
        packed=dict(atom_ptr=torch.tensor(ptr, dtype=torch.int32, device=dev), op_ptr=torch.tensor(op_ptr, device=dev),
                    map_ptr=torch.tensor(map_ptr, device=dev), rotations=rotations, translations=translations, atom_map=atom_map,
                    shifts=shifts, n_ops_total=int(op_ptr[-1]), n_map_total=int(map_ptr[-1]), device=dev))


def _check_symmetry(symmetry, ns: List[int], scs: List[tuple], masses: Sequence) -> None:
    """The checks of ``displacements="symmetry"`` that need no launch: the SymmetryResult belongs to these structures, and the
    atoms that the usable operations (include/alignn_phsym.h, rule 1) make equivalent have equal masses."""
    if not isinstance(symmetry, SymmetryResult) or not symmetry.packed:
        raise ValueError("phonons: displacements='symmetry' needs symmetry=, the SymmetryResult of find_symmetry for these "
                         f"structures, got {type(symmetry).__name__}")
    if list(symmetry.ns) != list(ns):
        raise ValueError(f"phonons: symmetry= was found for structures of {list(symmetry.ns)} atoms, these have {list(ns)}")
    for b, (n, g) in enumerate(zip(ns, symmetry.n_ops)):
        if n > PHSYM_MAX_ATOMS:
            raise ValueError(f"phonons: structure {b} has {n} atoms; displacements='symmetry' takes at most {PHSYM_MAX_ATOMS}")
        if g < 1:
            raise ValueError(f"phonons: symmetry= holds no operation for structure {b}")
    rotations = host(symmetry.packed["rotations"]).reshape(-1, 3, 3).astype(np.int64)
    atom_map = host(symmetry.packed["atom_map"]).astype(np.int64)
    op0 = map0 = 0
    for b, (n, g) in enumerate(zip(ns, symmetry.n_ops)):
        N = np.asarray(scs[b], dtype=np.int64)
        W = rotations[op0:op0 + g]
        use = ((W * N[None, None, :]) % N[None, :, None] == 0).all(axis=(1, 2))
        amap = atom_map[map0:map0 + g * n].reshape(g, n)[use]
        op0, map0 = op0 + g, map0 + g * n
        if amap.size and (amap.min() < 0 or amap.max() >= n):
            raise ValueError(f"phonons: symmetry= maps atoms of structure {b} outside it")
        m = np.asarray(host(masses[b]), dtype=np.float64).reshape(-1)
        for row in amap:
            if not np.array_equal(m[row], m):
                i = int(np.nonzero(m[row] != m)[0][0])
                raise ValueError(f"phonons: atoms {i} and {int(row[i])} of structure {b} are equivalent by symmetry but have the "
                                 f"masses {m[i]} and {m[row[i]]}")


def phonons(model, lattices: Sequence, positions: Sequence, atom_features: Optional[Sequence], masses: Sequence, *,
            supercell=(2, 2, 2), delta: float = 0.01, drift: Optional[str] = "frederiksen", symmetrize: Optional[int] = 3,
            acoustic: bool = True, qpoints=None, modes: bool = False, dos_kpts=(20, 20, 20), dos_npts: int = 100,
            dos_width: float = 1e-3, max_atoms_per_eval: Optional[int] = None, intensive: bool = True,
            force_multiplier: float = 1.0, cutoff: float = 8.0, max_neighbors: int = 12, neighbor_strategy: str = "k-nearest",
            forces_fn: Optional[Callable] = None, device=None, displacements: str = "all",
            symmetry: Optional[SymmetryResult] = None) -> PhononResult:
    """Finite-displacement phonons of B crystals (primitive cells), ASE's ``Phonons(atoms, calc, supercell, delta)`` +
    ``run()`` + ``read(method, symmetrize, acoustic)`` + ``band_structure(qpoints)`` + ``get_dos(kpts).sample_grid(npts,
    width)`` for each structure.

    The structures, ``masses``, the model (or ``forces_fn``), ``force_multiplier``, ``cutoff`` ... ``neighbor_strategy`` and
    the device: alignn_amd/_structures.py; energies are not used (``intensive`` is accepted for symmetry with ``run_md``).
    ``forces_fn`` gets the S displaced supercells of one evaluation, their Cartesian positions unwrapped.

    ``supercell``: (N1, N2, N3) for all or one per structure; ``delta`` (A); ``drift``: "frederiksen" (ASE's default),
    "mean" (the mean force off every atom, ff.py:1175-1177) or None; ``symmetrize`` passes (0 / None: none, and no acoustic
    rule); ``acoustic``.  ``qpoints`` [K, 3] (fractional reciprocal coordinates): frequencies there (``modes``: eigenvectors
    too); ``dos_kpts`` (None: no DOS): the Monkhorst-Pack mesh of the DOS, sampled on ``dos_npts`` points with Gaussians of
    ``dos_width`` eV.  ``max_atoms_per_eval``: supercell atoms per evaluation (whole -/+ pairs; default
    ``MAX_ATOMS_PER_EVAL``).

    ``displacements``: "all" (every atom along x, y, z: 6n supercells per structure) or "symmetry", with ``symmetry`` the
    ``SymmetryResult`` of ``find_symmetry`` for these B structures (at most 32 atoms each): only the operations that map a
    structure's supercell onto itself are used; one atom per class under them is displaced, along 1 to 3 directions chosen so
    that their images under the atom's site group span space, still by -delta and +delta; the force constants of the
    representatives are solved from those forces and rotated onto the other atoms.  Atoms that the symmetry makes equivalent
    must have equal masses.  A structure with the identity alone gives the bits of "all"."""
    ns = check_inputs("phonons", model, lattices, positions, atom_features, masses, forces_fn=forces_fn)
    B = len(ns)
    scs = _supercells(supercell, B)
    if displacements not in DISPLACEMENTS:
        raise ValueError(f"phonons: displacements must be 'all' or 'symmetry', got {displacements!r}")
    by_symmetry = displacements == "symmetry"
    if by_symmetry:
        if symmetry is None:
            raise ValueError("phonons: displacements='symmetry' needs symmetry=, the SymmetryResult of find_symmetry")
        _check_symmetry(symmetry, ns, scs, masses)
    elif symmetry is not None:
        raise ValueError("phonons: symmetry= is only used with displacements='symmetry'")
    if not (isinstance(delta, numbers.Real) and np.isfinite(delta) and delta > 0):
        raise ValueError(f"phonons: delta must be a finite number > 0, got {delta!r}")
    if drift not in DRIFTS:
        raise ValueError(f"phonons: drift must be 'frederiksen', 'mean' or None, got {drift!r}")
    if symmetrize is None:
        symmetrize = 0
    if not isinstance(symmetrize, numbers.Integral) or symmetrize < 0:
        raise ValueError(f"phonons: symmetrize must be an int >= 0 or None, got {symmetrize!r}")
    q = None if qpoints is None else _qpoints(qpoints)
    if modes and q is None:
        raise ValueError("phonons: modes=True needs qpoints")
    mesh = None
    if dos_kpts is not None:
        k = np.asarray(dos_kpts)
        if k.shape != (3,) or not all(float(v).is_integer() and v >= 1 for v in k):
            raise ValueError(f"phonons: dos_kpts must be three ints >= 1 or None, got {dos_kpts!r}")
        if not (isinstance(dos_npts, numbers.Integral) and dos_npts >= 2):
            raise ValueError("phonons: dos_npts must be an int >= 2")
        if not (np.isfinite(dos_width) and dos_width > 0):
            raise ValueError("phonons: dos_width must be > 0")
        mesh = monkhorst_pack(k.astype(np.int64))
    if max_atoms_per_eval is None:
        max_atoms_per_eval = MAX_ATOMS_PER_EVAL
    if not (isinstance(max_atoms_per_eval, numbers.Integral) and max_atoms_per_eval >= 1):
        raise ValueError("phonons: max_atoms_per_eval must be an int >= 1")
    for i, n in enumerate(ns):
        if 3 * n > MAX_DIM:
            raise ValueError(f"phonons: structure {i} has {n} atoms; the eigen launch takes 3n <= {MAX_DIM} "
                             f"(at most {MAX_DIM // 3} atoms per primitive cell)")
    dev = gpu_device("phonons", model, forces_fn, device)
    if by_symmetry:
        index = lambda d: torch.cuda.current_device() if d.index is None else d.index
        if index(symmetry.packed["device"]) != index(dev):
            raise ValueError(f"phonons: symmetry= lives on {symmetry.packed['device']}, the phonons run on {dev}")
    lib = _load_phsym() if by_symmetry else _lib.load()

    ncell = [int(np.prod(c)) for c in scs]
    ms = [3 * n for n in ns]
    n_sc = [n * c for n, c in zip(ns, ncell)]
    with _lib.device_guard(torch.empty(0, device=dev)):
        packed = pack(lattices, positions, ns, dev, masses, frac=False)
        lat, pos, mass, atom_ptr = packed.lat, packed.pos, packed.mass, packed.atom_ptr
        dims = torch.tensor(scs, dtype=torch.int32, device=dev)
        super_lat = (lat * dims.to(torch.float64)[:, :, None]).contiguous()
        # (3 x 3 inverses on the host, one at a time: a structure's supercell coordinates do not depend on the batch)
        inv_super = torch.tensor(np.stack([np.linalg.inv(x) for x in super_lat.cpu().numpy()]), device=dev).contiguous()
        fc_off_h = np.concatenate([[0], np.cumsum([c * m * m for c, m in zip(ncell, ms)])]).astype(np.int64)
        fc_off = torch.tensor(fc_off_h, device=dev)
        fc = torch.zeros(int(fc_off_h[-1]), dtype=torch.float64, device=dev)
        # one lattice tensor per structure: every chunk hands neighbors the same objects, so its lattice tables stay cached
        lat_v = [super_lat[s] for s in range(B)]
        # (each structure's features once per supercell copy, in the order of the displaced supercells' rows)
        feats = None if forces_fn is not None else [torch.as_tensor(f).repeat(c, 1) for f, c in zip(atom_features, ncell)]
        evaluate = ForceEvaluator("phonons", model, forces_fn, feats, n_sc, dev, cutoff=cutoff, max_neighbors=max_neighbors,
                                  neighbor_strategy=neighbor_strategy, intensive=intensive, force_multiplier=force_multiplier,
                                  energies=False)

        # chunks of whole -/+ pairs, in (structure, row) order; by symmetry in (structure, representative, direction) order,
        # x the place of the pair's rows in g
        if by_symmetry:
            plan = _plan(lib, symmetry, lat, dims, atom_ptr, ns, n_sc, dev)
            pairs = [(s, x) for x, (s, _, _) in enumerate(plan["slots"])]
            g_rows = torch.empty(max(int(plan["slot_rows"][-1]), 1), 3, dtype=torch.float64, device=dev)
        else:
            pairs = [(s, x) for s in range(B) for x in range(ms[s])]
        chunks, cur, atoms = [], [], 0
        for s, x in pairs:
            need = 2 * n_sc[s]
            if cur and atoms + need > max_atoms_per_eval:
                chunks.append(cur)
                cur, atoms = [], 0
            cur.append((s, x))
            atoms += need
        chunks.append(cur)
        rows_max = max(sum(2 * n_sc[s] for s, _ in ch) for ch in chunks)
        frac = torch.empty(rows_max, 3, dtype=torch.float64, device=dev)
        cart = torch.empty(rows_max, 3, dtype=torch.float64, device=dev) if forces_fn is not None else None
        drift_code = DRIFTS[drift]
        for ch in chunks:
            jobs, row_off, pair_rows, r = [], [], [], 0
            for s, x in ch:
                pair_rows.append(r)
                for sg in (0, 1):
                    jobs.append(plan["slots"][x] + (sg,) if by_symmetry else (s, 2 * x + sg))
                    row_off.append(r)
                    r += n_sc[s]
            jobs_d = torch.tensor(jobs, dtype=torch.int32, device=dev)
            rows_d = torch.tensor(row_off, dtype=torch.int64, device=dev)
            if by_symmetry:
                args = DisplaceArgs(positions=pos.data_ptr(), atom_ptr=atom_ptr.data_ptr(), lattice=lat.data_ptr(),
                                    inv_supercell=inv_super.data_ptr(), supercell=dims.data_ptr(), dirs=plan["dirs"].data_ptr(),
                                    jobs=jobs_d.data_ptr(), row_off=rows_d.data_ptr(), frac=frac.data_ptr(), cart=_lib.ptr(cart),
                                    delta=float(delta), n_jobs=len(jobs), n_structs=B)
                _lib.check(lib.alignn_phsym_displace(C.byref(args), _lib.stream()), "phsym_displace")
            else:
                _lib.check(lib.alignn_phonon_displace(
                    pos.data_ptr(), atom_ptr.data_ptr(), lat.data_ptr(), inv_super.data_ptr(), dims.data_ptr(), jobs_d.data_ptr(),
                    rows_d.data_ptr(), len(jobs), float(delta), frac.data_ptr(), _lib.ptr(cart), _lib.stream()), "phonon_displace")
            which = [job[0] for job in jobs]
            views = [(o, o + n_sc[s]) for s, o in zip(which, row_off)]
            _, forces, _ = evaluate(which, [lat_v[s] for s in which], [frac[a:b] for a, b in views],
                                    None if cart is None else [cart[a:b] for a, b in views])
            prow_d = torch.tensor(pair_rows, dtype=torch.int64, device=dev)
            if by_symmetry:
                pairs_d = torch.tensor([plan["slots"][x][:2] for _, x in ch], dtype=torch.int32, device=dev)
                out_d = torch.tensor([plan["slot_rows"][x] for _, x in ch], dtype=torch.int64, device=dev)
                args = RowsArgs(forces=forces.data_ptr(), pairs=pairs_d.data_ptr(), pair_rows=prow_d.data_ptr(),
                                out_rows=out_d.data_ptr(), atom_ptr=atom_ptr.data_ptr(), supercell=dims.data_ptr(),
                                g=g_rows.data_ptr(), delta=float(delta), drift=drift_code, n_pairs=len(ch), n_structs=B)
                _lib.check(lib.alignn_phsym_rows(C.byref(args), _lib.stream()), "phsym_rows")
            else:
                pairs_d = torch.tensor(ch, dtype=torch.int32, device=dev)
                _lib.check(lib.alignn_phonon_fc_rows(
                    forces.data_ptr(), pairs_d.data_ptr(), prow_d.data_ptr(), len(ch), atom_ptr.data_ptr(), dims.data_ptr(),
                    fc_off.data_ptr(), drift_code, float(delta), fc.data_ptr(), _lib.stream()), "phonon_fc_rows")
        if by_symmetry:
            _solve(lib, plan, symmetry, g_rows, fc, fc_off, atom_ptr, dims, B, max(n_sc), dev)

        max_elems = int(max(c * m * m for c, m in zip(ncell, ms)))
        other = torch.empty_like(fc)
        for _ in range(int(symmetrize)):
            _lib.check(lib.alignn_phonon_symmetrize(fc.data_ptr(), other.data_ptr(), atom_ptr.data_ptr(), dims.data_ptr(),
                                                    fc_off.data_ptr(), B, max_elems, _lib.stream()), "phonon_symmetrize")
            fc, other = other, fc
            if not acoustic:
                break
            _lib.check(lib.alignn_phonon_acoustic(fc.data_ptr(), atom_ptr.data_ptr(), dims.data_ptr(), fc_off.data_ptr(), B,
                                                  max(ns), _lib.stream()), "phonon_acoustic")
        dyn = other  # (the spare buffer)
        _lib.check(lib.alignn_phonon_mass_weight(fc.data_ptr(), dyn.data_ptr(), mass.data_ptr(), atom_ptr.data_ptr(),
                                                 dims.data_ptr(), fc_off.data_ptr(), B, max_elems, _lib.stream()),
                   "phonon_mass_weight")
        R_h = [lattice_points(c) for c in scs]
        R = torch.tensor(np.concatenate(R_h), dtype=torch.int32, device=dev)
        cell_ptr = torch.tensor(np.concatenate([[0], np.cumsum(ncell)]), dtype=torch.int32, device=dev)
        state = dict(device=dev, m=ms, dyn=dyn, off=fc_off, R=R, cell_ptr=cell_ptr, dims=torch.tensor(ms, dtype=torch.int32,
                                                                                                          device=dev))
        freqs = vecs = dos_e = dos_w = None
        if q is not None:
            freqs, vecs = _eigh(state, q, modes)
        if mesh is not None:
            mesh_f, _ = _eigh(state, mesh, False)
            K = mesh.shape[0]
            f_off = torch.tensor(np.concatenate([[0], np.cumsum([K * m for m in ms])]), dtype=torch.int64, device=dev)
            flat = torch.cat([f.reshape(-1) for f in mesh_f]).contiguous()
            energies = torch.empty(B, dos_npts, dtype=torch.float64, device=dev)
            weights = torch.empty(B, dos_npts, dtype=torch.float64, device=dev)
            _lib.check(lib.alignn_phonon_dos(flat.data_ptr(), f_off.data_ptr(), B, int(dos_npts), float(dos_width),
                                             energies.data_ptr(), weights.data_ptr(), _lib.stream()), "phonon_dos")
            dos_e, dos_w = list(energies.unbind(0)), list(weights.unbind(0))
        fcs = [fc[fc_off_h[s]:fc_off_h[s + 1]].view(ncell[s], ms[s], ms[s]) for s in range(B)]
        Rs = [torch.as_tensor(r) for r in R_h]
        atoms = dirs = None
        if by_symmetry:
            dirs_h = plan["dirs"].cpu().numpy().reshape(-1, 3, 3)
            ptr = np.concatenate([[0], np.cumsum(ns)])
            per = [[] for _ in range(B)]
            for s, a, m in plan["slots"]:
                per[s].append((a, m))
            atoms = [torch.tensor([a for a, _ in p], dtype=torch.int32) for p in per]
            dirs = [torch.tensor(np.array([dirs_h[ptr[b] + a, m] for a, m in p]).reshape(-1, 3)) for b, p in enumerate(per)]
        return PhononResult(force_constants=fcs, lattice_points=Rs, frequencies=freqs, modes=vecs, dos_energies=dos_e,
                            dos_weights=dos_w, n_evals=len(chunks), n_supercells=2 * len(pairs), _dyn=state,
                            displaced_atoms=atoms, directions=dirs)
