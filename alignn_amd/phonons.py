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
"""

from __future__ import annotations

import numbers
from dataclasses import dataclass, field
from typing import Callable, List, Optional, Sequence

import numpy as np
import torch

from . import _lib
from ._structures import ForceEvaluator, check_inputs, gpu_device, pack

__all__ = ["phonons", "PhononResult", "EV_TO_THZ", "EV_TO_CM1", "MAX_DIM", "monkhorst_pack", "lattice_points"]

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
    ``n_evals``: model (or ``forces_fn``) calls; ``n_supercells``: displaced supercells evaluated (6n per structure)."""

    force_constants: List[torch.Tensor]
    lattice_points: List[torch.Tensor]
    frequencies: Optional[List[torch.Tensor]]
    modes: Optional[List[torch.Tensor]]
    dos_energies: Optional[List[torch.Tensor]]
    dos_weights: Optional[List[torch.Tensor]]
    n_evals: int
    n_supercells: int
    _dyn: Optional[dict] = field(default=None, repr=False)

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


def phonons(model, lattices: Sequence, positions: Sequence, atom_features: Optional[Sequence], masses: Sequence, *,
            supercell=(2, 2, 2), delta: float = 0.01, drift: Optional[str] = "frederiksen", symmetrize: Optional[int] = 3,
            acoustic: bool = True, qpoints=None, modes: bool = False, dos_kpts=(20, 20, 20), dos_npts: int = 100,
            dos_width: float = 1e-3, max_atoms_per_eval: Optional[int] = None, intensive: bool = True,
            force_multiplier: float = 1.0, cutoff: float = 8.0, max_neighbors: int = 12, neighbor_strategy: str = "k-nearest",
            forces_fn: Optional[Callable] = None, device=None) -> PhononResult:
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
    ``MAX_ATOMS_PER_EVAL``)."""
    ns = check_inputs("phonons", model, lattices, positions, atom_features, masses, forces_fn=forces_fn)
    B = len(ns)
    scs = _supercells(supercell, B)
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
    lib = _lib.load()

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

        # chunks of whole -/+ pairs, in (structure, row) order
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
                    jobs.append((s, 2 * x + sg))
                    row_off.append(r)
                    r += n_sc[s]
            jobs_d = torch.tensor(jobs, dtype=torch.int32, device=dev)
            rows_d = torch.tensor(row_off, dtype=torch.int64, device=dev)
            _lib.check(lib.alignn_phonon_displace(
                pos.data_ptr(), atom_ptr.data_ptr(), lat.data_ptr(), inv_super.data_ptr(), dims.data_ptr(), jobs_d.data_ptr(),
                rows_d.data_ptr(), len(jobs), float(delta), frac.data_ptr(), _lib.ptr(cart), _lib.stream()), "phonon_displace")
            which = [s for s, _ in jobs]
            views = [(o, o + n_sc[s]) for s, o in zip(which, row_off)]
            _, forces, _ = evaluate(which, [lat_v[s] for s in which], [frac[a:b] for a, b in views],
                                    None if cart is None else [cart[a:b] for a, b in views])
            pairs_d = torch.tensor(ch, dtype=torch.int32, device=dev)
            prow_d = torch.tensor(pair_rows, dtype=torch.int64, device=dev)
            _lib.check(lib.alignn_phonon_fc_rows(
                forces.data_ptr(), pairs_d.data_ptr(), prow_d.data_ptr(), len(ch), atom_ptr.data_ptr(), dims.data_ptr(),
                fc_off.data_ptr(), drift_code, float(delta), fc.data_ptr(), _lib.stream()), "phonon_fc_rows")

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
        return PhononResult(force_constants=fcs, lattice_points=Rs, frequencies=freqs, modes=vecs, dos_energies=dos_e,
                            dos_weights=dos_w, n_evals=len(chunks), n_supercells=sum(2 * m for m in ms), _dyn=state)
