"""Batched harmonic thermodynamics and the quasi-harmonic approximation, on the device.

The reference's phonon paths end where phonopy takes over on the host: ``phonons3`` (alignn/ff/ff.py) asks phono3py for
properties on ``range(0, 1001, 10)`` K, and a user of ``ev_curve`` and ``ase_phonon`` who wants the thermal expansion loops over
volumes, runs phonopy's ``run_thermal_properties`` at each and hands the free energies to phonopy-qha.  Here, for B crystals
together:

``thermal_properties`` takes a ``PhononResult``: the frequencies of all structures on a Monkhorst-Pack mesh
(``PhononResult.frequencies_at``: one eigen launch), then ``alignn_phonon_thermal`` (csrc/thermo.hip): the sums over (q, mode)
of the free energy, internal energy, entropy and heat capacity at every temperature, one workgroup per (chunk of 1024
frequencies, structure) with the frequencies in registers and a loop over the temperatures.

``qha`` strings the drivers together: (1) the B P strained cells of ``ev_curve`` (``alignn_strain_build``); (2) E(V) by
``relax`` in groups of whole jobs (``steps=0``, or FIRE at the fixed cell with ``relax_ions``); (3) ONE ``phonons`` call on all
B P strained structures; (4) ``thermal_properties``; (5) ONE ``alignn_eos_fit`` launch on the B NT curves E(V) + F(V, T); (6)
``alignn_qha_derive``: thermal expansion, Cv, S, C_p and the Grueneisen parameter at the fitted volumes.

The kernels are float64 with fixed-order sums whose order depends on a structure's own data only, and ``relax`` and ``phonons``
keep a structure's bits independent of its batch, so a crystal's numbers are the same whatever else is in the call.
tests/thermo_ref.py restates the sums and the reduction in numpy.  The entry points are declared in include/alignn_thermo.h,
read here with the reader of alignn_amd/_abi.py.
"""

from __future__ import annotations

import numbers
from dataclasses import dataclass
from typing import Callable, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _abi, _lib
from ._jobs import (EVALUATION, MAX_ATOMS_PER_CALL, check_max_atoms, check_steps_fmax, evaluation_options, features,
                    prepare_parents, relax_jobs, strain_jobs)
from ._structures import EV_A3_TO_GPA, check_inputs, gpu_device
from .eos import EOS_FORMS, MAX_POINTS, MIN_POINTS, _check_dx, eos_fit
from .phonons import DISPLACEMENTS, MAX_DIM, PhononResult, _supercells, monkhorst_pack, phonons, repeat_symmetry

__all__ = ["thermal_sums", "thermal_properties", "qha", "ThermalResult", "QHAResult", "KB"]

KB = 1.38064852e-23 / 1.6021766208e-19  # eV/K, CODATA 2014: the unit set of alignn_amd/phonons.py (and the kernel's constant)
H = _abi.header("alignn_thermo.h")  # (it declares no structs)
HEADER, SIGNATURES = H.path, H.signatures
DEFAULT_TEMPERATURES = np.arange(0, 1001, 10)  # K: the reference's ``phonons3`` asks for these
DEFAULT_DX = np.arange(-0.05, 0.05, 0.01)  # the reference's ``ev_curve`` strains
# ``qha`` has a ``cutoff`` of its own (the mode cutoff, eV), so the neighbour cutoff of the evaluations cannot be passed through it
_EVALUATION = tuple(k for k in EVALUATION if k != "cutoff")
_ION_RELAXATION = ("steps", "fmax")


def _load():
    return _lib.bind(H)


@dataclass
class ThermalResult:
    """Per structure s of the ``PhononResult``, per primitive cell.  ``free_energy`` (eV), ``internal_energy`` (eV), ``entropy``
    (eV/K) and ``heat_capacity`` (Cv, eV/K) are [B, NT] float64 tensors on the device at ``temperatures`` [NT] (K);
    ``zero_point_energy`` [B] (eV).  ``n_modes[s]`` is the number of mesh modes (q-points x 3n) and ``n_skipped[s]`` how many of
    them were not counted: the imaginary ones (negative frequencies), the zero ones and every one at or below ``cutoff``."""

    temperatures: np.ndarray  # [NT]
    free_energy: torch.Tensor  # [B, NT]
    internal_energy: torch.Tensor
    entropy: torch.Tensor
    heat_capacity: torch.Tensor
    zero_point_energy: torch.Tensor  # [B]
    n_modes: np.ndarray  # [B] int
    n_skipped: np.ndarray  # [B] int


@dataclass
class QHAResult:
    """Per parent s, in the input order.  ``volumes[s, p]`` (A^3), ``energies[s, p]`` (eV) and ``phonon_free_energy[s, p, i]``
    (eV per cell) are those of the parent strained by ``dx[p]``, the last at ``temperatures[i]`` (K).  Per temperature, [B, NT],
    from the fit of E(V) + F(V, T_i): ``gibbs`` (its minimum, eV: the Gibbs energy at zero pressure), ``volume`` (A^3),
    ``bulk_modulus`` (isothermal, eV/A^3; ``bulk_modulus_GPa = bulk_modulus * 160.21766208``), ``bp`` (its pressure
    derivative) and ``fit_status`` (0 converged, 1 stopped after 100 steps, 2 no fit: NaN); from the reduction:
    ``thermal_expansion`` (volumetric, 1/K; central differences of ``volume``, one-sided at the two ends), ``heat_capacity_v``
    and ``entropy`` (eV/K, at ``volume``), ``heat_capacity_p`` (eV/K), ``gruneisen`` (alpha B V / Cv, NaN where Cv = 0, as at
    0 K) and ``inside``: whether ``volume`` lies within the strained volumes; outside the numbers are extrapolations.
    ``n_skipped[s, p]``: the mesh modes not counted (imaginary, zero or below ``cutoff``) at that volume - never an error, but
    a free energy that leaves modes out is not the crystal's.  ``converged`` those of the ion relaxations (``relax_ions``).
    ``lattices`` / ``positions`` are the parents the curve was taken on (the relaxed ones with ``on_relaxed_struct``),
    ``n_eval_calls`` the batched evaluation calls of E(V), ``n_phonon_evals`` those of the displaced supercells."""

    dx: np.ndarray  # [P]
    temperatures: np.ndarray  # [NT]
    volumes: np.ndarray  # [B, P]
    energies: np.ndarray  # [B, P]
    phonon_free_energy: np.ndarray  # [B, P, NT]
    gibbs: np.ndarray  # [B, NT]
    volume: np.ndarray
    bulk_modulus: np.ndarray
    bulk_modulus_GPa: np.ndarray
    bp: np.ndarray
    thermal_expansion: np.ndarray
    heat_capacity_v: np.ndarray
    heat_capacity_p: np.ndarray
    entropy: np.ndarray
    gruneisen: np.ndarray
    fit_status: np.ndarray  # [B, NT] int
    inside: np.ndarray  # [B, NT] bool
    n_skipped: np.ndarray  # [B, P] int
    converged: np.ndarray  # [B, P] bool
    lattices: torch.Tensor  # [B, 3, 3] float64
    positions: List[torch.Tensor]  # [n_s, 3] float64
    n_eval_calls: int
    n_phonon_evals: int


# --- checks (host) -----------------------------------------------------------------------------------------------------------------
def _check_temperatures(who: str, temperatures, increasing: bool = False) -> np.ndarray:
    if isinstance(temperatures, torch.Tensor):
        temperatures = temperatures.detach().cpu().numpy()
    try:
        t = np.asarray(temperatures, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError(f"{who}: temperatures must be a 1-D array of kelvins, got {temperatures!r}") from None
    if t.ndim != 1 or len(t) < 1:
        raise ValueError(f"{who}: temperatures must be 1-D with at least one entry, got shape {t.shape}")
    if not (np.isfinite(t).all() and (t >= 0).all()):
        raise ValueError(f"{who}: temperatures must be finite and >= 0 K")
    if increasing and not (np.diff(t) > 0).all():
        raise ValueError(f"{who}: temperatures must be strictly increasing (the thermal expansion is a difference along them)")
    return t


def _check_mesh(who: str, mesh) -> Tuple[int, int, int]:
    m = np.asarray(mesh)
    if m.shape != (3,) or not all(isinstance(v, numbers.Real) and float(v).is_integer() and v >= 1 for v in m.tolist()):
        raise ValueError(f"{who}: mesh must be three ints >= 1, got {mesh!r}")
    return tuple(int(v) for v in m)


def _check_cutoff(who: str, cutoff) -> float:
    if not (isinstance(cutoff, numbers.Real) and np.isfinite(cutoff) and cutoff >= 0):
        raise ValueError(f"{who}: cutoff must be a finite number >= 0 (eV), got {cutoff!r}")
    return float(cutoff)


# --- the launches ------------------------------------------------------------------------------------------------------------------
def thermal_sums(freqs: torch.Tensor, freq_off, n_q, temperatures, cutoff: float = 0.0) -> Tuple[torch.Tensor, ...]:
    """The sums launch alone: ``freqs`` the flat float64 mesh frequencies (eV) of B structures on the GPU, structure s owning
    ``freqs[freq_off[s]:freq_off[s + 1]]`` (``freq_off`` [B + 1] ints, 0 first; the layout ``alignn_phonon_dos`` takes), ``n_q``
    the number of q-points (one int, or one per structure), ``temperatures`` [NT] (K), ``cutoff`` (eV) -> (F, U, S, Cv [B, NT],
    zpe [B] float64, n_skipped [B] int32) on the device, as ``ThermalResult`` describes them."""
    who = "thermal_sums"
    if not isinstance(freqs, torch.Tensor) or freqs.ndim != 1:
        raise ValueError(f"{who}: freqs must be a flat tensor")
    off = np.asarray(freq_off.detach().cpu() if isinstance(freq_off, torch.Tensor) else freq_off)
    if off.ndim != 1 or len(off) < 2 or not np.issubdtype(off.dtype, np.integer):
        raise ValueError(f"{who}: freq_off must be [B + 1] ints with B >= 1, got shape {off.shape} of {off.dtype}")
    off = off.astype(np.int64)
    B = len(off) - 1
    if off[0] != 0 or (np.diff(off) < 0).any() or off[-1] > freqs.numel():
        raise ValueError(f"{who}: freq_off must start at 0, not decrease and end within the {freqs.numel()} frequencies")
    if B > 65535:
        raise ValueError(f"{who}: at most 65535 structures per launch, got {B}")
    nq = np.asarray(n_q)
    if nq.ndim == 0:
        nq = np.full(B, nq)
    if nq.shape != (B,) or not np.issubdtype(nq.dtype, np.integer) or (nq < 1).any():
        raise ValueError(f"{who}: n_q must be an int >= 1 or one per structure ({B}), got {n_q!r}")
    if (np.diff(off) % nq != 0).any():
        raise ValueError(f"{who}: every structure's frequencies must be n_q q-points of equally many modes")
    t = _check_temperatures(who, temperatures)
    cutoff = _check_cutoff(who, cutoff)
    if freqs.dtype != torch.float64 or not freqs.is_cuda:
        raise TypeError(f"{who}: freqs must be a float64 tensor on the GPU, got {freqs.dtype} on {freqs.device}")
    NT, dev = len(t), freqs.device
    lib = _load()
    with _lib.device_guard(freqs):
        freqs = freqs.contiguous()
        off_d = torch.tensor(off, dtype=torch.int64, device=dev)
        nq_d = torch.tensor(nq.astype(np.int32), dtype=torch.int32, device=dev)
        t_d = torch.tensor(t, dtype=torch.float64, device=dev)
        max_freqs = int(np.diff(off).max())
        ws_bytes = lib.alignn_phonon_thermal_workspace(B, max_freqs, NT)
        ws = torch.empty(ws_bytes // 8, dtype=torch.float64, device=dev)
        F, U, S, Cv = (torch.empty(B, NT, dtype=torch.float64, device=dev) for _ in range(4))
        zpe = torch.empty(B, dtype=torch.float64, device=dev)
        n_skipped = torch.empty(B, dtype=torch.int32, device=dev)
        _lib.check(lib.alignn_phonon_thermal(freqs.data_ptr(), off_d.data_ptr(), nq_d.data_ptr(), B, max_freqs, t_d.data_ptr(),
                                             NT, cutoff, ws.data_ptr(), ws_bytes, F.data_ptr(), U.data_ptr(), S.data_ptr(),
                                             Cv.data_ptr(), zpe.data_ptr(), n_skipped.data_ptr(), _lib.stream()), "phonon_thermal")
    return F, U, S, Cv, zpe, n_skipped


def qha_derive(volumes: torch.Tensor, heat_capacity: torch.Tensor, entropy: torch.Tensor, temperatures: torch.Tensor,
               v_eq: torch.Tensor, b_t: torch.Tensor, status: torch.Tensor) -> Tuple[torch.Tensor, ...]:
    """The reduction launch alone, on float64 tensors on the GPU: ``volumes`` [B, P] (4 <= P <= 64), ``heat_capacity`` and
    ``entropy`` [B, P, NT], ``temperatures`` [NT], the fits' ``v_eq`` and ``b_t`` [B, NT] and ``status`` [B, NT] int32 ->
    (alpha, cv, s, cp, gamma [B, NT] float64, inside [B, NT] int32) on the device, as ``QHAResult`` describes them."""
    who = "qha_derive"
    if volumes.ndim != 2 or not MIN_POINTS <= volumes.shape[1] <= MAX_POINTS:
        raise ValueError(f"{who}: volumes must be [B, P] with {MIN_POINTS} <= P <= {MAX_POINTS}, got {tuple(volumes.shape)}")
    B, P = volumes.shape
    if temperatures.ndim != 1 or len(temperatures) < 1:
        raise ValueError(f"{who}: temperatures must be [NT] with NT >= 1, got {tuple(temperatures.shape)}")
    NT = len(temperatures)
    if B > 65535:
        raise ValueError(f"{who}: at most 65535 structures per launch, got {B}")
    for name, t, shape, dtype in (("volumes", volumes, (B, P), torch.float64), ("heat_capacity", heat_capacity, (B, P, NT), torch.float64),
                                  ("entropy", entropy, (B, P, NT), torch.float64), ("temperatures", temperatures, (NT,), torch.float64),
                                  ("v_eq", v_eq, (B, NT), torch.float64), ("b_t", b_t, (B, NT), torch.float64),
                                  ("status", status, (B, NT), torch.int32)):
        if tuple(t.shape) != shape:
            raise ValueError(f"{who}: {name} must be {list(shape)}, got {tuple(t.shape)}")
        if t.dtype != dtype or not t.is_cuda or t.device != volumes.device:
            raise TypeError(f"{who}: {name} must be a {dtype} tensor on {volumes.device}, got {t.dtype} on {t.device}")
    dev = volumes.device
    lib = _load()
    with _lib.device_guard(volumes):
        ins = [t.contiguous() for t in (volumes, heat_capacity, entropy, temperatures, v_eq, b_t, status)]
        alpha, cv, s, cp, gamma = (torch.empty(B, NT, dtype=torch.float64, device=dev) for _ in range(5))
        inside = torch.empty(B, NT, dtype=torch.int32, device=dev)
        _lib.check(lib.alignn_qha_derive(*[t.data_ptr() for t in ins], B, P, NT, alpha.data_ptr(), cv.data_ptr(), s.data_ptr(),
                                         cp.data_ptr(), gamma.data_ptr(), inside.data_ptr(), _lib.stream()), "qha_derive")
    return alpha, cv, s, cp, gamma, inside


# --- the drivers -------------------------------------------------------------------------------------------------------------------
def thermal_properties(result: PhononResult, temperatures=DEFAULT_TEMPERATURES, *, mesh=(20, 20, 20),
                       cutoff: float = 0.0) -> ThermalResult:
    """Harmonic thermodynamics of the B structures of a ``phonons`` result, phonopy's ``run_mesh(mesh)`` +
    ``run_thermal_properties`` for each: the frequencies on the Monkhorst-Pack ``mesh`` from the stored dynamical matrices (no
    evaluation), then the mode sums at ``temperatures`` (K, finite and >= 0).  A mode counts only if its frequency is above
    ``cutoff`` (eV; phonopy's ``cutoff_frequency``); the others are counted in ``n_skipped``.  Per primitive cell, in eV and
    eV/K (phonopy reports kJ/mol and J/K/mol)."""
    who = "thermal_properties"
    if not isinstance(result, PhononResult) or result._dyn is None:
        raise ValueError(f"{who}: needs the PhononResult of a phonons call")
    t = _check_temperatures(who, temperatures)
    mesh = _check_mesh(who, mesh)
    cutoff = _check_cutoff(who, cutoff)
    # (row-major: ``monkhorst_pack`` returns a column-major array, and the eigen launch reads the q-points' storage as [K][3])
    q = np.ascontiguousarray(monkhorst_pack(mesh))
    K = len(q)
    freqs = result.frequencies_at(q)
    ms = [int(f.shape[1]) for f in freqs]
    off = np.concatenate([[0], np.cumsum([K * m for m in ms])]).astype(np.int64)
    with _lib.device_guard(freqs[0]):
        flat = torch.cat([f.reshape(-1) for f in freqs]).contiguous()
        F, U, S, Cv, zpe, n_skipped = thermal_sums(flat, off, K, t, cutoff)
        skipped = n_skipped.cpu().numpy().astype(np.int64)
    return ThermalResult(temperatures=t, free_energy=F, internal_energy=U, entropy=S, heat_capacity=Cv, zero_point_energy=zpe,
                         n_modes=np.array([K * m for m in ms], dtype=np.int64), n_skipped=skipped)


def qha(model, lattices: Sequence, positions: Sequence, atom_features: Optional[Sequence], masses: Sequence, *,
        dx=DEFAULT_DX, temperatures=DEFAULT_TEMPERATURES, eos: str = "murnaghan", supercell=(2, 2, 2), delta: float = 0.01,
        mesh=(20, 20, 20), cutoff: float = 0.0, relax_ions: bool = False, on_relaxed_struct: bool = False,
        max_atoms_per_call: int = MAX_ATOMS_PER_CALL, max_atoms_per_eval: Optional[int] = None,
        forces_fn: Optional[Callable] = None, device=None, displacements: str = "all", symmetry=None,
        **relax_kwargs) -> QHAResult:
    """The quasi-harmonic approximation at zero pressure for B crystals (primitive cells): every parent strained isotropically
    by each ``dx[p]`` as ``ev_curve`` does, E(V) and the phonons of all B P strained structures evaluated together, E(V) +
    F_phonon(V, T) fitted at every temperature, and the fits reduced to the thermal quantities of ``QHAResult`` - what a loop
    over volumes around ``ase_phonon``, phonopy's thermal properties and phonopy-qha gives for one crystal.

    The structures, ``masses``, the model (or ``forces_fn``) and the device: alignn_amd/_structures.py.  ``dx``, ``eos``,
    ``on_relaxed_struct`` and ``max_atoms_per_call``: ``ev_curve``.  ``temperatures`` (K): finite, >= 0, strictly increasing.
    ``supercell``, ``delta``, ``max_atoms_per_eval``, ``displacements`` and ``symmetry``: ``phonons`` (its other options at
    their defaults; 3n <= 96).  ``symmetry`` is the ``SymmetryResult`` of the B parents: the strains are isotropic, so every
    strained copy of a parent has the parent's operations, and with ``displacements="symmetry"`` every volume evaluates only
    the symmetry-inequivalent displacements (a relaxation that breaks the parents' symmetry is the caller's to exclude).
    ``mesh`` and ``cutoff`` (eV, the mode cutoff): ``thermal_properties``.

    ``relax_ions``: relax the atoms of every strained structure at its fixed cell before its energy and phonons are taken
    (``steps`` and ``fmax`` from ``relax_kwargs``); without it the ions follow the strain affinely, which is the whole answer
    only where the positions have no free parameter.  Without ``on_relaxed_struct`` and ``relax_ions``, ``relax_kwargs`` may
    only hold the evaluation options ``max_neighbors``, ``neighbor_strategy``, ``intensive`` and ``force_multiplier``, which
    reach every evaluation in all cases (the neighbour cutoff of the evaluations is the default one: ``cutoff`` here is the
    mode cutoff).

    Imaginary modes are counted in ``n_skipped`` and are never an error; a fit need not have its minimum inside the strains
    (``fit_status``, ``inside``).  The curves are returned whatever the fits say."""
    who = "qha"
    for name, v in (("on_relaxed_struct", on_relaxed_struct), ("relax_ions", relax_ions)):
        if not isinstance(v, (bool, np.bool_)):
            raise ValueError(f"{who}: {name} is one bool, got {type(v).__name__}")
    optimize_lattice = bool(on_relaxed_struct) and bool(relax_kwargs.get("optimize_lattice", True))
    ns = check_inputs(who, model, lattices, positions, atom_features, masses, forces_fn=forces_fn, stress=optimize_lattice)
    B = len(ns)
    if displacements not in DISPLACEMENTS:
        raise ValueError(f"{who}: displacements must be 'all' or 'symmetry', got {displacements!r}")
    if (displacements == "symmetry") != (symmetry is not None):
        raise ValueError(f"{who}: displacements='symmetry' and symmetry= (the SymmetryResult of the parents) go together")
    if symmetry is not None and list(getattr(symmetry, "ns", [])) != list(ns):
        raise ValueError(f"{who}: symmetry= must be the SymmetryResult of find_symmetry for these {B} structures")
    d = _check_dx(who, dx)
    P = len(d)
    t = _check_temperatures(who, temperatures, increasing=True)
    NT = len(t)
    if eos not in EOS_FORMS:
        raise ValueError(f"{who}: eos must be one of {sorted(EOS_FORMS)}, got {eos!r}")
    mesh = _check_mesh(who, mesh)
    cutoff = _check_cutoff(who, cutoff)
    for i, n in enumerate(ns):
        if 3 * n > MAX_DIM:
            raise ValueError(f"{who}: structure {i} has {n} atoms; the eigen launch takes 3n <= {MAX_DIM} "
                             f"(at most {MAX_DIM // 3} atoms per primitive cell)")
    try:
        scs = [sc for sc in _supercells(supercell, B) for _ in range(P)]  # job s P + p has the supercell of parent s
    except ValueError as e:
        raise ValueError(f"{who}: {e}") from None
    if B * P > 65535:
        raise ValueError(f"{who}: at most 65535 strained structures per call, got {B} x {P}")
    check_max_atoms(who, max_atoms_per_call)
    evaluation = evaluation_options(who, relax_kwargs, _EVALUATION, on_relaxed_struct, _ION_RELAXATION if relax_ions else ())
    check_steps_fmax(who, relax_kwargs)
    job_kw = dict(evaluation, optimize_lattice=optimize_lattice)
    if relax_ions:
        job_kw.update({k: v for k, v in relax_kwargs.items() if k in _ION_RELAXATION})
        if optimize_lattice:
            job_kw["cell_mask"] = np.zeros(6)  # the cell stays
    dev = gpu_device(who, model, forces_fn, device)

    with _lib.device_guard(torch.empty(0, device=dev)):
        packed, lat_out, pos_out = prepare_parents(model, lattices, positions, atom_features, ns, on_relaxed_struct, relax_kwargs,
                                                   forces_fn, dev)
        scale = torch.tensor(1.0 + d, dtype=torch.float64, device=dev)  # (1 + dx in float64, as ev_curve takes it)
        cells, cart, volumes, src, counts = strain_jobs(
            packed, ns, scale[:, None, None] * torch.eye(3, dtype=torch.float64, device=dev), dev)
        feats_all = features(atom_features, forces_fn, dev)
        r = relax_jobs(model, cells, cart, src, counts, feats_all, max_atoms_per_call, bool(relax_ions), job_kw, forces_fn, dev)
        volumes, energies = volumes.reshape(B, P), r.energies.reshape(B, P).contiguous()

        # one phonons call on the B P strained (ion-relaxed) structures: job s P + p has the features and masses of parent s
        job_feats = None if feats_all is None else list(torch.split(feats_all[src.long()], counts))
        job_masses = [torch.as_tensor(masses[s]) for s in range(B) for _ in range(P)]
        # (clamped ions: the strained structures as built; relaxed ions: as ``relax`` left them, the cells unchanged)
        job_pos = r.positions if relax_ions else list(torch.split(cart, counts))
        ph = phonons(model, list(cells), job_pos, job_feats, job_masses, supercell=scs, delta=delta, qpoints=None,
                     dos_kpts=None, max_atoms_per_eval=max_atoms_per_eval, forces_fn=forces_fn, device=dev,
                     displacements=displacements, symmetry=None if symmetry is None else repeat_symmetry(symmetry, P),
                     **evaluation)
        th = thermal_properties(ph, t, mesh=mesh, cutoff=cutoff)
        F = th.free_energy.view(B, P, NT)

        # one fit launch on the B NT curves E(V) + F(V, T_i), then the reduction
        vol_rows = volumes[:, None, :].expand(B, NT, P).reshape(B * NT, P)
        en_rows = (energies[:, None, :] + F.transpose(1, 2)).reshape(B * NT, P)
        params, _, _, status = eos_fit(vol_rows, en_rows, eos)
        params, status = params.view(B, NT, 4), status.view(B, NT)
        v_eq, b_t = params[..., 3].contiguous(), params[..., 1].contiguous()
        alpha, cv, s, cp, gamma, inside = qha_derive(volumes, th.heat_capacity.view(B, P, NT), th.entropy.view(B, P, NT),
                                                     torch.tensor(t, dtype=torch.float64, device=dev), v_eq, b_t, status)
        h = lambda x: x.cpu().numpy()
        b_h = h(b_t)
    return QHAResult(dx=d, temperatures=t, volumes=h(volumes), energies=h(energies), phonon_free_energy=h(F),
                     gibbs=h(params[..., 0]).copy(), volume=h(v_eq), bulk_modulus=b_h, bulk_modulus_GPa=b_h * EV_A3_TO_GPA,
                     bp=h(params[..., 2]).copy(), thermal_expansion=h(alpha), heat_capacity_v=h(cv), heat_capacity_p=h(cp),
                     entropy=h(s), gruneisen=h(gamma), fit_status=h(status).astype(np.int64), inside=h(inside).astype(bool),
                     n_skipped=th.n_skipped.reshape(B, P), converged=h(r.converged).reshape(B, P), lattices=lat_out,
                     positions=pos_out, n_eval_calls=r.n_calls, n_phonon_evals=ph.n_evals)
