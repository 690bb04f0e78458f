"""The extents of every array the remaining workflow launches take, as their headers state them - the four argument blocks of
alignn_hip.h, alignn_neb.h and alignn_idpp.h (``STRUCTS``) and the flat prototypes of alignn_hip.h, alignn_neb.h, alignn_thermo.h
and alignn_traj.h (``FLAT``) - in the form of tests/workflow_extents.py, whose ``Block`` puts each array between the guard bands
of tests/gate_parity.py.  tests/test_workflow_extents.py checks both tables against the headers without a GPU;
tests/test_gpu_step_extents.py hands the guarded buffers to the launches.

Both tables have the form of ``workflow_extents.TABLE``; an entry of ``FLAT`` is keyed by its entry point, its ``fields`` are the
prototype's pointer parameters in the prototype's order, and the scalars its counts rest on are the prototype's other parameters.
The extents that a header states through the contents of an index table rather than a scalar are ``derived`` names, each with the
header's own words; the caller passes their values.

Roles: those of tests/workflow_extents.py, and ``state``: an array the launch reads and rewrites (positions, velocities, the
optimiser's and the thermostat's state, the cell).  It is allocated guarded and gets the caller's tensor copied in.

``writes``: for every array that is not an input, which of its elements one launch writes, in the header's terms.  "all" is every
element (the entry's flag ``whole``, which ``verify`` goes by, is then set); anything else names a subset, and the elements
outside it keep what they held: the guard pattern of an ``out`` array, the copied-in values of a ``state`` array.  tests/test_gpu_step_extents.py computes that subset on the host, from the inputs
alone, and checks it in both directions."""

import ctypes as C
import functools
import re
import types

import torch

from alignn_amd import _abi
from tests import gate_parity as gp
from tests import workflow_extents as wx

F64, I32, I64, U8, U64 = torch.float64, torch.int32, torch.int64, torch.uint8, torch.uint64
ROLES = wx.ROLES + ("state",)
CTYPE = {F64: "double", I32: "int32_t", I64: "int64_t", U8: "uint8_t", U64: "uint64_t"}


def _f(dtype, count, row, role, writes=None, whole=None):
    """``whole``: one launch writes every element (the default where ``writes`` is exactly "all"); the flag, not the wording of
    ``writes``, decides whether a case has to name the written elements"""
    return dict(dtype=dtype, count=count, row=row, roles=(role,), writes=writes, whole=(writes == "all") if whole is None else bool(whole))


ACTIVE = "the rows of the active structures whose force rows fit"
STEPPED = "the rows of the structures this launch steps (status[1+k] = 0)"
MOVED = STEPPED + " that are not fixed"
FRAME = "frame t / interval when t % interval == 0 (and n_rows fits), else nothing"
FITS = "the rows of the jobs that fit"
BANDS = "the entries of the active bands that fit"

STRUCTS = {
    "alignn_fire_args": dict(
        header="alignn_hip.h", entries=("alignn_fire_step",), let={},
        derived=dict(B="the structures of the batch: atom_ptr has B + 1 entries", N="atom_ptr[B]", force_rows="force_ptr[n_active]"),
        fields=dict(
            forces=_f(F64, "3 * force_rows", 3, "in"), energy=_f(F64, "n_active", 1, "in"), stress=_f(F64, "9 * n_active", 3, "in"),
            force_ptr=_f(I32, "n_active + 1", 1, "in"), active=_f(I32, "n_active", 1, "in"), atom_ptr=_f(I32, "B + 1", 1, "in"),
            inv_lattice=_f(F64, "9 * B", 3, "in"), lattice0=_f(F64, "9 * B", 3, "in"),
            positions=_f(F64, "3 * N", 3, "state", MOVED + " (filter: fixed rows too)"),
            velocities=_f(F64, "3 * N", 3, "state", STEPPED), frac=_f(F64, "3 * N", 3, "out", MOVED),
            state=_f(F64, "2 * B", 2, "state", STEPPED), istate=_f(I32, "2 * B", 2, "state", STEPPED),
            xa=_f(F64, "3 * N", 3, "state", MOVED), xc=_f(F64, "9 * B", 3, "state", STEPPED),
            cell_velocities=_f(F64, "9 * B", 3, "state", STEPPED), defgrad=_f(F64, "9 * B", 3, "state", STEPPED),
            lattice=_f(F64, "9 * B", 3, "state", STEPPED), forces_out=_f(F64, "3 * N", 3, "out", ACTIVE),
            energy_out=_f(F64, "B", 1, "out", ACTIVE), fmax_out=_f(F64, "B", 1, "out", ACTIVE),
            stress_out=_f(F64, "9 * B", 3, "out", ACTIVE),
            status=_f(I32, "1 + n_active", 1, "out", "all ([1+k] = -1 where the force rows do not fit)", whole=True),
            fixed=_f(U8, "N", 1, "in"), cell_mask=_f(F64, "9 * B", 3, "in"), scalar_pressure=_f(F64, "B", 1, "in"),
            enthalpy_out=_f(F64, "B", 1, "out", ACTIVE))),
    "alignn_md_args": dict(
        header="alignn_hip.h", entries=("alignn_md_step",), let=dict(B="n_structures", frames="steps // interval + 1"),
        derived=dict(N="atom_ptr[n_structures]"),
        fields=dict(
            forces=_f(F64, "3 * n_rows", 3, "in"), energy=_f(F64, "B", 1, "in"), stress=_f(F64, "9 * B", 3, "in"),
            atom_ptr=_f(I32, "B + 1", 1, "in"), masses=_f(F64, "N", 1, "in"), t0_kelvin=_f(F64, "B", 1, "in"),
            seeds=_f(U64, "B", 1, "in"), pressure=_f(F64, "B", 1, "in"), compressibility=_f(F64, "B", 1, "in"),
            lattice=_f(F64, "9 * B", 3, "state", "all, by 4 and by 6 with ptime > 0 while t < steps; else nothing"),
            inv_lattice=_f(F64, "9 * B", 3, "state", "as lattice"),
            momenta=_f(F64, "3 * N", 3, "state", "all unless n_rows does not fit"),
            positions=_f(F64, "3 * N", 3, "state", "all while t < steps, unless n_rows does not fit"),
            frac=_f(F64, "3 * N", 3, "out", "all while t < steps, unless n_rows does not fit"),
            velocities=_f(F64, "3 * N", 3, "state", "all, by 1 and 3 while t < steps"),
            scratch=_f(F64, "3 * N", 3, "scratch", "all, by 1 and 3 while t < steps"),
            status=_f(I32, "1", 1, "add", "[0] = -1 where n_rows does not fit, else nothing"),
            epot=_f(F64, "frames * B", "B", "out", FRAME), ekin=_f(F64, "frames * B", "B", "out", FRAME),
            temperature=_f(F64, "frames * B", "B", "out", FRAME),
            pressure_out=_f(F64, "frames * B", "B", "out", FRAME + "; by 3, 4 and 6 with stress"),
            volume_out=_f(F64, "frames * B", "B", "out", FRAME + "; by 3, 4 and 6"),
            traj_positions=_f(F64, "3 * frames * N", 3, "out", FRAME), traj_momenta=_f(F64, "3 * frames * N", 3, "out", FRAME),
            traj_lattice=_f(F64, "9 * frames * B", 3, "out", FRAME + "; by 3, 4 and 6"),
            noise_out=_f(F64, "N * (18 if ensemble == 1 else 36)", "18 if ensemble == 1 else 36", "out",
                         "while t < steps: 1: all; 3: the first 24 of every atom's 36, the last 12 with fixcm only"),
            nhc_state=_f(F64, "34 * B", 34, "state", "all, by 5 and 6"),
            conserved_out=_f(F64, "frames * B", "B", "out", FRAME + "; by 5 and 6"))),
    "alignn_neb_args": dict(
        header="alignn_neb.h", entries=("alignn_neb_forces",), let={},
        derived=dict(B="the bands of the batch: row_ptr has B + 1 entries", N="row_ptr[B]", n_ends="end_ptr[B]: sum n_b",
                     n_images="image_ptr[B]: sum M_b", force_rows="force_ptr[n_active]", n_energies="energy_ptr[n_active]"),
        fields=dict(
            forces=_f(F64, "3 * force_rows", 3, "in"), energy=_f(F64, "n_energies", 1, "in"), force_ptr=_f(I32, "n_active + 1", 1, "in"),
            energy_ptr=_f(I32, "n_active + 1", 1, "in"), active=_f(I32, "n_active", 1, "in"), row_ptr=_f(I32, "B + 1", 1, "in"),
            image_ptr=_f(I32, "B + 1", 1, "in"), end_ptr=_f(I32, "B + 1", 1, "in"), lattice=_f(F64, "9 * B", 3, "in"),
            inv_lattice=_f(F64, "9 * B", 3, "in"), spring=_f(F64, "B", 1, "in"), initial=_f(F64, "3 * n_ends", 3, "in"),
            final=_f(F64, "3 * n_ends", 3, "in"), end_energy=_f(F64, "2 * B", 2, "in"), positions=_f(F64, "3 * N", 3, "in"),
            fixed=_f(U8, "N", 1, "in"), forces_out=_f(F64, "3 * force_rows", 3, "out", "the rows of the active bands that fit"),
            energies_out=_f(F64, "n_images", 1, "out", BANDS), imax=_f(I32, "n_active", 1, "out", "all (-1 for a band that does not fit)", whole=True),
            emax=_f(F64, "n_active", 1, "out", BANDS))),
    "alignn_idpp_args": dict(
        header="alignn_idpp.h", entries=("alignn_idpp_forces",), let={},
        derived=dict(B="the bands of the batch: row_ptr has B + 1 entries", N="row_ptr[B]", n_ends="end_ptr[B]: sum n_b",
                     force_rows="force_ptr[n_active]", n_energies="energy_ptr[n_active]"),
        fields=dict(
            force_ptr=_f(I32, "n_active + 1", 1, "in"), energy_ptr=_f(I32, "n_active + 1", 1, "in"), active=_f(I32, "n_active", 1, "in"),
            row_ptr=_f(I32, "B + 1", 1, "in"), end_ptr=_f(I32, "B + 1", 1, "in"), lattice=_f(F64, "9 * B", 3, "in"),
            inv_lattice=_f(F64, "9 * B", 3, "in"), initial=_f(F64, "3 * n_ends", 3, "in"), final=_f(F64, "3 * n_ends", 3, "in"),
            positions=_f(F64, "3 * N", 3, "in"), forces=_f(F64, "3 * force_rows", 3, "out", "the rows of the active bands that fit"),
            energy=_f(F64, "n_energies", 1, "out", BANDS), row_energy=_f(F64, "force_rows", 1, "scratch", "as forces"),
            status=_f(I32, "n_active", 1, "out", "all"))),
}


def _flat(header, fields, let=None, derived=None):
    return dict(header=header, let=dict(let or {}), derived=dict(derived or {}), fields=fields)


PARENTS = dict(B="the structures: atom_ptr has B + 1 entries", N="atom_ptr[B]")
FCS = dict(PARENTS, fc_total="the sum over the structures of Ncell_s m_s^2")
ALL = "all"
PER_JOB = dict(rows="row_off[n_jobs]")
P_NT = "n_structures * n_temps"
LAGS = "n_rows * (max_lag + 1)"

FLAT = {
    "alignn_md_init_momenta": _flat("alignn_hip.h", dict(
        atom_ptr=_f(I32, "n_structures + 1", 1, "in"), masses=_f(F64, "N", 1, "in"), t_kelvin=_f(F64, "n_structures", 1, "in"),
        seeds=_f(U64, "n_structures", 1, "in"), momenta=_f(F64, "3 * N", 3, "out", ALL)), derived=dict(N="atom_ptr[n_structures]")),
    "alignn_neb_interpolate": _flat("alignn_neb.h", dict(
        initial=_f(F64, "3 * n_ends", 3, "in"), final=_f(F64, "3 * n_ends", 3, "in"), end_ptr=_f(I32, "n_bands + 1", 1, "in"),
        lattice=_f(F64, "9 * n_bands", 3, "in"), row_ptr=_f(I32, "n_bands + 1", 1, "in"), positions=_f(F64, "3 * n_rows", 3, "out", ALL),
        inv_lattice=_f(F64, "9 * n_bands", 3, "out", ALL)), derived=dict(n_ends="end_ptr[n_bands]: sum n_b")),
    "alignn_phonon_displace": _flat("alignn_hip.h", dict(
        positions=_f(F64, "3 * N", 3, "in"), atom_ptr=_f(I32, "B + 1", 1, "in"), lattice=_f(F64, "9 * B", 3, "in"),
        inv_supercell=_f(F64, "9 * B", 3, "in"), supercell=_f(I32, "3 * B", 3, "in"), jobs=_f(I32, "2 * n_jobs", 2, "in"),
        row_off=_f(I64, "n_jobs", 1, "in"), frac=_f(F64, "3 * rows", 3, "out", "the n_s Ncell_s rows from row_off[k] of every job"),
        cart=_f(F64, "3 * rows", 3, "out", "as frac")),
        derived=dict(PARENTS, rows="the rows of the jobs' supercells: max_k row_off[k] + n_s Ncell_s")),
    "alignn_phonon_fc_rows": _flat("alignn_hip.h", dict(
        forces=_f(F64, "3 * force_rows", 3, "in"), pairs=_f(I32, "2 * n_pairs", 2, "in"), pair_rows=_f(I64, "n_pairs", 1, "in"),
        atom_ptr=_f(I32, "B + 1", 1, "in"), supercell=_f(I32, "3 * B", 3, "in"), fc_off=_f(I64, "B", 1, "in"),
        fc=_f(F64, "fc_total", 1, "out", "row x of every cell of the structure, for every pair (s, x)")),
        derived=dict(FCS, force_rows="the rows of the pairs' supercells: max_k pair_rows[k] + 2 n_s Ncell_s")),
    "alignn_phonon_symmetrize": _flat("alignn_hip.h", dict(
        fc_in=_f(F64, "fc_total", 1, "in"), fc_out=_f(F64, "fc_total", 1, "out", ALL), atom_ptr=_f(I32, "n_structures + 1", 1, "in"),
        supercell=_f(I32, "3 * n_structures", 3, "in"), fc_off=_f(I64, "n_structures", 1, "in")), derived=FCS),
    "alignn_phonon_acoustic": _flat("alignn_hip.h", dict(
        fc=_f(F64, "fc_total", 1, "state", "the diagonal 3 x 3 blocks of cell offset 0"), atom_ptr=_f(I32, "n_structures + 1", 1, "in"),
        supercell=_f(I32, "3 * n_structures", 3, "in"), fc_off=_f(I64, "n_structures", 1, "in")), derived=FCS),
    "alignn_phonon_mass_weight": _flat("alignn_hip.h", dict(
        fc=_f(F64, "fc_total", 1, "in"), dyn=_f(F64, "fc_total", 1, "out", ALL), masses=_f(F64, "N", 1, "in"),
        atom_ptr=_f(I32, "n_structures + 1", 1, "in"), supercell=_f(I32, "3 * n_structures", 3, "in"),
        fc_off=_f(I64, "n_structures", 1, "in")), derived=FCS),
    "alignn_phonon_eigh": _flat("alignn_hip.h", dict(
        dyn=_f(F64, "dyn_total", 1, "in"), dyn_off=_f(I64, "n_structures", 1, "in"), lattice_points=_f(I32, "3 * n_points", 3, "in"),
        cell_ptr=_f(I32, "n_structures + 1", 1, "in"), dims=_f(I32, "n_structures", 1, "in"), qpoints=_f(F64, "3 * n_q", 3, "in"),
        freqs=_f(F64, "n_q * sum_m", 1, "out", ALL), freq_off=_f(I64, "n_structures", 1, "in"),
        eigvals=_f(F64, "n_q * sum_m", 1, "out", ALL), modes=_f(F64, "2 * n_q * sum_mm", 2, "out", ALL),
        mode_off=_f(I64, "n_structures", 1, "in"), status=_f(I32, "1", 1, "add", "[0] = 1 when a (q, structure) hit the sweep cap")),
        derived=dict(dyn_total="the sum over the structures of Ncell_s m_s^2", n_points="cell_ptr[n_structures]",
                     sum_m="the sum of dims", sum_mm="the sum of dims squared")),
    "alignn_phonon_dos": _flat("alignn_hip.h", dict(
        freqs=_f(F64, "n_freqs", 1, "in"), freq_off=_f(I64, "n_structures + 1", 1, "in"),
        energies=_f(F64, "n_structures * npts", "npts", "out", ALL), weights=_f(F64, "n_structures * npts", "npts", "out", ALL)),
        derived=dict(n_freqs="freq_off[n_structures]")),
    "alignn_defect_supercells": _flat("alignn_hip.h", dict(
        positions=_f(F64, "3 * N", 3, "in"), atom_ptr=_f(I32, "n_structures + 1", 1, "in"), lattice=_f(F64, "9 * n_structures", 3, "in"),
        supercell=_f(I32, "3 * n_structures", 3, "in"), jobs=_f(I32, "2 * n_jobs", 2, "in"), row_off=_f(I64, "n_jobs + 1", 1, "in"),
        cells=_f(F64, "9 * n_jobs", 3, "out", FITS), cart=_f(F64, "3 * rows", 3, "out", FITS), frac=_f(F64, "3 * rows", 3, "out", FITS),
        src=_f(I32, "rows", 1, "out", FITS)), derived=dict(PER_JOB, N="atom_ptr[n_structures]")),
    "alignn_slab_build": _flat("alignn_hip.h", dict(
        positions=_f(F64, "3 * N", 3, "in"), atom_ptr=_f(I32, "n_structures + 1", 1, "in"), lattice=_f(F64, "9 * n_structures", 3, "in"),
        jobs=_f(I32, "11 * n_jobs", 11, "in"), vacuum=_f(F64, "n_jobs", 1, "in"), row_off=_f(I64, "n_jobs + 1", 1, "in"),
        cells=_f(F64, "9 * n_jobs", 3, "out", FITS), cart=_f(F64, "3 * rows", 3, "out", FITS), frac=_f(F64, "3 * rows", 3, "out", FITS),
        src=_f(I32, "rows", 1, "out", FITS)), derived=dict(PER_JOB, N="atom_ptr[n_structures]")),
    "alignn_strain_build": _flat("alignn_hip.h", dict(
        positions=_f(F64, "3 * N", 3, "in"), atom_ptr=_f(I32, "n_structures + 1", 1, "in"), lattice=_f(F64, "9 * n_structures", 3, "in"),
        jobs=_f(I32, "n_jobs", 1, "in"), defgrad=_f(F64, "9 * n_jobs", 3, "in"), row_off=_f(I64, "n_jobs + 1", 1, "in"),
        cells=_f(F64, "9 * n_jobs", 3, "out", FITS), cart=_f(F64, "3 * rows", 3, "out", FITS), volume=_f(F64, "n_jobs", 1, "out", FITS)),
        derived=dict(PER_JOB, N="atom_ptr[n_structures]")),
    "alignn_eos_fit": _flat("alignn_hip.h", dict(
        volume=_f(F64, "n_structures * ld", "ld", "in"), energy=_f(F64, "n_structures * ld", "ld", "in"),
        n_points=_f(I32, "n_structures", 1, "in"), params=_f(F64, "4 * n_structures", 4, "out", ALL),
        rms=_f(F64, "n_structures", 1, "out", ALL), n_iter=_f(I32, "n_structures", 1, "out", ALL),
        status=_f(I32, "n_structures", 1, "out", ALL))),
    "alignn_elastic_fit": _flat("alignn_hip.h", dict(
        strain=_f(F64, "6 * n_structures * ld", 6, "in"), stress=_f(F64, "9 * n_structures * ld", 9, "in"),
        n_points=_f(I32, "n_structures", 1, "in"), c_raw=_f(F64, "36 * n_structures", 6, "out", ALL),
        c=_f(F64, "36 * n_structures", 6, "out", ALL), compliance=_f(F64, "36 * n_structures", 6, "out", ALL),
        sigma0=_f(F64, "6 * n_structures", 6, "out", ALL), moduli=_f(F64, "9 * n_structures", 9, "out", ALL),
        rms=_f(F64, "n_structures", 1, "out", ALL), asymmetry=_f(F64, "n_structures", 1, "out", ALL),
        status=_f(I32, "n_structures", 1, "out", ALL))),
    "alignn_zsl_match": _flat("alignn_hip.h", dict(
        film_cells=_f(F64, "4 * n_pairs", 2, "in"), subs_cells=_f(F64, "4 * n_pairs", 2, "in"), nmax_film=_f(I32, "n_pairs", 1, "in"),
        nmax_subs=_f(I32, "n_pairs", 1, "in"), hnf=_f(I32, "3 * n_hnf", 3, "in"), prefix=_f(I32, "258", 1, "in"),
        film_off=_f(I64, "n_pairs", 1, "in"), subs_off=_f(I64, "n_pairs", 1, "in"), film_tab=_f(F64, "4 * film_rows", 4, "scratch"),
        film_int=_f(I32, "4 * film_rows", 4, "scratch"), subs_tab=_f(F64, "24 * subs_rows", 4, "scratch"),
        subs_int=_f(I32, "4 * subs_rows", 4, "scratch"), best_score=_f(F64, "n_pairs * max_film", "max_film", "scratch"),
        best_tag=_f(I64, "n_pairs * max_film", "max_film", "scratch"), status=_f(I32, "n_pairs", 1, "out", ALL),
        multiples=_f(I32, "2 * n_pairs", 2, "out", "the pairs of status 0"), film_matrix=_f(I32, "4 * n_pairs", 2, "out", "the pairs of status 0"),
        subs_matrix=_f(I32, "4 * n_pairs", 2, "out", "the pairs of status 0"), mismatch=_f(F64, "4 * n_pairs", 4, "out", "the pairs of status 0")),
        derived=dict(n_hnf="prefix[257]: the Hermite normal forms of every n <= 256")),
    "alignn_interface_build": _flat("alignn_hip.h", dict(
        slab_cells=_f(F64, "9 * n_slabs", 3, "in"), slab_cart=_f(F64, "3 * slab_rows", 3, "in"), slab_off=_f(I64, "n_slabs + 1", 1, "in"),
        slab_src=_f(I32, "slab_rows", 1, "in"), jobs=_f(I32, "10 * n_pairs", 10, "in"), separation=_f(F64, "n_pairs", 1, "in"),
        vacuum=_f(F64, "n_pairs", 1, "in"), out_off=_f(I64, "3 * n_pairs + 1", 1, "in"), cells=_f(F64, "27 * n_pairs", 3, "out", FITS),
        cart=_f(F64, "3 * rows", 3, "out", FITS), frac=_f(F64, "3 * rows", 3, "out", FITS), src=_f(I32, "rows", 1, "out", FITS),
        part=_f(I32, "rows", 1, "out", FITS), area=_f(F64, "n_pairs", 1, "out", FITS)),
        derived=dict(slab_rows="slab_off[n_slabs]", rows="out_off[3 n_pairs]")),
    "alignn_phonon_thermal": _flat("alignn_thermo.h", dict(
        freqs=_f(F64, "n_freqs", 1, "in"), freq_off=_f(I64, "n_structures + 1", 1, "in"), n_q=_f(I32, "n_structures", 1, "in"),
        temperatures=_f(F64, "n_temps", 1, "in"), workspace=_f(U8, "workspace_bytes", 1, "scratch"),
        free_energy=_f(F64, P_NT, "n_temps", "out", ALL), internal_energy=_f(F64, P_NT, "n_temps", "out", ALL),
        entropy=_f(F64, P_NT, "n_temps", "out", ALL), heat_capacity=_f(F64, P_NT, "n_temps", "out", ALL),
        zpe=_f(F64, "n_structures", 1, "out", ALL), n_skipped=_f(I32, "n_structures", 1, "out", ALL)),
        derived=dict(n_freqs="freq_off[n_structures]")),
    "alignn_qha_derive": _flat("alignn_thermo.h", dict(
        volumes=_f(F64, "n_structures * n_points", "n_points", "in"),
        heat_capacity=_f(F64, "n_structures * n_points * n_temps", "n_temps", "in"),
        entropy=_f(F64, "n_structures * n_points * n_temps", "n_temps", "in"), temperatures=_f(F64, "n_temps", 1, "in"),
        v_eq=_f(F64, P_NT, "n_temps", "in"), b_t=_f(F64, P_NT, "n_temps", "in"), status=_f(I32, P_NT, "n_temps", "in"),
        alpha=_f(F64, P_NT, "n_temps", "out", ALL), cv_out=_f(F64, P_NT, "n_temps", "out", ALL),
        s_out=_f(F64, P_NT, "n_temps", "out", ALL), cp_out=_f(F64, P_NT, "n_temps", "out", ALL),
        gamma=_f(F64, P_NT, "n_temps", "out", ALL), inside=_f(I32, P_NT, "n_temps", "out", ALL))),
    "alignn_traj_vdos": _flat("alignn_traj.h", dict(
        vacf=_f(F64, LAGS, "max_lag + 1", "in"), out=_f(F64, "n_rows * n_freq", "n_freq", "out", ALL))),
    "alignn_traj_fit": _flat("alignn_traj.h", dict(
        msd=_f(F64, "3 * " + LAGS, 3, "in"), out=_f(F64, "16 * n_rows", 4, "out", ALL))),
    "alignn_traj_green_kubo": _flat("alignn_traj.h", dict(
        vacf=_f(F64, LAGS, "max_lag + 1", "in"), out=_f(F64, LAGS, "max_lag + 1", "out", ALL))),
}
for _name, _t in FLAT.items():
    _t["entries"] = (_name,)
ENTRIES = tuple(e for t in STRUCTS.values() for e in t["entries"]) + tuple(FLAT)


@functools.lru_cache(maxsize=None)
def prototype(entry):
    """[(parameter name, the header's type name, pointer?, const?)] of a flat entry point, read from its header's text"""
    with open(wx.read_header(FLAT[entry]["header"]).path) as f:
        text = _abi._uncomment(f.read())
    m = re.search(rf"\b{entry}\s*\(([^;{{}}()]*)\)\s*;", text)
    out = []
    for p in m.group(1).split(","):
        d = re.fullmatch(r"\s*(const\s+)?(\w+)\s*(\*?)\s*(\w+)\s*", p)
        out.append((d.group(4), d.group(2), bool(d.group(3)), bool(d.group(1))))
    return out


def struct_fields(struct):
    """[(field name, the header's type name, pointer?, const?)] of an argument block, read from its header's text"""
    with open(wx.header_of(struct, STRUCTS).path) as f:
        text = _abi._uncomment(f.read())
    body = text[text.index("typedef struct " + struct):text.index("} " + struct)].split("{", 1)[1]
    out = []
    for s in body.split(";"):
        m = re.fullmatch(r"\s*(const\s+)?(\w+)\b(.*)", s, re.S)
        if m:
            for d in m.group(3).split(","):
                dm = re.fullmatch(r"\s*(\**)\s*(\w+)\s*", d)
                out.append((dm.group(2), m.group(2), bool(dm.group(1)), bool(m.group(1))))
    return out


class Call(wx.Block):
    """``workflow_extents.Block`` for a flat prototype: ``set`` its scalar parameters and derived extents, ``alloc`` its pointer
    parameters, ``launch`` passes them in the prototype's order (a parameter ``stream`` is the stream)."""

    def __init__(self, guards, entry, device=gp.DEV, case=""):
        self.guards, self.struct, self.device, self.case = guards, entry, device, case
        self.tables, self.table = FLAT, FLAT[entry]
        self.args, self.scalars = types.SimpleNamespace(), {}
        self.payload, self.derived = {}, {}
        self.params = prototype(entry)

    def set(self, **scalars):
        known = {n for n, _, pointer, _ in self.params if not pointer and n != "stream"}
        for k, v in scalars.items():
            if k in self.table["derived"]:
                self.derived[k] = int(v)
            else:
                assert k in known, f"{self.struct} has no scalar parameter {k}"
                self.scalars[k] = v
        return self

    def values(self):
        return dict(self.scalars, **self.derived)

    def alloc(self, inputs=None, null=()):
        for field in self.table["fields"]:
            if not hasattr(self.args, field):
                setattr(self.args, field, None)
        return super().alloc(self.struct, inputs, null)

    def arguments(self, pointers, stream):
        return [stream if n == "stream" else pointers.get(n) if pointer else self.scalars[n] for n, _, pointer, _ in self.params]

    def launch(self, lib, stream=None, expect=0):
        ptrs = {}
        for field, t in self.payload.items():
            ptrs[field] = None if t is None else self.guards.gptr(t)
        self.guards.launched(self.struct)
        rc = getattr(lib, self.struct)(*self.arguments(ptrs, stream))
        assert rc == expect, f"{self.case}: {self.struct} returned {rc}"
        found = self.guards.check()
        assert not found, f"{self.case}: after {self.struct}: " + "; ".join(f[4] for f in found)
        return self


def plain_copy(b):
    """the block's arrays as they stand, each on a plain allocation of its own (no guards): the reference's buffers"""
    return {k: None if t is None else t.clone() for k, t in b.payload.items()}


def plain_launch(b, lib, plain, stream=None, entry=None, expect=0):
    """the same launch on the arrays of ``plain_copy``"""
    ptrs = {k: None if t is None else t.data_ptr() for k, t in plain.items()}
    if isinstance(b, Call):
        rc = getattr(lib, b.struct)(*b.arguments(ptrs, stream))
    else:
        args = type(b.args).from_buffer_copy(b.args)
        for k, p in ptrs.items():
            setattr(args, k, p)
        rc = getattr(lib, entry or b.table["entries"][0])(C.byref(args), stream)
    assert rc == expect, f"{b.case}: {b.struct} on plain allocations returned {rc}"


def verify(b, plain, written=None, before=None):
    """Checks (b) and (c) of tests/test_gpu_step_extents.py over every array of the block ``b`` after a launch on it and on
    ``plain`` (``plain_copy`` taken before it).  ``written``: field -> True (every element), False (none) or a bool mask over the
    elements, of what the launches so far (``out`` arrays, whose pattern stays) or this launch (``state`` arrays, against
    ``before``: ``plain_copy`` of the block before the launch) write; an array whose table entry is flagged ``whole`` needs none, every other
    ``out`` or ``state`` array must be named.  An input must still hold the bits that were copied in."""
    entry = b.table["entries"][0]
    written = dict(written or {})
    for field, t in b.payload.items():
        if t is None:
            continue
        spec, role = b.table["fields"][field], b.role(field, entry)
        got, ref = bits(t).reshape(-1), bits(plain[field]).reshape(-1)
        what = f"{b.case}: {field} of {b.struct}"
        if role == "in":
            assert torch.equal(got, ref), f"{what}: an input was changed"
            continue
        if role == "scratch":
            continue
        mask = written.pop(field, None)
        if mask is None:  # (an ``add`` array - a status word - is compared with the plain launch's only)
            assert role == "add" or spec["whole"], f"{what}: which elements are written?"
            mask = True
        if isinstance(mask, bool):
            mask = torch.full((t.numel(),), mask, dtype=torch.bool)
        mask = mask.reshape(-1).to(t.device)
        assert mask.numel() == t.numel(), (what, mask.numel(), t.numel())
        if role == "out":
            pat = is_pattern(t).reshape(-1)
            missed = int((pat & mask).sum())
            assert missed == 0, f"{what}: {missed} elements the header calls written still hold the pattern"
            left, want = int(pat.sum()), int((~mask).sum())
            assert left == want, f"{what}: {left} elements hold the pattern, the header leaves {want} alone"
        elif role == "state" and before is not None:
            was = bits(before[field]).reshape(-1)
            assert torch.equal(got[~mask], was[~mask]), f"{what}: an element the header leaves alone was rewritten"
        assert torch.equal(got, ref), f"{what}: differs from the same launch on plain allocations"
    assert not written, f"{b.case}: no such array: {sorted(written)}"


def bits(t):
    """the tensor as integers of its width: bits are compared, never floats (a NaN equals itself)"""
    return t.view(gp._PATTERN[t.dtype][0]) if t.dtype in gp._PATTERN else t


def is_pattern(t):
    """per element: does it still hold the guard pattern"""
    return bits(t) == (gp._PATTERN[t.dtype][1] if t.dtype in gp._PATTERN else gp.INT_PATTERN[t.dtype])
