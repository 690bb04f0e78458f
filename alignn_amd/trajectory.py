"""Batched analysis of MD trajectories on the device: g(r), mean squared displacement, velocity autocorrelation, vibrational
density of states and diffusion coefficients, for the B structures of a ``run_md`` call together.

The reference's ``alignn/ff/ff.py`` writes ASE trajectory files and leaves their analysis to the user.  ``run_md`` keeps the
whole trajectory on the device (``MDResult.traj_positions`` / ``traj_momenta`` [n_frames, sum n_i, 3], ``traj_lattices`` under
NPT); the functions here read those tensors where they are:

* ``rdf``: pair histograms over every periodic image within ``r_max``, per species pair, with g(r) and the running coordination
  number derived from them;
* ``msd`` / ``vacf``: averages over time origins, per species and (MSD) per Cartesian component;
* ``vdos``: the cosine transform of the normalised VACF; ``diffusion``: Einstein's line through the MSD and, from a VACF, the
  Green-Kubo running integral; ``analyze_md``: all of them on an ``MDResult``.

Conventions.  Per structure, group 0 is every atom and groups 1 .. S are its species in ascending atomic number (at most 8); S
of a result is the largest of the batch, a structure with fewer species leaves its other rows zero.  Pair rows: row 0 every
pair, then the unordered group pairs a <= b in the order (1,1), (1,2), (2,2), (1,3), (2,3), (3,3), ... (``pair_row``), a row
a < b holding both orders.  Frames are selected by ``start`` / ``stop`` / ``step`` as a slice selects them; lags and origins
count the selected frames.  The kernels (csrc/trajectory.hip) are float64 without contraction, the histogram is summed with
integer atomics (exact), every floating-point sum has a fixed order over the structure's own rows and frames: a structure's
numbers are the same bits alone, in a batch and at any place of it.  Nothing is read back from the device but the status word of
``rdf``.  tests/traj_ref.py restates the formulas in numpy; the entry points are declared in include/alignn_traj.h, read here
with the reader of alignn_amd/_abi.py.  The checks of these conventions - frames, the trajectory tensor, cells, groups - are in
alignn_amd/_trajectory_inputs.py, which ``alignn_amd.order`` and ``alignn_amd.local_order`` use as well.

Units.  Positions in A, momenta in amu A per ASE time unit (what ``run_md`` records), so the VACF is in A^2 per ASE time unit
squared.  ``dtau_fs`` is the time between two selected frames in fs: ``timestep * interval * step``.  Diffusion coefficients are
returned in A^2/fs; multiply by ``A2_FS_TO_CM2_S`` for cm^2/s.

Not here: accumulation inside ``run_md`` without a stored trajectory, ionic conductivity.  Angle distributions, Steinhardt order
parameters and the static structure factor of the same trajectories: ``alignn_amd.order``.
"""

from __future__ import annotations

import ctypes as C
import numbers
from dataclasses import dataclass
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _abi, _lib
from ._structures import host
from ._trajectory_inputs import _frames, _groups, _masses, _positive, _traj, bins, inputs
from .dynamics import FS

__all__ = ["rdf", "msd", "vacf", "vdos", "diffusion", "green_kubo", "analyze_md", "pair_row", "RDFResult", "MSDResult",
           "VACFResult", "VDOSResult", "DiffusionResult", "TrajectoryAnalysis", "A2_FS_TO_CM2_S", "MAX_SPECIES", "MAX_BINS",
           "MAX_IMAGE_RANGE"]

H = _abi.header("alignn_traj.h")
HEADER, STRUCTS, SIGNATURES = H.path, H.structs, H.signatures  # the argument blocks; entry point -> (restype, argtypes)
RdfArgs, CorrArgs = STRUCTS["alignn_traj_rdf_args"], STRUCTS["alignn_traj_corr_args"]
MAX_SPECIES = H.defines["ALIGNN_TRAJ_MAX_SPECIES"]
MAX_BINS = H.defines["ALIGNN_TRAJ_MAX_BINS"]
MAX_IMAGE_RANGE = H.defines["ALIGNN_TRAJ_MAX_IMAGE_RANGE"]
STATUS_IMAGES = H.defines["ALIGNN_TRAJ_STATUS_IMAGES"]
A2_FS_TO_CM2_S = 0.1  # 1 A^2/fs = 1e-16 cm^2 / 1e-15 s
WINDOWS = {"none": 0, "hann": 1}


def _load():
    return _lib.bind(H)


def pair_row(a: int, b: int) -> int:
    """The row of ``RDFResult.counts`` / ``g`` / ``coordination`` that holds the pairs of groups ``a`` and ``b`` (1-based, either
    order); ``pair_row(0, 0)`` is row 0, every pair."""
    if a == 0 and b == 0:
        return 0
    lo, hi = min(a, b), max(a, b)
    if lo < 1:
        raise ValueError("pair_row: groups are 1-based (0, 0 for every pair)")
    return 1 + hi * (hi - 1) // 2 + (lo - 1)


# --- results -----------------------------------------------------------------------------------------------------------------------
@dataclass
class RDFResult:
    """``r`` [n_bins]: the bin centres (A).  ``counts`` [B, P, n_bins] int64: ordered pairs (i, j, image) per bin, summed over the
    frames used; P = 1 + S (S + 1) / 2, the rows as ``pair_row`` numbers them.  ``g`` [B, P, n_bins]: counts <V> / (F N_a N_b w
    shell), <V> the mean cell volume over the frames used (the mean-volume convention), w = 2 for a row a < b (it holds both
    orders) and 1 otherwise, so every g tends to 1.  ``coordination`` [B, P, n_bins]: the running coordination number at the bin's
    upper edge, cumsum(counts) / (F N_a w) - for a < b the b around an a.  ``volume`` [B]: <V>.  ``species[b]``: the atomic
    numbers of structure b's groups 1 .. S_b.  ``n_frames``: frames used."""

    r: torch.Tensor
    counts: torch.Tensor
    g: torch.Tensor
    coordination: torch.Tensor
    volume: torch.Tensor
    species: List[List[int]]
    n_frames: int
    r_max: float


@dataclass
class MSDResult:
    """``msd`` [B, S + 1, K + 1, 3] (A^2): per group (0: every atom) , lag and Cartesian component; ``total`` sums the components.
    ``n_origins`` [K + 1]: the time origins averaged at each lag."""

    msd: torch.Tensor
    n_origins: np.ndarray
    species: List[List[int]]
    origin_stride: int
    remove_com: bool

    @property
    def total(self) -> torch.Tensor:
        return (self.msd[..., 0] + self.msd[..., 1]) + self.msd[..., 2]


@dataclass
class VACFResult:
    """``vacf`` [B, S + 1, K + 1]: <v(t) . v(t + k)> per group and lag, in A^2 per ASE time unit squared (not normalised)."""

    vacf: torch.Tensor
    n_origins: np.ndarray
    species: List[List[int]]
    origin_stride: int


@dataclass
class VDOSResult:
    """``freq_THz`` [n_freq] and ``dos`` [B, S + 1, n_freq] in fs: D(nu) = 2 dtau sum_k c_k w_k C(k) / C(0) cos(2 pi nu k dtau),
    the Fourier transform of the normalised VACF.  Over the two-sided frequency axis (D is even in nu) D integrates to 1, so
    3 N_a D integrates to the group's 3 N_a modes; over nu >= 0 alone the integral is half of that (nu in 1/fs = 1000 THz)."""

    freq_THz: torch.Tensor
    dos: torch.Tensor
    window: str


@dataclass
class DiffusionResult:
    """Einstein: ``slope`` (A^2/fs), ``intercept`` (A^2), ``stderr`` (of the slope) and ``D`` (A^2/fs), each [B, S + 1, 4]: the
    components x, y, z (D = slope / 2) and the total (D = slope / 6).  ``fit``: the lags (k_lo, k_hi) of the line.
    ``green_kubo`` [B, S + 1, K + 1] (A^2/fs; with a VACF, else None): the running integral D_GK(k) = (1/3) int_0^tau_k C."""

    slope: torch.Tensor
    intercept: torch.Tensor
    stderr: torch.Tensor
    D: torch.Tensor
    fit: Tuple[int, int]
    green_kubo: Optional[torch.Tensor] = None


@dataclass
class TrajectoryAnalysis:
    rdf: RDFResult
    msd: MSDResult
    vacf: VACFResult
    vdos: VDOSResult
    diffusion: DiffusionResult


# --- the functions -----------------------------------------------------------------------------------------------------------------
def rdf(traj: torch.Tensor, lattices: torch.Tensor, ns: Sequence[int], species: Optional[Sequence] = None, *, r_max: float = 8.0,
        n_bins: int = 200, start: Optional[int] = None, stop: Optional[int] = None, step: Optional[int] = None) -> RDFResult:
    """The radial distribution functions of B structures over the frames ``start:stop:step`` of ``traj`` [F, sum ns, 3] (float64
    on the GPU, Cartesian, not wrapped).  ``lattices``: [B, 3, 3] for a fixed cell or [F, B, 3, 3] per frame
    (``MDResult.traj_lattices``).  ``species``: B integer arrays of atomic numbers, or None for one group.

    Pairs are the ordered triples (i, j, image) with (i, i, 0) left out; the fractional difference is wrapped by ``rint`` and the
    images run over |m_k| <= floor(r_max / h_k + 1/2), h_k the heights of each frame's own cell - an atom's own images included,
    so ``r_max`` may exceed half the cell.  A range above 8 on any axis is a ``ValueError`` (the status word, the one value read
    back).  r = sqrt((dx dx + dy dy) + dz dz) falls into bin floor(r (n_bins / r_max)); r >= r_max is dropped.  ``n_bins``: 1 ..
    4096."""
    who = "rdf"
    r_max, n_bins = _positive(who, "r_max", r_max), bins(who, n_bins, MAX_BINS, bool_ok=True)
    sel = inputs(who, traj, lattices, ns, start, stop, step, atom_limit=False)
    B, used, dev = len(sel.ns), sel.n_frames, sel.traj.device
    lib = _load()
    with _lib.device_guard(sel.traj):
        S, lists = sel.groups(species)
        P = 1 + S * (S + 1) // 2
        counts = torch.zeros(B, P, n_bins, dtype=torch.int64, device=dev)
        g, coord = torch.empty(B, P, n_bins, dtype=torch.float64, device=dev), torch.empty(B, P, n_bins, dtype=torch.float64, device=dev)
        volume, centres = torch.empty(B, dtype=torch.float64, device=dev), torch.empty(n_bins, dtype=torch.float64, device=dev)
        status = torch.zeros(1, dtype=torch.int32, device=dev)
        args = RdfArgs(counts=counts.data_ptr(), g=g.data_ptr(), coord=coord.data_ptr(), volume=volume.data_ptr(),
                       centres=centres.data_ptr(), r_max=r_max, n_bins=int(n_bins), **sel.fields(RdfArgs, status))
        _lib.check(lib.alignn_traj_rdf_counts(C.byref(args), _lib.stream()), "traj_rdf_counts")
        _lib.check(lib.alignn_traj_rdf_normalise(C.byref(args), _lib.stream()), "traj_rdf_normalise")
        if int(status.item()) & STATUS_IMAGES:
            raise ValueError(f"{who}: r_max = {r_max} needs periodic images beyond +-{MAX_IMAGE_RANGE} cells along an axis of some "
                             "frame's cell (or a cell is singular): lower r_max or analyse a supercell")
    return RDFResult(r=centres, counts=counts, g=g, coordination=coord, volume=volume, species=lists, n_frames=used, r_max=r_max)


def _correlate(who, traj, ns, species, masses, max_lag, origin_stride, start, stop, step, mode, remove_com):
    traj, ns = _traj(who, "traj" if mode == 0 else "traj_momenta", traj, ns)
    B, N, F = len(ns), sum(ns), traj.shape[0]
    frame0, fstep, used = _frames(who, F, start, stop, step)
    if used < 1:
        raise ValueError(f"{who}: the frame selection is empty")
    if max_lag is None:
        max_lag = used - 1
    if not isinstance(max_lag, numbers.Integral) or not 0 <= max_lag <= used - 1:
        raise ValueError(f"{who}: max_lag must be 0 .. {used - 1} (the frames used less one), got {max_lag!r}")
    if not isinstance(origin_stride, numbers.Integral) or origin_stride < 1:
        raise ValueError(f"{who}: origin_stride must be an int >= 1, got {origin_stride!r}")
    dev = traj.device
    lib = _load()
    K = int(max_lag)
    with _lib.device_guard(traj):
        ptr, group, count, S, lists = _groups(who, ns, species, dev)
        mass = _masses(who, masses, ns, dev) if (mode == 1 or remove_com) else None
        com = torch.empty(used, B, 3, dtype=torch.float64, device=dev) if (mode == 0 and remove_com) else None
        out = torch.empty((B, S + 1, K + 1, 3) if mode == 0 else (B, S + 1, K + 1), dtype=torch.float64, device=dev)
        args = CorrArgs(traj=traj.data_ptr(), masses=_lib.ptr(mass), atom_ptr=ptr.data_ptr(), group=group.data_ptr(),
                        group_count=count.data_ptr(), com=_lib.ptr(com), out=out.data_ptr(), n_structs=B, n_atoms=N, n_species=S,
                        n_total_frames=F, frame0=frame0, frame_step=fstep, n_frames=used, max_lag=K,
                        origin_stride=int(origin_stride), mode=mode)
        if com is not None:
            _lib.check(lib.alignn_traj_com(C.byref(args), _lib.stream()), "traj_com")
        _lib.check(lib.alignn_traj_corr(C.byref(args), _lib.stream()), "traj_corr")
    n_origins = (used - 1 - np.arange(K + 1)) // int(origin_stride) + 1
    return out, n_origins, lists


def msd(traj: torch.Tensor, ns: Sequence[int], species: Optional[Sequence] = None, masses: Optional[Sequence] = None, *,
        max_lag: Optional[int] = None, origin_stride: int = 1, remove_com: bool = True, start: Optional[int] = None,
        stop: Optional[int] = None, step: Optional[int] = None) -> MSDResult:
    """The mean squared displacement of the positions ``traj`` [F, sum ns, 3], per group, lag k = 0 .. ``max_lag`` (default and at
    most: the frames used less one) and Cartesian component, averaged over the group's atoms and the origins t = 0,
    ``origin_stride``, 2 ``origin_stride``, ... with t + k inside the selection:
    ``sum_t sum_i ((r_i(t + k) - r_i(t)) - (c(t + k) - c(t)))^2 / (n_origins(k) N_a)``.  ``remove_com``: c is the structure's
    mass-weighted centre of mass (``masses``: B arrays [n_i] as ``run_md`` takes them, required then), else zero."""
    who = "msd"
    if not isinstance(remove_com, (bool, np.bool_)):
        raise ValueError(f"{who}: remove_com is one bool, got {type(remove_com).__name__}")
    if remove_com and masses is None:
        raise ValueError(f"{who}: remove_com=True needs the masses")
    out, n_or, lists = _correlate(who, traj, ns, species, masses, max_lag, origin_stride, start, stop, step, 0, bool(remove_com))
    return MSDResult(msd=out, n_origins=n_or, species=lists, origin_stride=int(origin_stride), remove_com=bool(remove_com))


def vacf(traj_momenta: torch.Tensor, ns: Sequence[int], species: Optional[Sequence], masses: Sequence, *,
         max_lag: Optional[int] = None, origin_stride: int = 1, start: Optional[int] = None, stop: Optional[int] = None,
         step: Optional[int] = None) -> VACFResult:
    """The velocity autocorrelation of the momenta ``traj_momenta`` [F, sum ns, 3] (``MDResult.traj_momenta``), v = p / m:
    ``sum_t sum_i v_i(t) . v_i(t + k) / (n_origins(k) N_a)`` per group and lag, the origins as in ``msd``."""
    out, n_or, lists = _correlate("vacf", traj_momenta, ns, species, masses, max_lag, origin_stride, start, stop, step, 1, False)
    return VACFResult(vacf=out, n_origins=n_or, species=lists, origin_stride=int(origin_stride))


def _rows(who: str, name: str, t, last: int) -> torch.Tensor:
    if not isinstance(t, torch.Tensor) or t.dtype != torch.float64 or not t.is_cuda or t.ndim != last:
        raise TypeError(f"{who}: {name} must be a float64 tensor on the GPU with {last} axes")
    return t.contiguous()


def vdos(vacf_result, dtau_fs: float, *, n_freq: int = 256, f_max_THz: float = 30.0, window: str = "hann") -> VDOSResult:
    """The vibrational density of states from a ``VACFResult`` (or its ``vacf`` tensor): ``D(nu_j) = 2 dtau sum_k c_k w_k [C(k) /
    C(0)] cos(2 pi nu_j k dtau)`` at ``nu_j = j f_max_THz / (n_freq - 1)``, c_0 = 1/2 and 1 otherwise, ``window="hann"``: w_k = (1
    + cos(pi k / K)) / 2, ``"none"``: 1.  In fs.  D is the Fourier transform of the normalised VACF: over the two-sided frequency
    axis it integrates to 1 and 3 N_a D to the group's 3 N_a modes (over nu >= 0 alone: half, D being even)."""
    who = "vdos"
    c = _rows(who, "vacf", vacf_result.vacf if isinstance(vacf_result, VACFResult) else vacf_result, 3)
    dtau, f_max = _positive(who, "dtau_fs", dtau_fs), _positive(who, "f_max_THz", f_max_THz)
    if not isinstance(n_freq, numbers.Integral) or n_freq < 2:
        raise ValueError(f"{who}: n_freq must be an int >= 2, got {n_freq!r}")
    if window not in WINDOWS:
        raise ValueError(f"{who}: window must be one of {sorted(WINDOWS)}, got {window!r}")
    B, G, K1 = c.shape
    with _lib.device_guard(c):
        out = torch.empty(B, G, int(n_freq), dtype=torch.float64, device=c.device)
        _lib.check(_load().alignn_traj_vdos(c.data_ptr(), B * G, K1 - 1, dtau, int(n_freq), f_max, WINDOWS[window], out.data_ptr(),
                                            _lib.stream()), "traj_vdos")
        freq = torch.arange(int(n_freq), dtype=torch.float64, device=c.device) * (f_max / (int(n_freq) - 1))
    return VDOSResult(freq_THz=freq, dos=out, window=window)


def green_kubo(vacf_result, dtau_fs: float) -> torch.Tensor:
    """The Green-Kubo running integral ``D_GK(k) = (1/3) int_0^{tau_k} C dtau`` [B, S + 1, K + 1] by the trapezoid rule, in
    A^2/fs.  The velocities are in A per ASE time unit, so the integral over ``tau_k = k dtau_fs FS`` (ASE time units, ``FS`` =
    ``dynamics.FS``) is in A^2 per ASE time unit; it is multiplied by ``FS`` once more to arrive at A^2/fs."""
    who = "green_kubo"
    c = _rows(who, "vacf", vacf_result.vacf if isinstance(vacf_result, VACFResult) else vacf_result, 3)
    dtau = _positive(who, "dtau_fs", dtau_fs)
    B, G, K1 = c.shape
    with _lib.device_guard(c):
        out = torch.empty_like(c)
        _lib.check(_load().alignn_traj_green_kubo(c.data_ptr(), B * G, K1 - 1, dtau, FS, out.data_ptr(), _lib.stream()),
                   "traj_green_kubo")
    return out


def diffusion(msd_result, dtau_fs: float, *, fit: Tuple[int, int], vacf_result=None) -> DiffusionResult:
    """Einstein's relation: the ordinary least-squares line through msd(k) against ``tau_k = k dtau_fs`` over the lags ``fit =
    (k_lo, k_hi)``, 0 <= k_lo < k_hi <= K, per group for x, y, z (D = slope / 2) and their total (D = slope / 6), in A^2/fs
    (``A2_FS_TO_CM2_S`` converts to cm^2/s).  The centred form: the means, then Sxx and Sxy.  With ``vacf_result`` the Green-Kubo
    running integral (``green_kubo``) comes along."""
    who = "diffusion"
    m = _rows(who, "msd", msd_result.msd if isinstance(msd_result, MSDResult) else msd_result, 4)
    dtau = _positive(who, "dtau_fs", dtau_fs)
    B, G, K1, three = m.shape
    ok = isinstance(fit, (tuple, list)) and len(fit) == 2 and all(isinstance(k, numbers.Integral) for k in fit)
    if three != 3 or not ok or not 0 <= fit[0] < fit[1] <= K1 - 1 or B * G > 65535:
        raise ValueError(f"{who}: need msd [B, S + 1, K + 1, 3] and fit = (k_lo, k_hi) with 0 <= k_lo < k_hi <= {K1 - 1}, got "
                         f"{tuple(m.shape)} and {fit!r}")
    with _lib.device_guard(m):
        out = torch.empty(B, G, 4, 4, dtype=torch.float64, device=m.device)
        _lib.check(_load().alignn_traj_fit(m.data_ptr(), B * G, K1 - 1, dtau, int(fit[0]), int(fit[1]), out.data_ptr(),
                                           _lib.stream()), "traj_fit")
    gk = None if vacf_result is None else green_kubo(vacf_result, dtau)
    return DiffusionResult(slope=out[..., 0], intercept=out[..., 1], stderr=out[..., 2], D=out[..., 3],
                           fit=(int(fit[0]), int(fit[1])), green_kubo=gk)


def analyze_md(result, lattices, ns: Sequence[int], species: Optional[Sequence], masses: Sequence, *, timestep: float,
               interval: int = 1, r_max: float = 8.0, n_bins: int = 200, max_lag: Optional[int] = None, origin_stride: int = 1,
               fit: Optional[Tuple[int, int]] = None, remove_com: bool = True, n_freq: int = 256, f_max_THz: float = 30.0,
               window: str = "hann", start: Optional[int] = None, stop: Optional[int] = None,
               step: Optional[int] = None) -> TrajectoryAnalysis:
    """Every analysis above on an ``MDResult`` of ``run_md(..., trajectory=True)``: ``timestep`` (fs) and ``interval`` as they were
    given to ``run_md``, so that two selected frames are ``dtau_fs = timestep * interval * step`` apart.  The cells are
    ``result.traj_lattices`` when the run recorded them (NPT), else ``lattices`` ([B, 3, 3], a tensor or B arrays).  ``fit``
    defaults to the second half of the lags, (K // 2, K).  Raises when the run was made with ``trajectory=False``."""
    who = "analyze_md"
    if getattr(result, "traj_positions", None) is None or getattr(result, "traj_momenta", None) is None:
        raise ValueError(f"{who}: the MDResult holds no trajectory (run_md(..., trajectory=True) records one)")
    pos, mom = result.traj_positions, result.traj_momenta
    dev = pos.device
    if result.traj_lattices is not None:
        lat = result.traj_lattices
    elif isinstance(lattices, torch.Tensor):
        lat = lattices.to(dev, torch.float64)
    else:
        lat = torch.stack([torch.as_tensor(host(l), dtype=torch.float64) for l in lattices]).to(dev)
    interval_ok = isinstance(interval, numbers.Integral) and interval >= 1
    if not interval_ok:
        raise ValueError(f"{who}: interval must be an int >= 1, got {interval!r}")
    _, fstep, used = _frames(who, pos.shape[0], start, stop, step)
    dtau = _positive(who, "timestep", timestep) * int(interval) * fstep
    sel = dict(start=start, stop=stop, step=step)
    K = used - 1 if max_lag is None else max_lag
    if fit is None:
        fit = (K // 2, K)
    r = rdf(pos, lat, ns, species, r_max=r_max, n_bins=n_bins, **sel)
    m = msd(pos, ns, species, masses, max_lag=max_lag, origin_stride=origin_stride, remove_com=remove_com, **sel)
    v = vacf(mom, ns, species, masses, max_lag=max_lag, origin_stride=origin_stride, **sel)
    d = vdos(v, dtau, n_freq=n_freq, f_max_THz=f_max_THz, window=window)
    return TrajectoryAnalysis(rdf=r, msd=m, vacf=v, vdos=d, diffusion=diffusion(m, dtau, fit=fit, vacf_result=v))
