"""The trajectory analysis on the device (csrc/trajectory.hip, alignn_amd/trajectory.py) against the restatement of
tests/traj_ref.py: (a) the pair histograms bit for bit, g(r) and n(r) to a few roundings, B = 3 in one launch - own images only,
a strongly skewed cell, more than one tile of rows, the chunked pair types; (b) MSD and VACF under a bound derived from the
number of terms; (c) the density of states, the Einstein fit and the Green-Kubo integral on the outputs of (b); (d) ``run_md``
then ``analyze_md``, on the pair potential of tests/pair_ref.py (NVE and NPT with per-frame cells) and through the model.
Everywhere: a structure alone, and the batch rotated, give the batch's bits."""

import numpy as np
import pytest
import torch

from alignn_amd import analyze_md, diffusion, green_kubo, msd, rdf, run_md, vacf, vdos
from tests import pair_ref
from tests import traj_ref as ref
from tests.sim_gpu import DEV, _crystals, _model, _t

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -53
RDF_RTOL = 8 * EPS  # g and n(r): a handful of correctly rounded operations on exact integers
# (c): the largest deviations measured on an MI355X (each test's docstring says of what), and the bounds: 10 x, capped at 1e-9
VDOS_MEASURED = 1.43e-16
FIT_MEASURED = 3.47e-15
GK_MEASURED = 0.0  # the running sum is sequential on both sides: the same bits, and 10 x 0 is 0: equality
VDOS_RTOL, FIT_RTOL, GK_RTOL = (min(10.0 * m, 1e-9) for m in (VDOS_MEASURED, FIT_MEASURED, GK_MEASURED))

SIZES = [1, 5, 70]
SPECIES = [np.array([14]), np.array([8, 3, 8, 3, 3]), np.array([22, 8, 38] * 23 + [8])]
CELLS = np.array([[[3.15, 0.0, 0.0], [0.4, 3.15, 0.0], [0.3, -0.35, 3.2]],
                  [[4.0, 0.0, 0.0], [1.3, 3.8, 0.0], [0.7, -0.9, 4.4]],
                  [[13.0, 0.0, 0.0], [0.6, 13.5, 0.0], [-0.4, 0.5, 14.0]]])
R_MAX = 6.0
PTR = np.concatenate([[0], np.cumsum(SIZES)])
_CACHE = {}


def _rows(b):
    return slice(PTR[b], PTR[b + 1])


def _rdf_inputs():
    """F = 3 frames of random fractional positions, moved by whole cells (-2 .. 2 per axis) and by N(0, 0.05 A) noise, in the
    fixed cells and in per-frame cells that differ from them by a few percent."""
    if "rdf" not in _CACHE:
        rng = np.random.default_rng(11)
        F = 3
        grow = np.array([1.0, 1.03, 0.97])
        shear = rng.normal(0.0, 0.01, (F, 3, 3, 3))
        per_frame = np.stack([[grow[f] * (CELLS[b] + shear[f, b] * (f > 0)) for b in range(3)] for f in range(F)])  # [F, B, 3, 3]
        fixed, moving = np.zeros((F, PTR[-1], 3)), np.zeros((F, PTR[-1], 3))
        for b, n in enumerate(SIZES):
            for f in range(F):
                frac = rng.uniform(0, 1, (n, 3)) + rng.integers(-2, 3, (n, 3))
                noise = rng.normal(0.0, 0.05, (n, 3))
                fixed[f, _rows(b)] = frac @ CELLS[b] + noise
                moving[f, _rows(b)] = frac @ per_frame[f, b] + noise
        _CACHE["rdf"] = fixed, moving, per_frame
    return _CACHE["rdf"]


def _rdf_want(traj, cells, n_bins, frames):
    """The restatement per structure, once per case: [(counts, g, coord, V, centres)]."""
    key = ("want", id(traj), n_bins, frames)
    if key not in _CACHE:
        out, margin, pairs = [], np.inf, 0
        for b, n in enumerate(SIZES):
            rank, _ = ref.groups(SPECIES[b], n)
            S = int(rank.max())
            cb = cells[b] if cells.ndim == 3 else cells[list(frames), b]
            counts, m, p = ref.rdf_counts(traj[list(frames), _rows(b)], cb, rank, S, R_MAX, n_bins)
            margin, pairs = min(margin, m), pairs + p
            out.append((counts,) + ref.rdf_normalise(counts, cb, len(frames), ref.group_counts(rank, S), R_MAX))
        print(f"rdf n_bins {n_bins} frames {list(frames)}: {pairs} pairs, smallest margin {margin:.2e} bin widths")
        _CACHE[key] = out
    return _CACHE[key]


def _close(got, want, rtol):
    return bool((np.abs(got - want) <= rtol * np.abs(want)).all())


CASES = [("fixed", 50, None), ("fixed", 67, None), ("fixed", 4096, None), ("moving", 67, None), ("moving", 50, (1, 2)),
         ("fixed", 4096, (1, 2))]


# --- (a) the radial distribution function ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cells_kind,n_bins,select", CASES)
def test_rdf_counts_match_the_restatement_bit_for_bit(cells_kind, n_bins, select):
    """The geometry is what the restatement's precondition allows: no pair within 1e-9 bin widths of a bin edge or of r_max (the
    smallest margin of these seeds: printed).  n_bins = 4096 with three species is six pair types of 4096 bins: more than the
    LDS histogram holds, so the types go in two chunks."""
    fixed, moving, per_frame = _rdf_inputs()
    assert ref.image_range(CELLS[0], R_MAX) == [2, 2, 2] and ref.image_range(CELLS[1], R_MAX) == [2, 2, 1]
    assert ref.image_range(CELLS[2], R_MAX) == [0, 0, 0]
    traj, cells = (fixed, CELLS) if cells_kind == "fixed" else (moving, per_frame)
    sel = dict(start=select[0], step=select[1]) if select else {}
    frames = tuple(range(3)[slice(sel.get("start"), None, sel.get("step"))])
    want = _rdf_want(traj, cells, n_bins, frames)
    t_traj, t_cells = _t(traj), _t(cells)
    res = rdf(t_traj, t_cells, SIZES, SPECIES, r_max=R_MAX, n_bins=n_bins, **sel)
    assert res.n_frames == len(frames) and res.counts.shape == (3, 7, n_bins) and res.counts.dtype == torch.int64
    assert res.species == [[14], [3, 8], [8, 22, 38]]
    counts, g, coord = res.counts.cpu().numpy(), res.g.cpu().numpy(), res.coordination.cpu().numpy()
    assert (counts[:, 0] == counts[:, 1:].sum(1)).all()
    for b in range(3):
        wc, wg, wn, wv, wr = want[b]
        P = wc.shape[0]
        assert np.array_equal(counts[b, :P], wc), (b, np.abs(counts[b, :P] - wc).sum())
        assert not counts[b, P:].any() and not g[b, P:].any() and not coord[b, P:].any()  # the rows of species it has not
        assert wc[0].sum() > 0
        assert _close(g[b, :P], wg, RDF_RTOL) and _close(coord[b, :P], wn, RDF_RTOL), b
        assert _close(res.volume[b].item(), wv, RDF_RTOL)
    assert _close(res.r.cpu().numpy(), want[0][4], RDF_RTOL)
    # alone, and rotated: the batch's bits
    for b in range(3):
        lat_b = t_cells[b:b + 1] if t_cells.ndim == 3 else t_cells[:, b:b + 1]
        alone = rdf(t_traj[:, _rows(b)], lat_b, [SIZES[b]], [SPECIES[b]], r_max=R_MAX, n_bins=n_bins, **sel)
        P = alone.counts.shape[1]
        assert torch.equal(alone.counts[0], res.counts[b, :P]) and torch.equal(alone.g[0], res.g[b, :P]), b
        assert torch.equal(alone.coordination[0], res.coordination[b, :P]) and torch.equal(alone.volume[0], res.volume[b]), b
    order = [2, 0, 1]
    rot_traj = torch.cat([t_traj[:, _rows(b)] for b in order], dim=1)
    rot_cells = t_cells[order] if t_cells.ndim == 3 else t_cells[:, order]
    rot = rdf(rot_traj, rot_cells, [SIZES[b] for b in order], [SPECIES[b] for b in order], r_max=R_MAX, n_bins=n_bins, **sel)
    for at, b in enumerate(order):
        assert torch.equal(rot.counts[at], res.counts[b]) and torch.equal(rot.g[at], res.g[b]), b
        assert torch.equal(rot.coordination[at], res.coordination[b]), b


def test_rdf_refuses_a_cell_that_needs_too_many_images_and_one_group_without_species():
    fixed, _, _ = _rdf_inputs()
    t_traj = _t(fixed)
    small = CELLS.copy()
    small[0] *= 0.2  # heights of ~0.63 A: r_max = 6 needs ten images
    assert max(ref.image_range(small[0], R_MAX)) > 8
    with pytest.raises(ValueError, match="images"):
        rdf(t_traj, _t(small), SIZES, SPECIES, r_max=R_MAX, n_bins=50)
    with pytest.raises(ValueError, match="at most 8"):
        rdf(t_traj, _t(CELLS), SIZES, [SPECIES[0], SPECIES[1], np.arange(70) % 9], r_max=R_MAX, n_bins=50)
    one = rdf(t_traj, _t(CELLS), SIZES, None, r_max=R_MAX, n_bins=50)
    full = rdf(t_traj, _t(CELLS), SIZES, SPECIES, r_max=R_MAX, n_bins=50)
    assert one.counts.shape == (3, 2, 50) and torch.equal(one.counts[:, 0], full.counts[:, 0])
    assert torch.equal(one.counts[:, 1], one.counts[:, 0]) and torch.equal(one.g[:, 0], full.g[:, 0])
    none = rdf(t_traj, _t(CELLS), SIZES, SPECIES, r_max=R_MAX, n_bins=50, start=3)  # no frame selected: zeros
    assert none.n_frames == 0 and not none.counts.any() and not none.g.any() and not none.coordination.any()


# --- (b) MSD and VACF ---------------------------------------------------------------------------------------------------------------
def _walk(F):
    """Random-walk positions, Gaussian momenta, non-uniform masses for the three sizes."""
    if ("walk", F) not in _CACHE:
        rng = np.random.default_rng(100 + F)
        N = PTR[-1]
        masses = [rng.uniform(1.0, 100.0, n) for n in SIZES]
        pos = rng.uniform(0, 10, (1, N, 3)) + np.cumsum(rng.normal(0.0, 0.15, (F, N, 3)), axis=0)
        mom = rng.normal(0.0, 1.0, (F, N, 3)) * np.sqrt(np.concatenate(masses))[None, :, None]
        _CACHE[("walk", F)] = pos, mom, masses
    return _CACHE[("walk", F)]


def _check_msd(got, pos, masses, K, stride, remove_com):
    """[B, S + 1, K + 1, 3] against the restatement per structure: every term is >= 0 and the same bits on both sides, so a sum of
    m terms in any order is within (m + 8) 2^-53 of the true one, relatively."""
    worst = 0.0
    for b, n in enumerate(SIZES):
        rank, _ = ref.groups(SPECIES[b], n)
        S = int(rank.max())
        want, terms = ref.msd(pos[:, _rows(b)], rank, S, masses[b], K, stride, remove_com)
        g = got[b, :S + 1]
        assert not got[b, S + 1:].any()
        bound = (terms[..., None] + 8) * EPS * want
        assert (np.abs(g - want) <= bound).all(), (b, np.abs(g - want).max())
        nz = want > 0
        worst = max(worst, float((np.abs(g - want)[nz] / want[nz]).max()) if nz.any() else 0.0)
    return worst


def _check_vacf(got, mom, masses, K, stride):
    worst = 0.0
    for b, n in enumerate(SIZES):
        rank, _ = ref.groups(SPECIES[b], n)
        S = int(rank.max())
        want, mag, terms = ref.vacf(mom[:, _rows(b)], rank, S, masses[b], K, stride)
        g = got[b, :S + 1]
        assert not got[b, S + 1:].any()
        assert (np.abs(g - want) <= (terms + 8) * EPS * mag).all(), (b, np.abs(g - want).max())
        worst = max(worst, float((np.abs(g - want) / mag).max()))
    return worst


@pytest.mark.parametrize("F", [9, 33])
def test_msd_and_vacf_within_the_summation_bound(F):
    pos, mom, masses = _walk(F)
    t_pos, t_mom = _t(pos), _t(mom)
    for K in (F - 1, 4):
        for stride in (1, 3):
            v = vacf(t_mom, SIZES, SPECIES, masses, max_lag=K, origin_stride=stride)
            assert v.vacf.shape == (3, 4, K + 1) and list(v.n_origins) == [ref.n_origins(F, k, stride) for k in range(K + 1)]
            wv = _check_vacf(v.vacf.cpu().numpy(), mom, masses, K, stride)
            for remove_com in (True, False):
                m = msd(t_pos, SIZES, SPECIES, masses, max_lag=K, origin_stride=stride, remove_com=remove_com)
                assert m.msd.shape == (3, 4, K + 1, 3) and torch.equal(m.total, (m.msd[..., 0] + m.msd[..., 1]) + m.msd[..., 2])
                wm = _check_msd(m.msd.cpu().numpy(), pos, masses, K, stride, remove_com)
                print(f"F {F} K {K} stride {stride} com {remove_com}: msd rel {wm:.2e}, vacf / magnitude {wv:.2e}")
                if remove_com:
                    assert float(m.msd[0].abs().max()) < 1e-24  # one atom is its own centre of mass (to the rounding of m x / m)
                # alone and rotated: the batch's bits
                for b in range(3):
                    S = len(set(SPECIES[b].tolist()))
                    a = msd(t_pos[:, _rows(b)], [SIZES[b]], [SPECIES[b]], [masses[b]], max_lag=K, origin_stride=stride,
                            remove_com=remove_com)
                    assert torch.equal(a.msd[0], m.msd[b, :S + 1]), (b, K, stride, remove_com)
            for b in range(3):
                S = len(set(SPECIES[b].tolist()))
                a = vacf(t_mom[:, _rows(b)], [SIZES[b]], [SPECIES[b]], [masses[b]], max_lag=K, origin_stride=stride)
                assert torch.equal(a.vacf[0], v.vacf[b, :S + 1]), (b, K, stride)
    order = [1, 2, 0]
    cat = lambda t: torch.cat([t[:, _rows(b)] for b in order], dim=1)
    sub = lambda xs: [xs[b] for b in order]
    m = msd(t_pos, SIZES, SPECIES, masses, max_lag=4, origin_stride=3)
    v = vacf(t_mom, SIZES, SPECIES, masses, max_lag=4, origin_stride=3)
    rm = msd(cat(t_pos), sub(SIZES), sub(SPECIES), sub(masses), max_lag=4, origin_stride=3)
    rv = vacf(cat(t_mom), sub(SIZES), sub(SPECIES), sub(masses), max_lag=4, origin_stride=3)
    for at, b in enumerate(order):
        assert torch.equal(rm.msd[at], m.msd[b]) and torch.equal(rv.vacf[at], v.vacf[b]), b
    # a frame selection is the analysis of the selected frames
    sel = msd(t_pos, SIZES, SPECIES, masses, start=1, step=2)
    direct = msd(t_pos[1::2].contiguous(), SIZES, SPECIES, masses)
    assert sel.msd.shape[2] == (F - 1) // 2 and torch.equal(sel.msd, direct.msd)
    with pytest.raises(ValueError, match="max_lag"):
        msd(t_pos, SIZES, SPECIES, masses, max_lag=F)
    with pytest.raises(ValueError, match="masses"):
        msd(t_pos, SIZES, SPECIES, None)
    no_species = msd(t_pos, SIZES, None, masses, max_lag=4)
    assert no_species.msd.shape == (3, 2, 5, 3) and torch.equal(no_species.msd[:, 0], no_species.msd[:, 1])
    assert torch.equal(no_species.msd[:, 0], msd(t_pos, SIZES, SPECIES, masses, max_lag=4).msd[:, 0])


# --- (c) density of states, Einstein fit, Green-Kubo ------------------------------------------------------------------------------------
def _relative(got, want, scale):
    """max |got - want| / scale over the entries with a scale; where the scale is zero both must be zero."""
    scale = np.broadcast_to(scale, want.shape)
    zero = scale == 0
    assert not got[zero].any() and not want[zero].any()
    return float((np.abs(got - want)[~zero] / scale[~zero]).max())


def _check_vdos(v_dev, dtau, n_freq, f_max, window):
    got = vdos(v_dev, dtau, n_freq=n_freq, f_max_THz=f_max, window=window)
    want, scale, nu = ref.vdos(v_dev.cpu().numpy(), dtau, n_freq, f_max, window)
    assert np.array_equal(got.freq_THz.cpu().numpy(), nu)
    return _relative(got.dos.cpu().numpy(), want, scale[..., None])


def _check_fit(m_dev, dtau, lo, hi):
    d = diffusion(m_dev, dtau, fit=(lo, hi))
    want = ref.fit(m_dev.cpu().numpy(), dtau, lo, hi)  # [B, G, 4, 4]
    worst = 0.0
    for at, name in enumerate(("slope", "intercept", "stderr", "D")):
        g, w = getattr(d, name).cpu().numpy(), want[..., at]
        big = np.abs(w).max()
        worst = max(worst, float(np.abs(g - w).max() / big) if big > 0 else float(np.abs(g).max()))
    return worst


def _check_gk(v_dev, dtau):
    got = green_kubo(v_dev, dtau).cpu().numpy()
    want = ref.green_kubo(v_dev.cpu().numpy(), dtau)
    run = np.maximum.accumulate(np.abs(want), axis=-1).max(-1, keepdims=True)  # the row's largest value
    return _relative(got, want, np.broadcast_to(run, want.shape))


def test_vdos_fit_and_green_kubo_match_the_restatement_on_the_device_outputs():
    """On the MSD and VACF of the F = 33 walk.  The device's cos is not numpy's and its sums have another order, so the bounds
    are measured: the largest deviation of D(nu) relative to 2 dtau sum_k |c_k w_k C(k) / C(0)| (``VDOS_MEASURED``), of the
    fit's slope, intercept, standard error and D relative to the largest magnitude of each (``FIT_MEASURED``) and of the running
    integral relative to the row's largest value (``GK_MEASURED``), on an MI355X; 10 x that is allowed, 1e-9 at the most.
    Measured: density of states 1.42e-16, fit 3.46e-15, Green-Kubo 0."""
    pos, mom, masses = _walk(33)
    m = msd(_t(pos), SIZES, SPECIES, masses)
    v = vacf(_t(mom), SIZES, SPECIES, masses)
    dtau = 2.0
    dv = max(_check_vdos(v.vacf, dtau, 40, 50.0, w) for w in ("hann", "none"))
    df = max(_check_fit(m.msd, dtau, lo, hi) for lo, hi in ((4, 32), (0, 32), (1, 3)))
    dg = _check_gk(v.vacf, dtau)
    print(f"measured: vdos {dv:.3e}, fit {df:.3e}, green-kubo {dg:.3e}")
    assert dv <= VDOS_RTOL and df <= FIT_RTOL and dg <= GK_RTOL, (dv, df, dg)
    two = diffusion(m, dtau, fit=(3, 4))
    assert not two.stderr.any() and two.green_kubo is None  # two points: no residual
    both = diffusion(m, dtau, fit=(4, 32), vacf_result=v)
    assert torch.equal(both.green_kubo, green_kubo(v, dtau))
    slope, D = both.slope.cpu().numpy(), both.D.cpu().numpy()  # (on the host: torch divides by a scalar through its reciprocal)
    assert np.array_equal(D[..., :3], slope[..., :3] / 2.0) and np.array_equal(D[..., 3], slope[..., 3] / 6.0)
    for bad in (dict(fit=(4, 4)), dict(fit=(-1, 4)), dict(fit=(0, 33))):
        with pytest.raises(ValueError, match="fit"):
            diffusion(m, dtau, **bad)
    with pytest.raises(ValueError, match="window"):
        vdos(v, dtau, window="blackman")
    with pytest.raises(ValueError, match="n_freq"):
        vdos(v, dtau, n_freq=1)


# --- (d) end to end -----------------------------------------------------------------------------------------------------------------
def _check_analysis(an, res, lattices, ns, species, masses, dtau, r_max, n_bins, K, fit, f_max):
    """``analyze_md``'s results against the restatement applied to the run's own tensors copied to the host, under the bounds of
    (a) - (c)."""
    pos, mom = res.traj_positions.cpu().numpy(), res.traj_momenta.cpu().numpy()
    cells = res.traj_lattices.cpu().numpy() if res.traj_lattices is not None else np.stack(lattices)
    F = pos.shape[0]
    ptr = np.concatenate([[0], np.cumsum(ns)])
    counts, g, coord = an.rdf.counts.cpu().numpy(), an.rdf.g.cpu().numpy(), an.rdf.coordination.cpu().numpy()
    m_got, v_got = an.msd.msd.cpu().numpy(), an.vacf.vacf.cpu().numpy()
    for b, n in enumerate(ns):
        rows = slice(ptr[b], ptr[b + 1])
        rank, _ = ref.groups(None if species is None else species[b], n)
        S = int(rank.max())
        cb = cells[b] if cells.ndim == 3 else cells[:, b]
        wc, _, _ = ref.rdf_counts(pos[:, rows], cb, rank, S, r_max, n_bins)
        wg, wn, wv, _ = ref.rdf_normalise(wc, cb, F, ref.group_counts(rank, S), r_max)
        P = wc.shape[0]
        assert np.array_equal(counts[b, :P], wc) and wc[0].sum() > 0, b
        assert _close(g[b, :P], wg, RDF_RTOL) and _close(coord[b, :P], wn, RDF_RTOL), b
        wm, terms = ref.msd(pos[:, rows], rank, S, masses[b], K, 1, True)
        assert (np.abs(m_got[b, :S + 1] - wm) <= (terms[..., None] + 8) * EPS * wm).all(), b
        wvacf, mag, terms = ref.vacf(mom[:, rows], rank, S, masses[b], K, 1)
        assert (np.abs(v_got[b, :S + 1] - wvacf) <= (terms + 8) * EPS * mag).all(), b
    want, scale, _ = ref.vdos(v_got, dtau, an.vdos.dos.shape[-1], f_max, "hann")
    dv = _relative(an.vdos.dos.cpu().numpy(), want, scale[..., None])
    wfit = ref.fit(m_got, dtau, *fit)
    df = max(float(np.abs(getattr(an.diffusion, name).cpu().numpy() - wfit[..., at]).max() / np.abs(wfit[..., at]).max())
             for at, name in enumerate(("slope", "intercept", "stderr", "D")))
    wgk = ref.green_kubo(v_got, dtau)
    dg = float(np.abs(an.diffusion.green_kubo.cpu().numpy() - wgk).max() / np.abs(wgk).max())
    print(f"analyze_md: vdos {dv:.3e}, fit {df:.3e}, green-kubo {dg:.3e}")
    assert dv <= VDOS_RTOL and df <= FIT_RTOL and dg <= GK_RTOL, (dv, df, dg)
    for t in (an.rdf.g, an.rdf.coordination, an.msd.msd, an.vacf.vacf, an.vdos.dos, an.diffusion.D, an.diffusion.green_kubo):
        assert bool(torch.isfinite(t).all())


def _fcc32(a, rng, noise):
    base = np.array([[0, 0, 0], [0, 0.5, 0.5], [0.5, 0, 0.5], [0.5, 0.5, 0]])
    cells = np.array([[i, j, k] for i in range(2) for j in range(2) for k in range(2)])
    return 2 * a * np.eye(3), (cells[:, None, :] + base[None, :, :]).reshape(-1, 3) * a + rng.normal(0.0, noise, (32, 3))


@pytest.mark.parametrize("ensemble", ["nve", "npt_berendsen"])
def test_run_md_then_analyze_md_on_the_fcc_morse_crystal(ensemble):
    """Two 32-atom fcc crystals (a = 0.97 and 0.99 x 2.9 x sqrt 2 A, the second with two species by name only) under the pair
    potential, 40 steps of 2 fs from 300 K recorded every second step: 21 frames, dtau = 4 fs."""
    rng = np.random.default_rng(5)
    rc = 5.0
    npt = ensemble == "npt_berendsen"
    lats, pos = zip(*[_fcc32(s * pair_ref.R0 * np.sqrt(2.0), rng, 0.02) for s in (0.97, 0.99)])
    ns, masses = [32, 32], [np.full(32, 26.98), np.where(np.arange(32) % 4 == 0, 58.69, 26.98)]
    species = [np.full(32, 13), np.where(np.arange(32) % 4 == 0, 28, 13)]
    kw = dict(pressure=0.0, compressibility=1e-6, taut=50.0, taup=200.0, temperature_K=300.0) if npt else {}
    res = run_md(None, list(lats), list(pos), None, masses, ensemble=ensemble, timestep=2.0, steps=40, interval=2,
                 initial_temperature_K=300.0, seed=[3, 4], forces_fn=pair_ref.make_forces_fn(rc, stress=npt), device=DEV, **kw)
    assert res.traj_positions.shape == (21, 64, 3) and (res.traj_lattices is not None) == npt
    an = analyze_md(res, list(lats), ns, species, masses, timestep=2.0, interval=2, r_max=6.0, n_bins=60, fit=(5, 20), n_freq=64,
                    f_max_THz=25.0)
    assert an.rdf.counts.shape == (2, 4, 60) and an.msd.msd.shape == (2, 3, 21, 3) and an.vdos.dos.shape == (2, 3, 64)
    _check_analysis(an, res, lats, ns, species, masses, 4.0, 6.0, 60, 20, (5, 20), 25.0)
    # a solid: twelve nearest neighbours under the first peak (3.4 A lies between the first two shells, 2.8 and 4.0 A)
    k = int(np.floor(3.4 / 0.1)) - 1
    assert float((an.rdf.coordination[:, 0, k] - 12.0).abs().max()) < 0.5
    if npt:
        assert not torch.equal(res.traj_lattices[0], res.traj_lattices[-1])  # the per-frame cells were used, and they moved
    # a tensor of fixed cells in place of the list; a frame selection doubles dtau
    half = analyze_md(res, _t(np.stack(lats)), ns, species, masses, timestep=2.0, interval=2, r_max=6.0, n_bins=60, step=2)
    assert half.msd.msd.shape[2] == 11 and half.diffusion.fit == (5, 10)
    assert torch.equal(half.msd.msd, msd(res.traj_positions, ns, species, masses, step=2).msd)
    assert torch.equal(half.diffusion.green_kubo, green_kubo(half.vacf, 8.0))


def test_analyze_md_through_the_model_and_without_a_trajectory():
    lats, pos, feats = _crystals(2, 24)
    ns = [24, 26]
    masses = [np.random.default_rng(i).uniform(1.0, 100.0, n) for i, n in enumerate(ns)]
    species = [np.arange(n) % 3 + 1 for n in ns]
    model = _model()
    res = run_md(model, lats, pos, feats, masses, ensemble="nve", timestep=0.5, steps=5, interval=1, initial_temperature_K=300.0)
    lat_np = [np.asarray(l, dtype=np.float64) for l in lats]
    r_max = 4.0
    an = analyze_md(res, lats, ns, species, masses, timestep=0.5, interval=1, r_max=r_max, n_bins=40, fit=(1, 5), n_freq=16)
    _check_analysis(an, res, lat_np, ns, species, masses, 0.5, r_max, 40, 5, (1, 5), 30.0)
    bare = run_md(model, lats, pos, feats, masses, ensemble="nve", timestep=0.5, steps=1, trajectory=False)
    with pytest.raises(ValueError, match="trajectory=True"):
        analyze_md(bare, lats, ns, species, masses, timestep=0.5)
