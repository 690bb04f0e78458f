"""The van Hove analysis on the device (csrc/vanhove.hip, alignn_amd/vanhove.py) against the restatement of tests/vanhove_ref.py,
at the shapes of tests/test_gpu_trajectory.py - one atom, a few atoms, more than one tile of 64 rows; cells with image ranges
[2, 2, 2], [2, 2, 1] and [0, 0, 0] at r_max = 6 - on frames in which atoms jump by whole cells: (a) the self part: histograms bit
for bit with nothing dropped, the moments under a bound derived from the number of terms, alpha_2, the normalisations, F_s;
(b) the distinct part: histograms bit for bit, the atom's own displaced image left out, g; the intermediate scattering function
per vector and per shell under a measured bound; (c) against ``rdf``, ``msd`` and ``structure_factor``; (d) the refusals of the
host; (e) ``run_md``, then all three functions.  Everywhere: a structure alone, and the batch rotated, give
the batch's bits."""

import numpy as np
import pytest
import torch

from alignn_amd import intermediate_scattering, msd, rdf, run_md, structure_factor, van_hove_distinct, van_hove_self
from tests import pair_ref
from tests import traj_ref
from tests import vanhove_ref as ref
from tests.sim_gpu import DEV, _t

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -53
NORM_RTOL = 8 * EPS  # p, gs, g, volume, centres: a handful of correctly rounded operations on exact integers
# F_s: the largest deviation from the restatement measured on an MI355X, relative to 1 (every term is at most 1 in magnitude); the
# device's sin is not numpy's and its sum has another order.  The bound: 10 x that, capped at 1e-9.
FS_MEASURED = 2.22e-16  # (the synthetic cases: 1.11e-16; the run_md trajectory: 2.22e-16)
FS_TOL = min(10.0 * FS_MEASURED, 1e-9)
# F(q, t): the largest deviation of ``f_vectors`` and of ``f`` from the restatement measured on an MI355X, relative to
# sum_t |rho'| |rho| / (n_origins sqrt(N_a N_b)) of the restatement (for ``f``: its mean over the shell) - the device's sincospi is
# not numpy's cos and sin, and the sums have another order.  The bound: 10 x that, capped at 1e-9.
FQT_MEASURED = 8.30e-13  # (the synthetic cases: 9.27e-14; the run_md crystal, whose modes nearly cancel off the Bragg peaks: 8.29e-13)
FQT_TOL = min(10.0 * FQT_MEASURED, 1e-9)

SIZES, SPECIES, FIVE, CELLS, R_MAX, PTR = ref.SIZES, ref.SPECIES, ref.FIVE, ref.CELLS, ref.R_MAX, ref.PTR
F, LAGS, Q, Q_MAX, Q_BINS = ref.FRAMES, ref.LAGS, ref.Q, ref.Q_MAX, ref.Q_BINS
_inputs, _selected, _rows = ref.inputs, ref.selected, ref.rows
_CACHE = {}


def _close(got, want, rtol):
    return bool((np.abs(got - want) <= rtol * np.abs(want)).all())


# --- (a) the self part ------------------------------------------------------------------------------------------------------------------
SELF_FIELDS = ("counts", "overflow", "p", "gs", "moments", "alpha2", "fs")
SELF_CASES = [(50, 1, None, True, "three"), (4096, 3, None, False, "three"), (50, 3, (1, 2), True, "three"), (4096, 1, None, True, "five")]


def _self_want(n_bins, stride, select, remove_com, species):
    key = ("self", n_bins, stride, select, remove_com, id(species))
    if key not in _CACHE:
        traj, masses = _inputs()
        _, frames, lags = _selected(select)
        out, margin, terms = [], np.inf, 0
        for b, n in enumerate(SIZES):
            rank, _ = traj_ref.groups(species[b], n)
            S = int(rank.max())
            w, m, t = ref.self_part(traj[frames, _rows(b)], rank, S, masses[b], lags, stride, remove_com, R_MAX, n_bins, Q)
            margin, terms = min(margin, m), terms + t
            out.append((w, traj_ref.group_counts(rank, S)))
        print(f"self n_bins {n_bins} stride {stride} frames {frames} com {remove_com}: {terms} terms, smallest margin {margin:.2e} bin widths")
        assert margin > ref.EDGE_MARGIN, f"a displacement lies {margin:.3e} bin widths from a bin edge: choose another seed"
        _CACHE[key] = out
    return _CACHE[key]


def _check_self(res, want, n_frames, lags, stride):
    """-> the largest deviation of fs from the restatement"""
    counts, overflow = res.counts.cpu().numpy(), res.overflow.cpu().numpy()
    moments, a2, fs = res.moments.cpu().numpy(), res.alpha2.cpu().numpy(), res.fs.cpu().numpy()
    p, gs = res.p.cpu().numpy(), res.gs.cpu().numpy()
    assert (counts[:, 0] == counts[:, 1:].sum(1)).all() and (overflow[:, 0] == overflow[:, 1:].sum(1)).all()
    worst = 0.0
    for b, (w, count) in enumerate(want):
        G = len(count)
        assert np.array_equal(counts[b, :G], w["counts"]) and np.array_equal(overflow[b, :G], w["overflow"]), b
        n_or = np.array([traj_ref.n_origins(n_frames, k, stride) for k in lags])
        assert np.array_equal(counts[b, :G].sum(-1) + overflow[b, :G], count[:, None] * n_or[None, :]), b  # nothing is dropped
        for t in (counts, overflow, moments, a2, fs, p, gs):
            assert not t[b, G:].any()  # the rows of species it has not
        assert (np.abs(moments[b, :G] - w["moments"]) <= (w["terms"][..., None] + 8) * EPS * w["moments"]).all(), b
        wa = ref.alpha2(moments[b, :G])  # on the device's own moments
        assert (np.abs(a2[b, :G] - wa) <= 8 * EPS * (np.abs(wa) + 1.0)).all(), b
        wp, wg, wr = ref.self_normalise(w["counts"], n_frames, lags, stride, count, res.r_max)
        assert _close(p[b, :G], wp, NORM_RTOL) and _close(gs[b, :G], wg, NORM_RTOL), b
        assert _close(res.r.cpu().numpy(), wr, NORM_RTOL)
        worst = max(worst, float(np.abs(fs[b, :G] - w["fs"]).max()))
    return worst


@pytest.mark.parametrize("n_bins,stride,select,remove_com,which", SELF_CASES)
def test_van_hove_self_matches_the_restatement(n_bins, stride, select, remove_com, which):
    """Histograms and overflow bit for bit, and their sum n_origins N_a exactly; the precondition - no displacement within 1e-9
    bin widths of an inner bin edge or of r_max - is asserted with the margin printed.  Moments: every term is >= 0 and the same
    bits on both sides, so a sum of m terms in any order is within (m + 8) 2^-53 of the true one, relatively.  ``fs`` against
    ``FS_TOL``; measured on an MI355X: the largest |fs - restatement| of these cases, printed here."""
    traj, masses = _inputs()
    species = SPECIES if which == "three" else FIVE
    sel, frames, lags = _selected(select)
    want = _self_want(n_bins, stride, select, remove_com, species)
    t_traj = _t(traj)
    kw = dict(r_max=R_MAX, n_bins=n_bins, lags=lags, origin_stride=stride, remove_com=remove_com, q=Q, **sel)
    res = van_hove_self(t_traj, SIZES, species, masses if remove_com else None, **kw)
    G = 1 + max(len(set(s.tolist())) for s in species)
    assert res.counts.shape == (3, G, len(lags), n_bins) and res.counts.dtype == torch.int64 and res.fs.shape == (3, G, len(lags), 3)
    assert list(res.n_origins) == [traj_ref.n_origins(len(frames), k, stride) for k in lags] and list(res.lags) == list(lags)
    dev = _check_self(res, want, len(frames), lags, stride)
    print(f"measured: fs {dev:.3e}")
    assert dev <= FS_TOL
    assert float(res.overflow.sum()) > 0 and float(res.counts.sum()) > 0
    if remove_com:  # one atom is its own centre of mass (to the rounding of m x / m)
        assert float(res.moments[0].abs().max()) < 1e-24
    # alone, and rotated: the batch's bits
    for b in range(3):
        alone = van_hove_self(t_traj[:, _rows(b)], [SIZES[b]], [species[b]], [masses[b]] if remove_com else None, **kw)
        Gb = alone.counts.shape[1]
        for name in SELF_FIELDS:
            assert torch.equal(getattr(alone, name)[0], getattr(res, name)[b, :Gb]), (b, name)
    order = [2, 0, 1]
    rot = van_hove_self(torch.cat([t_traj[:, _rows(b)] for b in order], dim=1), [SIZES[b] for b in order], [species[b] for b in order],
                        [masses[b] for b in order] if remove_com else None, **kw)
    for at, b in enumerate(order):
        for name in SELF_FIELDS:
            assert torch.equal(getattr(rot, name)[at], getattr(res, name)[b]), (b, name)
    assert torch.equal(rot.r, res.r)


def test_van_hove_self_lag_range_and_one_group():
    traj, masses = _inputs()
    t_traj = _t(traj)
    full = van_hove_self(t_traj, SIZES, SPECIES, masses, r_max=R_MAX, n_bins=50, lags=LAGS)
    ranged = van_hove_self(t_traj, SIZES, SPECIES, masses, r_max=R_MAX, n_bins=50, max_lag=8)
    assert ranged.counts.shape[2] == 9 and ranged.fs is None and ranged.q is None
    for name in ("counts", "overflow", "moments", "alpha2", "p", "gs"):
        assert torch.equal(getattr(ranged, name)[:, :, list(LAGS)], getattr(full, name)), name
    assert int(full.counts[:, :, 0, 1:].sum()) == 0 and not full.moments[:, :, 0].any() and not full.alpha2[:, :, 0].any()  # lag 0
    one = van_hove_self(t_traj, SIZES, None, masses, r_max=R_MAX, n_bins=50, lags=LAGS)
    assert one.counts.shape == (3, 2, 4, 50) and torch.equal(one.counts[:, 0], full.counts[:, 0])
    assert torch.equal(one.counts[:, 1], one.counts[:, 0]) and torch.equal(one.moments[:, 0], full.moments[:, 0])
    # a frame selection is the analysis of the selected frames
    sel = van_hove_self(t_traj, SIZES, SPECIES, masses, r_max=R_MAX, n_bins=50, lags=(0, 1, 3), start=1, step=2)
    direct = van_hove_self(t_traj[1::2].contiguous(), SIZES, SPECIES, masses, r_max=R_MAX, n_bins=50, lags=(0, 1, 3))
    assert torch.equal(sel.counts, direct.counts) and torch.equal(sel.moments, direct.moments)


# --- (b) the distinct part --------------------------------------------------------------------------------------------------------------
DISTINCT_CASES = [(50, 1, None, False), (4096, 3, None, True), (50, 3, (1, 2), True)]


def _distinct_want(n_bins, stride, select, remove_com):
    key = ("distinct", n_bins, stride, select, remove_com)
    if key not in _CACHE:
        traj, masses = _inputs()
        _, frames, lags = _selected(select)
        out, margin, terms = [], np.inf, 0
        for b, n in enumerate(SIZES):
            rank, _ = traj_ref.groups(SPECIES[b], n)
            S = int(rank.max())
            counts, m, t = ref.distinct_counts(traj[frames, _rows(b)], CELLS[b], rank, S, masses[b], lags, stride, remove_com, R_MAX, n_bins)
            margin, terms = min(margin, m), terms + t
            g, V, centres = ref.distinct_normalise(counts, CELLS[b], len(frames), lags, stride, traj_ref.group_counts(rank, S), R_MAX)
            out.append((counts, g, V, centres))
        print(f"distinct n_bins {n_bins} stride {stride} frames {frames} com {remove_com}: {terms} terms, smallest margin {margin:.2e} bin widths")
        assert margin > ref.EDGE_MARGIN, f"a pair lies {margin:.3e} bin widths from a bin edge: choose another seed"
        _CACHE[key] = out
    return _CACHE[key]


@pytest.mark.parametrize("n_bins,stride,select,remove_com", DISTINCT_CASES)
def test_van_hove_distinct_matches_the_restatement_bit_for_bit(n_bins, stride, select, remove_com):
    """The precondition - no term within 1e-9 bin widths of a bin edge or of r_max - is asserted with the margin printed.
    n_bins = 4096 with three species is six pair rows of 4096 bins: more than the LDS histogram holds, so the rows go in two
    chunks.  In these frames most atoms have jumped by whole cells: the image left out for j = i is the one that undoes the
    wrap, not the image 0."""
    assert traj_ref.image_range(CELLS[0], R_MAX) == [2, 2, 2] and traj_ref.image_range(CELLS[1], R_MAX) == [2, 2, 1]
    assert traj_ref.image_range(CELLS[2], R_MAX) == [0, 0, 0]
    traj, masses = _inputs()
    sel, frames, lags = _selected(select)
    want = _distinct_want(n_bins, stride, select, remove_com)
    t_traj, t_cells = _t(traj), _t(CELLS)
    kw = dict(r_max=R_MAX, n_bins=n_bins, lags=lags, origin_stride=stride, remove_com=remove_com, **sel)
    res = van_hove_distinct(t_traj, t_cells, SIZES, SPECIES, masses if remove_com else None, **kw)
    assert res.counts.shape == (3, 7, len(lags), n_bins) and res.counts.dtype == torch.int64
    assert res.species == [[14], [3, 8], [8, 22, 38]] and list(res.n_origins) == [traj_ref.n_origins(len(frames), k, stride) for k in lags]
    counts, g = res.counts.cpu().numpy(), res.g.cpu().numpy()
    assert (counts[:, 0] == counts[:, 1:].sum(1)).all()
    for b in range(3):
        wc, wg, wv, wr = want[b]
        P = wc.shape[0]
        assert np.array_equal(counts[b, :P], wc), (b, np.abs(counts[b, :P] - wc).sum())
        assert not counts[b, P:].any() and not g[b, P:].any() and wc[0].sum() > 0
        assert _close(g[b, :P], wg, NORM_RTOL) and _close(res.volume[b].item(), wv, NORM_RTOL), b
    assert _close(res.r.cpu().numpy(), want[0][3], NORM_RTOL)
    for b in range(3):
        alone = van_hove_distinct(t_traj[:, _rows(b)], t_cells[b:b + 1], [SIZES[b]], [SPECIES[b]], [masses[b]] if remove_com else None, **kw)
        P = alone.counts.shape[1]
        assert torch.equal(alone.counts[0], res.counts[b, :P]) and torch.equal(alone.g[0], res.g[b, :P]), b
        assert torch.equal(alone.volume[0], res.volume[b])
    order = [2, 0, 1]
    rot = van_hove_distinct(torch.cat([t_traj[:, _rows(b)] for b in order], dim=1), t_cells[order], [SIZES[b] for b in order],
                            [SPECIES[b] for b in order], [masses[b] for b in order] if remove_com else None, **kw)
    for at, b in enumerate(order):
        assert torch.equal(rot.counts[at], res.counts[b]) and torch.equal(rot.g[at], res.g[b]) and torch.equal(rot.volume[at], res.volume[b]), b


def test_an_atom_that_moved_by_more_than_half_a_cell_leaves_out_its_own_displaced_image():
    """One atom in the small skewed cell, moved between two frames by the cell vector (1, -1, 0) and a bit, 4.2 A: the images
    of the moved atom around where it was are the lattice points shifted by the bit, all counted but the one that is the atom
    itself - the one at its unwrapped displacement, which ``van_hove_self`` bins.  The wrapped displacement, the bit, is the image
    that came in from the next cell: it counts."""
    C = CELLS[0]
    bit = np.array([0.21, -0.13, 0.08])
    x0 = np.array([[0.5, 0.7, 0.2]]) @ C
    move = np.array([1.0, -1.0, 0.0]) @ C + bit
    traj = np.stack([x0, x0 + move])
    n_bins = 60
    res = van_hove_distinct(_t(traj), _t(C[None]), [1], None, r_max=R_MAX, n_bins=n_bins, lags=(0, 1))
    counts = res.counts.cpu().numpy()[0]
    want, margin, _ = ref.distinct_counts(traj, C, np.ones(1, dtype=np.int64), 1, None, (0, 1), 1, False, R_MAX, n_bins)
    assert margin > ref.EDGE_MARGIN and np.array_equal(counts, want)
    static = rdf(_t(traj), _t(C[None]), [1], None, r_max=R_MAX, n_bins=n_bins).counts.cpu().numpy()[0]
    assert np.array_equal(counts[:, 0], static)  # lag 0: the atom's images around itself, in both frames
    # every lattice point shifted by the bit, by plain geometry (a range of 4 cells covers r_max with room to spare)
    m = np.array([[a, b, c] for a in range(-4, 5) for b in range(-4, 5) for c in range(-4, 5)], dtype=np.float64)
    r = np.sqrt((((m @ C) + bit) ** 2).sum(1))
    every = np.bincount(np.floor(r[r < R_MAX] * n_bins / R_MAX).astype(np.int64), minlength=n_bins)
    r_own = float(np.sqrt((move * move).sum()))
    assert 0.5 * min(np.linalg.norm(C, axis=1)) < r_own < R_MAX
    own = np.zeros(n_bins, dtype=np.int64)
    own[int(np.floor(r_own * n_bins / R_MAX))] = 1
    assert np.array_equal(counts[0, 1], every - own) and np.array_equal(counts[1, 1], counts[0, 1])
    assert counts[0, 1, int(np.floor(np.sqrt((bit * bit).sum()) * n_bins / R_MAX))] == 1  # the wrapped displacement counts
    s = van_hove_self(_t(traj), [1], None, None, r_max=R_MAX, n_bins=n_bins, lags=(1,), remove_com=False)
    assert np.array_equal(s.counts.cpu().numpy()[0, 0, 0], own)  # and the self part holds what was left out


# --- (b2) the intermediate scattering function -------------------------------------------------------------------------------------------
def _fqt_want(stride, select):
    key = ("fqt", stride, select)
    if key not in _CACHE:
        traj, _ = _inputs()
        _, frames, lags = _selected(select)
        out = []
        for b, n in enumerate(SIZES):
            rank, _ = traj_ref.groups(SPECIES[b], n)
            out.append(ref.intermediate_scattering(traj[frames, _rows(b)], CELLS[b], rank, int(rank.max()), Q_MAX, Q_BINS, lags, stride))
        _CACHE[key] = out
    return _CACHE[key]


def _check_fqt(res, want):
    """-> the largest deviation of f_vectors and of f from the restatement, relative to the restatement's scale"""
    worst = 0.0
    f, n_vectors = res.f.cpu().numpy(), res.n_vectors.cpu().numpy()
    for b, w in enumerate(want):
        P, V = w["f_vectors"].shape[0], len(w["hkl"])
        assert np.array_equal(res.hkl[b].cpu().numpy(), w["hkl"]) and np.array_equal(n_vectors[b], w["n_vectors"]), b
        got = res.f_vectors[b].cpu().numpy()
        assert got.shape[0] >= P and got.shape[1:] == w["f_vectors"].shape[1:] and not got[P:].any() and not f[b, P:].any()
        live = w["scale"] > 0
        assert not got[:P][~live].any() and not w["f_vectors"][~live].any()
        if live.any():
            worst = max(worst, float((np.abs(got[:P] - w["f_vectors"])[live] / w["scale"][live]).max()))
        shell_scale = np.stack([[np.bincount(w["shell_of"], weights=w["scale"][p, l], minlength=Q_BINS) for l in range(got.shape[1])]
                                for p in range(P)]) / np.maximum(w["n_vectors"], 1)
        live = shell_scale > 0
        assert not f[b, :P][~live].any()
        if live.any():
            worst = max(worst, float((np.abs(f[b, :P] - w["f"])[live] / shell_scale[live]).max()))
    assert _close(res.q.cpu().numpy(), want[0]["q"], NORM_RTOL)
    return worst


@pytest.mark.parametrize("stride,select", [(1, None), (3, None), (3, (1, 2))])
def test_intermediate_scattering_matches_the_restatement(stride, select):
    """q_max = 4.5 1/A: 13, 33 and about 1900 vectors - the large cell's are more than one workgroup's slab of 1024.  Measured on an
    MI355X: the largest deviation of ``f_vectors`` and ``f`` relative to the restatement's scale, printed here, against
    ``FQT_TOL``."""
    traj, _ = _inputs()
    sel, frames, lags = _selected(select)
    want = _fqt_want(stride, select)
    assert len(want[0]["hkl"]) > 8 and len(want[1]["hkl"]) > 20 and len(want[2]["hkl"]) > 1024
    t_traj, t_cells = _t(traj), _t(CELLS)
    kw = dict(q_max=Q_MAX, n_bins=Q_BINS, lags=lags, origin_stride=stride, **sel)
    res = intermediate_scattering(t_traj, t_cells, SIZES, SPECIES, **kw)
    assert res.f.shape == (3, 7, len(lags), Q_BINS) and res.n_vectors.dtype == torch.int64 and res.species == [[14], [3, 8], [8, 22, 38]]
    assert list(res.n_origins) == [traj_ref.n_origins(len(frames), k, stride) for k in lags]
    dev = _check_fqt(res, want)
    print(f"measured: fqt {dev:.3e}")
    assert dev <= FQT_TOL
    if stride == 1:  # lag 0 is S(q): the same terms in frame order, within the bound of a sum of F terms relative to its scale
        static = structure_factor(t_traj, t_cells, SIZES, SPECIES, q_max=Q_MAX, n_bins=Q_BINS, **sel)
        for b in range(3):
            assert torch.equal(static.hkl[b], res.hkl[b])
            P = want[b]["scale"].shape[0]
            diff = (static.s_vectors[b] - res.f_vectors[b][:, 0]).abs().cpu().numpy()[:P]
            assert (diff <= (len(frames) + 8) * EPS * want[b]["scale"][:, 0]).all(), b
        assert torch.equal(static.n_vectors, res.n_vectors) and torch.equal(static.q, res.q)
    for b in range(3):
        alone = intermediate_scattering(t_traj[:, _rows(b)], t_cells[b:b + 1], [SIZES[b]], [SPECIES[b]], **kw)
        P = alone.f.shape[1]
        assert torch.equal(alone.f[0], res.f[b, :P]) and torch.equal(alone.f_vectors[0], res.f_vectors[b][:P]), b
        assert torch.equal(alone.hkl[0], res.hkl[b]) and torch.equal(alone.n_vectors[0], res.n_vectors[b])
    order = [2, 0, 1]
    rot = intermediate_scattering(torch.cat([t_traj[:, _rows(b)] for b in order], dim=1), t_cells[order], [SIZES[b] for b in order],
                                  [SPECIES[b] for b in order], **kw)
    for at, b in enumerate(order):
        assert torch.equal(rot.f[at], res.f[b]) and torch.equal(rot.f_vectors[at], res.f_vectors[b]) and torch.equal(rot.hkl[at], res.hkl[b]), b


# --- (c) against the existing device functions ---------------------------------------------------------------------------------------------
def test_lag_zero_is_rdf_and_the_second_moment_is_msd():
    traj, masses = _inputs()
    t_traj, t_cells = _t(traj), _t(CELLS)
    for n_bins in (50, 4096):
        d = van_hove_distinct(t_traj, t_cells, SIZES, SPECIES, r_max=R_MAX, n_bins=n_bins, lags=[0], origin_stride=1)
        static = rdf(t_traj, t_cells, SIZES, SPECIES, r_max=R_MAX, n_bins=n_bins)
        assert torch.equal(d.counts[:, :, 0], static.counts) and int(static.counts.sum()) > 0
        assert _close(d.g[:, :, 0].cpu().numpy(), static.g.cpu().numpy(), NORM_RTOL)
    for stride, remove_com in ((1, True), (3, False)):
        s = van_hove_self(t_traj, SIZES, SPECIES, masses, r_max=R_MAX, n_bins=50, max_lag=8, origin_stride=stride, remove_com=remove_com)
        m = msd(t_traj, SIZES, SPECIES, masses, max_lag=8, origin_stride=stride, remove_com=remove_com)
        got, total = s.moments[..., 0].cpu().numpy(), m.total.cpu().numpy()
        counts = np.stack([np.concatenate([traj_ref.group_counts(traj_ref.groups(SPECIES[b], n)[0], 3)]) for b, n in enumerate(SIZES)])
        terms = counts[:, :, None] * np.asarray(s.n_origins)[None, None, :]
        # both are within (terms + 8) 2^-53 of their true sums; the terms of one are (dx^2 + dy^2) + dz^2 rounded, the other sums
        # three rounded means: 8 more roundings
        assert (np.abs(got - total) <= (2 * (terms + 8) + 8) * EPS * total).all(), (stride, remove_com)


# --- (d) what the host refuses -----------------------------------------------------------------------------------------------------------
def test_host_refusals():
    traj, masses = _inputs()
    t_traj, t_cells = _t(traj), _t(CELLS)
    kw = dict(r_max=R_MAX, n_bins=50)
    with pytest.raises(ValueError, match="per-frame lattice"):
        van_hove_distinct(t_traj, t_cells[None].repeat(F, 1, 1, 1), SIZES, SPECIES, lags=[0], **kw)
    small = CELLS.copy()
    small[0] *= 0.2  # heights of ~0.63 A: r_max = 6 needs ten images
    assert max(traj_ref.image_range(small[0], R_MAX)) > 8
    with pytest.raises(ValueError, match="images"):
        van_hove_distinct(t_traj, _t(small), SIZES, SPECIES, lags=[0], **kw)
    for bad in ([], [1, 1], [3, 1], [0, F], [-1, 2], list(range(F)) * 200):
        with pytest.raises(ValueError, match="lags"):
            van_hove_self(t_traj, SIZES, SPECIES, masses, lags=bad, **kw)
        with pytest.raises(ValueError, match="lags"):
            van_hove_distinct(t_traj, t_cells, SIZES, SPECIES, lags=bad, **kw)
    for bad in ([0.5], 3, "01"):
        with pytest.raises(TypeError, match="lags"):
            van_hove_self(t_traj, SIZES, SPECIES, masses, lags=bad, **kw)
    with pytest.raises(ValueError, match="max_lag"):
        van_hove_self(t_traj, SIZES, SPECIES, masses, max_lag=F, **kw)
    with pytest.raises(ValueError, match="not both"):
        van_hove_self(t_traj, SIZES, SPECIES, masses, lags=[0], max_lag=1, **kw)
    with pytest.raises(ValueError, match="masses"):
        van_hove_self(t_traj, SIZES, SPECIES, None, lags=[0], **kw)
    with pytest.raises(ValueError, match="masses"):
        van_hove_distinct(t_traj, t_cells, SIZES, SPECIES, None, lags=[0], remove_com=True, **kw)
    with pytest.raises(ValueError, match="q must be"):
        van_hove_self(t_traj, SIZES, SPECIES, masses, lags=[0], q=[0.1 * (u + 1) for u in range(17)], **kw)
    with pytest.raises(ValueError, match="q"):
        van_hove_self(t_traj, SIZES, SPECIES, masses, lags=[0], q=[1.0, -2.0], **kw)
    nine = [SPECIES[0], SPECIES[1], np.arange(70) % 9]
    with pytest.raises(ValueError, match="at most 8"):
        van_hove_self(t_traj, SIZES, nine, masses, lags=[0], **kw)
    with pytest.raises(ValueError, match="at most 8"):
        van_hove_distinct(t_traj, t_cells, SIZES, nine, lags=[0], **kw)
    with pytest.raises(ValueError, match="origin_stride"):
        van_hove_self(t_traj, SIZES, SPECIES, masses, lags=[0], origin_stride=0, **kw)
    with pytest.raises(ValueError, match="n_bins"):
        van_hove_distinct(t_traj, t_cells, SIZES, SPECIES, lags=[0], r_max=R_MAX, n_bins=4097)
    with pytest.raises(ValueError, match="empty"):  # as msd
        van_hove_self(t_traj, SIZES, SPECIES, masses, lags=[0], start=F, **kw)
    with pytest.raises(ValueError, match="empty"):
        van_hove_distinct(t_traj, t_cells, SIZES, SPECIES, lags=[0], start=F, **kw)
    with pytest.raises(TypeError, match="float64"):
        van_hove_self(t_traj.float(), SIZES, SPECIES, masses, lags=[0], **kw)
    # an output of 2^31 elements: 256 one-atom structures x 2 groups x 1024 lags x 4096 bins, refused before anything is allocated
    many = torch.zeros(1024, 256, 3, dtype=torch.float64, device=DEV)
    with pytest.raises(ValueError, match=r"\[256, 2, 1024, 4096\]"):
        van_hove_self(many, [1] * 256, None, None, r_max=R_MAX, n_bins=4096, max_lag=1023, remove_com=False)
    with pytest.raises(ValueError, match=r"\[256, 2, 1024, 4096\]"):
        van_hove_distinct(many, t_cells[:1].repeat(256, 1, 1), [1] * 256, None, r_max=R_MAX, n_bins=4096, max_lag=1023)
    fq = dict(q_max=Q_MAX, n_bins=Q_BINS)
    with pytest.raises(ValueError, match="per-frame lattice"):
        intermediate_scattering(t_traj, t_cells[None].repeat(F, 1, 1, 1), SIZES, SPECIES, lags=[0], **fq)
    with pytest.raises(ValueError, match=r"workspace.*\[9, 3, \d+, 2\].*bytes"):
        intermediate_scattering(t_traj, t_cells, SIZES, SPECIES, lags=[0], max_workspace_bytes=10 ** 5, **fq)
    with pytest.raises(ValueError, match="lags"):
        intermediate_scattering(t_traj, t_cells, SIZES, SPECIES, lags=[2, 1], **fq)
    with pytest.raises(ValueError, match="at most 8"):
        intermediate_scattering(t_traj, t_cells, SIZES, nine, lags=[0], **fq)
    with pytest.raises(ValueError, match="beyond"):
        intermediate_scattering(t_traj, t_cells, SIZES, SPECIES, lags=[0], q_max=20.0, n_bins=Q_BINS)  # |h| > 32 in the 13 A cell
    with pytest.raises(ValueError, match="n_bins"):
        intermediate_scattering(t_traj, t_cells, SIZES, SPECIES, lags=[0], q_max=Q_MAX, n_bins=1025)
    with pytest.raises(ValueError, match="empty"):
        intermediate_scattering(t_traj, t_cells, SIZES, SPECIES, lags=[0], start=F, **fq)


# --- (e) end to end -----------------------------------------------------------------------------------------------------------------
def _fcc32(a, rng, noise):
    base = np.array([[0, 0, 0], [0, 0.5, 0.5], [0.5, 0, 0.5], [0.5, 0.5, 0]])
    cells = np.array([[i, j, k] for i in range(2) for j in range(2) for k in range(2)])
    return 2 * a * np.eye(3), (cells[:, None, :] + base[None, :, :]).reshape(-1, 3) * a + rng.normal(0.0, noise, (32, 3))


def test_run_md_then_van_hove_on_the_fcc_morse_crystal():
    """The two 32-atom fcc crystals of tests/test_gpu_trajectory.py under the pair potential, 40 steps of 2 fs from 300 K
    recorded every second step: 21 frames.  All three functions on ``res.traj_positions``, against the restatement on the run's own
    tensors copied to the host, under the bounds of (a) and (b)."""
    rng = np.random.default_rng(5)
    lats, pos = zip(*[_fcc32(s * pair_ref.R0 * np.sqrt(2.0), rng, 0.02) for s in (0.97, 0.99)])
    ns, masses = [32, 32], [np.full(32, 26.98), np.where(np.arange(32) % 4 == 0, 58.69, 26.98)]
    species = [np.full(32, 13), np.where(np.arange(32) % 4 == 0, 28, 13)]
    res = run_md(None, list(lats), list(pos), None, masses, ensemble="nve", timestep=2.0, steps=40, interval=2,
                 initial_temperature_K=300.0, seed=[3, 4], forces_fn=pair_ref.make_forces_fn(5.0, stress=False), device=DEV)
    assert res.traj_positions.shape == (21, 64, 3)
    lags, stride, n_bins, r_self = (0, 1, 5, 20), 2, 60, 1.0
    s = van_hove_self(res.traj_positions, ns, species, masses, r_max=r_self, n_bins=n_bins, lags=lags, origin_stride=stride, q=Q)
    d = van_hove_distinct(res.traj_positions, _t(np.stack(lats)), ns, species, masses, r_max=R_MAX, n_bins=n_bins, lags=lags,
                          origin_stride=stride, remove_com=True)
    host = res.traj_positions.cpu().numpy()
    want_s, worst = [], 0.0
    for b in range(2):
        rank, _ = traj_ref.groups(species[b], 32)
        S = int(rank.max())
        w, margin, _ = ref.self_part(host[:, 32 * b:32 * b + 32], rank, S, masses[b], lags, stride, True, r_self, n_bins, Q)
        assert margin > ref.EDGE_MARGIN
        want_s.append((w, traj_ref.group_counts(rank, S)))
        wc, margin, _ = ref.distinct_counts(host[:, 32 * b:32 * b + 32], lats[b], rank, S, masses[b], lags, stride, True, R_MAX, n_bins)
        assert margin > ref.EDGE_MARGIN
        wg, wv, _ = ref.distinct_normalise(wc, lats[b], 21, lags, stride, traj_ref.group_counts(rank, S), R_MAX)
        P = wc.shape[0]
        assert np.array_equal(d.counts[b, :P].cpu().numpy(), wc) and wc[0].sum() > 0, b
        assert _close(d.g[b, :P].cpu().numpy(), wg, NORM_RTOL) and _close(d.volume[b].item(), wv, NORM_RTOL), b
    dev = _check_self(s, want_s, 21, lags, stride)
    print(f"run_md: measured fs {dev:.3e}")
    assert dev <= FS_TOL
    f = intermediate_scattering(res.traj_positions, _t(np.stack(lats)), ns, species, q_max=Q_MAX, n_bins=Q_BINS, lags=lags,
                                origin_stride=stride)
    want_f = []
    for b in range(2):
        rank, _ = traj_ref.groups(species[b], 32)
        want_f.append(ref.intermediate_scattering(host[:, 32 * b:32 * b + 32], lats[b], rank, int(rank.max()), Q_MAX, Q_BINS, lags, stride))
    dev = _check_fqt(f, want_f)
    print(f"run_md: measured fqt {dev:.3e}")
    assert dev <= FQT_TOL
    # a solid: the Bragg peak (1, 1, 1) of the conventional cell - (2, 2, 2) of the doubled cell - hardly decays
    for b in range(2):
        bragg = int(np.flatnonzero((want_f[b]["hkl"] == [2, 2, 2]).all(1))[0])
        peak = f.f_vectors[b][0, :, bragg]
        assert float(peak[0]) > 20.0 and float((peak / peak[0]).min()) > 0.9
    assert not s.overflow.any()  # a solid: nobody moves by 1 A in 160 fs
    # twelve nearest neighbours stay under the first peak of G_d at every lag (3.4 A lies between the first two shells)
    k = int(np.floor(3.4 / 0.1))
    near = d.counts[:, 0, :, :k].sum(-1).double() / (torch.as_tensor(d.n_origins, device=DEV)[None, :] * 32.0)
    assert float((near - 12.0).abs().max()) < 0.5
