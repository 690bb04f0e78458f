"""The structural order analysis on the device (csrc/order.hip, alignn_amd/order.py) against the restatement of
tests/order_ref.py, B = 3 in one launch - a one-atom structure whose neighbours are its own images, a strongly skewed cell of two
species, more than 64 rows of three species: (a) the angle histograms bit for bit, with their marginal rows, adf to a few
roundings; (b) the neighbour counts exactly, q_l and its means under a measured bound; (c) the reciprocal vectors exactly, S(q)
under a measured bound; (d) the refusals; (e) ``run_md`` then all three.  Everywhere: a structure alone, and the batch rotated,
give the batch's bits.  The inputs and their margins (asserted here, and on the CPU in tests/test_order_ref.py) are those of
tests/order_ref.py."""

import numpy as np
import pytest
import torch

from alignn_amd import adf, run_md, steinhardt, structure_factor
from alignn_amd.order import MAX_NEIGHBORS
from tests import order_ref as ref
from tests import pair_ref
from tests.order_ref import CELLS, PTR, Q_MAX, R_CUTS, SIZES, SPECIES, SQ_BINS
from tests.sim_gpu import DEV, _t

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -53
ADF_RTOL = 8 * EPS  # adf and theta: a handful of correctly rounded operations on exact integers, as g(r)
# the largest deviations measured on an MI355X (each test's docstring says of what), and the bounds: 10 x, capped at 1e-9
Q2_MEASURED = 2.23e-16
MEAN_MEASURED = 6.04e-16
SQ_MEASURED = 8.32e-16
Q2_TOL, MEAN_RTOL, SQ_RTOL = (min(10.0 * m, 1e-9) for m in (Q2_MEASURED, MEAN_MEASURED, SQ_MEASURED))
ORDER = [2, 0, 1]


def _rows(b):
    return slice(PTR[b], PTR[b + 1])


def _close(got, want, rtol):
    return bool((np.abs(got - want) <= rtol * np.abs(want)).all())


def _case(kind):
    fixed, moving, per_frame = ref.inputs()
    return (_t(fixed), _t(CELLS)) if kind == "fixed" else (_t(moving), _t(per_frame))


def _alone(fn, t_traj, t_cells, b, cuts, **kw):
    lat = t_cells[b:b + 1] if t_cells.ndim == 3 else t_cells[:, b:b + 1]
    return fn(t_traj[:, _rows(b)], lat, [SIZES[b]], [SPECIES[b]], r_cut=cuts[b], **kw)


def _rotated(fn, t_traj, t_cells, cuts, **kw):
    traj = torch.cat([t_traj[:, _rows(b)] for b in ORDER], dim=1)
    cells = t_cells[ORDER] if t_cells.ndim == 3 else t_cells[:, ORDER]
    return fn(traj, cells, [SIZES[b] for b in ORDER], [SPECIES[b] for b in ORDER], r_cut=[cuts[b] for b in ORDER], **kw)


# --- (a) the bond-angle distribution -----------------------------------------------------------------------------------------------
ADF_CASES = [(kind, cuts, n_bins, None) for kind in ("fixed", "moving") for cuts in ("one", "each") for n_bins in ref.ADF_BINS]
ADF_CASES.append(("moving", "each", 67, (1, 2)))


@pytest.mark.parametrize("kind,cuts,n_bins,select", ADF_CASES)
def test_adf_counts_match_the_restatement_bit_for_bit(kind, cuts, n_bins, select):
    """The geometry is what the restatement's precondition allows: no angle within 1e-9 bin widths of a bin edge, no pair within
    1e-9 (relatively) of r_cut (the margins of these seeds: printed).  n_bins = 1024 with three species is six pair rows of 1024
    bins: more than the LDS histogram holds, so the rows go in two chunks."""
    t_traj, t_cells = _case(kind)
    sel = dict(start=select[0], step=select[1]) if select else {}
    frames = tuple(range(3)[slice(sel.get("start"), None, sel.get("step"))])
    want = ref.want_angles(kind, cuts, n_bins, None, frames)
    rc = R_CUTS[cuts]
    res = adf(t_traj, t_cells, SIZES, SPECIES, r_cut=rc[0] if cuts == "one" else list(rc), n_bins=n_bins, **sel)
    assert res.n_frames == len(frames) and res.counts.shape == (3, 4, 7, n_bins) and res.counts.dtype == torch.int64
    assert res.species == [[14], [3, 8], [8, 22, 38]] and res.r_cut.cpu().tolist() == list(rc)
    counts, dens = res.counts.cpu().numpy(), res.adf.cpu().numpy()
    assert (counts[:, 1:, 0] == counts[:, 1:, 1:].sum(2)).all() and (counts[:, 0] == counts[:, 1:].sum(1)).all()  # the marginal rows
    for b in range(3):
        w = want[b]
        print(f"structure {b}: {w['triplets']} triplets, angle margin {w['angle_margin']:.2e}, cutoff margin {w['cut_margin']:.2e}")
        assert w["angle_margin"] >= ref.MARGIN and w["cut_margin"] >= ref.MARGIN and w["triplets"] > 0
        G, P = w["counts"].shape[:2]
        assert np.array_equal(counts[b, :G, :P], w["counts"]), (b, np.abs(counts[b, :G, :P] - w["counts"]).sum())
        assert not counts[b, G:].any() and not counts[b, :, P:].any()  # the rows of species it has not
        assert not dens[b, G:].any() and not dens[b, :, P:].any()
        wd, wt = ref.adf_normalise(w["counts"])
        assert _close(dens[b, :G, :P], wd, ADF_RTOL), b
    assert _close(res.theta.cpu().numpy(), wt, ADF_RTOL)
    # alone, and rotated: the batch's bits
    for b in range(3):
        alone = _alone(adf, t_traj, t_cells, b, rc, n_bins=n_bins, **sel)
        G, P = alone.counts.shape[1:3]
        assert torch.equal(alone.counts[0], res.counts[b, :G, :P]) and torch.equal(alone.adf[0], res.adf[b, :G, :P]), b
    rot = _rotated(adf, t_traj, t_cells, rc, n_bins=n_bins, **sel)
    for at, b in enumerate(ORDER):
        assert torch.equal(rot.counts[at], res.counts[b]) and torch.equal(rot.adf[at], res.adf[b]), b


def test_adf_of_one_group_and_of_no_frames():
    t_traj, t_cells = _case("fixed")
    one = adf(t_traj, t_cells, SIZES, None, r_cut=3.3, n_bins=67)
    full = adf(t_traj, t_cells, SIZES, SPECIES, r_cut=3.3, n_bins=67)
    assert one.counts.shape == (3, 2, 2, 67) and torch.equal(one.counts[:, 0, 0], full.counts[:, 0, 0])
    assert torch.equal(one.counts[:, 1, 1], one.counts[:, 0, 0]) and torch.equal(one.adf[:, 0, 0], full.adf[:, 0, 0])
    on_device = adf(t_traj, t_cells, SIZES, SPECIES, r_cut=_t(np.array(R_CUTS["each"])), n_bins=67)
    assert torch.equal(on_device.counts, adf(t_traj, t_cells, SIZES, SPECIES, r_cut=list(R_CUTS["each"]), n_bins=67).counts)
    none = adf(t_traj, t_cells, SIZES, SPECIES, r_cut=3.3, n_bins=67, start=3)  # no frame selected: zeros
    assert none.n_frames == 0 and not none.counts.any() and not none.adf.any()


# --- (b) Steinhardt's parameters ----------------------------------------------------------------------------------------------------
Q_CASES = [("fixed", "one", (4, 6)), ("fixed", "each", (1, 6, 12)), ("moving", "one", (1, 6, 12)), ("moving", "each", (4, 6))]


@pytest.mark.parametrize("kind,cuts,ls", Q_CASES)
def test_steinhardt_matches_the_restatement(kind, cuts, ls):
    """``n_neighbors`` exactly.  q_l under a measured bound, on its square: q^2 = (Nb + 2 sum P_l) / Nb^2 is what is summed, its
    terms are of order one, and the square root magnifies a rounding of the sum without limit where q tends to 0 (the one-atom
    structure's neighbours are its own images, in opposite pairs: its q_1 is exactly 0).  ``Q2_MEASURED``: the largest
    |q_got^2 - q_want^2| over these four cases.  ``mean`` against the mean of the device's own q, relatively (its terms are
    >= 0): ``MEAN_MEASURED``.  Both on an MI355X; 10 x that is allowed, 1e-9 at the most.  Measured: q^2 2.22e-16, mean 6.04e-16."""
    t_traj, t_cells = _case(kind)
    rc = R_CUTS[cuts]
    want = ref.want_angles(kind, cuts, None, ls)
    res = steinhardt(t_traj, t_cells, SIZES, SPECIES, r_cut=list(rc), ls=ls)
    L = len(ls)
    assert res.q.shape == (3, PTR[-1], L) and res.n_neighbors.shape == (3, PTR[-1]) and res.n_neighbors.dtype == torch.int32
    assert res.mean.shape == (3, 4, 3, L) and res.ls == tuple(ls) and res.n_frames == 3
    q, nn, mean = res.q.cpu().numpy(), res.n_neighbors.cpu().numpy(), res.mean.cpu().numpy()
    dq, dm = 0.0, 0.0
    for b in range(3):
        w = want[b]
        assert w["cut_margin"] >= ref.MARGIN
        assert np.array_equal(nn[:, _rows(b)], w["n_neighbors"]), b
        dq = max(dq, float(np.abs(q[:, _rows(b)] ** 2 - w["q"] ** 2).max()))
        rank, _ = ref.groups(SPECIES[b], SIZES[b])
        S = int(rank.max())
        for g in range(S + 1):
            m = q[:, _rows(b)][:, ref.members(rank, g)].mean(1)  # [F, L]
            nz = m > 0
            assert not mean[b, g][~nz].any()
            dm = max(dm, float((np.abs(mean[b, g] - m)[nz] / m[nz]).max()) if nz.any() else 0.0)
        assert not mean[b, S + 1:].any()
        assert np.abs(mean[b, :S + 1] - w["mean"]).max() < 1e-7  # (and the means are those of the restatement's q)
    assert (q >= 0).all() and (q <= 1.0 + 1e-12).all() and q.max() > 0.3
    print(f"measured: q^2 {dq:.3e}, mean {dm:.3e}")
    assert dq <= Q2_TOL and dm <= MEAN_RTOL, (dq, dm)
    for b in range(3):
        alone = _alone(steinhardt, t_traj, t_cells, b, rc, ls=ls)
        S = len(set(SPECIES[b].tolist()))
        assert torch.equal(alone.q, res.q[:, _rows(b)]) and torch.equal(alone.n_neighbors, res.n_neighbors[:, _rows(b)]), b
        assert torch.equal(alone.mean[0], res.mean[b, :S + 1]), b
    rot = _rotated(steinhardt, t_traj, t_cells, rc, ls=ls)
    assert torch.equal(rot.q, torch.cat([res.q[:, _rows(b)] for b in ORDER], dim=1))
    for at, b in enumerate(ORDER):
        assert torch.equal(rot.mean[at], res.mean[b]), b


def _fcc32(a):
    base = np.array([[0, 0, 0], [0, 0.5, 0.5], [0.5, 0, 0.5], [0.5, 0.5, 0]])
    cells = np.array([[i, j, k] for i in range(2) for j in range(2) for k in range(2)])
    return 2 * a * np.eye(3), (cells[:, None, :] + base[None, :, :]).reshape(-1, 3) * a


def test_steinhardt_and_adf_of_a_perfect_fcc_crystal():
    cell, pos = _fcc32(4.0)
    res = steinhardt(_t(pos[None]), _t(cell[None]), [32], None, r_cut=3.3, ls=(4, 6))
    assert (res.n_neighbors == 12).all()
    q = res.q.cpu().numpy()
    assert np.abs(q[..., 0] - 0.19094).max() < 1e-5 and np.abs(q[..., 1] - 0.57452).max() < 1e-5
    assert np.abs(res.mean.cpu().numpy() - [0.19094, 0.57452]).max() < 1e-5 and res.mean.shape == (1, 2, 1, 2)
    counts = adf(_t(pos[None]), _t(cell[None]), [32], None, r_cut=3.3, n_bins=67).counts[0, 1, 1].cpu().numpy()
    w = 180.0 / 67
    peaks = {int(60 / w): 24, int(90 / w): 12, int(120 / w): 24, 66: 6}
    assert [int(c) for c in counts] == [32 * peaks.get(k, 0) for k in range(67)]
    for bad in ((), (4, 4), (0,), (13,), (1, 2, 3, 4, 5), (4.0,), 6):
        with pytest.raises(ValueError, match="ls"):
            steinhardt(_t(pos[None]), _t(cell[None]), [32], None, r_cut=3.3, ls=bad)


# --- (c) the static structure factor ------------------------------------------------------------------------------------------------
def _check_sq(res, wants, P_call):
    """-> the largest deviation of ``s_vectors`` and ``s``, each relative to the structure's largest |value|."""
    worst = 0.0
    s, nv = res.s.cpu().numpy(), res.n_vectors.cpu().numpy()
    for b, w in enumerate(wants):
        print(f"structure {b}: {len(w['hkl'])} vectors, margin {w['margin']:.2e}")
        assert w["margin"] >= ref.MARGIN
        assert np.array_equal(res.hkl[b].cpu().numpy(), w["hkl"]) and res.hkl[b].dtype == torch.int32, b
        assert np.array_equal(nv[b], w["n_vectors"]), b
        P = w["s_vectors"].shape[0]
        sv = res.s_vectors[b].cpu().numpy()
        assert sv.shape == (P_call, len(w["hkl"])) and not sv[P:].any() and not s[b, P:].any()
        worst = max(worst, float(np.abs(sv[:P] - w["s_vectors"]).max() / np.abs(w["s_vectors"]).max()),
                    float(np.abs(s[b, :P] - w["s"]).max() / np.abs(w["s"]).max()))
        assert (sv[0] >= 0).all() and not s[b, 0][nv[b] == 0].any()
    assert np.array_equal(res.q.cpu().numpy(), wants[0]["q"])
    return worst


def test_structure_factor_matches_the_restatement():
    """``hkl`` and ``n_vectors`` exactly (no |q| within 1e-9, relatively, of a shell edge or of q_max: printed).  ``s_vectors``
    and ``s`` under a measured bound: the device's sincospi is not numpy's cos and sin and its sums have another order.
    ``SQ_MEASURED``: the largest deviation relative to the structure's largest |value|, over the batch of three (F = 3) and the
    130 frames of the five-atom structure (two full chunks of the frame sum and a part), on an MI355X; 10 x that is allowed,
    1e-9 at the most.  Measured: the batch 5.55e-16, the 130 frames 8.31e-16."""
    t_traj, t_cells = _case("fixed")
    res = structure_factor(t_traj, t_cells, SIZES, SPECIES, q_max=Q_MAX, n_bins=SQ_BINS)
    assert res.s.shape == (3, 7, SQ_BINS) and res.n_vectors.dtype == torch.int64 and res.n_frames == 3
    d_batch = _check_sq(res, ref.want_sq("batch"), 7)
    t_long = _t(ref.long_inputs())
    long = structure_factor(t_long, t_cells[1:2], [5], [SPECIES[1]], q_max=Q_MAX, n_bins=SQ_BINS)
    assert long.n_frames == ref.LONG_FRAMES == 130
    d_long = _check_sq(long, ref.want_sq("long"), 4)
    print(f"measured: batch {d_batch:.3e}, 130 frames {d_long:.3e}")
    assert max(d_batch, d_long) <= SQ_RTOL, (d_batch, d_long)
    # a frame selection is the analysis of the selected frames; the chunks do not depend on where the frames come from
    sel = structure_factor(t_long, t_cells[1:2], [5], [SPECIES[1]], q_max=Q_MAX, n_bins=SQ_BINS, start=1, step=2)
    direct = structure_factor(t_long[1::2].contiguous(), t_cells[1:2], [5], [SPECIES[1]], q_max=Q_MAX, n_bins=SQ_BINS)
    assert sel.n_frames == 65 and torch.equal(sel.s, direct.s) and torch.equal(sel.s_vectors[0], direct.s_vectors[0])
    # alone, and rotated: the batch's bits
    for b in range(3):
        alone = structure_factor(t_traj[:, _rows(b)], t_cells[b:b + 1], [SIZES[b]], [SPECIES[b]], q_max=Q_MAX, n_bins=SQ_BINS)
        P = alone.s.shape[1]
        assert torch.equal(alone.s[0], res.s[b, :P]) and torch.equal(alone.s_vectors[0], res.s_vectors[b][:P]), b
        assert torch.equal(alone.hkl[0], res.hkl[b]) and torch.equal(alone.n_vectors[0], res.n_vectors[b]), b
    rot = structure_factor(torch.cat([t_traj[:, _rows(b)] for b in ORDER], dim=1), t_cells[ORDER], [SIZES[b] for b in ORDER],
                           [SPECIES[b] for b in ORDER], q_max=Q_MAX, n_bins=SQ_BINS)
    for at, b in enumerate(ORDER):
        assert torch.equal(rot.s[at], res.s[b]) and torch.equal(rot.s_vectors[at], res.s_vectors[b]), b
        assert torch.equal(rot.hkl[at], res.hkl[b])
    one = structure_factor(t_traj, t_cells, SIZES, None, q_max=Q_MAX, n_bins=SQ_BINS)
    assert one.s.shape == (3, 2, SQ_BINS) and torch.equal(one.s[:, 1], one.s[:, 0])
    none = structure_factor(t_traj, t_cells, SIZES, SPECIES, q_max=Q_MAX, n_bins=SQ_BINS, start=3)
    assert none.n_frames == 0 and not none.s.any() and torch.equal(none.hkl[2], res.hkl[2])


# --- (d) refusals -------------------------------------------------------------------------------------------------------------------
def test_refusals():
    """The restatement finds at most 38 neighbours within 6 A in the 70-atom structure and 72 in the five-atom one (an atom's own
    images count): it is the batch at r_cut = 6.0 that is refused, the 70-atom structure alone is analysed; at 8.5 A it is
    refused too."""
    fixed, _, _ = ref.inputs()
    t_traj, t_cells = _case("fixed")
    small = CELLS.copy()
    small[0] *= 0.2  # heights of ~0.63 A: r_cut = 6 needs ten images
    assert max(ref.image_range(small[0], 6.0)) > 8
    for fn, kw in ((adf, dict(n_bins=67)), (steinhardt, dict())):
        with pytest.raises(ValueError, match="images"):
            fn(t_traj, _t(small), SIZES, SPECIES, r_cut=6.0, **kw)
    most = [max(len(r) for f in range(3) for _, _, r in ref.shells(CELLS[b], fixed[f, _rows(b)], 6.0)[0]) for b in range(3)]
    print(f"neighbours within 6.0 A at the most, per structure: {most}")
    assert max(most) > MAX_NEIGHBORS >= most[2]
    for fn, kw in ((adf, dict(n_bins=67)), (steinhardt, dict())):
        with pytest.raises(ValueError, match="neighbours.*r_cut"):
            fn(t_traj, t_cells, SIZES, SPECIES, r_cut=6.0, **kw)
    big = steinhardt(t_traj[:, _rows(2)], t_cells[2:3], [70], [SPECIES[2]], r_cut=6.0)
    assert int(big.n_neighbors.max()) == most[2]
    assert max(len(r) for _, _, r in ref.shells(CELLS[2], fixed[0, _rows(2)], 8.5)[0]) > MAX_NEIGHBORS
    with pytest.raises(ValueError, match="neighbours.*r_cut"):
        adf(t_traj[:, _rows(2)], t_cells[2:3], [70], [SPECIES[2]], r_cut=8.5, n_bins=67)
    assert max(ref.hkl_range(CELLS[2], 15.0)) > ref.MAX_HKL
    with pytest.raises(ValueError, match="q_max"):
        structure_factor(t_traj, t_cells, SIZES, SPECIES, q_max=15.0)
    with pytest.raises(ValueError, match="per-frame"):
        structure_factor(t_traj, _t(ref.inputs()[2]), SIZES, SPECIES, q_max=Q_MAX)
    nine = [SPECIES[0], SPECIES[1], np.arange(70) % 9]
    for call in (lambda: adf(t_traj, t_cells, SIZES, nine, r_cut=3.3), lambda: steinhardt(t_traj, t_cells, SIZES, nine, r_cut=3.3),
                 lambda: structure_factor(t_traj, t_cells, SIZES, nine, q_max=Q_MAX)):
        with pytest.raises(ValueError, match="at most 8"):
            call()
    for bad in (dict(r_cut=0.0), dict(r_cut=[3.3, 3.3]), dict(r_cut="3"), dict(r_cut=3.3, n_bins=0), dict(r_cut=3.3, n_bins=1025),
                dict(r_cut=3.3, step=0), dict(r_cut=torch.ones(3, device=DEV))):
        with pytest.raises(ValueError):
            adf(t_traj, t_cells, SIZES, SPECIES, **bad)
    with pytest.raises(TypeError):
        adf(t_traj.float(), t_cells, SIZES, SPECIES, r_cut=3.3)
    with pytest.raises(TypeError):
        structure_factor(t_traj, t_cells.cpu(), SIZES, SPECIES, q_max=Q_MAX)
    with pytest.raises(ValueError, match="q_max"):
        structure_factor(t_traj, t_cells, SIZES, SPECIES, q_max=-1.0)


# --- (e) end to end -----------------------------------------------------------------------------------------------------------------
def test_run_md_then_the_three_analyses_on_the_fcc_morse_crystal():
    """Two 32-atom fcc crystals (a = 0.97 and 0.99 x 2.9 x sqrt 2 A, the second with two species by name only) under the pair
    potential, 40 steps of 2 fs from 300 K recorded every second step: 21 frames; the restatement on the trajectory copied back,
    under the rules of (a) - (c)."""
    rng = np.random.default_rng(5)
    lats, pos = [], []
    for s in (0.97, 0.99):
        cell, p = _fcc32(s * pair_ref.R0 * np.sqrt(2.0))
        lats.append(cell)
        pos.append(p + rng.normal(0.0, 0.02, (32, 3)))
    ns, masses = [32, 32], [np.full(32, 26.98), np.where(np.arange(32) % 4 == 0, 58.69, 26.98)]
    species = [np.full(32, 13), np.where(np.arange(32) % 4 == 0, 28, 13)]
    res = run_md(None, lats, pos, None, masses, ensemble="nve", timestep=2.0, steps=40, interval=2, initial_temperature_K=300.0,
                 seed=[3, 4], forces_fn=pair_ref.make_forces_fn(5.0, stress=False), device=DEV)
    traj, cells = res.traj_positions, _t(np.stack(lats))
    assert traj.shape == (21, 64, 3)
    r_cut, n_bins, ls, q_max = 3.4, 90, (4, 6), 5.0  # (3.4 A lies between the first two shells, 2.8 and 4.0 A)
    a = adf(traj, cells, ns, species, r_cut=r_cut, n_bins=n_bins)
    st = steinhardt(traj, cells, ns, species, r_cut=r_cut, ls=ls)
    sq = structure_factor(traj, cells, ns, species, q_max=q_max, n_bins=40)
    host = traj.cpu().numpy()
    dq = dsq = 0.0
    for b in range(2):
        rows = slice(32 * b, 32 * b + 32)
        rank, _ = ref.groups(species[b], 32)
        S = int(rank.max())
        w = ref.angles(host[:, rows], lats[b], rank, S, r_cut, n_bins, ls)
        print(f"structure {b}: angle margin {w['angle_margin']:.2e}, cutoff margin {w['cut_margin']:.2e}")
        assert w["angle_margin"] >= ref.MARGIN and w["cut_margin"] >= ref.MARGIN
        G, P = w["counts"].shape[:2]
        assert np.array_equal(a.counts[b, :G, :P].cpu().numpy(), w["counts"]) and not a.counts[b, G:].any(), b
        assert _close(a.adf[b, :G, :P].cpu().numpy(), ref.adf_normalise(w["counts"])[0], ADF_RTOL), b
        assert np.array_equal(st.n_neighbors[:, rows].cpu().numpy(), w["n_neighbors"]), b
        dq = max(dq, float(np.abs(st.q[:, rows].cpu().numpy() ** 2 - w["q"] ** 2).max()))
        assert np.abs(st.mean[b, :S + 1].cpu().numpy() - w["mean"]).max() < 1e-7
        ws = ref.structure_factor(host[:, rows], lats[b], rank, S, q_max, 40)
        assert ws["margin"] >= ref.MARGIN and np.array_equal(sq.hkl[b].cpu().numpy(), ws["hkl"])
        assert np.array_equal(sq.n_vectors[b].cpu().numpy(), ws["n_vectors"])
        P = ws["s_vectors"].shape[0]
        dsq = max(dsq, float(np.abs(sq.s_vectors[b][:P].cpu().numpy() - ws["s_vectors"]).max() / np.abs(ws["s_vectors"]).max()),
                  float(np.abs(sq.s[b, :P].cpu().numpy() - ws["s"]).max() / np.abs(ws["s"]).max()))
    print(f"measured: q^2 {dq:.3e}, S(q) {dsq:.3e}")
    assert dq <= Q2_TOL and dsq <= SQ_RTOL, (dq, dsq)
    # a solid at 300 K: twelve neighbours, q6 near the fcc value, the (111) reflection of the conventional cell far above 1
    assert (st.n_neighbors == 12).all() and float((st.mean[:, 0, :, 1] - 0.57452).abs().max()) < 0.05
    hkl = sq.hkl[0].cpu().numpy()
    at = int(np.nonzero((hkl == [2, 2, 2]).all(1))[0][0])
    assert float(sq.s_vectors[0][0, at]) > 16.0
