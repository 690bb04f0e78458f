"""The local structure analysis on the device (csrc/local_order.hip, alignn_amd/local_order.py) against the restatement of
tests/local_ref.py, B = 8 in one launch - the three random structures of tests/order_ref.py (one atom whose neighbours are its own
images, a skewed cell of two species, 70 rows of three species), the fcc, hcp and bcc crystals in their smallest cells, a 13-atom
icosahedron and a noisy 32-atom fcc supercell, 3 frames: (a) every integer of ``cna`` exactly; (b) ``bond_order``: the neighbour
counts exactly, the sums s and t under a measured bound, q, w and the means against the device's own sums; (c) q_l of
``bond_order`` (harmonics) against q_l of ``steinhardt`` (addition theorem); (d) the edges and refusals; (e) ``run_md`` then both.
Everywhere: a structure alone, and the batch rotated, give the batch's bits.  The inputs and their margins (asserted on the CPU
in tests/test_local_ref.py) are those of tests/local_ref.py."""

import numpy as np
import pytest
import torch

from alignn_amd import BondOrderResult, CNAResult, bond_order, cna, run_md, steinhardt
from alignn_amd.local_order import MAX_NEIGHBORS
from tests import local_ref as ref
from tests import pair_ref
from tests.local_ref import PTR, R_CUTS, SIZES, SPECIES
from tests.sim_gpu import DEV, _t

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -53
# the largest deviations measured on an MI355X (each test's docstring says of what), and the bounds: 10 x, capped at 1e-9
ST_MEASURED = 1.11e-15
MEAN_MEASURED = 4.91e-16
Q2_AGREE_MEASURED = 3.56e-15
ST_TOL, MEAN_RTOL, Q2_AGREE_TOL = (min(10.0 * m, 1e-9) for m in (ST_MEASURED, MEAN_MEASURED, Q2_AGREE_MEASURED))
FORMULA_RTOL = 4 * EPS  # q and w from the device's own s and t: a square root, a product and a quotient, each correctly rounded
ORDER = [2, 0, 1, 5, 6, 7, 3, 4]
B = len(SIZES)
CNA_FIELDS = ("structure", "signature_counts", "n_neighbors")
BOND_FIELDS = ("s", "t", "q", "w", "s_avg", "t_avg", "q_avg", "w_avg", "n_neighbors")


def _rows(b):
    return slice(PTR[b], PTR[b + 1])


def _case(kind):
    fixed, moving, cells, per_frame = ref.inputs()
    return (_t(fixed), _t(cells)) if kind == "fixed" else (_t(moving), _t(per_frame))


def _alone(fn, t_traj, t_cells, b, cuts, **kw):
    lat = t_cells[b:b + 1] if t_cells.ndim == 3 else t_cells[:, b:b + 1]
    return fn(t_traj[:, _rows(b)], lat, [SIZES[b]], [SPECIES[b]], r_cut=cuts[b], **kw)


def _rotated(fn, t_traj, t_cells, cuts, **kw):
    traj = torch.cat([t_traj[:, _rows(b)] for b in ORDER], dim=1)
    cells = t_cells[ORDER] if t_cells.ndim == 3 else t_cells[:, ORDER]
    return fn(traj, cells, [SIZES[b] for b in ORDER], [SPECIES[b] for b in ORDER], r_cut=[cuts[b] for b in ORDER], **kw)


def _same_bits_alone_and_rotated(fn, res, fields, per_group, t_traj, t_cells, rc, **kw):
    """Every per-atom output ``fields`` and every per-group output ``per_group`` ([B, S + 1, ...]) of ``res``: the same bits from
    each structure alone and from the batch in another order."""
    for b in range(B):
        alone = _alone(fn, t_traj, t_cells, b, rc, **kw)
        for name in fields:
            assert torch.equal(getattr(alone, name), getattr(res, name)[:, _rows(b)]), (name, b)
        for name in per_group:
            G = getattr(alone, name).shape[1]
            assert torch.equal(getattr(alone, name)[0], getattr(res, name)[b, :G]) and not getattr(res, name)[b, G:].any(), (name, b)
    rot = _rotated(fn, t_traj, t_cells, rc, **kw)
    for name in fields:
        assert torch.equal(getattr(rot, name), torch.cat([getattr(res, name)[:, _rows(b)] for b in ORDER], dim=1)), name
    for name in per_group:
        for at, b in enumerate(ORDER):
            assert torch.equal(getattr(rot, name)[at], getattr(res, name)[b]), (name, b)


# --- (a) common-neighbour analysis --------------------------------------------------------------------------------------------------
CNA_CASES = [("fixed", "one", False, None), ("fixed", "each", False, None), ("moving", "each", False, None),
             ("fixed", "wide", True, None), ("moving", "wide", True, None), ("moving", "one", False, (1, 2))]


@pytest.mark.parametrize("kind,cuts,adaptive,select", CNA_CASES)
def test_cna_matches_the_restatement_integer_for_integer(kind, cuts, adaptive, select):
    """``structure``, ``signature_counts``, ``n_neighbors`` and ``counts`` are equal to the restatement's: the geometry is what its
    preconditions allow (tests/test_local_ref.py asserts the margins of these cases).  The crystals give their classes, with the
    fixed cutoff in the unscaled frames and with the adaptive rule at every scale."""
    t_traj, t_cells = _case(kind)
    sel = dict(start=select[0], step=select[1]) if select else {}
    frames = tuple(range(3)[slice(sel.get("start"), None, sel.get("step"))])
    want = ref.want_cna(kind, cuts, adaptive, frames)
    rc = R_CUTS[cuts]
    res = cna(t_traj, t_cells, SIZES, SPECIES, r_cut=rc[0] if cuts in ("one", "wide") else list(rc), adaptive=adaptive, **sel)
    F = len(frames)
    assert isinstance(res, CNAResult) and res.n_frames == F and res.adaptive is adaptive and res.r_cut.cpu().tolist() == list(rc)
    assert res.structure.shape == (F, PTR[-1]) and res.structure.dtype == torch.int32
    assert res.signature_counts.shape == (F, PTR[-1], 5) and res.signature_counts.dtype == torch.int32
    assert res.n_neighbors.shape == (F, PTR[-1]) and res.n_neighbors.dtype == torch.int32
    assert res.counts.shape == (B, 4, F, 5) and res.counts.dtype == torch.int64 and res.fraction.dtype == torch.float64
    assert res.species[:3] == [[14], [3, 8], [8, 22, 38]] and res.species[6] == [13, 29]
    got = {k: getattr(res, k).cpu().numpy() for k in CNA_FIELDS + ("counts", "fraction")}
    for b in range(B):
        w = want[b]
        for name in CNA_FIELDS:
            assert np.array_equal(got[name][:, _rows(b)], w[name]), (name, b, ref.NAMES[b])
        G = w["counts"].shape[0]
        assert np.array_equal(got["counts"][b, :G], w["counts"]) and not got["counts"][b, G:].any(), b
        members = np.array([SIZES[b]] + [int((SPECIES[b] == z).sum()) for z in res.species[b]], dtype=np.float64)
        assert np.array_equal(got["fraction"][b, :G], w["counts"] / members[:, None, None]) and not got["fraction"][b, G:].any(), b
        assert (got["counts"][b, 0].sum(-1) == SIZES[b]).all() and np.array_equal(got["counts"][b, 1:G].sum(0), got["counts"][b, 0])
    if kind == "fixed" or adaptive:
        for b, cls in ((3, ref.FCC), (4, ref.HCP), (5, ref.BCC)):
            assert (got["structure"][:, _rows(b)] == cls).all(), ref.NAMES[b]
        ico = got["structure"][:, _rows(6)]
        assert (ico[:, 0] == ref.ICO).all() and not ico[:, 1:].any()
        assert (got["signature_counts"][:, PTR[5]] == [0, 0, 6, 0, 8]).all() and (got["signature_counts"][:, PTR[6]] == [0, 0, 0, 12, 0]).all()
    noisy = got["structure"][:, _rows(7)]
    print(f"the noisy supercell: {int((noisy == ref.FCC).sum())} FCC, {int((noisy == ref.OTHER).sum())} OTHER of {noisy.size}")
    _same_bits_alone_and_rotated(cna, res, CNA_FIELDS, ("counts", "fraction"), t_traj, t_cells, rc, adaptive=adaptive, **sel)


# --- (b) bond-orientational order ---------------------------------------------------------------------------------------------------
BOND_CASES = [("fixed", "one", (4, 6)), ("moving", "each", (4, 6, 12)), ("moving", "wide", (4, 6))]


def _mean_deviation(mean_b, x, rank, S):
    """The largest |mean - numpy's mean| relative to the mean of |x| (the scale of the sum's terms: w_l has both signs), over the
    groups, frames and degrees where that is not zero; the others must be zeros."""
    worst = 0.0
    for g in range(S + 1):
        rows = ref.members(rank, g)
        m, scale = x[:, rows].mean(1), np.abs(x[:, rows]).mean(1)
        nz = scale > 0
        assert not mean_b[g][~nz].any()
        if nz.any():
            worst = max(worst, float((np.abs(mean_b[g] - m)[nz] / scale[nz]).max()))
    return worst


@pytest.mark.parametrize("kind,cuts,ls", BOND_CASES)
def test_bond_order_matches_the_restatement(kind, cuts, ls):
    """``n_neighbors`` exactly.  ``s``, ``t``, ``s_avg``, ``t_avg`` absolutely: they are sums of terms of order one, where the
    quotient w and the root q magnify a rounding without limit as s tends to 0 (s_4 of the icosahedron's centre is zero up to
    roundings).  ``ST_MEASURED``: the largest deviation from the float64 restatement over these three cases.  q, w, q_avg, w_avg
    against their defining formulas on the device's own s and t, to a few roundings.  ``mean`` against numpy's mean of the
    device's own arrays, relative to the mean of the absolute values: ``MEAN_MEASURED``.  Both on an MI355X; 10 x that is
    allowed, 1e-9 at the most.  Measured, case by case: s and t 3.33e-16, 1.11e-15, 2.78e-16; the means 4.91e-16 in each."""
    t_traj, t_cells = _case(kind)
    rc = R_CUTS[cuts]
    want = ref.want_bond(kind, cuts, ls)
    res = bond_order(t_traj, t_cells, SIZES, SPECIES, r_cut=list(rc), ls=ls)
    L = len(ls)
    assert isinstance(res, BondOrderResult) and res.ls == tuple(ls) and res.n_frames == 3
    for name in BOND_FIELDS[:-1]:
        assert getattr(res, name).shape == (3, PTR[-1], L) and getattr(res, name).dtype == torch.float64, name
    assert res.n_neighbors.shape == (3, PTR[-1]) and res.n_neighbors.dtype == torch.int32 and res.mean.shape == (B, 4, 3, 4, L)
    got = {k: getattr(res, k).cpu().numpy() for k in BOND_FIELDS + ("mean",)}
    d_st = d_mean = 0.0
    for b in range(B):
        w = want[b]
        assert np.array_equal(got["n_neighbors"][:, _rows(b)], w["n_neighbors"]), b
        for name in ("s", "t", "s_avg", "t_avg"):
            d_st = max(d_st, float(np.abs(got[name][:, _rows(b)] - w[name]).max()))
        rank, _ = ref.groups(SPECIES[b], SIZES[b])
        S = int(rank.max())
        for k, name in enumerate(("q", "q_avg", "w", "w_avg")):
            d_mean = max(d_mean, _mean_deviation(got["mean"][b, :, :, k], got[name][:, _rows(b)], rank, S))
            if name.startswith("q"):  # (and the means are those of the restatement's q; its w is magnified where s tends to 0)
                assert np.abs(got["mean"][b, :S + 1, :, k] - ref.group_means(w[name], rank, S)).max() < 1e-7, (name, b)
        assert not got["mean"][b, S + 1:].any()
    for key in ("", "_avg"):
        for u, l in enumerate(ls):
            q, w = ref.q_w(l, got["s" + key][..., u], got["t" + key][..., u])
            assert (np.abs(got["q" + key][..., u] - q) <= FORMULA_RTOL * np.abs(q)).all(), (key, l)
            assert (np.abs(got["w" + key][..., u] - w) <= FORMULA_RTOL * np.abs(w)).all(), (key, l)
    # the crystals: q4 and q6 of the fixed frames are the constants, and the averaged forms are the plain ones
    if kind == "fixed" and tuple(ls) == (4, 6):
        for b, name in ((3, "fcc"), (4, "hcp"), (5, "bcc")):
            q4, q6, w4, w6 = ref.CONSTANTS[name]
            for field in ("q", "q_avg"):
                assert np.abs(got[field][:, _rows(b)] - [q4, q6]).max() < 5e-6, (name, field)
            for field in ("w", "w_avg"):
                assert np.abs(got[field][:, _rows(b)] - [w4, w6]).max() < 5e-6, (name, field)
        assert abs(got["q"][0, PTR[6], 1] - 0.663325) < 5e-6 and abs(got["w"][0, PTR[6], 1] + 0.169754) < 5e-6
    print(f"measured: s, t {d_st:.3e}, mean {d_mean:.3e}")
    assert d_st <= ST_TOL and d_mean <= MEAN_RTOL, (d_st, d_mean)
    _same_bits_alone_and_rotated(bond_order, res, BOND_FIELDS, ("mean",), t_traj, t_cells, rc, ls=ls)


# --- (c) two independent kernels -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,cuts", [("fixed", "one"), ("moving", "each"), ("moving", "wide")])
def test_harmonics_and_addition_theorem_agree(kind, cuts):
    """q_l^2 of ``bond_order`` (the harmonics, summed over m) and of ``steinhardt`` (the Legendre polynomials of every pair of
    neighbours) on the same trajectory and cutoffs, l = 4, 6, 12; the neighbour counts are identical.  ``Q2_AGREE_MEASURED``: the
    largest |difference| of q^2 over these three cases on an MI355X; 10 x that is allowed, 1e-9 at the most.  Measured, case by
    case: 2.67e-15, 3.55e-15, 1.39e-15."""
    t_traj, t_cells = _case(kind)
    rc = list(R_CUTS[cuts])
    mine = bond_order(t_traj, t_cells, SIZES, SPECIES, r_cut=rc, ls=(4, 6, 12), average=False)
    theirs = steinhardt(t_traj, t_cells, SIZES, SPECIES, r_cut=rc, ls=(4, 6, 12))
    assert torch.equal(mine.n_neighbors, theirs.n_neighbors)
    d = float((mine.q ** 2 - theirs.q ** 2).abs().max())
    print(f"measured: q^2 {d:.3e}")
    assert d <= Q2_AGREE_TOL, d


# --- (d) edges and refusals ------------------------------------------------------------------------------------------------------------
def test_edges():
    t_traj, t_cells = _case("fixed")
    rc = list(R_CUTS["each"])
    full, one = cna(t_traj, t_cells, SIZES, SPECIES, r_cut=rc), cna(t_traj, t_cells, SIZES, None, r_cut=rc)  # species=None: one group
    assert one.counts.shape == (B, 2, 3, 5) and torch.equal(one.counts[:, 0], full.counts[:, 0]) and torch.equal(one.counts[:, 1], one.counts[:, 0])
    assert torch.equal(one.structure, full.structure) and one.species == [[0]] * B
    bo_full = bond_order(t_traj, t_cells, SIZES, SPECIES, r_cut=rc)
    bo_one = bond_order(t_traj, t_cells, SIZES, None, r_cut=rc)
    assert bo_one.mean.shape == (B, 2, 3, 4, 2) and torch.equal(bo_one.mean[:, 0], bo_full.mean[:, 0]) and torch.equal(bo_one.q, bo_full.q)
    on_device = _t(np.array(rc))  # r_cut as a device tensor
    assert torch.equal(cna(t_traj, t_cells, SIZES, SPECIES, r_cut=on_device).structure, full.structure)
    assert torch.equal(bond_order(t_traj, t_cells, SIZES, SPECIES, r_cut=on_device).t_avg, bo_full.t_avg)
    none = cna(t_traj, t_cells, SIZES, SPECIES, r_cut=rc, start=3)  # no frame selected: zeros
    assert none.n_frames == 0 and none.structure.shape == (0, PTR[-1]) and none.counts.shape == (B, 4, 0, 5)
    none = bond_order(t_traj, t_cells, SIZES, SPECIES, r_cut=rc, start=3)
    assert none.n_frames == 0 and none.q.shape == (0, PTR[-1], 2) and none.mean.shape == (B, 4, 0, 4, 2) and not none.mean.any()
    plain = bond_order(t_traj, t_cells, SIZES, SPECIES, r_cut=rc, average=False)  # average=False: None for the averaged outputs
    assert plain.q_avg is None and plain.w_avg is None and plain.s_avg is None and plain.t_avg is None
    assert torch.equal(plain.q, bo_full.q) and torch.equal(plain.w, bo_full.w) and torch.equal(plain.t, bo_full.t)
    assert torch.equal(plain.mean[:, :, :, 0], bo_full.mean[:, :, :, 0]) and not plain.mean[:, :, :, 1].any() and not plain.mean[:, :, :, 3].any()


def test_refusals():
    """The restatement finds more than 64 neighbours within 8.5 A in the 70-atom structure: both functions refuse it as
    ``alignn_amd.order`` does, by the status word; so they do a cutoff that needs more than eight images."""
    fixed, _, cells, _ = ref.inputs()
    t_traj, t_cells = _case("fixed")
    assert max(len(r) for _, _, r in ref.shells(cells[2], fixed[0, _rows(2)], 8.5)[0]) > MAX_NEIGHBORS
    for fn, kw in ((cna, dict()), (cna, dict(adaptive=True)), (bond_order, dict()), (bond_order, dict(average=False))):
        with pytest.raises(ValueError, match="neighbours.*r_cut"):
            fn(t_traj[:, _rows(2)], t_cells[2:3], [70], [SPECIES[2]], r_cut=8.5, **kw)
        small = cells[:1] * 0.2  # heights of ~0.63 A: r_cut = 6 needs ten images
        with pytest.raises(ValueError, match="images"):
            fn(t_traj[:, _rows(0)], _t(small), [1], [SPECIES[0]], r_cut=6.0, **kw)
        for bad in (dict(r_cut=0.0), dict(r_cut=[3.3, 3.3]), dict(r_cut=3.3, step=0), dict(r_cut=torch.ones(3, device=DEV))):
            with pytest.raises(ValueError):
                fn(t_traj, t_cells, SIZES, SPECIES, **{**kw, **bad})
        with pytest.raises(TypeError):
            fn(t_traj.float(), t_cells, SIZES, SPECIES, r_cut=3.3, **kw)


# --- (e) end to end -----------------------------------------------------------------------------------------------------------------
def test_run_md_then_cna_and_bond_order_on_the_fcc_morse_crystal():
    """Two 32-atom fcc crystals (a = 0.97 and 0.99 x 2.9 x sqrt 2 A, the second with two species by name only) under the pair
    potential, 40 steps of 2 fs from 300 K recorded every second step: 21 frames, analysed where ``run_md`` left them."""
    rng = np.random.default_rng(5)
    lats, pos = [], []
    for s in (0.97, 0.99):
        cell, p = ref.fcc_supercell(s * pair_ref.R0 * np.sqrt(2.0))
        lats.append(cell)
        pos.append(p + rng.normal(0.0, 0.02, (32, 3)))
    ns, masses = [32, 32], [np.full(32, 26.98), np.where(np.arange(32) % 4 == 0, 58.69, 26.98)]
    species = [np.full(32, 13), np.where(np.arange(32) % 4 == 0, 28, 13)]
    res = run_md(None, lats, pos, None, masses, ensemble="nve", timestep=2.0, steps=40, interval=2, initial_temperature_K=300.0,
                 seed=[3, 4], forces_fn=pair_ref.make_forces_fn(5.0, stress=False), device=DEV)
    traj, cells = res.traj_positions, _t(np.stack(lats))
    assert traj.shape == (21, 64, 3)
    for adaptive, r_cut in ((False, 3.4), (True, 4.6)):  # (3.4 A lies between the first two shells, 2.8 and 4.0 A)
        c = cna(traj, cells, ns, species, r_cut=r_cut, adaptive=adaptive)
        assert c.structure.shape == (21, 64) and c.structure.dtype == torch.int32 and c.signature_counts.shape == (21, 64, 5)
        assert c.counts.shape == (2, 3, 21, 5) and c.counts.dtype == torch.int64 and c.fraction.dtype == torch.float64
        assert torch.equal(c.fraction[:, 0].sum(-1), torch.ones(2, 21, dtype=torch.float64, device=traj.device))
        assert (c.counts[:, 0].sum(-1) == 32).all() and not c.counts[0, 2].any()  # (the first crystal has one species)
        assert c.counts[:, 0].sum(1).argmax(-1).tolist() == [ref.FCC, ref.FCC]  # the majority class of either crystal
    bo = bond_order(traj, cells, ns, species, r_cut=3.4, ls=(4, 6))
    assert bo.q.shape == bo.w_avg.shape == (21, 64, 2) and bo.q.dtype == torch.float64 and bo.mean.shape == (2, 3, 21, 4, 2)
    assert (bo.n_neighbors == 12).all() and float((bo.mean[:, 0, :, 0, 1] - 0.574524).abs().max()) < 0.05
    assert float((bo.mean[:, 0, :, 1, 1] - 0.574524).abs().max()) < 0.05  # (the averaged q6 stays at the fcc value too)
    host = traj.cpu().numpy()
    rank, _ = ref.groups(species[1], 32)
    w = ref.cna(host[::10, 32:], lats[1], rank, 2, 3.4)
    assert min(w["cut_margin"], w["bond_margin"]) >= ref.MARGIN
    got = cna(traj, cells, ns, species, r_cut=3.4, step=10)
    assert np.array_equal(got.structure[:, 32:].cpu().numpy(), w["structure"]) and np.array_equal(got.counts[1].cpu().numpy(), w["counts"])
