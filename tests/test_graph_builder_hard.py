"""Neighbour-list builders on HARD geometries against edge lists written by the reference's own builders
(oracle/make_golden_graphs_hard.py: ``nearest_neighbor_edges`` + ``build_undirected_edgedata`` and ``radius_graph``,
alignn/graphs.py:128-364, imported unmodified): lopsided cells (needle, plate, slab, 60-degree shear, a hand-strained cell,
a left-handed lattice), exact ties (sc / bcc / fcc / hcp-like, fractions exactly 0.0 and 1.0, a displaced phonon
supercell), atom counts around the kernels' loop boundaries (1, 2, 63, 64, 65, 200), more candidates per site than the
k-th-distance kernel keeps in LDS, other ``max_neighbors``, UNWRAPPED fractional coordinates (the reference scans the box
jarvis lays out around the fractional extent) and pairs closer than jarvis' ``bond_tol`` = 0.15 A (no neighbours).

Bars as in tests/test_graph_builder_golden.py / tests/test_radius_graph.py: kNN - the multiset of (u, v, image) identical,
direction pairs consecutive, bond vectors within 2e-5 of the reference's float32; radius - the same list in the same order,
vectors within 2e-6.  The HIP kernels additionally equal their torch twins element for element."""

import numpy as np
import pytest
import torch

from alignn_amd import neighbors, synthetic
from tests.helpers import load_golden, ref_keys

RADIUS_CUTOFF = 4.0
FIELDS = "seg_ptr seg_node src dst out_ptr out_slot perm inv grp_seg_ptr grp_src_ptr seg_rank".split()  # every index array of a CSRGraph


class Case:
    def __init__(self, z, i, name):
        self.name, self.lat, self.frac = name, z[f"{i}.lat"], z[f"{i}.frac"]
        self.cutoff, self.k, self.n = float(z[f"{i}.cutoff"]), int(z[f"{i}.k"]), len(self.frac)
        self.u, self.v, self.r = z[f"{i}.u"].astype(np.int64), z[f"{i}.v"].astype(np.int64), z[f"{i}.r"]
        image = z[f"{i}.image"].astype(np.int64).copy()
        image[1::2] *= -1  # the reference stores the forward image for both directions of a bond
        self.ref = sorted(zip(self.u.tolist(), self.v.tolist(), map(tuple, image.tolist())))
        self.rad = {k: z[f"{i}.rad.{k}"] for k in ("u", "v", "image", "r")} if bool(z["radius"][i]) else None

    def tensors(self):
        return torch.from_numpy(self.lat), torch.from_numpy(self.frac)


def _cases():
    z = load_golden("graphs_hard_cases.npz")
    return [Case(z, i, name) for i, name in enumerate(z["names"].tolist())]


CASES = _cases()
BY_NAME = {c.name: c for c in CASES}
RCASES = [c for c in CASES if c.rad is not None]
# ragged groups of three: neighbours in (cutoff, images x atoms^2) so that some groups pass knn_multigraph_batch's padding budget
_spacing = lambda c: 1.0 / np.linalg.norm(np.linalg.inv(c.lat), axis=0)  # noqa: E731
_ORDER = sorted(CASES, key=lambda c: (c.k, c.cutoff, c.n * c.n * float(np.prod(2 * np.ceil(c.cutoff / _spacing(c)) + 1))))
GROUPS = [_ORDER[i:i + 3] for i in range(0, len(_ORDER), 3)]


def test_the_fixture_holds_the_cases_the_kernels_need():
    names = set(BY_NAME)
    assert len(CASES) == 29 and len(RCASES) == 18
    assert {c.n for c in CASES} >= {1, 2, 63, 64, 65, 200} and {c.k for c in CASES} == {4, 12, 20}
    assert {"unwrapped_m03_p13", "unwrapped_m2_p3", "translated_rigidly", "close_pair_0p06", "close_pair_0p2"} <= names
    assert BY_NAME["unwrapped_m2_p3"].frac.min() < -1 and BY_NAME["unwrapped_m2_p3"].frac.max() > 2
    # candidate loop of one wave (64 lanes) over n * images candidates: one case exactly on a multiple of 64, one a multiple
    # plus one - from the image box the host computes
    totals = {}
    for c in CASES:
        lo, hi = synthetic.image_box(_spacing(c), c.frac.min(axis=0), c.frac.max(axis=0), c.cutoff)
        totals[c.name] = c.n * int(np.prod(hi - lo + 1))
    assert totals["atoms_64"] % 64 == 0 and totals["plate_1atom_c16"] % 64 == 1, totals
    # the dimer widens its cutoff twice (the 5-atom cluster once)
    c = BY_NAME["dimer_40A_box"]
    longest = float(np.linalg.norm(c.lat, axis=1).max())
    counts = lambda cut: np.bincount(synthetic._all_neighbors(c.lat, c.frac, cut)[0], minlength=c.n).min()  # noqa: E731
    assert counts(8.0) < 12 and counts(longest) < 12 and counts(2 * longest) >= 12


# ---------------------------------------------------------------------------------------------
# comparison with the golden
# ---------------------------------------------------------------------------------------------
def _check_knn(c, u, v, r, tol=2e-5):
    u, v, r = np.asarray(u), np.asarray(v), np.asarray(r)
    keys = ref_keys(u, v, r, c.lat, c.frac)
    assert sorted(keys) == c.ref, c.name
    assert np.array_equal(u[0::2], v[1::2]) and np.array_equal(v[0::2], u[1::2]), c.name  # consecutive direction pairs
    mine = {k: r[i] for i, k in enumerate(keys)}
    for i, k in enumerate(ref_keys(c.u, c.v, c.r, c.lat, c.frac)):
        assert np.abs(mine[k] - c.r[i]).max() < tol * max(1.0, np.abs(c.r[i]).max()), (c.name, k)


def _check_radius(c, u, v, r, img):
    g = c.rad
    u, v, r, img = np.asarray(u), np.asarray(v), np.asarray(r), np.asarray(img)
    assert len(u) == len(g["u"]), (c.name, len(u), len(g["u"]))
    assert np.array_equal(u, g["u"]) and np.array_equal(v, g["v"]) and np.array_equal(img, g["image"]), c.name
    assert np.abs(r - g["r"]).max() <= 2e-6 * max(1.0, np.abs(g["r"]).max()), c.name


def _split(cases, u, v, nn, *arrays):
    """per-crystal slices of a batched edge list (ids made local); the edges of crystal 0, 1, ... are contiguous"""
    u, v = u.cpu().numpy(), v.cpu().numpy()
    arrays = [a.cpu().numpy() for a in arrays]
    out, off = [], 0
    assert list(nn) == [c.n for c in cases]
    for c in cases:
        sel = (u >= off) & (u < off + c.n)
        assert ((v[sel] >= off) & (v[sel] < off + c.n)).all()
        idx = np.nonzero(sel)[0]
        assert len(idx) and np.array_equal(idx, np.arange(idx[0], idx[0] + len(idx))), c.name
        out.append((u[sel] - off, v[sel] - off) + tuple(a[sel] for a in arrays))
        off += c.n
    assert sum(len(o[0]) for o in out) == len(u)
    return out


# ---------------------------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", CASES, ids=lambda c: c.name)
def test_numpy_builder_on_hard_cases(c):
    _check_knn(c, *synthetic.knn_multigraph(c.lat, c.frac, c.cutoff, c.k))


@pytest.mark.parametrize("c", CASES, ids=lambda c: c.name)
def test_torch_builder_on_hard_cases(c):
    u, v, r = neighbors.knn_multigraph(*c.tensors(), cutoff=c.cutoff, max_neighbors=c.k)
    _check_knn(c, u.numpy(), v.numpy(), r.numpy())


def _run_groups(monkeypatch, budget, device="cpu"):
    """every group through knn_multigraph_batch; -> number of multi-crystal groups that took the padded branch"""
    calls = []
    single = neighbors.knn_multigraph
    monkeypatch.setattr(neighbors, "knn_multigraph", lambda *a, **k: (calls.append(1), single(*a, **k))[1])
    if budget is not None:
        monkeypatch.setattr(neighbors, "PAD_BUDGET", budget)
    padded = 0
    for grp in GROUPS:
        for cut, k in sorted({(c.cutoff, c.k) for c in grp}):  # (cutoff and k are per call: sub-group the few mixed groups)
            sub = [c for c in grp if (c.cutoff, c.k) == (cut, k)]
            del calls[:]
            u, v, r, nn = neighbors.knn_multigraph_batch([c.tensors()[0] for c in sub], [c.tensors()[1] for c in sub], cutoff=cut,
                                                         max_neighbors=k, device=device)
            padded += len(sub) > 1 and not calls
            assert budget != 0 or len(sub) == 1 or len(calls) == len(sub)
            for c, (cu, cv, cr) in zip(sub, _split(sub, u, v, nn, r)):
                _check_knn(c, cu, cv, cr)
    return padded


def test_batched_builder_on_hard_cases_padded_branch(monkeypatch):
    assert _run_groups(monkeypatch, None) >= 4  # ragged groups of two or three crystals that shared one padded image grid


def test_batched_builder_on_hard_cases_per_crystal_branch(monkeypatch):
    assert _run_groups(monkeypatch, 0) == 0


@pytest.mark.parametrize("c", RCASES, ids=lambda c: c.name)
def test_torch_radius_builder_on_hard_cases(c):
    u, v, r, img = neighbors.radius_graph(*c.tensors(), cutoff=RADIUS_CUTOFF)
    _check_radius(c, u.numpy(), v.numpy(), r.numpy(), img.numpy())


# ---------------------------------------------------------------------------------------------
# GPU: csrc/knn.hip, csrc/radius.hip, csrc/stage.hip
# ---------------------------------------------------------------------------------------------
def _by_call(cases):
    """cutoff and max_neighbors are arguments of a call: the cases that can share one, in the given order"""
    keys = []
    for c in cases:
        if (c.cutoff, c.k) not in keys:
            keys.append((c.cutoff, c.k))
    return [((cut, k), [c for c in cases if (c.cutoff, c.k) == (cut, k)]) for cut, k in keys]


def _hip_knn(cases, cut, k):
    lats, fracs = [c.tensors()[0] for c in cases], [c.tensors()[1] for c in cases]
    u, v, r, nn, img = neighbors.knn_multigraph_batch_hip(lats, fracs, cutoff=cut, max_neighbors=k, device="cuda", return_images=True)
    return u, v, r, nn, img


@pytest.mark.gpu
def test_hip_knn_kernels_on_hard_cases_against_the_reference_and_the_torch_twin():
    seen = 0
    for (cut, k), cases in _by_call(CASES):
        u, v, r, nn, img = _hip_knn(cases, cut, k)
        per = _split(cases, u, v, nn, r, img)
        e0 = 0
        for c, (cu, cv, cr, cimg) in zip(cases, per):
            _check_knn(c, cu, cv, cr)
            rec = np.array([key[2] for key in ref_keys(cu, cv, cr, c.lat, c.frac)], dtype=np.int64).reshape(-1, 3)
            fwd = cimg.astype(np.int64).copy()
            fwd[1::2] *= -1  # (the kernel stores the forward image for both directions, like the reference)
            assert np.array_equal(rec, fwd), c.name
            # the torch twin, element for element
            tu, tv, tr = neighbors.knn_multigraph(*c.tensors(), cutoff=cut, max_neighbors=k, device="cuda")
            sl = slice(e0, e0 + len(cu))
            off = sum(x.n for x in cases[:cases.index(c)])
            assert torch.equal(u[sl] - off, tu) and torch.equal(v[sl] - off, tv), c.name
            assert float((r[sl] - tr).abs().max()) <= 2e-6 * float(tr.abs().max()), c.name
            e0 += len(cu)
            seen += 1
    assert seen == len(CASES)


@pytest.mark.gpu
def test_hip_knn_kernels_batch_composition_does_not_change_a_crystal():
    """All cases of a call in one batch, in two different orders, and each case alone: a crystal's (u, v, r, image) alone is
    bit-equal to its slice of either batch - whatever shares its workgroup (four sites per workgroup) or its batch (crystals
    on different widening levels)."""
    for (cut, k), cases in _by_call(CASES):
        alone = {}
        for c in cases:
            u, v, r, _, img = _hip_knn([c], cut, k)
            alone[c.name] = (u, v, r, img)
        rng = np.random.default_rng(11)
        orders = [cases, [cases[i] for i in rng.permutation(len(cases))][::-1]] if len(cases) > 1 else [cases]
        if len(cases) > 2:
            assert [c.name for c in orders[0]] != [c.name for c in orders[1]]
        for order in orders:
            u, v, r, nn, img = _hip_knn(order, cut, k)
            e0, off = 0, 0
            for c in order:
                au, av, ar, aimg = alone[c.name]
                sl = slice(e0, e0 + au.numel())
                assert torch.equal(u[sl] - off, au) and torch.equal(v[sl] - off, av), c.name
                assert torch.equal(r[sl], ar) and torch.equal(img[sl], aimg), c.name
                e0 += au.numel()
                off += c.n
            assert e0 == u.numel()
    levels = set()
    for c in BY_NAME["dimer_40A_box"], BY_NAME["cluster_40A_box"], BY_NAME["fcc"]:
        cut, lv = 8.0, 0
        while np.bincount(synthetic._all_neighbors(c.lat, c.frac, cut)[0], minlength=c.n).min() < 12:
            longest = float(np.linalg.norm(c.lat, axis=1).max())
            cut, lv = (longest if cut < longest else 2 * cut), lv + 1
        levels.add(lv)
    assert levels == {0, 1, 2}  # the cutoff-8 batch above mixes crystals on different rungs of the ladder


@pytest.mark.gpu
def test_hip_knn_kth_search_by_rounds_beyond_the_lds_cap():
    """More candidates inside the cutoff than knn_kth_kernel's LDS list holds: the search by rounds.  The per-site candidate
    counts come from the twin's neighbour list on the CPU and are asserted to be on the intended side of the cap."""
    from alignn_amd import _lib

    cap = int(_lib.load().alignn_knn_kth_cap())
    assert cap >= 64
    for name, want_all_above in (("many_candidates_c16", True), ("many_candidates_mixed", False)):
        c = BY_NAME[name]
        src = neighbors._all_neighbors(*c.tensors(), c.cutoff)[0]
        counts = torch.bincount(src, minlength=c.n)
        if want_all_above:
            assert int(counts.min()) > cap, (name, int(counts.min()), cap)
        else:
            assert int(counts.min()) <= cap < int(counts.max()), (name, int(counts.min()), int(counts.max()), cap)
        u, v, r, nn, img = _hip_knn([c], c.cutoff, c.k)
        (cu, cv, cr, cimg), = _split([c], u, v, nn, r, img)
        _check_knn(c, cu, cv, cr)
        tu, tv, tr = neighbors.knn_multigraph(*c.tensors(), cutoff=c.cutoff, max_neighbors=c.k, device="cuda")
        assert torch.equal(u, tu) and torch.equal(v, tv)
        assert float((r - tr).abs().max()) <= 2e-6 * float(tr.abs().max())


@pytest.mark.gpu
def test_hip_knn_refuses_past_the_last_level_and_recovers():
    """More neighbours asked for than the widest of the KNN_LEVELS cutoffs holds: the level check raises (an error return of
    the builder, nothing faults), also when the crystal shares its batch, and an ordinary call afterwards is unaffected."""
    c, d = BY_NAME["bcc"], BY_NAME["left_handed"]
    before = _hip_knn([c, d], 8.0, 12)
    with pytest.raises(RuntimeError, match="fewer than 1000000 neighbours"):
        _hip_knn([c], 8.0, 10**6)
    with pytest.raises(RuntimeError, match="fewer than 1000000 neighbours"):
        _hip_knn([d, c], 8.0, 10**6)
    after = _hip_knn([c, d], 8.0, 12)
    for x, y in zip((before[0], before[1], before[2], before[4]), (after[0], after[1], after[2], after[4])):
        assert torch.equal(x, y)
    for cc, (cu, cv, cr, _) in zip((c, d), _split([c, d], after[0], after[1], after[3], after[2], after[4])):
        _check_knn(cc, cu, cv, cr)


@pytest.mark.gpu
def test_hip_radius_kernels_on_hard_cases():
    def run(cases):
        u, v, r, ns, img = neighbors.radius_graph_batch_hip([c.tensors()[0] for c in cases], [c.tensors()[1] for c in cases],
                                                            cutoff=RADIUS_CUTOFF, device="cuda", return_images=True)
        assert ns == [c.n for c in cases]
        return u.cpu().numpy(), v.cpu().numpy(), r.cpu().numpy(), img.cpu().numpy()

    u, v, r, img = run(RCASES)
    e0, off = 0, 0
    for c in RCASES:
        n_e = len(c.rad["u"])
        _check_radius(c, u[e0:e0 + n_e] - off, v[e0:e0 + n_e] - off, r[e0:e0 + n_e], img[e0:e0 + n_e])
        au, av, ar, aimg = run([c])
        _check_radius(c, au, av, ar, aimg)
        assert np.array_equal(ar, r[e0:e0 + n_e]), c.name
        tu, tv, tr, timg = neighbors.radius_graph(*c.tensors(), cutoff=RADIUS_CUTOFF)
        assert np.array_equal(au, tu.numpy()) and np.array_equal(av, tv.numpy()) and np.array_equal(aimg, timg.numpy()), c.name
        assert np.array_equal(ar, tr.numpy()), c.name  # (bit-identical to the torch twin, as its docstring promises)
        e0 += n_e
        off += c.n
    assert e0 == len(u)


@pytest.mark.gpu
@pytest.mark.parametrize("strategy", ["k-nearest", "radius_graph"])
def test_crystal_batch_on_the_device_equals_the_cpu_on_hard_cases(strategy):
    """crystal_batch: positions -> (g, L(g)) through the staging kernels (csrc/stage.hip).  One-atom cells make every bond a
    self-loop with up to a dozen images."""
    pool = RCASES if strategy == "radius_graph" else [c for c in CASES if (c.cutoff, c.k) == (8.0, 12)]
    assert sum(c.n == 1 for c in pool) >= 2
    cut = RADIUS_CUTOFF if strategy == "radius_graph" else 8.0
    for cases in (pool, [c for c in pool if c.n == 1], pool[::-1][:5]):
        lats, fracs = [c.tensors()[0] for c in cases], [c.tensors()[1] for c in cases]
        a = neighbors.crystal_batch(lats, fracs, device="cuda", cutoff=cut, neighbor_strategy=strategy)
        b = neighbors.crystal_batch(lats, fracs, device="cpu", cutoff=cut, neighbor_strategy=strategy)
        assert a.batch_size == b.batch_size and torch.equal(a.graph_ptr.cpu(), b.graph_ptr)
        a.lg.segment_rank(), b.lg.segment_rank()
        for name, ga, gb in (("g", a.g, b.g), ("lg", a.lg, b.lg)):
            assert (ga.n_nodes, ga.n_edges, ga.dense_max_src) == (gb.n_nodes, gb.n_edges, gb.dense_max_src), (strategy, name)
            for f in FIELDS:
                x, y = getattr(ga, f), getattr(gb, f)
                assert (x is None) == (y is None), (strategy, name, f)
                if x is not None:
                    assert x.dtype == y.dtype and torch.equal(x.cpu(), y), (strategy, name, f)
        assert float((a.r.cpu() - b.r).abs().max()) <= 2e-6 * float(b.r.abs().max())
