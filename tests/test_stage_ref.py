"""tests/stage_ref.py on the CPU: the definition-only reference the GPU pin of csrc/stage.hip (tests/test_gpu_stage_ref.py) compares
with must agree with itself (E x E comparison against the sort-based construction), with the numpy restatement of the kernel
arithmetic (tests/stage_arith_ref.stage_numpy), with the torch builders (graph.build_csr + line_graph_of) and with what
loader.pack derives on the host - and every case must still hold the feature it exists for."""

import time

import numpy as np
import pytest
import torch

from alignn_amd import loader
from alignn_amd.graph import build_csr, line_graph_of
from tests import stage_ref as S
from tests.stage_arith_ref import stage_numpy


def test_the_case_list_is_what_it_says():
    assert tuple(S.cases()) == S.ALL and S.LARGE not in S.SMALL
    for name, (u, v, N) in S.cases().items():
        assert u.dtype == v.dtype == np.int64 and u.shape == v.shape and u.ndim == 1 and u.size > 0, name
        assert 0 <= min(u.min(), v.min()) and max(u.max(), v.max()) < N, name
    again = {k: (u.copy(), v.copy(), N) for k, (u, v, N) in S.cases().items()}
    S.cases.cache_clear()
    for k, (u, v, N) in S.cases().items():  # deterministic
        assert np.array_equal(u, again[k][0]) and np.array_equal(v, again[k][1]) and N == again[k][2], k


@pytest.mark.parametrize("name", S.SMALL)
def test_brute_force_equals_the_sort_based_construction(name):
    u, v, N = S.cases()[name]
    a, b = S.brute(u, v, N), S.by_sorting(u, v, N)
    assert set(a) == set(b) and set(S.INDEX_FIELDS) <= set(a)
    for k in a:
        assert np.array_equal(a[k], b[k]), (name, k)
    E, T = u.shape[0], a["T"]
    for k in S.INDEX_FIELDS:
        assert a[k].shape == (S.length(k, N, E, T),) and a[k].dtype == np.int64, (name, k)
        info = np.iinfo(S.DTYPE[k])
        assert a[k].size == 0 or (info.min <= a[k].min() and a[k].max() <= info.max), (name, k)


@pytest.mark.parametrize("name", S.SMALL)
def test_reference_equals_the_restated_arithmetic_and_the_torch_builders(name):
    u, v, N = S.cases()[name]
    ref = S.reference(name)
    E, T = u.shape[0], ref["T"]
    got = stage_numpy(u, v, N)
    g = build_csr(torch.tensor(u), torch.tensor(v), N)
    lg = line_graph_of(g)
    torch_fields = dict(perm=g.perm, inv=g.inv, src=g.src, dst=g.dst, seg_ptr=g.seg_ptr, out_slot=g.out_slot, out_ptr=g.out_ptr,
                        lg_seg_ptr=lg.seg_ptr, lg_out_ptr=lg.out_ptr, lg_src=lg.src, lg_dst=lg.dst, lg_seg_rank=lg.seg_rank,
                        lg_out_slot=lg.out_slot, lg_ident=lg.perm)
    numpy_fields = {("lg_seg_rank" if k == "seg_rank" else k): x for k, x in got.items() if k != "T"}
    assert set(numpy_fields) <= set(S.INDEX_FIELDS) and set(torch_fields) | {"out_rank"} == set(S.INDEX_FIELDS)
    for k, x in numpy_fields.items():
        assert np.array_equal(np.asarray(x, dtype=np.int64).reshape(-1), ref[k]), (name, "stage_numpy", k)
    for k, x in torch_fields.items():
        assert str(x.dtype) == "torch." + S.DTYPE[k], (name, k)
        assert np.array_equal(x.numpy().astype(np.int64), ref[k]), (name, "torch builders", k)
    assert torch.equal(lg.seg_node, g.out_slot) and lg.inv is lg.perm
    assert got["T"] == lg.n_edges == T and lg.n_nodes == E and g.n_nodes == N and g.n_edges == E
    assert lg.dense_max_src == ref["max_in"]
    p = loader.pack(u, v, [N], np.zeros((E, 3), np.float32), np.eye(3, dtype=np.float32)[None], atom_features=np.zeros((N, 1), np.float32),
                    pin=False)
    assert (p.num_triplets, p.max_in_degree, p.num_nodes, p.num_edges) == (T, ref["max_in"], N, E)


def test_every_case_still_holds_what_it_exists_for():
    ref = {k: S.reference(k) for k in S.SMALL}
    size = {k: (N, u.shape[0], ref[k]["T"]) for k, (u, v, N) in S.cases().items() if k != S.LARGE}
    for k, T in S.EXPECTED_T.items():
        assert ref[k]["T"] == T, k
    assert size["one_atom_12_self"] == (1, 12, 132) and ref["one_atom_12_self"]["self_images"] == 12
    assert np.array_equal(np.diff(ref["one_atom_12_self"]["lg_seg_ptr"]), np.full(12, 11))  # every segment omits its own bond
    assert size["one_self"] == (1, 1, 0) and size["one_directed"] == (2, 1, 0) and ref["one_directed"]["max_in"] == 0
    assert ref["sinks_only"]["max_in"] == 0 and ref["sources_only"]["max_in"] == 0 and ref["pair"]["max_in"] == 1
    for k in ("isolated_first_and_last",):
        (u, v, N), r = S.cases()[k], ref[k]
        both = np.concatenate([u, v])
        assert 0 not in both and N - 1 not in both and r["self_images"] == 1 and r["T"] > 0
        assert r["seg_ptr"][0] == r["seg_ptr"][1] == 0 and r["seg_ptr"][N - 1] == r["seg_ptr"][N] == u.shape[0]
    for E in (255, 256, 257):
        assert size[f"E_{E}"][:2] == (9, E) and 0.1 * E < ref[f"E_{E}"]["self_images"] < 0.3 * E
    for N in (2, 3, 4, 5, 16, 17, 255, 256, 257):
        (u, v, n), r = S.cases()[f"N_{N}"], ref[f"N_{N}"]
        assert n == N and u.shape[0] == 40 and N - 1 in u and N - 1 in v
        assert r["seg_ptr"][N] > r["seg_ptr"][N - 1] and r["out_ptr"][N] > r["out_ptr"][N - 1]
    for T in (255, 256, 257):
        assert ref[f"T_{T}"]["self_images"] == 16
    hub = ref["hub_300"]
    assert hub["max_in"] == 300 and hub["T"] == 300 and size["hub_300"][1] == 301
    assert hub["seg_ptr"][1] - hub["seg_ptr"][0] == 300 and hub["out_ptr"][1] - hub["out_ptr"][0] == 1
    cr = ref["crystal_1_6_2"]
    assert size["crystal_1_6_2"][0] == 9 and cr["self_images"] >= 12  # (the one-atom cell: every bond of it is a self image)
    # mixed_self_multi: inside ONE segment of a self image e2 there are rows before and after e2's own place, and ONE source e1
    # reaches self images on both sides of itself as well as bonds that are none
    m = ref["mixed_self_multi"]
    is_self = m["src"] == m["dst"]
    seg_ok = src_ok = False
    for e in np.nonzero(is_self)[0]:
        rows_in = m["lg_src"][m["lg_dst"] == e]
        seg_ok |= bool((rows_in < e).any() and (rows_in > e).any())
        to = m["lg_dst"][m["lg_src"] == e]
        src_ok |= bool((is_self[to] & (to < e)).any() and (is_self[to] & (to > e)).any() and (~is_self[to]).any())
    assert seg_ok and src_ok and size["mixed_self_multi"][:2] == (2, 9)
    assert (~is_self[m["lg_dst"]]).any() and (~is_self[m["lg_src"]]).any()


def test_the_large_case_is_built_by_sorting_in_well_under_a_second():
    u, v, N = S.cases()[S.LARGE]
    t0 = time.perf_counter()
    ref = S.by_sorting(u, v, N)
    dt = time.perf_counter() - t0
    E, T = u.shape[0], ref["T"]
    print(f"stage-ref large: N {N} E {E} T {T} max_in {ref['max_in']} self {ref['self_images']}  by_sorting {dt * 1e3:.0f} ms")
    assert dt < 1.0
    assert 5900 <= N <= 6100 and 69000 <= E <= 71000 and T > 256 * 1024
    assert 0.04 * E < ref["self_images"] < 0.06 * E
    assert int((np.bincount(np.concatenate([u, v]), minlength=N) == 0).sum()) >= (3 * N) // 100
    # the defining properties, checked without the construction: every row joins an in-edge and an out-edge of one atom, no row
    # twice, none with e1 == e2, as many as the degrees say, in (segment, source) order
    e1, e2 = ref["lg_src"], ref["lg_dst"]
    assert np.array_equal(ref["dst"][e1], ref["src"][e2]) and not (e1 == e2).any()
    indeg = np.bincount(v, minlength=N)
    assert T == int(indeg[u].sum()) - ref["self_images"]
    key = ref["out_rank"][e2] * E + e1
    assert (np.diff(key) > 0).all()
    assert np.array_equal(ref["lg_seg_rank"], ref["out_rank"][e2])
    assert np.array_equal(np.sort(ref["lg_out_slot"]), np.arange(T)) and (np.diff(e1[ref["lg_out_slot"]]) >= 0).all()
