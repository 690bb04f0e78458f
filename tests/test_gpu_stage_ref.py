"""csrc/stage.hip - alignn_stage_batch and alignn_map_line_graph_rows, seven kernels, two radix sorts and two scans that build
every index table the convolution, norm and angle kernels address rows with - through the C ABI against tests/stage_ref.py, a
reference written from the definition in include/alignn_hip.h alone (tests/test_stage_ref.py holds it to the other
descriptions on the CPU), on the bond lists of stage_ref.cases(): E, N + 1 and T on either side of the 256-thread block, the
sorts' key width at N = 1, 2, 2^k, 2^k + 1, T = 0, a batch of self images only, an atom with more in-edges than a block has
threads, and one list large enough for many sort tiles and scan blocks.

Every operand, output and the workspace (exactly alignn_stage_batch_workspace bytes) is a buffer of its own between guard
bands (tests/gate_parity).  Integer guards and unwritten outputs hold gate_parity.INT_PATTERN - negative, no zero byte - so a
stray ZERO (ptr[0], the closing zeros of the counts) shows, and so does an element a call should have written and did not.
Everything is compared exactly; the one tolerance is the cosine bound tests/test_gpu_ff_head.py already uses (ff_head_ref.B_VALUE
plus 4 x the float32 restatement's error), for ``h``.

Each case prints a line ``stage-pin ...`` (profiles/stage_pins.txt keeps one run)."""

import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from alignn_amd import ALIGNN, ALIGNNConfig, _lib, loader  # noqa: E402
from alignn_amd import graph as G  # noqa: E402
from alignn_amd._lib import stream  # noqa: E402
from alignn_amd.synthetic import _one, batch_raw, line_graph_coo  # noqa: E402
from tests import ff_head_ref as R  # noqa: E402
from tests import stage_ref as S  # noqa: E402
from tests.gate_parity import INT_PATTERN, NAN_BITS, Report, gptr, guard_input, guarded  # noqa: E402

DEV = "cuda"
I32, I64, F32, U8 = torch.int32, torch.int64, torch.float32, torch.uint8
INVALID = 1  # hipErrorInvalidValue
# the outputs in the order of the prototype; the last four and the operand r are optional
OUTPUTS = ("seg_ptr", "src", "dst", "out_ptr", "out_slot", "perm", "inv", "r_canon", "lg_seg_ptr", "lg_src", "lg_dst", "lg_out_ptr",
           "lg_out_slot", "lg_seg_rank", "lg_ident", "h", "out_rank")
OPTIONAL = ("r_canon", "lg_ident", "h", "out_rank")
MANDATORY = tuple(k for k in OUTPUTS if k not in OPTIONAL)
FLOATS = ("r_canon", "h")


def _dtype(name):
    return F32 if name in FLOATS else getattr(torch, S.DTYPE[name])


def _pat(t, **kw):
    return guard_input(t, pattern=INT_PATTERN[t.dtype], **kw)


def _bits(t):
    return t.view(I32) if t.dtype == F32 else t


def _untouched(t):
    """the payload still holds what ``guarded`` put there"""
    return bool((_bits(t) == (NAN_BITS if t.dtype == F32 else INT_PATTERN[t.dtype])).all())


@functools.lru_cache(maxsize=None)
def _bonds(name):
    u, v, N = S.cases()[name]
    return torch.tensor(u, dtype=I32), torch.tensor(v, dtype=I32), torch.from_numpy(S.bond_vectors(u.shape[0])), N


class _Call:
    """one alignn_stage_batch call on fresh guarded buffers: ``o`` name -> output payload (the T-sized ones one element long when
    T == 0), ``ws`` the workspace"""

    def __init__(self, lib, name, optional=True):
        u, v, r, N = _bonds(name)
        self.N, self.E, self.T = N, int(u.numel()), S.reference(name)["T"]
        self.u, self.v = _pat(u.to(DEV), name="u"), _pat(v.to(DEV), name="v")
        self.r = guard_input(r.to(DEV), name="r") if optional else None
        self.o = {}
        for k in OUTPUTS:
            if not optional and k in OPTIONAL:
                continue
            n = max(self.T if k == "h" else S.length(k, N, self.E, self.T), 1)
            dt = _dtype(k)
            self.o[k] = guarded((self.E, 3) if k == "r_canon" else (n,), dt, name=k, pattern=None if dt == F32 else INT_PATTERN[dt])
        self.ws_bytes = int(lib.alignn_stage_batch_workspace(N, self.E))
        assert self.ws_bytes > 0
        self.ws = guarded((self.ws_bytes,), U8, name="workspace", pattern=INT_PATTERN[U8])
        self.lib = lib

    def run(self, drop=(), ws_bytes=None, **sizes):
        """``drop``: arguments handed as NULL; ``sizes``: N, E, T other than the case's"""
        p = lambda k, t: None if (t is None or k in drop) else gptr(t)  # noqa: E731
        n = {"N": self.N, "E": self.E, "T": self.T, **sizes}
        rc = self.lib.alignn_stage_batch(p("u", self.u), p("v", self.v), p("r", self.r), n["N"], n["E"], n["T"],
                                         *(p(k, self.o.get(k)) for k in OUTPUTS), p("workspace", self.ws),
                                         self.ws_bytes if ws_bytes is None else ws_bytes, stream())
        torch.cuda.synchronize()
        return rc

    def host(self):
        return {k: t.cpu() for k, t in self.o.items()}


def _compare(rep, what, call, name):
    """every output of ``call`` against the reference of case ``name``: dtype, length, every element; the failures are
    collected (Report.finish raises them together)"""
    ref, (_u, _v, r, N) = S.reference(name), _bonds(name)
    E, T = call.E, call.T
    got = call.host()
    fail = lambda *a: rep.failed.append((what,) + a)  # noqa: E731
    for k, t in got.items():
        if k in FLOATS:
            continue
        n = S.length(k, N, E, T)
        if t.dtype != _dtype(k) or t.numel() != max(n, 1):
            fail(k, "dtype / length", t.dtype, t.numel())
        elif n == 0:
            if not _untouched(t):
                fail(k, "T == 0: the one-element buffer was written", t.tolist())
        else:
            want = torch.from_numpy(ref[k].astype(S.DTYPE[k]))
            if not torch.equal(t, want):
                bad = (t != want).nonzero().flatten()
                fail(k, f"{bad.numel()} of {n} elements differ, first at {int(bad[0])}: got {int(t[bad[0]])} want {int(want[bad[0]])}")
    if "r_canon" in got and not torch.equal(got["r_canon"].view(I32), r[torch.tensor(ref["perm"])].view(I32)):
        fail("r_canon", "is not r[perm] bit for bit")
    if "h" in got and T == 0 and not _untouched(got["h"]):
        fail("h", "T == 0: the one-element buffer was written")
    for t, want, k in ((call.u, _bonds(name)[0], "u"), (call.v, _bonds(name)[1], "v")) + (((call.r, r, "r"),) if call.r is not None else ()):
        if not torch.equal(_bits(t.cpu()), _bits(want)):
            fail(k, "an operand was written")
    return got


def _same(rep, what, a, b, keys):
    for k in keys:
        if not torch.equal(_bits(a[k]), _bits(b[k])):
            rep.failed.append((what, k, "bits differ"))


@pytest.mark.parametrize("name", S.ALL)
def test_every_output_equals_the_brute_force_line_graph(name):
    """all outputs given, twice (the same bits), then with r, r_canon, h, lg_ident and out_rank NULL (the mandatory outputs: the
    same bits); ``h`` bit for bit what alignn_bond_cosine_fwd gives on the same rows and within the cosine bound of the float64
    cosine of the REFERENCE's rows"""
    rep = Report(name, "stage-pin")
    lib = rep.launcher(_lib.load())
    ref = S.reference(name)
    calls = [_Call(lib, name), _Call(lib, name), _Call(lib, name, optional=False)]
    for c in calls:
        assert c.run() == 0, name
    got = [_compare(rep, what, c, name) for what, c in zip(("all outputs", "all outputs, again", "optional NULL"), calls)]
    _same(rep, "second run", got[0], got[1], OUTPUTS)
    _same(rep, "optional NULL", got[0], got[2], MANDATORY)
    T, full = ref["T"], calls[0]
    if T > 0:
        h2 = guarded((T,), F32, name="h")
        assert lib.alignn_bond_cosine_fwd(gptr(full.o["r_canon"]), gptr(full.o["lg_src"]), gptr(full.o["lg_dst"]), gptr(h2), T, stream()) == 0
        torch.cuda.synchronize()
        _same(rep, "alignn_bond_cosine_fwd on the same rows", got[0], {"h": h2.cpu()}, ("h",))
        rc = _bonds(name)[2][torch.tensor(ref["perm"])]
        e1, e2 = torch.tensor(ref["lg_src"]), torch.tensor(ref["lg_dst"])
        rep.close("stage_batch", "h", got[0]["h"], R.bond_cosine(rc.double(), e1, e2), R.bond_cosine(rc, e1, e2), R.B_VALUE)
    launches = sum(n for n, _ in rep.guards.launches.values())
    checked = 2 * len(rep.guards.bufs)
    rep.finish()
    print(f"stage-pin {name:<24s} N {full.N:5d} E {full.E:6d} T {T:7d} max_in {ref['max_in']:4d} self {ref['self_images']:5d} "
          f"launches {launches} guards {checked}")


# ----------------------------------------------------------------------------------------------------------------------
# refusals
# ----------------------------------------------------------------------------------------------------------------------
def test_refusals_return_invalid_value_and_touch_nothing():
    name = "mixed_self_multi"
    rep = Report("refusals", "stage-pin")
    lib = rep.launcher(_lib.load())
    c = _Call(lib, name)
    tries = {"N = 0": dict(N=0), "E = 0": dict(E=0), "T < 0": dict(T=-1), "workspace one byte short": dict(ws_bytes=c.ws_bytes - 1),
             "r without r_canon": dict(drop=("r_canon",)), "h without r": dict(drop=("r", "r_canon"))}
    null = ("u", "v") + MANDATORY + ("workspace",)
    assert len(null) == 16
    tries.update({f"{k} NULL": dict(drop=(k,)) for k in null})
    rcs = {k: c.run(**kw) for k, kw in tries.items()}
    assert rcs == {k: INVALID for k in tries}, {k: rc for k, rc in rcs.items() if rc != INVALID}
    assert all(_untouched(t) for t in c.o.values()) and _untouched(c.ws), [k for k, t in c.o.items() if not _untouched(t)]
    u, v, r, _N = _bonds(name)
    assert torch.equal(c.u.cpu(), u) and torch.equal(c.v.cpu(), v) and torch.equal(c.r.cpu().view(I32), r.view(I32))
    rep.finish()
    assert c.run() == 0  # (the same buffers are a valid call)
    _compare(rep, "after the refusals", c, name)
    rep.finish()


# ----------------------------------------------------------------------------------------------------------------------
# alignn_map_line_graph_rows
# ----------------------------------------------------------------------------------------------------------------------
MAP_TABLES = ("inv", "seg_ptr", "src", "dst", "out_rank", "lg_seg_ptr")
BAD0 = 7  # what *bad holds before a call with a defect: the count is added to


def _map(lib, tabs, lu, lv, E, T, bad0=0):
    lu_d, lv_d = _pat(torch.from_numpy(lu).to(DEV), name="lg_u"), _pat(torch.from_numpy(lv).to(DEV), name="lg_v")
    perm = guarded((T,), I64, fill=-1, name="perm", pattern=INT_PATTERN[I64])
    inv_lg = guarded((T,), I64, name="inv_lg", pattern=INT_PATTERN[I64])
    bad = guarded((1,), I32, fill=bad0, name="bad", pattern=INT_PATTERN[I32])
    rc = lib.alignn_map_line_graph_rows(gptr(lu_d), gptr(lv_d), *(gptr(tabs[k]) for k in MAP_TABLES), E, T, gptr(perm), gptr(inv_lg),
                                        gptr(bad), stream())
    torch.cuda.synchronize()
    assert rc == 0
    assert torch.equal(lu_d.cpu(), torch.from_numpy(lu)) and torch.equal(lv_d.cpu(), torch.from_numpy(lv))
    return perm.cpu().numpy(), inv_lg.cpu().numpy(), int(bad)


def _perm_of(rows, T, skip=()):
    """perm as the header defines it: -1, then perm[row of k] = k for every caller edge that is a row"""
    want = np.full(T, -1, dtype=np.int64)
    is_row = rows >= 0
    is_row[list(skip)] = False
    k = np.nonzero(is_row)[0]
    want[rows[k]] = k
    return want


@pytest.mark.parametrize("name", [k for k in S.ALL if S.EXPECTED_T.get(k, 1) > 0])
def test_the_callers_line_graph_is_mapped_onto_the_reference_rows(name):
    """the caller's list = synthetic.line_graph_coo of the caller's bonds, in its own order and shuffled: bad == 0 and row inv_lg[k]
    of the reference is (inv[lg_u[k]], inv[lg_v[k]]), perm its inverse.  Then one defect at a time - an id of -1, an id of E, a
    pair (e, e), a pair that is not adjacent, one edge in three places - on top of a non-zero *bad: the count grows by the
    offending entries (for the repeat: the two extra copies, whichever of the three the kernel lets win), inv_lg is -1 exactly
    there and every other edge is mapped as before.  The tables are the REFERENCE's, so this holds without alignn_stage_batch."""
    u, v, N = S.cases()[name]
    ref = S.reference(name)
    E, T = u.shape[0], ref["T"]
    rep = Report(name, "stage-pin-map")
    lib = rep.launcher(_lib.load())
    tabs = {k: _pat(torch.from_numpy(ref[k].astype(S.DTYPE[k])).to(DEV), name=k) for k in MAP_TABLES}
    own_u, own_v = line_graph_coo(u, v, N)
    assert own_u.shape == own_v.shape == (T,)
    mix = np.random.default_rng(T).permutation(T)
    for what, lu, lv in (("own order", own_u, own_v), ("shuffled", own_u[mix], own_v[mix])):
        perm, inv_lg, bad = _map(lib, tabs, lu, lv, E, T)
        assert bad == 0, (name, what, bad)
        assert inv_lg.min() >= 0 and inv_lg.max() < T, (name, what)
        assert np.array_equal(ref["lg_src"][inv_lg], ref["inv"][lu]) and np.array_equal(ref["lg_dst"][inv_lg], ref["inv"][lv]), (name, what)
        assert np.array_equal(perm[inv_lg], np.arange(T)), (name, what)
        assert np.array_equal(inv_lg, S.line_graph_rows(ref, ref["inv"], lu, lv)), (name, what)
    lu0, lv0 = own_u[mix], own_v[mix]
    k0 = T // 2
    far = np.nonzero(u != v[lu0[k0]])[0]  # bonds that do not leave the atom edge lu0[k0] arrives at
    defects = {"id -1": ((k0,), -1, None), "id E": ((k0,), None, E), "pair (e, e)": ((k0,), None, lu0[k0])}
    if far.size:  # (one_atom_12_self has none: every pair of its bonds is adjacent)
        defects["not adjacent"] = ((k0,), None, far[0])
    else:
        assert N == 1
    done = []
    for what, (at, new_u, new_v) in defects.items():
        lu, lv = lu0.copy(), lv0.copy()
        for k in at:
            lu[k], lv[k] = (lu[k] if new_u is None else new_u), (lv[k] if new_v is None else new_v)
        rows = S.line_graph_rows(ref, ref["inv"], lu, lv)
        assert np.array_equal(np.nonzero(rows < 0)[0], np.sort(at)), (name, what)
        perm, inv_lg, bad = _map(lib, tabs, lu, lv, E, T, BAD0)
        assert bad == BAD0 + len(at), (name, what, bad)
        assert np.array_equal(inv_lg, rows), (name, what)
        assert np.array_equal(perm, _perm_of(rows, T)), (name, what)
        done.append(what)
    # one edge in 1 + copies places: the row is claimed once, the other claims are counted
    group = [k0] + [(k0 + i) % T for i in range(1, min(2, T - 1) + 1)]
    lu, lv = lu0.copy(), lv0.copy()
    lu[group], lv[group] = lu0[k0], lv0[k0]
    rows = S.line_graph_rows(ref, ref["inv"], lu, lv)
    assert (rows >= 0).all() and (rows[group] == rows[k0]).all()
    perm, inv_lg, bad = _map(lib, tabs, lu, lv, E, T, BAD0)
    assert bad == BAD0 + len(group) - 1, (name, "repeat", bad)
    rest = np.setdiff1d(np.arange(T), group)
    assert np.array_equal(inv_lg[rest], rows[rest]), (name, "repeat")
    assert sorted(inv_lg[group].tolist()) == [-1] * (len(group) - 1) + [int(rows[k0])], (name, "repeat", inv_lg[group])
    want = _perm_of(rows, T, skip=group)
    assert perm[rows[k0]] in group and np.array_equal(np.delete(perm, rows[k0]), np.delete(want, rows[k0])), (name, "repeat")
    done.append(f"repeat x{len(group)}")
    launches = sum(n for n, _ in rep.guards.launches.values())
    checked = 2 * len(rep.guards.bufs)
    rep.finish()
    print(f"stage-pin-map {name:<24s} N {N:5d} E {E:6d} T {T:7d} launches {launches} guards {checked}  defects: {', '.join(done)}")


def test_map_line_graph_rows_refuses_null_pointers_and_ignores_an_empty_list():
    name = "pair"
    ref = S.reference(name)
    E, T = 2, ref["T"]
    rep = Report("map refusals", "stage-pin-map")
    lib = rep.launcher(_lib.load())
    tabs = {k: _pat(torch.from_numpy(ref[k].astype(S.DTYPE[k])).to(DEV), name=k) for k in MAP_TABLES}
    lu, lv = (_pat(torch.from_numpy(x).to(DEV), name=k) for k, x in zip(("lg_u", "lg_v"), line_graph_coo(*S.cases()[name])))
    perm = guarded((T,), I64, fill=-1, name="perm", pattern=INT_PATTERN[I64])
    inv_lg = guarded((T,), I64, name="inv_lg", pattern=INT_PATTERN[I64])
    bad = guarded((1,), I32, fill=BAD0, name="bad", pattern=INT_PATTERN[I32])
    ptrs = [lu, lv] + [tabs[k] for k in MAP_TABLES] + [perm, inv_lg, bad]

    def run(null=None, E=E, T=T):
        a = [None if i == null else gptr(t) for i, t in enumerate(ptrs)]
        rc = lib.alignn_map_line_graph_rows(*a[:8], E, T, *a[8:], stream())
        torch.cuda.synchronize()
        return rc

    assert [run(i) for i in range(len(ptrs))] == [INVALID] * len(ptrs)
    assert run(E=0) == INVALID
    assert run(T=0) == 0  # nothing to map
    assert bool((perm == -1).all()) and _untouched(inv_lg) and int(bad) == BAD0
    rep.finish()


# ----------------------------------------------------------------------------------------------------------------------
# the two Python routes on the same cases
# ----------------------------------------------------------------------------------------------------------------------
FIELDS = "seg_ptr seg_node src dst out_ptr out_slot perm inv grp_seg_ptr grp_src_ptr seg_rank".split()


def _want_graphs(ref, N, E):
    """(g, lg): field -> (torch dtype, numpy values or None) as both routes must lay the reference out in a CSRGraph"""
    f = lambda k: (getattr(torch, S.DTYPE[k]), ref[k])  # noqa: E731
    g = dict(seg_ptr=f("seg_ptr"), seg_node=None, src=f("src"), dst=f("dst"), out_ptr=f("out_ptr"), out_slot=f("out_slot"),
             perm=f("perm"), inv=f("inv"), grp_seg_ptr=None, grp_src_ptr=None, seg_rank=None)
    lg = dict(seg_ptr=f("lg_seg_ptr"), seg_node=f("out_slot"), src=f("lg_src"), dst=f("lg_dst"), out_ptr=f("lg_out_ptr"),
              out_slot=f("lg_out_slot"), perm=f("lg_ident"), inv=f("lg_ident"), grp_seg_ptr=f("out_ptr"), grp_src_ptr=f("seg_ptr"),
              seg_rank=f("lg_seg_rank"))
    return (g, (N, E, 0)), (lg, (E, ref["T"], ref["max_in"]))


def _graphs_equal_reference(route, graphs, ref, N, E):
    for which, got, (want, sizes) in zip(("g", "lg"), graphs, _want_graphs(ref, N, E)):
        assert (got.n_nodes, got.n_edges, got.dense_max_src) == sizes, (route, which)
        for k in FIELDS:
            x = getattr(got, k)
            assert (x is None) == (want[k] is None), (route, which, k)
            if x is not None:
                dt, val = want[k]
                assert x.dtype == dt and x.shape == val.shape and x.is_cuda, (route, which, k, x.dtype, x.shape)
                assert np.array_equal(x.cpu().numpy(), val), (route, which, k)


def _tensors_equal(route, k, x, y):
    assert torch.is_tensor(x) and torch.is_tensor(y), (route, k, type(x), type(y))
    assert x.dtype == y.dtype and x.shape == y.shape and torch.equal(_bits(x.contiguous()), _bits(y.contiguous())), (route, k)


@pytest.mark.parametrize("name", S.ALL)
def test_loader_stage_and_csr_and_line_graph_equal_the_reference_both_ways(name):
    """loader.stage (through loader.pack) and graph.csr_and_line_graph, each with STAGE_HIP on and off: every field of g and L(g),
    the sizes, dense_max_src, r and h agree with the reference and with each other in dtype, shape and bits - T == 0 included,
    where h is an EMPTY tensor on both routes"""
    u, v, N = S.cases()[name]
    ref = S.reference(name)
    E, T = u.shape[0], ref["T"]
    r = S.bond_vectors(E)
    r_canon = torch.from_numpy(r[ref["perm"]])
    p = loader.pack(u, v, [N], r, np.eye(3, dtype=np.float32)[None], atom_features=np.zeros((N, 4), np.float32),
                    target=np.zeros(1, np.float32))
    assert (p.num_triplets, p.max_in_degree) == (T, ref["max_in"])
    staged = {}
    for flag in (True, False):
        loader.STAGE_HIP = flag
        try:
            staged[flag] = loader.stage(p, DEV)
        finally:
            loader.STAGE_HIP = True
    torch.cuda.synchronize()
    (a, ta), (b, tb) = staged[True], staged[False]
    assert "staged_block" in a.cache and "staged_block" not in b.cache
    for route, batch in (("loader.stage HIP", a), ("loader.stage torch", b)):
        _graphs_equal_reference(route, (batch.g, batch.lg), ref, N, E)
        _tensors_equal(route, "r", batch.r.cpu(), r_canon)
        assert torch.is_tensor(batch.h) and batch.h.dtype == F32 and batch.h.shape == (T,), (route, "h")
    for k in ("graph_ptr", "atom_features", "r", "h", "volume"):
        _tensors_equal("loader.stage HIP vs torch", k, getattr(a, k), getattr(b, k))
    _tensors_equal("loader.stage HIP vs torch", "target", ta, tb)
    if T > 0:
        e1, e2 = torch.tensor(ref["lg_src"]), torch.tensor(ref["lg_dst"])
        rep = Report(name, "stage-pin-routes")
        rep.close("loader.stage", "h", a.h.cpu(), R.bond_cosine(r_canon.double(), e1, e2), R.bond_cosine(r_canon, e1, e2), R.B_VALUE)
        rep.finish()
    ud, vd, rd = torch.from_numpy(u.copy()).to(DEV), torch.from_numpy(v.copy()).to(DEV), torch.from_numpy(r).to(DEV)
    built = {}
    for flag in (True, False):
        G.STAGE_HIP = flag
        try:
            built[flag] = G.csr_and_line_graph(ud, vd, N, rd)
        finally:
            G.STAGE_HIP = True
    torch.cuda.synchronize()
    for route, (g, lg, rr) in (("csr_and_line_graph HIP", built[True]), ("csr_and_line_graph torch", built[False])):
        _graphs_equal_reference(route, (g, lg), ref, N, E)
        _tensors_equal(route, "r", rr.cpu(), r_canon)
    assert built[True][1].perm is built[True][1].inv and built[False][1].perm is built[False][1].inv


def test_a_training_step_on_the_one_atom_cell_batch_is_bit_identical_both_ways():
    """crystal_1_6_2 (a one-atom cell: every bond of it a self image) staged by alignn_stage_batch and by the torch builders: the
    loss and every gradient of a small model are the same bits"""
    raw = batch_raw([_one(k, 60 + i, "crystal", 92) for i, k in enumerate((1, 6, 2))])
    u, v, N = S.cases()["crystal_1_6_2"]
    assert np.array_equal(raw.u, u) and np.array_equal(raw.v, v) and raw.num_nodes == N
    p = loader.pack_raw(raw, target=np.arange(raw.batch_size, dtype=np.float32))
    outs = []
    for flag in (True, False):
        loader.STAGE_HIP = flag
        try:
            batch, t = loader.stage(p, DEV)
        finally:
            loader.STAGE_HIP = True
        assert ("staged_block" in batch.cache) == flag
        torch.manual_seed(0)
        m = ALIGNN(ALIGNNConfig(name="alignn", alignn_layers=2, gcn_layers=2, hidden_features=64, embedding_features=32)).to(DEV).train()
        loss = torch.nn.functional.l1_loss(m(batch), t)
        loss.backward()
        torch.cuda.synchronize()
        outs.append([loss.detach().clone()] + [q.grad.clone() for q in m.parameters() if q.grad is not None])
    assert len(outs[0]) == len(outs[1]) > 10 and all(torch.equal(x, y) for x, y in zip(*outs))
    assert bool(torch.isfinite(outs[0][0]))
