"""csrc/embed.hip and csrc/ff.hip - geometry features, pooling, gathers, the ALIGNN-FF head and the seeds of the second-order pass
- entry point by entry point and output by output against the float64 restatements of tests/ff_head_ref.py (whose derivatives are
autograd / jvp of forward formulas: no derivative formula is shared with a kernel).

Three kinds of assertion, none of which takes anything from the kernel's own output:

* exact (``torch.equal``): inputs are small integers or dyadic fractions, so every partial sum is representable and any order of
  summation gives the same bits; an indexing error has no tolerance to hide behind.
* float64 parity (``_parity``), for what has a bound in the existing suite: 2e-6 absolute for an RBF value, 1e-6 of the largest
  element for lengths, cosines and means, 2e-5 of the largest element for gradients and tangents - plus 4x the error of the SAME
  restatement evaluated in float32 on the CPU on the same float32 inputs (the convention of tests/test_gpu_convln.py: the
  margin covers ``__expf`` and another summation order).
* format bound (``_within_roundoff``), for plain sums of n terms (segment sums, force reduction, stress, penalty, the seeds):
  element by element |got - float64| <= gamma_n * sum |terms|, gamma_n = n u / (1 - n u), u = 2^-24 - the classical bound of a
  float32 sum of n terms in ANY order (n counts every rounding on the way); the float32 restatement's error is printed beside.

The cosine derivatives are compared element by element, normalised by their own scale (|gh| / min(|a|, |b|) for the reverse,
|at| / |a| + |bt| / |b| for the tangent; NOT by the reference value, which vanishes at collinear triplets).  Where a triplet is
within sin(theta) < 1e-3 of collinear, float32 and float64 may decide the clamp differently (|c| is within a few ulp of 1); the
masked and the unmasked derivative differ by sin(theta) times the scale there, which is what such a triplet is allowed on top.

Every line ``ff-head-parity ...`` a test prints is a measured error (profiles/ff_head_float64_parity.txt keeps one run)."""

import functools
import math
import zlib
from types import SimpleNamespace

import pytest
import torch

pytestmark = pytest.mark.gpu

from alignn_amd import GraphBatch, _lib, ff, ff2, ops  # noqa: E402
from alignn_amd._lib import ptr, stream  # noqa: E402
from alignn_amd.graph import build_csr  # noqa: E402
from alignn_amd.synthetic import _one, batch_raw, make_batch  # noqa: E402
from tests import ff_head_ref as R  # noqa: E402

DEV = "cuda"
F32, F64 = torch.float32, torch.float64
U = 2.0 ** -24  # unit roundoff of float32
INVALID = 1  # hipErrorInvalidValue
B_RBF, B_VALUE, B_GRAD = R.B_RBF, R.B_VALUE, R.B_GRAD  # the existing suite's bounds (module docstring): 2e-6, 1e-6, 2e-5
SENTINEL = 777.0


def _seed(text):
    return torch.Generator().manual_seed(zlib.crc32(text.encode()))


def dev(t):
    return None if t is None else t.to(DEV).contiguous()


def i32(x):
    return torch.as_tensor(x).to(torch.int32)


def host(t):
    return t.detach().cpu()


def _parity(case, name, got, ref64, ref32, base, kind="rel"):
    """4 x (float32 restatement's error) + base, on max |a - b| (``abs``) or max |a - b| / max |b| (``rel``)"""
    got, ref64 = host(got).double().reshape(-1), ref64.double().reshape(-1)
    assert got.shape == ref64.shape, (case, name, got.shape, ref64.shape)
    den = 1.0 if kind == "abs" else max(float(ref64.abs().max()) if ref64.numel() else 0.0, 1e-30)
    e = float((got - ref64).abs().max()) / den if got.numel() else 0.0
    e32 = float((ref32.double().reshape(-1) - ref64).abs().max()) / den if got.numel() else 0.0
    allowed = 4 * e32 + base
    print(f"ff-head-parity {case:<44s} {name:<14s} {kind} err {e:8.2e}  float32 {e32:8.2e}  allowed {allowed:8.2e}")
    assert e < allowed, (case, name, e, e32, allowed)


def _within_roundoff(case, name, got, ref64, mag, n, ref32=None):
    """element by element |got - ref64| <= gamma_n * mag (``mag``: sum of the magnitudes of the terms; ``n``: roundings, number or
    tensor)"""
    got, ref64, mag = host(got).double(), ref64.double(), mag.double()
    assert got.shape == ref64.shape, (case, name, got.shape, ref64.shape)
    assert bool(torch.isfinite(got).all()), (case, name, "not finite")
    nu = torch.as_tensor(n, dtype=F64) * U
    tol = nu / (1 - nu) * mag
    err = (got - ref64).abs()
    worst = float((err / tol.clamp_min(1e-300)).max()) if got.numel() else 0.0
    den = max(float(ref64.abs().max()) if got.numel() else 0.0, 1e-30)
    e32 = "       -" if ref32 is None else f"{float((ref32.double() - ref64).abs().max()) / den:8.2e}"
    print(f"ff-head-parity {case:<44s} {name:<14s} rel err {float(err.max()) / den if got.numel() else 0.0:8.2e}  float32 {e32}  "
          f"of the format bound {worst:8.2e}")
    assert bool((err <= tol).all()), (case, name, worst)


def _exact(case, name, got, ref64):
    want = ref64.to(F32)
    assert torch.equal(want.double(), ref64.double()), (case, name, "the reference itself is not representable in float32")
    got = host(got)
    assert got.shape == want.shape and torch.equal(got, want), (case, name, int((got != want).sum()), "elements differ")


def _ok(rc):
    assert rc == 0, rc
    torch.cuda.synchronize()


def _run(fn, *args):
    """launch ``fn`` with device tensors given AS tensors (None: NULL) and wait for it.  The tensors stay referenced until the
    kernel has run: ``ptr(x.to(device))`` of a temporary would hand the kernel memory the allocator has already given away."""
    held = [a for a in args if torch.is_tensor(a)]
    assert all(t.is_cuda and t.is_contiguous() for t in held)
    _ok(fn(*[a.data_ptr() if torch.is_tensor(a) else a for a in args], stream()))
    del held


# ----------------------------------------------------------------------------------------------------------------------
# RBF expansion: forward, reverse, tangent
# ----------------------------------------------------------------------------------------------------------------------
RBF_RANGE = {"edge": (0.0, 8.0), "angle": (-1.0, 1.0)}
RBF_SHAPES = [(rows, bins) for bins in (80, 40, 30, 4, 1) for rows in (1, 255, 257)] + [(524289, 4)]


@pytest.mark.parametrize("kind", ["edge", "angle"])
@pytest.mark.parametrize("rows,bins", RBF_SHAPES)
def test_rbf_forward_reverse_tangent(kind, rows, bins):
    lo, hi = RBF_RANGE[kind]
    gamma = R.rbf_gamma(lo, hi, bins)
    g = _seed(f"rbf {kind} {rows} {bins}")
    c = torch.linspace(lo, hi, bins)
    span = hi - lo
    d = lo + span * torch.rand(rows, generator=g)
    if rows == 1:
        d[0] = lo + 0.3 * span / max(bins - 1, 1)  # between the first two centres
    else:  # on a centre (first, last, middle), between two centres, outside the range on both sides
        special = torch.stack([c[0], c[-1], c[bins // 2], (c[0] + c[min(1, bins - 1)]) / 2 + 0.01 * span,
                               torch.tensor(lo - 0.06 * span), torch.tensor(hi + 0.11 * span), torch.tensor(lo - span), torch.tensor(hi + span)])
        d[: special.numel()] = special
    G, t = torch.randn(rows, bins, generator=g), torch.randn(rows, generator=g)
    ref = {}
    for dt in (F64, F32):
        fn = lambda q, dt=dt: R.rbf(q, c.to(dt), gamma)  # noqa: E731
        ref[dt] = (fn(d.to(dt)), R.grad_of(fn, (d.to(dt),), G.to(dt))[0], R.jvp_of(fn, (d.to(dt),), (t.to(dt),)))
    cd = dev(c)
    dd = dev(d).requires_grad_(True)
    out = ops.rbf_expand(dd, cd, gamma)
    out.backward(dev(G))
    dual = ff2._rbf_dual(dev(d), dev(t), SimpleNamespace(centers=cd, gamma=gamma))
    torch.cuda.synchronize()
    case = f"rbf {kind} rows={rows} bins={bins}"
    assert torch.equal(ops.rbf_expand(dev(d), cd, gamma), out.detach()) and torch.equal(dual.p, out.detach())
    _parity(case, "rbf_fwd", out, ref[F64][0], ref[F32][0], B_RBF, "abs")
    _parity(case, "rbf_bwd", dd.grad, ref[F64][1], ref[F32][1], B_GRAD)
    _parity(case, "rbf_tangent", dual.t, ref[F64][2], ref[F32][2], B_GRAD)


# ----------------------------------------------------------------------------------------------------------------------
# bond length
# ----------------------------------------------------------------------------------------------------------------------
def _bond_vectors(rows, g):
    v = torch.randn(rows, 3, generator=g)
    return v / v.norm(dim=1, keepdim=True) * (0.5 + 11.5 * torch.rand(rows, 1, generator=g))  # lengths 0.5 .. 12


def _norm3(case, r, gcot):
    ref = {dt: (R.bond_length(r.to(dt)), R.grad_of(R.bond_length, (r.to(dt),), gcot.to(dt))[0]) for dt in (F64, F32)}
    rd = dev(r).requires_grad_(True)
    d = ops.bond_length(rd)
    d.backward(dev(gcot))
    torch.cuda.synchronize()
    assert torch.equal(ops.bond_length(dev(r)), d.detach())
    _parity(case, "norm3_fwd", d, ref[F64][0], ref[F32][0], B_VALUE)
    _parity(case, "norm3_bwd", rd.grad, ref[F64][1], ref[F32][1], B_GRAD)
    return d.detach(), rd.grad, ref


@pytest.mark.parametrize("rows", [1, 257, 524289])
def test_bond_length_forward_reverse(rows):
    g = _seed(f"norm3 {rows}")
    _norm3(f"norm3 rows={rows}", _bond_vectors(rows, g), torch.randn(rows, generator=g))


def test_bond_length_of_a_zero_vector():
    """torch.norm's backward takes the subgradient 0 at the zero vector; so must the kernel (g / 0 * 0 would be NaN)"""
    g = _seed("norm3 zero")
    r = _bond_vectors(257, g)
    r[100] = 0.0
    gcot = torch.randn(257, generator=g)
    d, gr, ref = _norm3("norm3 rows=257 one zero vector", r, gcot)
    assert ref[F32][1][100].tolist() == [0.0, 0.0, 0.0] and ref[F64][1][100].tolist() == [0.0, 0.0, 0.0]  # what torch does
    assert float(d[100]) == 0.0 and host(gr)[100].tolist() == [0.0, 0.0, 0.0]
    assert bool(torch.isfinite(gr).all())


# ----------------------------------------------------------------------------------------------------------------------
# bond cosines: forward, reverse, tangent
# ----------------------------------------------------------------------------------------------------------------------
def _hand_pairs():
    """(a, b) float32 [P, 3]: back-tracking (c = +1), straight-through (c = -1), 90 degrees, 1e-2 .. 1e-5 rad from both ends, each at
    length ratios 1, 10 and 1 / 10"""
    g = _seed("cos hand table")
    bases = [torch.tensor([1.0, 0.0, 0.0], dtype=F64), torch.tensor([0.3, -1.7, 2.2], dtype=F64), torch.tensor([2.0, 2.0, 2.0], dtype=F64),
             torch.randn(3, generator=g, dtype=F64) * 3]
    A, Bv = [], []
    for a in bases:
        axis = torch.tensor([0.0, 0.0, 1.0], dtype=F64) if abs(float(a[2])) < 0.9 * float(a.norm()) else torch.tensor([0.0, 1.0, 0.0], dtype=F64)
        p = torch.linalg.cross(a, axis)
        p = p / p.norm() * a.norm()  # perpendicular to a, of its length
        for ratio in (1.0, 10.0, 0.1):
            cand = [-a, a, p]
            for delta in (1e-2, 1e-3, 1e-4, 1e-5):
                for end in (-1.0, 1.0):
                    cand.append(end * (math.cos(delta) * a + math.sin(delta) * p))
            for b in cand:
                A.append(a)
                Bv.append(ratio * b)
    return torch.stack(A).float(), torch.stack(Bv).float()


@functools.lru_cache(maxsize=None)
def _cos_case(name):
    """-> (r float32 [n, 3], e1, e2 int32 [T], CSR line graph or None)"""
    if name in ("line_graph_2x9", "one_atom_cell"):
        raw = make_batch(2, 9, seed0=91) if name == "line_graph_2x9" else batch_raw([_one(1, 50, "crystal", 92)])
        b = GraphBatch.from_raw(raw, device=DEV)
        return host(b.r), host(b.lg.src), host(b.lg.dst), b.lg
    a, b = _hand_pairs()
    r = torch.stack([a, b], 1).reshape(-1, 3)
    P = a.shape[0]
    if name == "hand_table":
        return r, i32(torch.arange(P) * 2), i32(torch.arange(P) * 2 + 1), None
    T = int(name[1:])
    g = _seed("cos " + name)
    r = torch.cat([r, _bond_vectors(64, g)])
    e1, e2 = torch.randint(0, r.shape[0], (T,), generator=g), torch.randint(0, r.shape[0], (T,), generator=g)
    e1[0], e2[0] = 0, 1  # the first triplet back-tracks
    return r, i32(e1), i32(e2), None


def _normalised(got, ref64, scale, allow):
    """max over triplets of (largest component error / scale - what the triplet is allowed for the clamp decision), >= 0"""
    err = (got.double() - ref64).abs().reshape(ref64.shape[0], -1).max(1).values
    return float((err / scale - allow).clamp_min(0).max())


@pytest.mark.parametrize("name", ["line_graph_2x9", "one_atom_cell", "hand_table", "T1", "T257", "T524289"])
def test_bond_cosine_forward_reverse_tangent(name):
    lib = _lib.load()
    r, e1, e2, lg = _cos_case(name)
    T, n = e1.numel(), r.shape[0]
    g = _seed("cos data " + name)
    gh = (0.5 + torch.rand(T, generator=g)) * (1 - 2 * torch.randint(0, 2, (T,), generator=g)).float()  # no zero: the scale below
    rt = torch.randn(n, 3, generator=g)
    l1, l2 = e1.long(), e2.long()
    ref = {}
    for dt in (F64, F32):
        a, b, at, bt = r.to(dt)[l1], r.to(dt)[l2], rt.to(dt)[l1], rt.to(dt)[l2]
        ga, gb = R.grad_of(R.cosine_of_pairs, (a, b), gh.to(dt))
        ref[dt] = dict(h=R.cosine_of_pairs(a, b), ga=ga, gb=gb, ht=R.jvp_of(R.cosine_of_pairs, (a, b), (at, bt)))
    rd, rtd, e1d, e2d = dev(r), dev(rt), dev(e1), dev(e2)
    h = ops.bond_cosines(rd, e1d, e2d)
    h2, ht = ff2._cos_dual(rd, rtd, SimpleNamespace(src=e1d, dst=e2d, n_edges=T))
    ga, gb = torch.full((T, 3), SENTINEL, device=DEV), torch.full((T, 3), SENTINEL, device=DEV)
    _run(lib.alignn_bond_cosine_bwd, rd, e1d, e2d, dev(gh), ga, gb, T)
    case = f"cos {name} T={T}"
    assert torch.equal(h, h2)
    for t_ in (h, ht, ga, gb):
        assert bool(torch.isfinite(t_).all()), case
    assert float(h.max()) <= 1.0 and float(h.min()) >= -1.0
    _parity(case, "cos_fwd", h, ref[F64]["h"], ref[F32]["h"], B_VALUE)
    a, b, at, bt = r.double()[l1], r.double()[l2], rt.double()[l1], rt.double()[l2]
    na, nb = a.norm(dim=1), b.norm(dim=1)
    sin_t = torch.linalg.cross(a, b).norm(dim=1) / (na * nb)
    allow = torch.where(sin_t < 1e-3, sin_t, torch.zeros_like(sin_t))
    s_bwd = gh.double().abs() / torch.minimum(na, nb)
    s_tan = at.norm(dim=1) / na + bt.norm(dim=1) / nb
    for nm, got, key, scale in (("cos_bwd ga", ga, "ga", s_bwd), ("cos_bwd gb", gb, "gb", s_bwd), ("cos_tangent", ht, "ht", s_tan)):
        e = _normalised(host(got), ref[F64][key], scale, allow)
        e32 = _normalised(ref[F32][key], ref[F64][key], scale, allow)
        allowed = 4 * e32 + B_GRAD
        print(f"ff-head-parity {case:<44s} {nm:<14s} nrm err {e:8.2e}  float32 {e32:8.2e}  allowed {allowed:8.2e}")
        assert e < allowed, (case, nm, e, e32, allowed)
    if lg is not None:  # the product's differentiable entry: the reverse kernel + the two segment sums over the line graph
        rq = dev(r).requires_grad_(True)
        hq = ops.bond_cosines(rq, lg)
        hq.backward(dev(gh))
        torch.cuda.synchronize()
        assert torch.equal(hq.detach(), h)
        fn = lambda q: R.bond_cosine(q, e1, e2)  # noqa: E731
        g64, g32 = R.grad_of(fn, (r.double(),), gh.double())[0], R.grad_of(fn, (r,), gh)[0]
        _parity(case, "cos grad r", rq.grad, g64, g32, B_GRAD)


# ----------------------------------------------------------------------------------------------------------------------
# mean pooling
# ----------------------------------------------------------------------------------------------------------------------
POOL_BATCHES = {"ragged": (0, 1, 3, 4, 5, 8, 9, 12, 13, 200), "B1": (7,), "pow2": (1, 0, 2, 4, 8, 16, 256, 64)}


@pytest.mark.parametrize("batch", list(POOL_BATCHES))
@pytest.mark.parametrize("H", [4, 64, 256, 260])
def test_segment_mean_forward_reverse(H, batch):
    counts = POOL_BATCHES[batch]
    gp = torch.zeros(len(counts) + 1, dtype=torch.int32)
    gp[1:] = torch.cumsum(torch.tensor(counts), 0)
    N, B = int(gp[-1]), len(counts)
    g = _seed(f"pool {H} {batch}")
    exact = batch == "pow2"
    if exact:
        x, G = torch.randint(-8, 9, (N, H), generator=g).float(), torch.randint(-8, 9, (B, H), generator=g).float()
    else:
        x, G = torch.randn(N, H, generator=g), torch.randn(B, H, generator=g)
    fn = lambda q: R.segment_mean(q, gp)  # noqa: E731
    ref = {dt: (fn(x.to(dt)), R.grad_of(fn, (x.to(dt),), G.to(dt))[0]) for dt in (F64, F32)}
    xd = dev(x).requires_grad_(True)
    out = ops.AvgPoolFn.apply(xd, dev(gp))
    out.backward(dev(G))
    torch.cuda.synchronize()
    case = f"segment_mean H={H} {batch}"
    if exact:
        _exact(case, "fwd", out, ref[F64][0])
        _exact(case, "bwd", xd.grad, ref[F64][1])
    else:
        _parity(case, "mean_fwd", out, ref[F64][0], ref[F32][0], B_VALUE)
        _parity(case, "mean_bwd", xd.grad, ref[F64][1], ref[F32][1], B_VALUE)


# ----------------------------------------------------------------------------------------------------------------------
# segment sums: both kernels of alignn_segment_sum
# ----------------------------------------------------------------------------------------------------------------------
def _takes_long_kernel(n_seg, F):
    return n_seg * F <= 4096 and F <= 64 and n_seg <= 4096  # the dispatch of alignn_segment_sum


def _segsum_launch(vals, ldv, seg_ptr, slot, node, n_rows_out, ldo, n_seg, F):
    out = torch.full((n_rows_out, ldo), SENTINEL, device=DEV)
    _ok(_lib.load().alignn_segment_sum(ptr(vals), ldv, ptr(seg_ptr), ptr(slot), ptr(node), ptr(out), ldo, n_seg, F, stream()))
    return out


SEGSUM_SHAPES = [(4096, 1), (4097, 1), (64, 64), (65, 64), (1, 65), (16, 9), (5, 3)]


@pytest.mark.parametrize("variant", ["plain", "slot", "node_ld", "slot_node_ld"])
@pytest.mark.parametrize("n_seg,F", SEGSUM_SHAPES)
def test_segment_sum_both_kernels(n_seg, F, variant):
    G = max(256 // F, 1)
    pool = [4 * G + 1, G, 3000, 0, G - 1, 4 * G, 1]
    for rot in (range(0, 7, n_seg) if n_seg < 7 else (0,)):  # few segments: rotate until every length has been used
        lens = torch.tensor([pool[(i + rot) % 7] for i in range(n_seg)])
        sp = torch.zeros(n_seg + 1, dtype=torch.int32)
        sp[1:] = torch.cumsum(lens, 0)
        rows = int(sp[-1])
        g = _seed(f"segsum {n_seg} {F} {variant} {rot}")
        ldv = F + 3 if "ld" in variant else F
        ldo = F + 5 if "ld" in variant else F
        slot = i32(torch.randperm(rows, generator=g)) if "slot" in variant else None
        node = i32(torch.randperm(n_seg, generator=g)) if "node" in variant else None
        for exact in (True, False):
            wide = torch.randint(-8, 9, (rows, ldv), generator=g).float() if exact else torch.randn(rows, ldv, generator=g)
            vals = wide[:, :F]
            ref64 = R.segment_sum(vals.double(), sp, slot, node)
            case = f"segment_sum ({n_seg},{F}) {variant} rot={rot}"
            wd, spd, sd, nd = dev(wide), dev(sp), dev(slot), dev(node)
            out = _segsum_launch(wd, ldv, spd, sd, nd, n_seg, ldo, n_seg, F)
            assert bool((out[:, F:] == SENTINEL).all()), case  # nothing beyond the F columns is written
            outs = {("long" if _takes_long_kernel(n_seg, F) else "short"): host(out[:, :F])}
            # the other kernel on the same segments: padded with empty segments until the dispatch takes the thread-per-output
            # kernel, or (where that is what the shape takes already) without the last segment, if that takes the other
            if _takes_long_kernel(n_seg, F):
                n2 = 4096 // F + 1
                assert n2 > n_seg and not _takes_long_kernel(n2, F)
                sp2 = torch.cat([sp, sp[-1:].expand(n2 - n_seg)])
                node2 = None if node is None else torch.cat([node, i32(torch.arange(n_seg, n2))])
                o2 = _segsum_launch(wd, ldv, dev(sp2), sd, dev(node2), n2, ldo, n2, F)
                assert bool((o2[n_seg:, :F] == 0).all()) and bool((o2[:, F:] == SENTINEL).all()), case
                outs["short"] = host(o2[:n_seg, :F])
                keep = torch.arange(n_seg)
            elif n_seg > 1 and _takes_long_kernel(n_seg - 1, F):
                o2 = _segsum_launch(wd, ldv, dev(sp[:-1]), sd, None if node is None else dev(node[:-1]), n_seg, ldo, n_seg - 1, F)
                keep = torch.arange(n_seg - 1) if node is None else node[:-1].long()
                outs["long"] = host(o2[:, :F])
            else:
                keep = torch.arange(n_seg)
            if exact:
                for k, o in outs.items():
                    sel = keep if (k == "long" and not _takes_long_kernel(n_seg, F)) else torch.arange(n_seg)
                    assert torch.equal(o[sel], ref64.float()[sel]), (case, k)
                if len(outs) == 2:
                    assert torch.equal(outs["long"][keep], outs["short"][keep]), case
            else:
                mag = R.segment_sum(vals.double().abs(), sp, slot, node)
                n_terms = R.segment_sum(torch.ones(rows, 1, dtype=F64), sp, slot, node)
                ref32 = R.segment_sum(vals, sp, slot, node)
                for k, o in outs.items():
                    sel = keep if (k == "long" and not _takes_long_kernel(n_seg, F)) else torch.arange(n_seg)
                    _within_roundoff(case, f"segsum {k}", o[sel], ref64[sel], mag[sel], n_terms[sel].clamp_min(1), ref32[sel])


# ----------------------------------------------------------------------------------------------------------------------
# row gathers
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("perm_kind", ["repeated", "reversed"])
@pytest.mark.parametrize("rows,F", [(300, 3), (300, 4), (300, 256), (131073, 4)])  # the last: past the 2048-workgroup cap
def test_gather_rows(rows, F, perm_kind):
    g = _seed(f"gather {rows} {F} {perm_kind}")
    n_in = 97
    x = torch.randn(n_in, F, generator=g)
    perm = torch.randint(0, n_in, (rows,), generator=g) if perm_kind == "repeated" else torch.arange(rows - 1, -1, -1) % n_in
    out = ff.gather(dev(x), ff.Relation(dev(i32(perm)), None, None, None, n_in))
    torch.cuda.synchronize()
    _exact(f"gather_rows rows={rows} F={F} {perm_kind}", "out", out, R.gather(x.double(), perm))


@pytest.mark.parametrize("rows,F", [(300, 4), (300, 256), (1048577, 4)])  # the last: past the 4096-workgroup cap of the float4 form
def test_gather_rows_column_block_of_a_wider_matrix(rows, F):
    lib = _lib.load()
    g = _seed(f"gather_ld {rows} {F}")
    n_in, ld_in, ld_out, c_in, c_out = 97, F + 8, F + 4, 4, 0
    x = torch.randn(n_in, ld_in, generator=g)
    perm = torch.randint(0, n_in, (rows,), generator=g)
    xd, pd = dev(x), dev(i32(perm))
    out = torch.full((rows, ld_out), SENTINEL, device=DEV)
    _ok(lib.alignn_gather_rows_ld(xd.data_ptr() + 4 * c_in, ld_in, ptr(pd), out.data_ptr() + 4 * c_out, ld_out, rows, F, stream()))
    _exact(f"gather_rows_ld rows={rows} F={F}", "out", out[:, c_out:c_out + F], R.gather(x[:, c_in:c_in + F].double(), perm))
    assert bool((out[:, F:] == SENTINEL).all())


def test_gather_rows_ld_refuses_what_is_not_a_multiple_of_four():
    lib = _lib.load()
    x, out = torch.zeros(8, 16, device=DEV), torch.full((8, 16), SENTINEL, device=DEV)
    perm = dev(i32(torch.arange(8)))
    for F, ld_in, ld_out in ((3, 16, 16), (6, 16, 16), (4, 15, 16), (4, 16, 14), (0, 16, 16)):
        assert lib.alignn_gather_rows_ld(ptr(x), ld_in, ptr(perm), ptr(out), ld_out, 8, F, stream()) == INVALID
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all())


# ----------------------------------------------------------------------------------------------------------------------
# the head: force reduction, stress, energies and penalty
# ----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _force_graph(n):
    g = _seed(f"force graph {n}")
    if n == 1:  # a one-atom cell: self-image bonds only
        u = v = torch.zeros(26, dtype=torch.int64)
    else:  # atoms 0-4: no out-edges; 5-9: neither in nor out; 10-14: no in-edges
        m = 2000
        u = torch.randint(10, n, (m,), generator=g)
        v = torch.randint(0, n - 10, (m,), generator=g)
        v = torch.where(v >= 5, v + 10, v)
    return build_csr(u.to(DEV), v.to(DEV), n)


@pytest.mark.parametrize("add_reverse", [0, 1])
@pytest.mark.parametrize("n", [1, 300])
def test_pair_force_reduce(n, add_reverse):
    lib = _lib.load()
    csr = _force_graph(n)
    src, dst, m = host(csr.src), host(csr.dst), csr.n_edges
    if n == 300:
        deg_in, deg_out = torch.bincount(dst.long(), minlength=n), torch.bincount(src.long(), minlength=n)
        assert bool((deg_in[5:15] == 0).all()) and bool((deg_out[:10] == 0).all()) and int(deg_in[:5].min()) > 0 and int(deg_out[10:15].min()) > 0
    g = _seed(f"pair force {n} {add_reverse}")
    case = f"pair_force_reduce n={n} add_reverse={add_reverse}"
    for exact in (True, False):
        gr = torch.randint(-8, 9, (m, 3), generator=g).float() if exact else torch.randn(m, 3, generator=g)
        scale = -0.5 if exact else -1.7
        s32 = float(torch.tensor(scale, dtype=F32))
        ref64 = s32 * R.forces_of(gr.double(), src, dst, n, bool(add_reverse))
        out = torch.full((n, 3), SENTINEL, device=DEV)
        _run(lib.alignn_pair_force_reduce, dev(gr), scale, csr.seg_ptr, csr.out_ptr if add_reverse else None,
             csr.out_slot if add_reverse else None, add_reverse, out, n)
        if exact:
            _exact(case, "forces", out, ref64)
            prod = ff.pair_force_reduce(dev(gr), csr, bool(add_reverse))  # the product's composed entry (two segment sums)
            torch.cuda.synchronize()
            _exact(case, "ff.pair_force_reduce", prod, R.forces_of(gr.double(), src, dst, n, bool(add_reverse)))
        else:
            mag = abs(s32) * R.forces_of(gr.double().abs(), src, dst, n, False)
            terms = torch.bincount(dst.long(), minlength=n).double()
            if add_reverse:
                mag = mag + abs(s32) * torch.zeros(n, 3, dtype=F64).index_add(0, src.long(), gr.double().abs())
                terms = terms + torch.bincount(src.long(), minlength=n).double()
            _within_roundoff(case, "forces", out, ref64, mag, terms[:, None] + 2, s32 * R.forces_of(gr, src, dst, n, bool(add_reverse)))


def test_pair_force_reduce_refuses_a_missing_out_edge_table():
    lib = _lib.load()
    csr = _force_graph(300)
    gr = torch.ones(csr.n_edges, 3, device=DEV)
    out = torch.full((300, 3), SENTINEL, device=DEV)
    assert lib.alignn_pair_force_reduce(ptr(gr), 1.0, ptr(csr.seg_ptr), None, ptr(csr.out_slot), 1, ptr(out), 300, stream()) == INVALID
    assert lib.alignn_pair_force_reduce(ptr(gr), 1.0, ptr(csr.seg_ptr), ptr(csr.out_ptr), None, 1, ptr(out), 300, stream()) == INVALID
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all())  # refused without a launch


def _crystals(bonds, atoms, g):
    """atom offsets per crystal, bond offsets per atom (bonds sorted by destination atom), E"""
    gp = torch.zeros(len(atoms) + 1, dtype=torch.int32)
    gp[1:] = torch.cumsum(torch.tensor(atoms), 0)
    N = int(gp[-1])
    dst = [torch.sort(torch.randint(int(gp[b]), int(gp[b + 1]), (m,), generator=g)).values for b, m in enumerate(bonds) if m > 0]
    dst = torch.cat(dst) if dst else torch.zeros(0, dtype=torch.int64)
    sp = torch.zeros(N + 1, dtype=torch.int32)
    sp[1:] = torch.cumsum(torch.bincount(dst, minlength=N), 0)
    assert R.edge_ptr_of(gp, sp).tolist() == [0] + torch.cumsum(torch.tensor(bonds), 0).tolist()
    return gp, sp, dst, N


@pytest.mark.parametrize("batch", ["0_1_255_256_257_1000", "B1"])
def test_virial_stress(batch):
    lib = _lib.load()
    bonds, atoms = ((0, 1, 255, 256, 257, 1000), (2, 1, 3, 2, 4, 5)) if batch != "B1" else ((300,), (3,))
    g = _seed("virial " + batch)
    gp, sp, _, N = _crystals(bonds, atoms, g)
    ep, E, B = R.edge_ptr_of(gp, sp), sum(bonds), len(bonds)
    case = f"virial_stress bonds={batch}"
    for exact in (True, False):
        if exact:
            r, gr = torch.randint(-8, 9, (E, 3), generator=g).float() / 2, torch.randint(-8, 9, (E, 3), generator=g).float()
            vol, scale, k = torch.tensor([1.0, 2.0, 4.0, 8.0, 16.0, 32.0])[:B], 2.0, -0.5
        else:
            r, gr = torch.randn(E, 3, generator=g) * 2, torch.randn(E, 3, generator=g)
            vol, scale, k = 20 + 60 * torch.rand(B, generator=g), -1.0, float(torch.tensor(R.STRESS_UNIT, dtype=F32))
        assert B == 1 or len(set(vol.tolist())) == B  # unequal volumes
        ref64 = R.stresses_of(r.double(), scale * gr.double(), ep, vol.double(), k).reshape(B, 9)
        out = torch.full((B, 9), SENTINEL, device=DEV)
        _run(lib.alignn_virial_stress, dev(r), dev(gr), scale, dev(gp), dev(sp), dev(vol), k, out, B)
        if exact:
            _exact(case, "stress", out, ref64)
        else:
            mag = R.stresses_of(r.double().abs(), gr.double().abs(), ep, vol.double(), abs(k)).reshape(B, 9)
            n = torch.tensor(bonds, dtype=F64)[:, None] + 8  # a product per term, the sum, k * scale / V and the last product
            ref32 = R.stresses_of(r, scale * gr, ep, vol, k).reshape(B, 9)
            _within_roundoff(case, "stress", out, ref64, mag, n, ref32)


@pytest.mark.parametrize("use_penalty", [0, 1])
@pytest.mark.parametrize("mult_natoms", [0, 1])
@pytest.mark.parametrize("E", [0, 1000])
@pytest.mark.parametrize("B", [1, 256, 257])
def test_ff_energy_and_penalty_reverse(B, E, mult_natoms, use_penalty):
    lib = _lib.load()
    g = _seed(f"energy {B} {E} {mult_natoms} {use_penalty}")
    counts = torch.tensor([(7 * b + 1) % 5 for b in range(B)])  # 1, 3, 0, 2, 4, ...: a crystal without atoms among them
    gp = torch.zeros(B + 1, dtype=torch.int32)
    gp[1:] = torch.cumsum(counts, 0)
    case = f"ff_energy B={B} E={E} mult={mult_natoms} pen={use_penalty}"
    for exact in (True, False):
        if exact:  # dyadic: below (0.5, 0.75, 0.96875), on (1.0) and above (1.25, 2.0) the threshold
            pred = torch.randint(-64, 65, (B,), generator=g).float() / 16
            bl = torch.tensor([0.5, 0.75, 1.0, 1.25, 2.0, 0.96875])[torch.randint(0, 6, (E,), generator=g)]
            factor, thr = 0.25, 1.0
        else:
            pred, bl = torch.randn(B, generator=g), 0.5 + torch.rand(E, generator=g)
            factor, thr = float(torch.tensor(0.1, dtype=F32)), 1.0
            bl[:3] = torch.tensor([thr, thr - 2.0 ** -20, thr + 2.0 ** -20])[: min(E, 3)]  # on it and one step to either side
        out64, _ = R.energies(pred.double(), bl.double(), gp, bool(mult_natoms), bool(use_penalty), factor, thr)
        seed64 = R.energy_seed(pred.double(), bl.double(), gp, bool(mult_natoms), bool(use_penalty), factor, thr)
        out, seed = torch.full((B,), SENTINEL, device=DEV), torch.full((B,), SENTINEL, device=DEV)
        bld = dev(bl) if E > 0 else torch.zeros(1, device=DEV)  # (E == 0: any non-NULL pointer, never read)
        _run(lib.alignn_ff_energy, dev(pred), bld if use_penalty else None, dev(gp), B, E, mult_natoms, use_penalty, factor, thr, out, seed)
        _exact(case, "seed", seed, seed64)
        if exact or not use_penalty or mult_natoms:
            _exact(case, "out", out, out64)
        else:
            terms = torch.where(bl.double() < thr, factor * (thr - bl.double()), torch.zeros(E, dtype=F64))
            mag = pred.double().abs() + terms.abs().sum()
            out32, _ = R.energies(pred, bl, gp, False, True, factor, thr)
            _within_roundoff(case, "out", out, out64, mag, E + 4, out32)
        # reverse of the penalty: ACCUMULATES -factor * B into what the caller has put there
        pre = torch.randint(-8, 9, (max(E, 1),), generator=g).float()
        gbl = dev(pre)
        _run(lib.alignn_ff_penalty_bwd, bld, gbl, E, B, factor, thr)
        want = pre.double()
        if E > 0:
            want = want + R.penalty_grad(pred.double(), bl.double(), gp, factor, thr)
        if exact:
            _exact(case, "g_bl", gbl, want)
        else:
            _within_roundoff(case, "g_bl", gbl, want, want.abs() + pre.double().abs(), 3)


def test_ff_energy_refuses_a_penalty_without_bond_lengths():
    lib = _lib.load()
    z = torch.zeros(4, device=DEV)
    gp = dev(i32([0, 1, 2, 3, 4]))
    assert lib.alignn_ff_energy(ptr(z), None, ptr(gp), 4, 10, 1, 1, 0.1, 1.0, ptr(z), ptr(z), stream()) == INVALID
    assert lib.alignn_ff_energy(ptr(z), None, ptr(gp), 0, 10, 1, 0, 0.1, 1.0, ptr(z), ptr(z), stream()) == INVALID


# ----------------------------------------------------------------------------------------------------------------------
# seeds of the second-order pass
# ----------------------------------------------------------------------------------------------------------------------
def _weights_batch(E, g):
    """crystals 0, 3 and 5 (first, middle, last) have atoms and no bonds, crystal 2 has no atoms at all: the offsets of both levels
    repeat.  The graph containers take this as it is (offsets are cumulative sums of the counts given)."""
    atoms, bonds = (2, 3, 0, 2, 4, 2), (0, 100, 0, 0, E - 100, 0)
    gp, sp, dst, N = _crystals(bonds, atoms, g)
    own = R.owners(R.edge_ptr_of(gp, sp))
    lo, hi = gp[:-1].long()[own], gp[1:].long()[own]
    src = lo + (torch.rand(E, generator=g) * (hi - lo)).long()
    return gp, sp, i32(src), i32(dst), N, len(atoms)


@pytest.mark.parametrize("add_reverse", [0, 1])
@pytest.mark.parametrize("which", ["forces", "stress", "both"])
@pytest.mark.parametrize("E", [255, 256, 257])
def test_ff_pair_weights(E, which, add_reverse):
    lib = _lib.load()
    g = _seed(f"pair weights {E} {which} {add_reverse}")
    gp, sp, src, dst, N, B = _weights_batch(E, g)
    ep = R.edge_ptr_of(gp, sp)
    case = f"ff_pair_weights E={E} {which} add_reverse={add_reverse}"
    for exact in (True, False):
        if exact:
            gF, gS = torch.randint(-4, 5, (N, 3), generator=g).float(), torch.randint(-4, 5, (B, 3, 3), generator=g).float()
            r, vol, kS = torch.randint(-16, 17, (E, 3), generator=g).float() / 4, torch.tensor([1.0, 2.0, 4.0, 0.5, 8.0, 16.0]), -2.0
        else:
            gF, gS = torch.randn(N, 3, generator=g), torch.randn(B, 3, 3, generator=g)
            r, vol, kS = torch.randn(E, 3, generator=g) * 2, 20 + 60 * torch.rand(B, generator=g), float(torch.tensor(R.STRESS_UNIT, dtype=F32))
        gF_, gS_ = (gF if which != "stress" else None), (gS if which != "forces" else None)
        dbl = lambda t: None if t is None else t.double()  # noqa: E731
        ref64 = R.pair_weights(dbl(gF_), dbl(gS_), r.double(), src, dst, ep, vol.double(), kS, bool(add_reverse), N, E)
        for seeded in (0.0, 2.0 ** 100):
            w, wmax = torch.full((E, 3), SENTINEL, device=DEV), torch.full((1,), seeded, device=DEV)
            need = gS_ is not None
            _run(lib.alignn_ff_pair_weights, dev(gF_), dev(gS_), dev(r), dev(src), dev(dst), dev(gp) if need else None,
                 dev(sp) if need else None, dev(vol) if need else None, kS, add_reverse, B, E, w, wmax)
            if exact:
                _exact(case, "w", w, ref64)
            else:
                mag = torch.zeros(E, 3, dtype=F64)
                if gF_ is not None:
                    mag = mag + gF.double().abs()[dst.long()] + (gF.double().abs()[src.long()] if add_reverse else 0)
                if gS_ is not None:
                    mag = mag + R.pair_weights(None, gS.double().abs(), r.double().abs(), src, dst, ep, vol.double(), abs(kS), False, N, E)
                ref32 = R.pair_weights(gF_, gS_, r, src, dst, ep, vol, kS, bool(add_reverse), N, E)
                _within_roundoff(case, "w", w, ref64, mag, 12, ref32)  # k / V, 3 x (k s) r, 5 sums, and the reverse of each
            # an atomic max on the bit pattern: never falls below what it held, equals the largest |w| written from 0
            want = max(seeded, float(host(w).abs().max()))
            assert float(wmax) == want, (case, float(wmax), want)
            if exact and seeded == 0.0:
                assert float(wmax) == float(ref64.abs().max()), case


WMAX = {"2^3": 8.0, "2^3-1ulp": float(torch.nextafter(torch.tensor(8.0), torch.tensor(0.0))), "zero": 0.0, "2^-100": 2.0 ** -100, "2^100": 2.0 ** 100}


def _w_with_max(shape, wmax, g):
    """float32 w with max |w| == wmax exactly (all zero for wmax == 0)"""
    w = (2 * torch.rand(*shape, generator=g) - 1) * 0.999
    w = (w * torch.tensor(wmax, dtype=F32)).float()
    if wmax > 0:
        w.reshape(-1)[w.numel() // 2] = -wmax
    assert float(w.abs().max()) == wmax
    return w


@pytest.mark.parametrize("wname", list(WMAX))
def test_ff_tangent_geometry(wname):
    lib = _lib.load()
    E, wmax = 300, WMAX[wname]
    g = _seed("tangent geometry " + wname)
    r = _bond_vectors(E, g)
    w = _w_with_max((E, 3), wmax, g)
    d = R.bond_length(r.double()).float()
    rt64, dt64, k = R.tangent_geometry(r.double(), w.double(), wmax)
    rt32, dt32, _ = R.tangent_geometry(r, w, wmax)
    rt, dt = torch.full((E, 3), SENTINEL, device=DEV), torch.full((E,), SENTINEL, device=DEV)
    _run(lib.alignn_ff_tangent_geometry, dev(r), dev(w), torch.tensor([wmax], device=DEV), dev(d), rt, dt, E)
    case = f"ff_tangent_geometry wmax={wname}"
    assert bool(torch.isfinite(rt).all()) and bool(torch.isfinite(dt).all())
    assert torch.equal(host(rt).double() * 2.0 ** k, w.double()), case  # rt * 2^k == w, bit for bit
    _exact(case, "rt", rt, rt64)
    if wmax > 0:
        assert 1.0 <= float(rt.abs().max()) < 2.0
    _parity(case, "dt", dt, dt64, dt32, B_GRAD)


@pytest.mark.parametrize("wname", list(WMAX))
@pytest.mark.parametrize("mult_natoms", [0, 1])
@pytest.mark.parametrize("ge_set", [0, 1], ids=["ge_null", "ge_set"])
@pytest.mark.parametrize("H", [4, 256])
def test_ff_readout_seed_and_fc_grad(H, ge_set, mult_natoms, wname):
    lib = _lib.load()
    wmax = WMAX[wname]
    k = R.pow2_exponent(wmax)
    wm = torch.tensor([wmax], device=DEV)
    g = _seed(f"readout {H} {ge_set} {mult_natoms} {wname}")
    for exact, counts in ((True, (4, 1, 8, 2)), (False, (3, 1, 7, 2))):  # both ragged, both hold a one-atom crystal
        gp = torch.zeros(len(counts) + 1, dtype=torch.int32)
        gp[1:] = torch.cumsum(torch.tensor(counts), 0)
        N, B = int(gp[-1]), len(counts)
        case = f"readout H={H} ge={ge_set} mult={mult_natoms} wmax={wname} counts={counts}"
        if exact:
            q = lambda *s: torch.randint(-16, 17, s, generator=g).float() / 4  # noqa: E731
            fc_w, fc_b, ge, c, hp, hpt = q(1, H), q(1), q(B), -0.5, q(B, H), q(B, H)
        else:
            q = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
            fc_w, fc_b, ge, c, hp, hpt = q(1, H), q(1), q(B), float(torch.tensor(-1.3, dtype=F32)), q(B, H), q(B, H)
        ge_ = ge if ge_set else None
        dbl = lambda t: None if t is None else t.double()  # noqa: E731
        gx64, gxt64 = R.readout_seeds(N, gp, fc_w.double(), fc_b.double(), dbl(ge_), c, k, bool(mult_natoms))
        gW64, gb64 = R.fc_grad(hp.double(), hpt.double(), gp, fc_w.double(), fc_b.double(), dbl(ge_), c, k, bool(mult_natoms))
        gx, gxt = torch.full((N, H), SENTINEL, device=DEV), torch.full((N, H), SENTINEL, device=DEV)
        _run(lib.alignn_ff_readout_seed, dev(ge_), c, mult_natoms, wm, dev(gp), dev(fc_w), gx, gxt, B, N, H)
        gW, gb = torch.full((H,), SENTINEL, device=DEV), torch.full((1,), SENTINEL, device=DEV)
        _run(lib.alignn_ff_fc_grad, dev(ge_), c, mult_natoms, wm, dev(gp), dev(hp), dev(hpt), gW, gb, B, H)
        cnt = torch.tensor(counts, dtype=F64)
        gt = abs(c) * (cnt if mult_natoms else torch.ones(B, dtype=F64)) * 2.0 ** k
        mag_w = (gt[:, None] * hpt.double().abs()).sum(0) + ((ge.double().abs()[:, None] * hp.double().abs()).sum(0) if ge_set else 0)
        if exact:
            _exact(case, "gx", gx, gx64)
            _exact(case, "gxt", gxt, gxt64)
            _exact(case, "gb", gb.reshape(()), gb64)
            if not ge_set or abs(k) <= 8:
                _exact(case, "gW", gW, gW64)
            else:  # value terms of order 1 beside tangent terms of order 2^k: the sum rounds
                _within_roundoff(case, "gW", gW, gW64, mag_w, 2 * B + 3)
        else:
            _within_roundoff(case, "gx", gx, gx64, gx64.abs(), 4)
            _within_roundoff(case, "gxt", gxt, gxt64, gxt64.abs(), 6)
            _within_roundoff(case, "gb", gb.reshape(()), gb64, ge.double().abs().sum() if ge_set else torch.zeros(()), B + 1)
            _within_roundoff(case, "gW", gW, gW64, mag_w, 2 * B + 3)


def test_ff_readout_seed_refuses_a_width_that_is_no_multiple_of_four():
    lib = _lib.load()
    z, gp, wm = torch.full((4, 8), SENTINEL, device=DEV), dev(i32([0, 4])), torch.ones(1, device=DEV)
    for H in (6, 3, 0):
        assert lib.alignn_ff_readout_seed(None, 1.0, 0, ptr(wm), ptr(gp), ptr(z), ptr(z), ptr(z), 1, 4, H, stream()) == INVALID
    torch.cuda.synchronize()
    assert bool((z == SENTINEL).all())


@pytest.mark.parametrize("n", [4, 1028, 4096 * 256 * 4 + 4])  # the last: past the 4096-workgroup cap of both kernels
def test_add3_and_add_inplace(n):
    lib = _lib.load()
    g = _seed(f"add {n}")
    a, b, c = (torch.randint(-1000, 1001, (n,), generator=g).float() / 8 for _ in range(3))
    ad, bd, cd = dev(a), dev(b), dev(c)
    out = torch.full((n,), SENTINEL, device=DEV)
    _ok(lib.alignn_add3(ptr(ad), ptr(bd), ptr(cd), ptr(out), n, stream()))
    _exact(f"add3 n={n}", "out", out, a.double() + b.double() + c.double())
    _ok(lib.alignn_add_inplace(ptr(ad), ptr(bd), n, stream()))
    _exact(f"add_inplace n={n}", "a", ad, a.double() + b.double())
    assert torch.equal(host(bd), b)
    # any floats: each sum rounds once
    x, y, z = (torch.randn(n, generator=g) for _ in range(3))
    xd = dev(x)
    _run(lib.alignn_add3, xd, dev(y), dev(z), out, n)
    s = x.double() + y.double() + z.double()
    _within_roundoff(f"add3 n={n}", "out", out, s, x.double().abs() + y.double().abs() + z.double().abs(), 2, (x + y) + z)
    _run(lib.alignn_add_inplace, xd, dev(y), n)
    _within_roundoff(f"add_inplace n={n}", "a", xd, x.double() + y.double(), (x.double() + y.double()).abs(), 1, x + y)


def test_add_inplace_refuses_a_length_that_is_no_multiple_of_four():
    lib = _lib.load()
    a, b = torch.full((8,), SENTINEL, device=DEV), torch.ones(8, device=DEV)
    for n in (1, 6, 7):
        assert lib.alignn_add_inplace(ptr(a), ptr(b), n, stream()) == INVALID
    torch.cuda.synchronize()
    assert bool((a == SENTINEL).all())


# ----------------------------------------------------------------------------------------------------------------------
# composition: the normalisation tangent_geometry takes out is the one the seeds put back
# ----------------------------------------------------------------------------------------------------------------------
def test_second_order_geometry_chain_matches_one_float64_jvp():
    """pair_weights -> tangent_geometry -> (rbf_tangent of the lengths, bond_cosine_tangent -> rbf_tangent of the cosines), times
    the 2^k that readout_seed and fc_grad apply, against ONE float64 jvp of the restated featurisation along w"""
    lib = _lib.load()
    b = GraphBatch.from_raw(make_batch(3, 7, seed0=17), device=DEV)
    gg, lg = b.g, b.lg
    assert gg.seg_node is None
    vol = b.cell_volumes()
    assert len(set(host(vol).tolist())) == 3  # unequal cells
    N, E, B = gg.n_nodes, gg.n_edges, b.batch_size
    g = _seed("composition")
    gF, gS = torch.randn(N, 3, generator=g), torch.randn(B, 3, 3, generator=g) * 0.05
    kS = float(torch.tensor(R.STRESS_UNIT, dtype=F32))
    r = host(b.r)
    src, dst, gp, sp, e1, e2 = (host(t) for t in (gg.src, gg.dst, b.graph_ptr, gg.seg_ptr, lg.src, lg.dst))
    ce, ca = torch.linspace(0, 8, 80), torch.linspace(-1, 1, 40)
    ge_, ga_ = R.rbf_gamma(0, 8, 80), R.rbf_gamma(-1, 1, 40)
    ref = {}
    for dt in (F64, F32):
        w = R.pair_weights(gF.to(dt), gS.to(dt), r.to(dt), src, dst, R.edge_ptr_of(gp, sp), host(vol).to(dt), kS, True, N, E)
        feat = lambda q, dt=dt: R.featurisation(q, e1, e2, ce.to(dt), ge_, ca.to(dt), ga_)  # noqa: E731
        ref[dt] = (w,) + tuple(R.jvp_of(feat, (r.to(dt),), (w,)))
    w, wmax = torch.empty(E, 3, device=DEV), torch.zeros(1, device=DEV)
    _run(lib.alignn_ff_pair_weights, dev(gF), dev(gS), b.r, gg.src, gg.dst, b.graph_ptr, gg.seg_ptr, vol, kS, 1, B, E, w, wmax)
    d = ops.bond_length(b.r)
    rt, dt_ = torch.empty(E, 3, device=DEV), torch.empty(E, device=DEV)
    _ok(lib.alignn_ff_tangent_geometry(ptr(b.r), ptr(w), ptr(wmax), ptr(d), ptr(rt), ptr(dt_), E, stream()))
    te = ff2._rbf_dual(d, dt_, SimpleNamespace(centers=dev(ce), gamma=ge_)).t
    h, ht = ff2._cos_dual(b.r, rt, lg)
    ta = ff2._rbf_dual(h, ht, SimpleNamespace(centers=dev(ca), gamma=ga_)).t
    # the factor the seeds carry: one crystal of one atom, fc_w = 1, c = 1 -> gxt = 2^k; one crystal, hpt = 1 -> gW = 2^k
    one, gp1 = torch.ones(1, 4, device=DEV), dev(i32([0, 1]))
    gx, gxt, gW, gb = (torch.empty(1, 4, device=DEV) for _ in range(4))
    _ok(lib.alignn_ff_readout_seed(None, 1.0, 0, ptr(wmax), ptr(gp1), ptr(one), ptr(gx), ptr(gxt), 1, 1, 4, stream()))
    _ok(lib.alignn_ff_fc_grad(None, 1.0, 0, ptr(wmax), ptr(gp1), ptr(one), ptr(one), ptr(gW), ptr(gb), 1, 4, stream()))
    factor = float(gxt[0, 0])
    assert bool((gxt == factor).all()) and bool((gW == factor).all())
    assert factor == 2.0 ** R.pow2_exponent(float(ref[F64][0].abs().max())), (factor, float(ref[F64][0].abs().max()))
    case = "chain make_batch(3,7)"
    _parity(case, "w", w, ref[F64][0], ref[F32][0], B_GRAD)
    _parity(case, "edge rbf tan", te * factor, ref[F64][1], ref[F32][1], B_GRAD)
    _parity(case, "angle rbf tan", ta * factor, ref[F64][2], ref[F32][2], B_GRAD)
