"""csrc/gemm_f32.hip and csrc/gemm_x6.hip - the fp32 MFMA / element-wise products, the bf16x6 and f16x3 split products with every
fused epilogue, the weight images and the maxima - against the float64 restatements of tests/gemm_ref.py (checked on their own
by tests/test_gemm_ref.py), entry point by entry point through the raw C ABI.  The other tests of these kernels go through the
``ops`` wrappers on contiguous N(0,1) operands and measure max |err| / max |ref| over the whole tensor; here every operand is a
view with a leading dimension wider than its width, every output is NaN-filled inside a sentinel-filled wider buffer (the padding
must survive), every slab buffer is NaN-filled with three slabs more than the call may touch, and NO element is excluded.

Bounds (derived in tests/gemm_ref.py, none taken from what a kernel returns):
* every output element: |got - float64| <= accumulation_bound for the fp32 kernels, scheme bound + accumulation_bound for the
  split products (f16x3_scheme_bound_at with the maxima the kernel is handed; 2^-22 |A| |W|^T for bf16x6);
* on ``normal`` data also the max-norm bounds the older tests assert: 2e-6 NT / NN, 5e-6 fp32 TN, 2e-6 f16x3 TN;
* column-sum slabs (_stats, _gather with statistics): slab by slab against float64 sums of the kernel's OWN float32 output
  rows of that slab, within R 2^-24 sum |c| (sums) and R (2^-23 sum c^2 + 2^-149) (squares), R = rows per slab - which pins the
  slab-to-row map of every dispatch branch; slabs [0, row_tiles) finite, slab row_tiles anything, the three behind it untouched;
* _bnred sums: float32's silu' is not derivable, so 4x the float32 restatement on the identical operands (the kernel's own
  output, Xn, nstat) plus the floor B_BNRED = 2e-6, a decade above the worst error measured on ``normal`` data (1.9e-7,
  profiles/gemm_float64_parity.txt);
* weight images and maxima: bit for bit.

Row isolation: one NaN in A[M-1, 0] - the row the clamped out-of-range rows re-read - makes exactly row M-1 of C NaN, leaves the
bits of every other row, and makes exactly the slab that holds row M-1 NaN.

Shapes are the smallest at which each branch is live (BM 64 / 128, BN 256, BK 16; RM = 2 from 256 tiles of 128 rows with
K > 64; persistent from 1024 such tiles with N % 256 == 0 and K >= 80); the lists are at the parametrisations.

What reading the code settled (the suspects of this pass):
1. gemm_mfma_kernel's vector epilogue loads the bias as float4 and its predicate does not look at the bias pointer: a defect
   for a bias that is not 16-byte aligned (a misaligned vector load).  alignn_gemm_nt now sends such a call to the element-wise
   kernel (test_fp32_nt_misaligned_bias); alignn_hip.h says so.
2. alignn_gemm_nt_f16x3_gather2 did not check ldp >= N, ldbd2 >= N: rows of the tables would overlap and the last one be read
   past its end.  Now refused (test_refusals_x6_nt_family).
3. alignn_prepare_weights' records are read unchecked on the device.  ops.WeightPrep is the only builder (cmodel passes its
   table on); it already kept N % 16, K % 16, ldw % 4 and now also keeps out an empty weight, a base that is not 16-byte
   aligned and an image of more than 2^28 elements - such a list takes the per-weight route, whose wrappers check.
4. Maxima below 2^-113: f16_scale clamps to 2^127, the operand is scaled to less than 2^14 and the slices' resolution (2^-25
   absolute after scaling) coarsens by a factor of two per factor of two below - 2^-32 of the maximum at max|A| = 2^-120, still
   below float32's own 2^-24.  The inverse scale is then the subnormal 2^-127; the library is built with float32 denormals
   kept (code objects carry float_denorm_mode_32 = 3), and the two inverse scales are applied one after the other.  Documented
   at alignn_gemm_nt_f16x3 in alignn_hip.h and pinned by test_x6_nt_maximum_below_the_scale_clamp (max|A| in [2^-120, 2^-119):
   inside scheme + accumulation with the clamped scale); ``tiny`` (2^-100) is above the clamp and inside the bound as well.
5. launch_nt_p refuses ldc, ldadd, ldxn >= 2^20 (32-bit offsets inside a row tile), the one-tile kernels do not: documented in
   alignn_hip.h.  Not run: the refusal depends on an environment variable, and without it the call would write.
6. The row_tiles + 1 slab contract is in alignn_hip.h now and checked per dispatch branch here (_check_slabs): the one-tile
   kernels never touch the scratch slab, the persistent one writes zeros (or a strip's sums) there."""

import contextlib
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from alignn_amd import _lib  # noqa: E402
from alignn_amd._lib import ptr, stream  # noqa: E402
from tests import gemm_ref as ref  # noqa: E402
from tests.gate_parity import Report, err  # noqa: E402

DEV = "cuda"
TAG = "gemm-parity"
INVALID = 1  # hipErrorInvalidValue
NAN, SENTINEL, U = float("nan"), 7.0, ref.U
B_NT, B_TN32, B_TN16 = 2e-6, 5e-6, 2e-6  # inherited (tests/test_gpu_kernels.py, test_gpu_round2.py)
B_BNRED = 2e-6  # floor of the _bnred sums (module docstring)

d = lambda t: t.double()  # noqa: E731
cdiv = lambda a, b: (a + b - 1) // b  # noqa: E731


def _wide(t, extra):
    """t on the device as a view with leading dimension cols + extra (the padding holds the sentinel)"""
    rows, cols = t.shape
    buf = torch.full((max(rows, 1), cols + extra), SENTINEL, device=DEV, dtype=t.dtype)
    buf[:rows, :cols] = t.to(DEV)
    return buf[:rows, :cols]


def _out(rows, cols, before=4, after=8):
    """(buffer, view) of a NaN-filled [rows, cols] output inside a sentinel-filled wider buffer with two more rows"""
    buf = torch.full((rows + 2, before + cols + after), SENTINEL, device=DEV)
    buf[:rows, before:before + cols] = NAN
    return buf, buf[:rows, before:before + cols]


def _kept(rep, ent, buf, rows, cols, before=4):
    mask = torch.ones_like(buf, dtype=torch.bool)
    mask[:rows, before:before + cols] = False
    if not bool((buf[mask] == SENTINEL).all()):
        rep.failed.append((ent, "wrote outside its output"))


def _bits(t):
    return t.contiguous().view(torch.int32)


def _within(rep, ent, name, got, want64, bound):
    """every element: |got - want64| <= bound (recorded as the largest error / bound; an element off a zero bound, or a NaN,
    fails)"""
    if want64.numel() == 0:
        return
    e = (d(got) - want64).abs()
    ratio = torch.where(bound > 0, e / bound, torch.where(e == 0, torch.zeros_like(e), torch.full_like(e, float("inf"))))
    worst = float(ratio.max())
    rep.record(ent, name + "/bnd", worst, None, 1.0 + 1e-12)


def _maxnorm(rep, ent, name, got, want64, allowed):
    rep.record(ent, name, err(got, want64), None, allowed)


def _scalar(x):
    return x.abs().max().reshape(1).clone()


LIBC = ctypes.CDLL(None)


@contextlib.contextmanager
def _one_tile_kernels():
    """ALIGNN_AMD_X6_PERSIST=0 for the library's getenv (read per call), restored afterwards"""
    LIBC.setenv(b"ALIGNN_AMD_X6_PERSIST", b"0", 1)
    try:
        yield
    finally:
        LIBC.unsetenv(b"ALIGNN_AMD_X6_PERSIST")


# ---------------------------------------------------------------------------------------------------------------------------
# the x6 NT family
# ---------------------------------------------------------------------------------------------------------------------------

def _persistent(M, N, K):
    return K > 64 and K // 16 >= 3 and N % 256 == 0 and cdiv(M, 128) * (N // 256) >= 1024


def _slab_rows(M, N, K, persist):
    """rows per column-sum slab in each dispatch branch (alignn_hip.h at alignn_gemm_nt_f16x3)"""
    if persist and _persistent(M, N, K):
        return 64
    return 64 if (K <= 64 or cdiv(M, 128) * cdiv(N, 256) < 256) else 128


class X6:
    """one (M, N, K, distribution): operands as padded views, both weight images, the float64 product and the bounds - computed
    once and shared by every variant"""

    def __init__(self, M, N, K, data, pads):
        self.lib, self.M, self.N, self.K, self.data = _lib.load(), M, N, K, data
        a, w, bias, addend = ref.operands(M, N, K, data)
        pa, pw, padd, pxn, self.cpad = (4, 4, 4, 4, (4, 4)) if pads == "p4" else (8, 12, 16, 20, (8, 12))
        self.a, self.w, self.addend, self.bias = _wide(a, pa), _wide(w, pw), _wide(addend, padd), bias.to(DEV)
        self.a_amax, self.w_amax = _scalar(self.a), _scalar(self.w)
        lib, st = self.lib, stream()
        self.img16 = torch.empty(lib.alignn_split_f16x2_bytes(N, K), dtype=torch.uint8, device=DEV)
        self.img6 = torch.empty(lib.alignn_split_bf16x3_bytes(N, K), dtype=torch.uint8, device=DEV)
        assert lib.alignn_split_f16x2(ptr(self.w), self.w.stride(0), N, K, 0, ptr(self.w_amax), ptr(self.img16), st) == 0
        assert lib.alignn_split_bf16x3(ptr(self.w), self.w.stride(0), N, K, 0, ptr(self.img6), st) == 0
        self.prod = d(self.a) @ d(self.w).t() + d(self.bias)
        self.mag = ref.magnitude_product(self.a, self.w) + d(self.bias).abs()
        self.s16 = ref.f16x3_scheme_bound_at(self.a, self.w, float(self.a_amax), float(self.w_amax))
        self.s6 = ref.bf16x6_scheme_bound(self.a, self.w)
        # BatchNorm operands of the _bnred variants, node table and indices of the gather variants
        g = torch.Generator().manual_seed(M + N + K)
        scale = 2.0 ** -100 if data == "tiny" else 1.0
        xn = torch.randn(M, N, generator=g) * 2 + 0.5
        mean, var = d(xn).mean(0), d(xn).var(0, unbiased=False) + 1e-5
        gamma, beta = torch.randn(N, generator=g).double(), torch.randn(N, generator=g).double()
        self.xn = _wide(xn, pxn)
        self.nstat = torch.stack([mean, var.rsqrt(), gamma * var.rsqrt(), beta]).float().contiguous().to(DEV)
        self.nodes = 53
        self.P = {ld: _wide(torch.randn(self.nodes, ld * N, generator=g) * scale, 0) for ld in (4, 2)}
        src, dst = torch.randint(0, self.nodes, (M,), generator=g), torch.randint(0, self.nodes, (M,), generator=g)
        z = torch.zeros(M, dtype=torch.int64)
        self.index = {"sorted": (src.sort().values, dst), "first": (z, z), "last": (z + self.nodes - 1, z + self.nodes - 1)}
        self.index = {k: (s.int().to(DEV), t.int().to(DEV)) for k, (s, t) in self.index.items()}
        order = torch.randperm(self.nodes, generator=g)
        self.order, self.rank_of = order.to(DEV), torch.argsort(order).to(DEV)

    def acc(self, extra=None):
        return (self.K + 3) * U * (self.mag if extra is None else self.mag + extra)

    def base(self, f16=True):
        return [ptr(self.a), self.a.stride(0)] + ([ptr(self.a_amax), ptr(self.img16), ptr(self.w_amax)] if f16 else [ptr(self.img6)])

    def c_out(self):
        return _out(self.M, self.N, *self.cpad)

    def dims(self):
        return [self.M, self.N, self.K]

    def slabs(self, persist):
        R = _slab_rows(self.M, self.N, self.K, persist)
        T = self.lib.alignn_gemm_nt_x6_row_tiles(self.M, self.N, self.K)
        assert T == cdiv(self.M, R), ("alignn_gemm_nt_x6_row_tiles", T, R)
        return T, R, torch.full((T + 4, 2, self.N), NAN, device=DEV)


def _check_slabs(rep, ent, part, T):
    """slabs [0, T) finite, slab T anything, the three behind it untouched"""
    if not bool(torch.isfinite(part[:T]).all()):
        rep.failed.append((ent, "a promised slab was not written"))
    if not bool(torch.isnan(part[T + 1:]).all()):
        rep.failed.append((ent, "wrote behind the scratch slab"))


def _check_stats(rep, ent, part, C, T, R):
    _check_slabs(rep, ent, part, T)
    c = d(C)
    want = ref.stats_slabs(c, R)
    _within(rep, ent, "sum", part[:T, 0], want[:, 0], R * U * ref.stats_slabs(c.abs(), R)[:, 0])
    # (+ what a float32 square loses below the smallest subnormal, 2^-149 each: ``tiny`` rows square to 2^-200)
    _within(rep, ent, "sumsq", part[:T, 1], want[:, 1], R * 2 * U * want[:, 1] + R * 2.0 ** -149)


def _plain(p, rep, f16, full, tag=""):
    """alignn_gemm_nt_f16x3 / alignn_gemm_nt_x6 with (full) or without bias and addend"""
    lib, ent = p.lib, ("gemm_nt_f16x3" if f16 else "gemm_nt_x6") + (" +bias+addend" if full else "") + tag
    buf, C = p.c_out()
    fn = lib.alignn_gemm_nt_f16x3 if f16 else lib.alignn_gemm_nt_x6
    rc = fn(*p.base(f16), ptr(p.bias) if full else None, ptr(p.addend) if full else None, p.addend.stride(0) if full else 0, ptr(C),
            C.stride(0), *p.dims(), stream())
    torch.cuda.synchronize()
    assert rc == 0, (ent, rc)
    want = p.prod + d(p.addend) if full else p.prod - d(p.bias)
    scheme = p.s16 if f16 else p.s6
    _within(rep, ent, "C", C, want, scheme + p.acc(d(p.addend).abs() if full else None))
    if p.data == "normal":
        _maxnorm(rep, ent, "C", C, want, B_NT)
    if p.data == "zero_rows":  # nothing of a zero row's products may reach the output
        exact = (p.bias + p.addend) if full else torch.zeros_like(C)
        if not torch.equal(C[::4], exact[::4].expand_as(C[::4])):
            rep.failed.append((ent, "a zero row of A does not give bias + addend exactly"))
    _kept(rep, ent, buf, p.M, p.N, p.cpad[0])
    return C


def _stats(p, rep, persist, tag=""):
    ent = "gemm_nt_f16x3_stats" + tag
    T, R, part = p.slabs(persist)
    buf, C = p.c_out()
    rc = p.lib.alignn_gemm_nt_f16x3_stats(*p.base(), ptr(p.bias), ptr(C), C.stride(0), *p.dims(), ptr(part), stream())
    torch.cuda.synchronize()
    assert rc == 0, (ent, rc)
    _within(rep, ent, "C", C, p.prod, p.s16 + p.acc())
    if p.data == "normal":
        _maxnorm(rep, ent, "C", C, p.prod, B_NT)
    if p.data == "zero_rows" and not torch.equal(C[::4], p.bias.expand_as(C[::4])):
        rep.failed.append((ent, "a zero row of A does not give the bias exactly"))
    _check_stats(rep, ent, part, C, T, R)
    _kept(rep, ent, buf, p.M, p.N, p.cpad[0])
    return C, part


def _gather(p, rep, persist, pattern, ldp, with_stats, second_table, tag=""):
    """alignn_gemm_nt_f16x3_gather, or _gather2 on a segment-ordered copy of the Bd block with ldbd2 > N"""
    N = p.N
    ent = ("gemm_nt_f16x3_gather2" if second_table else "gemm_nt_f16x3_gather") + f" {pattern} ldp={ldp}N" + (" +stats" if with_stats else "") + tag
    T, R, part = p.slabs(persist)
    buf, C = p.c_out()
    P, (src, dst) = p.P[ldp], p.index[pattern]
    head = p.base() + [ptr(p.bias), ptr(C), C.stride(0)] + p.dims() + [ptr(P), P.stride(0), ptr(src)]
    if second_table:
        bd2 = _wide(P[p.order, N:2 * N], 8)
        rank = p.rank_of[dst.long()].int()
        rc = p.lib.alignn_gemm_nt_f16x3_gather2(*head, ptr(bd2), bd2.stride(0), ptr(rank), ptr(part) if with_stats else None, stream())
    else:
        rc = p.lib.alignn_gemm_nt_f16x3_gather(*head, ptr(dst), ptr(part) if with_stats else None, stream())
    torch.cuda.synchronize()
    assert rc == 0, (ent, rc)
    ga, gb = d(P[src.long(), :N]), d(P[dst.long(), N:2 * N])
    want = p.prod + ga + gb
    _within(rep, ent, "C", C, want, p.s16 + p.acc(ga.abs() + gb.abs()))
    if p.data == "normal":
        _maxnorm(rep, ent, "C", C, want, B_NT)
    if with_stats:
        _check_stats(rep, ent, part, C, T, R)
    elif not bool(torch.isnan(part).all()):
        rep.failed.append((ent, "no slab buffer was given"))
    _kept(rep, ent, buf, p.M, p.N, p.cpad[0])
    return C, part


def _bnred(p, rep, persist, with_addend, tag=""):
    ent = "gemm_nt_f16x3_bnred" + (" +addend" if with_addend else "") + tag
    T, R, part = p.slabs(persist)
    buf, C = p.c_out()
    rc = p.lib.alignn_gemm_nt_f16x3_bnred(*p.base(), ptr(p.bias), ptr(p.addend) if with_addend else None,
                                          p.addend.stride(0) if with_addend else 0, ptr(C), C.stride(0), *p.dims(), ptr(p.xn),
                                          p.xn.stride(0), ptr(p.nstat), ptr(part), stream())
    torch.cuda.synchronize()
    assert rc == 0, (ent, rc)
    want = p.prod + d(p.addend) if with_addend else p.prod
    _within(rep, ent, "C", C, want, p.s16 + p.acc(d(p.addend).abs() if with_addend else None))
    _check_slabs(rep, ent, part, T)
    Cc, xn = C.contiguous(), p.xn.contiguous()
    r64, r32 = ref.bnred_slabs(d(Cc), d(xn), d(p.nstat), R), ref.bnred_slabs(Cc, xn, p.nstat, R)
    for k, name in enumerate(("gz", "gzxhat")):
        rep.close(ent, name, part[:T, k], r64[:, k], r32[:, k], B_BNRED, floor=1e-60)
    _kept(rep, ent, buf, p.M, p.N, p.cpad[0])


def _row_isolation(p, rep, persist, clean_plain16, clean_plain6, clean_stats, tag=""):
    """one NaN in A[M-1, 0]: exactly row M-1 of C and exactly the slab that holds it"""
    M = p.M
    keep = p.a[M - 1, 0].clone()
    p.a[M - 1, 0] = NAN
    try:
        runs = []
        for f16, clean in ((True, clean_plain16), (False, clean_plain6)):
            buf, C = p.c_out()
            fn = p.lib.alignn_gemm_nt_f16x3 if f16 else p.lib.alignn_gemm_nt_x6
            assert fn(*p.base(f16), None, None, 0, ptr(C), C.stride(0), *p.dims(), stream()) == 0
            runs.append(("gemm_nt_f16x3" if f16 else "gemm_nt_x6", C, clean, None, None))
        T, R, part = p.slabs(persist)
        buf, C = p.c_out()
        assert p.lib.alignn_gemm_nt_f16x3_stats(*p.base(), ptr(p.bias), ptr(C), C.stride(0), *p.dims(), ptr(part), stream()) == 0
        runs.append(("gemm_nt_f16x3_stats", C, clean_stats[0], part, clean_stats[1]))
        torch.cuda.synchronize()
    finally:
        p.a[M - 1, 0] = keep
    for name, C, clean, part, clean_part in runs:
        if not (bool(torch.isnan(C[M - 1]).all()) and torch.equal(_bits(C[:M - 1]), _bits(clean[:M - 1]))):
            rep.failed.append((name + tag, "row isolation: a NaN in the last row of A"))
        if part is not None:
            last = (M - 1) // R
            others = torch.arange(T, device=DEV) != last
            if not (bool(torch.isnan(part[last]).all()) and torch.equal(_bits(part[:T][others]), _bits(clean_part[:T][others]))):
                rep.failed.append((name + tag, "row isolation: the slab of the last row"))


def _family(p, rep, persist, patterns, tag=""):
    """every entry point of the NT family on one problem"""
    c16 = _plain(p, rep, True, False, tag)
    c6 = _plain(p, rep, False, False, tag)
    _plain(p, rep, True, True, tag)
    _plain(p, rep, False, True, tag)
    st = _stats(p, rep, persist, tag)
    for i, pattern in enumerate(patterns):
        ldp = (4, 2)[i % 2]
        g1 = _gather(p, rep, persist, pattern, ldp, True, False, tag)
        g2 = _gather(p, rep, persist, pattern, ldp, True, True, tag)
        if not (torch.equal(_bits(g1[0]), _bits(g2[0])) and torch.equal(_bits(g1[1][:g1[1].shape[0] - 4]), _bits(g2[1][:g2[1].shape[0] - 4]))):
            rep.failed.append(("gemm_nt_f16x3_gather2" + tag, pattern, "not the bits of _gather on equal values"))
    _gather(p, rep, persist, patterns[0], 2, False, False, tag)
    _gather(p, rep, persist, patterns[0], 4, False, True, tag)
    _bnred(p, rep, persist, False, tag)
    _bnred(p, rep, persist, True, tag)
    _row_isolation(p, rep, persist, c16, c6, st, tag)


# RM = 1: every M, N and K of the issue's lists at least once, K = 16 (one k-step: fewer than the DMA ring holds) twice
SMALL = ((1, 128, 16), (63, 132, 32), (64, 256, 48), (65, 260, 64), (129, 1024, 80), (200, 260, 256), (65, 1024, 16))


@pytest.mark.parametrize("data", ref.DATA)
@pytest.mark.parametrize("M,N,K", SMALL)
def test_x6_nt_family_64_row_tiles(M, N, K, data):
    rep = Report(f"x6 nt ({M}, {N}, {K}) {data}", TAG)
    p = X6(M, N, K, data, "p4" if (M + K) % 2 else "mixed")
    assert _slab_rows(M, N, K, True) == 64
    _family(p, rep, True, ("sorted", "first", "last"))
    rep.finish()


# RM = 2: 256 tiles of 128 x 256 and K > 64; (16257, 260, 80) has a ragged second column tile (Npad = 512)
@pytest.mark.parametrize("data", ("normal", "row_blocks"))
@pytest.mark.parametrize("M,N,K", ((8065, 1024, 80), (8129, 1024, 256), (16257, 260, 80)))
def test_x6_nt_family_128_row_tiles(M, N, K, data):
    rep = Report(f"x6 nt ({M}, {N}, {K}) {data}", TAG)
    p = X6(M, N, K, data, "mixed" if K == 256 else "p4")
    assert _slab_rows(M, N, K, True) == 128 and not _persistent(M, N, K)
    _family(p, rep, True, ("sorted",))
    rep.finish()


# persistent: 1024 tiles with the last strip past the end / 1024 tiles / 1028 tiles (uneven tiles per workgroup) on four column
# tiles (tile / n_nt, tile % n_nt, no XCD map), two column tiles, one column tile (the XCD map, even and uneven chunks).  The
# variants with an addend take the one-tile kernel with strip slabs; all of them again with ALIGNN_AMD_X6_PERSIST=0.
@pytest.mark.parametrize("data", ("normal", "row_blocks"))
@pytest.mark.parametrize("M,N,K", ((32641, 1024, 80), (32705, 1024, 80), (32769, 1024, 96), (65409, 512, 80), (130945, 256, 80),
                                   (131329, 256, 80)))
def test_x6_nt_family_persistent(M, N, K, data):
    rep = Report(f"x6 nt ({M}, {N}, {K}) {data}", TAG)
    p = X6(M, N, K, data, "mixed" if N == 512 else "p4")
    assert _persistent(M, N, K)
    _family(p, rep, True, ("sorted",))
    with _one_tile_kernels():
        assert _slab_rows(M, N, K, False) == 128
        _family(p, rep, False, ("sorted",), " persist=0")
    rep.finish()


@pytest.mark.parametrize("M,N,K", ((65, 132, 32), (200, 260, 256)))
def test_x6_nt_maximum_below_the_scale_clamp(M, N, K):
    """suspect 4: max |A| in [2^-120, 2^-119) - f16_scale clamps to 2^127, the inverse scale is the subnormal 2^-127 and is applied
    on its own: the product still meets scheme + accumulation with the clamped scale in the scheme bound"""
    rep = Report(f"x6 nt ({M}, {N}, {K}) amax=2^-120", TAG)
    p = X6(M, N, K, "normal", "p4")
    shrink = 2.0 ** -120 / float(2.0 ** torch.floor(torch.log2(p.a_amax)))  # (a power of two: the operand keeps its bits)
    for t in (p.a, p.bias, p.addend):
        t *= shrink
    p.a_amax *= shrink
    assert 2.0 ** -120 <= float(p.a_amax) < 2.0 ** -119 and ref.f16_scale(float(p.a_amax)) == 2.0 ** 127
    p.prod, p.mag = d(p.a) @ d(p.w).t() + d(p.bias), ref.magnitude_product(p.a, p.w) + d(p.bias).abs()
    p.s16 = ref.f16x3_scheme_bound_at(p.a, p.w, float(p.a_amax), float(p.w_amax))
    p.data = "below the clamp"
    _plain(p, rep, True, False)
    _plain(p, rep, True, True)
    _stats(p, rep, True)
    rep.finish()


# ---------------------------------------------------------------------------------------------------------------------------
# fp32: alignn_gemm_nt, alignn_gemm_nn, alignn_gemm_nn_split, alignn_gemm_tn below the x6 gate
# ---------------------------------------------------------------------------------------------------------------------------

def _fp32_nt(rep, M, N, K, data, ldc_extra=(4, 8), bias_shift=0):
    lib = _lib.load()
    a, w, bias, addend = ref.operands(M, N, K, data)
    pa, pw, padd = (4, 4, 4) if (M + N + K) % 2 == 0 else (4, 8, 12)  # all + 4, or each operand padded differently
    a, w, addend = _wide(a, pa), _wide(w, pw), _wide(addend, padd)
    bias_buf = torch.full((N + 4,), SENTINEL, device=DEV)
    bias_buf[bias_shift:bias_shift + N] = bias.to(DEV)
    bias = bias_buf[bias_shift:bias_shift + N]
    prod, mag = d(a) @ d(w).t(), ref.magnitude_product(a, w)
    for with_bias, with_add in ((True, True), (False, False), (True, False)):
        ent = "gemm_nt" + (" +bias" if with_bias else "") + (" +addend" if with_add else "")
        buf, C = _out(M, N, *ldc_extra)
        rc = lib.alignn_gemm_nt(ptr(a), a.stride(0), ptr(w), w.stride(0), ptr(bias) if with_bias else None, ptr(addend) if with_add else None,
                                addend.stride(0) if with_add else 0, ptr(C), C.stride(0), M, N, K, stream())
        torch.cuda.synchronize()
        assert rc == 0, (ent, rc)
        want, m = prod, mag
        if with_bias:
            want, m = want + d(bias), m + d(bias).abs()
        if with_add:
            want, m = want + d(addend), m + d(addend).abs()
        _within(rep, ent, "C", C, want, (K + 3) * U * m)
        if data == "normal":
            _maxnorm(rep, ent, "C", C, want, B_NT)
        if data == "zero_rows":
            exact = torch.zeros_like(C) + (bias if with_bias else 0.0) + (addend if with_add else 0.0)
            if not torch.equal(C[::4], exact[::4]):
                rep.failed.append((ent, "a zero row of A does not give bias + addend exactly"))
        _kept(rep, ent, buf, M, N, ldc_extra[0])


# (5, 7, 6): N < 16 and K % 4 != 0, the element-wise kernel; (3, 5, 130) and (2, 8, 256): few outputs with K >= 128, a wave per
# output (not one output alone: its max-norm error is relative to a single, possibly cancelling, sum); (37, 18, 8), (129, 130, 40): MFMA with the scalar epilogue (N % 4 != 0); (65, 64, 36) / (300, 132, 92) / (1, 16, 4): one
# per tile configuration (128 x 64, 64 x 128, and one row)
FP32_NT = ((5, 7, 6), (3, 5, 130), (2, 8, 256), (37, 18, 8), (129, 130, 40), (65, 64, 36), (300, 132, 92), (1, 16, 4))


@pytest.mark.parametrize("data", ref.DATA)
@pytest.mark.parametrize("M,N,K", FP32_NT)
def test_fp32_nt(M, N, K, data):
    rep = Report(f"fp32 nt ({M}, {N}, {K}) {data}", TAG)
    _fp32_nt(rep, M, N, K, data)
    rep.finish()


@pytest.mark.parametrize("data", ("normal", "row_blocks"))
def test_fp32_nt_odd_ldc_takes_the_scalar_epilogue(data):
    rep = Report(f"fp32 nt (65, 64, 36) ldc=N+1 {data}", TAG)
    _fp32_nt(rep, 65, 64, 36, data, ldc_extra=(0, 1))
    rep.finish()


@pytest.mark.parametrize("data", ("normal", "row_blocks"))
def test_fp32_nt_128x256_tile_with_a_ragged_column_tile(data):
    rep = Report(f"fp32 nt (65409, 260, 20) {data}", TAG)
    _fp32_nt(rep, 65409, 260, 20, data)
    rep.finish()


@pytest.mark.parametrize("M,N,K", ((65, 64, 36), (300, 132, 92)))
def test_fp32_nt_misaligned_bias(M, N, K):
    """suspect 1: a bias that is not 16-byte aligned next to operands that all are"""
    rep = Report(f"fp32 nt ({M}, {N}, {K}) bias + 4 bytes", TAG)
    _fp32_nt(rep, M, N, K, "normal", bias_shift=1)
    rep.finish()


def test_fp32_nt_without_rows_writes_nothing():
    lib = _lib.load()
    a, w = _wide(torch.zeros(0, 36), 4), _wide(torch.ones(64, 36), 4)
    buf, C = _out(0, 64)
    before = buf.clone()
    assert lib.alignn_gemm_nt(ptr(a), a.stride(0), ptr(w), w.stride(0), None, None, 0, ptr(C), C.stride(0), 0, 64, 36, stream()) == 0
    torch.cuda.synchronize()
    assert torch.equal(buf, before)


# K (output columns) 12: element-wise; 20, 64: 128 x 64 tile; 68, 128: 128 x 128; 132, 260: 128 x 256
FP32_NN = ((1, 4, 12), (127, 36, 20), (129, 260, 64), (127, 4, 68), (129, 36, 128), (1, 260, 132), (129, 260, 260))


@pytest.mark.parametrize("data", ref.DATA)
@pytest.mark.parametrize("M,N,K", FP32_NN)
def test_fp32_nn(M, N, K, data):
    lib = _lib.load()
    rep = Report(f"fp32 nn ({M}, {N}, {K}) {data}", TAG)
    g, wt, _, addend = ref.operands(M, K, N, data)  # C[M, K] = g[M, N] w[N, K] = nt(g, w^T)
    pg, pw, padd = (4, 4, 4) if (M + N + K) % 2 == 0 else (4, 8, 12)
    g, w, addend = _wide(g, pg), _wide(wt.t().contiguous(), pw), _wide(addend, padd)
    prod, mag = d(g) @ d(w), d(g).abs() @ d(w).abs()
    for with_add in (False, True):
        ent = "gemm_nn" + (" +addend" if with_add else "")
        buf, C = _out(M, K)
        rc = lib.alignn_gemm_nn(ptr(g), g.stride(0), ptr(w), w.stride(0), ptr(addend) if with_add else None, addend.stride(0) if with_add else 0,
                                ptr(C), C.stride(0), M, N, K, stream())
        torch.cuda.synchronize()
        assert rc == 0, (ent, rc)
        want, m = (prod + d(addend), mag + d(addend).abs()) if with_add else (prod, mag)
        _within(rep, ent, "C", C, want, (N + 3) * U * m)
        if data == "normal":
            _maxnorm(rep, ent, "C", C, want, B_NT)
        _kept(rep, ent, buf, M, K)
    rep.finish()


@pytest.mark.parametrize("data", ("normal", "row_blocks", "cancelling"))
@pytest.mark.parametrize("M,N,K,slabs", ((65, 512, 132, 4), (777, 1024, 256, 8), (64, 2048, 260, 8)))
def test_fp32_nn_split(M, N, K, slabs, data):
    lib = _lib.load()
    rep = Report(f"fp32 nn_split ({M}, {N}, {K}) {data}", TAG)
    g, wt, _, addend = ref.operands(M, K, N, data)
    pg, pw, padd = (4, 4, 4) if (M + N + K) % 2 == 0 else (4, 8, 12)
    g, w, addend = _wide(g, pg), _wide(wt.t().contiguous(), pw), _wide(addend, padd)
    nbytes = lib.alignn_gemm_nn_split_workspace(M, N, K)
    assert nbytes == slabs * M * K * 4
    ws = torch.full((nbytes // 4 + 8,), SENTINEL, device=DEV)
    prod, mag = d(g) @ d(w), d(g).abs() @ d(w).abs()
    for with_add in (False, True):
        ent = "gemm_nn_split" + (" +addend" if with_add else "")
        buf, C = _out(M, K)
        rc = lib.alignn_gemm_nn_split(ptr(g), g.stride(0), ptr(w), w.stride(0), ptr(addend) if with_add else None,
                                      addend.stride(0) if with_add else 0, ptr(C), C.stride(0), M, N, K, ptr(ws), nbytes, stream())
        torch.cuda.synchronize()
        assert rc == 0, (ent, rc)
        want, m = (prod + d(addend), mag + d(addend).abs()) if with_add else (prod, mag)
        _within(rep, ent, "C", C, want, (N + 3) * U * m)
        if data == "normal":
            _maxnorm(rep, ent, "C", C, want, B_NT)
        _kept(rep, ent, buf, M, K)
        if not bool((ws[nbytes // 4:] == SENTINEL).all()):
            rep.failed.append((ent, "wrote behind its workspace"))
    rep.finish()


def _tn_operands(M, N, K, data):
    """g [M, N], x [M, K] of dW = g^T x; the distribution's rows are the rows of g^T"""
    gt, xt, _, _ = ref.operands(N, K, M, data)
    return gt.t().contiguous(), xt.t().contiguous()


# (1, 16, 16) one row; (31, 40, 64): 64 x 64 tile; (33, 64, 92): 128 x 128; (4097, 132, 64): 128 x 64, several slabs;
# (100, 1, 256): N % 4 != 0, the element-wise kernel
@pytest.mark.parametrize("data", ("normal", "row_blocks", "cancelling", "outlier"))
@pytest.mark.parametrize("M,N,K", ((1, 16, 16), (31, 40, 64), (33, 64, 92), (4097, 132, 64), (100, 1, 256), (0, 16, 16)))
def test_fp32_tn(M, N, K, data):
    lib = _lib.load()
    rep = Report(f"fp32 tn ({M}, {N}, {K}) {data}", TAG)
    g, x = _tn_operands(max(M, 1), N, K, data)
    g, x = _wide(g[:M], 4), _wide(x[:M], 4 if M % 2 else 8)
    nbytes = lib.alignn_gemm_tn_workspace(M, N, K)
    ws = torch.full((nbytes // 4 + 8,), SENTINEL, device=DEV)
    want, mag = d(g).t() @ d(x), d(g).abs().t() @ d(x).abs()
    for extra in (4, 1):  # lddw = K + 4, and K + 1: the scalar slab reduce
        ent = f"gemm_tn lddw=K+{extra}"
        buf, dW = _out(N, K, 0, extra)
        rc = lib.alignn_gemm_tn(ptr(g), g.stride(0), None, ptr(x), x.stride(0), None, ptr(dW), dW.stride(0), M, N, K, ptr(ws), nbytes, stream())
        torch.cuda.synchronize()
        assert rc == 0, (ent, rc)
        if M == 0:
            assert torch.equal(dW, torch.zeros_like(dW))
        _within(rep, ent, "dW", dW, want, (M + 3) * U * mag)
        if data == "normal" and M:
            _maxnorm(rep, ent, "dW", dW, want, B_TN32)
        _kept(rep, ent, buf, N, K, 0)
        if not bool((ws[nbytes // 4:] == SENTINEL).all()):
            rep.failed.append((ent, "wrote behind its workspace"))
    rep.finish()


# ---------------------------------------------------------------------------------------------------------------------------
# x6 TN
# ---------------------------------------------------------------------------------------------------------------------------

def _tn_x6_chunk(M, N, K):
    """reduction rows per slab (tn::tn_chunk): ceil(256 / tiles) slabs wanted, whole 16-row stages, at least 128 rows"""
    want = cdiv(256, (N // 256) * (K // 256))
    return max(cdiv(cdiv(M, want), 16) * 16, 128)


# (8200, 1024, 256): 57 slabs of 144 rows, the last one 136 rows - no multiple of 16.  ``small_maxima`` (gemm_ref.dw_operands: both
# maxima near 2^-62, the two operand scales multiply to 2^152): the product of the two inverse scales is 0 in float32, the kernel
# applies them one after the other there - the same bound form, for both entry points (the bf16x6 form has no scales)
X6_TN = tuple((M, N, K, data) for M, N, K in ((4096, 256, 256), (4113, 256, 512), (4113, 512, 256), (8200, 1024, 256))
              for data in ("normal", "row_blocks")) + ((4096, 256, 256, "small_maxima"),)


@pytest.mark.parametrize("M,N,K,data", X6_TN)
def test_x6_tn(M, N, K, data):
    lib = _lib.load()
    rep = Report(f"x6 tn ({M}, {N}, {K}) {data}", TAG)
    g, x = ref.dw_operands(M, data)[:2] if data == "small_maxima" else _tn_operands(M, N, K, data)
    g, x = _wide(g, 4), _wide(x, 4 if M % 2 else 12)
    g_amax, x_amax = _scalar(g), _scalar(x)
    chunk, splits = _tn_x6_chunk(M, N, K), lib.alignn_gemm_tn_x6_splits(M, N, K)
    assert splits == cdiv(M, chunk) and lib.alignn_gemm_tn_x6_supported(M, N, K) == 1
    if (M, N, K) == (8200, 1024, 256):
        assert (chunk, splits, M - (splits - 1) * chunk) == (144, 57, 136)
    nbytes = lib.alignn_gemm_tn_workspace(M, N, K)
    assert nbytes >= lib.alignn_gemm_tn_x6_workspace(M, N, K) == splits * N * K * 4
    ws = torch.full((nbytes // 4 + 8,), NAN, device=DEV)
    gt, xt = g.t(), x.t()
    want, mag = d(gt) @ d(x), d(gt).abs() @ d(x).abs()
    for f16 in (True, False):
        name = "f16x3" if f16 else "bf16x6"
        scheme = ref.f16x3_scheme_bound_at(gt, xt, float(g_amax), float(x_amax)) if f16 else 2.0 ** -22 * mag
        ent = f"gemm_tn {name}"
        buf, dW = _out(N, K, 4, 4)
        rc = lib.alignn_gemm_tn(ptr(g), g.stride(0), ptr(g_amax) if f16 else None, ptr(x), x.stride(0), ptr(x_amax) if f16 else None, ptr(dW),
                                dW.stride(0), M, N, K, ptr(ws), nbytes, stream())
        torch.cuda.synchronize()
        assert rc == 0, (ent, rc)
        _within(rep, ent, "dW", dW, want, scheme + (M + 3) * U * mag)
        if data == "normal" and f16:
            _maxnorm(rep, ent, "dW", dW, want, B_TN16)
        _kept(rep, ent, buf, N, K)
        # the slab partials on their own, slab by slab against the float64 product of that slab's rows
        ent = f"gemm_tn_x6_partials {name}"
        ws.fill_(NAN)
        rc = lib.alignn_gemm_tn_x6_partials(ptr(g), g.stride(0), ptr(g_amax) if f16 else None, ptr(x), x.stride(0), ptr(x_amax) if f16 else None,
                                            M, N, K, ptr(ws), splits * N * K * 4, stream())
        torch.cuda.synchronize()
        assert rc == 0, (ent, rc)
        part = ws[:splits * N * K].view(splits, N, K)
        if not bool(torch.isnan(ws[splits * N * K:]).all()):
            rep.failed.append((ent, "wrote behind its slabs"))
        for z in range(splits):
            rows = slice(z * chunk, min((z + 1) * chunk, M))
            gz, xz = gt[:, rows], xt[:, rows]
            mz = d(gz).abs() @ d(xz).abs().t()
            sz = ref.f16x3_scheme_bound_at(gz, xz, float(g_amax), float(x_amax)) if f16 else 2.0 ** -22 * mz
            _within(rep, ent, "slab", part[z], d(gz) @ d(xz).t(), sz + (chunk + 3) * U * mz)
    rep.finish()


# ---------------------------------------------------------------------------------------------------------------------------
# weight images and maxima
# ---------------------------------------------------------------------------------------------------------------------------

TAIL = 64  # sentinel bytes behind an image


def _image_buffer(nbytes):
    return torch.full((nbytes + TAIL,), 0xA5, dtype=torch.uint8, device=DEV)


def _image_equal(buf, nbytes, want):
    return want.numel() == nbytes and torch.equal(buf[:nbytes], want) and bool((buf[nbytes:] == 0xA5).all())


@pytest.mark.parametrize("data", ("normal", "tiny", "huge", "outlier"))
@pytest.mark.parametrize("N,K", ((16, 16), (80, 64), (260, 48), (1024, 80), (64, 1024), (256, 256)))
def test_weight_images_byte_for_byte(N, K, data):
    lib, st = _lib.load(), stream()
    w = ref.operands(N, 3, K, data)[0]  # (the [N, K] operand that carries the distribution)
    amax = _scalar(w.to(DEV))
    for transpose in (0, 1):
        stored = _wide(w.t().contiguous() if transpose else w, 4 if N % 2 else 12)
        n6, n16 = lib.alignn_split_bf16x3_bytes(N, K), lib.alignn_split_f16x2_bytes(N, K)
        b6, b16 = _image_buffer(n6), _image_buffer(n16)
        assert lib.alignn_split_bf16x3(ptr(stored), stored.stride(0), N, K, transpose, ptr(b6), st) == 0
        assert lib.alignn_split_f16x2(ptr(stored), stored.stride(0), N, K, transpose, ptr(amax), ptr(b16), st) == 0
        torch.cuda.synchronize()
        assert _image_equal(b6, n6, ref.image_bf16x3(stored, bool(transpose))), ("alignn_split_bf16x3", transpose)
        assert _image_equal(b16, n16, ref.image_f16x2(stored, float(amax), bool(transpose))), ("alignn_split_f16x2", transpose)
    if N % 16 == 0:
        stored = _wide(w, 8)
        n, nt_ = lib.alignn_split_f16x2_bytes(N, K), lib.alignn_split_f16x2_bytes(K, N)
        b, bt = _image_buffer(n), _image_buffer(nt_)
        assert lib.alignn_split_f16x2_both(ptr(stored), stored.stride(0), N, K, ptr(amax), ptr(b), ptr(bt), st) == 0
        torch.cuda.synchronize()
        assert _image_equal(b, n, ref.image_f16x2(stored, float(amax), False)), "alignn_split_f16x2_both: W"
        assert _image_equal(bt, nt_, ref.image_f16x2(stored, float(amax), True)), "alignn_split_f16x2_both: W^T"
    print(f"{TAG} images ({N}, {K}) {data:<28s} split_bf16x3 / split_f16x2 / split_f16x2_both  equal gemm_ref.image_*  (bit for bit)")


def test_prepare_weights_table():
    """seven records with different (N, K) and ldw: the maxima exactly, both images of each byte for byte, slots outside the table
    untouched"""
    lib, st = _lib.load(), stream()
    shapes = ((16, 64, 64), (64, 16, 20), (80, 256, 260), (256, 80, 84), (1024, 16, 16), (16, 1024, 1028), (256, 256, 264))
    n = len(shapes)
    slots = torch.full((n + 2,), 5.0, device=DEV)
    rec = np.zeros(n, dtype=np.dtype([("W", "<u8"), ("ldw", "<i8"), ("N", "<i4"), ("K", "<i4"), ("amax", "<u8"), ("out", "<u8"), ("outT", "<u8")]))
    assert rec.dtype.itemsize == 48
    keep = []
    for i, (N, K, ldw) in enumerate(shapes):
        w = _wide(ref.operands(3, N, K, "normal", seed=i)[1] * 2.0 ** (3 * i - 9), ldw - K)
        nb, nbt = lib.alignn_split_f16x2_bytes(N, K), lib.alignn_split_f16x2_bytes(K, N)
        b, bt = _image_buffer(nb), _image_buffer(nbt)
        keep.append((w, b, bt, nb, nbt))
        rec[i] = (ptr(w), ldw, N, K, slots[1:].data_ptr() + 4 * i, ptr(b), ptr(bt))
    desc = torch.from_numpy(rec.view(np.uint8).copy()).to(DEV)
    assert lib.alignn_prepare_weights(ptr(desc), n, ptr(slots[1:]), st) == 0
    torch.cuda.synchronize()
    assert float(slots[0]) == 5.0 and float(slots[n + 1]) == 5.0, "a slot outside the table changed"
    for i, (w, b, bt, nb, nbt) in enumerate(keep):
        assert float(slots[1 + i]) == float(w.abs().max()), ("amax", shapes[i])
        assert _image_equal(b, nb, ref.image_f16x2(w, float(slots[1 + i]), False)), ("image of W", shapes[i])
        assert _image_equal(bt, nbt, ref.image_f16x2(w, float(slots[1 + i]), True)), ("image of W^T", shapes[i])
    print(f"{TAG} prepare_weights {n} records: maxima exact, images equal gemm_ref.image_f16x2 (bit for bit)")


# rows F / 4 quads on 256 threads x 8 per workgroup: 6 quads (below one workgroup), 256 and 2048 (one workgroup exactly: one pass,
# eight passes), 2049 (two), 8 519 745 (above 4096 workgroups: the grid clamps and every thread strides)
@pytest.mark.parametrize("rows,F", ((3, 8), (64, 16), (512, 16), (683, 12), (131073, 260)))
def test_absmax(rows, F):
    lib, st = _lib.load(), stream()
    g = torch.Generator().manual_seed(rows)
    x = _wide(torch.randn(rows, F, generator=g), 4)
    x[rows - 1, F - 1] = -9.5  # the maximum is a negative element in the last quad
    slot = torch.full((3,), 5.0, device=DEV)
    assert lib.alignn_absmax(ptr(x), x.stride(0), rows, F, ptr(slot[1:]), st) == 0
    torch.cuda.synchronize()
    assert slot.tolist() == [5.0, 9.5, 5.0]  # (the padding holds 7.0: not read as data either)
    x[rows - 1, F - 1] = 1.0
    assert lib.alignn_absmax(ptr(x), x.stride(0), rows, F, ptr(slot[1:]), st) == 0
    torch.cuda.synchronize()
    assert float(slot[1]) == float(x.abs().max()) and float(slot[0]) == 5.0 and float(slot[2]) == 5.0
    # raise: keeps a larger slot, lifts a smaller one
    big = float(x.abs().max())
    for start, want in ((100.0, 100.0), (0.0, big), (0.5, big)):
        slot[1] = start
        assert lib.alignn_absmax_raise(ptr(x), x.stride(0), rows, F, ptr(slot[1:]), st) == 0
        torch.cuda.synchronize()
        assert slot.tolist() == [5.0, want, 5.0]
    # no rows: 0 / unchanged
    slot[1] = 3.0
    assert lib.alignn_absmax_raise(ptr(x), x.stride(0), 0, F, ptr(slot[1:]), st) == 0
    torch.cuda.synchronize()
    assert float(slot[1]) == 3.0
    assert lib.alignn_absmax(ptr(x), x.stride(0), 0, F, ptr(slot[1:]), st) == 0
    torch.cuda.synchronize()
    assert slot.tolist() == [5.0, 0.0, 5.0]
    # the contract for non-finite elements, as the code has it (fmaxf): a NaN is ignored, an infinity is taken
    x[0, 0] = NAN
    assert lib.alignn_absmax(ptr(x), x.stride(0), rows, F, ptr(slot[1:]), st) == 0
    torch.cuda.synchronize()
    x[0, 0] = 0.0
    assert float(slot[1]) == float(x.abs().max())
    x[rows // 2, 1] = float("-inf")
    assert lib.alignn_absmax(ptr(x), x.stride(0), rows, F, ptr(slot[1:]), st) == 0
    torch.cuda.synchronize()
    assert float(slot[1]) == float("inf")
    print(f"{TAG} absmax ({rows}, {F}) absmax / absmax_raise: exactly max |x|; NaN ignored, infinity taken")


# ---------------------------------------------------------------------------------------------------------------------------
# refusals: every argument check of the wrappers; hipErrorInvalidValue and no output byte changed
# ---------------------------------------------------------------------------------------------------------------------------

def _walk(fn, order, good, outputs, bad, expect_ok=True):
    """``good`` runs; each of ``bad`` (name, overrides) is refused and leaves every buffer of ``outputs`` as it was"""
    call = lambda **over: fn(*[dict(good, **over)[k] for k in order], stream())  # noqa: E731
    if expect_ok:
        assert call() == 0
        torch.cuda.synchronize()
    for name, over in bad:
        before = [o.clone() for o in outputs]
        rc = call(**over)
        torch.cuda.synchronize()
        assert rc == INVALID, (name, rc)
        for o, b in zip(outputs, before):
            assert torch.equal(_bits(o), _bits(b)), (name, "changed an output")


def test_refusals_fp32():
    lib = _lib.load()
    M, N, K = 65, 64, 36
    a, w, c = _wide(torch.randn(M, K), 4), _wide(torch.randn(N, K), 4), torch.full((M, N + 4), NAN, device=DEV)
    good = dict(A=ptr(a), lda=a.stride(0), W=ptr(w), ldw=w.stride(0), bias=None, addend=None, ldadd=0, C=ptr(c), ldc=c.stride(0), M=M, N=N, K=K)
    order = ("A", "lda", "W", "ldw", "bias", "addend", "ldadd", "C", "ldc", "M", "N", "K")
    bad = [("M < 0", dict(M=-1)), ("N = 0", dict(N=0)), ("N < 0", dict(N=-4)), ("K = 0", dict(K=0)), ("K < 0", dict(K=-4))]
    _walk(lib.alignn_gemm_nt, order, good, [c], bad)
    # nn: C[M, K] = G[M, N] W[N, K]
    g, w2, c2 = _wide(torch.randn(M, N), 4), _wide(torch.randn(N, K), 4), torch.full((M, K + 4), NAN, device=DEV)
    good = dict(G=ptr(g), ldg=g.stride(0), W=ptr(w2), ldw=w2.stride(0), addend=None, ldadd=0, C=ptr(c2), ldc=c2.stride(0), M=M, N=N, K=K)
    order = ("G", "ldg", "W", "ldw", "addend", "ldadd", "C", "ldc", "M", "N", "K")
    _walk(lib.alignn_gemm_nn, order, good, [c2], bad)
    # tn: dW[N, K] = G[M, N]^T A[M, K]
    nbytes = lib.alignn_gemm_tn_workspace(M, N, K)
    ws, dw = torch.full((nbytes // 4,), NAN, device=DEV), torch.full((N, K + 4), NAN, device=DEV)
    good = dict(G=ptr(g), ldg=g.stride(0), ga=None, A=ptr(a), lda=a.stride(0), aa=None, dW=ptr(dw), lddw=dw.stride(0), M=M, N=N, K=K, ws=ptr(ws),
                nbytes=nbytes)
    order = ("G", "ldg", "ga", "A", "lda", "aa", "dW", "lddw", "M", "N", "K", "ws", "nbytes")
    _walk(lib.alignn_gemm_tn, order, good, [dw, ws], bad + [("workspace too small", dict(nbytes=nbytes - 4)), ("no workspace", dict(ws=None))])


def test_refusals_nn_split():
    lib = _lib.load()
    M, N, K = 65, 512, 132
    g, w, addend = _wide(torch.randn(M, N), 4), _wide(torch.randn(N, K), 4), _wide(torch.randn(M, K), 4)
    c = torch.full((M, K + 4), NAN, device=DEV)
    nbytes = lib.alignn_gemm_nn_split_workspace(M, N, K)
    ws = torch.full((nbytes // 4 + 4,), NAN, device=DEV)
    assert lib.alignn_gemm_nn_split_workspace(M, 256, K) == 0 and lib.alignn_gemm_nn_split_workspace(M, N, 128) == 0
    good = dict(G=ptr(g), ldg=g.stride(0), W=ptr(w), ldw=w.stride(0), addend=ptr(addend), ldadd=addend.stride(0), C=ptr(c), ldc=c.stride(0), M=M, N=N,
                K=K, ws=ptr(ws), nbytes=nbytes)
    order = ("G", "ldg", "W", "ldw", "addend", "ldadd", "C", "ldc", "M", "N", "K", "ws", "nbytes")
    bad = [("one slab: N < 512", dict(N=256)), ("one slab: K <= 128", dict(K=128)), ("workspace too small", dict(nbytes=nbytes - 4)),
           ("no workspace", dict(ws=None)), ("misaligned workspace", dict(ws=ptr(ws) + 4)), ("ldg % 4", dict(ldg=g.stride(0) + 1)),
           ("ldw % 4", dict(ldw=w.stride(0) + 1)), ("ldc % 4", dict(ldc=c.stride(0) + 1)), ("ldadd % 4", dict(ldadd=addend.stride(0) + 1)),
           ("misaligned G", dict(G=ptr(g) + 4)), ("misaligned W", dict(W=ptr(w) + 4)), ("misaligned C", dict(C=ptr(c) + 4)),
           ("misaligned addend", dict(addend=ptr(addend) + 4))]
    _walk(lib.alignn_gemm_nn_split, order, good, [c, ws], bad)


def test_refusals_images_and_maxima():
    lib = _lib.load()
    N, K = 32, 32
    w = _wide(torch.randn(N, K), 4)
    amax = _scalar(w)
    out, out_t = _image_buffer(lib.alignn_split_bf16x3_bytes(N, K)), _image_buffer(lib.alignn_split_f16x2_bytes(K, N))
    shape = [("N = 0", dict(N=0)), ("N < 0", dict(N=-16)), ("K = 0", dict(K=0)), ("K % 16", dict(K=24)), ("no image", dict(out=None))]
    good = dict(W=ptr(w), ldw=w.stride(0), N=N, K=K, tr=0, amax=ptr(amax), out=ptr(out), out_t=ptr(out_t))
    _walk(lib.alignn_split_bf16x3, ("W", "ldw", "N", "K", "tr", "out"), good, [out], shape)
    _walk(lib.alignn_split_f16x2, ("W", "ldw", "N", "K", "tr", "amax", "out"), good, [out], shape + [("no maximum", dict(amax=None))])
    _walk(lib.alignn_split_f16x2_both, ("W", "ldw", "N", "K", "amax", "out", "out_t"), good, [out, out_t],
          shape + [("no maximum", dict(amax=None)), ("N % 16", dict(N=24)), ("no transposed image", dict(out_t=None))])
    slots = torch.full((4,), 5.0, device=DEV)
    desc = torch.zeros(48, dtype=torch.uint8, device=DEV)
    assert lib.alignn_prepare_weights(ptr(desc), 0, ptr(slots), stream()) == 0  # (an empty table: nothing to do)
    for name, args in (("no table", (None, 1, ptr(slots))), ("a negative count", (ptr(desc), -1, ptr(slots))), ("no slots", (ptr(desc), 1, None))):
        assert lib.alignn_prepare_weights(*args, stream()) == INVALID, name
    torch.cuda.synchronize()
    assert slots.tolist() == [5.0] * 4
    x = _wide(torch.randn(8, 8), 4)
    slot = torch.full((2,), 5.0, device=DEV)
    good = dict(X=ptr(x), ldx=x.stride(0), rows=8, F=8, amax=ptr(slot))
    bad = [("F = 0", dict(F=0)), ("F % 4", dict(F=6)), ("ldx % 4", dict(ldx=13)), ("rows < 0", dict(rows=-1)), ("no slot", dict(amax=None)),
           ("misaligned X", dict(X=ptr(x) + 4))]
    for fn in (lib.alignn_absmax, lib.alignn_absmax_raise):
        _walk(fn, ("X", "ldx", "rows", "F", "amax"), good, [slot], bad)


def test_refusals_x6_tn():
    lib = _lib.load()
    M, N, K = 4096, 256, 256
    g, x = _wide(torch.randn(M, N), 4), _wide(torch.randn(M, K), 4)
    ga, xa = _scalar(g), _scalar(x)
    nbytes = lib.alignn_gemm_tn_x6_workspace(M, N, K)
    ws = torch.full((nbytes // 4 + 4,), NAN, device=DEV)
    assert lib.alignn_gemm_tn_x6_supported(4095, N, K) == 0 and lib.alignn_gemm_tn_x6_supported(M, 260, K) == 0
    good = dict(G=ptr(g), ldg=g.stride(0), ga=ptr(ga), X=ptr(x), ldx=x.stride(0), xa=ptr(xa), M=M, N=N, K=K, ws=ptr(ws), nbytes=nbytes)
    order = ("G", "ldg", "ga", "X", "ldx", "xa", "M", "N", "K", "ws", "nbytes")
    bad = [("M < 4096", dict(M=4095)), ("N % 256", dict(N=128)), ("K % 256", dict(K=128)), ("ldg % 4", dict(ldg=g.stride(0) + 1)),
           ("ldx % 4", dict(ldx=x.stride(0) + 1)), ("misaligned G", dict(G=ptr(g) + 4)), ("misaligned X", dict(X=ptr(x) + 4)),
           ("misaligned workspace", dict(ws=ptr(ws) + 4)), ("workspace too small", dict(nbytes=nbytes - 4)), ("one maximum only", dict(ga=None)),
           ("the other maximum only", dict(xa=None))]
    _walk(lib.alignn_gemm_tn_x6_partials, order, good, [ws], bad)


def test_refusals_x6_nt_family():
    lib = _lib.load()
    M, N, K = 65, 132, 32
    p = X6(M, N, K, "normal", "p4")
    c = torch.full((M, N + 4), NAN, device=DEV)
    part = torch.full((6, 2, N), NAN, device=DEV)
    P, (src, dst) = p.P[2], p.index["sorted"]
    bd2 = _wide(P[:, N:2 * N], 8)
    good = dict(A=ptr(p.a), lda=p.a.stride(0), aa=ptr(p.a_amax), img=ptr(p.img16), img6=ptr(p.img6), wa=ptr(p.w_amax), bias=ptr(p.bias),
                addend=ptr(p.addend), ldadd=p.addend.stride(0), C=ptr(c), ldc=c.stride(0), M=M, N=N, K=K, P=ptr(P), ldp=P.stride(0), src=ptr(src),
                dst=ptr(dst), part=ptr(part), Bd2=ptr(bd2), ldbd2=bd2.stride(0), Xn=ptr(p.xn), ldxn=p.xn.stride(0), nstat=ptr(p.nstat))
    assert lib.alignn_gemm_nt_x6_supported(M, N, K) == 1
    shape = [("M = 0", dict(M=0)), ("M < 0", dict(M=-1)), ("N < 128", dict(N=124)), ("N % 4", dict(N=130)), ("K % 16", dict(K=24)), ("K = 0", dict(K=0))]
    core = [("lda % 4", dict(lda=p.a.stride(0) + 1)), ("ldc % 4", dict(ldc=c.stride(0) + 1)), ("misaligned A", dict(A=ptr(p.a) + 4)),
            ("misaligned C", dict(C=ptr(c) + 4)), ("misaligned bias", dict(bias=ptr(p.bias) + 4))]
    img = [("misaligned image", dict(img=ptr(p.img16) + 4))]
    add = [("ldadd % 4", dict(ldadd=p.addend.stride(0) + 1)), ("misaligned addend", dict(addend=ptr(p.addend) + 4))]
    amax = [("no max |A|", dict(aa=None)), ("no max |W|", dict(wa=None))]
    _walk(lib.alignn_gemm_nt_x6, ("A", "lda", "img6", "bias", "addend", "ldadd", "C", "ldc", "M", "N", "K"), good, [c],
          shape + core + add + [("misaligned image", dict(img6=ptr(p.img6) + 4))])
    _walk(lib.alignn_gemm_nt_f16x3, ("A", "lda", "aa", "img", "wa", "bias", "addend", "ldadd", "C", "ldc", "M", "N", "K"), good, [c],
          shape + core + add + img + amax)
    _walk(lib.alignn_gemm_nt_f16x3_stats, ("A", "lda", "aa", "img", "wa", "bias", "C", "ldc", "M", "N", "K", "part"), good, [c, part],
          shape + core + img + amax + [("no slabs", dict(part=None)), ("misaligned slabs", dict(part=ptr(part) + 4))])
    tables = [("no P", dict(P=None)), ("no src", dict(src=None)), ("ldp % 4", dict(ldp=P.stride(0) + 1)), ("misaligned P", dict(P=ptr(P) + 4)),
              ("misaligned slabs", dict(part=ptr(part) + 4))]
    _walk(lib.alignn_gemm_nt_f16x3_gather, ("A", "lda", "aa", "img", "wa", "bias", "C", "ldc", "M", "N", "K", "P", "ldp", "src", "dst", "part"), good,
          [c, part], shape + core + img + amax + tables + [("no dst", dict(dst=None)), ("ldp < 2 N", dict(ldp=2 * N - 4))])
    _walk(lib.alignn_gemm_nt_f16x3_gather2,
          ("A", "lda", "aa", "img", "wa", "bias", "C", "ldc", "M", "N", "K", "P", "ldp", "src", "Bd2", "ldbd2", "dst", "part"), good, [c, part],
          shape + core + img + amax + tables + [("no rank", dict(dst=None)), ("no Bd2", dict(Bd2=None)), ("ldbd2 % 4", dict(ldbd2=bd2.stride(0) + 1)),
                                                ("misaligned Bd2", dict(Bd2=ptr(bd2) + 4)), ("ldp < N", dict(ldp=N - 4)),
                                                ("ldbd2 < N", dict(ldbd2=N - 4))])
    _walk(lib.alignn_gemm_nt_f16x3_bnred,
          ("A", "lda", "aa", "img", "wa", "bias", "addend", "ldadd", "C", "ldc", "M", "N", "K", "Xn", "ldxn", "nstat", "part"), good, [c, part],
          shape + core + add + img + amax + [("no Xn", dict(Xn=None)), ("no nstat", dict(nstat=None)), ("no slabs", dict(part=None)),
                                             ("ldxn % 4", dict(ldxn=p.xn.stride(0) + 1)), ("misaligned Xn", dict(Xn=ptr(p.xn) + 4)),
                                             ("misaligned nstat", dict(nstat=ptr(p.nstat) + 4)), ("misaligned slabs", dict(part=ptr(part) + 4))])
