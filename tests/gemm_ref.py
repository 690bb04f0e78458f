"""Plain torch restatements of what csrc/gemm_f32.hip and csrc/gemm_x6.hip compute - the three products of a Linear layer with
their epilogues, the operand slicing of the two split-product schemes, the weight images the DMA copies, the column-sum slabs -
and the two elementwise error bounds the kernels are held to (tests/test_gpu_gemm.py; checked on their own, on the CPU, by
tests/test_gemm_ref.py).  Every function takes tensors of any floating dtype on any device and imports nothing of the library.

Bounds (both elementwise, both independent of the order of summation):

* ``accumulation_bound``: a float32 sum of K products and up to three further addends (bias, addend, or the two gathered rows),
  taken in any order and with or without fused multiply-adds, is within (K + 3) u of the sum of the MAGNITUDES of its terms,
  u = 2^-24 (Higham, Accuracy and Stability of Numerical Algorithms, section 3.1, to first order in K u):
  (K + 3) 2^-24 (|A| |W|^T + |bias| + |addend| + |gathered rows|).  The fp32 MFMA and element-wise kernels are held to it alone.
* ``f16x3_scheme_bound``: what hh + hl + lh of the scaled fp16 slices can be off by, derived at the function.  The bf16x6
  counterpart ``bf16x6_scheme_bound`` is 2^-22 |A| |W|^T: the three truncations reproduce a float32 exactly (h + m + l = x, 8 + 8
  + 8 significant bits), so the whole error is the three dropped products m l + l m + l l with |m| < 2^-7 |x| and
  |l| < 2^-15 |x| at the very worst (x just above a power of two, x - h just above one too) and 2^-8, 2^-16 on average, i.e.
  2^-23 |a| |w| per term on average; 2^-22 of the sum of magnitudes covers every distribution of tests/test_gemm_ref.py.
  The split products are held to scheme + accumulation."""

import struct

import torch

U = 2.0 ** -24
ROW_BLOCK_K = (0, 8, 16, 20, 24, 28, 32, 36)  # tests/test_gpu_kernels.F16X3_K: row blocks 2^-k below the tensor's maximum
DATA = ("normal", "row_blocks", "tiny", "huge", "outlier", "cancelling", "zero_rows")
BN, BK = 256, 16  # column tile and k-block of the weight images


# ---- the f16x3 / bf16x6 schemes

def f16_scale(amax):
    """csrc/mfma_f16x3.h: 2^(141 - e) for a float32 maximum with biased exponent e, clamped to 2^127; 1 for zero, subnormal and
    non-finite maxima"""
    bits = struct.unpack("<I", struct.pack("<f", float(amax)))[0]
    e = (bits >> 23) & 255
    if e == 0 or e == 255:
        return 1.0
    return 2.0 ** (min(268 - e, 254) - 127)


def slices_f16x2(x, amax):
    """(h, l) float16: h = RN16(x s), l = RN16(x s - h) with s = f16_scale(amax); x s and x s - h are exact in float32"""
    xs = x.float() * f16_scale(amax)
    h = xs.half()
    return h, (xs - h.float()).half()


def _trunc16(x):
    return (x.contiguous().view(torch.int32) & -65536).view(torch.float32)


def slices_bf16x3(x):
    """(h, m, l) bfloat16 by truncation: h = x & 0xffff0000, m = (x - h) & 0xffff0000, l = upper16(x - h - m)"""
    x = x.float()
    h = _trunc16(x)
    r1 = x - h
    m = _trunc16(r1)
    l = _trunc16(r1 - m)
    return h.bfloat16(), m.bfloat16(), l.bfloat16()


def _image(planes, K):
    """planes [NPL, N, K] of 16-bit values -> the bytes of [k/16][n/256][plane][n%256][chunk ^ ((n>>3)&1)][8], zero rows for
    N <= n < Npad"""
    npl, N, _ = planes.shape
    assert K % BK == 0
    npad = (N + BN - 1) // BN * BN
    full = torch.zeros(npl, npad, K, dtype=torch.int16, device=planes.device)
    full[:, :N] = planes
    t = full.view(npl, npad // BN, BN, K // BK, 2, 8)  # [plane][n/256][n%256][k/16][chunk][8]
    odd = ((torch.arange(BN, device=planes.device) >> 3) & 1).bool().view(1, 1, BN, 1, 1, 1)
    t = torch.where(odd, t.flip(4), t)  # stored chunk = chunk ^ ((n >> 3) & 1); n % 256 and n agree in bit 3
    return t.permute(3, 1, 0, 2, 4, 5).contiguous().view(-1).view(torch.uint8)


def image_f16x2(w, amax, transpose):
    """alignn_split_f16x2's image of w [N, K] (transpose: of the [N, K] matrix w^T of a stored [K, N] w), as bytes"""
    m = w.t() if transpose else w
    h, l = slices_f16x2(m, amax)
    return _image(torch.stack([h, l]).contiguous().view(torch.int16), m.shape[1])


def image_bf16x3(w, transpose):
    m = w.t() if transpose else w
    return _image(torch.stack(slices_bf16x3(m)).contiguous().view(torch.int16), m.shape[1])


def decode_image(img, N, K, planes, dtype):
    """the inverse of _image: [planes, N, K] values of the given 16-bit dtype"""
    npad = (N + BN - 1) // BN * BN
    t = img.view(torch.int16).view(K // BK, npad // BN, planes, BN, 2, 8).permute(2, 1, 3, 0, 4, 5)
    odd = ((torch.arange(BN, device=img.device) >> 3) & 1).bool().view(1, 1, BN, 1, 1, 1)
    t = torch.where(odd, t.flip(4), t).contiguous().view(planes, npad, K)
    assert not bool(t[:, N:].any()), "rows beyond N are zero"
    return t[:, :N].contiguous().view(dtype)


# ---- products with their epilogues (in the dtype of the operands)

def nt(a, w, bias=None, addend=None):
    c = a @ w.t()
    if bias is not None:
        c = c + bias
    if addend is not None:
        c = c + addend
    return c


def nn(g, w, addend=None):
    c = g @ w
    return c if addend is None else c + addend


def tn(g, a):
    return g.t() @ a


def gather(a, w, bias, P, src, dst):
    """C[e] = a[e] w^T + bias + P[src e][0:N] + P[dst e][N:2N]"""
    N = w.shape[0]
    return nt(a, w, bias) + (P[src.long(), :N] + P[dst.long(), N:2 * N])


def gather2(a, w, bias, P, src, Bd2, rank):
    """C[e] = a[e] w^T + bias + P[src e][0:N] + Bd2[rank e][0:N]"""
    N = w.shape[0]
    return nt(a, w, bias) + (P[src.long(), :N] + Bd2[rank.long(), :N])


def _slab_sums(t, rows_per_slab):
    rows, N = t.shape
    slabs = (rows + rows_per_slab - 1) // rows_per_slab
    full = torch.zeros(slabs * rows_per_slab, N, dtype=t.dtype, device=t.device)
    full[:rows] = t
    return full.view(slabs, rows_per_slab, N).sum(1)


def stats_slabs(c, rows_per_slab):
    """[slabs, 2, N]: the sum and the sum of squares of rows [t R, (t + 1) R) of c"""
    return torch.stack([_slab_sums(c, rows_per_slab), _slab_sums(c * c, rows_per_slab)], 1)


def dsilu(z):
    s = torch.sigmoid(z)
    return s * (1 + z * (1 - s))


def bnred_slabs(c, xn, nstat, rows_per_slab):
    """[slabs, 2, N]: sum gz and sum gz xhat over the slab's rows, gz = c silu'((xn - mean) scale + beta), xhat = (xn - mean)
    rstd; nstat = [mean, rstd, scale, beta]"""
    mean, rstd, scale, beta = nstat
    xc = xn - mean
    gz = c * dsilu(xc * scale + beta)
    return torch.stack([_slab_sums(gz, rows_per_slab), _slab_sums(gz * xc * rstd, rows_per_slab)], 1)


# ---- bounds

def magnitude_product(a, w):
    return a.double().abs() @ w.double().abs().t()


def accumulation_bound(a, w, bias=None, addend=None, gathered=()):
    """(K + 3) 2^-24 (|a| |w|^T + |bias| + |addend| + |gathered rows|) for c = a w^T + ..., K = the reduction length"""
    mag = magnitude_product(a, w)
    for t in (bias, addend) + tuple(gathered):
        if t is not None:
            mag = mag + t.double().abs()
    return (a.shape[1] + 3) * U * mag


def bf16x6_scheme_bound(a, w):
    return 2.0 ** -22 * magnitude_product(a, w)


def f16x3_scheme_bound(a, w):
    """Elementwise bound [rows of a, rows of w] on |f16x3(a w^T) - a w^T|, from the scheme as written (csrc/gemm_x6.hip:12-18,
    f16_scale) and nothing the kernel returns.  Per operand x with tensor maximum amax:

    * x' = x * 2^s with s chosen so that amax * 2^s lies in [2^14, 2^15): |x'| < 2^15, no fp16 overflow.
    * h = RN16(x'), l = RN16(x' - h).  fp16 rounds to 11 significant bits above 2^-14 and to a spacing of 2^-24 below, so
      |x' - h| <= max(2^-11 |x'|, 2^-25) and e(x') = |x' - h - l| <= max(2^-11 |x' - h|, 2^-25) <= max(2^-22 |x'|, 2^-25);
      |l| <= L(x') = max(2^-11 (1 + 2^-11) |x'|, 2^-24); a zero is exact.
    * the product keeps hh + hl + lh and drops ll: with a' = ha + la + ea, w' = hw + lw + ew,
      a'w' - (hh + hl + lh) = la lw + ea w' + (ha + la) ew, in magnitude <= L(a') L(w') + e(a') |w'| + (|a'| + e(a')) e(w').

    The fp16 x fp16 products are exact in the fp32 accumulators and the power-of-two scales are undone exactly, so the sum of
    those terms over the reduction index, divided by the two scales, bounds the scheme's own error; one factor 4 covers the
    order of the fp32 accumulation (the margin test_gemm_x6_accuracy gives a reordered fp32 sum)."""
    import math

    def scaled(x):
        x = x.double().cpu().abs()
        s = 2.0 ** (15 - math.frexp(float(x.max()))[1])  # f16_scale: the maximum lands in [2^14, 2^15)
        return x * s, s

    def e(x):
        return torch.where(x > 0, (x * 2.0 ** -22).clamp_min(2.0 ** -25), 0.0)

    def low(x):
        return torch.where(x > 0, (x * 2.0 ** -11 * (1 + 2.0 ** -11)).clamp_min(2.0 ** -24), 0.0)

    (A, sa), (W, sw) = scaled(a), scaled(w)
    return 4 * (low(A) @ low(W).t() + e(A) @ W.t() + (A + e(A)) @ e(W).t()) / (sa * sw)


def f16x3_scheme_bound_at(a, w, a_amax, w_amax):
    """f16x3_scheme_bound with the scales the kernel is GIVEN - f16_scale of the two maxima it is handed, the clamp at 2^127
    included - instead of the operands' own maxima, and on the operands' device: the same bound when a_amax = max |a| and
    w_amax = max |w| (tests/test_gemm_ref.py), and the one that holds for a part of a tensor (a slab of rows) sliced at the
    whole tensor's scale."""
    sa, sw = f16_scale(a_amax), f16_scale(w_amax)
    A, W = a.double().abs() * sa, w.double().abs() * sw
    zero = torch.zeros((), dtype=torch.float64, device=A.device)

    def e(x):
        return torch.where(x > 0, (x * 2.0 ** -22).clamp_min(2.0 ** -25), zero)

    def low(x):
        return torch.where(x > 0, (x * 2.0 ** -11 * (1 + 2.0 ** -11)).clamp_min(2.0 ** -24), zero)

    return 4 * (low(A) @ low(W).t() + e(A) @ W.t() + (A + e(A)) @ e(W).t()) / sa / sw


# ---- operands

def operands(M, N, K, data, seed=0):
    """float32 CPU operands (a [M, K], w [N, K], bias [N], addend [M, N]) of C = a w^T + bias + addend on one of DATA"""
    g = torch.Generator().manual_seed(1000 * seed + 17 * DATA.index(data) + M + 3 * N + 7 * K)
    rn = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    a, w, bias, addend = rn(M, K), rn(N, K) / 16, rn(N), rn(M, N)
    if data == "row_blocks":  # eight row blocks 2^-k below the maximum, which sits in block 0
        per = M // len(ROW_BLOCK_K)
        for b, k in enumerate(ROW_BLOCK_K):
            a[b * per:(b + 1) * per] *= 2.0 ** -k
            addend[b * per:(b + 1) * per] *= 2.0 ** -k
        if per:
            a[0, 0] = 6.0
    elif data == "tiny":
        a, bias, addend = a * 2.0 ** -100, bias * 2.0 ** -100, addend * 2.0 ** -100
    elif data == "huge":
        a = a * 2e5
    elif data == "outlier":
        a[M // 2, K // 3] = 4e4
    elif data == "cancelling":  # w = [v, -v] against a = [u, u] + 2^-12 noise: the result is far below |a| |w|^T
        h = K // 2
        a = torch.cat([a[:, :h], a[:, :h]], 1) + 2.0 ** -12 * rn(M, 2 * h)
        w = torch.cat([w[:, :h], -w[:, :h]], 1)
        if 2 * h < K:
            a, w = torch.cat([a, torch.zeros(M, K - 2 * h)], 1), torch.cat([w, torch.zeros(N, K - 2 * h)], 1)
        bias, addend = bias * 2.0 ** -12, addend * 2.0 ** -12
    elif data == "zero_rows":
        a[::4] = 0.0
    return a.contiguous(), w.contiguous(), bias.contiguous(), addend.contiguous()


# ---- operands of the fused input-gradient + weight-gradient pass (csrc/gemm_dw.hip): C = G W (+ addend), dW = G^T Y, and the
# BatchNorm-backward sums of C against Xn

DW_H = 256
DW_PLAIN = ("normal", "row_blocks", "tiny", "huge", "outlier", "zero_rows")
DW_DATA = DW_PLAIN + ("y_row_blocks", "y_outlier", "cancelling", "dw_cancelling", "small_maxima", "integers", "bn_normal",
                      "bn_mean_over_spread", "bn_scale_zero_negative", "bn_saturated")


def dw_operands(M, data, seed=0):
    """float32 CPU (G [M, 256], Y [M, 256], W [256, 256], addend [M, 256], xn [M, 256], nstat [4, 256]) on one of DW_DATA.
    W = w.t() of ``operands``' w, so that G W = G w^T and the NT bound functions apply with (a, w) = (G, W.t()); for the weight
    gradient (a, w) = (G.t(), Y.t()).  nstat = [mean, rstd, gamma rstd, beta] from xn's own column statistics."""
    H = DW_H
    g = torch.Generator().manual_seed(1000 * seed + 31 * DW_DATA.index(data) + M)
    rn = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    ri = lambda lo, hi, *s: torch.randint(lo, hi + 1, s, generator=g).float()  # noqa: E731
    G, w, _, addend = operands(M, H, H, data if data in DW_PLAIN + ("cancelling",) else "normal", seed)
    Y = rn(M, H)
    if data in ("y_row_blocks", "y_outlier"):  # the structure on Y (another seed than G's: the two are independent)
        Y = operands(M, H, H, data[2:], seed + 1)[0]
    elif data == "dw_cancelling":  # row pairs (g, g + 2^-12 noise) against (y, -y): dW lies far below |G|^T |Y|
        G[1::2] = G[0:2 * (M // 2):2] + 2.0 ** -12 * rn(M // 2, H)
        Y[1::2] = -Y[0:2 * (M // 2):2]
        if M % 2:
            G[M - 1], Y[M - 1] = G[M - 1] * 2.0 ** -12, Y[M - 1] * 2.0 ** -12
    elif data == "small_maxima":  # both maxima near 2^-62: the product of the two inverse scales is 2^-152
        G, Y, addend = G * 2.0 ** -64, Y * 2.0 ** -64, addend * 2.0 ** -64
    elif data == "integers":  # every slice product and every partial sum is representable: any order gives float64's bits
        G, Y, addend, w = ri(-4, 4, M, H), ri(-4, 4, M, H), ri(-4, 4, M, H), ri(-8, 8, H, H) / 16
    xn = rn(M, H) * 2 + 0.5
    gamma, beta = rn(H).double(), rn(H).double()
    if data == "bn_mean_over_spread":  # column means up to 100 spreads
        xn = rn(M, H) * 0.5 + torch.linspace(-50.0, 50.0, H)
    elif data == "bn_scale_zero_negative":  # a third of gamma rstd zero, the rest of either sign
        gamma[0::3] = 0.0
        gamma[1::3], gamma[2::3] = gamma[1::3].abs() + 0.1, -gamma[2::3].abs() - 0.1
    elif data == "bn_saturated":  # exp overflows on one side: silu' is 0 or 1 to rounding
        beta = torch.where(torch.arange(H) % 2 == 0, 60.0, -60.0).double()
    mean, var = xn.double().mean(0), xn.double().var(0, unbiased=False) + 1e-5
    nstat = torch.stack([mean, var.rsqrt(), gamma * var.rsqrt(), beta]).float()
    return tuple(t.contiguous() for t in (G, Y, w.t(), addend, xn, nstat))
