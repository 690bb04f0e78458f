"""tests/gemm_ref.py checked on its own, on the CPU: the restatements against torch's own Linear and autograd in float64, the two
slicing schemes emulated from the slices (exact slice products in float64) against the bounds derived for them, the weight
images decoded back to the values they hold, and the slab helpers against whole-tensor sums.  What tests/test_gpu_gemm.py holds
the kernels to is therefore not taken from the kernels."""

import pytest
import torch
import torch.nn.functional as F

from tests import gemm_ref as ref

SHAPES = ((65, 132, 80), (200, 260, 256), (8, 16, 16), (129, 128, 48))
d = lambda t: t.double()  # noqa: E731


def test_f16_scale_is_the_header_function():
    assert ref.f16_scale(0.0) == 1.0 and ref.f16_scale(float("inf")) == 1.0 and ref.f16_scale(float("nan")) == 1.0
    assert ref.f16_scale(2.0 ** -127) == 1.0  # subnormal
    assert ref.f16_scale(1.0) == 2.0 ** 14 and ref.f16_scale(1.999) == 2.0 ** 14 and ref.f16_scale(2.0) == 2.0 ** 13
    assert ref.f16_scale(2.0 ** -113) == 2.0 ** 127 and ref.f16_scale(2.0 ** -112) == 2.0 ** 126
    assert ref.f16_scale(2.0 ** -120) == 2.0 ** 127 and ref.f16_scale(2.0 ** -126) == 2.0 ** 127  # the clamp
    assert ref.f16_scale(3e38) == 2.0 ** -113
    for amax in (1e-30, 3e-5, 0.7, 1.0, 5.5, 65504.0, 8e5, 1e30):  # the maximum lands in [2^14, 2^15)
        assert 2.0 ** 14 <= amax * ref.f16_scale(amax) < 2.0 ** 15


@pytest.mark.parametrize("M,N,K", SHAPES)
def test_restatements_equal_linear_and_autograd(M, N, K):
    a, w, bias, addend = (d(t) for t in ref.operands(M, N, K, "normal"))
    a.requires_grad_(True), w.requires_grad_(True)
    y = F.linear(a, w, bias)
    assert torch.allclose(ref.nt(a, w, bias, addend), y + addend, rtol=1e-13, atol=1e-13)
    assert torch.allclose(ref.nt(a, w), F.linear(a, w), rtol=1e-13, atol=1e-13)
    gy = torch.randn(M, N, dtype=torch.float64, generator=torch.Generator().manual_seed(5))
    ga, gw = torch.autograd.grad(y, (a, w), gy)
    extra = torch.randn(M, K, dtype=torch.float64, generator=torch.Generator().manual_seed(6))
    assert torch.allclose(ref.nn(gy, w.detach()), ga, rtol=1e-13, atol=1e-13)
    assert torch.allclose(ref.nn(gy, w.detach(), extra), ga + extra, rtol=1e-13, atol=1e-13)
    assert torch.allclose(ref.tn(gy, a.detach()), gw, rtol=1e-13, atol=1e-13)
    # the gather forms: P = [A | Bd | ...] per node
    n = 7
    g = torch.Generator().manual_seed(7)
    P = torch.randn(n, 2 * N + 4, dtype=torch.float64, generator=g)
    src, dst = torch.randint(0, n, (M,), generator=g).int(), torch.randint(0, n, (M,), generator=g).int()
    want = y.detach() + P[src.long(), :N] + P[dst.long(), N:2 * N]
    assert torch.allclose(ref.gather(a.detach(), w.detach(), bias, P, src, dst), want, rtol=1e-13, atol=1e-13)
    order = torch.randperm(n, generator=g)
    Bd2, rank = P[order, N:2 * N].contiguous(), torch.argsort(order)[dst.long()].int()
    assert torch.equal(ref.gather2(a.detach(), w.detach(), bias, P, src, Bd2, rank), ref.gather(a.detach(), w.detach(), bias, P, src, dst))


@pytest.mark.parametrize("data", ref.DATA)
@pytest.mark.parametrize("M,N,K", SHAPES)
def test_emulated_schemes_stay_inside_their_bounds(M, N, K, data):
    a, w, _, _ = ref.operands(M, N, K, data)
    exact = d(a) @ d(w).t()
    # f16x3: hh + hl + lh of the scaled slices, every slice product exact in float64
    sa, sw = ref.f16_scale(a.abs().max()), ref.f16_scale(w.abs().max())
    (ha, la), (hw, lw) = ref.slices_f16x2(a, a.abs().max()), ref.slices_f16x2(w, w.abs().max())
    got = (d(ha) @ d(hw).t() + d(ha) @ d(lw).t() + d(la) @ d(hw).t()) / (sa * sw)
    bound = ref.f16x3_scheme_bound(a, w)
    assert torch.allclose(ref.f16x3_scheme_bound_at(a, w, a.abs().max(), w.abs().max()), bound, rtol=1e-12, atol=0.0)
    used =float(((got - exact).abs() / bound.clamp_min(1e-300)).max())
    assert bool(((got - exact).abs() <= bound).all()), ("f16x3", used)
    # bf16x6: the six products of weight >= 2^-16
    (ha, ma, la), (hw, mw, lw) = ref.slices_bf16x3(a), ref.slices_bf16x3(w)
    mm = lambda x, y: d(x) @ d(y).t()  # noqa: E731
    got = mm(ha, hw) + mm(ha, mw) + mm(ma, hw) + mm(ha, lw) + mm(la, hw) + mm(ma, mw)
    bound6 = ref.bf16x6_scheme_bound(a, w)
    used6 = float(((got - exact).abs() / bound6.clamp_min(1e-300)).max())
    assert bool(((got - exact).abs() <= bound6).all()), ("bf16x6", used6)
    # a float32 product of the same operands: the accumulation bound
    acc = ref.accumulation_bound(a, w)
    got32 = d(a @ w.t())
    used32 = float(((got32 - exact).abs() / acc.clamp_min(1e-300)).max())
    assert bool(((got32 - exact).abs() <= acc).all()), ("float32", used32)
    print(f"gemm-ref {data:<10s} ({M}, {N}, {K}): largest error / bound  f16x3 {used:8.2e}  bf16x6 {used6:8.2e}  float32 {used32:8.2e}")


@pytest.mark.parametrize("data", ref.DATA)
@pytest.mark.parametrize("transpose", (False, True))
@pytest.mark.parametrize("N,K", ((16, 16), (260, 48), (80, 64), (512, 32)))
def test_images_decode_back_to_the_slices(N, K, transpose, data):
    _, w, _, _ = ref.operands(3, N, K, data if data != "tiny" else "normal")
    if data == "tiny":
        w = w * 2.0 ** -100
    stored = w.t().contiguous() if transpose else w
    # bf16x3: h + m + l reproduces every float32 bit
    img = ref.image_bf16x3(stored, transpose)
    assert img.numel() == 3 * ((N + 255) // 256 * 256) * K * 2
    h, m, l = ref.decode_image(img, N, K, 3, torch.bfloat16)
    # (every bit, as long as the third slice is a normal number: a subnormal x - h - m keeps its bits in the low half of the word,
    # which the truncation drops - less than 2^-133, and only for |x| < 2^-110)
    back = (h.float() + m.float()) + l.float()
    assert torch.equal(back[w.abs() >= 2.0 ** -110], w[w.abs() >= 2.0 ** -110])
    assert bool(((d(back) - d(w)).abs() < 2.0 ** -133).all())
    assert torch.equal(torch.stack([h, m, l]), torch.stack(ref.slices_bf16x3(w)))
    # f16x2: h + l is x s up to max(2^-22 |x s|, 2^-25)
    amax = w.abs().max()
    s = ref.f16_scale(amax)
    img = ref.image_f16x2(stored, amax, transpose)
    assert img.numel() == 2 * ((N + 255) // 256 * 256) * K * 2
    h, l = ref.decode_image(img, N, K, 2, torch.float16)
    xs = d(w) * s
    assert bool(((d(h) + d(l) - xs).abs() <= (2.0 ** -22 * xs.abs()).clamp_min(2.0 ** -25)).all())
    assert bool(torch.isfinite(h.float()).all())


def test_image_index_map_element_by_element():
    """the vectorised map against the formula written above split_bf16x3_kernel, one element at a time"""
    N, K = 260, 32
    w = torch.arange(N * K, dtype=torch.float32).view(N, K) % 251 + 1  # (bf16-exact values: the h plane is the value)
    img = ref.image_bf16x3(w, False).view(torch.int16)
    ntiles, plane = 2, 256 * 16
    for n in (0, 7, 8, 15, 16, 255, 256, 259):
        for k in (0, 7, 8, 15, 16, 31):
            o = ((k // 16) * ntiles + n // 256) * (3 * plane) + (n % 256) * 16 + ((((k % 16) >> 3) ^ ((n >> 3) & 1)) << 3) + (k & 7)
            assert img[o:o + 1].view(torch.bfloat16).float().item() == w[n, k].item(), (n, k)
            assert img[o + plane].item() == 0 and img[o + 2 * plane].item() == 0
    rows = img.view(K // 16, ntiles, 3, 256, 16)
    assert not bool(rows[:, 1, :, 4:].any())  # rows 260 .. 511


# ---- dw_operands: what tests/test_gpu_gemm_dw_f64.py relies on

DW_M_MAX = 64 * (3 * 256 - 1) - 7  # the largest row count that module can reach: three tiles per workgroup on the largest grid


@pytest.mark.parametrize("data", ref.DW_DATA)
def test_dw_operands_shapes_and_statistics(data):
    M = 4096 + 33
    G, Y, W, addend, xn, nstat = ref.dw_operands(M, data)
    for t, shape in ((G, (M, 256)), (Y, (M, 256)), (W, (256, 256)), (addend, (M, 256)), (xn, (M, 256)), (nstat, (4, 256))):
        assert t.shape == shape and t.dtype == torch.float32 and t.is_contiguous() and bool(torch.isfinite(t).all()), data
    assert all(torch.equal(a, b) for a, b in zip(ref.dw_operands(M, data), (G, Y, W, addend, xn, nstat)))  # (a function of its arguments)
    mean, var = d(xn).mean(0), d(xn).var(0, unbiased=False) + 1e-5
    assert torch.allclose(d(nstat[0]), mean, rtol=1e-6, atol=1e-6) and torch.allclose(d(nstat[1]), var.rsqrt(), rtol=1e-6, atol=0)
    if data in ref.DW_PLAIN + ("cancelling",):  # G W = a w^T of ``operands``
        a, w, _, add = ref.operands(M, 256, 256, data)
        assert torch.equal(G, a) and torch.equal(W, w.t()) and torch.equal(addend, add)
    if data == "bn_mean_over_spread":
        assert float((mean.abs() * var.rsqrt()).max()) > 90
    if data == "bn_scale_zero_negative":
        s = nstat[2]
        assert int((s == 0).sum()) == 86 and int((s > 0).sum()) == 85 and int((s < 0).sum()) == 85
    if data == "bn_saturated":
        z = (d(xn) - mean) * d(nstat[2]) + d(nstat[3])
        assert float(z[:, 0::2].min()) > 30 and float(z[:, 1::2].max()) < -30


def test_dw_integers_are_exact_in_every_order():
    """at the largest M: every fp16 low slice is zero with the true maxima and with maxima 16 x (and 5.5: no power of two) too
    large, and a float32 product - one summation order among many, all of representable partial sums - has float64's bits"""
    G, Y, W, addend, _, _ = ref.dw_operands(DW_M_MAX, "integers")
    assert float(G.abs().max()) == 4 and float(Y.abs().max()) == 4 and float(W.abs().max()) == 0.5
    for x, maxima in ((G, (4.0, 5.5, 64.0)), (Y, (4.0, 5.5, 64.0)), (W, (0.5, 8.0))):
        for amax in maxima:
            h, l = ref.slices_f16x2(x, amax)
            assert not bool(l.any()) and torch.equal(d(h), d(x) * ref.f16_scale(amax)), amax
    assert torch.equal(d(G.t() @ Y), d(G).t() @ d(Y))
    assert torch.equal(d(G @ W + addend), d(G) @ d(W) + d(addend)) and torch.equal(d(G @ W), d(G) @ d(W))
    assert float((d(G).abs().t() @ d(Y).abs()).max()) < 2.0 ** 24  # (the sum of magnitudes itself is an exact float32)


@pytest.mark.parametrize("M", (4096 + 33, 64 * 224 + 1, 128 * 224 + 33))
def test_dw_small_maxima_references_are_float32_numbers(M):
    """both maxima in [2^-63, 2^-61): the two operand scales multiply to at least 2^150, so the product of their inverses is below
    float32's smallest subnormal - while the weight gradient itself is an ordinary float32 tensor: its largest entry is a normal
    number of 2^-123 or more, and so are nine in ten of the others.  (A sum of M products of independent N(0, 1) 2^-64 values is
    N(0, M) 2^-128: one entry in twenty at 4129 rows falls below 2^-126 by chance.  float32 holds those to 2^-150 absolute, which
    is below a thousandth of the bound the kernel is held to at every entry - asserted here, so the bound asks nothing of an
    entry that float32 cannot give.)"""
    G, Y, _, _, _, _ = ref.dw_operands(M, "small_maxima")
    ga, ya = float(G.abs().max()), float(Y.abs().max())
    assert 2.0 ** -63 <= ga < 2.0 ** -61 and 2.0 ** -63 <= ya < 2.0 ** -61
    assert ref.f16_scale(ga) * ref.f16_scale(ya) >= 2.0 ** 150
    inv = torch.tensor(1.0 / ref.f16_scale(ga)) * torch.tensor(1.0 / ref.f16_scale(ya))  # (float32 arithmetic)
    assert inv.dtype == torch.float32 and float(inv) == 0.0
    dw = (d(G).t() @ d(Y)).abs()
    normal = dw >= 2.0 ** -126
    assert float(dw.max()) >= 2.0 ** -123 and float(normal.double().mean()) > 0.9 and float(dw.median()) >= 2.0 ** -126
    bound = ref.f16x3_scheme_bound_at(G.t(), Y.t(), ga, ya) + (M + 3) * ref.U * (d(G).abs().t() @ d(Y).abs())
    assert float(bound.min()) > 2.0 ** 10 * 2.0 ** -150
    assert float((dw / bound).median()) > 2.0  # (a zero in its place is outside the bound at most entries, and by far at the largest)
    assert float((dw / bound).max()) > 8.0


@pytest.mark.parametrize("M", (4096 + 33, 64 * 224 + 1))
def test_dw_cancelling_lies_far_below_the_sum_of_magnitudes(M):
    G, Y, _, _, _, _ = ref.dw_operands(M, "dw_cancelling")
    dw, mag = (d(G).t() @ d(Y)).abs(), d(G).abs().t() @ d(Y).abs()
    assert float((dw / mag).median()) <= 2.0 ** -8


@pytest.mark.parametrize("rows,R", ((1, 64), (64, 64), (65, 64), (300, 128), (257, 64)))
def test_slab_helpers_sum_to_the_whole_tensor(rows, R):
    g = torch.Generator().manual_seed(rows)
    N = 12
    c, xn = torch.randn(rows, N, dtype=torch.float64, generator=g), torch.randn(rows, N, dtype=torch.float64, generator=g) * 2 + 1
    mean, var = xn.mean(0), xn.var(0, unbiased=False) + 1e-5
    gamma, beta = torch.randn(N, dtype=torch.float64, generator=g), torch.randn(N, dtype=torch.float64, generator=g)
    nstat = torch.stack([mean, var.rsqrt(), gamma * var.rsqrt(), beta])
    st = ref.stats_slabs(c, R)
    assert st.shape == ((rows + R - 1) // R, 2, N)
    assert torch.allclose(st.sum(0), torch.stack([c.sum(0), (c * c).sum(0)]), rtol=1e-12, atol=1e-12)
    assert torch.allclose(st[0, 0], c[:R].sum(0), rtol=1e-12, atol=1e-12)
    # the BatchNorm-backward sums against autograd of y = silu(BatchNorm(xn)) with frozen statistics
    z = ((xn - mean) * nstat[2] + beta).requires_grad_(True)
    (gz,) = torch.autograd.grad(F.silu(z), z, c)
    red = ref.bnred_slabs(c, xn, nstat, R)
    want = torch.stack([gz.sum(0), (gz * (xn - mean) * nstat[1]).sum(0)])
    assert torch.allclose(red.sum(0), want, rtol=1e-11, atol=1e-11)
