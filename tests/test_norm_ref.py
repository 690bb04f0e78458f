"""tests/norm_ref.py itself, before csrc/norm.hip is measured against it (tests/test_gpu_norm.py): in float64 the restatement is
``F.batch_norm`` / ``F.layer_norm`` + ``F.silu`` and their autograd - values, every gradient, the running statistics, training
and evaluation mode -, the input gradients are derivatives (central differences), the sums are sums, and every data distribution
of the GPU tests is well enough conditioned for a float32 kernel to be judged on it: the float32 restatement stays within 1e-4 of
float64 on every output (the bar of BASELINE.json's north star, the cap of tests/test_conv_bn_ref.py)."""

import pytest
import torch
import torch.nn.functional as F

from tests import norm_ref as ref

CAP = 1e-4
D = torch.float64


def err(a, b, floor=1e-30):
    a, b = a.detach().double(), b.detach().double()
    return float((a - b).abs().max() / b.abs().max().clamp_min(floor))


def _bn_problem(rows, H, seed):
    g = torch.Generator().manual_seed(seed)
    R = lambda *s: torch.randn(*s, generator=g, dtype=D)  # noqa: E731
    return dict(x=R(rows, H) * 2 + 0.5, gy=R(rows, H), r=R(rows, H), gamma=1 + 0.2 * R(H), beta=0.2 * R(H), rm=0.3 * R(H),
                rv=0.5 + torch.rand(H, generator=g, dtype=D))


@pytest.mark.parametrize("training", [True, False])
@pytest.mark.parametrize("rows", [1, 2, 3, 257])
def test_batchnorm_restatement_is_torch_autograd(rows, training):
    """bn_stat / eval_stat / running_update / bn_silu_fwd / bn_bwd_red / bn_bwd_apply against F.batch_norm + F.silu and its
    autograd: y (with the residual), gx, dgamma, dbeta, both running statistics.  One row in training mode, which torch
    refuses, is spelled out as tests/test_gpu_kernels.py::test_mlp_layer_fn_matches_torch_batchnorm spells it."""
    H = 8
    o = _bn_problem(rows, H, 10 * rows + training)
    x, gamma, beta = (o[k].clone().requires_grad_(True) for k in ("x", "gamma", "beta"))
    rm, rv = o["rm"].clone(), o["rv"].clone()
    if rows > 1 or not training:
        z = F.batch_norm(x, rm, rv, gamma, beta, training, ref.MOMENTUM, ref.EPS_BN)
    else:
        z = (x - x.mean(0)) * torch.rsqrt(x.var(0, unbiased=False) + ref.EPS_BN) * gamma + beta
        rm = 0.9 * rm + 0.1 * x.mean(0).detach()
        rv = 0.9 * rv + 0.1 * x.var(0, unbiased=False).detach()  # (the kernels' choice for one row: the biased variance, 0)
    y = F.silu(z) + o["r"]
    gx, dgamma, dbeta = torch.autograd.grad((o["gy"] * y).sum(), [x, gamma, beta])
    if training:
        stat, var = ref.bn_stat(o["x"], o["gamma"], o["beta"])
        rm2, rv2 = ref.running_update(o["rm"], o["rv"], stat[0], var, rows)
        assert err(stat[0], o["x"].mean(0)) < 1e-13 and err(var, o["x"].var(0, unbiased=False), 1e-3) < 1e-13
    else:
        stat = ref.eval_stat(o["rm"], o["rv"], o["gamma"], o["beta"])
        rm2, rv2 = o["rm"], o["rv"]
    assert err(rm2, rm) < 1e-13 and err(rv2, rv) < 1e-13
    assert torch.equal(stat[3], o["beta"]) and err(stat[2], o["gamma"] * stat[1]) < 1e-15
    assert err(ref.bn_silu_fwd(o["x"], o["r"], stat), y) < 1e-13
    assert err(ref.bn_silu_fwd(o["x"], None, stat), y - o["r"]) < 1e-13
    red = ref.bn_bwd_red(o["gy"], o["x"], stat)
    assert err(red[0], dbeta) < 1e-12 and err(red[1], dgamma, 1e-3) < 1e-10
    assert err(ref.bn_bwd_apply(o["gy"], o["x"], stat, red, not training), gx, 1e-3) < 1e-10


def test_eval_stat_defaults_are_one_and_zero():
    o = _bn_problem(5, 8, 3)
    a = ref.eval_stat(o["rm"], o["rv"], None, None)
    assert torch.equal(a, ref.eval_stat(o["rm"], o["rv"], torch.ones(8, dtype=D), torch.zeros(8, dtype=D)))


@pytest.mark.parametrize("rows,H", [(1, 4), (3, 8), (65, 260)])
def test_layernorm_restatement_is_torch_autograd(rows, H):
    """ln_silu_fwd / ln_silu_bwd against F.layer_norm + F.silu and its autograd: y (with the residual), the saved (mean, rstd)
    rows, gx, dgamma, dbeta."""
    g = torch.Generator().manual_seed(rows)
    R = lambda *s: torch.randn(*s, generator=g, dtype=D)  # noqa: E731
    x0, gy, r, gamma0, beta0 = R(rows, H) * 2 + 0.5, R(rows, H), R(rows, H), 1 + 0.2 * R(H), 0.2 * R(H)
    x, gamma, beta = (t.clone().requires_grad_(True) for t in (x0, gamma0, beta0))
    y = F.silu(F.layer_norm(x, (H,), gamma, beta, ref.EPS_LN)) + r
    gx, dgamma, dbeta = torch.autograd.grad((gy * y).sum(), [x, gamma, beta])
    y2, stats = ref.ln_silu_fwd(x0, r, gamma0, beta0)
    assert err(y2, y) < 1e-13 and err(ref.ln_silu_fwd(x0, None, gamma0, beta0)[0], y - r) < 1e-13
    assert err(stats[:, 0], x0.mean(1)) < 1e-14
    assert err(stats[:, 1], (x0.var(1, unbiased=False) + ref.EPS_LN).rsqrt()) < 1e-13
    gx2, dbeta2, dgamma2 = ref.ln_silu_bwd(gy, x0, gamma0, beta0, stats)
    assert err(gx2, gx, 1e-3) < 1e-10 and err(dbeta2, dbeta) < 1e-12 and err(dgamma2, dgamma) < 1e-12


def test_input_gradients_are_derivatives():
    """central differences in float64 along random directions: bn_bwd_apply in training and evaluation mode (the statistics
    move with x in the first and are constants in the second), ln_silu_bwd, node_adjoints."""
    rows, H, h = 37, 12, 1e-6
    o = _bn_problem(rows, H, 77)
    g = torch.Generator().manual_seed(5)
    ev = ref.eval_stat(o["rm"], o["rv"], o["gamma"], o["beta"])

    def bn_loss(x, training):
        stat = ref.bn_stat(x, o["gamma"], o["beta"])[0] if training else ev
        return (o["gy"] * ref.bn_silu_fwd(x, o["r"], stat)).sum()

    def ln_loss(x):
        return (o["gy"] * ref.ln_silu_fwd(x, o["r"], o["gamma"], o["beta"])[0]).sum()

    stat = ref.bn_stat(o["x"], o["gamma"], o["beta"])[0]
    gx_train = ref.bn_bwd_apply(o["gy"], o["x"], stat, ref.bn_bwd_red(o["gy"], o["x"], stat), False)
    gx_eval = ref.bn_bwd_apply(o["gy"], o["x"], ev, None, True)
    gx_ln = ref.ln_silu_bwd(o["gy"], o["x"], o["gamma"], o["beta"], ref.ln_silu_fwd(o["x"], None, o["gamma"], o["beta"])[1])[0]
    for _ in range(3):
        d = torch.randn(rows, H, generator=g, dtype=D)
        for gx, f in ((gx_train, lambda x: bn_loss(x, True)), (gx_eval, lambda x: bn_loss(x, False)), (gx_ln, ln_loss)):
            fd, an = (f(o["x"] + h * d) - f(o["x"] - h * d)) / (2 * h), (gx * d).sum()
            assert abs(float(fd - an)) < 1e-6 * abs(float(an)), (float(fd), float(an))
    # the quotient xpre = Ux + s1 / (s0 + eps), hh = s1 / (s0 + eps); s0 moves in proportion to itself (s0 = 0 sits one step
    # of h away from the pole at -eps)
    s0 = 8 * torch.rand(rows, H, generator=g, dtype=D)
    s0[::7] = 0.0
    s1 = torch.randn(rows, H, generator=g, dtype=D)
    gs1, gs0 = ref.node_adjoints(gx_train, s0, s1 / (s0 + ref.EPS_GATE))
    d1, d0 = torch.randn(rows, H, generator=g, dtype=D), s0 * torch.randn(rows, H, generator=g, dtype=D)
    q = lambda s: (gx_train * ((s1 + s * h * d1) / (s0 + s * h * d0 + ref.EPS_GATE))).sum()  # noqa: E731
    fd, an = (q(1) - q(-1)) / (2 * h), (gs1 * d1).sum() + (gs0 * d0).sum()
    assert abs(float(fd - an)) < 1e-6 * abs(float(an))


def test_sums():
    g = torch.Generator().manual_seed(2)
    for slabs in (1, 63, 64, 65, 257):
        p = torch.randn(slabs, 6, generator=g, dtype=D)
        f = ref.slab_fold(p)
        assert f.shape == (ref.FOLD, 6)
        for k in range(ref.FOLD):
            want = p[k::ref.FOLD].sum(0) if k < slabs else torch.zeros(6, dtype=D)
            assert err(f[k], want, 1.0) < 1e-14
            if k >= slabs:
                assert not bool(f[k].any())
        assert err(ref.slab_sum(f), ref.slab_sum(p), 1.0) < 1e-13 and torch.equal(ref.col_sum(p), p.sum(0))


def cap_errors(rows, H, data):
    """{output: error of the float32 restatement against float64} over everything the GPU tests compare on ``data``, each pass
    handed the float64 result of the one before it rounded once, as there"""
    out = {}
    f32, f64 = (lambda t: t.float()), (lambda t: t.double())
    o = ref.operands(rows, H, data, "cpu", "bn")
    stat64, var64 = ref.bn_stat(f64(o["x"]), f64(o["gamma"]), f64(o["beta"]))
    stat32, var32 = ref.bn_stat(o["x"], o["gamma"], o["beta"])
    out["bn mean"] = float((stat32[0].double() - stat64[0]).abs().max() / (stat64[0].abs().max() + 1.0))
    out["bn rstd"] = float(((stat32[1].double() - stat64[1]) / stat64[1]).abs().max())
    rv64 = ref.running_update(f64(o["rm"]), f64(o["rv"]), stat64[0], var64, rows)[1]
    rv32 = ref.running_update(o["rm"], o["rv"], stat32[0], var32, rows)[1]
    out["bn rvar"] = float(((rv32.double() - rv64) / rv64).abs().max())
    if data not in ref.DATA:  # (a statistics-only distribution)
        return out
    ev = ref.eval_stat(f64(o["rm"]), f64(o["rv"]), f64(o["gamma"]), f64(o["beta"])).float()
    for tag, st in (("", stat64.float()), (" eval", ev)):
        both = []
        red_in = ref.bn_bwd_red(f64(o["gy"]), f64(o["x"]), f64(st)).float()
        for c in (f64, f32):
            x, gy, s = c(o["x"]), c(o["gy"]), c(st)
            red = ref.bn_bwd_red(gy, x, s)
            gx = ref.bn_bwd_apply(gy, x, s, c(red_in), bool(tag))
            gs1, gs0 = ref.node_adjoints(gx, c(o["s0"]), c(o["hh"]))
            both.append({"y": ref.bn_silu_fwd(x, c(o["r"]), s), "red": red, "dbeta": red[0], "dgamma": red[1], "gx": gx, "gs1": gs1,
                         "gs0": gs0})
        out.update({f"bn {k}{tag}": err(both[1][k], both[0][k]) for k in both[0]})
    o = ref.operands(rows, H, data, "cpu", "ln")
    y64, st64 = ref.ln_silu_fwd(f64(o["x"]), f64(o["r"]), f64(o["gamma"]), f64(o["beta"]))
    y32, st32 = ref.ln_silu_fwd(o["x"], o["r"], o["gamma"], o["beta"])
    out["ln y"] = err(y32, y64)
    out["ln mean"] = float((st32[:, 0].double() - st64[:, 0]).abs().max() / (st64[:, 0].abs().max() + 1.0))
    out["ln rstd"] = float(((st32[:, 1].double() - st64[:, 1]) / st64[:, 1]).abs().max())
    b64 = ref.ln_silu_bwd(f64(o["gy"]), f64(o["x"]), f64(o["gamma"]), f64(o["beta"]), f64(st64.float()))
    b32 = ref.ln_silu_bwd(o["gy"], o["x"], o["gamma"], o["beta"], st64.float())
    for k, a, b in zip(("gx", "dbeta", "dgamma"), b32, b64):
        out[f"ln {k}"] = err(a, b)
    return out


@pytest.mark.parametrize("data", ref.STAT_DATA)
def test_every_distribution_is_within_the_conditioning_cap(data):
    """The float32 restatement against float64, per output, at rows 4099, F 64: below 1e-4 on every distribution of ref.DATA.
    ``offset300`` is a statistics-only distribution: its mean, rstd and running variance are inside the cap, its values and
    gradients are not (y 1.2e-3, gx 2.7e-3: the data's own float32 resolution) and are not compared anywhere."""
    errors = cap_errors(4099, 64, data)
    for k, e in errors.items():
        print(f"norm-cap {data:<10s} {k:<16s} float32 {e:8.2e}")
    bad = {k: e for k, e in errors.items() if not e < CAP}
    assert not bad, bad


def test_the_distributions_are_what_they_say():
    o = ref.operands(4099, 64, "constant", "cpu", "bn")
    assert bool((o["x"][:, ::4] == o["x"][:1, ::4]).all()) and not bool((o["x"][:, 1] == o["x"][0, 1]).all())
    o = ref.operands(4099, 64, "constant", "cpu", "ln")
    assert bool((o["x"][::4] == o["x"][::4, :1]).all())
    o = ref.operands(4099, 64, "saturated", "cpu", "bn")
    st = ref.eval_stat(o["rm"], o["rv"], o["gamma"], o["beta"])  # (batch statistics normalise the scale away: frozen ones)
    assert float(((o["x"] - st[0]) * st[2] + st[3]).abs().max()) > 80
    o = ref.operands(4099, 64, "gamma30", "cpu", "bn")
    st = ref.bn_stat(o["x"], o["gamma"], o["beta"])[0]
    assert float(((o["x"] - st[0]) * st[2] + st[3]).abs().max()) > 80
    o = ref.operands(4099, 64, "offset30", "cpu", "bn")
    assert 25 < float((o["x"].mean(0).abs() / o["x"].std(0)).min()) and float((o["x"].mean(0).abs() / o["x"].std(0)).max()) < 60
    assert bool((ref.operands(50, 8, "normal", "cpu")["s0"][::7] == 0).all())
