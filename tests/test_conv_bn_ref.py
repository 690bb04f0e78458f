"""tests/conv_bn_ref.py itself, before csrc/conv.hip is measured against it (tests/test_gpu_conv_bn.py): the restatement is the
model's own torch path, the closed-form BatchNorm backward the kernels use is autograd's, the reverse outputs are derivatives
(central differences), and every data distribution of the GPU tests is well enough conditioned for a float32 kernel to be judged
on it - the float32 restatement stays within 1e-4 of float64 on every output (the bar of BASELINE.json's north star)."""

import pytest
import torch
import torch.nn.functional as F

from alignn_amd import torch_path
from alignn_amd.alignn import EdgeGatedGraphConv
from tests import conv_bn_ref as ref
from tests.gate_parity import err, graph

MODES = ((0, 0), (1, 0), (1, 1), (2, 0))  # (mode, e_eval)
CAP = 1e-4


def _uv(gname):
    g = graph(gname, "cpu")
    return g.src.long(), g.dst.long(), g.n_nodes


@pytest.mark.parametrize("train", [True, False])
@pytest.mark.parametrize("residual", [True, False])
@pytest.mark.parametrize("gname", ["synthetic", "lg_small"])
def test_values_are_the_torch_path(gname, residual, train):
    """float64 on CPU: values() against alignn_amd.torch_path.edge_gated_conv on an EdgeGatedGraphConv in .double(), in
    training and evaluation mode, with and without the residual; the running statistics after the call too."""
    H = 12
    u, v, n = _uv(gname)
    torch.manual_seed(5)
    mod = EdgeGatedGraphConv(H, H, residual=residual).double()
    with torch.no_grad():
        for bn in (mod.bn_edges, mod.bn_nodes):
            bn.weight.copy_(1 + 0.2 * torch.randn(H))
            bn.bias.copy_(0.2 * torch.randn(H))
            bn.running_mean.copy_(0.3 * torch.randn(H))
            bn.running_var.copy_(0.5 + torch.rand(H))
    mod.train(train)
    x, y = torch.randn(n, H, dtype=torch.float64), torch.randn(u.numel(), H, dtype=torch.float64)
    running = dict(e_rm=mod.bn_edges.running_mean.clone(), e_rv=mod.bn_edges.running_var.clone(),
                   n_rm=mod.bn_nodes.running_mean.clone(), n_rv=mod.bn_nodes.running_var.clone())
    with torch.no_grad():
        P = torch.cat([mod.src_gate(x), mod.dst_gate(x), mod.dst_update(x), mod.src_update(x)], 1)
        C = mod.edge_gate(y)
        eg, eb, ng, nb = mod.bn_edges.weight, mod.bn_edges.bias, mod.bn_nodes.weight, mod.bn_nodes.bias
        e_stat = None if train else ref.eval_stat(running["e_rm"], running["e_rv"], eg, eb)
        n_stat = None if train else ref.eval_stat(running["n_rm"], running["n_rv"], ng, nb)
        f = ref.values(P, C, False, eg, eb, e_stat, u, v, n, H, n_gamma=ng, n_beta=nb, n_stat=n_stat, running=running)
        x_new, y_new = torch_path.edge_gated_conv(mod, u, v, n, x, y)
    assert err(f["x"] + (x if residual else 0), x_new) < 1e-12
    assert err(f["y"] + (y if residual else 0), y_new) < 1e-12
    g = ref.values(P, f["m"], True, eg, eb, e_stat, u, v, n, H)  # (the `pre` form: m handed over)
    assert torch.equal(g["y"], f["y"]) and torch.equal(g["xpre"], f["xpre"])
    for k, bn, attr in (("e_rm", mod.bn_edges, "running_mean"), ("e_rv", mod.bn_edges, "running_var"),
                        ("n_rm", mod.bn_nodes, "running_mean"), ("n_rv", mod.bn_nodes, "running_var")):
        want = getattr(bn, attr)
        if train:
            assert err(f[k], want) < 1e-12, k
            assert not torch.equal(want, running[k]), k
        else:
            assert torch.equal(want, running[k]), k
    # explicit column statistics = torch's
    assert err(f["e_mean"], f["m"].mean(0)) < 1e-12 and err(f["e_var"], f["m"].var(0, unbiased=False)) < 1e-12
    assert err(f["n_mean"], f["xpre"].mean(0)) < 1e-12 and err(f["n_var"], f["xpre"].var(0, unbiased=False)) < 1e-12


@pytest.mark.parametrize("rows", [1, 2, 257])
def test_closed_form_batchnorm_backward_is_autograd(rows):
    """The closed form csrc/conv.hip's edge_grad uses - sc * (gz - (c0 + xhat * c1) / rows) with (c0, c1) = (sum gz, sum gz *
    xhat), and gz * sc under frozen statistics - equals autograd of F.batch_norm + silu; (c0, c1) are the adjoints of beta
    and gamma."""
    H = 8
    g = torch.Generator().manual_seed(rows)
    x = torch.randn(rows, H, generator=g, dtype=torch.float64, requires_grad=True)
    gy = torch.randn(rows, H, generator=g, dtype=torch.float64)
    gamma = (1 + 0.2 * torch.randn(H, generator=g, dtype=torch.float64)).requires_grad_(True)
    beta = (0.2 * torch.randn(H, generator=g, dtype=torch.float64)).requires_grad_(True)
    rm, rv = 0.3 * torch.randn(H, generator=g, dtype=torch.float64), 0.5 + torch.rand(H, generator=g, dtype=torch.float64)
    dsilu = lambda z: torch.sigmoid(z) * (1 + z * (1 - torch.sigmoid(z)))  # noqa: E731
    for training in ((True, False) if rows > 1 else (False,)):  # (F.batch_norm refuses one row in training mode)
        z = F.batch_norm(x, None if training else rm.clone(), None if training else rv.clone(), gamma, beta, training, 0.1, ref.EPS_BN)
        gx, dgamma, dbeta = torch.autograd.grad((gy * F.silu(z)).sum(), [x, gamma, beta])
        with torch.no_grad():
            stat = ref.batch_stat(x, gamma, beta)[0] if training else ref.eval_stat(rm, rv, gamma, beta)
            mean, rstd, sc, sh = stat
            xhat = (x - mean) * rstd
            gz = gy * dsilu((x - mean) * sc + sh)
            c0, c1 = gz.sum(0), (gz * xhat).sum(0)
            closed = sc * (gz - (c0 + xhat * c1) / rows) if training else gz * sc
        assert err(closed, gx, 1e-3) < 1e-11, training
        assert err(c0, dbeta) < 1e-12 and err(c1, dgamma, 1e-3) < 1e-11, training


@pytest.mark.parametrize("mode,e_eval", MODES)
@pytest.mark.parametrize("gname", ["synthetic", "one_atom_cell"])
def test_the_restatements_are_consistent(gname, mode, e_eval):
    """The reverse outputs ARE the derivatives of <GY, y> + <Q1, s1> + <Q0, s0> (mode 2: <GY, m>; mode 0: no GY term): central
    differences in float64 along random directions of (M, A, Bd, Bh, gamma, beta); gb is the column sum of GM, and the node
    quotient reverse is the derivative of xpre = Ux + s1 / (s0 + eps)."""
    H = 8
    u, v, n = _uv(gname)
    o = {k: t.double() for k, t in ref.operands(H, u, v, n, "normal", gname, "cpu").items()}
    stat = ref.eval_stat(o["e_rm"], o["e_rv"], o["e_gamma"], o["e_beta"])
    r = ref.reverse(torch.float64, o["P"], o["M"], o["e_gamma"], o["e_beta"], stat, o["GY"], o["Q1"], o["Q0"], u, v, n, H, mode, e_eval)
    assert err(r["gb"], r["GM"].sum(0)) < 1e-13 and torch.equal(r["GP_bd"], r["GP"][:, H:2 * H])
    A0, Bd0, _, _ = ref.blocks(o["P"], H)

    def loss(P, M, gamma, beta):
        A, Bd, _, _ = ref.blocks(P, H)
        m = M + (A - A0)[u] + (Bd - Bd0)[v]
        fixed = ref.eval_stat(o["e_rm"], o["e_rv"], gamma, beta) if (mode == 1 and e_eval) else None
        f = ref.values(P, m, True, gamma, beta, fixed, u, v, n, H)
        out = (o["Q1"] * f["s1"]).sum() + (o["Q0"] * f["s0"]).sum()
        return out + ((o["GY"] * f["y"]).sum() if mode == 1 else (o["GY"] * m).sum() if mode == 2 else 0.0)

    gen = torch.Generator().manual_seed(7)
    h = 1e-6
    for _ in range(3):
        dP, dM = torch.randn(n, 4 * H, generator=gen, dtype=torch.float64), torch.randn(u.numel(), H, generator=gen, dtype=torch.float64)
        dP[:, 3 * H:] = 0.0  # (Ux does not enter the loss)
        dg, db = torch.randn(H, generator=gen, dtype=torch.float64), torch.randn(H, generator=gen, dtype=torch.float64)
        fd = (loss(o["P"] + h * dP, o["M"] + h * dM, o["e_gamma"] + h * dg, o["e_beta"] + h * db)
              - loss(o["P"] - h * dP, o["M"] - h * dM, o["e_gamma"] - h * dg, o["e_beta"] - h * db)) / (2 * h)
        an = (r["GM"] * dM).sum() + (r["GP"] * dP[:, :3 * H]).sum()
        if mode == 1:
            an = an + (r["e_red"][0] * db).sum() + (r["e_red"][1] * dg).sum()
        assert abs(float(fd - an)) < 1e-6 * abs(float(an)), (float(fd), float(an))
    # node quotient
    f = ref.values(o["P"], o["M"], True, o["e_gamma"], o["e_beta"], None, u, v, n, H)
    gs1, gs0 = ref.node_reverse(o["GX"], f["s0"], f["hh"])
    # (s0 moves in proportion to itself: an empty segment's s0 = 0 sits one step of h away from the pole at -eps)
    d1, d0 = torch.randn(n, H, generator=gen, dtype=torch.float64), f["s0"] * torch.randn(n, H, generator=gen, dtype=torch.float64)
    q = lambda s: (o["GX"] * ((f["s1"] + s * h * d1) / (f["s0"] + s * h * d0 + ref.EPS_GATE))).sum()  # noqa: E731
    fd, an = (q(1) - q(-1)) / (2 * h), (gs1 * d1).sum() + (gs0 * d0).sum()
    assert abs(float(fd - an)) < 1e-6 * abs(float(an))


def cap_errors(o, u, v, n, H):
    """{output: error of the float32 restatement against float64} over everything the GPU tests compare, with their floors"""
    out = {}
    both = []
    for dt in (torch.float64, torch.float32):
        c = {k: t.to(dt) for k, t in o.items()}
        ev = ref.eval_stat(c["e_rm"], c["e_rv"], c["e_gamma"], c["e_beta"])
        d = {}
        for pre in (False, True):
            f = ref.values(c["P"], c["M"] if pre else c["C"], pre, c["e_gamma"], c["e_beta"], None, u, v, n, H)
            d.update({f"{k}{' pre' if pre else ''}": f[k] for k in ("m", "s0", "hh", "xpre", "y")})
        d["y eval"] = ref.values(c["P"], c["C"], False, c["e_gamma"], c["e_beta"], ev, u, v, n, H)["y"]
        s0 = d["s0 pre"].clone()
        s0[::7] = 0.0
        d["GS1"], d["GS0"] = ref.node_reverse(c["GX"], s0, d["hh pre"])
        both.append(d)
    for k in both[0]:
        out[k] = err(both[1][k], both[0][k])
    stat64 = ref.batch_stat(o["M"].double(), o["e_gamma"].double(), o["e_beta"].double())[0]
    for mode, e_eval in MODES:
        st = ref.eval_stat(*(o[k].double() for k in ("e_rm", "e_rv", "e_gamma", "e_beta"))) if e_eval else stat64
        st = st.float()  # (what the kernels are handed: float64 statistics rounded once)
        a, b = (ref.reverse(dt, o["P"], o["M"], o["e_gamma"], o["e_beta"], st, o["GY"], o["Q1"], o["Q0"], u, v, n, H, mode, e_eval)
                for dt in (torch.float64, torch.float32))
        fl = 1e-2 * float(a["GP"].abs().max())
        for k in ("GM", "GP", "gb"):
            out[f"{k} mode {mode}{' eval' if e_eval else ''}"] = err(b[k], a[k], fl)
        if mode == 1 and not e_eval:
            out["e_red"] = err(b["e_red"], a["e_red"])
    return out


@pytest.mark.parametrize("data", ref.DATA)
@pytest.mark.parametrize("gname", ["lg_small", "lg_deg17", "bond", "synthetic", "one_atom_cell", "one_segment"])
def test_every_distribution_is_within_the_conditioning_cap(gname, data):
    """The float32 restatement against float64, per output, on every data distribution of the GPU tests: below 1e-4."""
    H = 36
    u, v, n = _uv(gname)
    o = ref.operands(H, u, v, n, data, gname, "cpu")
    if data == "constant_column":
        assert bool((o["M"][:, ::4] == o["M"][:1, ::4]).all())
    if data == "saturated_gates" and n >= 5:
        sg = torch.sigmoid(o["M"])
        assert float(((sg == 0) | (sg == 1)).float().mean()) > 0.3
    errors = cap_errors(o, u, v, n, H)
    for k, e in errors.items():
        print(f"conv-bn-cap H={H} {gname:<14s} {data:<20s} {k:<16s} float32 {e:8.2e}")
    bad = {k: e for k, e in errors.items() if not e < CAP}
    assert not bad, bad
