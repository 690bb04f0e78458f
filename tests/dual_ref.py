"""Plain torch restatements of what csrc/dual.hip and csrc/convln.hip compute: the LayerNorm flavour of ``EdgeGatedGraphConv.forward``
(alignn/models/alignn_atomwise.py:151-208) on dual numbers - every activation p next to its directional derivative pt - with
m = A[u] + Bd[v] + C, the LayerNorm + SiLU row map on duals, and the reverse passes as autograd of the same expressions.

Every function works in the dtype of its floating inputs: float64 is the reference, the same function on the identical float32
operands is the "float32 restatement" the GPU tests (tests/test_gpu_dual_f64.py, tests/test_gpu_convln.py) take their margin from
on every data distribution other than N(0,1).  Only forward formulas are written here (``index_add``, ``sigmoid``, explicit row
statistics, explicit tangents - torch's jvp tangents do not differentiate correctly with respect to the primal); every adjoint is
``torch.autograd.grad`` of them, so a wrong derivative formula cannot sit on both sides of a comparison.  The graph arguments
are plain index tensors ``u -> v`` (source and destination of every row).

``operands`` / ``row_operands`` draw the data distributions of the GPU tests.  The conditioning cap (tests/test_dual_ref.py): on
each of them the float32 restatement stays within 1e-4 of float64 on every output, the bar of BASELINE.json's north star; a
distribution that left it would be too ill-conditioned to judge a float32 kernel by, and is tamed HERE, never loosened or skipped
on the GPU side.  One was tamed that way:
* ``constant_rows`` (every third row of m exactly constant: variance 0, rstd = 1 / sqrt(eps) = 316).  Drawn as N(0,1) constants
  (as tests/test_gpu_convln.py draws them, at H <= 256) the float32 row mean of H equal values is not that value and 316
  multiplies the residue: yt 2.3e-4, GMt 3.2e-4, GPt 1.3e-4, dgamma 1.3e-4 measured at
  H in 64..1024.  Here the constant of such a row is k / 64 with integer |k| <= 256, so every partial sum of up to 1024 copies is
  exact in float32 in any order (<= 8e-7 measured on every output); variance 0 and rstd = 316 stay.  It is used at power-of-two
  widths only (4, 64, 256, 512, 1024): the forward kernel forms mean = sum * (1.0f / F), which at any other width is
  legitimately one rounding away from the constant, and 316 times that rounding is no defect.
How the others are drawn: ``mean_over_spread`` moves every row of m by up to 100 spreads; ``rows_1e-4_1e4`` scales every third
row by 1e-4 and every other third by 1e4; ``gamma_zero_negative`` zeroes a third of each gamma and lets the rest take either sign;
``saturated_gates`` is that of tests/conv_bn_ref.py: every third row sign * (110 + 20 |m|) (sigmoid exactly 0 or 1), the whole
segments of every fifth node m = -(22 + 2 |m|) (S0 ~ 1e-9, far below the epsilon) and those of another fifth -(110 + 20 |m|)
(S0 = 0) - on these two fifths of the nodes 1 / (S0 + eps) is near 1e6, and ``saturated_nodes`` names them so that errors are
taken over their rows and over the rest separately.

Worst float32 error of the restatements, as tests/test_dual_ref.py measures it (max |a - b| / max |b| per output, the gate
reverse with its floor of 1e-2 of the largest node gradient, over every case of GATE_CASES on the graphs ``synthetic``,
``lg_small``, ``lg_deg17``, ``one_atom_cell``, ``one_segment``, ``no_edges`` and the cases of ROW_CASES it runs):
    distribution          gate passes (worst output)               LayerNorm rows (worst output)
    normal                6.8e-6 (gb without GL, one_segment)      3.6e-7 (Q0)
    mean_over_spread      7.8e-6 (GL)                              6.3e-6 (Q0)
    constant_rows         1.2e-6 (GPt with GL)                     3.2e-7 (Q0t)
    rows_1e-4_1e4         6.5e-7 (s0)                              3.1e-7 (gx)
    gamma_zero_negative   8.4e-7 (s0)                              3.3e-7 (gx)
    saturated_gates       7.8e-7 (s0)                              3.0e-7 (dgamma)
All below the cap of 1e-4.
"""

import zlib

import torch
import torch.nn.functional as F

EPS, EPS_GATE = 1e-5, 1e-6  # nn.LayerNorm's default; ALIGNN_EPS_GATE (csrc/common.h)
DATA = ("normal", "mean_over_spread", "constant_rows", "rows_1e-4_1e4", "gamma_zero_negative", "saturated_gates")
CONSTANT_ROWS_WIDTHS = (4, 64, 256, 512, 1024)


def _blocks(P, H):
    """A | Bd | Bh | Ux of the fused node projection [n, 4H]"""
    return P[:, :H], P[:, H:2 * H], P[:, 2 * H:3 * H], P[:, 3 * H:]


# ----------------------------------------------------------------------------------------------------------------------
# forward
# ----------------------------------------------------------------------------------------------------------------------
def ln_dual(x, t, res, res_t, gamma, beta):
    """y = res + silu(LN(x)) and its tangent along (t, res_t), the row means and the row rstd = 1 / sqrt(var + eps)"""
    mean = x.mean(1, keepdim=True)
    rho = (((x - mean) ** 2).mean(1, keepdim=True) + EPS).rsqrt()
    xh = (x - mean) * rho
    th = rho * (t - t.mean(1, keepdim=True) - xh * (xh * t).mean(1, keepdim=True))
    zz, zt = gamma * xh + beta, gamma * th
    sz = torch.sigmoid(zz)
    y, yt = zz * sz, (sz + zz * sz * (1 - sz)) * zt
    if res is not None:
        y, yt = y + res, yt + res_t
    return y, yt, mean[:, 0], rho[:, 0]


def gate_dual(P, Pt, C_or_M, Ct_or_Mt, pre, u, v, n, H):
    """The gate pass on duals.  ``pre``: the arguments ARE m and mt; otherwise they are C and Ct, m = A[u] + Bd[v] + C.  The two
    segment sums of sigma(m) (times Bh[u]), the quotient h = s1 / (s0 + eps), the node pre-activation Ux + h, and the tangent of
    each."""
    A, Bd, Bh, Ux = _blocks(P, H)
    At, Bdt, Bht, Uxt = _blocks(Pt, H)
    m = C_or_M if pre else A[u] + Bd[v] + C_or_M
    mt = Ct_or_Mt if pre else At[u] + Bdt[v] + Ct_or_Mt
    sg = torch.sigmoid(m)
    sgt = sg * (1 - sg) * mt
    z = lambda: torch.zeros(n, H, dtype=m.dtype, device=m.device)  # noqa: E731
    s1, s0 = z().index_add(0, v, sg * Bh[u]), z().index_add(0, v, sg)
    s1t, s0t = z().index_add(0, v, sgt * Bh[u] + sg * Bht[u]), z().index_add(0, v, sgt)
    hh = s1 / (s0 + EPS_GATE)
    hht = (s1t - hh * s0t) / (s0 + EPS_GATE)
    return dict(m=m, mt=mt, s1=s1, s0=s0, s1t=s1t, s0t=s0t, hh=hh, hht=hht, xpre=Ux + hh, xpre_t=Uxt + hht)


def _values(P, M, gamma, beta, u, v, n, H):
    """what the forward pass writes: the LayerNorm branch y = silu(LN(m)), the row statistics, the two segment sums of
    sigma(m) and the node pre-activation Ux + s1 / (s0 + eps)"""
    _, _, Bh, Ux = _blocks(P, H)
    y = F.silu(F.layer_norm(M, (H,), gamma, beta, EPS))
    mean = M.mean(1)
    rstd = (((M - mean[:, None]) ** 2).mean(1) + EPS).rsqrt()
    sg = torch.sigmoid(M)
    z = lambda: torch.zeros(n, H, dtype=M.dtype, device=M.device)  # noqa: E731
    s1, s0 = z().index_add(0, v, sg * Bh[u]), z().index_add(0, v, sg)
    hh = s1 / (s0 + EPS_GATE)
    return dict(y=y, mean=mean, rstd=rstd, s1=s1, s0=s0, hh=hh, xpre=Ux + hh)


def _duals(P, Pt, M, Mt, gamma, beta, u, v, n, H):
    """value and tangent of the same (``ln_dual`` of the given m, mt without residual, and ``gate_dual`` of them)"""
    y, yt, _, _ = ln_dual(M, Mt, None, None, gamma, beta)
    d = gate_dual(P, Pt, M, Mt, True, u, v, n, H)
    return dict(y=y, yt=yt, s1=d["s1"], s0=d["s0"], s1t=d["s1t"], s0t=d["s0t"], hh=d["hh"], hht=d["hht"], xpre=d["xpre"],
                xpre_t=d["xpre_t"])


# ----------------------------------------------------------------------------------------------------------------------
# reverse (autograd of the forward formulas, in the dtype ``dt``)
# ----------------------------------------------------------------------------------------------------------------------
def ln_reverse(dt, x, t, gamma, beta, gy, gyt):
    """adjoints of x, t, beta and gamma for the adjoints (gy, gyt) of ``ln_dual``'s (y, yt); a residual passes its adjoint on
    unchanged and does not enter"""
    lv = [a.to(dt).clone().requires_grad_(True) for a in (x, t, beta, gamma)]
    y, yt, _, _ = ln_dual(lv[0], lv[1], None, None, lv[3], lv[2])
    gx, gxt, dbeta, dgamma = torch.autograd.grad((gy.to(dt) * y).sum() + (gyt.to(dt) * yt).sum(), lv)
    return dict(gx=gx, gxt=gxt, dbeta=dbeta, dgamma=dgamma)


def node_quotient_reverse(dt, g, gt, s0, hh, s0t, hht):
    """Q1, Q0, Q1t, Q0t: adjoints of s1, s0, s1t, s0t for the adjoints (g, gt) of hh = s1 / (s0 + eps) and
    hht = (s1t - hh * s0t) / (s0 + eps), at the point whose s0, hh, s0t, hht are given"""
    g, gt, s0, hh, s0t, hht = (a.to(dt) for a in (g, gt, s0, hh, s0t, hht))
    d = s0 + EPS_GATE
    lv = [a.clone().requires_grad_(True) for a in (hh * d, s0, hht * d + hh * s0t, s0t)]
    s1, s0_, s1t, s0t_ = lv
    h = s1 / (s0_ + EPS_GATE)
    ht = (s1t - h * s0t_) / (s0_ + EPS_GATE)
    return dict(zip(("Q1", "Q0", "Q1t", "Q0t"), torch.autograd.grad((g * h).sum() + (gt * ht).sum(), lv)))


def reverse(dt, o, u, v, n, H, has_gl):
    """float-``dt`` autograd of <Q1, s1> + <Q0, s0> + <Q1t, s1t> + <Q0t, s0t> and, with ``has_gl``, + <GY, y> + <GYt, yt> of the
    LayerNorm branch (without it the loss has no y or yt terms: the edge output is dead): adjoints GM, GMt of m, mt, of the
    node projections' A | Bd | Bh blocks (GP, GPt [n, 3H]), of the edge bias (gb: column sums of GM) and, with ``has_gl``, of
    the LayerNorm parameters.  m = A[u] + Bd[v] + C enters as the given tensor M plus terms that are zero in value and carry
    the gradient to A and Bd; the same for mt."""
    c = {k: t.to(dt) for k, t in o.items() if torch.is_floating_point(t)}
    names = ("M", "Mt", "P", "Pt") + (("gamma", "beta") if has_gl else ())
    lv = {k: c[k].clone().requires_grad_(True) for k in names}
    A, Bd, _, _ = _blocks(lv["P"], H)
    At, Bdt, _, _ = _blocks(lv["Pt"], H)
    m = lv["M"] + (A[u] - A[u].detach()) + (Bd[v] - Bd[v].detach())
    mt = lv["Mt"] + (At[u] - At[u].detach()) + (Bdt[v] - Bdt[v].detach())
    d = gate_dual(lv["P"], lv["Pt"], m, mt, True, u, v, n, H)
    loss = (c["Q1"] * d["s1"]).sum() + (c["Q0"] * d["s0"]).sum() + (c["Q1t"] * d["s1t"]).sum() + (c["Q0t"] * d["s0t"]).sum()
    if has_gl:
        y, yt, _, _ = ln_dual(m, mt, None, None, lv["gamma"], lv["beta"])
        loss = loss + (c["GY"] * y).sum() + (c["GYt"] * yt).sum()
    gr = dict(zip(names, torch.autograd.grad(loss, [lv[k] for k in names])))
    out = dict(GM=gr["M"], GMt=gr["Mt"], GP=gr["P"][:, :3 * H], GPt=gr["Pt"][:, :3 * H], gb=gr["M"].sum(0))
    if has_gl:
        out.update(dbeta=gr["beta"], dgamma=gr["gamma"])
    return out


# ----------------------------------------------------------------------------------------------------------------------
# operands (float32; what the kernels and both restatements read)
# ----------------------------------------------------------------------------------------------------------------------
def _shape_rows(X, data, gen, v=None):
    """the row distributions (module docstring) applied to a freshly drawn N(0,1) matrix; ``v``: the destination of every row"""
    rows, H = X.shape
    dev = X.device
    row = torch.arange(rows, device=dev)
    if data == "mean_over_spread":
        X = X + 100.0 * (2 * torch.rand(rows, 1, device=dev, generator=gen) - 1)
    elif data == "constant_rows":
        assert H in CONSTANT_ROWS_WIDTHS, "constant_rows: power-of-two widths only (see the module docstring)"
        k = torch.randint(-256, 257, (rows, 1), device=dev, generator=gen).float() / 64
        X = torch.where((row % 3 == 0)[:, None], k.expand(rows, H), X)
    elif data == "rows_1e-4_1e4":
        s = torch.where(row % 3 == 0, 1e-4, 1.0) * torch.where(row % 3 == 1, 1e4, 1.0)
        X = X * s[:, None].float()
    elif data == "saturated_gates":
        X = torch.where((row % 3 == 0)[:, None], torch.sign(X) * (110.0 + 20.0 * X.abs()), X)
        if v is not None:
            seg = (v + 2) % 5
            X = torch.where((seg == 0)[:, None], -(22.0 + 2.0 * X.abs().clamp_max(3.0)), X)
            X = torch.where((seg == 1)[:, None], -(110.0 + 20.0 * X.abs().clamp_max(3.0)), X)
    return X.contiguous()


def _params(H, data, R, which):
    gamma, beta = 1 + 0.2 * R(H), 0.2 * R(H)
    if data == "gamma_zero_negative":
        gamma = torch.where(torch.arange(H, device=gamma.device) % 3 == which, 0.0, 1.0) * R(H)
    return gamma, beta


def saturated_nodes(n, device):
    """mask over the nodes whose whole segments ``saturated_gates`` drives to S0 ~ 1e-9 or S0 = 0"""
    return (torch.arange(n, device=device) + 2) % 5 < 2


def row_operands(rows, H, data, device):
    """Operands of the LayerNorm row kernels: X, Xt, the residual R, Rt, the adjoints GY, GYt, the parameters, and for the reverse
    of the node-level quotient well-conditioned node sums S0 (positive), HH, S0t, HHt."""
    assert data in DATA
    gen = torch.Generator(device=device).manual_seed(zlib.crc32(f"rows {rows} {H} {data}".encode()))
    R = lambda *s: torch.randn(*s, device=device, generator=gen)  # noqa: E731
    o = {k: R(rows, H) for k in ("X", "Xt", "R", "Rt", "GY", "GYt", "HH", "S0t", "HHt")}
    o["S0"] = 0.05 + 4.0 * torch.rand(rows, H, device=device, generator=gen)
    o["gamma"], o["beta"] = _params(H, data, R, 0)
    o["X"] = _shape_rows(o["X"], data, gen)
    return o


def operands(H, g, data, device):
    """Operands of the gate passes on the graph ``g`` (``src``, ``dst`` per row, ``n_nodes``, ``n_edges``): P, Pt; m and mt as the
    float32 tensors M, Mt the reverse passes and the tangent-only forward are handed, and C = M - A[u] - Bd[v] in float32 (Ct the
    same), so that what the forward forms itself is M up to one rounding; residuals R, Rt and adjoints GY, GYt of the edge
    LayerNorm branch; residuals XR, XRt and adjoints GX, GXt of the node LayerNorm; the parameters of both."""
    assert data in DATA
    n, m = g.n_nodes, g.n_edges
    u, v = g.src.long().to(device), g.dst.long().to(device)
    gen = torch.Generator(device=device).manual_seed(zlib.crc32(f"{H} {n} {m} {data}".encode()))
    R = lambda *s: torch.randn(*s, device=device, generator=gen)  # noqa: E731
    o = {k: R(n, 4 * H) for k in ("P", "Pt")}
    o.update({k: R(m, H) for k in ("M", "Mt", "R", "Rt", "GY", "GYt")})
    o.update({k: R(n, H) for k in ("XR", "XRt", "GX", "GXt")})
    o["gamma"], o["beta"] = _params(H, data, R, 0)
    o["n_gamma"], o["n_beta"] = _params(H, data, R, 1)
    o["M"] = _shape_rows(o["M"], data, gen, v)
    A, Bd, _, _ = _blocks(o["P"], H)
    At, Bdt, _, _ = _blocks(o["Pt"], H)
    o["C"] = (o["M"] - A[u] - Bd[v]).contiguous()
    o["Ct"] = (o["Mt"] - At[u] - Bdt[v]).contiguous()
    return o


# ----------------------------------------------------------------------------------------------------------------------
# whole cases: every output the parity tests compare, from one set of operands
# ----------------------------------------------------------------------------------------------------------------------
def row_case(dt, o, res):
    """The LayerNorm row kernels on ``row_operands``: forward (y, yt, mean, rstd), reverse (gx, gxt, dbeta, dgamma) and the
    reverse of the node-level quotient at that (gx, gxt)."""
    c = {k: t.to(dt) for k, t in o.items()}
    y, yt, mean, rstd = ln_dual(c["X"], c["Xt"], c["R"] if res else None, c["Rt"] if res else None, c["gamma"], c["beta"])
    out = dict(y=y, yt=yt, mean=mean, rstd=rstd)
    out.update(ln_reverse(dt, c["X"], c["Xt"], c["gamma"], c["beta"], c["GY"], c["GYt"]))
    out.update(node_quotient_reverse(dt, out["gx"], out["gxt"], c["S0"], c["HH"], c["S0t"], c["HHt"]))
    return out


HANDED = ("s0", "hh", "s0t", "hht", "xpre", "xpre_t", "n_stat", "e_stat", "gx", "gxt", "Q1", "Q0", "Q1t", "Q0t", "GL", "GLt")


def gate_case(dt, o, u, v, n, H, handed=None):
    """One convolution on ``operands`` in the dtype ``dt``, pass by pass as ff2.py chains the kernels: the gate forward from C, Ct;
    the edge LayerNorm of M, Mt (residual R, Rt) and its reverse for (GY, GYt); the node LayerNorm of the pre-activations
    (residual XR, XRt), its reverse for (GX, GXt), the reverse of the node-level quotient; the gate reverse with and without the
    LayerNorm branch.  Every later pass reads what the earlier ones wrote as float32 tensors - ``handed`` (keys HANDED): the
    float64 results rounded once, which the float64 run returns under "handed" and the float32 run and the kernels are given, so
    that all three read identical operands."""
    c = {k: t.to(dt) for k, t in o.items()}
    f = gate_dual(c["P"], c["Pt"], c["C"], c["Ct"], False, u, v, n, H)
    out = {k: f[k] for k in ("m", "mt", "s0", "hh", "s0t", "hht", "xpre", "xpre_t")}
    out["e_y"], out["e_yt"], e_mean, e_rstd = ln_dual(c["M"], c["Mt"], c["R"], c["Rt"], c["gamma"], c["beta"])
    out["e_stat"] = torch.stack([e_mean, e_rstd], 1)
    first = handed is None
    if first:
        handed = {k: out[k].float().contiguous() for k in ("s0", "hh", "s0t", "hht", "xpre", "xpre_t", "e_stat")}
    h = lambda k: handed[k].to(dt)  # noqa: E731
    out["n_y"], out["n_yt"], n_mean, n_rstd = ln_dual(h("xpre"), h("xpre_t"), c["XR"], c["XRt"], c["n_gamma"], c["n_beta"])
    out["n_stat"] = torch.stack([n_mean, n_rstd], 1)
    nrev = ln_reverse(dt, h("xpre"), h("xpre_t"), c["n_gamma"], c["n_beta"], c["GX"], c["GXt"])
    out.update(gx=nrev["gx"], gxt=nrev["gxt"], n_dbeta=nrev["dbeta"], n_dgamma=nrev["dgamma"])
    erev = ln_reverse(dt, c["M"], c["Mt"], c["gamma"], c["beta"], c["GY"], c["GYt"])
    out.update(GL=erev["gx"], GLt=erev["gxt"], e_dbeta=erev["dbeta"], e_dgamma=erev["dgamma"])
    if first:
        handed.update({k: out[k].float().contiguous() for k in ("n_stat", "gx", "gxt", "GL", "GLt")})
    q = node_quotient_reverse(dt, h("gx"), h("gxt"), h("s0"), h("hh"), h("s0t"), h("hht"))
    out.update(q)
    if first:
        handed.update({k: q[k].float().contiguous() for k in q})
    oq = dict(o)
    oq.update({k: handed[k] for k in ("Q1", "Q0", "Q1t", "Q0t")})
    for has_gl, tag in ((True, "gl_"), (False, "nogl_")):
        r = reverse(dt, oq, u, v, n, H, has_gl)
        out.update({tag + k: t for k, t in r.items()})
    assert set(handed) == set(HANDED)
    out["handed"] = handed
    return out


# ----------------------------------------------------------------------------------------------------------------------
# the cases of tests/test_gpu_dual_f64.py (tests/test_dual_ref.py holds every one of them it can build without a GPU to the cap)
# ----------------------------------------------------------------------------------------------------------------------
GATE_CASES = ([(H, gname, "normal") for H in (4, 36, 64, 256, 260, 512, 1024)
               for gname in ("synthetic", "bond", "lg_small", "lg_deg17", "one_atom_cell", "one_segment", "no_edges")]
              + [(H, gname, data) for data in DATA[1:] for H in ((64, 512) if data == "constant_rows" else (64, 260, 512))
                 for gname in ("synthetic", "lg_small")]
              + [(64, "lg_4096seg", "normal")])
ROW_WIDTHS = (4, 36, 64, 252, 256, 260, 508, 512, 516, 768, 1020, 1024)
ROW_CASES = ([(rows, Fw, "normal") for rows in (1, 3, 5) for Fw in ROW_WIDTHS]
             + [(rows, Fw, "normal") for rows in (4097, 9001) for Fw in (64, 260, 1024)]  # a wave owns two or three rows
             + [(rows, Fw, data) for data in DATA[1:] for rows, Fw in ((5, 64), (5, 512), (4097, 64))]
             + [(5, 1024, "constant_rows")])
REVERSE_FLOORED = ("GM", "GMt", "GP", "GPt", "gb")  # compared with a floor of 1e-2 of the largest node gradient


def reverse_parts(data, n, v):
    """[(suffix, mask over the edge rows, mask over the node rows)]: the rows over which the errors of Q1 .. Q0t and of what is
    downstream of them are taken - all at once, but with ``saturated_gates`` the rows of the nodes whose 1 / (S0 + eps) is near
    1e6 (edge rows: by destination) and the rest separately, or the former's scale would mask the latter."""
    if data != "saturated_gates":
        return [("", None, None)]
    sat = saturated_nodes(n, v.device)
    return [(" sat", sat[v], sat), (" rest", ~sat[v], ~sat)]


def part(t, mask):
    return t if mask is None else t[mask]


def reverse_floors(r, tag, nm):
    """floors of the gate reverse's outputs (tag "gl_" / "nogl_" of ``gate_case``) over the node rows ``nm``"""
    fl = 1e-2 * float(part(r[tag + "GP"], nm).abs().max()) if r[tag + "GP"].numel() else 0.0
    flt = 1e-2 * float(part(r[tag + "GPt"], nm).abs().max()) if r[tag + "GPt"].numel() else 0.0
    return dict(GM=max(fl, 1e-30), GP=max(fl, 1e-30), gb=max(fl, 1e-30), GMt=max(flt, 1e-30), GPt=max(flt, 1e-30))
