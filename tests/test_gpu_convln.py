"""csrc/convln.hip - the line-graph and bond-graph convolutions of ALIGNNAtomWise with the edge LayerNorm formed inside the
gate passes - against float64 restatements (tests/dual_ref.py) of alignn/models/alignn_atomwise.py:151-208, entry point by entry point and
output by output.  tests/test_gpu_dual.py compares these kernels with the separate HIP kernels they replace (which pins the
summation order, but lets a formula shared by both pass); here the other side is ``index_add`` / ``layer_norm`` / ``silu`` /
``sigmoid`` in float64, explicit value + tangent expressions for the dual passes (validated by central differences), and
float64 autograd of those expressions for the reverse passes.

Tolerances.  On N(0,1) operands: the bounds tests/test_gpu_dual.py asserts for the separate kernels against float64 - 2e-6
for what a LayerNorm forward writes, 2e-5 for what a gate forward writes and for the LayerNorm parameter gradients, 5e-5 (with
its floor of 1e-2 of the largest node gradient) for what a gate reverse writes.  On every other data distribution the SAME
restatement is evaluated in float32 on the identical float32 operands; the kernel may be 4x as far from float64 as that
(the margin tests/test_gpu_kernels.py::test_gemm_x6_accuracy gives a reordered fp32 sum), plus the N(0,1) bound as a floor.
Errors are max |a - b| / max |b| over the whole tensor (tests/helpers.rel_err); no element, row or case is left out.

An ``amax`` output (zeroed before the launch) must EQUAL the largest magnitude among the elements the launch wrote: the next
f16x3 product takes its power-of-two scale from it, and a value too small overflows the fp16 slices silently."""

import zlib

import pytest
import torch

pytestmark = pytest.mark.gpu

from alignn_amd import _lib  # noqa: E402
from alignn_amd._lib import stream  # noqa: E402
from tests.dual_ref import _blocks, _duals, _values  # noqa: E402  (the restatements, any dtype)
from tests.gate_parity import Report as _Report  # noqa: E402
from tests.gate_parity import err as _err  # noqa: E402
from tests.gate_parity import gptr, guard_graph, guard_input, guarded  # noqa: E402
from tests.gate_parity import graph as _graph  # noqa: E402
from tests.gate_parity import is_line_graph as _is_line_graph  # noqa: E402

DEV = "cuda"
EPS, EPS_GATE = 1e-5, 1e-6  # nn.LayerNorm's default; ALIGNN_EPS_GATE (csrc/common.h)
INVALID = 1  # hipErrorInvalidValue
HS = (4, 36, 64, 100, 128, 252, 256)
DATA = ("normal", "mean_over_spread", "constant_rows", "rows_1e-4_1e4", "gamma_zero_negative")
# bounds on N(0,1) operands (see the module docstring) and floors of everything else
B_LN_FWD, B_GATE_FWD, B_LN_PARAM, B_REVERSE = 2e-6, 2e-5, 2e-5, 5e-5


# ----------------------------------------------------------------------------------------------------------------------
# operands (float32, on the device: what the kernels and both restatements read)
# ----------------------------------------------------------------------------------------------------------------------
def _operands(H, gname, data):
    g = _graph(gname)
    n, m = g.n_nodes, g.n_edges
    gen = torch.Generator(device=DEV).manual_seed(zlib.crc32(f"{H} {gname} {data}".encode()))
    R = lambda *s: torch.randn(*s, device=DEV, generator=gen)  # noqa: E731
    o = {k: R(n, 4 * H) for k in ("P", "Pt")}
    o.update({k: R(m, H) for k in ("M", "Mt", "Ct", "Y", "Rt", "GY", "GYt")})
    o.update({k: R(n, H) for k in ("Q1", "Q0", "Q1t", "Q0t")})
    o["gamma"], o["beta"] = 1 + 0.2 * R(H), 0.2 * R(H)
    row = torch.arange(m, device=DEV)
    if data == "mean_over_spread":  # row means up to 1e2 spreads
        o["M"] = o["M"] + 100.0 * (2 * torch.rand(m, 1, device=DEV, generator=gen) - 1)
    elif data == "constant_rows":  # variance exactly 0 in every third row
        c = R(m, 1).expand(m, H)
        o["M"] = torch.where((row % 3 == 0)[:, None], c, o["M"]).contiguous()
    elif data == "rows_1e-4_1e4":
        s = torch.where(row % 3 == 0, 1e-4, 1.0) * torch.where(row % 3 == 1, 1e4, 1.0)
        o["M"] = o["M"] * s[:, None].float()
    elif data == "gamma_zero_negative":
        o["gamma"] = torch.where(torch.arange(H, device=DEV) % 3 == 0, 0.0, 1.0) * R(H)
    return g, o


def _forward_ref(dt, g, o, H):
    u, v, n = g.src.long(), g.dst.long(), g.n_nodes
    c = {k: t.to(dt) for k, t in o.items()}
    f = _values(c["P"], c["M"], c["gamma"], c["beta"], u, v, n, H)
    At, Bdt, _, _ = _blocks(c["Pt"], H)
    mt = At[u] + Bdt[v] + c["Ct"]
    d = _duals(c["P"], c["Pt"], c["M"], mt, c["gamma"], c["beta"], u, v, n, H)
    return dict(y=f["y"], y_res=f["y"] + c["Y"], mean=f["mean"], rstd=f["rstd"], xpre=f["xpre"], s0=f["s0"], hh=f["hh"], mt=mt,
                xpre_t=d["xpre_t"], s0t=d["s0t"], hht=d["hht"], yt=d["yt"], yt_res=d["yt"] + c["Rt"])


def _reverse_ref(dt, g, o, H, dual):
    """float-``dt`` autograd of the restatements: adjoints of m (and mt), of the node projections' A / Bd / Bh blocks, of the
    edge bias (column sums of the adjoint of m) and of the LayerNorm parameters, for the adjoints GY (GYt) of the LayerNorm
    branch and Q1, Q0 (Q1t, Q0t) of the segment sums.  m = A[u] + Bd[v] + C enters as the given tensor M plus terms that are
    zero in value and carry the gradient to A and Bd."""
    u, v, n = g.src.long(), g.dst.long(), g.n_nodes
    c = {k: t.to(dt) for k, t in o.items()}
    leaves = {k: c[k].clone().requires_grad_(True) for k in ("M", "Mt", "P", "Pt", "gamma", "beta")}
    A, Bd, _, _ = _blocks(leaves["P"], H)
    At, Bdt, _, _ = _blocks(leaves["Pt"], H)
    m = leaves["M"] + (A[u] - A[u].detach()) + (Bd[v] - Bd[v].detach())
    if dual:
        mt = leaves["Mt"] + (At[u] - At[u].detach()) + (Bdt[v] - Bdt[v].detach())
        d = _duals(leaves["P"], leaves["Pt"], m, mt, leaves["gamma"], leaves["beta"], u, v, n, H)
        loss = ((c["GY"] * d["y"]).sum() + (c["GYt"] * d["yt"]).sum() + (c["Q1"] * d["s1"]).sum() + (c["Q0"] * d["s0"]).sum()
                + (c["Q1t"] * d["s1t"]).sum() + (c["Q0t"] * d["s0t"]).sum())
        names = ("M", "Mt", "P", "Pt", "gamma", "beta")
    else:
        f = _values(leaves["P"], m, leaves["gamma"], leaves["beta"], u, v, n, H)
        loss = (c["GY"] * f["y"]).sum() + (c["Q1"] * f["s1"]).sum() + (c["Q0"] * f["s0"]).sum()
        names = ("M", "P", "gamma", "beta")
    gr = dict(zip(names, torch.autograd.grad(loss, [leaves[k] for k in names])))
    out = dict(GM=gr["M"], GP=gr["P"][:, :3 * H], GP_bd=gr["P"][:, H:2 * H], gb=gr["M"].sum(0), dbeta=gr["beta"], dgamma=gr["gamma"])
    if dual:
        out.update(GMt=gr["Mt"], GPt=gr["Pt"][:, :3 * H], GPt_bd=gr["Pt"][:, H:2 * H])
    return out


def _run_case(H, gname, data):
    rep = _Report(f"H={H} {gname} {data}")
    lib = rep.launcher(_lib.load())
    # every buffer a launch is handed lies between guard bands (tests/gate_parity.Guards; rep.finish() checks them first), the
    # graph's tables and the operands as guarded copies, and every pointer goes through gptr, which refuses any other tensor
    g, o = _operands(H, gname, data)
    g, o = guard_graph(g), {k: guard_input(t, k) for k, t in o.items()}
    n, m = g.n_nodes, g.n_edges
    st = stream()
    other = data != "normal"
    E = lambda *s: guarded(s, row=H)  # noqa: E731  (an output: a NaN in whatever is not written)
    Z = lambda *s: guarded(s, fill=0.0, row=H)  # noqa: E731
    G = lambda t: guard_input(t.contiguous())  # noqa: E731  (a tensor made here, handed to a launch)
    P, Pt, M, gamma, beta = o["P"], o["Pt"], o["M"], o["gamma"], o["beta"]

    # ---- forward values and tangents
    r64 = _forward_ref(torch.float64, g, o, H)
    r32 = _forward_ref(torch.float32, g, o, H) if other else {}
    f32 = lambda k: r32.get(k)  # noqa: E731
    for res in (False, True):
        xpre, s0, hh, yout, stat, am = E(n, H), E(n, H), E(n, H), E(m, H), E(m, 2), Z(1)
        assert lib.alignn_egc_gate_fwd_pre_ln(gptr(P), gptr(M), gptr(g.seg_ptr), gptr(g.seg_node), gptr(g.src), n, m, H, gptr(xpre), gptr(s0),
                                              gptr(hh), gptr(gamma), gptr(beta), EPS, gptr(o["Y"]) if res else None, gptr(yout), gptr(stat),
                                              gptr(am), st) == 0
        torch.cuda.synchronize()
        ent = "gate_fwd_pre_ln" + (" +Y" if res else "")
        k = "y_res" if res else "y"
        rep.close(ent, "YOUT", yout, r64[k], f32(k), B_LN_FWD)
        rep.close(ent, "mean", stat[:, 0], r64["mean"], f32("mean"), B_LN_FWD)
        rep.close(ent, "rstd", stat[:, 1], r64["rstd"], f32("rstd"), B_LN_FWD)
        rep.close(ent, "XPRE", xpre, r64["xpre"], f32("xpre"), B_GATE_FWD)
        rep.close(ent, "S0", s0, r64["s0"], f32("s0"), B_GATE_FWD)
        rep.close(ent, "HH", hh, r64["hh"], f32("hh"), B_GATE_FWD)
        rep.amax(ent, "y_amax", am[0], yout)
    # (what the later passes are handed: the float64 statistics and node sums, rounded once)
    e_stat = G(torch.stack([r64["mean"], r64["rstd"]], 1).float())
    s0_in, hh_in = G(r64["s0"].float()), G(r64["hh"].float())
    for res in (False, True):
        mt, xpre_t, s0t, hht, yt, am2 = G(o["Ct"]), E(n, H), E(n, H), E(n, H), E(m, H), Z(2)
        assert lib.alignn_egc_gate_dual_tan_ln(gptr(P), gptr(Pt), gptr(M), gptr(mt), gptr(g.seg_ptr), gptr(g.seg_node), gptr(g.src), n, m, H,
                                               gptr(xpre_t), gptr(s0_in), gptr(hh_in), gptr(s0t), gptr(hht), gptr(gamma), gptr(beta), gptr(e_stat),
                                               gptr(o["Rt"]) if res else None, gptr(yt), gptr(am2), st) == 0
        torch.cuda.synchronize()
        ent = "gate_dual_tan_ln" + (" +Rt" if res else "")
        k = "yt_res" if res else "yt"
        rep.close(ent, "Mt", mt, r64["mt"], f32("mt"), B_LN_FWD)
        rep.close(ent, "xpre_t", xpre_t, r64["xpre_t"], f32("xpre_t"), B_GATE_FWD)
        rep.close(ent, "s0t", s0t, r64["s0t"], f32("s0t"), B_GATE_FWD)
        rep.close(ent, "hht", hht, r64["hht"], f32("hht"), B_GATE_FWD)
        rep.close(ent, "Yt", yt, r64[k], f32(k), B_LN_FWD)
        rep.amax(ent, "amax2[0]", am2[0], torch.zeros(0))  # (a tangent-only pass writes no values)
        rep.amax(ent, "amax2[1]", am2[1], yt)
    del r64, r32

    # ---- reverse passes
    v64 = _reverse_ref(torch.float64, g, o, H, dual=False)
    v32 = _reverse_ref(torch.float32, g, o, H, dual=False) if other else {}
    d64 = _reverse_ref(torch.float64, g, o, H, dual=True)
    d32 = _reverse_ref(torch.float32, g, o, H, dual=True) if other else {}
    Mt, GY, GYt, Q1, Q0, Q1t, Q0t = (o[k] for k in ("Mt", "GY", "GYt", "Q1", "Q0", "Q1t", "Q0t"))

    def reverse_asserts(ent, ref, r32_, GM, GP, gb, red, gp_key, GMt=None, GPt=None):
        fl = 1e-2 * float(ref["GP"].abs().max())
        rep.close(ent, "GM", GM, ref["GM"], r32_.get("GM"), B_REVERSE, fl)
        rep.close(ent, gp_key, GP, ref[gp_key], r32_.get(gp_key), B_REVERSE, fl)
        rep.close(ent, "gb", gb.sum(0), ref["gb"], r32_.get("gb"), B_REVERSE, fl)
        rep.close(ent, "dbeta", red[0], ref["dbeta"], r32_.get("dbeta"), B_LN_PARAM)
        rep.close(ent, "dgamma", red[1], ref["dgamma"], r32_.get("dgamma"), B_LN_PARAM)
        if GMt is not None:
            flt = 1e-2 * float(ref["GPt"].abs().max())
            kt = gp_key.replace("GP", "GPt")
            rep.close(ent, "GMt", GMt, ref["GMt"], r32_.get("GMt"), B_REVERSE, flt)
            rep.close(ent, kt, GPt, ref[kt], r32_.get(kt), B_REVERSE, flt)

    # destination-ordered halves (any CSR), then the unchanged source-ordered halves
    slabs = lib.alignn_egc_ln_dst_slabs(n)
    GM, GP, gb, lnp, red, gma, gpa = E(m, H), Z(n, 4 * H), E(slabs, H), E(slabs, 2, H), E(2, H), Z(1), Z(1)
    assert lib.alignn_egc_bwd_dst_ln(gptr(GY), gptr(M), gptr(P), gptr(Q1), gptr(Q0), gptr(gamma), gptr(beta), gptr(e_stat), gptr(g.seg_ptr),
                                     gptr(g.seg_node), gptr(g.src), n, H, gptr(GM), gptr(GP), gptr(gb), gptr(lnp), gptr(gma), gptr(gpa), st) == 0
    assert lib.alignn_bn_bwd_finalize(gptr(lnp), slabs, H, gptr(red), st) == 0
    torch.cuda.synchronize()
    assert float(GP[:, :H].abs().max()) == 0.0 and float(GP[:, 2 * H:].abs().max()) == 0.0  # (this half writes the Bd block only)
    reverse_asserts("bwd_dst_ln", v64, v32, GM, GP[:, H:2 * H], gb, red, "GP_bd")
    rep.amax("bwd_dst_ln", "gm_amax", gma[0], GM)
    rep.amax("bwd_dst_ln", "gp_amax", gpa[0], GP[:, H:2 * H])
    assert lib.alignn_egc_bwd_src(gptr(GM), gptr(M), gptr(Q1), gptr(g.out_ptr), gptr(g.out_slot), gptr(g.dst), n, H, gptr(GP), None, st) == 0
    torch.cuda.synchronize()
    fl = 1e-2 * float(v64["GP"].abs().max())
    rep.close("bwd_dst_ln + bwd_src", "GP", GP[:, :3 * H], v64["GP"], v32.get("GP"), B_REVERSE, fl)

    GM, GMt, GP, GPt, gma, gpa = E(m, H), E(m, H), Z(n, 4 * H), Z(n, 4 * H), Z(2), Z(2)
    assert lib.alignn_egc_dual_bwd_dst_ln(gptr(GY), gptr(GYt), gptr(M), gptr(Mt), gptr(P), gptr(Pt), gptr(Q1), gptr(Q0), gptr(Q1t), gptr(Q0t),
                                          gptr(gamma), gptr(beta), gptr(e_stat), gptr(g.seg_ptr), gptr(g.seg_node), gptr(g.src), n, H, gptr(GM),
                                          gptr(GMt), gptr(GP), gptr(GPt), gptr(gb), gptr(lnp), gptr(gma), gptr(gpa), st) == 0
    assert lib.alignn_bn_bwd_finalize(gptr(lnp), slabs, H, gptr(red), st) == 0
    torch.cuda.synchronize()
    reverse_asserts("dual_bwd_dst_ln", d64, d32, GM, GP[:, H:2 * H], gb, red, "GP_bd", GMt, GPt[:, H:2 * H])
    for w, (a, b) in enumerate(((GM, GP), (GMt, GPt))):
        rep.amax("dual_bwd_dst_ln", f"gm_amax2[{w}]", gma[w], a)
        rep.amax("dual_bwd_dst_ln", f"gp_amax2[{w}]", gpa[w], b[:, H:2 * H])
    assert lib.alignn_egc_dual_bwd_src(gptr(GM), gptr(GMt), gptr(M), gptr(Mt), gptr(Q1), gptr(Q1t), gptr(g.out_ptr), gptr(g.out_slot), gptr(g.dst),
                                       n, H, gptr(GP), gptr(GPt), None, st) == 0
    torch.cuda.synchronize()
    rep.close("dual_bwd_dst_ln + dual_bwd_src", "GP", GP[:, :3 * H], d64["GP"], d32.get("GP"), B_REVERSE, fl)
    rep.close("dual_bwd_dst_ln + dual_bwd_src", "GPt", GPt[:, :3 * H], d64["GPt"], d32.get("GPt"), B_REVERSE,
              1e-2 * float(d64["GPt"].abs().max()))

    # dense-block kernels (line graphs)
    if _is_line_graph(g):
        groups = g.grp_seg_ptr.numel() - 1
        GM, GP, gb, lnp, gma, gpa = E(m, H), Z(n, 4 * H), E(groups, H), E(groups, 2, H), Z(1), Z(1)
        assert lib.alignn_egc_bwd_lg_dense_ln(gptr(GY), gptr(M), gptr(P), gptr(Q1), gptr(Q0), gptr(gamma), gptr(beta), gptr(e_stat), m,
                                              gptr(g.grp_seg_ptr), gptr(g.grp_src_ptr), groups, g.dense_max_src, gptr(g.seg_ptr),
                                              gptr(g.seg_node), H, gptr(GM), gptr(GP), gptr(gb), gptr(lnp), gptr(gma), gptr(gpa), st) == 0
        assert lib.alignn_bn_bwd_finalize(gptr(lnp), groups, H, gptr(red), st) == 0
        torch.cuda.synchronize()
        ent = "bwd_lg_dense_ln"
        reverse_asserts(ent, v64, v32, GM, GP[:, :3 * H], gb, red, "GP")
        assert float(GP[:, 3 * H:].abs().max()) == 0.0
        rep.amax(ent, "gm_amax", gma[0], GM)
        rep.amax(ent, "gp_amax", gpa[0], GP)
        GM, GMt, GP, GPt, gma, gpa = E(m, H), E(m, H), Z(n, 4 * H), Z(n, 4 * H), Z(2), Z(2)
        assert lib.alignn_egc_dual_bwd_lg_dense_ln(gptr(GY), gptr(GYt), gptr(M), gptr(Mt), gptr(P), gptr(Pt), gptr(Q1), gptr(Q0), gptr(Q1t),
                                                   gptr(Q0t), gptr(gamma), gptr(beta), gptr(e_stat), m, gptr(g.grp_seg_ptr),
                                                   gptr(g.grp_src_ptr), groups, gptr(g.seg_ptr), gptr(g.seg_node), H, gptr(GM), gptr(GMt),
                                                   gptr(GP), gptr(GPt), gptr(gb), gptr(lnp), gptr(gma), gptr(gpa), st) == 0
        assert lib.alignn_bn_bwd_finalize(gptr(lnp), groups, H, gptr(red), st) == 0
        torch.cuda.synchronize()
        ent = "dual_bwd_lg_dense_ln"
        reverse_asserts(ent, d64, d32, GM, GP[:, :3 * H], gb, red, "GP", GMt, GPt[:, :3 * H])
        for w, (a, b) in enumerate(((GM, GP), (GMt, GPt))):
            rep.amax(ent, f"gm_amax2[{w}]", gma[w], a)
            rep.amax(ent, f"gp_amax2[{w}]", gpa[w], b)
    rep.finish()


SMALL = ("lg_small", "lg_deg17", "bond", "synthetic")
CASES = ([(H, gname, "normal") for H in HS for gname in SMALL]
         + [(H, gname, data) for H in (100, 256) for gname in ("lg_small", "synthetic") for data in DATA[1:]]
         + [(64, "lg_4096seg", "normal"), (252, "lg_4096seg", "mean_over_spread"),
            (256, "lg_stream", "normal"), (256, "lg_stream", "rows_1e-4_1e4")])


@pytest.mark.parametrize("H,gname,data", CASES)
def test_entry_points_against_float64(H, gname, data):
    """Every output of the six entry points of csrc/convln.hip against the float64 restatements: on line graphs all six, on other graphs the forward, the dual forward and the
    two destination-ordered reverse passes (completed by the source-ordered halves).  See the module docstring for the
    bounds; the worst error per entry point and output is printed."""
    _run_case(H, gname, data)


@pytest.mark.parametrize("H,gname", [(36, "lg_small"), (64, "synthetic")])
def test_the_restatements_are_consistent(H, gname):
    """The explicit value + tangent expressions: same values as the layer_norm / silu / index_add restatement, and tangents
    that ARE the directional derivative (central differences, the tolerances of tests/test_gpu_dual.py)."""
    g, o = _operands(H, gname, "normal")
    u, v, n = g.src.long(), g.dst.long(), g.n_nodes
    c = {k: t.double() for k, t in o.items()}
    args = (c["gamma"], c["beta"], u, v, n, H)
    d = _duals(c["P"], c["Pt"], c["M"], c["Mt"], *args)
    f = _values(c["P"], c["M"], *args)
    for k in ("y", "s1", "s0", "hh", "xpre"):
        assert _err(d[k], f[k]) < 1e-12, k
    h = 1e-6
    fp, fm = (_values(c["P"] + s * h * c["Pt"], c["M"] + s * h * c["Mt"], *args) for s in (1, -1))
    for k, kt, tol in (("y", "yt", 1e-7), ("s1", "s1t", 1e-7), ("s0", "s0t", 1e-7), ("hh", "hht", 1e-6), ("xpre", "xpre_t", 1e-6)):
        assert _err(d[kt], (fp[k] - fm[k]) / (2 * h)) < tol, kt


@pytest.mark.parametrize("H", [0, 2, 6, 260])
def test_unsupported_widths_are_refused(H):
    """hipErrorInvalidValue and no launch (every output buffer keeps its fill) at widths outside H % 4 == 0, 4 <= H <= 256."""
    rep = _Report(f"refusals H={H}")
    lib = rep.launcher(_lib.load())
    g = guard_graph(_graph("lg_small"))
    n, m, W = g.n_nodes, g.n_edges, 264
    groups = g.grp_seg_ptr.numel() - 1
    st = stream()
    I = lambda *s: guard_input(torch.randn(*s, device=DEV))  # noqa: E731, E741
    P, Pt, M, Mt, Y = I(n, 4 * W), I(n, 4 * W), I(m, W), I(m, W), I(m, W)
    q = [I(n, W) for _ in range(4)]
    gamma, beta, e_stat = I(W), I(W), I(m, 2)
    mt_before = Mt.clone()
    outs = [guarded(s, fill=7.0, row=W) for s in ((m, W), (m, W), (n, 4 * W), (n, 4 * W), (n, W), (n, W), (n, W), (1024, W),
                                                       (1024, 2, W), (m, 2), (2,), (2,))]
    em, emt, gp, gpt, na, nb, nc, gb, lnp, stat, am, am_b = outs
    rc = [
        lib.alignn_egc_gate_fwd_pre_ln(gptr(P), gptr(M), gptr(g.seg_ptr), gptr(g.seg_node), gptr(g.src), n, m, H, gptr(na), gptr(nb), gptr(nc),
                                       gptr(gamma), gptr(beta), EPS, gptr(Y), gptr(em), gptr(stat), gptr(am), st),
        lib.alignn_egc_gate_dual_tan_ln(gptr(P), gptr(Pt), gptr(M), gptr(Mt), gptr(g.seg_ptr), gptr(g.seg_node), gptr(g.src), n, m, H, gptr(na),
                                        gptr(q[0]), gptr(q[1]), gptr(nb), gptr(nc), gptr(gamma), gptr(beta), gptr(e_stat), gptr(Y), gptr(em),
                                        gptr(am), st),
        lib.alignn_egc_bwd_lg_dense_ln(gptr(Y), gptr(M), gptr(P), gptr(q[0]), gptr(q[1]), gptr(gamma), gptr(beta), gptr(e_stat), m,
                                       gptr(g.grp_seg_ptr), gptr(g.grp_src_ptr), groups, g.dense_max_src, gptr(g.seg_ptr), gptr(g.seg_node), H,
                                       gptr(em), gptr(gp), gptr(gb), gptr(lnp), gptr(am), gptr(am_b), st),
        lib.alignn_egc_dual_bwd_lg_dense_ln(gptr(Y), gptr(Y), gptr(M), gptr(Mt), gptr(P), gptr(Pt), *(gptr(t) for t in q), gptr(gamma),
                                            gptr(beta), gptr(e_stat), m, gptr(g.grp_seg_ptr), gptr(g.grp_src_ptr), groups, gptr(g.seg_ptr),
                                            gptr(g.seg_node), H, gptr(em), gptr(emt), gptr(gp), gptr(gpt), gptr(gb), gptr(lnp), gptr(am),
                                            gptr(am_b), st),
        lib.alignn_egc_bwd_dst_ln(gptr(Y), gptr(M), gptr(P), gptr(q[0]), gptr(q[1]), gptr(gamma), gptr(beta), gptr(e_stat), gptr(g.seg_ptr),
                                  gptr(g.seg_node), gptr(g.src), n, H, gptr(em), gptr(gp), gptr(gb), gptr(lnp), gptr(am), gptr(am_b), st),
        lib.alignn_egc_dual_bwd_dst_ln(gptr(Y), gptr(Y), gptr(M), gptr(Mt), gptr(P), gptr(Pt), *(gptr(t) for t in q), gptr(gamma), gptr(beta),
                                       gptr(e_stat), gptr(g.seg_ptr), gptr(g.seg_node), gptr(g.src), n, H, gptr(em), gptr(emt), gptr(gp),
                                       gptr(gpt), gptr(gb), gptr(lnp), gptr(am), gptr(am_b), st),
    ]
    torch.cuda.synchronize()
    assert rc == [INVALID] * 6, rc
    assert all(bool((t == 7.0).all()) for t in outs) and torch.equal(Mt, mt_before)
    assert lib.alignn_egc_ln_fused_supported(H, 1 << 30) == 0 and lib.alignn_egc_ln_dst_supported(H) == 0
    rep.finish()  # (and nothing beside the outputs either)
