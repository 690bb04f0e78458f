"""csrc/dual.hip - the dual-number (value + tangent) kernels behind force and stress training, the only path of every model wider
than 256 features and the default one of every small line graph - against the float64 restatements of tests/dual_ref.py, entry
point by entry point and output by output.  tests/test_gpu_dual.py compares these kernels with each other and with whole-model
runs (which pins the summation order, but lets a formula or a row arithmetic shared by two kernels pass); here the other side is
``layer_norm`` / ``silu`` / ``sigmoid`` / ``index_add`` in float64 with explicit tangents (validated by central differences in
tests/test_dual_ref.py), and float64 autograd of those expressions for every reverse pass.

Tolerances: the project's own, as in tests/test_gpu_convln.py.  On N(0,1) operands 2e-6 for what a LayerNorm forward writes (and for
m, mt = A[u] + Bd[v] + C, three roundings), 2e-5 for what a gate forward writes, for the adjoints Q1 .. Q0t of the node sums, for
the LayerNorm parameter gradients and the LayerNorm input gradients (the bound tests/test_gpu_dual.py asserts for them), 5e-5 with
a floor of 1e-2 of the largest node gradient for what a gate reverse writes.  On every other distribution the SAME restatement
is evaluated in float32 on the identical float32 operands and the kernel may be 4x as far from float64 as that, plus the N(0,1)
bound; tests/test_dual_ref.py holds that float32 error below 1e-4 on every case.  Errors are max |a - b| / max |b| over a whole
tensor; no element, row or case is left out.  Later passes are handed the float64 results of the earlier ones rounded once.  With
``saturated_gates`` the errors of Q1 .. Q0t and of what a gate reverse writes are taken separately over the rows of the nodes
whose 1 / (S0 + eps) is near 1e6 and over the rest (dual_ref.reverse_parts).

An ``amax`` slot zeroed before a launch must EQUAL the largest magnitude that launch wrote, and a slot already above it must be
left as it is: the next f16x3 product takes its power-of-two scale from it."""

import pytest
import torch

pytestmark = pytest.mark.gpu

from alignn_amd import _lib  # noqa: E402
from alignn_amd._lib import stream  # noqa: E402
from tests import dual_ref as D  # noqa: E402
from tests.gate_parity import Report, gptr, graph, guard_graph, guard_input, guarded, is_line_graph  # noqa: E402

DEV = "cuda"
INVALID = 1  # hipErrorInvalidValue
FILL = 7.0
ABOVE = 2.0 ** 100  # an amax slot that already holds more than any launch here writes
B_LN_FWD, B_GATE_FWD, B_LN_PARAM, B_LN_INPUT, B_REVERSE = 2e-6, 2e-5, 2e-5, 2e-5, 5e-5
F64, F32 = torch.float64, torch.float32


# Every buffer a launch is handed lies between guard bands (tests/gate_parity.Guards; Report.finish checks them first) - the
# graph's tables and the operands as guarded copies (``_G``) - and every pointer goes through gptr, which refuses any other tensor.
def _full(*s):
    return guarded(s, fill=FILL)


def _zeros(*s):
    return guarded(s, fill=0.0)


def _G(t, name="?"):
    return guard_input(t.contiguous(), name)


def _guard_all(o):
    return {k: _G(t, k) for k, t in o.items()}


def _strided(t, ld):
    """the same matrix as rows of a [rows, ld] buffer whose other columns hold FILL"""
    buf = _full(t.shape[0], ld)
    buf[:, :t.shape[1]] = t
    return buf


def _same_bits(rep, entry, name, got, other, what):
    """a bitwise comparison whose failure is reported with the case's other failures (Report.finish), not ahead of them"""
    if not torch.equal(got, other):
        rep.failed.append((entry, name, "bits differ from " + what))


def _finalize(lib, partial, slabs, Fw):
    red = _full(2, Fw)
    assert lib.alignn_bn_bwd_finalize(gptr(partial), slabs, Fw, gptr(red), stream()) == 0
    return red


# ----------------------------------------------------------------------------------------------------------------------
# LayerNorm row kernels
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,Fw,data", D.ROW_CASES)
def test_layernorm_row_kernels_against_float64(rows, Fw, data):
    """alignn_ln_silu_dual_fwd (with and without residual, with Y == NULL), alignn_ln_silu_dual_bwd and alignn_ln_silu_dual_bwd_node:
    y, yt, the row statistics, gx, gxt, dbeta and dgamma through alignn_bn_bwd_finalize, Q1 .. Q0t, on contiguous operands and on
    operands of leading dimension F + 8; the node variant writes the last column block of a [rows, 4F] buffer.  Up to one row per
    wave (rows <= 5) and two or three (4097, 9001: the grid is capped at 1024 workgroups of 4 waves, the dbeta / dgamma registers
    and the slab write then accumulate over a wave's rows)."""
    rep = Report(f"rows={rows} F={Fw} {data}", "dual-f64")
    lib = rep.launcher(_lib.load())
    st = stream()
    o = _guard_all(D.row_operands(rows, Fw, data, DEV))
    other = data != "normal"
    slabs = lib.alignn_dual_slabs(rows)
    assert slabs == min((rows + 3) // 4, 1024)
    ref = {}
    for res in (False, True):
        r64 = D.row_case(F64, o, res)
        r32 = D.row_case(F32, o, res) if other else None
        ref[res] = (r64, r32)
        f32 = lambda k: None if r32 is None else r32[k]  # noqa: E731
        for ld in (Fw, Fw + 8):
            X, Xt, R, Rt = (_strided(o[k], ld) for k in ("X", "Xt", "R", "Rt"))
            for have_y in (True, False):
                Y, Yt, stat, am = _full(rows, ld), _full(rows, ld), _full(rows, 2), _zeros(2)
                assert lib.alignn_ln_silu_dual_fwd(gptr(X), gptr(Xt), ld, gptr(R) if res else None, gptr(Rt) if res else None, ld,
                                                   gptr(o["gamma"]), gptr(o["beta"]), D.EPS, gptr(Y) if have_y else None, gptr(Yt), ld,
                                                   gptr(stat), rows, Fw, gptr(am), st) == 0
                torch.cuda.synchronize()
                ent = "ln_silu_dual_fwd" + (" +R" if res else "") + ("" if have_y else " Y=NULL") + f" ld={ld}"
                if have_y:
                    rep.close(ent, "y", Y[:, :Fw], r64["y"], f32("y"), B_LN_FWD)
                    rep.amax(ent, "amax2[0]", am[0], Y[:, :Fw])
                    assert bool((Y[:, Fw:] == FILL).all())
                else:
                    assert bool((Y == FILL).all()), "Y == NULL: the value buffer keeps its fill"
                    rep.amax(ent, "amax2[0]", am[0], torch.zeros(0))
                rep.close(ent, "yt", Yt[:, :Fw], r64["yt"], f32("yt"), B_LN_FWD)
                rep.amax(ent, "amax2[1]", am[1], Yt[:, :Fw])
                assert bool((Yt[:, Fw:] == FILL).all())
                rep.close(ent, "mean", stat[:, 0], r64["mean"], f32("mean"), B_LN_FWD)
                rep.close(ent, "rstd", stat[:, 1], r64["rstd"], f32("rstd"), B_LN_FWD)
    # ---- reverse (the residual does not enter); the statistics handed over are float64's, rounded once
    r64, r32 = ref[False]
    f32 = lambda k: None if r32 is None else r32[k]  # noqa: E731
    stat = _G(torch.stack([r64["mean"], r64["rstd"]], 1).float())
    node_in = [o[k] for k in ("S0", "HH", "S0t", "HHt")]
    for ld in (Fw, Fw + 8):
        X, Xt, GY, GYt = (_strided(o[k], ld) for k in ("X", "Xt", "GY", "GYt"))
        GX, GXt, partial, am = _full(rows, ld), _full(rows, ld), _full(slabs, 2, Fw), _zeros(2)
        assert lib.alignn_ln_silu_dual_bwd(gptr(GY), gptr(GYt), ld, gptr(X), gptr(Xt), ld, gptr(o["gamma"]), gptr(o["beta"]), gptr(stat),
                                           gptr(GX), gptr(GXt), ld, gptr(partial), rows, Fw, gptr(am), st) == 0
        red = _finalize(lib, partial, slabs, Fw)
        torch.cuda.synchronize()
        ent = f"ln_silu_dual_bwd ld={ld}"
        rep.close(ent, "gx", GX[:, :Fw], r64["gx"], f32("gx"), B_LN_INPUT)
        rep.close(ent, "gxt", GXt[:, :Fw], r64["gxt"], f32("gxt"), B_LN_INPUT)
        rep.close(ent, "dbeta", red[0], r64["dbeta"], f32("dbeta"), B_LN_PARAM)
        rep.close(ent, "dgamma", red[1], r64["dgamma"], f32("dgamma"), B_LN_PARAM)
        rep.amax(ent, "amax2[0]", am[0], GX[:, :Fw])
        rep.amax(ent, "amax2[1]", am[1], GXt[:, :Fw])
        assert bool((GX[:, Fw:] == FILL).all()) and bool((GXt[:, Fw:] == FILL).all())
        # the node variant: (gx, gxt) into the Ux column block of [rows, 4F] buffers, Q1 .. Q0t beside them
        GP, GPt, partial, am = _full(rows, 4 * Fw), _full(rows, 4 * Fw), _full(slabs, 2, Fw), _G(torch.tensor([0.0, ABOVE], device=DEV))
        ux, uxt = GP[:, 3 * Fw:], GPt[:, 3 * Fw:]
        q = [_full(rows, Fw) for _ in range(4)]
        assert lib.alignn_ln_silu_dual_bwd_node(gptr(GY), gptr(GYt), ld, gptr(X), gptr(Xt), ld, gptr(o["gamma"]), gptr(o["beta"]), gptr(stat),
                                                gptr(ux), gptr(uxt), 4 * Fw, gptr(partial), rows, Fw, gptr(am), *(gptr(t) for t in node_in),
                                                *(gptr(t) for t in q), st) == 0
        red = _finalize(lib, partial, slabs, Fw)
        q_own = [_full(rows, Fw) for _ in range(4)]
        assert lib.alignn_egc_node_dual_bwd(gptr(ux), gptr(uxt), 4 * Fw, *(gptr(t) for t in node_in), *(gptr(t) for t in q_own), rows, Fw,
                                            st) == 0
        torch.cuda.synchronize()
        ent = f"ln_silu_dual_bwd_node ld={ld}"
        rep.close(ent, "gx", ux, r64["gx"], f32("gx"), B_LN_INPUT)
        rep.close(ent, "gxt", uxt, r64["gxt"], f32("gxt"), B_LN_INPUT)
        rep.close(ent, "dbeta", red[0], r64["dbeta"], f32("dbeta"), B_LN_PARAM)
        rep.close(ent, "dgamma", red[1], r64["dgamma"], f32("dgamma"), B_LN_PARAM)
        for k, t, t_own in zip(("Q1", "Q0", "Q1t", "Q0t"), q, q_own):
            rep.close(ent, k, t, r64[k], f32(k), B_GATE_FWD)
            _same_bits(rep, ent, k, t, t_own, "alignn_egc_node_dual_bwd on the same (gx, gxt)")
        rep.amax(ent, "amax2[0]", am[0], ux)
        assert float(am[1]) == ABOVE, "a slot above what the launch wrote must be left as it is"
        _same_bits(rep, ent, "gx", ux, GX[:, :Fw], "alignn_ln_silu_dual_bwd (same arithmetic, another leading dimension)")
        _same_bits(rep, ent, "gxt", uxt, GXt[:, :Fw], "alignn_ln_silu_dual_bwd (same arithmetic, another leading dimension)")
        assert bool((GP[:, :3 * Fw] == FILL).all()) and bool((GPt[:, :3 * Fw] == FILL).all())
    rep.finish()


@pytest.mark.parametrize("Fw", [64, 260, 1024])
def test_layernorm_row_kernels_without_rows(Fw):
    """rows == 0: the forward returns 0 and touches nothing; both reverse entries return 0 and leave a zero slab, so that the
    finalised [2, F] is exactly 0 over a workspace that held 7.0."""
    rep = Report(f"rows=0 F={Fw}", "dual-f64")
    lib = rep.launcher(_lib.load())
    st = stream()
    o = _guard_all(D.row_operands(4, Fw, "normal", DEV))
    stat = _full(4, 2)
    outs = [_full(4, Fw) for _ in range(8)]
    am = _zeros(2)
    assert lib.alignn_dual_slabs(0) == 1
    assert lib.alignn_ln_silu_dual_fwd(gptr(o["X"]), gptr(o["Xt"]), Fw, gptr(o["R"]), gptr(o["Rt"]), Fw, gptr(o["gamma"]), gptr(o["beta"]), D.EPS,
                                       gptr(outs[0]), gptr(outs[1]), Fw, gptr(stat), 0, Fw, gptr(am), st) == 0
    torch.cuda.synchronize()
    assert bool((stat == FILL).all()) and float(am.abs().max()) == 0.0
    for node in (False, True):
        partial = _full(4, 2, Fw)
        if node:
            rc = lib.alignn_ln_silu_dual_bwd_node(gptr(o["GY"]), gptr(o["GYt"]), Fw, gptr(o["X"]), gptr(o["Xt"]), Fw, gptr(o["gamma"]),
                                                  gptr(o["beta"]), gptr(stat), gptr(outs[0]), gptr(outs[1]), Fw, gptr(partial), 0, Fw, gptr(am),
                                                  *(gptr(o[k]) for k in ("S0", "HH", "S0t", "HHt")), *(gptr(t) for t in outs[2:6]), st)
        else:
            rc = lib.alignn_ln_silu_dual_bwd(gptr(o["GY"]), gptr(o["GYt"]), Fw, gptr(o["X"]), gptr(o["Xt"]), Fw, gptr(o["gamma"]), gptr(o["beta"]),
                                             gptr(stat), gptr(outs[0]), gptr(outs[1]), Fw, gptr(partial), 0, Fw, gptr(am), st)
        assert rc == 0
        red = _finalize(lib, partial, 1, Fw)
        torch.cuda.synchronize()
        assert float(red.abs().max()) == 0.0 and bool((partial[1:] == FILL).all())
        assert all(bool((t == FILL).all()) for t in outs) and float(am.abs().max()) == 0.0
    rep.finish()


# ----------------------------------------------------------------------------------------------------------------------
# gate kernels
# ----------------------------------------------------------------------------------------------------------------------
def _run_gate_case(H, gname, data, stream_rows=False):
    rep = Report(f"H={H} {gname} {data}", "dual-f64")
    lib = rep.launcher(_lib.load())
    st = stream()
    g = graph(gname)
    o = _guard_all(D.operands(H, g, data, DEV))
    g = guard_graph(g)
    n, m = g.n_nodes, g.n_edges
    u, v = g.src.long(), g.dst.long()
    other = data != "normal"
    r64 = D.gate_case(F64, o, u, v, n, H)
    hd = r64["handed"] = _guard_all(r64["handed"])
    r32 = D.gate_case(F32, o, u, v, n, H, hd) if other else {}
    f32 = lambda k: r32.get(k)  # noqa: E731
    P, Pt = o["P"], o["Pt"]
    csr = (gptr(g.seg_ptr), gptr(g.seg_node), gptr(g.src))
    parts = D.reverse_parts(data, n, v)

    # ---- forward: values and tangents from C, Ct
    M, Mt = _G(o["C"]), _G(o["Ct"])
    xpre, xpre_t, s0, hh, s0t, hht = (_full(n, H) for _ in range(6))
    assert lib.alignn_egc_gate_dual_fwd(gptr(P), gptr(Pt), gptr(M), gptr(Mt), *csr, n, m, H, gptr(xpre), gptr(xpre_t), gptr(s0), gptr(hh),
                                        gptr(s0t), gptr(hht), st) == 0
    torch.cuda.synchronize()
    fwd = dict(m=M, mt=Mt, xpre=xpre, xpre_t=xpre_t, s0=s0, hh=hh, s0t=s0t, hht=hht)
    for k, t in fwd.items():
        rep.close("gate_dual_fwd", k, t, r64[k], f32(k), B_LN_FWD if k in ("m", "mt") else B_GATE_FWD)
    # the tangent half alone, handed the values the full pass wrote: the same bits, and M untouched
    M_before, Mt2 = M.clone(), _G(o["Ct"])
    xpre_t2, s0t2, hht2 = (_full(n, H) for _ in range(3))
    assert lib.alignn_egc_gate_dual_fwd_tangent(gptr(P), gptr(Pt), gptr(M), gptr(Mt2), *csr, n, m, H, gptr(xpre_t2), gptr(s0), gptr(hh), gptr(s0t2),
                                                gptr(hht2), st) == 0
    torch.cuda.synchronize()
    assert torch.equal(M, M_before), "alignn_egc_gate_dual_fwd_tangent wrote to M"
    for k, t in (("mt", Mt2), ("xpre_t", xpre_t2), ("s0t", s0t2), ("hht", hht2)):
        rep.close("gate_dual_fwd_tangent", k, t, r64[k], f32(k), B_LN_FWD if k == "mt" else B_GATE_FWD)
        _same_bits(rep, "gate_dual_fwd_tangent", k, t, fwd[k], "the tangent half of alignn_egc_gate_dual_fwd")

    # ---- node side of the reverse: LayerNorm reverse + quotient reverse in one launch, into the Ux block of GP / GPt
    GP, GPt = _full(n, 4 * H), _full(n, 4 * H)
    ux, uxt = GP[:, 3 * H:], GPt[:, 3 * H:]
    slabs = lib.alignn_dual_slabs(n)
    partial, gp_amax = _full(slabs, 2, H), _zeros(2)
    node_in = [hd[k] for k in ("s0", "hh", "s0t", "hht")]
    q = [_full(n, H) for _ in range(4)]
    assert lib.alignn_ln_silu_dual_bwd_node(gptr(o["GX"]), gptr(o["GXt"]), H, gptr(hd["xpre"]), gptr(hd["xpre_t"]), H, gptr(o["n_gamma"]),
                                            gptr(o["n_beta"]), gptr(hd["n_stat"]), gptr(ux), gptr(uxt), 4 * H, gptr(partial), n, H, gptr(gp_amax),
                                            *(gptr(t) for t in node_in), *(gptr(t) for t in q), st) == 0
    red = _finalize(lib, partial, slabs, H)
    q_own, q_handed = [_full(n, H) for _ in range(4)], [_full(n, H) for _ in range(4)]
    assert lib.alignn_egc_node_dual_bwd(gptr(ux), gptr(uxt), 4 * H, *(gptr(t) for t in node_in), *(gptr(t) for t in q_own), n, H, st) == 0
    assert lib.alignn_egc_node_dual_bwd(gptr(hd["gx"]), gptr(hd["gxt"]), H, *(gptr(t) for t in node_in), *(gptr(t) for t in q_handed), n, H,
                                        st) == 0
    torch.cuda.synchronize()
    ent = "ln_silu_dual_bwd_node"
    rep.close(ent, "gx", ux, r64["gx"], f32("gx"), B_LN_INPUT)
    rep.close(ent, "gxt", uxt, r64["gxt"], f32("gxt"), B_LN_INPUT)
    rep.close(ent, "dbeta", red[0], r64["n_dbeta"], f32("n_dbeta"), B_LN_PARAM)
    rep.close(ent, "dgamma", red[1], r64["n_dgamma"], f32("n_dgamma"), B_LN_PARAM)
    rep.amax(ent, "amax2[0]", gp_amax[0], ux)
    rep.amax(ent, "amax2[1]", gp_amax[1], uxt)
    assert bool((GP[:, :3 * H] == FILL).all()) and bool((GPt[:, :3 * H] == FILL).all())
    for sfx, _, nm in parts:
        for k, t, t_own, t_h in zip(("Q1", "Q0", "Q1t", "Q0t"), q, q_own, q_handed):
            r3 = None if f32(k) is None else D.part(f32(k), nm)
            rep.close(ent + sfx, k, D.part(t, nm), D.part(r64[k], nm), r3, B_GATE_FWD)
            rep.close("node_dual_bwd" + sfx, k, D.part(t_h, nm), D.part(r64[k], nm), r3, B_GATE_FWD)
            _same_bits(rep, ent + sfx, k, t, t_own, "alignn_egc_node_dual_bwd on the same (gx, gxt)")
    ux_before, uxt_before = ux.clone(), uxt.clone()

    # ---- reverse of the gate pass (handed M, Mt, the float64 adjoints Q1 .. Q0t and GL, GLt rounded once)
    Mo, Mto = o["M"], o["Mt"]
    qs = [hd[k] for k in ("Q1", "Q0", "Q1t", "Q0t")]

    def check(ent, tag, GM, GMt, gb, gm_amax, first_amax, preset=False):
        for sfx, em, nm in parts:
            fl = D.reverse_floors(r64, tag, nm)
            for k, t, mask in (("GM", GM, em), ("GMt", GMt, em), ("GP", GP[:, :3 * H], nm), ("GPt", GPt[:, :3 * H], nm)):
                r3 = None if f32(tag + k) is None else D.part(f32(tag + k), mask)
                rep.close(ent + sfx, k, D.part(t, mask), D.part(r64[tag + k], mask), r3, B_REVERSE, fl[k])
            if sfx != " sat":
                rep.close(ent + sfx, "gb", gb.sum(0), r64[tag + "gb"], f32(tag + "gb"), B_REVERSE, fl["gb"])
        # gb_partial over its slabs IS the column sums of the GM this launch wrote (float32 sums of m terms in any order)
        if m:
            exact = GM.double().sum(0)
            slack = m * 2.0 ** -24 * GM.double().abs().sum(0) + 1e-30
            assert bool(((gb.double().sum(0) - exact).abs() <= slack).all()), (ent, "gb_partial against the column sums of GM")
        rep.amax(ent, "gm_amax2[0]", gm_amax[0], GM)
        if preset:
            assert float(gm_amax[1]) == ABOVE, (ent, "a slot above what the launch wrote must be left as it is")
        else:
            rep.amax(ent, "gm_amax2[1]", gm_amax[1], GMt)
        # GP.amax is shared with the node LayerNorm reverse (ff2.conv_bwd): the larger of what both wrote
        rep.amax(ent, "gp_amax2[0]", gp_amax[0], GP if first_amax else GP[:, :3 * H])
        rep.amax(ent, "gp_amax2[1]", gp_amax[1], GPt if first_amax else GPt[:, :3 * H])
        assert torch.equal(ux, ux_before) and torch.equal(uxt, uxt_before), (ent, "the Ux block is not the gate reverse's")

    first = True
    for has_gl in (True, False):
        tag = "gl_" if has_gl else "nogl_"
        gl, glt = (gptr(hd["GL"]), gptr(hd["GLt"])) if has_gl else (None, None)
        variant = " GL" if has_gl else " GL=NULL"
        # destination-ordered and source-ordered halves
        GP[:, :3 * H] = FILL
        GPt[:, :3 * H] = FILL
        if not first:
            gp_amax.zero_()
        GM, GMt, gb, gm_amax, src_amax = _full(m, H), _full(m, H), _full(slabs, H), _zeros(2), _zeros(2)
        if not has_gl:
            gm_amax[1] = ABOVE
        assert lib.alignn_egc_dual_bwd_dst(gl, glt, gptr(Mo), gptr(Mto), gptr(P), gptr(Pt), *(gptr(t) for t in qs), *csr, n, H, gptr(GM), gptr(GMt),
                                           gptr(GP), gptr(GPt), gptr(gb), gptr(gm_amax), gptr(gp_amax), st) == 0
        torch.cuda.synchronize()
        assert bool((GP[:, :H] == FILL).all()) and bool((GP[:, 2 * H:3 * H] == FILL).all())  # (this half writes the Bd block only)
        if not first:
            for w, t in enumerate((GP, GPt)):
                rep.amax("dual_bwd_dst" + variant, f"gp_amax2[{w}]", gp_amax[w], t[:, H:2 * H])
        assert lib.alignn_egc_dual_bwd_src(gptr(GM), gptr(GMt), gptr(Mo), gptr(Mto), gptr(qs[0]), gptr(qs[2]), gptr(g.out_ptr), gptr(g.out_slot),
                                           gptr(g.dst), n, H, gptr(GP), gptr(GPt), gptr(src_amax), st) == 0
        torch.cuda.synchronize()
        for w, t in enumerate((GP, GPt)):
            rep.amax("dual_bwd_src" + variant, f"gp_amax2[{w}]", src_amax[w], torch.cat([t[:, :H], t[:, 2 * H:3 * H]], 1))
        gp_amax.copy_(torch.maximum(gp_amax, src_amax))  # (what one shared slot would hold after both halves)
        check("dual_bwd_dst+src" + variant, tag, GM, GMt, gb, gm_amax, first, preset=not has_gl)
        first = False
        # the dense-block kernel (line graphs): cached loads, and the streaming ones an m_rows at the threshold selects
        if is_line_graph(g):
            groups = g.grp_seg_ptr.numel() - 1
            for m_rows in (m,) + (((128 << 20) // (4 * H),) if stream_rows else ()):
                GP[:, :3 * H] = FILL
                GPt[:, :3 * H] = FILL
                gp_amax.zero_()
                GM, GMt, gb, gm_amax = _full(m, H), _full(m, H), _full(groups, H), _zeros(2)
                if not has_gl:
                    gm_amax[1] = ABOVE
                assert lib.alignn_egc_dual_bwd_lg_dense(gl, glt, gptr(Mo), gptr(Mto), gptr(P), gptr(Pt), *(gptr(t) for t in qs), m_rows,
                                                        gptr(g.grp_seg_ptr), gptr(g.grp_src_ptr), groups, gptr(g.seg_ptr), gptr(g.seg_node), H,
                                                        gptr(GM), gptr(GMt), gptr(GP), gptr(GPt), gptr(gb), gptr(gm_amax), gptr(gp_amax), st) == 0
                torch.cuda.synchronize()
                check("dual_bwd_lg_dense" + variant + ("" if m_rows == m else " m_rows=threshold"), tag, GM, GMt, gb, gm_amax, False,
                      preset=not has_gl)
    rep.finish()


@pytest.mark.parametrize("H,gname,data", D.GATE_CASES)
def test_gate_kernels_against_float64(H, gname, data):
    """alignn_egc_gate_dual_fwd, alignn_egc_gate_dual_fwd_tangent, alignn_ln_silu_dual_bwd_node writing the Ux block of GP,
    alignn_egc_node_dual_bwd, alignn_egc_dual_bwd_dst + _src and, on line graphs, alignn_egc_dual_bwd_lg_dense - each against the
    float64 restatement (the dense kernel and the two-pass pair each on its own, not only against each other), with GL given and
    GL == NULL; one to four feature panels and tail panels (H = 260, 512, 1024); empty segments beside a 331-row one, atoms of
    more than 16 in-edges, one-atom cells whose segments omit their own source, more than 4096 segments."""
    _run_gate_case(H, gname, data)


def test_dense_kernel_streaming_instantiations_on_a_small_graph():
    """m_rows only chooses between the cached and the streaming loads of alignn_egc_dual_bwd_lg_dense: at (128 << 20) / (4 H) a
    small graph runs the STREAM instantiations of both HAS_GL values, several panels and several passes of 16 sources."""
    _run_gate_case(512, "lg_deg17", "normal", stream_rows=True)


def test_dense_kernel_on_a_line_graph_that_streams():
    """a real streaming launch: >= 128 MiB per [rows, 256] tensor.  The dense kernel only, with GL given, on N(0,1) operands and
    adjoints."""
    rep = Report("H=256 lg_stream normal", "dual-f64")
    lib = rep.launcher(_lib.load())
    st = stream()
    H, g = 256, graph("lg_stream")
    n, m = g.n_nodes, g.n_edges
    assert m * H * 4 >= 128 << 20
    u, v = g.src.long(), g.dst.long()
    o = _guard_all(D.operands(H, g, "normal", DEV))
    g = guard_graph(g)
    gen = torch.Generator(device=DEV).manual_seed(11)
    o.update({k: _G(torch.randn(n, H, device=DEV, generator=gen), k) for k in ("Q1", "Q0", "Q1t", "Q0t")})
    rev = D.ln_reverse(F64, o["M"], o["Mt"], o["gamma"], o["beta"], o["GY"], o["GYt"])
    GL, GLt = _G(rev["gx"].float(), "GL"), _G(rev["gxt"].float(), "GLt")
    del rev
    r64 = D.reverse(F64, o, u, v, n, H, True)
    groups = g.grp_seg_ptr.numel() - 1
    GM, GMt, GP, GPt, gb, gm_amax, gp_amax = _full(m, H), _full(m, H), _full(n, 4 * H), _full(n, 4 * H), _full(groups, H), _zeros(2), _zeros(2)
    assert lib.alignn_egc_dual_bwd_lg_dense(gptr(GL), gptr(GLt), gptr(o["M"]), gptr(o["Mt"]), gptr(o["P"]), gptr(o["Pt"]),
                                            *(gptr(o[k]) for k in ("Q1", "Q0", "Q1t", "Q0t")), m, gptr(g.grp_seg_ptr), gptr(g.grp_src_ptr),
                                            groups, gptr(g.seg_ptr), gptr(g.seg_node), H, gptr(GM), gptr(GMt), gptr(GP), gptr(GPt), gptr(gb),
                                            gptr(gm_amax), gptr(gp_amax), st) == 0
    torch.cuda.synchronize()
    fl, flt = 1e-2 * float(r64["GP"].abs().max()), 1e-2 * float(r64["GPt"].abs().max())
    ent = "dual_bwd_lg_dense GL streaming"
    rep.close(ent, "GM", GM, r64["GM"], None, B_REVERSE, fl)
    rep.close(ent, "GMt", GMt, r64["GMt"], None, B_REVERSE, flt)
    rep.close(ent, "GP", GP[:, :3 * H], r64["GP"], None, B_REVERSE, fl)
    rep.close(ent, "GPt", GPt[:, :3 * H], r64["GPt"], None, B_REVERSE, flt)
    rep.close(ent, "gb", gb.sum(0), r64["gb"], None, B_REVERSE, fl)
    rep.amax(ent, "gm_amax2[0]", gm_amax[0], GM)
    rep.amax(ent, "gm_amax2[1]", gm_amax[1], GMt)
    rep.amax(ent, "gp_amax2[0]", gp_amax[0], GP[:, :3 * H])
    rep.amax(ent, "gp_amax2[1]", gp_amax[1], GPt[:, :3 * H])
    assert bool((GP[:, 3 * H:] == FILL).all()) and bool((GPt[:, 3 * H:] == FILL).all())
    rep.finish()


# ----------------------------------------------------------------------------------------------------------------------
# refusals
# ----------------------------------------------------------------------------------------------------------------------
def _refusal_calls(lib, g, W, H, t, drop=None):
    """every entry point of csrc/dual.hip at width H on buffers of width W >= H (a wrongly accepted call stays in bounds);
    ``drop``: an argument to pass as NULL"""
    n, m, st = g.n_nodes, g.n_edges, stream()
    groups = g.grp_seg_ptr.numel() - 1
    p = lambda k: None if k == drop else gptr(t[k])  # noqa: E731
    csr = (gptr(g.seg_ptr), gptr(g.seg_node), gptr(g.src))
    node_in = [p(k) for k in ("s0", "hh", "s0t", "hht")]
    q_out = [p(k) for k in ("o_q1", "o_q0", "o_q1t", "o_q0t")]
    q_in = [p(k) for k in ("s0", "hh", "s0t", "hht")]
    return {
        "ln_silu_dual_fwd": lambda: lib.alignn_ln_silu_dual_fwd(p("M"), p("Mt"), W, p("R"), p("Rt"), W, p("gamma"), p("beta"), D.EPS, p("o_em"),
                                                                p("o_emt"), W, p("o_stat"), m, H, p("o_am"), st),
        "ln_silu_dual_bwd": lambda: lib.alignn_ln_silu_dual_bwd(p("R"), p("Rt"), W, p("M"), p("Mt"), W, p("gamma"), p("beta"), p("stat"),
                                                                p("o_em"), p("o_emt"), W, p("o_part"), m, H, p("o_am"), st),
        "ln_silu_dual_bwd_node": lambda: lib.alignn_ln_silu_dual_bwd_node(p("hh"), p("s0t"), W, p("s0"), p("hht"), W, p("gamma"), p("beta"),
                                                                          p("stat"), p("o_gx"), p("o_gxt"), W, p("o_part"), n, H, p("o_am"),
                                                                          *node_in, *q_out, st),
        "gate_dual_fwd": lambda: lib.alignn_egc_gate_dual_fwd(p("P"), p("Pt"), p("M"), p("Mt"), *csr, n, m, H, p("o_q1"), p("o_q0"), p("o_q1t"),
                                                              p("o_q0t"), p("o_n4"), p("o_n5"), st),
        "gate_dual_fwd_tangent": lambda: lib.alignn_egc_gate_dual_fwd_tangent(p("P"), p("Pt"), p("M"), p("Mt"), *csr, n, m, H, p("o_q1"), p("s0"),
                                                                              p("hh"), p("o_q0"), p("o_q1t"), st),
        "node_dual_bwd": lambda: lib.alignn_egc_node_dual_bwd(p("hh"), p("hht"), W, *q_in, *q_out, n, H, st),
        "dual_bwd_dst": lambda: lib.alignn_egc_dual_bwd_dst(p("R"), p("Rt"), p("M"), p("Mt"), p("P"), p("Pt"), *q_in, *csr, n, H, p("o_em"),
                                                            p("o_emt"), p("o_gp"), p("o_gpt"), p("o_gb"), p("o_am"), p("o_am2"), st),
        "dual_bwd_src": lambda: lib.alignn_egc_dual_bwd_src(p("R"), p("Rt"), p("M"), p("Mt"), p("s0"), p("hh"), gptr(g.out_ptr), gptr(g.out_slot),
                                                            gptr(g.dst), n, H, p("o_gp"), p("o_gpt"), p("o_am2"), st),
        "dual_bwd_lg_dense": lambda: lib.alignn_egc_dual_bwd_lg_dense(p("R"), p("Rt"), p("M"), p("Mt"), p("P"), p("Pt"), *q_in, m,
                                                                      gptr(g.grp_seg_ptr), gptr(g.grp_src_ptr), groups, gptr(g.seg_ptr),
                                                                      gptr(g.seg_node), H, p("o_em"), p("o_emt"), p("o_gp"), p("o_gpt"), p("o_gb"),
                                                                      p("o_am"), p("o_am2"), st),
    }


def _refusal_buffers(g, W):
    n, m = g.n_nodes, g.n_edges
    I = lambda *s: _G(torch.randn(*s, device=DEV))  # noqa: E731, E741
    t = dict(P=I(n, 4 * W), Pt=I(n, 4 * W), M=I(m, W), Mt=I(m, W), R=I(m, W), Rt=I(m, W), gamma=I(W), beta=I(W), stat=I(max(n, m), 2),
             s0=_G(torch.randn(n, W, device=DEV).abs()), hh=I(n, W), s0t=I(n, W), hht=I(n, W))
    t.update(o_em=_full(m, W), o_emt=_full(m, W), o_gp=_full(n, 4 * W), o_gpt=_full(n, 4 * W), o_gb=_full(1024, W), o_part=_full(1024, 2, W),
             o_stat=_full(m, 2), o_am=_full(2), o_am2=_full(2), o_q1=_full(n, W), o_q0=_full(n, W), o_q1t=_full(n, W), o_q0t=_full(n, W),
             o_n4=_full(n, W), o_n5=_full(n, W), o_gx=_full(n, W), o_gxt=_full(n, W))
    return t


def _unchanged(t, before):
    return all(bool((x == FILL).all()) for k, x in t.items() if k.startswith("o_")) and all(torch.equal(t[k], before[k]) for k in before)


@pytest.mark.parametrize("H", [0, 2, 6, 1028])
def test_unsupported_widths_are_refused(H):
    """hipErrorInvalidValue and no launch (every output keeps its fill, M and Mt their contents) at widths outside
    F % 4 == 0, 4 <= F <= 1024, from every entry point."""
    rep = Report(f"refusals H={H}", "dual-f64")
    g = guard_graph(graph("lg_small"))
    t = _refusal_buffers(g, 1032)
    before = {k: t[k].clone() for k in ("M", "Mt")}
    rc = {k: f() for k, f in _refusal_calls(rep.launcher(_lib.load()), g, 1032, H, t).items()}
    torch.cuda.synchronize()
    assert all(r == INVALID for r in rc.values()), rc
    assert _unchanged(t, before)
    rep.finish()  # (and nothing beside the outputs either)


def test_half_given_pairs_and_null_node_pointers_are_refused():
    """R without Rt (and Rt without R), GL without GLt (and the reverse) and any null node pointer of alignn_ln_silu_dual_bwd_node:
    hipErrorInvalidValue and no launch, at a supported width."""
    rep = Report("refusals of half-given pairs", "dual-f64")
    lib = rep.launcher(_lib.load())
    g = guard_graph(graph("lg_small"))
    W = H = 64
    t = _refusal_buffers(g, W)
    before = {k: t[k].clone() for k in ("M", "Mt")}
    for drop in ("R", "Rt"):
        calls = _refusal_calls(lib, g, W, H, t, drop)
        rc = {k: calls[k]() for k in ("ln_silu_dual_fwd", "dual_bwd_dst", "dual_bwd_lg_dense")}
        torch.cuda.synchronize()
        assert all(r == INVALID for r in rc.values()), (drop, rc)
        assert _unchanged(t, before)
    for drop in ("s0", "hh", "s0t", "hht", "o_q1", "o_q0", "o_q1t", "o_q0t"):
        assert _refusal_calls(lib, g, W, H, t, drop)["ln_silu_dual_bwd_node"]() == INVALID, drop
        torch.cuda.synchronize()
        assert _unchanged(t, before)
    rep.finish()  # (and nothing beside the outputs either)
