"""csrc/conv.hip - the edge-gated convolution of plain ALIGNN: the gate passes with their BatchNorm pivot slabs, the node
quotient reverse and the three routes of the gate reverse - against the float64 torch restatements of tests/conv_bn_ref.py
(checked on their own by tests/test_conv_bn_ref.py), entry point by entry point and output by output.  The other tests of these
kernels pin summation orders and bit-identity between variants, or compare whole models; here the other side is ``index_add`` /
``sigmoid`` / ``silu`` / explicit column statistics in float64 and float64 autograd of those expressions.

Tolerances - all inherited; one carries a measured second term (below).  On N(0,1) operands the bounds tests/test_gpu_convln.py takes from tests/test_gpu_dual.py for these
very kernels: 2e-5 for what a gate forward writes (M, XPRE, S0, HH, YOUT) and for the BatchNorm parameter sums e_red, 5e-5 (with
its floor of 1e-2 of the largest GP entry) for what a gate reverse writes (GM, GP, gb; GS1 and GS0 of the node quotient without a
floor).  On every other data distribution the SAME restatement is evaluated in float32 on the identical float32 operands; the
kernel may be 4x as far from float64 as that, plus the N(0,1) bound as a floor.  Statistics that come out of pivot slabs
(alignn_bn_finalize_welford on e_partial / n_partial) take the bounds of tests/test_gpu_round3.py::
test_welford_column_statistics_are_well_conditioned on every distribution: mean and running mean within 2e-7 (max |mean| + 1) (plus
the term below), rstd and scale = gamma * rstd to 1e-4 relative in every column, the running variance to 1e-5 relative in every
column, shift == beta; the slab counts sum to exactly the number of rows.

One inherited bound was over-tight and carries a second term.  2e-7 (max |mean| + 1) comes from alignn_col_stats_welford, where a
thread sums few rows about its pivot before float64 takes over.  A gate pass sums ALL rows of a wave's segments in float32 about
the first value the wave sees, which can sit several spreads from the mean: on the ``synthetic`` graph (a 331-row segment in one
wave, 540 rows in all) the edge mean missed the bound on N(0,1) data by up to 4x (2.3e-6 against 7e-7) and on ``saturated_gates``
by 8x (9.2e-5 on columns spread over +-170), while rstd, the running variance and every output normalised with these statistics
stayed inside theirs.  That is the rounding of a float32 sum of deviations, proportional to the deviations and not to the mean,
and no defect: the largest |mean error| / max |x - mean| over all cases and passes is 8.65e-7 (the ``conv-bn-mean`` lines).
The means therefore may be off by 2e-7 (max |mean| + 1) + MEAN_DEV max |x - mean| with MEAN_DEV = 4 x 8.65e-7 = 3.5e-6, the
running means by the inherited term + 0.1 of the second (momentum).  Errors of tensors are max |a - b| / max |b| over the whole tensor; no
element, row, column or case is left out.  Output buffers are filled with NaN before a launch, so a row nobody wrote fails.

Each later pass is handed the float64 result of the earlier one rounded once (statistics, S0, HH, e_red), so one kernel's error
is not charged to the next.  An ``amax`` slot (zeroed before the launch) must EQUAL the largest magnitude among the elements the
launch wrote: the next f16x3 product takes its power-of-two scale from it, and a value too small overflows the fp16 slices
silently.  (The equality found alignn_egc_bwd_lg_dense counting the partial Bd sums of an earlier 16-source pass, which the next
pass overwrites: gp_amax 26.768 for a largest written magnitude of 25.657 at H=1024 on ``lg_deg17``; fixed in the kernel.)  The
worst error per entry point and output is printed as ``conv-bn-parity`` lines (one GPU run of them, summarised:
profiles/conv_bn_float64_parity.txt)."""

import pytest
import torch

pytestmark = pytest.mark.gpu

from alignn_amd import _lib  # noqa: E402
from alignn_amd._lib import stream  # noqa: E402
from tests import conv_bn_ref as ref  # noqa: E402
from tests.gate_parity import Report, gptr, graph, guard_graph, guard_input, guarded, is_line_graph  # noqa: E402

DEV = "cuda"
INVALID = 1  # hipErrorInvalidValue
HS = (4, 36, 64, 100, 256, 260, 512, 1024)  # 260: the second feature panel has one active lane
B_GATE_FWD, B_LN_PARAM, B_REVERSE = 2e-5, 2e-5, 5e-5  # on N(0,1) operands (see the module docstring); floors of everything else
MODES = ((0, 0), (1, 0), (1, 1), (2, 0))  # (MODE of edge_grad, e_eval)
NAN = float("nan")
MEAN_DEV = 3.5e-6  # 4 x 8.65e-7, the largest |mean error| / max |x - mean| measured (see the module docstring)


def _stat_asserts(rep, ent, side, stat, rm, rv, want, beta, x):
    """[4, H] stat and the running statistics out of alignn_bn_finalize_welford against float64 (bounds of
    test_welford_column_statistics_are_well_conditioned; see MEAN_DEV for the term the means take on top)"""
    d = lambda t: t.double()  # noqa: E731
    rel = lambda a, b: float(((d(a) - b).abs() / b.abs().clamp_min(1e-30)).max())  # noqa: E731
    mean, rstd, scale, rmean, rvar = (want[f"{side}_{k}"] for k in ("mean", "rstd", "scale", "rm", "rv"))
    dev = MEAN_DEV * float((x - mean).abs().max())
    e = float((d(stat[0]) - mean).abs().max())
    if dev > 0.0:
        print(f"conv-bn-mean {rep.case:<38s} {ent:<24s} {side} |mean error| / max |x - mean| = {e * MEAN_DEV / dev:8.2e}")
    rep.record(ent, side + ".mean", e, None, 2e-7 * (float(mean.abs().max()) + 1.0) + dev)
    rep.record(ent, side + ".rstd", rel(stat[1], rstd), None, 1e-4)
    rep.record(ent, side + ".scale", rel(stat[2], scale), None, 1e-4)
    rep.record(ent, side + ".rmean", float((d(rm) - rmean).abs().max()), None, 2e-7 * (float(rmean.abs().max()) + 1.0) + ref.MOMENTUM * dev)
    rep.record(ent, side + ".rvar", rel(rv, rvar), None, 1e-5)
    if not torch.equal(stat[3], beta):
        rep.failed.append((ent, side + ".shift", "is not beta"))


def _run_case(H, gname, data):
    rep = Report(f"H={H} {gname} {data}", "conv-bn-parity")
    lib = rep.launcher(_lib.load())
    # every buffer a launch is handed lies between guard bands (tests/gate_parity.Guards; rep.finish() checks them first), the
    # graph's tables and the operands as guarded copies, and every pointer goes through gptr, which refuses any other tensor
    g = guard_graph(graph(gname))
    n, m = g.n_nodes, g.n_edges
    u, v = g.src.long(), g.dst.long()
    o = {k: guard_input(t, k) for k, t in ref.operands(H, u, v, n, data, gname, DEV).items()}
    st = stream()
    other = data != "normal"
    E = lambda *s: guarded(s, fill=NAN, row=H)  # noqa: E731  (an output: whatever is not written fails)
    EM = lambda: guarded((max(m, 1), H), fill=NAN)  # noqa: E731  (an edge-row output: never a NULL pointer)
    Z = lambda *s: guarded(s, fill=0.0, row=H)  # noqa: E731
    G = lambda t: guard_input(t.contiguous())  # noqa: E731  (a tensor made here, handed to a launch)
    pad = Z(1, H)
    pin = lambda t: gptr(t if t.numel() else pad)  # noqa: E731  (an edge-row input of a graph without edges: not NULL either)
    P, C, M, Y, GY, Q1, Q0 = (o[k] for k in ("P", "C", "M", "Y", "GY", "Q1", "Q0"))
    eg, eb, ng, nb = o["e_gamma"], o["e_beta"], o["n_gamma"], o["n_beta"]
    slabs = lib.alignn_egc_slabs(n)
    seg = (gptr(g.seg_ptr), gptr(g.seg_node), gptr(g.src))

    def forward_ref(dt, second, pre, e_eval=False):
        c = {k: t.to(dt) for k, t in o.items()}
        fixed = ref.eval_stat(c["e_rm"], c["e_rv"], c["e_gamma"], c["e_beta"]) if e_eval else None
        return ref.values(c["P"], c[second], pre, c["e_gamma"], c["e_beta"], fixed, u, v, n, H, n_gamma=c["n_gamma"],
                          n_beta=c["n_beta"], running=c)

    def slab_buffers():  # exactly what include/alignn_hip.h states at alignn_egc_slabs: slabs * (3 H + 1) floats, nothing behind
        return E(slabs * (3 * H + 1)), E(slabs * (3 * H + 1))

    def node_side(ent, r64, r32, xpre, s0, hh, n_part):
        rep.close(ent, "XPRE", xpre, r64["xpre"], r32.get("xpre"), B_GATE_FWD)
        if s0 is not None:
            rep.close(ent, "S0", s0, r64["s0"], r32.get("s0"), B_GATE_FWD)
            rep.close(ent, "HH", hh, r64["hh"], r32.get("hh"), B_GATE_FWD)
        if n_part is not None:
            if float(n_part[slabs * 3 * H:].sum()) != n:
                rep.failed.append((ent, "node slab counts", n_part[slabs * 3 * H:].tolist(), n))
            stat, rm, rv = E(4, H), G(o["n_rm"]), G(o["n_rv"])
            assert lib.alignn_bn_finalize_welford(gptr(n_part), slabs, n, H, gptr(ng), gptr(nb), ref.EPS_BN, ref.MOMENTUM, gptr(rm), gptr(rv),
                                                  gptr(stat), st) == 0
            torch.cuda.synchronize()
            _stat_asserts(rep, ent, "n", stat, rm, rv, r64, nb, r64["xpre"])

    def edge_side(ent, r64, e_part):
        counts = e_part[slabs * 3 * H:]
        if float(counts.sum()) != m or (m == 0 and bool((counts != 0).any())):
            rep.failed.append((ent, "edge slab counts", counts.tolist(), m))
        if m == 0:  # (no finaliser is called with zero rows)
            return
        stat, rm, rv = E(4, H), G(o["e_rm"]), G(o["e_rv"])
        assert lib.alignn_bn_finalize_welford(gptr(e_part), slabs, m, H, gptr(eg), gptr(eb), ref.EPS_BN, ref.MOMENTUM, gptr(rm), gptr(rv),
                                              gptr(stat), st) == 0
        torch.cuda.synchronize()
        _stat_asserts(rep, ent, "e", stat, rm, rv, r64, eb, r64["m"])

    # ---- gate forward: m formed here (M holds C on entry, m on exit)
    f64 = forward_ref(torch.float64, "C", False)
    f32 = forward_ref(torch.float32, "C", False) if other else {}
    Mio, xpre, s0, hh = EM(), E(n, H), E(n, H), E(n, H)
    Mio[:m] = C
    e_part, n_part = slab_buffers()
    assert lib.alignn_egc_gate_fwd(gptr(P), gptr(Mio), *seg, n, m, H, gptr(xpre), gptr(s0), gptr(hh), gptr(e_part), gptr(n_part), st) == 0
    torch.cuda.synchronize()
    rep.close("gate_fwd", "M", Mio[:m], f64["m"], f32.get("m"), B_GATE_FWD)
    node_side("gate_fwd", f64, f32, xpre, s0, hh, n_part)
    edge_side("gate_fwd", f64, e_part)

    # ---- inference form: C only read, fixed affine map from running statistics that are not the batch's
    i64 = forward_ref(torch.float64, "C", False, e_eval=True)
    i32 = forward_ref(torch.float32, "C", False, e_eval=True) if other else {}
    ev_stat = G(i64["e_stat"].float())
    c_before = C.clone()
    xpre, am = E(n, H), Z(1)
    assert lib.alignn_egc_gate_infer(gptr(P), pin(C), *seg, n, m, H, gptr(xpre), None, None, None, gptr(am), st) == 0
    torch.cuda.synchronize()
    node_side("gate_infer -YOUT", i64, i32, xpre, None, None, None)
    rep.amax("gate_infer -YOUT", "y_amax", am[0], torch.zeros(0))  # (the YOUT = NULL form writes XPRE only)
    for res in (False, True):
        xpre, yout, am = E(n, H), EM(), Z(1)
        assert lib.alignn_egc_gate_infer(gptr(P), pin(C), *seg, n, m, H, gptr(xpre), gptr(ev_stat), pin(Y) if res else None, gptr(yout),
                                         gptr(am), st) == 0
        torch.cuda.synchronize()
        ent = "gate_infer" + (" +Y" if res else "")
        y32 = i32.get("y")
        rep.close(ent, "YOUT", yout[:m], i64["y"] + (Y.double() if res else 0), None if y32 is None else y32 + (Y if res else 0), B_GATE_FWD)
        node_side(ent, i64, i32, xpre, None, None, None)
        rep.amax(ent, "y_amax", am[0], yout[:m])
    assert torch.equal(C, c_before)
    del f64, f32, i64, i32

    # ---- gate forward on a given m (`pre`): M only read
    p64 = forward_ref(torch.float64, "M", True)
    p32 = forward_ref(torch.float32, "M", True) if other else {}
    Mio, xpre, s0, hh = G(M), E(n, H), E(n, H), E(n, H)
    e_part, n_part = slab_buffers()
    assert lib.alignn_egc_gate_fwd_pre(gptr(P), pin(Mio), *seg, n, m, H, gptr(xpre), gptr(s0), gptr(hh), gptr(e_part), gptr(n_part), st) == 0
    torch.cuda.synchronize()
    assert torch.equal(Mio, M)
    node_side("gate_fwd_pre", p64, p32, xpre, s0, hh, n_part)
    edge_side("gate_fwd_pre", p64, e_part)
    # (what the later passes are handed: the float64 statistics and node sums, rounded once)
    e_stat = G(p64["e_stat"].float())
    for res in (False, True):
        xpre, s0, hh, yout, am = E(n, H), E(n, H), E(n, H), EM(), Z(1)
        _, n_part = slab_buffers()
        assert lib.alignn_egc_gate_fwd_pre_norm(gptr(P), pin(M), *seg, n, m, H, gptr(xpre), gptr(s0), gptr(hh), gptr(n_part), gptr(e_stat),
                                                pin(Y) if res else None, gptr(yout), gptr(am), st) == 0
        torch.cuda.synchronize()
        ent = "gate_fwd_pre_norm" + (" +Y" if res else "")
        y32 = p32.get("y")
        rep.close(ent, "YOUT", yout[:m], p64["y"] + (Y.double() if res else 0), None if y32 is None else y32 + (Y if res else 0), B_GATE_FWD)
        node_side(ent, p64, p32, xpre, s0, hh, n_part)
        rep.amax(ent, "y_amax", am[0], yout[:m])

    # ---- node quotient reverse; every seventh row of S0 is zero (the epsilon alone in the denominator)
    s0_in, hh_in = p64["s0"].float(), G(p64["hh"].float())
    s0_in[::7] = 0.0
    s0_in = G(s0_in)
    del p64, p32
    for wide in (False, True):  # ldg = 4H: the Ux block of a [n, 4H] buffer, as ops calls it
        gx = o["GXW"][:, 3 * H:] if wide else o["GX"]
        gs1, gs0 = E(n, H), E(n, H)
        assert lib.alignn_egc_node_bwd(gptr(gx), gx.stride(0), gptr(s0_in), gptr(hh_in), gptr(gs1), gptr(gs0), n, H, st) == 0
        torch.cuda.synchronize()
        ent = "node_bwd" + (" ldg=4H" if wide else "")
        w64 = ref.node_reverse(gx.double(), s0_in.double(), hh_in.double())
        w32 = ref.node_reverse(gx, s0_in, hh_in) if other else (None, None)
        rep.close(ent, "GS1", gs1, w64[0], w32[0], B_REVERSE)
        rep.close(ent, "GS0", gs0, w64[1], w32[1], B_REVERSE)

    # ---- gate reverse, every route, every mode
    for mode, e_eval in MODES:
        stat_in = ev_stat if e_eval else e_stat
        rargs = (P, M, eg, eb, stat_in, GY, Q1, Q0, u, v, n, H, mode, e_eval)
        r64 = ref.reverse(torch.float64, *rargs)
        r32 = ref.reverse(torch.float32, *rargs) if other else {}
        fl = max(1e-2 * float(r64["GP"].abs().max()), 1e-30)
        tag = f" mode {mode}" + (" eval" if e_eval else "")
        e_red = None
        if mode == 1 and m > 0:
            # BatchNorm parameter sums by the column-reduction pass; the gate reverse then takes the float64 ones rounded once
            rslabs = lib.alignn_col_stats_slabs(m)
            part, red = E(rslabs, 2, H), E(2, H)
            assert lib.alignn_bn_silu_bwd_reduce(gptr(GY), H, gptr(M), H, gptr(stat_in), m, H, gptr(part), st) == 0
            assert lib.alignn_bn_bwd_finalize(gptr(part), rslabs, H, gptr(red), st) == 0
            torch.cuda.synchronize()
            rep.close("bn_silu_bwd_reduce" + tag, "e_red", red, r64["e_red"], r32.get("e_red"), B_LN_PARAM)
        if mode == 1:
            e_red = G(r64["e_red"].float())
        a_gy = pin(GY) if mode else None
        a_stat = gptr(stat_in) if mode == 1 else None

        def reverse_asserts(ent, GM, GP, gb, gma, gpa, blocks):
            rep.close(ent, "GM", GM[:m], r64["GM"], r32.get("GM"), B_REVERSE, fl)
            if blocks == 1:
                rep.close(ent, "GP_bd", GP[:, H:2 * H], r64["GP_bd"], r32.get("GP_bd"), B_REVERSE, fl)
                if float(GP[:, :H].abs().max()) != 0.0 or float(GP[:, 2 * H:].abs().max()) != 0.0:
                    rep.failed.append((ent, "GP", "wrote outside the Bd block"))
                rep.amax(ent, "gp_amax", gpa[0], GP[:, H:2 * H])
            else:
                rep.close(ent, "GP", GP[:, :3 * H], r64["GP"], r32.get("GP"), B_REVERSE, fl)
                if float(GP[:, 3 * H:].abs().max()) != 0.0:
                    rep.failed.append((ent, "GP", "wrote the Ux block"))
                rep.amax(ent, "gp_amax", gpa[0], GP[:, :3 * H])
            rep.close(ent, "gb", gb.double().sum(0), r64["gb"], r32.get("gb"), B_REVERSE, fl)
            rep.amax(ent, "gm_amax", gma[0], GM[:m])

        GM, GP, gb, gma, gpa = EM(), Z(n, 4 * H), E(slabs, H), Z(1), Z(1)
        assert lib.alignn_egc_bwd_dst(a_gy, pin(M), gptr(P), gptr(Q1), gptr(Q0), a_stat, gptr(eg), gptr(e_red), e_eval, m, *seg, n, H, gptr(GM),
                                      gptr(GP), gptr(gb), gptr(gma), gptr(gpa), st) == 0
        torch.cuda.synchronize()
        reverse_asserts("bwd_dst" + tag, GM, GP, gb, gma, gpa, 1)
        bd, gpa = GP[:, H:2 * H].clone(), Z(1)
        assert lib.alignn_egc_bwd_src(gptr(GM), pin(M), gptr(Q1), gptr(g.out_ptr), gptr(g.out_slot), gptr(g.dst), n, H, gptr(GP), gptr(gpa), st) == 0
        torch.cuda.synchronize()
        ent = "bwd_dst+bwd_src" + tag
        rep.close(ent, "GP", GP[:, :3 * H], r64["GP"], r32.get("GP"), B_REVERSE, fl)
        if not torch.equal(GP[:, H:2 * H], bd) or float(GP[:, 3 * H:].abs().max()) != 0.0:
            rep.failed.append((ent, "GP", "wrote outside the A and Bh blocks"))
        rep.amax(ent, "gp_amax", gpa[0], torch.cat([GP[:, :H], GP[:, 2 * H:3 * H]], 1))

        if is_line_graph(g):
            groups = g.grp_seg_ptr.numel() - 1
            GM, GP, gb, gma, gpa = EM(), Z(n, 4 * H), E(groups, H), Z(1), Z(1)
            assert lib.alignn_egc_bwd_lg_fused(a_gy, gptr(M), gptr(P), gptr(Q1), gptr(Q0), a_stat, gptr(e_red), e_eval, m, gptr(g.grp_seg_ptr),
                                               gptr(g.grp_src_ptr), groups, gptr(g.seg_ptr), gptr(g.seg_node), gptr(g.dst), gptr(g.out_ptr),
                                               gptr(g.out_slot), H, gptr(GM), gptr(GP), gptr(gb), gptr(gma), gptr(gpa), st) == 0
            torch.cuda.synchronize()
            reverse_asserts("bwd_lg_fused" + tag, GM, GP, gb, gma, gpa, 3)
            GM, GP, gb, gma, gpa = EM(), Z(n, 4 * H), E(groups, H), Z(1), Z(1)
            assert lib.alignn_egc_bwd_lg_dense(a_gy, gptr(M), gptr(P), gptr(Q1), gptr(Q0), a_stat, gptr(e_red), e_eval, m, gptr(g.grp_seg_ptr),
                                               gptr(g.grp_src_ptr), groups, g.dense_max_src, gptr(g.seg_ptr), gptr(g.seg_node), H, gptr(GM),
                                               gptr(GP), gptr(gb), gptr(gma), gptr(gpa), st) == 0
            torch.cuda.synchronize()
            reverse_asserts("bwd_lg_dense" + tag, GM, GP, gb, gma, gpa, 3)
        del r64, r32
    rep.finish()


SMALL = ("lg_small", "lg_deg17", "bond", "synthetic")
CASES = ([(H, gname, "normal") for H in HS for gname in SMALL]
         + [(H, gname, data) for H in (100, 256, 1024) for gname in ("lg_small", "synthetic") for data in ref.DATA[1:]]
         + [(36, "one_atom_cell", "normal"), (260, "one_atom_cell", "normal"), (4, "one_segment", "normal"),
            (260, "one_segment", "constant_column"), (4, "no_edges", "normal"), (260, "no_edges", "normal"),
            (64, "lg_4096seg", "normal"), (260, "lg_4096seg", "column_offset"),
            (256, "lg_stream", "normal"), (256, "lg_stream", "saturated_gates")])


@pytest.mark.parametrize("H,gname,data", CASES)
def test_entry_points_against_float64(H, gname, data):
    """Every output of the entry points of csrc/conv.hip against the float64 restatements: the four gate forward passes with
    the statistics alignn_bn_finalize_welford makes of their pivot slabs, the node quotient reverse, alignn_bn_silu_bwd_reduce
    + alignn_bn_bwd_finalize, and alignn_egc_bwd_dst + alignn_egc_bwd_src in MODE 0, MODE 1 with batch and with frozen
    statistics and MODE 2 - on line graphs alignn_egc_bwd_lg_fused and alignn_egc_bwd_lg_dense too.  ``one_atom_cell`` is
    the sensitivity of the dense kernel's excluded-entry row formula (a segment that omits its own self-image source:
    tests/gate_parity.graph asserts there is one); ``no_edges`` the zero-row launches.  See the module docstring for the
    bounds; the worst error per entry point and output is printed."""
    _run_case(H, gname, data)


@pytest.mark.parametrize("H", [0, 2, 6, 1028, 64])
def test_unsupported_calls_are_refused(H):
    """hipErrorInvalidValue and no launch (every output buffer keeps its fill) at widths outside H % 4 == 0, 4 <= H <= 1024,
    from every entry point; at a supported width (64) from the calls that miss a required argument."""
    rep = Report(f"refusals H={H}", "conv-bn-parity")
    lib = rep.launcher(_lib.load())
    g = guard_graph(graph("lg_small"))
    n, m, W = g.n_nodes, g.n_edges, 1032
    groups = g.grp_seg_ptr.numel() - 1
    slabs = lib.alignn_egc_slabs(n)
    st = stream()
    I = lambda *s: guard_input(torch.randn(*s, device=DEV))  # noqa: E731, E741
    P, M, Y, Q1, Q0, S0, stat, red = I(n, 4 * W), I(m, W), I(m, W), I(n, W), I(n, W), guard_input(I(n, W).abs()), I(4, W), I(2, W)
    m_before = M.clone()
    outs = [guarded(s, fill=7.0, row=W) for s in ((m, W), (n, 4 * W), (n, W), (n, W), (n, W), (max(slabs, groups) * (3 * W + 1),),
                                                       (slabs * (3 * W + 1),), (2,), (2,))]
    em, gp, na, nb, nc, part_a, part_b, am, am_b = outs
    seg = (gptr(g.seg_ptr), gptr(g.seg_node), gptr(g.src))
    lg = (gptr(g.grp_seg_ptr), gptr(g.grp_src_ptr))

    def fused(h, n_groups):
        return lib.alignn_egc_bwd_lg_fused(gptr(Y), gptr(M), gptr(P), gptr(Q1), gptr(Q0), gptr(stat), gptr(red), 0, m, *lg, n_groups,
                                           gptr(g.seg_ptr), gptr(g.seg_node), gptr(g.dst), gptr(g.out_ptr), gptr(g.out_slot), h, gptr(em),
                                           gptr(gp), gptr(part_a), gptr(am), gptr(am_b), st)

    def dense(h, n_groups, max_src):
        return lib.alignn_egc_bwd_lg_dense(gptr(Y), gptr(M), gptr(P), gptr(Q1), gptr(Q0), gptr(stat), gptr(red), 0, m, *lg, n_groups, max_src,
                                           gptr(g.seg_ptr), gptr(g.seg_node), h, gptr(em), gptr(gp), gptr(part_a), gptr(am), gptr(am_b), st)

    def pre_norm(h, e_stat, yout):
        return lib.alignn_egc_gate_fwd_pre_norm(gptr(P), gptr(M), *seg, n, m, h, gptr(na), gptr(nb), gptr(nc), gptr(part_b), gptr(e_stat), gptr(Y),
                                                gptr(yout), gptr(am), st)

    def infer(h, e_stat, yout):
        return lib.alignn_egc_gate_infer(gptr(P), gptr(M), *seg, n, m, h, gptr(na), gptr(e_stat), gptr(Y), gptr(yout), gptr(am), st)

    if H == 64:
        rc = [fused(H, 0), dense(H, 0, g.dense_max_src), dense(H, groups, 0), pre_norm(H, None, em), pre_norm(H, stat, None),
              infer(H, None, em)]
    else:
        rc = [
            lib.alignn_egc_gate_fwd(gptr(P), gptr(M), *seg, n, m, H, gptr(na), gptr(nb), gptr(nc), gptr(part_a), gptr(part_b), st),
            lib.alignn_egc_gate_fwd_pre(gptr(P), gptr(M), *seg, n, m, H, gptr(na), gptr(nb), gptr(nc), gptr(part_a), gptr(part_b), st),
            pre_norm(H, stat, em), infer(H, stat, em), infer(H, None, None),
            lib.alignn_egc_node_bwd(gptr(Q1), W, gptr(S0), gptr(Q0), gptr(na), gptr(nb), n, H, st),
            lib.alignn_egc_bwd_dst(gptr(Y), gptr(M), gptr(P), gptr(Q1), gptr(Q0), gptr(stat), None, gptr(red), 0, m, *seg, n, H, gptr(em), gptr(gp),
                                   gptr(part_a), gptr(am), gptr(am_b), st),
            lib.alignn_egc_bwd_dst(None, gptr(M), gptr(P), gptr(Q1), gptr(Q0), None, None, None, 0, m, *seg, n, H, gptr(em), gptr(gp),
                                   gptr(part_a), gptr(am), gptr(am_b), st),
            lib.alignn_egc_bwd_src(gptr(Y), gptr(M), gptr(Q1), gptr(g.out_ptr), gptr(g.out_slot), gptr(g.dst), n, H, gptr(gp), gptr(am), st),
            fused(H, groups), dense(H, groups, g.dense_max_src),
        ]
    torch.cuda.synchronize()
    assert rc == [INVALID] * len(rc), rc
    assert all(bool((t == 7.0).all()) for t in outs) and torch.equal(M, m_before)
    rep.finish()  # (and nothing beside them either)
