"""csrc/norm.hip - column statistics, BatchNorm1d + SiLU and LayerNorm + SiLU forward and backward, the column and slab sums -
against the float64 torch restatements of tests/norm_ref.py (checked on their own by tests/test_norm_ref.py), entry point by entry
point and output by output through the raw C ABI.  The other tests of these kernels reach float64 through whole layers on N(0,1)
data, or pin bit-identity between variants; here every launch is one entry point on the float32 operands the restatement sees.

Bounds.  A quantity an existing test bounds keeps that bound: pivot-slab statistics those of tests/test_gpu_round3.py::
test_welford_column_statistics_are_well_conditioned with the second mean term of tests/test_gpu_conv_bn.py (mean within
2e-7 (max |mean| + 1) + 3.5e-6 max |x - mean|, rstd and scale 1e-4 relative in every column, running variance 1e-5 relative,
shift == beta, counts sum to the rows); GX and GS1 of the BatchNorm backward 2e-5 (tests/test_gpu_round3.py); the parameter sums
2e-5 (tests/test_gpu_conv_bn.py); LayerNorm y 1e-5, gx / dgamma / dbeta 1e-4 (tests/test_gpu_model.py).  On N(0,1)-like data
(``normal``) these are the whole allowance; on every other distribution the SAME restatement is evaluated in float32 on the
identical operands and the kernel may be 4x as far from float64 as that, plus the bound as a floor (tests/gate_parity.Report.close).
Outputs no test bounded before (BatchNorm y, GS0, the saved LayerNorm rows, GS1 / GS0 of the LayerNorm node form, the
evaluation-mode stat block, column sums) take 4x the float32 restatement, on every distribution, plus a floor B_* about a decade
above the worst error measured on ``normal`` data (profiles/norm_float64_parity.txt: y 1.5e-7, GS0 3.9e-7, LayerNorm mean / rstd
1.9e-7, its GS1 / GS0 2.9e-7, evaluation-mode rstd / scale 1.2e-7, column sums 3.2e-7).  Errors are max |a - b| / max |b| over the
whole tensor unless said otherwise; column sums are measured against the largest column sum of MAGNITUDES (the training-mode
BatchNorm gradient sums to zero in every column up to the rounding of red, so the sum itself is no scale).  With one or two rows
the training-mode gradient itself is zero in exact arithmetic (one row: z = beta; two rows: xhat = +-1 whatever x is, up to
eps / var): GX, GS1, GS0 and the column sums are measured there against the terms scale * gz whose rounding they hold.

The plain sum / sum-of-squares slabs (alignn_col_stats + alignn_bn_finalize) take the variance as E[x^2] - mean^2 from float32
partial sums: its absolute error is c 2^-24 E[x^2] with c of a few, so rstd is off by c 2^-25 E[x^2] / (var + eps) relative.  They
are held to the pivot slabs' bounds on the well-conditioned distributions PLAIN_DATA, rstd, scale and the running variance in the
columns where E[x^2] <= PLAIN_RATIO (var + eps) with PLAIN_RATIO = 30 (c 9e-7 of rstd, c 1.8e-6 of the running variance) - which
is every column from 31 rows on (asserted; with one or two rows var can be anything against mean^2) -, the means in every column.
What they lose elsewhere - |mean| / std = 30, exactly constant columns - is printed as ``norm-plain-slabs`` lines and not
asserted (rstd 4e-5 at |mean| / std = 30 over thousands of rows and 2.5e-4 over 33, 7e-2 on a constant column, no correct digit
at |mean| / std = 3e4: the model takes plain slabs only from projection epilogues, whose outputs are centred).

alignn_slab_fold / alignn_slab_sum accumulate float32 terms in float64 and round once: every element within
2^-24 |ref| + slabs 2^-52 sum |terms| on terms of mixed sign spanning 1e-6 .. 1e6, which a float32 accumulation misses.

Each later pass is handed the float64 result of the earlier one rounded once.  Output buffers are filled with NaN (padding with a
sentinel that must survive); an ``amax`` slot, zeroed before the launch, must EQUAL the largest magnitude written.  Inputs and
outputs have leading dimensions wider than F; GX goes into the last quarter of a [rows, 4F] buffer, as the model's does.

Shapes (Q = F / 4 quads, RP = 256 / Q rows in flight per workgroup, slabs = min(ceil(rows / 32), 1024)) - the smallest at
which each branch is live:
* F = 4: Q 1, RP 256; 12: Q 3, RP 85, one idle thread; 368: Q 92, RP 2, 72 idle threads; 1020: Q 255, RP 1; 1024: Q 256.  F = 12,
  368, 1020 are the non-power-of-two RowQuad (its 32-bit branch: rows Q < 2^31; the 64-bit one needs 8 GiB per tensor and stays
  untested), 4 and 1024 the shift branch.
* rows 1, 2 (one or two rows: the unbiased / biased running variance), 31 (a slab not full), 33 (two slabs; at F = 4, 12 the
  second one is empty: rows < slabs RP).
* (4100, 1024) and (70001, 64): rows > 4 slabs RP, the four-way unrolled loop of col_reduce_kernel plus its tail;
  (32769, 256): 1025 row groups on 1024 slabs, the slab stride wraps.
* rows 16383 / 16384 at F = 256: element-wise / column-walking form of alignn_bn_silu_fwd.
* (32768, 1024) and (131072, 256): rows F 4 = 128 MiB, the STREAM instantiations (two distributions only: the largest shapes).
* finalisers: slabs 1, 2, 63, 64, 65, 129, 256, 257, 1024 (the 4-slab batched loads of the Welford finaliser from 193 slabs, the
  8-slab ones of bn_finalize / slab_sum from 449).
* LayerNorm: F = 4, 64, 252, 256, 260, 768, 1020, 1024 (every NC, a partial last chunk), rows 0 (the zero slab), 1, 3 (waves of
  the only workgroup without a row), 4097 and 9001 (more than one sweep of 1024 workgroups x 4 waves)."""

import pytest
import torch

pytestmark = pytest.mark.gpu

from alignn_amd import _lib  # noqa: E402
from alignn_amd._lib import ptr, stream  # noqa: E402
from tests import norm_ref as ref  # noqa: E402
from tests.gate_parity import Report  # noqa: E402

DEV = "cuda"
TAG = "norm-parity"
INVALID = 1  # hipErrorInvalidValue
NAN, SENTINEL = float("nan"), 7.0
MEAN_DEV = 3.5e-6  # tests/test_gpu_conv_bn.py
B_APPLY, B_RED, B_LN_Y, B_LN_BWD = 2e-5, 2e-5, 1e-5, 1e-4  # inherited (module docstring)
B_FWD, B_GS0, B_LN_NODE, B_LN_STAT, B_EVAL, B_SUM = 2e-6, 4e-6, 4e-6, 2e-6, 2e-6, 3e-6  # floors of outputs not bounded before
PLAIN_RATIO, PLAIN_DATA = 30.0, ("normal", "saturated", "gamma30", "tiny", "outlier")

E = lambda *s: torch.full(s, NAN, device=DEV)  # noqa: E731  (an output: whatever is not written fails)
Z = lambda *s: torch.zeros(*s, device=DEV)  # noqa: E731
d = lambda t: t.double()  # noqa: E731


def _wide(t, extra):
    """t as a view with leading dimension F + extra (the padding holds the sentinel)"""
    rows, F = t.shape
    buf = torch.full((max(rows, 1), F + extra), SENTINEL, device=DEV)
    buf[:rows, :F] = t
    return buf[:rows, :F]


def _out(rows, F, before=4, after=8):
    """(buffer, view) of a NaN-filled [rows, F] output inside a sentinel-filled wider buffer"""
    buf = torch.full((max(rows, 1), before + F + after), SENTINEL, device=DEV)
    buf[:, before:before + F] = NAN
    return buf, buf[:rows, before:before + F]


def _padding_kept(rep, ent, buf, F, before=4):
    if not (bool((buf[:, :before] == SENTINEL).all()) and bool((buf[:, before + F:] == SENTINEL).all())):
        rep.failed.append((ent, "wrote outside its F columns"))


def _rel(a, b):
    """largest element-wise relative error"""
    return float(((d(a) - d(b)).abs() / d(b).abs().clamp_min(1e-30)).max())


def _stat_asserts(rep, ent, stat, rm, rv, want, beta, x64, cols=None):
    """[4, F] stat and the running statistics out of a training-mode finaliser against float64.  ``cols``: the columns rstd, scale
    and the running variance are held to (all of them when None); the means are held in every column."""
    mean, rstd, scale, rmean, rvar = (want[k] for k in ("mean", "rstd", "scale", "rm", "rv"))
    c = slice(None) if cols is None else cols
    dev = MEAN_DEV * float((x64 - mean).abs().max())
    rep.record(ent, "mean", float((d(stat[0]) - mean).abs().max()), None, 2e-7 * (float(mean.abs().max()) + 1.0) + dev)
    rep.record(ent, "rmean", float((d(rm) - rmean).abs().max()), None, 2e-7 * (float(rmean.abs().max()) + 1.0) + ref.MOMENTUM * dev)
    if cols is None or bool(cols.any()):
        rep.record(ent, "rstd", _rel(stat[1][c], rstd[c]), None, 1e-4)
        rep.record(ent, "scale", _rel(stat[2][c], scale[c]), None, 1e-4)
        rep.record(ent, "rvar", _rel(rv[c], rvar[c]), None, 1e-5)
    if not torch.equal(stat[3], beta):
        rep.failed.append((ent, "shift is not beta"))


def _statistics(rep, lib, x, o, data):
    """alignn_col_stats_welford -> alignn_bn_finalize_welford and alignn_col_stats -> alignn_bn_finalize on x; returns the
    float64 training-mode stat block"""
    rows, F = x.shape
    st = stream()
    gamma, beta = o["gamma"], o["beta"]
    s64, var64 = ref.bn_stat(d(x), d(gamma), d(beta))
    rm64, rv64 = ref.running_update(d(o["rm"]), d(o["rv"]), s64[0], var64, rows)
    want = dict(mean=s64[0], rstd=s64[1], scale=s64[2], rm=rm64, rv=rv64)
    slabs = lib.alignn_col_stats_slabs(rows)
    part, stat, rm, rv = E(slabs * (3 * F + 1)), E(4, F), o["rm"].clone(), o["rv"].clone()
    assert lib.alignn_col_stats_welford(ptr(x), x.stride(0), rows, F, ptr(part), st) == 0
    assert lib.alignn_bn_finalize_welford(ptr(part), slabs, rows, F, ptr(gamma), ptr(beta), ref.EPS_BN, ref.MOMENTUM, ptr(rm), ptr(rv),
                                          ptr(stat), st) == 0
    torch.cuda.synchronize()
    counts = part[slabs * 3 * F:]
    if float(counts.sum()) != rows or not bool(torch.isfinite(part).all()):
        rep.failed.append(("welford", "slab counts / unwritten slab", counts.tolist(), rows))
    _stat_asserts(rep, "welford", stat, rm, rv, want, beta, d(x))
    # plain slabs
    part, stat, rm, rv = E(slabs, 2, F), E(4, F), o["rm"].clone(), o["rv"].clone()
    assert lib.alignn_col_stats(ptr(x), x.stride(0), rows, F, ptr(part), st) == 0
    assert lib.alignn_bn_finalize(ptr(part), slabs, rows, F, ptr(gamma), ptr(beta), ref.EPS_BN, ref.MOMENTUM, ptr(rm), ptr(rv), ptr(stat),
                                  st) == 0
    torch.cuda.synchronize()
    cols = (d(x) ** 2).mean(0) <= PLAIN_RATIO * (var64 + ref.EPS_BN)
    if data in PLAIN_DATA:
        if rows >= 31 and not bool(cols.all()):
            rep.failed.append(("plain", "a well-conditioned distribution has ill-conditioned columns", int((~cols).sum())))
        _stat_asserts(rep, "plain", stat, rm, rv, want, beta, d(x), cols)
    if data not in PLAIN_DATA or not bool(cols.all()):  # what the plain slabs lose where they are not held to a bound
        bad = ~cols if data in PLAIN_DATA else torch.ones_like(cols)
        print(f"norm-plain-slabs {rep.case:<38s} {int(bad.sum())} of {F} columns not asserted ({int((~cols).sum())} with E[x^2] > "
              f"{PLAIN_RATIO:g} (var + eps)): mean err {float((d(stat[0]) - s64[0]).abs().max()):8.2e}  rstd err "
              f"{_rel(stat[1][bad], s64[1][bad]):8.2e}  running var err {_rel(rv[bad], rv64[bad]):8.2e}")
    return s64


def _bn_case(rows, F, data):
    lib = _lib.load()
    st = stream()
    rep = Report(f"bn rows={rows} F={F} {data}", TAG)
    o = ref.operands(rows, F, data, DEV, "bn")
    own = (lambda t: t) if data != "normal" else (lambda t: None)  # noqa: E731  (an inherited bound stands alone on N(0,1)-like data)
    x, gy, r = _wide(o["x"], 4), _wide(o["gy"], 8), _wide(o["r"], 12)
    gamma, beta, s0, hh = o["gamma"], o["beta"], o["s0"], o["hh"]
    slabs = lib.alignn_col_stats_slabs(rows)
    s64 = _statistics(rep, lib, x, o, data)
    train = s64.float().contiguous()  # what the later passes are handed: the float64 statistics rounded once
    frozen = ref.eval_stat(d(o["rm"]), d(o["rv"]), d(gamma), d(beta)).float().contiguous()

    # ---- forward: batch statistics without / with the residual, frozen statistics with the residual and no amax slot
    for stat, res, track in ((train, False, True), (train, True, True), (frozen, True, False)):
        ent = "bn_silu_fwd" + (" +R" if res else "") + ("" if stat is train else " frozen")
        buf, y = _out(rows, F)
        am = Z(1)
        assert lib.alignn_bn_silu_fwd(ptr(x), x.stride(0), ptr(r) if res else None, r.stride(0) if res else 0, ptr(stat), ptr(y), y.stride(0),
                                      rows, F, ptr(am) if track else None, st) == 0
        torch.cuda.synchronize()
        rep.close(ent, "Y", y, ref.bn_silu_fwd(d(x), d(r) if res else None, d(stat)), ref.bn_silu_fwd(x, r if res else None, stat), B_FWD)
        _padding_kept(rep, ent, buf, F)
        if track:
            rep.amax(ent, "amax", am[0], y)

    # ---- backward: parameter sums, then the three forms of the input gradient
    for stat, ev in ((train, 0), (frozen, 1)):
        tag = " frozen" if ev else ""
        red64 = ref.bn_bwd_red(d(gy), d(x), d(stat))
        part, red = E(slabs, 2, F), E(2, F)
        assert lib.alignn_bn_silu_bwd_reduce(ptr(gy), gy.stride(0), ptr(x), x.stride(0), ptr(stat), rows, F, ptr(part), st) == 0
        assert lib.alignn_bn_bwd_finalize(ptr(part), slabs, F, ptr(red), st) == 0
        torch.cuda.synchronize()
        rep.close("bn_silu_bwd_reduce" + tag, "red", red, red64, own(ref.bn_bwd_red(gy, x, stat)), B_RED)
        red_in = red64.float().contiguous()
        g64 = ref.bn_bwd_apply(d(gy), d(x), d(stat), d(red_in), ev)
        g32 = ref.bn_bwd_apply(gy, x, stat, red_in, ev)
        n64 = ref.node_adjoints(g64, d(s0), d(hh))
        n32 = ref.node_adjoints(g32, s0, hh)
        # One or two rows in training mode: the gradient is zero in exact arithmetic (one row: z = beta; two rows: xhat = +-1
        # whatever x is, up to eps / var) and both sides hold the rounding of its terms scale * gz, which is what the errors
        # are measured against there
        terms = ref.bn_bwd_apply(d(gy), d(x), d(stat), None, True) if (rows <= 2 and not ev) else None
        t1 = None if terms is None else terms / (d(s0) + ref.EPS_GATE)
        fx, f1, f0 = (1e-30,) * 3 if terms is None else (float(t.abs().max()) for t in (terms, t1, t1 * d(hh)))
        GP = [Z(rows, 4 * F) for _ in range(3)]
        GX = [g[:, 3 * F:] for g in GP]
        am = [Z(1) for _ in range(3)]
        gs1, gs0, gpart, sums = E(rows, F), E(rows, F), E(slabs, F), E(F)
        head = (ptr(gy), gy.stride(0), ptr(x), x.stride(0), ptr(stat))
        assert lib.alignn_bn_silu_bwd_apply(*head, ptr(gamma), ptr(red_in), ev, ptr(GX[0]), 4 * F, rows, F, ptr(am[0]), st) == 0
        assert lib.alignn_bn_silu_bwd_apply_node(*head, ptr(gamma), ptr(red_in), ev, ptr(GX[1]), 4 * F, rows, F, ptr(am[1]), ptr(s0), ptr(hh),
                                                 ptr(gs1), ptr(gs0), st) == 0
        assert lib.alignn_bn_silu_bwd_apply_sum(*head, None if ev else ptr(red_in), ev, ptr(GX[2]), 4 * F, rows, F, ptr(am[2]), ptr(gpart),
                                                st) == 0
        assert lib.alignn_slab_sum(ptr(gpart), slabs, F, ptr(sums), st) == 0
        torch.cuda.synchronize()
        ent = "bn_silu_bwd_apply" + tag
        rep.close(ent, "GX", GX[0], g64, own(g32), B_APPLY, fx)
        rep.amax(ent, "amax", am[0][0], GX[0])
        for k, name in ((1, "_node"), (2, "_sum")):  # the same bits from the three forms; nothing outside the last quarter
            if not (torch.equal(GP[k], GP[0]) and torch.equal(am[k], am[0])):
                rep.failed.append((ent + name, "GX / amax differ from alignn_bn_silu_bwd_apply's"))
        if float(GP[0][:, :3 * F].abs().max()) != 0.0:
            rep.failed.append((ent, "wrote outside the last quarter"))
        rep.close("bn_silu_bwd_apply_node" + tag, "GS1", gs1, n64[0], own(n32[0]), B_APPLY, f1)
        rep.close("bn_silu_bwd_apply_node" + tag, "GS0", gs0, n64[1], n32[1], B_GS0, f0)
        # column sums: against the sum of magnitudes (in training mode the sum itself is zero up to the rounding of red)
        fl = float((g64 if terms is None else terms).abs().sum(0).max())
        rep.close("bn_silu_bwd_apply_sum" + tag, "colsum", sums, g64.sum(0), g32.sum(0), B_SUM, fl)
    rep.finish()


BN_SHAPES = [(rows, F) for F in (4, 12, 368, 1020, 1024) for rows in (1, 2, 31, 33)] + [
    (4100, 1024), (70001, 64), (32769, 256), (16383, 256), (16384, 256)]
BN_CASES = ([(rows, F, "normal") for rows, F in BN_SHAPES]
            + [(rows, F, data) for rows, F in ((33, 368), (4099, 64), (16384, 256)) for data in ref.DATA[1:]]
            + [(rows, F, data) for rows, F in ((32768, 1024), (131072, 256)) for data in ("normal", "offset30")])


@pytest.mark.parametrize("rows,F,data", BN_CASES)
def test_batchnorm_entry_points_against_float64(rows, F, data):
    """alignn_col_stats_welford + alignn_bn_finalize_welford, alignn_col_stats + alignn_bn_finalize, alignn_bn_silu_fwd (without and
    with a residual, batch and frozen statistics, with and without an amax slot), alignn_bn_silu_bwd_reduce +
    alignn_bn_bwd_finalize, alignn_bn_silu_bwd_apply / _apply_node / _apply_sum + alignn_slab_sum in training and evaluation
    mode.  See the module docstring for shapes and bounds; the worst error per entry point and output is printed."""
    _bn_case(rows, F, data)


@pytest.mark.parametrize("data", ["normal", "offset30", "constant", "offset300"])
@pytest.mark.parametrize("rows,F", [(2016, 64), (2048, 64), (2049, 12), (8192, 64), (8193, 368), (32769, 64)])
def test_column_statistics_against_float64(rows, F, data):
    """The two statistics passes alone, at the slab counts where the finalisers change path (63, 64, 65: the 64 slab-lanes;
    256, 257: the 4-slab batched loads of the Welford finaliser; 1024: the 8-slab ones of alignn_bn_finalize), on
    ``offset300`` too - |mean| / std = 3e4, where only the data's own float32 resolution limits the pivot slabs."""
    lib = _lib.load()
    rep = Report(f"stats rows={rows} F={F} {data}", TAG)
    o = ref.operands(rows, F, data, DEV, "bn")
    _statistics(rep, lib, _wide(o["x"], 4), o, data)
    rep.finish()


def test_welford_finaliser_skips_empty_leading_slabs():
    """Slabs whose count is 0 hold no pivot: alignn_bn_finalize_welford takes its common pivot from the first slab that has
    rows.  The gate passes can leave such slabs in front (alignn_col_stats_welford only behind: rows < slabs RP, the (33, 4)
    case); here 3 and 70 empty slabs with a poisoned pivot are put in front of the ones the statistics pass wrote."""
    lib = _lib.load()
    rows, F = 4099, 64
    o = ref.operands(rows, F, "offset30", DEV, "bn")
    x, gamma, beta = o["x"], o["gamma"], o["beta"]
    slabs = lib.alignn_col_stats_slabs(rows)
    part = E(slabs * (3 * F + 1))
    assert lib.alignn_col_stats_welford(ptr(x), F, rows, F, ptr(part), stream()) == 0
    s64, var64 = ref.bn_stat(d(x), d(gamma), d(beta))
    rm64, rv64 = ref.running_update(d(o["rm"]), d(o["rv"]), s64[0], var64, rows)
    for lead in (3, 70):
        rep = Report(f"welford {lead} empty slabs in front", TAG)
        empty = torch.full((lead, 3, F), 1e30, device=DEV)
        empty[:, 1:] = 0.0
        both = torch.cat([empty.reshape(-1), part[:slabs * 3 * F], Z(lead), part[slabs * 3 * F:]])
        stat, rm, rv = E(4, F), o["rm"].clone(), o["rv"].clone()
        assert lib.alignn_bn_finalize_welford(ptr(both), slabs + lead, rows, F, ptr(gamma), ptr(beta), ref.EPS_BN, ref.MOMENTUM, ptr(rm),
                                              ptr(rv), ptr(stat), stream()) == 0
        torch.cuda.synchronize()
        _stat_asserts(rep, "welford", stat, rm, rv, dict(mean=s64[0], rstd=s64[1], scale=s64[2], rm=rm64, rv=rv64), beta, d(x))
        rep.finish()


@pytest.mark.parametrize("F", [4, 368, 1024])
def test_evaluation_mode_finalize(F):
    """alignn_bn_finalize with slabs == 0 (the angle embedding's finalisers, the inference path): the stat block comes from the
    running statistics - mean and shift bit for bit -, which stay bit-unchanged; gamma == NULL is 1 and beta == NULL is 0."""
    lib = _lib.load()
    rep = Report(f"eval finalize F={F}", TAG)
    o = ref.operands(5, F, "normal", DEV, "bn")
    for g, b in ((o["gamma"], o["beta"]), (None, o["beta"]), (o["gamma"], None), (None, None)):
        stat, rm, rv = E(4, F), o["rm"].clone(), o["rv"].clone()
        assert lib.alignn_bn_finalize(None, 0, 12345, F, ptr(g), ptr(b), ref.EPS_BN, ref.MOMENTUM, ptr(rm), ptr(rv), ptr(stat), stream()) == 0
        torch.cuda.synchronize()
        assert torch.equal(rm, o["rm"]) and torch.equal(rv, o["rv"])
        w64 = ref.eval_stat(d(rm), d(rv), None if g is None else d(g), None if b is None else d(b))
        w32 = ref.eval_stat(rm, rv, g, b)
        ent = f"bn_finalize eval{'' if g is not None else ' -gamma'}{'' if b is not None else ' -beta'}"
        assert torch.equal(stat[0], rm) and torch.equal(stat[3], w32[3])
        rep.record(ent, "rstd", _rel(stat[1], w64[1]), _rel(w32[1], w64[1]), 4 * _rel(w32[1], w64[1]) + B_EVAL)
        rep.record(ent, "scale", _rel(stat[2], w64[2]), _rel(w32[2], w64[2]), 4 * _rel(w32[2], w64[2]) + B_EVAL)
    rep.finish()


# ----------------------------------------------------------------------------------------------------------------------
# LayerNorm
# ----------------------------------------------------------------------------------------------------------------------
def _ln_case(rows, F, data):
    lib = _lib.load()
    st = stream()
    rep = Report(f"ln rows={rows} F={F} {data}", TAG)
    o = ref.operands(rows, F, data, DEV, "ln")
    own = (lambda t: t) if data != "normal" else (lambda t: None)  # noqa: E731  (an inherited bound stands alone on N(0,1)-like data)
    x, gy, r = _wide(o["x"], 4), _wide(o["gy"], 8), _wide(o["r"], 12)
    gamma, beta, s0, hh = o["gamma"], o["beta"], o["s0"], o["hh"]
    _, s64 = ref.ln_silu_fwd(d(x), None, d(gamma), d(beta))
    s32 = ref.ln_silu_fwd(x, None, gamma, beta)[1]
    first = None
    for res, keep in ((False, True), (True, True), (True, False)):  # (the last: no stats rows, no amax slot - inference)
        ent = "ln_silu_fwd" + (" +R" if res else "") + ("" if keep else " -stats")
        buf, y = _out(rows, F)
        stats, am = E(max(rows, 1), 2), Z(1)
        assert lib.alignn_ln_silu_fwd(ptr(x), x.stride(0), ptr(r) if res else None, r.stride(0) if res else 0, ptr(gamma), ptr(beta), ref.EPS_LN,
                                      ptr(y), y.stride(0), ptr(stats) if keep else None, rows, F, ptr(am) if keep else None, st) == 0
        torch.cuda.synchronize()
        _padding_kept(rep, ent, buf, F)
        if not keep:
            if not torch.equal(y, first):
                rep.failed.append((ent, "Y differs from the call with stats"))
            continue
        first = y
        y32 = ref.ln_silu_fwd(x, r if res else None, gamma, beta)[0]
        rep.close(ent, "Y", y, ref.ln_silu_fwd(d(x), d(r) if res else None, d(gamma), d(beta))[0], own(y32), B_LN_Y)
        rep.amax(ent, "amax", am[0], y)
        if rows:
            rep.close(ent, "mean", stats[:rows, 0], s64[:, 0], s32[:, 0], B_LN_STAT, 1.0)
            e32 = _rel(s32[:, 1], s64[:, 1])
            rep.record(ent, "rstd", _rel(stats[:rows, 1], s64[:, 1]), e32, B_LN_STAT + 4 * e32)
    # ---- backward, handed the float64 statistics rounded once
    stats_in = torch.cat([s64.float(), Z(1, 2)]).contiguous()  # (never a NULL pointer)
    b64 = ref.ln_silu_bwd(d(gy), d(x), d(gamma), d(beta), d(stats_in[:rows]))
    b32 = ref.ln_silu_bwd(gy, x, gamma, beta, stats_in[:rows])
    n64 = ref.node_adjoints(b64[0], d(s0), d(hh))
    n32 = ref.node_adjoints(b32[0], s0, hh)
    slabs = lib.alignn_ln_slabs(rows)
    GP = [Z(max(rows, 1), 4 * F) for _ in range(2)]
    GX = [g[:rows, 3 * F:] for g in GP]
    am, part, red = [Z(1) for _ in range(2)], [E(slabs, 2, F) for _ in range(2)], [E(2, F) for _ in range(2)]
    gs1, gs0 = E(max(rows, 1), F), E(max(rows, 1), F)
    head = (ptr(gy), gy.stride(0), ptr(x), x.stride(0), ptr(gamma), ptr(beta), ptr(stats_in))
    assert lib.alignn_ln_silu_bwd(*head, ptr(GX[0]), 4 * F, ptr(part[0]), rows, F, ptr(am[0]), st) == 0
    assert lib.alignn_ln_silu_bwd_node(*head, ptr(GX[1]), 4 * F, ptr(part[1]), rows, F, ptr(am[1]), ptr(s0 if rows else gs1), ptr(hh if rows else gs1),
                                       ptr(gs1), ptr(gs0), st) == 0
    for k in range(2):
        assert lib.alignn_bn_bwd_finalize(ptr(part[k]), slabs, F, ptr(red[k]), st) == 0
    torch.cuda.synchronize()
    ent = "ln_silu_bwd"
    if not (torch.equal(GP[0], GP[1]) and torch.equal(am[0], am[1]) and torch.equal(part[0], part[1]) and torch.equal(red[0], red[1])):
        rep.failed.append((ent + "_node", "GX / amax / slabs differ from alignn_ln_silu_bwd's"))
    if float(GP[0][:, :3 * F].abs().max()) != 0.0:
        rep.failed.append((ent, "wrote outside the last quarter"))
    rep.amax(ent, "amax", am[0][0], GX[0])
    if rows == 0:  # the zero slab is written, and its sums are zero
        assert slabs == 1 and not bool(part[0].any()) and not bool(red[0].any())
        assert bool(torch.isnan(gs1).all()) and bool(torch.isnan(gs0).all())
    else:
        rep.close(ent, "GX", GX[0], b64[0], own(b32[0]), B_LN_BWD)
        rep.close(ent, "dbeta", red[0][0], b64[1], own(b32[1]), B_LN_BWD)
        rep.close(ent, "dgamma", red[0][1], b64[2], own(b32[2]), B_LN_BWD)
        rep.close(ent + "_node", "GS1", gs1[:rows], n64[0], n32[0], B_LN_NODE)
        rep.close(ent + "_node", "GS0", gs0[:rows], n64[1], n32[1], B_LN_NODE)
    rep.finish()


LN_CASES = ([(rows, F, "normal") for F in (4, 64, 252, 256, 260, 768, 1020, 1024) for rows in (0, 1, 3, 4097, 9001)]
            + [(rows, F, data) for rows, F in ((3, 260), (4097, 64), (9001, 1020)) for data in ref.DATA[1:]])


@pytest.mark.parametrize("rows,F,data", LN_CASES)
def test_layernorm_entry_points_against_float64(rows, F, data):
    """alignn_ln_silu_fwd (Y, the saved (mean, rstd) rows, amax; without stats and amax too), alignn_ln_silu_bwd and
    alignn_ln_silu_bwd_node (GX into the last quarter of a [rows, 4F] buffer, GS1, GS0, amax) and alignn_bn_bwd_finalize on their
    slabs (dbeta, dgamma).  rows == 0: the one slab is written as zeros."""
    _ln_case(rows, F, data)


# ----------------------------------------------------------------------------------------------------------------------
# sums
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows", [33, 4100])
@pytest.mark.parametrize("F", [4, 1024, 1028, 2052])
def test_col_sum_against_float64(rows, F):
    """alignn_col_sum in column panels of 1024 (1028: a second panel of one quad; 2052: three panels), ldx > F, the workspace
    sized as ops.col_sum sizes it."""
    lib = _lib.load()
    rep = Report(f"col_sum rows={rows} F={F}", TAG)
    g = torch.Generator(device=DEV).manual_seed(rows + F)
    x = _wide(torch.randn(rows, F, device=DEV, generator=g) * 2 + 0.5, 4)
    ws, out = E(lib.alignn_col_stats_slabs(rows) * 2 * F), torch.full((F + 4,), SENTINEL, device=DEV)
    out[:F] = NAN
    assert lib.alignn_col_sum(ptr(x), x.stride(0), rows, F, ptr(out), ptr(ws), stream()) == 0
    torch.cuda.synchronize()
    rep.close("col_sum", "out", out[:F], d(x).sum(0), x.sum(0), B_SUM, float(d(x).abs().sum(0).max()))
    assert bool((out[F:] == SENTINEL).all())
    rep.finish()


def _slab_terms(slabs, width, seed):
    """terms of mixed sign and magnitudes 1e-6 .. 1e6"""
    g = torch.Generator(device=DEV).manual_seed(seed)
    return torch.randn(slabs, width, device=DEV, generator=g) * 10.0 ** (12 * torch.rand(slabs, width, device=DEV, generator=g) - 6)


def _double_sum_check(rep, ent, got, ref64, absum, slabs):
    allowed = 2.0 ** -24 * ref64.abs() + slabs * 2.0 ** -52 * absum
    worst = float(((d(got) - ref64).abs() / allowed.clamp_min(1e-300)).max())
    f32 = float(((d(got) - ref64).abs() / ref64.abs().clamp_min(1e-300)).max())
    rep.record(ent, "out", worst, None, 1.0 + 1e-9)  # (in units of the derived bound; <= 1)
    print(f"{TAG} {rep.case:<38s} {ent:<32s} largest relative error {f32:8.2e}")


@pytest.mark.parametrize("width", [4, 60, 512])
@pytest.mark.parametrize("slabs", [1, 63, 64, 65, 257, 5283])
def test_slab_fold_against_float64(slabs, width):
    """out[g] = sum of the slabs k = g (mod 64), accumulated in float64; groups g >= slabs come out as exact zeros."""
    lib = _lib.load()
    G = lib.alignn_slab_fold_slabs()
    assert G == ref.FOLD
    rep = Report(f"slab_fold slabs={slabs} width={width}", TAG)
    p, out = _slab_terms(slabs, width, slabs * width), E(G, width)
    assert lib.alignn_slab_fold(ptr(p), slabs, width, ptr(out), stream()) == 0
    torch.cuda.synchronize()
    assert not bool(out[slabs:].any()) and bool(torch.isfinite(out).all())
    _double_sum_check(rep, "slab_fold", out, ref.slab_fold(d(p)), ref.slab_fold(d(p).abs()), slabs)
    rep.finish()


@pytest.mark.parametrize("width", [2, 1027])
@pytest.mark.parametrize("slabs", [1, 64, 65, 449, 513, 5283])
def test_slab_sum_against_float64(slabs, width):
    """out = sum over the slabs, accumulated in float64 (the 8-slab batched loads start at 449 slabs)."""
    lib = _lib.load()
    rep = Report(f"slab_sum slabs={slabs} width={width}", TAG)
    p, out = _slab_terms(slabs, width, slabs + width), torch.full((width + 3,), SENTINEL, device=DEV)
    out[:width] = NAN
    assert lib.alignn_slab_sum(ptr(p), slabs, width, ptr(out), stream()) == 0
    torch.cuda.synchronize()
    assert bool((out[width:] == SENTINEL).all())
    _double_sum_check(rep, "slab_sum", out[:width], ref.slab_sum(d(p)), ref.slab_sum(d(p).abs()), slabs)
    rep.finish()


# ----------------------------------------------------------------------------------------------------------------------
# refusals
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F", [0, 2, 6, 1028, 64])
def test_unsupported_calls_are_refused(F):
    """hipErrorInvalidValue and no launch (every output buffer keeps its fill): widths outside F % 4 == 0, 4 <= F <= 1024 from the
    entry points that take whole quads of at most four chunks (alignn_col_sum takes any multiple of 4); at a supported width (64)
    the calls that miss a required argument, slabs <= 0 / width <= 0 / F <= 0 from the folds, sums and finalisers, rows < 0."""
    lib = _lib.load()
    st = stream()
    rows, W = 40, 1032
    I = lambda *s: torch.randn(*s, device=DEV)  # noqa: E731, E741
    x, gy, r, s0, hh, stat, red, gamma, beta, lnst = I(rows, W), I(rows, W), I(rows, W), I(rows, W).abs(), I(rows, W), I(4, W), I(2, W), I(W), I(W), I(rows, 2)
    rm, rv = I(W), I(W).abs()
    outs = [torch.full(s, SENTINEL, device=DEV) for s in ((rows, W), (rows, W), (rows, W), (64 * (3 * W + 1),), (4, W), (rows, 2), (2,))]
    y, g1, g0, part, ostat, ostats, am = outs
    rm0, rv0 = rm.clone(), rv.clone()

    def calls(F, rows, S0=s0, HH=hh, G1=g1, G0=g0, partial=part, RED=red):
        head = (ptr(gy), W, ptr(x), W, ptr(stat))
        lhead = (ptr(gy), W, ptr(x), W, ptr(gamma), ptr(beta), ptr(lnst))
        return dict(
            col_stats=lambda: lib.alignn_col_stats(ptr(x), W, rows, F, ptr(part), st),
            col_stats_welford=lambda: lib.alignn_col_stats_welford(ptr(x), W, rows, F, ptr(part), st),
            col_sum=lambda: lib.alignn_col_sum(ptr(x), W, rows, F, ptr(y), ptr(part), st),
            bn_silu_fwd=lambda: lib.alignn_bn_silu_fwd(ptr(x), W, ptr(r), W, ptr(stat), ptr(y), W, rows, F, ptr(am), st),
            bwd_reduce=lambda: lib.alignn_bn_silu_bwd_reduce(*head, rows, F, ptr(part), st),
            apply=lambda: lib.alignn_bn_silu_bwd_apply(*head, ptr(gamma), ptr(red), 0, ptr(y), W, rows, F, ptr(am), st),
            apply_node=lambda: lib.alignn_bn_silu_bwd_apply_node(*head, ptr(gamma), ptr(red), 0, ptr(y), W, rows, F, ptr(am), ptr(S0), ptr(HH),
                                                                 ptr(G1), ptr(G0), st),
            apply_sum=lambda: lib.alignn_bn_silu_bwd_apply_sum(*head, ptr(RED), 0, ptr(y), W, rows, F, ptr(am), ptr(partial), st),
            ln_fwd=lambda: lib.alignn_ln_silu_fwd(ptr(x), W, ptr(r), W, ptr(gamma), ptr(beta), ref.EPS_LN, ptr(y), W, ptr(ostats), rows, F, ptr(am), st),
            ln_bwd=lambda: lib.alignn_ln_silu_bwd(*lhead, ptr(y), W, ptr(part), rows, F, ptr(am), st),
            ln_bwd_node=lambda: lib.alignn_ln_silu_bwd_node(*lhead, ptr(y), W, ptr(part), rows, F, ptr(am), ptr(S0), ptr(HH), ptr(G1), ptr(G0), st))

    if F != 64:
        c = calls(F, rows)
        if F == 1028:
            del c["col_sum"]
        rc = {k: f() for k, f in c.items()}
    else:
        rc = {}
        for k in ("col_stats", "col_stats_welford", "col_sum", "bwd_reduce", "apply_sum", "ln_bwd", "ln_bwd_node"):
            rc[k + " rows<0"] = calls(F, -1)[k]()
        for name in ("S0", "HH", "G1", "G0"):
            for k in ("apply_node", "ln_bwd_node"):
                rc[f"{k} {name}=NULL"] = calls(F, rows, **{name: None})[k]()
        rc["apply_sum partial=NULL"] = calls(F, rows, partial=None)["apply_sum"]()
        rc["apply_sum red=NULL"] = calls(F, rows, RED=None)["apply_sum"]()
        fin = lambda fn, p, slabs, n, width, a, b: fn(p, slabs, n, width, ptr(gamma), ptr(beta), ref.EPS_BN, ref.MOMENTUM, a, b, ptr(ostat), st)  # noqa: E731
        for slabs, n, width, tag in ((0, rows, F, "slabs=0"), (-1, rows, F, "slabs<0"), (2, rows, 0, "F=0"), (2, -1, F, "rows<0")):
            rc["finalize_welford " + tag] = fin(lib.alignn_bn_finalize_welford, ptr(x), slabs, n, width, ptr(rm), ptr(rv))
            if slabs != 0:
                rc["finalize " + tag] = fin(lib.alignn_bn_finalize, ptr(x), slabs, n, width, ptr(rm), ptr(rv))
        rc["finalize_welford partial=NULL"] = fin(lib.alignn_bn_finalize_welford, None, 2, rows, F, ptr(rm), ptr(rv))
        rc["finalize eval without running statistics"] = fin(lib.alignn_bn_finalize, None, 0, rows, F, None, None)
        for slabs, width, tag in ((0, F, "slabs=0"), (-1, F, "slabs<0"), (2, 0, "width=0"), (2, -4, "width<0")):
            rc["slab_fold " + tag] = lib.alignn_slab_fold(ptr(x), slabs, width, ptr(y), st)
            rc["slab_sum " + tag] = lib.alignn_slab_sum(ptr(x), slabs, width, ptr(y), st)
            rc["bwd_finalize " + tag] = lib.alignn_bn_bwd_finalize(ptr(x), slabs, width, ptr(y), st)
    torch.cuda.synchronize()
    assert all(v == INVALID for v in rc.values()), rc
    assert all(bool((t == SENTINEL).all()) for t in outs) and torch.equal(rm, rm0) and torch.equal(rv, rv0)


# ----------------------------------------------------------------------------------------------------------------------
# empty batches
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ev", [0, 1])
def test_apply_sum_of_an_empty_batch_writes_the_zero_slab(ev):
    """alignn_col_stats_slabs(0) == 1 and both callers (mlp_bwd of csrc/model.hip, ops.MLPLayerFn) run alignn_slab_sum over that
    one slab for the bias gradient of the Linear in front: alignn_bn_silu_bwd_apply_sum writes it as zeros at rows == 0, as
    alignn_ln_silu_bwd does.  (It returned before the launch and left the slab as allocated: the bias gradient of an empty
    batch was whatever the arena held.)"""
    lib = _lib.load()
    F = 368
    o = ref.operands(4, F, "normal", DEV, "bn")
    stat = ref.eval_stat(o["rm"], o["rv"], o["gamma"], o["beta"]).contiguous()
    assert lib.alignn_col_stats_slabs(0) == 1
    part, sums, gx, am = E(1, F), E(F), E(1, F), Z(1)
    assert lib.alignn_bn_silu_bwd_apply_sum(ptr(o["gy"]), F, ptr(o["x"]), F, ptr(stat), ptr(o["r"][:2].contiguous()), ev, ptr(gx), F, 0, F, ptr(am),
                                            ptr(part), stream()) == 0
    assert lib.alignn_slab_sum(ptr(part), 1, F, ptr(sums), stream()) == 0
    torch.cuda.synchronize()
    assert not bool(part.any()) and not bool(sums.any()) and float(am) == 0.0 and bool(torch.isnan(gx).all())


def test_bwd_reduce_of_an_empty_batch_writes_the_zero_slab():
    """rows == 0: the one slab alignn_bn_bwd_finalize reads is written as zeros.  rows < 0 is refused, as by its siblings (it was
    launched as an empty batch: harmless, no row is read, but not what the other entry points of the file do; the refusal is
    in test_unsupported_calls_are_refused)."""
    lib = _lib.load()
    F = 12
    o = ref.operands(4, F, "normal", DEV, "bn")
    stat = ref.eval_stat(o["rm"], o["rv"], o["gamma"], o["beta"]).contiguous()
    part, red = E(1, 2, F), E(2, F)
    assert lib.alignn_bn_silu_bwd_reduce(ptr(o["gy"]), F, ptr(o["x"]), F, ptr(stat), 0, F, ptr(part), stream()) == 0
    assert lib.alignn_bn_bwd_finalize(ptr(part), 1, F, ptr(red), stream()) == 0
    torch.cuda.synchronize()
    assert not bool(part.any()) and not bool(red.any())


@pytest.mark.parametrize("F", [4, 260])
def test_finalisers_of_an_empty_batch_keep_the_running_statistics(F):
    """rows == 0 in training mode.  The mean of no rows is 0 / 0: both finalisers wrote NaN into stat AND into the running
    statistics, which no later batch repairs (0.9 NaN + 0.1 x).  An empty batch (a line graph without angles) has no statistics
    of its own: it takes the evaluation form - stat from the running statistics, which stay bit-unchanged, as torch's batch_norm
    leaves them on an empty input.  Without running statistics there is nothing to take: refused, stat untouched.
    This is also the only way alignn_bn_finalize_welford meets slabs whose counts are ALL zero from alignn_col_stats_welford
    (the counts sum to the rows).  All-zero counts beside rows > 0 - an inconsistent call - stay finite: the common pivot is
    the last slab's, S = SS = 0, so mean = that pivot and var = 0 (asserted below)."""
    lib = _lib.load()
    st = stream()
    o = ref.operands(4, F, "normal", DEV, "bn")
    gamma, beta = o["gamma"], o["beta"]
    want = ref.eval_stat(d(o["rm"]), d(o["rv"]), d(gamma), d(beta))
    wpart, ppart = E(3 * F + 1), E(1, 2, F)
    assert lib.alignn_col_stats_welford(ptr(o["x"]), F, 0, F, ptr(wpart), st) == 0
    assert lib.alignn_col_stats(ptr(o["x"]), F, 0, F, ptr(ppart), st) == 0
    torch.cuda.synchronize()
    assert not bool(wpart.any()) and not bool(ppart.any())  # zero slabs, count 0
    for fn, part in ((lib.alignn_bn_finalize_welford, wpart), (lib.alignn_bn_finalize, ppart)):
        stat, rm, rv = E(4, F), o["rm"].clone(), o["rv"].clone()
        assert fn(ptr(part), 1, 0, F, ptr(gamma), ptr(beta), ref.EPS_BN, ref.MOMENTUM, ptr(rm), ptr(rv), ptr(stat), st) == 0
        torch.cuda.synchronize()
        assert torch.equal(rm, o["rm"]) and torch.equal(rv, o["rv"])
        assert torch.equal(stat[0], rm) and torch.equal(stat[3], beta)
        assert _rel(stat[1], want[1]) < 1e-6 and _rel(stat[2], want[2]) < 1e-6
        stat = torch.full((4, F), SENTINEL, device=DEV)
        assert fn(ptr(part), 1, 0, F, ptr(gamma), ptr(beta), ref.EPS_BN, ref.MOMENTUM, None, None, ptr(stat), st) == INVALID
        torch.cuda.synchronize()
        assert bool((stat == SENTINEL).all())
    # all-zero counts beside rows > 0
    slabs = 3
    part = Z(slabs * (3 * F + 1))
    part[2 * 3 * F:2 * 3 * F + F] = 1.5  # the last slab's pivot
    stat = E(4, F)
    assert lib.alignn_bn_finalize_welford(ptr(part), slabs, 5, F, ptr(gamma), ptr(beta), ref.EPS_BN, ref.MOMENTUM, None, None, ptr(stat), st) == 0
    torch.cuda.synchronize()
    assert bool((stat[0] == 1.5).all()) and _rel(stat[1], torch.full((F,), ref.EPS_BN ** -0.5, dtype=torch.float64, device=DEV)) < 1e-6
