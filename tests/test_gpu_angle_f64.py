"""csrc/angle.hip - the fused bond-angle embedding, alignn_angle_embed_fwd / _bwd / _infer - against the float64 restatement of
tests/angle_ref.py (checked on its own by tests/test_angle_ref.py), output by output through the C ABI on hard inputs.
tests/test_gpu_angle.py reaches float64 on uniform cosines and default weights at six shapes; here every output the three
entry points write is compared: stat1 / stat2 (mean, rstd, gamma rstd; beta bit for bit), the running statistics, z and max |z|,
red1 / red2 (dbeta, dgamma), gW1, gb1, gW2, gb2, and the evaluation-mode z.

Bounds.  An output tests/test_gpu_angle.py bounds keeps that bound on ``normal`` data, alone: z 2e-6, running statistics 1e-5,
parameter gradients (gW, dbeta, dgamma) 2e-5, gb within 1e-4 max(max |gW|, 1) of zero - at the conditioning those bounds were
set on, from 31 rows and 16 bins on (two rows have the statistics of two points, one bin makes all 64 features one function of
the cosine: the float32 restatement itself is 6e-5 / 5e-6 off in rstd2 there).  On every other distribution, on those small
shapes, and for every output not bounded before (stat1, stat2, the evaluation-mode z; dbeta and dgamma take it too, beside their
inherited bound), the SAME restatement is evaluated in float32 on the identical operands and the kernel may be 4x as far from
float64 as that, plus a floor (tests/gate_parity.Report.close) - the slack between two equally legitimate float32 summation
orders, as in tests/test_gpu_norm.py.  The floors of the newly bounded outputs sit about a decade above the worst error measured
on ``normal`` data (from 31 rows, 16 bins) on the MI355X (profiles/angle_float64_parity.txt: mean / rstd / scale 3.3e-7 ->
B_STAT 3e-6; dbeta / dgamma 1.3e-6 -> B_RED 1e-5; evaluation-mode z 3.7e-7 -> B_INFER 4e-6).  Errors are max |a - b| / max |b| over
the tensor.  Where a result is zero in exact arithmetic - one or two rows, ``constant``, parts of ``w_tiny`` and ``beta_heavy``
(angle_ref.TERM_SCALED says which and why) - it is measured against the magnitudes of its terms.

One or two rows.  xhat2 is (x2 - mean2) gamma2 rstd2 with x2 - mean2 = 0 (one row) or a spread that can be anything against
|mean2| (two rows), and rstd2 up to eps^-1/2.  stat2's mean is handed over in float32 and x2 is a 22-bit f16x3 product: the
pre-activation of z cannot be resolved below res = max_f gamma2 rstd2 (2^-23 (|mean2| + |b2|) + 2^-22 sum_j |W2[f][j]| max |a1[j]|),
whatever the summation order, while the restatement subtracts a mean it has itself just rounded (its error is 0 on one row).
z is allowed 1.1 res (|silu'| <= 1.1) and dbeta2 0.5 res max_f sum_rows |g_z| (|silu''| <= 0.5) on top; with one row mean2 = x2 of
the row likewise inherits layer 1's resolution through sum_j |W2[f][j]|.  These terms exist for rows <= 2 only.

``gz_columns`` (column scales 1 .. 2^-12): column j of red2 and row j of gW2 are held in ABSOLUTE terms, per column, to
max(4 x float32 restatement of that column, amax(g_z) 2^-38 rows) plus the output's floor (B_RED, 2e-5) times the column's own
scale.  The second term: g_z is sliced into two fp16 numbers at a power-of-two scale that puts amax(g_z) below 2^15; the low
slice's smallest step is the fp16 subnormal 2^-24, i.e. 2^-39 amax(g_z) at the tensor's scale, and a sum over the rows holds up
to rows / 2 of them; the factor 2 left is for the operand the slice is multiplied with (|xhat|, |gamma rstd a1| of order 1).
The floor: the float32 restatement of ONE column is off by 2e-9 .. 2e-7 of the column's scale - below the 6e-8 to which a float32
output can be rounded at all -, so without it the allowance is not one a float32 kernel can meet (measured without it: up to 38x
the allowance at column errors of 8e-8 .. 4e-6 of the column's own scale, which is float32 rounding; a kernel that sliced the
columns at the tensor's scale would be 2^-22 2^12 = 1e-3 off in the small ones).  Printed per case.

The statistics of both layers are sums about a pivot where plain sums would cancel: layer 1 about x1 of h[0], or of the MEDIAN of
the first 64 cosines when h[0] lies more than four of their interquartile ranges from it; layer 2 and a1's moments, per
feature, about a1 of that cosine where it exceeds 16 std(z1), else about 0 - so well-conditioned data keeps the plain sums bit
for bit.  This test found both: with x1 of row 0 always the shift ``row0_outlier`` lost rstd1 by 1.2e-5 (2049 rows) and 4.8e-5
(65569) against 1.4e-7 of the float32 restatement, and with layer 2's variance from unshifted sums ``beta_heavy`` lost rstd2 by
7e-2 (33 rows), 1e-2 (257), 9e-3 (2049) - z by as much -, ``constant`` by 1e-3 and one row by 4e-5; now 5e-7, 1.9e-5 .. 4e-6
(the float32 restatement: 1.7e-5 .. 3e-6) and 5e-8.  What is left: on ``row0_outlier`` at 65569 rows rstd2 is 2.10e-5 off against
6.0e-6 of the float32 restatement (allowed 2.7e-5: asserted) and scale2 = gamma2 rstd2 2.10e-5 against 4.4e-6 (allowed 2.06e-5:
4.8x where 4x + floor is the rule) - the cluster's activations hold the rounding of x1 and of the rcp / exp2 SiLU times
rstd1 = 290 against their own spread.  scale2 of that one case is printed as an ``angle-shift`` line and not asserted; every
other output of the case is.

``gz_zero``: every gradient output is exactly 0 (f16_scale(0) = 1: nothing divides by the maximum).

Output buffers are NaN-filled inside sentinel-padded allocations; the sentinel must survive.  z_amax, zeroed before the call,
must EQUAL max |z| written.

Shapes - the smallest at which each branch is live (one wave = a block of 32 rows):
* rows 1: training-mode forward z = silu(beta2), the biased running variance; its backward under the one-row rule; inference.
  (The pivot cosine is the only one; median and quartiles are those of 2 .. 63 cosines at rows 2 .. 33, of the first 64 beyond.)
* rows 2: the smallest batch with statistics (two-row rule for the gradients); 31 / 32 / 33: a ragged block, one full block
  (the uniform ``full`` branch of angle_rb_kernel), a full one and one row.
* rows 255 / 256 / 257: a ragged tile, the ``full`` branch of angle_sums_dw2_kernel (tile of 256 rows), a full tile and one row.
* rows 2048 / 2049: 64 / 68 layer-1 slabs (4 waves x ceil(rows / 128) workgroups): alignn_slab_sum alone / alignn_slab_fold
  first, on either side of alignn_slab_fold_slabs() = 64, for dW1.
* rows 16384 / 16385: 64 / 65 dW2 slabs, the same boundary.
* rows 65536 + 33: the first grid-stride iteration of the 64-feature kernels (kGrid 512 x 4 waves x 32 rows = 65536), on
  ``normal`` and ``row0_outlier`` only.
* bins 1, 16, 17, 32, 33, 40, 47 at rows 257: one k-step live and two padded .. three live; 33 = one bin in the third step.
* ALIGNN_AMD_ANGLE_GRID=8 in one fresh child process (the cap is read once per process), rows 2049, 4096, 6145: every
  512-thread pass walks 2-3 tiles per workgroup and prefetches h past the end.  The full-size cases stay those of
  tests/test_gpu_angle.py (200 003 and 676 200 rows).
Every distribution but ``normal`` runs at (33, 17), (257, 40) and (2049, 33).  Left out: nothing named in the list above;
training mode with one row has no autograd reference (the restatement's closed forms stand alone there)."""

import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

from alignn_amd import _lib  # noqa: E402
from alignn_amd.alignn import MLPLayer  # noqa: E402
from alignn_amd.angle import AngleEmbedding  # noqa: E402
from tests import angle_ref as ref  # noqa: E402
from tests.gate_parity import Report  # noqa: E402

DEV = "cuda"
TAG = "angle-parity"
INVALID = 1  # hipErrorInvalidValue
NAN, SENTINEL, PAD = float("nan"), 7.0, 64
B_Z, B_RUN, B_GRAD, B_GB = 2e-6, 1e-5, 2e-5, 1e-4  # inherited (module docstring)
B_STAT, B_RED, B_INFER = 3e-6, 1e-5, 4e-6  # floors of outputs not bounded before (profiles/angle_float64_parity.txt)
D = torch.float64
# (distribution, rows): outputs printed as ``angle-shift`` lines and not asserted (module docstring)
SHIFT_ONLY = {("row0_outlier", 65536 + 33): ("scale2",)}


def _out(*shape):
    """(buffer, view): a NaN-filled contiguous output of ``shape`` between PAD sentinel floats on either side"""
    n = 1
    for s in shape:
        n *= s
    buf = torch.full((n + 2 * PAD,), SENTINEL, device=DEV)
    buf[PAD:PAD + n] = NAN
    return buf, buf[PAD:PAD + n].view(*shape)


def _kept(rep, ent, bufs):
    for name, (buf, view) in bufs.items():
        if not (bool((buf[:PAD] == SENTINEL).all()) and bool((buf[PAD + view.numel():] == SENTINEL).all())):
            rep.failed.append((ent, name, "wrote outside its buffer"))


class Case:
    """the operands on the device, the modules that hold them, the embedding, and both restatements"""

    def __init__(self, rows, bins, data, reference=True):
        self.rows, self.bins, self.data = rows, bins, data
        self.o = {k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in ref.operands(rows, bins, data).items()}
        o = self.o
        self.layers = []
        for k, (fin, fout) in (("1", (bins, ref.E1)), ("2", (ref.E1, ref.E2))):
            m = MLPLayer(fin, fout).to(DEV).train()
            with torch.no_grad():
                for dst, src in ((m.layer[0].weight, "W"), (m.layer[0].bias, "b"), (m.layer[1].weight, "g"), (m.layer[1].bias, "be"),
                                 (m.layer[1].running_mean, "rm"), (m.layer[1].running_var, "rv")):
                    dst.copy_(o[src + k])
            self.layers.append(m)
        self.emb = AngleEmbedding(o["centers"], o["gamma"], self.layers, eps=ref.EPS, momentum=ref.MOMENTUM)
        # an inherited bound stands alone on ``normal`` data at the conditioning it was set on: from 31 rows and 16 bins on
        self.own = (lambda t: t) if data != "normal" or rows <= 2 or bins < 16 else (lambda t: None)
        if reference:
            self.f64, self.f32 = ref.forward(o), ref.forward(o, torch.float32)
        # one or two rows (module docstring): what float32 can resolve of layer 2's pre-activation, and of mean2 with one row
        self.res_pre2 = self.res_mean2 = 0.0
        if reference and rows <= 2:
            f, W2 = self.f64, o["W2"].double().abs()
            mean2, sc2 = f["stat2"][0].abs(), f["stat2"][2].abs()
            terms = W2 @ f["a1"].abs().max(0).values
            self.res_pre2 = float((sc2 * (2.0 ** -23 * (mean2 + o["b2"].double().abs()) + 2.0 ** -22 * terms)).max())
            if rows == 1:
                res_a1 = 1.1 * (f["stat1"][2].abs() * (2.0 ** -23 * (f["stat1"][0].abs() + o["b1"].double().abs())
                                                      + 2.0 ** -22 * (o["W1"].double().abs() @ f["rbf"][0]))).max()
                self.res_mean2 = float(res_a1 * W2.sum(1).max())

    def params(self):
        return [t for m in self.layers for t in (m.layer[0].weight, m.layer[0].bias, m.layer[1].weight, m.layer[1].bias)]

    def running(self):
        return [t for m in self.layers for t in (m.layer[1].running_mean, m.layer[1].running_var)]

    def set_running(self, values):
        with torch.no_grad():
            for dst, src in zip(self.running(), values):
                dst.copy_(src)

    # ---- alignn_angle_embed_fwd
    def forward(self, rep):
        emb, f64, f32, own = self.emb, self.f64, self.f32, self.own
        bufs = dict(z=_out(self.rows, ref.E2), stat1=_out(4 * ref.E1), stat2=_out(4 * ref.E2))
        emb.stat1, emb.stat2 = bufs["stat1"][1], bufs["stat2"][1]
        am = torch.zeros(1, device=DEV)
        z, _ = emb.forward(self.o["h"], z=bufs["z"][1], amax=am)
        torch.cuda.synchronize()
        ent = "angle_embed_fwd"
        res_z = 1.1 * self.res_pre2 / float(f64["z"].abs().max())  # (|silu'| <= 1.1)
        res_mean2 = self.res_mean2 / float(f64["stat2"][0].abs().max())
        shift_only = SHIFT_ONLY.get((self.data, self.rows), ())
        rep.close(ent, "z", z, f64["z"], own(f32["z"]), B_Z + res_z)
        rep.amax(ent, "amax", am[0], z)
        for k, F in (("1", ref.E1), ("2", ref.E2)):
            stat = bufs["stat" + k][1].view(4, F)
            for i, name in enumerate(("mean", "rstd", "scale")):
                if name + k in shift_only:
                    e, e32 = (float((t[i].double() - f64["stat" + k][i]).abs().max() / f64["stat" + k][i].abs().max()) for t in (stat, f32["stat" + k]))
                    print(f"angle-shift {rep.case:<38s} {name + k:<8s} err {e:8.2e}  float32 {e32:8.2e}  (not asserted)")
                    continue
                rep.close(ent, f"{name}{k}", stat[i], f64["stat" + k][i], f32["stat" + k][i], B_STAT + (res_mean2 if name + k == "mean2" else 0.0))
            if not torch.equal(stat[3], self.o["be" + k]):
                rep.failed.append((ent, "stat" + k, "shift is not beta"))
            bn = self.layers[int(k) - 1].layer[1]
            rep.close(ent, "rmean" + k, bn.running_mean, f64["rm" + k], own(f32["rm" + k]), B_RUN)
            rep.close(ent, "rvar" + k, bn.running_var, f64["rv" + k], own(f32["rv" + k]), B_RUN)
        _kept(rep, ent, bufs)
        return z

    # ---- alignn_angle_embed_bwd
    def grad_buffers(self):
        bufs = dict(gW1=_out(ref.E1, self.bins), gb1=_out(ref.E1), red1=_out(2 * ref.E1), gW2=_out(ref.E2, ref.E1), gb2=_out(ref.E2),
                    red2=_out(2 * ref.E2))
        return bufs, tuple(tuple(bufs[n + k][1] for n in ("gW", "gb", "red")) for k in ("1", "2"))

    def backward(self, rep):
        o, own = self.o, self.own
        b64, b32 = ref.backward(o, self.f64), ref.backward(o, self.f32)
        fl = ref.floors(b64, self.rows, self.data)
        bufs, out = self.grad_buffers()
        self.emb.backward(o["gz"], out=out)
        torch.cuda.synchronize()
        ent = "angle_embed_bwd"
        _kept(rep, ent, bufs)
        got = {k: v[1] for k, v in bufs.items()}
        if self.data == "gz_zero":
            for k, t in got.items():
                if bool(t.any()) or not bool(torch.isfinite(t).all()):
                    rep.failed.append((ent, k, "not exactly zero for g_z = 0"))
            return
        for k, F in (("1", ref.E1), ("2", ref.E2)):
            rep.close(ent, "gW" + k, got["gW" + k], b64["gW" + k], own(b32["gW" + k]), B_GRAD, fl.get("gW" + k, 1e-30))
            red = got["red" + k].view(2, F)
            for i, name in enumerate(("dbeta", "dgamma")):
                floor = fl.get(f"red{k}/{name}", 1e-30)
                res = 0.0
                if name + k == "dbeta2" and self.res_pre2:  # (|silu''| <= 0.5)
                    res = 0.5 * self.res_pre2 * float(o["gz"].double().abs().sum(0).max()) / float(b64["red2"][0].abs().max())
                rep.close(ent, name + k, red[i], b64["red" + k][i], b32["red" + k][i], B_RED + res, floor)
                if own(1) is None:
                    rep.close(ent + " inherited", name + k, red[i], b64["red" + k][i], None, B_GRAD, floor)
            # Linear bias in front of BatchNorm: exact gradient 0, every side holds rounding noise
            scale = float(b64["gW" + k].abs().max())
            gb, gb32 = float(got["gb" + k].abs().max()), float(b32["gb" + k].abs().max())
            if own(1) is None:
                rep.record(ent, "gb" + k, gb, None, B_GB * max(scale, 1.0))
            else:
                rep.record(ent, "gb" + k, gb, gb32, 4 * gb32 + B_GB * max(scale, fl.get("gW" + k, 0.0)))
        if self.data == "gz_columns":  # per column, absolute (module docstring)
            step = float(o["gz"].abs().max()) * 2.0 ** -38 * self.rows
            # (a column's own scale: of a sum, the sum of its summands' magnitudes - the sum itself can cancel to anything)
            for name, a, b, c, floor, scales in (("dbeta2", got["red2"][:ref.E2], b64["red2"][0], b32["red2"][0], B_RED, b64["m_red2"][0]),
                                                 ("dgamma2", got["red2"][ref.E2:], b64["red2"][1], b32["red2"][1], B_RED, b64["m_red2"][1]),
                                                 ("gW2", got["gW2"], b64["gW2"], b32["gW2"], B_GRAD, b64["gW2"].abs().max(1).values)):
                e = (a.double() - b).abs().reshape(ref.E2, -1).max(1).values
                e32 = (c.double() - b).abs().reshape(ref.E2, -1).max(1).values
                bare = e / torch.maximum(4 * e32, torch.full_like(e, step))
                worst = e / (torch.maximum(4 * e32, torch.full_like(e, step)) + floor * scales)
                j = int(worst.argmax())
                scale = float(scales[j])
                print(f"{TAG} {rep.case:<38s} per column {name:<8s} worst column {j}: err {float(e[j]) / scale:8.2e}  float32 "
                      f"{float(e32[j]) / scale:8.2e} of the column's scale; without the floor {float(bare.max()):8.2e} of the allowance")
                rep.record(ent + " per column", "c." + name, float(worst.max()), None, 1.0)

    # ---- alignn_angle_embed_infer
    def infer(self, rep, running, what):
        before = [t.clone() for t in self.params() + self.running()]
        bufs = dict(z=_out(self.rows, ref.E2))
        am = torch.zeros(1, device=DEV)
        z, _ = self.emb.infer(self.o["h"], z=bufs["z"][1], amax=am)
        torch.cuda.synchronize()
        ent = "angle_embed_infer " + what
        rep.close(ent, "z", z, ref.infer(self.o, D, running), ref.infer(self.o, torch.float32, running), B_INFER)
        rep.amax(ent, "amax", am[0], z)
        _kept(rep, ent, bufs)
        if not all(torch.equal(a, b) for a, b in zip(before, self.params() + self.running())):
            rep.failed.append((ent, "parameters or running statistics changed"))


def _train_case(rows, bins, data):
    rep = Report(f"rows={rows} bins={bins} {data}", TAG)
    c = Case(rows, bins, data)
    c.forward(rep)
    c.backward(rep)
    rep.finish()


ROWS = (1, 2, 31, 32, 33, 255, 256, 257, 2048, 2049, 16384, 16385)
BINS = (1, 16, 17, 32, 33, 47)
HARD_SHAPES = ((33, 17), (257, 40), (2049, 33))
TRAIN_CASES = ([(rows, 40, "normal") for rows in ROWS] + [(257, bins, "normal") for bins in BINS]
               + [(rows, bins, data) for data in ref.DATA[1:] for rows, bins in HARD_SHAPES]
               + [(65536 + 33, 40, data) for data in ("normal", "row0_outlier")])


@pytest.mark.parametrize("rows,bins,data", TRAIN_CASES)
def test_forward_and_backward_against_float64(rows, bins, data):
    """alignn_angle_embed_fwd, then alignn_angle_embed_bwd on its state: every output against the float64 restatement.  See
    the module docstring for shapes, distributions and bounds; the worst error per output is printed."""
    _train_case(rows, bins, data)


def _eval_case(rows, bins, data):
    rep = Report(f"eval rows={rows} bins={bins} {data}", TAG)
    c = Case(rows, bins, data, reference=rows > 1)
    o = c.o
    c.infer(rep, [o[k] for k in ("rm1", "rv1", "rm2", "rv2")], "own")  # running statistics that are not the batch's
    if rows > 1:
        f = c.f64
        for _ in range(2):  # two training steps
            c.emb.forward(o["h"])
        torch.cuda.synchronize()
        c.infer(rep, [t.clone() for t in c.running()], "trained")
        # the mean off by 3 sigma, the variance x 100 (even features) and x 0.01 (odd ones)
        far = []
        for k, F in (("1", ref.E1), ("2", ref.E2)):
            s = torch.where(torch.arange(F, device=DEV) % 2 == 0, 100.0, 0.01)
            far += [(f["stat" + k][0] + 3 * f["var" + k].sqrt()).float(), (f["var" + k] * s).float()]
        c.set_running(far)
        c.infer(rep, far, "far")
    tiny = [o["rm1"], o["rv1"].clone(), o["rm2"], o["rv2"].clone()]
    tiny[1][::3] = 1e-12
    tiny[3][::5] = 1e-12
    c.set_running(tiny)
    c.infer(rep, tiny, "var=1e-12")
    rep.finish()


@pytest.mark.parametrize("rows,bins,data", [(1, 40, "normal"), (33, 17, "normal"), (257, 40, "lattice"), (2049, 33, "normal"),
                                            (2049, 40, "w_huge"), (257, 47, "beta_heavy")])
def test_evaluation_mode_against_float64(rows, bins, data):
    """alignn_angle_embed_infer (AngleEmbedding.infer) from running statistics that are not the batch's, from those two training
    steps leave, from ones set far from the batch's (mean off by 3 sigma, variance x 100 / x 0.01), with a running variance of
    1e-12 in some features, and on ONE row; parameters and running statistics stay bit-unchanged."""
    _eval_case(rows, bins, data)


def test_a_second_backward_on_one_forward_scales_bit_for_bit():
    """forward once; backward with g, with g 2^-30, with g again.  Every operand scale is a power of two and nothing else depends
    on the magnitude of g_z: the second result is 2^-30 of the first and the third IS the first, bit for bit.  (The backward only
    ever RAISED its maxima and bounds in scal[], so the second call sliced its operands at the first one's scales - into fp16
    subnormals; alignn_angle_embed_bwd now resets its own six scalars.)"""
    c = Case(2049, 40, "normal", reference=False)
    c.emb.forward(c.o["h"])
    s = 2.0 ** -30
    runs = []
    for g in (c.o["gz"], c.o["gz"] * s, c.o["gz"]):
        _, out = c.grad_buffers()
        c.emb.backward(g, out=out)
        torch.cuda.synchronize()
        runs.append([t for grp in out for t in grp])
    names = ("gW1", "gb1", "red1", "gW2", "gb2", "red2")
    assert all(bool(torch.isfinite(t).all()) for r in runs for t in r)
    assert float(runs[0][0].abs().max()) > 0 and float(runs[0][3].abs().max()) > 0
    bad = [n for n, a, b in zip(names, runs[0], runs[1]) if not torch.equal(a * s, b)]
    bad += [n + " (third)" for n, a, b in zip(names, runs[0], runs[2]) if not torch.equal(a, b)]
    assert not bad, bad


def test_unsupported_calls_are_refused():
    """hipErrorInvalidValue and nothing written: bins 0 and 48, a workspace one byte short, a null h or z."""
    import ctypes as C

    lib = _lib.load()
    c = Case(257, 40, "normal", reference=False)
    emb, h = c.emb, c.o["h"]
    bufs, out = c.grad_buffers()
    emb.grads = out
    bufs.update(z=_out(257, ref.E2), stat1=_out(4 * ref.E1), stat2=_out(4 * ref.E2))
    emb.stat1, emb.stat2 = bufs["stat1"][1], bufs["stat2"][1]
    ws = torch.empty(max(lib.alignn_angle_embed_workspace(257, 47, k) for k in (0, 1)), dtype=torch.uint8, device=DEV)
    am = torch.zeros(1, device=DEV)
    before = [t.clone() for t in c.params() + c.running()]

    def call(fn, backward, **change):
        a = emb._args(h)
        a.z, a.z_amax, a.gz, a.workspace = bufs["z"][1].data_ptr(), am.data_ptr(), c.o["gz"].data_ptr(), ws.data_ptr()
        a.workspace_bytes = lib.alignn_angle_embed_workspace(257, 40, backward)
        for k, v in change.items():
            if k == "bins":
                a.bins = a.l1.in_ = v
            elif k == "short":
                a.workspace_bytes -= 1
            else:
                setattr(a, k, v)
        return fn(C.byref(a), _lib.stream())

    fwd, bwd, inf = lib.alignn_angle_embed_fwd, lib.alignn_angle_embed_bwd, lib.alignn_angle_embed_infer
    rc = {}
    for name, fn, backward in (("fwd", fwd, 0), ("bwd", bwd, 1), ("infer", inf, 0)):
        rc[name + " bins=48"] = call(fn, backward, bins=48)
        rc[name + " bins=0"] = call(fn, backward, bins=0)
        rc[name + " h=NULL"] = call(fn, backward, h=None)
        rc[name + " rows=0"] = call(fn, backward, rows=0)
        if name != "bwd":
            rc[name + " z=NULL"] = call(fn, backward, z=None)
        if name != "infer":
            rc[name + " workspace one byte short"] = call(fn, backward, short=True)
    rc["bwd gz=NULL"] = call(bwd, 1, gz=None)
    torch.cuda.synchronize()
    assert all(v == INVALID for v in rc.values()), rc
    for name, (buf, view) in bufs.items():
        assert bool(torch.isnan(view).all()) and bool((buf[:PAD] == SENTINEL).all()) and bool((buf[-PAD:] == SENTINEL).all()), name
    assert float(am) == 0.0 and all(torch.equal(a, b) for a, b in zip(before, c.params() + c.running()))


GRID_ROWS = (2049, 4096, 6145)


def _grid_child():
    """(runs in the child process of the test below: this file as a script)"""
    assert os.environ.get("ALIGNN_AMD_ANGLE_GRID") == "8"
    for rows in GRID_ROWS:
        _train_case(rows, 40, "normal")
        _eval_case(rows, 40, "normal")


def test_grid_stride_of_the_512_thread_passes_in_a_child_process():
    """ALIGNN_AMD_ANGLE_GRID=8 (read once per process, hence the child): 8 workgroups of 8 waves - 2048 rows per sweep of the
    one-wave-per-block passes and of angle_sums_dw2_kernel's tiles of 256 - on 2049, 4096 and 6145 rows: two to three tiles per
    workgroup, the last sweep ragged or missing, h prefetched past the end.  Forward, backward and inference against float64 as
    above; the child prints its angle-parity lines and fails on the first case out of bounds."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, ALIGNN_AMD_ANGLE_GRID="8", PYTHONPATH=os.pathsep.join([root] + os.environ.get("PYTHONPATH", "").split(os.pathsep)))
    r = subprocess.run([sys.executable, os.path.abspath(__file__)], cwd=root, env=env, capture_output=True, text=True, timeout=240)
    print(r.stdout)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    assert r.stdout.count(TAG) > 10 * len(GRID_ROWS)


if __name__ == "__main__":
    _grid_child()
