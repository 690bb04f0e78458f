"""csrc/gemm_dw.hip - the input gradient C = G W (+ addend), the weight gradient dW = G^T Y and the BatchNorm-backward column
sums of a 256 x 256 projection in one pass - against the float64 restatements of tests/gemm_ref.py (``dw_operands`` and the
bounds, checked on their own on the CPU by tests/test_gemm_ref.py), through the raw C ABI, element by element.  The other tests
of this kernel (tests/test_gpu_gemm_dw.py, tests/test_gpu_kernels.py) go through the ``ops`` wrapper on N(0, 1) or row-block
data, with one leading dimension, and measure a max-norm over the whole tensor.

Buffers.  Every operand is a view with a leading dimension of its own (264, 268, 272, 276, 284, 260 for G, Y, addend, Xn, C, dW;
all 256 at the even row counts) in a buffer with four NaN rows behind its M rows: an over-read shows as a NaN in an output,
nothing faults.  C and dW are NaN-filled inside sentinel-filled wider buffers with two more rows, ``workspace`` and
``red_partial`` NaN-filled with three slabs more than the call may touch.  No element, row or case is left out.

Bounds (tests/gemm_ref.py; nothing is taken from what the kernel returns except where said):
* C: every element within f16x3_scheme_bound_at(G, W^T, handed max|G|, max|W|) + accumulation_bound - what the NT family is held
  to - and the bits of alignn_gemm_nt_f16x3 / _bnred on the same operands;
* dW: every element within f16x3_scheme_bound_at(G^T, Y^T, handed maxima) + (M + 3) 2^-24 |G|^T |Y| (as test_x6_tn); on
  ``normal`` also the inherited 3e-6 max-norm;
* workspace slab b: against the float64 product of the rows of tiles b, b + grid, ...: scheme + (64 J_b + 3) 2^-24 |.|, J_b that
  workgroup's tile count - the tile walk per workgroup;
* BatchNorm sums (the float64 sum of the written slabs, and alignn_bn_bwd_finalize's result): against gemm_ref.bnred_slabs of
  the kernel's OWN C, Xn, nstat as one slab, within 4 x the float32 restatement's error + the floor B_BNRED = 2e-6 of
  tests/test_gpu_gemm.py;
* ``integers``: C and dW equal float64 exactly, with the true maxima and with maxima 16 x too large.

Shapes (cap = alignn_gemm_dgrad_wgrad_slabs(10^6), read from the library): 4096 + r, r in (0, 1, 2, 15, 16, 17, 31, 32, 33, 47,
49, 63) - one tile per workgroup, the last tile ragged at the Y stages of 16 rows, the 32-row halves and the epilogue's 8- and
4-row steps; 64 cap (tiles = workgroups); 64 cap + 1 (one workgroup walks a second, one-row tile, the others request phantom
tiles); 128 cap + 33 and 64 (3 cap - 1) - 7 (three tiles: the steady-state waits twice).  ``integers`` and ``normal`` run at all
of them, the other distributions at 4096 + 33, 64 cap + 1 and 128 cap + 33, all four instantiations (addend x sums) everywhere.
ALIGNN_AMD_DW_GRID=8 (read once per process: a child process) walks eight and nine tiles per workgroup.

The six hypotheses, and what the device showed (MI355X):
1. The product of the two inverse scales underflows for max|G| max|Y| below about 2^-121 (sg sy >= 2^150).  CONFIRMED: before
   the fix ``small_maxima`` returned dW = 0 everywhere - largest error / bound 4.5e+02 at 4129 rows (61 at 14337, 23 at 28705;
   slab by slab 1.3e+05), and alignn_gemm_tn 4.3e+02, alignn_gemm_tn_x6_partials 6.3e+04 in
   tests/test_gpu_gemm.py::test_x6_tn - while C was inside its bound (1.6e-02).  After: dW 5.3e-05 / 9.5e-06 / 3.9e-06 of its bound, slabs 3.1e-02.
   Both kernels now apply the two inverse scales one after the other where their product is 0 and the product otherwise, so
   no other input changes a bit: asserted against outputs of the unfixed build on every other distribution
   (profiles/gemm_dw_float64_parity.txt).
2. Leading dimensions were checked modulo 4 only.  CONFIRMED by reading (not run: such a launch writes overlapping or wrapped
   rows); alignn_gemm_dgrad_wgrad_f16x3 now refuses ld < 256 and ld >= 2^20 (test_refusals).
3. Maxima above the true ones: REFUTED as a defect - 4 x and (``integers``) 16 x the true maxima stay inside the bounds
   evaluated at the handed maxima, ``integers`` exactly.
4. Rows past M: REFUTED - no NaN of the four rows behind any operand reaches an output at any ragged end, and a NaN in row
   M - 1 of G, Y or Xn stays in its row or column (test_row_isolation).
5. The steady-state waits: REFUTED - the three-tile shapes and the eight / nine-tile walks of the grid override meet the
   elementwise and the slab-by-slab bounds on every distribution, ``integers`` exactly.
6. Extents: REFUTED - exactly slabs(M) workspace slabs and 2 slabs(M) slabs of red_partial are written, the three behind
   each stay NaN, the paddings of C and dW keep the sentinel.

Not tested: infinities in the operands.  A phantom row of Y is the last row times 0, so an Inf there is a NaN by
construction."""

import hashlib
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

from alignn_amd import _lib  # noqa: E402
from alignn_amd._lib import ptr, stream  # noqa: E402
from tests import gemm_ref as ref  # noqa: E402
from tests.gate_parity import Report, err  # noqa: E402

DEV = "cuda"
TAG = "gemm-dw-parity"
H, R = 256, 64
INVALID = 1  # hipErrorInvalidValue
NAN, SENTINEL, U = float("nan"), 7.0, ref.U
B_DW = 3e-6  # inherited (tests/test_gpu_gemm_dw.py)
B_BNRED = 2e-6  # floor of the BatchNorm sums, inherited (tests/test_gpu_gemm.py)

d = lambda t: t.double()  # noqa: E731
cdiv = lambda a, b: (a + b - 1) // b  # noqa: E731


# (the helpers of tests/test_gpu_gemm.py, restated: no module imports from a test module)
def _out(rows, cols, before, after):
    """(buffer, view) of a NaN-filled [rows, cols] output inside a sentinel-filled wider buffer with two more rows"""
    buf = torch.full((rows + 2, before + cols + after), SENTINEL, device=DEV)
    buf[:rows, before:before + cols] = NAN
    return buf, buf[:rows, before:before + cols]


def _kept(rep, ent, buf, rows, cols, before):
    mask = torch.ones_like(buf, dtype=torch.bool)
    mask[:rows, before:before + cols] = False
    if not bool((buf[mask] == SENTINEL).all()):
        rep.failed.append((ent, "wrote outside its output"))


def _bits(t):
    return t.contiguous().view(torch.int32)


def _within(rep, ent, name, got, want64, bound):
    """every element: |got - want64| <= bound (recorded as the largest error / bound; an element off a zero bound, or a NaN,
    fails)"""
    e = (d(got) - want64).abs()
    ratio = torch.where(bound > 0, e / bound, torch.where(e == 0, torch.zeros_like(e), torch.full_like(e, float("inf"))))
    rep.record(ent, name + "/bnd", float(ratio.max()), None, 1.0 + 1e-12)
    return ratio


def _scalar(x):
    return x.abs().max().reshape(1).clone()
INSTANCES = ((False, False), (True, False), (False, True), (True, True))  # (addend, BatchNorm sums)
RAGGED = (0, 1, 2, 15, 16, 17, 31, 32, 33, 47, 49, 63)
# row counts as functions of cap = the largest grid (resolved in the test: collecting this module loads no library)
SHAPES = {f"4096+{r}": (lambda cap, r=r: 4096 + r) for r in RAGGED}
SHAPES.update({"64cap": lambda cap: 64 * cap, "64cap+1": lambda cap: 64 * cap + 1, "128cap+33": lambda cap: 128 * cap + 33,
               "64(3cap-1)-7": lambda cap: 64 * (3 * cap - 1) - 7})
SOME_SHAPES = ("4096+33", "64cap+1", "128cap+33")
OTHER_DATA = tuple(k for k in ref.DW_DATA if k not in ("integers", "normal"))


def _rows(name):
    lib = _lib.load()
    M = SHAPES[name](lib.alignn_gemm_dgrad_wgrad_slabs(10 ** 6))
    assert lib.alignn_gemm_dgrad_wgrad_supported(M, H, H) == 1
    return M


def _operand(t, ld):
    """t on the device as a view with leading dimension ld: the sentinel in the padding, four NaN rows behind the last one"""
    rows, cols = t.shape
    buf = torch.full((rows + 4, ld), SENTINEL, device=DEV)
    buf[rows:] = NAN
    buf[:rows, :cols] = t.to(DEV)
    return buf[:rows, :cols]


class Problem:
    """one (M, distribution): the operands as views, the weight image, the float64 products and magnitudes - computed once and
    shared by the four instantiations and every variant of the maxima"""

    def __init__(self, M, data, equal_ld=None):
        self.lib, self.M, self.data = _lib.load(), M, data
        lib, st = self.lib, stream()
        equal_ld = M % 2 == 0 if equal_ld is None else equal_ld
        ld = dict(G=H, Y=H, add=H, xn=H, W=H, C=(0, 0), dW=(0, 0)) if equal_ld else dict(G=264, Y=268, add=272, xn=276, W=280, C=(8, 20), dW=(4, 0))
        G, Y, W, addend, xn, nstat = ref.dw_operands(M, data)
        self.G, self.Y, self.addend, self.xn = _operand(G, ld["G"]), _operand(Y, ld["Y"]), _operand(addend, ld["add"]), _operand(xn, ld["xn"])
        self.W, self.nstat, self.cpad, self.dwpad = _operand(W, ld["W"]), nstat.to(DEV), ld["C"], ld["dW"]
        self.g_amax, self.y_amax, self.w_amax = _scalar(self.G), _scalar(self.Y), _scalar(self.W)
        self.img = torch.empty(lib.alignn_split_f16x2_bytes(H, H), dtype=torch.uint8, device=DEV)
        assert lib.alignn_split_f16x2(ptr(self.W), self.W.stride(0), H, H, 1, ptr(self.w_amax), ptr(self.img), st) == 0
        self.grid, self.tiles = lib.alignn_gemm_dgrad_wgrad_slabs(M), cdiv(M, R)
        assert 1 <= self.grid <= self.tiles and lib.alignn_gemm_dgrad_wgrad_workspace(M) == self.grid * H * H * 4
        self.prod, self.dw = d(self.G) @ d(self.W), d(self.G).t() @ d(self.Y)
        self.dw_mag = d(self.G).abs().t() @ d(self.Y).abs()
        self.acc = {False: ref.accumulation_bound(self.G, self.W.t()), True: ref.accumulation_bound(self.G, self.W.t(), addend=self.addend)}
        self._bounds = {}

    def want_c(self, with_add):
        return self.prod + d(self.addend) if with_add else self.prod

    def bounds(self, ga, ya):
        """(C scheme bound, dW bound, per-slab float64 products, per-slab bounds) with the maxima the kernel is handed"""
        if (ga, ya) not in self._bounds:
            wa = float(self.w_amax)
            Gt, Yt = self.G.t(), self.Y.t()
            c_scheme = ref.f16x3_scheme_bound_at(self.G, self.W.t(), ga, wa)
            dw_bound = ref.f16x3_scheme_bound_at(Gt, Yt, ga, ya) + (self.M + 3) * U * self.dw_mag
            want = torch.empty(self.grid, H, H, dtype=torch.float64, device=DEV)
            bound = torch.empty_like(want)
            for b in range(self.grid):  # the rows of tiles b, b + grid, ...
                mine = range(b, self.tiles, self.grid)
                rows = torch.cat([torch.arange(t * R, min((t + 1) * R, self.M), device=DEV) for t in mine])
                g, y = Gt[:, rows], Yt[:, rows]
                want[b] = d(g) @ d(y).t()
                bound[b] = ref.f16x3_scheme_bound_at(g, y, ga, ya) + (R * len(mine) + 3) * U * (d(g).abs() @ d(y).abs().t())
            self._bounds[(ga, ya)] = (c_scheme, dw_bound, want, bound)
        return self._bounds[(ga, ya)]


class Run:
    """one launch into fresh NaN-filled buffers"""

    def __init__(self, p, with_add, with_bn, ga=None, ya=None):
        lib, M, grid = p.lib, p.M, p.grid
        self.ga = p.g_amax if ga is None else torch.tensor([ga], device=DEV)
        self.ya = p.y_amax if ya is None else torch.tensor([ya], device=DEV)
        self.cbuf, self.C = _out(M, H, *p.cpad)
        self.dwbuf, self.dW = _out(H, H, *p.dwpad)
        self.ws = torch.full((grid + 3, H, H), NAN, device=DEV)
        self.red = torch.full((2 * grid + 3, 2, H), NAN, device=DEV)
        self.rc = lib.alignn_gemm_dgrad_wgrad_f16x3(
            ptr(p.G), p.G.stride(0), ptr(self.ga), ptr(p.Y), p.Y.stride(0), ptr(self.ya), ptr(p.img), ptr(p.w_amax),
            ptr(p.addend) if with_add else None, p.addend.stride(0) if with_add else 0, ptr(self.C), self.C.stride(0),
            ptr(p.xn) if with_bn else None, p.xn.stride(0) if with_bn else 0, ptr(p.nstat) if with_bn else None,
            ptr(self.red) if with_bn else None, ptr(self.dW), self.dW.stride(0), M, ptr(self.ws), grid * H * H * 4, stream())
        self.fin = None
        if with_bn and self.rc == 0:
            self.fin = torch.full((2, H), NAN, device=DEV)
            assert lib.alignn_bn_bwd_finalize(ptr(self.red), 2 * grid, H, ptr(self.fin), stream()) == 0
        torch.cuda.synchronize()
        assert self.rc == 0, (M, with_add, with_bn, self.rc)

    def same_bits(self, other):
        return all(torch.equal(_bits(a), _bits(b)) for a, b in ((self.cbuf, other.cbuf), (self.dwbuf, other.dwbuf), (self.ws, other.ws), (self.red, other.red)))

    def digest(self):
        """sha256 over the bits of C, dW, the written slabs and the finished sums"""
        h = hashlib.sha256()
        for t in (self.C, self.dW, self.ws, self.red) + (() if self.fin is None else (self.fin,)):
            h.update(t.contiguous().cpu().numpy().tobytes())
        return h.hexdigest()


def _name(with_add, with_bn):
    return "gemm_dgrad_wgrad" + (" +addend" if with_add else "") + (" +sums" if with_bn else "")


def _nt_bits(p, run, with_add, with_bn):
    """C of alignn_gemm_nt_f16x3 / _bnred on the same operands and maxima"""
    lib = p.lib
    _, C = _out(p.M, H, *p.cpad)
    head = [ptr(p.G), p.G.stride(0), ptr(run.ga), ptr(p.img), ptr(p.w_amax), None, ptr(p.addend) if with_add else None,
            p.addend.stride(0) if with_add else 0, ptr(C), C.stride(0), p.M, H, H]
    if with_bn:
        part = torch.full((lib.alignn_gemm_nt_x6_row_tiles(p.M, H, H) + 1, 2, H), NAN, device=DEV)
        rc = lib.alignn_gemm_nt_f16x3_bnred(*head, ptr(p.xn), p.xn.stride(0), ptr(p.nstat), ptr(part), stream())
    else:
        rc = lib.alignn_gemm_nt_f16x3(*head, stream())
    torch.cuda.synchronize()
    assert rc == 0
    return torch.equal(_bits(C), _bits(run.C))


def _check(p, rep, run, with_add, with_bn, tag=""):
    """every assertion on one launch, at the maxima it was handed"""
    ent, M, grid = _name(with_add, with_bn) + tag, p.M, p.grid
    c_scheme, dw_bound, slab_want, slab_bound = p.bounds(float(run.ga), float(run.ya))
    # extents
    _kept(rep, ent, run.cbuf, M, H, p.cpad[0])
    _kept(rep, ent, run.dwbuf, H, H, p.dwpad[0])
    if not bool(torch.isfinite(run.ws[:grid]).all()) or not bool(torch.isnan(run.ws[grid:]).all()):
        rep.failed.append((ent, "workspace: slabs(M) slabs finite, nothing behind them touched"))
    written = 2 * grid if with_bn else 0
    if not bool(torch.isfinite(run.red[:written]).all()) or not bool(torch.isnan(run.red[written:]).all()):
        rep.failed.append((ent, "red_partial: 2 slabs(M) slabs finite, nothing behind them touched"))
    # C, dW
    if p.data == "integers":
        if not (torch.equal(d(run.C), p.want_c(with_add)) and torch.equal(d(run.dW), p.dw)):
            rep.failed.append((ent, "integers: C and dW are not float64's"))
    _within(rep, ent, "C", run.C, p.want_c(with_add), c_scheme + p.acc[with_add])
    _within(rep, ent, "dW", run.dW, p.dw, dw_bound)
    if p.data == "normal":
        rep.record(ent, "dW", err(run.dW, p.dw), None, B_DW)
    if not _nt_bits(p, run, with_add, with_bn):
        rep.failed.append((ent, "C: not the bits of alignn_gemm_nt_f16x3" + ("_bnred" if with_bn else "")))
    # the workspace, slab by slab
    per_slab = _within(rep, ent, "slab", run.ws[:grid], slab_want, slab_bound).amax((1, 2))
    worst = int(per_slab.argmax())
    if not float(per_slab[worst]) <= 1.0:  # (which workgroup's walk)
        rep.failed.append((ent, f"slab {worst} (tiles {list(range(worst, p.tiles, grid))})", [int(i) for i in (per_slab > 1).nonzero().flatten()[:16]]))
    # the BatchNorm sums against the restatement on the kernel's own C
    if with_bn:
        Cc, xn = run.C.contiguous(), p.xn.contiguous()
        r64, r32 = ref.bnred_slabs(d(Cc), d(xn), d(p.nstat), M)[0], ref.bnred_slabs(Cc, xn, p.nstat, M)[0]
        got = d(run.red[:2 * grid]).sum(0)
        for k, name in enumerate(("gz", "gzxhat")):
            rep.close(ent, name, got[k], r64[k], r32[k], B_BNRED, floor=1e-60)
            rep.close(ent, name + "/fin", run.fin[k], r64[k], r32[k], B_BNRED, floor=1e-60)


def _case(M, data, rep, maxima=(1.0,), equal_ld=None):
    """the four instantiations, each with the true maxima times every factor of ``maxima``, each launched twice"""
    p = Problem(M, data, equal_ld)
    for with_add, with_bn in INSTANCES:
        for k in maxima:
            ga, ya = (None, None) if k == 1.0 else (float(p.g_amax) * k, float(p.y_amax) * k)
            run = Run(p, with_add, with_bn, ga, ya)
            _check(p, rep, run, with_add, with_bn, "" if k == 1.0 else f" maxima x{k:g}")
            if not run.same_bits(Run(p, with_add, with_bn, ga, ya)):
                rep.failed.append((_name(with_add, with_bn), "a second launch gives other bits"))
    return p


@pytest.mark.parametrize("shape", tuple(SHAPES))
def test_integers_exactly(shape):
    """hypotheses 3, 5: any order of exact sums is float64's result - with the true maxima and with maxima 16 x too large"""
    M = _rows(shape)
    rep = Report(f"dw {shape} = {M} integers", TAG)
    _case(M, "integers", rep, maxima=(1.0, 16.0))
    rep.finish()


@pytest.mark.parametrize("shape", tuple(SHAPES))
def test_normal(shape):
    M = _rows(shape)
    rep = Report(f"dw {shape} = {M} normal", TAG)
    _case(M, "normal", rep)
    rep.finish()


@pytest.mark.parametrize("data", OTHER_DATA)
@pytest.mark.parametrize("shape", SOME_SHAPES)
def test_hard_data(shape, data):
    M = _rows(shape)
    rep = Report(f"dw {shape} = {M} {data}", TAG)
    _case(M, data, rep)
    rep.finish()


@pytest.mark.parametrize("data", ("normal", "row_blocks"))
@pytest.mark.parametrize("shape", SOME_SHAPES)
def test_maxima_above_the_true_ones(shape, data):
    """hypothesis 3: the header allows g_amax >= max|G|, y_amax >= max|Y| - the same bounds, evaluated at the handed maxima"""
    M = _rows(shape)
    rep = Report(f"dw {shape} = {M} {data} maxima x4", TAG)
    _case(M, data, rep, maxima=(4.0,))
    rep.finish()


def test_all_zero_gradient():
    """g_amax = 0 (f16_scale gives 1): C has the addend's bits, dW is exactly 0"""
    p = Problem(4096 + 33, "normal")
    p.G.zero_()
    for with_add, with_bn in INSTANCES:
        run = Run(p, with_add, with_bn, ga=0.0)
        assert torch.equal(_bits(run.C), _bits(p.addend if with_add else torch.zeros_like(run.C))), _name(with_add, with_bn)
        assert torch.equal(_bits(run.dW), _bits(torch.zeros_like(run.dW))) and not bool(run.ws[:p.grid].any()), _name(with_add, with_bn)
    print(f"{TAG} all-zero G, g_amax = 0: C = addend (bits), dW = 0, every written slab 0")


@pytest.mark.parametrize("shape", ("4096+33", "128cap+33"))
def test_row_isolation(shape):
    """hypothesis 4: a NaN in the row the clamped out-of-range rows re-read, or anywhere else, stays in its row / column"""
    M = _rows(shape)
    assert M % R == 33
    p = Problem(M, "normal")
    grid = p.grid
    others = lambda n, i: torch.arange(n, device=DEV) != i  # noqa: E731
    for with_add, with_bn in INSTANCES:
        ent = _name(with_add, with_bn)
        clean = Run(p, with_add, with_bn)

        def poked(t, r, c):
            keep = t[r, c].clone()
            t[r, c] = NAN
            try:
                return Run(p, with_add, with_bn)
            finally:
                t[r, c] = keep

        for r, c in ((M - 1, 0), (100, 7)):
            run = poked(p.G, r, c)
            assert bool(torch.isnan(run.C[r]).all()) and torch.equal(_bits(run.C[others(M, r)]), _bits(clean.C[others(M, r)])), (ent, "G", r, c, "C")
            assert bool(torch.isnan(run.dW[c]).all()) and torch.equal(_bits(run.dW[others(H, c)]), _bits(clean.dW[others(H, c)])), (ent, "G", r, c, "dW")
        run = poked(p.Y, M - 1, 5)
        assert torch.equal(_bits(run.cbuf), _bits(clean.cbuf)), (ent, "Y", "C")
        assert bool(torch.isnan(run.dW[:, 5]).all()) and torch.equal(_bits(run.dW[:, others(H, 5)]), _bits(clean.dW[:, others(H, 5)])), (ent, "Y", "dW")
        if with_bn:
            run = poked(p.xn, M - 1, 9)
            assert torch.equal(_bits(run.cbuf), _bits(clean.cbuf)) and torch.equal(_bits(run.dwbuf), _bits(clean.dwbuf)), (ent, "Xn", "C, dW")
            got, was = d(run.red[:2 * grid]).sum(0), d(clean.red[:2 * grid]).sum(0)
            assert bool(torch.isnan(got[:, 9]).all()) and bool(torch.isnan(run.fin[:, 9]).all()), (ent, "Xn", "column 9 of both sums")
            assert torch.equal(got[:, others(H, 9)], was[:, others(H, 9)]), (ent, "Xn", "the other columns of the slabs")
            assert torch.equal(_bits(run.fin[:, others(H, 9)]), _bits(clean.fin[:, others(H, 9)])), (ent, "Xn", "the other columns, finished")
            assert torch.equal(_bits(run.red[:, :, others(H, 9)]), _bits(clean.red[:, :, others(H, 9)])), (ent, "Xn", "slab by slab")
    print(f"{TAG} row isolation at {M} rows: G[M-1, 0], G[100, 7], Y[M-1, 5], Xn[M-1, 9] - exactly their row / column, four instantiations")


def test_refusals():
    """hypothesis 2 and the pointer checks: hipErrorInvalidValue before any launch - every output still NaN"""
    lib, M = _lib.load(), 4096
    p = Problem(M, "normal", equal_ld=False)
    cbuf, C = _out(M, H, *p.cpad)
    dwbuf, dW = _out(H, H, *p.dwpad)
    cbuf.fill_(NAN), dwbuf.fill_(NAN)
    nbytes = lib.alignn_gemm_dgrad_wgrad_workspace(M)
    ws, red = torch.full((nbytes // 4 + 4,), NAN, device=DEV), torch.full((2 * p.grid + 1, 2, H), NAN, device=DEV)
    good = dict(G=ptr(p.G), ldg=p.G.stride(0), ga=ptr(p.g_amax), Y=ptr(p.Y), ldy=p.Y.stride(0), ya=ptr(p.y_amax), img=ptr(p.img), wa=ptr(p.w_amax),
                addend=ptr(p.addend), ldadd=p.addend.stride(0), C=ptr(C), ldc=C.stride(0), Xn=ptr(p.xn), ldxn=p.xn.stride(0), nstat=ptr(p.nstat),
                part=ptr(red), dW=ptr(dW), lddw=dW.stride(0), M=M, ws=ptr(ws), nbytes=nbytes)
    order = ("G", "ldg", "ga", "Y", "ldy", "ya", "img", "wa", "addend", "ldadd", "C", "ldc", "Xn", "ldxn", "nstat", "part", "dW", "lddw", "M", "ws",
             "nbytes")
    lds = ("ldg", "ldy", "ldadd", "ldxn", "ldc", "lddw")
    # (the first refusals are of leading dimensions that keep every access inside the buffers)
    bad = [(f"{k} = 252: rows overlap", {k: 252}) for k in lds] + [(f"{k} = 0", {k: 0}) for k in lds] + [(f"{k} < 0", {k: -H}) for k in lds]
    bad += [(f"{k} = 2^20: 32-bit offsets inside a tile", {k: 1 << 20}) for k in lds] + [(f"{k} % 4", {k: good[k] + 2}) for k in lds]
    bad += [(f"misaligned {k}", {k: good[k] + 4}) for k in ("G", "Y", "C", "dW", "addend", "Xn", "nstat", "part", "ws", "img")]
    bad += [("no max|G|", dict(ga=None)), ("no max|Y|", dict(ya=None)), ("no max|W|", dict(wa=None)), ("M < 4096", dict(M=4095)),
            ("Xn without nstat", dict(nstat=None)), ("Xn without slabs", dict(part=None)), ("workspace too small", dict(nbytes=nbytes - 4)),
            ("no workspace", dict(ws=None))]
    call = lambda **over: lib.alignn_gemm_dgrad_wgrad_f16x3(*[dict(good, **over)[k] for k in order], stream())  # noqa: E731
    for name, over in bad:
        rc = call(**over)
        torch.cuda.synchronize()
        assert rc == INVALID, (name, rc)
        assert all(bool(torch.isnan(t).all()) for t in (cbuf, dwbuf, ws, red)), (name, "wrote an output")
    # ldadd and ldxn count only where their pointer is given
    assert call(addend=None, ldadd=0, Xn=None, ldxn=0, nstat=None, part=None) == 0
    torch.cuda.synchronize()
    assert bool(torch.isfinite(C).all()) and bool(torch.isfinite(dW).all()) and bool(torch.isnan(red).all())
    print(f"{TAG} refusals: {len(bad)} calls refused with every output still NaN")


# ---- the grid override: read once per process, so a child process each

GRID_ROWS = (4096, 4096 + 64 + 17)  # eight tiles per workgroup; nine for two of them, the last one ragged


def _child(env_value, *args):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, ALIGNN_AMD_DW_GRID=env_value, PYTHONPATH=os.pathsep.join([root] + os.environ.get("PYTHONPATH", "").split(os.pathsep)))
    r = subprocess.run([sys.executable, os.path.abspath(__file__), *args], cwd=root, env=env, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    return r.stdout


def _grid_child():
    """(runs in the child process of the test below: this file as a script)"""
    assert os.environ.get("ALIGNN_AMD_DW_GRID") == "8" and _lib.load().alignn_gemm_dgrad_wgrad_slabs(4096) == 8
    for M in GRID_ROWS:
        for data, maxima in (("integers", (1.0, 16.0)), ("normal", (1.0,)), ("row_blocks", (1.0,))):
            rep = Report(f"dw grid=8 {M} {data}", TAG)
            p = _case(M, data, rep, maxima, equal_ld=False)
            assert p.grid == 8 and p.tiles == cdiv(M, R)
            rep.finish()


def test_grid_override_walks_eight_and_nine_tiles():
    """hypothesis 5: ALIGNN_AMD_DW_GRID=8 - at 4096 rows every workgroup walks eight tiles, at 4177 two of them nine, the last
    one of 17 rows; ``integers`` exactly, ``normal`` and ``row_blocks`` inside every bound, all four instantiations.  The child
    prints its gemm-dw-parity lines and fails at the first case out of bounds."""
    out = _child("8")
    print(out)
    assert out.count(TAG) >= 6 * len(GRID_ROWS)


@pytest.mark.parametrize("value,slabs", (("13", 8), ("1000", 256)))
def test_grid_override_is_clamped_to_multiples_of_eight(value, slabs):
    """host side only: no kernel is launched in the child"""
    assert _child(value, "slabs").split() == [str(slabs)]


if __name__ == "__main__":
    if sys.argv[1:] == ["slabs"]:
        print(_lib.load().alignn_gemm_dgrad_wgrad_slabs(10 ** 6))
    else:
        _grid_child()
