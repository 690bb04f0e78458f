"""The guard bands of tests/gate_parity.py (``guarded``, ``guard_input``, ``gptr``, ``Report.finish``), on the CPU: the detector
the GPU pins of conv.hip, convln.hip and dual.hip rely on must itself report a planted stray access - with the right buffer,
side and offset - and must stay silent otherwise.  Every stray access here is a torch indexing op on the helper's own base
buffer; nothing reads or writes outside an allocation of the test's own."""

import pytest
import torch

from tests import conv_bn_ref as ref
from tests import gate_parity as gp

CPU = "cpu"
I32 = torch.int32


def _base(rep, t):
    return rep.guards.record_of(t)


def test_guard_widths_and_alignment():
    """the larger of 1024 elements and two rows, in whole 512-byte granules; the payload starts a whole number of granules into a
    fresh allocation"""
    assert gp.guard_elements(1) == 1024 and gp.guard_elements(512) == 1024 and gp.guard_elements(513) == 1152
    assert gp.guard_elements(4 * 1024) == 8192 and gp.guard_elements(3 * 260 + 1) == 1664
    assert gp.guard_elements(1, 2) % 256 == 0 and gp.guard_elements(1, 8) == 1024
    rep = gp.Report("widths")
    for shape in ((7, 260), (1,), (0, 64), (5, 2, 36)):
        t = gp.guarded(shape, name="t", device=CPU)
        rec = _base(rep, t)
        assert tuple(t.shape) == shape and t.is_contiguous()
        assert rec.before == rec.base.numel() - rec.before - rec.numel == gp.guard_elements(shape[-1] if len(shape) > 1 else 1)
        assert (t.data_ptr() - rec.base.data_ptr()) % 512 == 0 or t.numel() == 0
    rep.finish()


def test_the_nan_payload_survives_copies_bit_for_bit():
    """clone(), copy_ and a round trip through the int32 view keep the guard pattern's bits; as a float it is a NaN"""
    rep = gp.Report("payload")
    t = gp.guarded((3, 5), name="t", device=CPU)  # (no fill: the payload holds the pattern too)
    want = torch.full((3, 5), gp.NAN_BITS, dtype=I32)
    assert bool(torch.isnan(t).all())
    assert torch.equal(t.view(I32), want)
    assert torch.equal(t.clone().view(I32), want)
    assert torch.equal(torch.empty(3, 5).copy_(t).view(I32), want)
    assert torch.equal(want.view(torch.float32).view(I32), want)
    assert torch.equal(gp.guard_input(t, "copy").view(I32), want)
    for side in _base(rep, t).sides():
        assert bool((side[1] == gp.NAN_BITS).all())
    # torch.full(.., nan) carries no payload, and a float comparison cannot tell: the reason the check is on bits
    assert not torch.equal(torch.full((1,), float("nan")).view(I32), want[:1, 0])
    assert not bool((t == t).any())
    rep.finish()


def test_integer_operands_get_guards_of_zeros():
    rep = gp.Report("indices")
    idx = gp.guard_input(torch.arange(7, dtype=I32), "seg_ptr")
    rec = _base(rep, idx)
    assert torch.equal(idx, torch.arange(7, dtype=I32)) and int(rec.base.abs().sum()) == 21
    rep.finish()
    rec.base[rec.before + 7] = 3
    with pytest.raises(AssertionError, match="seg_ptr: the guard after the payload changed at offset 0 elements"):
        rep.finish()


def test_a_zero_written_into_a_default_integer_guard_is_not_seen():
    """the blind spot ``pattern=`` closes, and the unchanged default: guards of zeros, the payload left as allocated"""
    rep = gp.Report("indices, default")
    ptr = gp.guarded((7,), I32, name="ptr", device=CPU)
    rec = _base(rep, ptr)
    assert rec.pattern == 0 and all(bool((side == 0).all()) and pat == 0 for _, side, pat in rec.sides())
    rec.base[rec.before - 1] = 0
    rec.base[rec.before + 7] = 0
    assert rep.guards.check() == []
    rep.finish()


@pytest.mark.parametrize("dtype", [I32, torch.int64, torch.uint8])
def test_a_patterned_integer_guard_reports_a_stray_zero(dtype):
    """``pattern=``: guards and the unfilled payload hold a value no table can hold (negative, no zero byte), so a zero written
    beside the payload - ptr[0], the closing zero of a count - is reported, and so is any other valid value; an element of the
    payload nobody wrote still holds the pattern"""
    pat = gp.INT_PATTERN[dtype]
    nbytes = torch.empty(0, dtype=dtype).element_size()
    assert (pat < 0 or dtype == torch.uint8) and all((pat >> (8 * b)) & 0xFF for b in range(nbytes))
    rep = gp.Report("indices, patterned")
    out = gp.guarded((9,), dtype, name="lg_seg_ptr", device=CPU, pattern=pat)
    rec = _base(rep, out)
    assert rec.pattern == pat and bool((out == pat).all()) and bool((rec.base == pat).all())
    assert rep.guards.check() == []
    out[:8] = torch.arange(8, dtype=dtype)  # (the launch's own writes; element 8 is "left out")
    assert rep.guards.check() == [] and int((out == pat).nonzero()) == 8
    rec.base[rec.before + 9] = 0
    assert [f[:3] for f in rep.guards.check()] == [("lg_seg_ptr", "after", 0)]
    rec.base[rec.before + 9] = pat
    rec.base[rec.before - 2] = 0
    rec.base[rec.before - 1] = 5
    assert [f[:3] for f in rep.guards.check()] == [("lg_seg_ptr", "before", -1)]
    rec.base[rec.before - 1] = pat
    assert [f[:3] for f in rep.guards.check()] == [("lg_seg_ptr", "before", -2)]
    with pytest.raises(AssertionError, match="lg_seg_ptr: the guard before the payload changed at offset -2 elements"):
        rep.finish()


def test_pattern_goes_with_guard_input_and_fill_and_is_refused_for_floats():
    rep = gp.Report("indices, patterned inputs")
    pat = gp.INT_PATTERN[I32]
    idx = gp.guard_input(torch.arange(7, dtype=I32), "src", pattern=pat)
    rec = _base(rep, idx)
    assert torch.equal(idx, torch.arange(7, dtype=I32))
    assert all(bool((side == pat).all()) for _, side, _p in rec.sides())
    z = gp.guarded((3,), I32, fill=0, name="bad", device=CPU, pattern=pat)
    assert bool((z == 0).all()) and bool((_base(rep, z).base[:4] == pat).all())
    plain = gp.guard_input(torch.arange(7, dtype=I32), "plain")  # (beside patterned buffers: still guards of zeros)
    assert int(_base(rep, plain).base.abs().sum()) == 21
    rep.finish()
    with pytest.raises(ValueError, match="integer dtypes"):
        gp.guarded((3,), torch.float32, device=CPU, pattern=1)
    rec.base[rec.before + 7] = 0
    with pytest.raises(AssertionError, match="src: the guard after the payload changed at offset 0 elements"):
        rep.finish()


@pytest.mark.parametrize("where,side,offset,rows", [("before", "before", -1, -1 / 36), ("after", "after", 0, 0.0),
                                                     ("row_after", "after", 36, 1.0)])
def test_a_stray_write_is_reported_with_buffer_side_and_offset(where, side, offset, rows):
    rep = gp.Report("stray write")
    quiet = gp.guarded((9, 36), fill=0.0, name="quiet", device=CPU)
    gm = gp.guarded((9, 36), fill=0.0, name="GM", device=CPU)
    rec = _base(rep, gm)
    gp.gptr(gm), gp.gptr(quiet)
    rep.guards.launched("alignn_egc_bwd_dst")
    assert rep.guards.check() == []
    end = rec.before + rec.numel
    rec.base[{"before": rec.before - 1, "after": end, "row_after": end + 36}[where]] = 1.0
    found = rep.guards.check()
    assert [f[:4] for f in found] == [("GM", side, offset, rows)]
    assert "alignn_egc_bwd_dst" in found[0][4] and f"offset {offset} elements" in found[0][4]
    with pytest.raises(AssertionError, match="GM: the guard " + side):
        rep.finish()


def test_a_stray_write_beside_an_amax_slot_is_reported():
    """a one-float slot: the easiest neighbour for an atomicMax to hit; rewriting the very NaN it held (no payload) counts"""
    rep = gp.Report("amax")
    am = gp.guarded((1,), fill=0.0, name="gp_amax", device=CPU)
    rec = _base(rep, am)
    assert rec.before == 1024 and rep.guards.check() == []
    rec.base[rec.before + 1] = float("nan")
    assert [f[:3] for f in rep.guards.check()] == [("gp_amax", "after", 0)]
    rec.base[rec.before - 3] = 0.5
    assert [f[:3] for f in rep.guards.check()] == [("gp_amax", "before", -3), ("gp_amax", "after", 0)]
    assert float(am) == 0.0


def test_a_stray_read_that_is_used_fails_the_comparison():
    """a guard element copied into the payload of an input - what a kernel reading one row too far would use - poisons the
    restatement's output, and Report.record rejects it (``not e < allowed``)"""
    n, H = 6, 8
    gen = torch.Generator().manual_seed(5)
    gx, s0, hh = (torch.randn(n, H, generator=gen) for _ in range(3))
    s0 = s0.abs() + 0.1
    want = ref.node_reverse(gx.double(), s0.double(), hh.double())
    rep = gp.Report("stray read")
    g_in = gp.guard_input(gx, "GX")
    got = ref.node_reverse(g_in, s0, hh)
    rep.close("node_bwd", "GS1", got[0], want[0], None, 5e-5)
    assert not rep.failed
    rec = _base(rep, g_in)
    g_in[n - 1, H - 1] = rec.base[rec.before + rec.numel]  # the first element behind the payload
    got = ref.node_reverse(g_in, s0, hh)
    rep.close("node_bwd", "GS1", got[0], want[0], None, 5e-5)
    assert len(rep.failed) == 1 and rep.failed[0][:2] == ("node_bwd", "GS1")
    assert rep.guards.check() == []  # (a read leaves the guard as it is: only the poisoned output shows it)
    with pytest.raises(AssertionError):
        rep.finish()


def test_gptr_refuses_what_is_not_inside_a_payload():
    rep = gp.Report("gptr")
    t = gp.guarded((4, 8), fill=1.0, name="P", device=CPU)
    rec = _base(rep, t)
    assert gp.gptr(t) == t.data_ptr() and gp.gptr(None) is None
    assert gp.gptr(t[:, 4:]) == t.data_ptr() + 16  # (a column block: a strided view inside the payload)
    assert gp.gptr(t[1:3]) == t.data_ptr() + 32 * 1
    with pytest.raises(AssertionError, match="not in a guarded buffer"):
        gp.gptr(torch.zeros(4, 8))
    with pytest.raises(AssertionError, match="not in a guarded buffer"):
        gp.gptr(t.clone())
    for moved in (rec.base[rec.before + 8:rec.before + 40].view(4, 8),  # one row on: the last row lies in the guard
                  rec.base[rec.before - 1:rec.before + 31].view(4, 8), rec.base.as_strided((4, 8), (9, 1), rec.before)):
        with pytest.raises(AssertionError, match="a view of P covers elements"):
            gp.gptr(moved)
    gp.Report("another case")  # a new report owns a new registry: the earlier buffers are no longer known
    with pytest.raises(AssertionError, match="not in a guarded buffer"):
        gp.gptr(t)


def test_the_launcher_names_buffers_after_the_header():
    """a buffer allocated without a name is reported under the argument it was handed as"""
    rep = gp.Report("names")
    calls = []

    class Lib:
        def alignn_egc_node_bwd(self, *a):
            calls.append(a)
            return 0

        def alignn_egc_slabs(self, n):
            return 1

    lib = rep.launcher(Lib())
    bufs = [gp.guarded((3, 4), fill=0.0, device=CPU) for _ in range(5)]
    assert lib.alignn_egc_slabs(3) == 1
    assert lib.alignn_egc_node_bwd(gp.gptr(bufs[0]), 4, *(gp.gptr(t) for t in bufs[1:]), 3, 4, None) == 0
    assert [_base(rep, t).name for t in bufs] == [k + " of alignn_egc_node_bwd" for k in ("GXPRE", "S0", "HH", "GS1", "GS0")]
    assert rep.guards.launches == {"alignn_egc_node_bwd": [1, 5]} and len(calls) == 1
    rep.finish()
