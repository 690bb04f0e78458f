"""The device-free input checks the trajectory analyses share (alignn_amd/_trajectory_inputs.py): what they accept, what they
return and the messages they raise, as ``trajectory``, ``order`` and ``local_order`` had them when each kept its own copy."""

import re
from pathlib import Path

import numpy as np
import pytest
import torch

from alignn_amd import _trajectory_inputs as ti
from alignn_amd import local_order, order, trajectory


def _raises(message, fn, *args, **kw):
    with pytest.raises(ValueError, match="^" + re.escape(message) + "$"):
        fn(*args, **kw)


def test_frames_select_as_a_slice_does():
    assert ti._frames("t", 10, None, None, None) == (0, 1, 10)
    assert ti._frames("t", 10, 1, None, 3) == (1, 3, 3)  # 1, 4, 7
    assert ti._frames("t", 10, -3, None, None) == (7, 1, 3)
    assert ti._frames("t", 10, None, -8, 2) == (0, 2, 1)
    assert ti._frames("t", 10, np.int64(2), np.int32(6), None) == (2, 1, 4)
    for empty in ((5, 5, None), (8, 2, None), (10, None, None), (-20, -15, 4)):
        assert ti._frames("t", 10, *empty) == (0, 1 if empty[2] is None else empty[2], 0)
    assert ti._frames("t", 0, None, None, None) == (0, 1, 0)
    for step in (0, -1):
        _raises(f"t: step must be >= 1, got {step}", ti._frames, "t", 10, None, None, step)
    _raises("t: start must be an int or None, got True", ti._frames, "t", 10, True, None, None)
    _raises("t: stop must be an int or None, got 2.0", ti._frames, "t", 10, None, 2.0, None)
    _raises("t: step must be an int or None, got '1'", ti._frames, "t", 10, None, None, "1")


def test_degrees_are_one_to_four_distinct_integers():
    assert ti.degrees("t", (4, 6), 4, 12) == (4, 6)
    assert ti.degrees("t", [12, np.int64(1), 6, 4], 4, 12) == (12, 1, 6, 4)
    assert all(type(l) is int for l in ti.degrees("t", [np.int32(3)], 4, 12))
    for bad in ((), [], (1, 2, 3, 4, 5), (4, 4), (6, 4, 6), (0,), (4, 13), (-2,), (True,), (4, np.True_), (4.0,), 4, "46", None,
                np.array([4, 6]), iter((4, 6))):
        _raises(f"t: ls must be 1 to 4 distinct integers in 1 .. 12, got {bad!r}", ti.degrees, "t", bad, 4, 12)
    _raises("u: ls must be 1 to 2 distinct integers in 1 .. 6, got (1, 2, 3)", ti.degrees, "u", (1, 2, 3), 2, 6)
    assert (order.MAX_LS, order.MAX_L) == (local_order.MAX_LS, local_order.MAX_L) == (4, 12)


def test_bins_in_both_flavours():
    for bool_ok in (False, True):
        assert ti.bins("t", 1, 1024, bool_ok) == 1 and ti.bins("t", 1024, 1024, bool_ok) == 1024
        assert ti.bins("t", np.int64(7), 1024, bool_ok) == 7
        for bad in (0, -1, 1025, 1.0, 7.5, "7", None, np.float64(7.0)):
            _raises(f"t: n_bins must be 1 .. 1024, got {bad!r}", ti.bins, "t", bad, 1024, bool_ok)
    assert type(ti.bins("t", np.int64(7), 1024)) is int
    # adf and structure_factor refuse a bool; rdf has always let one through its check, a bool being an Integral
    _raises("t: n_bins must be 1 .. 1024, got True", ti.bins, "t", True, 1024)
    _raises("t: n_bins must be 1 .. 1024, got False", ti.bins, "t", False, 1024)
    assert ti.bins("t", True, 4096, bool_ok=True) is True
    _raises("t: n_bins must be 1 .. 4096, got False", ti.bins, "t", False, 4096, bool_ok=True)  # (it is 0)
    assert (trajectory.MAX_BINS, order.MAX_BINS) == (4096, 1024)


def test_positive_is_a_finite_real_above_zero_and_no_bool():
    assert ti._positive("t", "x", 2) == 2.0 and type(ti._positive("t", "x", 2)) is float
    assert ti._positive("t", "x", np.float32(0.5)) == 0.5 and ti._positive("t", "x", 1e-300) == 1e-300
    for bad in (0, 0.0, -1.5, float("inf"), float("-inf"), float("nan"), True, np.True_, "1", None, 1j):
        _raises(f"t: x must be a finite number > 0, got {bad!r}", ti._positive, "t", "x", bad)


def test_the_shared_fields_are_those_a_block_declares():
    """On the host: a record filled by hand (``inputs`` itself wants the trajectory on the GPU)."""
    ns = [3, 5]
    traj, cells = torch.zeros(7, 8, 3, dtype=torch.float64), torch.zeros(7, 2, 3, 3, dtype=torch.float64)
    sel = ti.Inputs("t", traj, ns, cells, *ti._frames("t", 7, 1, None, 2))
    assert sel.groups([np.array([8, 1, 8]), np.array([14] * 5)]) == (2, [[1, 8], [14]])
    assert sel.atom_ptr.tolist() == [0, 3, 8] and sel.group.tolist() == [2, 1, 2, 1, 1, 1, 1, 1]
    assert sel.group_count.tolist() == [[3, 1, 2], [5, 5, 0]]
    status = torch.zeros(1, dtype=torch.int32)
    want = dict(traj=traj.data_ptr(), lattice=cells.data_ptr(), atom_ptr=sel.atom_ptr.data_ptr(), group=sel.group.data_ptr(),
                group_count=sel.group_count.data_ptr(), status=status.data_ptr(), n_structs=2, n_atoms=8, max_atoms=5, n_species=2,
                n_total_frames=7, frame0=1, frame_step=2, n_frames=3, lattice_per_frame=1)
    for Args in (trajectory.RdfArgs, order.AngleArgs, local_order.CnaArgs, local_order.BondArgs):
        assert sel.fields(Args, status) == want
        assert all(getattr(Args(**sel.fields(Args, status)), k) == v for k, v in want.items())
    sq = sel.fields(order.SqArgs, status)
    assert sq == {k: v for k, v in want.items() if k not in ("max_atoms", "lattice_per_frame")}
    order.SqArgs(**sq)
    sel.lattices = cells[0]
    assert sel.fields(trajectory.RdfArgs, status)["lattice_per_frame"] == 0


def test_no_module_takes_a_private_name_from_a_sibling():
    package = Path(trajectory.__file__).parent
    for path in package.glob("*.py"):
        assert not re.search(r"from \.(order|trajectory|local_order) import _", path.read_text()), path.name
