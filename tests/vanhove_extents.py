"""The extents of every array the entry points of include/alignn_vanhove.h take, as the header states them, in the form of
tests/workflow_extents.py's ``TABLE`` and used through its ``Block(..., table=TABLE)``: argument struct -> its header, the entry
points that take it, and per pointer field (dtype, element count, row length, one role per entry point).  tests/test_vanhove_abi.py
checks the table against the header without a GPU; tests/test_gpu_vanhove_extents.py hands the guarded buffers to the launches.

One role beyond those of tests/workflow_extents.py: ``host`` - ``lags_host``, the one array in host memory, which the entry point
reads itself before it launches.  ``Block.alloc`` is told to leave it NULL (``null=HOST``) and the caller points it at its own
numpy array (``set_lags``): a guard band is for what a kernel may write beside.  The table only restates the header comments."""

import torch

from tests.workflow_extents import _f, _same

F64, I32, I64 = torch.float64, torch.int32, torch.int64
ROLES = ("in", "out", "add", "scratch", "unused", "host")
HOST = ("lags_host",)
TRAJ = "3 * n_total_frames * N"
ROWS = "B * (S + 1) * L"  # a row per (structure, group, lag)
PAIRS = "B * P * L"       # a row per (structure, pair row, lag)

TABLE = {
    "alignn_vh_self_args": dict(
        header="alignn_vanhove.h", entries=("alignn_vh_self", "alignn_vh_self_finish"),
        let=dict(B="n_structs", N="n_atoms", S="n_species", L="n_lags"), derived={},
        fields=dict(
            traj=_f(F64, TRAJ, 3, "in", "unused"), atom_ptr=_f(I32, "B + 1", 1, "in", "unused"), group=_f(I32, "N", 1, "in", "unused"),
            group_count=_same(I32, "B * (S + 1)", "S + 1", 2, "in"), com=_f(F64, "3 * n_frames * B", 3, "in", "unused"),
            lags=_same(I32, "L", 1, 2, "in"), lags_host=_same(I32, "L", 1, 2, "host"), q=_f(F64, "n_q", 1, "in", "unused"),
            counts=_f(I64, ROWS + " * n_bins", "n_bins", "add", "in"), overflow=_f(I64, ROWS, "L", "add", "unused"),
            sums=_f(F64, ROWS + " * 2", 2, "out", "in"), fs_sum=_f(F64, ROWS + " * n_q", "n_q", "out", "in"),
            moments=_f(F64, ROWS + " * 2", 2, "unused", "out"), alpha2=_f(F64, ROWS, "L", "unused", "out"),
            p=_f(F64, ROWS + " * n_bins", "n_bins", "unused", "out"), gs=_f(F64, ROWS + " * n_bins", "n_bins", "unused", "out"),
            fs=_f(F64, ROWS + " * n_q", "n_q", "unused", "out"), centres=_f(F64, "n_bins", 1, "unused", "out"))),
    "alignn_vh_distinct_args": dict(
        header="alignn_vanhove.h", entries=("alignn_vh_distinct", "alignn_vh_distinct_finish"),
        let=dict(B="n_structs", N="n_atoms", S="n_species", L="n_lags", P="1 + n_species * (n_species + 1) // 2"), derived={},
        fields=dict(
            traj=_f(F64, TRAJ, 3, "in", "unused"), lattice=_same(F64, "9 * B", 3, 2, "in"), atom_ptr=_f(I32, "B + 1", 1, "in", "unused"),
            group=_f(I32, "N", 1, "in", "unused"), group_count=_same(I32, "B * (S + 1)", "S + 1", 2, "in"),
            com=_f(F64, "3 * n_frames * B", 3, "in", "unused"), lags=_same(I32, "L", 1, 2, "in"),
            lags_host=_same(I32, "L", 1, 2, "host"), counts=_f(I64, PAIRS + " * n_bins", "n_bins", "add", "in"),
            g=_f(F64, PAIRS + " * n_bins", "n_bins", "unused", "out"), volume=_f(F64, "B", 1, "unused", "out"),
            centres=_f(F64, "n_bins", 1, "unused", "out"), status=_f(I32, "1", 1, "add", "unused"))),
    "alignn_vh_fqt_args": dict(
        header="alignn_vanhove.h", entries=("alignn_vh_fqt_modes", "alignn_vh_fqt_correlate", "alignn_vh_fqt_bin"),
        let=dict(B="n_structs", N="n_atoms", S="n_species", L="n_lags", V="n_vectors", P="1 + n_species * (n_species + 1) // 2"),
        derived={},
        fields=dict(
            traj=_f(F64, TRAJ, 3, "in", "unused", "unused"), lattice=_f(F64, "9 * B", 3, "in", "unused", "unused"),
            atom_ptr=_f(I32, "B + 1", 1, "in", "unused", "unused"), group=_f(I32, "N", 1, "in", "unused", "unused"),
            group_count=_f(I32, "B * (S + 1)", "S + 1", "unused", "in", "unused"), vec_ptr=_same(I32, "B + 1", 1, 3, "in"),
            hkl=_f(I32, "3 * V", 3, "in", "unused", "unused"), vbin=_f(I32, "V", 1, "unused", "unused", "in"),
            lags=_f(I32, "L", 1, "unused", "in", "unused"), lags_host=_f(I32, "L", 1, "unused", "host", "unused"),
            modes=_f(F64, "2 * n_frames * S * V", 2, "out", "in", "unused"), f_vec=_f(F64, "P * L * V", "V", "unused", "out", "in"),
            f=_f(F64, PAIRS + " * n_bins", "n_bins", "unused", "unused", "out"),
            n_vectors_bin=_f(I64, "B * n_bins", "n_bins", "unused", "unused", "out"),
            centres=_f(F64, "n_bins", 1, "unused", "unused", "out"))),
}


def entry_points():
    """entry point -> the struct it takes"""
    return {e: s for s, t in TABLE.items() for e in t["entries"]}


def set_lags(block, lags):
    """points ``lags_host`` of a ``workflow_extents.Block`` at the int32 numpy array ``lags``, which the caller keeps alive"""
    assert lags.dtype.name == "int32" and lags.flags["C_CONTIGUOUS"] and len(lags) == block.args.n_lags
    block.args.lags_host = lags.ctypes.data
    return block
