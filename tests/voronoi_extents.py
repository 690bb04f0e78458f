"""The extents of every array the entry points of include/alignn_voronoi.h take, as the header states them, in the form of
tests/workflow_extents.py's ``TABLE`` and used through its ``Block(..., table=TABLE)``: the argument struct -> its header, the
entry points that take it, and per pointer field (dtype, element count, row length, one role per entry point).
tests/test_voronoi_abi.py checks the table against the header without a GPU; tests/test_gpu_voronoi_extents.py hands the guarded
buffers to the launches.  The four face arrays are looked at with ``faces = 1`` only: without it the caller leaves them NULL
(``Block.alloc(..., null=FACES)``).  The table only restates the header comments."""

import torch

from tests.workflow_extents import CELLS, ROLES, TRAJ, _f, _same  # noqa: F401

F64, I32, I64 = torch.float64, torch.int32, torch.int64
FACES = ("face_j", "face_d", "face_area", "face_edges")
ROWS = "n_frames * N"  # a row per (frame used, atom)

TABLE = {
    "alignn_voro_args": dict(
        header="alignn_voronoi.h", entries=("alignn_voro_cells", "alignn_voro_means"),
        let=dict(B="n_structs", N="n_atoms", S="n_species"), derived={},
        fields=dict(
            traj=_f(F64, TRAJ, 3, "in", "unused"), lattice=_f(F64, CELLS, 3, "in", "unused"), atom_ptr=_same(I32, "B + 1", 1, 2, "in"),
            group=_same(I32, "N", 1, 2, "in"), group_count=_f(I32, "B * (S + 1)", "S + 1", "in", "unused"),
            r_cut=_f(F64, "B", 1, "in", "unused"),
            volume=_f(F64, ROWS, 1, "out", "in"), area=_f(F64, ROWS, 1, "out", "in"), r_max=_f(F64, ROWS, 1, "out", "unused"),
            n_faces=_f(I32, ROWS, 1, "out", "in"), index=_f(I32, ROWS + " * ALIGNN_VORO_INDEX", "ALIGNN_VORO_INDEX", "out", "unused"),
            complete=_f(I32, ROWS, 1, "out", "in"),
            mean=_f(F64, "B * (S + 1) * n_frames * 3", 3, "unused", "out"), n_complete=_f(I64, "B * (S + 1) * n_frames", 1, "unused", "out"),
            face_j=_f(I32, ROWS + " * ALIGNN_VORO_MAX_FACES", "ALIGNN_VORO_MAX_FACES", "out", "unused"),
            face_d=_f(F64, ROWS + " * ALIGNN_VORO_MAX_FACES * 3", 3, "out", "unused"),
            face_area=_f(F64, ROWS + " * ALIGNN_VORO_MAX_FACES", "ALIGNN_VORO_MAX_FACES", "out", "unused"),
            face_edges=_f(I32, ROWS + " * ALIGNN_VORO_MAX_FACES", "ALIGNN_VORO_MAX_FACES", "out", "unused"),
            status=_f(I32, "1", 1, "add", "unused"))),
}


def entry_points():
    """entry point -> the struct it takes"""
    return {e: s for s, t in TABLE.items() for e in t["entries"]}
