"""The launches of include/alignn_voronoi.h, each between the guard bands of tests/gate_parity.py, every buffer of exactly the
extent the header states (tests/voronoi_extents.py, through ``workflow_extents.Block``).  The argument block is filled here in the
sequence the driver uses.  Asserted per entry point, in this order: (a) no guard bit changed after the launch; (b) no array the
header calls written holds a pattern element; (c) every output equals, bit for bit, what the driver returns for the same inputs on
its own plain allocations.  The shapes are those of tests/test_gpu_voronoi.py (tests/voronoi_ref.py holds them), with ``faces`` on
and off - off, the four face arrays are NULL.

Blind spots (those of the instrument): an access farther from a buffer than its guard - 1024 elements or two rows - and a read
beside a buffer whose value is never used."""

import numpy as np
import pytest
import torch

from alignn_amd import _lib, voronoi
from alignn_amd import _trajectory_inputs as TI
from alignn_amd.voronoi import _load
from tests import gate_parity as gp
from tests import voronoi_extents as vx
from tests import voronoi_ref as ref
from tests import workflow_extents as wx

pytestmark = pytest.mark.gpu
DEV = "cuda"
F64, I32 = torch.float64, torch.int32
OUTPUTS = ("volume", "area", "r_max", "n_faces", "index", "mean", "n_complete")


def _t(x, dtype=F64):
    return torch.tensor(np.ascontiguousarray(x), dtype=dtype, device=DEV)


def _eq(a, b):
    a, b = a.reshape(-1), b.reshape(-1)
    if a.dtype == F64:
        a, b = a.view(torch.int64), b.view(torch.int64)
    return a.numel() == b.numel() and a.dtype == b.dtype and torch.equal(a, b)


def _cases():
    crystals = [(C, traj, r_cut) for C, traj, r_cut, _ in map(ref.crystal, ref.CRYSTALS)]
    generic = [ref.generic("J") + (ref.GENERIC_R_CUT,), ref.generic("K") + (ref.GENERIC_R_CUT,)]
    cells, traj = ref.scaled()
    slab = [ref.slab() + (ref.SLAB_R_CUT,)]
    return {"crystals": (crystals, None, ref.CRYSTAL_THRESHOLDS, {}), "batch": (crystals[:1] + crystals[2:4] + generic, None, ref.CRYSTAL_THRESHOLDS, {}),
            "generic": (generic, [ref.GENERIC_SPECIES, np.full(32, 13)], {}, dict(start=1, step=2)),
            "scaled": ([(cells[:, 0], traj, ref.GENERIC_R_CUT)], None, dict(relative_face_threshold=ref.REL_THRESHOLD, edge_threshold=ref.EDGE_THRESHOLD), {}),
            "slab": (slab, None, ref.CRYSTAL_THRESHOLDS, {})}


@pytest.mark.parametrize("faces", [False, True])
@pytest.mark.parametrize("case", ["crystals", "batch", "generic", "scaled", "slab"])
def test_voronoi_between_guards(case, faces):
    structs, species, thresholds, select = _cases()[case]
    per_frame = np.ndim(structs[0][0]) == 3
    lattices = _t(np.stack([s[0] for s in structs], axis=1 if per_frame else 0))
    traj = _t(np.concatenate([s[1] for s in structs], axis=1))
    ns, cuts = [s[1].shape[1] for s in structs], [s[2] for s in structs]
    rep = gp.Report(f"voronoi {case} faces={int(faces)}", tag="voronoi-extents")
    lib = _load()
    rec = TI.inputs("voronoi", traj, lattices, ns, select.get("start"), None, select.get("step"))
    S, _ = rec.groups(species)
    b = wx.Block(rep.guards, "alignn_voro_args", DEV, rep.case, table=vx.TABLE)
    b.set(n_structs=len(ns), n_atoms=sum(ns), max_atoms=max(ns), n_species=S, n_total_frames=traj.shape[0], frame0=rec.frame0,
          frame_step=rec.frame_step, n_frames=rec.n_frames, lattice_per_frame=int(per_frame), faces=int(faces),
          face_threshold=thresholds.get("face_threshold", 0.0), relative_face_threshold=thresholds.get("relative_face_threshold", 0.0),
          edge_threshold=thresholds.get("edge_threshold", 0.0))
    inputs = dict(traj=traj, lattice=lattices, atom_ptr=rec.atom_ptr, group=rec.group, group_count=rec.group_count, r_cut=_t(cuts))
    null = () if faces else vx.FACES
    b.alloc("alignn_voro_cells", inputs, null=null)
    b.launch(lib, "alignn_voro_cells", _lib.stream()).written("alignn_voro_cells")
    b.alloc("alignn_voro_means", null=null)
    b.launch(lib, "alignn_voro_means", _lib.stream()).written("alignn_voro_means")
    assert int(b.payload["status"]) == 0
    res = voronoi(traj, lattices, ns, species, r_cut=cuts, faces=faces, strict=False, **thresholds, **select)
    P = b.payload
    for field in OUTPUTS + (vx.FACES if faces else ()):
        assert _eq(P[field], getattr(res, field)), field
    assert _eq(P["complete"] != 0, res.complete) and all(P.get(f) is None for f in (() if faces else vx.FACES))
    assert int(res.n_faces.sum()) > 0 and (case != "slab" or not bool(res.complete.all()))
    rep.finish()  # (prints the case's launches and guarded buffers, per entry point)
