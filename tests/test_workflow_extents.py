"""tests/workflow_extents.py against the six headers it restates, without a GPU: the table names every pointer field of every
argument struct and nothing else, its extents rest on the struct's own scalars, every entry point has a role for every array - and
the guard bands report a stray write beside a buffer that the helper built."""

import ctypes as C
import re

import pytest
import torch

from alignn_amd import _abi
from tests import gate_parity as gp
from tests import workflow_extents as wx

HEADERS = ("alignn_sym.h", "alignn_cells.h", "alignn_phsym.h", "alignn_local.h", "alignn_order.h", "alignn_traj.h")
# the entry points of those headers that take no argument block (flat prototypes): not in the table
FLAT = {"alignn_traj_vdos", "alignn_traj_fit", "alignn_traj_green_kubo"}
CTYPE = {torch.float64: "double", torch.int32: "int32_t", torch.int64: "int64_t", torch.uint8: "uint8_t"}


def _pointer_fields(struct):
    return [n for n, t in struct._fields_ if t is C.c_void_p]


def _scalar_fields(struct):
    return {n for n, t in struct._fields_ if t is not C.c_void_p}


def test_the_table_names_every_struct_and_every_launching_entry_point_of_the_six_headers():
    structs, entries = {}, set()
    for name in HEADERS:
        h = _abi.header(name)
        structs.update({s: name for s in h.structs})
        entries |= {e for e in h.signatures if not e.endswith("_size")}
    assert {s: t["header"] for s, t in wx.TABLE.items()} == structs
    assert set(wx.entry_points()) == entries - FLAT
    assert len(wx.entry_points()) == sum(len(t["entries"]) for t in wx.TABLE.values()) == 26


@pytest.mark.parametrize("struct", list(wx.TABLE))
def test_every_pointer_field_has_an_extent_and_a_role_per_entry_point(struct):
    table, h = wx.TABLE[struct], wx.header_of(struct)
    cls = h.structs[struct]
    assert list(table["fields"]) == _pointer_fields(cls)  # every pointer field, no other, in the header's order
    known = _scalar_fields(cls) | set(h.defines) | set(table["derived"])
    assert not set(table["derived"]) & {n for n, _ in cls._fields_} and not set(table["let"]) & known
    for field, spec in table["fields"].items():
        assert len(spec["roles"]) == len(table["entries"]) and set(spec["roles"]) <= set(wx.ROLES), field
        assert any(r != "unused" for r in spec["roles"]), field
        counts = spec["count"].values() if isinstance(spec["count"], dict) else [spec["count"]]
        if isinstance(spec["count"], dict):
            assert set(spec["count"]) == set(table["entries"]), field
        for expr in list(counts) + [spec["row"]]:
            assert wx.names_used(struct, expr) <= known, (field, expr, wx.names_used(struct, expr) - known)
    # the dtype is the header's: the declaration of the field, read from the text
    with open(h.path) as f:
        text = _abi._uncomment(f.read())
    body = text[text.index("typedef struct " + struct):text.index("} " + struct)]
    for field, spec in table["fields"].items():
        name = "in" if field == "in_" else field  # (_abi.parse renames a Python keyword)
        assert re.search(rf"\b{CTYPE[spec['dtype']]}\s*\*\s*{name}\s*;", body), (field, spec["dtype"])


def test_extents_follow_the_scalars():
    rep = gp.Report("extents")
    b = wx.Block(rep.guards, "alignn_traj_rdf_args", device="cpu")
    b.set(n_structs=3, n_atoms=76, n_species=3, n_bins=67, n_total_frames=5, n_frames=2, lattice_per_frame=0, r_max=6.0)
    assert b.extent("counts") == (3 * 7 * 67, 67) and b.extent("lattice") == (27, 3) and b.extent("traj") == (3 * 5 * 76, 3)
    b.set(lattice_per_frame=1)
    assert b.extent("lattice") == (5 * 27, 3)
    s = wx.Block(rep.guards, "alignn_sym_find_args", device="cpu").set(n_structs=2, n_atoms=7, n_ops_total=60, n_map_total=200)
    assert s.extent("accepted") == (48 * 7, 1) and s.extent("rotations") == (540, 3) and s.extent("lattice_ops") == (2 * 48 * 9, 9)
    a = wx.Block(rep.guards, "alignn_sym_apply_args", device="cpu").set(n_structs=2, n_atoms=7)
    assert a.extent("out", "alignn_sym_stress") == (18, 3) and a.extent("out", "alignn_sym_forces") == (21, 3)
    q = wx.Block(rep.guards, "alignn_local_bond_args", device="cpu").set(n_atoms=6, n_ls=4, chunk_frames=2, n_frames=3)
    assert q.extent("qlm") == (2 * 6 * 4 * 13 * 2, 2) and q.extent("w3j") == (4 * 625, 625) and q.extent("q") == (72, 4)
    sq = wx.Block(rep.guards, "alignn_order_sq_args", device="cpu").set(n_frames=130, n_species=2, n_vectors=11)
    assert sq.extent("partial") == (3 * 4 * 11, 11)
    d = wx.Block(rep.guards, "alignn_phsym_displace_args", device="cpu").set(n_structs=2, n_jobs=3, N=5, rows=48)
    assert d.extent("frac") == (144, 3) and d.extent("dirs") == (45, 3) and d.extent("jobs") == (12, 4)


def test_payloads_follow_the_roles():
    """inputs are copies between patterned guards, ``add`` arrays hold zeros, ``out`` arrays the pattern - and count as
    unwritten until every element has been overwritten; an extent of zero is a NULL pointer"""
    rep = gp.Report("roles")
    ptr = torch.tensor([0, 1, 6], dtype=torch.int32)
    scalars = dict(n_structs=2, n_atoms=6, max_atoms=5, n_species=1, n_bins=5, n_total_frames=1, n_frames=1, frame_step=1, r_max=2.0)
    inputs = dict(traj=torch.zeros(1, 6, 3, dtype=torch.float64), lattice=torch.eye(3, dtype=torch.float64).repeat(2, 1, 1),
                  atom_ptr=ptr, group=torch.ones(6, dtype=torch.int32), group_count=torch.tensor([[1, 1], [5, 5]], dtype=torch.int32))
    b = wx.Block(rep.guards, "alignn_traj_rdf_args", device="cpu").set(**scalars).alloc("alignn_traj_rdf_counts", inputs)
    assert set(b.payload) == {"traj", "lattice", "atom_ptr", "group", "group_count", "counts", "status"}
    assert torch.equal(b.payload["atom_ptr"], ptr) and not b.payload["counts"].any() and not b.payload["status"].any()
    rec = rep.guards.record_of(b.payload["atom_ptr"])
    assert rec.pattern == gp.INT_PATTERN[torch.int32] and rec.numel == 3 and b.args.atom_ptr == b.payload["atom_ptr"].data_ptr()
    assert b.args.g is None
    b.alloc("alignn_traj_rdf_normalise")
    assert b.payload["g"].shape == (4, 5) and wx.pattern_left(b.payload["g"]) == 20 and wx.pattern_left(b.payload["counts"]) == 0
    assert b.unwritten("alignn_traj_rdf_normalise") == [("g", 20), ("coord", 20), ("volume", 2), ("centres", 5)]
    for k in ("g", "coord", "volume"):
        b.payload[k].zero_()
    b.payload["centres"][:4] = 0.0
    assert b.unwritten("alignn_traj_rdf_normalise") == [("centres", 1)] and b.unwritten("alignn_traj_rdf_counts") == []
    with pytest.raises(AssertionError, match="left elements unwritten"):
        b.written("alignn_traj_rdf_normalise")
    with pytest.raises(AssertionError, match="the header says"):
        wx.Block(rep.guards, "alignn_traj_rdf_args", device="cpu").set(**scalars).alloc(
            "alignn_traj_rdf_counts", dict(inputs, group=torch.ones(7, dtype=torch.int32)))
    args, payload = wx.block(rep.guards, "alignn_sym_apply_args", dict(n_structs=1, n_atoms=2, n_ops_total=0, n_map_total=0),
                             dict(lattice=torch.eye(3, dtype=torch.float64)[None], in_=torch.ones(2, 3, dtype=torch.float64),
                                  atom_ptr=torch.tensor([0, 2], dtype=torch.int32), op_ptr=torch.zeros(2, dtype=torch.int64),
                                  map_ptr=torch.zeros(2, dtype=torch.int64)), entry="alignn_sym_forces", device="cpu")
    assert payload["rotations"] is None and payload["atom_map"] is None and args.rotations is None and args.out == payload["out"].data_ptr()
    rep.finish()


@pytest.mark.parametrize("field,dtype,where,side,offset", [("volume", torch.float64, "row_before", "before", -1),
                                                           ("counts", torch.int64, "after", "after", 0),
                                                           ("accepted", torch.uint8, "after", "after", 0)])
def test_a_stray_write_beside_a_buffer_of_the_helper_is_reported(field, dtype, where, side, offset):
    """the planted-write detector of tests/test_gate_parity_guards.py on buffers built by ``Block``: a write one element behind
    an int64 and a uint8 array, one row in front of a float64 array; named by the struct's field"""
    rep = gp.Report("stray write, workflow")
    if field == "accepted":
        b = wx.Block(rep.guards, "alignn_sym_find_args", device="cpu").set(n_structs=1, n_atoms=3, max_atoms=3, symprec=1e-3)
        b.alloc("alignn_sym_search", dict(lattice=torch.eye(3, dtype=torch.float64)[None], pos=torch.zeros(3, 3, dtype=torch.float64),
                                          atom_ptr=torch.tensor([0, 3], dtype=torch.int32), order=torch.arange(3, dtype=torch.int32),
                                          seg_lo=torch.zeros(3, dtype=torch.int32), seg_hi=torch.full((3,), 3, dtype=torch.int32),
                                          pivot_lo=torch.zeros(1, dtype=torch.int32), pivot_hi=torch.full((1,), 3, dtype=torch.int32)))
    else:
        b = wx.Block(rep.guards, "alignn_traj_rdf_args", device="cpu").set(n_structs=2, n_species=1, n_bins=5)
        b.alloc("alignn_traj_rdf_normalise", dict(lattice=torch.eye(3, dtype=torch.float64).repeat(2, 1, 1),
                                                  group_count=torch.ones(2, 2, dtype=torch.int32),
                                                  **({"counts": torch.zeros(2, 2, 5, dtype=torch.int64)} if field == "counts" else {})),
                null=("counts",) if field != "counts" else ())
    t = b.payload[field]
    rec = rep.guards.record_of(t)
    assert t.dtype == dtype and rep.guards.check() == []
    at = rec.before + rec.numel if where == "after" else rec.before - rec.row
    rec.base[at] = 0  # (a valid value of every one of these arrays)
    found = rep.guards.check()
    assert [f[:3] for f in found] == [(f"{field} of {b.struct}", side, offset)]
    with pytest.raises(AssertionError, match=f"{field} of {b.struct}: the guard {side}"):
        rep.finish()
