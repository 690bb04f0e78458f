"""tests/workflow_extents.py against the six headers it restates, without a GPU: the table names every pointer field of every
argument struct and nothing else, its extents rest on the struct's own scalars, every entry point has a role for every array - and
the guard bands report a stray write beside a buffer that the helper built."""

import ctypes as C
import re

import pytest
import torch

from alignn_amd import _abi
from tests import gate_parity as gp
from tests import step_extents as sx
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


# ----------------------------------------------------------------------------------------------------------------------
# tests/step_extents.py: the argument blocks of the step kernels and the flat prototypes
# ----------------------------------------------------------------------------------------------------------------------
STEP_ENTRIES = {
    "alignn_fire_step", "alignn_md_step", "alignn_neb_forces", "alignn_idpp_forces", "alignn_md_init_momenta", "alignn_neb_interpolate",
    "alignn_phonon_displace", "alignn_phonon_fc_rows", "alignn_phonon_symmetrize", "alignn_phonon_acoustic", "alignn_phonon_mass_weight",
    "alignn_phonon_eigh", "alignn_phonon_dos", "alignn_defect_supercells", "alignn_slab_build", "alignn_strain_build", "alignn_eos_fit",
    "alignn_elastic_fit", "alignn_zsl_match", "alignn_interface_build", "alignn_phonon_thermal", "alignn_qha_derive", "alignn_traj_vdos",
    "alignn_traj_fit", "alignn_traj_green_kubo"}


def test_the_step_tables_name_every_listed_entry_point():
    assert set(sx.ENTRIES) == STEP_ENTRIES and len(sx.ENTRIES) == len(STEP_ENTRIES) == 25
    assert set(sx.STRUCTS) == {"alignn_fire_args", "alignn_md_args", "alignn_neb_args", "alignn_idpp_args"}
    assert FLAT <= set(sx.FLAT)  # what the six headers' table leaves out is covered here
    # with the six headers' table: every launching entry point of every workflow header (the size and workspace queries launch nothing)
    for name in _abi.WORKFLOW_HEADERS + _abi.LATER_HEADERS:
        launching = {e for e in _abi.header(name).signatures if not e.endswith(("_size", "_workspace"))}
        assert launching <= set(sx.ENTRIES) | set(wx.entry_points()), (name, launching - set(sx.ENTRIES) - set(wx.entry_points()))
    for struct, table in sx.STRUCTS.items():
        h = wx.header_of(struct, sx.STRUCTS)
        assert struct in h.structs and all(e in h.signatures for e in table["entries"])
    for entry, table in sx.FLAT.items():
        assert entry in wx.read_header(table["header"]).signatures


def _checked_against(declared, table, struct, tables, scalars, defines):
    """``declared``: [(name, type name, pointer?, const?)] from the header's text"""
    pointers = [d for d in declared if d[2] and d[0] != "stream"]
    assert list(table["fields"]) == [d[0] for d in pointers]  # every pointer, no other, in the header's order
    known = set(scalars) | set(defines) | set(table["derived"])
    assert not set(table["derived"]) & {d[0] for d in declared} and not set(table["let"]) & known
    for (name, ctype, _, const), spec in zip(pointers, table["fields"].values()):
        (role,) = spec["roles"]
        assert role in sx.ROLES and role != "unused", name
        assert ctype == sx.CTYPE[spec["dtype"]] or (ctype, spec["dtype"]) == ("void", torch.uint8), (name, ctype)
        assert const == (role == "in"), (name, role)  # a const pointer is read only, and no other is called an input
        assert (spec["writes"] is None) == (role == "in") or role == "scratch", name  # which elements a launch writes
        assert spec["whole"] == (spec["writes"] == "all") or (spec["whole"] and role == "out" and spec["writes"].startswith("all (")), name
        for expr in (spec["count"], spec["row"]):
            used = wx.names_used(struct, expr, tables)
            assert used <= known, (name, expr, used - known)


@pytest.mark.parametrize("struct", list(sx.STRUCTS))
def test_every_pointer_field_of_a_step_block_has_its_extent_dtype_and_role(struct):
    declared = sx.struct_fields(struct)
    cls = wx.header_of(struct, sx.STRUCTS).structs[struct]
    assert [d[0] for d in declared] == [n for n, _ in cls._fields_]  # (the text was read as _abi reads it)
    assert [d[0] for d in declared if d[2]] == _pointer_fields(cls)
    _checked_against(declared, sx.STRUCTS[struct], struct, sx.STRUCTS, _scalar_fields(cls), wx.header_of(struct, sx.STRUCTS).defines)


@pytest.mark.parametrize("entry", list(sx.FLAT))
def test_every_pointer_parameter_of_a_flat_entry_point_has_its_extent_dtype_and_role(entry):
    declared = sx.prototype(entry)
    h = wx.read_header(sx.FLAT[entry]["header"])
    argtypes = h.signatures[entry][1]
    assert len(declared) == len(argtypes)
    assert [d[2] or d[1] == "alignn_stream_t" for d in declared] == [t is C.c_void_p for t in argtypes]
    _checked_against(declared, sx.FLAT[entry], entry, sx.FLAT, {d[0] for d in declared if not d[2]}, h.defines)


def test_step_extents_follow_the_scalars():
    rep = gp.Report("step extents")
    f = wx.Block(rep.guards, "alignn_fire_args", device="cpu", table=sx.STRUCTS).set(n_active=3, B=4, N=266, force_rows=263)
    assert f.extent("forces") == (789, 3) and f.extent("status") == (4, 1) and f.extent("stress") == (27, 3)
    assert f.extent("positions") == (798, 3) and f.extent("fixed") == (266, 1) and f.extent("state") == (8, 2)
    m = wx.Block(rep.guards, "alignn_md_args", device="cpu", table=sx.STRUCTS).set(n_structures=3, N=260, n_rows=260, steps=5, interval=2,
                                                                                  ensemble=1)
    assert m.extent("epot") == (9, 3) and m.extent("traj_positions") == (3 * 3 * 260, 3) and m.extent("traj_lattice") == (81, 3)
    assert m.extent("noise_out") == (260 * 18, 18) and m.extent("nhc_state") == (102, 34) and m.extent("seeds") == (3, 1)
    m.set(ensemble=3, steps=6, n_rows=261)
    assert m.extent("noise_out") == (260 * 36, 36) and m.extent("conserved_out") == (12, 3) and m.extent("forces") == (783, 3)
    n = wx.Block(rep.guards, "alignn_neb_args", device="cpu", table=sx.STRUCTS).set(n_active=2, B=3, N=1082, n_ends=263, n_images=70,
                                                                                   force_rows=772, n_energies=2)
    assert n.extent("forces_out") == (2316, 3) and n.extent("energies_out") == (70, 1) and n.extent("end_energy") == (6, 2)
    assert n.extent("initial") == (789, 3) and n.extent("imax") == (2, 1)
    i = wx.Block(rep.guards, "alignn_idpp_args", device="cpu", table=sx.STRUCTS).set(n_active=2, B=3, N=441, n_ends=71, force_rows=131,
                                                                                    n_energies=3)
    assert i.extent("row_energy") == (131, 1) and i.extent("forces") == (393, 3) and i.extent("energy") == (3, 1)
    z = sx.Call(rep.guards, "alignn_zsl_match", device="cpu").set(n_pairs=3, max_film=5, max_subs=7, film_rows=40, subs_rows=60, n_hnf=54077)
    assert z.extent("subs_tab") == (1440, 4) and z.extent("best_tag") == (15, 5) and z.extent("prefix") == (258, 1)
    e = sx.Call(rep.guards, "alignn_phonon_eigh", device="cpu").set(n_structures=2, n_q=3, sum_m=12, sum_mm=90, n_points=9, dyn_total=99)
    assert e.extent("modes") == (540, 2) and e.extent("freqs") == (36, 1) and e.extent("lattice_points") == (27, 3)
    t = sx.Call(rep.guards, "alignn_phonon_thermal", device="cpu").set(n_structures=2, n_temps=5, workspace_bytes=640, n_freqs=66)
    assert t.extent("workspace") == (640, 1) and t.extent("entropy") == (10, 5)
    k = sx.Call(rep.guards, "alignn_traj_fit", device="cpu").set(n_rows=7, max_lag=4)
    assert k.extent("msd") == (105, 3) and k.extent("out") == (112, 4)


def test_a_flat_call_passes_its_arguments_in_the_prototype_order():
    rep = gp.Report("flat call")
    c = sx.Call(rep.guards, "alignn_traj_green_kubo", device="cpu").set(n_rows=2, max_lag=3, dtau=0.5, time_unit=2.0)
    c.alloc(dict(vacf=torch.ones(2, 4, dtype=torch.float64)))
    assert c.payload["out"].shape == (2, 4) and wx.pattern_left(c.payload["out"]) == 8 and bool(sx.is_pattern(c.payload["out"]).all())
    seen = []
    lib = type("Lib", (), {"alignn_traj_green_kubo": staticmethod(lambda *a: seen.append(a) or 0)})
    c.launch(lib, stream=7)
    assert seen == [(c.payload["vacf"].data_ptr(), 2, 3, 0.5, 2.0, c.payload["out"].data_ptr(), 7)]
    assert rep.guards.launches == {"alignn_traj_green_kubo": [1, 2]}
    plain = sx.plain_copy(c)
    sx.plain_launch(c, lib, plain, stream=7)
    assert seen[1] == (plain["vacf"].data_ptr(), 2, 3, 0.5, 2.0, plain["out"].data_ptr(), 7) and seen[1][0] != seen[0][0]
    with pytest.raises(AssertionError, match="an input of"):
        sx.Call(rep.guards, "alignn_traj_vdos", device="cpu").set(n_rows=1, max_lag=0, n_freq=2).alloc()


def _stepped(arrays, skip=(), stray=()):
    """what a FIRE launch that steps structure 1 (rows 1 and 2 of 3) of a batch of two writes, done by hand on ``arrays``"""
    for k, v in (("forces_out", 5.0), ("frac", 0.25), ("positions", 3.0), ("velocities", 0.5)):
        arrays[k][1:] = v
    for k, v in (("energy_out", -1.0), ("fmax_out", 2.0), ("state", 0.2)):
        arrays[k][1] = v
    arrays["istate"][1] = 1
    arrays["status"][:] = torch.tensor([1, 0], dtype=torch.int32)
    for k, at in skip:
        sx.bits(arrays[k]).view(-1)[at] = gp._PATTERN[torch.float64][1]
    for k, at, v in stray:
        arrays[k].view(-1)[at] = v


@pytest.mark.parametrize("finding,message", [
    (None, None), ("unwritten", "forces_out of alignn_fire_args: 1 elements the header calls written still hold the pattern"),
    ("stray", "energy_out of alignn_fire_args: 0 elements hold the pattern, the header leaves 1 alone"),
    ("state", "positions of alignn_fire_args: an element the header leaves alone was rewritten"),
    ("input", "forces of alignn_fire_args: an input was changed"),
    ("bits", "fmax_out of alignn_fire_args: differs from the same launch on plain allocations"),
    ("unnamed", "velocities of alignn_fire_args: which elements are written"), ("unknown", "no such array")])
def test_verify_reports_each_kind_of_finding(finding, message):
    """``step_extents.verify`` on a launch done by hand: as the header describes it, and with one planted departure of each kind -
    a written element left out, an untouched element of an output written, a state row of another structure rewritten (on both
    sides: it equals the plain launch's), an input changed, a differing bit, an array whose written elements the case does not
    name"""
    rep = gp.Report("verify")
    b = wx.Block(rep.guards, "alignn_fire_args", device="cpu", case="verify", table=sx.STRUCTS).set(B=2, N=3, n_active=1, force_rows=2)
    z = lambda *s: torch.zeros(*s, dtype=torch.float64)  # noqa: E731
    i32 = lambda x: torch.tensor(x, dtype=torch.int32)  # noqa: E731
    off = ("stress", "lattice0", "xa", "xc", "cell_velocities", "defgrad", "lattice", "stress_out", "cell_mask", "scalar_pressure",
           "enthalpy_out", "fixed")
    b.alloc("alignn_fire_step", dict(forces=z(2, 3) + 1, energy=z(1), force_ptr=i32([0, 2]), active=i32([1]), atom_ptr=i32([0, 1, 3]),
                                     inv_lattice=torch.eye(3, dtype=torch.float64).repeat(2, 1, 1), positions=z(3, 3) + 2, velocities=z(3, 3),
                                     state=z(2, 2) + 0.1, istate=i32([[0, 0], [0, 0]])), off)
    before, plain = sx.plain_copy(b), sx.plain_copy(b)
    rows = torch.tensor([False] * 3 + [True] * 6)
    one = lambda w: torch.tensor([False] * w + [True] * w)  # noqa: E731
    written = dict(forces_out=rows, frac=rows, positions=rows, velocities=rows, energy_out=one(1), fmax_out=one(1), state=one(2), istate=one(2))
    planted = dict(unwritten=dict(skip=[("forces_out", 4)]), stray=dict(stray=[("energy_out", 0, 0.0)]), state=dict(stray=[("positions", 1, 9.0)]))
    for arrays in (b.payload, plain):
        _stepped(arrays, **planted.get(finding, {}))
    if finding == "input":
        b.payload["forces"][0, 0] = 7.0
    if finding == "bits":
        b.payload["fmax_out"][1] = 2.0000000000000004
    if finding == "unnamed":
        del written["velocities"]
    if finding == "unknown":
        written["stress_out"] = True
    if finding is None:
        sx.verify(b, plain, written, before)
        assert rep.guards.check() == []
        return
    with pytest.raises(AssertionError, match=re.escape(message)):
        sx.verify(b, plain, written, before)


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
