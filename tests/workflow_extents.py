"""The extents of every array the struct-argument workflow entry points take, as the six headers state them - alignn_sym.h,
alignn_cells.h, alignn_phsym.h, alignn_local.h, alignn_order.h, alignn_traj.h - and the helper that puts each of them between the
guard bands of tests/gate_parity.py (``Block``, ``block``).  tests/test_workflow_extents.py checks the table against the headers
without a GPU; tests/test_gpu_workflow_extents.py hands the guarded buffers to the launches.

``TABLE``: argument struct -> its header, the entry points that take it, and per pointer field (dtype, element count, row
length, one role per entry point).  A count is an expression over the struct's scalar fields, the header's ``#define``s and the
struct's ``let`` abbreviations of those; a dict (entry point -> expression) where the entry points differ.  The few extents the
headers state through the contents of an index table rather than a scalar field are the struct's ``derived`` names, each with
the header's own words for it; the caller passes their values.  The row length (the last dimension) sets the guard width.

Roles.  ``in``: read only.  ``out``: this launch writes every element (of a call that sets no status bit: what a structure or
a frame with a status bit leaves unwritten is said in the headers).  ``add``: the caller zeroes the array and the launch adds or
ORs into it, or rewrites part of it from the rest.  ``scratch``: written by one launch of a pair and read by the next, and only
where the second reads it.  ``unused``: not looked at by this entry point.  The table only restates the header comments.

Payloads before a launch: ``in`` arrays are copies of the caller's tensors, ``add`` arrays hold zeros, ``out`` and ``scratch``
arrays hold the guard pattern (a NaN with a payload; for integers ``gate_parity.INT_PATTERN``, which no count, index or flag can
be), so that an element of an ``out`` array that still holds the pattern after the launch was never written.

``Block`` also takes another table of the same form (``table=``): tests/step_extents.py holds the argument blocks of the step
kernels and the flat prototypes, with a further role ``state`` (read and rewritten; allocated like an input).  A dtype that torch
cannot fill (uint64) is held as the signed integer of the same width (``STORAGE``).

Blind spots, those of the instrument: an access farther from an array than its guard (1024 elements or two rows) lands in
another buffer or outside the registry, and a value that is fetched from beside an array but never used changes nothing."""

import ast
import ctypes as C
import functools

import torch

from alignn_amd import _abi
from tests import gate_parity as gp

F64, I32, I64, U8 = torch.float64, torch.int32, torch.int64, torch.uint8
ROLES = ("in", "out", "add", "scratch", "unused")
STORAGE = {torch.uint64: torch.int64}  # what a buffer of a dtype torch cannot fill holds instead: the same width, signed
TRAJ = "3 * n_total_frames * n_atoms"
CELLS = "9 * B * (n_total_frames if lattice_per_frame else 1)"


def _f(dtype, count, row, *roles):
    return dict(dtype=dtype, count=count, row=row, roles=roles)


def _same(dtype, count, row, n, role):
    return _f(dtype, count, row, *([role] * n))


TABLE = {
    "alignn_sym_find_args": dict(
        header="alignn_sym.h", entries=("alignn_sym_search", "alignn_sym_fill"), let=dict(B="n_structs", N="n_atoms"), derived={},
        fields=dict(
            lattice=_same(F64, "9 * B", 3, 2, "in"), pos=_same(F64, "3 * N", 3, 2, "in"), atom_ptr=_same(I32, "B + 1", 1, 2, "in"),
            order=_same(I32, "N", 1, 2, "in"), seg_lo=_same(I32, "N", 1, 2, "in"), seg_hi=_same(I32, "N", 1, 2, "in"),
            pivot_lo=_same(I32, "B", 1, 2, "in"), pivot_hi=_same(I32, "B", 1, 2, "in"),
            frac=_same(F64, "3 * N", 3, 2, "scratch"),
            lattice_ops=_same(I32, "B * ALIGNN_SYM_MAX_LATTICE_OPS * 9", 9, 2, "scratch"),
            accepted=_same(U8, "ALIGNN_SYM_MAX_LATTICE_OPS * N", 1, 2, "scratch"),
            op_count=_same(I32, "B * ALIGNN_SYM_MAX_LATTICE_OPS", 48, 2, "scratch"),
            info=_f(I32, "B * ALIGNN_SYM_INFO", 8, "out", "in"),
            op_ptr=_f(I64, "B + 1", 1, "unused", "in"), map_ptr=_f(I64, "B + 1", 1, "unused", "in"),
            rotations=_f(I32, "9 * n_ops_total", 3, "unused", "out"), translations=_f(F64, "3 * n_ops_total", 3, "unused", "out"),
            atom_map=_f(I32, "n_map_total", 1, "unused", "out"), shifts=_f(I32, "3 * n_map_total", 3, "unused", "out"),
            orbits=_f(I32, "N", 1, "unused", "out"))),
    "alignn_sym_apply_args": dict(
        header="alignn_sym.h", entries=("alignn_sym_forces", "alignn_sym_stress", "alignn_sym_positions"),
        let=dict(B="n_structs", N="n_atoms"), derived={},
        fields=dict(
            lattice=_same(F64, "9 * B", 3, 3, "in"),
            in_=_same(F64, dict(alignn_sym_forces="3 * N", alignn_sym_stress="9 * B", alignn_sym_positions="3 * N"), 3, 3, "in"),
            out=_same(F64, dict(alignn_sym_forces="3 * N", alignn_sym_stress="9 * B", alignn_sym_positions="3 * N"), 3, 3, "out"),
            atom_ptr=_f(I32, "B + 1", 1, "in", "unused", "in"), op_ptr=_same(I64, "B + 1", 1, 3, "in"),
            map_ptr=_same(I64, "B + 1", 1, 3, "in"), rotations=_same(I32, "9 * n_ops_total", 3, 3, "in"),
            translations=_f(F64, "3 * n_ops_total", 3, "unused", "unused", "in"),
            atom_map=_f(I32, "n_map_total", 1, "in", "unused", "in"), shifts=_f(I32, "3 * n_map_total", 3, "unused", "unused", "in"))),
    "alignn_cells_args": dict(
        header="alignn_cells.h", entries=("alignn_cells_reduce", "alignn_cells_fill"), let=dict(B="n_structs", N="n_atoms"), derived={},
        fields=dict(
            lattice=_same(F64, "9 * B", 3, 2, "in"), pos=_same(F64, "3 * N", 3, 2, "in"), atom_ptr=_same(I32, "B + 1", 1, 2, "in"),
            op_ptr=_f(I64, "B + 1", 1, "in", "unused"), map_ptr=_f(I64, "B + 1", 1, "in", "unused"),
            rotations=_f(I32, "9 * n_ops_total", 3, "in", "unused"), translations=_f(F64, "3 * n_ops_total", 3, "in", "unused"),
            atom_map=_f(I32, "n_map_total", 1, "in", "unused"),
            info=_f(I32, "B * ALIGNN_CELLS_INFO", 8, "out", "in"), transform_num=_f(I64, "9 * B", 3, "out", "unused"),
            transform_den=_f(I64, "B", 1, "out", "unused"), cells=_f(F64, "9 * B", 3, "out", "in"),
            points=_f(I64, "12 * B", 3, "out", "in"), reps=_same(I32, "N", 1, 2, "scratch"),
            out_ptr=_f(I64, "B + 1", 1, "unused", "in"), out_pos=_f(F64, "3 * n_out_total", 3, "unused", "out"),
            source_atom=_f(I32, "n_out_total", 1, "unused", "out"))),
    "alignn_phsym_plan_args": dict(
        header="alignn_phsym.h", entries=("alignn_phsym_plan",), let=dict(B="n_structs", N="n_atoms", G="n_ops_total"), derived={},
        fields=dict(
            lattice=_f(F64, "9 * B", 3, "in"), supercell=_f(I32, "3 * B", 3, "in"), atom_ptr=_f(I32, "B + 1", 1, "in"),
            op_ptr=_f(I64, "B + 1", 1, "in"), map_ptr=_f(I64, "B + 1", 1, "in"), rotations=_f(I32, "9 * G", 3, "in"),
            atom_map=_f(I32, "n_map_total", 1, "in"), usable=_f(I32, "G", 1, "out"), rot=_f(F64, "9 * G", 3, "out"),
            rep=_f(I32, "N", 1, "out"), n_site=_f(I32, "N", 1, "out"), site_ops=_f(I32, "N * ALIGNN_PHSYM_MAX_SITE_OPS", 48, "out"),
            n_dir=_f(I32, "N", 1, "out"), dirs=_f(F64, "9 * N", 3, "out"), minv=_f(F64, "9 * N", 3, "out"),
            dist_op=_f(I32, "N", 1, "out"))),
    "alignn_phsym_displace_args": dict(
        header="alignn_phsym.h", entries=("alignn_phsym_displace",), let=dict(B="n_structs"),
        derived=dict(N="atom_ptr[B]", rows="the sum over the jobs of their supercell atoms n_sc"),
        fields=dict(
            positions=_f(F64, "3 * N", 3, "in"), atom_ptr=_f(I32, "B + 1", 1, "in"), lattice=_f(F64, "9 * B", 3, "in"),
            inv_supercell=_f(F64, "9 * B", 3, "in"), supercell=_f(I32, "3 * B", 3, "in"), dirs=_f(F64, "9 * N", 3, "in"),
            jobs=_f(I32, "4 * n_jobs", 4, "in"), row_off=_f(I64, "n_jobs", 1, "in"), frac=_f(F64, "3 * rows", 3, "out"),
            cart=_f(F64, "3 * rows", 3, "out"))),
    "alignn_phsym_rows_args": dict(
        header="alignn_phsym.h", entries=("alignn_phsym_rows",), let=dict(B="n_structs"),
        derived=dict(force_rows="the rows of the chunk's supercells: twice the sum over the pairs of n_sc",
                     n_g_rows="the rows of g: the sum over every direction of every representative of n_sc"),
        fields=dict(
            forces=_f(F64, "3 * force_rows", 3, "in"), pairs=_f(I32, "2 * n_pairs", 2, "in"), pair_rows=_f(I64, "n_pairs", 1, "in"),
            out_rows=_f(I64, "n_pairs", 1, "in"), atom_ptr=_f(I32, "B + 1", 1, "in"), supercell=_f(I32, "3 * B", 3, "in"),
            g=_f(F64, "3 * n_g_rows", 3, "out"))),
    "alignn_phsym_fc_args": dict(
        header="alignn_phsym.h", entries=("alignn_phsym_solve", "alignn_phsym_distribute"), let=dict(B="n_structs", G="n_ops_total"),
        derived=dict(N="atom_ptr[B]", n_g_rows="the rows of g: the sum over every direction of every representative of n_sc",
                     fc_total="the sum over the structures of (N0 N1 N2) (3 n_b)^2"),
        fields=dict(
            items=_same(I32, "2 * n_items", 2, 2, "in"), g_rows=_f(I64, "n_items", 1, "in", "unused"),
            g=_f(F64, "3 * n_g_rows", 3, "in", "unused"), fc=_same(F64, "fc_total", 1, 2, "scratch"), fc_off=_same(I64, "B", 1, 2, "in"),
            atom_ptr=_same(I32, "B + 1", 1, 2, "in"), supercell=_same(I32, "3 * B", 3, 2, "in"), op_ptr=_same(I64, "B + 1", 1, 2, "in"),
            map_ptr=_same(I64, "B + 1", 1, 2, "in"), rotations=_same(I32, "9 * G", 3, 2, "in"),
            atom_map=_same(I32, "n_map_total", 1, 2, "in"), shifts=_same(I32, "3 * n_map_total", 3, 2, "in"),
            rot=_same(F64, "9 * G", 3, 2, "in"), rep=_f(I32, "N", 1, "unused", "in"), n_site=_f(I32, "N", 1, "in", "unused"),
            site_ops=_f(I32, "N * ALIGNN_PHSYM_MAX_SITE_OPS", 48, "in", "unused"), n_dir=_f(I32, "N", 1, "in", "unused"),
            dirs=_f(F64, "9 * N", 3, "in", "unused"), minv=_f(F64, "9 * N", 3, "in", "unused"),
            dist_op=_f(I32, "N", 1, "unused", "in"))),
    "alignn_local_cna_args": dict(
        header="alignn_local.h", entries=("alignn_local_cna", "alignn_local_cna_counts"),
        let=dict(B="n_structs", N="n_atoms", S="n_species", F="n_frames"), derived={},
        fields=dict(
            traj=_f(F64, TRAJ, 3, "in", "unused"), lattice=_f(F64, CELLS, 3, "in", "unused"), atom_ptr=_same(I32, "B + 1", 1, 2, "in"),
            group=_same(I32, "N", 1, 2, "in"), group_count=_same(I32, "B * (S + 1)", "S + 1", 2, "in"),
            r_cut=_f(F64, "B", 1, "in", "unused"), structure=_f(I32, "F * N", "N", "out", "in"),
            signature_counts=_f(I32, "F * N * ALIGNN_LOCAL_SIGNATURES", 5, "out", "unused"),
            n_neighbors=_f(I32, "F * N", "N", "out", "unused"),
            counts=_f(I64, "B * (S + 1) * F * ALIGNN_LOCAL_CLASSES", 5, "unused", "out"),
            fraction=_f(F64, "B * (S + 1) * F * ALIGNN_LOCAL_CLASSES", 5, "unused", "out"), status=_f(I32, "1", 1, "add", "unused"))),
    "alignn_local_bond_args": dict(
        header="alignn_local.h", entries=("alignn_local_bond_qlm", "alignn_local_bond_finish"),
        let=dict(B="n_structs", N="n_atoms", S="n_species", F="n_frames", L="n_ls"), derived={},
        fields=dict(
            traj=_same(F64, TRAJ, 3, 2, "in"), lattice=_same(F64, CELLS, 3, 2, "in"), atom_ptr=_same(I32, "B + 1", 1, 2, "in"),
            group=_same(I32, "N", 1, 2, "in"), group_count=_same(I32, "B * (S + 1)", "S + 1", 2, "in"),
            r_cut=_same(F64, "B", 1, 2, "in"),
            ynorm=_f(F64, "(ALIGNN_LOCAL_MAX_L + 1) * ALIGNN_LOCAL_M_STRIDE", 13, "in", "unused"),
            w3j=_f(F64, "L * ALIGNN_LOCAL_W3J_STRIDE", 625, "unused", "in"),
            qlm=_same(F64, "chunk_frames * N * L * ALIGNN_LOCAL_M_STRIDE * 2", 2, 2, "scratch"),
            s=_f(F64, "F * N * L", "L", "unused", "out"), t=_f(F64, "F * N * L", "L", "unused", "out"),
            q=_f(F64, "F * N * L", "L", "unused", "out"), w=_f(F64, "F * N * L", "L", "unused", "out"),
            s_avg=_f(F64, "F * N * L", "L", "unused", "out"), t_avg=_f(F64, "F * N * L", "L", "unused", "out"),
            q_avg=_f(F64, "F * N * L", "L", "unused", "out"), w_avg=_f(F64, "F * N * L", "L", "unused", "out"),
            n_neighbors=_f(I32, "F * N", "N", "out", "unused"), status=_f(I32, "1", 1, "add", "unused"))),
    "alignn_order_angle_args": dict(
        header="alignn_order.h", entries=("alignn_order_angles", "alignn_order_adf_finish", "alignn_order_steinhardt_mean"),
        let=dict(B="n_structs", N="n_atoms", S="n_species", F="n_frames", L="n_ls", P="1 + n_species * (n_species + 1) // 2"),
        derived={},
        fields=dict(
            traj=_f(F64, TRAJ, 3, "in", "unused", "unused"), lattice=_f(F64, CELLS, 3, "in", "unused", "unused"),
            atom_ptr=_f(I32, "B + 1", 1, "in", "unused", "in"), group=_f(I32, "N", 1, "in", "unused", "in"),
            group_count=_f(I32, "B * (S + 1)", "S + 1", "in", "unused", "in"), r_cut=_f(F64, "B", 1, "in", "unused", "unused"),
            counts=_f(I64, "B * (S + 1) * P * n_bins", "n_bins", "add", "add", "unused"),
            adf=_f(F64, "B * (S + 1) * P * n_bins", "n_bins", "unused", "out", "unused"),
            theta=_f(F64, "n_bins", 1, "unused", "out", "unused"), q=_f(F64, "F * N * L", "L", "out", "unused", "in"),
            n_neighbors=_f(I32, "F * N", "N", "out", "unused", "unused"),
            mean=_f(F64, "B * (S + 1) * F * L", "L", "unused", "unused", "out"), status=_f(I32, "1", 1, "add", "unused", "unused"))),
    "alignn_order_sq_args": dict(
        header="alignn_order.h", entries=("alignn_order_sq_vectors", "alignn_order_sq_accumulate", "alignn_order_sq_bin"),
        let=dict(B="n_structs", N="n_atoms", S="n_species", V="n_vectors", P="1 + n_species * (n_species + 1) // 2",
                 n_chunks="-(-n_frames // ALIGNN_ORDER_SQ_FRAME_CHUNK)"), derived={},
        fields=dict(
            traj=_f(F64, "3 * n_total_frames * N", 3, "unused", "in", "unused"), lattice=_f(F64, "9 * B", 3, "in", "in", "unused"),
            atom_ptr=_f(I32, "B + 1", 1, "unused", "in", "unused"), group=_f(I32, "N", 1, "unused", "in", "unused"),
            group_count=_f(I32, "B * (S + 1)", "S + 1", "unused", "unused", "in"), vec_ptr=_same(I32, "B + 1", 1, 3, "in"),
            n_vec=_f(I32, "B", 1, "out", "unused", "unused"), hkl=_f(I32, "3 * V", 3, "out", "in", "unused"),
            qnorm=_f(F64, "V", 1, "out", "unused", "unused"), vbin=_f(I32, "V", 1, "out", "unused", "in"),
            partial=_f(F64, "n_chunks * P * V", "V", "unused", "out", "in"), s_vec=_f(F64, "P * V", "V", "unused", "unused", "out"),
            s=_f(F64, "B * P * n_bins", "n_bins", "unused", "unused", "out"),
            n_vectors_bin=_f(I64, "B * n_bins", "n_bins", "unused", "unused", "out"),
            centres=_f(F64, "n_bins", 1, "unused", "unused", "out"), status=_f(I32, "1", 1, "add", "unused", "unused"))),
    "alignn_traj_rdf_args": dict(
        header="alignn_traj.h", entries=("alignn_traj_rdf_counts", "alignn_traj_rdf_normalise"),
        let=dict(B="n_structs", N="n_atoms", S="n_species", P="1 + n_species * (n_species + 1) // 2"), derived={},
        fields=dict(
            traj=_f(F64, TRAJ, 3, "in", "unused"), lattice=_same(F64, CELLS, 3, 2, "in"), atom_ptr=_f(I32, "B + 1", 1, "in", "unused"),
            group=_f(I32, "N", 1, "in", "unused"), group_count=_same(I32, "B * (S + 1)", "S + 1", 2, "in"),
            counts=_f(I64, "B * P * n_bins", "n_bins", "add", "in"), g=_f(F64, "B * P * n_bins", "n_bins", "unused", "out"),
            coord=_f(F64, "B * P * n_bins", "n_bins", "unused", "out"), volume=_f(F64, "B", 1, "unused", "out"),
            centres=_f(F64, "n_bins", 1, "unused", "out"), status=_f(I32, "1", 1, "add", "unused"))),
    "alignn_traj_corr_args": dict(
        header="alignn_traj.h", entries=("alignn_traj_com", "alignn_traj_corr"),
        let=dict(B="n_structs", N="n_atoms", S="n_species"), derived={},
        fields=dict(
            traj=_same(F64, "3 * n_total_frames * N", 3, 2, "in"), masses=_same(F64, "N", 1, 2, "in"),
            atom_ptr=_same(I32, "B + 1", 1, 2, "in"), group=_f(I32, "N", 1, "unused", "in"),
            group_count=_f(I32, "B * (S + 1)", "S + 1", "unused", "in"), com=_f(F64, "3 * n_frames * B", 3, "out", "in"),
            out=_f(F64, "B * (S + 1) * (max_lag + 1) * (3 if mode == 0 else 1)", "3 if mode == 0 else 1", "unused", "out"))),
}


def entry_points():
    """entry point -> the struct it takes"""
    return {e: s for s, t in TABLE.items() for e in t["entries"]}


@functools.lru_cache(maxsize=None)
def read_header(name):
    """``_abi.header``; for alignn_hip.h, whose blocks come with ``S_sizeof`` queries that ``_lib.load`` checks, the same record"""
    if name == "alignn_hip.h":
        with open(_abi.HEADER) as f:
            return _abi.Header(_abi.HEADER, _abi.STRUCTS, _abi.SIGNATURES, _abi.defines(f.read()))
    return _abi.header(name)


def header_of(struct, table=None):
    return read_header((table or TABLE)[struct]["header"])


def _names(expr):
    return {n.id for n in ast.walk(ast.parse(str(expr), mode="eval")) if isinstance(n, ast.Name)}


def names_used(struct, expr, table=None):
    """the names a count or row expression rests on, its struct's ``let`` abbreviations resolved"""
    let, out, todo = (table or TABLE)[struct]["let"], set(), _names(expr)
    while todo:
        n = todo.pop()
        if n in let:
            todo |= _names(let[n])
        else:
            out.add(n)
    return out


def count_of(struct, field, entry=None, table=None):
    c = (table or TABLE)[struct]["fields"][field]["count"]
    return c[entry] if isinstance(c, dict) else c


def evaluate(struct, expr, values, table=None):
    """``expr`` with the scalars ``values`` (fields and derived names), the header's defines and the struct's abbreviations"""
    env = dict(header_of(struct, table).defines)
    env.update(values)
    for k, v in (table or TABLE)[struct]["let"].items():
        env[k] = eval(v, {"__builtins__": {}}, env)  # noqa: S307 (the table's own text)
    return int(eval(str(expr), {"__builtins__": {}}, env))  # noqa: S307


def pattern_left(t):
    """how many elements of ``t`` still hold the guard pattern"""
    if t.dtype in gp._PATTERN:
        view, pat = gp._PATTERN[t.dtype]
        return int((t.view(view) == pat).sum())
    return int((t == gp.INT_PATTERN[t.dtype]).sum())


class Block:
    """One argument block whose every non-NULL pointer lies in a guarded buffer of exactly the tabled extent.  ``set`` the scalars,
    ``alloc`` the arrays of an entry point (``inputs``: field -> the tensor to copy in; the other arrays by role), ``launch`` it,
    ``unwritten`` lists the ``out`` arrays that still hold a pattern element.  The struct's field names name the buffers.
    ``table``: another table of the same form (tests/step_extents.py), whose further role ``state`` - an array the launch reads and
    rewrites - is allocated like an input: guarded, with the caller's tensor copied in."""

    def __init__(self, guards, struct, device=gp.DEV, case="", table=None):
        self.guards, self.struct, self.device, self.case = guards, struct, device, case
        self.tables = table or TABLE
        self.table = self.tables[struct]
        self.args = header_of(struct, self.tables).structs[struct]()
        self.payload, self.derived = {}, {}

    def set(self, **scalars):
        for k, v in scalars.items():
            if k in self.table["derived"]:
                self.derived[k] = int(v)
            else:
                assert k in {f[0] for f in self.args._fields_}, f"{self.struct} has no field {k}"
                setattr(self.args, k, v)
        return self

    def values(self):
        kinds = (C.c_void_p,)
        out = {n: getattr(self.args, n) for n, t in self.args._fields_ if t not in kinds}
        out.update(self.derived)
        return out

    def extent(self, field, entry=None):
        spec = self.table["fields"][field]
        n = evaluate(self.struct, count_of(self.struct, field, entry, self.tables), self.values(), self.tables)
        return n, max(1, evaluate(self.struct, spec["row"], self.values(), self.tables))

    def role(self, field, entry):
        return self.table["fields"][field]["roles"][self.table["entries"].index(entry)]

    def alloc(self, entry, inputs=None, null=()):
        """Every array ``entry`` uses that the block does not hold yet.  An extent of zero, or a name in ``null``, stays NULL."""
        inputs = dict(inputs or {})
        for field, spec in self.table["fields"].items():
            if field in self.payload or field in null or self.role(field, entry) == "unused":
                continue
            n, row = self.extent(field, entry)
            dtype = STORAGE.get(spec["dtype"], spec["dtype"])
            pat = gp.INT_PATTERN.get(dtype)
            if n == 0:
                self.payload[field] = None
                assert field not in inputs or inputs.pop(field).numel() == 0
                continue
            shape = (n // row, row) if row > 1 and n % row == 0 else (n,)
            name = f"{field} of {self.struct}"
            if field in inputs:
                src = inputs.pop(field)
                assert src.dtype == dtype and src.numel() == n, (
                    f"{name}: the caller's tensor is {src.dtype} x {src.numel()}, the header says {dtype} x {n}")
                t = self.guards.guarded(shape, dtype, None, name, self.device, row, pat)
                t.copy_(src.reshape(shape))
            else:
                assert self.role(field, entry) not in ("in", "state"), f"{name}: an input of {entry} without a tensor"
                fill = 0 if "add" in spec["roles"] else None
                t = self.guards.guarded(shape, dtype, fill, name, self.device, row, pat)
            self.payload[field] = t
            setattr(self.args, field, t.data_ptr())
        assert not inputs, f"{sorted(inputs)}: no array of {entry} that is still to be allocated"
        return self

    def adopt(self, other, *fields):
        """takes over arrays of another block of the same registry (one buffer handed to two argument blocks, as ``fc``)"""
        for field in fields:
            t = other.payload[field]
            assert t is not None and t.numel() == self.extent(field, self.table["entries"][0])[0], field
            self.payload[field] = t
            setattr(self.args, field, t.data_ptr())
        return self

    def launch(self, lib, entry, stream=None):
        """hands every array ``entry`` uses through ``Guards.gptr``, calls it, and checks every guard of the registry"""
        for field, t in self.payload.items():
            if t is not None and self.role(field, entry) != "unused":
                assert self.guards.gptr(t) == getattr(self.args, field)
        self.guards.launched(entry)
        rc = getattr(lib, entry)(C.byref(self.args), stream)
        assert rc == 0, f"{self.case}: {entry} returned {rc}"
        found = self.guards.check()
        assert not found, f"{self.case}: after {entry}: " + "; ".join(f[4] for f in found)
        return self

    def unwritten(self, entry):
        """[(field, elements that still hold the pattern)] over the ``out`` arrays of ``entry``"""
        out = []
        for field, t in self.payload.items():
            if t is not None and self.role(field, entry) == "out":
                left = pattern_left(t)
                if left:
                    out.append((field, left))
        return out

    def written(self, entry):
        left = self.unwritten(entry)
        assert not left, f"{self.case}: {entry} left elements unwritten: {left}"
        return self


def block(guards, struct, scalars, inputs, entry=None, null=(), device=gp.DEV):
    """-> (the filled argument block, field -> payload tensor): the arrays of ``entry`` (default: the struct's first entry point)"""
    b = Block(guards, struct, device).set(**scalars)
    b.alloc(entry or TABLE[struct]["entries"][0], inputs, null)
    return b.args, b.payload
