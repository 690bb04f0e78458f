"""The struct-argument workflow launches - symmetry search and symmetrisers, primitive and conventional cells, symmetry-reduced
phonons, common-neighbour analysis and bond order, angle and S(q) analyses, RDF and time correlations - each between the guard
bands of tests/gate_parity.py, every buffer of exactly the extent its header states (tests/workflow_extents.py).  The argument
blocks are filled here, in the sequence the drivers use, the host read-backs included.  Asserted per case, in this order:
(a) no guard bit changed after any launch; (b) no array the header calls written holds a pattern element; (c) every output equals,
bit for bit, what the driver returns for the same inputs on its own plain allocations - the headers promise that a structure's
bits depend on its own data alone, and the drivers are tied to the numpy restatements by their own test modules; (d) where a
driver exposes its packed arrays, their ``numel()`` is the tabled extent.

Blind spots (those of the instrument): an access farther from a buffer than its guard - 1024 elements or two rows - and a read
beside a buffer whose value is never used."""

import sys

import numpy as np
import pytest
import torch

from alignn_amd import (_lib, adf, bond_order, cna, conventional_cell, find_symmetry, msd, phonons, primitive_cell, rdf, steinhardt,
                        structure_factor, symmetrize_forces, symmetrize_positions, symmetrize_stress, vacf)
from alignn_amd import _trajectory_inputs as TI
from tests import cells_ref, local_ref, order_ref, sym_ref
from tests import gate_parity as gp
from tests import workflow_extents as wx

pytestmark = pytest.mark.gpu
DEV = "cuda"
F64, I32, I64 = torch.float64, torch.int32, torch.int64
SYM, CELLS, PH, LOCAL, ORDER, TRAJ = (sys.modules["alignn_amd." + m] for m in
                                      ("symmetry", "cells", "phonons", "local_order", "order", "trajectory"))


def _t(x, dtype=F64):
    return torch.tensor(np.ascontiguousarray(x), dtype=dtype, device=DEV)


def _report(case):
    return gp.Report(case, tag="workflow-extents")


def _block(rep, struct):
    return wx.Block(rep.guards, struct, DEV, rep.case)


def _run(b, lib, entry, written=True):
    b.launch(lib, entry, _lib.stream())
    return b.written(entry) if written else b


def _result(fn, *a, **kw):
    """the driver's result; that of the other structures where one of them raises"""
    try:
        return fn(*a, **kw)
    except ValueError as e:
        if getattr(e, "result", None) is None:
            raise
        return e.result


def _eq(a, b):
    """the same bits in the same order (a guarded payload is [rows, row length], whatever shape the driver gives its array)"""
    return a.numel() == b.numel() and a.dtype == b.dtype and torch.equal(a.reshape(-1), b.reshape(-1))


# ======================================================================================================================
# symmetry
# ======================================================================================================================
def _ten():
    """the ten structures of tests/test_gpu_symmetry.py, in its order"""
    C = sym_ref.crystals()
    fcc, diamond = C["fcc"][:3], C["diamond"][:3]
    noise = lambda amp: diamond[1] + np.random.default_rng(0).uniform(-amp, amp, diamond[1].shape)
    return [C["simple_cubic"][:3], C["triclinic_inversion_pair"][:3], C["wurtzite"][:3], C["hcp"][:3],
            (sym_ref.rebased(fcc[0], [[1, 2, 0], [0, 1, 1], [0, 0, 1]]), fcc[1], fcc[2]),
            (fcc[0] @ np.diag([1.0, 1.0, 1.0 + 1e-5]), fcc[1], fcc[2]), (diamond[0], noise(1e-4), diamond[2]),
            (diamond[0], noise(1e-2), diamond[2]), C["fcc_2x2x2"][:3], sym_ref.supercell(*sym_ref.diamond_cube(), (3, 2, 2))]


def _far():
    fcc = sym_ref.crystals()["fcc"]
    far = (sym_ref.rebased(fcc[0], [[1, 2, 0], [0, 1, 3], [0, 0, 1]]), fcc[1], fcc[2])
    assert max(sym_ref.image_range(far[0], 1e-3)) > 8
    return far


def _one_species(sizes=(1, 17, 33, 65)):
    """random atoms of one species in a cubic cell: every atom is a candidate translation of each of the 48 lattice operations -
    1, 17, 33 and 65 of them: one chunk of 16 candidates, one above it, one above two, one above a wavefront"""
    rng = np.random.default_rng(5)
    out = []
    for n in sizes:
        a = 2.4 * n ** (1.0 / 3.0)
        out.append((a * np.eye(3), rng.uniform(0.0, 1.0, (n, 3)) * a, np.full(n, 14)))
    return out


def _sym_case(name):
    C = sym_ref.crystals()
    hcp, wurtzite, far = C["hcp"][:3], C["wurtzite"][:3], _far()
    if name == "ten":
        return _ten()
    if name == "table23":
        return [v[:3] for v in cells_ref.table().values()]
    if name == "sizes":
        return _one_species()
    if name == "sc_343":  # more candidates than a workgroup has threads: 22 chunks of candidates, all accepted
        return [sym_ref.supercell(3.0 * np.eye(3), np.zeros((1, 3)), np.array([7]), (7, 7, 7))]
    # a structure that gets no operations: empty segments of op_ptr and map_ptr at each place, NULL pointers when alone
    return {"far_first": [far, hcp, wurtzite], "far_middle": [hcp, far, wurtzite], "far_last": [hcp, wurtzite, far], "far_alone": [far]}[name]


def guarded_find(rep, lats, poss, zs, symprec=1e-3):
    """``find_symmetry``'s two entry points with the read-back of info in between -> (the block, info, op_ptr, map_ptr)"""
    lib = SYM._load()
    ns = [len(p) for p in poss]
    B, N = len(ns), sum(ns)
    order, lo, hi, plo, phi = SYM._sorting("guarded_find", ns, zs)
    ptr = np.concatenate([[0], np.cumsum(ns)])
    b = _block(rep, "alignn_sym_find_args").set(symprec=float(symprec), n_structs=B, n_atoms=N, max_atoms=max(ns))
    b.alloc("alignn_sym_search", dict(lattice=_t(np.stack(lats)), pos=_t(np.concatenate(poss)), atom_ptr=_t(ptr, I32), order=_t(order, I32),
                                      seg_lo=_t(lo, I32), seg_hi=_t(hi, I32), pivot_lo=_t(plo, I32), pivot_hi=_t(phi, I32)))
    _run(b, lib, "alignn_sym_search")
    info = b.payload["info"].cpu().numpy()
    n_ops = [int(v) for v in info[:, 0]]
    assert min(n_ops) >= 0 and max(n_ops) <= 48 * max(ns)  # (what sizes the second launch's buffers)
    op_ptr = np.concatenate([[0], np.cumsum(n_ops)]).astype(np.int64)
    map_ptr = np.concatenate([[0], np.cumsum([g * n for g, n in zip(n_ops, ns)])]).astype(np.int64)
    b.set(n_ops_total=int(op_ptr[-1]), n_map_total=int(map_ptr[-1]))
    b.alloc("alignn_sym_fill", dict(op_ptr=_t(op_ptr, I64), map_ptr=_t(map_ptr, I64)))
    _run(b, lib, "alignn_sym_fill")
    return b, info, op_ptr, map_ptr


def same_symmetry(b, info, op_ptr, map_ptr, res):
    """(c) and (d) against the driver's SymmetryResult"""
    pk, P = res.packed, b.payload
    assert res.n_ops == info[:, 0].tolist() and res.n_translations == info[:, 1].tolist()
    assert res.point_group_order == info[:, 2].tolist() and res.crystal_system == [SYM.CRYSTAL_SYSTEMS[v] for v in info[:, 3]]
    assert pk["op_ptr"].tolist() == op_ptr.tolist() and pk["map_ptr"].tolist() == map_ptr.tolist()
    assert (pk["n_ops_total"], pk["n_map_total"]) == (b.args.n_ops_total, b.args.n_map_total)
    for k in ("rotations", "translations", "atom_map", "shifts"):
        want = b.extent(k)[0]
        assert pk[k].numel() == want, (k, pk[k].numel(), want)  # (d)
        assert want == 0 and P[k] is None or torch.equal(P[k].reshape(-1), pk[k].reshape(-1)), k
    assert pk["atom_ptr"].numel() == b.extent("atom_ptr")[0] and pk["op_ptr"].numel() == b.extent("op_ptr")[0]
    assert torch.equal(P["orbits"], torch.cat(res.orbits))
    for g, (W, t) in enumerate(zip(res.rotations, res.translations)):
        lo, hi = int(op_ptr[g]), int(op_ptr[g + 1])
        assert W.shape == (hi - lo, 3, 3) and (hi == lo or torch.equal(P["rotations"].view(-1, 3, 3)[lo:hi], W))
        assert hi == lo or torch.equal(P["translations"][lo:hi], t)


def guarded_apply(rep, entry, b, lats, x):
    """one symmetriser on the operations the block ``b`` holds -> out"""
    P = b.payload
    a = _block(rep, "alignn_sym_apply_args").set(n_ops_total=b.args.n_ops_total, n_map_total=b.args.n_map_total,
                                                  n_structs=b.args.n_structs, n_atoms=b.args.n_atoms)
    inputs = dict(lattice=_t(np.stack(lats)), in_=x)
    for k in a.table["fields"]:
        if k not in ("lattice", "in_", "out") and a.role(k, entry) != "unused" and P[k] is not None:
            inputs[k] = P[k]
    a.alloc(entry, inputs)
    _run(a, SYM._load(), entry)
    return a.payload["out"]


@pytest.mark.parametrize("name", ["ten", "table23", "far_first", "far_middle", "far_last", "far_alone", "sizes", "sc_343"])
def test_symmetry_search_and_symmetrisers_between_guards(name):
    structures = _sym_case(name)
    lats, poss, zs = ([s[i] for s in structures] for i in range(3))
    rep = _report(f"symmetry {name}")
    b, info, op_ptr, map_ptr = guarded_find(rep, lats, poss, zs)
    res = _result(find_symmetry, lats, poss, zs, device=DEV)
    same_symmetry(b, info, op_ptr, map_ptr, res)
    if name.startswith("far"):
        bad = [i for i in range(len(structures)) if info[i, 4]]
        assert len(bad) == 1 and info[bad[0], 0] == 0 and info[bad[0], 4] == SYM.STATUS_IMAGES
    if name == "sizes":
        assert info[:, 5].tolist() == [48] * 4 and info[:, 4].tolist() == [0] * 4
    if name == "sc_343":
        assert info[0, :3].tolist() == [48 * 343, 343, 48]
    g = torch.Generator().manual_seed(2)
    N, B = b.args.n_atoms, b.args.n_structs
    forces, stress = torch.randn(N, 3, generator=g, dtype=F64).to(DEV), torch.randn(B, 3, 3, generator=g, dtype=F64).to(DEV)
    pos = _t(np.concatenate(poss))
    for entry, fn, x in (("alignn_sym_forces", symmetrize_forces, forces), ("alignn_sym_stress", symmetrize_stress, stress),
                         ("alignn_sym_positions", symmetrize_positions, pos)):
        got = guarded_apply(rep, entry, b, lats, x)
        assert _eq(got, fn(res, lats, x)), entry
    rep.finish()  # (prints the case's launches and guarded buffers, per entry point)


# ======================================================================================================================
# primitive and conventional cells
# ======================================================================================================================
def guarded_pass(rep, conventional, lat, pos, ns, pk, symprec):
    """``cells._pass``: _cells_reduce, the read-back of info, _cells_fill -> what ``cells._pass`` returns"""
    lib = CELLS._load()
    B, N = len(ns), sum(ns)
    b = _block(rep, "alignn_cells_args").set(symprec=float(symprec), n_ops_total=pk["n_ops_total"], n_map_total=pk["n_map_total"],
                                              n_structs=B, n_atoms=N, conventional=int(conventional))
    b.alloc("alignn_cells_reduce", dict(lattice=lat, pos=pos, **{k: pk[k] for k in ("atom_ptr", "op_ptr", "map_ptr", "rotations",
                                                                                   "translations", "atom_map")}))
    _run(b, lib, "alignn_cells_reduce")
    got = b.payload["info"].cpu().numpy()
    n_out = [int(v) for v in got[:, 0]]
    assert min(n_out) >= 0 and max(n_out) <= CELLS.MAX_ATOMS
    out_ptr = np.concatenate([[0], np.cumsum(n_out)]).astype(np.int64)
    b.set(n_out_total=int(out_ptr[-1]), max_out=max(n_out))
    b.alloc("alignn_cells_fill", dict(out_ptr=_t(out_ptr, I64)))
    _run(b, lib, "alignn_cells_fill")
    P = b.payload
    empty = lambda dtype, *shape: torch.empty(*shape, dtype=dtype, device=DEV)
    return dict(info=got, n_out=n_out, out_ptr=out_ptr, num=P["transform_num"].view(B, 3, 3), cells=P["cells"].view(B, 3, 3),
                pos=P["out_pos"] if P["out_pos"] is not None else empty(F64, 0, 3),
                source=P["source_atom"] if P["source_atom"] is not None else empty(I32, 0), block=b)


def same_pass(mine, theirs):
    assert np.array_equal(mine["info"], theirs["info"]) and mine["n_out"] == theirs["n_out"]
    for k in ("num", "cells", "pos", "source"):
        assert _eq(mine[k], theirs[k]), k
    b = mine["block"]
    assert theirs["pos"].numel() == b.extent("out_pos")[0] and theirs["source"].numel() == b.extent("source_atom")[0]  # (d)
    assert theirs["num"].numel() == b.extent("transform_num")[0] and theirs["cells"].numel() == b.extent("cells")[0]


@pytest.mark.parametrize("conventional", [False, True])
@pytest.mark.parametrize("name", ["table23", "ten", "far_first", "far_middle", "far_last", "far_alone", "sizes"])
def test_cells_between_guards(name, conventional):
    """Both passes of the driver: with ``conventional`` the supercells of the tables (fcc_2x2x2, bcc_cube, ortho_c, diamond_cube,
    diamond_96) come back as reduced primitive cells with info word 7 set, and the search and the two launches run again on those.
    The structure without operations leaves an empty segment of out_ptr at the start, in the middle and at the end of a batch."""
    structures = _sym_case(name)
    lats, poss, zs = ([s[i] for s in structures] for i in range(3))
    ns, symprec, dev = [len(p) for p in poss], 1e-3, torch.device(DEV, torch.cuda.current_device())
    rep = _report(f"cells {name} conventional={int(conventional)}")
    sym = _result(find_symmetry, lats, poss, zs, device=DEV)
    lat, pos = _t(np.stack(lats)), _t(np.concatenate(poss))
    one = guarded_pass(rep, conventional, lat, pos, ns, sym.packed, symprec)
    theirs = CELLS._pass(conventional, lat, poss, ns, sym, symprec)
    same_pass(one, theirs)
    B = len(ns)
    status = [int(v) for v in one["info"][:, 4]]
    cut = lambda x, ptr, b: x[ptr[b]:ptr[b + 1]]
    pos_of, src_of = [cut(one["pos"], one["out_ptr"], b) for b in range(B)], [cut(one["source"], one["out_ptr"], b) for b in range(B)]
    cells, num = one["cells"].clone(), one["num"].clone()
    # transform_den and points, which the driver never reads back: n_t (info word 5; 0 with a status), and the origin first
    den, points, info = one["block"].payload["transform_den"].tolist(), one["block"].payload["points"].view(B, 4, 3), one["info"].copy()
    assert den == one["info"][:, 5].tolist() and not bool(points[:, 0].any())
    assert all(bool(points[b, max(int(one["info"][b, 1]), 1):].eq(0).all()) for b in range(B))  # (no point beyond the multiplicity)
    again = [b for b in range(B) if one["info"][b, 7] and not status[b]]
    if name in ("table23", "ten"):
        assert bool(again) == conventional
    if again:
        idx = torch.tensor(again, dtype=I64, device=DEV)
        lats2, poss2 = [cells[b].cpu().numpy() for b in again], [pos_of[b].cpu().numpy() for b in again]
        zs2 = [np.asarray(zs[b])[src_of[b].cpu().numpy()] for b in again]
        b2, info2, op2, map2 = guarded_find(rep, lats2, poss2, zs2, symprec)
        sym2 = _result(find_symmetry, cells[idx], [pos_of[b] for b in again], zs2, symprec=symprec, device=dev)
        same_symmetry(b2, info2, op2, map2, sym2)
        ns2 = [len(p) for p in poss2]
        two = guarded_pass(rep, True, cells[idx].contiguous(), torch.cat([pos_of[b] for b in again]), ns2, sym2.packed, symprec)
        same_pass(two, CELLS._pass(True, cells[idx].contiguous(), [pos_of[b] for b in again], ns2, sym2, symprec))
        cells[idx] = two["cells"]
        num[idx] = (two["num"][:, :, :, None] * num[idx][:, None, :, :]).sum(2)
        for k, b in enumerate(again):
            assert not two["info"][k, 4] and not two["info"][k, 7] and two["block"].payload["transform_den"][k] == 1
            info[b, :4] = two["info"][k, :4]
            src_of[b], pos_of[b] = src_of[b][cut(two["source"], two["out_ptr"], k).long()], cut(two["pos"], two["out_ptr"], k)
    res = _result(conventional_cell if conventional else primitive_cell, lats, poss, zs, symprec=symprec, device=DEV)
    assert _eq(res.lattices, cells) and res.ns == [len(p) for p in pos_of]
    for b in range(B):
        assert _eq(res.positions[b], pos_of[b]) and _eq(res.source_atom[b], src_of[b]) and _eq(res.transform_num[b], num[b]), b
    assert _eq(res.packed["positions"], torch.cat(pos_of)) and _eq(res.packed["source_atom"], torch.cat(src_of))
    assert res.packed["transform_num"].numel() == one["block"].extent("transform_num")[0]
    for b in range(B):  # (a structure that raised has zeros)
        if status[b]:
            info[b, :4], info[b, 5] = 0, 0
    assert res.transform_den == den and res.n_translations == info[:, 5].tolist() and res.multiplicity == info[:, 1].tolist()
    assert res.centring == [CELLS.CENTRINGS[v] for v in info[:, 2]] and res.crystal_system == [SYM.CRYSTAL_SYSTEMS[v] for v in info[:, 3]]
    if name.startswith("far") and name != "far_alone":
        k = {"far_first": 0, "far_middle": 1, "far_last": 2}[name]
        assert status[k] == CELLS.STATUS_SYMMETRY and one["out_ptr"][k] == one["out_ptr"][k + 1] and sum(bool(v) for v in status) == 1
    if name == "far_alone":
        assert one["n_out"] == [0] and one["block"].payload["out_pos"] is None and status == [CELLS.STATUS_SYMMETRY]
    rep.finish()  # (prints the case's launches and guarded buffers, per entry point)


# ======================================================================================================================
# symmetry-reduced phonons
# ======================================================================================================================
# the batch of tests/test_gpu_phonons_sym.py: its crystals of sym_ref.crystals(), its supercells, its masses and its forces
MASS = {29: 63.5, 6: 12.0, 12: 24.3, 30: 65.4, 16: 32.1, 50: 118.7, 3: 6.9, 8: 16.0, 11: 23.0, 17: 35.5}
NAMES = ["fcc", "diamond", "hcp", "wurtzite", "monoclinic", "triclinic_two_species", "fcc"]
SCS = [(2, 2, 2), (3, 3, 3), (2, 2, 2), (2, 2, 2), (3, 3, 3), (2, 2, 2), (2, 3, 4)]


def pair_forces(sl, cart):
    """a deterministic exponential pair repulsion over the images within one supercell of each other (float64 numpy)"""
    sl, cart = np.asarray(sl, dtype=np.float64), np.asarray(cart, dtype=np.float64)
    shifts = (np.indices((3, 3, 3)).reshape(3, -1).T - 1.0) @ sl
    d = cart[None, :, None, :] + shifts[None, None, :, :] - cart[:, None, None, :]
    r = np.sqrt((d * d).sum(-1))
    r = np.where(r > 1e-9, r, np.inf)
    return ((-2.0 * np.exp(-r / 0.7) / 0.7 / r)[..., None] * d).sum((1, 2))


def forces_fn(lats, poss):
    fs = [pair_forces(l.cpu().numpy(), p.cpu().numpy()) for l, p in zip(lats, poss)]
    return torch.zeros(len(fs), device=DEV), _t(np.concatenate(fs))


@pytest.mark.parametrize("names,scs", [(NAMES, SCS), (["fcc"], [(2, 2, 2)])], ids=["seven", "smallest"])
def test_symmetry_reduced_phonons_between_guards(names, scs):
    """The batch of tests/test_gpu_phonons_sym.py - 1, 1, 1, 2, 2, 6 and 3 displaced pairs, supercells of 8 to 54 atoms - and its
    smallest structure alone: plan, read-back of n_dir, displace, rows, solve, distribute, all pairs in one chunk."""
    Cs = sym_ref.crystals()
    lats, poss, zs = ([Cs[k][i] for k in names] for i in range(3))
    masses = [np.array([MASS[int(v)] for v in z]) for z in zs]
    res = find_symmetry(lats, poss, zs, device=DEV)
    pk, lib, delta = res.packed, PH._load_phsym(), 0.0137
    ns = [len(p) for p in poss]
    B, N = len(ns), sum(ns)
    ncell = [int(np.prod(c)) for c in scs]
    n_sc = [n * c for n, c in zip(ns, ncell)]
    ptr = np.concatenate([[0], np.cumsum(ns)])
    lat, dims, atom_ptr, pos = _t(np.stack(lats)), _t(scs, I32), _t(ptr, I32), _t(np.concatenate(poss))
    sym_in = {k: pk[k] for k in ("op_ptr", "map_ptr", "rotations", "atom_map")}
    rep = _report(f"phsym {len(names)} structures")

    plan = _block(rep, "alignn_phsym_plan_args").set(n_ops_total=pk["n_ops_total"], n_map_total=pk["n_map_total"], n_structs=B, n_atoms=N)
    plan.alloc("alignn_phsym_plan", dict(lattice=lat, supercell=dims, atom_ptr=atom_ptr, **sym_in))
    _run(plan, lib, "alignn_phsym_plan")
    n_dir = plan.payload["n_dir"].cpu().numpy()
    assert n_dir.min() >= 0 and n_dir.max() <= 3
    slots, slot_rows, reps, others, r = [], [], [], [], 0
    for b, n in enumerate(ns):
        for a in range(n):
            k = int(n_dir[ptr[b] + a])
            (reps if k else others).append((b, a))
            for m in range(k):
                slots.append((b, a, m))
                slot_rows.append(r)
                r += n_sc[b]
    g_total = r
    if len(names) > 1:
        assert sorted({sum(1 for s in slots if s[0] == b) for b in range(B)}) == [1, 2, 3, 6] and others

    jobs, row_off, pair_rows, r = [], [], [], 0
    for b, a, m in slots:
        pair_rows.append(r)
        for sg in (0, 1):
            jobs.append((b, a, m, sg))
            row_off.append(r)
            r += n_sc[b]
    super_lat = np.stack(lats) * np.array(scs, dtype=np.float64)[:, :, None]
    inv_super = np.stack([np.linalg.inv(x) for x in super_lat])
    disp = _block(rep, "alignn_phsym_displace_args").set(delta=delta, n_jobs=len(jobs), n_structs=B, N=N, rows=r)
    disp.alloc("alignn_phsym_displace", dict(positions=pos, atom_ptr=atom_ptr, lattice=lat, inv_supercell=_t(inv_super), supercell=dims,
                                             dirs=plan.payload["dirs"], jobs=_t(jobs, I32), row_off=_t(row_off, I64)))
    _run(disp, lib, "alignn_phsym_displace")
    cart = disp.payload["cart"].cpu().numpy()
    # cart = NULL, as the driver calls it on the model path: the same frac
    bare = _block(rep, "alignn_phsym_displace_args").set(delta=delta, n_jobs=len(jobs), n_structs=B, N=N, rows=r)
    bare.alloc("alignn_phsym_displace", {k: disp.payload[k] for k in disp.payload if k not in ("frac", "cart")}, null=("cart",))
    _run(bare, lib, "alignn_phsym_displace")
    assert bare.args.cart is None and _eq(bare.payload["frac"], disp.payload["frac"])
    forces = np.concatenate([pair_forces(super_lat[j[0]], cart[o:o + n_sc[j[0]]]) for j, o in zip(jobs, row_off)])

    rows = _block(rep, "alignn_phsym_rows_args").set(delta=delta, drift=PH.DRIFTS["frederiksen"], n_pairs=len(slots), n_structs=B,
                                                      force_rows=r, n_g_rows=g_total)
    rows.alloc("alignn_phsym_rows", dict(forces=_t(forces), pairs=_t([s[:2] for s in slots], I32), pair_rows=_t(pair_rows, I64),
                                         out_rows=_t(slot_rows, I64), atom_ptr=atom_ptr, supercell=dims))
    _run(rows, lib, "alignn_phsym_rows")

    fc_off = np.concatenate([[0], np.cumsum([c * 9 * n * n for c, n in zip(ncell, ns)])]).astype(np.int64)
    first = {(b, a): slot_rows[x] for x, (b, a, m) in enumerate(slots) if m == 0}
    common = dict(n_ops_total=pk["n_ops_total"], n_map_total=pk["n_map_total"], n_structs=B, max_supercell_atoms=max(n_sc), N=N,
                  n_g_rows=g_total, fc_total=int(fc_off[-1]))
    shared = dict(fc_off=_t(fc_off[:-1], I64), atom_ptr=atom_ptr, supercell=dims, shifts=pk["shifts"], rot=plan.payload["rot"], **sym_in)
    solve = _block(rep, "alignn_phsym_fc_args").set(n_items=len(reps), **common)
    solve.alloc("alignn_phsym_solve", dict(items=_t(reps, I32), g_rows=_t([first[x] for x in reps], I64), g=rows.payload["g"],
                                           **{k: plan.payload[k] for k in ("n_site", "site_ops", "n_dir", "dirs", "minv")}, **shared))
    _run(solve, lib, "alignn_phsym_solve")
    if others:
        dist = _block(rep, "alignn_phsym_fc_args").set(n_items=len(others), **common).adopt(solve, "fc")
        dist.alloc("alignn_phsym_distribute", dict(items=_t(others, I32), rep=plan.payload["rep"], dist_op=plan.payload["dist_op"], **shared))
        _run(dist, lib, "alignn_phsym_distribute")

    want = phonons(None, lats, poss, None, masses, supercell=scs, delta=delta, drift="frederiksen", symmetrize=0, dos_kpts=None,
                   forces_fn=forces_fn, device=DEV, displacements="symmetry", symmetry=res)
    assert want.n_supercells == len(jobs)
    assert _eq(solve.payload["fc"], torch.cat([c.reshape(-1) for c in want.force_constants]))
    theirs = PH._plan(lib, res, lat, dims, atom_ptr, ns, n_sc, torch.device(DEV))
    assert theirs["slots"] == slots and theirs["reps"] == reps and theirs["others"] == others
    for k in ("usable", "rot", "rep", "n_site", "site_ops", "n_dir", "dirs", "minv", "dist_op"):
        assert torch.equal(plan.payload[k].reshape(-1), theirs[k].reshape(-1)), k
        assert theirs[k].numel() == plan.extent(k)[0], k  # (d)
    rep.finish()  # (prints the case's launches and guarded buffers, per entry point)


# ======================================================================================================================
# the trajectory analyses: what their argument blocks share
# ======================================================================================================================
def _shared(b, sel, **more):
    """the scalars and the arrays that ``Inputs.fields`` fills, for the block ``b``: -> the inputs of its first allocation"""
    fields = {f[0] for f in b.args._fields_}
    scalars = dict(n_structs=len(sel.ns), n_atoms=sum(sel.ns), max_atoms=max(sel.ns), n_species=sel.n_species,
                   n_total_frames=sel.traj.shape[0], frame0=sel.frame0, frame_step=sel.frame_step, n_frames=sel.n_frames,
                   lattice_per_frame=int(sel.lattices.ndim == 4))
    b.set(**{k: v for k, v in scalars.items() if k in fields}, **more)
    return dict(traj=sel.traj, lattice=sel.lattices, atom_ptr=sel.atom_ptr, group=sel.group, group_count=sel.group_count)


def _only(b, entry, inputs):
    return {k: v for k, v in inputs.items() if k in b.table["fields"] and b.role(k, entry) != "unused"}


def _local_inputs(kind, cuts, first=None):
    fixed, moving, cells, per_frame = local_ref.inputs()
    traj, lat = (fixed, cells) if kind == "fixed" else (moving, per_frame)
    B = first or len(local_ref.SIZES)
    n = int(local_ref.PTR[B])
    lat = lat[:B] if lat.ndim == 3 else lat[:, :B]
    return _t(traj[:, :n]), _t(lat), local_ref.SIZES[:B], local_ref.SPECIES[:B], list(local_ref.R_CUTS[cuts][:B])


# ======================================================================================================================
# common-neighbour analysis and bond order
# ======================================================================================================================
@pytest.mark.parametrize("kind,cuts,adaptive,first,select", [("fixed", "each", False, None, {}), ("moving", "wide", True, None, {}),
                                                             ("moving", "each", False, 3, dict(start=1, step=2)),
                                                             ("fixed", "wide", True, 3, {})])
def test_cna_between_guards(kind, cuts, adaptive, first, select):
    traj, lat, ns, species, rc = _local_inputs(kind, cuts, first)
    rep = _report(f"cna {kind} {cuts} adaptive={int(adaptive)} B={len(ns)} {select}")
    sel = TI.inputs("cna", traj, lat, ns, select.get("start"), None, select.get("step"))
    sel.groups(species)
    lib = LOCAL._load()
    b = _block(rep, "alignn_local_cna_args")
    inputs = dict(_shared(b, sel, adaptive=int(adaptive)), r_cut=_t(rc))
    b.alloc("alignn_local_cna", _only(b, "alignn_local_cna", inputs))
    _run(b, lib, "alignn_local_cna")
    b.alloc("alignn_local_cna_counts")
    _run(b, lib, "alignn_local_cna_counts")
    assert int(b.payload["status"]) == 0
    res = cna(traj, lat, ns, species, r_cut=rc, adaptive=adaptive, **select)
    F, N, S = sel.n_frames, sum(ns), sel.n_species
    if select:
        assert (sel.frame0, sel.frame_step, F) == (1, 2, 1)
    P = b.payload
    assert _eq(P["structure"].view(F, N), res.structure) and _eq(P["signature_counts"].view(F, N, 5), res.signature_counts)
    assert _eq(P["n_neighbors"].view(F, N), res.n_neighbors) and _eq(P["counts"].view(len(ns), S + 1, F, 5), res.counts)
    assert _eq(P["fraction"].view(len(ns), S + 1, F, 5), res.fraction)
    rep.finish()  # (prints the case's launches and guarded buffers, per entry point)


@pytest.mark.parametrize("kind,cuts,ls,average,first,select,chunk", [("fixed", "each", (4, 6, 8, 12), True, None, {}, 2),
                                                                     ("moving", "each", (6,), False, 3, dict(start=1, step=2), 1),
                                                                     ("moving", "one", (4, 6), True, None, {}, 3),
                                                                     ("fixed", "one", (12,), True, 3, {}, 1)])
def test_bond_order_between_guards(kind, cuts, ls, average, first, select, chunk):
    """``chunk``: the frames per pass - 2 of 3 frames leaves a last chunk of one frame, with the scratch sized for two"""
    traj, lat, ns, species, rc = _local_inputs(kind, cuts, first)
    rep = _report(f"bond {kind} {cuts} ls={ls} average={int(average)} B={len(ns)} {select} chunk={chunk}")
    sel = TI.inputs("bond_order", traj, lat, ns, select.get("start"), None, select.get("step"))
    sel.groups(species)
    lib, L, F, N, S = LOCAL._load(), len(ls), sel.n_frames, sum(ns), sel.n_species
    table = np.zeros((L, LOCAL.W3J_STRIDE))
    for u, l in enumerate(ls):
        table[u, :(2 * l + 1) ** 2] = LOCAL.wigner_3j_table(l).reshape(-1)
    degree = {f"l{u}": l for u, l in enumerate(ls)}
    b = _block(rep, "alignn_local_bond_args")
    chunk = min(chunk, F)
    inputs = dict(_shared(b, sel, average=int(average), n_ls=L, chunk0=0, chunk_frames=chunk, **degree), r_cut=_t(rc),
                  ynorm=_t(np.array(LOCAL.ylm_norms())), w3j=_t(table))
    b.alloc("alignn_local_bond_qlm", _only(b, "alignn_local_bond_qlm", inputs))
    b.alloc("alignn_local_bond_finish", dict(w3j=inputs["w3j"]), null=() if average else ("s_avg", "t_avg", "q_avg", "w_avg"))
    for chunk0 in range(0, F, chunk):
        b.set(chunk0=chunk0, chunk_frames=min(chunk, F - chunk0))
        _run(b, lib, "alignn_local_bond_qlm", written=False)
        _run(b, lib, "alignn_local_bond_finish", written=False)
    b.written("alignn_local_bond_qlm").written("alignn_local_bond_finish")  # (after the last chunk: every frame has been written)
    assert int(b.payload["status"]) == 0
    res = bond_order(traj, lat, ns, species, r_cut=rc, ls=ls, average=average, **select)
    assert _eq(b.payload["n_neighbors"].view(F, N), res.n_neighbors)
    names = ("s", "t", "q", "w") + (("s_avg", "t_avg", "q_avg", "w_avg") if average else ())
    for k in names:
        assert _eq(b.payload[k].view(F, N, L), getattr(res, k)), k
    # the group means, as the driver takes them: alignn_order_steinhardt_mean on each array
    olib = ORDER._load()
    for k, name in enumerate(("q", "q_avg", "w", "w_avg")):
        if name not in names:
            continue
        m = _block(rep, "alignn_order_angle_args")
        m_in = dict(_shared(m, sel, n_bins=1, n_ls=L, **degree), q=b.payload[name])
        m.alloc("alignn_order_steinhardt_mean", _only(m, "alignn_order_steinhardt_mean", m_in))
        _run(m, olib, "alignn_order_steinhardt_mean")
        assert _eq(m.payload["mean"].view(len(ns), S + 1, F, L), res.mean[:, :, :, k].contiguous()), name
    rep.finish()  # (prints the case's launches and guarded buffers, per entry point)


# ======================================================================================================================
# angle distributions, Steinhardt q_l, S(q)
# ======================================================================================================================
def _order_inputs(kind):
    fixed, moving, per_frame = order_ref.inputs()
    return (_t(fixed), _t(order_ref.CELLS)) if kind == "fixed" else (_t(moving), _t(per_frame))


@pytest.mark.parametrize("kind,cuts,n_bins,select", [("fixed", "each", 67, {}), ("moving", "one", 67, dict(start=1, step=2))])
def test_adf_between_guards(kind, cuts, n_bins, select):
    """B = 3 with one structure of a single atom; 67 bins: no multiple of the 64 lanes that walk them"""
    traj, lat = _order_inputs(kind)
    ns, species, rc = order_ref.SIZES, order_ref.SPECIES, list(order_ref.R_CUTS[cuts])
    rep = _report(f"adf {kind} {cuts} {n_bins} {select}")
    sel = TI.inputs("adf", traj, lat, ns, select.get("start"), None, select.get("step"))
    sel.groups(species)
    lib = ORDER._load()
    b = _block(rep, "alignn_order_angle_args")
    inputs = dict(_shared(b, sel, n_bins=n_bins), r_cut=_t(rc))
    b.alloc("alignn_order_angles", _only(b, "alignn_order_angles", inputs), null=("q", "n_neighbors"))
    _run(b, lib, "alignn_order_angles")
    b.alloc("alignn_order_adf_finish")
    _run(b, lib, "alignn_order_adf_finish")
    assert int(b.payload["status"]) == 0
    res = adf(traj, lat, ns, species, r_cut=rc, n_bins=n_bins, **select)
    assert _eq(b.payload["counts"].view(res.counts.shape), res.counts) and _eq(b.payload["adf"].view(res.adf.shape), res.adf)
    assert _eq(b.payload["theta"], res.theta) and int(res.counts.sum()) > 0
    rep.finish()  # (prints the case's launches and guarded buffers, per entry point)


@pytest.mark.parametrize("kind,cuts,ls,select", [("moving", "each", (1, 6, 12), {}), ("fixed", "one", (4,), dict(start=1, step=2)),
                                                 ("fixed", "each", (4, 6, 8, 12), {})])
def test_steinhardt_between_guards(kind, cuts, ls, select):
    traj, lat = _order_inputs(kind)
    ns, species, rc = order_ref.SIZES, order_ref.SPECIES, list(order_ref.R_CUTS[cuts])
    rep = _report(f"steinhardt {kind} {cuts} {ls} {select}")
    sel = TI.inputs("steinhardt", traj, lat, ns, select.get("start"), None, select.get("step"))
    sel.groups(species)
    lib, L = ORDER._load(), len(ls)
    b = _block(rep, "alignn_order_angle_args")
    inputs = dict(_shared(b, sel, n_bins=1, n_ls=L, **{f"l{u}": l for u, l in enumerate(ls)}), r_cut=_t(rc))
    b.alloc("alignn_order_angles", _only(b, "alignn_order_angles", inputs), null=("counts",))
    _run(b, lib, "alignn_order_angles")
    b.alloc("alignn_order_steinhardt_mean")
    _run(b, lib, "alignn_order_steinhardt_mean")
    assert int(b.payload["status"]) == 0
    res = steinhardt(traj, lat, ns, species, r_cut=rc, ls=ls, **select)
    assert _eq(b.payload["q"].view(res.q.shape), res.q) and _eq(b.payload["n_neighbors"].view(res.n_neighbors.shape), res.n_neighbors)
    assert _eq(b.payload["mean"].view(res.mean.shape), res.mean)
    rep.finish()  # (prints the case's launches and guarded buffers, per entry point)


@pytest.mark.parametrize("which", ["batch", "long"])
def test_structure_factor_between_guards(which):
    """batch: B = 3 (one structure of a single atom), 50 bins; long: 130 frames of the 5-atom structure, every second from frame 1:
    65 frames used, one full chunk of the frame sum and a last chunk of one frame"""
    if which == "batch":
        traj, lat = _order_inputs("fixed")
        ns, species, select = order_ref.SIZES, order_ref.SPECIES, {}
    else:
        traj, lat = _t(order_ref.long_inputs()), _t(order_ref.CELLS[1:2])
        ns, species, select = [5], [order_ref.SPECIES[1]], dict(start=1, step=2)
    n_bins, q_max = order_ref.SQ_BINS, order_ref.Q_MAX
    rep = _report(f"sq {which}")
    sel = TI.inputs("structure_factor", traj, lat, ns, select.get("start"), None, select.get("step"), per_frame=False, atom_limit=False)
    sel.groups(species)
    lib, B = ORDER._load(), len(ns)
    b = _block(rep, "alignn_order_sq_args")
    inputs = _shared(b, sel, q_max=q_max, n_bins=n_bins, n_vectors=0, max_vectors=0)
    V1, V2 = "alignn_order_sq_vectors", "alignn_order_sq_accumulate"
    b.alloc(V1, _only(b, V1, inputs), null=("vec_ptr", "hkl", "qnorm", "vbin"))  # the counting call: hkl = NULL
    _run(b, lib, V1)
    assert int(b.payload["status"]) == 0
    n_vec = b.payload["n_vec"].cpu().numpy().astype(np.int64)
    offsets = np.concatenate([[0], np.cumsum(n_vec)])
    V = int(offsets[-1])
    assert 0 < V < 10 ** 6 and n_vec.min() >= 0
    b.set(n_vectors=V, max_vectors=int(n_vec.max()))
    b.alloc(V1, dict(vec_ptr=_t(offsets, I32)))
    _run(b, lib, V1)
    b.alloc(V2, _only(b, V2, {k: v for k, v in inputs.items() if k not in b.payload}))
    _run(b, lib, V2)
    b.alloc("alignn_order_sq_bin", dict(group_count=inputs["group_count"]))
    _run(b, lib, "alignn_order_sq_bin")
    if which == "long":
        assert sel.n_frames == 65 and b.extent("partial")[0] == 2 * 4 * V
    res = structure_factor(traj, lat, ns, species, q_max=q_max, n_bins=n_bins, **select)
    P = b.payload
    assert _eq(P["s"].view(res.s.shape), res.s) and _eq(P["n_vectors_bin"].view(res.n_vectors.shape), res.n_vectors) and _eq(P["centres"], res.q)
    assert _eq(P["hkl"], torch.cat(res.hkl)) and _eq(P["s_vec"], torch.cat(res.s_vectors, dim=1))
    # qnorm and vbin, which the driver does not return, against the restatement of the header's formula: the same dozen correctly
    # rounded float64 operations in the same order on both sides, so at most 16 roundings of 2^-53 apart; the shell of a vector
    # is the same integer where |q| lies farther than that from a shell edge (the margin the restatement returns)
    cells_h = lat.cpu().numpy()
    for b in range(B):
        hkl, qn, shell, margin = order_ref.sq_vectors(cells_h[b], q_max, n_bins)
        lo, hi = int(offsets[b]), int(offsets[b + 1])
        assert np.array_equal(P["hkl"][lo:hi].cpu().numpy(), hkl) and margin > 16 * 2.0 ** -53
        assert bool((np.abs(P["qnorm"][lo:hi].cpu().numpy() - qn) <= 16 * 2.0 ** -53 * qn).all())
        assert np.array_equal(P["vbin"][lo:hi].cpu().numpy(), shell)
    rep.finish()  # (prints the case's launches and guarded buffers, per entry point)


# ======================================================================================================================
# RDF and time correlations
# ======================================================================================================================
@pytest.mark.parametrize("kind,n_bins,select", [("fixed", 50, {}), ("fixed", 67, dict(start=1, step=2)), ("moving", 67, {}),
                                                ("fixed", 4096, {})])
def test_rdf_between_guards(kind, n_bins, select):
    """SIZES = [1, 5, 70]; 4096 bins x six pair types is more than the LDS histogram holds: the chunked pair types (once)"""
    traj, lat = _order_inputs(kind)
    ns, species, r_max = order_ref.SIZES, order_ref.SPECIES, 6.0
    rep = _report(f"rdf {kind} {n_bins} {select}")
    sel = TI.inputs("rdf", traj, lat, ns, select.get("start"), None, select.get("step"), atom_limit=False)
    sel.groups(species)
    lib = TRAJ._load()
    b = _block(rep, "alignn_traj_rdf_args")
    inputs = _shared(b, sel, r_max=r_max, n_bins=n_bins)
    b.alloc("alignn_traj_rdf_counts", _only(b, "alignn_traj_rdf_counts", inputs))
    _run(b, lib, "alignn_traj_rdf_counts")
    b.alloc("alignn_traj_rdf_normalise")
    _run(b, lib, "alignn_traj_rdf_normalise")
    assert int(b.payload["status"]) == 0
    res = rdf(traj, lat, ns, species, r_max=r_max, n_bins=n_bins, **select)
    P = b.payload
    assert _eq(P["counts"].view(res.counts.shape), res.counts) and _eq(P["g"].view(res.g.shape), res.g) and int(res.counts.sum()) > 0
    assert _eq(P["coord"].view(res.coordination.shape), res.coordination) and _eq(P["volume"], res.volume) and _eq(P["centres"], res.r)
    rep.finish()  # (prints the case's launches and guarded buffers, per entry point)


@pytest.mark.parametrize("mode,com,max_lag,stride,select", [(0, True, None, 1, {}), (0, False, 0, 1, {}), (0, True, 2, 2, dict(start=1, step=2)),
                                                            (1, False, None, 1, dict(start=1, step=2)), (1, False, 0, 2, {})])
def test_time_correlations_between_guards(mode, com, max_lag, stride, select):
    """mode 0 (MSD) with the centre of mass given and NULL, mode 1 (VACF); max_lag 0 and the frames used less one (None)"""
    ns, species = order_ref.SIZES, order_ref.SPECIES
    N, F = sum(ns), 7
    g = torch.Generator().manual_seed(4)
    traj = torch.randn(F, N, 3, generator=g, dtype=F64).cumsum(0).to(DEV)
    masses = [1.0 + 30.0 * torch.rand(n, generator=g, dtype=F64).numpy() for n in ns]
    rep = _report(f"corr mode={mode} com={int(com)} max_lag={max_lag} stride={stride} {select}")
    frame0, fstep, used = TI._frames("corr", F, select.get("start"), None, select.get("step"))
    ptr, group, count, S, _ = TI._groups("corr", ns, species, torch.device(DEV))
    K = used - 1 if max_lag is None else max_lag
    lib = TRAJ._load()
    b = _block(rep, "alignn_traj_corr_args").set(n_structs=len(ns), n_atoms=N, n_species=S, n_total_frames=F, frame0=frame0,
                                                  frame_step=fstep, n_frames=used, max_lag=K, origin_stride=stride, mode=mode)
    inputs = dict(traj=traj, atom_ptr=ptr, group=group, group_count=count)
    if mode == 1 or com:
        inputs["masses"] = TI._masses("corr", masses, ns, torch.device(DEV))
    if com:
        b.alloc("alignn_traj_com", _only(b, "alignn_traj_com", inputs))
        _run(b, lib, "alignn_traj_com")
    b.alloc("alignn_traj_corr", {k: v for k, v in inputs.items() if k not in b.payload}, null=() if com else ("com", "masses")[:2 - mode])
    _run(b, lib, "alignn_traj_corr")
    if mode == 0:
        res = msd(traj, ns, species, masses if com else None, max_lag=max_lag, origin_stride=stride, remove_com=com, **select).msd
    else:
        res = vacf(traj, ns, species, masses, max_lag=max_lag, origin_stride=stride, **select).vacf
    assert res.shape[2] == K + 1 and _eq(b.payload["out"].view(res.shape), res)
    rep.finish()  # (prints the case's launches and guarded buffers, per entry point)


# ======================================================================================================================
# the detector itself, on the device
# ======================================================================================================================
def test_a_stray_write_on_the_device_is_reported():
    """the counterpart of test_gpu_conv_extents.py's: a torch indexing operation on the test's own buffers, no kernel involved - one
    element behind a guarded int64 array and one row in front of a guarded float64 array that ``Block`` built"""
    rep = _report("stray write on the device")
    b = _block(rep, "alignn_traj_rdf_args").set(n_structs=2, n_species=1, n_bins=67)
    b.alloc("alignn_traj_rdf_normalise", dict(lattice=torch.eye(3, dtype=F64, device=DEV).repeat(2, 1, 1),
                                              group_count=torch.ones(2, 2, dtype=I32, device=DEV),
                                              counts=torch.zeros(2, 2, 67, dtype=I64, device=DEV)))
    assert rep.guards.check() == []
    counts, g = rep.guards.record_of(b.payload["counts"]), rep.guards.record_of(b.payload["g"])
    assert g.row == 67 and counts.base.is_cuda
    counts.base[counts.before + counts.numel] = 0
    found = rep.guards.check()
    assert [f[:3] for f in found] == [("counts of alignn_traj_rdf_args", "after", 0)]
    counts.base[counts.before + counts.numel] = gp.INT_PATTERN[I64]
    g.base[g.before - 67] = 1.0
    found = rep.guards.check()
    assert [f[:4] for f in found] == [("g of alignn_traj_rdf_args", "before", -67, -1.0)]
    with pytest.raises(AssertionError, match="g of alignn_traj_rdf_args: the guard before the payload changed at offset -67"):
        rep.finish()
