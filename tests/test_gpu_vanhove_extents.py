"""The launches of include/alignn_vanhove.h, each between the guard bands of tests/gate_parity.py, every buffer of exactly the
extent the header states (tests/vanhove_extents.py, through ``workflow_extents.Block``).  The argument blocks are filled here in
the sequence the driver uses.  Asserted per entry point, in this order: (a) no guard bit changed after the launch; (b) no array the
header calls written holds a pattern element; (c) every output equals, bit for bit, what the driver returns for the same inputs on
its own plain allocations.  The shapes are those of tests/test_gpu_vanhove.py (tests/vanhove_ref.py holds them).

Blind spots (those of the instrument): an access farther from a buffer than its guard - 1024 elements or two rows - and a read
beside a buffer whose value is never used."""

import numpy as np
import pytest
import torch

from alignn_amd import _lib, intermediate_scattering, order, van_hove_distinct, van_hove_self, vanhove
from alignn_amd import _trajectory_inputs as TI
from tests import gate_parity as gp
from tests import vanhove_extents as vx
from tests import workflow_extents as wx
from tests.vanhove_ref import CELLS, FIVE, FRAMES as F, Q, Q_BINS, Q_MAX, R_MAX, SIZES, SPECIES, inputs as _inputs, selected as _selected

pytestmark = pytest.mark.gpu
DEV = "cuda"
F64, I32 = torch.float64, torch.int32


def _t(x, dtype=F64):
    return torch.tensor(np.ascontiguousarray(x), dtype=dtype, device=DEV)


def _block(rep, struct):
    return wx.Block(rep.guards, struct, DEV, rep.case, table=vx.TABLE)


def _run(b, lib, entry):
    b.launch(lib, entry, _lib.stream())
    return b.written(entry)


def _eq(a, b):
    return a.numel() == b.numel() and a.dtype == b.dtype and torch.equal(a.reshape(-1), b.reshape(-1))


def _only(b, entry, inputs):
    """the inputs that ``entry`` uses and the block does not hold yet"""
    return {k: v for k, v in inputs.items() if b.role(k, entry) != "unused" and k not in b.payload}


def _frames_and_lags(b, select, stride):
    sel, frames, lags = _selected(select)
    frame0, fstep, used = TI._frames("vanhove", F, sel.get("start"), None, sel.get("step"))
    lag = np.asarray(lags, dtype=np.int32)
    b.set(n_total_frames=F, frame0=frame0, frame_step=fstep, n_frames=used, n_lags=len(lag), origin_stride=stride)
    return sel, lag, vx.set_lags(b, lag)


def _com(traj, masses, ptr, S, b):
    a = b.args
    return vanhove._com("vanhove", traj, masses, SIZES, ptr, S, a.frame0, a.frame_step, a.n_frames)


@pytest.mark.parametrize("n_bins,stride,select,remove_com,which", [(50, 1, None, True, "three"), (4096, 3, (1, 2), False, "five")])
def test_van_hove_self_between_guards(n_bins, stride, select, remove_com, which):
    """three species in one chunk of the histogram, five in two; with and without the centre of mass (``com`` NULL)"""
    traj, masses = _inputs()
    species = SPECIES if which == "three" else FIVE
    t_traj, dev = _t(traj), torch.device(DEV)
    rep = gp.Report(f"vh_self {n_bins} {stride} {select} com={int(remove_com)} {which}", tag="vanhove-extents")
    ptr, group, count, S, _ = TI._groups("vh_self", SIZES, species, dev)
    lib = vanhove._load()
    b = _block(rep, "alignn_vh_self_args").set(r_max=R_MAX, n_structs=len(SIZES), n_atoms=sum(SIZES), n_species=S, n_bins=n_bins, n_q=len(Q))
    sel, lag, _ = _frames_and_lags(b, select, stride)
    inputs = dict(traj=t_traj, atom_ptr=ptr, group=group, group_count=count, lags=_t(lag, I32), q=_t(Q))
    if remove_com:
        inputs["com"] = _com(t_traj, masses, ptr, S, b)
    b.alloc("alignn_vh_self", _only(b, "alignn_vh_self", inputs), null=vx.HOST + (() if remove_com else ("com",)))
    _run(b, lib, "alignn_vh_self")
    b.alloc("alignn_vh_self_finish", null=vx.HOST)
    _run(b, lib, "alignn_vh_self_finish")
    res = van_hove_self(t_traj, SIZES, species, masses if remove_com else None, r_max=R_MAX, n_bins=n_bins, lags=list(lag),
                        origin_stride=stride, remove_com=remove_com, q=Q, **sel)
    P = b.payload
    for field, got in (("counts", res.counts), ("overflow", res.overflow), ("moments", res.moments), ("alpha2", res.alpha2), ("p", res.p),
                       ("gs", res.gs), ("fs", res.fs), ("centres", res.r)):
        assert _eq(P[field], got), field
    assert int(res.counts.sum()) > 0 and int(res.overflow.sum()) > 0
    rep.finish()  # (prints the case's launches and guarded buffers, per entry point)


@pytest.mark.parametrize("n_bins,stride,select,remove_com", [(50, 1, None, False), (4096, 3, (1, 2), True)])
def test_van_hove_distinct_between_guards(n_bins, stride, select, remove_com):
    """six pair rows of 4096 bins are more than the LDS histogram holds: the chunked rows (once)"""
    traj, masses = _inputs()
    t_traj, t_cells = _t(traj), _t(CELLS)
    rep = gp.Report(f"vh_distinct {n_bins} {stride} {select} com={int(remove_com)}", tag="vanhove-extents")
    lib = vanhove._load()
    b = _block(rep, "alignn_vh_distinct_args")
    sel, lag, _ = _frames_and_lags(b, select, stride)
    rec = TI.inputs("vh_distinct", t_traj, t_cells, SIZES, sel.get("start"), None, sel.get("step"), per_frame=False, atom_limit=False)
    S, _ = rec.groups(SPECIES)
    b.set(r_max=R_MAX, n_structs=len(SIZES), n_atoms=sum(SIZES), max_atoms=max(SIZES), n_species=S, n_bins=n_bins, lattice_per_frame=0)
    inputs = dict(traj=t_traj, lattice=t_cells, atom_ptr=rec.atom_ptr, group=rec.group, group_count=rec.group_count, lags=_t(lag, I32))
    if remove_com:
        inputs["com"] = _com(t_traj, masses, rec.atom_ptr, S, b)
    b.alloc("alignn_vh_distinct", _only(b, "alignn_vh_distinct", inputs), null=vx.HOST + (() if remove_com else ("com",)))
    _run(b, lib, "alignn_vh_distinct")
    b.alloc("alignn_vh_distinct_finish", null=vx.HOST)
    _run(b, lib, "alignn_vh_distinct_finish")
    assert int(b.payload["status"]) == 0
    res = van_hove_distinct(t_traj, t_cells, SIZES, SPECIES, masses if remove_com else None, r_max=R_MAX, n_bins=n_bins, lags=list(lag),
                            origin_stride=stride, remove_com=remove_com, **sel)
    P = b.payload
    assert _eq(P["counts"], res.counts) and _eq(P["g"], res.g) and _eq(P["volume"], res.volume) and _eq(P["centres"], res.r)
    assert int(res.counts.sum()) > 0
    rep.finish()  # (prints the case's launches and guarded buffers, per entry point)


@pytest.mark.parametrize("stride,select", [(1, None), (3, (1, 2))])
def test_intermediate_scattering_between_guards(stride, select):
    """about 1900 vectors in the large cell: two slabs of the modes launch, the second not full"""
    traj, _ = _inputs()
    t_traj, t_cells = _t(traj), _t(CELLS)
    rep = gp.Report(f"vh_fqt {stride} {select}", tag="vanhove-extents")
    lib = vanhove._load()
    b = _block(rep, "alignn_vh_fqt_args")
    sel, lag, _ = _frames_and_lags(b, select, stride)
    rec = TI.inputs("vh_fqt", t_traj, t_cells, SIZES, sel.get("start"), None, sel.get("step"), per_frame=False, atom_limit=False)
    S, _ = rec.groups(SPECIES)
    vec = order.reciprocal_vectors("vh_fqt", rec, Q_MAX, Q_BINS)
    assert vec.n_vectors > 1024 and vec.hkl.shape[0] == vec.n_vectors
    b.set(q_max=Q_MAX, n_structs=len(SIZES), n_atoms=sum(SIZES), n_species=S, n_bins=Q_BINS, n_vectors=vec.n_vectors,
          max_vectors=vec.max_vectors, lattice_per_frame=0)
    inputs = dict(traj=t_traj, lattice=t_cells, atom_ptr=rec.atom_ptr, group=rec.group, group_count=rec.group_count, vec_ptr=vec.vec_ptr,
                  hkl=vec.hkl, vbin=vec.vbin, lags=_t(lag, I32))
    for entry in ("alignn_vh_fqt_modes", "alignn_vh_fqt_correlate", "alignn_vh_fqt_bin"):
        b.alloc(entry, _only(b, entry, inputs), null=vx.HOST)
        _run(b, lib, entry)
    res = intermediate_scattering(t_traj, t_cells, SIZES, SPECIES, q_max=Q_MAX, n_bins=Q_BINS, lags=list(lag), origin_stride=stride, **sel)
    P = b.payload
    assert _eq(P["f"], res.f) and _eq(P["n_vectors_bin"], res.n_vectors) and _eq(P["centres"], res.q)
    assert _eq(P["f_vec"], torch.cat(res.f_vectors, dim=2).contiguous()) and float(res.f.abs().sum()) > 0
    rep.finish()  # (prints the case's launches and guarded buffers, per entry point)
