"""The Voronoi analysis on the device (csrc/voronoi.hip, alignn_amd/voronoi.py) against the restatement of tests/voronoi_ref.py,
whose inputs these are (tests/test_voronoi_ref.py asserts the conditions under which the integers below are comparable exactly):
(a) perfect crystals - one atom among its own images at image range 2, fcc, bcc, diamond (polygons of 12 vertices), ideal hcp -
with small thresholds: the textbook index and V / N; (b) a jittered structure of 32 atoms in a triclinic cell, up to 50 list
entries, thresholds 0: every integer bit for bit, every float under the measured bound, the volumes sum to |det C|; (c) per-frame
cells; (d) a structure alone and in a batch of 5 (1, 2, 8, 32, 32 atoms) at two places: the same bits in every output; (e)
species; (f) thresholds that count faces and edges out; (g) certification - an r_cut too small, a slab; (h) the refusals; (i)
``voronoi_census``.

With thresholds of 0 the raw face counts of the perfect crystals depend on rounding - several planes pass through one vertex, and
a face of 1e-30 A^2 is there or not: 12, 13 or 14 faces for fcc as the crystal moves as a whole.  No test here pins them.

The bound on the floats.  MEASURED: the largest deviation of ``volume``, ``area``, ``r_max``, ``face_area`` and ``mean`` from the
float64 restatement seen on an MI355X over all the tests of this file, relative to the largest magnitude of the array compared
(every test prints its own).  The sums against V / N of a crystal and |det C| of a frame are held to the same allowance.  The per-face arithmetic is restated operation for operation and came out bit for bit; what differs
is the order of the sums over the faces and over the atoms, which the restatement takes exactly.  The tests allow 10 x that, the
margin the earlier analysis modules took for rounding in a different operation order."""

import collections

import numpy as np
import pytest
import torch

from alignn_amd import voronoi, voronoi_census
from tests import traj_ref
from tests import voronoi_ref as ref

pytestmark = pytest.mark.gpu
DEV = "cuda"

MEASURED = 2.22e-16  # (the means; volume, area and face_area 2.2e-16 at most, r_max 0; the sums against V / N and |det C| 9.0e-16)
# The cube of the scale of a per-frame cell is no comparison with the restatement: the scaled positions and cells are rounded
# (2^-53 each) before either sees them, and a volume is a cubic form in some twenty differences of them - a few tens of roundings.
# Measured: 1.58e-15.
SCALE_TOL = 64 * 2.0 ** -53
TOL = 10.0 * MEASURED
FLOATS = ("volume", "area", "r_max")
INTS = ("n_faces", "index", "complete")
F = ref.FRAMES
R = ref.GENERIC_R_CUT


def _t(x, dtype=torch.float64):
    return torch.tensor(np.ascontiguousarray(x), dtype=dtype, device=DEV)


def _batch(structs):
    """[(C [3, 3] or [F, 3, 3], traj [F, n, 3], r_cut)] -> (traj, lattices, ns, r_cut) of one call"""
    per_frame = any(np.ndim(s[0]) == 3 for s in structs)
    cells = [np.broadcast_to(s[0], (F, 3, 3)) for s in structs] if per_frame else [s[0] for s in structs]
    lattices = np.stack(cells, axis=1) if per_frame else np.stack(cells)
    return _t(np.concatenate([s[1] for s in structs], axis=1)), _t(lattices), [s[1].shape[1] for s in structs], [s[2] for s in structs]


def _want(struct, frames=None, **thresholds):
    """the restatement of one structure, stacked over the frames: field -> [F_used, n, ..]"""
    C, traj, r_cut = struct
    frames = range(F) if frames is None else frames
    rows = [ref.cells(C[f] if np.ndim(C) == 3 else C, traj[f], r_cut, thresholds.get("face_threshold", 0.0),
                      thresholds.get("relative_face_threshold", 0.0), thresholds.get("edge_threshold", 0.0)) for f in frames]
    return {k: np.stack([r[k] for r in rows]) for k in rows[0] if k != "max_vertices"}


def _dev(name, got, want):
    """the deviation relative to the array's scale, printed before anything is asserted on it"""
    d = float(np.abs(got - want).max() / np.abs(want).max())
    print(f"{name}: deviation {d:.3e} of its scale (allowed {TOL:.3e})")
    return d


def _compare(res, structs, wants, what):
    """every per-atom output of ``res`` against the restatement -> the largest deviation of the floats"""
    worst, beg = 0.0, 0
    for b, (struct, want) in enumerate(zip(structs, wants)):
        n = struct[1].shape[1]
        rows = slice(beg, beg + n)
        beg += n
        for k in INTS + (("face_j", "face_edges") if res.face_j is not None else ()):
            got = getattr(res, k)[:, rows].cpu().numpy()
            assert got.dtype == want[k].dtype and np.array_equal(got, want[k]), (what, b, k)
        for k in FLOATS + (("face_area", "face_d") if res.face_j is not None else ()):
            got = getattr(res, k)[:, rows].cpu().numpy()
            if k == "face_d":
                assert np.array_equal(got, want[k]), (what, b, k)  # (the list's own numbers)
            else:
                worst = max(worst, _dev(f"{what} [{b}] {k}", got, want[k]))
    return worst


def _crystal_structs():
    return [(C, traj, r_cut) for C, traj, r_cut, _ in map(ref.crystal, ref.CRYSTALS)]


def _generic_structs():
    return [ref.generic("J") + (R,), ref.generic("K") + (R,)]


# --- (a) perfect crystals -----------------------------------------------------------------------------------------------------------
def test_perfect_crystals_have_the_textbook_index_and_volume():
    structs = _crystal_structs()
    traj, lattices, ns, cuts = _batch(structs)
    res = voronoi(traj, lattices, ns, r_cut=cuts, faces=True, **ref.CRYSTAL_THRESHOLDS)
    assert bool(res.complete.all()) and res.index.dtype == torch.int32 and res.volume.shape == (F, sum(ns))
    beg, worst = 0, 0.0
    for name, (C, _, _), n in zip(ref.CRYSTALS, structs, ns):
        index = np.array(ref.crystal(name)[3], dtype=np.int32)
        got = res.index[:, beg:beg + n].cpu().numpy()
        assert (got == index).all() and (res.n_faces[:, beg:beg + n].cpu().numpy() == index.sum()).all(), name
        volume = res.volume[:, beg:beg + n].cpu().numpy()
        worst = max(worst, _dev(f"{name} volume against V / N", volume, np.full_like(volume, ref.volume_of(C) / n)))
        beg += n
    worst = max(worst, _compare(res, structs, [_want(s, **ref.CRYSTAL_THRESHOLDS) for s in structs], "crystals"))
    assert worst <= TOL


# --- (b) the generic structure ------------------------------------------------------------------------------------------------------
def test_generic_structure_against_the_restatement():
    structs = _generic_structs()
    traj, lattices, ns, cuts = _batch(structs)
    res = voronoi(traj, lattices, ns, r_cut=R, faces=True)
    wants = [_want(s) for s in structs]
    assert max(int(w["n_entries"].max()) for w in wants) > 32 and bool(res.complete.all())
    worst = _compare(res, structs, wants, "generic")
    total = res.volume.cpu().numpy().reshape(F, 2, 32).sum(-1)  # per frame and structure
    worst = max(worst, _dev("generic: the volumes of a frame against |det C|", total, np.full_like(total, ref.volume_of(ref.GENERIC_CELL))))
    mean, count = res.mean.cpu().numpy(), res.n_complete.cpu().numpy()
    assert mean.shape == (2, 2, F, 3) and (count == 32).all() and np.array_equal(mean[:, 0], mean[:, 1])  # one species: group 1 is group 0
    for b, w in enumerate(wants):
        for f in range(F):
            m, _ = ref.group_means((w["volume"][f], w["area"][f], w["n_faces"][f]), w["complete"][f], np.ones(32, dtype=np.int64), 1)
            for c, k in enumerate(("volume", "area", "n_faces")):
                worst = max(worst, _dev(f"generic [{b}] frame {f} mean {k}", mean[b, :, f, c], m[:, c]))
    assert worst <= TOL


# --- (c) per-frame cells -------------------------------------------------------------------------------------------------------------
def test_per_frame_lattices_scale_the_volumes_by_the_cube():
    cells, traj = ref.scaled()
    struct = (cells[:, 0], traj, R)
    res = voronoi(_t(traj), _t(cells), [32], r_cut=R, faces=True)
    assert res.volume.shape == (F, 32)
    worst = _compare(res, [struct], [_want(struct)], "scaled")
    volume = res.volume.cpu().numpy()
    for f, s in enumerate(ref.SCALES):
        assert _dev(f"scaled by {s}: volume against s^3 x frame 0", volume[f], s ** 3 * volume[0]) <= SCALE_TOL
    assert np.array_equal(res.index[0].cpu().numpy(), res.index[2].cpu().numpy())  # the same cells, larger
    assert worst <= TOL


# --- (d) batch invariance ------------------------------------------------------------------------------------------------------------
OUTPUTS = ("volume", "area", "r_max", "n_faces", "index", "complete", "face_j", "face_d", "face_area", "face_edges")


def _bits(t):
    return t.view(torch.int64) if t.dtype == torch.float64 else t


def test_a_structure_alone_and_in_a_batch_gives_the_same_bits():
    sc, bcc, dia = [(C, traj, r_cut) for C, traj, r_cut, _ in map(ref.crystal, ("sc", "bcc", "diamond"))]
    J, K = _generic_structs()
    batch = [sc, bcc, dia, J, K]
    assert [s[1].shape[1] for s in batch] == [1, 2, 8, 32, 32]
    kw = dict(faces=True, **ref.CRYSTAL_THRESHOLDS)
    alone = []
    for s in batch:
        traj, lattices, ns, cuts = _batch([s])
        alone.append(voronoi(traj, lattices, ns, r_cut=cuts, **kw))
    for order in ([0, 1, 2, 3, 4], [4, 3, 0, 2, 1]):  # every structure at two places of the batch
        traj, lattices, ns, cuts = _batch([batch[k] for k in order])
        res = voronoi(traj, lattices, ns, r_cut=_t(cuts), **kw)
        beg = 0
        for at, k in enumerate(order):
            n = ns[at]
            for name in OUTPUTS:
                assert torch.equal(_bits(getattr(res, name)[:, beg:beg + n]), _bits(getattr(alone[k], name))), (order, k, name)
            assert torch.equal(_bits(res.mean[at]), _bits(alone[k].mean[0])) and torch.equal(res.n_complete[at], alone[k].n_complete[0])
            beg += n


# --- (e) species -----------------------------------------------------------------------------------------------------------------------
def test_means_per_species_over_the_complete_atoms():
    structs = _generic_structs()
    traj, lattices, ns, _ = _batch(structs)
    species = [ref.GENERIC_SPECIES, np.full(32, 13)]  # two species, and a structure with one: its group 2 has no member
    res = voronoi(traj, lattices, ns, species, r_cut=R)
    assert res.species == [[29, 40], [13]] and res.mean.shape == (2, 3, F, 3)
    mean, count = res.mean.cpu().numpy(), res.n_complete.cpu().numpy()
    worst = 0.0
    for b, s in enumerate(structs):
        w = _want(s)
        rank, _ = traj_ref.groups(species[b], 32)
        for f in range(F):
            m, c = ref.group_means((w["volume"][f], w["area"][f], w["n_faces"][f]), w["complete"][f], rank, 2)
            assert np.array_equal(count[b, :, f], c) and c[0] == c[1] + c[2] == 32
            for q, k in enumerate(("volume", "area", "n_faces")):
                worst = max(worst, _dev(f"species [{b}] frame {f} mean {k}", mean[b, :, f, q], m[:, q]))
            # group 0 is the union: its sum is the sum of the groups', to the rounding of the sums
            union = (mean[b, 1, f] * c[1] + mean[b, 2, f] * c[2]) / 32.0
            assert np.allclose(mean[b, 0, f], union, rtol=1e-14, atol=0.0)
    assert not mean[1, 2].any() and not count[1, 2].any()
    assert worst <= TOL


# --- (f) thresholds --------------------------------------------------------------------------------------------------------------------
def test_thresholds_count_faces_and_edges_out_and_leave_the_volume_alone():
    C, traj = ref.generic("J")
    kw = dict(relative_face_threshold=ref.REL_THRESHOLD, edge_threshold=ref.EDGE_THRESHOLD)
    args = (_t(traj), _t(C[None]), [32])
    plain = voronoi(*args, r_cut=R, faces=True, stop=1)
    cut = voronoi(*args, r_cut=R, faces=True, stop=1, **kw)
    struct = (C, traj, R)
    worst = _compare(cut, [struct], [_want(struct, frames=[0], **kw)], "thresholds")
    assert not torch.equal(cut.n_faces, plain.n_faces) and not torch.equal(cut.index, plain.index)
    for k in FLOATS:
        assert torch.equal(_bits(getattr(cut, k)), _bits(getattr(plain, k))), k
    assert (cut.relative_face_threshold, cut.edge_threshold, cut.face_threshold, cut.n_frames) == (ref.REL_THRESHOLD, ref.EDGE_THRESHOLD, 0.0, 1)
    assert worst <= TOL


# --- (g) certification -----------------------------------------------------------------------------------------------------------------
def test_an_r_cut_too_small_is_refused_or_flagged():
    C, traj = ref.generic("J")
    args = (_t(traj), _t(C[None]), [32])
    with pytest.raises(ValueError, match=r"not complete.*largest finite r_max.*raise r_cut.*strict=False"):
        voronoi(*args, r_cut=3.0)
    res = voronoi(*args, r_cut=3.0, strict=False, faces=True)
    struct = (C, traj, 3.0)
    want = _want(struct)
    assert not want["complete"].all()
    worst = _compare(res, [struct], [want], "r_cut 3.0")
    assert np.array_equal(res.n_complete.cpu().numpy()[0, 0], want["complete"].sum(-1))
    assert worst <= TOL


def test_a_slab_has_complete_cells_inside_and_open_ones_at_its_surfaces():
    C, traj = ref.slab()
    args = (_t(traj), _t(C[None]), [12])
    with pytest.raises(ValueError, match="strict=False for slabs"):
        voronoi(*args, r_cut=ref.SLAB_R_CUT, **ref.CRYSTAL_THRESHOLDS)
    res = voronoi(*args, r_cut=ref.SLAB_R_CUT, strict=False, **ref.CRYSTAL_THRESHOLDS)
    struct = (C, traj, ref.SLAB_R_CUT)
    want = _want(struct, **ref.CRYSTAL_THRESHOLDS)
    worst = _compare(res, [struct], [want], "slab")
    complete = res.complete.cpu().numpy()
    z = traj[..., 2] - traj[..., 2].min(axis=1, keepdims=True)
    assert np.array_equal(complete, (z > 1.0) & (z < 9.0)) and (res.n_complete.cpu().numpy() == 8).all()
    mean = res.mean.cpu().numpy()
    for f in range(F):  # the mean is over the complete atoms only: the interior's 16 A^3 and 12 faces, not the surfaces' squares
        m, _ = ref.group_means((want["volume"][f], want["area"][f], want["n_faces"][f]), want["complete"][f], np.ones(12, dtype=np.int64), 1)
        for q, k in enumerate(("volume", "area", "n_faces")):
            worst = max(worst, _dev(f"slab frame {f} mean {k}", mean[0, :, f, q], m[:, q]))
        assert abs(mean[0, 0, f, 0] - 16.0) < 1e-12 and mean[0, 0, f, 2] == 12.0
    assert float(res.r_max[~res.complete].min()) > 4.0 * ref.SLAB_R_CUT  # the first square shows: those cells are open
    assert worst <= TOL


# --- (h) the refusals ------------------------------------------------------------------------------------------------------------------
def test_error_paths():
    C, traj = ref.generic("J")
    t, lat = _t(traj), _t(C[None])
    with pytest.raises(ValueError, match="more than 64 neighbours"):
        voronoi(t, lat, [32], r_cut=7.0)
    sc, sc_traj, _, _ = ref.crystal("sc")
    with pytest.raises(ValueError, match="periodic images beyond"):
        voronoi(_t(sc_traj), _t(sc[None]), [1], r_cut=25.0)
    with pytest.raises(ValueError, match="select no frame"):
        voronoi(t, lat, [32], r_cut=R, start=F)
    with pytest.raises(TypeError, match="float64 tensor on the GPU"):
        voronoi(t.float(), lat, [32], r_cut=R)
    with pytest.raises(TypeError, match="float64 tensor on the GPU"):
        voronoi(t.cpu(), lat, [32], r_cut=R)
    with pytest.raises(TypeError, match="lattices must be a float64 tensor"):
        voronoi(t, lat.float(), [32], r_cut=R)
    with pytest.raises(ValueError, match=r"must be \[n_frames, 31, 3\]"):
        voronoi(t, lat, [31], r_cut=R)
    with pytest.raises(ValueError, match="lattices must be"):
        voronoi(t, lat[0], [32], r_cut=R)
    with pytest.raises(ValueError, match="lattices must be"):
        voronoi(t, _t(np.broadcast_to(C, (F + 1, 1, 3, 3))), [32], r_cut=R)
    with pytest.raises(ValueError, match="r_cut needs one number or one per structure"):
        voronoi(t, lat, [32], r_cut=[R, R])
    with pytest.raises(ValueError, match="r_cut as a tensor"):
        voronoi(t, lat, [32], r_cut=torch.tensor([R], dtype=torch.float32, device=DEV))
    for bad in (dict(face_threshold=-1.0), dict(relative_face_threshold=float("nan")), dict(edge_threshold=float("inf")),
                dict(edge_threshold="1"), dict(faces=1), dict(strict="no"), dict(step=0), dict(start=0.5)):
        with pytest.raises(ValueError):
            voronoi(t, lat, [32], r_cut=R, **bad)
    with pytest.raises(ValueError, match="species needs one array"):
        voronoi(t, lat, [32], [ref.GENERIC_SPECIES, ref.GENERIC_SPECIES], r_cut=R)


# --- (i) the census --------------------------------------------------------------------------------------------------------------------
def test_census_against_a_counter_on_the_host():
    structs = _generic_structs()
    traj, lattices, ns, _ = _batch(structs)
    species = [ref.GENERIC_SPECIES, np.full(32, 13)]
    res = voronoi(traj, lattices, ns, species, r_cut=R)
    index = res.index.cpu().numpy()
    for b, group, top in ((0, 0, 10), (0, 1, 3), (0, 2, 50), (1, 0, 1), (1, 1, 10)):
        rank, _ = traj_ref.groups(species[b], 32)
        cols = np.nonzero(traj_ref.members(rank, group))[0] + 32 * b
        counter = collections.Counter(tuple(int(x) for x in row) for row in index[:, cols].reshape(-1, 8))
        want = sorted(counter.items(), key=lambda kv: (-kv[1], kv[0]))[:top]
        tuples, counts, fraction = voronoi_census(res, b, group, top)
        assert tuples.dtype == torch.int32 and counts.dtype == torch.int64 and fraction.dtype == torch.float64
        assert [tuple(r) for r in tuples.cpu().tolist()] == [k for k, _ in want] and counts.cpu().tolist() == [v for _, v in want]
        assert np.array_equal(fraction.cpu().numpy(), np.array([v for _, v in want], dtype=np.float64) / float(F * len(cols)))
    for bad in (dict(b=2), dict(b=-1), dict(b=0, group=3), dict(b=1, group=2), dict(b=0, top=0), dict(b=0.0)):
        with pytest.raises(ValueError):
            voronoi_census(res, **bad)
