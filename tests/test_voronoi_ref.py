"""The numpy restatement of the Voronoi analysis (tests/voronoi_ref.py) against an independent tessellation, without a GPU, and
the conditions on the test inputs that make the device's integers comparable exactly (tests/test_gpu_voronoi.py).

* On the jittered structures the restatement's volumes equal those of ``scipy.spatial.Voronoi`` + ``ConvexHull`` on the 27-image
  point set, and its face counts equal the ridge counts of the same tessellation.
* The volumes of a frame sum to |det C|.
* The perfect crystals have the textbook index with the thresholds of ``CRYSTAL_THRESHOLDS``.
* Input conditions: no face area lies within a factor 10 of a face threshold used, no edge length within a factor 10 of an edge
  threshold used, every atom has at most 64 entries, every atom of the jittered structures has r_max <= 0.9 r_cut / 2."""

import itertools

import numpy as np
import pytest

from tests import voronoi_ref as ref

R = ref.GENERIC_R_CUT


def _scipy_cells(C, pos):
    """-> (volume [n], ridges [n]) of the central cells of the 27-image point set"""
    spatial = pytest.importorskip("scipy.spatial")
    shifts = np.array(sorted(itertools.product((-1, 0, 1), repeat=3), key=lambda s: s != (0, 0, 0)), dtype=np.float64)
    n = len(pos)
    points = (pos[None, :, :] + (shifts @ C)[:, None, :]).reshape(-1, 3)
    v = spatial.Voronoi(points)
    volume = np.array([spatial.ConvexHull(v.vertices[v.regions[v.point_region[i]]]).volume for i in range(n)])
    ridges = np.zeros(n, dtype=np.int64)
    for a, b in v.ridge_points:
        for i in (a, b):
            if i < n:
                ridges[i] += 1
    return volume, ridges


@pytest.mark.parametrize("which", ["J", "K"])
def test_volumes_and_face_counts_are_those_of_scipy(which):
    pytest.importorskip("scipy")
    C, traj = ref.generic(which)
    for f in range(ref.FRAMES):
        volume, ridges = _scipy_cells(C, traj[f])
        mine = ref.cells(C, traj[f], R)
        assert np.allclose(mine["volume"], volume, rtol=1e-9, atol=0.0), (which, f)
        assert np.array_equal(mine["n_faces"], ridges), (which, f)
        assert np.array_equal(mine["index"].sum(-1), mine["n_faces"])  # no face of these has more than 10 edges
        assert mine["complete"].all()


@pytest.mark.parametrize("which", ["J", "K"])
def test_volumes_sum_to_the_cell(which):
    C, traj = ref.generic(which)
    for f in range(ref.FRAMES):
        mine = ref.cells(C, traj[f], R)
        assert abs(mine["volume"].sum() - ref.volume_of(C)) <= 1e-12 * ref.volume_of(C)
    cells, traj = ref.scaled()
    for f, s in enumerate(ref.SCALES):
        mine = ref.cells(cells[f, 0], traj[f], R)
        assert abs(mine["volume"].sum() - s ** 3 * ref.volume_of(C)) <= 1e-12 * ref.volume_of(C) and mine["complete"].all()


@pytest.mark.parametrize("name", ref.CRYSTALS)
def test_perfect_crystals_have_the_textbook_index(name):
    """With thresholds of 0 the raw counts of these degenerate cells depend on rounding (12, 13 or 14 faces for fcc, as the whole
    crystal moves from frame to frame): they are not pinned."""
    C, traj, r_cut, index = ref.crystal(name)
    n = traj.shape[1]
    for f in range(ref.FRAMES):
        mine = ref.cells(C, traj[f], r_cut, **ref.CRYSTAL_THRESHOLDS)
        assert (mine["index"] == np.array(index)).all() and (mine["n_faces"] == sum(index)).all(), (name, f)
        assert np.allclose(mine["volume"], ref.volume_of(C) / n, rtol=1e-12, atol=0.0)
        assert mine["n_entries"].max() <= 32 and mine["complete"].all() and mine["max_vertices"] <= 12
    if name == "diamond":
        assert max(ref.cells(C, traj[f], r_cut)["max_vertices"] for f in range(ref.FRAMES)) == 12


def _clear(values, threshold):
    """no value within a factor 10 of the threshold (a threshold of 0: no value is 0 but those of the faces that are not there)"""
    values = values[values > 0.0]
    return not ((values > threshold / 10.0) & (values < threshold * 10.0)).any()


def test_input_conditions_of_the_device_comparison():
    for which in ("J", "K"):
        C, traj = ref.generic(which)
        for f in range(ref.FRAMES):
            areas, rel, sides, entries, r_max = ref.margins(C, traj[f], R)
            assert entries <= 64 and r_max <= 0.9 * R / 2.0, (which, f, entries, r_max)
            for t in (0.0, ref.CRYSTAL_THRESHOLDS["face_threshold"]):
                assert _clear(areas, t)
            for t in (0.0, ref.CRYSTAL_THRESHOLDS["edge_threshold"]):
                assert _clear(sides, t)
            assert not (sides == 0.0).any() and not ((areas < 0.0) & (areas > -1e-300)).any()
    # the thresholds of the threshold test, on the one frame it uses: they count something out and nothing is near them
    C, traj = ref.generic("J")
    areas, rel, sides, _, _ = ref.margins(C, traj[0], R)
    assert _clear(rel, ref.REL_THRESHOLD) and _clear(sides, ref.EDGE_THRESHOLD)
    assert ((rel > 0.0) & (rel < ref.REL_THRESHOLD)).sum() >= 1 and ((sides > 0.0) & (sides < ref.EDGE_THRESHOLD)).sum() >= 1
    plain, cut = ref.cells(C, traj[0], R), ref.cells(C, traj[0], R, 0.0, ref.REL_THRESHOLD, ref.EDGE_THRESHOLD)
    assert (plain["n_faces"] != cut["n_faces"]).any() and (plain["index"] != cut["index"]).any()
    assert np.array_equal(plain["volume"], cut["volume"]) and np.array_equal(plain["area"], cut["area"])
    for name in ref.CRYSTALS:  # the crystals: every face and edge is of order 1 or of order 1e-15
        C, traj, r_cut, _ = ref.crystal(name)
        for f in range(ref.FRAMES):
            areas, _, sides, entries, r_max = ref.margins(C, traj[f], r_cut)
            assert _clear(areas, ref.CRYSTAL_THRESHOLDS["face_threshold"]) and _clear(sides, ref.CRYSTAL_THRESHOLDS["edge_threshold"])
            assert entries <= 64 and r_max < r_cut / 2.0


def test_certification_in_the_restatement():
    C, traj = ref.generic("J")
    small = ref.cells(C, traj[0], 3.0)  # an r_cut that is too small: no cell is certified, though every list has entries
    assert not small["complete"].any() and small["n_entries"].min() >= 1 and np.isfinite(small["r_max"]).all()
    C, traj = ref.slab()
    for f in range(ref.FRAMES):
        z = traj[f][:, 2] - traj[f][:, 2].min()
        mine = ref.cells(C, traj[f], ref.SLAB_R_CUT, **ref.CRYSTAL_THRESHOLDS)
        assert np.array_equal(mine["complete"], (z > 1.0) & (z < 9.0)) and mine["complete"].sum() == 8
        assert (mine["index"][mine["complete"]] == np.array([0, 12, 0, 0, 0, 0, 0, 0])).all()
        assert np.allclose(mine["volume"][mine["complete"]], 16.0, rtol=1e-12, atol=0.0)
        assert (mine["r_max"][~mine["complete"]] > 4.0 * ref.SLAB_R_CUT).all()  # the square shows: the cell is open


def test_an_atom_alone_has_no_face():
    mine = ref.cells(20.0 * np.eye(3), np.array([[0.0, 0.0, 0.0], [10.0, 10.0, 10.0]]), 3.0)
    assert mine["n_entries"][0] == 0 and np.isinf(mine["r_max"][0]) and not mine["complete"][0] and mine["volume"][0] == 0.0
