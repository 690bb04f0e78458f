"""The host side of alignn_amd/_jobs.py without a GPU: the grouping of the jobs into ``relax`` calls, and the layer count of a
slab against the restatement of tests/defects_ref.py."""

import numpy as np
import pytest

from alignn_amd._jobs import group_jobs, slab_layers
from alignn_amd.synthetic import make_crystal
from tests import defects_ref as ref

HKLS = [(1, 0, 0), (0, 0, 1), (1, 1, 0), (1, 1, 1), (2, 1, 1), (2, 1, 0), (1, -1, 0), (3, 2, 1)]  # those of tests/test_defects_ref.py


def _triclinic():
    lat, frac, _ = make_crystal(6, 77)
    lat = np.asarray(lat, dtype=np.float64)
    return lat, np.asarray(frac, dtype=np.float64) @ lat


PARENTS = {"fcc": ref.fcc(4.0), "rock_salt": ref.rock_salt(4.0)[:2], "triclinic": _triclinic()}

CASES = [([4] * 48, 8), ([4] * 48, 192), ([4] * 48, 10 ** 6), ([4] * 48, 1), ([4] * 48, 7), ([5], 3), ([1], 1),
         ([3, 9, 2, 2, 8, 1, 1, 1, 7], 8), ([8, 8, 1, 7, 1], 8), ([2, 3, 4], 9), ([2, 3, 4], 8)]


@pytest.mark.parametrize("counts,cap", CASES)
def test_groups_hold_every_job_once_in_order_and_whole(counts, cap):
    groups = group_jobs(counts, cap)
    assert [j for g in groups for j in g] == list(range(len(counts)))
    assert all(len(g) >= 1 for g in groups)
    for g in groups:
        assert sum(counts[j] for j in g) <= cap or len(g) == 1
    # first fit in sequence: a group is closed only when the next job would not have fitted
    for g, nxt in zip(groups, groups[1:]):
        assert sum(counts[j] for j in g) + counts[nxt[0]] > cap


def test_the_groupings_the_gpu_tests_count():
    counts = [4] * 48
    assert group_jobs(counts, 8) == [[2 * i, 2 * i + 1] for i in range(24)]  # tests/test_gpu_elastic.py: 24 calls
    assert group_jobs(counts, 192) == [list(range(48))] and group_jobs(counts, 32768) == [list(range(48))]
    assert group_jobs(counts, 1) == [[j] for j in range(48)]
    assert group_jobs([3, 9, 2, 2, 8, 1, 1, 1, 7], 8) == [[0], [1], [2, 3], [4], [5, 6, 7], [8]]


@pytest.mark.parametrize("name", list(PARENTS))
@pytest.mark.parametrize("hkl", HKLS)
@pytest.mark.parametrize("thickness", [0.5, 12.0, 25.0])
def test_slab_layers_is_the_restatement(name, hkl, thickness):
    lat, pos = PARENTS[name]
    basis = ref.miller_basis(lat, hkl)
    assert slab_layers("t", "the lattice", "the slab", lat, basis, hkl, thickness, len(pos)) == ref.layers_for(lat, basis, thickness)


def test_slab_layers_words_its_errors_as_the_caller_says():
    basis = np.eye(3, dtype=np.int64)
    flat = np.array([[4.0, 0.0, 0.0], [0.0, 4.0, 0.0], [4.0, 4.0, 0.0]])
    with pytest.raises(ValueError, match=r"^who: lattices\[3\] has no volume$"):
        slab_layers("who", "lattices[3]", "structure 3", flat, basis, (0, 0, 1), 12.0, 4)
    with pytest.raises(ValueError, match=r"^who: thickness 1e\+300 gives too many layers of \(0, 0, 1\) for pairs\[2\]$"):
        slab_layers("who", "the film lattice 0", "pairs[2]", 4.0 * np.eye(3), basis, (0, 0, 1), 1e300, 4)
