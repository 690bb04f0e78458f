"""Identities of the numpy restatement of the van Hove analysis (tests/vanhove_ref.py), without a GPU: nothing is dropped from
the self histogram; it agrees with the restatements it stands beside - ``traj_ref.msd``, ``traj_ref.rdf_counts``,
``order_ref.structure_factor`` - where the quantities coincide; a rigid translation gives what it must; and an atom that moved by
more than half a cell is left out of the distinct part as itself and counted as its images."""

import numpy as np

from tests import order_ref, traj_ref
from tests import vanhove_ref as ref

CELL = np.array([[4.0, 0.0, 0.0], [1.3, 3.8, 0.0], [0.7, -0.9, 4.4]])
SPECIES = np.array([8, 3, 8, 3, 3, 8])
R_MAX, N_BINS = 6.0, 50
LAGS = (0, 1, 3, 5)


def _walk(F=7, seed=3):
    rng = np.random.default_rng(seed)
    n = len(SPECIES)
    jump = np.cumsum(rng.integers(-2, 3, (F, n, 3)) * (rng.uniform(0, 1, (F, n, 1)) < 0.3), axis=0)
    traj = (rng.uniform(0, 1, (1, n, 3)) + jump) @ CELL + np.cumsum(rng.normal(0.0, 0.15, (F, n, 3)), axis=0)
    return traj, rng.uniform(1.0, 100.0, n)


def test_the_self_histogram_drops_nothing_and_its_second_moment_is_the_msd():
    traj, masses = _walk()
    rank, _ = traj_ref.groups(SPECIES, len(SPECIES))
    count = traj_ref.group_counts(rank, 2)
    for stride, remove_com in ((1, True), (2, False)):
        w, margin, binned = ref.self_part(traj, rank, 2, masses, LAGS, stride, remove_com, R_MAX, N_BINS, (0.8, 3.0))
        n_or = np.array([traj_ref.n_origins(len(traj), k, stride) for k in LAGS])
        assert margin > ref.EDGE_MARGIN and binned == int(n_or.sum()) * len(SPECIES)
        assert np.array_equal(w["counts"].sum(-1) + w["overflow"], count[:, None] * n_or[None, :])
        assert np.array_equal(w["counts"][0], w["counts"][1:].sum(0)) and np.array_equal(w["terms"], count[:, None] * n_or[None, :])
        assert w["overflow"].sum() > 0 and w["counts"][:, 1:].sum() > 0  # both kinds of term are there
        m, _ = traj_ref.msd(traj, rank, 2, masses, max(LAGS), stride, remove_com)
        total = (m[..., 0] + m[..., 1]) + m[..., 2]
        assert np.allclose(w["moments"][..., 0], total[:, list(LAGS)], rtol=1e-13, atol=0.0)
        assert not w["moments"][:, 0].any() and np.array_equal(w["fs"][:, 0], np.ones((3, 2)))  # lag 0: nobody has moved
        assert np.array_equal(w["counts"][:, 0, 0], count * n_or[0])
        p, gs, centres = ref.self_normalise(w["counts"], len(traj), LAGS, stride, count, R_MAX)
        share = w["overflow"] / (count[:, None] * n_or[None, :])
        assert np.allclose(p.sum(-1) * (R_MAX / N_BINS), 1.0 - share, rtol=1e-13) and np.allclose(centres[:2], [0.06, 0.18])
        assert np.allclose(gs * 4.0 * np.pi * (centres ** 2 + (R_MAX / N_BINS) ** 2 / 12.0), p, rtol=1e-12)


def test_the_distinct_part_at_lag_zero_is_the_pair_histogram_and_f_at_lag_zero_is_s():
    traj, masses = _walk()
    rank, _ = traj_ref.groups(SPECIES, len(SPECIES))
    counts, margin, binned = ref.distinct_counts(traj, CELL, rank, 2, None, (0,), 1, False, R_MAX, N_BINS)
    static, _, pairs = traj_ref.rdf_counts(traj, CELL, rank, 2, R_MAX, N_BINS)
    assert margin > ref.EDGE_MARGIN and binned == pairs and np.array_equal(counts[:, 0], static) and static.sum() > 0
    count = traj_ref.group_counts(rank, 2)
    g, V, centres = ref.distinct_normalise(counts, CELL, len(traj), (0,), 1, count, R_MAX)
    wg, _, wv, wr = traj_ref.rdf_normalise(static, CELL, len(traj), count, R_MAX)
    assert np.array_equal(g[:, 0], wg) and V == wv and np.array_equal(centres, wr)
    q_max, shells = 4.5, 20
    f = ref.intermediate_scattering(traj, CELL, rank, 2, q_max, shells, (0, 2), 1)
    s = order_ref.structure_factor(traj, CELL, rank, 2, q_max, shells)
    assert np.array_equal(f["hkl"], s["hkl"]) and len(f["hkl"]) > 20 and np.array_equal(f["n_vectors"], s["n_vectors"])
    assert np.allclose(f["f_vectors"][:, 0], s["s_vectors"], rtol=0.0, atol=1e-13) and np.allclose(f["f"][:, 0], s["s"], rtol=0.0, atol=1e-13)
    assert (np.abs(f["f_vectors"]) <= f["scale"] * (1.0 + 1e-12)).all() and np.abs(f["f_vectors"][:, 1]).max() > 0.01


def test_a_rigid_translation():
    """r(t) = r(0) + v t.  Without the centre of mass taken off every atom has moved by |v| k: one populated bin per lag, alpha_2
    = -2/5 (a delta distribution: <r^4> = <r^2>^2) and fs = j0(q |v| k).  With it taken off nothing has moved: every lag of the
    distinct part is the static pair histogram, once per origin."""
    rng = np.random.default_rng(8)
    n, F = len(SPECIES), 6
    x0, masses = rng.uniform(0, 1, (n, 3)) @ CELL, rng.uniform(1.0, 100.0, n)
    v = np.array([0.31, -0.22, 0.4])
    traj = x0[None] + v[None, None, :] * np.arange(F)[:, None, None]
    rank, _ = traj_ref.groups(SPECIES, n)
    count = traj_ref.group_counts(rank, 2)
    q = (0.9, 2.5)
    w, margin, _ = ref.self_part(traj, rank, 2, masses, LAGS, 1, False, R_MAX, N_BINS, q)
    assert margin > ref.EDGE_MARGIN and not w["overflow"].any()
    speed = float(np.sqrt((v * v).sum()))
    for l, k in enumerate(LAGS):
        n_or = traj_ref.n_origins(F, k, 1)
        assert np.array_equal(w["counts"][:, l, int(np.floor(speed * k * N_BINS / R_MAX))], count * n_or)  # the one bin holds them all
        assert np.allclose(w["moments"][:, l, 0], (speed * k) ** 2, rtol=1e-13) and np.allclose(w["fs"][:, l], ref.j0(np.array(q) * speed * k), atol=1e-13)
    a2 = ref.alpha2(w["moments"])
    assert np.allclose(a2[:, 1:], -0.4, atol=1e-12) and not a2[:, 0].any()
    counts, margin, _ = ref.distinct_counts(traj, CELL, rank, 2, masses, LAGS, 1, True, R_MAX, N_BINS)
    static, _, _ = traj_ref.rdf_counts(traj[:1], CELL, rank, 2, R_MAX, N_BINS)
    assert margin > ref.EDGE_MARGIN
    for l, k in enumerate(LAGS):
        assert np.array_equal(counts[:, l], static * traj_ref.n_origins(F, k, 1)), k


def test_an_atom_that_moved_by_more_than_half_a_cell():
    """One of three atoms moves between two frames by the cell vector (1, -1, 0) and a bit.  The distinct part leaves out
    exactly one term of that atom with itself - its unwrapped displacement, which the self part bins - and counts its other
    images, the wrapped displacement (the image that came in from the next cell) among them."""
    x0 = np.array([[0.5, 0.7, 0.2], [0.1, 0.2, 0.9], [0.8, 0.3, 0.5]]) @ CELL
    bit = np.array([0.21, -0.13, 0.08])
    move = np.array([1.0, -1.0, 0.0]) @ CELL + bit
    x1 = x0.copy()
    x1[0] += move
    r_own = float(np.sqrt((move * move).sum()))
    assert 0.5 * np.linalg.norm(CELL, axis=1).min() < r_own < R_MAX
    I, J, r = ref.cross_distances(CELL, x0, x1, R_MAX)
    M = traj_ref.image_range(CELL, R_MAX)
    images = int(np.prod([2 * m + 1 for m in M]))
    assert len(r) == 9 * images - 3  # one term left out per atom
    own = r[(I == 0) & (J == 0)]
    assert len(own) == images - 1 and np.abs(own - r_own).min() > 1e-3  # the unwrapped displacement is not among them ...
    assert np.abs(own - np.sqrt((bit * bit).sum())).min() < 1e-12      # ... the wrapped one is
    # every lattice point shifted by the bit, by plain geometry: those inside r_max, less the atom itself
    m = np.array([[a, b, c] for a in range(-4, 5) for b in range(-4, 5) for c in range(-4, 5)], dtype=np.float64)
    every = np.sqrt((((m @ CELL) + bit) ** 2).sum(1))
    assert np.allclose(np.sort(own[own < R_MAX]), np.sort(every[(every < R_MAX) & (np.abs(every - r_own) > 1e-9)]), rtol=0, atol=1e-12)
    # the atoms that did not move leave out their image 0, as the static pair histogram does
    Is, Js, r_static = traj_ref.pair_distances(CELL, x0, R_MAX)
    still = (I != 0) & (J != 0)
    assert np.allclose(np.sort(r[still]), np.sort(r_static[(Is != 0) & (Js != 0)]), rtol=0, atol=1e-12)
    rank = np.ones(3, dtype=np.int64)
    w, _, _ = ref.self_part(np.stack([x0, x1]), rank, 1, None, (1,), 1, False, R_MAX, N_BINS)
    assert w["counts"][0, 0, int(np.floor(r_own * N_BINS / R_MAX))] == 1 and w["counts"][0, 0, 0] == 2 and not w["overflow"].any()


def test_the_inputs_of_the_device_tests_keep_clear_of_the_bin_edges():
    """tests/test_gpu_vanhove.py compares histograms bit for bit: no term of its inputs lies within ``EDGE_MARGIN`` bin widths of an
    inner bin edge or of r_max (the seed was chosen so), with and without the centre of mass, at both bin counts."""
    traj, masses = ref.inputs()
    assert traj.shape == (ref.FRAMES, 76, 3) and [traj_ref.image_range(C, ref.R_MAX) for C in ref.CELLS] == [[2, 2, 2], [2, 2, 1], [0, 0, 0]]
    for b, n in enumerate(ref.SIZES):
        rank, _ = traj_ref.groups(ref.SPECIES[b], n)
        S = int(rank.max())
        x = traj[:, ref.rows(b)]
        for n_bins in (50, 4096):
            for remove_com in (True, False):
                _, m_self, _ = ref.self_part(x, rank, S, masses[b], ref.LAGS, 1, remove_com, ref.R_MAX, n_bins)
                _, m_distinct, _ = ref.distinct_counts(x, ref.CELLS[b], rank, S, masses[b], ref.LAGS, 1, remove_com, ref.R_MAX, n_bins)
                assert m_self > ref.EDGE_MARGIN and m_distinct > ref.EDGE_MARGIN, (b, n_bins, remove_com, m_self, m_distinct)
    jumped = np.abs(np.diff(traj, axis=0)).max(-1) > 1.5  # a move of more than half the smallest cell between two frames
    assert jumped[:, ref.rows(0)].any() and jumped[:, ref.rows(1)].any() and jumped[:, ref.rows(2)].mean() > 0.1
