"""The restatement of the structural order analysis (tests/order_ref.py) against known answers, on the CPU: the Steinhardt
parameters and the bond angles of perfect lattices, the marginal rows of a two-species cell, S(q) of a perfect crystal (Bragg
peaks at the allowed reflections, nothing between them) and of an ideal gas (1), q_l against the spherical harmonics themselves;
and the precondition of the device tests' exact comparisons: the margins of their inputs."""

import numpy as np
import pytest

from tests import order_ref as ref

N_BINS = 67  # odd and no multiple of 3: 60, 90, 120 and 109.47 degrees fall inside bins


def _fcc(a=4.0):
    return a * np.eye(3), a * np.array([[0, 0, 0], [0, 0.5, 0.5], [0.5, 0, 0.5], [0.5, 0.5, 0]])


def _hcp(a=3.0):
    c = a * np.sqrt(8.0 / 3.0)
    cell = np.array([[a, 0, 0], [-a / 2, a * np.sqrt(3.0) / 2, 0], [0, 0, c]])
    return cell, np.array([[0, 0, 0], [1 / 3, 2 / 3, 0.5]]) @ cell


def _bcc(a=3.0):
    return a * np.eye(3), a * np.array([[0, 0, 0], [0.5, 0.5, 0.5]])


def _sc(a=3.0):
    return a * np.eye(3), np.zeros((1, 3))


# lattice, r_cut between the first two shells, Nb, q4, q6
LATTICES = [(_fcc, 3.3, 12, 0.19094, 0.57452), (_hcp, 3.6, 12, 0.09722, 0.48476), (_bcc, 2.8, 8, 0.50918, 0.62854),
            (_sc, 3.5, 6, 0.76376, 0.35355)]


@pytest.mark.parametrize("make,r_cut,nb,q4,q6", LATTICES)
def test_steinhardt_parameters_of_perfect_first_shells(make, r_cut, nb, q4, q6):
    cell, pos = make()
    n = len(pos)
    out = ref.angles(pos[None], cell, np.ones(n, dtype=np.int64), 1, r_cut, n_bins=N_BINS, ls=(4, 6))
    assert (out["n_neighbors"] == nb).all() and out["max_neighbors"] == nb
    assert np.abs(out["q"][..., 0] - q4).max() < 1e-5 and np.abs(out["q"][..., 1] - q6).max() < 1e-5
    assert np.abs(out["mean"][:, 0] - [q4, q6]).max() < 1e-5
    assert out["counts"][0, 0].sum() == n * nb * (nb - 1) // 2 == out["triplets"]


def test_bond_angles_of_fcc_and_the_normalisation():
    cell, pos = _fcc()
    out = ref.angles(pos[None], cell, np.ones(4, dtype=np.int64), 1, 3.3, n_bins=N_BINS)
    counts = out["counts"]
    assert counts.shape == (2, 2, N_BINS) and (counts[0, 0] == counts[1, 1]).all()
    w = 180.0 / N_BINS
    per_atom = {int(60 / w): 24, int(90 / w): 12, int(120 / w): 24, N_BINS - 1: 6}  # 180 degrees: the last bin
    for k in range(N_BINS):
        assert counts[1, 1, k] == 4 * per_atom.get(k, 0), k
    adf, theta = ref.adf_normalise(counts)
    assert np.allclose(adf.sum(-1) * w, 1.0, atol=1e-14) and theta[0] == w / 2 and abs(theta[-1] - (180.0 - w / 2)) < 1e-12
    assert not ref.adf_normalise(np.zeros((2, 2, 5), dtype=np.int64))[0].any()


def test_marginal_rows_of_a_rock_salt_cell_are_the_sums_of_their_specific_rows():
    a = 5.6
    frac = np.array([[0, 0, 0], [0, 0.5, 0.5], [0.5, 0, 0.5], [0.5, 0.5, 0], [0.5, 0, 0], [0, 0.5, 0], [0, 0, 0.5], [0.5, 0.5, 0.5]])
    rank, species = ref.groups(np.array([11] * 4 + [17] * 4), 8)
    assert species == [11, 17]
    rng = np.random.default_rng(0)
    out = ref.angles((frac * a + rng.normal(0, 0.05, (8, 3)))[None], a * np.eye(3), rank, 2, 3.3, n_bins=N_BINS, ls=(4, 6))
    c = out["counts"]
    assert c.shape == (3, 4, N_BINS) and (out["n_neighbors"] == 6).all()
    assert (c[1:, 0] == c[1:, 1:].sum(1)).all() and (c[0] == c[1:].sum(0)).all() and c[0, 0].sum() == 8 * 15
    # the neighbours of a Na are Cl and the other way round: only (centre 1, pair (2, 2)) and (centre 2, pair (1, 1))
    assert c[1, ref.pair_row(2, 2)].sum() == c[2, ref.pair_row(1, 1)].sum() == 4 * 15
    assert not c[1, ref.pair_row(1, 1)].any() and not c[1, ref.pair_row(1, 2)].any() and not c[2, ref.pair_row(2, 2)].any()


def test_structure_factor_of_a_perfect_fcc_crystal_and_of_an_ideal_gas():
    a = 4.0
    cell, base = _fcc(a)
    shifts = np.array([[i, j, k] for i in range(2) for j in range(2) for k in range(2)], dtype=np.float64) * a
    pos = (shifts[:, None, :] + base[None, :, :]).reshape(-1, 3)
    out = ref.structure_factor(pos[None], 2 * cell, np.ones(32, dtype=np.int64), 1, 4.0, 40)
    hkl, s = out["hkl"], out["s_vectors"][0]
    assert len(hkl) > 100 and (hkl[:, 0] >= 0).all() and list(map(tuple, hkl)) == sorted(map(tuple, hkl))
    whole = (hkl % 2 == 0).all(1)  # an index of the conventional cell
    conv = hkl // 2
    bragg = whole & ((conv % 2 == 0).all(1) | (conv % 2 != 0).all(1))
    assert bragg.sum() >= 4 and np.abs(s[bragg] - 32.0).max() < 1e-12 and s[~bragg].max() < 1e-20
    assert np.array_equal(out["s_vectors"][1], s) and out["n_vectors"].sum() == len(hkl)  # one species: row (1, 1) is the total
    # uniform random positions: S = 1 at every q but 0
    rng = np.random.default_rng(3)
    gas = rng.uniform(0, 12.0, (6, 64, 3))
    out = ref.structure_factor(gas, 12.0 * np.eye(3), np.ones(64, dtype=np.int64), 1, 4.0, 40)
    s = out["s_vectors"][0]
    stderr = s.std(ddof=1) / np.sqrt(len(s))
    print(f"ideal gas: {len(s)} vectors, mean S {s.mean():.4f}, standard error {stderr:.4f}")
    assert len(s) > 500 and abs(s.mean() - 1.0) < 3.0 * stderr
    filled = out["n_vectors"] > 0
    assert not out["s"][0][~filled].any() and abs(np.average(out["s"][0][filled], weights=out["n_vectors"][filled]) - s.mean()) < 1e-12


def test_q_l_is_the_rotational_invariant_of_the_spherical_harmonics():
    special = pytest.importorskip("scipy.special")
    rng = np.random.default_rng(5)
    d = rng.normal(size=(9, 3))
    r = np.sqrt((d * d).sum(1))
    polar, azimuth = np.arccos(d[:, 2] / r), np.arctan2(d[:, 1], d[:, 0])
    _, _, c = ref.cosines(d, r)
    for l, got in zip(range(1, 13), ref.q_l(tuple(range(1, 13)), c, len(r))):
        if hasattr(special, "sph_harm_y"):
            y = np.array([special.sph_harm_y(l, m, polar, azimuth).mean() for m in range(-l, l + 1)])
        else:
            y = np.array([special.sph_harm(m, l, azimuth, polar).mean() for m in range(-l, l + 1)])
        want = np.sqrt(4.0 * np.pi / (2 * l + 1) * (np.abs(y) ** 2).sum())
        assert abs(got - want) < 1e-12, (l, got, want)
    assert not ref.q_l((4, 6), c[:0], 0).any() and np.array_equal(ref.q_l((4, 6), c[:0], 1), [1.0, 1.0])


def test_the_inputs_of_the_device_tests_keep_their_margins():
    """The exact comparisons of tests/test_gpu_order.py hold only if no angle lies within ``MARGIN`` bin widths of a bin edge, no
    pair distance within ``MARGIN`` (relatively) of r_cut and no |q| within ``MARGIN`` (relatively) of a shell edge or of q_max:
    the last bits of acos, sqrt and their arguments then move nothing.  The seeds are chosen so; the margins are printed."""
    for kind in ("fixed", "moving"):
        for cuts in ref.R_CUTS:
            for n_bins in ref.ADF_BINS:
                for b, out in enumerate(ref.want_angles(kind, cuts, n_bins)):
                    print(f"{kind} cells, r_cut {ref.R_CUTS[cuts][b]}, {n_bins} bins, structure {b}: {out['triplets']} triplets, at most "
                          f"{out['max_neighbors']} neighbours, angle margin {out['angle_margin']:.2e} bin widths, cutoff margin "
                          f"{out['cut_margin']:.2e}")
                    assert out["angle_margin"] >= ref.MARGIN and out["cut_margin"] >= ref.MARGIN
                    assert 0 < out["max_neighbors"] <= ref.MAX_NEIGHBORS and out["triplets"] > 0
    for which in ("batch", "long"):
        for b, out in enumerate(ref.want_sq(which)):
            print(f"S(q) {which}, structure {b}: {len(out['hkl'])} vectors, margin {out['margin']:.2e}")
            assert out["margin"] >= ref.MARGIN and len(out["hkl"]) > 0
    assert max(ref.hkl_range(ref.CELLS[2], ref.Q_MAX)) <= ref.MAX_HKL
