"""The numpy restatement of the local structure analysis (tests/local_ref.py) against what is known from first principles: the
signatures and classes of the perfect crystals in their smallest cells, their q_l and w_l, the 3j symbols, the adaptive rule on
scaled cells; the host tables of alignn_amd/local_order.py against the same; and the margins of the inputs of the device tests.
No GPU."""

import numpy as np
import pytest

from alignn_amd import local_order
from tests import local_ref as ref
from tests.traj_ref import groups

ONE = lambda n: groups(np.ones(n, dtype=np.int64), n)[0]


@pytest.mark.parametrize("name,nb,signatures", [("fcc", 12, [12, 0, 0, 0, 0]), ("hcp", 12, [6, 6, 0, 0, 0]), ("bcc", 14, [0, 0, 6, 0, 8])])
def test_perfect_crystals_in_their_smallest_cells(name, nb, signatures):
    """Four, two and two atoms: most neighbours are images of the cell's own atoms, an atom's own images among them."""
    (C, pos), cut, cls = ref.CRYSTALS[name]
    w = ref.cna(pos[None], C, ONE(len(pos)), 1, cut)
    assert (w["n_neighbors"] == nb).all() and (w["structure"] == cls).all() and (w["signature_counts"] == signatures).all()
    assert (w["counts"][:, 0, cls] == len(pos)).all() and w["counts"].sum() == 2 * len(pos)  # (group 0 and the one species)
    assert w["cut_margin"] > 0.1 and w["bond_margin"] > 0.1


def test_a_one_atom_cell_classifies_through_its_own_images():
    a = ref.A_FCC
    C = a * np.array([[0.0, 0.5, 0.5], [0.5, 0.0, 0.5], [0.5, 0.5, 0.0]])
    w = ref.cna(np.zeros((1, 1, 3)), C, ONE(1), 1, ref.CUT_FCC)
    assert w["structure"].tolist() == [[ref.FCC]] and w["n_neighbors"].tolist() == [[12]]
    C = ref.A_BCC * np.array([[-0.5, 0.5, 0.5], [0.5, -0.5, 0.5], [0.5, 0.5, -0.5]])
    w = ref.cna(np.zeros((1, 1, 3)), C, ONE(1), 1, ref.CUT_BCC)
    assert w["structure"].tolist() == [[ref.BCC]] and w["n_neighbors"].tolist() == [[14]]


def test_the_centre_of_an_icosahedron():
    (C, pos), cut, _ = ref.CRYSTALS["ico"]
    assert len(pos) == 13 and np.allclose(np.linalg.norm(pos[1:] - pos[0], axis=1), ref.R_ICO)
    for adaptive, rc in ((False, cut), (True, 4.2)):
        w = ref.cna(pos[None], C, ONE(13), 1, rc, adaptive)
        assert w["structure"][0].tolist() == [ref.ICO] + [ref.OTHER] * 12
        assert w["signature_counts"][0, 0].tolist() == [0, 0, 0, 12, 0] and w["n_neighbors"][0].tolist() == [12] + [6] * 12


def test_n_lcb_counts_the_bonds_of_the_largest_component():
    """Two disjoint bonds give 1, a chain of two bonds 2, a ring of k bonds k: the common neighbours of entry 0 laid out by hand."""
    def lcb(points, rc=1.1):
        d = np.array([[0.0, 0.0, 0.0]] + points)
        return ref.signatures(d, np.arange(len(d)), rc)[0][0]
    far = 0.9
    assert lcb([[far, 0, 0], [far, 1, 0], [-far, 0, 0], [-far, 1, 0]], rc=1.4) == (4, 2, 1)
    assert lcb([[0, 0, 1.0], [0, 0.9, 0.5], [0, -0.9, 0.5]]) == (3, 2, 2)
    ring = [[np.cos(t), np.sin(t), 0.3] for t in 2 * np.pi * np.arange(5) / 5]  # edge 1.18, the next distance 1.90
    assert lcb(ring, rc=1.3) == (5, 5, 5)


@pytest.mark.parametrize("name", ["fcc", "hcp", "bcc", "ico"])
def test_q_and_w_of_the_perfect_first_shells(name):
    """Six-digit constants, recomputed with scipy's harmonics and sympy's 3j: 5e-6 absolute.  On the periodic crystals every atom
    has the same q_lm, so the averaged forms are the plain ones."""
    (C, pos), cut, _ = ref.CRYSTALS[name]
    w = ref.bond_order(pos[None], C, ONE(len(pos)), 1, cut, (4, 6))
    q4, q6, w4, w6 = ref.CONSTANTS[name]
    rows = slice(0, 1) if name == "ico" else slice(None)  # (the centre)
    for got, want in ((w["q"][0, rows, 0], q4), (w["q"][0, rows, 1], q6), (w["w"][0, rows, 0], w4), (w["w"][0, rows, 1], w6)):
        if want is not None:
            assert np.abs(got - want).max() <= 5e-6, (name, got, want)
    if name != "ico":
        assert np.abs(w["q_avg"] - w["q"]).max() < 1e-13 and np.abs(w["w_avg"] - w["w"]).max() < 1e-11
        assert np.abs(w["s_avg"] - w["s"]).max() < 1e-13 and np.abs(w["t_avg"] - w["t"]).max() < 1e-13


def test_harmonics_against_scipy():
    special = pytest.importorskip("scipy.special")
    rng = np.random.default_rng(0)
    d = rng.normal(size=(20, 3))
    r = np.sqrt((d * d).sum(1))
    theta, phi = np.arccos(d[:, 2] / r), np.arctan2(d[:, 1], d[:, 0])
    for l in (1, 4, 6, 12):
        got = ref.ylm(l, d, r)
        for m in range(l + 1):
            want = special.sph_harm_y(l, m, theta, phi) if hasattr(special, "sph_harm_y") else special.sph_harm(m, l, phi, theta)
            assert np.abs(got[:, m] - want).max() < 1e-12, (l, m)
    for l in (1, 4, 6, 12):  # (Y_l0 at the pole is the driver's norm itself)
        assert local_order.ylm_norms()[l, 0] == ref.ylm(l, np.array([[0.0, 0.0, 1.0]]), np.ones(1))[0, 0].real


@pytest.mark.parametrize("l", [1, 4, 6, 12])
def test_three_j_tables(l):
    """Orthogonality: sum over (m1, m2) of (l l l; m1 m2 m3)^2 = 1 / (2l + 1) for every m3; the symmetry under a swap of two
    columns; the driver's table and the restatement's are the same numbers."""
    table, mine = ref.three_j(l), local_order.wigner_3j_table(l)
    assert np.abs(table - mine).max() <= 4 * 2.0 ** -53
    for t in (table, mine):
        for m3 in range(-l, l + 1):
            total = sum(t[m1 + l, m2 + l] ** 2 for m1 in range(-l, l + 1) for m2 in range(-l, l + 1) if m1 + m2 + m3 == 0)
            assert abs(total - 1.0 / (2 * l + 1)) < 1e-14, (l, m3)
        assert np.abs(t - (-1.0) ** (3 * l) * t.T).max() < 1e-15
    assert table.shape == (2 * l + 1, 2 * l + 1) and not mine.flags.writeable


@pytest.mark.parametrize("l", [4, 6, 12])
def test_three_j_tables_against_sympy(l):
    wigner = pytest.importorskip("sympy.physics.wigner")
    mine = local_order.wigner_3j_table(l)
    for m1 in range(-l, l + 1):
        for m2 in range(-l, l + 1):
            m3 = -(m1 + m2)
            want = float(wigner.wigner_3j(l, l, l, m1, m2, m3).evalf(30)) if abs(m3) <= l else 0.0
            assert abs(mine[m1 + l, m2 + l] - want) <= 1e-15, (l, m1, m2)


def test_adaptive_cna_follows_the_scale_of_the_cell():
    """One search radius, 4.2 A, for the fcc, hcp and bcc cells scaled by 0.92 and 1.08: the classes of the unscaled cells.  With
    the one fixed cutoff that classifies all three unscaled cells, 3.3 A, the bcc cell scaled by 1.08 is not classified: its second
    shell, 3.456 A, has moved beyond the cutoff and 8 neighbours are left.  (With each cell's own midway cutoff all six scaled
    cells still classify: those windows are +-17 % wide.)"""
    for name in ("fcc", "hcp", "bcc"):
        (C, pos), cut, cls = ref.CRYSTALS[name]
        rank = ONE(len(pos))
        assert (ref.cna(pos[None], C, rank, 1, 3.3)["structure"] == cls).all()
        for scale in (0.92, 1.08):
            w = ref.cna(scale * pos[None], scale * C, rank, 1, 4.2, adaptive=True)
            assert (w["structure"] == cls).all() and w["max_neighbors"] <= ref.MAX_NEIGHBORS, (name, scale)
            assert (ref.cna(scale * pos[None], scale * C, rank, 1, cut)["structure"] == cls).all()
    (C, pos), _, _ = ref.CRYSTALS["bcc"]
    fixed = ref.cna(1.08 * pos[None], 1.08 * C, ONE(2), 1, 3.3)
    assert (fixed["structure"] == ref.OTHER).all() and (fixed["n_neighbors"] == 8).all()


def test_adaptive_stages_with_too_few_entries_do_not_match():
    (C, pos), _, _ = ref.CRYSTALS["bcc"]
    w = ref.cna(pos[None], C, ONE(2), 1, 3.0, adaptive=True)  # 8 entries
    assert (w["n_neighbors"] == 8).all() and not w["structure"].any() and not w["signature_counts"].any()
    (C, pos), _, _ = ref.CRYSTALS["fcc"]
    w = ref.cna(pos[None], C, ONE(4), 1, 3.0, adaptive=True)  # 12 entries: stage 12 decides, stage 14 is not needed
    assert (w["structure"] == ref.FCC).all() and (w["signature_counts"] == [12, 0, 0, 0, 0]).all()


CASES = [("fixed", "one", False), ("fixed", "each", False), ("moving", "each", False), ("moving", "one", False), ("fixed", "wide", True),
         ("moving", "wide", True)]


def test_the_inputs_of_the_device_tests_keep_their_margins():
    """No pair distance within 1e-9 (relatively) of r_cut, no bond distance within 1e-9 of r_c, and for the adaptive rule no tie
    between the 12th and 13th or the 14th and 15th distance, in the random structures of every case of tests/test_gpu_local.py;
    no atom has more than 64 entries.  The perfect crystals are ties by construction (the six second neighbours of bcc): which 12
    of its 14 the first stage takes decides nothing, it matches with none."""
    assert ref.SIZES == [1, 5, 70, 4, 2, 2, 13, 32] and ref.PTR[-1] == 129
    for kind, cuts, adaptive in CASES:
        for b, w in enumerate(ref.want_cna(kind, cuts, adaptive)):
            assert w["max_neighbors"] <= ref.MAX_NEIGHBORS, (kind, cuts, b)
            if b in ref.RANDOM:
                assert min(w["cut_margin"], w["bond_margin"], w["gap_margin"]) >= ref.MARGIN, (kind, cuts, adaptive, b)
    sel = ref.want_cna("moving", "one", False, (1,))
    assert all(min(sel[b]["cut_margin"], sel[b]["bond_margin"]) >= ref.MARGIN for b in ref.RANDOM)
    for kind, cuts in (("fixed", "one"), ("moving", "each"), ("moving", "wide")):
        for ls in ref.LS:
            for b, w in enumerate(ref.want_bond(kind, cuts, ls)):
                assert w["cut_margin"] >= ref.MARGIN or b not in ref.RANDOM


def test_the_noisy_supercell_is_mostly_fcc_but_not_wholly():
    """N(0, 0.094 A) on a 32-atom fcc supercell (nearest neighbours at 2.546 A), three frames, the midway cutoff."""
    w = ref.want_cna("fixed", "each", False)[7]
    n_fcc, n_other = int((w["structure"] == ref.FCC).sum()), int((w["structure"] == ref.OTHER).sum())
    assert w["structure"].size == 96 and n_fcc + n_other == 96 and n_fcc >= 0.9 * 96 and n_other >= 1, (n_fcc, n_other)
    a = ref.want_cna("fixed", "wide", True)[7]
    assert int((a["structure"] == ref.FCC).sum()) >= n_fcc  # (the adaptive rule loses no atom here)


def test_the_crystals_of_the_device_batch_give_their_classes():
    for kind, cuts, adaptive in (("fixed", "one", False), ("fixed", "each", False), ("moving", "each", False), ("fixed", "wide", True),
                                 ("moving", "wide", True)):
        want = ref.want_cna(kind, cuts, adaptive)
        for b, name in ((3, "fcc"), (4, "hcp"), (5, "bcc")):
            assert (want[b]["structure"] == ref.CRYSTALS[name][2]).all(), (kind, cuts, name)
        assert (want[6]["structure"][:, 0] == ref.ICO).all() and not want[6]["structure"][:, 1:].any()
    moved = ref.want_cna("moving", "one", False)[5]["structure"]  # 3.3 A and the bcc cell scaled by 1.08: the third frame
    assert (moved[:2] == ref.BCC).all() and (moved[2] == ref.OTHER).all()


def test_driver_refusals_that_need_no_gpu():
    import torch
    for fn in (local_order.cna, local_order.bond_order):
        with pytest.raises(TypeError, match="float64 tensor on the GPU"):
            fn(torch.zeros(1, 1, 3, dtype=torch.float64), torch.eye(3, dtype=torch.float64)[None], [1], r_cut=3.0)
    for bad in ((), (4, 4), (0,), (13,), (1, 2, 3, 4, 5), (4.0,), 6):
        with pytest.raises(ValueError, match="ls"):
            local_order.bond_order(None, None, [1], r_cut=3.0, ls=bad)
    with pytest.raises(ValueError, match="average"):
        local_order.bond_order(None, None, [1], r_cut=3.0, average=1)
    with pytest.raises(ValueError, match="adaptive"):
        local_order.cna(None, None, [1], r_cut=3.0, adaptive="yes")
