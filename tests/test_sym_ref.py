"""The restatement of the symmetry search (tests/sym_ref.py) pinned without a GPU: the operation counts, distinct rotations and
crystal systems of the common structure types, the group properties of what it finds, the symmetrisers' defining properties, and
the host logic of ``alignn_amd.symmetry.distinct_miller_indices`` against a brute-force restatement."""

import numpy as np
import pytest

from alignn_amd.symmetry import SymmetryResult, distinct_miller_indices
from tests import pair_ref
from tests import sym_ref as ref

CRYSTALS = ref.crystals()
_CACHE = {}


def _sym(name):
    if name not in _CACHE:
        A, pos, z = CRYSTALS[name][:3]
        _CACHE[name] = ref.find_symmetry(A, pos, z, 1e-3)
    return _CACHE[name]


@pytest.mark.parametrize("name", sorted(CRYSTALS))
def test_counts_and_crystal_system(name):
    want = CRYSTALS[name][3:]
    s = _sym(name)
    assert (s["n_ops"], s["point_group_order"], s["crystal_system"]) == want
    assert s["margin"] > 0.99  # an ideal structure: every comparison is far from symprec
    assert s["n_ops"] == s["n_translations"] * s["point_group_order"]
    assert ((s["translations"] >= 0.0) & (s["translations"] < 1.0)).all()
    keys = [tuple(W.reshape(-1)) for W in s["rotations"]]
    assert keys == sorted(keys)


@pytest.mark.parametrize("name", sorted(CRYSTALS))
def test_operations_form_a_group_and_the_maps_are_permutations(name):
    A, pos, z = CRYSTALS[name][:3]
    s = _sym(name)
    G, n = s["n_ops"], len(pos)
    W, t, m = s["rotations"], s["translations"], s["atom_map"]

    def key(Wg, tg):
        f = tg - np.floor(tg + 1e-9)  # modulo lattice translations, to well below the distance of two operations
        return tuple(Wg.reshape(-1)) + tuple(np.round(f, 6) % 1.0)

    have = {key(W[g], t[g]) for g in range(G)}
    assert len(have) == G
    assert key(np.eye(3, dtype=np.int64), np.zeros(3)) in have
    for g in range(G):
        assert sorted(m[g]) == list(range(n)) and (z[m[g]] == z).all()
        assert abs(ref.det3i(W[g])) == 1
        for h in range(G):  # {W_g | t_g} {W_h | t_h} = {W_g W_h | W_g t_h + t_g}
            assert key(W[g] @ W[h], W[g].astype(np.float64) @ t[h] + t[g]) in have
    # the orbits are the connected classes of the maps
    label = np.arange(n)
    changed = True
    while changed:
        changed = False
        for g in range(G):
            low = np.minimum(label, label[m[g]])
            low[m[g]] = np.minimum(low[m[g]], low)
            changed = changed or not np.array_equal(low, label)
            label = low
    assert np.array_equal(label, s["orbits"])
    # W x_i + t = x_map + shift within symprec
    x = ref.fractional(A, pos)
    for g in range(G):
        res = (ref.apply_w(W[g], x) + t[g]) - (x[m[g]] + s["shifts"][g])
        assert np.sqrt(((res @ A) ** 2).sum(1)).max() <= 1e-3


def test_a_rebased_cell_keeps_the_operations():
    A, pos, z = CRYSTALS["fcc"][:3]
    A2 = ref.rebased(A, [[1, 2, 0], [0, 1, 1], [0, 0, 1]])
    assert max(ref.image_range(A2, 1e-3)) == 8
    s = ref.find_symmetry(A2, pos, z)
    assert (s["n_ops"], s["crystal_system"]) == (48, "cubic") and np.abs(s["rotations"]).max() > 1
    with pytest.raises(ValueError):
        ref.find_symmetry(ref.rebased(A, [[1, 2, 0], [0, 1, 3], [0, 0, 1]]), pos, z)


def test_noise_and_strain_against_symprec():
    A, pos, z = CRYSTALS["diamond"][:3]
    quiet = ref.find_symmetry(A, pos + np.random.default_rng(0).uniform(-1e-4, 1e-4, pos.shape), z)
    loud = ref.find_symmetry(A, pos + np.random.default_rng(0).uniform(-1e-2, 1e-2, pos.shape), z)
    assert quiet["n_ops"] == 48 and loud["n_ops"] < 48
    A, pos, z = CRYSTALS["fcc"][:3]
    strained = A @ np.diag([1.0, 1.0, 1.0 + 1e-5])
    assert ref.find_symmetry(strained, pos, z, 1e-3)["n_ops"] == 48
    tight = ref.find_symmetry(strained, pos, z, 1e-6)
    assert (tight["n_ops"], tight["crystal_system"]) == (16, "tetragonal")


def _result(*names):
    s = [_sym(n) for n in names]
    return SymmetryResult(rotations=[v["rotations"] for v in s], translations=[v["translations"] for v in s],
                          atom_map=[v["atom_map"] for v in s], shifts=[v["shifts"] for v in s], orbits=[v["orbits"] for v in s],
                          n_ops=[v["n_ops"] for v in s], n_translations=[v["n_translations"] for v in s],
                          point_group_order=[v["point_group_order"] for v in s], crystal_system=[v["crystal_system"] for v in s],
                          ns=[v["atom_map"].shape[1] for v in s], symprec=1e-3)


def test_distinct_miller_indices():
    sym = _result("simple_cubic", "hcp", "tetragonal", "triclinic_two_species")
    counts = [[len(h) for h in distinct_miller_indices(sym, m)] for m in (1, 2, 3)]
    assert counts == [[3, 5, 5, 13], [6, 12, 12, 49], [13, 29, 29, 145]]
    got = distinct_miller_indices(sym, 2)
    assert got[0] == [(1, 0, 0), (1, 1, 0), (1, 1, 1), (2, 1, 0), (2, 1, 1), (2, 2, 1)]
    for b, name in enumerate(("simple_cubic", "hcp", "tetragonal", "triclinic_two_species")):
        for merge in (True, False):
            want = ref.distinct_miller_indices(_sym(name)["rotations"], 2, merge)
            assert distinct_miller_indices(_result(name), 2, merge)[0] == want, (name, merge)
    assert len(distinct_miller_indices(_result("triclinic_two_species"), 1, False)[0]) == 26
    with pytest.raises(ValueError):
        distinct_miller_indices(sym, 0)


@pytest.mark.parametrize("name", ["wurtzite", "fcc_2x2x2", "bcc_cube", "triclinic_inversion_pair"])
def test_symmetrised_forces_are_equivariant_and_the_projection_is_idempotent(name):
    A, pos, z = CRYSTALS[name][:3]
    s = _sym(name)
    F = np.random.default_rng(5).normal(size=pos.shape)
    Fs, mag = ref.symmetrize_forces(s, A, F)
    scale = np.abs(F).max()
    for W, m in zip(s["rotations"], s["atom_map"]):
        Q = ref.cartesian_rotation(A, W)
        assert np.abs(Q @ Q.T - np.eye(3)).max() < 1e-12
        assert np.abs(Fs[m] - Fs @ Q.T).max() < 1e-12 * scale  # F'_map = Q F'_i
    again, _ = ref.symmetrize_forces(s, A, Fs)
    assert np.abs(again - Fs).max() < 1e-12 * scale
    S = np.random.default_rng(6).normal(size=(3, 3))
    Ss, _ = ref.symmetrize_stress(s, A, S)
    for W in s["rotations"]:
        Q = ref.cartesian_rotation(A, W)
        assert np.abs(Q.T @ Ss @ Q - Ss).max() < 1e-12
    assert np.abs(ref.symmetrize_stress(s, A, Ss)[0] - Ss).max() < 1e-12
    moved, _ = ref.symmetrize_positions(s, A, pos)
    assert np.abs(moved - pos).max() < 1e-12 * max(1.0, np.abs(pos).max())


def test_symmetrised_positions_restore_a_noisy_crystal():
    A, pos, z = CRYSTALS["diamond"][:3]
    noisy = pos + np.random.default_rng(0).uniform(-1e-4, 1e-4, pos.shape)
    s = ref.find_symmetry(A, noisy, z)
    moved, _ = ref.symmetrize_positions(s, A, noisy)
    d = moved[1] - moved[0]
    assert np.abs(d - pos[1]).max() < 1e-12  # the two atoms a quarter of the diagonal apart again, wherever the pair sits
    assert np.abs(moved - noisy).max() <= 2e-4


def test_forces_of_a_pair_potential_on_a_symmetric_structure_are_left_unchanged():
    A, pos, z = CRYSTALS["wurtzite"][:3]
    _, F, stress = pair_ref.make_efs(4.5)(A, pos)
    assert np.abs(F).max() > 1e-3  # the internal parameter u = 0.375 is not at its equilibrium: forces along c
    s = _sym("wurtzite")
    Fs, _ = ref.symmetrize_forces(s, A, F)
    assert np.abs(Fs - F).max() < 1e-12 * np.abs(F).max()
    Ss, _ = ref.symmetrize_stress(s, A, stress)
    assert np.abs(Ss - stress).max() < 1e-12 * np.abs(stress).max()


# --- the hard structures of tests/test_gpu_symmetry_hard.py, and the checks that restate nothing ---------------------------------
HARD = ref.hard_crystals()
MOVED = ref.moved_copies()
NOISY = ref.noisy_copies()


def _hard(name):
    if name not in _CACHE:
        A, pos, z = (HARD[name] if name in HARD else MOVED[name][1:] if name in MOVED else NOISY[name])[:3]
        _CACHE[name] = ref.find_symmetry(A, pos, z, 1e-3)
    return _CACHE[name]


def _original(name):
    return _hard(name) if name in HARD else _sym(name)


def test_the_hard_crystals_are_the_table_of_their_issue():
    n = {k: len(v[1]) for k, v in HARD.items()}
    assert len(HARD) == 19 and n["zincblende"] == n["cscl"] == n["hBN"] == n["diamond_left"] == 2 and n["rhomb_obtuse"] == 3
    assert (n["quartz"], n["rutile"], n["ortho_C"], n["mono_C2m"], n["wurtzite_shifted"]) == (9, 6, 6, 6, 4)
    assert (n["fluorite_2x2x1"], n["fluorite_2x2x2"]) == (48, 96)
    assert ref.image_range(HARD["hBN"][0], 1e-3) == [3, 3, 1]
    assert np.linalg.det(HARD["diamond_left"][0]) < 0.0 < np.linalg.det(ref.crystals()["diamond"][0])
    A = HARD["rhomb_obtuse"][0]
    assert all(A[i] @ A[j] < 0.0 for i, j in ((0, 1), (0, 2), (1, 2)))
    x = ref.fractional(*HARD["wurtzite_shifted"][:2])
    assert x.min() < -6.0 and x.max() > 4.0
    # the pivot species of fluorite is decided by count, not by number, and is sorted last: 32 pivots from slot 64, two chunks
    z = HARD["fluorite_2x2x2"][2]
    assert z[0] == 20 and (z == 20).sum() == 32 and (z == 9).sum() == 64
    assert sorted({"zincblende", "rocksalt", "cscl", "bcc_cube", "tetragonal", "orthorhombic", "monoclinic", "triclinic_two_species",
                   "rhombohedral"}) == sorted(k for k in HARD if k in CRYSTALS)


@pytest.mark.parametrize("name", sorted(HARD))
def test_hard_counts_and_systems(name):
    s = _hard(name)
    assert (s["n_ops"], s["n_translations"], s["point_group_order"], s["crystal_system"]) == HARD[name][3:]
    assert s["margin"] > 0.99
    assert ((s["translations"] >= 0.0) & (s["translations"] < 1.0)).all()


def test_quartz_has_thirds_and_a_translation_just_below_one():
    t = _hard("quartz")["translations"]
    assert ((t > 1.0 - 1e-12) & (t < 1.0)).any()  # 1 - eps where 0 is meant: what the comparison modulo 1 is for
    thirds = np.abs(t[:, 2] * 3.0 - np.rint(t[:, 2] * 3.0)) < 1e-9
    assert thirds.all() and sorted(np.rint(t[:, 2] * 3.0).astype(int) % 3) == [0, 0, 1, 1, 2, 2]  # the screw 3_1 (or 3_2)
    t = _hard("rutile")["translations"]
    assert (np.abs(t - 0.5) < 1e-12).all(axis=1).sum() == 8  # the 4_2 screw and the n glides


@pytest.mark.parametrize("name", sorted(HARD))
def test_hard_crystals_pass_the_independent_checks(name):
    A, pos, z = HARD[name][:3]
    ref.check_space_group(A, pos, z, _hard(name), 1e-3, exact=1e-9)


@pytest.mark.parametrize("name", sorted(MOVED))
def test_moved_copies_keep_the_group(name):
    orig, A, pos, z, U, perm = MOVED[name]
    N = ref.image_range(A, 1e-3)
    assert max(N) <= ref.MAX_IMAGE_RANGE and abs(ref.det3i(U)) == 1
    assert name != "quartz_moved" or N == [1, 2, 1]
    assert name != "rutile_moved" or N == [2, 5, 6]
    assert sorted(perm) == list(range(len(pos))) and (len(pos) < 3 or not np.array_equal(perm, np.arange(len(pos))))
    s = _hard(name)
    assert s["margin"] >= 0.05, s["margin"]
    ref.check_space_group(A, pos, z, s, 1e-3, exact=1e-9)
    ref.same_group(_original(orig), s, U, perm)
    assert {"quartz_moved": 2, "rutile_moved": 5}.get(name, 1) <= np.abs(s["rotations"]).max()
    assert np.abs(s["shifts"]).max() >= 3  # atoms in other cells


def test_same_group_is_the_conjugation_by_the_basis():
    """The formula of ``same_group`` on one rotation, by hand: the fourfold axis of the tetragonal cell along c, in the basis
    a' = a + b, b' = b, c' = c."""
    U = np.array([[1, 1, 0], [0, 1, 0], [0, 0, 1]])
    W = np.array([[0, -1, 0], [1, 0, 0], [0, 0, 1]])  # a -> b, b -> -a
    A = CRYSTALS["tetragonal"][0]
    A2 = ref.rebased(A, U)
    W2 = ref.inverse_int(U).T @ W @ U.T
    # column i of W holds the coefficients of the image of a_i, so the images of the rows of A are W^T A; Q = A^T W A^-T
    Q, Q2 = ref.cartesian_rotation(A, W), ref.cartesian_rotation(A2, W2)
    assert np.abs(Q - Q2).max() < 1e-14 and np.abs(W.T @ A - A @ Q.T).max() < 1e-14 and np.abs(W2.T @ A2 - A2 @ Q.T).max() < 1e-14
    s = _sym("tetragonal")
    s2 = ref.find_symmetry(A2, *CRYSTALS["tetragonal"][1:3])
    ref.same_group(s, s2, U, np.arange(1))
    with pytest.raises(AssertionError, match="conjugates"):
        ref.same_group(s, s2, np.eye(3, dtype=np.int64), np.arange(1))


def _tampered(s, **changed):
    out = dict(s)
    out.update(changed)
    return out


def test_the_independent_checks_can_fail():
    A, pos, z = HARD["rutile"][:3]
    s = _hard("rutile")
    keep = np.arange(s["n_ops"]) != 5
    dropped = _tampered(s, n_ops=s["n_ops"] - 1, **{f: s[f][keep] for f in ("rotations", "translations", "atom_map", "shifts")})
    with pytest.raises(AssertionError, match="is no member"):
        ref.check_space_group(A, pos, z, dropped, 1e-3)
    amap = s["atom_map"].copy()
    amap[3, [2, 3]] = amap[3, [3, 2]]  # two oxygens exchanged: still a permutation within the species
    with pytest.raises(AssertionError, match="operation 3: an image"):
        ref.check_space_group(A, pos, z, _tampered(s, atom_map=amap), 1e-3)
    orbits = s["orbits"].copy()
    orbits[3] += 1
    with pytest.raises(AssertionError, match="orbits"):
        ref.check_space_group(A, pos, z, _tampered(s, orbits=orbits), 1e-3)
    for field in ("n_translations", "point_group_order"):
        with pytest.raises(AssertionError, match=field):
            ref.check_space_group(A, pos, z, _tampered(s, **{field: s[field] + 1}), 1e-3)
    t = s["translations"].copy()
    t[7, 0] += 0.01  # 0.05 A, past 2 symprec: neither the residual nor the closure holds
    with pytest.raises(AssertionError, match="operation 7"):
        ref.check_space_group(A, pos, z, _tampered(s, translations=t), 1e-3)
    # and a pair of orbits merged is seen through the permutation
    orig, A2, pos2, z2, U, perm = MOVED["rutile_moved"]
    merged = _tampered(_hard("rutile_moved"), orbits=np.zeros(len(pos2), dtype=np.int64))
    with pytest.raises(AssertionError, match="partitions"):
        ref.same_group(s, merged, U, perm)


@pytest.mark.parametrize("name", sorted(NOISY))
def test_noisy_copies_are_restored_to_within_their_noise(name):
    """The preconditions of the device test of the same name: the margin, and that the float64 restatement itself returns the
    copy to within NOISE of the exact crystal and to a fixed point."""
    A, noisy, z, exact = NOISY[name]
    assert 0.0 < ref._norm(noisy - exact).max() <= ref.NOISE
    s = _hard(name)
    assert s["margin"] >= 0.05 and s["n_ops"] == HARD[name[:-len("_noisy")]][3]
    ref.check_space_group(A, noisy, z, s, 1e-3)
    back, _ = ref.symmetrize_positions(s, A, noisy)
    assert ref._norm(back - exact).max() <= ref.NOISE
    again, _ = ref.symmetrize_positions(s, A, back)
    assert np.abs(again - back).max() < 1e-12


def test_a_symprec_that_overflows_the_lattice_operations_but_not_the_candidates():
    """Simple cubic a = 1 at symprec = 0.45: the 6 vectors of length 1 and the 12 of length sqrt 2 are candidates for every axis,
    18 < 256, and 768 > 48 triples keep the metric; no decision is taken near symprec."""
    A = np.eye(3)
    assert ref.image_range(A, 0.45) == [1, 1, 1]
    n = np.array([[i, j, k] for i in (-1, 0, 1) for j in (-1, 0, 1) for k in (-1, 0, 1)], dtype=np.float64)
    assert (np.abs(ref._norm(n) - 1.0) <= 0.45).sum() == 18
    ops, margin = ref.lattice_operations(A, 0.45)
    assert len(ops) == 768 and 0.05 <= margin < 0.1
    for name in ("hBN", "rutile"):  # its neighbours in the device test have nothing between 1e-3 and 0.45 A
        wide, fine = ref.find_symmetry(*HARD[name][:3], 0.45), _hard(name)
        assert wide["margin"] >= 0.01  # (hBN: 0.017, some 8e-3 A off a decision, thirteen orders above rounding)
        assert all(np.array_equal(wide[f], fine[f]) for f in ("rotations", "translations", "atom_map", "shifts", "orbits"))


def test_the_crystal_at_the_atom_limit():
    A, pos, z = ref.crystal_at_the_atom_limit()
    assert len(pos) == 1024 and (z == 8).sum() == 1 and z[0] == 8 and np.argsort(z, kind="stable")[-1] == 0
    assert ref.image_range(A, 1e-3) == [2, 2, 1]
    ops, margin = ref.lattice_operations(A, 1e-3)
    assert len(ops) == 16 and margin > 0.99


def test_noise_near_symprec_gives_no_group():
    """The limit stated in ``find_symmetry``'s docstring: each operation is decided on its own, so with noise of 4e-4 A at a
    symprec of 1e-3 A what is accepted does not close.  The margin says so beforehand, and ``check_space_group`` afterwards."""
    A, pos, z = HARD["fluorite_2x2x2"][:3]
    s = ref.find_symmetry(A, pos + np.random.default_rng(0).uniform(-4e-4, 4e-4, pos.shape), z, 1e-3)
    assert s["margin"] < 0.05 and (s["n_ops"], s["point_group_order"], s["n_translations"]) == (14, 12, 2)
    with pytest.raises(AssertionError):
        ref.check_space_group(A, pos, z, s, 1e-3)
