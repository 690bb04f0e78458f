"""The symmetry search and the symmetrisers on the device (csrc/symmetry.hip, alignn_amd/symmetry.py) against the restatement of
tests/sym_ref.py, ten structures in one call: (a) rotations, atom maps, lattice shifts, orbits, counts and crystal systems equal
the restatement's, the translations agree modulo 1; every structure alone, and the batch rotated, give the batch's bits; a cell
past the image range raises and leaves the others' results intact; (b) the symmetrisers under a bound derived from the number
of terms; (c) ``vacancy_formation(site_labels="auto")`` on the pair potential of tests/pair_ref.py.

The precondition of (a): a decision taken exactly at symprec may fall either way on two machines, so the restatement reports the
smallest |value - symprec| / symprec over every comparison it makes (rejected candidates and the atoms after the first miss
included) and the inputs are chosen so that it is at least 0.05; that is asserted before anything is compared."""

import numpy as np
import pytest
import torch

from alignn_amd import find_symmetry, symmetrize_forces, symmetrize_positions, symmetrize_stress, vacancy_formation
from tests import pair_ref
from tests import sym_ref as ref
from tests.sim_gpu import DEV, _t
from tests.sym_ref import same_as_restated as _same_as_restated, same_bits as _same_bits

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -53
_CACHE = {}


def _structures():
    """name -> (cell, positions, species): one of every case the kernels can go wrong at."""
    if "structures" not in _CACHE:
        C = ref.crystals()
        fcc, diamond = C["fcc"][:3], C["diamond"][:3]
        noise = lambda amp: diamond[1] + np.random.default_rng(0).uniform(-amp, amp, diamond[1].shape)
        _CACHE["structures"] = {
            "one_atom": C["simple_cubic"][:3],
            "inversion_pair": C["triclinic_inversion_pair"][:3],
            "wurtzite": C["wurtzite"][:3],  # species [30, 30, 16, 16]: the pivot species starts at atom 2
            "hcp": C["hcp"][:3],
            "fcc_rebased": (ref.rebased(fcc[0], [[1, 2, 0], [0, 1, 1], [0, 0, 1]]), fcc[1], fcc[2]),  # image range 3, 8, 8
            "fcc_strained": (fcc[0] @ np.diag([1.0, 1.0, 1.0 + 1e-5]), fcc[1], fcc[2]),
            "diamond_noise_1e-4": (diamond[0], noise(1e-4), diamond[2]),
            "diamond_noise_1e-2": (diamond[0], noise(1e-2), diamond[2]),
            "fcc_2x2x2": C["fcc_2x2x2"][:3],  # 8 pure translations
            "diamond_96": ref.supercell(*ref.diamond_cube(), (3, 2, 2)),  # one species: lanes, waves and pivots beyond one tile
        }
    return _CACHE["structures"]


def _want(name, symprec=1e-3):
    key = ("want", name, symprec)
    if key not in _CACHE:
        A, pos, z = _structures()[name]
        _CACHE[key] = ref.find_symmetry(A, pos, z, symprec)
    return _CACHE[key]


def _find(names, symprec=1e-3):
    S = _structures()
    return find_symmetry([S[n][0] for n in names], [S[n][1] for n in names], [S[n][2] for n in names], symprec=symprec, device=DEV)


def _batch():
    if "batch" not in _CACHE:
        _CACHE["batch"] = _find(list(_structures()))
    return _CACHE["batch"]


# --- (a) the search --------------------------------------------------------------------------------------------------------------
def test_the_batch_equals_the_restatement():
    names = list(_structures())
    res = _batch()
    assert res.ns == [1, 2, 4, 2, 1, 1, 2, 2, 8, 96]
    worst = 0.0
    for b, name in enumerate(names):
        want = _want(name)
        worst = max(worst, _same_as_restated(res, b, want, name))
        print(f"{name}: {want['n_ops']} operations, {want['point_group_order']} rotations, {want['crystal_system']}, margin "
              f"{want['margin']:.3f}")
    print(f"largest deviation of a translation modulo 1: {worst:.2e}")
    got = dict(zip(names, zip(res.n_ops, res.crystal_system)))
    assert got["wurtzite"] == (12, "hexagonal") and got["hcp"] == (24, "hexagonal") and got["fcc_rebased"] == (48, "cubic")
    assert got["fcc_strained"] == (48, "cubic") and got["diamond_noise_1e-4"] == (48, "cubic") and got["diamond_noise_1e-2"][0] < 48
    assert got["fcc_2x2x2"] == (384, "cubic") and got["diamond_96"] == (768, "tetragonal") and got["one_atom"] == (48, "cubic")
    assert int(res.rotations[names.index("fcc_rebased")].abs().max()) > 1  # the cell is not reduced


def test_a_tighter_symprec_sees_the_strain():
    names = ["fcc_strained", "hcp"]
    res = _find(names, symprec=1e-6)
    for b, name in enumerate(names):
        _same_as_restated(res, b, _want(name, 1e-6), (name, 1e-6))
    assert (res.n_ops[0], res.crystal_system[0]) == (16, "tetragonal") and res.n_ops[1] == 24


def test_every_structure_alone_and_the_batch_rotated_give_the_batchs_bits():
    names = list(_structures())
    res = _batch()
    for b, name in enumerate(names):
        assert _same_bits(_find([name]), 0, res, b), name
    rolled = names[3:] + names[:3]
    other = _find(rolled)
    for b, name in enumerate(rolled):
        assert _same_bits(other, b, res, names.index(name)), name


def test_a_cell_past_the_image_range_raises_and_leaves_the_others_intact():
    S = _structures()
    fcc = S["fcc_strained"]
    far = (ref.rebased(ref.crystals()["fcc"][0], [[1, 2, 0], [0, 1, 3], [0, 0, 1]]), fcc[1], fcc[2])
    assert max(ref.image_range(far[0], 1e-3)) > 8
    trio = [S["hcp"], far, S["wurtzite"]]
    with pytest.raises(ValueError, match="structure 1") as err:
        find_symmetry([s[0] for s in trio], [s[1] for s in trio], [s[2] for s in trio], device=DEV)
    part, res, names = err.value.result, _batch(), list(S)
    assert part.n_ops == [24, 0, 12] and part.rotations[1].shape == (0, 3, 3) and part.orbits[1].tolist() == [0]
    assert _same_bits(part, 0, res, names.index("hcp")) and _same_bits(part, 2, res, names.index("wurtzite"))
    with pytest.raises(ValueError, match="1025 atoms"):
        find_symmetry([np.eye(3) * 40.0], [np.zeros((1025, 3))], device=DEV)
    # a symprec of several cells: 4.5 cells of range, more lattice vectors within it of |a_i| than the candidate list holds
    with pytest.raises(ValueError, match="structure 0: more than 256 candidate") as err:
        find_symmetry([np.eye(3)], [np.zeros((1, 3))], symprec=3.5, device=DEV)
    assert err.value.result.n_ops[0] == 0


def test_more_candidates_than_a_workgroup_has_threads():
    """343 atoms of one species, a 7 x 7 x 7 supercell of simple cubic: 343 candidate translations for each of the 48 lattice
    operations, over 22 workgroups each, all accepted.  What must come out follows from the structure alone: 48 x 343 operations,
    every map a permutation, one orbit, and W x_i + t = x_map + shift to rounding."""
    A, pos, z = ref.supercell(3.0 * np.eye(3), np.zeros((1, 3)), np.array([7]), (7, 7, 7))
    res = find_symmetry([A], [pos], [z], device=DEV)
    n, G = 343, 48 * 343
    assert (res.n_ops[0], res.n_translations[0], res.point_group_order[0], res.crystal_system[0]) == (G, n, 48, "cubic")
    amap, W, t, sh = res.atom_map[0].long(), res.rotations[0].double(), res.translations[0], res.shifts[0].double()
    assert torch.equal(amap.sort(dim=1).values, torch.arange(n, device=DEV).expand(G, n)) and not res.orbits[0].any()
    keys = ((res.rotations[0].view(G, 9).long() + 8) * (17 ** torch.arange(8, -1, -1, device=DEV))).sum(1)
    assert bool((keys[1:] >= keys[:-1]).all()) and keys.unique().numel() == 48
    x = _t(pos @ np.linalg.inv(A))
    image = torch.einsum("grc,ic->gir", W, x) + t[:, None, :]
    assert (image - (x[amap] + sh)).abs().max().item() < 1e-12
    # within one W the operations follow the atom the pivot atom (atom 0) is sent to
    first = amap[:, 0].reshape(48, n)
    assert torch.equal(first, torch.arange(n, device=DEV).expand(48, n))


# --- (b) the symmetrisers --------------------------------------------------------------------------------------------------------
def test_symmetrisers_agree_with_the_restatement():
    """A sum of G terms in the stored order on both sides: each lies within (G + 8) x 2^-53 of the sum of the magnitudes of its
    terms (G - 1 additions and a handful of roundings per term), so the two within twice that; the mean divides both by G.  The
    positions are returned Cartesian: the bound of the fractional mean is carried through |A|, whose three products and two
    additions the + 8 also covers.  Measured on an MI355X: printed (the two sides do the same operations in the same order)."""
    S, names, res = _structures(), list(_structures()), _batch()
    rng = np.random.default_rng(9)
    lats = [S[n][0] for n in names]
    forces = [rng.normal(size=S[n][1].shape) for n in names]
    stress = rng.normal(size=(len(names), 3, 3))
    got_f = symmetrize_forces(res, lats, forces)
    got_s = symmetrize_stress(res, _t(np.array(lats)), _t(stress))
    got_p = symmetrize_positions(res, lats, [S[n][1] for n in names])
    packed = symmetrize_forces(res, lats, _t(np.concatenate(forces)))
    assert torch.equal(packed, torch.cat(got_f))  # a packed tensor and B arrays: the same launch
    worst = {"forces": 0.0, "stress": 0.0, "positions": 0.0}
    for b, name in enumerate(names):
        want = _want(name)
        G, A = want["n_ops"], S[name][0]
        bound = 2.0 * (G + 8) * EPS / G
        for what, got, (exp, mag) in (("forces", got_f[b], ref.symmetrize_forces(want, A, forces[b])),
                                      ("stress", got_s[b], ref.symmetrize_stress(want, A, stress[b])),
                                      ("positions", got_p[b], ref.symmetrize_positions(want, A, S[name][1]))):
            if what == "positions":
                mag = mag @ np.abs(A)
            dev = np.abs(got.cpu().numpy() - exp)
            assert mag.min() > 0.0 or (dev[mag == 0.0] == 0.0).all()
            assert (dev <= bound * mag).all(), (name, what, (dev / np.maximum(bound * mag, 1e-300)).max())
            worst[what] = max(worst[what], float((dev / np.maximum(mag / G, 1e-300)).max()))
    print("largest deviations in units of the mean magnitude of a term: " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()))
    # what a projection is for: equivariant, idempotent, and the noise of a noisy crystal is gone
    again = symmetrize_forces(res, lats, got_f)
    for b in range(len(names)):
        assert (again[b] - got_f[b]).abs().max().item() <= 1e-12
    b = names.index("diamond_noise_1e-4")
    d = (got_p[b][1] - got_p[b][0]).cpu().numpy()
    assert np.abs(d - ref.crystals()["diamond"][1][1]).max() < 1e-12


# --- (c) the classes of sites of a vacancy calculation ---------------------------------------------------------------------------
def test_vacancy_formation_takes_its_classes_from_the_symmetry():
    A, pos, z = ref.crystals(4.0)["rocksalt"][:3]
    kw = dict(supercell=(2, 2, 2), steps=0, forces_fn=pair_ref.make_forces_fn(3.4, stress=True), device=DEV)
    auto = vacancy_formation(None, [A], [pos], site_labels="auto", species=[z], symprec=1e-3, **kw)
    assert auto.labels[0].tolist() == [0, 1] and auto.multiplicity[0].tolist() == [1, 1] and auto.removed_atom[0].tolist() == [0, 1]
    hand = vacancy_formation(None, [A], [pos], site_labels=[np.array([0, 1])], **kw)
    assert auto.e_bulk[0] == hand.e_bulk[0] and np.array_equal(auto.e_defect[0], hand.e_defect[0])
    assert np.array_equal(auto.formation_energy[0], hand.formation_energy[0])
    # without species the two sites of the (then simple cubic) lattice are one class
    alike = vacancy_formation(None, [A], [pos], site_labels="auto", **kw)
    assert alike.labels[0].tolist() == [0] and alike.multiplicity[0].tolist() == [2]
    with pytest.raises(ValueError, match="auto"):
        vacancy_formation(None, [A], [pos], site_labels="wyckoff", **kw)
