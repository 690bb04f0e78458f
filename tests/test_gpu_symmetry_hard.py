"""The symmetry search and the symmetrisers on the device (csrc/symmetry.hip) on the structures the kernels can be wrong at
without tests/test_gpu_symmetry.py noticing: every branch of the crystal-system rule, screws and glides with translations of
thirds, a pivot species chosen by count and sorted last with more than one chunk of pivots, left-handed and obtuse cells, atoms
many cells outside [0, 1), the same crystal in another basis, orientation, origin and atom order, 1024 atoms, and more lattice
operations than the list holds.  All of ``ref.hard_crystals()`` and ``ref.moved_copies()`` in one call:

(a) against the restatement of tests/sym_ref.py, integers bit for bit, translations modulo 1, with the counts of the table;
(b) ``ref.check_space_group`` and ``ref.same_group`` on the device's own arrays: they restate nothing of the search;
(c) every structure alone, and the batch rotated, give the batch's bits;
(d) 1024 atoms; (e) the lattice-operation overflow; (f) the symmetrisers: the term-count bound against the restatement, and what
a projection satisfies under every operation, on the device's outputs alone.

The precondition of (a), as in tests/test_gpu_symmetry.py: the restatement's margin is at least 0.05, asserted first."""

import numpy as np
import pytest

from alignn_amd import find_symmetry, symmetrize_forces, symmetrize_positions, symmetrize_stress
from tests import sym_ref as ref
from tests.sim_gpu import DEV, _t
from tests.sym_ref import same_as_restated as _same_as_restated, same_bits as _same_bits

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -53
SYMPREC = 1e-3
EXACT = 1e-9  # A: the residual of W x_i + t = x_map + shift on an exact crystal (ref.check_space_group derives it)
_CACHE = {}

# name: (atoms, operations, pure translations, distinct rotations, system), the table of the issue, literally
TABLE = {
    "zincblende": (2, 24, 1, 24, "cubic"), "rocksalt": (2, 48, 1, 48, "cubic"), "cscl": (2, 48, 1, 48, "cubic"),
    "bcc_cube": (2, 96, 2, 48, "cubic"), "tetragonal": (1, 16, 1, 16, "tetragonal"), "orthorhombic": (1, 8, 1, 8, "orthorhombic"),
    "monoclinic": (1, 4, 1, 4, "monoclinic"), "triclinic_two_species": (2, 1, 1, 1, "triclinic"),
    "rhombohedral": (1, 12, 1, 12, "trigonal"), "hBN": (2, 12, 1, 12, "hexagonal"), "quartz": (9, 6, 1, 6, "trigonal"),
    "rutile": (6, 16, 1, 16, "tetragonal"), "ortho_C": (6, 16, 2, 8, "orthorhombic"), "mono_C2m": (6, 8, 2, 4, "monoclinic"),
    "rhomb_obtuse": (3, 12, 1, 12, "trigonal"), "diamond_left": (2, 48, 1, 48, "cubic"),
    "wurtzite_shifted": (4, 12, 1, 12, "hexagonal"), "fluorite_2x2x1": (48, 256, 16, 16, "tetragonal"),
    "fluorite_2x2x2": (96, 1536, 32, 48, "cubic"), "triclinic_inversion_pair": (2, 2, 1, 2, "triclinic"),
}


def _structures():
    """name -> (cell, positions, species): the hard crystals, the original of the fifth moved copy, the moved copies."""
    if "structures" not in _CACHE:
        S = {k: v[:3] for k, v in ref.hard_crystals().items()}
        S["triclinic_inversion_pair"] = ref.crystals()["triclinic_inversion_pair"][:3]
        S.update({k: v[1:4] for k, v in ref.moved_copies().items()})
        _CACHE["structures"] = S
    return _CACHE["structures"]


def _want(name):
    if ("want", name) not in _CACHE:
        _CACHE["want", name] = ref.find_symmetry(*_structures()[name], SYMPREC)
    return _CACHE["want", name]


def _find(structures, symprec=SYMPREC):
    return find_symmetry([s[0] for s in structures], [s[1] for s in structures], [s[2] for s in structures], symprec=symprec, device=DEV)


def _batch():
    if "batch" not in _CACHE:
        _CACHE["batch"] = _find(list(_structures().values()))
    return _CACHE["batch"]


def _numpy(res, b):
    """The device's arrays of structure b under the names of the restatement's dict."""
    out = {f: getattr(res, f)[b].cpu().numpy() for f in ("rotations", "translations", "atom_map", "shifts", "orbits")}
    out.update({f: getattr(res, f)[b] for f in ("n_ops", "n_translations", "point_group_order", "crystal_system")})
    return out


# --- (a) against the restatement -------------------------------------------------------------------------------------------------
def test_the_hard_batch_equals_the_restatement():
    S, names, res = _structures(), list(_structures()), _batch()
    assert len(names) == 25 and res.ns == [len(S[n][1]) for n in names]
    worst = 0.0
    for b, name in enumerate(names):
        want = _want(name)
        dev = _same_as_restated(res, b, want, name)
        worst = max(worst, dev)
        print(f"{name}: {res.n_ops[b]} operations, {res.n_translations[b]} translations, {res.point_group_order[b]} rotations, "
              f"{res.crystal_system[b]}, margin {want['margin']:.3f}, |W| <= {int(res.rotations[b].abs().max())}, |shift| <= "
              f"{int(res.shifts[b].abs().max())}, translations modulo 1 off by {dev:.2e}")
        table = TABLE[ref.moved_copies()[name][0] if name.endswith("_moved") else name]
        assert (res.ns[b], res.n_ops[b], res.n_translations[b], res.point_group_order[b], res.crystal_system[b]) == table, name
    print(f"(a) largest deviation of a translation modulo 1: {worst:.2e}")
    # the cases are what they are meant to be: every system, entries of W above 1, atoms in other cells, 1 - eps for 0
    assert set(res.crystal_system) == set(ref.SYSTEMS)
    assert int(res.rotations[names.index("rutile_moved")].abs().max()) == 5 and int(res.rotations[names.index("quartz_moved")].abs().max()) == 2
    assert int(res.shifts[names.index("wurtzite_shifted")].abs().max()) >= 7 and int(res.shifts[names.index("rutile_moved")].abs().max()) >= 10
    t = res.translations[names.index("quartz")]
    assert bool(((t > 1.0 - 1e-12) & (t < 1.0)).any())


# --- (b) what needs no restatement -----------------------------------------------------------------------------------------------
def test_the_devices_operations_are_space_groups():
    names, res = list(_structures()), _batch()
    for b, name in enumerate(names):
        ref.check_space_group(*_structures()[name], _numpy(res, b), SYMPREC, exact=EXACT)
    print(f"(b) check_space_group passes on {len(names)} structures, the residual of W x + t = x_map + shift at most {EXACT} A")


def test_a_crystal_described_differently_has_the_same_group():
    names, res = list(_structures()), _batch()
    for name, (orig, _, _, _, U, perm) in ref.moved_copies().items():
        ref.same_group(_numpy(res, names.index(orig)), _numpy(res, names.index(name)), U, perm)
    print(f"(b) same_group passes on {len(ref.moved_copies())} pairs")


# --- (c) batch invariance --------------------------------------------------------------------------------------------------------
def test_every_hard_structure_alone_and_the_batch_rotated_give_the_batchs_bits():
    S, names, res = _structures(), list(_structures()), _batch()
    for b, name in enumerate(names):
        assert _same_bits(_find([S[name]]), 0, res, b), name
    rolled = names[7:] + names[:7]
    other = _find([S[n] for n in rolled])
    for b, name in enumerate(rolled):
        assert _same_bits(other, b, res, names.index(name)), name


# --- (d) the limit of 1024 atoms -------------------------------------------------------------------------------------------------
def test_a_structure_of_1024_atoms():
    """Simple cubic 8 x 8 x 16 with one atom substituted: the operations are those of the tetragonal supercell that fix that atom
    (no translation moves the only atom of its species), 4/mmm about it: 16, one with W = 1."""
    A, pos, z = ref.crystal_at_the_atom_limit()
    res = _find([(A, pos, z)])
    assert (res.ns, res.n_ops, res.n_translations, res.point_group_order, res.crystal_system) == ([1024], [16], [1], [16], ["tetragonal"])
    got = _numpy(res, 0)
    ref.check_space_group(A, pos, z, got, SYMPREC, exact=EXACT)
    assert (got["orbits"] == 0).sum() == 1 and (got["atom_map"][:, 0] == 0).all() and not got["shifts"][:, 0].any()
    # the classes of the sites of the 8 x 8 x 16 torus under 4/mmm about a site: {|x|, |y|} unordered from 0 .. 4, |z| from 0 .. 8
    assert len(np.unique(got["orbits"])) == 15 * 9
    print("(d) 1024 atoms: 16 operations, one translation, tetragonal, 135 orbits, check_space_group passes")


# --- (e) more lattice operations than the list holds -----------------------------------------------------------------------------
def test_too_many_lattice_operations_raise_and_leave_the_others_intact():
    """Simple cubic a = 1 at symprec = 0.45: 18 candidates per axis fit the list of 256, their 768 triples that keep the metric do
    not fit the 48 lattice operations.  hBN and rutile have nothing between 1e-3 and 0.45 A (tests/test_sym_ref.py asserts that the
    restatement finds the same at both), so beside it they must come out as they did in the batch."""
    S, names, res = _structures(), list(_structures()), _batch()
    with pytest.raises(ValueError, match="structure 1") as err:
        _find([S["hBN"], (np.eye(3), np.zeros((1, 3)), np.array([1])), S["rutile"]], symprec=0.45)
    assert "lattice operations" in str(err.value) and "structure 0" not in str(err.value) and "structure 2" not in str(err.value)
    part = err.value.result
    assert part.n_ops == [12, 0, 16] and part.rotations[1].shape == (0, 3, 3) and part.orbits[1].tolist() == [0]
    assert _same_bits(part, 0, res, names.index("hBN")) and _same_bits(part, 2, res, names.index("rutile"))
    print("(e) 768 lattice operations of one structure: ValueError, n_ops 0, the neighbours' bits are the batch's")


# --- (f) the symmetrisers --------------------------------------------------------------------------------------------------------
def _rotations(A, W):
    return np.array([ref.cartesian_rotation(A, w) for w in W])  # [G, 3, 3]


def _force_residual(F, Q, amap):
    """|F'[map_g(i)] - Q_g F'[i]| over g, i and the components -> [G, n, 3]."""
    return np.abs(F[amap] - np.einsum("gab,ib->gia", Q, F))


def _stress_residual(S, Q):
    return np.abs(np.einsum("gab,bc,gdc->gad", Q, S, Q) - S)  # |Q_g s' Q_g^T - s'| -> [G, 3, 3]


def test_symmetrised_values_on_the_hard_structures():
    """Against the restatement: the term-count bound of the first symmetriser test, b = 2 (G + 8) 2^-53 / G x sum |terms| per
    element.  And on the device's outputs alone, for every operation g: F'[map_g(i)] = Q_g F'[i], Q_g s' Q_g^T = s', and the
    positions of an exact crystal unchanged.  A float64 projection satisfies these to rounding only, so the same residuals are
    evaluated on the restatement's output; the device's lies within b of that on both sides of an identity, which allows
    b[map_g(i)] + |Q_g| b[i] for the forces, b + |Q_g| b |Q_g|^T for the stress and b for the positions, plus 4 x the
    restatement's largest residual (the evaluation of the identity itself rounds again, on other values)."""
    S, names, res = _structures(), list(_structures()), _batch()
    rng = np.random.default_rng(11)
    lats = [S[n][0] for n in names]
    forces = [rng.normal(size=S[n][1].shape) for n in names]
    stress = rng.normal(size=(len(names), 3, 3))
    got_f = symmetrize_forces(res, lats, forces)
    got_s = symmetrize_stress(res, _t(np.array(lats)), _t(stress))
    got_p = symmetrize_positions(res, lats, [S[n][1] for n in names])
    worst = {k: 0.0 for k in ("forces", "stress", "positions")}
    resid = {k: [0.0, 0.0] for k in ("forces", "stress", "positions")}  # the device's, the restatement's
    for b, name in enumerate(names):
        want = _want(name)
        G, (A, pos, _) = want["n_ops"], S[name]
        bound = 2.0 * (G + 8) * EPS / G
        exp, allow = {}, {}
        for what, got, (e, mag) in (("forces", got_f[b], ref.symmetrize_forces(want, A, forces[b])),
                                    ("stress", got_s[b], ref.symmetrize_stress(want, A, stress[b])),
                                    ("positions", got_p[b], ref.symmetrize_positions(want, A, pos))):
            if what == "positions":
                mag = mag @ np.abs(A)
            dev = np.abs(got.cpu().numpy() - e)
            assert mag.min() > 0.0 or (dev[mag == 0.0] == 0.0).all()
            assert (dev <= bound * mag).all(), (name, what, (dev / np.maximum(bound * mag, 1e-300)).max())
            worst[what] = max(worst[what], float((dev / np.maximum(mag / G, 1e-300)).max()))
            exp[what], allow[what] = e, bound * mag
        # the identities, from the device's own operations and outputs
        mine = _numpy(res, b)
        Q, amap = _rotations(A, mine["rotations"]), mine["atom_map"]
        absQ = np.abs(Q)
        Fd, Sd, Pd = got_f[b].cpu().numpy(), got_s[b].cpu().numpy(), got_p[b].cpu().numpy()
        for what, dev, of_ref, allowed in (
                ("forces", _force_residual(Fd, Q, amap), _force_residual(exp["forces"], Q, amap),
                 allow["forces"][amap] + np.einsum("gab,ib->gia", absQ, allow["forces"])),
                ("stress", _stress_residual(Sd, Q), _stress_residual(exp["stress"], Q),
                 allow["stress"] + np.einsum("gab,bc,gdc->gad", absQ, allow["stress"], absQ)),
                ("positions", np.abs(Pd - pos), np.abs(exp["positions"] - pos), allow["positions"])):
            at = np.unravel_index(np.argmax(dev - allowed), dev.shape)
            assert (dev <= allowed + 4.0 * of_ref.max()).all(), (name, what, at, dev[at], allowed[at], of_ref.max())
            resid[what] = [max(resid[what][0], float(dev.max())), max(resid[what][1], float(of_ref.max()))]
    print("(f) largest deviations from the restatement in units of the mean magnitude of a term: " +
          ", ".join(f"{k} {v:.2e}" for k, v in worst.items()))
    print("(f) largest residuals of F'[map(i)] = Q F'[i], Q s' Q^T = s' and r' = r, the device's (the restatement's): " +
          ", ".join(f"{k} {v[0]:.2e} ({v[1]:.2e})" for k, v in resid.items()))


def test_noisy_copies_come_back_to_the_exact_crystal_and_stay():
    """Every atom displaced by at most 1e-5 A (``ref.noisy_copies``; tests/test_sym_ref.py asserts the margin and that the
    restatement passes what is asked here): the symmetrised positions lie within 1e-5 A of the exact crystal, and a second
    application leaves them where they are - within the term-count bounds of both applications, the first carried through the
    second, plus 4 x what the restatement moves its own on the second."""
    N = ref.noisy_copies()
    names = list(N)
    res = _find([N[n][:3] for n in names])
    lats = [N[n][0] for n in names]
    back = symmetrize_positions(res, lats, [N[n][1] for n in names])
    again = symmetrize_positions(res, lats, back)
    for b, name in enumerate(names):
        A, noisy, z, exact = N[name]
        want = ref.find_symmetry(A, noisy, z, SYMPREC)
        _same_as_restated(res, b, want, name)
        ref.check_space_group(A, noisy, z, _numpy(res, b), SYMPREC)
        G = want["n_ops"]
        bound = 2.0 * (G + 8) * EPS / G
        first, mag1 = ref.symmetrize_positions(want, A, noisy)
        second, mag2 = ref.symmetrize_positions(want, A, first)
        b1, b2 = bound * (mag1 @ np.abs(A)), bound * (mag2 @ np.abs(A))
        c1 = float(ref._norm(b1).max())  # a mean of rotated vectors is no longer than the longest: what b1 can become in a second pass
        got1, got2 = back[b].cpu().numpy(), again[b].cpu().numpy()
        assert (np.abs(got1 - first) <= b1).all() and (np.abs(got2 - second) <= c1 + b2).all(), name
        off = float(ref._norm(got1 - exact).max())
        assert off <= ref.NOISE, (name, off)
        moved, of_ref = np.abs(got2 - got1), np.abs(second - first)  # |got2 - second| + |second - first| + |first - got1|
        assert (moved <= (c1 + b2) + b1 + 4.0 * of_ref.max()).all(), (name, moved.max(), of_ref.max())
        print(f"(f) {name}: margin {want['margin']:.3f}, {off:.3e} A from the exact crystal, moved by {moved.max():.2e} A on a second "
              f"application (the restatement: {of_ref.max():.2e})")
