"""The restatement of the symmetry-reduced phonons (tests/phonons_sym_ref.py, the rules of include/alignn_phsym.h) held to
what it must give, on the CPU: the direction counts derived by hand from the site groups, the gap around the spanning
threshold tau, and - with an exactly linear force field, where central differences are exact - the force constants of all
6n displacements, their covariance under every usable operation, and the bits of the all-displacement path for a structure
with the identity alone."""

import os
import re

import numpy as np
import pytest

from tests import phonons_ref as P
from tests import phonons_sym_ref as R
from tests import sym_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SUPERCELLS = ((2, 2, 2), (3, 3, 3), (2, 3, 4))
# the two extreme ratios det M / (trace M / 3)^3 over every subset tried (test_tau_sits_in_a_wide_gap lists them); the header
# quotes the same figures
HIGHEST_DEFICIENT, LOWEST_SPANNING = 1.9e-16, 0.729


@pytest.fixture(scope="module")
def crystals():
    out = {}
    for name, (A, pos, z, *_) in sym_ref.crystals().items():
        out[name] = (A, pos, z, sym_ref.find_symmetry(A, pos, z))
    return out


def test_candidates_are_the_headers_thirteen_unit_vectors():
    text = open(os.path.join(ROOT, "include", "alignn_phsym.h")).read()
    assert float(re.search(r"#define\s+ALIGNN_PHSYM_TAU\s+(\S+)", text).group(1)) == R.TAU
    assert int(re.search(r"#define\s+ALIGNN_PHSYM_N_CANDIDATES\s+(\d+)", text).group(1)) == len(R.CANDIDATES) == 13
    assert set(np.abs(R.CANDIDATES).reshape(-1)) == {0.0, 1.0, 0.7071067811865475, 0.5773502691896258}
    assert "0.7071067811865475" in text and "0.5773502691896258" in text
    assert np.abs(np.linalg.norm(R.CANDIDATES, axis=1) - 1.0).max() <= 2e-16


# the table of the feature's issue, derived by hand from the site groups at (N, N, N): directions per representative
DIRECTIONS = {"fcc": [1], "diamond": [1], "rocksalt": [1, 1], "zincblende": [1, 1], "bcc_cube": [1], "hcp": [1], "wurtzite": [1, 1],
              "tetragonal": [1], "orthorhombic": [1], "monoclinic": [2], "triclinic_inversion_pair": [3],
              "triclinic_two_species": [3, 3]}


@pytest.mark.parametrize("N", [(2, 2, 2), (3, 3, 3)])
def test_direction_counts_match_the_table(crystals, N):
    for name, want in DIRECTIONS.items():
        A, pos, z, sym = crystals[name]
        pl = R.plan(sym, A, N)
        assert [len(pl["cand"][i]) for i in pl["reps"]] == want, name
        assert len(pl["displaced_atoms"]) == sum(want) and pl["directions"].shape == (sum(want), 3)
    assert crystals["hcp"][3]["n_ops"] == 24
    A, _, _, sym = crystals["hcp"]
    assert R.plan(sym, A, N)["cand"][0] == [4]  # (1, 0, 1) is the first candidate whose images span space
    A, _, _, sym = crystals["orthorhombic"]
    assert R.plan(sym, A, N)["cand"][0] == [9]  # a body diagonal
    A, _, _, sym = crystals["bcc_cube"]
    pl = R.plan(sym, A, N)
    assert pl["reps"] == [0] and len(pl["site"][0]) == 48 and pl["dist"][1] >= 0  # one representative, through the centring


def test_only_a_subgroup_is_usable_in_an_uneven_supercell(crystals):
    A, _, _, sym = crystals["fcc"]
    assert R.plan(sym, A, (3, 3, 3))["usable"].sum() == 48
    pl = R.plan(sym, A, (2, 3, 4))
    assert pl["usable"].sum() == 2 and len(pl["site"][0]) == 2 and pl["cand"][0] == [0, 1, 2]  # identity and inversion
    A, _, _, sym = crystals["simple_cubic"]
    assert R.plan(sym, A, (2, 3, 4))["usable"].sum() == 8  # the operations that keep every axis


def test_tau_sits_in_a_wide_gap(crystals):
    lo_span, hi_def = np.inf, 0.0
    for name, (A, _, _, sym) in crystals.items():
        for N in SUPERCELLS:
            for k, subset, ratio in R.plan(sym, A, N)["ratios"]:
                if ratio >= R.TAU:
                    lo_span = min(lo_span, ratio)
                else:
                    hi_def = max(hi_def, abs(ratio))
    print(f"span ratios: highest rank-deficient {hi_def:.3e}, lowest spanning {lo_span:.6f}, tau {R.TAU:g}")
    assert hi_def <= HIGHEST_DEFICIENT and lo_span >= LOWEST_SPANNING
    assert hi_def * 100.0 <= R.TAU <= lo_span / 100.0
    # and with room for a structure that is symmetric only to a loose symprec: (symprec / cell edge)^2 ~ (1e-3 / 3)^2
    assert (1e-3 / 3.0) ** 2 * 100.0 <= R.TAU


def _harmonic_case(A, pos, z, sym, N, delta=0.01):
    """-> (C of all 6n displacements, C by symmetry, the plan) with harmonic forces, no drift correction and no passes."""
    n = len(pos)
    sl = np.asarray(A, dtype=np.float64) * np.asarray(N, dtype=np.float64)[:, None]
    cart0 = R.ideal_supercell(A, pos, N)
    forces_of = R.harmonic_forces(R.pair_spring_hessian(sl, cart0, np.tile(z, int(np.prod(N)))), cart0)
    inv = P.inv_supercell(A, N)
    full = P.force_constants([forces_of(sl, c) for _, c in P.displaced_supercells(A, pos, N, delta, inv)], n, N, delta, None, 0)
    pl = R.plan(sym, A, N)
    cells = R.displaced_supercells_sym(A, pos, N, delta, inv, pl)
    assert len(cells) == 2 * len(pl["displaced_atoms"])
    reduced = R.force_constants_sym([forces_of(sl, c) for _, c in cells], pl, sym, delta, None, 0)
    return full, reduced, pl


CASES = [(name, N) for name in ("diamond", "hcp", "wurtzite", "monoclinic") for N in ((2, 2, 2), (3, 3, 3))] + [("fcc", (2, 3, 4))]


@pytest.mark.parametrize("name,N", CASES)
def test_reduced_force_constants_equal_all_displacements_and_are_covariant(crystals, name, N):
    """Central differences of a linear force field are exact, so the two differ by rounding through a 3 x 3 solve whose
    conditioning tau limits.  1e-9 of max |C| would be safe for any M that passes tau; the CPU run allows 1e-12 (the worst case measures 2.6e-14:
    a few hundred roundings of 1.1e-16 through an M whose ratio det M / t^3 is at least 0.729, a condition number below 2)."""
    A, pos, z, sym = crystals[name]
    full, reduced, pl = _harmonic_case(A, pos, z, sym, N)
    scale = np.abs(full).max()
    err = np.abs(reduced - full).max() / scale
    cov = R.covariance_error(reduced, sym, pl) / scale
    print(f"{name} {N}: {len(pl['displaced_atoms'])} directions of {3 * len(pos)}, |dC| / max |C| {err:.2e}, covariance {cov:.2e}")
    assert len(pl["displaced_atoms"]) < 3 * len(pos) or name == "fcc"
    assert scale > 0.1 and err <= 1e-12 and cov <= 1e-12


def test_identity_only_structure_gives_the_all_displacement_bits(crystals):
    A, pos, z, sym = crystals["triclinic_two_species"]
    assert sym["n_ops"] == 1
    N, delta = (2, 3, 2), 0.013
    sl = A * np.asarray(N, dtype=np.float64)[:, None]
    rng = np.random.default_rng(5)
    table = {}

    def forces_of(sl, cart):  # any forces at all: a fixed random array per displaced supercell
        return table.setdefault(cart.tobytes(), rng.normal(size=cart.shape))

    inv = P.inv_supercell(A, N)
    pl = R.plan(sym, A, N)
    assert pl["displaced_atoms"].tolist() == [0, 0, 0, 1, 1, 1] and np.array_equal(pl["directions"], np.tile(np.eye(3), (2, 1)))
    all_cells = P.displaced_supercells(A, pos, N, delta, inv)
    sym_cells = R.displaced_supercells_sym(A, pos, N, delta, inv, pl)
    assert len(all_cells) == len(sym_cells) == 12
    for (f0, c0), (f1, c1) in zip(all_cells, sym_cells):
        assert np.array_equal(f0, f1) and np.array_equal(c0, c1)
    forces = [forces_of(sl, c) for _, c in all_cells]
    for drift in ("frederiksen", "mean", None):
        for n_sym in (0, 3):
            assert np.array_equal(R.force_constants_sym(forces, pl, sym, delta, drift, n_sym),
                                  P.force_constants(forces, 2, N, delta, drift, n_sym))
