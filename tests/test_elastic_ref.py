"""The restatements of tests/elastic_ref.py pinned without a GPU: the restated fit against numpy's ``lstsq`` / ``inv`` on
planted tensors, the restated driver against the analytic elastic constants of the pair potential of tests/pair_ref.py on fcc
(Born's lattice sum, the cubic pattern, the Cauchy relation, -V dP/dV), the relaxed-ion tensor of hcp against the clamped one,
and the host-side argument checks of ``alignn_amd.elastic``."""

import numpy as np
import pytest

from alignn_amd import elastic
from tests import defects_ref
from tests import elastic_ref as ref
from tests import pair_ref
from tests.relax_ref import run_constrained_ref

RC = ref.RC
# 10 x the largest relative deviation (of any entry of c_raw, c, compliance, sigma0 and the moduli, each relative to the largest
# magnitude of its array) between the restated fit and numpy.linalg.lstsq / inv, measured over the six sets of synthetic_sets():
# 3.5e-15 (the moduli of p12); lstsq works on the unscaled design matrix by SVD, the restatement on scaled normal equations by
# Cholesky
NUMPY_RTOL = 3.5e-14
TRUNCATION, TRUNCATION_K = ref.TRUNCATION, ref.TRUNCATION_K  # (measured here, kept where the GPU tests find them too)
HCP_STRAINS, HCP_FMAX, HCP_STEPS, HCP_FMAX_DEFAULT = ref.HCP_STRAINS, ref.HCP_FMAX, ref.HCP_STEPS, ref.HCP_FMAX_DEFAULT
hcp_parent = ref.hcp_parent


def _relmax(got, want):
    return float(np.max(np.abs(np.asarray(got) - np.asarray(want))) / np.max(np.abs(want)))


# --- the strain set and the deformation ----------------------------------------------------------------------------------------
def test_the_default_strain_set_and_the_deformation():
    e = ref.strain_set()
    assert e.shape == (24, 6) and np.count_nonzero(e) == 24
    assert np.array_equal(e[:4, 0], ref.STRAINS_DEFAULT) and np.array_equal(e[20:, 5], ref.STRAINS_DEFAULT)
    assert np.array_equal(e, elastic._strain_points("t", elastic.DEFAULT_STRAINS, None))
    F = ref.defgrad([0.01, -0.02, 0.03, 0.04, -0.06, 0.08])
    assert np.array_equal(F, F.T)
    assert np.array_equal(F, np.array([[1.01, 0.04, -0.03], [0.04, 0.98, 0.02], [-0.03, 0.02, 1.03]]))
    assert np.array_equal(elastic._defgrad(e), np.stack([ref.defgrad(row) for row in e]))
    s = np.arange(9.0).reshape(3, 3)
    assert np.array_equal(ref.voigt_stress(s), [0.0, 4.0, 8.0, 6.0, 4.0, 2.0])
    assert np.array_equal(ref.voigt_stress(ref.full_stress(np.arange(6.0))), np.arange(6.0))
    assert elastic.MODULI == ref.MODULI and elastic.EV_A3_TO_GPA == ref.EV_A3_TO_GPA == 160.21766208


def test_the_second_derivative_of_the_pair_potential():
    r = np.linspace(2.0, 4.95, 60)
    h = 1e-5
    num = (pair_ref.phi(r + h, RC)[1] - pair_ref.phi(r - h, RC)[1]) / (2 * h)
    assert np.abs(ref.d2phi(r, RC) - num).max() <= 1e-8 * np.abs(num).max()
    assert ref.d2phi(np.array([5.0, 6.0]), RC).tolist() == [0.0, 0.0]


# --- the restated fit against numpy ------------------------------------------------------------------------------------------------
def test_fit_agrees_with_numpy_lstsq_and_inv():
    """Every output of the restated fit against ``lstsq_fit`` on the six synthetic sets; the deviations measured are in the
    comment of NUMPY_RTOL."""
    worst = 0.0
    for name, (e, g) in ref.synthetic_sets().items():
        got = ref.fit(e, g)
        c_raw, c, S, sigma0, mod, rms = ref.lstsq_fit(e, g)
        assert got["status"] == 0, name
        devs = dict(c_raw=_relmax(got["c_raw"], c_raw), c=_relmax(got["c"], c), compliance=_relmax(got["compliance"], S),
                    sigma0=_relmax(got["sigma0"], sigma0), moduli=_relmax(got["moduli"], mod))
        print(name, {k: f"{v:.2e}" for k, v in devs.items()}, f"rms {got['rms']:.3e} / {rms:.3e}")
        worst = max(worst, max(devs.values()))
        assert max(devs.values()) <= NUMPY_RTOL, (name, devs)
        if "noise" in name:
            assert got["rms"] == pytest.approx(rms, rel=1e-6) or len(e) == 7  # (seven points: an interpolation, rms is rounding)
        else:
            assert got["rms"] <= 1e-15 and got["asymmetry"] <= 1e-13, name
    print(f"largest relative deviation from numpy: {worst:.3e}")


def test_the_exact_sets_recover_the_planted_tensor():
    """The bound is the rounding of normal equations, cond(N) eps with N the scaled normal matrix (cond(N) = cond(A)^2), times
    16 for the 7 x 7 accumulations; cond(N) is 9.6 (P = 24), 6.0 (P = 12), 7.3 (P = 7), so the bounds are 2.1e-14 ... 3.4e-14."""
    C, sigma0 = ref.planted()
    for name in ("p24", "p12", "p7"):
        e, g = ref.synthetic_sets()[name]
        A = np.concatenate([np.ones((len(e), 1)), e / np.abs(e).max()], axis=1)
        tol = 16 * np.linalg.cond(A.T @ A) * np.finfo(np.float64).eps
        got = ref.fit(e, g)
        print(name, f"cond(N) {np.linalg.cond(A.T @ A):.3e} tol {tol:.2e} dev {_relmax(got['c_raw'], C):.2e}")
        assert _relmax(got["c_raw"], C) <= tol and _relmax(got["c"], C) <= tol and _relmax(got["sigma0"], sigma0) <= tol, name
        assert got["status"] == 0 and np.all(np.linalg.eigvalsh(got["c"]) > 0)
        assert _relmax(got["compliance"] @ C, np.eye(6)) <= 100 * tol


def test_status_1_and_2_come_out_where_planted():
    e, g = ref.unstable_set()
    got = ref.fit(e, g)
    assert got["status"] == 1 and np.linalg.eigvalsh(got["c"]).min() < 0
    assert np.isfinite(got["c_raw"]).all() and np.isfinite(got["c"]).all() and np.isfinite(got["sigma0"]).all()
    assert np.isfinite([got["rms"], got["asymmetry"]]).all()
    assert np.isnan(got["compliance"]).all()
    assert np.isfinite(got["moduli"][[0, 3]]).all() and np.isnan(got["moduli"][[1, 2, 4, 5, 6, 7, 8]]).all()
    want = ref.lstsq_fit(e, g)
    assert _relmax(got["c"], want[1]) <= NUMPY_RTOL
    for e, g in (ref.deficient_set(), (e[:6], g[:6]), (e, np.where(np.arange(24)[:, None, None] == 3, np.nan, g)),
                 (np.zeros_like(e), g)):
        got = ref.fit(e, g)
        assert got["status"] == 2
        for k in ("c_raw", "c", "compliance", "sigma0", "moduli", "rms", "asymmetry"):
            assert np.isnan(got[k]).all(), k


def test_the_moduli_of_an_isotropic_tensor():
    lam, mu = 0.7, 0.4
    C = np.zeros((6, 6))
    C[:3, :3] = lam
    C[np.arange(3), np.arange(3)] = lam + 2 * mu
    C[np.arange(3, 6), np.arange(3, 6)] = mu
    K = lam + 2 * mu / 3
    want = [K, K, K, mu, mu, mu, 9 * K * mu / (3 * K + mu), (3 * K - 2 * mu) / (2 * (3 * K + mu)), 0.0]
    assert ref.moduli(C, np.linalg.inv(C)) == pytest.approx(want, rel=1e-14, abs=1e-14)


# --- physics: fcc under the pair potential ---------------------------------------------------------------------------------------------
_FCC = {}
HALF = tuple(0.5 * np.array(ref.STRAINS_DEFAULT))


def zero_pressure_fcc():
    """fcc at the lattice constant where ``make_efs(RC)`` gives zero pressure, found by bisection between 3.8 (compressed) and
    4.2 (stretched): dict(a, efs, full / half: the restated tensor at the default strains / at half of them, born)."""
    if not _FCC:
        efs = pair_ref.make_efs(RC)
        lo, hi = 3.8, 4.2
        assert ref.fcc_pressure(efs, lo) > 0 > ref.fcc_pressure(efs, hi)
        for _ in range(60):
            mid = 0.5 * (lo + hi)
            lo, hi = (mid, hi) if ref.fcc_pressure(efs, mid) > 0 else (lo, mid)
        a = 0.5 * (lo + hi)
        assert abs(ref.fcc_pressure(efs, a)) < 1e-14
        lat, pos = defects_ref.fcc(a)
        _FCC.update(a=a, efs=efs, full=ref.elastic_tensor(lat, pos, efs), half=ref.elastic_tensor(lat, pos, efs, strains=HALF),
                    born=ref.born_cubic(RC, a))
    return _FCC


def _born_deviation(C, born, tol):
    """The cubic pattern, the Cauchy relation and Born's constants, all relative to C11 -> the largest deviation from Born's."""
    c11, c12, c44 = ref.cubic_pattern(C, tol)
    assert abs(c12 - c44) <= tol * c11  # the Cauchy relation of a pair potential with every atom an inversion centre
    dev = max(abs(c11 - born[0]), abs(c12 - born[1]), abs(c44 - born[2])) / c11
    assert dev <= tol, dev
    return dev


def test_fcc_tensor_is_cubic_obeys_cauchy_and_agrees_with_born():
    case = zero_pressure_fcc()
    born = case["born"]
    assert born[1] == pytest.approx(born[2], rel=1e-13)  # (Cauchy holds exactly in the lattice sum)
    full, half = case["full"], case["half"]
    assert full["status"] == 0 and half["status"] == 0
    dev_full = _born_deviation(full["c"], born, TRUNCATION)
    dev_half = _born_deviation(half["c"], born, TRUNCATION / 4)
    print(f"a {case['a']:.10f} born {born} truncation error: default strains {dev_full:.3e}, halved {dev_half:.3e}")
    assert 3.5 <= dev_full / dev_half <= 4.5  # second order in the strain
    assert dev_full >= TRUNCATION / 4  # (the bound is no wider than it is said to be)


@pytest.mark.parametrize("a", [None, 3.9, 4.0], ids=["zero_pressure", "3.9", "4.0"])
def test_voigt_bulk_modulus_is_minus_v_dp_dv(a):
    """K_V of the stress-strain slopes is -V dP/dV at any pressure (an isotropic strain eps changes V by 3 eps V): at zero
    pressure and on the two parents of the GPU test.  The deviations measured are in the comment of TRUNCATION_K."""
    case = zero_pressure_fcc()
    efs = case["efs"]
    if a is None:
        a, full, half = case["a"], case["full"], case["half"]
        assert ref.bulk_modulus_fd(efs, a) == pytest.approx((case["born"][0] + 2 * case["born"][1]) / 3, rel=1e-6)
    else:
        lat, pos = defects_ref.fcc(a)
        full, half = ref.elastic_tensor(lat, pos, efs), ref.elastic_tensor(lat, pos, efs, strains=HALF)
        ref.cubic_pattern(full["c"])
    K = ref.bulk_modulus_fd(efs, a)
    dev_full, dev_half = abs(full["moduli"][0] - K) / K, abs(half["moduli"][0] - K) / K
    print(f"a {a}: -V dP/dV {K:.8f}, K_V {full['moduli'][0]:.8f}: rel {dev_full:.3e}, strains halved {dev_half:.3e}")
    assert dev_full <= TRUNCATION_K and dev_half <= TRUNCATION_K / 4
    assert 3.5 <= dev_full / dev_half <= 4.5 and dev_full >= TRUNCATION_K / 4


# --- relaxed ions ----------------------------------------------------------------------------------------------------------------------
def test_hcp_relaxes_at_fixed_cell_on_every_default_strained_structure():
    lat, pos = hcp_parent()
    efs = pair_ref.make_efs(RC)
    most = 0
    for e in ref.strain_set():
        cell, cart = ref.strained(lat, pos, e)
        run = run_constrained_ref(cell, cart, efs, fmax=HCP_FMAX_DEFAULT, steps=100, mask=np.zeros(6))
        assert run["converged"] and np.array_equal(run["C"], cell), e
        most = max(most, run["n_steps"])
    print("most steps", most)
    assert 1 <= most < 100


def test_relaxed_ion_tensor_differs_from_the_clamped_one():
    """The bound of the difference is 100 x the larger rms / max |eps| of the two fits.  The residual of a linear fit to the
    curved response grows as eps^2 (rms 6.7e-5 eV/A^3 at the default strains), so at the default strains the bound is 0.67 eV/A^3,
    more than any C_ij of this crystal, while the internal relaxation changes C by a fixed amount: the strains are therefore
    HCP_STRAINS, a hundredth of the default ones.  Measured there: rms 7.4e-9 (clamped) and 7.2e-9 (relaxed), the bound 7.4e-3,
    the largest difference 3.87e-2 (C11, C22: 0.5136 -> 0.4753 at the default strains; C66 0.2063 -> 0.1676)."""
    lat, pos = hcp_parent()
    efs = pair_ref.make_efs(RC)
    clamped = ref.elastic_tensor(lat, pos, efs, strains=HCP_STRAINS)
    relaxed = ref.elastic_tensor(lat, pos, efs, strains=HCP_STRAINS, relax_ions=True, fmax=HCP_FMAX, steps=HCP_STEPS)
    assert relaxed["converged"].all() and 1 <= relaxed["n_steps"].max() < HCP_STEPS
    assert clamped["status"] == 0 and relaxed["status"] == 0
    bound = 100 * max(clamped["rms"], relaxed["rms"]) / np.abs(clamped["strains"]).max()
    diff = np.abs(relaxed["c"] - clamped["c"])
    print(f"rms {clamped['rms']:.3e} / {relaxed['rms']:.3e}, bound {bound:.3e}, largest difference {diff.max():.3e}")
    assert diff.max() > bound
    assert relaxed["c"][0, 0] < clamped["c"][0, 0]  # (relaxing the ions can only soften a stretch)


# --- the driver's argument checks -----------------------------------------------------------------------------------------------------
def _fn(lats, poss):
    raise AssertionError("an argument error must come before any evaluation")


@pytest.mark.parametrize("kw", [
    dict(strains=(-0.01, 0.0, 0.01)), dict(strains=(-0.01, 0.01, 0.01)), dict(strains=(0.01,)), dict(strains=np.linspace(0.001, 0.011, 11)),
    dict(strains=(-0.01, np.nan)), dict(strains=(-0.01, np.inf)), dict(strains=(-0.3, 0.01)), dict(strains=np.zeros((2, 2))),
    dict(strain_set=0.01 * np.eye(6)), dict(strain_set=np.zeros((65, 6))), dict(strain_set=np.zeros((8, 5))),
    dict(strain_set=np.full((8, 6), 0.2)), dict(strain_set=np.full((8, 6), np.nan)),
    dict(strains=(-0.01, 0.01), strain_set=ref.SEVEN), dict(steps=5), dict(fmax=0.05), dict(optimize_lattice=False),
    dict(cell_mask=[1, 1, 1, 0, 0, 0]), dict(relax_ions=True, cell_mask=[1, 1, 1, 0, 0, 0]), dict(relax_ions=True, steps=-1),
    dict(relax_ions=1), dict(on_relaxed_struct="yes"), dict(max_atoms_per_call=0), dict(max_atoms_per_call=2.5),
], ids=lambda kw: ",".join(kw))
def test_argument_errors_come_before_any_device_work(kw):
    lat, pos = defects_ref.fcc(4.0)
    with pytest.raises(ValueError):
        elastic.elastic_tensor(None, [lat], [pos], forces_fn=_fn, **kw)


def test_structure_errors_are_those_of_the_other_drivers():
    lat, pos = defects_ref.fcc(4.0)
    with pytest.raises(ValueError):
        elastic.elastic_tensor(None, [lat], [pos[:, :2]], forces_fn=_fn)
    with pytest.raises(ValueError):
        elastic.elastic_tensor(None, [lat, lat], [pos], forces_fn=_fn)
    with pytest.raises(TypeError):
        elastic.elastic_tensor(object(), [lat], [pos])
