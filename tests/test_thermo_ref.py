"""CPU checks of the thermodynamics task (alignn_amd/thermo.py, csrc/thermo.hip): (1) the numpy restatement of the mode sums
(tests/thermo_ref.py) against forms it was not derived from - the closed forms of an Einstein oscillator, thermodynamic
identities and limits; (2) the restated quasi-harmonic pipeline on an Einstein solid whose Grueneisen parameter is known; (3)
the second header, include/alignn_thermo.h, through the reader of alignn_amd/_abi.py and against the built library; (4) the
input checks of the drivers, which raise before any device work."""

import numpy as np
import pytest
import torch

from alignn_amd import _abi, _lib, thermo
from alignn_amd.phonons import PhononResult
from tests import abi_checks, pair_ref
from tests import thermo_ref as ref

KB = ref.KB


# --- (1) the mode sums -----------------------------------------------------------------------------------------------------------------
def test_kb_is_codata_2014():
    assert KB == thermo.KB == pytest.approx(8.6173303e-5, rel=1e-8)


def test_einstein_oscillator_closed_forms():
    """n equal modes eps at one q-point, y = eps / (2 kB T) between 0.05 and 10, where sinh and coth are well conditioned:
    F = n kB T ln(2 sinh y), U = n (eps / 2) coth y, S = n kB (y coth y - ln(2 sinh y)), Cv = n kB (y / sinh y)^2."""
    n = 5
    for eps in (0.004, 0.03, 0.11):
        T = eps / (2.0 * KB * np.array([0.05, 0.3, 1.0, 3.0, 10.0]))
        got = ref.thermal_sums(np.full(n, eps), 1, T)
        y = eps / (2.0 * KB * T)
        want = dict(F=n * KB * T * np.log(2.0 * np.sinh(y)), U=n * 0.5 * eps / np.tanh(y),
                    S=n * KB * (y / np.tanh(y) - np.log(2.0 * np.sinh(y))), Cv=n * KB * (y / np.sinh(y)) ** 2)
        for k, w in want.items():
            assert np.abs(got[k] - w).max() <= 1e-13 * np.abs(w).max(), (eps, k)
        assert got["zpe"] == pytest.approx(n * eps / 2, rel=1e-15) and got["n_skipped"] == 0


def _mesh(seed=0, n_q=7, m=9):
    return np.random.default_rng(seed).uniform(1e-3, 0.08, (n_q, m)), n_q


def test_identities_between_the_sums():
    f, n_q = _mesh()
    T = np.array([5.0, 40.0, 300.0, 900.0])
    r = ref.thermal_sums(f, n_q, T)
    assert np.abs(r["U"] - (r["F"] + T * r["S"])).max() <= 1e-14 * np.abs(r["U"]).max()
    h = 1e-3 * T  # S = -dF/dT by central difference: error (h^2 / 6) F''' ~ 1e-6 relative
    up, dn = ref.thermal_sums(f, n_q, T + h), ref.thermal_sums(f, n_q, T - h)
    assert np.abs(-(up["F"] - dn["F"]) / (2 * h) - r["S"]).max() <= 1e-5 * np.abs(r["S"]).max()
    assert np.abs((up["U"] - dn["U"]) / (2 * h) - r["Cv"]).max() <= 1e-5 * np.abs(r["Cv"]).max()  # Cv = dU/dT


def test_limits_in_temperature():
    f, n_q = _mesh(1)
    m = f.shape[1]
    r = ref.thermal_sums(f, n_q, [0.0, 1e-3, 1e6])
    zpe = 0.5 * f.sum() / n_q
    assert r["zpe"] == pytest.approx(zpe, rel=1e-14)
    assert r["F"][0] == r["U"][0] == r["zpe"] and r["S"][0] == 0.0 and r["Cv"][0] == 0.0  # T = 0, bit for bit
    for k in ("F", "U", "S", "Cv"):
        assert np.isfinite(r[k]).all(), k
    assert r["F"][1] == r["U"][1] == r["zpe"] and r["S"][1] == 0.0 and r["Cv"][1] == 0.0  # x >= 1e7 at 1e-3 K: frozen out
    assert r["Cv"][2] == pytest.approx(m * KB, rel=1e-7)  # Dulong-Petit: kB per mode, short by x^2 / 12 < 1e-7
    assert r["U"][2] == pytest.approx(m * KB * 1e6, rel=1e-6)


def test_no_nan_from_tiny_temperatures_and_frequencies():
    r = ref.thermal_sums([1e-300, 0.02], 1, [1e-320, 1e-3, 300.0, 1e6])
    for k in ("F", "U", "S", "Cv"):
        assert np.isfinite(r[k]).all(), (k, r[k])
    assert r["Cv"][3] == pytest.approx(2 * KB, rel=1e-6)  # x = 1e-304 in the first mode: (x / om)^2, not x^2 / om^2


def test_skipped_modes_and_the_cutoff():
    f = np.array([-0.01, 0.0, 0.002, 0.002, 0.05, np.nextafter(0.002, 1.0)])
    a, b = ref.thermal_sums(f, 2, [300.0]), ref.thermal_sums(f, 2, [300.0], cutoff=0.002)
    assert a["n_skipped"] == 2 and b["n_skipped"] == 4  # a mode at the cutoff is skipped
    only = ref.thermal_sums(f[4:], 2, [300.0])
    assert b["F"][0] == pytest.approx(only["F"][0], rel=1e-15) and b["zpe"] == pytest.approx(only["zpe"], rel=1e-15)
    many = np.random.default_rng(3).uniform(-0.01, 0.05, 3 * ref.CHUNK + 1)  # several chunks and a last one of one mode
    r = ref.thermal_sums(many, 1, [300.0])
    terms = ref.mode_terms(many[many > 0], 300.0).sum(0)
    assert r["n_skipped"] == (many <= 0).sum() and r["F"][0] == pytest.approx(terms[0], rel=1e-13)


# --- (2) an Einstein solid whose Grueneisen parameter is 2 -------------------------------------------------------------------------------
def test_einstein_solid_gruneisen_parameter():
    """E(V) Murnaghan with eos_ref.TRUE, three modes eps = 0.03 (V / V0)^-2 eV, the default strains, T = 0 ... 1000 step 10:
    every mode's Grueneisen parameter is 2, so the thermodynamic one, alpha B V / Cv, is 2 up to the curvature of the fits and
    the difference quotient of alpha.  Observed: gamma between 1.9945 and 1.9987 over 100 ... 990 K (2.20 at 50 K, where alpha
    is a difference of two nearly equal volumes), V_eq from 65.15 to 65.89 inside 55.73 ... 73.12."""
    V, E, freqs = ref.einstein_solid()
    T = np.arange(0.0, 1001.0, 10.0)
    r = ref.qha(V, E, freqs, 1, T)
    assert (r["status"] == 0).all() and (r["inside"] == 1).all()
    assert V.min() < r["volume"].min() and r["volume"].max() < V.max()
    band = (T >= 100) & (T <= 990)
    print("gamma", r["gamma"][band].min(), r["gamma"][band].max(), "V_eq", r["volume"].min(), r["volume"].max())
    assert np.abs(r["gamma"][band] - 2.0).max() <= 0.01
    assert np.isnan(r["gamma"][0]) and r["cv"][0] == 0.0  # Cv = 0 at 0 K
    assert (np.diff(r["volume"]) >= 0).all() and (r["alpha"][band] > 0).all()  # (frozen out below 20 K: the same volume)
    assert (r["cp"][band] > r["cv"][band]).all() and (np.diff(r["bulk_modulus"][band]) < 0).all()


def test_derive_step_edges():
    V, E, freqs = ref.einstein_solid()
    T = np.array([100.0, 300.0, 500.0, 700.0])
    full = ref.qha(V, E, freqs, 1, T)
    sums = [ref.thermal_sums(f, 1, T) for f in freqs]
    cv, s = (np.stack([x[k] for x in sums]) for k in ("Cv", "S"))
    one = ref.qha_derive(V, cv[:, :1], s[:, :1], T[:1], full["volume"][:1], full["bulk_modulus"][:1], full["status"][:1])
    assert np.isnan(one["alpha"][0]) and np.isnan(one["cp"][0]) and np.isnan(one["gamma"][0])  # NT = 1
    assert one["cv"][0] == full["cv"][0] and one["inside"][0] == 1
    status = np.array([0, 2, 0, 0])
    r = ref.qha_derive(V, cv, s, T, full["volume"], full["bulk_modulus"], status)
    assert np.isnan([r[k][1] for k in ("alpha", "cv", "s", "cp", "gamma")]).all() and r["inside"][1] == 0
    assert np.isnan(r["alpha"][[0, 2]]).all() and np.isfinite(r["cv"][[0, 2]]).all() and np.isfinite(r["s"][[0, 2]]).all()
    assert all(r[k][3] == full[k][3] for k in ("alpha", "cv", "s", "cp", "gamma"))
    out = ref.qha_derive(V, cv, s, T, full["volume"] + 100.0, full["bulk_modulus"], full["status"])
    assert (out["inside"] == 0).all()


# --- (3) the second header -----------------------------------------------------------------------------------------------------------
def test_second_header_reads_and_the_library_exports_it():
    from alignn_amd.build import build

    build()
    structs, sigs = _abi.parse(open(thermo.HEADER).read())
    assert structs == {} and set(sigs) == abi_checks.declared(thermo.HEADER) == set(thermo.SIGNATURES)
    assert set(sigs) == {"alignn_phonon_thermal_workspace", "alignn_phonon_thermal", "alignn_qha_derive"}
    lib = thermo._load()
    assert lib is _lib.load()
    abi_checks.assert_typed(lib, sigs)
    chunk = ref.CHUNK
    assert lib.alignn_phonon_thermal_workspace(1, chunk, 3) == (4 * 3 + 2) * 8
    assert lib.alignn_phonon_thermal_workspace(2, 2 * chunk + 1, 5) == 2 * 3 * (4 * 5 + 2) * 8
    assert lib.alignn_phonon_thermal_workspace(0, chunk, 3) == 0


# --- (4) the input checks --------------------------------------------------------------------------------------------------------------
def _fcc():
    a = 0.97 * pair_ref.R0 * np.sqrt(2.0)
    return [0.5 * a * np.array([[0.0, 1.0, 1.0], [1.0, 0.0, 1.0], [1.0, 1.0, 0.0]])], [np.zeros((1, 3))], [np.array([26.98])]


def _never(*a, **k):
    raise AssertionError("device work before the checks")


@pytest.mark.parametrize("kw", [
    dict(temperatures=[0.0, -1.0]), dict(temperatures=[0.0, np.inf]), dict(temperatures=[[0.0, 1.0]]), dict(temperatures=[]),
    dict(temperatures=[0.0, 10.0, 10.0]), dict(temperatures=[10.0, 0.0]),  # strictly increasing
    dict(mesh=(4, 4)), dict(mesh=(4, 0, 4)), dict(mesh=(4, 4.5, 4)), dict(cutoff=-1e-3), dict(cutoff=np.nan),
    dict(dx=[-0.01, 0.0, 0.01]), dict(dx=[-1.0, 0.0, 0.01, 0.02]), dict(eos="vinet"), dict(supercell=(2, 2)),
    dict(relax_ions=1), dict(steps=5), dict(max_atoms_per_call=0)])
def test_qha_checks_its_options_before_any_device_work(kw):
    lats, pos, masses = _fcc()
    with pytest.raises(ValueError, match="qha"):
        thermo.qha(None, lats, pos, None, masses, forces_fn=_never, device="cuda", **kw)


def test_qha_checks_its_structures():
    lats, pos, masses = _fcc()
    with pytest.raises(ValueError, match="masses"):
        thermo.qha(None, lats, pos, None, [np.array([-1.0])], forces_fn=_never)
    with pytest.raises(ValueError, match="3n <= 96"):
        thermo.qha(None, lats, [np.zeros((33, 3))], None, [np.ones(33)], forces_fn=_never)


def test_thermal_properties_and_sums_check_their_inputs():
    empty = PhononResult(force_constants=[], lattice_points=[], frequencies=None, modes=None, dos_energies=None,
                         dos_weights=None, n_evals=0, n_supercells=0, _dyn={})
    for kw in (dict(temperatures=[-1.0]), dict(temperatures=[np.nan]), dict(mesh=(2, 2, 0)), dict(cutoff=-1.0)):
        with pytest.raises(ValueError, match="thermal_properties"):
            thermo.thermal_properties(empty, **kw)
    with pytest.raises(ValueError, match="PhononResult"):
        thermo.thermal_properties(None)
    f = torch.zeros(12, dtype=torch.float64)
    for args in ((f, [0, 6, 13], 2, [300.0]), (f, [1, 12], 1, [300.0]), (f, [0, 8, 4], 2, [300.0]), (f, [0, 12], 5, [300.0]),
                 (f, [0, 12], 0, [300.0]), (f, [0, 12], 3, [-5.0]), (f, [0, 12], 3, [300.0], -1.0), (f, [0.0, 12.0], 3, [300.0]),
                 (f.view(3, 4), [0, 12], 3, [300.0])):
        with pytest.raises(ValueError, match="thermal_sums"):
            thermo.thermal_sums(*args)
    with pytest.raises(TypeError, match="GPU"):
        thermo.thermal_sums(f, [0, 12], 3, [300.0])  # (a host tensor: the last check)
