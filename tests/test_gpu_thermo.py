"""The thermodynamics task on the device (csrc/thermo.hip, alignn_amd/thermo.py) against the restatements of
tests/thermo_ref.py: (1) the mode sums in one launch of structures of mixed sizes, with imaginary, zero and at-cutoff modes, at
temperatures from 0 to 1e6 K, alone and rotated within the batch; (2) the reduction of the per-temperature fits for every
P and NT at which it takes another path; (3) ``qha`` end to end on the fcc Morse crystal of tests/pair_ref.py against the numpy
pipeline (phonons_ref + pair_ref + eos_ref.fit + thermo_ref); (4) the model path: the bits of ``ev_curve`` and of ``phonons`` +
``thermal_properties`` called by hand, whole and in groups."""

import numpy as np
import pytest
import torch

from alignn_amd import ev_curve, phonons, qha, thermal_properties, thermal_sums
from alignn_amd.phonons import monkhorst_pack
from alignn_amd.synthetic import make_crystal
from alignn_amd.thermo import qha_derive
from tests import eos_ref, pair_ref, phonons_ref
from tests import thermo_ref as ref
from tests.sim_gpu import DEV, _model, _t

pytestmark = pytest.mark.gpu

SUMS_RTOL = 1e-12  # per quantity, max |got - want| / max |want|: the device's exp / expm1 / log are within a few ulp per term
DERIVE_RTOL = 1e-12  # closed form, the restatement's operations in its order
# qha on the fcc Morse crystal, device against the numpy pipeline: 10 x the largest relative deviation measured on an MI355X
# (test_qha_on_the_fcc_morse_crystal's docstring), capped at 1e-6
QHA_MEASURED = 4.731e-9
QHA_RTOL = min(10.0 * QHA_MEASURED, 1e-6)
TEMPERATURES = np.array([0.0, 1e-3, 10.0, 300.0, 1e6])
CUTOFF = 0.004


def _rel(got, want):
    return float(np.abs(np.asarray(got) - np.asarray(want)).max() / max(1e-300, np.abs(np.asarray(want)).max()))


def _same(a, b):
    return np.array_equal(a, b, equal_nan=True)


# --- (1) the mode sums -----------------------------------------------------------------------------------------------------------------
def _mesh_sets():
    """(frequencies [Nq, m], Nq) with (m, Nq) = (3, 1), (9, 7), (96, 64) - the 3n limit, six whole chunks - and (25, 41): one
    chunk plus one mode.  Each holds imaginary (negative) modes, exact zeros and modes exactly at ``CUTOFF``."""
    rng = np.random.default_rng(11)
    out = []
    for m, nq in ((3, 1), (9, 7), (96, 64), (25, 41)):
        f = rng.uniform(-0.01, 0.08, (nq, m))
        flat = f.reshape(-1)
        idx = rng.permutation(flat.size)[:max(4, flat.size // 20)]
        flat[idx[::2]], flat[idx[1::2]] = 0.0, CUTOFF
        out.append((f, nq))
    out[0] = (np.array([[-0.003, CUTOFF, 0.031]]), 1)
    assert [f.size for f, _ in out] == [3, 63, 6 * ref.CHUNK, ref.CHUNK + 1]
    return out


def _sums_launch(sets, cutoff):
    off = np.concatenate([[0], np.cumsum([f.size for f, _ in sets])])
    flat = _t(np.concatenate([f.reshape(-1) for f, _ in sets]))
    out = thermal_sums(flat, off, np.array([nq for _, nq in sets]), TEMPERATURES, cutoff)
    return [x.cpu().numpy() for x in out]


@pytest.mark.parametrize("cutoff", [0.0, CUTOFF])
def test_mode_sums_match_the_restatement(cutoff):
    """One launch of B = 4: 3, 63, 6144 and 1025 frequencies.  Measured on an MI355X, max |got - want| / max |want| per
    structure and quantity: at most 1.7e-15 (U of the 1025-frequency structure, cutoff 0; F 1.2e-15, S 1.0e-15, Cv 8.1e-16),
    2.5e-16 ... 7.2e-16 for the 6144 frequencies, below 3.4e-16 for the two small ones; n_skipped exact; each structure alone
    and the batch rotated gave the batch's bits."""
    sets = _mesh_sets()
    got = _sums_launch(sets, cutoff)
    for s, (f, nq) in enumerate(sets):
        want = ref.thermal_sums(f, nq, TEMPERATURES, cutoff)
        assert got[5][s] == want["n_skipped"] == int((f <= cutoff).sum()) > 0, s
        for k, name in enumerate(("F", "U", "S", "Cv")):
            dev = _rel(got[k][s], want[name])
            print(f"cutoff {cutoff} structure {s} {name}: max |d| / max |want| {dev:.3e}")
            assert np.isfinite(got[k][s]).all() and dev <= SUMS_RTOL, (s, name, dev)
        assert abs(got[4][s] - want["zpe"]) <= SUMS_RTOL * want["zpe"], s
        assert got[0][s][0] == got[1][s][0] == got[4][s] and got[2][s][0] == 0.0 and got[3][s][0] == 0.0  # T = 0
    for s in range(len(sets)):
        alone = _sums_launch([sets[s]], cutoff)
        rolled = _sums_launch(sets[s:] + sets[:s], cutoff)
        for g, one, rol in zip(got, alone, rolled):
            assert _same(one[0], g[s]) and _same(rol[0], g[s]), s


# --- (2) the reduction of the fits -------------------------------------------------------------------------------------------------------
def _derive_inputs(P, NT, seed):
    """B = 3 structures of P volume points and NT temperatures: smooth Cv(V) and S(V) with noise, fitted volumes inside the
    range - but for structure 2, whose last one lies outside - and, for NT = 3, a status-2 row in the middle of structure 1."""
    rng = np.random.default_rng(seed)
    B = 3
    T = np.array([300.0, 450.0, 700.0])[:NT]
    V = np.stack([rng.uniform(40.0, 90.0) * (1.0 + np.linspace(-0.05, 0.06, P)) ** 3 for _ in range(B)])
    u = (V - V.mean(1, keepdims=True)) / np.ptp(V, axis=1, keepdims=True)
    cv = 2e-4 * (1.0 + 0.3 * u + 0.1 * u * u)[:, :, None] * (1.0 + 0.1 * np.arange(NT)) + rng.normal(0, 1e-7, (B, P, NT))
    s = 5e-4 * (1.0 + 0.5 * u - 0.2 * u * u)[:, :, None] * (1.0 + 0.3 * np.arange(NT)) + rng.normal(0, 1e-7, (B, P, NT))
    v_eq = V.mean(1, keepdims=True) * (1.0 + 0.004 * np.arange(NT)[None, :] + rng.uniform(-0.001, 0.001, (B, NT)))
    v_eq[2, -1] = V[2].max() * 1.01
    b_t = rng.uniform(0.3, 0.8, (B, NT))
    status = np.zeros((B, NT), dtype=np.int32)
    status[0, 0] = 1  # stopped after 100 steps: the parameters as they stood, used
    if NT == 3:
        status[1, 1] = 2
        v_eq[1, 1] = b_t[1, 1] = np.nan
    return V, cv, s, T, v_eq, b_t, status


_NAMES = ("alpha", "cv", "s", "cp", "gamma", "inside")


def _derive_launch(V, cv, s, T, v_eq, b_t, status):
    out = qha_derive(_t(V), _t(cv), _t(s), _t(T), _t(v_eq), _t(b_t), _t(status, torch.int32))
    return [x.cpu().numpy() for x in out]


@pytest.mark.parametrize("P", [4, 5, 64])
@pytest.mark.parametrize("NT", [1, 2, 3])
def test_qha_derive_matches_the_restatement(P, NT):
    """Measured on an MI355X for every (P, NT): the largest relative deviation of alpha, Cv, S, C_p and gamma from the
    restatement was 0 - the same bits, as the fit of test_gpu_eos on the same primitives; the NaN pattern and ``inside`` equal;
    each structure alone the batch's bits."""
    V, cv, s, T, v_eq, b_t, status = _derive_inputs(P, NT, 100 * P + NT)
    got = _derive_launch(V, cv, s, T, v_eq, b_t, status)
    worst = 0.0
    for b in range(len(V)):
        want = ref.qha_derive(V[b], cv[b], s[b], T, v_eq[b], b_t[b], status[b])
        for g, name in zip(got, _NAMES):
            w = want[name]
            assert np.array_equal(np.isnan(g[b]), np.isnan(w)), (b, name)
            ok = ~np.isnan(w)
            if name == "inside":
                assert np.array_equal(g[b], w), b
            elif ok.any():
                dev = float(np.max(np.abs(g[b][ok] - w[ok]) / np.abs(w[ok])))
                worst = max(worst, dev)
                assert dev <= DERIVE_RTOL, (b, name, dev)
        alone = _derive_launch(V[b:b + 1], cv[b:b + 1], s[b:b + 1], T, v_eq[b:b + 1], b_t[b:b + 1], status[b:b + 1])
        for g, one in zip(got, alone):
            assert _same(one[0], g[b]), b
    print(f"P {P} NT {NT}: largest relative deviation, kernel vs restatement: {worst:.3e}")
    alpha, cv_o, s_o, cp, gamma, inside = got
    if NT == 1:
        assert np.isnan(alpha).all() and np.isnan(cp).all() and np.isnan(gamma).all() and np.isfinite(cv_o).all()
    else:
        assert np.isfinite(alpha[0]).all() and np.isfinite(gamma[0]).all() and inside[0].all()
        assert inside[2].tolist() == [1] * (NT - 1) + [0]
    if NT == 3:  # the status-2 row: NaN itself, and the alpha (with cp and gamma, formed from it) of its two neighbours only
        for x in got[:5]:
            assert np.isnan(x[1, 1])
        assert inside[1].tolist() == [1, 0, 1] and np.isnan(alpha[1]).all()
        assert np.isfinite(cv_o[1, [0, 2]]).all() and np.isfinite(s_o[1, [0, 2]]).all()
        assert np.isfinite(alpha[[0, 2]]).all()


# --- (3) qha on the fcc Morse crystal ----------------------------------------------------------------------------------------------------
RC = 5.0
FCC = dict(supercell=(3, 3, 3), delta=0.01, mesh=(4, 4, 4), dx=np.linspace(-0.03, 0.05, 5),
           temperatures=np.arange(0.0, 801.0, 100.0), eos="murnaghan")
_CACHE = {}


def _fcc():
    a = 0.97 * pair_ref.R0 * np.sqrt(2.0)
    return 0.5 * a * np.array([[0.0, 1.0, 1.0], [1.0, 0.0, 1.0], [1.0, 1.0, 0.0]]), np.zeros((1, 3)), np.array([26.98])


def fcc_numpy_pipeline():
    """The numpy pipeline, once: per strain the cell of eos_ref.strain, the energy of pair_ref's efs, ASE's finite-displacement
    phonons (phonons_ref) on the mesh, then thermo_ref.qha."""
    if "numpy" not in _CACHE:
        lat, pos, masses = _fcc()
        efs = pair_ref.make_efs(RC)
        q = monkhorst_pack(FCC["mesh"])
        vols, ens, freqs = [], [], []
        for d in FCC["dx"]:
            cell, cart, v = eos_ref.strain(lat, pos, eos_ref.isotropic(d))
            vols.append(v)
            ens.append(efs(cell, cart)[0])
            freqs.append(phonons_ref.phonons_ref(cell, cart, masses, FCC["supercell"], FCC["delta"],
                                                 lambda sl, c: efs(sl, c)[1], qs=q)[3])
        _CACHE["numpy"] = (np.array(vols), np.array(ens), freqs,
                           ref.qha(np.array(vols), np.array(ens), freqs, len(q), FCC["temperatures"]))
    return _CACHE["numpy"]


def _fcc_device():
    if "device" not in _CACHE:
        lat, pos, masses = _fcc()
        _CACHE["device"] = qha(None, [lat], [pos], None, [masses], forces_fn=pair_ref.make_forces_fn(RC, stress=False), device=DEV,
                               **FCC)
    return _CACHE["device"]


_PAIRS = (("volume", "volume"), ("gibbs", "gibbs"), ("bulk_modulus", "bulk_modulus"), ("thermal_expansion", "alpha"),
          ("heat_capacity_p", "cp"), ("gruneisen", "gamma"))


def test_qha_on_the_fcc_morse_crystal():
    """fcc Morse (a = 0.97 x 2.9 x sqrt 2 A, one atom of mass 26.98), 3 x 3 x 3 supercell, 4 x 4 x 4 mesh, five strains from
    -0.03 to 0.05, T = 0 ... 800 step 100.  The tolerance cannot be derived (device and numpy forces differ in their last bits
    and the fit's sensitivity to them is not known): it is 10 x the largest relative deviation of V_eq, G, B, alpha, C_p and
    gamma measured on an MI355X against the numpy pipeline (``QHA_MEASURED``), capped at 1e-6.  Measured: V_eq 3.9e-11, G
    2.5e-12, B 2.4e-10, alpha 4.7e-9, C_p 8.5e-10, gamma 3.0e-9 (the phonon free energies themselves 1.0e-14 of their largest);
    no skipped mode, every fit converged, V_eq from 15.249 to 16.041 A^3 inside 14.365 ... 18.221, gamma 1.93 ... 2.25."""
    vols, ens, freqs, want = fcc_numpy_pipeline()
    res = _fcc_device()
    T = FCC["temperatures"]
    assert (want["n_skipped"] == 0).all() and (want["status"] == 0).all() and (want["inside"] == 1).all()
    assert res.volumes.shape == res.energies.shape == (1, 5) and res.phonon_free_energy.shape == (1, 5, 9)
    assert (res.n_skipped == 0).all() and (res.fit_status == 0).all() and res.inside.all()
    assert (res.thermal_expansion[0][T >= 100] > 0).all()
    assert np.array_equal(res.volumes[0], vols) and _rel(res.energies[0], ens) <= 1e-9
    print(f"F_phonon: max |d| / max |want| {_rel(res.phonon_free_energy[0], want['F']):.3e}")
    print("V_eq", res.volume[0], "gamma", res.gruneisen[0], "alpha", res.thermal_expansion[0])
    worst = 0.0
    for got_name, want_name in _PAIRS:
        g, w = getattr(res, got_name)[0], want[want_name]
        assert np.array_equal(np.isnan(g), np.isnan(w)), got_name  # (gamma at 0 K)
        ok = ~np.isnan(w) & (w != 0.0)
        dev = float(np.max(np.abs(g[ok] - w[ok]) / np.abs(w[ok])))
        print(f"{got_name}: largest relative deviation, device vs numpy pipeline: {dev:.3e}")
        worst = max(worst, dev)
    print(f"largest relative deviation of V_eq, G, B, alpha, C_p, gamma: {worst:.3e} (QHA_RTOL {QHA_RTOL:.1e})")
    assert worst <= QHA_RTOL
    assert res.bulk_modulus_GPa[0] == pytest.approx(res.bulk_modulus[0] * 160.21766208, rel=1e-15)
    assert res.n_eval_calls == 1 and res.n_phonon_evals == 1


def test_qha_per_parent_gives_the_calls_bits():
    """Two parents in one call: each the bits of its own call (the second is the first scaled by 1.01)."""
    lat, pos, masses = _fcc()
    fn = pair_ref.make_forces_fn(RC, stress=False)
    one = _fcc_device()
    both = qha(None, [1.01 * lat, lat], [pos, pos], None, [masses, masses], forces_fn=fn, device=DEV, **FCC)
    for f in ("volumes", "energies", "phonon_free_energy", "gibbs", "volume", "bulk_modulus", "bp", "thermal_expansion",
              "heat_capacity_v", "heat_capacity_p", "entropy", "gruneisen", "fit_status", "inside", "n_skipped"):
        assert _same(getattr(both, f)[1], getattr(one, f)[0]), f


# --- (4) a random-initialised ALIGNNAtomWise -----------------------------------------------------------------------------------------
def _by_hand(model, lats, pos, feats, masses, dx, T, kw, **groups):
    """``qha`` against ``ev_curve`` and against ``phonons`` + ``thermal_properties`` called by hand on the strained structures of
    the restated builder, with the same grouping options: the same bits.  -> the qha result."""
    res = qha(model, lats, pos, feats, masses, dx=dx, temperatures=T, **kw, **groups)
    ev = ev_curve(model, lats, pos, feats, dx=dx, **{k: v for k, v in groups.items() if k == "max_atoms_per_call"})
    assert np.array_equal(res.energies, ev.energies) and np.array_equal(res.volumes, ev.volumes)
    assert res.n_eval_calls == ev.n_eval_calls
    cells, carts, fs, ms = [], [], [], []
    for s in range(len(lats)):
        for d in dx:
            cell, cart, _ = eos_ref.strain(lats[s], pos[s], eos_ref.isotropic(d))
            cells.append(cell), carts.append(cart), fs.append(feats[s]), ms.append(masses[s])
    ph = phonons(model, cells, carts, fs, ms, supercell=kw["supercell"], delta=kw["delta"], qpoints=None, dos_kpts=None,
                 **{k: v for k, v in groups.items() if k == "max_atoms_per_eval"})
    th = thermal_properties(ph, T, mesh=kw["mesh"])
    shape = (len(lats), len(dx))
    assert np.array_equal(res.phonon_free_energy, th.free_energy.cpu().numpy().reshape(shape + (len(T),)))
    assert res.n_phonon_evals == ph.n_evals
    mesh_f = ph.frequencies_at(np.ascontiguousarray(monkhorst_pack(kw["mesh"])))  # (row-major, as the launch reads it)
    host_count = np.array([int((f.cpu().numpy() <= 0.0).sum()) for f in mesh_f]).reshape(shape)
    print("skipped modes per strained structure", host_count.tolist(), "of", th.n_modes.tolist())
    assert np.array_equal(res.n_skipped, host_count) and np.array_equal(th.n_skipped.reshape(shape), host_count)
    assert host_count.sum() > 0  # (random weights: imaginary modes, counted and never an error)
    assert set(res.fit_status.reshape(-1).tolist()) <= {0, 1, 2} and np.isfinite(res.phonon_free_energy).all()
    return res


def test_qha_model_path_is_ev_curve_and_phonons_by_hand_and_in_groups():
    """Two crystals of 2 and 3 atoms, four strains, three temperatures, whole and in several groups (``max_atoms_per_call`` /
    ``max_atoms_per_eval``).  The energies do not depend on the grouping; the model's float32 forces, and with them the free
    energies, follow the composition of an evaluation in their last digits (as in test_gpu_phonons), so the two calls' free
    energies are printed, not compared."""
    model = _model()
    sizes, dx, T = [2, 3], (-0.02, 0.0, 0.01, 0.03), [0.0, 150.0, 600.0]
    kw = dict(supercell=(2, 2, 2), mesh=(2, 2, 2), delta=0.05)
    lats, pos = [], []
    for i, n in enumerate(sizes):
        lat, frac, _ = make_crystal(n, 1700 + i)
        lats.append(np.asarray(lat, dtype=np.float64))
        pos.append(np.asarray(frac, dtype=np.float64) @ lats[-1])
    g = torch.Generator().manual_seed(5)
    feats = [torch.randn(n, 92, generator=g) for n in sizes]
    masses = [np.random.default_rng(i).uniform(5.0, 80.0, n) for i, n in enumerate(sizes)]
    res = _by_hand(model, lats, pos, feats, masses, dx, T, kw)
    assert res.n_eval_calls == 1 and res.n_phonon_evals == 1
    grouped = _by_hand(model, lats, pos, feats, masses, dx, T, kw, max_atoms_per_call=5, max_atoms_per_eval=100)
    assert grouped.n_eval_calls > 1 and grouped.n_phonon_evals > 1
    assert np.array_equal(grouped.energies, res.energies) and np.array_equal(grouped.volumes, res.volumes)
    print(f"free energies, in groups vs whole: max |d| / max |F| {_rel(grouped.phonon_free_energy, res.phonon_free_energy):.3e}")
