"""The elastic-tensor task on the device (csrc/elastic.hip, alignn_amd/elastic.py) against the restatements of
tests/elastic_ref.py: (1) the stress-strain fit on exact, noisy, unstable and rank-deficient sets of mixed lengths in one
launch; (2) ``elastic_tensor`` on the pair potential of tests/pair_ref.py; (3) relaxed ions on hcp: the same bits as a direct
``relax`` at fixed cell; (4) the model path: the same bits as a direct ``relax`` on the restated structures, and in groups;
(5) argument errors."""

import numpy as np
import pytest
import torch

from alignn_amd import _lib, elastic_fit, elastic_tensor
from alignn_amd.relax import relax
from tests import defects_ref
from tests import elastic_ref as ref
from tests import pair_ref
from tests.sim_gpu import DEV, _crystals, _model

pytestmark = pytest.mark.gpu

RC = ref.RC
# The largest deviation of any output of the fit kernel from the restated fit, relative to the largest magnitude of its array,
# measured on the inputs of test_elastic_fit_matches_the_restatement and on the drivers' own stresses (MI355X): 0 - the kernel's
# arithmetic is +, -, x, /, sqrt and max in a fixed order, so every field, the NaN patterns and the flags came out as the
# restatement's bits.  10 x 0 is 0: equality.
FIT_RTOL = 0.0
SENTINEL = -7.0
_OUT = ("c_raw", "c", "compliance", "sigma0", "moduli", "rms", "asymmetry", "status")


def _same(a, b):
    return np.array_equal(a, b, equal_nan=True)


# --- (1) the fit ----------------------------------------------------------------------------------------------------------------------
def _fit_sets():
    sets = dict(ref.synthetic_sets())
    order = ["p24", "p12", "p7", "p24_noise", "p12_noise", "p7_noise"]
    out = {k: sets[k] for k in order}
    out["unstable"] = ref.unstable_set()
    out["deficient"] = ref.deficient_set()
    return out


def _launch(sets, ld=None, n_points=None):
    """One launch over ``sets`` (a list of (strain [P, 6], stress [P, 3, 3])) padded to ``ld`` points with the sentinel -> dict
    of numpy outputs."""
    B, ld = len(sets), ld or max(len(e) for e, _ in sets)
    strain = np.full((B, ld, 6), SENTINEL)
    stress = np.full((B, ld, 3, 3), SENTINEL)
    for s, (e, g) in enumerate(sets):
        strain[s, :len(e)], stress[s, :len(e)] = e, g
    n = torch.tensor([len(e) for e, _ in sets] if n_points is None else n_points, dtype=torch.int32, device=DEV)
    out = elastic_fit(torch.tensor(strain, device=DEV), torch.tensor(stress, device=DEV), n)
    return dict(zip(_OUT, [t.cpu().numpy() for t in out]))


def _deviation(got, want, s):
    """The largest relative deviation of structure s of the launch ``got`` from the restated ``want``; the NaN pattern and the
    status must match exactly."""
    assert got["status"][s] == want["status"]
    worst = 0.0
    for k in _OUT[:-1]:
        g, w = np.asarray(got[k][s]), np.asarray(want[k])
        assert np.array_equal(np.isnan(g), np.isnan(w)), k
        if np.isfinite(w).any() and np.nanmax(np.abs(w)) > 0:
            worst = max(worst, float(np.nanmax(np.abs(g - w)) / np.nanmax(np.abs(w))))
    return worst


def test_elastic_fit_matches_the_restatement():
    """One launch of B = 8 with P = 24, 12, 7 (exact), 24, 12, 7 (1e-6 noise), the unstable set (status 1) and the
    rank-deficient one (status 2) in the last place, rows padded with the sentinel.  Each structure alone and the batch rolled by
    one place give the launch's bits."""
    sets = _fit_sets()
    names, data = list(sets), list(sets.values())
    assert [len(e) for e, _ in data] == [24, 12, 7, 24, 12, 7, 24, 24]
    got = _launch(data)
    assert got["status"].tolist() == [0, 0, 0, 0, 0, 0, 1, 2]
    worst = 0.0
    C, _ = ref.planted()
    for s, name in enumerate(names):
        want = ref.fit(*data[s])
        dev = _deviation(got, want, s)
        print(f"{name}: status {got['status'][s]} rms {got['rms'][s]:.3e} asymmetry {got['asymmetry'][s]:.3e} K_V "
              f"{got['moduli'][s][0]:.6f}; largest relative deviation from the restatement {dev:.3e}")
        worst = max(worst, dev)
        assert dev <= FIT_RTOL, (name, dev)
        if name in ("p24", "p12", "p7"):
            assert np.abs(got["c_raw"][s] - C).max() <= 1e-13 * np.abs(C).max(), name
    print(f"largest relative deviation of an output, kernel vs restatement: {worst:.3e}")
    assert np.isnan(got["compliance"][6]).all() and np.isfinite(got["c"][6]).all() and np.isfinite(got["moduli"][6][[0, 3]]).all()
    for k in _OUT[:-1]:
        assert np.isnan(got[k][7]).all(), k
    for s in range(len(data)):  # alone, in a launch of its own length
        alone = _launch([data[s]])
        for k in _OUT:
            assert _same(alone[k][0], got[k][s]), (names[s], k, "alone")
    rolled = _launch(data[1:] + data[:1])
    for s in range(len(data)):
        for k in _OUT:
            assert _same(rolled[k][(s - 1) % len(data)], got[k][s]), (names[s], k, "rolled")


def test_elastic_fit_rejects_what_it_cannot_fit():
    e, g = ref.synthetic_sets()["p7_noise"]
    e8, g8 = np.concatenate([e, e[:1] * 0.5]), np.concatenate([g, g[:1]])
    # fewer points than unknowns, more than the row holds: status 2, the neighbour untouched by it
    got = _launch([(e8, g8)] * 3, ld=8, n_points=[6, 8, 9])
    assert got["status"].tolist() == [2, 0, 2]
    for k in _OUT[:-1]:
        assert np.isnan(got[k][[0, 2]]).all(), k
    assert _deviation(got, ref.fit(e8, g8), 1) <= FIT_RTOL
    lib = _lib.load()
    buf = torch.zeros(65 * 9, dtype=torch.float64, device=DEV)
    out = torch.empty(36, dtype=torch.float64, device=DEV)
    p, o = buf.data_ptr(), out.data_ptr()
    for ld in (6, 65):
        assert lib.alignn_elastic_fit(p, p, None, 1, ld, o, o, o, o, o, o, o, o, _lib.stream()) != 0
    assert lib.alignn_elastic_fit(p, p, None, 1, 7, o, o, None, o, o, o, o, o, _lib.stream()) != 0
    assert lib.alignn_elastic_fit(p, p, None, -1, 7, o, o, o, o, o, o, o, o, _lib.stream()) != 0
    assert lib.alignn_elastic_fit(p, p, None, 0, 7, o, o, o, o, o, o, o, o, _lib.stream()) == 0
    with pytest.raises(ValueError):
        elastic_fit(torch.zeros(1, 6, 6, dtype=torch.float64, device=DEV), torch.zeros(1, 6, 3, 3, dtype=torch.float64, device=DEV))
    with pytest.raises(TypeError):
        elastic_fit(torch.zeros(1, 7, 6, device=DEV), torch.zeros(1, 7, 3, 3, device=DEV))


# --- (2) elastic_tensor on the pair potential ---------------------------------------------------------------------------------------
_FIELDS = ("stresses", "c", "c_raw", "compliance", "c_GPa", "sigma0", "rms", "asymmetry", "status", "converged", "n_steps") + \
    ref.MODULI + tuple(m + "_GPa" for m in ref.MODULI[:7])


def _same_result(a, s, b, t, what):
    for f in _FIELDS:
        assert _same(getattr(a, f)[s], getattr(b, f)[t]), (what, f)
    assert torch.equal(a.lattices[s], b.lattices[t]) and torch.equal(a.positions[s], b.positions[t]), what


def _against_restated_fit(res, s, what):
    """The tensor of parent s against the restated fit of the device's own stresses, under the rule of the fit test."""
    want = ref.fit(res.strains, ref.full_stress(res.stresses[s]))
    got = dict(c_raw=res.c_raw, c=res.c, compliance=res.compliance, sigma0=res.sigma0, rms=res.rms, asymmetry=res.asymmetry,
               status=res.status, moduli=np.stack([getattr(res, m) for m in ref.MODULI], axis=1))
    dev = _deviation(got, want, s)
    print(f"{what} parent {s}: largest relative deviation from the restated fit of the device's stresses {dev:.3e}")
    assert dev <= FIT_RTOL, (what, s, dev)


_CACHE = {}


def _pair_case():
    if not _CACHE:
        parents = [defects_ref.fcc(3.9), defects_ref.fcc(4.0)]
        lats, pos = [l for l, _ in parents], [p for _, p in parents]
        _CACHE["pair"] = (lats, pos, elastic_tensor(None, lats, pos, forces_fn=pair_ref.make_forces_fn(RC, stress=True), device=DEV))
    return _CACHE["pair"]


def test_elastic_tensor_on_a_pair_potential():
    lats, pos, res = _pair_case()
    efs = pair_ref.make_efs(RC)
    assert np.array_equal(res.strains, ref.strain_set()) and res.stresses.shape == (2, 24, 6)
    assert res.n_eval_calls == 1 and res.status.tolist() == [0, 0]
    assert res.converged.shape == res.n_steps.shape == (2, 24) and not res.n_steps.any()
    for s, a in enumerate((3.9, 4.0)):
        want = np.array([ref.voigt_stress(efs(*ref.strained(lats[s], pos[s], e))[2]) for e in res.strains])
        scale = np.abs(want).max()
        print(f"parent {s}: max |d stress| / max |stress| {np.abs(res.stresses[s] - want).max() / scale:.3e}")
        assert np.abs(res.stresses[s] - want).max() <= 1e-9 * scale
        _against_restated_fit(res, s, "pair")
        ref.cubic_pattern(res.c[s])
        K = ref.bulk_modulus_fd(efs, a)
        print(f"parent {s}: K_V {res.k_voigt[s]:.8f}, -V dP/dV {K:.8f}, rel {abs(res.k_voigt[s] - K) / K:.3e}")
        assert abs(res.k_voigt[s] - K) <= ref.TRUNCATION_K * K
        assert np.array_equal(res.c_GPa[s], res.c[s] * 160.21766208)
        assert res.k_hill_GPa[s] == res.k_hill[s] * 160.21766208
        assert np.array_equal(res.lattices[s].cpu().numpy(), lats[s]) and np.array_equal(res.positions[s].cpu().numpy(), pos[s])


def test_elastic_tensor_per_parent_and_in_groups_gives_the_calls_bits():
    lats, pos, res = _pair_case()
    fn = pair_ref.make_forces_fn(RC, stress=True)
    for s in range(2):
        alone = elastic_tensor(None, lats[s:s + 1], pos[s:s + 1], forces_fn=fn, device=DEV)
        _same_result(alone, 0, res, s, ("alone", s))
    grouped = elastic_tensor(None, lats, pos, forces_fn=fn, device=DEV, max_atoms_per_call=8)
    assert grouped.n_eval_calls == 24  # (two four-atom structures per call)
    for s in range(2):
        _same_result(grouped, s, res, s, ("in groups", s))


# --- (3) relaxed ions ---------------------------------------------------------------------------------------------------------------
def test_relaxed_ions_equal_a_direct_relax_at_fixed_cell():
    """hcp (tests/elastic_ref.py hcp_parent) at the strains, fmax and step cap that tests/test_elastic_ref.py shows to converge."""
    lat, pos = ref.hcp_parent()
    fn = pair_ref.make_forces_fn(RC, stress=True)
    kw = dict(fmax=ref.HCP_FMAX, steps=ref.HCP_STEPS)
    res = elastic_tensor(None, [lat], [pos], forces_fn=fn, device=DEV, strains=ref.HCP_STRAINS, relax_ions=True, **kw)
    built = [ref.strained(lat, pos, e) for e in res.strains]
    direct = relax(None, [b[0] for b in built], [b[1] for b in built], forces_fn=fn, device=DEV, optimize_lattice=True,
                   cell_mask=np.zeros(6), **kw)
    print("steps", res.n_steps[0].tolist())
    assert res.converged.all() and direct.converged.all() and 1 <= res.n_steps.max() < ref.HCP_STEPS
    assert np.array_equal(res.n_steps[0], direct.n_steps.cpu().numpy())
    assert np.array_equal(direct.lattices.cpu().numpy(), np.stack([b[0] for b in built]))  # every cell is its built cell
    strains = torch.tensor(res.strains, device=DEV)[None]
    fit = dict(zip(_OUT, [t.cpu().numpy() for t in elastic_fit(strains, direct.stresses[None].contiguous())]))
    assert np.array_equal(res.stresses[0], ref.voigt_stress(direct.stresses.cpu().numpy()))
    for k in ("c_raw", "c", "compliance", "sigma0", "rms", "asymmetry", "status"):
        assert _same(getattr(res, k)[0], fit[k][0]), k
    for i, m in enumerate(ref.MODULI):
        assert _same(getattr(res, m)[0], fit["moduli"][0][i]), m
    clamped = elastic_tensor(None, [lat], [pos], forces_fn=fn, device=DEV, strains=ref.HCP_STRAINS)
    bound = 100 * max(clamped.rms[0], res.rms[0]) / np.abs(res.strains).max()
    diff = np.abs(res.c[0] - clamped.c[0]).max()
    print(f"rms {clamped.rms[0]:.3e} / {res.rms[0]:.3e}, bound {bound:.3e}, largest difference {diff:.3e}")
    assert diff > bound


# --- (4) a random-initialised ALIGNNAtomWise -----------------------------------------------------------------------------------------
def test_elastic_tensor_model_path_equals_a_direct_relax_and_in_groups():
    model = _model()
    lats, pos, feats = _crystals(2, 6)
    res = elastic_tensor(model, lats, pos, feats, strain_set=ref.SEVEN)
    assert res.n_eval_calls == 1
    built, fs = [], []
    for s in range(2):
        for e in ref.SEVEN:
            built.append(ref.strained(np.asarray(lats[s], dtype=np.float64), np.asarray(pos[s], dtype=np.float64), e))
            fs.append(feats[s])
    direct = relax(model, [b[0] for b in built], [b[1] for b in built], fs, steps=0, optimize_lattice=True)
    want = ref.voigt_stress(direct.stresses.cpu().numpy()).reshape(2, 7, 6)
    print("whole call vs direct relax: max |d stress|", np.abs(want - res.stresses).max(), "of", np.abs(want).max())
    assert np.array_equal(want, res.stresses)
    grouped = elastic_tensor(model, lats, pos, feats, strain_set=ref.SEVEN, max_atoms_per_call=12)
    assert grouped.n_eval_calls > 1
    for s in range(2):
        _same_result(grouped, s, res, s, ("in groups", s))
        _against_restated_fit(res, s, "model")
    # nothing is asserted about a random model's stability: only the flags' range and finite stresses
    assert set(res.status.tolist()) <= {0, 1, 2}
    assert np.isfinite(res.stresses).all()


# --- (5) argument errors ------------------------------------------------------------------------------------------------------------
def _fn(lats, poss):
    raise AssertionError("an argument error must come before any evaluation")


@pytest.mark.parametrize("kw", [
    dict(strains=(-0.01, 0.0, 0.01)), dict(strains=(-0.01, 0.01, 0.01)), dict(strain_set=0.01 * np.eye(6)),
    dict(strains=(-0.01, 0.01), strain_set=ref.SEVEN), dict(steps=5), dict(fmax=0.05),
], ids=lambda kw: ",".join(kw))
def test_argument_errors_come_before_any_launch(kw):
    lat, pos = defects_ref.fcc(4.0)
    with pytest.raises(ValueError):
        elastic_tensor(None, [lat], [pos], forces_fn=_fn, device=DEV, **kw)


def test_a_model_without_stresses_is_refused():
    lats, pos, feats = _crystals(1, 6)
    with pytest.raises(ValueError, match="stresses"):
        elastic_tensor(_model(stresswise_weight=0.0), lats, pos, feats)
