"""The E-V curve task on the device (csrc/eos.hip, alignn_amd/eos.py) against the restatements of tests/eos_ref.py: (1) the
strain builder bit for bit, alone and in a batch, isotropic and sheared; (2) the equation-of-state fit on exact, noisy and
concave curves of mixed lengths in one launch; (3) ``ev_curve`` on the pair potential of tests/pair_ref.py, as given and on
relaxed parents; (4) the model path: the same bits as a direct ``relax`` on the restated structures, and in groups."""

import numpy as np
import pytest
import torch

from alignn_amd import _lib, eos_fit, ev_curve
from alignn_amd.relax import relax
from alignn_amd.synthetic import make_crystal
from tests import defects_ref
from tests import eos_ref as ref
from tests import pair_ref
from tests.sim_gpu import DEV, _crystals, _model

pytestmark = pytest.mark.gpu

RC = 5.0
# The largest deviation of a fit parameter between the kernel and the restated fit, measured on the inputs of
# test_eos_fit_matches_the_restatement (MI355X): 0 - the kernel's log and exp are the restatement's, operation for operation, and
# every sum has its order, so the parameters, rms, step counts and flags came out as the same bits.  10 x 0 is 0: equality.
FIT_RTOL = 0.0
SENTINEL = -7.0


def _triclinic():
    lat, frac, _ = make_crystal(6, 77)
    lat = np.asarray(lat, dtype=np.float64)
    return lat, np.asarray(frac, dtype=np.float64) @ lat


# --- (1) the builder ------------------------------------------------------------------------------------------------------------------
def _strain_build(pos, atom_ptr, lat, B, jobs, Fs, counts):
    lib = _lib.load()
    off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    J = len(jobs)
    cells = torch.full((J, 3, 3), SENTINEL, dtype=torch.float64, device=DEV)
    cart = torch.full((int(off[-1]), 3), SENTINEL, dtype=torch.float64, device=DEV)
    vol = torch.full((J,), SENTINEL, dtype=torch.float64, device=DEV)
    jobs_d = torch.tensor(jobs, dtype=torch.int32, device=DEV)
    F_d = torch.tensor(np.stack(Fs), dtype=torch.float64, device=DEV)
    off_d = torch.tensor(off, dtype=torch.int64, device=DEV)
    _lib.check(lib.alignn_strain_build(pos.data_ptr(), atom_ptr.data_ptr(), lat.data_ptr(), B, jobs_d.data_ptr(), F_d.data_ptr(),
                                       off_d.data_ptr(), J, cells.data_ptr(), cart.data_ptr(), vol.data_ptr(), _lib.stream()),
               "strain_build")
    return cells.cpu().numpy(), cart.cpu().numpy(), vol.cpu().numpy(), off


def test_strain_builder_matches_the_restatement_bit_for_bit():
    ps = [defects_ref.fcc(4.0), _triclinic()]
    ptr = np.concatenate([[0], np.cumsum([len(p) for _, p in ps])])
    pos = torch.tensor(np.concatenate([p for _, p in ps]), device=DEV)
    atom_ptr = torch.tensor(ptr, dtype=torch.int32, device=DEV)
    lat = torch.tensor(np.stack([l for l, _ in ps]), device=DEV)
    shear = np.array([[1.01, 0.03, -0.015], [0.02, 0.97, 0.04], [-0.025, 0.01, 1.02]])
    jobs, Fs, counts = [], [], []
    for s, (_, p) in enumerate(ps):
        for F in [ref.isotropic(dx) for dx in (-0.05, 0.0, 0.04)] + [shear]:
            jobs.append(s)
            Fs.append(F)
            counts.append(len(p))
    jobs.append(2)  # no such parent: nothing is written
    Fs.append(np.eye(3))
    counts.append(3)
    cells, cart, vol, off = _strain_build(pos, atom_ptr, lat, 2, jobs, Fs, counts)
    for k, (s, F) in enumerate(zip(jobs[:-1], Fs)):
        want = ref.strain(ps[s][0], ps[s][1], F)
        got = (cells[k], cart[off[k]:off[k + 1]], vol[k])
        for name, g, w in zip(("cell", "cart", "volume"), got, want):
            assert np.shape(g) == np.shape(w) and np.array_equal(g, w), (k, name, np.abs(g - w).max())
        c1, r1, v1, _ = _strain_build(pos, atom_ptr, lat, 2, [s], [F], [counts[k]])
        assert np.array_equal(c1[0], got[0]) and np.array_equal(r1, got[1]) and v1[0] == got[2], ("alone", k)
    assert (cells[-1] == SENTINEL).all() and (cart[off[-2]:] == SENTINEL).all() and vol[-1] == SENTINEL
    # the isotropic volumes are (1 + dx)^3 V to rounding, the shear's |det F| V
    v0 = [abs(np.linalg.det(l)) for l, _ in ps]
    assert vol[1] == pytest.approx(v0[0], rel=1e-15) and vol[4 + 2] == pytest.approx(1.04 ** 3 * v0[1], rel=1e-14)
    assert vol[3] == pytest.approx(abs(np.linalg.det(shear)) * v0[0], rel=1e-14)


# --- (2) the fit ----------------------------------------------------------------------------------------------------------------------
def _fit_sets(form):
    sets = dict(ref.synthetic_sets(form))
    sets["concave"] = ref.concave()
    return sets


def _launch(sets, form, ld=None):
    """One launch over ``sets`` (a list of (V, E)) padded to ``ld`` points with the sentinel -> numpy (params, rms, n_iter,
    status)."""
    B, ld = len(sets), ld or max(len(V) for V, _ in sets)
    vol = np.full((B, ld), SENTINEL)
    en = np.full((B, ld), SENTINEL)
    for s, (V, E) in enumerate(sets):
        vol[s, :len(V)], en[s, :len(V)] = V, E
    n = torch.tensor([len(V) for V, _ in sets], dtype=torch.int32, device=DEV)
    out = eos_fit(torch.tensor(vol, device=DEV), torch.tensor(en, device=DEV), {v: k for k, v in ref.FORMS.items()}[form], n)
    return [t.cpu().numpy() for t in out]


def _same(a, b):
    return np.array_equal(a, b, equal_nan=True)


@pytest.mark.parametrize("form", [ref.MURNAGHAN, ref.BIRCH_MURNAGHAN])
def test_eos_fit_matches_the_restatement(form):
    """One launch of B = 7 with K = 10, 10, 5, 5, 4, 4, 5: the exact curve on ten, five and four points, each also with 1e-4
    noise, and the concave curve (status 2, NaN) in the last place.  Measured on an MI355X, both forms: parameters and rms equal
    to the restated fit's bit for bit (largest relative deviation 0), n_iter and status equal (5 or 6 steps, status 0; the
    concave one 0 steps, status 2); each structure alone the batch's bits."""
    sets = _fit_sets(form)
    names, data = list(sets), list(sets.values())
    assert sorted(len(V) for V, _ in data) == [4, 4, 5, 5, 5, 10, 10]
    params, rms, n_iter, status = _launch(data, form)
    worst = 0.0
    for s, name in enumerate(names):
        want = ref.fit(*data[s], form)
        print(f"form {form} {name}: device {params[s]!r} rms {rms[s]:.3e} n_iter {n_iter[s]} status {status[s]}; "
              f"restated {want['params']!r} rms {want['rms']:.3e} n_iter {want['n_iter']} status {want['status']}")
        assert status[s] == want["status"] and n_iter[s] == want["n_iter"], name
        if want["status"] == 2:
            assert name == "concave" and np.isnan(params[s]).all() and np.isnan(rms[s])
            continue
        dev = float(np.max(np.abs(params[s] - want["params"]) / np.abs(want["params"])))
        worst = max(worst, dev)
        assert dev <= FIT_RTOL, (name, dev)
        assert abs(rms[s] - want["rms"]) <= FIT_RTOL * want["rms"], name
        if "noise" not in name:
            assert np.max(np.abs(params[s] - np.array(ref.TRUE)) / np.abs(ref.TRUE)) <= 1e-10, name
    print(f"form {form}: largest relative deviation of a parameter, kernel vs restatement: {worst:.3e}")
    for s in range(len(data)):  # alone, in a launch of its own length, and shifted to another place of the batch
        alone = _launch([data[s]], form)
        rolled = _launch(data[s:] + data[:s], form)
        for got, one, rol in zip((params, rms, n_iter, status), alone, rolled):
            assert _same(one[0], got[s]) and _same(rol[0], got[s]), names[s]


def test_eos_fit_rejects_what_it_cannot_fit():
    V, E = ref.synthetic_sets()["k5"]
    # fewer points than parameters, more than the row holds: status 2, the neighbour untouched by it
    vol = torch.tensor(np.stack([V, V, V]), device=DEV)
    en = torch.tensor(np.stack([E, E, E]), device=DEV)
    n = torch.tensor([3, 5, 6], dtype=torch.int32, device=DEV)
    params, rms, n_iter, status = [t.cpu().numpy() for t in eos_fit(vol, en, "murnaghan", n)]
    assert status.tolist() == [2, 0, 2] and n_iter[0] == 0 and n_iter[2] == 0
    assert np.isnan(params[[0, 2]]).all() and np.isnan(rms[[0, 2]]).all()
    assert _same(params[1], ref.fit(V, E)["params"])
    lib = _lib.load()
    out = torch.empty(8, dtype=torch.float64, device=DEV)
    bad = dict(ld=[3, 65], form=[2, -1])
    for ld in bad["ld"]:
        assert lib.alignn_eos_fit(vol.data_ptr(), en.data_ptr(), None, 1, ld, 0, out.data_ptr(), out.data_ptr(), out.data_ptr(),
                                  out.data_ptr(), _lib.stream()) != 0
    for form in bad["form"]:
        assert lib.alignn_eos_fit(vol.data_ptr(), en.data_ptr(), None, 1, 5, form, out.data_ptr(), out.data_ptr(), out.data_ptr(),
                                  out.data_ptr(), _lib.stream()) != 0
    with pytest.raises(ValueError):
        eos_fit(vol, en, "vinet")
    with pytest.raises(ValueError):
        eos_fit(vol[:, :3], en[:, :3])


# --- (3) ev_curve on the pair potential -------------------------------------------------------------------------------------------------
_FIELDS = ("volumes", "energies", "e0", "b0", "bp", "v0", "bulk_modulus_GPa", "rms", "n_iter", "status")


def _same_result(a, s, b, t, what):
    for f in _FIELDS:
        assert _same(getattr(a, f)[s], getattr(b, f)[t]), (what, f)
    assert torch.equal(a.lattices[s], b.lattices[t]) and torch.equal(a.positions[s], b.positions[t]), what


_CACHE = {}


def _pair_case():
    if not _CACHE:
        parents = [defects_ref.fcc(3.9), defects_ref.fcc(4.0)]
        lats, pos = [l for l, _ in parents], [p for _, p in parents]
        _CACHE["pair"] = (lats, pos, ev_curve(None, lats, pos, forces_fn=pair_ref.make_forces_fn(RC, stress=False), device=DEV))
    return _CACHE["pair"]


def test_ev_curve_on_a_pair_potential():
    lats, pos, res = _pair_case()
    efs = pair_ref.make_efs(RC)
    assert np.array_equal(res.dx, ref.DX_DEFAULT) and res.volumes.shape == res.energies.shape == (2, 10)
    assert res.n_eval_calls == 1
    for s in range(2):
        built = [ref.strain(lats[s], pos[s], ref.isotropic(dx)) for dx in res.dx]
        assert np.array_equal(res.volumes[s], np.array([b[2] for b in built]))
        want_e = np.array([efs(b[0], b[1])[0] for b in built])
        print(f"parent {s}: max rel |dE| {np.max(np.abs(res.energies[s] - want_e) / np.abs(want_e)):.3e}")
        assert res.energies[s] == pytest.approx(want_e, rel=1e-9)
        want = ref.fit(res.volumes[s], res.energies[s], ref.MURNAGHAN)
        got = np.array([res.e0[s], res.b0[s], res.bp[s], res.v0[s]])
        print(f"parent {s}: device {got!r} restated {want['params']!r}, n_iter {res.n_iter[s]} / {want['n_iter']}")
        assert np.max(np.abs(got - want["params"]) / np.abs(want["params"])) <= FIT_RTOL
        assert abs(res.rms[s] - want["rms"]) <= FIT_RTOL * want["rms"]
        assert res.status[s] == 0 == want["status"] and res.n_iter[s] == want["n_iter"]
        assert res.bulk_modulus_GPa[s] == res.b0[s] * 160.21766208
        assert res.volumes[s].min() < res.v0[s] < res.volumes[s].max() and res.b0[s] > 0
        assert np.array_equal(res.lattices[s].cpu().numpy(), lats[s]) and np.array_equal(res.positions[s].cpu().numpy(), pos[s])


def test_ev_curve_per_parent_gives_the_calls_bits():
    lats, pos, res = _pair_case()
    fn = pair_ref.make_forces_fn(RC, stress=False)
    for s in range(2):
        alone = ev_curve(None, lats[s:s + 1], pos[s:s + 1], forces_fn=fn, device=DEV)
        _same_result(alone, 0, res, s, ("alone", s))
    bm = ev_curve(None, lats, pos, forces_fn=fn, device=DEV, eos="birchmurnaghan")
    for s in range(2):
        want = ref.fit(bm.volumes[s], bm.energies[s], ref.BIRCH_MURNAGHAN)
        assert np.array_equal(bm.energies[s], res.energies[s]) and bm.status[s] == 0 and bm.n_iter[s] == want["n_iter"]
        got = np.array([bm.e0[s], bm.b0[s], bm.bp[s], bm.v0[s]])
        assert np.max(np.abs(got - want["params"]) / np.abs(want["params"])) <= FIT_RTOL


def test_ev_curve_on_relaxed_parents_is_ev_curve_on_a_direct_relax():
    lats, pos, _ = _pair_case()
    pos = [p + np.random.default_rng(5 + s).normal(0.0, 0.03, p.shape) for s, p in enumerate(pos)]  # (forces to relax along)
    fn = pair_ref.make_forces_fn(RC, stress=True)
    kw = dict(steps=3, fmax=0.0)
    res = ev_curve(None, lats, pos, forces_fn=fn, device=DEV, on_relaxed_struct=True, **kw)
    direct = relax(None, lats, pos, forces_fn=fn, device=DEV, optimize_lattice=True, **kw)
    assert direct.n_steps.tolist() == [3, 3]
    assert not torch.equal(direct.lattices.cpu(), torch.tensor(np.stack(lats)))
    want = ev_curve(None, list(direct.lattices), direct.positions, forces_fn=pair_ref.make_forces_fn(RC, stress=False), device=DEV)
    for s in range(2):
        _same_result(res, s, want, s, ("relaxed", s))
        assert torch.equal(res.lattices[s], direct.lattices[s]) and torch.equal(res.positions[s], direct.positions[s])


# --- (4) a random-initialised ALIGNNAtomWise -----------------------------------------------------------------------------------------
def test_ev_curve_model_path_equals_a_direct_relax_and_in_groups():
    model = _model()
    lats, pos, feats = _crystals(2, 6)
    dx = (-0.02, 0.0, 0.01, 0.03)
    res = ev_curve(model, lats, pos, feats, dx=dx)
    assert res.n_eval_calls == 1
    built, fs = [], []
    for s in range(2):
        for d in dx:
            built.append(ref.strain(np.asarray(lats[s], dtype=np.float64), np.asarray(pos[s], dtype=np.float64), ref.isotropic(d)))
            fs.append(feats[s])
    direct = relax(model, [b[0] for b in built], [b[1] for b in built], fs, steps=0)
    e = direct.energies.cpu().numpy().reshape(2, 4)
    print("whole call vs direct relax: max |dE|", np.abs(e - res.energies).max(), "of", np.abs(e).max())
    assert np.array_equal(e, res.energies)
    assert np.array_equal(res.volumes, np.array([b[2] for b in built]).reshape(2, 4))
    grouped = ev_curve(model, lats, pos, feats, dx=dx, max_atoms_per_call=12)
    assert grouped.n_eval_calls > 1
    for s in range(2):
        _same_result(grouped, s, res, s, ("in groups", s))
    # a random model's curve need not have a minimum: only the flags' range and finite curves
    assert set(res.status.tolist()) <= {0, 1, 2}
    assert np.isfinite(res.volumes).all() and np.isfinite(res.energies).all()
