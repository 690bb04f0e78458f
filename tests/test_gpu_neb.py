"""The nudged elastic band on the device (csrc/neb.hip, alignn_amd/neb.py) against the restatements of tests/neb_ref.py: (a) the
interpolation bit for bit; (b) ``alignn_neb_forces`` on hand-made random bands, every tangent branch, alone and in a batch; (c)
``neb`` end to end on the pair potential of tests/pair_ref.py against ``run_neb_ref`` - a vacancy hop in fcc, symmetric and
not; (d) the model path: the same bits as a direct ``relax`` on the images, in chunks and per band; (e) the host checks that sit
behind the ones tests/test_neb_ref.py reaches without a GPU."""

import ctypes as C

import numpy as np
import pytest
import torch

from alignn_amd import _lib
from alignn_amd.neb import METHODS, NebArgs, _load, neb, neb_interpolate
from alignn_amd.relax import relax
from tests import neb_ref as ref
from tests import pair_ref
from tests.sim_gpu import DEV, _close, _crystals, _model, _t

pytestmark = pytest.mark.gpu

RC, vacancy_hop = ref.RC, ref.vacancy_hop


# --- (a) the interpolation ----------------------------------------------------------------------------------------------------------
def _interpolation_bands():
    rng = np.random.default_rng(21)
    bands = []
    cell = ref.triclinic(rng)
    bands.append((cell, rng.uniform(0, 1, (1, 3)) @ cell, rng.uniform(0, 1, (1, 3)) @ cell, 3))
    cell = ref.triclinic(rng, 9.0)
    first = rng.uniform(0, 1, (31, 3)) @ cell
    bands.append((cell, first, first + rng.normal(0, 0.6, (31, 3)), 5))
    # dyadic entries and a determinant of 32: the fractional differences below are exact
    cell = np.array([[4.0, 0.0, 0.0], [1.0, 4.0, 0.0], [0.5, 1.0, 2.0]])
    f0 = np.round(rng.uniform(0, 1, (70, 3)) * 64) / 64
    df = np.round(rng.uniform(-0.3, 0.3, (70, 3)) * 64) / 64
    df[:6] = [[0.5, 0, 0], [-0.5, 0, 0], [0, 1.5, 0], [0, -1.5, 0.25], [0.25, 0, 2.5], [0.5, -0.5, 0.5]]
    f0[6:12, 0], df[6:12, 0] = 0.96875, 0.125  # six atoms that leave through the +a face ...
    f1 = f0 + df
    f1[6:12] -= np.floor(f1[6:12])  # ... and are given on the far side
    bands.append((cell, f0 @ cell, f1 @ cell, 64))
    return bands


def test_interpolation_matches_the_restatement_bit_for_bit():
    bands = _interpolation_bands()
    cell, first, last, M = bands[2]
    frac = (last - first) @ np.linalg.inv(cell)
    assert np.array_equal(frac[:3], [[0.5, 0, 0], [-0.5, 0, 0], [0, 1.5, 0]]) and np.array_equal(frac[5], [0.5, -0.5, 0.5])
    assert (np.abs(frac[6:12, 0]) > 0.5).all()  # across a face: the wrap takes a lattice vector out
    ns, Ms = [len(b[1]) for b in bands], [b[3] for b in bands]
    rows, inv = neb_interpolate(_t(np.stack([b[0] for b in bands])), _t(np.concatenate([b[1] for b in bands])),
                                _t(np.concatenate([b[2] for b in bands])), ns, Ms)
    got = torch.split(rows, [(m - 2) * n for m, n in zip(Ms, ns)])
    for b, (cell, first, last, M) in enumerate(bands):
        want = ref.interpolate(first, last, cell, M)
        g = got[b].cpu().numpy().reshape(M - 2, ns[b], 3)
        assert np.array_equal(g, want), (b, np.abs(g - want).max())
        assert np.array_equal(inv[b].cpu().numpy(), ref.inv3_cof(cell)), b
        alone, _ = neb_interpolate(_t(cell[None]), _t(first), _t(last), [ns[b]], [M])
        assert torch.equal(alone, got[b]), b
    step = ref.mic(bands[2][2] - bands[2][1], bands[2][0])
    assert (ref.row_dot(step, ref.inv3_cof(bands[2][0]))[6:12, 0] == 0.125).all()  # the short way: +1/8 along a, not -7/8


# --- (b) alignn_neb_forces ----------------------------------------------------------------------------------------------------------
def _energies(rng, M, kind):
    """Band energies with a set shape: one hump, or several humps and dips (every branch of the improved tangent)."""
    x = np.linspace(0.0, 1.0, M)
    if kind == "hump":
        E = np.sin(np.pi * x) + 0.3 * x
    elif kind == "late":  # the maximum in the last interior image: images below imax only
        E = x * (x < 1.0) * 1.3
    elif kind == "early":  # ... in the first one: images above imax only
        E = (1.0 - x) * (x > 0.0) * 1.3
    else:
        E = np.sin(3.5 * np.pi * x) * (1.0 + x) + 0.2 * x
    return E + rng.uniform(-0.01, 0.01, M)


# (n, M, the shape of the energies, the spring constant)
BANDS = [(1, 3, "hump", 0.1), (63, 4, "late", 0.25), (64, 64, "waves", 0.05), (65, 4, "early", 1.5), (300, 3, "hump", 0.4),
         (300, 64, "waves", 0.1), (64, 4, "hump", 0.7)]


def _hand_made():
    rng = np.random.default_rng(4)
    out = []
    for n, M, kind, k in BANDS:
        cell = ref.triclinic(rng, 7.0)
        R, F = ref.random_band(rng, n, M, cell, pushed=(1,) if M == 3 else (1, M - 2))
        fixed = rng.uniform(0, 1, n) < 0.25
        out.append(dict(n=n, M=M, k=k, cell=cell, R=R, F=F, E=_energies(rng, M, kind), fixed=fixed))
    return out


def _launch(bands, active, method, climb, with_fixed):
    """One alignn_neb_forces launch on a batch of hand-made bands -> per active band (F [M - 2, n, 3], imax, emax), and the
    full-batch image energies."""
    B = len(bands)
    pre = lambda c: torch.tensor(np.concatenate([[0], np.cumsum(c)]), dtype=torch.int32, device=DEV)
    rows = [(b["M"] - 2) * b["n"] for b in bands]
    frows = [b["F"].size // 3 for b in bands]  # (the rows' number unless a test hands over forces of another shape)
    t = dict(
        forces=_t(np.concatenate([bands[s]["F"].reshape(-1, 3) for s in active])),
        energy=_t(np.concatenate([bands[s]["E"][1:-1] for s in active])),
        force_ptr=pre([frows[s] for s in active]), energy_ptr=pre([bands[s]["M"] - 2 for s in active]),
        active=torch.tensor(active, dtype=torch.int32, device=DEV), row_ptr=pre(rows), image_ptr=pre([b["M"] for b in bands]),
        end_ptr=pre([b["n"] for b in bands]), lattice=_t(np.stack([b["cell"] for b in bands])),
        inv_lattice=_t(np.stack([ref.inv3_cof(b["cell"]) for b in bands])), spring=_t([b["k"] for b in bands]),
        initial=_t(np.concatenate([b["R"][0] for b in bands])), final=_t(np.concatenate([b["R"][-1] for b in bands])),
        end_energy=_t(np.array([[b["E"][0], b["E"][-1]] for b in bands])),
        positions=_t(np.concatenate([b["R"][1:-1].reshape(-1, 3) for b in bands])),
        energies_out=torch.full((sum(b["M"] for b in bands),), -7.0, dtype=torch.float64, device=DEV),
        imax=torch.full((len(active),), -7, dtype=torch.int32, device=DEV),
        emax=torch.full((len(active),), -7.0, dtype=torch.float64, device=DEV))
    t["forces_out"] = torch.full_like(t["forces"], -7.0)
    if with_fixed:
        t["fixed"] = torch.tensor(np.concatenate([np.tile(b["fixed"], b["M"] - 2) for b in bands]).astype(np.uint8), device=DEV)
    args = NebArgs(n_active=len(active), max_images=max(bands[s]["M"] for s in active), method=METHODS[method], climb=int(climb),
                   **{k: v.data_ptr() for k, v in t.items()})
    _lib.check(_load().alignn_neb_forces(C.byref(args), _lib.stream()), "neb_forces")
    F = torch.split(t["forces_out"], [frows[s] for s in active])
    imax, emax = t["imax"].cpu().numpy(), t["emax"].cpu().numpy()
    return ([(F[k].cpu().numpy().reshape(bands[s]["M"] - 2, -1, 3), int(imax[k]), float(emax[k]))
             for k, s in enumerate(active)], t["energies_out"].cpu().numpy())


def test_hand_made_bands_cover_every_branch_and_do_not_cancel():
    """The host-side premises of the comparison below (checked on the GPU machine too, before it)."""
    bands = _hand_made()
    seen, sides = set(), set()
    for b in bands:
        imax = 1 + int(np.argmax(b["E"][1:-1]))
        for i in range(1, b["M"] - 1):
            seen.add(ref.branch(b["E"], i))
            sides.add(np.sign(i - imax))
        for method in ref.METHODS:
            assert ref.cancellation(b["R"], b["E"], method, b["cell"]).min() >= 0.1, (b["n"], b["M"], method)
    assert seen >= {"rising", "falling", "max up", "max down", "min up", "min down"} and sides == {-1, 0, 1}
    assert {b["n"] for b in bands} == {1, 63, 64, 65, 300} and {b["M"] for b in bands} == {3, 4, 64}


@pytest.mark.parametrize("with_fixed", [False, True])
@pytest.mark.parametrize("climb", [False, True])
@pytest.mark.parametrize("method", ref.METHODS)
def test_neb_forces_match_the_restatement(method, climb, with_fixed):
    test_hand_made_bands_cover_every_branch_and_do_not_cancel()
    bands = _hand_made()
    got, energies = _launch(bands, list(range(len(bands))), method, climb, with_fixed)
    at = np.concatenate([[0], np.cumsum([b["M"] for b in bands])])
    for s, b in enumerate(bands):
        want, imax = ref.neb_forces(b["R"], b["E"], b["F"], b["k"], climb, method, b["fixed"] if with_fixed else None,
                                    cell=b["cell"])
        F, imax_got, emax = got[s]
        assert imax_got == imax and emax == b["E"][imax]
        assert np.array_equal(energies[at[s]:at[s + 1]], b["E"])
        for i in range(b["M"] - 2):
            err = np.abs(F[i] - want[i]).max() / (np.abs(want[i]).max() or 1.0)
            if err > 1e-13:
                print(f"n {b['n']} M {b['M']} image {i + 1}: rel err {err:.2e}")
            assert np.abs(F[i] - want[i]).max() <= 1e-12 * np.abs(want[i]).max(), (b["n"], b["M"], i + 1)
            assert _close(F[i], want[i])


@pytest.mark.parametrize("method", ref.METHODS)
def test_neb_forces_of_a_band_do_not_depend_on_the_launch(method):
    bands = _hand_made()
    whole, _ = _launch(bands, list(range(len(bands))), method, True, True)
    # two active bands of a batch of three: the middle one has retired
    three = [bands[5], bands[0], bands[3]]
    part, energies = _launch(three, [0, 2], method, True, True)
    assert np.array_equal(part[0][0], whole[5][0]) and np.array_equal(part[1][0], whole[3][0])
    assert (part[0][1], part[1][1]) == (whole[5][1], whole[3][1])
    assert (energies[64:67] == -7.0).all() and np.array_equal(energies[:64], bands[5]["E"])  # the retired band's stay
    for s in (0, 2, 4, 5):
        alone, _ = _launch([bands[s]], [0], method, True, True)
        assert np.array_equal(alone[0][0], whole[s][0]) and alone[0][1:] == whole[s][1:], s


def test_neb_forces_flags_rows_that_do_not_fit():
    bands = _hand_made()[:2]
    bands[1] = dict(bands[1], F=bands[1]["F"][:, :-1])  # force rows of another count than the band's
    got, _ = _launch(bands, [0, 1], "aseneb", False, False)
    assert got[0][1] == 1 and got[1][1] == -1 and (got[1][0] == -7.0).all()


# --- (c) end to end on the pair potential ---------------------------------------------------------------------------------------
_RUNS = {}


def _ef(cell):
    efs = pair_ref.make_efs(RC)
    return lambda p: efs(cell, p)[:2]


def _cases():
    if "cases" not in _RUNS:
        _RUNS["cases"] = [vacancy_hop(False), vacancy_hop(True)]
    return _RUNS["cases"]


def _run(method, climb, steps, which=(0, 1), fixed=None):
    key = (method, climb, steps, which, fixed is not None)
    if key not in _RUNS:
        cs = [_cases()[c] for c in which]
        _RUNS[key] = neb(None, [c[0] for c in cs], [c[1] for c in cs], [c[2] for c in cs], n_images=3, k=0.1, climb=climb,
                         method=method, fmax=0.05, steps=steps, fixed=fixed, forces_fn=pair_ref.make_forces_fn(RC, stress=False),
                         device=DEV)
    return _RUNS[key]


def _want(case, method, climb, steps, fixed=None):
    key = ("ref", case, method, climb, steps, fixed is not None)
    if key not in _RUNS:
        cell, first, last = _cases()[case]
        _RUNS[key] = ref.run_neb_ref(cell, first, last, _ef(cell), 3, 0.1, climb, method, 0.05, steps, fixed)
    return _RUNS[key]


def _like_the_restated_run(res, b, want, what):
    got = res.positions[b].cpu().numpy()
    print(f"{what}: max |dpos| {np.abs(got - want['r']).max():.3e}, max |dE| {np.abs(res.energies[b] - want['e']).max():.3e}, "
          f"steps {int(res.n_steps[b])} vs {want['n_steps']}, margins {want['margins']}")
    assert np.abs(got - want["r"]).max() <= 1e-10 * max(1.0, np.abs(want["r"]).max()), what
    assert res.energies[b] == pytest.approx(want["e"], rel=1e-9, abs=1e-12), what
    assert int(res.n_steps[b]) == want["n_steps"] and bool(res.converged[b]) == want["converged"], what
    assert res.imax[b] == want["imax"], what
    assert res.barrier[b] == res.energies[b].max() - res.energies[b][0] and res.delta_e[b] == res.energies[b][-1] - res.energies[b][0]


def _margins_hold(want, case, what):
    """No energy comparison of the restated run is closer than 1e-6 eV, so the device run takes the same branches.  The one
    exception is the symmetric case's middle image under the improved tangent: E[3] and E[1] tie to rounding there by symmetry,
    and so do dmax and dmin, so both orders give the same tangent t1 + t2 (times dmax) to rounding."""
    kinds = {k: v for k, v in want["margins"].items() if not (case == 0 and k == "across")}
    assert kinds and min(kinds.values()) >= 1e-6, (what, want["margins"])
    if case == 0 and "across" in want["margins"]:
        assert abs(want["e"][3] - want["e"][1]) <= 1e-9


@pytest.mark.parametrize("climb", [False, True])
@pytest.mark.parametrize("method", ref.METHODS)
def test_neb_after_five_steps_matches_the_restated_run(method, climb):
    which = (0, 1) if not climb else (1,)  # both cases in one call; the climbing image on the asymmetric one
    res = _run(method, climb, 5, which)
    assert res.n_evals == 6
    for b, case in enumerate(which):
        want = _want(case, method, climb, 5)
        _margins_hold(want, case, (method, climb, case))
        _like_the_restated_run(res, b, want, (method, climb, "case " + "AB"[case]))
        f = res.forces[b].cpu().numpy()
        # positions within 1e-10 A, a stiffness below 2 D alpha^2 = 2 eV/A^2 for each of 12 neighbours: 2.5e-9 eV/A
        assert f.shape == (3, 31, 3) and np.abs(f - want["f"]).max() <= 2.5e-9


@pytest.mark.parametrize("method", ref.METHODS)
def test_neb_converges_to_the_restated_barrier(method):
    res = _run(method, False, 60)
    climbed = _run(method, True, 60, (1,))
    for b in range(2):
        want = _want(b, method, False, 60)
        _margins_hold(want, b, (method, b))
        assert bool(res.converged[b]) and want["converged"] and int(res.n_steps[b]) == want["n_steps"] <= 30
        assert float(res.fmax[b]) < 0.05
        assert res.barrier[b] == pytest.approx(want["barrier"], rel=1e-9)
    assert res.imax[0] == 2 and res.barrier[0] > 0.05
    want = _want(1, method, True, 60)
    assert bool(climbed.converged[0]) and climbed.barrier[0] == pytest.approx(want["barrier"], rel=1e-9)
    assert not np.array_equal(climbed.energies[0][1:-1], res.energies[1][1:-1])  # the climbing image changes the path ...
    assert not np.array_equal(want["e"][1:-1], _want(1, method, False, 60)["e"][1:-1])  # ... as the restatement's does
    assert np.array_equal(climbed.energies[0][[0, -1]], res.energies[1][[0, -1]])


def test_neb_holds_fixed_atoms_in_every_image():
    fixed = np.zeros(31, dtype=bool)
    fixed[[9, 17, 23, 30]] = True  # four spectators (neither the hopping atom, row 0, nor the displaced row 5)
    res = _run("aseneb", False, 5, (1,), [fixed])
    want = _want(1, "aseneb", False, 5, fixed)
    _like_the_restated_run(res, 0, want, "fixed")
    cell, first, last = _cases()[1]
    start = ref.interpolate(first, last, cell, 5)
    got = res.positions[0].cpu().numpy()
    assert np.array_equal(got[1:-1][:, fixed], start[:, fixed]) and not np.array_equal(got[1:-1][:, ~fixed], start[:, ~fixed])
    free = _run("aseneb", False, 5, (1,))
    assert not torch.equal(free.positions[0], res.positions[0])


@pytest.mark.parametrize("method", ref.METHODS)
def test_a_band_alone_gives_the_bits_it_has_beside_another(method):
    both, alone = _run(method, False, 5), _run(method, False, 5, (1,))
    assert torch.equal(alone.positions[0], both.positions[1]) and np.array_equal(alone.energies[0], both.energies[1])
    assert torch.equal(alone.forces[0], both.forces[1]) and int(alone.n_steps[0]) == int(both.n_steps[1])


def test_bands_of_different_lengths_and_springs_in_one_call():
    cs = _cases()
    fn = pair_ref.make_forces_fn(RC, stress=False)
    res = neb(None, [c[0] for c in cs], [c[1] for c in cs], [c[2] for c in cs], n_images=[1, 3], k=[0.3, 0.1], steps=5,
              forces_fn=fn, device=DEV)
    assert [tuple(p.shape) for p in res.positions] == [(3, 31, 3), (5, 31, 3)] and res.imax.tolist() == [1, 2]
    both = _run("aseneb", False, 5)
    assert torch.equal(res.positions[1], both.positions[1])
    cell, first, last = cs[0]
    want = ref.run_neb_ref(cell, first, last, _ef(cell), 1, 0.3, False, "aseneb", 0.05, 5)
    _like_the_restated_run(res, 0, want, "one interior image")


# --- (d) the model path -------------------------------------------------------------------------------------------------------------
_MODEL_KW = dict(n_images=3, steps=2, fmax=0.0)


def _model_case():
    if "model" not in _RUNS:
        model = _model()
        lats, pos, feats = _crystals(2, 6)
        pos = [np.asarray(p, dtype=np.float64) for p in pos]
        last = []
        for s, p in enumerate(pos):
            q = p.copy()
            q[s + 1] += np.array([0.4, 0.0, 0.0])  # one atom displaced by 0.4 A
            last.append(q)
        _RUNS["model"] = (model, lats, pos, last, feats, neb(model, lats, pos, last, feats, **_MODEL_KW))
    return _RUNS["model"]


def test_neb_model_path_equals_a_direct_relax_on_its_images():
    model, lats, pos, last, feats, res = _model_case()
    assert res.n_steps.tolist() == [2, 2] and res.n_evals == 3
    cells, images, fs = [], [], []
    for b in range(2):
        for j in range(1, 4):
            cells.append(lats[b])
            images.append(res.positions[b][j])
            fs.append(feats[b])
    direct = relax(model, cells, images, fs, steps=0)
    e = direct.energies.cpu().numpy()
    got = np.concatenate([res.energies[b][1:-1] for b in range(2)])
    print("neb vs direct relax on the images: max |dE|", np.abs(e - got).max(), "of", np.abs(e).max())
    assert np.array_equal(e, got)
    ends = relax(model, lats * 2, pos + last, feats * 2, steps=0).energies.cpu().numpy()
    assert np.array_equal(ends, np.array([res.energies[0][0], res.energies[1][0], res.energies[0][-1], res.energies[1][-1]]))
    for b in range(2):
        assert np.array_equal(res.positions[b][0].cpu().numpy(), pos[b]) and np.array_equal(res.positions[b][-1].cpu().numpy(), last[b])


def _same_as_the_whole_call(other, k, res, b, what):
    print(f"{what}, band {b}: max |dE| {np.abs(other.energies[k] - res.energies[b]).max():.3e}")
    assert np.array_equal(other.energies[k], res.energies[b]), what
    assert torch.equal(other.positions[k], res.positions[b]) and torch.equal(other.forces[k], res.forces[b]), what


def test_neb_model_path_in_chunks_gives_the_whole_calls_bits():
    model, lats, pos, last, feats, res = _model_case()
    chunked = neb(model, lats, pos, last, feats, max_atoms_per_eval=7, **_MODEL_KW)
    for b in range(2):
        _same_as_the_whole_call(chunked, b, res, b, "in chunks")


def test_neb_model_path_per_band_gives_the_whole_calls_bits():
    model, lats, pos, last, feats, res = _model_case()
    for b in range(2):
        alone = neb(model, lats[b:b + 1], pos[b:b + 1], last[b:b + 1], feats[b:b + 1], **_MODEL_KW)
        _same_as_the_whole_call(alone, 0, res, b, "per band")


# --- (e) the host checks behind the device ------------------------------------------------------------------------------------------
def _never(*a, **k):
    raise AssertionError("device work before the checks")


def test_neb_refuses_coinciding_endpoints_and_a_wrong_fixed_mask():
    cell, first, last = _cases()[0]
    shifted = first + 2.0 * cell[0] - cell[2]  # the same structure, whole lattice vectors away
    with pytest.raises(ValueError, match="coincide"):
        neb(None, [cell], [first], [shifted], forces_fn=_never, device=DEV)
    with pytest.raises(ValueError, match="coincide"):
        neb(None, [cell], [first], [first.copy()], forces_fn=_never, device=DEV)
    for bad in ([np.zeros(30, dtype=bool)], [np.zeros(31)], [None, None], np.zeros((1, 30), dtype=bool)):
        with pytest.raises(ValueError, match="fixed"):
            neb(None, [cell], [first], [last], fixed=bad, forces_fn=_never, device=DEV)


@pytest.mark.parametrize("kw", [dict(final="short"), dict(n_images=0), dict(n_images=63), dict(k=0.0), dict(k=float("nan")),
                                dict(method="string")])
def test_neb_checks_come_before_any_launch(kw):
    cell, first, last = _cases()[0]
    final = [last[:-1]] if kw.pop("final", None) else [last]
    with pytest.raises(ValueError, match="neb"):
        neb(None, [cell], [first], final, forces_fn=_never, device=DEV, **kw)
