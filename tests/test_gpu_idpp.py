"""The IDPP band initialisation on the device (csrc/idpp.hip, alignn_amd/idpp.py) against the restatements of tests/idpp_ref.py:
(a) ``alignn_idpp_forces`` on hand-made random bands, alone and in a batch, and on a dyadic band with pairs exactly at half a cell
vector; (b) ``idpp_interpolate`` end to end on a turning dimer against ``run_idpp_ref``; (c) ``neb`` from the IDPP path and from
images handed in, on the pair potential of tests/pair_ref.py; (d) the host checks that sit behind the ones
tests/test_idpp_ref.py reaches without a GPU."""

import ctypes as C

import numpy as np
import pytest
import torch

from alignn_amd import _lib
from alignn_amd.idpp import IdppArgs, _load, idpp_forces, idpp_interpolate
from alignn_amd.neb import neb
from tests import idpp_ref as ref
from tests import neb_ref, pair_ref
from tests.sim_gpu import DEV, _t

pytestmark = pytest.mark.gpu

_RUNS = {}


# --- (a) alignn_idpp_forces ---------------------------------------------------------------------------------------------------------
# (n, M, the cell's edge): one atom, one pair, one below / at / above a wavefront's 64 lanes, several strides of the lanes and
# more rows than one workgroup of the energy sum holds
BANDS = [(1, 3, 7.0), (2, 4, 7.0), (63, 4, 9.0), (64, 64, 9.0), (65, 3, 9.0), (300, 4, 14.0), (300, 64, 14.0)]
SEED = 4


def _hand_made():
    if "bands" not in _RUNS:
        rng = np.random.default_rng(SEED)
        out = []
        for n, M, edge in BANDS:
            cell = neb_ref.triclinic(rng, edge)
            R, _ = neb_ref.random_band(rng, n, M, cell, pushed=(1,) if M == 3 else (1, M - 2))
            E, F = ref.band_objective(R, cell)
            d1, d2 = ref.pair_vectors(R[0], cell)[1], ref.pair_vectors(R[-1], cell)[1]
            sc = [ref.scales(R[m], ref.targets(d1, d2, m, M), cell) for m in range(1, M - 1)]
            out.append(dict(n=n, M=M, cell=cell, R=R, E=E, F=F, escale=np.array([s[0] for s in sc]),
                            fscale=np.stack([s[1] for s in sc]), wrap=min(ref.wrap_margin(r, cell) for r in R)))
        _RUNS["bands"] = out
    return _RUNS["bands"]


def _dyadic():
    """A band whose fractional coordinates are multiples of 1/64 in a cell of dyadic entries and determinant 32: every fractional
    difference is exact, and some pairs of every image sit exactly at half a cell vector."""
    if "dyadic" not in _RUNS:
        rng = np.random.default_rng(11)
        cell = np.array([[4.0, 0.0, 0.0], [1.0, 4.0, 0.0], [0.5, 1.0, 2.0]])
        n, M = 6, 4
        frac = np.round(rng.uniform(0, 1, (M, n, 3)) * 64) / 64
        frac[:, 1] = frac[:, 0] + [0.5, 0.125, -0.25]    # +1/2 along a in every image
        frac[:, 3] = frac[:, 2] + [0.25, -0.5, 1.5]      # -1/2 along b, 3/2 along c
        frac[1, 5] = frac[1, 4] + [-1.5, 2.5, 0.5]       # all three components, in one interior image
        R = frac @ cell
        _RUNS["dyadic"] = dict(n=n, M=M, cell=cell, R=R, frac=frac)
        E, F = ref.band_objective(R, cell)
        d1, d2 = ref.pair_vectors(R[0], cell)[1], ref.pair_vectors(R[-1], cell)[1]
        sc = [ref.scales(R[m], ref.targets(d1, d2, m, M), cell) for m in range(1, M - 1)]
        _RUNS["dyadic"].update(E=E, F=F, escale=np.array([s[0] for s in sc]), fscale=np.stack([s[1] for s in sc]))
    return _RUNS["dyadic"]


def _launch(bands, active, short=()):
    """One alignn_idpp_forces launch on a batch of hand-made bands -> per active band (F [M - 2, n, 3] or the flat rows of a
    band in ``short``, E [M - 2], status).  The bands in ``short`` get one force row too few."""
    pre = lambda c: torch.tensor(np.concatenate([[0], np.cumsum(c)]), dtype=torch.int32, device=DEV)
    rows = [(b["M"] - 2) * b["n"] for b in bands]
    frows = [rows[s] - (1 if s in short else 0) for s in range(len(bands))]
    t = dict(
        force_ptr=pre([frows[s] for s in active]), energy_ptr=pre([bands[s]["M"] - 2 for s in active]),
        active=torch.tensor(active, dtype=torch.int32, device=DEV), row_ptr=pre(rows), end_ptr=pre([b["n"] for b in bands]),
        lattice=_t(np.stack([b["cell"] for b in bands])), inv_lattice=_t(np.stack([neb_ref.inv3_cof(b["cell"]) for b in bands])),
        initial=_t(np.concatenate([b["R"][0] for b in bands])), final=_t(np.concatenate([b["R"][-1] for b in bands])),
        positions=_t(np.concatenate([b["R"][1:-1].reshape(-1, 3) for b in bands])),
        forces=torch.full((sum(frows[s] for s in active), 3), -7.0, dtype=torch.float64, device=DEV),
        energy=torch.full((sum(bands[s]["M"] - 2 for s in active),), -7.0, dtype=torch.float64, device=DEV),
        row_energy=torch.full((sum(frows[s] for s in active),), -7.0, dtype=torch.float64, device=DEV),
        status=torch.full((len(active),), -7, dtype=torch.int32, device=DEV))
    args = IdppArgs(n_active=len(active), max_images=max(bands[s]["M"] for s in active), max_atoms=max(bands[s]["n"] for s in active),
                    **{k: v.data_ptr() for k, v in t.items()})
    _lib.check(_load().alignn_idpp_forces(C.byref(args), _lib.stream()), "idpp_forces")
    F = torch.split(t["forces"], [frows[s] for s in active])
    E = torch.split(t["energy"], [bands[s]["M"] - 2 for s in active])
    status = t["status"].cpu().numpy()
    return [(F[k].cpu().numpy() if s in short else F[k].cpu().numpy().reshape(bands[s]["M"] - 2, -1, 3), E[k].cpu().numpy(),
             int(status[k])) for k, s in enumerate(active)]


def _like_the_restatement(b, F, E, what):
    """Forces per row within 1e-12 of that row's sum over b of |term|, energies within 1e-12 of the sum of |terms|: a pair's
    term is the same operations on both sides, and a sum of n terms in another order differs by about (n + 20) eps of the sum of
    their sizes, 4e-14 at n = 300."""
    ferr = np.abs(F - b["F"]).max(-1)
    worst_f = float((ferr / np.where(b["fscale"] > 0, b["fscale"], 1.0)).max())
    worst_e = float((np.abs(E - b["E"][1:-1]) / np.where(b["escale"] > 0, b["escale"], 1.0)).max())
    print(f"{what}: n {b['n']} M {b['M']}: force error {worst_f:.2e} of the row's scale, energy error {worst_e:.2e} of its scale")
    assert (ferr <= 1e-12 * b["fscale"]).all(), what
    assert (np.abs(E - b["E"][1:-1]) <= 1e-12 * b["escale"]).all(), what


def test_hand_made_bands_are_away_from_the_wraps_cusp():
    """The host-side premises of the comparison below (checked on the GPU machine too, before it)."""
    bands = _hand_made()
    assert {b["n"] for b in bands} == {1, 2, 63, 64, 65, 300} and {b["M"] for b in bands} == {3, 4, 64}
    for b in bands:
        assert b["wrap"] >= 1e-10, (b["n"], b["M"], b["wrap"])
        # the pushed images are whole lattice vectors away, and the objective does not see it
        assert b["n"] < 2 or np.abs(b["R"][1] - b["R"][0]).max() > 3.0
        assert np.isfinite(b["F"]).all() and (b["n"] < 2 or (b["fscale"] > 0).all())
    d = _dyadic()
    for m in range(d["M"]):
        assert ref.wrap_margin(d["R"][m], d["cell"]) == 0.0  # pairs exactly at +-1/2, in the endpoints too
    assert np.array_equal(neb_ref.row_dot(d["R"].reshape(-1, 3), neb_ref.inv3_cof(d["cell"])), d["frac"].reshape(-1, 3))


def test_idpp_forces_match_the_restatement():
    test_hand_made_bands_are_away_from_the_wraps_cusp()
    bands = _hand_made()
    got = _launch(bands, list(range(len(bands))))
    for b, (F, E, status) in zip(bands, got):
        assert status == 0
        _like_the_restatement(b, F, E, "batch")
    F, E, status = got[0]
    assert bands[0]["n"] == 1 and status == 0 and not F.any() and not E.any()  # one atom: no pairs, exact zeros


def test_idpp_forces_on_pairs_at_exactly_half_a_cell_vector():
    d = _dyadic()
    (F, E, status), = _launch([d], [0])
    assert status == 0
    _like_the_restatement(d, F, E, "dyadic")


def test_idpp_forces_launcher_gives_the_kernels_bits():
    bands = [_hand_made()[s] for s in (1, 2, 4)] + [_dyadic()]
    whole = _launch(bands, list(range(len(bands))))
    E, F = idpp_forces(_t(np.stack([b["cell"] for b in bands])), _t(np.concatenate([b["R"][0] for b in bands])),
                       _t(np.concatenate([b["R"][-1] for b in bands])),
                       _t(np.concatenate([b["R"][1:-1].reshape(-1, 3) for b in bands])), [b["n"] for b in bands],
                       [b["M"] for b in bands])
    assert np.array_equal(F.cpu().numpy(), np.concatenate([w[0].reshape(-1, 3) for w in whole]))
    assert np.array_equal(E.cpu().numpy(), np.concatenate([w[1] for w in whole]))
    with pytest.raises(ValueError, match="positions"):
        idpp_forces(_t(bands[0]["cell"][None]), _t(bands[0]["R"][0]), _t(bands[0]["R"][-1]), _t(bands[0]["R"][1]), [2], [4])
    with pytest.raises(TypeError, match="float64"):
        idpp_forces(_t(bands[0]["cell"][None]), _t(bands[0]["R"][0]), _t(bands[0]["R"][-1]),
                    _t(bands[0]["R"][1:-1].reshape(-1, 3)).float(), [2], [4])


def test_idpp_forces_of_a_band_do_not_depend_on_the_launch():
    bands = _hand_made()
    whole = _launch(bands, list(range(len(bands))))
    # two active bands of a batch of three: the middle one has retired
    three = [bands[6], bands[1], bands[3]]
    part = _launch(three, [0, 2])
    for k, s in ((0, 6), (1, 3)):
        assert np.array_equal(part[k][0], whole[s][0]) and np.array_equal(part[k][1], whole[s][1]) and part[k][2] == 0
    for s in (1, 2, 4, 5):
        (F, E, status), = _launch([bands[s]], [0])
        assert np.array_equal(F, whole[s][0]) and np.array_equal(E, whole[s][1]) and status == 0, s


def test_idpp_forces_flags_rows_that_do_not_fit():
    bands = _hand_made()[1:3]
    got = _launch(bands, [0, 1], short=(1,))  # force rows of another count than the band's
    assert got[0][2] == 0 and got[1][2] == -1 and (got[1][0] == -7.0).all() and (got[1][1] == -7.0).all()
    assert np.array_equal(got[0][0], _launch(bands, [0, 1])[0][0])


# --- (b) idpp_interpolate end to end --------------------------------------------------------------------------------------------------
def _dimer():
    if "dimer" not in _RUNS:
        _RUNS["dimer"] = ref.turning_dimer()
    return _RUNS["dimer"]


def _want(method, fmax, n_images=3, fixed=None):
    key = ("ref", method, fmax, n_images, fixed is not None)
    if key not in _RUNS:
        cell, first, last = _dimer()
        _RUNS[key] = ref.run_idpp_ref(cell, first, last, n_images, 0.1, method, fmax, 100, fixed)
    return _RUNS[key]


def _like_the_restated_pass(res, b, want, what):
    got = res.positions[b].cpu().numpy()
    print(f"{what}: max |dpos| {np.abs(got - want['r']).max():.3e}, max |dE| {np.abs(res.energies[b] - want['e']).max():.3e}, "
          f"steps {int(res.n_steps[b])} vs {want['n_steps']}, margins {want['margins']}, wrap {want['wrap']:.2e}")
    # no energy comparison and no wrap of the restated run is close enough for the device run to take another branch
    assert want["margin"] >= 1e-8 and want["wrap"] >= 1e-3 and want["wrap_ends"] >= 1e-10, what
    assert np.abs(got - want["r"]).max() <= 1e-10, what
    assert res.energies[b] == pytest.approx(want["e"], rel=1e-9, abs=0.0), what
    assert int(res.n_steps[b]) == want["n_steps"] and bool(res.converged[b]) == want["converged"], what


@pytest.mark.parametrize("fmax", [0.1, 0.01])
@pytest.mark.parametrize("method", neb_ref.METHODS)
def test_idpp_interpolate_matches_the_restated_pass(method, fmax):
    cell, first, last = _dimer()
    res = idpp_interpolate([cell], [first], [last], n_images=3, k=0.1, method=method, fmax=fmax, steps=100, device=DEV)
    want = _want(method, fmax)
    _like_the_restated_pass(res, 0, want, (method, fmax))
    assert want["converged"] and want["n_steps"] == {0.1: 7, 0.01: 26}[fmax] and res.n_evals == want["n_evals"]
    assert float(res.fmax[0]) < fmax and res.energies[0][0] == res.energies[0][-1] == 0.0
    got = res.positions[0].cpu().numpy()
    assert np.array_equal(got[0], first) and np.array_equal(got[-1], last)
    linear = ref.bond(neb_ref.interpolate(first, last, cell, 5), cell)
    bonds = ref.bond(got, cell)[1:-1]
    print("bond on the linear path", linear, "on the IDPP path", bonds)
    assert (bonds > linear).all() and linear[1] < 1.23 < 1.45 < bonds[1]


def test_idpp_interpolate_takes_bands_of_different_lengths_and_holds_fixed_atoms():
    cell, first, last = _dimer()
    fixed = np.zeros(8, dtype=bool)
    fixed[[2, 4, 7]] = True
    res = idpp_interpolate([cell] * 3, [first] * 3, [last] * 3, n_images=[3, 5, 3], fixed=[None, None, fixed], device=DEV)
    assert [tuple(p.shape) for p in res.positions] == [(5, 8, 3), (7, 8, 3), (5, 8, 3)]
    _like_the_restated_pass(res, 0, _want("aseneb", 0.1), "3 images beside 5")
    _like_the_restated_pass(res, 1, _want("aseneb", 0.1, 5), "5 images beside 3")
    _like_the_restated_pass(res, 2, _want("aseneb", 0.1, 3, fixed), "fixed spectators")
    alone = idpp_interpolate([cell], [first], [last], n_images=5, device=DEV)
    assert torch.equal(alone.positions[0], res.positions[1]) and np.array_equal(alone.energies[0], res.energies[1])
    start = neb_ref.interpolate(first, last, cell, 5)
    got = res.positions[2].cpu().numpy()[1:-1]
    assert np.array_equal(got[:, fixed], start[:, fixed]) and not np.array_equal(got[:, ~fixed], start[:, ~fixed])
    assert not torch.equal(res.positions[2], res.positions[0])


# --- (c) neb from the IDPP path ----------------------------------------------------------------------------------------------------------
RC = neb_ref.RC


def _neb(**kw):
    cell, first, last = _dimer()
    return neb(None, [cell], [first], [last], n_images=3, k=0.1, fmax=0.05, steps=5,
               forces_fn=pair_ref.make_forces_fn(RC, stress=False), device=DEV, **kw)


def _same_bits(a, b):
    return (torch.equal(a.positions[0], b.positions[0]) and np.array_equal(a.energies[0], b.energies[0])
            and torch.equal(a.forces[0], b.forces[0]) and int(a.n_steps[0]) == int(b.n_steps[0]) and a.n_evals == b.n_evals)


def _like_the_restated_run(res, b, want, what):
    """tests/test_gpu_neb.py's comparison of a ``neb`` call with a restated run."""
    got = res.positions[b].cpu().numpy()
    print(f"{what}: max |dpos| {np.abs(got - want['r']).max():.3e}, max |dE| {np.abs(res.energies[b] - want['e']).max():.3e}, "
          f"steps {int(res.n_steps[b])} vs {want['n_steps']}, margins {want['margins']}")
    assert np.abs(got - want["r"]).max() <= 1e-10 * max(1.0, np.abs(want["r"]).max()), what
    assert res.energies[b] == pytest.approx(want["e"], rel=1e-9, abs=1e-12), what
    assert int(res.n_steps[b]) == want["n_steps"] and bool(res.converged[b]) == want["converged"], what
    assert res.imax[b] == want["imax"], what
    assert res.barrier[b] == res.energies[b].max() - res.energies[b][0] and res.delta_e[b] == res.energies[b][-1] - res.energies[b][0]


@pytest.mark.parametrize("method", neb_ref.METHODS)
def test_neb_from_the_idpp_path_is_neb_started_on_idpp_interpolates_images(method):
    cell, first, last = _dimer()
    composed = _neb(interpolation="idpp", method=method)
    path = idpp_interpolate([cell], [first], [last], n_images=3, k=0.1, method=method, device=DEV)
    handed = _neb(start=[path.positions[0][1:-1]], method=method)
    assert _same_bits(composed, handed)
    assert _same_bits(_neb(start=[path.positions[0][1:-1].cpu().numpy()], method=method), handed)  # (a host array: the same)
    assert not torch.equal(composed.positions[0], _neb(method=method).positions[0])
    # the restated run from the restated IDPP path
    efs = pair_ref.make_efs(RC)
    ef = lambda p: efs(cell, p)[:2]
    idpp = _want(method, 0.1)
    want = ref.run_band_ref(cell, first, last, lambda m, p: ef(p), idpp["r"][1:-1], ef(first)[0], ef(last)[0], 0.1, False, method,
                            0.05, 5)
    assert want["margin"] >= 1e-6 and idpp["margin"] >= 1e-8 and idpp["wrap"] >= 1e-3
    _like_the_restated_run(composed, 0, want, (method, "composed"))
    _like_the_restated_run(handed, 0, want, (method, "handed in"))


def test_neb_with_the_default_interpolation_is_unchanged():
    cell, first, last = _dimer()
    plain = _neb()
    assert _same_bits(_neb(interpolation="linear"), plain)
    assert _same_bits(_neb(start=[neb_ref.interpolate(first, last, cell, 5)]), plain)
    assert _same_bits(_neb(interpolation="linear", idpp_steps=0, idpp_fmax=5.0), plain)  # (the pass's limits are not read)
    efs = pair_ref.make_efs(RC)
    want = neb_ref.run_neb_ref(cell, first, last, lambda p: efs(cell, p)[:2], 3, 0.1, False, "aseneb", 0.05, 5)
    assert want["margin"] >= 1e-6
    _like_the_restated_run(plain, 0, want, "linear")


def test_neb_with_no_idpp_steps_starts_from_the_linear_path():
    assert _same_bits(_neb(interpolation="idpp", idpp_steps=0), _neb())


# --- (d) the host checks behind the device --------------------------------------------------------------------------------------------
def _never(*a, **k):
    raise AssertionError("device work before the checks")


@pytest.mark.parametrize("kw", [dict(interpolation="spline"), dict(interpolation="idpp", start="linear"), dict(start="short"),
                                dict(start="flat"), dict(start="two"), dict(interpolation="idpp", idpp_steps=-1),
                                dict(interpolation="idpp", idpp_fmax=-1.0)])
def test_neb_checks_where_the_band_starts_before_any_launch(kw):
    cell, first, last = _dimer()
    linear = neb_ref.interpolate(first, last, cell, 5)
    starts = {"linear": [linear], "short": [linear[:2]], "flat": [linear.reshape(-1, 3)], "two": [linear, linear]}
    if "start" in kw:
        kw = dict(kw, start=[_t(s) for s in starts[kw["start"]]])
    with pytest.raises(ValueError, match="neb"):
        neb(None, [cell], [first], [last], forces_fn=_never, device=DEV, **kw)
