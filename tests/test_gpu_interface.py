"""The interface task on the device (csrc/interface.hip, alignn_amd/interface.py) against the restatements of
tests/interface_ref.py: (1) ``alignn_zsl_match`` bit for bit, alone and in a batch; (2) ``alignn_interface_build`` bit for bit,
alone and in a batch; (3) ``interface_energy`` on the pair potential of tests/pair_ref.py against the closed forms of a pair
potential; (4) a strained, rotated match end to end against a host loop over the restated matcher, the restated builder and the
restated FIRE; (5) the model path: the same bits per pair alone, together and in groups, and the atom features reach the model
through ``src``."""

import math

import numpy as np
import pytest
import torch

from alignn_amd import _lib, interface_energy, match_lattices, surface_energy
from tests import defects_ref as dref
from tests import interface_ref as ref
from tests import pair_ref
from tests.relax_ref import run_ref
from tests.sim_gpu import DEV, _crystals, _model

pytestmark = pytest.mark.gpu

SENTINEL = -7


A, RC = 4.0, 3.4  # first neighbours of fcc only (as in test_gpu_defects.py)
_rot, _hex, _triclinic, _ref_slab = ref.rot, ref.hexagonal, ref.triclinic, ref.ref_slab


# the tolerances of test_gpu_defects.py, section (b): relax on a forces_fn against the restated FIRE
def _like_the_restated_run(pos_got, e_got, steps_got, conv_got, want, what):
    got = pos_got.cpu().numpy()
    print(f"{what}: max |dpos| {np.abs(got - want['r']).max():.3e}, e {e_got!r} vs {want['e']!r}, steps {steps_got}")
    assert np.abs(got - want["r"]).max() <= 1e-10 * max(1.0, np.abs(want["r"]).max()), what
    assert e_got == pytest.approx(want["e"], rel=1e-9, abs=1e-12), what
    assert steps_got == want["n_steps"] and bool(conv_got) == want["converged"], what


# --- (1) the match -------------------------------------------------------------------------------------------------------------------
def _zsl(films, subs, max_area=500.0, max_area_ratio_tol=1.0, ltol=0.05, atol=1.0):
    """alignn_zsl_match through the C ABI, the outputs pre-filled with a sentinel -> (status, multiples, film matrices,
    substrate matrices, mismatches) as numpy."""
    lib = _lib.load()
    P = len(films)
    hnf, prefix = ref.hnf_tables()
    nmax = np.zeros((P, 2), dtype=np.int32)
    for p in range(P):
        if ref.cell_valid(films[p]) and ref.cell_valid(subs[p]):
            nmax[p] = [ref.largest_multiple(ref.cross2(c), max_area) for c in (films[p], subs[p])]
    rows = prefix[nmax + 1].astype(np.int64)
    off = np.concatenate([[[0, 0]], np.cumsum(rows, axis=0)])
    t = lambda x, dt: torch.tensor(np.ascontiguousarray(x), dtype=dt, device=DEV)  # noqa: E731
    film_d, subs_d = t(np.stack(films), torch.float64), t(np.stack(subs), torch.float64)
    nf_d, ns_d = t(nmax[:, 0], torch.int32), t(nmax[:, 1], torch.int32)
    hnf_d, prefix_d = t(hnf, torch.int32), t(prefix, torch.int32)
    foff, soff = t(off[:-1, 0], torch.int64), t(off[:-1, 1], torch.int64)
    f_rows, s_rows, max_f, max_s = int(off[-1, 0]), int(off[-1, 1]), int(nmax[:, 0].max()), int(nmax[:, 1].max())
    ftab = torch.empty(max(f_rows, 1), 4, dtype=torch.float64, device=DEV)
    fint = torch.empty(max(f_rows, 1), 4, dtype=torch.int32, device=DEV)
    stab = torch.empty(max(s_rows, 1), 6, 4, dtype=torch.float64, device=DEV)
    sint = torch.empty(max(s_rows, 1), 4, dtype=torch.int32, device=DEV)
    best_s = torch.empty(P * max(max_f, 1), dtype=torch.float64, device=DEV)
    best_t = torch.empty(P * max(max_f, 1), dtype=torch.int64, device=DEV)
    out = (torch.full((P,), SENTINEL, dtype=torch.int32, device=DEV), torch.full((P, 2), SENTINEL, dtype=torch.int32, device=DEV),
           torch.full((P, 2, 2), SENTINEL, dtype=torch.int32, device=DEV), torch.full((P, 2, 2), SENTINEL, dtype=torch.int32, device=DEV),
           torch.full((P, 4), float(SENTINEL), dtype=torch.float64, device=DEV))
    _lib.check(lib.alignn_zsl_match(
        film_d.data_ptr(), subs_d.data_ptr(), P, nf_d.data_ptr(), ns_d.data_ptr(), max_f, max_s, hnf_d.data_ptr(), prefix_d.data_ptr(),
        foff.data_ptr(), soff.data_ptr(), f_rows, s_rows, ftab.data_ptr(), fint.data_ptr(), stab.data_ptr(), sint.data_ptr(),
        best_s.data_ptr(), best_t.data_ptr(), float(max_area_ratio_tol), float(ltol), ref.cos_of_degrees(atol),
        *[x.data_ptr() for x in out], _lib.stream()), "zsl_match")
    return [x.cpu().numpy() for x in out]


def _same_match(got, p, want, what):
    status, mult, fmat, smat, mis = got
    assert status[p] == want["status"], (what, status[p], want)
    if want["status"] != 0:  # nothing else is written
        assert (mult[p] == SENTINEL).all() and (fmat[p] == SENTINEL).all() and (smat[p] == SENTINEL).all() and (mis[p] == SENTINEL).all(), what
        return
    assert mult[p].tolist() == [want["i"], want["j"]], (what, mult[p], want)
    assert np.array_equal(fmat[p], want["film_matrix"]) and np.array_equal(smat[p], want["subs_matrix"]), (what, fmat[p], smat[p], want)
    bits = np.array([want["ru"], want["rw"], want["sin"], want["score"]])
    assert np.array_equal(mis[p], bits), (what, mis[p], bits)
    assert round(np.linalg.det(fmat[p])) == want["i"] and round(np.linalg.det(smat[p])) == want["j"], what


def _check_batch(films, subs, expect=None, **kw):
    """The batch against the restatement, then every pair alone against its rows of the batch."""
    got = _zsl(films, subs, **kw)
    wants = [ref.match(f, s, **kw) for f, s in zip(films, subs)]
    for p, want in enumerate(wants):
        _same_match(got, p, want, ("batch", p))
        alone = _zsl(films[p:p + 1], subs[p:p + 1], **kw)
        for x, y in zip(alone, got):
            assert np.array_equal(x[0], y[p]), ("alone", p, x[0], y[p])
    found = [(w["status"], w.get("i"), w.get("j")) for w in wants]
    print(found)
    if expect is not None:
        assert found == expect
    return got, wants


def test_match_reference_cases_and_invalid_cells():
    ob = np.array([[3.1, 0.0], [1.2, 2.7]])
    bad = np.array([[3.0, np.nan], [0.0, 3.0]])
    flat = np.array([[1.0, 2.0], [2.0, 4.0]])
    films = [ob, _hex(3.0 * math.sqrt(3.0)), bad, 3.0 * np.eye(2), _hex(2.9), flat, np.eye(2)[::-1] * 3.0]
    subs = [ob @ _rot(0.7), _hex(3.0) @ _rot(0.3), ob, 4.0 * np.eye(2), 3.6 * np.eye(2), ob, ob]
    got, wants = _check_batch(films, subs, expect=[(0, 1, 1), (0, 1, 3), (2, None, None), (0, 9, 5), (0, 5, 3), (2, None, None),
                                                   (2, None, None)])
    assert wants[3]["score"] == pytest.approx(6.19e-3, abs=5e-6)
    # the public wrapper gives the same, with zeros / NaN where nothing is matched
    res = match_lattices(np.stack(films), np.stack(subs), device=DEV)
    assert np.array_equal(res.status, got[0])
    ok = res.status == 0
    assert np.array_equal(res.film_multiple[ok], got[1][ok, 0]) and np.array_equal(res.subs_matrix[ok], got[3][ok])
    assert np.array_equal(res.score[ok], got[4][ok, 3]) and np.isnan(res.score[~ok]).all() and (res.film_multiple[~ok] == 0).all()


def test_match_mirror_image_and_no_coincidence():
    cell, mirror = np.array([[3.0, 0.0], [0.9, 2.6]]), np.array([[3.0, 0.0], [-0.9, 2.6]])
    _check_batch([cell, cell], [mirror, cell], expect=[(0, 4, 4), (0, 1, 1)], max_area=150.0)  # (never (1, 1) for the mirror image)
    _check_batch([cell, _hex(2.9), cell], [mirror, 3.6 * np.eye(2), mirror @ _rot(0.5)], expect=[(1, None, None)] * 3,
                 max_area=30.0, ltol=0.01, atol=0.2)


def test_match_random_pairs():
    """The forty pairs that the CPU tests hold against the brute force; with the area ratio within 10 % many film
    multiples have no admissible j."""
    films, subs = (list(x) for x in zip(*ref.random_pairs(40, 2024)))
    got, wants = _check_batch(films, subs, max_area=110.0, max_area_ratio_tol=0.1, ltol=0.05, atol=1.0)
    assert {w["status"] for w in wants} == {0, 1}


def test_match_multiples_beyond_a_wavefront_and_a_workgroup():
    """sigma(60) = 168 Hermite normal forms are more than a wavefront, sigma(120) = 360 more than a workgroup: as the film's
    entries held in LDS and as the substrate's entries walked by the threads.  Cells of about 1 A^2 keep the tables small."""
    c0 = np.array([[1.0, 0.0], [0.31, 1.07]])
    sup = lambda a, b, d: np.array([[a, b], [0, d]], dtype=np.float64) @ c0  # noqa: E731
    films = [sup(8, 5, 15) @ _rot(0.4) * 1.003, c0, c0 @ _rot(0.2)]
    subs = [c0, sup(5, 3, 12) @ _rot(1.1) * 1.004, sup(8, 5, 15) * 0.997]
    _check_batch(films, subs, expect=[(0, 1, 120), (0, 60, 1), (0, 120, 1)], max_area=130.0, max_area_ratio_tol=0.1, ltol=0.01,
                 atol=0.5)


def test_match_refuses_multiples_above_256():
    with pytest.raises(ValueError, match="256"):
        match_lattices(np.eye(2)[None], np.eye(2)[None], max_area=300.0, device=DEV)


# --- (2) the builder -----------------------------------------------------------------------------------------------------------------
def _build(slabs, jobs, separation, vacuum, counts):
    lib = _lib.load()
    t = lambda x, dt: torch.tensor(np.ascontiguousarray(x), dtype=dt, device=DEV)  # noqa: E731
    slab_off = np.concatenate([[0], np.cumsum([len(s[1]) for s in slabs])])
    off = np.concatenate([[0], np.cumsum(counts)])
    K, rows = len(jobs), int(off[-1])
    out = (torch.full((3 * K, 3, 3), float(SENTINEL), dtype=torch.float64, device=DEV),
           torch.full((rows, 3), float(SENTINEL), dtype=torch.float64, device=DEV),
           torch.full((rows, 3), float(SENTINEL), dtype=torch.float64, device=DEV),
           torch.full((rows,), SENTINEL, dtype=torch.int32, device=DEV), torch.full((rows,), SENTINEL, dtype=torch.int32, device=DEV),
           torch.full((K,), float(SENTINEL), dtype=torch.float64, device=DEV))
    args = (t(np.stack([s[0] for s in slabs]), torch.float64), t(np.concatenate([s[1] for s in slabs]), torch.float64),
            t(slab_off, torch.int64), t(np.concatenate([s[2] for s in slabs]), torch.int32))
    tail = (t(jobs, torch.int32), t(separation, torch.float64), t(vacuum, torch.float64), t(off, torch.int64))
    _lib.check(lib.alignn_interface_build(*[x.data_ptr() for x in args], len(slabs), *[x.data_ptr() for x in tail], K,
                                          *[x.data_ptr() for x in out], _lib.stream()), "interface_build")
    return [x.cpu().numpy() for x in out], off


def _same_build(got, off, k, want, what):
    cells, cart, frac, src, part, area = got
    A_, carts, fracs, srcs, parts, ar = want
    for q in range(3):
        a, b = off[3 * k + q], off[3 * k + q + 1]
        for name, g, w in (("cell", cells[3 * k + q], A_), ("cart", cart[a:b], carts[q]), ("frac", frac[a:b], fracs[q]),
                           ("src", src[a:b], srcs[q]), ("part", part[a:b], parts[q])):
            assert g.shape == w.shape and np.array_equal(g, w), (what, q, name, np.abs(g - w).max())
        assert (frac[a:b] >= 0.0).all() and (frac[a:b] < 1.0).all(), what
    assert area[k] == ar, (what, area[k], ar)


def test_interface_builder_matches_the_restatement_bit_for_bit():
    CASES = ref.BUILDER_CASES
    parents = {"fcc": dref.fcc(A), "tri": _triclinic()}
    beg = {"fcc": 0, "tri": 4}
    slabs, index = [], {}
    for fp, fh, fl, sp, sh, sl, _, _ in CASES:
        for key in ((fp, fh, fl), (sp, sh, sl)):
            if key not in index:
                index[key] = len(slabs)
                slabs.append(_ref_slab(parents[key[0]], key[1], key[2], beg[key[0]]))
    jobs, counts, sep, vac = [], [], [], []
    for k, (fp, fh, fl, sp, sh, sl, Mf, Ms) in enumerate(CASES):
        f, s = index[(fp, fh, fl)], index[(sp, sh, sl)]
        jobs.append([f, s] + list(np.array(Mf).reshape(-1)) + list(np.array(Ms).reshape(-1)))
        n_s, n_f = round(np.linalg.det(Ms)) * len(slabs[s][1]), round(np.linalg.det(Mf)) * len(slabs[f][1])
        counts += [n_s, n_f, n_s + n_f]
        sep.append(2.0 + 0.5 * k)
        vac.append(7.5 + 0.25 * k)
    got, off = _build(slabs, jobs, sep, vac, counts)
    for k, job in enumerate(jobs):
        want = ref.interface(slabs[job[0]], slabs[job[1]], job[2:6], job[6:10], sep[k], vac[k])
        _same_build(got, off, k, want, ("interface", k))
        alone, off1 = _build(slabs, [job], [sep[k]], [vac[k]], counts[3 * k:3 * k + 3])
        _same_build(alone, off1, 0, want, ("interface alone", k))
    # a pair whose row ranges disagree writes nothing
    wrong = list(counts[:3])
    wrong[1] += 1
    wrong[2] += 1
    skipped, _ = _build(slabs, [jobs[0]], [sep[0]], [vac[0]], wrong)
    assert all((x == SENTINEL).all() for x in skipped)


# --- (3) the closed form of a pair potential ---------------------------------------------------------------------------------------
def test_fcc_on_itself_is_twice_the_surface_energy():
    """fcc(100) on the same fcc(100) at the bulk's layer spacing is the bulk: W_ad is the energy of cutting it, two surfaces."""
    lat, pos = dref.fcc(A)
    fn = pair_ref.make_forces_fn(RC, stress=True)
    res = interface_energy(None, ([lat], [pos]), ([lat], [pos]), [(0, (1, 0, 0), 0, (1, 0, 0))], film_thickness=8.0,
                           subs_thickness=8.0, separation=A / 2, vacuum=8.0, relax_structures=False, forces_fn=fn, device=DEV)
    assert res.status.tolist() == [0] and (res.film_multiple[0], res.subs_multiple[0]) == (1, 1) and res.score[0] == 0.0
    assert res.area[0] == pytest.approx(A * A, rel=1e-14) and res.n_steps[0].tolist() == [0, 0, 0] and res.n_relax_calls == 1
    surf = surface_energy(None, [lat], [pos], miller_indices=[(1, 0, 0)], thickness=8.0, vacuum=8.0, relax_structures=False,
                          forces_fn=fn, device=DEV)
    print("w_ad", res.w_ad[0], "2 surf_en", 2 * surf.surf_en[0][0])
    assert res.w_ad[0] == pytest.approx(2 * surf.surf_en[0][0], rel=1e-9)
    cell = res.lattices[0][2].cpu().numpy()
    bonds = [pair_ref.bond_count(cell, res.positions[0][q].cpu().numpy(), RC) for q in range(3)]
    phi1 = float(pair_ref.phi(A / np.sqrt(2), RC)[0])
    assert bonds[2] - bonds[0] - bonds[1] == 8  # two atoms per (100) plane of the cell, four first neighbours each across the cut
    assert res.w_ad[0] == pytest.approx(-phi1 * (bonds[2] - bonds[0] - bonds[1]) / res.area[0], rel=1e-9)
    assert res.w_ad_J_m2[0] == res.w_ad[0] * dref.EV_A2_TO_J_M2
    assert res.e_interface[0] - res.e_subs[0] - res.e_film[0] == pytest.approx(-res.w_ad[0] * res.area[0], rel=1e-12)
    assert res.part[0][2].cpu().tolist() == [0] * 8 + [1] * 8 and res.part[0][0].cpu().tolist() == [0] * 8


# --- (4) a strained, rotated match end to end --------------------------------------------------------------------------------------
def test_strained_rotated_interface_against_the_host_loop():
    af, rc = 3.6, 4.5
    asub = af * math.sqrt(2.0) * 1.01
    film, subs = dref.fcc(af), dref.fcc(asub)
    efs = pair_ref.make_efs(rc)
    # a second pair beside it: no coincidence within max_area (status 1) must leave the first untouched
    res = interface_energy(None, ([film[0]], [film[1]]), ([subs[0], 0.77 * subs[0]], [subs[1], 0.77 * subs[1]]),
                           [(0, (1, 0, 0), 0, (1, 0, 0)), (0, (1, 0, 0), 1, (1, 0, 0))], film_thickness=4.0, subs_thickness=5.5,
                           separation=2.2, vacuum=9.0, max_area=40.0, max_area_ratio_tol=0.05, ltol=0.02, steps=5, fmax=1e-6,
                           optimize_lattice=False, forces_fn=pair_ref.make_forces_fn(rc, stress=False), device=DEV)
    f_slab, s_slab = _ref_slab(film, (1, 0, 0), 1, 0), _ref_slab(subs, (1, 0, 0), 1, 4)
    m = ref.match(ref.plane_cell(f_slab[0]), ref.plane_cell(s_slab[0]), max_area=40.0, max_area_ratio_tol=0.05, ltol=0.02)
    assert m["status"] == 0 and (m["i"], m["j"]) == (2, 1) and m["ru"] == pytest.approx(0.01, abs=1e-12)
    assert res.status.tolist() == [0, 1] and (res.film_multiple[0], res.subs_multiple[0]) == (2, 1)
    assert np.array_equal(res.film_matrix[0], m["film_matrix"]) and np.array_equal(res.subs_matrix[0], m["subs_matrix"])
    assert (res.mismatch_u[0], res.mismatch_w[0], res.mismatch_sin[0], res.score[0]) == (m["ru"], m["rw"], m["sin"], m["score"])
    assert np.isnan(res.w_ad[1]) and np.isnan(res.e_film[1]) and res.positions[1] is None and res.lattices[1] is None
    cell, carts, _, srcs, parts, area = ref.interface(f_slab, s_slab, m["film_matrix"], m["subs_matrix"], 2.2, 9.0)
    assert res.area[0] == area
    e = [res.e_subs[0], res.e_film[0], res.e_interface[0]]
    for q in range(3):
        want = run_ref(carts[q], lambda r: efs(cell, r)[:2], fmax=1e-6, steps=5)
        _like_the_restated_run(res.positions[0][q], e[q], int(res.n_steps[0][q]), res.converged[0][q], want, ("interface job", q))
        assert np.array_equal(res.src[0][q].cpu().numpy(), srcs[q]) and np.array_equal(res.part[0][q].cpu().numpy(), parts[q])
        assert np.array_equal(res.lattices[0][q].cpu().numpy(), cell)
    assert res.w_ad[0] == pytest.approx(ref.work_of_adhesion(e[2], e[0], e[1], area), rel=1e-14)
    assert res.n_steps[0][2] == 5


# --- (5) a random-initialised ALIGNNAtomWise ---------------------------------------------------------------------------------------
_KW = dict(film_thickness=1.0, subs_thickness=1.0, separation=2.0, vacuum=6.0, max_area=60.0, steps=2, fmax=0.0)
_PAIRS = [(0, (1, 0, 0), 0, (1, 0, 0)), (1, (0, 1, 0), 1, (0, 1, 0))]
_CACHE = {}


def _model_case():
    if not _CACHE:
        model = _model()
        lats, pos, feats = _crystals(2, 6)
        _CACHE["case"] = (model, lats, pos, feats, interface_energy(model, (lats, pos, feats), (lats, pos, feats), _PAIRS, **_KW))
    return _CACHE["case"]


def _same_pair(other, k, res, p, what):
    for name in ("e_subs", "e_film", "e_interface", "w_ad", "area", "score"):
        assert getattr(other, name)[k] == getattr(res, name)[p], (what, name)
    assert torch.equal(other.lattices[k], res.lattices[p]), what
    assert all(torch.equal(x, y) for x, y in zip(other.positions[k], res.positions[p])), what


def test_model_path_per_pair_and_in_groups_gives_the_whole_calls_bits():
    model, lats, pos, feats, res = _model_case()
    assert res.status.tolist() == [0, 0] and res.film_multiple.tolist() == [1, 1] and res.subs_multiple.tolist() == [1, 1]
    assert res.n_relax_calls == 1 and all(n.tolist() == [2, 2, 2] for n in res.n_steps) and np.isfinite(res.w_ad).all()
    for p in range(2):
        alone = interface_energy(model, (lats, pos, feats), (lats, pos, feats), _PAIRS[p:p + 1], **_KW)
        _same_pair(alone, 0, res, p, "alone")
        # the two slabs keep their cell (an all-zero mask), the interface keeps its vacuum axis
        built = res.lattices[p].cpu().numpy()
        # (1e-12 A: float64 rounding of a 10 A cell through the filter's deformation gradient, the identity in these components)
        assert np.abs(built[0] - built[1]).max() <= 1e-12 and np.abs(built[2][2] - built[0][2]).max() <= 1e-12
        assert np.abs(built[2][:2] - built[0][:2]).max() > 1e-9
    grouped = interface_energy(model, (lats, pos, feats), (lats, pos, feats), _PAIRS, max_atoms_per_call=20, **_KW)
    assert grouped.n_relax_calls > 1
    for p in range(2):
        _same_pair(grouped, p, res, p, "in groups")


def test_model_path_features_through_src_and_stress_check():
    model, lats, pos, feats, _ = _model_case()
    kw = dict(_KW, relax_structures=False)
    base = interface_energy(model, (lats, pos, feats), (lats, pos, feats), _PAIRS[:1], **kw)
    same = interface_energy(model, (lats, pos, [f.clone() for f in feats]), (lats, pos, feats), _PAIRS[:1], **kw)
    rolled = interface_energy(model, (lats, pos, [feats[0].roll(1, 0), feats[1]]), (lats, pos, feats), _PAIRS[:1], **kw)
    assert base.n_steps[0].tolist() == [0, 0, 0]
    assert base.e_film[0] == same.e_film[0] and base.e_interface[0] == same.e_interface[0]
    assert base.e_film[0] != rolled.e_film[0] and base.e_interface[0] != rolled.e_interface[0]
    assert base.e_subs[0] == rolled.e_subs[0]  # the substrate's features were not touched
    n, n_film = len(pos[0]), len(pos[0]) + len(pos[1])  # the packed parents: the film crystals' rows, then the substrate crystals'
    src = base.src[0][2].cpu().tolist()
    assert sorted(src[:n]) == list(range(n_film, n_film + n)) and sorted(src[n:]) == list(range(n))
    with pytest.raises(ValueError, match="stress"):
        interface_energy(_model(stresswise_weight=0.0), (lats, pos, feats), (lats, pos, feats), _PAIRS[:1], **_KW)
    with pytest.raises(ValueError, match="interface_cell_mask"):
        interface_energy(model, (lats, pos, feats), (lats, pos, feats), _PAIRS[:1], cell_mask=[1, 1, 0, 0, 0, 1], **_KW)
    with pytest.raises(ValueError, match="fixed"):
        interface_energy(model, (lats, pos, feats), (lats, pos, feats), _PAIRS[:1], fixed=[None], **_KW)
