"""Phonons from symmetry-reduced displacements on the device (csrc/phonon_sym.hip, ``phonons(displacements="symmetry")``)
against the numpy restatement of include/alignn_phsym.h in phonons_sym_ref.py: (1) the plan - representatives, site groups,
directions, distributing operations - identical, and the displaced supercells bit for bit; (2) force constants and frequencies
from forces_fn forces for every drift mode; (3) identity-only structures give the bits of displacements="all"; (4) a structure
alone, in a batch and chunked, bit for bit; (5) operations with entries of W beyond +-1 and lattice shifts that are negative and
beyond N; (6) the model path against one model(batch) per displaced supercell; (7) the errors, before any launch."""

import ctypes as C
import sys

import numpy as np
import pytest
import torch

from alignn_amd import _lib, find_symmetry, neighbors, phonons
from alignn_amd.phonons import lattice_points
from alignn_amd.synthetic import make_crystal
from tests import phonons_sym_ref as R
from tests import sym_ref
from tests.phonons_ref import dynamical_matrices, frequencies, inv_supercell
from tests.sim_gpu import DEV, _model, _t

pytestmark = pytest.mark.gpu
PH = sys.modules["alignn_amd.phonons"]
MASS = {29: 63.5, 6: 12.0, 12: 24.3, 30: 65.4, 16: 32.1, 50: 118.7, 3: 6.9, 8: 16.0, 11: 23.0, 17: 35.5}
NAMES = ["fcc", "diamond", "hcp", "wurtzite", "monoclinic", "triclinic_two_species", "fcc"]
SCS = [(2, 2, 2), (3, 3, 3), (2, 2, 2), (2, 2, 2), (3, 3, 3), (2, 2, 2), (2, 3, 4)]  # at most 54 supercell atoms
_CACHE = {}


def pair_forces(sl, cart):
    """A deterministic exponential pair repulsion over the images within one supercell of each other (float64 numpy).  The
    box of images is no symmetric cutoff, so these forces are only nearly symmetric: the device and the restatement are fed
    the same ones, which is all these tests need."""
    sl, cart = np.asarray(sl, dtype=np.float64), np.asarray(cart, dtype=np.float64)
    shifts = (np.indices((3, 3, 3)).reshape(3, -1).T - 1.0) @ sl
    d = cart[None, :, None, :] + shifts[None, None, :, :] - cart[:, None, None, :]  # [i, j, image, 3]
    r = np.sqrt((d * d).sum(-1))
    r = np.where(r > 1e-9, r, np.inf)
    g = -2.0 * np.exp(-r / 0.7) / 0.7 / r  # phi'(r) / r, phi = 2 exp(-r / 0.7)
    return (g[..., None] * d).sum((1, 2))


class NumpyForces:
    """forces_fn through a numpy force function, one displaced supercell at a time."""

    def __init__(self, fn):
        self.fn, self.calls = fn, 0

    def __call__(self, lats, poss):
        self.calls += 1
        fs = [self.fn(l.cpu().numpy(), p.cpu().numpy()) for l, p in zip(lats, poss)]
        return torch.zeros(len(fs), device=DEV), _t(np.concatenate(fs))


def _sym_dict(res, b):
    return dict(rotations=res.rotations[b].cpu().numpy().astype(np.int64), atom_map=res.atom_map[b].cpu().numpy().astype(np.int64),
                shifts=res.shifts[b].cpu().numpy().astype(np.int64), n_ops=res.n_ops[b])


def _batch(names=NAMES):
    """(cells, positions, species, masses, SymmetryResult) of the named crystals of sym_ref.crystals(), found once."""
    key = tuple(names)
    if key not in _CACHE:
        Cs = sym_ref.crystals()
        lats, pos, zs = ([Cs[k][i] for k in names] for i in range(3))
        _CACHE[key] = (lats, pos, zs, [np.array([MASS[int(v)] for v in z]) for z in zs], find_symmetry(lats, pos, zs, device=DEV))
    return _CACHE[key]


def _cached_pair_forces():
    cache = {}

    def fn(sl, cart):
        key = sl.tobytes() + cart.tobytes()
        if key not in cache:
            cache[key] = pair_forces(sl, cart)
        return cache[key]

    return fn


def _want(lat, pos, sc, sym, delta, fn, drift, n_sym, acoustic=True):
    """The restatement for one structure, its forces from fn(superlattice, cart): -> (C_N, the plan)."""
    pl = R.plan(sym, lat, sc)
    sl = np.asarray(lat, dtype=np.float64) * np.array(sc, dtype=np.float64)[:, None]
    cells = R.displaced_supercells_sym(lat, pos, sc, delta, inv_supercell(lat, sc), pl)
    return R.force_constants_sym([fn(sl, c) for _, c in cells], pl, sym, delta, drift, n_sym, acoustic), pl


# --- (1) the plan and the displaced supercells --------------------------------------------------------------------------------
def test_plan_and_displaced_supercells_are_the_restatement():
    lats, pos, zs, _, res = _batch()
    B, ns, delta = len(NAMES), [len(p) for p in pos], 0.0137
    ncell = [int(np.prod(c)) for c in SCS]
    n_sc = [n * c for n, c in zip(ns, ncell)]
    lib = PH._load_phsym()
    lat_d, dims = _t(np.stack(lats)), _t(SCS, torch.int32)
    ptr = np.concatenate([[0], np.cumsum(ns)])
    ptr_d, pos_d = _t(ptr, torch.int32), _t(np.concatenate(pos))
    plan = PH._plan(lib, res, lat_d, dims, ptr_d, ns, n_sc, torch.device(DEV))
    h = {k: plan[k].cpu().numpy() for k in ("usable", "rot", "rep", "n_site", "site_ops", "n_dir", "dirs", "minv", "dist_op")}
    op_ptr = np.concatenate([[0], np.cumsum(res.n_ops)])
    want_slots, plans = [], []
    for b in range(B):
        pl = R.plan(_sym_dict(res, b), lats[b], SCS[b])
        plans.append(pl)
        rows = slice(ptr[b], ptr[b + 1])
        assert np.array_equal(h["usable"][op_ptr[b]:op_ptr[b + 1]].astype(bool), pl["usable"]), NAMES[b]
        assert np.abs(h["rot"][op_ptr[b]:op_ptr[b + 1]].reshape(-1, 3, 3) - pl["Q"]).max() <= 1e-14
        assert np.array_equal(h["rep"][rows], pl["rep"]) and np.array_equal(h["dist_op"][rows], pl["dist"]), NAMES[b]
        for i in range(ns[b]):
            r = ptr[b] + i
            if i in pl["reps"]:
                k = len(pl["cand"][i])
                assert h["n_dir"][r] == k and h["n_site"][r] == len(pl["site"][i]), (NAMES[b], i)
                assert h["site_ops"][r, :h["n_site"][r]].tolist() == pl["site"][i] and (h["site_ops"][r, h["n_site"][r]:] == -1).all()
                assert np.array_equal(h["dirs"][r].reshape(3, 3)[:k], pl["dirs"][i]) and (h["dirs"][r].reshape(3, 3)[k:] == 0).all()
                assert np.abs(h["minv"][r].reshape(3, 3) - pl["Minv"][i]).max() <= 1e-13 * np.abs(pl["Minv"][i]).max()
                want_slots += [(b, i, m) for m in range(k)]
            else:
                assert h["n_dir"][r] == 0 and h["n_site"][r] == 0
    assert plan["slots"] == want_slots
    assert [len(p["displaced_atoms"]) for p in plans] == [1, 1, 1, 2, 2, 6, 3]
    assert plans[2]["cand"][0] == [4] and plans[6]["usable"].sum() == 2 and plans[0]["usable"].sum() == 48

    # the displaced supercells, bit for bit
    inv = _t(np.stack([inv_supercell(lats[b], SCS[b]) for b in range(B)]))
    jobs, rows, r = [], [], 0
    for b, i, m in plan["slots"]:
        for sg in (0, 1):
            jobs.append((b, i, m, sg))
            rows.append(r)
            r += n_sc[b]
    frac = torch.full((r, 3), np.nan, dtype=torch.float64, device=DEV)
    cart = torch.full((r, 3), np.nan, dtype=torch.float64, device=DEV)
    jobs_d, rows_d = _t(jobs, torch.int32), _t(rows, torch.int64)
    args = PH.DisplaceArgs(positions=pos_d.data_ptr(), atom_ptr=ptr_d.data_ptr(), lattice=lat_d.data_ptr(), inv_supercell=inv.data_ptr(),
                           supercell=dims.data_ptr(), dirs=plan["dirs"].data_ptr(), jobs=jobs_d.data_ptr(), row_off=rows_d.data_ptr(),
                           frac=frac.data_ptr(), cart=cart.data_ptr(), delta=delta, n_jobs=len(jobs), n_structs=B)
    _lib.check(lib.alignn_phsym_displace(C.byref(args), _lib.stream()), "phsym_displace")
    frac, cart, inv_h = frac.cpu().numpy(), cart.cpu().numpy(), inv.cpu().numpy()
    k = 0
    for b in range(B):
        for f, c in R.displaced_supercells_sym(lats[b], pos[b], SCS[b], delta, inv_h[b], plans[b]):
            o = rows[k]
            assert np.array_equal(frac[o:o + len(f)], f) and np.array_equal(cart[o:o + len(c)], c), (NAMES[b], k)
            k += 1
    assert k == len(jobs) and (frac >= 0).all() and (frac < 1).all()


# --- (2) force constants and frequencies -------------------------------------------------------------------------------------
def test_force_constants_and_frequencies_match_the_restatement():
    lats, pos, zs, masses, res = _batch()
    delta = 0.01
    fn = _cached_pair_forces()
    ff = NumpyForces(fn)
    qs = np.random.default_rng(0).uniform(-0.5, 0.5, (5, 3))
    worst = 0.0
    for drift in ("frederiksen", "mean", None):
        for n_sym in (0, 3):
            got = phonons(None, lats, pos, None, masses, supercell=SCS, delta=delta, drift=drift, symmetrize=n_sym, qpoints=qs,
                          dos_kpts=None, forces_fn=ff, device=DEV, displacements="symmetry", symmetry=res)
            for b, name in enumerate(NAMES):
                want, pl = _want(lats[b], pos[b], SCS[b], _sym_dict(res, b), delta, fn, drift, n_sym)
                C_b = got.force_constants[b].cpu().numpy()
                err = np.abs(C_b - want).max() / np.abs(want).max()
                worst = max(worst, err)
                assert err <= 1e-12, (name, drift, n_sym, err)
                w = frequencies(dynamical_matrices(want, masses[b]), lattice_points(SCS[b]), qs)
                assert np.abs(got.frequencies[b].cpu().numpy() - w).max() <= 1e-10 * np.abs(w).max(), (name, drift, n_sym)
                assert np.array_equal(got.displaced_atoms[b].numpy(), pl["displaced_atoms"]) and got.displaced_atoms[b].dtype == torch.int32
                assert np.array_equal(got.directions[b].numpy(), pl["directions"]) and got.directions[b].dtype == torch.float64
    print(f"force constants by symmetry vs the restatement: worst |dC| / max |C| {worst:.2e}")
    assert got.n_supercells == 2 * 16 and sum(len(a) for a in got.displaced_atoms) == 16
    full = phonons(None, lats[:1], pos[:1], None, masses[:1], supercell=SCS[0], delta=delta, dos_kpts=None, forces_fn=ff, device=DEV)
    assert full.displaced_atoms is None and full.directions is None and full.n_supercells == 6


# --- (3) identity only ---------------------------------------------------------------------------------------------------------
def test_identity_only_structures_give_the_bits_of_all_displacements():
    lats, pos = [], []
    for i, n in enumerate((2, 3)):
        lat, frac, _ = make_crystal(n, 4100 + i)
        lats.append(np.asarray(lat, dtype=np.float64))
        pos.append(np.asarray(frac, dtype=np.float64) @ lats[-1])
    masses = [np.array([12.0, 30.0]), np.array([12.0, 30.0, 55.0])]
    res = find_symmetry(lats, pos, [np.arange(2), np.arange(3)], device=DEV)  # (two atoms alike would be an inversion pair)
    assert res.n_ops == [1, 1]
    qs = np.random.default_rng(3).uniform(-0.5, 0.5, (4, 3))
    kw = dict(supercell=[(2, 3, 2), (2, 2, 2)], delta=0.02, qpoints=qs, dos_kpts=None, forces_fn=NumpyForces(pair_forces), device=DEV)
    for drift in ("frederiksen", "mean", None):
        a = phonons(None, lats, pos, None, masses, drift=drift, **kw)
        s = phonons(None, lats, pos, None, masses, drift=drift, displacements="symmetry", symmetry=res, **kw)
        assert s.n_supercells == a.n_supercells == 30 and s.n_evals == a.n_evals
        for b in range(2):
            assert torch.equal(s.force_constants[b], a.force_constants[b]) and torch.equal(s.frequencies[b], a.frequencies[b])
            assert torch.equal(s.directions[b], torch.eye(3, dtype=torch.float64).repeat(len(pos[b]), 1))


# --- (4) alone, batched, chunked ---------------------------------------------------------------------------------------------
def test_structure_alone_equals_its_slice_of_the_batch_and_of_a_chunked_run():
    lats, pos, zs, masses, res = _batch()
    qs = np.random.default_rng(2).uniform(-0.5, 0.5, (3, 3))
    kw = dict(delta=0.02, qpoints=qs, dos_kpts=(3, 3, 3), dos_npts=20, device=DEV, displacements="symmetry")
    ff = NumpyForces(_cached_pair_forces())
    both = phonons(None, lats, pos, None, masses, supercell=SCS, forces_fn=ff, symmetry=res, **kw)
    # 64 supercell atoms per evaluation: one -/+ pair of wurtzite (2 x 32) at a time, so its two pairs sit in two chunks
    chunked = phonons(None, lats, pos, None, masses, supercell=SCS, forces_fn=ff, symmetry=res, max_atoms_per_eval=64, **kw)
    assert chunked.n_evals > both.n_evals
    for b in range(len(NAMES)):
        alone = find_symmetry(lats[b:b + 1], pos[b:b + 1], zs[b:b + 1], device=DEV)
        one = phonons(None, lats[b:b + 1], pos[b:b + 1], None, masses[b:b + 1], supercell=SCS[b], forces_fn=ff, symmetry=alone, **kw)
        for r in (both, chunked):
            assert torch.equal(one.force_constants[0], r.force_constants[b]), NAMES[b]
            assert torch.equal(one.frequencies[0], r.frequencies[b]) and torch.equal(one.dos_weights[0], r.dos_weights[b])


# --- (5) shift arithmetic -------------------------------------------------------------------------------------------------------
def test_rebased_cells_and_atoms_moved_by_lattice_vectors():
    Cs = sym_ref.crystals()
    A, p, z = Cs["diamond"][:3]
    Ar = sym_ref.rebased(A, [[1, 2, 0], [0, 1, 1], [0, 0, 1]])  # the same lattice: operations with entries of W beyond +-1
    moved = p.copy()
    moved[1] = moved[1] + 5.0 * A[0] - 7.0 * A[2]  # shifts that are negative and beyond N
    lats, pos, zs, scs = [Ar, Ar, A], [p, p, moved], [z, z, z], [(3, 3, 3), (2, 3, 4), (2, 2, 2)]
    masses = [np.array([12.0, 12.0])] * 3
    res = find_symmetry(lats, pos, zs, device=DEV)
    assert res.n_ops == [48, 48, 48] and int(res.rotations[0].abs().max()) > 1
    sh = res.shifts[2].cpu().numpy()
    assert sh.min() < 0 and np.abs(sh).max() > 2
    fn = _cached_pair_forces()
    got = phonons(None, lats, pos, None, masses, supercell=scs, delta=0.01, dos_kpts=None, forces_fn=NumpyForces(fn), device=DEV,
                  displacements="symmetry", symmetry=res)
    n_dirs = []
    for b in range(3):
        want, pl = _want(lats[b], pos[b], scs[b], _sym_dict(res, b), 0.01, fn, "frederiksen", 3)
        n_dirs.append(len(pl["displaced_atoms"]))
        err = np.abs(got.force_constants[b].cpu().numpy() - want).max() / np.abs(want).max()
        assert err <= 1e-12, (b, err)
        assert np.array_equal(got.displaced_atoms[b].numpy(), pl["displaced_atoms"])
    assert n_dirs[0] == 1 and n_dirs[2] == 1 and got.n_supercells == 2 * sum(n_dirs)


# --- (6) the model path ----------------------------------------------------------------------------------------------------------
def test_model_path_matches_one_evaluation_per_supercell():
    """The method and tolerance of test_gpu_phonons.py's model-path test.  The graphs are radius graphs with the cutoff between
    two shells (diamond at a = 3.6: 4 neighbours at 1.56, 12 at 2.55, the next at 2.99; rocksalt: 6 at 1.80, 12 at 2.55, the next
    at 3.12; the displacement is 0.05): the default 12 nearest neighbours would cut the shell of 12 in two, and which of its
    equidistant members a graph keeps is not defined, so two evaluations of one supercell need not agree.  Every atom has
    features of its own, diamond's two carbon atoms too: where all atoms carry the same features, the normalised gated sum of
    an edge-gated convolution does not depend on the gates, the model's force constants come out near 1e-7 and the comparison
    would be one of float32 noise.  The solve is linear in whatever forces it is fed; both sides are fed these."""
    model = _model()
    graph = dict(cutoff=2.8, neighbor_strategy="radius_graph")
    names, sc, delta = ["diamond", "rocksalt"], (2, 2, 2), 0.05
    lats, pos, zs, masses, res = _batch(names)
    g = torch.Generator().manual_seed(3)
    feats = [torch.randn(len(z), 92, generator=g) for z in zs]
    got = phonons(model, lats, pos, feats, masses, supercell=sc, delta=delta, dos_kpts=None, displacements="symmetry", symmetry=res,
                  **graph)
    assert got.n_supercells == 2 + 4 and [len(a) for a in got.displaced_atoms] == [1, 2]
    worst = 0.0
    for b in range(2):
        sl_d = _t(lats[b] * np.array(sc, dtype=np.float64)[:, None])
        f_sc = feats[b].repeat(8, 1)
        sym = _sym_dict(res, b)
        pl = R.plan(sym, lats[b], sc)
        forces = []
        for f, _ in R.displaced_supercells_sym(lats[b], pos[b], sc, delta, inv_supercell(lats[b], sc), pl):
            batch = neighbors.crystal_batch([sl_d], [_t(f)], atom_features=[f_sc], device=DEV, line_graph=True, **graph)
            with torch.enable_grad():
                out = model(batch)
            forces.append(out["grad"].detach().reshape(-1, 3).double().cpu().numpy())
        want = R.force_constants_sym(forces, pl, sym, delta)
        err = np.abs(got.force_constants[b].cpu().numpy() - want).max() / np.abs(want).max()
        print(f"model path by symmetry, {names[b]}: |dC| / max |C| {err:.2e}, max |C| {np.abs(want).max():.3e}")
        worst = max(worst, err)
        assert err <= 1e-5, (names[b], err)
    print(f"model path by symmetry vs one evaluation per supercell: worst |dC| / max |C| {worst:.2e}")


# --- (7) errors --------------------------------------------------------------------------------------------------------------------
def test_errors_are_raised_before_any_launch(monkeypatch):
    lats, pos, zs, masses, res = _batch(["diamond", "rocksalt"])
    launches = []
    real = _lib.check
    monkeypatch.setattr(_lib, "check", lambda rc, what: (launches.append(what), real(rc, what))[1])
    ff = NumpyForces(pair_forces)
    kw = dict(supercell=(2, 2, 2), dos_kpts=None, forces_fn=ff, device=DEV)
    with pytest.raises(ValueError, match="needs symmetry="):
        phonons(None, lats, pos, None, masses, displacements="symmetry", **kw)
    with pytest.raises(ValueError, match="equivalent by symmetry but have the masses"):
        phonons(None, lats, pos, None, [np.array([12.0, 13.0]), masses[1]], displacements="symmetry", symmetry=res, **kw)
    with pytest.raises(ValueError, match="displacements must be"):
        phonons(None, lats, pos, None, masses, displacements="phonopy", symmetry=res, **kw)
    with pytest.raises(ValueError, match="only used with displacements='symmetry'"):
        phonons(None, lats, pos, None, masses, symmetry=res, **kw)
    with pytest.raises(ValueError, match="only used with displacements='symmetry'"):
        phonons(None, lats, pos, None, masses, displacements="all", symmetry=res, **kw)
    # a SymmetryResult of other structures: the number of structures, the atom counts
    with pytest.raises(ValueError, match="atoms, these have"):
        phonons(None, lats[:1], pos[:1], None, masses[:1], displacements="symmetry", symmetry=res, **kw)
    with pytest.raises(ValueError, match="atoms, these have"):
        phonons(None, [lats[0]] * 2, [pos[0][:1]] * 2, None, [masses[0][:1]] * 2, displacements="symmetry", symmetry=res, **kw)
    with pytest.raises(ValueError, match="SymmetryResult"):
        phonons(None, lats, pos, None, masses, displacements="symmetry", symmetry="spglib", **kw)
    assert launches == [] and ff.calls == 0
    # rocksalt's two atoms are no images of each other: different masses are fine there, and the run goes through
    ok = phonons(None, lats, pos, None, masses, displacements="symmetry", symmetry=res, **kw)
    assert ok.n_supercells == 6 and "phsym_plan" in launches and "phsym_solve" in launches and "phonon_fc_rows" not in launches
