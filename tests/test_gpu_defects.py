"""The defect tasks on the device (csrc/defects.hip, alignn_amd/defects.py) against the restatements of tests/defects_ref.py:
(a) the two builder kernels bit for bit, alone and in a batch; (b) ``vacancy_formation`` and ``surface_energy`` on the pair
potential of tests/pair_ref.py against a host loop over the restated builders and the restated FIRE, and against the closed
forms of a pair potential; (c) the model path: the same bits per parent, in groups, and as a direct ``relax`` on the restated
structures; (d) the atom features reach the model through ``src``."""

import numpy as np
import pytest
import torch

from alignn_amd import _lib, surface_energy, vacancy_formation
from alignn_amd.relax import relax
from alignn_amd.synthetic import make_crystal
from tests import defects_ref as ref
from tests import pair_ref
from tests.relax_ref import run_ref
from tests.sim_gpu import DEV, _crystals, _model

pytestmark = pytest.mark.gpu

A, RC = 4.0, 3.4  # first neighbours of fcc only


def _triclinic():
    lat, frac, _ = make_crystal(6, 77)
    lat = np.asarray(lat, dtype=np.float64)
    return lat, np.asarray(frac, dtype=np.float64) @ lat


def _parents():
    ps = [ref.fcc(A), _triclinic()]
    ptr = np.concatenate([[0], np.cumsum([len(p) for _, p in ps])])
    return ps, ptr


def _device_parents(ps, ptr):
    return (torch.tensor(np.concatenate([p for _, p in ps]), device=DEV), torch.tensor(ptr, dtype=torch.int32, device=DEV),
            torch.tensor(np.stack([l for l, _ in ps]), device=DEV))


def _outputs(J, rows):
    return (torch.full((J, 3, 3), -7.0, dtype=torch.float64, device=DEV), torch.full((rows, 3), -7.0, dtype=torch.float64, device=DEV),
            torch.full((rows, 3), -7.0, dtype=torch.float64, device=DEV), torch.full((rows,), -7, dtype=torch.int32, device=DEV))


def _supercells(pos, atom_ptr, lat, dims, jobs, counts):
    lib = _lib.load()
    off = np.concatenate([[0], np.cumsum(counts)])
    out = _outputs(len(jobs), int(off[-1]))
    dims_d = torch.tensor(dims, dtype=torch.int32, device=DEV)
    jobs_d = torch.tensor(jobs, dtype=torch.int32, device=DEV)
    off_d = torch.tensor(off, dtype=torch.int64, device=DEV)
    _lib.check(lib.alignn_defect_supercells(pos.data_ptr(), atom_ptr.data_ptr(), lat.data_ptr(), dims_d.data_ptr(), len(dims),
                                            jobs_d.data_ptr(), off_d.data_ptr(), len(jobs), *[t.data_ptr() for t in out],
                                            _lib.stream()), "defect_supercells")
    return [t.cpu().numpy() for t in out], off


def _slabs(pos, atom_ptr, lat, B, jobs, vacuum, counts):
    lib = _lib.load()
    off = np.concatenate([[0], np.cumsum(counts)])
    out = _outputs(len(jobs), int(off[-1]))
    jobs_d = torch.tensor(jobs, dtype=torch.int32, device=DEV)
    vac_d = torch.tensor(vacuum, dtype=torch.float64, device=DEV)
    off_d = torch.tensor(off, dtype=torch.int64, device=DEV)
    _lib.check(lib.alignn_slab_build(pos.data_ptr(), atom_ptr.data_ptr(), lat.data_ptr(), B, jobs_d.data_ptr(), vac_d.data_ptr(),
                                     off_d.data_ptr(), len(jobs), *[t.data_ptr() for t in out], _lib.stream()), "slab_build")
    return [t.cpu().numpy() for t in out], off


def _same_bits(got, off, k, want, what):
    cells, cart, frac, src = got
    a, b = off[k], off[k + 1]
    for name, g, w in (("cell", cells[k], want[0]), ("cart", cart[a:b], want[1]), ("frac", frac[a:b], want[2]),
                       ("src", src[a:b], want[3])):
        assert g.shape == w.shape and np.array_equal(g, w), (what, name, np.abs(g - w).max())
    assert (frac[a:b] >= 0.0).all() and (frac[a:b] < 1.0).all(), what


# --- (a) the builders -----------------------------------------------------------------------------------------------------------
def test_supercell_builder_matches_the_restatement_bit_for_bit():
    ps, ptr = _parents()
    pos, atom_ptr, lat = _device_parents(ps, ptr)
    dims = [(2, 2, 2), (2, 1, 3)]
    jobs, counts = [], []
    for s, (_, p) in enumerate(ps):
        n, n_sc = len(p), len(p) * int(np.prod(dims[s]))
        for a in (-1, 0, n_sc - 1, n + 1):  # pristine, the first atom, the last one, one of a later image
            jobs.append((s, a))
            counts.append(n_sc - (a >= 0))
    got, off = _supercells(pos, atom_ptr, lat, dims, jobs, counts)
    for k, (s, a) in enumerate(jobs):
        _same_bits(got, off, k, ref.supercell(ps[s][0], ps[s][1], dims[s], a, beg=ptr[s]), ("supercell", s, a))
        alone, off1 = _supercells(pos, atom_ptr, lat, dims, [jobs[k]], [counts[k]])
        _same_bits(alone, off1, 0, [got[0][k]] + [x[off[k]:off[k + 1]] for x in got[1:]], ("supercell alone", s, a))


def test_slab_builder_matches_the_restatement_bit_for_bit():
    ps, ptr = _parents()
    pos, atom_ptr, lat = _device_parents(ps, ptr)
    jobs, counts, vacuum = [], [], []
    for s, (l, p) in enumerate(ps):
        for hkl in ((1, 0, 0), (1, 1, 1), (1, -1, 0), (3, 2, 1)):
            for layers in (1, 3):
                jobs.append([s] + [int(v) for v in ref.miller_basis(l, hkl).reshape(-1)] + [layers])
                counts.append(len(p) * layers)
                vacuum.append(7.5 + 0.25 * len(jobs))
    got, off = _slabs(pos, atom_ptr, lat, len(ps), jobs, vacuum, counts)
    for k, job in enumerate(jobs):
        s, basis, layers = job[0], np.array(job[1:10]).reshape(3, 3), job[10]
        want = ref.slab(ps[s][0], ps[s][1], basis, layers, vacuum[k], beg=ptr[s])
        _same_bits(got, off, k, want, ("slab", s, basis.tolist(), layers))
        assert (np.bincount(got[3][off[k]:off[k + 1]] - ptr[s], minlength=len(ps[s][1])) == layers).all()
        alone, off1 = _slabs(pos, atom_ptr, lat, len(ps), [job], [vacuum[k]], [counts[k]])
        _same_bits(alone, off1, 0, [got[0][k]] + [x[off[k]:off[k + 1]] for x in got[1:]], ("slab alone", k))


# --- (b) end to end on the pair potential -------------------------------------------------------------------------------------
# the tolerances of test_gpu_relax.py's comparison of relax on a forces_fn with the restated FIRE
def _like_the_restated_run(pos_got, e_got, steps_got, conv_got, want, what):
    """``conv_got`` None: not compared (with the cell filter the flag also covers the cell rows, which the host run has not)."""
    got = pos_got.cpu().numpy()
    print(f"{what}: max |dpos| {np.abs(got - want['r']).max():.3e}, e {e_got!r} vs {want['e']!r}, steps {steps_got}")
    assert np.abs(got - want["r"]).max() <= 1e-10 * max(1.0, np.abs(want["r"]).max()), what
    assert e_got == pytest.approx(want["e"], rel=1e-9, abs=1e-12), what
    assert steps_got == want["n_steps"] and (conv_got is None or bool(conv_got) == want["converged"]), what


@pytest.mark.parametrize("steps", [0, 5])
def test_vacancy_formation_on_a_pair_potential(steps):
    lat, pos, labels = ref.rock_salt(A)
    efs = pair_ref.make_efs(RC)
    kw = dict(optimize_lattice=False, fmax=1e-6) if steps else {}  # steps = 0 with the default: the cell filter, stresses used
    res = vacancy_formation(None, [lat], [pos], site_labels=[labels], supercell=(2, 2, 2), steps=steps,
                            forces_fn=pair_ref.make_forces_fn(RC, stress=not steps), device=DEV, **kw)
    assert res.labels[0].tolist() == [0, 1] and res.removed_atom[0].tolist() == [0, 4] and res.multiplicity[0].tolist() == [4, 4]
    assert res.n_bulk == [64] and res.supercell == [(2, 2, 2)]
    e_all = [res.e_bulk[0]] + list(res.e_defect[0])
    for k, a in enumerate((-1, 0, 4)):
        cell, cart, _, src = ref.supercell(lat, pos, (2, 2, 2), a)
        want = run_ref(cart, lambda r: efs(cell, r)[:2], fmax=1e-6 if steps else 0.1, steps=steps)
        _like_the_restated_run(res.positions[0][k], e_all[k], int(res.n_steps[0][k]), res.converged[0][k] if steps else None, want,
                               ("vacancy", a))
        assert np.array_equal(res.src[0][k].cpu().numpy(), src)
        assert np.array_equal(res.lattices[0][k].cpu().numpy(), cell)
    if steps:
        assert res.n_steps[0].tolist() == [0, 5, 5]  # the pristine supercell is at rest
    for c in range(2):
        want = ref.formation_energy(res.e_defect[0][c], 63, res.e_bulk[0], 64)
        assert res.formation_energy[0][c] == pytest.approx(want, rel=1e-14)
        if not steps:  # every site of this lattice is the same to a pair potential: a vacancy costs one atom's bonds
            assert res.e_defect[0][c] - res.e_bulk[0] == pytest.approx(-2 * res.e_bulk[0] / 64, rel=1e-9)


@pytest.mark.parametrize("steps", [0, 5])
def test_surface_energy_on_a_pair_potential(steps):
    lat, pos = ref.fcc(A)
    efs = pair_ref.make_efs(RC)
    hkls = [(1, 0, 0), (1, 1, 1)]
    kw = dict(optimize_lattice=False, fmax=1e-6) if steps else {}
    res = surface_energy(None, [lat], [pos], miller_indices=hkls, thickness=8.0, vacuum=8.0, steps=steps,
                         forces_fn=pair_ref.make_forces_fn(RC, stress=not steps), device=DEV, **kw)
    want0 = run_ref(pos, lambda r: efs(lat, r)[:2], fmax=1e-6 if steps else 0.1, steps=steps)
    assert res.epa[0] == pytest.approx(want0["e"] / 4, rel=1e-9)
    phi1 = float(pair_ref.phi(A / np.sqrt(2), RC)[0])
    for m, (hkl, broken) in enumerate(zip(hkls, (8, 12))):
        basis = ref.miller_basis(lat, hkl)
        layers = ref.layers_for(lat, basis, 8.0)
        cell, cart, _, src = ref.slab(lat, pos, basis, layers, 8.0)
        assert np.array_equal(res.basis[0][m], basis) and res.layers[0][m] == layers and res.n_slab[0][m] == len(cart)
        want = run_ref(cart, lambda r: efs(cell, r)[:2], fmax=1e-6 if steps else 0.1, steps=steps)
        _like_the_restated_run(res.positions[0][1 + m], res.e_slab[0][m], int(res.n_steps[0][1 + m]),
                               res.converged[0][1 + m] if steps else None, want, ("slab", hkl))
        assert np.array_equal(res.src[0][1 + m].cpu().numpy(), src)
        assert np.array_equal(res.lattices[0][1 + m].cpu().numpy(), cell)
        assert res.area[0][m] == pytest.approx(A * A * np.linalg.norm(hkl), rel=1e-12)
        assert res.surf_en[0][m] == pytest.approx(ref.surface_energy(res.e_slab[0][m], len(cart), res.epa[0], cell), rel=1e-12)
        assert res.surf_en_J_m2[0][m] == res.surf_en[0][m] * ref.EV_A2_TO_J_M2
        if steps:
            assert res.n_steps[0][1 + m] == 5 and res.surf_en[0][m] > 0
        else:  # as cut: the broken first-neighbour bonds over the two faces
            assert res.surf_en[0][m] == pytest.approx(-phi1 * broken / (2 * res.area[0][m]), rel=1e-9)


# --- (c), (d) a random-initialised ALIGNNAtomWise -------------------------------------------------------------------------------
def _labels(n):
    return np.arange(n) % 2


_MODEL_KW = dict(supercell=(1, 1, 2), steps=2, fmax=0.0, optimize_lattice=True)
_CACHE = {}


def _model_case():
    """The model, two parents and the whole call's result, computed once for the three comparisons below."""
    if not _CACHE:
        model = _model()
        lats, pos, feats = _crystals(2, 6)
        labels = [_labels(len(p)) for p in pos]
        res = vacancy_formation(model, lats, pos, feats, site_labels=labels, **_MODEL_KW)
        _CACHE["case"] = (model, lats, pos, feats, labels, res)
    return _CACHE["case"]


def _flat(res, s):
    return np.concatenate([[res.e_bulk[s]], res.e_defect[s]])


def test_vacancy_model_path_equals_a_direct_relax_on_the_restated_structures():
    model, lats, pos, feats, labels, res = _model_case()
    assert res.n_relax_calls == 1 and all(n.tolist() == [2, 2, 2] for n in res.n_steps)
    built, fs = [], []
    for s in range(2):
        lat, p = np.asarray(lats[s], dtype=np.float64), np.asarray(pos[s], dtype=np.float64)
        for a in (-1, 0, 1):  # the lowest-index atoms of the labels 0 and 1
            built.append(ref.supercell(lat, p, (1, 1, 2), a))
            fs.append(feats[s][torch.as_tensor(built[-1][3]).long()])
    direct = relax(model, [b[0] for b in built], [b[1] for b in built], fs, steps=2, fmax=0.0, optimize_lattice=True)
    e = direct.energies.cpu().numpy()
    print("whole call vs direct relax: max |dE|", np.abs(e - np.concatenate([_flat(res, 0), _flat(res, 1)])).max())
    assert np.array_equal(e, np.concatenate([_flat(res, 0), _flat(res, 1)]))
    assert torch.equal(direct.lattices, torch.cat(res.lattices))
    assert all(torch.equal(x, y) for x, y in zip(direct.positions, res.positions[0] + res.positions[1]))


def _same_as_the_whole_call(other, k, res, s, what):
    print(f"{what}, parent {s}: max |dE| {np.abs(_flat(other, k) - _flat(res, s)).max():.3e} of |E| {np.abs(_flat(res, s)).max():.3e}")
    assert np.array_equal(_flat(other, k), _flat(res, s)), what
    assert np.array_equal(other.formation_energy[k], res.formation_energy[s]), what
    assert all(torch.equal(x, y) for x, y in zip(other.positions[k], res.positions[s])), what
    assert torch.equal(other.lattices[k], res.lattices[s]), what


def test_vacancy_model_path_per_parent_gives_the_whole_calls_bits():
    model, lats, pos, feats, labels, res = _model_case()
    for s in range(2):
        alone = vacancy_formation(model, lats[s:s + 1], pos[s:s + 1], feats[s:s + 1], site_labels=labels[s:s + 1], **_MODEL_KW)
        _same_as_the_whole_call(alone, 0, res, s, "per parent")


def test_vacancy_model_path_in_groups_gives_the_whole_calls_bits():
    model, lats, pos, feats, labels, res = _model_case()
    grouped = vacancy_formation(model, lats, pos, feats, site_labels=labels, max_atoms_per_call=40, **_MODEL_KW)
    assert grouped.n_relax_calls > 1
    for s in range(2):
        _same_as_the_whole_call(grouped, s, res, s, "in groups")


def test_atom_features_reach_the_model_through_src():
    model = _model()
    lats, pos, feats = _crystals(1, 6)
    kw = dict(site_labels=[_labels(6)], supercell=(1, 1, 2), relax_structures=False, optimize_lattice=False)
    base = vacancy_formation(model, lats, pos, feats, **kw)
    same = vacancy_formation(model, lats, pos, [feats[0].clone()], **kw)
    rolled = vacancy_formation(model, lats, pos, [feats[0].roll(1, 0)], **kw)
    assert base.n_steps[0].tolist() == [0, 0, 0]
    assert base.e_bulk[0] == same.e_bulk[0] and np.array_equal(base.e_defect[0], same.e_defect[0])
    assert base.e_bulk[0] != rolled.e_bulk[0] and (base.e_defect[0] != rolled.e_defect[0]).all()
    # a slab: the parent and the slab as a direct relax on the restated slab with the features of its src
    lat, p = np.asarray(lats[0], dtype=np.float64), np.asarray(pos[0], dtype=np.float64)
    res = surface_energy(model, lats, pos, feats, miller_indices=[(1, 1, 0)], thickness=1.0, vacuum=6.0, relax_structures=False,
                         optimize_lattice=False)
    basis = ref.miller_basis(lat, (1, 1, 0))
    cell, cart, _, src = ref.slab(lat, p, basis, ref.layers_for(lat, basis, 1.0), 6.0)
    direct = relax(model, [lat, cell], [p, cart], [feats[0], feats[0][torch.as_tensor(src).long()]], steps=0)
    e = direct.energies.cpu().numpy()
    assert res.epa[0] == e[0] / 6 and res.e_slab[0][0] == e[1]
    assert res.surf_en[0][0] == ref.surface_energy(e[1], len(cart), e[0] / 6, cell)
