"""CPU checks of the IDPP band initialisation (alignn_amd/idpp.py, csrc/idpp.hip): (1) the numpy restatement of the objective
(tests/idpp_ref.py) against the gradient of its own energy and at its zero; (2) the premises of the cases tests/test_gpu_idpp.py
runs on the device - the turning dimer by the restatement alone; (3) the input checks of the drivers, which raise before any
device work."""

import numpy as np
import pytest

from alignn_amd.idpp import idpp_interpolate
from alignn_amd.neb import neb
from tests import idpp_ref as ref, neb_ref


def _image(seed, n=7):
    rng = np.random.default_rng(seed)
    cell = neb_ref.triclinic(rng)
    R = rng.uniform(0.0, 1.0, (n, 3)) @ cell
    R[::2] += rng.integers(-1, 2, (len(R[::2]), 3)).astype(np.float64) @ cell  # every other atom whole lattice vectors away
    t = ref.pair_vectors(R + rng.normal(0.0, 0.3, (n, 3)), cell)[1]
    return cell, R, t


# --- (1) the objective -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_forces_are_minus_the_gradient_of_the_energy(seed):
    cell, R, t = _image(seed)
    assert ref.wrap_margin(R, cell) >= 1e-3  # (no pair changes its image inside the difference quotient)
    _, F = ref.objective(R, t, cell)
    h, G = 1e-5, np.zeros_like(R)
    for a in range(len(R)):
        for j in range(3):
            Rp, Rm = R.copy(), R.copy()
            Rp[a, j] += h
            Rm[a, j] -= h
            G[a, j] = (ref.objective(Rp, t, cell)[0] - ref.objective(Rm, t, cell)[0]) / (2 * h)
    print(f"seed {seed}: max |F + dE/dR| / max |F| = {np.abs(F + G).max() / np.abs(F).max():.2e}")
    assert np.abs(F + G).max() <= 1e-7 * np.abs(F).max()


def test_energy_and_forces_vanish_when_the_targets_are_the_images_own_distances():
    cell, R, _ = _image(3)
    E, F = ref.objective(R, ref.pair_vectors(R, cell)[1], cell)
    assert E == 0.0 and not F.any()
    E, F = ref.objective(R[:1], np.zeros((1, 1)), cell)  # a single atom has no pairs
    assert E == 0.0 and F.shape == (1, 3) and not F.any()
    band = np.stack([R, R + 0.1, R + 0.3])
    E, F = ref.band_objective(band, cell)  # a rigid translation keeps every distance, to the rounding of the shifted rows
    assert E.shape == (3,) and F.shape == (1,) + R.shape and np.abs(F).max() <= 1e-10 and E.max() <= 1e-20


def test_every_pair_is_counted_from_both_sides():
    cell, R, t = _image(4, n=2)
    D, d = ref.pair_vectors(R, cell)
    delta = d[0, 1] - t[0, 1]
    E, F = ref.objective(R, t, cell)
    assert E == pytest.approx(delta ** 2 / d[0, 1] ** 4, rel=1e-14)  # 1/2 (the pair twice)
    assert F[0] == pytest.approx(-2 * delta * (1 - 2 * delta / d[0, 1]) / d[0, 1] ** 5 * D[0, 1], rel=1e-13)
    assert np.array_equal(F[1], -F[0])
    escale, fscale = ref.scales(R, t, cell)
    assert escale == pytest.approx(E) and fscale == pytest.approx(np.sqrt((F * F).sum(1)))


def test_wrap_margin_is_the_distance_from_half_a_cell_vector():
    cell = np.array([[4.0, 0.0, 0.0], [1.0, 4.0, 0.0], [0.5, 1.0, 2.0]])  # dyadic entries, det 32: the fractions are exact
    frac = np.array([[0.0, 0.0, 0.0], [0.25, 0.125, 1.375]])
    assert ref.wrap_margin(frac @ cell, cell) == 0.125
    frac[1, 0] = 0.5
    assert ref.wrap_margin(frac @ cell, cell) == 0.0 and ref.wrap_margin(frac[:1] @ cell, cell) == np.inf


# --- (2) the turning dimer -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", neb_ref.METHODS)
def test_turning_dimer_by_the_restatement(method):
    cell, first, last = ref.turning_dimer()
    assert first.shape == last.shape == (8, 3) and ref.bond(np.stack([first, last]), cell) == pytest.approx([ref.BOND] * 2, abs=1e-14)
    linear = ref.bond(neb_ref.interpolate(first, last, cell, 5), cell)
    assert linear[1] == pytest.approx(1.2257, abs=5e-5)  # the straight line squeezes the bond
    loose, tight = (ref.run_idpp_ref(cell, first, last, 3, 0.1, method, fmax, 100) for fmax in (0.1, 0.01))
    print(method, loose["n_steps"], tight["n_steps"], ref.bond(loose["r"], cell), ref.bond(tight["r"], cell), loose["margins"],
          tight["margins"], loose["wrap"], tight["wrap"], loose["wrap_ends"])
    assert loose["converged"] and tight["converged"] and (loose["n_steps"], tight["n_steps"]) == (7, 26)
    assert loose["n_evals"] == 8 and loose["e"][0] == loose["e"][-1] == 0.0 and (loose["e"][1:-1] > 0).all()
    assert ref.bond(loose["r"], cell)[2] == pytest.approx(1.4506, abs=5e-5)
    assert ref.bond(tight["r"], cell)[2] == pytest.approx(1.6285, abs=2e-3)
    for run in (loose, tight):
        assert (ref.bond(run["r"], cell)[1:-1] > linear).all()
        assert run["margin"] >= 1e-8 and run["wrap"] >= 1e-3 and run["wrap_ends"] >= 1e-10


def test_fixed_atoms_stay_on_the_linear_path_in_the_restated_pass():
    cell, first, last = ref.turning_dimer()
    fixed = np.zeros(8, dtype=bool)
    fixed[[2, 4, 7]] = True  # two of the spectators that move between the endpoints, one that does not
    run = ref.run_idpp_ref(cell, first, last, 3, 0.1, "aseneb", 0.1, 100, fixed)
    start = neb_ref.interpolate(first, last, cell, 5)
    assert run["n_steps"] > 0 and np.array_equal(run["r"][1:-1][:, fixed], start[:, fixed])
    assert not np.array_equal(run["r"][1:-1][:, ~fixed], start[:, ~fixed])


def test_a_band_run_from_the_linear_start_is_the_restated_neb():
    """``run_band_ref`` with the straight path handed in is ``neb_ref.run_neb_ref``."""
    from tests import pair_ref

    cell, first, last = neb_ref.vacancy_hop(True)
    efs = pair_ref.make_efs(neb_ref.RC)
    ef = lambda p: efs(cell, p)[:2]
    want = neb_ref.run_neb_ref(cell, first, last, ef, 3, 0.1, True, "improvedtangent", 0.05, 3)
    got = ref.run_band_ref(cell, first, last, lambda m, p: ef(p), neb_ref.interpolate(first, last, cell, 5), ef(first)[0],
                           ef(last)[0], 0.1, True, "improvedtangent", 0.05, 3)
    assert np.array_equal(got["r"], want["r"]) and np.array_equal(got["e"], want["e"]) and got["n_steps"] == want["n_steps"] == 3


# --- (3) the input checks ----------------------------------------------------------------------------------------------------------
def _never(*a, **k):
    raise AssertionError("device work before the checks")


@pytest.mark.parametrize("kw,match", [
    (dict(interpolation="spline"), "interpolation"), (dict(interpolation="idpp", start="linear"), "start"),
    (dict(start="short"), "start"), (dict(start="flat"), "start"), (dict(start="two"), "start"), (dict(start="nan"), "finite"),
    (dict(interpolation="idpp", idpp_steps=-1), "idpp_steps"), (dict(idpp_steps=2.5), "idpp_steps"),
    (dict(interpolation="idpp", idpp_fmax=-0.1), "idpp_fmax")])
def test_neb_checks_where_the_band_starts_before_the_device(kw, match):
    """On a CPU device with a ``forces_fn``: the ``ValueError`` comes before the ``TypeError`` of a device that is no GPU."""
    cell, first, last = ref.turning_dimer()
    linear = neb_ref.interpolate(first, last, cell, 5)
    starts = {"linear": [linear], "short": [linear[:2]], "flat": [linear.reshape(-1, 3)], "two": [linear, linear],
              "nan": [np.where(np.arange(3)[:, None, None] == 1, np.nan, linear)]}
    if "start" in kw:
        kw = dict(kw, start=starts[kw["start"]])
    with pytest.raises(ValueError, match=match):
        neb(None, [cell], [first], [last], forces_fn=_never, device="cpu", **kw)


@pytest.mark.parametrize("kw,match", [
    (dict(n_images=0), "n_images"), (dict(n_images=63), "n_images"), (dict(k=0.0), "k must"), (dict(method="string"), "method"),
    (dict(steps=-1), "steps"), (dict(fmax=-0.1), "fmax"), (dict(fixed=[np.zeros(7, dtype=bool)]), "fixed"),
    (dict(timestep=0.1), "unknown"), (dict(final="short"), "endpoints"), (dict(final="same"), "coincide")])
def test_idpp_interpolate_checks_its_options_before_the_device(kw, match):
    cell, first, last = ref.turning_dimer()
    final = {"short": [last[:-1]], "same": [first.copy()], None: [last]}[kw.pop("final", None)]
    with pytest.raises(ValueError, match="idpp_interpolate.*" + match):
        idpp_interpolate([cell], [first], final, device="cpu", **kw)


def test_the_drivers_refuse_a_cpu_device_after_their_checks():
    cell, first, last = ref.turning_dimer()
    with pytest.raises(TypeError, match="GPU"):
        idpp_interpolate([cell], [first], [last], device="cpu")
    with pytest.raises(TypeError, match="GPU"):
        neb(None, [cell], [first], [last], forces_fn=_never, device="cpu", interpolation="idpp")
    with pytest.raises(TypeError, match="GPU"):
        neb(None, [cell], [first], [last], forces_fn=_never, device="cpu", start=[neb_ref.interpolate(first, last, cell, 5)])
