"""CPU checks of the nudged-elastic-band task (alignn_amd/neb.py, csrc/neb.hip): (1) the numpy restatement of the NEB forces
(tests/neb_ref.py) against the properties that define them - what is left along the tangent and what across it - on random bands
in a triclinic cell with an image pushed across a cell face; (2) every branch of the two tangents on energies built by hand; (3)
the interpolation; (4) a vacancy hop in fcc on the pair potential of tests/pair_ref.py by the restatement alone; (5) the input
checks of the driver, which raise before any device work."""

import numpy as np
import pytest

from alignn_amd.neb import neb
from tests import defects_ref, neb_ref as ref, pair_ref

N, M, K = 7, 5, 0.37


def _band(seed, pushed=(2,)):
    rng = np.random.default_rng(seed)
    cell = ref.triclinic(rng)
    R, F = ref.random_band(rng, N, M, cell, pushed=pushed)
    return cell, R, F


def _unit(t):
    return t / np.sqrt(np.vdot(t, t))


def _tangents(R, cell, i):
    return ref.mic(R[i] - R[i - 1], cell), ref.mic(R[i + 1] - R[i], cell)


# energies by hand: the climbing image is 2 in all of them
E_PEAK = np.array([0.0, 0.4, 1.0, 0.7, 0.1])


# --- (1) what the projection leaves ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [0, 1, 2])
@pytest.mark.parametrize("method", ref.METHODS)
def test_along_the_tangent_the_springs_alone_and_across_it_the_force_alone(seed, method):
    cell, R, F = _band(seed)
    got, imax = ref.neb_forces(R, E_PEAK, F, K, False, method, cell=cell)
    assert imax == 2
    for i in range(1, M - 1):
        t1, t2 = _tangents(R, cell, i)
        a, b = ref.tangent_coefficients(E_PEAK, i, imax, method)
        tau, f, g = _unit(a * t1 + b * t2), F[i - 1], got[i - 1]
        if method == "aseneb":  # the springs' own component along tau: -(k t1 - k t2).tau_hat
            spring = -np.vdot(K * t1 - K * t2, tau)
        else:  # the difference of the springs' lengths
            spring = K * np.sqrt(np.vdot(t2, t2)) - K * np.sqrt(np.vdot(t1, t1))
        scale = np.abs(f).max()
        assert abs(np.vdot(g, tau) - spring) <= 1e-13 * scale, (i, np.vdot(g, tau), spring)
        assert np.abs((g - np.vdot(g, tau) * tau) - (f - np.vdot(f, tau) * tau)).max() <= 1e-13 * scale, i


@pytest.mark.parametrize("seed", [0, 1, 2])
@pytest.mark.parametrize("method", ref.METHODS)
def test_the_climbing_image_has_its_force_along_the_tangent_reversed(seed, method):
    cell, R, F = _band(seed)
    got, imax = ref.neb_forces(R, E_PEAK, F, K, True, method, cell=cell)
    plain, _ = ref.neb_forces(R, E_PEAK, F, K, False, method, cell=cell)
    t1, t2 = _tangents(R, cell, imax)
    a, b = ref.tangent_coefficients(E_PEAK, imax, imax, method)
    tau, f, g = _unit(a * t1 + b * t2), F[imax - 1], got[imax - 1]
    assert abs(np.vdot(g, tau) + np.vdot(f, tau)) <= 1e-13 * np.abs(f).max()
    assert np.abs((g - np.vdot(g, tau) * tau) - (f - np.vdot(f, tau) * tau)).max() <= 1e-13 * np.abs(f).max()
    others = [i - 1 for i in range(1, M - 1) if i != imax]
    assert np.array_equal(got[others], plain[others]) and not np.array_equal(got[imax - 1], plain[imax - 1])


@pytest.mark.parametrize("method", ref.METHODS)
def test_an_image_pushed_across_a_cell_face_changes_nothing(method):
    cell, R, F = _band(5, pushed=(2,))
    _, R0, _ = _band(5, pushed=())
    assert np.abs(R[2] - R0[2]).max() > 3.0 and np.array_equal(R[1], R0[1])  # (whole lattice vectors apart)
    got, _ = ref.neb_forces(R, E_PEAK, F, K, False, method, cell=cell)
    want, _ = ref.neb_forces(R0, E_PEAK, F, K, False, method, cell=cell)
    assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max()


def test_fixed_atoms_lose_their_raw_force_ahead_of_the_projection():
    cell, R, F = _band(3)
    fixed = np.arange(N) % 3 == 0
    F0 = F.copy()
    F0[:, fixed] = 0.0
    for method in ref.METHODS:
        got, _ = ref.neb_forces(R, E_PEAK, F, K, True, method, fixed, cell=cell)
        want, _ = ref.neb_forces(R, E_PEAK, F0, K, True, method, cell=cell)
        assert np.array_equal(got, want)
    assert (F[:, fixed] != 0.0).all()  # (the caller's forces are not modified)


# --- (2) every branch of the tangents ----------------------------------------------------------------------------------------------
# (energies, image, the branch's name, (a, b) of tau = a t1 + b t2 worked out by hand from the issue's formulas)
BRANCHES = [
    ([0.0, 1.0, 2.0, 3.0, 4.0], 2, "rising", (0.0, 1.0)),
    ([4.0, 3.0, 2.0, 1.0, 0.0], 2, "falling", (1.0, 0.0)),
    ([0.0, 1.0, 3.0, 2.0, 0.0], 2, "max up", (1.0, 2.0)),    # |E3 - E2| = 1, |E1 - E2| = 2, E3 > E1: t2 dmax + t1 dmin
    ([0.0, 2.5, 3.0, 1.0, 0.0], 2, "max down", (2.0, 0.5)),  # |E3 - E2| = 2, |E1 - E2| = 0.5, E3 < E1: t2 dmin + t1 dmax
    ([5.0, 2.0, 1.0, 4.0, 5.0], 2, "min up", (1.0, 3.0)),    # |E3 - E2| = 3, |E1 - E2| = 1, E3 > E1
    ([5.0, 4.0, 1.0, 2.0, 5.0], 2, "min down", (3.0, 1.0)),  # |E3 - E2| = 1, |E1 - E2| = 3, E3 < E1
    ([0.0, 1.0, 1.0, 2.0, 0.0], 2, "min up", (0.0, 1.0)),    # E2 = E1: not strictly rising; dmin = 0
    ([0.0, 1.0, 2.0, 1.0, 0.0], 2, "max down", (1.0, 1.0)),  # a symmetric maximum: E3 > E1 is false, dmax = dmin
]


@pytest.mark.parametrize("E,i,name,ab", BRANCHES)
def test_improved_tangent_takes_every_branch(E, i, name, ab):
    cell, R, F = _band(7)
    E = np.array(E)
    assert ref.branch(E, i) == name
    got, _ = ref.neb_forces(R, E, F, K, False, "improvedtangent", cell=cell)
    t1, t2 = _tangents(R, cell, i)
    tau = _unit(ab[0] * t1 + ab[1] * t2)
    change = got[i - 1] - F[i - 1]  # the projection and the springs only ever add a multiple of tau
    assert np.abs(change - np.vdot(change, tau) * tau).max() <= 1e-13 * np.abs(change).max()
    assert abs(np.vdot(got[i - 1], tau) - (K * np.sqrt(np.vdot(t2, t2)) - K * np.sqrt(np.vdot(t1, t1)))) <= 1e-13


def test_aseneb_takes_its_three_tangents_and_the_lowest_index_on_ties():
    cell, R, F = _band(8)
    E = np.array([0.0, 1.0, 2.0, 2.0, 0.5])  # a tie of images 2 and 3: imax = 2
    got, imax = ref.neb_forces(R, E, F, K, False, "aseneb", cell=cell)
    assert imax == 2
    for i, ab in ((1, (0.0, 1.0)), (2, (1.0, 1.0)), (3, (1.0, 0.0))):
        t1, t2 = _tangents(R, cell, i)
        tau = _unit(ab[0] * t1 + ab[1] * t2)
        change = got[i - 1] - F[i - 1]
        assert np.abs(change - np.vdot(change, tau) * tau).max() <= 1e-13 * np.abs(change).max(), i


def test_margins_record_the_comparisons_made():
    cell, R, F = _band(9)
    m = {}
    ref.neb_forces(R, [0.0, 1.0, 3.0, 2.5, 0.0], F, K, False, "improvedtangent", cell=cell, margins=m)
    assert m == {"top2": 0.5, "adjacent": 0.5, "across": 1.5}
    m = {}
    ref.neb_forces(R, [0.0, 1.0, 3.0, 2.5, 0.0], F, K, False, "aseneb", cell=cell, margins=m)
    assert m == {"top2": 0.5}


# --- (3) the interpolation -------------------------------------------------------------------------------------------------------
def test_interpolation_takes_the_short_way_and_reaches_the_final_image():
    rng = np.random.default_rng(11)
    cell = ref.triclinic(rng)
    frac0 = rng.uniform(0.0, 1.0, (N, 3))
    frac0[0], frac0[1] = [0.95, 0.5, 0.5], [0.5, 0.03, 0.5]
    d = rng.uniform(-0.2, 0.2, (N, 3))
    d[0], d[1] = [0.1, 0.0, 0.0], [0.0, -0.08, 0.0]  # atom 0 leaves through the +a face, atom 1 through -b
    frac1 = frac0 + d
    frac1 -= np.floor(frac1)  # the final image is given wrapped: atoms 0 and 1 appear on the far side
    first, last = frac0 @ cell, frac1 @ cell
    assert np.abs(last - first).max() > 4.0
    band = ref.interpolate(first, last, cell, M)
    assert band.shape == (M - 2, N, 3)
    step = (d @ cell) / (M - 1)
    for j in range(1, M - 1):
        assert np.abs(band[j - 1] - (first + j * step)).max() <= 1e-13
    # j = M - 1 lands on the final image, up to the lattice vector the wrap took out
    end = first + (M - 1) * (ref.mic(last - first, cell) / (M - 1))
    off = (end - last) @ np.linalg.inv(cell)
    assert np.abs(off - np.round(off)).max() <= 1e-13 and np.abs(np.round(off)).max() == 1.0
    assert np.abs(ref.mic(end - last, cell)).max() <= 1e-13


def test_mic_rounds_half_to_even():
    cell = np.array([[4.0, 0.0, 0.0], [1.0, 4.0, 0.0], [0.5, 1.0, 2.0]])  # dyadic entries, det 32: the fractions are exact
    f = np.array([[0.5, -0.5, 1.5], [2.5, -1.5, 0.25]])
    want = np.array([[0.5, -0.5, -0.5], [0.5, 0.5, 0.25]])
    assert np.array_equal(ref.mic(defects_ref.row_dot(f, cell), cell), defects_ref.row_dot(want, cell))


# --- (4) a vacancy hop in fcc -----------------------------------------------------------------------------------------------------
A, RC, vacancy_hop = ref.A, ref.RC, ref.vacancy_hop


@pytest.mark.parametrize("method", ref.METHODS)
def test_vacancy_hop_by_the_restatement(method):
    cell, first, last = vacancy_hop()
    assert len(first) == 31 and np.sqrt(((last[0] - first[0]) ** 2).sum()) == pytest.approx(A / np.sqrt(2))
    efs = pair_ref.make_efs(RC)
    r = ref.run_neb_ref(cell, first, last, lambda p: efs(cell, p)[:2], n_images=3, k=0.1, method=method, fmax=0.05, steps=30)
    print(method, r["n_steps"], r["barrier"], r["e"], r["margins"])
    assert r["converged"] and r["n_steps"] <= 30
    assert r["imax"] == 2
    assert abs(r["e"][1] - r["e"][3]) <= 1e-9
    assert r["barrier"] > 0 and r["barrier"] == r["e"][2] - r["e"][0]
    assert abs(r["delta_e"]) <= 1e-9


# --- (5) the input checks ----------------------------------------------------------------------------------------------------------
def _never(*a, **k):
    raise AssertionError("device work before the checks")


@pytest.mark.parametrize("kw,match", [
    (dict(final="short"), "endpoints"), (dict(n_images=0), "n_images"), (dict(n_images=63), "n_images"),
    (dict(n_images=2.5), "n_images"), (dict(n_images=[3, 3]), "n_images"), (dict(k=0.0), "k must"), (dict(k=-0.1), "k must"),
    (dict(k=float("nan")), "k must"), (dict(k=[0.1, 0.2]), "k needs"), (dict(method="eb"), "method"), (dict(climb=1), "climb"),
    (dict(steps=-1), "steps"), (dict(fmax=-0.1), "fmax"), (dict(max_atoms_per_eval=0), "max_atoms_per_eval"),
    (dict(timestep=0.1), "unknown"), (dict(maxstep=0.0), "maxstep")])
def test_neb_checks_its_options_before_the_device(kw, match):
    """On a CPU device with a ``forces_fn``: the ``ValueError`` comes before the ``TypeError`` of a device that is no GPU."""
    cell, first, last = vacancy_hop()
    if kw.get("final") == "short":
        kw = dict(kw, final=[last[:-1]])
    with pytest.raises(ValueError, match=match):
        neb(None, [cell], [first], kw.pop("final", [last]), forces_fn=_never, device="cpu", **kw)


def test_neb_refuses_a_cpu_device_after_its_checks():
    cell, first, last = vacancy_hop()
    with pytest.raises(TypeError, match="GPU"):
        neb(None, [cell], [first], [last], forces_fn=_never, device="cpu")
