"""The executable specification of ``alignn_amd.neb`` (csrc/neb.hip): float64 numpy restatements of ASE 3.22's ``ase/neb.py`` for
``method="aseneb"`` and ``"improvedtangent"`` - ``NEB.interpolate(mic=True)``, ``NEB.get_forces`` with ``FixAtoms`` applied
inside every image's ``get_forces``, and ``FIRE(neb).run(fmax, steps)`` through tests/relax_ref.py - with the plain-wrap minimum
image convention of the kernels in place of ASE's Minkowski-reduced ``find_mic``.  ASE is not a dependency of this project, and
the reference has no NEB.

``mic`` and ``interpolate`` are written operation for operation as the kernels are (``defects_ref.inv3_cof`` / ``row_dot``,
elementwise numpy only), so the device results are expected to be the same bits.  ``neb_forces`` is written with vectors - the
tangent, its dot products and the projection as ASE writes them - where the kernel works from five sums; the two agree to
rounding.  tests/test_neb_ref.py pins this file by the projections' own properties; tests/test_gpu_neb.py holds the kernels and
the driver to it.  This module holds no tests."""

import numpy as np

from tests import defects_ref
from tests.defects_ref import inv3_cof, row_dot
from tests.relax_ref import run_fixed_ref, run_ref

METHODS = ("aseneb", "improvedtangent")


def mic(d, C):
    """The plain wrap of the row differences ``d`` [rows, 3] in the cell ``C`` (rows a, b, c)."""
    C = np.asarray(C, dtype=np.float64)
    f = row_dot(np.asarray(d, dtype=np.float64), inv3_cof(C))
    f = f - np.round(f)  # (half to even, as rint)
    return row_dot(f, C)


def interpolate(initial, final, C, M):
    """NEB.interpolate(mic=True) for a band of M images: -> the M - 2 interior images [M - 2, n, 3]."""
    initial, final = np.asarray(initial, dtype=np.float64), np.asarray(final, dtype=np.float64)
    step = mic(final - initial, C) / (M - 1)
    return np.stack([initial + j * step for j in range(1, M - 1)])


def _note(margins, kind, x):
    if margins is not None:
        margins[kind] = min(margins.get(kind, np.inf), float(x))


def neb_forces(R, E, F, k, climb, method, fixed=None, *, cell, margins=None):
    """NEB.get_forces: ``R`` [M, n, 3] the band (endpoints included), ``E`` [M] its energies, ``F`` [M - 2, n, 3] the raw forces of
    the interior images, ``k`` the spring constant, ``fixed`` [n] bool (FixAtoms of every image) -> (the projected forces
    [M - 2, n, 3], imax).  ``margins``: a dict that collects the smallest margin of every energy comparison made, by kind:
    "top2" (the two largest interior energies), "adjacent" (E[i + 1] vs E[i]) and "across" (E[i + 1] vs E[i - 1])."""
    R, E = np.asarray(R, dtype=np.float64), np.asarray(E, dtype=np.float64)
    M = len(R)
    assert method in METHODS and E.shape == (M,) and M >= 3
    F = np.array(F, dtype=np.float64)
    if fixed is not None:
        F[:, np.asarray(fixed, dtype=bool)] = 0.0
    imax = 1 + int(np.argmax(E[1:-1]))  # the lowest index on ties
    if M > 3:
        top = np.sort(E[1:-1])
        _note(margins, "top2", top[-1] - top[-2])
    out = np.empty_like(F)
    for i in range(1, M - 1):
        f = F[i - 1]
        t1, t2 = mic(R[i] - R[i - 1], cell), mic(R[i + 1] - R[i], cell)
        if method == "aseneb":
            tau = t2 if i < imax else t1 if i > imax else t1 + t2
            ft, tt = np.vdot(f, tau), np.vdot(tau, tau)
            if climb and i == imax:
                out[i - 1] = f - 2 * ft / tt * tau
            else:
                out[i - 1] = f - ft / tt * tau - np.vdot(k * t1 - k * t2, tau) / tt * tau
        else:
            _note(margins, "adjacent", min(abs(E[i + 1] - E[i]), abs(E[i] - E[i - 1])))
            if E[i + 1] > E[i] > E[i - 1]:
                tau = t2.copy()
            elif E[i + 1] < E[i] < E[i - 1]:
                tau = t1.copy()
            else:
                dmax = max(abs(E[i + 1] - E[i]), abs(E[i - 1] - E[i]))
                dmin = min(abs(E[i + 1] - E[i]), abs(E[i - 1] - E[i]))
                _note(margins, "across", abs(E[i + 1] - E[i - 1]))
                tau = t2 * dmax + t1 * dmin if E[i + 1] > E[i - 1] else t2 * dmin + t1 * dmax
            tau = tau / np.sqrt(np.vdot(tau, tau))
            if climb and i == imax:
                out[i - 1] = f - 2 * np.vdot(f, tau) * tau
            else:
                out[i - 1] = f - np.vdot(f, tau) * tau + (k * np.sqrt(np.vdot(t2, t2)) - k * np.sqrt(np.vdot(t1, t1))) * tau
    return out, imax


def tangent_coefficients(E, i, imax, method):
    """(a, b) with tau = a t1 + b t2 before any normalisation: what the five-sum form of the kernel works from."""
    if method == "aseneb":
        return (0.0, 1.0) if i < imax else (1.0, 0.0) if i > imax else (1.0, 1.0)
    if E[i + 1] > E[i] > E[i - 1]:
        return 0.0, 1.0
    if E[i + 1] < E[i] < E[i - 1]:
        return 1.0, 0.0
    dmax = max(abs(E[i + 1] - E[i]), abs(E[i - 1] - E[i]))
    dmin = min(abs(E[i + 1] - E[i]), abs(E[i - 1] - E[i]))
    return (dmin, dmax) if E[i + 1] > E[i - 1] else (dmax, dmin)


def cancellation(R, E, method, cell):
    """Per interior image, tau.tau / (a^2 |t1|^2 + b^2 |t2|^2): how much of the tangent's two parts survives their sum."""
    R, E = np.asarray(R, dtype=np.float64), np.asarray(E, dtype=np.float64)
    M = len(R)
    imax = 1 + int(np.argmax(E[1:-1]))
    out = []
    for i in range(1, M - 1):
        a, b = tangent_coefficients(E, i, imax, method)
        t1, t2 = mic(R[i] - R[i - 1], cell), mic(R[i + 1] - R[i], cell)
        tau = a * t1 + b * t2
        out.append(np.vdot(tau, tau) / (a * a * np.vdot(t1, t1) + b * b * np.vdot(t2, t2)))
    return np.array(out)


def run_neb_ref(cell, initial, final, ef, n_images=3, k=0.1, climb=False, method="aseneb", fmax=0.05, steps=100, fixed=None,
                fire=None):
    """``FIRE(NEB(images, k, climb, method)).run(fmax, steps)`` after ``interpolate(mic=True)``: the band's interior rows as one
    structure through relax_ref's ``run_ref`` / ``run_fixed_ref``.  ``ef(pos) -> (e, f)`` of one image in ``cell``.
    -> dict(r [M, n, 3], e [M], f (the NEB forces of the last evaluation [M - 2, n, 3]), imax, barrier, delta_e, n_steps,
    converged, n_evals, margins (``neb_forces``'s, over the whole run), margin (their minimum))."""
    initial, final = np.asarray(initial, dtype=np.float64), np.asarray(final, dtype=np.float64)
    M, n = n_images + 2, len(initial)
    e_first, e_last = ef(initial)[0], ef(final)[0]
    last, margins = {}, {}

    def band(rows):
        R = np.concatenate([initial[None], rows.reshape(M - 2, n, 3), final[None]])
        ev = [ef(r) for r in R[1:-1]]
        E = np.array([e_first] + [e for e, _ in ev] + [e_last], dtype=np.float64)
        g, imax = neb_forces(R, E, np.stack([f for _, f in ev]), k, climb, method, fixed, cell=cell, margins=margins)
        last.update(R=R, E=E, g=g, imax=imax)
        return E[imax], g.reshape(-1, 3)

    rows0 = interpolate(initial, final, cell, M).reshape(-1, 3)
    if fixed is None:
        run = run_ref(rows0, band, fmax=fmax, steps=steps, **(fire or {}))
    else:
        run = run_fixed_ref(rows0, band, np.tile(np.asarray(fixed, dtype=bool), M - 2), fmax=fmax, steps=steps, fire=fire)
    E = last["E"]
    return dict(r=last["R"], e=E, f=last["g"], imax=last["imax"], barrier=E.max() - E[0], delta_e=E[-1] - E[0],
                n_steps=run["n_steps"], converged=run["converged"], n_evals=run["n_evals"], margins=margins,
                margin=min(margins.values()) if margins else np.inf)


# --- hand-made bands for the tests ---------------------------------------------------------------------------------------------
def branch(E, i):
    """Which tangent the improved-tangent method takes at image i: "rising", "falling", or at an extremum "up" / "down" (E[i + 1]
    above / not above E[i - 1]) with "max" / "min" in front."""
    if E[i + 1] > E[i] > E[i - 1]:
        return "rising"
    if E[i + 1] < E[i] < E[i - 1]:
        return "falling"
    kind = "max" if E[i] >= max(E[i - 1], E[i + 1]) else "min" if E[i] <= min(E[i - 1], E[i + 1]) else "flat"
    return kind + (" up" if E[i + 1] > E[i - 1] else " down")


def triclinic(rng, a=6.0):
    """A cell of edge about ``a`` with every off-diagonal entry set."""
    return a * np.eye(3) + rng.uniform(-0.15 * a, 0.15 * a, (3, 3))


def random_band(rng, n, M, cell, hop=0.8, noise=0.05, pushed=()):
    """A band of M images of n atoms near the straight line between two random endpoints ``hop`` apart per atom, the interior
    images jittered by ``noise``; the images ``pushed`` have every other atom moved by a lattice vector, which the minimum
    image convention has to undo.  -> (R [M, n, 3], raw forces [M - 2, n, 3])."""
    first = rng.uniform(0.0, 1.0, (n, 3)) @ cell
    last = first + rng.normal(0.0, hop, (n, 3)) / np.sqrt(3.0)
    w = np.linspace(0.0, 1.0, M)[:, None, None]
    R = (1.0 - w) * first[None] + w * last[None]
    R[1:-1] += rng.normal(0.0, noise, (M - 2, n, 3))
    for i in pushed:
        R[i, ::2] += rng.integers(-1, 2, (len(R[i, ::2]), 3)).astype(np.float64) @ cell
    return R, rng.normal(0.0, 1.0, (M - 2, n, 3))


# --- a vacancy hop in fcc, for the pair potential of tests/pair_ref.py -----------------------------------------------------------
A, RC = 4.0, 3.4


def vacancy_hop(asymmetric=False):
    """Case A: the 31-atom fcc cell with one site removed; the final image has the vacancy's nearest neighbour (row 0) on the
    vacancy.  Case B: row 5 of the final image displaced as well."""
    lat, pos = defects_ref.fcc(A)
    cell, first, _, _ = defects_ref.supercell(lat, pos, (2, 2, 2), removed=0)
    last = first.copy()
    last[0] = defects_ref.supercell(lat, pos, (2, 2, 2))[1][0]
    if asymmetric:
        last[5] += np.array([0.25, 0.10, -0.05])
    return cell, first, last
