"""The executable specification of ``alignn_amd.idpp`` (csrc/idpp.hip): float64 numpy restatements of ASE 3.22's image dependent
pair potential (``ase/neb.py``: class ``IDPP`` and ``NEB.idpp_interpolate``) with the plain-wrap minimum image convention of
tests/neb_ref.py in place of ASE's ``find_mic``, and of the pass that relaxes a band on it - ``neb_ref.neb_forces`` with
relax_ref's FIRE where ASE's default is ``MDMin``, which this project does not have.  ASE is not a dependency of this project.

For image m of a band of M images, atom a and every b != a:
    D_ab = mic(R_a - R_b), d_ab = |D_ab|, t_ab(m) = d1_ab + m ((d2_ab - d1_ab) / (M - 1)), delta = d_ab - t_ab(m)
    E_m = 1/2 sum_a sum_{b != a} delta^2 / d_ab^4,   F_a = -2 sum_{b != a} delta (1 - 2 delta / d_ab) / d_ab^5 D_ab
with d1 and d2 the same distances in image 0 and in image M - 1.  A pair's term is written operation for operation as the kernel
writes it; the sums over b and over a are numpy's, so the two agree to the rounding of a sum of n terms.
tests/test_idpp_ref.py pins this file by the gradient of its own energy; tests/test_gpu_idpp.py holds the kernel and the driver
to it.  This module holds no tests."""

import numpy as np

from tests import neb_ref
from tests.defects_ref import inv3_cof, row_dot
from tests.relax_ref import run_fixed_ref, run_ref


def pair_vectors(R, C):
    """D [n, n, 3] with D[a, b] = mic(R_a - R_b), and d [n, n] = |D| (the diagonal is zero)."""
    R = np.asarray(R, dtype=np.float64)
    n = len(R)
    D = neb_ref.mic((R[:, None, :] - R[None, :, :]).reshape(-1, 3), C).reshape(n, n, 3)
    return D, np.sqrt((D[..., 0] * D[..., 0] + D[..., 1] * D[..., 1]) + D[..., 2] * D[..., 2])


def targets(d1, d2, m, M):
    """t(m) = d1 + m ((d2 - d1) / (M - 1)) for the pair distances d1 of image 0 and d2 of image M - 1."""
    return d1 + float(m) * ((d2 - d1) / float(M - 1))


def _terms(R, t, C):
    """Per ordered pair: the energy term delta^2 / d^4 [n, n] and the force term c D [n, n, 3], zero on the diagonal."""
    D, d = pair_vectors(R, C)
    off = ~np.eye(len(d), dtype=bool)
    with np.errstate(invalid="ignore", divide="ignore"):
        delta = d - t
        dd = d * d
        d4 = dd * dd
        e = np.where(off, (delta * delta) / d4, 0.0)
        c = np.where(off, (delta * (1.0 - (2.0 * delta) / d)) / (d4 * d), 0.0)
    return e, c[..., None] * D


def objective(R, t, C):
    """(E, F [n, 3]) of one image with positions ``R`` [n, 3] and target distances ``t`` [n, n] in the cell ``C``."""
    e, f = _terms(R, t, C)
    return 0.5 * float(e.sum(1).sum()), -2.0 * f.sum(1)


def scales(R, t, C):
    """What a comparison of ``objective`` is measured against: (sum over all pairs of |energy term|, per row a the sum over b
    of the length of the force term 2 |c| d)."""
    e, f = _terms(R, t, C)
    return 0.5 * float(np.abs(e).sum()), 2.0 * np.sqrt((f * f).sum(-1)).sum(1)


def wrap_margin(R, C):
    """The smallest distance of any pair's fractional difference component (before the wrap) from a half-integer: how far the
    image is from a pair changing its periodic image.  inf for a single atom."""
    R = np.asarray(R, dtype=np.float64)
    n = len(R)
    if n < 2:
        return np.inf
    f = row_dot((R[:, None, :] - R[None, :, :]).reshape(-1, 3), inv3_cof(np.asarray(C, dtype=np.float64))).reshape(n, n, 3)
    f = f[~np.eye(n, dtype=bool)]
    return float(np.abs(np.abs(f - np.round(f)) - 0.5).min())


def band_objective(R, C):
    """The IDPP energies [M] and forces [M - 2, n, 3] (interior images) of the band ``R`` [M, n, 3]."""
    R = np.asarray(R, dtype=np.float64)
    M = len(R)
    d1, d2 = pair_vectors(R[0], C)[1], pair_vectors(R[-1], C)[1]
    ev = [objective(R[m], targets(d1, d2, m, M), C) for m in range(1, M - 1)]
    return np.array([0.0] + [e for e, _ in ev] + [0.0]), np.stack([f for _, f in ev])


def run_band_ref(cell, initial, final, ef, rows0, e_first, e_last, k=0.1, climb=False, method="aseneb", fmax=0.05, steps=100,
                 fixed=None, fire=None, note=None):
    """``FIRE(NEB(images, k, climb, method)).run(fmax, steps)`` of a band from the given interior images ``rows0`` [M - 2, n, 3]:
    ``neb_ref.run_neb_ref`` with the start, the endpoint energies and the image index handed in.  ``ef(m, pos) -> (e, f)`` of
    image m.  ``note(R)`` is called with the band [M, n, 3] of every evaluation.  -> ``run_neb_ref``'s dict."""
    initial, final = np.asarray(initial, dtype=np.float64), np.asarray(final, dtype=np.float64)
    rows0 = np.asarray(rows0, dtype=np.float64)
    M, n = len(rows0) + 2, len(initial)
    last, margins = {}, {}

    def band(rows):
        R = np.concatenate([initial[None], rows.reshape(M - 2, n, 3), final[None]])
        if note is not None:
            note(R)
        ev = [ef(m, R[m]) for m in range(1, M - 1)]
        E = np.array([e_first] + [e for e, _ in ev] + [e_last], dtype=np.float64)
        g, imax = neb_ref.neb_forces(R, E, np.stack([f for _, f in ev]), k, climb, method, fixed, cell=cell, margins=margins)
        last.update(R=R, E=E, g=g, imax=imax)
        return E[imax], g.reshape(-1, 3)

    if fixed is None:
        run = run_ref(rows0.reshape(-1, 3), band, fmax=fmax, steps=steps, **(fire or {}))
    else:
        run = run_fixed_ref(rows0.reshape(-1, 3), band, np.tile(np.asarray(fixed, dtype=bool), M - 2), fmax=fmax, steps=steps,
                            fire=fire)
    E = last["E"]
    return dict(r=last["R"], e=E, f=last["g"], imax=last["imax"], barrier=E.max() - E[0], delta_e=E[-1] - E[0],
                n_steps=run["n_steps"], converged=run["converged"], n_evals=run["n_evals"], margins=margins,
                margin=min(margins.values()) if margins else np.inf)


def run_idpp_ref(cell, initial, final, n_images=3, k=0.1, method="aseneb", fmax=0.1, steps=100, fixed=None, fire=None):
    """``NEB.idpp_interpolate(fmax=fmax, steps=steps)`` with FIRE: the linear path of ``neb_ref.interpolate``, then the band's own
    NEB (no climbing image) on the IDPP objective.  -> ``run_band_ref``'s dict, with ``wrap`` added, the smallest
    ``wrap_margin`` over the interior images of every evaluation (the images that move), and ``wrap_ends``, that of the two
    endpoints (whose distances are the targets)."""
    initial, final = np.asarray(initial, dtype=np.float64), np.asarray(final, dtype=np.float64)
    M = n_images + 2
    d1, d2 = pair_vectors(initial, cell)[1], pair_vectors(final, cell)[1]
    wrap = [np.inf]

    def note(R):
        wrap[0] = min([wrap[0]] + [wrap_margin(r, cell) for r in R[1:-1]])

    out = run_band_ref(cell, initial, final, lambda m, pos: objective(pos, targets(d1, d2, m, M), cell),
                       neb_ref.interpolate(initial, final, cell, M), 0.0, 0.0, k, False, method, fmax, steps, fixed, fire, note)
    out["wrap"], out["wrap_ends"] = wrap[0], min(wrap_margin(initial, cell), wrap_margin(final, cell))
    return out


# --- the cases of the tests --------------------------------------------------------------------------------------------------------
TURN_CELL = np.array([[8.0, 0.0, 0.0], [0.7, 8.3, 0.0], [0.4, -0.6, 7.9]])
BOND = 1.6


def turning_dimer(angle=80.0):
    """A dimer of bond 1.6 A among six spectators in a triclinic cell; in the final image its centre is shifted and its axis
    turned by ``angle`` degrees in the xy plane, and three spectators are moved.  Rows 0 and 1 are the dimer.
    -> (cell, initial [8, 3], final [8, 3])."""
    centre, th = np.array([4.1, 4.2, 3.9]), np.deg2rad(angle)
    spectators = np.array([[1.0, 1.1, 0.9], [6.9, 1.3, 1.2], [1.2, 7.0, 1.0], [1.1, 0.8, 6.8], [6.8, 6.9, 6.7], [6.7, 1.0, 6.9]])
    axis0, axis1 = np.array([1.0, 0.0, 0.0]), np.array([np.cos(th), np.sin(th), 0.0])
    first = np.concatenate([[centre - 0.5 * BOND * axis0, centre + 0.5 * BOND * axis0], spectators])
    c1 = centre + np.array([0.3, 0.1, 0.2])
    moved = spectators.copy()
    moved[0] += [0.2, 0.0, 0.0]
    moved[2] += [0.0, -0.15, 0.1]
    moved[5] += [0.1, 0.1, 0.0]
    last = np.concatenate([[c1 - 0.5 * BOND * axis1, c1 + 0.5 * BOND * axis1], moved])
    return TURN_CELL.copy(), first, last


def bond(R, cell):
    """The dimer's bond length (rows 0 and 1) in every image of ``R`` [M, n, 3]."""
    return np.array([np.sqrt((neb_ref.mic((r[1] - r[0])[None], cell) ** 2).sum()) for r in np.asarray(R)])
