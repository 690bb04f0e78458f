"""The executable specification of ``alignn_amd.eos`` (csrc/eos.hip): float64 numpy restatements of the strained-structure
builder and of the equation-of-state fit of the reference's ``ev_curve`` (alignn/ff/ff.py:762-805), which strains a crystal with
jarvis-tools' ``Atoms.strain_atoms`` and fits with ASE's ``EquationOfState(vol, e, eos="murnaghan").fit()`` (ase/eos.py: two
``scipy.optimize.curve_fit`` calls).  ASE and jarvis-tools are not dependencies of this project; ``ase_fit`` is ASE's procedure on
scipy.

The builder is written operation for operation as the kernel is - every three-term sum as ``(x + y) + z``, elementwise numpy
only - so the device results are expected to be the same bits.  The fit follows the kernel step for step too, its sums over
the strain points in the kernel's order (``wave_sum``: the 64-lane butterfly).  Its stopping tests sit at the rounding level of
the residuals, so the number of steps - and the parameters in their eighth digit - follow the last bits of x^BP: perturbing
``log`` / ``exp`` by one unit in the last place changes ``n_iter`` on most of the inputs of the tests.  The device's ``pow`` and
``log`` are not libm's, so neither is used: ``flog`` / ``fexp`` below are written in +, -, *, / and ``frexp`` / ``ldexp`` only
(within 3 units in the last place of libm), the kernel has the same two functions, and the fit is expected to be the same bits
as well.  tests/test_eos_ref.py pins this file against ``ase_fit``; tests/test_gpu_eos.py holds the kernels to it."""

import numpy as np

MURNAGHAN, BIRCH_MURNAGHAN = 0, 1
FORMS = {"murnaghan": MURNAGHAN, "birchmurnaghan": BIRCH_MURNAGHAN}
EV_A3_TO_GPA = 160.21766208
WAVE = 64
LAMBDA0, LAMBDA_MIN, LAMBDA_MAX = 1e-3, 1e-15, 1e15
XTOL, FTOL, MAX_STEPS = 1e-13, 1e-16, 100


# --- the strain builder ----------------------------------------------------------------------------------------------------------
def row_dot(x, m):
    """x [rows, 3] times m [3, 3]: (x0 m0k + x1 m1k) + x2 m2k."""
    return (x[:, 0:1] * m[0] + x[:, 1:2] * m[1]) + x[:, 2:3] * m[2]


def strain(lat, pos, F):
    """alignn_strain_build for one job: -> (cell [3, 3], cart [n, 3], volume).  Row i of the cell is row i of the parent times
    F, every Cartesian position r' = r F, both as ``row_dot``; the volume is |det| of the NEW cell along its first row,
    ``(c0 (c4 c8 - c5 c7) - c1 (c3 c8 - c5 c6)) + c2 (c3 c7 - c4 c6)``."""
    lat, pos, F = (np.asarray(x, dtype=np.float64) for x in (lat, pos, F))
    cell, cart = row_dot(lat, F), row_dot(pos, F)
    c = [float(v) for v in cell.reshape(-1)]
    det = (c[0] * (c[4] * c[8] - c[5] * c[7]) - c[1] * (c[3] * c[8] - c[5] * c[6])) + c[2] * (c[3] * c[7] - c[4] * c[6])
    return cell, cart, abs(det)


def isotropic(dx):
    """The deformation of ``ev_curve``: (1 + dx) I."""
    return (1.0 + float(dx)) * np.eye(3)


# --- log and exp in plain arithmetic ---------------------------------------------------------------------------------------------
LN2_HI, LN2_LO = 6.93147180369123816490e-01, 1.90821492927058770002e-10  # ln 2 = hi + lo, the low 21 bits of hi zero
INV_LN2, SQRT_HALF = 1.44269504088896338700e+00, 0.70710678118654752440


def flog(x):
    """ln x for finite x > 0, NaN otherwise.  x = 2^e m with m in [sqrt(1/2), sqrt(2)), s = (m - 1) / (m + 1), z = s^2:
    ln m = 2 s (1 + z / 3 + ... + z^11 / 23) by Horner (z <= 0.0295: the first term left out is 2e-20), and
    ln x = (e ln2_hi + ln m) + e ln2_lo."""
    x = np.asarray(x, dtype=np.float64)
    ok = (x > 0.0) & (x < np.inf)
    m, e = np.frexp(np.where(ok, x, 1.0))
    low = m < SQRT_HALF
    m, e = np.where(low, m + m, m), np.where(low, e - 1, e).astype(np.float64)
    s = (m - 1.0) / (m + 1.0)
    z = s * s
    p = 1.0 / 23.0
    for d in range(21, 0, -2):
        p = 1.0 / d + z * p
    return np.where(ok, (e * LN2_HI + (2.0 * s) * p) + e * LN2_LO, np.nan)


def fexp(x):
    """e^x for |x| <= 700; inf above, 0 below, NaN for NaN.  k = floor(x / ln 2 + 1/2), r = (x - k ln2_hi) - k ln2_lo (|r| <=
    0.347), e^r by its Taylor polynomial of degree 13 as p = 1 + r p / n for n = 13 ... 1 (the first term left out is 4e-18),
    then ldexp(p, k)."""
    x = np.asarray(x, dtype=np.float64)
    ok = np.abs(x) <= 700.0
    xs = np.where(ok, x, 0.0)
    k = np.floor(xs * INV_LN2 + 0.5)
    r = (xs - k * LN2_HI) - k * LN2_LO
    p = 1.0
    for n in range(13, 0, -1):
        p = 1.0 + (r * p) / float(n)
    return np.where(ok, np.ldexp(p, k.astype(np.int32)), np.where(x > 700.0, np.inf, np.where(x < -700.0, 0.0, np.nan)))


# --- the two forms, as ase/eos.py writes them, and their Jacobians -----------------------------------------------------------------
def murnaghan(V, E0, B0, BP, V0):
    return E0 + B0 * V / BP * (((V0 / V) ** BP) / (BP - 1) + 1) - V0 * B0 / (BP - 1)


def birchmurnaghan(V, E0, B0, BP, V0):
    eta = (V0 / V) ** (1 / 3)
    return E0 + 9 * B0 * V0 / 16 * (eta ** 2 - 1) ** 2 * (6 + BP * (eta ** 2 - 1) - 4 * eta ** 2)


def parabola(x, a, b, c):
    return a + b * x + c * x ** 2


ASE_FORMS = {MURNAGHAN: murnaghan, BIRCH_MURNAGHAN: birchmurnaghan}


def model(form, V, p):
    """The kernel's statement of the form at p = (E0, B0, BP, V0): -> (E [K], J [K, 4] = dE / dp), the operations in the
    kernel's order."""
    E0, B0, BP, V0 = (float(v) for v in p)
    V = np.asarray(V, dtype=np.float64)
    x = V0 / V
    if form == MURNAGHAN:
        lx = flog(x)
        t = fexp(BP * lx)  # x^BP
        q = BP - 1.0
        u = t / q + 1.0
        E = (E0 + (B0 * V) / BP * u) - (V0 * B0) / q
        dB0 = V / BP * u - V0 / q
        dBP = (B0 * V) * ((t * lx / q - t / (q * q)) / BP - u / (BP * BP)) + (V0 * B0) / (q * q)
        dV0 = B0 * (t / x - 1.0) / q
    else:
        y = fexp((2.0 / 3.0) * flog(x))  # eta^2 = x^(2/3)
        f = y - 1.0
        P = (6.0 + BP * f) - 4.0 * y
        f2 = f * f
        E = E0 + (0.5625 * B0 * V0) * (f2 * P)
        dB0 = (0.5625 * V0) * (f2 * P)
        dBP = (0.5625 * B0 * V0) * (f2 * f)
        dV0 = (0.5625 * B0) * (f2 * P + (2.0 / 3.0) * y * ((2.0 * f) * P + f2 * (BP - 4.0)))
    return E, np.stack([np.ones_like(V), dB0, dBP, dV0], axis=1)


# --- the sums of a wavefront ---------------------------------------------------------------------------------------------------------
def _butterfly(v, op, fill):
    w = np.full(WAVE, fill, dtype=np.float64)
    w[:len(v)] = v
    lane = np.arange(WAVE)
    for o in (32, 16, 8, 4, 2, 1):
        w = op(w, w[lane ^ o])
    assert (w == w[0]).all() or np.isnan(w).all()  # (a + b == b + a: every lane ends with the same bits)
    return float(w[0])


def wave_sum(v):
    """The sum over the strain points as the kernel takes it: one value per lane, 0 in the lanes past K, then the xor
    butterfly over the offsets 32, 16, 8, 4, 2, 1."""
    return _butterfly(v, np.add, 0.0)


def wave_max(v):
    return _butterfly(v, np.fmax, -np.inf)


def wave_min(v):
    return _butterfly(v, np.fmin, np.inf)


# --- the parabola start --------------------------------------------------------------------------------------------------------------
def cholesky_solve(A, b):
    """Solve A x = b for a symmetric positive definite A [n, n] by Cholesky (lower triangle, row by row, every inner sum in
    ascending index order): -> x, or None where a pivot is not > 0 or not finite."""
    n = len(b)
    L = np.zeros((n, n))
    for i in range(n):
        for j in range(i + 1):
            s = float(A[i][j])
            for k in range(j):
                s = s - L[i, k] * L[j, k]
            if i == j:
                if not (s > 0.0 and np.isfinite(s)):
                    return None
                L[i, i] = np.sqrt(s)
            else:
                L[i, j] = s / L[j, j]
    y = np.zeros(n)
    for i in range(n):
        s = float(b[i])
        for k in range(i):
            s = s - L[i, k] * y[k]
        y[i] = s / L[i, i]
    x = np.zeros(n)
    for i in range(n - 1, -1, -1):
        s = y[i]
        for k in range(i + 1, n):
            s = s - L[k, i] * x[k]
        x[i] = s / L[i, i]
    return x


def parabola_start(V, E):
    """Step 1: the least-squares parabola in u = (V - mean V) / (max V - min V), mapped back to a + b V + c V^2, and ASE's start
    values from it: -> (E0, B0, BP, V0) or None (c <= 0 or a non-finite value)."""
    V, E = np.asarray(V, dtype=np.float64), np.asarray(E, dtype=np.float64)
    K = len(V)
    with np.errstate(all="ignore"):
        m = wave_sum(V) / float(K)
        w = wave_max(V) - wave_min(V)
        u = (V - m) / w
        u2 = u * u
        s1, s2, s3, s4 = wave_sum(u), wave_sum(u2), wave_sum(u2 * u), wave_sum(u2 * u2)
        t0, t1, t2 = wave_sum(E), wave_sum(E * u), wave_sum(E * u2)
        sol = cholesky_solve([[float(K), s1, s2], [s1, s2, s3], [s2, s3, s4]], [t0, t1, t2])
        if sol is None:
            return None
        a1, b1, c1 = (float(v) for v in sol)
        c = c1 / (w * w)
        b = b1 / w - (2.0 * c) * m
        a = (a1 - (b1 / w) * m) + (c * m) * m
        vmin = -b / (2.0 * c)
        p = np.array([(a + b * vmin) + (c * vmin) * vmin, (2.0 * c) * vmin, 4.0, vmin])
    if not (c > 0.0) or not np.isfinite(p).all():
        return None
    return p


# --- the Levenberg-Marquardt loop ------------------------------------------------------------------------------------------------------
def _sumsq(form, V, E, p):
    r = model(form, V, p)[0] - E
    return wave_sum(r * r)


def fit(V, E, form=MURNAGHAN):
    """alignn_eos_fit for one structure: -> dict(params = (E0, B0, BP, V0), rms, n_iter, status).

    status 0: converged; 1: 100 accepted steps without it (the parameters as they stand); 2: no start (fewer than 4 or more than
    64 points, the parabola opens downwards, or a non-finite value in the start or in its residuals): NaN parameters and rms,
    n_iter 0, no loop.

    The loop: S = sum r^2 at p, lambda = 1e-3.  A trial: A = J^T J and g = J^T r at p (the ten entries of A and the four of g
    one ``wave_sum`` each), (A + lambda diag A) delta = -g by Cholesky, S' at p + delta.  Where S' is finite and S' <= S the
    step is taken: n_iter += 1, lambda = max(lambda / 10, 1e-15), and the fit has converged when max |delta| <= 1e-13 max |p +
    delta| or S - S' <= 1e-16 S.  Otherwise (a failed Cholesky too) lambda = 10 lambda and the trial is repeated at the same p;
    lambda > 1e15 ends the fit as converged: no step of any length lowers S, p is a minimum to rounding.  rms = sqrt(S / K)."""
    V, E = np.asarray(V, dtype=np.float64), np.asarray(E, dtype=np.float64)
    K = len(V)
    nan = dict(params=np.full(4, np.nan), rms=np.nan, n_iter=0, status=2)
    p = parabola_start(V, E) if 4 <= K <= WAVE else None
    if p is None:
        return nan
    with np.errstate(all="ignore"):
        S = _sumsq(form, V, E, p)
        if not np.isfinite(S):
            return nan
        lam, n_iter, status = LAMBDA0, 0, 1
        while n_iter < MAX_STEPS:
            Em, J = model(form, V, p)
            r = Em - E
            A = np.zeros((4, 4))
            g = np.zeros(4)
            for i in range(4):
                for j in range(i + 1):
                    A[i, j] = A[j, i] = wave_sum(J[:, i] * J[:, j])
                g[i] = wave_sum(J[:, i] * r)
            done = False
            while True:
                M = A.copy()
                for i in range(4):
                    M[i, i] = A[i, i] + lam * A[i, i]
                delta = cholesky_solve(M, -g)
                S_new = np.nan
                if delta is not None:
                    p_new = p + delta
                    S_new = _sumsq(form, V, E, p_new)
                if np.isfinite(S_new) and S_new <= S:
                    n_iter += 1
                    lam = max(lam / 10.0, LAMBDA_MIN)
                    done = bool(np.abs(delta).max() <= XTOL * np.abs(p_new).max() or S - S_new <= FTOL * S)
                    p, S = p_new, S_new
                    break
                lam = lam * 10.0
                if lam > LAMBDA_MAX:
                    done = True
                    break
            if done:
                status = 0
                break
    return dict(params=p, rms=float(np.sqrt(S / float(K))), n_iter=n_iter, status=status)


# --- ASE's procedure on scipy ----------------------------------------------------------------------------------------------------------
def ase_fit(v, e, form=MURNAGHAN, tol=None):
    """ase/eos.py ``EquationOfState.fit`` for eos = "murnaghan" / "birchmurnaghan": ``curve_fit`` of the parabola from p0 =
    [min(e), 1, 1], ASE's start values from it, ``curve_fit`` of the form.  ``tol``: ftol = xtol = gtol of both calls (default:
    scipy's, as ASE runs it).  -> (E0, B0, BP, V0); ``curve_fit`` raises a RuntimeError where MINPACK does not converge (its
    warning that four points leave no covariance for four parameters is not one)."""
    import warnings

    from scipy.optimize import OptimizeWarning, curve_fit

    kw = {} if tol is None else dict(ftol=tol, xtol=tol, gtol=tol)
    v, e = np.asarray(v, dtype=np.float64), np.asarray(e, dtype=np.float64)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", OptimizeWarning)
        (a, b, c), _ = curve_fit(parabola, v, e, [min(e), 1, 1], **kw)
        vmin = -b / 2 / c
        p0 = [parabola(vmin, a, b, c), 2 * c * vmin, 4, vmin]
        popt, _ = curve_fit(ASE_FORMS[form], v, e, p0, **kw)
    return np.asarray(popt, dtype=np.float64)


# --- the inputs of the tests -------------------------------------------------------------------------------------------------------------
TRUE = (-3.2, 0.6, 4.5, 65.0)  # (E0, B0, BP, V0) of the synthetic curves
DX_DEFAULT = np.arange(-0.05, 0.05, 0.01)
DX_5 = np.array([-0.04, -0.02, 0.0, 0.03, 0.05])
DX_4 = np.array([-0.03, -0.01, 0.01, 0.03])


def synthetic_sets(form=MURNAGHAN):
    """name -> (V, E): the exact curve of ``TRUE`` on V = 64 (1 + dx)^3 for the default ten strains, five uneven ones and four
    (the smallest K), and each with normal noise of 1e-4 eV (fixed seed)."""
    rng = np.random.default_rng(20240607)
    out = {}
    for name, dx in (("k10", DX_DEFAULT), ("k5", DX_5), ("k4", DX_4)):
        V = 64.0 * (1.0 + dx) ** 3
        E = ASE_FORMS[form](V, *TRUE)
        out[name] = (V, E)
        out[name + "_noise"] = (V, E + rng.normal(0.0, 1e-4, len(V)))
    return out


def concave(dx=DX_5):
    V = 64.0 * (1.0 + np.asarray(dx)) ** 3
    return V, -V * V
