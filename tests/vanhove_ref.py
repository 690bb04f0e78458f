"""The numpy restatement of the van Hove analysis (alignn_amd/vanhove.py, csrc/vanhove.hip; include/alignn_vanhove.h states the
formulas), one structure at a time and on the frames already selected.  A support module: it holds no tests.

What is restated operation for operation, because the device's bits are compared with it: the displacement of the self part and
the pair distances of the distinct part (the centre of mass, the wrap, the image shifts, the association of every sum), hence
every histogram; r^2 and r^2 r^2 of every term of the moments; the normalisations.  The sums OVER the terms are taken in extended
precision instead (``traj_ref._true_sum``): they stand for the true sum, which the device's fixed-order sum is compared with under
a bound derived from the number of terms.  The conventions - groups, centre of mass, origins, image range - are those of
tests/traj_ref.py, the reciprocal vectors and the phases those of tests/order_ref.py.

Every histogram function also returns the smallest distance of a term's r from a bin edge or from r_max, in bin widths, and the
number of terms.  The edge at r = 0 is not among them: no r lies below it, so the last bits of r cannot move a term across it
(at lag 0 every self displacement is exactly 0)."""

import itertools

import numpy as np

from tests import order_ref
from tests.defects_ref import inv3_cof, row_dot
from tests.traj_ref import (EDGE_MARGIN, _true_sum, com, det_cof, group_counts, image_range, members, n_origins, pair_row,  # noqa: F401
                            row_groups)


def origins(F, k, stride):
    """t = 0, stride, 2 stride, ... with t + k <= F - 1: ``traj_ref.n_origins(F, k, stride)`` of them."""
    ts = np.arange(0, F - k, stride)
    assert len(ts) == n_origins(F, k, stride)
    return ts


def _centres(traj, masses, remove_com):
    return com(traj, masses) if remove_com else np.zeros((np.asarray(traj).shape[0], 3))


def _margin(x, n_bins):
    """The smallest distance of the scaled distances x = r (n_bins / r_max) from the edges 1 .. n_bins, in bin widths."""
    near = x < n_bins + 0.5
    if not near.any():
        return np.inf
    return float(np.abs(x[near] - np.maximum(np.round(x[near]), 1.0)).min())


def shells(r_max, n_bins):
    """-> (dr, the shell volumes 4 pi / 3 (r_{j+1}^3 - r_j^3), the bin centres)."""
    dr = r_max / float(n_bins)
    j = np.arange(n_bins, dtype=np.float64)
    r0, r1 = j * dr, (j + 1.0) * dr
    return dr, (4.0 * np.pi / 3.0) * ((r1 * r1) * r1 - (r0 * r0) * r0), (j + 0.5) * dr


# --- the self part ------------------------------------------------------------------------------------------------------------------
def displacements(traj, c, k, stride):
    """[origins, n] r^2 and r of d = (r_i(t + k) - r_i(t)) - (c(t + k) - c(t)), the kernel's operations."""
    ts = origins(len(traj), k, stride)
    d = (traj[ts + k] - traj[ts]) - (c[ts + k] - c[ts])[:, None, :]
    r2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
    return r2, np.sqrt(r2)


def j0(x):
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(x == 0.0, 1.0, np.sin(x) / x)


def self_part(traj, rank, S, masses, lags, stride, remove_com, r_max, n_bins, q=()):
    """``traj`` [F, n, 3] -> (a dict: ``counts`` [S + 1, L, n_bins] and ``overflow`` [S + 1, L] int64, ``moments`` [S + 1, L, 2]
    (<r^2>, <r^4>), ``terms`` [S + 1, L] (the terms of every sum), ``fs`` [S + 1, L, n_q]; the smallest margin; the number of
    terms binned)."""
    traj = np.asarray(traj, dtype=np.float64)
    F, L, nq = traj.shape[0], len(lags), len(q)
    c = _centres(traj, masses, remove_com)
    count = group_counts(rank, S)
    counts, overflow = np.zeros((S + 1, L, n_bins), dtype=np.int64), np.zeros((S + 1, L), dtype=np.int64)
    moments, terms, fs = np.zeros((S + 1, L, 2)), np.zeros((S + 1, L), dtype=np.int64), np.zeros((S + 1, L, nq))
    scale = float(n_bins) / r_max
    margin, binned = np.inf, 0
    for l, k in enumerate(lags):
        r2, r = displacements(traj, c, int(k), stride)
        x = r * scale
        margin = min(margin, _margin(x, n_bins))
        kb = np.floor(x)
        inside = (r < r_max) & (kb < n_bins)
        binned += r.size
        for g in range(S + 1):
            if count[g] == 0:
                continue
            sel = members(rank, g)
            counts[g, l] = np.bincount(kb[:, sel][inside[:, sel]].astype(np.int64), minlength=n_bins)
            overflow[g, l] = int((~inside[:, sel]).sum())
            terms[g, l] = r2[:, sel].size
            norm = float(r2.shape[0]) * float(count[g])
            moments[g, l, 0], moments[g, l, 1] = _true_sum(r2[:, sel]) / norm, _true_sum(r2[:, sel] * r2[:, sel]) / norm
            for u, qu in enumerate(q):
                fs[g, l, u] = _true_sum(j0(float(qu) * r[:, sel])) / norm
    return dict(counts=counts, overflow=overflow, moments=moments, terms=terms, fs=fs), margin, binned


def alpha2(moments):
    """3 <r^4> / (5 <r^2>^2) - 1 in the kernel's association, 0 where <r^2> = 0.  ``moments`` [..., 2]."""
    m2, m4 = moments[..., 0], moments[..., 1]
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(m2 != 0.0, (3.0 * m4) / (5.0 * (m2 * m2)) - 1.0, 0.0)


def self_normalise(counts, F, lags, stride, count, r_max):
    """``counts`` [S + 1, L, n_bins] -> (p, gs, the bin centres)."""
    n_bins = counts.shape[-1]
    dr, shell, centres = shells(r_max, n_bins)
    p, gs = np.zeros(counts.shape), np.zeros(counts.shape)
    for l, k in enumerate(lags):
        for g in range(counts.shape[0]):
            if count[g] > 0:
                norm = float(n_origins(F, int(k), stride)) * float(count[g])
                p[g, l] = counts[g, l].astype(np.float64) / (norm * dr)
                gs[g, l] = counts[g, l].astype(np.float64) / (norm * shell)
    return p, gs, centres


# --- the distinct part --------------------------------------------------------------------------------------------------------------
def cross_distances(C, xi, xj, r_max):
    """Every ordered (i, j, image) from the rows ``xi`` to the rows ``xj`` (another frame of the same atoms) but, for j = i, the
    image m = rint(df), the atom's own unwrapped displacement: -> (i, j, r), all images of the range, r not yet cut.  The kernel's operations, those of
    ``traj_ref.pair_distances``."""
    C = np.asarray(C, dtype=np.float64)
    n = len(xi)
    dp = (xj[None, :, :] - xi[:, None, :]).reshape(-1, 3)  # [i, j] = x_j - x_i
    df = row_dot(dp, inv3_cof(C))
    shift = np.round(df)  # (half to even, as rint)
    df = df - shift
    d0 = row_dot(df, C)
    M = image_range(C, r_max)
    I, J = np.divmod(np.arange(n * n), n)
    out_i, out_j, out_r = [], [], []
    for m0, m1, m2 in itertools.product(*[range(-m, m + 1) for m in M]):
        s = (m0 * C[0] + m1 * C[1]) + m2 * C[2]
        d = d0 + s
        r = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
        own = (I == J) & (shift[:, 0] == m0) & (shift[:, 1] == m1) & (shift[:, 2] == m2)  # d0 + shift C = x_j - x_i, unwrapped
        out_i.append(I[~own])
        out_j.append(J[~own])
        out_r.append(r[~own])
    return np.concatenate(out_i), np.concatenate(out_j), np.concatenate(out_r)


def distinct_counts(traj, C, rank, S, masses, lags, stride, remove_com, r_max, n_bins):
    """``traj`` [F, n, 3] in the fixed cell ``C`` -> (counts [P, L, n_bins] int64, the smallest margin, the number of terms
    binned)."""
    traj = np.asarray(traj, dtype=np.float64)
    F, P = traj.shape[0], 1 + S * (S + 1) // 2
    c = _centres(traj, masses, remove_com)
    x = traj - c[:, None, :]
    counts = np.zeros((P, len(lags), n_bins), dtype=np.int64)
    rows_of = np.array([[pair_row(a, b) if a and b else 0 for b in range(S + 1)] for a in range(S + 1)], dtype=np.int64)
    scale = float(n_bins) / r_max
    margin, binned = np.inf, 0
    for l, k in enumerate(lags):
        for t in origins(F, int(k), stride):
            I, J, r = cross_distances(C, x[t], x[t + int(k)], r_max)
            xs = r * scale
            margin = min(margin, _margin(xs, n_bins))
            kb = np.floor(xs)
            keep = (r < r_max) & (kb < n_bins)
            rows = rows_of[rank[I[keep]], rank[J[keep]]]
            np.add.at(counts[:, l], (rows, kb[keep].astype(np.int64)), 1)
            np.add.at(counts[0, l], kb[keep].astype(np.int64), 1)
            binned += int(keep.sum())
    return counts, margin, binned


def distinct_normalise(counts, C, F, lags, stride, count, r_max):
    """``counts`` [P, L, n_bins] -> (g, V, the bin centres)."""
    P, L, n_bins = counts.shape
    V = abs(det_cof(C))
    _, shell, centres = shells(r_max, n_bins)
    g = np.zeros(counts.shape)
    for p in range(P):
        a, b = row_groups(p)
        Na, Nb, w = float(count[a]), float(count[b]), 2.0 if a < b else 1.0
        if Na > 0 and Nb > 0:
            for l, k in enumerate(lags):
                n = float(n_origins(F, int(k), stride))
                g[p, l] = (counts[p, l].astype(np.float64) * V) / ((((n * Na) * Nb) * w) * shell)
    return g, V, centres


# --- the intermediate scattering function ---------------------------------------------------------------------------------------------
def intermediate_scattering(traj, C, rank, S, q_max, n_bins, lags, stride):
    """-> a dict: ``hkl`` [V, 3], ``f_vectors`` [P, L, V], ``scale`` [P, L, V] (sum_t |rho'| |rho| / (n_origins sqrt(N_a N_b)),
    what a deviation of ``f_vectors`` is measured against), ``f`` [P, L, n_bins], ``n_vectors`` [n_bins], ``q`` [n_bins]."""
    C, traj = np.asarray(C, dtype=np.float64), np.asarray(traj, dtype=np.float64)
    hkl, _, shell_of, _ = order_ref.sq_vectors(C, q_max, n_bins)
    F, P, V, L = len(traj), 1 + S * (S + 1) // 2, len(hkl), len(lags)
    count = group_counts(rank, S)
    f_vec, scale = np.zeros((P, L, V)), np.zeros((P, L, V))
    if V and F:
        ph = order_ref.phases(traj, C, hkl)
        rho = [None] + [ph[:, rank == g].sum(1) for g in range(1, S + 1)]  # [F, V] each
        rho[0] = sum(rho[2:], rho[1])
        for p in range(P):
            a, b = row_groups(p)
            if count[a] == 0 or count[b] == 0:
                continue
            for l, k in enumerate(lags):
                ts = origins(F, int(k), stride)
                norm = float(len(ts)) * np.sqrt(float(count[a]) * float(count[b]))
                ab = (rho[a][ts + int(k)] * np.conj(rho[b][ts])).real
                ba = (rho[b][ts + int(k)] * np.conj(rho[a][ts])).real
                f_vec[p, l] = (0.5 * (ab + ba)).astype(np.longdouble).sum(0).astype(np.float64) / norm
                mag = 0.5 * (np.abs(rho[a][ts + int(k)]) * np.abs(rho[b][ts]) + np.abs(rho[b][ts + int(k)]) * np.abs(rho[a][ts]))
                scale[p, l] = mag.sum(0) / norm
    n_vectors = np.bincount(shell_of, minlength=n_bins).astype(np.int64)
    f = np.zeros((P, L, n_bins))
    for p in range(P):
        for l in range(L):
            tot = np.bincount(shell_of, weights=f_vec[p, l], minlength=n_bins)
            f[p, l] = np.where(n_vectors > 0, tot / np.maximum(n_vectors, 1), 0.0)
    return dict(hkl=hkl, f_vectors=f_vec, scale=scale, f=f, n_vectors=n_vectors, shell_of=shell_of,
                q=(np.arange(n_bins) + 0.5) * (q_max / float(n_bins)))


# --- the inputs of the device tests (tests/test_gpu_vanhove.py, tests/test_gpu_vanhove_extents.py), those of tests/test_gpu_trajectory.py ----
SIZES = [1, 5, 70]
SPECIES = [np.array([14]), np.array([8, 3, 8, 3, 3]), np.array([22, 8, 38] * 23 + [8])]
FIVE = [SPECIES[0], SPECIES[1], np.arange(70) % 5 + 20]  # five species in the large structure: the self histograms go in two chunks
CELLS = np.array([[[3.15, 0.0, 0.0], [0.4, 3.15, 0.0], [0.3, -0.35, 3.2]],
                  [[4.0, 0.0, 0.0], [1.3, 3.8, 0.0], [0.7, -0.9, 4.4]],
                  [[13.0, 0.0, 0.0], [0.6, 13.5, 0.0], [-0.4, 0.5, 14.0]]])
R_MAX = 6.0
PTR = np.concatenate([[0], np.cumsum(SIZES)])
FRAMES, LAGS, SEED = 9, (0, 1, 3, 8), 21
Q = (0.7, 2.1, 6.5)
Q_MAX, Q_BINS = 4.5, 40
_CACHE = {}


def rows(b):
    return slice(PTR[b], PTR[b + 1])


def inputs():
    """FRAMES = 9 frames: random fractional positions, a random walk of N(0, 0.15 A) steps, and every atom jumps by whole cells
    (-2 .. 2 per axis) between two frames with probability 0.3 - so a displacement is wrapped to another image more often than
    not, and many atoms move by more than half a cell.  Non-uniform masses."""
    if "inputs" not in _CACHE:
        rng = np.random.default_rng(SEED)
        traj = np.zeros((FRAMES, PTR[-1], 3))
        for b, n in enumerate(SIZES):
            frac = rng.uniform(0, 1, (n, 3))
            jump = np.cumsum(rng.integers(-2, 3, (FRAMES, n, 3)) * (rng.uniform(0, 1, (FRAMES, n, 1)) < 0.3), axis=0)
            walk = np.cumsum(rng.normal(0.0, 0.15, (FRAMES, n, 3)), axis=0)
            traj[:, rows(b)] = (frac[None] + jump) @ CELLS[b] + walk
        _CACHE["inputs"] = traj, [rng.uniform(1.0, 100.0, n) for n in SIZES]
    return _CACHE["inputs"]


def selected(select):
    sel = dict(start=select[0], step=select[1]) if select else {}
    frames = list(range(FRAMES)[slice(sel.get("start"), None, sel.get("step"))])
    lags = tuple(k for k in LAGS if k < len(frames))
    return sel, frames, lags
