"""The numpy restatement of the trajectory analysis (alignn_amd/trajectory.py, csrc/trajectory.hip; include/alignn_traj.h states
the formulas), one structure at a time and on the frames already selected.  A support module: it holds no tests.

What is restated operation for operation, because the device's bits are compared with it: the pair distances of ``rdf_counts``
(the wrap, the image shifts, the association of every sum), the mean volume and the normalisation of g(r), the centre of mass
(row order) and every term of the MSD and the VACF.  The sums OVER the terms are taken in extended precision instead: they stand
for the true sum, which the device's fixed-order sum is compared with under a bound derived from the number of terms."""

import itertools

import numpy as np

from tests.defects_ref import inv3_cof, row_dot

FS = 0.09822694788464063  # alignn_amd.dynamics.FS: the femtosecond in ASE time units
EDGE_MARGIN = 1e-9  # in bin widths: the precondition of an exact comparison of histograms


def groups(species, n):
    """-> (rank [n]: the 1-based rank of every atom's species among the structure's, the species in ascending order)."""
    if species is None:
        return np.ones(n, dtype=np.int64), [0]
    uniq, inverse = np.unique(np.asarray(species), return_inverse=True)
    return inverse.reshape(-1) + 1, [int(u) for u in uniq]


def group_counts(rank, S):
    """[S + 1]: every atom, then the members of groups 1 .. S."""
    return np.concatenate([[len(rank)], np.bincount(rank, minlength=S + 1)[1:S + 1]])


def members(rank, g):
    return np.ones(len(rank), dtype=bool) if g == 0 else rank == g


def pair_row(a, b):
    """Row of the pair of groups a, b (1-based, either order): 1 + hi (hi - 1) / 2 + (lo - 1); row 0 is every pair."""
    lo, hi = min(a, b), max(a, b)
    return 1 + hi * (hi - 1) // 2 + (lo - 1)


def row_groups(p):
    """The inverse of ``pair_row``: row p -> (a, b), a <= b; row 0 -> (0, 0)."""
    if p == 0:
        return 0, 0
    hi = 1
    while hi * (hi + 1) // 2 < p:
        hi += 1
    return p - 1 - hi * (hi - 1) // 2 + 1, hi


def det_cof(C):
    a = [float(v) for v in np.asarray(C, dtype=np.float64).reshape(-1)]
    c00, c01, c02 = a[4] * a[8] - a[5] * a[7], a[3] * a[8] - a[5] * a[6], a[3] * a[7] - a[4] * a[6]
    return (a[0] * c00 - a[1] * c01) + a[2] * c02


def image_range(C, r_max):
    """floor(r_max / h_k + 1/2) per axis, h_k = |det| / |C_{k+1} x C_{k+2}|."""
    C = np.asarray(C, dtype=np.float64)
    vol = abs(det_cof(C))
    out = []
    for k in range(3):
        u, v = C[(k + 1) % 3], C[(k + 2) % 3]
        cx, cy, cz = u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0]
        out.append(int(np.floor(r_max / (vol / np.sqrt((cx * cx + cy * cy) + cz * cz)) + 0.5)))
    return out


def pair_distances(C, pos, r_max):
    """Every ordered (i, j, image) but (i, i, 0), the kernel's operations: -> (i, j, r), all images of the range, r not yet cut."""
    C, pos = np.asarray(C, dtype=np.float64), np.asarray(pos, dtype=np.float64)
    n = len(pos)
    dp = (pos[None, :, :] - pos[:, None, :]).reshape(-1, 3)  # [i, j] = r_j - r_i
    df = row_dot(dp, inv3_cof(C))
    df = df - np.round(df)  # (half to even, as rint)
    d0 = row_dot(df, C)
    M = image_range(C, r_max)
    I, J = np.divmod(np.arange(n * n), n)
    out_i, out_j, out_r = [], [], []
    for m0, m1, m2 in itertools.product(*[range(-m, m + 1) for m in M]):
        s = (m0 * C[0] + m1 * C[1]) + m2 * C[2]
        d = d0 + s
        r = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
        keep = np.ones(n * n, dtype=bool) if (m0, m1, m2) != (0, 0, 0) else I != J
        out_i.append(I[keep])
        out_j.append(J[keep])
        out_r.append(r[keep])
    return np.concatenate(out_i), np.concatenate(out_j), np.concatenate(out_r)


def rdf_counts(traj, cells, rank, S, r_max, n_bins):
    """``traj`` [F, n, 3], ``cells`` [3, 3] or [F, 3, 3] -> (counts [P, n_bins] int64 summed over the frames, the smallest distance
    of a pair from a bin edge or from r_max in bin widths, the number of pairs binned).  Asserts its own precondition: no pair lies
    within ``EDGE_MARGIN`` bin widths of an edge, so that the last bits of r cannot move a pair."""
    traj, cells = np.asarray(traj, dtype=np.float64), np.asarray(cells, dtype=np.float64)
    P = 1 + S * (S + 1) // 2
    counts = np.zeros((P, n_bins), dtype=np.int64)
    scale = n_bins / r_max
    margin, pairs = np.inf, 0
    for f in range(len(traj)):
        C = cells if cells.ndim == 2 else cells[f]
        I, J, r = pair_distances(C, traj[f], r_max)
        x = r * scale
        near = x < n_bins + 0.5
        if near.any():
            margin = min(margin, float(np.abs(x[near] - np.round(x[near])).min()))
        keep = r < r_max
        bins = np.floor(x[keep]).astype(np.int64)
        rows = np.array([pair_row(a, b) for a, b in zip(rank[I[keep]], rank[J[keep]])], dtype=np.int64)
        np.add.at(counts, (rows, bins), 1)
        np.add.at(counts, (np.zeros_like(rows), bins), 1)
        pairs += int(keep.sum())
    assert margin > EDGE_MARGIN, f"a pair lies {margin:.3e} bin widths from a bin edge: choose another seed"
    return counts, margin, pairs


def rdf_normalise(counts, cells, n_frames, count, r_max):
    """-> (g [P, n_bins], the running coordination number [P, n_bins], <V>, the bin centres).  ``count`` = ``group_counts``."""
    counts, cells = np.asarray(counts), np.asarray(cells, dtype=np.float64)
    P, n_bins = counts.shape
    V = 0.0
    for f in range(n_frames):  # in frame order
        V = V + abs(det_cof(cells if cells.ndim == 2 else cells[f]))
    V = V / float(n_frames)
    dr = r_max / float(n_bins)
    k = np.arange(n_bins, dtype=np.float64)
    r0, r1 = k * dr, (k + 1.0) * dr
    shell = (4.0 * np.pi / 3.0) * ((r1 * r1) * r1 - (r0 * r0) * r0)
    g, coord = np.zeros((P, n_bins)), np.zeros((P, n_bins))
    F = float(n_frames)
    for p in range(P):
        a, b = row_groups(p)
        Na, Nb, w = float(count[a]), float(count[b]), 2.0 if a < b else 1.0
        if Na > 0 and Nb > 0:
            g[p] = (counts[p].astype(np.float64) * V) / ((((F * Na) * Nb) * w) * shell)
            coord[p] = np.cumsum(counts[p]).astype(np.float64) / ((F * Na) * w)
    return g, coord, V, (k + 0.5) * dr


def com(traj, masses):
    """[F, 3]: (sum_i m_i r_i) / (sum_i m_i), both sums in row order."""
    traj, masses = np.asarray(traj, dtype=np.float64), np.asarray(masses, dtype=np.float64)
    s, mt = np.zeros((traj.shape[0], 3)), 0.0
    for i in range(traj.shape[1]):
        s = s + masses[i] * traj[:, i, :]
        mt = mt + masses[i]
    return s / mt


def n_origins(F, k, stride):
    return (F - 1 - k) // stride + 1


def _true_sum(terms):
    """Sum in extended precision, rounded once: stands for the exact sum of the float64 terms."""
    return float(np.sum(terms.astype(np.longdouble)))


def msd(traj, rank, S, masses, max_lag, stride=1, remove_com=True):
    """-> (msd [S + 1, K + 1, 3], the number of terms of every sum [S + 1, K + 1])."""
    traj = np.asarray(traj, dtype=np.float64)
    F = traj.shape[0]
    c = com(traj, masses) if remove_com else np.zeros((F, 3))
    count = group_counts(rank, S)
    out, terms = np.zeros((S + 1, max_lag + 1, 3)), np.zeros((S + 1, max_lag + 1), dtype=np.int64)
    for k in range(max_lag + 1):
        ts = np.arange(0, F - k, stride)
        d = (traj[ts + k] - traj[ts]) - (c[ts + k] - c[ts])[:, None, :]
        sq = d * d  # [origins, n, 3]
        for g in range(S + 1):
            if count[g] == 0:
                continue
            sel = sq[:, members(rank, g), :]
            terms[g, k] = sel.shape[0] * sel.shape[1]
            for x in range(3):
                out[g, k, x] = _true_sum(sel[:, :, x]) / (float(len(ts)) * float(count[g]))
    return out, terms


def vacf(momenta, rank, S, masses, max_lag, stride=1):
    """-> (vacf [S + 1, K + 1], the same average of |v . v'| [S + 1, K + 1], the number of terms [S + 1, K + 1])."""
    v = np.asarray(momenta, dtype=np.float64) / np.asarray(masses, dtype=np.float64)[None, :, None]
    F = v.shape[0]
    count = group_counts(rank, S)
    out, mag = np.zeros((S + 1, max_lag + 1)), np.zeros((S + 1, max_lag + 1))
    terms = np.zeros((S + 1, max_lag + 1), dtype=np.int64)
    for k in range(max_lag + 1):
        ts = np.arange(0, F - k, stride)
        a, b = v[ts], v[ts + k]
        dot = (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]  # [origins, n]
        for g in range(S + 1):
            if count[g] == 0:
                continue
            sel = dot[:, members(rank, g)]
            terms[g, k] = sel.size
            norm = float(len(ts)) * float(count[g])
            out[g, k], mag[g, k] = _true_sum(sel) / norm, _true_sum(np.abs(sel)) / norm
    return out, mag, terms


def vdos(C, dtau, n_freq, f_max, window="hann"):
    """``C`` [..., K + 1] -> (D [..., n_freq] in fs, the magnitude 2 dtau sum_k |c_k w_k C(k) / C(0)| [...], nu [n_freq] in THz)."""
    C = np.asarray(C, dtype=np.float64)
    K = C.shape[-1] - 1
    k = np.arange(K + 1, dtype=np.float64)
    ck = np.where(k == 0, 0.5, 1.0)
    wk = (1.0 + np.cos(np.pi * k / K)) / 2.0 if (window == "hann" and K > 0) else np.ones(K + 1)
    nu = np.arange(n_freq, dtype=np.float64) * (f_max / float(n_freq - 1))
    omega = (2.0 * np.pi) * (nu * 1e-3)
    C0 = C[..., :1]
    with np.errstate(invalid="ignore", divide="ignore"):
        w = np.where(C0 != 0.0, (ck * wk) * (C / C0), 0.0)  # [..., K + 1]
    cos = np.cos(omega[:, None] * (k * dtau)[None, :])  # [n_freq, K + 1]
    D = np.zeros(C.shape[:-1] + (n_freq,))
    for kk in range(K + 1):  # ascending k
        D = D + w[..., kk:kk + 1] * cos[:, kk]
    return (2.0 * dtau) * D, (2.0 * dtau) * np.abs(w).sum(-1), nu


def fit(msd_, dtau, k_lo, k_hi):
    """``msd_`` [..., K + 1, 3] -> [..., 4, 4]: x, y, z and the total, each (slope, intercept, standard error of the slope, D)."""
    msd_ = np.asarray(msd_, dtype=np.float64)
    y4 = np.concatenate([msd_, ((msd_[..., 0] + msd_[..., 1]) + msd_[..., 2])[..., None]], axis=-1)[..., k_lo:k_hi + 1, :]
    x = np.arange(k_lo, k_hi + 1, dtype=np.float64) * dtau
    npts = float(len(x))
    xm = x.sum() / npts
    ym = y4.sum(-2) / npts  # [..., 4]
    dx = x - xm
    sxx = (dx * dx).sum()
    sxy = (dx[:, None] * (y4 - ym[..., None, :])).sum(-2)
    slope = sxy / sxx
    icpt = ym - slope * xm
    e = y4 - (icpt[..., None, :] + slope[..., None, :] * x[:, None])
    ss = (e * e).sum(-2)
    se = np.sqrt((ss / (npts - 2.0)) / sxx) if npts > 2 else np.zeros_like(slope)
    return np.stack([slope, icpt, se, slope / np.array([2.0, 2.0, 2.0, 6.0])], axis=-1)


def green_kubo(C, dtau, unit=FS):
    """``C`` [..., K + 1] -> the running trapezoid [(I(k) (dtau unit)) unit] / 3, I(0) = 0, I(k) = I(k - 1) + (C(k - 1) + C(k)) / 2."""
    C = np.asarray(C, dtype=np.float64)
    I = np.concatenate([np.zeros(C.shape[:-1] + (1,)), np.cumsum((C[..., :-1] + C[..., 1:]) / 2.0, axis=-1)], axis=-1)
    return ((I * (dtau * unit)) * unit) / 3.0
