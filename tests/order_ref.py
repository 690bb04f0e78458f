"""The numpy restatement of the structural order analysis (alignn_amd/order.py, csrc/order.hip; include/alignn_order.h states the
formulas), one structure at a time and on the frames already selected.  A support module: it holds no tests.

What is restated operation for operation, because the device's integers are compared with it: the pair geometry of the
neighbour shells (that of tests/traj_ref.py), the cosine of every triplet, and the reciprocal vectors with their lengths.  The
sums over triplets, rows, frames and vectors are numpy's: the device's fixed-order sums are compared with them under a measured
bound.  Beside its results every function returns the smallest margins of its inputs, the precondition of an exact comparison
(``MARGIN``): an angle from a bin edge in bin widths, a pair distance from r_cut and a |q| from a shell edge or from q_max,
relatively."""

import itertools

import numpy as np

from tests.defects_ref import inv3_cof, row_dot
from tests.traj_ref import group_counts, groups, image_range, members, pair_row, row_groups  # noqa: F401

MARGIN = 1e-9
MAX_NEIGHBORS, MAX_HKL = 64, 32


def shells(C, pos, r_cut):
    """The neighbours of every atom of one frame: -> ([(j [Nb], d [Nb, 3], r [Nb])] per atom, in the order j ascending, then
    (m0, m1, m2) lexicographic; the smallest |r - r_cut| / r_cut over every candidate)."""
    C, pos = np.asarray(C, dtype=np.float64), np.asarray(pos, dtype=np.float64)
    n = len(pos)
    dp = (pos[None, :, :] - pos[:, None, :]).reshape(-1, 3)  # [i, j] = r_j - r_i
    df = row_dot(dp, inv3_cof(C))
    df = df - np.round(df)  # (half to even, as rint)
    d0 = row_dot(df, C)
    shifts = list(itertools.product(*[range(-m, m + 1) for m in image_range(C, r_cut)]))
    D = np.stack([d0 + ((m0 * C[0] + m1 * C[1]) + m2 * C[2]) for m0, m1, m2 in shifts], axis=1)  # [n n, images, 3]
    r = np.sqrt((D[..., 0] * D[..., 0] + D[..., 1] * D[..., 1]) + D[..., 2] * D[..., 2])
    own = (np.arange(n)[:, None] == np.arange(n)[None, :]).reshape(-1, 1) & np.array([s == (0, 0, 0) for s in shifts])[None, :]
    margin = float((np.abs(r - r_cut) / r_cut)[~own].min())
    keep = (~own & (r < r_cut)).reshape(n, -1)
    D, r = D.reshape(n, -1, 3), r.reshape(n, -1)
    out = []
    for i in range(n):
        at = np.nonzero(keep[i])[0]
        out.append((at // len(shifts), D[i, at], r[i, at]))
    return out, margin


def cosines(d, r):
    """The unordered pairs j < k of one shell: -> (j, k, c = ((dxj dxk + dyj dyk) + dzj dzk) / (rj rk) clamped to [-1, 1])."""
    j, k = np.triu_indices(len(r), 1)
    c = ((d[j, 0] * d[k, 0] + d[j, 1] * d[k, 1]) + d[j, 2] * d[k, 2]) / (r[j] * r[k])
    return j, k, np.clip(c, -1.0, 1.0)


def legendre(l, c):
    """P_l(c) by P_{n+1} = (((2n + 1) c) P_n - n P_{n-1}) / (n + 1)."""
    pm, pn = np.ones_like(c), c
    for n in range(1, l):
        pm, pn = pn, ((float(2 * n + 1) * c) * pn - float(n) * pm) / float(n + 1)
    return pn


def q_l(ls, c, nb):
    """sqrt(max(0, (Nb + 2 sum_{j<k} P_l(c_jk)) / Nb^2)) per l; Nb = 0 gives 0."""
    if nb == 0:
        return np.zeros(len(ls))
    return np.array([np.sqrt(max(0.0, (float(nb) + 2.0 * float(legendre(l, c).sum())) / (float(nb) * float(nb)))) for l in ls])


def angles(traj, cells, rank, S, r_cut, n_bins=None, ls=None):
    """``traj`` [F, n, 3], ``cells`` [3, 3] or [F, 3, 3] -> a dict: ``counts`` [S + 1, P, n_bins] int64 with the marginal rows
    (``n_bins`` given); ``q`` [F, n, L], ``n_neighbors`` [F, n], ``mean`` [S + 1, F, L] (``ls`` given); ``max_neighbors``;
    ``triplets``; ``angle_margin`` (bin widths, to an inner bin edge) and ``cut_margin`` (relative)."""
    traj, cells = np.asarray(traj, dtype=np.float64), np.asarray(cells, dtype=np.float64)
    F, n = traj.shape[:2]
    P = 1 + S * (S + 1) // 2
    out = dict(max_neighbors=0, triplets=0, angle_margin=np.inf, cut_margin=np.inf)
    if n_bins is not None:
        out["counts"] = np.zeros((S + 1, P, n_bins), dtype=np.int64)
        scale = float(n_bins) / np.pi
    if ls is not None:
        out["q"], out["n_neighbors"] = np.zeros((F, n, len(ls))), np.zeros((F, n), dtype=np.int64)
    for f in range(F):
        per_atom, margin = shells(cells if cells.ndim == 2 else cells[f], traj[f], r_cut)
        out["cut_margin"] = min(out["cut_margin"], margin)
        for i, (nj, d, r) in enumerate(per_atom):
            out["max_neighbors"] = max(out["max_neighbors"], len(r))
            if len(r) > MAX_NEIGHBORS:
                continue  # (the device refuses it)
            j, k, c = cosines(d, r)
            out["triplets"] += len(c)
            if ls is not None:
                out["q"][f, i], out["n_neighbors"][f, i] = q_l(ls, c, len(r)), len(r)
            if n_bins is not None and len(c):
                x = np.arccos(c) * scale
                inner = (x > 0.5) & (x < n_bins - 0.5)  # (the edges 0 and n_bins move nothing: the bin is clamped)
                if inner.any():
                    out["angle_margin"] = min(out["angle_margin"], float(np.abs(x[inner] - np.round(x[inner])).min()))
                bins = np.minimum(np.floor(x).astype(np.int64), n_bins - 1)
                rows = np.array([pair_row(a, b) for a, b in zip(rank[nj[j]], rank[nj[k]])], dtype=np.int64)
                np.add.at(out["counts"], (np.full_like(rows, rank[i]), rows, bins), 1)
    if n_bins is not None:
        out["counts"][1:, 0] = out["counts"][1:, 1:].sum(1)
        out["counts"][0] = out["counts"][1:].sum(0)
    if ls is not None:
        count = group_counts(rank, S)
        out["mean"] = np.zeros((S + 1, F, len(ls)))
        for g in range(S + 1):
            if count[g] > 0:
                out["mean"][g] = out["q"][:, members(rank, g)].sum(1) / float(count[g])
    return out


def adf_normalise(counts):
    """-> (adf: counts / (the row's total x the bin width in degrees), zeros for an empty row; theta: the bin centres in degrees)."""
    counts = np.asarray(counts)
    n_bins = counts.shape[-1]
    w = 180.0 / float(n_bins)
    total = counts.sum(-1, keepdims=True).astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        adf = np.where(total > 0, counts.astype(np.float64) / (total * w), 0.0)
    return adf, (np.arange(n_bins, dtype=np.float64) + 0.5) * w


def hkl_range(C, q_max):
    """H_k = floor((q_max |C_k|) / (2 pi))."""
    C = np.asarray(C, dtype=np.float64)
    return [int(np.floor((q_max * np.sqrt((C[k, 0] * C[k, 0] + C[k, 1] * C[k, 1]) + C[k, 2] * C[k, 2])) / (2.0 * np.pi))) for k in range(3)]


def sq_vectors(C, q_max, n_bins):
    """The half space of reciprocal vectors inside q_max in lexicographic order: -> (hkl [V, 3], |q| [V], their shells [V], the
    smallest relative distance of a candidate's |q| from a shell edge or from q_max)."""
    Ci = inv3_cof(C)
    H = hkl_range(C, q_max)
    h = np.array(list(itertools.product(range(0, H[0] + 1), range(-H[1], H[1] + 1), range(-H[2], H[2] + 1))), dtype=np.int64)
    half = (h[:, 0] > 0) | ((h[:, 0] == 0) & ((h[:, 1] > 0) | ((h[:, 1] == 0) & (h[:, 2] > 0))))
    h = h[half]
    x = h.astype(np.float64)
    q = [(2.0 * np.pi) * ((x[:, 0] * Ci[c, 0] + x[:, 1] * Ci[c, 1]) + x[:, 2] * Ci[c, 2]) for c in range(3)]
    qn = np.sqrt((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2])
    xs = qn * (float(n_bins) / q_max)
    near = xs < n_bins + 0.5
    margin = float((np.abs(xs[near] - np.round(xs[near])) / xs[near]).min()) if near.any() else np.inf
    keep = qn < q_max
    return h[keep], qn[keep], np.minimum(np.floor(xs[keep]).astype(np.int64), n_bins - 1), margin


def phases(traj, C, hkl):
    """exp(2 pi i h . f) [F, n, V], f = r Cinv - floor(r Cinv), as the product (e_0(h0) e_1(h1)) e_2(h2) of the factors
    e_k(h) = exp(i pi x), x = 2 (h f_k) reduced to (-2, 2) exactly."""
    traj = np.asarray(traj, dtype=np.float64)
    F, n = traj.shape[:2]
    fr = row_dot(traj.reshape(-1, 3), inv3_cof(C))
    fr = (fr - np.floor(fr)).reshape(F, n, 3)
    e = []
    for k in range(3):
        x = np.fmod(2.0 * (hkl[None, None, :, k].astype(np.float64) * fr[:, :, None, k]), 2.0)
        e.append(np.cos(np.pi * x) + 1j * np.sin(np.pi * x))
    return (e[0] * e[1]) * e[2]


def structure_factor(traj, C, rank, S, q_max, n_bins):
    """-> a dict: ``hkl`` [V, 3], ``s_vectors`` [P, V], ``s`` [P, n_bins], ``n_vectors`` [n_bins], ``q`` [n_bins], ``margin``."""
    C = np.asarray(C, dtype=np.float64)
    hkl, qn, bins, margin = sq_vectors(C, q_max, n_bins)
    F, P, V = len(traj), 1 + S * (S + 1) // 2, len(hkl)
    count = group_counts(rank, S)
    s_vec = np.zeros((P, V))
    if V and F:
        ph = phases(traj, C, hkl)
        rho = [None] + [ph[:, rank == g].sum(1) for g in range(1, S + 1)]  # [F, V] each
        rho[0] = sum(rho[2:], rho[1])
        for p in range(P):
            a, b = row_groups(p)
            if count[a] > 0 and count[b] > 0:
                s_vec[p] = (rho[a] * np.conj(rho[b])).real.sum(0) / (float(F) * np.sqrt(float(count[a]) * float(count[b])))
    n_vectors = np.bincount(bins, minlength=n_bins).astype(np.int64)
    s = np.zeros((P, n_bins))
    for p in range(P):
        tot = np.bincount(bins, weights=s_vec[p], minlength=n_bins)
        s[p] = np.where(n_vectors > 0, tot / np.maximum(n_vectors, 1), 0.0)
    return dict(hkl=hkl, s_vectors=s_vec, s=s, n_vectors=n_vectors, q=(np.arange(n_bins) + 0.5) * (q_max / float(n_bins)),
                margin=margin)


# --- the inputs of the device tests (tests/test_gpu_order.py), here so that tests/test_order_ref.py can assert their margins ------------
SIZES = [1, 5, 70]
SPECIES = [np.array([14]), np.array([8, 3, 8, 3, 3]), np.array([22, 8, 38] * 23 + [8])]
CELLS = np.array([[[3.15, 0.0, 0.0], [0.4, 3.15, 0.0], [0.3, -0.35, 3.2]],
                  [[4.0, 0.0, 0.0], [1.3, 3.8, 0.0], [0.7, -0.9, 4.4]],
                  [[13.0, 0.0, 0.0], [0.6, 13.5, 0.0], [-0.4, 0.5, 14.0]]])  # (those of tests/test_gpu_trajectory.py)
PTR = np.concatenate([[0], np.cumsum(SIZES)])
R_CUTS = {"one": (3.3, 3.3, 3.3), "each": (3.3, 2.9, 3.1)}
ADF_BINS = (67, 1024)
LS = ((4, 6), (1, 6, 12))
Q_MAX = 6.0
SQ_BINS = 50
SEED = 11
LONG_FRAMES, LONG_SEED = 130, 12
_CACHE = {}


def inputs():
    """F = 3 frames of random fractional positions, moved by whole cells (-2 .. 2 per axis) and by N(0, 0.05 A) noise, in the
    fixed cells and in per-frame cells that differ from them by a few percent: -> (fixed [F, N, 3], moving [F, N, 3], the
    per-frame cells [F, B, 3, 3])."""
    if "inputs" not in _CACHE:
        rng = np.random.default_rng(SEED)
        F = 3
        grow = np.array([1.0, 1.03, 0.97])
        shear = rng.normal(0.0, 0.01, (F, 3, 3, 3))
        per_frame = np.stack([[grow[f] * (CELLS[b] + shear[f, b] * (f > 0)) for b in range(3)] for f in range(F)])
        fixed, moving = np.zeros((F, PTR[-1], 3)), np.zeros((F, PTR[-1], 3))
        for b, n in enumerate(SIZES):
            for f in range(F):
                frac = rng.uniform(0, 1, (n, 3)) + rng.integers(-2, 3, (n, 3))
                noise = rng.normal(0.0, 0.05, (n, 3))
                fixed[f, PTR[b]:PTR[b + 1]] = frac @ CELLS[b] + noise
                moving[f, PTR[b]:PTR[b + 1]] = frac @ per_frame[f, b] + noise
        _CACHE["inputs"] = fixed, moving, per_frame
    return _CACHE["inputs"]


def long_inputs():
    """LONG_FRAMES frames of the 5-atom structure (two full chunks of the frame sum of S(q) and a part): [F, 5, 3]."""
    if "long" not in _CACHE:
        rng = np.random.default_rng(LONG_SEED)
        _CACHE["long"] = (rng.uniform(0, 1, (LONG_FRAMES, 5, 3)) + rng.integers(-2, 3, (LONG_FRAMES, 5, 3))) @ CELLS[1]
    return _CACHE["long"]


def want_angles(kind, cuts, n_bins=None, ls=None, frames=(0, 1, 2)):
    """``angles`` per structure of the frames ``frames`` of ``inputs()`` (``kind``: "fixed" / "moving"; ``cuts``: a key of
    ``R_CUTS``), once per case."""
    key = ("angles", kind, cuts, n_bins, ls, frames)
    if key not in _CACHE:
        fixed, moving, per_frame = inputs()
        out = []
        for b, n in enumerate(SIZES):
            rank, _ = groups(SPECIES[b], n)
            traj, cells = (fixed, CELLS[b]) if kind == "fixed" else (moving, per_frame[list(frames), b])
            out.append(angles(traj[list(frames), PTR[b]:PTR[b + 1]], cells, rank, int(rank.max()), R_CUTS[cuts][b], n_bins, ls))
        _CACHE[key] = out
    return _CACHE[key]


def want_sq(which="batch"):
    """``structure_factor`` per structure of ``inputs()`` in the fixed cells ("batch"), or of ``long_inputs()`` ("long")."""
    key = ("sq", which)
    if key not in _CACHE:
        if which == "long":
            rank, _ = groups(SPECIES[1], 5)
            _CACHE[key] = [structure_factor(long_inputs(), CELLS[1], rank, int(rank.max()), Q_MAX, SQ_BINS)]
        else:
            out = []
            for b, n in enumerate(SIZES):
                rank, _ = groups(SPECIES[b], n)
                out.append(structure_factor(inputs()[0][:, PTR[b]:PTR[b + 1]], CELLS[b], rank, int(rank.max()), Q_MAX, SQ_BINS))
            _CACHE[key] = out
    return _CACHE[key]
