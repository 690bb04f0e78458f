"""The numpy restatement of the local structure analysis (alignn_amd/local_order.py, csrc/local_order.hip; include/alignn_local.h
states the rules), one structure at a time and on the frames already selected.  A support module: it holds no tests.

The neighbour shells are those of tests/order_ref.py (``shells``).  What is restated operation for operation, because the
device's integers are compared with it: the bond distances between list entries, the sort of the adaptive rule and its cutoffs.
The harmonics follow the header's recurrence; their sums are numpy's, and the device's fixed-order sums are compared with them
under a measured bound.  Beside its results every function returns the smallest margins of its inputs, the precondition of an
exact comparison (``order_ref.MARGIN``): a pair distance from r_cut, a bond distance from r_c, and for the adaptive rule the gap
between the 12th and 13th and between the 14th and 15th distance, all relative."""

import math
from fractions import Fraction

import numpy as np

from tests import order_ref
from tests.order_ref import MARGIN, MAX_NEIGHBORS, shells  # noqa: F401
from tests.traj_ref import group_counts, groups, members

OTHER, FCC, HCP, BCC, ICO = range(5)
SIGNATURES = ((4, 2, 1), (4, 2, 2), (4, 4, 4), (5, 5, 5), (6, 6, 6))
ADAPTIVE_FACTOR = (1.0 + np.sqrt(2.0)) / 2.0
BCC_FACTOR = 2.0 / np.sqrt(3.0)


# --- common-neighbour analysis -----------------------------------------------------------------------------------------------------
def signatures(d, sel, rc):
    """The entries ``sel`` (indices) of one shell with displacements ``d``: -> ([(n_cn, n_b, n_lcb)] per selected entry, the
    smallest |distance - rc| / rc over the pairs of selected entries)."""
    e = d[sel][:, None, :] - d[sel][None, :, :]
    dist = np.sqrt((e[..., 0] * e[..., 0] + e[..., 1] * e[..., 1]) + e[..., 2] * e[..., 2])
    k = len(sel)
    off = ~np.eye(k, dtype=bool)
    margin = float((np.abs(dist - rc) / rc)[off].min()) if k > 1 else np.inf
    bonded = (dist < rc) & off
    out = []
    for a in range(k):
        common = np.nonzero(bonded[a])[0]
        sub = bonded[np.ix_(common, common)]
        n_lcb, seen = 0, set()
        for start in range(len(common)):
            if start in seen:
                continue
            comp, stack = {start}, [start]
            while stack:
                v = stack.pop()
                for u in np.nonzero(sub[v])[0]:
                    if int(u) not in comp:
                        comp.add(int(u))
                        stack.append(int(u))
            seen |= comp
            at = sorted(comp)
            n_lcb = max(n_lcb, int(sub[np.ix_(at, at)].sum()) // 2)
        out.append((len(common), int(sub.sum()) // 2, n_lcb))
    return out, margin


def classify(sigs, close_packed=True, bcc=True):
    """-> (the class, the counts of ``SIGNATURES``)."""
    count = [sum(1 for s in sigs if s == want) for want in SIGNATURES]
    nb = len(sigs)
    if close_packed and nb == 12:
        if count[0] == 12:
            return FCC, count
        if count[0] == 6 and count[1] == 6:
            return HCP, count
        if count[3] == 12:
            return ICO, count
    if bcc and nb == 14 and count[2] == 6 and count[4] == 8:
        return BCC, count
    return OTHER, count


def cna_atom(d, r, r_cut, adaptive):
    """One atom's list -> (class, signature counts [5], bond margin, gap margin)."""
    nb = len(r)
    if not adaptive:
        sigs, margin = signatures(d, np.arange(nb), r_cut)
        cls, count = classify(sigs)
        return cls, count, margin, np.inf
    order = np.argsort(r, kind="stable")  # (ties by list order)
    rs = r[order]
    gap = min([(rs[k] - rs[k - 1]) / rs[k - 1] for k in (12, 14) if nb > k], default=np.inf)
    bond = np.inf
    if nb >= 12:
        total = 0.0
        for k in range(12):
            total = total + rs[k]
        sigs, margin = signatures(d, order[:12], ADAPTIVE_FACTOR * (total / 12.0))
        bond = min(bond, margin)
        cls, count = classify(sigs, True, False)
        if cls != OTHER:
            return cls, count, bond, gap
    if nb >= 14:
        s8 = s6 = 0.0
        for k in range(8):
            s8 = s8 + rs[k]
        for k in range(8, 14):
            s6 = s6 + rs[k]
        sigs, margin = signatures(d, order[:14], ADAPTIVE_FACTOR * (((BCC_FACTOR * s8) + s6) / 14.0))
        cls, count = classify(sigs, False, True)
        return cls, count, min(bond, margin), gap
    return OTHER, [0] * 5, bond, gap


def cna(traj, cells, rank, S, r_cut, adaptive=False):
    """``traj`` [F, n, 3], ``cells`` [3, 3] or [F, 3, 3] -> a dict: ``structure`` [F, n], ``signature_counts`` [F, n, 5],
    ``n_neighbors`` [F, n], ``counts`` [S + 1, F, 5]; ``cut_margin``, ``bond_margin``, ``gap_margin``; ``max_neighbors``."""
    traj, cells = np.asarray(traj, dtype=np.float64), np.asarray(cells, dtype=np.float64)
    F, n = traj.shape[:2]
    out = dict(structure=np.zeros((F, n), dtype=np.int64), signature_counts=np.zeros((F, n, 5), dtype=np.int64),
               n_neighbors=np.zeros((F, n), dtype=np.int64), counts=np.zeros((S + 1, F, 5), dtype=np.int64), cut_margin=np.inf,
               bond_margin=np.inf, gap_margin=np.inf, max_neighbors=0)
    for f in range(F):
        per_atom, margin = shells(cells if cells.ndim == 2 else cells[f], traj[f], r_cut)
        out["cut_margin"] = min(out["cut_margin"], margin)
        for i, (nj, d, r) in enumerate(per_atom):
            out["n_neighbors"][f, i] = len(r)
            out["max_neighbors"] = max(out["max_neighbors"], len(r))
            if len(r) > MAX_NEIGHBORS:
                continue  # (the device refuses it)
            cls, count, bond, gap = cna_atom(d, r, r_cut, adaptive)
            out["structure"][f, i], out["signature_counts"][f, i] = cls, count
            out["bond_margin"], out["gap_margin"] = min(out["bond_margin"], bond), min(out["gap_margin"], gap)
        for g in range(S + 1):
            out["counts"][g, f] = np.bincount(out["structure"][f, members(rank, g)], minlength=5)
    return out


# --- bond-orientational order --------------------------------------------------------------------------------------------------------
def three_j(l):
    """(l l l; m1 m2 m3) [2l + 1, 2l + 1] by Racah's formula in rationals, one square root at the end."""
    fact = math.factorial
    out = np.zeros((2 * l + 1, 2 * l + 1))
    delta = Fraction(fact(l) ** 3, fact(3 * l + 1))
    for m1 in range(-l, l + 1):
        for m2 in range(-l, l + 1):
            m3 = -(m1 + m2)
            if abs(m3) > l:
                continue
            total = Fraction(0)
            for k in range(max(0, -m1, m2), min(l, l - m1, l + m2) + 1):
                total += Fraction((-1) ** k, fact(k) * fact(l - k) * fact(l - m1 - k) * fact(l + m2 - k) * fact(m1 + k) * fact(k - m2))
            pref = delta * fact(l + m1) * fact(l - m1) * fact(l + m2) * fact(l - m2) * fact(l + m3) * fact(l - m3)
            out[m1 + l, m2 + l] = (-1) ** (m3 % 2) * (1 if total >= 0 else -1) * math.sqrt(float(pref * total * total))
    return out


def ylm(l, d, r):
    """Y_lm of the unit vectors d / r for m = 0 .. l: [Nb, l + 1] complex, by the header's recurrence."""
    x, y, z = d[:, 0] / r, d[:, 1] / r, d[:, 2] / r
    out = np.zeros((len(r), l + 1), dtype=np.complex128)
    e, gmm = np.ones(len(r), dtype=np.complex128), 1.0
    for m in range(l + 1):
        if m > 0:
            e = e * (x + 1j * y)
            gmm = -float(2 * m - 1) * gmm
        gm2, gm1 = 0.0, np.full(len(r), gmm)
        for k in range(m + 1, l + 1):
            g = (float(2 * m + 1) * z) * gm1 if k == m + 1 else ((float(2 * k - 1) * z) * gm1 - float(k + m - 1) * gm2) / float(k - m)
            gm2, gm1 = gm1, g
        norm = math.sqrt(float(Fraction((2 * l + 1) * math.factorial(l - m), math.factorial(l + m))) / (4.0 * math.pi))
        out[:, m] = norm * (gm1 * e)
    return out


def invariants(l, q, table):
    """q [.., l + 1] complex (m >= 0) -> (s, t) [..]."""
    m = np.arange(1, l + 1)
    full = np.concatenate([((-1.0) ** m * np.conj(q[..., 1:]))[..., ::-1], q], axis=-1)  # m = -l .. l
    s = (np.abs(full) ** 2).sum(-1)
    t = np.zeros(q.shape[:-1])
    for m1 in range(-l, l + 1):
        for m2 in range(-l, l + 1):
            m3 = -(m1 + m2)
            if abs(m3) <= l:
                t = t + table[m1 + l, m2 + l] * (full[..., m1 + l] * full[..., m2 + l] * full[..., m3 + l]).real
    return s, t


def q_w(l, s, t):
    """The device's defining formulas: q = sqrt((4 pi / (2l + 1)) s), w = t / (s sqrt(s)), 0 where s is."""
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.sqrt(((4.0 * np.pi) / float(2 * l + 1)) * s), np.where(s > 0.0, t / (s * np.sqrt(s)), 0.0)


def bond_order(traj, cells, rank, S, r_cut, ls):
    """-> a dict: ``s``, ``t``, ``q``, ``w``, ``s_avg``, ``t_avg``, ``q_avg``, ``w_avg`` [F, n, L]; ``n_neighbors`` [F, n];
    ``cut_margin``; ``max_neighbors``."""
    traj, cells = np.asarray(traj, dtype=np.float64), np.asarray(cells, dtype=np.float64)
    F, n = traj.shape[:2]
    L = len(ls)
    out = {k: np.zeros((F, n, L)) for k in ("s", "t", "q", "w", "s_avg", "t_avg", "q_avg", "w_avg")}
    out.update(n_neighbors=np.zeros((F, n), dtype=np.int64), cut_margin=np.inf, max_neighbors=0)
    tables = [three_j(l) for l in ls]
    for f in range(F):
        per_atom, margin = shells(cells if cells.ndim == 2 else cells[f], traj[f], r_cut)
        out["cut_margin"] = min(out["cut_margin"], margin)
        for i, (nj, d, r) in enumerate(per_atom):
            out["n_neighbors"][f, i] = len(r)
        out["max_neighbors"] = max(out["max_neighbors"], int(out["n_neighbors"][f].max()))
        for u, l in enumerate(ls):
            qlm = np.zeros((n, l + 1), dtype=np.complex128)
            for i, (nj, d, r) in enumerate(per_atom):
                if 0 < len(r) <= MAX_NEIGHBORS:
                    qlm[i] = ylm(l, d, r).sum(0) / float(len(r))
            avg = np.zeros_like(qlm)
            for i, (nj, d, r) in enumerate(per_atom):
                if len(r) <= MAX_NEIGHBORS:
                    avg[i] = (qlm[i] + qlm[nj].sum(0)) / float(len(r) + 1)
            for key, q in (("", qlm), ("_avg", avg)):
                s, t = invariants(l, q, tables[u])
                out["s" + key][f, :, u], out["t" + key][f, :, u] = s, t
                out["q" + key][f, :, u], out["w" + key][f, :, u] = q_w(l, s, t)
    return out


# --- the perfect crystals, each in its smallest cell -------------------------------------------------------------------------------
def fcc_cell(a):
    return a * np.eye(3), a * np.array([[0, 0, 0], [0, 0.5, 0.5], [0.5, 0, 0.5], [0.5, 0.5, 0]])


def hcp_cell(a):
    """Two atoms, ideal c / a = sqrt(8 / 3)."""
    C = np.array([[a, 0.0, 0.0], [-0.5 * a, np.sqrt(3.0) / 2.0 * a, 0.0], [0.0, 0.0, np.sqrt(8.0 / 3.0) * a]])
    return C, np.array([[0.0, 0.0, 0.0], [1.0 / 3.0, 2.0 / 3.0, 0.5]]) @ C


def bcc_cell(a):
    return a * np.eye(3), a * np.array([[0, 0, 0], [0.5, 0.5, 0.5]])


def icosahedron(radius, box=12.0):
    """The centre (atom 0) and the 12 vertices at ``radius`` from it, in the middle of a cubic box."""
    g = (1.0 + np.sqrt(5.0)) / 2.0
    v = np.array([[0, s1, s2 * g] for s1 in (1, -1) for s2 in (1, -1)], dtype=np.float64)
    v = np.concatenate([v, v[:, [2, 0, 1]], v[:, [1, 2, 0]]]) * (radius / np.sqrt(1.0 + g * g))
    return box * np.eye(3), np.concatenate([np.zeros((1, 3)), v]) + box / 2.0


def fcc_supercell(a, reps=2):
    C, base = fcc_cell(a)
    shifts = np.array([[i, j, k] for i in range(reps) for j in range(reps) for k in range(reps)], dtype=np.float64) * a
    return reps * C, (shifts[:, None, :] + base[None, :, :]).reshape(-1, 3)


A_FCC, A_HCP, A_BCC, R_ICO = 3.6, 2.9, 3.2, 2.6
# midway between the shells each must separate: fcc and hcp the first and second, bcc the second and third, the icosahedron its
# edge (1.0515 r) and the next distance between two vertices (1.7013 r)
CUT_FCC = (A_FCC / np.sqrt(2.0) + A_FCC) / 2.0
CUT_HCP = (A_HCP + A_HCP * np.sqrt(2.0)) / 2.0
CUT_BCC = (A_BCC + A_BCC * np.sqrt(2.0)) / 2.0
CUT_ICO = R_ICO * (1.0514622242382672 + 1.7013016167040798) / 2.0
CRYSTALS = {"fcc": (fcc_cell(A_FCC), CUT_FCC, FCC), "hcp": (hcp_cell(A_HCP), CUT_HCP, HCP), "bcc": (bcc_cell(A_BCC), CUT_BCC, BCC),
            "ico": (icosahedron(R_ICO), CUT_ICO, ICO)}
# q4, q6, w4, w6 of the perfect first shells (bcc: both shells, 14 neighbours), recomputed with scipy's harmonics and sympy's 3j
CONSTANTS = {"fcc": (0.190941, 0.574524, -0.159317, -0.013161), "hcp": (0.097222, 0.484762, 0.134097, -0.012442),
             "bcc": (0.036370, 0.510688, 0.159317, 0.013161), "ico": (None, 0.663325, None, -0.169754)}

# --- the inputs of the device tests (tests/test_gpu_local.py), here so that tests/test_local_ref.py can assert their margins ---------
# the B = 3 batch of tests/order_ref.py, then the four crystals, then a 32-atom fcc supercell with Gaussian noise
NOISE, NOISE_SEED = 0.094, 3
SCALES = (1.0, 0.92, 1.08)  # of the crystals' cells and positions per frame, in the "moving" kind
SIZES = list(order_ref.SIZES) + [4, 2, 2, 13, 32]
SPECIES = list(order_ref.SPECIES) + [np.array([13] * 4), np.array([22, 22]), np.array([26, 26]), np.array([29] + [13] * 12),
                                     np.array([28, 13, 13, 13] * 8)]
NAMES = ["one", "five", "seventy", "fcc", "hcp", "bcc", "ico", "noisy"]
PTR = np.concatenate([[0], np.cumsum(SIZES)])
RANDOM = (0, 1, 2, 7)  # the structures whose margins are asserted
# "one": 3.3 A lies between the shells of every crystal here; "each": per structure, the crystals' midway cutoffs; "wide": the
# search radius of the adaptive rule (it reaches the 14 nearest of the bcc cell at every scale, and gives no atom more than 64)
R_CUTS = {"one": (3.3,) * 8, "each": (3.3, 2.9, 3.1, CUT_FCC, CUT_HCP, CUT_BCC, CUT_ICO, CUT_FCC), "wide": (4.2,) * 8}
LS = ((4, 6), (4, 6, 12))
_CACHE = {}


def inputs():
    """F = 3 frames: -> (fixed [F, N, 3], moving [F, N, 3], the fixed cells [B, 3, 3], the per-frame cells [F, B, 3, 3]).  The
    first three structures are ``order_ref.inputs()``; the crystals are the same in every fixed frame and scaled by ``SCALES`` in
    the moving ones; the noisy supercell has its own N(0, NOISE A) displacements in every frame."""
    if "inputs" not in _CACHE:
        fixed3, moving3, per_frame3 = order_ref.inputs()
        rng = np.random.default_rng(NOISE_SEED)
        F, B = 3, len(SIZES)
        cells, per_frame = np.zeros((B, 3, 3)), np.zeros((F, B, 3, 3))
        fixed, moving = np.zeros((F, PTR[-1], 3)), np.zeros((F, PTR[-1], 3))
        cells[:3], per_frame[:, :3] = order_ref.CELLS, per_frame3
        fixed[:, :PTR[3]], moving[:, :PTR[3]] = fixed3, moving3
        for b, name in enumerate(NAMES[3:], start=3):
            C, pos = fcc_supercell(A_FCC) if name == "noisy" else CRYSTALS[name][0]
            cells[b] = C
            for f in range(F):
                p = pos + (rng.normal(0.0, NOISE, pos.shape) if name == "noisy" else 0.0)
                per_frame[f, b] = SCALES[f] * C
                fixed[f, PTR[b]:PTR[b + 1]], moving[f, PTR[b]:PTR[b + 1]] = p, SCALES[f] * p
        _CACHE["inputs"] = fixed, moving, cells, per_frame
    return _CACHE["inputs"]


def _per_structure(fn, key, kind, cuts, frames, *extra):
    key = (key, kind, cuts, frames) + extra
    if key not in _CACHE:
        fixed, moving, cells, per_frame = inputs()
        out = []
        for b, n in enumerate(SIZES):
            rank, _ = groups(SPECIES[b], n)
            traj, C = (fixed, cells[b]) if kind == "fixed" else (moving, per_frame[list(frames), b])
            out.append(fn(traj[list(frames), PTR[b]:PTR[b + 1]], C, rank, int(rank.max()), R_CUTS[cuts][b], *extra))
        _CACHE[key] = out
    return _CACHE[key]


def want_cna(kind, cuts, adaptive, frames=(0, 1, 2)):
    """``cna`` per structure of the frames ``frames`` of ``inputs()`` (``kind``: "fixed" / "moving"; ``cuts``: a key of
    ``R_CUTS``), once per case."""
    return _per_structure(cna, "cna", kind, cuts, frames, adaptive)


def want_bond(kind, cuts, ls, frames=(0, 1, 2)):
    return _per_structure(bond_order, "bond", kind, cuts, frames, ls)


def group_means(x, rank, S):
    """x [F, n, L] -> [S + 1, F, L], zeros for a group without members."""
    count = group_counts(rank, S)
    out = np.zeros((S + 1,) + x.shape[:1] + x.shape[2:])
    for g in range(S + 1):
        if count[g] > 0:
            out[g] = x[:, members(rank, g)].sum(1) / float(count[g])
    return out
