"""Edge-set goldens for the neighbour-list builders on HARD geometries, written by the REFERENCE's own
``nearest_neighbor_edges`` + ``build_undirected_edgedata`` (alignn/graphs.py:128-264) and ``radius_graph`` (:267-364),
imported unmodified on ``oracle/shims`` (jarvis' ``Atoms`` is the shim's minimal restatement, see its header).

    python oracle/make_golden_graphs_hard.py          (authoring container only: needs /root/reference)

The structures are this project's own, spelled out below or drawn from a fixed seed: lopsided cells (needle, plate, slab,
60-degree shear, a hand-strained cell as cell relaxation leaves it, a left-handed lattice), exact ties (sc / bcc / fcc /
hcp-like with representable coordinates, fractions exactly 0.0 and 1.0, a phonon supercell with one displaced atom), atom
counts around the kernels' loop boundaries (1, 2, 63, 64, 65, 200), more than a thousand candidates per site (60 atoms at
cutoff 16), other ``max_neighbors``, UNWRAPPED fractional coordinates and pairs closer than jarvis' ``bond_tol``.

-> tests/golden/graphs_hard_cases.npz: per case the lattice, fractional coordinates, ``cutoff``, ``max_neighbors`` and the
reference's kNN (u, v, image, r) in its own (dict-insertion) order; for the cases marked R also the reference's
``radius_graph`` lists at cutoff 4.0 in the reference's order.  Only arrays and case names.  Test infrastructure only.

Random cases are redrawn (seed + 1000) until the reference's k-th-shell decision of every site is not a near-tie: the
gap between the k-th kept distance and the first dropped one is > 1e-9 relative.  The exact-tie cases carry the tie coverage.
"""

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(HERE, "shims"))
sys.path.insert(0, "/root/reference")

from jarvis.core.atoms import Atoms  # noqa: E402  (shim)
from alignn.graphs import build_undirected_edgedata, nearest_neighbor_edges, radius_graph  # noqa: E402  (the reference)

RADIUS_CUTOFF = 4.0


def spread(rng, n, lat, dmin, lo=0.0, hi=1.0):
    """n fractional positions uniform in [lo, hi)^3, no two periodic images closer than dmin (rejection sampling)"""
    shifts = np.array([[i, j, k] for i in (-1, 0, 1) for j in (-1, 0, 1) for k in (-1, 0, 1)], dtype=np.float64)
    pts = []
    while len(pts) < n:
        f = rng.uniform(lo, hi, 3)
        w = f - np.floor(f)
        ok = True
        for p in pts:
            d = ((p - np.floor(p)) - w)[None, :] + shifts
            if np.min(np.linalg.norm(d @ lat, axis=1)) < dmin:
                ok = False
                break
        if ok:
            pts.append(f)
    return np.array(pts)


def jittered_grid(rng, m, n, amp):
    """n of the m^3 sites of a regular grid, each moved by up to amp grid spacings (a dense but well separated cell)"""
    g = np.stack(np.meshgrid(*[np.arange(m)] * 3, indexing="ij"), -1).reshape(-1, 3)
    g = g[rng.permutation(len(g))[:n]]
    return (g + 0.5 + rng.uniform(-amp, amp, g.shape)) / m


def fixed_cases():
    s3 = np.sqrt(3.0)
    rhomb = 4.0 * np.array([[1.0, 0.0, 0.0], [0.5, s3 / 2, 0.0], [0.5, s3 / 6, np.sqrt(2.0 / 3.0)]])  # 60 degrees between all axes
    cubic8 = np.array([[0, 0, 0], [.5, .5, 0], [.5, 0, .5], [0, .5, .5], [.25, .25, .25], [.75, .75, .25], [.75, .25, .75], [.25, .75, .75]])
    strain = np.array([[0.22, 0.18, -0.12], [0.18, -0.15, 0.25], [-0.12, 0.25, 0.10]])  # large symmetric strain, by hand
    two = np.array([[0.0, 0.0, 0.0], [0.5, 0.5, 0.5]])
    sup = np.array([[(i + b[0]) / 3.0, (j + b[1]) / 3.0, (k + b[2]) / 3.0] for i in range(3) for j in range(3) for k in range(3) for b in two])
    sup[7, 0] += 0.01 / 9.0  # one atom moved by 0.01 A along a (the phonon displacement)
    fcc = np.array([[0, 0, 0], [.5, .5, 0], [.5, 0, .5], [0, .5, .5]])
    return [
        # --- shape of the cell (R)
        ("needle_1atom", np.diag([2.6, 2.9, 21.0]), np.array([[0.25, 0.5, 0.75]]), 8.0, 12, True),
        ("plate_1atom_c16", np.diag([6.2, 6.4, 2.2]), np.array([[0.1, 0.2, 0.3]]), 16.0, 12, False),  # 7 x 7 x 17 = 833 images
        ("plate_2atoms_c16", np.diag([6.2, 6.4, 2.2]), np.array([[0.1, 0.2, 0.3], [0.6, 0.7, 0.4]]), 16.0, 12, False),
        ("sheared_60deg", rhomb, np.array([[0.1, 0.15, 0.2], [0.55, 0.4, 0.7], [0.8, 0.85, 0.35]]), 8.0, 12, True),
        ("slab_45A_vacuum", np.diag([3.1, 3.3, 48.0]), np.array([[0.0, 0.0, 0.02], [0.5, 0.5, 0.06]]), 8.0, 12, True),
        ("left_handed", np.array([[0.0, 4.1, 0.3], [3.9, 0.0, -0.2], [0.4, 0.1, 5.2]]),
         np.array([[0.05, 0.1, 0.1], [0.5, 0.6, 0.4], [0.3, 0.9, 0.8], [0.8, 0.3, 0.6]]), 8.0, 12, True),
        ("strained_after_cell_relax", (5.4 * np.eye(3)) @ (np.eye(3) + strain), cubic8, 8.0, 12, True),
        # a dimer in a 40 A box: 1 neighbour at cutoff 8, 11 at the longest lattice vector (41), so it widens TWICE
        ("dimer_40A_box", np.diag([40.0, 40.5, 41.0]), np.array([[0.49, 0.49, 0.49], [0.51, 0.5146875, 0.511953125]]), 8.0, 12, True),
        # --- exact ties (R): every number representable
        ("sc", 2.5 * np.eye(3), np.zeros((1, 3)), 8.0, 12, True),
        ("bcc", 3.0 * np.eye(3), two, 8.0, 12, True),
        ("fcc", 4.0 * np.eye(3), fcc, 8.0, 12, True),
        ("hcp_like", np.array([[3.0, 0.0, 0.0], [1.5, 2.5, 0.0], [0.0, 0.0, 5.0]]), np.array([[0.0, 0.0, 0.0], [0.5, 0.25, 0.5]]), 8.0, 12, True),
        ("frac_exactly_0_and_1", 4.5 * np.eye(3), np.array([[0.0, 0.0, 0.0], [1.0, 0.5, 0.5], [0.5, 1.0, 0.0], [0.5, 0.5, 1.0]]), 8.0, 12, True),
        ("phonon_3x3x3_displaced", 9.0 * np.eye(3), sup, 8.0, 12, True),
        # --- other k
        ("fcc_k4", 4.0 * np.eye(3), fcc, 8.0, 4, False),
        ("strained_k20", (5.4 * np.eye(3)) @ (np.eye(3) + strain), cubic8, 8.0, 20, False),
    ]


def random_case(name, seed):
    rng = np.random.default_rng(seed)

    def cell(a, skew=0.3):
        return np.diag(a * (1 + 0.08 * rng.random(3))) + skew * rng.standard_normal((3, 3))

    if name == "cluster_40A_box":  # (R) widens once, to the longest lattice vector
        lat = cell(40.0, 0.5)
        return lat, 0.5 + (rng.uniform(-1.6, 1.6, (5, 3)) @ np.linalg.inv(lat)), 8.0, 12, True
    if name in ("atoms_63", "atoms_64", "atoms_65"):
        return cell(9.0, 0.2), jittered_grid(rng, 5, int(name[-2:]), 0.2), 8.0, 12, False
    if name == "atoms_200":  # the MD size
        return cell(13.6, 0.2), jittered_grid(rng, 6, 200, 0.2), 8.0, 12, False
    if name in ("many_candidates_c16", "many_candidates_mixed"):  # 60 atoms: > 1024 candidates inside cutoff 16
        lat = cell(9.2, 0.2)
        return lat, spread(rng, 60, lat, 1.6), (16.0 if name.endswith("c16") else MIXED_CUTOFF), 12, False
    if name == "unwrapped_m03_p13":  # (R) a drifted frame
        lat = cell(5.6)
        return lat, spread(rng, 8, lat, 1.4, -0.3, 1.3), 8.0, 12, True
    if name == "unwrapped_m2_p3":  # (R)
        lat = cell(6.0)
        return lat, spread(rng, 10, lat, 1.4, -2.0, 3.0), 8.0, 12, True
    if name == "translated_rigidly":  # (R) a perovskite-like cell moved by (1.37, -2.2, 0.5) lattice vectors
        lat = cell(3.95, 0.05)
        f = np.array([[0, 0, 0], [.5, .5, .5], [.5, .5, 0], [.5, 0, .5], [0, .5, .5]]) + 0.02 * rng.standard_normal((5, 3))
        return lat, f - np.floor(f) + np.array([1.37, -2.2, 0.5]), 8.0, 12, True
    if name in ("close_pair_0p06", "close_pair_0p2"):  # (R) below / above jarvis' bond_tol = 0.15
        lat = cell(6.0, 0.1)
        f = spread(rng, 5, lat, 1.8)
        dirn = rng.standard_normal(3)
        dirn /= np.linalg.norm(dirn)
        f[4] = f[3] + ((0.06 if name.endswith("0p06") else 0.2) * dirn) @ np.linalg.inv(lat)
        f = f - np.floor(f)
        return lat, f, 8.0, 12, True
    if name == "unwrapped_k20":
        lat = cell(5.6)
        return lat, spread(rng, 6, lat, 1.4, -1.0, 2.0), 8.0, 20, False
    raise KeyError(name)


MIXED_CUTOFF = 15.13  # 60 atoms: some sites above, some at or below 1024 candidates (checked below and in the test)
RANDOM = ["cluster_40A_box", "atoms_63", "atoms_64", "atoms_65", "atoms_200", "many_candidates_c16", "many_candidates_mixed",
          "unwrapped_m03_p13", "unwrapped_m2_p3", "translated_rigidly", "close_pair_0p06", "close_pair_0p2", "unwrapped_k20"]


def shell_gap(atoms, cutoff, k):
    """smallest relative gap, over the sites, between the k-th kept distance and the first dropped one, at the cutoff the
    reference ends on (its widening rule applied to the shim's neighbour list)"""
    while True:
        nb = atoms.get_all_neighbors(r=cutoff)
        if min(len(x) for x in nb) >= k:
            break
        longest = max(atoms.lattice.abc)
        cutoff = longest if cutoff < longest else 2 * cutoff
    gap = np.inf
    for site in nb:
        d = np.sort(np.array([x[2] for x in site]))
        beyond = d[d > d[k - 1]]
        if len(beyond):
            gap = min(gap, float((beyond[0] - d[k - 1]) / d[k - 1]))
    return gap, [len(x) for x in nb]


if __name__ == "__main__":
    cases = fixed_cases()
    for j, name in enumerate(RANDOM):
        seed = 100 + j
        while True:
            lat, frac, cutoff, k, rad = random_case(name, seed)
            gap, _ = shell_gap(Atoms(lattice_mat=lat, coords=frac, elements=["Si"] * len(frac)), cutoff, k)
            if gap > 1e-9:
                break
            print(name, "seed", seed, "near-tie", gap, "-> redrawn")
            seed += 1000
        cases.append((name, lat, frac, cutoff, k, rad))
    out, names = {}, []
    for i, (name, lat, frac, cutoff, k, rad) in enumerate(cases):
        atoms = Atoms(lattice_mat=lat, coords=frac, elements=["Si"] * len(frac))
        edges, _ = nearest_neighbor_edges(atoms=atoms, cutoff=cutoff, max_neighbors=k, use_canonize=True)
        u, v, r, images = build_undirected_edgedata(atoms, edges)
        names.append(name)
        out[f"{i}.lat"] = atoms.lattice_mat
        out[f"{i}.frac"] = atoms.frac_coords
        out[f"{i}.cutoff"] = np.float64(cutoff)
        out[f"{i}.k"] = np.int64(k)
        out[f"{i}.u"] = u.numpy().astype(np.int32)
        out[f"{i}.v"] = v.numpy().astype(np.int32)
        assert np.abs(images.numpy()).max() < 127
        out[f"{i}.image"] = np.rint(images.numpy()).astype(np.int8)
        out[f"{i}.r"] = r.numpy().astype(np.float32)
        n_rad = None
        if rad:
            ru, rv, rr, rimg = radius_graph(atoms, cutoff=RADIUS_CUTOFF)
            out[f"{i}.rad.u"], out[f"{i}.rad.v"] = ru.numpy().astype(np.int16), rv.numpy().astype(np.int16)
            out[f"{i}.rad.image"] = np.rint(rimg.numpy()).astype(np.int8)
            out[f"{i}.rad.r"] = rr.numpy().astype(np.float32)
            n_rad = len(ru)
        if name.startswith("many_candidates"):
            _, cnt = shell_gap(atoms, cutoff, k)
            print("   candidates per site: min", min(cnt), "max", max(cnt))
            assert min(cnt) > 1024 if name.endswith("c16") else (min(cnt) <= 1024 < max(cnt))
        print(name, "atoms", atoms.num_atoms, "cutoff", cutoff, "k", k, "edges", len(u), "radius edges", n_rad)
    out["names"] = np.array(names)
    out["radius"] = np.array([c[5] for c in cases])
    np.savez_compressed(os.path.join(ROOT, "tests", "golden", "graphs_hard_cases.npz"), **out)
    print(len(names), "cases")
