"""An analytic periodic potential for the relax and MD restatements (tests/relax_ref.py, tests/md_nose_hoover_ref.py) and
their tests: harmonic springs over a fixed list of periodic images, at rest in a target structure.  float64 numpy only."""

import itertools

import numpy as np


# --- an analytic periodic potential: harmonic springs over a fixed image list, at rest in a target structure ----------------
def spring_list(lat, frac, nnb=8):
    """Each atom tied to its ``nnb`` nearest neighbours (images within one cell) of the target (lat, frac), rest length the
    target distance.  -> (i, j, image [m, 3], d0, k)."""
    lat, frac = np.asarray(lat, dtype=np.float64), np.asarray(frac, dtype=np.float64)
    pos = frac @ lat
    n = len(pos)
    rows = []
    for i in range(n):
        cand = []
        for j in range(n):
            for img in itertools.product((-1, 0, 1), repeat=3):
                if i == j and img == (0, 0, 0):
                    continue
                d = pos[j] + np.array(img) @ lat - pos[i]
                cand.append((float(np.linalg.norm(d)), j, img))
        cand.sort(key=lambda t: t[0])
        rows += [(i, j, img, d0) for d0, j, img in cand[:nnb]]
    I = np.array([r[0] for r in rows])
    J = np.array([r[1] for r in rows])
    img = np.array([r[2] for r in rows], dtype=np.float64)
    d0 = np.array([r[3] for r in rows])
    k = 1.0 + 0.5 * (np.arange(len(rows)) % 3)
    return I, J, img, d0, k


def springs_efs(I, J, img, d0, k):
    """-> efs(C, pos) = (E, forces, stress = (1/V) dE/d strain): ASE's sign (positive under tension)."""

    def efs(C, pos):
        d = pos[J] - pos[I] + img @ C
        r = np.sqrt((d * d).sum(1))
        dphi = k * (r - d0)
        fv = (dphi / r)[:, None] * d  # dE / dd
        f = np.zeros_like(pos)
        np.add.at(f, I, fv)
        np.add.at(f, J, -fv)
        s = fv.T @ d / abs(np.linalg.det(C))
        return 0.5 * float((k * (r - d0) ** 2).sum()), f, s

    return efs


def simple_cubic(a0, k=2.0):
    """One atom, springs of rest length a0 (faces) and a0 sqrt(2) (edges) to its periodic images."""
    imgs = [v for v in itertools.product((-1, 0, 1), repeat=3) if 0 < sum(abs(x) for x in v) <= 2]
    img = np.array(imgs, dtype=np.float64)
    d0 = a0 * np.sqrt((img ** 2).sum(1))
    z = np.zeros(len(imgs), dtype=int)
    return springs_efs(z, z, img, d0, np.full(len(imgs), k))
