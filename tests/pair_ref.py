"""A pair potential defined for any periodic structure, for the tests of ``alignn_amd.defects`` (the spring crystals of
tests/springs_ref.py have a fixed bond list and cannot lose an atom or gain a surface):

    phi(r) = D [(1 - exp(-alpha (r - r0)))^2 - 1] (1 - (r / rc)^2)^2   for r < rc, else 0

a Morse well times a cutoff that takes value and slope to zero at rc, summed over all periodic images within rc (an atom's own
images included).  ``efs`` is the float64 numpy statement with analytic forces and stress; ``forces_fn`` the same sums on the
device in a fixed order (dense [n, n, images] tensors reduced by ``sum`` over fixed axes, one structure at a time: no atomics,
the same bits for a structure whatever else is evaluated beside it)."""

import itertools

import numpy as np

D, ALPHA, R0 = 0.4, 1.6, 2.9


def phi(r, rc):
    """-> (phi, d phi / d r), zero from rc on; numpy arrays or torch tensors."""
    if isinstance(r, (np.ndarray, float, int)):
        xp, r = np, np.asarray(r, dtype=np.float64)
    else:
        import torch as xp
    ex = xp.exp(-ALPHA * (r - R0))
    morse, dmorse = D * ((1.0 - ex) ** 2 - 1.0), 2.0 * D * ALPHA * (1.0 - ex) * ex
    u = 1.0 - (r / rc) ** 2
    cut, dcut = u * u, -4.0 * u * r / rc ** 2
    inside = r < rc
    return xp.where(inside, morse * cut, 0.0 * r), xp.where(inside, dmorse * cut + morse * dcut, 0.0 * r)


def image_range(C, rc):
    """Per axis the largest |m| an image within rc of a minimum-image pair can have: floor(rc / height + 1/2)."""
    C = np.asarray(C, dtype=np.float64)
    vol = abs(np.linalg.det(C))
    heights = [vol / np.linalg.norm(np.cross(C[(k + 1) % 3], C[(k + 2) % 3])) for k in range(3)]
    return [int(np.floor(rc / h + 0.5)) for h in heights]


def images(C, rc):
    M = image_range(C, rc)
    return np.array(list(itertools.product(*[range(-m, m + 1) for m in M])), dtype=np.float64)


def pairs(C, pos, rc):
    """Every ordered pair (i, j, image) within rc: -> (i, j, d [m, 3] = r_j + image - r_i, r [m])."""
    C, pos = np.asarray(C, dtype=np.float64), np.asarray(pos, dtype=np.float64)
    n = len(pos)
    df = (pos[None, :, :] - pos[:, None, :]) @ np.linalg.inv(C)
    df = df - np.round(df)
    img = images(C, rc)
    d = (df[:, :, None, :] + img[None, None, :, :]) @ C  # [n, n, images, 3]
    r = np.sqrt((d * d).sum(-1))
    own = (np.eye(n)[:, :, None] > 0) & ((img == 0).all(1))[None, None, :]
    I, J, K = np.nonzero((r < rc) & ~own)
    return I, J, d[I, J, K], r[I, J, K]


def make_efs(rc):
    """-> efs(C, pos) = (E, forces [n, 3], stress [3, 3] = (1 / V) dE / d strain, ASE's sign)."""

    def efs(C, pos):
        C, pos = np.asarray(C, dtype=np.float64), np.asarray(pos, dtype=np.float64)
        I, J, d, r = pairs(C, pos, rc)
        p, dp = phi(r, rc)
        fv = (dp / r)[:, None] * d  # d phi / d d
        f = np.zeros_like(pos)
        np.add.at(f, I, fv)  # every ordered pair once: the pair (j, i, -image) gives atom j its share
        return 0.5 * float(p.sum()), f, 0.5 * (fv.T @ d) / abs(np.linalg.det(C))

    return efs


def bond_count(C, pos, rc):
    """Unordered pairs within rc (an atom's own images included)."""
    return len(pairs(C, pos, rc)[0]) // 2


def make_forces_fn(rc, stress):
    """The device ``forces_fn`` of ``relax`` and the drivers on it: (energy, forces) or, with ``stress``, (energy, forces,
    stress)."""
    import torch

    def fn(lats, poss):
        es, fs, ss = [], [], []
        for lat, pos in zip(lats, poss):
            n = pos.shape[0]
            img = torch.tensor(images(lat.cpu().numpy(), rc), device=pos.device)
            inv = torch.linalg.inv(lat)
            dp = pos[None, :, :] - pos[:, None, :]
            df = (dp[..., 0:1] * inv[0] + dp[..., 1:2] * inv[1]) + dp[..., 2:3] * inv[2]
            df = df - torch.round(df)
            g = df[:, :, None, :] + img[None, None, :, :]
            d = (g[..., 0:1] * lat[0] + g[..., 1:2] * lat[1]) + g[..., 2:3] * lat[2]  # [n, n, images, 3]
            r = torch.sqrt((d * d).sum(-1))
            own = (torch.eye(n, device=pos.device)[:, :, None] > 0) & ((img == 0).all(1))[None, None, :]
            r = torch.where(own, torch.full_like(r, 2.0 * rc), r)
            p, dphi = phi(r, rc)
            fv = (dphi / r)[..., None] * d
            es.append(0.5 * p.sum(2).sum(1).sum(0))
            fs.append(fv.sum(2).sum(1))
            if stress:
                vol = torch.linalg.det(lat).abs()
                ss.append(0.5 * (fv[..., :, None] * d[..., None, :]).sum(2).sum(1).sum(0) / vol)
        return (torch.stack(es), torch.cat(fs), torch.stack(ss)) if stress else (torch.stack(es), torch.cat(fs))

    return fn
