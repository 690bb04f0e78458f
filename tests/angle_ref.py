"""Plain torch restatement of what csrc/angle.hip writes: the bond-angle embedding
``z = MLPLayer(64 -> 256)(MLPLayer(bins -> 64)(RBFExpansion(h)))`` (alignn/models/alignn.py:215-222), MLPLayer = Linear +
BatchNorm1d + SiLU, entry point by entry point - ``forward`` (alignn_angle_embed_fwd: stat1 / stat2 = mean | rstd | gamma rstd |
beta, the running statistics after the update, z and max |z|), ``backward`` (alignn_angle_embed_bwd: red1 / red2 = dbeta |
dgamma, gW1, gb1, gW2, gb2) and ``infer`` (alignn_angle_embed_infer: z from the running statistics).

Every function works in the dtype it is asked for on the float32 operands of ``operands``: float64 is the reference, the same
function in float32 on the identical operands is the "float32 restatement" tests/test_gpu_angle_f64.py takes its margins from.
No kernel and no ``alignn_amd.ops`` is used.  The backward is written in the closed forms the kernels use;
tests/test_angle_ref.py shows that in float64 they are autograd through RBFExpansion and two MLPLayer modules.

Statistics are the plain two-pass mean and biased variance, as torch's BatchNorm1d takes them - NOT about a pivot row: the kernel's
own pivots (x1 of h[0] or of the median of the first 64 cosines, a1 of that cosine) are among the things under test, and a
float32 restatement that shared them would hide what they cost.

Where a gradient is zero in exact arithmetic - one row (z = silu(beta)), two rows (xhat = +-1 whatever x is), all rows equal
(``constant``) - both sides hold the rounding of its terms; ``backward`` returns the sums of the terms' magnitudes (``t_*``),
against which the errors are measured there (tests/test_gpu_norm.py's rule for one and two rows).

``operands`` draws the distributions of ``DATA`` (module docstring of tests/test_gpu_angle_f64.py).  The conditioning cap
(tests/test_angle_ref.py): the float32 restatement stays within 1e-2 of float64 on every output of every distribution - the
cluster width of ``row0_outlier`` (1e-3) and the beta / gamma ratio of ``beta_heavy`` (up to 500) are frozen inside it."""

import zlib

import torch
import torch.nn.functional as F

EPS, MOMENTUM = 1e-5, 0.1  # nn.BatchNorm1d's defaults
E1, E2 = 64, 256  # embedding_features, hidden_features
DATA = ("normal", "lattice", "row0_outlier", "constant", "beta_heavy", "gamma_zero", "w_tiny", "w_huge", "gz_tiny", "gz_huge",
        "gz_columns", "gz_zero")
# outputs that are zero, or next to it, in exact arithmetic and are therefore measured against the magnitudes of their terms
# (``floors``).  constant: all rows equal - dx sums to zero over the rows and multiplies identical rows, xhat = 0.  w_tiny: the
# spread of x1 is 1e-6 of sqrt(eps), so a1 is constant to 1e-6 and layer 2 is the constant case but for that.  beta_heavy:
# silu'(z1) is constant to 1e-2 and da1 = dx2 W2 sums to zero over the rows, so layer 1's dbeta is 1e-2 of its terms at most.
_ALL = ("gW1", "gW2", "red1/dbeta", "red1/dgamma", "red2/dgamma")
TERM_SCALED = {"constant": _ALL, "w_tiny": ("gW2", "red1/dbeta", "red1/dgamma", "red2/dgamma"), "beta_heavy": ("red1/dbeta",)}
CLUSTER, OUTLIER = 1e-3, -1.0  # row0_outlier: h[0] = -1, the others 0.5 +- 1e-3


def rbf(h, centers, gamma):
    return torch.exp(-gamma * (h[:, None] - centers[None, :]) ** 2)


def dsilu(z):
    s = torch.sigmoid(z)
    return s * (1 + z * (1 - s))


def bn_stat(x, gamma, beta, eps=EPS):
    """[4, F] = mean | rstd | gamma rstd | beta of the batch, and the biased variance"""
    mean = x.mean(0)
    var = ((x - mean) ** 2).mean(0)
    rstd = (var + eps).rsqrt()
    return torch.stack([mean, rstd, gamma * rstd, beta]), var


def eval_stat(rm, rv, gamma, beta, eps=EPS):
    rstd = (rv + eps).rsqrt()
    return torch.stack([rm, rstd, gamma * rstd, beta])


def running_update(rm, rv, mean, var, rows, momentum=MOMENTUM):
    """nn.BatchNorm1d's update: the unbiased variance; with one row the biased one (angle_stat_finalize_kernel)"""
    unbiased = var * rows / (rows - 1) if rows > 1 else var
    return (1 - momentum) * rm + momentum * mean, (1 - momentum) * rv + momentum * unbiased


def _cast(o, dtype):
    return {k: (v.to(dtype) if torch.is_tensor(v) else v) for k, v in o.items()}


def _chain(o, stat1=None, stat2=None):
    """the two layers; batch statistics where none are given"""
    r = rbf(o["h"], o["centers"], o["gamma"])
    x1 = r @ o["W1"].T + o["b1"]
    var1 = None
    if stat1 is None:
        stat1, var1 = bn_stat(x1, o["g1"], o["be1"])
    z1 = (x1 - stat1[0]) * stat1[2] + stat1[3]
    a1 = F.silu(z1)
    x2 = a1 @ o["W2"].T + o["b2"]
    var2 = None
    if stat2 is None:
        stat2, var2 = bn_stat(x2, o["g2"], o["be2"])
    z2 = (x2 - stat2[0]) * stat2[2] + stat2[3]
    return dict(rbf=r, x1=x1, z1=z1, a1=a1, x2=x2, z2=z2, z=F.silu(z2), stat1=stat1, stat2=stat2, var1=var1, var2=var2)


def forward(o, dtype=torch.float64):
    """what alignn_angle_embed_fwd writes (and the intermediates ``backward`` takes)"""
    o = _cast(o, dtype)
    rows = o["h"].numel()
    f = _chain(o)
    f["rm1"], f["rv1"] = running_update(o["rm1"], o["rv1"], f["stat1"][0], f["var1"], rows)
    f["rm2"], f["rv2"] = running_update(o["rm2"], o["rv2"], f["stat2"][0], f["var2"], rows)
    f["zmax"] = f["z"].abs().max()
    return f


def infer(o, dtype=torch.float64, running=None):
    """what alignn_angle_embed_infer writes: z from the running statistics (rm1, rv1, rm2, rv2; default: the operands')"""
    o = _cast(o, dtype)
    rm1, rv1, rm2, rv2 = (t.to(dtype) for t in running) if running is not None else (o[k] for k in ("rm1", "rv1", "rm2", "rv2"))
    return _chain(o, eval_stat(rm1, rv1, o["g1"], o["be1"]), eval_stat(rm2, rv2, o["g2"], o["be2"]))["z"]


def backward(o, f, gz=None):
    """what alignn_angle_embed_bwd writes from ``f = forward(o, dtype)``, in f's dtype: red = [dbeta | dgamma], gW, gb per layer,
    and t_* = the sums of the magnitudes of the terms each of them adds up"""
    dtype = f["z"].dtype
    o = _cast(o, dtype)
    gz = o["gz"] if gz is None else gz.to(dtype)
    n = o["h"].numel()
    out = {}

    def layer(g_out, zl, x, stat, inp, tag):
        gzl = g_out * dsilu(zl)
        xh = (x - stat[0]) * stat[1]
        red = torch.stack([gzl.sum(0), (gzl * xh).sum(0)])
        dx = stat[2] * (gzl - (red[0] + xh * red[1]) / n)
        out["red" + tag], out["gW" + tag], out["gb" + tag] = red, dx.T @ inp, dx.sum(0)
        t = stat[2].abs() * gzl.abs()
        xt = (x.abs() + stat[0].abs()) * stat[1]  # |x| rstd + |mean| rstd: the terms of xhat
        out["t_red" + tag] = torch.stack([gzl.abs().sum(0), (gzl.abs() * xt).sum(0)])
        out["t_gW" + tag] = t.T @ inp.abs()
        out["m_red" + tag] = torch.stack([gzl.abs().sum(0), (gzl * xh).abs().sum(0)])  # magnitudes of the summands
        return dx, t

    dx2, t2 = layer(gz, f["z2"], f["x2"], f["stat2"], f["a1"], "2")
    da1 = dx2 @ o["W2"]
    t_da1 = t2 @ o["W2"].abs()
    layer(da1, f["z1"], f["x1"], f["stat1"], f["rbf"], "1")
    # layer 1's sums are sums of da1, itself a sum: their terms are those of da1
    d1 = dsilu(f["z1"]).abs() * t_da1
    xh1 = (f["x1"].abs() + f["stat1"][0].abs()) * f["stat1"][1]
    out["t_red1"] = torch.stack([d1.sum(0), (d1 * xh1).sum(0)])
    out["t_gW1"] = (f["stat1"][2].abs() * d1).T @ f["rbf"]
    return out


def floors(b, rows, data):
    """{output: scale below which its error is not taken relative} from b = backward(...) in float64: the terms' magnitudes
    where the result is zero in exact arithmetic (one or two rows, TERM_SCALED), else nothing"""
    names = _ALL if rows <= 2 else TERM_SCALED.get(data, ())
    t = {"gW1": b["t_gW1"], "gW2": b["t_gW2"], "red1/dbeta": b["t_red1"][0], "red1/dgamma": b["t_red1"][1], "red2/dgamma": b["t_red2"][1]}
    return {k: max(float(t[k].max()), 1e-30) for k in names}


# ----------------------------------------------------------------------------------------------------------------------
# operands (float32, on the CPU: what the kernel and both restatements read)
# ----------------------------------------------------------------------------------------------------------------------
def rbf_gamma(centers):
    """RBFExpansion's: 1 / mean spacing of the centres, taken in float32; one bin has no spacing: 1"""
    if centers.numel() < 2:
        return 1.0
    return float(1.0 / (centers[1:] - centers[:-1]).mean(dtype=torch.float32))


def operands(rows, bins, data, seed=0):
    """h [rows], centers [bins] and gamma of the expansion, W1 b1 g1 be1 / W2 b2 g2 be2 (Linear as nn.Linear draws it, BatchNorm
    affine away from (1, 0)), running statistics that are not the batch's, and the adjoint gz [rows, 256]"""
    assert data in DATA
    gen = torch.Generator().manual_seed(zlib.crc32(f"{rows} {bins} {data} {seed}".encode()))
    R = lambda *s: torch.randn(*s, generator=gen)  # noqa: E731
    U = lambda *s: torch.rand(*s, generator=gen)  # noqa: E731
    sign = lambda *s: torch.where(U(*s) < 0.5, -1.0, 1.0)  # noqa: E731
    centers = torch.linspace(-1.0, 1.0, bins)
    o = dict(centers=centers, gamma=rbf_gamma(centers))
    for k, (fin, fout) in (("1", (bins, E1)), ("2", (E1, E2))):
        o["W" + k], o["b" + k] = (2 * U(fout, fin) - 1) / fin ** 0.5, (2 * U(fout) - 1) / fin ** 0.5
        o["g" + k], o["be" + k] = 0.5 + U(fout), U(fout) - 0.5
        o["rm" + k], o["rv" + k] = 0.3 * R(fout), 0.5 + U(fout)
    h = 2 * U(rows) - 1  # cosines
    gz = R(rows, E2) * (U(E2) + 0.1) + 0.05
    if data == "lattice":  # crystal cosines: a handful of exact values, heavily repeated
        h = torch.tensor([-1.0, -0.5, 0.0, 0.5, 1.0])[torch.randint(0, 5, (rows,), generator=gen)]
    elif data == "row0_outlier":
        h = 0.5 + CLUSTER * (2 * U(rows) - 1)
        h[0] = OUTLIER
    elif data == "constant":
        h = torch.full((rows,), 0.3)
    elif data == "beta_heavy":  # mean(a1) >> std(a1)
        o["g1"], o["be1"] = sign(E1) * (0.01 + 0.01 * U(E1)), sign(E1) * (3 + 2 * U(E1))
    elif data == "gamma_zero":
        o["g1"][::4] = 0.0
        o["g2"][::4] = 0.0
    elif data in ("w_tiny", "w_huge"):
        s = 2.0 ** (-20 if data == "w_tiny" else 10)
        o["W1"], o["W2"] = o["W1"] * s, o["W2"] * s
    elif data in ("gz_tiny", "gz_huge"):
        gz = gz * 2.0 ** (-40 if data == "gz_tiny" else 20)
    elif data == "gz_columns":  # column scales 1 .. 2^-12
        gz = gz * 2.0 ** (-12 * torch.arange(E2) / (E2 - 1))
    elif data == "gz_zero":
        gz = torch.zeros(rows, E2)
    o["h"], o["gz"] = h.contiguous(), gz.contiguous()
    return o
