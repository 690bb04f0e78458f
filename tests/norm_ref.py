"""Plain torch restatements of what csrc/norm.hip computes on [rows, F] matrices: column statistics and BatchNorm1d + SiLU
(+ residual) forward and backward (alignn/models/alignn.py:122-127, 175-179), LayerNorm + SiLU forward and backward
(alignn/models/utils.py:277-292), the quotient adjoints the node forms add, and the column / slab sums.

Every function works in the dtype of its floating inputs - float64 is the reference, the same function on the identical float32
operands is the "float32 restatement" tests/test_gpu_norm.py takes its margins from.  No kernel and no ``alignn_amd.ops`` is
used.  The backward passes are written in the closed forms the kernels use (they take the parameter sums ``red`` and the saved
statistics as inputs, so autograd cannot state them); tests/test_norm_ref.py shows that the closed forms are autograd of
``F.batch_norm`` / ``F.layer_norm`` + ``F.silu`` and derivatives by central differences.

Column statistics are taken about a pivot row, as tests/conv_bn_ref.py does and for the same reason: the same value in exact
arithmetic, and in float32 an exactly constant column stays exactly constant and a column whose mean is thirty spreads away
keeps its spread - which is what the kernels' pivot slabs do.

``operands`` draws the data distributions of the GPU tests.  The conditioning cap (tests/test_norm_ref.py): on each of them the
float32 restatement stays within 1e-4 of float64 on every output.  ``offset300`` (300 (1 + 0.01 col) + 1e-2 noise) does NOT -
y 1.2e-3, gx 2.7e-3: there the data's own float32 resolution (ulp 3e-5 against a spread of 1e-2) is the limit - and is therefore
in STAT_DATA only: the statistics entry points (mean, rstd, running variance) are measured on it, nothing else."""

import zlib

import torch
import torch.nn.functional as F

EPS_BN, EPS_LN, EPS_GATE, MOMENTUM = 1e-5, 1e-5, 1e-6, 0.1  # nn.BatchNorm1d's / nn.LayerNorm's defaults; ALIGNN_EPS_GATE
FOLD = 64  # alignn_slab_fold_slabs()
DATA = ("normal", "offset30", "constant", "saturated", "gamma30", "tiny", "outlier")
STAT_DATA = DATA + ("offset300",)


# ----------------------------------------------------------------------------------------------------------------------
# column statistics, BatchNorm
# ----------------------------------------------------------------------------------------------------------------------
def col_stats(x):
    """(mean, biased variance) of every column, about the first row as pivot"""
    p = x[:1]
    mean = p[0] + (x - p).mean(0)
    return mean, ((x - mean) ** 2).mean(0)


def bn_stat(x, gamma, beta, eps=EPS_BN):
    """[4, F] = mean, rstd = 1 / sqrt(var + eps), scale = gamma * rstd, shift = beta from the batch; and the biased variance"""
    mean, var = col_stats(x)
    rstd = (var + eps).rsqrt()
    return torch.stack([mean, rstd, gamma * rstd, beta]), var


def eval_stat(running_mean, running_var, gamma, beta, eps=EPS_BN):
    """the same block from the running statistics (evaluation mode); gamma / beta None: 1 / 0"""
    rstd = (running_var + eps).rsqrt()
    gamma = torch.ones_like(rstd) if gamma is None else gamma
    beta = torch.zeros_like(rstd) if beta is None else beta
    return torch.stack([running_mean, rstd, gamma * rstd, beta])


def running_update(running_mean, running_var, mean, var, rows, momentum=MOMENTUM):
    """nn.BatchNorm1d's update: the unbiased variance when there is more than one row, else the biased one (the kernels)"""
    unbiased = var * rows / (rows - 1) if rows > 1 else var
    return (1 - momentum) * running_mean + momentum * mean, (1 - momentum) * running_var + momentum * unbiased


def dsilu(z):
    s = torch.sigmoid(z)
    return s * (1 + z * (1 - s))


def bn_silu_fwd(x, res, stat):
    y = F.silu((x - stat[0]) * stat[2] + stat[3])
    return y if res is None else y + res


def bn_bwd_red(gy, x, stat):
    """[2, F] = (sum gz, sum gz * xhat): the adjoints of beta and gamma"""
    xc = x - stat[0]
    gz = gy * dsilu(xc * stat[2] + stat[3])
    return torch.stack([gz.sum(0), (gz * (xc * stat[1])).sum(0)])


def bn_bwd_apply(gy, x, stat, red, eval_mode):
    """adjoint of x: scale * (gz - (red0 + xhat * red1) / rows) from batch statistics, gz * scale from frozen ones"""
    xc = x - stat[0]
    gz = gy * dsilu(xc * stat[2] + stat[3])
    if eval_mode:
        return gz * stat[2]
    return stat[2] * (gz - (red[0] + xc * stat[1] * red[1]) / x.shape[0])


def node_adjoints(gx, s0, hh):
    """adjoints of the two segment sums from the adjoint gx of xpre = Ux + s1 / (s0 + eps), hh = s1 / (s0 + eps)"""
    gs1 = gx / (s0 + EPS_GATE)
    return gs1, -gs1 * hh


# ----------------------------------------------------------------------------------------------------------------------
# LayerNorm
# ----------------------------------------------------------------------------------------------------------------------
def ln_silu_fwd(x, res, gamma, beta, eps=EPS_LN):
    """-> y, stats [rows, 2] = (mean, rstd) of every row"""
    mean = x.mean(1, keepdim=True)
    rstd = (((x - mean) ** 2).mean(1, keepdim=True) + eps).rsqrt()
    y = F.silu((x - mean) * rstd * gamma + beta)
    return (y if res is None else y + res), torch.cat([mean, rstd], 1)


def ln_silu_bwd(gy, x, gamma, beta, stats):
    """-> gx, dbeta, dgamma from the saved (mean, rstd) rows"""
    mean, rstd = stats[:, :1], stats[:, 1:]
    xh = (x - mean) * rstd
    gz = gy * dsilu(xh * gamma + beta)
    gh = gz * gamma
    gx = rstd * (gh - gh.mean(1, keepdim=True) - xh * (gh * xh).mean(1, keepdim=True))
    return gx, gz.sum(0), (gz * xh).sum(0)


# ----------------------------------------------------------------------------------------------------------------------
# sums
# ----------------------------------------------------------------------------------------------------------------------
def col_sum(x):
    return x.sum(0)


def slab_fold(partial, groups=FOLD):
    """out[g] = sum of partial[k] over k = g (mod groups); zeros where there is no such slab"""
    out = partial.new_zeros(groups, partial.shape[1])
    return out.index_add(0, torch.arange(partial.shape[0], device=partial.device) % groups, partial)


def slab_sum(partial):
    return partial.sum(0)


# ----------------------------------------------------------------------------------------------------------------------
# operands (float32; what the kernels and both restatements read)
# ----------------------------------------------------------------------------------------------------------------------
def operands(rows, Fdim, data, device, kind="bn"):
    """x, the adjoint gy, the residual r, gamma, beta, running statistics that are not the batch's, and for the node forms s0
    (exact zeros on every 7th row) and hh.  ``kind``: "bn" varies columns where "ln" varies rows (``constant``: every fourth
    column / row exactly constant; ``offset30``: the means of the columns / rows).  See the module docstring."""
    assert data in STAT_DATA and kind in ("bn", "ln")
    gen = torch.Generator(device=device).manual_seed(zlib.crc32(f"{rows} {Fdim} {data} {kind}".encode()))
    R = lambda *s: torch.randn(*s, device=device, generator=gen)  # noqa: E731
    U = lambda *s: torch.rand(*s, device=device, generator=gen)  # noqa: E731
    o = dict(gy=R(rows, Fdim), r=R(rows, Fdim), hh=R(rows, Fdim), s0=8 * U(rows, Fdim), gamma=1 + 0.2 * R(Fdim), beta=0.2 * R(Fdim),
             rm=0.3 * R(Fdim), rv=0.5 + U(Fdim))
    o["s0"][::7] = 0.0
    z = R(rows, Fdim)
    col = torch.arange(Fdim, device=device, dtype=torch.float32)
    idx = col[None, :] if kind == "bn" else torch.arange(rows, device=device, dtype=torch.float32)[:, None]
    if data == "normal":
        x = z * 2 + 0.5
    elif data == "offset30":  # |mean| / std = 30 .. 50
        x = 30.0 * (1 + 0.01 * (idx % 64)) + z
    elif data == "offset300":
        x = 300.0 * (1 + 0.01 * (idx % 64)) + 1e-2 * z
    elif data == "constant":  # var = 0 exactly: rstd = 1 / sqrt(eps)
        c = R(1, Fdim) if kind == "bn" else R(rows, 1)
        x = torch.where(idx % 4 == 0, c.expand(rows, Fdim), z * 2 + 0.5)
    elif data == "saturated":  # |z| up to ~150: sigmoid is 0 or 1
        x = z * 40
    elif data == "gamma30":
        x = z
        o["gamma"] = o["gamma"] * 30
    elif data == "tiny":  # var << eps
        x = z * 1e-4
    elif data == "outlier":
        x = z * 2 + 0.5
        if rows > 0:
            x[rows // 2, Fdim // 2] = 4e4
    o["x"] = x.contiguous()
    return o
