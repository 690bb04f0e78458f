"""Plain torch restatements of what csrc/conv.hip computes: ``EdgeGatedGraphConv.forward`` (alignn/models/alignn.py:78-129) in
its BatchNorm flavour with m = A[u] + Bd[v] + C, its two column normalisations with their running statistics, and the reverse
passes as autograd of the same expressions.

Every function works in the dtype of its floating inputs - float64 is the reference, the same function on the identical float32
operands is the "float32 restatement" the GPU tests (tests/test_gpu_conv_bn.py) take their margin from on every data
distribution other than N(0,1).  Only forward formulas are written here (``index_add``, ``sigmoid``, ``silu``, explicit column
statistics); every adjoint is ``torch.autograd.grad`` of them, so a wrong derivative formula cannot sit on both sides of a
comparison.  The graph arguments are plain index tensors ``u -> v`` (source and destination of every row).

Column statistics are taken about a pivot row (mean = p + mean(x - p), var = mean((x - mean)^2)): the same value in exact
arithmetic, and in float32 it keeps an exactly constant column exactly constant and does not lose the spread of a column whose
mean is a hundred spreads away - which is what the kernels' pivot slabs do, so the float32 restatement stays a fair yardstick.

``operands`` draws the data distributions of the GPU tests.  The conditioning cap (tests/test_conv_bn_ref.py): on each of them
the float32 restatement stays within 1e-4 of float64 on every output, the bar of BASELINE.json's north star; a distribution
that left it would be too ill-conditioned to judge a float32 kernel by, and would be tamed HERE, never loosened or skipped on
the GPU side.  One was tamed that way:
* ``constant_column``: a column of m that is exactly constant has rstd = 1 / sqrt(eps) = 316, and the training-mode BatchNorm
  backward there is 316 * gamma times a sum that cancels; the column sums gb of GM then lose digits in float32 (1.7e-4 measured
  with gamma ~ 1).  The constant columns take gamma / 16 (1.2e-5 measured); variance 0 and rstd = 1 / sqrt(eps) stay.
How the others are drawn:
* ``column_offset`` moves the column means of m by up to 100 spreads of m in every fourth column (the gate's sigmoid is
  saturated there) and by up to +-8 in the others, where the gate is still alive and the quotient h = S1 / (S0 + eps) is
  still measured;
* ``saturated_gates`` builds every third row as sign * (110 + 20 |m|), so that the sigmoid is exactly 0 or 1 in float32 and in
  float64 alike (scaling an N(0, 3) row would leave values near 0 whose gate is anything); the whole segments of every
  fifth node take m = -(22 + 2 |m|), S0 ~ 1e-9 far below the epsilon, and those of another fifth -(110 + 20 |m|), S0 = 0.
  The remaining rows stay as drawn."""

import zlib

import torch
import torch.nn.functional as F

EPS_BN, EPS_GATE, MOMENTUM = 1e-5, 1e-6, 0.1  # nn.BatchNorm1d's defaults; ALIGNN_EPS_GATE (csrc/common.h)
DATA = ("normal", "column_offset", "constant_column", "saturated_gates", "gamma_zero_negative")


def blocks(P, H):
    """A | Bd | Bh | Ux of the fused node projection [n, 4H]"""
    return P[:, :H], P[:, H:2 * H], P[:, 2 * H:3 * H], P[:, 3 * H:]


# ----------------------------------------------------------------------------------------------------------------------
# column normalisation
# ----------------------------------------------------------------------------------------------------------------------
def column_stats(x):
    """(mean, biased variance) of every column, about the first row as pivot; zeros for a matrix without rows"""
    if x.shape[0] == 0:
        z = x.new_zeros(x.shape[1])
        return z, z.clone()
    p = x[:1].detach()
    mean = p[0] + (x - p).mean(0)
    return mean, ((x - mean) ** 2).mean(0)


def batch_stat(x, gamma, beta):
    """[4, H] = mean, rstd, scale = gamma * rstd, shift = beta from the batch statistics (training mode), and the variance"""
    mean, var = column_stats(x)
    rstd = (var + EPS_BN).rsqrt()
    return torch.stack([mean, rstd, gamma * rstd, beta]), var


def eval_stat(running_mean, running_var, gamma, beta):
    """the same [4, H] from running statistics (evaluation mode: a fixed affine map)"""
    rstd = (running_var + EPS_BN).rsqrt()
    return torch.stack([running_mean, rstd, gamma * rstd, beta])


def running_update(running_mean, running_var, mean, var, rows):
    """nn.BatchNorm1d's update: momentum 0.1, unbiased variance"""
    unbiased = var * rows / (rows - 1) if rows > 1 else var
    return (1 - MOMENTUM) * running_mean + MOMENTUM * mean, (1 - MOMENTUM) * running_var + MOMENTUM * unbiased


def norm_silu(x, stat):
    return F.silu((x - stat[0]) * stat[2] + stat[3])


# ----------------------------------------------------------------------------------------------------------------------
# forward
# ----------------------------------------------------------------------------------------------------------------------
def values(P, C_or_M, pre, gamma, beta, stat, u, v, n, H, n_gamma=None, n_beta=None, n_stat=None, running=None):
    """What the forward pass writes.  ``pre``: the second argument IS m; otherwise it is C and m = A[u] + Bd[v] + C.  ``stat``
    ([4, H], evaluation mode) replaces the batch statistics of the edge normalisation by a fixed affine map, ``n_stat`` those
    of the node normalisation; ``n_gamma`` / ``n_beta`` add the node branch x = silu(norm(xpre)); ``running`` = dict(e_rm,
    e_rv, n_rm, n_rv) adds the updated running statistics under the same keys."""
    A, Bd, Bh, Ux = blocks(P, H)
    m = C_or_M if pre else A[u] + Bd[v] + C_or_M
    sg = torch.sigmoid(m)
    z = lambda: torch.zeros(n, H, dtype=m.dtype, device=m.device)  # noqa: E731
    s1, s0 = z().index_add(0, v, sg * Bh[u]), z().index_add(0, v, sg)
    hh = s1 / (s0 + EPS_GATE)
    xpre = Ux + hh
    out = dict(m=m, s1=s1, s0=s0, hh=hh, xpre=xpre)
    e_batch, e_var = batch_stat(m, gamma, beta)
    e_use = e_batch if stat is None else stat
    out.update(e_mean=e_batch[0], e_var=e_var, e_rstd=e_batch[1], e_scale=e_batch[2], e_shift=e_batch[3], e_stat=e_use,
               y=norm_silu(m, e_use))
    n_mean, n_var = column_stats(xpre)
    out.update(n_mean=n_mean, n_var=n_var, n_rstd=(n_var + EPS_BN).rsqrt())
    if n_gamma is not None:
        n_batch, _ = batch_stat(xpre, n_gamma, n_beta)
        n_use = n_batch if n_stat is None else n_stat
        out.update(n_scale=n_batch[2], n_shift=n_batch[3], n_stat=n_use, x=norm_silu(xpre, n_use))
    if running is not None:
        out["e_rm"], out["e_rv"] = running_update(running["e_rm"], running["e_rv"], e_batch[0], e_var, m.shape[0])
        out["n_rm"], out["n_rv"] = running_update(running["n_rm"], running["n_rv"], n_mean, n_var, n)
    return out


def node_reverse(g, s0, hh):
    """adjoints of the two segment sums from the adjoint g of xpre = Ux + s1 / (s0 + eps), hh = s1 / (s0 + eps)"""
    gs1 = g / (s0 + EPS_GATE)
    return gs1, -gs1 * hh


# ----------------------------------------------------------------------------------------------------------------------
# reverse
# ----------------------------------------------------------------------------------------------------------------------
def reverse(dtype, P, M, gamma, beta, stat, GY, Q1, Q0, u, v, n, H, mode, e_eval):
    """float-``dtype`` autograd of <GY, y> + <Q1, s1> + <Q0, s0>.  mode 1: y = silu(norm(m)), the norm from the batch statistics
    of m, or (``e_eval``) from the fixed mean and rstd in rows 0 and 1 of ``stat``; mode 0: no GY term; mode 2: GY is added to
    the adjoint of m as is (<GY, m>).  m = A[u] + Bd[v] + C enters as the given M plus terms that are zero in value and carry
    the adjoint to A and Bd.  Returns GM (adjoint of m), GP [n, 3H] (A | Bd | Bh), GP_bd, gb = GM.sum(0) and, in mode 1, e_red
    [2, H] = (sum gz, sum gz * xhat) - the adjoints of beta and gamma."""
    c = lambda t: t.to(dtype)  # noqa: E731
    lv = {k: c(t).clone().requires_grad_(True) for k, t in (("M", M), ("P", P), ("gamma", gamma), ("beta", beta))}
    A, Bd, _, _ = blocks(lv["P"], H)
    m = lv["M"] + (A[u] - A[u].detach()) + (Bd[v] - Bd[v].detach())
    fixed = None
    if mode == 1 and e_eval:
        mean, rstd = c(stat[0]), c(stat[1])
        fixed = torch.stack([mean, rstd, lv["gamma"] * rstd, lv["beta"]])
    f = values(lv["P"], m, True, lv["gamma"], lv["beta"], fixed, u, v, n, H)
    loss = (c(Q1) * f["s1"]).sum() + (c(Q0) * f["s0"]).sum()
    if mode == 1:
        loss = loss + (c(GY) * f["y"]).sum()
    elif mode == 2:
        loss = loss + (c(GY) * m).sum()
    gm, gp, dgamma, dbeta = torch.autograd.grad(loss, [lv["M"], lv["P"], lv["gamma"], lv["beta"]], allow_unused=True)
    out = dict(GM=gm, GP=gp[:, :3 * H], GP_bd=gp[:, H:2 * H], gb=gm.sum(0))
    if mode == 1:
        out["e_red"] = torch.stack([dbeta, dgamma])
    return out


# ----------------------------------------------------------------------------------------------------------------------
# operands (float32; what the kernels and both restatements read)
# ----------------------------------------------------------------------------------------------------------------------
def operands(H, u, v, n, data, key, device):
    """P, the edge term C and m = A[u] + Bd[v] + C as the float32 tensor M the `pre` entry points and the reverse passes are
    handed (C = M - A[u] - Bd[v] in float32, so what the non-pre entry points form themselves is M up to one rounding), the
    adjoints GY, Q1, Q0, GX, the residual Y, the parameters of both normalisations and running statistics that differ
    from the batch's.  See the module docstring for the distributions."""
    assert data in DATA
    m = int(u.numel())
    gen = torch.Generator(device=device).manual_seed(zlib.crc32(f"{H} {key} {data}".encode()))
    R = lambda *s: torch.randn(*s, device=device, generator=gen)  # noqa: E731
    U = lambda *s: torch.rand(*s, device=device, generator=gen)  # noqa: E731
    o = dict(P=R(n, 4 * H), Y=R(m, H), GY=R(m, H), Q1=R(n, H), Q0=R(n, H), GX=R(n, H), GXW=R(n, 4 * H))
    C0 = R(m, H)
    for k in ("e", "n"):
        o[k + "_gamma"], o[k + "_beta"], o[k + "_rm"], o[k + "_rv"] = 1 + 0.2 * R(H), 0.2 * R(H), 0.3 * R(H), 0.5 + U(H)
    col, row = torch.arange(H, device=device), torch.arange(m, device=device)
    if data == "constant_column":  # every fourth column of m exactly constant: A and Bd contribute an exact 0 there
        o["P"][:, :2 * H][:, (col % 4 == 0).repeat(2)] = 0.0
    A, Bd, _, _ = blocks(o["P"], H)
    M = A[u] + Bd[v] + C0
    if data == "column_offset" and m > 0:
        spread = float(M.std())
        off = (2 * U(1, H) - 1) * torch.where(col % 4 == 0, 100.0 * spread, 8.0)
        M = M + off
    elif data == "constant_column":
        M = torch.where((col % 4 == 0)[None, :], R(1, H).expand(m, H), M)
        o["e_gamma"] = torch.where(col % 4 == 0, 1.0 / 16, 1.0) * o["e_gamma"]
    elif data == "saturated_gates":
        seg = (v + 2) % 5
        M = torch.where((row % 3 == 0)[:, None], torch.sign(M) * (110.0 + 20.0 * M.abs()), M)
        M = torch.where((seg == 0)[:, None], -(22.0 + 2.0 * M.abs().clamp_max(3.0)), M)
        M = torch.where((seg == 1)[:, None], -(110.0 + 20.0 * M.abs().clamp_max(3.0)), M)
    elif data == "gamma_zero_negative":
        o["e_gamma"] = torch.where(col % 3 == 0, 0.0, 1.0) * R(H)
        o["n_gamma"] = torch.where(col % 3 == 1, 0.0, 1.0) * R(H)
    o["M"] = M.contiguous()
    o["C"] = (o["M"] - A[u] - Bd[v]).contiguous()
    return o
