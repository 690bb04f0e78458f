"""Plain torch restatements of what csrc/embed.hip and csrc/ff.hip compute: the geometry features, the pooling and gather
primitives, the ALIGNN-FF head (alignn/models/alignn_atomwise.py:494-638) and the seeds of the second-order pass.

Every function works in the dtype of its floating inputs - float64 is the reference, the same function on float32 CPU tensors is
the "float32 restatement" the GPU tests take their margin from.  Only FORWARD formulas are written here (indexing, ``index_add``,
``clamp``, ``exp``, ``norm``); every derivative and tangent is ``grad_of`` / ``jvp_of`` of such a formula, so a wrong derivative
formula cannot sit on both sides of a comparison.  Nothing of alignn_amd is imported: the graph arguments are plain index tensors
(``src``, ``dst``, ``graph_ptr``, ...), which is what the graph containers hold.

tests/test_ff_head_ref.py checks this file itself (central differences, cases by hand, the reference's goldens)."""

import math

import torch

STRESS_UNIT = -160.21766208  # eV / A^3 -> GPa with the sign of the virial (alignn_atomwise.py:621-622)
# what a GPU test allows a kernel on top of 4 x this file's float32 error: 2e-6 absolute for an RBF value, 1e-6 of the largest
# element for lengths, cosines and means, 2e-5 of the largest element for gradients and tangents (tests/test_gpu_ff_head.py;
# tests/test_gpu_stage_ref.py takes the cosine bound for the h of alignn_stage_batch)
B_RBF, B_VALUE, B_GRAD = 2e-6, 1e-6, 2e-5


# ----------------------------------------------------------------------------------------------------------------------
# differentiation of a restatement
# ----------------------------------------------------------------------------------------------------------------------
def grad_of(fn, inputs, cotangent):
    """gradients of <cotangent, fn(*inputs)> w.r.t. every input (a tuple), by reverse autograd"""
    leaves = [t.detach().clone().requires_grad_(True) for t in inputs]
    out = fn(*leaves)
    got = torch.autograd.grad((out * cotangent).sum(), leaves, allow_unused=True)
    return tuple(torch.zeros_like(x) if g is None else g for g, x in zip(got, leaves))


def jvp_of(fn, inputs, tangents):
    """directional derivative of fn at ``inputs`` along ``tangents``, by forward-over-reverse autograd"""
    return torch.autograd.functional.jvp(fn, tuple(inputs), tuple(tangents))[1]


# ----------------------------------------------------------------------------------------------------------------------
# geometry features
# ----------------------------------------------------------------------------------------------------------------------
def rbf(d, centers, gamma):
    """RBFExpansion.forward (alignn/models/utils.py:40-44): [rows, bins]"""
    return torch.exp(-gamma * (d.unsqueeze(1) - centers.to(d.dtype)) ** 2)


def rbf_gamma(vmin, vmax, bins):
    """1 / lengthscale with lengthscale = mean spacing of the centres (utils.py:30-36); 9.875 and 19.5 for the model's two"""
    return (bins - 1) / (vmax - vmin) if bins > 1 else 1.0


def bond_length(r):
    return torch.norm(r, dim=1)


def cosine_of_pairs(a, b):
    """compute_bond_cosines (alignn/graphs.py:847-864) for bond vectors a = r[e1], b = r[e2]: r1 = -a, r2 = b"""
    r1 = -a
    c = (r1 * b).sum(1) / (torch.norm(r1, dim=1) * torch.norm(b, dim=1))
    return torch.clamp(c, -1, 1)


def bond_cosine(r, e1, e2):
    return cosine_of_pairs(r[e1.long()], r[e2.long()])


# ----------------------------------------------------------------------------------------------------------------------
# pooling, sums over segments, gathers
# ----------------------------------------------------------------------------------------------------------------------
def owners(ptr):
    """segment of every row, for offsets ptr [n + 1] (repeated offsets = empty segments)"""
    counts = (ptr[1:] - ptr[:-1]).long()
    return torch.repeat_interleave(torch.arange(counts.numel()), counts)


def segment_sum(vals, ptr, slot=None, node=None, n_out=None):
    """out[node[s] or s] = sum over k in [ptr[s], ptr[s + 1]) of vals[slot[k] or k]; rows no segment writes stay 0"""
    n_seg = ptr.numel() - 1
    own = owners(ptr)
    rows = vals[slot.long()] if slot is not None else vals[: own.numel()]
    out = torch.zeros(n_seg, vals.shape[1], dtype=vals.dtype).index_add(0, own, rows)
    if node is None:
        return out
    full = torch.zeros(n_seg if n_out is None else n_out, vals.shape[1], dtype=vals.dtype)
    full[node.long()] = out
    return full


def segment_mean(x, graph_ptr):
    """dgl.nn.AvgPooling (alignn/models/alignn.py:325); a crystal without atoms pools to 0"""
    counts = (graph_ptr[1:] - graph_ptr[:-1]).to(x.dtype)
    s = torch.zeros(counts.numel(), x.shape[1], dtype=x.dtype).index_add(0, owners(graph_ptr), x)
    return s / counts.clamp_min(1).unsqueeze(1)


def gather(x, perm):
    return x[perm.long()]


# ----------------------------------------------------------------------------------------------------------------------
# the head: energies, forces, stresses
# ----------------------------------------------------------------------------------------------------------------------
def energies(pred, bl, graph_ptr, mult_natoms, use_penalty, factor=0.1, thr=1.0):
    """alignn_atomwise.py:494-510 -> (out, en_out).  ``en_out`` is what the forces differentiate: pred * natoms with
    energy_mult_natoms, plus the batch's short-bond penalty (added to EVERY crystal's energy).  Without energy_mult_natoms
    ``en_out`` IS ``out`` and the penalty is added in place, so the returned energies carry it too."""
    counts = (graph_ptr[1:] - graph_ptr[:-1]).to(pred.dtype)
    en_out = pred * counts if mult_natoms else pred
    if use_penalty:
        en_out = en_out + torch.where(bl < thr, factor * (thr - bl), torch.zeros_like(bl)).sum()
    return (pred if mult_natoms else en_out), en_out


def energy_seed(pred, bl, graph_ptr, mult_natoms, use_penalty, factor=0.1, thr=1.0):
    """d(sum_g en_out_g) / d pred: what the reverse pass of the model starts from (grad_outputs = ones, :532-538)"""
    fn = lambda p: energies(p, bl, graph_ptr, mult_natoms, use_penalty, factor, thr)[1]  # noqa: E731
    return grad_of(fn, (pred,), torch.ones_like(pred))[0]


def penalty_grad(pred, bl, graph_ptr, factor=0.1, thr=1.0):
    """d(sum_g en_out_g) / d bl: the penalty's share of dE/d(bond length)"""
    fn = lambda b: energies(pred, b, graph_ptr, True, True, factor, thr)[1]  # noqa: E731
    return grad_of(fn, (bl,), torch.ones_like(pred))[0]


def forces_of(pf, src, dst, n_atoms, add_reverse=True):
    """alignn_atomwise.py:547-565: in-edge sum of the pair forces minus (add_reverse_forces) the out-edge sum"""
    f = torch.zeros(n_atoms, 3, dtype=pf.dtype).index_add(0, dst.long(), pf)
    if add_reverse:
        f = f - torch.zeros(n_atoms, 3, dtype=pf.dtype).index_add(0, src.long(), pf)
    return f


def stresses_of(r, pf, edge_ptr, volume, k=STRESS_UNIT):
    """alignn_atomwise.py:615-638: S_g = k r_g^T pf_g / V_g over the bonds [edge_ptr[g], edge_ptr[g + 1]) of crystal g, from the
    SCALED pair forces; k = stress_multiplier * STRESS_UNIT; V_g is the V of the crystal's first atom (:629)"""
    own = owners(edge_ptr)
    outer = r[: own.numel(), :, None] * pf[: own.numel(), None, :]
    s = torch.zeros(edge_ptr.numel() - 1, 3, 3, dtype=pf.dtype).index_add(0, own, outer)
    return k * s / volume.to(pf.dtype)[:, None, None]


def edge_ptr_of(graph_ptr, seg_ptr):
    """bond offsets per crystal from atom offsets per crystal and bond offsets per (destination) atom"""
    return seg_ptr[graph_ptr.long()]


# ----------------------------------------------------------------------------------------------------------------------
# seeds of the second-order pass
# ----------------------------------------------------------------------------------------------------------------------
def pair_weights(gF, gS, r, src, dst, edge_ptr, volume, kS, add_reverse, n_atoms, n_edges):
    """w = dL/df for L = <gF, F(f)> + <gS, S(f)> (either may be None), by autograd through forces_of / stresses_of"""
    dt = r.dtype if r is not None else gF.dtype
    f = torch.zeros(n_edges, 3, dtype=dt, requires_grad=True)
    loss = f.sum() * 0
    if gF is not None:
        loss = loss + (gF * forces_of(f, src, dst, n_atoms, add_reverse)).sum()
    if gS is not None:
        loss = loss + (gS.reshape(-1, 3, 3) * stresses_of(r, f, edge_ptr, volume, kS)).sum()
    return torch.autograd.grad(loss, f)[0]


def pow2_exponent(wmax):
    """k with 2^k <= wmax < 2^(k + 1); 0 for wmax == 0 (the tangent direction is w itself)"""
    wmax = float(wmax)
    return math.frexp(wmax)[1] - 1 if wmax > 0 else 0


def tangent_geometry(r, w, wmax):
    """(rt, dt, k): rt = w / 2^k with k = floor(log2 wmax), dt = the derivative of the bond length along rt"""
    k = pow2_exponent(wmax)
    rt = w * 2.0 ** -k  # (a power of two: exact)
    return rt, jvp_of(bond_length, (r,), (rt,)), k


def readout(x, graph_ptr, fc_w, fc_b):
    """E_g = fc(mean_i x_i) (alignn_atomwise.py:464-466), one output feature"""
    return segment_mean(x, graph_ptr) @ fc_w.reshape(-1) + fc_b.reshape(())


def pooled_loss(hp, hpt, fc_w, fc_b, ge, c, k, mult_natoms, graph_ptr):
    """sum_g ge_g E_g + c_g 2^k (D E)_g on pooled features: E_g = fc_w . hp_g + b, (D E)_g = fc_w . hpt_g (the tangent of an affine
    map drops the bias); c_g = c * atoms of g with energy_mult_natoms"""
    counts = (graph_ptr[1:] - graph_ptr[:-1]).to(hp.dtype)
    cg = c * (counts if mult_natoms else torch.ones_like(counts)) * 2.0 ** k
    loss = (cg * (hpt @ fc_w.reshape(-1))).sum()
    if ge is not None:
        loss = loss + (ge * (hp @ fc_w.reshape(-1) + fc_b.reshape(()))).sum()
    return loss


def readout_seeds(n_atoms, graph_ptr, fc_w, fc_b, ge, c, k, mult_natoms):
    """(gx, gxt): adjoints of the atom features and of their tangents (the loss is linear in both, so any x serves)"""
    H = fc_w.numel()
    x = torch.zeros(n_atoms, H, dtype=fc_w.dtype, requires_grad=True)
    xt = torch.zeros(n_atoms, H, dtype=fc_w.dtype, requires_grad=True)
    loss = pooled_loss(segment_mean(x, graph_ptr), segment_mean(xt, graph_ptr), fc_w, fc_b, ge, c, k, mult_natoms, graph_ptr)
    got = torch.autograd.grad(loss, (x, xt), allow_unused=True)  # (ge None: the loss does not depend on x)
    return tuple(torch.zeros_like(x) if g is None else g for g in got)


def fc_grad(hp, hpt, graph_ptr, fc_w, fc_b, ge, c, k, mult_natoms):
    """(gW [H], gb []): gradient of the same loss w.r.t. the readout's weight and bias"""
    w = fc_w.detach().clone().requires_grad_(True)
    b = fc_b.detach().clone().requires_grad_(True)
    loss = pooled_loss(hp, hpt, w, b, ge, c, k, mult_natoms, graph_ptr) + 0 * b.sum()  # (ge None: no bias in the loss)
    gw, gb = torch.autograd.grad(loss, (w, b))
    return gw.reshape(-1), gb.reshape(())


def featurisation(r, e1, e2, edge_centers, edge_gamma, angle_centers, angle_gamma):
    """(edge RBF of the bond lengths, angle RBF of the bond cosines): everything the model derives from the bond vectors"""
    return rbf(bond_length(r), edge_centers, edge_gamma), rbf(bond_cosine(r, e1, e2), angle_centers, angle_gamma)
