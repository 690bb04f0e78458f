"""The float64 restatements of tests/ff_head_ref.py, checked on their own (no GPU, no HIP library): central differences for
every gradient and tangent, one case by hand per operation on a batch small enough to write out, and the reference's goldens -
``h`` of the stored line graph, and energies / forces / stresses of the reference's own ALIGNNAtomWise."""

import math

import numpy as np
import pytest
import torch

from tests import ff_head_ref as R
from tests.helpers import load_golden, raw_from_golden, rel_err, state_dict_from_golden

D = torch.float64
T = lambda x: torch.tensor(x, dtype=D)  # noqa: E731
I = lambda x: torch.tensor(x, dtype=torch.int32)  # noqa: E731


def _central(fn, x, t, eps=1e-6):
    return (fn(x + eps * t) - fn(x - eps * t)) / (2 * eps)


def _gen(seed):
    return torch.Generator().manual_seed(seed)


# ----------------------------------------------------------------------------------------------------------------------
# central differences
# ----------------------------------------------------------------------------------------------------------------------
def _geometry(seed=0):
    g = _gen(seed)
    r = torch.randn(12, 3, generator=g, dtype=D) * 2
    e1 = torch.randint(0, 12, (40,), generator=g)
    e2 = torch.randint(0, 12, (40,), generator=g)
    keep = e1 != e2
    return r, e1[keep], e2[keep], torch.randn(12, 3, generator=g, dtype=D)


@pytest.mark.parametrize("name", ["bond_length", "bond_cosine", "rbf_edge", "rbf_angle"])
def test_jvp_and_gradient_match_central_differences(name):
    r, e1, e2, rt = _geometry()
    if name == "bond_length":
        fn, x, t = R.bond_length, r, rt
    elif name == "bond_cosine":
        fn, x, t = (lambda q: R.bond_cosine(q, e1, e2)), r, rt
    else:
        lo, hi, bins = (0.0, 8.0, 80) if name == "rbf_edge" else (-1.0, 1.0, 40)
        c = torch.linspace(lo, hi, bins, dtype=D)
        fn = lambda d: R.rbf(d, c, R.rbf_gamma(lo, hi, bins))  # noqa: E731
        x = lo + (hi - lo) * torch.rand(12, generator=_gen(1), dtype=D)
        t = torch.randn(12, generator=_gen(2), dtype=D)
    fd = _central(fn, x, t)
    jv = R.jvp_of(fn, (x,), (t,))
    assert rel_err(jv, fd) < 1e-8
    cot = torch.randn(fd.shape, generator=_gen(3), dtype=D)
    (gr,) = R.grad_of(fn, (x,), cot)
    assert abs(float((gr * t).sum() - (cot * fd).sum())) < 1e-7 * float((cot * fd).abs().sum())


def test_cosine_gradient_is_zero_outside_the_clamp_and_torch_includes_the_boundary():
    """torch's clamp passes the gradient where the input EQUALS a bound (inclusive mask): at c == 1 exactly the restated gradient
    is the unclamped formula's (which is 0 up to rounding for collinear vectors), not a masked 0"""
    x = torch.tensor([1.0, -1.0, 1.5, 0.3], dtype=D, requires_grad=True)
    torch.clamp(x, -1, 1).sum().backward()
    assert x.grad.tolist() == [1.0, 1.0, 0.0, 1.0]
    a = T([[1.0, 2.0, 2.0], [0.0, 3.0, 4.0]])
    ga, gb = R.grad_of(R.cosine_of_pairs, (a, -a), torch.ones(2, dtype=D))  # back-tracking pairs: c == 1
    assert float(ga.abs().max()) < 1e-15 and float(gb.abs().max()) < 1e-15
    assert R.cosine_of_pairs(a, -a).tolist() == [1.0, 1.0] and R.cosine_of_pairs(a, 3 * a).tolist() == [-1.0, -1.0]


def _head_batch(seed=5):
    """ragged batch: crystals of 3, 1 and 4 atoms, random bonds inside each crystal, sorted by destination atom"""
    g = _gen(seed)
    counts = [3, 1, 4]
    gp = I([0, 3, 4, 8])
    u, v = [], []
    for b, n in enumerate(counts):
        m = 5 * n
        u.append(torch.randint(0, n, (m,), generator=g) + int(gp[b]))
        v.append(torch.randint(0, n, (m,), generator=g) + int(gp[b]))
    u, v = torch.cat(u), torch.cat(v)
    order = torch.argsort(v, stable=True)
    u, v = u[order], v[order]
    seg_ptr = torch.zeros(9, dtype=torch.int32)
    seg_ptr[1:] = torch.cumsum(torch.bincount(v, minlength=8), 0)
    E = u.numel()
    r = torch.randn(E, 3, generator=g, dtype=D) * 1.5
    return dict(gp=gp, u=u, v=v, seg_ptr=seg_ptr, ep=R.edge_ptr_of(gp, seg_ptr), r=r, E=E, N=8, B=3,
                vol=T([30.0, 11.0, 52.5]), g=g)


def test_pair_weights_match_central_differences_of_the_force_and_stress_loss():
    h = _head_batch()
    g = h["g"]
    gF = torch.randn(h["N"], 3, generator=g, dtype=D)
    gS = torch.randn(h["B"], 3, 3, generator=g, dtype=D)
    kS = 0.7 * R.STRESS_UNIT
    for add_reverse in (False, True):
        w = R.pair_weights(gF, gS, h["r"], h["u"], h["v"], h["ep"], h["vol"], kS, add_reverse, h["N"], h["E"])
        loss = lambda f: ((gF * R.forces_of(f, h["u"], h["v"], h["N"], add_reverse)).sum()  # noqa: E731
                          + (gS * R.stresses_of(h["r"], f, h["ep"], h["vol"], kS)).sum())
        f0 = torch.randn(h["E"], 3, generator=g, dtype=D)
        t = torch.randn(h["E"], 3, generator=g, dtype=D)
        assert abs(float(_central(loss, f0, t, 1e-3) - (w * t).sum())) < 1e-9 * float((w * t).abs().sum())


def test_energy_seed_and_penalty_gradient_match_central_differences():
    h = _head_batch()
    g = h["g"]
    pred = torch.randn(h["B"], generator=g, dtype=D)
    bl = 0.5 + torch.rand(h["E"], generator=g, dtype=D)  # on both sides of the threshold 1.0, none within 1e-3 of it
    bl = torch.where((bl - 1.0).abs() < 1e-3, bl + 0.01, bl)
    for mult in (False, True):
        for pen in (False, True):
            tot = lambda p, b: R.energies(p, b, h["gp"], mult, pen, 0.1, 1.0)[1].sum()  # noqa: E731
            seed = R.energy_seed(pred, bl, h["gp"], mult, pen)
            tp = torch.randn(h["B"], generator=g, dtype=D)
            assert abs(float(_central(lambda p: tot(p, bl), pred, tp) - (seed * tp).sum())) < 1e-8
    gbl = R.penalty_grad(pred, bl, h["gp"], 0.1, 1.0)
    tb = torch.randn(h["E"], generator=g, dtype=D)
    fd = _central(lambda b: R.energies(pred, b, h["gp"], True, True, 0.1, 1.0)[1].sum(), bl, tb, 1e-5)
    assert abs(float(fd - (gbl * tb).sum())) < 1e-8


def test_tangent_geometry_and_readout_seeds_match_central_differences():
    h = _head_batch()
    g = h["g"]
    w = torch.randn(h["E"], 3, generator=g, dtype=D) * 37.0
    rt, dt, k = R.tangent_geometry(h["r"], w, w.abs().max())
    assert 2.0 ** k <= float(w.abs().max()) < 2.0 ** (k + 1) and torch.equal(rt * 2.0 ** k, w)
    assert rel_err(dt, _central(R.bond_length, h["r"], rt)) < 1e-8
    H = 8
    fc_w, fc_b = torch.randn(1, H, generator=g, dtype=D), torch.randn(1, generator=g, dtype=D)
    ge, c = torch.randn(h["B"], generator=g, dtype=D), -1.5
    x, xt = (torch.randn(h["N"], H, generator=g, dtype=D) for _ in range(2))
    for mult in (False, True):
        for ge_ in (None, ge):
            def loss(x_, xt_, w_=fc_w, b_=fc_b):
                return R.pooled_loss(R.segment_mean(x_, h["gp"]), R.segment_mean(xt_, h["gp"]), w_, b_, ge_, c, k, mult, h["gp"])
            gx, gxt = R.readout_seeds(h["N"], h["gp"], fc_w, fc_b, ge_, c, k, mult)
            tx = torch.randn(h["N"], H, generator=g, dtype=D)
            assert abs(float(_central(lambda q: loss(q, xt), x, tx) - (gx * tx).sum())) < 1e-7
            assert abs(float(_central(lambda q: loss(x, q), xt, tx) - (gxt * tx).sum())) < 1e-7 * 2.0 ** k
            hp, hpt = R.segment_mean(x, h["gp"]), R.segment_mean(xt, h["gp"])
            gW, gb = R.fc_grad(hp, hpt, h["gp"], fc_w, fc_b, ge_, c, k, mult)
            tw = torch.randn(1, H, generator=g, dtype=D)
            assert abs(float(_central(lambda q: loss(x, xt, w_=q), fc_w, tw) - (gW * tw.reshape(-1)).sum())) < 1e-7 * 2.0 ** k
            assert abs(float(_central(lambda q: loss(x, xt, b_=q), fc_b, torch.ones(1, dtype=D)) - gb)) < 1e-7


# ----------------------------------------------------------------------------------------------------------------------
# by hand: two crystals, A = atoms {0, 1} with bonds 0: 0->1, 1: 1->0, 2: 1->1 (a self image) and B = atom {2} with bond 3: 2->2
# ----------------------------------------------------------------------------------------------------------------------
SRC, DST = I([1, 0, 1, 2]), I([0, 1, 1, 2])  # sorted by destination: slot 0 = 1->0, slot 1 = 0->1, slot 2 = 1->1, slot 3 = 2->2
GP, SEG = I([0, 2, 3]), I([0, 1, 3, 4])
RV = T([[3.0, 0.0, 4.0], [-3.0, 0.0, -4.0], [0.0, 2.0, 0.0], [0.0, 0.0, 0.5]])


def test_by_hand_rbf_and_bond_length():
    d = R.bond_length(RV)
    assert d.tolist() == [5.0, 5.0, 2.0, 0.5]
    out = R.rbf(T([1.0, 0.5]), T([0.0, 1.0, 2.0]), 2.0)
    want = [[math.exp(-2.0), 1.0, math.exp(-2.0)], [math.exp(-0.5), math.exp(-0.5), math.exp(-4.5)]]
    assert rel_err(out, T(want)) < 1e-15
    assert R.rbf_gamma(0.0, 8.0, 80) == 9.875 and R.rbf_gamma(-1.0, 1.0, 40) == 19.5
    # d|r|/dr = r / |r|
    (g,) = R.grad_of(R.bond_length, (RV,), T([1.0, 2.0, 1.0, 1.0]))
    assert rel_err(g, T([[0.6, 0, 0.8], [-1.2, 0, -1.6], [0, 1, 0], [0, 0, 1]])) < 1e-15
    # d/dd exp(-gamma (d - c)^2) = -2 gamma (d - c) exp(.)
    (gd,) = R.grad_of(lambda q: R.rbf(q, T([0.0]), 2.0), (T([0.5]),), T([[1.0]]))
    assert abs(float(gd) - (-2.0 * math.exp(-0.5))) < 1e-15


def test_by_hand_bond_cosines():
    # triplets (e1 -> e2): 0 -> 1 back-tracking (r[1] == -r[0]): +1;  2 -> 0 with r1 = -(0,2,0), r2 = (3,0,4): 0;
    # 1 -> 2 with r1 = (3,0,4), r2 = (0,2,0): 0;  0 -> 0 (never in a line graph) straight through: -1
    h = R.bond_cosine(RV, I([0, 2, 1, 0]), I([1, 0, 2, 0]))
    assert h.tolist() == [1.0, 0.0, 0.0, -1.0]
    a, b = T([[1.0, 0.0, 0.0]]), T([[-1.0, 1.0, 0.0]])  # r1 = (-1,0,0)... c = -a.b / (|a||b|) = 1 / sqrt 2
    assert abs(float(R.cosine_of_pairs(a, b)) - 1 / math.sqrt(2)) < 1e-15
    # dc/db = -a/(|a||b|) - c b/|b|^2 = (-1,0,0)/sqrt2 - (1/sqrt2)(-1,1,0)/2 = (-1/2, -1/2, 0)/sqrt2
    _, gb = R.grad_of(R.cosine_of_pairs, (a, b), T([1.0]))
    assert rel_err(gb, T([[-0.5, -0.5, 0.0]]) / math.sqrt(2)) < 1e-15


def test_by_hand_pooling_sums_and_gather():
    x = T([[1.0, 2.0], [3.0, 6.0], [5.0, -1.0]])
    assert R.segment_mean(x, GP).tolist() == [[2.0, 4.0], [5.0, -1.0]]
    assert R.segment_mean(x, I([0, 0, 3])).tolist() == [[0.0, 0.0], [3.0, 7.0 / 3.0]]
    v = T([[1.0], [10.0], [100.0], [1000.0]])
    assert R.segment_sum(v, SEG).reshape(-1).tolist() == [1.0, 110.0, 1000.0]
    assert R.segment_sum(v, SEG, slot=I([3, 2, 1, 0])).reshape(-1).tolist() == [1000.0, 110.0, 1.0]
    assert R.segment_sum(v, SEG, node=I([2, 0, 1])).reshape(-1).tolist() == [110.0, 1000.0, 1.0]
    assert R.gather(x, I([2, 2, 0])).tolist() == [[5.0, -1.0], [5.0, -1.0], [1.0, 2.0]]
    (gx,) = R.grad_of(lambda q: R.segment_mean(q, GP), (x,), T([[2.0, 4.0], [1.0, 1.0]]))
    assert gx.tolist() == [[1.0, 2.0], [1.0, 2.0], [1.0, 1.0]]


def test_by_hand_head():
    pred = T([2.0, -1.0])
    bl = R.bond_length(RV)  # 5, 5, 2, 0.5: one bond below the threshold 1.0 -> penalty 0.1 * 0.5 = 0.05
    out, en = R.energies(pred, bl, GP, True, True, 0.1, 1.0)
    assert out.tolist() == [2.0, -1.0] and rel_err(en, T([4.05, -0.95])) < 1e-15
    out, en = R.energies(pred, bl, GP, False, True, 0.1, 1.0)
    assert rel_err(out, T([2.05, -0.95])) < 1e-15 and torch.equal(out, en)
    out, en = R.energies(pred, T([5.0, 5.0, 2.0, 1.0]), GP, False, True, 0.1, 1.0)  # exactly on the threshold: no penalty
    assert out.tolist() == [2.0, -1.0]
    assert R.energy_seed(pred, bl, GP, True, True).tolist() == [2.0, 1.0] and R.energy_seed(pred, bl, GP, False, False).tolist() == [1.0, 1.0]
    assert rel_err(R.penalty_grad(pred, bl, GP, 0.1, 1.0), T([0.0, 0.0, 0.0, -0.2])) < 1e-15  # both energies carry it
    pf = T([[1.0, 0, 0], [0, 2.0, 0], [0, 0, 4.0], [8.0, 8.0, 8.0]])
    # atom 0: in {0}, out {1};  atom 1: in {1, 2}, out {0, 2};  atom 2: in {3}, out {3}
    assert R.forces_of(pf, SRC, DST, 3, True).tolist() == [[1.0, -2.0, 0.0], [-1.0, 2.0, 0.0], [0.0, 0.0, 0.0]]
    assert R.forces_of(pf, SRC, DST, 3, False).tolist() == [[1.0, 0.0, 0.0], [0.0, 2.0, 4.0], [8.0, 8.0, 8.0]]
    ep = R.edge_ptr_of(GP, SEG)
    assert ep.tolist() == [0, 3, 4]
    s = R.stresses_of(RV, pf, ep, T([2.0, 0.5]), k=-1.0)
    # crystal A: r0 (x) pf0 + r1 (x) pf1 + r2 (x) pf2 = [[3,0,0],[0,0,0],[4,0,0]] + [[0,-6,0],[0,0,0],[0,-8,0]] + [[0,0,0],[0,0,8],[0,0,0]]
    assert s[0].tolist() == [[-1.5, 3.0, 0.0], [0.0, 0.0, -4.0], [-2.0, 4.0, 0.0]]
    assert s[1].tolist() == [[0.0, 0.0, 0.0], [0.0, 0.0, 0.0], [-8.0, -8.0, -8.0]]


def test_by_hand_second_order_seeds():
    gF = T([[1.0, 0, 0], [0, 1.0, 0], [0, 0, 1.0]])
    w = R.pair_weights(gF, None, None, SRC, DST, None, None, 0.0, True, 3, 4)  # gF[dst] - gF[src]
    assert w.tolist() == [[1.0, -1.0, 0.0], [-1.0, 1.0, 0.0], [0.0, 0.0, 0.0], [0.0, 0.0, 0.0]]
    gS = torch.zeros(2, 3, 3, dtype=D)
    gS[1, 0, 2] = 1.0  # dL/dS_B[x, z]: w_3 = k / V_B * r_3[x] along z ... = gS^T r
    gS[0, 1, 0] = 2.0
    w = R.pair_weights(None, gS, RV, SRC, DST, I([0, 3, 4]), T([2.0, 0.5]), -1.0, True, 3, 4)
    assert w.tolist() == [[0.0, 0.0, 0.0], [0.0, 0.0, 0.0], [-2.0, 0.0, 0.0], [0.0, 0.0, 0.0]]  # r_2[y] = 2, r_3[x] = 0
    assert [R.pow2_exponent(v) for v in (8.0, 7.999, 0.0, 2.0 ** -100, 2.0 ** 100, 1.0)] == [3, 2, 0, -100, 100, 0]
    rt, dt, k = R.tangent_geometry(RV, T([[8.0, 0, 0], [0, 0, 4.0], [0, 2.0, 0], [0, 0, 0]]), 8.0)
    assert k == 3 and rt[0].tolist() == [1.0, 0.0, 0.0] and rel_err(dt, T([0.6, -0.4, 0.25, 0.0])) < 1e-15  # r . rt / |r|
    fc_w, fc_b = T([[1.0, -2.0]]), T([0.5])
    assert R.readout(T([[1.0, 2.0], [3.0, 6.0], [5.0, -1.0]]), GP, fc_w, fc_b).tolist() == [-5.5, 7.5]
    gx, gxt = R.readout_seeds(3, GP, fc_w, fc_b, T([4.0, 3.0]), -1.0, 3, True)
    # value seed ge_g / n_g * fc_w; tangent seed c * n_g * 2^k / n_g * fc_w = -8 fc_w
    assert gx.tolist() == [[2.0, -4.0], [2.0, -4.0], [3.0, -6.0]] and gxt.tolist() == [[-8.0, 16.0]] * 3
    gx, gxt = R.readout_seeds(3, GP, fc_w, fc_b, None, -1.0, 3, False)
    assert gx.abs().max() == 0 and gxt.tolist() == [[-4.0, 8.0], [-4.0, 8.0], [-8.0, 16.0]]
    hp, hpt = T([[1.0, 0.0], [0.0, 1.0]]), T([[0.0, 1.0], [1.0, 1.0]])
    gW, gb = R.fc_grad(hp, hpt, GP, fc_w, fc_b, T([4.0, 3.0]), -1.0, 3, True)
    # 4 hp_A + 3 hp_B + (-1 * 2 * 8) hpt_A + (-1 * 1 * 8) hpt_B
    assert gW.tolist() == [4.0 - 8.0, 3.0 - 16.0 - 8.0] and float(gb) == 7.0


# ----------------------------------------------------------------------------------------------------------------------
# the reference's goldens
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["atomwise_ff_tiny.npz", "alignn_tiny_train.npz"])
def test_cosine_restatement_reproduces_the_golden_line_graph(name):
    z = load_golden(name)
    r = torch.from_numpy(z["in.r"])
    e1, e2 = torch.from_numpy(z["in.lg_u"]), torch.from_numpy(z["in.lg_v"])
    want = torch.from_numpy(z["in.h"]).double()
    # the golden holds float32 arithmetic on the same float32 r: 3 products, 2 sums, 2 norms, a product and a quotient, each within
    # half an ulp of a number <= 1 (2^-24): 8 * 2^-24 = 4.8e-7 bounds its distance from float64, and from float32 in another order
    assert float((R.bond_cosine(r.double(), e1, e2) - want).abs().max()) < 4.8e-7
    assert float((R.bond_cosine(r, e1, e2).double() - want).abs().max()) < 4.8e-7


def test_head_restatement_reproduces_the_golden_energies_forces_and_stresses():
    """atomwise_ff_tiny.npz stores no pair forces, so they come from the model: dE/dr of the oracle's conv stack (pinned to the
    reference's class by tests/test_oracle_golden.py), run in float64, through the RESTATED energies (natoms factor + penalty)."""
    from oracle import alignn_oracle as O

    z = load_golden("atomwise_ff_tiny.npz")
    raw = raw_from_golden(z)
    p = O.as_params(state_dict_from_golden(z), D)
    graph = O.TorchGraph(raw)
    r = graph.r.double().requires_grad_(True)
    graph.r = r
    pred = O.alignn_atomwise_forward(p, graph, int(z["cfg.alignn_layers"]), int(z["cfg.gcn_layers"]), True)
    bnn = torch.from_numpy(raw.batch_num_nodes)
    gp = torch.zeros(bnn.numel() + 1, dtype=torch.int64)
    gp[1:] = torch.cumsum(bnn, 0)
    out, en_out = R.energies(pred, R.bond_length(r), gp, True, True, 0.1, 1.0)
    assert rel_err(out, z["pred"]) < 2e-5
    pf = -1.0 * torch.autograd.grad(en_out.sum(), r)[0]  # grad_multiplier = -1
    forces = R.forces_of(pf, graph.u, graph.v, raw.num_nodes, True)
    assert rel_err(forces, z["forces"]) < 1e-4
    ep = torch.zeros(bnn.numel() + 1, dtype=torch.int64)
    ep[1:] = torch.cumsum(torch.from_numpy(raw.batch_num_edges), 0)
    stresses = R.stresses_of(r.detach(), pf, ep, torch.from_numpy(z["volume"]).double())
    assert rel_err(stresses, z["stresses"]) < 1e-4
    # the stress is built from the SCALED pair forces and each crystal's own volume: neither may be swapped
    assert rel_err(R.stresses_of(r.detach(), pf, ep, torch.from_numpy(z["volume"]).double().flip(0)), z["stresses"]) > 1e-2
    assert np.abs(z["volume"][0] - z["volume"][1]) > 1e-3
