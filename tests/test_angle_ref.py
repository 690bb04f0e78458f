"""tests/angle_ref.py itself, before csrc/angle.hip is measured against it (tests/test_gpu_angle_f64.py): in float64 the
restatement is autograd through RBFExpansion and two MLPLayer modules - z, the running statistics, the gradients of all eight
parameter tensors, evaluation mode -, every distribution is what it says, no float64 output is non-finite, and every
distribution is well enough conditioned for a float32 kernel to be judged on it: the float32 restatement, the yardstick of
the GPU test, stays within CAP = 1e-2 of float64 on every output (a yardstick that is further off proves nothing)."""

import pytest
import torch

from alignn_amd.alignn import MLPLayer, RBFExpansion
from tests import angle_ref as ref

CAP = 1e-2
D = torch.float64


def err(a, b, floor=1e-30):
    a, b = a.detach().double(), b.detach().double()
    return float((a - b).abs().max() / b.abs().max().clamp_min(floor))


def same(a, b, floor, terms):
    """1e-12 relative, or - where the terms cancel (beta_heavy's dW2: mean(a1) = 300 std(a1)) - within 1e-14 of the sum of
    the terms' magnitudes, which is what two float64 summation orders may differ by"""
    return err(a, b, floor) < 1e-12 or float((a.detach() - b.detach()).abs().max()) <= 1e-14 * float(terms.max())


def _modules(o):
    """the chain of modules in float64 holding the operands"""
    bins = o["centers"].numel()
    rbf = RBFExpansion(vmin=-1.0, vmax=1.0, bins=max(bins, 2))
    rbf.centers, rbf.gamma = o["centers"].clone(), o["gamma"]
    layers = []
    for k, (fin, fout) in (("1", (bins, ref.E1)), ("2", (ref.E1, ref.E2))):
        m = MLPLayer(fin, fout).double()
        with torch.no_grad():
            for dst, src in ((m.layer[0].weight, "W"), (m.layer[0].bias, "b"), (m.layer[1].weight, "g"), (m.layer[1].bias, "be"),
                             (m.layer[1].running_mean, "rm"), (m.layer[1].running_var, "rv")):
                dst.copy_(o[src + k])
        layers.append(m)
    return rbf, layers[0], layers[1]


@pytest.mark.parametrize("rows,bins", [(2, 17), (257, 40)])
@pytest.mark.parametrize("data", ref.DATA)
def test_restatement_is_autograd_through_the_modules(data, rows, bins):
    o = ref.operands(rows, bins, data)
    rbf, l1, l2 = _modules(o)
    l1.train(), l2.train()
    z = l2(l1(rbf(o["h"].double())))
    z.backward(o["gz"].double())
    f = ref.forward(o)
    b = ref.backward(o, f)
    fl = ref.floors(b, rows, data)
    assert all(bool(torch.isfinite(v).all()) for v in list(f.values()) + list(b.values()))
    assert err(f["z"], z) < 1e-12 and float(f["zmax"]) == float(f["z"].abs().max())
    for k, m in (("1", l1), ("2", l2)):
        lin, bn = m.layer[0], m.layer[1]
        assert err(f["rm" + k], bn.running_mean) < 1e-12 and err(f["rv" + k], bn.running_var) < 1e-12
        assert torch.equal(f["stat" + k][3], o["be" + k].double())
        assert err(f["stat" + k][2], o["g" + k].double() * f["stat" + k][1], 1e-300) < 1e-15
        assert same(b["gW" + k], lin.weight.grad, fl.get("gW" + k, 1e-30), b["t_gW" + k]), (k, "gW")
        assert same(b["red" + k][0], bn.bias.grad, fl.get(f"red{k}/dbeta", 1e-30), b["t_red" + k][0]), (k, "dbeta")
        assert same(b["red" + k][1], bn.weight.grad, fl.get(f"red{k}/dgamma", 1e-30), b["t_red" + k][1]), (k, "dgamma")
        # Linear bias in front of BatchNorm: zero but for the rounding of its terms, on both sides
        scale = float(b["t_gW" + k].max())
        assert float(b["gb" + k].abs().max()) <= 1e-12 * scale and float(lin.bias.grad.abs().max()) <= 1e-12 * scale
    if data == "gz_zero":
        assert not any(bool(b[k].any()) for k in ("red1", "red2", "gW1", "gW2", "gb1", "gb2"))
    # evaluation mode, from the statistics the training step left and from the operands' own
    l1.eval(), l2.eval()
    with torch.no_grad():
        assert err(ref.infer(o, D, (f["rm1"], f["rv1"], f["rm2"], f["rv2"])), l2(l1(rbf(o["h"].double())))) < 1e-12
        _, e1, e2 = _modules(o)
        assert err(ref.infer(o), e2.eval()(e1.eval()(rbf(o["h"].double())))) < 1e-12


def test_one_row_in_training_mode_is_silu_of_beta():
    """torch refuses one row in training mode; the kernel does not: var = 0, z = silu(beta2), the biased running variance"""
    o = ref.operands(1, 40, "normal")
    f = ref.forward(o)
    assert err(f["z"][0], torch.nn.functional.silu(o["be2"].double())) < 1e-15
    assert not bool(f["var1"].any()) and not bool(f["var2"].any())
    assert err(f["rv1"], 0.9 * o["rv1"].double()) < 1e-15 and err(f["rm2"], 0.9 * o["rm2"].double() + 0.1 * f["x2"][0]) < 1e-15
    b = ref.backward(o, f)
    assert err(b["red2"][0], o["gz"][0].double() * ref.dsilu(o["be2"].double())) < 1e-15
    assert float(b["gW2"].abs().max()) <= 1e-15 * float(b["t_gW2"].max())


def cap_errors(rows, bins, data):
    """{output: error of the float32 restatement against float64} over everything the GPU test compares on ``data``"""
    o = ref.operands(rows, bins, data)
    f64, f32 = ref.forward(o), ref.forward(o, torch.float32)
    b64, b32 = ref.backward(o, f64), ref.backward(o, f32)
    fl = ref.floors(b64, rows, data)
    out = {"z": err(f32["z"], f64["z"]), "infer z": err(ref.infer(o, torch.float32), ref.infer(o))}
    for k in ("1", "2"):
        for i, name in enumerate(("mean", "rstd", "scale")):
            out[f"stat{k} {name}"] = err(f32["stat" + k][i], f64["stat" + k][i])
        out["rm" + k], out["rv" + k] = err(f32["rm" + k], f64["rm" + k]), err(f32["rv" + k], f64["rv" + k])
        out["gW" + k] = err(b32["gW" + k], b64["gW" + k], fl.get("gW" + k, 1e-30))
        for i, name in enumerate(("dbeta", "dgamma")):
            out[f"red{k} {name}"] = err(b32["red" + k][i], b64["red" + k][i], fl.get(f"red{k}/{name}", 1e-30))
    return out


@pytest.mark.parametrize("data", ref.DATA)
def test_every_distribution_is_within_the_conditioning_cap(data):
    """rows 2049, bins 40.  ``gz_zero`` has nothing to be relative to: its gradients are exact zeros on both sides."""
    errors = cap_errors(2049, 40, data)
    for k, e in errors.items():
        print(f"angle-cap {data:<12s} {k:<14s} float32 {e:8.2e}")
    bad = {k: e for k, e in errors.items() if not e < CAP}
    assert not bad, bad


def test_the_distributions_are_what_they_say():
    rows, bins = 2049, 40
    o = ref.operands(rows, bins, "lattice")
    assert set(o["h"].tolist()) == {-1.0, -0.5, 0.0, 0.5, 1.0}
    o = ref.operands(rows, bins, "row0_outlier")
    assert float(o["h"][0]) == -1.0 and float((o["h"][1:] - 0.5).abs().max()) <= 1.0001e-3
    f = ref.forward(o)
    # the outlier IS the variance: sums shifted by x1(h[0]) hold q / n = (mean - x1[0])^2 = rows var - q / n - dm^2 cancels by `rows`
    ratio = (f["stat1"][0] - f["x1"][0]) ** 2 / f["var1"]
    assert float(ratio.median()) > 0.9 * rows, float(ratio.median())
    # and the cluster's own variance is small against E[x^2]
    assert float((f["var1"] / (f["x1"] ** 2).mean(0)).median()) < 1e-3
    o = ref.operands(rows, bins, "constant")
    f = ref.forward(o)
    assert bool((o["h"] == o["h"][0]).all())
    assert float(f["var1"].max()) < 1e-28 and err(f["stat1"][1], torch.full((ref.E1,), ref.EPS ** -0.5, dtype=D)) < 1e-12
    o = ref.operands(rows, bins, "beta_heavy")
    f = ref.forward(o)
    assert 0.01 <= float(o["g1"].abs().min()) and float(o["g1"].abs().max()) <= 0.02
    assert 3 <= float(o["be1"].abs().min()) and float(o["be1"].abs().max()) <= 5
    a1 = f["a1"]
    big = o["be1"] > 0  # (silu(-4) is itself small: the features with beta > 0 are the ones whose mean dwarfs their spread)
    assert float((a1.mean(0).abs() / a1.std(0))[big].min()) > 100
    o = ref.operands(rows, bins, "gamma_zero")
    assert not bool(o["g1"][::4].any()) and not bool(o["g2"][::4].any()) and bool(o["g1"][1::4].all())
    base = ref.operands(rows, bins, "normal")
    for name, key, s in (("w_tiny", "W1", 2.0 ** -20), ("w_huge", "W2", 2.0 ** 10), ("gz_tiny", "gz", 2.0 ** -40), ("gz_huge", "gz", 2.0 ** 20)):
        o = ref.operands(rows, bins, name)
        assert 0.2 * s < float(o[key].abs().max()) / float(base[key].abs().max()) < 5 * s
    o = ref.operands(rows, bins, "gz_columns")
    col = o["gz"].abs().max(0).values
    assert 2.0 ** -14 < float(col[-1] / col[0]) < 2.0 ** -10
    assert not bool(ref.operands(rows, bins, "gz_zero")["gz"].any())
