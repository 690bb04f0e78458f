"""tests/dual_ref.py, the restatements tests/test_gpu_dual_f64.py and tests/test_gpu_convln.py hold the HIP kernels to, checked on
the CPU: the explicit tangents are the directional derivative, the values are those of ``layer_norm`` / ``silu`` /
``index_add``, and on every case of the GPU test that can be built without a GPU the float32 restatement stays within 1e-4 of
float64 on every output (the conditioning cap: see the docstring of tests/dual_ref.py, which records what is measured here)."""

import pytest
import torch
import torch.nn.functional as F

from tests import dual_ref as D
from tests.gate_parity import err, graph

CAP = 1e-4  # the north-star bar of BASELINE.json
CPU_GRAPHS = ("synthetic", "lg_small", "lg_deg17", "one_atom_cell", "one_segment", "no_edges")


def _index(g):
    return g.src.long(), g.dst.long(), g.n_nodes


@pytest.mark.parametrize("H,gname,data", [(36, "lg_small", "normal"), (64, "synthetic", "normal"), (260, "one_atom_cell", "normal")])
def test_the_restatements_are_consistent(H, gname, data):
    """Same values as the layer_norm / silu / index_add restatement (1e-12) and tangents that ARE the directional derivative
    (central differences with h = 1e-6, the tolerances of tests/test_gpu_convln.py::test_the_restatements_are_consistent)."""
    g = graph(gname, "cpu")
    u, v, n = _index(g)
    c = {k: t.double() for k, t in D.operands(H, g, data, "cpu").items()}
    args = (c["gamma"], c["beta"], u, v, n, H)
    d = D._duals(c["P"], c["Pt"], c["M"], c["Mt"], *args)
    f = D._values(c["P"], c["M"], *args)
    for k in ("y", "s1", "s0", "hh", "xpre"):
        assert err(d[k], f[k]) < 1e-12, k
    y, yt, mean, rstd = D.ln_dual(c["M"], c["Mt"], c["R"], c["Rt"], c["gamma"], c["beta"])
    assert err(y, F.silu(F.layer_norm(c["M"], (H,), c["gamma"], c["beta"], D.EPS)) + c["R"]) < 1e-12
    assert err(mean, f["mean"]) < 1e-12 and err(rstd, f["rstd"]) < 1e-12
    assert err(yt, d["yt"] + c["Rt"]) < 1e-12
    h = 1e-6
    fp, fm = (D._values(c["P"] + s * h * c["Pt"], c["M"] + s * h * c["Mt"], *args) for s in (1, -1))
    for k, kt, tol in (("y", "yt", 1e-7), ("s1", "s1t", 1e-7), ("s0", "s0t", 1e-7), ("hh", "hht", 1e-6), ("xpre", "xpre_t", 1e-6)):
        assert err(d[kt], (fp[k] - fm[k]) / (2 * h)) < tol, kt
    # from C, Ct: m = A[u] + Bd[v] + C is M up to the rounding of the float32 operands, mt the derivative of m
    A, Bd, _, _ = D._blocks(c["P"], H)
    w = D.gate_dual(c["P"], c["Pt"], c["C"], c["Ct"], False, u, v, n, H)
    assert err(w["m"], A[u] + Bd[v] + c["C"]) < 1e-12 and err(w["m"], c["M"]) < 1e-6
    wp, wm = (D.gate_dual(c["P"] + s * h * c["Pt"], c["Pt"], c["C"] + s * h * c["Ct"], c["Ct"], False, u, v, n, H) for s in (1, -1))
    for k, kt, tol in (("m", "mt", 1e-7), ("s0", "s0t", 1e-7), ("xpre", "xpre_t", 1e-6)):
        assert err(w[kt], (wp[k] - wm[k]) / (2 * h)) < tol, kt


def test_the_quotient_reverse_is_the_adjoint_of_the_quotient():
    """<Q, perturbation of the sums> equals <g, perturbation of (hh, hht)> to first order (central differences)."""
    gen = torch.Generator().manual_seed(1)
    R = lambda: torch.randn(7, 12, generator=gen, dtype=torch.float64)  # noqa: E731
    s0, s1, s0t, s1t, g, gt = R().abs() + 0.1, R(), R(), R(), R(), R()
    quot = lambda a1, a0, b1, b0: (a1 / (a0 + D.EPS_GATE), (b1 - a1 / (a0 + D.EPS_GATE) * b0) / (a0 + D.EPS_GATE))  # noqa: E731
    hh, hht = quot(s1, s0, s1t, s0t)
    q = D.node_quotient_reverse(torch.float64, g, gt, s0, hh, s0t, hht)
    d = [R() for _ in range(4)]
    e = 1e-6
    (hp, htp), (hm, htm) = (quot(s1 + s * e * d[0], s0 + s * e * d[1], s1t + s * e * d[2], s0t + s * e * d[3]) for s in (1, -1))
    lhs = sum(float((q[k] * dk).sum()) for k, dk in zip(("Q1", "Q0", "Q1t", "Q0t"), d))
    rhs = float((g * (hp - hm)).sum() + (gt * (htp - htm)).sum()) / (2 * e)
    assert abs(lhs - rhs) < 1e-6 * max(abs(rhs), 1.0)


def gate_cap_errors(H, gname, data):
    """{output: error of the float32 restatement against float64}, measured as tests/test_gpu_dual_f64.py measures the kernels"""
    g = graph(gname, "cpu")
    u, v, n = _index(g)
    o = D.operands(H, g, data, "cpu")
    r64 = D.gate_case(torch.float64, o, u, v, n, H)
    r32 = D.gate_case(torch.float32, o, u, v, n, H, r64["handed"])
    out = {}
    if g.n_edges == 0:
        return {k: err(r32[k], r64[k]) for k in r64 if k != "handed" and r64[k].numel() and r64[k].shape[0] == n}
    for k in r64:
        if k.endswith("_stat"):  # (mean and rstd each on its own scale)
            out[k[:2] + "mean"], out[k[:2] + "rstd"] = (err(r32[k][:, j], r64[k][:, j]) for j in (0, 1))
        elif k != "handed" and k.split("_")[-1] not in D.REVERSE_FLOORED and k[0] != "Q":
            out[k] = err(r32[k], r64[k])
    for sfx, em, nm in D.reverse_parts(data, n, v):
        for k in ("Q1", "Q0", "Q1t", "Q0t"):
            out[k + sfx] = err(D.part(r32[k], nm), D.part(r64[k], nm))
        for tag in ("gl_", "nogl_"):
            fl = D.reverse_floors(r64, tag, nm)
            for k in ("GM", "GMt"):
                out[tag + k + sfx] = err(D.part(r32[tag + k], em), D.part(r64[tag + k], em), fl[k])
            for k in ("GP", "GPt"):
                out[tag + k + sfx] = err(D.part(r32[tag + k], nm), D.part(r64[tag + k], nm), fl[k])
            if sfx != " sat":
                out[tag + "gb"] = err(r32[tag + "gb"], r64[tag + "gb"], fl["gb"])
    return out


def row_cap_errors(rows, Fw, data):
    o = D.row_operands(rows, Fw, data, "cpu")
    out = {}
    for res in (False, True):
        r64, r32 = D.row_case(torch.float64, o, res), D.row_case(torch.float32, o, res)
        out.update({k: max(out.get(k, 0.0), err(r32[k], r64[k])) for k in r64})
    return out


@pytest.mark.parametrize("H,gname,data", [c for c in D.GATE_CASES if c[1] in CPU_GRAPHS])
def test_float32_gate_restatement_stays_within_the_cap(H, gname, data):
    errs = gate_cap_errors(H, gname, data)
    print(f"dual-ref-cap H={H} {gname} {data}: worst {max(errs.values()):.2e} ({max(errs, key=errs.get)})")
    assert all(e < CAP for e in errs.values()), {k: e for k, e in errs.items() if not e < CAP}


@pytest.mark.parametrize("rows,Fw,data", [c for c in D.ROW_CASES if c[2] != "normal" or c[0] <= 5 or c[1] == 64])
def test_float32_row_restatement_stays_within_the_cap(rows, Fw, data):
    errs = row_cap_errors(rows, Fw, data)
    print(f"dual-ref-cap rows={rows} F={Fw} {data}: worst {max(errs.values()):.2e} ({max(errs, key=errs.get)})")
    assert all(e < CAP for e in errs.values()), {k: e for k, e in errs.items() if not e < CAP}


def test_constant_rows_are_refused_off_the_exact_widths():
    with pytest.raises(AssertionError):
        D.row_operands(5, 260, "constant_rows", "cpu")
