"""One whole training step of the per-operator path with every activation, gradient, tape tensor and scratch block between
guard bands (tests/gate_parity.Guards): the extents of what alignn_amd/ops.py and alignn_amd/ff2.py allocate, as the kernels
are really called - where tests/test_gpu_conv_bn.py, test_gpu_convln.py and test_gpu_dual_f64.py check them entry point by
entry point on buffers of the test's own sizing.

``ops._empty`` (and its twin ``ff2._empty`` of the dual-number path) is the one allocator of that path and ``ops._scratch`` the
one of the composite calls' scratch blocks, which are then exactly alignn_egc_conv_{fwd,bwd,wgrad}_scratch bytes long; pytest's
monkeypatch substitutes an allocator that hands out guarded payloads and keeps the base buffers alive.  After the step every
guard is checked bit for bit, and the loss and every parameter gradient must EQUAL those of the same step on plain allocations:
guards must not change what runs, and a kernel that read a guard (or an element nobody wrote - unwritten payload holds the
guard's NaN, not torch.empty's leftovers) would show there.

Scope.  Parameters, graph tables, weight images, the amax arena and whatever torch itself allocates (zeros_like, clone) are the
caller's tensors and are not guarded here.  The whole-model C path (alignn_amd/cmodel.py) carves one arena, so its interior
extents are invisible to guards: it is switched off (ALIGNN_AMD_CMODEL=0).  Blind spots of the instrument: an access farther
away than the guard (1024 elements or two rows), and a read that is fetched but never used."""

import sys

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from alignn_amd import ALIGNN, ALIGNNAtomWise, ALIGNNAtomWiseConfig, ALIGNNConfig, GraphBatch, cmodel, ff2, ops  # noqa: E402
from alignn_amd.synthetic import _one, batch_raw, make_batch  # noqa: E402
from tests.gate_parity import NAN_BITS, Report  # noqa: E402

DEV = "cuda"
# the smallest batch on either side of the dispatch thresholds of ops.py, and a one-atom cell (self-image segments: the
# excluded row of the dense line-graph kernels)
BATCHES = {"3x14": lambda: make_batch(3, 14, seed0=31), "16x60": lambda: make_batch(16, 60, seed0=3),
           "one_atom_cell": lambda: batch_raw([_one(k, 60 + i, "crystal", 92) for i, k in enumerate((1, 6, 2))])}
STATS = ("COMPOSITE_STATS", "DW_STATS", "BNRED_STATS", "BD_TABLE_STATS")


def _alignn_step(batch, raw):
    torch.manual_seed(0)
    # hidden 256: the N of the thresholds; two line-graph layers: the second one's edge input comes out of a BatchNorm (bnred)
    model = ALIGNN(ALIGNNConfig(name="alignn", alignn_layers=2, gcn_layers=1)).to(DEV).train()
    target = torch.randn(raw.batch_size, generator=torch.Generator().manual_seed(2)).to(DEV)
    loss = F.l1_loss(model(batch), target)
    loss.backward()
    return model, loss


def _atomwise_step(batch, raw):
    torch.manual_seed(7)
    cfg = ALIGNNAtomWiseConfig(name="alignn_atomwise", alignn_layers=1, gcn_layers=1, hidden_features=256, atom_input_features=92,
                               calculate_gradient=True, stresswise_weight=0.05)
    model = ALIGNNAtomWise(cfg).to(DEV).train()
    gen, B = torch.Generator().manual_seed(4), raw.batch_size
    te, tf, ts = (torch.randn(B, generator=gen).to(DEV), torch.randn(raw.num_nodes, 3, generator=gen).to(DEV),
                  torch.randn(B, 3, 3, generator=gen).to(DEV))
    res = model(batch)
    loss = F.l1_loss(res["out"], te) + F.l1_loss(res["grad"], tf) + 0.05 * F.l1_loss(res["stresses"], ts)
    loss.backward()
    return model, loss


def _run(monkeypatch, step, batch, raw, composite, rep=None):
    """one forward and backward on the per-operator path; with ``rep`` every ops / ff2 allocation inside its guards"""
    with monkeypatch.context() as mp:
        mp.setenv("ALIGNN_AMD_CMODEL", "0")
        mp.setattr(cmodel, "ENABLED", False)
        mp.setattr(ops, "COMPOSITE", composite)
        # labels of the f16x3 products the host launches - on the per-kernel path only: an armed timer switches the composite off
        mp.setattr(ops, "KERNEL_TIMER", None if composite else {"min_rows": 0, "events": []})
        mp.setitem(ops._SIDE, "streams", {})
        for name in STATS:
            mp.setattr(ops, name, dict.fromkeys(getattr(ops, name), 0))
        n_scratch = [0]
        if rep is not None:
            def where():
                f = sys._getframe(2)
                return f"{f.f_code.co_filename.rsplit('/', 1)[-1]}:{f.f_lineno} {f.f_code.co_name}"

            def empty(*shape, like):
                return rep.guards.guarded(shape, torch.float32, None, where(), like.device)

            def scratch(nbytes, like):
                n_scratch[0] += 1
                return rep.guards.guarded((nbytes // 4,), torch.float32, None, "scratch of " + where(), like.device)

            mp.setattr(ops, "_empty", empty)
            mp.setattr(ff2, "_empty", empty)
            mp.setattr(ops, "_scratch", scratch)
        model, loss = step(batch, raw)
        torch.cuda.synchronize()
        out = {"loss": loss.detach().clone()}
        out.update({k: p.grad.clone() for k, p in model.named_parameters() if p.grad is not None})
        seen = {name: dict(getattr(ops, name)) for name in STATS}
        seen.update(labels=None if composite else {e[0] for e in ops.KERNEL_TIMER["events"]}, side=len(ops._SIDE["streams"]), scratch=n_scratch[0])
        return out, seen


@pytest.mark.parametrize("composite", [True, False], ids=["composite", "per_kernel"])
@pytest.mark.parametrize("bname", list(BATCHES))
@pytest.mark.parametrize("flavour", ["alignn_bn", "atomwise_ln_dual"])
def test_a_training_step_stays_inside_its_buffers(monkeypatch, flavour, bname, composite):
    """ALIGNN (BatchNorm) and ALIGNNAtomWise with calculate_gradient=True (LayerNorm, the dual-number path), ops.COMPOSITE on and
    off: no guard of any allocation changes, and the guarded step gives the plain step's loss and gradients bit for bit.
    ``3x14`` and ``one_atom_cell``: no product reaches X6_MIN_TILES, every one is fp32.  ``16x60`` (about 169 000 triplet rows): above
    X6_MIN_TILES, DW_MIN_ROWS and the side stream's min_rows - the f16x3 gather with its statistics epilogue, the bnred epilogue,
    gemm_dw and (BatchNorm flavour) the side stream all run, which the counters below assert."""
    step = _alignn_step if flavour == "alignn_bn" else _atomwise_step
    raw = BATCHES[bname]()
    batch = GraphBatch.from_raw(raw, device=DEV)
    plain, seen_plain = _run(monkeypatch, step, batch, raw, composite)
    rep = Report(f"{flavour} {bname} {'composite' if composite else 'per-kernel'}", "conv-extents")
    inside, seen = _run(monkeypatch, step, batch, raw, composite, rep)
    print("conv-extents", rep.case, seen)
    assert {k: v for k, v in seen.items() if k != "scratch"} == {k: v for k, v in seen_plain.items() if k != "scratch"}
    assert len(rep.guards.bufs) > 20
    # ---- the dispatch this batch is here for
    big, bn = bname == "16x60", flavour == "alignn_bn"
    lg_rows = batch.lg.n_edges
    if big:
        assert lg_rows >= max(ops.DW_MIN_ROWS, ops._SIDE["min_rows"], 64 * ops.X6_MIN_TILES) and seen["side"] == int(bn)
    else:
        # (6978 and 2090 triplet rows: 3x14 is past ops.AMAX_MIN_ROWS, so maxima are tracked, but no product reaches X6_MIN_TILES)
        assert lg_rows < 64 * ops.X6_MIN_TILES and not seen["labels"] and seen["DW_STATS"]["fused"] == 0 and seen["side"] == 0
    if bn:
        n_conv, c = 5, seen["COMPOSITE_STATS"]
        dw = seen["DW_STATS"]["fused"]
        assert dw == (2 if big else 0)  # (the line-graph convolution's edge-gate reverse: csrc/gemm_dw.hip; the composite declines)
        assert c == ({"fwd": n_conv, "bwd": n_conv - dw, "wgrad": n_conv - dw} if composite else {"fwd": 0, "bwd": 0, "wgrad": 0})
        assert seen["scratch"] == sum(c.values())
        if big:
            assert seen["BNRED_STATS"]["fused"] >= 1 and seen["BD_TABLE_STATS"]["used"] >= 1
            # (no product here takes the separate "stats" variant: the edge statistics are the gather's own epilogue)
            assert composite or {"gather", "dw_bnred", "dw_addend", "plain"} <= seen["labels"]
    elif big:
        assert seen["DW_STATS"]["fused"] >= 1 and seen["BD_TABLE_STATS"]["used"] >= 1
        assert composite or {"gather", "dw", "plain"} <= seen["labels"]
    # ---- guards first (Report.finish), then: the guards changed nothing that ran
    rep.finish()
    assert plain.keys() == inside.keys() and len(plain) > 20
    for k in plain:
        assert torch.equal(plain[k], inside[k]), (rep.case, k)
        assert bool(torch.isfinite(plain[k]).all()), (rep.case, k)


def test_a_stray_write_on_the_device_is_reported():
    """the detector on the device, once: one element behind an amax-sized slot and one row in front of a [rows, H] payload,
    planted with a torch indexing op on the helper's own base buffers"""
    rep = Report("planted", "conv-extents")
    slot = rep.guards.guarded((1,), fill=0.0, name="gp_amax", device=DEV)
    gm = rep.guards.guarded((9, 260), fill=0.0, name="GM", device=DEV)
    assert rep.guards.check() == []
    a, b = rep.guards.record_of(slot), rep.guards.record_of(gm)
    assert bool((a.base[:a.before].view(torch.int32) == NAN_BITS).all()) and bool(torch.isnan(b.base[b.before + b.numel:]).all())
    a.base[a.before + 1] = 3.0
    b.base[b.before - 260] = 0.0
    assert [f[:4] for f in rep.guards.check()] == [("gp_amax", "after", 0, 0.0), ("GM", "before", -260, -1.0)]
    with pytest.raises(AssertionError, match="GM: the guard before the payload changed at offset -260 elements"):
        rep.finish()
    assert float(slot) == 0.0 and float(gm.abs().max()) == 0.0


@pytest.mark.parametrize("n,m,H,Kin", [(42, 540, 64, 64), (540, 6978, 256, 256), (12662, 168694, 256, 256), (9, 134, 100, 36)])
def test_the_forward_scratch_reserves_what_its_writers_are_documented_to_write(n, m, H, Kin):
    """alignn_egc_conv_fwd_scratch, block by block (each rounded up to 64 floats), from the extents include/alignn_hip.h states
    for the writers: the gate pass's pivot slabs are exactly alignn_egc_slabs(n) * (3 H + 1) floats, the projection epilogue's
    sums (row_tiles + 1) * 2 H.  (The edge block used to be (slabs + 1) * (3 H + 1) "for the gate pass", one slab more than the
    header, ops.py, model.hip and the kernel agree on; a guard cannot see a reservation that is too large.)"""
    from alignn_amd import _lib

    lib = _lib.load()
    al = lambda floats: -(-floats // 64) * 64  # noqa: E731
    slabs, fold = lib.alignn_egc_slabs(n), lib.alignn_slab_fold_slabs()
    for edge_kind in (0, 1, 2):
        e_part = (lib.alignn_gemm_nt_x6_row_tiles(m, H, Kin) + 1) * 2 * H if edge_kind else slabs * (3 * H + 1)
        want = al(e_part) + al(fold * 2 * H) + al(slabs * (3 * H + 1)) + (al(n * H) if edge_kind == 2 else 0)
        assert lib.alignn_egc_conv_fwd_scratch(n, m, H, Kin, edge_kind) == 4 * want, edge_kind
