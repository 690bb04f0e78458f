"""ALIGNNAtomWise on the whole-model C entry points (csrc/model.hip + csrc/ff.hip, alignn_amd/cmodel.py): energy-only training
(``alignn_model_fwd / _bwd``, LayerNorm flavour), training THROUGH the forces (``alignn_ff_eval`` + ``alignn_ff_grad``) and the
force evaluation of MD (``alignn_ff_eval``).  They issue the launches of the per-operator path (alignn_amd/ops.py, alignn_amd/ff2.py)
with the same arguments, so the bar is BIT equality of energies, forces, stresses, every parameter gradient and the parameters
after optimizer steps; the parity of both paths against the reference's own class is tests/test_gpu_round2.py /
tests/test_gpu_full_size.py (which run through these calls by default)."""

import pytest
import torch

pytestmark = pytest.mark.gpu

from alignn_amd import ALIGNNAtomWise, ALIGNNAtomWiseConfig, GraphBatch, cmodel, ops  # noqa: E402
from alignn_amd.synthetic import make_batch  # noqa: E402

DEV = "cuda"


def _mk(seed=0, ff=True, **kw):
    torch.manual_seed(seed)
    cfg = dict(name="alignn_atomwise", alignn_layers=2, gcn_layers=2, hidden_features=256, atom_input_features=92,
               calculate_gradient=ff, stresswise_weight=0.05 if ff else 0.0)
    cfg.update(kw)
    m = ALIGNNAtomWise(ALIGNNAtomWiseConfig(**cfg)).to(DEV).train()
    with torch.no_grad():  # LayerNorm affine parameters that are not the initial 1 / 0
        for n_, p_ in m.named_parameters():
            if ".bn_" in n_ or ".layer.1." in n_:
                p_.add_(0.1 * torch.randn_like(p_))
    return m


def _same(a, b, what=""):
    assert a.keys() == b.keys(), set(a) ^ set(b)
    for k in a:
        assert torch.equal(a[k], b[k]), (what, k, float((a[k].double() - b[k].double()).abs().max()),
                                        float(b[k].double().abs().max()))


def _targets(raw, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(raw.batch_size, generator=g).to(DEV), torch.randn(raw.num_nodes, 3, generator=g).to(DEV),
            torch.randn(raw.batch_size, 3, 3, generator=g).to(DEV))


def _train(model, batches, targets, use_c, ff=True, steps_opt=True):
    prev = cmodel.ENABLED
    cmodel.ENABLED = use_c
    l1 = torch.nn.functional.l1_loss
    try:
        opt = torch.optim.AdamW(model.parameters(), lr=1e-3, fused=True)
        for b, (te, tf, ts) in zip(batches, targets):
            opt.zero_grad(set_to_none=True)
            o = model(b)
            loss = l1(o["out"], te)
            if ff:
                loss = loss + l1(o["grad"], tf)
                if o["stresses"].dim() == 3:  # (stresswise_weight == 0: the reference's placeholder)
                    loss = loss + l1(o["stresses"], ts)
            loss.backward()
            if steps_opt:
                opt.step()
        torch.cuda.synchronize()
        out = {"out": o["out"].detach().clone(), "loss": loss.detach().clone()}
        if ff:
            out["forces"] = o["grad"].detach().clone()
            if o["stresses"].dim() == 3:  # (else: the reference's uninitialised placeholder)
                out["stress"] = o["stresses"].detach().clone()
        out.update({"g." + k: p.grad.clone() for k, p in model.named_parameters() if p.grad is not None})
        out.update({"p." + k: p.detach().clone() for k, p in model.named_parameters()})
        return out
    finally:
        cmodel.ENABLED = prev


def _reset_stats():
    for k in list(cmodel.STATS):
        cmodel.STATS[k] = 0


@pytest.mark.parametrize("B,atoms", [(3, 30), (16, 60)])  # (the second: T = 169 k rows - lane T and the side stream are in use)
def test_force_training_equals_the_per_operator_path_bit_for_bit(B, atoms):
    raws = [make_batch(B, atoms, seed0=40 + i) for i in range(2)]
    batches = [GraphBatch.from_raw(r, device=DEV) for r in raws]
    targets = [_targets(r, i) for i, r in enumerate(raws)]
    _reset_stats()
    a = _train(_mk(1), batches, targets, True)
    assert cmodel.STATS.get("ff_eval", 0) == 2 and cmodel.STATS.get("ff_grad", 0) == 2, cmodel.STATS
    b = _train(_mk(1), batches, targets, False)
    assert sum(k.startswith("g.") for k in a) > 100
    _same(a, b, f"B={B}")
    assert all(bool(torch.isfinite(t).all()) for t in a.values())


def test_switching_the_fused_dw_pass_between_steps_plans_the_workspace_again():
    """``ops.DGRAD_WGRAD_FUSED`` on, off, on over three steps of ONE model and one batch: the workspace of alignn_ff_plan depends
    on the switch (fewer bytes with the fused pass), so a plan cached under a key without it hands the second step the first
    one's smaller byte count and alignn_ff_grad refuses the workspace.  Every step stays on the C calls and gives the gradients
    of the per-operator path under the same switch sequence, bit for bit."""
    raw = make_batch(8, 60, seed0=44)
    assert raw.num_triplets >= ops.DW_MIN_ROWS  # (where the fused dW pass starts to apply)
    batch = GraphBatch.from_raw(raw, device=DEV)
    te, tf, ts = _targets(raw, 2)
    l1 = torch.nn.functional.l1_loss

    def run(use_c):
        saved, prev, cmodel.ENABLED = ops.DGRAD_WGRAD_FUSED, cmodel.ENABLED, use_c
        try:
            m = _mk(10)
            opt = torch.optim.AdamW(m.parameters(), lr=1e-3, fused=True)
            grads = []
            for fused in (True, False, True):
                ops.DGRAD_WGRAD_FUSED = fused
                opt.zero_grad(set_to_none=True)
                o = m(batch)
                (l1(o["out"], te) + l1(o["grad"], tf) + l1(o["stresses"], ts)).backward()
                torch.cuda.synchronize()
                grads.append({"g." + k: p.grad.clone() for k, p in m.named_parameters() if p.grad is not None})
                opt.step()
            return grads
        finally:
            ops.DGRAD_WGRAD_FUSED, cmodel.ENABLED = saved, prev

    _reset_stats()
    a = run(True)
    assert cmodel.STATS.get("ff_grad", 0) == 3, cmodel.STATS
    b = run(False)
    for i, (ga, gb) in enumerate(zip(a, b)):
        assert len(ga) > 100
        _same(ga, gb, f"step {i}")


def test_force_training_switches_energy_only_forces_only_no_reverse_natoms():
    raw = make_batch(4, 24, seed0=7)
    batch = GraphBatch.from_raw(raw, device=DEV)
    tgt = _targets(raw, 3)
    for kw in (dict(stresswise_weight=0.0), dict(add_reverse_forces=False), dict(force_mult_natoms=True),
               dict(energy_mult_natoms=False, use_penalty=False), dict(lg_on_fly=False), dict(grad_multiplier=-2.0, stress_multiplier=0.5)):
        _reset_stats()
        a = _train(_mk(2, **kw), [batch], [tgt], True)
        assert cmodel.STATS.get("ff_grad", 0) == 1, (kw, cmodel.STATS)
        b = _train(_mk(2, **kw), [batch], [tgt], False)
        _same(a, b, str(kw))


def test_partial_losses_energy_only_or_forces_only():
    """A loss that uses only some of the three outputs: the unused ones arrive as None in backward."""
    raw = make_batch(4, 24, seed0=8)
    batch = GraphBatch.from_raw(raw, device=DEV)
    te, tf, ts = _targets(raw, 4)
    l1 = torch.nn.functional.l1_loss

    def run(use_c, which):
        prev, cmodel.ENABLED = cmodel.ENABLED, use_c
        try:
            m = _mk(3)
            o = m(batch)
            loss = {"e": lambda: l1(o["out"], te), "f": lambda: l1(o["grad"], tf), "s": lambda: l1(o["stresses"], ts)}[which]()
            loss.backward()
            torch.cuda.synchronize()
            return {k: p.grad.clone() for k, p in m.named_parameters() if p.grad is not None}
        finally:
            cmodel.ENABLED = prev

    for which in "efs":
        _same(run(True, which), run(False, which), which)


def test_force_evaluation_in_eval_mode_is_one_c_call():
    """MD / calculators (alignn/ff/calculators.py:280-291): model.eval(), grad enabled, forces as values."""
    raw = make_batch(1, 200, seed0=5)
    batch = GraphBatch.from_raw(raw, device=DEV)
    m = _mk(4, alignn_layers=4, gcn_layers=4).eval()
    _reset_stats()
    a = m(batch)
    assert cmodel.STATS.get("ff_eval", 0) == 1 and cmodel.STATS.get("ff_grad", 0) == 0
    with cmodel.disabled():
        b = m(batch)
    torch.cuda.synchronize()
    for k in ("out", "grad", "stresses"):
        assert a[k].shape == b[k].shape and torch.equal(a[k], b[k]), (k, float((a[k] - b[k]).abs().max()))
    assert not a["grad"].requires_grad and a["out"].dim() == 0


def test_energy_only_training_of_the_layernorm_model():
    raws = [make_batch(B, n, seed0=s) for B, n, s in ((6, 30, 1), (16, 60, 2), (5, 44, 3))]
    batches = [GraphBatch.from_raw(r, device=DEV) for r in raws]
    targets = [_targets(r, i) for i, r in enumerate(raws)]
    _reset_stats()
    a = _train(_mk(5, ff=False), batches, targets, True, ff=False)
    assert cmodel.STATS["fwd"] == 3 and cmodel.STATS["bwd"] == 3, cmodel.STATS
    b = _train(_mk(5, ff=False), batches, targets, False, ff=False)
    _same(a, b, "energy only")
    c = _train(_mk(5, ff=False, lg_on_fly=False), batches, targets, True, ff=False)  # the loader's cosines instead of recomputed ones
    assert float((a["out"] - c["out"]).abs().max()) < 1e-5 * float(a["out"].abs().max())


class _ForeignMFMA:
    """A kernel of SOMEBODY ELSE on its own stream while the step runs: fp16 matrix products of the vendor library (MFMA waves
    that share the compute units with the step's kernels - the stand-in for a collective or a co-tenant)."""

    def __init__(self, on, n=40):
        self.on, self.n = on, n
        if on:
            self.s = torch.cuda.Stream()
            self.a = torch.randn(4096, 4096, device=DEV, dtype=torch.float16)
            self.c = torch.empty_like(self.a)

    def __enter__(self):
        if self.on:
            self.s.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(self.s):
                for _ in range(self.n):
                    torch.matmul(self.a, self.a, out=self.c)
        return self

    def __exit__(self, *exc):
        if self.on:
            torch.cuda.current_stream().wait_stream(self.s)
        return False


@pytest.mark.parametrize("B,ff,use_c,foreign", [(16, True, True, False), (48, True, True, False), (64, False, True, False),
                                                (64, False, False, False), (48, True, True, True), (96, True, True, True),
                                                (64, False, False, True)])
def test_a_step_is_bit_reproducible_run_to_run(B, ff, use_c, foreign):
    """Round 5 found steps of the LayerNorm model NOT bit-reproducible on helper streams (forces off by 1e-3 run to run at 48
    crystals, gradients by 1e-5; hipGraph replays already at 16).  Round 6 reproduced the cause stand-alone
    (tools/pk_f32_repro2.hip, profiles/r06_pk_f32_repro.txt): a packed-fp32 instruction whose op_sel takes the HIGH half of src1
    for the LOW result reads that operand as +0.0 in lanes 48-63 while MFMA waves of another workgroup issue on the same SIMD -
    in the model, ``ln_silu_bwd_kernel`` beside the T-row projection of the other lane.  No object of the library contains
    that form any more (alignn_amd/build.py refuses to link one; tests/test_build_isa.py): four runs of the same step -
    energies, forces, stresses, every gradient - are bit-identical with lane T, the aux and the side stream in use, through
    the C calls and through the per-operator path, up to 96 crystals, and with a FOREIGN MFMA kernel (a vendor-library fp16
    product on its own stream) running beside the step."""
    raw = make_batch(B, 60, seed0=11)
    batch = GraphBatch.from_raw(raw, device=DEV)
    tgt = _targets(raw, 6)
    m = _mk(9, ff=ff)
    ref = _train(m, [batch], [tgt], use_c, ff=ff, steps_opt=False)
    for _ in range(3):
        with _ForeignMFMA(foreign):
            got = _train(m, [batch], [tgt], use_c, ff=ff, steps_opt=False)
        _same(ref, got, "run to run")


def test_the_headline_step_is_bit_reproducible_beside_a_foreign_mfma_kernel():
    """The same bar for the BatchNorm model of the headline (configs[1]: 64 crystals, T = 1.0 M rows) - its kernels share the
    compute units with a foreign MFMA kernel in a multi-tenant / collective-overlapped deployment."""
    from alignn_amd import ALIGNN, ALIGNNConfig
    raw = make_batch(64, 60, seed0=0)
    batch = GraphBatch.from_raw(raw, device=DEV)
    torch.manual_seed(3)
    model = ALIGNN(ALIGNNConfig(name="alignn")).to(DEV).train()
    target = torch.randn(raw.batch_size, device=DEV)

    def step(foreign):
        for p in model.parameters():
            p.grad = None
        with _ForeignMFMA(foreign, n=30):
            out = model(batch)
            torch.nn.functional.mse_loss(out.view(-1), target).backward()
        torch.cuda.synchronize()
        res = {"out": out.detach().clone()}
        res.update({"g." + k: p.grad.clone() for k, p in model.named_parameters() if p.grad is not None})
        return res

    ref = step(False)
    for rep in range(3):
        _same(ref, step(True), f"headline beside foreign MFMA, run {rep}")


def test_one_stream_and_helper_streams_give_the_same_bits_and_capture_replays():
    raw = make_batch(16, 60, seed0=11)
    batch = GraphBatch.from_raw(raw, device=DEV)
    tgt = _targets(raw, 6)
    ref = _train(_mk(6), [batch] * 2, [tgt] * 2, True)
    saved = (ops._LANE["enabled"], ops._SIDE["enabled"], ops.FORK_DGRAD)
    ops._LANE["enabled"], ops._SIDE["enabled"], ops.FORK_DGRAD = "0", False, "0"
    try:
        one = _train(_mk(6), [batch] * 2, [tgt] * 2, True)
    finally:
        ops._LANE["enabled"], ops._SIDE["enabled"], ops.FORK_DGRAD = saved
    _same(ref, one, "streams")
    for _ in range(2):
        _same(ref, _train(_mk(6), [batch] * 2, [tgt] * 2, True), "repeat")
    # captured into a hipGraph and replayed: same gradients as the eager step
    l1 = torch.nn.functional.l1_loss
    model = _mk(6)
    eager = _train(_mk(6), [batch], [tgt], True, steps_opt=False)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        o = model(batch)
        (l1(o["out"], tgt[0]) + l1(o["grad"], tgt[1]) + l1(o["stresses"], tgt[2])).backward()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    for p in model.parameters():
        p.grad = None
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, capture_error_mode="thread_local"):
        o = model(batch)
        loss = l1(o["out"], tgt[0]) + l1(o["grad"], tgt[1]) + l1(o["stresses"], tgt[2])
        loss.backward()
    grads = {k: p.grad for k, p in model.named_parameters() if p.grad is not None}
    for _ in range(2):
        graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(loss, eager["loss"])
    for k, g in grads.items():
        assert torch.equal(g, eager["g." + k]), k


def test_the_step_is_free_of_torch_and_vendor_kernels():
    """nothing but this library's kernels between the model call and the end of backward (the einsum of
    the stress seed was a hipBLASLt GEMM; ~80 at::native element-wise / index / reduce kernels per step)."""
    from torch.profiler import ProfilerActivity, profile

    raw = make_batch(4, 40, seed0=12)
    batch = GraphBatch.from_raw(raw, device=DEV)
    te, tf, ts = _targets(raw, 7)
    l1 = torch.nn.functional.l1_loss
    m = _mk(7)

    gE = torch.ones(raw.batch_size, device=DEV)

    def fwd_bwd():
        for p_ in m.parameters():
            p_.grad = None
        o = m(batch)
        # (the loss itself is the caller's: a few element-wise torch kernels on [B] / [N, 3] / [B, 3, 3] tensors)
        torch.autograd.backward([o["out"], o["grad"], o["stresses"]], [gE, tf, ts])

    fwd_bwd()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fwd_bwd()
        torch.cuda.synchronize()
    names = [e.key for e in prof.key_averages()]
    # (autograd's AccumulateGrad may copy a gradient that is a view of the flat buffer: those copies are the engine's)
    foreign = [n for n in names if ("at::native" in n or n.startswith("Cijk_") or "elementwise" in n or "rocblas" in n.lower())
               and "copy" not in n.lower()]
    assert not foreign, foreign
    assert any("gemm_nt" in n or "egc_" in n for n in names), names[:10]


def test_force_training_writes_into_the_packed_gradient_buffer_of_flat_adamw():
    """alignn_ff_grad with a second region of destinations (gsink / gsink_t): from the second step on the loss gradient through
    the forces lands in FlatAdamW's packed gradient buffer - value halves there, tangent halves in a scratch twin, added in place
    by the C call - and no gather of per-parameter gradients follows.  Same training state as the per-operator path, bit for bit."""
    from alignn_amd.optim import FlatAdamW, group_decay

    raw = make_batch(3, 30, seed0=21)
    batch = GraphBatch.from_raw(raw, device=DEV)
    te, tf, ts = _targets(raw, 5)
    l1 = torch.nn.functional.l1_loss

    def run(use_c):
        prev = cmodel.ENABLED
        cmodel.ENABLED = use_c
        try:
            m = _mk(3)
            opt = FlatAdamW(group_decay(m), lr=1e-3, weight_decay=1e-2, module=m)
            _reset_stats()
            cmodel.STATS["ff_sink"] = 0
            in_place = n_live = 0
            for _ in range(3):
                opt.zero_grad(set_to_none=True)
                o = m(batch)
                (l1(o["out"], te) + l1(o["grad"], tf) + l1(o["stresses"], ts)).backward()
                live = [p for p in m.parameters() if p.grad is not None]
                n_live = len(live)
                in_place = sum(1 for p in live if opt.gradient_slot(p) is not None
                               and p.grad.data_ptr() == opt.gradient_slot(p).data_ptr())
                opt.step()
            torch.cuda.synchronize()
            out = {"p." + k: p.detach().clone() for k, p in m.named_parameters()}
            out.update({"g." + k: p.grad.clone() for k, p in m.named_parameters() if p.grad is not None})
            return out, dict(cmodel.STATS), in_place, n_live
        finally:
            cmodel.ENABLED = prev

    a, stats, in_place, n_live = run(True)
    b, _s, _i, _n = run(False)
    _same(a, b, "FlatAdamW, force training")
    assert stats.get("ff_grad", 0) == 3 and stats.get("ff_sink", 0) == 2, stats
    assert in_place >= n_live - 10, (in_place, n_live)
    print(f"force training into FlatAdamW's buffer: {in_place} of {n_live} gradients in place")
