"""Host-only checks of the whole-model entry points (csrc/model.hip): ``alignn_model_plan`` is pure host arithmetic (which
kernel every product takes, the workspace layout), so its decisions are testable without a GPU - the launches themselves are
covered by tests/test_gpu_cmodel.py."""

import ctypes as C

import pytest

from alignn_amd import cmodel

NOT_SUPPORTED = 801


def _desc(H=256, la=4, lg=4, images=True, lanes=True):
    d = cmodel.ModelDesc()
    n = 2 * la + lg
    arr = (cmodel.ConvParams * n)()
    for i in range(n):
        for f, _ in cmodel.ConvParams._fields_:
            setattr(arr[i], f, 0x1000)
        if not images:
            for f in ("wcat_img", "wcat_img_t", "weg_img", "weg_img_t"):
                setattr(arr[i], f, None)
    d.convs = C.addressof(arr)
    d.alignn_layers, d.gcn_layers, d.H, d.out_features = la, lg, H, 1
    d.atom_in, d.edge_bins, d.angle_bins, d.embed = 92, 80, 40, 64
    for name, (i, o) in dict(atom=(92, H), edge1=(80, 64), edge2=(64, H), angle1=(40, 64), angle2=(64, H)).items():
        blk = getattr(d, name)
        for f, _ in cmodel.MlpParams._fields_[:12]:
            setattr(blk, f, 0x1000)
        blk.in_, blk.out = i, o
        if not images:
            blk.img = blk.img_t = None
    d.x6_min_tiles, d.bd_segment_table = 256, 1
    d.amax_min_rows, d.lane_min_rows, d.side_min_rows = 4096, 131072, 32768
    d.fc_W = d.fc_b = d.g_fc_W = d.g_fc_b = 0x1000
    if lanes:
        d.lane_T, d.side, d.aux = 0x10, 0x20, 0x30
    return d, arr


def _batch(N, E, T, B):
    mb = cmodel.ModelBatch()
    for g, (n, m) in ((mb.g, (N, E)), (mb.lg, (E, T))):
        g.n, g.m = n, m
        for f in ("seg_ptr", "src", "dst", "out_ptr", "out_slot"):
            setattr(g, f, 0x1000)
    mb.lg.seg_node = mb.lg.seg_rank = mb.lg.grp_seg_ptr = mb.lg.grp_src_ptr = 0x1000
    mb.lg.n_groups, mb.lg.dense_max_src = N, 16
    mb.graph_ptr = mb.atom_features = mb.r = mb.h = 0x1000
    mb.B = B
    return mb


def _plan(d, mb):
    lib = cmodel._lib_model()
    f, t = C.c_size_t(0), C.c_size_t(0)
    rc = lib.alignn_model_plan(C.addressof(d), C.addressof(mb), C.addressof(f), C.addressof(t))
    return rc, f.value, t.value


@pytest.mark.parametrize("N,E,T,B", [(3840, 50712, 676200, 64), (480, 6339, 84525, 8), (15360, 202848, 2704800, 256)])
def test_workspace_of_the_baseline_batches(N, E, T, B):
    d, _keep = _desc()
    rc, fwd, tot = _plan(d, _batch(N, E, T, B))
    assert rc == 0
    t_row = T * 256 * 4
    # forward tape: 2 T-row tensors per line-graph convolution (7: the last edge output is dead) + the angle embedding (2.5)
    assert 9 * t_row < fwd < 16 * t_row, fwd / t_row
    # backward: two more T-row tensors per line-graph convolution + the angle embedding's
    assert fwd + 9 * t_row < tot < fwd + 16 * t_row, (tot - fwd) / t_row
    assert fwd % 256 == 0 and tot % 256 == 0
    # the layout does not depend on whether the helper streams exist beyond the stream-local scratch regions
    d1, _k1 = _desc(lanes=False)
    rc1, fwd1, tot1 = _plan(d1, _batch(N, E, T, B))
    assert rc1 == 0 and fwd1 == fwd and tot1 <= tot


def test_kernel_choices_the_c_side_does_not_carry_are_reported():
    d, _keep = _desc(images=False)  # split-product shapes without slice images: the per-operator path slices for itself
    assert _plan(d, _batch(3840, 50712, 676200, 64))[0] == NOT_SUPPORTED
    d, _keep = _desc(H=32, la=2, lg=2, images=False)  # nothing reaches the split-product kernels: fine without images
    rc, fwd, tot = _plan(d, _batch(24, 200, 1500, 3))
    assert rc == 0 and 0 < fwd < tot < 64 << 20


def test_argument_checks():
    d, _keep = _desc()
    mb = _batch(100, 1000, 9000, 2)
    mb.lg.n = 999  # L(g)'s nodes must be g's bonds
    assert _plan(d, mb)[0] == 1
    d.alignn_layers = 0
    assert _plan(d, _batch(100, 1000, 9000, 2))[0] == 1


def test_per_model_state_is_not_part_of_the_module():
    """ctypes blocks with pointer fields cannot be pickled or deep-copied, so nothing of the C path's per-model
    state may sit in ``model.__dict__`` (``copy.deepcopy(model)`` for EMA / SWA copies and best-model snapshots walks it).
    The state lives in a weak dictionary keyed by the model and dies with it."""
    import copy
    import gc
    import pickle

    from alignn_amd import ALIGNN, ALIGNNConfig

    with pytest.raises(ValueError):
        pickle.dumps(cmodel.ModelDesc())  # (what used to sit in model.__dict__['_cmodel'])
    m = ALIGNN(ALIGNNConfig(name="alignn", alignn_layers=1, gcn_layers=1, hidden_features=32, embedding_features=16, link="log"))
    cmodel.model_cache(m)["binding"] = cmodel.ModelDesc()
    twin = copy.deepcopy(m)
    assert pickle.loads(pickle.dumps(m)).fc.weight.shape == m.fc.weight.shape
    assert "binding" in cmodel.model_cache(m) and cmodel.model_cache(twin) == {}
    n = len(cmodel._PER_MODEL)
    del m, twin
    gc.collect()
    assert len(cmodel._PER_MODEL) == n - 2


def _ff(lg_on_fly=1, stress=1):
    f = cmodel.FFDesc()
    f.lg_on_fly, f.add_reverse_forces, f.force_mult_natoms, f.energy_mult_natoms = lg_on_fly, 1, 0, 1
    f.has_stress, f.use_penalty, f.dense_lg_reverse = stress, 1, 1
    f.grad_multiplier, f.stress_multiplier, f.penalty_factor, f.penalty_threshold = -1.0, 1.0, 0.1, 1.0
    f.volume = 0x1000 if stress else None
    return f


def _ff_plan(d, mb, f):
    lib = cmodel._lib_model()
    a, b = C.c_size_t(0), C.c_size_t(0)
    rc = lib.alignn_ff_plan(C.addressof(d), C.addressof(mb), C.addressof(f), C.addressof(a), C.addressof(b))
    return rc, a.value, b.value


def test_layernorm_flavour_and_force_field_plans():
    """ALIGNNAtomWise on the whole-model entry points: the LayerNorm flavour of alignn_model_plan, and alignn_ff_plan (force
    evaluation = forward + reverse w.r.t. the bond vectors; + the tangent-carrying second-order pass) at BASELINE configs[3]
    (16 x 200 atoms) and at an MD cell (1 x 200 atoms).  Host arithmetic only."""
    N, E, T, B = 3200, 42224, 561792, 16
    d, _keep = _desc()
    d.norm = 1
    rc, fwd, tot = _plan(d, _batch(N, E, T, B))
    assert rc == 0
    t_row = T * 256 * 4
    assert 9 * t_row < fwd < 18 * t_row and fwd < tot < fwd + 20 * t_row, (fwd / t_row, tot / t_row)
    f = _ff()
    rc, ev, full = _ff_plan(d, _batch(N, E, T, B), f)
    assert rc == 0
    # evaluation: the tape of the energy-only forward + its reverse w.r.t. r; the second-order pass about twice that again
    assert fwd < ev < tot + 4 * t_row, (ev / t_row, fwd / t_row, tot / t_row)
    assert ev + 20 * t_row < full < ev + 60 * t_row, ((full - ev) / t_row)
    rc1, ev1, full1 = _ff_plan(d, _batch(200, 2644, 35326, 1), _ff(stress=0))
    assert rc1 == 0 and 0 < ev1 < full1 < 4 << 30
    # the force field is the LayerNorm model with a one-wide readout; stress needs the volumes; lg_on_fly = 0 needs the cosines
    d.norm = 0
    assert _ff_plan(d, _batch(N, E, T, B), f)[0] == 1
    d.norm = 1
    g = _ff()
    g.volume = None
    assert _ff_plan(d, _batch(N, E, T, B), g)[0] == 1
    mb = _batch(N, E, T, B)
    mb.h = None
    assert _ff_plan(d, mb, _ff(lg_on_fly=0))[0] == 1 and _ff_plan(d, mb, _ff(lg_on_fly=1))[0] == 0
    # no slice images: split-product shapes are not carried
    d2, _k2 = _desc(images=False)
    d2.norm = 1
    assert _ff_plan(d2, _batch(N, E, T, B), f)[0] == NOT_SUPPORTED


def test_tape_reuse_saves_one_t_row_buffer_per_line_graph_convolution():
    """desc.reuse_tape: the edge input gradient of a convolution is written over its own dead gate pre-activation (VERDICT r04
    weak 11 / Next 8): at the benchmark batch 4 T-row buffers (+ 8 E-row ones) of the backward's share disappear."""
    N, E, T, B = 3840, 50712, 676200, 64
    d, _keep = _desc()
    rc, fwd, tot = _plan(d, _batch(N, E, T, B))
    d.reuse_tape = 1
    rc2, fwd2, tot2 = _plan(d, _batch(N, E, T, B))
    assert rc == 0 and rc2 == 0 and fwd2 == fwd
    t_row, e_row = T * 1024, E * 1024
    saved = tot - tot2
    assert 4 * t_row + 8 * e_row - (1 << 20) < saved < 4 * t_row + 8 * e_row + (1 << 20), saved / t_row
    assert tot2 < 16.6e9 < tot  # (19.3 GB -> 16.5 GB)


def test_where_the_fused_layernorm_passes_apply(monkeypatch):
    """alignn_egc_ln_fused_supported (csrc/convln.hip, host arithmetic): one feature panel per wavefront (H <= 256, H % 4 == 0) and
    edge tensors too large for the cache (>= 64 MiB); ALIGNN_AMD_LN_FUSED = 0 never, 2 whenever H allows; read per call."""
    lib = cmodel._lib_model()
    monkeypatch.delenv("ALIGNN_AMD_LN_FUSED", raising=False)
    f = lib.alignn_egc_ln_fused_supported
    assert f(256, 561792) == 1 and f(256, 676200) == 1          # BASELINE configs[3] / [1]: 575 / 692 MB per tensor
    assert f(256, 35326) == 0 and f(256, 65535) == 0 and f(256, 65536) == 1  # a 200-atom MD cell stays on the separate kernels
    assert f(64, 262144) == 1 and f(64, 200000) == 0
    assert f(512, 10 ** 7) == 0 and f(258, 10 ** 7) == 0 and f(0, 10 ** 7) == 0
    monkeypatch.setenv("ALIGNN_AMD_LN_FUSED", "2")
    assert f(256, 100) == 1 and f(512, 10 ** 7) == 0
    monkeypatch.setenv("ALIGNN_AMD_LN_FUSED", "0")
    assert f(256, 10 ** 7) == 0


def test_plan_keys_cover_what_the_planners_read():
    """``cmodel.plan_key`` is what ``Binding.plan`` caches a planner's answer under: whenever a per-call switch, a force-field
    switch or a missing graph array changes what the planner says, it must change the key too - else a later step of the same
    shape under another switch gets the byte count of the earlier one (the force-field key used to lack ``dw_fused``: 39.54 GB
    with the fused dW pass off, 39.50 GB with it on, at the batch below).  One field at a time against the real planners; the
    minimum counts keep the test from passing because nothing moved the planners."""
    import inspect
    import re

    lib = cmodel._lib_model()

    def model(d, mb, f):
        return _plan(d, mb)

    def ff(d, mb, f):
        return _ff_plan(d, mb, f)

    def infer(d, mb, f):
        return 0, lib.alignn_model_infer_workspace(C.addressof(d), C.addressof(mb))

    desc_edits = [(k, v) for k, v in dict(dw_fused=65536, angle_fused=1, reuse_tape=1, lane_T=None, side=None, aux=None,
                                          side_min_rows=0, lane_min_rows=1 << 40).items()]
    ff_flips = ["lg_on_fly", "has_stress", "dense_lg_reverse", "use_penalty"]
    cases = {"model": (model, 0, (3840, 50712, 676200, 64), 8), "ff": (ff, 1, (3200, 42224, 561792, 16), 7),
             "infer": (infer, 0, (3840, 50712, 676200, 64), 1)}
    for kind, (planner, norm, shape, at_least) in cases.items():
        def answer(edit):
            (d, _keep), mb, f = _desc(), _batch(*shape), (_ff() if kind == "ff" else None)
            d.norm = norm
            edit(d, mb, f)
            return planner(d, mb, f), cmodel.plan_key(kind, d, mb, f)

        base, base_key = answer(lambda d, mb, f: None)
        assert base[0] == 0 and base[-1] > 0, (kind, base)
        edits = {name: (lambda d, mb, f, name=name, v=v: setattr(d, name, v)) for name, v in desc_edits}
        edits["lg.seg_rank"] = lambda d, mb, f: setattr(mb.lg, "seg_rank", None)
        if kind == "ff":
            edits.update({name: (lambda d, mb, f, name=name: setattr(f, name, 1 - getattr(f, name))) for name in ff_flips})
        moved = []
        for name, edit in edits.items():
            got, key = answer(edit)
            if got != base:
                moved.append(name)
                assert key != base_key, (kind, name, base, got)
        assert len(moved) >= at_least, (kind, moved)
    # "every field set_mode() writes" stays true when set_mode() learns another one
    written = set(re.findall(r"\bd\.(\w+) = ", inspect.getsource(cmodel.Binding.set_mode)))
    assert written == set(cmodel.MODE_FIELDS), written ^ set(cmodel.MODE_FIELDS)
