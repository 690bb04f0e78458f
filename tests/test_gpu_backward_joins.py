"""Where the backward of the whole-model C path (csrc/model.hip) joins its helper streams.

A bond-graph convolution's node input gradient g_x is made on the aux stream and leaves with an event: the caller's stream no
longer waits for it at the end of ``conv_bwd``, its readers do - the node branch of the next bond-graph convolution's backward
(enqueued on aux right behind it, beside the line-graph backward), the atom embedding's backward at the tail, and the final join
before the C call returns.  Nothing is launched differently, so a missing dependency is a race and the bar is BIT equality:
four streams against one, repeats against each other, a replayed hipGraph against eager launches (an unjoined helper stream makes
the capture itself fail).

4 crystals of 20 atoms, a few thousand triplet rows, under two settings of the row thresholds (``SETTINGS``):

``all_lane_T``  both at 1: every convolution and every MLP on lane T, weight gradients on the side stream.  A convolution on lane
                T does not fork its node product, so the aux stream stays idle here (asserted: no event is recorded on it).
``aux``         the lane threshold between the bond count and the triplet count, the side threshold at 1 - the split of the
                full-size step: line-graph convolutions on lane T, bond-graph convolutions on the caller's stream with g_x and
                the hoisted node branch on aux.  The C path reports the events it recorded on aux (``alignn_debug_joins``),
                and their number is asserted: per backward one g_x per bond-graph convolution and one node branch for each
                but the model's last (its output gradient comes from the pooling, on the caller's stream),
                2 (alignn_layers + gcn_layers) - 1.

The layer layouts cover the first and last convolution of each kind and the hand-over between the two loops.  The C calls take a
model with at least one layer of each kind (``cmodel._structure_ok``): (1, 0), (0, 2) and (2, 0) run the per-operator path under
the same switches, so the ``aux`` setting brings (1, 1), (1, 2) and (2, 1), which do reach ``conv_bwd``."""

import contextlib
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

from alignn_amd import ALIGNN, ALIGNNAtomWise, ALIGNNAtomWiseConfig, ALIGNNConfig, GraphBatch, _lib, cmodel, ops  # noqa: E402
from alignn_amd.synthetic import make_batch  # noqa: E402

DEV = "cuda"
FLAVOURS = ["batchnorm", "layernorm"]
SETTINGS = ["all_lane_T", "aux"]
CASES = ([("all_lane_T", la) for la in [(2, 2), (1, 0), (0, 2), (2, 0)]]
         + [("aux", la) for la in [(2, 2), (1, 1), (1, 2), (2, 1)]])
POOL = 512  # kEvents of csrc/model.hip


@contextlib.contextmanager
def _thresholds(setting, raw):
    lane = 1 if setting == "all_lane_T" else raw.num_edges + 1
    assert setting == "all_lane_T" or raw.num_edges < lane <= raw.num_triplets  # line graph on lane T, bond graph not
    saved = (ops._LANE["min_rows"], ops._SIDE["min_rows"])
    ops._LANE["min_rows"], ops._SIDE["min_rows"] = lane, 1
    try:
        yield
    finally:
        ops._LANE["min_rows"], ops._SIDE["min_rows"] = saved


def _joins():
    """(events recorded on aux, waits for a deferred event, most marks between an event's record and a wait for it) of the C
    calls since the last query"""
    fn = _lib.load().alignn_debug_joins  # (a test hook of csrc/model.hip, not declared in alignn_hip.h: bound here)
    fn.restype, fn.argtypes = ctypes.c_int, [ctypes.c_void_p]
    out = (ctypes.c_int64 * 3)()
    fn(out)
    return tuple(out)


def _check_aux(setting, layers, joins, n_bwd, first_gx=True):
    """what ``joins`` must say after ``n_bwd`` backward passes of a model the C calls take"""
    print(setting, layers, "aux marks, late waits, largest distance:", joins)
    if setting == "all_lane_T":
        assert joins[0] == 0, joins
    else:
        # on aux: one g_x per bond-graph convolution (but the model's first one's, where nobody reads it) and one node branch for
        # each but the model's last; waited for on the caller's stream: those node branches and, where it was made, the first
        # convolution's g_x
        assert joins[0] == n_bwd * (2 * sum(layers) - (1 if first_gx else 2)), joins
        assert joins[1] == n_bwd * (sum(layers) - (0 if first_gx else 1)), joins
    assert joins[2] < POOL // 4, joins


@pytest.fixture(scope="module")
def data():
    raw = make_batch(4, 20, seed0=17)
    return raw, GraphBatch.from_raw(raw, device=DEV), torch.randn(4, generator=torch.Generator().manual_seed(3)).to(DEV)


def _mk(flavour, layers, seed=0, ff=False):
    torch.manual_seed(seed)
    if flavour == "batchnorm":
        return ALIGNN(ALIGNNConfig(name="alignn", alignn_layers=layers[0], gcn_layers=layers[1])).to(DEV).train()
    m = ALIGNNAtomWise(ALIGNNAtomWiseConfig(name="alignn_atomwise", alignn_layers=layers[0], gcn_layers=layers[1],
                                            atom_input_features=92, calculate_gradient=ff,
                                            stresswise_weight=0.05 if ff else 0.0)).to(DEV).train()
    with torch.no_grad():  # LayerNorm affine parameters that are not the initial 1 / 0
        for n_, p_ in m.named_parameters():
            if ".bn_" in n_ or ".layer.1." in n_:
                p_.add_(0.1 * torch.randn_like(p_))
    return m


def _pred(model, batch):
    o = model(batch)
    return o["out"] if isinstance(o, dict) else o


def _state(model, pred=None):
    out = {} if pred is None else {"pred": pred.detach().clone()}
    out.update({"g." + k: p.grad.clone() for k, p in model.named_parameters() if p.grad is not None})
    out.update({"s." + k: v.clone() for k, v in model.state_dict().items()})
    return out


def _same(a, b, what=""):
    assert a.keys() == b.keys(), set(a) ^ set(b)
    for k in a:
        assert torch.equal(a[k], b[k]), (what, k, float((a[k].double() - b[k].double()).abs().max()))


def _two_steps(model, batch, target):
    opt = torch.optim.AdamW(model.parameters(), lr=1e-3, fused=True)
    for _ in range(2):
        opt.zero_grad(set_to_none=True)
        pred = _pred(model, batch)
        torch.nn.functional.l1_loss(pred, target).backward()
        opt.step()
    torch.cuda.synchronize()
    return _state(model, pred)


class _helpers_off:
    """the switches of tests/test_gpu_cmodel.py::test_one_stream_and_four_streams_give_the_same_bits"""

    def __enter__(self):
        self.saved = (ops._LANE["enabled"], ops._SIDE["enabled"], ops.FORK_DGRAD)
        ops._LANE["enabled"], ops._SIDE["enabled"], ops.FORK_DGRAD = "0", False, "0"

    def __exit__(self, *exc):
        ops._LANE["enabled"], ops._SIDE["enabled"], ops.FORK_DGRAD = self.saved


def _stream_apart(model, layers):
    """A stream that is none of the model's helper streams.  torch hands streams out of a small pool, round robin: now and then
    a new one IS a binding's lane T or aux, the C call then sees that helper as the caller's stream and leaves it unused - right,
    but not what the counts of ``_check_aux`` describe."""
    taken = {st.cuda_stream for st in cmodel.binding_of(model).streams} if min(layers) >= 1 else set()
    while True:
        s = torch.cuda.Stream()
        if s.cuda_stream not in taken:
            return s


def _c_calls(fn):
    for k in list(cmodel.STATS):
        cmodel.STATS[k] = 0
    _joins()
    out = fn()
    return out, dict(cmodel.STATS), _joins()


@pytest.mark.parametrize("setting,layers", CASES)
@pytest.mark.parametrize("flavour", FLAVOURS)
def test_four_streams_one_stream_and_repeats_give_the_same_bits(data, flavour, setting, layers):
    raw, batch, target = data
    assert raw.num_triplets >= 1000
    with _thresholds(setting, raw):
        runs, stats, joins = _c_calls(lambda: [_two_steps(_mk(flavour, layers), batch, target) for _ in range(5)])
        if min(layers) >= 1:
            assert stats.get("bwd", 0) == 10, stats  # (every backward went through alignn_model_bwd)
            _check_aux(setting, layers, joins, 10)
        with _helpers_off():
            one = _two_steps(_mk(flavour, layers), batch, target)
    _same(runs[0], one, "streams")
    for i in range(1, 5):
        _same(runs[0], runs[i], f"repeat {i}")
    assert all(bool(torch.isfinite(t).all()) for t in runs[0].values() if t.is_floating_point())


@pytest.mark.parametrize("setting,layers", CASES)
@pytest.mark.parametrize("flavour", FLAVOURS)
def test_a_captured_step_replays_to_the_eager_bits(data, flavour, setting, layers):
    """Every helper stream - aux with a pending event included - has to be joined into the caller's stream before the C call
    returns, or ending the capture fails."""
    raw, batch, target = data
    l1 = torch.nn.functional.l1_loss
    for k in list(cmodel.STATS):
        cmodel.STATS[k] = 0
    _joins()
    with _thresholds(setting, raw):
        eager = _mk(flavour, layers)
        losses = []
        for _ in range(3):
            for p in eager.parameters():
                p.grad = None
            loss = l1(_pred(eager, batch), target)
            loss.backward()
            losses.append(loss.detach().clone())
        ref = _state(eager)
        model = _mk(flavour, layers)
        s = _stream_apart(model, layers)
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):  # warm-up on a side stream (torch's capture recipe)
            l1(_pred(model, batch), target).backward()
        torch.cuda.current_stream().wait_stream(s)
        torch.cuda.synchronize()
        for p in model.parameters():
            p.grad = None
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=_stream_apart(model, layers), capture_error_mode="thread_local"):
            g_loss = l1(_pred(model, batch), target)
            g_loss.backward()
    if min(layers) >= 1:
        assert cmodel.STATS.get("bwd", 0) == 5, cmodel.STATS  # (3 eager steps, the warm-up and the captured one)
        _check_aux(setting, layers, _joins(), 5)
    grads = {k: p.grad for k, p in model.named_parameters() if p.grad is not None}
    for i in (1, 2):  # (the warm-up step was step 0 of the running statistics)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(g_loss, losses[i]), (i, g_loss.item(), losses[i].item())
    got = {"g." + k: v for k, v in grads.items()}
    got.update({"s." + k: v for k, v in model.state_dict().items()})
    _same(ref, got, "replay")


@pytest.mark.parametrize("setting", SETTINGS)
def test_force_evaluation_reverse_pass_on_four_streams(data, setting):
    """One ``calculate_gradient=True`` forward (``alignn_ff_eval``): its reverse pass runs ``conv_bwd`` without parameter
    gradients, and the first convolution's node input gradient is never made (``need_gx == false``: one event fewer on aux)
    while - in the ``aux`` setting - its node branch still sits on the aux stream, which the call joins before it returns."""
    raw, batch, _target = data
    model = _mk("layernorm", (2, 2), seed=4, ff=True).eval()

    def values():
        o = model(batch)
        torch.cuda.synchronize()
        return {k: o[k].detach().clone() for k in ("out", "grad", "stresses")}

    with _thresholds(setting, raw):
        runs, stats, joins = _c_calls(lambda: [values() for _ in range(5)])
        assert stats.get("ff_eval", 0) == 5 and stats.get("ff_grad", 0) == 0, stats
        _check_aux(setting, (2, 2), joins, 5, first_gx=False)
        with _helpers_off():
            one = values()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, capture_error_mode="thread_local"):
            o = model(batch)
    _same(runs[0], one, "streams")
    for i in range(1, 5):
        _same(runs[0], runs[i], f"repeat {i}")
    assert all(bool(torch.isfinite(t).all()) for t in runs[0].values())
    graph.replay()
    torch.cuda.synchronize()
    _same(runs[0], {k: o[k] for k in ("out", "grad", "stresses")}, "replay")


@pytest.mark.parametrize("setting", SETTINGS)
@pytest.mark.parametrize("flavour", FLAVOURS)
def test_deferred_events_stay_inside_the_pool_with_four_plus_four_layers(data, flavour, setting):
    """The event pool rotates through 512 events and a deferred event must be waited for before it is recorded again: the C call
    counts the marks in between and fails rather than wait for a recycled one (``_lib.check`` raises then).  The longest-lived
    events are a bond-graph convolution's g_x and the node branch behind it: recorded in front of one line-graph convolution's
    backward and waited for right behind it, whatever the number of layers, and one convolution's backward records about ten
    events.  So the largest distance the C path saw (``_check_aux``) has to stay below a quarter of the pool in the deepest
    model of the configurations too - in the ``aux`` setting, where such events exist (``joins[1]`` counts the waits for them)."""
    raw, batch, target = data
    with _thresholds(setting, raw):
        four, stats, joins = _c_calls(lambda: _two_steps(_mk(flavour, (4, 4)), batch, target))
        assert stats.get("fwd", 0) == 2 and stats.get("bwd", 0) == 2, stats
        _check_aux(setting, (4, 4), joins, 2)
        if setting == "aux":
            assert joins[1] > 0 and 0 < joins[2], joins
        with _helpers_off():
            one = _two_steps(_mk(flavour, (4, 4)), batch, target)
    _same(four, one, "streams")
