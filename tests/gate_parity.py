"""What the float64 parity tests of the edge-gated convolution kernels share (tests/test_gpu_convln.py: the LayerNorm flavour,
csrc/convln.hip; tests/test_gpu_conv_bn.py: the BatchNorm flavour, csrc/conv.hip): the hard graphs, the error measure and the
report that collects every failure of a case before it asserts and prints the worst error per (entry point, output) - which
tests/test_gpu_norm.py (csrc/norm.hip) uses too - and the guard bands (``guarded``, ``guard_input``, ``gptr``) that the pins of
conv.hip, convln.hip, dual.hip and stage.hip (tests/test_gpu_stage_ref.py: integer tables with ``pattern=``) put round every
buffer they hand to a launch."""

import functools
import os
import re
import types

import torch

from alignn_amd import GraphBatch
from alignn_amd.graph import build_csr
from alignn_amd.synthetic import _one, batch_raw, make_batch

DEV = "cuda"
SEG_LENGTHS = (0, 1, 2, 3, 4, 5, 0, 7, 8, 9, 0, 0, 331, 1, 11, 12, 13, 15, 16, 17, 0, 64, 3)  # around multiples of the row unroll 4


@functools.lru_cache(maxsize=None)
def graph(name, device=DEV):
    if name == "synthetic":  # empty segments next to a long one, a one-row segment, lengths on and around multiples of 4
        n = len(SEG_LENGTHS)
        g = torch.Generator().manual_seed(3)
        v = torch.repeat_interleave(torch.arange(n), torch.tensor(SEG_LENGTHS))
        u = torch.randint(0, n, (int(v.numel()),), generator=g)
        return build_csr(u.to(device), v.to(device), n)
    if name == "one_segment":  # five self-loops on the only node: three of the four waves of the only workgroup see nothing
        z = torch.zeros(5, dtype=torch.int64, device=device)
        return build_csr(z, z, 1)
    if name == "no_edges":
        z = torch.zeros(0, dtype=torch.int64, device=device)
        return build_csr(z, z, 3)
    raw = {"lg_small": lambda: make_batch(3, 14, seed0=31), "bond": lambda: make_batch(3, 14, seed0=31),
           "lg_deg17": lambda: make_batch(4, 3, seed0=11),  # atoms with more than 16 in-edges: several dense passes
           "lg_4096seg": lambda: make_batch(8, 60, seed0=5),  # more than 4 x 1024 segments: a wave owns several
           "lg_stream": lambda: make_batch(16, 60, seed0=3),  # >= 128 MiB per [rows, 256] tensor: STREAM = true
           # a one-atom crystal in the batch: every bond of it is a self-image, whose segment omits its own source
           "one_atom_cell": lambda: batch_raw([_one(k, 60 + i, "crystal", 92) for i, k in enumerate((1, 6, 2))])}[name]()
    batch = GraphBatch.from_raw(raw, device=device)
    if name == "bond":
        return batch.g
    lg = batch.lg
    assert lg.dense_max_src > 0 and lg.grp_seg_ptr is not None
    if name == "lg_deg17":
        assert lg.dense_max_src > 16
    if name == "lg_4096seg":
        assert lg.n_nodes > 4096
    if name == "lg_stream":
        assert lg.n_edges * 256 * 4 >= 128 << 20
    if name == "one_atom_cell":
        assert bool(self_image_segments(lg).any())
    return lg


def is_line_graph(g):
    return g.grp_seg_ptr is not None and g.dense_max_src > 0


def self_image_segments(lg):
    """mask over the segments of a dense line graph: the segment's own bond is one of its atom's sources and is left out
    of its rows (the "excluded entry" of alignn_egc_bwd_lg_dense's row arithmetic)"""
    gs, gp, sp = lg.grp_seg_ptr.long(), lg.grp_src_ptr.long(), lg.seg_ptr.long()
    grp = torch.repeat_interleave(torch.arange(gs.numel() - 1, device=gs.device), gs[1:] - gs[:-1])
    node = lg.seg_node.long() if lg.seg_node is not None else torch.arange(lg.n_nodes, device=gs.device)
    beg, end = gp[grp], gp[grp + 1]
    return (node >= beg) & (node < end) & (sp[1:] - sp[:-1] == end - beg - 1)


def err(a, b, floor=1e-30):
    """tests/helpers.rel_err on the device"""
    return float((a.double() - b.double()).abs().max() / b.double().abs().max().clamp_min(floor))


# ----------------------------------------------------------------------------------------------------------------------
# guard bands: the only instrument here for a launch that reads or writes beside a buffer
# ----------------------------------------------------------------------------------------------------------------------
GUARD_MIN, GRANULE = 1024, 128  # elements; 128 float32 = 512 bytes, the granule of torch's caching allocator
NAN_BITS = 0x7FF8A5A5  # a quiet NaN with a payload: torch.full(.., nan) has none, and bits are compared, never floats
# dtype -> (integer view of the same width, guard pattern); integer tensors are index operands: guards of zeros (a valid row)
_PATTERN = {torch.float32: (torch.int32, NAN_BITS), torch.float64: (torch.int64, 0x7FF8A5A5A5A5A5A5),
            torch.float16: (torch.int16, 0x7FA5), torch.bfloat16: (torch.int16, 0x7FA5)}
# ``pattern=`` for index tables: negative (no index, count or offset is) and non-zero in every byte; uint8 is raw scratch
INT_PATTERN = {torch.int32: -0x5A5A5A5B, torch.int64: -0x5A5A5A5A5A5A5A5B, torch.uint8: 0xA5}


def guard_elements(row, itemsize=4):
    """elements on either side of a payload: the larger of GUARD_MIN and two rows, rounded up to whole 512-byte granules"""
    unit = GRANULE * max(1, 4 // itemsize)
    return -(-max(GUARD_MIN, 2 * row) // unit) * unit


class _Guarded:
    def __init__(self, name, base, before, numel, row, pattern=0):
        self.name, self.base, self.before, self.numel, self.row, self.entry = name, base, before, numel, row, None
        self.pattern = pattern  # (integer dtypes only: what their guards hold)

    def sides(self):
        view, pat = _PATTERN.get(self.base.dtype, (self.base.dtype, self.pattern))
        end = self.before + self.numel
        return (("before", self.base[:self.before].view(view), pat), ("after", self.base[end:].view(view), pat))


class Guards:
    """Registry of guarded buffers, each one flat allocation [before | payload | after].  Float guards hold NAN_BITS: a launch
    that writes there changes the bits (``check``), one that reads there and uses the value poisons an output, which
    Report.record rejects.  Integer guards hold zeros and only "unwritten" is checked - a stray zero is not seen - unless the
    buffer is made with ``pattern=``: an integer of the dtype's range that no table can hold (INT_PATTERN), kept in the guards
    and, without ``fill``, in the payload too, so that a stray write of ANY valid value, zero included, and an element of an
    output that was never written both show.  Blind spots: an access farther from the payload than the guard (GUARD_MIN
    elements or two rows) lands in another buffer's payload or outside the registry and is not seen; neither is a read that
    is fetched and never used."""

    def __init__(self):
        self.bufs, self.pending, self.last_entry, self.launches = {}, [], None, {}

    def guarded(self, shape, dtype=torch.float32, fill=None, name="?", device=DEV, row=None, pattern=None):
        if pattern is not None and dtype in _PATTERN:
            raise ValueError(f"pattern= is for integer dtypes: {dtype} guards always hold the NaN pattern")
        shape = tuple(int(s) for s in (shape if isinstance(shape, (tuple, list, torch.Size)) else (shape,)))
        numel = 1
        for s in shape:
            numel *= s
        row = int(row) if row else (shape[-1] if len(shape) >= 2 else 1)
        g = guard_elements(max(row, 1), torch.empty(0, dtype=dtype).element_size())
        base = torch.empty(2 * g + numel, dtype=dtype, device=device)  # a fresh allocation: the payload keeps its alignment
        rec = _Guarded(name, base, g, numel, max(row, 1), 0 if pattern is None else int(pattern))
        for _, side, pat in rec.sides():
            side.fill_(pat)
        # (a tensor of its own on the same storage, not a view of ``base``: autograd and version counters see a fresh tensor)
        payload = torch.empty(0, dtype=dtype, device=device).set_(base.untyped_storage(), g, shape)
        if fill is not None:
            payload.fill_(fill)
        elif dtype in _PATTERN:
            payload.view(_PATTERN[dtype][0]).fill_(_PATTERN[dtype][1])  # (never torch.empty's leftovers: a run is repeatable)
        elif pattern is not None:
            payload.fill_(rec.pattern)
        self.bufs[base.untyped_storage().data_ptr()] = rec
        return payload

    def guard_input(self, t, name="?", pattern=None):
        if t is None:
            return None
        out = self.guarded(t.shape, t.dtype, None, name, t.device, pattern=pattern)
        out.copy_(t)
        return out

    def record_of(self, t, what="tensor"):
        """the registered buffer whose PAYLOAD holds every element of ``t``; raises otherwise"""
        rec = self.bufs.get(t.untyped_storage().data_ptr())
        if rec is None:
            raise AssertionError(f"gptr: {what} {tuple(t.shape)} {t.dtype} is not in a guarded buffer")
        lo = t.storage_offset()
        hi = lo + (sum((n - 1) * st for n, st in zip(t.shape, t.stride())) + 1 if t.numel() else 0)
        if lo < rec.before or hi > rec.before + rec.numel or t.dtype != rec.base.dtype:
            raise AssertionError(f"gptr: a view of {rec.name} covers elements [{lo - rec.before}, {hi - rec.before}) of a payload of "
                                 f"{rec.numel}")
        return rec

    def gptr(self, t):
        if t is None:
            return None
        self.pending.append(self.record_of(t))
        return t.data_ptr()  # (what alignn_amd._lib.ptr returns)

    def launched(self, entry):
        """name the launch that the pointers taken since the last one went to"""
        self.last_entry = entry
        n = self.launches.setdefault(entry, [0, 0])
        n[0] += 1
        n[1] += len({id(r) for r in self.pending})
        for rec in self.pending:
            rec.entry = entry
        self.pending = []

    def check(self):
        """[(name, side, offset, rows, message)] of every guard whose bits changed.  offset: elements from the payload - 0 is the
        first element behind it, -1 the last one in front (the changed element nearest to the payload is reported)."""
        recs = list(self.bufs.values())
        if not recs:
            return []
        flags = torch.stack([(side != pat).any() for rec in recs for _, side, pat in rec.sides()]).tolist()  # one transfer
        found = []
        for i, rec in enumerate(recs):
            for k, (label, side, pat) in enumerate(rec.sides()):
                if not flags[2 * i + k]:
                    continue
                hit = (side != pat).nonzero().flatten()
                off = int(hit[0]) if label == "after" else int(hit[-1]) - rec.before
                rows = off / rec.row
                found.append((rec.name, label, off, rows,
                              f"{rec.name}: the guard {label} the payload changed at offset {off} elements ({rows:+.2f} rows of {rec.row}); "
                              f"last launch handed this buffer: {rec.entry}; last launch: {self.last_entry}"))
        return found


class Launcher:
    """the library, with every call that was handed guarded pointers recorded by name (Guards.launched)"""

    def __init__(self, lib, guards, case=""):
        self._lib, self._guards, self._case = lib, guards, case

    def __getattr__(self, name):
        fn = getattr(self._lib, name)

        def call(*args):
            if self._guards.pending:
                names = _argument_names().get(name, ())
                at = {rec.base.data_ptr() + rec.before * rec.base.element_size(): rec for rec in self._guards.pending}
                for i, a in enumerate(args):  # a buffer allocated without a name takes the one the header gives its argument
                    rec = at.get(a) if isinstance(a, int) and not isinstance(a, bool) else None
                    if rec is not None and rec.name == "?" and i < len(names):
                        rec.name = f"{names[i]} of {name}"
                handed = list(self._guards.pending)
                self._guards.launched(name)
                rc = fn(*args)
                if DIGEST_LOG:
                    _digest(self._case, name, rc, handed)
                return rc
            return fn(*args)
        return call


DIGEST_LOG = os.environ.get("GATE_PARITY_DIGEST")  # a file: one line per launch, to compare two builds of the library bit for bit


def _digest(case, entry, rc, recs):
    """appends "<case> | <entry> <rc> <sum of the bits of every buffer the launch was handed, inputs and outputs>" """
    if recs[0].base.is_cuda:
        torch.cuda.synchronize()
    view = lambda r: r.base[r.before:r.before + r.numel].view(_PATTERN.get(r.base.dtype, (r.base.dtype, 0))[0])  # noqa: E731
    sums = torch.stack([view(r).sum(dtype=torch.int64) for r in recs]).tolist()
    with open(DIGEST_LOG, "a") as f:
        f.write(f"{case} | {entry} {rc} {' '.join(f'{s:x}' for s in sums)}\n")


@functools.lru_cache(maxsize=None)
def _argument_names():
    """entry point -> the parameter names of its prototype in include/alignn_hip.h"""
    from alignn_amd import _abi
    with open(_abi.HEADER) as f:
        text = _abi._uncomment(f.read())
    return {m.group(1): tuple(re.findall(r"(\w+)\s*(?:,|$)", m.group(2))) for m in re.finditer(r"\b(alignn_\w+)\s*\(([^;{}()]*)\)\s*;", text)}


_ACTIVE = Guards()  # the registry of the Report made last


def guarded(shape, dtype=torch.float32, fill=None, name="?", device=DEV, row=None, pattern=None):
    """A contiguous tensor of ``shape`` in the middle of one flat allocation [before | payload | after], registered with the
    current Report.  before == after == guard_elements(row) (``row``: the last dimension unless given), so the payload sits
    where a fresh allocation's would, 512-byte aligned.  ``fill`` None leaves the guard pattern in the payload too
    (``pattern``: what the guards of an INTEGER buffer hold instead of zeros, see Guards).  A stray
    access farther away than the guard lands in another buffer's payload or outside the registry: the helper does not see it
    (see Guards)."""
    return _ACTIVE.guarded(shape, dtype, fill, name, device, row, pattern)


def guard_input(t, name="?", pattern=None):
    """a copy of the operand ``t`` (contiguous, same dtype) inside a guarded buffer; None stays None"""
    return _ACTIVE.guard_input(t, name, pattern)


def gptr(t):
    """alignn_amd._lib.ptr for a tensor that lies inside the payload of a guarded buffer; raises for any other"""
    return _ACTIVE.gptr(t)


GRAPH_TABLES = ("seg_ptr", "seg_node", "src", "dst", "out_ptr", "out_slot", "seg_rank", "grp_seg_ptr", "grp_src_ptr")


def guard_graph(g):
    """the graph's index tables (the cached graph's own stay as they are) as guarded copies; everything else as it is"""
    out = types.SimpleNamespace(**{k: getattr(g, k) for k in ("n_nodes", "n_edges", "dense_max_src")})
    for k in GRAPH_TABLES:
        setattr(out, k, guard_input(getattr(g, k, None), k))
    return out


class Report:
    def __init__(self, case, tag="convln-parity"):
        global _ACTIVE
        self.case, self.tag, self.failed, self.worst = case, tag, [], {}
        self.guards = _ACTIVE = Guards()

    def launcher(self, lib):
        return Launcher(lib, self.guards, self.case)

    def record(self, entry, name, e, e32, allowed):
        key = (entry.split(" ")[0], name)
        if key not in self.worst or e / allowed > self.worst[key][0] / self.worst[key][2]:
            self.worst[key] = (e, e32, allowed, entry)
        if not e < allowed:
            self.failed.append((entry, name, e, e32, allowed))

    def close(self, entry, name, got, ref64, ref32, bound, floor=1e-30):
        if ref64.numel() == 0:  # (a graph without edges: nothing to compare but the shape)
            assert got.shape == ref64.shape
            return
        e = err(got, ref64, floor)
        e32 = None if ref32 is None else err(ref32, ref64, floor)
        self.record(entry, name, e, e32, bound if e32 is None else 4 * e32 + bound)

    def amax(self, entry, name, slot, written):
        got, want = float(slot), float(written.abs().max()) if written.numel() else 0.0
        if got != want:
            self.failed.append((entry, name, got, "amax: largest magnitude written", want))

    def finish(self):
        found = self.guards.check()  # (first: a launch that wrote beside a buffer may have left every compared value alone)
        if self.guards.bufs:
            print(f"{self.tag}-guards {self.case:<38s} buffers {len(self.guards.bufs)}  launches "
                  f"{sum(v[0] for v in self.guards.launches.values())}  findings {len(found)}")
            for entry, (calls, handed) in sorted(self.guards.launches.items()):
                print(f"{self.tag}-guards-entry {entry} launches {calls} buffers {handed}")
        assert not found, [f[4] for f in found]
        for (entry, name), (e, e32, allowed, where) in sorted(self.worst.items()):
            f32 = "       -" if e32 is None else f"{e32:8.2e}"
            print(f"{self.tag} {self.case:<38s} {entry:<32s} {name:<8s} err {e:8.2e}  float32 {f32}  allowed {allowed:8.2e}  [{where}]")
        assert not self.failed, self.failed
