"""What the float64 parity tests of the edge-gated convolution kernels share (tests/test_gpu_convln.py: the LayerNorm flavour,
csrc/convln.hip; tests/test_gpu_conv_bn.py: the BatchNorm flavour, csrc/conv.hip): the hard graphs, the error measure and the
report that collects every failure of a case before it asserts and prints the worst error per (entry point, output) - which
tests/test_gpu_norm.py (csrc/norm.hip) uses too."""

import functools

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


class Report:
    def __init__(self, case, tag="convln-parity"):
        self.case, self.tag, self.failed, self.worst = case, tag, [], {}

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
        for (entry, name), (e, e32, allowed, where) in sorted(self.worst.items()):
            f32 = "       -" if e32 is None else f"{e32:8.2e}"
            print(f"{self.tag} {self.case:<38s} {entry:<32s} {name:<8s} err {e:8.2e}  float32 {f32}  allowed {allowed:8.2e}  [{where}]")
        assert not self.failed, self.failed
