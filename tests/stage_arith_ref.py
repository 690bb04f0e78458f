"""The index arithmetic of csrc/stage.hip (alignn_stage_batch) restated in numpy line for line: what tests/test_stage_arithmetic.py
compares with the torch builders, and tests/test_stage_ref.py with the definition-only reference of tests/stage_ref.py."""

import numpy as np


def stage_numpy(u, v, N):
    E = u.shape[0]
    perm = np.argsort(v, kind="stable")  # radix sort of (key v, value iota)
    dst = v[perm]
    src = u[perm]
    seg_ptr = np.searchsorted(dst, np.arange(N + 1), side="left")
    out_slot = np.argsort(src, kind="stable")
    out_ptr = np.searchsorted(src[out_slot], np.arange(N + 1), side="left")
    # lg_counts_kernel
    e2 = out_slot
    j = src[e2]
    cnt_seg = seg_ptr[j + 1] - seg_ptr[j] - (dst[e2] == j)
    out_rank = np.empty(E, dtype=np.int64)
    out_rank[e2] = np.arange(E)
    a = dst
    cnt_out = out_ptr[a + 1] - out_ptr[a] - (src == a)
    lg_seg_ptr = np.concatenate([[0], np.cumsum(cnt_seg)])
    lg_out_ptr = np.concatenate([[0], np.cumsum(cnt_out)])
    T = int(lg_seg_ptr[-1])
    assert T == int(lg_out_ptr[-1])
    # lg_rows_kernel
    t = np.arange(T)
    s = np.searchsorted(lg_seg_ptr, t, side="right") - 1
    pos = t - lg_seg_ptr[s]
    e2 = out_slot[s]
    j = src[e2]
    base = seg_ptr[j]
    has_self = dst[e2] == j
    lg_src = base + pos + (has_self & (pos >= e2 - base))
    lg_dst = e2
    # lg_out_slot_kernel
    q = np.arange(T)
    e1 = np.searchsorted(lg_out_ptr, q, side="right") - 1
    pos = q - lg_out_ptr[e1]
    j = dst[e1]
    first = out_ptr[j]
    is_out = src[e1] == j
    s2 = first + pos + (is_out & (pos >= out_rank[e1] - first))
    e2 = out_slot[s2]
    base = seg_ptr[j]
    seg_has_self = dst[e2] == j
    lg_out_slot = lg_seg_ptr[s2] + (e1 - base) - (seg_has_self & (e2 < e1))
    return dict(perm=perm, src=src, dst=dst, seg_ptr=seg_ptr, out_slot=out_slot, out_ptr=out_ptr, lg_seg_ptr=lg_seg_ptr,
                lg_out_ptr=lg_out_ptr, lg_src=lg_src, lg_dst=lg_dst, seg_rank=s, lg_out_slot=lg_out_slot, T=T)
