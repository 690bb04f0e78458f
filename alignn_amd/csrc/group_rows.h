// The sum over the rows of a group that the time correlations share (trajectory.hip: corr_kernel; vanhove.hip: vh_self_kernel):
// a workgroup of 256 threads holds one partial sum per row of a chunk of 256 rows in LDS, with the row's group; wave w owns the
// groups w, w + 4, ...; a lane adds its rows lane, lane + 64, lane + 128, lane + 192 in that order, then the xor butterfly, and
// lane 0 adds the chunk's sum to the group's accumulator.  The chunks come in row order.  include/alignn_traj.h states this order
// and include/alignn_vanhove.h takes it over.  float64 without contraction.
#pragma once
#include "common.h"

#pragma clang fp contract(off)

constexpr int GROUP_ROWS_BLOCK = 256, GROUP_ROWS_WAVES = GROUP_ROWS_BLOCK / ALIGNN_WAVE;

// part [256][NC] and acc [groups][NC] in LDS, grp [256] the group of every row of the chunk (< 1: no row).  Every thread of the
// workgroup calls it, between two __syncthreads of the caller: part and grp are written, and acc is not read before the next one.
template <int NC>
__device__ __forceinline__ void group_rows_add(const double (*part)[NC], const int* grp, double (*acc)[NC], int S) {
    const int lane = threadIdx.x & (ALIGNN_WAVE - 1), wave = threadIdx.x / ALIGNN_WAVE;
    for (int g = wave; g <= S; g += GROUP_ROWS_WAVES) {
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            double v = 0.0;
#pragma unroll
            for (int q = 0; q < GROUP_ROWS_WAVES; ++q) {
                const int r = lane + ALIGNN_WAVE * q;
                const bool member = grp[r] >= 1 && (g == 0 || grp[r] == g);
                v = v + (member ? part[r][c] : 0.0);
            }
            v = wave_sum(v);
            if (lane == 0) acc[g][c] = acc[g][c] + v;
        }
    }
}
