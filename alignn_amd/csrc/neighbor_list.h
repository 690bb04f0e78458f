// What the trajectory analyses share on the device (trajectory.hip, order.hip, local_order.hip): the species of a structure that
// have members, the cell of a (frame, structure) with its inverse and its range of periodic images, and - for the kernels that
// take a wavefront per (frame, centre atom): angles_kernel, cna_kernel, bond_qlm_kernel, bond_finish_kernel - the neighbour list of
// the atom and the fence that lets the wavefront read it.  The list is defined once, here: its order, its cap of 64 and what
// counts as an entry are the contract of include/alignn_order.h and include/alignn_local.h alike.  float64 without contraction;
// tests/order_ref.py (shells) restates the list, tests/traj_ref.py the pair geometry.
#pragma once
#include "common.h"
#include "cell3.h"

#pragma clang fp contract(off)

constexpr int NEIGHBOR_LIST_CAP = 64;  // entries kept, a lane of the wavefront each; the *_MAX_NEIGHBORS of both headers
static_assert(NEIGHBOR_LIST_CAP == ALIGNN_WAVE, "a lane per list entry");

__device__ __forceinline__ void wave_sync() {  // the wavefront's LDS writes are seen by its lanes
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// the species of structure b that have members: groups 1 .. Sb
__device__ __forceinline__ int species_of(const int32_t* group_count, int b, int S) {
    int Sb = 0;
    for (int g = 1; g <= S; ++g)
        if (group_count[b * (S + 1) + g] > 0) Sb = g;
    return Sb;
}

// the cell of structure b in the frame `frame` (an index into the whole trajectory)
__device__ __forceinline__ const double* frame_lattice(const double* lattice, int lattice_per_frame, int n_structs, int frame,
                                                       int b) {
    return lattice + 9 * (lattice_per_frame ? (int64_t)frame * n_structs + b : (int64_t)b);
}

// That cell, its inverse and the images a sphere of radius r reaches; false when the frame is to be skipped (an axis needs more
// than max_range images, or the cell is singular or not finite): the caller raises the status bit of its own header.  The inverse
// is taken either way, so that what the caller adds to the condition (r > 0) joins it in one branch.
__device__ __forceinline__ bool frame_cell(const double* lattice, int lattice_per_frame, int n_structs, int frame, int b, double r,
                                           int max_range, double (&C)[9], double (&Ci)[9], int (&M)[3]) {
    load9(frame_lattice(lattice, lattice_per_frame, n_structs, frame, b), C);
    const bool ok = image_range(C, r, max_range, M);
    inv3_cof(C, Ci);
    return ok;
}

// The neighbour list of atom il of one frame, in the order j ascending, then (m0, m1, m2) lexicographic: (dx, dy, dz, r) of
// entry a into list[a], a < NEIGHBOR_LIST_CAP, with its j into lj[a] (WITH_J) and the group of j into lg[a] (WITH_GROUP).  An
// entry is a (j, image) other than (il, 0) with r < r_cut and a group in 1 .. Sb.  Returns the number found (uniform), which may
// exceed the cap.  All lanes of the wavefront call it, `lane` their index; the caller fences before the list is read (wave_sync).
template <bool WITH_J, bool WITH_GROUP>
__device__ __forceinline__ int build_list(const double* X, const int32_t* GR, int n, int il, int Sb, const double (&C)[9],
                                          const double (&Ci)[9], const int (&M)[3], double r_cut, int lane, double (*list)[4],
                                          int* lj, int* lg) {
    const double xi[3] = {X[3 * il], X[3 * il + 1], X[3 * il + 2]};
    const int w1 = 2 * M[1] + 1, w2 = 2 * M[2] + 1, nimg = (2 * M[0] + 1) * w1 * w2;
    const int64_t total = (int64_t)n * nimg;
    const bool narrow = total < ((int64_t)1 << 31);
    int count = 0;  // (uniform)
    for (int64_t c0 = 0; c0 < total; c0 += ALIGNN_WAVE) {
        const int64_t cand = c0 + lane;
        bool hit = false;
        double dx = 0.0, dy = 0.0, dz = 0.0, r = 0.0;
        int j = 0, gj = 0;
        if (cand < total) {
            int img;
            if (narrow) {
                j = (int)((unsigned)cand / (unsigned)nimg);
                img = (int)((unsigned)cand - (unsigned)j * (unsigned)nimg);
            } else {
                j = (int)(cand / nimg);
                img = (int)(cand - (int64_t)j * nimg);
            }
            const int q2 = img / w2, m2 = img - q2 * w2 - M[2];
            const int q1 = q2 / w1, m1 = q2 - q1 * w1 - M[1], m0 = q1 - M[0];
            gj = GR[j];
            double dp[3], d0[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) dp[c] = X[3 * j + c] - xi[c];
            wrap_difference(dp, C, Ci, d0);
            dx = image_offset(d0, m0, m1, m2, C, 0);
            dy = image_offset(d0, m0, m1, m2, C, 1);
            dz = image_offset(d0, m0, m1, m2, C, 2);
            r = sqrt((dx * dx + dy * dy) + dz * dz);
            const bool self = j == il && m0 == 0 && m1 == 0 && m2 == 0;
            hit = !self && r < r_cut && gj >= 1 && gj <= Sb;
        }
        const unsigned long long mask = __ballot(hit);
        const int at = count + __popcll(mask & ((1ull << lane) - 1ull));
        if (hit && at < NEIGHBOR_LIST_CAP) {
            list[at][0] = dx;
            list[at][1] = dy;
            list[at][2] = dz;
            list[at][3] = r;
            if (WITH_J) lj[at] = j;
            if (WITH_GROUP) lg[at] = gj;
        }
        count += __popcll(mask);
    }
    return count;
}
