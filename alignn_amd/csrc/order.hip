// Device side of the structural order analysis (alignn_amd/order.py): bond-angle distributions, Steinhardt q_l and the static
// structure factor for the B structures of a run_md trajectory.  The reference has none of it; tests/order_ref.py is the numpy
// restatement, include/alignn_order.h states the formulas, the layouts and every field of the argument blocks.
//
//   angles_kernel          one workgroup of four wavefronts per (chunk of 64 frames, centre atom, structure), a wavefront per
//                          frame: the neighbour list by ballot and prefix into LDS (neighbor_list.h's build_list, the pair
//                          geometry of trajectory.hip's rdf_counts_kernel), then the pairs of the list lane-strided: the angle
//                          into an LDS histogram of 32-bit counts (LDS integer atomics, flushed with integer atomic adds; rows
//                          that do not fit go in chunks) and the Legendre sums of the Steinhardt parameters (lane-strided, then
//                          the xor butterfly);
//   adf_marginal_kernel, adf_normalise_kernel     the rows of group 0 by integer sums; adf and the bin centres;
//   steinhardt_mean_kernel one wavefront per (frame, structure): the group means in the row order of trajectory.hip's corr_kernel;
//   sq_vectors_kernel      one wavefront per structure: the half space of reciprocal vectors inside q_max, counted or listed in
//                          lexicographic order by ballot and prefix;
//   sq_accumulate_kernel   one workgroup per (2048 or 1024 vectors, chunk of 64 frames, structure): exp(2 pi i h f_k) of 16
//                          atoms at a time tabulated in LDS by sincospi, the phase of (atom, vector) by two complex products;
//   sq_reduce_kernel, sq_bin_kernel               the chunks in order and the normalisation; the shells of |q|.
// float64, no contraction, no atomics on floating-point values: the histogram is integer (exact, order-free), every floating-point
// sum has a fixed order over the structure's own rows, frames and vectors, so a structure's bits are the same alone, in a batch
// and at any place of the batch.
#include "../../include/alignn_order.h"
#include "neighbor_list.h"
#include "sq_modes.h"

#pragma clang fp contract(off)

namespace {

constexpr int ANG_WAVES = 4, ANG_BLOCK = ANG_WAVES * ALIGNN_WAVE, ANG_FRAMES = 64;
constexpr int ANG_HIST_CAP = 4096;  // 32-bit counts of the LDS histogram at the most (16 KiB beside the 9 KiB of the lists)
constexpr int NBR = ALIGNN_ORDER_MAX_NEIGHBORS;
static_assert(NBR == NEIGHBOR_LIST_CAP, "the list of neighbor_list.h");
constexpr int MAX_LS = ALIGNN_ORDER_MAX_LS, MAX_L = ALIGNN_ORDER_MAX_L;
constexpr int MEAN_ROWS = 4;  // rows per lane in a chunk of 256 (corr_kernel's CORR_WAVES)
constexpr int SQ_CHUNK = ALIGNN_ORDER_SQ_FRAME_CHUNK;
constexpr int SMALL_BLOCK = 256;
constexpr double PI = 3.14159265358979323846, TWO_PI = 2.0 * PI;

using AngleArgs = alignn_order_angle_args;
using SqArgs = alignn_order_sq_args;

// the pair index t = k (k - 1) / 2 + j, j < k  ->  (j, k)
__device__ __forceinline__ void pair_of(int t, int& j, int& k) {
    k = (int)((1.0f + sqrtf(1.0f + 8.0f * (float)t)) * 0.5f);
    while (k * (k - 1) / 2 > t) --k;
    while ((k + 1) * k / 2 <= t) ++k;
    j = t - k * (k - 1) / 2;
}

__global__ __launch_bounds__(ANG_BLOCK) void angles_kernel(const AngleArgs a, int rows_per_chunk) {
    extern __shared__ unsigned hist[];       // [rows_per_chunk][n_bins] (with counts)
    __shared__ double nd[ANG_WAVES][NBR][4];  // dx, dy, dz, r of the wavefront's neighbours
    __shared__ int ng[ANG_WAVES][NBR];        // their groups
    const int fc = blockIdx.x, il = blockIdx.y, b = blockIdx.z;
    const int beg = a.atom_ptr[b], n = a.atom_ptr[b + 1] - beg;
    if (n < 1 || beg < 0 || (int64_t)beg + n > a.n_atoms || il >= n) return;  // (uniform over the workgroup)
    const int lane = threadIdx.x & (ALIGNN_WAVE - 1), wave = threadIdx.x / ALIGNN_WAVE;
    const int S = a.n_species, G = S + 1, nb = a.n_bins, P = 1 + S * (S + 1) / 2;
    const int Sb = species_of(a.group_count, b, S);
    const int rows = Sb * (Sb + 1) / 2;
    const int32_t* GR = a.group + beg;
    const int gi = GR[il];
    const bool centre_ok = gi >= 1 && gi <= Sb;
    const double r_cut = a.r_cut[b], scale = (double)nb / PI;
    const bool want_hist = a.counts != nullptr && centre_ok && rows > 0, want_q = a.q != nullptr;
    const int L = a.n_ls;
    const int ls[MAX_LS] = {a.l0, a.l1, a.l2, a.l3};
    int lmax = 0;
#pragma unroll
    for (int u = 0; u < MAX_LS; ++u)
        if (u < L) lmax = max(lmax, ls[u]);
    double(*list)[4] = nd[wave];
    int* lgrp = ng[wave];
    const int passes = want_hist ? (rows + rows_per_chunk - 1) / rows_per_chunk : 1;

    for (int pass = 0; pass < passes; ++pass) {
        const int t0 = pass * rows_per_chunk, t1 = min(rows, t0 + rows_per_chunk), used = want_hist ? (t1 - t0) * nb : 0;
        for (int k = threadIdx.x; k < used; k += ANG_BLOCK) hist[k] = 0u;
        __syncthreads();
        const bool do_q = want_q && pass == 0;
        for (int fl = wave; fl < ANG_FRAMES; fl += ANG_WAVES) {
            const int f = fc * ANG_FRAMES + fl;
            if (f >= a.n_frames) break;  // (uniform over the wavefront; no barrier inside this loop)
            const int frame = a.frame0 + f * a.frame_step;
            double C[9], Ci[9];
            int M[3];
            if (!frame_cell(a.lattice, a.lattice_per_frame, a.n_structs, frame, b, r_cut, ALIGNN_ORDER_MAX_IMAGE_RANGE, C, Ci, M) ||
                !(r_cut > 0.0)) {  // (or r_cut is not a number > 0)
                if (lane == 0) atomicOr(a.status, ALIGNN_ORDER_STATUS_IMAGES);
                continue;
            }
            const double* X = a.traj + 3 * ((int64_t)frame * a.n_atoms + beg);
            const int count = build_list<false, true>(X, GR, n, il, Sb, C, Ci, M, r_cut, lane, list, nullptr, lgrp);
            const int64_t row = (int64_t)f * a.n_atoms + beg + il;
            if (count > NBR) {
                if (lane == 0) {
                    atomicOr(a.status, ALIGNN_ORDER_STATUS_NEIGHBORS);
                    if (do_q) {
                        a.n_neighbors[row] = count;
                        for (int u = 0; u < L; ++u) a.q[row * L + u] = 0.0;
                    }
                }
                continue;
            }
            wave_sync();

            const int npairs = count * (count - 1) / 2;
            double sl[MAX_LS] = {0.0, 0.0, 0.0, 0.0};
            for (int t = lane; t < npairs; t += ALIGNN_WAVE) {
                int j, k;
                pair_of(t, j, k);
                double c = ((list[j][0] * list[k][0] + list[j][1] * list[k][1]) + list[j][2] * list[k][2]) / (list[j][3] * list[k][3]);
                c = c > 1.0 ? 1.0 : c < -1.0 ? -1.0 : c;
                if (do_q) {
                    double pm = 1.0, pn = c;  // P_0, P_1
#pragma unroll
                    for (int d = 1; d <= MAX_L; ++d) {  // pn = P_d
                        if (d <= lmax) {
#pragma unroll
                            for (int u = 0; u < MAX_LS; ++u)
                                if (u < L && ls[u] == d) sl[u] = sl[u] + pn;
                            const double next = (((double)(2 * d + 1) * c) * pn - (double)d * pm) / (double)(d + 1);
                            pm = pn;
                            pn = next;
                        }
                    }
                }
                if (want_hist) {
                    const int ga = lgrp[j], gb = lgrp[k];
                    const int lo = min(ga, gb), hi = max(ga, gb), tr = hi * (hi - 1) / 2 + (lo - 1);
                    if (tr >= t0 && tr < t1) {
                        const double kb = floor(acos(c) * scale);
                        if (kb >= 0.0) atomicAdd(hist + (tr - t0) * nb + (kb < (double)nb ? (int)kb : nb - 1), 1u);  // (not a NaN)
                    }
                }
            }
            if (do_q) {
#pragma unroll
                for (int u = 0; u < MAX_LS; ++u) {
                    if (u < L) {  // (uniform)
                        const double sum = wave_sum(sl[u]), nn = (double)count;
                        double v = count > 0 ? (nn + 2.0 * sum) / (nn * nn) : 0.0;
                        v = v < 0.0 ? 0.0 : v;
                        if (lane == 0) a.q[row * L + u] = sqrt(v);
                    }
                }
                if (lane == 0) a.n_neighbors[row] = count;
            }
            __builtin_amdgcn_wave_barrier();  // (the list is rewritten for the next frame)
        }
        __syncthreads();
        for (int k = threadIdx.x; k < used; k += ANG_BLOCK) {
            const unsigned v = hist[k];
            if (v) {
                const int lt = k / nb, bin = k - lt * nb;
                unsigned long long* row0 = reinterpret_cast<unsigned long long*>(a.counts) + ((int64_t)b * G + gi) * P * nb;
                atomicAdd(row0 + (int64_t)(1 + t0 + lt) * nb + bin, (unsigned long long)v);
            }
        }
        __syncthreads();  // (the next chunk zeroes the histogram)
    }
}

// counts[b][a][0] = sum_{p >= 1} counts[b][a][p] (a >= 1), then counts[b][0][p] = sum_{a >= 1} counts[b][a][p] (every p)
__global__ __launch_bounds__(SMALL_BLOCK) void adf_marginal_kernel(const AngleArgs a) {
    const int b = blockIdx.y, k = blockIdx.x * SMALL_BLOCK + threadIdx.x;
    const int S = a.n_species, G = S + 1, nb = a.n_bins, P = 1 + S * (S + 1) / 2;
    if (k >= nb) return;
    int64_t* Cb = a.counts + (int64_t)b * G * P * nb + k;
    for (int g = 1; g <= S; ++g) {
        int64_t sum = 0;
        for (int p = 1; p < P; ++p) sum += Cb[((int64_t)g * P + p) * nb];
        Cb[((int64_t)g * P) * nb] = sum;
    }
    for (int p = 0; p < P; ++p) {
        int64_t sum = 0;
        for (int g = 1; g <= S; ++g) sum += Cb[((int64_t)g * P + p) * nb];
        Cb[(int64_t)p * nb] = sum;
    }
}

// one wavefront per (row (a, p), structure)
__global__ __launch_bounds__(ALIGNN_WAVE) void adf_normalise_kernel(const AngleArgs a) {
    const int row = blockIdx.x, b = blockIdx.y, lane = threadIdx.x;
    const int S = a.n_species, G = S + 1, nb = a.n_bins, P = 1 + S * (S + 1) / 2;
    const int64_t at = ((int64_t)b * G * P + row) * nb;
    long long part = 0;
    for (int k = lane; k < nb; k += ALIGNN_WAVE) part += a.counts[at + k];
#pragma unroll
    for (int o = ALIGNN_WAVE / 2; o > 0; o >>= 1) part += __shfl_xor(part, o, ALIGNN_WAVE);
    const double w = 180.0 / (double)nb, T = (double)part;
    for (int k = lane; k < nb; k += ALIGNN_WAVE) {
        a.adf[at + k] = part > 0 ? (double)a.counts[at + k] / (T * w) : 0.0;
        if (row == 0 && b == 0) a.theta[k] = ((double)k + 0.5) * w;
    }
}

__global__ __launch_bounds__(ALIGNN_WAVE) void steinhardt_mean_kernel(const AngleArgs a) {
    const int f = blockIdx.x, b = blockIdx.y, lane = threadIdx.x;
    const int beg = a.atom_ptr[b], n = a.atom_ptr[b + 1] - beg;
    const int S = a.n_species, G = S + 1, L = a.n_ls;
    const bool ok = n >= 1 && beg >= 0 && (int64_t)beg + n <= a.n_atoms;
    const double* Q = a.q + ((int64_t)f * a.n_atoms + beg) * L;
    for (int g = 0; g <= S; ++g) {
        const double Na = (double)a.group_count[b * G + g];
        for (int u = 0; u < L; ++u) {
            double acc = 0.0;
            for (int c0 = 0; ok && c0 < n; c0 += MEAN_ROWS * ALIGNN_WAVE) {
                double v = 0.0;
#pragma unroll
                for (int q = 0; q < MEAN_ROWS; ++q) {
                    const int r = c0 + lane + ALIGNN_WAVE * q;
                    double x = 0.0;
                    if (r < n) {
                        const int gr = a.group[beg + r];
                        if (gr >= 1 && (g == 0 || gr == g)) x = Q[(int64_t)r * L + u];
                    }
                    v = v + x;
                }
                acc = acc + wave_sum(v);
            }
            if (lane == 0) a.mean[(((int64_t)b * G + g) * a.n_frames + f) * L + u] = ok && Na > 0.0 ? acc / Na : 0.0;
        }
    }
}

// ---- the static structure factor ----

__global__ __launch_bounds__(ALIGNN_WAVE) void sq_vectors_kernel(const SqArgs a) {
    const int b = blockIdx.x, lane = threadIdx.x;
    double C[9], Ci[9];
    int H[3];
#pragma unroll
    for (int j = 0; j < 9; ++j) C[j] = a.lattice[9 * (int64_t)b + j];
    const bool fill = a.hkl != nullptr;
    if (!hkl_range(C, a.q_max, H, Ci)) {
        if (lane == 0) {
            atomicOr(a.status, ALIGNN_ORDER_STATUS_HKL);
            if (!fill) a.n_vec[b] = 0;
        }
        return;
    }
    const int off = fill ? a.vec_ptr[b] : 0, cap = fill ? a.vec_ptr[b + 1] - off : 0;
    if (fill && (off < 0 || cap < 0 || (int64_t)off + cap > a.n_vectors)) return;
    const int w1 = 2 * H[1] + 1, w2 = 2 * H[2] + 1, total = (H[0] + 1) * w1 * w2;
    const double scale = (double)a.n_bins / a.q_max;
    int count = 0;  // (uniform)
    for (int c0 = 0; c0 < total; c0 += ALIGNN_WAVE) {
        const int cand = c0 + lane;
        bool hit = false;
        int h0 = 0, h1 = 0, h2 = 0;
        double qn = 0.0;
        if (cand < total) {
            const int q2 = cand / w2;
            h2 = cand - q2 * w2 - H[2];
            h0 = q2 / w1;
            h1 = q2 - h0 * w1 - H[1];
            const double x0 = (double)h0, x1 = (double)h1, x2 = (double)h2;
            const double qx = TWO_PI * ((x0 * Ci[0] + x1 * Ci[1]) + x2 * Ci[2]);
            const double qy = TWO_PI * ((x0 * Ci[3] + x1 * Ci[4]) + x2 * Ci[5]);
            const double qz = TWO_PI * ((x0 * Ci[6] + x1 * Ci[7]) + x2 * Ci[8]);
            qn = sqrt((qx * qx + qy * qy) + qz * qz);
            const bool half = h0 > 0 || (h0 == 0 && (h1 > 0 || (h1 == 0 && h2 > 0)));
            hit = half && qn < a.q_max;
        }
        const unsigned long long mask = __ballot(hit);
        const int at = count + __popcll(mask & ((1ull << lane) - 1ull));
        if (fill && hit && at < cap) {
            const int64_t v = (int64_t)off + at;
            a.hkl[3 * v] = h0;
            a.hkl[3 * v + 1] = h1;
            a.hkl[3 * v + 2] = h2;
            a.qnorm[v] = qn;
            const double kb = floor(qn * scale);
            a.vbin[v] = kb < (double)a.n_bins ? (int)kb : a.n_bins - 1;
        }
        count += __popcll(mask);
    }
    if (!fill && lane == 0) a.n_vec[b] = count;
}

// NS: the species accumulators a thread keeps per vector (S <= NS)
template <int NS>
__global__ __launch_bounds__(SQ_BLOCK) void sq_accumulate_kernel(const SqArgs a) {
    constexpr int SQ_VPT = sq_vectors_per_thread(NS), SQ_SLAB = SQ_BLOCK * SQ_VPT;
    __shared__ SqTile lds;
    const int slab = blockIdx.x, chunk = blockIdx.y, b = blockIdx.z, tid = threadIdx.x;
    const int beg = a.atom_ptr[b], n = a.atom_ptr[b + 1] - beg;
    const int off = a.vec_ptr[b], V = a.vec_ptr[b + 1] - off;
    if (n < 1 || beg < 0 || (int64_t)beg + n > a.n_atoms || off < 0 || V < 0 || (int64_t)off + V > a.n_vectors ||
        slab * SQ_SLAB >= V)
        return;  // (uniform over the workgroup)
    double C[9], Ci[9];
    int H[3];
#pragma unroll
    for (int j = 0; j < 9; ++j) C[j] = a.lattice[9 * (int64_t)b + j];
    if (!hkl_range(C, a.q_max, H, Ci)) return;  // (such a structure has no vectors: not reached)
    const int S = a.n_species, P = 1 + S * (S + 1) / 2;
    const int64_t Vt = a.n_vectors;

    int i0[SQ_VPT], i1[SQ_VPT], i2[SQ_VPT];
    bool live[SQ_VPT];
    sq_thread_vectors<SQ_VPT>(a.hkl + 3 * (int64_t)off, V, slab * SQ_SLAB, H, i0, i1, i2, live);

    const int f_end = min(a.n_frames, (chunk + 1) * SQ_CHUNK);
    for (int f = chunk * SQ_CHUNK; f < f_end; ++f) {
        const double* X = a.traj + 3 * ((int64_t)(a.frame0 + f * a.frame_step) * a.n_atoms + beg);
        double re[SQ_VPT][NS], im[SQ_VPT][NS];
        sq_frame_modes<NS, SQ_VPT>(X, a.group + beg, n, Ci, H, i0, i1, i2, lds, re, im);  // (sq_modes.h)
        const bool first = f == chunk * SQ_CHUNK;
#pragma unroll
        for (int j = 0; j < SQ_VPT; ++j) {
            if (!live[j]) continue;
            double* out = a.partial + (int64_t)chunk * P * Vt + off + (slab * SQ_SLAB + j * SQ_BLOCK + tid);
            double tr = re[j][0], ti = im[j][0];
#pragma unroll
            for (int s = 1; s < NS; ++s) {
                tr = tr + re[j][s];
                ti = ti + im[j][s];
            }
            const double all = tr * tr + ti * ti;
            out[0] = first ? all : out[0] + all;
#pragma unroll
            for (int hi = 0; hi < NS; ++hi) {
#pragma unroll
                for (int lo = 0; lo <= hi; ++lo) {
                    if (hi < S) {
                        const double v = re[j][lo] * re[j][hi] + im[j][lo] * im[j][hi];
                        double* o = out + (int64_t)(1 + hi * (hi + 1) / 2 + lo) * Vt;
                        *o = first ? v : *o + v;
                    }
                }
            }
        }
    }
}

// the row p -> its groups (a <= b; row 0: 0, 0)
__device__ __forceinline__ void row_groups(int p, int& ga, int& gb) {
    ga = gb = 0;
    if (p > 0) {
        int hi = 1;
        while (hi * (hi + 1) / 2 < p) ++hi;
        gb = hi;
        ga = p - 1 - hi * (hi - 1) / 2 + 1;
    }
}

__global__ __launch_bounds__(SMALL_BLOCK) void sq_reduce_kernel(const SqArgs a) {
    const int p = blockIdx.y, b = blockIdx.z, v = blockIdx.x * SMALL_BLOCK + threadIdx.x;
    const int off = a.vec_ptr[b], V = a.vec_ptr[b + 1] - off;
    if (off < 0 || V < 0 || (int64_t)off + V > a.n_vectors || v >= V) return;
    const int S = a.n_species, G = S + 1, P = 1 + S * (S + 1) / 2;
    const int chunks = (a.n_frames + SQ_CHUNK - 1) / SQ_CHUNK;
    int ga, gb;
    row_groups(p, ga, gb);
    const double Na = (double)a.group_count[b * G + ga], Nb = (double)a.group_count[b * G + gb];
    double sum = 0.0;
    for (int c = 0; c < chunks; ++c) sum = sum + a.partial[((int64_t)c * P + p) * a.n_vectors + off + v];
    const bool empty = !(Na > 0.0 && Nb > 0.0 && a.n_frames > 0);
    a.s_vec[(int64_t)p * a.n_vectors + off + v] = empty ? 0.0 : sum / ((double)a.n_frames * sqrt(Na * Nb));
}

__global__ __launch_bounds__(ALIGNN_WAVE) void sq_bin_kernel(const SqArgs a) {
    const int p = blockIdx.y, b = blockIdx.z, k = blockIdx.x * ALIGNN_WAVE + threadIdx.x;
    const int S = a.n_species, P = 1 + S * (S + 1) / 2, nb = a.n_bins;
    int off = a.vec_ptr[b], V = a.vec_ptr[b + 1] - off;
    if (off < 0 || V < 0 || (int64_t)off + V > a.n_vectors) V = 0;
    const double* sv = a.s_vec + (int64_t)p * a.n_vectors + off;
    const int32_t* vb = a.vbin + off;
    double acc = 0.0;
    long long cnt = 0;
    for (int v = 0; v < V; ++v) {
        if (vb[v] == k) {
            acc = acc + sv[v];
            ++cnt;
        }
    }
    if (k < nb) {
        a.s[((int64_t)b * P + p) * nb + k] = cnt > 0 ? acc / (double)cnt : 0.0;
        if (p == 0) a.n_vectors_bin[(int64_t)b * nb + k] = cnt;
        if (p == 0 && b == 0) a.centres[k] = ((double)k + 0.5) * (a.q_max / (double)nb);
    }
}

// the frame selection of both argument blocks: every frame used lies inside the trajectory
bool frames_ok(int n_total, int frame0, int step, int n_frames) {
    if (n_total < 0 || frame0 < 0 || step < 1 || n_frames < 0) return false;
    return n_frames == 0 || (int64_t)frame0 + (int64_t)(n_frames - 1) * step < n_total;
}

bool angle_args_ok(const AngleArgs& a) {
    if (a.n_structs < 0 || a.n_structs > 65535 || a.n_atoms < 0 || a.n_species < 1 || a.n_species > ALIGNN_ORDER_MAX_SPECIES ||
        a.n_bins < 1 || a.n_bins > ALIGNN_ORDER_MAX_BINS || a.lattice_per_frame < 0 || a.lattice_per_frame > 1 || a.n_ls < 0 ||
        a.n_ls > MAX_LS)
        return false;
    const int ls[MAX_LS] = {a.l0, a.l1, a.l2, a.l3};
    for (int u = 0; u < a.n_ls; ++u) {
        if (ls[u] < 1 || ls[u] > MAX_L) return false;
        for (int w = 0; w < u; ++w)
            if (ls[w] == ls[u]) return false;
    }
    return frames_ok(a.n_total_frames, a.frame0, a.frame_step, a.n_frames);
}

bool sq_args_ok(const SqArgs& a) {
    if (a.n_structs < 0 || a.n_structs > 65535 || a.n_atoms < 0 || a.n_species < 1 || a.n_species > ALIGNN_ORDER_MAX_SPECIES ||
        a.n_bins < 1 || a.n_bins > ALIGNN_ORDER_MAX_BINS || a.n_vectors < 0 || a.max_vectors < 0 || a.max_vectors > a.n_vectors)
        return false;
    if (!(a.q_max > 0.0) || !(a.q_max < 1e300)) return false;
    return frames_ok(a.n_total_frames, a.frame0, a.frame_step, a.n_frames);
}

}  // namespace

extern "C" size_t alignn_order_angle_args_size(void) { return sizeof(alignn_order_angle_args); }
extern "C" size_t alignn_order_sq_args_size(void) { return sizeof(alignn_order_sq_args); }

extern "C" int alignn_order_angles(const alignn_order_angle_args* args, void* stream) {
    if (!args || !angle_args_ok(*args)) return (int)hipErrorInvalidValue;
    const AngleArgs& a = *args;
    if (a.n_structs == 0 || a.n_frames == 0) return 0;
    if (a.n_atoms < 1 || a.max_atoms < 1 || a.max_atoms > a.n_atoms || a.max_atoms > 65535) return (int)hipErrorInvalidValue;
    if (!a.traj || !a.lattice || !a.atom_ptr || !a.group || !a.group_count || !a.r_cut || !a.status) return (int)hipErrorInvalidValue;
    if (!a.counts && !a.q) return (int)hipErrorInvalidValue;
    if (a.q && (a.n_ls < 1 || !a.n_neighbors)) return (int)hipErrorInvalidValue;
    const int rows = a.n_species * (a.n_species + 1) / 2;
    const int per_chunk = rows * a.n_bins <= ANG_HIST_CAP ? rows : ANG_HIST_CAP / a.n_bins;  // >= 4: n_bins <= 1024
    const size_t lds = a.counts ? (size_t)per_chunk * a.n_bins * sizeof(unsigned) : 0;
    angles_kernel<<<dim3(alignn_ceil_div(a.n_frames, ANG_FRAMES), a.max_atoms, a.n_structs), ANG_BLOCK, lds, (hipStream_t)stream>>>(
        a, per_chunk);
    ALIGNN_CHECK_LAUNCH();
    return 0;
}

extern "C" int alignn_order_adf_finish(const alignn_order_angle_args* args, void* stream) {
    if (!args || !angle_args_ok(*args)) return (int)hipErrorInvalidValue;
    const AngleArgs& a = *args;
    if (a.n_structs == 0) return 0;
    if (!a.counts || !a.adf || !a.theta) return (int)hipErrorInvalidValue;
    const int G = a.n_species + 1, P = 1 + a.n_species * (a.n_species + 1) / 2;
    adf_marginal_kernel<<<dim3(alignn_ceil_div(a.n_bins, SMALL_BLOCK), a.n_structs), SMALL_BLOCK, 0, (hipStream_t)stream>>>(a);
    ALIGNN_CHECK_LAUNCH();
    adf_normalise_kernel<<<dim3(G * P, a.n_structs), ALIGNN_WAVE, 0, (hipStream_t)stream>>>(a);
    ALIGNN_CHECK_LAUNCH();
    return 0;
}

extern "C" int alignn_order_steinhardt_mean(const alignn_order_angle_args* args, void* stream) {
    if (!args || !angle_args_ok(*args)) return (int)hipErrorInvalidValue;
    const AngleArgs& a = *args;
    if (a.n_structs == 0 || a.n_frames == 0) return 0;
    if (a.n_ls < 1 || a.n_atoms < 1 || !a.atom_ptr || !a.group || !a.group_count || !a.q || !a.mean) return (int)hipErrorInvalidValue;
    steinhardt_mean_kernel<<<dim3(a.n_frames, a.n_structs), ALIGNN_WAVE, 0, (hipStream_t)stream>>>(a);
    ALIGNN_CHECK_LAUNCH();
    return 0;
}

extern "C" int alignn_order_sq_vectors(const alignn_order_sq_args* args, void* stream) {
    if (!args || !sq_args_ok(*args)) return (int)hipErrorInvalidValue;
    const SqArgs& a = *args;
    if (a.n_structs == 0) return 0;
    if (!a.lattice || !a.status) return (int)hipErrorInvalidValue;
    if (a.hkl ? (!a.vec_ptr || !a.qnorm || !a.vbin) : !a.n_vec) return (int)hipErrorInvalidValue;
    sq_vectors_kernel<<<a.n_structs, ALIGNN_WAVE, 0, (hipStream_t)stream>>>(a);
    ALIGNN_CHECK_LAUNCH();
    return 0;
}

extern "C" int alignn_order_sq_accumulate(const alignn_order_sq_args* args, void* stream) {
    if (!args || !sq_args_ok(*args)) return (int)hipErrorInvalidValue;
    const SqArgs& a = *args;
    if (a.n_structs == 0 || a.n_frames == 0 || a.max_vectors == 0) return 0;
    if (a.n_atoms < 1 || !a.traj || !a.lattice || !a.atom_ptr || !a.group || !a.vec_ptr || !a.hkl || !a.partial)
        return (int)hipErrorInvalidValue;
    const int chunks = alignn_ceil_div(a.n_frames, SQ_CHUNK);
    if (chunks > 65535) return (int)hipErrorInvalidValue;
    const auto grid = [&](int ns) { return dim3(alignn_ceil_div(a.max_vectors, SQ_BLOCK * sq_vectors_per_thread(ns)), chunks, a.n_structs); };
    if (a.n_species <= 1)
        sq_accumulate_kernel<1><<<grid(1), SQ_BLOCK, 0, (hipStream_t)stream>>>(a);
    else if (a.n_species <= 2)
        sq_accumulate_kernel<2><<<grid(2), SQ_BLOCK, 0, (hipStream_t)stream>>>(a);
    else if (a.n_species <= 4)
        sq_accumulate_kernel<4><<<grid(4), SQ_BLOCK, 0, (hipStream_t)stream>>>(a);
    else
        sq_accumulate_kernel<8><<<grid(8), SQ_BLOCK, 0, (hipStream_t)stream>>>(a);
    ALIGNN_CHECK_LAUNCH();
    return 0;
}

extern "C" int alignn_order_sq_bin(const alignn_order_sq_args* args, void* stream) {
    if (!args || !sq_args_ok(*args)) return (int)hipErrorInvalidValue;
    const SqArgs& a = *args;
    if (a.n_structs == 0) return 0;
    if (!a.group_count || !a.vec_ptr || !a.s || !a.n_vectors_bin || !a.centres) return (int)hipErrorInvalidValue;
    if (a.n_vectors > 0 && (!a.partial || !a.s_vec || !a.vbin)) return (int)hipErrorInvalidValue;
    if ((int64_t)a.n_frames > (int64_t)65535 * SQ_CHUNK) return (int)hipErrorInvalidValue;
    const int P = 1 + a.n_species * (a.n_species + 1) / 2;
    if (a.max_vectors > 0) {
        sq_reduce_kernel<<<dim3(alignn_ceil_div(a.max_vectors, SMALL_BLOCK), P, a.n_structs), SMALL_BLOCK, 0, (hipStream_t)stream>>>(a);
        ALIGNN_CHECK_LAUNCH();
    }
    sq_bin_kernel<<<dim3(alignn_ceil_div(a.n_bins, ALIGNN_WAVE), P, a.n_structs), ALIGNN_WAVE, 0, (hipStream_t)stream>>>(a);
    ALIGNN_CHECK_LAUNCH();
    return 0;
}
