// Device side of the van Hove analysis (alignn_amd/vanhove.py): how the pair correlations of a run_md trajectory decay in time,
// for the B structures of a call together.  The reference has none of it; tests/vanhove_ref.py is the numpy restatement,
// include/alignn_vanhove.h states the formulas, the layouts and every field of the argument blocks.
//
//   vh_self_kernel            one workgroup per (lag, structure): a thread walks the origins of its row; r^2, r^4 and j0(q r)
//                             summed per row, then per group in the order of corr_kernel (group_rows.h); r binned into an LDS
//                             histogram of 32-bit counts per species, flushed to the int64 counts with integer atomic adds;
//   vh_self_finish_kernel     one workgroup per (lag, group, structure): moments, alpha2, 4 pi r^2 G_s, G_s, F_s, bin centres;
//   vh_distinct_kernel        one workgroup per (lag, tile of 64 rows i, structure): the pair walk of rdf_counts_kernel per origin,
//                             i of frame t against j of frame t + k in tiles of 64 through LDS, one LDS histogram over all origins;
//   vh_distinct_finish_kernel one workgroup per (lag, pair row, structure): G_d normalised as g(r), the volume, the bin centres;
//   fqt_modes_kernel          one workgroup per (2048 or 1024 vectors, chunk of 64 frames, structure): rho_a(q, t) per species, the
//                             phases of order.hip's sq_accumulate_kernel (sq_modes.h), into the workspace;
//   fqt_correlate_kernel      one thread per (vector, lag, structure): the origins in order, every pair row at once;
//   fqt_bin_kernel            one wavefront per (64 shells, (pair row, lag), structure): the mean over a shell's vectors in order.
// float64, no contraction, no atomics on floating-point values: the histograms are integer (exact, order-free), every
// floating-point sum has a fixed order over the structure's own rows and frames, so a structure's bits are the same alone, in a
// batch and at any place of the batch.
#include "../../include/alignn_vanhove.h"
#include "neighbor_list.h"
#include "group_rows.h"
#include "sq_modes.h"

#pragma clang fp contract(off)

namespace {

constexpr int VH_BLOCK = GROUP_ROWS_BLOCK, VH_TILE = 64, VH_ROUNDS = VH_TILE / (VH_BLOCK / VH_TILE);
constexpr int VH_HIST_CAP = 14336;  // 32-bit counts of the LDS histogram at the most (56 KiB beside the rest)
constexpr int64_t VH_COUNT_MAX = ((int64_t)1 << 31) - 1;  // the terms a workgroup bins between two flushes, at the most
constexpr int SELF_SEGMENT = 1 << 20;                     // origins between two looks at that number
constexpr int MAX_GROUPS = ALIGNN_VH_MAX_SPECIES + 1;
constexpr int SELF_SUMS = 2 + ALIGNN_VH_MAX_Q;  // r^2, r^4, j0(q_u r)
constexpr double PI = 3.14159265358979323846;

using SelfArgs = alignn_vh_self_args;
using DistinctArgs = alignn_vh_distinct_args;
using FqtArgs = alignn_vh_fqt_args;
constexpr int FQT_CHUNK = ALIGNN_VH_FQT_FRAME_CHUNK;
static_assert(ALIGNN_VH_MAX_HKL == ALIGNN_ORDER_MAX_HKL && ALIGNN_VH_MAX_Q_BINS == ALIGNN_ORDER_MAX_BINS, "the vectors of alignn_order_sq_vectors");

__device__ __forceinline__ void add64(int64_t* at, unsigned v) {
    atomicAdd(reinterpret_cast<unsigned long long*>(at), (unsigned long long)v);
}

__global__ __launch_bounds__(VH_BLOCK) void vh_self_kernel(const SelfArgs a, int groups_per_chunk) {
    extern __shared__ unsigned hist[];  // [groups_per_chunk][n_bins + 1]: the last count of a row holds r >= r_max
    __shared__ double part[VH_BLOCK][1];
    __shared__ int grp[VH_BLOCK];
    __shared__ double acc[SELF_SUMS][MAX_GROUPS][1];
    __shared__ double qs[ALIGNN_VH_MAX_Q];
    const int l = blockIdx.x, b = blockIdx.y;
    const int beg = a.atom_ptr[b], n = a.atom_ptr[b + 1] - beg;
    const int k = a.lags[l];
    if (n < 1 || beg < 0 || (int64_t)beg + n > a.n_atoms || k < 0 || k > a.n_frames - 1) return;  // (uniform)
    const int S = a.n_species, G = S + 1, B = a.n_structs, L = a.n_lags, nb = a.n_bins, nq = a.n_q, stride = nb + 1;
    const int Sb = species_of(a.group_count, b, S);
    const int n_or = (a.n_frames - 1 - k) / a.origin_stride + 1;
    const double r_max = a.r_max, scale = (double)nb / r_max;
    const int64_t fstride = 3 * (int64_t)a.n_atoms;
    for (int e = threadIdx.x; e < SELF_SUMS * MAX_GROUPS; e += VH_BLOCK) (&acc[0][0][0])[e] = 0.0;
    if (threadIdx.x < ALIGNN_VH_MAX_Q) qs[threadIdx.x] = threadIdx.x < nq ? a.q[threadIdx.x] : 0.0;

    for (int g0 = 1; g0 == 1 || g0 <= Sb; g0 += groups_per_chunk) {
        const int g1 = min(Sb + 1, g0 + groups_per_chunk), used = max(0, g1 - g0) * stride;
        const bool first = g0 == 1;  // the pass that also takes the sums
        auto flush = [&]() {         // (between two __syncthreads of the caller) adds the histogram to the counts and zeroes it
            for (int e = threadIdx.x; e < used; e += VH_BLOCK) {
                const unsigned v = hist[e];
                if (!v) continue;
                hist[e] = 0u;
                const int lg = e / stride, bin = e - lg * stride;
                const int64_t row = ((int64_t)b * G + (g0 + lg)) * L + l, row0 = ((int64_t)b * G) * L + l;
                if (bin < nb) {
                    add64(a.counts + row * nb + bin, v);
                    add64(a.counts + row0 * nb + bin, v);
                } else {
                    add64(a.overflow + row, v);
                    add64(a.overflow + row0, v);
                }
            }
        };
        for (int e = threadIdx.x; e < used; e += VH_BLOCK) hist[e] = 0u;
        int64_t pending = 0;  // (uniform) the terms binned since the last flush, a full workgroup's for every origin
        __syncthreads();
        for (int c0 = 0; c0 < n; c0 += VH_BLOCK) {
            const int i = c0 + threadIdx.x;
            const int gi = i < n ? a.group[beg + i] : -1;
            const bool binned = gi >= g0 && gi < g1;
            const bool work = i < n && (first || binned);
            const double* X = a.traj + 3 * ((int64_t)beg + (i < n ? i : 0));
            unsigned* H = hist + (binned ? (gi - g0) * stride : 0);
            double s[SELF_SUMS];
#pragma unroll
            for (int c = 0; c < SELF_SUMS; ++c) s[c] = 0.0;
            for (int64_t o0 = 0; o0 < n_or; o0 += SELF_SEGMENT) {
                const int64_t o1 = o0 + SELF_SEGMENT < n_or ? o0 + SELF_SEGMENT : (int64_t)n_or;
                const int64_t terms = (int64_t)VH_BLOCK * (o1 - o0);
                if (pending + terms > VH_COUNT_MAX) {
                    __syncthreads();
                    flush();
                    __syncthreads();
                    pending = 0;
                }
                pending += terms;
                if (!work) continue;
                for (int64_t o = o0; o < o1; ++o) {
                    const int64_t t = o * a.origin_stride;
                    const double* xa = X + (a.frame0 + t * a.frame_step) * fstride;
                    const double* xb = X + (a.frame0 + (t + k) * a.frame_step) * fstride;
                    double d[3];
#pragma unroll
                    for (int c = 0; c < 3; ++c) {
                        const double dc = a.com ? a.com[3 * ((t + k) * B + b) + c] - a.com[3 * (t * B + b) + c] : 0.0;
                        d[c] = (xb[c] - xa[c]) - dc;
                    }
                    const double r2 = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2];
                    const double r = sqrt(r2);
                    if (first) {
                        s[0] = s[0] + r2;
                        s[1] = s[1] + r2 * r2;
#pragma unroll
                        for (int u = 0; u < ALIGNN_VH_MAX_Q; ++u) {
                            if (u < nq) {
                                const double x = qs[u] * r;
                                s[2 + u] = s[2 + u] + (x == 0.0 ? 1.0 : sin(x) / x);
                            }
                        }
                    }
                    if (binned) {
                        const double kb = floor(r * scale);
                        atomicAdd(H + ((r < r_max && kb < (double)nb) ? (int)kb : nb), 1u);
                    }
                }
            }
            if (first) {
#pragma unroll
                for (int c = 0; c < SELF_SUMS; ++c) {
                    if (c < 2 + nq) {    // (uniform)
                        __syncthreads();  // (the last sum's partial sums have been read; acc is zero)
                        part[threadIdx.x][0] = s[c];
                        grp[threadIdx.x] = gi;
                        __syncthreads();
                        group_rows_add<1>(part, grp, acc[c], S);
                    }
                }
            }
        }
        __syncthreads();
        flush();
        __syncthreads();  // (the next chunk zeroes the histogram; acc is complete)
    }
    const int per = 2 + nq;
    if (threadIdx.x < G * per) {
        const int g = threadIdx.x / per, c = threadIdx.x - g * per;
        const int64_t row = ((int64_t)b * G + g) * L + l;
        if (c < 2)
            a.sums[2 * row + c] = acc[c][g][0];
        else
            a.fs_sum[row * nq + (c - 2)] = acc[c][g][0];
    }
}

__global__ __launch_bounds__(VH_BLOCK) void vh_self_finish_kernel(const SelfArgs a) {
    const int l = blockIdx.x, g = blockIdx.y, b = blockIdx.z;
    const int G = a.n_species + 1, L = a.n_lags, nb = a.n_bins, nq = a.n_q;
    const int k = a.lags[l];
    const bool lag_ok = k >= 0 && k <= a.n_frames - 1;
    const double n_or = lag_ok ? (double)((a.n_frames - 1 - k) / a.origin_stride + 1) : 0.0;
    const double Na = (double)a.group_count[b * G + g];
    const bool empty = !(Na > 0.0 && n_or > 0.0);
    const double norm = n_or * Na, dr = a.r_max / (double)nb;
    const int64_t row = ((int64_t)b * G + g) * L + l;
    for (int j = threadIdx.x; j < nb; j += VH_BLOCK) {
        const double r0 = (double)j * dr, r1 = (double)(j + 1) * dr;
        const double shell = (4.0 * PI / 3.0) * ((r1 * r1) * r1 - (r0 * r0) * r0);
        const double c = (double)a.counts[row * nb + j];
        a.p[row * nb + j] = empty ? 0.0 : c / (norm * dr);
        a.gs[row * nb + j] = empty ? 0.0 : c / (norm * shell);
        if (l == 0 && g == 0 && b == 0) a.centres[j] = ((double)j + 0.5) * dr;
    }
    if (threadIdx.x == 0) {
        const double m2 = empty ? 0.0 : a.sums[2 * row] / norm, m4 = empty ? 0.0 : a.sums[2 * row + 1] / norm;
        a.moments[2 * row] = m2;
        a.moments[2 * row + 1] = m4;
        a.alpha2[row] = m2 != 0.0 ? (3.0 * m4) / (5.0 * (m2 * m2)) - 1.0 : 0.0;
    }
    if (threadIdx.x < nq) a.fs[row * nq + threadIdx.x] = empty ? 0.0 : a.fs_sum[row * nq + threadIdx.x] / norm;
}

__global__ __launch_bounds__(VH_BLOCK) void vh_distinct_kernel(const DistinctArgs a, int types_per_chunk) {
    extern __shared__ unsigned hist[];  // [types_per_chunk][n_bins]
    __shared__ double xj[VH_TILE][3];
    __shared__ int gj[VH_TILE];
    const int l = blockIdx.x, tile = blockIdx.y, b = blockIdx.z;
    const int beg = a.atom_ptr[b], n = a.atom_ptr[b + 1] - beg;
    const int k = a.lags[l];
    if (n < 1 || beg < 0 || (int64_t)beg + n > a.n_atoms || tile * VH_TILE >= n || k < 0 || k > a.n_frames - 1) return;  // (uniform)
    const int S = a.n_species, B = a.n_structs, L = a.n_lags;
    const int Sb = species_of(a.group_count, b, S);
    const int types = Sb * (Sb + 1) / 2;
    double C[9], Ci[9];
    int M[3];
    if (!frame_cell(a.lattice, 0, B, 0, b, a.r_max, ALIGNN_VH_MAX_IMAGE_RANGE, C, Ci, M)) {
        if (threadIdx.x == 0) atomicOr(a.status, ALIGNN_VH_STATUS_IMAGES);
        return;
    }
    const int n_or = (a.n_frames - 1 - k) / a.origin_stride + 1;
    const int nb = a.n_bins, P = 1 + S * (S + 1) / 2;
    const double r_max = a.r_max, scale = (double)nb / r_max;
    const int64_t fstride = 3 * (int64_t)a.n_atoms;
    const int64_t tile_terms = (int64_t)VH_TILE * VH_TILE * ((2 * M[0] + 1) * (2 * M[1] + 1) * (2 * M[2] + 1));  // <= 2^12 17^3

    const int il = threadIdx.x & (VH_TILE - 1), jl0 = threadIdx.x / VH_TILE;
    const int i = tile * VH_TILE + il;
    const int32_t* GR = a.group + beg;
    const int gi = i < n ? GR[i] : 0;
    const bool row_ok = i < n && gi >= 1 && gi <= Sb;

    for (int t0 = 0; t0 < types; t0 += types_per_chunk) {
        const int t1 = min(types, t0 + types_per_chunk), used = (t1 - t0) * nb;
        auto flush = [&]() {  // (between two __syncthreads of the caller) adds the histogram to the counts and zeroes it
            for (int e = threadIdx.x; e < used; e += VH_BLOCK) {
                const unsigned v = hist[e];
                if (!v) continue;
                hist[e] = 0u;
                const int lt = e / nb, bin = e - lt * nb;
                add64(a.counts + (((int64_t)b * P + (1 + t0 + lt)) * L + l) * nb + bin, v);
                add64(a.counts + (((int64_t)b * P) * L + l) * nb + bin, v);
            }
        };
        for (int e = threadIdx.x; e < used; e += VH_BLOCK) hist[e] = 0u;
        int64_t pending = 0;  // (uniform) the terms binned since the last flush, a full pair of tiles' for every pair of tiles
        for (int o = 0; o < n_or; ++o) {
            const int64_t t = (int64_t)o * a.origin_stride;
            const double* Xa = a.traj + (a.frame0 + t * a.frame_step) * fstride + 3 * (int64_t)beg;
            const double* Xb = a.traj + (a.frame0 + (t + k) * a.frame_step) * fstride + 3 * (int64_t)beg;
            double ca[3], cb[3], xi[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                ca[c] = a.com ? a.com[3 * (t * B + b) + c] : 0.0;
                cb[c] = a.com ? a.com[3 * ((t + k) * B + b) + c] : 0.0;
                xi[c] = i < n ? Xa[3 * i + c] - ca[c] : 0.0;
            }
            for (int j0 = 0; j0 < n; j0 += VH_TILE) {
                if (pending + tile_terms > VH_COUNT_MAX) {
                    __syncthreads();
                    flush();
                    pending = 0;
                }
                pending += tile_terms;
                __syncthreads();  // (the histogram is zero or flushed; the last tile has been read)
                if (threadIdx.x < VH_TILE) {
                    const int j = j0 + threadIdx.x;
                    const bool in = j < n;
#pragma unroll
                    for (int c = 0; c < 3; ++c) xj[threadIdx.x][c] = in ? Xb[3 * j + c] - cb[c] : 0.0;
                    gj[threadIdx.x] = in ? GR[j] : 0;
                }
                __syncthreads();
                for (int q = 0; q < VH_ROUNDS; ++q) {
                    const int jl = jl0 + q * (VH_BLOCK / VH_TILE), j = j0 + jl;
                    const int gb = gj[jl];
                    if (!row_ok || j >= n || gb < 1 || gb > Sb) continue;
                    const int lo = min(gi, gb), hi = max(gi, gb);
                    const int ty = hi * (hi - 1) / 2 + (lo - 1);
                    if (ty < t0 || ty >= t1) continue;
                    unsigned* H = hist + (ty - t0) * nb;
                    double dp[3], d0[3], shift[3];
#pragma unroll
                    for (int c = 0; c < 3; ++c) dp[c] = xj[jl][c] - xi[c];
                    wrap_difference(dp, C, Ci, d0, shift);
                    for (int m0 = -M[0]; m0 <= M[0]; ++m0) {
                        for (int m1 = -M[1]; m1 <= M[1]; ++m1) {
                            for (int m2 = -M[2]; m2 <= M[2]; ++m2) {
                                // the image of i that is i itself, displaced (d0 + shift C = D): the self part
                                if (i == j && (double)m0 == shift[0] && (double)m1 == shift[1] && (double)m2 == shift[2]) continue;
                                const double dx = image_offset(d0, m0, m1, m2, C, 0), dy = image_offset(d0, m0, m1, m2, C, 1),
                                             dz = image_offset(d0, m0, m1, m2, C, 2);
                                const double r = sqrt((dx * dx + dy * dy) + dz * dz);
                                if (!(r < r_max)) continue;
                                const double kb = floor(r * scale);
                                if (kb >= 0.0 && kb < (double)nb) atomicAdd(H + (int)kb, 1u);
                            }
                        }
                    }
                }
            }
        }
        __syncthreads();
        flush();
        __syncthreads();  // (the next chunk zeroes the histogram)
    }
}

__global__ __launch_bounds__(VH_BLOCK) void vh_distinct_finish_kernel(const DistinctArgs a) {
    const int l = blockIdx.x, p = blockIdx.y, b = blockIdx.z;
    const int S = a.n_species, G = S + 1, L = a.n_lags, nb = a.n_bins, P = 1 + S * (S + 1) / 2;
    int ga = 0, gb = 0;  // the groups of pair row p (row 0: every atom with every atom)
    if (p > 0) {
        int hi = 1;
        while (hi * (hi + 1) / 2 < p) ++hi;  // p - 1 in [hi (hi - 1) / 2, hi (hi + 1) / 2)
        gb = hi;
        ga = p - 1 - hi * (hi - 1) / 2 + 1;
    }
    const int k = a.lags[l];
    const bool lag_ok = k >= 0 && k <= a.n_frames - 1;
    const double n_or = lag_ok ? (double)((a.n_frames - 1 - k) / a.origin_stride + 1) : 0.0;
    const double Na = (double)a.group_count[b * G + ga], Nb = (double)a.group_count[b * G + gb];
    const double w = ga < gb ? 2.0 : 1.0;
    const bool empty = !(Na > 0.0 && Nb > 0.0 && n_or > 0.0);
    double C[9];
    load9(a.lattice + 9 * (int64_t)b, C);
    const double V = fabs(det3_cof(C)), dr = a.r_max / (double)nb;
    const int64_t at = (((int64_t)b * P + p) * L + l) * nb;
    for (int j = threadIdx.x; j < nb; j += VH_BLOCK) {
        const double r0 = (double)j * dr, r1 = (double)(j + 1) * dr;
        const double shell = (4.0 * PI / 3.0) * ((r1 * r1) * r1 - (r0 * r0) * r0);
        a.g[at + j] = empty ? 0.0 : ((double)a.counts[at + j] * V) / ((((n_or * Na) * Nb) * w) * shell);
        if (l == 0 && p == 0 && b == 0) a.centres[j] = ((double)j + 0.5) * dr;
    }
    if (l == 0 && p == 0 && threadIdx.x == 0) a.volume[b] = V;
}

// ---- the intermediate scattering function ----

// NS: the species a thread keeps per vector (S <= NS)
template <int NS>
__global__ __launch_bounds__(SQ_BLOCK) void fqt_modes_kernel(const FqtArgs a) {
    constexpr int VPT = sq_vectors_per_thread(NS), SLAB = SQ_BLOCK * VPT;
    __shared__ SqTile lds;
    const int slab = blockIdx.x, chunk = blockIdx.y, b = blockIdx.z;
    const int beg = a.atom_ptr[b], n = a.atom_ptr[b + 1] - beg;
    const int off = a.vec_ptr[b], V = a.vec_ptr[b + 1] - off;
    if (n < 1 || beg < 0 || (int64_t)beg + n > a.n_atoms || off < 0 || V < 0 || (int64_t)off + V > a.n_vectors || slab * SLAB >= V)
        return;  // (uniform over the workgroup)
    double C[9], Ci[9];
    int H[3];
    load9(a.lattice + 9 * (int64_t)b, C);
    if (!hkl_range(C, a.q_max, H, Ci)) return;  // (such a structure has no vectors: not reached)
    const int S = a.n_species;
    const int64_t Vt = a.n_vectors;
    int i0[VPT], i1[VPT], i2[VPT];
    bool live[VPT];
    sq_thread_vectors<VPT>(a.hkl + 3 * (int64_t)off, V, slab * SLAB, H, i0, i1, i2, live);
    const int f_end = min(a.n_frames, (chunk + 1) * FQT_CHUNK);
    for (int f = chunk * FQT_CHUNK; f < f_end; ++f) {
        const double* X = a.traj + 3 * ((a.frame0 + (int64_t)f * a.frame_step) * a.n_atoms + beg);
        double re[VPT][NS], im[VPT][NS];
        sq_frame_modes<NS, VPT>(X, a.group + beg, n, Ci, H, i0, i1, i2, lds, re, im);
#pragma unroll
        for (int j = 0; j < VPT; ++j) {
            const int v = slab * SLAB + j * SQ_BLOCK + (int)threadIdx.x;
            if (v >= V) continue;
#pragma unroll
            for (int s = 0; s < NS; ++s) {
                if (s < S) {
                    double* out = a.modes + 2 * (((int64_t)f * S + s) * Vt + off + v);
                    out[0] = live[j] ? re[j][s] : 0.0;
                    out[1] = live[j] ? im[j][s] : 0.0;
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

template <int NS>
__global__ __launch_bounds__(VH_BLOCK) void fqt_correlate_kernel(const FqtArgs a) {
    constexpr int ROWS = 1 + NS * (NS + 1) / 2;
    const int v = blockIdx.x * VH_BLOCK + threadIdx.x, l = blockIdx.y, b = blockIdx.z;
    const int off = a.vec_ptr[b], V = a.vec_ptr[b + 1] - off;
    const int k = a.lags[l];
    if (off < 0 || V < 0 || (int64_t)off + V > a.n_vectors || v >= V || k < 0 || k > a.n_frames - 1) return;
    const int S = a.n_species, G = S + 1, L = a.n_lags;
    const int64_t Vt = a.n_vectors;
    const int n_or = (a.n_frames - 1 - k) / a.origin_stride + 1;
    double acc[ROWS];
#pragma unroll
    for (int p = 0; p < ROWS; ++p) acc[p] = 0.0;
    for (int o = 0; o < n_or; ++o) {
        const int64_t t = (int64_t)o * a.origin_stride;
        const double* m0 = a.modes + 2 * ((t * S) * Vt + off + v);        // rho(t): species s at + 2 s Vt
        const double* m1 = a.modes + 2 * (((t + k) * S) * Vt + off + v);  // rho(t + k)
        double re[NS], im[NS], re1[NS], im1[NS];
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            const bool in = s < S;
            re[s] = in ? m0[2 * s * Vt] : 0.0;
            im[s] = in ? m0[2 * s * Vt + 1] : 0.0;
            re1[s] = in ? m1[2 * s * Vt] : 0.0;
            im1[s] = in ? m1[2 * s * Vt + 1] : 0.0;
        }
        double tr = re[0], ti = im[0], tr1 = re1[0], ti1 = im1[0];
#pragma unroll
        for (int s = 1; s < NS; ++s) {
            tr = tr + re[s];
            ti = ti + im[s];
            tr1 = tr1 + re1[s];
            ti1 = ti1 + im1[s];
        }
        acc[0] = acc[0] + (tr * tr1 + ti * ti1);
#pragma unroll
        for (int hi = 0; hi < NS; ++hi) {
#pragma unroll
            for (int lo = 0; lo <= hi; ++lo) {
                if (hi < S) {
                    const double x = lo == hi ? re[lo] * re1[lo] + im[lo] * im1[lo]
                                              : 0.5 * ((re[hi] * re1[lo] + im[hi] * im1[lo]) + (re[lo] * re1[hi] + im[lo] * im1[hi]));
                    acc[1 + hi * (hi + 1) / 2 + lo] = acc[1 + hi * (hi + 1) / 2 + lo] + x;
                }
            }
        }
    }
    const int P = 1 + S * (S + 1) / 2;
#pragma unroll
    for (int p = 0; p < ROWS; ++p) {
        if (p < P) {
            int ga, gb;
            row_groups(p, ga, gb);
            const double Na = (double)a.group_count[b * G + ga], Nb = (double)a.group_count[b * G + gb];
            a.f_vec[((int64_t)p * L + l) * Vt + off + v] = Na > 0.0 && Nb > 0.0 ? acc[p] / ((double)n_or * sqrt(Na * Nb)) : 0.0;
        }
    }
}

__global__ __launch_bounds__(ALIGNN_WAVE) void fqt_bin_kernel(const FqtArgs a) {
    const int S = a.n_species, P = 1 + S * (S + 1) / 2, L = a.n_lags, nb = a.n_bins;
    const int j = blockIdx.x * ALIGNN_WAVE + threadIdx.x, p = blockIdx.y / L, l = blockIdx.y - p * L, b = blockIdx.z;
    int off = a.vec_ptr[b], V = a.vec_ptr[b + 1] - off;
    if (off < 0 || V < 0 || (int64_t)off + V > a.n_vectors) V = 0;
    const double* fv = a.f_vec + ((int64_t)p * L + l) * a.n_vectors + off;
    const int32_t* vb = a.vbin + off;
    double acc = 0.0;
    long long cnt = 0;
    for (int v = 0; v < V; ++v) {
        if (vb[v] == j) {
            acc = acc + fv[v];
            ++cnt;
        }
    }
    if (j < nb) {
        a.f[(((int64_t)b * P + p) * L + l) * nb + j] = cnt > 0 ? acc / (double)cnt : 0.0;
        if (blockIdx.y == 0) a.n_vectors_bin[(int64_t)b * nb + j] = cnt;
        if (blockIdx.y == 0 && b == 0) a.centres[j] = ((double)j + 0.5) * (a.q_max / (double)nb);
    }
}

// the frame selection: every frame used lies inside the trajectory
bool frames_ok(int n_total, int frame0, int step, int n_frames) {
    if (n_total < 0 || frame0 < 0 || step < 1 || n_frames < 0) return false;
    return n_frames == 0 || (int64_t)frame0 + (int64_t)(n_frames - 1) * step < n_total;
}

// what both argument blocks share: the scalars, whose names are the same
template <class Args>
bool common_ok(const Args& a) {
    if (a.n_structs < 0 || a.n_structs > 65535 || a.n_atoms < 0 || a.n_species < 1 || a.n_species > ALIGNN_VH_MAX_SPECIES ||
        a.n_bins < 1 || a.n_bins > ALIGNN_VH_MAX_BINS || a.n_lags < 1 || a.n_lags > ALIGNN_VH_MAX_LAGS || a.origin_stride < 1)
        return false;
    if (!(a.r_max > 0.0) || !(a.r_max < 1e300)) return false;
    return frames_ok(a.n_total_frames, a.frame0, a.frame_step, a.n_frames);
}

// the lags as the host holds them: strictly ascending, each a lag of the frames used
bool lags_ok(const int32_t* lags, int n_lags, int n_frames) {
    for (int l = 0; l < n_lags; ++l)
        if (lags[l] < 0 || lags[l] > n_frames - 1 || (l > 0 && lags[l] <= lags[l - 1])) return false;
    return true;
}

bool self_ok(const SelfArgs& a) { return common_ok(a) && a.n_q >= 0 && a.n_q <= ALIGNN_VH_MAX_Q; }
bool distinct_ok(const DistinctArgs& a) { return common_ok(a) && a.lattice_per_frame == 0; }

bool fqt_ok(const FqtArgs& a) {
    if (a.n_structs < 0 || a.n_structs > 65535 || a.n_atoms < 0 || a.n_species < 1 || a.n_species > ALIGNN_VH_MAX_SPECIES ||
        a.n_bins < 1 || a.n_bins > ALIGNN_VH_MAX_Q_BINS || a.n_lags < 1 || a.n_lags > ALIGNN_VH_MAX_LAGS || a.origin_stride < 1 ||
        a.n_vectors < 0 || a.max_vectors < 0 || a.max_vectors > a.n_vectors || a.lattice_per_frame != 0)
        return false;
    if (!(a.q_max > 0.0) || !(a.q_max < 1e300)) return false;
    return frames_ok(a.n_total_frames, a.frame0, a.frame_step, a.n_frames);
}

}  // namespace

extern "C" size_t alignn_vh_self_args_size(void) { return sizeof(alignn_vh_self_args); }
extern "C" size_t alignn_vh_distinct_args_size(void) { return sizeof(alignn_vh_distinct_args); }
extern "C" size_t alignn_vh_fqt_args_size(void) { return sizeof(alignn_vh_fqt_args); }

extern "C" int alignn_vh_self(const alignn_vh_self_args* args, void* stream) {
    if (!args || !self_ok(*args)) return (int)hipErrorInvalidValue;
    const SelfArgs& a = *args;
    if (a.n_structs == 0 || a.n_frames == 0) return 0;
    if (a.n_atoms < 1) return (int)hipErrorInvalidValue;
    if (!a.traj || !a.atom_ptr || !a.group || !a.group_count || !a.lags || !a.lags_host || !a.counts || !a.overflow || !a.sums ||
        (a.n_q > 0 && (!a.q || !a.fs_sum)))
        return (int)hipErrorInvalidValue;
    if (!lags_ok(a.lags_host, a.n_lags, a.n_frames)) return (int)hipErrorInvalidValue;
    const int stride = a.n_bins + 1;
    const int per_chunk = a.n_species * stride <= VH_HIST_CAP ? a.n_species : VH_HIST_CAP / stride;  // >= 3: n_bins <= 4096
    vh_self_kernel<<<dim3(a.n_lags, a.n_structs), VH_BLOCK, (size_t)per_chunk * stride * sizeof(unsigned), (hipStream_t)stream>>>(
        a, per_chunk);
    ALIGNN_CHECK_LAUNCH();
    return 0;
}

extern "C" int alignn_vh_self_finish(const alignn_vh_self_args* args, void* stream) {
    if (!args || !self_ok(*args)) return (int)hipErrorInvalidValue;
    const SelfArgs& a = *args;
    if (a.n_structs == 0 || a.n_frames == 0) return 0;
    if (!a.group_count || !a.lags || !a.lags_host || !a.counts || !a.sums || !a.moments || !a.alpha2 || !a.p || !a.gs ||
        !a.centres || (a.n_q > 0 && (!a.fs_sum || !a.fs)))
        return (int)hipErrorInvalidValue;
    if (!lags_ok(a.lags_host, a.n_lags, a.n_frames)) return (int)hipErrorInvalidValue;
    vh_self_finish_kernel<<<dim3(a.n_lags, a.n_species + 1, a.n_structs), VH_BLOCK, 0, (hipStream_t)stream>>>(a);
    ALIGNN_CHECK_LAUNCH();
    return 0;
}

extern "C" int alignn_vh_distinct(const alignn_vh_distinct_args* args, void* stream) {
    if (!args || !distinct_ok(*args)) return (int)hipErrorInvalidValue;
    const DistinctArgs& a = *args;
    if (a.n_structs == 0 || a.n_frames == 0) return 0;
    if (a.n_atoms < 1 || a.max_atoms < 1 || a.max_atoms > a.n_atoms) return (int)hipErrorInvalidValue;
    if (!a.traj || !a.lattice || !a.atom_ptr || !a.group || !a.group_count || !a.lags || !a.lags_host || !a.counts || !a.status)
        return (int)hipErrorInvalidValue;
    if (!lags_ok(a.lags_host, a.n_lags, a.n_frames)) return (int)hipErrorInvalidValue;
    const int tiles = alignn_ceil_div(a.max_atoms, VH_TILE);
    if (tiles > 65535) return (int)hipErrorInvalidValue;
    const int types = a.n_species * (a.n_species + 1) / 2;
    const int per_chunk = types * a.n_bins <= VH_HIST_CAP ? types : VH_HIST_CAP / a.n_bins;  // >= 3: n_bins <= 4096
    vh_distinct_kernel<<<dim3(a.n_lags, tiles, a.n_structs), VH_BLOCK, (size_t)per_chunk * a.n_bins * sizeof(unsigned),
                         (hipStream_t)stream>>>(a, per_chunk);
    ALIGNN_CHECK_LAUNCH();
    return 0;
}

extern "C" int alignn_vh_distinct_finish(const alignn_vh_distinct_args* args, void* stream) {
    if (!args || !distinct_ok(*args)) return (int)hipErrorInvalidValue;
    const DistinctArgs& a = *args;
    if (a.n_structs == 0 || a.n_frames == 0) return 0;
    if (!a.lattice || !a.group_count || !a.lags || !a.lags_host || !a.counts || !a.g || !a.volume || !a.centres)
        return (int)hipErrorInvalidValue;
    if (!lags_ok(a.lags_host, a.n_lags, a.n_frames)) return (int)hipErrorInvalidValue;
    vh_distinct_finish_kernel<<<dim3(a.n_lags, 1 + a.n_species * (a.n_species + 1) / 2, a.n_structs), VH_BLOCK, 0,
                                (hipStream_t)stream>>>(a);
    ALIGNN_CHECK_LAUNCH();
    return 0;
}

extern "C" int alignn_vh_fqt_modes(const alignn_vh_fqt_args* args, void* stream) {
    if (!args || !fqt_ok(*args)) return (int)hipErrorInvalidValue;
    const FqtArgs& a = *args;
    if (a.n_structs == 0 || a.n_frames == 0 || a.max_vectors == 0) return 0;
    if (a.n_atoms < 1 || !a.traj || !a.lattice || !a.atom_ptr || !a.group || !a.vec_ptr || !a.hkl || !a.modes)
        return (int)hipErrorInvalidValue;
    const int chunks = alignn_ceil_div(a.n_frames, FQT_CHUNK);
    if (chunks > 65535) return (int)hipErrorInvalidValue;
    const auto grid = [&](int ns) { return dim3(alignn_ceil_div(a.max_vectors, SQ_BLOCK * sq_vectors_per_thread(ns)), chunks, a.n_structs); };
    if (a.n_species <= 1)
        fqt_modes_kernel<1><<<grid(1), SQ_BLOCK, 0, (hipStream_t)stream>>>(a);
    else if (a.n_species <= 2)
        fqt_modes_kernel<2><<<grid(2), SQ_BLOCK, 0, (hipStream_t)stream>>>(a);
    else if (a.n_species <= 4)
        fqt_modes_kernel<4><<<grid(4), SQ_BLOCK, 0, (hipStream_t)stream>>>(a);
    else
        fqt_modes_kernel<8><<<grid(8), SQ_BLOCK, 0, (hipStream_t)stream>>>(a);
    ALIGNN_CHECK_LAUNCH();
    return 0;
}

extern "C" int alignn_vh_fqt_correlate(const alignn_vh_fqt_args* args, void* stream) {
    if (!args || !fqt_ok(*args)) return (int)hipErrorInvalidValue;
    const FqtArgs& a = *args;
    if (a.n_structs == 0 || a.n_frames == 0 || a.max_vectors == 0) return 0;
    if (!a.group_count || !a.vec_ptr || !a.lags || !a.lags_host || !a.modes || !a.f_vec) return (int)hipErrorInvalidValue;
    if (!lags_ok(a.lags_host, a.n_lags, a.n_frames)) return (int)hipErrorInvalidValue;
    const dim3 grid(alignn_ceil_div(a.max_vectors, VH_BLOCK), a.n_lags, a.n_structs);
    if (a.n_species <= 1)
        fqt_correlate_kernel<1><<<grid, VH_BLOCK, 0, (hipStream_t)stream>>>(a);
    else if (a.n_species <= 2)
        fqt_correlate_kernel<2><<<grid, VH_BLOCK, 0, (hipStream_t)stream>>>(a);
    else if (a.n_species <= 4)
        fqt_correlate_kernel<4><<<grid, VH_BLOCK, 0, (hipStream_t)stream>>>(a);
    else
        fqt_correlate_kernel<8><<<grid, VH_BLOCK, 0, (hipStream_t)stream>>>(a);
    ALIGNN_CHECK_LAUNCH();
    return 0;
}

extern "C" int alignn_vh_fqt_bin(const alignn_vh_fqt_args* args, void* stream) {
    if (!args || !fqt_ok(*args)) return (int)hipErrorInvalidValue;
    const FqtArgs& a = *args;
    if (a.n_structs == 0 || a.n_frames == 0) return 0;
    if (!a.vec_ptr || !a.f || !a.n_vectors_bin || !a.centres) return (int)hipErrorInvalidValue;
    if (a.n_vectors > 0 && (!a.f_vec || !a.vbin)) return (int)hipErrorInvalidValue;
    const int P = 1 + a.n_species * (a.n_species + 1) / 2;  // P n_lags <= 37 * 1024
    fqt_bin_kernel<<<dim3(alignn_ceil_div(a.n_bins, ALIGNN_WAVE), P * a.n_lags, a.n_structs), ALIGNN_WAVE, 0, (hipStream_t)stream>>>(a);
    ALIGNN_CHECK_LAUNCH();
    return 0;
}
