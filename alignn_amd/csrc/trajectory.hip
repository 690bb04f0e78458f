// Device side of the trajectory analysis (alignn_amd/trajectory.py): the radial distribution function, the mean squared
// displacement, the velocity autocorrelation and what is derived from them (density of states, Einstein fit, Green-Kubo integral)
// for the B structures of a run_md trajectory.  The reference has none of it; tests/traj_ref.py is the numpy restatement,
// include/alignn_traj.h states the formulas, the layouts and every field of the argument blocks.
//
//   rdf_counts_kernel      one workgroup per (frame, tile of 64 rows i, structure): j in tiles of 64 through LDS, every periodic
//                          image of the pair, an LDS histogram of 32-bit counts per pair type (LDS integer atomics), flushed to the
//                          int64 counts with integer atomic adds; pair types that do not fit the histogram go in chunks;
//   rdf_volume_kernel      one thread per structure: the mean cell volume in frame order;
//   rdf_normalise_kernel   one workgroup per (pair type, structure): g(r), the running coordination number, the bin centres;
//   com_kernel             one thread per (frame, structure): the centre of mass in row order;
//   corr_kernel<MODE>      one workgroup per (lag, structure): MSD (per component) or VACF, one body;
//   vdos_kernel, fit_kernel, green_kubo_kernel.
// float64, no contraction, no atomics on floating-point values: the histogram is integer (exact, order-free), every floating-point
// sum has a fixed order over the structure's own rows and frames, so a structure's bits are the same alone, in a batch and at any
// place of the batch.
#include "../../include/alignn_traj.h"
#include "neighbor_list.h"
#include "group_rows.h"

#pragma clang fp contract(off)

namespace {

constexpr int RDF_BLOCK = 256, RDF_TILE = 64, RDF_ROUNDS = RDF_TILE / (RDF_BLOCK / RDF_TILE);
constexpr int RDF_HIST_CAP = 14336;  // 32-bit counts of the LDS histogram at the most (56 KiB beside the j tile)
constexpr int CORR_BLOCK = GROUP_ROWS_BLOCK;
constexpr int MAX_GROUPS = ALIGNN_TRAJ_MAX_SPECIES + 1;
constexpr int SMALL_BLOCK = 256, SMALL_MAX_BLOCKS = 4096;
constexpr double PI = 3.14159265358979323846;

using RdfArgs = alignn_traj_rdf_args;
using CorrArgs = alignn_traj_corr_args;

__global__ __launch_bounds__(RDF_BLOCK) void rdf_counts_kernel(const RdfArgs a, int types_per_chunk) {
    extern __shared__ unsigned hist[];  // [types_per_chunk][n_bins]
    __shared__ double xj[RDF_TILE][3];
    __shared__ int gj[RDF_TILE];
    const int f = blockIdx.x, tile = blockIdx.y, b = blockIdx.z;
    const int beg = a.atom_ptr[b], n = a.atom_ptr[b + 1] - beg;
    if (n < 1 || beg < 0 || (int64_t)beg + n > a.n_atoms || tile * RDF_TILE >= n) return;  // (uniform over the workgroup)
    const int S = a.n_species;
    const int Sb = species_of(a.group_count, b, S);
    const int types = Sb * (Sb + 1) / 2;
    const int frame = a.frame0 + f * a.frame_step;
    double C[9], Ci[9];
    int M[3];
    if (!frame_cell(a.lattice, a.lattice_per_frame, a.n_structs, frame, b, a.r_max, ALIGNN_TRAJ_MAX_IMAGE_RANGE, C, Ci, M)) {
        if (threadIdx.x == 0) atomicOr(a.status, ALIGNN_TRAJ_STATUS_IMAGES);
        return;
    }
    const double* X = a.traj + 3 * ((int64_t)frame * a.n_atoms + beg);
    const int32_t* GR = a.group + beg;
    const int nb = a.n_bins, P = 1 + S * (S + 1) / 2;
    const double r_max = a.r_max, scale = (double)nb / r_max;

    const int il = threadIdx.x & (RDF_TILE - 1), jl0 = threadIdx.x / RDF_TILE;
    const int i = tile * RDF_TILE + il;
    double xi[3] = {0.0, 0.0, 0.0};
    int gi = 0;
    if (i < n) {
#pragma unroll
        for (int c = 0; c < 3; ++c) xi[c] = X[3 * i + c];
        gi = GR[i];
    }
    const bool row_ok = i < n && gi >= 1 && gi <= Sb;

    for (int t0 = 0; t0 < types; t0 += types_per_chunk) {
        const int t1 = min(types, t0 + types_per_chunk), used = (t1 - t0) * nb;
        for (int k = threadIdx.x; k < used; k += RDF_BLOCK) hist[k] = 0u;
        for (int j0 = 0; j0 < n; j0 += RDF_TILE) {
            __syncthreads();  // (the histogram is zero; the last tile has been read)
            if (threadIdx.x < RDF_TILE) {
                const int j = j0 + threadIdx.x;
                const bool in = j < n;
#pragma unroll
                for (int c = 0; c < 3; ++c) xj[threadIdx.x][c] = in ? X[3 * j + c] : 0.0;
                gj[threadIdx.x] = in ? GR[j] : 0;
            }
            __syncthreads();
            for (int q = 0; q < RDF_ROUNDS; ++q) {
                const int jl = jl0 + q * (RDF_BLOCK / RDF_TILE), j = j0 + jl;
                const int gb = gj[jl];
                if (!row_ok || j >= n || gb < 1 || gb > Sb) continue;
                const int lo = min(gi, gb), hi = max(gi, gb);
                const int t = hi * (hi - 1) / 2 + (lo - 1);
                if (t < t0 || t >= t1) continue;
                unsigned* H = hist + (t - t0) * nb;
                double dp[3], d0[3];
#pragma unroll
                for (int c = 0; c < 3; ++c) dp[c] = xj[jl][c] - xi[c];
                wrap_difference(dp, C, Ci, d0);
                for (int m0 = -M[0]; m0 <= M[0]; ++m0) {
                    for (int m1 = -M[1]; m1 <= M[1]; ++m1) {
                        for (int m2 = -M[2]; m2 <= M[2]; ++m2) {
                            if (i == j && m0 == 0 && m1 == 0 && m2 == 0) continue;
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
        __syncthreads();
        for (int k = threadIdx.x; k < used; k += RDF_BLOCK) {
            const unsigned v = hist[k];
            if (v) {
                const int lt = k / nb, bin = k - lt * nb;
                unsigned long long* row0 = reinterpret_cast<unsigned long long*>(a.counts) + (int64_t)b * P * nb;
                atomicAdd(row0 + (int64_t)(1 + t0 + lt) * nb + bin, (unsigned long long)v);
                atomicAdd(row0 + bin, (unsigned long long)v);
            }
        }
        __syncthreads();  // (the next chunk zeroes the histogram)
    }
}

__global__ void rdf_volume_kernel(const RdfArgs a) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= a.n_structs) return;
    double sum = 0.0;
    for (int f = 0; f < a.n_frames; ++f) {
        double C[9];
        load9(frame_lattice(a.lattice, a.lattice_per_frame, a.n_structs, a.frame0 + f * a.frame_step, b), C);
        sum = sum + fabs(det3_cof(C));
    }
    a.volume[b] = a.n_frames > 0 ? sum / (double)a.n_frames : 0.0;
}

__global__ __launch_bounds__(SMALL_BLOCK) void rdf_normalise_kernel(const RdfArgs a) {
    const int p = blockIdx.x, b = blockIdx.y;
    const int S = a.n_species, G = S + 1, nb = a.n_bins, P = 1 + S * (S + 1) / 2;
    int ga = 0, gb = 0;  // the groups of pair type p (row 0: every atom with every atom)
    if (p > 0) {
        int hi = 1;
        while (hi * (hi + 1) / 2 < p) ++hi;  // p - 1 in [hi (hi - 1) / 2, hi (hi + 1) / 2)
        gb = hi;
        ga = p - 1 - hi * (hi - 1) / 2 + 1;
    }
    const double Na = (double)a.group_count[b * G + ga], Nb = (double)a.group_count[b * G + gb];
    const double w = ga < gb ? 2.0 : 1.0, F = (double)a.n_frames;
    const bool empty = !(Na > 0.0 && Nb > 0.0 && F > 0.0);
    const double V = a.volume[b], dr = a.r_max / (double)nb;
    const int64_t at = ((int64_t)b * P + p) * nb;
    for (int k = threadIdx.x; k < nb; k += SMALL_BLOCK) {
        const double r0 = (double)k * dr, r1 = (double)(k + 1) * dr;
        const double shell = (4.0 * PI / 3.0) * ((r1 * r1) * r1 - (r0 * r0) * r0);
        a.g[at + k] = empty ? 0.0 : ((double)a.counts[at + k] * V) / ((((F * Na) * Nb) * w) * shell);
        if (p == 0 && b == 0) a.centres[k] = ((double)k + 0.5) * dr;
    }
    if (threadIdx.x == 0) {
        int64_t run = 0;
        for (int k = 0; k < nb; ++k) {
            run += a.counts[at + k];
            a.coord[at + k] = empty ? 0.0 : (double)run / ((F * Na) * w);
        }
    }
}

__global__ __launch_bounds__(SMALL_BLOCK) void com_kernel(const CorrArgs a) {
    const int64_t total = (int64_t)a.n_frames * a.n_structs;
    for (int64_t w = (int64_t)blockIdx.x * SMALL_BLOCK + threadIdx.x; w < total; w += (int64_t)gridDim.x * SMALL_BLOCK) {
        const int t = (int)(w / a.n_structs), b = (int)(w - (int64_t)t * a.n_structs);
        const int beg = a.atom_ptr[b], n = a.atom_ptr[b + 1] - beg;
        double s[3] = {0.0, 0.0, 0.0}, mt = 0.0;
        if (n >= 1 && beg >= 0 && (int64_t)beg + n <= a.n_atoms) {
            const double* X = a.traj + 3 * ((int64_t)(a.frame0 + t * a.frame_step) * a.n_atoms + beg);
            for (int i = 0; i < n; ++i) {
                const double m = a.masses[beg + i];
#pragma unroll
                for (int c = 0; c < 3; ++c) s[c] = s[c] + m * X[3 * i + c];
                mt = mt + m;
            }
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) a.com[3 * w + c] = mt > 0.0 ? s[c] / mt : 0.0;
    }
}

// MODE 0: NC = 3 squared displacements; MODE 1: NC = 1 velocity product
template <int MODE>
__global__ __launch_bounds__(CORR_BLOCK) void corr_kernel(const CorrArgs a) {
    constexpr int NC = MODE == 0 ? 3 : 1;
    __shared__ double part[CORR_BLOCK][NC];
    __shared__ int grp[CORR_BLOCK];
    __shared__ double acc[MAX_GROUPS][NC];
    const int k = blockIdx.x, b = blockIdx.y;
    const int beg = a.atom_ptr[b], n = a.atom_ptr[b + 1] - beg;
    if (n < 1 || beg < 0 || (int64_t)beg + n > a.n_atoms) return;  // (uniform)
    const int S = a.n_species, G = S + 1, B = a.n_structs;
    const int n_or = (a.n_frames - 1 - k) / a.origin_stride + 1;  // k <= max_lag <= n_frames - 1
    if (threadIdx.x < MAX_GROUPS * NC) acc[threadIdx.x / NC][threadIdx.x % NC] = 0.0;
    const int64_t fstride = 3 * (int64_t)a.n_atoms;

    for (int c0 = 0; c0 < n; c0 += CORR_BLOCK) {
        const int i = c0 + threadIdx.x;
        double s[NC];
#pragma unroll
        for (int c = 0; c < NC; ++c) s[c] = 0.0;
        int gi = -1;
        if (i < n) {
            gi = a.group[beg + i];
            const double m = MODE == 1 ? a.masses[beg + i] : 1.0;
            const double* X = a.traj + 3 * ((int64_t)beg + i);
            for (int o = 0; o < n_or; ++o) {
                const int t = o * a.origin_stride;
                const double* xa = X + (int64_t)(a.frame0 + t * a.frame_step) * fstride;
                const double* xb = X + (int64_t)(a.frame0 + (t + k) * a.frame_step) * fstride;
                if (MODE == 0) {
#pragma unroll
                    for (int c = 0; c < 3; ++c) {
                        const double dc = a.com ? a.com[3 * ((int64_t)(t + k) * B + b) + c] - a.com[3 * ((int64_t)t * B + b) + c] : 0.0;
                        const double d = (xb[c] - xa[c]) - dc;
                        s[c] = s[c] + d * d;
                    }
                } else {
                    const double v0 = xa[0] / m, v1 = xa[1] / m, v2 = xa[2] / m;
                    const double u0 = xb[0] / m, u1 = xb[1] / m, u2 = xb[2] / m;
                    s[0] = s[0] + ((v0 * u0 + v1 * u1) + v2 * u2);
                }
            }
        }
        __syncthreads();  // (the last chunk's partial sums have been read; acc is zero)
#pragma unroll
        for (int c = 0; c < NC; ++c) part[threadIdx.x][c] = s[c];
        grp[threadIdx.x] = gi;
        __syncthreads();
        group_rows_add<NC>(part, grp, acc, S);  // (group_rows.h: the fixed order of the rows of a group)
    }
    __syncthreads();
    if (threadIdx.x < G * NC) {
        const int g = threadIdx.x / NC, c = threadIdx.x % NC;
        const double Na = (double)a.group_count[b * G + g];
        a.out[(((int64_t)b * G + g) * (a.max_lag + 1) + k) * NC + c] = Na > 0.0 ? acc[g][c] / ((double)n_or * Na) : 0.0;
    }
}

__global__ __launch_bounds__(SMALL_BLOCK) void vdos_kernel(const double* __restrict__ vacf, int n_rows, int K, double dtau,
                                                           int n_freq, double f_max, int window, double* __restrict__ out) {
    const int64_t total = (int64_t)n_rows * n_freq;
    for (int64_t w = (int64_t)blockIdx.x * SMALL_BLOCK + threadIdx.x; w < total; w += (int64_t)gridDim.x * SMALL_BLOCK) {
        const int row = (int)(w / n_freq), j = (int)(w - (int64_t)row * n_freq);
        const double* Cv = vacf + (int64_t)row * (K + 1);
        const double C0 = Cv[0];
        double sum = 0.0;
        if (C0 != 0.0) {
            const double nu = (double)j * (f_max / (double)(n_freq - 1));
            const double omega = (2.0 * PI) * (nu * 1e-3);
            for (int k = 0; k <= K; ++k) {
                const double ck = k == 0 ? 0.5 : 1.0;
                const double wk = window && K > 0 ? (1.0 + cos(PI * (double)k / (double)K)) / 2.0 : 1.0;
                sum = sum + ((ck * wk) * (Cv[k] / C0)) * cos(omega * ((double)k * dtau));
            }
        }
        out[w] = (2.0 * dtau) * sum;
    }
}

__global__ __launch_bounds__(ALIGNN_WAVE) void fit_kernel(const double* __restrict__ msd, int K, double dtau, int k_lo, int k_hi,
                                                          double* __restrict__ out) {
    const int comp = blockIdx.x, row = blockIdx.y, lane = threadIdx.x;
    const double* Y = msd + 3 * (int64_t)row * (K + 1);
    auto y = [&](int k) { return comp < 3 ? Y[3 * k + comp] : (Y[3 * k] + Y[3 * k + 1]) + Y[3 * k + 2]; };
    const double np = (double)(k_hi - k_lo + 1);
    double sx = 0.0, sy = 0.0;
    for (int k = k_lo + lane; k <= k_hi; k += ALIGNN_WAVE) {
        sx = sx + (double)k * dtau;
        sy = sy + y(k);
    }
    const double xm = wave_sum(sx) / np, ym = wave_sum(sy) / np;
    double sxx = 0.0, sxy = 0.0;
    for (int k = k_lo + lane; k <= k_hi; k += ALIGNN_WAVE) {
        const double dx = (double)k * dtau - xm;
        sxx = sxx + dx * dx;
        sxy = sxy + dx * (y(k) - ym);
    }
    sxx = wave_sum(sxx);
    sxy = wave_sum(sxy);
    const double slope = sxy / sxx, icpt = ym - slope * xm;
    double ss = 0.0;
    for (int k = k_lo + lane; k <= k_hi; k += ALIGNN_WAVE) {
        const double e = y(k) - (icpt + slope * ((double)k * dtau));
        ss = ss + e * e;
    }
    ss = wave_sum(ss);
    if (lane == 0) {
        double* o = out + 4 * ((int64_t)row * 4 + comp);
        o[0] = slope;
        o[1] = icpt;
        o[2] = np > 2.0 ? sqrt((ss / (np - 2.0)) / sxx) : 0.0;
        o[3] = slope / (comp < 3 ? 2.0 : 6.0);
    }
}

__global__ __launch_bounds__(SMALL_BLOCK) void green_kubo_kernel(const double* __restrict__ vacf, int n_rows, int K, double dtau,
                                                                 double unit, double* __restrict__ out) {
    for (int row = blockIdx.x * SMALL_BLOCK + threadIdx.x; row < n_rows; row += gridDim.x * SMALL_BLOCK) {
        const double* Cv = vacf + (int64_t)row * (K + 1);
        double* o = out + (int64_t)row * (K + 1);
        double I = 0.0;
        o[0] = 0.0;
        for (int k = 1; k <= K; ++k) {
            I = I + (Cv[k - 1] + Cv[k]) / 2.0;
            o[k] = ((I * (dtau * unit)) * unit) / 3.0;
        }
    }
}

// the frame selection of both argument blocks: every frame used lies inside the trajectory
bool frames_ok(int n_total, int frame0, int step, int n_frames) {
    if (n_total < 0 || frame0 < 0 || step < 1 || n_frames < 0) return false;
    return n_frames == 0 || (int64_t)frame0 + (int64_t)(n_frames - 1) * step < n_total;
}

bool rdf_args_ok(const RdfArgs& a) {
    if (a.n_structs < 0 || a.n_structs > 65535 || a.n_atoms < 0 || a.n_species < 1 || a.n_species > ALIGNN_TRAJ_MAX_SPECIES ||
        a.n_bins < 1 || a.n_bins > ALIGNN_TRAJ_MAX_BINS || a.lattice_per_frame < 0 || a.lattice_per_frame > 1)
        return false;
    if (!(a.r_max > 0.0) || !(a.r_max < 1e300)) return false;
    return frames_ok(a.n_total_frames, a.frame0, a.frame_step, a.n_frames);
}

}  // namespace

extern "C" size_t alignn_traj_rdf_args_size(void) { return sizeof(alignn_traj_rdf_args); }
extern "C" size_t alignn_traj_corr_args_size(void) { return sizeof(alignn_traj_corr_args); }

extern "C" int alignn_traj_rdf_counts(const alignn_traj_rdf_args* args, void* stream) {
    if (!args || !rdf_args_ok(*args)) return (int)hipErrorInvalidValue;
    const RdfArgs& a = *args;
    if (a.n_structs == 0 || a.n_frames == 0) return 0;
    if (a.n_atoms < 1 || a.max_atoms < 1 || a.max_atoms > a.n_atoms) return (int)hipErrorInvalidValue;
    if (!a.traj || !a.lattice || !a.atom_ptr || !a.group || !a.group_count || !a.counts || !a.status)
        return (int)hipErrorInvalidValue;
    const int tiles = alignn_ceil_div(a.max_atoms, RDF_TILE);
    if (tiles > 65535) return (int)hipErrorInvalidValue;
    const int types = a.n_species * (a.n_species + 1) / 2;
    const int per_chunk = types * a.n_bins <= RDF_HIST_CAP ? types : RDF_HIST_CAP / a.n_bins;  // >= 3: n_bins <= 4096
    rdf_counts_kernel<<<dim3(a.n_frames, tiles, a.n_structs), RDF_BLOCK, (size_t)per_chunk * a.n_bins * sizeof(unsigned),
                        (hipStream_t)stream>>>(a, per_chunk);
    ALIGNN_CHECK_LAUNCH();
    return 0;
}

extern "C" int alignn_traj_rdf_normalise(const alignn_traj_rdf_args* args, void* stream) {
    if (!args || !rdf_args_ok(*args)) return (int)hipErrorInvalidValue;
    const RdfArgs& a = *args;
    if (a.n_structs == 0) return 0;
    if (!a.lattice || !a.group_count || !a.counts || !a.g || !a.coord || !a.volume || !a.centres) return (int)hipErrorInvalidValue;
    rdf_volume_kernel<<<alignn_ceil_div(a.n_structs, SMALL_BLOCK), SMALL_BLOCK, 0, (hipStream_t)stream>>>(a);
    ALIGNN_CHECK_LAUNCH();
    rdf_normalise_kernel<<<dim3(1 + a.n_species * (a.n_species + 1) / 2, a.n_structs), SMALL_BLOCK, 0, (hipStream_t)stream>>>(a);
    ALIGNN_CHECK_LAUNCH();
    return 0;
}

static bool corr_args_ok(const alignn_traj_corr_args& a) {
    if (a.n_structs < 0 || a.n_structs > 65535 || a.n_atoms < 0 || a.n_species < 1 || a.n_species > ALIGNN_TRAJ_MAX_SPECIES ||
        a.origin_stride < 1 || a.mode < 0 || a.mode > 1)
        return false;
    return frames_ok(a.n_total_frames, a.frame0, a.frame_step, a.n_frames);
}

extern "C" int alignn_traj_com(const alignn_traj_corr_args* args, void* stream) {
    if (!args || !corr_args_ok(*args)) return (int)hipErrorInvalidValue;
    const CorrArgs& a = *args;
    if (a.n_structs == 0 || a.n_frames == 0) return 0;
    if (a.n_atoms < 1 || !a.traj || !a.masses || !a.atom_ptr || !a.com) return (int)hipErrorInvalidValue;
    com_kernel<<<capped_blocks((int64_t)a.n_frames * a.n_structs, SMALL_BLOCK, SMALL_MAX_BLOCKS), SMALL_BLOCK, 0,
                 (hipStream_t)stream>>>(a);
    ALIGNN_CHECK_LAUNCH();
    return 0;
}

extern "C" int alignn_traj_corr(const alignn_traj_corr_args* args, void* stream) {
    if (!args || !corr_args_ok(*args)) return (int)hipErrorInvalidValue;
    const CorrArgs& a = *args;
    if (a.n_structs == 0 || a.n_frames == 0) return 0;
    if (a.max_lag < 0 || a.max_lag > a.n_frames - 1) return (int)hipErrorInvalidValue;
    if (a.n_atoms < 1 || !a.traj || !a.atom_ptr || !a.group || !a.group_count || !a.out || (a.mode == 1 && !a.masses))
        return (int)hipErrorInvalidValue;
    const dim3 grid(a.max_lag + 1, a.n_structs);
    if (a.mode == 0)
        corr_kernel<0><<<grid, CORR_BLOCK, 0, (hipStream_t)stream>>>(a);
    else
        corr_kernel<1><<<grid, CORR_BLOCK, 0, (hipStream_t)stream>>>(a);
    ALIGNN_CHECK_LAUNCH();
    return 0;
}

extern "C" int alignn_traj_vdos(const double* vacf, int n_rows, int max_lag, double dtau, int n_freq, double f_max_thz, int window,
                                double* out, void* stream) {
    if (n_rows < 0 || max_lag < 0 || n_freq < 2 || window < 0 || window > 1 || !(dtau > 0.0) || !(dtau < 1e300) ||
        !(f_max_thz > 0.0) || !(f_max_thz < 1e300))
        return (int)hipErrorInvalidValue;
    if (n_rows == 0) return 0;
    if (!vacf || !out) return (int)hipErrorInvalidValue;
    vdos_kernel<<<capped_blocks((int64_t)n_rows * n_freq, SMALL_BLOCK, SMALL_MAX_BLOCKS), SMALL_BLOCK, 0, (hipStream_t)stream>>>(
        vacf, n_rows, max_lag, dtau, n_freq, f_max_thz, window, out);
    ALIGNN_CHECK_LAUNCH();
    return 0;
}

extern "C" int alignn_traj_fit(const double* msd, int n_rows, int max_lag, double dtau, int k_lo, int k_hi, double* out,
                               void* stream) {
    if (n_rows < 0 || n_rows > 65535 || max_lag < 1 || k_lo < 0 || k_hi <= k_lo || k_hi > max_lag || !(dtau > 0.0) || !(dtau < 1e300))
        return (int)hipErrorInvalidValue;
    if (n_rows == 0) return 0;
    if (!msd || !out) return (int)hipErrorInvalidValue;
    fit_kernel<<<dim3(4, n_rows), ALIGNN_WAVE, 0, (hipStream_t)stream>>>(msd, max_lag, dtau, k_lo, k_hi, out);
    ALIGNN_CHECK_LAUNCH();
    return 0;
}

extern "C" int alignn_traj_green_kubo(const double* vacf, int n_rows, int max_lag, double dtau, double time_unit, double* out,
                                      void* stream) {
    if (n_rows < 0 || max_lag < 0 || !(dtau > 0.0) || !(dtau < 1e300) || !(time_unit > 0.0) || !(time_unit < 1e300))
        return (int)hipErrorInvalidValue;
    if (n_rows == 0) return 0;
    if (!vacf || !out) return (int)hipErrorInvalidValue;
    green_kubo_kernel<<<capped_blocks(n_rows, SMALL_BLOCK, SMALL_MAX_BLOCKS), SMALL_BLOCK, 0, (hipStream_t)stream>>>(
        vacf, n_rows, max_lag, dtau, time_unit, out);
    ALIGNN_CHECK_LAUNCH();
    return 0;
}
