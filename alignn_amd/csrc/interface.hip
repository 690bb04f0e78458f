// The interface task (alignn_amd/interface.py): the coincidence-lattice search of two surface cells (Zur and McGill, J. Appl.
// Phys. 55, 378 (1984)) and the builder that stacks two matched slabs into one cell, written in the arrays ``relax`` takes.  The
// reference does both on the host for one pair at a time (jarvis-tools' make_interface; alignn/ff/ff.py:984-1116).  The
// specification is the one written out in INTEGRATION.md; tests/interface_ref.py is the numpy restatement this file follows
// operation for operation.
//
//   zsl_reduce_kernel        one thread per (pair, side, multiple n, Hermite normal form): the super-lattice reduced, its norms,
//                            dot and cross product and its integer matrix written to a table (the substrate's six variants too);
//   zsl_match_kernel         one workgroup per (pair, film multiple i): every film entry of i against every substrate variant of
//                            every admissible j, the smallest key (score, j, film entry, substrate entry, variant) kept;
//   zsl_pick_kernel          one thread per pair: the smallest i that has a match, the outputs;
//   interface_build_kernel   one workgroup per matched pair: substrate, film and interface in one common cell.
// float64, no contraction, min / max only across threads and a total order on the keys: no atomics, and a pair's bits do not
// depend on what else shares the launch.
#include "../../include/alignn_hip.h"
#include "common.h"
#include "cell3.h"
#include "wave_fit.h"

#pragma clang fp contract(off)

namespace {

constexpr int IF_BLOCK = 256;
constexpr int IF_WAVES = IF_BLOCK / ALIGNN_WAVE;
constexpr int ZSL_MAX_N = 256;      // the largest multiple of a side
constexpr int ZSL_MAX_SIGMA = 744;  // the most Hermite normal forms of one multiple n <= 256 (n = 240)
constexpr int ZSL_VARIANTS = 6;
constexpr int ZSL_ROUNDS = 64;
constexpr int64_t ZSL_NONE = INT64_MAX;
constexpr double IF_TOL = 1e-10;  // the builders' tolerance of the wrap: s -= floor(s + tol)

__device__ __forceinline__ bool finite4(const double* c) {
    return isfinite(c[0]) && isfinite(c[1]) && isfinite(c[2]) && isfinite(c[3]);
}
// the signed area of a 2 x 2 cell (rows v1, v2)
__device__ __forceinline__ double cell_cross(const double* c) { return c[0] * c[3] - c[1] * c[2]; }
__device__ __forceinline__ bool cell_valid(const double* c) {
    if (!finite4(c)) return false;
    const double a = cell_cross(c);
    return a > 0.0 && a < INFINITY;
}

// (|u|, |w|, u.w, u x w) of a basis
__device__ __forceinline__ void basis_entry(double ux, double uy, double wx, double wy, double* out) {
    out[0] = sqrt(ux * ux + uy * uy);
    out[1] = sqrt(wx * wx + wy * wy);
    out[2] = ux * wx + uy * wy;
    out[3] = ux * wy - uy * wx;
}

// the mismatch of a film entry f and a substrate entry s, both (|u|, |w|, d, c): false where the pair is not accepted
__device__ __forceinline__ bool zsl_eval(const double* f, const double* s, double ltol, double cos_atol, double& ru, double& rw,
                                         double& sn, double& score) {
    ru = fabs(s[0] / f[0] - 1.0);
    if (!(ru <= ltol)) return false;
    rw = fabs(s[1] / f[1] - 1.0);
    if (!(rw <= ltol)) return false;
    const double den = ((f[0] * f[1]) * s[0]) * s[1];
    const double cs = (f[2] * s[2] + f[3] * s[3]) / den;
    if (!(cs >= cos_atol)) return false;
    sn = (f[2] * s[3] - f[3] * s[2]) / den;
    score = fmax(fmax(ru, rw), fabs(sn));
    return true;
}

__device__ __forceinline__ bool key_less(double s1, int64_t t1, double s2, int64_t t2) {
    return s1 < s2 || (s1 == s2 && t1 < t2);
}

// variant v of the reduced basis rows (u, w): (u, w), (u, w + u), (u, w - u), (w, -u), (w, -u + w), (w, -u - w)
template <typename T>
__device__ __forceinline__ void zsl_variant(int v, T ux, T uy, T wx, T wy, T& ax, T& ay, T& bx, T& by) {
    if (v < 3) {
        ax = ux, ay = uy;
        bx = v == 0 ? wx : (v == 1 ? wx + ux : wx - ux);
        by = v == 0 ? wy : (v == 1 ? wy + uy : wy - uy);
    } else {
        ax = wx, ay = wy;
        bx = v == 3 ? -ux : (v == 4 ? -ux + wx : -ux - wx);
        by = v == 3 ? -uy : (v == 4 ? -uy + wy : -uy - wy);
    }
}

// hnf [.][3] = (n, a, b) of every Hermite normal form [[a, b], [0, n / a]] in the order (n, a, b); prefix [n] its first entry of
// multiple n (prefix [1] = 0, prefix [ZSL_MAX_N + 1] the total).
__global__ __launch_bounds__(IF_BLOCK) void zsl_reduce_kernel(
    const double* __restrict__ film_cells, const double* __restrict__ subs_cells, const int32_t* __restrict__ nmax_film,
    const int32_t* __restrict__ nmax_subs, const int32_t* __restrict__ hnf, const int32_t* __restrict__ prefix,
    const int64_t* __restrict__ film_off, const int64_t* __restrict__ subs_off, int64_t film_rows, int64_t subs_rows,
    double* __restrict__ film_tab, int32_t* __restrict__ film_int, double* __restrict__ subs_tab, int32_t* __restrict__ subs_int) {
    const int pair = blockIdx.y >> 1, side = blockIdx.y & 1;
    const int nmax = min(side ? nmax_subs[pair] : nmax_film[pair], ZSL_MAX_N);
    if (nmax < 1) return;
    const int e = blockIdx.x * IF_BLOCK + threadIdx.x;
    const int count = prefix[nmax + 1];
    if (e >= count) return;
    const int64_t off = side ? subs_off[pair] : film_off[pair];
    if (off < 0 || off + count > (side ? subs_rows : film_rows)) return;
    const double* cell = (side ? subs_cells : film_cells) + 4 * (int64_t)pair;
    if (!cell_valid(cell)) return;
    const int n = hnf[3 * e], a = hnf[3 * e + 1], b = hnf[3 * e + 2], d = n / a;
    double ux = (double)a * cell[0] + (double)b * cell[2], uy = (double)a * cell[1] + (double)b * cell[3];
    double wx = (double)d * cell[2], wy = (double)d * cell[3];
    int64_t m[4] = {a, b, 0, d};  // rows: u, w in units of (v1, v2)
    for (int round = 0; round < ZSL_ROUNDS; ++round) {
        double uu = ux * ux + uy * uy;
        if (uu > wx * wx + wy * wy) {  // (u, w) <- (w, -u)
            double t = ux;
            ux = wx, wx = -t;
            t = uy;
            uy = wy, wy = -t;
            int64_t q = m[0];
            m[0] = m[2], m[2] = -q;
            q = m[1];
            m[1] = m[3], m[3] = -q;
            uu = ux * ux + uy * uy;
        }
        const double k = rint((ux * wx + uy * wy) / uu);
        if (k == 0.0) break;
        wx = wx - k * ux;
        wy = wy - k * uy;
        const int64_t ki = (int64_t)k;
        m[2] -= ki * m[0];
        m[3] -= ki * m[1];
    }
    if (ux * ux + uy * uy > wx * wx + wy * wy) {
        double t = ux;
        ux = wx, wx = -t;
        t = uy;
        uy = wy, wy = -t;
        int64_t q = m[0];
        m[0] = m[2], m[2] = -q;
        q = m[1];
        m[1] = m[3], m[3] = -q;
    }
    int32_t* mi = (side ? subs_int : film_int) + 4 * (off + e);
#pragma unroll
    for (int k = 0; k < 4; ++k) mi[k] = (int32_t)m[k];
    if (!side) {
        basis_entry(ux, uy, wx, wy, film_tab + 4 * (off + e));
    } else {
        for (int v = 0; v < ZSL_VARIANTS; ++v) {
            double ax, ay, bx, by;
            zsl_variant<double>(v, ux, uy, wx, wy, ax, ay, bx, by);
            basis_entry(ax, ay, bx, by, subs_tab + 4 * ((off + e) * ZSL_VARIANTS + v));
        }
    }
}

// tag = ((j 1024 + film entry) 1024 + substrate entry) 8 + variant: the key's integer part after the score
__global__ __launch_bounds__(IF_BLOCK) void zsl_match_kernel(
    const double* __restrict__ film_cells, const double* __restrict__ subs_cells, const int32_t* __restrict__ nmax_film,
    const int32_t* __restrict__ nmax_subs, const int32_t* __restrict__ prefix, const int64_t* __restrict__ film_off,
    const int64_t* __restrict__ subs_off, int64_t film_rows, int64_t subs_rows, const double* __restrict__ film_tab,
    const double* __restrict__ subs_tab, int max_film, double ratio_tol, double ltol, double cos_atol,
    double* __restrict__ best_score, int64_t* __restrict__ best_tag) {
    __shared__ double fsh[ZSL_MAX_SIGMA][4];
    __shared__ double ssh[IF_WAVES];
    __shared__ int64_t tsh[IF_WAVES];
    const int pair = blockIdx.y, i = blockIdx.x + 1;
    const int nf_max = min(nmax_film[pair], min(max_film, ZSL_MAX_N)), ns_max = min(nmax_subs[pair], ZSL_MAX_N);
    if (i > nf_max) return;
    double bs = INFINITY;
    int64_t bt = ZSL_NONE;
    const double* fc = film_cells + 4 * (int64_t)pair;
    const double* sc = subs_cells + 4 * (int64_t)pair;
    const int64_t foff = film_off[pair], soff = subs_off[pair];
    const int nf = prefix[i + 1] - prefix[i];
    const bool ok = cell_valid(fc) && cell_valid(sc) && ns_max >= 1 && nf <= ZSL_MAX_SIGMA && foff >= 0 && soff >= 0 &&
                    foff + prefix[nf_max + 1] <= film_rows && soff + prefix[max(ns_max, 0) + 1] <= subs_rows;  // uniform
    if (ok) {
        const double af = cell_cross(fc), as = cell_cross(sc);
        for (int t = threadIdx.x; t < 4 * nf; t += IF_BLOCK) fsh[t >> 2][t & 3] = film_tab[4 * (foff + prefix[i]) + t];
        __syncthreads();
        for (int j = 1; j <= ns_max; ++j) {
            const double ratio = ((double)i * af) / ((double)j * as);
            if (!(fabs(ratio - 1.0) <= ratio_tol)) continue;
            const int ns6 = (prefix[j + 1] - prefix[j]) * ZSL_VARIANTS;
            const double* st = subs_tab + 4 * ((soff + prefix[j]) * ZSL_VARIANTS);
            for (int r = threadIdx.x; r < ns6; r += IF_BLOCK) {
                const double s[4] = {st[4 * r], st[4 * r + 1], st[4 * r + 2], st[4 * r + 3]};
                const int se = r / ZSL_VARIANTS, v = r - se * ZSL_VARIANTS;
                for (int fe = 0; fe < nf; ++fe) {
                    double ru, rw, sn, score;
                    if (!zsl_eval(fsh[fe], s, ltol, cos_atol, ru, rw, sn, score)) continue;
                    const int64_t tag = ((((int64_t)j * 1024 + fe) * 1024 + se) * 8) + v;
                    if (key_less(score, tag, bs, bt)) bs = score, bt = tag;
                }
            }
        }
    }
    // the smallest key of the workgroup: the xor butterfly within a wavefront, then the wavefronts in order
#pragma unroll
    for (int o = ALIGNN_WAVE / 2; o > 0; o >>= 1) {
        const double os = __shfl_xor(bs, o, ALIGNN_WAVE);
        const int lo = __shfl_xor((int)(bt & 0xffffffff), o, ALIGNN_WAVE), hi = __shfl_xor((int)(bt >> 32), o, ALIGNN_WAVE);
        const int64_t ot = ((int64_t)hi << 32) | (uint32_t)lo;
        if (key_less(os, ot, bs, bt)) bs = os, bt = ot;
    }
    const int lane = threadIdx.x & (ALIGNN_WAVE - 1), wave = threadIdx.x / ALIGNN_WAVE;
    if (lane == 0) ssh[wave] = bs, tsh[wave] = bt;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < IF_WAVES; ++w)
            if (key_less(ssh[w], tsh[w], bs, bt)) bs = ssh[w], bt = tsh[w];
        best_score[(int64_t)pair * max_film + (i - 1)] = bs;
        best_tag[(int64_t)pair * max_film + (i - 1)] = bt;
    }
}

__global__ __launch_bounds__(IF_BLOCK) void zsl_pick_kernel(
    const double* __restrict__ film_cells, const double* __restrict__ subs_cells, int n_pairs,
    const int32_t* __restrict__ nmax_film, const int32_t* __restrict__ prefix, const int64_t* __restrict__ film_off,
    const int64_t* __restrict__ subs_off, const double* __restrict__ film_tab, const int32_t* __restrict__ film_int,
    const double* __restrict__ subs_tab, const int32_t* __restrict__ subs_int, int max_film, double ltol, double cos_atol,
    const int64_t* __restrict__ best_tag, int32_t* __restrict__ status, int32_t* __restrict__ multiples,
    int32_t* __restrict__ film_matrix, int32_t* __restrict__ subs_matrix, double* __restrict__ mismatch) {
    const int pair = blockIdx.x * IF_BLOCK + threadIdx.x;
    if (pair >= n_pairs) return;
    if (!cell_valid(film_cells + 4 * (int64_t)pair) || !cell_valid(subs_cells + 4 * (int64_t)pair)) {
        status[pair] = 2;
        return;
    }
    const int nf_max = min(nmax_film[pair], min(max_film, ZSL_MAX_N));
    for (int i = 1; i <= nf_max; ++i) {
        const int64_t tag = best_tag[(int64_t)pair * max_film + (i - 1)];
        if (tag == ZSL_NONE) continue;
        const int v = (int)(tag & 7), se = (int)((tag >> 3) & 1023), fe = (int)((tag >> 13) & 1023), j = (int)(tag >> 23);
        const int64_t fr = film_off[pair] + prefix[i] + fe, sr = subs_off[pair] + prefix[j] + se;
        double ru, rw, sn, score;
        zsl_eval(film_tab + 4 * fr, subs_tab + 4 * (sr * ZSL_VARIANTS + v), ltol, cos_atol, ru, rw, sn, score);
        const int32_t* ms = subs_int + 4 * sr;
        int32_t ax, ay, bx, by;
        zsl_variant<int32_t>(v, ms[0], ms[1], ms[2], ms[3], ax, ay, bx, by);
        status[pair] = 0;
        multiples[2 * pair] = i, multiples[2 * pair + 1] = j;
#pragma unroll
        for (int k = 0; k < 4; ++k) film_matrix[4 * (int64_t)pair + k] = film_int[4 * fr + k];
        int32_t* so = subs_matrix + 4 * (int64_t)pair;
        so[0] = ax, so[1] = ay, so[2] = bx, so[3] = by;
        double* mo = mismatch + 4 * (int64_t)pair;
        mo[0] = ru, mo[1] = rw, mo[2] = sn, mo[3] = score;
        return;
    }
    status[pair] = 1;
}

// ---- the builder ------------------------------------------------------------------------------------------------------------------

__device__ __forceinline__ int64_t gcd64(int64_t a, int64_t b) {
    a = a < 0 ? -a : a;
    b = b < 0 ? -b : b;
    while (b) {
        const int64_t t = a % b;
        a = b, b = t;
    }
    return a;
}

// one side of a pair: its slab and its super-cell matrix
struct IfSide {
    double inv[9];   // the slab cell's inverse
    double la3;      // |a3|
    double m[4];     // the integer matrix (rows u, w in units of C0, C1)
    double det;
    int64_t beg;     // the slab's first row
    int n, a, d;     // the slab's atoms; the Hermite normal form's diagonal: images m0 < a, m1 < d
};

// the 2-d cell (rows p0 = (l0, 0), p1 = (x1, y1)) of a slab cell's first two rows, x along row 0
__device__ __forceinline__ void plane_cell(const double* C, double& l0, double& x1, double& y1) {
    l0 = sqrt((C[0] * C[0] + C[1] * C[1]) + C[2] * C[2]);
    x1 = ((C[0] * C[3] + C[1] * C[4]) + C[2] * C[5]) / l0;
    const double n0 = C[1] * C[5] - C[2] * C[4], n1 = C[2] * C[3] - C[0] * C[5], n2 = C[0] * C[4] - C[1] * C[3];
    y1 = sqrt((n0 * n0 + n1 * n1) + n2 * n2) / l0;
}

__device__ __forceinline__ void side_setup(const double* C, const int32_t* M, int64_t beg, int n, IfSide& s) {
    double c[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) c[k] = C[k];
    inv3_cof(c, s.inv);
    s.la3 = sqrt((c[6] * c[6] + c[7] * c[7]) + c[8] * c[8]);
#pragma unroll
    for (int k = 0; k < 4; ++k) s.m[k] = (double)M[k];
    const int64_t det = (int64_t)M[0] * M[3] - (int64_t)M[1] * M[2];
    s.det = (double)det;
    s.beg = beg, s.n = n;
    s.a = (int)gcd64(M[0], M[2]);
    s.d = s.a > 0 ? (int)(det / s.a) : 0;
}

// the height of slab row b over the slab cell's in-plane face
__device__ __forceinline__ double side_height(const IfSide& s, const double* __restrict__ cart, int b) {
    const double r[3] = {cart[3 * (s.beg + b)], cart[3 * (s.beg + b) + 1], cart[3 * (s.beg + b) + 2]};
    return row_dot(r, s.inv, 2) * s.la3;
}

// min over the workgroup of v[0], v[2] and max of v[1], v[3]; every thread returns the same values (exact, whatever the order)
__device__ __forceinline__ void block_minmax(double (&v)[4], double (*sh)[IF_WAVES]) {
    const int lane = threadIdx.x & (ALIGNN_WAVE - 1), wave = threadIdx.x / ALIGNN_WAVE;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        v[k] = (k & 1) ? wave_max(v[k]) : wave_min(v[k]);
        if (lane == 0) sh[k][wave] = v[k];
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        double s = sh[k][0];
#pragma unroll
        for (int w = 1; w < IF_WAVES; ++w) s = (k & 1) ? fmax(s, sh[k][w]) : fmin(s, sh[k][w]);
        v[k] = s;
    }
}

// jobs [pair][10] = (film slab, substrate slab, film matrix [4], substrate matrix [4])
constexpr int IF_JOB = 10;
__global__ __launch_bounds__(IF_BLOCK) void interface_build_kernel(
    const double* __restrict__ slab_cells, const double* __restrict__ slab_cart, const int64_t* __restrict__ slab_off,
    const int32_t* __restrict__ slab_src, int n_slabs, const int32_t* __restrict__ jobs, const double* __restrict__ separation,
    const double* __restrict__ vacuum, const int64_t* __restrict__ out_off, double* __restrict__ cells, double* __restrict__ cart,
    double* __restrict__ frac, int32_t* __restrict__ src, int32_t* __restrict__ part, double* __restrict__ area) {
    __shared__ double sh[4][IF_WAVES];
    const int pair = blockIdx.x;
    const int32_t* J = jobs + IF_JOB * (int64_t)pair;
    const int fs = J[0], ss = J[1];
    if (fs < 0 || fs >= n_slabs || ss < 0 || ss >= n_slabs) return;
    const int64_t nf64 = slab_off[fs + 1] - slab_off[fs], ns64 = slab_off[ss + 1] - slab_off[ss];
    const int64_t det_f = (int64_t)J[2] * J[5] - (int64_t)J[3] * J[4], det_s = (int64_t)J[6] * J[9] - (int64_t)J[7] * J[8];
    if (nf64 < 1 || ns64 < 1 || det_f < 1 || det_s < 1 || det_f > ZSL_MAX_N || det_s > ZSL_MAX_N) return;
    const int64_t rows_s = det_s * ns64, rows_f = det_f * nf64;
    if (rows_s + rows_f > INT32_MAX) return;
    const int64_t o0 = out_off[3 * (int64_t)pair], o1 = out_off[3 * (int64_t)pair + 1], o2 = out_off[3 * (int64_t)pair + 2];
    if (o1 - o0 != rows_s || o2 - o1 != rows_f || out_off[3 * (int64_t)pair + 3] - o2 != rows_s + rows_f) return;
    IfSide F, S;
    side_setup(slab_cells + 9 * (int64_t)fs, J + 2, slab_off[fs], (int)nf64, F);
    side_setup(slab_cells + 9 * (int64_t)ss, J + 6, slab_off[ss], (int)ns64, S);
    // the heights' ranges: (min_s, max_s, min_f, max_f)
    double mm[4] = {INFINITY, -INFINITY, INFINITY, -INFINITY};
    for (int b = threadIdx.x; b < S.n; b += IF_BLOCK) {
        const double h = side_height(S, slab_cart, b);
        mm[0] = fmin(mm[0], h), mm[1] = fmax(mm[1], h);
    }
    for (int b = threadIdx.x; b < F.n; b += IF_BLOCK) {
        const double h = side_height(F, slab_cart, b);
        mm[2] = fmin(mm[2], h), mm[3] = fmax(mm[3], h);
    }
    block_minmax(mm, sh);
    // the common cell: the substrate's super-cell in the plane, x along u_s
    double l0, x1, y1;
    plane_cell(slab_cells + 9 * (int64_t)ss, l0, x1, y1);
    const double ux = S.m[0] * l0 + S.m[1] * x1, uy = S.m[1] * y1, wx = S.m[2] * l0 + S.m[3] * x1, wy = S.m[3] * y1;
    const double nu = sqrt(ux * ux + uy * uy);
    const double top_s = mm[1] - mm[0];  // max_s z
    const double sep = separation[pair];
    const double lz = (((mm[3] - mm[2]) + top_s) + sep) + vacuum[pair];
    double A[9] = {nu, 0.0, 0.0, (ux * wx + uy * wy) / nu, (ux * wy - uy * wx) / nu, 0.0, 0.0, 0.0, lz}, Ainv[9];
    inv3_cof(A, Ainv);
    if (threadIdx.x < 27) cells[9 * (3 * (int64_t)pair) + threadIdx.x] = A[threadIdx.x % 9];
    if (threadIdx.x == 0) area[pair] = fabs(A[0] * A[4]);
    const int total = (int)(rows_s + rows_f);
    for (int t = threadIdx.x; t < total; t += IF_BLOCK) {
        const bool film = t >= rows_s;
        const IfSide& X = film ? F : S;
        const int q = film ? t - (int)rows_s : t;
        const int img = q / X.n, b = q - img * X.n;
        const int m0 = img / X.d, m1 = img - m0 * X.d;
        const double r0[3] = {slab_cart[3 * (X.beg + b)], slab_cart[3 * (X.beg + b) + 1], slab_cart[3 * (X.beg + b) + 2]};
        const double f0 = row_dot(r0, X.inv, 0) + (double)m0, f1 = row_dot(r0, X.inv, 1) + (double)m1;
        const double h = row_dot(r0, X.inv, 2) * X.la3;
        double g0 = (f0 * X.m[3] - f1 * X.m[2]) / X.det, g1 = (f1 * X.m[0] - f0 * X.m[1]) / X.det;
        g0 = g0 - floor(g0 + IF_TOL);
        g1 = g1 - floor(g1 + IF_TOL);
        const double r[3] = {g0 * A[0] + g1 * A[3], g1 * A[4], film ? ((h - mm[2]) + top_s) + sep : h - mm[0]};
        const int32_t from = slab_src[X.beg + b];
        const int64_t rows[2] = {(film ? o1 : o0) + q, o2 + t};
#pragma unroll
        for (int w = 0; w < 2; ++w) {
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                cart[3 * rows[w] + k] = r[k];
                frac[3 * rows[w] + k] = wrap01(row_dot(r, Ainv, k));
            }
            src[rows[w]] = from;
            part[rows[w]] = film ? 1 : 0;
        }
    }
}

}  // namespace

extern "C" int alignn_zsl_match(const double* film_cells, const double* subs_cells, int n_pairs, const int32_t* nmax_film,
                                const int32_t* nmax_subs, int max_film, int max_subs, const int32_t* hnf, const int32_t* prefix,
                                const int64_t* film_off, const int64_t* subs_off, int64_t film_rows, int64_t subs_rows,
                                double* film_tab, int32_t* film_int, double* subs_tab, int32_t* subs_int, double* best_score,
                                int64_t* best_tag, double max_area_ratio_tol, double ltol, double cos_atol, int32_t* status,
                                int32_t* multiples, int32_t* film_matrix, int32_t* subs_matrix, double* mismatch,
                                alignn_stream_t stream) {
    if (n_pairs < 0 || max_film < 0 || max_subs < 0 || max_film > ZSL_MAX_N || max_subs > ZSL_MAX_N || film_rows < 0 ||
        subs_rows < 0 || !film_cells || !subs_cells || !nmax_film || !nmax_subs || !hnf || !prefix || !film_off || !subs_off ||
        !film_tab || !film_int || !subs_tab || !subs_int || !best_score || !best_tag || !status || !multiples || !film_matrix ||
        !subs_matrix || !mismatch)
        return (int)hipErrorInvalidValue;
    if (n_pairs == 0) return 0;
    if (n_pairs > 32767) return (int)hipErrorInvalidValue;  // (2 n_pairs is a grid's y extent)
    hipStream_t st = (hipStream_t)stream;
    // entries of the largest multiple either side can have: prefix[max + 1] <= 54077; the kernel reads the count per pair
    const int max_n = max_film > max_subs ? max_film : max_subs;
    if (max_n >= 1 && max_film >= 1) {
        const int64_t most = (int64_t)max_n * (max_n + 1);  // >= sum of sigma(n), n <= max_n
        const int blocks = alignn_ceil_div(most < 54077 ? most : 54077, IF_BLOCK);
        zsl_reduce_kernel<<<dim3(blocks, 2 * n_pairs), IF_BLOCK, 0, st>>>(film_cells, subs_cells, nmax_film, nmax_subs, hnf, prefix,
                                                                         film_off, subs_off, film_rows, subs_rows, film_tab,
                                                                         film_int, subs_tab, subs_int);
        ALIGNN_CHECK_LAUNCH();
        zsl_match_kernel<<<dim3(max_film, n_pairs), IF_BLOCK, 0, st>>>(film_cells, subs_cells, nmax_film, nmax_subs, prefix,
                                                                       film_off, subs_off, film_rows, subs_rows, film_tab,
                                                                       subs_tab, max_film, max_area_ratio_tol, ltol, cos_atol,
                                                                       best_score, best_tag);
        ALIGNN_CHECK_LAUNCH();
    }
    zsl_pick_kernel<<<alignn_ceil_div(n_pairs, IF_BLOCK), IF_BLOCK, 0, st>>>(
        film_cells, subs_cells, n_pairs, nmax_film, prefix, film_off, subs_off, film_tab, film_int, subs_tab, subs_int, max_film,
        ltol, cos_atol, best_tag, status, multiples, film_matrix, subs_matrix, mismatch);
    ALIGNN_CHECK_LAUNCH();
    return 0;
}

extern "C" int alignn_interface_build(const double* slab_cells, const double* slab_cart, const int64_t* slab_off,
                                      const int32_t* slab_src, int n_slabs, const int32_t* jobs, const double* separation,
                                      const double* vacuum, const int64_t* out_off, int n_pairs, double* cells, double* cart,
                                      double* frac, int32_t* src, int32_t* part, double* area, alignn_stream_t stream) {
    if (n_pairs < 0 || n_slabs < 1 || !slab_cells || !slab_cart || !slab_off || !slab_src || !jobs || !separation || !vacuum ||
        !out_off || !cells || !cart || !frac || !src || !part || !area)
        return (int)hipErrorInvalidValue;
    if (n_pairs == 0) return 0;
    interface_build_kernel<<<n_pairs, IF_BLOCK, 0, (hipStream_t)stream>>>(slab_cells, slab_cart, slab_off, slab_src, n_slabs, jobs,
                                                                           separation, vacuum, out_off, cells, cart, frac, src,
                                                                           part, area);
    ALIGNN_CHECK_LAUNCH();
    return 0;
}
