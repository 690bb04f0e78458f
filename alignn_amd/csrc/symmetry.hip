// Device side of the symmetry search and the symmetrisers (alignn_amd/symmetry.py): the space-group operations of B crystals found
// together, their atom permutations and orbits, and the projection of forces, stresses and positions onto the symmetric subspace.
// The reference gets this from spglib, one structure at a time on the host; tests/sym_ref.py is the numpy restatement,
// include/alignn_sym.h states the definitions, the layouts and every field of the argument blocks.
//
//   sym_lattice_kernel   one workgroup per structure: fractional coordinates, the candidate images of the three lattice vectors
//                        (at most 17^3 lattice points), the triples that keep the metric, sorted by their entries;
//   sym_accept_kernel    one workgroup per (lattice operation, structure, 16 candidate translations), the structure's sorted
//                        fractional coordinates and species ranges in LDS, one wavefront per candidate translation, lanes over
//                        the atoms i against the atoms of i's species; the wavefront leaves at the first atoms without a
//                        partner.  The hot path;
//   sym_summary_kernel   one thread per structure: the counts and the crystal system;
//   sym_fill_kernel      the same grid, one wavefront per accepted operation: W, t, atom map and lattice shifts;
//   sym_orbits_kernel    one thread per atom: the lowest image of the atom;
//   sym_forces_kernel, sym_stress_kernel, sym_positions_kernel: one thread per atom or per element, over g in stored order.
// float64 without contraction, no atomics on floating-point values (the only atomics count candidates and accepted operations,
// as integers), every floating-point sum in a fixed order: a structure's bits are the same alone, in a batch and at any
// place of the batch.
#include "../../include/alignn_sym.h"
#include "common.h"
#include "cell3.h"

#pragma clang fp contract(off)

namespace {

constexpr int BLOCK = 256, WAVES = BLOCK / ALIGNN_WAVE;
constexpr int MAX_OPS = ALIGNN_SYM_MAX_LATTICE_OPS, MAX_CAND = ALIGNN_SYM_MAX_CANDIDATES, RANGE = ALIGNN_SYM_MAX_IMAGE_RANGE;
constexpr int INFO = ALIGNN_SYM_INFO;
constexpr int CHUNK = 4 * WAVES;  // candidate translations of one workgroup of the acceptance and of the fill
constexpr double SLACK = 1.000001;  // of the two cheap tests that come before the exact one; they only ever let more through

using FindArgs = alignn_sym_find_args;
using ApplyArgs = alignn_sym_apply_args;

__device__ __forceinline__ double norm3(double x, double y, double z) { return sqrt((x * x + y * y) + z * z); }

__device__ __forceinline__ int det3i(const int (&W)[9]) {
    return W[0] * (W[4] * W[8] - W[5] * W[7]) - W[1] * (W[3] * W[8] - W[5] * W[6]) + W[2] * (W[3] * W[7] - W[4] * W[6]);
}

// W x per row: (W_r0 x_0 + W_r1 x_1) + W_r2 x_2
__device__ __forceinline__ void apply_w(const double (&W)[9], const double* x, double (&y)[3]) {
#pragma unroll
    for (int r = 0; r < 3; ++r) y[r] = (W[3 * r] * x[0] + W[3 * r + 1] * x[1]) + W[3 * r + 2] * x[2];
}

// (n_0 a_0 + n_1 a_1) + n_2 a_2
__device__ __forceinline__ void lattice_vector(const double (&A)[9], int n0, int n1, int n2, double (&v)[3]) {
    const double f0 = (double)n0, f1 = (double)n1, f2 = (double)n2;
#pragma unroll
    for (int c = 0; c < 3; ++c) v[c] = (f0 * A[c] + f1 * A[3 + c]) + f2 * A[6 + c];
}

// t = d - floor(d) of d = x_j - W x_p; a component that rounds to 1.0 becomes 0
__device__ __forceinline__ void translation(const double* xj, const double (&yp)[3], double (&t)[3]) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const double d = xj[c] - yp[c];
        const double f = d - floor(d);
        t[c] = f < 1.0 ? f : 0.0;
    }
}

// What the acceptance and the map share: the atoms of one species range against the image y + t of an atom.
struct Matcher {
    double A[9], bound[3], symprec, s2_hi;

    __device__ __forceinline__ void init(const double (&cell)[9], double sp) {
        double h[3];
#pragma unroll
        for (int j = 0; j < 9; ++j) A[j] = cell[j];
        heights(cell, h);
#pragma unroll
        for (int c = 0; c < 3; ++c) bound[c] = (sp / h[c]) * SLACK;  // |f_c| <= |r| / h_c
        symprec = sp;
        s2_hi = (sp * sp) * SLACK;
    }

    // the squared distance of image and atom k when it can lie within symprec, else a negative number; delta as it was before rint
    __device__ __forceinline__ double near2(const double (&img)[3], const double* xk, double (&delta)[3]) const {
        double f[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            delta[c] = img[c] - xk[c];
            f[c] = delta[c] - rint(delta[c]);
            if (fabs(f[c]) > bound[c]) return -1.0;
        }
        const double cx = (f[0] * A[0] + f[1] * A[3]) + f[2] * A[6];
        const double cy = (f[0] * A[1] + f[1] * A[4]) + f[2] * A[7];
        const double cz = (f[0] * A[2] + f[1] * A[5]) + f[2] * A[8];
        const double d2 = (cx * cx + cy * cy) + cz * cz;
        if (!(d2 <= s2_hi)) return -1.0;
        return sqrt(d2) <= symprec ? d2 : -1.0;
    }
};

struct Rows {
    int beg, n, plo, phi;
    bool ok;
};

// the rows of structure b and its pivot range, as far as they fit the arrays
__device__ __forceinline__ Rows rows_of(const FindArgs& a, int b) {
    Rows r;
    r.beg = a.atom_ptr[b];
    r.n = a.atom_ptr[b + 1] - r.beg;
    r.plo = a.pivot_lo[b];
    r.phi = a.pivot_hi[b];
    r.ok = r.n >= 1 && r.n <= a.max_atoms && r.beg >= 0 && (int64_t)r.beg + r.n <= a.n_atoms && r.plo >= 0 && r.plo < r.phi &&
           r.phi <= r.n;
    return r;
}

__device__ __forceinline__ int64_t op_key(const int (&W)[9]) {
    int64_t key = 0;
#pragma unroll
    for (int j = 0; j < 9; ++j) key = key * (2 * RANGE + 1) + (W[j] + RANGE);
    return key;
}

__global__ __launch_bounds__(BLOCK) void sym_lattice_kernel(const FindArgs a) {
    __shared__ int cand[3][MAX_CAND];  // n_0 + 8 | (n_1 + 8) << 5 | (n_2 + 8) << 10
    __shared__ int n_cand[3], n_ops;
    __shared__ int64_t keys[MAX_OPS];
    const int b = blockIdx.x, tid = threadIdx.x;
    int32_t* info = a.info + (int64_t)INFO * b;
    int32_t* ops = a.lattice_ops + (int64_t)MAX_OPS * 9 * b;
    const Rows R = rows_of(a, b);
    int status = 0;
    // the caller's sorting: every slot names a row of the structure and lies in its own range
    int bad = R.ok ? 0 : 1;
    if (R.ok) {
        for (int q = tid; q < R.n; q += BLOCK) {
            const int o = a.order[R.beg + q], lo = a.seg_lo[R.beg + q], hi = a.seg_hi[R.beg + q];
            if (o < 0 || o >= R.n || lo < 0 || lo > q || hi <= q || hi > R.n) bad = 1;
        }
    }
    if (tid < 3) n_cand[tid] = 0;
    if (tid == 0) n_ops = 0;
    if (__syncthreads_or(bad)) status |= ALIGNN_SYM_STATUS_INPUT;

    double A[9], Ai[9], h[3], len[3];
    load9(a.lattice + 9 * (int64_t)b, A);
    heights(A, h);
    double longest = 0.0;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        len[i] = norm3(A[3 * i], A[3 * i + 1], A[3 * i + 2]);
        longest = fmax(longest, len[i]);
    }
    int M[3] = {0, 0, 0};
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const double q = floor((longest + a.symprec) / h[k]);
        if (!(q >= 0.0 && q <= (double)RANGE))  // (a NaN fails both)
            status |= ALIGNN_SYM_STATUS_IMAGES;
        else
            M[k] = (int)q;
    }
    if (status == 0) {
        inv3_cof(A, Ai);
        for (int i = tid; i < R.n; i += BLOCK) {
            const double* r = a.pos + 3 * ((int64_t)R.beg + i);
            double* x = a.frac + 3 * ((int64_t)R.beg + i);
#pragma unroll
            for (int c = 0; c < 3; ++c) x[c] = row_dot(r, Ai, c);
        }
        // the candidate images of a_0, a_1, a_2
        const int d1 = 2 * M[1] + 1, d2 = 2 * M[2] + 1, points = (2 * M[0] + 1) * d1 * d2;
        for (int e = tid; e < points; e += BLOCK) {
            const int n0 = e / (d1 * d2) - M[0], n1 = (e / d2) % d1 - M[1], n2 = e % d2 - M[2];
            double v[3];
            lattice_vector(A, n0, n1, n2, v);
            const double vl = norm3(v[0], v[1], v[2]);
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                if (fabs(vl - len[i]) <= a.symprec) {
                    const int slot = atomicAdd(&n_cand[i], 1);
                    if (slot < MAX_CAND) cand[i][slot] = (n0 + RANGE) | (n1 + RANGE) << 5 | (n2 + RANGE) << 10;
                }
            }
        }
    }
    __syncthreads();
    const int c0 = n_cand[0], c1 = n_cand[1], c2 = n_cand[2];
    if (c0 > MAX_CAND || c1 > MAX_CAND || c2 > MAX_CAND) status |= ALIGNN_SYM_STATUS_OVERFLOW;
    if (status == 0) {
        double want[3];  // |a_0 - a_1|, |a_0 - a_2|, |a_1 - a_2|
        want[0] = norm3(A[0] - A[3], A[1] - A[4], A[2] - A[5]);
        want[1] = norm3(A[0] - A[6], A[1] - A[7], A[2] - A[8]);
        want[2] = norm3(A[3] - A[6], A[4] - A[7], A[5] - A[8]);
        const int64_t triples = (int64_t)c0 * c1 * c2;
        for (int64_t e = tid; e < triples; e += BLOCK) {
            const int pick[3] = {cand[0][e / ((int64_t)c1 * c2)], cand[1][(e / c2) % c1], cand[2][e % c2]};
            int W[9];
#pragma unroll
            for (int i = 0; i < 3; ++i) {  // column i: the coefficients of the image of a_i
                W[i] = (pick[i] & 31) - RANGE;
                W[3 + i] = (pick[i] >> 5 & 31) - RANGE;
                W[6 + i] = (pick[i] >> 10 & 31) - RANGE;
            }
            const int det = det3i(W);
            if (det != 1 && det != -1) continue;
            double v[3][3];
#pragma unroll
            for (int i = 0; i < 3; ++i) lattice_vector(A, W[i], W[3 + i], W[6 + i], v[i]);
            const double g01 = norm3(v[0][0] - v[1][0], v[0][1] - v[1][1], v[0][2] - v[1][2]);
            const double g02 = norm3(v[0][0] - v[2][0], v[0][1] - v[2][1], v[0][2] - v[2][2]);
            const double g12 = norm3(v[1][0] - v[2][0], v[1][1] - v[2][1], v[1][2] - v[2][2]);
            if (fabs(g01 - want[0]) <= a.symprec && fabs(g02 - want[1]) <= a.symprec && fabs(g12 - want[2]) <= a.symprec) {
                const int slot = atomicAdd(&n_ops, 1);
                if (slot < MAX_OPS) keys[slot] = op_key(W);
            }
        }
    }
    __syncthreads();
    const int found = n_ops;
    if (found > MAX_OPS) status |= ALIGNN_SYM_STATUS_OVERFLOW;
    if (status == 0 && tid < found) {  // the rank of a key is its place: the keys differ
        const int64_t key = keys[tid];
        int rank = 0;
        for (int o = 0; o < found; ++o) rank += keys[o] < key ? 1 : 0;
        int64_t k = key;
        for (int j = 8; j >= 0; --j) {
            ops[9 * rank + j] = (int)(k % (2 * RANGE + 1)) - RANGE;
            k /= 2 * RANGE + 1;
        }
    }
    if (tid < INFO) info[tid] = tid == 4 ? status : tid == 5 ? (status ? 0 : found) : 0;
    if (tid < MAX_OPS) a.op_count[b * MAX_OPS + tid] = 0;  // (sym_accept_kernel adds to it)
}

// LDS of the acceptance and the fill: the sorted fractional coordinates, the species range of every sorted slot, the local index
extern __shared__ double sym_lds[];

__device__ __forceinline__ void stage(const FindArgs& a, const Rows& R, int max_atoms, double*& xs, int*& lo, int*& hi, int*& ord) {
    xs = sym_lds;
    lo = reinterpret_cast<int*>(sym_lds + 3 * (size_t)max_atoms);
    hi = lo + max_atoms;
    ord = hi + max_atoms;
    for (int q = threadIdx.x; q < R.n; q += BLOCK) {
        const int o = a.order[R.beg + q];
        const double* x = a.frac + 3 * ((int64_t)R.beg + o);
        xs[3 * q] = x[0];
        xs[3 * q + 1] = x[1];
        xs[3 * q + 2] = x[2];
        lo[q] = a.seg_lo[R.beg + q];
        hi[q] = a.seg_hi[R.beg + q];
        ord[q] = o;
    }
    __syncthreads();
}

__global__ __launch_bounds__(BLOCK) void sym_accept_kernel(const FindArgs a) {
    __shared__ int total;
    const int w = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    const int lane = tid & (ALIGNN_WAVE - 1), wave = tid / ALIGNN_WAVE;
    const int32_t* info = a.info + (int64_t)INFO * b;
    const Rows R = rows_of(a, b);
    // (uniform over the workgroup; sym_lattice_kernel has checked order and seg and has zeroed op_count)
    if (info[4] != 0 || w >= info[5] || !R.ok) return;
    const int js0 = blockIdx.z * CHUNK, js1 = min(R.phi - R.plo, js0 + CHUNK);
    if (js0 >= js1) return;
    if (tid == 0) total = 0;
    double* xs;
    int *lo, *hi, *ord;
    stage(a, R, a.max_atoms, xs, lo, hi, ord);
    double cell[9], W[9], yp[3];
    load9(a.lattice + 9 * (int64_t)b, cell);
    Matcher m;
    m.init(cell, a.symprec);
#pragma unroll
    for (int j = 0; j < 9; ++j) W[j] = (double)a.lattice_ops[((int64_t)b * MAX_OPS + w) * 9 + j];
    apply_w(W, xs + 3 * R.plo, yp);
    uint8_t* flags = a.accepted + (int64_t)MAX_OPS * R.beg + (int64_t)w * R.n;
    int mine = 0;
    for (int js = js0 + wave; js < js1; js += WAVES) {
        double t[3];
        translation(xs + 3 * (R.plo + js), yp, t);
        bool all = true;
        for (int q0 = 0; q0 < R.n && all; q0 += ALIGNN_WAVE) {
            const int q = q0 + lane;
            bool found = true;
            if (q < R.n) {
                double y[3], img[3], delta[3];
                apply_w(W, xs + 3 * q, y);
#pragma unroll
                for (int c = 0; c < 3; ++c) img[c] = y[c] + t[c];
                found = false;
                const int k1 = hi[q];
                for (int k = lo[q]; k < k1; ++k) {
                    if (m.near2(img, xs + 3 * k, delta) >= 0.0) {
                        found = true;
                        break;
                    }
                }
            }
            all = __ballot(!found) == 0ull;
        }
        if (lane == 0) flags[js] = all ? 1 : 0;
        mine += all ? 1 : 0;
    }
    if (lane == 0 && mine) atomicAdd(&total, mine);
    __syncthreads();
    if (tid == 0 && total) atomicAdd(a.op_count + b * MAX_OPS + w, total);  // (integers: exact in any order)
}

__global__ void sym_summary_kernel(const FindArgs a) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= a.n_structs) return;
    int32_t* info = a.info + (int64_t)INFO * b;
    const int n_lat = info[4] != 0 ? 0 : min(info[5], MAX_OPS);
    const int32_t* ops = a.lattice_ops + (int64_t)MAX_OPS * 9 * b;
    const int32_t* cnt = a.op_count + b * MAX_OPS;
    int n_ops = 0, n_tr = 0, pg = 0, of_order[7] = {0, 0, 0, 0, 0, 0, 0};
    for (int w = 0; w < n_lat; ++w) {
        if (cnt[w] <= 0) continue;
        n_ops += cnt[w];
        ++pg;
        int W[9], P[9];
        for (int j = 0; j < 9; ++j) W[j] = ops[9 * w + j];
        const int det = det3i(W);
        bool identity = true, first = true;
        for (int j = 0; j < 9; ++j) {
            P[j] = det * W[j];
            identity = identity && W[j] == (j % 4 == 0 ? 1 : 0);
        }
        if (identity) n_tr = cnt[w];
        for (int o = 0; o < w && first; ++o) {  // the proper part of an earlier accepted W?
            if (cnt[o] <= 0) continue;
            int V[9];
            for (int j = 0; j < 9; ++j) V[j] = ops[9 * o + j];
            const int dv = det3i(V);
            bool same = true;
            for (int j = 0; j < 9; ++j) same = same && dv * V[j] == P[j];
            first = !same;
        }
        if (!first) continue;
        const int tr = P[0] + P[4] + P[8];
        const int order = tr == 3 ? 1 : tr == -1 ? 2 : tr == 0 ? 3 : tr == 1 ? 4 : tr == 2 ? 6 : 0;
        ++of_order[order == 6 ? 5 : order];  // slots 1, 2, 3, 4 and 5 (order 6); 0: none of them
    }
    int system = 0;
    if (of_order[5] > 0) system = 5;
    else if (of_order[3] == 8) system = 6;
    else if (of_order[3] == 2) system = 4;
    else if (of_order[4] > 0) system = 3;
    else if (of_order[2] == 3) system = 2;
    else if (of_order[2] == 1) system = 1;
    info[0] = n_ops;
    info[1] = n_tr;
    info[2] = pg;
    info[3] = system;
}

__global__ __launch_bounds__(BLOCK) void sym_fill_kernel(const FindArgs a) {
    const int w = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    const int lane = tid & (ALIGNN_WAVE - 1), wave = tid / ALIGNN_WAVE;
    const int32_t* info = a.info + (int64_t)INFO * b;
    const Rows R = rows_of(a, b);
    if (info[4] != 0 || w >= info[5] || !R.ok) return;  // (uniform over the workgroup)
    const int32_t* cnt = a.op_count + b * MAX_OPS;
    const int js0 = blockIdx.z * CHUNK, js1 = min(R.phi - R.plo, js0 + CHUNK);
    if (cnt[w] <= 0 || js0 >= js1) return;
    const uint8_t* flags = a.accepted + (int64_t)MAX_OPS * R.beg + (int64_t)w * R.n;
    int here = 0;
    for (int js = js0; js < js1; ++js) here += flags[js] ? 1 : 0;  // (the same bytes for every thread)
    if (here == 0) return;
    int64_t base = 0;  // the operations of the structure that come before this workgroup's: earlier W, earlier candidates of W
    for (int o = 0; o < w; ++o) base += max(cnt[o], 0);
    for (int j0 = 0; j0 < js0; j0 += BLOCK) base += __syncthreads_count(j0 + tid < js0 && flags[j0 + tid]);
    const int64_t op0 = a.op_ptr[b], G = a.op_ptr[b + 1] - op0, map0 = a.map_ptr[b];
    double* xs;
    int *lo, *hi, *ord;
    stage(a, R, a.max_atoms, xs, lo, hi, ord);
    double cell[9], W[9], yp[3];
    load9(a.lattice + 9 * (int64_t)b, cell);
    Matcher m;
    m.init(cell, a.symprec);
    const int32_t* Wi = a.lattice_ops + ((int64_t)b * MAX_OPS + w) * 9;
#pragma unroll
    for (int j = 0; j < 9; ++j) W[j] = (double)Wi[j];
    apply_w(W, xs + 3 * R.plo, yp);
    for (int js = js0 + wave; js < js1; js += WAVES) {  // one wavefront per operation, its lanes over the atoms
        if (!flags[js]) continue;
        int64_t g = base;
        for (int o = js0; o < js; ++o) g += flags[o] ? 1 : 0;
        const int64_t og = op0 + g, row = map0 + g * R.n;
        if (g >= G || og < 0 || og >= a.n_ops_total || row < 0 || row + R.n > a.n_map_total) continue;  // (counts that do not fit)
        double t[3];
        translation(xs + 3 * (R.plo + js), yp, t);
        if (lane < 9) a.rotations[9 * og + lane] = Wi[lane];
        if (lane < 3) a.translations[3 * og + lane] = lane == 0 ? t[0] : lane == 1 ? t[1] : t[2];
        for (int q = lane; q < R.n; q += ALIGNN_WAVE) {
            double y[3], img[3], delta[3], best = -1.0;
            int at = -1, sh[3] = {0, 0, 0};
            apply_w(W, xs + 3 * q, y);
#pragma unroll
            for (int c = 0; c < 3; ++c) img[c] = y[c] + t[c];
            const int k1 = hi[q];
            for (int k = lo[q]; k < k1; ++k) {  // ascending local index within a species: the lowest of equals stays
                const double d2 = m.near2(img, xs + 3 * k, delta);
                if (d2 >= 0.0 && (at < 0 || d2 < best)) {
                    best = d2;
                    at = k;
#pragma unroll
                    for (int c = 0; c < 3; ++c) sh[c] = (int)rint(delta[c]);
                }
            }
            const int i = ord[q];
            a.atom_map[row + i] = at >= 0 ? ord[at] : i;
#pragma unroll
            for (int c = 0; c < 3; ++c) a.shifts[3 * (row + i) + c] = sh[c];
        }
    }
}

__global__ __launch_bounds__(BLOCK) void sym_orbits_kernel(const FindArgs a) {
    const int b = blockIdx.y, i = blockIdx.x * BLOCK + threadIdx.x;
    const int beg = a.atom_ptr[b], n = a.atom_ptr[b + 1] - beg;
    if (i >= n || beg < 0 || (int64_t)beg + n > a.n_atoms) return;
    const int64_t G = a.op_ptr[b + 1] - a.op_ptr[b], map0 = a.map_ptr[b];
    int lowest = i;
    if (map0 >= 0 && G >= 0 && map0 + G * n <= a.n_map_total)
        for (int64_t g = 0; g < G; ++g) lowest = min(lowest, a.atom_map[map0 + g * n + i]);
    a.orbits[beg + i] = lowest;
}

// --- the symmetrisers ----------------------------------------------------------------------------------------------------------
// the structure that owns row r: atom_ptr[b] <= r < atom_ptr[b + 1]
__device__ __forceinline__ int owner(const int32_t* ptr, int B, int r) {
    int lo = 0, hi = B;
    while (hi - lo > 1) {
        const int mid = (lo + hi) / 2;
        if (ptr[mid] <= r) lo = mid; else hi = mid;
    }
    return lo;
}

struct Ops {
    int64_t op0, G, map0;
    bool ok;
};

__device__ __forceinline__ Ops ops_of(const ApplyArgs& a, int b, int n) {
    Ops o;
    o.op0 = a.op_ptr[b];
    o.G = a.op_ptr[b + 1] - o.op0;
    o.map0 = a.map_ptr[b];
    o.ok = o.op0 >= 0 && o.G >= 1 && o.op0 + o.G <= a.n_ops_total && (!a.atom_map || (o.map0 >= 0 && o.map0 + o.G * n <= a.n_map_total));
    return o;
}

__global__ __launch_bounds__(BLOCK) void sym_forces_kernel(const ApplyArgs a) {
    const int r = blockIdx.x * BLOCK + threadIdx.x;
    if (r >= a.n_atoms) return;
    const int b = owner(a.atom_ptr, a.n_structs, r), beg = a.atom_ptr[b], n = a.atom_ptr[b + 1] - beg, i = r - beg;
    const Ops o = ops_of(a, b, n);
    double acc[3] = {0.0, 0.0, 0.0};
    if (!o.ok || i >= n) {
#pragma unroll
        for (int c = 0; c < 3; ++c) a.out[3 * (int64_t)r + c] = a.in[3 * (int64_t)r + c];
        return;
    }
    double A[9], Ai[9], Q[9];
    load9(a.lattice + 9 * (int64_t)b, A);
    inv3_cof(A, Ai);
    for (int64_t g = 0; g < o.G; ++g) {
        cartesian_rotation(A, Ai, a.rotations + 9 * (o.op0 + g), Q);
        int k = a.atom_map[o.map0 + g * n + i];
        if (k < 0 || k >= n) k = i;
        const double* F = a.in + 3 * ((int64_t)beg + k);
#pragma unroll
        for (int d = 0; d < 3; ++d) acc[d] = acc[d] + ((Q[d] * F[0] + Q[3 + d] * F[1]) + Q[6 + d] * F[2]);
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) a.out[3 * (int64_t)r + c] = acc[c] / (double)o.G;
}

__global__ __launch_bounds__(BLOCK) void sym_stress_kernel(const ApplyArgs a) {
    const int e = blockIdx.x * BLOCK + threadIdx.x;
    if (e >= 9 * a.n_structs) return;
    const int b = e / 9, r = (e % 9) / 3, c = e % 3;
    const Ops o = ops_of(a, b, 0);
    const double* S = a.in + 9 * (int64_t)b;
    if (!o.ok) {
        a.out[e] = S[3 * r + c];
        return;
    }
    double A[9], Ai[9], Q[9], acc = 0.0;
    load9(a.lattice + 9 * (int64_t)b, A);
    inv3_cof(A, Ai);
    for (int64_t g = 0; g < o.G; ++g) {
        cartesian_rotation(A, Ai, a.rotations + 9 * (o.op0 + g), Q);
        double u[3];
#pragma unroll
        for (int p = 0; p < 3; ++p) u[p] = (S[3 * p] * Q[c] + S[3 * p + 1] * Q[3 + c]) + S[3 * p + 2] * Q[6 + c];
        acc = acc + ((Q[r] * u[0] + Q[3 + r] * u[1]) + Q[6 + r] * u[2]);
    }
    a.out[e] = acc / (double)o.G;
}

__global__ __launch_bounds__(BLOCK) void sym_positions_kernel(const ApplyArgs a) {
    const int r = blockIdx.x * BLOCK + threadIdx.x;
    if (r >= a.n_atoms) return;
    const int b = owner(a.atom_ptr, a.n_structs, r), beg = a.atom_ptr[b], n = a.atom_ptr[b + 1] - beg, i = r - beg;
    const Ops o = ops_of(a, b, n);
    if (!o.ok || i >= n) {
#pragma unroll
        for (int c = 0; c < 3; ++c) a.out[3 * (int64_t)r + c] = a.in[3 * (int64_t)r + c];
        return;
    }
    double A[9], Ai[9], acc[3] = {0.0, 0.0, 0.0};
    load9(a.lattice + 9 * (int64_t)b, A);
    inv3_cof(A, Ai);
    for (int64_t g = 0; g < o.G; ++g) {
        const int32_t* Wg = a.rotations + 9 * (o.op0 + g);
        int W[9];
#pragma unroll
        for (int j = 0; j < 9; ++j) W[j] = Wg[j];
        const double det = (double)det3i(W);
        const double V[9] = {det * (double)(W[4] * W[8] - W[5] * W[7]), det * (double)(W[2] * W[7] - W[1] * W[8]), det * (double)(W[1] * W[5] - W[2] * W[4]),
                             det * (double)(W[5] * W[6] - W[3] * W[8]), det * (double)(W[0] * W[8] - W[2] * W[6]), det * (double)(W[2] * W[3] - W[0] * W[5]),
                             det * (double)(W[3] * W[7] - W[4] * W[6]), det * (double)(W[1] * W[6] - W[0] * W[7]), det * (double)(W[0] * W[4] - W[1] * W[3])};
        const int64_t at = o.map0 + g * n + i;
        int k = a.atom_map[at];
        if (k < 0 || k >= n) k = i;
        const double* rk = a.in + 3 * ((int64_t)beg + k);
        double u[3], term[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) u[c] = (row_dot(rk, Ai, c) + (double)a.shifts[3 * at + c]) - a.translations[3 * (o.op0 + g) + c];
        apply_w(V, u, term);
#pragma unroll
        for (int c = 0; c < 3; ++c) acc[c] = acc[c] + term[c];
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) acc[c] = acc[c] / (double)o.G;
#pragma unroll
    for (int c = 0; c < 3; ++c) a.out[3 * (int64_t)r + c] = row_dot(acc, A, c);
}

bool find_args_ok(const FindArgs& a) {
    if (a.n_structs < 0 || a.n_structs > 65535 || a.n_atoms < 0) return false;
    return a.symprec > 0.0 && a.symprec < 1e300;  // (a NaN fails)
}

bool find_rows_ok(const FindArgs& a) {
    return a.n_atoms >= 1 && a.max_atoms >= 1 && a.max_atoms <= a.n_atoms && a.max_atoms <= ALIGNN_SYM_MAX_ATOMS && a.lattice && a.pos &&
           a.atom_ptr && a.order && a.seg_lo && a.seg_hi && a.pivot_lo && a.pivot_hi && a.frac && a.lattice_ops && a.accepted &&
           a.op_count && a.info;
}

size_t lds_bytes(int max_atoms) { return (size_t)max_atoms * (3 * sizeof(double) + 3 * sizeof(int)); }

bool apply_args_ok(const ApplyArgs& a) {
    return a.n_structs >= 0 && a.n_structs <= 65535 && a.n_atoms >= 0 && a.n_ops_total >= 0 && a.n_map_total >= 0;
}

}  // namespace

extern "C" size_t alignn_sym_find_args_size(void) { return sizeof(alignn_sym_find_args); }
extern "C" size_t alignn_sym_apply_args_size(void) { return sizeof(alignn_sym_apply_args); }

extern "C" int alignn_sym_search(const alignn_sym_find_args* args, void* stream) {
    if (!args || !find_args_ok(*args)) return (int)hipErrorInvalidValue;
    const FindArgs& a = *args;
    if (a.n_structs == 0) return 0;
    if (!find_rows_ok(a)) return (int)hipErrorInvalidValue;
    hipStream_t s = (hipStream_t)stream;
    sym_lattice_kernel<<<a.n_structs, BLOCK, 0, s>>>(a);
    ALIGNN_CHECK_LAUNCH();
    sym_accept_kernel<<<dim3(MAX_OPS, a.n_structs, alignn_ceil_div(a.max_atoms, CHUNK)), BLOCK, lds_bytes(a.max_atoms), s>>>(a);
    ALIGNN_CHECK_LAUNCH();
    sym_summary_kernel<<<alignn_ceil_div(a.n_structs, ALIGNN_WAVE), ALIGNN_WAVE, 0, s>>>(a);
    ALIGNN_CHECK_LAUNCH();
    return 0;
}

extern "C" int alignn_sym_fill(const alignn_sym_find_args* args, void* stream) {
    if (!args || !find_args_ok(*args) || args->n_ops_total < 0 || args->n_map_total < 0) return (int)hipErrorInvalidValue;
    const FindArgs& a = *args;
    if (a.n_structs == 0) return 0;
    if (!find_rows_ok(a) || !a.op_ptr || !a.map_ptr || !a.orbits) return (int)hipErrorInvalidValue;
    if (a.n_ops_total > 0 && (!a.rotations || !a.translations)) return (int)hipErrorInvalidValue;
    if (a.n_map_total > 0 && (!a.atom_map || !a.shifts)) return (int)hipErrorInvalidValue;
    hipStream_t s = (hipStream_t)stream;
    if (a.n_ops_total > 0 && a.n_map_total > 0) {
        sym_fill_kernel<<<dim3(MAX_OPS, a.n_structs, alignn_ceil_div(a.max_atoms, CHUNK)), BLOCK, lds_bytes(a.max_atoms), s>>>(a);
        ALIGNN_CHECK_LAUNCH();
    }
    sym_orbits_kernel<<<dim3(alignn_ceil_div(a.max_atoms, BLOCK), a.n_structs), BLOCK, 0, s>>>(a);
    ALIGNN_CHECK_LAUNCH();
    return 0;
}

static int apply_common(const alignn_sym_apply_args* args, bool per_atom, bool positions) {
    if (!args || !apply_args_ok(*args)) return (int)hipErrorInvalidValue;
    const ApplyArgs& a = *args;
    if (a.n_structs == 0) return 0;
    if (!a.lattice || !a.in || !a.out || !a.op_ptr || !a.map_ptr) return (int)hipErrorInvalidValue;
    if (a.n_ops_total > 0 && !a.rotations) return (int)hipErrorInvalidValue;
    if (per_atom && (a.n_atoms < 1 || !a.atom_ptr || (a.n_map_total > 0 && !a.atom_map))) return (int)hipErrorInvalidValue;
    if (per_atom && a.n_ops_total > 0 && a.n_map_total == 0) return (int)hipErrorInvalidValue;
    if (positions && a.n_ops_total > 0 && (!a.translations || !a.shifts)) return (int)hipErrorInvalidValue;
    return -1;  // launch
}

extern "C" int alignn_sym_forces(const alignn_sym_apply_args* args, void* stream) {
    const int rc = apply_common(args, true, false);
    if (rc >= 0) return rc;
    sym_forces_kernel<<<alignn_ceil_div(args->n_atoms, BLOCK), BLOCK, 0, (hipStream_t)stream>>>(*args);
    ALIGNN_CHECK_LAUNCH();
    return 0;
}

extern "C" int alignn_sym_stress(const alignn_sym_apply_args* args, void* stream) {
    const int rc = apply_common(args, false, false);
    if (rc >= 0) return rc;
    ApplyArgs a = *args;
    a.atom_map = nullptr;  // (not used: the check of a structure's operations leaves the map out)
    sym_stress_kernel<<<alignn_ceil_div(9 * (int64_t)a.n_structs, BLOCK), BLOCK, 0, (hipStream_t)stream>>>(a);
    ALIGNN_CHECK_LAUNCH();
    return 0;
}

extern "C" int alignn_sym_positions(const alignn_sym_apply_args* args, void* stream) {
    const int rc = apply_common(args, true, true);
    if (rc >= 0) return rc;
    sym_positions_kernel<<<alignn_ceil_div(args->n_atoms, BLOCK), BLOCK, 0, (hipStream_t)stream>>>(*args);
    ALIGNN_CHECK_LAUNCH();
    return 0;
}
