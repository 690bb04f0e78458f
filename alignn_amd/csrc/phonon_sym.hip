// Phonons from symmetry-reduced displacements: the rules of include/alignn_phsym.h (alignn_amd/phonons.py is the host loop;
// tests/phonons_sym_ref.py the numpy restatement this file follows).  float64 throughout, without contraction, no float atomics,
// every sum in a fixed order.
//
//   phsym_plan_kernel        per structure: the usable operations and their Cartesian rotations, the representatives, their site
//                            groups, the direction search, Minv, and the distributing operation of every other atom;
//   phsym_displace_kernel    phonon_displace_kernel's arithmetic with a direction per job, one workgroup per supercell;
//   phsym_rows_kernel        G_m from the forces of a -/+ pair (the arithmetic of phonon_fc_rows_kernel: phonon_rows.h);
//   phsym_solve_kernel       Phi(i; B) = Minv sum_{g, m} u_gm (G_m[g~ B] Q_g): a thread per supercell atom B, the site group in LDS;
//   phsym_distribute_kernel  Phi(i'; g~ B) = Q Phi(i; B) Q^T for the atoms that were not displaced.
#include "../../include/alignn_phsym.h"
#include "common.h"
#include "cell3.h"
#include "phonon_rows.h"

#pragma clang fp contract(off)

namespace {

constexpr int MAX_ATOMS = ALIGNN_PHSYM_MAX_ATOMS, MAX_SITE = ALIGNN_PHSYM_MAX_SITE_OPS, N_CAND = ALIGNN_PHSYM_N_CANDIDATES;
constexpr double TAU = ALIGNN_PHSYM_TAU;
constexpr double R2 = 0.7071067811865475, R3 = 0.5773502691896258;  // 1 / sqrt(2), 1 / sqrt(3) as float64 divisions give them

using PlanArgs = alignn_phsym_plan_args;
using DisplaceArgs = alignn_phsym_displace_args;
using RowsArgs = alignn_phsym_rows_args;
using FcArgs = alignn_phsym_fc_args;

__constant__ double CANDIDATES[N_CAND][3] = {{1.0, 0.0, 0.0}, {0.0, 1.0, 0.0}, {0.0, 0.0, 1.0}, {R2, R2, 0.0},  {R2, 0.0, R2},
                                             {0.0, R2, R2},   {R2, -R2, 0.0},  {R2, 0.0, -R2},  {0.0, R2, -R2}, {R3, R3, R3},
                                             {R3, R3, -R3},   {R3, -R3, R3},   {-R3, R3, R3}};

// a structure's slices of the packed symmetry arrays, checked against the arrays' sizes
struct Slices {
    int beg, n;
    int64_t op0, G, map0;
    Cells c;
    bool ok;
};

__device__ __forceinline__ Slices slices_of(const int32_t* atom_ptr, const int64_t* op_ptr, const int64_t* map_ptr,
                                            const int32_t* dims, int s, int n_atoms, int64_t n_ops_total, int64_t n_map_total) {
    Slices o;
    o.beg = atom_ptr[s];
    o.n = atom_ptr[s + 1] - o.beg;
    o.op0 = op_ptr[s];
    o.G = op_ptr[s + 1] - o.op0;
    o.map0 = map_ptr[s];
    o.c = cells_of(dims, s);
    o.ok = o.beg >= 0 && o.n >= 1 && o.n <= MAX_ATOMS && o.beg + o.n <= n_atoms && o.op0 >= 0 && o.G >= 1 &&
           o.op0 + o.G <= n_ops_total && o.map0 >= 0 && o.map0 + o.G * o.n <= n_map_total && o.c.n0 >= 1 && o.c.n1 >= 1 &&
           o.c.n2 >= 1;
    return o;
}

__device__ __forceinline__ int mod_into(int v, int N) {
    const int r = v % N;
    return r < 0 ? r + N : r;
}

// g~ (m, j) = ((W m + shift_j - back) mod N, map_j) as a supercell atom index; -1 when map_j is no atom of the structure
__device__ __forceinline__ int image_of(const int* W, const int32_t* shift_j, const int* back, int map_j, int cell, int n,
                                        const Cells& c) {
    if (map_j < 0 || map_j >= n) return -1;
    const int m[3] = {cell / (c.n1 * c.n2), (cell / c.n2) % c.n1, cell % c.n2};
    const int N[3] = {c.n0, c.n1, c.n2};
    int mm[3];
#pragma unroll
    for (int r = 0; r < 3; ++r)
        mm[r] = mod_into(((W[3 * r] * m[0] + W[3 * r + 1] * m[1]) + W[3 * r + 2] * m[2]) + shift_j[r] - back[r], N[r]);
    return ((mm[0] * c.n1 + mm[1]) * c.n2 + mm[2]) * n + map_j;
}

// u = Q^T d
__device__ __forceinline__ void image_of_direction(const double* Q, const double* d, double (&u)[3]) {
#pragma unroll
    for (int a = 0; a < 3; ++a) u[a] = (Q[a] * d[0] + Q[3 + a] * d[1]) + Q[6 + a] * d[2];
}

// M = sum over the site group, then the k directions, of u u^T
__device__ __forceinline__ void span_matrix(const double* rot, const int32_t* site, int n_site, const double (*dirs)[3], int k,
                                            double (&M)[9]) {
#pragma unroll
    for (int e = 0; e < 9; ++e) M[e] = 0.0;
    for (int q = 0; q < n_site; ++q) {
        const double* Q = rot + 9 * (int64_t)site[q];
        for (int m = 0; m < k; ++m) {
            double u[3];
            image_of_direction(Q, dirs[m], u);
#pragma unroll
            for (int a = 0; a < 3; ++a)
#pragma unroll
                for (int b = 0; b < 3; ++b) M[3 * a + b] = M[3 * a + b] + u[a] * u[b];
        }
    }
}

__device__ __forceinline__ bool spans(const double (&M)[9]) {
    const double c00 = M[4] * M[8] - M[5] * M[7], c01 = M[3] * M[8] - M[5] * M[6], c02 = M[3] * M[7] - M[4] * M[6];
    const double det = (M[0] * c00 - M[1] * c01) + M[2] * c02;
    const double t = ((M[0] + M[4]) + M[8]) / 3.0;
    return det >= TAU * ((t * t) * t);
}

__global__ __launch_bounds__(PH_BLOCK) void phsym_plan_kernel(const PlanArgs a) {
    __shared__ int label[MAX_ATOMS];
    __shared__ int bad;
    const int s = blockIdx.x;
    const Slices o = slices_of(a.atom_ptr, a.op_ptr, a.map_ptr, a.supercell, s, a.n_atoms, a.n_ops_total, a.n_map_total);
    if (!o.ok) {
        for (int64_t i = (int64_t)o.beg + threadIdx.x; i < (int64_t)o.beg + o.n && i < a.n_atoms; i += PH_BLOCK)
            if (i >= 0) a.n_dir[i] = -1;
        return;
    }
    const int n = o.n;
    if (threadIdx.x == 0) bad = 0;
    __syncthreads();
    // rule 1, and Q_g of every operation
    double A[9], Ai[9];
    load9(a.lattice + 9 * (int64_t)s, A);
    inv3_cof(A, Ai);
    const int N[3] = {o.c.n0, o.c.n1, o.c.n2};
    for (int64_t g = threadIdx.x; g < o.G; g += PH_BLOCK) {
        const int32_t* W = a.rotations + 9 * (o.op0 + g);
        bool use = true, identity = true;
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                use = use && ((int64_t)W[3 * r + c] * N[c]) % N[r] == 0;
                identity = identity && W[3 * r + c] == (r == c ? 1 : 0);
            }
        a.usable[o.op0 + g] = use ? 1 : 0;
        double Q[9];
        if (identity) {
#pragma unroll
            for (int e = 0; e < 9; ++e) Q[e] = (e % 4 == 0) ? 1.0 : 0.0;
        } else {
            cartesian_rotation(A, Ai, W, Q);
        }
#pragma unroll
        for (int e = 0; e < 9; ++e) a.rot[9 * (o.op0 + g) + e] = Q[e];
        for (int j = 0; j < n; ++j) {
            const int k = a.atom_map[o.map0 + g * n + j];
            if (k < 0 || k >= n) bad = 1;
        }
    }
    __syncthreads();
    // rule 2: the classes under the usable operations, named by their lowest atom (a handful of integers: one thread)
    if (threadIdx.x == 0 && !bad) {
        for (int j = 0; j < n; ++j) label[j] = j;
        bool changed = true;
        while (changed) {
            changed = false;
            for (int64_t g = 0; g < o.G; ++g) {
                if (!a.usable[o.op0 + g]) continue;
                for (int j = 0; j < n; ++j) {
                    const int k = a.atom_map[o.map0 + g * n + j];
                    const int lo = min(label[j], label[k]);
                    if (label[j] != lo || label[k] != lo) {
                        label[j] = label[k] = lo;
                        changed = true;
                    }
                }
            }
        }
    }
    __syncthreads();
    const bool broken = bad != 0;
    __syncthreads();
    // rules 3 and 4 for a representative, the choice of rule 6 for the others: one thread per atom
    const int i = threadIdx.x;
    bool fail = broken;
    if (i < n && !broken) {
        const int64_t row = (int64_t)o.beg + i;
        const int rep = label[i];
        a.rep[row] = rep;
        int32_t* site = a.site_ops + MAX_SITE * row;
        double* dirs_out = a.dirs + 9 * row;
        double* minv_out = a.minv + 9 * row;
#pragma unroll
        for (int e = 0; e < 9; ++e) dirs_out[e] = minv_out[e] = 0.0;
        if (rep == i) {
            int count = 0;
            for (int64_t g = 0; g < o.G; ++g)
                if (a.usable[o.op0 + g] && a.atom_map[o.map0 + g * n + i] == i) {
                    if (count < MAX_SITE) site[count] = (int)g;
                    ++count;
                }
            a.dist_op[row] = -1;
            if (count < 1 || count > MAX_SITE) {
                fail = true;
            } else {
                for (int q = count; q < MAX_SITE; ++q) site[q] = -1;
                a.n_site[row] = count;
                const double* rot = a.rot + 9 * o.op0;
                double d[3][3], M[9];
                int k = 0;
                for (int c0 = 0; c0 < N_CAND && k == 0; ++c0) {
#pragma unroll
                    for (int x = 0; x < 3; ++x) d[0][x] = CANDIDATES[c0][x];
                    span_matrix(rot, site, count, d, 1, M);
                    if (spans(M)) k = 1;
                }
                for (int c0 = 0; c0 < N_CAND && k == 0; ++c0)
                    for (int c1 = c0 + 1; c1 < N_CAND && k == 0; ++c1) {
#pragma unroll
                        for (int x = 0; x < 3; ++x) {
                            d[0][x] = CANDIDATES[c0][x];
                            d[1][x] = CANDIDATES[c1][x];
                        }
                        span_matrix(rot, site, count, d, 2, M);
                        if (spans(M)) k = 2;
                    }
                if (k == 0) {
                    k = 3;
#pragma unroll
                    for (int m = 0; m < 3; ++m)
#pragma unroll
                        for (int x = 0; x < 3; ++x) d[m][x] = CANDIDATES[m][x];
                    span_matrix(rot, site, count, d, 3, M);
                }
                double Mi[9];
                inv3_cof(M, Mi);
                for (int m = 0; m < k; ++m)
#pragma unroll
                    for (int x = 0; x < 3; ++x) dirs_out[3 * m + x] = d[m][x];
#pragma unroll
                for (int e = 0; e < 9; ++e) minv_out[e] = Mi[e];
                a.n_dir[row] = k;
            }
        } else {
            int found = -1;
            for (int64_t g = 0; g < o.G && found < 0; ++g)
                if (a.usable[o.op0 + g] && a.atom_map[o.map0 + g * n + rep] == i) found = (int)g;
            for (int q = 0; q < MAX_SITE; ++q) site[q] = -1;
            a.n_site[row] = 0;
            a.dist_op[row] = found;
            a.n_dir[row] = 0;
            if (found < 0) fail = true;
        }
    }
    // a structure that cannot be planned says so in every atom's n_dir
    if (__syncthreads_or(fail ? 1 : 0)) {
        if (i < n) a.n_dir[(int64_t)o.beg + i] = -1;
    }
}

__global__ __launch_bounds__(PH_BLOCK) void phsym_displace_kernel(const DisplaceArgs a) {
    const int job = blockIdx.x;
    const int s = a.jobs[4 * job], atom = a.jobs[4 * job + 1], dm = a.jobs[4 * job + 2], sg = a.jobs[4 * job + 3];
    if (s < 0 || s >= a.n_structs) return;
    const int beg = a.atom_ptr[s], n = a.atom_ptr[s + 1] - beg;
    if (atom < 0 || atom >= n || dm < 0 || dm > 2) return;
    const Cells c = cells_of(a.supercell, s);
    const double disp = sg ? a.delta : -a.delta;
    const double* L = a.lattice + 9 * (int64_t)s;
    const double* S = a.inv_supercell + 9 * (int64_t)s;
    const double* d = a.dirs + 9 * ((int64_t)beg + atom) + 3 * dm;
    const int64_t row0 = a.row_off[job];
    const int n_sc = n * c.count();
    for (int j = threadIdx.x; j < n_sc; j += PH_BLOCK) {
        const int img = j / n, b = j - img * n;
        const double m2 = (double)(img % c.n2), m1 = (double)((img / c.n2) % c.n1), m0 = (double)(img / (c.n1 * c.n2));
        double r[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            r[k] = a.positions[3 * ((int64_t)beg + b) + k] + m0 * L[k];
            r[k] = r[k] + m1 * L[3 + k];
            r[k] = r[k] + m2 * L[6 + k];
        }
        if (j == atom) {
#pragma unroll
            for (int k = 0; k < 3; ++k) r[k] = r[k] + disp * d[k];
        }
        const int64_t row = row0 + j;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            double f = r[0] * S[k] + r[1] * S[3 + k];
            f = f + r[2] * S[6 + k];
            a.frac[3 * row + k] = wrap01(f);
            if (a.cart) a.cart[3 * row + k] = r[k];
        }
    }
}

__global__ __launch_bounds__(PH_BLOCK) void phsym_rows_kernel(const RowsArgs a) {
    __shared__ double sh[6][PH_WAVES];
    const int p = blockIdx.x;
    const int s = a.pairs[2 * p], atom = a.pairs[2 * p + 1];
    if (s < 0 || s >= a.n_structs) return;  // (uniform over the workgroup)
    const int n = a.atom_ptr[s + 1] - a.atom_ptr[s];
    const int n_sc = n * cells_of(a.supercell, s).count();
    const double* Fm = a.forces + 3 * a.pair_rows[p];
    double* G = a.g + 3 * a.out_rows[p];
    difference_rows(Fm, Fm + 3 * (int64_t)n_sc, n_sc, atom, a.drift, a.delta, sh,
                    [&](int j, int k, double v) { G[3 * (int64_t)j + k] = v; });
}

// LDS of the solve: the site group of the workgroup's representative
struct SiteGroup {
    double Q[MAX_SITE][9];
    double u[MAX_SITE][3][3];
    double Minv[9];
    int W[MAX_SITE][9];
    int back[MAX_SITE][3];  // shift[g][i]
    int op[MAX_SITE];
};

__global__ __launch_bounds__(PH_BLOCK) void phsym_solve_kernel(const FcArgs a) {
    __shared__ SiteGroup sg;
    const int item = blockIdx.y;
    const int s = a.items[2 * item], i = a.items[2 * item + 1];
    if (s < 0 || s >= a.n_structs) return;
    const Slices o = slices_of(a.atom_ptr, a.op_ptr, a.map_ptr, a.supercell, s, INT32_MAX, a.n_ops_total, a.n_map_total);
    if (!o.ok || i < 0 || i >= o.n) return;
    const int n = o.n, n_sc = n * o.c.count();
    if ((int64_t)blockIdx.x * PH_BLOCK >= n_sc) return;
    const int64_t row = (int64_t)o.beg + i;
    const int S = a.n_site[row], k = a.n_dir[row];
    if (S < 1 || S > MAX_SITE || k < 1 || k > 3) return;
    for (int q = threadIdx.x; q < S; q += PH_BLOCK) {
        int g = a.site_ops[MAX_SITE * row + q];
        if (g < 0 || g >= o.G) g = 0;
        sg.op[q] = g;
        const double* Q = a.rot + 9 * (o.op0 + g);
        const int32_t* W = a.rotations + 9 * (o.op0 + g);
#pragma unroll
        for (int e = 0; e < 9; ++e) {
            sg.Q[q][e] = Q[e];
            sg.W[q][e] = W[e];
        }
#pragma unroll
        for (int r = 0; r < 3; ++r) sg.back[q][r] = a.shifts[3 * (o.map0 + (int64_t)g * n + i) + r];
        for (int m = 0; m < k; ++m) {
            double u[3];
            image_of_direction(Q, a.dirs + 9 * row + 3 * m, u);
#pragma unroll
            for (int x = 0; x < 3; ++x) sg.u[q][m][x] = u[x];
        }
    }
    if (threadIdx.x < 9) sg.Minv[threadIdx.x] = a.minv[9 * row + threadIdx.x];
    __syncthreads();
    const int B = blockIdx.x * PH_BLOCK + threadIdx.x;
    if (B >= n_sc) return;
    const int cell = B / n, j = B - cell * n;
    const double* G0 = a.g + 3 * a.g_rows[item];
    double T[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int q = 0; q < S; ++q) {
        const int64_t at = o.map0 + (int64_t)sg.op[q] * n + j;
        const int Bp = image_of(sg.W[q], a.shifts + 3 * at, sg.back[q], a.atom_map[at], cell, n, o.c);
        if (Bp < 0) return;
        for (int m = 0; m < k; ++m) {
            const double* Gm = G0 + 3 * ((int64_t)m * n_sc + Bp);
            const double g0 = Gm[0], g1 = Gm[1], g2 = Gm[2];
            double rowQ[3];
#pragma unroll
            for (int b = 0; b < 3; ++b) rowQ[b] = (g0 * sg.Q[q][b] + g1 * sg.Q[q][3 + b]) + g2 * sg.Q[q][6 + b];
#pragma unroll
            for (int x = 0; x < 3; ++x)
#pragma unroll
                for (int b = 0; b < 3; ++b) T[3 * x + b] = T[3 * x + b] + sg.u[q][m][x] * rowQ[b];
        }
    }
    const int M = 3 * n;
    double* C = a.fc + a.fc_off[s] + ((int64_t)cell * M + 3 * i) * M + 3 * j;
#pragma unroll
    for (int x = 0; x < 3; ++x)
#pragma unroll
        for (int b = 0; b < 3; ++b)
            C[(int64_t)x * M + b] = (sg.Minv[3 * x] * T[b] + sg.Minv[3 * x + 1] * T[3 + b]) + sg.Minv[3 * x + 2] * T[6 + b];
}

__global__ __launch_bounds__(PH_BLOCK) void phsym_distribute_kernel(const FcArgs a) {
    const int item = blockIdx.y;
    const int s = a.items[2 * item], ip = a.items[2 * item + 1];
    if (s < 0 || s >= a.n_structs) return;
    const Slices o = slices_of(a.atom_ptr, a.op_ptr, a.map_ptr, a.supercell, s, INT32_MAX, a.n_ops_total, a.n_map_total);
    if (!o.ok || ip < 0 || ip >= o.n) return;
    const int n = o.n, n_sc = n * o.c.count();
    const int B = blockIdx.x * PH_BLOCK + threadIdx.x;
    if (B >= n_sc) return;
    const int i = a.rep[(int64_t)o.beg + ip], g = a.dist_op[(int64_t)o.beg + ip];
    if (i < 0 || i >= n || i == ip || g < 0 || g >= o.G) return;
    const int cell = B / n, j = B - cell * n;
    int W[9], back[3];
    double Q[9];
#pragma unroll
    for (int e = 0; e < 9; ++e) {
        W[e] = a.rotations[9 * (o.op0 + g) + e];
        Q[e] = a.rot[9 * (o.op0 + g) + e];
    }
#pragma unroll
    for (int r = 0; r < 3; ++r) back[r] = a.shifts[3 * (o.map0 + (int64_t)g * n + i) + r];
    const int64_t at = o.map0 + (int64_t)g * n + j;
    const int jp = a.atom_map[at];
    const int Bp = image_of(W, a.shifts + 3 * at, back, jp, cell, n, o.c);
    if (Bp < 0) return;
    const int M = 3 * n;
    double* base = a.fc + a.fc_off[s];
    const double* Pin = base + ((int64_t)cell * M + 3 * i) * M + 3 * j;
    double P[9], PQ[9];
#pragma unroll
    for (int x = 0; x < 3; ++x)
#pragma unroll
        for (int b = 0; b < 3; ++b) P[3 * x + b] = Pin[(int64_t)x * M + b];
#pragma unroll
    for (int x = 0; x < 3; ++x)
#pragma unroll
        for (int b = 0; b < 3; ++b) PQ[3 * x + b] = (P[3 * x] * Q[3 * b] + P[3 * x + 1] * Q[3 * b + 1]) + P[3 * x + 2] * Q[3 * b + 2];
    const int cellp = Bp / n;
    double* out = base + ((int64_t)cellp * M + 3 * ip) * M + 3 * jp;
#pragma unroll
    for (int x = 0; x < 3; ++x)
#pragma unroll
        for (int b = 0; b < 3; ++b) out[(int64_t)x * M + b] = (Q[3 * x] * PQ[b] + Q[3 * x + 1] * PQ[3 + b]) + Q[3 * x + 2] * PQ[6 + b];
}

bool finite_positive(double v) { return v > 0.0 && v < 1e300; }  // (a NaN fails)

bool fc_args_ok(const FcArgs& a) {
    return a.n_items >= 0 && a.n_structs >= 0 && a.n_structs <= 65535 && a.n_ops_total >= 0 && a.n_map_total >= 0;
}

bool fc_rows_ok(const FcArgs& a) {
    return a.n_structs >= 1 && a.n_ops_total >= 1 && a.n_map_total >= 1 && a.max_supercell_atoms >= 1 && a.n_items <= 65535 &&
           a.items && a.fc && a.fc_off && a.atom_ptr && a.supercell && a.op_ptr && a.map_ptr && a.rotations && a.atom_map &&
           a.shifts && a.rot;
}

}  // namespace

extern "C" size_t alignn_phsym_plan_args_size(void) { return sizeof(alignn_phsym_plan_args); }
extern "C" size_t alignn_phsym_displace_args_size(void) { return sizeof(alignn_phsym_displace_args); }
extern "C" size_t alignn_phsym_rows_args_size(void) { return sizeof(alignn_phsym_rows_args); }
extern "C" size_t alignn_phsym_fc_args_size(void) { return sizeof(alignn_phsym_fc_args); }

extern "C" int alignn_phsym_plan(const alignn_phsym_plan_args* args, void* stream) {
    if (!args || args->n_structs < 0 || args->n_structs > 65535 || args->n_atoms < 0 || args->n_ops_total < 0 ||
        args->n_map_total < 0)
        return (int)hipErrorInvalidValue;
    const PlanArgs& a = *args;
    if (a.n_structs == 0) return 0;
    if (a.n_atoms < 1 || a.n_ops_total < 1 || a.n_map_total < 1 || !a.lattice || !a.supercell || !a.atom_ptr || !a.op_ptr ||
        !a.map_ptr || !a.rotations || !a.atom_map || !a.usable || !a.rot || !a.rep || !a.n_site || !a.site_ops || !a.n_dir ||
        !a.dirs || !a.minv || !a.dist_op)
        return (int)hipErrorInvalidValue;
    phsym_plan_kernel<<<a.n_structs, PH_BLOCK, 0, (hipStream_t)stream>>>(a);
    ALIGNN_CHECK_LAUNCH();
    return 0;
}

extern "C" int alignn_phsym_displace(const alignn_phsym_displace_args* args, void* stream) {
    if (!args || args->n_jobs < 0 || args->n_structs < 0 || !finite_positive(args->delta)) return (int)hipErrorInvalidValue;
    const DisplaceArgs& a = *args;
    if (a.n_jobs == 0) return 0;
    if (a.n_structs < 1 || !a.positions || !a.atom_ptr || !a.lattice || !a.inv_supercell || !a.supercell || !a.dirs || !a.jobs ||
        !a.row_off || !a.frac)
        return (int)hipErrorInvalidValue;
    phsym_displace_kernel<<<a.n_jobs, PH_BLOCK, 0, (hipStream_t)stream>>>(a);
    ALIGNN_CHECK_LAUNCH();
    return 0;
}

extern "C" int alignn_phsym_rows(const alignn_phsym_rows_args* args, void* stream) {
    if (!args || args->n_pairs < 0 || args->n_structs < 0 || args->drift < DRIFT_NONE || args->drift > DRIFT_MEAN ||
        !finite_positive(args->delta))
        return (int)hipErrorInvalidValue;
    const RowsArgs& a = *args;
    if (a.n_pairs == 0) return 0;
    if (a.n_structs < 1 || !a.forces || !a.pairs || !a.pair_rows || !a.out_rows || !a.atom_ptr || !a.supercell || !a.g)
        return (int)hipErrorInvalidValue;
    phsym_rows_kernel<<<a.n_pairs, PH_BLOCK, 0, (hipStream_t)stream>>>(a);
    ALIGNN_CHECK_LAUNCH();
    return 0;
}

extern "C" int alignn_phsym_solve(const alignn_phsym_fc_args* args, void* stream) {
    if (!args || !fc_args_ok(*args)) return (int)hipErrorInvalidValue;
    const FcArgs& a = *args;
    if (a.n_items == 0) return 0;
    if (!fc_rows_ok(a) || !a.g_rows || !a.g || !a.n_site || !a.site_ops || !a.n_dir || !a.dirs || !a.minv)
        return (int)hipErrorInvalidValue;
    phsym_solve_kernel<<<dim3(alignn_ceil_div(a.max_supercell_atoms, PH_BLOCK), a.n_items), PH_BLOCK, 0, (hipStream_t)stream>>>(a);
    ALIGNN_CHECK_LAUNCH();
    return 0;
}

extern "C" int alignn_phsym_distribute(const alignn_phsym_fc_args* args, void* stream) {
    if (!args || !fc_args_ok(*args)) return (int)hipErrorInvalidValue;
    const FcArgs& a = *args;
    if (a.n_items == 0) return 0;
    if (!fc_rows_ok(a) || !a.rep || !a.dist_op) return (int)hipErrorInvalidValue;
    phsym_distribute_kernel<<<dim3(alignn_ceil_div(a.max_supercell_atoms, PH_BLOCK), a.n_items), PH_BLOCK, 0,
                              (hipStream_t)stream>>>(a);
    ALIGNN_CHECK_LAUNCH();
    return 0;
}
