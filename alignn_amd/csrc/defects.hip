// Device builders of the derived structures of the defect tasks (alignn_amd/defects.py): the supercells of vacancy_formation
// (pristine, or with one atom removed) and the slabs of surface_energy, written in the arrays ``relax`` takes.  The reference
// builds them on the host one at a time (jarvis-tools' Vacancy.generate_defects and Surface.make_surface, the latter a port of
// ASE's ase/build/general_surface.py; alignn/ff/ff.py:808-981).  tests/defects_ref.py is the numpy restatement this file
// follows operation for operation.
//
//   defect_supercell_kernel   one workgroup per job (structure, removed supercell atom or -1);
//   slab_build_kernel         one workgroup per job (structure, unimodular integer basis, layers, vacuum).
// float64, no contraction, every sum written in a fixed order and no atomics: a job's bits do not depend on what else shares
// the launch.  A job whose structure index, removed atom, layer count or row range does not fit writes nothing.
#include "../../include/alignn_hip.h"
#include "common.h"
#include "cell3.h"

#pragma clang fp contract(off)

namespace {

constexpr int DF_BLOCK = 256;
constexpr double DF_TOL = 1e-10;  // general_surface's tolerance of the wrap: s -= floor(s + tol)

// Supercell atom j = image * n + b, image = (m0 N1 + m1) N2 + m2, cart = ((r_b + m0 L0) + m1 L1) + m2 L2 (the order of
// phonon_displace_kernel).  With a removed atom a >= 0 the rows after a move up by one.
__global__ __launch_bounds__(DF_BLOCK) void defect_supercell_kernel(
    const double* __restrict__ pos, const int32_t* __restrict__ atom_ptr, const double* __restrict__ lattice,
    const int32_t* __restrict__ dims, int n_structures, const int32_t* __restrict__ jobs, const int64_t* __restrict__ row_off,
    double* __restrict__ cells, double* __restrict__ cart, double* __restrict__ frac, int32_t* __restrict__ src) {
    const int job = blockIdx.x;
    const int s = jobs[2 * job], a = jobs[2 * job + 1];
    if (s < 0 || s >= n_structures) return;
    const int beg = atom_ptr[s], n = atom_ptr[s + 1] - beg;
    const int n0 = dims[3 * s], n1 = dims[3 * s + 1], n2 = dims[3 * s + 2];
    if (n < 1 || n0 < 1 || n1 < 1 || n2 < 1) return;
    const int64_t n_sc64 = (int64_t)n * n0 * n1 * n2;
    const int64_t row0 = row_off[job];
    if (n_sc64 > INT32_MAX || a < -1 || a >= n_sc64 || row_off[job + 1] - row0 != n_sc64 - (a >= 0 ? 1 : 0)) return;
    const int n_sc = (int)n_sc64;
    const double* L = lattice + 9 * (int64_t)s;
    const double nd[3] = {(double)n0, (double)n1, (double)n2};
    double S[9], Sinv[9];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int k = 0; k < 3; ++k) S[3 * i + k] = nd[i] * L[3 * i + k];
    inv3_cof(S, Sinv);
    if (threadIdx.x < 9) cells[9 * (int64_t)job + threadIdx.x] = S[threadIdx.x];
    for (int j = threadIdx.x; j < n_sc; j += DF_BLOCK) {
        if (j == a) continue;
        const int img = j / n, b = j - img * n;
        const double m2 = (double)(img % n2), m1 = (double)((img / n2) % n1), m0 = (double)(img / (n1 * n2));
        double r[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            r[k] = pos[3 * ((int64_t)beg + b) + k] + m0 * L[k];
            r[k] = r[k] + m1 * L[3 + k];
            r[k] = r[k] + m2 * L[6 + k];
        }
        const int64_t row = row0 + (a >= 0 && j > a ? j - 1 : j);
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            cart[3 * row + k] = r[k];
            frac[3 * row + k] = wrap01(row_dot(r, Sinv, k));
        }
        src[row] = beg + b;
    }
}

// jobs[job] = (s, c1 [3], c2 [3], c3 [3], layers); the steps are those of the header (general_surface's build()).
constexpr int SLAB_JOB = 11;
__global__ __launch_bounds__(DF_BLOCK) void slab_build_kernel(
    const double* __restrict__ pos, const int32_t* __restrict__ atom_ptr, const double* __restrict__ lattice, int n_structures,
    const int32_t* __restrict__ jobs, const double* __restrict__ vacuum, const int64_t* __restrict__ row_off,
    double* __restrict__ cells, double* __restrict__ cart, double* __restrict__ frac, int32_t* __restrict__ src) {
    const int job = blockIdx.x;
    const int32_t* J = jobs + SLAB_JOB * (int64_t)job;
    const int s = J[0], layers = J[10];
    if (s < 0 || s >= n_structures || layers < 1) return;
    const int beg = atom_ptr[s], n = atom_ptr[s + 1] - beg;
    const int64_t row0 = row_off[job];
    if (n < 1 || (int64_t)n * layers > INT32_MAX || row_off[job + 1] - row0 != (int64_t)n * layers) return;
    // the integer inverse of the unimodular basis: adjugate * det (det = +-1), in 64-bit integers
    int64_t Bm[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) Bm[i] = J[1 + i];
    int64_t adj[9];
    adj[0] = Bm[4] * Bm[8] - Bm[5] * Bm[7];
    adj[1] = Bm[2] * Bm[7] - Bm[1] * Bm[8];
    adj[2] = Bm[1] * Bm[5] - Bm[2] * Bm[4];
    adj[3] = Bm[5] * Bm[6] - Bm[3] * Bm[8];
    adj[4] = Bm[0] * Bm[8] - Bm[2] * Bm[6];
    adj[5] = Bm[2] * Bm[3] - Bm[0] * Bm[5];
    adj[6] = Bm[3] * Bm[7] - Bm[4] * Bm[6];
    adj[7] = Bm[1] * Bm[6] - Bm[0] * Bm[7];
    adj[8] = Bm[0] * Bm[4] - Bm[1] * Bm[3];
    const int64_t det = Bm[0] * adj[0] + Bm[1] * adj[3] + Bm[2] * adj[6];
    if (det != 1 && det != -1) return;
    const double* Lp = lattice + 9 * (int64_t)s;
    double L[9], Linv[9], Binv[9], C[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) {
        L[i] = Lp[i];
        Binv[i] = (double)(adj[i] * det);
    }
    inv3_cof(L, Linv);
    // 1. the oriented cell C = Bm L
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int k = 0; k < 3; ++k)
            C[3 * i + k] = ((double)Bm[3 * i] * L[k] + (double)Bm[3 * i + 1] * L[3 + k]) + (double)Bm[3 * i + 2] * L[6 + k];
    // 5., 6. the cell [C0, C1, a3], a3 along nu = C0 x C1
    const double nu[3] = {C[1] * C[5] - C[2] * C[4], C[2] * C[3] - C[0] * C[5], C[0] * C[4] - C[1] * C[3]};
    const double ld = (double)layers;
    const double t[3] = {ld * C[6], ld * C[7], ld * C[8]};
    const double q = ((t[0] * nu[0] + t[1] * nu[1]) + t[2] * nu[2]) / ((nu[0] * nu[0] + nu[1] * nu[1]) + nu[2] * nu[2]);
    double S[9], Sinv[9], Finv[9];
#pragma unroll
    for (int k = 0; k < 6; ++k) S[k] = C[k];
#pragma unroll
    for (int k = 0; k < 3; ++k) S[6 + k] = nu[k] * q;
    inv3_cof(S, Sinv);
    // 8. the vacuum on the third vector
    const double len = sqrt((S[6] * S[6] + S[7] * S[7]) + S[8] * S[8]);
    const double vac = vacuum[job];
    double Fc[9];
#pragma unroll
    for (int k = 0; k < 6; ++k) Fc[k] = S[k];
#pragma unroll
    for (int k = 0; k < 3; ++k) Fc[6 + k] = S[6 + k] + vac * (S[6 + k] / len);
    inv3_cof(Fc, Finv);
    if (threadIdx.x < 9) cells[9 * (int64_t)job + threadIdx.x] = Fc[threadIdx.x];
    const int rows = n * layers;
    for (int j = threadIdx.x; j < rows; j += DF_BLOCK) {
        const int m = j / n, b = j - m * n;
        double r[3], f[3], o[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) r[k] = pos[3 * ((int64_t)beg + b) + k];
        // 2., 3. the parent's fractions, then the oriented ones, wrapped
#pragma unroll
        for (int k = 0; k < 3; ++k) f[k] = row_dot(r, Linv, k);
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            o[k] = row_dot(f, Binv, k);
            o[k] = o[k] - floor(o[k] + DF_TOL);
        }
        // 4. layer m
        const double o2 = o[2] + (double)m;
#pragma unroll
        for (int k = 0; k < 3; ++k) r[k] = (o[0] * C[k] + o[1] * C[3 + k]) + o2 * C[6 + k];
        // 7. wrapped into [C0, C1, a3]
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            f[k] = row_dot(r, Sinv, k);
            f[k] = f[k] - floor(f[k] + DF_TOL);
        }
#pragma unroll
        for (int k = 0; k < 3; ++k) r[k] = row_dot(f, S, k);
        // 9., 10. the positions stay, their fractions in the final cell
        const int64_t row = row0 + j;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            cart[3 * row + k] = r[k];
            frac[3 * row + k] = wrap01(row_dot(r, Finv, k));
        }
        src[row] = beg + b;
    }
}

}  // namespace

extern "C" int alignn_defect_supercells(const double* positions, const int32_t* atom_ptr, const double* lattice,
                                        const int32_t* supercell, int n_structures, const int32_t* jobs, const int64_t* row_off,
                                        int n_jobs, double* cells, double* cart, double* frac, int32_t* src,
                                        alignn_stream_t stream) {
    if (n_jobs < 0 || n_structures < 1 || !positions || !atom_ptr || !lattice || !supercell || !jobs || !row_off || !cells ||
        !cart || !frac || !src)
        return (int)hipErrorInvalidValue;
    if (n_jobs == 0) return 0;
    defect_supercell_kernel<<<n_jobs, DF_BLOCK, 0, (hipStream_t)stream>>>(positions, atom_ptr, lattice, supercell, n_structures,
                                                                           jobs, row_off, cells, cart, frac, src);
    ALIGNN_CHECK_LAUNCH();
    return 0;
}

extern "C" int alignn_slab_build(const double* positions, const int32_t* atom_ptr, const double* lattice, int n_structures,
                                 const int32_t* jobs, const double* vacuum, const int64_t* row_off, int n_jobs, double* cells,
                                 double* cart, double* frac, int32_t* src, alignn_stream_t stream) {
    if (n_jobs < 0 || n_structures < 1 || !positions || !atom_ptr || !lattice || !jobs || !vacuum || !row_off || !cells || !cart ||
        !frac || !src)
        return (int)hipErrorInvalidValue;
    if (n_jobs == 0) return 0;
    slab_build_kernel<<<n_jobs, DF_BLOCK, 0, (hipStream_t)stream>>>(positions, atom_ptr, lattice, n_structures, jobs, vacuum,
                                                                     row_off, cells, cart, frac, src);
    ALIGNN_CHECK_LAUNCH();
    return 0;
}
