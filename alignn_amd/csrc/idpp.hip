// Device side of the IDPP band initialisation (alignn_amd/idpp.py): the image dependent pair potential of ASE 3.22's ase/neb.py
// (class IDPP) for the interior images of a batch of bands, with the plain-wrap minimum image convention of neb.hip.  The
// reference has no NEB; tests/idpp_ref.py is the numpy restatement, include/alignn_idpp.h states the formulas and every field of
// the argument block.
//
//   idpp_pair_kernel     one wavefront per (active band, interior image m, atom a), four of them to a workgroup: the lanes stride
//                        over b, each pair's three wrapped distances (in image m, image 0 and image M - 1) recomputed from the
//                        rows, then a butterfly sum over the lanes gives F_a and the row's share e_a of E_m;
//   idpp_energy_kernel   one workgroup per (active band, interior image): E_m = sum_a e_a by one block_reduce.
// float64, no contraction, no atomics, every sum in a fixed order that depends on the image's own rows only: a band's bits are the
// same alone, in a batch and at any place of the batch.
#include "../../include/alignn_idpp.h"
#include "../../include/alignn_neb.h"
#include "common.h"
#include "cell3.h"

#pragma clang fp contract(off)

namespace {

constexpr int IDPP_BLOCK = 256, IDPP_WAVES = IDPP_BLOCK / ALIGNN_WAVE;

using IdppArgs = alignn_idpp_args;

// the active band k: its index, shape and first rows; false when its row counts do not fit (uniform over a launch's workgroups)
struct Band {
    int s, M, n, rbeg, ebeg, fbeg, gbeg;
};
__device__ __forceinline__ bool band_fits(const IdppArgs& a, int k, Band& g) {
    g.s = a.active[k];
    g.rbeg = a.row_ptr[g.s];
    g.ebeg = a.end_ptr[g.s];
    g.n = a.end_ptr[g.s + 1] - g.ebeg;
    g.fbeg = a.force_ptr[k];
    g.gbeg = a.energy_ptr[k];
    const int rows = a.row_ptr[g.s + 1] - g.rbeg;
    if (g.n < 1 || g.n > a.max_atoms || rows < g.n || rows % g.n != 0) return false;
    g.M = rows / g.n + 2;
    return g.M <= a.max_images && a.force_ptr[k + 1] - g.fbeg == rows && a.energy_ptr[k + 1] - g.gbeg == g.M - 2;
}

// |mic(x - y)| in the cell C with inverse Ci (cell3.h's wrap_difference, as in neb.hip), the wrapped difference in D
__device__ __forceinline__ double wrapped(const double (&x)[3], const double* y, const double (&C)[9], const double (&Ci)[9],
                                          double (&D)[3]) {
    const double d[3] = {x[0] - y[0], x[1] - y[1], x[2] - y[2]};
    wrap_difference(d, C, Ci, D);
    return sqrt((D[0] * D[0] + D[1] * D[1]) + D[2] * D[2]);
}

__global__ __launch_bounds__(IDPP_BLOCK) void idpp_pair_kernel(const IdppArgs a) {
    const int k = blockIdx.z, m = blockIdx.y + 1;  // interior image m = 1 .. M - 2
    Band g;
    const bool fits = band_fits(a, k, g);
    if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) a.status[k] = fits ? 0 : -1;
    if (!fits || m > g.M - 2) return;
    const int lane = threadIdx.x & (ALIGNN_WAVE - 1), row = blockIdx.x * IDPP_WAVES + threadIdx.x / ALIGNN_WAVE;
    if (row >= g.n) return;  // (the whole wavefront)

    double C[9], Ci[9];
    load9(a.lattice + 9 * (int64_t)g.s, C);
    load9(a.inv_lattice + 9 * (int64_t)g.s, Ci);
    const int64_t image = (int64_t)(m - 1) * g.n;
    const double* R = a.positions + 3 * ((int64_t)g.rbeg + image);
    const double* R1 = a.initial + 3 * (int64_t)g.ebeg;
    const double* R2 = a.final + 3 * (int64_t)g.ebeg;
    double x[3], x1[3], x2[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        x[j] = R[3 * row + j];
        x1[j] = R1[3 * row + j];
        x2[j] = R2[3 * row + j];
    }
    const double w = (double)m, images = (double)(g.M - 1);

    double F[3] = {0.0, 0.0, 0.0}, e = 0.0;
    for (int b = lane; b < g.n; b += ALIGNN_WAVE) {
        if (b == row) continue;
        double D[3], D1[3], D2[3];
        const double d = wrapped(x, R + 3 * b, C, Ci, D);
        const double d1 = wrapped(x1, R1 + 3 * b, C, Ci, D1);
        const double d2 = wrapped(x2, R2 + 3 * b, C, Ci, D2);
        const double delta = d - (d1 + w * ((d2 - d1) / images));
        const double dd = d * d, d4 = dd * dd;
        e = e + (delta * delta) / d4;
        const double c = (delta * (1.0 - (2.0 * delta) / d)) / (d4 * d);
#pragma unroll
        for (int j = 0; j < 3; ++j) F[j] = F[j] + c * D[j];
    }
#pragma unroll
    for (int j = 0; j < 3; ++j) F[j] = wave_sum(F[j]);
    e = wave_sum(e);
    if (lane == 0) {
        const int64_t out = (int64_t)g.fbeg + image + row;
#pragma unroll
        for (int j = 0; j < 3; ++j) a.forces[3 * out + j] = -2.0 * F[j];
        a.row_energy[out] = 0.5 * e;
    }
}

__global__ __launch_bounds__(IDPP_BLOCK) void idpp_energy_kernel(const IdppArgs a) {
    __shared__ double sh[1][IDPP_WAVES];
    const int k = blockIdx.y, m = blockIdx.x + 1;
    Band g;
    if (!band_fits(a, k, g) || m > g.M - 2) return;  // (uniform over the workgroup)
    const double* e = a.row_energy + (int64_t)g.fbeg + (int64_t)(m - 1) * g.n;
    double v[1] = {0.0};
    for (int r = threadIdx.x; r < g.n; r += IDPP_BLOCK) v[0] = v[0] + e[r];
    block_reduce<1, false>(v, sh);
    if (threadIdx.x == 0) a.energy[g.gbeg + m - 1] = v[0];
}

}  // namespace

extern "C" size_t alignn_idpp_args_size(void) { return sizeof(alignn_idpp_args); }

extern "C" int alignn_idpp_forces(const alignn_idpp_args* args, void* stream) {
    if (!args) return (int)hipErrorInvalidValue;
    const IdppArgs& a = *args;
    if (a.n_active < 0 || a.n_active > 65535 || a.max_images < 3 || a.max_images > ALIGNN_NEB_MAX_IMAGES || a.max_atoms < 1)
        return (int)hipErrorInvalidValue;
    if (!a.force_ptr || !a.energy_ptr || !a.active || !a.row_ptr || !a.end_ptr || !a.lattice || !a.inv_lattice || !a.initial ||
        !a.final || !a.positions || !a.forces || !a.energy || !a.row_energy || !a.status)
        return (int)hipErrorInvalidValue;
    if (a.n_active == 0) return 0;
    const int images = a.max_images - 2;
    idpp_pair_kernel<<<dim3(alignn_ceil_div(a.max_atoms, IDPP_WAVES), images, a.n_active), IDPP_BLOCK, 0, (hipStream_t)stream>>>(a);
    ALIGNN_CHECK_LAUNCH();
    idpp_energy_kernel<<<dim3(images, a.n_active), IDPP_BLOCK, 0, (hipStream_t)stream>>>(a);
    ALIGNN_CHECK_LAUNCH();
    return 0;
}
