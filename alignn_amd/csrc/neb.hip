// Device side of the nudged elastic band (alignn_amd/neb.py): the interpolation of a band between its endpoints and the NEB
// forces of ASE 3.22's ase/neb.py (method "aseneb" and "improvedtangent", with or without the climbing image) for a batch of
// bands.  The reference has no NEB; tests/neb_ref.py is the numpy restatement, include/alignn_neb.h states the formulas and
// every field of the argument block.
//
//   neb_interpolate_kernel   one thread per interior row, grid-strided: initial + j * (mic(final - initial) / (M - 1));
//   neb_forces_kernel        one workgroup per (active band, interior image): the five sums |t1|^2, |t2|^2, t1.t2, f.t1, f.t2 over
//                            the image's rows by one block_reduce, the tangent tau = a t1 + b t2 and the projection's scalars
//                            from them (every thread alike), then a second pass over the rows that recomputes t1, t2 and
//                            writes F.
// float64, no contraction, no atomics, every sum in a fixed order that depends on the image's own rows only: a band's bits are the
// same alone, in a batch and at any place of the batch.  The minimum image convention is the plain wrap of the fractional
// difference (cell3.h's wrap_difference; rint: half to even), not a Minkowski-reduced search.
#include "../../include/alignn_neb.h"
#include "common.h"
#include "cell3.h"

#pragma clang fp contract(off)

namespace {

constexpr int NEB_BLOCK = 256, NEB_WAVES = NEB_BLOCK / ALIGNN_WAVE;
constexpr int NEB_INTERP_BLOCK = 256, NEB_INTERP_MAX_BLOCKS = 4096;

// the band of output row r: the last b with row_ptr[b] <= r (empty bands are stepped over)
__device__ __forceinline__ int band_of(const int32_t* __restrict__ row_ptr, int n_bands, int64_t r) {
    int lo = 0, hi = n_bands;  // row_ptr[lo] <= r < row_ptr[hi]
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (row_ptr[mid] <= r)
            lo = mid;
        else
            hi = mid;
    }
    return lo;
}

__global__ __launch_bounds__(NEB_INTERP_BLOCK) void neb_interpolate_kernel(
    const double* __restrict__ initial, const double* __restrict__ final, const int32_t* __restrict__ end_ptr,
    const double* __restrict__ lattice, const int32_t* __restrict__ row_ptr, int n_bands, int64_t n_rows,
    double* __restrict__ positions, double* __restrict__ inv_lattice) {
    const int64_t t0 = (int64_t)blockIdx.x * NEB_INTERP_BLOCK + threadIdx.x, stride = (int64_t)gridDim.x * NEB_INTERP_BLOCK;
    if (inv_lattice) {
        for (int64_t b = t0; b < n_bands; b += stride) {
            double C[9], Ci[9];
#pragma unroll
            for (int j = 0; j < 9; ++j) C[j] = lattice[9 * b + j];
            inv3_cof(C, Ci);
#pragma unroll
            for (int j = 0; j < 9; ++j) inv_lattice[9 * b + j] = Ci[j];
        }
    }
    for (int64_t r = t0; r < n_rows; r += stride) {
        const int b = band_of(row_ptr, n_bands, r);
        const int e0 = end_ptr[b], n = end_ptr[b + 1] - e0;
        const int64_t local = r - row_ptr[b], rows = (int64_t)row_ptr[b + 1] - row_ptr[b];
        if (n < 1 || rows % n != 0) continue;  // (the host checks this; nothing is read out of a band's range)
        const int64_t img = local / n, atom = local - img * n;  // interior image 1 + img
        const double images = (double)(rows / n + 1);            // M - 1
        double C[9], Ci[9], d[3], x0[3], step[3];
#pragma unroll
        for (int j = 0; j < 9; ++j) C[j] = lattice[9 * (int64_t)b + j];
        inv3_cof(C, Ci);
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            x0[j] = initial[3 * (e0 + atom) + j];
            d[j] = final[3 * (e0 + atom) + j] - x0[j];
        }
        wrap_difference(d, C, Ci, step);
        const double jd = (double)(img + 1);
#pragma unroll
        for (int j = 0; j < 3; ++j) positions[3 * r + j] = x0[j] + jd * (step[j] / images);
    }
}

using NebArgs = alignn_neb_args;

__global__ __launch_bounds__(NEB_BLOCK) void neb_forces_kernel(const NebArgs a) {
    __shared__ double sh[5][NEB_WAVES];
    __shared__ double Esh[ALIGNN_NEB_MAX_IMAGES];
    const int k = blockIdx.y, i = blockIdx.x + 1;  // interior image i = 1 .. M - 2
    const int s = a.active[k];
    const int M = a.image_ptr[s + 1] - a.image_ptr[s];
    const int rbeg = a.row_ptr[s], rows = a.row_ptr[s + 1] - rbeg;
    const int ebeg = a.end_ptr[s], n = a.end_ptr[s + 1] - ebeg;
    const int fbeg = a.force_ptr[k], gbeg = a.energy_ptr[k];
    // rows of another shape than the band: touch nothing (uniform over the workgroup, and the same in all of a band's workgroups)
    if (M < 3 || M > a.max_images || n < 1 || (int64_t)(M - 2) * n != rows || a.force_ptr[k + 1] - fbeg != rows ||
        a.energy_ptr[k + 1] - gbeg != M - 2) {
        if (blockIdx.x == 0 && threadIdx.x == 0) a.imax[k] = -1;
        return;
    }
    if (i > M - 2) return;

    // the band's energies, and the interior image of largest energy (the lowest index on ties)
    for (int m = threadIdx.x; m < M; m += NEB_BLOCK)
        Esh[m] = m == 0 ? a.end_energy[2 * s] : m == M - 1 ? a.end_energy[2 * s + 1] : a.energy[gbeg + m - 1];
    __syncthreads();
    int imax = 1;
    for (int m = 2; m <= M - 2; ++m)
        if (Esh[m] > Esh[imax]) imax = m;
    const double Em = Esh[i - 1], E0 = Esh[i], Ep = Esh[i + 1];
    if (threadIdx.x == 0) {
        a.energies_out[a.image_ptr[s] + i] = E0;
        if (i == 1) {
            a.energies_out[a.image_ptr[s]] = Esh[0];
            a.imax[k] = imax;
            a.emax[k] = Esh[imax];
        }
        if (i == M - 2) a.energies_out[a.image_ptr[s] + M - 1] = Esh[M - 1];
    }

    double C[9], Ci[9];
#pragma unroll
    for (int j = 0; j < 9; ++j) {
        C[j] = a.lattice[9 * (int64_t)s + j];
        Ci[j] = a.inv_lattice[9 * (int64_t)s + j];
    }
    const double* Rm = i == 1 ? a.initial + 3 * (int64_t)ebeg : a.positions + 3 * ((int64_t)rbeg + (int64_t)(i - 2) * n);
    const double* R0 = a.positions + 3 * ((int64_t)rbeg + (int64_t)(i - 1) * n);
    const double* Rp = i == M - 2 ? a.final + 3 * (int64_t)ebeg : a.positions + 3 * ((int64_t)rbeg + (int64_t)i * n);
    const double* Fo = a.forces + 3 * ((int64_t)fbeg + (int64_t)(i - 1) * n);
    double* FOUT = a.forces_out + 3 * ((int64_t)fbeg + (int64_t)(i - 1) * n);
    const uint8_t* FIX = a.fixed ? a.fixed + rbeg + (int64_t)(i - 1) * n : nullptr;

    // t1, t2 and the raw force (zero where the atom is fixed) of row r
    auto row = [&](int r, double (&t1)[3], double (&t2)[3], double (&f)[3]) {
        double d1[3], d2[3];
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const double x = R0[3 * r + j];
            d1[j] = x - Rm[3 * r + j];
            d2[j] = Rp[3 * r + j] - x;
            f[j] = Fo[3 * r + j];
        }
        wrap_difference(d1, C, Ci, t1);
        wrap_difference(d2, C, Ci, t2);
        if (FIX && FIX[r]) f[0] = f[1] = f[2] = 0.0;
    };

    double v[5] = {0.0, 0.0, 0.0, 0.0, 0.0};  // |t1|^2, |t2|^2, t1.t2, f.t1, f.t2
    for (int r = threadIdx.x; r < n; r += NEB_BLOCK) {
        double t1[3], t2[3], f[3];
        row(r, t1, t2, f);
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            v[0] = v[0] + t1[j] * t1[j];
            v[1] = v[1] + t2[j] * t2[j];
            v[2] = v[2] + t1[j] * t2[j];
            v[3] = v[3] + f[j] * t1[j];
            v[4] = v[4] + f[j] * t2[j];
        }
    }
    block_reduce<5, false>(v, sh);
    const double s11 = v[0], s22 = v[1], s12 = v[2], f1 = v[3], f2 = v[4];
    const double ks = a.spring[s];
    const bool climbing = a.climb && i == imax;

    // tau = ta t1 + tb t2 (then / norm), F = f - cf tau
    double ta, tb, norm = 1.0, cf;
    if (a.method == 0) {
        ta = i < imax ? 0.0 : 1.0;
        tb = i > imax ? 0.0 : 1.0;
        const double tt = (ta * ta) * s11 + 2.0 * (ta * tb) * s12 + (tb * tb) * s22;
        const double ft = ta * f1 + tb * f2;
        // (k t1 - k t2).tau
        const double spr = ks * (ta * s11 + tb * s12) - ks * (ta * s12 + tb * s22);
        cf = climbing ? 2.0 * ft / tt : ft / tt + spr / tt;
    } else {
        if (Ep > E0 && E0 > Em) {
            ta = 0.0, tb = 1.0;
        } else if (Ep < E0 && E0 < Em) {
            ta = 1.0, tb = 0.0;
        } else {
            const double dp = fabs(Ep - E0), dm = fabs(Em - E0);
            const double dmax = fmax(dp, dm), dmin = fmin(dp, dm);
            if (Ep > Em)
                ta = dmin, tb = dmax;
            else
                ta = dmax, tb = dmin;
        }
        norm = sqrt((ta * ta) * s11 + 2.0 * (ta * tb) * s12 + (tb * tb) * s22);
        const double ft = (ta * f1 + tb * f2) / norm;
        cf = climbing ? 2.0 * ft : ft - (ks * sqrt(s22) - ks * sqrt(s11));
    }
    for (int r = threadIdx.x; r < n; r += NEB_BLOCK) {
        double t1[3], t2[3], f[3];
        row(r, t1, t2, f);
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const double tau = (ta * t1[j] + tb * t2[j]) / norm;
            FOUT[3 * r + j] = f[j] - cf * tau;
        }
    }
}

}  // namespace

extern "C" size_t alignn_neb_args_size(void) { return sizeof(alignn_neb_args); }

extern "C" int alignn_neb_interpolate(const double* initial, const double* final, const int32_t* end_ptr, const double* lattice,
                                      const int32_t* row_ptr, int n_bands, int64_t n_rows, double* positions, double* inv_lattice,
                                      void* stream) {
    if (n_bands < 0 || n_rows < 0 || n_rows > 0x7fffffff) return (int)hipErrorInvalidValue;
    if (n_bands == 0) return n_rows == 0 ? 0 : (int)hipErrorInvalidValue;
    if (!initial || !final || !end_ptr || !lattice || !row_ptr || (n_rows > 0 && !positions)) return (int)hipErrorInvalidValue;
    const int64_t work = n_rows > n_bands ? n_rows : n_bands;
    neb_interpolate_kernel<<<capped_blocks(work, NEB_INTERP_BLOCK, NEB_INTERP_MAX_BLOCKS), NEB_INTERP_BLOCK, 0,
                             (hipStream_t)stream>>>(initial, final, end_ptr, lattice, row_ptr, n_bands, n_rows, positions,
                                                    inv_lattice);
    ALIGNN_CHECK_LAUNCH();
    return 0;
}

extern "C" int alignn_neb_forces(const alignn_neb_args* args, void* stream) {
    if (!args) return (int)hipErrorInvalidValue;
    const NebArgs& a = *args;
    if (a.n_active < 0 || a.n_active > 65535 || a.max_images < 3 || a.max_images > ALIGNN_NEB_MAX_IMAGES || a.method < 0 ||
        a.method > 1 || a.climb < 0 || a.climb > 1)
        return (int)hipErrorInvalidValue;
    if (!a.forces || !a.energy || !a.force_ptr || !a.energy_ptr || !a.active || !a.row_ptr || !a.image_ptr || !a.end_ptr ||
        !a.lattice || !a.inv_lattice || !a.spring || !a.initial || !a.final || !a.end_energy || !a.positions || !a.forces_out ||
        !a.energies_out || !a.imax || !a.emax)
        return (int)hipErrorInvalidValue;
    if (a.n_active == 0) return 0;
    neb_forces_kernel<<<dim3(a.max_images - 2, a.n_active), NEB_BLOCK, 0, (hipStream_t)stream>>>(a);
    ALIGNN_CHECK_LAUNCH();
    return 0;
}
