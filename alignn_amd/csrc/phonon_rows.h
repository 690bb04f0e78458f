// What phonon.hip and phonon_sym.hip share: the block size of their launches, the supercell's image counts, and the rows of
// central differences of a -/+ pair of displaced supercells with the three drift corrections (tests/phonons_ref.py
// raw_force_constants restates them).  float64, every sum in a fixed order.
#pragma once
#include "common.h"

constexpr int PH_BLOCK = 256;
constexpr int PH_WAVES = PH_BLOCK / ALIGNN_WAVE;
enum { DRIFT_NONE = 0, DRIFT_FREDERIKSEN = 1, DRIFT_MEAN = 2 };

struct Cells {
    int n0, n1, n2;
    __device__ __forceinline__ int count() const { return n0 * n1 * n2; }
};
__device__ __forceinline__ Cells cells_of(const int32_t* dims, int s) { return {dims[3 * s], dims[3 * s + 1], dims[3 * s + 2]}; }

// out(j, k, (F-[j][k] - F+[j][k]) / (2 delta)) for the n_sc supercell atoms j of a pair whose displaced atom is supercell atom a,
// after ASE's Frederiksen correction (the supercell's force sum taken off atom a's row) or the mean drift (sum / n_sc off every
// row).  Every thread of the workgroup of PH_BLOCK threads must call it (it reduces over the workgroup).
template <class Out>
__device__ __forceinline__ void difference_rows(const double* __restrict__ Fm, const double* __restrict__ Fp, int n_sc, int a,
                                                int drift, double delta, double (*sh)[PH_WAVES], Out out) {
    double sum[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    if (drift != DRIFT_NONE) {
        for (int j = threadIdx.x; j < n_sc; j += PH_BLOCK) {
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                sum[k] += Fm[3 * j + k];
                sum[3 + k] += Fp[3 * j + k];
            }
        }
        block_reduce<6, false>(sum, sh);
        if (drift == DRIFT_MEAN) {
#pragma unroll
            for (int k = 0; k < 6; ++k) sum[k] /= (double)n_sc;
        }
    }
    const double two_delta = 2.0 * delta;
    for (int j = threadIdx.x; j < n_sc; j += PH_BLOCK) {
        const bool sub = drift == DRIFT_MEAN || (drift == DRIFT_FREDERIKSEN && j == a);
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            double fm = Fm[3 * j + k], fp = Fp[3 * j + k];
            if (sub) {
                fm -= sum[k];
                fp -= sum[3 + k];
            }
            out(j, k, (fm - fp) / two_delta);
        }
    }
}
