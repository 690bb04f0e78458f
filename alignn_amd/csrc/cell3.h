// What the builders of derived structures share (defects.hip, interface.hip, eos.hip): the inverse of a 3 x 3 cell by cofactors and
// the product of a row vector with a cell; and, for symmetry.hip and phonon_sym.hip, the Cartesian rotation of an operation.  float64 without contraction, every sum in a fixed order; tests/defects_ref.py restates
// both operation for operation (inv3_cof, row_dot).
#pragma once
#include <stdint.h>

#pragma clang fp contract(off)

// inverse of a row-major 3 x 3 by cofactors, every element its cofactor / det (common.h's inverse3, here without contraction)
__device__ __forceinline__ void inv3_cof(const double (&a)[9], double (&inv)[9]) {
    const double c00 = a[4] * a[8] - a[5] * a[7], c01 = a[3] * a[8] - a[5] * a[6], c02 = a[3] * a[7] - a[4] * a[6];
    const double det = (a[0] * c00 - a[1] * c01) + a[2] * c02;
    inv[0] = c00 / det;
    inv[1] = (a[2] * a[7] - a[1] * a[8]) / det;
    inv[2] = (a[1] * a[5] - a[2] * a[4]) / det;
    inv[3] = -c01 / det;
    inv[4] = (a[0] * a[8] - a[2] * a[6]) / det;
    inv[5] = (a[2] * a[3] - a[0] * a[5]) / det;
    inv[6] = c02 / det;
    inv[7] = (a[1] * a[6] - a[0] * a[7]) / det;
    inv[8] = (a[0] * a[4] - a[1] * a[3]) / det;
}

// x M for a row vector x and a row-major M: (x0 M0k + x1 M1k) + x2 M2k
__device__ __forceinline__ double row_dot(const double* x, const double (&m)[9], int k) {
    return (x[0] * m[k] + x[1] * m[3 + k]) + x[2] * m[6 + k];
}

__device__ __forceinline__ void load9(const double* p, double (&A)[9]) {
#pragma unroll
    for (int j = 0; j < 9; ++j) A[j] = p[j];
}

// Q = A^T W A^-T: M = A^T W, then M A^-T
__device__ __forceinline__ void cartesian_rotation(const double (&A)[9], const double (&Ai)[9], const int32_t* Wg, double (&Q)[9]) {
    double W[9], M[9];
#pragma unroll
    for (int j = 0; j < 9; ++j) W[j] = (double)Wg[j];
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) M[3 * r + c] = (A[r] * W[c] + A[3 + r] * W[3 + c]) + A[6 + r] * W[6 + c];
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int d = 0; d < 3; ++d) Q[3 * r + d] = (M[3 * r] * Ai[3 * d] + M[3 * r + 1] * Ai[3 * d + 1]) + M[3 * r + 2] * Ai[3 * d + 2];
}
