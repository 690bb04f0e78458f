// What the per-wavefront least-squares fits share (eos.hip, elastic.hip) beside the wave sums of common.h (xor butterfly: every
// lane ends with the same bits): the Cholesky solve of the small normal equations, held in registers by every
// lane.  float64 without contraction, every sum in a fixed order; tests/eos_ref.py restates both operation for operation.
#pragma once
#include "common.h"

#pragma clang fp contract(off)

// A = L L^T for a symmetric positive definite A: the lower triangle row by row, every inner sum in ascending index order; false
// where a pivot is not > 0 or not finite
template <int N>
__device__ __forceinline__ bool cholesky_factor(const double (&A)[N][N], double (&L)[N][N]) {
#pragma unroll
    for (int i = 0; i < N; ++i)
#pragma unroll
        for (int j = 0; j <= i; ++j) {
            double s = A[i][j];
#pragma unroll
            for (int k = 0; k < j; ++k) s = s - L[i][k] * L[j][k];
            if (i == j) {
                if (!(s > 0.0 && s < INFINITY)) return false;
                L[i][i] = sqrt(s);
            } else {
                L[i][j] = s / L[j][j];
            }
        }
    return true;
}

// L L^T x = b: forward, then backward substitution
template <int N>
__device__ __forceinline__ void cholesky_substitute(const double (&L)[N][N], const double (&b)[N], double (&x)[N]) {
    double y[N];
#pragma unroll
    for (int i = 0; i < N; ++i) {
        double s = b[i];
#pragma unroll
        for (int k = 0; k < i; ++k) s = s - L[i][k] * y[k];
        y[i] = s / L[i][i];
    }
#pragma unroll
    for (int i = N - 1; i >= 0; --i) {
        double s = y[i];
#pragma unroll
        for (int k = i + 1; k < N; ++k) s = s - L[k][i] * x[k];
        x[i] = s / L[i][i];
    }
}

// A x = b for a symmetric positive definite A by Cholesky; false where a pivot is not > 0 or not finite
template <int N>
__device__ __forceinline__ bool cholesky_solve(const double (&A)[N][N], const double (&b)[N], double (&x)[N]) {
    double L[N][N];
    if (!cholesky_factor<N>(A, L)) return false;
    cholesky_substitute<N>(L, b, x);
    return true;
}
