// What the builders of derived structures share (defects.hip, interface.hip, eos.hip): the inverse of a 3 x 3 cell by cofactors and
// the product of a row vector with a cell; for symmetry.hip and phonon_sym.hip, the Cartesian rotation of an operation; for
// trajectory.hip, order.hip and symmetry.hip, the determinant, the heights and the range of periodic images of a cell; and, for
// every kernel that takes a minimum image in Cartesian space (trajectory.hip, neb.hip, idpp.hip and, through neighbor_list.h,
// order.hip and local_order.hip), the wrapped difference and the shift to a periodic image.  float64 without contraction, every sum
// in a fixed order; tests/defects_ref.py restates the first two operation for operation (inv3_cof, row_dot), tests/traj_ref.py the
// image range, the wrap and the shift.
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

// det A along its first row, the association of inv3_cof
__device__ __forceinline__ double det3_cof(const double (&a)[9]) {
    const double c00 = a[4] * a[8] - a[5] * a[7], c01 = a[3] * a[8] - a[5] * a[6], c02 = a[3] * a[7] - a[4] * a[6];
    return (a[0] * c00 - a[1] * c01) + a[2] * c02;
}

// the height h_k = vol / |a_{k+1} x a_{k+2}| of a cell of volume vol = |det A|
__device__ __forceinline__ double height(const double (&A)[9], double vol, int k) {
    const double* u = A + 3 * ((k + 1) % 3);
    const double* v = A + 3 * ((k + 2) % 3);
    const double cx = u[1] * v[2] - u[2] * v[1], cy = u[2] * v[0] - u[0] * v[2], cz = u[0] * v[1] - u[1] * v[0];
    return vol / sqrt((cx * cx + cy * cy) + cz * cz);
}

__device__ __forceinline__ void heights(const double (&A)[9], double (&h)[3]) {
    const double vol = fabs(det3_cof(A));
#pragma unroll
    for (int k = 0; k < 3; ++k) h[k] = height(A, vol, k);
}

// the periodic images a sphere of radius r reaches: M_k = floor(r / h_k + 1/2) per axis; false when an axis needs more than
// max_range (or the cell is singular or not finite)
__device__ __forceinline__ bool image_range(const double (&C)[9], double r, int max_range, int (&M)[3]) {
    const double vol = fabs(det3_cof(C));
    bool ok = true;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const double q = floor(r / height(C, vol, k) + 0.5);
        if (!(q >= 0.0 && q <= (double)max_range)) {  // (a NaN fails both)
            ok = false;
            M[k] = 0;
        } else {
            M[k] = (int)q;
        }
    }
    return ok;
}

// x M for a row vector x and a row-major M: (x0 M0k + x1 M1k) + x2 M2k
__device__ __forceinline__ double row_dot(const double* x, const double (&m)[9], int k) {
    return (x[0] * m[k] + x[1] * m[3 + k]) + x[2] * m[6 + k];
}

// the plain wrap of the row difference d in the cell C with inverse Ci: f = d Ci, f - rint(f) (half to even), then that row x C
// (shift: the whole cells rint(f) that were taken off, for vanhove.hip, which has to know which image of an atom is the atom)
__device__ __forceinline__ void wrap_difference(const double (&d)[3], const double (&C)[9], const double (&Ci)[9],
                                                double (&d0)[3], double (&shift)[3]) {
    double f[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        f[c] = row_dot(d, Ci, c);
        shift[c] = rint(f[c]);
        f[c] -= shift[c];
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) d0[c] = row_dot(f, C, c);
}

__device__ __forceinline__ void wrap_difference(const double (&d)[3], const double (&C)[9], const double (&Ci)[9],
                                                double (&d0)[3]) {
    double shift[3];
    wrap_difference(d, C, Ci, d0, shift);
}

// component c of d0 moved to the periodic image (m0, m1, m2): d0[c] + ((m0 C[0][c] + m1 C[1][c]) + m2 C[2][c])
__device__ __forceinline__ double image_offset(const double (&d0)[3], int m0, int m1, int m2, const double (&C)[9], int c) {
    return d0[c] + (((double)m0 * C[c] + (double)m1 * C[3 + c]) + (double)m2 * C[6 + c]);
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
