// What the builders of derived structures share (defects.hip, interface.hip, eos.hip): the inverse of a 3 x 3 cell by cofactors and
// the product of a row vector with a cell.  float64 without contraction, every sum in a fixed order; tests/defects_ref.py restates
// both operation for operation (inv3_cof, row_dot).
#pragma once

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
