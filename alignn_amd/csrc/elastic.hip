// Device side of the elastic-tensor task (alignn_amd/elastic.py): the least-squares fit of every crystal's stress-strain points,
// sigma_i(p) = sigma0_i + sum_j C_ij eps_j(p) in Voigt order (xx, yy, zz, yz, xz, xy; engineering shear), then the compliance and
// the Voigt-Reuss-Hill moduli.  The strained structures themselves are built by alignn_strain_build (eos.hip).
// tests/elastic_ref.py is the numpy restatement this file follows operation for operation.
//
//   elastic_fit_kernel   one wavefront per crystal, one lane per strained structure: the 7 x 7 normal matrix of the rows
//                        (1, eps / w) and its six right-hand sides by wave_sum, one Cholesky factorisation and six solves in every
//                        lane, the residuals per lane, the symmetrised tensor, its inverse by a 6 x 6 Cholesky, the moduli.
// float64, no contraction, no atomics, every sum in a fixed order (wave_fit.h), after which every lane holds the same bits, so the
// control flow is wave-uniform: a crystal's bits do not depend on what else shares the launch.
#include "../../include/alignn_hip.h"
#include "common.h"
#include "wave_fit.h"

#pragma clang fp contract(off)

namespace {

constexpr int EL_UNKNOWNS = 7;  // sigma0_i and C_i1 ... C_i6 of one stress component
constexpr int EL_MIN_POINTS = EL_UNKNOWNS, EL_MAX_POINTS = ALIGNN_WAVE;

__device__ __forceinline__ bool finite(double x) { return fabs(x) < INFINITY; }

// (a0 + a1) + a2
__device__ __forceinline__ double sum3(double a0, double a1, double a2) { return (a0 + a1) + a2; }

// One wavefront per crystal; lane p < P holds strained structure p, the other lanes add zeros.  The steps are those of
// tests/elastic_ref.py fit().  Compiled for gfx950 (hipcc -O3, --save-temps): 256 VGPRs and 26 AGPRs, scratch 0 bytes per lane,
// no spills: the unrolled 7 x 7 and 6 x 6 arrays stay in registers, one wave per SIMD.
__global__ __launch_bounds__(ALIGNN_WAVE) void elastic_fit_kernel(
    const double* __restrict__ strain, const double* __restrict__ stress, const int32_t* __restrict__ n_points, int ld,
    double* __restrict__ c_raw, double* __restrict__ c_sym, double* __restrict__ compliance, double* __restrict__ sigma0,
    double* __restrict__ moduli, double* __restrict__ rms_out, double* __restrict__ asym_out, int32_t* __restrict__ status_out) {
    constexpr int U = EL_UNKNOWNS;
    const int s = blockIdx.x, lane = threadIdx.x;
    const int P = n_points ? n_points[s] : ld;
    const bool fits = P >= EL_MIN_POINTS && P <= ld;  // (ld <= 64: the entry point)
    const bool live = fits && lane < P;
    const double nan = NAN;
    double C[6][6], Cs[6][6], S[6][6], s0[6], mod[9], rms = nan, asym = nan;
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        s0[i] = nan;
#pragma unroll
        for (int j = 0; j < 6; ++j) C[i][j] = Cs[i][j] = S[i][j] = nan;
    }
#pragma unroll
    for (int i = 0; i < 9; ++i) mod[i] = nan;
    int status = 2;

    // 1. the lane's point and the column scale w = max |eps| over the live points
    double e[6], t[6];
    bool bad = false;
    {
        double g[9];
        const int64_t row = (int64_t)s * ld + lane;
#pragma unroll
        for (int j = 0; j < 6; ++j) {
            e[j] = live ? strain[6 * row + j] : 0.0;
            bad = bad || !finite(e[j]);
        }
#pragma unroll
        for (int j = 0; j < 9; ++j) {
            g[j] = live ? stress[9 * row + j] : 0.0;
            bad = bad || !finite(g[j]);
        }
        t[0] = g[0], t[1] = g[4], t[2] = g[8];
        t[3] = (g[5] + g[7]) * 0.5, t[4] = (g[2] + g[6]) * 0.5, t[5] = (g[1] + g[3]) * 0.5;
    }
    double m = fabs(e[0]);
#pragma unroll
    for (int j = 1; j < 6; ++j) m = fmax(m, fabs(e[j]));
    const double w = wave_max(live ? m : 0.0);
    const bool any_bad = wave_max(bad ? 1.0 : 0.0) > 0.0;
    bool fitted = false;
    double q[6][U];  // q[i]: (sigma0_i, w C_i1 ... w C_i6)
    if (fits && !any_bad && w > 0.0) {
        // 2. the design row, 3. the normal equations
        double a[U], N[U][U], L[U][U];
        a[0] = 1.0;
#pragma unroll
        for (int j = 0; j < 6; ++j) a[j + 1] = e[j] / w;
#pragma unroll
        for (int i = 0; i < U; ++i)
#pragma unroll
            for (int j = 0; j <= i; ++j) N[i][j] = N[j][i] = wave_sum(live ? a[i] * a[j] : 0.0);
        // 4. one factorisation, six solves
        if (cholesky_factor<U>(N, L)) {
            fitted = true;
#pragma unroll
            for (int i = 0; i < 6; ++i) {
                double b[U];
#pragma unroll
                for (int k = 0; k < U; ++k) b[k] = wave_sum(live ? a[k] * t[i] : 0.0);
                cholesky_substitute<U>(L, b, q[i]);
            }
            // 5. the residuals of the lane's six stress values, the scale undone, the asymmetry of the raw fit
            double ss = 0.0;
#pragma unroll
            for (int i = 0; i < 6; ++i) {
                double f = q[i][0];
#pragma unroll
                for (int k = 1; k < U; ++k) f = f + q[i][k] * a[k];
                const double r = f - t[i];
                ss = ss + r * r;
            }
            rms = sqrt(wave_sum(live ? ss : 0.0) / (6.0 * (double)P));
            double cmax = 0.0, dmax = 0.0;
#pragma unroll
            for (int i = 0; i < 6; ++i) {
                s0[i] = q[i][0];
#pragma unroll
                for (int j = 0; j < 6; ++j) {
                    C[i][j] = q[i][j + 1] / w;
                    cmax = fmax(cmax, fabs(C[i][j]));
                }
            }
#pragma unroll
            for (int i = 0; i < 6; ++i)
#pragma unroll
                for (int j = 0; j < 6; ++j) {
                    Cs[i][j] = (C[i][j] + C[j][i]) * 0.5;
                    if (j > i) dmax = fmax(dmax, fabs(C[i][j] - C[j][i]));
                }
            asym = dmax / cmax;
        }
    }
    if (fitted) {
        // 6. the compliance: positive definite (Born's criterion) or status 1; 7. the moduli
        const double ca = sum3(Cs[0][0], Cs[1][1], Cs[2][2]), cb = sum3(Cs[0][1], Cs[0][2], Cs[1][2]),
                     cc = sum3(Cs[3][3], Cs[4][4], Cs[5][5]);
        const double KV = (ca + 2.0 * cb) / 9.0, GV = ((ca - cb) + 3.0 * cc) / 15.0;
        mod[0] = KV, mod[3] = GV;
        double L6[6][6];
        status = 1;
        if (cholesky_factor<6>(Cs, L6)) {
            status = 0;
#pragma unroll
            for (int j = 0; j < 6; ++j) {
                double unit[6], x[6];
#pragma unroll
                for (int k = 0; k < 6; ++k) unit[k] = k == j ? 1.0 : 0.0;
                cholesky_substitute<6>(L6, unit, x);
#pragma unroll
                for (int k = 0; k < 6; ++k) S[k][j] = x[k];
            }
            const double sa = sum3(S[0][0], S[1][1], S[2][2]), sb = sum3(S[0][1], S[0][2], S[1][2]),
                         sc = sum3(S[3][3], S[4][4], S[5][5]);
            const double KR = 1.0 / (sa + 2.0 * sb), GR = 15.0 / ((4.0 * sa - 4.0 * sb) + 3.0 * sc);
            const double KH = (KV + KR) * 0.5, GH = (GV + GR) * 0.5;
            const double d = 3.0 * KH + GH;
            mod[1] = KR, mod[2] = KH, mod[4] = GR, mod[5] = GH;
            mod[6] = ((9.0 * KH) * GH) / d;
            mod[7] = (3.0 * KH - 2.0 * GH) / (2.0 * d);
            mod[8] = ((5.0 * GV) / GR + KV / KR) - 6.0;
        }
    }
    if (lane == 0) {
#pragma unroll
        for (int i = 0; i < 6; ++i) {
            sigma0[6 * (int64_t)s + i] = s0[i];
#pragma unroll
            for (int j = 0; j < 6; ++j) {
                const int64_t k = 36 * (int64_t)s + 6 * i + j;
                c_raw[k] = C[i][j], c_sym[k] = Cs[i][j], compliance[k] = S[i][j];
            }
        }
#pragma unroll
        for (int i = 0; i < 9; ++i) moduli[9 * (int64_t)s + i] = mod[i];
        rms_out[s] = rms;
        asym_out[s] = asym;
        status_out[s] = status;
    }
}

}  // namespace

extern "C" int alignn_elastic_fit(const double* strain, const double* stress, const int32_t* n_points, int n_structures, int ld,
                                  double* c_raw, double* c, double* compliance, double* sigma0, double* moduli, double* rms,
                                  double* asymmetry, int32_t* status, alignn_stream_t stream) {
    if (n_structures < 0 || ld < EL_MIN_POINTS || ld > EL_MAX_POINTS || !strain || !stress || !c_raw || !c || !compliance ||
        !sigma0 || !moduli || !rms || !asymmetry || !status)
        return (int)hipErrorInvalidValue;
    if (n_structures == 0) return 0;
    elastic_fit_kernel<<<n_structures, ALIGNN_WAVE, 0, (hipStream_t)stream>>>(strain, stress, n_points, ld, c_raw, c, compliance,
                                                                              sigma0, moduli, rms, asymmetry, status);
    ALIGNN_CHECK_LAUNCH();
    return 0;
}
