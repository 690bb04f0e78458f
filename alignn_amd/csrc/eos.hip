// Device side of the E-V curve task (alignn_amd/eos.py): the strained copies of the parent crystals, written in the arrays
// ``relax`` takes, and the equation-of-state fit of every crystal's (volume, energy) points.  The reference strains one crystal
// at a time on the host (jarvis-tools' Atoms.strain_atoms) and fits with ASE's EquationOfState.fit, two scipy curve_fit calls per
// crystal (alignn/ff/ff.py:762-805).  tests/eos_ref.py is the numpy restatement this file follows operation for operation.
//
//   strain_build_kernel   one workgroup per job (parent, deformation F): cell' = cell F, r' = r F, |det cell'|;
//   eos_fit_kernel        one wavefront per structure, one lane per strain point: the parabola start, then Levenberg-Marquardt
//                         on (E0, B0, BP, V0) with the analytic Jacobian, the 4 x 4 normal equations solved in every lane
//                         (wave_sum and cholesky_solve: wave_fit.h, shared with elastic.hip).
// float64, no contraction, no atomics, every sum in a fixed order (the sums over the strain points by the xor butterfly of
// wave_sum, after which every lane holds the same bits, so the control flow is wave-uniform): a structure's bits do not depend
// on what else shares the launch.  The stopping tests of the fit sit at the rounding level of its residuals, so its step count
// follows the last bits of x^BP; flog / fexp below are therefore written in +, -, *, / and frexp / ldexp only, as the restatement
// has them, and the fit is the restatement's bits too.
#include "../../include/alignn_hip.h"
#include "common.h"
#include "cell3.h"
#include "wave_fit.h"

#pragma clang fp contract(off)

namespace {

constexpr int SB_BLOCK = 256;
constexpr int EOS_MIN_POINTS = 4, EOS_MAX_POINTS = ALIGNN_WAVE;
constexpr double EOS_LAMBDA0 = 1e-3, EOS_LAMBDA_MIN = 1e-15, EOS_LAMBDA_MAX = 1e15;
constexpr double EOS_XTOL = 1e-13, EOS_FTOL = 1e-16;
constexpr int EOS_MAX_STEPS = 100;

// Row i of the new cell is row i of the parent times F, r' = r F for every atom, the volume |det| of the NEW cell along its first
// row.  A job whose parent index or row range does not fit writes nothing.
__global__ __launch_bounds__(SB_BLOCK) void strain_build_kernel(
    const double* __restrict__ pos, const int32_t* __restrict__ atom_ptr, const double* __restrict__ lattice, int n_structures,
    const int32_t* __restrict__ jobs, const double* __restrict__ defgrad, const int64_t* __restrict__ row_off,
    double* __restrict__ cells, double* __restrict__ cart, double* __restrict__ volume) {
    const int job = blockIdx.x;
    const int s = jobs[job];
    if (s < 0 || s >= n_structures) return;
    const int beg = atom_ptr[s], n = atom_ptr[s + 1] - beg;
    const int64_t row0 = row_off[job];
    if (n < 1 || row_off[job + 1] - row0 != n) return;
    const double* L = lattice + 9 * (int64_t)s;
    double F[9], C[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) F[i] = defgrad[9 * (int64_t)job + i];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int k = 0; k < 3; ++k) C[3 * i + k] = row_dot(L + 3 * i, F, k);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int i = 0; i < 9; ++i) cells[9 * (int64_t)job + i] = C[i];
        const double det = (C[0] * (C[4] * C[8] - C[5] * C[7]) - C[1] * (C[3] * C[8] - C[5] * C[6])) + C[2] * (C[3] * C[7] - C[4] * C[6]);
        volume[job] = fabs(det);
    }
    for (int j = threadIdx.x; j < n; j += SB_BLOCK) {
        const double* r = pos + 3 * ((int64_t)beg + j);
        const double x[3] = {r[0], r[1], r[2]};
#pragma unroll
        for (int k = 0; k < 3; ++k) cart[3 * (row0 + j) + k] = row_dot(x, F, k);
    }
}

// ---- log and exp in plain arithmetic (tests/eos_ref.py flog / fexp) ----
constexpr double LN2_HI = 6.93147180369123816490e-01, LN2_LO = 1.90821492927058770002e-10;  // the low 21 bits of hi are zero
constexpr double INV_LN2 = 1.44269504088896338700e+00, SQRT_HALF = 0.70710678118654752440;

// ln x for finite x > 0, NaN otherwise: x = 2^e m, m in [sqrt(1/2), sqrt(2)), s = (m - 1) / (m + 1), z = s^2,
// ln m = 2 s (1 + z / 3 + ... + z^11 / 23), ln x = (e ln2_hi + ln m) + e ln2_lo
__device__ __forceinline__ double flog(double x) {
    if (!(x > 0.0 && x < INFINITY)) return NAN;
    int e;
    double m = frexp(x, &e);
    if (m < SQRT_HALF) {
        m = m + m;
        e -= 1;
    }
    const double s = (m - 1.0) / (m + 1.0), z = s * s;
    double p = 1.0 / 23.0;
#pragma unroll
    for (int d = 21; d > 0; d -= 2) p = 1.0 / (double)d + z * p;
    const double ed = (double)e;
    return (ed * LN2_HI + (2.0 * s) * p) + ed * LN2_LO;
}

// e^x for |x| <= 700 (inf above, 0 below, NaN for NaN): k = floor(x / ln 2 + 1/2), r = (x - k ln2_hi) - k ln2_lo, e^r by its
// Taylor polynomial of degree 13 as p = 1 + r p / n, n = 13 ... 1, then ldexp(p, k)
__device__ __forceinline__ double fexp(double x) {
    if (!(fabs(x) <= 700.0)) return x > 700.0 ? INFINITY : (x < -700.0 ? 0.0 : NAN);
    const double k = floor(x * INV_LN2 + 0.5);
    const double r = (x - k * LN2_HI) - k * LN2_LO;
    double p = 1.0;
#pragma unroll
    for (int n = 13; n > 0; --n) p = 1.0 + (r * p) / (double)n;
    return ldexp(p, (int)k);
}

// ---- the fit ----
// The form at p = (E0, B0, BP, V0) and volume V, as ase/eos.py states it: the energy and (JAC) its derivatives J[1..3] by B0, BP,
// V0 (the one by E0 is 1).
//   Murnaghan        E = E0 + B0 V / BP (x^BP / (BP - 1) + 1) - V0 B0 / (BP - 1),               x = V0 / V
//   Birch-Murnaghan  E = E0 + 9/16 B0 V0 f^2 (6 + BP f - 4 y),                                y = x^(2/3), f = y - 1
template <bool JAC>
__device__ __forceinline__ double eos_model(int form, double V, const double (&p)[4], double (&J)[4]) {
    const double E0 = p[0], B0 = p[1], BP = p[2], V0 = p[3];
    const double x = V0 / V;
    double E;
    if (form == 0) {
        const double lx = flog(x);
        const double t = fexp(BP * lx);  // x^BP
        const double q = BP - 1.0;
        const double u = t / q + 1.0;
        E = (E0 + ((B0 * V) / BP) * u) - (V0 * B0) / q;
        if (JAC) {
            J[1] = (V / BP) * u - V0 / q;
            J[2] = (B0 * V) * ((((t * lx) / q) - t / (q * q)) / BP - u / (BP * BP)) + (V0 * B0) / (q * q);
            J[3] = (B0 * (t / x - 1.0)) / q;
        }
    } else {
        const double y = fexp((2.0 / 3.0) * flog(x));
        const double f = y - 1.0;
        const double P = (6.0 + BP * f) - 4.0 * y;
        const double f2 = f * f;
        E = E0 + ((0.5625 * B0) * V0) * (f2 * P);
        if (JAC) {
            J[1] = (0.5625 * V0) * (f2 * P);
            J[2] = ((0.5625 * B0) * V0) * (f2 * f);
            J[3] = (0.5625 * B0) * (f2 * P + ((2.0 / 3.0) * y) * ((2.0 * f) * P + f2 * (BP - 4.0)));
        }
    }
    if (JAC) J[0] = 1.0;
    return E;
}

__device__ __forceinline__ double sum_sq(int form, double V, double E, bool live, const double (&p)[4]) {
    double J[4];
    const double r = eos_model<false>(form, V, p, J) - E;
    return wave_sum(live ? r * r : 0.0);
}

// One wavefront per structure; lane k < K holds point k, the other lanes add zeros.  The steps are those of tests/eos_ref.py
// parabola_start() and fit().
__global__ __launch_bounds__(ALIGNN_WAVE) void eos_fit_kernel(
    const double* __restrict__ volume, const double* __restrict__ energy, const int32_t* __restrict__ n_points, int ld, int form,
    double* __restrict__ params, double* __restrict__ rms, int32_t* __restrict__ n_iter_out, int32_t* __restrict__ status_out) {
    const int s = blockIdx.x, lane = threadIdx.x;
    const int K = n_points ? n_points[s] : ld;
    const double nan = NAN;
    double p[4] = {nan, nan, nan, nan}, S = nan;
    int n_iter = 0, status = 2;
    const bool fits = K >= EOS_MIN_POINTS && K <= ld;  // (ld <= 64: the entry point)
    const bool live = fits && lane < K;
    const double V = live ? volume[(int64_t)s * ld + lane] : 1.0, E = live ? energy[(int64_t)s * ld + lane] : 0.0;
    bool start = false;
    if (fits) {
        // 1. the parabola in u = (V - mean V) / (max V - min V), mapped back, and ASE's start values
        const double Kd = (double)K;
        const double m = wave_sum(live ? V : 0.0) / Kd;
        const double w = wave_max(live ? V : -INFINITY) - wave_min(live ? V : INFINITY);
        const double u = (V - m) / w, u2 = u * u;
        const double s1 = wave_sum(live ? u : 0.0), s2 = wave_sum(live ? u2 : 0.0), s3 = wave_sum(live ? u2 * u : 0.0),
                     s4 = wave_sum(live ? u2 * u2 : 0.0);
        const double t0 = wave_sum(live ? E : 0.0), t1 = wave_sum(live ? E * u : 0.0), t2 = wave_sum(live ? E * u2 : 0.0);
        const double A3[3][3] = {{Kd, s1, s2}, {s1, s2, s3}, {s2, s3, s4}}, b3[3] = {t0, t1, t2};
        double q3[3];
        if (cholesky_solve<3>(A3, b3, q3)) {
            const double c = q3[2] / (w * w);
            const double b = q3[1] / w - (2.0 * c) * m;
            const double a = (q3[0] - (q3[1] / w) * m) + (c * m) * m;
            const double vmin = -b / (2.0 * c);
            const double e0 = (a + b * vmin) + (c * vmin) * vmin, b0 = (2.0 * c) * vmin;
            if (c > 0.0 && fabs(e0) < INFINITY && fabs(b0) < INFINITY && fabs(vmin) < INFINITY) {
                p[0] = e0, p[1] = b0, p[2] = 4.0, p[3] = vmin;
                S = sum_sq(form, V, E, live, p);
                start = fabs(S) < INFINITY;
            }
        }
    }
    if (start) {
        // 2. Levenberg-Marquardt
        double lam = EOS_LAMBDA0;
        status = 1;
        while (n_iter < EOS_MAX_STEPS) {
            double J[4], A[4][4], g[4];
            const double r = eos_model<true>(form, V, p, J) - E;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
#pragma unroll
                for (int j = 0; j <= i; ++j) A[i][j] = A[j][i] = wave_sum(live ? J[i] * J[j] : 0.0);
                g[i] = wave_sum(live ? J[i] * r : 0.0);
            }
            bool done = false;
            for (;;) {
                double M[4][4], mg[4], delta[4], pn[4], Sn = nan;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
#pragma unroll
                    for (int j = 0; j < 4; ++j) M[i][j] = A[i][j];
                    M[i][i] = A[i][i] + lam * A[i][i];
                    mg[i] = -g[i];
                }
                if (cholesky_solve<4>(M, mg, delta)) {
#pragma unroll
                    for (int i = 0; i < 4; ++i) pn[i] = p[i] + delta[i];
                    Sn = sum_sq(form, V, E, live, pn);
                }
                if (fabs(Sn) < INFINITY && Sn <= S) {  // the step is taken
                    ++n_iter;
                    lam = fmax(lam / 10.0, EOS_LAMBDA_MIN);
                    const double dmax = fmax(fmax(fabs(delta[0]), fabs(delta[1])), fmax(fabs(delta[2]), fabs(delta[3])));
                    const double pmax = fmax(fmax(fabs(pn[0]), fabs(pn[1])), fmax(fabs(pn[2]), fabs(pn[3])));
                    done = dmax <= EOS_XTOL * pmax || S - Sn <= EOS_FTOL * S;
#pragma unroll
                    for (int i = 0; i < 4; ++i) p[i] = pn[i];
                    S = Sn;
                    break;
                }
                lam = lam * 10.0;
                if (lam > EOS_LAMBDA_MAX) {  // no step of any length lowers S: a minimum to rounding
                    done = true;
                    break;
                }
            }
            if (done) {
                status = 0;
                break;
            }
        }
    } else {
#pragma unroll
        for (int i = 0; i < 4; ++i) p[i] = nan;
        S = nan;
    }
    if (lane == 0) {
#pragma unroll
        for (int i = 0; i < 4; ++i) params[4 * (int64_t)s + i] = p[i];
        rms[s] = start ? sqrt(S / (double)K) : nan;
        n_iter_out[s] = n_iter;
        status_out[s] = status;
    }
}

}  // namespace

extern "C" int alignn_strain_build(const double* positions, const int32_t* atom_ptr, const double* lattice, int n_structures,
                                   const int32_t* jobs, const double* defgrad, const int64_t* row_off, int n_jobs, double* cells,
                                   double* cart, double* volume, alignn_stream_t stream) {
    if (n_jobs < 0 || n_structures < 1 || !positions || !atom_ptr || !lattice || !jobs || !defgrad || !row_off || !cells || !cart ||
        !volume)
        return (int)hipErrorInvalidValue;
    if (n_jobs == 0) return 0;
    strain_build_kernel<<<n_jobs, SB_BLOCK, 0, (hipStream_t)stream>>>(positions, atom_ptr, lattice, n_structures, jobs, defgrad,
                                                                       row_off, cells, cart, volume);
    ALIGNN_CHECK_LAUNCH();
    return 0;
}

extern "C" int alignn_eos_fit(const double* volume, const double* energy, const int32_t* n_points, int n_structures, int ld,
                              int form, double* params, double* rms, int32_t* n_iter, int32_t* status, alignn_stream_t stream) {
    if (n_structures < 0 || ld < EOS_MIN_POINTS || ld > EOS_MAX_POINTS || (form != 0 && form != 1) || !volume || !energy || !params ||
        !rms || !n_iter || !status)
        return (int)hipErrorInvalidValue;
    if (n_structures == 0) return 0;
    eos_fit_kernel<<<n_structures, ALIGNN_WAVE, 0, (hipStream_t)stream>>>(volume, energy, n_points, ld, form, params, rms, n_iter,
                                                                          status);
    ALIGNN_CHECK_LAUNCH();
    return 0;
}
