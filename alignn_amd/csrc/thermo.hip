// Device side of the harmonic thermodynamics and of the quasi-harmonic approximation (alignn_amd/thermo.py): the sums over the
// phonon modes of a q-mesh at every temperature, and the reduction of the per-temperature equation-of-state fits to the thermal
// quantities.  The reference has neither on the device: its phonon paths hand a mesh to phonopy's ``run_thermal_properties`` on
// the host (alignn/ff/ff.py), mode by mode and temperature by temperature.  tests/thermo_ref.py is the numpy restatement.
//
//   thermal_partial_kernel   one workgroup per (chunk of TH_CHUNK frequencies, structure): its frequencies in registers, a loop
//                            over the temperatures, the four sums of the chunk by block_reduce -> partials [chunk][NT][4];
//   thermal_finish_kernel    the chunks of a structure added in ascending order, the averages over the q-points -> F, U, S, Cv;
//   qha_derive_kernel        one wavefront per (structure, temperature), one lane per volume point: the thermal expansion by
//                            differences of the fitted volumes, Cv and S at the fitted volume by a least-squares quadratic
//                            (wave_sum and cholesky_solve: wave_fit.h), then C_p and the Grueneisen parameter.
// float64, no contraction, no atomics, every sum in a fixed order that depends on the structure's own data only (TH_CHUNK is a
// constant): a structure's bits are the same alone, in a batch and at any place of the batch.
#include "../../include/alignn_thermo.h"
#include "common.h"
#include "wave_fit.h"

#pragma clang fp contract(off)

namespace {

constexpr int TH_BLOCK = 256, TH_WAVES = TH_BLOCK / ALIGNN_WAVE, TH_PER_THREAD = 4;
constexpr int TH_CHUNK = TH_BLOCK * TH_PER_THREAD;  // frequencies per workgroup
constexpr int TH_FIN_BLOCK = 64;
constexpr double TH_KB = 1.38064852e-23 / 1.6021766208e-19;  // eV/K, CODATA 2014 (the unit set of alignn_amd/phonons.py)
// x = eps / (kB T) above which a mode is at its T -> 0 limit: the terms left out are below 700 e^-700 = 1e-301 of a kB.  The
// branch also keeps x = inf (a temperature below eps / kB / 1.8e308) away from 0 * inf.
constexpr double TH_X_COLD = 700.0;
constexpr int QHA_MIN_POINTS = 4, QHA_MAX_POINTS = ALIGNN_WAVE;

__host__ __device__ inline int64_t chunks_of(int64_t n) { return (n + TH_CHUNK - 1) / TH_CHUNK; }

// The four terms of one counted mode eps at temperature T (kT = kB T): those of F, U, S / kB and Cv / kB.
__device__ __forceinline__ void mode_terms(double eps, double T, double kT, double (&t)[4]) {
    const double half = 0.5 * eps;
    const double x = eps / kT;
    if (!(T > 0.0) || !(x <= TH_X_COLD)) {  // T = 0, or frozen out
        t[0] = half, t[1] = half, t[2] = 0.0, t[3] = 0.0;
        return;
    }
    const double em = exp(-x), om = -expm1(-x);
    const double lg = log(om);
    const double r = x / om;  // -> 1 for x -> 0, where x^2 alone would underflow
    t[0] = half + kT * lg;
    t[1] = eps * (0.5 + em / om);
    t[2] = r * em - lg;
    t[3] = (r * r) * em;
}

// Workgroup (c, s): frequencies [beg + c TH_CHUNK, ...) of structure s, thread t holding those at t, t + 256, t + 512, t + 768 of
// the chunk.  part [(s max_chunks + c)][NT][4] and aux [(s max_chunks + c)][2] = (sum of eps / 2, skipped modes) of the chunk.
__global__ __launch_bounds__(TH_BLOCK) void thermal_partial_kernel(
    const double* __restrict__ freqs, const int64_t* __restrict__ freq_off, const double* __restrict__ temperatures, int n_temps,
    double cutoff, int max_chunks, double* __restrict__ part, double* __restrict__ aux) {
    __shared__ double sh[4][TH_WAVES];
    const int c = blockIdx.x, s = blockIdx.y;
    const int64_t beg = freq_off[s], n = freq_off[s + 1] - beg;
    if (c >= chunks_of(n)) return;  // (uniform over the workgroup)
    double eps[TH_PER_THREAD];
    bool counted[TH_PER_THREAD];
    double head[2] = {0.0, 0.0};
#pragma unroll
    for (int i = 0; i < TH_PER_THREAD; ++i) {
        const int64_t k = (int64_t)c * TH_CHUNK + i * TH_BLOCK + threadIdx.x;
        const bool in = k < n;
        eps[i] = in ? freqs[beg + k] : 0.0;
        counted[i] = in && eps[i] > cutoff;  // (a NaN is skipped as well)
        if (counted[i]) head[0] = head[0] + 0.5 * eps[i];
        if (in && !counted[i]) head[1] = head[1] + 1.0;
    }
    block_reduce<2, false>(head, sh);
    const int64_t slot = (int64_t)s * max_chunks + c;
    if (threadIdx.x == 0) aux[2 * slot] = head[0], aux[2 * slot + 1] = head[1];
    for (int it = 0; it < n_temps; ++it) {
        const double T = temperatures[it], kT = TH_KB * T;
        double v[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int i = 0; i < TH_PER_THREAD; ++i)
            if (counted[i]) {
                double t[4];
                mode_terms(eps[i], T, kT, t);
#pragma unroll
                for (int j = 0; j < 4; ++j) v[j] = v[j] + t[j];
            }
        block_reduce<4, false>(v, sh);
        if (threadIdx.x == 0) {
#pragma unroll
            for (int j = 0; j < 4; ++j) part[(slot * n_temps + it) * 4 + j] = v[j];
        }
    }
}

// Thread e of structure s: value e < 4 NT is (temperature e / 4, quantity e % 4), 4 NT the zero-point energy, 4 NT + 1 the skipped
// modes; each the sum over the structure's chunks in ascending order, then the average over the q-points.
__global__ __launch_bounds__(TH_FIN_BLOCK) void thermal_finish_kernel(
    const int64_t* __restrict__ freq_off, const int32_t* __restrict__ n_q, int n_temps, int max_chunks,
    const double* __restrict__ part, const double* __restrict__ aux, double* __restrict__ F, double* __restrict__ U,
    double* __restrict__ S, double* __restrict__ Cv, double* __restrict__ zpe, int32_t* __restrict__ n_skipped) {
    const int s = blockIdx.y, e = blockIdx.x * TH_FIN_BLOCK + threadIdx.x;
    const int n_values = 4 * n_temps;
    if (e >= n_values + 2) return;
    const int64_t nc_s = chunks_of(freq_off[s + 1] - freq_off[s]);
    const int nc = (int)(nc_s < max_chunks ? nc_s : max_chunks);  // (max_chunks: what the first launch wrote)
    const double nq = (double)n_q[s];
    const int64_t slot0 = (int64_t)s * max_chunks;
    double acc = 0.0;
    if (e < n_values) {
        for (int c = 0; c < nc; ++c) acc = acc + part[(slot0 + c) * n_values + e];
        const int it = e >> 2, j = e & 3;
        const int64_t o = (int64_t)s * n_temps + it;
        if (j == 0) F[o] = acc / nq;
        if (j == 1) U[o] = acc / nq;
        if (j == 2) S[o] = TH_KB * (acc / nq);
        if (j == 3) Cv[o] = TH_KB * (acc / nq);
    } else {
        const int j = e - n_values;
        for (int c = 0; c < nc; ++c) acc = acc + aux[2 * (slot0 + c) + j];
        if (j == 0) zpe[s] = acc / nq;
        if (j == 1) n_skipped[s] = (int32_t)acc;  // (whole numbers below 2^53: exact)
    }
}

// The least-squares quadratic in x through (x, y) of the live lanes at xe: (q0 + q1 xe) + (q2 xe) xe, NaN without a solution.
__device__ __forceinline__ double quadratic_at(double x, double y, bool live, double Pd, double xe) {
    const double x2 = x * x;
    const double s1 = wave_sum(live ? x : 0.0), s2 = wave_sum(live ? x2 : 0.0), s3 = wave_sum(live ? x2 * x : 0.0),
                 s4 = wave_sum(live ? x2 * x2 : 0.0);
    const double t0 = wave_sum(live ? y : 0.0), t1 = wave_sum(live ? y * x : 0.0), t2 = wave_sum(live ? y * x2 : 0.0);
    const double A[3][3] = {{Pd, s1, s2}, {s1, s2, s3}, {s2, s3, s4}}, b[3] = {t0, t1, t2};
    double q[3];
    if (!cholesky_solve<3>(A, b, q)) return NAN;
    return (q[0] + q[1] * xe) + (q[2] * xe) * xe;
}

// One wavefront per (temperature i, structure s); lane p < P holds volume point p, the other lanes add zeros.  The steps are those
// of tests/thermo_ref.py qha_derive().
__global__ __launch_bounds__(ALIGNN_WAVE) void qha_derive_kernel(
    const double* __restrict__ volumes, const double* __restrict__ cv_in, const double* __restrict__ s_in,
    const double* __restrict__ temperatures, const double* __restrict__ v_eq, const double* __restrict__ b_t,
    const int32_t* __restrict__ status, int P, int NT, double* __restrict__ alpha, double* __restrict__ cv_out,
    double* __restrict__ s_out, double* __restrict__ cp_out, double* __restrict__ gamma, int32_t* __restrict__ inside) {
    const int i = blockIdx.x, s = blockIdx.y, lane = threadIdx.x;
    const int64_t row = (int64_t)s * NT;
    const bool live = lane < P;
    const double nan = NAN;
    const double V = live ? volumes[(int64_t)s * P + lane] : 0.0;
    const double vmax = wave_max(live ? V : -INFINITY), vmin = wave_min(live ? V : INFINITY);
    const double Vi = v_eq[row + i], Bi = b_t[row + i], Ti = temperatures[i];
    const bool fitted = status[row + i] != 2;

    // the thermal expansion: central differences of the fitted volumes inside, one-sided ones at the two ends
    double a = nan;
    if (NT > 1) {
        const int lo = i > 0 ? i - 1 : i, hi = i < NT - 1 ? i + 1 : i;
        if (fitted && status[row + lo] != 2 && status[row + hi] != 2)
            a = ((v_eq[row + hi] - v_eq[row + lo]) / (temperatures[hi] - temperatures[lo])) / Vi;
    }

    // Cv and S at the fitted volume
    double cv = nan, en = nan, cp = nan, g = nan;
    int in = 0;
    if (fitted) {  // (uniform over the wavefront)
        const double mid = (vmax + vmin) / 2.0, h = (vmax - vmin) / 2.0;
        const double x = (V - mid) / h, xe = (Vi - mid) / h;
        const int64_t k = ((int64_t)s * P + lane) * NT + i;
        cv = quadratic_at(x, live ? cv_in[k] : 0.0, live, (double)P, xe);
        en = quadratic_at(x, live ? s_in[k] : 0.0, live, (double)P, xe);
        cp = cv + ((Ti * Vi) * (a * a)) * Bi;
        g = cv == 0.0 ? nan : ((a * Bi) * Vi) / cv;
        in = vmin <= Vi && Vi <= vmax;
    }
    if (lane == 0) {
        alpha[row + i] = a;
        cv_out[row + i] = cv;
        s_out[row + i] = en;
        cp_out[row + i] = cp;
        gamma[row + i] = g;
        inside[row + i] = in;
    }
}

}  // namespace

extern "C" size_t alignn_phonon_thermal_workspace(int n_structures, int64_t max_freqs, int n_temps) {
    if (n_structures < 1 || max_freqs < 0 || n_temps < 1) return 0;
    const int64_t slots = (int64_t)n_structures * (chunks_of(max_freqs) > 0 ? chunks_of(max_freqs) : 1);
    return (size_t)slots * ((size_t)4 * n_temps + 2) * sizeof(double);
}

extern "C" int alignn_phonon_thermal(const double* freqs, const int64_t* freq_off, const int32_t* n_q, int n_structures,
                                     int64_t max_freqs, const double* temperatures, int n_temps, double cutoff, void* workspace,
                                     size_t workspace_bytes, double* free_energy, double* internal_energy, double* entropy,
                                     double* heat_capacity, double* zpe, int32_t* n_skipped, void* stream) {
    if (n_structures < 1 || max_freqs < 0 || n_temps < 1 || !(cutoff >= 0.0) || !freqs || !freq_off || !n_q || !temperatures ||
        !workspace || !free_energy || !internal_energy || !entropy || !heat_capacity || !zpe || !n_skipped)
        return (int)hipErrorInvalidValue;
    const int64_t max_chunks = chunks_of(max_freqs) > 0 ? chunks_of(max_freqs) : 1;
    if (n_structures > 65535 || max_chunks > 0x7fffffff ||
        workspace_bytes < alignn_phonon_thermal_workspace(n_structures, max_freqs, n_temps))
        return (int)hipErrorInvalidValue;
    double* part = (double*)workspace;
    double* aux = part + (int64_t)n_structures * max_chunks * 4 * n_temps;
    thermal_partial_kernel<<<dim3((unsigned)max_chunks, n_structures), TH_BLOCK, 0, (hipStream_t)stream>>>(
        freqs, freq_off, temperatures, n_temps, cutoff, (int)max_chunks, part, aux);
    ALIGNN_CHECK_LAUNCH();
    thermal_finish_kernel<<<dim3(alignn_ceil_div(4 * (int64_t)n_temps + 2, TH_FIN_BLOCK), n_structures), TH_FIN_BLOCK, 0,
                            (hipStream_t)stream>>>(freq_off, n_q, n_temps, (int)max_chunks, part, aux, free_energy,
                                                   internal_energy, entropy, heat_capacity, zpe, n_skipped);
    ALIGNN_CHECK_LAUNCH();
    return 0;
}

extern "C" int alignn_qha_derive(const double* volumes, const double* heat_capacity, const double* entropy,
                                 const double* temperatures, const double* v_eq, const double* b_t, const int32_t* status,
                                 int n_structures, int n_points, int n_temps, double* alpha, double* cv_out, double* s_out,
                                 double* cp_out, double* gamma, int32_t* inside, void* stream) {
    if (n_structures < 0 || n_structures > 65535 || n_points < QHA_MIN_POINTS || n_points > QHA_MAX_POINTS || n_temps < 1 ||
        !volumes || !heat_capacity || !entropy || !temperatures || !v_eq || !b_t || !status || !alpha || !cv_out || !s_out ||
        !cp_out || !gamma || !inside)
        return (int)hipErrorInvalidValue;
    if (n_structures == 0) return 0;
    qha_derive_kernel<<<dim3(n_temps, n_structures), ALIGNN_WAVE, 0, (hipStream_t)stream>>>(
        volumes, heat_capacity, entropy, temperatures, v_eq, b_t, status, n_points, n_temps, alpha, cv_out, s_out, cp_out, gamma,
        inside);
    ALIGNN_CHECK_LAUNCH();
    return 0;
}
