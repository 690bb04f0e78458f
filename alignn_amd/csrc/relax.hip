// One FIRE step (fixed cell) for a batch of crystals: ASE's ase/optimize/fire.py as the reference's
// ForceField.optimize_atoms drives it (alignn/ff/ff.py:373-415: FIRE, downhill_check=False) with the convergence test of
// Optimizer.run in front of it, every structure's optimiser state on the device (alignn_amd/relax.py is the host loop).
//
// One workgroup per ACTIVE structure, threads grid-strided over its atoms, float64 throughout.  Three passes over the
// structure's atoms, each followed by a fixed-order workgroup reduction (shuffle-down within a wave, then the four wave
// partials added in wave order by every thread alike): no float atomics, so a structure's step is bit-identical from run to
// run and does not depend on which other structures share the launch.
//   pass 1  record F (and E) in the full-batch result arrays; F.v, |F|^2, |v|^2, max_i |F_i|^2
//           converged (max |F_i|^2 < fmax^2) or out of steps -> retire flag, no step
//   pass 2  v <- mix / reset (ASE's branch on P = F.v), v += dt F; |dr|^2 with dr = dt v
//   pass 3  dr clipped to maxstep over the whole structure, r += dr, frac = r inv(L) wrapped into [0, 1)
#include "../../include/alignn_hip.h"
#include "common.h"

namespace {

constexpr int FIRE_BLOCK = 256;
constexpr int FIRE_WAVES = FIRE_BLOCK / ALIGNN_WAVE;

// sums over the workgroup of NV values per thread (the last one a max when LAST_MAX); every thread returns the same bits
template <int NV, bool LAST_MAX>
__device__ __forceinline__ void block_reduce(double (&v)[NV], double (*sh)[FIRE_WAVES]) {
    const int lane = threadIdx.x & (ALIGNN_WAVE - 1), wave = threadIdx.x / ALIGNN_WAVE;
#pragma unroll
    for (int j = 0; j < NV; ++j) {
        const bool mx = LAST_MAX && j == NV - 1;
#pragma unroll
        for (int o = ALIGNN_WAVE / 2; o > 0; o >>= 1) {
            const double u = __shfl_down(v[j], o, ALIGNN_WAVE);
            v[j] = mx ? fmax(v[j], u) : v[j] + u;
        }
        if (lane == 0) sh[j][wave] = v[j];
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < NV; ++j) {
        const bool mx = LAST_MAX && j == NV - 1;
        double s = sh[j][0];
#pragma unroll
        for (int w = 1; w < FIRE_WAVES; ++w) s = mx ? fmax(s, sh[j][w]) : s + sh[j][w];
        v[j] = s;
    }
    __syncthreads();  // (sh is reused by the next reduction)
}

__device__ __forceinline__ double wrap01(double f) {
    f -= floor(f);
    return f < 1.0 ? f : 0.0;  // (-tiny - floor(-tiny) rounds to 1.0)
}

__global__ __launch_bounds__(FIRE_BLOCK) void fire_step_kernel(
    const double* __restrict__ forces, const double* __restrict__ energy, const int32_t* __restrict__ force_ptr,
    const int32_t* __restrict__ active, const int32_t* __restrict__ atom_ptr, const double* __restrict__ inv_lattice,
    double* __restrict__ pos, double* __restrict__ vel, double* __restrict__ frac, double* __restrict__ forces_out,
    double* __restrict__ energy_out, double* __restrict__ state, int32_t* __restrict__ istate, double* __restrict__ fmax_out,
    int32_t* __restrict__ status, double fmax_tol, int steps, double maxstep, double dtmax, int nmin, double finc, double fdec,
    double astart, double fa) {
    __shared__ double sh[4][FIRE_WAVES];
    const int k = blockIdx.x;
    const int s = active[k];
    const int beg = atom_ptr[s], n = atom_ptr[s + 1] - beg;
    const int fbeg = force_ptr[k];
    if (force_ptr[k + 1] - fbeg != n) {  // forces of another shape than the structure: touch nothing
        if (threadIdx.x == 0) status[1 + k] = -1;
        return;
    }
    const double* F = forces + 3 * (int64_t)fbeg;
    double* R = pos + 3 * (int64_t)beg;
    double* V = vel + 3 * (int64_t)beg;
    const int taken = istate[2 * s + 1];

    // pass 1
    double red[4] = {0.0, 0.0, 0.0, 0.0};  // F.v, |F|^2, |v|^2, max |F_i|^2
    for (int i = threadIdx.x; i < n; i += FIRE_BLOCK) {
        double f[3], v[3], fi2 = 0.0;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            f[c] = F[3 * i + c];
            v[c] = V[3 * i + c];
            forces_out[3 * ((int64_t)beg + i) + c] = f[c];
            red[0] += f[c] * v[c];
            fi2 += f[c] * f[c];
            red[2] += v[c] * v[c];
        }
        red[1] += fi2;
        red[3] = fmax(red[3], fi2);
    }
    block_reduce<4, true>(red, sh);
    const int converged = red[3] < fmax_tol * fmax_tol;
    if (threadIdx.x == 0) {
        energy_out[s] = energy[k];
        fmax_out[s] = sqrt(red[3]);
        const int flag = converged ? 1 : (taken >= steps ? 2 : 0);
        status[1 + k] = flag;
        if (!flag) atomicAdd(status, 1);  // (an integer count: order-independent)
    }
    if (converged || taken >= steps) return;

    // pass 2: ASE FIRE.step
    double dt = state[2 * s], a = state[2 * s + 1];
    int nsteps = istate[2 * s];
    bool zero_v = taken == 0;  // first step: v = 0, no mixing
    double mix_v = 1.0, mix_f = 0.0;
    if (!zero_v) {
        if (red[0] > 0.0) {
            mix_v = 1.0 - a;
            mix_f = a / sqrt(red[1]) * sqrt(red[2]);
            if (nsteps > nmin) {
                dt = fmin(dt * finc, dtmax);
                a *= fa;
            }
            nsteps += 1;
        } else {
            zero_v = true;
            a = astart;
            dt *= fdec;
            nsteps = 0;
        }
    }
    double dr2[1] = {0.0};
    for (int i = threadIdx.x; i < n; i += FIRE_BLOCK) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const double f = F[3 * i + c];
            double v = zero_v ? 0.0 : mix_v * V[3 * i + c] + mix_f * f;
            v += dt * f;
            V[3 * i + c] = v;
            const double d = dt * v;
            dr2[0] += d * d;
        }
    }
    block_reduce<1, false>(dr2, sh);

    // pass 3
    const double normdr = sqrt(dr2[0]);
    const bool clip = normdr > maxstep;
    const double* L = inv_lattice + 9 * (int64_t)s;
    for (int i = threadIdx.x; i < n; i += FIRE_BLOCK) {
        double r[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            double d = dt * V[3 * i + c];
            if (clip) d = maxstep * d / normdr;
            r[c] = R[3 * i + c] + d;
            R[3 * i + c] = r[c];
        }
#pragma unroll
        for (int c = 0; c < 3; ++c)
            frac[3 * ((int64_t)beg + i) + c] = wrap01(r[0] * L[c] + r[1] * L[3 + c] + r[2] * L[6 + c]);
    }
    if (threadIdx.x == 0) {
        state[2 * s] = dt;
        state[2 * s + 1] = a;
        istate[2 * s] = nsteps;
        istate[2 * s + 1] = taken + 1;
    }
}

}  // namespace

extern "C" int alignn_fire_step(const double* forces, const double* energy, const int32_t* force_ptr, const int32_t* active,
                                int n_active, const int32_t* atom_ptr, const double* inv_lattice, double* positions,
                                double* velocities, double* frac, double* forces_out, double* energy_out, double* state,
                                int32_t* istate, double* fmax_out, int32_t* status, double fmax_tol, int steps, double maxstep,
                                double dtmax, int nmin, double finc, double fdec, double astart, double fa,
                                alignn_stream_t stream) {
    if (n_active < 0 || !status) return (int)hipErrorInvalidValue;
    hipStream_t st = (hipStream_t)stream;
    hipError_t e = hipMemsetAsync(status, 0, sizeof(int32_t), st);
    if (e != hipSuccess) return (int)e;
    if (n_active == 0) return 0;
    fire_step_kernel<<<n_active, FIRE_BLOCK, 0, st>>>(forces, energy, force_ptr, active, atom_ptr, inv_lattice, positions,
                                                      velocities, frac, forces_out, energy_out, state, istate, fmax_out, status,
                                                      fmax_tol, steps, maxstep, dtmax, nmin, finc, fdec, astart, fa);
    ALIGNN_CHECK_LAUNCH();
    return 0;
}
