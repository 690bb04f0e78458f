// Batched molecular dynamics: ASE 3.22.1's VelocityVerlet, Langevin, NVTBerendsen, Andersen and NPTBerendsen (ase/md/*.py) as
// the reference's ForceField.run_nve_velocity_verlet / run_nvt_langevin / run_nvt_berendsen / run_nvt_andersen /
// run_npt_berendsen drive them (alignn/ff/ff.py:419-600), every structure's integrator state on the device
// (alignn_amd/dynamics.py is the host loop; tests/test_md_ref.py and tests/test_md_npt_ref.py the numpy restatements this file
// follows).  md_step_kernel runs the three fixed-cell ensembles 0-2, md_step_cell_kernel Andersen (3) and NPT Berendsen (4).
//
// Iteration t of the host loop evaluates the forces F_t at r_t; one md_step_kernel launch then
//   1. finishes step t (t > 0): the second half-kick with F_t (Langevin: v += c1 F/m - c2 v + rnd_vel, p = v m);
//   2. records frame t / interval when t % interval == 0: E_pot, KE, T, and the trajectory rows;
//   3. begins step t + 1 (t < steps): the first half-kick and the drift (Berendsen: the velocity scaling first; Langevin: the
//      noise of this step), the wrapped fractional coordinates of r_{t+1} for the next neighbour search.
// One workgroup per structure, threads grid-strided over its atoms, float64 throughout.  Every sum (KE, the Berendsen
// momentum sum, the Langevin fixcm sums) goes through the fixed-order block_reduce: a structure's trajectory is the same bits
// whether it runs alone or beside others.
//
// Random numbers: Philox4x32-10, key (seed & 0xffffffff, seed >> 32), counter (atom i within the structure, t, block j,
// purpose).  A block's words (w0, w1, w2, w3) give u1 = unit(w0, w1), u2 = unit(w2, w3) and the two normals
// sqrt(-2 ln u1) (cos, sin)(2 pi u2).  Langevin (purpose 0) takes blocks j = 0, 1, 2 at counter t = the iteration that
// begins the step: normals g0..g5 in block order, cos before sin; xi = (g0, g1, g2), eta = (g3, g4, g5).  The initial
// Maxwell-Boltzmann momenta (purpose 1) take blocks 0 and 1 at t = 0: xi = (g0, g1, g2).  Andersen (purpose 2) takes blocks
// j = 0 .. 3 of counter (atom, t, j, 2): blocks 0, 1 give the normals g0..g3 (replacement velocity = (g0, g1, g2) sqrt(kB T0 / m)),
// blocks 2, 3 the uniforms u0 = unit(w0, w1), u1 = unit(w2, w3) of block 2 and u2, u3 of block 3; component c is replaced when
// u_c <= andersen_prob (unit() lies in (0, 1]: probability 0 never replaces, 1 always).  Its centre-of-mass velocity (purpose 3)
// takes blocks j = 0, 1 of counter (0, t, j, 3): (g0, g1, g2) sqrt(kB T0 / sum m).  Purposes 0 and 1 are drawn as before.
//
// md_step_cell_kernel has the same three parts.  NPT Berendsen begins a step with NVTBerendsen's velocity scaling, then the
// pressure P = -tr(S_t) / 3 + 2 KE / (3 V) of the scaled momenta and the evaluation's stress S_t, V = |det cell|, the factor
// mu = 1 - (dt / taup) compressibility / 3 (P_target - P), cell and positions times mu (every thread computes mu, the new cell
// and its inverse by cofactors alike; thread 0 writes them), then NVTBerendsen's half-kick, fixcm and drift; frac uses the new
// inverse.  Andersen keeps v between the halves (velocities) and the positions before the drift (rnd_vel, as scratch).
#include "../../include/alignn_hip.h"
#include "common.h"

namespace {

constexpr int MD_BLOCK = 256;
constexpr int MD_WAVES = MD_BLOCK / ALIGNN_WAVE;
enum { MD_NVE = 0, MD_LANGEVIN = 1, MD_BERENDSEN = 2, MD_ANDERSEN = 3, MD_NPT_BERENDSEN = 4 };
enum { PURPOSE_LANGEVIN = 0, PURPOSE_MOMENTA = 1, PURPOSE_ANDERSEN = 2, PURPOSE_ANDERSEN_COM = 3 };

// Philox4x32-10 (Salmon et al., SC'11), the counter c overwritten by the output block
__device__ __forceinline__ void philox4x32_10(uint32_t (&c)[4], uint32_t k0, uint32_t k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        if (r) {
            k0 += 0x9E3779B9u;
            k1 += 0xBB67AE85u;
        }
        const uint32_t lo0 = 0xD2511F53u * c[0], hi0 = __umulhi(0xD2511F53u, c[0]);
        const uint32_t lo1 = 0xCD9E8D57u * c[2], hi1 = __umulhi(0xCD9E8D57u, c[2]);
        const uint32_t n0 = hi1 ^ c[1] ^ k0, n2 = hi0 ^ c[3] ^ k1;
        c[0] = n0;
        c[1] = lo1;
        c[2] = n2;
        c[3] = lo0;
    }
}

// 53 random bits from two words, in (0, 1]: never 0; the + 0.5 rounds to 1.0 only for the largest pattern (probability 2^-53)
__device__ __forceinline__ double unit_interval(uint32_t a, uint32_t b) {
    return ((double)(a >> 5) * 67108864.0 + (double)(b >> 6) + 0.5) * 0x1p-53;
}

// the two Box-Muller normals of Philox block (i, t, j, purpose); w returns its four words
__device__ __forceinline__ void normal_pair(uint32_t i, uint32_t t, uint32_t j, uint32_t purpose, uint32_t k0, uint32_t k1,
                                            double& z0, double& z1, uint32_t (&w)[4]) {
    w[0] = i;
    w[1] = t;
    w[2] = j;
    w[3] = purpose;
    philox4x32_10(w, k0, k1);
    const double rad = sqrt(-2.0 * log(unit_interval(w[0], w[1]))), th = 6.283185307179586 * unit_interval(w[2], w[3]);
    z0 = rad * cos(th);
    z1 = rad * sin(th);
}

__global__ __launch_bounds__(MD_BLOCK) void md_step_kernel(
    const double* __restrict__ forces, const double* __restrict__ energy, int64_t n_rows, const int32_t* __restrict__ atom_ptr,
    const double* __restrict__ masses, const double* __restrict__ inv_lattice, double* __restrict__ mom, double* __restrict__ pos,
    double* __restrict__ frac, double* __restrict__ vel, double* __restrict__ rnd_vel, const double* __restrict__ t0_kelvin,
    const uint64_t* __restrict__ seeds, double* __restrict__ epot, double* __restrict__ ekin, double* __restrict__ temperature,
    double* __restrict__ traj_pos, double* __restrict__ traj_mom, double* __restrict__ noise_out, int32_t* __restrict__ status,
    int t, int interval, int steps, int ensemble, double dt, double friction, double taut, int fixcm, double kB) {
    __shared__ double sh[6][MD_WAVES];
    const int s = blockIdx.x, B = gridDim.x;
    if (atom_ptr[B] != n_rows) {  // forces of another shape than the batch: touch nothing
        if (threadIdx.x == 0) status[0] = -1;
        return;
    }
    const int beg = atom_ptr[s], n = atom_ptr[s + 1] - beg;
    const double* F = forces + 3 * (int64_t)beg;
    const double* M = masses + beg;
    double* P = mom + 3 * (int64_t)beg;
    double* R = pos + 3 * (int64_t)beg;
    const bool langevin = ensemble == MD_LANGEVIN;
    double* V = langevin ? vel + 3 * (int64_t)beg : nullptr;
    double* RV = langevin ? rnd_vel + 3 * (int64_t)beg : nullptr;
    const double half_dt = 0.5 * dt;
    const double c1 = dt / 2.0 - dt * dt * friction / 8.0;
    const double c2 = dt * friction / 2.0 - dt * dt * friction * friction / 8.0;

    // 1. + 2.
    const bool record = t % interval == 0;
    const int64_t frame = t / interval;
    double* TP = (record && traj_pos) ? traj_pos + 3 * (frame * n_rows + beg) : nullptr;
    double* TM = (record && traj_mom) ? traj_mom + 3 * (frame * n_rows + beg) : nullptr;
    double ke[1] = {0.0};
    for (int i = threadIdx.x; i < n; i += MD_BLOCK) {
        const double m = M[i];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const int k = 3 * i + c;
            double p = P[k];
            if (t > 0) {
                if (langevin) {
                    double v = V[k];
                    v += c1 * F[k] / m - c2 * v + RV[k];
                    p = v * m;
                } else {
                    p += half_dt * F[k];
                }
                P[k] = p;
            }
            ke[0] += p * p / m;
            if (TM) TM[k] = p;
            if (TP) TP[k] = R[k];
        }
    }
    block_reduce<1, false>(ke, sh);
    const double KE = 0.5 * ke[0];
    const double T = 2.0 * KE / (3.0 * n * kB);
    if (record && threadIdx.x == 0) {
        epot[frame * B + s] = energy[s];
        ekin[frame * B + s] = KE;
        temperature[frame * B + s] = T;
    }
    if (t >= steps) return;

    // 3.
    const double* L = inv_lattice + 9 * (int64_t)s;
    double* FR = frac + 3 * (int64_t)beg;
    auto drift_to = [&](int i, const double (&r)[3]) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            R[3 * i + c] = r[c];
            FR[3 * i + c] = wrap01(r[0] * L[c] + r[1] * L[3 + c] + r[2] * L[6 + c]);
        }
    };
    if (ensemble == MD_NVE) {
        for (int i = threadIdx.x; i < n; i += MD_BLOCK) {
            const double m = M[i];
            double r[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const double p = P[3 * i + c] + half_dt * F[3 * i + c];
                P[3 * i + c] = p;
                r[c] = R[3 * i + c] + dt * p / m;
            }
            drift_to(i, r);
        }
    } else if (ensemble == MD_BERENDSEN) {
        // T == 0: T0 / T is +inf (or NaN for T0 == 0), the scale clips to 1.1.  taut >= dt (checked by the host) keeps the
        // radicand >= 0.
        double scl = 1.1;
        if (T > 0.0) scl = fmin(fmax(sqrt(1.0 + (t0_kelvin[s] / T - 1.0) * dt / taut), 0.9), 1.1);
        double psum[3] = {0.0, 0.0, 0.0};
        for (int i = threadIdx.x; i < n; i += MD_BLOCK) {
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const double p = scl * P[3 * i + c] + half_dt * F[3 * i + c];
                P[3 * i + c] = p;
                psum[c] += p;
            }
        }
        if (fixcm) {
            block_reduce<3, false>(psum, sh);
#pragma unroll
            for (int c = 0; c < 3; ++c) psum[c] /= (double)n;  // a plain mean of the momenta, as ASE takes it
        }
        for (int i = threadIdx.x; i < n; i += MD_BLOCK) {
            const double m = M[i];
            double r[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                double p = P[3 * i + c];
                if (fixcm) {
                    p -= psum[c];
                    P[3 * i + c] = p;
                }
                r[c] = R[3 * i + c] + dt * p / m;
            }
            drift_to(i, r);
        }
    } else {  // Langevin: the noise of the step (rnd_pos parked in V until the second pass), then the first half and the drift
        const double Tev = kB * t0_kelvin[s];
        const double sqdt = sqrt(dt), dt15 = pow(dt, 1.5);
        const uint64_t seed = seeds[s];
        const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
        double sums[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};  // sum rnd_pos, sum m rnd_vel
        for (int i = threadIdx.x; i < n; i += MD_BLOCK) {
            const double m = M[i];
            const double sigma = sqrt(2.0 * Tev * friction / m);
            const double c3 = sqdt * sigma / 2.0 - dt15 * friction * sigma / 8.0;
            const double c5 = dt15 * sigma / (2.0 * 1.7320508075688772);
            const double c4 = friction / 2.0 * c5;
            double g[6];
            uint32_t w[3][4];
#pragma unroll
            for (int j = 0; j < 3; ++j) normal_pair(i, t, j, PURPOSE_LANGEVIN, k0, k1, g[2 * j], g[2 * j + 1], w[j]);
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const double xi = g[c], eta = g[3 + c];
                const double rp = c5 * eta, rv = c3 * xi - c4 * eta;
                V[3 * i + c] = rp;
                RV[3 * i + c] = rv;
                sums[c] += rp;
                sums[3 + c] += rv * m;
            }
            if (noise_out) {  // (tests only)
                double* o = noise_out + 18 * ((int64_t)beg + i);
#pragma unroll
                for (int c = 0; c < 6; ++c) o[c] = g[c];
#pragma unroll
                for (int j = 0; j < 3; ++j)
#pragma unroll
                    for (int c = 0; c < 4; ++c) o[6 + 4 * j + c] = (double)w[j][c];
            }
        }
        if (fixcm) {
            block_reduce<6, false>(sums, sh);
        } else {
#pragma unroll
            for (int c = 0; c < 6; ++c) sums[c] = 0.0;
        }
        for (int i = threadIdx.x; i < n; i += MD_BLOCK) {
            const double m = M[i];
            double r[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const int k = 3 * i + c;
                const double rp = V[k] - sums[c] / n;
                const double rv = RV[k] - sums[3 + c] / (m * n);
                double v = P[k] / m;
                v += c1 * F[k] / m - c2 * v + rv;
                const double x = R[k];
                r[c] = x + dt * v + rp;
                V[k] = (r[c] - x - rp) / dt;  // as ASE recomputes it after setting the positions
                RV[k] = rv;
            }
            drift_to(i, r);
        }
    }
}

// det and inverse of a row-major 3 x 3 matrix by cofactors
__device__ __forceinline__ double inverse3(const double (&a)[9], double (&inv)[9]) {
    const double c00 = a[4] * a[8] - a[5] * a[7], c01 = a[3] * a[8] - a[5] * a[6], c02 = a[3] * a[7] - a[4] * a[6];
    const double det = a[0] * c00 - a[1] * c01 + a[2] * c02;
    inv[0] = c00 / det;
    inv[1] = (a[2] * a[7] - a[1] * a[8]) / det;
    inv[2] = (a[1] * a[5] - a[2] * a[4]) / det;
    inv[3] = -c01 / det;
    inv[4] = (a[0] * a[8] - a[2] * a[6]) / det;
    inv[5] = (a[2] * a[3] - a[0] * a[5]) / det;
    inv[6] = c02 / det;
    inv[7] = (a[1] * a[6] - a[0] * a[7]) / det;
    inv[8] = (a[0] * a[4] - a[1] * a[3]) / det;
    return det;
}

// Andersen NVT (ensemble 3) and Berendsen NPT (ensemble 4): the header comment
__global__ __launch_bounds__(MD_BLOCK) void md_step_cell_kernel(
    const double* __restrict__ forces, const double* __restrict__ energy, const double* __restrict__ stress, int64_t n_rows,
    const int32_t* __restrict__ atom_ptr, const double* __restrict__ masses, double* __restrict__ lattice,
    double* __restrict__ inv_lattice, double* __restrict__ mom, double* __restrict__ pos, double* __restrict__ frac,
    double* __restrict__ vel, double* __restrict__ pos_old, const double* __restrict__ t0_kelvin,
    const uint64_t* __restrict__ seeds, const double* __restrict__ pressure, const double* __restrict__ compressibility,
    double* __restrict__ epot, double* __restrict__ ekin, double* __restrict__ temperature, double* __restrict__ pressure_out,
    double* __restrict__ volume_out, double* __restrict__ traj_pos, double* __restrict__ traj_mom,
    double* __restrict__ traj_lattice, double* __restrict__ noise_out, int32_t* __restrict__ status, int t, int interval,
    int steps, int ensemble, double dt, double andersen_prob, double taut, double taup, int fixcm, double kB) {
    __shared__ double sh[6][MD_WAVES];
    const int s = blockIdx.x, B = gridDim.x;
    if (atom_ptr[B] != n_rows) {  // forces of another shape than the batch: touch nothing
        if (threadIdx.x == 0) status[0] = -1;
        return;
    }
    const int beg = atom_ptr[s], n = atom_ptr[s + 1] - beg;
    const double* F = forces + 3 * (int64_t)beg;
    const double* M = masses + beg;
    double* P = mom + 3 * (int64_t)beg;
    double* R = pos + 3 * (int64_t)beg;
    double* FR = frac + 3 * (int64_t)beg;
    const bool andersen = ensemble == MD_ANDERSEN;
    double* V = andersen ? vel + 3 * (int64_t)beg : nullptr;
    double* X = andersen ? pos_old + 3 * (int64_t)beg : nullptr;
    const double half_dt = 0.5 * dt;
    // the cell of the current state, read by every thread before the first barrier: thread 0 rewrites it further down
    double C[9], Ci[9];
#pragma unroll
    for (int c = 0; c < 9; ++c) {
        C[c] = lattice[9 * (int64_t)s + c];
        Ci[c] = inv_lattice[9 * (int64_t)s + c];
    }

    // 1. + 2.
    const bool record = t % interval == 0;
    const int64_t frame = t / interval;
    double* TP = (record && traj_pos) ? traj_pos + 3 * (frame * n_rows + beg) : nullptr;
    double* TM = (record && traj_mom) ? traj_mom + 3 * (frame * n_rows + beg) : nullptr;
    double ke[1] = {0.0};
    for (int i = threadIdx.x; i < n; i += MD_BLOCK) {
        const double m = M[i];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const int k = 3 * i + c;
            double p = P[k];
            if (t > 0) {
                if (andersen)
                    p = m * (V[k] + 0.5 * F[k] / m * dt);
                else
                    p += half_dt * F[k];
                P[k] = p;
            }
            ke[0] += p * p / m;
            if (TM) TM[k] = p;
            if (TP) TP[k] = R[k];
        }
    }
    block_reduce<1, false>(ke, sh);
    const double KE = 0.5 * ke[0];
    const double T = 2.0 * KE / (3.0 * n * kB);
    double tmp[9];
    const double volume = fabs(inverse3(C, tmp));
    const double* S = stress ? stress + 9 * (int64_t)s : nullptr;
    const double virial = S ? -(S[0] + S[4] + S[8]) / 3.0 : 0.0;
    if (record && threadIdx.x == 0) {
        epot[frame * B + s] = energy[s];
        ekin[frame * B + s] = KE;
        temperature[frame * B + s] = T;
        if (pressure_out && S) pressure_out[frame * B + s] = virial + 2.0 * KE / (3.0 * volume);
        if (volume_out) volume_out[frame * B + s] = volume;
        if (traj_lattice)
#pragma unroll
            for (int c = 0; c < 9; ++c) traj_lattice[9 * (frame * B + s) + c] = C[c];
    }
    if (t >= steps) return;

    // 3.
    if (!andersen) {
        double scl = 1.1;  // (as md_step_kernel's Berendsen branch)
        if (T > 0.0) scl = fmin(fmax(sqrt(1.0 + (t0_kelvin[s] / T - 1.0) * dt / taut), 0.9), 1.1);
        // the kinetic energy of the scaled momenta, summed as the frame's
        ke[0] = 0.0;
        for (int i = threadIdx.x; i < n; i += MD_BLOCK) {
            const double m = M[i];
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const double p = scl * P[3 * i + c];
                P[3 * i + c] = p;
                ke[0] += p * p / m;
            }
        }
        block_reduce<1, false>(ke, sh);
        const double p_now = virial + 2.0 * (0.5 * ke[0]) / (3.0 * volume);  // with the ideal-gas term
        const double mu = 1.0 - dt / taup * compressibility[s] / 3.0 * (pressure[s] - p_now);
#pragma unroll
        for (int c = 0; c < 9; ++c) C[c] = mu * C[c];
        inverse3(C, Ci);
        if (threadIdx.x == 0) {
#pragma unroll
            for (int c = 0; c < 9; ++c) {
                lattice[9 * (int64_t)s + c] = C[c];
                inv_lattice[9 * (int64_t)s + c] = Ci[c];
            }
        }
        double psum[3] = {0.0, 0.0, 0.0};
        for (int i = threadIdx.x; i < n; i += MD_BLOCK) {
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const double p = P[3 * i + c] + half_dt * F[3 * i + c];
                P[3 * i + c] = p;
                psum[c] += p;
            }
        }
        if (fixcm) {
            block_reduce<3, false>(psum, sh);
#pragma unroll
            for (int c = 0; c < 3; ++c) psum[c] /= (double)n;
        }
        for (int i = threadIdx.x; i < n; i += MD_BLOCK) {
            const double m = M[i];
            double r[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                double p = P[3 * i + c];
                if (fixcm) {
                    p -= psum[c];
                    P[3 * i + c] = p;
                }
                r[c] = mu * R[3 * i + c] + dt * p / m;
            }
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                R[3 * i + c] = r[c];
                FR[3 * i + c] = wrap01(r[0] * Ci[c] + r[1] * Ci[3 + c] + r[2] * Ci[6 + c]);
            }
        }
        return;
    }

    // Andersen
    const double Tev = kB * t0_kelvin[s];
    const uint64_t seed = seeds[s];
    const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
    double vcom[3] = {0.0, 0.0, 0.0};
    double msum[1] = {0.0};
    if (fixcm) {
        for (int i = threadIdx.x; i < n; i += MD_BLOCK) msum[0] += M[i];
        block_reduce<1, false>(msum, sh);
        double g[4];
        uint32_t w[2][4];
        normal_pair(0, t, 0, PURPOSE_ANDERSEN_COM, k0, k1, g[0], g[1], w[0]);
        normal_pair(0, t, 1, PURPOSE_ANDERSEN_COM, k0, k1, g[2], g[3], w[1]);
        const double width = sqrt(Tev / msum[0]);
#pragma unroll
        for (int c = 0; c < 3; ++c) vcom[c] = g[c] * width;
        if (noise_out) {  // (tests only)
            for (int i = threadIdx.x; i < n; i += MD_BLOCK) {
                double* o = noise_out + 36 * ((int64_t)beg + i) + 24;
#pragma unroll
                for (int c = 0; c < 4; ++c) o[c] = g[c];
#pragma unroll
                for (int c = 0; c < 8; ++c) o[4 + c] = (double)w[c / 4][c % 4];
            }
        }
    }
    double sums[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};  // sum m x, sum m v
    for (int i = threadIdx.x; i < n; i += MD_BLOCK) {
        const double m = M[i];
        const double width = sqrt(Tev / m);
        double g[4], u[4];
        uint32_t w[4][4];
        normal_pair(i, t, 0, PURPOSE_ANDERSEN, k0, k1, g[0], g[1], w[0]);
        normal_pair(i, t, 1, PURPOSE_ANDERSEN, k0, k1, g[2], g[3], w[1]);
#pragma unroll
        for (int j = 2; j < 4; ++j) {
            w[j][0] = i;
            w[j][1] = t;
            w[j][2] = j;
            w[j][3] = PURPOSE_ANDERSEN;
            philox4x32_10(w[j], k0, k1);
            u[2 * (j - 2)] = unit_interval(w[j][0], w[j][1]);
            u[2 * (j - 2) + 1] = unit_interval(w[j][2], w[j][3]);
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const int k = 3 * i + c;
            double v = P[k] / m;
            if (fixcm) v += vcom[c];
            v += 0.5 * F[k] / m * dt;
            if (u[c] <= andersen_prob) v = g[c] * width;
            const double x = R[k];
            V[k] = v;
            X[k] = x;
            sums[c] += m * x;
            sums[3 + c] += m * v;
        }
        if (noise_out) {  // (tests only)
            double* o = noise_out + 36 * ((int64_t)beg + i);
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                o[c] = g[c];
                o[4 + c] = u[c];
            }
#pragma unroll
            for (int c = 0; c < 16; ++c) o[8 + c] = (double)w[c / 4][c % 4];
        }
    }
    double shift[3] = {0.0, 0.0, 0.0};
    if (fixcm) {  // the mass-weighted mean velocity out; the centre of mass stays where it was through the drift
        block_reduce<6, false>(sums, sh);
        double rsum[3] = {0.0, 0.0, 0.0};
        for (int i = threadIdx.x; i < n; i += MD_BLOCK) {
            const double m = M[i];
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const int k = 3 * i + c;
                const double v = V[k] - sums[3 + c] / msum[0];
                const double r = X[k] + v * dt;
                V[k] = v;
                R[k] = r;
                rsum[c] += m * r;
            }
        }
        block_reduce<3, false>(rsum, sh);
#pragma unroll
        for (int c = 0; c < 3; ++c) shift[c] = sums[c] / msum[0] - rsum[c] / msum[0];
    }
    for (int i = threadIdx.x; i < n; i += MD_BLOCK) {
        double r[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const int k = 3 * i + c;
            const double x = X[k];
            r[c] = fixcm ? R[k] + shift[c] : x + V[k] * dt;
            V[k] = (r[c] - x) / dt;  // as ASE recomputes it after setting the positions
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            R[3 * i + c] = r[c];
            FR[3 * i + c] = wrap01(r[0] * Ci[c] + r[1] * Ci[3 + c] + r[2] * Ci[6 + c]);
        }
    }
}

__global__ __launch_bounds__(MD_BLOCK) void md_init_momenta_kernel(const int32_t* __restrict__ atom_ptr,
                                                                  const double* __restrict__ masses,
                                                                  const double* __restrict__ t_kelvin,
                                                                  const uint64_t* __restrict__ seeds, double* __restrict__ mom,
                                                                  double kB) {
    const int s = blockIdx.x;
    const int beg = atom_ptr[s], n = atom_ptr[s + 1] - beg;
    const double temp = kB * t_kelvin[s];
    const uint64_t seed = seeds[s];
    const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
    for (int i = threadIdx.x; i < n; i += MD_BLOCK) {
        double g[4];
        uint32_t w[4];
        normal_pair(i, 0, 0, PURPOSE_MOMENTA, k0, k1, g[0], g[1], w);
        normal_pair(i, 0, 1, PURPOSE_MOMENTA, k0, k1, g[2], g[3], w);
        const double sc = sqrt(masses[beg + i] * temp);
#pragma unroll
        for (int c = 0; c < 3; ++c) mom[3 * ((int64_t)beg + i) + c] = g[c] * sc;
    }
}

}  // namespace

extern "C" int alignn_md_step(const double* forces, const double* energy, int64_t n_rows, const int32_t* atom_ptr,
                              int n_structures, const double* masses, const double* inv_lattice, double* momenta,
                              double* positions, double* frac, double* velocities, double* rnd_vel, const double* t0_kelvin,
                              const uint64_t* seeds, double* epot, double* ekin, double* temperature, double* traj_positions,
                              double* traj_momenta, double* noise_out, int32_t* status, int t, int interval, int steps,
                              int ensemble, double dt, double friction, double taut, int fixcm, double kB,
                              alignn_stream_t stream) {
    if (n_structures < 1 || !status || !epot || !ekin || !temperature || interval < 1 || t < 0 || t > steps ||
        ensemble < MD_NVE || ensemble > MD_BERENDSEN)
        return (int)hipErrorInvalidValue;
    if (ensemble == MD_LANGEVIN && (!velocities || !rnd_vel || !seeds)) return (int)hipErrorInvalidValue;
    if (ensemble != MD_NVE && !t0_kelvin) return (int)hipErrorInvalidValue;
    md_step_kernel<<<n_structures, MD_BLOCK, 0, (hipStream_t)stream>>>(
        forces, energy, n_rows, atom_ptr, masses, inv_lattice, momenta, positions, frac, velocities, rnd_vel, t0_kelvin, seeds,
        epot, ekin, temperature, traj_positions, traj_momenta, noise_out, status, t, interval, steps, ensemble, dt, friction, taut,
        fixcm, kB);
    ALIGNN_CHECK_LAUNCH();
    return 0;
}

extern "C" int alignn_md_step_cell(const double* forces, const double* energy, const double* stress, int64_t n_rows,
                                   const int32_t* atom_ptr, int n_structures, const double* masses, double* lattice,
                                   double* inv_lattice, double* momenta, double* positions, double* frac, double* velocities,
                                   double* rnd_vel, const double* t0_kelvin, const uint64_t* seeds, const double* pressure,
                                   const double* compressibility, double* epot, double* ekin, double* temperature,
                                   double* pressure_out, double* volume_out, double* traj_positions, double* traj_momenta,
                                   double* traj_lattice, double* noise_out, int32_t* status, int t, int interval, int steps,
                                   int ensemble, double dt, double andersen_prob, double taut, double taup, int fixcm, double kB,
                                   alignn_stream_t stream) {
    if (n_structures < 1 || !status || !epot || !ekin || !temperature || !lattice || !inv_lattice || !t0_kelvin || interval < 1 ||
        t < 0 || t > steps || (ensemble != MD_ANDERSEN && ensemble != MD_NPT_BERENDSEN))
        return (int)hipErrorInvalidValue;
    if (ensemble == MD_ANDERSEN && (!velocities || !rnd_vel || !seeds)) return (int)hipErrorInvalidValue;
    if (ensemble == MD_NPT_BERENDSEN && (!stress || !pressure || !compressibility)) return (int)hipErrorInvalidValue;
    md_step_cell_kernel<<<n_structures, MD_BLOCK, 0, (hipStream_t)stream>>>(
        forces, energy, stress, n_rows, atom_ptr, masses, lattice, inv_lattice, momenta, positions, frac, velocities, rnd_vel,
        t0_kelvin, seeds, pressure, compressibility, epot, ekin, temperature, pressure_out, volume_out, traj_positions, traj_momenta,
        traj_lattice, noise_out, status, t, interval, steps, ensemble, dt, andersen_prob, taut, taup, fixcm, kB);
    ALIGNN_CHECK_LAUNCH();
    return 0;
}

extern "C" int alignn_md_init_momenta(const int32_t* atom_ptr, int n_structures, const double* masses, const double* t_kelvin,
                                      const uint64_t* seeds, double* momenta, double kB, alignn_stream_t stream) {
    if (n_structures < 1) return (int)hipErrorInvalidValue;
    md_init_momenta_kernel<<<n_structures, MD_BLOCK, 0, (hipStream_t)stream>>>(atom_ptr, masses, t_kelvin, seeds, momenta, kB);
    ALIGNN_CHECK_LAUNCH();
    return 0;
}
