// Batched molecular dynamics: ASE 3.22.1's VelocityVerlet, Langevin, NVTBerendsen, Andersen and NPTBerendsen (ase/md/*.py) as
// the reference's ForceField.run_nve_velocity_verlet / run_nvt_langevin / run_nvt_berendsen / run_nvt_andersen /
// run_npt_berendsen drive them (alignn/ff/ff.py:419-600), every structure's integrator state on the device
// (alignn_amd/dynamics.py is the host loop; tests/md_ref.py and tests/md_npt_ref.py the numpy restatements this file
// follows).  One kernel, md_step_kernel<ENS>, instantiated per ensemble 0-6 on the argument block alignn_md_args
// (include/alignn_hip.h names every field); what the ensembles share is written once, what differs sits under if constexpr.
//
// Iteration t of the host loop evaluates the forces F_t at r_t; one md_step_kernel launch then
//   1. finishes step t (t > 0): the second half-kick with F_t (Langevin: v += c1 F/m - c2 v + rnd_vel, p = v m; Andersen:
//      p = m (v + F/m dt/2));
//   2. records frame t / interval when t % interval == 0: E_pot, KE, T, the trajectory rows and, for Andersen and NPT, the
//      pressure P = -tr(S_t) / 3 + 2 KE / (3 V), V = |det cell| and the cell;
//   3. begins step t + 1 (t < steps): the first half-kick and the drift (Berendsen: the velocity scaling first; Langevin and
//      Andersen: the random numbers of this step), the wrapped fractional coordinates of r_{t+1} for the next neighbour search.
// One workgroup per structure, threads grid-strided over its atoms, float64 throughout.  Every sum (KE, the Berendsen
// momentum sum, the fixcm sums) goes through the fixed-order block_reduce: a structure's trajectory is the same bits whether it
// runs alone or beside others.
//
// Random numbers: Philox4x32-10, key (seed & 0xffffffff, seed >> 32), counter (atom i within the structure, t, block j,
// purpose).  A block's words (w0, w1, w2, w3) give u1 = unit(w0, w1), u2 = unit(w2, w3) and the two normals
// sqrt(-2 ln u1) (cos, sin)(2 pi u2).  Langevin (purpose 0) takes blocks j = 0, 1, 2 at counter t = the iteration that
// begins the step: normals g0..g5 in block order, cos before sin; xi = (g0, g1, g2), eta = (g3, g4, g5).  The initial
// Maxwell-Boltzmann momenta (purpose 1) take blocks 0 and 1 at t = 0: xi = (g0, g1, g2).  Andersen (purpose 2) takes blocks
// j = 0 .. 3 of counter (atom, t, j, 2): blocks 0, 1 give the normals g0..g3 (replacement velocity = (g0, g1, g2) sqrt(kB T0 / m)),
// blocks 2, 3 the uniforms u0 = unit(w0, w1), u1 = unit(w2, w3) of block 2 and u2, u3 of block 3; component c is replaced when
// u_c <= andersen_prob (unit() lies in (0, 1]: probability 0 never replaces, 1 always).  Its centre-of-mass velocity (purpose 3)
// takes blocks j = 0, 1 of counter (0, t, j, 3): (g0, g1, g2) sqrt(kB T0 / sum m).
//
// NPT Berendsen begins a step with NVTBerendsen's velocity scaling, then the pressure of the scaled momenta and the
// evaluation's stress S_t, the factor mu = 1 - (dt / taup) compressibility / 3 (P_target - P), cell and positions times mu
// (every thread computes mu, the new cell and its inverse by cofactors alike; thread 0 writes them), then NVTBerendsen's
// half-kick, fixcm and drift; frac uses the new inverse.  Andersen keeps v between the halves (velocities) and the positions
// before the drift (scratch).
//
// Ensembles 5 and 6 are not ASE's: Nose-Hoover chain NVT and the isotropic MTK NPT in the explicit reversible form of Martyna,
// Tuckerman, Tobias and Klein (Mol. Phys. 87, 1117, 1996), the barostat measure-preserving (Tuckerman et al., J. Phys. A 39,
// 5629, 2006); tests/md_nose_hoover_ref.py is the restatement.  Per structure kT = kB T0, g = 3N, Q_0 = g kT ttime^2,
// Q_k = kT ttime^2, W = (g + 3) kT ptime^2, the barostat's own chain Q'_k = kT ptime^2 (one degree of freedom), alpha = 1 + 3 / g.
// A step is: chains dt/2 (barostat's, then the particles'), v_eps += dt/2 G_eps, half-kick, drift (cell and positions times
// exp(v_eps dt)) | evaluate | half-kick, v_eps += dt/2 G_eps, chains dt/2 (particles', then barostat's); G_eps = (alpha sum
// p^2/m + 3 V (P_vir - P_ext)) / W.  The 34 doubles of a structure's chain state (nhc_state) are read by every thread before the
// first reduction's barrier; every lane runs the scalar chain from the reduced sum p^2/m (the same instructions, the same
// bits) and thread 0 writes the state back at the end.  ttime <= 0 / ptime <= 0 switch a part off; both off is velocity Verlet
// in the expressions of ensemble 0.  fixcm takes the centre-of-mass velocity out once, at t = 0.
#include "../../include/alignn_hip.h"
#include "common.h"

namespace {

constexpr int MD_BLOCK = 256;
constexpr int MD_WAVES = MD_BLOCK / ALIGNN_WAVE;
constexpr int NHC_MAX = 8, NHC_STATE = 4 * NHC_MAX + 2;  // eta[8], v[8], eta'[8], v'[8], eps, v_eps
enum {
    MD_NVE = 0,
    MD_LANGEVIN = 1,
    MD_BERENDSEN = 2,
    MD_ANDERSEN = 3,
    MD_NPT_BERENDSEN = 4,
    MD_NVT_NOSE_HOOVER = 5,
    MD_NPT_NOSE_HOOVER = 6
};
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

// the four words of Philox block (i, t, j, purpose)
__device__ __forceinline__ void philox_block(uint32_t i, uint32_t t, uint32_t j, uint32_t purpose, uint32_t k0, uint32_t k1,
                                             uint32_t (&w)[4]) {
    w[0] = i;
    w[1] = t;
    w[2] = j;
    w[3] = purpose;
    philox4x32_10(w, k0, k1);
}

// the two Box-Muller normals of that block; w returns its four words
__device__ __forceinline__ void normal_pair(uint32_t i, uint32_t t, uint32_t j, uint32_t purpose, uint32_t k0, uint32_t k1,
                                            double& z0, double& z1, uint32_t (&w)[4]) {
    philox_block(i, t, j, purpose, k0, k1, w);
    const double rad = sqrt(-2.0 * log(unit_interval(w[0], w[1]))), th = 6.283185307179586 * unit_interval(w[2], w[3]);
    z0 = rad * cos(th);
    z1 = rad * sin(th);
}

// its two uniforms in (0, 1]
__device__ __forceinline__ void uniform_pair(uint32_t i, uint32_t t, uint32_t j, uint32_t purpose, uint32_t k0, uint32_t k1,
                                             double& u0, double& u1, uint32_t (&w)[4]) {
    philox_block(i, t, j, purpose, k0, k1, w);
    u0 = unit_interval(w[0], w[1]);
    u1 = unit_interval(w[2], w[3]);
}

using MdArgs = alignn_md_args;
using MdShared = double (*)[MD_WAVES];

// the ensembles that read the cell and record pressure, volume and cell; those that keep velocities and scratch between the halves
constexpr bool md_has_cell(int ens) { return ens == MD_ANDERSEN || ens == MD_NPT_BERENDSEN || ens == MD_NPT_NOSE_HOOVER; }
constexpr bool md_is_nose_hoover(int ens) { return ens == MD_NVT_NOSE_HOOVER || ens == MD_NPT_NOSE_HOOVER; }
constexpr bool md_keeps_velocity(int ens) { return ens == MD_LANGEVIN || ens == MD_ANDERSEN; }

// What structure s owns: its rows of the per-atom arrays (V, W: velocities and scratch, for the ensembles that keep them) and
// its cell as every thread reads it before the first barrier (C: the ensembles with a cell only; NPT's thread 0 rewrites both
// further down).
struct MdView {
    int s, beg, n;
    const double *F, *M;
    double *P, *R, *FR, *V, *W;
    double C[9], Ci[9];
};

template <int ENS>
__device__ __forceinline__ MdView md_view(const MdArgs& a, int s) {
    MdView w;
    w.s = s;
    w.beg = a.atom_ptr[s];
    w.n = a.atom_ptr[s + 1] - w.beg;
    const int64_t row = 3 * (int64_t)w.beg;
    w.F = a.forces + row;
    w.M = a.masses + w.beg;
    w.P = a.momenta + row;
    w.R = a.positions + row;
    w.FR = a.frac + row;
    w.V = md_keeps_velocity(ENS) ? a.velocities + row : nullptr;
    w.W = md_keeps_velocity(ENS) ? a.scratch + row : nullptr;
#pragma unroll
    for (int c = 0; c < 9; ++c) {
        w.C[c] = md_has_cell(ENS) ? a.lattice[9 * (int64_t)s + c] : 0.0;
        w.Ci[c] = a.inv_lattice[9 * (int64_t)s + c];
    }
    return w;
}

// 1. + 2.: the second half of step t (t > 0) and the frame's trajectory rows; returns the kinetic energy of the finished state
template <int ENS>
__device__ __forceinline__ double md_finish(const MdArgs& a, const MdView& w, bool record, int64_t frame, MdShared sh) {
    const int t = a.t;
    const double dt = a.dt, half_dt = 0.5 * dt, friction = a.friction;
    const double c1 = dt / 2.0 - dt * dt * friction / 8.0;
    const double c2 = dt * friction / 2.0 - dt * dt * friction * friction / 8.0;
    double* TP = (record && a.traj_positions) ? a.traj_positions + 3 * (frame * a.n_rows + w.beg) : nullptr;
    double* TM = (record && a.traj_momenta) ? a.traj_momenta + 3 * (frame * a.n_rows + w.beg) : nullptr;
    double ke[1] = {0.0};
    for (int i = threadIdx.x; i < w.n; i += MD_BLOCK) {
        const double m = w.M[i];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const int k = 3 * i + c;
            double p = w.P[k];
            if (t > 0) {
                if constexpr (ENS == MD_LANGEVIN) {
                    double v = w.V[k];
                    v += c1 * w.F[k] / m - c2 * v + w.W[k];
                    p = v * m;
                } else if constexpr (ENS == MD_ANDERSEN) {
                    p = m * (w.V[k] + 0.5 * w.F[k] / m * dt);
                } else {
                    p += half_dt * w.F[k];
                }
                w.P[k] = p;
            }
            ke[0] += p * p / m;
            if (TM) TM[k] = p;
            if (TP) TP[k] = w.R[k];
        }
    }
    block_reduce<1, false>(ke, sh);
    return 0.5 * ke[0];
}

// 2.: the frame's scalars (thread 0); pressure, volume and cell where the ensemble has a cell and the block those outputs
template <int ENS>
__device__ __forceinline__ void md_record(const MdArgs& a, const MdView& w, int64_t frame, double KE, double T, double virial,
                                          double volume) {
    const int64_t f = frame * gridDim.x + w.s;
    a.epot[f] = a.energy[w.s];
    a.ekin[f] = KE;
    a.temperature[f] = T;
    if constexpr (md_has_cell(ENS)) {
        if (a.pressure_out && a.stress) a.pressure_out[f] = virial + 2.0 * KE / (3.0 * volume);
        if (a.volume_out) a.volume_out[f] = volume;
        if (a.traj_lattice)
#pragma unroll
            for (int c = 0; c < 9; ++c) a.traj_lattice[9 * f + c] = w.C[c];
    }
}

// atom i to r, its fractional coordinates r Ci wrapped into [0, 1)
__device__ __forceinline__ void md_drift_to(const MdView& w, const double (&Ci)[9], int i, const double (&r)[3]) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        w.R[3 * i + c] = r[c];
        w.FR[3 * i + c] = wrap01(r[0] * Ci[c] + r[1] * Ci[3 + c] + r[2] * Ci[6 + c]);
    }
}

__device__ __forceinline__ void md_begin_verlet(const MdArgs& a, const MdView& w) {
    const double dt = a.dt, half_dt = 0.5 * dt;
    for (int i = threadIdx.x; i < w.n; i += MD_BLOCK) {
        const double m = w.M[i];
        double r[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const double p = w.P[3 * i + c] + half_dt * w.F[3 * i + c];
            w.P[3 * i + c] = p;
            r[c] = w.R[3 * i + c] + dt * p / m;
        }
        md_drift_to(w, w.Ci, i, r);
    }
}

// NVTBerendsen (mu = 1, the inverse cell as it is) and NPTBerendsen.  The two round the scaled half-kick differently - NVT
// scl p + dt/2 F in one expression, NPT the scaled p stored (its kinetic energy enters mu), then the kick - and each keeps its own.
template <int ENS>
__device__ __forceinline__ void md_begin_berendsen(const MdArgs& a, const MdView& w, double T, double virial, double volume,
                                                   MdShared sh) {
    constexpr bool NPT = ENS == MD_NPT_BERENDSEN;
    const int s = w.s, n = w.n;
    const double dt = a.dt, half_dt = 0.5 * dt;
    // T == 0: T0 / T is +inf (or NaN for T0 == 0), the scale clips to 1.1.  taut >= dt (checked by the host) keeps the
    // radicand >= 0.
    double scl = 1.1;
    if (T > 0.0) scl = fmin(fmax(sqrt(1.0 + (a.t0_kelvin[s] / T - 1.0) * dt / a.taut), 0.9), 1.1);
    double mu = 1.0, Ci[9];
#pragma unroll
    for (int c = 0; c < 9; ++c) Ci[c] = w.Ci[c];
    if constexpr (NPT) {
        double ke[1] = {0.0};  // the kinetic energy of the scaled momenta, summed as the frame's
        for (int i = threadIdx.x; i < n; i += MD_BLOCK) {
            const double m = w.M[i];
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const double p = scl * w.P[3 * i + c];
                w.P[3 * i + c] = p;
                ke[0] += p * p / m;
            }
        }
        block_reduce<1, false>(ke, sh);
        const double p_now = virial + 2.0 * (0.5 * ke[0]) / (3.0 * volume);  // with the ideal-gas term
        mu = 1.0 - dt / a.taup * a.compressibility[s] / 3.0 * (a.pressure[s] - p_now);
        double C[9];
#pragma unroll
        for (int c = 0; c < 9; ++c) C[c] = mu * w.C[c];
        inverse3(C, Ci);
        if (threadIdx.x == 0) {
#pragma unroll
            for (int c = 0; c < 9; ++c) {
                a.lattice[9 * (int64_t)s + c] = C[c];
                a.inv_lattice[9 * (int64_t)s + c] = Ci[c];
            }
        }
    }
    double psum[3] = {0.0, 0.0, 0.0};
    for (int i = threadIdx.x; i < n; i += MD_BLOCK) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            double p;
            if constexpr (NPT)
                p = w.P[3 * i + c] + half_dt * w.F[3 * i + c];
            else
                p = scl * w.P[3 * i + c] + half_dt * w.F[3 * i + c];
            w.P[3 * i + c] = p;
            psum[c] += p;
        }
    }
    if (a.fixcm) {
        block_reduce<3, false>(psum, sh);
#pragma unroll
        for (int c = 0; c < 3; ++c) psum[c] /= (double)n;  // a plain mean of the momenta, as ASE takes it
    }
    for (int i = threadIdx.x; i < n; i += MD_BLOCK) {
        const double m = w.M[i];
        double r[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            double p = w.P[3 * i + c];
            if (a.fixcm) {
                p -= psum[c];
                w.P[3 * i + c] = p;
            }
            if constexpr (NPT)
                r[c] = mu * w.R[3 * i + c] + dt * p / m;
            else
                r[c] = w.R[3 * i + c] + dt * p / m;
        }
        md_drift_to(w, Ci, i, r);
    }
}

// Langevin: the noise of the step (rnd_pos parked in V until the second pass), then the first half and the drift
__device__ __forceinline__ void md_begin_langevin(const MdArgs& a, const MdView& w, MdShared sh) {
    const int n = w.n, t = a.t;
    const double dt = a.dt, friction = a.friction;
    const double c1 = dt / 2.0 - dt * dt * friction / 8.0;
    const double c2 = dt * friction / 2.0 - dt * dt * friction * friction / 8.0;
    const double Tev = a.kB * a.t0_kelvin[w.s];
    const double sqdt = sqrt(dt), dt15 = pow(dt, 1.5);
    const uint64_t seed = a.seeds[w.s];
    const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
    double sums[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};  // sum rnd_pos, sum m rnd_vel
    for (int i = threadIdx.x; i < n; i += MD_BLOCK) {
        const double m = w.M[i];
        const double sigma = sqrt(2.0 * Tev * friction / m);
        const double c3 = sqdt * sigma / 2.0 - dt15 * friction * sigma / 8.0;
        const double c5 = dt15 * sigma / (2.0 * 1.7320508075688772);
        const double c4 = friction / 2.0 * c5;
        double g[6];
        uint32_t wd[3][4];
#pragma unroll
        for (int j = 0; j < 3; ++j) normal_pair(i, t, j, PURPOSE_LANGEVIN, k0, k1, g[2 * j], g[2 * j + 1], wd[j]);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const double xi = g[c], eta = g[3 + c];
            const double rp = c5 * eta, rv = c3 * xi - c4 * eta;
            w.V[3 * i + c] = rp;
            w.W[3 * i + c] = rv;
            sums[c] += rp;
            sums[3 + c] += rv * m;
        }
        if (a.noise_out) {  // (tests only)
            double* o = a.noise_out + 18 * ((int64_t)w.beg + i);
#pragma unroll
            for (int c = 0; c < 6; ++c) o[c] = g[c];
#pragma unroll
            for (int j = 0; j < 3; ++j)
#pragma unroll
                for (int c = 0; c < 4; ++c) o[6 + 4 * j + c] = (double)wd[j][c];
        }
    }
    if (a.fixcm) {
        block_reduce<6, false>(sums, sh);
    } else {
#pragma unroll
        for (int c = 0; c < 6; ++c) sums[c] = 0.0;
    }
    for (int i = threadIdx.x; i < n; i += MD_BLOCK) {
        const double m = w.M[i];
        double r[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const int k = 3 * i + c;
            const double rp = w.V[k] - sums[c] / n;
            const double rv = w.W[k] - sums[3 + c] / (m * n);
            double v = w.P[k] / m;
            v += c1 * w.F[k] / m - c2 * v + rv;
            const double x = w.R[k];
            r[c] = x + dt * v + rp;
            w.V[k] = (r[c] - x - rp) / dt;  // as ASE recomputes it after setting the positions
            w.W[k] = rv;
        }
        md_drift_to(w, w.Ci, i, r);
    }
}

// Andersen: v = p / m (fixcm: + a random centre-of-mass velocity), the half-kick, the replacements, the drift (fixcm: about
// the centre of mass); the positions before the drift wait in W
__device__ __forceinline__ void md_begin_andersen(const MdArgs& a, const MdView& w, MdShared sh) {
    const int n = w.n, t = a.t, fixcm = a.fixcm;
    const double dt = a.dt;
    const double Tev = a.kB * a.t0_kelvin[w.s];
    const uint64_t seed = a.seeds[w.s];
    const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
    double vcom[3] = {0.0, 0.0, 0.0};
    double msum[1] = {0.0};
    if (fixcm) {
        for (int i = threadIdx.x; i < n; i += MD_BLOCK) msum[0] += w.M[i];
        block_reduce<1, false>(msum, sh);
        double g[4];
        uint32_t wd[2][4];
        normal_pair(0, t, 0, PURPOSE_ANDERSEN_COM, k0, k1, g[0], g[1], wd[0]);
        normal_pair(0, t, 1, PURPOSE_ANDERSEN_COM, k0, k1, g[2], g[3], wd[1]);
        const double width = sqrt(Tev / msum[0]);
#pragma unroll
        for (int c = 0; c < 3; ++c) vcom[c] = g[c] * width;
        if (a.noise_out) {  // (tests only)
            for (int i = threadIdx.x; i < n; i += MD_BLOCK) {
                double* o = a.noise_out + 36 * ((int64_t)w.beg + i) + 24;
#pragma unroll
                for (int c = 0; c < 4; ++c) o[c] = g[c];
#pragma unroll
                for (int c = 0; c < 8; ++c) o[4 + c] = (double)wd[c / 4][c % 4];
            }
        }
    }
    double sums[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};  // sum m x, sum m v
    for (int i = threadIdx.x; i < n; i += MD_BLOCK) {
        const double m = w.M[i];
        const double width = sqrt(Tev / m);
        double g[4], u[4];
        uint32_t wd[4][4];
        normal_pair(i, t, 0, PURPOSE_ANDERSEN, k0, k1, g[0], g[1], wd[0]);
        normal_pair(i, t, 1, PURPOSE_ANDERSEN, k0, k1, g[2], g[3], wd[1]);
        uniform_pair(i, t, 2, PURPOSE_ANDERSEN, k0, k1, u[0], u[1], wd[2]);
        uniform_pair(i, t, 3, PURPOSE_ANDERSEN, k0, k1, u[2], u[3], wd[3]);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const int k = 3 * i + c;
            double v = w.P[k] / m;
            if (fixcm) v += vcom[c];
            v += 0.5 * w.F[k] / m * dt;
            if (u[c] <= a.andersen_prob) v = g[c] * width;
            const double x = w.R[k];
            w.V[k] = v;
            w.W[k] = x;
            sums[c] += m * x;
            sums[3 + c] += m * v;
        }
        if (a.noise_out) {  // (tests only)
            double* o = a.noise_out + 36 * ((int64_t)w.beg + i);
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                o[c] = g[c];
                o[4 + c] = u[c];
            }
#pragma unroll
            for (int c = 0; c < 16; ++c) o[8 + c] = (double)wd[c / 4][c % 4];
        }
    }
    double shift[3] = {0.0, 0.0, 0.0};
    if (fixcm) {  // the mass-weighted mean velocity out; the centre of mass stays where it was through the drift
        block_reduce<6, false>(sums, sh);
        double rsum[3] = {0.0, 0.0, 0.0};
        for (int i = threadIdx.x; i < n; i += MD_BLOCK) {
            const double m = w.M[i];
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const int k = 3 * i + c;
                const double v = w.V[k] - sums[3 + c] / msum[0];
                const double r = w.W[k] + v * dt;
                w.V[k] = v;
                w.R[k] = r;
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
            const double x = w.W[k];
            r[c] = fixcm ? w.R[k] + shift[c] : x + w.V[k] * dt;
            w.V[k] = (r[c] - x) / dt;  // as ASE recomputes it after setting the positions
        }
        md_drift_to(w, w.Ci, i, r);
    }
}

// sinh(x) / x; the series below |x| = 1e-2 (its next term is x^10 / 39916800 < 3e-28)
__device__ __forceinline__ double sinhc(double x) {
    const double x2 = x * x;
    if (fabs(x) < 1e-2) return 1.0 + x2 / 6.0 + x2 * x2 / 120.0 + x2 * x2 * x2 / 5040.0 + x2 * x2 * x2 * x2 / 362880.0;
    return sinh(x) / x;
}

// A Nose-Hoover chain by dt / 2 (MTK 1996, eqs. 25-29): a.nhc_loops loops over the a.nhc_order Suzuki-Yoshida weights.  K2 is
// sum p^2 / m of what the chain thermostats, dof its degrees of freedom, Q0 / Qk the masses of link 0 / the others.  Returns the
// factor s on the thermostatted momenta.  The loops over the links are unrolled to NHC_MAX and predicated on a.chain, so v and
// eta stay in registers.
__device__ __forceinline__ double nhc_half(const MdArgs& a, double K2, double dof, double kT, double Q0, double Qk,
                                           double (&v)[NHC_MAX], double (&eta)[NHC_MAX]) {
    const int M = a.chain, order = a.nhc_order, loops = a.nhc_loops;
    // 1 / (2 - 2^(1/3)) and 1 / (4 - 4^(1/3)) with the cube roots as float64 literals
    const double wside = order == 3 ? 1.0 / (2.0 - 1.2599210498948732) : order == 5 ? 1.0 / (4.0 - 1.5874010519681994) : 1.0;
    const double wmid = 1.0 - (order - 1) * wside;
    double s = 1.0;
    auto G = [&](int k) {
        if (k == 0) return (K2 * s * s - dof * kT) / Q0;
        return ((k == 1 ? Q0 : Qk) * v[k - 1] * v[k - 1] - kT) / Qk;
    };
    for (int l = 0; l < loops; ++l) {
        for (int j = 0; j < order; ++j) {
            const double h = (2 * j + 1 == order ? wmid : wside) * (0.5 * a.dt) / loops;
#pragma unroll
            for (int k = 0; k < NHC_MAX; ++k)
                if (k == M - 1) v[k] += 0.5 * h * G(k);
#pragma unroll
            for (int k = NHC_MAX - 2; k >= 0; --k)
                if (k <= M - 2) {
                    const double e = exp(-0.25 * h * v[k + 1]);
                    v[k] *= e;
                    v[k] += 0.5 * h * G(k);
                    v[k] *= e;
                }
            s *= exp(-h * v[0]);
#pragma unroll
            for (int k = 0; k < NHC_MAX; ++k)
                if (k < M) eta[k] += h * v[k];
#pragma unroll
            for (int k = 0; k < NHC_MAX - 1; ++k)
                if (k <= M - 2) {
                    const double e = exp(-0.25 * h * v[k + 1]);
                    v[k] *= e;
                    v[k] += 0.5 * h * G(k);
                    v[k] *= e;
                }
#pragma unroll
            for (int k = 0; k < NHC_MAX; ++k)
                if (k == M - 1) v[k] += 0.5 * h * G(k);
        }
    }
    return s;
}

// Ensembles 5 and 6, the whole launch: 1. - 3. of the header comment.  thermo / baro: the thermostat / the barostat is on.
template <int ENS>
__device__ __forceinline__ void md_step_nose_hoover(const MdArgs& a, const MdView& w, bool record, int64_t frame, MdShared sh) {
    const int s = w.s, n = w.n, t = a.t;
    const bool thermo = a.ttime > 0.0, baro = ENS == MD_NPT_NOSE_HOOVER && a.ptime > 0.0;
    const double dt = a.dt, half_dt = 0.5 * dt;
    const double kT = a.kB * a.t0_kelvin[s], g = 3.0 * n, alpha = 1.0 + 3.0 / g;
    const double Q0 = g * kT * a.ttime * a.ttime, Qk = kT * a.ttime * a.ttime;
    const double Qb = kT * a.ptime * a.ptime, Wm = (g + 3.0) * kT * a.ptime * a.ptime;
    const double p_ext = baro ? a.pressure[s] : 0.0;
    double* st = a.nhc_state + NHC_STATE * (int64_t)s;
    double eta[NHC_MAX], v[NHC_MAX], etab[NHC_MAX], vb[NHC_MAX];
#pragma unroll
    for (int k = 0; k < NHC_MAX; ++k) {
        eta[k] = st[k];
        v[k] = st[NHC_MAX + k];
        etab[k] = st[2 * NHC_MAX + k];
        vb[k] = st[3 * NHC_MAX + k];
    }
    double eps = st[4 * NHC_MAX], veps = st[4 * NHC_MAX + 1];
    double volume = 0.0, virial = 0.0;
    if constexpr (md_has_cell(ENS)) {
        volume = fabs(det3(w.C));
        const double* S = a.stress ? a.stress + 9 * (int64_t)s : nullptr;
        virial = S ? -(S[0] + S[4] + S[8]) / 3.0 : 0.0;
    }
    auto g_eps = [&](double K2) { return (alpha * K2 + 3.0 * volume * (virial - p_ext)) / Wm; };

    if (t == 0 && a.fixcm) {  // once: p_i -= m_i sum p / sum m
        double sums[4] = {0.0, 0.0, 0.0, 0.0};
        for (int i = threadIdx.x; i < n; i += MD_BLOCK) {
#pragma unroll
            for (int c = 0; c < 3; ++c) sums[c] += w.P[3 * i + c];
            sums[3] += w.M[i];
        }
        block_reduce<4, false>(sums, sh);
        for (int i = threadIdx.x; i < n; i += MD_BLOCK) {
            const double m = w.M[i];
#pragma unroll
            for (int c = 0; c < 3; ++c) w.P[3 * i + c] -= m * sums[c] / sums[3];
        }
    }

    // 1. the second half-kick, v_eps += dt/2 G_eps, the chains
    double ke[1] = {0.0};
    {
        double ea = 1.0, eb = 1.0;
        if (baro) {
            const double x = alpha * veps * 0.25 * dt;
            ea = exp(-alpha * veps * half_dt);
            eb = exp(-x) * sinhc(x);
        }
        for (int i = threadIdx.x; i < n; i += MD_BLOCK) {
            const double m = w.M[i];
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const int k = 3 * i + c;
                double p = w.P[k];
                if (t > 0) {
                    if (baro)
                        p = p * ea + half_dt * w.F[k] * eb;
                    else
                        p += half_dt * w.F[k];
                    w.P[k] = p;
                }
                ke[0] += p * p / m;
            }
        }
        block_reduce<1, false>(ke, sh);
    }
    if (t > 0) {
        if (baro) veps += half_dt * g_eps(ke[0]);
        if (thermo) {
            const double sc = nhc_half(a, ke[0], g, kT, Q0, Qk, v, eta);
            if (baro) veps *= nhc_half(a, Wm * veps * veps, 1.0, kT, Qb, Qb, vb, etab);
            ke[0] = 0.0;
            for (int i = threadIdx.x; i < n; i += MD_BLOCK) {
                const double m = w.M[i];
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const double p = sc * w.P[3 * i + c];
                    w.P[3 * i + c] = p;
                    ke[0] += p * p / m;
                }
            }
            block_reduce<1, false>(ke, sh);
        }
    }
    const double KE = 0.5 * ke[0];

    // 2.
    if (record) {
        double* TP = a.traj_positions ? a.traj_positions + 3 * (frame * a.n_rows + w.beg) : nullptr;
        double* TM = a.traj_momenta ? a.traj_momenta + 3 * (frame * a.n_rows + w.beg) : nullptr;
        // (per atom, the mapping of every loop that writes P and R: a thread records what it alone rewrites in 3., no barrier)
        for (int i = threadIdx.x; i < n; i += MD_BLOCK) {
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                if (TM) TM[3 * i + c] = w.P[3 * i + c];
                if (TP) TP[3 * i + c] = w.R[3 * i + c];
            }
        }
        if (threadIdx.x == 0) {
            md_record<ENS>(a, w, frame, KE, 2.0 * KE / (3.0 * n * a.kB), virial, volume);
            if (a.conserved_out) {
                double H = KE + a.energy[s];
                if (thermo) {
                    double q = 0.0, e = 0.0;
#pragma unroll
                    for (int k = 0; k < NHC_MAX; ++k)
                        if (k < a.chain) {
                            q += (k == 0 ? Q0 : Qk) * v[k] * v[k];
                            if (k > 0) e += eta[k];
                        }
                    H += 0.5 * q + g * kT * eta[0] + kT * e;
                }
                if (baro) H += p_ext * volume + 0.5 * Wm * veps * veps;
                if (baro && thermo) {
                    double q = 0.0, e = 0.0;
#pragma unroll
                    for (int k = 0; k < NHC_MAX; ++k)
                        if (k < a.chain) {
                            q += Qb * vb[k] * vb[k];
                            e += etab[k];
                        }
                    H += 0.5 * q + kT * e;
                }
                a.conserved_out[frame * gridDim.x + s] = H;
            }
        }
    }

    // 3. the chains, v_eps += dt/2 G_eps, the first half-kick, the drift
    if (t < a.steps) {
        if (thermo) {
            if (baro) veps *= nhc_half(a, Wm * veps * veps, 1.0, kT, Qb, Qb, vb, etab);
            const double sc = nhc_half(a, ke[0], g, kT, Q0, Qk, v, eta);
            ke[0] = 0.0;
            for (int i = threadIdx.x; i < n; i += MD_BLOCK) {
                const double m = w.M[i];
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const double p = sc * w.P[3 * i + c];
                    w.P[3 * i + c] = p;
                    ke[0] += p * p / m;
                }
            }
            if (baro) block_reduce<1, false>(ke, sh);
        }
        if (baro) {
            veps += half_dt * g_eps(ke[0]);
            const double x = alpha * veps * 0.25 * dt, y = veps * half_dt;
            const double ea = exp(-alpha * veps * half_dt), eb = exp(-x) * sinhc(x);
            const double er = exp(veps * dt), ed = exp(y) * sinhc(y);
            eps += veps * dt;
            double C[9], Ci[9];
#pragma unroll
            for (int c = 0; c < 9; ++c) C[c] = er * w.C[c];
            inverse3(C, Ci);
            if (threadIdx.x == 0) {
#pragma unroll
                for (int c = 0; c < 9; ++c) {
                    a.lattice[9 * (int64_t)s + c] = C[c];
                    a.inv_lattice[9 * (int64_t)s + c] = Ci[c];
                }
            }
            for (int i = threadIdx.x; i < n; i += MD_BLOCK) {
                const double m = w.M[i];
                double r[3];
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const double p = w.P[3 * i + c] * ea + half_dt * w.F[3 * i + c] * eb;
                    w.P[3 * i + c] = p;
                    r[c] = w.R[3 * i + c] * er + dt * (p / m) * ed;
                }
                md_drift_to(w, Ci, i, r);
            }
        } else {
            md_begin_verlet(a, w);
        }
    }
    if (threadIdx.x == 0) {  // (every thread read st before the first reduction's barrier)
#pragma unroll
        for (int k = 0; k < NHC_MAX; ++k) {
            st[k] = eta[k];
            st[NHC_MAX + k] = v[k];
            st[2 * NHC_MAX + k] = etab[k];
            st[3 * NHC_MAX + k] = vb[k];
        }
        st[4 * NHC_MAX] = eps;
        st[4 * NHC_MAX + 1] = veps;
    }
}

template <int ENS>
__global__ __launch_bounds__(MD_BLOCK) void md_step_kernel(const MdArgs a) {
    __shared__ double sh[6][MD_WAVES];
    const int s = blockIdx.x, B = gridDim.x;
    if (a.atom_ptr[B] != a.n_rows) {  // forces of another shape than the batch: touch nothing
        if (threadIdx.x == 0) a.status[0] = -1;
        return;
    }
    const MdView w = md_view<ENS>(a, s);

    // 1. + 2.
    const bool record = a.t % a.interval == 0;
    const int64_t frame = a.t / a.interval;
    if constexpr (md_is_nose_hoover(ENS)) {
        md_step_nose_hoover<ENS>(a, w, record, frame, sh);
        return;
    }
    const double KE = md_finish<ENS>(a, w, record, frame, sh);
    const double T = 2.0 * KE / (3.0 * w.n * a.kB);
    double volume = 0.0, virial = 0.0;
    if constexpr (md_has_cell(ENS)) {
        volume = fabs(det3(w.C));
        const double* S = a.stress ? a.stress + 9 * (int64_t)s : nullptr;
        virial = S ? -(S[0] + S[4] + S[8]) / 3.0 : 0.0;
    }
    if (record && threadIdx.x == 0) md_record<ENS>(a, w, frame, KE, T, virial, volume);
    if (a.t >= a.steps) return;

    // 3.
    if constexpr (ENS == MD_NVE)
        md_begin_verlet(a, w);
    else if constexpr (ENS == MD_LANGEVIN)
        md_begin_langevin(a, w, sh);
    else if constexpr (ENS == MD_ANDERSEN)
        md_begin_andersen(a, w, sh);
    else
        md_begin_berendsen<ENS>(a, w, T, virial, volume, sh);
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

template <int ENS>
void md_launch(const MdArgs& a, hipStream_t stream) {
    md_step_kernel<ENS><<<a.n_structures, MD_BLOCK, 0, stream>>>(a);
}

}  // namespace

extern "C" size_t alignn_md_args_sizeof(void) { return sizeof(alignn_md_args); }

extern "C" int alignn_md_step(const alignn_md_args* args, alignn_stream_t stream) {
    if (!args) return (int)hipErrorInvalidValue;
    const MdArgs& a = *args;
    const int ens = a.ensemble;
    if (a.n_structures < 1 || !a.status || !a.epot || !a.ekin || !a.temperature || a.interval < 1 || a.t < 0 || a.t > a.steps ||
        ens < MD_NVE || ens > MD_NPT_NOSE_HOOVER)
        return (int)hipErrorInvalidValue;
    if (ens != MD_NVE && !a.t0_kelvin) return (int)hipErrorInvalidValue;
    if (md_keeps_velocity(ens) && (!a.velocities || !a.scratch || !a.seeds)) return (int)hipErrorInvalidValue;
    if (md_has_cell(ens) && (!a.lattice || !a.inv_lattice)) return (int)hipErrorInvalidValue;
    if (ens == MD_NPT_BERENDSEN && (!a.stress || !a.pressure || !a.compressibility)) return (int)hipErrorInvalidValue;
    if (md_is_nose_hoover(ens)) {
        if (!a.nhc_state || a.chain < 1 || a.chain > NHC_MAX || a.nhc_loops < 1 || a.nhc_loops > 16 ||
            !(a.nhc_order == 1 || a.nhc_order == 3 || a.nhc_order == 5))
            return (int)hipErrorInvalidValue;
        if (ens == MD_NPT_NOSE_HOOVER && a.ptime > 0.0 && (!a.stress || !a.pressure || !a.lattice || !a.inv_lattice))
            return (int)hipErrorInvalidValue;
    }
    hipStream_t st = (hipStream_t)stream;
    switch (ens) {
        case MD_NVE: md_launch<MD_NVE>(a, st); break;
        case MD_LANGEVIN: md_launch<MD_LANGEVIN>(a, st); break;
        case MD_BERENDSEN: md_launch<MD_BERENDSEN>(a, st); break;
        case MD_ANDERSEN: md_launch<MD_ANDERSEN>(a, st); break;
        case MD_NPT_BERENDSEN: md_launch<MD_NPT_BERENDSEN>(a, st); break;
        case MD_NVT_NOSE_HOOVER: md_launch<MD_NVT_NOSE_HOOVER>(a, st); break;
        default: md_launch<MD_NPT_NOSE_HOOVER>(a, st); break;
    }
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
