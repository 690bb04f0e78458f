// One FIRE step for a batch of crystals: ASE's ase/optimize/fire.py as the reference's ForceField.optimize_atoms drives it
// (alignn/ff/ff.py:373-415: FIRE, downhill_check=False) with the convergence test of Optimizer.run in front of it, every
// structure's optimiser state on the device (alignn_amd/relax.py is the host loop).  One kernel, fire_step_kernel<CELL>, on
// the argument block alignn_fire_args (include/alignn_hip.h names every field): at fixed cell over the atoms' rows, with
// ASE's ExpCellFilter (CELL) over the filter's n + 3 generalised rows; what the filter adds sits under if constexpr (CELL).
//
// One workgroup per ACTIVE structure, threads grid-strided over its atoms, float64 throughout.  Three passes over the
// structure's rows, each followed by a fixed-order workgroup reduction (shuffle-down within a wave, then the four wave
// partials added in wave order by every thread alike): no float atomics, so a structure's step is bit-identical from run to
// run and does not depend on which other structures share the launch.
//   reduce  record F (and E) in the full-batch result arrays; F.v, |F|^2, |v|^2, max_i |F_i|^2 over the rows
//   test    converged (max |F_i|^2 < fmax^2) or out of steps -> retire flag, no step
//   mix     v <- mix / reset (ASE's branch on P = F.v), v += dt F; |dr|^2 with dr = dt v
//   move    dr clipped to maxstep over the whole structure, rows += dr, frac = atom rows inv(L) wrapped into [0, 1)
//
// The filter (ase/constraints.py, 3.22.1, default arguments).  Generalised positions of a structure of n atoms: n atom rows
// X_a = positions F^-T and three cell rows X_c = c logm(F), c = n, F the deformation gradient of the current cell C = C0 F^T.
// Generalised forces: atom rows f F; cell rows the virial W = -V sym(stress) (the "naive" force) or, when it points too far
// from it, the exact gradient -d E / d logm(F), the Frechet derivative of expm at L = X_c / c applied to W expm(-L); either
// one / c.  X_c is kept as state instead of recomputing logm(F) from the cell every step (the round trip is the identity to
// rounding: tests/relax_ref.py).  The cell rows are thread 0's.
//
// Constraints (the last fields of the block, NULL / 0 = off and then the same instructions on the same values as without
// them; tests/relax_ref.py restates them).  FixAtoms: a fixed atom's force row reads as zero everywhere but in
// forces_out, so its velocity stays zero and its row in place; the move leaves its row and its frac unwritten.  ExpCellFilter's
// scalar_pressure, hydrostatic_strain and mask shape the virial W before the naive / exact choice, constant_volume takes the
// trace off the chosen force after it.  The flags are the same for a whole workgroup: scalar branches.
#include "../../include/alignn_hip.h"
#include "common.h"

namespace {

constexpr int FIRE_BLOCK = 256;
constexpr int FIRE_WAVES = FIRE_BLOCK / ALIGNN_WAVE;

// Record the evaluation (energy, max_i |F_i| from the reduced max |F_i|^2 in red[3]) and the outcome of Optimizer.run's
// test: converged (max |F_i|^2 < fmax^2) or out of steps -> retire flag 1 / 2 in status[1 + k], else counted in status[0]
__device__ __forceinline__ void fire_record(const double* red, int converged, int taken, int steps, int k, int s,
                                            const double* energy, double* energy_out, double* fmax_out, int32_t* status,
                                            double* enthalpy_out, double pv) {
    if (threadIdx.x == 0) {
        energy_out[s] = energy[k];
        if (enthalpy_out) enthalpy_out[s] = energy[k] + pv;
        fmax_out[s] = sqrt(red[3]);
        const int flag = converged ? 1 : (taken >= steps ? 2 : 0);
        status[1 + k] = flag;
        if (!flag) atomicAdd(status, 1);  // (an integer count: order-independent)
    }
}

// ASE FIRE.step's scalar part from the reduced F.v, |F|^2, |v|^2 (red[0..2]): the mixing weights (zero_v: v restarts from
// zero) and the structure's new dt, a and Nsteps
struct FireScalars {
    double dt, a, mix_v, mix_f;
    int nsteps;
    bool zero_v;
};

__device__ __forceinline__ FireScalars fire_scalars(const double* red, const double* state, const int32_t* istate, int s,
                                                    int taken, double dtmax, int nmin, double finc, double fdec, double astart,
                                                    double fa) {
    FireScalars f{state[2 * s], state[2 * s + 1], 1.0, 0.0, istate[2 * s], taken == 0};  // first step: v = 0, no mixing
    if (!f.zero_v) {
        if (red[0] > 0.0) {
            f.mix_v = 1.0 - f.a;
            f.mix_f = f.a / sqrt(red[1]) * sqrt(red[2]);
            if (f.nsteps > nmin) {
                f.dt = fmin(f.dt * finc, dtmax);
                f.a *= fa;
            }
            f.nsteps += 1;
        } else {
            f.zero_v = true;
            f.a = astart;
            f.dt *= fdec;
            f.nsteps = 0;
        }
    }
    return f;
}

// the step's optimiser state back to the structure's slots
__device__ __forceinline__ void fire_store(const FireScalars& f, int taken, int s, double* state, int32_t* istate) {
    if (threadIdx.x == 0) {
        state[2 * s] = f.dt;
        state[2 * s + 1] = f.a;
        istate[2 * s] = f.nsteps;
        istate[2 * s + 1] = taken + 1;
    }
}

constexpr int EXPM_TAYLOR = 18;  // with |X| <= 1/2 after scaling the remainder is below 1e-22 of |expm|

// squarings s with |A| / 2^s <= 1/2 (|.| any bound of the infinity norm); a non-finite norm gives NaN anyway
__device__ __forceinline__ int expm_squarings(double nrm) {
    if (!(nrm > 0.5)) return 0;
    return min(ilogb(nrm) + 2, 1100);  // nrm < 2^(ilogb + 1): nrm / 2^(ilogb + 2) < 1/2
}

// expm of the 6x6 block upper-triangular [[L, B], [0, L]] as its blocks (E11 = expm(L), E12 = the Frechet derivative of expm
// at L in the direction B): scaling and squaring of a Taylor polynomial, every product done blockwise (three 3x3 products
// instead of one 6x6).  B = 0 gives the 3x3 expm(L) in E11.
__device__ void expm_block(const double* L, const double* B, double* E11, double* E12) {
    double nrm = 0.0;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        double r = 0.0;
#pragma unroll
        for (int j = 0; j < 3; ++j) r += fabs(L[3 * i + j]) + fabs(B[3 * i + j]);
        nrm = fmax(nrm, r);
    }
    const int s = expm_squarings(nrm);
    const double sc = ldexp(1.0, -s);
    double X11[9], X12[9], T11[9], T12[9], U[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) {
        X11[i] = L[i] * sc;
        X12[i] = B[i] * sc;
        E11[i] = (i % 4 == 0) ? 1.0 : 0.0;
        E12[i] = 0.0;
    }
    // Horner: P <- I + X P / k, k = K .. 1
    for (int k = EXPM_TAYLOR; k >= 1; --k) {
        mm3(X11, E11, T11);
        mm3(X11, E12, T12);
        mm3(X12, E11, U);
#pragma unroll
        for (int i = 0; i < 9; ++i) {
            E11[i] = ((i % 4 == 0) ? 1.0 : 0.0) + T11[i] / k;
            E12[i] = (T12[i] + U[i]) / k;
        }
    }
    for (int q = 0; q < s; ++q) {  // [[P, Q], [0, P]]^2 = [[P P, P Q + Q P], [0, P P]]
        mm3(E11, E11, T11);
        mm3(E11, E12, T12);
        mm3(E12, E11, U);
#pragma unroll
        for (int i = 0; i < 9; ++i) {
            E11[i] = T11[i];
            E12[i] = T12[i] + U[i];
        }
    }
}

__device__ __forceinline__ void expm3(const double* L, double* E) {
    const double Z[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    double unused[9];
    expm_block(L, Z, E, unused);
}

// ExpCellFilter's arguments for one structure (all off: pressure and mask NULL, the flags 0)
struct CellOptions {
    const double* pressure;  // the structure's scalar_pressure
    const double* mask;      // its 3 x 3 mask
    int hydrostatic_strain, constant_volume;
};

// the filter's cell rows (before the division by c) from the current cell C, the stress S (eV/A^3, ASE sign) and L = X_c / c;
// Ssym (the symmetrised stress) is returned as well, and the cell's volume
__device__ double cell_force(const double* C, const double* S, const double* L, const CellOptions& o, double* G, double* Ssym) {
    const double V = fabs(det3(C));
    double W[9];  // the virial; naive force
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            Ssym[3 * i + j] = i == j ? S[3 * i + j] : (S[3 * i + j] + S[3 * j + i]) / 2;
            W[3 * i + j] = -V * Ssym[3 * i + j];
        }
    if (o.pressure) {
        const double p = *o.pressure;
#pragma unroll
        for (int i = 0; i < 9; i += 4) W[i] = -V * (Ssym[i] + p);
    }
    if (o.hydrostatic_strain) {
        const double t = (W[0] + W[4] + W[8]) / 3.0;
#pragma unroll
        for (int i = 0; i < 9; ++i) W[i] = (i % 4 == 0) ? t : 0.0;
    }
    if (o.mask) {
#pragma unroll
        for (int i = 0; i < 9; ++i) W[i] *= o.mask[i];
    }
    // exact force: -expm([[L, -W expm(-L)], [0, L]])[0:3, 3:6], symmetrised; the upper-right block is linear in W, so it is
    // computed for W scaled by a power of two to below one
    double mL[9], Em[9], Bm[9], E11[9], E12[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) mL[i] = -L[i];
    expm3(mL, Em);
    mm3(W, Em, Bm);
    double bmax = 0.0;
#pragma unroll
    for (int i = 0; i < 9; ++i) bmax = fmax(bmax, fabs(Bm[i]));
    const int be = bmax > 0.0 && bmax <= 1.7e308 ? ilogb(bmax) + 1 : 0;  // bmax / 2^be in [1/2, 1)
#pragma unroll
    for (int i = 0; i < 9; ++i) Bm[i] = -ldexp(Bm[i], -be);
    expm_block(L, Bm, E11, E12);
    double E[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) E[i] = -ldexp(E12[i], be);
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = i + 1; j < 3; ++j) {
            const double f = 0.5 * (E[3 * i + j] + E[3 * j + i]);
            E[3 * i + j] = f;
            E[3 * j + i] = f;
        }
    // ASE's switch: the naive force when numpy.isclose holds everywhere (rtol 1e-5, atol 1e-8, against the naive one) or the
    // cosine of the two exceeds 0.8 (a NaN cosine does not)
    bool close = true;
    double en = 0.0, ee = 0.0, nn = 0.0;
#pragma unroll
    for (int i = 0; i < 9; ++i) {
        close = close && (E[i] == W[i] || fabs(E[i] - W[i]) <= 1e-8 + 1e-5 * fabs(W[i]));
        en += E[i] * W[i];
        ee += E[i] * E[i];
        nn += W[i] * W[i];
    }
    const bool naive = close || en / sqrt(ee * nn) > 0.8;
#pragma unroll
    for (int i = 0; i < 9; ++i) G[i] = naive ? W[i] : E[i];
    if (o.constant_volume) {
        const double t = (G[0] + G[4] + G[8]) / 3.0;
#pragma unroll
        for (int i = 0; i < 9; i += 4) G[i] -= t;
    }
    return V;
}

using FireArgs = alignn_fire_args;

template <bool CELL>
__global__ __launch_bounds__(FIRE_BLOCK) void fire_step_kernel(const FireArgs a) {
    __shared__ double sh[4][FIRE_WAVES];
    const int k = blockIdx.x;
    const int s = a.active[k];
    const int beg = a.atom_ptr[s], n = a.atom_ptr[s + 1] - beg;
    const int fbeg = a.force_ptr[k];
    if (a.force_ptr[k + 1] - fbeg != n) {  // forces of another shape than the structure: touch nothing
        if (threadIdx.x == 0) a.status[1 + k] = -1;
        return;
    }
    const double* Fo = a.forces + 3 * (int64_t)fbeg;
    double* X = (CELL ? a.xa : a.positions) + 3 * (int64_t)beg;  // the atom rows
    double* V = a.velocities + 3 * (int64_t)beg;
    double* FOUT = a.forces_out + 3 * (int64_t)beg;
    const uint8_t* FIX = a.fixed ? a.fixed + beg : nullptr;  // FixAtoms: the structure's flags
    const int taken = a.istate[2 * s + 1];
    const double maxstep = a.maxstep;
    double pv = 0.0;  // scalar_pressure * volume (thread 0)

    // the filter's part of the rows: the deformation gradient of the evaluated cell and, on thread 0, the cell rows' forces
    // (ExpCellFilter's cell_factor is n) and velocities
    double D[9], G[9], vc[9];
    [[maybe_unused]] double* XC = nullptr;
    [[maybe_unused]] double* VC = nullptr;
    if constexpr (CELL) {
        const double c = (double)n;
        XC = a.xc + 9 * (int64_t)s;
        VC = a.cell_velocities + 9 * (int64_t)s;
#pragma unroll
        for (int i = 0; i < 9; ++i) D[i] = a.defgrad[9 * (int64_t)s + i];
        if (threadIdx.x == 0) {
            double L[9], Ssym[9];
#pragma unroll
            for (int i = 0; i < 9; ++i) L[i] = XC[i] / c;
            const CellOptions opt{a.scalar_pressure ? a.scalar_pressure + s : nullptr,
                                  a.cell_mask ? a.cell_mask + 9 * (int64_t)s : nullptr, a.hydrostatic_strain, a.constant_volume};
            const double vol = cell_force(a.lattice + 9 * (int64_t)s, a.stress + 9 * (int64_t)k, L, opt, G, Ssym);
            if (opt.pressure) pv = *opt.pressure * vol;
#pragma unroll
            for (int i = 0; i < 9; ++i) {
                G[i] /= c;
                vc[i] = VC[i];
                a.stress_out[9 * (int64_t)s + i] = Ssym[i];
            }
        }
    }
    // the generalised force of atom row i: f F under the filter, else f (f: as evaluated); a fixed atom's is zero
    auto atom_force = [&](int i, double (&f)[3], double (&g)[3]) {
#pragma unroll
        for (int j = 0; j < 3; ++j) f[j] = Fo[3 * i + j];
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            if constexpr (CELL)
                g[j] = f[0] * D[j] + f[1] * D[3 + j] + f[2] * D[6 + j];
            else
                g[j] = f[j];
        }
        if (FIX && FIX[i]) g[0] = g[1] = g[2] = 0.0;
    };

    // reduce over the rows (the cell rows are thread 0's last), record, test convergence
    double red[4] = {0.0, 0.0, 0.0, 0.0};  // G.v, |G|^2, |v|^2, max |G_i|^2
    auto reduce_row = [&](const double* g, const double* v) {
        double fi2 = 0.0;
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            red[0] += g[j] * v[j];
            fi2 += g[j] * g[j];
            red[2] += v[j] * v[j];
        }
        red[1] += fi2;
        red[3] = fmax(red[3], fi2);
    };
    for (int i = threadIdx.x; i < n; i += FIRE_BLOCK) {
        double f[3], g[3], v[3];
        atom_force(i, f, g);
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            FOUT[3 * i + j] = f[j];
            v[j] = V[3 * i + j];
        }
        reduce_row(g, v);
    }
    if constexpr (CELL) {
        if (threadIdx.x == 0) {
#pragma unroll
            for (int r = 0; r < 3; ++r) reduce_row(G + 3 * r, vc + 3 * r);
        }
    }
    block_reduce<4, true>(red, sh);
    const int converged = red[3] < a.fmax * a.fmax;
    fire_record(red, converged, taken, a.steps, k, s, a.energy, a.energy_out, a.fmax_out, a.status,
                CELL ? a.enthalpy_out : nullptr, pv);
    if (converged || taken >= a.steps) return;

    // ASE FIRE.step: mix and kick
    const FireScalars fire = fire_scalars(red, a.state, a.istate, s, taken, a.dtmax, a.nmin, a.finc, a.fdec, a.astart, a.fa);
    const double dt = fire.dt;
    double dr2[1] = {0.0};
    auto kick = [&](double v, double g) {
        v = fire.zero_v ? 0.0 : fire.mix_v * v + fire.mix_f * g;
        v += dt * g;
        const double d = dt * v;
        dr2[0] += d * d;
        return v;
    };
    for (int i = threadIdx.x; i < n; i += FIRE_BLOCK) {
        double f[3], g[3];
        atom_force(i, f, g);
#pragma unroll
        for (int j = 0; j < 3; ++j) V[3 * i + j] = kick(V[3 * i + j], g[j]);
    }
    if constexpr (CELL) {
        if (threadIdx.x == 0) {
#pragma unroll
            for (int i = 0; i < 9; ++i) vc[i] = kick(vc[i], G[i]);
        }
    }
    block_reduce<1, false>(dr2, sh);

    // the clipped move; under the filter F = expm(X_c / c), C = C0 F^T (thread 0), positions X_a F^T
    const double normdr = sqrt(dr2[0]);
    const bool clip = normdr > maxstep;
    auto step_of = [&](double v) {
        double d = dt * v;
        if (clip) d = maxstep * d / normdr;
        return d;
    };
    double Fn[9];
    if constexpr (CELL) {
        __shared__ double Fsh[9];
        if (threadIdx.x == 0) {
            const double c = (double)n;
            double L[9];
#pragma unroll
            for (int i = 0; i < 9; ++i) {
                const double x = XC[i] + step_of(vc[i]);
                XC[i] = x;
                VC[i] = vc[i];
                L[i] = x / c;
            }
            expm3(L, Fn);
            const double* C0 = a.lattice0 + 9 * (int64_t)s;
#pragma unroll
            for (int i = 0; i < 3; ++i)
#pragma unroll
                for (int j = 0; j < 3; ++j)
                    a.lattice[9 * (int64_t)s + 3 * i + j] = C0[3 * i] * Fn[3 * j] + C0[3 * i + 1] * Fn[3 * j + 1] + C0[3 * i + 2] * Fn[3 * j + 2];
#pragma unroll
            for (int i = 0; i < 9; ++i) {
                a.defgrad[9 * (int64_t)s + i] = Fn[i];
                Fsh[i] = Fn[i];
            }
        }
        __syncthreads();
#pragma unroll
        for (int i = 0; i < 9; ++i) Fn[i] = Fsh[i];
    }
    const double* Li = a.inv_lattice + 9 * (int64_t)s;
    for (int i = threadIdx.x; i < n; i += FIRE_BLOCK) {
        const bool held = FIX && FIX[i];  // its row and its frac stay as they are; under the filter it rides with the cell
        double x[3];
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            if (held) {
                x[j] = X[3 * i + j];
            } else {
                x[j] = X[3 * i + j] + step_of(V[3 * i + j]);
                X[3 * i + j] = x[j];
            }
        }
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            if constexpr (CELL) a.positions[3 * ((int64_t)beg + i) + j] = x[0] * Fn[3 * j] + x[1] * Fn[3 * j + 1] + x[2] * Fn[3 * j + 2];
            if (!held) a.frac[3 * ((int64_t)beg + i) + j] = wrap01(x[0] * Li[j] + x[1] * Li[3 + j] + x[2] * Li[6 + j]);
        }
    }
    fire_store(fire, taken, s, a.state, a.istate);
}

}  // namespace

extern "C" size_t alignn_fire_args_sizeof(void) { return sizeof(alignn_fire_args); }

extern "C" int alignn_fire_step(const alignn_fire_args* args, alignn_stream_t stream) {
    if (!args || args->n_active < 0 || !args->status) return (int)hipErrorInvalidValue;
    const FireArgs& a = *args;
    const bool cell = a.xc != nullptr;  // a cell-filter state: every field of the filter is then needed
    if (cell && (!a.stress || !a.lattice0 || !a.xa || !a.cell_velocities || !a.defgrad || !a.lattice || !a.stress_out))
        return (int)hipErrorInvalidValue;
    if (!cell && (a.cell_mask || a.scalar_pressure || a.hydrostatic_strain || a.constant_volume || a.enthalpy_out))
        return (int)hipErrorInvalidValue;  // the filter's options without the filter
    hipStream_t st = (hipStream_t)stream;
    hipError_t e = hipMemsetAsync(a.status, 0, sizeof(int32_t), st);
    if (e != hipSuccess) return (int)e;
    if (a.n_active == 0) return 0;
    if (cell)
        fire_step_kernel<true><<<a.n_active, FIRE_BLOCK, 0, st>>>(a);
    else
        fire_step_kernel<false><<<a.n_active, FIRE_BLOCK, 0, st>>>(a);
    ALIGNN_CHECK_LAUNCH();
    return 0;
}
