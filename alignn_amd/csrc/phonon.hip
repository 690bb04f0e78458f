// Batched finite-displacement phonons: ASE 3.22.1's Phonons (ase/phonons.py: run, read, band_structure, get_dos) as the
// reference's ase_phonon drives it (alignn/ff/ff.py:1337), every structure's arrays on the device (alignn_amd/phonons.py is
// the host loop; tests/phonons_ref.py the numpy restatement this file follows).  float64 throughout.
//
//   phonon_displace_kernel   the wrapped fractional (and unwrapped Cartesian) coordinates of the displaced supercells of a
//                            chunk of model evaluations, one workgroup per supercell;
//   phonon_fc_rows_kernel    one force-constant row 3a+i from the forces of its -/+ pair of supercells, drift-corrected;
//   phonon_symmetrize_kernel C_R <- (C_R + C_-R^T) / 2 as ASE's symmetrize (out of place);
//   phonon_acoustic_kernel   ASE's acoustic sum rule on the diagonal blocks of cell 0 (in place);
//   phonon_mass_kernel       D_R = C_R * (m^-1/2 m^-1/2);
//   phonon_eigh_kernel       D(q) formed in LDS from the upper triangle, diagonalised by parallel cyclic complex Jacobi;
//   phonon_dos_*_kernel      the Gaussian-smeared DOS on the per-structure grid.
// No float atomics: every sum runs in a fixed order, so a structure's result is the same bits alone or in a batch.
#include "../../include/alignn_hip.h"
#include "common.h"
#include "phonon_rows.h"

namespace {

constexpr int PH_MAX_M = 96;           // 3n limit of the eigen launch: 96 x 97 x 16 B of LDS for the matrix
constexpr int PH_PHASE_CHUNK = 128;    // cells whose phase factors are staged in LDS at a time
constexpr int PH_MAX_SWEEPS = 40;      // Jacobi sweep cap (status word when hit)
constexpr double PH_OFF_TOL = 1e-14;   // converged: off-diagonal Frobenius norm <= PH_OFF_TOL * ||D(q)||_F

// Supercell atom j = image * n + b, image = (m0 N1 + m1) N2 + m2 (ASE's atoms * (N0, N1, N2)).  Displacement d = 6a + 2i + sg
// moves atom a of image 0 along axis i by -delta (sg = 0) or +delta (sg = 1).  The arithmetic is the restatement's, operation
// for operation (no contraction): cart = ((r_b + m0 L0) + m1 L1) + m2 L2 (+ the displacement), frac_c = wrap01((x S0c + y S1c)
// + z S2c) with S the inverse supercell.
__global__ __launch_bounds__(PH_BLOCK) void phonon_displace_kernel(
    const double* __restrict__ pos, const int32_t* __restrict__ atom_ptr, const double* __restrict__ lattice,
    const double* __restrict__ inv_super, const int32_t* __restrict__ dims, const int32_t* __restrict__ jobs,
    const int64_t* __restrict__ row_off, double delta, double* __restrict__ frac, double* __restrict__ cart) {
#pragma clang fp contract(off)
    const int job = blockIdx.x;
    const int s = jobs[2 * job], d = jobs[2 * job + 1];
    const int beg = atom_ptr[s], n = atom_ptr[s + 1] - beg;
    const Cells c = cells_of(dims, s);
    const int a = d / 6, ax = (d / 2) % 3;
    const double disp = (d & 1) ? delta : -delta;
    const double* L = lattice + 9 * (int64_t)s;
    const double* S = inv_super + 9 * (int64_t)s;
    const int64_t row0 = row_off[job];
    const int n_sc = n * c.count();
    for (int j = threadIdx.x; j < n_sc; j += PH_BLOCK) {
        const int img = j / n, b = j - img * n;
        const double m2 = (double)(img % c.n2), m1 = (double)((img / c.n2) % c.n1), m0 = (double)(img / (c.n1 * c.n2));
        double r[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            r[k] = pos[3 * ((int64_t)beg + b) + k] + m0 * L[k];
            r[k] = r[k] + m1 * L[3 + k];
            r[k] = r[k] + m2 * L[6 + k];
        }
        if (j == a) r[ax] = r[ax] + disp;
        const int64_t row = row0 + j;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            double f = r[0] * S[k] + r[1] * S[3 + k];
            f = f + r[2] * S[6 + k];
            frac[3 * row + k] = wrap01(f);
            if (cart) cart[3 * row + k] = r[k];
        }
    }
}

// Row x = 3a + i of C_N[Ncell][3n][3n] of structure s from the forces of its minus supercell (rows [r0, r0 + n_sc)) and its
// plus supercell (the n_sc rows after): C[cell][x][3b + c] = (F-[cell n + b][c] - F+[...][c]) / (2 delta), after ASE's
// Frederiksen correction (the supercell's force sum taken off atom a's row) or the mean drift (sum / n_sc off every row).
__global__ __launch_bounds__(PH_BLOCK) void phonon_fc_rows_kernel(
    const double* __restrict__ forces, const int32_t* __restrict__ pairs, const int64_t* __restrict__ pair_rows,
    const int32_t* __restrict__ atom_ptr, const int32_t* __restrict__ dims, const int64_t* __restrict__ fc_off, int drift,
    double delta, double* __restrict__ fc) {
    __shared__ double sh[6][PH_WAVES];
    const int p = blockIdx.x;
    const int s = pairs[2 * p], x = pairs[2 * p + 1];
    const int n = atom_ptr[s + 1] - atom_ptr[s], m = 3 * n;
    const int n_sc = n * cells_of(dims, s).count();
    const double* Fm = forces + 3 * pair_rows[p];
    double* C = fc + fc_off[s];
    difference_rows(Fm, Fm + 3 * (int64_t)n_sc, n_sc, x / 3, drift, delta, sh, [&](int j, int k, double v) {
        const int cell = j / n, b = j - cell * n;
        C[((int64_t)cell * m + x) * m + 3 * b + k] = v;
    });
}

// ASE's symmetrize with offset 0: per axis k = (l + N/2) mod N is the fftshifted index; cells with k >= 1 - N % 2 on every
// axis become 0.5 C_l + 0.5 C_l'^T with l' the cell of -R (the reversed slice), the others are copied.
__global__ __launch_bounds__(PH_BLOCK) void phonon_symmetrize_kernel(const double* __restrict__ in, double* __restrict__ out,
                                                                     const int32_t* __restrict__ atom_ptr,
                                                                     const int32_t* __restrict__ dims,
                                                                     const int64_t* __restrict__ fc_off) {
    const int s = blockIdx.y;
    const int m = 3 * (atom_ptr[s + 1] - atom_ptr[s]);
    const Cells c = cells_of(dims, s);
    const int64_t mm = (int64_t)m * m, total = (int64_t)c.count() * mm;
    const double* I = in + fc_off[s];
    double* O = out + fc_off[s];
    for (int64_t e = (int64_t)blockIdx.x * PH_BLOCK + threadIdx.x; e < total; e += (int64_t)gridDim.x * PH_BLOCK) {
        const int cell = (int)(e / mm);
        const int rc = (int)(e - (int64_t)cell * mm), x = rc / m, y = rc - x * m;
        const int l[3] = {cell / (c.n1 * c.n2), (cell / c.n2) % c.n1, cell % c.n2};
        const int N[3] = {c.n0, c.n1, c.n2};
        bool inside = true;
        int lp[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const int i0 = 1 - N[k] % 2, h = N[k] / 2;
            const int kk = (l[k] + h) % N[k];
            inside = inside && kk >= i0;
            const int kr = N[k] - 1 + i0 - kk;
            lp[k] = ((kr - h) % N[k] + N[k]) % N[k];
        }
        if (inside) {
            const int64_t partner = (int64_t)((lp[0] * c.n1 + lp[1]) * c.n2 + lp[2]);
            O[e] = 0.5 * I[e] + 0.5 * I[partner * mm + (int64_t)y * m + x];
        } else {
            O[e] = I[e];
        }
    }
}

// ASE's acoustic: C[0][3a+i][3a+j] -= C_copy[cell][3a+i][3a'+j] for cell, then a', in that order, one thread per (a, i, j).
// In place: the elements a thread reads are never another thread's diagonal-block elements, and its own is read first.
__global__ __launch_bounds__(PH_BLOCK) void phonon_acoustic_kernel(double* __restrict__ fc, const int32_t* __restrict__ atom_ptr,
                                                                   const int32_t* __restrict__ dims,
                                                                   const int64_t* __restrict__ fc_off) {
    const int s = blockIdx.y;
    const int n = atom_ptr[s + 1] - atom_ptr[s], m = 3 * n;
    const int ncell = cells_of(dims, s).count();
    double* C = fc + fc_off[s];
    const int t = blockIdx.x * PH_BLOCK + threadIdx.x;
    if (t >= 9 * n) return;
    const int a = t / 9, i = (t / 3) % 3, j = t % 3;
    const int64_t row = 3 * a + i;
    double v = C[row * m + 3 * a + j];
    for (int cell = 0; cell < ncell; ++cell)
        for (int b = 0; b < n; ++b) v -= C[((int64_t)cell * m + row) * m + 3 * b + j];
    C[row * m + 3 * a + j] = v;
}

// D_R[x][y] = C_R[x][y] * (w_x w_y), w = m^-1/2 of the atom of the index
__global__ __launch_bounds__(PH_BLOCK) void phonon_mass_kernel(const double* __restrict__ fc, double* __restrict__ dyn,
                                                               const double* __restrict__ masses,
                                                               const int32_t* __restrict__ atom_ptr,
                                                               const int32_t* __restrict__ dims,
                                                               const int64_t* __restrict__ fc_off) {
    const int s = blockIdx.y;
    const int beg = atom_ptr[s], m = 3 * (atom_ptr[s + 1] - beg);
    const int64_t mm = (int64_t)m * m, total = (int64_t)cells_of(dims, s).count() * mm;
    const double* C = fc + fc_off[s];
    double* D = dyn + fc_off[s];
    for (int64_t e = (int64_t)blockIdx.x * PH_BLOCK + threadIdx.x; e < total; e += (int64_t)gridDim.x * PH_BLOCK) {
        const int rc = (int)(e % mm), x = rc / m, y = rc - x * m;
        const double w = (1.0 / sqrt(masses[beg + x / 3])) * (1.0 / sqrt(masses[beg + y / 3]));
        D[e] = C[e] * w;
    }
}

__host__ __device__ __forceinline__ int lds_stride(int m) { return m | 1; }  // odd stride in doubles: column walks hit 32 distinct banks

// One workgroup per (q, structure).  LDS: the re / im planes of D(q) [m][stride], then the staged phases, the rotations of
// the round, and the sorted order.  Eigenvectors (modes != NULL) are kept as the rows of W = V^T in the caller's output (row
// j = eigenvector j), rotated there, and written at the end as columns in ascending eigenvalue order.
//
// Rotation of pair (p, q), b = A_pq = |b| e^{i phi}: tau = (A_qq - A_pp) / (2 |b|), t = sgn(tau) / (|tau| + sqrt(1 + tau^2)),
// c = 1 / sqrt(1 + t^2), s = t c; J = [[c, s e^{i phi}], [-s e^{-i phi}, c]] on (p, q); A <- J^H A J, W <- J^T W; then
// A_pp = A_pp - t |b|, A_qq = A_qq + t |b| (of the values before the round), A_pq = A_qp = 0 exactly.  Round r of a sweep pairs (m'-1, r) and
// ((r + k) mod (m'-1), (r - k) mod (m'-1)), k = 1 .. m'/2 - 1, m' = m rounded up to even (the odd player m idles).
__global__ __launch_bounds__(PH_BLOCK) void phonon_eigh_kernel(
    const double* __restrict__ dyn, const int64_t* __restrict__ dyn_off, const int32_t* __restrict__ lattice_points,
    const int32_t* __restrict__ cell_ptr, const int32_t* __restrict__ dim_m, const double* __restrict__ qpoints, int n_q,
    double scale, double* __restrict__ freqs, const int64_t* __restrict__ freq_off, double* __restrict__ eigvals,
    double* __restrict__ modes, const int64_t* __restrict__ mode_off, int32_t* __restrict__ status) {
    extern __shared__ double lds[];
    __shared__ double sh[2][PH_WAVES];
    const int qi = blockIdx.x, s = blockIdx.y;
    const int m = dim_m[s], ld = lds_stride(m);
    const int cbeg = cell_ptr[s], ncell = cell_ptr[s + 1] - cbeg;
    double* Ar = lds;
    double* Ai = Ar + m * ld;
    double* ph = Ai + m * ld;                  // [2][PH_PHASE_CHUNK]
    double* rot = ph + 2 * PH_PHASE_CHUNK;     // [PH_MAX_M / 2][5]: c, s cos phi, s sin phi, new A_pp, new A_qq
    int* pr = reinterpret_cast<int*>(rot + 5 * (PH_MAX_M / 2));  // [PH_MAX_M / 2][2]
    int* order = pr + PH_MAX_M;                // [PH_MAX_M]: order[rank] = index
    const double* DN = dyn + dyn_off[s];
    const double qx = qpoints[3 * qi], qy = qpoints[3 * qi + 1], qz = qpoints[3 * qi + 2];
    const int mm = m * m;

    // D(q) = sum_R D_R exp(-2 pi i q.R), upper triangle (and the diagonal's real part), mirrored as its conjugate
    for (int e = threadIdx.x; e < mm; e += PH_BLOCK) {
        Ar[(e / m) * ld + e % m] = 0.0;
        Ai[(e / m) * ld + e % m] = 0.0;
    }
    for (int c0 = 0; c0 < ncell; c0 += PH_PHASE_CHUNK) {
        const int nc = min(PH_PHASE_CHUNK, ncell - c0);
        __syncthreads();
        for (int c = threadIdx.x; c < nc; c += PH_BLOCK) {
            const int32_t* R = lattice_points + 3 * (int64_t)(cbeg + c0 + c);
            const double th = -6.283185307179586 * (qx * R[0] + qy * R[1] + qz * R[2]);
            ph[c] = cos(th);
            ph[PH_PHASE_CHUNK + c] = sin(th);
        }
        __syncthreads();
        for (int e = threadIdx.x; e < mm; e += PH_BLOCK) {
            const int x = e / m, y = e - x * m;
            if (y < x) continue;
            double re = Ar[x * ld + y], im = Ai[x * ld + y];
            for (int c = 0; c < nc; ++c) {
                const double d = DN[(int64_t)(c0 + c) * mm + e];
                re += d * ph[c];
                im += d * ph[PH_PHASE_CHUNK + c];
            }
            Ar[x * ld + y] = re;
            Ai[x * ld + y] = im;
        }
    }
    __syncthreads();
    for (int e = threadIdx.x; e < mm; e += PH_BLOCK) {
        const int x = e / m, y = e - x * m;
        if (y < x) {
            Ar[x * ld + y] = Ar[y * ld + x];
            Ai[x * ld + y] = -Ai[y * ld + x];
        } else if (y == x) {
            Ai[x * ld + x] = 0.0;
        }
    }
    double* W = modes ? modes + mode_off[s] + 2 * (int64_t)qi * mm : nullptr;  // interleaved re, im
    if (W) {
        for (int e = threadIdx.x; e < mm; e += PH_BLOCK) {
            W[2 * e] = (e / m == e % m) ? 1.0 : 0.0;
            W[2 * e + 1] = 0.0;
        }
    }
    __syncthreads();

    auto sums = [&](bool off_only) {
        double v[1] = {0.0};
        for (int e = threadIdx.x; e < mm; e += PH_BLOCK) {
            const int x = e / m, y = e - x * m;
            if (off_only && x == y) continue;
            const double re = Ar[x * ld + y], im = Ai[x * ld + y];
            v[0] += re * re + im * im;
        }
        block_reduce<1, false>(v, sh);
        return sqrt(v[0]);
    };
    const double fro = sums(false);
    const int mp = m + (m & 1), half = mp / 2;
    bool converged = false;
    for (int sweep = 0; sweep <= PH_MAX_SWEEPS; ++sweep) {
        if (sums(true) <= PH_OFF_TOL * fro) {
            converged = true;
            break;
        }
        if (sweep == PH_MAX_SWEEPS) break;
        for (int r = 0; r < mp - 1; ++r) {
            if (threadIdx.x < half) {
                const int k = threadIdx.x;
                int p = k == 0 ? mp - 1 : (r + k) % (mp - 1);
                int q = k == 0 ? r : (r - k + (mp - 1)) % (mp - 1);
                if (p > q) {
                    const int u = p;
                    p = q;
                    q = u;
                }
                double c = 1.0, sr = 0.0, si = 0.0, app = 0.0, aqq = 0.0;
                if (q < m) {
                    const double br = Ar[p * ld + q], bi = Ai[p * ld + q];
                    const double ab = hypot(br, bi);
                    app = Ar[p * ld + p];
                    aqq = Ar[q * ld + q];
                    if (ab > 0.0) {
                        const double tau = (aqq - app) / (2.0 * ab);
                        const double t = (tau >= 0.0 ? 1.0 : -1.0) / (fabs(tau) + sqrt(1.0 + tau * tau));
                        c = 1.0 / sqrt(1.0 + t * t);
                        const double sn = t * c;
                        sr = sn * (br / ab);
                        si = sn * (bi / ab);
                        app -= t * ab;
                        aqq += t * ab;
                    }
                } else {
                    p = q = -1;
                }
                pr[2 * k] = p;
                pr[2 * k + 1] = q;
                rot[5 * k] = c;
                rot[5 * k + 1] = sr;
                rot[5 * k + 2] = si;
                rot[5 * k + 3] = app;
                rot[5 * k + 4] = aqq;
            }
            __syncthreads();
            // rows: row_p' = c row_p - (sr + i si) row_q, row_q' = (sr - i si) row_p + c row_q
            for (int it = threadIdx.x; it < half * m; it += PH_BLOCK) {
                const int k = it / m, j = it - k * m;
                const int p = pr[2 * k], q = pr[2 * k + 1];
                if (p < 0 || (rot[5 * k + 1] == 0.0 && rot[5 * k + 2] == 0.0)) continue;
                const double c = rot[5 * k], sr = rot[5 * k + 1], si = rot[5 * k + 2];
                const double xr = Ar[p * ld + j], xi = Ai[p * ld + j], yr = Ar[q * ld + j], yi = Ai[q * ld + j];
                Ar[p * ld + j] = c * xr - (sr * yr - si * yi);
                Ai[p * ld + j] = c * xi - (sr * yi + si * yr);
                Ar[q * ld + j] = (sr * xr + si * xi) + c * yr;
                Ai[q * ld + j] = (sr * xi - si * xr) + c * yi;
            }
            __syncthreads();
            // columns: col_p' = c col_p - (sr - i si) col_q, col_q' = (sr + i si) col_p + c col_q; W rows as the columns of V
            for (int it = threadIdx.x; it < half * m; it += PH_BLOCK) {
                const int k = it / m, i = it - k * m;
                const int p = pr[2 * k], q = pr[2 * k + 1];
                if (p < 0 || (rot[5 * k + 1] == 0.0 && rot[5 * k + 2] == 0.0)) continue;
                const double c = rot[5 * k], sr = rot[5 * k + 1], si = rot[5 * k + 2];
                if (i == p) {  // (the 2 x 2 block of the pair: its exact result, from the values before the round)
                    Ar[p * ld + p] = rot[5 * k + 3];
                    Ai[p * ld + p] = 0.0;
                    Ar[p * ld + q] = Ai[p * ld + q] = 0.0;
                } else if (i == q) {
                    Ar[q * ld + q] = rot[5 * k + 4];
                    Ai[q * ld + q] = 0.0;
                    Ar[q * ld + p] = Ai[q * ld + p] = 0.0;
                } else {
                    const double xr = Ar[i * ld + p], xi = Ai[i * ld + p], yr = Ar[i * ld + q], yi = Ai[i * ld + q];
                    Ar[i * ld + p] = c * xr - (sr * yr + si * yi);
                    Ai[i * ld + p] = c * xi - (sr * yi - si * yr);
                    Ar[i * ld + q] = (sr * xr - si * xi) + c * yr;
                    Ai[i * ld + q] = (sr * xi + si * xr) + c * yi;
                }
                if (W) {
                    double* wp = W + 2 * ((int64_t)p * m + i);
                    double* wq = W + 2 * ((int64_t)q * m + i);
                    const double xr = wp[0], xi = wp[1], yr = wq[0], yi = wq[1];
                    wp[0] = c * xr - (sr * yr + si * yi);
                    wp[1] = c * xi - (sr * yi - si * yr);
                    wq[0] = (sr * xr - si * xi) + c * yr;
                    wq[1] = (sr * xi + si * xr) + c * yi;
                }
            }
            __syncthreads();
        }
    }
    if (!converged && threadIdx.x == 0) status[0] = 1;

    // ascending order (ties by index), frequencies sign(l) scale sqrt(|l|)
    for (int i = threadIdx.x; i < m; i += PH_BLOCK) {
        const double li = Ar[i * ld + i];
        int rank = 0;
        for (int j = 0; j < m; ++j) {
            const double lj = Ar[j * ld + j];
            rank += (lj < li || (lj == li && j < i)) ? 1 : 0;
        }
        order[rank] = i;
        const int64_t o = (int64_t)qi * m + rank;
        const double w = scale * sqrt(fabs(li));
        freqs[freq_off[s] + o] = li < 0.0 ? -w : w;
        if (eigvals) eigvals[freq_off[s] + o] = li;
    }
    if (!W) return;
    __syncthreads();
    for (int e = threadIdx.x; e < mm; e += PH_BLOCK) {  // W (rows = eigenvectors) into the LDS planes
        const int j = e / m, i = e - j * m;
        Ar[j * ld + i] = W[2 * e];
        Ai[j * ld + i] = W[2 * e + 1];
    }
    __syncthreads();
    for (int e = threadIdx.x; e < mm; e += PH_BLOCK) {  // modes[i][rank] = eigenvector order[rank], component i
        const int i = e / m, r = e - i * m, j = order[r];
        W[2 * e] = Ar[j * ld + i];
        W[2 * e + 1] = Ai[j * ld + i];
    }
}

// per structure: grid[s][g] = linspace(min - 3 width, max + 3 width, npts)[g] over its n_q * m frequencies
__global__ __launch_bounds__(PH_BLOCK) void phonon_dos_grid_kernel(const double* __restrict__ freqs,
                                                                   const int64_t* __restrict__ freq_off, int npts, double width,
                                                                   double* __restrict__ grid) {
#pragma clang fp contract(off)
    __shared__ double sh[1][PH_WAVES];
    const int s = blockIdx.x;
    const int64_t beg = freq_off[s], end = freq_off[s + 1];
    double lo[1] = {-INFINITY}, hi[1] = {-INFINITY};
    for (int64_t k = beg + threadIdx.x; k < end; k += PH_BLOCK) {
        lo[0] = fmax(lo[0], -freqs[k]);
        hi[0] = fmax(hi[0], freqs[k]);
    }
    block_reduce<1, true>(lo, sh);
    block_reduce<1, true>(hi, sh);
    const double pad = 3.0 * width;
    const double start = -lo[0] - pad, stop = hi[0] + pad;
    const double step = (stop - start) / (double)(npts - 1);
    for (int g = threadIdx.x; g < npts; g += PH_BLOCK) grid[(int64_t)s * npts + g] = g == npts - 1 ? stop : (double)g * step + start;
}

// weights[s][g] = sum_k exp(-0.5 ((x_g - e_k) / width)^2) / (sqrt(2 pi) width), one workgroup per (g, s)
__global__ __launch_bounds__(PH_BLOCK) void phonon_dos_kernel(const double* __restrict__ freqs, const int64_t* __restrict__ freq_off,
                                                              int npts, double width, const double* __restrict__ grid,
                                                              double* __restrict__ weights) {
    __shared__ double sh[1][PH_WAVES];
    const int g = blockIdx.x, s = blockIdx.y;
    const double x = grid[(int64_t)s * npts + g];
    const double norm = 2.5066282746310002 * width;
    double v[1] = {0.0};
    for (int64_t k = freq_off[s] + threadIdx.x; k < freq_off[s + 1]; k += PH_BLOCK) {
        const double u = (x - freqs[k]) / width;
        v[0] += exp(-0.5 * (u * u)) / norm;
    }
    block_reduce<1, false>(v, sh);
    if (threadIdx.x == 0) weights[(int64_t)s * npts + g] = v[0];
}

size_t eigh_lds_bytes(int max_m) {
    return (size_t)2 * max_m * lds_stride(max_m) * sizeof(double) + 2 * PH_PHASE_CHUNK * sizeof(double) +
           5 * (PH_MAX_M / 2) * sizeof(double) + 2 * PH_MAX_M * sizeof(int);
}

int grid_for(int64_t total) { return (int)std::min<int64_t>(std::max<int64_t>(alignn_ceil_div(total, PH_BLOCK), 1), 1024); }

}  // namespace

extern "C" int alignn_phonon_displace(const double* positions, const int32_t* atom_ptr, const double* lattice,
                                      const double* inv_supercell, const int32_t* supercell, const int32_t* jobs,
                                      const int64_t* row_off, int n_jobs, double delta, double* frac, double* cart,
                                      alignn_stream_t stream) {
    if (n_jobs < 0 || !positions || !atom_ptr || !lattice || !inv_supercell || !supercell || !jobs || !row_off || !frac)
        return (int)hipErrorInvalidValue;
    if (n_jobs == 0) return 0;
    phonon_displace_kernel<<<n_jobs, PH_BLOCK, 0, (hipStream_t)stream>>>(positions, atom_ptr, lattice, inv_supercell, supercell,
                                                                          jobs, row_off, delta, frac, cart);
    ALIGNN_CHECK_LAUNCH();
    return 0;
}

extern "C" int alignn_phonon_fc_rows(const double* forces, const int32_t* pairs, const int64_t* pair_rows, int n_pairs,
                                     const int32_t* atom_ptr, const int32_t* supercell, const int64_t* fc_off, int drift,
                                     double delta, double* fc, alignn_stream_t stream) {
    if (n_pairs < 0 || drift < DRIFT_NONE || drift > DRIFT_MEAN || !(delta > 0.0) || !forces || !pairs || !pair_rows || !fc)
        return (int)hipErrorInvalidValue;
    if (n_pairs == 0) return 0;
    phonon_fc_rows_kernel<<<n_pairs, PH_BLOCK, 0, (hipStream_t)stream>>>(forces, pairs, pair_rows, atom_ptr, supercell, fc_off,
                                                                          drift, delta, fc);
    ALIGNN_CHECK_LAUNCH();
    return 0;
}

extern "C" int alignn_phonon_symmetrize(const double* fc_in, double* fc_out, const int32_t* atom_ptr, const int32_t* supercell,
                                        const int64_t* fc_off, int n_structures, int64_t max_elems, alignn_stream_t stream) {
    if (n_structures < 1 || max_elems < 1 || fc_in == fc_out) return (int)hipErrorInvalidValue;
    phonon_symmetrize_kernel<<<dim3(grid_for(max_elems), n_structures), PH_BLOCK, 0, (hipStream_t)stream>>>(fc_in, fc_out, atom_ptr,
                                                                                                          supercell, fc_off);
    ALIGNN_CHECK_LAUNCH();
    return 0;
}

extern "C" int alignn_phonon_acoustic(double* fc, const int32_t* atom_ptr, const int32_t* supercell, const int64_t* fc_off,
                                      int n_structures, int max_atoms, alignn_stream_t stream) {
    if (n_structures < 1 || max_atoms < 1) return (int)hipErrorInvalidValue;
    phonon_acoustic_kernel<<<dim3(alignn_ceil_div(9 * (int64_t)max_atoms, PH_BLOCK), n_structures), PH_BLOCK, 0,
                             (hipStream_t)stream>>>(fc, atom_ptr, supercell, fc_off);
    ALIGNN_CHECK_LAUNCH();
    return 0;
}

extern "C" int alignn_phonon_mass_weight(const double* fc, double* dyn, const double* masses, const int32_t* atom_ptr,
                                         const int32_t* supercell, const int64_t* fc_off, int n_structures, int64_t max_elems,
                                         alignn_stream_t stream) {
    if (n_structures < 1 || max_elems < 1) return (int)hipErrorInvalidValue;
    phonon_mass_kernel<<<dim3(grid_for(max_elems), n_structures), PH_BLOCK, 0, (hipStream_t)stream>>>(fc, dyn, masses, atom_ptr,
                                                                                                    supercell, fc_off);
    ALIGNN_CHECK_LAUNCH();
    return 0;
}

extern "C" int alignn_phonon_eigh_max_dim(void) { return PH_MAX_M; }

extern "C" int alignn_phonon_eigh(const double* dyn, const int64_t* dyn_off, const int32_t* lattice_points,
                                  const int32_t* cell_ptr, const int32_t* dims, int n_structures, int max_dim,
                                  const double* qpoints, int n_q, double scale, double* freqs, const int64_t* freq_off,
                                  double* eigvals, double* modes, const int64_t* mode_off, int32_t* status,
                                  alignn_stream_t stream) {
    if (n_structures < 1 || n_q < 0 || max_dim < 1 || max_dim > PH_MAX_M || !dyn || !dyn_off || !lattice_points || !cell_ptr ||
        !dims || !qpoints || !freqs || !freq_off || !status || (modes && !mode_off))
        return (int)hipErrorInvalidValue;
    if (n_q == 0) return 0;
    const size_t bytes = eigh_lds_bytes(max_dim);
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&phonon_eigh_kernel),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
    if (e != hipSuccess) return (int)e;
    phonon_eigh_kernel<<<dim3(n_q, n_structures), PH_BLOCK, bytes, (hipStream_t)stream>>>(
        dyn, dyn_off, lattice_points, cell_ptr, dims, qpoints, n_q, scale, freqs, freq_off, eigvals, modes, mode_off, status);
    ALIGNN_CHECK_LAUNCH();
    return 0;
}

extern "C" int alignn_phonon_dos(const double* freqs, const int64_t* freq_off, int n_structures, int npts, double width,
                                 double* energies, double* weights, alignn_stream_t stream) {
    if (n_structures < 1 || npts < 2 || !(width > 0.0) || !freqs || !freq_off || !energies || !weights)
        return (int)hipErrorInvalidValue;
    phonon_dos_grid_kernel<<<n_structures, PH_BLOCK, 0, (hipStream_t)stream>>>(freqs, freq_off, npts, width, energies);
    ALIGNN_CHECK_LAUNCH();
    phonon_dos_kernel<<<dim3(npts, n_structures), PH_BLOCK, 0, (hipStream_t)stream>>>(freqs, freq_off, npts, width, energies,
                                                                                       weights);
    ALIGNN_CHECK_LAUNCH();
    return 0;
}
