// The density modes on the reciprocal lattice that order.hip (sq_accumulate_kernel: the static structure factor) and vanhove.hip
// (fqt_modes_kernel: the intermediate scattering function) share: rho_a(q) = sum_{i in a} exp(2 pi i h . f_i) of one frame, for the
// vectors a thread owns.  include/alignn_order.h states the formulas: f_k = (r Cinv)_k - floor((r Cinv)_k); e_k(h) =
// exp(i pi (2 (h f_k))) by sincospi for h >= 0 and e_k(-h) its conjugate, tabulated in LDS for 16 atoms at a time; the phase of
// (atom, vector) is (e_0(h0) e_1(h1)) e_2(h2), two complex products; the atoms are summed in row order.  float64 without
// contraction; tests/order_ref.py (phases) restates it.
#pragma once
#include "../../include/alignn_order.h"
#include "common.h"
#include "cell3.h"

#pragma clang fp contract(off)

constexpr int SQ_BLOCK = 256, SQ_ATOMS = 16;
constexpr int sq_vectors_per_thread(int ns) { return ns <= 2 ? 8 : 4; }  // (what the registers hold beside NS sums per vector)
constexpr int SQ_HKL = ALIGNN_ORDER_MAX_HKL;
constexpr int SQ_SLOT1 = SQ_HKL + 1, SQ_SLOT2 = SQ_SLOT1 + 2 * SQ_HKL + 1, SQ_SLOTS = SQ_SLOT2 + 2 * SQ_HKL + 1;  // h0 >= 0 | h1 | h2
constexpr double SQ_TWO_PI = 2.0 * 3.14159265358979323846;

// what a workgroup of SQ_BLOCK threads keeps in LDS for a tile of SQ_ATOMS atoms
struct SqTile {
    double2 tab[SQ_ATOMS][SQ_SLOTS];  // (cos, sin) of pi (2 (h f_k)): slots [0, 33) h0 | [33, 98) h1 | [98, 163) h2
    double fr[SQ_ATOMS][3];
    int grp[SQ_ATOMS];
};

// H_k = floor(q_max |C_k| / (2 pi)) and the inverse cell; false when an axis needs more than the range or the cell is singular
__device__ __forceinline__ bool hkl_range(const double (&C)[9], double q_max, int (&H)[3], double (&Ci)[9]) {
    const double det = det3_cof(C);
    bool ok = fabs(det) > 0.0 && fabs(det) < 1e300;  // (a NaN fails)
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const double len = sqrt((C[3 * k] * C[3 * k] + C[3 * k + 1] * C[3 * k + 1]) + C[3 * k + 2] * C[3 * k + 2]);
        const double h = floor((q_max * len) / SQ_TWO_PI);
        if (!(h >= 0.0 && h <= (double)SQ_HKL)) {
            ok = false;
            H[k] = 0;
        } else {
            H[k] = (int)h;
        }
    }
    inv3_cof(C, Ci);
    return ok;
}

// The vectors first + j SQ_BLOCK + threadIdx.x, j < VPT, of a structure with V vectors whose triples begin at hkl: their slots in
// the table, and whether the thread has such a vector (a triple outside the range of this cell is not a vector of it).
template <int VPT>
__device__ __forceinline__ void sq_thread_vectors(const int32_t* hkl, int V, int first, const int (&H)[3], int (&i0)[VPT],
                                                  int (&i1)[VPT], int (&i2)[VPT], bool (&live)[VPT]) {
#pragma unroll
    for (int j = 0; j < VPT; ++j) {
        const int v = first + j * SQ_BLOCK + (int)threadIdx.x;
        live[j] = v < V;
        int h0 = 0, h1 = 0, h2 = 0;
        if (live[j]) {
            h0 = hkl[3 * (int64_t)v];
            h1 = hkl[3 * (int64_t)v + 1];
            h2 = hkl[3 * (int64_t)v + 2];
            if (h0 < 0 || h0 > H[0] || h1 < -H[1] || h1 > H[1] || h2 < -H[2] || h2 > H[2]) {  // (not a vector of this cell)
                live[j] = false;
                h0 = h1 = h2 = 0;
            }
        }
        i0[j] = h0;
        i1[j] = SQ_SLOT1 + SQ_HKL + h1;
        i2[j] = SQ_SLOT2 + SQ_HKL + h2;
    }
}

// rho_a of the frame whose n rows begin at X (their groups at GR), a = 1 .. NS, for the thread's vectors: re, im [VPT][NS].  Every
// thread of the workgroup calls it.
template <int NS, int VPT>
__device__ __forceinline__ void sq_frame_modes(const double* X, const int32_t* GR, int n, const double (&Ci)[9], const int (&H)[3],
                                               const int (&i0)[VPT], const int (&i1)[VPT], const int (&i2)[VPT], SqTile& lds,
                                               double (&re)[VPT][NS], double (&im)[VPT][NS]) {
    const int tid = threadIdx.x;
#pragma unroll
    for (int j = 0; j < VPT; ++j)
#pragma unroll
        for (int g = 0; g < NS; ++g) re[j][g] = im[j][g] = 0.0;
    for (int t0 = 0; t0 < n; t0 += SQ_ATOMS) {
        const int na = min(SQ_ATOMS, n - t0);
        __syncthreads();  // (the last tile's table has been read)
        if (tid < SQ_ATOMS * 3) {
            const int at = tid / 3, k = tid - 3 * at;
            if (at < na) {
                const double x = row_dot(X + 3 * (t0 + at), Ci, k);
                lds.fr[at][k] = x - floor(x);
                if (k == 0) lds.grp[at] = GR[t0 + at];
            }
        }
        __syncthreads();
        for (int e = tid; e < SQ_ATOMS * 3 * (SQ_HKL + 1); e += SQ_BLOCK) {  // h >= 0; e_k(-h) is the conjugate
            const int at = e / (3 * (SQ_HKL + 1)), rest = e - at * (3 * (SQ_HKL + 1));
            const int k = rest / (SQ_HKL + 1), h = rest - k * (SQ_HKL + 1);
            const int Hk = k == 0 ? H[0] : k == 1 ? H[1] : H[2];
            if (at < na && h <= Hk) {
                const double fk = k == 0 ? lds.fr[at][0] : k == 1 ? lds.fr[at][1] : lds.fr[at][2];
                double s, c;
                sincospi(2.0 * ((double)h * fk), &s, &c);
                const int zero = k == 0 ? 0 : k == 1 ? SQ_SLOT1 + SQ_HKL : SQ_SLOT2 + SQ_HKL;
                lds.tab[at][zero + h] = make_double2(c, s);
                if (k > 0 && h > 0) lds.tab[at][zero - h] = make_double2(c, -s);
            }
        }
        __syncthreads();
        for (int at = 0; at < na; ++at) {
            const int g = lds.grp[at];
#pragma unroll
            for (int j = 0; j < VPT; ++j) {
                const double2 e0 = lds.tab[at][i0[j]], e1 = lds.tab[at][i1[j]], e2 = lds.tab[at][i2[j]];
                const double pr = e0.x * e1.x - e0.y * e1.y, pi = e0.x * e1.y + e0.y * e1.x;
                const double xr = pr * e2.x - pi * e2.y, xi = pr * e2.y + pi * e2.x;
#pragma unroll
                for (int s = 0; s < NS; ++s) {
                    const bool member = g == s + 1;
                    re[j][s] = re[j][s] + (member ? xr : 0.0);
                    im[j][s] = im[j][s] + (member ? xi : 0.0);
                }
            }
        }
    }
}
