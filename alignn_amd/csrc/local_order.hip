// Device side of the local structure analysis (alignn_amd/local_order.py): common-neighbour analysis and the bond-orientational
// order parameters q_l, w_l with their averaged forms, for the B structures of a run_md trajectory.  The reference has none of it;
// tests/local_ref.py is the numpy restatement, include/alignn_local.h states the rules, the formulas, the layouts and every field
// of the argument blocks.
//
//   cna_kernel             one wavefront per (frame, centre atom), four per workgroup: the neighbour list by ballot and prefix into
//                          LDS (neighbor_list.h's build_list, the list of order.hip's angles_kernel), the adaptive sort as a
//                          rank count, lane a the 64-bit mask of the entries bonded to entry a, the signature from popcounts and a
//                          flood fill over the masks in LDS, the class from ballots;
//   cna_counts_kernel      one wavefront per (frame, structure): atoms per group and class by LDS integer atomics, the fractions;
//   bond_qlm_kernel        pass 1, one wavefront per (frame, atom): lane a the harmonics of entry a, an xor butterfly per (l, m);
//   bond_finish_kernel     pass 2: the same list again, the gather of q_lm(j), then s, t, q, w of q_lm and of the averaged q_lm.
// float64, no contraction, no atomics on floating-point values, every sum in a fixed order over the atom's own list: a structure's
// bits are the same alone, in a batch and at any place of the batch.
#include "../../include/alignn_local.h"
#include "neighbor_list.h"

#pragma clang fp contract(off)

namespace {

constexpr int WAVES = 4, BLOCK = WAVES * ALIGNN_WAVE;
constexpr int BLOCK_FRAMES = 16;  // frames used per workgroup, a wavefront takes every fourth
constexpr int NBR = ALIGNN_LOCAL_MAX_NEIGHBORS;
constexpr int MAX_LS = ALIGNN_LOCAL_MAX_LS, MAX_L = ALIGNN_LOCAL_MAX_L, MS = ALIGNN_LOCAL_M_STRIDE;
constexpr int W3J = ALIGNN_LOCAL_W3J_STRIDE, NSIG = ALIGNN_LOCAL_SIGNATURES, NCLS = ALIGNN_LOCAL_CLASSES;
constexpr double PI = 3.14159265358979323846;
constexpr double SQRT2 = 1.4142135623730951, SQRT3 = 1.7320508075688772;  // (the correctly rounded square roots)

using CnaArgs = alignn_local_cna_args;
using BondArgs = alignn_local_bond_args;

static_assert(NBR == NEIGHBOR_LIST_CAP, "the list of neighbor_list.h");
static_assert(MS == MAX_L + 1 && W3J == (2 * MAX_L + 1) * (2 * MAX_L + 1), "the strides of qlm and w3j");

// ---- common-neighbour analysis ----

// Lane a < 64: the mask of the entries of `sel` other than a within rc of entry a (0 when a is not in sel); then the signature of
// entry a from the masks in LDS, as its code: 0 (4,2,1), 1 (4,2,2), 2 (4,4,4), 3 (5,5,5), 4 (6,6,6), 5 any other, -1 not selected.
__device__ __forceinline__ int signature_code(const double (*list)[4], unsigned long long* masks, int count, unsigned long long sel,
                                              double rc, int lane) {
    const bool mine = (sel >> lane) & 1ull;
    unsigned long long mask = 0ull;
    if (mine) {
        const double ax = list[lane][0], ay = list[lane][1], az = list[lane][2];
        for (int b = 0; b < count; ++b) {
            const double ex = ax - list[b][0], ey = ay - list[b][1], ez = az - list[b][2];
            const bool bonded = sqrt((ex * ex + ey * ey) + ez * ez) < rc;
            if (bonded && b != lane && ((sel >> b) & 1ull)) mask |= 1ull << b;
        }
    }
    wave_sync();  // (the masks of the stage before have been read)
    masks[lane] = mask;
    wave_sync();
    if (!mine) return -1;
    const int n_cn = __popcll(mask);
    int twice = 0;
    for (unsigned long long rest = mask; rest; rest &= rest - 1ull) twice += __popcll(masks[__ffsll((long long)rest) - 1] & mask);
    const int n_b = twice / 2;
    int n_lcb = 0;
    for (unsigned long long rest = mask; rest;) {  // the components of the bond graph among the common neighbours
        unsigned long long comp = rest & (~rest + 1ull), front = comp;
        while (front) {
            unsigned long long next = 0ull;
            for (unsigned long long f = front; f; f &= f - 1ull) next |= masks[__ffsll((long long)f) - 1] & mask;
            front = next & ~comp;
            comp |= front;
        }
        int bonds = 0;
        for (unsigned long long c = comp; c; c &= c - 1ull) bonds += __popcll(masks[__ffsll((long long)c) - 1] & comp);
        n_lcb = max(n_lcb, bonds / 2);
        rest &= ~comp;
    }
    if (n_cn == 4 && n_b == 2) return n_lcb == 1 ? 0 : n_lcb == 2 ? 1 : 5;
    if (n_cn == 4 && n_b == 4 && n_lcb == 4) return 2;
    if (n_cn == 5 && n_b == 5 && n_lcb == 5) return 3;
    if (n_cn == 6 && n_b == 6 && n_lcb == 6) return 4;
    return 5;
}

// the signatures counted over the wavefront (uniform) and the class they give with nb entries selected
__device__ __forceinline__ int classify(int code, int nb, bool close_packed, bool bcc, int (&sig)[NSIG]) {
#pragma unroll
    for (int k = 0; k < NSIG; ++k) sig[k] = __popcll(__ballot(code == k));
    if (close_packed && nb == 12) {
        if (sig[0] == 12) return 1;
        if (sig[0] == 6 && sig[1] == 6) return 2;
        if (sig[3] == 12) return 4;
    }
    if (bcc && nb == 14 && sig[2] == 6 && sig[4] == 8) return 3;
    return 0;
}

__global__ __launch_bounds__(BLOCK) void cna_kernel(const CnaArgs a) {
    __shared__ double nd[WAVES][NBR][4];  // dx, dy, dz, r of the wavefront's entries
    __shared__ unsigned long long bonded[WAVES][NBR];
    __shared__ double sorted[WAVES][NBR];  // r in ascending order (adaptive)
    const int fc = blockIdx.x, il = blockIdx.y, b = blockIdx.z;
    const int beg = a.atom_ptr[b], n = a.atom_ptr[b + 1] - beg;
    if (n < 1 || beg < 0 || (int64_t)beg + n > a.n_atoms || il >= n) return;  // (uniform over the workgroup)
    const int lane = threadIdx.x & (ALIGNN_WAVE - 1), wave = threadIdx.x / ALIGNN_WAVE;
    const int Sb = species_of(a.group_count, b, a.n_species);
    const int32_t* GR = a.group + beg;
    const double r_cut = a.r_cut[b];
    double(*list)[4] = nd[wave];
    unsigned long long* masks = bonded[wave];
    double* rs = sorted[wave];

    for (int fl = wave; fl < BLOCK_FRAMES; fl += WAVES) {
        const int f = fc * BLOCK_FRAMES + fl;
        if (f >= a.n_frames) break;  // (uniform over the wavefront; no workgroup barrier in this kernel)
        const int frame = a.frame0 + f * a.frame_step;
        double C[9], Ci[9];
        int M[3];
        if (!frame_cell(a.lattice, a.lattice_per_frame, a.n_structs, frame, b, r_cut, ALIGNN_LOCAL_MAX_IMAGE_RANGE, C, Ci, M) ||
            !(r_cut > 0.0)) {  // (or r_cut is not a number > 0)
            if (lane == 0) atomicOr(a.status, ALIGNN_LOCAL_STATUS_IMAGES);
            continue;
        }
        const double* X = a.traj + 3 * ((int64_t)frame * a.n_atoms + beg);
        wave_sync();  // (the list of the frame before has been read)
        const int count = build_list<false, false>(X, GR, n, il, Sb, C, Ci, M, r_cut, lane, list, nullptr, nullptr);
        const int64_t row = (int64_t)f * a.n_atoms + beg + il;
        int cls = 0, sig[NSIG] = {0, 0, 0, 0, 0};
        if (count > NBR) {
            if (lane == 0) atomicOr(a.status, ALIGNN_LOCAL_STATUS_NEIGHBORS);
        } else {
            wave_sync();
            if (!a.adaptive) {
                const unsigned long long sel = count == NBR ? ~0ull : (1ull << count) - 1ull;
                const int code = signature_code(list, masks, count, sel, r_cut, lane);
                cls = classify(code, count, true, true, sig);
            } else {
                int rank = NBR;  // the place of entry `lane` in the order of r, ties by list order
                if (lane < count) {
                    const double mine = list[lane][3];
                    rank = 0;
                    for (int k = 0; k < count; ++k) {
                        const double other = list[k][3];
                        rank += (other < mine || (other == mine && k < lane)) ? 1 : 0;
                    }
                    rs[rank] = mine;
                }
                wave_sync();
                if (count >= 12) {
                    double sum = 0.0;
                    for (int k = 0; k < 12; ++k) sum = sum + rs[k];
                    const double rc = ((1.0 + SQRT2) / 2.0) * (sum / 12.0);
                    const int code = signature_code(list, masks, count, __ballot(rank < 12), rc, lane);
                    cls = classify(code, 12, true, false, sig);
                }
                if (cls == 0) {
#pragma unroll
                    for (int k = 0; k < NSIG; ++k) sig[k] = 0;
                    if (count >= 14) {
                        double s8 = 0.0, s6 = 0.0;
                        for (int k = 0; k < 8; ++k) s8 = s8 + rs[k];
                        for (int k = 8; k < 14; ++k) s6 = s6 + rs[k];
                        const double rc = ((1.0 + SQRT2) / 2.0) * ((((2.0 / SQRT3) * s8) + s6) / 14.0);
                        const int code = signature_code(list, masks, count, __ballot(rank < 14), rc, lane);
                        cls = classify(code, 14, false, true, sig);
                    }
                }
            }
        }
        if (lane == 0) {
            a.structure[row] = cls;
            a.n_neighbors[row] = count;
#pragma unroll
            for (int k = 0; k < NSIG; ++k) a.signature_counts[row * NSIG + k] = sig[k];
        }
    }
}

__global__ __launch_bounds__(ALIGNN_WAVE) void cna_counts_kernel(const CnaArgs a) {
    __shared__ int acc[(ALIGNN_LOCAL_MAX_SPECIES + 1) * NCLS];
    const int f = blockIdx.x, b = blockIdx.y, lane = threadIdx.x;
    const int beg = a.atom_ptr[b], n = a.atom_ptr[b + 1] - beg;
    const int S = a.n_species, G = S + 1;
    const bool ok = n >= 1 && beg >= 0 && (int64_t)beg + n <= a.n_atoms;
    for (int k = lane; k < G * NCLS; k += ALIGNN_WAVE) acc[k] = 0;
    __syncthreads();
    for (int r = lane; ok && r < n; r += ALIGNN_WAVE) {
        const int g = a.group[beg + r], c = a.structure[(int64_t)f * a.n_atoms + beg + r];
        if (g >= 1 && g <= S && c >= 0 && c < NCLS) {
            atomicAdd(acc + c, 1);
            atomicAdd(acc + g * NCLS + c, 1);
        }
    }
    __syncthreads();
    for (int k = lane; k < G * NCLS; k += ALIGNN_WAVE) {
        const int g = k / NCLS, c = k - g * NCLS;
        const int64_t at = (((int64_t)b * G + g) * a.n_frames + f) * NCLS + c;
        const double Na = (double)a.group_count[b * G + g];
        a.counts[at] = (int64_t)acc[k];
        a.fraction[at] = Na > 0.0 ? (double)acc[k] / Na : 0.0;
    }
}

// ---- bond-orientational order ----

__global__ __launch_bounds__(BLOCK) void bond_qlm_kernel(const BondArgs a) {
    __shared__ double nd[WAVES][NBR][4];
    const int fc = blockIdx.x, il = blockIdx.y, b = blockIdx.z;
    const int beg = a.atom_ptr[b], n = a.atom_ptr[b + 1] - beg;
    if (n < 1 || beg < 0 || (int64_t)beg + n > a.n_atoms || il >= n) return;  // (uniform over the workgroup)
    const int lane = threadIdx.x & (ALIGNN_WAVE - 1), wave = threadIdx.x / ALIGNN_WAVE;
    const int Sb = species_of(a.group_count, b, a.n_species);
    const int32_t* GR = a.group + beg;
    const double r_cut = a.r_cut[b];
    const int L = a.n_ls;
    const int ls[MAX_LS] = {a.l0, a.l1, a.l2, a.l3};
    int lmax = 0;
#pragma unroll
    for (int u = 0; u < MAX_LS; ++u)
        if (u < L) lmax = max(lmax, ls[u]);
    double(*list)[4] = nd[wave];

    for (int fl = wave; fl < BLOCK_FRAMES; fl += WAVES) {
        const int fk = fc * BLOCK_FRAMES + fl;  // the frame of the chunk
        if (fk >= a.chunk_frames) break;        // (uniform over the wavefront)
        const int f = a.chunk0 + fk, frame = a.frame0 + f * a.frame_step;
        double C[9], Ci[9];
        int M[3];
        if (!frame_cell(a.lattice, a.lattice_per_frame, a.n_structs, frame, b, r_cut, ALIGNN_LOCAL_MAX_IMAGE_RANGE, C, Ci, M) ||
            !(r_cut > 0.0)) {  // (or r_cut is not a number > 0)
            if (lane == 0) atomicOr(a.status, ALIGNN_LOCAL_STATUS_IMAGES);
            continue;
        }
        const double* X = a.traj + 3 * ((int64_t)frame * a.n_atoms + beg);
        wave_sync();  // (the list of the frame before has been read)
        const int count = build_list<false, false>(X, GR, n, il, Sb, C, Ci, M, r_cut, lane, list, nullptr, nullptr);
        double* out = a.qlm + ((int64_t)fk * a.n_atoms + beg + il) * L * MS * 2;
        if (lane == 0) a.n_neighbors[(int64_t)f * a.n_atoms + beg + il] = count;
        if (count > NBR || count == 0) {
            if (count > NBR && lane == 0) atomicOr(a.status, ALIGNN_LOCAL_STATUS_NEIGHBORS);
            for (int k = lane; k < L * MS * 2; k += ALIGNN_WAVE) out[k] = 0.0;
            continue;
        }
        wave_sync();
        const bool mine = lane < count;
        double x = 0.0, y = 0.0, z = 0.0;
        if (mine) {
            const double r = list[lane][3];
            x = list[lane][0] / r;
            y = list[lane][1] / r;
            z = list[lane][2] / r;
        }
        const double nn = (double)count;
        double er = 1.0, ei = 0.0, gmm = 1.0;  // (x + i y)^m and G_mm
        for (int m = 0; m <= lmax; ++m) {       // (every bound and branch below is uniform)
            if (m > 0) {
                const double nr = er * x - ei * y, ni = er * y + ei * x;
                er = nr;
                ei = ni;
                gmm = -((double)(2 * m - 1)) * gmm;
            }
            double gm2 = 0.0, gm1 = 0.0;  // G_(l-2)m, G_(l-1)m
            for (int l = m; l <= lmax; ++l) {
                double g;
                if (l == m)
                    g = gmm;
                else if (l == m + 1)
                    g = ((double)(2 * m + 1) * z) * gm1;
                else
                    g = (((double)(2 * l - 1) * z) * gm1 - (double)(l + m - 1) * gm2) / (double)(l - m);
                gm2 = gm1;
                gm1 = g;
#pragma unroll
                for (int u = 0; u < MAX_LS; ++u) {
                    if (u < L && ls[u] == l) {
                        const double nm = a.ynorm[l * MS + m];
                        const double re = wave_sum(mine ? nm * (g * er) : 0.0), im = wave_sum(mine ? nm * (g * ei) : 0.0);
                        if (lane == 0) {
                            out[(u * MS + m) * 2] = re / nn;
                            out[(u * MS + m) * 2 + 1] = im / nn;
                        }
                    }
                }
            }
        }
    }
}

// q_(l,m) of m in -l .. l from the stored half: q_(l,-m) = (-1)^m conj(q_lm)
__device__ __forceinline__ void signed_m(const double (*q)[2], int m, double& re, double& im) {
    const int am = m < 0 ? -m : m;
    re = q[am][0];
    im = q[am][1];
    if (m < 0) {
        im = -im;
        if (am & 1) {
            re = -re;
            im = -im;
        }
    }
}

// s, t, q, w of the degree l from its q_lm in LDS (uniform over the wavefront)
__device__ __forceinline__ void invariants(const double (*q)[2], int l, const double* w3j, int lane, double& s, double& t, double& ql,
                                           double& wl) {
    s = q[0][0] * q[0][0] + q[0][1] * q[0][1];
    for (int m = 1; m <= l; ++m) s = s + 2.0 * (q[m][0] * q[m][0] + q[m][1] * q[m][1]);
    const int w = 2 * l + 1;
    double part = 0.0;
    for (int k = lane; k < w * w; k += ALIGNN_WAVE) {
        const int i1 = k / w, m1 = i1 - l, m2 = k - i1 * w - l, m3 = -(m1 + m2);
        if (m3 >= -l && m3 <= l) {
            double ar, ai, br, bi, cr, ci;
            signed_m(q, m1, ar, ai);
            signed_m(q, m2, br, bi);
            signed_m(q, m3, cr, ci);
            const double pr = ar * br - ai * bi, pi = ar * bi + ai * br;
            part = part + w3j[k] * (pr * cr - pi * ci);
        }
    }
    t = wave_sum(part);
    ql = sqrt(((4.0 * PI) / (double)(2 * l + 1)) * s);
    wl = s > 0.0 ? t / (s * sqrt(s)) : 0.0;
}

__global__ __launch_bounds__(BLOCK) void bond_finish_kernel(const BondArgs a) {
    __shared__ double nd[WAVES][NBR][4];
    __shared__ int nj[WAVES][NBR];
    __shared__ double own[WAVES][MS][2], avg[WAVES][MS][2];
    const int fc = blockIdx.x, il = blockIdx.y, b = blockIdx.z;
    const int beg = a.atom_ptr[b], n = a.atom_ptr[b + 1] - beg;
    if (n < 1 || beg < 0 || (int64_t)beg + n > a.n_atoms || il >= n) return;  // (uniform over the workgroup)
    const int lane = threadIdx.x & (ALIGNN_WAVE - 1), wave = threadIdx.x / ALIGNN_WAVE;
    const int Sb = species_of(a.group_count, b, a.n_species);
    const int32_t* GR = a.group + beg;
    const double r_cut = a.r_cut[b];
    const int L = a.n_ls;
    const int ls[MAX_LS] = {a.l0, a.l1, a.l2, a.l3};
    double(*list)[4] = nd[wave];
    int* lj = nj[wave];
    double(*qo)[2] = own[wave];
    double(*qa)[2] = avg[wave];

    for (int fl = wave; fl < BLOCK_FRAMES; fl += WAVES) {
        const int fk = fc * BLOCK_FRAMES + fl;
        if (fk >= a.chunk_frames) break;  // (uniform over the wavefront)
        const int f = a.chunk0 + fk, frame = a.frame0 + f * a.frame_step;
        double C[9], Ci[9];
        int M[3];
        if (!frame_cell(a.lattice, a.lattice_per_frame, a.n_structs, frame, b, r_cut, ALIGNN_LOCAL_MAX_IMAGE_RANGE, C, Ci, M) ||
            !(r_cut > 0.0))
            continue;  // (pass 1 has set the bit)
        const int64_t row = (int64_t)f * a.n_atoms + beg + il;
        const double* Qf = a.qlm + ((int64_t)fk * a.n_atoms + beg) * L * MS * 2;  // the q_lm of this structure in this frame
        int count = 0;
        if (a.average) {
            const double* X = a.traj + 3 * ((int64_t)frame * a.n_atoms + beg);
            wave_sync();  // (the list of the frame before has been read)
            count = build_list<true, false>(X, GR, n, il, Sb, C, Ci, M, r_cut, lane, list, lj, nullptr);
            wave_sync();
        }
        const bool over = count > NBR;  // (pass 1 has written zeros for q_lm and set the bit)
        const int j = !over && lane < count ? lj[lane] : -1;
        for (int u = 0; u < L; ++u) {
            const int l = ls[u];
            wave_sync();  // (the q_lm of the degree before have been read; the list is written)
            const double* mine = Qf + ((int64_t)il * L + u) * MS * 2;
            for (int m = 0; m <= l; ++m) {
                const double re = mine[2 * m], im = mine[2 * m + 1];
                if (a.average) {
                    double gr = 0.0, gi = 0.0;
                    if (j >= 0) {
                        const double* theirs = Qf + ((int64_t)j * L + u) * MS * 2;
                        gr = theirs[2 * m];
                        gi = theirs[2 * m + 1];
                    }
                    const double sr = wave_sum(gr), si = wave_sum(gi), nn = (double)(count + 1);
                    if (lane == 0) {
                        qa[m][0] = over ? 0.0 : (re + sr) / nn;
                        qa[m][1] = over ? 0.0 : (im + si) / nn;
                    }
                }
                if (lane == 0) {
                    qo[m][0] = re;
                    qo[m][1] = im;
                }
            }
            wave_sync();
            double s, t, ql, wl;
            invariants(qo, l, a.w3j + (int64_t)u * W3J, lane, s, t, ql, wl);
            if (lane == 0) {
                a.s[row * L + u] = s;
                a.t[row * L + u] = t;
                a.q[row * L + u] = ql;
                a.w[row * L + u] = wl;
            }
            if (a.average) {
                invariants(qa, l, a.w3j + (int64_t)u * W3J, lane, s, t, ql, wl);
                if (lane == 0) {
                    a.s_avg[row * L + u] = s;
                    a.t_avg[row * L + u] = t;
                    a.q_avg[row * L + u] = ql;
                    a.w_avg[row * L + u] = wl;
                }
            }
        }
    }
}

// the frame selection: every frame used lies inside the trajectory
bool frames_ok(int n_total, int frame0, int step, int n_frames) {
    if (n_total < 0 || frame0 < 0 || step < 1 || n_frames < 0) return false;
    return n_frames == 0 || (int64_t)frame0 + (int64_t)(n_frames - 1) * step < n_total;
}

bool cna_args_ok(const CnaArgs& a) {
    if (a.n_structs < 0 || a.n_structs > 65535 || a.n_atoms < 0 || a.n_species < 1 || a.n_species > ALIGNN_LOCAL_MAX_SPECIES ||
        a.lattice_per_frame < 0 || a.lattice_per_frame > 1 || a.adaptive < 0 || a.adaptive > 1)
        return false;
    return frames_ok(a.n_total_frames, a.frame0, a.frame_step, a.n_frames);
}

bool bond_args_ok(const BondArgs& a) {
    if (a.n_structs < 0 || a.n_structs > 65535 || a.n_atoms < 0 || a.n_species < 1 || a.n_species > ALIGNN_LOCAL_MAX_SPECIES ||
        a.lattice_per_frame < 0 || a.lattice_per_frame > 1 || a.average < 0 || a.average > 1 || a.n_ls < 1 || a.n_ls > MAX_LS)
        return false;
    const int ls[MAX_LS] = {a.l0, a.l1, a.l2, a.l3};
    for (int u = 0; u < a.n_ls; ++u) {
        if (ls[u] < 1 || ls[u] > MAX_L) return false;
        for (int w = 0; w < u; ++w)
            if (ls[w] == ls[u]) return false;
    }
    if (!frames_ok(a.n_total_frames, a.frame0, a.frame_step, a.n_frames)) return false;
    return a.chunk0 >= 0 && a.chunk0 <= a.n_frames && a.chunk_frames >= 0 && a.chunk_frames <= a.n_frames - a.chunk0;
}

// the launch of the three kernels that take a wavefront per (frame, atom)
template <class Args>
bool shape_ok(const Args& a) {
    return a.n_atoms >= 1 && a.max_atoms >= 1 && a.max_atoms <= a.n_atoms && a.max_atoms <= 65535;
}

}  // namespace

extern "C" size_t alignn_local_cna_args_size(void) { return sizeof(alignn_local_cna_args); }
extern "C" size_t alignn_local_bond_args_size(void) { return sizeof(alignn_local_bond_args); }

extern "C" int alignn_local_cna(const alignn_local_cna_args* args, void* stream) {
    if (!args || !cna_args_ok(*args)) return (int)hipErrorInvalidValue;
    const CnaArgs& a = *args;
    if (a.n_structs == 0 || a.n_frames == 0) return 0;
    if (!shape_ok(a)) return (int)hipErrorInvalidValue;
    if (!a.traj || !a.lattice || !a.atom_ptr || !a.group || !a.group_count || !a.r_cut || !a.structure || !a.signature_counts ||
        !a.n_neighbors || !a.status)
        return (int)hipErrorInvalidValue;
    cna_kernel<<<dim3(alignn_ceil_div(a.n_frames, BLOCK_FRAMES), a.max_atoms, a.n_structs), BLOCK, 0, (hipStream_t)stream>>>(a);
    ALIGNN_CHECK_LAUNCH();
    return 0;
}

extern "C" int alignn_local_cna_counts(const alignn_local_cna_args* args, void* stream) {
    if (!args || !cna_args_ok(*args)) return (int)hipErrorInvalidValue;
    const CnaArgs& a = *args;
    if (a.n_structs == 0 || a.n_frames == 0) return 0;
    if (a.n_atoms < 1 || !a.atom_ptr || !a.group || !a.group_count || !a.structure || !a.counts || !a.fraction)
        return (int)hipErrorInvalidValue;
    cna_counts_kernel<<<dim3(a.n_frames, a.n_structs), ALIGNN_WAVE, 0, (hipStream_t)stream>>>(a);
    ALIGNN_CHECK_LAUNCH();
    return 0;
}

extern "C" int alignn_local_bond_qlm(const alignn_local_bond_args* args, void* stream) {
    if (!args || !bond_args_ok(*args)) return (int)hipErrorInvalidValue;
    const BondArgs& a = *args;
    if (a.n_structs == 0 || a.n_frames == 0 || a.chunk_frames == 0) return 0;
    if (!shape_ok(a)) return (int)hipErrorInvalidValue;
    if (!a.traj || !a.lattice || !a.atom_ptr || !a.group || !a.group_count || !a.r_cut || !a.ynorm || !a.qlm || !a.n_neighbors ||
        !a.status)
        return (int)hipErrorInvalidValue;
    bond_qlm_kernel<<<dim3(alignn_ceil_div(a.chunk_frames, BLOCK_FRAMES), a.max_atoms, a.n_structs), BLOCK, 0, (hipStream_t)stream>>>(a);
    ALIGNN_CHECK_LAUNCH();
    return 0;
}

extern "C" int alignn_local_bond_finish(const alignn_local_bond_args* args, void* stream) {
    if (!args || !bond_args_ok(*args)) return (int)hipErrorInvalidValue;
    const BondArgs& a = *args;
    if (a.n_structs == 0 || a.n_frames == 0 || a.chunk_frames == 0) return 0;
    if (!shape_ok(a)) return (int)hipErrorInvalidValue;
    if (!a.traj || !a.lattice || !a.atom_ptr || !a.group || !a.group_count || !a.r_cut || !a.w3j || !a.qlm || !a.s || !a.t || !a.q ||
        !a.w)
        return (int)hipErrorInvalidValue;
    if (a.average && (!a.s_avg || !a.t_avg || !a.q_avg || !a.w_avg)) return (int)hipErrorInvalidValue;
    bond_finish_kernel<<<dim3(alignn_ceil_div(a.chunk_frames, BLOCK_FRAMES), a.max_atoms, a.n_structs), BLOCK, 0, (hipStream_t)stream>>>(a);
    ALIGNN_CHECK_LAUNCH();
    return 0;
}
