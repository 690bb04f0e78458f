/* alignn_local.h - the entry points of libalignn_hip.so for the local structure analysis of MD trajectories: common-neighbour
 * analysis (fixed cutoff and adaptive) and the bond-orientational order parameters q_l, w_l with their averaged forms of Lechner
 * and Dellago (csrc/local_order.hip; alignn_amd/local_order.py is the driver and binds this header, tests/local_ref.py the numpy
 * restatement).
 *
 * A header added after alignn_order.h, in the same regular form (one extern "C" block, argument structs with a size query each,
 * prototypes over the base types): alignn_amd/_abi.py reads it.  Every pointer is a device pointer; `stream` is a hipStream_t.
 * Every entry point returns 0 or the HIP error; hipErrorInvalidValue (1) for an argument out of its range, before any launch and
 * before any pointer is looked at.  No structures, or no selected frame, is a no-op that returns 0.
 *
 * float64 without contraction, no atomics on floating-point values, every floating-point sum in a fixed order over the atom's own
 * neighbour list: a structure's bits do not depend on the launch it is in, nor on its place in it.
 *
 * The trajectory, the frame selection (frame0 + f * frame_step, f = 0 .. n_frames - 1), the groups (group 0 every atom, groups
 * 1 .. S_b the species in ascending atomic number, group[i] in 1 .. S_b, group_count [B][S + 1]), the cells ([B][3][3] or
 * [n_total_frames][B][3][3]) and the neighbour list are those of alignn_order.h, and so are the limits and the status bits, by
 * value: the list of atom i in a frame is the ordered (j, m), m an image shift, (i, 0) left out, with
 *     df = (r_j - r_i) Cinv;  df -= rint(df);  d0 = df C;  d = d0 + ((m0 C0 + m1 C1) + m2 C2);  r = sqrt((dx dx + dy dy) + dz dz)
 * and r < r_cut[b], over |m_k| <= floor(r_cut / h_k + 1/2), in the order j ascending, then (m0, m1, m2) lexicographic.  A range
 * above ALIGNN_LOCAL_MAX_IMAGE_RANGE (or an r_cut that is not a finite number > 0) sets ALIGNN_LOCAL_STATUS_IMAGES and the frame
 * is skipped (its outputs are not written: the caller zeroes them); more than ALIGNN_LOCAL_MAX_NEIGHBORS entries set
 * ALIGNN_LOCAL_STATUS_NEIGHBORS and that atom's outputs of that frame are zeros (n_neighbors = the number found).
 */
#ifndef ALIGNN_LOCAL_H
#define ALIGNN_LOCAL_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ALIGNN_LOCAL_MAX_SPECIES 8      /* = ALIGNN_ORDER_MAX_SPECIES */
#define ALIGNN_LOCAL_MAX_IMAGE_RANGE 8  /* = ALIGNN_ORDER_MAX_IMAGE_RANGE */
#define ALIGNN_LOCAL_MAX_NEIGHBORS 64   /* = ALIGNN_ORDER_MAX_NEIGHBORS */
#define ALIGNN_LOCAL_MAX_L 12           /* = ALIGNN_ORDER_MAX_L */
#define ALIGNN_LOCAL_MAX_LS 4           /* = ALIGNN_ORDER_MAX_LS */
#define ALIGNN_LOCAL_STATUS_IMAGES 1    /* = ALIGNN_ORDER_STATUS_IMAGES */
#define ALIGNN_LOCAL_STATUS_NEIGHBORS 2 /* = ALIGNN_ORDER_STATUS_NEIGHBORS */
#define ALIGNN_LOCAL_CLASSES 5          /* OTHER 0, FCC 1, HCP 2, BCC 3, ICO 4 */
#define ALIGNN_LOCAL_SIGNATURES 5       /* the signatures counted, in the order 421, 422, 444, 555, 666 */
#define ALIGNN_LOCAL_M_STRIDE 13        /* m = 0 .. ALIGNN_LOCAL_MAX_L: the complex numbers of one degree in qlm */
#define ALIGNN_LOCAL_W3J_STRIDE 625     /* (2 MAX_L + 1)^2: the doubles of one degree in w3j */

/* ------------------------------------------------------------------------------------------
 * Common-neighbour analysis.  All geometry is in the centre atom's local frame, on the displacements d_a of its list entries, so
 * a cell smaller than the cutoff is analysed through its own images.  Of the entries selected (below) two, a != b, are bonded iff
 *     sqrt((ex ex + ey ey) + ez ez) < r_c,   e = d_a - d_b
 * (the square root is compared, as r < r_cut is).  The signature (n_cn, n_b, n_lcb) of a selected entry a: its common neighbours
 * are the selected entries bonded to it (every entry is a neighbour of the centre), n_cn their number, n_b the number of bonded
 * pairs among them, n_lcb the number of bonds of the connected component of that bond graph that has the most bonds.  With Nb
 * the number of selected entries:
 *     Nb = 12, 12 x (4,2,1): FCC (1);   Nb = 12, 6 x (4,2,1) + 6 x (4,2,2): HCP (2);   Nb = 14, 6 x (4,4,4) + 8 x (6,6,6): BCC (3);
 *     Nb = 12, 12 x (5,5,5): ICO (4);   anything else: OTHER (0).
 * adaptive = 0: every entry is selected and r_c = r_cut[b].
 * adaptive = 1 (after Stukowski's adaptive CNA; the rule is this header's): r_cut is the search radius only.  The entries are
 * sorted by r, ties by list order; r_(1) <= r_(2) <= .. are the sorted distances and every sum below runs in that order from 0.
 *     stage 12 (needs 12 entries): the 12 nearest, r_c = ((1 + sqrt 2) / 2) ((r_(1) + .. + r_(12)) / 12); FCC, HCP and ICO are tested.
 *     stage 14 (when stage 12 gave no class; needs 14 entries): the 14 nearest,
 *         r_c = ((1 + sqrt 2) / 2) ((((2 / sqrt 3) (r_(1) + .. + r_(8))) + (r_(9) + .. + r_(14))) / 14); BCC is tested.
 * signature_counts are those of the stage that gave the class, else those of stage 14, else (fewer than 14 entries) zeros.
 *
 * _local_cna: one wavefront per (frame, centre atom), four wavefronts per workgroup; the list by ballot and prefix into LDS, lane
 * a owns entry a and its 64-bit mask of bonded entries.  structure, signature_counts and n_neighbors are written.
 * _local_cna_counts: counts[b][a][f][c] = the atoms of group a (0: all) of structure b whose class in frame f is c, by integer
 * sums; fraction = counts / N_a (a group without members: 0).
 * ------------------------------------------------------------------------------------------ */
typedef struct alignn_local_cna_args {
    const double* traj;         /* [n_total_frames][n_atoms][3]   (_local_cna) */
    const double* lattice;      /* [B][3][3] (lattice_per_frame 0) or [n_total_frames][B][3][3] (1), row-major   (_local_cna) */
    const int32_t* atom_ptr;    /* [B + 1], 0 first */
    const int32_t* group;       /* [n_atoms] */
    const int32_t* group_count; /* [B][S + 1] */
    const double* r_cut;        /* [B]   (_local_cna) */
    int32_t* structure;         /* [n_frames][n_atoms]   (these three: _local_cna writes every element of a frame without
                                 * ALIGNN_LOCAL_STATUS_IMAGES - a skipped frame is left to the caller's zeros; _local_cna_counts reads structure) */
    int32_t* signature_counts;  /* [n_frames][n_atoms][ALIGNN_LOCAL_SIGNATURES] */
    int32_t* n_neighbors;       /* [n_frames][n_atoms] */
    int64_t* counts;            /* [B][S + 1][n_frames][ALIGNN_LOCAL_CLASSES]   (_local_cna_counts writes every element of these two) */
    double* fraction;           /* [B][S + 1][n_frames][ALIGNN_LOCAL_CLASSES]   (_local_cna_counts) */
    int32_t* status;            /* [1], bits are ORed in (_local_cna) */
    int n_structs;              /* B >= 0 */
    int n_atoms;                /* atom_ptr[B] >= 0 */
    int max_atoms;              /* the largest n_b (sizes the launch), 1 .. n_atoms */
    int n_species;              /* S, 1 .. ALIGNN_LOCAL_MAX_SPECIES */
    int n_total_frames;         /* >= 0 */
    int frame0;                 /* >= 0 */
    int frame_step;             /* >= 1 */
    int n_frames;               /* frames used, >= 0 */
    int lattice_per_frame;      /* 0 / 1 */
    int adaptive;               /* 0 / 1 */
} alignn_local_cna_args;
int alignn_local_cna(const alignn_local_cna_args* args, void* stream);
int alignn_local_cna_counts(const alignn_local_cna_args* args, void* stream);
size_t alignn_local_cna_args_size(void); /* a binding checks its own packing against this */

/* ------------------------------------------------------------------------------------------
 * Bond-orientational order.  With (x, y, z) = (dx / r, dy / r, dz / r) of a list entry, the complex spherical harmonics are
 *     Y_lm = ynorm[l][m] (G_lm(z) (x + i y)^m),   m = 0 .. l,     ynorm[l][m] = sqrt(((2l + 1) (l - m)! / (l + m)!) / (4 pi))
 * a polynomial in z times a power of (x + i y), no division by sin theta: (x + i y)^0 = 1, (x + i y)^(m+1) = (x + i y)^m (x + i y)
 * (re = ar x - ai y, im = ar y + ai x) and, G_lm being P_l^m(z) / sin^m theta with the Condon-Shortley phase,
 *     G_00 = 1;  G_mm = -(2m - 1) G_(m-1)(m-1);  G_(m+1)m = ((2m + 1) z) G_mm;  G_lm = (((2l - 1) z) G_(l-1)m - (l + m - 1) G_(l-2)m) / (l - m)
 * Only m >= 0 is stored: q_(l,-m) = (-1)^m conj(q_lm).  Per atom i with Nb list entries, per degree l of l0 .. (the first n_ls):
 *     q_lm(i) = (sum over the entries of Y_lm) / Nb, re and im each lane-wise then by the xor butterfly; Nb = 0: 0
 *     qbar_lm(i) = (q_lm(i) + sum over the entries (j, m) of i of q_lm(j)) / (Nb + 1), the sum by the same butterfly; every entry
 *         counts once, the same j through several images and i through its own images included
 *     s_l = |q_l0|^2 + 2 |q_l1|^2 + .. + 2 |q_ll|^2 in that order, |.|^2 = re re + im im;   q_l = sqrt(((4 pi) / (2l + 1)) s_l)
 *     t_l = sum over (m1, m2), m3 = -(m1 + m2), of w3j[m1 + l][m2 + l] Re((q_lm1 q_lm2) q_lm3), the index (m1 + l) (2l + 1) +
 *         (m2 + l) lane-strided in ascending order, then the xor butterfly; w_l = t_l / (s_l sqrt(s_l)), s_l = 0: 0
 * and sbar, tbar, qbar_l, wbar_l the same on qbar_lm.  w3j [n_ls][ALIGNN_LOCAL_W3J_STRIDE]: per degree the Wigner 3j symbols
 * (l l l; m1 m2 m3) at [(m1 + l) (2l + 1) + (m2 + l)], zero where |m1 + m2| > l; ynorm [MAX_L + 1][ALIGNN_LOCAL_M_STRIDE]; both
 * are built on the host.
 *
 * Two passes over a chunk of frames, f = chunk0 .. chunk0 + chunk_frames - 1 of the frames used, so that neither the lists nor the
 * q_lm of a whole trajectory are stored: qlm [chunk_frames][n_atoms][n_ls][ALIGNN_LOCAL_M_STRIDE][2] is the scratch of one chunk.
 * _local_bond_qlm (pass 1): one wavefront per (frame, atom), lanes over the entries; writes qlm and n_neighbors.
 * _local_bond_finish (pass 2): rebuilds the same list (average = 1), gathers q_lm(j), writes s, t, q, w and, with average = 1,
 * s_avg, t_avg, q_avg, w_avg, each [n_frames][n_atoms][n_ls].
 * ------------------------------------------------------------------------------------------ */
typedef struct alignn_local_bond_args {
    const double* traj;         /* [n_total_frames][n_atoms][3] */
    const double* lattice;      /* [B][3][3] (lattice_per_frame 0) or [n_total_frames][B][3][3] (1), row-major */
    const int32_t* atom_ptr;    /* [B + 1], 0 first */
    const int32_t* group;       /* [n_atoms] */
    const int32_t* group_count; /* [B][S + 1] */
    const double* r_cut;        /* [B] */
    const double* ynorm;        /* [ALIGNN_LOCAL_MAX_L + 1][ALIGNN_LOCAL_M_STRIDE]   (_local_bond_qlm) */
    const double* w3j;          /* [n_ls][ALIGNN_LOCAL_W3J_STRIDE]   (_local_bond_finish) */
    double* qlm;                /* [chunk_frames][n_atoms][n_ls][ALIGNN_LOCAL_M_STRIDE][2] */
    double* s;                  /* [n_frames][n_atoms][n_ls]   (these eight: _local_bond_finish writes the frames of the chunk that have no
                                 * ALIGNN_LOCAL_STATUS_IMAGES; a skipped frame is left to the caller's zeros) */
    double* t;
    double* q;
    double* w;
    double* s_avg;              /* with average = 1 */
    double* t_avg;
    double* q_avg;
    double* w_avg;
    int32_t* n_neighbors;       /* [n_frames][n_atoms]   (_local_bond_qlm writes the frames of the chunk that are not skipped) */
    int32_t* status;            /* [1], bits are ORed in (_local_bond_qlm) */
    int n_structs;              /* B >= 0 */
    int n_atoms;                /* atom_ptr[B] >= 0 */
    int max_atoms;              /* the largest n_b (sizes the launch), 1 .. n_atoms */
    int n_species;              /* S, 1 .. ALIGNN_LOCAL_MAX_SPECIES */
    int n_total_frames;         /* >= 0 */
    int frame0;                 /* >= 0 */
    int frame_step;             /* >= 1 */
    int n_frames;               /* frames used, >= 0 */
    int lattice_per_frame;      /* 0 / 1 */
    int chunk0;                 /* the first frame used of this chunk, 0 .. n_frames */
    int chunk_frames;           /* 0 .. n_frames - chunk0 */
    int average;                /* 0 / 1 */
    int n_ls;                   /* 1 .. ALIGNN_LOCAL_MAX_LS */
    int l0;                     /* the degrees: the first n_ls are read, each 1 .. ALIGNN_LOCAL_MAX_L, distinct */
    int l1;
    int l2;
    int l3;
} alignn_local_bond_args;
int alignn_local_bond_qlm(const alignn_local_bond_args* args, void* stream);
int alignn_local_bond_finish(const alignn_local_bond_args* args, void* stream);
size_t alignn_local_bond_args_size(void);

#ifdef __cplusplus
}
#endif
#endif /* ALIGNN_LOCAL_H */
