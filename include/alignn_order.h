/* alignn_order.h - the entry points of libalignn_hip.so for the structural order analysis of MD trajectories: bond-angle
 * distributions, Steinhardt q_l and the static structure factor (csrc/order.hip; alignn_amd/order.py is the driver and binds
 * this header, tests/order_ref.py the numpy restatement).
 *
 * A header of its own beside alignn_traj.h, in the same regular form (one extern "C" block, argument structs, prototypes over the
 * base types): alignn_amd/_abi.py reads it.  Every pointer is a device pointer; `stream` is a hipStream_t.  Every entry point
 * returns 0 or the HIP error; hipErrorInvalidValue (1) for an argument out of its range, before any launch.  No structures is a
 * no-op that returns 0, and so is no selected frame for the entry points that walk the frames (_order_angles,
 * _order_steinhardt_mean, _order_sq_accumulate).
 *
 * float64 without contraction, no atomics on floating-point values (the angle histogram is summed with integer atomics: exact and
 * independent of the order), every floating-point sum in a fixed order over the structure's own rows, frames and vectors: a
 * structure's bits do not depend on the launch it is in, nor on its place in it.
 *
 * The trajectory, the frame selection (frame0 + f * frame_step, f = 0 .. n_frames - 1), the groups (group 0 every atom, groups
 * 1 .. S_b the species in ascending atomic number, S <= ALIGNN_ORDER_MAX_SPECIES, group[i] in 1 .. S_b, group_count [B][S + 1])
 * and the pair rows (row 0 every pair, row 1 + b (b - 1) / 2 + (a - 1) the groups a <= b) are those of alignn_traj.h.
 */
#ifndef ALIGNN_ORDER_H
#define ALIGNN_ORDER_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ALIGNN_ORDER_MAX_SPECIES 8      /* species per structure */
#define ALIGNN_ORDER_MAX_IMAGE_RANGE 8  /* |m_k| of a periodic image, per axis */
#define ALIGNN_ORDER_MAX_NEIGHBORS 64   /* neighbours (j, image) of one atom inside r_cut */
#define ALIGNN_ORDER_MAX_BINS 1024      /* bins of the angle distribution and of S(q) */
#define ALIGNN_ORDER_MAX_L 12           /* degree l of a Steinhardt parameter */
#define ALIGNN_ORDER_MAX_LS 4           /* degrees per call */
#define ALIGNN_ORDER_MAX_HKL 32         /* |h_k| of a reciprocal vector, per axis */
#define ALIGNN_ORDER_SQ_FRAME_CHUNK 64  /* frames used per partial sum of S(q) */
#define ALIGNN_ORDER_STATUS_IMAGES 1    /* bit of *status: a frame's cell needs images beyond the range (or is singular) */
#define ALIGNN_ORDER_STATUS_NEIGHBORS 2 /* bit of *status: an atom has more than ALIGNN_ORDER_MAX_NEIGHBORS neighbours */
#define ALIGNN_ORDER_STATUS_HKL 4       /* bit of *status: q_max needs |h_k| beyond ALIGNN_ORDER_MAX_HKL (or the cell is singular) */

/* ------------------------------------------------------------------------------------------
 * _order_angles: the neighbour shell of every atom and the walk over its triplets; two optional outputs, the angle histogram
 * (counts) and the Steinhardt parameters (q, n_neighbors).
 *
 * The neighbours of atom i in a frame are the ordered (j, m), m an image shift, (i, 0) left out, with r < r_cut[b].  With C the
 * frame's cell, Cinv its inverse by cofactors (csrc/cell3.h) and x M = (x0 M0 + x1 M1) + x2 M2:
 *     df = (r_j - r_i) Cinv;  df -= rint(df);  d0 = df C;  d = d0 + ((m0 C0 + m1 C1) + m2 C2);  r = sqrt((dx dx + dy dy) + dz dz)
 * over |m_k| <= floor(r_cut / h_k + 1/2), h_k the cell's heights, from each frame's own cell.  A range above
 * ALIGNN_ORDER_MAX_IMAGE_RANGE (or an r_cut that is not a finite number > 0) sets ALIGNN_ORDER_STATUS_IMAGES and the frame is not
 * counted.  The list is in the order j ascending, then (m0, m1, m2) lexicographic; more than ALIGNN_ORDER_MAX_NEIGHBORS entries
 * set ALIGNN_ORDER_STATUS_NEIGHBORS and that atom of that frame is not counted (q = 0, n_neighbors = the number found).
 *
 * For every unordered pair j < k of the Nb list entries:
 *     c = ((dxj dxk + dyj dyk) + dzj dzk) / (rj rk), clamped to [-1, 1]
 * counts (when not NULL): theta = acos(c) falls into bin min(floor(theta (n_bins / pi)), n_bins - 1) of row
 * [b][a][p], a the centre's group and p the pair row of the two neighbours' groups, both >= 1.  _order_angles ADDS to counts
 * (the caller zeroes it) and touches no row with a = 0 or p = 0.
 * q (when not NULL), per degree l of l0 .. (the first n_ls of them), P_l by P_{n+1} = ((2n + 1) c P_n - n P_{n-1}) / (n + 1):
 *     q[f][i][.] = sqrt(max(0, (Nb + 2 sum_{j<k} P_l(c_jk)) / (Nb Nb)));  Nb = 0: 0
 * the pair sum lane-strided over the pair index k (k - 1) / 2 + j in ascending order, then the xor butterfly.
 *
 * One workgroup of four wavefronts per (chunk of 64 frames used, centre atom, structure), a wavefront per frame: the lanes scan
 * the (j, image) candidates and compact the hits into a list in LDS by ballot and prefix, then share the pairs.  The workgroup
 * bins into an LDS histogram of 32-bit counts (at most 4096 of them: more pair rows than fit are walked in chunks) and adds its
 * non-zero bins to counts with integer atomic adds.
 * ------------------------------------------------------------------------------------------ */
typedef struct alignn_order_angle_args {
    const double* traj;         /* [n_total_frames][n_atoms][3]   (_order_angles) */
    const double* lattice;      /* [B][3][3] (lattice_per_frame 0) or [n_total_frames][B][3][3] (1), row-major   (_order_angles) */
    const int32_t* atom_ptr;    /* [B + 1], 0 first   (these three: _order_angles, _order_steinhardt_mean) */
    const int32_t* group;       /* [n_atoms] */
    const int32_t* group_count; /* [B][S + 1] */
    const double* r_cut;        /* [B]   (_order_angles) */
    int64_t* counts;            /* [B][S + 1][P][n_bins], or NULL   (_order_angles adds; _order_adf_finish writes the marginal rows) */
    double* adf;                /* [B][S + 1][P][n_bins]   (_order_adf_finish) */
    double* theta;              /* [n_bins]                (_order_adf_finish) */
    double* q;                  /* [n_frames][n_atoms][n_ls], or NULL   (_order_angles writes every element of a frame without
                                 * ALIGNN_ORDER_STATUS_IMAGES - a frame that is not counted is left to the caller's zeros; _order_steinhardt_mean reads) */
    int32_t* n_neighbors;       /* [n_frames][n_atoms]     (with q: _order_angles writes it where it writes q) */
    double* mean;               /* [B][S + 1][n_frames][n_ls]   (_order_steinhardt_mean) */
    int32_t* status;            /* [1], bits are ORed in (_order_angles) */
    int n_structs;              /* B >= 0 */
    int n_atoms;                /* atom_ptr[B] >= 0 */
    int max_atoms;              /* the largest n_b (sizes the launch), 1 .. n_atoms */
    int n_species;              /* S, 1 .. ALIGNN_ORDER_MAX_SPECIES */
    int n_bins;                 /* 1 .. ALIGNN_ORDER_MAX_BINS */
    int n_total_frames;         /* >= 0 */
    int frame0;                 /* >= 0 */
    int frame_step;             /* >= 1 */
    int n_frames;               /* frames used, >= 0 */
    int lattice_per_frame;      /* 0 / 1 */
    int n_ls;                   /* 0 .. ALIGNN_ORDER_MAX_LS; >= 1 with q */
    int l0;                     /* the degrees: the first n_ls are read, each 1 .. ALIGNN_ORDER_MAX_L, distinct */
    int l1;
    int l2;
    int l3;
} alignn_order_angle_args;
int alignn_order_angles(const alignn_order_angle_args* args, void* stream);

/* _order_adf_finish: the marginal rows of counts by integer sums, counts[b][a][0] = sum_{p >= 1} counts[b][a][p] for a >= 1, then
 * counts[b][0][p] = sum_{a >= 1} counts[b][a][p] for every p; and, with T the sum of a row over its bins and w = 180 / n_bins,
 *     adf[k] = counts[k] / (T w)   (a row with T = 0: zeros);   theta[k] = (k + 1/2) w   in degrees */
int alignn_order_adf_finish(const alignn_order_angle_args* args, void* stream);

/* _order_steinhardt_mean: mean[b][a][f][.] = (sum_{i in a} q[f][i][.]) / N_a (a group without members: 0), the rows summed in the
 * order of alignn_traj_corr: chunks of 256 rows in order; in a chunk a lane's four rows in order, then the xor butterfly. */
int alignn_order_steinhardt_mean(const alignn_order_angle_args* args, void* stream);
size_t alignn_order_angle_args_size(void); /* a binding checks its own packing against this */

/* ------------------------------------------------------------------------------------------
 * The static structure factor of fixed cells.  With Cinv the inverse of structure b's cell, the vectors of b are the integer
 * triples h of the half space (h0 > 0; or h0 = 0 and h1 > 0; or h0 = h1 = 0 and h2 > 0) with |h_k| <= H_k =
 * floor(q_max |C_k| / (2 pi)), |C_k| the length of row k, and |q| < q_max,
 *     q_c = (2 pi) ((h0 Cinv[c][0] + h1 Cinv[c][1]) + h2 Cinv[c][2]);  |q| = sqrt((qx qx + qy qy) + qz qz)
 * in lexicographic order of (h0, h1, h2).  H_k > ALIGNN_ORDER_MAX_HKL sets ALIGNN_ORDER_STATUS_HKL and b has no vectors.
 *
 * _order_sq_vectors, one wavefront per structure.  hkl = NULL: n_vec[b] = the number of b's vectors.  Else, vec_ptr [B + 1] being
 * the running sum of those numbers: hkl, qnorm = |q| and vbin = min(floor(|q| (n_bins / q_max)), n_bins - 1) of b's vectors at
 * vec_ptr[b] ..
 *
 * _order_sq_accumulate.  Per frame and atom f_k = (r Cinv)_k - floor((r Cinv)_k); per vector
 *     rho_a = sum_{i in a} (e_0(h0) e_1(h1)) e_2(h2),  a = 1 .. S, in row order;   rho_0 = (rho_1 + rho_2) + ...
 *     e_k(h) = exp(i pi (2 (h f_k)))  by sincospi for h >= 0,  e_k(-h) its conjugate
 * and row p of the frame is Re(rho_a rho_b*) = rho_a.re rho_b.re + rho_a.im rho_b.im (row 0: a = b = 0).  partial
 * [n_chunks][P][n_vectors], n_chunks = ceil(n_frames / ALIGNN_ORDER_SQ_FRAME_CHUNK): the sum of the rows over the chunk's frames
 * in frame order.  One workgroup of 256 threads per (256 w vectors, chunk, structure), every thread owning w vectors (8 up to
 * two species, else 4): the e_k of 16 atoms at a time are tabulated in LDS for h = -H_k .. H_k (h0 from 0).
 *
 * _order_sq_bin.  s_vec[p][v] = (sum of the chunks' partials in chunk order) / (F sqrt(N_a N_b)) (Ashcroft-Langreth; row 0:
 * N_a = N_b = n_b; no frames or an empty group: 0).  Then one wavefront per (64 bins, row, structure) walks b's vectors in order:
 * s[b][p][k] = the mean of s_vec[p] over the vectors of bin k (their sum in list order / their number; no vectors: 0),
 * n_vectors[b][k] their number, centres[k] = (k + 1/2) (q_max / n_bins).
 * ------------------------------------------------------------------------------------------ */
typedef struct alignn_order_sq_args {
    const double* traj;         /* [n_total_frames][n_atoms][3]   (_order_sq_accumulate) */
    const double* lattice;      /* [B][3][3], row-major   (_order_sq_vectors, _order_sq_accumulate) */
    const int32_t* atom_ptr;    /* [B + 1]   (_order_sq_accumulate) */
    const int32_t* group;       /* [n_atoms]   (_order_sq_accumulate) */
    const int32_t* group_count; /* [B][S + 1]   (_order_sq_bin) */
    const int32_t* vec_ptr;     /* [B + 1], 0 first (not read by the counting call of _order_sq_vectors) */
    int32_t* n_vec;             /* [B]                     (_order_sq_vectors with hkl = NULL) */
    int32_t* hkl;               /* [n_vectors][3], or NULL (these three: _order_sq_vectors with hkl given writes every element;
                                 * _order_sq_accumulate reads hkl, _order_sq_bin reads vbin) */
    double* qnorm;              /* [n_vectors] */
    int32_t* vbin;              /* [n_vectors] */
    double* partial;            /* [n_chunks][P][n_vectors] (_order_sq_accumulate writes every element, _order_sq_bin reads) */
    double* s_vec;              /* [P][n_vectors]          (_order_sq_bin) */
    double* s;                  /* [B][P][n_bins]          (_order_sq_bin) */
    int64_t* n_vectors_bin;     /* [B][n_bins]             (_order_sq_bin) */
    double* centres;            /* [n_bins]                (_order_sq_bin) */
    int32_t* status;            /* [1], bits are ORed in (_order_sq_vectors) */
    double q_max;               /* finite, > 0 */
    int n_structs;              /* B >= 0 */
    int n_atoms;                /* atom_ptr[B] >= 0 */
    int n_species;              /* S, 1 .. ALIGNN_ORDER_MAX_SPECIES */
    int n_bins;                 /* 1 .. ALIGNN_ORDER_MAX_BINS */
    int n_total_frames;         /* >= 0 */
    int frame0;                 /* >= 0 */
    int frame_step;             /* >= 1 */
    int n_frames;               /* frames used, >= 0 */
    int n_vectors;              /* vec_ptr[B] >= 0 */
    int max_vectors;            /* the largest number of vectors of a structure (sizes the launches), 0 .. n_vectors */
} alignn_order_sq_args;
int alignn_order_sq_vectors(const alignn_order_sq_args* args, void* stream);
int alignn_order_sq_accumulate(const alignn_order_sq_args* args, void* stream);
int alignn_order_sq_bin(const alignn_order_sq_args* args, void* stream);
size_t alignn_order_sq_args_size(void);

#ifdef __cplusplus
}
#endif
#endif /* ALIGNN_ORDER_H */
