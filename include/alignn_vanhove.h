/* alignn_vanhove.h - the entry points of libalignn_hip.so for the time-dependent pair correlations of MD trajectories: the self
 * and the distinct part of the van Hove function and the coherent intermediate scattering function (csrc/vanhove.hip;
 * alignn_amd/vanhove.py is the driver and binds this header, tests/vanhove_ref.py the numpy restatement).
 *
 * A header of its own beside alignn_traj.h, in the same regular form (one extern "C" block, argument structs, prototypes over the
 * base types): alignn_amd/_abi.py reads it.  `stream` is a hipStream_t.  Every pointer is a device pointer but `lags_host`, which
 * is the one array the entry points read themselves.  Every entry point returns 0 or the HIP error; hipErrorInvalidValue (1) for an
 * argument out of its range or a needed pointer that is NULL, before any launch and before any pointer is followed.  No structures
 * or no selected frames is a no-op that returns 0.
 *
 * float64 without contraction, no atomics on floating-point values (the histograms are summed with integer atomics: exact and
 * independent of the order), every floating-point sum in a fixed order over the structure's own rows and frames: a structure's
 * bits do not depend on the launch it is in, nor on its place in it.
 *
 * The trajectory, the frame selection (frame0 + f * frame_step, f = 0 .. n_frames - 1; frames t below count the frames USED), the
 * groups (group 0 every atom, groups 1 .. S_b the species in ascending atomic number, S <= ALIGNN_VH_MAX_SPECIES, group[i] in
 * 1 .. S_b, group_count [B][S + 1]) and the pair rows (row 0 every pair, row 1 + b (b - 1) / 2 + (a - 1) the groups a <= b,
 * P = 1 + S (S + 1) / 2) are those of alignn_traj.h.  Rows of an output that belong to a group without members are zero.
 *
 * Lags.  lags_host [n_lags] (host memory) and lags [n_lags] (its copy on the device, which the kernels read) hold the lags k_0 <
 * k_1 < ..., each 0 .. n_frames - 1, 1 .. ALIGNN_VH_MAX_LAGS of them; an entry point checks lags_host before it launches.  The
 * origins of lag k are t = 0, origin_stride, 2 origin_stride, ... with t + k <= n_frames - 1, n_origins(k) = (n_frames - 1 - k) /
 * origin_stride + 1 of them (>= 1).
 *
 * Centre of mass.  com [n_frames][B][3] is what alignn_traj_com writes (alignn_traj.h); com = NULL: c = 0.
 */
#ifndef ALIGNN_VANHOVE_H
#define ALIGNN_VANHOVE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ALIGNN_VH_MAX_SPECIES 8     /* species per structure */
#define ALIGNN_VH_MAX_BINS 4096     /* bins of r */
#define ALIGNN_VH_MAX_IMAGE_RANGE 8 /* |m_k| of a periodic image, per axis */
#define ALIGNN_VH_MAX_LAGS 1024     /* lags per call */
#define ALIGNN_VH_MAX_Q 16          /* magnitudes q of the self intermediate scattering function per call */
#define ALIGNN_VH_STATUS_IMAGES 1   /* bit of *status: a cell needs images beyond the range (or is singular) */

/* ------------------------------------------------------------------------------------------
 * _vh_self / _vh_self_finish: the self part.  For every structure, lag k = lags[l], origin t and atom i:
 *     d = (r_i(t + k) - r_i(t)) - (c(t + k) - c(t));   r2 = (dx dx + dy dy) + dz dz;   r = sqrt(r2)
 * counts [B][S + 1][L][n_bins]: the terms with r < r_max, in bin floor(r (n_bins / r_max)); overflow [B][S + 1][L]: those with
 * r >= r_max, so that counts summed over the bins + overflow = n_origins(k) N_a exactly.  _vh_self ADDS to both (the caller
 * zeroes them); row 0 is the sum of the species rows.
 * sums [B][S + 1][L][2]: the sums of r2 and of r2 r2 over the origins and the group's rows; fs_sum [B][S + 1][L][n_q]: the sums
 * of j0(q_u r), j0(x) = sin(x) / x and j0(0) = 1, x = q_u r.  _vh_self writes every element of both.  One workgroup of 256
 * threads per (lag, structure): a thread sums its row over the origins in order, the rows of a group are then summed in the
 * order of alignn_traj_corr (chunks of 256 rows in order; in a chunk a lane's four rows in order, then the xor butterfly).
 * The workgroup bins into an LDS histogram of 32-bit counts (at most 14336 of them: more species than fit are walked in
 * chunks), which it adds to counts with 64-bit integer atomics, at the end and before its terms could reach 2^31.
 *
 * _vh_self_finish, with n = n_origins(k), N_a the members of the group, dr = r_max / n_bins, r_j = j dr:
 *     moments[0] = sums[0] / (n N_a);  moments[1] = sums[1] / (n N_a)              <r^2>, <r^4>
 *     alpha2  = (3 moments[1]) / (5 (moments[0] moments[0])) - 1                   (0 where moments[0] = 0)
 *     p[j]    = counts[j] / ((n N_a) dr)                                           the radial density 4 pi r^2 G_s
 *     gs[j]   = counts[j] / ((n N_a) (4 pi / 3 (r_{j+1}^3 - r_j^3)))               G_s
 *     fs[u]   = fs_sum[u] / (n N_a)
 *     centres[j] = (j + 1/2) dr
 * ------------------------------------------------------------------------------------------ */
typedef struct alignn_vh_self_args {
    const double* traj;         /* [n_total_frames][n_atoms][3]   (_vh_self) */
    const int32_t* atom_ptr;    /* [B + 1], 0 first   (_vh_self) */
    const int32_t* group;       /* [n_atoms]   (_vh_self) */
    const int32_t* group_count; /* [B][S + 1] */
    const double* com;          /* [n_frames][B][3], or NULL   (_vh_self) */
    const int32_t* lags;        /* [n_lags], on the device */
    const int32_t* lags_host;   /* [n_lags], in host memory: what the entry points check */
    const double* q;            /* [n_q], each finite and > 0; not looked at with n_q = 0   (_vh_self) */
    int64_t* counts;            /* [B][S + 1][L][n_bins]   (_vh_self adds, _vh_self_finish reads) */
    int64_t* overflow;          /* [B][S + 1][L]           (_vh_self adds) */
    double* sums;               /* [B][S + 1][L][2]        (_vh_self writes, _vh_self_finish reads) */
    double* fs_sum;             /* [B][S + 1][L][n_q]      (_vh_self writes, _vh_self_finish reads; not looked at with n_q = 0) */
    double* moments;            /* [B][S + 1][L][2]        (these six: _vh_self_finish) */
    double* alpha2;             /* [B][S + 1][L] */
    double* p;                  /* [B][S + 1][L][n_bins] */
    double* gs;                 /* [B][S + 1][L][n_bins] */
    double* fs;                 /* [B][S + 1][L][n_q]; not looked at with n_q = 0 */
    double* centres;            /* [n_bins] */
    double r_max;               /* finite, > 0 */
    int n_structs;              /* B >= 0 */
    int n_atoms;                /* atom_ptr[B] >= 0 */
    int n_species;              /* S, 1 .. ALIGNN_VH_MAX_SPECIES */
    int n_bins;                 /* 1 .. ALIGNN_VH_MAX_BINS */
    int n_total_frames;         /* >= 0 */
    int frame0;                 /* >= 0 */
    int frame_step;             /* >= 1 */
    int n_frames;               /* frames used, >= 0 */
    int n_lags;                 /* L, 1 .. ALIGNN_VH_MAX_LAGS */
    int origin_stride;          /* >= 1 */
    int n_q;                    /* 0 .. ALIGNN_VH_MAX_Q */
} alignn_vh_self_args;
int alignn_vh_self(const alignn_vh_self_args* args, void* stream);
int alignn_vh_self_finish(const alignn_vh_self_args* args, void* stream);
size_t alignn_vh_self_args_size(void); /* a binding checks its own packing against this */

/* ------------------------------------------------------------------------------------------
 * _vh_distinct / _vh_distinct_finish: the distinct part, in one fixed cell per structure (lattice_per_frame must be 0: a
 * difference between two frames has no single cell).  For every lag k, origin t and ordered (i, j, image m), with C the cell,
 * Cinv its inverse by cofactors (csrc/cell3.h) and x M = (x0 M0 + x1 M1) + x2 M2:
 *     D = (r_j(t + k) - c(t + k)) - (r_i(t) - c(t));  df = D Cinv;  n = rint(df);  df -= n;  d0 = df C
 *     d = d0 + ((m0 C0 + m1 C1) + m2 C2);  r = sqrt((dx dx + dy dy) + dz dz)
 * over |m_k| <= floor(r_max / h_k + 1/2), h_k the cell's heights: the arithmetic of alignn_traj_rdf_counts.  A range above
 * ALIGNN_VH_MAX_IMAGE_RANGE sets ALIGNN_VH_STATUS_IMAGES in *status and the structure is not counted.  For j = i the image m = n
 * (component for component) is left out: d0 + n C = D, the atom's own unwrapped displacement, the self part.  Every other image of
 * i counts, the wrapped one (m = 0) among them when the atom has left its cell; at k = 0 exactly (i, i, 0) is left out.  Terms
 * with r >= r_max are dropped; the others fall into bin
 * floor(r (n_bins / r_max)) of the row of (group of i, group of j), both orders in a row a < b.
 *
 * counts [B][P][L][n_bins]: _vh_distinct ADDS to it (the caller zeroes it); row 0 is the sum of the others.  One workgroup of 256
 * threads per (lag, tile of 64 rows i, structure): per origin, j of frame t + k in tiles of 64 through LDS against the tile of i
 * of frame t.  The workgroup keeps an LDS histogram of 32-bit counts (at most 14336: more pair rows than fit are walked in
 * chunks) over all its origins and adds the non-zero bins to counts with 64-bit integer atomics once, or before its terms could
 * reach 2^31.
 *
 * _vh_distinct_finish, with V = |det C|, n = n_origins(k), w = 2 for a < b and 1 otherwise (row 0: a = b = group 0):
 *     g[j] = (counts[j] V) / ((((n N_a) N_b) w) (4 pi / 3 (r_{j+1}^3 - r_j^3)));  volume[b] = V;  centres[j] = (j + 1/2) dr
 * At lag 0 and origin_stride 1 this is the g(r) of alignn_traj_rdf_normalise.
 * ------------------------------------------------------------------------------------------ */
typedef struct alignn_vh_distinct_args {
    const double* traj;         /* [n_total_frames][n_atoms][3]   (_vh_distinct) */
    const double* lattice;      /* [B][3][3], row-major */
    const int32_t* atom_ptr;    /* [B + 1], 0 first   (_vh_distinct) */
    const int32_t* group;       /* [n_atoms]   (_vh_distinct) */
    const int32_t* group_count; /* [B][S + 1] */
    const double* com;          /* [n_frames][B][3], or NULL   (_vh_distinct) */
    const int32_t* lags;        /* [n_lags], on the device */
    const int32_t* lags_host;   /* [n_lags], in host memory: what the entry points check */
    int64_t* counts;            /* [B][P][L][n_bins]   (_vh_distinct adds, _vh_distinct_finish reads) */
    double* g;                  /* [B][P][L][n_bins]   (_vh_distinct_finish) */
    double* volume;             /* [B]                 (_vh_distinct_finish) */
    double* centres;            /* [n_bins]            (_vh_distinct_finish) */
    int32_t* status;            /* [1], bits are ORed in (_vh_distinct) */
    double r_max;               /* finite, > 0 */
    int n_structs;              /* B >= 0 */
    int n_atoms;                /* atom_ptr[B] >= 0 */
    int max_atoms;              /* the largest n_b (sizes the launch), 1 .. n_atoms   (_vh_distinct) */
    int n_species;              /* S, 1 .. ALIGNN_VH_MAX_SPECIES */
    int n_bins;                 /* 1 .. ALIGNN_VH_MAX_BINS */
    int n_total_frames;         /* >= 0 */
    int frame0;                 /* >= 0 */
    int frame_step;             /* >= 1 */
    int n_frames;               /* frames used, >= 0 */
    int n_lags;                 /* L, 1 .. ALIGNN_VH_MAX_LAGS */
    int origin_stride;          /* >= 1 */
    int lattice_per_frame;      /* 0: one cell per structure; anything else is refused */
} alignn_vh_distinct_args;
int alignn_vh_distinct(const alignn_vh_distinct_args* args, void* stream);
int alignn_vh_distinct_finish(const alignn_vh_distinct_args* args, void* stream);
size_t alignn_vh_distinct_args_size(void);

/* ------------------------------------------------------------------------------------------
 * _vh_fqt_modes / _vh_fqt_correlate / _vh_fqt_bin: the coherent intermediate scattering function of fixed cells
 * (lattice_per_frame must be 0), on the reciprocal-lattice vectors of the static structure factor: vec_ptr, hkl and vbin are what
 * alignn_order_sq_vectors writes for the same lattice, q_max and n_bins (alignn_order.h: the half space, the order, |h_k| <=
 * ALIGNN_VH_MAX_HKL, the shells).
 *
 * _vh_fqt_modes.  modes [n_frames][S][n_vectors][2]: (re, im) of rho_a(q, t) = sum_{i in a} exp(2 pi i h . f_i(t)), a = 1 .. S,
 * for every frame used and every vector, formed as alignn_order_sq_accumulate forms them (csrc/sq_modes.h, shared): f_k = x -
 * floor(x), x = (r Cinv)_k; sincospi(2 (h f_k)) tabulated per axis in LDS; two complex products; the atoms in row order.  It
 * writes every element.  One workgroup of 256 threads per (256 w vectors, chunk of ALIGNN_VH_FQT_FRAME_CHUNK frames, structure).
 *
 * _vh_fqt_correlate.  f_vec [P][L][n_vectors], per (vector, lag) one thread, the origins t summed in order; with rho = rho(t),
 * rho' = rho(t + k), n = n_origins(k), and every product written out as rho.re rho'.re + rho.im rho'.im:
 *     row (a, a):        sum_t (rho_a.re rho'_a.re + rho_a.im rho'_a.im) / (n sqrt(N_a N_a))
 *     row (a, b), a < b: sum_t 0.5 ((rho_b.re rho'_a.re + rho_b.im rho'_a.im) + (rho_a.re rho'_b.re + rho_a.im rho'_b.im)) / (n sqrt(N_a N_b))
 *     row 0:             sum_t (R.re R'.re + R.im R'.im) / (n sqrt(N N)),   R = (rho_1 + rho_2) + ... in group order
 * (Ashcroft-Langreth; an empty group: 0).  At lag 0 and origin_stride 1 the terms are those of alignn_order_sq_accumulate.
 *
 * _vh_fqt_bin.  One wavefront per (64 bins, (row, lag), structure) walks the structure's vectors in order: f[b][p][l][j] = the mean
 * of f_vec[p][l] over the vectors of shell j (their sum in list order / their number; no vectors: 0), n_vectors_bin[b][j] their
 * number, centres[j] = (j + 1/2) (q_max / n_bins).
 * ------------------------------------------------------------------------------------------ */
#define ALIGNN_VH_MAX_HKL 32         /* |h_k| of a reciprocal vector, per axis: ALIGNN_ORDER_MAX_HKL */
#define ALIGNN_VH_MAX_Q_BINS 1024    /* shells of |q|: ALIGNN_ORDER_MAX_BINS */
#define ALIGNN_VH_FQT_FRAME_CHUNK 64 /* frames used per workgroup of _vh_fqt_modes */
typedef struct alignn_vh_fqt_args {
    const double* traj;         /* [n_total_frames][n_atoms][3]   (_vh_fqt_modes) */
    const double* lattice;      /* [B][3][3], row-major   (_vh_fqt_modes) */
    const int32_t* atom_ptr;    /* [B + 1], 0 first   (_vh_fqt_modes) */
    const int32_t* group;       /* [n_atoms]   (_vh_fqt_modes) */
    const int32_t* group_count; /* [B][S + 1]   (_vh_fqt_correlate) */
    const int32_t* vec_ptr;     /* [B + 1], 0 first */
    const int32_t* hkl;         /* [n_vectors][3]   (_vh_fqt_modes) */
    const int32_t* vbin;        /* [n_vectors]   (_vh_fqt_bin) */
    const int32_t* lags;        /* [n_lags], on the device   (_vh_fqt_correlate) */
    const int32_t* lags_host;   /* [n_lags], in host memory: what the entry points check */
    double* modes;              /* [n_frames][S][n_vectors][2]   (_vh_fqt_modes writes, _vh_fqt_correlate reads) */
    double* f_vec;              /* [P][L][n_vectors]   (_vh_fqt_correlate writes, _vh_fqt_bin reads) */
    double* f;                  /* [B][P][L][n_bins]   (_vh_fqt_bin) */
    int64_t* n_vectors_bin;     /* [B][n_bins]         (_vh_fqt_bin) */
    double* centres;            /* [n_bins]            (_vh_fqt_bin) */
    double q_max;               /* finite, > 0 */
    int n_structs;              /* B >= 0 */
    int n_atoms;                /* atom_ptr[B] >= 0 */
    int n_species;              /* S, 1 .. ALIGNN_VH_MAX_SPECIES */
    int n_bins;                 /* 1 .. ALIGNN_VH_MAX_Q_BINS */
    int n_total_frames;         /* >= 0 */
    int frame0;                 /* >= 0 */
    int frame_step;             /* >= 1 */
    int n_frames;               /* frames used, >= 0 */
    int n_lags;                 /* L, 1 .. ALIGNN_VH_MAX_LAGS */
    int origin_stride;          /* >= 1 */
    int n_vectors;              /* vec_ptr[B] >= 0 */
    int max_vectors;            /* the largest number of vectors of a structure (sizes the launches), 0 .. n_vectors */
    int lattice_per_frame;      /* 0: one cell per structure; anything else is refused */
} alignn_vh_fqt_args;
int alignn_vh_fqt_modes(const alignn_vh_fqt_args* args, void* stream);
int alignn_vh_fqt_correlate(const alignn_vh_fqt_args* args, void* stream);
int alignn_vh_fqt_bin(const alignn_vh_fqt_args* args, void* stream);
size_t alignn_vh_fqt_args_size(void);

#ifdef __cplusplus
}
#endif
#endif /* ALIGNN_VANHOVE_H */
