/* alignn_traj.h - the entry points of libalignn_hip.so for the analysis of MD trajectories (csrc/trajectory.hip;
 * alignn_amd/trajectory.py is the driver and binds this header, tests/traj_ref.py the numpy restatement).
 *
 * A header of its own beside alignn_hip.h, in the same regular form (one extern "C" block, argument structs, prototypes over the
 * base types): alignn_amd/_abi.py reads it.  Every pointer is a device pointer; `stream` is a hipStream_t.  Every entry point
 * returns 0 or the HIP error; hipErrorInvalidValue (1) for an argument out of its range, before any launch.  No structures or no
 * selected frames is a no-op that returns 0.
 *
 * float64 without contraction, no atomics on floating-point values (the pair histogram is summed with integer atomics: exact and
 * independent of the order), every floating-point sum in a fixed order over the structure's own rows and frames: a structure's
 * bits do not depend on the launch it is in, nor on its place in it.
 *
 * The trajectory is what run_md records: [n_total_frames][n_atoms][3] Cartesian, not wrapped, the B structures packed (structure
 * b owns rows [atom_ptr[b], atom_ptr[b + 1])).  The frames used are frame0 + f * frame_step, f = 0 .. n_frames - 1; the last of
 * them must lie below n_total_frames.
 *
 * Groups.  Per structure, group 0 is every atom and groups 1 .. S_b are its species in ascending atomic number; S is the largest
 * S_b of the call, 1 .. ALIGNN_TRAJ_MAX_SPECIES.  group[i] is row i's group, 1 .. S_b; group_count [B][S + 1] holds the members
 * of every group (entry 0: n_b; groups above S_b: 0).  Rows of an output that belong to a group without members are zero.
 */
#ifndef ALIGNN_TRAJ_H
#define ALIGNN_TRAJ_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ALIGNN_TRAJ_MAX_SPECIES 8     /* species per structure */
#define ALIGNN_TRAJ_MAX_BINS 4096     /* bins of g(r) */
#define ALIGNN_TRAJ_MAX_IMAGE_RANGE 8 /* |m_k| of a periodic image, per axis */
#define ALIGNN_TRAJ_STATUS_IMAGES 1   /* bit of *status: a frame's cell needs images beyond the range (or is singular) */

/* ------------------------------------------------------------------------------------------
 * _traj_rdf_counts / _traj_rdf_normalise: the radial distribution function.
 *
 * Pairs are the ordered triples (i, j, m), m an image shift, (i, i, 0) left out.  With C the frame's cell (rows a, b, c), Cinv its
 * inverse by cofactors (csrc/cell3.h) and x M = (x0 M0 + x1 M1) + x2 M2:
 *     df = (r_j - r_i) Cinv;  df -= rint(df);  d0 = df C;  d = d0 + ((m0 C0 + m1 C1) + m2 C2);  r = sqrt((dx dx + dy dy) + dz dz)
 * over |m_k| <= floor(r_max / h_k + 1/2), h_k = |det C| / |C_{k+1} x C_{k+2}| the cell's heights, from each frame's own cell.  A
 * range above ALIGNN_TRAJ_MAX_IMAGE_RANGE sets ALIGNN_TRAJ_STATUS_IMAGES in *status and the frame is not counted.  Pairs with
 * r >= r_max are dropped; the others fall into bin floor(r (n_bins / r_max)).
 *
 * counts [B][P][n_bins], P = 1 + S (S + 1) / 2: row 0 every pair; row 1 + b (b - 1) / 2 + (a - 1) the pairs of groups a <= b
 * (1-based: (1,1), (1,2), (2,2), (1,3), ...), both orders for a < b, so a structure's rows do not depend on the S of the call.
 * _rdf_counts ADDS to counts (the caller zeroes it); row 0 is the sum of the others.  One workgroup of 256 threads per (frame,
 * tile of 64 rows i, structure) walks j in tiles of 64 through LDS and bins into an LDS histogram of 32-bit counts (at most 14336
 * of them: more pair types than fit are walked in chunks), then adds the non-zero bins to counts.
 *
 * _rdf_normalise, with F = n_frames, <V> the mean of |det C| over the frames used (summed in frame order), N_a the members of a
 * group, w = 2 for a < b and 1 otherwise (row 0: a = b = group 0), r_k = k (r_max / n_bins):
 *     g[k]     = (counts[k] <V>) / ((((F N_a) N_b) w) (4 pi / 3 (r_{k+1}^3 - r_k^3)))
 *     coord[k] = (counts[0] + ... + counts[k]) / ((F N_a) w)      the b around an a within r_{k+1}
 *     centres[k] = (k + 1/2) (r_max / n_bins)
 * ------------------------------------------------------------------------------------------ */
typedef struct alignn_traj_rdf_args {
    const double* traj;         /* [n_total_frames][n_atoms][3]   (_rdf_counts) */
    const double* lattice;      /* [B][3][3] (lattice_per_frame 0) or [n_total_frames][B][3][3] (1), row-major */
    const int32_t* atom_ptr;    /* [B + 1], 0 first   (_rdf_counts) */
    const int32_t* group;       /* [n_atoms]   (_rdf_counts) */
    const int32_t* group_count; /* [B][S + 1] */
    int64_t* counts;            /* [B][P][n_bins]   (_rdf_counts adds, _rdf_normalise reads) */
    double* g;                  /* [B][P][n_bins]   (_rdf_normalise) */
    double* coord;              /* [B][P][n_bins]   (_rdf_normalise) */
    double* volume;             /* [B] <V>          (_rdf_normalise) */
    double* centres;            /* [n_bins]         (_rdf_normalise) */
    int32_t* status;            /* [1], bits are ORed in (_rdf_counts) */
    double r_max;               /* finite, > 0 */
    int n_structs;              /* B >= 0 */
    int n_atoms;                /* atom_ptr[B] >= 0 */
    int max_atoms;              /* the largest n_b (sizes the launch), 1 .. n_atoms */
    int n_species;              /* S, 1 .. ALIGNN_TRAJ_MAX_SPECIES */
    int n_bins;                 /* 1 .. ALIGNN_TRAJ_MAX_BINS */
    int n_total_frames;         /* >= 0 */
    int frame0;                 /* >= 0 */
    int frame_step;             /* >= 1 */
    int n_frames;               /* frames used, >= 0 */
    int lattice_per_frame;      /* 0 / 1 */
} alignn_traj_rdf_args;
int alignn_traj_rdf_counts(const alignn_traj_rdf_args* args, void* stream);
int alignn_traj_rdf_normalise(const alignn_traj_rdf_args* args, void* stream);
size_t alignn_traj_rdf_args_size(void); /* a binding checks its own packing against this */

/* ------------------------------------------------------------------------------------------
 * _traj_com / _traj_corr: the time correlations.  Frames t below count the frames USED.  For lag k = 0 .. max_lag (<= n_frames -
 * 1) the origins are t = 0, origin_stride, 2 origin_stride, ... with t + k <= n_frames - 1, n_origins(k) of them.
 *
 * mode 0, mean squared displacement, out [B][S + 1][max_lag + 1][3], per Cartesian component x:
 *     out = sum_t sum_{i in a} ((r_i(t + k) - r_i(t)) - (c(t + k) - c(t)))_x^2 / (n_origins(k) N_a)
 * c the structure's centre of mass, com [n_frames][B][3] = (sum_i m_i r_i) / (sum_i m_i), each sum in row order by one thread
 * (_traj_com writes it); com = NULL: c = 0.
 * mode 1, velocity autocorrelation of the momenta `traj`, v = p / m, out [B][S + 1][max_lag + 1]:
 *     out = sum_t sum_{i in a} ((vx vx' + vy vy') + vz vz') / (n_origins(k) N_a),  v = v_i(t), v' = v_i(t + k)
 * One workgroup of 256 threads per (lag, structure): a thread sums its row over the origins in order, the rows of a group are
 * then summed in a fixed order (chunks of 256 rows in order; in a chunk a lane's four rows in order, then the xor butterfly).
 * ------------------------------------------------------------------------------------------ */
typedef struct alignn_traj_corr_args {
    const double* traj;         /* [n_total_frames][n_atoms][3]: positions (mode 0) or momenta (mode 1) */
    const double* masses;       /* [n_atoms], > 0 (_traj_com and mode 1) */
    const int32_t* atom_ptr;    /* [B + 1] */
    const int32_t* group;       /* [n_atoms]   (_traj_corr) */
    const int32_t* group_count; /* [B][S + 1]   (_traj_corr) */
    double* com;                /* [n_frames][B][3], or NULL (mode 0: no centre of mass is removed); _traj_com writes every element, _traj_corr reads */
    double* out;                /* [B][S + 1][max_lag + 1][3] (mode 0) or [B][S + 1][max_lag + 1] (mode 1) */
    int n_structs;              /* B >= 0 */
    int n_atoms;                /* atom_ptr[B] */
    int n_species;              /* S, 1 .. ALIGNN_TRAJ_MAX_SPECIES */
    int n_total_frames;
    int frame0;
    int frame_step;             /* >= 1 */
    int n_frames;               /* frames used, >= 0 */
    int max_lag;                /* 0 .. n_frames - 1 */
    int origin_stride;          /* >= 1 */
    int mode;                   /* 0 mean squared displacement, 1 velocity autocorrelation */
} alignn_traj_corr_args;
int alignn_traj_com(const alignn_traj_corr_args* args, void* stream);
int alignn_traj_corr(const alignn_traj_corr_args* args, void* stream);
size_t alignn_traj_corr_args_size(void);

/* ------------------------------------------------------------------------------------------
 * _traj_vdos: the vibrational density of states of a normalised velocity autocorrelation.  vacf [n_rows][max_lag + 1] (a row per
 * structure and group), out [n_rows][n_freq] in fs; one thread per (row, frequency) sums over k in ascending order:
 *     out[j] = (2 dtau) sum_k (c_k w_k) (C(k) / C(0)) cos((2 pi (nu_j 1e-3)) (k dtau)),   nu_j = j (f_max_thz / (n_freq - 1))
 * c_0 = 1/2, else 1; window 1 (Hann): w_k = (1 + cos(pi k / K)) / 2 (K = max_lag; 1 when K = 0); window 0: w_k = 1.  dtau in fs,
 * nu in THz.  A row with C(0) = 0 gives zeros.  n_freq >= 2, f_max_thz > 0, dtau > 0: anything else is refused with
 * hipErrorInvalidValue before a launch, and out is left as it was.
 * ------------------------------------------------------------------------------------------ */
int alignn_traj_vdos(const double* vacf, int n_rows, int max_lag, double dtau, int n_freq, double f_max_thz, int window,
                     double* out, void* stream);

/* ------------------------------------------------------------------------------------------
 * _traj_fit: Einstein's relation.  The least-squares line through msd(k) against tau_k = k dtau over k_lo <= k <= k_hi (0 <= k_lo
 * < k_hi <= max_lag), msd [n_rows][max_lag + 1][3]; out [n_rows][4][4]: the components x, y, z and their total (mx + my) + mz,
 * each (slope, intercept, standard error of the slope, D = slope / 2 - the total: slope / 6).  One wavefront per (row, component):
 * the means first, then Sxx = sum (x - xm)^2 and Sxy = sum (x - xm)(y - ym), slope = Sxy / Sxx, intercept = ym - slope xm, standard
 * error sqrt((sum (y - (intercept + slope x))^2 / (n - 2)) / Sxx) (0 with two points); every sum lane-strided, then the xor butterfly.
 * ------------------------------------------------------------------------------------------ */
int alignn_traj_fit(const double* msd, int n_rows, int max_lag, double dtau, int k_lo, int k_hi, double* out, void* stream);

/* ------------------------------------------------------------------------------------------
 * _traj_green_kubo: the running integral of the velocity autocorrelation, vacf and out [n_rows][max_lag + 1]; one thread per row:
 *     I(0) = 0,  I(k) = I(k - 1) + (C(k - 1) + C(k)) / 2;   out[k] = ((I(k) (dtau time_unit)) time_unit) / 3
 * dtau in fs, time_unit the femtosecond in the time unit of the velocities (ASE's: dynamics.FS), so that out is in A^2 / fs.
 * ------------------------------------------------------------------------------------------ */
int alignn_traj_green_kubo(const double* vacf, int n_rows, int max_lag, double dtau, double time_unit, double* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* ALIGNN_TRAJ_H */
