/* alignn_neb.h - the entry points of libalignn_hip.so for the nudged elastic band (csrc/neb.hip; alignn_amd/neb.py is the driver
 * and binds this header, tests/neb_ref.py the numpy restatement).
 *
 * A header of its own beside alignn_hip.h, in the same regular form (one extern "C" block, one argument struct, prototypes over
 * the base types): alignn_amd/_abi.py reads it.  Every pointer is a device pointer; `stream` is a hipStream_t.  Every entry point
 * returns 0 or the HIP error; hipErrorInvalidValue (1) for an argument out of its range.
 *
 * The formulas are those of ASE 3.22's ase/neb.py for method="aseneb" and "improvedtangent".  float64 without contraction, no
 * atomics on floating-point values, every sum in a fixed order that depends on the image's own rows only: a band's bits do not
 * depend on the launch it is in, nor on its place in it.
 *
 * A band b of M_b images (endpoints included, 3 .. ALIGNN_NEB_MAX_IMAGES) of n_b >= 1 atoms in the cell C_b (rows a, b, c).  The
 * minimum image convention, for a row difference d, is the plain wrap
 *     f = (d0 Cinv[0] + d1 Cinv[1]) + d2 Cinv[2];  f -= rint(f);  mic(d) = (f0 C[0] + f1 C[1]) + f2 C[2]
 * with Cinv the inverse of C by cofactors (csrc/cell3.h) - not ASE's Minkowski-reduced find_mic: in a strongly skewed cell the
 * two can differ.
 *
 * Not here: the image dependent pair potential that a band can be started on (IDPP) has a header of its own, alignn_idpp.h; its
 * results are laid out as _neb_forces reads an evaluation.
 */
#ifndef ALIGNN_NEB_H
#define ALIGNN_NEB_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ALIGNN_NEB_MAX_IMAGES 64 /* images per band, the two endpoints included */

/* ------------------------------------------------------------------------------------------
 * _neb_interpolate: NEB.interpolate(mic=True).  One thread per output row, grid-strided.
 *
 *   initial, final [sum n_b][3] the endpoints of all bands, packed: band b owns rows [end_ptr[b], end_ptr[b + 1])
 *   end_ptr        [n_bands + 1] int32, 0 first; n_b = end_ptr[b + 1] - end_ptr[b]
 *   lattice        [n_bands][3][3] row-major
 *   row_ptr        [n_bands + 1] int32, 0 first: band b owns output rows [row_ptr[b], row_ptr[b + 1]), (M_b - 2) n_b of them, so
 *                  M_b = 2 + (row_ptr[b + 1] - row_ptr[b]) / n_b; its interior images follow one another, image 1 first
 *   n_bands        >= 0
 *   n_rows         row_ptr[n_bands], >= 0
 *   positions      [n_rows][3] out: image j (1 .. M_b - 2), atom r: initial + j * step, step = mic(final - initial) / (M_b - 1),
 *                  in exactly these operations
 *   inv_lattice    [n_bands][3][3] out, or NULL: the inverse cells by cofactors, as _neb_forces takes them
 * ------------------------------------------------------------------------------------------ */
int alignn_neb_interpolate(const double* initial, const double* final, const int32_t* end_ptr, const double* lattice,
                           const int32_t* row_ptr, int n_bands, int64_t n_rows, double* positions, double* inv_lattice,
                           void* stream);

/* ------------------------------------------------------------------------------------------
 * _neb_forces: NEB.get_forces for the ACTIVE bands of a batch.  One workgroup of 256 threads per (active band k, interior image
 * i = 1 .. M - 2), its threads strided over the image's n rows; band s = active[k].
 *
 * With E the band's M energies (endpoints included), imax the interior image of largest energy (the lowest index on ties),
 * t1 = mic(R_i - R_{i-1}), t2 = mic(R_{i+1} - R_i), f the raw force with its fixed rows set to zero first (ASE applies FixAtoms
 * inside get_forces, ahead of the projection) and k the band's spring constant:
 *   method 0, aseneb:  tau = t2 if i < imax, t1 if i > imax, t1 + t2 at imax (not normalised); ft = f.tau, tt = tau.tau;
 *       climbing image (climb and i = imax):  F = f - 2 ft/tt tau
 *       otherwise:                            F = f - ft/tt tau - ((k t1 - k t2).tau)/tt tau
 *   method 1, improvedtangent:  tau = t2 if E[i+1] > E[i] > E[i-1];  t1 if E[i+1] < E[i] < E[i-1];  otherwise, with dmax / dmin the
 *       larger / smaller of |E[i+1] - E[i]|, |E[i-1] - E[i]|:  t2 dmax + t1 dmin if E[i+1] > E[i-1], else t2 dmin + t1 dmax;
 *       then tau /= |tau|;
 *       climbing image:  F = f - 2 (f.tau) tau
 *       otherwise:       F = f - (f.tau) tau + (k |t2| - k |t1|) tau
 * All of it from five sums over the image's 3n components (|t1|^2, |t2|^2, t1.t2, f.t1, f.t2) with tau = a t1 + b t2: one
 * fixed-order workgroup reduction, then a second pass over the rows that writes F.  A band whose endpoints coincide has tt = 0
 * and gets what the arithmetic gives.
 *
 * A band whose row counts do not fit (rows that are no (M - 2) n, M above max_images, force rows of another count) is left
 * untouched but for imax[k] = -1.
 * ------------------------------------------------------------------------------------------ */
typedef struct alignn_neb_args {
    /* the evaluation of the active bands' interior images, in evaluation order: band by band, image 1 first */
    const double* forces;      /* [force_ptr[n_active]][3] raw forces: rows [force_ptr[k], force_ptr[k+1]) are active[k]'s,
                                  (M - 2) n of them */
    const double* energy;      /* [energy_ptr[n_active]] energies: entries [energy_ptr[k], energy_ptr[k+1]) are active[k]'s,
                                  M - 2 of them */
    const int32_t* force_ptr;  /* [n_active + 1] */
    const int32_t* energy_ptr; /* [n_active + 1] */
    const int32_t* active;     /* [n_active] band indices */
    /* the bands (B of them) */
    const int32_t* row_ptr;    /* [B + 1] band b owns rows [row_ptr[b], row_ptr[b+1]) of `positions` / `fixed` (relax's atom_ptr) */
    const int32_t* image_ptr;  /* [B + 1] band b owns entries [image_ptr[b], image_ptr[b+1]) of energies_out: M_b of them */
    const int32_t* end_ptr;    /* [B + 1] band b owns rows [end_ptr[b], end_ptr[b+1]) of `initial` / `final`: n_b of them */
    const double* lattice;     /* [B][3][3] row-major */
    const double* inv_lattice; /* [B][3][3] the inverse cells (by cofactors: _neb_interpolate writes them) */
    const double* spring;      /* [B] the spring constants k_b */
    const double* initial;     /* [sum n_b][3] image 0 of every band */
    const double* final;       /* [sum n_b][3] image M_b - 1 */
    const double* end_energy;  /* [B][2] the energies of image 0 and of image M_b - 1 */
    const double* positions;   /* [N][3] the bands' interior rows: relax's position array */
    const uint8_t* fixed;      /* [N] non-zero: the row's raw force is zero (FixAtoms), or NULL */
    /* outputs */
    double* forces_out;        /* [force_ptr[n_active]][3] the projected forces, laid out as `forces` (alignn_fire_step takes them as its
                                  forces): the rows of the active bands that fit are written */
    double* energies_out;      /* [sum M_b] every image's energy by global image index (written for the active bands) */
    int32_t* imax;             /* [n_active] */
    double* emax;              /* [n_active] E[imax] (not written for a band that does not fit) */
    /* scalars */
    int n_active;              /* >= 0 */
    int max_images;            /* the largest M_b of the active bands: 3 .. ALIGNN_NEB_MAX_IMAGES (sizes the launch) */
    int method;                /* 0 aseneb, 1 improvedtangent */
    int climb;                 /* 0 / 1 */
} alignn_neb_args;
int alignn_neb_forces(const alignn_neb_args* args, void* stream);
size_t alignn_neb_args_size(void); /* a binding checks its own packing against this */

#ifdef __cplusplus
}
#endif
#endif /* ALIGNN_NEB_H */
