/* alignn_idpp.h - the entry point of libalignn_hip.so for the image dependent pair potential (IDPP) that starts a nudged elastic
 * band (csrc/idpp.hip; alignn_amd/idpp.py is the driver and binds this header, tests/idpp_ref.py the numpy restatement).
 *
 * A header of its own beside alignn_neb.h, in the same regular form (one extern "C" block, one argument struct, prototypes over
 * the base types): alignn_amd/_abi.py reads it.  Every pointer is a device pointer; `stream` is a hipStream_t.  The entry point
 * returns 0 or the HIP error; hipErrorInvalidValue (1) for an argument out of its range.
 *
 * The objective is that of ASE 3.22's ase/neb.py (class IDPP, NEB.idpp_interpolate) with the minimum image convention of
 * alignn_neb.h (the plain wrap `mic`, not ASE's Minkowski-reduced find_mic).  For a band of M images (endpoints 0 and M - 1) of n
 * atoms, image m, atom a and every b != a:
 *     D_ab = mic(R_a - R_b)        d_ab = |D_ab| = sqrt((D0 D0 + D1 D1) + D2 D2)
 *     t_ab(m) = d1_ab + m ((d2_ab - d1_ab) / (M - 1))      d1, d2: the same d_ab taken in image 0 and in image M - 1
 *     delta = d_ab - t_ab(m)
 *     E_m = 1/2 sum_a sum_{b != a} delta^2 / d_ab^4
 *     F_a = -2 sum_{b != a} delta (1 - 2 delta / d_ab) / d_ab^5 D_ab
 * Every pair is counted from both sides, as ASE does; d1 and d2 are recomputed per pair from the endpoint rows (no [n][n] tables).
 * Coinciding atoms (d = 0) get what the arithmetic gives; a pair at exactly half a cell vector takes the image rint gives (half
 * to even): the cusp of the wrap, as in ASE.
 *
 * float64 without contraction, no atomics on floating-point values, every sum in a fixed order that depends on the image's own
 * rows only: a band's bits do not depend on the launch it is in, nor on its place in it.
 */
#ifndef ALIGNN_IDPP_H
#define ALIGNN_IDPP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------------------------
 * _idpp_forces: the IDPP energies and forces of the interior images of the ACTIVE bands of a batch; band s = active[k], its
 * M = 2 + (row_ptr[s + 1] - row_ptr[s]) / n images (endpoints included) of n = end_ptr[s + 1] - end_ptr[s] atoms.
 *
 * Two launches.  The first: one wavefront per (active band k, interior image m = 1 .. M - 2, atom a), its 64 lanes strided over
 * b (lane l takes b = l, l + 64, ... in this order, the pair b = a skipped), then a butterfly sum over the lanes: F_a and the
 * row's share e_a = 1/2 sum_b delta^2 / d^4 of E_m.  The second: one workgroup of 256 threads per (k, m) sums e_a over the image's
 * rows in a fixed order (threads strided over a, lanes, then waves).
 *
 * `forces` and `energy` are laid out as alignn_neb_forces reads its `forces` and `energy`: one follows the other with no copy.
 *
 * A band whose row counts do not fit (rows that are no multiple of n, M outside 3 .. max_images, n above max_atoms, force rows or
 * energies of another count) is left untouched but for status[k] = -1; every other active band gets status[k] = 0.
 * ------------------------------------------------------------------------------------------ */
typedef struct alignn_idpp_args {
    /* the active bands, in evaluation order: band by band, image 1 first */
    const int32_t* force_ptr;  /* [n_active + 1] rows [force_ptr[k], force_ptr[k+1]) of `forces` / `row_energy` are active[k]'s */
    const int32_t* energy_ptr; /* [n_active + 1] entries [energy_ptr[k], energy_ptr[k+1]) of `energy` are active[k]'s, M - 2 of them */
    const int32_t* active;     /* [n_active] band indices */
    /* the bands (B of them) */
    const int32_t* row_ptr;    /* [B + 1] band b owns rows [row_ptr[b], row_ptr[b+1]) of `positions`: (M_b - 2) n_b of them */
    const int32_t* end_ptr;    /* [B + 1] band b owns rows [end_ptr[b], end_ptr[b+1]) of `initial` / `final`: n_b of them */
    const double* lattice;     /* [B][3][3] row-major */
    const double* inv_lattice; /* [B][3][3] the inverse cells (by cofactors: alignn_neb_interpolate writes them) */
    const double* initial;     /* [sum n_b][3] image 0 of every band */
    const double* final;       /* [sum n_b][3] image M_b - 1 */
    const double* positions;   /* [N][3] the bands' interior rows, a band's images one after the other, image 1 first */
    /* outputs */
    double* forces;            /* [force_ptr[n_active]][3] F_a of every interior row of the active bands */
    double* energy;            /* [energy_ptr[n_active]] E_m of every interior image of the active bands */
    double* row_energy;        /* [force_ptr[n_active]] scratch, one entry per row of `forces`: e_a (the second launch reads it) */
    int32_t* status;           /* [n_active] 0, or -1 for a band whose row counts do not fit */
    /* scalars */
    int n_active;              /* 0 .. 65535 */
    int max_images;            /* the largest M_b of the active bands: 3 .. ALIGNN_NEB_MAX_IMAGES of alignn_neb.h (sizes the launch) */
    int max_atoms;             /* the largest n_b of the active bands, >= 1 (sizes the launch) */
} alignn_idpp_args;
int alignn_idpp_forces(const alignn_idpp_args* args, void* stream);
size_t alignn_idpp_args_size(void); /* a binding checks its own packing against this */

#ifdef __cplusplus
}
#endif
#endif /* ALIGNN_IDPP_H */
