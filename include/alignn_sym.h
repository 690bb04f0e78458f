/* alignn_sym.h - the entry points of libalignn_hip.so for crystal symmetry (csrc/symmetry.hip; alignn_amd/symmetry.py is the
 * driver and binds this header, tests/sym_ref.py the numpy restatement): the space-group operations of B crystals found
 * together, the atom permutations and orbits that follow from them, and the projection of forces, stresses and positions onto
 * the symmetric subspace.
 *
 * A header of its own beside alignn_hip.h, in the same regular form (one extern "C" block, argument structs, prototypes over the
 * base types): alignn_amd/_abi.py reads it.  Every pointer is a device pointer; `stream` is a hipStream_t.  Every entry point
 * returns 0 or the HIP error; hipErrorInvalidValue (1) for an argument out of its range, before any launch.  No structures is a
 * no-op that returns 0.
 *
 * float64 without contraction, no atomics on floating-point values, every floating-point sum in a fixed order over the
 * structure's own atoms and operations: a structure's bits do not depend on the launch it is in, nor on its place in it.
 *
 * Conventions.  The cell's rows are the lattice vectors a_0, a_1, a_2 (A row-major); the B structures are packed (structure b
 * owns the rows [atom_ptr[b], atom_ptr[b + 1]) of every per-atom array).  Fractional coordinates are the row x = r Ainv, Ainv
 * the inverse by cofactors (csrc/cell3.h), not wrapped.  An operation {W | t} has an integer W with det +-1 and t in [0, 1) and
 * acts on fractional column coordinates as x' = W x + t; W x is (W_r0 x_0 + W_r1 x_1) + W_r2 x_2 per row r.
 *
 * Lattice operations.  With L = max_i |a_i| and h_k = |det A| / |a_{k+1} x a_{k+2}| the cell's heights, the candidates for the
 * image of a_i are the lattice vectors v = (n_0 a_0 + n_1 a_1) + n_2 a_2 over |n_k| <= floor((L + symprec) / h_k) with
 * | |v| - |a_i| | <= symprec.  A range above ALIGNN_SYM_MAX_IMAGE_RANGE on an axis sets ALIGNN_SYM_STATUS_IMAGES for the structure
 * and it has no operations; more than ALIGNN_SYM_MAX_CANDIDATES candidates for an axis, or more than ALIGNN_SYM_MAX_LATTICE_OPS
 * accepted W, set ALIGNN_SYM_STATUS_OVERFLOW likewise (symprec is then not small against the cell).  Column i of W holds the n
 * of the image of a_i; W is a lattice operation when |det W| = 1 and | |a'_i - a'_j| - |a_i - a_j| | <= symprec for the three
 * pairs i < j.  No angle tolerance, no cell reduction: entries of W may exceed +-1.  The W are sorted by their nine entries
 * row-major, ascending.
 *
 * Space-group operations.  The pivot species is the one with the fewest atoms (the lowest species number among equals), the
 * pivot atom p its lowest index.  For every lattice operation W and every atom j of the pivot species, in ascending j:
 * d = x_j - W x_p, t = d - floor(d), a component that rounds to 1.0 becomes 0.  {W | t} is accepted when every atom i has an atom
 * k of its own species with |(f_0 a_0 + f_1 a_1) + f_2 a_2| <= symprec, f = delta - rint(delta), delta = (W x_i + t) - x_k.  The
 * nearest such k is map[i] (the lowest k among equals) and shift[i] = rint(delta) for that k.  The operations of a structure are
 * ordered by W, then by j; all are reported, centring and supercell translations included.
 */
#ifndef ALIGNN_SYM_H
#define ALIGNN_SYM_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ALIGNN_SYM_MAX_ATOMS 1024      /* atoms per structure: fractional coordinates and species ranges in LDS (36 KiB) */
#define ALIGNN_SYM_MAX_IMAGE_RANGE 8   /* |n_k| of a candidate lattice vector, per axis */
#define ALIGNN_SYM_MAX_CANDIDATES 256  /* candidate images of one lattice vector */
#define ALIGNN_SYM_MAX_LATTICE_OPS 48  /* lattice operations of a structure (the order of the largest holohedry) */
#define ALIGNN_SYM_INFO 8              /* int32 words of info per structure, below */
#define ALIGNN_SYM_STATUS_IMAGES 1     /* bit of the status word: the cell needs images beyond the range (or is singular) */
#define ALIGNN_SYM_STATUS_OVERFLOW 2   /* bit: more candidates or lattice operations than the limits above */
#define ALIGNN_SYM_STATUS_INPUT 4      /* bit: order / segment / pivot do not describe the structure's rows */

/* info [B][ALIGNN_SYM_INFO], the one array a driver reads back between _sym_search and _sym_fill:
 *   0 n_ops   1 n_translations (operations with W = I)   2 point_group_order (distinct W)   3 crystal system, 0 triclinic,
 *   1 monoclinic, 2 orthorhombic, 3 tetragonal, 4 trigonal, 5 hexagonal, 6 cubic   4 status bits   5 lattice operations   6, 7 zero.
 * The system is decided from the distinct proper parts det(W) W of the distinct W, their order from the trace (3: 1, -1: 2, 0: 3,
 * 1: 4, 2: 6), the rules in this order: any of order 6 hexagonal; eight of order 3 cubic; two of order 3 trigonal; any of order 4
 * tetragonal; three of order 2 orthorhombic; one of order 2 monoclinic; otherwise triclinic.
 *
 * The caller sorts each structure's atoms by species (stable): order[q] is the local index of the atom in sorted slot q,
 * seg_lo[q] / seg_hi[q] the sorted slots [lo, hi) of the atoms of its species, pivot_lo[b] / pivot_hi[b] the slots of the pivot
 * species.  Values that do not fit the structure set ALIGNN_SYM_STATUS_INPUT and it has no operations.
 *
 * _sym_search (three launches): one workgroup per structure writes frac and the sorted lattice operations; one workgroup of 256
 * threads per (lattice operation, structure, 16 candidates j) holds the structure's sorted fractional coordinates and species
 * ranges in LDS and gives each wavefront a candidate translation: the lanes run over the atoms i against the atoms of i's species
 * and the wavefront leaves at the first 64 atoms with one left without a partner; accepted[48 atom_ptr[b] + w n_b + (slot of j)]
 * = 1 and op_count[b][w] counts them (integer adds); one thread per structure then fills info.
 * _sym_fill (two launches), with op_ptr the prefix sums of info's n_ops: the same grid, one wavefront per accepted operation
 * writes its rotation, translation, atom_map and shifts, a lane per atom scanning the atoms of its species for the nearest; one
 * thread per atom then takes orbits[i] = min_g atom_map[g][i] (local indices).
 * Per-operation outputs are packed: operation g of structure b is entry op_ptr[b] + g of rotations and translations, and its
 * atom_map / shifts rows start at map_ptr[b] + g n_b, map_ptr[b] = sum_{b' < b} n_ops[b'] n_b'.  atom_map holds local indices. */
typedef struct alignn_sym_find_args {
    const double* lattice;    /* [B][3][3] */
    const double* pos;        /* [N][3] Cartesian */
    const int32_t* atom_ptr;  /* [B + 1], 0 first */
    const int32_t* order;     /* [N] */
    const int32_t* seg_lo;    /* [N] */
    const int32_t* seg_hi;    /* [N] */
    const int32_t* pivot_lo;  /* [B] */
    const int32_t* pivot_hi;  /* [B] */
    double* frac;             /* [N][3]             (these four: scratch of the pair, the caller need not zero them.  _sym_search */
    int32_t* lattice_ops;     /* [B][48][9]          writes what _sym_fill reads and nothing else: the frac rows of a structure */
    uint8_t* accepted;        /* [48 N]              without a status bit, its first info[5] lattice operations, the flag of every */
    int32_t* op_count;        /* [B][48]             candidate of those, and every count, zeroed first) */
    int32_t* info;            /* [B][8]             (_sym_search writes every word, _sym_fill reads the status and the counts) */
    const int64_t* op_ptr;    /* [B + 1]            (_sym_fill) */
    const int64_t* map_ptr;   /* [B + 1]            (_sym_fill) */
    int32_t* rotations;       /* [G][3][3]          (_sym_fill writes every element of these five), G = op_ptr[B] */
    double* translations;     /* [G][3]             (_sym_fill) */
    int32_t* atom_map;        /* [map_ptr[B]]       (_sym_fill) */
    int32_t* shifts;          /* [map_ptr[B]][3]    (_sym_fill) */
    int32_t* orbits;          /* [N]                (_sym_fill) */
    double symprec;           /* finite, > 0 */
    int64_t n_ops_total;      /* G >= 0             (_sym_fill) */
    int64_t n_map_total;      /* map_ptr[B] >= 0    (_sym_fill) */
    int n_structs;            /* B, 0 .. 65535 */
    int n_atoms;              /* N = atom_ptr[B] */
    int max_atoms;            /* the largest n_b (sizes the LDS), 1 .. min(N, ALIGNN_SYM_MAX_ATOMS) */
} alignn_sym_find_args;
int alignn_sym_search(const alignn_sym_find_args* args, void* stream);
int alignn_sym_fill(const alignn_sym_find_args* args, void* stream);
size_t alignn_sym_find_args_size(void); /* a binding checks its own packing against this */

/* ------------------------------------------------------------------------------------------
 * The symmetrisers, one launch each for the whole batch, over the operations g of a structure in their stored order.  With
 * Q_g = A^T W_g A^-T the Cartesian rotation, computed as M = A^T W (M_ac = (A_0a W_0c + A_1a W_1c) + A_2a W_2c), then
 * Q_ad = (M_a0 Ainv_d0 + M_a1 Ainv_d1) + M_a2 Ainv_d2:
 *   _sym_forces     out_i = (sum_g Q_g^T F_map[g][i]) / G, a term's element d (Q_0d F_0 + Q_1d F_1) + Q_2d F_2; one thread per atom;
 *   _sym_stress     out = (sum_g Q_g^T s Q_g) / G, a term's element (a, c) (Q_0a u_0 + Q_1a u_1) + Q_2a u_2 with
 *                   u_p = (s_p0 Q_0c + s_p1 Q_1c) + s_p2 Q_2c; one thread per element, in [B][3][3];
 *   _sym_positions  in fractional coordinates x'_i = (sum_g Winv_g ((x_map[g][i] + shift[g][i]) - t_g)) / G, Winv the integer
 *                   adjugate times det; out_i = x'_i A, Cartesian; one thread per atom.
 * A structure without operations (G = 0) gets its input back.
 * ------------------------------------------------------------------------------------------ */
typedef struct alignn_sym_apply_args {
    const double* lattice;      /* [B][3][3] */
    const double* in;           /* [N][3] forces or Cartesian positions; [B][3][3] stresses */
    double* out;                /* as in: every element is written */
    const int32_t* atom_ptr;    /* [B + 1]         (_sym_forces, _sym_positions) */
    const int64_t* op_ptr;      /* [B + 1] */
    const int64_t* map_ptr;     /* [B + 1] */
    const int32_t* rotations;   /* [G][3][3] */
    const double* translations; /* [G][3]          (_sym_positions) */
    const int32_t* atom_map;    /* [map_ptr[B]]    (_sym_forces, _sym_positions) */
    const int32_t* shifts;      /* [map_ptr[B]][3] (_sym_positions) */
    int64_t n_ops_total;        /* G >= 0 */
    int64_t n_map_total;        /* map_ptr[B] >= 0 */
    int n_structs;              /* B, 0 .. 65535 */
    int n_atoms;                /* N = atom_ptr[B] >= 0 */
} alignn_sym_apply_args;
int alignn_sym_forces(const alignn_sym_apply_args* args, void* stream);
int alignn_sym_stress(const alignn_sym_apply_args* args, void* stream);
int alignn_sym_positions(const alignn_sym_apply_args* args, void* stream);
size_t alignn_sym_apply_args_size(void);

#ifdef __cplusplus
}
#endif
#endif /* ALIGNN_SYM_H */
