/* alignn_phsym.h - the entry points of libalignn_hip.so for phonons from symmetry-reduced displacements (csrc/phonon_sym.hip;
 * alignn_amd/phonons.py is the driver and binds this header, tests/phonons_sym_ref.py the numpy restatement): instead of every
 * atom of the primitive cell along x, y and z, only the symmetry-inequivalent atoms are displaced, each along as few directions
 * as its site group allows, and the force constants of all atoms are solved for and distributed on the device.
 *
 * A header of its own beside alignn_hip.h, in the same regular form (one extern "C" block, argument structs, prototypes over the
 * base types): alignn_amd/_abi.py reads it.  Every pointer is a device pointer; `stream` is a hipStream_t.  Every entry point
 * returns 0 or the HIP error; hipErrorInvalidValue (1) for an argument out of its range, before any launch.  Nothing to do (no
 * structures, jobs, pairs or items) is a no-op that returns 0.
 *
 * float64 without contraction, no atomics on floating-point values, every floating-point sum in a fixed order over the
 * structure's own atoms and operations: a structure's bits do not depend on the launch it is in, nor on its place in it.
 *
 * Conventions.  Those of alignn_hip.h (phonons) and alignn_sym.h hold: the B structures are packed (structure b owns the rows
 * [atom_ptr[b], atom_ptr[b + 1]) of every per-atom array, the operations [op_ptr[b], op_ptr[b + 1]), the atom_map / shifts rows
 * from map_ptr[b]); atom indices are local to the structure.  The supercell N = (N0, N1, N2) of a structure has the images
 * m = (m0, m1, m2), image index (m0 N1 + m1) N2 + m2; supercell atom (m, j), basis atom j of image m, has the row
 * (image index) n + j of a displaced supercell.  The force constants are C[image][3i + a][3j + b] at fc_off[b]; Phi(i; m, j) is
 * the 3 x 3 block C[m][3i + .][3j + .].
 *
 * 1. Usable operations.  Operation g = {W | t} is usable with N iff (W[r][c] N[c]) % N[r] == 0 for all r, c.  It then maps
 *    supercell atoms by integers alone: g sends (m, j) to ((W m + shift[g][j]) mod N, map[g][j]), the mod taken into [0, N)
 *    (shifts may be negative and beyond N).  Its Cartesian rotation is Q_g = A^T W A^-T with the arithmetic of alignn_sym.h's
 *    symmetrisers (csrc/cell3.h cartesian_rotation); for W = I, Q = I exactly.
 * 2. Representatives.  The classes of the n atoms under the usable operations alone (j and map[g][j] are in one class for every
 *    usable g; not alignn_sym's orbits, which take every operation); the representative of a class is its lowest atom.
 * 3. Site group.  S_i of representative i: the usable g with map[g][i] == i, in operation order, each followed by the lattice
 *    translation -shift[g][i] so that it fixes supercell atom (0, i): g~ (m, j) = ((W m + shift[g][j] - shift[g][i]) mod N,
 *    map[g][j]).  |S_i| <= ALIGNN_PHSYM_MAX_SITE_OPS.
 * 4. Directions.  The 13 candidates, in this order, each divided by its length sqrt((c0 c0 + c1 c1) + c2 c2) (the components are
 *    +-1, +-0.7071067811865475 and +-0.5773502691896258):
 *        x, y, z; (1,1,0), (1,0,1), (0,1,1), (1,-1,0), (1,0,-1), (0,1,-1); (1,1,1), (1,1,-1), (1,-1,1), (-1,1,1).
 *    For k = 1, then 2: the first k-subset, in lexicographic order of the candidate indices, whose images span space; at k = 3
 *    {x, y, z} without a test.  "Span": M = sum over g in S_i (ascending), then d in the subset (ascending), of u u^T with
 *    u = Q_g^T d, u_a = (Q_0a d_0 + Q_1a d_1) + Q_2a d_2, every element M_ab = M_ab + u_a u_b; det M along the first row from
 *    the cofactors, (M_00 c_00 - M_01 c_01) + M_02 c_02; t = ((M_00 + M_11) + M_22) / 3; the subset spans iff
 *    det M >= ALIGNN_PHSYM_TAU ((t t) t).
 *    tau = 1e-4.  Over every subset tried for every crystal of tests/sym_ref.crystals() at the supercells (2,2,2), (3,3,3) and
 *    (2,3,4), the ratio det M / t^3 of the rank-deficient subsets is at most 1.9e-16 in magnitude and that of the spanning ones
 *    at least 0.729 (tests/test_phonons_sym_ref.py lists them and checks the gap): tau has a factor 1e3 to the spanning side and
 *    1e12 to the other - and still 1e2 above (symprec / cell edge)^2 ~ 1e-6 for a structure symmetric only to a loose symprec.
 * 5. Solve.  G_m [n_sc][3] is the drift-corrected central difference (F- - F+) / (2 delta) of the pair of supercells of
 *    direction d_m of representative i (the arithmetic and the three drift modes of alignn_phonon_fc_rows).  For every
 *    supercell atom B: Phi(i; B) = Minv T, T = sum over g in S_i (ascending), then m (ascending), of u_gm (G_m[g~ B] Q_g), the
 *    row (G Q)_b = (G_0 Q_0b + G_1 Q_1b) + G_2 Q_2b, T_ab = T_ab + u_a (G Q)_b, Minv the inverse of M by cofactors
 *    (csrc/cell3.h inv3_cof) and Phi_ab = (Minv_a0 T_0b + Minv_a1 T_1b) + Minv_a2 T_2b.
 * 6. Distribute.  A non-representative i' with representative i takes the lowest usable g with map[g][i] == i' (followed by
 *    -shift[g][i] as in 3): Phi(i'; g~ B) = Q_g Phi(i; B) Q_g^T for every B, as P = Phi Q^T, P_ab = (Phi_a0 Q_b0 + Phi_a1 Q_b1)
 *    + Phi_a2 Q_b2, then (Q_a0 P_0b + Q_a1 P_1b) + Q_a2 P_2b.  B -> g~ B is a permutation of the supercell atoms: no two threads
 *    write the same block.
 * 7. A structure whose only operation is the identity gets k = 3, {x, y, z}, Q = I, M = Minv = I: its displaced supercells and
 *    force constants are those of alignn_phonon_displace / alignn_phonon_fc_rows, bit for bit.
 */
#ifndef ALIGNN_PHSYM_H
#define ALIGNN_PHSYM_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ALIGNN_PHSYM_MAX_ATOMS 32      /* atoms of a primitive cell (the 3n <= 96 of the eigen launch) */
#define ALIGNN_PHSYM_MAX_SITE_OPS 48   /* operations of a site group (the order of the largest point group) */
#define ALIGNN_PHSYM_N_CANDIDATES 13   /* candidate directions */
#define ALIGNN_PHSYM_TAU 1e-4          /* the spanning threshold of rule 4 */

/* _phsym_plan, one launch, one workgroup per structure, straight from the packed arrays of the symmetry search: usable [G]
 * (0 / 1) and rot [G][3][3] (Q_g) per operation; per atom rep (its representative), n_site and site_ops [48] (the site group of
 * a representative, operation indices local to the structure), n_dir, dirs [3][3] (the chosen directions as rows, the unused
 * rows zero), minv [3][3], dist_op (the distributing operation of a non-representative, -1 for a representative).
 * n_dir is the one array a driver reads back: the directions of a representative (1 .. 3), 0 for a non-representative, -1 for
 * every atom of a structure that cannot be planned (more than ALIGNN_PHSYM_MAX_ATOMS atoms, no operations, an atom_map entry
 * outside the structure, a site group without the identity's place or beyond ALIGNN_PHSYM_MAX_SITE_OPS, offsets that do not fit
 * the arrays).  Every element of the nine outputs is written; of a structure that cannot be planned, n_dir alone. */
typedef struct alignn_phsym_plan_args {
    const double* lattice;      /* [B][3][3] */
    const int32_t* supercell;   /* [B][3] */
    const int32_t* atom_ptr;    /* [B + 1] */
    const int64_t* op_ptr;      /* [B + 1] */
    const int64_t* map_ptr;     /* [B + 1] */
    const int32_t* rotations;   /* [G][3][3] */
    const int32_t* atom_map;    /* [map_ptr[B]] */
    int32_t* usable;            /* [G] */
    double* rot;                /* [G][3][3] */
    int32_t* rep;               /* [N] */
    int32_t* n_site;            /* [N] */
    int32_t* site_ops;          /* [N][48] */
    int32_t* n_dir;             /* [N] */
    double* dirs;               /* [N][3][3] */
    double* minv;               /* [N][3][3] */
    int32_t* dist_op;           /* [N] */
    int64_t n_ops_total;        /* G >= 1 */
    int64_t n_map_total;        /* map_ptr[B] >= 1 */
    int n_structs;              /* B, 0 .. 65535 */
    int n_atoms;                /* N = atom_ptr[B] >= 1 */
} alignn_phsym_plan_args;
int alignn_phsym_plan(const alignn_phsym_plan_args* args, void* stream);
size_t alignn_phsym_plan_args_size(void); /* a binding checks its own packing against this */

/* _phsym_displace, one workgroup per displaced supercell: alignn_phonon_displace's arithmetic with a direction per job.  Job
 * (s, atom, m, sg): cart = ((r_b + m0 L0) + m1 L1) + m2 L2 for every supercell atom, then for atom `atom` of image 0
 * cart_k = cart_k + (sg ? delta : -delta) d_k with d = dirs[atom_ptr[s] + atom][m]; frac_c = wrap01((x S0c + y S1c) + z S2c)
 * with S the inverse supercell.  The rows of job q start at row_off[q] of frac (and of cart when it is given). */
typedef struct alignn_phsym_displace_args {
    const double* positions;      /* [N][3] Cartesian, N = atom_ptr[B] */
    const int32_t* atom_ptr;      /* [B + 1] */
    const double* lattice;        /* [B][3][3] */
    const double* inv_supercell;  /* [B][3][3] */
    const int32_t* supercell;     /* [B][3] */
    const double* dirs;           /* [N][3][3] (_phsym_plan) */
    const int32_t* jobs;          /* [n_jobs][4]: structure, atom, direction m, sign (0: -, 1: +) */
    const int64_t* row_off;       /* [n_jobs] */
    double* frac;                 /* [rows][3] wrapped fractional rows, rows = the sum over the jobs of their supercell atoms n_sc; every row is written */
    double* cart;                 /* [rows][3] unwrapped Cartesian rows, every one written; or NULL: only frac is written */
    double delta;                 /* finite, > 0 */
    int n_jobs;                   /* >= 0 */
    int n_structs;                /* B >= 1: the range of a job's structure */
} alignn_phsym_displace_args;
int alignn_phsym_displace(const alignn_phsym_displace_args* args, void* stream);
size_t alignn_phsym_displace_args_size(void);

/* _phsym_rows, one workgroup per -/+ pair: G [n_sc][3] = (F- - F+) / (2 delta) from the forces of the minus supercell (rows
 * from pair_rows[p]) and the plus supercell (the n_sc rows after), after the drift correction of alignn_phonon_fc_rows (drift
 * 0 none, 1 Frederiksen: the supercell's force sum off the displaced atom's row, 2 mean: sum / n_sc off every row; the kernels
 * share csrc/phonon_rows.h), written to the rows from out_rows[p] of g. */
typedef struct alignn_phsym_rows_args {
    const double* forces;       /* [force_rows][3], the rows of the chunk's supercells: twice the sum over the pairs of n_sc */
    const int32_t* pairs;       /* [n_pairs][2]: structure, displaced atom */
    const int64_t* pair_rows;   /* [n_pairs] */
    const int64_t* out_rows;    /* [n_pairs] */
    const int32_t* atom_ptr;    /* [B + 1] */
    const int32_t* supercell;   /* [B][3] */
    double* g;                  /* [g_rows][3], g_rows = the sum over every direction of every representative of n_sc; a pair's n_sc rows are written */
    double delta;               /* finite, > 0 */
    int drift;                  /* 0, 1, 2 */
    int n_pairs;                /* >= 0 */
    int n_structs;              /* B >= 1 */
} alignn_phsym_rows_args;
int alignn_phsym_rows(const alignn_phsym_rows_args* args, void* stream);
size_t alignn_phsym_rows_args_size(void);

/* _phsym_solve (rule 5) and _phsym_distribute (rule 6), one launch each: a thread per (item, supercell atom B), the items
 * (structure, atom) being the representatives for _solve - g_rows[q] the first row in g of the item's direction 0, direction m
 * n_sc rows further - and the non-representatives for _distribute (after _solve: it reads the representatives' blocks of fc and
 * writes those of the others).  _solve stages the site group's W, Q_g, u_gm and Minv in LDS once per workgroup. */
typedef struct alignn_phsym_fc_args {
    const int32_t* items;       /* [n_items][2] */
    const int64_t* g_rows;      /* [n_items]                      (_solve) */
    const double* g;            /* [g_rows][3]                    (_solve) */
    double* fc;                 /* [fc_total], fc_total = the sum over the structures of (N0 N1 N2) (3 n_b)^2: the packed force constants.
                                 * _solve writes every block Phi(i; .) of its items, _distribute reads those and writes every block of its
                                 * items: the caller need not zero it */
    const int64_t* fc_off;      /* [B] */
    const int32_t* atom_ptr;    /* [B + 1] */
    const int32_t* supercell;   /* [B][3] */
    const int64_t* op_ptr;      /* [B + 1] */
    const int64_t* map_ptr;     /* [B + 1] */
    const int32_t* rotations;   /* [G][3][3] */
    const int32_t* atom_map;    /* [map_ptr[B]] */
    const int32_t* shifts;      /* [map_ptr[B]][3] */
    const double* rot;          /* [G][3][3]  (_phsym_plan) */
    const int32_t* rep;         /* [N]        (_distribute), N = atom_ptr[B] */
    const int32_t* n_site;      /* [N]        (_solve) */
    const int32_t* site_ops;    /* [N][48]    (_solve) */
    const int32_t* n_dir;       /* [N]        (_solve) */
    const double* dirs;         /* [N][3][3]  (_solve) */
    const double* minv;         /* [N][3][3]  (_solve) */
    const int32_t* dist_op;     /* [N]        (_distribute) */
    int64_t n_ops_total;        /* G >= 1 */
    int64_t n_map_total;        /* map_ptr[B] >= 1 */
    int n_items;                /* >= 0 */
    int n_structs;              /* B >= 1 */
    int max_supercell_atoms;    /* the largest n_sc of the items' structures (sizes the grid), >= 1 */
} alignn_phsym_fc_args;
int alignn_phsym_solve(const alignn_phsym_fc_args* args, void* stream);
int alignn_phsym_distribute(const alignn_phsym_fc_args* args, void* stream);
size_t alignn_phsym_fc_args_size(void);

#ifdef __cplusplus
}
#endif
#endif /* ALIGNN_PHSYM_H */
