/* alignn_voronoi.h - the entry points of libalignn_hip.so for the Voronoi analysis of MD trajectories: the Voronoi cell of every
 * atom of every frame used - its volume, its surface, its faces and the Voronoi index <n3, n4, n5, n6, ...> - with a certificate
 * that the cell is complete, and the per-frame means per species (csrc/voronoi.hip; alignn_amd/voronoi.py is the driver and binds
 * this header, tests/voronoi_ref.py the numpy restatement).
 *
 * A header of its own tuple (alignn_amd/_abi.py: STRUCTURE_HEADERS), in the regular form of the others (one extern "C" block, an
 * argument struct with its size query, prototypes over the base types): alignn_amd/_abi.py reads it.  Every pointer is a device
 * pointer; `stream` is a hipStream_t.  Every entry point returns 0 or the HIP error; hipErrorInvalidValue (1) for an argument out
 * of its range, before any launch and before any pointer is looked at.  No structures, or no selected frame, is a no-op that
 * returns 0.
 *
 * float64 without contraction, no atomics on floating-point values (the status word is set by an integer atomic OR), every
 * floating-point sum in a fixed order over the atom's own neighbour list: a structure's bits do not depend on the launch it is in,
 * nor on its place in it.
 *
 * The trajectory, the frame selection (frame0 + f * frame_step, f = 0 .. n_frames - 1), the groups (group 0 every atom, groups
 * 1 .. S_b the species in ascending atomic number, group[i] in 1 .. S_b, group_count [B][S + 1]) and the cells ([B][3][3] or
 * [n_total_frames][B][3][3]) are those of alignn_order.h, and so are the limits and the first two status bits, by value.
 *
 * Neighbour list.  For centre atom i of one frame, the candidates are the entries of the shared list (csrc/neighbor_list.h),
 * exactly as build_list defines them: (j, image) != (i, 0), r < r_cut[b], own images included, at most ALIGNN_VORO_MAX_NEIGHBORS,
 * in the order j ascending, then the image (m0, m1, m2) lexicographic, with
 *     df = (r_j - r_i) Cinv;  df -= rint(df);  d0 = df C;  d = d0 + ((m0 C0 + m1 C1) + m2 C2);  r = sqrt((dx dx + dy dy) + dz dz)
 * over |m_k| <= floor(r_cut / h_k + 1/2).  A range above ALIGNN_VORO_MAX_IMAGE_RANGE (or an r_cut that is not a finite number > 0)
 * sets ALIGNN_VORO_STATUS_IMAGES and the frame is skipped (its outputs are not written: the caller zeroes them, face_j to -1); more
 * than ALIGNN_VORO_MAX_NEIGHBORS entries set ALIGNN_VORO_STATUS_NEIGHBORS and that atom's outputs of that frame are zeros
 * (complete = 0, face_j = -1).
 *
 * Cell.  Entry a has the displacement d_a and gives the half-space d_a . x <= |d_a|^2 / 2.  The cell is the intersection of these
 * half-spaces.
 *
 * Face.  The face of entry a is its plane clipped by every other entry's half-space.  The polygon is kept as 2-D coordinates
 * (p, q) in an orthonormal basis (u, v) of the plane, x = d_a / 2 + p u + q v, chosen so: k the component of d_a of the smallest
 * magnitude (the first of equals), e_k that axis,
 *     t = e_k x d_a;  u = t / sqrt((tx tx + ty ty) + tz tz);  w = d_a x u;  v = w / r_a          (x: the vector product)
 * It starts as the square (-H, -H), (H, -H), (H, H), (-H, H) of half-side H = 4 r_cut and is clipped by the entries b != a in
 * list order (Sutherland-Hodgman on a convex polygon).  Entry b is the line A p + B q <= c,
 *     A = (bx ux + by uy) + bz uz;  B = (bx vx + by vy) + bz vz;  c = (r_b r_b - ((bx ax + by ay) + bz az)) / 2
 * a vertex has the slack s = c - (A p + B q) and is inside iff s >= 0.  With the last vertex as the first `prev`, for every vertex
 * `cur` in order: if one of prev, cur is inside and the other is not, the point prev + (s_prev / (s_prev - s_cur)) (cur - prev) is
 * put out, component by component; then cur, if it is inside.  A polygon that comes to more than ALIGNN_VORO_MAX_POLYGON vertices
 * sets ALIGNN_VORO_STATUS_POLYGON (the face stops there: a ValueError for the caller).  For each polygon of n vertices
 * (p_k, q_k), k = 0 .. n - 1:
 *   - its area A_a comes from a fan of triangles from its first vertex:
 *         A_a = (sum over k = 1 .. n - 2, from 0 in that order, of (p_k - p_0) (q_k+1 - q_0) - (q_k - q_0) (p_k+1 - p_0)) / 2
 *     (0 with fewer than 3 vertices);
 *   - its height is h_a = |d_a| / 2 = r_a / 2;
 *   - its edges are the polygon's sides k -> k + 1 (the last to the first), of length sqrt(dp dp + dq dq);
 *   - |vertex| = sqrt((h_a h_a + p p) + q q).
 *
 * Cell quantities.
 *   - volume = sum_a A_a h_a / 3 and area = sum_a A_a.  Both run over all faces in list order, thresholds or not: lane a of the
 *     wavefront holds the term (A_a h_a) / 3 or A_a of entry a (0 beyond the list) and the 64 are added by the xor butterfly
 *     (v = v + v[lane ^ 32], then ^ 16, 8, 4, 2, 1).
 *   - r_max is the largest |vertex| over all faces; an atom without a single entry has no face and r_max = +infinity.
 *
 * Counted faces.  An edge counts iff its length > edge_threshold (A).  A face counts iff all of these hold:
 *   - A_a > face_threshold (A^2);
 *   - A_a > relative_face_threshold * area (that product is rounded once);
 *   - it has at least 3 counted edges.
 * From the counted faces:
 *   - n_faces is their number.
 *   - index[.., k] is the number of counted faces with k + 3 counted edges, for k = 0 .. 7, i.e. 3 .. 10 edges.
 *   - Faces with more than 10 counted edges appear in n_faces only.
 * With thresholds of 0 a face counts when its area is > 0 and three of its sides are longer than 0.
 *
 * Certification.  A cell is complete iff r_max <= r_cut / 2.  In that case no atom outside the list can cut it: its plane lies at
 * least r_cut / 2 from the centre.  Each face starts from a square of half-side 4 r_cut in its plane: an unbounded cell then fails
 * the test by itself.  This covers slab-surface atoms next to vacuum, and an r_cut that is too small.  complete [n_frames][n_atoms]
 * is 1 or 0; incomplete cells keep their numbers as computed and are left out of `mean`.
 *
 * Faces (faces = 1).  The counted faces of an atom in list order, slot s = 0 .. n_faces - 1, at most ALIGNN_VORO_MAX_FACES: face_j
 * the index of the entry's atom within its structure, face_d its displacement d_a (which carries the image), face_area A_a,
 * face_edges its counted edges; the slots beyond n_faces hold -1 (face_j) or 0.  More than ALIGNN_VORO_MAX_FACES counted faces set
 * ALIGNN_VORO_STATUS_FACES (the first ALIGNN_VORO_MAX_FACES are written: a ValueError for the caller).
 *
 * _voro_cells: one wavefront per (frame used, atom), one wavefront per workgroup.  The list by ballot and prefix into LDS, lane a
 * owns entry a and clips its own polygon against the other entries.  The polygons live in LDS, two buffers of
 * ALIGNN_VORO_MAX_POLYGON vertices per lane, 2 x 32 x 16 B x 64 lanes = 64 KiB per wavefront, laid out [buffer][vertex][p|q][lane]
 * so that the 64 lanes of an access fall into 64 different banks.  With the list that is 66.5 KiB of the 160 KiB of a gfx950
 * compute unit: a workgroup holds ONE wavefront and a compute unit two workgroups - two wavefronts of 64 KiB do not leave room
 * for a third either way, and a workgroup of one needs no barrier.  Nothing per lane is indexed in private memory, so nothing
 * spills to scratch.
 * _voro_means: one workgroup per (frame used, structure); mean[b][g][f] = (the sums of volume, area and n_faces over the complete
 * atoms of group g) / their number n_complete[b][g][f], zeros for a group without a complete member.  The sums run in the fixed
 * order of csrc/group_rows.h: chunks of 256 rows in row order, in a chunk lane l adds its rows l, l + 64, l + 128, l + 192 in that
 * order from 0, then the xor butterfly, and the chunk's sum is added to the group's accumulator.
 */
#ifndef ALIGNN_VORONOI_H
#define ALIGNN_VORONOI_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ALIGNN_VORO_MAX_SPECIES 8      /* = ALIGNN_ORDER_MAX_SPECIES */
#define ALIGNN_VORO_MAX_IMAGE_RANGE 8  /* = ALIGNN_ORDER_MAX_IMAGE_RANGE */
#define ALIGNN_VORO_MAX_NEIGHBORS 64   /* = ALIGNN_ORDER_MAX_NEIGHBORS */
#define ALIGNN_VORO_MAX_POLYGON 32     /* vertices of a face polygon at any stage of the clipping */
#define ALIGNN_VORO_MAX_FACES 32       /* counted faces of one atom that faces = 1 stores */
#define ALIGNN_VORO_INDEX 8            /* the last axis of index: faces of 3 .. 10 counted edges */
#define ALIGNN_VORO_SQUARE 4.0         /* the half-side of a face's first square, in r_cut */
#define ALIGNN_VORO_STATUS_IMAGES 1    /* = ALIGNN_ORDER_STATUS_IMAGES */
#define ALIGNN_VORO_STATUS_NEIGHBORS 2 /* = ALIGNN_ORDER_STATUS_NEIGHBORS */
#define ALIGNN_VORO_STATUS_POLYGON 4   /* bit of *status: a face polygon exceeded ALIGNN_VORO_MAX_POLYGON vertices during clipping */
#define ALIGNN_VORO_STATUS_FACES 8     /* bit of *status: faces = 1 and an atom has more than ALIGNN_VORO_MAX_FACES counted faces */

typedef struct alignn_voro_args {
    const double* traj;         /* [n_total_frames][n_atoms][3]   (_voro_cells) */
    const double* lattice;      /* [B][3][3] (lattice_per_frame 0) or [n_total_frames][B][3][3] (1), row-major   (_voro_cells) */
    const int32_t* atom_ptr;    /* [B + 1], 0 first */
    const int32_t* group;       /* [n_atoms] */
    const int32_t* group_count; /* [B][S + 1]   (_voro_cells) */
    const double* r_cut;        /* [B]   (_voro_cells) */
    double* volume;             /* [n_frames][n_atoms]   (these six: _voro_cells writes every element of a frame without
                                 * ALIGNN_VORO_STATUS_IMAGES - a skipped frame is left to the caller's zeros; _voro_means reads volume, area,
                                 * n_faces and complete) */
    double* area;               /* [n_frames][n_atoms] */
    double* r_max;              /* [n_frames][n_atoms] */
    int32_t* n_faces;           /* [n_frames][n_atoms] */
    int32_t* index;             /* [n_frames][n_atoms][ALIGNN_VORO_INDEX] */
    int32_t* complete;          /* [n_frames][n_atoms], 1 / 0 */
    double* mean;               /* [B][S + 1][n_frames][3]: volume, area, n_faces   (_voro_means writes every element of these two) */
    int64_t* n_complete;        /* [B][S + 1][n_frames]   (_voro_means) */
    int32_t* face_j;            /* with faces = 1 (else not looked at), [n_frames][n_atoms][ALIGNN_VORO_MAX_FACES]   (these four:
                                 * _voro_cells, as the six above) */
    double* face_d;             /* [n_frames][n_atoms][ALIGNN_VORO_MAX_FACES][3] */
    double* face_area;          /* [n_frames][n_atoms][ALIGNN_VORO_MAX_FACES] */
    int32_t* face_edges;        /* [n_frames][n_atoms][ALIGNN_VORO_MAX_FACES] */
    int32_t* status;            /* [1], bits are ORed in (_voro_cells) */
    double face_threshold;      /* A^2, finite and >= 0 */
    double relative_face_threshold; /* of the cell's area, finite and >= 0 */
    double edge_threshold;      /* A, finite and >= 0 */
    int n_structs;              /* B >= 0 */
    int n_atoms;                /* atom_ptr[B] >= 0 */
    int max_atoms;              /* the largest n_b (sizes the launch), 1 .. n_atoms, at most 65535 */
    int n_species;              /* S, 1 .. ALIGNN_VORO_MAX_SPECIES */
    int n_total_frames;         /* >= 0 */
    int frame0;                 /* >= 0 */
    int frame_step;             /* >= 1 */
    int n_frames;               /* frames used, >= 0 */
    int lattice_per_frame;      /* 0 / 1 */
    int faces;                  /* 0 / 1 */
} alignn_voro_args;
int alignn_voro_cells(const alignn_voro_args* args, void* stream);
int alignn_voro_means(const alignn_voro_args* args, void* stream);
size_t alignn_voro_args_size(void); /* a binding checks its own packing against this */

#ifdef __cplusplus
}
#endif
#endif /* ALIGNN_VORONOI_H */
