// Device side of the Voronoi analysis (alignn_amd/voronoi.py): the Voronoi cell of every atom of every frame used of a run_md
// trajectory - volume, surface, faces, the Voronoi index - with the certificate that the cell is complete, and the means per
// species.  The reference has none of it; tests/voronoi_ref.py is the numpy restatement, include/alignn_voronoi.h states the rules,
// the formulas, the layouts and every field of the argument block.
//
//   voro_cells_kernel   one wavefront per (frame, centre atom), one per workgroup: the neighbour list by ballot and prefix into LDS
//                       (neighbor_list.h's build_list, the list of cna_kernel), lane a the face of entry a: a square in the plane
//                       of the entry, clipped by the half-spaces of the other entries (Sutherland-Hodgman, 2-D coordinates in the
//                       plane), then area, sides and the farthest vertex of what is left; volume, area and r_max by butterflies,
//                       the counted faces and the index by ballots.  A face needs no other face: no shared topology.
//   voro_means_kernel   one workgroup per (frame, structure): the sums over the complete atoms of a group (group_rows.h).
//
// The polygons are in LDS, [buffer][vertex][p | q][lane]: 2 x 32 x 2 x 64 doubles = 64 KiB per wavefront.  A lane reads and writes
// its own column only (no fence between the clips), and lanes at different vertices still fall into different banks.  With the list
// a workgroup takes 66.5 KiB of a compute unit's 160 KiB: two workgroups of one wavefront each per compute unit (the header says
// why one).  float64, no contraction, no atomics on floating-point values, every sum in a fixed order over the atom's own list: a
// structure's bits are the same alone, in a batch and at any place of the batch.
#include "../../include/alignn_voronoi.h"
#include "group_rows.h"
#include "neighbor_list.h"

#pragma clang fp contract(off)

namespace {

constexpr int BLOCK_FRAMES = 4;  // frames used per workgroup, one after the other
constexpr int NBR = ALIGNN_VORO_MAX_NEIGHBORS, MAXP = ALIGNN_VORO_MAX_POLYGON, MAXF = ALIGNN_VORO_MAX_FACES;
constexpr int NIDX = ALIGNN_VORO_INDEX, MAXS = ALIGNN_VORO_MAX_SPECIES;
constexpr int POLY = MAXP * 2 * ALIGNN_WAVE;  // the doubles of one buffer

using Args = alignn_voro_args;

static_assert(NBR == NEIGHBOR_LIST_CAP, "the list of neighbor_list.h");
static_assert(MAXF <= ALIGNN_WAVE, "a lane per stored face");
static_assert((2 * POLY + NBR * 4) * 8 + NBR * 4 <= 80 * 1024, "two workgroups per compute unit");

// component c of vertex k of the lane's polygon in the buffer `buf`
__device__ __forceinline__ int slot(int buf, int k, int c, int lane) { return buf * POLY + (2 * k + c) * ALIGNN_WAVE + lane; }

__global__ __launch_bounds__(ALIGNN_WAVE) void voro_cells_kernel(const Args a) {
    __shared__ double nd[NBR][4];  // dx, dy, dz, r of the entries
    __shared__ int nj[NBR];        // their atoms
    __shared__ double poly[2 * POLY];
    const int fc = blockIdx.x, il = blockIdx.y, b = blockIdx.z;
    const int beg = a.atom_ptr[b], n = a.atom_ptr[b + 1] - beg;
    if (n < 1 || beg < 0 || (int64_t)beg + n > a.n_atoms || il >= n) return;  // (uniform over the workgroup)
    const int lane = threadIdx.x;
    const int Sb = species_of(a.group_count, b, a.n_species);
    const int32_t* GR = a.group + beg;
    const double r_cut = a.r_cut[b];
    const double face_thr = a.face_threshold, rel_thr = a.relative_face_threshold, edge_thr = a.edge_threshold;

    for (int fl = 0; fl < BLOCK_FRAMES; ++fl) {
        const int f = fc * BLOCK_FRAMES + fl;
        if (f >= a.n_frames) break;
        const int frame = a.frame0 + f * a.frame_step;
        double C[9], Ci[9];
        int M[3];
        if (!frame_cell(a.lattice, a.lattice_per_frame, a.n_structs, frame, b, r_cut, ALIGNN_VORO_MAX_IMAGE_RANGE, C, Ci, M) ||
            !(r_cut > 0.0)) {  // (or r_cut is not a number > 0)
            if (lane == 0) atomicOr(a.status, ALIGNN_VORO_STATUS_IMAGES);
            continue;
        }
        const double* X = a.traj + 3 * ((int64_t)frame * a.n_atoms + beg);
        wave_sync();  // (the list of the frame before has been read)
        const int count = build_list<true, false>(X, GR, n, il, Sb, C, Ci, M, r_cut, lane, nd, nj, nullptr);
        const int64_t row = (int64_t)f * a.n_atoms + beg + il;
        const bool listed = count <= NBR;
        if (!listed && lane == 0) atomicOr(a.status, ALIGNN_VORO_STATUS_NEIGHBORS);
        wave_sync();

        // ---- the face of entry `lane` ----
        const bool mine = listed && lane < count;
        int nv = 0, buf = 0;
        bool over = false;
        double ax = 0.0, ay = 0.0, az = 0.0, ra = 0.0, ux = 0.0, uy = 0.0, uz = 0.0, vx = 0.0, vy = 0.0, vz = 0.0;
        if (mine) {
            ax = nd[lane][0];
            ay = nd[lane][1];
            az = nd[lane][2];
            ra = nd[lane][3];
            const double fx = fabs(ax), fy = fabs(ay), fz = fabs(az);
            int k = 0;
            double fm = fx;
            if (fy < fm) {
                k = 1;
                fm = fy;
            }
            if (fz < fm) k = 2;
            const double tx = k == 0 ? 0.0 : (k == 1 ? az : -ay);  // e_k x d_a
            const double ty = k == 0 ? -az : (k == 1 ? 0.0 : ax);
            const double tz = k == 0 ? ay : (k == 1 ? -ax : 0.0);
            const double tn = sqrt((tx * tx + ty * ty) + tz * tz);
            ux = tx / tn;
            uy = ty / tn;
            uz = tz / tn;
            vx = (ay * uz - az * uy) / ra;  // d_a x u
            vy = (az * ux - ax * uz) / ra;
            vz = (ax * uy - ay * ux) / ra;
            const double H = ALIGNN_VORO_SQUARE * r_cut;
            poly[slot(0, 0, 0, lane)] = -H;
            poly[slot(0, 0, 1, lane)] = -H;
            poly[slot(0, 1, 0, lane)] = H;
            poly[slot(0, 1, 1, lane)] = -H;
            poly[slot(0, 2, 0, lane)] = H;
            poly[slot(0, 2, 1, lane)] = H;
            poly[slot(0, 3, 0, lane)] = -H;
            poly[slot(0, 3, 1, lane)] = H;
            nv = 4;
        }
        const int entries = listed ? count : 0;
        for (int e = 0; e < entries; ++e) {  // (uniform)
            const double bx = nd[e][0], by = nd[e][1], bz = nd[e][2], rb = nd[e][3];
            if (!mine || e == lane || nv == 0 || over) continue;
            const double A = (bx * ux + by * uy) + bz * uz, B = (bx * vx + by * vy) + bz * vz;
            const double c = (rb * rb - ((bx * ax + by * ay) + bz * az)) / 2.0;
            double pp = poly[slot(buf, nv - 1, 0, lane)], pq = poly[slot(buf, nv - 1, 1, lane)];
            double sp = c - (A * pp + B * pq);
            int o = 0;
            for (int k = 0; k < nv; ++k) {
                const double cp = poly[slot(buf, k, 0, lane)], cq = poly[slot(buf, k, 1, lane)];
                const double sc = c - (A * cp + B * cq);
                const bool in_p = sp >= 0.0, in_c = sc >= 0.0;
                if (in_p != in_c) {
                    if (o < MAXP) {
                        const double t = sp / (sp - sc);
                        poly[slot(buf ^ 1, o, 0, lane)] = pp + t * (cp - pp);
                        poly[slot(buf ^ 1, o, 1, lane)] = pq + t * (cq - pq);
                    }
                    ++o;
                }
                if (in_c) {
                    if (o < MAXP) {
                        poly[slot(buf ^ 1, o, 0, lane)] = cp;
                        poly[slot(buf ^ 1, o, 1, lane)] = cq;
                    }
                    ++o;
                }
                pp = cp;
                pq = cq;
                sp = sc;
            }
            if (o > MAXP) {
                over = true;
                o = MAXP;
            }
            nv = o;
            buf ^= 1;
        }

        // ---- what is left of it: area by the fan from vertex 0, the counted sides, the farthest vertex ----
        double area_a = 0.0, far = 0.0;
        const double h = ra / 2.0;
        int edges = 0;
        if (nv > 0) {
            const double p0 = poly[slot(buf, 0, 0, lane)], q0 = poly[slot(buf, 0, 1, lane)];
            double pp = poly[slot(buf, nv - 1, 0, lane)], pq = poly[slot(buf, nv - 1, 1, lane)];
            double fan = 0.0;
            for (int k = 0; k < nv; ++k) {
                const double cp = poly[slot(buf, k, 0, lane)], cq = poly[slot(buf, k, 1, lane)];
                const double dp = cp - pp, dq = cq - pq;
                edges += sqrt(dp * dp + dq * dq) > edge_thr ? 1 : 0;
                far = fmax(far, sqrt((h * h + cp * cp) + cq * cq));
                if (k >= 2) fan = fan + ((pp - p0) * (cq - q0) - (pq - q0) * (cp - p0));
                pp = cp;
                pq = cq;
            }
            area_a = fan / 2.0;
        }
        const double area = wave_sum(area_a);
        const double volume = wave_sum((area_a * h) / 3.0);
        double r_max = wave_max(far);
        if (entries == 0) r_max = listed ? (double)INFINITY : 0.0;
        const bool counted = mine && area_a > face_thr && area_a > rel_thr * area && edges >= 3;
        const unsigned long long mask = __ballot(counted);
        const int n_faces = __popcll(mask);
        int idx[NIDX];
#pragma unroll
        for (int k = 0; k < NIDX; ++k) idx[k] = __popcll(__ballot(counted && edges == k + 3));
        if (__any(over) && lane == 0) atomicOr(a.status, ALIGNN_VORO_STATUS_POLYGON);
        if (lane == 0) {
            a.volume[row] = volume;
            a.area[row] = area;
            a.r_max[row] = r_max;
            a.n_faces[row] = n_faces;
            a.complete[row] = (listed && r_max <= r_cut / 2.0) ? 1 : 0;
#pragma unroll
            for (int k = 0; k < NIDX; ++k) a.index[row * NIDX + k] = idx[k];
        }
        if (a.faces) {
            if (n_faces > MAXF && lane == 0) atomicOr(a.status, ALIGNN_VORO_STATUS_FACES);
            const int at = __popcll(mask & ((1ull << lane) - 1ull));
            if (counted && at < MAXF) {
                const int64_t s = row * MAXF + at;
                a.face_j[s] = nj[lane];
                a.face_d[3 * s] = ax;
                a.face_d[3 * s + 1] = ay;
                a.face_d[3 * s + 2] = az;
                a.face_area[s] = area_a;
                a.face_edges[s] = edges;
            }
            if (lane >= n_faces && lane < MAXF) {
                const int64_t s = row * MAXF + lane;
                a.face_j[s] = -1;
                a.face_d[3 * s] = 0.0;
                a.face_d[3 * s + 1] = 0.0;
                a.face_d[3 * s + 2] = 0.0;
                a.face_area[s] = 0.0;
                a.face_edges[s] = 0;
            }
        }
    }
}

__global__ __launch_bounds__(GROUP_ROWS_BLOCK) void voro_means_kernel(const Args a) {
    __shared__ double part[GROUP_ROWS_BLOCK][3];
    __shared__ int grp[GROUP_ROWS_BLOCK];
    __shared__ double acc[MAXS + 1][3];
    __shared__ int members[MAXS + 1];
    const int f = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    const int beg = a.atom_ptr[b], n = a.atom_ptr[b + 1] - beg;
    const int S = a.n_species, G = S + 1;
    const bool ok = n >= 1 && beg >= 0 && (int64_t)beg + n <= a.n_atoms;
    if (tid < G) {
        acc[tid][0] = 0.0;
        acc[tid][1] = 0.0;
        acc[tid][2] = 0.0;
        members[tid] = 0;
    }
    for (int c0 = 0; ok && c0 < n; c0 += GROUP_ROWS_BLOCK) {  // (uniform)
        __syncthreads();  // (the chunk before has been added)
        const int r = c0 + tid;
        int g = 0;
        double v0 = 0.0, v1 = 0.0, v2 = 0.0;
        if (r < n) {
            const int64_t row = (int64_t)f * a.n_atoms + beg + r;
            const int gi = a.group[beg + r];
            if (a.complete[row] != 0 && gi >= 1 && gi <= S) {
                g = gi;
                v0 = a.volume[row];
                v1 = a.area[row];
                v2 = (double)a.n_faces[row];
                atomicAdd(members, 1);
                atomicAdd(members + g, 1);
            }
        }
        part[tid][0] = v0;
        part[tid][1] = v1;
        part[tid][2] = v2;
        grp[tid] = g;
        __syncthreads();
        group_rows_add<3>(part, grp, acc, S);
    }
    __syncthreads();
    if (tid < G * 3) {
        const int g = tid / 3, c = tid - 3 * g;
        const double m = (double)members[g];
        a.mean[(((int64_t)b * G + g) * a.n_frames + f) * 3 + c] = m > 0.0 ? acc[g][c] / m : 0.0;
    }
    if (tid < G) a.n_complete[((int64_t)b * G + tid) * a.n_frames + f] = (int64_t)members[tid];
}

// the frame selection: every frame used lies inside the trajectory
bool frames_ok(int n_total, int frame0, int step, int n_frames) {
    if (n_total < 0 || frame0 < 0 || step < 1 || n_frames < 0) return false;
    return n_frames == 0 || (int64_t)frame0 + (int64_t)(n_frames - 1) * step < n_total;
}

bool threshold_ok(double x) { return x >= 0.0 && x <= 1.7976931348623157e308; }  // (a NaN fails both)

bool args_ok(const Args& a) {
    if (a.n_structs < 0 || a.n_structs > 65535 || a.n_atoms < 0 || a.n_species < 1 || a.n_species > MAXS || a.lattice_per_frame < 0 ||
        a.lattice_per_frame > 1 || a.faces < 0 || a.faces > 1)
        return false;
    if (!threshold_ok(a.face_threshold) || !threshold_ok(a.relative_face_threshold) || !threshold_ok(a.edge_threshold)) return false;
    return frames_ok(a.n_total_frames, a.frame0, a.frame_step, a.n_frames);
}

}  // namespace

extern "C" size_t alignn_voro_args_size(void) { return sizeof(alignn_voro_args); }

extern "C" int alignn_voro_cells(const alignn_voro_args* args, void* stream) {
    if (!args || !args_ok(*args)) return (int)hipErrorInvalidValue;
    const Args& a = *args;
    if (a.n_structs == 0 || a.n_frames == 0) return 0;
    if (a.n_atoms < 1 || a.max_atoms < 1 || a.max_atoms > a.n_atoms || a.max_atoms > 65535) return (int)hipErrorInvalidValue;
    if (!a.traj || !a.lattice || !a.atom_ptr || !a.group || !a.group_count || !a.r_cut || !a.volume || !a.area || !a.r_max ||
        !a.n_faces || !a.index || !a.complete || !a.status)
        return (int)hipErrorInvalidValue;
    if (a.faces && (!a.face_j || !a.face_d || !a.face_area || !a.face_edges)) return (int)hipErrorInvalidValue;
    voro_cells_kernel<<<dim3(alignn_ceil_div(a.n_frames, BLOCK_FRAMES), a.max_atoms, a.n_structs), ALIGNN_WAVE, 0, (hipStream_t)stream>>>(a);
    ALIGNN_CHECK_LAUNCH();
    return 0;
}

extern "C" int alignn_voro_means(const alignn_voro_args* args, void* stream) {
    if (!args || !args_ok(*args)) return (int)hipErrorInvalidValue;
    const Args& a = *args;
    if (a.n_structs == 0 || a.n_frames == 0) return 0;
    if (a.n_atoms < 1 || !a.atom_ptr || !a.group || !a.volume || !a.area || !a.n_faces || !a.complete || !a.mean || !a.n_complete)
        return (int)hipErrorInvalidValue;
    voro_means_kernel<<<dim3(a.n_frames, a.n_structs), GROUP_ROWS_BLOCK, 0, (hipStream_t)stream>>>(a);
    ALIGNN_CHECK_LAUNCH();
    return 0;
}
