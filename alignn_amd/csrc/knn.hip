// Periodic k-nearest-neighbour bond lists on the device, one wavefront per site.
//
// Reference: alignn/graphs.py:155-264 (nearest_neighbor_edges + build_undirected_edgedata + canonize_edge, :128-153) on
// jarvis' get_all_neighbors - rebuilt at EVERY molecular-dynamics step by the ASE calculators
// (alignn/ff/calculators.py:280-291).  Semantics restated (and pinned bit-exactly to the reference's own functions over
// its 70 example structures, tests/test_graph_builder_golden.py):
//   * candidates of site i: all (j, image I) with lo_k <= I_k <= hi_k and kBondTol < dist <= cutoff.  The box comes from
//     the caller (alignn_amd/neighbors.py: _image_box): |I_k| <= ceil(cutoff / plane spacing_k) for fractional coordinates
//     inside [0, 1], the box jarvis lays out around the fractional extent for unwrapped ones - which is NOT symmetric and
//     does not hold every image within the cutoff, so "b sees a at -I" is true only if -I is in the box too;
//   * some site of the crystal has fewer than k candidates -> the WHOLE crystal is redone with a larger cutoff
//     (longest lattice vector if the cutoff was below it, else twice the cutoff; :170-188) - a larger box can add
//     near neighbours the smaller box did not scan, so the level is a property of the crystal, not of the site;
//   * per site keep everything out to the distance of its k-th nearest candidate, ties included (:206-216);
//   * undirected multigraph keyed (smaller id, larger id, image seen from the smaller id): the union of what either end
//     kept; both directions of a bond are emitted as a consecutive pair, r = Cartesian displacement src -> dst (:230-264).
//
// Index work: the bar is bit-exact.  Tie decisions compare float64 distances, so every distance is evaluated as the SAME
// fixed sequence of IEEE operations as the numpy / torch restatements (alignn_amd/synthetic.py, neighbors.py):
// shift = (i0*a + i1*b) + i2*c ; d = (cart_j + shift) - cart_i ; dist = sqrt((dx*dx + dy*dy) + dz*dz), no fused
// multiply-add (contraction is switched off for this file's arithmetic).
//
// Shape of the work: a crystal of n atoms with an image box of I cells has n*I candidates per site (60 atoms, 27 images:
// 1 620) - the "cell list" of a cell that is about as large as the cutoff IS the image loop.  One wave per site scans
// its candidates 64 at a time; the k-th distance is the k-th smallest of the few dozen distances inside the cutoff, which
// the scan leaves in LDS (exact, ties included; beyond 1 024 of them: rounds of "smallest distance above the last one + its
// multiplicity"); the edge list is compacted in candidate order by ballot / popcount, so a
// site's bonds leave sorted by (neighbour, image) - the order torch.unique gives the torch builder.  No atomics on the
// output, no host synchronisation inside (the host reads ONE number - the total bond count - to size the output).
#include "common.h"
#include "../../include/alignn_hip.h"

namespace {

constexpr int kSitesPerBlock = 4;
constexpr int kThreads = kSitesPerBlock * ALIGNN_WAVE;
constexpr int kKthCap = 1024;  // distances inside the cutoff a site's wave keeps in LDS for the k-th smallest (more: the search by rounds)
constexpr double kBondTol = 0.15;  // jarvis' get_all_neighbors(r, bond_tol=0.15): closer than this is no neighbour

struct Cell {
    double lat[9];
    int lo[3], hi[3];    // image box scanned by the crystal's sites, inclusive
    int s0, s1, s2;      // first image of the ENUMERATED box (the scanned box, or its hull with its mirror image)
    int n1, n2, nimg;    // extents of the enumerated box along b and c, images in it
    double cutoff;
};

// HULL: enumerate the smallest box symmetric about 0 that holds the scanned one (the canonical image of a bond kept by
// its larger end is the NEGATIVE of an image that end scanned); for a symmetric box - wrapped coordinates - the same box.
template <bool HULL>
__device__ __forceinline__ Cell load_cell(const double* __restrict__ lat, const double* __restrict__ cut,
                                          const int32_t* __restrict__ box, int b, int L, int level) {
    Cell c;
#pragma unroll
    for (int i = 0; i < 9; ++i) c.lat[i] = lat[(size_t)b * 9 + i];
    const int32_t* r = box + ((size_t)b * L + level) * 6;
    int e[3][2];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        c.lo[k] = r[k], c.hi[k] = r[3 + k];
        e[k][0] = HULL ? min(c.lo[k], -c.hi[k]) : c.lo[k];
        e[k][1] = HULL ? max(c.hi[k], -c.lo[k]) : c.hi[k];
    }
    c.s0 = e[0][0], c.s1 = e[1][0], c.s2 = e[2][0];
    c.n1 = e[1][1] - e[1][0] + 1;
    c.n2 = e[2][1] - e[2][0] + 1;
    c.nimg = (e[0][1] - e[0][0] + 1) * c.n1 * c.n2;
    c.cutoff = cut[(size_t)b * L + level];
    return c;
}

__device__ __forceinline__ bool in_box(const Cell& c, int i0, int i1, int i2) {
    return i0 >= c.lo[0] && i0 <= c.hi[0] && i1 >= c.lo[1] && i1 <= c.hi[1] && i2 >= c.lo[2] && i2 <= c.hi[2];
}

// distance of (cart_j + shift(image)) from cart_i, in the reference's operation order
__device__ __forceinline__ double image_distance(const Cell& c, const double ci[3], const double cj[3], int i0, int i1,
                                                 int i2) {
#pragma clang fp contract(off)
    double d[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const double s = ((double)i0 * c.lat[k] + (double)i1 * c.lat[3 + k]) + (double)i2 * c.lat[6 + k];
        d[k] = (cj[k] + s) - ci[k];
    }
    return __dsqrt_rn((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]);
}

// candidate index -> (j, image): candidates are ordered by (j, i0, i1, i2), images ascending from the box's first
__device__ __forceinline__ void split_candidate(const Cell& c, int cand, int& j, int& i0, int& i1, int& i2) {
    j = cand / c.nimg;
    int im = cand - j * c.nimg;
    const int q = c.n1 * c.n2;
    i0 = im / q;
    im -= i0 * q;
    i1 = im / c.n2;
    i2 = im - i1 * c.n2;
    i0 += c.s0;
    i1 += c.s1;
    i2 += c.s2;
}

// number of candidates of site i (global id) at the given level
__device__ __forceinline__ int count_candidates(const Cell& c, const double* __restrict__ cart, int base, int n, int i,
                                                int lane) {
    const double ci[3] = {cart[3 * (size_t)i], cart[3 * (size_t)i + 1], cart[3 * (size_t)i + 2]};
    const int total = n * c.nimg;
    int cnt = 0;
    for (int cand = lane; cand < total; cand += ALIGNN_WAVE) {
        int j, i0, i1, i2;
        split_candidate(c, cand, j, i0, i1, i2);
        const double cj[3] = {cart[3 * (size_t)(base + j)], cart[3 * (size_t)(base + j) + 1], cart[3 * (size_t)(base + j) + 2]};
        const double d = image_distance(c, ci, cj, i0, i1, i2);
        cnt += (d <= c.cutoff && d > kBondTol) ? 1 : 0;
    }
    return wave_sum(cnt);
}

// ---- pass 0: the image box of every crystal at every level, from the fractional extent of its sites (one wave per
// crystal).  Axis with floor(min frac) == 0 and ceil(max frac) <= 1: [-reach, reach]; otherwise jarvis' box
// [floor(min) - maxr, ceil(max) + maxr - 1] (the rule of alignn_amd/neighbors.py: _image_box).  A box whose candidate count
// would not fit the kernels' 32-bit candidate index (absurd coordinates, NaN) is written EMPTY (lo 0, hi -1): the crystal
// then finds no neighbour at any level and the caller raises.
__global__ __launch_bounds__(ALIGNN_WAVE) void knn_box_kernel(const double* __restrict__ frac,
                                                              const int32_t* __restrict__ graph_ptr,
                                                              const int32_t* __restrict__ reach,
                                                              const int32_t* __restrict__ maxr, int L,
                                                              int32_t* __restrict__ box) {
    const int lane = threadIdx.x, b = blockIdx.x;
    const int base = graph_ptr[b], n = graph_ptr[b + 1] - base;
    const double inf = __longlong_as_double(0x7ff0000000000000LL);
    double mn0 = inf, mn1 = inf, mn2 = inf, mx0 = -inf, mx1 = -inf, mx2 = -inf;
    bool bad = false;
    for (int j = lane; j < n; j += ALIGNN_WAVE) {
        const double* f = frac + 3 * (size_t)(base + j);
        mn0 = fmin(mn0, f[0]), mn1 = fmin(mn1, f[1]), mn2 = fmin(mn2, f[2]);
        mx0 = fmax(mx0, f[0]), mx1 = fmax(mx1, f[1]), mx2 = fmax(mx2, f[2]);
        bad |= !(fabs(f[0]) < 1e6 && fabs(f[1]) < 1e6 && fabs(f[2]) < 1e6);  // (NaN included)
    }
    mn0 = wave_min(mn0), mn1 = wave_min(mn1), mn2 = wave_min(mn2);
    mx0 = -wave_min(-mx0), mx1 = -wave_min(-mx1), mx2 = -wave_min(-mx2);
    bad = __ballot(bad) != 0ull || n <= 0;
    const int flo[3] = {bad ? 0 : (int)floor(mn0), bad ? 0 : (int)floor(mn1), bad ? 0 : (int)floor(mn2)};
    const int fhi[3] = {bad ? 0 : (int)ceil(mx0), bad ? 0 : (int)ceil(mx1), bad ? 0 : (int)ceil(mx2)};
    for (int level = lane; level < L; level += ALIGNN_WAVE) {
        const int32_t* r = reach + ((size_t)b * L + level) * 3;
        const int32_t* m = maxr + ((size_t)b * L + level) * 3;
        int lo[3], hi[3];
        long long images = 1;  // of the hull with the mirrored box: what the bond passes enumerate (>= the scanned box)
        bool fits = !bad;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const bool wrapped = flo[k] == 0 && fhi[k] <= 1;
            const long long l = wrapped ? -(long long)r[k] : (long long)flo[k] - m[k];
            const long long h = wrapped ? (long long)r[k] : (long long)fhi[k] + m[k] - 1;
            const long long a = l < -h ? l : -h, z = h > -l ? h : -l;
            fits = fits && r[k] >= 0 && m[k] >= 0 && z - a + 1 <= (1 << 20);
            images *= fits ? z - a + 1 : 1;
            fits = fits && images * (long long)n <= (long long)INT32_MAX;
            lo[k] = (int)l, hi[k] = (int)h;
        }
        int32_t* o = box + ((size_t)b * L + level) * 6;
#pragma unroll
        for (int k = 0; k < 3; ++k) o[k] = fits ? lo[k] : 0, o[3 + k] = fits ? hi[k] : -1;
    }
}

// ---- pass 1: the crystal's level = the first cutoff of its sequence at which EVERY site has >= k candidates
__global__ __launch_bounds__(kThreads) void knn_level_kernel(const double* __restrict__ lat, const double* __restrict__ cart,
                                                             const int32_t* __restrict__ graph_ptr,
                                                             const int32_t* __restrict__ site_graph,
                                                             const double* __restrict__ cut,
                                                             const int32_t* __restrict__ box, int L, int k, int N,
                                                             int32_t* __restrict__ crystal_level) {
    const int lane = threadIdx.x & 63;
    const int i = blockIdx.x * kSitesPerBlock + (threadIdx.x >> 6);
    if (i >= N) return;
    const int b = site_graph[i], base = graph_ptr[b], n = graph_ptr[b + 1] - base;
    int level = 0;
    for (; level < L; ++level) {
        const Cell c = load_cell<false>(lat, cut, box, b, L, level);
        if (count_candidates(c, cart, base, n, i, lane) >= k) break;
    }
    // (level == L: not even the widest cutoff reaches k candidates - reported to the host through the level array)
    if (lane == 0 && level > 0) atomicMax(crystal_level + b, level);  // integer max: order independent
}

// ---- pass 2: distance of the k-th nearest candidate of every site, at the crystal's level
__global__ __launch_bounds__(kThreads) void knn_kth_kernel(const double* __restrict__ lat, const double* __restrict__ cart,
                                                           const int32_t* __restrict__ graph_ptr,
                                                           const int32_t* __restrict__ site_graph,
                                                           const double* __restrict__ cut, const int32_t* __restrict__ box,
                                                           int L, int k, int N, const int32_t* __restrict__ crystal_level,
                                                           double* __restrict__ kth) {
    const int lane = threadIdx.x & 63;
    const int i = blockIdx.x * kSitesPerBlock + (threadIdx.x >> 6);
    if (i >= N) return;
    const int b = site_graph[i], base = graph_ptr[b], n = graph_ptr[b + 1] - base;
    const int level = crystal_level[b];
    if (level >= L) {
        if (lane == 0) kth[i] = -1.0;
        return;
    }
    const Cell c = load_cell<false>(lat, cut, box, b, L, level);
    const double ci[3] = {cart[3 * (size_t)i], cart[3 * (size_t)i + 1], cart[3 * (size_t)i + 2]};
    const int total = n * c.nimg;
    const double inf = __longlong_as_double(0x7ff0000000000000LL);
    // ONE scan: the distances inside the cutoff (a few dozen of the n * I candidates) go to the wave's list in LDS, compacted
    // by ballot / popcount; the k-th smallest of the list is the element x with #(y < x) < k <= #(y <= x) - ties included, the
    // same number the round-by-round search below returns (round 5: 600 -> ~30 us for a 200-atom cell, where that search -
    // up to k rounds of two scans each - was three quarters of the neighbour list's time).
    __shared__ double sh_d[kSitesPerBlock][kKthCap];
    double* buf = sh_d[threadIdx.x >> 6];
    int M = 0;  // (wave-uniform)
    for (int cand0 = 0; cand0 < total; cand0 += ALIGNN_WAVE) {
        const int cand = cand0 + lane;
        bool ok = false;
        double d = 0.0;
        if (cand < total) {
            int j, i0, i1, i2;
            split_candidate(c, cand, j, i0, i1, i2);
            const double cj[3] = {cart[3 * (size_t)(base + j)], cart[3 * (size_t)(base + j) + 1], cart[3 * (size_t)(base + j) + 2]};
            d = image_distance(c, ci, cj, i0, i1, i2);
            ok = d > kBondTol && d <= c.cutoff;
        }
        const unsigned long long mask = __ballot(ok);
        const int pos = M + __popcll(mask & ((1ull << lane) - 1ull));
        if (ok && pos < kKthCap) buf[pos] = d;
        M += __popcll(mask);
    }
    double last = kBondTol;
    if (M <= kKthCap) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        double best = inf, top = kBondTol;
        for (int q = lane; q < M; q += ALIGNN_WAVE) {
            const double x = buf[q];
            int lt = 0, le = 0;
            for (int t = 0; t < M; ++t) {
                const double y = buf[t];
                lt += y < x ? 1 : 0;
                le += y <= x ? 1 : 0;
            }
            if (lt < k && k <= le) best = x;
            top = fmax(top, x);
        }
        best = wave_min(best);
        // (fewer than k candidates cannot happen - the level guarantees k -; the search below would end at the largest one)
        last = best < inf ? best : -wave_min(-top);
        if (lane == 0) kth[i] = last;
        return;
    }
    // more candidates inside the cutoff than the list holds: ascending over the DISTINCT distances, `last` = the largest
    // distance accounted for, `seen` = candidates <= last
    int seen = 0;
    while (seen < k) {
        double mn = inf;
        for (int cand = lane; cand < total; cand += ALIGNN_WAVE) {
            int j, i0, i1, i2;
            split_candidate(c, cand, j, i0, i1, i2);
            const double cj[3] = {cart[3 * (size_t)(base + j)], cart[3 * (size_t)(base + j) + 1], cart[3 * (size_t)(base + j) + 2]};
            const double d = image_distance(c, ci, cj, i0, i1, i2);
            if (d > last && d <= c.cutoff) mn = fmin(mn, d);
        }
        mn = wave_min(mn);
        if (!(mn < inf)) break;  // (cannot happen: the level guarantees k candidates)
        int mult = 0;
        for (int cand = lane; cand < total; cand += ALIGNN_WAVE) {
            int j, i0, i1, i2;
            split_candidate(c, cand, j, i0, i1, i2);
            const double cj[3] = {cart[3 * (size_t)(base + j)], cart[3 * (size_t)(base + j) + 1], cart[3 * (size_t)(base + j) + 2]};
            mult += image_distance(c, ci, cj, i0, i1, i2) == mn ? 1 : 0;
        }
        seen += wave_sum(mult);
        last = mn;
    }
    if (lane == 0) kth[i] = last;
}

// Is the canonical bond (a, b, image of b seen from a), a <= b, in the graph?  Kept by a: +im is an image a scanned and
// a's own distance to (b, +im) is within a's shell; kept by b: -im is an image b scanned and b's distance to (a, -im) -
// evaluated the way b's wave evaluates it - is within b's shell.
__device__ __forceinline__ bool bond_exists(const Cell& c, const double ca[3], const double cb[3], bool same, int i0, int i1,
                                            int i2, double kth_a, double kth_b) {
    if (in_box(c, i0, i1, i2)) {
        const double da = image_distance(c, ca, cb, i0, i1, i2);
        if (da > kBondTol && da <= c.cutoff && da <= kth_a) return true;
    }
    if (same || !in_box(c, -i0, -i1, -i2)) return false;  // a == b: (a, a, im) and (a, a, -im) are separate keys, each kept on its own
    const double db = image_distance(c, cb, ca, -i0, -i1, -i2);
    return db > kBondTol && db <= c.cutoff && db <= kth_b;
}

// ---- pass 3 (COUNT) / pass 4 (EMIT): canonical bonds owned by site a = those to sites b >= a
template <bool EMIT>
__global__ __launch_bounds__(kThreads) void knn_bonds_kernel(const double* __restrict__ lat, const double* __restrict__ cart,
                                                             const int32_t* __restrict__ graph_ptr,
                                                             const int32_t* __restrict__ site_graph,
                                                             const double* __restrict__ cut, const int32_t* __restrict__ box,
                                                             int L, int N, const int32_t* __restrict__ crystal_level,
                                                             const double* __restrict__ kth, int64_t* __restrict__ count,
                                                             const int64_t* __restrict__ offset, int64_t* __restrict__ U,
                                                             int64_t* __restrict__ V, float* __restrict__ R,
                                                             int32_t* __restrict__ IMG) {
    const int lane = threadIdx.x & 63;
    const int a = blockIdx.x * kSitesPerBlock + (threadIdx.x >> 6);
    if (a >= N) return;
    const int b_ = site_graph[a], base = graph_ptr[b_], n = graph_ptr[b_ + 1] - base;
    const int level = crystal_level[b_];
    if (level >= L) {
        if (!EMIT && lane == 0) count[a] = 0;
        return;
    }
    const Cell c = load_cell<true>(lat, cut, box, b_, L, level);
    const double ca[3] = {cart[3 * (size_t)a], cart[3 * (size_t)a + 1], cart[3 * (size_t)a + 2]};
    const double kth_a = kth[a];
    const int la = a - base;
    const int total = (n - la) * c.nimg;  // candidates (b, im) with local id of b >= la, in (b, image) order
    int64_t pos = EMIT ? offset[a] : 0;  // bonds (not directed edges) before this site's
    int cnt = 0;
    for (int c0 = 0; c0 < total; c0 += ALIGNN_WAVE) {
        const int cand = c0 + lane;
        bool keep = false;
        int j = 0, i0 = 0, i1 = 0, i2 = 0;
        if (cand < total) {
            split_candidate(c, cand, j, i0, i1, i2);
            j += la;
            const size_t gb = (size_t)(base + j);
            const double cb[3] = {cart[3 * gb], cart[3 * gb + 1], cart[3 * gb + 2]};
            keep = bond_exists(c, ca, cb, j == la, i0, i1, i2, kth_a, kth[gb]);
        }
        const unsigned long long mask = __ballot(keep);
        if (EMIT && keep) {
            const int64_t e = pos + __popcll(mask & ((1ull << lane) - 1ull));
            const size_t gb = (size_t)(base + j);
            // r = cart(b) + shift(im) - cart(a) as one float64 expression of the FRACTIONAL difference, like
            // build_undirected_edgedata (:245-250): d = lattice.cart_coords(frac_b + im - frac_a); here from the
            // Cartesian positions (equal to rounding, the bar the golden test sets for the float32 bond vectors)
            double d[3];
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const double s = ((double)i0 * c.lat[k] + (double)i1 * c.lat[3 + k]) + (double)i2 * c.lat[6 + k];
                d[k] = (cart[3 * gb + k] + s) - ca[k];
            }
            U[2 * e] = a, V[2 * e] = (int64_t)gb;
            U[2 * e + 1] = (int64_t)gb, V[2 * e + 1] = a;
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                R[3 * (2 * e) + k] = (float)d[k];
                R[3 * (2 * e + 1) + k] = (float)(-d[k]);
            }
            if (IMG) {
                IMG[3 * (2 * e)] = i0, IMG[3 * (2 * e) + 1] = i1, IMG[3 * (2 * e) + 2] = i2;
                IMG[3 * (2 * e + 1)] = i0, IMG[3 * (2 * e + 1) + 1] = i1, IMG[3 * (2 * e + 1) + 2] = i2;  // (forward image for both, like the reference)
            }
        }
        const int got = __popcll(mask);
        pos += got;
        cnt += got;
    }
    if (!EMIT && lane == 0) count[a] = cnt;
}

}  // namespace

extern "C" {

int alignn_knn_box(const double* frac, const int32_t* graph_ptr, const int32_t* reach, const int32_t* maxr, int levels,
                   int64_t n_crystals, int32_t* box, alignn_stream_t stream) {
    if (levels <= 0 || n_crystals < 0 || n_crystals > INT32_MAX || !box) return (int)hipErrorInvalidValue;
    if (n_crystals == 0) return 0;
    hipLaunchKernelGGL(knn_box_kernel, dim3((unsigned)n_crystals), dim3(ALIGNN_WAVE), 0, (hipStream_t)stream, frac, graph_ptr,
                       reach, maxr, levels, box);
    ALIGNN_CHECK_LAUNCH();
    return 0;
}

int alignn_knn_levels(const double* lat, const double* cart, const int32_t* graph_ptr, const int32_t* site_graph,
                      const double* cut, const int32_t* box, int levels, int k, int64_t n_sites, int32_t* crystal_level,
                      alignn_stream_t stream) {
    if (levels <= 0 || k <= 0 || n_sites < 0 || n_sites > INT32_MAX) return (int)hipErrorInvalidValue;
    if (n_sites == 0) return 0;
    hipLaunchKernelGGL(knn_level_kernel, dim3(alignn_ceil_div(n_sites, kSitesPerBlock)), dim3(kThreads), 0, (hipStream_t)stream,
                       lat, cart, graph_ptr, site_graph, cut, box, levels, k, (int)n_sites, crystal_level);
    ALIGNN_CHECK_LAUNCH();
    return 0;
}

int alignn_knn_kth(const double* lat, const double* cart, const int32_t* graph_ptr, const int32_t* site_graph,
                   const double* cut, const int32_t* box, int levels, int k, int64_t n_sites, const int32_t* crystal_level,
                   double* kth, alignn_stream_t stream) {
    if (levels <= 0 || k <= 0 || n_sites < 0 || n_sites > INT32_MAX) return (int)hipErrorInvalidValue;
    if (n_sites == 0) return 0;
    hipLaunchKernelGGL(knn_kth_kernel, dim3(alignn_ceil_div(n_sites, kSitesPerBlock)), dim3(kThreads), 0, (hipStream_t)stream, lat,
                       cart, graph_ptr, site_graph, cut, box, levels, k, (int)n_sites, crystal_level, kth);
    ALIGNN_CHECK_LAUNCH();
    return 0;
}

int alignn_knn_count(const double* lat, const double* cart, const int32_t* graph_ptr, const int32_t* site_graph,
                     const double* cut, const int32_t* box, int levels, int64_t n_sites, const int32_t* crystal_level,
                     const double* kth, int64_t* count, alignn_stream_t stream) {
    if (levels <= 0 || n_sites < 0 || n_sites > INT32_MAX) return (int)hipErrorInvalidValue;
    if (n_sites == 0) return 0;
    hipLaunchKernelGGL(knn_bonds_kernel<false>, dim3(alignn_ceil_div(n_sites, kSitesPerBlock)), dim3(kThreads), 0,
                       (hipStream_t)stream, lat, cart, graph_ptr, site_graph, cut, box, levels, (int)n_sites, crystal_level, kth,
                       count, nullptr, nullptr, nullptr, nullptr, nullptr);
    ALIGNN_CHECK_LAUNCH();
    return 0;
}

int alignn_knn_emit(const double* lat, const double* cart, const int32_t* graph_ptr, const int32_t* site_graph,
                    const double* cut, const int32_t* box, int levels, int64_t n_sites, const int32_t* crystal_level,
                    const double* kth, const int64_t* offset, int64_t* u, int64_t* v, float* r, int32_t* image,
                    alignn_stream_t stream) {
    if (levels <= 0 || n_sites < 0 || n_sites > INT32_MAX || !u || !v || !r) return (int)hipErrorInvalidValue;
    if (n_sites == 0) return 0;
    hipLaunchKernelGGL(knn_bonds_kernel<true>, dim3(alignn_ceil_div(n_sites, kSitesPerBlock)), dim3(kThreads), 0,
                       (hipStream_t)stream, lat, cart, graph_ptr, site_graph, cut, box, levels, (int)n_sites, crystal_level, kth,
                       nullptr, offset, u, v, r, image);
    ALIGNN_CHECK_LAUNCH();
    return 0;
}

int alignn_knn_kth_cap(void) { return kKthCap; }

}  // extern "C"
