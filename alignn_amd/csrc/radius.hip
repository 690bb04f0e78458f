// Radius bond graphs on the device, one wavefront per site (second half).
//
// Reference: alignn/graphs.py:267-364 (radius_graph) - the neighbour strategy the reference's force-field configs select
// (alignn/examples/sample_data_ff/config_example_atomwise.json:6,37) and alignn/ff/calculators.py:280-291 therefore re-runs
// at every molecular-dynamics step.  Semantics restated (and pinned to the reference's own function over its 70 example
// structures, edge ORDER included: tests/test_radius_graph.py):
//   * candidates of site i: (periodic image I, site j) for every image of the box [nmin, nmax) per axis (graphs.py:296-309:
//     floor / ceil of the fractional extent widened by ceil((cutoff + 0.5) / plane spacing) - the caller lays the box out);
//   * kept: atol < dist <= cutoff (torch.isclose(dist, 0, atol) excluded), in torch.where order: by source i, then by the
//     flat index image * n + j of the destination (image index lexicographic, first axis major);
//   * the graph lacks the crystal's LAST site (dgl.graph((u, v)).num_nodes() != n) -> the whole crystal is redone with
//     cutoff + 0.5 (:349-358).  In a periodic box that covers the cutoff the pair (i, I, j) is kept iff (j, -I, i) is, so
//     "the last site appears" == "the last site has a neighbour": one wave per crystal decides the level.
//   * u, v, r = x_dst - x_src, image (the box offsets); both directions of a bond exist but are NOT adjacent.
// float32 arithmetic like the reference (torch.get_default_dtype()), evaluated as ONE fixed sequence of IEEE operations
// shared with the torch twin (alignn_amd/neighbors._radius_pass): shift = (i0*a + i1*b) + i2*c ; x = shift + cart_j ;
// d = cart_i - x ; dist = sqrt((dx*dx + dy*dy) + dz*dz); no fused multiply-add (contraction off).
// One wave scans its candidates 64 at a time and compacts the kept ones by ballot / popcount: a site's bonds leave in
// candidate order, sites in order - the reference's order with no sort and no atomics; the host reads ONE number (the
// total bond count, to size the output).
#include "common.h"
#include "../../include/alignn_hip.h"

namespace {

constexpr int kSitesPerBlock = 4;
constexpr int kThreads = kSitesPerBlock * ALIGNN_WAVE;

struct Box {
    float lat[9];
    int lo0, lo1, lo2;  // first image per axis
    int n1, n2, nimg;   // extents of axes 1, 2; images in the box
    float cutoff;
};

__device__ __forceinline__ Box load_box(const float* __restrict__ lat, const int32_t* __restrict__ box,
                                        const float* __restrict__ cut, int b, int L, int level) {
    Box c;
#pragma unroll
    for (int i = 0; i < 9; ++i) c.lat[i] = lat[(size_t)b * 9 + i];
    const int32_t* q = box + ((size_t)b * L + level) * 6;  // nmin[3], nmax[3]
    c.lo0 = q[0], c.lo1 = q[1], c.lo2 = q[2];
    const int n0 = q[3] - q[0];
    c.n1 = q[4] - q[1];
    c.n2 = q[5] - q[2];
    c.nimg = (n0 > 0 && c.n1 > 0 && c.n2 > 0) ? n0 * c.n1 * c.n2 : 0;
    c.cutoff = cut[level];
    return c;
}

// candidate `cand` = image * n + j of site i: distance, and (optionally) what the edge stores
__device__ __forceinline__ float candidate(const Box& c, const float* __restrict__ cart, int base, int n, const float ci[3],
                                           int cand, int& j, int im[3], float r[3]) {
#pragma clang fp contract(off)
    const int image = cand / n;
    j = cand - image * n;
    const int q = c.n1 * c.n2;
    int i0 = image / q;
    int rem = image - i0 * q;
    int i1 = rem / c.n2;
    int i2 = rem - i1 * c.n2;
    i0 += c.lo0, i1 += c.lo1, i2 += c.lo2;
    im[0] = i0, im[1] = i1, im[2] = i2;
    float d[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float shift = ((float)i0 * c.lat[k] + (float)i1 * c.lat[3 + k]) + (float)i2 * c.lat[6 + k];
        const float x = shift + cart[3 * (size_t)(base + j) + k];
        r[k] = x - ci[k];
        d[k] = ci[k] - x;
    }
    return __fsqrt_rn((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]);
}

__device__ __forceinline__ int count_site(const Box& c, const float* __restrict__ cart, int base, int n, int i, float atol,
                                          int lane) {
    const float ci[3] = {cart[3 * (size_t)i], cart[3 * (size_t)i + 1], cart[3 * (size_t)i + 2]};
    const int64_t total = (int64_t)n * c.nimg;
    int cnt = 0;
    for (int64_t cand = lane; cand < total; cand += ALIGNN_WAVE) {
        int j, im[3];
        float r[3];
        const float d = candidate(c, cart, base, n, ci, (int)cand, j, im, r);
        cnt += (d <= c.cutoff && !(d <= atol)) ? 1 : 0;
    }
    return wave_sum(cnt);
}

// ---- pass 1: the crystal's level = the first cutoff of the ladder at which its LAST site has a neighbour
__global__ __launch_bounds__(ALIGNN_WAVE) void radius_level_kernel(const float* __restrict__ lat, const float* __restrict__ cart,
                                                                   const int32_t* __restrict__ graph_ptr,
                                                                   const int32_t* __restrict__ box, const float* __restrict__ cut,
                                                                   float atol, int L, int32_t* __restrict__ crystal_level) {
    const int b = blockIdx.x, lane = threadIdx.x;
    const int base = graph_ptr[b], n = graph_ptr[b + 1] - base;
    int level = 0;
    if (n > 0) {
        for (; level < L; ++level) {
            const Box c = load_box(lat, box, cut, b, L, level);
            if (count_site(c, cart, base, n, base + n - 1, atol, lane) > 0) break;
        }
    }
    if (lane == 0) crystal_level[b] = level;  // (== L: not found on the ladder - the host raises)
}

// ---- pass 2 / 3: count, then emit, the bonds of every site at its crystal's level
template <bool EMIT>
__global__ __launch_bounds__(kThreads) void radius_bonds_kernel(const float* __restrict__ lat, const float* __restrict__ cart,
                                                                const int32_t* __restrict__ graph_ptr,
                                                                const int32_t* __restrict__ site_graph,
                                                                const int32_t* __restrict__ box, const float* __restrict__ cut,
                                                                float atol, int L, int N, const int32_t* __restrict__ crystal_level,
                                                                int64_t* __restrict__ count, const int64_t* __restrict__ offset,
                                                                int64_t* __restrict__ u, int64_t* __restrict__ v,
                                                                float* __restrict__ rvec, int32_t* __restrict__ image) {
    const int lane = threadIdx.x & 63;
    const int i = blockIdx.x * kSitesPerBlock + (threadIdx.x >> 6);
    if (i >= N) return;
    const int b = site_graph[i], base = graph_ptr[b], n = graph_ptr[b + 1] - base;
    int level = crystal_level[b];
    if (level >= L) level = L - 1;  // (the host has raised already; stay in bounds)
    const Box c = load_box(lat, box, cut, b, L, level);
    if (!EMIT) {
        const int cnt = count_site(c, cart, base, n, i, atol, lane);
        if (lane == 0) count[i] = cnt;
        return;
    }
    const float ci[3] = {cart[3 * (size_t)i], cart[3 * (size_t)i + 1], cart[3 * (size_t)i + 2]};
    const int64_t total = (int64_t)n * c.nimg;
    int64_t out = offset[i];
    for (int64_t c0 = 0; c0 < total; c0 += ALIGNN_WAVE) {  // (uniform trip count: the ballot needs every lane)
        const int64_t cand = c0 + lane;
        int j = 0, im[3] = {0, 0, 0};
        float r[3] = {0.f, 0.f, 0.f};
        bool keep = false;
        if (cand < total) {
            const float d = candidate(c, cart, base, n, ci, (int)cand, j, im, r);
            keep = d <= c.cutoff && !(d <= atol);
        }
        const unsigned long long mask = __ballot(keep);
        if (keep) {
            const int64_t e = out + __popcll(mask & ((1ull << lane) - 1ull));
            u[e] = i;
            v[e] = base + j;
            rvec[3 * e] = r[0], rvec[3 * e + 1] = r[1], rvec[3 * e + 2] = r[2];
            if (image != nullptr) image[3 * e] = im[0], image[3 * e + 1] = im[1], image[3 * e + 2] = im[2];
        }
        out += __popcll(mask);
    }
}

}  // namespace

extern "C" {

int alignn_radius_levels(const float* lat, const float* cart, const int32_t* graph_ptr, const int32_t* box, const float* cut,
                         float atol, int levels, int n_crystals, int32_t* crystal_level, alignn_stream_t stream) {
    if (n_crystals <= 0) return 0;
    if (!lat || !cart || !graph_ptr || !box || !cut || !crystal_level || levels <= 0) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(radius_level_kernel, dim3(n_crystals), dim3(ALIGNN_WAVE), 0, (hipStream_t)stream, lat, cart, graph_ptr, box,
                       cut, atol, levels, crystal_level);
    ALIGNN_CHECK_LAUNCH();
    return 0;
}

int alignn_radius_count(const float* lat, const float* cart, const int32_t* graph_ptr, const int32_t* site_graph,
                        const int32_t* box, const float* cut, float atol, int levels, int64_t n_sites,
                        const int32_t* crystal_level, int64_t* count, alignn_stream_t stream) {
    if (n_sites <= 0) return 0;
    if (!lat || !cart || !graph_ptr || !site_graph || !box || !cut || !crystal_level || !count || levels <= 0)
        return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(radius_bonds_kernel<false>, dim3(alignn_ceil_div(n_sites, kSitesPerBlock)), dim3(kThreads), 0,
                       (hipStream_t)stream, lat, cart, graph_ptr, site_graph, box, cut, atol, levels, (int)n_sites, crystal_level,
                       count, (const int64_t*)nullptr, (int64_t*)nullptr, (int64_t*)nullptr, (float*)nullptr, (int32_t*)nullptr);
    ALIGNN_CHECK_LAUNCH();
    return 0;
}

int alignn_radius_emit(const float* lat, const float* cart, const int32_t* graph_ptr, const int32_t* site_graph,
                       const int32_t* box, const float* cut, float atol, int levels, int64_t n_sites,
                       const int32_t* crystal_level, const int64_t* offset, int64_t* u, int64_t* v, float* r, int32_t* image,
                       alignn_stream_t stream) {
    if (n_sites <= 0) return 0;
    if (!lat || !cart || !graph_ptr || !site_graph || !box || !cut || !crystal_level || !offset || !u || !v || !r || levels <= 0)
        return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(radius_bonds_kernel<true>, dim3(alignn_ceil_div(n_sites, kSitesPerBlock)), dim3(kThreads), 0,
                       (hipStream_t)stream, lat, cart, graph_ptr, site_graph, box, cut, atol, levels, (int)n_sites, crystal_level,
                       (int64_t*)nullptr, offset, u, v, r, image);
    ALIGNN_CHECK_LAUNCH();
    return 0;
}

}  // extern "C"
