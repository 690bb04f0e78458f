// Shared device helpers for the gfx950 kernels (wave = 64 lanes, fp32 rows of H features).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#define ALIGNN_WAVE 64
#define ALIGNN_EPS_GATE 1e-6f

#define ALIGNN_CHECK_LAUNCH()                      \
    do {                                           \
        hipError_t e__ = hipGetLastError();        \
        if (e__ != hipSuccess) return (int)e__;    \
    } while (0)

static inline int alignn_ceil_div(int64_t a, int64_t b) { return (int)((a + b - 1) / b); }

// ---- host-side launch predicates and grid sizes ----
static inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }  // float4 accesses
// feature counts of the row kernels: whole float4 quads, at most four 256-feature chunks per wavefront
static inline bool feat_ok(int F) { return F >= 4 && (F & 3) == 0 && F <= 1024; }
// a [rows, cols] fp32 tensor that cannot stay in the 256 MiB last-level cache anyway: its kernels take the streaming
// (read-once / write-once hint) variant
static inline bool exceeds_llc(int64_t rows, int64_t cols) { return rows * cols * 4 >= (int64_t)128 << 20; }
// arena offsets: every buffer starts on a 256-byte boundary
static inline size_t al256(size_t b) { return (b + 255) / 256 * 256; }
// workgroups for n items at per_block each: at least one (it writes the zero slab of an empty launch), at most cap
static inline int capped_blocks(int64_t n, int per_block, int cap) {
    const int64_t b = (n + per_block - 1) / per_block;
    return (int)(b < 1 ? 1 : b > cap ? cap : b);
}
// ops.FOLD_ABOVE: more reduction slabs than this are pre-summed to alignn_slab_fold_slabs() before a finaliser reads them
constexpr int kFoldAbove = 1024;
// per-device tables of events (the stream forks of composite.hip and model.hip) have this many entries
constexpr int kMaxDevices = 32;
// run-time feature count F (feat_ok) -> compile-time number NC of 256-feature chunks a lane walks, 1..4:
// f(std::integral_constant<int, NC>) launches the kernel instantiated for it
template <class Fn>
static inline void with_feature_chunks(int F, Fn&& f) {
    switch ((F + 255) / 256) {
        case 1: f(std::integral_constant<int, 1>{}); break;
        case 2: f(std::integral_constant<int, 2>{}); break;
        case 3: f(std::integral_constant<int, 3>{}); break;
        default: f(std::integral_constant<int, 4>{}); break;
    }
}

// sigmoid with the hardware reciprocal (v_rcp_f32, 1 ulp) instead of an IEEE division (v_div_scale x2, v_rcp, four fma,
// v_div_fmas, v_div_fixup: ten instructions per element, 40 % of the line-graph backward kernel's VALU work); the exponential
// is __expf (2 ulp) already.  Every kernel - forward, recomputation in backward, the oracle comparison - goes through this
// one function.
__device__ __forceinline__ float fast_sigmoid(float x) { return __builtin_amdgcn_rcpf(1.0f + __expf(-x)); }

// flat element index i -> (row, quad) of a [rows, Q quads] matrix.  Q is a run-time value, so `i / Q` on a 64-bit index
// is a ~100-instruction emulated division PER ELEMENT in kernels that otherwise do a handful of FMAs; feature counts are
// powers of two almost everywhere (256, 64, 1024): shift and mask then, 32-bit division when the index fits, the general
// case last.  (Wave-uniform branches.)
struct RowQuad {
    int Q, shift;  // shift = log2(Q) when Q is a power of two, else -1
    __device__ __forceinline__ explicit RowQuad(int q) : Q(q), shift((q & (q - 1)) == 0 ? __ffs(q) - 1 : -1) {}
    __device__ __forceinline__ void split(int64_t i, int64_t total, int64_t& r, int& q) const {
        if (shift >= 0) {
            r = i >> shift;
            q = (int)(i & (Q - 1));
        } else if (total < ((int64_t)1 << 31)) {
            const unsigned ri = (unsigned)i / (unsigned)Q;
            r = ri;
            q = (int)((unsigned)i - ri * (unsigned)Q);
        } else {
            r = i / Q;
            q = (int)(i - r * Q);
        }
    }
};

__device__ __forceinline__ float4 f4_ld(const float* p) { return *reinterpret_cast<const float4*>(p); }
__device__ __forceinline__ void f4_st(float* p, float4 v) { *reinterpret_cast<float4*>(p) = v; }
// streaming (read-once / write-once) variants: nontemporal hint, measured +9 % on a 2-read 1-write pass over 2 GB
typedef float alignn_v4f __attribute__((ext_vector_type(4)));
template <bool STREAM>
__device__ __forceinline__ float4 f4_lds(const float* p) {
    if (!STREAM) return *reinterpret_cast<const float4*>(p);
    alignn_v4f v = __builtin_nontemporal_load(reinterpret_cast<const alignn_v4f*>(p));
    return make_float4(v.x, v.y, v.z, v.w);
}
template <bool STREAM>
__device__ __forceinline__ void f4_sts(float* p, float4 r) {
    if (!STREAM) {
        *reinterpret_cast<float4*>(p) = r;
        return;
    }
    alignn_v4f v = {r.x, r.y, r.z, r.w};
    __builtin_nontemporal_store(v, reinterpret_cast<alignn_v4f*>(p));
}
__device__ __forceinline__ float4 f4_zero() { return make_float4(0.f, 0.f, 0.f, 0.f); }
__device__ __forceinline__ float4 f4_add(float4 a, float4 b) {
    return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w);
}
__device__ __forceinline__ float4 f4_sub(float4 a, float4 b) {
    return make_float4(a.x - b.x, a.y - b.y, a.z - b.z, a.w - b.w);
}
__device__ __forceinline__ float4 f4_scale(float4 a, float s) { return make_float4(a.x * s, a.y * s, a.z * s, a.w * s); }
__device__ __forceinline__ float4 f4_mul(float4 a, float4 b) {
    return make_float4(a.x * b.x, a.y * b.y, a.z * b.z, a.w * b.w);
}
__device__ __forceinline__ float4 f4_fma(float4 a, float4 b, float4 c) {
    return make_float4(fmaf(a.x, b.x, c.x), fmaf(a.y, b.y, c.y), fmaf(a.z, b.z, c.z), fmaf(a.w, b.w, c.w));
}
__device__ __forceinline__ float4 f4_sigmoid(float4 a) {
    return make_float4(fast_sigmoid(a.x), fast_sigmoid(a.y), fast_sigmoid(a.z), fast_sigmoid(a.w));
}

// silu(z) = z*s, silu'(z) = s*(1 + z*(1-s)) with s = sigmoid(z)
__device__ __forceinline__ float silu_f(float z) { return z * fast_sigmoid(z); }
__device__ __forceinline__ float dsilu_f(float z) {
    float s = fast_sigmoid(z);
    return s * (1.0f + z * (1.0f - s));
}

__device__ __forceinline__ float hsum4(float4 a) { return (a.x + a.y) + (a.z + a.w); }
// silu'(z), silu''(z)
__device__ __forceinline__ void dsilu2(float z, float& d1, float& d2) {
    const float s = fast_sigmoid(z), sp = s * (1.0f - s);
    d1 = s + z * sp;
    d2 = sp * (2.0f + z * (1.0f - 2.0f * s));
}

// ---- sums over the 64 lanes of a wavefront, the result in every lane ----
// xor butterfly (6 ds_bpermute round trips): fixed order, every lane ends with the same bits
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = ALIGNN_WAVE / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, ALIGNN_WAVE);
    return v;
}
__device__ __forceinline__ int wave_sum(int v) {
#pragma unroll
    for (int o = ALIGNN_WAVE / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, ALIGNN_WAVE);
    return v;
}
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int o = ALIGNN_WAVE / 2; o > 0; o >>= 1) v = v + __shfl_xor(v, o, ALIGNN_WAVE);
    return v;
}
__device__ __forceinline__ double wave_max(double v) {
#pragma unroll
    for (int o = ALIGNN_WAVE / 2; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, ALIGNN_WAVE));
    return v;
}
__device__ __forceinline__ double wave_min(double v) {
#pragma unroll
    for (int o = ALIGNN_WAVE / 2; o > 0; o >>= 1) v = fmin(v, __shfl_xor(v, o, ALIGNN_WAVE));
    return v;
}
// The same float sum by another instruction sequence, so another summation order and a name of its own.  Within a row of 16
// lanes by DPP adds (xor 1, xor 2, mirror of 8, mirror of 16: every lane of the row ends with the row's sum), the four rows by
// v_readlane - 4 DPP adds + 4 readlanes + 3 adds instead of the 6 ds_bpermute round trips of the butterfly (the LayerNorm-in-gate
// passes of convln.hip take 2-7 such sums per row).  Fixed order: ((r0 + r1) + (r2 + r3)) over the row sums.
template <int CTRL>
__device__ __forceinline__ float dpp_mov(float v) {
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xF, 0xF, true));
}
__device__ __forceinline__ float wave_sum_dpp(float v) {
    v += dpp_mov<0xB1>(v);   // quad_perm [1, 0, 3, 2]
    v += dpp_mov<0x4E>(v);   // quad_perm [2, 3, 0, 1]
    v += dpp_mov<0x141>(v);  // row_half_mirror
    v += dpp_mov<0x140>(v);  // row_mirror
    const int b = __builtin_bit_cast(int, v);
    const float r0 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(b, 0)), r1 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(b, 16));
    const float r2 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(b, 32)), r3 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(b, 48));
    return (r0 + r1) + (r2 + r3);
}

// Merge of two BatchNorm "pivot slabs" (norm.hip: col_stats_welford_kernel; conv.hip writes the same slabs and
// bn_finalize_welford reads both): (n, p, S, SS) of set a  <-  union with set b, expressed about a's pivot; empty sets pass through
__device__ __forceinline__ void pivot_merge(float& na, float4& pa, float4& Sa, float4& SSa, float nb, float4 pb, float4 Sb,
                                            float4 SSb) {
    if (nb == 0.0f) return;
    if (na == 0.0f) {
        na = nb, pa = pb, Sa = Sb, SSa = SSb;
        return;
    }
    const float4 d = f4_sub(pb, pa);
    // sum (x - pa)^2 over b = SSb + 2 d Sb + nb d^2 ;  sum (x - pa) over b = Sb + nb d
    SSa = make_float4(SSa.x + SSb.x + d.x * (2.0f * Sb.x + nb * d.x), SSa.y + SSb.y + d.y * (2.0f * Sb.y + nb * d.y),
                      SSa.z + SSb.z + d.z * (2.0f * Sb.z + nb * d.z), SSa.w + SSb.w + d.w * (2.0f * Sb.w + nb * d.w));
    Sa = make_float4(Sa.x + Sb.x + nb * d.x, Sa.y + Sb.y + nb * d.y, Sa.z + Sb.z + nb * d.z, Sa.w + Sb.w + nb * d.w);
    na += nb;
}

// Running max|x| of a tensor, tracked by the kernel that produces it (consumed by the f16x3 GEMMs to pick their
// power-of-two operand scale).  Wave max by DPP-free shuffles, then ONE atomicMax per workgroup on the bit pattern:
// non-negative floats order like unsigned ints and max is order independent, so the result is deterministic.
// Every thread of the workgroup must call it (it contains a barrier); `amax` may be null.
__device__ __forceinline__ void block_amax_commit(float m, float* amax) {
    if (amax == nullptr) return;  // uniform
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) m = fmaxf(m, __shfl_xor(m, off));
    __shared__ float amax_sh[16];
    const int wave = threadIdx.x >> 6, nw = (blockDim.x * blockDim.y + 63) >> 6;
    if ((threadIdx.x & 63) == 0) amax_sh[wave] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        float r = amax_sh[0];
        for (int w = 1; w < nw; ++w) r = fmaxf(r, amax_sh[w]);
        // most workgroups find the running maximum already above their own: look before paying for the atomic (a
        // stale read only costs a redundant atomicMax)
        if (r > 0.0f && r > *reinterpret_cast<volatile float*>(amax))
            atomicMax(reinterpret_cast<unsigned*>(amax), __float_as_uint(r));
    }
    __syncthreads();  // the scratch array may be reused by a second commit
}
__device__ __forceinline__ float f4_absmax(float4 v) { return fmaxf(fmaxf(fabsf(v.x), fabsf(v.y)), fmaxf(fabsf(v.z), fabsf(v.w))); }

// ---- float64 helpers of the per-structure integrators (relax.hip, dynamics.hip): one workgroup of WAVES waves per structure ----

// sums over the workgroup of NV values per thread (the last one a max when LAST_MAX); every thread returns the same bits.
// Fixed order (shuffle-down within a wave, then the wave partials in wave order): no float atomics, so a structure's result
// does not depend on which other structures share the launch.  Every thread of the workgroup must call it (barriers).
template <int NV, bool LAST_MAX, int WAVES>
__device__ __forceinline__ void block_reduce(double (&v)[NV], double (*sh)[WAVES]) {
    const int lane = threadIdx.x & (ALIGNN_WAVE - 1), wave = threadIdx.x / ALIGNN_WAVE;
#pragma unroll
    for (int j = 0; j < NV; ++j) {
        const bool mx = LAST_MAX && j == NV - 1;
#pragma unroll
        for (int o = ALIGNN_WAVE / 2; o > 0; o >>= 1) {
            const double u = __shfl_down(v[j], o, ALIGNN_WAVE);
            v[j] = mx ? fmax(v[j], u) : v[j] + u;
        }
        if (lane == 0) sh[j][wave] = v[j];
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < NV; ++j) {
        const bool mx = LAST_MAX && j == NV - 1;
        double s = sh[j][0];
#pragma unroll
        for (int w = 1; w < WAVES; ++w) s = mx ? fmax(s, sh[j][w]) : s + sh[j][w];
        v[j] = s;
    }
    __syncthreads();  // (sh is reused by the next reduction)
}

// fractional coordinate wrapped into [0, 1)
__device__ __forceinline__ double wrap01(double f) {
    f -= floor(f);
    return f < 1.0 ? f : 0.0;  // (-tiny - floor(-tiny) rounds to 1.0)
}

// row-major 3 x 3: c = a b
__device__ __forceinline__ void mm3(const double* a, const double* b, double* c) {
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) c[3 * i + j] = a[3 * i] * b[j] + a[3 * i + 1] * b[3 + j] + a[3 * i + 2] * b[6 + j];
}

// det of a row-major 3 x 3 matrix, along its first row
__device__ __forceinline__ double det3(const double* a) {
    return a[0] * (a[4] * a[8] - a[5] * a[7]) - a[1] * (a[3] * a[8] - a[5] * a[6]) + a[2] * (a[3] * a[7] - a[4] * a[6]);
}

// det and inverse of a row-major 3 x 3 matrix by cofactors
__device__ __forceinline__ double inverse3(const double (&a)[9], double (&inv)[9]) {
    const double c00 = a[4] * a[8] - a[5] * a[7], c01 = a[3] * a[8] - a[5] * a[6], c02 = a[3] * a[7] - a[4] * a[6];
    const double det = a[0] * c00 - a[1] * c01 + a[2] * c02;
    inv[0] = c00 / det;
    inv[1] = (a[2] * a[7] - a[1] * a[8]) / det;
    inv[2] = (a[1] * a[5] - a[2] * a[4]) / det;
    inv[3] = -c01 / det;
    inv[4] = (a[0] * a[8] - a[2] * a[6]) / det;
    inv[5] = (a[2] * a[3] - a[0] * a[5]) / det;
    inv[6] = c02 / det;
    inv[7] = (a[1] * a[6] - a[0] * a[7]) / det;
    inv[8] = (a[0] * a[4] - a[1] * a[3]) / det;
    return det;
}
