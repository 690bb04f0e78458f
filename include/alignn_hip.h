/*
 * alignn_hip.h - C ABI of libalignn_hip.so: the MI355X (gfx950) kernels behind the
 * ALIGNN message-passing hot path.
 *
 * Drop-in boundary.  The reference (usnistgov/alignn) is pure Python; the "FFI" it has for this
 * path is the set of torch / DGL calls its model files make.  Each entry point below names the
 * reference call site(s) it replaces (paths relative to the reference root).  A maintainer binds
 * them with ctypes; nothing torch-specific crosses this boundary.
 *
 * Conventions
 *   - all pointers are DEVICE pointers into buffers owned by the caller (PyTorch's caching
 *     allocator in our host code); the library never allocates, frees or synchronises;
 *   - every call only enqueues work on `stream` (graph-capture safe) and returns a hipError_t
 *     as int (0 == hipSuccess); argument errors return hipErrorInvalidValue (1);
 *   - matrices are row-major fp32; `ld*` are leading dimensions in ELEMENTS;
 *   - graph structure is "canonical CSR": the m edges of a graph are stored so that the in-edges
 *     of one destination node are contiguous ("segment").  Segment s covers edge rows
 *     [seg_ptr[s], seg_ptr[s+1]) and belongs to node seg_node[s] (seg_node == NULL: node s).
 *     Edge-feature row k IS CSR slot k.  `src[k]` is the source node of slot k.  The by-source
 *     view (needed by backward) is out_ptr[n+1] / out_slot[m] (slots grouped by source node) and
 *     `dst[k]`, the destination node of slot k.  Indices are int32;
 *   - reductions are atomics-free and run in a fixed order: results are bit-reproducible from
 *     run to run (the reference trains with torch.use_deterministic_algorithms(True),
 *     alignn/train.py:164-179).
 */
#ifndef ALIGNN_HIP_H
#define ALIGNN_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* alignn_stream_t; /* hipStream_t */

/* Library / build identification: returns a static string such as "alignn_hip 0.2 gfx950". */
const char* alignn_version(void);

/* ------------------------------------------------------------------------------------------
 * Dense projections (fp32 in / fp32 accumulate on v_mfma_f32_32x32x2_f32; exact fp32).
 * Replace torch.nn.Linear forward/backward at alignn/models/alignn.py:98-99,101,104,110
 * (src_gate, dst_gate, edge_gate, dst_update, src_update), :175-177 (MLPLayer) and :341 (fc).
 * ------------------------------------------------------------------------------------------ */

/* C[M,N] = A[M,K] * W[N,K]^T (+ bias[N]) (+ addend[M,N])      -- nn.Linear forward.
 * No alignment is required of any operand: what is not 16-byte aligned (or a K, lda, ldw that is no multiple of 4) takes an
 * element-wise kernel - a `bias` that is not 16-byte aligned included, whatever the other operands are. */
int alignn_gemm_nt(const float* A, int64_t lda, const float* W, int64_t ldw, const float* bias,
                   const float* addend, int64_t ldadd, float* C, int64_t ldc,
                   int64_t M, int N, int K, alignn_stream_t stream);

/* C[M,K] = G[M,N] * W[N,K] (+ addend[M,K])                    -- nn.Linear input gradient */
int alignn_gemm_nn(const float* G, int64_t ldg, const float* W, int64_t ldw,
                   const float* addend, int64_t ldadd, float* C, int64_t ldc,
                   int64_t M, int N, int K, alignn_stream_t stream);
/* The same product with the reduction split into slabs when there are few output tiles and a long reduction (the input
 * gradient of the fused node projection on atom rows: [n, 4H] x [4H, H]): `_workspace` returns the bytes of slab storage the
 * shape wants, 0 when alignn_gemm_nn is the right call.  Slabs are added in a fixed order (bit-reproducible). */
size_t alignn_gemm_nn_split_workspace(int64_t M, int N, int K);
int alignn_gemm_nn_split(const float* G, int64_t ldg, const float* W, int64_t ldw, const float* addend, int64_t ldadd,
                         float* C, int64_t ldc, int64_t M, int N, int K, void* workspace, size_t workspace_bytes,
                         alignn_stream_t stream);

/* dW[N,K] = G[M,N]^T * A[M,K]                                  -- nn.Linear weight gradient.
 * Split over M in `splits` deterministic slabs; `workspace` holds splits*N*K floats
 * (alignn_gemm_tn_workspace tells how many bytes for a given shape). */
size_t alignn_gemm_tn_workspace(int64_t M, int N, int K);
/* g_amax / a_amax (both or neither; may be NULL): device scalars holding max|G| and max|A| (upper bounds are
 * fine) - when both are given and the shape suits the split-product kernel, the three-product fp16 scheme runs
 * instead of the six-product bf16 one (see alignn_gemm_nt_f16x3). */
int alignn_gemm_tn(const float* G, int64_t ldg, const float* g_amax, const float* A, int64_t lda,
                   const float* a_amax, float* dW, int64_t lddw, int64_t M, int N, int K, void* workspace,
                   size_t workspace_bytes, alignn_stream_t stream);

/* fp32-accurate projection on the bf16 matrix cores ("bf16x6", csrc/gemm_x6.hip): every fp32 value is cut
 * into three truncated bf16 slices and the six slice products of weight >= 2^-16 are accumulated in fp32
 * (error <= an fp32 FMA chain; 2.7x the fp32-MFMA rate, which makes the HxH projections HBM-bound).
 *   alignn_split_bf16x3: slices W[N,K] (transpose != 0: the [N,K] matrix W^T of a stored [K,N] W) into the
 *                        kernel's DMA image (three bf16 planes, k-blocked, rows padded to 256, XOR-swizzled);
 *                        `out` holds alignn_split_bf16x3_bytes(N, K) bytes; K % 16 == 0.  Run once per
 *                        weight per step (384 KiB for 256x256).
 *   alignn_gemm_nt_x6:   C[M,N] = A[M,K] * W[N,K]^T (+bias) (+addend), W given pre-sliced;
 *                        needs K % 16 == 0, N >= 128, N % 4 == 0 (alignn_gemm_nt_x6_supported). */
size_t alignn_split_bf16x3_bytes(int N, int K);
int alignn_split_bf16x3(const float* W, int64_t ldw, int N, int K, int transpose, void* out,
                        alignn_stream_t stream);
int alignn_gemm_nt_x6_supported(int64_t M, int N, int K);
int alignn_gemm_nt_x6(const float* A, int64_t lda, const void* Wsplit, const float* bias,
                      const float* addend, int64_t ldadd, float* C, int64_t ldc,
                      int64_t M, int N, int K, alignn_stream_t stream);

/* Weight gradient on the split product (both operands sliced in registers): slab partials ws[z][N][K] for
 * z < alignn_gemm_tn_x6_splits(M,N,K); needs N % 256 == 0, K % 256 == 0, M >= 4096.  alignn_gemm_tn uses it
 * automatically for such shapes and sums the slabs.
 * Range of the maxima (f16x3, here and in alignn_gemm_tn): the accumulators are divided by the two operand scales.  Where
 * the product of the two inverse scales is an fp32 number - scales multiplying to less than 2^150, about
 * max|G| max|X| >= 2^-121 - it is applied as one factor; below, where that product is 0 in fp32, the two inverse scales
 * are applied one after the other, so a weight gradient of ordinary fp32 size (max|G| = max|X| = 2^-62, 4096 rows: entries
 * around 1e-37) is returned as such and not as 0.  Results on every other input keep their bits. */
int alignn_gemm_tn_x6_supported(int64_t M, int N, int K);
size_t alignn_gemm_tn_x6_workspace(int64_t M, int N, int K);
int alignn_gemm_tn_x6_splits(int64_t M, int N, int K);
int alignn_gemm_tn_x6_partials(const float* G, int64_t ldg, const float* g_amax, const float* X, int64_t ldx,
                               const float* x_amax, int64_t M, int N, int K, void* workspace,
                               size_t workspace_bytes, alignn_stream_t stream);

/* Same projection with HALF the matrix-core work ("f16x3"), for callers that know max|A|: operands are scaled
 * by a power of two into the fp16 range and cut into two fp16 slices (11 + 11 mantissa bits); the three products
 * hh + hl + lh are accumulated in fp32 and the scales undone in the epilogue - fp32-grade error (dropped term
 * < 2^-22), sustained-MFMA time 153 us instead of 306 us for T x 256 x 256, i.e. the projection is HBM-bound.
 *   alignn_absmax:        amax[0] = max|X| (device scalar; the fused producers track it themselves - see the
 *                         `amax` argument of alignn_bn_silu_fwd, alignn_egc_bwd_dst, alignn_egc_bwd_lg_fused, ...)
 *   alignn_split_f16x2:   pre-slice W * 2^s (s from *w_amax) into the two-plane DMA image
 *   alignn_gemm_nt_f16x3: C = A W^T (+bias)(+addend); shapes as alignn_gemm_nt_x6_supported */
int alignn_absmax(const float* X, int64_t ldx, int64_t rows, int F, float* amax, alignn_stream_t stream);
size_t alignn_split_f16x2_bytes(int N, int K);
int alignn_split_f16x2(const float* W, int64_t ldw, int N, int K, int transpose, const float* w_amax, void* out,
                       alignn_stream_t stream);
/* The image of W and the image of W^T (N % 16 == 0 as well) in ONE launch: what alignn_split_f16x2(transpose=0) and
 * alignn_split_f16x2(transpose=1) produce, bit for bit.  The forward products (alignn/models/alignn.py:98-110 nn.Linear)
 * and torch.autograd's input gradients of the same Linear use the two images of one optimizer step. */
int alignn_split_f16x2_both(const float* W, int64_t ldw, int N, int K, const float* w_amax, void* out, void* out_t,
                            alignn_stream_t stream);
/* max|W| + both images of EVERY split-product weight of a model in three stream operations (once per optimizer step; the
 * per-weight calls above cost two launches each, ~28 weights): `descs` = n_weights device records {const float* W;
 * int64_t ldw; int32_t N, K; float* amax; void* out; void* out_t} (48 bytes), `amax_slots` = the n_weights floats the
 * records' `amax` fields point into (zeroed here first); N, K multiples of 16, ldw of 4. */
int alignn_prepare_weights(const void* descs, int n_weights, float* amax_slots, alignn_stream_t stream);
/* *amax = max(*amax, max|X|): alignn_absmax (below) without its reset, for a slot known to hold 0 */
int alignn_absmax_raise(const float* X, int64_t ldx, int64_t rows, int F, float* amax, alignn_stream_t stream);
/* alignn_gemm_nt_f16x3 and its variants below (_bnred, _gather, _gather2, _stats):
 * - Leading dimensions.  Long products without an addend (K >= 80, N % 256 == 0, at least 1024 tiles of 128 x 256) run on a
 *   persistent kernel that addresses C, the addend and Xn with 32-bit offsets inside a row tile: it refuses (invalid value)
 *   ldc, ldadd or ldxn >= 2^20.  Every other shape takes any multiple of 4.  A caller that wants one answer for every
 *   row count keeps all three below 2^20.
 * - Slabs.  `stats_partial` / `red_partial` hold alignn_gemm_nt_x6_row_tiles(M, N, K) + 1 slabs of [2][N] floats.  Slab t
 *   (t < row_tiles) receives the sums over rows [t R, min((t + 1) R, M)), R = 64 or 128 being the unit
 *   alignn_gemm_nt_x6_row_tiles counts with (row_tiles = ceil(M / R)): 64 wherever the persistent kernel's shape test holds,
 *   with or without an addend; otherwise the block tile of the one-tile kernel, 64 rows for K <= 64 or fewer than 256
 *   tiles of 128 x 256, else 128 (ALIGNN_AMD_X6_PERSIST=0 switches the shape test off for the count and the launch alike).
 *   Every one of these slabs is written by every call.  The slab behind them is scratch: the persistent kernel parks the
 *   sums of a wave strip that lies past row M there (zeros), the one-tile kernels leave it alone.  Nothing behind it is
 *   touched.
 * - Small maxima.  The operand scale is 2^(141 - e) for a maximum in [2^(e-127), 2^(e-126)), clamped to 2^127: a tensor
 *   whose maximum is below 2^-113 is scaled to less than 2^14, and what the slices resolve - 2^-25 absolute after scaling,
 *   2^-39 of the maximum at full scale - coarsens by a factor of two per factor of two below 2^-113 (max|A| = 2^-120:
 *   2^-32 of the maximum, still below fp32's 2^-24).  Maxima down to 2^-113 are scaled in full.
 *   The inverse scale of a clamped operand is the fp32 subnormal 2^-127; the library is built with fp32 denormals kept,
 *   and the two inverse scales are applied one after the other, so nothing underflows that the result itself does not. */
int alignn_gemm_nt_f16x3(const float* A, int64_t lda, const float* a_amax, const void* Wsplit,
                         const float* w_amax, const float* bias, const float* addend, int64_t ldadd, float* C,
                         int64_t ldc, int64_t M, int N, int K, alignn_stream_t stream);

/* The same projection when its OUTPUT is the gradient g_y of y = r + silu(BatchNorm(Xn)) (the next thing autograd does
 * with g_y is BatchNorm's backward: alignn/models/alignn.py:126 bn_edges / :178 MLPLayer's BatchNorm1d under
 * torch.autograd): additionally writes, per row tile of the product, the column sums over the tile's rows of
 *   gz = g_y * silu'((Xn - mean) * scale + beta)   and   gz * (Xn - mean) * rstd
 * into red_partial [row_tiles + 1][2][N] (the last slab is scratch for the kernel, never summed; nstat = [4][N] as
 * written by alignn_bn_finalize; a "row tile" is the 64 / 128-row unit alignn_gemm_nt_x6_row_tiles counts for the shape
 * - the block tile of the one-tile kernels, the 64-row wave strip of the persistent one).  alignn_bn_bwd_finalize
 * over `alignn_gemm_nt_x6_row_tiles(M, N, K)` slabs then gives dbeta / dgamma - what alignn_bn_silu_bwd_reduce
 * computes with two more passes over g_y and Xn. */
/* The edge-gate projection of EdgeGatedGraphConv with DGL's u_add_v folded in (alignn/models/alignn.py:98-101:
 * m = src_gate(x)[u] + dst_gate(x)[v] + edge_gate(y)):  C[e] = A[e] W^T + bias + P[src[e]][0:N] + P[dst[e]][N:2N],
 * P = the fused node projection [n, ldp] = A | Bd | Bh | Ux.  alignn_egc_gate_fwd_pre is the gate pass that takes such
 * an M (already m: it neither gathers A / Bd nor stores m) - same values, one write and one gather of a T-row
 * tensor less than alignn_gemm_nt_f16x3 + alignn_egc_gate_fwd. */
int alignn_gemm_nt_f16x3_gather(const float* A, int64_t lda, const float* a_amax, const void* Wsplit,
                                const float* w_amax, const float* bias, float* C, int64_t ldc, int64_t M, int N, int K,
                                const float* P, int64_t ldp, const int32_t* src, const int32_t* dst,
                                float* stats_partial, alignn_stream_t stream);
/* The same with the second gathered row from its own table: C[e] = A[e] W^T + bias + P[src[e]][0:N] + Bd2[rank[e]][0:N].
 * For a line graph: Bd2 = the Bd block of P with its rows in SEGMENT order (alignn_gather_rows_ld by seg_node), rank[e] =
 * the segment of edge row e - consecutive rows then read consecutive table rows instead of one random row per segment.
 * Only P's first N columns are read here: ldp >= N and ldbd2 >= N (alignn_gemm_nt_f16x3_gather: ldp >= 2 N). */
int alignn_gemm_nt_f16x3_gather2(const float* A, int64_t lda, const float* a_amax, const void* Wsplit, const float* w_amax,
                                 const float* bias, float* C, int64_t ldc, int64_t M, int N, int K, const float* P, int64_t ldp,
                                 const int32_t* src, const float* Bd2, int64_t ldbd2, const int32_t* rank,
                                 float* stats_partial, alignn_stream_t stream);
/* out[r][0:F] = in[perm[r]][0:F] for matrices with leading dimensions (F, ld_in, ld_out multiples of 4) */
int alignn_gather_rows_ld(const float* in, int64_t ld_in, const int32_t* perm, float* out, int64_t ld_out, int64_t rows, int F,
                          alignn_stream_t stream);
/* stats_partial (above: may be NULL) / alignn_gemm_nt_f16x3_stats: the projection also leaves, per row tile, the column
 * sums of its output and of its square - [alignn_gemm_nt_x6_row_tiles + 1][2][N] (last slab: scratch), the slab layout
 * alignn_bn_finalize takes -
 * i.e. the BatchNorm statistics torch's BatchNorm1d would compute with another pass over the tensor
 * (alignn/models/alignn.py:122-127 bn_edges, :175-179 MLPLayer).  alignn_egc_gate_fwd_pre_norm is the gate pass for an M
 * that already holds m AND whose statistics are known: it writes Y' = Y + silu((m - mean) scale + beta) itself (e_stat as
 * from alignn_bn_finalize; Y may be NULL), so the edge branch needs no separate normalise / activate pass. */
int alignn_gemm_nt_f16x3_stats(const float* A, int64_t lda, const float* a_amax, const void* Wsplit,
                               const float* w_amax, const float* bias, float* C, int64_t ldc, int64_t M, int N, int K,
                               float* stats_partial, alignn_stream_t stream);
int alignn_egc_gate_fwd_pre_norm(const float* P, const float* M, const int32_t* seg_ptr, const int32_t* seg_node,
                                 const int32_t* src, int64_t n_seg, int64_t m_rows, int H, float* XPRE, float* S0,
                                 float* HH, float* n_partial, const float* e_stat, const float* Y, float* YOUT,
                                 float* y_amax, alignn_stream_t stream);
int alignn_egc_gate_fwd_pre(const float* P, float* M, const int32_t* seg_ptr, const int32_t* seg_node,
                            const int32_t* src, int64_t n_seg, int64_t m_rows, int H, float* XPRE, float* S0, float* HH,
                            float* e_partial, float* n_partial, alignn_stream_t stream);
int alignn_gemm_nt_x6_row_tiles(int64_t M, int N, int K);
int alignn_gemm_nt_f16x3_bnred(const float* A, int64_t lda, const float* a_amax, const void* Wsplit,
                               const float* w_amax, const float* bias, const float* addend, int64_t ldadd,
                               float* C, int64_t ldc, int64_t M, int N, int K, const float* Xn, int64_t ldxn,
                               const float* nstat, float* red_partial, alignn_stream_t stream);

/* Input gradient AND weight gradient of a 256 -> 256 projection in one pass over the projection's output gradient G
 * (csrc/gemm_dw.hip; replaces the pair alignn_gemm_nt_f16x3[_bnred] + alignn_gemm_tn, which each streamed G from HBM):
 *     C[M,256]    = G[M,256] W[256,256] (+ addend)      autograd's grad_input of nn.Linear, alignn/models/alignn.py:101 (edge_gate)
 *     dW[256,256] = G[M,256]^T Y[M,256]                 ... and its grad_weight; Y = the Linear's input
 * f16x3 split products as alignn_gemm_nt_f16x3 (same bits for C): `Wt_split` = alignn_split_f16x2(W, transpose = 1) with its
 * max|W| scalar, g_amax / y_amax = device scalars >= max|G|, max|Y|.  Optional, as alignn_gemm_nt_f16x3_bnred: Xn / nstat /
 * red_partial - the BatchNorm-backward column sums of C against the pre-activation Xn, left as
 * alignn_gemm_dgrad_wgrad_slabs(M) * 2 slabs of [2][256] for alignn_bn_bwd_finalize.  `workspace`:
 * alignn_gemm_dgrad_wgrad_workspace(M) bytes (one 256 x 256 partial of dW per workgroup, summed in fp64 in slab order:
 * bit-reproducible).  Shapes: N = K = 256, M >= 4096 (alignn_gemm_dgrad_wgrad_supported).
 * - Leading dimensions.  ldg, ldy, ldc, lddw - and ldadd, ldxn where their pointer is given - are multiples of 4 in
 *   [256, 2^20): rows must not overlap, and the kernel addresses the rows of a 64-row tile with 32-bit offsets (as the
 *   persistent kernel of alignn_gemm_nt_f16x3).  Anything else is refused (invalid value) before any launch.
 * - Range of the maxima.  C: as alignn_gemm_nt_f16x3.  dW: as alignn_gemm_tn_x6_partials - the two inverse scales are one
 *   factor where their product is an fp32 number and are applied one after the other where it is not (scales multiplying to
 *   2^150 or more, about g_amax y_amax < 2^-121), so dW is not flushed to 0 there.
 * - Rows past M.  The last tile re-reads row M - 1 of G, addend and Xn for its missing rows and multiplies those of Y by 0
 *   (an infinity in row M - 1 of Y therefore gives NaN in its column of dW); no row behind the M given is read.
 * - Extents.  Exactly alignn_gemm_dgrad_wgrad_slabs(M) slabs of `workspace` and twice as many of `red_partial` are written. */
int alignn_gemm_dgrad_wgrad_supported(int64_t M, int N, int K);
int alignn_gemm_dgrad_wgrad_slabs(int64_t M);
size_t alignn_gemm_dgrad_wgrad_workspace(int64_t M);
int alignn_gemm_dgrad_wgrad_f16x3(const float* G, int64_t ldg, const float* g_amax, const float* Y, int64_t ldy,
                                  const float* y_amax, const void* Wt_split, const float* w_amax, const float* addend,
                                  int64_t ldadd, float* C, int64_t ldc, const float* Xn, int64_t ldxn, const float* nstat,
                                  float* red_partial, float* dW, int64_t lddw, int64_t M, void* workspace,
                                  size_t workspace_bytes, alignn_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Column statistics / BatchNorm1d + SiLU (+ residual).
 * Replace nn.BatchNorm1d (training: batch statistics over ALL rows; eps 1e-5; momentum 0.1,
 * unbiased running_var) + F.silu at alignn/models/alignn.py:122-127 and :175-179.
 * ------------------------------------------------------------------------------------------ */

/* number of partial slabs alignn_col_stats writes for `rows` rows (each slab = 2*F floats) */
int alignn_col_stats_slabs(int64_t rows);
/* partial[s][0][f] = sum_r X[r,f], partial[s][1][f] = sum_r X[r,f]^2 over slab s's rows */
int alignn_col_stats(const float* X, int64_t ldx, int64_t rows, int F, float* partial,
                     alignn_stream_t stream);
/* The same statistics as PIVOT SLABS - well-conditioned when |mean| >> std, where sum x^2 - (sum x)^2 / n cancels and a
 * float32 mean cannot even hold the sub-ulp part: partial[s][0][f] = a pivot p (the first value slab s saw in column f),
 * partial[s][1][f] = sum (x - p), partial[s][2][f] = sum (x - p)^2 over the slab's rows, followed by counts[s] (float) at
 * partial + slabs*3*F; partial holds slabs*(3*F+1) floats.  Threads / waves / slabs are merged by re-centring onto one
 * pivot (float64 in alignn_bn_finalize_welford; same outputs as alignn_bn_finalize).  The gate passes
 * (alignn_egc_gate_fwd, _pre, _pre_norm) write their e_partial / n_partial in THIS layout (slabs =
 * alignn_egc_slabs(n_seg)); the projection epilogues (alignn_gemm_nt_f16x3_stats / _gather) keep plain sum /
 * sum-of-squares slabs for alignn_bn_finalize. */
int alignn_col_stats_welford(const float* X, int64_t ldx, int64_t rows, int F, float* partial, alignn_stream_t stream);
int alignn_bn_finalize_welford(const float* partial, int slabs, int64_t rows, int F, const float* gamma, const float* beta,
                               float eps, float momentum, float* running_mean, float* running_var, float* stat,
                               alignn_stream_t stream);
/* column sums only: out[f] = sum_r X[r,f] (bias gradients); workspace = slabs*2*F floats */
int alignn_col_sum(const float* X, int64_t ldx, int64_t rows, int F, float* out, float* workspace,
                   alignn_stream_t stream);

/* Finalise: from `slabs` partial slabs over `rows` rows produce, per feature,
 *   stat[0]=mean, stat[1]=rstd, stat[2]=scale=gamma*rstd, stat[3]=beta   (stat is [4][F])
 * and (if running_mean != NULL) update running_mean/var in place with `momentum`.
 * slabs == 0: evaluation mode - take mean/var from running_mean/running_var.
 * rows == 0 (an empty batch, here and in alignn_bn_finalize_welford): the evaluation form too - stat comes from the running
 * statistics, which are required then and stay unchanged (no 0 / 0 reaches them). */
int alignn_bn_finalize(const float* partial, int slabs, int64_t rows, int F, const float* gamma,
                       const float* beta, float eps, float momentum, float* running_mean,
                       float* running_var, float* stat, alignn_stream_t stream);

/* Y[r,f] = (R ? R[r,f] : 0) + silu((X[r,f]-mean[f])*scale[f] + beta[f])
 * amax (here and below; may be NULL): device scalar the kernel raises to max|output| with one atomicMax per
 * workgroup - the caller zeroes it first; several kernels writing parts of one tensor may share it.  It is what
 * alignn_gemm_nt_f16x3 / alignn_gemm_tn need to run the next projection at half the matrix-core work. */
int alignn_bn_silu_fwd(const float* X, int64_t ldx, const float* R, int64_t ldr, const float* stat,
                       float* Y, int64_t ldy, int64_t rows, int F, float* amax, alignn_stream_t stream);

/* backward, phase 1: partial[s][0][f] = sum_r gz, partial[s][1][f] = sum_r gz*xhat, where
 * z = (X-mean)*scale+beta, gz = GY * silu'(z), xhat = (X-mean)*rstd   (rows == 0: the one slab is written as zeros) */
int alignn_bn_silu_bwd_reduce(const float* GY, int64_t ldgy, const float* X, int64_t ldx,
                              const float* stat, int64_t rows, int F, float* partial,
                              alignn_stream_t stream);
/* phase 1b: red[0][f]=sum gz (=dbeta), red[1][f]=sum gz*xhat (=dgamma) from the slabs */
int alignn_bn_bwd_finalize(const float* partial, int slabs, int F, float* red, alignn_stream_t stream);
/* LayerNorm flavour (ALIGNNAtomWise: alignn/models/alignn_atomwise.py:151,155; MLPLayer of
 * alignn/models/utils.py:277-292): per-ROW statistics over the F features, eps, affine gamma/beta.
 *   fwd: Y = (R ? R : 0) + silu(LayerNorm(X)); stats[r] = (mean, rstd) (may be NULL for inference)
 *   bwd: GX = LayerNorm/SiLU backward of GY; partial[alignn_ln_slabs(rows)][2][F] = slabs of
 *        (sum gz, sum gz*xhat) = (dbeta, dgamma), finished with alignn_bn_bwd_finalize. */
int alignn_ln_slabs(int64_t rows);
int alignn_ln_silu_fwd(const float* X, int64_t ldx, const float* R, int64_t ldr, const float* gamma,
                       const float* beta, float eps, float* Y, int64_t ldy, float* stats, int64_t rows, int F,
                       float* amax, alignn_stream_t stream);
int alignn_ln_silu_bwd(const float* GY, int64_t ldgy, const float* X, int64_t ldx, const float* gamma,
                       const float* beta, const float* stats, float* GX, int64_t ldgx, float* partial,
                       int64_t rows, int F, float* amax, alignn_stream_t stream);
/* alignn_ln_silu_bwd on the node pre-activations xpre = Ux + S1 / (S0 + eps) of an edge-gated convolution, the adjoints of the two
 * segment sums written in the same pass (alignn_egc_node_bwd's arithmetic on the gradient just formed: GS1 = g / (S0 + eps),
 * GS0 = -GS1 * HH) - one launch instead of two on the reverse chain of every LayerNorm-flavoured convolution. */
int alignn_ln_silu_bwd_node(const float* GY, int64_t ldgy, const float* X, int64_t ldx, const float* gamma, const float* beta,
                            const float* stats, float* GX, int64_t ldgx, float* partial, int64_t rows, int F, float* amax,
                            const float* S0, const float* HH, float* GS1, float* GS0, alignn_stream_t stream);
/* out[f] = sum_s partial[s][f] over `slabs` slabs of `width` floats (fp64 accumulation, fixed order) */
int alignn_slab_sum(const float* partial, int slabs, int width, float* out, alignn_stream_t stream);
/* Pre-pass for very many slabs (one per row tile of a T-row projection): out[g][f] = sum of partial[k][f] over
 * k = g, g + G, ... with G = alignn_slab_fold_slabs() (64); out is [G][width].  Same fixed order every time. */
int alignn_slab_fold_slabs(void);
int alignn_slab_fold(const float* partial, int slabs, int width, float* out, alignn_stream_t stream);
/* phase 2: GX = gamma*rstd*(gz - red0/rows - xhat*red1/rows)   (training-mode BatchNorm backward)
 * eval_mode != 0: GX = gz*scale (running statistics are constants) */
int alignn_bn_silu_bwd_apply(const float* GY, int64_t ldgy, const float* X, int64_t ldx,
                             const float* stat, const float* gamma, const float* red, int eval_mode,
                             float* GX, int64_t ldgx, int64_t rows, int F, float* amax,
                             alignn_stream_t stream);
/* ... for the NODE norm of a convolution (GX = gradient of x_pre = Ux + S1 / (S0 + 1e-6), alignn/models/alignn.py:110-111,
 * 122-123): the quotient's adjoints GS1 = GX / (S0 + 1e-6), GS0 = -GS1 * HH in the same pass - alignn_bn_silu_bwd_apply
 * followed by alignn_egc_node_bwd, same bits, one launch.  S0, HH, GS1, GS0: [rows, F] contiguous. */
int alignn_bn_silu_bwd_apply_node(const float* GY, int64_t ldgy, const float* X, int64_t ldx, const float* stat,
                                  const float* gamma, const float* red, int eval_mode, float* GX, int64_t ldgx,
                                  int64_t rows, int F, float* amax, const float* S0, const float* HH, float* GS1, float* GS0,
                                  alignn_stream_t stream);
/* ... and, in the same pass, the column sums of GX - the bias gradient of the nn.Linear in front of the BatchNorm
 * (MLPLayer, alignn/models/alignn.py:170-184) - as [alignn_col_stats_slabs(rows)][F] slabs for alignn_slab_sum
 * (rows == 0: the one slab is written as zeros). */
int alignn_bn_silu_bwd_apply_sum(const float* GY, int64_t ldgy, const float* X, int64_t ldx, const float* stat,
                                 const float* red, int eval_mode, float* GX, int64_t ldgx, int64_t rows, int F,
                                 float* amax, float* partial, alignn_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Edge-gated graph convolution core (gather -> gate -> segment-sum), one wavefront per
 * destination segment.  Replaces, in EdgeGatedGraphConv.forward (alignn/models/alignn.py:78-129):
 *   g.apply_edges(fn.u_add_v("e_src","e_dst","e_nodes"))            :100   (DGL g-SDDMM)
 *   m = e_nodes + edge_gate(edge_feats); sigma = sigmoid(m)           :101-103
 *   g.update_all(fn.u_mul_e("Bh","sigma","m"), fn.sum(...))           :105-107 (DGL g-SpMM)
 *   g.update_all(fn.copy_e("sigma","m"), fn.sum("m","sum_sigma"))     :108
 *   h = sum_sigma_h / (sum_sigma + 1e-6); x = src_update(x) + h       :109-110
 * and DGL's autograd of those calls (backward).
 *
 * P is the fused node projection [n, 4H] = [A | Bd | Bh | Ux] = x * [W_sg;W_dg;W_du;W_su]^T + b.
 * ------------------------------------------------------------------------------------------ */

/* number of stat slabs the gate kernel writes for a graph with n segments (pivot-slab layout: slabs*(3*H+1) floats, see
 * alignn_col_stats_welford).  Extents: e_partial and n_partial of alignn_egc_gate_fwd / _pre / _pre_norm are written in full and
 * hold exactly alignn_egc_slabs(n_seg) * (3 * H + 1) floats each - no slab behind them is scratch, unlike the projection
 * epilogues' [row_tiles + 1][2][N]; gb_partial of the reverse passes exactly [slabs][H] (tests/test_gpu_conv_bn.py hands
 * every one of them at that size inside guard bands). */
int alignn_egc_slabs(int64_t n_seg);

/* In : P[n,4H]; M[m,H] holds C = y*W_eg^T + b on entry.
 * Out: M[m,H] = m_pre = A[src] + Bd[dst] + C (in place); XPRE[n,H] = Ux + S1/(S0+1e-6);
 *      S0[n,H], HH[n,H] = S1/(S0+1e-6) (saved for backward; may be NULL for inference);
 *      e_partial: Welford column-stat slabs of m_pre; n_partial: of XPRE (each may be NULL; alignn_bn_finalize_welford).
 * m_rows = number of edge rows of M (only decides whether M is streamed with read-once/write-once hints). */
int alignn_egc_gate_fwd(const float* P, float* M, const int32_t* seg_ptr, const int32_t* seg_node,
                        const int32_t* src, int64_t n_seg, int64_t m_rows, int H, float* XPRE,
                        float* S0, float* HH, float* e_partial, float* n_partial,
                        alignn_stream_t stream);

/* Inference form of the same pass (no backward, edge normalisation = the fixed affine map of BatchNorm in eval
 * mode, e_stat = [mean, rstd, scale, shift] from the running statistics): C is only read, m_pre is never written,
 * and the edge output YOUT = (Y ? Y : 0) + silu((m_pre - mean) * scale + shift) comes straight out of the gate pass
 * (YOUT == NULL: the edge output is dead; y_amax, optional: raised to max|YOUT|).  XPRE as above. */
int alignn_egc_gate_infer(const float* P, const float* C, const int32_t* seg_ptr, const int32_t* seg_node,
                          const int32_t* src, int64_t n_seg, int64_t m_rows, int H, float* XPRE,
                          const float* e_stat, const float* Y, float* YOUT, float* y_amax,
                          alignn_stream_t stream);

/* Node-side backward glue: from g_xpre (BatchNorm-backward output on nodes) produce
 * GS1 = g_xpre/(S0+eps), GS0 = -g_xpre*HH/(S0+eps).  GXPRE has leading dimension ldg (it usually
 * lives in the Ux block of the [n,4H] projection gradient). */
int alignn_egc_node_bwd(const float* GXPRE, int64_t ldg, const float* S0, const float* HH, float* GS1, float* GS0,
                        int64_t n_nodes, int H, alignn_stream_t stream);

/* Destination-ordered backward pass.  Per slot e (dst i, src u):
 *   g_mbn = BatchNorm/SiLU backward of the edge branch (skipped when GY == NULL: dead edge output;
 *           when e_stat == NULL, GY is taken to BE g_mbn already - the LayerNorm flavour computes it
 *           with alignn_ln_silu_bwd)
 *   sigma = sigmoid(M[e]);  g_sigma = GS1[i]*Bh[u] + GS0[i]
 *   GM[e] = g_mbn + g_sigma*sigma*(1-sigma);   GP[i, H:2H] (g_Bd) = sum_e GM[e]
 * GP is the [n,4H] gradient of the fused node projection; this pass fills its Bd block.
 * gb_partial (optional): [alignn_egc_slabs(n_seg)][H] column-sum slabs of GM (the edge_gate bias gradient,
 * finished with alignn_slab_sum) - saves a separate pass over GM.
 * gm_amax / gp_amax (optional): raised to max|GM| and max|the GP entries written here| (see alignn_bn_silu_fwd). */
int alignn_egc_bwd_dst(const float* GY, const float* M, const float* P, const float* GS1,
                       const float* GS0, const float* e_stat, const float* e_gamma,
                       const float* e_red, int e_eval, int64_t m_rows,
                       const int32_t* seg_ptr, const int32_t* seg_node, const int32_t* src,
                       int64_t n_seg, int H, float* GM, float* GP, float* gb_partial,
                       float* gm_amax, float* gp_amax, alignn_stream_t stream);

/* Line-graph backward with the destination- and source-ordered passes fused (one workgroup per centre atom j;
 * L(g)'s edges form one dense block per atom: sources = in-edges of j = L(g) nodes [grp_src_ptr[j],
 * grp_src_ptr[j+1]), segments = out-edges of j = segment ranks [grp_seg_ptr[j], grp_seg_ptr[j+1])).  Same inputs,
 * outputs and bit-identical results as alignn_egc_bwd_dst followed by alignn_egc_bwd_src, with 2 reads + 1 write
 * per edge row instead of 4 + 1.  gb_partial: [n_groups][H] column-sum slabs of GM. */
int alignn_egc_bwd_lg_fused(const float* GY, const float* M, const float* P, const float* GS1,
                            const float* GS0, const float* e_stat, const float* e_red, int e_eval,
                            int64_t m_rows, const int32_t* grp_seg_ptr, const int32_t* grp_src_ptr,
                            int64_t n_groups, const int32_t* seg_ptr, const int32_t* seg_node,
                            const int32_t* dst, const int32_t* out_ptr, const int32_t* out_slot, int H,
                            float* GM, float* GP, float* gb_partial, float* gm_amax, float* gp_amax,
                            alignn_stream_t stream);

/* The same backward for line graphs whose blocks are DENSE and source-sorted (every segment of atom j lists all
 * in-edges of j in ascending order, minus itself for a self-image bond - true for DGL's g.line_graph() after
 * alignn_amd.graph's canonicalisation and for graphs built by graph.line_graph_of; max_group_src = the largest
 * in-degree, > 0 - atoms with more than 16 in-edges take extra passes of 16 sources).  Rows are addressed by index arithmetic, the block is walked segment by segment, every T-row of
 * GY and M is read once and GM written once (the by-source kernel above re-reads GM: 3.6 row passes of fetch vs 2).
 * Same outputs; sums in a different but fixed order. */
int alignn_egc_bwd_lg_dense_supported(int max_group_src);
int alignn_egc_bwd_lg_dense(const float* GY, const float* M, const float* P, const float* GS1,
                            const float* GS0, const float* e_stat, const float* e_red, int e_eval,
                            int64_t m_rows, const int32_t* grp_seg_ptr, const int32_t* grp_src_ptr,
                            int64_t n_groups, int max_group_src, const int32_t* seg_ptr,
                            const int32_t* seg_node, int H, float* GM, float* GP, float* gb_partial,
                            float* gm_amax, float* gp_amax, alignn_stream_t stream);

/* Source-ordered backward pass (deterministic scatter-by-source):
 *   GP[j, 0:H]   (g_A)  = sum_{e: src e = j} GM[e]
 *   GP[j, 2H:3H] (g_Bh) = sum_{e: src e = j} sigmoid(M[e]) * GS1[dst e] */
int alignn_egc_bwd_src(const float* GM, const float* M, const float* GS1, const int32_t* out_ptr,
                       const int32_t* out_slot, const int32_t* dst, int64_t n_nodes, int H,
                       float* GP, float* gp_amax, alignn_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Featurisation and readout.
 * ------------------------------------------------------------------------------------------ */

/* RBFExpansion.forward (alignn/models/utils.py:40-44): out[r,k] = exp(-gamma (d[r]-c[k])^2) */
int alignn_rbf_fwd(const float* d, const float* centers, float gamma, float* out, int64_t rows,
                   int bins, alignn_stream_t stream);
/* compute_bond_cosines on L(g) (alignn/graphs.py:847-864; re-run inside ALIGNNAtomWise.forward when
 * lg_on_fly, alignn_atomwise.py:424-431): h[k] = clamp(-r[e1[k]].r[e2[k]] / (|r[e1]| |r[e2]|), -1, 1) */
int alignn_bond_cosine_fwd(const float* r, const int32_t* e1, const int32_t* e2, float* h, int64_t T,
                           alignn_stream_t stream);
/* torch.norm(r, dim=1) (alignn/models/alignn.py:313): out[r] = ||v[r,0:3]|| */
int alignn_norm3_fwd(const float* v, float* out, int64_t rows, alignn_stream_t stream);
/* First derivatives of the three featurisation steps w.r.t. the geometry - what torch autograd does for the
 * reference when ALIGNNAtomWise takes forces = -dE/dr (alignn_atomwise.py:512-539):
 *   rbf:    gd[r] = sum_k G[r,k] * d/dd exp(-gamma (d[r]-c[k])^2)
 *   norm3:  gv[r,:] = g[r] * v[r,:]/|v[r]|
 *   cosine: per triplet k, ga[k,:] = gh[k] dh/dr[e1[k]], gb[k,:] = gh[k] dh/dr[e2[k]] (zero where the clamp is
 *           active); the caller segment-sums ga by source and gb by destination of L(g) (alignn_segment_sum). */
int alignn_rbf_bwd(const float* d, const float* centers, float gamma, const float* G, float* gd, int64_t rows,
                   int bins, alignn_stream_t stream);
int alignn_norm3_bwd(const float* v, const float* g, float* gv, int64_t rows, alignn_stream_t stream);
int alignn_bond_cosine_bwd(const float* r, const int32_t* e1, const int32_t* e2, const float* gh, float* ga,
                           float* gb, int64_t T, alignn_stream_t stream);
/* dgl.nn.AvgPooling (alignn/models/alignn.py:325): out[b] = mean_{i in graph b} x[i]; graph_ptr[B+1] */
int alignn_segment_mean_fwd(const float* X, const int32_t* graph_ptr, float* out, int B, int H,
                            alignn_stream_t stream);
/* its backward: GX[i] = G[b(i)] / count[b(i)] */
int alignn_segment_mean_bwd(const float* G, const int32_t* graph_ptr, float* GX, int B, int H,
                            alignn_stream_t stream);
/* Generic segment sum (any width F): out[node ? node[s] : s, :] = sum_{k in [ptr[s], ptr[s+1])}
 * vals[slot ? slot[k] : k, :].  With alignn_gather_rows it forms the adjoint pair (gather by index <-> sum by
 * group) from which the twice-differentiable force path is composed: DGL copy_e/sum on g and on dgl.reverse(g)
 * (alignn/models/alignn_atomwise.py:547-565) and every gather/scatter of the conv when create_graph=True. */
int alignn_segment_sum(const float* vals, int64_t ldv, const int32_t* ptr, const int32_t* slot,
                       const int32_t* node, float* out, int64_t ldo, int64_t n_seg, int F,
                       alignn_stream_t stream);
/* row permutation: out[k] = in[perm[k]] (canonical reordering of edge features) */
int alignn_gather_rows(const float* in, const int32_t* perm, float* out, int64_t rows, int F,
                       alignn_stream_t stream);

/* alignn_ln_silu_dual_bwd on the node pre-activations of an edge-gated convolution + alignn_egc_node_dual_bwd in the same pass */
int alignn_ln_silu_dual_bwd_node(const float* GY, const float* GYt, int64_t ldg, const float* X, const float* Xt, int64_t ldx,
                                 const float* gamma, const float* beta, const float* stats, float* GX, float* GXt, int64_t ldo,
                                 float* partial, int64_t rows, int F, float* amax2, const float* s0, const float* hh,
                                 const float* s0t, const float* hht, float* q1, float* q0, float* q1t, float* q0t,
                                 alignn_stream_t stream);
/* ------------------------------------------------------------------------------------------
 * Dual-number kernels (value + directional derivative along a bond-vector displacement) of the LayerNorm-flavoured
 * stack - training THROUGH the forces: the reference takes pair forces with autograd.grad(create_graph=True)
 * (alignn/models/alignn_atomwise.py:512-565) and differentiates the force / stress loss through them
 * (alignn/train.py:387).  sum_e w_e . f_e = -D_w E_tot, so the loss gradient is the reverse pass of a forward pass
 * that carries tangents; these are its non-linear pieces (csrc/dual.hip), "t" = tangent, amax2 = two device scalars
 * (value, tangent) raised like `amax` elsewhere.  Slab counts: alignn_dual_slabs(rows).
 *   ln_silu_dual_fwd:  Y = R + silu(LN(X)), Yt = Rt + d[silu o LN](X).Xt;  stats[rows][2] = mean, rstd
 *   ln_silu_dual_bwd:  (GY, GYt) -> (GX, GXt); partial[slabs][2][F] = dbeta | dgamma partial sums
 *   egc_gate_dual_fwd: DGL u_add_v + sigmoid + u_mul_e/sum + copy_e/sum + h = S1/(S0+eps) (alignn_atomwise.py:177-189)
 *                      on duals; M / Mt hold C / Ct on entry and m / mt on exit
 *   egc_node_dual_bwd, egc_dual_bwd_dst, egc_dual_bwd_src: its reverse (adjoints Q of the four segment sums; GM / GMt;
 *                      the A | Bd | Bh blocks of GP / GPt; gb_partial[slabs][H] = column sums of GM) */
int alignn_dual_slabs(int64_t rows);
int alignn_ln_silu_dual_fwd(const float* X, const float* Xt, int64_t ldx, const float* R, const float* Rt, int64_t ldr,
                            const float* gamma, const float* beta, float eps, float* Y, float* Yt, int64_t ldy,
                            float* stats, int64_t rows, int F, float* amax2, alignn_stream_t stream);
int alignn_ln_silu_dual_bwd(const float* GY, const float* GYt, int64_t ldg, const float* X, const float* Xt, int64_t ldx,
                            const float* gamma, const float* beta, const float* stats, float* GX, float* GXt,
                            int64_t ldo, float* partial, int64_t rows, int F, float* amax2, alignn_stream_t stream);
int alignn_egc_gate_dual_fwd(const float* P, const float* Pt, float* M, float* Mt, const int32_t* seg_ptr,
                             const int32_t* seg_node, const int32_t* src, int64_t n, int64_t m, int H, float* xpre,
                             float* xpre_t, float* s0, float* hh, float* s0t, float* hht, alignn_stream_t stream);
/* the tangent half of alignn_egc_gate_dual_fwd alone, for a caller that already holds the values (M = m, s0, hh from the force
 * evaluation): Mt holds Ct on entry and mt on exit; writes xpre_t, s0t, hht.  alignn_ln_silu_dual_fwd likewise takes Y == NULL
 * (value output not written, R not read). */
int alignn_egc_gate_dual_fwd_tangent(const float* P, const float* Pt, const float* M, float* Mt, const int32_t* seg_ptr,
                                     const int32_t* seg_node, const int32_t* src, int64_t n, int64_t m, int H, float* xpre_t,
                                     const float* s0, const float* hh, float* s0t, float* hht, alignn_stream_t stream);
int alignn_egc_node_dual_bwd(const float* g, const float* gt, int64_t ldg, const float* s0, const float* hh,
                             const float* s0t, const float* hht, float* q1, float* q0, float* q1t, float* q0t, int64_t n,
                             int H, alignn_stream_t stream);
int alignn_egc_dual_bwd_dst(const float* GL, const float* GLt, const float* M, const float* Mt, const float* P,
                            const float* Pt, const float* q1, const float* q0, const float* q1t, const float* q0t,
                            const int32_t* seg_ptr, const int32_t* seg_node, const int32_t* src, int64_t n, int H,
                            float* GM, float* GMt, float* GP, float* GPt, float* gb_partial, float* gm_amax2,
                            float* gp_amax2, alignn_stream_t stream);
int alignn_egc_dual_bwd_src(const float* GM, const float* GMt, const float* M, const float* Mt, const float* q1,
                            const float* q1t, const int32_t* out_ptr, const int32_t* out_slot, const int32_t* dst,
                            int64_t n, int H, float* GP, float* GPt, float* gp_amax2, alignn_stream_t stream);
/* egc_dual_bwd_dst + egc_dual_bwd_src as ONE pass for line graphs with dense, source-sorted blocks (see
 * alignn_egc_bwd_lg_dense: one workgroup per centre atom, rows by index arithmetic): M, Mt, GL, GLt read once, GM, GMt
 * written once - 6 T-row passes instead of 10; same outputs, sums in a different but fixed order; gb_partial
 * [n_groups][H].  m_rows (the rows of M) is not used to index anything: it only chooses between the cached loads and
 * stores and the streaming ones, taken when a [m_rows, H] fp32 tensor reaches 128 MiB, i.e. m_rows >= (128 << 20) / (4 H).
 * A caller may therefore pass such a value with a small graph to run the streaming instantiations (the tests do). */
int alignn_egc_dual_bwd_lg_dense(const float* GL, const float* GLt, const float* M, const float* Mt, const float* P,
                                 const float* Pt, const float* q1, const float* q0, const float* q1t, const float* q0t,
                                 int64_t m_rows, const int32_t* grp_seg_ptr, const int32_t* grp_src_ptr, int64_t n_groups,
                                 const int32_t* seg_ptr, const int32_t* seg_node, int H, float* GM, float* GMt, float* GP,
                                 float* GPt, float* gb_partial, float* gm_amax2, float* gp_amax2, alignn_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Line-graph convolutions of the LayerNorm flavour with the edge LayerNorm inside the gate passes (csrc/convln.hip).
 * Reference: EdgeGatedGraphConv.forward with nn.LayerNorm, alignn/models/alignn_atomwise.py:151-208 (:199-206 the two
 * normalised branches), and its autograd / double backward for the reverse passes.  A wavefront of the gate passes holds a
 * whole H <= 256 row of m, so the row statistics are wave reductions and y' = y + silu(LN(m)) (forward) resp. the LayerNorm /
 * SiLU adjoint of g_y' (reverse) cost no pass of their own.  Same formulas and summation orders as the separate kernels
 * (alignn_ln_silu_fwd / _bwd, alignn_ln_silu_dual_fwd / _bwd + the gate passes); LayerNorm parameter gradients leave as
 * ln_partial [n_groups][2][H] (dbeta | dgamma per workgroup; alignn_bn_bwd_finalize sums the slabs in order).
 * e_stat [m][2] = (mean, rstd) per row, written by the forward, read by everything else.
 * alignn_egc_ln_fused_supported(H, m_rows): 1 when they are the ones to take (H % 4 == 0, H <= 256, edge tensors of >= 64 MiB:
 * on cache-resident line graphs the separate kernels' finer grids win; ALIGNN_AMD_LN_FUSED = 0 never, 2 whenever H allows). */
int alignn_egc_ln_fused_supported(int H, int64_t m_rows);
/* alignn_egc_gate_fwd_pre (M holds m = A[u] + Bd[v] + C) + alignn_ln_silu_fwd(M, residual Y or NULL) -> YOUT, e_stat, y_amax */
int alignn_egc_gate_fwd_pre_ln(const float* P, const float* M, const int32_t* seg_ptr, const int32_t* seg_node, const int32_t* src,
                               int64_t n_seg, int64_t m_rows, int H, float* XPRE, float* S0, float* HH, const float* gamma,
                               const float* beta, float eps, const float* Y, float* YOUT, float* e_stat, float* y_amax,
                               alignn_stream_t stream);
/* alignn_ln_silu_bwd(GY, M) + alignn_egc_bwd_lg_dense(MODE 2): GY is the adjoint of the edge OUTPUT (before the LayerNorm) */
int alignn_egc_bwd_lg_dense_ln(const float* GY, const float* M, const float* P, const float* GS1, const float* GS0,
                               const float* gamma, const float* beta, const float* e_stat, int64_t m_rows,
                               const int32_t* grp_seg_ptr, const int32_t* grp_src_ptr, int64_t n_groups, int max_group_src,
                               const int32_t* seg_ptr, const int32_t* seg_node, int H, float* GM, float* GP, float* gb_partial,
                               float* ln_partial, float* gm_amax, float* gp_amax, alignn_stream_t stream);
/* The same for graphs without dense blocks (the bond graph g): the destination-ordered reverse halves with the LayerNorm adjoint
 * of the edge output formed in the pass - alignn_ln_silu_bwd + alignn_egc_bwd_dst(e_stat = NULL), resp. alignn_ln_silu_dual_bwd +
 * alignn_egc_dual_bwd_dst, as one launch; the source-ordered halves follow unchanged.  gb_partial [alignn_egc_ln_dst_slabs(n_seg)][H],
 * ln_partial [...][2][H].  alignn_egc_ln_dst_supported(H): H % 4 == 0, H <= 256, ALIGNN_AMD_LN_FUSED != 0 (any row count). */
int alignn_egc_ln_dst_slabs(int64_t n_seg);
int alignn_egc_ln_dst_supported(int H);
int alignn_egc_bwd_dst_ln(const float* GY, const float* M, const float* P, const float* GS1, const float* GS0, const float* gamma,
                          const float* beta, const float* e_stat, const int32_t* seg_ptr, const int32_t* seg_node,
                          const int32_t* src, int64_t n_seg, int H, float* GM, float* GP, float* gb_partial, float* ln_partial,
                          float* gm_amax, float* gp_amax, alignn_stream_t stream);
int alignn_egc_dual_bwd_dst_ln(const float* GY, const float* GYt, const float* M, const float* Mt, const float* P, const float* Pt,
                               const float* q1, const float* q0, const float* q1t, const float* q0t, const float* gamma,
                               const float* beta, const float* e_stat, const int32_t* seg_ptr, const int32_t* seg_node,
                               const int32_t* src, int64_t n_seg, int H, float* GM, float* GMt, float* GP, float* GPt,
                               float* gb_partial, float* ln_partial, float* gm_amax2, float* gp_amax2, alignn_stream_t stream);
/* alignn_egc_gate_dual_fwd_tangent + the tangent of y' = y + silu(LN(m)) (alignn_ln_silu_dual_fwd with Y == NULL): Mt holds Ct
 * on entry and mt on exit, Yt = Rt + d[silu o LN](m) . mt; amax2[1] is raised to max|Yt| */
int alignn_egc_gate_dual_tan_ln(const float* P, const float* Pt, const float* M, float* Mt, const int32_t* seg_ptr,
                                const int32_t* seg_node, const int32_t* src, int64_t n, int64_t m, int H, float* xpre_t,
                                const float* s0, const float* hh, float* s0t, float* hht, const float* gamma, const float* beta,
                                const float* e_stat, const float* Rt, float* Yt, float* amax2, alignn_stream_t stream);
/* alignn_ln_silu_dual_bwd(GY, GYt, M, Mt) + alignn_egc_dual_bwd_lg_dense: GY / GYt are the adjoints of the edge output's value
 * and tangent */
int alignn_egc_dual_bwd_lg_dense_ln(const float* GY, const float* GYt, const float* M, const float* Mt, const float* P,
                                    const float* Pt, const float* q1, const float* q0, const float* q1t, const float* q0t,
                                    const float* gamma, const float* beta, const float* e_stat, int64_t m_rows,
                                    const int32_t* grp_seg_ptr, const int32_t* grp_src_ptr, int64_t n_groups,
                                    const int32_t* seg_ptr, const int32_t* seg_node, int H, float* GM, float* GMt, float* GP,
                                    float* GPt, float* gb_partial, float* ln_partial, float* gm_amax2, float* gp_amax2,
                                    alignn_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Periodic k-nearest-neighbour bond lists on the device (csrc/knn.hip).
 * Replace alignn/graphs.py:155-264 (nearest_neighbor_edges on jarvis' get_all_neighbors, canonize_edge :128-153,
 * build_undirected_edgedata :230-264), which alignn/ff/calculators.py:280-291 re-runs at every MD step.
 * One wavefront per site; float64 distances evaluated in the reference's operation order (bit-exact tie decisions);
 * no atomics on the output, no host synchronisation.  Inputs shared by the four passes:
 *   lat[B][9] float64 (rows a, b, c), cart[N][3] float64 Cartesian positions (frac . lat, the caller's fixed-order
 *   product), graph_ptr[B+1] site offsets, site_graph[N] crystal of each site, cut[B][levels] the crystal's cutoff
 *   sequence (cutoff, then "longest lattice vector if below it, else twice", graphs.py:170-188), box[B][levels][6]
 *   the inclusive image range (lo[3], hi[3]) the crystal's sites scan.  Candidates are the pairs with
 *   0.15 (jarvis' bond_tol) < distance <= cutoff.
 *   knn_box:    box from frac[N][3] float64 and the lattice-only tables reach / maxr [B][levels][3] =
 *               ceil(cut / plane spacing) / ceil((cut + 0.15) / plane spacing): per axis [-reach, reach] when every
 *               fraction of the crystal lies in [0, 1], else jarvis' [floor(min) - maxr, ceil(max) + maxr - 1] (unwrapped
 *               input; not symmetric, and a bond is kept by an end only at an image that end scans).  A box too large for
 *               32-bit candidate indices is written empty (lo 0, hi -1): the crystal then ends on level == levels.
 *   knn_levels: crystal_level[B] (zeroed by the caller) = first level at which EVERY site of the crystal has >= k
 *               candidates (== levels: not reachable - the caller raises)
 *   knn_kth:    kth[N] = distance of the k-th nearest candidate (ties share it)
 *   knn_count:  count[N] = canonical bonds (a, b >= a, image) owned by site a: kept by a OR by b
 *   knn_emit:   offset[N] = exclusive prefix sum of count; writes both directions of bond e at rows 2e, 2e+1 of
 *               u, v (int64), r[.][3] float32 = src -> dst displacement, image[.][3] int32 (optional; forward image for
 *               both directions, like the reference's `images`); a site's bonds leave sorted by (b, image). */
int alignn_knn_box(const double* frac, const int32_t* graph_ptr, const int32_t* reach, const int32_t* maxr, int levels,
                   int64_t n_crystals, int32_t* box, alignn_stream_t stream);
/* distances inside the cutoff a site's wave keeps in LDS for the k-th smallest; above it knn_kth searches by rounds */
int alignn_knn_kth_cap(void);
int alignn_knn_levels(const double* lat, const double* cart, const int32_t* graph_ptr, const int32_t* site_graph,
                      const double* cut, const int32_t* box, int levels, int k, int64_t n_sites, int32_t* crystal_level,
                      alignn_stream_t stream);
int alignn_knn_kth(const double* lat, const double* cart, const int32_t* graph_ptr, const int32_t* site_graph,
                   const double* cut, const int32_t* box, int levels, int k, int64_t n_sites, const int32_t* crystal_level,
                   double* kth, alignn_stream_t stream);
int alignn_knn_count(const double* lat, const double* cart, const int32_t* graph_ptr, const int32_t* site_graph,
                     const double* cut, const int32_t* box, int levels, int64_t n_sites, const int32_t* crystal_level,
                     const double* kth, int64_t* count, alignn_stream_t stream);
int alignn_knn_emit(const double* lat, const double* cart, const int32_t* graph_ptr, const int32_t* site_graph,
                    const double* cut, const int32_t* box, int levels, int64_t n_sites, const int32_t* crystal_level,
                    const double* kth, const int64_t* offset, int64_t* u, int64_t* v, float* r, int32_t* image,
                    alignn_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Composite entry points (csrc/composite.hip): ONE call = one EdgeGatedGraphConv forward / backward, BatchNorm
 * flavour in training mode (alignn/models/alignn.py:78-129 and torch.autograd's backward of it).  They issue exactly
 * the launches the per-kernel entry points above would, in the same order with the same arguments (bit-identical
 * results), so that an eagerly launched training step costs ~3 host calls per convolution instead of ~30.
 * Every pointer is a device pointer owned by the caller; `scratch` is one block of alignn_egc_conv_*_scratch() bytes.
 * Shapes: x [n,Kin], y [m,Kin], P [n,4H], M [m,H], everything else [n,H] / [m,H] / [4,H] / [2,H] as named.
 *   node_kind  0: P by alignn_gemm_nt(wcat)            1: alignn_gemm_nt_f16x3(wcat_img, x_amax)
 *   edge_kind  0: alignn_gemm_nt(w_eg) + alignn_egc_gate_fwd + alignn_bn_silu_fwd
 *              1: alignn_gemm_nt_f16x3_gather(+statistics) + alignn_egc_gate_fwd_pre_norm
 *   y_out == NULL: dead edge output (statistics / running buffers still updated)
 *   gate_mode  0: alignn_egc_bwd_dst + _src   1: alignn_egc_bwd_lg_fused   2: alignn_egc_bwd_lg_dense
 *   dx_kind / dy_kind (input gradients g_x = GP wcat, g_y = GM w_eg):
 *              1: f16x3 on the W^T image (dy: + BatchNorm-backward sums of (src_xn, src_nstat) -> src_red)
 *              2: alignn_gemm_nn_split (dx only)   3: alignn_gemm_nn   4: alignn_gemm_nt on a transposed copy (wcat_t / weg_t)
 *              5: f16x3 on the W^T image, no sums (dy only)
 * ------------------------------------------------------------------------------------------ */
typedef struct alignn_egc_fwd_args {
    const int32_t *seg_ptr, *seg_node, *src, *dst;
    const int32_t* seg_rank; /* edge_kind 2: [m] segment of every edge row (the destination term is then read from a
                                segment-ordered copy of P's Bd block, alignn_gather_rows_ld + alignn_gemm_nt_f16x3_gather2) */
    int64_t n, m;
    int32_t H, Kin, node_kind, edge_kind, residual, pad_;
    float eps, momentum;
    const float *x, *y, *x_amax, *y_amax;
    const float *wcat, *bcat, *wcat_amax;
    const void* wcat_img;
    const float *w_eg, *b_eg, *weg_amax;
    const void* weg_img;
    const float *n_gamma, *n_beta, *e_gamma, *e_beta;
    float *n_rm, *n_rv, *e_rm, *e_rv;
    float *P, *M, *xpre, *s0, *hh, *n_stat, *e_stat, *x_out, *y_out, *x_out_amax, *y_out_amax;
    float* scratch;
    size_t scratch_bytes;
} alignn_egc_fwd_args;
/* bytes of `scratch`: the call touches nothing outside them (the edge-statistics block inside is sized as its writer's entry
 * above states: [row_tiles + 1][2][H] for edge_kind >= 1, alignn_egc_slabs(n) * (3 * H + 1) floats for edge_kind 0) */
size_t alignn_egc_conv_fwd_scratch(int64_t n, int64_t m, int H, int Kin, int edge_kind);
int alignn_egc_conv_fwd(const alignn_egc_fwd_args* args, alignn_stream_t stream);

typedef struct alignn_egc_bwd_args {
    const int32_t *seg_ptr, *seg_node, *src, *dst, *out_ptr, *out_slot, *grp_seg_ptr, *grp_src_ptr;
    int64_t n, m, n_groups;
    int32_t H, Kin, gate_mode, dense_max_src, dx_kind, dy_kind, residual, pad_;
    const float *gx_out, *gy_out;                                       /* incoming gradients (gy_out may be NULL) */
    const float *P, *M, *xpre, *s0, *hh, *n_stat, *e_stat, *n_gamma, *e_gamma; /* saved by the forward */
    const float* e_red_in;                                              /* pre-reduced sums of the edge norm, or NULL */
    const float *wcat, *wcat_t, *wcat_amax;
    const void* wcat_t_img;
    const float *w_eg, *weg_t, *weg_amax;
    const void* weg_t_img;
    const float *src_xn, *src_nstat;                                    /* dy_kind 1: the norm y came out of */
    int64_t src_ldxn;
    float *GP, *GM, *gs1, *gs0, *n_red, *e_red, *gb_part, *g_x, *g_y, *src_red, *gp_amax, *gm_amax;
    alignn_stream_t aux_stream; /* optional second stream: the node input gradient g_x = GP wcat runs there, beside
                                   g_y = GM w_eg on the caller's stream (fork after the gate backward, join before the call
                                   returns; needs alignn_fork_events_init() to have run on this device - otherwise, or with
                                   NULL, everything stays on the one stream).  Same kernels, same results. */
    float* scratch;
    size_t scratch_bytes;
} alignn_egc_bwd_args;
/* creates (once per device, for the CURRENT device) the two events the composite entry points fork / join with; call it
 * outside stream capture.  Returns 0, or the HIP error. */
int alignn_fork_events_init(void);
size_t alignn_egc_conv_bwd_scratch(int64_t n, int64_t m, int H, int Kin, int dx_kind, int dy_kind);
int alignn_egc_conv_bwd(const alignn_egc_bwd_args* args, alignn_stream_t stream);

/* the weight / bias gradients of the same convolution (the host code runs this one on its side stream):
 * g_beg = column sums of GM (from gb_part), g_weg = GM^T y, g_wcat = GP^T x, g_bcat = column sums of GP */
typedef struct alignn_egc_wgrad_args {
    int64_t n, m;
    int32_t H, Kin, gb_slabs, pad_;
    const float *GM, *GP, *x, *y, *gb_part, *gm_amax, *gp_amax, *x_amax, *y_amax;
    float *g_weg, *g_beg, *g_wcat, *g_bcat;
    float* scratch;
    size_t scratch_bytes;
} alignn_egc_wgrad_args;
size_t alignn_egc_conv_wgrad_scratch(int64_t n, int64_t m, int H, int Kin);
int alignn_egc_conv_wgrad(const alignn_egc_wgrad_args* args, alignn_stream_t stream);
/* sizeof the three argument structs (0: fwd, 1: bwd, 2: wgrad) - a binding checks its own packing against these */
size_t alignn_egc_args_sizeof(int which);

/* ------------------------------------------------------------------------------------------
 * Whole-model entry points (csrc/model.hip): ONE call = ALIGNN.forward in training mode
 * (alignn/models/alignn.py:282-349: RBF + MLPLayer embeddings :201-222, ALIGNNConv x alignn_layers :132-167,
 * EdgeGatedGraphConv x gcn_layers :48-129, AvgPooling + fc :325,341) or torch.autograd's backward of it - what the
 * reference's per-batch loop (alignn/train.py:258-270: a NEW (g, lg) every iteration, so nothing can be replayed) pays
 * per step.  The same kernels with the same arguments as the per-operator entry points above (bit-identical results),
 * issued from C over ONE caller-owned workspace whose layout is a pure function of the model dimensions and (N, E, T).
 *   alignn_model_init:  once per device, outside stream capture - the event pool the helper streams are ordered with
 *   alignn_model_plan:  bytes of workspace the forward / forward + backward of this batch need; hipErrorNotSupported
 *                       (801) when a kernel choice is not carried here (the caller then sequences the operators itself)
 *   alignn_model_fwd:   out[B, out_features] = fc(pool(...)); running statistics and num_batches_tracked updated
 *   alignn_model_bwd:   parameter gradients into the g_* / *red pointers of the parameter blocks; the workspace must be
 *                       the one the forward of the same (desc, batch) filled
 * Gradient layout: `red` / `n_red` / `e_red` = [2, F] = (dbeta | dgamma) of the norm; g_wcat [4H, H] = the four node
 * projections' weight gradients as row blocks (src_gate, dst_gate, dst_update, src_update), g_bcat [4H] likewise.
 * Streams (desc): lane_T / side / aux optional helper streams (NULL: the caller's); every one is joined back into
 * `stream` before a call returns.
 * ------------------------------------------------------------------------------------------ */
typedef struct alignn_mlp_params {
    const float *W, *b, *gamma, *beta;         /* Linear [out, in] / [out], BatchNorm1d affine */
    float *rm, *rv;                            /* running_mean / running_var (updated) */
    float *gW, *gb, *red;                      /* gradients: [out, in], [out], [2, out] = dbeta | dgamma */
    const void *img, *img_t;                   /* f16x2 slice images of W / W^T (alignn_prepare_weights) or NULL */
    const float* w_amax;
    int32_t in, out;
} alignn_mlp_params;

typedef struct alignn_conv_params {
    const float *wcat, *bcat, *w_eg, *b_eg;    /* fused node projection [4H, H] / [4H]; edge_gate [H, H] / [H] */
    const float *n_gamma, *n_beta, *e_gamma, *e_beta;
    float *n_rm, *n_rv, *e_rm, *e_rv;
    float *g_wcat, *g_bcat, *g_weg, *g_beg, *n_red, *e_red;
    const void *wcat_img, *wcat_img_t, *weg_img, *weg_img_t;
    const float *wcat_amax, *weg_amax;
} alignn_conv_params;

typedef struct alignn_graph_csr {              /* canonical CSR (see the conventions at the top of this file) */
    const int32_t *seg_ptr, *seg_node, *src, *dst, *out_ptr, *out_slot;
    const int32_t *grp_seg_ptr, *grp_src_ptr, *seg_rank; /* line graphs: dense blocks per centre atom; segment of every row */
    int64_t n, m, n_groups;
    int32_t dense_max_src, pad_;
} alignn_graph_csr;

typedef struct alignn_model_batch {
    alignn_graph_csr g, lg;
    const int32_t* graph_ptr;                  /* [B + 1] atom offsets per crystal */
    const float *atom_features, *r, *h;        /* [N, atom_in], [E, 3] bond vectors, [T] bond-angle cosines (canonical order) */
    int32_t B, pad_;
} alignn_model_batch;

typedef struct alignn_model_desc {
    int32_t alignn_layers, gcn_layers, H, out_features, atom_in, edge_bins, angle_bins, embed;
    float edge_gamma, angle_gamma, eps, momentum;
    const float *edge_centers, *angle_centers;
    alignn_mlp_params atom, edge1, edge2, angle1, angle2;
    const alignn_conv_params* convs;           /* HOST array: (node_update, edge_update) x alignn_layers, then gcn_layers */
    const float *fc_W, *fc_b;
    float *g_fc_W, *g_fc_b;
    const void* weight_descs;                  /* alignn_prepare_weights' device table (n_weights records) or NULL */
    float* weight_amax;
    const void* bump_ptrs;                     /* device array of n_bump int64_t* (num_batches_tracked), each += 1 per forward */
    int32_t n_weights, n_bump;
    int32_t x6_min_tiles, bd_segment_table;    /* kernel-choice constants of the per-operator path (256, 1) */
    int32_t angle_fused, norm;                 /* 1: the angle embedding through alignn_angle_embed_fwd / _bwd where its shapes allow;
                                                  norm: 0 BatchNorm1d (ALIGNN), 1 LayerNorm (ALIGNNAtomWise: rm / rv / bump_ptrs unused) */
    int32_t reuse_tape, dw_fused;              /* reuse_tape 1: a convolution's edge input gradient is written over its own (then dead)
                                                  gate pre-activation m - one T-row buffer per line-graph convolution less; the tape
                                                  does not survive the backward (no second backward of a retained graph).
                                                  dw_fused n > 0: the edge-gate projection's input gradient and weight gradient in one
                                                  pass over g_m (csrc/gemm_dw.hip) for convolutions of >= n edge rows where
                                                  alignn_gemm_dgrad_wgrad_supported; 0: always the two launches */
    int64_t amax_min_rows, lane_min_rows, side_min_rows; /* 4096; rows from which a kernel goes to lane_T / side */
    alignn_stream_t lane_T, side, aux;
} alignn_model_desc;

int alignn_model_init(void);
size_t alignn_model_sizeof(int which); /* 0 mlp_params, 1 conv_params, 2 graph_csr, 3 model_batch, 4 model_desc */
int alignn_model_plan(const alignn_model_desc* desc, const alignn_model_batch* batch, size_t* fwd_bytes, size_t* total_bytes);
int alignn_model_fwd(const alignn_model_desc* desc, const alignn_model_batch* batch, void* workspace, size_t workspace_bytes,
                     float* out, alignn_stream_t stream);
int alignn_model_bwd(const alignn_model_desc* desc, const alignn_model_batch* batch, void* workspace, size_t workspace_bytes,
                     const float* g_out, alignn_stream_t stream);
/* ALIGNN.forward in eval mode without autograd (alignn/pretrained.py; model.eval() under torch.no_grad()): BatchNorm = the
 * affine map of its running statistics, edge outputs straight from alignn_egc_gate_infer, nothing kept.  _workspace: bytes
 * for this (desc, batch), 0 when a kernel choice is not carried here.  Uses desc->lane_T only. */
size_t alignn_model_infer_workspace(const alignn_model_desc* desc, const alignn_model_batch* batch);
int alignn_model_infer(const alignn_model_desc* desc, const alignn_model_batch* batch, void* workspace, size_t workspace_bytes,
                       float* out, alignn_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * ALIGNNAtomWise with the force / stress head as whole-model calls (csrc/model.hip + csrc/ff.hip):
 * alignn/models/alignn_atomwise.py:364-660 with calculate_gradient=True - what alignn/train.py:291-387 trains and what
 * alignn/ff/calculators.py:280-291 evaluates at every MD step.  desc->norm must be 1 (LayerNorm flavour).
 *   alignn_ff_eval: energies out[B] (:494-510), forces[N, 3] = reduce(grad_multiplier dE_tot/dr) (:530-565), stresses
 *                   [B, 3, 3] (:615-638; NULL: none) - the forward pass with the bond vectors as a leaf and its reverse
 *                   w.r.t. them (no parameter gradients); bond cosines recomputed from r when lg_on_fly (:424-431),
 *                   else batch->h.
 *   alignn_ff_grad: parameter gradients of a loss L(out, forces, stresses) given g_out[B], g_forces[N, 3], g_stress[B, 3, 3]
 *                   (each may be NULL = zero): the force / stress part is linear in the pair forces, sum_e w_e . f_e =
 *                   c D_w E_tot, so its parameter gradient is ONE reverse pass over a forward pass that carries a tangent
 *                   next to every activation (forward-over-reverse instead of autograd.grad(create_graph=True) + a second
 *                   backward; csrc/dual.hip).  The value halves are the tape alignn_ff_eval left in the workspace, which
 *                   must be the one that call filled for the same (desc, batch, ff).  Gradients go to the g_* / *red
 *                   pointers of desc, which must all lie inside gflat[0 .. grad_floats) ; gflat_t is scratch of the same
 *                   size (the tangent halves of the weight gradients, added on return).  Optionally a SECOND region of
 *                   destinations, gsink[0 .. sink_floats) with scratch gsink_t of the same size: the optimizer's packed
 *                   gradient buffer (alignn_amd/optim.py FlatAdamW) - desc pointers inside it get their tangent halves in
 *                   gsink_t and the sum in place, so that no gather of per-parameter gradients follows (NULL, NULL, 0: none).
 *   alignn_ff_plan: workspace bytes for eval alone / eval + grad; 801 when a kernel choice is not carried here.
 * ------------------------------------------------------------------------------------------ */
typedef struct alignn_ff_desc {
    int32_t lg_on_fly, add_reverse_forces, force_mult_natoms, energy_mult_natoms, has_stress, use_penalty;
    int32_t dense_lg_reverse, pad_;
    float grad_multiplier, stress_multiplier, penalty_factor, penalty_threshold;
    const float* volume;                       /* [B] cell volumes (stress) or NULL */
} alignn_ff_desc;
size_t alignn_ff_desc_sizeof(void);
int alignn_debug_allocs(size_t* out, int cap); /* debugging aid, see csrc/model.hip */
int alignn_ff_plan(const alignn_model_desc* desc, const alignn_model_batch* batch, const alignn_ff_desc* ff, size_t* eval_bytes,
                   size_t* total_bytes);
int alignn_ff_eval(const alignn_model_desc* desc, const alignn_model_batch* batch, const alignn_ff_desc* ff, void* workspace,
                   size_t workspace_bytes, float* out, float* forces, float* stress, alignn_stream_t stream);
int alignn_ff_grad(const alignn_model_desc* desc, const alignn_model_batch* batch, const alignn_ff_desc* ff, void* workspace,
                   size_t workspace_bytes, const float* g_out, const float* g_forces, const float* g_stress, float* gflat,
                   float* gflat_t, int64_t grad_floats, float* gsink, float* gsink_t, int64_t sink_floats, alignn_stream_t stream);

/* The small kernels of the force-field head (csrc/ff.hip), also used one by one by the per-operator path
 * (alignn_amd/alignn_atomwise.py, alignn_amd/ff2.py) - they replace ~100 torch element-wise / index / reduce launches and a
 * vendor GEMM (torch.einsum for a 3 x 3 mat-vec per bond) per training step:
 *   pair_force_reduce   forces[i] = scale (sum_{e into i} g_r[e] - [add_reverse] sum_{e out of i} g_r[e])  (DGL copy_e / sum on
 *                       g and dgl.reverse(g), alignn_atomwise.py:547-565); scale = grad_multiplier (* N: force_mult_natoms)
 *   virial_stress       stress[g] = (k scale / V_g) sum_{e in g} r_e (x) g_r[e], k = stress_multiplier * -160.21766208 (:615-638)
 *   ff_energy           out[g] per alignn_atomwise.py:494-510 (penalty summed over ALL bonds of the batch) and seed[g] =
 *                       d(sum en_out)/d pred[g];  ff_penalty_bwd: g_bl[e] += -B factor [bl[e] < thr]
 *   ff_pair_weights     w[e] = dL/d(pair force e) = gF[dst] - [add_reverse] gF[src] + (kS / V_g) gS_g^T r[e]; *wmax raised to
 *                       max|w| (zeroed by the caller)
 *   ff_tangent_geometry rt = w / 2^floor(log2 wmax) (1 if wmax == 0), dt = r . rt / d
 *   rbf_tangent         out_t[r][k] = exp(-gamma (d - c_k)^2) (-2 gamma (d - c_k)) dt[r]
 *   bond_cosine_tangent ht[k] = D_rt of compute_bond_cosines (alignn/graphs.py:847-864), 0 where its clamp is active
 *   ff_readout_seed     adjoints of x_i under E_g = fc(mean_i x_i): gx[i] = (ge[g] / n_g) fc_w, gxt[i] = (c_g 2^k / n_g) fc_w,
 *                       c_g = c (* n_g: energy_mult_natoms);  ff_fc_grad: gW = sum_g ge[g] hp[g] + c_g 2^k hpt[g], gb = sum ge
 *   add_inplace / add3  a += b;  out = (a + b) + c   (n % 4 == 0 / any n) */
int alignn_pair_force_reduce(const float* g_r, float scale, const int32_t* seg_ptr, const int32_t* out_ptr, const int32_t* out_slot,
                             int add_reverse, float* forces, int64_t n_nodes, alignn_stream_t stream);
int alignn_virial_stress(const float* r, const float* g_r, float scale, const int32_t* graph_ptr, const int32_t* seg_ptr,
                         const float* volume, float k, float* stress, int B, alignn_stream_t stream);
int alignn_ff_energy(const float* pred, const float* bl, const int32_t* graph_ptr, int B, int64_t E, int mult_natoms,
                     int use_penalty, float factor, float thr, float* out, float* seed, alignn_stream_t stream);
int alignn_ff_penalty_bwd(const float* bl, float* g_bl, int64_t E, int B, float factor, float thr, alignn_stream_t stream);
int alignn_ff_pair_weights(const float* gF, const float* gS, const float* r, const int32_t* src, const int32_t* dst,
                           const int32_t* graph_ptr, const int32_t* seg_ptr, const float* volume, float kS, int add_reverse, int B,
                           int64_t E, float* w, float* wmax, alignn_stream_t stream);
int alignn_ff_tangent_geometry(const float* r, const float* w, const float* wmax, const float* d, float* rt, float* dt, int64_t E,
                               alignn_stream_t stream);
int alignn_rbf_tangent(const float* d, const float* dt, const float* centers, float gamma, float* out_t, int64_t rows, int bins,
                       alignn_stream_t stream);
int alignn_bond_cosine_tangent(const float* r, const float* rt, const int32_t* e1, const int32_t* e2, float* ht, int64_t T,
                               alignn_stream_t stream);
int alignn_ff_readout_seed(const float* ge, float c, int mult_natoms, const float* wmax, const int32_t* graph_ptr, const float* fc_w,
                           float* gx, float* gxt, int B, int64_t N, int H, alignn_stream_t stream);
int alignn_ff_fc_grad(const float* ge, float c, int mult_natoms, const float* wmax, const int32_t* graph_ptr, const float* hp,
                      const float* hpt, float* gW, float* gb, int B, int H, alignn_stream_t stream);
int alignn_add_inplace(float* a, const float* b, int64_t n, alignn_stream_t stream);
int alignn_add3(const float* a, const float* b, const float* c, float* out, int64_t n, alignn_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * The bond-angle embedding on T rows (csrc/angle.hip):  z = MLPLayer(64 -> 256)(MLPLayer(bins -> 64)(RBFExpansion(h)))
 * (alignn/models/alignn.py:215-222 angle_embedding, :170-184 MLPLayer, alignn/models/utils.py:9-47 RBFExpansion) and
 * the gradients of its eight parameter tensors, WITHOUT the [T, bins] / [T, 64] / [T, 256] intermediates: every row is a
 * function of one cosine, so each pass recomputes what it needs from h on the matrix cores (f16x3 split products) and only z
 * (forward) / g_z and a [T, 64] gradient (backward) cross HBM.  Shapes carried: bins <= 48, 64 embedding features, 256
 * hidden features (alignn_angle_embed_supported).  BatchNorm in training mode: batch statistics, running statistics
 * updated (momentum), statistics kept in stat1 / stat2 for the backward; l1 / l2: the two layers' parameters, running
 * statistics and gradient destinations (img / img_t / w_amax unused).  scal: 128 floats the forward zeroes and both
 * directions use (operand scales, bounds).  Backward writes l?.gW, l?.gb, l?.red (= dbeta | dgamma); h gets no gradient.
 * The backward resets the maxima and bounds it raises itself: any number of backwards on the state of one forward, each
 * sliced at the scales of its own g_z. */
typedef struct alignn_angle_args {
    const float* h;                /* [rows] cosines */
    int64_t rows;
    const float* centers;          /* [bins] */
    float gamma;
    int32_t bins;
    alignn_mlp_params l1, l2;
    float eps, momentum;
    float *stat1, *stat2;          /* [4, 64], [4, 256]: mean | rstd | gamma rstd | beta */
    float* scal;                   /* [alignn_angle_embed_scal_floats()] */
    float *z, *z_amax;             /* forward: [rows, 256] and (optional) the tracked max|z| */
    const float* gz;               /* backward: [rows, 256] */
    void* workspace;
    size_t workspace_bytes;
} alignn_angle_args;
int alignn_angle_embed_supported(int bins, int embed, int hidden);
size_t alignn_angle_embed_workspace(int64_t rows, int bins, int backward);
size_t alignn_angle_args_sizeof(void);
int alignn_angle_embed_scal_floats(void);
int alignn_angle_embed_fwd(const alignn_angle_args* args, alignn_stream_t stream);
int alignn_angle_embed_bwd(const alignn_angle_args* args, alignn_stream_t stream);
/* evaluation mode: BatchNorm as the affine map of l?.rm / l?.rv (not updated); writes z (and z_amax), uses stat1 / stat2 /
 * scal as scratch, needs no workspace */
int alignn_angle_embed_infer(const alignn_angle_args* args, alignn_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Batch staging in one call (csrc/stage.hip): canonical CSR of g (slots = bonds stably sorted by
 * destination atom), its by-source view, the canonical line graph L(g) with its by-source view and segment ranks, the
 * bond vectors in slot order and the bond-angle cosines - from the COO bond list (u -> v, caller's order, int32) a loader
 * ships.  Replaces dgl.batch + g.to(device) + lg.to(device) of alignn/train.py:264-270 (alignn/lmdb_dataset.py:87-108
 * builds and ships L(g)'s T-sized COO list and compute_bond_cosines' output, alignn/graphs.py:847-864, per batch).
 * T = rows of L(g) = sum over bonds e2 of (in-degree of src(e2)) - [e2 is a self image] is a function of the bond list:
 * the caller computes it (and the largest in-degree, for alignn_egc_bwd_lg_dense) on the host when it packs the batch,
 * so nothing is read back.  Outputs (all caller-owned): seg_ptr / out_ptr [N+1], src / dst / out_slot [E] (out_slot is
 * also L(g)'s seg_node), perm / inv [E] int64 (slot k holds caller edge perm[k]), r_canon [E,3]; lg_seg_ptr / lg_out_ptr
 * [E+1], lg_src / lg_dst / lg_out_slot / lg_seg_rank [T], lg_ident [T] int64 = 0..T-1 (optional), h [T] (optional; needs
 * r).  workspace: alignn_stage_batch_workspace(N, E) bytes.  ~15 launches, no atomics, bit-identical to alignn_amd.graph's
 * build_csr + line_graph_of and to a line graph built from this definition alone (tests/test_gpu_stage_ref.py).
 * ------------------------------------------------------------------------------------------ */
size_t alignn_stage_batch_workspace(int64_t n_nodes, int64_t n_edges);
int alignn_stage_batch(const int32_t* u, const int32_t* v, const float* r, int64_t n_nodes, int64_t n_edges, int64_t n_triplets,
                       int32_t* seg_ptr, int32_t* src, int32_t* dst, int32_t* out_ptr, int32_t* out_slot, int64_t* perm,
                       int64_t* inv, float* r_canon, int32_t* lg_seg_ptr, int32_t* lg_src, int32_t* lg_dst,
                       int32_t* lg_out_ptr, int32_t* lg_out_slot, int32_t* lg_seg_rank, int64_t* lg_ident, float* h,
                       int32_t* out_rank /* optional [E]: rank of every slot in the by-source order */,
                       void* workspace, size_t workspace_bytes, alignn_stream_t stream);
/* The caller's OWN edge list of L(g) (the lg of the reference's (g, lg) pair: dgl's g.line_graph(shared=True), edges lg_u[k] ->
 * lg_v[k] in the caller's ids of g's edges, int64) mapped onto the canonical rows alignn_stage_batch laid out, by index
 * arithmetic (no T-sized sort): perm[t] = k (pre-fill with -1), inv_lg[k] = t, *bad (zeroed by the caller) += edges that are
 * not line-graph edges of g or repeat an earlier one.  n_triplets (= the T alignn_stage_batch was given) edges with bad == 0:
 * the caller's lg IS the line graph, perm a bijection, and its edge features go to canonical order as h[perm]. */
int alignn_map_line_graph_rows(const int64_t* lg_u, const int64_t* lg_v, const int64_t* inv, const int32_t* seg_ptr,
                               const int32_t* src, const int32_t* dst, const int32_t* out_rank, const int32_t* lg_seg_ptr,
                               int64_t n_edges, int64_t n_triplets, int64_t* perm, int64_t* inv_lg, int32_t* bad,
                               alignn_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Radius bond graphs on the device (csrc/radius.hip): alignn/graphs.py:267-364 (radius_graph),
 * the neighbour strategy of the reference's force-field configs, re-run by alignn/ff/calculators.py:280-291 at every MD
 * step.  One wavefront per site, float32 distances in the reference's dtype evaluated as one fixed operation sequence,
 * bonds emitted in torch.where order (source, then periodic image, then destination) - the reference's edge ORDER, no
 * sort, no atomics, no host synchronisation.  Inputs: lat[B][9] float32 (rows a, b, c), cart[N][3] float32, graph_ptr
 * [B+1], site_graph[N], box[B][levels][6] = nmin[3], nmax[3] of the image box per cutoff level (graphs.py:296-309),
 * cut[levels] = cutoff, cutoff + 0.5, ... (:349-358), atol (isclose-zero exclusion, 1e-5).
 *   radius_levels: crystal_level[B] = first level at which the crystal's last site has a neighbour (== levels: none)
 *   radius_count:  count[N] = bonds leaving each site at its crystal's level
 *   radius_emit:   offset[N] = exclusive prefix sum of count; u, v int64, r[.][3] float32 = x_dst - x_src, image[.][3]
 *                  int32 (optional)
 * ------------------------------------------------------------------------------------------ */
int alignn_radius_levels(const float* lat, const float* cart, const int32_t* graph_ptr, const int32_t* box, const float* cut,
                         float atol, int levels, int n_crystals, int32_t* crystal_level, alignn_stream_t stream);
int alignn_radius_count(const float* lat, const float* cart, const int32_t* graph_ptr, const int32_t* site_graph,
                        const int32_t* box, const float* cut, float atol, int levels, int64_t n_sites,
                        const int32_t* crystal_level, int64_t* count, alignn_stream_t stream);
int alignn_radius_emit(const float* lat, const float* cart, const int32_t* graph_ptr, const int32_t* site_graph,
                       const int32_t* box, const float* cut, float atol, int levels, int64_t n_sites,
                       const int32_t* crystal_level, const int64_t* offset, int64_t* u, int64_t* v, float* r, int32_t* image,
                       alignn_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Batched structure relaxation (csrc/relax.hip; alignn_amd/relax.py is the host loop): one FIRE step, ASE's
 * ase/optimize/fire.py as alignn/ff/ff.py:373-415 runs it (downhill_check=False), preceded by the convergence test of
 * Optimizer.run (max_i |F_i|^2 < fmax^2) on the forces of the current positions.  float64.  One workgroup per ACTIVE structure
 * k < n_active; structure s = active[k] owns atoms [atom_ptr[s], atom_ptr[s+1]) of the full-batch [N][3] arrays and row s of
 * the [B] / [B][3][3] (row-major) ones; the evaluation is that of the active batch.  A structure is recorded (forces_out,
 * energy_out, fmax_out, stress_out), then either retired (status[1+k] = 1: converged, 2: `steps` steps taken; -1: force rows
 * of another count than its atoms, nothing written) or stepped (status[1+k] = 0): |dr| over the structure clipped to maxstep.
 * Fixed-order reductions: a structure's step is bit-identical whatever else shares the launch.  B is the number of structures
 * of the batch (atom_ptr has B + 1 entries), N = atom_ptr[B].  Only a stepped structure's state is rewritten - its rows of
 * positions, velocities, frac (xa), its state and istate (xc, cell_velocities, defgrad, lattice) - and nothing of a structure
 * that is not in `active` is read or written.
 *
 * At fixed cell (xc == NULL; optimize_lattice=False) the rows are the atoms'.  With a cell-filter state (xc != NULL: every
 * field marked "filter" is then required, and ignored otherwise) the step is that of ASE's ExpCellFilter (ase/constraints.py,
 * default arguments; optimize_lattice=True) over n + 3 generalised rows per structure of n atoms: atom rows X_a = positions
 * F^-T with forces f F, cell rows X_c = n logm(F) of the deformation gradient F with the forces: the virial W = -|det C|
 * sym(stress), or the exact gradient -expm([[L, -W expm(-L)], [0, L]])[0:3, 3:6] (symmetrised, L = X_c / n) where the two
 * point apart (cosine <= 0.8 and not numpy-isclose), divided by n.  Convergence and fmax_out run over all n + 3 rows.
 * Initial filter state: xa = positions, xc = cell_velocities = 0, defgrad = I, lattice = lattice0.
 *
 * Constraints (the last fields of the block; NULL / 0 is off, and the step is then the same bits as without them).
 * `fixed` is ASE's FixAtoms: a fixed atom's force row is zero wherever the step reduces or integrates it (forces_out keeps
 * the force as evaluated), so its row X_a and its velocity never change; its frac is not rewritten, and at fixed cell neither
 * is its position.  The others are ExpCellFilter's arguments, in ASE's order: W = -|det C| (sym(stress) + scalar_pressure I);
 * hydrostatic_strain: W <- (tr W / 3) I; W <- W * cell_mask elementwise; the naive / exact choice on this W; constant_volume:
 * tr / 3 taken off the diagonal of the chosen force; then / n.  enthalpy_out[s] = energy + scalar_pressure |det C| of the
 * evaluated cell.
 * ------------------------------------------------------------------------------------------ */
typedef struct alignn_fire_args {
    /* inputs of the step: the evaluation of the active batch */
    const double* forces;      /* [force_ptr[n_active]][3]: rows [force_ptr[k], force_ptr[k+1]) are active[k]'s */
    const double* energy;      /* [n_active] */
    const double* stress;      /* filter: [n_active][3][3], eV/A^3, ASE's sign */
    const int32_t* force_ptr;  /* [n_active + 1] */
    const int32_t* active;     /* [n_active] structure indices */
    const int32_t* atom_ptr;   /* [B + 1] */
    const double* inv_lattice; /* [B][3][3] inverse of the cell (filter: of lattice0): frac = rows times it, wrapped into [0, 1) */
    const double* lattice0;    /* filter: [B][3][3] the starting cells C0 */
    /* state */
    double* positions;       /* [N][3] Cartesian, unwrapped (filter: written as X_a F^T) */
    double* velocities;      /* [N][3] of the atom rows */
    double* frac;            /* [N][3] for the next neighbour search */
    double* state;           /* [B][2] = {dt, a} */
    int32_t* istate;         /* [B][2] = {Nsteps, steps taken} */
    double* xa;              /* filter: [N][3] atom rows X_a */
    double* xc;              /* filter: [B][3][3] cell rows X_c; non-NULL selects the filter */
    double* cell_velocities; /* filter: [B][3][3] */
    double* defgrad;         /* filter: [B][3][3] F of the evaluated cell */
    double* lattice;         /* filter: [B][3][3] the current cells C = C0 F^T */
    /* outputs */
    double* forces_out;  /* [N][3]; these five: the rows of the active structures whose force rows fit */
    double* energy_out;  /* [B] */
    double* fmax_out;    /* [B] max over the rows of |F_i| */
    double* stress_out;  /* filter: [B][3][3] symmetrised */
    int32_t* status;     /* [1 + n_active]: [0] the number of structures stepped, [1+k] as above */
    /* scalars */
    int n_active, steps, nmin; /* `steps`: the cap per structure; nmin: FIRE's Nmin */
    double fmax, maxstep, dtmax, finc, fdec, astart, fa; /* the tolerance and FIRE's parameters */
    /* constraints: NULL / 0 is off */
    const uint8_t* fixed;          /* [N] non-zero: the atom is held (FixAtoms) */
    const double* cell_mask;       /* filter: [B][3][3] of 0 / 1, ExpCellFilter's mask as the full 3x3 */
    const double* scalar_pressure; /* filter: [B] eV/A^3 */
    int hydrostatic_strain, constant_volume; /* filter: ExpCellFilter's flags, the same for every structure */
    double* enthalpy_out;          /* filter: [B] energy + scalar_pressure * volume */
} alignn_fire_args;
int alignn_fire_step(const alignn_fire_args* args, alignn_stream_t stream);
size_t alignn_fire_args_sizeof(void); /* a binding checks its own packing against this */

/* ------------------------------------------------------------------------------------------
 * Batched molecular dynamics (csrc/dynamics.hip; alignn_amd/dynamics.py is the host loop): ASE 3.22.1's VelocityVerlet
 * (ensemble 0), Langevin (1), NVTBerendsen (2), Andersen (3) and NPTBerendsen (4; isotropic) as alignn/ff/ff.py:419-600 runs
 * them, and Nose-Hoover chain NVT (5) and isotropic MTK NPT (6), float64, ASE units (eV, A, amu, A sqrt(amu / eV)).  One workgroup per structure s < n_structures; it owns atoms
 * [atom_ptr[s], atom_ptr[s+1]) of the [N] / [N][3] arrays and row s of the [B] / [B][3][3] (row-major) ones.  One launch per
 * evaluation t = 0 .. steps: finish step t (t > 0: the second half-kick with these forces), record frame t / interval when
 * t % interval == 0, then, unless t == steps, begin step t + 1 (Berendsen's velocity scaling; the first half-kick; fixcm's
 * corrections; the drift; frac).  NPT begins a step with the Berendsen velocity scaling, then mu = 1 - dt / taup *
 * compressibility / 3 * (pressure - P) with P from the scaled momenta, lattice and positions times mu, inv_lattice
 * recomputed, then the half-kick, fixcm and the drift.  Andersen begins a step with v = p / m, fixcm: + a random
 * centre-of-mass velocity of width sqrt(kB T0 / sum m); the half-kick; every velocity component whose uniform draw is <=
 * andersen_prob replaced by a normal of width sqrt(kB T0 / m); fixcm: the mass-weighted mean velocity removed and the centre
 * of mass kept through the drift; v recomputed from the positions.  Random numbers: Philox4x32-10, key seeds[s], counter (atom,
 * t, block, purpose): Langevin blocks 0..2 of purpose 0 (6 normals); Andersen blocks 0..3 of purpose 2 (0, 1: normals; 2, 3:
 * uniforms in (0, 1]) and, for the centre of mass, blocks 0..1 of (0, t, ., 3).  Fixed-order reductions: a structure's
 * trajectory is bit-identical whatever else shares the launch.  "Required" below: NULL is hipErrorInvalidValue.
 * Ensembles 5 (nvt_nose_hoover) and 6 (npt_nose_hoover; isotropic) are not ASE's: Nose-Hoover chains and the MTK barostat in
 * the explicit reversible form of Martyna, Tuckerman, Tobias and Klein (Mol. Phys. 87, 1117, 1996; the barostat as in Tuckerman
 * et al., J. Phys. A 39, 5629, 2006).  With kT = kB t0_kelvin[s], g = 3 n: chain masses Q_0 = g kT ttime^2, Q_k = kT ttime^2,
 * barostat mass W = (g + 3) kT ptime^2, its own chain Q'_k = kT ptime^2.  A launch finishes step t (half-kick, v_eps += dt/2
 * G_eps, the particles' chain dt/2, the barostat's chain dt/2), records, and begins step t + 1 in the mirrored order (chains,
 * v_eps, half-kick, drift with cell and positions times exp(v_eps dt)); G_eps = ((1 + 3/g) sum p^2/m - V tr(stress) - 3 V
 * pressure) / W.  conserved_out: H' = KE + energy + sum_k Q_k v_k^2 / 2 + g kT eta_0 + kT sum_{k>=1} eta_k + pressure V + W
 * v_eps^2 / 2 + sum_k Q'_k v'_k^2 / 2 + kT sum_k eta'_k (the parts that are on).  fixcm (5, 6): at t = 0 only, momenta -= m sum
 * p / sum m.  Out-of-range chain / nhc_loops / nhc_order are hipErrorInvalidValue.
 * ------------------------------------------------------------------------------------------ */
typedef struct alignn_md_args {
    /* inputs of the step: the evaluation at the current positions */
    const double* forces;  /* [n_rows][3] */
    const double* energy;  /* [B] = [n_structures]; N below is atom_ptr[B] */
    const double* stress;  /* [B][3][3], eV/A^3, ASE's sign: required by 4 and by 6 with ptime > 0; 3, 6: NULL records no
                              pressure; 0-2, 5: ignored */
    int64_t n_rows;        /* must equal atom_ptr[n_structures], else status[0] = -1 and nothing is written */
    const int32_t* atom_ptr;       /* [B + 1] */
    const double* masses;          /* [N] */
    const double* t0_kelvin;       /* [B] thermostat targets: required by 1-6 */
    const uint64_t* seeds;         /* [B]: required by 1 and 3 */
    const double* pressure;        /* [B] barostat targets, eV/A^3: required by 4 and by 6 with ptime > 0 */
    const double* compressibility; /* [B] A^3/eV: required by 4 */
    /* state */
    double* lattice;     /* [B][3][3]: required by 3 (read), 4 and 6 (rewritten; 6: while ptime > 0); 0-2, 5: ignored */
    double* inv_lattice; /* [B][3][3]: frac = positions times it, wrapped into [0, 1); 4 and 6 rewrite it */
    double* momenta;     /* [N][3] */
    double* positions;   /* [N][3] Cartesian, unwrapped */
    double* frac;        /* [N][3] for the next neighbour search */
    double* velocities;  /* [N][3] v between the halves: required by 1 and 3 */
    double* scratch;     /* [N][3] between the halves, 1: the velocity noise of the step, 3: the positions before the drift; required by both */
    int32_t* status;     /* [1]; required; zeroed by the caller: a launch writes it only where n_rows does not fit */
    /* outputs: frames [steps / interval + 1]; epot, ekin, temperature required, the others written unless NULL */
    double* epot;           /* [frames][B] = energy */
    double* ekin;           /* [frames][B] KE = 0.5 sum p^2 / m */
    double* temperature;    /* [frames][B] 2 KE / (3 n kB) */
    double* pressure_out;   /* 3, 4, 6: [frames][B] -tr(stress) / 3 + 2 KE / (3 V); needs stress */
    double* volume_out;     /* 3, 4, 6: [frames][B] V = |det lattice| */
    double* traj_positions; /* [frames][N][3] */
    double* traj_momenta;   /* [frames][N][3] */
    double* traj_lattice;   /* 3, 4, 6: [frames][B][3][3] */
    double* noise_out;      /* tests: 1: [N][18] per atom xi[3], eta[3], the 12 Philox words as doubles; 3: [N][36] (with and
                               without fixcm) per atom 4 normals, 4 uniforms, 16 words, then the structure's 4 centre-of-mass
                               normals and their 8 words (written with fixcm only: without it the last 12 of every 36 are left
                               as they are); written by the launches that begin a step (t < steps); 0, 2, 4-6: ignored */
    /* scalars */
    int n_structures, t, interval, steps, ensemble, fixcm;
    double dt, friction, andersen_prob, taut, taup, kB; /* friction: 1; andersen_prob: 3; taut: 2, 4; taup: 4 */
    /* Nose-Hoover chains (5) and isotropic MTK (6): NULL / 0 is off, and 0-4 ignore them */
    double* nhc_state;     /* [B][34] per structure eta[8], v[8] (the particles' chain: positions and velocities of its links),
                              eta'[8], v'[8] (the barostat's chain), eps = ln(V / V0) / 3, v_eps; zero at the start; required by
                              5 and 6, rewritten every launch */
    double* conserved_out; /* 5, 6: [frames][B] the conserved energy H' (eV), see above */
    int chain, nhc_loops, nhc_order; /* 5, 6: links per chain 1..8, n_c 1..16, the Suzuki-Yoshida order 1, 3 or 5 */
    double ttime, ptime;   /* 5, 6: the thermostat's / (6) the barostat's time constant, ASE time units; <= 0: that part is off */
} alignn_md_args;
int alignn_md_step(const alignn_md_args* args, alignn_stream_t stream);
size_t alignn_md_args_sizeof(void); /* a binding checks its own packing against this */

/* Maxwell-Boltzmann momenta (ASE's MaxwellBoltzmannDistribution, no Stationary): momenta[i] = xi sqrt(m_i kB t_kelvin[s]) with
 * xi three normals of the stream above (counter (atom, 0, block 0..1, 1)). */
int alignn_md_init_momenta(const int32_t* atom_ptr, int n_structures, const double* masses, const double* t_kelvin,
                           const uint64_t* seeds, double* momenta, double kB, alignn_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Batched finite-displacement phonons (csrc/phonon.hip; alignn_amd/phonons.py is the host loop): ASE 3.22.1's Phonons as
 * the reference's ase_phonon runs it (alignn/ff/ff.py:1337), float64.  Structure s has n_s = atom_ptr[s+1] - atom_ptr[s]
 * atoms, m_s = 3 n_s, a supercell supercell[s] = (N0, N1, N2) of Ncell_s = N0 N1 N2 images (atom j = image n_s + b, image =
 * (m0 N1 + m1) N2 + m2), and its force constants C [Ncell_s][m_s][m_s] at fc_off[s] of the fc buffers.
 *
 * _displace: for job k < n_jobs, jobs [n_jobs][2] (int), jobs[k] = (s, d), d = 6a + 2i + sign (0: -delta, 1: +delta) moves atom
 * a of image 0 along axis i; row_off [n_jobs].  Writes the supercell's n_s Ncell_s rows from row_off[k] of frac [rows][3]
 * (wrapped into [0, 1) with inv_supercell[s], the inverse of the supercell lattice) and, unless NULL, of cart [rows][3]
 * (Cartesian, unwrapped: positions + image offsets of the primitive lattice[s] + the displacement); rows = the largest
 * row_off[k] + n_s Ncell_s.  positions [atom_ptr[B]][3], atom_ptr [B + 1], lattice and inv_supercell [B][3][3], supercell [B][3].
 * _fc_rows: pair k: pairs [n_pairs][2], pairs[k] = (s, x = 3a + i); the minus supercell's forces are rows [pair_rows[k], + n_s
 * Ncell_s) of forces, the plus supercell's the rows after (pair_rows [n_pairs]; forces [.][3] ends with the last pair's plus
 * supercell).  Writes row x of every cell of fc (fc_off [B]; fc holds every structure's C): (F- - F+) / (2 delta) after the
 * drift correction (0 none, 1 Frederiksen: the supercell's force sum off atom a's row, 2 mean: sum / (n_s Ncell_s) off every
 * row).
 * _symmetrize (out of place), _acoustic (in place): one pass of ASE's Phonons.symmetrize / Phonons.acoustic (offset 0).
 * _mass_weight: dyn = fc * (m_x^-1/2 m_y^-1/2) (masses [atoms] in amu).  max_elems = max_s Ncell_s m_s^2, max_atoms = max_s n_s.
 * _eigh: one workgroup per (q < n_q, structure).  D(q) = sum_R dyn[R] exp(-2 pi i q.R) over the lattice points of rows
 * [cell_ptr[s], cell_ptr[s+1]) of lattice_points [.][3] (int) paired with the cells of dyn at dyn_off[s] (dims[s] = m_s <=
 * max_dim <= alignn_phonon_eigh_max_dim()), from its upper triangle; parallel cyclic Jacobi in LDS.  dyn_off, dims, freq_off
 * and mode_off are [n_structures], cell_ptr [n_structures + 1], qpoints [n_q][3].  Writes per structure,
 * ascending per q: freqs [n_q][m_s] at freq_off[s] (sign(l) scale sqrt(|l|)), eigvals (the same shape; NULL: not written),
 * modes [n_q][m_s][m_s] complex (interleaved re, im; column r = the eigenvector of eigenvalue r; NULL: not computed) at
 * mode_off[s] (in doubles).  status[0] = 1 when a (q, structure) hit the sweep cap; untouched otherwise.
 * _dos: per structure s < n_structures over freqs [freq_off[s], freq_off[s+1]) (freq_off [n_structures + 1]): energies
 * [s][npts] = linspace(min - 3 width, max + 3 width, npts), weights [s][npts] = sum of unit Gaussians of `width` at those
 * energies.
 * Fixed-order reductions: a structure's results are bit-identical whatever else shares the launches.
 * ------------------------------------------------------------------------------------------ */
int alignn_phonon_displace(const double* positions, const int32_t* atom_ptr, const double* lattice, const double* inv_supercell,
                           const int32_t* supercell, const int32_t* jobs, const int64_t* row_off, int n_jobs, double delta,
                           double* frac, double* cart, alignn_stream_t stream);
int alignn_phonon_fc_rows(const double* forces, const int32_t* pairs, const int64_t* pair_rows, int n_pairs,
                          const int32_t* atom_ptr, const int32_t* supercell, const int64_t* fc_off, int drift, double delta,
                          double* fc, alignn_stream_t stream);
int alignn_phonon_symmetrize(const double* fc_in, double* fc_out, const int32_t* atom_ptr, const int32_t* supercell,
                             const int64_t* fc_off, int n_structures, int64_t max_elems, alignn_stream_t stream);
int alignn_phonon_acoustic(double* fc, const int32_t* atom_ptr, const int32_t* supercell, const int64_t* fc_off,
                           int n_structures, int max_atoms, alignn_stream_t stream);
int alignn_phonon_mass_weight(const double* fc, double* dyn, const double* masses, const int32_t* atom_ptr,
                              const int32_t* supercell, const int64_t* fc_off, int n_structures, int64_t max_elems,
                              alignn_stream_t stream);
int alignn_phonon_eigh_max_dim(void);
int alignn_phonon_eigh(const double* dyn, const int64_t* dyn_off, const int32_t* lattice_points, const int32_t* cell_ptr,
                       const int32_t* dims, int n_structures, int max_dim, const double* qpoints, int n_q, double scale,
                       double* freqs, const int64_t* freq_off, double* eigvals, double* modes, const int64_t* mode_off,
                       int32_t* status, alignn_stream_t stream);
int alignn_phonon_dos(const double* freqs, const int64_t* freq_off, int n_structures, int npts, double width, double* energies,
                      double* weights, alignn_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Builders of the defect tasks' derived structures (csrc/defects.hip; alignn_amd/defects.py is the driver, tests/defects_ref.py
 * the numpy restatement).  positions [atoms][3] Cartesian, atom_ptr [n_structures + 1] and lattice [n_structures][3][3] (rows
 * a, b, c) are the packed parents.  Job k writes its cell to cells [k][3][3] and its rows [row_off[k], row_off[k+1]) (row_off
 * [n_jobs + 1]; the row arrays have row_off[n_jobs] rows) of cart [.][3] (Cartesian), frac [.][3] (wrapped into [0, 1) of its
 * cell) and src [.] (the row of positions an atom came from).  One
 * workgroup per job, float64 without contraction, fixed-order sums: a job's bits do not depend on the launch it is in.  A job
 * whose fields or row range do not fit (structure index, removed atom, layers, |det| of the basis, row count) writes nothing.
 *
 * _supercells: jobs [n_jobs][2] = (s, a): the supercell (N0, N1, N2) = supercell[s] of structure s, atom j = image n_s + b,
 * image = (m0 N1 + m1) N2 + m2, cart = ((r_b + m0 L0) + m1 L1) + m2 L2, cell diag(N) L; a = -1: all n_s N0 N1 N2 atoms; a >= 0:
 * without supercell atom a, the later rows one up.
 * _slab_build: jobs [n_jobs][11] = (s, c1 [3], c2 [3], c3 [3], layers), vacuum [n_jobs] (A): the slab of `layers` repeats of the
 * parent re-expressed in the unimodular integer basis Bm (rows c1, c2, c3), n_s layers atoms, atom j = layer n_s + b.
 * C = Bm L; oriented fractions o = frac Bm^-1 (integer adjugate), o -= floor(o + 1e-10); layer m at (o0 C0 + o1 C1) + (o2 + m) C2;
 * a3 = nu ((layers C2) . nu) / (nu . nu), nu = C0 x C1; the positions wrapped (floor(f + 1e-10)) into [C0, C1, a3]; the cell
 * written is [C0, C1, a3 + vacuum a3 / |a3|]: the slab at the bottom of the cell, the vacuum above it.
 * ------------------------------------------------------------------------------------------ */
int alignn_defect_supercells(const double* positions, const int32_t* atom_ptr, const double* lattice, const int32_t* supercell,
                             int n_structures, const int32_t* jobs, const int64_t* row_off, int n_jobs, double* cells,
                             double* cart, double* frac, int32_t* src, alignn_stream_t stream);
int alignn_slab_build(const double* positions, const int32_t* atom_ptr, const double* lattice, int n_structures,
                      const int32_t* jobs, const double* vacuum, const int64_t* row_off, int n_jobs, double* cells, double* cart,
                      double* frac, int32_t* src, alignn_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * The E-V curve task (csrc/eos.hip; alignn_amd/eos.py is the driver, tests/eos_ref.py the numpy restatement).  float64 without
 * contraction, no atomics, fixed-order sums: a job's / a structure's bits do not depend on the launch it is in.
 *
 * _strain_build: the packed parents as for the builders above; job k strains parent jobs[k] by the deformation defgrad [k][3][3]
 * (row-major F): row i of cells [k][3][3] is row i of the parent's cell times F, (x0 F0j + x1 F1j) + x2 F2j; its n_s rows
 * [row_off[k], row_off[k+1]) of cart [.][3] are r F in the same order; volume [k] = |det| of the new cell by the cofactor
 * expansion along its first row.  One workgroup per job.  A job whose parent index or row count does not fit writes nothing.
 *
 * _eos_fit: structure s has its points in volume / energy [s][0 .. K_s) of rows of `ld` doubles, K_s = n_points[s] (NULL: ld);
 * 4 <= ld <= 64.  form 0: Murnaghan, 1: Birch-Murnaghan (ase/eos.py).  One wavefront per structure, one lane per point: the
 * least-squares parabola in (V - mean V) / (max V - min V) gives ASE's start (E0 = parabola(vmin), B0 = 2 c vmin, BP = 4, V0 =
 * vmin = -b / 2c); then Levenberg-Marquardt with the analytic Jacobian, (J^T J + lambda diag J^T J) delta = -J^T r by Cholesky,
 * lambda from 1e-3: a step with a finite sum of squares S' <= S is taken (lambda = max(lambda / 10, 1e-15)) and ends the fit
 * when max |delta| <= 1e-13 max |p| or S - S' <= 1e-16 S; otherwise lambda = 10 lambda, and lambda > 1e15 ends it too (no step
 * lowers S).  Writes params [s][4] = (E0, B0, BP, V0), rms [s] = sqrt(S / K_s), n_iter [s] (steps taken) and status [s]: 0
 * converged, 1 stopped after 100 steps (the parameters as they stand), 2 no start (K_s < 4 or > ld, a parabola with c <= 0, a
 * non-finite value): NaN params and rms, n_iter 0.  log and exp are the file's own (plain arithmetic), so the results are the
 * restatement's bits.
 * ------------------------------------------------------------------------------------------ */
int alignn_strain_build(const double* positions, const int32_t* atom_ptr, const double* lattice, int n_structures,
                        const int32_t* jobs, const double* defgrad, const int64_t* row_off, int n_jobs, double* cells, double* cart,
                        double* volume, alignn_stream_t stream);
int alignn_eos_fit(const double* volume, const double* energy, const int32_t* n_points, int n_structures, int ld, int form,
                   double* params, double* rms, int32_t* n_iter, int32_t* status, alignn_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * The elastic-tensor task (csrc/elastic.hip; alignn_amd/elastic.py is the driver, tests/elastic_ref.py the numpy restatement).
 * float64 without contraction, no atomics, fixed-order sums: a crystal's bits do not depend on the launch it is in.
 *
 * _elastic_fit: crystal s has its points in strain [s][0 .. P_s)[6] and stress [s][0 .. P_s)[3][3] of rows of `ld` points, P_s =
 * n_points[s] (NULL: ld); 7 <= ld <= 64.  strain is the applied small strain in Voigt order xx, yy, zz, yz, xz, xy with
 * engineering shear (gamma = 2 eps); the Voigt stress is taken from the 3 x 3 one, its off-diagonals the mean of the two stored
 * halves.  One wavefront per crystal, one lane per point: least squares of sigma_i = sigma0_i + sum_j C_ij eps_j, the columns
 * scaled by w = max |eps|, one 7 x 7 Cholesky factorisation and six solves.  Writes c_raw [s][6][6] (the fit), c [s][6][6] =
 * (c_raw + c_raw^T) / 2, compliance [s][6][6] = c^-1 (a 6 x 6 Cholesky), sigma0 [s][6], moduli [s][9] = (K_V, K_R, K_H, G_V,
 * G_R, G_H, E, nu, A_U) in the Voigt-Reuss-Hill form, rms [s] (root mean square residual of the 6 P_s stress values),
 * asymmetry [s] = max |c_raw - c_raw^T| / max |c_raw| and status [s]: 0 fitted and c positive definite (Born stable); 1 fitted,
 * c not positive definite: compliance and every modulus but K_V and G_V are NaN; 2 no fit (P_s < 7 or > ld, a non-finite
 * input, no non-zero strain, a rank-deficient strain set): every float output is NaN.
 * ------------------------------------------------------------------------------------------ */
int alignn_elastic_fit(const double* strain, const double* stress, const int32_t* n_points, int n_structures, int ld,
                       double* c_raw, double* c, double* compliance, double* sigma0, double* moduli, double* rms,
                       double* asymmetry, int32_t* status, alignn_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * The interface task (csrc/interface.hip; alignn_amd/interface.py is the driver, tests/interface_ref.py the numpy restatement,
 * INTEGRATION.md the specification).  float64 without contraction, no atomics, min / max and a total order on the match keys
 * only: a pair's bits do not depend on the launch it is in.
 *
 * _zsl_match: pair p has the surface cells film_cells [p][2][2] and subs_cells [p][2][2] (rows v1, v2 in the plane, v1 x v2 > 0)
 * and the largest multiples nmax_film [p], nmax_subs [p] <= max_film, max_subs <= 256 of its two sides (n area <= max_area; the
 * host's).  hnf [.][3] = (n, a, b) lists the Hermite normal forms [[a, b], [0, n / a]] of every n <= 256 in the order (n, a, b),
 * prefix [258]: prefix [n] (n = 1 .. 257) the first entry of multiple n ([0] is not read), so that hnf has prefix [257] rows.  film_off
 * and subs_off are [n_pairs].  Workspaces (written and read by the launch; what they hold afterwards is not part of the
 * result): film_tab [film_rows][4], film_int [film_rows][4],
 * subs_tab [subs_rows][6][4], subs_int [subs_rows][4] with pair p's prefix [nmax + 1] rows from film_off [p] / subs_off [p], and
 * best_score, best_tag [n_pairs][max_film].  Every super-lattice u = a v1 + b v2, w = (n / a) v2 is Lagrange-reduced keeping its
 * orientation ((u, w) <- (w, -u) while |u| > |w|, w <- w - rint(u.w / u.u) u, at most 64 rounds); a film basis is compared with
 * the six variants (u, w), (u, w + u), (u, w - u), (w, -u), (w, -u + w), (w, -u - w) of a substrate basis where
 * |i A_f / (j A_s) - 1| <= max_area_ratio_tol, and accepted where ru = | |u_s| / |u_f| - 1 | <= ltol, rw likewise and
 * cos(dtheta) >= cos_atol; score = max(ru, rw, |sin(dtheta)|).  Of the accepted candidates the one with the smallest key (i,
 * score, j, film entry, substrate entry, variant) gives status [p] = 0, multiples [p][2] = (i, j), film_matrix [p][2][2] and
 * subs_matrix [p][2][2] (rows u, w in units of v1, v2; dets i and j) and mismatch [p][4] = (ru, rw, sin(dtheta), score).
 * status 1: no candidate was accepted; status 2: a cell is not finite or v1 x v2 is not > 0.  With status != 0 nothing else is
 * written for the pair.
 *
 * _interface_build: the slabs are alignn_slab_build's with vacuum 0 (slab_cells [n_slabs][3][3], rows slab_off [k] ..
 * slab_off [k + 1] of slab_cart and slab_src).  jobs [n_pairs][10] = (film slab, substrate slab, film matrix [4], substrate
 * matrix [4]); pair p writes three structures in one cell, cells [3 p + (0, 1, 2)] of cells [3 n_pairs][3][3], rows out_off [3 p +
 * k] .. out_off [3 p + k + 1] (out_off [3 n_pairs + 1]; the row arrays have out_off [3 n_pairs] rows) of cart, frac (wrapped
 * into [0, 1)), src (slab_src of the slab row) and part (0 substrate, 1 film): the substrate's j n_s
 * rows, the film's i n_f rows, then both (substrate first).  Cell: A0 = (|u_s|, 0, 0), A1 = (u_s.w_s, u_s x w_s, 0) / |u_s|, A2 =
 * (0, 0, Lz), u_s and w_s the substrate's super-cell vectors in the plane of its slab (x along the slab's row 0).  A slab atom
 * with fractions f, image (m0, m1), m0 < a, m1 < det / a, a = gcd(M00, M10), row (m0 det / a + m1) n + atom, sits at the
 * in-plane fractions g = (f0 + m0, f1 + m1) M^-1, g -= floor(g + 1e-10), of (A0, A1) - the film strained onto the substrate's
 * cell - and at the height h = f2 |a3| of its slab: z = h - min_s h for the substrate, z = ((h - min_f h) + max_s z) +
 * separation [p] for the film, Lz = max_f z + vacuum [p].  area [p] = |A0 x A1|.  A pair whose slab indices, dets (1 .. 256) or
 * row ranges do not fit writes nothing.
 * ------------------------------------------------------------------------------------------ */
int alignn_zsl_match(const double* film_cells, const double* subs_cells, int n_pairs, const int32_t* nmax_film,
                     const int32_t* nmax_subs, int max_film, int max_subs, const int32_t* hnf, const int32_t* prefix,
                     const int64_t* film_off, const int64_t* subs_off, int64_t film_rows, int64_t subs_rows, double* film_tab,
                     int32_t* film_int, double* subs_tab, int32_t* subs_int, double* best_score, int64_t* best_tag,
                     double max_area_ratio_tol, double ltol, double cos_atol, int32_t* status, int32_t* multiples,
                     int32_t* film_matrix, int32_t* subs_matrix, double* mismatch, alignn_stream_t stream);
int alignn_interface_build(const double* slab_cells, const double* slab_cart, const int64_t* slab_off, const int32_t* slab_src,
                           int n_slabs, const int32_t* jobs, const double* separation, const double* vacuum,
                           const int64_t* out_off, int n_pairs, double* cells, double* cart, double* frac, int32_t* src,
                           int32_t* part, double* area, alignn_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* ALIGNN_HIP_H */
