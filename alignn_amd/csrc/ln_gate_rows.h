// Row arithmetic of the LayerNorm(+SiLU) and gate reverse passes, per lane and float4, on values and on duals (value +
// directional derivative): the ONE copy of what norm.hip (ln_silu_bwd), dual.hip (ln_silu_dual_bwd, egc_dual_bwd_dst,
// egc_dual_bwd_lg_dense) and convln.hip (the four reverse kernels with the LayerNorm inside) compute between their wave
// reductions.  The reductions themselves stay with the kernels - wave_sum in norm.hip / dual.hip, wave_sum_dpp in convln.hip,
// the partial sums of NC feature panels added first in the multi-panel kernels - and so does what a kernel does with a row
// before and after (loads, stores, amax, the segment and source sums).
//
// The functions fix the expression forms: outputs are bit for bit those of the bodies these replace.  A partial sum that
// the kernels accumulate component by component (x, y, z, w) is added into a reference argument in that order; one they
// take as hsum4 of a quad is returned as that hsum4.  Do not trade one form for the other, and do not merge two functions
// whose formulas look alike.  Which product of a sum the compiler contracts into an FMA depends on the operand order it
// settles on, and that can differ between a body written in the kernel and the same body inlined from a function: one formula
// (ALIGNN_GATE_DUAL_BWD) is a macro for that reason.  After a change here, compare every output with the previous build's.
//
// For the three files built with -fno-slp-vectorize only (alignn_amd/build.py EXTRA_FLAGS).  conv.hip is
// built WITH SLP vectorisation and does not include this header: its edge_grad remains the second copy of gate_bwd below.
#pragma once
#include "common.h"

// x-hat = (x - mean) rstd
__device__ __forceinline__ float4 ln_xhat(float4 x, float mean, float rstd) {
    return make_float4((x.x - mean) * rstd, (x.y - mean) * rstd, (x.z - mean) * rstd, (x.w - mean) * rstd);
}

// ---------------------------------------------------------------------------------------------------------------------
// LayerNorm + SiLU adjoint on values: y = silu(gamma x-hat + beta)
// ---------------------------------------------------------------------------------------------------------------------
// stage 1: x-hat and gh = gamma gz (gz: the adjoint of z); gz joins the parameter gradients db (dbeta), dg (dgamma); s1, s2:
// this quad's part of the row sums of gh and gh x-hat
__device__ __forceinline__ void ln_bwd_gh(float4 x, float4 gy, float mean, float rstd, float4 g, float4 b, float4& xh, float4& gh,
                                          float4& db, float4& dg, float& s1, float& s2) {
    xh = ln_xhat(x, mean, rstd);
    const float4 z = f4_fma(xh, g, b);
    const float4 gz = make_float4(gy.x * dsilu_f(z.x), gy.y * dsilu_f(z.y), gy.z * dsilu_f(z.z), gy.w * dsilu_f(z.w));
    db = f4_add(db, gz);
    dg = f4_fma(gz, xh, dg);
    gh = f4_mul(gz, g);
    s1 = hsum4(gh);
    s2 = hsum4(f4_mul(gh, xh));
}
// stage 2: the adjoint of x, with c1 = mean(gh), c2 = mean(gh x-hat) of the row
__device__ __forceinline__ float4 ln_bwd_gx(float4 gh, float4 xh, float rstd, float c1, float c2) {
    float4 o;
    o.x = rstd * (gh.x - c1 - xh.x * c2);
    o.y = rstd * (gh.y - c1 - xh.y * c2);
    o.z = rstd * (gh.z - c1 - xh.z * c2);
    o.w = rstd * (gh.w - c1 - xh.w * c2);
    return o;
}

// ---------------------------------------------------------------------------------------------------------------------
// LayerNorm + SiLU adjoint on duals (x, t = x-dot): t-hat = rstd (t - m1 - x-hat m2), m1 = mean(t), m2 = mean(x-hat t)
// ---------------------------------------------------------------------------------------------------------------------
// stage 0: x-hat; st, sxt: this quad's part of the row sums of t and x-hat t
__device__ __forceinline__ void ln_dual_bwd_xhat(float4 x, float4 t, float mean, float rstd, float4& xh, float& st, float& sxt) {
    xh = ln_xhat(x, mean, rstd);
    st = hsum4(t);
    sxt = hsum4(f4_mul(xh, t));
}
// stage 1, one component: a = adjoint of t-hat, b = direct adjoint of x-hat; the adjoints of z join db, dg; a, a x-hat, a t-hat
// are added to the row sums sa, sax, sat
__device__ __forceinline__ void ln_dual_bwd_ab1(float xh, float t, float gy, float gyt, float rstd, float m1, float m2, float g,
                                                float be, float& a, float& b, float& db, float& dg, float& sa, float& sax,
                                                float& sat) {
    const float th = rstd * (t - m1 - xh * m2);
    const float z = fmaf(xh, g, be), zt = g * th;
    float d1, d2;
    dsilu2(z, d1, d2);
    const float gzt = gyt * d1;                // adjoint of z-dot
    const float gz = gy * d1 + gyt * d2 * zt;  // adjoint of z
    db += gz;
    dg += gz * xh + gzt * th;
    a = g * gzt;
    b = g * gz;
    sa += a;
    sax += a * xh;
    sat += a * th;
}
__device__ __forceinline__ void ln_dual_bwd_ab(float4 xh, float4 t, float4 gy, float4 gyt, float rstd, float m1, float m2, float4 g,
                                               float4 be, float4& a, float4& b, float4& db, float4& dg, float& sa, float& sax,
                                               float& sat) {
    ln_dual_bwd_ab1(xh.x, t.x, gy.x, gyt.x, rstd, m1, m2, g.x, be.x, a.x, b.x, db.x, dg.x, sa, sax, sat);
    ln_dual_bwd_ab1(xh.y, t.y, gy.y, gyt.y, rstd, m1, m2, g.y, be.y, a.y, b.y, db.y, dg.y, sa, sax, sat);
    ln_dual_bwd_ab1(xh.z, t.z, gy.z, gyt.z, rstd, m1, m2, g.z, be.z, a.z, b.z, db.z, dg.z, sa, sax, sat);
    ln_dual_bwd_ab1(xh.w, t.w, gy.w, gyt.w, rstd, m1, m2, g.w, be.w, a.w, b.w, db.w, dg.w, sa, sax, sat);
}
// stage 2: b becomes the total adjoint of x-hat, direct part - rstd (a m2 + t A2), A2 = mean(a x-hat); sb, sbx: this quad's part
// of the row sums of b and b x-hat
__device__ __forceinline__ void ln_dual_bwd_b(float4 a, float4 t, float4 xh, float rstd, float m2, float A2, float4& b, float& sb,
                                              float& sbx) {
    b.x -= rstd * (a.x * m2 + t.x * A2);
    b.y -= rstd * (a.y * m2 + t.y * A2);
    b.z -= rstd * (a.z * m2 + t.z * A2);
    b.w -= rstd * (a.w * m2 + t.w * A2);
    sb = hsum4(b);
    sbx = hsum4(f4_mul(b, xh));
}
// stage 3: the adjoints gx of x and gxt of t; A1 = mean(a), A3 = mean(a t-hat), B1 = mean(b), B2 = mean(b x-hat)
__device__ __forceinline__ void ln_dual_bwd_gx(float4 a, float4 b, float4 xh, float rstd, float A1, float A2, float A3, float B1,
                                               float B2, float4& gx, float4& gxt) {
#define ALIGNN_LN_DUAL_O(q)                   \
    gxt.q = rstd * (a.q - A1 - xh.q * A2);    \
    gx.q = rstd * (b.q - B1 - xh.q * B2) - rstd * xh.q * A3;
    ALIGNN_LN_DUAL_O(x) ALIGNN_LN_DUAL_O(y) ALIGNN_LN_DUAL_O(z) ALIGNN_LN_DUAL_O(w)
#undef ALIGNN_LN_DUAL_O
}

// ---------------------------------------------------------------------------------------------------------------------
// gate adjoint: S1 = sum sigma(m) Bh[u], S0 = sum sigma(m) over a destination's edges
// ---------------------------------------------------------------------------------------------------------------------
// values: the adjoint of m through sg = sigma(m), from the adjoints g1, g0 of the two segment sums (conv.hip: edge_grad)
__device__ __forceinline__ float4 gate_bwd(float4 sg, float4 g1, float4 g0, float4 bh) {
    const float4 gsig = f4_fma(g1, bh, g0);
    float4 gm;
    gm.x = gsig.x * sg.x * (1.0f - sg.x);
    gm.y = gsig.y * sg.y * (1.0f - sg.y);
    gm.z = gsig.z * sg.z * (1.0f - sg.z);
    gm.w = gsig.w * sg.w * (1.0f - sg.w);
    return gm;
}
// duals: the gate's part is ADDED to gm, gmt (the adjoints of m, mt from the edge LayerNorm branch, or zero) from the adjoints
// q1, q0, q1t, q0t of S1, S0, S1-dot, S0-dot.  SRC: this row's terms of the source-side sums g_Bh, g_Bh-dot are added to gbh, gbht
// too (the dense-block kernels, which keep them per source; egc_dual_bwd_src forms them otherwise).
// The body is a macro because the dense-block kernels must expand it in place: called as an inlined function there, the
// compiler orders the two products of the sum added to gm the other way round and contracts the other one into the FMA - GM
// changes in the last bit.  The destination-ordered kernels take it through the function below, which leaves theirs alone.
#define ALIGNN_GATE_DUAL_BWD_1(c, SRC, m, mt, bh, bht, q1, q0, q1t, q0t, gm, gmt, gbh, gbht) \
    {                                                                                        \
        const float sg = fast_sigmoid((m).c), sp = sg * (1.0f - sg);                          \
        const float gs = (q1).c * (bh).c + (q0).c + (q1t).c * (bht).c; /* adjoint of sigma */ \
        const float gst = (q1t).c * (bh).c + (q0t).c;                  /* adjoint of sigma-dot */ \
        (gm).c += gs * sp + gst * sp * (1.0f - 2.0f * sg) * (mt).c;                           \
        (gmt).c += gst * sp;                                                                 \
        if (SRC) {                                                                           \
            const float sgt = sp * (mt).c;                                                   \
            (gbh).c += sg * (q1).c + sgt * (q1t).c;                                           \
            (gbht).c += sg * (q1t).c;                                                        \
        }                                                                                    \
    }
#define ALIGNN_GATE_DUAL_BWD(...) \
    ALIGNN_GATE_DUAL_BWD_1(x, __VA_ARGS__) ALIGNN_GATE_DUAL_BWD_1(y, __VA_ARGS__) ALIGNN_GATE_DUAL_BWD_1(z, __VA_ARGS__) ALIGNN_GATE_DUAL_BWD_1(w, __VA_ARGS__)
__device__ __forceinline__ void gate_dual_bwd(float4 m, float4 mt, float4 bh, float4 bht, float4 q1, float4 q0, float4 q1t, float4 q0t,
                                              float4& gm, float4& gmt) {
    float4 none;  // (never touched)
    ALIGNN_GATE_DUAL_BWD(false, m, mt, bh, bht, q1, q0, q1t, q0t, gm, gmt, none, none)
}

// ---------------------------------------------------------------------------------------------------------------------
// one feature panel of the workgroup's LayerNorm parameter-gradient slab [2][F]: [0] = dbeta, [1] = dgamma, the W waves' sums
// in wave order.  Every thread of the workgroup must call it (barriers; the first one also guards an earlier use of sh).
// ---------------------------------------------------------------------------------------------------------------------
template <int W>
__device__ __forceinline__ void ln_slab_store(float4 db, float4 dg, float4 (*sh)[W][ALIGNN_WAVE], float* slab, int F, int f, bool active,
                                              int wave, int lane) {
    __syncthreads();
    sh[0][wave][lane] = db;
    sh[1][wave][lane] = dg;
    __syncthreads();
    if (wave == 0 && active) {
        float4 a = sh[0][0][lane], b = sh[1][0][lane];
#pragma unroll
        for (int w = 1; w < W; ++w) {
            a = f4_add(a, sh[0][w][lane]);
            b = f4_add(b, sh[1][w][lane]);
        }
        f4_st(slab + f, a);
        f4_st(slab + F + f, b);
    }
}
