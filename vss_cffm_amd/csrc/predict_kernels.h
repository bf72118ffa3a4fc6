// predict_kernels.h -- evaluation's tail without the full-resolution logits: two-stage bilinear resize + (soft-max) + flip + arg-max.
// Reference (segmentors/encoder_decoder.py:367-378, 502-572): the [B,K,h,w] logits of the head are resized to the network input size
// (Hm, Wm), resized again to ori_shape (H, W) (both bilinear, align_corners=False), soft-maxed over K, optionally flipped and arg-maxed:
// three [B,K,H,W] fp32 tensors (205 MB each at VSPW's 124 x 480 x 853) for 12.8 MB in and 3.3 MB out.
// Here, as in k_upce_fwd (segloss_kernels.h), the resized logits exist only in registers: a workgroup stages the low-resolution
// footprint of its 16 x 16 output pixels in LDS as [cell][class], every thread interpolates the K logits of its pixel from it and
// keeps the running maximum.  The arg-max is taken over the interpolated LOGITS (no exponential): the soft-max is monotone, so it is
// the reference's arg-max wherever two classes are further apart than rounding.
//
// Both stages folded per axis: stage 2 taps two neighbouring stage-1 rows m0, m1 (weights 1 - l2, l2), each of them taps two source rows;
// stage 1 never shrinks (Hm >= h), so the second one's rows start at most one row below the first one's and the (up to) four source
// rows lie in a0 .. a0 + 2.  A pixel therefore has composite weights wy[3] x wx[3] over a 3 x 3 neighbourhood -- one rounding per tap
// away from the nested form, the licence upce_interp4 takes -- and when a stage-2 axis is the identity (l2 = 0 for every pixel) the
// weights ARE stage 1's and the third row / column is not read at all (NY / NX = 2).
#pragma once
#include "cffm_common.h"
#include "gemm_kernels.h"      // xcd_linear_id
#include "segfuse_kernels.h"   // segf_taps: the bilinear tap rule (ATen's, in fp32)
#include "segloss_kernels.h"   // UPCE_KP, upce_max3, UPCE_ROWS_KPER

#define PRED_TILE 16             // output pixels per workgroup side
#define PRED_MAX_RATIO 8         // stage 1: Hm / h, Wm / w in 1 .. 8; stage 2: H / Hm, W / Wm in 0.5 .. 2
#define PRED_LDS_FLOATS 16384    // the LDS tile: rn * cn cells x KC classes (64 KB: two workgroups per CU at the worst)

struct PredGeom {
    int M, K, h, w, Hm, Wm, H, W;
    int flip;                    // 0 none, 1 horizontal, 2 vertical: the OUTPUT is flipped (encoder_decoder.py:543-550)
    int accumulate;              // probs += instead of =
    int rn, cn;                  // rows / columns of the low-resolution LDS tile
    int KC, nchunk;              // classes per LDS tile (a multiple of 4) and class chunks per tile: 1 unless the footprint is large
    long ms_outer, ms_inner;     // the logits' layout: UpceGeom's descriptor (segloss_kernels.h)
    int inner, ks, ps;
};

// first source row of output index dst under both stages
__device__ __forceinline__ int pred_first(int dst, int in, int mid, int out) {
    int m0, m1, a0, a1;
    float l;
    segf_taps(dst, mid, out, m0, m1, l);
    segf_taps(m0, in, mid, a0, a1, l);
    return a0;
}
// composite taps of output index dst along one axis: weights w0, w1 (, w2) of the source rows i0, i0 + 1 (, i0 + 2)
template <int N>
__device__ __forceinline__ void pred_axis(int dst, int in, int mid, int out, int& i0, float& w0, float& w1, float& w2) {
    int m0, m1, a0, a1;
    float l2, la;
    segf_taps(dst, mid, out, m0, m1, l2);
    segf_taps(m0, in, mid, a0, a1, la);
    i0 = a0;
    const float h2 = 1.f - l2, v0 = h2 * (1.f - la), v1 = h2 * la;
    w0 = v0 + (a1 == a0 ? v1 : 0.f);
    w1 = a1 == a0 ? 0.f : v1;
    w2 = 0.f;
    if (N == 3) {
        int b0, b1;
        float lb;
        segf_taps(m1, in, mid, b0, b1, lb);
        const int p0 = b0 - a0, p1 = b1 - a0;
        const float u0 = l2 * (1.f - lb), u1 = l2 * lb;
        w0 += (p0 == 0 ? u0 : 0.f) + (p1 == 0 ? u1 : 0.f);
        w1 += (p0 == 1 ? u0 : 0.f) + (p1 == 1 ? u1 : 0.f);
        w2 += (p0 == 2 ? u0 : 0.f) + (p1 == 2 ? u1 : 0.f);
    }
}
// four classes of one interpolated pixel: explicit FMAs in a fixed order, so that every evaluation of a group gives the same bits
template <int NY, int NX>
__device__ __forceinline__ f32x4 pred_interp4(const float* s_l, const int (&off)[NY * NX], const float (&wt)[NY * NX], int k4) {
    f32x4 acc = ((const f32x4*)(s_l + off[0]))[k4] * wt[0];
#pragma unroll
    for (int n = 1; n < NY * NX; ++n) {
        const f32x4 t = ((const f32x4*)(s_l + off[n]))[k4];
        const float wv = wt[n];
        acc = __builtin_elementwise_fma(t, (f32x4){wv, wv, wv, wv}, acc);
    }
    return acc;
}

// grid M * ceil(H/16) * ceil(W/16), 256 threads = 16 x 16 output pixels; dynamic LDS rn * cn * KC floats.
// pred[m][y][x] (int64, may be NULL when PROBS) = the lowest class index with the largest interpolated logit;
// PROBS: probs[m][k][y][x] (+)= softmax over the K interpolated logits (online maximum / sum in a first pass over the classes, the
// probabilities in a second one) -- the instantiation without it has neither the exponentials nor the second pass.
template <bool PROBS, int NY, int NX>
__global__ void __launch_bounds__(256) k_predict(const float* __restrict__ logits, long long* __restrict__ pred, float* __restrict__ probs,
                                                  PredGeom G) {
    CFFM_DYN_SMEM(smem);
    float* s_l = (float*)smem;
    // XCD-contiguous tile order, as in k_upce_fwd: the tiles that share lines of the low-resolution logits fill one L2
    const int gx = (G.W + PRED_TILE - 1) / PRED_TILE, gy = (G.H + PRED_TILE - 1) / PRED_TILE;
    const int lin = xcd_linear_id(), m = lin / (gx * gy), trem = lin - m * gx * gy;
    const int ty = (trem / gx) * PRED_TILE, tx = (trem - (trem / gx) * gx) * PRED_TILE;
    const int r0 = pred_first(ty, G.h, G.Hm, G.H), c0 = pred_first(tx, G.w, G.Wm, G.W);
    const int KP = UPCE_KP(G.K), KC = G.KC, cells = G.rn * G.cn;
    const int oy = ty + (threadIdx.x >> 4), ox = tx + (threadIdx.x & 15);
    const bool live = oy < G.H && ox < G.W;
    int off[NY * NX];          // tap (j, i) at j * NX + i
    float wt[NY * NX];
    {
        float wy0, wy1, wy2, wx0, wx1, wx2;
        int y0, x0;
        pred_axis<NY>(live ? oy : ty, G.h, G.Hm, G.H, y0, wy0, wy1, wy2);
        pred_axis<NX>(live ? ox : tx, G.w, G.Wm, G.W, x0, wx0, wx1, wx2);
#pragma unroll
        for (int j = 0; j < NY; ++j)
#pragma unroll
            for (int i = 0; i < NX; ++i) {
                // (the host sizes the tile from a bound on the span of any 16 pixels, so every weighted tap lies inside it; offsets past
                // a pixel's last tap carry weight 0 and the clamp only keeps their reads inside the tile)
                int rr = y0 - r0 + j, cc = x0 - c0 + i;
                rr = rr < 0 ? 0 : (rr > G.rn - 1 ? G.rn - 1 : rr);
                cc = cc < 0 ? 0 : (cc > G.cn - 1 ? G.cn - 1 : cc);
                off[j * NX + i] = (rr * G.cn + cc) * KC;
                wt[j * NX + i] = (j == 0 ? wy0 : j == 1 ? wy1 : wy2) * (i == 0 ? wx0 : i == 1 ? wx1 : wx2);
            }
    }
    // the output position: the reference flips the result, so pixel (y, x) holds what was computed for its mirror image
    const int py = G.flip == 2 ? G.H - 1 - oy : oy, px = G.flip == 1 ? G.W - 1 - ox : ox;
    const float* base = logits + (long)(m / G.inner) * G.ms_outer + (long)(m % G.inner) * G.ms_inner;
    float best = -3.0e38f, sum = 0.f, inv = 0.f;
    int arg = 0;
    for (int pass = 0; pass < (PROBS ? 2 : 1); ++pass) {
        for (int ch = 0; ch < G.nchunk; ++ch) {
            const int k0 = ch * KC, kc = KP - k0 < KC ? KP - k0 : KC;
            if (pass == 0 || G.nchunk > 1) {
                if (pass | ch) __syncthreads();
                // thread = (cell, class residue).  Token rows: 32 residues per cell, consecutive threads = consecutive classes (128-byte
                // runs).  [K][h][w] logits: consecutive threads = consecutive cells of one class (runs of cn floats), the classes spread
                // over 256 / cells groups of threads when the footprint has fewer than 256 cells.
                const bool rows = G.ps != 1;
                const int cw = cells >= 256 ? 256 : cells, kper = rows ? UPCE_ROWS_KPER : 256 / cw;
                const int kofs = rows ? threadIdx.x % kper : threadIdx.x / cw, rstep = rows ? 256 / kper : cw;
                const int rc0 = rows ? threadIdx.x / kper : (kofs < kper ? threadIdx.x - kofs * cw : cells);
                for (int rc = rc0; rc < cells; rc += rstep) {
                    const int r = rc / G.cn, c = rc - r * G.cn;
                    const int rr = r0 + r < G.h ? r0 + r : G.h - 1, cc = c0 + c < G.w ? c0 + c : G.w - 1;
                    const float* src = base + (long)(rr * G.w + cc) * G.ps + (long)k0 * G.ks;
                    float* dst = s_l + rc * KC;
                    for (int k = kofs; k < kc; k += kper) dst[k] = k0 + k < G.K ? src[(long)k * G.ks] : -1.0e30f;
                }
                __syncthreads();
            }
            if (!live) continue;
            if (pass == 0) {
                // running maximum with v_max3; only the GROUP that raised it is remembered, the class is recovered from that group
                // at the end of the tile (first occurrence: a later equal value does not raise the maximum)
                int grp = -1;
                for (int k4 = 0; k4 < kc / 4; ++k4) {
                    const f32x4 v = pred_interp4<NY, NX>(s_l, off, wt, k4);
                    const float nbest = upce_max3(upce_max3(best, v[0], v[1]), v[2], v[3]);
                    if (PROBS) {      // online soft-max: differences first (exact near the maximum), then one multiply in front of v_exp_f32
                        sum = sum * fast_exp2((best - nbest) * CFFM_LOG2E)
                            + ((fast_exp2((v[0] - nbest) * CFFM_LOG2E) + fast_exp2((v[1] - nbest) * CFFM_LOG2E))
                             + (fast_exp2((v[2] - nbest) * CFFM_LOG2E) + fast_exp2((v[3] - nbest) * CFFM_LOG2E)));
                    }
                    grp = nbest > best ? k4 : grp;
                    best = nbest;
                }
                if (grp >= 0) {
                    const f32x4 v = pred_interp4<NY, NX>(s_l, off, wt, grp);
                    arg = k0 + 4 * grp + (v[0] >= best ? 0 : v[1] >= best ? 1 : v[2] >= best ? 2 : 3);
                }
            } else {
                if (ch == 0) inv = 1.f / sum;
                float* out = probs + (((long)m * G.K + k0) * G.H + py) * G.W + px;
                const long plane = (long)G.H * G.W;
                for (int k4 = 0; k4 < kc / 4; ++k4) {
                    const f32x4 v = pred_interp4<NY, NX>(s_l, off, wt, k4);
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const int k = 4 * k4 + j;
                        if (k0 + k < G.K) {
                            const float p = fast_exp2((v[j] - best) * CFFM_LOG2E) * inv;
                            out[k * plane] = G.accumulate ? out[k * plane] + p : p;
                        }
                    }
                }
            }
        }
        if (pass == 0 && live && pred) pred[((long)m * G.H + py) * G.W + px] = (long long)arg;
    }
}
