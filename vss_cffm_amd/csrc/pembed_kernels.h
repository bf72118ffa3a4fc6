// pembed_kernels.h -- MiT's overlapping patch embedding (mix_transformer.py OverlapPatchEmbed.forward, eval mode) as one kernel (gfx950):
// Conv2d(Cin, Cout, k, stride, padding = k / 2) on an NCHW map, flatten(2).transpose(1, 2), LayerNorm(Cout) -> token rows [B, Ho Wo, Cout].
//
// A convolution with overlapping windows is a GEMM on gathered input patches: output row m = (b, oy, ox) is the K = Cin k^2 input values
// x[b][ci][oy s - p + ky][ox s - p + kx] (zero outside the image) times the [K, Cout] matrix the Conv2d weight [co][ci][ky][kx] already IS,
// read along its contiguous K.  Nothing is repacked: there is no im2col buffer, no copy of the weight and no NCHW copy of the result.
//
// Arithmetic: the three-pass bf16 split of the Linear GEMMs (gemm_kernels.h): every fp32 operand is split into bf16 hi + bf16 lo while it
// is staged (here: between the global load and the MFMA, in registers), and a product is hi.lo + lo.hi + hi.hi on
// v_mfma_f32_16x16x32_bf16 with fp32 accumulation.  k-slot j of lane group g of a k-step stands for contraction index 32 step + 8 g + j for
// both operands; indices >= K (K = 147 at stage 1) and taps outside the image are zeros in the fragment, so they contribute exactly zero.
//
//   k_pembed_fwd   a workgroup of WAVES waves owns NT tiles of 16 ADJACENT output pixels of ONE output row each (consecutive tiles in the
//                  order (b, oy, tx)) and ALL Cout columns, NCW column tiles at a time.  WAVES / NT waves share a tile and split its K (wave
//                  ks of a tile: k-steps ks, ks + WAVES / NT, ...); they leave their partial tiles in LDS and the workgroup adds them in
//                  wave order; bias + LayerNorm read the finished rows from LDS, half a wave per row (as k_srln_fwd).  The weight fragment
//                  of a (k-step, column tile) is loaded by one wave per tile, which is why it is not staged in LDS.
//                  The host picks NT by Cout (cffm_hip.hip pemb_go; WAVES = 8): narrow rows come with many output pixels and a short K
//                  (stage 1: 115,200 rows, K = 147 = 5 k-steps), so a wave takes a whole tile (NT = 8, no K split: 128 pixels per
//                  workgroup; NT = 4, two waves per tile, up to Cout = 128); wide rows come with few pixels and a long K (stage 4: 1800
//                  rows at B = 8, K = 2880 = 90 k-steps: 120 tiles for 256 compute units), so ONE tile is split over the 8 waves.  K split
//                  rather than finer row tiles there: every workgroup reads the whole weight whatever its rows, so finer tiles only
//                  multiply that traffic.  (Measured: 16 waves per tile change nothing at stage 4 and cost 15 % at stage 3 -- what bounds
//                  the wide shapes is the weight each compute unit pulls through its own L2 port, 5.9 MB at stage 4, not the loads in flight.)
// LayerNorm as mitln_kernels.h: mean first, the centred values re-centred once by their own mean, variance = mean(d^2), rstd = 1 / sqrtf.
// No atomics, a fixed summation order: two calls give the same bits.
#pragma once
#include "cffm_common.h"
#include "gemm_kernels.h"
#include <math.h>

#define PEMB_MAXC 512    // widest row: 16 values per lane in the LayerNorm epilogue; a workgroup with NT tiles takes rows up to 512 / NT

struct PembGeom {
    int B, Cin, H, W, Cout, Ho, Wo, K, tpr;      // K = Cin k^2; tpr = ceil(Wo / 16) tiles per output row
};

__device__ __forceinline__ void pemb_split8(f32x4 a, f32x4 b, bf16x8& hi, bf16x8& lo) {
    bf16x4 h0, l0, h1, l1;
    split4(a, h0, l0);
    split4(b, h1, l1);
    hi = __builtin_shufflevector(h0, h1, 0, 1, 2, 3, 4, 5, 6, 7);
    lo = __builtin_shufflevector(l0, l1, 0, 1, 2, 3, 4, 5, 6, 7);
}

// grid (ceil(B Ho tpr / NT)); Cout <= PEMB_MAXC / NT
template <int KS, int ST, int NCW, int NT, int WAVES>
__global__ void __launch_bounds__(WAVES * 64) k_pembed_fwd(const float* __restrict__ x, const float* __restrict__ w, const float* __restrict__ bias,
                                                           const float* __restrict__ gamma, const float* __restrict__ beta,
                                                           float* __restrict__ out, PembGeom G, float eps) {
    constexpr int KK = KS * KS, PAD = KS / 2, RW = NCW * 16 + 4, KSPLIT = WAVES / NT, ZC = PEMB_MAXC / NT, NV = ZC / 32;
    __shared__ f32x4 red4[WAVES * 16 * RW / 4], zrow4[NT * 16 * (ZC + 4) / 4];
    float* red = (float*)red4;
    float* zrow = (float*)zrow4;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l15 = lane & 15, g = lane >> 4;
    const int Cout = G.Cout, ZS = Cout + 4, K = G.K;
    const int ntile = G.B * G.Ho * G.tpr, tile0 = blockIdx.x * NT;
    const int nstep = (K + 31) / 32;
    {
        // this wave's tile and its share of K; this lane's pixel of the patch operand (a tile past the end computes zeros)
        const int tw = wave / KSPLIT, ks = wave - tw * KSPLIT, tile = tile0 + tw;
        const int tx = tile % G.tpr, orow = tile / G.tpr, oy = orow % G.Ho, b = orow / G.Ho;
        const int ox = tx * 16 + l15, iy0 = oy * ST - PAD, ix0 = ox * ST - PAD;
        const bool live = tile < ntile && ox < G.Wo;
        const float* xb = x + (long)(live ? b : 0) * G.Cin * G.H * G.W;
        for (int cg = 0; cg < Cout / (16 * NCW); ++cg) {
            f32x4 acc[NCW];
#pragma unroll
            for (int t = 0; t < NCW; ++t) acc[t] = (f32x4){0.f, 0.f, 0.f, 0.f};
            for (int step = ks; step < nstep; step += KSPLIT) {
                const int k0 = step * 32 + 8 * g;
                f32x4 xv[2];
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    const int kk = k0 + e, ci = kk / KK, r = kk - ci * KK, ky = r / KS, kx = r - ky * KS, iy = iy0 + ky, ix = ix0 + kx;
                    const bool in = live && kk < K && (unsigned)iy < (unsigned)G.H && (unsigned)ix < (unsigned)G.W;
                    xv[e >> 2][e & 3] = in ? xb[((long)ci * G.H + iy) * G.W + ix] : 0.f;
                }
                bf16x8 xh, xl;
                pemb_split8(xv[0], xv[1], xh, xl);
#pragma unroll
                for (int t = 0; t < NCW; ++t) {
                    const float* wp = w + (long)((cg * NCW + t) * 16 + l15) * K + k0;
                    f32x4 wv[2];
                    if (KS == 3) {          // K = 9 Cin, Cin a multiple of 4: rows and chunks are 16-byte aligned and lie inside K or outside it
#pragma unroll
                        for (int q = 0; q < 2; ++q) wv[q] = k0 + 4 * q < K ? *(const f32x4*)(wp + 4 * q) : (f32x4){0.f, 0.f, 0.f, 0.f};
                    } else {                // K = 49 Cin: rows start anywhere
#pragma unroll
                        for (int e = 0; e < 8; ++e) wv[e >> 2][e & 3] = k0 + e < K ? wp[e] : 0.f;
                    }
                    bf16x8 wh, wl;
                    pemb_split8(wv[0], wv[1], wh, wl);
                    acc[t] = mfma16x16x32_bf16(wh, xl, acc[t]);
                    acc[t] = mfma16x16x32_bf16(wl, xh, acc[t]);
                    acc[t] = mfma16x16x32_bf16(wh, xh, acc[t]);
                }
            }
            // register r of lane (l15, g) of tile t = pixel l15, column 16 t + 4 g + r of this column group
#pragma unroll
            for (int t = 0; t < NCW; ++t) *(f32x4*)(red + (wave * 16 + l15) * RW + 16 * t + 4 * g) = acc[t];
            __syncthreads();
            for (int i = tid; i < NT * 16 * NCW * 4; i += WAVES * 64) {
                const int r = i / (NCW * 4), c4 = i - r * (NCW * 4), rt = r >> 4, rp = r & 15;
                f32x4 v = *(const f32x4*)(red + (rt * KSPLIT * 16 + rp) * RW + 4 * c4);
                for (int wv = 1; wv < KSPLIT; ++wv) v += *(const f32x4*)(red + ((rt * KSPLIT + wv) * 16 + rp) * RW + 4 * c4);
                *(f32x4*)(zrow + r * ZS + cg * NCW * 16 + 4 * c4) = v;
            }
            __syncthreads();
        }
    }
    // bias + LayerNorm: 32 lanes per row, the row in registers (both halves of a wave make the same number of passes)
    const int h = tid & 31;
    const float n = (float)Cout;
    for (int r = tid >> 5; r < NT * 16; r += WAVES * 2) {
        const int tile = tile0 + (r >> 4), tx = tile % G.tpr, orow = tile / G.tpr, ox = tx * 16 + (r & 15);
        float v[NV];
        float sum = 0.f;
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            const int c = h + 32 * i;
            v[i] = c < Cout ? zrow[r * ZS + c] + bias[c] : 0.f;
            sum += v[i];
        }
        for (int o = 16; o >= 1; o >>= 1) sum += __shfl_xor(sum, o, 64);
        const float m0 = sum / n;
        sum = 0.f;
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            v[i] = h + 32 * i < Cout ? v[i] - m0 : 0.f;
            sum += v[i];
        }
        for (int o = 16; o >= 1; o >>= 1) sum += __shfl_xor(sum, o, 64);
        const float m1 = sum / n;
        float sq = 0.f;
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            v[i] = h + 32 * i < Cout ? v[i] - m1 : 0.f;
            sq = fmaf(v[i], v[i], sq);
        }
        for (int o = 16; o >= 1; o >>= 1) sq += __shfl_xor(sq, o, 64);
        const float rstd = 1.f / sqrtf(sq / n + eps);
        if (tile < ntile && ox < G.Wo) {
            float* orow_p = out + ((long)orow * G.Wo + ox) * Cout;
#pragma unroll
            for (int i = 0; i < NV; ++i) {
                const int c = h + 32 * i;
                if (c < Cout) orow_p[c] = v[i] * rstd * gamma[c] + beta[c];
            }
        }
    }
}
