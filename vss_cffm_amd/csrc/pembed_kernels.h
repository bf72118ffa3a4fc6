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
// The training forward is the same kernel with TRAIN = true (it also stores the pre-LayerNorm rows); the backward is the second half of
// this file.
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

// grid (ceil(B Ho tpr / NT)); Cout <= PEMB_MAXC / NT.  TRAIN: the pre-LayerNorm rows (convolution + bias, the values the epilogue reads from
// LDS) are stored to zout [B][Ho Wo][Cout] as well -- what the backward recomputes mean and rstd from; out has the same bits either way.
template <int KS, int ST, int NCW, int NT, int WAVES, bool TRAIN>
__global__ void __launch_bounds__(WAVES * 64) k_pembed_fwd(const float* __restrict__ x, const float* __restrict__ w, const float* __restrict__ bias,
                                                           const float* __restrict__ gamma, const float* __restrict__ beta,
                                                           float* __restrict__ out, float* __restrict__ zout, PembGeom G, float eps) {
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
        if (TRAIN && tile < ntile && ox < G.Wo) {
            float* zrow_p = zout + ((long)orow * G.Wo + ox) * Cout;
#pragma unroll
            for (int i = 0; i < NV; ++i)
                if (h + 32 * i < Cout) zrow_p[h + 32 * i] = v[i];
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

// ------------------------------------------------------------------------------------------------ backward
// dout [B][Ho Wo][Cout] -> dz (the LayerNorm backward of mitln_kernels.h on the saved rows z: k_ln_rows_bwd + k_ln_bwd_final, which also
// give dgamma and dbeta) -> dw, db and, for (3, 2), dx.  The same three-pass bf16 split as the forward, fp32 accumulation, no atomics, every
// sum in an order that follows from the shapes alone.
//
//   k_pembed_dw        dw[co][kk] = sum over the output pixels m of dz[m][co] patch(m; kk): both operands contract along m.  A workgroup of 4
//                      waves owns one SLAB of rows m (the M split, host: pemb_bwd_layout), 64 columns co and 64 patch columns kk; wave w
//                      takes the 16 kk of its own and all four co tiles.  Per step of 32 rows the dz tile goes through LDS, split into
//                      bf16 hi / lo once and transposed to [co][m] (80-byte rows: the 16 lanes of a ds_read_b128 touch 16 different
//                      16-byte slots), so a fragment -- 8 consecutive m of one co -- is one 16-byte read per part.  The patch operand is
//                      gathered as in the forward: a lane's kk = (ci, ky, kx) is fixed for the whole kernel, its 8 rows are consecutive
//                      output pixels; taps outside the image, kk >= K and rows past the slab are exact zeros.  The partial [Cout][KP] tile
//                      of slab s is written to the workspace (KP = K rounded up to 16; columns K.. are zeros nobody reads).
//   k_pembed_db        db[co] = sum over m of dz[m][co] in fp32: records [Cout] of at most PEMB_DB_CAP workgroups.
//   k_pembed_dw_final  adds the slabs in slab order -> dw in the Conv2d weight's own layout [Cout][K], and the db records in their order.
//   k_pembed_wt        wt[ky][kx][ci][co] = w[co][ci][ky][kx]: the input gradient contracts along co, which the weight has at stride K.
//   k_pembed_dx        (3, 2) only.  dx[b][ci][iy][ix] = sum over co and the taps with (iy + 1 - ky) and (ix + 1 - kx) even of
//                      dz[b][(iy + 1 - ky) / 2][(ix + 1 - kx) / 2][co] w[co][ci][ky][kx]: the gather form.  A workgroup owns 32 consecutive
//                      ix of one input row; waves 0 / 2 take the 16 even ix (kx = 1), waves 1 / 3 the 16 odd ones (kx = 0 and 2); the row's
//                      parity gives ky = 1 or ky = 0 and 2.  The two wave pairs take alternate groups of 64 ci; a group's tile goes
//                      through LDS so that both parities leave as one run of 32 floats per ci.  Output pixels outside the map contribute
//                      exact zeros, so a pixel no tap reaches is an exact zero.
#define PEMB_DW_ROWS 32          // rows of dz per contraction step of k_pembed_dw
#define PEMB_DW_SLAB_CAP 128     // slabs of the M split at most
#define PEMB_DW_WG_TARGET 512    // the split aims at this many workgroups (two per compute unit)
#define PEMB_DB_CAP 256          // db records at most
#define PEMB_DW_LDM 40           // bf16 per LDS row of the dz tile: 32 m + 8 pad

// grid (nslab, ceil(Cout / 64), ceil(KP / 64)), 256 threads; slab [nslab][Cout][KP]; RS = rows per slab
template <int KS, int ST>
__global__ void __launch_bounds__(256) k_pembed_dw(const float* __restrict__ x, const float* __restrict__ dz, float* __restrict__ slab,
                                                   PembGeom G, int RS, int KP) {
    constexpr int KK = KS * KS, PAD = KS / 2, LDM = PEMB_DW_LDM;
    __shared__ bf16x8 Th8[64 * LDM / 8], Tl8[64 * LDM / 8];
    bf16* Th = (bf16*)Th8;
    bf16* Tl = (bf16*)Tl8;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l15 = lane & 15, g = lane >> 4;
    const int Cout = G.Cout, K = G.K, M = G.B * G.Ho * G.Wo;
    const int s = blockIdx.x, co0 = blockIdx.y * 64, kk = blockIdx.z * 64 + wave * 16 + l15;
    const int m_begin = s * RS, m_end = m_begin + RS < M ? m_begin + RS : M;
    // this lane's column of the patch operand
    const int ci = kk / KK, rk = kk - ci * KK, ky = rk / KS, kx = rk - ky * KS;
    const bool klive = kk < K;
    f32x4 acc[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) acc[t] = (f32x4){0.f, 0.f, 0.f, 0.f};
    for (int m0 = m_begin; m0 < m_end; m0 += PEMB_DW_ROWS) {       // (uniform over the workgroup)
        for (int i = tid; i < PEMB_DW_ROWS * 16; i += 256) {
            const int mr = i >> 4, c4 = i & 15, m = m0 + mr, co = co0 + 4 * c4;
            const f32x4 v = (m < m_end && co < Cout) ? *(const f32x4*)(dz + (long)m * Cout + co) : (f32x4){0.f, 0.f, 0.f, 0.f};
            bf16x4 hi, lo;
            split4(v, hi, lo);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                Th[(4 * c4 + e) * LDM + mr] = hi[e];
                Tl[(4 * c4 + e) * LDM + mr] = lo[e];
            }
        }
        __syncthreads();
        const int m = m0 + 8 * g;
        int ox = m % G.Wo, oy = (m / G.Wo) % G.Ho, b = m / (G.Wo * G.Ho);
        f32x4 xv[2];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int iy = oy * ST - PAD + ky, ix = ox * ST - PAD + kx;
            const bool in = klive && m + j < m_end && (unsigned)iy < (unsigned)G.H && (unsigned)ix < (unsigned)G.W;
            xv[j >> 2][j & 3] = in ? x[(((long)b * G.Cin + ci) * G.H + iy) * G.W + ix] : 0.f;
            if (++ox == G.Wo) {
                ox = 0;
                if (++oy == G.Ho) { oy = 0; ++b; }
            }
        }
        bf16x8 xh, xl;
        pemb_split8(xv[0], xv[1], xh, xl);
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const bf16x8 ah = *(const bf16x8*)(Th + (16 * t + l15) * LDM + 8 * g), al = *(const bf16x8*)(Tl + (16 * t + l15) * LDM + 8 * g);
            acc[t] = mfma16x16x32_bf16(ah, xl, acc[t]);
            acc[t] = mfma16x16x32_bf16(al, xh, acc[t]);
            acc[t] = mfma16x16x32_bf16(ah, xh, acc[t]);
        }
        __syncthreads();
    }
    // register r of lane (l15, g) of tile t = row co0 + 16 t + 4 g + r, column kk
    if (kk < KP) {
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int co = co0 + 16 * t + 4 * g + r;
                if (co < Cout) slab[((long)s * Cout + co) * KP + kk] = acc[t][r];
            }
    }
}

// rec[blockIdx.x][Cout] = the sum of rows blockIdx.x RB .. + RB - 1 of dz[M][Cout].  256 threads = 256 / (Cout / 4) row groups x the row's
// 16-byte chunks; the row groups are added in their order through LDS.
__global__ void __launch_bounds__(256) k_pembed_db(const float* __restrict__ dz, float* __restrict__ rec, int M, int Cout, int RB) {
    __shared__ f32x4 S[256];
    const int C4 = Cout / 4, RG = 256 / C4, c4 = threadIdx.x % C4, rg = threadIdx.x / C4;
    const int r0 = blockIdx.x * RB, r1 = r0 + RB < M ? r0 + RB : M;
    f32x4 acc = (f32x4){0.f, 0.f, 0.f, 0.f};
    if (rg < RG)
        for (int r = r0 + rg; r < r1; r += RG) acc += *(const f32x4*)(dz + (long)r * Cout + 4 * c4);
    S[threadIdx.x] = acc;
    __syncthreads();
    if ((int)threadIdx.x < C4) {
        f32x4 v = S[threadIdx.x];
        for (int q = 1; q < RG; ++q) v += S[q * C4 + threadIdx.x];
        *(f32x4*)(rec + (long)blockIdx.x * Cout + 4 * threadIdx.x) = v;
    }
}

// one 16-byte chunk per lane: chunks 0 .. Cout KP / 4 - 1 are dw (the slabs added in slab order), the Cout / 4 behind them db (the
// records added in their order).  grid = ceil((Cout KP / 4 + Cout / 4) / 256).
__global__ void __launch_bounds__(256) k_pembed_dw_final(const float* __restrict__ slab, const float* __restrict__ dbrec, float* __restrict__ dw,
                                                         float* __restrict__ db, int nslab, int ndb, int Cout, int K, int KP) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x, nw = (long)Cout * KP / 4;
    f32x4 acc = (f32x4){0.f, 0.f, 0.f, 0.f};
    if (i < nw) {
        const int co = (int)(i / (KP / 4)), k0 = 4 * (int)(i % (KP / 4));
#pragma unroll 8
        for (int s = 0; s < nslab; ++s) acc += *(const f32x4*)(slab + ((long)s * Cout + co) * KP + k0);
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (k0 + e < K) dw[(long)co * K + k0 + e] = acc[e];
    } else if (i < nw + Cout / 4) {
        const int c0 = 4 * (int)(i - nw);
#pragma unroll 8
        for (int r = 0; r < ndb; ++r) acc += *(const f32x4*)(dbrec + (long)r * Cout + c0);
        *(f32x4*)(db + c0) = acc;
    }
}

// wt[tap][ci][co] = w[co][ci][tap], tap = 3 ky + kx.  grid = ceil(9 Cin Cout / 256)
__global__ void __launch_bounds__(256) k_pembed_wt(const float* __restrict__ w, float* __restrict__ wt, int Cin, int Cout) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= 9L * Cin * Cout) return;
    const int co = (int)(i % Cout), ci = (int)(i / Cout % Cin), tap = (int)(i / Cout / Cin);
    wt[i] = w[((long)co * Cin + ci) * 9 + tap];
}

#define PEMB_DX_LDX 36           // floats per LDS row of the dx tile: 32 ix + 4 pad
// grid = B H ceil(W / 32) (segment fastest), 256 threads
__global__ void __launch_bounds__(256) k_pembed_dx(const float* __restrict__ dz, const float* __restrict__ wt, float* __restrict__ dx, PembGeom G) {
    constexpr int LDX = PEMB_DX_LDX;
    __shared__ f32x4 T4[2 * 64 * LDX / 4];
    float* T = (float*)T4;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l15 = lane & 15, g = lane >> 4;
    const int px = wave & 1, wp = wave >> 1;
    const int Cin = G.Cin, Cout = G.Cout, nseg = (G.W + 31) / 32;
    const int ix0 = (blockIdx.x % nseg) * 32, iy = (blockIdx.x / nseg) % G.H, b = blockIdx.x / nseg / G.H;
    const int ix = ix0 + 2 * l15 + px;
    const int ncg = (Cin + 63) / 64;                                // groups of 64 ci
    const int nky = (iy & 1) ? 2 : 1, ky0 = (iy & 1) ? 0 : 1, nkx = px ? 2 : 1, kx0 = px ? 0 : 1;
    for (int cg0 = 0; cg0 < ncg; cg0 += 2) {                        // (uniform over the workgroup)
        const int cg = cg0 + wp;
        f32x4 acc[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) acc[t] = (f32x4){0.f, 0.f, 0.f, 0.f};
        if (cg < ncg) {                                             // (uniform over the wave, as every condition around an MFMA below)
            for (int a = 0; a < nky; ++a) {
                const int ky = ky0 + 2 * a, oy = (iy + 1 - ky) / 2;
                if (oy >= G.Ho) continue;
                for (int c = 0; c < nkx; ++c) {
                    const int kx = kx0 + 2 * c, ox = (ix + 1 - kx) / 2;
                    const bool plive = ix < G.W && ox < G.Wo;
                    const float* zp = dz + (((long)b * G.Ho + oy) * G.Wo + (plive ? ox : 0)) * Cout;
                    const float* wtap = wt + (long)(ky * 3 + kx) * Cin * Cout;
                    for (int c0 = 0; c0 < Cout; c0 += 32) {
                        const int k0 = c0 + 8 * g;                  // (Cout is a multiple of 16: a chunk of 8 lies inside it or outside)
                        const bool kin = k0 < Cout;
                        f32x4 zv[2];
#pragma unroll
                        for (int q = 0; q < 2; ++q) zv[q] = (plive && kin) ? *(const f32x4*)(zp + k0 + 4 * q) : (f32x4){0.f, 0.f, 0.f, 0.f};
                        bf16x8 zh, zl;
                        pemb_split8(zv[0], zv[1], zh, zl);
#pragma unroll
                        for (int t = 0; t < 4; ++t) {
                            const int ci = (cg * 4 + t) * 16 + l15;
                            f32x4 wv[2];
#pragma unroll
                            for (int q = 0; q < 2; ++q)
                                wv[q] = (ci < Cin && kin) ? *(const f32x4*)(wtap + (long)ci * Cout + k0 + 4 * q) : (f32x4){0.f, 0.f, 0.f, 0.f};
                            bf16x8 wh, wl;
                            pemb_split8(wv[0], wv[1], wh, wl);
                            acc[t] = mfma16x16x32_bf16(wh, zl, acc[t]);
                            acc[t] = mfma16x16x32_bf16(wl, zh, acc[t]);
                            acc[t] = mfma16x16x32_bf16(wh, zh, acc[t]);
                        }
                    }
                }
            }
        }
        // register r of lane (l15, g) of tile t = channel 16 t + 4 g + r of the group, pixel ix0 + 2 l15 + px
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) T[(wp * 64 + 16 * t + 4 * g + r) * LDX + 2 * l15 + px] = acc[t][r];
        __syncthreads();
        for (int i = tid; i < 2 * 64 * 32; i += 256) {
            const int q = i >> 11, rr = (i >> 5) & 63, xx = i & 31, ci = (cg0 + q) * 64 + rr;
            if (ci < Cin && ix0 + xx < G.W) dx[(((long)b * Cin + ci) * G.H + iy) * G.W + ix0 + xx] = T[(q * 64 + rr) * LDX + xx];
        }
        __syncthreads();
    }
}
