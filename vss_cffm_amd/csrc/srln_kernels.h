// srln_kernels.h -- MiT's spatial-reduction convolution + LayerNorm on token rows, forward and backward, exact fp32 on the matrix pipe (gfx950).
//
// The reference (mix_transformer.py Attention.forward, sr_ratio > 1) takes the NCHW view of the token rows x [B, H W, C], runs
// Conv2d(C, C, kernel_size = s, stride = s), permutes back and applies LayerNorm(C).  Kernel = stride: the windows do not overlap, so on
// token rows this is ONE GEMM -- output row m = (b, oy, ox) is the s^2 input rows (oy s + ky, ox s + kx) of C floats each, times a
// [s^2 C, C] matrix -- with bias and LayerNorm as its epilogue.  Nothing is repacked: x is read where the previous layer left it, the weight
// in the Conv2d's own [co][ci][ky][kx] layout, and out / dx / dw are written in those layouts.  Rows y >= Ho s and columns x >= Wo s
// (Ho = H / s, Wo = W / s, rounded down) are never read; their dx is zero.  Kept for the backward: z (the rows before LayerNorm) and
// (mean, rstd) per row -- M = B Ho Wo rows, small.
//
// Arithmetic: every product is v_mfma_f32_16x16x4_f32 (mfma16x16x4_f32 of cffm_common.h), f32 operands and a chain of f32 fmaf.  The k-slots
// of an MFMA may stand for any four contraction indices as long as both operands agree, which is what lets every operand be read with
// 16-byte loads from the layout it already has: a lane's four k-steps are four consecutive ci of x (one position) against four
// weight rows ci .. ci + 3, whose s^2 positions are contiguous.  LayerNorm: mean, then the variance of the centred values held in
// registers, rstd = 1 / sqrtf (both correctly rounded).
//
//   k_srln_fwd       a workgroup of 8 waves owns 16 output rows and ALL C columns, NCW column tiles at a time.  The waves split K = s^2 C
//                    (a wave's share: every 8th (16-ci block, position group)), leave their partial tiles in LDS and the workgroup adds
//                    them in wave order; bias + LayerNorm read the finished rows from LDS, half a wave per row.
//   k_srln_bwd_rows  a wave per row: dz from dout, z, stats, gamma (to the workspace), and the row's share of the column sums dgamma,
//                    dbeta, db; a workgroup (16 rows) leaves its sums in a slab.  The same launch writes the zeros of dx's tail.
//   k_srln_colsum    adds the slabs in workgroup order.
//   k_srln_bwd_dx    dx = dz W^T: a wave owns 16 rows x 16 ci x 4 or 16 positions and walks all co; every result goes to exactly one
//                    input position (16-byte stores of 4 consecutive ci).
//   k_srln_bwd_dw    dw = dz^T x-patches: a workgroup of 8 waves owns a tile of 16 co x 16 ci x 4 positions, its waves walk the rows
//                    in 16-row steps (wave w: steps w, w + 8, ...) and the partial tiles are added in wave order through LDS.
// No atomics: two calls give the same bits.  Every workspace word that is read was written by the same call.
#pragma once
#include "cffm_common.h"
#include <math.h>

#define SRLN_MAXC 512    // widest row: 16 values per lane in the LayerNorm epilogue, 8 in the row pass
#define SRLN_WAVES 8     // waves of k_srln_fwd and k_srln_bwd_dw

struct SrGeom {
    int B, H, W, C, Ho, Wo, M;      // M = B Ho Wo
};

__device__ __forceinline__ f32x4 srln_zero() { return (f32x4){0.f, 0.f, 0.f, 0.f}; }

// first float of the window of output row m: x[b][(oy s) W + ox s][0]
__device__ __forceinline__ long srln_row_base(const SrGeom& G, int m, int s) {
    const int hw = G.Ho * G.Wo, b = m / hw, r = m - b * hw, oy = r / G.Wo, ox = r - oy * G.Wo;
    return (((long)b * G.H + (long)oy * s) * G.W + (long)ox * s) * G.C;
}

// grid (ceil(M / 16)); z and stats may be null
template <int S, int NCW>
__global__ void __launch_bounds__(512) k_srln_fwd(const float* __restrict__ x, const float* __restrict__ w, const float* __restrict__ bias,
                                                  const float* __restrict__ gamma, const float* __restrict__ beta, float* __restrict__ out,
                                                  float* __restrict__ z, float* __restrict__ stats, SrGeom G, float eps) {
    constexpr int S2 = S * S, P = S2 < 8 ? S2 : 8, NPASS = S2 / P, RW = NCW * 16 + 4;
    __shared__ f32x4 red4[SRLN_WAVES * 16 * RW / 4], zrow4[16 * (SRLN_MAXC + 4) / 4];
    float* red = (float*)red4;
    float* zrow = (float*)zrow4;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l15 = lane & 15, g = lane >> 4;
    const int C = G.C, ZS = C + 4;
    const long K = (long)S2 * C;
    const int nit = (C / 16) * NPASS;
    {
        const int m = blockIdx.x * 16 + l15;
        const bool live = m < G.M;
        const float* xrow = x + srln_row_base(G, live ? m : 0, S);
        for (int cg = 0; cg < C / (16 * NCW); ++cg) {
            f32x4 acc[NCW];
#pragma unroll
            for (int t = 0; t < NCW; ++t) acc[t] = srln_zero();
            for (int it = wave; it < nit; it += SRLN_WAVES) {
                const int cb = it / NPASS, ps = it - cb * NPASS, ci = cb * 16 + 4 * g;
                f32x4 xa[P];
#pragma unroll
                for (int j = 0; j < P; ++j) {
                    const int p = ps * P + j, ky = p / S, kx = p % S;
                    xa[j] = live ? *(const f32x4*)(xrow + ((long)ky * G.W + kx) * C + ci) : srln_zero();
                }
#pragma unroll
                for (int t = 0; t < NCW; ++t) {
                    const float* wp = w + (long)((cg * NCW + t) * 16 + l15) * K + (long)ci * S2 + ps * P;
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        f32x4 wv[P / 4];
#pragma unroll
                        for (int q = 0; q < P / 4; ++q) wv[q] = *(const f32x4*)(wp + e * S2 + 4 * q);
#pragma unroll
                        for (int j = 0; j < P; ++j) acc[t] = mfma16x16x4_f32(wv[j / 4][j % 4], xa[j][e], acc[t]);
                    }
                }
            }
            // register r of lane (l15, g) of tile t = row l15, column 16 t + 4 g + r of this column group
#pragma unroll
            for (int t = 0; t < NCW; ++t) *(f32x4*)(red + (wave * 16 + l15) * RW + 16 * t + 4 * g) = acc[t];
            __syncthreads();
            for (int i = tid; i < 16 * NCW * 4; i += 512) {
                const int r = i / (NCW * 4), c4 = i - r * (NCW * 4);
                f32x4 v = *(const f32x4*)(red + r * RW + 4 * c4);
                for (int wv = 1; wv < SRLN_WAVES; ++wv) v += *(const f32x4*)(red + (wv * 16 + r) * RW + 4 * c4);
                *(f32x4*)(zrow + r * ZS + cg * NCW * 16 + 4 * c4) = v;
            }
            __syncthreads();
        }
    }
    // bias + LayerNorm: 32 lanes per row, the row in registers
    const int r = tid >> 5, h = tid & 31, m = blockIdx.x * 16 + r;
    float v[SRLN_MAXC / 32];
    float sum = 0.f;
#pragma unroll
    for (int i = 0; i < SRLN_MAXC / 32; ++i) {
        const int c = h + 32 * i;
        v[i] = c < C ? zrow[r * ZS + c] + bias[c] : 0.f;
        sum += v[i];
    }
    for (int o = 16; o >= 1; o >>= 1) sum += __shfl_xor(sum, o, 64);
    const float mean = sum / (float)C;
    float sq = 0.f;
#pragma unroll
    for (int i = 0; i < SRLN_MAXC / 32; ++i) {
        const float d = h + 32 * i < C ? v[i] - mean : 0.f;
        sq = fmaf(d, d, sq);
    }
    for (int o = 16; o >= 1; o >>= 1) sq += __shfl_xor(sq, o, 64);
    const float rstd = 1.f / sqrtf(sq / (float)C + eps);
    if (m < G.M) {
#pragma unroll
        for (int i = 0; i < SRLN_MAXC / 32; ++i) {
            const int c = h + 32 * i;
            if (c < C) {
                if (z) z[(long)m * C + c] = v[i];
                out[(long)m * C + c] = (v[i] - mean) * rstd * gamma[c] + beta[c];
            }
        }
        if (stats && h == 0) {
            stats[2 * (long)m] = mean;
            stats[2 * (long)m + 1] = rstd;
        }
    }
}

// grid (ceil(M / 16)): dz [M][C]; part [gridDim.x][3][C] = this workgroup's sums of dout xhat, dout, dz; the tail of dx = 0
template <int S>
__global__ void __launch_bounds__(256) k_srln_bwd_rows(const float* __restrict__ z, const float* __restrict__ stats, const float* __restrict__ gamma,
                                                       const float* __restrict__ dout, float* __restrict__ dz, float* __restrict__ part,
                                                       float* __restrict__ dx, SrGeom G) {
    constexpr int NJ = SRLN_MAXC / 64;
    __shared__ float sums[4][3][SRLN_MAXC];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, C = G.C;
    float sg[NJ], sb[NJ], sd[NJ], gm[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        sg[j] = sb[j] = sd[j] = 0.f;
        gm[j] = lane + 64 * j < C ? gamma[lane + 64 * j] : 0.f;
    }
    for (int rr = 0; rr < 4; ++rr) {
        const int m = blockIdx.x * 16 + wave * 4 + rr;
        if (m >= G.M) break;                                       // (the whole wave)
        const float mean = stats[2 * (long)m], rstd = stats[2 * (long)m + 1];
        float xh[NJ], dy[NJ];
        float s1 = 0.f, s2 = 0.f;
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            const int c = lane + 64 * j;
            const bool in = c < C;
            const float dv = in ? dout[(long)m * C + c] : 0.f;
            xh[j] = in ? (z[(long)m * C + c] - mean) * rstd : 0.f;
            dy[j] = dv * gm[j];
            s1 += dy[j];
            s2 = fmaf(dy[j], xh[j], s2);
            sg[j] = fmaf(dv, xh[j], sg[j]);
            sb[j] += dv;
        }
        s1 = wave_sum(s1) / (float)C;
        s2 = wave_sum(s2) / (float)C;
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            const int c = lane + 64 * j;
            if (c < C) {
                const float d = rstd * (dy[j] - s1 - xh[j] * s2);
                dz[(long)m * C + c] = d;
                sd[j] += d;
            }
        }
    }
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        sums[wave][0][lane + 64 * j] = sg[j];
        sums[wave][1][lane + 64 * j] = sb[j];
        sums[wave][2][lane + 64 * j] = sd[j];
    }
    __syncthreads();
    for (int i = tid; i < 3 * C; i += 256) {
        const int which = i / C, c = i - which * C;
        part[(long)blockIdx.x * 3 * C + i] = ((sums[0][which][c] + sums[1][which][c]) + sums[2][which][c]) + sums[3][which][c];
    }
    // rows y >= Ho s (tb positions per image, contiguous) and columns x >= Wo s of the rows above (tr positions)
    const int Hs = G.Ho * S, Ws = G.Wo * S, tb = (G.H - Hs) * G.W, tr = Hs * (G.W - Ws), tpi = tb + tr, C4 = C / 4;
    if (tpi == 0) return;
    const long units = (long)G.B * tpi * C4;
    for (long u = (long)blockIdx.x * 256 + tid; u < units; u += (long)gridDim.x * 256) {
        const long pos = u / C4;
        const int c4 = (int)(u - pos * C4), b = (int)(pos / tpi);
        int q = (int)(pos - (long)b * tpi), y, xx;
        if (q < tb) {
            y = Hs + q / G.W;
            xx = q % G.W;
        } else {
            q -= tb;
            y = q / (G.W - Ws);
            xx = Ws + q % (G.W - Ws);
        }
        *(f32x4*)(dx + (((long)b * G.H + y) * G.W + xx) * C + 4 * c4) = srln_zero();
    }
}

// dgamma | dbeta | db [C] = the slabs added in workgroup order; grid (ceil(3 C / 256))
__global__ void __launch_bounds__(256) k_srln_colsum(const float* __restrict__ part, float* __restrict__ dgamma, float* __restrict__ dbeta,
                                                     float* __restrict__ db, int nblk, int C) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= 3 * C) return;
    float v = part[i];
    for (int k = 1; k < nblk; ++k) v += part[(long)k * 3 * C + i];
    const int which = i / C, c = i - which * C;
    (which == 0 ? dgamma : which == 1 ? dbeta : db)[c] = v;
}

// a wave = (row tile, 16-ci block, group of PQ position quads); grid (ceil(units / 4)), units = ceil(M / 16) (C / 16) (s^2 / (4 PQ))
template <int S>
__global__ void __launch_bounds__(256) k_srln_bwd_dx(const float* __restrict__ dz, const float* __restrict__ w, float* __restrict__ dx, SrGeom G,
                                                     long units) {
    constexpr int S2 = S * S, PQ = S2 < 16 ? S2 / 4 : 4, NPG = S2 / (4 * PQ);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l15 = lane & 15, g = lane >> 4, C = G.C, ncb = C / 16;
    const long unit = (long)blockIdx.x * 4 + wave;
    if (unit >= units) return;                                     // (the whole wave; no barrier below)
    const int pg = (int)(unit % NPG), cib = (int)((unit / NPG) % ncb), mt = (int)(unit / ((long)NPG * ncb));
    const long K = (long)S2 * C;
    const int m = mt * 16 + l15;
    const bool live = m < G.M;
    const float* dzr = dz + (long)(live ? m : 0) * C;
    const float* wb = w + (long)(cib * 16 + l15) * S2 + pg * PQ * 4;
    f32x4 acc[PQ][4];
#pragma unroll
    for (int q = 0; q < PQ; ++q)
#pragma unroll
        for (int t = 0; t < 4; ++t) acc[q][t] = srln_zero();
    for (int co0 = 0; co0 < C; co0 += 16) {
        const f32x4 dv = live ? *(const f32x4*)(dzr + co0 + 4 * g) : srln_zero();
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float* wp = wb + (long)(co0 + 4 * g + e) * K;
#pragma unroll
            for (int q = 0; q < PQ; ++q) {
                const f32x4 wv = *(const f32x4*)(wp + 4 * q);
#pragma unroll
                for (int t = 0; t < 4; ++t) acc[q][t] = mfma16x16x4_f32(wv[t], dv[e], acc[q][t]);
            }
        }
    }
    if (live) {
        // register r of lane (l15, g) of tile (q, t) = row l15, position 4 (pg PQ + q) + t, ci 16 cib + 4 g + r
        float* o = dx + srln_row_base(G, m, S) + cib * 16 + 4 * g;
#pragma unroll
        for (int q = 0; q < PQ; ++q)
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const int p = (pg * PQ + q) * 4 + t, ky = p / S, kx = p % S;
                *(f32x4*)(o + ((long)ky * G.W + kx) * C) = acc[q][t];
            }
    }
}

// a workgroup = 16 co x 16 ci x 4 positions of dw; grid (s^2 / 4, C / 16, C / 16)
template <int S>
__global__ void __launch_bounds__(512) k_srln_bwd_dw(const float* __restrict__ dz, const float* __restrict__ x, float* __restrict__ dw, SrGeom G) {
    constexpr int S2 = S * S;
    __shared__ f32x4 red4[SRLN_WAVES * 4 * 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l15 = lane & 15, g = lane >> 4, C = G.C;
    const int pq = blockIdx.x, cib = blockIdx.y, cob = blockIdx.z;
    const int ntile = (G.M + 15) / 16;
    f32x4 acc[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[j] = srln_zero();
    for (int it = wave; it < ntile; it += SRLN_WAVES) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int m = it * 16 + 4 * g + e;
            const bool live = m < G.M;
            const float* xr = x + srln_row_base(G, live ? m : 0, S) + cib * 16 + l15;
            const float a = live ? dz[(long)m * C + cob * 16 + l15] : 0.f;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int p = pq * 4 + j, ky = p / S, kx = p % S;
                const float xb = live ? xr[((long)ky * G.W + kx) * C] : 0.f;
                acc[j] = mfma16x16x4_f32(a, xb, acc[j]);
            }
        }
    }
    // register r of lane (l15, g) of tile j = co 16 cob + 4 g + r, ci 16 cib + l15, position 4 pq + j: the four j are one 16-byte piece of dw
#pragma unroll
    for (int r = 0; r < 4; ++r) red4[(wave * 4 + r) * 64 + lane] = (f32x4){acc[0][r], acc[1][r], acc[2][r], acc[3][r]};
    __syncthreads();
    if (tid < 256) {
        const int r = tid >> 6, ln = tid & 63;
        f32x4 v = red4[r * 64 + ln];
        for (int wv = 1; wv < SRLN_WAVES; ++wv) v += red4[(wv * 4 + r) * 64 + ln];
        const int co = cob * 16 + 4 * (ln >> 4) + r, ci = cib * 16 + (ln & 15);
        *(f32x4*)(dw + ((long)co * C + ci) * S2 + 4 * pq) = v;
    }
}
