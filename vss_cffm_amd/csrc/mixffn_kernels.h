// mixffn_kernels.h -- the middle of MiT's Mix-FFN on token rows: 3 x 3 depthwise convolution + bias + GELU in one pass (gfx950).
//
// The reference (mix_transformer.py:48-55, 358-369) views the fc1 output [M, H W, C] as NCHW, runs a depthwise Conv2d, flattens and
// transposes back and applies GELU: five to seven passes over the hidden tensor and three saved copies of it.  On token rows the same
// thing is a 9-tap stencil per channel with the channel as the fastest index:
//     u[m,y,x,c] = b[c] + sum_{i,j} w[c,i,j] h[m, y+i-1, x+j-1, c]   (zero outside the image),     out = u Phi(u)
//
// Work split.  A lane owns 4 consecutive channels (one 16-byte access) of an x-run of XR consecutive pixels and marches down a strip
// of YS rows, keeping input rows y-1, y, y+1 of its run (+ one halo pixel either side) in registers: every input is fetched once per
// strip, the halo comes out of the caches.  The 9 taps and the bias of the lane's channels stay in registers for the whole march.
// Consecutive lanes take consecutive channel quads and then the next x-run: a wave reads 1 KB contiguous per pixel at C = 256, two
// 512-byte pixels at C = 128.  No LDS.  A lane keeps its channel quad for life (slot T -> quad T % C4, spatial slot T / C4) and strides
// over the spatial items (image, strip, run), so the grid is capped (cdna_hip_programming.md Guidelines 11, 13) and the taps load once.
//
// Backward (h and dout in; u is recomputed, never stored):
//   k_dwg_bwd1   the same march: g = dout gelu'(u) to the workspace, and per lane the sums of g (db) and g h[y+i-1, x+j-1] (dw) over
//                its items.  A workgroup is 64 slots x 4 waves (the waves take different items of the same slots); the waves' sums are
//                added in a fixed order through LDS and the workgroup leaves one slab [10][64 slots] of f32x4.
//   k_dwg_bwd2   dh = the transposed stencil on g (the forward march with the taps reversed, no bias, no GELU); its leading workgroups
//                add the slabs in a fixed order (16 sequential chunks, then the 16 chunk sums in order) into dw [C,1,3,3] and db.
// No atomics: dw / db are the same bits run after run.  Every workspace byte that is read was written by the same call.
#pragma once
#include "cffm_common.h"

#define DWG_XR 4        // pixels per lane and row, forward and dh
#define DWG_XR_BWD 2    // ... in k_dwg_bwd1 (40 accumulators more per lane)
#define DWG_NACC 10     // 9 taps + bias: one f32x4 (the lane's channels) each
#define DWG_MIN_YS 8    // shortest y-strip the plan splits an image into (halo rows: 2 per strip)

struct DwgGeom {
    int M, H, W, C, C4;
    int YS, nys, nxr;   // rows per strip, strips per image, x-runs per row
    long nsp;           // spatial items = M * nys * nxr
    long S;             // spatial slots: S * C4 lanes are live
};

__device__ __forceinline__ f32x4 dwg_zero() { return (f32x4){0.f, 0.f, 0.f, 0.f}; }

// w[c][3][3] of the lane's 4 channels = 36 consecutive floats (144 c4 bytes in: 16-byte aligned) -> one f32x4 per tap; FLIP reverses
// the taps (the transposed stencil)
template <bool FLIP>
__device__ __forceinline__ void dwg_load_taps(const float* __restrict__ w, int c4, f32x4 (&tap)[9]) {
    f32x4 raw[9];
#pragma unroll
    for (int q = 0; q < 9; ++q) raw[q] = ((const f32x4*)w)[(long)c4 * 9 + q];
#pragma unroll
    for (int k = 0; k < 9; ++k)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int f = e * 9 + (FLIP ? 8 - k : k);
            tap[k][e] = raw[f >> 2][f & 3];
        }
}

// pixels x0-1 .. x0+XR of row y of one image (img points at the lane's channels of pixel (0,0)); zeros outside the image
template <int XR>
__device__ __forceinline__ void dwg_load_row(const float* __restrict__ img, int y, int x0, const DwgGeom& G, f32x4 (&r)[XR + 2]) {
    const bool yin = y >= 0 && y < G.H;
#pragma unroll
    for (int j = 0; j < XR + 2; ++j) {
        const int x = x0 + j - 1;
        r[j] = (yin && x >= 0 && x < G.W) ? *(const f32x4*)(img + ((long)y * G.W + x) * G.C) : dwg_zero();
    }
}

template <int XR>
__device__ __forceinline__ f32x4 dwg_stencil(const f32x4 (&a)[XR + 2], const f32x4 (&b)[XR + 2], const f32x4 (&c)[XR + 2],
                                             const f32x4 (&tap)[9], f32x4 bias, int j) {
    f32x4 u = bias;
#pragma unroll
    for (int jj = 0; jj < 3; ++jj) u += tap[jj] * a[j + jj];
#pragma unroll
    for (int jj = 0; jj < 3; ++jj) u += tap[3 + jj] * b[j + jj];
#pragma unroll
    for (int jj = 0; jj < 3; ++jj) u += tap[6 + jj] * c[j + jj];
    return u;
}

// (image, first row, last row + 1, first x) of spatial item sp: runs fastest, then strips, then images
__device__ __forceinline__ void dwg_item(const DwgGeom& G, long sp, int& m, int& y0, int& y1, int& x0, int xr) {
    const int r = (int)(sp % G.nxr);
    const long t = sp / G.nxr;
    m = (int)(t / G.nys);
    y0 = (int)(t % G.nys) * G.YS;
    y1 = y0 + G.YS < G.H ? y0 + G.YS : G.H;
    x0 = r * xr;
}

// one output row of the forward / dh march: a, b hold rows y-1, y; row y+1 is loaded into c
template <int XR, bool GELU>
__device__ __forceinline__ void dwg_row(const float* __restrict__ img, float* __restrict__ oimg, int y, int x0, const DwgGeom& G,
                                        const f32x4 (&a)[XR + 2], const f32x4 (&b)[XR + 2], f32x4 (&c)[XR + 2], const f32x4 (&tap)[9],
                                        f32x4 bias) {
    dwg_load_row<XR>(img, y + 1, x0, G, c);
#pragma unroll
    for (int j = 0; j < XR; ++j) {
        if (x0 + j < G.W) {
            f32x4 u = dwg_stencil<XR>(a, b, c, tap, bias, j);
            if (GELU) {
#pragma unroll
                for (int e = 0; e < 4; ++e) u[e] = gelu_erf(u[e]);
            }
            *(f32x4*)(oimg + ((long)y * G.W + x0 + j) * G.C) = u;
        }
    }
}

// the march of lane slot T over its spatial items: dst = [gelu](bias + stencil(src))
template <int XR, bool GELU, bool FLIP>
__device__ __forceinline__ void dwg_march(const float* __restrict__ src, const float* __restrict__ w, const float* __restrict__ bias,
                                          float* __restrict__ dst, const DwgGeom& G, long T) {
    if (T >= G.S * G.C4) return;
    const int c4 = (int)(T % G.C4);
    f32x4 tap[9];
    dwg_load_taps<FLIP>(w, c4, tap);
    const f32x4 bv = bias ? ((const f32x4*)bias)[c4] : dwg_zero();
    for (long sp = T / G.C4; sp < G.nsp; sp += G.S) {
        int m, y0, y1, x0;
        dwg_item(G, sp, m, y0, y1, x0, XR);
        const long base = (long)m * G.H * G.W * G.C + 4 * c4;
        const float* img = src + base;
        float* oimg = dst + base;
        f32x4 r0[XR + 2], r1[XR + 2], r2[XR + 2];
        dwg_load_row<XR>(img, y0 - 1, x0, G, r0);
        dwg_load_row<XR>(img, y0, x0, G, r1);
        for (int y = y0; y < y1;) {      // the three row buffers rotate by name, not by copy
            dwg_row<XR, GELU>(img, oimg, y, x0, G, r0, r1, r2, tap, bv);
            if (++y >= y1) break;
            dwg_row<XR, GELU>(img, oimg, y, x0, G, r1, r2, r0, tap, bv);
            if (++y >= y1) break;
            dwg_row<XR, GELU>(img, oimg, y, x0, G, r2, r0, r1, tap, bv);
            ++y;
        }
    }
}

// out = gelu(b + dwconv3x3(h)); grid = ceil(S C4 / 256)
__global__ void __launch_bounds__(256) k_dwg_fwd(const float* __restrict__ h, const float* __restrict__ w, const float* __restrict__ b,
                                                 float* __restrict__ out, DwgGeom G) {
    dwg_march<DWG_XR, true, false>(h, w, b, out, G, (long)blockIdx.x * 256 + threadIdx.x);
}

// one row of the first backward pass: g = dout gelu'(u) stored, db / dw sums of the lane's channels accumulated
template <int XR>
__device__ __forceinline__ void dwg_row_bwd(const float* __restrict__ img, const float* __restrict__ dimg, float* __restrict__ gimg, int y,
                                            int x0, const DwgGeom& G, const f32x4 (&a)[XR + 2], const f32x4 (&b)[XR + 2], f32x4 (&c)[XR + 2],
                                            const f32x4 (&tap)[9], f32x4 bias, f32x4 (&acc)[DWG_NACC]) {
    dwg_load_row<XR>(img, y + 1, x0, G, c);
#pragma unroll
    for (int j = 0; j < XR; ++j) {
        if (x0 + j < G.W) {
            const long o = ((long)y * G.W + x0 + j) * G.C;
            const f32x4 u = dwg_stencil<XR>(a, b, c, tap, bias, j);
            f32x4 g = *(const f32x4*)(dimg + o);
#pragma unroll
            for (int e = 0; e < 4; ++e) g[e] *= gelu_erf_grad(u[e]);
            *(f32x4*)(gimg + o) = g;
#pragma unroll
            for (int jj = 0; jj < 3; ++jj) {
                acc[jj] += g * a[j + jj];
                acc[3 + jj] += g * b[j + jj];
                acc[6 + jj] += g * c[j + jj];
            }
            acc[9] += g;
        }
    }
}

// grid = ceil(S C4 / 64): 64 slots per workgroup, wave q of a workgroup takes the items 4 s + q, 4 s + q + 4 S, ... of its slots.
// part: [S][DWG_NACC][C4] f32x4, every entry written.
__global__ void __launch_bounds__(256) k_dwg_bwd1(const float* __restrict__ h, const float* __restrict__ w, const float* __restrict__ b,
                                                  const float* __restrict__ dout, float* __restrict__ g, f32x4* __restrict__ part, DwgGeom G) {
    constexpr int XR = DWG_XR_BWD;
    __shared__ f32x4 red[3][DWG_NACC][64];
    const int lane = threadIdx.x & 63, q = threadIdx.x >> 6;
    const long T = (long)blockIdx.x * 64 + lane;
    const bool on = T < G.S * G.C4;
    const int c4 = (int)(T % G.C4);
    const long s = T / G.C4;
    f32x4 acc[DWG_NACC];
#pragma unroll
    for (int k = 0; k < DWG_NACC; ++k) acc[k] = dwg_zero();
    if (on) {
        f32x4 tap[9];
        dwg_load_taps<false>(w, c4, tap);
        const f32x4 bv = ((const f32x4*)b)[c4];
        for (long sp = 4 * s + q; sp < G.nsp; sp += 4 * G.S) {
            int m, y0, y1, x0;
            dwg_item(G, sp, m, y0, y1, x0, XR);
            const long base = (long)m * G.H * G.W * G.C + 4 * c4;
            const float* img = h + base;
            const float* dimg = dout + base;
            float* gimg = g + base;
            f32x4 r0[XR + 2], r1[XR + 2], r2[XR + 2];
            dwg_load_row<XR>(img, y0 - 1, x0, G, r0);
            dwg_load_row<XR>(img, y0, x0, G, r1);
            for (int y = y0; y < y1;) {
                dwg_row_bwd<XR>(img, dimg, gimg, y, x0, G, r0, r1, r2, tap, bv, acc);
                if (++y >= y1) break;
                dwg_row_bwd<XR>(img, dimg, gimg, y, x0, G, r1, r2, r0, tap, bv, acc);
                if (++y >= y1) break;
                dwg_row_bwd<XR>(img, dimg, gimg, y, x0, G, r2, r0, r1, tap, bv, acc);
                ++y;
            }
        }
    }
    if (q > 0) {
#pragma unroll
        for (int k = 0; k < DWG_NACC; ++k) red[q - 1][k][lane] = acc[k];
    }
    __syncthreads();
    if (q == 0 && on) {
#pragma unroll
        for (int k = 0; k < DWG_NACC; ++k)
            part[(s * DWG_NACC + k) * G.C4 + c4] = ((acc[k] + red[0][k][lane]) + red[1][k][lane]) + red[2][k][lane];
    }
}

// workgroups 0 .. nred-1 (nred = DWG_NACC * ceil(C4 / 16)): sum of the S1 slabs of `part` for one accumulator and 16 channel quads, into
// dw [C][9] / db [C]; the others: dh = transposed stencil of g, grid = nred + ceil(S C4 / 256)
__global__ void __launch_bounds__(256) k_dwg_bwd2(const float* __restrict__ g, const float* __restrict__ w, float* __restrict__ dh,
                                                  const f32x4* __restrict__ part, float* __restrict__ dw, float* __restrict__ db, DwgGeom G,
                                                  long S1, int nred) {
    if ((int)blockIdx.x < nred) {
        __shared__ f32x4 red[16][16];
        const int k = blockIdx.x % DWG_NACC, oi = threadIdx.x & 15, j = threadIdx.x >> 4;
        const int c4 = (blockIdx.x / DWG_NACC) * 16 + oi;
        const long per = (S1 + 15) / 16, s0 = j * per, s1 = s0 + per < S1 ? s0 + per : S1;
        f32x4 a = dwg_zero();
        if (c4 < G.C4)
            for (long s = s0; s < s1; ++s) a += part[(s * DWG_NACC + k) * G.C4 + c4];
        red[j][oi] = a;
        __syncthreads();
        if (j == 0 && c4 < G.C4) {
            f32x4 v = red[0][oi];
            for (int jj = 1; jj < 16; ++jj) v += red[jj][oi];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                if (k < 9) dw[(long)(4 * c4 + e) * 9 + k] = v[e];
                else db[4 * c4 + e] = v[e];
            }
        }
        return;
    }
    dwg_march<DWG_XR, false, true>(g, w, nullptr, dh, G, (long)(blockIdx.x - nred) * 256 + threadIdx.x);
}
