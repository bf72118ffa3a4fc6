// mitln_kernels.h -- LayerNorm of fp32 token rows at any width C = 4 * C4, 16 <= C <= 512, and the two layout changes at the ends of a MiT
// stage (backbones/mix_transformer.py: OverlapPatchEmbed.forward's flatten(2).transpose(1, 2) + norm; forward_features' norm_i +
// reshape(B, H, W, C).permute(0, 3, 1, 2).contiguous()), forward and backward.  The forwards save nothing: the backwards (second half of
// this file) recompute mean and rstd from the input with the forward's own arithmetic.
//
// One row lives in the registers of a GROUP of PW lanes of one wave (PW a power of two, 4..64): lane j of the group holds the 16-byte
// chunks j, j + L, ... (V of them) of the row, L = ceil(C4 / V) <= PW lanes of the group have work, the others carry zeros.  V = 1 up
// to C = 256 (PW = the power of two at or above C / 4: a wave holds 64 / PW rows), V = 2 above.  C = 160 / 320: L = 40 of 64 lanes.
// The sums are butterflies inside the group (DPP inside 16 lanes, a lane permute above): no LDS, no atomics, a fixed order -- the same
// bits run after run.  mean first, then the centred values d = x - mean, re-centred once by mean(d) (the first mean carries the rounding
// of a sum of magnitude C * |mean|; for rows with |mean| >> std that rounding is most of the error), variance = mean(d^2),
// rstd = 1 / sqrtf(var + eps).
//
// The two transposing kernels move a tile of TP pixels x C channels through LDS as T[pixel][LD], LD = C or C + 4 floats so that LD / 4
// is odd.  The NCHW side is accessed 16 bytes wide ALONG PIXELS (4 consecutive pixels of one channel per lane; a channel's run of TP
// pixels is contiguous), the row side 16 bytes wide along channels.  Between the two a quad of lanes that holds 4 channels x 4 pixels
// transposes its 4 x 4 block in registers (two exchange steps), so that the LDS, too, is only ever accessed 16 bytes wide:
//   quad side   lane (i, q) touches T[4 i + q][c0 .. c0 + 3]: the 8 lanes a ds_write_b128 serves together touch 8 consecutive pixels, whose
//               rows start LD apart = 8 different 16-byte slots of the 32 banks (LD / 4 odd); the 16 lanes of a ds_read_b128 group touch 16
//               pixels that are distinct mod 16 = 16 different slots of the 64 banks: no conflicts on either.
//   row side    the lanes of a group touch consecutive chunks of one row: no conflicts while a row fills the 8 (write) / 16 (read) lanes
//               served together, i.e. from C = 32 / C = 128 on (one wave = one row); below that two to four rows share an access and
//               one 16-byte slot of it can collide (C = 64: 1 extra LDS cycle on 4).  These kernels move 8 bytes per element through HBM
//               and 8 through LDS: the LDS side is not what bounds them.
// TP = 64 pixels up to C = 240, 32 up to C = 496, 16 above: at most 64,000 bytes of LDS, two to four workgroups per compute unit.
// H * W need not be a multiple of 4 (15 x 15 maps): the NCHW side is addressed with 4-byte alignment, and the last pixels of an image
// are moved one by one; rows / pixels past the end are neither read nor written.
#pragma once
#include "cffm_common.h"

#define MLN_LDS_FLOATS 16000
typedef f32x4 f32x4u __attribute__((aligned(4)));     // a 16-byte access at 4-byte alignment (NCHW rows of odd length)

struct MlnGeom {
    int C, C4, L;        // row width, its 16-byte chunks, lanes with work per group
    int HW, TP, LD;      // transposing kernels: pixels per image and per tile, floats per LDS row
    int tiles;           // tiles per image
};

static inline int mln_pw(int C) {           // group width: the power of two at or above the lanes with work
    const int C4 = C / 4, L = C4 > 64 ? (C4 + 1) / 2 : C4;
    int p = 4;
    while (p < L) p *= 2;
    return p;
}
static inline MlnGeom mln_geom(int C, int HW) {
    MlnGeom G;
    G.C = C; G.C4 = C / 4; G.L = G.C4 > 64 ? (G.C4 + 1) / 2 : G.C4;
    G.HW = HW;
    G.LD = (G.C4 & 1) ? C : C + 4;
    G.TP = 64;
    while (G.TP > 16 && G.TP * G.LD > MLN_LDS_FLOATS) G.TP /= 2;
    G.tiles = (HW + G.TP - 1) / G.TP;
    return G;
}

// sum over the aligned group of PW lanes this lane belongs to; every lane of the wave must call it
template <int PW>
__device__ __forceinline__ float mln_sum(float v) {
#ifdef CFFM_EMU
    for (int m = PW / 2; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
#else
    v += dpp_f32<0xB1>(v);                  // quad_perm [1,0,3,2]
    v += dpp_f32<0x4E>(v);                  // quad_perm [2,3,0,1]
    if (PW >= 8) v += dpp_f32<0x141>(v);    // row_half_mirror
    if (PW >= 16) v += dpp_f32<0x140>(v);   // row_mirror
    if (PW >= 32) v += __shfl_xor(v, 16, 64);
    if (PW >= 64) v += __shfl_xor(v, 32, 64);
#endif
    return v;
}

// mean, one re-centring and variance of the row held by this lane's group: x[k] = chunk (j + k L) of the row (zeros where !act[k]) -> the
// centred values (zeros where !act[k]); returns rstd.  The forward and the backwards share it: xhat = x[k] * rstd on both sides.
template <int PW, int V>
__device__ __forceinline__ float mln_centre(f32x4 (&x)[V], const bool (&act)[V], int C, float eps) {
    const float n = (float)C;
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < V; ++k) s += (x[k][0] + x[k][1]) + (x[k][2] + x[k][3]);
    const float m0 = mln_sum<PW>(s) / n;
    s = 0.f;
#pragma unroll
    for (int k = 0; k < V; ++k) {
#pragma unroll
        for (int e = 0; e < 4; ++e) x[k][e] = act[k] ? x[k][e] - m0 : 0.f;
        s += (x[k][0] + x[k][1]) + (x[k][2] + x[k][3]);
    }
    const float m1 = mln_sum<PW>(s) / n;
    s = 0.f;
#pragma unroll
    for (int k = 0; k < V; ++k) {
#pragma unroll
        for (int e = 0; e < 4; ++e) x[k][e] = act[k] ? x[k][e] - m1 : 0.f;
        s += (x[k][0] * x[k][0] + x[k][1] * x[k][1]) + (x[k][2] * x[k][2] + x[k][3] * x[k][3]);
    }
    return 1.f / sqrtf(mln_sum<PW>(s) / n + eps);
}

// LayerNorm of the row held by this lane's group: x[k] as for mln_centre -> the normalised chunks
template <int PW, int V>
__device__ __forceinline__ void mln_row(f32x4 (&x)[V], const bool (&act)[V], const f32x4 (&g)[V], const f32x4 (&b)[V], int C, float eps) {
    const float rstd = mln_centre<PW, V>(x, act, C, eps);
#pragma unroll
    for (int k = 0; k < V; ++k)
#pragma unroll
        for (int e = 0; e < 4; ++e) x[k][e] = x[k][e] * rstd * g[k][e] + b[k][e];
}

// this lane's chunks of gamma / beta (fixed for the whole kernel)
template <int V>
__device__ __forceinline__ void mln_affine(const float* __restrict__ gamma, const float* __restrict__ beta, const MlnGeom& G, int j,
                                           bool (&act)[V], f32x4 (&g)[V], f32x4 (&b)[V]) {
    const f32x4 z = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int k = 0; k < V; ++k) {
        const int ch = j + k * G.L;
        act[k] = j < G.L && ch < G.C4;
        g[k] = act[k] ? *(const f32x4*)(gamma + 4 * ch) : z;
        b[k] = act[k] ? *(const f32x4*)(beta + 4 * ch) : z;
    }
}

// out[M][C] = LN(x[M][C]).  256 threads = 4 waves x (64 / PW) rows; the grid strides over the rows.
template <int PW, int V>
__global__ void __launch_bounds__(256) k_ln_rows(const float* __restrict__ x, const float* __restrict__ gamma, const float* __restrict__ beta,
                                                  float* __restrict__ out, long M, MlnGeom G, float eps) {
    constexpr int RPB = 4 * (64 / PW);
    const int j = threadIdx.x & (PW - 1), sub = threadIdx.x / PW;
    const f32x4 z = (f32x4){0.f, 0.f, 0.f, 0.f};
    bool act[V];
    f32x4 g[V], b[V];
    mln_affine<V>(gamma, beta, G, j, act, g, b);
    for (long row0 = (long)blockIdx.x * RPB; row0 < M; row0 += (long)gridDim.x * RPB) {   // (uniform over the workgroup)
        const long row = row0 + sub;
        const bool live = row < M;
        f32x4 v[V];
#pragma unroll
        for (int k = 0; k < V; ++k) v[k] = (live && act[k]) ? *(const f32x4*)(x + row * G.C + 4 * (j + k * G.L)) : z;
        mln_row<PW, V>(v, act, g, b, G.C, eps);
#pragma unroll
        for (int k = 0; k < V; ++k)
            if (live && act[k]) *(f32x4*)(out + row * G.C + 4 * (j + k * G.L)) = v[k];
    }
}

// 4 x 4 transpose inside a quad of lanes: lane q holds m[q][0..3] on entry and m[0..3][q] on return (its own inverse); every lane of the
// wave must call it
__device__ __forceinline__ float mln_xchg1(float v) {
#ifdef CFFM_EMU
    return __shfl_xor(v, 1, 64);
#else
    return dpp_f32<0xB1>(v);
#endif
}
__device__ __forceinline__ float mln_xchg2(float v) {
#ifdef CFFM_EMU
    return __shfl_xor(v, 2, 64);
#else
    return dpp_f32<0x4E>(v);
#endif
}
__device__ __forceinline__ f32x4 mln_quad_transpose(f32x4 v, int q) {
    const bool hi2 = q & 2, hi1 = q & 1;
    const float a = mln_xchg2(hi2 ? v[0] : v[2]), b = mln_xchg2(hi2 ? v[1] : v[3]);   // the off-diagonal 2 x 2 blocks change lanes
    if (hi2) { v[0] = a; v[1] = b; } else { v[2] = a; v[3] = b; }
    const float c = mln_xchg1(hi1 ? v[0] : v[1]), d = mln_xchg1(hi1 ? v[2] : v[3]);   // then the off-diagonal elements of every 2 x 2 block
    if (hi1) { v[0] = c; v[2] = d; } else { v[1] = c; v[3] = d; }
    return v;
}

// quad items of a tile: item = (channel quad cq, pixel quad i), i fastest: lane (i, q) is channel 4 cq + q, pixels 4 i .. 4 i + 3 on
// the NCHW side and pixel 4 i + q, channels 4 cq .. 4 cq + 3 on the LDS side
#define MLN_ITEMS(G) ((G).C4 * ((G).TP / 4))

// x [B][C][HW] -> out [B][HW][C] = LN over C of every pixel.  grid = B * tiles, 256 threads, dynamic LDS = TP * LD floats.
template <int PW, int V>
__global__ void __launch_bounds__(256) k_nchw_ln_rows(const float* __restrict__ x, const float* __restrict__ gamma, const float* __restrict__ beta,
                                                       float* __restrict__ out, MlnGeom G, float eps) {
    CFFM_DYN_SMEM(smem);
    float* T = (float*)smem;
    const int img = blockIdx.x / G.tiles, p0 = (blockIdx.x % G.tiles) * G.TP;
    const int np = G.HW - p0 < G.TP ? G.HW - p0 : G.TP;       // pixels of this tile
    const float* xi = x + (long)img * G.C * G.HW + p0;
    const int q = threadIdx.x & 3, PG = G.TP / 4, items = MLN_ITEMS(G);
    const f32x4 z = (f32x4){0.f, 0.f, 0.f, 0.f};
    for (int it0 = 0; it0 < items; it0 += 64) {               // (uniform over the workgroup: the exchanges need whole waves)
        const int it = it0 + (threadIdx.x >> 2);
        const bool live = it < items;
        const int cq = it / PG, i = it % PG;
        f32x4 v = z;
        if (live && 4 * i < np) {
            const float* src = xi + (long)(4 * cq + q) * G.HW + 4 * i;
            if (4 * i + 3 < np) v = *(const f32x4u*)src;
            else
                for (int e = 0; e < 4; ++e)
                    if (4 * i + e < np) v[e] = src[e];
        }
        v = mln_quad_transpose(v, q);
        if (live) *(f32x4*)(T + (4 * i + q) * G.LD + 4 * cq) = v;   // (pixels past np: zeros, never read back)
    }
    __syncthreads();
    constexpr int RPB = 4 * (64 / PW);
    const int j = threadIdx.x & (PW - 1), sub = threadIdx.x / PW;
    bool act[V];
    f32x4 g[V], b[V];
    mln_affine<V>(gamma, beta, G, j, act, g, b);
    float* oi = out + ((long)img * G.HW + p0) * G.C;
    for (int r0 = 0; r0 < G.TP; r0 += RPB) {
        const int r = r0 + sub;
        const bool live = r < np;
        f32x4 v[V];
#pragma unroll
        for (int k = 0; k < V; ++k) v[k] = (live && act[k]) ? *(const f32x4*)(T + r * G.LD + 4 * (j + k * G.L)) : z;
        mln_row<PW, V>(v, act, g, b, G.C, eps);
#pragma unroll
        for (int k = 0; k < V; ++k)
            if (live && act[k]) *(f32x4*)(oi + (long)r * G.C + 4 * (j + k * G.L)) = v[k];
    }
}

// x [B][HW][C] -> out [B][C][HW] = LN over C of every pixel, as an NCHW map.  Same grid, block and LDS as k_nchw_ln_rows.
template <int PW, int V>
__global__ void __launch_bounds__(256) k_ln_rows_nchw(const float* __restrict__ x, const float* __restrict__ gamma, const float* __restrict__ beta,
                                                       float* __restrict__ out, MlnGeom G, float eps) {
    CFFM_DYN_SMEM(smem);
    float* T = (float*)smem;
    const int img = blockIdx.x / G.tiles, p0 = (blockIdx.x % G.tiles) * G.TP;
    const int np = G.HW - p0 < G.TP ? G.HW - p0 : G.TP;
    const f32x4 z = (f32x4){0.f, 0.f, 0.f, 0.f};
    {
        constexpr int RPB = 4 * (64 / PW);
        const int j = threadIdx.x & (PW - 1), sub = threadIdx.x / PW;
        bool act[V];
        f32x4 g[V], b[V];
        mln_affine<V>(gamma, beta, G, j, act, g, b);
        const float* xi = x + ((long)img * G.HW + p0) * G.C;
        for (int r0 = 0; r0 < G.TP; r0 += RPB) {
            const int r = r0 + sub;
            const bool live = r < np;
            f32x4 v[V];
#pragma unroll
            for (int k = 0; k < V; ++k) v[k] = (live && act[k]) ? *(const f32x4*)(xi + (long)r * G.C + 4 * (j + k * G.L)) : z;
            mln_row<PW, V>(v, act, g, b, G.C, eps);
#pragma unroll
            for (int k = 0; k < V; ++k)
                if (live && act[k]) *(f32x4*)(T + r * G.LD + 4 * (j + k * G.L)) = v[k];
        }
    }
    __syncthreads();
    float* oi = out + (long)img * G.C * G.HW + p0;
    const int q = threadIdx.x & 3, PG = G.TP / 4, items = MLN_ITEMS(G);
    for (int it0 = 0; it0 < items; it0 += 64) {
        const int it = it0 + (threadIdx.x >> 2);
        const bool live = it < items;
        const int cq = it / PG, i = it % PG;
        f32x4 v = z;
        if (live && 4 * i + q < np) v = *(const f32x4*)(T + (4 * i + q) * G.LD + 4 * cq);   // (rows past np were never written)
        v = mln_quad_transpose(v, q);
        if (live && 4 * i < np) {
            float* dst = oi + (long)(4 * cq + q) * G.HW + 4 * i;
            if (4 * i + 3 < np) *(f32x4u*)dst = v;
            else
                for (int e = 0; e < 4; ++e)
                    if (4 * i + e < np) dst[e] = v[e];
        }
    }
}

// ------------------------------------------------------------------------------------------------ backward
// dx = rstd * (g - mean(g) - xhat * mean(g * xhat)), g = gamma * dy, in the row layout of the forwards.  mean and rstd are NOT saved by the
// forward: mln_centre recomputes them from x, so xhat has the forward's bits.  dgamma[c] = sum over rows of dy * xhat, dbeta[c] = sum
// over rows of dy: a lane adds up its channels over the rows it handles, the workgroup adds its row groups in a fixed order through LDS
// (mln_record) and writes ONE record [2][C] to the workspace; k_ln_bwd_final adds the records.  How many records there are and the
// order they are added in follow from (M, C, HW) alone: the same bits run after run, on any device.

#define MLN_BWD_GRID_CAP 1024                      // rows form: workgroups = records at most (the map forms: one record per tile)
#define MLN_RED_FLOATS(V) (2048 * (V))             // LDS of mln_record: 256 lanes x (dgamma | dbeta) x V chunks

// this lane's chunks of gamma
template <int V>
__device__ __forceinline__ void mln_gamma(const float* __restrict__ gamma, const MlnGeom& G, int j, bool (&act)[V], f32x4 (&g)[V]) {
#pragma unroll
    for (int k = 0; k < V; ++k) {
        const int ch = j + k * G.L;
        act[k] = j < G.L && ch < G.C4;
        g[k] = act[k] ? *(const f32x4*)(gamma + 4 * ch) : (f32x4){0.f, 0.f, 0.f, 0.f};
    }
}

// backward of the row held by this lane's group: x[k] / dy[k] = this lane's chunks of the row and of its output gradient (zeros where
// !act[k] or the row is not live) -> dx in x[k]; dg / db take the row's terms of dgamma / dbeta
template <int PW, int V>
__device__ __forceinline__ void mln_row_bwd(f32x4 (&x)[V], f32x4 (&dy)[V], const bool (&act)[V], const f32x4 (&g)[V], bool live, int C, float eps,
                                            f32x4 (&dg)[V], f32x4 (&db)[V]) {
    const float n = (float)C;
    const float rstd = mln_centre<PW, V>(x, act, C, eps);
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int k = 0; k < V; ++k) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float xh = x[k][e] * rstd, d = dy[k][e];
            dg[k][e] += live ? d * xh : 0.f;        // (a row past the end: x = 0 and, at eps = 0, rstd = inf)
            db[k][e] += d;
            x[k][e] = xh;
            dy[k][e] = g[k][e] * d;
        }
        s1 += (dy[k][0] + dy[k][1]) + (dy[k][2] + dy[k][3]);
        s2 += (dy[k][0] * x[k][0] + dy[k][1] * x[k][1]) + (dy[k][2] * x[k][2] + dy[k][3] * x[k][3]);
    }
    const float a = mln_sum<PW>(s1) / n, c = mln_sum<PW>(s2) / n;
#pragma unroll
    for (int k = 0; k < V; ++k)
#pragma unroll
        for (int e = 0; e < 4; ++e) x[k][e] = rstd * (dy[k][e] - a - x[k][e] * c);
}

// the workgroup's record: R[row group][dgamma | dbeta][k][lane of the group] <- every lane's sums; then lane (which, k, j) adds the row
// groups in their order and writes chunk j + k L of rec[which][C].  R: MLN_RED_FLOATS(V) floats of LDS that nobody reads or writes any
// more when the first lane gets here (the caller's barrier)
template <int PW, int V>
__device__ __forceinline__ void mln_record(f32x4* R, const f32x4 (&dg)[V], const f32x4 (&db)[V], const MlnGeom& G, float* __restrict__ rec) {
    constexpr int RPB = 4 * (64 / PW);
    const int j = threadIdx.x & (PW - 1), sub = threadIdx.x / PW;
#pragma unroll
    for (int k = 0; k < V; ++k) {
        R[((sub * 2 + 0) * V + k) * PW + j] = dg[k];
        R[((sub * 2 + 1) * V + k) * PW + j] = db[k];
    }
    __syncthreads();
    if (threadIdx.x < 2 * V * PW) {
        const int k = (threadIdx.x / PW) % V, which = threadIdx.x / (PW * V);
        f32x4 s = R[(which * V + k) * PW + j];
        for (int r = 1; r < RPB; ++r) s += R[((r * 2 + which) * V + k) * PW + j];
        const int ch = j + k * G.L;
        if (j < G.L && ch < G.C4) *(f32x4*)(rec + which * G.C + 4 * ch) = s;
    }
}

// dx[M][C] of out = LN(x[M][C]) from dy[M][C]; rec[gridDim.x][2][C].  Block and row walk of k_ln_rows; the grid is at most
// MLN_BWD_GRID_CAP workgroups.
template <int PW, int V>
__global__ void __launch_bounds__(256) k_ln_rows_bwd(const float* __restrict__ x, const float* __restrict__ gamma, const float* __restrict__ dy,
                                                      float* __restrict__ dx, float* __restrict__ rec, long M, MlnGeom G, float eps) {
    constexpr int RPB = 4 * (64 / PW);
    __shared__ f32x4 R[MLN_RED_FLOATS(V) / 4];
    const int j = threadIdx.x & (PW - 1), sub = threadIdx.x / PW;
    const f32x4 z = (f32x4){0.f, 0.f, 0.f, 0.f};
    bool act[V];
    f32x4 g[V], dg[V], db[V];
    mln_gamma<V>(gamma, G, j, act, g);
#pragma unroll
    for (int k = 0; k < V; ++k) dg[k] = db[k] = z;
    for (long row0 = (long)blockIdx.x * RPB; row0 < M; row0 += (long)gridDim.x * RPB) {   // (uniform over the workgroup)
        const long row = row0 + sub;
        const bool live = row < M;
        f32x4 v[V], d[V];
#pragma unroll
        for (int k = 0; k < V; ++k) {
            v[k] = (live && act[k]) ? *(const f32x4*)(x + row * G.C + 4 * (j + k * G.L)) : z;
            d[k] = (live && act[k]) ? *(const f32x4*)(dy + row * G.C + 4 * (j + k * G.L)) : z;
        }
        mln_row_bwd<PW, V>(v, d, act, g, live, G.C, eps, dg, db);
#pragma unroll
        for (int k = 0; k < V; ++k)
            if (live && act[k]) *(f32x4*)(dx + row * G.C + 4 * (j + k * G.L)) = v[k];
    }
    mln_record<PW, V>(R, dg, db, G, rec + (long)blockIdx.x * 2 * G.C);
}

// a + b rounded on its own: the add carries no contract flag, so it is never fused with the multiply that made an operand.  (__fadd_rn
// is a plain `+` in the HIP headers and IS fused under the device default -ffp-contract=fast.)
__device__ __forceinline__ float mln_add_rn(float a, float b) {
#pragma clang fp contract(off)
    return a + b;
}

// k_ln_rows_bwd with the adds autograd puts around a block's LayerNorms fused in:  d = dya (+ dyb, HAS_B),  v = LN-backward(x, gamma, d),
// dx = dres + v (HAS_RES) or v.  Each add is one fp32 add rounded on its own, so dx / dgamma / dbeta have the bits of
// k_ln_rows_bwd(x, gamma, dya + dyb) followed by dres + dx as two separate element-wise passes.  For that mln_row_bwd has to be compiled
// to the instructions it has in k_ln_rows_bwd: where a product with two users may be folded into an FMA or not (g * dy in g * dy - a),
// what the compiler does depends on the code around it.  With the two adds as run-time branches the V = 2 form came out with other
// FMAs than k_ln_rows_bwd's, and so did every form with the result passed through an empty asm before the last add; as template
// parameters, nothing else added, all forms have k_ln_rows_bwd's multiplies and FMAs (counted in the ISA, and tested bit for bit).
// dx == dres is allowed: a lane reads its own chunks of dres before it writes them (hence no __restrict__ on the two).  rec, grid,
// block: as k_ln_rows_bwd.
template <int PW, int V, bool HAS_B, bool HAS_RES>
__global__ void __launch_bounds__(256) k_ln_rows_bwd_add(const float* __restrict__ x, const float* __restrict__ gamma, const float* __restrict__ dya,
                                                          const float* __restrict__ dyb, const float* dres, float* dx, float* __restrict__ rec,
                                                          long M, MlnGeom G, float eps) {
    constexpr int RPB = 4 * (64 / PW);
    __shared__ f32x4 R[MLN_RED_FLOATS(V) / 4];
    const int j = threadIdx.x & (PW - 1), sub = threadIdx.x / PW;
    const f32x4 z = (f32x4){0.f, 0.f, 0.f, 0.f};
    bool act[V];
    f32x4 g[V], dg[V], db[V];
    mln_gamma<V>(gamma, G, j, act, g);
#pragma unroll
    for (int k = 0; k < V; ++k) dg[k] = db[k] = z;
    for (long row0 = (long)blockIdx.x * RPB; row0 < M; row0 += (long)gridDim.x * RPB) {   // (uniform over the workgroup)
        const long row = row0 + sub;
        const bool live = row < M;
        f32x4 v[V], d[V], r[V];
#pragma unroll
        for (int k = 0; k < V; ++k) {
            v[k] = (live && act[k]) ? *(const f32x4*)(x + row * G.C + 4 * (j + k * G.L)) : z;
            d[k] = (live && act[k]) ? *(const f32x4*)(dya + row * G.C + 4 * (j + k * G.L)) : z;
            if (HAS_B) {
                const f32x4 e = (live && act[k]) ? *(const f32x4*)(dyb + row * G.C + 4 * (j + k * G.L)) : z;
#pragma unroll
                for (int c = 0; c < 4; ++c) d[k][c] = mln_add_rn(d[k][c], e[c]);
            }
            if (HAS_RES) r[k] = (live && act[k]) ? *(const f32x4*)(dres + row * G.C + 4 * (j + k * G.L)) : z;
        }
        mln_row_bwd<PW, V>(v, d, act, g, live, G.C, eps, dg, db);
#pragma unroll
        for (int k = 0; k < V; ++k) {
            if (HAS_RES) {
#pragma unroll
                for (int c = 0; c < 4; ++c) v[k][c] = mln_add_rn(r[k][c], v[k][c]);
            }
            if (live && act[k]) *(f32x4*)(dx + row * G.C + 4 * (j + k * G.L)) = v[k];
        }
    }
    mln_record<PW, V>(R, dg, db, G, rec + (long)blockIdx.x * 2 * G.C);
}

// one image's NCHW pixels p0 .. p0 + np - 1 (src = channel 0, pixel p0) -> T[pixel][LD]: the input side of k_nchw_ln_rows
__device__ __forceinline__ void mln_tile_in(float* T, const float* __restrict__ src0, const MlnGeom& G, int np) {
    const int q = threadIdx.x & 3, PG = G.TP / 4, items = MLN_ITEMS(G);
    for (int it0 = 0; it0 < items; it0 += 64) {               // (uniform over the workgroup: the exchanges need whole waves)
        const int it = it0 + (threadIdx.x >> 2);
        const bool live = it < items;
        const int cq = it / PG, i = it % PG;
        f32x4 v = (f32x4){0.f, 0.f, 0.f, 0.f};
        if (live && 4 * i < np) {
            const float* src = src0 + (long)(4 * cq + q) * G.HW + 4 * i;
            if (4 * i + 3 < np) v = *(const f32x4u*)src;
            else
                for (int e = 0; e < 4; ++e)
                    if (4 * i + e < np) v[e] = src[e];
        }
        v = mln_quad_transpose(v, q);
        if (live) *(f32x4*)(T + (4 * i + q) * G.LD + 4 * cq) = v;   // (pixels past np: zeros, never read back)
    }
}
// T[pixel][LD], rows 0 .. np - 1 -> one image's NCHW pixels p0 .. p0 + np - 1 (dst0 = channel 0, pixel p0): the output side of k_ln_rows_nchw
__device__ __forceinline__ void mln_tile_out(const float* T, float* __restrict__ dst0, const MlnGeom& G, int np) {
    const int q = threadIdx.x & 3, PG = G.TP / 4, items = MLN_ITEMS(G);
    for (int it0 = 0; it0 < items; it0 += 64) {
        const int it = it0 + (threadIdx.x >> 2);
        const bool live = it < items;
        const int cq = it / PG, i = it % PG;
        f32x4 v = (f32x4){0.f, 0.f, 0.f, 0.f};
        if (live && 4 * i + q < np) v = *(const f32x4*)(T + (4 * i + q) * G.LD + 4 * cq);
        v = mln_quad_transpose(v, q);
        if (live && 4 * i < np) {
            float* dst = dst0 + (long)(4 * cq + q) * G.HW + 4 * i;
            if (4 * i + 3 < np) *(f32x4u*)dst = v;
            else
                for (int e = 0; e < 4; ++e)
                    if (4 * i + e < np) dst[e] = v[e];
        }
    }
}

// dynamic LDS of the two transposing backwards (floats): the tile, and room for mln_record once the tile is dead
static inline size_t mln_bwd_lds_floats(const MlnGeom& G, int V) {
    const size_t tile = (size_t)G.TP * G.LD, red = MLN_RED_FLOATS(V);
    return tile > red ? tile : red;
}

// backward of k_ln_rows_nchw (a stage's norm + the NCHW map): x [B][HW][C] rows, dy [B][C][HW] through the tile -> dx [B][HW][C] rows;
// rec[B * tiles][2][C].  grid = B * tiles, 256 threads, dynamic LDS = mln_bwd_lds_floats.
template <int PW, int V>
__global__ void __launch_bounds__(256) k_ln_rows_nchw_bwd(const float* __restrict__ x, const float* __restrict__ gamma, const float* __restrict__ dy,
                                                           float* __restrict__ dx, float* __restrict__ rec, MlnGeom G, float eps) {
    CFFM_DYN_SMEM(smem);
    float* T = (float*)smem;
    const int img = blockIdx.x / G.tiles, p0 = (blockIdx.x % G.tiles) * G.TP;
    const int np = G.HW - p0 < G.TP ? G.HW - p0 : G.TP;
    mln_tile_in(T, dy + (long)img * G.C * G.HW + p0, G, np);
    __syncthreads();
    constexpr int RPB = 4 * (64 / PW);
    const int j = threadIdx.x & (PW - 1), sub = threadIdx.x / PW;
    const f32x4 z = (f32x4){0.f, 0.f, 0.f, 0.f};
    bool act[V];
    f32x4 g[V], dg[V], db[V];
    mln_gamma<V>(gamma, G, j, act, g);
#pragma unroll
    for (int k = 0; k < V; ++k) dg[k] = db[k] = z;
    const long base = ((long)img * G.HW + p0) * G.C;
    for (int r0 = 0; r0 < G.TP; r0 += RPB) {
        const int r = r0 + sub;
        const bool live = r < np;
        f32x4 v[V], d[V];
#pragma unroll
        for (int k = 0; k < V; ++k) {
            v[k] = (live && act[k]) ? *(const f32x4*)(x + base + (long)r * G.C + 4 * (j + k * G.L)) : z;
            d[k] = (live && act[k]) ? *(const f32x4*)(T + r * G.LD + 4 * (j + k * G.L)) : z;
        }
        mln_row_bwd<PW, V>(v, d, act, g, live, G.C, eps, dg, db);
#pragma unroll
        for (int k = 0; k < V; ++k)
            if (live && act[k]) *(f32x4*)(dx + base + (long)r * G.C + 4 * (j + k * G.L)) = v[k];
    }
    __syncthreads();                                          // (the tile is dead: mln_record takes its room)
    mln_record<PW, V>((f32x4*)T, dg, db, G, rec + (long)blockIdx.x * 2 * G.C);
}

// backward of k_nchw_ln_rows (the embedding's flatten / transpose + norm): x [B][C][HW] through the tile, dy [B][HW][C] rows; every row
// group overwrites its own tile row with dx, and the tile leaves as dx [B][C][HW].  Grid, block, LDS and rec as k_ln_rows_nchw_bwd.
template <int PW, int V>
__global__ void __launch_bounds__(256) k_nchw_ln_rows_bwd(const float* __restrict__ x, const float* __restrict__ gamma, const float* __restrict__ dy,
                                                           float* __restrict__ dx, float* __restrict__ rec, MlnGeom G, float eps) {
    CFFM_DYN_SMEM(smem);
    float* T = (float*)smem;
    const int img = blockIdx.x / G.tiles, p0 = (blockIdx.x % G.tiles) * G.TP;
    const int np = G.HW - p0 < G.TP ? G.HW - p0 : G.TP;
    mln_tile_in(T, x + (long)img * G.C * G.HW + p0, G, np);
    __syncthreads();
    constexpr int RPB = 4 * (64 / PW);
    const int j = threadIdx.x & (PW - 1), sub = threadIdx.x / PW;
    const f32x4 z = (f32x4){0.f, 0.f, 0.f, 0.f};
    bool act[V];
    f32x4 g[V], dg[V], db[V];
    mln_gamma<V>(gamma, G, j, act, g);
#pragma unroll
    for (int k = 0; k < V; ++k) dg[k] = db[k] = z;
    const long base = ((long)img * G.HW + p0) * G.C;
    for (int r0 = 0; r0 < G.TP; r0 += RPB) {
        const int r = r0 + sub;
        const bool live = r < np;
        f32x4 v[V], d[V];
#pragma unroll
        for (int k = 0; k < V; ++k) {
            v[k] = (live && act[k]) ? *(const f32x4*)(T + r * G.LD + 4 * (j + k * G.L)) : z;
            d[k] = (live && act[k]) ? *(const f32x4*)(dy + base + (long)r * G.C + 4 * (j + k * G.L)) : z;
        }
        mln_row_bwd<PW, V>(v, d, act, g, live, G.C, eps, dg, db);
#pragma unroll
        for (int k = 0; k < V; ++k)
            if (live && act[k]) *(f32x4*)(T + r * G.LD + 4 * (j + k * G.L)) = v[k];   // (a lane rewrites the chunks it read, nobody else's)
    }
    __syncthreads();
    mln_tile_out(T, dx + (long)img * G.C * G.HW + p0, G, np);
    __syncthreads();                                          // (the tile has left: mln_record takes its room)
    mln_record<PW, V>((f32x4*)T, dg, db, G, rec + (long)blockIdx.x * 2 * G.C);
}

// dgamma[C] | dbeta[C] = the sum of R records [2][C].  A workgroup takes ONE of the record's C / 2 16-byte chunks, its 256 lanes are 256
// slices: slice s adds the records s, s + 256, s + 512, ... in that order (1800 records: 8 loads a lane, independent of each other),
// then the slices are added as a binary tree through LDS -- a fixed shape, whatever R.  grid = C / 2, 256 threads.  (8 chunks x 32
// slices per workgroup, the first form, walked 57 records per lane one load after the other: 18.5 us at stage 1, more than the backward.)
#define MLN_FIN_SLICES 256
__global__ void __launch_bounds__(MLN_FIN_SLICES) k_ln_bwd_final(const float* __restrict__ rec, float* __restrict__ dgamma,
                                                                  float* __restrict__ dbeta, int R, int C) {
    __shared__ f32x4 S[MLN_FIN_SLICES];
    const int s = threadIdx.x, ch = blockIdx.x;               // slice; chunk of the record
    f32x4 acc = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll 4
    for (int r = s; r < R; r += MLN_FIN_SLICES) acc += *(const f32x4*)(rec + (long)r * 2 * C + 4 * ch);
    S[s] = acc;
    __syncthreads();
    for (int h = MLN_FIN_SLICES / 2; h >= 1; h >>= 1) {
        if (s < h) S[s] += S[s + h];
        __syncthreads();
    }
    if (s == 0) *(f32x4*)(4 * ch < C ? dgamma + 4 * ch : dbeta + (4 * ch - C)) = S[0];
}
