// kmeans_kernels.h -- Lloyd's k-means on [N,256] fp32 rows for K <= 128 centres (the prototype-generating stage of CFFM++,
// cffm_head.py:280-282), all iterations enqueued by one library call: two kernels per iteration, no host round trip.
//
//   k_km_step<KT>   one workgroup per chunk of 64 * tpw consecutive points, four waves:
//     assign   label_i = argmin_j (|c_j|^2 - 2 x_i.c_j).  S^T [centres x points] = C X^T on the matrix pipe in the three-pass bf16
//              hi / lo split of the Linear GEMMs (hi x lo + lo x hi + hi x hi): the centre fragments (A operand, packed once per iteration
//              by k_km_reduce) sit in LDS, a wave owns 16-point tiles and takes the B operand straight from the lanes' own x rows; the argmin
//              runs over the C registers of a lane (ascending centre index, strict <) and then over the four lane groups with the index as
//              tie break: bit-equal scores go to the lowest centre.
//     update   the chunk's one-hot product  sums^T [channels x centres] = X^T onehot  on the matrix pipe: the 0 / 1 operand is exact in bf16
//              and x enters in three bf16 pieces hi + lo + lo2 that reproduce the fp32 value exactly, so the three passes add the fp32
//              values themselves in fp32 accumulators.  A wave owns 64 channels; the chunk's labels stay in LDS.  The workgroup leaves one
//              record [K][256] of partial sums and one [K] of integer counts.
//   k_km_reduce     adds the records of a centre in a fixed order in fp64 (deterministic: no atomics), divides by the count -- a centre
//              that attracted no point keeps its value --, stores the new centre and its hi / lo fragments for the next k_km_step.  With
//              P = 0 records it only packs the centres it is given (the call's first launch).
//
// Fragment layout (16-byte words, unit = 64 lanes): unit (kt, ks, hi | lo) = (kt * 8 + ks) * 2 + {0, 1}; lane (l15, g) holds centre
// 16 kt + l15, k-slots j = 0..7 <-> channels km_ch(ks, g, j) = 32 ks + 16 (j >> 2) + 4 g + (j & 3): with this bijection a lane's B operand
// of k-step ks is two of the sixteen 16-byte loads that read its x row 64 contiguous bytes per row and instruction.  Rows >= K of the last
// tile are stored as zeros (the workspace may hold anything on entry).
#pragma once
#include "gemm_kernels.h"      // mfma16x16x32_bf16

#ifndef KM_WGS
#define KM_WGS 256             // workgroups k_km_step aims for: a wave walks tpw = ceil(tiles / (4 KM_WGS)) 16-point tiles
#endif
#define KM_MAX_TPW 32          // chunk <= 2048 points (8 KiB of labels in LDS); beyond that the grid grows instead
#define KM_CT 4                // channel tiles of 16 per wave in the update (4 waves x 64 channels)

__host__ __device__ constexpr int km_frag_words(int KT) { return KT * 16 * 64; }                 // f32x4 words of the centre fragments
__host__ __device__ constexpr int km_step_lds(int KT, int tpw) { return km_frag_words(KT) * 16 + 256 * 4 + 64 * tpw * 4; }

__device__ __forceinline__ int km_min(int a, int b) { return a < b ? a : b; }

// grid (16 KT, 4): workgroup (centre j, 64-channel slice q), 256 threads = 16 record groups x 16 lanes of four channels.
// partial [P][K][256], pcount [P][K]; frags: bf16 view of the fragment words; counts_out may be NULL.
__global__ void __launch_bounds__(256) k_km_reduce(const float* __restrict__ partial, const int* __restrict__ pcount, int P, int K,
                                                   float* __restrict__ centers, bf16* __restrict__ frags, int* __restrict__ counts_out) {
    __shared__ double red[16][64];
    __shared__ int cnt_s[4];
    const int j = blockIdx.x, q = blockIdx.y, tid = threadIdx.x, l16 = tid & 15, pg = tid >> 4;
    const bool real = j < K;                               // (workgroup-uniform)
    double s0 = 0., s1 = 0., s2 = 0., s3 = 0.;
    int c = 0;
    if (real) {
#pragma unroll 4
        for (int p = pg; p < P; p += 16) {                 // record group pg: records pg, pg + 16, ... in this order
            const f32x4 v = *(const f32x4*)(partial + ((long)p * K + j) * CFFM_C + 64 * q + 4 * l16);
            s0 += (double)v[0]; s1 += (double)v[1]; s2 += (double)v[2]; s3 += (double)v[3];
        }
        for (int p = tid; p < P; p += 256) c += pcount[(long)p * K + j];
    }
    red[pg][4 * l16 + 0] = s0; red[pg][4 * l16 + 1] = s1; red[pg][4 * l16 + 2] = s2; red[pg][4 * l16 + 3] = s3;
    for (int m = 32; m >= 1; m >>= 1) c += __shfl_xor(c, m, 64);       // (integers: any order gives the same sum)
    if ((tid & 63) == 0) cnt_s[tid >> 6] = c;
    __syncthreads();
    if (tid >= 64) return;
    const int ch = 64 * q + tid, cnt = cnt_s[0] + cnt_s[1] + cnt_s[2] + cnt_s[3];
    float v = 0.f;                                         // rows >= K: zero fragments
    if (real) {
        if (cnt > 0) {
            double tot = 0.;
#pragma unroll
            for (int gq = 0; gq < 16; ++gq) tot += red[gq][tid];
            v = (float)(tot / (double)cnt);
            centers[(long)j * CFFM_C + ch] = v;
        } else {
            v = centers[(long)j * CFFM_C + ch];            // an empty cluster keeps its centre
        }
        if (counts_out && q == 0 && tid == 0) counts_out[j] = cnt;
    }
    const bf16 hi = (bf16)v, lo = (bf16)(v - (float)hi);
    const int kt = j >> 4, ks = ch >> 5, c32 = ch & 31, slot = 4 * (c32 >> 4) + (c32 & 3), lane = 16 * ((c32 & 15) >> 2) + (j & 15);
    const long w = ((long)((kt * 8 + ks) * 2) * 64 + lane) * 8 + slot;
    frags[w] = hi;
    frags[w + 64 * 8] = lo;
}

// the update's raw operand of one k-step: x[p0 + 8 g + j][channel 16 ct + the lane's] (rows behind N: the last row, zeroed when used)
__device__ __forceinline__ void km_load_x(const float* __restrict__ xc, int N, int p0, int g, float (&xv)[KM_CT][8]) {
#pragma unroll
    for (int ct = 0; ct < KM_CT; ++ct)
#pragma unroll
        for (int j = 0; j < 8; ++j) xv[ct][j] = xc[(long)km_min(p0 + 8 * g + j, N - 1) * CFFM_C + 16 * ct];
}

// grid (P), 256 threads, km_step_lds(KT, tpw) bytes of dynamic LDS.  labels_out may be NULL.
template <int KT>
__global__ void __launch_bounds__(256) k_km_step(const float* __restrict__ x, int N, int K, const f32x4* __restrict__ frags,
                                                 float* __restrict__ partial, int* __restrict__ pcount, int* __restrict__ labels_out, int tpw) {
    CFFM_DYN_SMEM(smem);
    f32x4* F = (f32x4*)smem;                               // the centre fragments
    float* norm_s = (float*)(F + km_frag_words(KT));       // |c_j|^2 in two halves [2][128], 16 KT of 128 used
    int* lab_s = (int*)(norm_s + 256);                     // the chunk's labels (-1 behind row N)
    const int tid = threadIdx.x, lane = tid & 63, wave = wave_uniform(tid >> 6), l15 = lane & 15, g = lane >> 4;
    const int CH = 64 * tpw, base = blockIdx.x * CH;
    const f32x4 z4 = (f32x4){0.f, 0.f, 0.f, 0.f};
    // the first tile's x rows are requested before anything else: the fragment copy and the norms hide their latency
    f32x4 xn[16];
    {
        const int p = km_min(base + 16 * wave * tpw + l15, N - 1);          // (rows behind N: clamped here, zeroed when used)
        const float* xp = x + (long)p * CFFM_C + 4 * g;
#pragma unroll
        for (int i = 0; i < 16; ++i) xn[i] = *(const f32x4*)(xp + 16 * i);
    }
    {   // fragments -> LDS: all 4 KT loads of a thread in flight at once (a rolled loop pays one memory round trip per 4 KiB)
        f32x4 fr[4 * KT];
#pragma unroll
        for (int i = 0; i < 4 * KT; ++i) fr[i] = frags[256 * i + tid];
#pragma unroll
        for (int i = 0; i < 4 * KT; ++i) F[256 * i + tid] = fr[i];
    }
    __syncthreads();
    // |c_j|^2 of the centre the products see (hi + lo): two threads per centre, four k-steps each, fixed order; the halves are added
    // where they are used
    {
        const int cj = tid & 127, half = tid >> 7;
        if (cj < 16 * KT) {
            const int kt = cj >> 4, r = cj & 15;
            float s = 0.f;
#pragma unroll
            for (int k4 = 0; k4 < 4; ++k4)
#pragma unroll
                for (int gg = 0; gg < 4; ++gg) {
                    const int ks = 4 * half + k4;
                    const bf16x8 h = __builtin_bit_cast(bf16x8, F[((kt * 8 + ks) * 2) * 64 + 16 * gg + r]);
                    const bf16x8 l = __builtin_bit_cast(bf16x8, F[((kt * 8 + ks) * 2 + 1) * 64 + 16 * gg + r]);
#pragma unroll
                    for (int e = 0; e < 8; ++e) {
                        const float cv = (float)h[e] + (float)l[e];
                        s = fmaf(cv, cv, s);
                    }
                }
            norm_s[128 * half + cj] = s;
        }
    }
    __syncthreads();

    // ---- assign: wave `wave` owns tiles wave * tpw .. + tpw - 1 of the chunk
    for (int ti = 0; ti < tpw; ++ti) {
        const int tl = 16 * (wave * tpw + ti), t0 = base + tl;
        if (t0 >= N) {                                     // (wave-uniform)
            if (g == 0) lab_s[tl + l15] = -1;
            continue;
        }
        const int p = t0 + l15;
        const bool live = p < N;
        f32x4 xr[16];
#pragma unroll
        for (int i = 0; i < 16; ++i) xr[i] = live ? xn[i] : z4;
        if (ti + 1 < tpw && t0 + 16 < N) {                 // (wave-uniform) the next tile's rows, a tile ahead
            const float* xp = x + (long)km_min(p + 16, N - 1) * CFFM_C + 4 * g;
#pragma unroll
            for (int i = 0; i < 16; ++i) xn[i] = *(const f32x4*)(xp + 16 * i);
        }
        f32x4 c[KT];
#pragma unroll
        for (int kt = 0; kt < KT; ++kt) c[kt] = z4;
#pragma unroll
        for (int ks = 0; ks < 8; ++ks) {
            bf16x8 qh, ql;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float a = xr[2 * ks][e], b = xr[2 * ks + 1][e];
                qh[e] = (bf16)a; ql[e] = (bf16)(a - (float)qh[e]);
                qh[4 + e] = (bf16)b; ql[4 + e] = (bf16)(b - (float)qh[4 + e]);
            }
#pragma unroll
            for (int kt = 0; kt < KT; ++kt) {
                const bf16x8 kh = __builtin_bit_cast(bf16x8, F[((kt * 8 + ks) * 2) * 64 + lane]);
                const bf16x8 kl = __builtin_bit_cast(bf16x8, F[((kt * 8 + ks) * 2 + 1) * 64 + lane]);
                c[kt] = mfma16x16x32_bf16(kh, ql, c[kt]);
                c[kt] = mfma16x16x32_bf16(kl, qh, c[kt]);
                c[kt] = mfma16x16x32_bf16(kh, qh, c[kt]);
            }
        }
        // the lane (point l15) holds centres 16 kt + 4 g + r: ascending index, strict <
        float best = INFINITY;
        int bi = 0x7fffffff;
#pragma unroll
        for (int kt = 0; kt < KT; ++kt) {
            const f32x4 nv = *(const f32x4*)(norm_s + 16 * kt + 4 * g) + *(const f32x4*)(norm_s + 128 + 16 * kt + 4 * g);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int idx = 16 * kt + 4 * g + r;
                const float s = idx < K ? nv[r] - 2.f * c[kt][r] : INFINITY;
                if (s < best) { best = s; bi = idx; }
            }
        }
#pragma unroll
        for (int m = 16; m <= 32; m <<= 1) {
            const float os = __shfl_xor(best, m, 64);
            const int oi = __shfl_xor(bi, m, 64);
            if (os < best || (os == best && oi < bi)) { best = os; bi = oi; }
        }
        if (bi >= K) bi = 0;                               // (only a row of NaNs gets here)
        if (g == 0) {
            lab_s[tl + l15] = live ? bi : -1;
            if (labels_out && live) labels_out[p] = bi;
        }
    }
    // the update's first k-step is requested before the barrier (it does not depend on the labels)
    const float* xc = x + 64 * wave + l15;
    float xv[KM_CT][8];
    if (base < N) km_load_x(xc, N, base, g, xv);
    __syncthreads();
    if (tid < K) {
        int cn = 0;
        for (int i = 0; i < CH; ++i) cn += lab_s[i] == tid;
        pcount[(long)blockIdx.x * K + tid] = cn;
    }

    // ---- update: sums^T [64 channels of the wave x centres] over the chunk, 32 points per k-step; k-slot (g, j) <-> point 8 g + j
    f32x4 acc[KM_CT][KT];
#pragma unroll
    for (int ct = 0; ct < KM_CT; ++ct)
#pragma unroll
        for (int kt = 0; kt < KT; ++kt) acc[ct][kt] = z4;
    for (int s = 0; s < 2 * tpw; ++s) {
        const int p0 = base + 32 * s;
        if (p0 >= N) break;                                // (workgroup-uniform)
        typedef int i32x4 __attribute__((ext_vector_type(4)));
        const i32x4 la = *(const i32x4*)(lab_s + 32 * s + 8 * g), lb = *(const i32x4*)(lab_s + 32 * s + 8 * g + 4);
        bf16x8 xh[KM_CT], xl[KM_CT], xl2[KM_CT];
#pragma unroll
        for (int ct = 0; ct < KM_CT; ++ct) {
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const float v = p0 + 8 * g + j < N ? xv[ct][j] : 0.f;
                const bf16 h = (bf16)v;
                const float r1 = v - (float)h;
                const bf16 l = (bf16)r1;
                xh[ct][j] = h; xl[ct][j] = l; xl2[ct][j] = (bf16)(r1 - (float)l);
            }
        }
        if (s + 1 < 2 * tpw && p0 + 32 < N) km_load_x(xc, N, p0 + 32, g, xv);      // (workgroup-uniform) the next k-step, one ahead
#pragma unroll
        for (int kt = 0; kt < KT; ++kt) {
            const int cj = 16 * kt + l15;
            typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
            u32x4 w;                                        // bf16 1.0 = 0x3F80 where the point carries label cj
            w[0] = (la[0] == cj ? 0x3F80u : 0u) | (la[1] == cj ? 0x3F800000u : 0u);
            w[1] = (la[2] == cj ? 0x3F80u : 0u) | (la[3] == cj ? 0x3F800000u : 0u);
            w[2] = (lb[0] == cj ? 0x3F80u : 0u) | (lb[1] == cj ? 0x3F800000u : 0u);
            w[3] = (lb[2] == cj ? 0x3F80u : 0u) | (lb[3] == cj ? 0x3F800000u : 0u);
            const bf16x8 oh = __builtin_bit_cast(bf16x8, w);
#pragma unroll
            for (int ct = 0; ct < KM_CT; ++ct) {
                acc[ct][kt] = mfma16x16x32_bf16(xl2[ct], oh, acc[ct][kt]);
                acc[ct][kt] = mfma16x16x32_bf16(xl[ct], oh, acc[ct][kt]);
                acc[ct][kt] = mfma16x16x32_bf16(xh[ct], oh, acc[ct][kt]);
            }
        }
    }
    // C register r of lane (l15, g): channel 64 wave + 16 ct + 4 g + r of centre 16 kt + l15
#pragma unroll
    for (int kt = 0; kt < KT; ++kt) {
        const int cj = 16 * kt + l15;
        if (cj < K) {
            float* dst = partial + ((long)blockIdx.x * K + cj) * CFFM_C + 64 * wave + 4 * g;
#pragma unroll
            for (int ct = 0; ct < KM_CT; ++ct) *(f32x4*)(dst + 16 * ct) = acc[ct][kt];
        }
    }
}
