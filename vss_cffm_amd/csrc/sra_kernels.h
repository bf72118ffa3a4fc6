// sra_kernels.h -- the core of MiT's spatial-reduction attention on token rows, forward and backward, exact fp32 on the matrix pipe (gfx950).
//
// The reference (mix_transformer.py Attention.forward) reshapes / permutes q [B,N,C] and kv [B,Nk,2C] into per-head tensors, forms the score
// tensor [B,heads,N,Nk], scales it, takes the soft-max and multiplies by v: the scores are written and re-read by four ops and kept for the
// backward.  Here they never exist: the kernels read q and kv where the two Linear layers left them (head h = columns h hd .. of q, K =
// columns h hd .. and V = columns C + h hd .. of kv) and write out / dq / dkv in the layout the next Linear layers read.  Kept for the backward:
// one log-sum-exp per (image, head, query).
//
// Arithmetic: every product is v_mfma_f32_16x16x4_f32 (mfma16x16x4_f32 of cffm_common.h): f32 operands, a k-ordered chain of f32 fmaf -- the
// numerics of the fp32 op sequence.  Orientation (gtc_kernels.h): keys x queries, S^T = K Q^T, so a lane owns a query (column l15) and the
// soft-max over keys runs over its 4 C registers per key tile and then over the 4 lane groups (two shuffles).  The C/D fragment of S^T
// (register r of lane (l15, g) = key 4 g + r, query l15) IS the B operand of O^T += V^T P^T with k-slot g <-> key 4 g + r: P never goes
// through LDS.  The channel k-slots use the bijection (step s, group g) <-> channel (hd / 4) g + s, so a lane's operand values of one row
// are hd / 4 consecutive floats (16-byte reads, from global memory and from LDS alike).
//
//   k_sra_fwd      a wave owns 16 QW queries of one (image, head); the four waves of a workgroup share a staged tile of SRA_KS keys
//                  (K and V rows, zero-filled past Nk; the next tile is fetched into registers under the products) and walk all keys in
//                  such tiles with an online soft-max on raw scores: running maximum M, p = 2^(c (s - M)), c = scale log2(e), accumulator and sum rescaled by 2^(c (M_old - M_new)) per tile;
//                  keys past Nk carry s = -inf, queries past N are computed on zeros and not stored.  lse = scale M + log(sum).
//   k_sra_bwd_dq   the same tiling: p = 2^(c s - lse log2(e)) (c and lse log2(e) as hi + lo pairs), dP^T = V dO^T, dS^T = P^T (dP^T - delta),
//                  dQ^T += K^T dS^T; delta = rowsum(dout out) is the diagonal of one extra MFMA tile out dO^T -- the same fmaf chain as
//                  dP^T, so a one-key problem gives dq = 0 exactly -- and goes to the workspace for k_sra_bwd_dkv.
//   k_sra_bwd_dkv  a wave owns 16 keys (K and V operands in registers for its whole life), a workgroup 64 keys and one chunk of the queries
//                  of a (image, head); Q and dO rows pass through LDS in tiles of SRA_QB.  The other orientation, S = Q K^T (the same
//                  operand registers, swapped), puts the key on the lane: dV^T += dO^T P and dK^T += Q^T dS take the C fragments as
//                  B operands again.  Each chunk leaves its sums in a slab [B, Nk, 2C] of the workspace;
//   k_sra_dkv_sum  adds the slabs in chunk order.  With one chunk k_sra_bwd_dkv writes dkv itself.
// No atomics: two calls give the same bits.  Every workspace word that is read was written by the same call.
#pragma once
#include "cffm_common.h"
#include <math.h>

#define SRA_KS 64       // keys per LDS stage: 4 MFMA key tiles (forward, dq)
#define SRA_QB 64       // queries per LDS stage of k_sra_bwd_dkv, and the keys of its workgroup

__device__ __forceinline__ f32x4 sra_zero() { return (f32x4){0.f, 0.f, 0.f, 0.f}; }

// A tile of 64 rows of HD floats passes through registers: sra_fetch loads the thread's HD / 16 pieces (row r of the tile = row row0 + r of
// `src`, whose rows are `stride` floats apart; zeros from row `end` on), sra_put stores them to dst[r][HD + 4].  The fetch of the next
// tile is issued before the products of the current one, so its latency hides behind them.
template <int HD>
__device__ __forceinline__ void sra_fetch(f32x4 (&pre)[HD / 16], const float* __restrict__ src, long stride, int row0, int end, int tid) {
    constexpr int Q4 = HD / 4;
#pragma unroll
    for (int i = 0; i < HD / 16; ++i) {
        const int e = tid + 256 * i, r = e / Q4, c4 = e % Q4;
        pre[i] = row0 + r < end ? *(const f32x4*)(src + (long)(row0 + r) * stride + 4 * c4) : sra_zero();
    }
}
template <int HD>
__device__ __forceinline__ void sra_put(float* dst, const f32x4 (&pre)[HD / 16], int tid) {
    constexpr int ST = HD + 4, Q4 = HD / 4;
#pragma unroll
    for (int i = 0; i < HD / 16; ++i) {
        const int e = tid + 256 * i;
        *(f32x4*)(dst + (e / Q4) * ST + 4 * (e % Q4)) = pre[i];
    }
}
// the lane's operand values of one row: floats (HD / 4) g .. + HD / 4 - 1
template <int HD>
__device__ __forceinline__ void sra_row_frag(const float* row, int g, float (&f)[HD / 4]) {
#pragma unroll
    for (int j = 0; j < HD / 16; ++j) {
        const f32x4 v = *(const f32x4*)(row + (HD / 4) * g + 4 * j);
#pragma unroll
        for (int e = 0; e < 4; ++e) f[4 * j + e] = v[e];
    }
}
template <int HD>
__device__ __forceinline__ void sra_row_frag_or_zero(const float* row, bool live, int g, float (&f)[HD / 4]) {
    if (live) sra_row_frag<HD>(row, g, f);
    else {
#pragma unroll
        for (int j = 0; j < HD / 4; ++j) f[j] = 0.f;
    }
}
template <int NS>
__device__ __forceinline__ f32x4 sra_dot(const float (&a)[NS], const float (&b)[NS]) {
    f32x4 c = sra_zero();
#pragma unroll
    for (int s = 0; s < NS; ++s) c = mfma16x16x4_f32(a[s], b[s], c);
    return c;
}
__device__ __forceinline__ float sra_group_sum(float v) {      // over the four lane groups of a column
    v += __shfl_xor(v, 16, 64);
    return v + __shfl_xor(v, 32, 64);
}

// grid (ceil(N / (64 QW)), 1, B heads)
template <int HD, int QW>
__global__ void __launch_bounds__(256) k_sra_fwd(const float* __restrict__ q, const float* __restrict__ kv, float* __restrict__ out,
                                                 float* __restrict__ lse, int N, int Nk, int heads, float scale) {
    constexpr int ST = HD + 4, NS = HD / 4, NC = HD / 16, KT = SRA_KS / 16;
    __shared__ f32x4 Ks4[SRA_KS * ST / 4], Vs4[SRA_KS * ST / 4];
    float* Ks = (float*)Ks4;
    float* Vs = (float*)Vs4;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l15 = lane & 15, g = lane >> 4;
    const int b = blockIdx.z / heads, h = blockIdx.z % heads, C = heads * HD;
    const int n0 = blockIdx.x * (64 * QW) + wave * (16 * QW);
    const float c2 = scale * CFFM_LOG2E;
    const float* kbase = kv + (long)b * Nk * 2 * C + h * HD;
    float qf[QW][NS];
    f32x4 acc[QW][NC];
    float m[QW], l[QW];
#pragma unroll
    for (int w = 0; w < QW; ++w) {
        const int n = n0 + 16 * w + l15;
        sra_row_frag_or_zero<HD>(q + ((long)b * N + (n < N ? n : 0)) * C + h * HD, n < N, g, qf[w]);
#pragma unroll
        for (int ct = 0; ct < NC; ++ct) acc[w][ct] = sra_zero();
        m[w] = -INFINITY;
        l[w] = 0.f;
    }
    f32x4 pk[HD / 16], pv[HD / 16];
    sra_fetch<HD>(pk, kbase, 2 * C, 0, Nk, tid);
    sra_fetch<HD>(pv, kbase + C, 2 * C, 0, Nk, tid);
    for (int k0 = 0; k0 < Nk; k0 += SRA_KS) {
        __syncthreads();
        sra_put<HD>(Ks, pk, tid);
        sra_put<HD>(Vs, pv, tid);
        __syncthreads();
        if (k0 + SRA_KS < Nk) {
            sra_fetch<HD>(pk, kbase, 2 * C, k0 + SRA_KS, Nk, tid);
            sra_fetch<HD>(pv, kbase + C, 2 * C, k0 + SRA_KS, Nk, tid);
        }
        const int nkt = Nk - k0 >= SRA_KS ? KT : (Nk - k0 + 15) / 16;
        f32x4 s[QW][KT];
#pragma unroll
        for (int kt = 0; kt < KT; ++kt) {
            if (kt < nkt) {
                float kf[NS];
                sra_row_frag<HD>(Ks + (16 * kt + l15) * ST, g, kf);
#pragma unroll
                for (int w = 0; w < QW; ++w) {
                    f32x4 c = sra_dot<NS>(kf, qf[w]);
#pragma unroll
                    for (int r = 0; r < 4; ++r)
                        if (k0 + 16 * kt + 4 * g + r >= Nk) c[r] = -INFINITY;
                    s[w][kt] = c;
                }
            } else {
#pragma unroll
                for (int w = 0; w < QW; ++w) s[w][kt] = (f32x4){-INFINITY, -INFINITY, -INFINITY, -INFINITY};
            }
        }
#pragma unroll
        for (int w = 0; w < QW; ++w) {
            float mx = m[w];
#pragma unroll
            for (int kt = 0; kt < KT; ++kt)
#pragma unroll
                for (int r = 0; r < 4; ++r) mx = fmaxf(mx, s[w][kt][r]);
            mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
            mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
            const float alpha = fast_exp2(c2 * (m[w] - mx));      // (0 at the first tile: m = -inf, mx finite -- a tile has a live key)
            m[w] = mx;
            float ps = 0.f;
#pragma unroll
            for (int kt = 0; kt < KT; ++kt)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float p = fast_exp2(c2 * (s[w][kt][r] - mx));
                    s[w][kt][r] = p;
                    ps += p;
                }
            l[w] = l[w] * alpha + ps;                                // (the lane's keys only: the groups are added at the end)
#pragma unroll
            for (int ct = 0; ct < NC; ++ct) acc[w][ct] *= alpha;
        }
#pragma unroll
        for (int kt = 0; kt < KT; ++kt) {
            if (kt < nkt) {
#pragma unroll
                for (int ct = 0; ct < NC; ++ct)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const float vt = Vs[(16 * kt + 4 * g + r) * ST + 16 * ct + l15];
#pragma unroll
                        for (int w = 0; w < QW; ++w) acc[w][ct] = mfma16x16x4_f32(vt, s[w][kt][r], acc[w][ct]);
                    }
            }
        }
    }
#pragma unroll
    for (int w = 0; w < QW; ++w) {
        const int n = n0 + 16 * w + l15;
        const float lt = sra_group_sum(l[w]);
        if (n < N) {
            const float inv = 1.0f / lt;
            float* o = out + ((long)b * N + n) * C + h * HD + 4 * g;
#pragma unroll
            for (int ct = 0; ct < NC; ++ct) *(f32x4*)(o + 16 * ct) = acc[w][ct] * inv;
            // (in double: lse is a dozen ulps of its own size away from the scores' noise, one rounding is all it should add)
            if (lse && g == 0) lse[((long)b * heads + h) * N + n] = (float)((double)m[w] * (double)scale + log((double)lt));
        }
    }
}

// 2^(c s - lse log2 e) with c = chi + clo and lse log2 e = lhi + llo
__device__ __forceinline__ float sra_prob(float s, float chi, float clo, float lhi, float llo) {
    return fast_exp2(fmaf(s, chi, -lhi) + fmaf(s, clo, -llo));
}

// grid (ceil(N / (64 QW)), 1, B heads); delta [B, heads, N]
template <int HD, int QW>
__global__ void __launch_bounds__(256) k_sra_bwd_dq(const float* __restrict__ q, const float* __restrict__ kv, const float* __restrict__ out,
                                                    const float* __restrict__ lse, const float* __restrict__ dout, float* __restrict__ dq,
                                                    float* __restrict__ delta, int N, int Nk, int heads, float scale, float chi, float clo) {
    constexpr int ST = HD + 4, NS = HD / 4, NC = HD / 16, KT = SRA_KS / 16;
    __shared__ f32x4 Ks4[SRA_KS * ST / 4], Vs4[SRA_KS * ST / 4];
    float* Ks = (float*)Ks4;
    float* Vs = (float*)Vs4;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l15 = lane & 15, g = lane >> 4;
    const int b = blockIdx.z / heads, h = blockIdx.z % heads, C = heads * HD;
    const int n0 = blockIdx.x * (64 * QW) + wave * (16 * QW);
    const float* kbase = kv + (long)b * Nk * 2 * C + h * HD;
    float qf[QW][NS], df[QW][NS];
    f32x4 acc[QW][NC];
    float dl[QW], lhi[QW], llo[QW];
#pragma unroll
    for (int w = 0; w < QW; ++w) {
        const int n = n0 + 16 * w + l15;
        const bool live = n < N;
        const long row = ((long)b * N + (live ? n : 0)) * C + h * HD;
        sra_row_frag_or_zero<HD>(q + row, live, g, qf[w]);
        sra_row_frag_or_zero<HD>(dout + row, live, g, df[w]);
        {   // delta of query l15 = entry (l15, l15) of out dO^T: row 4 g + r of lane group g
            float of[NS];
            sra_row_frag_or_zero<HD>(out + row, live, g, of);
            const f32x4 c = sra_dot<NS>(of, df[w]);
            const int r = l15 & 3;
            const float d = r == 0 ? c[0] : r == 1 ? c[1] : r == 2 ? c[2] : c[3];
            dl[w] = sra_group_sum(g == (l15 >> 2) ? d : 0.f);
        }
        const float ls = live ? lse[((long)b * heads + h) * N + n] : 0.f;
        lhi[w] = ls * CFFM_LOG2E;
        llo[w] = fmaf(ls, CFFM_LOG2E, -lhi[w]);
        if (live && g == 0) delta[((long)b * heads + h) * N + n] = dl[w];
#pragma unroll
        for (int ct = 0; ct < NC; ++ct) acc[w][ct] = sra_zero();
    }
    f32x4 pk[HD / 16], pv[HD / 16];
    sra_fetch<HD>(pk, kbase, 2 * C, 0, Nk, tid);
    sra_fetch<HD>(pv, kbase + C, 2 * C, 0, Nk, tid);
    for (int k0 = 0; k0 < Nk; k0 += SRA_KS) {
        __syncthreads();
        sra_put<HD>(Ks, pk, tid);
        sra_put<HD>(Vs, pv, tid);
        __syncthreads();
        if (k0 + SRA_KS < Nk) {
            sra_fetch<HD>(pk, kbase, 2 * C, k0 + SRA_KS, Nk, tid);
            sra_fetch<HD>(pv, kbase + C, 2 * C, k0 + SRA_KS, Nk, tid);
        }
        const int nkt = Nk - k0 >= SRA_KS ? KT : (Nk - k0 + 15) / 16;
#pragma unroll
        for (int kt = 0; kt < KT; ++kt) {
            if (kt < nkt) {
                f32x4 ds[QW];
                {
                    float kf[NS], vf[NS];
                    sra_row_frag<HD>(Ks + (16 * kt + l15) * ST, g, kf);
                    sra_row_frag<HD>(Vs + (16 * kt + l15) * ST, g, vf);
#pragma unroll
                    for (int w = 0; w < QW; ++w) {
                        const f32x4 s = sra_dot<NS>(kf, qf[w]), dp = sra_dot<NS>(vf, df[w]);
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            const float p = k0 + 16 * kt + 4 * g + r < Nk ? sra_prob(s[r], chi, clo, lhi[w], llo[w]) : 0.f;
                            ds[w][r] = p * (dp[r] - dl[w]);
                        }
                    }
                }
#pragma unroll
                for (int ct = 0; ct < NC; ++ct)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const float kt_ = Ks[(16 * kt + 4 * g + r) * ST + 16 * ct + l15];
#pragma unroll
                        for (int w = 0; w < QW; ++w) acc[w][ct] = mfma16x16x4_f32(kt_, ds[w][r], acc[w][ct]);
                    }
            }
        }
    }
#pragma unroll
    for (int w = 0; w < QW; ++w) {
        const int n = n0 + 16 * w + l15;
        if (n < N) {
            float* o = dq + ((long)b * N + n) * C + h * HD + 4 * g;
#pragma unroll
            for (int ct = 0; ct < NC; ++ct) *(f32x4*)(o + 16 * ct) = acc[w][ct] * scale;
        }
    }
}

// grid (ceil(Nk / 64), chunks, B heads): chunk y takes the 16-query tiles y tpc .. y tpc + tpc - 1 (tpc a multiple of 4) and writes
// slab[y][B, Nk, 2C] (`slab_stride` floats apart), both halves of every key row of its head
template <int HD>
__global__ void __launch_bounds__(256) k_sra_bwd_dkv(const float* __restrict__ q, const float* __restrict__ kv, const float* __restrict__ lse,
                                                     const float* __restrict__ dout, const float* __restrict__ delta, float* __restrict__ slab,
                                                     long slab_stride, int tpc, int N, int Nk, int heads, float scale, float chi, float clo) {
    constexpr int ST = HD + 4, NS = HD / 4, NC = HD / 16, QT = SRA_QB / 16;
    __shared__ f32x4 Qs4[SRA_QB * ST / 4], Ds4[SRA_QB * ST / 4], Ls4[SRA_QB / 4], Dl4[SRA_QB / 4];
    float* Qs = (float*)Qs4;
    float* Ds = (float*)Ds4;
    float* Ls = (float*)Ls4;
    float* Dl = (float*)Dl4;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l15 = lane & 15, g = lane >> 4;
    const int b = blockIdx.z / heads, h = blockIdx.z % heads, C = heads * HD;
    const int key = blockIdx.x * SRA_QB + wave * 16 + l15;
    const bool klive = key < Nk;
    float kf[NS], vf[NS];
    {
        const float* krow = kv + ((long)b * Nk + (klive ? key : 0)) * 2 * C + h * HD;
        sra_row_frag_or_zero<HD>(krow, klive, g, kf);
        sra_row_frag_or_zero<HD>(krow + C, klive, g, vf);
    }
    f32x4 dk[NC], dv[NC];
#pragma unroll
    for (int ct = 0; ct < NC; ++ct) dk[ct] = dv[ct] = sra_zero();
    const long first = (long)blockIdx.y * tpc * 16, last = first + (long)tpc * 16;
    const int end = (int)(last < N ? last : N);
    const float* qbase = q + (long)b * N * C + h * HD;
    const float* dbase = dout + (long)b * N * C + h * HD;
    const long sbase = ((long)b * heads + h) * N;
    f32x4 pq[HD / 16], pd[HD / 16];
    float pl = 0.f, pdl = 0.f;
    auto fetch = [&](int n0) {
        sra_fetch<HD>(pq, qbase, C, n0, end, tid);
        sra_fetch<HD>(pd, dbase, C, n0, end, tid);
        const bool live = tid < SRA_QB && n0 + tid < end;
        pl = live ? lse[sbase + n0 + tid] : 0.f;
        pdl = live ? delta[sbase + n0 + tid] : 0.f;
    };
    if ((int)first < end) fetch((int)first);
    for (int n0 = (int)first; n0 < end; n0 += SRA_QB) {
        __syncthreads();
        sra_put<HD>(Qs, pq, tid);
        sra_put<HD>(Ds, pd, tid);
        if (tid < SRA_QB) {
            Ls[tid] = pl;
            Dl[tid] = pdl;
        }
        __syncthreads();
        if (n0 + SRA_QB < end) fetch(n0 + SRA_QB);
        const int nqt = end - n0 >= SRA_QB ? QT : (end - n0 + 15) / 16;
#pragma unroll
        for (int qt = 0; qt < QT; ++qt) {
            if (qt < nqt) {
                f32x4 p, ds;
                {
                    float qf[NS], df[NS];
                    sra_row_frag<HD>(Qs + (16 * qt + l15) * ST, g, qf);
                    sra_row_frag<HD>(Ds + (16 * qt + l15) * ST, g, df);
                    const f32x4 s = sra_dot<NS>(qf, kf), dp = sra_dot<NS>(df, vf);        // rows = queries 4 g + r, column = key l15
                    const f32x4 ls = *(const f32x4*)(Ls + 16 * qt + 4 * g), dl = *(const f32x4*)(Dl + 16 * qt + 4 * g);
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const float lhi = ls[r] * CFFM_LOG2E, llo = fmaf(ls[r], CFFM_LOG2E, -lhi);
                        p[r] = (klive && n0 + 16 * qt + 4 * g + r < end) ? sra_prob(s[r], chi, clo, lhi, llo) : 0.f;
                        ds[r] = p[r] * (dp[r] - dl[r]);
                    }
                }
#pragma unroll
                for (int ct = 0; ct < NC; ++ct)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int o = (16 * qt + 4 * g + r) * ST + 16 * ct + l15;
                        dv[ct] = mfma16x16x4_f32(Ds[o], p[r], dv[ct]);
                        dk[ct] = mfma16x16x4_f32(Qs[o], ds[r], dk[ct]);
                    }
            }
        }
    }
    if (klive) {
        float* o = slab + (long)blockIdx.y * slab_stride + ((long)b * Nk + key) * 2 * C + h * HD + 4 * g;
#pragma unroll
        for (int ct = 0; ct < NC; ++ct) {
            *(f32x4*)(o + 16 * ct) = dk[ct] * scale;
            *(f32x4*)(o + C + 16 * ct) = dv[ct];
        }
    }
}

// dkv = slab[0] + slab[1] + ... in this order; n4 = B Nk 2C / 4
__global__ void __launch_bounds__(256) k_sra_dkv_sum(const f32x4* __restrict__ slab, f32x4* __restrict__ dkv, long n4, long stride4, int chunks) {
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long)gridDim.x * 256) {
        f32x4 v = slab[i];
        for (int c = 1; c < chunks; ++c) v += slab[c * stride4 + i];
        dkv[i] = v;
    }
}
