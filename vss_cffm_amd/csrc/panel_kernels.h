// panel_kernels.h -- "row panel" Linear GEMMs: one workgroup owns 16*MT complete rows of the activation matrix.
//
// Why a second GEMM form (round 3).  At CFFM-B1 sizes the Linear layers are small for this chip (M = 7200 token rows, N / K in
// {256, 768, 1024}: 28 rows per CU): the tiled kernels of gemm_kernels.h run 64x64 tiles that re-stage BOTH operands through
// LDS with one barrier per 32-deep K-tile and reach 9-17 % of the three-pass bf16 peak.  Here the activation operand of a
// workgroup (a panel of 32 or 48 rows x the whole contraction) is staged ONCE into LDS as hi / lo bf16 images, and the weight
// operand never touches LDS at all: k_param_prep leaves a copy of every weight in MFMA-FRAGMENT ORDER (16 output features x 32
// contraction steps per 2 KiB unit: 64 lanes x {8 bf16 hi | 8 bf16 lo}), so that a wave fetches its B fragments with fully
// coalesced 1 KiB buffer loads straight into registers, a ring of D k-steps ahead of the MFMAs.  The K-loop has no barrier
// (one per 256-deep chunk of the contraction, for the double-buffered panel image), every wave streams on its own, and a
// whole output row lives in one workgroup -- which is what lets residual + LayerNorm + the next Linear follow in the same
// kernel (fused forms below).  Products are computed transposed (D = W_frag x X_frag^T), so a lane ends up with 4 consecutive
// output features of one row: 16-byte stores, and 8-byte hi / lo stores when the result is the next GEMM's panel image.
#pragma once
#include "cffm_common.h"
#include "gemm_kernels.h"
#include "dws_kernels.h"

#define PNL_KC 256          // contraction chunk held in LDS (floats per row)
#define PNL_THREADS 512     // 8 waves: two per SIMD
#define PNL_WAVES 8
// bf16 element offset of 16-byte chunk `chunk` (8 k) of panel row `row` inside a [rows][256] image: the chunk index is XOR-ed
// with the row so that the 16-lane groups a ds_read_b128 is served in ({0-3,12-15,20-27}, {4-11,16-19,28-31}, ...: rows x two
// adjacent k-chunks) cover the 16 bank quads exactly once (checked exhaustively in tests/test_geometry.py)
__device__ __forceinline__ int pnl_off(int row, int chunk) { return row * PNL_KC + (((chunk ^ row) & 15) << 3) + ((chunk & 16) << 3); }
#define PNL_IMG(MT) (16 * (MT) * PNL_KC)                       // bf16 elements of one image
#define PNL_LDS(MT) (2 * 2 * PNL_IMG(MT) * 2 + 2 * PNL_THREADS * 16)   // bytes: double-buffered {hi, lo} + the column-sum exchange (k_panel_gemm colrec)

// index (in 16-byte units) of the fragment of output tile jt, k-step ks, half h (0 hi, 1 lo) in a fragment-ordered weight
__device__ __host__ __forceinline__ long pnl_frag_unit(int jt, int ks, int h, int KS) { return ((long)(jt * KS + ks) * 2 + h) * 64; }

// Fragment-ordered copy of a weight for the two uses:
//   NT form (forward, y = x W^T, W [N][K]):        out feature n = 16 jt + l15, contraction k = 32 ks + 8 g + e  -> W[n][k]
//   NN form (input gradient, dx = dy W, W [N][K]): out feature k' = 16 jt + l15, contraction n = 32 ks + 8 g + e -> W[n][k']
// one thread per (unit lane): writes 16 B hi + 16 B lo
__device__ __forceinline__ void pnl_pack_weight(const float* __restrict__ W, int N, int K, bool nn, f32x4* __restrict__ dst, long item) {
    const int lane = (int)(item & 63);
    const long u = item >> 6;
    const int OUT = nn ? K : N, KS = (nn ? N : K) / 32;
    const int ks = (int)(u % KS), jt = (int)(u / KS);
    if (jt * 16 >= OUT) return;
    const int l15 = lane & 15, g = lane >> 4;
    bf16x8 hi, lo;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const int o = 16 * jt + l15, c = 32 * ks + 8 * g + e;
        const float x = nn ? W[(long)c * K + o] : W[(long)o * K + c];
        hi[e] = (bf16)x;
        lo[e] = (bf16)(x - (float)hi[e]);
    }
    dst[pnl_frag_unit(jt, ks, 0, KS) + lane] = __builtin_bit_cast(f32x4, hi);
    dst[pnl_frag_unit(jt, ks, 1, KS) + lane] = __builtin_bit_cast(f32x4, lo);
}
__global__ void __launch_bounds__(256) k_pnl_pack_weight(const float* __restrict__ W, int N, int K, int nn, f32x4* __restrict__ dst) {
    const long item = (long)blockIdx.x * 256 + threadIdx.x;
    if (item < (long)N * K / 8) pnl_pack_weight(W, N, K, nn != 0, dst, item);
}

// up to four weights in one launch (the CFFM++ block packs q | proj_cluster | fc1 | fc2 per direction)
struct PnlPackJobs { const float* w[4]; f32x4* dst[4]; int N[4], K[4]; long end[4]; int n, nn; };
__global__ void __launch_bounds__(256) k_pnl_pack_weights(PnlPackJobs J) {
    long item = (long)blockIdx.x * 256 + threadIdx.x;
    int j = 0;
#pragma unroll
    for (int q = 0; q < 3; ++q)
        if (q + 1 < J.n && item >= J.end[q]) j = q + 1;
    if (j > 0) item -= J.end[j - 1];
    if (item < (long)J.N[j] * J.K[j] / 8) pnl_pack_weight(J.w[j], J.N[j], J.K[j], J.nn != 0, J.dst[j], item);
}

// Workgroup barrier that orders LDS traffic only.  __syncthreads() is a release / acquire of ALL memory: on gfx9 it waits vmcnt(0),
// i.e. for every global store issued so far to be acknowledged AND for the whole B-fragment ring that is in flight -- measured on the
// fused forward kernel: 44.6 us with __syncthreads(), of which 20 us were the (seven times drained) stores.
__device__ __forceinline__ void pnl_lds_barrier() {
#ifdef CFFM_EMU
    __syncthreads();
#else
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
#endif
}

// ---- panel staging: global -> registers -> LDS images -------------------------------------------------------------------
template <int MT>
struct PnlStage { f32x4 v[2 * MT]; };
// rows m0 .. m0+16MT-1, floats [kc0, kc0+256) of each; rows >= M read as zeros (buffer bounds)
template <int MT>
__device__ __forceinline__ void pnl_stage_load(PnlStage<MT>& r, buf_t rs, int lda, int m0, int kc0, int tid) {
#pragma unroll
    for (int it = 0; it < 2 * MT; ++it) {
        const int item = tid + PNL_THREADS * it, row = item >> 6, c4 = item & 63;
        r.v[it] = buf_ld16(rs, (uint32_t)((row * lda + 4 * c4) * 4), (uint32_t)(((long)m0 * lda + kc0) * 4));
    }
}
template <int MT, bool PRE>
__device__ __forceinline__ void pnl_stage_store(const PnlStage<MT>& r, bf16* __restrict__ hi, bf16* __restrict__ lo, int tid) {
#pragma unroll
    for (int it = 0; it < 2 * MT; ++it) {
        const int item = tid + PNL_THREADS * it, row = item >> 6, c4 = item & 63;
        bf16x4 h, l;
        if (PRE) unsplit4(r.v[it], h, l);
        else split4(r.v[it], h, l);
        const int o = pnl_off(row, c4 >> 1) + 4 * (c4 & 1);
        *(bf16x4*)(hi + o) = h;
        *(bf16x4*)(lo + o) = l;
    }
}

// ---- the streaming product of one 256-deep chunk --------------------------------------------------------------------------
// acc[t][i] += W_frag(tile jt0 + t, k-steps ks0 .. ks0+7) x panel(rows 16 i .., chunk image)^T for t < NTW, in passes of NT tiles.
// B ring: D k-steps of NT tiles x {hi, lo} in registers; the loads of step s + D are issued while step s is multiplied.
// The ring runs across passes, chunks and (for the fused kernels) across GEMMs: `next` tells where the stream continues.
template <int NT, int D>
struct PnlRing { f32x4 v[D][NT][2]; };

struct PnlStream {       // position of a wave's B stream: base unit of (jt, ks) = (jt0, 0) and the k-steps per tile
    buf_t rs;
    uint32_t voff;       // lane * 16
    int KS;              // k-steps of 32 per output tile in this weight
};
template <int NT, int D>
__device__ __forceinline__ void pnl_ring_load(PnlRing<NT, D>& ring, int slot, const PnlStream& st, int jt, int ks) {
#pragma unroll
    for (int j = 0; j < NT; ++j)
#pragma unroll
        for (int h = 0; h < 2; ++h)
            ring.v[slot][j][h] = buf_ld16(st.rs, st.voff, (uint32_t)(pnl_frag_unit(jt + j, ks, h, st.KS) * 16));
}

// VMEM issue points are pinned per step (everything else may be scheduled across): left alone, hipcc sinks every prefetch down to
// its first use and waits vmcnt(0) there, i.e. no prefetch at all (round-3 ISA dump: 26 us instead of 10 for fc1)
__device__ __forceinline__ void pnl_pin_vmem() {
#ifndef CFFM_EMU
    __builtin_amdgcn_sched_barrier(0);
#endif
}
// Invariant at entry: the ring holds steps 0 .. D-2 of this chunk (slot = step % D); at exit: steps 0 .. D-2 of what follows.
// `extra(sc)`: the caller's own memory traffic of step sc (deferred epilogue stores, operand prefetches), issued at the step's pinned
// VMEM point.  Why: a CU's vector-memory path is one in-order queue -- a burst of epilogue stores (64 KiB per workgroup and chunk in the
// fused forward) that drains at the HBM write rate (~6.5 B/clk per CU with every CU storing) holds up the B-fragment loads queued behind
// it, and the matrix pipe idles: measured 44.6 us for the fused forward with the stores in bursts vs 24.4 us without any store.
struct PnlNoExtra { __device__ __forceinline__ void operator()(int) const {} };
// LAST: nothing follows this chunk -- the ring is not refilled past it (`nst` is not read)
template <int MT, int NTW, int NT, int D, class Extra = PnlNoExtra, bool LAST = false>
__device__ __forceinline__ void pnl_chunk_mma(f32x4 (&acc)[NTW][MT], PnlRing<NT, D>& ring, const bf16* __restrict__ Ahi,
                                              const bf16* __restrict__ Alo, const PnlStream& st, int jt0, int ks0, int l15, int g,
                                              // where the stream goes after this chunk (its first D-1 steps are prefetched from here)
                                              const PnlStream& nst, int njt0, int nks0, const Extra& extra = Extra()) {
    constexpr int NPASS = NTW / NT, SC = NPASS * 8;
    static_assert(NTW % NT == 0 && SC % D == 0 && D <= SC && D >= 2, "ring depth must divide the steps of a chunk");
    bf16x8 ah[2][MT], al[2][MT];
#pragma unroll
    for (int i = 0; i < MT; ++i) {
        ah[0][i] = *(const bf16x8*)(Ahi + pnl_off(16 * i + l15, g));
        al[0][i] = *(const bf16x8*)(Alo + pnl_off(16 * i + l15, g));
    }
#pragma unroll
    for (int sc = 0; sc < SC; ++sc) {
        const int p = sc / 8, cur = sc & 1;
        // the slot consumed by the previous step takes step sc + D - 1 (of this chunk, or of what follows it)
        const int sn = sc + D - 1, slot_n = sn % D;
        if (sn < SC) pnl_ring_load<NT, D>(ring, slot_n, st, jt0 + (sn / 8) * NT, ks0 + sn % 8);
        else if (!LAST) pnl_ring_load<NT, D>(ring, slot_n, nst, njt0 + ((sn - SC) / 8) * NT, nks0 + (sn - SC) % 8);
        extra(sc);
        pnl_pin_vmem();
        if (sc + 1 < SC) {
            const int k8n = (sc + 1) % 8;
#pragma unroll
            for (int i = 0; i < MT; ++i) {
                ah[cur ^ 1][i] = *(const bf16x8*)(Ahi + pnl_off(16 * i + l15, 4 * k8n + g));
                al[cur ^ 1][i] = *(const bf16x8*)(Alo + pnl_off(16 * i + l15, 4 * k8n + g));
            }
        }
        const int slot = sc % D;
#pragma unroll
        for (int j = 0; j < NT; ++j) {
            const bf16x8 bh = __builtin_bit_cast(bf16x8, ring.v[slot][j][0]), bl = __builtin_bit_cast(bf16x8, ring.v[slot][j][1]);
#pragma unroll
            for (int i = 0; i < MT; ++i) {
                f32x4 c = acc[p * NT + j][i];
                c = mfma16x16x32_bf16(bh, al[cur][i], c);
                c = mfma16x16x32_bf16(bl, ah[cur][i], c);
                c = mfma16x16x32_bf16(bh, ah[cur][i], c);
                acc[p * NT + j][i] = c;
            }
        }
    }
}

// ---- T-frag copies of a panel image (dws_kernels.h: the operand order of the streaming weight-gradient kernel) ---------------------------
// The hi / lo images [16 MT rows][256 columns] of a panel hold 16 MT / 8 row groups of 8 token rows; unit (k-step, column tile jt, h) of the
// T-frag array wants, in lane (l15, g), rows 8 g .. 8 g + 7 of column 16 jt + l15: two transposed LDS reads (ds_read_b64_tr_b16: inside a
// group of 16 lanes, lane i points at 4 contiguous columns 4 (i & 3) of row (i >> 2) and receives column (i & 15) of the 4 rows) and one
// 16-byte store per lane -- 256 contiguous bytes per 16-lane group, a whole 1 KiB unit per wave instruction when the panel is a k-step.
// `m0`: first token row of the panel (a multiple of 8); `jt0`: first column tile of the image in the array; `CT`: column tiles of the
// array; `R`: token rows that exist (rows past R are written as zeros: an image row of a COMPUTED panel past the end holds finite
// garbage); `R32`: rows of the array (R rounded up to 32; row groups past it are not written).  Wave-collective; call between the
// barrier that publishes the image and the one that lets it be overwritten.
template <int MT>
__device__ __forceinline__ void pnl_tfrag_store(const bf16* __restrict__ hi, const bf16* __restrict__ lo, f32x4* __restrict__ dst, int m0, int jt0, int CT,
                                                long R, long R32, int wave, int lane) {
    const int l15 = lane & 15, g = lane >> 4;
    constexpr int NRG = 2 * MT, NOP = (NRG + 3) / 4;      // row groups of the panel, wave operations per unit
#pragma unroll
    for (int q = 0; q < 32 * NOP / PNL_WAVES; ++q) {
        const int item = wave + PNL_WAVES * q;           // (unit, operation): units 0..31 = (column tile, h)
        const int u = item / NOP, op = item % NOP, jt = u >> 1, h = u & 1;
        const int rgl = 4 * op + g;                      // row group of the panel this 16-lane group transposes
        const bf16* img = h ? lo : hi;
        const int row = 8 * (rgl < NRG ? rgl : 0) + (l15 >> 2), col = 16 * jt + 4 * (l15 & 3);
        const bf16x4 a = lds_tr4_bf16(img + pnl_off(row, col >> 3) + (col & 4));
        const bf16x4 b = lds_tr4_bf16(img + pnl_off(row + 4, col >> 3) + (col & 4));
        const long rg = (long)(m0 >> 3) + rgl, r0 = 8 * rg;
        bf16x8 f;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            f[e] = r0 + e < R ? a[e] : (bf16)0.f;
            f[4 + e] = r0 + 4 + e < R ? b[e] : (bf16)0.f;
        }
        // A 48-row panel (MT = 3) is one and a half k-steps: when the LAST panel ends inside a k-step (M mod 96 in 33..48) the row groups
        // between its end and R32 belong to nobody, and the streaming kernel contracts over them ("rows >= R are zeros") -- the last
        // workgroup writes them too (at most two groups: rgl 6, 7 of its second operation; r0 >= R there, so f is all zeros).
        const bool tail = (NRG % 4 != 0) && rgl >= NRG && (long)m0 + 16 * MT >= R;
        if ((rgl < NRG || tail) && r0 < R32) dst[tfrag_unit(rg >> 2, jt0 + jt, h, CT) + 16 * (int)(rg & 3) + l15] = __builtin_bit_cast(f32x4, f);
    }
}

// L2 warm-up of a fragment-ordered weight at the start of a fused kernel.  Every workgroup streams ALL of the block's weights (2.4 MB);
// when nobody has read them since k_param_prep wrote them at the start of the step they sit in HBM, and the B ring (D k-steps = 16 KB
// per wave in flight) cannot cover that latency: the second block's fused forward took 62 us against 42 for the first, whose weights
// had just been written (round-3 timeline; with the second block pointed at the FIRST block's weights both took 42; same-box A/B of
// the whole step: 0.758-0.771 ms without the warm-up, 0.715-0.731 with it; the fused backward 64 -> 51-55 us).  So the
// workgroups that share an L2 (blockIdx.x % 8: workgroups go round-robin over the 8 XCDs) each request one 16-byte word of a
// different 128-byte line -- one load per thread and weight, all in flight together with the first panel -- which pulls the whole
// weight into that XCD's L2 (and the memory-side cache) one round trip after the kernel starts.  A hint only: grids under 128
// workgroups do not cover every line.  The loaded words are XOR-ed into a value that is kept (a never-taken store at the end of the
// kernel) so that the loads cannot be dropped.
__device__ __forceinline__ uint32_t pnl_l2_touch(const void* w, long bytes, int tid) {
    const long nlines = bytes >> 7;
    const int nsl = (int)(gridDim.x >> 3) > 0 ? (int)(gridDim.x >> 3) : 1, rank = (int)(blockIdx.x >> 3) % nsl;
    const long per = (nlines + nsl - 1) / nsl, l = rank * per + tid;
    return (tid < per && l < nlines) ? *(const uint32_t*)((const char*)w + (l << 7)) : 0u;
}
// (the fused kernels always warm the L2 with their fc1 / fc2 / proj weights; the plain panel GEMMs -- q|k|v: 0.75 MB of weights -- do not:
//  no difference measured, 0.719-0.727 ms per step with, 0.715-0.731 without)
// ---- plain panel GEMM: C[M][N] = A[M][K] W^T (+ bias), W in fragment order (NT or NN form decides what "W^T" means) ---------
// grid = ceil(M / (16 MT)) workgroups of 512 threads; N = 8 waves x NTW tiles x 16; K a multiple of 256.
// EPI: 0 plain fp32 (+bias) -- the only epilogue left: the q|k|v forward, once EPI 3 here, is k_panel_qkv3 below
template <int MT, int NTW, int NT, int D, bool A_PRE, int EPI>
__global__ void __launch_bounds__(PNL_THREADS) k_panel_gemm(const float* __restrict__ A, int lda, int M, int K, const f32x4* __restrict__ Wf,
                                                            float* __restrict__ C, int ldc, const float* __restrict__ bias,
                                                            float* __restrict__ colrec = nullptr,
                                                            f32x4* __restrict__ a_t = nullptr /* T-frag copy of A [M][K] (pnl_tfrag_store), or NULL */) {
    CFFM_DYN_SMEM(smem);
    bf16* img = (bf16*)smem;     // [buf][hi | lo][16 MT][256]
    // colrec (fp32 A only): record blockIdx.x [K] = the column sums of this workgroup's 16 MT rows of A -- the bias gradient of the
    // Linear whose output gradient A is, out of the registers the panel is staged through (no second pass over A).  A thread stages
    // the same four columns of 2 MT rows (pnl_stage_load); the eight waves' partial sums meet in LDS behind the chunk's barrier
    f32x4* csum = (f32x4*)(img + 4 * PNL_IMG(MT));     // [2][8 waves][64 lanes]
#define PNL_COLSUM_PUT(c_)                                                                        \
    if (!A_PRE && colrec) {                                                                       \
        f32x4 s_ = sr.v[0];                                                                       \
        _Pragma("unroll") for (int it = 1; it < 2 * MT; ++it) s_ += sr.v[it];                     \
        csum[((c_) & 1) * PNL_THREADS + tid] = s_;                                                \
    }
#define PNL_COLSUM_GET(c_)                                                                        \
    if (!A_PRE && colrec && wave == ((c_) & 7)) {                                                 \
        const f32x4* p_ = csum + ((c_) & 1) * PNL_THREADS + lane;                                 \
        f32x4 t_ = p_[0];                                                                         \
        _Pragma("unroll") for (int w = 1; w < PNL_WAVES; ++w) t_ += p_[64 * w];                   \
        *(f32x4*)(colrec + (long)blockIdx.x * K + (c_) * PNL_KC + 4 * lane) = t_;                 \
    }
    const int tid = threadIdx.x, lane = tid & 63, wave = wave_uniform(tid >> 6), l15 = lane & 15, g = lane >> 4;
    const int m0 = blockIdx.x * 16 * MT;
    const int NCH = K / PNL_KC, KS = K / 32, N = PNL_WAVES * NTW * 16;
    const buf_t rsa = buf_make(A, (uint32_t)((long)M * lda * 4));
    PnlStream st;
    st.rs = buf_make(Wf, (uint32_t)((long)N * K * 4));
    st.voff = lane * 16;
    st.KS = KS;
    const int jt0 = wave * NTW;
    f32x4 acc[NTW][MT];
#pragma unroll
    for (int t = 0; t < NTW; ++t)
#pragma unroll
        for (int i = 0; i < MT; ++i) acc[t][i] = (f32x4){0.f, 0.f, 0.f, 0.f};
    PnlRing<NT, D> ring;
#pragma unroll
    for (int s = 0; s < D - 1; ++s) pnl_ring_load<NT, D>(ring, s, st, jt0 + (s / 8) * NT, s % 8);
    pnl_pin_vmem();
    PnlStage<MT> sr;
    pnl_stage_load<MT>(sr, rsa, lda, m0, 0, tid);
    pnl_stage_store<MT, A_PRE>(sr, img, img + PNL_IMG(MT), tid);
    PNL_COLSUM_PUT(0)
    if (NCH > 1) pnl_stage_load<MT>(sr, rsa, lda, m0, PNL_KC, tid);
    pnl_lds_barrier();
    for (int c = 0; c < NCH; ++c) {
        PNL_COLSUM_GET(c)
        const bf16* hi = img + (c & 1) * 2 * PNL_IMG(MT);
        pnl_chunk_mma<MT, NTW, NT, D>(acc, ring, hi, hi + PNL_IMG(MT), st, jt0, 8 * c, l15, g, st, jt0, 8 * (c + 1));
        // T-frag copy of this chunk BEHIND its product (the image stays until the chunk after next is staged): in front of it the 48 KB of
        // stores hold up the B-fragment loads queued behind them (q|k|v forward 24 -> 31 us); spread over the product's steps
        // the transposed reads stall the MFMA stream instead (q|k|v input gradient 28 -> 42 us, burst in front: 31)
        if (a_t) pnl_tfrag_store<MT>(hi, hi + PNL_IMG(MT), a_t, m0, 16 * c, K / 16, M, ((long)M + 31) / 32 * 32, wave, lane);
        if (c + 1 < NCH) {
            bf16* nx = img + ((c + 1) & 1) * 2 * PNL_IMG(MT);
            pnl_stage_store<MT, A_PRE>(sr, nx, nx + PNL_IMG(MT), tid);
            PNL_COLSUM_PUT(c + 1)
            if (c + 2 < NCH) pnl_stage_load<MT>(sr, rsa, lda, m0, (c + 2) * PNL_KC, tid);
            pnl_lds_barrier();
        }
    }
#undef PNL_COLSUM_PUT
#undef PNL_COLSUM_GET
    // epilogue: acc[t][i][r] = C[m0 + 16 i + l15][16 (jt0 + t) + 4 g + r]
    {
        // Through LDS: a lane of the MFMA C layout owns 4 consecutive features of one row, so a store instruction writes 16 rows x 32 B
        // (fp32) -- short runs that drain at about half the rate of whole rows (the q|k|v forward, then a form of this kernel, spent 8 of
        // its 20 us on its 15.9 MB of 32 B f16 runs).  The panel's output [16 MT rows][N] is assembled in the (now free) image buffers, rows padded by
        // 32 B against bank conflicts, and leaves as 16-byte units in row order: every wave instruction writes 1 KiB of one or two rows.
        static_assert(EPI == 0, "k_panel_gemm epilogue");
        constexpr int ESZ = 4, NCOL = PNL_WAVES * NTW * 16, ROWB = NCOL * ESZ + 32, UPR = NCOL * ESZ / 16;
        static_assert(16 * MT * ROWB <= PNL_LDS(MT), "panel output does not fit the image buffers");
        char* out = (char*)smem;
        __syncthreads();               // every wave has read its last fragments
#pragma unroll
        for (int t = 0; t < NTW; ++t) {
            const int n = 16 * (jt0 + t) + 4 * g;
            f32x4 bv = (f32x4){0.f, 0.f, 0.f, 0.f};
            if (bias) bv = *(const f32x4*)(bias + n);
#pragma unroll
            for (int i = 0; i < MT; ++i) {
                *(f32x4*)(out + (16 * i + l15) * ROWB + n * ESZ) = acc[t][i] + bv;
            }
        }
        __syncthreads();
        char* dst = (char*)C;
        for (int u = tid; u < 16 * MT * UPR; u += PNL_THREADS) {
            const int r = u / UPR, c = u % UPR;
            if (m0 + r < M) *(f32x4*)(dst + ((long)(m0 + r) * ldc) * ESZ + 16 * c) = *(const f32x4*)(out + r * ROWB + 16 * c);
        }
    }
}

// ---- the q|k|v forward as column thirds: qkv16[M][768] (f16) = f16((x W^T + b) [q third * 32^-0.5]), K = 256 -----------------------------
// As k_panel_gemm<MT, 6, .., EPI 3> this Linear was one workgroup per CU (256 VGPRs with spills, 112 KB of LDS): every CU staged its
// panel, multiplied and drained its stores at the same time, and the three phases added up (20 us, 8 of them the store drain).  Here a
// workgroup computes ONE third (q, k or v: 256 columns, two tiles per wave) of a panel from one {hi, lo} image pair (K = 256 is a single
// chunk) in <= 128 VGPRs and 32 / 48 KB of LDS, so that two workgroups share a CU (and leave room beside the side stream's kernels): one's
// stores drain under the other's product.  Per output element the arithmetic is that of the former kernel: same fragments, same pass
// order, k-steps 0..7 into one accumulator, same epilogue expression -- the same bits.
// grid = 24 * ceil(panels / 8): workgroups are dealt round-robin over the 8 XCDs by linear id, so id = 8 (3 j + t) + x is panel 8 j + x,
// third t -- the three readers of a panel share an L2.  x in split-4 storage; x_t (or NULL): T-frag copy of x, written by third 0.
// Ring depth 2 (one k-step ahead): the co-resident workgroups cover the latency, and depth 4 pushes MT = 3 past 128 VGPRs
// (profiles/qkv_fwd_thirds_ab.txt has the shapes that were measured)
#define QKV3_LDS(MT) (2 * PNL_IMG(MT) * 2)
template <int MT>
__global__ void __launch_bounds__(PNL_THREADS, 4) k_panel_qkv3(const float* __restrict__ xs, int M, const f32x4* __restrict__ Wf,
                                                               const float* __restrict__ bias, h16* __restrict__ qkv16, f32x4* __restrict__ x_t) {
    constexpr int NTW = 2, D = 2, KS = CFFM_C / 32;
    static_assert(CFFM_C == PNL_KC && PNL_WAVES * NTW * 16 == CFFM_C, "one chunk, 256 columns per third");
    CFFM_DYN_SMEM(smem);
    bf16* img = (bf16*)smem;     // [hi | lo][16 MT][256]
    const int tid = threadIdx.x, lane = tid & 63, wave = wave_uniform(tid >> 6), l15 = lane & 15, g = lane >> 4;
    const int q = blockIdx.x >> 3, t = q % 3, pan = 8 * (q / 3) + (blockIdx.x & 7);
    if (pan >= (M + 16 * MT - 1) / (16 * MT)) return;      // the last group of 8 panels may be short
    const int m0 = pan * 16 * MT;
    const buf_t rsa = buf_make(xs, (uint32_t)((long)M * CFFM_C * 4));
    PnlStream st;
    st.rs = buf_make(Wf, (uint32_t)(3 * CFFM_C * CFFM_C * 4));
    st.voff = lane * 16;
    st.KS = KS;
    const int jt0 = 16 * t + wave * NTW;
    f32x4 acc[NTW][MT];
#pragma unroll
    for (int j = 0; j < NTW; ++j)
#pragma unroll
        for (int i = 0; i < MT; ++i) acc[j][i] = (f32x4){0.f, 0.f, 0.f, 0.f};
    PnlRing<2, D> ring;
    pnl_ring_load<2, D>(ring, 0, st, jt0, 0);
    pnl_pin_vmem();
    {
        PnlStage<MT> sr;
        pnl_stage_load<MT>(sr, rsa, CFFM_C, m0, 0, tid);
        pnl_stage_store<MT, true>(sr, img, img + PNL_IMG(MT), tid);
    }
    pnl_lds_barrier();
    pnl_chunk_mma<MT, NTW, 2, D, PnlNoExtra, true>(acc, ring, img, img + PNL_IMG(MT), st, jt0, 0, l15, g, st, jt0, 0);
    // (behind the product, as in k_panel_gemm: in front of it the stores hold up the B-fragment loads)
    if (x_t && t == 0) pnl_tfrag_store<MT>(img, img + PNL_IMG(MT), x_t, m0, 0, CFFM_C / 16, M, ((long)M + 31) / 32 * 32, wave, lane);
    // epilogue through LDS (see k_panel_gemm): the third's [16 MT rows][256] f16 leave as whole 512-byte row segments
    constexpr int ROWB = CFFM_C * 2 + 32, UPR = CFFM_C * 2 / 16;
    static_assert(16 * MT * ROWB <= QKV3_LDS(MT), "panel output does not fit the image");
    char* out = (char*)smem;
    pnl_lds_barrier();                 // every wave has read its last fragments
    const float sc = t == 0 ? 0.17677669529663687f : 1.f;
#pragma unroll
    for (int j = 0; j < NTW; ++j) {
        const int nl = 16 * (wave * NTW + j) + 4 * g;
        const f32x4 bv = *(const f32x4*)(bias + CFFM_C * t + nl);
#pragma unroll
        for (int i = 0; i < MT; ++i) {
            typedef h16 h16x4 __attribute__((ext_vector_type(4)));
            h16x4 o;
            for (int e = 0; e < 4; ++e) o[e] = (h16)((acc[j][i][e] + bv[e]) * sc);
            *(h16x4*)(out + (16 * i + l15) * ROWB + nl * 2) = o;
        }
    }
    pnl_lds_barrier();
    char* dst = (char*)qkv16 + CFFM_C * 2 * t;
    for (int u = tid; u < 16 * MT * UPR; u += PNL_THREADS) {
        const int r = u / UPR, c = u % UPR;
        if (m0 + r < M) *(f32x4*)(dst + (long)(m0 + r) * (3 * CFFM_C * 2) + 16 * c) = *(const f32x4*)(out + r * ROWB + 16 * c);
    }
}

// =====================================================================================================================
// Fused row-panel kernels of the block (round 3): everything between the attention output and the block output in ONE
// launch per direction.  A workgroup owns 16 MT token rows; intermediates (x1, LN2(x1), the hidden activations) live in LDS
// / registers as the next GEMM's panel image, the three weights stream through the B ring back to back.
//   forward  (cffm_transformer.py:602 proj, :823 residual, :824 norm2 + Mlp :10-26 + residual):
//       x1 = xt + ao Wp^T + bp;  z2 = LN2(x1);  hraw = z2 W1^T;  act = gelu(hraw + b1);  x2 = x1 + act W2^T + b2
//   backward (the input-gradient chain of the same lines):
//       dh = (dout W2) * gelu'(hraw + b1);  dz2 = dh W1;  dx1 = dout + LN2'(dz2);  dao = dx1 Wp
// replacing (forward) k_gemm_split<proj> + k_residual_ln + k_gemm_split<fc1+GELU> + k_gemm_split<fc2+residual> and (backward)
// k_gemm_split<fc2 dX + GELU'> + k_gemm_split<fc1 dX> + k_ln_bwd_residual + k_gemm_split<proj dX>; the weight gradients keep
// reading z2 / act / dh (split-4 storage) and x1 / dx1 / ao from memory as before.
__device__ __forceinline__ f32x4 pnl_pack_hl(bf16x4 h, bf16x4 l) {
    const f32x2_t a = __builtin_bit_cast(f32x2_t, h), b = __builtin_bit_cast(f32x2_t, l);
    return (f32x4){a[0], a[1], b[0], b[1]};
}
// 4 consecutive features n .. n+3 of panel row `row` -> the hi / lo images (8-byte stores)
__device__ __forceinline__ void pnl_img_put(bf16* __restrict__ hi, bf16* __restrict__ lo, int row, int n, bf16x4 h, bf16x4 l) {
    const int o = pnl_off(row, n >> 3) + (n & 4);
    *(bf16x4*)(hi + o) = h;
    *(bf16x4*)(lo + o) = l;
}
// sum over the four lane groups g (lanes l15, l15 + 16, l15 + 32, l15 + 48): result in every lane
__device__ __forceinline__ float pnl_sum_g(float v) {
    v += __shfl_xor(v, 16, 64);
    v += __shfl_xor(v, 32, 64);
    return v;
}
#define PNL_STORE4(p, v) (*(f32x4*)(p) = (v))
#define PNL_FUSED_LDS(MT) (6 * PNL_IMG(MT) * 2 + 2 * PNL_WAVES * 16 * (MT) * 4)   // P + 2 x ACT (hi | lo each) + reduction scratch

struct MlpFwdArgs {
    const float* ao;                    // [NP][256] attention output
    const float* xt; long xt_bs; int rows_per_batch;   // residual input: row m = xt + (m / rpb) * xt_bs + (m % rpb) * 256
    const f32x4 *wp, *w1, *w2;          // fragment-ordered weights, NT form (pnl_pack_weight)
    const float *bp, *b1, *b2, *g2, *be2;
    float *x1, *z2s /* split-4, or NULL */, *mean2, *rstd2, *hraw, *acts /* split-4, or NULL: not stored (the fc2 weight gradient re-applies bias + GELU to hraw) */, *x2;
    f32x4 *ao_t, *z2_t, *act_t;         // T-frag copies of ao [NP][256], z2 [NP][256], act [NP][1024] for the streaming weight gradients (each may be NULL)
    int NP;
    // NCHW instantiations only (x2 is not read there): row m is pixel m % rows_per_batch of image m / rows_per_batch, and its feature n
    // goes to x2_nchw[(m / rows_per_batch) * x2_bs + n * rows_per_batch + m % rows_per_batch]
    float* x2_nchw; long x2_bs;
};

// The finished x2 tile of the NCHW instantiations, [256 channels][16 MT pixels] fp32 in LDS: the pitch keeps a channel's pixels 16-byte
// aligned, and the four channel groups g of a wave's scalar writes (4 g channels apart: 4 g PITCH = 16 g mod 64 words) in four bank groups
#define PNL_NCHW_PITCH(MT) (16 * (MT) + 4)

// INFER = true: the forward of a call that keeps nothing for a backward (the inference forward of the layer) -- of everything below
// only x2 is stored (x1, the LayerNorm statistics, hraw and the split-4 / T-frag operand copies of the weight gradients are not, and
// their pointers are not read).  Selected at compile time: the training instantiation is the kernel it was, and the arithmetic of the
// two is the same, instruction for instruction.
// NCHW = true: the layer's last block -- x2 leaves as the target frame of the layer's NCHW output (a.x2_nchw) instead of as token rows,
// which nothing but a layout pass would read.  The tile (one 64- or 128-byte run of pixels per channel) goes through LDS so that a lane
// stores four consecutive pixels of one channel; the values are those of the rows form.  Also selected at compile time.
template <int MT, int D, bool INFER = false, bool NCHW = false>
__global__ void __launch_bounds__(PNL_THREADS) k_mlp_fwd(MlpFwdArgs a) {
    CFFM_DYN_SMEM(smem);
    bf16* P = (bf16*)smem;                         // ao panel, later the z2 panel
    bf16* ACT = P + 2 * PNL_IMG(MT);               // two hidden-chunk images
    float* red = (float*)(ACT + 4 * PNL_IMG(MT));  // [2][8 waves][16 MT]
    const int tid = threadIdx.x, lane = tid & 63, wave = wave_uniform(tid >> 6), l15 = lane & 15, g = lane >> 4;
    const int m0 = blockIdx.x * 16 * MT, NP = a.NP;
    PnlStream sp, s1, s2;
    sp.rs = buf_make(a.wp, 256u * 256 * 4); sp.voff = lane * 16; sp.KS = 8;
    s1.rs = buf_make(a.w1, 1024u * 256 * 4); s1.voff = lane * 16; s1.KS = 8;
    s2.rs = buf_make(a.w2, 1024u * 256 * 4); s2.voff = lane * 16; s2.KS = 32;
    PnlRing<2, D> ring;
#pragma unroll
    for (int s = 0; s < D - 1; ++s) pnl_ring_load<2, D>(ring, s, sp, 2 * wave, s);
    uint32_t touch = 0;
    pnl_pin_vmem();
    const f32x4 z4 = (f32x4){0.f, 0.f, 0.f, 0.f};
    bool valid[MT];
    long mrow[MT];
#pragma unroll
    for (int i = 0; i < MT; ++i) {
        const long m = m0 + 16 * i + l15;
        valid[i] = m < NP;
        mrow[i] = m;
    }
    f32x4 xtv[2][MT], bpv[2];
    {
        PnlStage<MT> sr;
        pnl_stage_load<MT>(sr, buf_make(a.ao, (uint32_t)((long)NP * 256 * 4)), 256, m0, 0, tid);
        // the residual rows and the proj bias ride behind the panel's loads (staging does not wait for them) and are consumed behind the
        // proj product: requested there, they would be one exposed HBM round trip with the ring empty (operand prefetch rule, k_mlp_bwd)
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            const int n = 32 * wave + 16 * t + 4 * g;
            bpv[t] = *(const f32x4*)(a.bp + n);
#pragma unroll
            for (int i = 0; i < MT; ++i) {
                xtv[t][i] = z4;
                if (valid[i]) {
                    const long b = mrow[i] / a.rows_per_batch, rr = mrow[i] % a.rows_per_batch;
                    xtv[t][i] = *(const f32x4*)(a.xt + b * a.xt_bs + rr * 256 + n);
                }
            }
        }
        // L2 warm-up (pnl_l2_touch), behind the panel's loads in the memory queue: staging does not wait for it
        pnl_pin_vmem();
        const uint32_t t0 = pnl_l2_touch(a.w1, 1024L * 256 * 4, tid), t1 = pnl_l2_touch(a.w2, 1024L * 256 * 4, tid);
        pnl_pin_vmem();
        pnl_stage_store<MT, false>(sr, P, P + PNL_IMG(MT), tid);
        touch = t0 ^ t1;
    }
    pnl_lds_barrier();
    const long NP32 = ((long)NP + 31) / 32 * 32;
    if (!INFER && a.ao_t) pnl_tfrag_store<MT>(P, P + PNL_IMG(MT), a.ao_t, m0, 0, 16, NP, NP32, wave, lane);
    f32x4 acc[2][MT];
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int i = 0; i < MT; ++i) acc[t][i] = z4;
    pnl_chunk_mma<MT, 2, 2, D>(acc, ring, P, P + PNL_IMG(MT), sp, 2 * wave, 0, l15, g, s1, 2 * wave, 0);
    // ---- x1 = xt + proj + bp, LayerNorm statistics over the 256 features of a row (8 waves x 32 features)
    f32x4 x1v[2][MT];
    float s[MT];
#pragma unroll
    for (int i = 0; i < MT; ++i) s[i] = 0.f;
    // LayerNorm weights: requested here, used behind the two reductions below
    f32x4 gmv[2], bev[2];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        const int n = 32 * wave + 16 * t + 4 * g;
        gmv[t] = *(const f32x4*)(a.g2 + n);
        bev[t] = *(const f32x4*)(a.be2 + n);
    }
    pnl_pin_vmem();
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        const int n = 32 * wave + 16 * t + 4 * g;
#pragma unroll
        for (int i = 0; i < MT; ++i) {
            const f32x4 v = acc[t][i] + bpv[t] + xtv[t][i];
            x1v[t][i] = v;
            if (!INFER && valid[i]) *(f32x4*)(a.x1 + mrow[i] * 256 + n) = v;
            s[i] += (v[0] + v[1]) + (v[2] + v[3]);
        }
    }
#pragma unroll
    for (int i = 0; i < MT; ++i) {
        s[i] = pnl_sum_g(s[i]);
        if (g == 0) red[wave * 16 * MT + 16 * i + l15] = s[i];
    }
    pnl_lds_barrier();
    float mu[MT], rs[MT];
#pragma unroll
    for (int i = 0; i < MT; ++i) {
        float tot = 0.f;
#pragma unroll
        for (int w = 0; w < PNL_WAVES; ++w) tot += red[w * 16 * MT + 16 * i + l15];
        mu[i] = tot * (1.f / 256);
        float q = 0.f;
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            const f32x4 d = x1v[t][i] - mu[i];
            q += (d[0] * d[0] + d[1] * d[1]) + (d[2] * d[2] + d[3] * d[3]);
        }
        q = pnl_sum_g(q);
        if (g == 0) red[(PNL_WAVES + wave) * 16 * MT + 16 * i + l15] = q;
    }
    pnl_lds_barrier();
#pragma unroll
    for (int i = 0; i < MT; ++i) {
        float tot = 0.f;
#pragma unroll
        for (int w = 0; w < PNL_WAVES; ++w) tot += red[(PNL_WAVES + w) * 16 * MT + 16 * i + l15];
        rs[i] = 1.f / sqrtf(tot * (1.f / 256) + CFFM_LN_EPS);
        if (!INFER && wave == 0 && g == 0 && valid[i]) { a.mean2[mrow[i]] = mu[i]; a.rstd2[mrow[i]] = rs[i]; }
    }
    // z2 -> the panel image (the ao image is dead: every wave finished its proj product before the first barrier above)
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        const int n = 32 * wave + 16 * t + 4 * g;
        const f32x4 gm = gmv[t], be = bev[t];
#pragma unroll
        for (int i = 0; i < MT; ++i) {
            const f32x4 zv = (x1v[t][i] - mu[i]) * rs[i] * gm + be;
            bf16x4 h, l;
            split4(zv, h, l);
            pnl_img_put(P, P + PNL_IMG(MT), 16 * i + l15, n, h, l);
            if (!INFER && valid[i] && a.z2s) *(f32x4*)(a.z2s + mrow[i] * 256 + n) = pnl_pack_hl(h, l);
        }
    }
    pnl_lds_barrier();
    if (!INFER && a.z2_t) pnl_tfrag_store<MT>(P, P + PNL_IMG(MT), a.z2_t, m0, 0, 16, NP, NP32, wave, lane);
    // ---- Mlp: hidden chunks of 256 features: fc1 chunk -> GELU -> chunk image -> fc2 accumulates over the chunk
    f32x4 acc2[2][MT];
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int i = 0; i < MT; ++i) acc2[t][i] = z4;
    // the fc2 bias of the last lines: requested ahead of the hidden chunks
    f32x4 b2v[2];
#pragma unroll
    for (int t = 0; t < 2; ++t) b2v[t] = *(const f32x4*)(a.b2 + 32 * wave + 16 * t + 4 * g);
    for (int c = 0; c < 4; ++c) {
        f32x4 h1[2][MT];
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int i = 0; i < MT; ++i) h1[t][i] = z4;
        // the chunk's fc1 bias: requested in front of the product whose epilogue adds it
        f32x4 b1v[2];
#pragma unroll
        for (int t = 0; t < 2; ++t) b1v[t] = *(const f32x4*)(a.b1 + 256 * c + 32 * wave + 16 * t + 4 * g);
        pnl_pin_vmem();
        pnl_chunk_mma<MT, 2, 2, D>(h1, ring, P, P + PNL_IMG(MT), s1, 16 * c + 2 * wave, 0, l15, g, s2, 2 * wave, 8 * c);
        bf16* Ah = ACT + (c & 1) * 2 * PNL_IMG(MT);
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            const int nl = 32 * wave + 16 * t + 4 * g, n = 256 * c + nl;
            const f32x4 bv = b1v[t];
#pragma unroll
            for (int i = 0; i < MT; ++i) {
                const f32x4 raw = h1[t][i];
                f32x4 av;
                for (int e = 0; e < 4; ++e) av[e] = gelu_erf(raw[e] + bv[e]);
                bf16x4 h, l;
                split4(av, h, l);
                pnl_img_put(Ah, Ah + PNL_IMG(MT), 16 * i + l15, nl, h, l);
                if (!INFER && valid[i]) {
                    *(f32x4*)(a.hraw + mrow[i] * 1024 + n) = raw;
                    if (a.acts) *(f32x4*)(a.acts + mrow[i] * 1024 + n) = pnl_pack_hl(h, l);
                }
            }
        }
        pnl_lds_barrier();
        if (!INFER && a.act_t) pnl_tfrag_store<MT>(Ah, Ah + PNL_IMG(MT), a.act_t, m0, 16 * c, 64, NP, NP32, wave, lane);
        const int cn = c < 3 ? c + 1 : 0;
        pnl_chunk_mma<MT, 2, 2, D>(acc2, ring, Ah, Ah + PNL_IMG(MT), s2, 2 * wave, 8 * c, l15, g, s1, 16 * cn + 2 * wave, 0);
    }
    if constexpr (!NCHW) {
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            const int n = 32 * wave + 16 * t + 4 * g;
            const f32x4 bv = b2v[t];
#pragma unroll
            for (int i = 0; i < MT; ++i)
                if (valid[i]) *(f32x4*)(a.x2 + mrow[i] * 256 + n) = x1v[t][i] + acc2[t][i] + bv;
        }
    } else {
        // The tile is assembled over the z2 image and the FIRST pair of hidden-chunk images: every wave read them for the last time in
        // front of chunk 3's barrier (chunk 3's fc1 product, chunk 2's fc2 product); the last product, which slower waves may still be
        // in, reads the second pair only -- so no barrier is needed in front of these writes
        constexpr int PITCH = PNL_NCHW_PITCH(MT), QPC = 4 * MT;      // quads of pixels per channel
        static_assert(256 * PITCH * 4 <= 4 * PNL_IMG(MT) * 2, "the x2 tile does not fit the z2 image + one pair of hidden-chunk images");
        float* tile = (float*)smem;
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            const int n = 32 * wave + 16 * t + 4 * g;
            const f32x4 bv = b2v[t];
#pragma unroll
            for (int i = 0; i < MT; ++i) {
                const f32x4 v = x1v[t][i] + acc2[t][i] + bv;
#pragma unroll
                for (int e = 0; e < 4; ++e) tile[(n + e) * PITCH + 16 * i + l15] = v[e];
            }
        }
        pnl_lds_barrier();
        // a lane stores four consecutive pixels of one channel (a wave instruction: whole 16 MT-pixel runs of 32 / MT channels); a quad
        // that crosses into the next image, runs past NP or is not 16-byte aligned (pixels per image not a multiple of 4) goes out pixel by pixel
        const int HW = a.rows_per_batch;
#pragma unroll
        for (int it = 0; it < 256 * QPC / PNL_THREADS; ++it) {
            const int u = tid + PNL_THREADS * it, ch = u / QPC, q = u % QPC, m = m0 + 4 * q;
            if (m >= NP) continue;
            const f32x4 v = *(const f32x4*)(tile + ch * PITCH + 4 * q);
            int b = m / HW, pix = m % HW;
            float* dst = a.x2_nchw + (long)b * a.x2_bs + (long)ch * HW + pix;
            if (m + 3 < NP && pix + 3 < HW && ((uintptr_t)dst & 15) == 0) {
                *(f32x4*)dst = v;
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    if (m + e < NP) a.x2_nchw[(long)b * a.x2_bs + (long)ch * HW + pix] = v[e];
                    if (++pix == HW) { pix = 0; ++b; }
                }
            }
        }
    }
    if (a.NP < 0) (INFER ? (NCHW ? a.x2_nchw : a.x2) : a.mean2)[tid] = (float)touch;     // (never taken: keeps the warm-up loads)
}

struct MlpBwdArgs {
    const float* dout;                  // [NP][256] gradient of the block's output rows
    const float* hraw; const float* b1; // saved fc1 product, fc1 bias
    const float *x1, *mean2, *rstd2, *g2;
    const f32x4 *w2n, *w1n, *wpn;       // fragment-ordered weights, NN form
    float* dhs;                         // [NP][1024] split-4: gradient of hraw (or NULL)
    f32x4 *dout_t, *dh_t, *dx1_t;       // T-frag copies of dout [NP][256], dh [NP][1024], dx1 [NP][256] for the streaming weight gradients (each may be NULL)
    float* dx1;                         // [NP][256]
    float* dao;                         // [NP][256]
    float* rec_b1;                      // [workgroups][1024] column sums of dh (fc1 bias gradient records)
    float* rec_ln;                      // [workgroups][1024] dgamma2 | dbeta2 | colsum(dout) | colsum(dx1) records
    int NP;
    // NCHW instantiation only (dout is not read there): the gradient arrives as NCHW images of `pix` pixels, dy_bs floats apart -- row m is
    // pixel m % pix of image m / pix, its feature n is dy_nchw[(m / pix) * dy_bs + n * pix + m % pix] -- and the kernel writes the rows
    // [NP][256] to dout_rows itself (the fc2 weight gradient reads them)
    const float* dy_nchw; long dy_bs; int pix; float* dout_rows;
};
#define PNL_FUSED_LDS_NCHW(MT) (PNL_FUSED_LDS(MT) + 256 * PNL_NCHW_PITCH(MT) * 4)   // + the fp32 dout tile, which lives to the LayerNorm backward

// NCHW = true: the layer's last block -- the upstream gradient is read as the target frame of the layer's NCHW gradient (a.dy_nchw), which
// nothing but a layout pass would turn into rows first.  The panel arrives as 16-byte units of four consecutive pixels of a channel and
// is turned in LDS (fp32 tile [256 channels][16 MT pixels], as in k_mlp_fwd's NCHW form); from there every wave takes its rows in
// accumulator layout: for the panel image, for the rows it writes to a.dout_rows, and again for the LayerNorm backward.  Same values, same
// order of every sum as the rows form.  Selected at compile time: the rows instantiation is the kernel it was.
template <int MT, int D, bool NCHW = false>
__global__ void __launch_bounds__(PNL_THREADS) k_mlp_bwd(MlpBwdArgs a) {
    CFFM_DYN_SMEM(smem);
    bf16* P = (bf16*)smem;                         // dout panel, later the dx1 panel
    bf16* DH = P + 2 * PNL_IMG(MT);                // two hidden-chunk images of dh
    float* red = (float*)(DH + 4 * PNL_IMG(MT));   // [2][8 waves][16 MT]
    float* T = red + 2 * PNL_WAVES * 16 * MT;      // (NCHW) fp32 dout tile [256][PNL_NCHW_PITCH]
    constexpr int TP = PNL_NCHW_PITCH(MT);
    const int tid = threadIdx.x, lane = tid & 63, wave = wave_uniform(tid >> 6), l15 = lane & 15, g = lane >> 4;
    const int m0 = blockIdx.x * 16 * MT, NP = a.NP;
    PnlStream s2, s1, sp;
    s2.rs = buf_make(a.w2n, 1024u * 256 * 4); s2.voff = lane * 16; s2.KS = 8;    // out 1024 hidden, contraction 256
    s1.rs = buf_make(a.w1n, 1024u * 256 * 4); s1.voff = lane * 16; s1.KS = 32;   // out 256, contraction 1024
    sp.rs = buf_make(a.wpn, 256u * 256 * 4); sp.voff = lane * 16; sp.KS = 8;
    PnlRing<2, D> ring;
#pragma unroll
    for (int s = 0; s < D - 1; ++s) pnl_ring_load<2, D>(ring, s, s2, 2 * wave, s);
    uint32_t touch = 0;
    pnl_pin_vmem();
    const f32x4 z4 = (f32x4){0.f, 0.f, 0.f, 0.f};
    bool valid[MT];
    long mrow[MT];
#pragma unroll
    for (int i = 0; i < MT; ++i) {
        const long m = m0 + 16 * i + l15;
        valid[i] = m < NP;
        mrow[i] = m;
    }
    // (NCHW) rows 16 i + l15, features n .. n + 3 of the dout tile: accumulator layout (conflict-free: see PNL_NCHW_PITCH)
    const auto tile_get = [&](int n, int i) {
        f32x4 v;
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = T[(n + e) * TP + 16 * i + l15];
        return v;
    };
    // Operand prefetch.  The CU's vector-memory path is one in-order queue and vmcnt counts a wave's loads in issue order (see
    // pnl_chunk_mma), so a B-ring slot is consumed only after every load issued before it has returned: an HBM read (2-3 us under
    // this load) requested in front of a product, or between two, stalls the weight stream (D - 1 k-steps, about 1 us of lead) until
    // it is back.  Rule: an HBM operand is requested at the START of a phase that does not consume the ring -- panel staging, the
    // VALU / LDS epilogue between two products -- so that the phase plus the D - 1 prefetched k-steps cover it:
    //   hr[c & 1]  the saved fc1 product of chunk c: chunk 0 with the dout panel, chunk c + 1 at the start of chunk c's epilogue;
    //   the LayerNorm operands (x1 in the hr buffer that has no next chunk, dout, mean2, rstd2, g2): at the start of the LAST
    //   chunk's epilogue, consumed behind the last dz product.
    // The chunk loop is unrolled so that buffer indices and "last chunk" are compile-time.
    f32x4 hr[2][2][MT];
    const auto hr_request = [&](int c) {
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int i = 0; i < MT; ++i)
                hr[c & 1][t][i] = valid[i] ? *(const f32x4*)(a.hraw + mrow[i] * 1024 + 256 * c + 32 * wave + 16 * t + 4 * g) : z4;
    };
    if constexpr (!NCHW) {
        const buf_t rs_dout = buf_make(a.dout, (uint32_t)((long)NP * 256 * 4));
        PnlStage<MT> sr;
        pnl_stage_load<MT>(sr, rs_dout, 256, m0, 0, tid);
        hr_request(0);
        // L2 warm-up (pnl_l2_touch), behind the panel's loads in the memory queue
        pnl_pin_vmem();
        const uint32_t t0 = pnl_l2_touch(a.w2n, 1024L * 256 * 4, tid), t1 = pnl_l2_touch(a.w1n, 1024L * 256 * 4, tid), t2 = pnl_l2_touch(a.wpn, 256L * 256 * 4, tid);
        pnl_pin_vmem();
        pnl_stage_store<MT, false>(sr, P, P + PNL_IMG(MT), tid);
        touch = t0 ^ t1 ^ t2;
    } else {
        // a thread loads the same four pixels (quad q of the panel) of 2 MT channels; pixels at and past NP read as zeros (as the rows
        // form's rows past NP do); a quad that crosses into the next image or is not 16-byte aligned is read pixel by pixel
        constexpr int QPC = 4 * MT;
        const int HW = a.pix, q = tid % QPC, m = m0 + 4 * q;
        const int b0 = m < NP ? m / HW : 0, pix0 = m < NP ? m % HW : 0;
        const bool whole = m + 3 < NP && pix0 + 3 < HW;
        f32x4 qv[2 * MT];
#pragma unroll
        for (int it = 0; it < 2 * MT; ++it) {
            const int ch = tid / QPC + (PNL_THREADS / QPC) * it;
            const float* src = a.dy_nchw + (long)b0 * a.dy_bs + (long)ch * HW + pix0;
            if (whole && ((uintptr_t)src & 15) == 0) {
                qv[it] = *(const f32x4*)src;
            } else {
                qv[it] = z4;
                int b = b0, pix = pix0;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    if (m + e < NP) qv[it][e] = a.dy_nchw[(long)b * a.dy_bs + (long)ch * HW + pix];
                    if (++pix == HW) { pix = 0; ++b; }
                }
            }
        }
        hr_request(0);
        // L2 warm-up (pnl_l2_touch), behind the panel's loads in the memory queue
        pnl_pin_vmem();
        const uint32_t t0 = pnl_l2_touch(a.w2n, 1024L * 256 * 4, tid), t1 = pnl_l2_touch(a.w1n, 1024L * 256 * 4, tid), t2 = pnl_l2_touch(a.wpn, 256L * 256 * 4, tid);
        pnl_pin_vmem();
#pragma unroll
        for (int it = 0; it < 2 * MT; ++it) *(f32x4*)(T + (tid / QPC + (PNL_THREADS / QPC) * it) * TP + 4 * q) = qv[it];
        touch = t0 ^ t1 ^ t2;
        pnl_lds_barrier();
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int i = 0; i < MT; ++i) {
                const int n = 32 * wave + 16 * t + 4 * g;
                bf16x4 h, l;
                split4(tile_get(n, i), h, l);
                pnl_img_put(P, P + PNL_IMG(MT), 16 * i + l15, n, h, l);
            }
    }
    pnl_lds_barrier();
    // (NCHW) the dout rows leave beside the first product, one 16-byte store per thread and step (a burst in front of it would hold up the
    // B-fragment loads queued behind it, see pnl_chunk_mma)
    const auto rows_put = [&](int sc) {
        if (sc < 2 * MT) {
            const int t = sc / MT, i = sc % MT, n = 32 * wave + 16 * t + 4 * g;
            const f32x4 v = tile_get(n, i);
            if (valid[i]) *(f32x4*)(a.dout_rows + mrow[i] * 256 + n) = v;
        }
    };
    const long NP32 = ((long)NP + 31) / 32 * 32;
    if (a.dout_t) pnl_tfrag_store<MT>(P, P + PNL_IMG(MT), a.dout_t, m0, 0, 16, NP, NP32, wave, lane);
    f32x4 dz[2][MT];
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int i = 0; i < MT; ++i) dz[t][i] = z4;
    f32x4 dr[2][MT], gmv[2];
    float mu[MT], rs[MT];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        f32x4 da[2][MT];
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int i = 0; i < MT; ++i) da[t][i] = z4;
        // the chunk's fc1 bias (an L2 hit) goes in front of the product whose epilogue adds it
        f32x4 b1v[2];
#pragma unroll
        for (int t = 0; t < 2; ++t) b1v[t] = *(const f32x4*)(a.b1 + 256 * c + 32 * wave + 16 * t + 4 * g);
        pnl_pin_vmem();
        if (NCHW && c == 0)
            pnl_chunk_mma<MT, 2, 2, D, decltype(rows_put)>(da, ring, P, P + PNL_IMG(MT), s2, 16 * c + 2 * wave, 0, l15, g, s1, 2 * wave, 8 * c, rows_put);
        else
            pnl_chunk_mma<MT, 2, 2, D>(da, ring, P, P + PNL_IMG(MT), s2, 16 * c + 2 * wave, 0, l15, g, s1, 2 * wave, 8 * c);
        const bool more = c < 3;
        if (more) {
            hr_request(c + 1);
        } else {
#pragma unroll
            for (int i = 0; i < MT; ++i) {
                mu[i] = valid[i] ? a.mean2[mrow[i]] : 0.f;
                rs[i] = valid[i] ? a.rstd2[mrow[i]] : 0.f;
            }
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                const int n = 32 * wave + 16 * t + 4 * g;
                gmv[t] = *(const f32x4*)(a.g2 + n);
#pragma unroll
                for (int i = 0; i < MT; ++i) {
                    hr[(c + 1) & 1][t][i] = dr[t][i] = z4;
                    if (valid[i]) {
                        hr[(c + 1) & 1][t][i] = *(const f32x4*)(a.x1 + mrow[i] * 256 + n);
                        if (!NCHW) dr[t][i] = *(const f32x4*)(a.dout + mrow[i] * 256 + n);
                    }
                    if (NCHW) dr[t][i] = tile_get(n, i);     // (pixels past NP are zeros in the tile)
                }
            }
        }
        pnl_pin_vmem();
        bf16* Ah = DH + (c & 1) * 2 * PNL_IMG(MT);
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            const int nl = 32 * wave + 16 * t + 4 * g, n = 256 * c + nl;
            const f32x4 bv = b1v[t];
            f32x4 cs = z4;
#pragma unroll
            for (int i = 0; i < MT; ++i) {
                f32x4 dh = z4;
                if (valid[i]) {
                    const f32x4 hv = hr[c & 1][t][i] + bv;
                    for (int e = 0; e < 4; ++e) dh[e] = da[t][i][e] * gelu_erf_grad(hv[e]);
                }
                bf16x4 h, l;
                split4(dh, h, l);
                pnl_img_put(Ah, Ah + PNL_IMG(MT), 16 * i + l15, nl, h, l);
                if (valid[i] && a.dhs) *(f32x4*)(a.dhs + mrow[i] * 1024 + n) = pnl_pack_hl(h, l);
                cs += dh;
            }
            for (int e = 0; e < 4; ++e) cs[e] = row16_sum(cs[e]);
            if (l15 == 0) *(f32x4*)(a.rec_b1 + (long)blockIdx.x * 1024 + n) = cs;
        }
        pnl_lds_barrier();
        if (a.dh_t) pnl_tfrag_store<MT>(Ah, Ah + PNL_IMG(MT), a.dh_t, m0, 16 * c, 64, NP, NP32, wave, lane);
        pnl_chunk_mma<MT, 2, 2, D>(dz, ring, Ah, Ah + PNL_IMG(MT), s1, 2 * wave, 8 * c, l15, g, more ? s2 : sp, more ? 16 * (c + 1) + 2 * wave : 2 * wave, 0);
    }
    // ---- LayerNorm backward + residual: dx1 = dout + rstd (gz - mean(gz) - xh mean(gz xh)), gz = dz2 * gamma
    f32x4 xh[2][MT], gz[2][MT];
    float m1[MT], m2[MT];
#pragma unroll
    for (int i = 0; i < MT; ++i) m1[i] = m2[i] = 0.f;
    f32x4 ag[2], ab[2], ar[2], ax[2];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        const int n = 32 * wave + 16 * t + 4 * g;
        const f32x4 gm = gmv[t];
        ag[t] = ab[t] = ar[t] = ax[t] = z4;
#pragma unroll
        for (int i = 0; i < MT; ++i) {
            const f32x4 xv = hr[0][t][i], dv = dr[t][i];      // (hr[0]: the x1 rows since the last chunk's epilogue)
            xh[t][i] = (xv - mu[i]) * rs[i];
            gz[t][i] = dz[t][i] * gm;
            ag[t] += dz[t][i] * xh[t][i];
            ab[t] += dz[t][i];
            ar[t] += dv;
            const f32x4 p = gz[t][i] * xh[t][i];
            m1[i] += (gz[t][i][0] + gz[t][i][1]) + (gz[t][i][2] + gz[t][i][3]);
            m2[i] += (p[0] + p[1]) + (p[2] + p[3]);
        }
    }
#pragma unroll
    for (int i = 0; i < MT; ++i) {
        m1[i] = pnl_sum_g(m1[i]);
        m2[i] = pnl_sum_g(m2[i]);
        if (g == 0) {
            red[wave * 16 * MT + 16 * i + l15] = m1[i];
            red[(PNL_WAVES + wave) * 16 * MT + 16 * i + l15] = m2[i];
        }
    }
    pnl_lds_barrier();
#pragma unroll
    for (int i = 0; i < MT; ++i) {
        float t1 = 0.f, t2 = 0.f;
#pragma unroll
        for (int w = 0; w < PNL_WAVES; ++w) {
            t1 += red[w * 16 * MT + 16 * i + l15];
            t2 += red[(PNL_WAVES + w) * 16 * MT + 16 * i + l15];
        }
        m1[i] = t1 * (1.f / 256);
        m2[i] = t2 * (1.f / 256);
    }
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        const int n = 32 * wave + 16 * t + 4 * g;
#pragma unroll
        for (int i = 0; i < MT; ++i) {
            const f32x4 dxv = (gz[t][i] - m1[i] - xh[t][i] * m2[i]) * rs[i] + dr[t][i];
            ax[t] += dxv;
            bf16x4 h, l;
            split4(dxv, h, l);
            pnl_img_put(P, P + PNL_IMG(MT), 16 * i + l15, n, h, l);     // (the dout image is dead since the last hidden chunk)
            if (valid[i]) *(f32x4*)(a.dx1 + mrow[i] * 256 + n) = dxv;
        }
        for (int e = 0; e < 4; ++e) {
            ag[t][e] = row16_sum(ag[t][e]);
            ab[t][e] = row16_sum(ab[t][e]);
            ar[t][e] = row16_sum(ar[t][e]);
            ax[t][e] = row16_sum(ax[t][e]);
        }
        if (l15 == 0) {
            float* rec = a.rec_ln + (long)blockIdx.x * 1024 + n;
            *(f32x4*)(rec) = ag[t];
            *(f32x4*)(rec + 256) = ab[t];
            *(f32x4*)(rec + 512) = ar[t];
            *(f32x4*)(rec + 768) = ax[t];
        }
    }
    pnl_lds_barrier();
    if (a.dx1_t) pnl_tfrag_store<MT>(P, P + PNL_IMG(MT), a.dx1_t, m0, 0, 16, NP, NP32, wave, lane);
    f32x4 dq[2][MT];
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int i = 0; i < MT; ++i) dq[t][i] = z4;
    pnl_chunk_mma<MT, 2, 2, D>(dq, ring, P, P + PNL_IMG(MT), sp, 2 * wave, 0, l15, g, sp, 2 * wave, 8);
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        const int n = 32 * wave + 16 * t + 4 * g;
#pragma unroll
        for (int i = 0; i < MT; ++i)
            if (valid[i]) *(f32x4*)(a.dao + mrow[i] * 256 + n) = dq[t][i];
    }
    if (a.NP < 0) a.dao[tid] = (float)touch;       // (never taken: keeps the warm-up loads)
}

