/* cffm_hip.h -- C ABI of libcffm_hip.so: the MI355X-native (gfx950) CFFM hot path.
 *
 * The reference (GuoleiSun/VSS-CFFM) is pure Python; it has no FFI for this path.  The entry points
 * below are what a binding of the reference's hot-path *modules* needs, one per module / stage, with
 * plain device pointers and sizes (no torch types):
 *
 *   cffm_layer_forward / _backward   <->  BasicLayer3d3.forward            cffm_transformer.py:917-927
 *   cffm_block_forward / _backward   <->  CffmTransformerBlock3d3.forward  cffm_transformer.py:709-832
 *   cffm_ln_pool_fwd                 <->  CFFA: norm1 + pad + pool_layers / pool_layers_clips
 *                                                                           cffm_transformer.py:716-805
 *   cffm_ln_pool_bwd                 <->  autograd through the same lines (the stage-level backward of the CFFA)
 *   cffm_bias_assemble / _scatter    <->  relative-position bias gathers (and their adjoint)  cffm_transformer.py:536-587
 *   cffm_attn_fwd / _bwd             <->  WindowAttention3d3.forward (CFM)  cffm_transformer.py:364-606
 *   cffm_linear_*                    <->  nn.Linear (qkv :374, proj :602, Mlp :10-26)
 *   cffm_panel_qkv_fwd / _bwd_input  <->  the q|k|v Linear (:374) on token rows, forward and input gradient
 *   cffm_mlp_fwd / _bwd              <->  proj + residual + norm2 + Mlp + residual  :602, :823-824
 *   cffm_gtc_*                       <->  BasicLayer_cluster / WindowAttention_cluster (CFFM++)
 *                                                         pvt/swin_transformer_2d.py:1103-1148, :208-262
 *   cffm_kmeans                      <->  KMeans(...).fit_predict of the prototype-generating head  cffm_head.py:280-282
 *   cffm_predict                     <->  EncoderDecoder_clips' resize, resize, softmax, flip, argmax
 *                                                         segmentors/encoder_decoder.py:367-378, :502-572
 *   cffm_dwconv_gelu_fwd / _bwd      <->  Mlp's DWConv + GELU of the MiT backbone  backbones/mix_transformer.py:48-55, 358-369
 *   cffm_sra_attn_fwd / _bwd         <->  the attention core of the MiT backbone's Attention.forward (q k^T, scale, softmax, attn v)
 *                                                         backbones/mix_transformer.py (Attention.forward)
 *   cffm_sr_ln_fwd / _bwd            <->  the `sr` Conv2d (kernel = stride = sr_ratio) + LayerNorm in front of kv, same forward
 *
 * Conventions: every pointer is a DEVICE pointer (fp32 unless stated) borrowed for the duration of
 * the call; `stream` is a hipStream_t (NULL = default stream); work is enqueued asynchronously on it;
 * functions return 0 on success, otherwise a negative code and cffm_last_error() describes it
 * (mirrors the reference's Python asserts: wrong T / shape is an error, not UB).  Single-threaded per
 * process (one process per GPU).  C = 256, 8 heads, window 7 are fixed as in cffm_head.py:74-95.
 */
#ifndef CFFM_HIP_H
#define CFFM_HIP_H
#ifdef __cplusplus
extern "C" {
#endif

#define CFFM_ABI_VERSION 13

typedef struct cffm_geom {
    int B, H0, W0;      /* clips, unpadded 1/8-scale grid                                   */
    int Hp, Wp, gy, gx; /* padded to multiples of 7; windows per side                        */
    int nW, HW, RC;     /* windows per clip; H0*W0; token rows per clip = 64*nW (49 + 15)    */
} cffm_geom;

/* parameters of one CffmTransformerBlock3d3 (state_dict names in SURVEY.md Appendix C) */
typedef struct cffm_block_params {
    const float *norm1_w, *norm1_b;
    const float *pool_w[4], *pool_b[4]; /* pool_layers.0, pool_layers_clips.{0,1,2}: [49],[49],[9],[4] / [1] */
    const float *rpb_own;               /* attn.relative_position_bias_table [169,8]                         */
    const float *rpb_ring;              /* attn.relative_position_bias_table_to_neighbors [1,8,49,132]      */
    const float *rpb_pool[4];           /* ..._to_windows.0 [8,121], ..._to_windows_clips.{0,1,2} [8,169|121|81] */
    const float *qkv_w, *qkv_b;         /* [768,256], [768] */
    const float *proj_w, *proj_b;       /* [256,256], [256] */
    const float *norm2_w, *norm2_b;
    const float *fc1_w, *fc1_b;         /* [1024,256], [1024] */
    const float *fc2_w, *fc2_b;         /* [256,1024], [256]  */
} cffm_block_params;

/* same fields, writable: gradients (every field is fully written by cffm_block_backward) */
typedef struct cffm_block_grads {
    float *norm1_w, *norm1_b;
    float *pool_w[4], *pool_b[4];
    float *rpb_own, *rpb_ring, *rpb_pool[4];
    float *qkv_w, *qkv_b, *proj_w, *proj_b, *norm2_w, *norm2_b, *fc1_w, *fc1_b, *fc2_w, *fc2_b;
} cffm_block_grads;

/* float offsets of the activations one block saves for its backward (inside its slice of `saved`) */
typedef struct cffm_block_ws {
    long mean1, rstd1, M, zall, qkv, bias, biasT, lse, ao, x1, mean2, rstd2, z2, hraw, act, x2, w_split, w_frag, ao_t, zall_t /* ABI 9 */, total;
} cffm_block_ws;

int cffm_abi_version(void);
const char* cffm_last_error(void);
int cffm_geom_init(cffm_geom* g, int B, int H0, int W0);
int cffm_block_ws_layout(const cffm_geom* g, cffm_block_ws* out);
long cffm_layer_saved_floats(const cffm_geom* g, int depth);  /* NHWC stack + depth * block_ws.total */
long cffm_layer_scratch_floats(const cffm_geom* g);

/* ---- optional per-stage HIP-event timing on the caller's stream (bench.py's live roofline numbers) ---- */
int cffm_profile_enable(long long stage_mask); /* bit i = stage i; 0 off; -1 all (perturbs: two event records per launch) */
int cffm_profile_sample_every(int period); /* time every period-th launch of an enabled stage only (1 = all; counted from the next cffm_profile_enable) */
int cffm_side_streams(int on); /* 0: parameter-gradient work stays on the caller's stream (per-kernel timing); returns the previous setting */
/* ABI 10: branches for the caller.  cffm_branch_begin(stream, i), i = 0..3: a library-owned stream ordered behind everything issued on `stream`
 * so far (or `stream` itself when side streams are off / unavailable); pass it as the `stream` argument of independent stage calls (the head's
 * per-scale embedding chains of cffm_head.py:102-119, weight vs input gradients of a classifier); cffm_branch_join(stream): `stream` continues
 * behind every branch.  Tensors a branch touches must outlive the join.  Stage calls that use library-owned scratch (cffm_linear_bwd_weight,
 * cffm_linear_bwd_weight_group, cffm_colsum) take it from a pool of the branch they are issued on, so they may run on different branches at
 * the same time; every other entry point with scratch of its own (the layer / block / gtc calls) belongs on the caller's stream. */
void* cffm_branch_begin(void* stream, int i);
int cffm_branch_join(void* stream);
/* the same in two steps, for callers that launch their own (longest) chain FIRST: under stream capture the first-launched dependant of a node keeps
 * the node's hardware queue.  cffm_branch_mark(stream): remember this point of `stream` (returns 1 when branches are available);
 * cffm_branch_take(stream, i): branch i ordered behind the marked point (or `stream` itself). */
int cffm_branch_mark(void* stream);
void* cffm_branch_take(void* stream, int i);
/* a DEFERRED branch: a library-owned stream of its own for work whose results `stream` needs only much later (the frame classifier's backward
 * of the CFFM heads, cffm_head.py:121, beside the whole CFFM layer's backward).  cffm_defer_begin(stream): that stream, ordered behind `stream`
 * (or `stream` itself); cffm_defer_join(stream): `stream` continues behind it (no-op when nothing is pending).  Nothing on `stream` may read the
 * deferred results before the join.  cffm_add_inplace: a += b (n floats, n % 4 == 0) on a stream. */
void* cffm_defer_begin(void* stream);
int cffm_defer_join(void* stream);
int cffm_add_inplace(float* a, const float* b, long n, void* stream);
int cffm_profile_stage_count(void);
int cffm_profile_null_pair(void* stream); /* stage "event_pair_null": two event records with nothing between (the interval's own cost) */
const char* cffm_profile_stage_name(int i);
int cffm_profile_collect(float* ms /*[stage_count]*/, int* calls /*[stage_count]*/); /* synchronises, sums, clears */
/* Stages enabled while the caller's stream is being CAPTURED into a HIP graph put their event pairs into the graph as
 * event-record nodes (re-recorded by every replay).  This reads, per stage, the intervals of the most recent replay;
 * the pairs stay valid for the life of the graph; reset != 0 forgets them (before capturing another graph). */
int cffm_profile_collect_graph(float* ms /*[stage_count]*/, int* calls /*[stage_count]*/, int reset);

/* ---- stage level (each is one kernel; used by the parity tests and by the block functions) ---- */
/* dst[n][c][r] = src[n][r][c] for n < batch (element strides src_bs / dst_bs between batches) */
int cffm_transpose(const float* src, float* dst, int batch, int rows, int cols, long src_bs, long dst_bs, void* stream);
int cffm_pool_matrix(const float* const pool_w[4], float* M /*[15*49]*/, void* stream);
/* Process-wide: tells the library that EVERY gradient tensor handed to the block / layer backward sits in a slice of a flat buffer
 * padded to a multiple of 4 floats (vss_cffm_amd.ops lays them out so; a data-parallel exchange all-reduces that buffer whole), and
 * asks it to zero the padding itself: the backward of the pooling Linears -- owners of the only tensors whose length is not a multiple
 * of 4 (49 / 49 / 9 weights, four scalar biases) -- writes 3 zeros behind each of them.  Off by default (tensors of their own);
 * vss_cffm_amd.ops switches it on around its own layer-backward calls only.  The setting is PER CALLING THREAD (thread_local). */
void cffm_grad_slices_padded(int yes);
int cffm_ln_pool_fwd(const cffm_geom* g, const float* x_ref, long ref_bs, const float* x_tgt, long tgt_bs,
                     const float* gamma, const float* beta, const float* M, const float* const pool_b[4],
                     float* zall, float* mean, float* rstd, void* stream);
/* the dense additive bias [8 heads][64 queries][304 keys] (cffm_transformer.py:536-587 gathers it from six tables) in two
 * layouts, each may be NULL: bias = query-major fp32 [8,64,304] (checks); biasH = what cffm_attn_fwd / cffm_attn_bwd read: f16
 * B-operand fragments [8 heads][4 waves][10 key-tile pairs][64 lanes][8], entry (h, wave, p, lane = 16 g + j, e) = bias(h, query
 * 16 wave + j, key 16 (2 p + (g >> 1)) + 8 (g & 1) + e), keys 304..319 = 0 -- the kernels add the bias on the matrix pipe
 * (S^T tile t = K Q^T + Sel_(t & 1) * B) from one contiguous 1 KiB load per (wave, tile pair).  (8*4*10*512 halfs = 320 KB; ABI 6:
 * tile pairs, ABI <= 5 kept one tile per fragment.) */
int cffm_bias_assemble(const float* own, const float* ring, const float* const pool[4], float* bias, void* biasH, void* stream);
/* qkv16 [B*RC,768] f16 = zall w^T + b with the q third times 32^-0.5 (cffm_linear_qkv_fwd) */
int cffm_linear_qkv_fwd(const float* zall, const float* w /*[768,256]*/, const float* b /*[768]*/, void* qkv16, long M,
                        void* stream);
int cffm_attn_fwd(const cffm_geom* g, const void* qkv16, const int* key_src /*[nW,304]*/, const int* q_dst /*[nW,49]*/,
                  const void* biasH /* f16 fragments, see cffm_bias_assemble */, float* ao /*[B*HW,256]*/, float* lse /*[B*nW*8,64]*/,
                  void* stream);
/* inv_ptr [RC+1] / inv_idx: CSR inverse of key_src (token row -> the window*304+slot pairs reading it);
 * dkv_part: scratch of B*nW*(304*256 + 8) floats: the per-window dK/dV rows the gather pass sums, kept as f16 [B*nW*304][512]
 * (a row = 8 heads x (K 32 | V 32) since ABI 6) in units of a per-(window, head) power-of-two scale, followed by those scales.
 * Replaces the backward of WindowAttention3d3.forward (cffm_transformer.py:364-606: autograd through the gather / roll / unfold /
 * softmax chain); one fused key-split kernel + the bias-tile sum + the dK / dV gather (csrc/cfm_attn_kernels.h). */
int cffm_attn_bwd(const cffm_geom* g, const void* qkv16, const int* key_src, const int* q_dst,
                  const int* inv_ptr, const int* inv_idx, const void* biasH, const float* ao,
                  const float* dao, const float* lse, float* dqkv /*[B*RC,768] fp32: d(zall w^T), overwritten*/,
                  float* dbiasT /*[8,304,64], overwritten*/, float* dkv_part, void* stream);
/* the last pass of cffm_attn_bwd as a stage (additive under ABI 13): dqkv[b][row][256..767] = the sum, over the (window, slot) pairs
 * inv_idx lists for `row`, of the f16 partial rows of dkv_part times their (window, head) scale.  Per element: the readers in inv_idx
 * order, whole batches of four as ((x0 s0 + x1 s1) + (x2 s2 + x3 s3)) added one batch after the other, then the remaining one to three
 * singly.  Rows >= 49 nW (pooled) also get their q third [0..255] zeroed; the q third of the target rows is left as it is.  Partial
 * rows no reader names are never read. */
int cffm_dkv_gather(const cffm_geom* g, const int* inv_ptr, const int* inv_idx, const float* dkv_part, float* dqkv, void* stream);
/* y[M,N] = x[M,K] w[N,K]^T ;  dx[M,K] = dy[M,N] w[N,K] ;  dw[N,K] = dy[M,N]^T x[M,K]   (row-major, no bias) */
int cffm_linear_fwd(const float* x, const float* w, float* y, long M, int N, int K, void* stream);
/* y[M,N] = x[M,K] w[N,K]^T + b[N]   (a 1x1 convolution on channels-last token rows: the head's classifiers, cffm_head.py:121,147) */
int cffm_linear_bias_fwd(const float* x, const float* w, const float* b, float* y, long M, int N, int K, void* stream);
int cffm_linear_bwd_input(const float* dy, const float* w, float* dx, long M, int N, int K, void* stream);
int cffm_linear_bwd_weight(const float* dy, const float* x, float* dw, long M, int N, int K, void* stream);
/* n <= 4 independent weight gradients (dw_i[N_i,K_i] = dy_i[M_i,N_i]^T x_i[M_i,K_i]) in one launch: the four Linear layers of a
 * block (qkv / proj / fc1 / fc2 .weight.grad, cffm_transformer.py:374, :381, :18-19), none of which feeds the backward chain */
typedef struct { const float* dy; const float* x; float* dw; long M; int N; int K; } cffm_wgrad;
int cffm_linear_bwd_weight_group(const cffm_wgrad* problems /* host */, int n, void* stream);
/* added under ABI 13, additive: the same call with what the block backward passes to the grouped kernel, for the parity tests.  forms (host,
 * [n]): dy_pre / x_pre = 0: the operand is fp32; 1: it is in "split-4" storage ({bf16 hi x4, bf16 lo x4} per 4 floats of a row, same bytes);
 * x_pre = 2: x is gelu(stored + x_bias[K]), applied while the tile is staged (only where the grouped kernel runs: every N and K a multiple of
 * 128, every M >= 32; an error otherwise).  target_wgs: workgroups the launch aims for (sets the common k-slice length; 0 = the default). */
typedef struct { int dy_pre, x_pre; const float* x_bias; } cffm_wgrad_form;
int cffm_linear_bwd_weight_group_forms(const cffm_wgrad* problems /* host */, const cffm_wgrad_form* forms /* host */, int n, int target_wgs,
                                       void* stream);
/* ABI 9: weight gradient with both operands in "T-frag" storage (csrc/dws_kernels.h): MFMA fragments along the contraction -- unit (ks, jt, h)
 * = 64 lanes x 16 B at 16-byte word ((ks * C/16 + jt) * 2 + h) * 64, lane (l15, g) holding x[32 ks + 8 g + e][16 jt + l15], e = 0..7, as bf16
 * hi (h = 0) / lo (h = 1), rows past M zero -- streamed straight into registers: no LDS staging, no barrier in the contraction loop.  The
 * block's row-panel kernels leave z2 / act / dh / dx1 / ao / dout (and the q|k|v panel GEMMs zall / dqkv) in this order for the block's four
 * weight gradients (qkv / proj / fc1 / fc2 .weight.grad, cffm_transformer.py:374, :381, :18-19); cffm_tfrag_pack makes such a copy of a plain
 * row-major fp32 array (dst: cffm_tfrag_floats(R, C) floats).  N a multiple of 64, K of 128. */
long cffm_tfrag_floats(long R, int C);
/* Which form the block's four weight gradients take (process-wide; returns the previous setting, on < 0 only asks): 1 = the streaming kernel on
 * T-frag operands the row-panel kernels leave behind, 0 = the LDS-staged grouped kernel on split-4 / fp32 operands.  A block forward stores its
 * operands in the form the backward will read, so the setting must not change between a forward and its backward. */
int cffm_dw_stream(int on);
int cffm_tfrag_pack(const float* x, float* dst, long R, int C /* % 16 == 0 */, void* stream);
int cffm_linear_bwd_weight_tfrag(const float* dy_t, const float* x_t, float* dw, long M, int N, int K, void* stream);
int cffm_linear_bwd_weight_tfrag_group(const cffm_wgrad* problems /* host; dy / x in T-frag storage */, int n /* <= 4 */, void* stream);
/* ---- fused row-panel stages (round 3): one launch per direction for everything between the attention output and the block
 * output -- proj (cffm_transformer.py:602), residual (:823), norm2 + Mlp (fc1, exact GELU, fc2: :10-26) + residual (:824).
 * Weights are passed in MFMA-fragment order (cffm_panel_pack_weight: form 0 = forward y = x W^T, form 1 = input gradient
 * dx = dy W; N*K floats each; inside a block k_param_prep makes these copies).  z2s / acts / dhs are written in "split-4"
 * storage ({bf16 hi x4, bf16 lo x4} per 4 floats: the operand format of the weight-gradient GEMMs); acts may be NULL (not
 * stored: inside a block the fc2 weight gradient re-applies bias + GELU to hraw while it stages its tiles).
 *   forward : x1 = xt + ao Wp^T + bp; z2 = LN(x1; g2, be2); hraw = z2 W1^T; act = gelu(hraw + b1); x2 = x1 + act W2^T + b2
 *   backward: dh = (dout W2) * gelu'(hraw + b1); dx1 = dout + LN'(dh W1); dao = dx1 Wp; dg2, dbe2, db1, db2 = colsum(dout),
 *             dbp = colsum(dx1) (every one fully written)                                                                   */
int cffm_panel_pack_weight(const float* w, int N, int K, int form, float* w_frag, void* stream);
int cffm_mlp_fwd(const float* ao, const float* xt, long xt_bs, int rows_per_batch, const float* wp_f, const float* w1_f,
                 const float* w2_f, const float* bp, const float* b1, const float* b2, const float* g2, const float* be2,
                 float* x1, float* z2s, float* mean2, float* rstd2, float* hraw, float* acts, float* x2, long NP, void* stream);
int cffm_mlp_bwd(const float* dout, const float* hraw, const float* b1, const float* x1, const float* mean2,
                 const float* rstd2, const float* g2, const float* w2_n, const float* w1_n, const float* wp_n, float* dhs,
                 float* dx1, float* dao, float* dg2, float* dbe2, float* db1, float* db2, float* dbp, long NP, void* stream);
/* added under ABI 13, additive: cffm_mlp_fwd whose x2 leaves as NCHW images instead of token rows (what the layer's last block runs,
 * so that no layout pass follows it): row m is pixel m % rows_per_batch of image m / rows_per_batch, and feature n of it goes to
 * x2_nchw[(m / rows_per_batch) * x2_bs + n * rows_per_batch + m % rows_per_batch]; x2_bs >= 256 * rows_per_batch floats, nothing
 * between the images is touched.  Same arithmetic: the values (and every other output) are those of cffm_mlp_fwd, bit for bit. */
int cffm_mlp_fwd_nchw(const float* ao, const float* xt, long xt_bs, int rows_per_batch, const float* wp_f, const float* w1_f,
                      const float* w2_f, const float* bp, const float* b1, const float* b2, const float* g2, const float* be2,
                      float* x1, float* z2s, float* mean2, float* rstd2, float* hraw, float* acts, float* x2_nchw, long x2_bs,
                      long NP, void* stream);
/* ... and cffm_mlp_bwd whose upstream gradient is read from NCHW images (same indexing, dy_bs >= 256 * rows_per_batch) instead of from
 * token rows; the rows [NP,256] of it are written to dout_rows (inside a block the fc2 weight gradient reads them).  Every output
 * equals cffm_mlp_bwd's on the transposed gradient, bit for bit. */
int cffm_mlp_bwd_nchw(const float* dy_nchw, long dy_bs, int rows_per_batch, float* dout_rows, const float* hraw, const float* b1,
                      const float* x1, const float* mean2, const float* rstd2, const float* g2, const float* w2_n, const float* w1_n,
                      const float* wp_n, float* dhs, float* dx1, float* dao, float* dg2, float* dbe2, float* db1, float* db2,
                      float* dbp, long NP, void* stream);
int cffm_colsum(const float* a, long rows, int cols /* multiple of 4 */, float* out /* overwritten */, void* stream);
/* added under ABI 13, additive: the block's q|k|v Linear as a stage -- qkv16 [M,768] f16 = x w^T + b with the q third times 32^-0.5, from
 * x in split-4 storage ([M,256]) and w in fragment order (cffm_panel_pack_weight of w [768,256], form 0).  Each workgroup computes one of
 * the q / k / v column thirds of a row panel, two workgroups per CU.  x_t (or NULL): also writes the T-frag copy of x
 * (cffm_tfrag_floats(M, 256) floats, rows past M zero). */
int cffm_panel_qkv_fwd(const float* x_split4, const float* w_frag, const float* b /*[768]*/, void* qkv16, long M, float* x_t, void* stream);
/* added under ABI 13, additive: three pieces of the block backward as stages (what cffm_block_backward / cffm_layer_backward* run, through
 * the same launch helpers), for the parity tests.
 *
 * cffm_ln_pool_bwd: the CFFA backward -- the whole adjoint of cffm_pool_matrix + cffm_ln_pool_fwd -- for n = 1..8 blocks that share the
 * reference frames x_ref [B,3,HW,256] (batch stride ref_bs).  Per block (a HOST array of n structs): x_tgt [B,HW,256] (batch stride tgt_bs),
 * norm1's gamma / beta, the block's composed pooling matrix M [15*49], mean / rstd [B*4*HW] as cffm_ln_pool_fwd wrote them (the reference
 * pass reads the copy of the first block of each launch), the token-row gradient dzall [B*RC,256] (rows of padded target pixels are not
 * read) and dres [B*HW,256] or NULL, the residual-path gradient added to dx_tgt.  Written per block: dx_tgt [B,HW,256] (batch stride
 * dtgt_bs), dgamma / dbeta [256], dpool_w (49 / 49 / 9 / 4 floats) and dpool_b (1 float each; with cffm_grad_slices_padded(1) also 3 zeros
 * behind the first three weights and behind every bias).  dx_ref [B,3,HW,256] (batch stride dref_bs) = the sum over the blocks, added to
 * what it holds when accum_ref != 0.  Blocks go four per reference launch (blocks 0..3, then 4..7), the second launch accumulating. */
typedef struct cffm_cffa_bwd_block {
    const float* x_tgt; long tgt_bs;
    const float *gamma, *beta, *M, *mean, *rstd, *dzall, *dres;
    float* dx_tgt; long dtgt_bs;
    float *dgamma, *dbeta, *dpool_w[4], *dpool_b[4];
} cffm_cffa_bwd_block;
int cffm_ln_pool_bwd(const cffm_geom* g, int n, const cffm_cffa_bwd_block* blocks /* host [n] */, const float* x_ref, long ref_bs,
                     float* dx_ref, long dref_bs, int accum_ref, void* stream);
/* added under ABI 13, additive: the end of a range of block backwards as stages.
 *
 * A record set: `count` records `stride` floats apart (rec 16-byte aligned, stride a multiple of 4 and >= total rounded up to 4); column c
 * < total of the records is summed in a fixed order and written to (accumulate[k] != 0: added to) out[k][c - off[k]] of every segment k with
 * off[k] <= c < off[k] + width[k] (nseg <= 8).
 * cffm_reduce_records: up to 10 record sets in one launch (the second stage of every block-partial reduction).
 * cffm_pool_matrix_bwd: dM [15*49] of n = 1..4 blocks -> their pooling-weight gradients dpool_w (49 / 49 / 9 / 4 floats; dpool_b is not
 * written, but with cffm_grad_slices_padded(1) the 3 floats behind the first three weights and behind each dpool_b are zeroed).
 * cffm_bwd_tail: ONE launch of workgroups that do not depend on each other -- the sums of the record sets and the tiles of
 * dst[z][c][r] = src[z][r][c] (+ addend[z][c][r] unless z % add_mod == add_skip; tr or tr->addend may be NULL).  The bits are those of
 * cffm_reduce_records and of cffm_transpose (+ one fp32 addition). */
typedef struct cffm_record_set {
    const float* rec; int count, stride, total;
    int nseg, off[8], width[8], accumulate[8];
    float* out[8];
} cffm_record_set;
typedef struct cffm_pool_grads { const float* dM; float *dpool_w[4], *dpool_b[4]; } cffm_pool_grads;
typedef struct cffm_tail_transpose {
    const float* src; float* dst; int batch, rows, cols; long src_bs, dst_bs;
    const float* addend; int add_mod, add_skip;
} cffm_tail_transpose;
int cffm_reduce_records(int nsets, const cffm_record_set* sets /* host [nsets] */, void* stream);
int cffm_pool_matrix_bwd(int n, const cffm_pool_grads* blocks /* host [n] */, void* stream);
int cffm_bwd_tail(int nsets, const cffm_record_set* sets /* host [nsets] */, const cffm_tail_transpose* tr, void* stream);
/* the q|k|v input gradient: dx [M,256] = dqkv [M,768] w, dqkv fp32, w in fragment order (cffm_panel_pack_weight of w [768,256], form 1);
 * db (or NULL) [768] = the column sums of dqkv (qkv.bias.grad: records out of the same launch, then one reduction); dqkv_t (or NULL): also
 * writes the T-frag copy of dqkv (cffm_tfrag_floats(M, 768) floats, rows past M zero).  Nothing past row M of dqkv is read. */
int cffm_panel_qkv_bwd_input(const float* dqkv, const float* w_frag, float* dx, float* db, float* dqkv_t, long M, void* stream);
/* the adjoint of cffm_bias_assemble: dbiasT [8 heads][304 keys][64 queries] (key-major, as cffm_attn_bwd leaves it) -> the gradients of
 * the six tables (shapes as in cffm_block_params), every entry written; query columns 49..63 and key rows 289..303 are not read. */
int cffm_bias_scatter(const float* dbiasT, float* down, float* dring, float* const dpool[4], void* stream);

/* ---- CFFM++ global temporal context (WindowAttention_cluster, pvt/swin_transformer_2d.py:208-262) ---- */
/* q_raw [B*T,256] = LN(x) Wq^T without bias, kv_raw [B*K,512] = LN(centers) Wkv^T without bias; softmax over the K
 * prototypes per (token, head); o [B*T,256]; lse [B*T,8].  K <= 128: on the matrix pipe (three-pass bf16 split of every product: the
 * 1e-4 tolerance of the fp32 form is kept), the head's Kc / Vc packed once per call as MFMA fragments; above: fp32 on the VALU.  The
 * backward's `o` is not read by the matrix-pipe form (D = sum_keys p dp comes out of the same products as dp). */
int cffm_gtc_attn_fwd(const float* q_raw, const float* q_b, const float* kv_raw, const float* kv_b, float* o, float* lse,
                      int B, int T, int K, void* stream);
int cffm_gtc_attn_bwd(const float* q_raw, const float* q_b, const float* kv_raw, const float* kv_b, const float* o,
                      const float* dout, const float* lse, float* dq_raw, float* dkv /* overwritten */, int B, int T, int K,
                      void* stream);

/* The whole block of the CFFM++ prototype layer in one call per direction (round 5, ABI 7; replaces the ~33 stage launches a caller
 * had to sequence): SwinTransformerBlock_cluster.forward, pvt/swin_transformer_2d.py:605-665, shift 0, with
 * WindowAttention_cluster.forward :208-262 inside (only_use_cluster_center_as_context, :216: no in-window keys, no position bias, no mask
 * -- window partition / padding are numerically no-ops, SURVEY.md A "GTC is window-independent").
 *   x [B,T,256] tokens, centers [B,K,256] prototypes (1 <= K <= 256), out [B,T,256]; `ws`: cffm_gtc_ws_floats(B, T, K) floats, written
 *   by the forward and read (and extended) by the backward of the same call pair.
 * Parameter order = the reference's state_dict of `decoder_swin.blocks.0`: norm1, attn.qkv (only its first 256 rows / entries -- the q
 * third -- are used and receive a gradient; the rest of the gradient is written as zeros), attn.qkv_cluster, attn.proj_cluster, norm2,
 * mlp.fc1, mlp.fc2.  (attn.proj and attn.relative_position_bias_table exist in the reference module but receive no gradient: not here.) */
typedef struct {
    const float *norm1_w, *norm1_b, *qkv_w /* [768,256] */, *qkv_b /* [768] */, *kv_w /* [512,256] */, *kv_b /* [512] */, *proj_w, *proj_b,
        *norm2_w, *norm2_b, *fc1_w, *fc1_b, *fc2_w, *fc2_b;
} cffm_gtc_params;
typedef struct {
    float *norm1_w, *norm1_b, *qkv_w, *qkv_b, *kv_w, *kv_b, *proj_w, *proj_b, *norm2_w, *norm2_b, *fc1_w, *fc1_b, *fc2_w, *fc2_b;
} cffm_gtc_grads;
long cffm_gtc_ws_floats(int B, int T, int K);
int cffm_gtc_block_forward(const cffm_gtc_params* p, const float* x, const float* centers, float* out, float* ws, int B, int T, int K,
                           void* stream);
int cffm_gtc_block_backward(const cffm_gtc_params* p, const cffm_gtc_grads* g, const float* x, const float* centers, const float* dout,
                            float* dx, float* dcenters, float* ws, int B, int T, int K, void* stream);

/* ABI 10: the composed embedding weights of ops.segformer_fuse (cffm_head.py:102-119 without the 1024-channel concat): mats[i] [e][C_i] =
 * Wf_i W_i (Wf_i = input-channel block k - 1 - i of linear_fuse.conv.weight [e][k e], W_i = linear_c{i+1}.proj.weight), d [e] = sum_i Wf_i b_i;
 * and the gradients of the nine tensors from dmats / dd.  The k products run on branches of their own (cffm_branch_begin). */
int cffm_fuse_compose_fwd(const float* fuse_w, const float* const* lin_w /* host [k] */, const float* const* lin_b /* host [k] */,
                          const int* C_in /* host [k] */, int k /* <= 4 */, int e /* 256 */, float* const* mats /* host [k] */, float* d, void* stream);
int cffm_fuse_compose_bwd(const float* fuse_w, const float* const* lin_w, const float* const* lin_b, const int* C_in, int k, int e,
                          const float* const* dmats /* host [k] */, const float* dd, float* dfuse_w /* [e][k e] */, float* const* dlin_w /* host [k] */,
                          float* const* dlin_b /* host [k] */, void* stream);

/* ---- SegFormer embedding in front of the hot path, without the 1024-channel concat ----
 * Replaces cffm_head.py:102-119 (4 x `MLP` embed, 3 x bilinear resize to the 1/4 map, torch.cat, 1x1 `linear_fuse.conv`):
 * conv(cat_i up_i(W_i c_i + b_i)) = sum_i up_i((Wf_i W_i) c_i) + sum_i Wf_i b_i.  The host embeds every scale once at its own
 * resolution with the composed matrix (cffm_linear_fwd on token rows) and calls this for the full-resolution pass:
 *   y [N*H*W,256] (the 1/4-scale embedding on entry) += d[256] + sum_m bilinear(z_m [N*h_m*w_m,256] -> H x W)
 * with F.interpolate(mode='bilinear', align_corners=False) taps; nmaps <= 3, resize factors <= 16 per dimension. */
int cffm_segfuse_fwd(float* y, const float* d, const float* const z[3], const int h[3], const int w[3], int nmaps, int N,
                     int H, int W, void* stream);
/* the adjoint of the three resizes: dz_m [N*h_m*w_m,256] = up_m^T g, g [N*H*W,256] (gather form, deterministic) */
int cffm_segfuse_bwd(const float* g, float* const dz[3], const int h[3], const int w[3], int nmaps, int N, int H, int W,
                     void* stream);
/* added under ABI 13, additive: the eval tail of a frame in one pass (streaming inference).  With y, d, z, h, w, nmaps as for
 * cffm_segfuse_fwd (y is only read here), H and W even, and scale / shift = coef[0] / coef[1] of cffm_bn_finalize_fwd(part = NULL):
 *   out[n, patch, :] = 0.25 * ((r00 + r01) + (r10 + r11)),   r = max((y + d + sum_m bilinear(z_m)) * scale + shift, 0)
 * over the 2 x 2 patches of the map: rows [N, H/2 * W/2, 256] with the bits of cffm_segfuse_fwd followed by cffm_bn_relu_pool_fwd's `stack`;
 * the pre-BN map and `fused` are never written.  out = ring + slot * slot_floats, slot = slots[which] read on the device (slots: device
 * int[4], which in 0..3; NULL: slot 0, which = 0) and clamped there into [0, nslots): a bad table cannot address outside the ring.
 * slot_floats >= N * H/2 * W/2 * 256, a multiple of 4.  Odd H or W, null or misaligned pointers (16 bytes; the table 4), and a ring that
 * overlaps y, d, scale, shift or a map are errors, returned before anything is enqueued.  One launch on `stream`, no LDS, no atomics. */
int cffm_segfuse_pool_fwd(const float* y, const float* d, const float* const z[3], const int h[3], const int w[3], int nmaps,
                          const float* scale, const float* shift, float* ring, long slot_floats, int nslots, const int* slots, int which,
                          int N, int H, int W, void* stream);
/* added under ABI 13, additive: the same with ONE SLOT PER FRAME (a chunk of a video in one call).  Frame n's H/2 * W/2 rows go to
 * ring + clamp(slots[n], 0, nslots - 1) * slot_floats; slots is a DEVICE int[N] read by the kernel, so a captured launch serves any slots;
 * slot_floats >= H/2 * W/2 * 256 (one frame), a multiple of 4.  Arithmetic and parenthesisation are cffm_segfuse_pool_fwd's: the rows have
 * the bits of N calls of it at N = 1 on the frames' slices of the inputs.  Two frames that name the same slot are the caller's mistake: that
 * slot then holds an unspecified mix of their rows; nothing is written outside the ring (the clamp).  Refused before anything is enqueued:
 * odd H or W, null or misaligned pointers (16 bytes; the table 4, and it must not be NULL), a ring that overlaps y, d, scale, shift, the
 * table or a map.  One launch on `stream`, no LDS, no atomics. */
int cffm_segfuse_pool_fwd_frames(const float* y, const float* d, const float* const z[3], const int h[3], const int w[3], int nmaps,
                                 const float* scale, const float* shift, float* ring, long slot_floats, int nslots, const int* slots, int N,
                                 int H, int W, void* stream);

/* ---- the head's training loss without full-resolution logits ----
 * Replaces decode_head.py:744-835's resize(seg_logit, size=label size, 'bilinear', align_corners=False) followed by
 * F.cross_entropy(reduction='none', ignore_index) (losses/cross_entropy_loss.py:9-40) and `accuracy` (losses/accuracy.py:4):
 * logits [M,K,h,w] fp32, labels [M,H,W] int64 (ignore_index, and anything outside [0,K), contributes 0), H <= 8h, W <= 8w, K <= 256.
 * fwd: lse [M,H,W] (log-sum-exp of the interpolated logits, kept for bwd); part [cffm_upce_blocks(...)][2]: per-workgroup
 *      sums of the per-pixel losses and of the pixels whose arg-max is the label (the caller adds them up and divides).
 * bwd: dlogits [M,K,h,w] = scale * (*gscale, device scalar, or 1 when NULL) * d(sum of per-pixel losses)/dlogits. */
long cffm_upce_blocks(int M, int H, int W);
int cffm_upce_fwd(const float* logits, const long long* labels, float* lse, float* part, int M, int K, int h, int w, int H, int W,
                  int ignore_index, void* stream);
int cffm_upce_bwd(const float* logits, const long long* labels, const float* lse, const float* gscale, float scale,
                  float* dlogits, int M, int K, int h, int w, int H, int W, int ignore_index, void* stream);
/* The same with the caller's layout of the logits / their gradient (the heads keep them as token rows straight out of the classifier
 * GEMMs, the T frame maps and the clip-level map of a clip in one buffer): element (map m, class k, cell (r, c)) at
 *   (m / inner) * ms_outer + (m % inner) * ms_inner + k * ks + (r * w + c) * ps      (floats; one of ks, ps is 1)
 * label_idx[M] (device int32, NULL = identity): the label map a logits map is judged on (the clip-level map: the last frame's);
 * map_scale[M] (device fp32, NULL = 1): per-map factor on the gradient (0.5 / pixels for frame maps, 1 / pixels for clip maps:
 * decode_head.py:805-835); part records are ordered map-major (cffm_upce_blocks(M,H,W) / M per map), so the caller weights them. */
int cffm_upce_maps_fwd(const float* logits, const long long* labels, const int* label_idx, float* lse, float* part, int M, int K, int h,
                       int w, int H, int W, int ignore_index, int inner, long ms_outer, long ms_inner, int ks, int ps, void* stream);
/* ABI 10: the two loss scalars from those records on the device: out[0] = sum_m wl[m] * sum(loss records of map m), out[1] = sum_m wh[m] *
 * sum(hit records of map m), accumulated in double in a fixed order (wl, wh: M doubles each, device) -- decode_head.py:805-835's weighting. */
int cffm_upce_maps_finalize(const float* part, int M, long per, const double* wl, const double* wh, float* out /* [2] */, void* stream);
int cffm_upce_maps_bwd(const float* logits, const long long* labels, const int* label_idx, const float* lse, const float* gscale,
                       const float* map_scale, float scale, float* dlogits, int M, int K, int h, int w, int H, int W, int ignore_index,
                       int inner, long ms_outer, long ms_inner, int ks, int ps, void* stream);

/* ---- evaluation counts ----
 * mmseg/core/evaluation/metrics.py:62-119 `intersect_and_union` for one prediction / label map pair of n pixels (both int64 on
 * the device): counts [3][num_classes] int64 = per-class pixels of (prediction == label) | prediction | label, over the pixels
 * whose label is not ignore_index, ACCUMULATED into what is there (zero it first; `total_intersect_and_union` = call per image);
 * union = prediction + label - intersect.  Exact integers; num_classes <= 1024; at most 2^32 pixels per call. */
int cffm_seg_counts(const long long* pred, const long long* label, long n, int num_classes, int ignore_index,
                    int reduce_zero_label, long long* counts, void* stream);

/* video consistency VC_n, VC_perclip.py:62-78 `get_common`: gt / pred [F, npix] int64 label maps of one video; for every start
 * frame i < F - n: counts[i][0] += pixels whose label is constant over frames i..i+n-1 in BOTH gt and pred, counts[i][1] += pixels
 * constant in gt (acc_i = counts[i][0] / counts[i][1]); counts int64 [F - n][2], zero it first. */
int cffm_vc_counts(const long long* gt, const long long* pred, int F, long npix, int n, long long* counts, void* stream);

/* ---- block / layer level ---- */
/* x_ref: NHWC frames 0..2 [B,3,HW,256] (batch stride ref_bs), x_tgt NHWC target [B,HW,256] (stride tgt_bs);
 * writes the block's saved activations into `ws` (layout: cffm_block_ws_layout; ws[x2] is the output). */
int cffm_block_forward(const cffm_geom* g, const cffm_block_params* p, const float* x_ref, long ref_bs,
                       const float* x_tgt, long tgt_bs, const int* key_src, const int* q_dst, float* ws,
                       float* scratch, void* stream);
int cffm_block_backward(const cffm_geom* g, const cffm_block_params* p, const cffm_block_grads* gr,
                        const float* x_ref, long ref_bs, const float* x_tgt, long tgt_bs, const int* key_src,
                        const int* q_dst, const int* inv_ptr, const int* inv_idx, const float* ws,
                        const float* dout /*[B*HW,256]*/,
                        float* dx_ref, long dref_bs, int accum_ref, float* dx_tgt, long dtgt_bs,
                        float* scratch, void* stream);
/* x [B,4,256,H0,W0] -> y_tgt [B,256,H0,W0] (frames 0..2 of the reference's output equal the input) */
int cffm_layer_forward(const cffm_geom* g, int depth, const cffm_block_params* params, const float* x_nchw,
                       float* y_tgt_nchw, const int* key_src, const int* q_dst, float* saved, float* scratch,
                       void* stream);
/* dy_tgt [B,256,H0,W0] -> dx [B,4,256,H0,W0] (gradient through the hot path only; the pass-through of
 * frames 0..2 is the caller's torch.cat) and every parameter gradient of every block */
int cffm_layer_backward(const cffm_geom* g, int depth, const cffm_block_params* params, const cffm_block_grads* grads,
                        const float* dy_tgt_nchw, long dy_bs /* elements between clips: 256*H0*W0 when dy is dense, 4x that
                        when it is the last-frame slice of a [B,4,256,H0,W0] gradient */, float* dx_nchw, const int* key_src, const int* q_dst,
                        const int* inv_ptr, const int* inv_idx, const float* saved, float* scratch, void* stream);
/* The same in pieces: blocks first_block, first_block - 1, ..., last_block (depth - 1 >= first >= last >= 0), issued in order on
 * one stream; the piece with first == depth - 1 starts from dy, the piece with last == 0 writes dx.  Lets a data-parallel
 * trainer start the gradient all-reduce of block i while block i - 1 is still running (mmseg/apis/train.py:57-65). */
int cffm_layer_backward_range(const cffm_geom* g, int depth, const cffm_block_params* params, const cffm_block_grads* grads,
                        const float* dy_tgt_nchw, long dy_bs /* elements between clips: 256*H0*W0 when dy is dense, 4x that
                        when it is the last-frame slice of a [B,4,256,H0,W0] gradient */, float* dx_nchw, const int* key_src, const int* q_dst,
                        const int* inv_ptr, const int* inv_idx, const float* saved, float* scratch, int first_block, int last_block, void* stream);
/* The same pair on the reference's whole output (BasicLayer3d3.forward returns [B,4,C,H,W] whose frames 0..2 ARE the input frames,
 * cffm_transformer.py:826,917-927): forward writes y_full = [x[:, :3] | new target frame] (the copy runs on the library's side
 * stream under the blocks), backward takes the upstream gradient of that whole tensor and adds its pass-through frames into dx in
 * the final layout pass -- no torch.cat, no zero-fill / add of the pass-through gradient around the call. */
int cffm_layer_forward_full(const cffm_geom* g, int depth, const cffm_block_params* params, const float* x_nchw,
                            float* y_full_nchw, const int* key_src, const int* q_dst, float* saved, float* scratch,
                            void* stream);
int cffm_layer_backward_full(const cffm_geom* g, int depth, const cffm_block_params* params, const cffm_block_grads* grads,
                             const float* dy_full_nchw, float* dx_nchw, const int* key_src, const int* q_dst, const int* inv_ptr,
                             const int* inv_idx, const float* saved, float* scratch, int first_block, int last_block, void* stream);

/* The layer on token rows (channels-last) on both sides -- what the heads call (their neighbours work on rows too):
 * x_rows [B,4,HW,256] -> y_rows [B,HW,256]; no layout transposes, `x_rows` itself is the stack the blocks read and must be
 * handed to the backward again; dy_rows [B,HW,256] -> dx_rows [B,4,HW,256]. */
int cffm_layer_forward_rows(const cffm_geom* g, int depth, const cffm_block_params* params, const float* x_rows, float* y_rows,
                            const int* key_src, const int* q_dst, float* saved, float* scratch, void* stream);
int cffm_layer_backward_rows(const cffm_geom* g, int depth, const cffm_block_params* params, const cffm_block_grads* grads,
                             const float* x_rows, const float* dy_rows, float* dx_rows, const int* key_src, const int* q_dst,
                             const int* inv_ptr, const int* inv_idx, const float* saved, float* scratch, void* stream);

/* ---- ABI 12: the layer's forward for inference (nothing is kept for a backward) ----
 * The same kernels as the training forward in store-free instantiations: the output equals cffm_layer_forward_rows / _forward_full
 * bit for bit.  What depends on the parameters alone -- per block the f16 position-bias fragments, the pooling matrix and the
 * forward-form fragment-ordered copies of the four Linear weights -- is prepared ONCE per set of weights:
 *   cffm_layer_prepared_floats: floats of `prepared` for a layer of `depth` blocks (independent of the geometry);
 *   cffm_layer_prepare:         fills it; call again whenever a parameter has changed;
 *   cffm_layer_infer_ws_floats: floats of the transient workspace `ws` (zall | f16 q|k|v | ao | two x2 buffers the blocks
 *                               ping-pong between): independent of depth, contents undefined before and after a call;
 *   cffm_layer_infer_rows:      x_rows [B,4,HW,256] -> y_rows [B,HW,256] (the new target frame), channels-last on both sides;
 *   cffm_layer_infer_full:      x [B,4,256,H0,W0] -> y_full [B,4,256,H0,W0], frames 0..2 = the input frames
 *                               (y_full also serves as scratch during the call; it must not alias x).
 * Everything is enqueued on `stream` alone (no side streams, no allocation): a call captured into a HIP graph is one chain. */
long cffm_layer_prepared_floats(int depth);
int cffm_layer_prepare(int depth, const cffm_block_params* params, float* prepared, void* stream);
long cffm_layer_infer_ws_floats(const cffm_geom* g);
int cffm_layer_infer_rows(const cffm_geom* g, int depth, const cffm_block_params* params, const float* prepared, const float* x_rows,
                          float* y_rows, const int* key_src, const int* q_dst, float* ws, void* stream);
int cffm_layer_infer_full(const cffm_geom* g, int depth, const cffm_block_params* params, const float* prepared, const float* x_nchw,
                          float* y_full_nchw, const int* key_src, const int* q_dst, float* ws, void* stream);
/* added under ABI 13, additive: cffm_layer_infer_rows on four frames that lie in a ring of per-frame row buffers (streaming inference).
 * Frame t (0..3, the target last) of sample b is ring + clamp(slots[t], 0, nslots - 1) * slot_floats + b * frame_bs, [HW,256] floats;
 * slots is a DEVICE int[4] read by the kernels, entries may repeat.  No pointer argument depends on the table, so a captured call is
 * replayed for other frames by rewriting the table.  The target frame is also block 0's residual.  Same prepared data, same workspace
 * (cffm_layer_infer_ws_floats), every launch on `stream`; the ring is only read.  y_rows or ws inside the ring is an error.  With
 * ring = x_rows, slot_floats = HW * 256, nslots = 4, slots = {0,1,2,3} and frame_bs = 4 * HW * 256 the call is cffm_layer_infer_rows. */
int cffm_layer_infer_rows_ring(const cffm_geom* g, int depth, const cffm_block_params* params, const float* prepared, const float* ring,
                               long slot_floats, int nslots, const int* slots, long frame_bs, float* y_rows, const int* key_src,
                               const int* q_dst, float* ws, void* stream);
/* added under ABI 13, additive: the same with ONE TABLE PER SAMPLE (the g->B targets of a chunk of one video, each with its own clip, in one
 * call).  Frame t of sample b is ring + clamp(slots[4 * b + t], 0, nslots - 1) * slot_floats, [HW,256] floats; slots is a DEVICE int[B * 4].
 * There is no frame_bs: every sample reads whole slots of the one ring, and entries may repeat within a sample and across samples.  Block
 * 0's residual is sample b's own target (slots[4 * b + 3]).  Same prepared data, same workspace (cffm_layer_infer_ws_floats at g->B), every
 * launch on `stream`; the ring is only read.  y_rows or ws inside the ring is an error, as is a null or misaligned table.  With B = 1 the
 * call is cffm_layer_infer_rows_ring; with B > 1 sample b's rows have the bits of a B = 1 call of it with that sample's four entries. */
int cffm_layer_infer_rows_ring_tables(const cffm_geom* g, int depth, const cffm_block_params* params, const float* prepared, const float* ring,
                                      long slot_floats, int nslots, const int* slots, float* y_rows, const int* key_src, const int* q_dst,
                                      float* ws, void* stream);

/* ---- `linear_fuse`'s BatchNorm + ReLU and the 1/4 -> 1/8 resize that builds the clip stack (cffm_head.py:119, :131-135), on token
 * rows [pixels,256].  With even H, W the bilinear 1/2 resize (align_corners=False) is exactly a 2x2 average.
 *   cffm_colstats:          part[cffm_colstats_records(rows)][512] = per-workgroup column sums | sums of squares of y [rows,256]
 *                           (the caller adds the records -- in fp64 -- and, under SyncBN, all-reduces them)
 *   cffm_bn_relu_pool_fwd:  fused = max(y*scale + shift, 0) [N*H*W,256]; stack = 2x2 average of fused [N*(H/2)*(W/2),256] (or NULL)
 *   cffm_bn_relu_pool_bwd1: g = [y*scale+shift > 0] * (dfused + dstack(parent)/4) (g may alias dfused; either gradient may be
 *                           NULL); part[cffm_bn_relu_pool_records(N,H,W)][512] = sums of g | g*xhat, xhat = y*xs + xo
 *   cffm_bn_bwd2:           g <- c1 * (g - mg - xhat*mgx)   (c1 = gamma*rstd, mg / mgx = per-channel means of g / g*xhat)
 *   mask (fwd / bwd1, may be NULL): Dropout2d in front of `linear_pred` (cffm_head.py:120) folded in: [N,256] factors 0 or 1/(1-p) per
 *                           (frame, channel), applied to `fused` (not to `stack`) and to dfused
 *   cffm_bn_finalize_fwd:   the per-channel arithmetic between the passes in one launch: part (NULL = eval mode, running statistics)
 *                           -> coef[4][256] = scale | shift | rstd | -mean*rstd (fp64 inside); running buffers updated as torch does
 *   cffm_bn_finalize_bwd:   part -> out[5][256] = dbias | dweight | mean g | mean g*xhat (0 in eval mode) | gamma*rstd */
long cffm_colstats_records(long rows);
int cffm_colstats(const float* y, long rows, float* part, void* stream);
long cffm_bn_relu_pool_records(int N, int H, int W);
int cffm_bn_relu_pool_fwd(const float* y, const float* scale, const float* shift, const float* mask, float* fused, float* stack, int N,
                          int H, int W, void* stream);
int cffm_bn_relu_pool_bwd1(const float* y, const float* scale, const float* shift, const float* xs, const float* xo, const float* mask,
                           const float* dfused, const float* dstack, float* g, float* part, int N, int H, int W, void* stream);
int cffm_bn_bwd2(float* g, const float* y, const float* xs, const float* xo, const float* c1, const float* mg, const float* mgx, long rows,
                 void* stream);
int cffm_bn_finalize_fwd(const float* part, long nrec, double count, const float* weight, const float* bias, float* running_mean,
                         float* running_var, float momentum, float eps, float* coef, void* stream);
int cffm_bn_finalize_bwd(const float* part, long nrec, double count, const float* weight, const float* xs, int training, float* out,
                         void* stream);
/* Bilinear resize (align_corners = False, ATen's tap rule and nesting) of token rows [N][h*w][C] -> [N][H*W][C], maps `*_map_stride`
 * floats apart (so a map may sit inside a larger buffer: the clip-level logits inside the [B, T+1, h, w, K] logits rows,
 * cffm_head.py:149); C % 4 == 0.  bwd = the adjoint in gather form (deterministic), reading the gradient where it lies. */
int cffm_rows_resize_fwd(const float* src, long src_map_stride, float* dst, long dst_map_stride, int N, int h, int w, int H, int W, int C,
                         void* stream);
int cffm_rows_resize_bwd(const float* ddst, long ddst_map_stride, float* dsrc, long dsrc_map_stride, int N, int h, int w, int H, int W, int C,
                         void* stream);

/* ---- clip data path after decoding: the `*_clips` transforms of local_configs/_base_/datasets/vspw_repeat2.py:8-19
 * -- LoadAnnotations(reduce_zero_label), RandomCrop_clips (transforms.py:1524), RandomFlip_clips (:852), Normalize_clips (:1260),
 * Pad_clips (:990), DefaultFormatBundle_clips (formating.py:261) -- applied to a whole clip in one pass.
 * frames [T,H,W,3] uint8 (BGR as decoded), labels [T,H,W] uint8 or NULL (then out_lab must be NULL);
 * crop box rows y1..y1+ch-1, columns x1..x1+cw-1 (one box for all frames), then an optional horizontal flip, BGR->RGB (to_rgb),
 * (v - mean) * (1/std) in float32, padding of the bottom / right to Ho x Wo with pad_val (image, after normalisation) and
 * seg_pad_val (labels); out_img [T,3,Ho,Wo] float32, out_lab [T,1,Ho,Wo] int64.  The random draws stay on the host
 * (vss_cffm_amd/data.py draws them in the reference's order). */
/* The whole of PhotoMetricDistortion_clips.__call__ (mmseg/datasets/pipelines/transforms.py:2028-2150, ABI 8) between flip and
 * normalisation, per frame: brightness (v = u8(clip(v + beta)), convert() :2057, in float32 as numpy does), contrast when
 * contrast_first[t] (the reference's mode == 1), saturation (:2082-2091: S of mmcv.bgr2hsv = cv2 COLOR_BGR2HSV scaled by saturation[t],
 * convert()-style, back through COLOR_HSV2BGR), hue (:2093-2102: H + hue_shift[t] mod 180, its own round trip), contrast when
 * !contrast_first[t] (v = u8(clip(v * alpha))).  HOST arrays of T entries or NULL; NaN = branch not taken; hue_shift holds integers.  The two colour conversions
 * restate OpenCV's 8-bit arithmetic (color_hsv.cpp RGB2HSV_b: integer with the 12-bit division tables, hue range 180; HSV2RGB_b: float32
 * through HSV2RGB_native, * 255, cvRound) -- OpenCV is not available where this library is built or tested, so that restatement is checked
 * against oracle/cv_oracle.py only (parity unpinned). */
int cffm_clip_format_hsv(const unsigned char* frames, const unsigned char* labels, float* out_img, long long* out_lab, int T, int H, int W,
                         int y1, int x1, int ch, int cw, int flip, int Ho, int Wo, const float mean[3], const float std[3], int to_rgb,
                         float pad_val, int seg_pad_val, int reduce_zero_label, const float* brightness_beta, const float* contrast_alpha,
                         const int* contrast_first, const float* saturation, const float* hue_shift, void* stream);
/* ABI 8: cv2.resize of a clip, as mmcv.imrescale / imresize call it from Resize (transforms.py:475, config vspw_repeat2.py:10) and
 * AlignedResize_clips (:236, config :27): frames [T,H,W,3] uint8 -> out_frames [T,Ho,Wo,3] with INTER_LINEAR (OpenCV's 8-bit path:
 * 11-bit fixed-point weights, horizontal then vertical pass, the 2x2 -> 1 case as INTER_AREA's box mean), labels [T,H,W] uint8 ->
 * out_labels [T,Ho,Wo] with INTER_NEAREST; either pair may be NULL.  The target size is the caller's (vss_cffm_amd/data.py applies
 * mmcv.rescale_size and the size_divisor alignment).  Restated from resize.cpp; parity unpinned like cffm_clip_format_hsv. */
int cffm_clip_resize(const unsigned char* frames, const unsigned char* labels, int T, int H, int W, unsigned char* out_frames,
                     unsigned char* out_labels, int Ho, int Wo, void* stream);

/* ---- parameter update of the training step (the reference trains the head with AdamW, lr 6e-5, betas (0.9, 0.999),
 * weight decay 0.01: local_configs/cffm/B1/cffm.b1.480x480.vspw2.160k.py:35) ----
 * One launch over every parameter tensor of the hot path: `chunks` is a device table, one entry per <= CFFM_ADAMW_CHUNK
 * consecutive elements of one tensor.  Decoupled weight decay, bias-corrected moments, exactly torch.optim.AdamW
 * (amsgrad off): p *= 1 - lr*wd; m = b1 m + (1-b1) g; v = b2 v + (1-b2) g^2; p -= lr/(1-b1^t) * m / (sqrt(v)/sqrt(1-b2^t) + eps). */
#define CFFM_ADAMW_CHUNK 2048
/* Every parameter group of the optimizer in ONE launch (the reference's paramwise_cfg -- `head` lr_mult 10, `norm` /
 * `pos_block` decay_mult 0: local_configs/cffm/B1/cffm.b1.480x480.vspw2.160k.py:35-39 -- makes several): a chunk names the
 * ROW of the hyper-parameter tables it is updated with.  Device tables, `nrows` rows each:
 *   consts [nrows][12] double: beta1, beta2, eps, schedule kind, max_iters, power, min_lr, warmup_iters, warmup_ratio, first
 *                              iteration, GLOBAL iteration (slot 10: how many steps the optimizer has taken -- the call ADVANCES it
 *                              for every row, whether or not the row owns a chunk), (1 unused).  kind 0: lr_t = sched's lr.  kind 1:
 *                              the reference's schedule evaluated ON THE DEVICE (mmcv poly decay + linear warm-up,
 *                              cffm.b1...160k.py:41-45) from the global iteration, as mmcv derives every group's rate from the
 *                              runner's iteration: it = global - first; lr_t = (lr - min_lr) (1 - it/max_iters)^power + min_lr,
 *                              times 1 - (1 - it/warmup_iters)(1 - warmup_ratio) while it < warmup_iters; 0 for it < 0
 *   sched  [nrows][2] float : (base) lr, weight_decay                -- refreshed by the caller; vss_cffm_amd.optim copies it
 *                              from a pinned host mirror INSIDE the captured step, so graph replays see the current values
 *                              (the caller must order mirror writes against replays in flight; kind 1 needs no writes)
 *   state  [nrows][4] float : t, lr_t/(1-b1^t), 1/sqrt(1-b2^t), 1-lr_t*wd -- t advanced by the call (zero-initialise, or seed
 *                              with the step count of a resumed run)
 * grad_base != NULL: every chunk's `g` is a byte offset from grad_base instead of a pointer (all the gradients of the layer live in one
 * buffer; its address may change between steps, the table does not). */
#define CFFM_ADAMW_TICKETS 65
typedef struct {
    float* p;
    const float* g;
    float* m;
    float* v;
    int n;              /* 1..CFFM_ADAMW_CHUNK elements */
    int row;            /* row of consts / sched / state */
} cffm_adamw_chunk2;
/* active_rows (device, [nrows] ints, or NULL = every row): only rows that own a chunk of this call advance their step count.
 * ticket (device int[CFFM_ADAMW_TICKETS], zero before the first call, or NULL): with tickets the step count is advanced INSIDE the update
 * launch (one kernel; the workgroup that finishes last stores the new state) -- same results as the two-launch form used without.
 * The one-launch kernel keeps every row's factors in LDS: with more than 64 rows the call takes the two launches, tickets or not.
 * sched is read by the device when the launch runs: it may be device memory or pinned, device-visible host memory. */
int cffm_adamw_step_rows(const cffm_adamw_chunk2* chunks /* device */, int nchunks, const float* grad_base, float* state,
                         const float* sched, double* consts, int nrows, const int* active_rows, int* ticket, void* stream);

/* ---- ABI 13: k-means on token rows (the prototype-generating stage of CFFM++, cffm_head.py:280-282) ----
 * Lloyd's algorithm, euclidean, `iters` iterations, on x [N,256] for 1 <= K <= 128 centres, N >= K:
 *   assign  label_i = argmin_j (|c_j|^2 - 2 x_i.c_j) on the matrix pipe (three-pass bf16 hi / lo split); bit-equal scores go to the
 *           lowest centre index;
 *   update  c_j = mean of the points labelled j (fixed summation order: the same bits on every run); a centre that attracted no
 *           point keeps its value.
 * centers_inout [K,256] holds the initial centres on entry and the result on return.  labels_out [N] / counts_out [K] (int32, either
 * may be NULL) are those of the LAST ASSIGNMENT MADE, i.e. against the centres that entered the last iteration.
 * workspace: cffm_kmeans_workspace_bytes(N, K) bytes (-1 for bad sizes), written before it is read.  All iterations are enqueued on
 * `stream` by the one call (2 * iters + 1 kernels, no host round trip, no allocation): it can be captured into a HIP graph.
 * x, centers_inout and workspace must be 16-byte aligned.  K < 1, K > 128, N < K, iters < 1 are errors. */
long cffm_kmeans_workspace_bytes(long N, int K);
int cffm_kmeans(const float* x, long N, int K, int iters, float* centers_inout, int* labels_out, int* counts_out, void* workspace,
                void* stream);

/* ---- added under ABI 13, additive (no existing declaration changes, so the version stays 13): prediction ----
 * What EncoderDecoder_clips does between the head's eval forward and the metrics (segmentors/encoder_decoder.py:367-378 encode_decode's
 * resize to the input size, :502-516 whole_inference's resize to ori_shape, :542 softmax, :543-550 flip, :564 argmax) in ONE launch:
 *   pred[M][H][W] (int64) = argmax_k of the logits [.,K,h,w] resized bilinearly (align_corners=False) to (Hm,Wm) and then to (H,W); the
 *   resized logits exist only in registers.  The arg-max is taken over the interpolated logits (no exponential); equal values go to the
 *   lowest class index, as in torch.argmax.  When (Hm,Wm) == (H,W) the second stage is the identity.
 *   probs[M][K][H][W] (fp32, or NULL): the softmax over K of the same interpolated logits, written (accumulate = 0) or added
 *   (accumulate != 0: the in-place sum over augmentations of aug_test, :582-586).  probs == NULL selects a kernel without exponentials;
 *   pred may be NULL only when probs is given.
 * flip: 0 none, 1 horizontal, 2 vertical -- the OUTPUT is flipped: pixel (y, x) of pred / probs is what the unflipped call has at
 * (y, W-1-x) / (H-1-y, x).
 * The logits are addressed as in cffm_upce_maps_fwd: element (m, k, r, c) at (m / inner) * ms_outer + (m % inner) * ms_inner + k * ks +
 * (r * w + c) * ps with one of ks, ps equal to 1 -- plain [M,K,h,w], the heads' token rows [.., h, w, K], several maps of a clip buffer.
 * 1 <= K <= 256; Hm / h and Wm / w in 1..8; H / Hm and W / Wm in 0.5..2 (per axis, integer or not); anything else is an error and
 * enqueues nothing.  No workspace, no allocation, no host round trip: the call can be captured into a HIP graph. */
int cffm_predict(const float* logits, long long* pred, float* probs, int accumulate, int M, int K, int h, int w, int Hm, int Wm, int H,
                 int W, int flip, int inner, long ms_outer, long ms_inner, int ks, int ps, void* stream);

/* ---- added under ABI 13, additive: the middle of MiT's Mix-FFN (backbones/mix_transformer.py:48-55, 358-369) on token rows ----
 * h [M][H*W][C] (M images, row-major pixels, channel fastest), w [C][1][3][3], b [C]; zero padding outside each image:
 *   u[m,y,x,c] = b[c] + sum_{i,j in 0..2} w[c,i,j] h[m, y+i-1, x+j-1, c],     out = u Phi(u)   (the exact-erf GELU)
 * in one pass: the NCHW view, the depthwise Conv2d, the transpose back and the GELU of the reference never exist as tensors, and u is
 * not stored.  The backward recomputes u from h; with g = dout gelu'(u):
 *   dh[m,y,x,c] = sum_{i,j} w[c,i,j] g[m, y-i+1, x-j+1, c],   dw[c,i,j] = sum_{m,y,x} g[m,y,x,c] h[m, y+i-1, x+j-1, c],   db[c] = sum g
 * dw / db are summed in a fixed order (no atomics): the same bits run after run.  workspace: cffm_dwconv_gelu_bwd_workspace_bytes
 * bytes (-1 for bad sizes), 16-byte aligned; every byte that is read is written by the same call.
 * Errors (nothing is enqueued, the outputs stay as they are): C < 4, C % 4 != 0, M / H / W < 1, M*H*W*C >= 2^31, a null pointer or
 * one that is not 16-byte aligned.  No allocation, no host round trip: the calls can be captured into a HIP graph. */
int cffm_dwconv_gelu_fwd(const float* h, const float* w, const float* b, float* out, int M, int H, int W, int C, void* stream);
long cffm_dwconv_gelu_bwd_workspace_bytes(int M, int H, int W, int C);
int cffm_dwconv_gelu_bwd(const float* h, const float* w, const float* b, const float* dout, float* dh, float* dw, float* db,
                         void* workspace, int M, int H, int W, int C, void* stream);

/* ---- added under ABI 13, additive: the core of MiT's spatial-reduction attention (backbones/mix_transformer.py Attention.forward) ----
 * Soft-max attention of N query rows against Nk key rows per (image, head), fp32, in the layouts the module's Linear layers produce:
 *   q   [B][N][C]     C = heads * hd, head h = columns h*hd .. h*hd+hd-1                        (the output of self.q)
 *   kv  [B][Nk][2C]   K of head h = columns h*hd .., V of head h = columns C + h*hd ..         (the output of self.kv)
 *   out [B][N][C]     out[b,n,h*hd+c] = sum_k softmax_k(scale q_h[n] . k_h[k]) v_h[k][c]         (the reference's transpose(1,2).reshape)
 *   lse [B][heads][N] scale max_k(q.k) + log sum_k exp(scale (q.k - max)); NULL in cffm_sra_attn_fwd = not wanted (inference)
 * The score tensor never exists: keys are walked in tiles with an online soft-max, every product is the f32-input MFMA (fp32 operands, a
 * k-ordered fp32 fmaf chain).  The backward recomputes the probabilities from q, kv and lse; dq [B][N][C] and both halves of dkv
 * [B][Nk][2C] are written completely (the caller need not clear them); the dk / dv sums over the queries are partial slabs added in a
 * fixed order (no atomics): the same bits run after run.  workspace: cffm_sra_attn_bwd_workspace_bytes bytes (< 0 for bad sizes),
 * 16-byte aligned; every byte that is read is written by the same call.
 * Limits: hd 32 or 64; B, N, Nk, heads >= 1 (no cap on Nk); B*heads <= 65535; B*N*C and B*Nk*2C below 2^31; scale positive and finite.
 * Errors (nothing is enqueued, the outputs stay as they are): any of these limits, a null pointer (lse of the forward excepted) or one
 * that is not 16-byte aligned.  No allocation, no host round trip: the calls can be captured into a HIP graph. */
int cffm_sra_attn_fwd(const float* q, const float* kv, float* out, float* lse /* may be NULL: inference */,
                      int B, int N, int Nk, int heads, int hd, float scale, void* stream);
long cffm_sra_attn_bwd_workspace_bytes(int B, int N, int Nk, int heads, int hd);
int cffm_sra_attn_bwd(const float* q, const float* kv, const float* out, const float* lse, const float* dout,
                      float* dq, float* dkv, void* workspace, int B, int N, int Nk, int heads, int hd, float scale, void* stream);

/* ---- added under ABI 13, additive: the spatial-reduction Conv2d + LayerNorm of MiT's Attention (sr_ratio > 1) on token rows ----
 * What `self.norm(self.sr(x.permute(0, 2, 1).reshape(B, C, H, W)).reshape(B, C, -1).permute(0, 2, 1))` computes, as one GEMM with a
 * LayerNorm epilogue (kernel = stride: the windows do not overlap):
 *   x, dx    [B][H*W][C]       token rows (row-major pixels, channel fastest)
 *   w, dw    [C][C][s][s]      the Conv2d's own weight layout (co, ci, ky, kx); b, db [C]; gamma, beta, dgamma, dbeta [C] (the LayerNorm)
 *   Ho = H / s, Wo = W / s (rounded down), M = B*Ho*Wo
 *   z        [M][C]            z[(b,oy,ox), co] = b[co] + sum_{ky,kx,ci} w[co,ci,ky,kx] x[b, (oy*s+ky)*W + ox*s+kx, ci]
 *   stats    [M][2]            mean and rstd = 1 / sqrt(var + eps) of each row of z (variance of the centred values, biased)
 *   out      [M][C]            (z - mean) * rstd * gamma + beta
 * z and stats are outputs of the forward kept for the backward; both NULL = not wanted (inference).  Pixel rows >= Ho*s and columns >=
 * Wo*s are never read; their dx is written as zero, so dx, dw, db, dgamma and dbeta are written completely (the caller need not clear
 * them).  Every product is the f32-input MFMA (fp32 operands, an fp32 fmaf chain); all sums are taken in a fixed order (no atomics):
 * the same bits run after run.  workspace: cffm_sr_ln_bwd_workspace_bytes bytes (< 0 for bad sizes), 16-byte aligned; every byte that
 * is read is written by the same call.
 * Limits: s 2, 4 or 8; C a multiple of 16 in 16..512; B >= 1, H >= s, W >= s; B*H*W*C below 2^31; eps finite and >= 0.
 * Errors (nothing is enqueued, the outputs stay as they are): any of these limits, a null pointer (z and stats of the forward excepted,
 * together), only one of z and stats, or a pointer that is not 16-byte aligned.  No allocation, no host round trip: the calls can be
 * captured into a HIP graph. */
int cffm_sr_ln_fwd(const float* x, const float* w, const float* b, const float* gamma, const float* beta, float* out,
                   float* z /* may be NULL */, float* stats /* NULL with z */, int B, int H, int W, int C, int s, float eps, void* stream);
long cffm_sr_ln_bwd_workspace_bytes(int B, int H, int W, int C, int s);
int cffm_sr_ln_bwd(const float* x, const float* w, const float* gamma, const float* z, const float* stats, const float* dout, float* dx,
                   float* dw, float* db, float* dgamma, float* dbeta, void* workspace, int B, int H, int W, int C, int s, float eps,
                   void* stream);

/* ---- added under ABI 13, additive: LayerNorm of token rows at any width, and one MiT stage's inference forward per call ----
 * LayerNorm over the C channels of fp32 token rows, C a multiple of 4 in 16..512 (csrc/mitln_kernels.h): a row is held in registers, the
 * mean is taken first and the variance from the centred values, rstd = 1 / sqrt(var + eps); fixed summation order, no atomics: the same
 * bits run after run.  The forwards save nothing; the backwards below recompute mean and rstd from the input.
 *   cffm_ln_rows       out[M][C] = LN(x[M][C])
 *   cffm_nchw_ln_rows   x_nchw [B][C][H][W] -> out_rows [B][H*W][C], normalised: OverlapPatchEmbed's flatten(2).transpose(1, 2) + norm
 *   cffm_ln_rows_nchw   x_rows [B][H*W][C] -> out_nchw [B][C][H][W], normalised: a stage's norm + reshape(B, H, W, C).permute(0, 3, 1, 2)
 * Errors (nothing is enqueued, the outputs stay as they are): C outside the limits, M / B / H / W < 1, M*C or B*C*H*W >= 2^31, eps
 * negative or not finite, a null pointer or one that is not 16-byte aligned.  No workspace, no allocation, no host round trip. */
int cffm_ln_rows(const float* x, const float* gamma, const float* beta, float* out, long M, int C, float eps, void* stream);
int cffm_nchw_ln_rows(const float* x_nchw, const float* gamma, const float* beta, float* out_rows, int B, int C, int H, int W, float eps,
                      void* stream);
int cffm_ln_rows_nchw(const float* x_rows, const float* gamma, const float* beta, float* out_nchw, int B, int C, int H, int W, float eps,
                      void* stream);

/* added under ABI 13, additive: the backwards of the three calls above.  x is the forward's input in the forward's layout, dout the gradient
 * of its output in the output's layout, dx the gradient of x in x's layout; dgamma [C], dbeta [C].  Nothing was saved: mean and rstd are
 * recomputed from x with the forward's arithmetic (xhat has the forward's bits);  g = gamma * dout,  dx = rstd * (g - mean(g) - xhat *
 * mean(g * xhat)),  dgamma = sum over rows of dout * xhat,  dbeta = sum over rows of dout.  dgamma / dbeta are summed without atomics: every
 * workgroup writes one record [2][C] to the workspace and a second kernel adds the records; how many there are and the order they are added
 * in depend on (M, C, H*W) only, never on the device: the same bits run after run.  workspace: cffm_ln_bwd_workspace_bytes(M, C, HW) bytes,
 * 16-byte aligned, need not be initialised; M = B*H*W and HW = H*W for the two map calls, HW = 1 for cffm_ln_rows_bwd (a map of one pixel
 * per image is a set of rows and runs as such); < 0 when C is outside the limits, M < 1, HW < 1, M is no multiple of HW or M*C >= 2^31.
 * Limits and errors as the forwards (nothing is enqueued, every output stays as it is).  No allocation, no host round trip. */
long cffm_ln_bwd_workspace_bytes(long M, int C, int HW);
int cffm_ln_rows_bwd(const float* x, const float* gamma, const float* dout, float* dx, float* dgamma, float* dbeta, void* ws, long M, int C,
                     float eps, void* stream);
int cffm_nchw_ln_rows_bwd(const float* x_nchw, const float* gamma, const float* dout_rows, float* dx_nchw, float* dgamma, float* dbeta, void* ws,
                          int B, int C, int H, int W, float eps, void* stream);
int cffm_ln_rows_nchw_bwd(const float* x_rows, const float* gamma, const float* dout_nchw, float* dx_rows, float* dgamma, float* dbeta, void* ws,
                          int B, int C, int H, int W, float eps, void* stream);

/* One stage of a Mix Transformer (backbones/mix_transformer.py forward_features, one iteration of its loop) in eval mode, behind the
 * patch embedding's convolution: conv_nchw [B,C,H,W] (patch_embed.proj's output) -> out_nchw [B,C,H,W] (what the stage hands to the head):
 *   cffm_nchw_ln_rows (patch_embed.norm);
 *   per block: LN (norm1) | q GEMM | sr conv + LN (sr_ratio > 1: cffm_sr_ln_fwd's kernel) | kv GEMM | attention (cffm_sra_attn_fwd's
 *     kernel, no lse) | proj GEMM + bias + residual | LN (norm2) | fc1 GEMM | depthwise 3x3 + GELU (cffm_dwconv_gelu_fwd's kernel) |
 *     fc2 GEMM + bias + residual;
 *   cffm_ln_rows_nchw (norm_i).
 * The Linear layers are the library's three-pass bf16-split GEMMs (fp32 operands split into bf16 hi + lo, fp32 accumulation).
 * Device pointers, each tensor in the nn.Module's own layout (Linear [out][in], sr [C][C][s][s], dwconv [hidden][1][3][3]); q_b / kv_b
 * may be NULL (qkv_bias=False); sr_w / sr_b / srn_g / srn_b are NULL if and only if sr_ratio == 1.  No prepared copies are made or kept.
 * Everything is enqueued on `stream` alone: no side streams, no allocation, no host synchronisation -- the call can be captured into a
 * HIP graph as a single chain.  ws: cffm_mit_stage_infer_ws_floats(cfg) floats (it depends on the cfg, not on depth), 16-byte aligned;
 * every byte of it that is read is written by the same call.
 * Limits: head size C / heads 32 or 64; C a multiple of 16 in 16..512; hidden a multiple of 4; sr_ratio 1, 2, 4 or 8 and H, W >= sr_ratio;
 * B*heads <= 65535; B*H*W*max(2C, hidden) below 2^30 (the GEMMs address an operand with 32-bit byte offsets); scale positive and finite;
 * every eps finite and >= 0.  Errors (nothing is enqueued, the output stays as it is; cffm_mit_stage_infer_ws_floats returns < 0): any of
 * these limits, a null pointer where one is required, a pointer that is not 16-byte aligned, conv_nchw == out_nchw. */
typedef struct {
    const float *n1_g, *n1_b, *q_w, *q_b, *kv_w, *kv_b, *sr_w, *sr_b, *srn_g, *srn_b, *proj_w, *proj_b,
                *n2_g, *n2_b, *fc1_w, *fc1_b, *dw_w, *dw_b, *fc2_w, *fc2_b;
} cffm_mit_block_params;
typedef struct {
    int B, H, W, C, heads, hidden, sr_ratio, depth;
    float scale;                                    /* the attention's q.k scale */
    float eps_embed, eps_block, eps_sr, eps_out;    /* patch_embed.norm | norm1 and norm2 of every block | attn.norm | norm_i */
} cffm_mit_stage_cfg;
long cffm_mit_stage_infer_ws_floats(const cffm_mit_stage_cfg* c);          /* < 0: unsupported sizes */
int cffm_mit_stage_infer(const cffm_mit_stage_cfg* c, const cffm_mit_block_params* blocks /* host [depth] */,
                         const float* embed_g, const float* embed_b, const float* out_g, const float* out_b,
                         const float* conv_nchw /* [B,C,H,W]: patch_embed.proj's output */, float* out_nchw /* [B,C,H,W] */,
                         float* ws, void* stream);

/* ---- added under ABI 13, additive: MiT's overlapping patch embedding as a kernel, and n consecutive stages per call ----
 * OverlapPatchEmbed.forward in eval mode (csrc/pembed_kernels.h): Conv2d(Cin, Cout, k, stride, padding = k / 2) on x_nchw [B][Cin][H][W],
 * flatten(2).transpose(1, 2), LayerNorm(Cout) -> out_rows [B][Ho*Wo][Cout], Ho = (H + 2 (k / 2) - k) / stride + 1 and Wo likewise.  A GEMM
 * on gathered patches: the input and the weight [Cout][Cin][k][k] are read where they lie (no im2col buffer, no repacked weight, no NCHW
 * copy of the result), taps outside the image contribute exactly zero.  Products: the three-pass bf16 split of the Linear GEMMs (fp32
 * operands split into bf16 hi + lo, hi.lo + lo.hi + hi.hi, fp32 accumulation); LayerNorm as cffm_ln_rows.  Fixed summation order, no
 * atomics: the same bits on every call.  No workspace, no allocation, no host round trip.
 * Limits: (k, stride) = (7, 4) or (3, 2); Cin in 1..4 for k = 7, a multiple of 4 in 4..512 for k = 3; Cout a multiple of 16 in 16..512;
 * B, H, W >= 1; B*Cin*H*W and B*Ho*Wo*Cout below 2^31; eps finite and >= 0; pointers non-null and 16-byte aligned.  Errors enqueue
 * nothing and leave the output as it is. */
int cffm_patch_embed_fwd(const float* x_nchw, const float* w, const float* b, const float* gamma, const float* beta, float* out_rows, int B,
                         int Cin, int H, int W, int Cout, int k, int stride, float eps, void* stream);

/* added under ABI 13, additive: the patch embedding for a training pass (csrc/pembed_kernels.h, second half).
 *   cffm_patch_embed_fwd_train   cffm_patch_embed_fwd that also stores z_rows [B][Ho*Wo][Cout], the pre-LayerNorm rows (convolution + bias:
 *                                the values the LayerNorm epilogue reads); out_rows has the bits of cffm_patch_embed_fwd.
 *   cffm_patch_embed_bwd         dout_rows [B][Ho*Wo][Cout] -> dgamma, dbeta [Cout] and dz (cffm_ln_rows_bwd's kernels on z_rows: mean and rstd
 *                                recomputed), then dw [Cout][Cin][k][k] = sum over the output pixels of dz x patch and db [Cout] = sum of dz,
 *                                and -- (k, stride) = (3, 2) and dx_nchw non-null -- dx_nchw [B][Cin][H][W] = the taps of dz that reach each
 *                                input pixel, times w (a pixel no tap reaches: exact zero).  dx_nchw == NULL skips the input gradient; with
 *                                (7, 4) a non-null dx_nchw is refused.
 * Products in dw and dx: the forward's three-pass bf16 split, fp32 accumulation; db, dgamma, dbeta: fp32 sums.  No atomics: the contraction
 * over the output pixels is split into slabs whose count and order follow from the shapes alone, a second kernel adds them in slab order:
 * the same bits on every call, on any device.  workspace: cffm_patch_embed_bwd_workspace_bytes(..., with_dx) bytes (with_dx = whether
 * dx_nchw will be non-null), 16-byte aligned, need not be initialised: every byte that is read is written by the same call; dz lives there.
 * Limits as cffm_patch_embed_fwd.  Errors (nothing is enqueued, every output stays as it is; the workspace query returns < 0): these limits,
 * a null pointer (dx_nchw excepted) or one that is not 16-byte aligned, (7, 4) with dx.  No allocation, no host round trip, everything on
 * `stream` alone. */
int cffm_patch_embed_fwd_train(const float* x_nchw, const float* w, const float* b, const float* gamma, const float* beta, float* out_rows,
                               float* z_rows, int B, int Cin, int H, int W, int Cout, int k, int stride, float eps, void* stream);
long cffm_patch_embed_bwd_workspace_bytes(int B, int Cin, int H, int W, int Cout, int k, int stride, int with_dx);   /* < 0: refused */
int cffm_patch_embed_bwd(const float* x_nchw, const float* w, const float* gamma, const float* z_rows, const float* dout_rows,
                         float* dx_nchw /* may be NULL */, float* dw, float* db, float* dgamma, float* dbeta, void* workspace, int B, int Cin,
                         int H, int W, int Cout, int k, int stride, float eps, void* stream);

/* ---- added under ABI 13, additive: one Linear layer on token rows, forward and backward, with a residual and a per-sample factor ----
 * What a MiT block's q / kv / fc1 (no residual, no factor) and proj / fc2 (residual = the block input, factor = the DropPath mask / keep)
 * compute in a training pass (csrc/gemm_kernels.h, host side csrc/gemm.h).  x [M][K], w [N][K] (nn.Linear's own layout), b [N] or NULL,
 * residual [M][N] or NULL, scale [B] or NULL with M = B * rows_per_sample; row m belongs to sample m / rows_per_sample.
 *   cffm_linear_rows_fwd   y[m] = residual[m] + scale[m / rps] * (x[m] w^T + b); a NULL b, residual or scale drops its term.  A sample
 *                          whose scale is 0 gets the bits of residual (zeros without one), for finite operands.  Nothing is saved.
 *   cffm_linear_rows_bwd   with g[m] = scale[m / rps] * dy[m], which is never written to memory:  dx [M][K] = g w (the factor applied to
 *                          the finished rows; dx == NULL skips it; rows of a sample whose scale is 0 are exact zeros);  dw [N][K] = g^T x
 *                          (the factor applied to the dy tile while it is staged);  db [N] = the column sum of g in fp32 (NULL skips it).
 *                          The gradient of residual is dy itself: the caller passes it on, nothing is copied.
 * Products: the three-pass bf16 split of the other Linear GEMMs (fp32 operands split into bf16 hi + lo, hi.lo + lo.hi + hi.hi, fp32
 * accumulation).  No atomics: dw's contraction over the M rows is split into slabs and db into records whose count and order follow from
 * (M, N, K) alone, a second kernel adds them in that order: the same bits on every call.  workspace:
 * cffm_linear_rows_bwd_workspace_bytes(...) bytes, 16-byte aligned, need not be initialised; it holds the dw slabs [ksplit][N][K] and the db
 * records only (never an [M][N] temporary) and may be 0 bytes, in which case NULL is accepted; with_dx is taken for symmetry and changes
 * nothing (dx needs no workspace), with_db = whether db will be non-null.
 * Limits: M >= 1; N and K multiples of 4 (not 16 as in cffm_mit_stage_infer: the tile loads read 16-byte pieces and nothing else here asks
 * for more; hidden sizes such as 20 C stay inside); M a multiple of rows_per_sample >= 1; M*max(N, K) and N*K below 2^30 (an operand is
 * addressed with 32-bit byte offsets).  Errors (nothing is enqueued, every output stays as it is, cffm_last_error is set; the workspace
 * query returns < 0): these limits; a NULL x / w / y / dy / dw, or a NULL workspace of non-zero size; a pointer that is not 16-byte
 * aligned (scale: 4-byte); y equal to any input pointer -- x, w, b, residual, scale: there is no in-place form, y == residual included;
 * dx / dw / db equal to dy, x, w or scale, to each other or to the workspace (only equal pointers are looked for, not overlapping ranges).
 * All of these, and the grant of the kernels' LDS, are settled before the first launch.  The one error that can follow a launch is the
 * runtime refusing it (code -2): what was enqueued before it then stays enqueued.  Everything is enqueued on `stream` alone: no allocation,
 * no host round trip, so the calls can be captured into a graph.  dw cannot be skipped (dx and db can): a layer with a frozen weight still
 * has it formed. */
int cffm_linear_rows_fwd(const float* x, const float* w, const float* b /* NULL ok */, const float* residual /* NULL ok */,
                         const float* scale /* NULL ok */, float* y, long M, int N, int K, int rows_per_sample, void* stream);
long cffm_linear_rows_bwd_workspace_bytes(long M, int N, int K, int rows_per_sample, int with_dx, int with_db);   /* < 0: refused */
int cffm_linear_rows_bwd(const float* dy, const float* x, const float* w, const float* scale /* NULL ok */, float* dx /* NULL ok */,
                         float* dw, float* db /* NULL ok */, void* workspace, long M, int N, int K, int rows_per_sample, void* stream);

/* n = 1..4 consecutive MiT stages, each WITH its patch embedding, as one call: per stage cffm_patch_embed_fwd's kernel writes the
 * normalised rows straight into the stage's residual buffer (cffm_nchw_ln_rows does not run), then the blocks and cffm_ln_rows_nchw exactly as
 * cffm_mit_stage_infer enqueues them.  x_nchw [B, stages[0].Cin, Hin, Win] is stage 0's input, outs[i] (host array of n device pointers)
 * receives stage i's map [B, cfg.C, cfg.H, cfg.W] and is stage i + 1's input.  Everything is enqueued on `stream` alone: one chain in a
 * captured graph.  ws: cffm_mit_infer_ws_floats(stages, n) floats = the MAXIMUM over the stages of cffm_mit_stage_infer_ws_floats (the
 * stages run one after another), 16-byte aligned; every byte of it that is read is written by the same call.
 * Errors (nothing is enqueued; cffm_mit_infer_ws_floats returns < 0): n outside 1..4, anything cffm_patch_embed_fwd or cffm_mit_stage_infer
 * refuses, a cfg whose (H, W, C) is not the convolution's output shape, a stage whose input is not the previous stage's output,
 * outputs that alias each other or the input. */
typedef struct {
    cffm_mit_stage_cfg cfg;                         /* C = the convolution's Cout, (H, W) = its output size */
    int Cin, Hin, Win, k, stride;                   /* patch_embed.proj: its input map and (kernel, stride) */
    const float *conv_w, *conv_b;                   /* patch_embed.proj weight [C][Cin][k][k] and bias [C] */
    const float *embed_g, *embed_b, *out_g, *out_b; /* patch_embed.norm and norm_i */
    const cffm_mit_block_params* blocks;            /* host [cfg.depth] */
} cffm_mit_stage;
long cffm_mit_infer_ws_floats(const cffm_mit_stage* stages /* host [n] */, int n);          /* < 0: refused */
int cffm_mit_infer(const cffm_mit_stage* stages /* host [n] */, int n, const float* x_nchw, float* const* outs /* host [n] */, float* ws,
                   void* stream);

/* ---- added under ABI 13, additive: LayerNorm backward of token rows with the neighbouring adds fused in (csrc/mitln_kernels.h) ----
 *   d  = dout_a + dout_b            one rounded fp32 add per element; dout_b == NULL: d = dout_a
 *   v  = LN-backward(x, gamma, d)   cffm_ln_rows_bwd's arithmetic, to the bit
 *   dx = dres + v                   one fp32 add rounded on its own, never fused with the multiply that makes v; dres == NULL: dx = v
 * dgamma / dbeta are those of d.  The result has the bits of cffm_ln_rows_bwd(x, gamma, dout_a + dout_b) followed by dres + dx with the two
 * adds done as separate fp32 passes, and with dout_b == dres == NULL the bits of cffm_ln_rows_bwd itself.  These are the two passes
 * autograd adds around a MiT block's LayerNorms: d(norm1 out) = dx_q + dx_sr and dx1 = dy + LN2-backward.  dx == dres (in place) is allowed: a
 * lane reads its own elements before it writes them; dx equal to x, dout_a or dout_b is refused.  ws: cffm_ln_bwd_workspace_bytes(M, C, 1).
 * Limits and errors as cffm_ln_rows_bwd (nothing is enqueued, every output stays as it is); dout_b / dres 16-byte aligned or NULL. */
int cffm_ln_rows_bwd_add(const float* x, const float* gamma, const float* dout_a, const float* dout_b /* NULL ok */,
                         const float* dres /* NULL ok */, float* dx, float* dgamma, float* dbeta, void* ws, long M, int C, float eps,
                         void* stream);

/* ---- added under ABI 13, additive: the blocks of one MiT stage in a training pass, one call per direction ----
 * x_rows [B][H*W][C] (what the patch embedding hands to the first block) -> y_rows (what the last block hands to the stage's norm), and
 * back.  The patch embedding and the stage's norm are not part of the calls.  cffm_mit_stage_cfg is reused: B, H, W, C, heads, hidden,
 * sr_ratio, depth, scale, eps_block and eps_sr are read, eps_embed / eps_out are not.  scales: host [depth] or NULL (no factor anywhere);
 * each factor [B] or NULL: what DropPath multiplies a sample's attention / Mix-FFN branch with (0 or 1 / keep).
 *   forward, per block    LN (norm1) | q | sr conv + LN (sr_ratio > 1, rows before the LN and their stats kept) | kv | attention (lse kept) |
 *                         proj + bias + residual, scale_attn | LN (norm2) | fc1 | depthwise 3x3 + GELU | fc2 + bias + residual, scale_mlp.
 *                         The kernels, launch plans and bits of cffm_ln_rows, cffm_linear_rows_fwd, cffm_sr_ln_fwd, cffm_sra_attn_fwd and
 *                         cffm_dwconv_gelu_fwd chained in that order.
 *   saved, per block      z1 | q | (sr_ratio > 1: sr rows before the LN | their stats | r) | kv | attention output | lse | x1 | z2 | h | a |
 *                         the block's output (every block but the last), each carve 256-byte aligned.  Nothing is recomputed in the backward
 *                         beyond what the single kernels already recompute.
 *   backward, g = the gradient of a block's output, blocks in reverse
 *                         fc2 (dw, db from scale_mlp g and a; da) | dwconv + GELU backward (dh, ddw, ddb) | fc1 (dw, db; dz2) |
 *                         g1 = g + LN2-backward(x1, dz2) (cffm_ln_rows_bwd_add's kernel) | proj (dw, db from scale_attn g1 and ao; dao) |
 *                         attention backward (dq, dkv) | kv (dw, db; dr) | sr backward (sr_ratio > 1: dz1b and the four sr gradients; else
 *                         dz1b = dr) | q (dw, db; dz1a) | g' = g1 + LN1-backward(x, dz1a + dz1b): the previous block's g, dx_rows for block 0.
 *                         Every gradient has the bits the single calls give when autograd chains them.
 * grads: host [depth], the fields of cffm_mit_block_params as writable pointers, non-null exactly where the parameter is non-null; every
 * gradient is formed (written, not accumulated).  ws: cffm_mit_blocks_train_bwd_ws_floats(cfg) floats for the backward -- the running
 * gradients, the temporaries of one block, and ONE set of dw slabs / db records / LayerNorm records / attention, sr and dwconv workspaces,
 * each the maximum over the call's uses; the forward keeps every intermediate in `saved` and needs no workspace
 * (cffm_mit_blocks_train_fwd_ws_floats returns 0 and ws may be NULL).  Every byte of saved and ws that is read is written by the same
 * forward + backward pair; neither needs initialising.  Everything is enqueued on `stream` alone: no allocation, no host round trip, no
 * atomics, so both calls can be captured into a HIP graph.
 * Limits: those of cffm_mit_stage_infer.  Errors (every check is settled before the first launch: nothing is enqueued, every output stays
 * as it is; the three size queries return < 0): those limits, a null pointer where one is required, sr pointers at sr_ratio 1, a pointer
 * that is not 16-byte aligned (a factor: 4-byte), a gradient pointer that is null where the parameter is not or the reverse, and any two of
 * x_rows / y_rows / saved / ws (forward) or x_rows / saved / dy_rows / dx_rows / ws (backward) being equal. */
typedef struct {
    float *n1_g, *n1_b, *q_w, *q_b, *kv_w, *kv_b, *sr_w, *sr_b, *srn_g, *srn_b, *proj_w, *proj_b,
          *n2_g, *n2_b, *fc1_w, *fc1_b, *dw_w, *dw_b, *fc2_w, *fc2_b;
} cffm_mit_block_grad_ptrs;
typedef struct { const float *scale_attn, *scale_mlp; } cffm_mit_block_scales;      /* [B] each, NULL = no DropPath factor */
long cffm_mit_blocks_train_saved_floats(const cffm_mit_stage_cfg* c);      /* the whole call: depth blocks; < 0: refused */
long cffm_mit_blocks_train_fwd_ws_floats(const cffm_mit_stage_cfg* c);
long cffm_mit_blocks_train_bwd_ws_floats(const cffm_mit_stage_cfg* c);
int cffm_mit_blocks_train_fwd(const cffm_mit_stage_cfg* c, const cffm_mit_block_params* blocks /* host [depth] */,
                              const cffm_mit_block_scales* scales /* host [depth], NULL = none anywhere */,
                              const float* x_rows /* [B][H*W][C] */, float* y_rows, float* saved, float* ws, void* stream);
int cffm_mit_blocks_train_bwd(const cffm_mit_stage_cfg* c, const cffm_mit_block_params* blocks, const cffm_mit_block_scales* scales,
                              const cffm_mit_block_grad_ptrs* grads /* host [depth] */, const float* x_rows, const float* saved,
                              const float* dy_rows, float* dx_rows, float* ws, void* stream);

#ifdef __cplusplus
}
#endif
#endif
