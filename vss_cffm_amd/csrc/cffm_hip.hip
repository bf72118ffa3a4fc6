// cffm_hip.hip -- C-ABI entry points of libcffm_hip.so (see include/cffm_hip.h) and the host-side
// orchestration of one CFFM block / layer on a HIP stream.  gfx950 only.
#include "cfm_attn_kernels.h"
#include "clip_kernels.h"
#include "rowops_kernels.h"
#include "gtc_kernels.h"
#include "gemm.h"
#include "segfuse_kernels.h"
#include "segloss_kernels.h"
#include "headfuse_kernels.h"
#include "kmeans_kernels.h"
#include "predict_kernels.h"
#include "mixffn_kernels.h"
#include "sra_kernels.h"
#include "srln_kernels.h"
#include "mitln_kernels.h"
#include "pembed_kernels.h"

#include <stdarg.h>
#include <stdio.h>

#include "../../include/cffm_hip.h"

static thread_local char g_err[512] = "";

static int fail(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}
#define CHECK_LAUNCH(name)                                                                        \
    do {                                                                                          \
        hipError_t e_ = hipGetLastError();                                                        \
        if (e_ != hipSuccess) return fail(-2, "%s: launch failed: %s", name, hipGetErrorString(e_)); \
    } while (0)
#define REQUIRE(cond, ...) \
    do { if (!(cond)) return fail(-1, __VA_ARGS__); } while (0)
#define TRY(call) \
    do { int rc_ = (call); if (rc_) return rc_; } while (0)

static Geo to_geo(const cffm_geom* g) {
    Geo G;
    G.B = g->B; G.H0 = g->H0; G.W0 = g->W0; G.Hp = g->Hp; G.Wp = g->Wp; G.gy = g->gy; G.gx = g->gx;
    G.nW = g->nW; G.HW = g->HW; G.RC = g->RC;
    return G;
}


// ------------------------------------------------------------------------------------------- stage timing
// Optional per-stage HIP-event timing on the caller's stream (bench.py's live `roofline` numbers):
// when enabled every stage-level entry point brackets its launches with two events.
enum { ST_TRANSPOSE, ST_POOLMAT, ST_LN_POOL_FWD, ST_LN_POOL_BWD, ST_BIAS_ASM, ST_BIAS_SCT, ST_ATTN_FWD, ST_ATTN_BWD,
       ST_GEMM, ST_COLSUM, ST_RES_LN, ST_LN_BWD, ST_GELU, ST_GELU_BWD, ST_RES_OUT, ST_GTC_FWD, ST_GTC_BWD, ST_LN, ST_ADAMW, ST_NULL_PAIR,
       // per-kernel-family stages of the block (bench.py's `roofline_kernels`); the ST_GEMM / ST_ATTN_BWD totals above stay
       ST_G_QKV_FWD, ST_G_PROJ_FWD, ST_G_FC1_FWD, ST_G_FC2_FWD, ST_G_FC2_DX, ST_G_FC1_DX, ST_G_PROJ_DX, ST_G_QKV_DX, ST_G_DW,
       ST_ATTN_BWD_Q, ST_ATTN_BWD_KV, ST_DKV_GATHER, ST_MLP_FWD, ST_MLP_BWD, ST_LN_POOL_BWD_REF, ST_COUNT };
static const char* const k_stage_names[ST_COUNT] = {"transpose", "pool_matrix", "ln_pool_fwd", "ln_pool_bwd", "bias_assemble",
    "bias_scatter", "cfm_attn_fwd", "cfm_attn_bwd", "linear_gemm", "colsum", "residual_ln", "ln_bwd", "bias_gelu", "gelu_bwd",
    "residual_out", "gtc_attn_fwd", "gtc_attn_bwd", "layernorm", "adamw", "event_pair_null",
    "gemm_qkv_fwd", "gemm_proj_fwd", "gemm_fc1_fwd", "gemm_fc2_fwd", "gemm_fc2_dx_gelu", "gemm_fc1_dx", "gemm_proj_dx", "gemm_qkv_dx",
    "gemm_dw_group", "attn_bwd_fused", "attn_bwd_bias_sum", "attn_dkv_gather", "mlp_fwd_fused", "mlp_bwd_fused", "ln_pool_bwd_ref"};
#ifndef CFFM_EMU
#include <vector>
struct ProfRec { int stage; hipEvent_t e0, e1; };
static unsigned long long g_prof_mask = 0;   // bit i = time stage i
static std::vector<ProfRec> g_prof_recs;
static std::vector<hipEvent_t> g_prof_pool;
static hipEvent_t prof_event() {
    hipEvent_t e;
    if (!g_prof_pool.empty()) { e = g_prof_pool.back(); g_prof_pool.pop_back(); return e; }
    (void)hipEventCreate(&e);
    return e;
}
// Event pairs recorded while the stream was being captured into a HIP graph: they become event-record NODES of the graph,
// every replay re-records them, and they stay readable for the life of the graph.  The node is added explicitly
// (capture info -> hipGraphAddEventRecordNode -> new capture dependency): the HIP 7.0 runtime PyTorch bundles rejects
// hipEventRecordWithFlags(hipEventRecordExternal), the explicit form works on 7.0 and 7.2 (scripts/graph_bench_check.sh).
static std::vector<ProfRec> g_prof_graph_recs;
static bool g_prof_capture_failed = false;
static hipEvent_t prof_capture_event(hipStream_t st) {
    hipEvent_t ev = nullptr;
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    unsigned long long id = 0;
    hipGraph_t graph = nullptr;
    const hipGraphNode_t* deps = nullptr;
    size_t ndeps = 0;
    hipGraphNode_t node;
    bool ok = hipEventCreate(&ev) == hipSuccess
        && hipStreamGetCaptureInfo_v2(st, &cs, &id, &graph, &deps, &ndeps) == hipSuccess
        && hipGraphAddEventRecordNode(&node, graph, deps, ndeps, ev) == hipSuccess
        && hipStreamUpdateCaptureDependencies(st, &node, 1, hipStreamSetCaptureDependencies) == hipSuccess;
    if (!ok) { g_prof_capture_failed = true; (void)hipGetLastError(); }
    return ev;
}
static int g_prof_period = 1;
static unsigned g_prof_seen[ST_COUNT] = {};
struct ProfScope {
    int stage; hipStream_t st; hipEvent_t e0; bool on, cap;
    ProfScope(int s, void* stream) : stage(s), st((hipStream_t)stream), on((g_prof_mask >> s) & 1ull), cap(false) {
        if (on && g_prof_period > 1) on = (g_prof_seen[s]++ % g_prof_period) == 0;     // cffm_profile_sample_every
        if (!on) return;
        hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
        cap = hipStreamIsCapturing(st, &cs) == hipSuccess && cs == hipStreamCaptureStatusActive;
        if (cap) e0 = prof_capture_event(st);
        else { e0 = prof_event(); (void)hipEventRecord(e0, st); }
    }
    ~ProfScope() {
        if (!on) return;
        if (cap) {
            hipEvent_t e1 = prof_capture_event(st);
            g_prof_graph_recs.push_back({stage, e0, e1});
        } else {
            hipEvent_t e1 = prof_event(); (void)hipEventRecord(e1, st); g_prof_recs.push_back({stage, e0, e1});
        }
    }
};
#define PROF(stage) ProfScope prof_scope_(stage, stream)
#define PROF2(stage) ProfScope prof_scope2_(stage, stream)      // a second (inner / family) interval in the same scope
#else
#define PROF(stage) (void)0
#define PROF2(stage) (void)0
#endif

static bool g_side_off = false;     // cffm_side_streams(0): everything on the caller's stream (per-kernel timing passes)
extern "C" {
// mask: bit i enables stage i (cffm_profile_stage_name); 0 = off, -1 = every stage.  Each timed launch costs two event
// records on the stream (~2 us of GPU time), so timing every stage perturbs a ~1.5 ms step by ~25 %: bench.py times only
// the roofline kernel inside its timed region and takes the full breakdown in a separate pass.
int cffm_profile_enable(long long mask) {
#ifndef CFFM_EMU
    g_prof_mask = (unsigned long long)mask;
    for (int i = 0; i < ST_COUNT; ++i) g_prof_seen[i] = 0;
#endif
    return 0;
}
// time only every `period`-th launch of an enabled stage (counted from the next cffm_profile_enable): an event pair around a kernel
// of a captured step keeps its neighbours from being dispatched back to back (~10 us per pair on the chain of a replayed graph)
int cffm_profile_sample_every(int period) {
#ifndef CFFM_EMU
    g_prof_period = period > 1 ? period : 1;
#endif
    (void)period;
    return 0;
}
// an event pair with NOTHING between its two records (stage "event_pair_null"): what a timed interval costs by itself on this
// stream / in this graph -- bench.py reports it next to the roofline kernel's interval (22.6 us between events vs 19.7 us in
// rocprofv3's kernel trace; the empty pair measures 5-6 us, so it is not simply additive and is not subtracted)
int cffm_profile_null_pair(void* stream) {
    PROF(ST_NULL_PAIR);
    return 0;
}
// on = 0: the library's side streams are not used until switched on again -- every kernel of a block backward then runs on the caller's
// stream, one after the other (bench.py's per-kernel pass: an interval measured while another stream's GEMMs share the chip says
// little about the kernel).  Returns the previous setting.  Not to be changed while a stream is being captured.
int cffm_side_streams(int on) {
    const int was = g_side_off ? 0 : 1;
    g_side_off = on == 0;
    return was;
}
int cffm_profile_stage_count(void) { return ST_COUNT; }
const char* cffm_profile_stage_name(int i) { return (i >= 0 && i < ST_COUNT) ? k_stage_names[i] : ""; }
// sums the recorded intervals per stage (ms) and launch counts, then clears the records; synchronises.
int cffm_profile_collect(float* ms /*[count]*/, int* calls /*[count]*/) {
    for (int i = 0; i < ST_COUNT; ++i) { ms[i] = 0.f; calls[i] = 0; }
#ifndef CFFM_EMU
    for (auto& r : g_prof_recs) {
        float t = 0.f;
        (void)hipEventSynchronize(r.e1);
        (void)hipEventElapsedTime(&t, r.e0, r.e1);
        ms[r.stage] += t;
        calls[r.stage] += 1;
        g_prof_pool.push_back(r.e0);
        g_prof_pool.push_back(r.e1);
    }
    g_prof_recs.clear();
#endif
    return 0;
}
// the event pairs captured INTO a HIP graph (stages enabled while the caller's stream was capturing): per stage, the
// intervals of the graph's most recent replay (ms) and the number of pairs; synchronises; the pairs stay valid.
// reset != 0 forgets them (call before capturing another graph).
int cffm_profile_collect_graph(float* ms /*[count]*/, int* calls /*[count]*/, int reset) {
    for (int i = 0; i < ST_COUNT; ++i) { ms[i] = 0.f; calls[i] = 0; }
#ifndef CFFM_EMU
    if (g_prof_capture_failed) {
        g_prof_capture_failed = false;
        g_prof_graph_recs.clear();
        return fail(-2, "cffm_profile_collect_graph: the runtime refused an event-record node during the capture");
    }
    for (auto& r : g_prof_graph_recs) {
        float t = 0.f;
        if (hipEventSynchronize(r.e1) != hipSuccess || hipEventElapsedTime(&t, r.e0, r.e1) != hipSuccess) {
            (void)hipGetLastError();
            return fail(-2, "cffm_profile_collect_graph: captured events are not readable (graph not replayed yet?)");
        }
        ms[r.stage] += t;
        calls[r.stage] += 1;
    }
    if (reset) { g_prof_graph_recs.clear(); (void)hipGetLastError(); }   // (the events themselves belong to the graph's nodes: not destroyed here)
#endif
    return 0;
}
}

extern "C" {

int cffm_abi_version(void) { return CFFM_ABI_VERSION; }
const char* cffm_last_error(void) { return g_err; }

int cffm_geom_init(cffm_geom* g, int B, int H0, int W0) {
    REQUIRE(g, "geom_init: null");
    REQUIRE(B >= 1 && H0 >= 1 && W0 >= 1, "geom_init: bad sizes B=%d H0=%d W0=%d", B, H0, W0);
    g->B = B; g->H0 = H0; g->W0 = W0;
    g->Hp = (H0 + 6) / 7 * 7; g->Wp = (W0 + 6) / 7 * 7;
    g->gy = g->Hp / 7; g->gx = g->Wp / 7;
    g->nW = g->gy * g->gx; g->HW = H0 * W0; g->RC = 64 * g->nW;
    return 0;
}

static long up(long v) { return (v + 63) / 64 * 64; }  // keep every carve 256-B aligned

int cffm_block_ws_layout(const cffm_geom* g, cffm_block_ws* o) {
    REQUIRE(g && o, "ws_layout: null");
    const long B = g->B, HW = g->HW, RC = g->RC, nW = g->nW;
    long p = 0;
    o->mean1 = p; p += up(B * 4 * HW);
    o->rstd1 = p; p += up(B * 4 * HW);
    o->M = p; p += up(CFFM_NCELL * CFFM_WA);
    o->zall = p; p += up(B * RC * CFFM_C);
    o->qkv = p; p += up(B * RC * 768 / 2);   // f16 q|k|v
    o->bias = p; p += up((long)BIASH_HALFS / 2);                  // biasH: f16 B-operand fragments of the position bias (tile pairs)
    o->biasT = o->bias;                                           // (kept in the struct for ABI stability: no key-major table any more)
    o->lse = p; p += up(B * nW * CFFM_HEADS * CFFM_NQ_PAD);
    o->ao = p; p += up(B * HW * CFFM_C);
    o->x1 = p; p += up(B * HW * CFFM_C);
    o->mean2 = p; p += up(B * HW);
    o->rstd2 = p; p += up(B * HW);
    const long NP32 = (B * HW + 31) / 32 * 32, NR32 = (B * RC + 31) / 32 * 32;   // T-frag storage pads the token rows to whole k-steps of 32
    o->z2 = p; p += up(NP32 * CFFM_C);
    o->hraw = p; p += up(B * HW * CFFM_HID);
    o->act = p; p += up(NP32 * CFFM_HID);
    o->x2 = p; p += up(B * HW * CFFM_C);
    o->w_split = p; p += up(PREP_WFLOATS);   // qkv | proj | fc1 | fc2 weights in split-4 storage (k_param_prep)
    o->w_frag = p; p += up(2 * PREP_WFLOATS); // the same in MFMA-fragment order: forward forms, then input-gradient forms (row-panel kernels)
    o->ao_t = p; p += up(NP32 * CFFM_C);      // T-frag copies of ao and zall: operands of the streaming weight gradients (dws_kernels.h; ABI 9)
    o->zall_t = p; p += up(NR32 * CFFM_C);
    o->total = p;
    return 0;
}

long cffm_layer_saved_floats(const cffm_geom* g, int depth) {
    cffm_block_ws w;
    if (cffm_block_ws_layout(g, &w)) return -1;
    return up((long)g->B * 4 * g->HW * CFFM_C) + depth * w.total;
}

// scratch carve (floats): fwd uses [0, BHW*C); bwd uses all of it
struct Scratch { long a, a2, b, dz2, dao, dact, dqkv, dzall, dM, dbiasT, dxs, dkvp, alt, tf, tf_stride, total; };
static Scratch scratch_layout(const cffm_geom* g) {
    const long B = g->B, HW = g->HW, RC = g->RC;
    Scratch s;
    long p = 0;
    s.a = p; p += up(B * HW * CFFM_C);
    s.a2 = p; p += up(B * HW * CFFM_C);   // the blocks' target-frame gradient ping-pongs between a and a2 (see layer_backward_impl)
    s.b = p; p += up(B * HW * CFFM_C);
    s.dz2 = p; p += up(B * HW * CFFM_C);
    s.dao = p; p += up(B * HW * CFFM_C);
    const long NP32 = (B * HW + 31) / 32 * 32, NR32 = (B * RC + 31) / 32 * 32;   // T-frag storage pads the token rows to whole k-steps of 32
    s.dact = p; p += up(NP32 * CFFM_HID);
    s.dqkv = p; p += up(B * RC * 768);
    s.dzall = p; p += up(B * RC * CFFM_C);
    s.dM = p; p += up(CFFM_NCELL * CFFM_WA);
    s.dbiasT = p; p += up((long)CFFM_HEADS * CFFM_NQ_PAD * CFFM_NKEY_PAD);
    s.dxs = p; p += up(B * 4 * HW * CFFM_C);
    s.dkvp = p; p += up(B * g->nW * ((long)CFFM_NKEY_PAD * 256 + CFFM_HEADS));   // f16 partial rows + their (window, head) scales
    // second copies of what a block's side work (weight-gradient GEMMs, column sums, bias-tile sum) still reads after the chain has
    // moved on to the next block: blocks alternate between the two sets (block_backward_impl `par`), so the next block's chain never
    // waits for the side streams.  Offsets relative to `alt`: b | dact | dqkv | dbiasT | dM
    s.alt = p;
    p += up(B * HW * CFFM_C) + up(NP32 * CFFM_HID) + up(B * RC * 768) + up((long)CFFM_HEADS * CFFM_NQ_PAD * CFFM_NKEY_PAD) + up(CFFM_NCELL * CFFM_WA);
    // T-frag copies of dout | dx1 | dqkv for the streaming weight gradients, one set per parity (the side stream reads them after the chain has moved on)
    s.tf = p;
    s.tf_stride = 2 * up(NP32 * CFFM_C) + up(NR32 * 768);
    p += 2 * s.tf_stride;
    s.total = p;
    return s;
}
long cffm_layer_scratch_floats(const cffm_geom* g) { return scratch_layout(g).total; }


// ------------------------------------------------------------------------------------------- internal scratch
// Every library-owned buffer is a DevBuf: it only grows, to exactly what is asked; the old buffer is freed behind a device
// synchronisation (work in flight may still use it); NULL, and nothing held, when the allocation fails.
struct DevBuf {
    float* p = nullptr;
    size_t floats = 0;
    float* grow(size_t nfloats) {
        if (nfloats <= floats) return p;
        if (p) { (void)hipDeviceSynchronize(); (void)hipFree(p); }
        if (hipMalloc((void**)&p, nfloats * sizeof(float)) != hipSuccess) p = nullptr;
        floats = p ? nfloats : 0;
        return p;
    }
};
// Small library-owned device buffer for the block-partial records of the two-stage reductions
// (grows on demand; stream-ordered reuse, one stream at a time as the ABI's threading rule says).
// One pool per stream a stage call can arrive on: the caller's (0), the four branches of cffm_branch_begin / _take (1..4) and the deferred
// branch of cffm_defer_begin (5) -- stage calls
// that need scratch (split-K slabs of the weight gradients, column-sum records) may then run on different branches at the same time.
// ScratchFor selects the pool for the duration of a public stage call from its `stream` argument; everything else uses pool 0.
static DevBuf g_scr[6];
static int g_scr_sel = 0;
extern "C++" __attribute__((visibility("hidden"))) float* lib_scratch(size_t nfloats) { return g_scr[g_scr_sel].grow(nfloats); }
// second scratch buffer, for work issued on the library's side stream (runs concurrently with users of lib_scratch)
static DevBuf g_scr2;
static float* lib_scratch2(size_t nfloats) { return g_scr2.grow(nfloats); }
// third scratch buffer: the per-group bias-gradient tiles of the attention backward (read by a side-stream kernel while the
// caller's stream goes on using lib_scratch)
static DevBuf g_scr3;
static float* lib_scratch3(size_t nfloats) { return g_scr3.grow(nfloats); }
// ---- side stream of the block backward -----------------------------------------------------------------------------------
// Everything of a block backward that only produces PARAMETER gradients feeds nothing inside the chain (only the optimizer reads
// it): the four weight-gradient GEMMs, the bias-gradient tile sum + scatter, the q|k|v bias column sum, the record reductions and
// the pooling-matrix backward.  The small ones are launch- / latency-bound kernels of a few workgroups each (~45 us per block
// back to back) that truly overlap with the chain's kernels; the GEMMs need the whole chip and overlap only partly.
// All of it is issued on a library-owned second stream, forked from / joined to the caller's stream with events:
// launched eagerly the two streams overlap on the device; captured into a HIP graph (bench.py) the fork becomes a parallel
// branch of the graph.  cffm_side_streams(0) keeps everything on the caller's stream (per-kernel timing).
struct SideStream {
    bool on = false;
    int ns = 1;                 // side streams in use: 1 launched eagerly, 4 under stream capture and for the caller's branches
    hipStream_t st[4] = {nullptr, nullptr, nullptr, nullptr};
    hipEvent_t fork[4] = {nullptr, nullptr, nullptr, nullptr}, join[2] = {nullptr, nullptr}, order = nullptr, tail_order = nullptr;
    // deferred join of a block backward (layer_backward_impl): what the NEXT block has to wait for
    hipEvent_t dw_done[2] = {nullptr, nullptr}, bias_done[2] = {nullptr, nullptr}, tail_done[2] = {nullptr, nullptr}, join_all[4] = {nullptr, nullptr, nullptr, nullptr};
    bool bias_pending[2] = {false, false}, dw_pending[2] = {false, false}, tail_pending[2] = {false, false};
    const float* dw_dout[2] = {nullptr, nullptr};   // the `dout` a pending weight-gradient group still reads
    int par = 0;                // scratch set of the block backward being issued
    unsigned used = 0;          // side streams forked since the last full join
};
static SideStream g_side;
static struct { hipStream_t st = nullptr; hipEvent_t fork = nullptr, done = nullptr; bool used = false; int state = -1; } g_defer;   // cffm_defer_begin
struct ScratchFor {       // RAII: pool of the branch `stream` is (cffm_branch_begin / _take, cffm_defer_begin), else the caller's pool
    explicit ScratchFor(void* stream) {
        g_scr_sel = 0;
        for (int i = 0; i < 4; ++i)
            if (stream && (hipStream_t)stream == g_side.st[i]) g_scr_sel = i + 1;
        if (stream && (hipStream_t)stream == g_defer.st) g_scr_sel = 5;
    }
    ~ScratchFor() { g_scr_sel = 0; }
};
static int stream_is_capturing(hipStream_t st) {
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(st, &cs) != hipSuccess) { (void)hipGetLastError(); return 0; }
    return cs == hipStreamCaptureStatusActive ? 1 : 0;
}
// `main`: the caller's stream.  Launched eagerly ONE side stream measured best (0.877 vs 0.929 ms per step with two); under stream
// capture more (two: 0.882-0.895 vs 0.902-0.906 replayed: branches that do not queue behind each other give the graph executor more
// to run side by side; FOUR -- every branch of a block backward on its own stream -- another 0.8 %: 0.8894 vs 0.8963 as means of five
// alternating runs).
static bool side_init(hipStream_t main) {
    static int state = -1;
    if (state < 0) {
        state = 0;
        auto mk = [](hipStream_t* st_) { return hipStreamCreateWithFlags(st_, hipStreamNonBlocking) == hipSuccess; };
        if (mk(&g_side.st[0]) && mk(&g_side.st[1]) && mk(&g_side.st[2]) && mk(&g_side.st[3])) {
            bool ok = hipEventCreateWithFlags(&g_side.order, hipEventDisableTiming) == hipSuccess &&
                      hipEventCreateWithFlags(&g_side.tail_order, hipEventDisableTiming) == hipSuccess;
            for (int i = 0; i < 4; ++i) ok = ok && hipEventCreateWithFlags(&g_side.fork[i], hipEventDisableTiming) == hipSuccess;
            for (int i = 0; i < 2; ++i) ok = ok && hipEventCreateWithFlags(&g_side.join[i], hipEventDisableTiming) == hipSuccess;
            for (int i = 0; i < 2; ++i) ok = ok && hipEventCreateWithFlags(&g_side.tail_done[i], hipEventDisableTiming) == hipSuccess;
            for (int i = 0; i < 4; ++i) ok = ok && hipEventCreateWithFlags(&g_side.join_all[i], hipEventDisableTiming) == hipSuccess;
            for (int i = 0; i < 2; ++i) ok = ok && hipEventCreateWithFlags(&g_side.dw_done[i], hipEventDisableTiming) == hipSuccess &&
                                             hipEventCreateWithFlags(&g_side.bias_done[i], hipEventDisableTiming) == hipSuccess;
            state = ok ? 1 : 0;
        }
        (void)hipGetLastError();
    }
    g_side.on = state == 1 && !g_side_off;
    g_side.ns = stream_is_capturing(main) ? 4 : 1;
    return g_side.on;
}
// the stream branch `i` (0 / 1) of the side work runs on, ordered after everything issued on `main` so far
// How the side work of a block backward is attached to the chain.  Under stream capture the graph executor (ROCm 7.2) gives a node's
// FIRST-captured dependant the node's own stream and every further dependant the next of its (four) streams, depth first -- so whatever
// is launched first behind a fork stays on the chain's stream, and side branches that reach the same stream number run one after the
// other in topological order.  The chain must therefore be launched first at every fork and must never wait for a side branch inside
// the step.  block_backward_impl
//   launches the q|k|v input-gradient GEMM before the weight-gradient group,
//   gives the bias-tile sum + scatter no branch of their own: they follow the weight-gradient group on its stream,
//   launches the record reductions + pooling-matrix backward only after the NEXT chain kernel (tail_flush).
// Measured as a bit mask of forms (bits 1 / 2 / 5: the three choices above; bit 0: the dK/dV gather launched before a forked bias-tile
// sum) on B = 2, depth 2, replayed graph, same box: 0 -> 0.830-0.833 ms per step, 4 -> 0.808-0.810, 38 (with the two scratch sets
// of scratch_layout, so that no block waits for the previous block's weight gradients) -> 0.798-0.811 against 0.821-0.848 for 4;
// 35 (the bias-tile sum early again, now that every side branch lands on the same graph stream in launch order: it runs in the idle
// stretch beside the gather instead of behind the weight gradients on the step's tail) -> 0.773-0.785 against 0.783-0.786 for 38; with
// the last block's tail on the caller's stream and the L2 warm-up of the fused kernels 38 is ahead again (one fork less on the chain:
// a node with a dependant on another stream costs its same-stream successor ~5 us): 0.724-0.728 against 0.732-0.737 for 35.
// How the four weight-gradient GEMMs of a block backward are issued.  `one`: ONE grouped launch late in the block (59 us of GEMM +
// sum); `split`: two groups of two, each forked to the side stream as early as its operands allow (2 x 53 us, but off the chain
// sooner).  Launched eagerly the side stream really runs beside the chain and `split` wins (0.886 vs 0.911 ms per step); a replayed
// HIP graph executes its branches almost serially, so there the cheaper `one` wins (0.927 vs 0.950).  Default: by whether the
// caller's stream is being captured; CFFM_DW_GROUP=one|split forces a form.
static int dw_one_group(hipStream_t st) {
    static int forced = -2;
    if (forced == -2) { const char* e = getenv("CFFM_DW_GROUP"); forced = !e ? -1 : (e[0] == 's' ? 0 : 1); }
    if (forced >= 0) return forced;
#ifdef CFFM_EMU
    (void)st;
    return 1;     // (the emulator tests walk the grouped form; the split form is reached with CFFM_DW_GROUP=split)
#else
    return stream_is_capturing(st);
#endif
}
// Launch ORDER matters under stream capture: of the kernels that depend on one node, the graph executor keeps the FIRST-launched on
// the node's own hardware queue and moves the others to different queues -- and a dependency that crosses queues costs 5-10 us where
// same-queue succession costs ~1.5 (round-3 timeline: the chain hopped queues at every fork because the side work was launched first).
// So a fork is split: side_fork_mark() records the point on `main`, the chain's next kernel is launched, and only then
// side_fork_take() makes the side stream wait for the mark and hands it out.
static bool side_fork_mark(hipStream_t main, int i) { return g_side.on && hipEventRecord(g_side.fork[i], main) == hipSuccess; }
static hipStream_t side_fork_take(hipStream_t main, int i) {
    const int idx = g_side.ns >= 4 ? (i & 3) : 0;
    hipStream_t s = g_side.st[idx];
    if (g_side.on && hipStreamWaitEvent(s, g_side.fork[i], 0) == hipSuccess) {
        g_side.used |= 1u << idx;
        return s;
    }
    (void)hipGetLastError();
    return main;
}
static hipStream_t side_fork(hipStream_t main, int i) {     // (a mark that failed is not taken)
    if (side_fork_mark(main, i)) return side_fork_take(main, i);
    (void)hipGetLastError();
    return main;
}
// what is issued on `later` from here on runs after what has been issued on `earlier` (two different side streams)
static void side_order(hipStream_t earlier, hipStream_t later) {
    if (earlier != later && hipEventRecord(g_side.order, earlier) == hipSuccess) (void)hipStreamWaitEvent(later, g_side.order, 0);
}
static void side_mark(hipStream_t side, hipStream_t main, int i) {   // end of branch i
    if (side != main) (void)hipEventRecord(g_side.join[i], side);
}
static void side_join(hipStream_t side, hipStream_t main, int i) {   // `main` continues after branch i
    if (side != main) (void)hipStreamWaitEvent(main, g_side.join[i], 0);
}

// `main` continues after everything issued on any side stream since the last full join
static void side_join_all(hipStream_t main) {
    for (int i = 0; i < 4; ++i)
        if ((g_side.used >> i) & 1u) {
            if (hipEventRecord(g_side.join_all[i], g_side.st[i]) == hipSuccess) (void)hipStreamWaitEvent(main, g_side.join_all[i], 0);
        }
    g_side.used = 0;
    g_side.bias_pending[0] = g_side.bias_pending[1] = g_side.dw_pending[0] = g_side.dw_pending[1] = g_side.tail_pending[0] = g_side.tail_pending[1] = false;
    (void)hipGetLastError();
}
// ---- branches for the CALLER (ABI 10): independent stage calls of the head's rows path side by side -------------------------------
// The head around the hot path (rows f.1 / f.2 of SURVEY 8: embedding per scale, composed weights, classifiers) is a sequence of stage
// calls from Python, most of them 5-15 us kernels that do not depend on each other (four scales, weight vs input gradients): on ONE
// stream a replayed step pays ~5 us of launch latency per kernel (profiles/r06_head_timeline_before.txt: ~60 such kernels).
// cffm_branch_begin(stream, i) hands out library-owned stream i (0..3), ordered behind everything issued on `stream` so far; the caller
// passes it as the `stream` argument of the stage calls of that branch; cffm_branch_join(stream) makes `stream` continue behind all
// branches.  Under stream capture the branches become parallel branches of the graph.  Rules: every tensor a branch touches stays alive
// until the join; the stage calls that use the library's own scratch (weight gradients, column sums) take it from the pool of the
// branch they are issued on (ScratchFor); with side streams off (cffm_side_streams(0)), on failure, or in the emulator build the
// caller's own stream comes back and everything simply runs in order.
// Launch ORDER matters under capture (see side_fork_mark): of the dependants of one node the graph executor keeps the FIRST-launched on the
// node's own hardware queue, the others start on other queues ~10 us later each.  So the caller marks the fork point (cffm_branch_mark), launches
// its own -- longest -- chain on `stream` first and only then takes the branches (cffm_branch_take) for the shorter ones.
// cffm_branch_begin = mark + take of one branch at the current point.
int cffm_branch_mark(void* stream) {
    hipStream_t main = (hipStream_t)stream;
    if (!side_init(main)) return 0;
    g_side.ns = 4;
    for (int i = 0; i < 4; ++i)
        if (hipEventRecord(g_side.fork[i], main) != hipSuccess) { (void)hipGetLastError(); return 0; }
    return 1;
}
void* cffm_branch_take(void* stream, int i) {
    if (i < 0 || i > 3 || !g_side.on) return stream;
    hipStream_t s = g_side.st[i];
    if (hipStreamWaitEvent(s, g_side.fork[i], 0) == hipSuccess) {
        g_side.used |= 1u << i;
        return (void*)s;
    }
    (void)hipGetLastError();
    return stream;
}
void* cffm_branch_begin(void* stream, int i) {
    hipStream_t main = (hipStream_t)stream;
    if (i < 0 || i > 3 || !side_init(main)) return stream;
    g_side.ns = 4;
    if (hipEventRecord(g_side.fork[i], main) == hipSuccess) return cffm_branch_take(stream, i);
    (void)hipGetLastError();
    return stream;
}
int cffm_branch_join(void* stream) {
    side_join_all((hipStream_t)stream);
    return 0;
}
// A DEFERRED branch for the caller (ABI 10): work whose results the caller's stream needs much later than the next call -- the frame
// classifier's backward of the CFFM heads (cffm_head.py:121: its input gradient is needed by linear_fuse's BatchNorm backward, its weight /
// bias gradients by the optimizer, and the whole CFFM layer's backward lies between).  cffm_defer_begin(stream): a library-owned stream
// of its own (not one of the four branches: the layer's own side work uses those and must not queue behind 270 us of classifier kernels),
// ordered behind everything issued on `stream` so far; cffm_defer_join(stream): `stream` continues behind it (a no-op when nothing is
// pending).  Everything the deferred work touches must stay alive, and nothing on `stream` may read its results, until the join.
void* cffm_defer_begin(void* stream) {
    hipStream_t main = (hipStream_t)stream;
    if (g_side_off) return stream;
    if (g_defer.state < 0) {
        g_defer.state = (hipStreamCreateWithFlags(&g_defer.st, hipStreamNonBlocking) == hipSuccess &&
                         hipEventCreateWithFlags(&g_defer.fork, hipEventDisableTiming) == hipSuccess &&
                         hipEventCreateWithFlags(&g_defer.done, hipEventDisableTiming) == hipSuccess) ? 1 : 0;
        (void)hipGetLastError();
    }
    if (g_defer.state == 1 && hipEventRecord(g_defer.fork, main) == hipSuccess && hipStreamWaitEvent(g_defer.st, g_defer.fork, 0) == hipSuccess) {
        g_defer.used = true;
        return (void*)g_defer.st;
    }
    (void)hipGetLastError();
    return stream;
}
int cffm_defer_join(void* stream) {
    if (g_defer.used) {
        if (hipEventRecord(g_defer.done, g_defer.st) == hipSuccess) (void)hipStreamWaitEvent((hipStream_t)stream, g_defer.done, 0);
        g_defer.used = false;
        (void)hipGetLastError();
    }
    return 0;
}
// event helpers of the deferred join (no-ops when the work ran on `main` itself)
static void side_record(hipStream_t side, hipStream_t main, void* ev) {
    if (side != main) (void)hipEventRecord((hipEvent_t)ev, side);
}
static void side_wait(hipStream_t main, void* ev) { (void)hipStreamWaitEvent(main, (hipEvent_t)ev, 0); }
static void dw_group_launched(hipStream_t side) { (void)hipEventRecord(g_side.dw_done[g_side.par], side); }

static void seg_add(RedSegs& r, int off, int width, float* out, int accumulate) {
    if (!out) return;
    const int k = r.nseg++;
    r.off[k] = off; r.width[k] = width; r.out[k] = out; r.accumulate[k] = accumulate;
}
// Deferred second stages: inside a block backward (RedScope) the reductions are queued -- each with its own slice of a
// library-owned record buffer -- and run as ONE launch at the end of the scope; outside a scope they launch at once.
// Two record buffers, used alternately by consecutive scopes (block backwards): the reduction of block i (side stream) may still
// read its records while block i - 1 already writes its own (deferred join, see block_backward_impl)
static DevBuf g_redbuf[2];
static int g_red_parity = 0;
static struct { bool active; size_t bump; RedJobs jobs; } g_rq = {false, 0, {}};
static void redq_launch(RedJobs& J, hipStream_t st) {
    if (J.njob == 1) {
        CFFM_LAUNCH(k_reduce_records, ((J.total[0] + 63) / 64), (1024), 0, st, J.part[0], J.nblk[0], J.stride[0], J.total[0], J.segs[0]);
    } else if (J.njob > 1) {
        CFFM_LAUNCH(k_reduce_records_multi, ((unsigned)J.blk_end[J.njob - 1]), (1024), 0, st, J);
    }
    J.njob = 0;
}
static void redq_flush(hipStream_t st) { redq_launch(g_rq.jobs, st); }
struct RedScope {
    hipStream_t st;
    explicit RedScope(hipStream_t s) : st(s) { g_red_parity ^= 1; g_rq.active = true; g_rq.bump = 0; g_rq.jobs.njob = 0; }
    void finish() { redq_flush(st); g_rq.active = false; }
    void finish_on(hipStream_t other) { redq_flush(other); g_rq.active = false; }
    ~RedScope() { g_rq.active = false; g_rq.jobs.njob = 0; }
};
// block-partial record buffer of one reduction
static float* red_scratch(size_t nfloats, hipStream_t st) {
    if (!g_rq.active) return lib_scratch(nfloats);
    nfloats = (nfloats + 63) / 64 * 64;
    DevBuf& red = g_redbuf[g_red_parity];
    if (g_rq.bump + nfloats > red.floats) {
        (void)hipDeviceSynchronize();   // (growth happens in the first step only) the records queued so far may have been written on another stream
        redq_flush(st);   // queued jobs read the old buffer
        const size_t want = 2 * (g_rq.bump + nfloats);
        g_rq.bump = 0;
        if (!red.grow(want)) return nullptr;
    }
    float* p = red.p + g_rq.bump;
    g_rq.bump += nfloats;
    return p;
}
static void reduce_records(const float* part, int nblk, int stride, int total, const RedSegs& segs, hipStream_t st) {
    if (!g_rq.active) {
        CFFM_LAUNCH(k_reduce_records, ((total + 63) / 64), (1024), 0, st, part, nblk, stride, total, segs);
        return;
    }
    RedJobs& J = g_rq.jobs;
    if (J.njob == RED_MAXJOB) redq_flush(st);
    const int j = J.njob++;
    J.part[j] = part; J.nblk[j] = nblk; J.stride[j] = stride; J.total[j] = total; J.segs[j] = segs;
    J.blk_end[j] = (j ? J.blk_end[j - 1] : 0) + (total + 63) / 64;
}

static bool aligned16(const void* p) { return p && (uintptr_t)p % 16 == 0; }     // what the vector loads of a kernel ask of a tensor
static unsigned ew_grid(long n4) {
    long b = (n4 + 255) / 256;
    return (unsigned)(b > 4096 ? 4096 : (b < 1 ? 1 : b));
}

// ------------------------------------------------------------------------------------------- stages
static int transpose_add(const float* src, float* dst, int batch, int rows, int cols, long src_bs, long dst_bs, const float* addend,
                         int add_mod, int add_skip, void* stream, float* copy_dst = nullptr) {
    PROF(ST_TRANSPOSE);
    REQUIRE(src && dst && batch > 0 && rows > 0 && cols > 0, "transpose: bad arguments");
    CFFM_LAUNCH(k_transpose, ((cols + 63) / 64, (rows + 63) / 64, batch), (256), 0, (hipStream_t)stream, src, dst, rows, cols,
                src_bs, dst_bs, addend, add_mod > 0 ? add_mod : 1, add_skip, copy_dst);
    CHECK_LAUNCH("transpose");
    return 0;
}
// a += b over n floats (n % 4 == 0): summing the per-clip pieces of a gradient on the stream they were computed on
int cffm_add_inplace(float* a, const float* b, long n, void* stream) {
    REQUIRE(a && b && n >= 0 && n % 4 == 0, "add_inplace: n must be a multiple of 4");
    if (!n) return 0;
    CFFM_LAUNCH(k_add_inplace, (ew_grid(n / 4)), (256), 0, (hipStream_t)stream, a, b, n / 4);
    CHECK_LAUNCH("add_inplace");
    return 0;
}
int cffm_transpose(const float* src, float* dst, int batch, int rows, int cols, long src_bs, long dst_bs, void* stream) {
    return transpose_add(src, dst, batch, rows, cols, src_bs, dst_bs, nullptr, 1, -1, stream);
}

int cffm_pool_matrix(const float* const pool_w[4], float* M, void* stream) {
    PROF(ST_POOLMAT);
    PoolW pw;
    for (int i = 0; i < 4; ++i) { REQUIRE(pool_w[i], "pool_matrix: null weight %d", i); pw.w[i] = pool_w[i]; }
    CFFM_LAUNCH(k_pool_matrix, (1), (256), 0, (hipStream_t)stream, pw, M);
    CHECK_LAUNCH("pool_matrix");
    return 0;
}

static thread_local int g_grad_pads = 0;   // per calling thread (autograd runs one backward thread per device: ADVICE r4)
void cffm_grad_slices_padded(int yes) { g_grad_pads = yes ? 1 : 0; }

// `split`: the rows a GEMM is the only reader of are written in split-4 storage (cffm_common.h); the public stage
// functions always write plain fp32, the block orchestration asks for split-4 when the hand-written GEMMs are in use
static int ln_pool_fwd_impl(const cffm_geom* g, const float* x_ref, long ref_bs, const float* x_tgt, long tgt_bs,
                            const float* gamma, const float* beta, const float* M, const float* const pool_b[4],
                            float* zall, float* mean, float* rstd, int split, void* stream, const float* const* pool_w = nullptr) {
    PROF(ST_LN_POOL_FWD);
    REQUIRE(g && x_ref && x_tgt && zall, "ln_pool_fwd: null");
    PoolB pb;
    PoolW pw;
    for (int i = 0; i < 4; ++i) { pb.b[i] = pool_b[i]; pw.w[i] = pool_w ? pool_w[i] : nullptr; }
    CFFM_LAUNCH(k_ln_pool_fwd<false>, (g->nW, 4, g->B), (LNP_THREADS), 0, (hipStream_t)stream, to_geo(g), x_ref, ref_bs, x_tgt, tgt_bs, gamma,
                beta, pool_w ? nullptr : M, pw, pb, zall, mean, rstd, split, LnpNoRing());
    CHECK_LAUNCH("ln_pool_fwd");
    return 0;
}
int cffm_ln_pool_fwd(const cffm_geom* g, const float* x_ref, long ref_bs, const float* x_tgt, long tgt_bs,
                     const float* gamma, const float* beta, const float* M, const float* const pool_b[4],
                     float* zall, float* mean, float* rstd, void* stream) {
    return ln_pool_fwd_impl(g, x_ref, ref_bs, x_tgt, tgt_bs, gamma, beta, M, pool_b, zall, mean, rstd, 0, stream);
}

// ---- CFFA backward (cffa_kernels.h): target frame per block, reference frames once per range of blocks ------------------------------
static long cffa_rows(const cffm_geom* g) { return (long)g->B * g->nW * LNB_SPLIT; }     // records per kernel launch and block
static int ln_pool_bwd_tgt(const cffm_geom* g, const float* x_tgt, long tgt_bs, const float* gamma, const float* beta, const float* M,
                           const float* mean, const float* rstd, const float* dzall, const float* dres, float* dx_tgt, long dtgt_bs,
                           float* rec, void* stream) {
    PROF(ST_LN_POOL_BWD);
    CFFM_LAUNCH(k_ln_pool_bwd_tgt, ((unsigned)cffa_rows(g)), (LNB_THREADS), 0, (hipStream_t)stream, to_geo(g), x_tgt, tgt_bs, gamma, beta, M, mean, rstd,
                dzall, dres, dx_tgt, dtgt_bs, rec);
    CHECK_LAUNCH("ln_pool_bwd_tgt");
    return 0;
}
extern "C++" {
template <int D>
static int ln_pool_bwd_ref_d(const cffm_geom* g, const float* x_ref, long ref_bs, const CffaRefBlocks& Bk, const float* mean, const float* rstd,
                             float* dx_ref, long dref_bs, int accum, hipStream_t st) {
    constexpr int lds = cffa_ref_lds(D);
    static int lds_have = 0;
    if (lds > 64 * 1024 && !lds_grant(lds_have, {{(const void*)k_ln_pool_bwd_ref<D, false>, lds}, {(const void*)k_ln_pool_bwd_ref<D, true>, lds}})) return -1;
    if (accum) CFFM_LAUNCH((k_ln_pool_bwd_ref<D, true>), ((unsigned)cffa_rows(g)), (LNB_THREADS), lds, st, to_geo(g), x_ref, ref_bs, Bk, mean, rstd, dx_ref, dref_bs);
    else CFFM_LAUNCH((k_ln_pool_bwd_ref<D, false>), ((unsigned)cffa_rows(g)), (LNB_THREADS), lds, st, to_geo(g), x_ref, ref_bs, Bk, mean, rstd, dx_ref, dref_bs);
    return 0;
}
}  // extern "C++"
// the reference frames of Bk.n <= RB_MAXD blocks; accum: dx_ref already holds the share of blocks handled earlier
static int ln_pool_bwd_ref(const cffm_geom* g, const float* x_ref, long ref_bs, const CffaRefBlocks& Bk, const float* mean, const float* rstd,
                           float* dx_ref, long dref_bs, int accum, void* stream) {
    PROF(ST_LN_POOL_BWD_REF);
    hipStream_t st = (hipStream_t)stream;
    int rc = -1;
    switch (Bk.n) {
        case 1: rc = ln_pool_bwd_ref_d<1>(g, x_ref, ref_bs, Bk, mean, rstd, dx_ref, dref_bs, accum, st); break;
        case 2: rc = ln_pool_bwd_ref_d<2>(g, x_ref, ref_bs, Bk, mean, rstd, dx_ref, dref_bs, accum, st); break;
        case 3: rc = ln_pool_bwd_ref_d<3>(g, x_ref, ref_bs, Bk, mean, rstd, dx_ref, dref_bs, accum, st); break;
        case 4: rc = ln_pool_bwd_ref_d<4>(g, x_ref, ref_bs, Bk, mean, rstd, dx_ref, dref_bs, accum, st); break;
        default: break;
    }
    REQUIRE(!rc, "ln_pool_bwd_ref: bad block count %d or LDS grant failed", Bk.n);
    CHECK_LAUNCH("ln_pool_bwd_ref");
    return 0;
}
// The three record sums of one block (its target records in rec[0, rows), its reference records in rec[rows, 2 rows)): norm1's
// dgamma | dbeta over both, the target tail (dM cell 0, pool bias 0), the reference tail (dM cells 1..14, pool biases 1..3) -- appended
// to J (launched when it is full; the caller launches the rest with redq_launch).
static void job_add(RedJobs& J, const float* part, int nblk, int stride, int total, const RedSegs& segs, hipStream_t st) {
    if (J.njob == RED_MAXJOB) redq_launch(J, st);
    const int j = J.njob++;
    J.part[j] = part; J.nblk[j] = nblk; J.stride[j] = stride; J.total[j] = total; J.segs[j] = segs;
    J.blk_end[j] = (j ? J.blk_end[j - 1] : 0) + (total + 63) / 64;
}
static void cffa_jobs(RedJobs& J, const float* rec, long rows, float* dgamma, float* dbeta, float* dM, float* const dpool_b[4], hipStream_t st) {
    RedSegs a, b, c;
    a.nseg = b.nseg = c.nseg = 0;
    seg_add(a, 0, CFFM_C, dgamma, 0);
    seg_add(a, CFFM_C, CFFM_C, dbeta, 0);
    job_add(J, rec, (int)(2 * rows), LNP_RSTRIDE, 2 * CFFM_C, a, st);
    seg_add(b, 0, CFFM_WA, dM, 0);
    seg_add(b, CFFM_WA, 1, dpool_b[0], 0);
    job_add(J, rec + 2 * CFFM_C, (int)rows, LNP_RSTRIDE, LNP_TAIL_TGT, b, st);
    seg_add(c, 0, 14 * CFFM_WA, dM + CFFM_WA, 0);
    for (int i = 1; i < 4; ++i) seg_add(c, 14 * CFFM_WA + i - 1, 1, dpool_b[i], 0);
    job_add(J, rec + rows * LNP_RSTRIDE + 2 * CFFM_C, (int)rows, LNP_RSTRIDE, LNP_TAIL_REF, c, st);
}
// The end of a range: the record reductions of J and the dx transpose's tiles (A.T.gx == 0: none) as ONE launch (k_bwd_tail,
// rowops_kernels.h).  The forward's k_transpose_prep is the model: work that does not depend on each other shares a launch instead of a
// side stream, which the graph executor would queue ahead of the weight-gradient groups.  The pooling-matrix backward reads the dM the
// reductions write, so it stays a launch of its own behind this one.
static void tail_transpose(TailArgs& A, const float* src, float* dst, int batch, int rows, int cols, long src_bs, long dst_bs, const float* addend,
                           int add_mod, int add_skip) {
    A.T = {src, dst, rows, cols, src_bs, dst_bs, add_mod > 0 ? add_mod : 1, add_skip, nullptr, (cols + 63) / 64, (rows + 63) / 64, batch};
    A.addend = addend;
}
static void bwd_tail_launch(TailArgs& A, RedJobs& J, hipStream_t st) {
    for (int j = 0; j < J.njob; ++j) A.red_end[j] = (j ? A.red_end[j - 1] : 0) + (J.total[j] + 31) / 32;
    const long grid = (long)A.T.gx * A.T.gy * A.T.gz + (J.njob ? A.red_end[J.njob - 1] : 0);
    if (grid > 0) CFFM_LAUNCH(k_bwd_tail, ((unsigned)grid), (256), 0, st, A, J);
    J.njob = 0;
}

// Library-owned state of the CFFA backward, one SLOT per block of the layer: the block's token-row gradient dzall (written by the q|k|v
// input-gradient GEMM, its pooled-cell rows are read again by the reference pass at the end of the range), the records of its target
// and reference workgroups, its pooling-matrix gradient.
static DevBuf g_scr4;
struct CffaSlot { float* dzall; float* rec; float* dM; };
static int cffa_slot(const cffm_geom* g, int slot, int nslots, CffaSlot* o) {
    const long a = up((long)g->B * g->RC * CFFM_C), b = up(2 * cffa_rows(g) * LNP_RSTRIDE), c = up(CFFM_NCELL * CFFM_WA);
    float* base = g_scr4.grow((size_t)(a + b + c) * nslots);
    REQUIRE(base && slot >= 0 && slot < nslots, "cffa: scratch allocation failed");
    float* p = base + (a + b + c) * slot;
    o->dzall = p; o->rec = p + a; o->dM = p + a + b;
    return 0;
}
// One block's share of the end of the CFFA backward: what the reference pass reads of it (norm1, its composed pooling matrix, the saved
// LayerNorm statistics, its token-row gradient), its records (target workgroups in rec[0, rows), reference workgroups behind them), its
// pooling-matrix gradient and where its parameter gradients go.
struct CffaBlk {
    const float *gamma, *beta, *M, *mean, *rstd, *dzall;
    float *rec, *dM;
    float *dgamma, *dbeta;
    float* const* dpool_w;
    float* const* dpool_b;
};
// The reference frames of `count` blocks in one pass (RB_MAXD blocks per launch, the launches after the first add to dx_ref) -> dx_ref,
// then every CFFA parameter gradient of those blocks: norm1, the pooling matrix -> the pooling Linears, the pool biases.  The target
// records of every block are written by now (ln_pool_bwd_tgt).
// `extra` (or NULL): record reductions of the caller that are due at this point of the stream anyway (the last block's parameter-gradient
// tail): they join the final reduction launch instead of taking one of their own.
// `tail` (or NULL): the caller's dx transpose (tail_transpose), which rides in the same launch.
static int cffa_finish_blocks(const cffm_geom* g, const CffaBlk* blk, int count, const float* x_ref, long ref_bs, float* dx_ref, long dref_bs,
                              int accum, void* stream, RedJobs* extra = nullptr, const TailArgs* tail = nullptr) {
    hipStream_t st = (hipStream_t)stream;
    const long rows = cffa_rows(g);
    static_assert(PMB_MAXD == RB_MAXD, "one pooling-matrix launch per reference launch");
    for (int k0 = 0; k0 < count; k0 += RB_MAXD) {
        const int n = count - k0 < RB_MAXD ? count - k0 : RB_MAXD;
        const bool last = k0 + RB_MAXD >= count;     // the last round's reductions share a launch with the caller's transpose: k_bwd_tail
        CffaRefBlocks Bk;
        PoolWGN pw;
        RedJobs J;
        TailArgs A;
        if (tail) A = *tail; else A.T.gx = A.T.gy = A.T.gz = 0;
        Bk.n = n; J.njob = 0;
        for (int d = 0; d < RB_MAXD; ++d) {
            const CffaBlk& b = blk[k0 + (d < n ? d : 0)];
            Bk.gamma[d] = b.gamma; Bk.beta[d] = b.beta; Bk.M[d] = b.M;
            Bk.dzall[d] = b.dzall; Bk.rec[d] = b.rec + rows * LNP_RSTRIDE;
            pw.dM[d] = b.dM;
            for (int q = 0; q < 4; ++q) { pw.gw[d].w[q] = b.dpool_w[q]; pw.gw[d].b[q] = g_grad_pads ? b.dpool_b[q] : nullptr; }
        }
        // (the LayerNorm statistics of the reference frames are the same in every block: any block's saved copy serves)
        TRY(ln_pool_bwd_ref(g, x_ref, ref_bs, Bk, blk[k0].mean, blk[k0].rstd, dx_ref, dref_bs, accum || k0 != 0, stream));
        for (int d = 0; d < n; ++d) {
            const CffaBlk& b = blk[k0 + d];
            cffa_jobs(J, b.rec, rows, b.dgamma, b.dbeta, b.dM, b.dpool_b, st);
        }
        if (last && extra) {
            for (int j = 0; j < extra->njob; ++j) job_add(J, extra->part[j], extra->nblk[j], extra->stride[j], extra->total[j], extra->segs[j], st);
            extra->njob = 0;
        }
        if (last) bwd_tail_launch(A, J, st);
        else redq_launch(J, st);
        CHECK_LAUNCH("cffa reductions");
        {
            PROF(ST_POOLMAT);
            CFFM_LAUNCH(k_pool_matrix_bwd_n, (111, n), (64), 0, st, pw);
            CHECK_LAUNCH("pool_matrix_bwd");
        }
    }
    return 0;
}
// End of a range of block backwards (blocks first, first - 1, ..., last of a layer with `nslots` blocks; block i's parameters / gradients
// at params[i] / grads[i], its workspace at ws0 + i * ws_stride, its token-row gradient, records and pooling-matrix gradient in slot i).
static int cffa_finish(const cffm_geom* g, int nslots, const cffm_block_params* params, const cffm_block_grads* grads, int first, int last,
                       const float* ws0, long ws_stride, const float* x_ref, long ref_bs, float* dx_ref, long dref_bs, int accum, void* stream,
                       RedJobs* extra = nullptr, const TailArgs* tail = nullptr) {
    cffm_block_ws L;
    cffm_block_ws_layout(g, &L);
    const int count = first - last + 1;
    CffaBlk few[8];
    std::vector<CffaBlk> many;
    CffaBlk* blk = few;
    if (count > 8) { many.resize(count); blk = many.data(); }
    for (int k = 0; k < count; ++k) {
        const int i = first - k;
        const float* ws = ws0 + (long)i * ws_stride;
        CffaSlot S;
        TRY(cffa_slot(g, i, nslots, &S));
        blk[k] = {params[i].norm1_w, params[i].norm1_b, ws + L.M, ws + L.mean1, ws + L.rstd1, S.dzall, S.rec, S.dM,
                  grads[i].norm1_w, grads[i].norm1_b, grads[i].pool_w, grads[i].pool_b};
    }
    return cffa_finish_blocks(g, blk, count, x_ref, ref_bs, dx_ref, dref_bs, accum, stream, extra, tail);
}
// The CFFA backward as a stage: the target frame of each block (as the block backward runs it), then the end of the range above
int cffm_ln_pool_bwd(const cffm_geom* g, int n, const cffm_cffa_bwd_block* blocks, const float* x_ref, long ref_bs, float* dx_ref, long dref_bs,
                     int accum_ref, void* stream) {
    REQUIRE(g && blocks && x_ref && dx_ref, "ln_pool_bwd: null");
    REQUIRE(n >= 1 && n <= 8, "ln_pool_bwd: %d blocks (1..8 per call)", n);
    for (int d = 0; d < n; ++d) {
        const cffm_cffa_bwd_block& b = blocks[d];
        bool ok = b.x_tgt && b.gamma && b.beta && b.M && b.mean && b.rstd && b.dzall && b.dx_tgt && b.dgamma && b.dbeta;
        for (int q = 0; q < 4; ++q) ok = ok && b.dpool_w[q] && b.dpool_b[q];
        REQUIRE(ok, "ln_pool_bwd: null pointer in block %d", d);
    }
    CffaBlk blk[8];
    for (int d = 0; d < n; ++d) {
        const cffm_cffa_bwd_block& b = blocks[d];
        CffaSlot S;              // (the slot's own dzall stays unused: the caller brings the token-row gradient)
        TRY(cffa_slot(g, d, n, &S));
        TRY(ln_pool_bwd_tgt(g, b.x_tgt, b.tgt_bs, b.gamma, b.beta, b.M, b.mean, b.rstd, b.dzall, b.dres, b.dx_tgt, b.dtgt_bs, S.rec, stream));
        blk[d] = {b.gamma, b.beta, b.M, b.mean, b.rstd, b.dzall, S.rec, S.dM, b.dgamma, b.dbeta, b.dpool_w, b.dpool_b};
    }
    return cffa_finish_blocks(g, blk, n, x_ref, ref_bs, dx_ref, dref_bs, accum_ref, stream);
}

// ---- the end of a range as stages: the one launch, and the launches it replaced -------------------------------------------------------
static int record_sets(RedJobs& J, int nsets, const cffm_record_set* sets, const char* who) {
    REQUIRE(nsets >= 0 && nsets <= RED_MAXJOB && (sets || !nsets), "%s: %d record sets (0..%d per call)", who, nsets, RED_MAXJOB);
    J.njob = 0;
    for (int j = 0; j < nsets; ++j) {
        const cffm_record_set& s = sets[j];
        REQUIRE(aligned16(s.rec) && s.count >= 1 && s.total >= 1 && s.stride % 4 == 0 && s.stride >= (s.total + 3) / 4 * 4 && s.nseg >= 0 &&
                    s.nseg <= RED_MAXSEG, "%s: bad record set %d", who, j);
        RedSegs g;
        g.nseg = 0;
        for (int k = 0; k < s.nseg; ++k) {
            REQUIRE(s.out[k] && s.off[k] >= 0 && s.width[k] >= 0 && s.off[k] + s.width[k] <= s.total, "%s: bad segment %d of record set %d", who, k, j);
            seg_add(g, s.off[k], s.width[k], s.out[k], s.accumulate[k]);
        }
        const int i = J.njob++;
        J.part[i] = s.rec; J.nblk[i] = s.count; J.stride[i] = s.stride; J.total[i] = s.total; J.segs[i] = g;
        J.blk_end[i] = (i ? J.blk_end[i - 1] : 0) + (s.total + 63) / 64;
    }
    return 0;
}
int cffm_reduce_records(int nsets, const cffm_record_set* sets, void* stream) {
    RedJobs J;
    TRY(record_sets(J, nsets, sets, "reduce_records"));
    redq_launch(J, (hipStream_t)stream);
    CHECK_LAUNCH("reduce_records");
    return 0;
}
int cffm_pool_matrix_bwd(int n, const cffm_pool_grads* blocks, void* stream) {
    REQUIRE(n >= 1 && n <= PMB_MAXD && blocks, "pool_matrix_bwd: %d blocks (1..%d per call)", n, PMB_MAXD);
    PoolWGN pw;
    for (int d = 0; d < PMB_MAXD; ++d) {
        const cffm_pool_grads& b = blocks[d < n ? d : 0];
        REQUIRE(b.dM, "pool_matrix_bwd: null dM in block %d", d);
        for (int q = 0; q < 4; ++q) {
            REQUIRE(b.dpool_w[q] && b.dpool_b[q], "pool_matrix_bwd: null pointer in block %d", d);
            pw.gw[d].w[q] = b.dpool_w[q]; pw.gw[d].b[q] = g_grad_pads ? b.dpool_b[q] : nullptr;
        }
        pw.dM[d] = b.dM;
    }
    CFFM_LAUNCH(k_pool_matrix_bwd_n, (111, n), (64), 0, (hipStream_t)stream, pw);
    CHECK_LAUNCH("pool_matrix_bwd");
    return 0;
}
int cffm_bwd_tail(int nsets, const cffm_record_set* sets, const cffm_tail_transpose* tr, void* stream) {
    RedJobs J;
    TailArgs A;
    TRY(record_sets(J, nsets, sets, "bwd_tail"));
    A.T.gx = A.T.gy = A.T.gz = 0;
    if (tr) {
        REQUIRE(tr->src && tr->dst && tr->batch > 0 && tr->rows > 0 && tr->cols > 0, "bwd_tail: bad transpose");
        tail_transpose(A, tr->src, tr->dst, tr->batch, tr->rows, tr->cols, tr->src_bs, tr->dst_bs, tr->addend, tr->add_mod, tr->add_skip);
    }
    bwd_tail_launch(A, J, (hipStream_t)stream);
    CHECK_LAUNCH("bwd_tail");
    return 0;
}

int cffm_bias_assemble(const float* own, const float* ring, const float* const pool[4], float* bias, void* biasH, void* stream) {
    PROF(ST_BIAS_ASM);
    BiasTables t;
    t.own = own; t.ring = ring;
    for (int i = 0; i < 4; ++i) t.pool[i] = pool[i];
    const int n = CFFM_HEADS * CFFM_NQ_PAD * CFFM_NKEY_PAD;
    CFFM_LAUNCH(k_bias_assemble, ((n + 255) / 256), (256), 0, (hipStream_t)stream, t, bias, (h16*)biasH);
    CHECK_LAUNCH("bias_assemble");
    return 0;
}

int cffm_bias_scatter(const float* dbiasT, float* down, float* dring, float* const dpool[4], void* stream) {
    REQUIRE(dbiasT && down && dring && dpool && dpool[0] && dpool[1] && dpool[2] && dpool[3], "bias_scatter: null");
    PROF(ST_BIAS_SCT);
    BiasTablesG t;
    t.own = down; t.ring = dring;
    for (int i = 0; i < 4; ++i) t.pool[i] = dpool[i];
    CFFM_LAUNCH(k_bias_scatter, ((BIAS_SCATTER_THREADS + 255) / 256), (256), 0, (hipStream_t)stream, dbiasT, t);
    CHECK_LAUNCH("bias_scatter");
    return 0;
}

int cffm_attn_fwd(const cffm_geom* g, const void* qkv16, const int* key_src, const int* q_dst, const void* biasH, float* ao,
                  float* lse, void* stream) {
    PROF(ST_ATTN_FWD);
    REQUIRE(g && qkv16 && key_src && q_dst && biasH && ao && lse, "attn_fwd: null");
    const h16* bias = (const h16*)biasH;
    // one workgroup per (window, head), four per CU
    CFFM_LAUNCH(k_cfm_attn_fwd<false>, (g->B * g->nW * CFFM_HEADS), (256), ATT_FWD_LDS, (hipStream_t)stream, to_geo(g), (const h16*)qkv16,
                key_src, q_dst, bias, ao, lse);
    CHECK_LAUNCH("attn_fwd");
    return 0;
}

// window groups of the fused backward: 8 heads x groups <= one 12-wave workgroup per CU on 256 CUs, every group the same length
static int attn_bwd_groups(const cffm_geom* g, int* per_group) {
    const int total = g->B * g->nW;
    const int ng = total < 32 ? total : 32;
    *per_group = (total + ng - 1) / ng;
    return (total + *per_group - 1) / *per_group;
}

// the three pieces of the attention backward (the block backward puts the bias-gradient sum on its side stream)
static int attn_bwd_fused(const cffm_geom* g, const void* qkv16, const int* key_src, const int* q_dst, const h16* bias, const float* ao,
                          const float* dao, const float* lse, float* dqkv, float* dkv_part, float** dbp_out, int* ng_out, int par, void* stream) {
    PROF2(ST_ATTN_BWD_Q);
    int per;
    const int ng = attn_bwd_groups(g, &per);
    const long nb = (long)CFFM_HEADS * CFFM_NQ_PAD * CFFM_NKEY_PAD;   // one bias-gradient tile set per window group
    float* dbp = lib_scratch3((size_t)2 * ng * nb);      // two sets: see scratch_layout (alt)
    REQUIRE(dbp, "attn_bwd: scratch allocation failed");
    dbp += (size_t)(par ? 1 : 0) * ng * nb;
    static int lds_have = 0;
    REQUIRE(lds_grant(lds_have, {{(const void*)k_cfm_attn_bwd, ATT_BK_LDS}}), "attn_bwd: LDS grant failed");
    CFFM_LAUNCH(k_cfm_attn_bwd, (CFFM_HEADS, ng), (ATT_BK_THREADS), ATT_BK_LDS, (hipStream_t)stream, to_geo(g), (const h16*)qkv16, key_src, q_dst, bias,
                ao, dao, lse, dqkv, dbp, dkv_part, per);
    CHECK_LAUNCH("attn_bwd");
    *dbp_out = dbp; *ng_out = ng;
    return 0;
}
static int attn_bwd_bias_sum(const float* dbp, int ng, float* dbiasT, void* stream) {
    PROF2(ST_ATTN_BWD_KV);
    const long nb = (long)CFFM_HEADS * CFFM_NQ_PAD * CFFM_NKEY_PAD;
    CFFM_LAUNCH(k_sum_splits, ((unsigned)((nb / 4 + 63) / 64)), (256), 0, (hipStream_t)stream, dbp, ng, nb, dbiasT);
    CHECK_LAUNCH("attn_bwd bias sum");
    return 0;
}
static int attn_bwd_gather(const cffm_geom* g, const int* inv_ptr, const int* inv_idx, const float* dkv_part, float* dqkv, void* stream) {
    PROF2(ST_DKV_GATHER);
    REQUIRE((long)g->nW * CFFM_NKEY_PAD * 1024 < (1L << 32), "attn_bwd gather: a clip's partial rows must stay under 4 GB");
    CFFM_LAUNCH(k_dkv_gather, ((unsigned)(((long)g->B * g->RC + 3) / 4)), (256), 0, (hipStream_t)stream, to_geo(g), inv_ptr, inv_idx, dkv_part, dqkv);
    CHECK_LAUNCH("attn_bwd gather");
    return 0;
}
int cffm_dkv_gather(const cffm_geom* g, const int* inv_ptr, const int* inv_idx, const float* dkv_part, float* dqkv, void* stream) {
    REQUIRE(g && inv_ptr && inv_idx && dkv_part && dqkv, "dkv_gather: null");
    REQUIRE(g->B >= 1 && g->nW >= 1 && g->RC == 64 * g->nW && (long)g->B * g->RC < (1L << 31), "dkv_gather: bad geometry");
    return attn_bwd_gather(g, inv_ptr, inv_idx, dkv_part, dqkv, stream);
}
int cffm_attn_bwd(const cffm_geom* g, const void* qkv16, const int* key_src, const int* q_dst,
                  const int* inv_ptr, const int* inv_idx, const void* biasH, const float* ao,
                  const float* dao, const float* lse, float* dqkv, float* dbiasT, float* dkv_part, void* stream) {
    PROF(ST_ATTN_BWD);
    const h16* bias = (const h16*)biasH;
    REQUIRE(g && qkv16 && bias && dao && dqkv && dbiasT && dkv_part && inv_ptr && inv_idx, "attn_bwd: null");
    float* dbp;
    int ng;
    TRY(attn_bwd_fused(g, qkv16, key_src, q_dst, bias, ao, dao, lse, dqkv, dkv_part, &dbp, &ng, 0, stream));
    TRY(attn_bwd_bias_sum(dbp, ng, dbiasT, stream));
    TRY(attn_bwd_gather(g, inv_ptr, inv_idx, dkv_part, dqkv, stream));
    return 0;
}

int cffm_linear_fwd(const float* x, const float* w, float* y, long M, int N, int K, void* stream) {
    PROF(ST_GEMM);
    return gemm_nt(x, w, y, M, N, K, (hipStream_t)stream) ? fail(-3, "linear_fwd: gemm failed") : 0;
}
int cffm_linear_bias_fwd(const float* x, const float* w, const float* b, float* y, long M, int N, int K, void* stream) {
    REQUIRE(M >= 0 && N >= 4 && N % 4 == 0 && K >= 1, "linear_bias_fwd: bad sizes (N must be a multiple of 4)");
    if (!M) return 0;
    REQUIRE(x && w && b && y, "linear_bias_fwd: null");
    PROF(ST_GEMM);
    return gemm_split_launch<false, false>(x, w, y, (int)M, N, K, K, K, N, 1, (hipStream_t)stream, b) ? fail(-3, "linear_bias_fwd: gemm failed") : 0;
}
int cffm_linear_bwd_input(const float* dy, const float* w, float* dx, long M, int N, int K, void* stream) {
    PROF(ST_GEMM);
    return gemm_nn(dy, w, dx, M, N, K, (hipStream_t)stream) ? fail(-3, "linear_bwd_input: gemm failed") : 0;
}
int cffm_linear_bwd_weight(const float* dy, const float* x, float* dw, long M, int N, int K, void* stream) {
    ScratchFor pool(stream);
    PROF(ST_GEMM);
    return gemm_tn(dy, x, dw, M, N, K, (hipStream_t)stream) ? fail(-3, "linear_bwd_weight: gemm failed") : 0;
}

int cffm_linear_bwd_weight_group(const cffm_wgrad* problems, int n, void* stream) {
    REQUIRE(problems && n >= 1 && n <= 4, "linear_bwd_weight_group: 1..4 problems");
    static_assert(sizeof(cffm_wgrad) == sizeof(GemmTN), "wgrad layout");
    for (int i = 0; i < n; ++i) REQUIRE(problems[i].dy && problems[i].x && problems[i].dw, "linear_bwd_weight_group: null operand");
    ScratchFor pool(stream);
    PROF(ST_GEMM);
    if (gemm_tn_group((const GemmTN*)problems, n, (hipStream_t)stream)) return fail(-3, "linear_bwd_weight_group: gemm failed");
    CHECK_LAUNCH("linear_bwd_weight_group");
    return 0;
}

// the same call with the operand storage forms and the workgroup target the block backward passes (parity tests of the grouped kernel's forms)
int cffm_linear_bwd_weight_group_forms(const cffm_wgrad* problems, const cffm_wgrad_form* forms, int n, int target_wgs, void* stream) {
    REQUIRE(problems && forms && n >= 1 && n <= 4 && target_wgs >= 0, "linear_bwd_weight_group_forms: 1..4 problems");
    static_assert(sizeof(cffm_wgrad) == sizeof(GemmTN) && sizeof(cffm_wgrad_form) == sizeof(GemmTNPre), "wgrad layout");
    for (int i = 0; i < n; ++i) {
        REQUIRE(problems[i].dy && problems[i].x && problems[i].dw, "linear_bwd_weight_group_forms: null operand");
        REQUIRE((forms[i].dy_pre == 0 || forms[i].dy_pre == 1) && forms[i].x_pre >= 0 && forms[i].x_pre <= 2 && (forms[i].x_pre != 2 || forms[i].x_bias),
                "linear_bwd_weight_group_forms: unknown storage form");
    }
    ScratchFor pool(stream);
    PROF(ST_GEMM);
    if (gemm_tn_group((const GemmTN*)problems, n, (hipStream_t)stream, (const GemmTNPre*)forms, lib_scratch, target_wgs))
        return fail(-3, "linear_bwd_weight_group_forms: gemm failed");
    CHECK_LAUNCH("linear_bwd_weight_group_forms");
    return 0;
}

// row-major fp32 x[R][C] -> T-frag storage (dws_kernels.h: MFMA fragments along the contraction, bf16 hi | lo, rows padded to a multiple of
// 32 with zeros): what the operands of cffm_linear_bwd_weight_tfrag are stored as.  dst: cffm_tfrag_floats(R, C) floats.  A utility: inside
// the block the row-panel kernels leave their operands in this order themselves.
long cffm_tfrag_floats(long R, int C) { return R < 0 || C < 16 ? 0 : ((R + 31) / 32) * 32 * (long)C; }
int cffm_tfrag_pack(const float* x, float* dst, long R, int C, void* stream) {
    REQUIRE(x && dst && R >= 1 && C >= 16 && C % 16 == 0, "tfrag_pack: C must be a multiple of 16");
    const long items = ((R + 31) / 32) * (C / 16) * 64;
    CFFM_LAUNCH(k_tfrag_pack, ((unsigned)((items + 255) / 256)), (256), 0, (hipStream_t)stream, x, R, C, 0, (f32x4*)dst, items);
    CHECK_LAUNCH("tfrag_pack");
    return 0;
}
// dw[N,K] = dy[M,N]^T x[M,K] with dy and x in T-frag storage: the streaming weight-gradient kernel of the block backward (dws_kernels.h) as
// a stage.  N a multiple of 64, K a multiple of 128
int cffm_linear_bwd_weight_tfrag_group(const cffm_wgrad* problems, int n, void* stream) {
    REQUIRE(problems && n >= 1 && n <= DWS_MAX, "linear_bwd_weight_tfrag_group: 1..%d problems", DWS_MAX);
    for (int i = 0; i < n; ++i) REQUIRE(problems[i].dy && problems[i].x && problems[i].dw, "linear_bwd_weight_tfrag_group: null operand");
    PROF(ST_GEMM);
    DwsPlan P;
    REQUIRE(dw_stream_plan((const GemmTN*)problems, n, dw_stream_target(), &P), "linear_bwd_weight_tfrag_group: N must be a multiple of 64, K of 128, operands under 4 GB");
    float* part = P.part_floats ? lib_scratch(P.part_floats) : nullptr;
    REQUIRE(!P.part_floats || part, "linear_bwd_weight_tfrag_group: scratch allocation failed");
    REQUIRE(!dw_group_stream((const GemmTN*)problems, n, (hipStream_t)stream, part, dw_stream_target()), "linear_bwd_weight_tfrag_group: launch failed");
    CHECK_LAUNCH("linear_bwd_weight_tfrag_group");
    return 0;
}
int cffm_linear_bwd_weight_tfrag(const float* dy_t, const float* x_t, float* dw, long M, int N, int K, void* stream) {
    const cffm_wgrad pr = {dy_t, x_t, dw, M, N, K};
    return cffm_linear_bwd_weight_tfrag_group(&pr, 1, stream);
}

// q|k|v Linear feeding the CFM kernels: qkv16[M,768] (f16) = x w^T + b, q third times 32^-0.5 (cffm_transformer.py:374, :528)
int cffm_linear_qkv_fwd(const float* x, const float* w, const float* b, void* qkv16, long M, void* stream) {
    REQUIRE(x && w && b && qkv16, "linear_qkv_fwd: null");
    PROF(ST_GEMM);
    return gemm_nt_qkv16_split(x, w, b, (h16*)qkv16, M, 768, CFFM_C, (hipStream_t)stream) ? fail(-3, "linear_qkv_fwd: gemm failed") : 0;
}

int cffm_colsum(const float* a, long rows, int cols, float* out, void* stream) {
    ScratchFor pool(stream);
    PROF(ST_COLSUM);
    hipStream_t st = (hipStream_t)stream;
    REQUIRE(a && out && cols >= 4 && cols % 4 == 0, "colsum: cols must be a multiple of 4");
    const int slices = (int)((rows + COLSUM_ROWS - 1) / COLSUM_ROWS);
    float* part = red_scratch((size_t)slices * cols, st);
    REQUIRE(part, "colsum: scratch allocation failed");
    CFFM_LAUNCH(k_colsum_partial, (slices), (256), 0, st, a, rows, cols, part);
    RedSegs segs;
    segs.nseg = 0;
    seg_add(segs, 0, cols, out, 0);
    reduce_records(part, slices, cols, cols, segs, st);
    CHECK_LAUNCH("colsum");
    return 0;
}

// dx1 = (dres or 0) + LNbwd(dz2); dgamma / dbeta overwritten (zero_grads != 0) or accumulated into; the column sums of dres and of dx1
// (the bias gradients of the Linear layers on either side, or NULL) come for free
static int cffm_ln_bwd_residual(const float* x1, const float* mean, const float* rstd, const float* gamma, const float* dz2,
                                const float* dres, float* dx1, float* dgamma, float* dbeta, long nrows, int zero_grads,
                                float* dres_colsum, float* dx1_colsum, void* stream) {
    PROF(ST_LN_BWD);
    hipStream_t st = (hipStream_t)stream;
    const int rpb = LNB_ROWS;
    const int nblk = (int)((nrows + rpb - 1) / rpb);
    float* part = red_scratch((size_t)nblk * 1024, st);
    REQUIRE(part, "ln_bwd_residual: scratch allocation failed");
    CFFM_LAUNCH(k_ln_bwd_residual, (nblk), (256), 0, st, x1, mean, rstd, gamma, dz2, dres, dx1, part, nrows, rpb);
    RedSegs segs;
    segs.nseg = 0;
    seg_add(segs, 0, CFFM_C, dgamma, !zero_grads);
    seg_add(segs, CFFM_C, CFFM_C, dbeta, !zero_grads);
    seg_add(segs, 2 * CFFM_C, CFFM_C, dres_colsum, 0);
    seg_add(segs, 3 * CFFM_C, CFFM_C, dx1_colsum, 0);
    reduce_records(part, nblk, 1024, 1024, segs, st);
    CHECK_LAUNCH("ln_bwd_residual");
    return 0;
}


// ------------------------------------------------------------------------------------------- optimizer
int cffm_adamw_step_rows(const cffm_adamw_chunk2* chunks, int nchunks, const float* grad_base, float* state, const float* sched,
                         double* consts, int nrows, const int* active_rows, int* ticket, void* stream) {
    static_assert(sizeof(cffm_adamw_chunk2) == sizeof(AdamwChunk2), "chunk layout");
    if (nchunks <= 0) return 0;
    REQUIRE(chunks && state && sched && consts && nrows >= 1, "adamw_step_rows: null table or no rows");
    PROF(ST_ADAMW);
    if (ticket && nrows <= ADAMW_FUSED_ROWS) {      // (more rows than the one-launch kernel keeps in LDS: the two launches, same results)
        CFFM_LAUNCH(k_adamw_rows_tick, ((unsigned)((nchunks + ADAMW_WG_CHUNKS - 1) / ADAMW_WG_CHUNKS)), (256), 0, (hipStream_t)stream,
                    (const AdamwChunk2*)chunks, nchunks, grad_base, state, sched, consts, nrows, active_rows, ticket);
    } else {
        CFFM_LAUNCH(k_adamw_tick_rows, ((unsigned)((nrows + 63) / 64)), (64), 0, (hipStream_t)stream, state, sched, consts, nrows, active_rows);
        CFFM_LAUNCH(k_adamw_rows, ((unsigned)nchunks), (256), 0, (hipStream_t)stream, (const AdamwChunk2*)chunks, grad_base, (const float*)state, consts);
    }
    CHECK_LAUNCH("adamw_rows");
    return 0;
}

// ------------------------------------------------------------------------------------------- CFFM++ (GTC) stages
// the prototype attention on the matrix pipe for K <= 128 (gtc_kernels.h), fp32 on the VALU above
// workgroups the three matrix-pipe kernels aim for (a wave walks ceil(tiles / (4 x workgroups)) tiles)
#ifndef GTM_WGS_FWD
#define GTM_WGS_FWD 512
#endif
#ifndef GTM_WGS_DQ
#define GTM_WGS_DQ 512
#endif
#ifndef GTM_WGS_DKV
#define GTM_WGS_DKV 256
#endif
int cffm_gtc_attn_fwd(const float* q_raw, const float* q_b, const float* kv_raw, const float* kv_b, float* o, float* lse,
                      int B, int T, int K, void* stream) {
    PROF(ST_GTC_FWD);
    REQUIRE(K >= 1 && K <= 256, "gtc_attn_fwd: K=%d outside 1..256", K);
    static int lds_have = 0;
    REQUIRE(lds_grant(lds_have, {{(const void*)k_gtc_attn_fwd, gtf_lds(256)}}), "gtc_attn_fwd: LDS grant failed");
    if (K <= 128) {
        // the matrix-pipe form (three-pass bf16 split): ~512 workgroups of four waves, each wave a run of 16-token tiles
        const int tiles = (T + 15) / 16;
        int tpw = (tiles * CFFM_HEADS * B + 4 * GTM_WGS_FWD - 1) / (4 * GTM_WGS_FWD);
        if (tpw < 1) tpw = 1;
        const unsigned gx = (unsigned)((tiles + 4 * tpw - 1) / (4 * tpw));
        const int U = (K + 31) / 32;
        hipStream_t st = (hipStream_t)stream;
        f32x4* fr = (f32x4*)lib_scratch((size_t)B * CFFM_HEADS * gtm_frag_units(U) * 256);
        REQUIRE(fr, "gtc_attn_fwd: scratch allocation failed");
#define GTM_FWD(U_)                                                                                                                          \
        do {                                                                                                                             \
            if (U_ > 1) CFFM_LAUNCH(k_gtc_pack_frags<U_>, (CFFM_HEADS, B, 2 * U_), (256), 0, st, kv_raw, kv_b, fr, K);                   \
            CFFM_LAUNCH(k_gtc_attn_fwd_mfma<U_>, (gx, CFFM_HEADS, B), (256), 0, st, q_raw, q_b, (const f32x4*)(U_ > 1 ? fr : nullptr), kv_raw, kv_b, o, lse, T, K, tpw);   \
        } while (0)
        if (U == 1) GTM_FWD(1); else if (U == 2) GTM_FWD(2); else if (U == 3) GTM_FWD(3); else GTM_FWD(4);
#undef GTM_FWD
        CHECK_LAUNCH("gtc_attn_fwd");
        return 0;
    }
    CFFM_LAUNCH(k_gtc_attn_fwd, ((T + GTC_TOK - 1) / GTC_TOK, CFFM_HEADS, B), (256), (size_t)gtf_lds(K), (hipStream_t)stream, q_raw, q_b, kv_raw, kv_b, o,
                lse, T, K);
    CHECK_LAUNCH("gtc_attn_fwd");
    return 0;
}

int cffm_gtc_attn_bwd(const float* q_raw, const float* q_b, const float* kv_raw, const float* kv_b, const float* o,
                      const float* dout, const float* lse, float* dq_raw, float* dkv, int B, int T, int K, void* stream) {
    PROF(ST_GTC_BWD);
    hipStream_t st = (hipStream_t)stream;
    REQUIRE(K >= 1 && K <= 256 && B >= 1 && T >= 1, "gtc_attn_bwd: K=%d outside 1..256", K);
    if (K <= 128) {
        // the matrix-pipe form (gtc_kernels.h): dq per 16-token tile, then dKc / dVc per pair of tiles into one record per workgroup
        const int tiles = (T + 15) / 16, pairs = (T + 31) / 32, U = (K + 31) / 32;
        int tpw = (tiles * CFFM_HEADS * B + 4 * GTM_WGS_DQ - 1) / (4 * GTM_WGS_DQ), ppw = (pairs * CFFM_HEADS * B + 4 * GTM_WGS_DKV - 1) / (4 * GTM_WGS_DKV);
        if (tpw < 1) tpw = 1;
        if (ppw < 1) ppw = 1;
        const unsigned g1 = (unsigned)((tiles + 4 * tpw - 1) / (4 * tpw)), g2 = (unsigned)((pairs + 4 * ppw - 1) / (4 * ppw));
        const size_t nD = ((size_t)B * T * CFFM_HEADS + 63) / 64 * 64;
        const size_t nrecf = ((size_t)B * CFFM_HEADS * g2 * K * 64 + 63) / 64 * 64;
        float* scr = lib_scratch(nD + nrecf + (size_t)B * CFFM_HEADS * gtm_frag_units(U) * 256);
        REQUIRE(scr, "gtc_attn_bwd: scratch allocation failed");
        float* Dbuf = scr;
        float* rec = scr + nD;
        f32x4* fr = (f32x4*)(scr + nD + nrecf);
        static int lds_have_m = 0;
        REQUIRE(lds_grant(lds_have_m, {{(const void*)k_gtc_attn_bwd_dkv_mfma<3>, gtm_bwd_lds(4)}, {(const void*)k_gtc_attn_bwd_dkv_mfma<4>, gtm_bwd_lds(4)}}),
                "gtc_attn_bwd: LDS grant failed");
#define GTM_BWD(U_)                                                                                                                                              \
        do {                                                                                                                                                 \
            const f32x4* fq = U_ > 1 ? (const f32x4*)fr : nullptr;        /* U = 1: the kernels make their own copy (gtm_pack_local) */                        \
            if (U_ > 1) CFFM_LAUNCH(k_gtc_pack_frags<U_>, (CFFM_HEADS, B, 2 * U_), (256), 0, st, kv_raw, kv_b, fr, K);                                       \
            CFFM_LAUNCH(k_gtc_attn_bwd_dq_mfma<U_>, (g1, CFFM_HEADS, B), (256), (size_t)(8 * U_ * 1024), st, q_raw, q_b, fq, kv_raw, kv_b, dout, lse, dq_raw, Dbuf, T, K, tpw); \
            CFFM_LAUNCH(k_gtc_attn_bwd_dkv_mfma<U_>, (g2, CFFM_HEADS, B), (256), (size_t)gtm_bwd_lds(U_), st, q_raw, q_b, fq, kv_raw, kv_b, dout, lse, (const float*)Dbuf, rec, T, K, ppw); \
        } while (0)
        if (U == 1) GTM_BWD(1); else if (U == 2) GTM_BWD(2); else if (U == 3) GTM_BWD(3); else GTM_BWD(4);
        (void)o;
#undef GTM_BWD
        CFFM_LAUNCH(k_gtc_dkv_sum, (K, CFFM_HEADS, B), (64), 0, st, (const float*)rec, (int)g2, K, dkv);
        CHECK_LAUNCH("gtc_attn_bwd");
        return 0;
    }
    const int per = gtb_tok(K) * GTB_CHUNKS, nwg = (T + per - 1) / per;
    float* rec = lib_scratch((size_t)B * CFFM_HEADS * nwg * K * 64);       // one [K][64] record per workgroup: k_gtc_dkv_sum adds them in order
    REQUIRE(rec, "gtc_attn_bwd: scratch allocation failed");
    static int lds_have = 0;
    REQUIRE(lds_grant(lds_have, {{(const void*)k_gtc_attn_bwd, 160 * 1024}}), "gtc_attn_bwd: LDS grant failed");
    CFFM_LAUNCH(k_gtc_attn_bwd, (nwg, CFFM_HEADS, B), (256), (size_t)gtb_lds(K), st, q_raw, q_b, kv_raw, kv_b, o, dout, lse, dq_raw, rec, T, K);
    CFFM_LAUNCH(k_gtc_dkv_sum, (K, CFFM_HEADS, B), (64), 0, st, (const float*)rec, nwg, K, dkv);
    CHECK_LAUNCH("gtc_attn_bwd");
    return 0;
}

// ------------------------------------------------------------------------------------------- fused row-panel stages
// The fused forward stores act = gelu(hraw + b1) for the fc2 weight gradient (re-applying bias + GELU to hraw while that GEMM stages its
// tiles writes 29.5 MB less per block but puts the GELU in its staging path: 0.8914 vs 0.8843 ms per step, means of three alternating runs)
#ifndef MLP_MT
#define MLP_MT 2
#endif
#define MLP_D 4
static int mlp_lds_grant() {
    static int lds_have = 0;
    return lds_grant(lds_have, {{(const void*)k_mlp_fwd<MLP_MT, MLP_D>, PNL_FUSED_LDS(MLP_MT)}, {(const void*)k_mlp_fwd<MLP_MT, MLP_D, false, true>, PNL_FUSED_LDS(MLP_MT)},
                                {(const void*)k_mlp_bwd<MLP_MT, MLP_D>, PNL_FUSED_LDS(MLP_MT)}, {(const void*)k_mlp_bwd<MLP_MT, MLP_D, true>, PNL_FUSED_LDS_NCHW(MLP_MT)}}) ? 0 : -1;
}
// The q|k|v input gradient (and the prototype block's q projection) as row-panel GEMMs (weights in fragment order): rows per workgroup
// (32 or 48) chosen so that the grid wastes the least of its last round on 256 CUs
static int panel_mt(long M) {
    const long w2 = (M + 31) / 32, w3 = (M + 47) / 48;
    return ((w3 + 255) / 256) * 3 < ((w2 + 255) / 256) * 2 ? 3 : 2;
}
extern "C++" {
template <int MT, int NTW, bool A_PRE, int EPI>
static int panel_gemm_launch(const float* A, int lda, long M, int K, const float* wf, float* Cout, int ldc, const float* bias,
                             hipStream_t st, float* colrec = nullptr, float* a_t = nullptr) {
    auto kern = k_panel_gemm<MT, NTW, 2, 4, A_PRE, EPI>;
    static int lds_have = 0;
    if (!lds_grant(lds_have, {{(const void*)kern, PNL_LDS(MT)}})) return -1;
    CFFM_LAUNCH(kern, ((unsigned)((M + 16 * MT - 1) / (16 * MT))), (PNL_THREADS), PNL_LDS(MT), st, A, lda, (int)M, K, (const f32x4*)wf, Cout, ldc, bias, colrec, (f32x4*)a_t);
    return 0;
}
}  // extern "C++"
// qkv16[M][768] (f16) = f16((x W^T + b) [q third * 32^-0.5]), x in split-4 storage, W fragment-ordered (forward form)
// x_t (or NULL): T-frag copy of x for the streaming weight gradient.  One workgroup per (panel, column third), two resident per CU
// (k_panel_qkv3): rows per panel by the reasoning of panel_mt, on 512 slots and three workgroups per panel
static int panel_qkv_fwd_mt(long M) {
    const long w2 = 3 * ((M + 31) / 32), w3 = 3 * ((M + 47) / 48);
    return ((w3 + 511) / 512) * 3 < ((w2 + 511) / 512) * 2 ? 3 : 2;
}
extern "C++" {
template <int MT>
static int panel_qkv3_launch(const float* x_s, const float* wf, const float* b, h16* qkv16, long M, hipStream_t st, float* x_t) {
    const long panels = (M + 16 * MT - 1) / (16 * MT);
    CFFM_LAUNCH(k_panel_qkv3<MT>, ((unsigned)(24 * ((panels + 7) / 8))), (PNL_THREADS), QKV3_LDS(MT), st, x_s, (int)M, (const f32x4*)wf, b, qkv16, (f32x4*)x_t);
    return 0;
}
}  // extern "C++"
static int panel_qkv_fwd(const float* x_s, const float* wf, const float* b, h16* qkv16, long M, hipStream_t st, float* x_t = nullptr) {
    return panel_qkv_fwd_mt(M) == 3 ? panel_qkv3_launch<3>(x_s, wf, b, qkv16, M, st, x_t) : panel_qkv3_launch<2>(x_s, wf, b, qkv16, M, st, x_t);
}
// dx[M][256] = dqkv[M][768] W, W fragment-ordered (input-gradient form); colrec (or NULL): panel_qkv_records(M) records of 768
// column sums of dqkv (the q|k|v bias gradient before its reduction)
static long panel_qkv_records(long M) { return (M + 16 * panel_mt(M) - 1) / (16 * panel_mt(M)); }
// dqkv_t (or NULL): T-frag copy of dqkv for the streaming weight gradient
static int panel_qkv_dx(const float* dqkv, const float* wfn, float* dx, long M, hipStream_t st, float* colrec = nullptr, float* dqkv_t = nullptr) {
    return panel_mt(M) == 3 ? panel_gemm_launch<3, 2, false, 0>(dqkv, 768, M, 768, wfn, dx, 256, nullptr, st, colrec, dqkv_t)
                            : panel_gemm_launch<2, 2, false, 0>(dqkv, 768, M, 768, wfn, dx, 256, nullptr, st, colrec, dqkv_t);
}
// (the q|k|v Linear as row panels against the tiled GEMMs: 0.8729 vs 0.8843 ms per step, means of three alternating runs)
// The block's four weight gradients take one of two forms: the streaming kernel (dws_kernels.h) on operands in T-frag storage, written
// by the row-panel kernels that have them in LDS anyway, or the LDS-staged group on split-4 / fp32 operands (CFFM_DW_STREAM_DEFAULT 0).
#ifndef CFFM_DW_STREAM_DEFAULT
#define CFFM_DW_STREAM_DEFAULT 0
#endif
static int g_dw_stream = CFFM_DW_STREAM_DEFAULT;
static int dw_stream_sw() { return g_dw_stream; }
// Process-wide choice between the two forms of the block's weight gradients (both tested): 1 = streaming kernel on T-frag operands, 0 = the
// LDS-staged group.  The forward leaves the operands in the form the backward will read: do not change it between a forward and its backward.
int cffm_dw_stream(int on) { const int was = g_dw_stream; if (on >= 0) g_dw_stream = on != 0; return was; }

static long cffm_mlp_records(long NP) { return (NP + 16 * MLP_MT - 1) / (16 * MLP_MT); }

int cffm_panel_pack_weight(const float* w, int N, int K, int form, float* w_frag, void* stream) {
    REQUIRE(w && w_frag && N >= 16 && K >= 16 && N % 32 == 0 && K % 32 == 0 && (form == 0 || form == 1), "panel_pack_weight: bad arguments");
    CFFM_LAUNCH(k_pnl_pack_weight, ((unsigned)(((long)N * K / 8 + 255) / 256)), (256), 0, (hipStream_t)stream, w, N, K, form, (f32x4*)w_frag);
    CHECK_LAUNCH("panel_pack_weight");
    return 0;
}

// the q|k|v Linear of the block as a stage (k_panel_qkv3): x in split-4 storage, w_frag = cffm_panel_pack_weight(w [768][256], form 0)
int cffm_panel_qkv_fwd(const float* x_split4, const float* w_frag, const float* b, void* qkv16, long M, float* x_t, void* stream) {
    REQUIRE(x_split4 && w_frag && b && qkv16 && M >= 1 && M < (1L << 21), "panel_qkv_fwd: bad arguments");
    PROF(ST_GEMM);
    REQUIRE(!panel_qkv_fwd(x_split4, w_frag, b, (h16*)qkv16, M, (hipStream_t)stream, x_t), "panel_qkv_fwd: launch failed");
    CHECK_LAUNCH("panel_qkv_fwd");
    return 0;
}

// the q|k|v input gradient of the block as a stage (k_panel_gemm, K = 768): w_frag = cffm_panel_pack_weight(w [768][256], form 1)
int cffm_panel_qkv_bwd_input(const float* dqkv, const float* w_frag, float* dx, float* db, float* dqkv_t, long M, void* stream) {
    REQUIRE(dqkv && w_frag && dx && M >= 1 && M < (1L << 21), "panel_qkv_bwd_input: bad arguments");
    hipStream_t st = (hipStream_t)stream;
    float* rec = nullptr;
    const long nrec = panel_qkv_records(M);
    if (db) {
        rec = red_scratch((size_t)nrec * 768, st);
        REQUIRE(rec, "panel_qkv_bwd_input: scratch allocation failed");
    }
    {
        PROF(ST_GEMM); PROF2(ST_G_QKV_DX);
        REQUIRE(!panel_qkv_dx(dqkv, w_frag, dx, M, st, rec, dqkv_t), "panel_qkv_bwd_input: launch failed");
        CHECK_LAUNCH("panel_qkv_bwd_input");
    }
    if (db) {    // the q|k|v bias gradient: the column sums of dqkv, out of the records of the launch above
        RedSegs segs;
        segs.nseg = 0;
        seg_add(segs, 0, 768, db, 0);
        reduce_records(rec, (int)nrec, 768, 768, segs, st);
        CHECK_LAUNCH("panel_qkv_bwd_input reduction");
    }
    return 0;
}

// z2s / acts: split-4 copies (what the LDS-staged weight-gradient kernels read), ao_t / z2_t / act_t: T-frag copies (what the streaming one
// reads, cffm_tfrag_floats(NP, 256 | 256 | 1024) floats each); every one of the five may be NULL.
// x2_nchw (with x2 NULL): x2 leaves as NCHW images of rows_per_batch pixels, x2_bs floats apart, instead of as rows (k_mlp_fwd's NCHW form)
static int cffm_mlp_fwd_tfrag(const float* ao, const float* xt, long xt_bs, int rows_per_batch, const float* wp_f, const float* w1_f, const float* w2_f,
                              const float* bp, const float* b1, const float* b2, const float* g2, const float* be2, float* x1, float* z2s, float* mean2,
                              float* rstd2, float* hraw, float* acts, float* x2, float* ao_t, float* z2_t, float* act_t, long NP, void* stream,
                              float* x2_nchw = nullptr, long x2_bs = 0) {
    REQUIRE(NP >= 0 && NP < (1L << 21) && rows_per_batch >= 1, "mlp_fwd: bad sizes");
    if (!NP) return 0;
    REQUIRE(ao && xt && wp_f && w1_f && w2_f && bp && b1 && b2 && g2 && be2 && x1 && mean2 && rstd2 && hraw && (x2 || x2_nchw), "mlp_fwd: null");
    REQUIRE(!x2_nchw || (!x2 && x2_bs >= 256L * rows_per_batch), "mlp_fwd: bad NCHW destination");
    REQUIRE(!mlp_lds_grant(), "mlp_fwd: LDS grant failed");
    PROF2(ST_MLP_FWD);
    MlpFwdArgs a;
    a.ao = ao; a.xt = xt; a.xt_bs = xt_bs; a.rows_per_batch = rows_per_batch;
    a.wp = (const f32x4*)wp_f; a.w1 = (const f32x4*)w1_f; a.w2 = (const f32x4*)w2_f;
    a.bp = bp; a.b1 = b1; a.b2 = b2; a.g2 = g2; a.be2 = be2;
    a.x1 = x1; a.z2s = z2s; a.mean2 = mean2; a.rstd2 = rstd2; a.hraw = hraw; a.acts = acts; a.x2 = x2; a.NP = (int)NP;
    a.ao_t = (f32x4*)ao_t; a.z2_t = (f32x4*)z2_t; a.act_t = (f32x4*)act_t;
    a.x2_nchw = x2_nchw; a.x2_bs = x2_bs;
    if (x2_nchw) {
        CFFM_LAUNCH((k_mlp_fwd<MLP_MT, MLP_D, false, true>), ((unsigned)cffm_mlp_records(NP)), (PNL_THREADS), PNL_FUSED_LDS(MLP_MT), (hipStream_t)stream, a);
    } else {
        CFFM_LAUNCH((k_mlp_fwd<MLP_MT, MLP_D>), ((unsigned)cffm_mlp_records(NP)), (PNL_THREADS), PNL_FUSED_LDS(MLP_MT), (hipStream_t)stream, a);
    }
    CHECK_LAUNCH("mlp_fwd");
    return 0;
}
int cffm_mlp_fwd(const float* ao, const float* xt, long xt_bs, int rows_per_batch, const float* wp_f, const float* w1_f, const float* w2_f,
                 const float* bp, const float* b1, const float* b2, const float* g2, const float* be2, float* x1, float* z2s, float* mean2,
                 float* rstd2, float* hraw, float* acts, float* x2, long NP, void* stream) {
    REQUIRE(z2s || !NP, "mlp_fwd: null");   // (acts may be NULL: not stored)
    return cffm_mlp_fwd_tfrag(ao, xt, xt_bs, rows_per_batch, wp_f, w1_f, w2_f, bp, b1, b2, g2, be2, x1, z2s, mean2, rstd2, hraw, acts, x2, nullptr, nullptr,
                              nullptr, NP, stream);
}
// cffm_mlp_fwd with x2 written as NCHW images: row m = pixel m % rows_per_batch of image m / rows_per_batch, images x2_bs floats apart
int cffm_mlp_fwd_nchw(const float* ao, const float* xt, long xt_bs, int rows_per_batch, const float* wp_f, const float* w1_f, const float* w2_f,
                      const float* bp, const float* b1, const float* b2, const float* g2, const float* be2, float* x1, float* z2s, float* mean2,
                      float* rstd2, float* hraw, float* acts, float* x2_nchw, long x2_bs, long NP, void* stream) {
    REQUIRE((z2s && x2_nchw) || !NP, "mlp_fwd_nchw: null");
    return cffm_mlp_fwd_tfrag(ao, xt, xt_bs, rows_per_batch, wp_f, w1_f, w2_f, bp, b1, b2, g2, be2, x1, z2s, mean2, rstd2, hraw, acts, nullptr, nullptr, nullptr,
                              nullptr, NP, stream, x2_nchw, x2_bs);
}

// dhs: split-4 copy of dh; dout_t / dh_t / dx1_t: T-frag copies of dout, dh, dx1 (cffm_tfrag_floats(NP, 256 | 1024 | 256) floats); each may be NULL.
// dy_nchw (with dout NULL): the gradient arrives as NCHW images of rows_per_batch pixels, dy_bs floats apart, and its rows [NP][256] are
// written to dout_rows (k_mlp_bwd's NCHW form)
static int cffm_mlp_bwd_tfrag(const float* dout, const float* hraw, const float* b1, const float* x1, const float* mean2, const float* rstd2,
                              const float* g2, const float* w2_n, const float* w1_n, const float* wp_n, float* dhs, float* dx1, float* dao, float* dg2,
                              float* dbe2, float* db1, float* db2, float* dbp, float* dout_t, float* dh_t, float* dx1_t, long NP, void* stream,
                              const float* dy_nchw = nullptr, long dy_bs = 0, int rows_per_batch = 0, float* dout_rows = nullptr) {
    REQUIRE(NP >= 0 && NP < (1L << 21), "mlp_bwd: bad sizes");
    if (!NP) return 0;
    REQUIRE((dout || dy_nchw) && hraw && b1 && x1 && mean2 && rstd2 && g2 && w2_n && w1_n && wp_n && dx1 && dao, "mlp_bwd: null");
    REQUIRE(!dy_nchw || (!dout && dout_rows && rows_per_batch >= 1 && dy_bs >= 256L * rows_per_batch), "mlp_bwd: bad NCHW source");
    REQUIRE(!mlp_lds_grant(), "mlp_bwd: LDS grant failed");
    PROF2(ST_MLP_BWD);
    hipStream_t st = (hipStream_t)stream;
    const int nrec = (int)cffm_mlp_records(NP);
    float* rec = red_scratch((size_t)nrec * 2048, st);
    REQUIRE(rec, "mlp_bwd: scratch allocation failed");
    MlpBwdArgs a;
    a.dout = dout; a.hraw = hraw; a.b1 = b1; a.x1 = x1; a.mean2 = mean2; a.rstd2 = rstd2; a.g2 = g2;
    a.w2n = (const f32x4*)w2_n; a.w1n = (const f32x4*)w1_n; a.wpn = (const f32x4*)wp_n;
    a.dhs = dhs; a.dx1 = dx1; a.dao = dao; a.rec_b1 = rec; a.rec_ln = rec + (size_t)nrec * 1024; a.NP = (int)NP;
    a.dout_t = (f32x4*)dout_t; a.dh_t = (f32x4*)dh_t; a.dx1_t = (f32x4*)dx1_t;
    a.dy_nchw = dy_nchw; a.dy_bs = dy_bs; a.pix = rows_per_batch; a.dout_rows = dout_rows;
    if (dy_nchw) {
        CFFM_LAUNCH((k_mlp_bwd<MLP_MT, MLP_D, true>), ((unsigned)nrec), (PNL_THREADS), PNL_FUSED_LDS_NCHW(MLP_MT), st, a);
    } else {
        CFFM_LAUNCH((k_mlp_bwd<MLP_MT, MLP_D>), ((unsigned)nrec), (PNL_THREADS), PNL_FUSED_LDS(MLP_MT), st, a);
    }
    RedSegs s1, s2;
    s1.nseg = 0;
    seg_add(s1, 0, CFFM_HID, db1, 0);
    reduce_records(a.rec_b1, nrec, CFFM_HID, CFFM_HID, s1, st);
    s2.nseg = 0;
    seg_add(s2, 0, CFFM_C, dg2, 0);
    seg_add(s2, CFFM_C, CFFM_C, dbe2, 0);
    seg_add(s2, 2 * CFFM_C, CFFM_C, db2, 0);
    seg_add(s2, 3 * CFFM_C, CFFM_C, dbp, 0);
    reduce_records(a.rec_ln, nrec, 1024, 1024, s2, st);
    CHECK_LAUNCH("mlp_bwd");
    return 0;
}
int cffm_mlp_bwd(const float* dout, const float* hraw, const float* b1, const float* x1, const float* mean2, const float* rstd2,
                 const float* g2, const float* w2_n, const float* w1_n, const float* wp_n, float* dhs, float* dx1, float* dao, float* dg2,
                 float* dbe2, float* db1, float* db2, float* dbp, long NP, void* stream) {
    REQUIRE(dhs || !NP, "mlp_bwd: null");
    return cffm_mlp_bwd_tfrag(dout, hraw, b1, x1, mean2, rstd2, g2, w2_n, w1_n, wp_n, dhs, dx1, dao, dg2, dbe2, db1, db2, dbp, nullptr, nullptr, nullptr, NP,
                              stream);
}
// cffm_mlp_bwd with the gradient read as NCHW images: row m = pixel m % rows_per_batch of image m / rows_per_batch, images dy_bs floats
// apart; its rows [NP][256] are written to dout_rows
int cffm_mlp_bwd_nchw(const float* dy_nchw, long dy_bs, int rows_per_batch, float* dout_rows, const float* hraw, const float* b1, const float* x1,
                      const float* mean2, const float* rstd2, const float* g2, const float* w2_n, const float* w1_n, const float* wp_n, float* dhs,
                      float* dx1, float* dao, float* dg2, float* dbe2, float* db1, float* db2, float* dbp, long NP, void* stream) {
    REQUIRE((dhs && dy_nchw) || !NP, "mlp_bwd_nchw: null");
    return cffm_mlp_bwd_tfrag(nullptr, hraw, b1, x1, mean2, rstd2, g2, w2_n, w1_n, wp_n, dhs, dx1, dao, dg2, dbe2, db1, db2, dbp, nullptr, nullptr, nullptr, NP,
                              stream, dy_nchw, dy_bs, rows_per_batch, dout_rows);
}

// ------------------------------------------------------------------------------------------- CFFM++ (GTC) block, fused (round 5)
// SwinTransformerBlock_cluster.forward (pvt/swin_transformer_2d.py:605-665) with shift 0 and only_use_cluster_center_as_context (:216):
//   z = LN1(x), cn = LN1(centers) (:619-622);  q = (z Wq^T + bq) 32^-0.5, q third of `qkv` only (:219-226);  [Kc|Vc] = cn Wkv^T + bkv
//   (:223-224);  o = softmax_K(q Kc^T) Vc (:232-257);  x1 = x + o Wpc^T + bpc (:258, :662);  x2 = x1 + fc2(GELU(fc1(LN2(x1)))) (:663).
// Round 1-4 sequenced ~13 forward / ~20 backward stage launches from Python (vss_cffm_amd/ops.py).  Now ONE entry point per
// direction, built from the base head's kernels: the q projection and its input gradient are row-panel GEMMs (k_panel_gemm), everything
// from proj_cluster to the block output is the fused Mlp launch of the base block (k_mlp_fwd / k_mlp_bwd: same shapes), the four large
// weight gradients are one streaming launch (k_dw_stream), every bias / norm gradient is a record reduction in one launch.
struct GtcWs {     // float offsets into the caller's workspace: what the forward keeps for the backward, then the backward's temporaries
    long z, mean1, rstd1, cn, cmean, crstd, qraw, kvraw, ao, lse, x1, z2, mean2, rstd2, hraw, act, wf, wn, z_t, ao_t, saved;
    long dh, dx1, dao, dq, dz, dkv, dcn, dout_t, dx1_t, dq_t, total;
};
// The block's four large weight gradients by the streaming kernel (dws_kernels.h) -- everything of this block runs on ONE stream, so what the
// kernel saves alone (51 -> 38 us) is saved in the step.  z2 / act / dh are then kept in T-frag storage only, z / ao / dout / dx1 / dq get
// T-frag copies from the row-panel kernels that stage them.
#define GTC_WFLOATS (2 * 256 * 256 + 2 * 1024 * 256)     // q third | proj_cluster | fc1 | fc2 in fragment order
static GtcWs gtc_ws_layout(long nt, long nk) {
    GtcWs w;
    long p = 0;
    w.z = p; p += up(nt * CFFM_C);
    w.mean1 = p; p += up(nt); w.rstd1 = p; p += up(nt);
    w.cn = p; p += up(nk * CFFM_C); w.cmean = p; p += up(nk); w.crstd = p; p += up(nk);
    w.qraw = p; p += up(nt * CFFM_C); w.kvraw = p; p += up(nk * 512);
    w.ao = p; p += up(nt * CFFM_C); w.lse = p; p += up(nt * CFFM_HEADS);
    const long nt32 = (nt + 31) / 32 * 32;      // T-frag storage pads the token rows to whole k-steps of 32
    w.x1 = p; p += up(nt * CFFM_C); w.z2 = p; p += up(nt32 * CFFM_C); w.mean2 = p; p += up(nt); w.rstd2 = p; p += up(nt);
    w.hraw = p; p += up(nt * CFFM_HID); w.act = p; p += up(nt32 * CFFM_HID);
    w.wf = p; p += up(GTC_WFLOATS); w.wn = p; p += up(GTC_WFLOATS);
    w.z_t = p; p += up(nt32 * CFFM_C); w.ao_t = p; p += up(nt32 * CFFM_C);
    w.saved = p;
    w.dh = p; p += up(nt32 * CFFM_HID);
    w.dx1 = p; p += up(nt * CFFM_C); w.dao = p; p += up(nt * CFFM_C); w.dq = p; p += up(nt * CFFM_C); w.dz = p; p += up(nt * CFFM_C);
    w.dkv = p; p += up(nk * 512); w.dcn = p; p += up(nk * CFFM_C);
    w.dout_t = p; p += up(nt32 * CFFM_C); w.dx1_t = p; p += up(nt32 * CFFM_C); w.dq_t = p; p += up(nt32 * CFFM_C);
    w.total = p;
    return w;
}
long cffm_gtc_ws_floats(int B, int T, int K) { return (B < 1 || T < 1 || K < 1) ? -1 : gtc_ws_layout((long)B * T, (long)B * K).total; }

static int gtc_pack(const cffm_gtc_params* p, float* wfrag, int form, void* stream) {
    PnlPackJobs J;
    const float* w[4] = {p->qkv_w /* rows 0..255 of qkv.weight: the q third */, p->proj_w, p->fc1_w, p->fc2_w};
    const int N[4] = {256, 256, CFFM_HID, 256}, K[4] = {256, 256, 256, CFFM_HID};
    const long off[4] = {0, 256 * 256, 2 * 256 * 256, 2 * 256 * 256 + CFFM_HID * 256};
    long end = 0;
    for (int j = 0; j < 4; ++j) {
        J.w[j] = w[j]; J.dst[j] = (f32x4*)(wfrag + off[j]); J.N[j] = N[j]; J.K[j] = K[j];
        end += ((long)N[j] * K[j] / 8 + 255) / 256 * 256;       // whole workgroups per weight
        J.end[j] = end;
    }
    J.n = 4; J.nn = form;
    CFFM_LAUNCH(k_pnl_pack_weights, ((unsigned)(end / 256)), (256), 0, (hipStream_t)stream, J);
    CHECK_LAUNCH("gtc weight pack");
    return 0;
}
static int gtc_check(const cffm_gtc_params* p, const void* a, const void* b, const void* c, const void* ws, int B, int T, int K, const char* who) {
    REQUIRE(p && a && b && c && ws && B >= 1 && T >= 1 && K >= 1 && K <= 256, "%s: bad arguments (1 <= K <= 256)", who);
    REQUIRE(p->norm1_w && p->norm1_b && p->qkv_w && p->qkv_b && p->kv_w && p->kv_b && p->proj_w && p->proj_b && p->norm2_w && p->norm2_b &&
            p->fc1_w && p->fc1_b && p->fc2_w && p->fc2_b, "%s: null parameter", who);
    return 0;
}
int cffm_gtc_block_forward(const cffm_gtc_params* p, const float* x, const float* centers, float* out, float* ws, int B, int T, int K,
                           void* stream) {
    TRY(gtc_check(p, x, centers, out, ws, B, T, K, "gtc_block_forward"));
    hipStream_t st = (hipStream_t)stream;
    const long nt = (long)B * T, nk = (long)B * K;
    const GtcWs W = gtc_ws_layout(nt, nk);
    float* wf = ws + W.wf;
    TRY(gtc_pack(p, wf, 0, stream));
    {
        PROF(ST_LN);
        CFFM_LAUNCH(k_layernorm, ((unsigned)((nt + 3) / 4)), (256), 0, st, x, p->norm1_w, p->norm1_b, ws + W.z, ws + W.mean1, ws + W.rstd1, nt, 1);
        CFFM_LAUNCH(k_layernorm, ((unsigned)((nk + 3) / 4)), (256), 0, st, centers, p->norm1_w, p->norm1_b, ws + W.cn, ws + W.cmean, ws + W.crstd, nk, 0);
        CHECK_LAUNCH("gtc layernorm");
    }
    {
        PROF(ST_GEMM);
        float* z_t = ws + W.z_t;
        const int rc = panel_mt(nt) == 3 ? panel_gemm_launch<3, 2, true, 0>(ws + W.z, 256, nt, 256, wf, ws + W.qraw, 256, nullptr, st, nullptr, z_t)
                                         : panel_gemm_launch<2, 2, true, 0>(ws + W.z, 256, nt, 256, wf, ws + W.qraw, 256, nullptr, st, nullptr, z_t);
        REQUIRE(!rc, "gtc_block_forward: q gemm failed");
        REQUIRE(!gemm_nt(ws + W.cn, p->kv_w, ws + W.kvraw, nk, 512, 256, st), "gtc_block_forward: kv gemm failed");
    }
    TRY(cffm_gtc_attn_fwd(ws + W.qraw, p->qkv_b, ws + W.kvraw, p->kv_b, ws + W.ao, ws + W.lse, B, T, K, stream));
    TRY(cffm_mlp_fwd_tfrag(ws + W.ao, x, 0, (int)nt, wf + 256 * 256, wf + 2 * 256 * 256, wf + 2 * 256 * 256 + CFFM_HID * 256, p->proj_b, p->fc1_b, p->fc2_b,
                           p->norm2_w, p->norm2_b, ws + W.x1, nullptr, ws + W.mean2, ws + W.rstd2, ws + W.hraw, nullptr, out, ws + W.ao_t, ws + W.z2,
                           ws + W.act, nt, stream));
    return 0;
}

// every gradient of cffm_gtc_grads is written (qkv_w / qkv_b: rows / entries >= 256 -- the unused k, v thirds, :216 -- are zeroed)
int cffm_gtc_block_backward(const cffm_gtc_params* p, const cffm_gtc_grads* g, const float* x, const float* centers, const float* dout,
                            float* dx, float* dcenters, float* ws, int B, int T, int K, void* stream) {
    TRY(gtc_check(p, x, centers, dout, ws, B, T, K, "gtc_block_backward"));
    REQUIRE(g && dx && dcenters && g->norm1_w && g->norm1_b && g->qkv_w && g->qkv_b && g->kv_w && g->kv_b && g->proj_w && g->proj_b && g->norm2_w &&
            g->norm2_b && g->fc1_w && g->fc1_b && g->fc2_w && g->fc2_b, "gtc_block_backward: null gradient");
    hipStream_t st = (hipStream_t)stream;
    const long nt = (long)B * T, nk = (long)B * K;
    const GtcWs W = gtc_ws_layout(nt, nk);
    float* wn = ws + W.wn;
    TRY(gtc_pack(p, wn, 1, stream));
    REQUIRE(hipMemsetAsync(g->qkv_w + 256 * 256, 0, sizeof(float) * 512 * 256, st) == hipSuccess &&
            hipMemsetAsync(g->qkv_b + 256, 0, sizeof(float) * 512, st) == hipSuccess, "gtc_block_backward: memset failed");
    RedScope reductions(st);      // the bias / norm record reductions below run as ONE launch (finish())
    // x2 = x1 + Mlp(LN2(x1)), x1 = x + o Wpc^T + bpc: the fused input-gradient chain of the base block
    TRY(cffm_mlp_bwd_tfrag(dout, ws + W.hraw, p->fc1_b, ws + W.x1, ws + W.mean2, ws + W.rstd2, p->norm2_w, wn + 2 * 256 * 256 + CFFM_HID * 256,
                           wn + 2 * 256 * 256, wn + 256 * 256, nullptr, ws + W.dx1, ws + W.dao, g->norm2_w, g->norm2_b, g->fc1_b, g->fc2_b, g->proj_b,
                           ws + W.dout_t, ws + W.dh, ws + W.dx1_t, nt, stream));
    TRY(cffm_gtc_attn_bwd(ws + W.qraw, p->qkv_b, ws + W.kvraw, p->kv_b, ws + W.ao, ws + W.dao, ws + W.lse, ws + W.dq, ws + W.dkv, B, T, K, stream));
    {
        // dz = dq Wq (row panels; the q bias gradient = column sums of dq out of the staging registers)
        PROF(ST_GEMM);
        const int mt = panel_mt(nt);
        const long nrec = (nt + 16 * mt - 1) / (16 * mt);
        float* qrec = red_scratch((size_t)nrec * 256, st);
        REQUIRE(qrec, "gtc_block_backward: scratch allocation failed");
        float* dq_t = ws + W.dq_t;
        const int rc = mt == 3 ? panel_gemm_launch<3, 2, false, 0>(ws + W.dq, 256, nt, 256, wn, ws + W.dz, 256, nullptr, st, qrec, dq_t)
                               : panel_gemm_launch<2, 2, false, 0>(ws + W.dq, 256, nt, 256, wn, ws + W.dz, 256, nullptr, st, qrec, dq_t);
        REQUIRE(!rc, "gtc_block_backward: q input-gradient gemm failed");
        RedSegs segs;
        segs.nseg = 0;
        seg_add(segs, 0, 256, g->qkv_b, 0);
        reduce_records(qrec, (int)nrec, 256, 256, segs, st);
    }
    {
        // the four large weight gradients in one streaming launch (operands in T-frag storage)
        PROF(ST_GEMM); PROF2(ST_G_DW);
        const cffm_wgrad wt4[4] = {{ws + W.dq_t, ws + W.z_t, g->qkv_w, nt, 256, 256}, {ws + W.dh, ws + W.z2, g->fc1_w, nt, CFFM_HID, 256},
                                   {ws + W.dout_t, ws + W.act, g->fc2_w, nt, 256, CFFM_HID}, {ws + W.dx1_t, ws + W.ao_t, g->proj_w, nt, 256, 256}};
        DwsPlan P;
        REQUIRE(dw_stream_plan((const GemmTN*)wt4, 4, dw_stream_target(), &P), "gtc_block_backward: weight-gradient plan failed");
        float* part = P.part_floats ? lib_scratch(P.part_floats) : nullptr;
        REQUIRE(!P.part_floats || part, "gtc_block_backward: scratch allocation failed");
        // (on the library's side stream, beside the prototype side's chain of small launches below: measured 0.268 vs 0.262 ms at K = 8, 0.296 vs
        //  0.293 at K = 100 -- the fork and the join cost a replayed graph more than the overlap returns; it stays on the caller's stream)
        REQUIRE(!dw_group_stream((const GemmTN*)wt4, 4, st, part, dw_stream_target()), "gtc_block_backward: weight-gradient gemm failed");
    }
    // the prototype side: [Kc|Vc] = cn Wkv^T + bkv on B*K rows
    TRY(cffm_colsum(ws + W.dkv, nk, 512, g->kv_b, stream));
    {
        PROF(ST_GEMM);
        REQUIRE(!gemm_tn(ws + W.dkv, ws + W.cn, g->kv_w, nk, 512, 256, st), "gtc_block_backward: kv weight-gradient gemm failed");
        REQUIRE(!gemm_nn(ws + W.dkv, p->kv_w, ws + W.dcn, nk, 512, 256, st), "gtc_block_backward: kv input-gradient gemm failed");
    }
    // LN1 backward of the tokens (+ the residual path dx1), then of the prototypes: the same norm1 (:622), so the second ACCUMULATES
    TRY(cffm_ln_bwd_residual(x, ws + W.mean1, ws + W.rstd1, p->norm1_w, ws + W.dz, ws + W.dx1, dx, g->norm1_w, g->norm1_b, nt, 1, nullptr, nullptr, stream));
    reductions.finish();
    TRY(cffm_ln_bwd_residual(centers, ws + W.cmean, ws + W.crstd, p->norm1_w, ws + W.dcn, nullptr, dcenters, g->norm1_w, g->norm1_b, nk, 0, nullptr, nullptr,
                             stream));
    CHECK_LAUNCH("gtc_block_backward");
    return 0;
}

// ------------------------------------------------------------------------------------------- block
// bias tiles + pooling matrices of `n` blocks (workspaces ws0 + i*ws_stride) in ceil(n / PREP_MAXD) launches
static int prep_args(PrepArgs& a, const cffm_block_params* params, int d0, int nd, float* ws0, long ws_stride, const cffm_block_ws& L) {
    const int nb = (CFFM_HEADS * CFFM_NQ_PAD * CFFM_NKEY_PAD + 255) / 256;
    for (int d = 0; d < PREP_MAXD; ++d) {
        const cffm_block_params& p = params[d0 + (d < nd ? d : 0)];
        float* ws = ws0 + (long)(d0 + (d < nd ? d : 0)) * ws_stride;
        a.t[d].own = p.rpb_own; a.t[d].ring = p.rpb_ring;
        for (int i = 0; i < 4; ++i) { a.t[d].pool[i] = p.rpb_pool[i]; a.pw[d].w[i] = p.pool_w[i]; }
        a.bias[d] = ws + L.bias; a.M[d] = ws + L.M;
        a.w[d][0] = p.qkv_w; a.w[d][1] = p.proj_w; a.w[d][2] = p.fc1_w; a.w[d][3] = p.fc2_w;
        a.w_s[d] = ws + L.w_split;
        a.w_f[d] = ws + L.w_frag;
    }
    a.nbias = nb;
    // pack 2: the fragment-ordered weight copies only -- every Linear of the block runs as a row-panel kernel and nobody reads a split-4
    // copy (3 MB read + 3 MB written per block saved; k_param_prep also knows 0: nothing, 1: split-4 + fragment-ordered copies)
    a.pack = 2;
    return nb + 1 + PREP_WBLOCKS + PREP_FBLOCKS;      // workgroups per block
}
static int param_prep(const cffm_block_params* params, int n, float* ws0, long ws_stride, const cffm_block_ws& L, void* stream) {
    PROF(ST_BIAS_ASM);
    for (int d0 = 0; d0 < n; d0 += PREP_MAXD) {
        const int nd = (n - d0 < PREP_MAXD) ? n - d0 : PREP_MAXD;
        PrepArgs a;
        const int pnx = prep_args(a, params, d0, nd, ws0, ws_stride, L);
        CFFM_LAUNCH(k_param_prep, (pnx, nd), (256), 0, (hipStream_t)stream, a);
    }
    CHECK_LAUNCH("param_prep");
    return 0;
}

static int block_forward_impl(const cffm_geom* g, const cffm_block_params* p, const float* x_ref, long ref_bs,
                              const float* x_tgt, long tgt_bs, const int* key_src, const int* q_dst, float* ws,
                              float* scratch, void* stream, float* x2_rows = nullptr, float* x2_nchw = nullptr, long x2_bs = 0);
int cffm_block_forward(const cffm_geom* g, const cffm_block_params* p, const float* x_ref, long ref_bs,
                       const float* x_tgt, long tgt_bs, const int* key_src, const int* q_dst, float* ws,
                       float* scratch, void* stream) {
    REQUIRE(g && p && ws && scratch, "block_forward: null");
    cffm_block_ws L;
    cffm_block_ws_layout(g, &L);
    TRY(param_prep(p, 1, ws, 0, L, stream));
    return block_forward_impl(g, p, x_ref, ref_bs, x_tgt, tgt_bs, key_src, q_dst, ws, scratch, stream);
}
// the block after its parameter-only inputs (ws.bias, ws.biasT, ws.M) have been prepared
static struct { bool pending; hipStream_t side; } g_prep_join = {false, nullptr};
// The block's output rows go to ws + L.x2, or where the layer's last block is told to put them (its ws.x2 is then not written: nothing reads
// it): x2_rows = rows somewhere else, x2_nchw = NCHW images x2_bs floats apart (k_mlp_fwd's NCHW form)
static int block_forward_impl(const cffm_geom* g, const cffm_block_params* p, const float* x_ref, long ref_bs,
                              const float* x_tgt, long tgt_bs, const int* key_src, const int* q_dst, float* ws,
                              float* scratch, void* stream, float* x2_rows, float* x2_nchw, long x2_bs) {
    cffm_block_ws L;
    cffm_block_ws_layout(g, &L);
    const long NR = (long)g->B * g->RC, NP = (long)g->B * g->HW;
    hipStream_t st = (hipStream_t)stream;
    // zall is written in split-4 storage (only GEMMs read it; the fused kernels do the same for z2, act and dh)
    // (a pending join with the side-stream parameter prep -- layer_forward_impl -- is taken AFTER this launch: the kernel builds its
    //  pooling-matrix rows from the raw weights then, and the chain's first kernel does not wait for another stream)
    const bool late_join = g_prep_join.pending;
    TRY(ln_pool_fwd_impl(g, x_ref, ref_bs, x_tgt, tgt_bs, p->norm1_w, p->norm1_b, ws + L.M, p->pool_b, ws + L.zall,
                         ws + L.mean1, ws + L.rstd1, 1, stream, late_join ? p->pool_w : nullptr));
    if (late_join) {
        g_prep_join.pending = false;
        side_join(g_prep_join.side, st, 0);
    }
    {
        PROF(ST_GEMM); PROF2(ST_G_QKV_FWD);
        REQUIRE(!panel_qkv_fwd(ws + L.zall, ws + L.w_frag, p->qkv_b, (h16*)(ws + L.qkv), NR, st, dw_stream_sw() ? ws + L.zall_t : nullptr), "block_forward: qkv gemm failed");
    }
    TRY(cffm_attn_fwd(g, ws + L.qkv, key_src, q_dst, (const void*)(ws + L.bias), ws + L.ao, ws + L.lse, stream));
    {
        // proj + residual + norm2 + Mlp in one row-panel launch (panel_kernels.h); weights in fragment order from k_param_prep
        const float* wf = ws + L.w_frag;
        PROF(ST_GEMM);
        float* x2 = x2_nchw ? nullptr : x2_rows ? x2_rows : ws + L.x2;
        if (dw_stream_sw())     // z2 / act (and a copy of ao) in T-frag storage: operands of the streaming weight gradients
            TRY(cffm_mlp_fwd_tfrag(ws + L.ao, x_tgt, tgt_bs, g->HW, wf + 768 * 256, wf + 768 * 256 + 256 * 256, wf + 768 * 256 + 256 * 256 + 1024 * 256,
                                   p->proj_b, p->fc1_b, p->fc2_b, p->norm2_w, p->norm2_b, ws + L.x1, nullptr, ws + L.mean2, ws + L.rstd2, ws + L.hraw,
                                   nullptr, x2, ws + L.ao_t, ws + L.z2, ws + L.act, NP, stream, x2_nchw, x2_bs));
        else
        TRY(cffm_mlp_fwd_tfrag(ws + L.ao, x_tgt, tgt_bs, g->HW, wf + 768 * 256, wf + 768 * 256 + 256 * 256, wf + 768 * 256 + 256 * 256 + 1024 * 256,
                               p->proj_b, p->fc1_b, p->fc2_b, p->norm2_w, p->norm2_b, ws + L.x1, ws + L.z2, ws + L.mean2, ws + L.rstd2, ws + L.hraw,
                               ws + L.act, x2, nullptr, nullptr, nullptr, NP, stream, x2_nchw, x2_bs));
        CHECK_LAUNCH("block_forward");
    }
    (void)scratch;
    return 0;
}

static int block_backward_impl(const cffm_geom* g, const cffm_block_params* p, const cffm_block_grads* gr,
                               const float* x_ref, long ref_bs, const float* x_tgt, long tgt_bs, const int* key_src,
                               const int* q_dst, const int* inv_ptr, const int* inv_idx, const float* ws, const float* dout,
                               float* dx_tgt, long dtgt_bs, float* scratch, int defer, int par, int slot, int nslots, void* stream,
                               const float* dy_nchw = nullptr, long dy_bs = 0);
// The parameter-gradient tail of a block backward (record reductions, pooling-matrix backward), LAUNCHED LATE: its fork point is the end
// of ln_pool_bwd (event fork[3]), but the launches happen only after the chain's next kernel has been launched (tail_flush), so that
// under stream capture the chain's kernel is ln_pool_bwd's FIRST dependant and keeps its place on the graph's first stream (the graph
// executor hands every further dependant of a node the next stream, see side_fork_mark).
static struct { bool has; RedJobs jobs; int parity; } g_tail = {false, {}, 0};
// (the LAST block's tail of a layer backward is not launched here: the optimizer is what waits for those gradients, so they ride in the
// CFFA's final reduction launch on the caller's stream, in front of everything else that follows the last ln_pool_bwd -- layer_backward_impl)
static int tail_flush(hipStream_t st) {
    if (!g_tail.has) return 0;
    g_tail.has = false;
    hipStream_t s3 = side_fork_take(st, 3);
    // the tail waits for the weight-gradient stream's whole block (tail_order: the graph executor then queues it right behind the block's
    // side work; waiting for a single kernel of it, the tail was queued behind the NEXT block's side work)
    (void)hipStreamWaitEvent(s3, g_side.tail_order, 0);
    redq_launch(g_tail.jobs, s3);
    CHECK_LAUNCH("block_backward reductions");
    if (s3 != st) {
        side_record(s3, st, g_side.tail_done[g_tail.parity]);
        g_side.tail_pending[g_tail.parity] = true;
    }
    return 0;
}
static void tail_reset() {      // entry of a layer backward: nothing of a previous (failed) call is left to launch or to wait for
    g_tail.has = false;
    for (int i = 0; i < 2; ++i) g_side.dw_pending[i] = g_side.bias_pending[i] = g_side.tail_pending[i] = false;   // (a call that returned normally ended in side_join_all)
}
int cffm_block_backward(const cffm_geom* g, const cffm_block_params* p, const cffm_block_grads* gr,
                        const float* x_ref, long ref_bs, const float* x_tgt, long tgt_bs, const int* key_src,
                        const int* q_dst, const int* inv_ptr, const int* inv_idx, const float* ws, const float* dout,
                        float* dx_ref, long dref_bs, int accum_ref, float* dx_tgt, long dtgt_bs, float* scratch, void* stream) {
    REQUIRE(x_ref && dx_ref, "block_backward: null");
    TRY(block_backward_impl(g, p, gr, x_ref, ref_bs, x_tgt, tgt_bs, key_src, q_dst, inv_ptr, inv_idx, ws, dout, dx_tgt, dtgt_bs, scratch, 0, 0, 0, 1,
                            stream));
    return cffa_finish(g, 1, p, gr, 0, 0, ws, 0, x_ref, ref_bs, dx_ref, dref_bs, accum_ref, stream);
}
// `defer` (layer backward, round 3): the call returns with this block's parameter-gradient tail (partial-slab sums, record reductions,
// pooling-matrix backward, bias-table scatter) still running on the side streams; the caller's stream has only waited for what reads
// the scratch operands the NEXT block overwrites (the weight-gradient GEMMs).  The next block_backward_impl waits for the rest where
// it needs it; the caller ends the sequence with side_join_all().  (Measured on the round-3 timeline: the chain idled ~32 us per
// block between ln_pool_bwd and the next block's first kernel, behind four small side kernels.)
// dy_nchw (the layer's last block): the gradient of the block's output as NCHW images dy_bs floats apart; `dout` is then where the fused
// Mlp kernel WRITES its rows (a buffer of `scratch`), for the fc2 weight gradient
static int block_backward_impl(const cffm_geom* g, const cffm_block_params* p, const cffm_block_grads* gr,
                               const float* x_ref, long ref_bs, const float* x_tgt, long tgt_bs, const int* key_src,
                               const int* q_dst, const int* inv_ptr, const int* inv_idx, const float* ws, const float* dout,
                               float* dx_tgt, long dtgt_bs, float* scratch, int defer, int par, int slot, int nslots, void* stream,
                               const float* dy_nchw, long dy_bs) {
    REQUIRE(g && p && gr && ws && dout && scratch, "block_backward: null");
    cffm_block_ws L;
    cffm_block_ws_layout(g, &L);
    const Scratch S = scratch_layout(g);
    const long NR = (long)g->B * g->RC, NP = (long)g->B * g->HW;
    par = (defer && par) ? 1 : 0;
    const long altb = S.alt, altact = altb + up(NP * CFFM_C), altqkv = altact + up((NP + 31) / 32 * 32 * CFFM_HID), altbias = altqkv + up(NR * 768);
    float* dx1 = scratch + (par ? altb : S.b);
    float* dz2 = scratch + S.dz2;
    float* dao = scratch + S.dao;
    float* dact = scratch + (par ? altact : S.dact);
    float* dqkv = scratch + (par ? altqkv : S.dqkv);
    // T-frag copies of dout | dx1 | dqkv (streaming weight gradients), one set per parity
    const long NP32 = (NP + 31) / 32 * 32;
    float* dout_t = scratch + S.tf + (par ? S.tf_stride : 0);
    float* dx1_t = dout_t + up(NP32 * CFFM_C);
    float* dqkv_t = dx1_t + up(NP32 * CFFM_C);
    const int stream_dw = dw_stream_sw();
    CffaSlot cffa;           // library-owned: this block's dzall lives until the reference pass at the end of the range (cffa_finish)
    TRY(cffa_slot(g, slot, nslots, &cffa));
    float* dzall = cffa.dzall;
    float* dbiasT = scratch + (par ? altbias : S.dbiasT);
    RedScope reductions((hipStream_t)stream);   // the four parameter-gradient reductions below run as one launch (finish())
    hipStream_t st = (hipStream_t)stream;
    hipStream_t sa = st;
    side_init(st);
    if (g_side.tail_pending[g_red_parity]) {    // the reduction that last read this scope's record buffer (two blocks ago)
        side_wait(st, g_side.tail_done[g_red_parity]);
        g_side.tail_pending[g_red_parity] = false;
    }
    g_side.par = par;
    if (g_side.dw_pending[par]) {               // the weight-gradient group that last read this scratch set (two blocks ago)
        side_wait(st, g_side.dw_done[par]);
        g_side.dw_pending[par] = false;
    }
    const int one_group = dw_one_group(st);
    if (!one_group) {
        // the grouped form (chosen under stream capture) needs larger partial slabs than the split form: size the side scratch for it
        // now, while allocating is still allowed -- a capture that follows eager steps must not grow it
        const GemmTN all4[4] = {{nullptr, nullptr, nullptr, NR, 768, CFFM_C}, {nullptr, nullptr, nullptr, NP, CFFM_HID, CFFM_C},
                                {nullptr, nullptr, nullptr, NP, CFFM_C, CFFM_HID}, {nullptr, nullptr, nullptr, NP, CFFM_C, CFFM_C}};
        size_t need = gemm_tn_group_partial_floats(all4, 4, 480);
        DwsPlan P4;
        if (stream_dw && dw_stream_plan(all4, 4, dw_stream_target(), &P4)) need = P4.part_floats;
        REQUIRE(!need || lib_scratch2(need), "block_backward: scratch allocation failed");
    }
    // a group of the block's weight gradients: the streaming kernel on T-frag operands (default), or the LDS-staged group
    auto dw_group = [&](const cffm_wgrad* wg, const GemmTNPre* pre, int n, hipStream_t s, int target, void (*after)(hipStream_t)) -> int {
        if (!stream_dw) return gemm_tn_group((const GemmTN*)wg, n, s, pre, s == st ? lib_scratch : lib_scratch2, target, after);
        DwsPlan P;
        if (!dw_stream_plan((const GemmTN*)wg, n, dw_stream_target(), &P)) return -1;
        float* part = P.part_floats ? (s == st ? lib_scratch : lib_scratch2)(P.part_floats) : nullptr;
        if (P.part_floats && !part) return -1;
        return dw_group_stream((const GemmTN*)wg, n, s, part, dw_stream_target(), after);
    };
    // the four problems' operands: T-frag copies (streaming) or the split-4 / fp32 tensors themselves
    const cffm_wgrad wg_qkv = {stream_dw ? dqkv_t : dqkv, stream_dw ? ws + L.zall_t : ws + L.zall, gr->qkv_w, NR, 768, CFFM_C};
    const cffm_wgrad wg_fc1 = {dact, ws + L.z2, gr->fc1_w, NP, CFFM_HID, CFFM_C};
    const cffm_wgrad wg_fc2 = {stream_dw ? dout_t : dout, ws + L.act, gr->fc2_w, NP, CFFM_C, CFFM_HID};
    const cffm_wgrad wg_proj = {stream_dw ? dx1_t : dx1, stream_dw ? ws + L.ao_t : ws + L.ao, gr->proj_w, NP, CFFM_C, CFFM_C};
    // x2 = x1 + act W2^T + b2
    // act = gelu(hraw + b1); hraw = z2 W1^T: the GELU backward runs in the epilogue of the fc2 input-gradient GEMM (dact is
    // never materialised; what is stored is dh, in split-4 storage since only GEMMs read it, plus column-sum records of it)
    {
        // the input-gradient chain fc2 -> GELU' -> fc1 -> norm2 -> proj in one row-panel launch; dh (split-4), dx1 and the bias / norm
        // gradient records come out of it for the weight-gradient groups and the reductions below
        const float* wfn = ws + L.w_frag + PREP_WFLOATS;
        PROF(ST_GEMM);
        const float* dout_in = dy_nchw ? nullptr : dout;
        float* dout_rows = dy_nchw ? (float*)dout : nullptr;
        if (stream_dw)
            TRY(cffm_mlp_bwd_tfrag(dout_in, ws + L.hraw, p->fc1_b, ws + L.x1, ws + L.mean2, ws + L.rstd2, p->norm2_w, wfn + 768 * 256 + 256 * 256 + 1024 * 256,
                                   wfn + 768 * 256 + 256 * 256, wfn + 768 * 256, nullptr, dx1, dao, gr->norm2_w, gr->norm2_b, gr->fc1_b, gr->fc2_b, gr->proj_b,
                                   dout_t, dact, dx1_t, NP, stream, dy_nchw, dy_bs, g->HW, dout_rows));
        else
        TRY(cffm_mlp_bwd_tfrag(dout_in, ws + L.hraw, p->fc1_b, ws + L.x1, ws + L.mean2, ws + L.rstd2, p->norm2_w, wfn + 768 * 256 + 256 * 256 + 1024 * 256,
                               wfn + 768 * 256 + 256 * 256, wfn + 768 * 256, dact, dx1, dao, gr->norm2_w, gr->norm2_b, gr->fc1_b, gr->fc2_b, gr->proj_b,
                               nullptr, nullptr, nullptr, NP, stream, dy_nchw, dy_bs, g->HW, dout_rows));
        TRY(tail_flush(st));    // the previous block's parameter-gradient tail, now that this block's first kernel is ln_pool_bwd's first dependant
        if (!one_group) {
            sa = side_fork(st, 0);
            void* stream_a = (void*)sa;
            const cffm_wgrad wga[2] = {wg_fc1, wg_fc2};
            const GemmTNPre prea[2] = {{1, 1, nullptr}, {0, 1, p->fc1_b}};
            {
                void* stream = stream_a;
                PROF2(ST_G_DW);
                REQUIRE(!dw_group(wga, prea, 2, sa, 320, nullptr), "block_backward: weight-gradient gemm failed");
            }
            side_mark(sa, st, 0);
        }
    }
    // attention: the fused kernel and the dK/dV gather stay on the chain; the bias-gradient tile sum and its scatter into the six
    // tables get no branch of their own: they follow the weight-gradient group on ITS stream (side_b), so the attention backward has
    // ONE dependant and the chain stays on its hardware queue
    hipStream_t sb = st, s1 = st;
    float* dbp;
    int ng;
    {
        PROF(ST_ATTN_BWD);
        if (g_side.bias_pending[par]) {   // the bias-gradient tile sum of two blocks ago still owns this set's tile buffer / dbiasT
            side_wait(st, g_side.bias_done[par]);
            g_side.bias_pending[par] = false;
        }
        TRY(attn_bwd_fused(g, ws + L.qkv, key_src, q_dst, (const h16*)(ws + L.bias), ws + L.ao, dao, ws + L.lse, dqkv, scratch + S.dkvp, &dbp, &ng, par, stream));
        TRY(attn_bwd_gather(g, inv_ptr, inv_idx, scratch + S.dkvp, dqkv, stream));
    }
    // q|k|v = zall Wqkv^T + b (bias folded into the f16 epilogue); its gradient = the column sums of dqkv, as records out of the
    // row-panel input-gradient GEMM, which stages every row of dqkv anyway
    const long nrec = panel_qkv_records(NR);
    float* qkv_rec = red_scratch((size_t)nrec * 768, st);
    REQUIRE(qkv_rec, "block_backward: scratch allocation failed");
    {
        RedSegs segs;
        segs.nseg = 0;
        seg_add(segs, 0, 768, gr->qkv_b, 0);
        reduce_records(qkv_rec, (int)nrec, 768, 768, segs, st);
    }
    {   // chain first: the q|k|v input gradient is launched before the side work
        // (streaming weight gradients: the side work forks BEHIND this kernel -- it leaves the T-frag copy of dqkv the q|k|v weight gradient reads)
        if (!stream_dw) side_fork_mark(st, 2);
        PROF(ST_GEMM); PROF2(ST_G_QKV_DX);
        REQUIRE(!panel_qkv_dx(dqkv, ws + L.w_frag + PREP_WFLOATS, dzall, NR, st, qkv_rec, stream_dw ? dqkv_t : nullptr), "block_backward: q|k|v input-gradient gemm failed");
        if (stream_dw) side_fork_mark(st, 2);
    }
    // the block's side work behind the q|k|v input gradient: the weight gradients, then the bias-gradient tiles on the same stream
    auto side_b = [&]() -> int {
        sb = side_fork_take(st, 2);
        void* stream_b = (void*)sb;
        if (one_group) {
            // ALL four weight gradients as one grouped launch (~480 workgroups with one slice length, one partial-sum launch: 59 us
            // where two groups of two take 2 x 53), on the side stream beside q|k|v's input gradient and the CFFA backward; every
            // operand lives until the end of the block now that ln_pool_bwd no longer writes over `dout`
            const cffm_wgrad wg4[4] = {wg_qkv, wg_fc1, wg_fc2, wg_proj};
            const GemmTNPre pre4[4] = {{0, 1, nullptr}, {1, 1, nullptr}, {0, 1, p->fc1_b}, {0, 0, nullptr}};
            void* stream = stream_b;
            PROF(ST_GEMM); PROF2(ST_G_DW);
            REQUIRE(!dw_group(wg4, pre4, 4, sb, 480, dw_group_launched), "block_backward: weight-gradient gemm failed");
            sa = sb;
            side_mark(sa, st, 0);
            {
                PROF(ST_ATTN_BWD);
                s1 = sb;
                TRY(attn_bwd_bias_sum(dbp, ng, dbiasT, (void*)s1));
                TRY(cffm_bias_scatter(dbiasT, gr->rpb_own, gr->rpb_ring, gr->rpb_pool, (void*)s1));
            }
        } else {
            const cffm_wgrad wgb[2] = {wg_qkv, wg_proj};
            const GemmTNPre preb[2] = {{0, 1, nullptr}, {0, 0, nullptr}};
            {
                void* stream = stream_b;
                PROF(ST_GEMM); PROF2(ST_G_DW);
                REQUIRE(!dw_group(wgb, preb, 2, sb, 320, dw_group_launched), "block_backward: weight-gradient gemm failed");
            }
            PROF(ST_ATTN_BWD);
            s1 = sb;
            TRY(attn_bwd_bias_sum(dbp, ng, dbiasT, (void*)s1));
            TRY(cffm_bias_scatter(dbiasT, gr->rpb_own, gr->rpb_ring, gr->rpb_pool, (void*)s1));
        }
        return 0;
    };
    // Streaming weight gradients under capture: the group is launched AFTER the chain's next kernel (ln_pool_bwd_tgt below), so that kernel
    // is the q|k|v input gradient's first-launched dependant and keeps the chain's hardware queue (see side_fork_mark); nothing the
    // group reads is written by it (fc2's weight gradient reads the T-frag copy of dout, not dout).
    const bool side_late = stream_dw && one_group;
    if (!side_late) TRY(side_b());
    if (!side_late && (!one_group || dx_tgt == dout)) side_join(sa, st, 0);    // fc2's weight gradient has read dout before an in-place ln_pool_bwd overwrites it
    if (g_side.dw_pending[par ^ 1] && g_side.dw_dout[par ^ 1] == dx_tgt) {   // (depth >= 3: the block before still reads its dout = our dx_tgt)
        side_wait(st, g_side.dw_done[par ^ 1]);
        g_side.dw_pending[par ^ 1] = false;
    }
    // CFFA, target frame: dx_tgt for the next block + this block's target records.  The reference frames of every block of the range
    // follow in ONE pass at its end (cffa_finish): they need this block's pooled-cell rows of dzall and nothing else.
    TRY(ln_pool_bwd_tgt(g, x_tgt, tgt_bs, p->norm1_w, p->norm1_b, ws + L.M, ws + L.mean1, ws + L.rstd1, dzall, dx1, dx_tgt, dtgt_bs, cffa.rec,
                        stream));
    if (side_late) TRY(side_b());
    // the record reductions (every block-partial record of this backward except the CFFA's is written by now):
    // parameter gradients only -> side stream (branch 3); the caller's stream then waits for the side stream once
    if (defer && sb != st && s1 != st && g_side.on) {
        if (g_tail.has) TRY(tail_flush(st));    // (an earlier block's tail nobody has launched yet: before its slot is reused)
        side_fork_mark(st, 3);
        if (s1 != sb) side_order(s1, sb);
        (void)hipEventRecord(g_side.tail_order, sb);
        g_tail.has = true; g_tail.jobs = g_rq.jobs; g_tail.parity = g_red_parity;
        g_rq.jobs.njob = 0; g_rq.active = false;
        g_side.dw_pending[par] = true;
        g_side.dw_dout[par] = dout;
        side_record(s1, st, g_side.bias_done[par]);
        g_side.bias_pending[par] = true;
        return 0;
    }
    hipStream_t s3 = side_fork(st, 3);
    if (sb != st && s3 != st) side_order(sb, s3);     // (behind the block's side work, as in tail_flush)
    if (s1 != st && s3 != st && s1 != s3) side_order(s1, s3);   // (four side streams: branch 1 joins through branch 3)
    reductions.finish_on(s3);
    CHECK_LAUNCH("block_backward reductions");
    if (defer && sb != st && s3 != st) {
        // (no wait for the weight-gradient GEMMs: the next block works in the other scratch set; whoever reuses THIS set, or writes
        //  the `dout` they read, waits for dw_done[par] then)
        g_side.dw_pending[par] = true;
        g_side.dw_dout[par] = dout;
        side_record(s1, st, g_side.bias_done[par]);
        g_side.bias_pending[par] = s1 != st;
        side_record(s3, st, g_side.tail_done[g_red_parity]);
        g_side.tail_pending[g_red_parity] = true;
        return 0;
    }
    side_mark(s3, st, 1);
    side_join(s3, st, 1);    // the caller's stream owns every gradient (and the scratch operands) again
    if (sb != st && sb != s3) { side_mark(sb, st, 0); side_join(sb, st, 0); }   // ... on both side streams
    return 0;
}

// ------------------------------------------------------------------------------------------- SegFormer embedding
static int segf_maps(SegfMaps& mp, const int* h, const int* w, int nmaps, int H, int W, const char* who) {
    if (nmaps < 0 || nmaps > 3 || H < 1 || W < 1) return fail(-1, "%s: bad map count / size", who);
    mp.cnt = nmaps;
    mp.nseg = 0; mp.per_frame = 0;
    for (int m = 0; m < 3; ++m) {
        mp.z[m] = nullptr; mp.dz[m] = nullptr; mp.h[m] = mp.w[m] = 1;
        if (m >= nmaps) continue;
        // the 2x2-patch forward assumes every tap of a patch lies in a 3x3 neighbourhood and the adjoint windows assume an
        // UPsampling map: a map larger than the output (or more than SEGF_MAX_RATIO times smaller) is rejected, not mis-resized
        if (h[m] < 1 || w[m] < 1 || h[m] > H || w[m] > W || (long)H > (long)SEGF_MAX_RATIO * h[m] || (long)W > (long)SEGF_MAX_RATIO * w[m])
            return fail(-1, "%s: map %d is %dx%d for a %dx%d output (only upsampling by factors 1..%d is supported)", who, m, h[m], w[m],
                        H, W, SEGF_MAX_RATIO);
        mp.h[m] = h[m]; mp.w[m] = w[m];
    }
    return 0;
}
// ---- composed embedding weights (ABI 10) --------------------------------------------------------------------------------------------
// A_i = Wf_i W_i for the k <= 4 scales (Wf_i = input-channel block k - 1 - i of linear_fuse.conv.weight [e][k e], read in place through
// its leading dimension; W_i = linear_c{i+1}.proj.weight [e][C_i]) and d = sum_i Wf_i b_i -- what ops.segformer_fuse feeds the per-scale
// embedding GEMMs (cffm_head.py:102-119 without the 1024-channel concat).  The k products are independent 10-MFLOP GEMMs: in the backward
// (2 k of them) each scale on its own branch; round 5 ran them from Python behind two layout copies of the fuse weight, with torch's
// cat / gemv / ger for the constant (97 us of a replayed head step, 120 us for the backward).
static void fuse_bias_ptrs(FuseBias& fb, const float* const* lin_b, float* const* dlin_b, int k) {
    for (int j = 0; j < 4; ++j) { fb.b[j] = j < k ? lin_b[k - 1 - j] : nullptr; fb.db[j] = (j < k && dlin_b) ? dlin_b[k - 1 - j] : nullptr; }
}
int cffm_fuse_compose_fwd(const float* fuse_w, const float* const* lin_w, const float* const* lin_b, const int* C_in, int k, int e,
                          float* const* mats, float* d, void* stream) {
    REQUIRE(fuse_w && lin_w && lin_b && C_in && mats && d && k >= 1 && k <= 4 && e >= 64 && e % 64 == 0, "fuse_compose_fwd: bad arguments");
    for (int i = 0; i < k; ++i) REQUIRE(lin_w[i] && lin_b[i] && mats[i] && C_in[i] >= 4 && C_in[i] % 4 == 0, "fuse_compose_fwd: bad scale %d", i);
    hipStream_t st = (hipStream_t)stream;
    FuseBias fb;
    fuse_bias_ptrs(fb, lin_b, nullptr, k);
    // (one behind the other: these are the first nodes of a replayed step, where starting a second hardware queue costs more -- ~11 us per
    // branch, profiles/r06_head_timeline_branches_first_version.txt -- than a 7 us GEMM)
    for (int i = 0; i < k; ++i) {
        // A_i [e][C_i] = Wf_i [e][e] (lda = k e) x W_i [e][C_i]
        if (gemm_split_launch<false, true>(fuse_w + (long)(k - 1 - i) * e, lin_w[i], mats[i], e, C_in[i], e, k * e, C_in[i], C_in[i], 1, st))
            return fail(-3, "fuse_compose_fwd: gemm failed");
    }
    CFFM_LAUNCH(k_fuse_const, ((e + 3) / 4), (256), 0, st, fuse_w, fb, k, e, d);
    CHECK_LAUNCH("fuse_compose_fwd");
    return 0;
}
// gradients of the nine tensors from dmats[i] [e][C_i] and dd [e]: dfuse_w [e][k e] (every element written), dlin_w[i] [e][C_i], dlin_b[i] [e]
int cffm_fuse_compose_bwd(const float* fuse_w, const float* const* lin_w, const float* const* lin_b, const int* C_in, int k, int e,
                          const float* const* dmats, const float* dd, float* dfuse_w, float* const* dlin_w, float* const* dlin_b, void* stream) {
    REQUIRE(fuse_w && lin_w && lin_b && C_in && dmats && dd && dfuse_w && dlin_w && dlin_b && k >= 1 && k <= 4 && e >= 64 && e % 64 == 0,
            "fuse_compose_bwd: bad arguments");
    for (int i = 0; i < k; ++i)
        REQUIRE(lin_w[i] && lin_b[i] && dmats[i] && dlin_w[i] && dlin_b[i] && C_in[i] >= 4 && C_in[i] % 4 == 0, "fuse_compose_bwd: bad scale %d", i);
    hipStream_t st = (hipStream_t)stream;
    cffm_branch_mark(stream);
    for (int i = 0; i < k; ++i) {          // (the caller's own chain first: see cffm_branch_mark)
        hipStream_t s = i ? (hipStream_t)cffm_branch_take(stream, i) : st;
        const float* wf = fuse_w + (long)(k - 1 - i) * e;
        // dWf_i [e][e] (ldc = k e) = dA_i [e][C_i] x W_i^T;  dW_i [e][C_i] = Wf_i^T x dA_i (one slice: no library scratch on a branch)
        if (gemm_split_launch<false, false>(dmats[i], lin_w[i], dfuse_w + (long)(k - 1 - i) * e, e, e, C_in[i], C_in[i], C_in[i], k * e, 1, s) ||
            gemm_split_launch<true, true>(wf, dmats[i], dlin_w[i], e, C_in[i], e, k * e, C_in[i], C_in[i], 1, s))
            return fail(-3, "fuse_compose_bwd: gemm failed");
    }
    cffm_branch_join(stream);
    FuseBias fb;
    fuse_bias_ptrs(fb, lin_b, dlin_b, k);
    CFFM_LAUNCH(k_fuse_const_bwd, (k * e / 64), (256), 0, st, fuse_w, dd, fb, k, e, dfuse_w);
    CHECK_LAUNCH("fuse_compose_bwd");
    return 0;
}
int cffm_segfuse_fwd(float* y, const float* d, const float* const z[3], const int h[3], const int w[3], int nmaps, int N, int H,
                     int W, void* stream) {
    REQUIRE(y && d && N >= 0 && (nmaps == 0 || (z && h && w)), "segfuse_fwd: bad arguments");
    SegfMaps mp;
    TRY(segf_maps(mp, h, w, nmaps, H, W, "segfuse_fwd"));
    for (int m = 0; m < nmaps; ++m) { REQUIRE(z[m], "segfuse_fwd: null map"); mp.z[m] = z[m]; }
    const long rows = (long)N * H * W;
    if (!rows) return 0;
    REQUIRE(rows < (1L << 31), "segfuse_fwd: too many output pixels");
    hipStream_t st = (hipStream_t)stream;
    const long patches = (long)N * ((H + 1) / 2) * ((W + 1) / 2);
    CFFM_LAUNCH(k_segfuse_fwd<false>, ((unsigned)((patches + 3) / 4)), (256), 0, st, y, d, mp, N, H, W, SegfNoPool());
    CHECK_LAUNCH("segfuse_fwd");
    return 0;
}
int cffm_segfuse_bwd(const float* g, float* const dz[3], const int h[3], const int w[3], int nmaps, int N, int H, int W,
                     void* stream) {
    REQUIRE(g && N >= 0 && nmaps >= 1 && dz && h && w, "segfuse_bwd: bad arguments");
    SegfMaps mp;
    TRY(segf_maps(mp, h, w, nmaps, H, W, "segfuse_bwd"));
    for (int m = 0; m < nmaps; ++m) { REQUIRE(dz[m], "segfuse_bwd: null map"); mp.dz[m] = dz[m]; }
    // bands of BR output rows (BR = the largest resize factor, at most SEGF_MAX_BANDS bands); a low-resolution row belongs to
    // the band its centre falls into
    int BR = 1;
    for (int m = 0; m < nmaps; ++m) BR = std::max(BR, (H + h[m] - 1) / h[m]);
    BR = std::max(BR, (H + SEGF_MAX_BANDS - 1) / SEGF_MAX_BANDS);
    const int nb = (H + BR - 1) / BR;
    long items = 0;
    int next_q[3] = {0, 0, 0};
    for (int b = 0; b < nb; ++b)
        for (int m = 0; m < nmaps; ++m) {
            const int q0 = next_q[m];
            int q = q0;
            while (q < h[m] && (b == nb - 1 || (int)(((double)q + 0.5) * H / h[m]) / BR <= b)) ++q;
            next_q[m] = q;
            items += (long)(q - q0) * ((w[m] + SEGF_XQ - 1) / SEGF_XQ);
            mp.seg_q0[b * nmaps + m] = q0;
            mp.seg_end[b * nmaps + m] = (int)items;
        }
    mp.nseg = nb * nmaps;
    mp.per_frame = (int)items;
    const long blocks = items * N;
    REQUIRE(blocks < (1L << 31), "segfuse_bwd: too many work items");
    if (!blocks) return 0;
    hipStream_t st = (hipStream_t)stream;
    CFFM_LAUNCH(k_segfuse_bwd, ((unsigned)blocks), (256), 0, st, g, mp, N, H, W);
    CHECK_LAUNCH("segfuse_bwd");
    return 0;
}
// [a, a + na) and [b, b + nb) floats share an address
static bool spans_overlap(const float* a, long na, const float* b, long nb) {
    const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
    return na > 0 && nb > 0 && a0 < b0 + (uintptr_t)nb * sizeof(float) && b0 < a0 + (uintptr_t)na * sizeof(float);
}
// the eval tail of a frame in one pass (k_segfuse_fwd<true>, "k_segfuse_pool_fwd"): y, d and the maps as for cffm_segfuse_fwd, but y is only
// read; the pooled rows go to slot clamp(slots[which]) of the ring
int cffm_segfuse_pool_fwd(const float* y, const float* d, const float* const z[3], const int h[3], const int w[3], int nmaps,
                          const float* scale, const float* shift, float* ring, long slot_floats, int nslots, const int* slots, int which,
                          int N, int H, int W, void* stream) {
    REQUIRE(y && d && scale && shift && ring && N >= 0 && (nmaps == 0 || (z && h && w)), "segfuse_pool_fwd: bad arguments (null pointer)");
    REQUIRE(H >= 2 && W >= 2 && H % 2 == 0 && W % 2 == 0, "segfuse_pool_fwd: even map sides expected, got %dx%d", H, W);
    SegfMaps mp;
    TRY(segf_maps(mp, h, w, nmaps, H, W, "segfuse_pool_fwd"));
    for (int m = 0; m < nmaps; ++m) { REQUIRE(z[m], "segfuse_pool_fwd: null map"); mp.z[m] = z[m]; }
    const long rows = (long)N * H * W, patches = rows / 4, out_floats = patches * SEGF_C;
    REQUIRE(rows < (1L << 31), "segfuse_pool_fwd: too many output pixels");
    REQUIRE(nslots >= 1 && slot_floats >= out_floats && slot_floats % 4 == 0, "segfuse_pool_fwd: %d slots of %ld floats for %ld floats of rows",
            nslots, slot_floats, out_floats);
    REQUIRE(which >= 0 && (slots ? which < 4 : which == 0), "segfuse_pool_fwd: table index %d", which);
    bool aligned = !(((uintptr_t)y | (uintptr_t)d | (uintptr_t)scale | (uintptr_t)shift | (uintptr_t)ring) & 15) && !((uintptr_t)slots & 3);
    for (int m = 0; m < nmaps; ++m) aligned = aligned && !((uintptr_t)z[m] & 15);
    REQUIRE(aligned, "segfuse_pool_fwd: pointers must be 16-byte aligned (the slot table: 4)");
    // the ring as a whole (any slot may be the one written) must not share memory with anything the launch reads
    const long ring_floats = (long)(nslots - 1) * slot_floats + out_floats;
    bool clash = spans_overlap(ring, ring_floats, y, rows * SEGF_C) || spans_overlap(ring, ring_floats, d, SEGF_C) ||
                 spans_overlap(ring, ring_floats, scale, SEGF_C) || spans_overlap(ring, ring_floats, shift, SEGF_C);
    for (int m = 0; m < nmaps; ++m) clash = clash || spans_overlap(ring, ring_floats, z[m], (long)N * h[m] * w[m] * SEGF_C);
    REQUIRE(!clash, "segfuse_pool_fwd: the ring overlaps an input");
    if (!patches) return 0;
    const SegfPool pa = {scale, shift, ring, slot_floats, nslots, slots, which};
    CFFM_LAUNCH(k_segfuse_fwd<true>, ((unsigned)((patches + 3) / 4)), (256), 0, (hipStream_t)stream, const_cast<float*>(y), d, mp, N, H, W, pa);
    CHECK_LAUNCH("segfuse_pool_fwd");
    return 0;
}
// the same with one slot per frame (k_segfuse_fwd<true, true>): frame n's rows go to slot clamp(slots[n]) of the ring, slots a device int[N]
int cffm_segfuse_pool_fwd_frames(const float* y, const float* d, const float* const z[3], const int h[3], const int w[3], int nmaps,
                                 const float* scale, const float* shift, float* ring, long slot_floats, int nslots, const int* slots, int N,
                                 int H, int W, void* stream) {
    REQUIRE(y && d && scale && shift && ring && slots && N >= 0 && (nmaps == 0 || (z && h && w)),
            "segfuse_pool_fwd_frames: bad arguments (null pointer)");
    REQUIRE(H >= 2 && W >= 2 && H % 2 == 0 && W % 2 == 0, "segfuse_pool_fwd_frames: even map sides expected, got %dx%d", H, W);
    SegfMaps mp;
    TRY(segf_maps(mp, h, w, nmaps, H, W, "segfuse_pool_fwd_frames"));
    for (int m = 0; m < nmaps; ++m) { REQUIRE(z[m], "segfuse_pool_fwd_frames: null map"); mp.z[m] = z[m]; }
    const long rows = (long)N * H * W, patches = rows / 4, frame_floats = (long)(H / 2) * (W / 2) * SEGF_C;
    REQUIRE(rows < (1L << 31), "segfuse_pool_fwd_frames: too many output pixels");
    REQUIRE(nslots >= 1 && slot_floats >= frame_floats && slot_floats % 4 == 0,
            "segfuse_pool_fwd_frames: %d slots of %ld floats for frames of %ld floats of rows", nslots, slot_floats, frame_floats);
    bool aligned = !(((uintptr_t)y | (uintptr_t)d | (uintptr_t)scale | (uintptr_t)shift | (uintptr_t)ring) & 15) && !((uintptr_t)slots & 3);
    for (int m = 0; m < nmaps; ++m) aligned = aligned && !((uintptr_t)z[m] & 15);
    REQUIRE(aligned, "segfuse_pool_fwd_frames: pointers must be 16-byte aligned (the slot table: 4)");
    // the ring as a whole (any slot may be written) must not share memory with anything the launch reads
    const long ring_floats = (long)(nslots - 1) * slot_floats + frame_floats;
    bool clash = spans_overlap(ring, ring_floats, y, rows * SEGF_C) || spans_overlap(ring, ring_floats, d, SEGF_C) ||
                 spans_overlap(ring, ring_floats, scale, SEGF_C) || spans_overlap(ring, ring_floats, shift, SEGF_C) ||
                 spans_overlap(ring, ring_floats, (const float*)slots, N);
    for (int m = 0; m < nmaps; ++m) clash = clash || spans_overlap(ring, ring_floats, z[m], (long)N * h[m] * w[m] * SEGF_C);
    REQUIRE(!clash, "segfuse_pool_fwd_frames: the ring overlaps an input");
    if (!patches) return 0;
    const SegfPoolFrames pa = {{scale, shift, ring, slot_floats, nslots, slots, 0}};
    CFFM_LAUNCH((k_segfuse_fwd<true, true>), ((unsigned)((patches + 3) / 4)), (256), 0, (hipStream_t)stream, const_cast<float*>(y), d, mp, N, H, W, pa);
    CHECK_LAUNCH("segfuse_pool_fwd_frames");
    return 0;
}

// ------------------------------------------------------------------------------------------- resize + cross entropy
static int upce_geom(UpceGeom& G, int M, int K, int h, int w, int H, int W, int ignore, const char* who) {
    if (M < 0 || K < 1 || K > 256 || h < 1 || w < 1 || H < h || W < w || (long)H > (long)UPCE_MAX_RATIO * h ||
        (long)W > (long)UPCE_MAX_RATIO * w)
        return fail(-1, "%s: unsupported sizes (K=%d, %dx%d -> %dx%d; 1 <= K <= 256, resize factor 1..%d)", who, K, h, w, H, W,
                    UPCE_MAX_RATIO);
    G.M = M; G.K = K; G.h = h; G.w = w; G.H = H; G.W = W; G.ignore = ignore; G.rn = G.cn = 0; G.foot = G.win = 0;
    G.inner = 1; G.ms_outer = (long)K * h * w; G.ms_inner = 0; G.ks = h * w; G.ps = 1;       // plain [M,K,h,w]
    G.label_idx = nullptr; G.map_scale = nullptr;
    return 0;
}
// the caller's layout of the logits (include/cffm_hip.h: cffm_upce_maps_*); every element offset must fit 31 bits past its map base
static int upce_layout(UpceGeom& G, int inner, long ms_outer, long ms_inner, int ks, int ps, const char* who) {
    REQUIRE(inner >= 1 && ks >= 1 && ps >= 1 && ms_outer >= 0 && ms_inner >= 0, "%s: bad logits layout", who);
    REQUIRE((ks == 1) != (ps == 1) || (G.K == 1 || G.h * G.w == 1), "%s: either classes (ks = 1, token rows) or cells (ps = 1, [K][h][w]) must be contiguous", who);
    REQUIRE((long)(G.K - 1) * ks + (long)(G.h * G.w - 1) * ps < (1L << 31), "%s: a logits map spans more than 2^31 elements", who);
    G.inner = inner; G.ms_outer = ms_outer; G.ms_inner = ms_inner; G.ks = ks; G.ps = ps;
    return 0;
}
// host restatement of segf_taps (the LDS tile of the forward pass has to cover first tap .. last tap of a 16-pixel span)
static void host_taps(int dst, int in, int out, int& i0, int& i1) {
    const float scale = (float)in / (float)out;
    float s = scale * ((float)dst + 0.5f) - 0.5f;
    s = s < 0.f ? 0.f : s;
    i0 = std::min((int)s, in - 1);
    i1 = i0 + (i0 < in - 1 ? 1 : 0);
}
static int span_taps(int in, int out) {
    int need = 1;
    for (int t = 0; t < out; t += UPCE_TILE) {
        int a0, a1, b0, b1;
        host_taps(t, in, out, a0, a1);
        host_taps(std::min(t + UPCE_TILE, out) - 1, in, out, b0, b1);
        need = std::max(need, b1 - a0 + 1);
    }
    return need;
}
static int upce_lds(const void* kernel, size_t bytes, const char* who) {
    if (bytes > 160 * 1024) return fail(-1, "%s: the low-resolution tile needs %zu bytes of LDS", who, bytes);
    int have = 0;      // (the size changes with the geometry: asked at every call)
    if (bytes > 65536 && !lds_grant(have, {{kernel, (int)bytes}})) return fail(-2, "%s: cannot reserve %zu bytes of LDS", who, bytes);
    return 0;
}
long cffm_upce_blocks(int M, int H, int W) {
    return (long)M * ((H + UPCE_TILE - 1) / UPCE_TILE) * ((W + UPCE_TILE - 1) / UPCE_TILE);
}
int cffm_upce_fwd(const float* logits, const long long* labels, float* lse, float* part, int M, int K, int h, int w, int H, int W,
                  int ignore_index, void* stream) {
    return cffm_upce_maps_fwd(logits, labels, nullptr, lse, part, M, K, h, w, H, W, ignore_index, 1, (long)K * h * w, 0, h * w, 1, stream);
}
int cffm_upce_maps_fwd(const float* logits, const long long* labels, const int* label_idx, float* lse, float* part, int M, int K, int h,
                       int w, int H, int W, int ignore_index, int inner, long ms_outer, long ms_inner, int ks, int ps, void* stream) {
    UpceGeom G;
    TRY(upce_geom(G, M, K, h, w, H, W, ignore_index, "upce_fwd"));
    if (!M) return 0;
    REQUIRE(logits && labels && lse && part, "upce_fwd: null");
    TRY(upce_layout(G, inner, ms_outer, ms_inner, ks, ps, "upce_fwd"));
    G.label_idx = label_idx;
    G.rn = span_taps(h, H);
    G.cn = span_taps(w, W);
    const int cells = G.rn * G.cn, kper = ps != 1 ? UPCE_ROWS_KPER : (cells >= 256 ? 1 : 256 / cells);
    const size_t lds = ((size_t)cells * (UPCE_KP(K) + 1) + (size_t)cells * kper + 8) * sizeof(float);
    TRY(upce_lds((const void*)k_upce_fwd, lds, "upce_fwd"));
    hipStream_t st = (hipStream_t)stream;
    REQUIRE(cffm_upce_blocks(M, H, W) < (1L << 31), "upce_fwd: too many tiles");
    CFFM_LAUNCH(k_upce_fwd, ((unsigned)cffm_upce_blocks(M, H, W)), (256), lds, st, logits, labels, lse, part, G);
    CHECK_LAUNCH("upce_fwd");
    return 0;
}
// out[0] = sum_m wl[m] * (sum of map m's loss records), out[1] = sum_m wh[m] * (sum of its hit records); part as cffm_upce_maps_fwd left it
// (cffm_upce_blocks(M, H, W) / M records per map, map-major); wl / wh: M doubles each on the device
int cffm_upce_maps_finalize(const float* part, int M, long per, const double* wl, const double* wh, float* out, void* stream) {
    REQUIRE(part && wl && wh && out && M >= 1 && per >= 1 && per < (1L << 30), "upce_maps_finalize: bad arguments");
    CFFM_LAUNCH(k_upce_finalize, (1), (256), 0, (hipStream_t)stream, part, M, (int)per, wl, wh, out);
    CHECK_LAUNCH("upce_maps_finalize");
    return 0;
}
int cffm_upce_bwd(const float* logits, const long long* labels, const float* lse, const float* gscale, float scale,
                  float* dlogits, int M, int K, int h, int w, int H, int W, int ignore_index, void* stream) {
    return cffm_upce_maps_bwd(logits, labels, nullptr, lse, gscale, nullptr, scale, dlogits, M, K, h, w, H, W, ignore_index, 1,
                              (long)K * h * w, 0, h * w, 1, stream);
}
int cffm_upce_maps_bwd(const float* logits, const long long* labels, const int* label_idx, const float* lse, const float* gscale,
                       const float* map_scale, float scale, float* dlogits, int M, int K, int h, int w, int H, int W, int ignore_index,
                       int inner, long ms_outer, long ms_inner, int ks, int ps, void* stream) {
    UpceGeom G;
    TRY(upce_geom(G, M, K, h, w, H, W, ignore_index, "upce_bwd"));
    if (!M) return 0;
    REQUIRE(logits && labels && lse && dlogits, "upce_bwd: null");
    TRY(upce_layout(G, inner, ms_outer, ms_inner, ks, ps, "upce_bwd"));
    G.label_idx = label_idx;
    G.map_scale = map_scale;
    const bool plain = inner == 1 && ms_outer == (long)K * h * w && ks == h * w && ps == 1;
    G.rn = std::min(h, UPCE_QT + 2);
    G.cn = std::min(w, UPCE_QT + 2);
    // LDS capacities for this resize factor, from the kernel's own formulas (the same float expressions): the largest output
    // footprint of a 4 x 4 tile along each dimension and the largest candidate window of one pixel
    auto span = [](int q0, int q1, int in, int out) {     // candidate range of low-resolution indices q0..q1, clamped
        const float is = (float)out / (float)in;
        int lo = (int)floorf(((float)q0 - 0.5f) * is - 0.5f) - 1, hi = (int)ceilf(((float)q1 + 1.5f) * is - 0.5f) + 1;
        lo = std::max(lo, 0); hi = std::min(hi, out - 1);
        return hi - lo + 1;
    };
    int fy = 1, fx = 1, win = 1;
    for (int q0 = 0; q0 < h; q0 += UPCE_QT) fy = std::max(fy, span(q0, std::min(q0 + UPCE_QT - 1, h - 1), h, H));
    for (int q0 = 0; q0 < w; q0 += UPCE_QT) fx = std::max(fx, span(q0, std::min(q0 + UPCE_QT - 1, w - 1), w, W));
    for (int q = 0; q < h; ++q) win = std::max(win, span(q, q, h, H));
    for (int q = 0; q < w; ++q) win = std::max(win, span(q, q, w, W));
    G.foot = (fy * fx + 1) & ~1;      // even: the tap tables behind the two footprint arrays stay 16-byte aligned
    G.win = win;
    hipStream_t st = (hipStream_t)stream;
    REQUIRE((long)M * ((w + UPCE_QT - 1) / UPCE_QT) * ((h + UPCE_QT - 1) / UPCE_QT) < (1L << 31), "upce_bwd: too many tiles");
    const unsigned grid = (unsigned)((long)M * ((w + UPCE_QT - 1) / UPCE_QT) * ((h + UPCE_QT - 1) / UPCE_QT));
    // two forms: the block form evaluates every output pixel's soft-max about 1.2 x per launch from register-resident cells; the gather
    // form re-evaluates it in each low-resolution pixel it taps (round 1; the fallback for down-sampling geometries, where blocks are not
    // contiguous runs)
    static int slots = 0;
    if (!slots) {
        slots = 1024;                                   // resident workgroups of the block kernel on the whole device
#ifndef CFFM_EMU
        int per_cu = 0, dev = 0, cus = 0;
        if (hipGetDevice(&dev) == hipSuccess && hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess &&
            hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, (const void*)k_upce_bwd_blk, UPCE_BLK_THREADS, 16 * 1024) == hipSuccess &&
            per_cu > 0 && cus > 0)
            slots = per_cu * cus;
#endif
    }
    if (H >= h && W >= w) {
        // owned cell rows per workgroup: the ring row costs (ty + 1) / ty, a partly filled last wave of workgroups costs its idle slots
        const int TXo = UPCE_BLK_COLS - 1, gxb = (w + TXo - 1) / TXo, cpw = UPCE_BLK_THREADS / UPCE_BLK_COLS, nch = (UPCE_KP(K) / 4 + cpw - 1) / cpw;
        int ty = 0;
        double best = -1.0;
        for (int t = 2; t <= 16 && t <= std::max(h, 2); ++t) {
            const long nwg = (long)M * gxb * ((h + t - 1) / t) * nch;
            const long waves = (nwg + slots - 1) / slots;
            const double eff = (double)t / (t + 1) * (double)nwg / (double)(waves * slots);
            if (eff > best) { best = eff; ty = t; }
        }
        UpceBlkGeom Bk;
        Bk.ty = ty;
        Bk.xcap = (int)ceil((double)UPCE_BLK_COLS * W / w) + 4;
        Bk.ycap = (int)ceil((double)(ty + 1) * H / h) + 4;
        Bk.fcap = Bk.xcap * Bk.ycap;
        const size_t lds_blk = ((size_t)2 * (Bk.fcap + Bk.xcap + Bk.ycap) + (ty + 3) + (UPCE_BLK_COLS + 3)) * sizeof(float);
        const long nwg = (long)M * gxb * ((h + ty - 1) / ty) * nch;
        REQUIRE(nwg < (1L << 31), "upce_bwd: too many tiles");
        TRY(upce_lds((const void*)k_upce_bwd_blk, lds_blk, "upce_bwd"));
        CFFM_LAUNCH(k_upce_bwd_blk, ((unsigned)nwg), (UPCE_BLK_THREADS), lds_blk, st, logits, labels, lse, gscale, scale, dlogits, G, Bk);
    } else {
        REQUIRE(plain && (long)M * K * h * w < (1L << 31), "upce_bwd: the gather form reads plain [M,K,h,w] logits below 2^31 elements");
        const size_t lds = ((size_t)G.rn * G.cn * UPCE_KP(K) + 2 * (size_t)G.foot + 2 * 16 * G.win * 4) * sizeof(float);
        TRY(upce_lds((const void*)k_upce_bwd, lds, "upce_bwd"));
        CFFM_LAUNCH(k_upce_bwd, (grid), (256), lds, st, logits, labels, lse, gscale, scale, dlogits, G);
    }
    CHECK_LAUNCH("upce_bwd");
    return 0;
}

// ------------------------------------------------------------------------------------------- BatchNorm + ReLU + 1/8 stack (head)
static unsigned hf_stat_grid(long units) {
    long b = (units + 63) / 64;
    return (unsigned)(b > 1024 ? 1024 : (b < 1 ? 1 : b));
}
long cffm_colstats_records(long rows) { return (long)hf_stat_grid((rows + 3) / 4); }
int cffm_colstats(const float* y, long rows, float* part, void* stream) {
    REQUIRE(rows >= 0 && (rows == 0 || (y && part)), "colstats: null");
    if (!rows) return 0;
    CFFM_LAUNCH(k_colstats_partial, (hf_stat_grid((rows + 3) / 4)), (256), 0, (hipStream_t)stream, y, rows, part);
    CHECK_LAUNCH("colstats");
    return 0;
}
long cffm_bn_relu_pool_records(int N, int H, int W) { return ((long)N * (H / 2) * (W / 2) + HF_BLOCKS_PER_WG - 1) / HF_BLOCKS_PER_WG; }
int cffm_bn_relu_pool_fwd(const float* y, const float* scale, const float* shift, const float* mask, float* fused, float* stack, int N,
                          int H, int W, void* stream) {
    REQUIRE(N >= 0 && H >= 2 && W >= 2 && H % 2 == 0 && W % 2 == 0, "bn_relu_pool_fwd: even map sides expected, got %dx%d", H, W);
    if (!N) return 0;
    REQUIRE(y && scale && shift && fused, "bn_relu_pool_fwd: null");
    CFFM_LAUNCH(k_bn_relu_pool_fwd, ((unsigned)cffm_bn_relu_pool_records(N, H, W)), (256), 0, (hipStream_t)stream, y, scale, shift, mask, fused,
                stack, N, H, W);
    CHECK_LAUNCH("bn_relu_pool_fwd");
    return 0;
}
int cffm_bn_relu_pool_bwd1(const float* y, const float* scale, const float* shift, const float* xs, const float* xo, const float* mask,
                           const float* dfused, const float* dstack, float* g, float* part, int N, int H, int W, void* stream) {
    REQUIRE(N >= 0 && H >= 2 && W >= 2 && H % 2 == 0 && W % 2 == 0, "bn_relu_pool_bwd1: even map sides expected, got %dx%d", H, W);
    if (!N) return 0;
    REQUIRE(y && scale && shift && xs && xo && g && part, "bn_relu_pool_bwd1: null");
    CFFM_LAUNCH(k_bn_relu_pool_bwd1, ((unsigned)cffm_bn_relu_pool_records(N, H, W)), (256), 0, (hipStream_t)stream, y, scale, shift, xs, xo,
                mask, dfused, dstack, g, part, N, H, W);
    CHECK_LAUNCH("bn_relu_pool_bwd1");
    return 0;
}
int cffm_bn_bwd2(float* g, const float* y, const float* xs, const float* xo, const float* c1, const float* mg, const float* mgx, long rows,
                 void* stream) {
    if (!rows) return 0;
    REQUIRE(g && y && xs && xo && c1 && mg && mgx, "bn_bwd2: null");
    CFFM_LAUNCH(k_bn_bwd2, (hf_stat_grid((rows + 3) / 4) * 4), (256), 0, (hipStream_t)stream, g, y, xs, xo, c1, mg, mgx, rows);
    CHECK_LAUNCH("bn_bwd2");
    return 0;
}

int cffm_bn_finalize_fwd(const float* part, long nrec, double count, const float* weight, const float* bias, float* running_mean,
                         float* running_var, float momentum, float eps, float* coef, void* stream) {
    REQUIRE(weight && bias && coef, "bn_finalize_fwd: null");
    REQUIRE(part ? (nrec >= 1 && count >= 1.0) : (running_mean && running_var), "bn_finalize_fwd: records (training) or running statistics (eval) needed");
    REQUIRE(!running_mean == !running_var, "bn_finalize_fwd: running_mean and running_var come together");
    CFFM_LAUNCH(k_bn_finalize_fwd, (CFFM_C / HF_FIN_CH), (1024), 0, (hipStream_t)stream, part, nrec, count, weight, bias, running_mean, running_var, momentum,
                eps, coef);
    CHECK_LAUNCH("bn_finalize_fwd");
    return 0;
}
int cffm_bn_finalize_bwd(const float* part, long nrec, double count, const float* weight, const float* xs, int training, float* out,
                         void* stream) {
    REQUIRE(part && weight && xs && out && nrec >= 1 && count >= 1.0, "bn_finalize_bwd: null / empty");
    CFFM_LAUNCH(k_bn_finalize_bwd, (CFFM_C / HF_FIN_CH), (1024), 0, (hipStream_t)stream, part, nrec, count, weight, xs, training, out);
    CHECK_LAUNCH("bn_finalize_bwd");
    return 0;
}

int cffm_rows_resize_fwd(const float* src, long src_map_stride, float* dst, long dst_map_stride, int N, int h, int w, int H, int W, int C,
                         void* stream) {
    REQUIRE(N >= 0 && h >= 1 && w >= 1 && H >= 1 && W >= 1 && C >= 4 && C % 4 == 0, "rows_resize_fwd: bad sizes");
    if (!N) return 0;
    REQUIRE(src && dst && src_map_stride >= (long)h * w * C && dst_map_stride >= (long)H * W * C && src_map_stride % 4 == 0 && dst_map_stride % 4 == 0,
            "rows_resize_fwd: null / overlapping maps");
    const long total = (long)N * H * W * (C / 4);
    CFFM_LAUNCH(k_rows_resize_fwd, ((unsigned)std::min<long>((total + 255) / 256, 1 << 16)), (256), 0, (hipStream_t)stream, src, src_map_stride, dst,
                dst_map_stride, N, h, w, H, W, C);
    CHECK_LAUNCH("rows_resize_fwd");
    return 0;
}
int cffm_rows_resize_bwd(const float* ddst, long ddst_map_stride, float* dsrc, long dsrc_map_stride, int N, int h, int w, int H, int W, int C,
                         void* stream) {
    REQUIRE(N >= 0 && h >= 1 && w >= 1 && H >= 1 && W >= 1 && C >= 4 && C % 4 == 0, "rows_resize_bwd: bad sizes");
    if (!N) return 0;
    REQUIRE(ddst && dsrc && dsrc_map_stride >= (long)h * w * C && ddst_map_stride >= (long)H * W * C && dsrc_map_stride % 4 == 0 && ddst_map_stride % 4 == 0,
            "rows_resize_bwd: null / overlapping maps");
    const long total = (long)N * h * w * (C / 4);
    CFFM_LAUNCH(k_rows_resize_bwd, ((unsigned)std::min<long>((total + 255) / 256, 1 << 16)), (256), 0, (hipStream_t)stream, ddst, ddst_map_stride, dsrc,
                dsrc_map_stride, N, h, w, H, W, C);
    CHECK_LAUNCH("rows_resize_bwd");
    return 0;
}

// ------------------------------------------------------------------------------------------- clip data path
int cffm_clip_format_hsv(const unsigned char* frames, const unsigned char* labels, float* out_img, long long* out_lab, int T, int H, int W,
                         int y1, int x1, int ch, int cw, int flip, int Ho, int Wo, const float mean[3], const float std[3], int to_rgb,
                         float pad_val, int seg_pad_val, int reduce_zero_label, const float* brightness_beta, const float* contrast_alpha,
                         const int* contrast_first, const float* saturation, const float* hue_shift, void* stream) {
    REQUIRE(T >= 0 && H >= 1 && W >= 1 && Ho >= 1 && Wo >= 1, "clip_format: bad sizes");
    const bool any_photo = brightness_beta || contrast_alpha || saturation || hue_shift;
    REQUIRE(!any_photo || T <= CLIP_MAXT, "clip_format: at most %d frames with photometric parameters", CLIP_MAXT);
    REQUIRE(y1 >= 0 && x1 >= 0 && ch >= 0 && cw >= 0 && y1 + ch <= H && x1 + cw <= W && ch <= Ho && cw <= Wo,
            "clip_format: crop box %d+%d x %d+%d does not fit a %dx%d frame / %dx%d output", y1, ch, x1, cw, H, W, Ho, Wo);
    if (!T) return 0;
    REQUIRE(frames && out_img && mean && std && (!out_lab || labels), "clip_format: null");
    ClipFmt P;
    P.T = T; P.H = H; P.W = W; P.y1 = y1; P.x1 = x1; P.ch = ch; P.cw = cw; P.flip = flip ? 1 : 0; P.Ho = Ho; P.Wo = Wo;
    P.to_rgb = to_rgb ? 1 : 0; P.reduce_zero_label = reduce_zero_label ? 1 : 0; P.seg_pad = seg_pad_val; P.pad_val = pad_val;
    P.photo = any_photo ? 1 : 0;
    for (int t = 0; t < CLIP_MAXT; ++t) {   // NaN = "not taken" (the reference draws a parameter only when the branch is taken)
        const float bt = (brightness_beta && t < T) ? brightness_beta[t] : NAN, al = (contrast_alpha && t < T) ? contrast_alpha[t] : NAN;
        const float sa = (saturation && t < T) ? saturation[t] : NAN, hu = (hue_shift && t < T) ? hue_shift[t] : NAN;
        P.has_b[t] = bt == bt; P.has_c[t] = al == al; P.has_s[t] = sa == sa; P.has_h[t] = hu == hu;
        P.beta[t] = P.has_b[t] ? bt : 0.f; P.alpha[t] = P.has_c[t] ? al : 1.f;
        P.sat[t] = P.has_s[t] ? sa : 1.f;
        REQUIRE(!P.has_h[t] || (hu == (float)(int)hu && hu > -100000.f && hu < 100000.f), "clip_format: the hue shift of frame %d is not an integer", t);
        P.hue[t] = P.has_h[t] ? (int)hu : 0;
        P.c_first[t] = (contrast_first && t < T && contrast_first[t]) ? 1 : 0;
    }
    for (int c = 0; c < 3; ++c) {
        REQUIRE(std[c] != 0.f, "clip_format: zero std");
        P.mean[c] = mean[c];
        P.stdinv[c] = (float)(1.0 / (double)std[c]);     // mmcv.imnormalize: stdinv = 1 / np.float64(std), applied in float32
    }
    const long n = (long)T * Ho * Wo, want = (n + 255) / 256;
    CFFM_LAUNCH(k_clip_format, ((unsigned)(want < 8192 ? want : 8192)), (256), 0, (hipStream_t)stream, frames, labels, out_img, out_lab, P);
    CHECK_LAUNCH("clip_format");
    return 0;
}
int cffm_clip_resize(const unsigned char* frames, const unsigned char* labels, int T, int H, int W, unsigned char* out_frames,
                     unsigned char* out_labels, int Ho, int Wo, void* stream) {
    REQUIRE(T >= 0 && H >= 1 && W >= 1 && Ho >= 1 && Wo >= 1 && H < (1 << 15) && W < (1 << 15) && Ho < (1 << 15) && Wo < (1 << 15), "clip_resize: bad sizes");
    if (!T) return 0;
    REQUIRE((frames || labels) && (!frames || out_frames) && (!labels || out_labels), "clip_resize: null");
    ClipResize P;
    P.T = T; P.H = H; P.W = W; P.Ho = Ho; P.Wo = Wo;
    P.scale_x = 1.0 / ((double)Wo / (double)W);          // scale_x = 1. / inv_scale_x, as cv::resize computes it
    P.scale_y = 1.0 / ((double)Ho / (double)H);
    P.half = (W == 2 * Wo && H == 2 * Ho) ? 1 : 0;
    const long n = (long)T * Ho * Wo, want = (n + 255) / 256;
    CFFM_LAUNCH(k_clip_resize, ((unsigned)(want < 8192 ? want : 8192)), (256), 0, (hipStream_t)stream, frames, labels, out_frames, out_labels, P);
    CHECK_LAUNCH("clip_resize");
    return 0;
}

// ------------------------------------------------------------------------------------------- evaluation counts
int cffm_seg_counts(const long long* pred, const long long* label, long n, int num_classes, int ignore_index, int reduce_zero_label,
                    long long* counts, void* stream) {
    REQUIRE(n >= 0 && n < (1L << 32) && num_classes >= 1 && num_classes <= SEGCNT_MAXK, "seg_counts: bad sizes");
    if (!n) return 0;
    REQUIRE(pred && label && counts, "seg_counts: null");
    const long want = (n + 255) / 256;
    const unsigned blocks = (unsigned)(want < 2048 ? want : 2048);
    CFFM_LAUNCH(k_seg_counts, (blocks), (256), 0, (hipStream_t)stream, pred, label, n, num_classes, ignore_index, reduce_zero_label,
                (unsigned long long*)counts);
    CHECK_LAUNCH("seg_counts");
    return 0;
}

int cffm_vc_counts(const long long* gt, const long long* pred, int F, long npix, int n, long long* counts, void* stream) {
    REQUIRE(F >= 0 && npix >= 0 && n >= 1 && npix < (1L << 31), "vc_counts: bad sizes");
    if (F - n <= 0 || !npix) return 0;
    REQUIRE(gt && pred && counts, "vc_counts: null");
    REQUIRE(F - n <= 65535, "vc_counts: more than 65535 start frames in one call");
    CFFM_LAUNCH(k_vc_counts, ((unsigned)((npix + 255) / 256), (unsigned)(F - n)), (256), 0, (hipStream_t)stream, gt, pred, npix, n,
                (unsigned long long*)counts);
    CHECK_LAUNCH("vc_counts");
    return 0;
}

// ------------------------------------------------------------------------------------------- layer
// The layer on token rows (channels-last) on both sides: x_rows [B,4,HW,256] -> y_rows [B,HW,256] (new target frame).  No layout
// transposes and no copy of the input: `x_rows` itself is the NHWC stack the blocks read (the caller keeps it for the backward).
int cffm_layer_forward_rows(const cffm_geom* g, int depth, const cffm_block_params* params, const float* x_rows, float* y_rows,
                            const int* key_src, const int* q_dst, float* saved, float* scratch, void* stream) {
    REQUIRE(g && params && x_rows && y_rows && saved && scratch && depth >= 1, "layer_forward_rows: bad arguments");
    cffm_block_ws L;
    cffm_block_ws_layout(g, &L);
    const long HW = g->HW, img = HW * CFFM_C;
    float* blk0 = saved + up((long)g->B * 4 * img);
    TRY(param_prep(params, depth, blk0, L.total, L, stream));
    for (int i = 0; i < depth; ++i) {
        float* ws = blk0 + (long)i * L.total;
        const float* tgt = (i == 0) ? x_rows + 3 * img : blk0 + (long)(i - 1) * L.total + L.x2;
        const long tgt_bs = (i == 0) ? 4 * img : img;
        // the last block writes its output rows straight into the caller's (as layer_infer_blocks does)
        TRY(block_forward_impl(g, &params[i], x_rows, 4 * img, tgt, tgt_bs, key_src, q_dst, ws, scratch, stream, i == depth - 1 ? y_rows : nullptr));
    }
    return 0;
}
// dy_rows [B,HW,256] -> dx_rows [B,4,HW,256] and every parameter gradient; x_rows as given to cffm_layer_forward_rows
int cffm_layer_backward_rows(const cffm_geom* g, int depth, const cffm_block_params* params, const cffm_block_grads* grads,
                             const float* x_rows, const float* dy_rows, float* dx_rows, const int* key_src, const int* q_dst,
                             const int* inv_ptr, const int* inv_idx, const float* saved, float* scratch, void* stream) {
    REQUIRE(g && params && grads && x_rows && dy_rows && dx_rows && saved && scratch && depth >= 1, "layer_backward_rows: bad arguments");
    cffm_block_ws L;
    cffm_block_ws_layout(g, &L);
    const Scratch S = scratch_layout(g);
    const long HW = g->HW, img = HW * CFFM_C;
    const float* blk0 = saved + up((long)g->B * 4 * img);
    tail_reset();
    for (int i = depth - 1; i >= 0; --i) {
        const float* ws = blk0 + (long)i * L.total;
        const float* tgt = (i == 0) ? x_rows + 3 * img : blk0 + (long)(i - 1) * L.total + L.x2;
        const long tgt_bs = (i == 0) ? 4 * img : img;
        // block i reads the gradient of its output from buffer (depth - 1 - i) & 1 and writes the next block's into the other one
        // (never in place: its weight-gradient GEMMs on the side stream still read `dout` while ln_pool_bwd writes dtgt)
        float* dtgt = (i == 0) ? dx_rows + 3 * img : scratch + (((depth - i) & 1) ? S.a2 : S.a);
        const long dtgt_bs = (i == 0) ? 4 * img : img;
        // the last block reads the caller's gradient directly
        const float* dout = (i == depth - 1) ? dy_rows : scratch + (((depth - 1 - i) & 1) ? S.a2 : S.a);
        TRY(block_backward_impl(g, &params[i], &grads[i], x_rows, 4 * img, tgt, tgt_bs, key_src, q_dst, inv_ptr, inv_idx, ws, dout, dtgt, dtgt_bs,
                                scratch, 1, (depth - 1 - i) & 1, i, depth, stream));
    }
    // the reference frames of every block in one pass + the CFFA parameter gradients, then the last block's parameter-gradient tail
    RedJobs* tail_jobs = nullptr;
    if (g_tail.has) {     // the last block's record reductions ride in the CFFA's final reduction launch
        g_tail.has = false;
        tail_jobs = &g_tail.jobs;
    }
    TRY(cffa_finish(g, depth, params, grads, depth - 1, 0, blk0, L.total, x_rows, 4 * img, dx_rows, 4 * img, 0, stream, tail_jobs));
    side_join_all((hipStream_t)stream);
    return 0;
}

// y_tgt_nchw: the new target frame, images y_bs floats apart; y_full (or NULL): the reference's whole output [B,4,C,H,W], whose
// frames 0..2 are copies of the input (cffm_transformer.py:826) -- copied on the side stream while the blocks run
static int layer_forward_impl(const cffm_geom* g, int depth, const cffm_block_params* params, const float* x_nchw,
                              float* y_tgt_nchw, long y_bs, float* y_full, const int* key_src, const int* q_dst, float* saved,
                              float* scratch, void* stream) {
    REQUIRE(g && params && x_nchw && y_tgt_nchw && saved && scratch && depth >= 1, "layer_forward: bad arguments");
    cffm_block_ws L;
    cffm_block_ws_layout(g, &L);
    const long HW = g->HW, img = HW * CFFM_C;
    float* xs = saved;  // NHWC stack [B,4,HW,C]
    float* blk0 = saved + up((long)g->B * 4 * img);
    // the parameter-derived tables do not depend on x: they are built in the launch of the input transpose, or beside it
    hipStream_t st = (hipStream_t)stream;
    side_init(st);
    if (depth <= PREP_MAXD) {
        // ONE launch: the input transpose (frames 0..2 also copied to y_full) + the parameter prep of every block (k_transpose_prep)
        PROF(ST_TRANSPOSE);
        PrepArgs a;
        const int pnx = prep_args(a, params, 0, depth, blk0, L.total, L);
        TrArgs T;
        T.src = x_nchw; T.dst = xs; T.rows = CFFM_C; T.cols = (int)HW; T.src_bs = img; T.dst_bs = img; T.add_mod = 4; T.add_skip = 3; T.copy_dst = y_full;
        T.gx = ((int)HW + 63) / 64; T.gy = (CFFM_C + 63) / 64; T.gz = g->B * 4;
        CFFM_LAUNCH(k_transpose_prep, ((unsigned)(T.gx * T.gy * T.gz + pnx * depth)), (256), 0, st, T, a, pnx);
        CHECK_LAUNCH("transpose + param_prep");
        g_prep_join.pending = false;
    } else {
        // deeper layers: the prep on the side stream while the input is transposed
        side_fork_mark(st, 0);
        // NCHW -> NHWC of the four frames; frames 0..2 also go to y_full as they are (the reference's pass-through frames) with the same read
        TRY(transpose_add(x_nchw, xs, g->B * 4, CFFM_C, (int)HW, img, img, nullptr, 4, 3, stream, y_full));
        hipStream_t sd = side_fork_take(st, 0);
        TRY(param_prep(params, depth, blk0, L.total, L, (void*)sd));
        side_mark(sd, st, 0);
        g_prep_join.pending = sd != st;      // joined behind the first block's ln_pool_fwd (block_forward_impl)
        g_prep_join.side = sd;
    }
    g_side.used = 0;   // (that was this call's only side branch, joined here)
    for (int i = 0; i < depth; ++i) {
        float* ws = blk0 + (long)i * L.total;
        const float* tgt = (i == 0) ? xs + 3 * img : blk0 + (long)(i - 1) * L.total + L.x2;
        const long tgt_bs = (i == 0) ? 4 * img : img;
        // the last block's fused Mlp kernel writes the target frame in NCHW itself (no rows, no transpose behind it)
        const bool last = i == depth - 1;
        TRY(block_forward_impl(g, &params[i], xs, 4 * img, tgt, tgt_bs, key_src, q_dst, ws, scratch, stream, nullptr, last ? y_tgt_nchw : nullptr,
                               last ? y_bs : 0));
    }
    return 0;
}
int cffm_layer_forward(const cffm_geom* g, int depth, const cffm_block_params* params, const float* x_nchw,
                       float* y_tgt_nchw, const int* key_src, const int* q_dst, float* saved, float* scratch,
                       void* stream) {
    REQUIRE(g, "layer_forward: bad arguments");
    return layer_forward_impl(g, depth, params, x_nchw, y_tgt_nchw, g->HW * CFFM_C, nullptr, key_src, q_dst, saved, scratch, stream);
}
int cffm_layer_forward_full(const cffm_geom* g, int depth, const cffm_block_params* params, const float* x_nchw,
                            float* y_full_nchw, const int* key_src, const int* q_dst, float* saved, float* scratch,
                            void* stream) {
    REQUIRE(g && y_full_nchw && y_full_nchw != x_nchw, "layer_forward_full: bad arguments");
    const long img = g->HW * CFFM_C;
    return layer_forward_impl(g, depth, params, x_nchw, y_full_nchw + 3 * img, 4 * img, y_full_nchw, key_src, q_dst, saved, scratch, stream);
}

// ------------------------------------------------------------------------------------------- inference forward (ABI 12)
// BasicLayer3d3.forward (cffm_transformer.py:917-927) for calls that autograd records nothing of: the same four kernels per block in their
// store-free instantiations (k_ln_pool_fwd<true>, the q|k|v row-panel GEMM without its T-frag copy, k_cfm_attn_fwd<true>,
// k_mlp_fwd<MT, D, true>) -- same arithmetic in the same order, so the output equals the training forward's bit for bit -- with
//   * the parameter-only data (bias fragments, pooling matrix, forward-form fragment-ordered weights) in a buffer the caller prepares
//     ONCE per set of weights (cffm_layer_prepare: k_param_prep on a grid that stops in front of the input-gradient forms),
//   * one transient workspace that does not grow with depth: zall | f16 q|k|v | ao | two x2 buffers the blocks ping-pong between,
//   * the last block's x2 written straight into the caller's rows,
//   * every launch on the caller's stream, no library-side allocation: a captured call is a single chain.
struct PreparedLayout { long bias, M, w_frag, total; };
static PreparedLayout prepared_layout() {
    PreparedLayout L;
    long p = 0;
    L.bias = p; p += up((long)BIASH_HALFS / 2);
    L.M = p; p += up(CFFM_NCELL * CFFM_WA);
    L.w_frag = p; p += up(PREP_WFLOATS);          // qkv | proj | fc1 | fc2, forward (NT) form
    L.total = p;
    return L;
}
struct InferWs { long zall, qkv, ao, x2[2], total; };
static InferWs infer_ws_layout(const cffm_geom* g) {
    const long B = g->B, HW = g->HW, RC = g->RC;
    InferWs w;
    long p = 0;
    w.zall = p; p += up(B * RC * CFFM_C);
    w.qkv = p; p += up(B * RC * 768 / 2);         // f16 q|k|v
    w.ao = p; p += up(B * HW * CFFM_C);
    w.x2[0] = p; p += up(B * HW * CFFM_C);
    w.x2[1] = p; p += up(B * HW * CFFM_C);
    w.total = p;
    return w;
}
long cffm_layer_prepared_floats(int depth) { return depth < 1 ? -1 : depth * prepared_layout().total; }
long cffm_layer_infer_ws_floats(const cffm_geom* g) { return (!g || g->B < 1 || g->HW < 1 || g->RC < 1) ? -1 : infer_ws_layout(g).total; }

static int infer_lds_grant() {
    static int lds_have = 0;
    return lds_grant(lds_have, {{(const void*)k_mlp_fwd<MLP_MT, MLP_D, true>, PNL_FUSED_LDS(MLP_MT)}, {(const void*)k_mlp_fwd<MLP_MT, MLP_D, true, true>, PNL_FUSED_LDS(MLP_MT)}}) ? 0 : -1;
}
// Panel height of the inference Mlp kernel.  The training choice (MLP_MT = 2: 32 rows) leaves more than half of the 256 CUs idle when a
// call has under 4096 rows (B = 1 on the 60 x 60 grid: 113 workgroups); 16-row panels then still fit one round (225 workgroups).  Measured
// on the layer, depth 2, eager: 126.0 -> 119.3 us at 3600 rows; 16-row panels in two rounds lose (B = 2 60 x 60 166 -> 200 us, 60 x 108
// 155 -> 189 us: every workgroup streams all 2.25 MB of weights), so the rule stops at one round.  Below 1024 rows nothing was measured:
// the training choice stays.  Rows are independent and a row's sums keep their order: the output does not depend on the choice.
static int infer_mlp_mt(long NP) { return (NP > 1024 && (NP + 15) / 16 <= 256) ? 1 : MLP_MT; }
static int infer_check_params(const cffm_block_params* params, int depth, const char* who) {
    for (int i = 0; i < depth; ++i) {
        const cffm_block_params& p = params[i];
        bool ok = p.norm1_w && p.norm1_b && p.rpb_own && p.rpb_ring && p.qkv_w && p.qkv_b && p.proj_w && p.proj_b && p.norm2_w && p.norm2_b &&
                  p.fc1_w && p.fc1_b && p.fc2_w && p.fc2_b;
        for (int q = 0; q < 4; ++q) ok = ok && p.pool_w[q] && p.pool_b[q] && p.rpb_pool[q];
        REQUIRE(ok, "%s: null parameter in block %d", who, i);
    }
    return 0;
}
int cffm_layer_prepare(int depth, const cffm_block_params* params, float* prepared, void* stream) {
    REQUIRE(params && prepared && depth >= 1, "layer_prepare: bad arguments");
    TRY(infer_check_params(params, depth, "layer_prepare"));
    REQUIRE(!infer_lds_grant(), "layer_prepare: LDS grant failed");     // (here, so that the first inference call may already be a captured one)
    const PreparedLayout P = prepared_layout();
    cffm_block_ws L = {};
    L.bias = P.bias; L.M = P.M; L.w_frag = P.w_frag;     // (w_split is not written: pack 2)
    PROF(ST_BIAS_ASM);
    for (int d0 = 0; d0 < depth; d0 += PREP_MAXD) {
        const int nd = (depth - d0 < PREP_MAXD) ? depth - d0 : PREP_MAXD;
        PrepArgs a;
        // the grid stops in front of the workgroups that write the input-gradient forms: only a backward reads those
        const int pnx = prep_args(a, params, d0, nd, prepared, P.total, L) - PREP_FBLOCKS / 2;
        CFFM_LAUNCH(k_param_prep, (pnx, nd), (256), 0, (hipStream_t)stream, a);
    }
    CHECK_LAUNCH("layer_prepare");
    return 0;
}

// the blocks of one call: `stack` = NHWC frames [B,4,HW,256]; the last block's output rows [B,HW,256] go to `y_rows`, or (y_rows NULL) as
// NCHW images y_bs floats apart to `y_nchw` (k_mlp_fwd's NCHW form)
static int layer_infer_blocks(const cffm_geom* g, int depth, const cffm_block_params* params, const float* prepared, const float* stack,
                              float* y_rows, const int* key_src, const int* q_dst, float* ws, void* stream, float* y_nchw = nullptr, long y_bs = 0,
                              const LnpRing* ring = nullptr, long frame_bs = 0, bool tables = false) {
    // ring != NULL: `stack` is a ring of frame buffers and the four frames are those of ring->slots (k_ln_pool_fwd<true, true>); block 0's
    // residual rows are the copy that launch leaves in the x2 buffer no block touches before block 1 writes it.  tables: ring->slots holds
    // one 4-entry table per sample and every sample reads whole slots (k_ln_pool_fwd<true, true, true>; frame_bs is not used)
    REQUIRE(!infer_lds_grant(), "layer_infer: LDS grant failed");
    const PreparedLayout P = prepared_layout();
    const InferWs W = infer_ws_layout(g);
    const long HW = g->HW, img = HW * CFFM_C, NR = (long)g->B * g->RC, NP = (long)g->B * HW;
    REQUIRE(NP < (1L << 21), "layer_infer: bad sizes");
    hipStream_t st = (hipStream_t)stream;
    const Geo G = to_geo(g);
    for (int i = 0; i < depth; ++i) {
        const cffm_block_params* p = &params[i];
        const float* pre = prepared + (long)i * P.total;
        const float* wf = pre + P.w_frag;
        const bool ring0 = ring && i == 0;
        const float* tgt = ring0 ? ws + W.x2[1] : (i == 0) ? stack + 3 * img : ws + W.x2[(i - 1) & 1];
        const long tgt_bs = (i == 0 && !ring) ? 4 * img : img;
        float* x2 = (i == depth - 1) ? y_rows : ws + W.x2[i & 1];
        {
            PROF(ST_LN_POOL_FWD);
            PoolB pb;
            for (int q = 0; q < 4; ++q) pb.b[q] = p->pool_b[q];
            if (ring) {
                LnpRing rg = *ring;
                rg.tgt_copy = ws + W.x2[1];
                if (tables) {
                    const LnpRingTables rt = {rg};
                    CFFM_LAUNCH((k_ln_pool_fwd<true, true, true>), (g->nW, 4, g->B), (LNP_THREADS), 0, st, G, stack, 0L, ring0 ? nullptr : tgt, tgt_bs,
                                p->norm1_w, p->norm1_b, pre + P.M, PoolW(), pb, ws + W.zall, nullptr, nullptr, 1, rt);
                } else
                    CFFM_LAUNCH((k_ln_pool_fwd<true, true>), (g->nW, 4, g->B), (LNP_THREADS), 0, st, G, stack, frame_bs, ring0 ? nullptr : tgt, tgt_bs,
                                p->norm1_w, p->norm1_b, pre + P.M, PoolW(), pb, ws + W.zall, nullptr, nullptr, 1, rg);
            } else
                CFFM_LAUNCH(k_ln_pool_fwd<true>, (g->nW, 4, g->B), (LNP_THREADS), 0, st, G, stack, 4 * img, tgt, tgt_bs, p->norm1_w, p->norm1_b,
                            pre + P.M, PoolW(), pb, ws + W.zall, nullptr, nullptr, 1, LnpNoRing());
        }
        {
            PROF(ST_GEMM); PROF2(ST_G_QKV_FWD);
            REQUIRE(!panel_qkv_fwd(ws + W.zall, wf, p->qkv_b, (h16*)(ws + W.qkv), NR, st, nullptr), "layer_infer: qkv gemm failed");
        }
        {
            PROF(ST_ATTN_FWD);
            CFFM_LAUNCH(k_cfm_attn_fwd<true>, (g->B * g->nW * CFFM_HEADS), (256), ATT_FWD_LDS, st, G, (const h16*)(ws + W.qkv), key_src, q_dst,
                        (const h16*)(pre + P.bias), ws + W.ao, nullptr);
        }
        {
            PROF(ST_GEMM); PROF2(ST_MLP_FWD);
            MlpFwdArgs a = {};
            a.ao = ws + W.ao; a.xt = tgt; a.xt_bs = tgt_bs; a.rows_per_batch = g->HW;
            a.wp = (const f32x4*)(wf + 768 * 256); a.w1 = (const f32x4*)(wf + 768 * 256 + 256 * 256); a.w2 = (const f32x4*)(wf + 768 * 256 + 256 * 256 + 1024 * 256);
            a.bp = p->proj_b; a.b1 = p->fc1_b; a.b2 = p->fc2_b; a.g2 = p->norm2_w; a.be2 = p->norm2_b;
            a.x2 = x2; a.NP = (int)NP;
            const bool nchw = i == depth - 1 && !y_rows;
            if (nchw) { a.x2 = nullptr; a.x2_nchw = y_nchw; a.x2_bs = y_bs; }
            if (infer_mlp_mt(NP) == 1) {
                if (nchw) CFFM_LAUNCH((k_mlp_fwd<1, MLP_D, true, true>), ((unsigned)((NP + 15) / 16)), (PNL_THREADS), PNL_FUSED_LDS(1), st, a);
                else CFFM_LAUNCH((k_mlp_fwd<1, MLP_D, true>), ((unsigned)((NP + 15) / 16)), (PNL_THREADS), PNL_FUSED_LDS(1), st, a);
            } else {
                if (nchw) CFFM_LAUNCH((k_mlp_fwd<MLP_MT, MLP_D, true, true>), ((unsigned)cffm_mlp_records(NP)), (PNL_THREADS), PNL_FUSED_LDS(MLP_MT), st, a);
                else CFFM_LAUNCH((k_mlp_fwd<MLP_MT, MLP_D, true>), ((unsigned)cffm_mlp_records(NP)), (PNL_THREADS), PNL_FUSED_LDS(MLP_MT), st, a);
            }
        }
        CHECK_LAUNCH("layer_infer block");
    }
    return 0;
}
static int layer_infer_check(const cffm_geom* g, int depth, const cffm_block_params* params, const float* prepared, const void* x, const void* y,
                             const int* key_src, const int* q_dst, const float* ws, const char* who) {
    REQUIRE(g && params && prepared && x && y && key_src && q_dst && ws && depth >= 1, "%s: bad arguments", who);
    REQUIRE(g->B >= 1 && g->HW == g->H0 * g->W0 && g->RC == 64 * g->nW && g->nW == g->gy * g->gx && g->nW >= 1, "%s: geometry not initialised", who);
    REQUIRE(x != y, "%s: input and output must not alias", who);
    return infer_check_params(params, depth, who);
}
int cffm_layer_infer_rows(const cffm_geom* g, int depth, const cffm_block_params* params, const float* prepared, const float* x_rows, float* y_rows,
                          const int* key_src, const int* q_dst, float* ws, void* stream) {
    TRY(layer_infer_check(g, depth, params, prepared, x_rows, y_rows, key_src, q_dst, ws, "layer_infer_rows"));
    return layer_infer_blocks(g, depth, params, prepared, x_rows, y_rows, key_src, q_dst, ws, stream);
}
// The four frames where a ring of per-frame row buffers holds them: frame t of sample b = ring + clamp(slots[t]) * slot_floats + b * frame_bs
// (slots: device int[4], the target last; entries may repeat).  No pointer argument depends on the table: a captured call is replayed for
// other frames by rewriting the 16 bytes of the table.  Otherwise cffm_layer_infer_rows: same workspace, same prepared data, one stream.
int cffm_layer_infer_rows_ring(const cffm_geom* g, int depth, const cffm_block_params* params, const float* prepared, const float* ring,
                               long slot_floats, int nslots, const int* slots, long frame_bs, float* y_rows, const int* key_src,
                               const int* q_dst, float* ws, void* stream) {
    TRY(layer_infer_check(g, depth, params, prepared, ring, y_rows, key_src, q_dst, ws, "layer_infer_rows_ring"));
    const long img = (long)g->HW * CFFM_C;
    REQUIRE(slots && !((uintptr_t)slots & 3) && !((uintptr_t)ring & 15), "layer_infer_rows_ring: null or misaligned slot table / ring");
    // (a slot may be shorter than a batch of frames: with slot_floats = img and frame_bs = 4 img the ring is the stack of cffm_layer_infer_rows)
    REQUIRE(nslots >= 1 && frame_bs >= img && frame_bs % 4 == 0 && slot_floats % 4 == 0 && slot_floats >= img,
            "layer_infer_rows_ring: %d slots of %ld floats, frames %ld apart, for %d frames of %ld floats", nslots, slot_floats, frame_bs, g->B, img);
    const long ring_floats = (long)(nslots - 1) * slot_floats + (long)(g->B - 1) * frame_bs + img;
    REQUIRE(!spans_overlap(ring, ring_floats, y_rows, (long)g->B * img), "layer_infer_rows_ring: y_rows lies inside the ring");
    REQUIRE(!spans_overlap(ring, ring_floats, ws, infer_ws_layout(g).total), "layer_infer_rows_ring: the workspace lies inside the ring");
    LnpRing rg = {slots, slot_floats, nslots, nullptr};
    return layer_infer_blocks(g, depth, params, prepared, ring, y_rows, key_src, q_dst, ws, stream, nullptr, 0, &rg, frame_bs);
}
// The same with one table per sample: frame t of sample b = ring + clamp(slots[4 * b + t]) * slot_floats (slots: device int[B * 4]), whole
// slots of the one ring -- the B targets of a chunk of one video, each with its own clip, in one call.
int cffm_layer_infer_rows_ring_tables(const cffm_geom* g, int depth, const cffm_block_params* params, const float* prepared, const float* ring,
                                      long slot_floats, int nslots, const int* slots, float* y_rows, const int* key_src, const int* q_dst,
                                      float* ws, void* stream) {
    TRY(layer_infer_check(g, depth, params, prepared, ring, y_rows, key_src, q_dst, ws, "layer_infer_rows_ring_tables"));
    const long img = (long)g->HW * CFFM_C;
    REQUIRE(slots && !((uintptr_t)slots & 3) && !((uintptr_t)ring & 15), "layer_infer_rows_ring_tables: null or misaligned slot tables / ring");
    REQUIRE(nslots >= 1 && slot_floats % 4 == 0 && slot_floats >= img, "layer_infer_rows_ring_tables: %d slots of %ld floats for frames of %ld floats",
            nslots, slot_floats, img);
    const long ring_floats = (long)(nslots - 1) * slot_floats + img;
    REQUIRE(!spans_overlap(ring, ring_floats, y_rows, (long)g->B * img), "layer_infer_rows_ring_tables: y_rows lies inside the ring");
    REQUIRE(!spans_overlap(ring, ring_floats, ws, infer_ws_layout(g).total), "layer_infer_rows_ring_tables: the workspace lies inside the ring");
    LnpRing rg = {slots, slot_floats, nslots, nullptr};
    return layer_infer_blocks(g, depth, params, prepared, ring, y_rows, key_src, q_dst, ws, stream, nullptr, 0, &rg, 0, true);
}
// The reference's whole output [B,4,C,H,W].  The NHWC stack the blocks read needs as much room as the output has: it is built IN
// y_full (so the workspace stays what the rows form needs) and y_full gets its real contents when the last block is done -- frames
// 0..2 copied from the input, frame 3 transposed from the last block's rows.
int cffm_layer_infer_full(const cffm_geom* g, int depth, const cffm_block_params* params, const float* prepared, const float* x_nchw,
                          float* y_full_nchw, const int* key_src, const int* q_dst, float* ws, void* stream) {
    TRY(layer_infer_check(g, depth, params, prepared, x_nchw, y_full_nchw, key_src, q_dst, ws, "layer_infer_full"));
    const InferWs W = infer_ws_layout(g);
    const long HW = g->HW, img = HW * CFFM_C;
    float* stack = y_full_nchw;
    TRY(transpose_add(x_nchw, stack, g->B * 4, CFFM_C, (int)HW, img, img, nullptr, 1, -1, stream));
    // From depth 2 on the last block's fused Mlp kernel writes frame 3 in NCHW itself: the stack was last read by that block's
    // k_ln_pool_fwd, and its residual rows are the block before's x2 in `ws`.  At depth 1 the residual rows ARE frame 3 of the stack,
    // which other workgroups of the launch still read: rows + a transpose, as before.
    float* last = depth > 1 ? nullptr : ws + W.x2[0];
    TRY(layer_infer_blocks(g, depth, params, prepared, stack, last, key_src, q_dst, ws, stream, y_full_nchw + 3 * img, 4 * img));
    for (int b = 0; b < g->B; ++b)
        REQUIRE(hipMemcpyAsync(y_full_nchw + (long)b * 4 * img, x_nchw + (long)b * 4 * img, (size_t)3 * img * sizeof(float), hipMemcpyDeviceToDevice,
                               (hipStream_t)stream) == hipSuccess, "layer_infer_full: copy failed");
    if (last) TRY(cffm_transpose(last, y_full_nchw + 3 * img, g->B, (int)HW, CFFM_C, img, 4 * img, stream));
    return 0;
}

// blocks first_block, first_block - 1, ..., last_block of the layer backward (depth - 1 >= first >= last >= 0): the piece with
// first == depth - 1 starts from dy (its layout transpose included), the piece with last == 0 ends with the transpose of the
// gradient stack into dx; the intermediate state lives in `scratch`, so consecutive pieces must be issued in order on one stream.
// Data-parallel training calls it block by block and starts the gradient all-reduce of block i while block i - 1 runs
// (vss_cffm_amd/distributed.py; the reference's DDP does the same with its buckets: mmseg/apis/train.py:57-65).
static int layer_backward_impl(const cffm_geom* g, int depth, const cffm_block_params* params, const cffm_block_grads* grads,
                               const float* dy_tgt_nchw, long dy_bs, const float* dy_full, float* dx_nchw, const int* key_src,
                               const int* q_dst, const int* inv_ptr, const int* inv_idx, const float* saved, float* scratch,
                               int first_block, int last_block, void* stream) {
    REQUIRE(g && params && grads && dy_tgt_nchw && dx_nchw && saved && scratch && depth >= 1, "layer_backward: bad arguments");
    REQUIRE(first_block < depth && last_block >= 0 && first_block >= last_block, "layer_backward: bad block range %d..%d of %d", first_block,
            last_block, depth);
    cffm_block_ws L;
    cffm_block_ws_layout(g, &L);
    const Scratch S = scratch_layout(g);
    const long HW = g->HW, img = HW * CFFM_C;
    const float* xs = saved;
    const float* blk0 = saved + up((long)g->B * 4 * img);
    float* dxs = scratch + S.dxs;   // NHWC gradient stack [B,4,HW,C]
    REQUIRE(dy_bs >= img, "layer_backward: dy batch stride %ld < %ld", dy_bs, img);
    tail_reset();
    for (int i = first_block; i >= last_block; --i) {
        const float* ws = blk0 + (long)i * L.total;
        const float* tgt = (i == 0) ? xs + 3 * img : blk0 + (long)(i - 1) * L.total + L.x2;
        const long tgt_bs = (i == 0) ? 4 * img : img;
        // gradient of the current block's output target [B,HW,C]: buffer (depth - 1 - i) & 1 of {a, a2}; the target-frame gradient
        // goes to the stack for block 0, otherwise into the OTHER buffer (the block's weight-gradient GEMMs on the side stream
        // still read `dout` while ln_pool_bwd writes it)
        float* dcur = scratch + (((depth - 1 - i) & 1) ? S.a2 : S.a);
        float* dtgt = (i == 0) ? dxs + 3 * img : scratch + (((depth - i) & 1) ? S.a2 : S.a);
        const long dtgt_bs = (i == 0) ? 4 * img : img;
        // the last block's fused Mlp kernel reads dy in NCHW itself and leaves its rows in `dcur` (no transpose in front of it)
        const bool from_dy = i == depth - 1;
        TRY(block_backward_impl(g, &params[i], &grads[i], xs, 4 * img, tgt, tgt_bs, key_src, q_dst, inv_ptr, inv_idx, ws, dcur, dtgt, dtgt_bs, scratch,
                                1, (depth - 1 - i) & 1, i, depth, stream, from_dy ? dy_tgt_nchw : nullptr, from_dy ? dy_bs : 0));
    }
    // The reference frames of every block of the range in ONE pass (they pass through the layer unchanged: one read of x_ref, one write
    // of dx_ref per range instead of a read + read-modify-write per block) and the range's CFFA parameter gradients.  A caller that
    // walks the layer block by block (data-parallel training, BlockwiseReducer) gets a pass per block, accumulating into dx_ref, so
    // that every block's gradient slice is complete when its range returns.
    RedJobs* tail_jobs = nullptr;
    if (last_block == 0 && g_tail.has) {     // the last block's record reductions ride in the end-of-range launch (k_bwd_tail)
        g_tail.has = false;
        tail_jobs = &g_tail.jobs;
    }
    // The output transpose of a range that ends at block 0 (dy_full: the upstream gradient of the whole [B,4,C,H,W] output -- its
    // pass-through frames 0..2 join dx in the same pass) shares the launch of the range's record reductions (k_bwd_tail): neither reads
    // what the other writes, and no fork follows the last ln_pool_bwd -- the transpose on a side stream of its
    // own was queued AHEAD of the blocks' side work by the graph executor and held it up until the chain had finished (0.95 ms per step).
    TailArgs tr;
    if (last_block == 0) tail_transpose(tr, dxs, dx_nchw, g->B * 4, (int)HW, CFFM_C, img, img, dy_full, 4, 3);
    TRY(cffa_finish(g, depth, params, grads, first_block, last_block, blk0, L.total, xs, 4 * img, dxs, 4 * img, first_block != depth - 1, stream, tail_jobs,
                    last_block == 0 ? &tr : nullptr));
    TRY(tail_flush((hipStream_t)stream));
    side_join_all((hipStream_t)stream);   // every parameter gradient of the range is complete behind this point of the stream
    return 0;
}
int cffm_layer_backward_range(const cffm_geom* g, int depth, const cffm_block_params* params, const cffm_block_grads* grads,
                              const float* dy_tgt_nchw, long dy_bs, float* dx_nchw, const int* key_src, const int* q_dst,
                              const int* inv_ptr, const int* inv_idx, const float* saved, float* scratch, int first_block,
                              int last_block, void* stream) {
    return layer_backward_impl(g, depth, params, grads, dy_tgt_nchw, dy_bs, nullptr, dx_nchw, key_src, q_dst, inv_ptr, inv_idx, saved,
                               scratch, first_block, last_block, stream);
}
int cffm_layer_backward_full(const cffm_geom* g, int depth, const cffm_block_params* params, const cffm_block_grads* grads,
                             const float* dy_full_nchw, float* dx_nchw, const int* key_src, const int* q_dst, const int* inv_ptr,
                             const int* inv_idx, const float* saved, float* scratch, int first_block, int last_block, void* stream) {
    REQUIRE(g && dy_full_nchw && dy_full_nchw != dx_nchw, "layer_backward_full: bad arguments");
    const long img = g->HW * CFFM_C;
    return layer_backward_impl(g, depth, params, grads, dy_full_nchw + 3 * img, 4 * img, dy_full_nchw, dx_nchw, key_src, q_dst, inv_ptr,
                               inv_idx, saved, scratch, first_block, last_block, stream);
}
int cffm_layer_backward(const cffm_geom* g, int depth, const cffm_block_params* params, const cffm_block_grads* grads,
                        const float* dy_tgt_nchw, long dy_bs, float* dx_nchw, const int* key_src, const int* q_dst,
                        const int* inv_ptr, const int* inv_idx, const float* saved, float* scratch, void* stream) {
    return cffm_layer_backward_range(g, depth, params, grads, dy_tgt_nchw, dy_bs, dx_nchw, key_src, q_dst, inv_ptr, inv_idx, saved, scratch,
                                     depth - 1, 0, stream);
}

// ------------------------------------------------------------------------------------------- k-means (CFFM++ prototype generation)
// workspace: centre fragments | partial sums [P][K][256] | partial counts [P][K]   (kmeans_kernels.h)
}  // extern "C"
struct KmPlan { int KT, tpw, P; size_t frag_b, part_b, cnt_b; };
static KmPlan km_plan(long N, int K) {
    KmPlan p;
    p.KT = (K + 15) / 16;
    const long tiles = (N + 15) / 16;
    long tpw = (tiles + 4L * KM_WGS - 1) / (4L * KM_WGS);
    if (tpw < 1) tpw = 1;
    if (tpw > KM_MAX_TPW) tpw = KM_MAX_TPW;
    p.tpw = (int)tpw;
    p.P = (int)((N + 64 * tpw - 1) / (64 * tpw));
    p.frag_b = (size_t)km_frag_words(p.KT) * 16;
    p.part_b = ((size_t)p.P * K * CFFM_C * 4 + 255) / 256 * 256;
    p.cnt_b = ((size_t)p.P * K * 4 + 255) / 256 * 256;
    return p;
}
static int km_check(const char* who, long N, int K) {
    REQUIRE(K >= 1 && K <= 128, "%s: K=%d outside 1..128", who, K);
    REQUIRE(N >= K && N <= (1L << 30), "%s: N=%ld outside K..2^30 (K=%d)", who, N, K);
    return 0;
}
template <int KT>
static int km_run(const float* x, int N, int K, int iters, float* centers, int* labels, int* counts, char* ws, const KmPlan& p, hipStream_t st) {
    const size_t lds = (size_t)km_step_lds(KT, p.tpw);
    static int lds_have = 0;      // (granted for the most tiles per wave a plan can ask for: lds never exceeds it)
    REQUIRE(lds_grant(lds_have, {{(const void*)k_km_step<KT>, km_step_lds(KT, KM_MAX_TPW)}}), "kmeans: LDS grant failed");
    f32x4* frags = (f32x4*)ws;
    float* partial = (float*)(ws + p.frag_b);
    int* pcount = (int*)(ws + p.frag_b + p.part_b);
    // the fragments of the centres as given (no records: every centre "keeps its value")
    CFFM_LAUNCH(k_km_reduce, (16 * KT, 4), (256), 0, st, (const float*)partial, (const int*)pcount, 0, K, centers, (bf16*)frags, (int*)nullptr);
    for (int it = 0; it < iters; ++it) {
        const bool last = it == iters - 1;
        CFFM_LAUNCH(k_km_step<KT>, (p.P), (256), lds, st, x, N, K, (const f32x4*)frags, partial, pcount, last ? labels : (int*)nullptr, p.tpw);
        CFFM_LAUNCH(k_km_reduce, (16 * KT, 4), (256), 0, st, (const float*)partial, (const int*)pcount, p.P, K, centers, (bf16*)frags,
                    last ? counts : (int*)nullptr);
    }
    CHECK_LAUNCH("kmeans");
    return 0;
}
extern "C" {
long cffm_kmeans_workspace_bytes(long N, int K) {
    if (km_check("kmeans_workspace_bytes", N, K)) return -1;
    const KmPlan p = km_plan(N, K);
    return (long)(p.frag_b + p.part_b + p.cnt_b);
}
int cffm_kmeans(const float* x, long N, int K, int iters, float* centers_inout, int* labels_out, int* counts_out, void* workspace, void* stream) {
    TRY(km_check("kmeans", N, K));
    REQUIRE(iters >= 1, "kmeans: iters=%d < 1", iters);
    REQUIRE(x && centers_inout && workspace, "kmeans: null x / centers / workspace");
    REQUIRE(((uintptr_t)x | (uintptr_t)centers_inout | (uintptr_t)workspace) % 16 == 0, "kmeans: x / centers / workspace must be 16-byte aligned");
    const KmPlan p = km_plan(N, K);
    hipStream_t st = (hipStream_t)stream;
    char* ws = (char*)workspace;
    switch (p.KT) {
#define KM_CASE(KT_) case KT_: return km_run<KT_>(x, (int)N, K, iters, centers_inout, labels_out, counts_out, ws, p, st);
        KM_CASE(1) KM_CASE(2) KM_CASE(3) KM_CASE(4) KM_CASE(5) KM_CASE(6) KM_CASE(7) KM_CASE(8)
#undef KM_CASE
    }
    return fail(-1, "kmeans: K=%d", K);
}

// ------------------------------------------------------------------------------------------- prediction: two-stage resize + (soft-max) + flip + arg-max
}  // extern "C"
// rows of the low-resolution map that PRED_TILE consecutive output pixels can tap under both stages, as a bound in closed form (no
// restatement of the tap rule whose rounding could differ from the device's): a resize with source step s = in / out maps pixels d .. d + n
// to source positions s n apart, and first tap .. last tap (floor + 1) of positions p apart are at most p + 3 rows; PRED_TILE instead of
// PRED_TILE - 1 steps leaves a whole row to fp32 rounding in either stage
static int pred_span(int in, int mid, int out) {
    const int mid_dist = (int)std::ceil((double)PRED_TILE * mid / out) + 2;      // last minus first stage-1 row
    return std::min((int)std::ceil((double)mid_dist * in / mid) + 3, in);
}
template <bool PROBS>
static void pred_launch(int ny, int nx, unsigned grid, size_t lds, hipStream_t st, const float* logits, long long* pred, float* probs,
                        const PredGeom& G) {
    if (ny == 2 && nx == 2) CFFM_LAUNCH((k_predict<PROBS, 2, 2>), (grid), (256), lds, st, logits, pred, probs, G);
    else if (ny == 2) CFFM_LAUNCH((k_predict<PROBS, 2, 3>), (grid), (256), lds, st, logits, pred, probs, G);
    else if (nx == 2) CFFM_LAUNCH((k_predict<PROBS, 3, 2>), (grid), (256), lds, st, logits, pred, probs, G);
    else CFFM_LAUNCH((k_predict<PROBS, 3, 3>), (grid), (256), lds, st, logits, pred, probs, G);
}
extern "C" {
int cffm_predict(const float* logits, long long* pred, float* probs, int accumulate, int M, int K, int h, int w, int Hm, int Wm, int H,
                 int W, int flip, int inner, long ms_outer, long ms_inner, int ks, int ps, void* stream) {
    REQUIRE(K >= 1 && K <= 256, "predict: K=%d outside 1..256", K);
    REQUIRE(M >= 0 && h >= 1 && w >= 1 && Hm >= 1 && Wm >= 1 && H >= 1 && W >= 1, "predict: bad sizes M=%d, %dx%d -> %dx%d -> %dx%d", M, h, w, Hm,
            Wm, H, W);
    REQUIRE(Hm >= h && Wm >= w && (long)Hm <= (long)PRED_MAX_RATIO * h && (long)Wm <= (long)PRED_MAX_RATIO * w,
            "predict: stage-1 resize %dx%d -> %dx%d outside the factors 1..%d", h, w, Hm, Wm, PRED_MAX_RATIO);
    REQUIRE(2L * H >= Hm && H <= 2L * Hm && 2L * W >= Wm && W <= 2L * Wm, "predict: stage-2 resize %dx%d -> %dx%d outside the factors 0.5..2", Hm,
            Wm, H, W);
    REQUIRE(flip >= 0 && flip <= 2, "predict: flip=%d (0 none, 1 horizontal, 2 vertical)", flip);
    REQUIRE(probs || !accumulate, "predict: accumulate needs probs");
    if (!M) return 0;
    REQUIRE(logits && (pred || probs), "predict: null logits, or neither pred nor probs");
    UpceGeom U;
    U.K = K; U.h = h; U.w = w;
    TRY(upce_layout(U, inner, ms_outer, ms_inner, ks, ps, "predict"));
    PredGeom G;
    G.M = M; G.K = K; G.h = h; G.w = w; G.Hm = Hm; G.Wm = Wm; G.H = H; G.W = W; G.flip = flip; G.accumulate = accumulate ? 1 : 0;
    G.inner = inner; G.ms_outer = ms_outer; G.ms_inner = ms_inner; G.ks = ks; G.ps = ps;
    G.rn = pred_span(h, Hm, H);
    G.cn = pred_span(w, Wm, W);
    // the tile holds every class when it fits the LDS budget (any upsampling in total does), otherwise the classes pass through in chunks
    const int KP = UPCE_KP(K), cells = G.rn * G.cn;
    REQUIRE(cells <= PRED_LDS_FLOATS / 4, "predict: the low-resolution footprint of a tile (%d x %d cells) does not fit the LDS", G.rn, G.cn);
    G.KC = std::min(KP, (PRED_LDS_FLOATS / cells) & ~3);
    G.nchunk = (KP + G.KC - 1) / G.KC;
    const size_t lds = (size_t)cells * G.KC * sizeof(float);
    const long tiles = (long)M * ((H + PRED_TILE - 1) / PRED_TILE) * ((W + PRED_TILE - 1) / PRED_TILE);
    REQUIRE(tiles < (1L << 31), "predict: too many tiles");
    // a stage-2 axis of equal sizes is the identity (every lambda is 0): two taps per axis instead of three
    const int ny = H == Hm ? 2 : 3, nx = W == Wm ? 2 : 3;
    hipStream_t st = (hipStream_t)stream;
    if (probs) pred_launch<true>(ny, nx, (unsigned)tiles, lds, st, logits, pred, probs, G);
    else pred_launch<false>(ny, nx, (unsigned)tiles, lds, st, logits, pred, probs, G);
    CHECK_LAUNCH("predict");
    return 0;
}

// ------------------------------------------------------------------------------------------- Mix-FFN middle: depthwise 3 x 3 + bias + GELU on token rows
}  // extern "C"
static int dwg_check(const char* who, int M, int H, int W, int C) {
    REQUIRE(C >= 4 && C % 4 == 0, "%s: C=%d must be a multiple of 4, at least 4", who, C);
    REQUIRE(M >= 1 && H >= 1 && W >= 1, "%s: bad sizes M=%d H=%d W=%d", who, M, H, W);
    REQUIRE((long)M * H * W * C < (1L << 31), "%s: M*H*W*C = %ld is not below 2^31", who, (long)M * H * W * C);
    return 0;
}
// Strips and slots of one launch (mixffn_kernels.h).  The image is cut into y-strips until `lanes` lanes have work (never below
// DWG_MIN_YS rows: every strip re-reads two halo rows); the live lanes are capped at `lanes` (a memory-bound grid of <= 2048
// workgroups, the rest is strided), `per_slot` waves sharing a slot.
static DwgGeom dwg_plan(int M, int H, int W, int C, int xr, long lanes, int per_slot) {
    DwgGeom G;
    G.M = M; G.H = H; G.W = W; G.C = C; G.C4 = C / 4;
    G.nxr = (W + xr - 1) / xr;
    int ys = H;
    while (ys > DWG_MIN_YS && (long)M * ((H + ys - 1) / ys) * G.nxr * G.C4 < lanes) ys = (ys + 1) / 2;
    G.YS = ys;
    G.nys = (H + ys - 1) / ys;
    G.nsp = (long)M * G.nys * G.nxr;
    G.S = std::min((G.nsp + per_slot - 1) / per_slot, std::max(1L, lanes / per_slot / G.C4));
    return G;
}
#define DWG_FWD_LANES (2048L * 256)     // forward and dh: up to 2048 workgroups of 256 lanes
#define DWG_BWD1_LANES (1024L * 256)    // first backward pass: up to 1024 workgroups, each leaving a 10 KB slab of partial sums
// (checked arguments -> the launch: shared with the MiT stage call)
static void dwg_fwd_launch(const float* h, const float* w, const float* b, float* out, int M, int H, int W, int C, hipStream_t st) {
    const DwgGeom G = dwg_plan(M, H, W, C, DWG_XR, DWG_FWD_LANES, 1);
    CFFM_LAUNCH(k_dwg_fwd, ((unsigned)((G.S * G.C4 + 255) / 256)), (256), 0, st, h, w, b, out, G);
}
// workspace of the backward (floats): the GELU-scaled gradient [M][H][W][C] | the partial weight-gradient slabs [S][10][C4] f32x4
static long dwg_bwd_ws_floats(int M, int H, int W, int C) {
    const DwgGeom G1 = dwg_plan(M, H, W, C, DWG_XR_BWD, DWG_BWD1_LANES, 4);
    return (long)M * H * W * C + G1.S * DWG_NACC * G1.C4 * 4;
}
// (checked arguments -> the two launches: shared with the MiT stage-blocks training call)
static void dwg_bwd_launch(const float* h, const float* w, const float* b, const float* dout, float* dh, float* dw, float* db, float* workspace,
                           int M, int H, int W, int C, hipStream_t st) {
    const DwgGeom G1 = dwg_plan(M, H, W, C, DWG_XR_BWD, DWG_BWD1_LANES, 4);
    const DwgGeom G2 = dwg_plan(M, H, W, C, DWG_XR, DWG_FWD_LANES, 1);
    float* g = workspace;                                      // [M][H][W][C]
    f32x4* part = (f32x4*)(g + (long)M * H * W * C);           // [S][10][C4] f32x4 (M*H*W*C is a multiple of 4: 16-byte aligned)
    const int nred = DWG_NACC * ((G1.C4 + 15) / 16);
    CFFM_LAUNCH(k_dwg_bwd1, ((unsigned)((G1.S * G1.C4 + 63) / 64)), (256), 0, st, h, w, b, dout, g, part, G1);
    CFFM_LAUNCH(k_dwg_bwd2, ((unsigned)(nred + (G2.S * G2.C4 + 255) / 256)), (256), 0, st, (const float*)g, w, dh, (const f32x4*)part, dw, db, G2,
                G1.S, nred);
}
extern "C" {
int cffm_dwconv_gelu_fwd(const float* h, const float* w, const float* b, float* out, int M, int H, int W, int C, void* stream) {
    TRY(dwg_check("dwconv_gelu_fwd", M, H, W, C));
    REQUIRE(aligned16(h) && aligned16(w) && aligned16(b) && aligned16(out), "dwconv_gelu_fwd: h / w / b / out must be non-null and 16-byte aligned");
    dwg_fwd_launch(h, w, b, out, M, H, W, C, (hipStream_t)stream);
    CHECK_LAUNCH("dwconv_gelu_fwd");
    return 0;
}
long cffm_dwconv_gelu_bwd_workspace_bytes(int M, int H, int W, int C) {
    if (dwg_check("dwconv_gelu_bwd_workspace_bytes", M, H, W, C)) return -1;
    return dwg_bwd_ws_floats(M, H, W, C) * 4;
}
int cffm_dwconv_gelu_bwd(const float* h, const float* w, const float* b, const float* dout, float* dh, float* dw, float* db,
                         void* workspace, int M, int H, int W, int C, void* stream) {
    TRY(dwg_check("dwconv_gelu_bwd", M, H, W, C));
    REQUIRE(aligned16(h) && aligned16(w) && aligned16(b) && aligned16(dout) && aligned16(dh) && aligned16(dw) && aligned16(db) &&
            aligned16(workspace), "dwconv_gelu_bwd: h / w / b / dout / dh / dw / db / workspace must be non-null and 16-byte aligned");
    dwg_bwd_launch(h, w, b, dout, dh, dw, db, (float*)workspace, M, H, W, C, (hipStream_t)stream);
    CHECK_LAUNCH("dwconv_gelu_bwd");
    return 0;
}

// ------------------------------------------------------------------------------------------- spatial-reduction attention core (sra_kernels.h)
}  // extern "C"
static int sra_check(const char* who, int B, int N, int Nk, int heads, int hd, float scale) {
    REQUIRE(hd == 32 || hd == 64, "%s: head size %d is not 32 or 64", who, hd);
    REQUIRE(B >= 1 && N >= 1 && Nk >= 1 && heads >= 1, "%s: bad sizes B=%d N=%d Nk=%d heads=%d", who, B, N, Nk, heads);
    REQUIRE(scale > 0.f && scale < INFINITY, "%s: scale %g must be positive and finite", who, (double)scale);
    REQUIRE((long)B * heads <= 65535, "%s: B*heads = %ld is above 65535", who, (long)B * heads);
    const long C = (long)heads * hd;
    REQUIRE((long)B * N * C < (1L << 31) && 2L * B * Nk * C < (1L << 31),
            "%s: B*N*C = %ld or B*Nk*2C = %ld is not below 2^31", who, (long)B * N * C, 2L * B * Nk * C);
    return 0;
}
// query chunks of k_sra_bwd_dkv: enough workgroups to fill the device, at most 64 slabs; *tpc = 16-query tiles per chunk (a multiple of 4)
static int sra_chunks(int B, int N, int Nk, int heads, int* tpc) {
    const long groups = (long)B * heads * ((Nk + SRA_QB - 1) / SRA_QB), nqt = (N + 15) / 16;
    const long want = std::max(1L, std::min(std::min(64L, nqt), (1024 + groups - 1) / groups));
    *tpc = (int)(((nqt + want - 1) / want + 3) / 4 * 4);
    return (int)((nqt + *tpc - 1) / *tpc);
}
static long sra_delta_floats(int B, int N, int heads) { return ((long)B * heads * N + 3) / 4 * 4; }
// two query tiles per wave halve the K / V traffic; one when that leaves fewer than two workgroups per compute unit
static bool sra_wide(int B, int N, int heads) { return (long)B * heads * ((N + 127) / 128) >= 512; }
// (checked arguments -> the launch: shared with the MiT stage call)
static void sra_fwd_launch(const float* q, const float* kv, float* out, float* lse, int B, int N, int Nk, int heads, int hd, float scale, hipStream_t st) {
    const unsigned gz = (unsigned)(B * heads);
#define SRA_FWD(HD_, QW_) CFFM_LAUNCH((k_sra_fwd<HD_, QW_>), ((unsigned)((N + 64 * QW_ - 1) / (64 * QW_)), 1, gz), (256), 0, st, q, kv, out, lse, N, Nk, heads, scale)
    if (sra_wide(B, N, heads)) { if (hd == 64) SRA_FWD(64, 2); else SRA_FWD(32, 2); }
    else { if (hd == 64) SRA_FWD(64, 1); else SRA_FWD(32, 1); }
#undef SRA_FWD
}
// workspace of the backward (floats): delta [B][heads][N] | with more than one query chunk, the dk / dv slabs [chunks][B][Nk][2C]
static long sra_bwd_ws_floats(int B, int N, int Nk, int heads, int hd) {
    int tpc;
    const int chunks = sra_chunks(B, N, Nk, heads, &tpc);
    return sra_delta_floats(B, N, heads) + (chunks > 1 ? 2L * chunks * B * Nk * heads * hd : 0L);
}
// (checked arguments -> the launches: shared with the MiT stage-blocks training call)
static void sra_bwd_launch(const float* q, const float* kv, const float* out, const float* lse, const float* dout, float* dq, float* dkv,
                           float* workspace, int B, int N, int Nk, int heads, int hd, float scale, hipStream_t st) {
    const unsigned gz = (unsigned)(B * heads);
    const double c = (double)scale * 1.4426950408889634;
    const float chi = (float)c, clo = (float)(c - (double)chi);
    int tpc;
    const int chunks = sra_chunks(B, N, Nk, heads, &tpc);
    float* delta = workspace;                                    // [B][heads][N]
    const long stride = 2L * B * Nk * heads * hd;                // floats of one slab [B][Nk][2C]
    float* slab = chunks > 1 ? delta + sra_delta_floats(B, N, heads) : dkv;
#define SRA_DQ(HD_, QW_) CFFM_LAUNCH((k_sra_bwd_dq<HD_, QW_>), ((unsigned)((N + 64 * QW_ - 1) / (64 * QW_)), 1, gz), (256), 0, st, q, kv, out, lse, dout, dq, delta, N, Nk, heads, scale, chi, clo)
    if (sra_wide(B, N, heads)) { if (hd == 64) SRA_DQ(64, 2); else SRA_DQ(32, 2); }
    else { if (hd == 64) SRA_DQ(64, 1); else SRA_DQ(32, 1); }
#undef SRA_DQ
#define SRA_DKV(HD_) CFFM_LAUNCH(k_sra_bwd_dkv<HD_>, ((unsigned)((Nk + SRA_QB - 1) / SRA_QB), (unsigned)chunks, gz), (256), 0, st, q, kv, lse, dout, (const float*)delta, slab, stride, tpc, N, Nk, heads, scale, chi, clo)
    if (hd == 64) SRA_DKV(64); else SRA_DKV(32);
#undef SRA_DKV
    if (chunks > 1) {
        const long n4 = stride / 4;
        CFFM_LAUNCH(k_sra_dkv_sum, ((unsigned)std::min(2048L, (n4 + 255) / 256)), (256), 0, st, (const f32x4*)slab, (f32x4*)dkv, n4, n4, chunks);
    }
}
extern "C" {
int cffm_sra_attn_fwd(const float* q, const float* kv, float* out, float* lse, int B, int N, int Nk, int heads, int hd, float scale, void* stream) {
    TRY(sra_check("sra_attn_fwd", B, N, Nk, heads, hd, scale));
    REQUIRE(aligned16(q) && aligned16(kv) && aligned16(out) && (uintptr_t)lse % 16 == 0,
            "sra_attn_fwd: q / kv / out must be non-null and q / kv / out / lse 16-byte aligned");
    sra_fwd_launch(q, kv, out, lse, B, N, Nk, heads, hd, scale, (hipStream_t)stream);
    CHECK_LAUNCH("sra_attn_fwd");
    return 0;
}
long cffm_sra_attn_bwd_workspace_bytes(int B, int N, int Nk, int heads, int hd) {
    if (sra_check("sra_attn_bwd_workspace_bytes", B, N, Nk, heads, hd, 1.f)) return -1;
    return 4 * sra_bwd_ws_floats(B, N, Nk, heads, hd);
}
int cffm_sra_attn_bwd(const float* q, const float* kv, const float* out, const float* lse, const float* dout, float* dq, float* dkv,
                      void* workspace, int B, int N, int Nk, int heads, int hd, float scale, void* stream) {
    TRY(sra_check("sra_attn_bwd", B, N, Nk, heads, hd, scale));
    REQUIRE(aligned16(q) && aligned16(kv) && aligned16(out) && aligned16(lse) && aligned16(dout) && aligned16(dq) && aligned16(dkv) &&
            aligned16(workspace), "sra_attn_bwd: q / kv / out / lse / dout / dq / dkv / workspace must be non-null and 16-byte aligned");
    sra_bwd_launch(q, kv, out, lse, dout, dq, dkv, (float*)workspace, B, N, Nk, heads, hd, scale, (hipStream_t)stream);
    CHECK_LAUNCH("sra_attn_bwd");
    return 0;
}

// ------------------------------------------------------------------------------------------- spatial-reduction conv + LayerNorm (srln_kernels.h)
}  // extern "C"
static int srln_check(const char* who, int B, int H, int W, int C, int s, float eps, SrGeom* G) {
    REQUIRE(s == 2 || s == 4 || s == 8, "%s: s=%d is not 2, 4 or 8", who, s);
    REQUIRE(C >= 16 && C <= SRLN_MAXC && C % 16 == 0, "%s: C=%d must be a multiple of 16 in 16..%d", who, C, SRLN_MAXC);
    REQUIRE(B >= 1 && H >= s && W >= s, "%s: bad sizes B=%d H=%d W=%d (H and W at least s=%d)", who, B, H, W, s);
    REQUIRE(eps >= 0.f && eps < INFINITY, "%s: eps %g must be finite and not negative", who, (double)eps);
    REQUIRE((long)B * H * W * C < (1L << 31), "%s: B*H*W*C = %ld is not below 2^31", who, (long)B * H * W * C);
    G->B = B; G->H = H; G->W = W; G->C = C; G->Ho = H / s; G->Wo = W / s; G->M = B * G->Ho * G->Wo;
    return 0;
}
static long srln_dz_floats(const SrGeom& G) { return (long)G.M * G.C; }                       // (a multiple of 16)
static int srln_row_blocks(const SrGeom& G) { return (G.M + 15) / 16; }
// column tiles per wave of k_srln_fwd: the largest of 5, 4, 2, 1 that divides C / 16
static int srln_ncw(int C) { const int nc = C / 16; return nc % 5 == 0 ? 5 : nc % 4 == 0 ? 4 : nc % 2 == 0 ? 2 : 1; }
template <int S>
static void srln_launch_fwd(int ncw, unsigned grid, hipStream_t st, const float* x, const float* w, const float* b, const float* gamma,
                            const float* beta, float* out, float* z, float* stats, SrGeom G, float eps) {
#define SRLN_FWD(NCW_) CFFM_LAUNCH((k_srln_fwd<S, NCW_>), (grid), (512), 0, st, x, w, b, gamma, beta, out, z, stats, G, eps)
    if (ncw == 5) SRLN_FWD(5); else if (ncw == 4) SRLN_FWD(4); else if (ncw == 2) SRLN_FWD(2); else SRLN_FWD(1);
#undef SRLN_FWD
}
template <int S>
static void srln_launch_bwd(hipStream_t st, const float* x, const float* w, const float* gamma, const float* z, const float* stats,
                            const float* dout, float* dx, float* dw, float* db, float* dgamma, float* dbeta, float* dz, float* part, SrGeom G) {
    constexpr int S2 = S * S, PQ = S2 < 16 ? S2 / 4 : 4;
    const int nrb = srln_row_blocks(G), C = G.C;
    const long units = (long)nrb * (C / 16) * (S2 / (4 * PQ));
    CFFM_LAUNCH(k_srln_bwd_rows<S>, ((unsigned)nrb), (256), 0, st, z, stats, gamma, dout, dz, part, dx, G);
    CFFM_LAUNCH(k_srln_colsum, ((unsigned)((3 * C + 255) / 256)), (256), 0, st, (const float*)part, dgamma, dbeta, db, nrb, C);
    CFFM_LAUNCH(k_srln_bwd_dx<S>, ((unsigned)((units + 3) / 4)), (256), 0, st, (const float*)dz, w, dx, G, units);
    CFFM_LAUNCH(k_srln_bwd_dw<S>, ((unsigned)(S2 / 4), (unsigned)(C / 16), (unsigned)(C / 16)), (512), 0, st, (const float*)dz, x, dw, G);
}
// (checked arguments -> the launch: shared with the MiT stage call)
static void srln_fwd_launch(int s, hipStream_t st, const float* x, const float* w, const float* b, const float* gamma, const float* beta, float* out,
                            float* z, float* stats, const SrGeom& G, float eps) {
    const unsigned grid = (unsigned)srln_row_blocks(G);
    const int ncw = srln_ncw(G.C);
    if (s == 2) srln_launch_fwd<2>(ncw, grid, st, x, w, b, gamma, beta, out, z, stats, G, eps);
    else if (s == 4) srln_launch_fwd<4>(ncw, grid, st, x, w, b, gamma, beta, out, z, stats, G, eps);
    else srln_launch_fwd<8>(ncw, grid, st, x, w, b, gamma, beta, out, z, stats, G, eps);
}
// workspace of the backward (floats): dz [M][C] | the partial column sums [row blocks][3][C]
static long srln_bwd_ws_floats(const SrGeom& G) { return srln_dz_floats(G) + 3L * srln_row_blocks(G) * G.C; }
// (checked arguments -> the launches: shared with the MiT stage-blocks training call)
static void srln_bwd_launch(int s, hipStream_t st, const float* x, const float* w, const float* gamma, const float* z, const float* stats,
                            const float* dout, float* dx, float* dw, float* db, float* dgamma, float* dbeta, float* workspace, const SrGeom& G) {
    float* dz = workspace;                                       // [M][C]
    float* part = dz + srln_dz_floats(G);                        // [row blocks][3][C]
    if (s == 2) srln_launch_bwd<2>(st, x, w, gamma, z, stats, dout, dx, dw, db, dgamma, dbeta, dz, part, G);
    else if (s == 4) srln_launch_bwd<4>(st, x, w, gamma, z, stats, dout, dx, dw, db, dgamma, dbeta, dz, part, G);
    else srln_launch_bwd<8>(st, x, w, gamma, z, stats, dout, dx, dw, db, dgamma, dbeta, dz, part, G);
}
extern "C" {
int cffm_sr_ln_fwd(const float* x, const float* w, const float* b, const float* gamma, const float* beta, float* out, float* z, float* stats,
                   int B, int H, int W, int C, int s, float eps, void* stream) {
    SrGeom G;
    TRY(srln_check("sr_ln_fwd", B, H, W, C, s, eps, &G));
    REQUIRE(aligned16(x) && aligned16(w) && aligned16(b) && aligned16(gamma) && aligned16(beta) && aligned16(out) &&
            (uintptr_t)z % 16 == 0 && (uintptr_t)stats % 16 == 0,
            "sr_ln_fwd: x / w / b / gamma / beta / out must be non-null and all pointers 16-byte aligned");
    REQUIRE(!z == !stats, "sr_ln_fwd: z and stats must both be given or both be null");
    srln_fwd_launch(s, (hipStream_t)stream, x, w, b, gamma, beta, out, z, stats, G, eps);
    CHECK_LAUNCH("sr_ln_fwd");
    return 0;
}
long cffm_sr_ln_bwd_workspace_bytes(int B, int H, int W, int C, int s) {
    SrGeom G;
    if (srln_check("sr_ln_bwd_workspace_bytes", B, H, W, C, s, 0.f, &G)) return -1;
    return 4 * srln_bwd_ws_floats(G);
}
int cffm_sr_ln_bwd(const float* x, const float* w, const float* gamma, const float* z, const float* stats, const float* dout, float* dx,
                   float* dw, float* db, float* dgamma, float* dbeta, void* workspace, int B, int H, int W, int C, int s, float eps,
                   void* stream) {
    SrGeom G;
    TRY(srln_check("sr_ln_bwd", B, H, W, C, s, eps, &G));
    REQUIRE(aligned16(x) && aligned16(w) && aligned16(gamma) && aligned16(z) && aligned16(stats) && aligned16(dout) &&
            aligned16(dx) && aligned16(dw) && aligned16(db) && aligned16(dgamma) && aligned16(dbeta) && aligned16(workspace),
            "sr_ln_bwd: x / w / gamma / z / stats / dout / dx / dw / db / dgamma / dbeta / workspace must be non-null and 16-byte aligned");
    srln_bwd_launch(s, (hipStream_t)stream, x, w, gamma, z, stats, dout, dx, dw, db, dgamma, dbeta, (float*)workspace, G);
    CHECK_LAUNCH("sr_ln_bwd");
    return 0;
}

// ------------------------------------------------------------------------------------------- LayerNorm of token rows at any width + one MiT stage per call (mitln_kernels.h)
}  // extern "C"
static int mln_check(const char* who, int C, float eps) {
    REQUIRE(C >= 16 && C <= 512 && C % 4 == 0, "%s: C=%d must be a multiple of 4 in 16..512", who, C);
    REQUIRE(eps >= 0.f && eps < INFINITY, "%s: eps %g must be finite and not negative", who, (double)eps);
    return 0;
}
static int mln_check_map(const char* who, int B, int C, int H, int W, float eps) {
    TRY(mln_check(who, C, eps));
    REQUIRE(B >= 1 && H >= 1 && W >= 1, "%s: bad sizes B=%d H=%d W=%d", who, B, H, W);
    REQUIRE((long)B * C * H * W < (1L << 31), "%s: B*C*H*W = %ld is not below 2^31", who, (long)B * C * H * W);
    return 0;
}
// which: 0 rows -> rows (nimg unused) | 1 NCHW -> rows | 2 rows -> NCHW
template <int PW, int V>
static void mln_go(int which, hipStream_t st, const float* x, const float* g, const float* b, float* out, long M, int nimg, const MlnGeom& G, float eps) {
    if (which == 0) {
        constexpr int RPB = 4 * (64 / PW);
        CFFM_LAUNCH((k_ln_rows<PW, V>), ((unsigned)std::min(4096L, (M + RPB - 1) / RPB)), (256), 0, st, x, g, b, out, M, G, eps);
    } else if (which == 1) {
        CFFM_LAUNCH((k_nchw_ln_rows<PW, V>), ((unsigned)(nimg * G.tiles)), (256), (size_t)G.TP * G.LD * sizeof(float), st, x, g, b, out, G, eps);
    } else {
        CFFM_LAUNCH((k_ln_rows_nchw<PW, V>), ((unsigned)(nimg * G.tiles)), (256), (size_t)G.TP * G.LD * sizeof(float), st, x, g, b, out, G, eps);
    }
}
// (checked arguments -> the launch)
static void mln_launch(int which, hipStream_t st, const float* x, const float* g, const float* b, float* out, long M, int nimg, int C, int HW, float eps) {
    const MlnGeom G = mln_geom(C, HW);
    if (G.C4 > 64) return mln_go<64, 2>(which, st, x, g, b, out, M, nimg, G, eps);
    switch (mln_pw(C)) {
        case 4: return mln_go<4, 1>(which, st, x, g, b, out, M, nimg, G, eps);
        case 8: return mln_go<8, 1>(which, st, x, g, b, out, M, nimg, G, eps);
        case 16: return mln_go<16, 1>(which, st, x, g, b, out, M, nimg, G, eps);
        case 32: return mln_go<32, 1>(which, st, x, g, b, out, M, nimg, G, eps);
        default: return mln_go<64, 1>(which, st, x, g, b, out, M, nimg, G, eps);
    }
}

// records [2][C] the backward of M rows leaves in its workspace.  HW = 1: the rows form, one per workgroup of a capped grid; HW > 1: the
// map forms, one per tile.  (A map of one pixel per image IS [B][C] rows: it runs as the rows form.)
static long mln_bwd_records(long M, int C, int HW) {
    if (HW == 1) {
        const long RPB = 4 * (64 / mln_pw(C));
        return std::min((long)MLN_BWD_GRID_CAP, (M + RPB - 1) / RPB);
    }
    return M / HW * mln_geom(C, HW).tiles;
}
// which: as mln_go, the forward whose backward runs
template <int PW, int V>
static void mln_bwd_go(int which, hipStream_t st, const float* x, const float* g, const float* dy, float* dx, float* rec, long M, int nimg,
                       const MlnGeom& G, float eps) {
    const size_t lds = mln_bwd_lds_floats(G, V) * sizeof(float);
    if (which == 0) {
        CFFM_LAUNCH((k_ln_rows_bwd<PW, V>), ((unsigned)mln_bwd_records(M, G.C, 1)), (256), 0, st, x, g, dy, dx, rec, M, G, eps);
    } else if (which == 1) {
        CFFM_LAUNCH((k_nchw_ln_rows_bwd<PW, V>), ((unsigned)(nimg * G.tiles)), (256), lds, st, x, g, dy, dx, rec, G, eps);
    } else {
        CFFM_LAUNCH((k_ln_rows_nchw_bwd<PW, V>), ((unsigned)(nimg * G.tiles)), (256), lds, st, x, g, dy, dx, rec, G, eps);
    }
}
// (checked arguments -> the two launches)
static void mln_bwd_launch(int which, hipStream_t st, const float* x, const float* g, const float* dy, float* dx, float* dgamma, float* dbeta,
                           float* rec, long M, int nimg, int C, int HW, float eps) {
    if (HW == 1) which = 0;
    const MlnGeom G = mln_geom(C, HW);
    if (G.C4 > 64) mln_bwd_go<64, 2>(which, st, x, g, dy, dx, rec, M, nimg, G, eps);
    else switch (mln_pw(C)) {
        case 4: mln_bwd_go<4, 1>(which, st, x, g, dy, dx, rec, M, nimg, G, eps); break;
        case 8: mln_bwd_go<8, 1>(which, st, x, g, dy, dx, rec, M, nimg, G, eps); break;
        case 16: mln_bwd_go<16, 1>(which, st, x, g, dy, dx, rec, M, nimg, G, eps); break;
        case 32: mln_bwd_go<32, 1>(which, st, x, g, dy, dx, rec, M, nimg, G, eps); break;
        default: mln_bwd_go<64, 1>(which, st, x, g, dy, dx, rec, M, nimg, G, eps);
    }
    CFFM_LAUNCH((k_ln_bwd_final), ((unsigned)(C / 2)), (MLN_FIN_SLICES), 0, st, rec, dgamma, dbeta, (int)mln_bwd_records(M, C, HW), C);
}
// the rows form with the neighbouring adds fused in (k_ln_rows_bwd_add): dout = dya (+ dyb), dx = (dres +) LN-backward.  Grid, records and
// the final sum are those of mln_bwd_launch(0, ...)
template <int PW, int V>
static void mln_bwd_add_go(hipStream_t st, const float* x, const float* g, const float* dya, const float* dyb, const float* dres, float* dx,
                           float* rec, long M, const MlnGeom& G, float eps) {
#define MLN_ADD(B_, R_) CFFM_LAUNCH((k_ln_rows_bwd_add<PW, V, B_, R_>), ((unsigned)mln_bwd_records(M, G.C, 1)), (256), 0, st, x, g, dya, dyb, dres, dx, rec, M, G, eps)
    if (dyb) { if (dres) MLN_ADD(true, true); else MLN_ADD(true, false); }
    else { if (dres) MLN_ADD(false, true); else MLN_ADD(false, false); }
#undef MLN_ADD
}
static void mln_bwd_add_launch(hipStream_t st, const float* x, const float* g, const float* dya, const float* dyb, const float* dres, float* dx,
                               float* dgamma, float* dbeta, float* rec, long M, int C, float eps) {
    const MlnGeom G = mln_geom(C, 1);
    if (G.C4 > 64) mln_bwd_add_go<64, 2>(st, x, g, dya, dyb, dres, dx, rec, M, G, eps);
    else switch (mln_pw(C)) {
        case 4: mln_bwd_add_go<4, 1>(st, x, g, dya, dyb, dres, dx, rec, M, G, eps); break;
        case 8: mln_bwd_add_go<8, 1>(st, x, g, dya, dyb, dres, dx, rec, M, G, eps); break;
        case 16: mln_bwd_add_go<16, 1>(st, x, g, dya, dyb, dres, dx, rec, M, G, eps); break;
        case 32: mln_bwd_add_go<32, 1>(st, x, g, dya, dyb, dres, dx, rec, M, G, eps); break;
        default: mln_bwd_add_go<64, 1>(st, x, g, dya, dyb, dres, dx, rec, M, G, eps);
    }
    CFFM_LAUNCH((k_ln_bwd_final), ((unsigned)(C / 2)), (MLN_FIN_SLICES), 0, st, rec, dgamma, dbeta, (int)mln_bwd_records(M, C, 1), C);
}

// workspace of one stage call (floats).  The residual stream alternates between xa and xb inside a block (xa -> proj + residual -> xb ->
// fc2 + residual -> xa), so every block reads and leaves its rows in xa, whatever the depth.  z: the LayerNorm outputs and, once q and kv
// are made from it, the attention output.  q | r (the reduced map) | kv are dead when fc1 runs: they share their room with h.
struct MitWs { long xa, xb, z, q, r, kv, h, a, total; long M; int N, Nk; };
static int mit_cfg_check(const char* who, const cffm_mit_stage_cfg* c, MitWs* Wo) {
    REQUIRE(c, "%s: null cfg", who);
    REQUIRE(c->B >= 1 && c->H >= 1 && c->W >= 1 && c->depth >= 1 && c->heads >= 1,
            "%s: bad sizes B=%d H=%d W=%d depth=%d heads=%d", who, c->B, c->H, c->W, c->depth, c->heads);
    REQUIRE(c->C >= 16 && c->C <= 512 && c->C % 16 == 0, "%s: C=%d must be a multiple of 16 in 16..512", who, c->C);
    REQUIRE(c->C % c->heads == 0 && (c->C / c->heads == 32 || c->C / c->heads == 64), "%s: C=%d with %d heads: the head size must be 32 or 64",
            who, c->C, c->heads);
    REQUIRE(c->hidden >= 4 && c->hidden % 4 == 0, "%s: hidden=%d must be a multiple of 4, at least 4", who, c->hidden);
    const int s = c->sr_ratio;
    REQUIRE(s == 1 || s == 2 || s == 4 || s == 8, "%s: sr_ratio=%d is not 1, 2, 4 or 8", who, s);
    REQUIRE(c->H >= s && c->W >= s, "%s: H=%d and W=%d must be at least sr_ratio=%d", who, c->H, c->W, s);
    const float eps[4] = {c->eps_embed, c->eps_block, c->eps_sr, c->eps_out};
    for (int i = 0; i < 4; ++i) REQUIRE(eps[i] >= 0.f && eps[i] < INFINITY, "%s: eps %g must be finite and not negative", who, (double)eps[i]);
    MitWs W;
    W.N = c->H * c->W;
    W.Nk = s > 1 ? (c->H / s) * (c->W / s) : W.N;
    const long N = (long)c->H * c->W;
    W.M = (long)c->B * N;
    const long widest = std::max(2L * c->C, (long)c->hidden);
    // (the GEMMs address an operand through a buffer descriptor: 32-bit byte offsets)
    REQUIRE(N < (1L << 31) && W.M < (1L << 31) && W.M * widest < (1L << 30), "%s: B*H*W*max(2C, hidden) = %ld is not below 2^30", who, W.M * widest);
    TRY(sra_check(who, c->B, W.N, W.Nk, c->heads, c->C / c->heads, c->scale));
    TRY(dwg_check(who, c->B, c->H, c->W, c->hidden));
    if (s > 1) {
        SrGeom G;
        TRY(srln_check(who, c->B, c->H, c->W, c->C, s, c->eps_sr, &G));
    }
    const long MC = W.M * c->C, KC = (long)c->B * W.Nk * c->C;
    long p = 0;
    W.xa = p; p += up(MC);
    W.xb = p; p += up(MC);
    W.z = p; p += up(MC);
    W.h = p; W.q = p;
    W.r = W.q + up(MC);
    W.kv = W.r + (s > 1 ? up(KC) : 0);
    p += std::max(up(W.M * c->hidden), W.kv + up(2 * KC) - W.q);
    W.a = p; p += up(W.M * c->hidden);
    W.total = p;
    if (Wo) *Wo = W;
    return 0;
}
// the pointers of a stage: everything cffm_mit_stage_infer and cffm_mit_infer read besides the maps and the workspace
static int mit_ptr_check(const char* who, const cffm_mit_stage_cfg* c, const cffm_mit_block_params* blocks, const float* embed_g, const float* embed_b,
                         const float* out_g, const float* out_b) {
    REQUIRE(blocks, "%s: null block parameters", who);
    REQUIRE(aligned16(embed_g) && aligned16(embed_b) && aligned16(out_g) && aligned16(out_b),
            "%s: embed_g / embed_b / out_g / out_b must be non-null and 16-byte aligned", who);
    const int s = c->sr_ratio;
    for (int i = 0; i < c->depth; ++i) {
        const cffm_mit_block_params& p = blocks[i];
        const float* need[] = {p.n1_g, p.n1_b, p.q_w, p.kv_w, p.proj_w, p.proj_b, p.n2_g, p.n2_b, p.fc1_w, p.fc1_b, p.dw_w, p.dw_b, p.fc2_w, p.fc2_b};
        for (const float* t : need) REQUIRE(aligned16(t), "%s: block %d: a parameter is null or not 16-byte aligned", who, i);
        REQUIRE((uintptr_t)p.q_b % 16 == 0 && (uintptr_t)p.kv_b % 16 == 0, "%s: block %d: q_b / kv_b not 16-byte aligned", who, i);
        const float* sr[] = {p.sr_w, p.sr_b, p.srn_g, p.srn_b};
        for (const float* t : sr)
            REQUIRE(s > 1 ? aligned16(t) : !t, "%s: block %d: sr_w / sr_b / srn_g / srn_b must be %s", who, i,
                    s > 1 ? "non-null and 16-byte aligned (sr_ratio > 1)" : "null (sr_ratio == 1)");
    }
    return 0;
}
// a stage behind its embedding (checked arguments; the normalised rows of the embedding are in ws + W.xa): the blocks, then norm_i + the change
// to an NCHW map.  Shared by cffm_mit_stage_infer and cffm_mit_infer.
static int mit_stage_body(const char* who, const cffm_mit_stage_cfg* c, const MitWs& W, const cffm_mit_block_params* blocks, const float* out_g,
                          const float* out_b, float* out_nchw, float* ws, hipStream_t st) {
    const int s = c->sr_ratio;
    const int B = c->B, H = c->H, Wd = c->W, C = c->C, hid = c->hidden, N = W.N, Nk = W.Nk, M = (int)W.M, Mk = B * Nk;
    float *xa = ws + W.xa, *xb = ws + W.xb, *z = ws + W.z, *q = ws + W.q, *r = ws + W.r, *kv = ws + W.kv, *h = ws + W.h, *a = ws + W.a;
    SrGeom SG = {};
    if (s > 1) TRY(srln_check(who, B, H, Wd, C, s, c->eps_sr, &SG));
    for (int i = 0; i < c->depth; ++i) {
        const cffm_mit_block_params& p = blocks[i];
        mln_launch(0, st, xa, p.n1_g, p.n1_b, z, W.M, 0, C, 1, c->eps_block);
        bool bad = gemm_split_launch<false, false>(z, p.q_w, q, M, C, C, C, C, C, 1, st, p.q_b);
        if (s > 1) srln_fwd_launch(s, st, z, p.sr_w, p.sr_b, p.srn_g, p.srn_b, r, nullptr, nullptr, SG, c->eps_sr);
        bad = bad || gemm_split_launch<false, false>(s > 1 ? r : z, p.kv_w, kv, Mk, 2 * C, C, C, C, 2 * C, 1, st, p.kv_b);
        sra_fwd_launch(q, kv, z, nullptr, B, N, Nk, c->heads, C / c->heads, c->scale, st);
        bad = bad || gemm_split_launch<false, false, 2>(z, p.proj_w, xb, M, C, C, C, C, C, 1, st, p.proj_b, xa);
        mln_launch(0, st, xb, p.n2_g, p.n2_b, z, W.M, 0, C, 1, c->eps_block);
        bad = bad || gemm_split_launch<false, false>(z, p.fc1_w, h, M, hid, C, C, C, hid, 1, st, p.fc1_b);
        dwg_fwd_launch(h, p.dw_w, p.dw_b, a, B, H, Wd, hid, st);
        bad = bad || gemm_split_launch<false, false, 2>(a, p.fc2_w, xa, M, C, hid, hid, hid, C, 1, st, p.fc2_b, xb);
        REQUIRE(!bad, "%s: gemm failed", who);
    }
    mln_launch(2, st, xa, out_g, out_b, out_nchw, W.M, B, C, N, c->eps_out);
    return 0;
}

// ---- the overlapping patch embedding (pembed_kernels.h)
static int pemb_check(const char* who, int B, int Cin, int H, int W, int Cout, int k, int stride, float eps, PembGeom* Go) {
    REQUIRE((k == 7 && stride == 4) || (k == 3 && stride == 2), "%s: (k, stride) = (%d, %d) is neither (7, 4) nor (3, 2)", who, k, stride);
    REQUIRE(k == 7 ? (Cin >= 1 && Cin <= 4) : (Cin >= 4 && Cin <= 512 && Cin % 4 == 0),
            "%s: Cin=%d must be %s", who, Cin, k == 7 ? "in 1..4 (k = 7)" : "a multiple of 4 in 4..512 (k = 3)");
    REQUIRE(Cout >= 16 && Cout <= 512 && Cout % 16 == 0, "%s: Cout=%d must be a multiple of 16 in 16..512", who, Cout);
    REQUIRE(B >= 1 && H >= 1 && W >= 1, "%s: bad sizes B=%d H=%d W=%d", who, B, H, W);
    REQUIRE(eps >= 0.f && eps < INFINITY, "%s: eps %g must be finite and not negative", who, (double)eps);
    PembGeom G;
    G.B = B; G.Cin = Cin; G.H = H; G.W = W; G.Cout = Cout; G.K = Cin * k * k;
    G.Ho = (H + 2 * (k / 2) - k) / stride + 1;
    G.Wo = (W + 2 * (k / 2) - k) / stride + 1;
    G.tpr = (G.Wo + 15) / 16;
    const long nin = (long)B * Cin * H * W, nout = (long)B * G.Ho * G.Wo * Cout;
    REQUIRE(nin < (1L << 31) && nout < (1L << 31), "%s: B*Cin*H*W = %ld and B*Ho*Wo*Cout = %ld must be below 2^31", who, nin, nout);
    if (Go) *Go = G;
    return 0;
}
// column tiles per pass of k_pembed_fwd: the largest of (8 with one tile per workgroup,) 5, 4, 2, 1 that divides Cout / 16
static int pemb_ncw(int Cout, int nt) {
    const int nc = Cout / 16;
    return nt == 1 && nc % 8 == 0 ? 8 : nc % 5 == 0 ? 5 : nc % 4 == 0 ? 4 : nc % 2 == 0 ? 2 : 1;
}
// tiles per workgroup of 8 waves (pembed_kernels.h): Cout <= 64: 8 tiles, a wave each | Cout <= 128: 4 tiles, two waves each | wider: one
// tile, its K split over the 8 waves.  TRAIN: the instantiation that also stores the pre-LayerNorm rows z
template <int KS, int ST, int NT, int WAVES, bool TRAIN>
static void pemb_go_nt(hipStream_t st, const float* x, const float* w, const float* b, const float* gamma, const float* beta, float* out, float* z,
                       const PembGeom& G, float eps) {
    const unsigned grid = (unsigned)(((long)G.B * G.Ho * G.tpr + NT - 1) / NT);
#define PEMB_FWD(NCW_) CFFM_LAUNCH((k_pembed_fwd<KS, ST, NCW_, NT, WAVES, TRAIN>), (grid), (WAVES * 64), 0, st, x, w, b, gamma, beta, out, z, G, eps)
    switch (pemb_ncw(G.Cout, NT)) {
        case 8: if constexpr (NT == 1) PEMB_FWD(8); break;       // (Cout = 512 at stage 4: 218 us against 275 with NCW = 4)
        case 5: PEMB_FWD(5); break;
        case 4: PEMB_FWD(4); break;
        case 2: PEMB_FWD(2); break;
        default: PEMB_FWD(1); break;
    }
#undef PEMB_FWD
}
template <int KS, int ST, bool TRAIN>
static void pemb_go(hipStream_t st, const float* x, const float* w, const float* b, const float* gamma, const float* beta, float* out, float* z,
                    const PembGeom& G, float eps) {
    if (G.Cout <= 64) pemb_go_nt<KS, ST, 8, 8, TRAIN>(st, x, w, b, gamma, beta, out, z, G, eps);
    else if (G.Cout <= 128) pemb_go_nt<KS, ST, 4, 8, TRAIN>(st, x, w, b, gamma, beta, out, z, G, eps);
    else pemb_go_nt<KS, ST, 1, 8, TRAIN>(st, x, w, b, gamma, beta, out, z, G, eps);
}
// (checked arguments -> the launch: shared with cffm_mit_infer)
static void pemb_launch(int k, hipStream_t st, const float* x, const float* w, const float* b, const float* gamma, const float* beta, float* out,
                        const PembGeom& G, float eps) {
    if (k == 7) pemb_go<7, 4, false>(st, x, w, b, gamma, beta, out, nullptr, G, eps);
    else pemb_go<3, 2, false>(st, x, w, b, gamma, beta, out, nullptr, G, eps);
}
// workspace of cffm_patch_embed_bwd (floats; every carve 256-byte aligned): dz [M][Cout] | the LayerNorm backward's records | the dw slabs
// [nslab][Cout][KP] | the db records [ndb][Cout] | with dx: the transposed weight [9][Cin][Cout].
// The M split of k_pembed_dw: its grid has ncb * nkb workgroups per slab (64 x 64 output tiles); nslab = ceil(PEMB_DW_WG_TARGET / (ncb * nkb)),
// at most PEMB_DW_SLAB_CAP and at most one slab per PEMB_DW_ROWS rows; a slab is RS = ceil(M / nslab) rows and the count is then ceil(M / RS).
struct PembBwdWs { long dz, rec, slab, dbrec, wt, total; int M, nslab, RS, KP, ncb, nkb, ndb, RB; };
static PembBwdWs pemb_bwd_layout(const PembGeom& G, int with_dx) {
    PembBwdWs W;
    W.M = G.B * G.Ho * G.Wo;
    W.KP = (G.K + 15) / 16 * 16;
    W.ncb = (G.Cout + 63) / 64;
    W.nkb = (W.KP + 63) / 64;
    const int blocks = W.ncb * W.nkb, steps = (W.M + PEMB_DW_ROWS - 1) / PEMB_DW_ROWS;
    int n = (PEMB_DW_WG_TARGET + blocks - 1) / blocks;
    n = std::max(1, std::min(n, std::min(PEMB_DW_SLAB_CAP, steps)));
    W.RS = (W.M + n - 1) / n;
    W.nslab = (W.M + W.RS - 1) / W.RS;
    const int nb = std::max(1, std::min(PEMB_DB_CAP, (W.M + 63) / 64));
    W.RB = (W.M + nb - 1) / nb;
    W.ndb = (W.M + W.RB - 1) / W.RB;
    long p = 0;
    W.dz = p; p += up((long)W.M * G.Cout);
    W.rec = p; p += up(mln_bwd_records(W.M, G.Cout, 1) * 2 * G.Cout);
    W.slab = p; p += up((long)W.nslab * G.Cout * W.KP);
    W.dbrec = p; p += up((long)W.ndb * G.Cout);
    W.wt = p; p += with_dx ? up(9L * G.Cin * G.Cout) : 0;
    W.total = p;
    return W;
}
template <int KS, int ST>
static void pemb_dw_go(hipStream_t st, const float* x, const float* dz, float* slab, const PembGeom& G, const PembBwdWs& W) {
    CFFM_LAUNCH((k_pembed_dw<KS, ST>), ((unsigned)W.nslab, (unsigned)W.ncb, (unsigned)W.nkb), (256), 0, st, x, dz, slab, G, W.RS, W.KP);
}
// (checked arguments -> the launches, all on st, one after the other)
static void pemb_bwd_launch(int k, hipStream_t st, const float* x, const float* w, const float* gamma, const float* z, const float* dout, float* dx,
                            float* dw, float* db, float* dgamma, float* dbeta, float* ws, const PembGeom& G, float eps) {
    const PembBwdWs W = pemb_bwd_layout(G, dx != nullptr);
    float* dz = ws + W.dz;
    mln_bwd_launch(0, st, z, gamma, dout, dz, dgamma, dbeta, ws + W.rec, W.M, 0, G.Cout, 1, eps);
    if (k == 7) pemb_dw_go<7, 4>(st, x, dz, ws + W.slab, G, W);
    else pemb_dw_go<3, 2>(st, x, dz, ws + W.slab, G, W);
    CFFM_LAUNCH(k_pembed_db, ((unsigned)W.ndb), (256), 0, st, (const float*)dz, ws + W.dbrec, W.M, G.Cout, W.RB);
    const long chunks = (long)G.Cout * W.KP / 4 + G.Cout / 4;
    CFFM_LAUNCH(k_pembed_dw_final, ((unsigned)((chunks + 255) / 256)), (256), 0, st, (const float*)(ws + W.slab), (const float*)(ws + W.dbrec), dw, db,
                W.nslab, W.ndb, G.Cout, G.K, W.KP);
    if (dx) {
        CFFM_LAUNCH(k_pembed_wt, ((unsigned)((9L * G.Cin * G.Cout + 255) / 256)), (256), 0, st, w, ws + W.wt, G.Cin, G.Cout);
        CFFM_LAUNCH(k_pembed_dx, ((unsigned)((long)G.B * G.H * ((G.W + 31) / 32))), (256), 0, st, (const float*)dz, (const float*)(ws + W.wt), dx, G);
    }
}
// n consecutive stages: every limit of both parts, the chain of shapes, and the workspace (the maximum over the stages: they run one
// after another).  W / PG (host [n]) may be null.
static int mit_infer_check(const char* who, const cffm_mit_stage* stages, int n, MitWs* W, PembGeom* PG, long* need) {
    REQUIRE(stages, "%s: null stage list", who);
    REQUIRE(n >= 1 && n <= 4, "%s: n=%d stages: 1..4 expected", who, n);
    long most = 0;
    for (int i = 0; i < n; ++i) {
        const cffm_mit_stage& s = stages[i];
        const cffm_mit_stage_cfg& c = s.cfg;
        MitWs Wi;
        PembGeom Gi;
        TRY(mit_cfg_check(who, &c, &Wi));
        TRY(pemb_check(who, c.B, s.Cin, s.Hin, s.Win, c.C, s.k, s.stride, c.eps_embed, &Gi));
        REQUIRE(Gi.Ho == c.H && Gi.Wo == c.W, "%s: stage %d: cfg (H, W) = (%d, %d) is not the convolution's output (%d, %d)", who, i, c.H, c.W,
                Gi.Ho, Gi.Wo);
        if (i > 0) {
            const cffm_mit_stage_cfg& p = stages[i - 1].cfg;
            REQUIRE(c.B == p.B && s.Cin == p.C && s.Hin == p.H && s.Win == p.W,
                    "%s: stage %d: the input [%d,%d,%d,%d] is not stage %d's output [%d,%d,%d,%d]", who, i, c.B, s.Cin, s.Hin, s.Win, i - 1, p.B,
                    p.C, p.H, p.W);
        }
        most = std::max(most, Wi.total);
        if (W) W[i] = Wi;
        if (PG) PG[i] = Gi;
    }
    *need = most;
    return 0;
}
extern "C" {
int cffm_ln_rows(const float* x, const float* gamma, const float* beta, float* out, long M, int C, float eps, void* stream) {
    TRY(mln_check("ln_rows", C, eps));
    REQUIRE(M >= 1 && M * C < (1L << 31), "ln_rows: M=%ld rows of C=%d: M must be at least 1 and M*C below 2^31", M, C);
    REQUIRE(aligned16(x) && aligned16(gamma) && aligned16(beta) && aligned16(out), "ln_rows: x / gamma / beta / out must be non-null and 16-byte aligned");
    mln_launch(0, (hipStream_t)stream, x, gamma, beta, out, M, 0, C, 1, eps);
    CHECK_LAUNCH("ln_rows");
    return 0;
}
int cffm_nchw_ln_rows(const float* x_nchw, const float* gamma, const float* beta, float* out_rows, int B, int C, int H, int W, float eps, void* stream) {
    TRY(mln_check_map("nchw_ln_rows", B, C, H, W, eps));
    REQUIRE(aligned16(x_nchw) && aligned16(gamma) && aligned16(beta) && aligned16(out_rows),
            "nchw_ln_rows: x_nchw / gamma / beta / out_rows must be non-null and 16-byte aligned");
    mln_launch(1, (hipStream_t)stream, x_nchw, gamma, beta, out_rows, (long)B * H * W, B, C, H * W, eps);
    CHECK_LAUNCH("nchw_ln_rows");
    return 0;
}
int cffm_ln_rows_nchw(const float* x_rows, const float* gamma, const float* beta, float* out_nchw, int B, int C, int H, int W, float eps, void* stream) {
    TRY(mln_check_map("ln_rows_nchw", B, C, H, W, eps));
    REQUIRE(aligned16(x_rows) && aligned16(gamma) && aligned16(beta) && aligned16(out_nchw),
            "ln_rows_nchw: x_rows / gamma / beta / out_nchw must be non-null and 16-byte aligned");
    mln_launch(2, (hipStream_t)stream, x_rows, gamma, beta, out_nchw, (long)B * H * W, B, C, H * W, eps);
    CHECK_LAUNCH("ln_rows_nchw");
    return 0;
}

long cffm_ln_bwd_workspace_bytes(long M, int C, int HW) {
    if (mln_check("ln_bwd_workspace_bytes", C, 0.f)) return -1;
    if (!(M >= 1 && HW >= 1 && M % HW == 0 && M * C < (1L << 31)))
        return fail(-1, "ln_bwd_workspace_bytes: M=%ld rows of C=%d, HW=%d: M must be a positive multiple of HW >= 1 and M*C below 2^31", M, C, HW);
    return mln_bwd_records(M, C, HW) * 2 * C * (long)sizeof(float);
}
int cffm_ln_rows_bwd(const float* x, const float* gamma, const float* dout, float* dx, float* dgamma, float* dbeta, void* ws, long M, int C,
                     float eps, void* stream) {
    TRY(mln_check("ln_rows_bwd", C, eps));
    REQUIRE(M >= 1 && M * C < (1L << 31), "ln_rows_bwd: M=%ld rows of C=%d: M must be at least 1 and M*C below 2^31", M, C);
    REQUIRE(aligned16(x) && aligned16(gamma) && aligned16(dout) && aligned16(dx) && aligned16(dgamma) && aligned16(dbeta) && aligned16(ws),
            "ln_rows_bwd: x / gamma / dout / dx / dgamma / dbeta / ws must be non-null and 16-byte aligned");
    mln_bwd_launch(0, (hipStream_t)stream, x, gamma, dout, dx, dgamma, dbeta, (float*)ws, M, 0, C, 1, eps);
    CHECK_LAUNCH("ln_rows_bwd");
    return 0;
}
int cffm_ln_rows_bwd_add(const float* x, const float* gamma, const float* dout_a, const float* dout_b, const float* dres, float* dx, float* dgamma,
                         float* dbeta, void* ws, long M, int C, float eps, void* stream) {
    TRY(mln_check("ln_rows_bwd_add", C, eps));
    REQUIRE(M >= 1 && M * C < (1L << 31), "ln_rows_bwd_add: M=%ld rows of C=%d: M must be at least 1 and M*C below 2^31", M, C);
    REQUIRE(aligned16(x) && aligned16(gamma) && aligned16(dout_a) && aligned16(dx) && aligned16(dgamma) && aligned16(dbeta) && aligned16(ws) &&
            (uintptr_t)dout_b % 16 == 0 && (uintptr_t)dres % 16 == 0,
            "ln_rows_bwd_add: x / gamma / dout_a / dx / dgamma / dbeta / ws must be non-null and 16-byte aligned, dout_b / dres 16-byte aligned or null");
    REQUIRE((const float*)dx != x && (const float*)dx != dout_a && (const float*)dx != dout_b,
            "ln_rows_bwd_add: dx must not alias x, dout_a or dout_b (dx == dres is the one in-place form)");
    mln_bwd_add_launch((hipStream_t)stream, x, gamma, dout_a, dout_b, dres, dx, dgamma, dbeta, (float*)ws, M, C, eps);
    CHECK_LAUNCH("ln_rows_bwd_add");
    return 0;
}
int cffm_nchw_ln_rows_bwd(const float* x_nchw, const float* gamma, const float* dout_rows, float* dx_nchw, float* dgamma, float* dbeta, void* ws,
                          int B, int C, int H, int W, float eps, void* stream) {
    TRY(mln_check_map("nchw_ln_rows_bwd", B, C, H, W, eps));
    REQUIRE(aligned16(x_nchw) && aligned16(gamma) && aligned16(dout_rows) && aligned16(dx_nchw) && aligned16(dgamma) && aligned16(dbeta) && aligned16(ws),
            "nchw_ln_rows_bwd: x_nchw / gamma / dout_rows / dx_nchw / dgamma / dbeta / ws must be non-null and 16-byte aligned");
    mln_bwd_launch(1, (hipStream_t)stream, x_nchw, gamma, dout_rows, dx_nchw, dgamma, dbeta, (float*)ws, (long)B * H * W, B, C, H * W, eps);
    CHECK_LAUNCH("nchw_ln_rows_bwd");
    return 0;
}
int cffm_ln_rows_nchw_bwd(const float* x_rows, const float* gamma, const float* dout_nchw, float* dx_rows, float* dgamma, float* dbeta, void* ws,
                          int B, int C, int H, int W, float eps, void* stream) {
    TRY(mln_check_map("ln_rows_nchw_bwd", B, C, H, W, eps));
    REQUIRE(aligned16(x_rows) && aligned16(gamma) && aligned16(dout_nchw) && aligned16(dx_rows) && aligned16(dgamma) && aligned16(dbeta) && aligned16(ws),
            "ln_rows_nchw_bwd: x_rows / gamma / dout_nchw / dx_rows / dgamma / dbeta / ws must be non-null and 16-byte aligned");
    mln_bwd_launch(2, (hipStream_t)stream, x_rows, gamma, dout_nchw, dx_rows, dgamma, dbeta, (float*)ws, (long)B * H * W, B, C, H * W, eps);
    CHECK_LAUNCH("ln_rows_nchw_bwd");
    return 0;
}

long cffm_mit_stage_infer_ws_floats(const cffm_mit_stage_cfg* c) {
    MitWs W;
    return mit_cfg_check("mit_stage_infer_ws_floats", c, &W) ? -1 : W.total;
}
int cffm_mit_stage_infer(const cffm_mit_stage_cfg* c, const cffm_mit_block_params* blocks, const float* embed_g, const float* embed_b,
                         const float* out_g, const float* out_b, const float* conv_nchw, float* out_nchw, float* ws, void* stream) {
    MitWs W;
    TRY(mit_cfg_check("mit_stage_infer", c, &W));
    TRY(mit_ptr_check("mit_stage_infer", c, blocks, embed_g, embed_b, out_g, out_b));
    REQUIRE(aligned16(conv_nchw) && aligned16(out_nchw) && aligned16(ws), "mit_stage_infer: conv_nchw / out_nchw / ws must be non-null and 16-byte aligned");
    REQUIRE(conv_nchw != out_nchw, "mit_stage_infer: input and output must not alias");
    hipStream_t st = (hipStream_t)stream;
    mln_launch(1, st, conv_nchw, embed_g, embed_b, ws + W.xa, W.M, c->B, c->C, W.N, c->eps_embed);
    TRY(mit_stage_body("mit_stage_infer", c, W, blocks, out_g, out_b, out_nchw, ws, st));
    CHECK_LAUNCH("mit_stage_infer");
    return 0;
}

int cffm_patch_embed_fwd(const float* x_nchw, const float* w, const float* b, const float* gamma, const float* beta, float* out_rows, int B,
                         int Cin, int H, int W, int Cout, int k, int stride, float eps, void* stream) {
    PembGeom G;
    TRY(pemb_check("patch_embed_fwd", B, Cin, H, W, Cout, k, stride, eps, &G));
    REQUIRE(aligned16(x_nchw) && aligned16(w) && aligned16(b) && aligned16(gamma) && aligned16(beta) && aligned16(out_rows),
            "patch_embed_fwd: x_nchw / w / b / gamma / beta / out_rows must be non-null and 16-byte aligned");
    REQUIRE((const float*)out_rows != x_nchw, "patch_embed_fwd: input and output must not alias");
    pemb_launch(k, (hipStream_t)stream, x_nchw, w, b, gamma, beta, out_rows, G, eps);
    CHECK_LAUNCH("patch_embed_fwd");
    return 0;
}

int cffm_patch_embed_fwd_train(const float* x_nchw, const float* w, const float* b, const float* gamma, const float* beta, float* out_rows,
                               float* z_rows, int B, int Cin, int H, int W, int Cout, int k, int stride, float eps, void* stream) {
    PembGeom G;
    TRY(pemb_check("patch_embed_fwd_train", B, Cin, H, W, Cout, k, stride, eps, &G));
    REQUIRE(aligned16(x_nchw) && aligned16(w) && aligned16(b) && aligned16(gamma) && aligned16(beta) && aligned16(out_rows) && aligned16(z_rows),
            "patch_embed_fwd_train: x_nchw / w / b / gamma / beta / out_rows / z_rows must be non-null and 16-byte aligned");
    REQUIRE((const float*)out_rows != x_nchw && (const float*)z_rows != x_nchw && out_rows != z_rows,
            "patch_embed_fwd_train: input and outputs must not alias");
    hipStream_t st = (hipStream_t)stream;
    if (k == 7) pemb_go<7, 4, true>(st, x_nchw, w, b, gamma, beta, out_rows, z_rows, G, eps);
    else pemb_go<3, 2, true>(st, x_nchw, w, b, gamma, beta, out_rows, z_rows, G, eps);
    CHECK_LAUNCH("patch_embed_fwd_train");
    return 0;
}
long cffm_patch_embed_bwd_workspace_bytes(int B, int Cin, int H, int W, int Cout, int k, int stride, int with_dx) {
    PembGeom G;
    if (pemb_check("patch_embed_bwd_workspace_bytes", B, Cin, H, W, Cout, k, stride, 0.f, &G)) return -1;
    if (with_dx && k != 3) return fail(-1, "patch_embed_bwd_workspace_bytes: the input gradient exists for (k, stride) = (3, 2) only");
    return pemb_bwd_layout(G, with_dx != 0).total * (long)sizeof(float);
}
int cffm_patch_embed_bwd(const float* x_nchw, const float* w, const float* gamma, const float* z_rows, const float* dout_rows, float* dx_nchw,
                         float* dw, float* db, float* dgamma, float* dbeta, void* workspace, int B, int Cin, int H, int W, int Cout, int k,
                         int stride, float eps, void* stream) {
    PembGeom G;
    TRY(pemb_check("patch_embed_bwd", B, Cin, H, W, Cout, k, stride, eps, &G));
    REQUIRE(!dx_nchw || k == 3, "patch_embed_bwd: the input gradient exists for (k, stride) = (3, 2) only: pass dx_nchw = NULL");
    REQUIRE(aligned16(x_nchw) && aligned16(w) && aligned16(gamma) && aligned16(z_rows) && aligned16(dout_rows) && aligned16(dw) && aligned16(db) &&
            aligned16(dgamma) && aligned16(dbeta) && aligned16(workspace) && (uintptr_t)dx_nchw % 16 == 0,
            "patch_embed_bwd: x_nchw / w / gamma / z_rows / dout_rows / dw / db / dgamma / dbeta / workspace must be non-null and 16-byte "
            "aligned, dx_nchw 16-byte aligned or null");
    pemb_bwd_launch(k, (hipStream_t)stream, x_nchw, w, gamma, z_rows, dout_rows, dx_nchw, dw, db, dgamma, dbeta, (float*)workspace, G, eps);
    CHECK_LAUNCH("patch_embed_bwd");
    return 0;
}

// ---- one Linear layer on token rows, forward and backward (gemm.h: gemm_rows_*) ----
// the limits of the three calls: what the tile loads can read (16-byte pieces along N and K, 32-bit byte offsets into an operand)
static int lrows_check(const char* who, long M, int N, int K, int rps) {
    REQUIRE(M >= 1 && N >= 4 && K >= 4 && N % 4 == 0 && K % 4 == 0, "%s: M=%ld N=%d K=%d: M must be at least 1, N and K multiples of 4", who, M, N, K);
    REQUIRE(rps >= 1 && M % rps == 0, "%s: M=%ld is no multiple of rows_per_sample=%d", who, M, rps);
    REQUIRE(M < (1L << 31) && M * std::max(N, K) < (1L << 30) && (long)N * K < (1L << 30),
            "%s: M*max(N, K) = %ld and N*K = %ld must be below 2^30", who, M * std::max(N, K), (long)N * K);
    return 0;
}
// workspace of cffm_linear_rows_bwd (floats, every carve 256-byte aligned): the dw slabs [ksplit][N][K] (ksplit > 1) | the db records [nrec][N]
struct LrowsWs { RowsBwdPlan P; long slab, rec, total; };
static LrowsWs lrows_layout(long M, int N, int K, int with_db) {
    LrowsWs W;
    W.P = gemm_rows_bwd_plan(M, N, K);
    long p = 0;
    W.slab = p; p += W.P.ksplit > 1 ? up((long)W.P.ksplit * N * K) : 0;
    W.rec = p; p += with_db ? up((long)W.P.nrec * N) : 0;
    W.total = p;
    return W;
}
int cffm_linear_rows_fwd(const float* x, const float* w, const float* b, const float* residual, const float* scale, float* y, long M, int N,
                         int K, int rows_per_sample, void* stream) {
    TRY(lrows_check("linear_rows_fwd", M, N, K, rows_per_sample));
    REQUIRE(aligned16(x) && aligned16(w) && aligned16(y) && (uintptr_t)b % 16 == 0 && (uintptr_t)residual % 16 == 0 && (uintptr_t)scale % 4 == 0,
            "linear_rows_fwd: x / w / y must be non-null and 16-byte aligned, b / residual 16-byte aligned or null, scale 4-byte aligned or null");
    REQUIRE((const float*)y != x && (const float*)y != w && (const float*)y != b && (const float*)y != residual && (const float*)y != scale,
            "linear_rows_fwd: y must not alias an input (x, w, b, residual, scale)");
    REQUIRE(gemm_rows_fwd(x, w, b, residual, scale, y, M, N, K, rows_per_sample, (hipStream_t)stream) == 0, "linear_rows_fwd: launch refused");
    CHECK_LAUNCH("linear_rows_fwd");
    return 0;
}
long cffm_linear_rows_bwd_workspace_bytes(long M, int N, int K, int rows_per_sample, int with_dx, int with_db) {
    (void)with_dx;      // the input gradient needs no workspace
    if (lrows_check("linear_rows_bwd_workspace_bytes", M, N, K, rows_per_sample)) return -1;
    return lrows_layout(M, N, K, with_db != 0).total * (long)sizeof(float);
}
int cffm_linear_rows_bwd(const float* dy, const float* x, const float* w, const float* scale, float* dx, float* dw, float* db, void* workspace,
                         long M, int N, int K, int rows_per_sample, void* stream) {
    TRY(lrows_check("linear_rows_bwd", M, N, K, rows_per_sample));
    const LrowsWs W = lrows_layout(M, N, K, db != nullptr);
    REQUIRE(aligned16(dy) && aligned16(x) && aligned16(w) && aligned16(dw) && (uintptr_t)dx % 16 == 0 && (uintptr_t)db % 16 == 0 &&
            (uintptr_t)scale % 4 == 0 && (uintptr_t)workspace % 16 == 0 && (workspace || !W.total),
            "linear_rows_bwd: dy / x / w / dw (and the workspace, unless its size is 0) must be non-null and 16-byte aligned, dx / db 16-byte "
            "aligned or null, scale 4-byte aligned or null");
    const float* const ins[4] = {dy, x, w, scale};
    float* const outs[3] = {dx, dw, db};
    for (int o = 0; o < 3; ++o) {
        for (int i = 0; i < 4; ++i) REQUIRE(!outs[o] || (const float*)outs[o] != ins[i], "linear_rows_bwd: an output aliases an input");
        for (int q = 0; q < o; ++q) REQUIRE(!outs[o] || outs[o] != outs[q], "linear_rows_bwd: two outputs alias");
        REQUIRE(!outs[o] || !workspace || (void*)outs[o] != workspace, "linear_rows_bwd: an output aliases the workspace");
    }
    // (every refusal before the first launch: with dx enqueued, a refused dw would break "nothing is enqueued")
    REQUIRE(gemm_rows_bwd_grant(M, N, K, scale != nullptr, dx != nullptr, W.P), "linear_rows_bwd: LDS grant refused");
    hipStream_t st = (hipStream_t)stream;
    float* ws = (float*)workspace;
    if (dx) REQUIRE(gemm_rows_dx(dy, w, scale, dx, M, N, K, rows_per_sample, st) == 0, "linear_rows_bwd: launch refused (dx)");
    REQUIRE(gemm_rows_dw(dy, x, scale, dw, M, N, K, rows_per_sample, W.P, W.P.ksplit > 1 ? ws + W.slab : nullptr, st) == 0,
            "linear_rows_bwd: launch refused (dw)");
    if (db) gemm_rows_db(dy, scale, db, M, N, rows_per_sample, W.P, ws + W.rec, st);
    CHECK_LAUNCH("linear_rows_bwd");
    return 0;
}

// ---- the blocks of one MiT stage in a training pass: one call per direction (cffm_mit_blocks_train_*) ----
}  // extern "C"
// Float offsets.  `saved`: depth slices of `per` floats, one per block, in the order below (xout = the block's output, the next block's
// input: the last block has none, its output is y_rows).  The backward's workspace: g / g1, the running gradient and the gradient behind
// norm2's residual add, live across a block; `phase`, which the Mix-FFN half of a block's backward (da | dh | dwconv workspace | dz2) and
// then its attention half (dao | dq | dkv | attention workspace | dr | sr workspace | dz1a | dz1b) lay out anew; and the three carves every
// Linear / LayerNorm backward of the call shares, each the maximum over its users: the dw slabs, the db records, the LayerNorm records.
// The forward needs no workspace: every intermediate it makes is kept.
struct MitTrainLay {
    MitWs W;
    SrGeom SG;
    long z1, q, sz, sstats, r, kv, ao, lse, x1, z2, h, a, xout, per, saved_total;
    long g, g1, phase, da, dh, dwgws, dz2, dao, dq, dkv, sraws, dr, srws, dz1a, dz1b, slab, rec, lnrec, bwd_total;
};
struct MitLin { long M; int N, K; };
static void mit_train_linears(const cffm_mit_stage_cfg* c, const MitWs& W, MitLin (&L)[5]) {     // q | kv | proj | fc1 | fc2
    const long Mk = (long)c->B * W.Nk;
    L[0] = {W.M, c->C, c->C}; L[1] = {Mk, 2 * c->C, c->C}; L[2] = {W.M, c->C, c->C}; L[3] = {W.M, c->hidden, c->C}; L[4] = {W.M, c->C, c->hidden};
}
static int mit_train_check(const char* who, const cffm_mit_stage_cfg* c0, cffm_mit_stage_cfg* co, MitTrainLay* Lo) {
    REQUIRE(c0, "%s: null cfg", who);
    cffm_mit_stage_cfg c = *c0;
    c.eps_embed = c.eps_out = 0.f;                               // (not read by these calls)
    MitTrainLay L = {};
    TRY(mit_cfg_check(who, &c, &L.W));
    const int s = c.sr_ratio, C = c.C, hid = c.hidden;
    if (s > 1) TRY(srln_check(who, c.B, c.H, c.W, C, s, c.eps_sr, &L.SG));
    TRY(mln_check(who, C, c.eps_block));
    MitLin lin[5];
    mit_train_linears(&c, L.W, lin);
    for (const MitLin& l : lin) TRY(lrows_check(who, l.M, l.N, l.K, 1));
    const long MC = L.W.M * C, KC = (long)c.B * L.W.Nk * C, MH = L.W.M * hid;
    long p = 0;
    L.z1 = p; p += up(MC);
    L.q = p; p += up(MC);
    L.sz = p; p += s > 1 ? up(KC) : 0;
    L.sstats = p; p += s > 1 ? up(2L * c.B * L.W.Nk) : 0;
    L.r = p; p += s > 1 ? up(KC) : 0;
    L.kv = p; p += up(2 * KC);
    L.ao = p; p += up(MC);
    L.lse = p; p += up((long)c.B * c.heads * L.W.N);
    L.x1 = p; p += up(MC);
    L.z2 = p; p += up(MC);
    L.h = p; p += up(MH);
    L.a = p; p += up(MH);
    L.xout = p; p += up(MC);
    L.per = p;
    L.saved_total = (long)c.depth * L.per - up(MC);
    p = 0;
    L.g = p; p += up(MC);
    L.g1 = p; p += up(MC);
    L.phase = p;
    long m = p;                                                  // the Mix-FFN half
    L.da = m; m += up(MH);
    L.dh = m; m += up(MH);
    L.dwgws = m; m += up(dwg_bwd_ws_floats(c.B, c.H, c.W, hid));
    L.dz2 = m; m += up(MC);
    long a = p;                                                  // the attention half
    L.dao = a; a += up(MC);
    L.dq = a; a += up(MC);
    L.dkv = a; a += up(2 * KC);
    L.sraws = a; a += up(sra_bwd_ws_floats(c.B, L.W.N, L.W.Nk, c.heads, C / c.heads));
    L.dz1a = a; a += up(MC);
    L.dz1b = a; a += up(MC);
    L.dr = s > 1 ? a : L.dz1b; a += s > 1 ? up(KC) : 0;          // (sr_ratio 1: kv's input gradient IS dz1b)
    L.srws = a; a += s > 1 ? up(srln_bwd_ws_floats(L.SG)) : 0;
    p = std::max(m, a);
    long slab = 0, rec = 0;
    for (int i = 0; i < 5; ++i) {
        const RowsBwdPlan P = gemm_rows_bwd_plan(lin[i].M, lin[i].N, lin[i].K);
        slab = std::max(slab, P.ksplit > 1 ? (long)P.ksplit * lin[i].N * lin[i].K : 0L);
        rec = std::max(rec, (long)P.nrec * lin[i].N);
    }
    L.slab = p; p += up(slab);
    L.rec = p; p += up(rec);
    L.lnrec = p; p += up(mln_bwd_records(L.W.M, C, 1) * 2 * C);
    L.bwd_total = p;
    if (co) *co = c;
    if (Lo) *Lo = L;
    return 0;
}
// the pointers of both directions: the parameters as cffm_mit_stage_infer asks for them, the factors, and (backward) a gradient pointer
// exactly where there is a parameter
static int mit_train_ptr_check(const char* who, const cffm_mit_stage_cfg* c, const cffm_mit_block_params* blocks, const cffm_mit_block_scales* scales,
                               const cffm_mit_block_grad_ptrs* grads, bool bwd) {
    alignas(16) static const float dummy[4] = {0.f, 0.f, 0.f, 0.f};      // (the stage's own norms are not part of these calls)
    TRY(mit_ptr_check(who, c, blocks, dummy, dummy, dummy, dummy));
    for (int i = 0; scales && i < c->depth; ++i)
        REQUIRE((uintptr_t)scales[i].scale_attn % 4 == 0 && (uintptr_t)scales[i].scale_mlp % 4 == 0, "%s: block %d: a scale is not 4-byte aligned", who, i);
    if (!bwd) return 0;
    REQUIRE(grads, "%s: null gradient pointers", who);
    constexpr int NF = sizeof(cffm_mit_block_params) / sizeof(const float*);
    static_assert(sizeof(cffm_mit_block_grad_ptrs) == sizeof(cffm_mit_block_params), "the two structs have the same fields");
    for (int i = 0; i < c->depth; ++i) {
        const float* const* pp = (const float* const*)&blocks[i];
        float* const* gp = (float* const*)&grads[i];
        for (int f = 0; f < NF; ++f) {
            REQUIRE(!pp[f] == !gp[f] && (uintptr_t)gp[f] % 16 == 0,
                    "%s: block %d: gradient %d must be non-null exactly where the parameter is, and 16-byte aligned", who, i, f);
            REQUIRE((const float*)gp[f] != pp[f] || !gp[f], "%s: block %d: gradient %d aliases its parameter", who, i, f);
        }
    }
    return 0;
}
static int mit_train_alias_check(const char* who, const void* const* ptrs, const char* const* names, int n) {
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < i; ++j)
            REQUIRE(!ptrs[i] || ptrs[i] != ptrs[j], "%s: %s and %s must not alias", who, names[j], names[i]);
    return 0;
}
// one Linear layer's backward on the call's shared carves (cffm_linear_rows_bwd's three launches, in its order)
static int mit_train_linear_bwd(const float* dy, const float* x, const float* w, const float* s, float* dx, float* dw, float* db, const MitLin& l,
                                int rps, float* slab, float* rec, hipStream_t st) {
    const RowsBwdPlan P = gemm_rows_bwd_plan(l.M, l.N, l.K);
    if (gemm_rows_dx(dy, w, s, dx, l.M, l.N, l.K, rps, st)) return -1;
    if (gemm_rows_dw(dy, x, s, dw, l.M, l.N, l.K, rps, P, P.ksplit > 1 ? slab : nullptr, st)) return -1;
    if (db) gemm_rows_db(dy, s, db, l.M, l.N, rps, P, rec, st);
    return 0;
}
extern "C" {
long cffm_mit_blocks_train_saved_floats(const cffm_mit_stage_cfg* c) {
    MitTrainLay L;
    return mit_train_check("mit_blocks_train_saved_floats", c, nullptr, &L) ? -1 : L.saved_total;
}
long cffm_mit_blocks_train_fwd_ws_floats(const cffm_mit_stage_cfg* c) {
    return mit_train_check("mit_blocks_train_fwd_ws_floats", c, nullptr, nullptr) ? -1 : 0;
}
long cffm_mit_blocks_train_bwd_ws_floats(const cffm_mit_stage_cfg* c) {
    MitTrainLay L;
    return mit_train_check("mit_blocks_train_bwd_ws_floats", c, nullptr, &L) ? -1 : L.bwd_total;
}
int cffm_mit_blocks_train_fwd(const cffm_mit_stage_cfg* c0, const cffm_mit_block_params* blocks, const cffm_mit_block_scales* scales,
                              const float* x_rows, float* y_rows, float* saved, float* ws, void* stream) {
    const char* who = "mit_blocks_train_fwd";
    cffm_mit_stage_cfg c;
    MitTrainLay L;
    TRY(mit_train_check(who, c0, &c, &L));
    TRY(mit_train_ptr_check(who, &c, blocks, scales, nullptr, false));
    REQUIRE(aligned16(x_rows) && aligned16(y_rows) && aligned16(saved) && (uintptr_t)ws % 16 == 0,
            "%s: x_rows / y_rows / saved must be non-null and 16-byte aligned, ws 16-byte aligned (the forward needs none: NULL is accepted)", who);
    const void* const ptrs[] = {x_rows, y_rows, saved, ws};
    const char* const names[] = {"x_rows", "y_rows", "saved", "ws"};
    TRY(mit_train_alias_check(who, ptrs, names, 4));
    MitLin lin[5];
    mit_train_linears(&c, L.W, lin);
    for (const MitLin& l : lin)
        REQUIRE((gemm_split_grant<false, false, 8, 0, 0>((int)l.M, l.N, l.K, 1, 0)), "%s: LDS grant refused", who);
    hipStream_t st = (hipStream_t)stream;
    const int s = c.sr_ratio, B = c.B, C = c.C, hid = c.hidden, N = L.W.N, Nk = L.W.Nk;
    const long M = L.W.M;
    for (int i = 0; i < c.depth; ++i) {
        const cffm_mit_block_params& p = blocks[i];
        const float* sa = scales ? scales[i].scale_attn : nullptr;
        const float* sm = scales ? scales[i].scale_mlp : nullptr;
        float* S = saved + (long)i * L.per;
        const float* xin = i ? S - L.per + L.xout : x_rows;
        float* xout = i + 1 < c.depth ? S + L.xout : y_rows;
        mln_launch(0, st, xin, p.n1_g, p.n1_b, S + L.z1, M, 0, C, 1, c.eps_block);
        bool bad = gemm_rows_fwd(S + L.z1, p.q_w, p.q_b, nullptr, nullptr, S + L.q, M, C, C, (int)M, st) != 0;
        if (s > 1) srln_fwd_launch(s, st, S + L.z1, p.sr_w, p.sr_b, p.srn_g, p.srn_b, S + L.r, S + L.sz, S + L.sstats, L.SG, c.eps_sr);
        bad = bad || gemm_rows_fwd(s > 1 ? S + L.r : S + L.z1, p.kv_w, p.kv_b, nullptr, nullptr, S + L.kv, lin[1].M, 2 * C, C, (int)lin[1].M, st);
        sra_fwd_launch(S + L.q, S + L.kv, S + L.ao, S + L.lse, B, N, Nk, c.heads, C / c.heads, c.scale, st);
        bad = bad || gemm_rows_fwd(S + L.ao, p.proj_w, p.proj_b, xin, sa, S + L.x1, M, C, C, sa ? N : (int)M, st);
        mln_launch(0, st, S + L.x1, p.n2_g, p.n2_b, S + L.z2, M, 0, C, 1, c.eps_block);
        bad = bad || gemm_rows_fwd(S + L.z2, p.fc1_w, p.fc1_b, nullptr, nullptr, S + L.h, M, hid, C, (int)M, st);
        dwg_fwd_launch(S + L.h, p.dw_w, p.dw_b, S + L.a, B, c.H, c.W, hid, st);
        bad = bad || gemm_rows_fwd(S + L.a, p.fc2_w, p.fc2_b, S + L.x1, sm, xout, M, C, hid, sm ? N : (int)M, st);
        REQUIRE(!bad, "%s: launch refused", who);
    }
    CHECK_LAUNCH("mit_blocks_train_fwd");
    return 0;
}
int cffm_mit_blocks_train_bwd(const cffm_mit_stage_cfg* c0, const cffm_mit_block_params* blocks, const cffm_mit_block_scales* scales,
                              const cffm_mit_block_grad_ptrs* grads, const float* x_rows, const float* saved, const float* dy_rows, float* dx_rows,
                              float* ws, void* stream) {
    const char* who = "mit_blocks_train_bwd";
    cffm_mit_stage_cfg c;
    MitTrainLay L;
    TRY(mit_train_check(who, c0, &c, &L));
    TRY(mit_train_ptr_check(who, &c, blocks, scales, grads, true));
    REQUIRE(aligned16(x_rows) && aligned16(saved) && aligned16(dy_rows) && aligned16(dx_rows) && aligned16(ws),
            "%s: x_rows / saved / dy_rows / dx_rows / ws must be non-null and 16-byte aligned", who);
    const void* const ptrs[] = {x_rows, saved, dy_rows, dx_rows, ws};
    const char* const names[] = {"x_rows", "saved", "dy_rows", "dx_rows", "ws"};
    TRY(mit_train_alias_check(who, ptrs, names, 5));
    MitLin lin[5];
    mit_train_linears(&c, L.W, lin);
    for (int i = 0; i < 5; ++i) {
        // (a block's factor may be null where another's is not: both forms of the scaled layers are asked for when any factor is given)
        const RowsBwdPlan P = gemm_rows_bwd_plan(lin[i].M, lin[i].N, lin[i].K);
        REQUIRE(gemm_rows_bwd_grant(lin[i].M, lin[i].N, lin[i].K, false, true, P), "%s: LDS grant refused", who);
        if (scales && (i == 2 || i == 4)) REQUIRE(gemm_rows_bwd_grant(lin[i].M, lin[i].N, lin[i].K, true, true, P), "%s: LDS grant refused", who);
    }
    hipStream_t st = (hipStream_t)stream;
    const int s = c.sr_ratio, B = c.B, C = c.C, hid = c.hidden, N = L.W.N, Nk = L.W.Nk;
    const long M = L.W.M;
    float *gA = ws + L.g, *g1 = ws + L.g1, *slab = ws + L.slab, *rec = ws + L.rec, *lnrec = ws + L.lnrec;
    for (int i = c.depth - 1; i >= 0; --i) {
        const cffm_mit_block_params& p = blocks[i];
        const cffm_mit_block_grad_ptrs& d = grads[i];
        const float* sa = scales ? scales[i].scale_attn : nullptr;
        const float* sm = scales ? scales[i].scale_mlp : nullptr;
        const float* S = saved + (long)i * L.per;
        const float* xin = i ? S - L.per + L.xout : x_rows;
        const float* g = i + 1 < c.depth ? gA : dy_rows;
        float* gx = i ? gA : dx_rows;
        bool bad = mit_train_linear_bwd(g, S + L.a, p.fc2_w, sm, ws + L.da, d.fc2_w, d.fc2_b, lin[4], sm ? N : (int)M, slab, rec, st) != 0;
        dwg_bwd_launch(S + L.h, p.dw_w, p.dw_b, ws + L.da, ws + L.dh, d.dw_w, d.dw_b, ws + L.dwgws, B, c.H, c.W, hid, st);
        bad = bad || mit_train_linear_bwd(ws + L.dh, S + L.z2, p.fc1_w, nullptr, ws + L.dz2, d.fc1_w, d.fc1_b, lin[3], (int)M, slab, rec, st);
        mln_bwd_add_launch(st, S + L.x1, p.n2_g, ws + L.dz2, nullptr, g, g1, d.n2_g, d.n2_b, lnrec, M, C, c.eps_block);
        bad = bad || mit_train_linear_bwd(g1, S + L.ao, p.proj_w, sa, ws + L.dao, d.proj_w, d.proj_b, lin[2], sa ? N : (int)M, slab, rec, st);
        sra_bwd_launch(S + L.q, S + L.kv, S + L.ao, S + L.lse, ws + L.dao, ws + L.dq, ws + L.dkv, ws + L.sraws, B, N, Nk, c.heads, C / c.heads,
                       c.scale, st);
        bad = bad || mit_train_linear_bwd(ws + L.dkv, s > 1 ? S + L.r : S + L.z1, p.kv_w, nullptr, ws + L.dr, d.kv_w, d.kv_b, lin[1], (int)lin[1].M,
                                          slab, rec, st);
        if (s > 1)
            srln_bwd_launch(s, st, S + L.z1, p.sr_w, p.srn_g, S + L.sz, S + L.sstats, ws + L.dr, ws + L.dz1b, d.sr_w, d.sr_b, d.srn_g, d.srn_b,
                            ws + L.srws, L.SG);
        bad = bad || mit_train_linear_bwd(ws + L.dq, S + L.z1, p.q_w, nullptr, ws + L.dz1a, d.q_w, d.q_b, lin[0], (int)M, slab, rec, st);
        mln_bwd_add_launch(st, xin, p.n1_g, ws + L.dz1a, ws + L.dz1b, g1, gx, d.n1_g, d.n1_b, lnrec, M, C, c.eps_block);
        REQUIRE(!bad, "%s: launch refused", who);
    }
    CHECK_LAUNCH("mit_blocks_train_bwd");
    return 0;
}

long cffm_mit_infer_ws_floats(const cffm_mit_stage* stages, int n) {
    long need = 0;
    return mit_infer_check("mit_infer_ws_floats", stages, n, nullptr, nullptr, &need) ? -1 : need;
}
int cffm_mit_infer(const cffm_mit_stage* stages, int n, const float* x_nchw, float* const* outs, float* ws, void* stream) {
    MitWs W[4];
    PembGeom PG[4];
    long need = 0;
    TRY(mit_infer_check("mit_infer", stages, n, W, PG, &need));
    REQUIRE(outs, "mit_infer: null output list");
    REQUIRE(aligned16(x_nchw) && aligned16(ws), "mit_infer: x_nchw / ws must be non-null and 16-byte aligned");
    for (int i = 0; i < n; ++i) {
        const cffm_mit_stage& s = stages[i];
        REQUIRE(aligned16(outs[i]), "mit_infer: stage %d: the output must be non-null and 16-byte aligned", i);
        REQUIRE((const float*)outs[i] != x_nchw, "mit_infer: stage %d: input and output must not alias", i);
        for (int j = 0; j < i; ++j) REQUIRE(outs[i] != outs[j], "mit_infer: outputs %d and %d alias", j, i);
        REQUIRE(aligned16(s.conv_w) && aligned16(s.conv_b), "mit_infer: stage %d: conv_w / conv_b must be non-null and 16-byte aligned", i);
        TRY(mit_ptr_check("mit_infer", &s.cfg, s.blocks, s.embed_g, s.embed_b, s.out_g, s.out_b));
    }
    hipStream_t st = (hipStream_t)stream;
    const float* in = x_nchw;
    for (int i = 0; i < n; ++i) {
        const cffm_mit_stage& s = stages[i];
        // the embedding's normalised rows go straight into the residual buffer the first block reads
        pemb_launch(s.k, st, in, s.conv_w, s.conv_b, s.embed_g, s.embed_b, ws + W[i].xa, PG[i], s.cfg.eps_embed);
        TRY(mit_stage_body("mit_infer", &s.cfg, W[i], s.blocks, s.out_g, s.out_b, outs[i], ws, st));
        in = outs[i];
    }
    CHECK_LAUNCH("mit_infer");
    return 0;
}

}  // extern "C"

#ifdef CFFM_EMU
#include "hipemu_impl.h"
#endif
