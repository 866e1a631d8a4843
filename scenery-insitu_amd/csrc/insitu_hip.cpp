// insitu_hip.cpp -- host side of libinsitu_hip.so: the C ABI declared in include/insitu_hip.h.
//
// Owns the per-rank device state of the in-situ frame (bricks, transfer function, sub-VDI
// send/receive blocks, octree counters, composited strip, gathered image) and orders the
// four stages on one HIP stream:
//   render    -> VDIGenerator.comp+AccumulateVDI.comp / VolumeRaycaster.comp+AccumulatePlainImage.comp
//   exchange  -> distributeVDIs' MPI_Alltoall (DistributedVolumes.kt:860), here RCCL send/recv
//                of contiguous screen-strip blocks over xGMI
//   composite -> PlainImageCompositor.comp / VDI flatten (VDIGenerator.comp:147-185)
//   gather    -> gatherCompositedVDIs' MPI_Gather (DistributedVolumes.kt:903), RCCL to rank 0
#include "insitu_hip.h"
#include "insitu_kernels.h"
#include "vdi_pack_format.h"
#include "vdi_view_layout.h"

#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <cmath>
#include <cstdio>
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#pragma clang fp contract(off)

using namespace insitu;

namespace {

thread_local std::string g_create_error;

int fail(insitu_ctx* c, int code, const std::string& msg);

// Owner of one device allocation of `count()` elements (Pinned: of page-locked host memory), freed when it goes
// out of scope: with the context, a frame slot, the view state or a brick, or at the end of a readback.  Reads as
// the T* it holds.
template <typename T, bool Pinned = false>
class DevBuf {
public:
    DevBuf() = default;
    DevBuf(DevBuf&& o) noexcept : p_(o.p_), n_(o.n_) { o.p_ = nullptr; o.n_ = 0; }
    DevBuf& operator=(DevBuf&& o) noexcept {
        if (this != &o) {
            reset();
            std::swap(p_, o.p_);
            std::swap(n_, o.n_);
        }
        return *this;
    }
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    ~DevBuf() { reset(); }

    operator T*() const { return p_; }
    T* operator->() const { return p_; }
    T* get() const { return p_; }
    size_t count() const { return n_; }

    void reset() {
        if (p_) (void)(Pinned ? hipHostFree(p_) : hipFree(p_));
        p_ = nullptr;
        n_ = 0;
    }
    // frees what it holds, then allocates `count` elements (0: none); on failure it is left empty and the error is
    // returned, not reported
    hipError_t try_alloc(size_t count) {
        reset();
        if (count == 0) return hipSuccess;
        const hipError_t e = Pinned ? hipHostMalloc((void**)&p_, count * sizeof(T), 0) : hipMalloc((void**)&p_, count * sizeof(T));
        if (e != hipSuccess) {
            p_ = nullptr;
            (void)hipGetLastError();
            return e;
        }
        n_ = count;
        return hipSuccess;
    }
    // the same, reporting a failure as the context's error (code -5)
    int alloc(insitu_ctx* c, size_t count) {
        const hipError_t e = try_alloc(count);
        if (e == hipSuccess) return 0;
        return fail(c, -5, std::string(Pinned ? "hipHostMalloc of " : "hipMalloc of ") + std::to_string(count * sizeof(T)) +
                               " bytes failed: " + hipGetErrorString(e));
    }
    // grow-only: keeps what it holds when that is large enough
    int reserve(insitu_ctx* c, size_t count) { return count <= n_ ? 0 : alloc(c, count); }

private:
    T* p_ = nullptr;
    size_t n_ = 0;
};
template <typename T>
using PinnedBuf = DevBuf<T, true>;

struct Brick {
    DevBuf<unsigned char> d;            // blocked layout with halo (insitu_sampling.h)
    int dtype = -1;
    int dims[3] = {0, 0, 0};
    float im[16];
    bool valid = false;
};

size_t dtype_size(int dt) { return dt == INSITU_U8 ? 1 : (dt == INSITU_U16 ? 2 : 4); }

// float mat4 product with the same operation order as the shaders' `A * B` (and the oracle)
void mat4_mul_f(const float* a, const float* b, float* out) {
    float t[16];
    for (int c = 0; c < 4; ++c) {
        const float x = b[c * 4 + 0], y = b[c * 4 + 1], z = b[c * 4 + 2], w = b[c * 4 + 3];
        for (int r = 0; r < 4; ++r)
            t[c * 4 + r] = std::fmaf(a[12 + r], w, std::fmaf(a[8 + r], z, std::fmaf(a[4 + r], y, a[r] * x)));
    }
    std::memcpy(out, t, sizeof t);
}

// general 4x4 inverse in double, rounded to float (column-major in and out)
bool mat4_inverse(const float* m, float* out) {
    double a[4][8];
    for (int r = 0; r < 4; ++r) {
        for (int c = 0; c < 4; ++c) a[r][c] = (double)m[c * 4 + r];
        for (int c = 0; c < 4; ++c) a[r][4 + c] = (r == c) ? 1.0 : 0.0;
    }
    for (int col = 0; col < 4; ++col) {
        int piv = col;
        for (int r = col + 1; r < 4; ++r)
            if (std::fabs(a[r][col]) > std::fabs(a[piv][col])) piv = r;
        if (a[piv][col] == 0.0) return false;
        if (piv != col)
            for (int c = 0; c < 8; ++c) std::swap(a[piv][c], a[col][c]);
        const double inv = 1.0 / a[col][col];
        for (int c = 0; c < 8; ++c) a[col][c] *= inv;
        for (int r = 0; r < 4; ++r) {
            if (r == col) continue;
            const double f = a[r][col];
            for (int c = 0; c < 8; ++c) a[r][c] -= f * a[col][c];
        }
    }
    for (int r = 0; r < 4; ++r)
        for (int c = 0; c < 4; ++c) out[c * 4 + r] = (float)a[r][4 + c];
    return true;
}

}  // namespace

struct insitu_local_group {
    std::vector<insitu_ctx*> ranks;
};

// tuning knobs of the VDI generator (insitu_set_option; seeded from the environment at create)
struct Tuning {
    long long exact_search = 0;
    long long search_depth = 0;
    long long long_samples = 384;   // measured optimum
    long long round_batch = 28;     // round 5: 28 vs 20, three A/Bs on one box each: search -0.1 to -0.2 ms
    long long search_oversub = 6;   // measured: one brick per GPU (N=8) 12.2 -> 10.9 ms, N=1..4 unchanged
    long long pipe_oversub = 3;     // pipelined frames (their search overlaps the next first pass): emulated N=8
                                    // share 4.62 -> 4.18 ms/frame, N=4 6.11 -> 5.62, N=1..2 unchanged
    long long pipe_search_rays = 2048;   // pipelined frames: queued rays per searching block (0: the full grid)
    long long tile_order = 1;       // sampling tiles longest-first
    long long super_tile = 1;       // ... by the longest ray of super-tiles of this many tiles per edge
    long long regroup = 1;          // search: deeper tree groups for the rays left once the queue is drained
    long long exact_tile_keys = 0;  // 1: tile keys from all 64 rays of a tile (0: 16 of them)
};

// hipEvents of a frame (FrameSlot::ev).  EvRenderStart..EvGatherEnd stay consecutive: the stage times of
// insitu_get_stats are the spans ev[i], ev[i + 1] over them.
enum FrameEvent {
    EvRenderStart = 0,
    EvRenderEnd,       // the send buffers are ready
    EvExchangeEnd,
    EvCompositeEnd,
    EvGatherEnd,
    EvSampleEnd,       // sample / search split
    EvCompactStart,
    EvPeerReadsDone,   // (local group) this rank's copies out of its peers' buffers are done -- recorded after its
                       // exchange and its gather; a peer's next render/composite waits on it before rewriting them
    EvCountsIn,        // exchange counts in
    EvPayloadStart,
    EvImageOnHost,     // the root's image copied to the host buffer of insitu_gather
    EvSlotFree,        // (pipelined) the frame's completion is done: its slot may be rendered into again
    EvCompactEnd,
    EvSearchEnd,       // (pipelined) the next frame's sampling may start (trigger mode 0)
    kFrameEvents
};

// The generator's per-frame buffers and the frame's camera, events and stage flags.  Pipelined frames
// (insitu_frame_pipelined) render frame k+1 into one slot while frame k is composited from the other.  The stage
// functions (render_frame .. gather_frame) and their helpers are handed the slot they work on and the stream(s)
// they enqueue on; insitu_ctx::cur and ::alt only say which slot holds what (below).  Unpipelined contexts use
// one slot (the other stays empty).
struct FrameSlot {
    DevBuf<float4> vcol_send;
    DevBuf<float2> vdep_send;
    DevBuf<uint32_t> octree;
    DevBuf<uint8_t> passes;
    DevBuf<uint16_t> seg_pending;       // per brick and pixel: supersegments awaiting vdi_finish_kernel
    DevBuf<uint16_t> seg_steps;         // per sub-VDI entry: step count of a deferred colour
    DevBuf<GenCounters> counters;       // cache cursor + search queue counters
    DevBuf<PendingRay> queue;           // rays queued for the search kernel (B*W*H)
    DevBuf<float> cache;                // per-sample raymarch cache (32-byte chunks of 4 samples)
    uint32_t cache_chunks = 0;          // its size as the kernels take it (0 while a reallocation has failed)
    // default-sized caches (insitu_ctx::cache_adaptive) grow to the measured demand: the frame's cursor (chunks
    // asked for) is copied to pinned h_ctr at the end of every render, read after the next synchronisation
    uint32_t cache_grow_to = 0;         // > cache_chunks: reallocate before the next render
    bool cache_sized = false;           // the default cache was sized from a frame's measured demand
    PinnedBuf<GenCounters> h_ctr;       // pinned copy of `counters` (valid after a synchronisation)
    bool h_ctr_pending = false;         // h_ctr's copy was enqueued and not yet observed after a synchronisation
    bool h_ctr_valid = false;           // h_ctr holds the last render's counters (observed after a synchronisation)
    bool search_launched = false;       // a render ran the persistent search kernel (fault flag valid)
    DevBuf<uint32_t> tile_keys;         // longest-tiles-first order: keys / ids (2 x B*tiles each)
    DevBuf<uint32_t> tile_ids;
    DevBuf<unsigned char> sort_tmp;     // hipcub temporary storage (insitu_ctx::sort_tmp_bytes)
    float ipv[16] = {}, pv[16] = {}, view[16] = {};
    bool rendered = false, composited = false;
    bool exchanged = false;             // the compositor's input lists are complete (VDI set readable)
    bool pipelined = false;   // rendered by insitu_frame_pipelined (compaction runs with the completion)
    hipStream_t search_stream = nullptr;   // pipelined: the slot's search, finish and counter copy run here
    int flag_index = 0;                    // the slot's index in insitu_ctx::slots; pipelined: its drain trigger
                                           // is insitu_ctx::pipe_flag[flag_index]
    unsigned long long flag_value = 0;     // the last value a search of this slot stores to that flag (0: none yet);
                                           // the slot's frames are sequential, so each stores one more than the last
    hipEvent_t ev[kFrameEvents] = {};      // (FrameEvent above)
    bool ev_valid[kFrameEvents] = {};
};

// The bound VDI of insitu_view_bind / insitu_view_bind_host -- a snapshot in the view layout, with its generating
// camera -- and the output of the last insitu_view_render.  Its buffers belong to no frame slot and its work
// runs on a stream of its own, which is idle between calls (both calls block).
struct ViewState {
    DevBuf<float4> col;                 // the snapshot's buffers (grown by a larger bind) ...
    DevBuf<float2> dep;
    DevBuf<uint8_t> cnt, tmax;
    ViewVdi vdi{};                      // ... as the kernels take them, with its dimensions (view_reserve)
    float pv_g[16] = {};                // proj * view of the generating camera
    bool bound = false;
    DevBuf<float4> out_color;           // (out_h, out_w) rgba32f / rgba8 of the last render (grown by a larger one)
    DevBuf<uint32_t> out_image;
    int out_w = 0, out_h = 0;           // of the last render (0: none yet)
    hipStream_t stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    float ms = 0.0f;                    // the last render's kernel
    long long skip = 1;                 // INSITU_OPT_VIEW_SKIP
    // the compact view layout: vdi.loc != null says the bound VDI has it
    long long compact_next = 0;         // INSITU_OPT_VIEW_COMPACT: the layout the next bind takes
    DevBuf<uint16_t> loc;               // a pixel's entries before it in its block (vdi.boff is pk_boff)
    // the packed stream of the bound VDI (insitu_view_pack, insitu_view_bind_packed; vdi_pack.hip)
    bool counted = false;               // pk_boff and pk_E describe the bound VDI (once per bind; view_reserve clears it)
    unsigned long long pk_E = 0;        // its stored entries
    DevBuf<uint32_t> pk_bstat;          // PackOffsets of the bound VDI, a block each (grown by a larger bind)
    DevBuf<unsigned long long> pk_boff;
    DevBuf<PackTotals> pk_totals;       // device; read back through h_totals (pinned)
    PinnedBuf<PackTotals> h_totals;
    DevBuf<unsigned char> pk_stage;     // the depth and colour sections on the device, kept across calls
    float ms_pack = 0.0f;               // the last pack's or unpack's kernels
    // the merged bind (INSITU_VIEW_MERGED, insitu_view_bind_host_set; vdi_view_merge.hip)
    DevBuf<MergeTotals> mg_totals;      // device; read back through h_mg_totals (pinned)
    PinnedBuf<MergeTotals> h_mg_totals;
    long long overlaps = 0;             // of the bound VDI (0 for the single-VDI binds)
    float ms_bind = 0.0f;               // the last bind's kernels
};

struct insitu_ctx {
    insitu_config cfg{};
    insitu_local_group* group = nullptr;   // in-process rank group (test transport), else RCCL
    int W = 0, H = 0, S = 0, N = 1, rank = 0, B = 1, V = 1, mode = INSITU_MODE_VDI;
    int BV = 1;   // sub-VDIs per rank: B, or 1 when the bricks are the volumes of one VDI (merge_bricks)
    int strip_w = 0, strip_tiles = 0, rows = 0, ncx = 0, ncy = 0;
    size_t blockE = 0;      // VDI entries per (strip, brick) block
    size_t plainBlock = 0;  // pixels per (strip, brick) block in plain mode
    size_t stripPx = 0;     // pixels of one composited strip
    hipStream_t stream = nullptr;
    bool own_stream = false;
    ncclComm_t comm = nullptr;
    std::vector<Brick> bricks;
    DevBuf<float> d_tf;
    DevBuf<float> d_cmap;
    int n_tf = 0, n_cm = 0;
    float cmag = 1.0f;                  // TransferDesc::cmag of the current LUTs
    float conv_scale = 1.0f, conv_offset = 0.0f;
    DevBuf<float4> d_vcol_recv;
    DevBuf<float2> d_vdep_recv;
    DevBuf<uint32_t> d_pcol_send;
    DevBuf<uint32_t> d_pdep_send;
    DevBuf<uint32_t> d_pcol_recv;
    DevBuf<uint32_t> d_pdep_recv;
    DevBuf<uint32_t> d_strip;
    DevBuf<uint32_t> d_gather;
    DevBuf<uint32_t> d_image;
    DevBuf<float4> d_ref_col;           // reference-layout staging for insitu_distribute_vdis: send | recv
    DevBuf<float> d_ref_dep;
    DevBuf<uint16_t> d_ref_cnt;         // per source strip [y][xl] counts of the host-buffer path's lists
    bool lists_from_reference = false;  // the last composite input came through insitu_distribute_vdis
    // variable-length exchange (N > 1, VDI mode): compact messages per destination
    DevBuf<float4> d_ccol_send;         // [d] regions of B*blockE entries
    DevBuf<float2> d_cdep_send;
    DevBuf<uint8_t> d_meta_send;        // [d] regions of meta_bytes
    DevBuf<uint8_t> d_meta_recv;        // [s]
    DevBuf<uint32_t> d_cursor;          // [d] entries packed for d | [N + s] entries received from s
    PinnedBuf<uint32_t> h_tot;          // pinned copy of d_cursor
    size_t meta_bytes = 0;
    bool camera_set = false;
    DevBuf<unsigned char> d_staging;    // host-buffer brick uploads (kept: re-ingest every N frames)
    bool cache_adaptive = false;        // a default-sized sample cache: the slots' caches grow (FrameSlot)
    size_t cache_max_chunks = 0;        // growth limit (45 % of the HBM free at create, 2^32 chunks)
    int num_cus = 256;
    int search_blocks = 0;
    int search_lanes = 0;               // resident lanes of the search grid for the LUT sizes below
    int search_lanes_tf = -1, search_lanes_cm = -1;
    Tuning tune;
    DevBuf<unsigned long long> d_dbg;      // INSITU_DEBUG_RAYS: per-round search timing
    size_t sort_tmp_bytes = 0;          // of the slots' hipcub temporary storage
    size_t dbg_entries = 0;
    std::string dbg_path;
    bool dbg_pending = false;
    long long last_exchange_bytes = 0, last_exchange_entries = 0;
    bool composite_vdi = false;         // VDICompositor output instead of the RGBA flatten
    int S_out = 0;
    size_t cblockE = 0;                 // composited-VDI entries per strip block (S_out slots)
    DevBuf<float4> d_cvdi_col;          // this rank's composited strip (non-root ranks)
    DevBuf<float2> d_cvdi_dep;
    DevBuf<float4> d_gvdi_col;          // root: gathered composited strips [rank][block]
    DevBuf<float2> d_gvdi_dep;
    bool gvdi_valid = false;            // root: a gather has filled them, from the frame of camera gvdi_pv
    float gvdi_pv[16] = {};
    DevBuf<uint16_t> d_cvdi_cnt;        // per pixel of this rank's composited strip: slots written (non-root ranks)
    DevBuf<uint16_t> d_gvdi_cnt;        // root: the gathered counts [rank][y][x_local]
    DevBuf<uint8_t> d_cpasses;          // compositor search passes of the strip
    DevBuf<float4> d_cseq;              // VDICompositor merge cache (kCompEntryF4 float4 per entry)
    DevBuf<unsigned long long> d_cseq_cursor;
    PinnedBuf<unsigned long long> h_cseq_demand;   // pinned: the last composite's demand (entries), written
                                                   // by an async copy; read only by cache_observe after a sync
    bool cseq_pending = false;          // that copy is enqueued and not yet observed
    unsigned long long cseq_demand = 0; // the demand observed after the last composite's synchronisation
    unsigned long long cseq_cap = 0;    // capacity (entries)
    unsigned long long cseq_max = 0;    // growth limit (entries): 20 % of the HBM free at create
    // the frame slots: `cur` holds the completed frame (what the unpipelined stage calls and the readers work
    // on) and is the slot the next pipelined frame renders into.  Cross-frame pipelining
    // (insitu_frame_pipelined, DistributedVolumeRenderer.kt:530-542: the composite is one frame stale) fills
    // the second one, `alt` -- the frame in flight -- and adds the sampling and completion streams and the
    // trigger flags below
    FrameSlot slots[2];
    FrameSlot* cur = &slots[0];
    FrameSlot* alt = &slots[1];
    insitu_ctx() { slots[1].flag_index = 1; }
    insitu_ctx(const insitu_ctx&) = delete;   // (cur and alt point into the context)
    insitu_ctx& operator=(const insitu_ctx&) = delete;
    bool pipe_ready = false;            // *alt allocated, streams created
    bool pipe_inflight = false;         // *alt holds a rendered frame whose completion is pending
    bool ingest_batch = false;          // re-ingests since the last render: ev_ingest0 marks their start
    hipEvent_t ev_ingest0 = nullptr, ev_ingest = nullptr;   // the last batch of re-ingests (start, end)
    hipEvent_t ev_gate = nullptr;       // pipelined: `stream`'s work so far, waited for by the next first pass
    hipStream_t pipe_sample = nullptr;  // the first pass of every pipelined frame (low priority)
    hipStream_t pipe_comp = nullptr;    // exchange, composite, gather of the frame one behind (high priority)
    // search-drain triggers, one per slot (device memory, written at system scope): a slot's frames are
    // sequential, so its flag only grows (FrameSlot::flag_value) -- two slots' searches may overlap and drain
    // in either order
    DevBuf<unsigned long long> pipe_flag;
    long long pipe_frames = 0;          // frame index of the next pipelined render
    int pipe_trigger = 2;               // 0: after the previous search; 1: at its queue drain; 2: none (default:
                                        // the search keeps only the blocks its queue needs)
    bool pipe_wait_value = true;        // hipStreamWaitValue64 works here (else mode 1 falls back to 0)
    ViewState view;
    std::string err;
};

namespace {

int fail(insitu_ctx* c, int code, const std::string& msg) {
    if (c) c->err = msg;
    else g_create_error = msg;
    return code;
}

#define HIPCHK(ctx, expr)                                                                          \
    do {                                                                                           \
        hipError_t e_ = (expr);                                                                    \
        if (e_ != hipSuccess)                                                                      \
            return fail(ctx, -3, std::string(#expr " failed: ") + hipGetErrorString(e_));          \
    } while (0)

#define NCCLCHK(ctx, expr)                                                                         \
    do {                                                                                           \
        ncclResult_t r_ = (expr);                                                                  \
        if (r_ != ncclSuccess)                                                                     \
            return fail(ctx, -4, std::string(#expr " failed: ") + ncclGetErrorString(r_));         \
    } while (0)

// Everything of a context that is not memory: its streams' work first, then the events, the streams, the
// communicator and the local-group slot.  The memory (every DevBuf of the context, its slots, view and bricks) is
// freed after it, when the caller deletes the context with the device still current.
void release(insitu_ctx* c) {
    if (!c) return;
    (void)hipSetDevice(c->cfg.device);
    // every stream first: a pipelined frame left in flight (no insitu_pipeline_flush) still runs on the sampling,
    // search and completion streams and reads the buffers, events and trigger flags (each of its waits has its
    // producer enqueued ahead of it, so these synchronisations end)
    for (hipStream_t st : {c->stream, c->pipe_sample, c->pipe_comp, c->view.stream})
        if (st) (void)hipStreamSynchronize(st);
    for (FrameSlot& f : c->slots)
        if (f.search_stream) (void)hipStreamSynchronize(f.search_stream);
    for (FrameSlot& f : c->slots) {
        for (auto& e : f.ev)
            if (e) (void)hipEventDestroy(e);
        if (f.search_stream) (void)hipStreamDestroy(f.search_stream);
    }
    for (hipEvent_t e : {c->view.ev0, c->view.ev1, c->ev_ingest, c->ev_ingest0, c->ev_gate})
        if (e) (void)hipEventDestroy(e);
    for (hipStream_t st : {c->view.stream, c->pipe_sample, c->pipe_comp})
        if (st) (void)hipStreamDestroy(st);
    if (c->comm) ncclCommDestroy(c->comm);
    if (c->group && c->rank < (int)c->group->ranks.size() && c->group->ranks[c->rank] == c) c->group->ranks[c->rank] = nullptr;
    if (c->own_stream && c->stream) (void)hipStreamDestroy(c->stream);
}

bool is_root(const insitu_ctx* c) { return c->rank == 0; }

// the other frame slot becomes the current one
void swap_slot(insitu_ctx* c) { std::swap(c->cur, c->alt); }

// the completed frame's slot and the stream its readbacks run on: with a pipelined frame in flight the completion
// stream (the context stream may be busy with work for the next frame, the completion stream holds nothing of it)
struct CompletedFrame {
    FrameSlot& f;
    hipStream_t s;
};
CompletedFrame completed_frame(const insitu_ctx* c) { return {*c->cur, c->pipe_inflight ? c->pipe_comp : c->stream}; }

// after a synchronisation of the stream of slot f's last render: its cache demand (h_ctr) decides whether a
// default-sized cache grows before the slot's next render
void cache_observe(insitu_ctx* c, FrameSlot& f) {
    if (c->cseq_pending) {   // the compositor merge cache's demand (composite_frame grows it)
        c->cseq_pending = false;
        c->cseq_demand = *c->h_cseq_demand;
    }
    if (!f.h_ctr_pending) return;
    f.h_ctr_pending = false;
    f.h_ctr_valid = true;
    if (!c->cache_adaptive || f.h_ctr->march_rays == 0) return;
    const unsigned long long want = f.h_ctr->cache_cursor + f.h_ctr->cache_cursor / 4;
    const size_t to = std::min((size_t)want, c->cache_max_chunks);
    if (to > f.cache_chunks) f.cache_grow_to = (uint32_t)to;
}

// (re)allocate slot f's sample cache to `chunks` 32-byte units; on failure nothing is left allocated and the
// error is returned
hipError_t cache_realloc(FrameSlot& f, size_t chunks) {
    f.cache_chunks = 0;
    const hipError_t e = f.cache.try_alloc(chunks * 8);
    if (e == hipSuccess) f.cache_chunks = (uint32_t)chunks;
    return e;
}

// after a synchronisation of the stream of slot f's last render: did a persistent kernel of that render hit its
// wall-clock bound?
int check_fault(insitu_ctx* c, FrameSlot& f) {
    cache_observe(c, f);   // (a pending copy of the frame's counters reached h_ctr: we are after a synchronisation)
    if (!f.counters || !f.search_launched) return 0;
    uint32_t fault = 0;
    if (f.h_ctr_valid) fault = f.h_ctr->fault;
    else if (hipMemcpy(&fault, &f.counters->fault, sizeof fault, hipMemcpyDeviceToHost) != hipSuccess) fault = 1;
    if (fault) return fail(c, -6, "VDI search kernel exceeded its loop bound (internal error)");
    return 0;
}

// this rank's composited-VDI strip block (the root composites straight into its gather slot)
float4* cvdi_col(const insitu_ctx* c) { return c->rank == 0 ? c->d_gvdi_col : c->d_cvdi_col; }
float2* cvdi_dep(const insitu_ctx* c) { return c->rank == 0 ? c->d_gvdi_dep : c->d_cvdi_dep; }
uint16_t* cvdi_cnt(const insitu_ctx* c) { return c->rank == 0 ? c->d_gvdi_cnt : c->d_cvdi_cnt; }

// records slot f's event `i` on stream s
void record(FrameSlot& f, FrameEvent i, hipStream_t s) {
    if (hipEventRecord(f.ev[i], s) == hipSuccess) f.ev_valid[i] = true;
}

// N > 1, VDI mode: pack the stored supersegments of slot f's blocks bound for the other ranks into the compact
// messages (vdi_compact_kernel), on stream s, between EvCompactStart and EvCompactEnd
hipError_t compact_enqueue(insitu_ctx* c, FrameSlot& f, hipStream_t s) {
    record(f, EvCompactStart, s);
    hipError_t e = hipMemsetAsync(c->d_cursor, 0, sizeof(uint32_t) * (size_t)c->N, s);
    if (e != hipSuccess) return e;
    CompactParams cp{};
    cp.col = f.vcol_send;
    cp.dep = f.vdep_send;
    cp.pend = f.seg_pending;
    cp.pend_stride = (size_t)c->W * (size_t)c->H;
    cp.W = c->W; cp.H = c->H; cp.S = c->S; cp.B = c->BV; cp.nstrips = c->N; cp.strip_w = c->strip_w;
    cp.strip_tiles = c->strip_tiles; cp.ytiles = (c->H + 7) / 8; cp.skip_d = c->rank;
    cp.blockE = c->blockE;
    cp.out_col = c->d_ccol_send;
    cp.out_dep = c->d_cdep_send;
    cp.out_meta = c->d_meta_send;
    cp.meta_bytes = c->meta_bytes;
    cp.cursor = c->d_cursor;
    e = launch_vdi_compact(cp, s);
    if (e == hipSuccess) record(f, EvCompactEnd, s);
    return e;
}

// local group: before this rank rewrites buffers its peers copy from (send blocks, counts, strips),
// order stream s after the peers' last reads of them (write-after-read across streams)
hipError_t wait_peer_reads(insitu_ctx* c, hipStream_t s) {
    if (!c->group) return hipSuccess;
    for (const insitu_ctx* q : c->group->ranks) {
        if (!q || q == c || !q->cur->ev_valid[EvPeerReadsDone]) continue;
        hipError_t e = hipStreamWaitEvent(s, q->cur->ev[EvPeerReadsDone], 0);
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

// a frame slot's events (all a plain-mode slot needs)
int create_slot_events(insitu_ctx* c, FrameSlot& f) {
    for (auto& ev : f.ev)
        if (!ev && hipEventCreate(&ev) != hipSuccess) return fail(c, -3, "hipEventCreate failed");
    return 0;
}

// allocate one frame slot's generator buffers (VDI mode): send blocks, octree counters, pass counts, pending
// counts and step counts, generator counters, and -- with a sample cache of `chunks` 32-byte units -- the
// cache, the search queue, the pinned counter copy and the tile-order keys; plus the slot's events
int alloc_slot(insitu_ctx* c, FrameSlot& f, size_t chunks) {
    int rc = 0;
    if ((rc = create_slot_events(c, f))) return rc;
    const size_t sendE = (size_t)c->N * (size_t)c->BV * c->blockE;
    const size_t px = (size_t)c->BV * (size_t)c->W * (size_t)c->H;
    if ((rc = f.vcol_send.alloc(c, sendE)) || (rc = f.vdep_send.alloc(c, sendE))) return rc;
    const size_t oct = (size_t)c->BV * (size_t)c->S * (size_t)c->ncx * (size_t)c->ncy;
    if ((rc = f.octree.alloc(c, oct ? oct : 1))) return rc;
    if ((rc = f.seg_pending.alloc(c, px)) || (rc = f.seg_steps.alloc(c, sendE))) return rc;
    // per-pixel supersegment counts: empty until the first render (the slots are not zero-filled)
    if (hipMemset(f.seg_pending, 0, sizeof(uint16_t) * px) != hipSuccess)
        return fail(c, -3, "hipMemset of the supersegment counts failed");
    if (c->cfg.keep_passes && (rc = f.passes.alloc(c, px))) return rc;
    // generator counters, zeroed here so the fault flag reads 0 before any render (the host-buffer path
    // never renders)
    if ((rc = f.counters.alloc(c, 1))) return rc;
    if (hipMemset(f.counters, 0, sizeof(GenCounters)) != hipSuccess)
        return fail(c, -3, "hipMemset of the generator counters failed");
    if (chunks == 0) return 0;
    if ((rc = f.cache.alloc(c, chunks * 8)) || (rc = f.queue.alloc(c, (size_t)c->B * (size_t)c->W * (size_t)c->H)))
        return rc;
    if (f.h_ctr.try_alloc(1) != hipSuccess) return fail(c, -5, "hipHostMalloc of the generator counters failed");
    std::memset(f.h_ctr, 0, sizeof(GenCounters));
    f.cache_chunks = (uint32_t)chunks;
    // longest-tiles-first order of the sampling kernel: keys, ids and the sort's scratch (the key keeps 24
    // bits of tile position; super-tiles of up to 4x4 tiles pad the grid, so larger frames keep the order
    // only with super_tile 1: insitu_set_option checks that)
    const size_t ntile = (size_t)c->B * (size_t)((c->H + 7) / 8) * (size_t)c->N * (size_t)c->strip_tiles;
    if (ntile < ((size_t)1 << 24)) {
        size_t tb = 0;
        if (sort_tiles_desc(nullptr, tb, nullptr, nullptr, nullptr, nullptr, (int)ntile, nullptr) != hipSuccess)
            return fail(c, -3, "hipcub radix sort: temporary storage query failed");
        if ((rc = f.tile_keys.alloc(c, 2 * ntile)) || (rc = f.tile_ids.alloc(c, 2 * ntile)) ||
            (rc = f.sort_tmp.alloc(c, tb + 1)))
            return rc;
        c->sort_tmp_bytes = tb;
    }
    return 0;
}

// the padded tile count of super-tiles of `sup` tiles per edge: the sort key keeps 24 bits of tile position
size_t padded_tiles(const insitu_ctx* c, int sup) {
    return (size_t)c->B * (size_t)((((c->H + 7) / 8) + sup - 1) / sup * sup) *
           (size_t)((c->N * c->strip_tiles + sup - 1) / sup * sup);
}

}  // namespace

extern "C" {

int insitu_abi_version(void) { return INSITU_ABI_VERSION; }

int insitu_local_group_create(int nranks, insitu_local_group** out) {
    if (!out || nranks < 1 || nranks > kMaxLists) return fail(nullptr, -1, "insitu_local_group_create: bad arguments");
    *out = new insitu_local_group();
    (*out)->ranks.assign((size_t)nranks, nullptr);
    return 0;
}

void insitu_local_group_destroy(insitu_local_group* g) { delete g; }

int insitu_comm_id(void* out, size_t cap) {
    if (!out || cap < sizeof(ncclUniqueId)) return fail(nullptr, -1, "insitu_comm_id: buffer too small");
    ncclUniqueId id;
    ncclResult_t r = ncclGetUniqueId(&id);
    if (r != ncclSuccess) return fail(nullptr, -4, std::string("ncclGetUniqueId: ") + ncclGetErrorString(r));
    std::memcpy(out, &id, sizeof id);
    return 0;
}

const char* insitu_last_error(const insitu_ctx* ctx) { return ctx ? ctx->err.c_str() : g_create_error.c_str(); }

int insitu_create(const insitu_config* cfg, insitu_ctx** out) {
    if (!cfg || !out) return fail(nullptr, -1, "insitu_create: null argument");
    *out = nullptr;
    const insitu_config& k = *cfg;
    if (k.nranks < 1 || k.rank < 0 || k.rank >= k.nranks) return fail(nullptr, -1, "insitu_create: bad rank/nranks");
    if (k.width <= 0 || k.height <= 0) return fail(nullptr, -1, "insitu_create: bad window size");
    if (k.mode != INSITU_MODE_VDI && k.mode != INSITU_MODE_PLAIN) return fail(nullptr, -1, "insitu_create: bad mode");
    if (k.bricks_per_rank < 1 || k.bricks_per_rank > kMaxBricks)
        return fail(nullptr, -1, "insitu_create: bricks_per_rank must be in [1," + std::to_string(kMaxBricks) + "]");
    if (k.nranks * k.bricks_per_rank > kMaxLists)
        return fail(nullptr, -1, "insitu_create: nranks*bricks_per_rank exceeds " + std::to_string(kMaxLists));
    if (k.mode == INSITU_MODE_VDI && (k.max_supersegments < 1 || k.max_supersegments > 255))
        return fail(nullptr, -1, "insitu_create: max_supersegments must be in [1,255]");
    if (k.mode == INSITU_MODE_VDI && k.width % k.nranks != 0)
        return fail(nullptr, -1, "insitu_create: width must divide evenly into nranks screen strips");
    if (k.mode == INSITU_MODE_PLAIN && k.height % k.nranks != 0)
        return fail(nullptr, -1, "insitu_create: height (texture dim1) must divide evenly into nranks strips");
    if (k.nranks > 1 && !k.comm_id && !k.local_group)
        return fail(nullptr, -1, "insitu_create: comm_id (or local_group) required when nranks > 1");
    if (k.local_group && ((int)k.local_group->ranks.size() != k.nranks || k.local_group->ranks[k.rank]))
        return fail(nullptr, -1, "insitu_create: local_group size differs from nranks, or rank already taken");
    if (k.composite_vdi && k.mode != INSITU_MODE_VDI)
        return fail(nullptr, -1, "insitu_create: composite_vdi needs VDI mode");
    if (k.merge_bricks && k.mode != INSITU_MODE_VDI)
        return fail(nullptr, -1, "insitu_create: merge_bricks needs VDI mode");
    if (k.max_output_supersegments < 0 || k.max_output_supersegments > 255)
        return fail(nullptr, -1, "insitu_create: max_output_supersegments must be in [0,255]");
    if (k.faithful & ~(INSITU_FAITHFUL_COMPOSITOR_NDC_X | INSITU_FAITHFUL_PLAIN_NUM_PROCESSES))
        return fail(nullptr, -1, "insitu_create: unknown faithful bits");

    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev == 0) return fail(nullptr, -2, "insitu_create: no HIP device available");
    if (k.device < 0 || k.device >= ndev) return fail(nullptr, -2, "insitu_create: device index out of range");
    e = hipSetDevice(k.device);
    if (e != hipSuccess) return fail(nullptr, -2, std::string("hipSetDevice: ") + hipGetErrorString(e));

    insitu_ctx* c = new insitu_ctx();
    c->cfg = k;
    {
        hipDeviceProp_t prop;
        if (hipGetDeviceProperties(&prop, k.device) == hipSuccess && prop.multiProcessorCount > 0)
            c->num_cus = prop.multiProcessorCount;
    }
    c->cfg.comm_id = nullptr;
    c->W = k.width; c->H = k.height; c->N = k.nranks; c->rank = k.rank; c->B = k.bricks_per_rank;
    c->BV = (k.mode == INSITU_MODE_VDI && k.merge_bricks) ? 1 : c->B;
    c->V = c->N * c->BV; c->mode = k.mode;
    c->S = (k.mode == INSITU_MODE_VDI) ? k.max_supersegments : 1;
    c->bricks.resize(c->B);
    int rc = 0;
    auto bail = [&](int code) { std::string m = c->err; release(c); delete c; g_create_error = m; return code; };
    if (k.stream) {
        c->stream = (hipStream_t)k.stream;
    } else {
        if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess) {
            c->err = "hipStreamCreate failed";
            return bail(-3);
        }
        c->own_stream = true;
    }
    if (hipEventCreate(&c->ev_ingest0) != hipSuccess || hipEventCreate(&c->ev_ingest) != hipSuccess ||
        hipEventCreate(&c->ev_gate) != hipSuccess) {
        c->err = "hipEventCreate failed";
        return bail(-3);
    }

    if (c->mode == INSITU_MODE_VDI) {
        c->strip_w = c->W / c->N;
        c->strip_tiles = (c->strip_w + 7) / 8;
        c->blockE = (size_t)c->strip_tiles * (size_t)c->S * (size_t)c->H * 8;
        c->stripPx = (size_t)c->H * (size_t)c->strip_w;
        c->ncx = c->W / 8; c->ncy = c->H / 8;
        const size_t sendE = (size_t)c->N * (size_t)c->BV * c->blockE;
        if (c->N > 1) {
            // compact exchange: send regions per destination, receive regions per source, meta blocks
            c->meta_bytes = compact_meta_bytes(c->BV, c->strip_tiles, (c->H + 7) / 8);
            if ((rc = c->d_vcol_recv.alloc(c, sendE)) || (rc = c->d_vdep_recv.alloc(c, sendE)) ||
                (rc = c->d_ccol_send.alloc(c, sendE)) || (rc = c->d_cdep_send.alloc(c, sendE)) ||
                (rc = c->d_meta_send.alloc(c, (size_t)c->N * c->meta_bytes)) ||
                (rc = c->d_meta_recv.alloc(c, (size_t)c->N * c->meta_bytes)) ||
                (rc = c->d_cursor.alloc(c, 2 * (size_t)c->N)))
                return bail(rc);
            // received counts/offsets read as empty lists until the first exchange fills them
            if (hipMemset(c->d_meta_recv, 0, (size_t)c->N * c->meta_bytes) != hipSuccess) {
                c->err = "hipMemset of the exchange meta blocks failed";
                return bail(-3);
            }
            if (c->h_tot.try_alloc(2 * (size_t)c->N) != hipSuccess) {
                c->err = "hipHostMalloc of the exchange totals failed";
                return bail(-5);
            }
        }
        size_t chunks = 0;
        bool start_knob = false;
        if (k.sample_cache_mb >= 0) {
            // default: 512 B (64 samples of 8 B) per pixel per brick to start with (config 2 asks for
            // 4.1 GB = 250 B per pixel per brick), grown after a frame
            // whose rays did not fit to 1.25x that frame's demand, up to 45 % of the HBM free at create
            // (this is an in-situ library: the simulation shares the GPU, so the cache takes what the
            // frames need, not what is free).  Rays that do not fit are searched by re-sampling (same
            // results, slower) and counted (insitu_stats.rays_uncached).  sample_cache_mb > 0 fixes it.
            size_t freeb = 0, totalb = 0;
            if (hipMemGetInfo(&freeb, &totalb) != hipSuccess) freeb = (size_t)32 << 30;
            c->cache_max_chunks = std::min(freeb / 20 * 9 / 32, (size_t)0xffffffffu);
            size_t bytes = (size_t)k.sample_cache_mb << 20;
            if (k.sample_cache_mb == 0) {
                bytes = std::min((size_t)c->B * (size_t)c->W * (size_t)c->H * 512, c->cache_max_chunks * 32);
                c->cache_adaptive = true;
            }
            chunks = std::min(bytes / 32, (size_t)0xffffffffu);
            if (const char* v = std::getenv("INSITU_CACHE_START_CHUNKS")) {
                // test knob: a default-sized cache that starts at this size, below the first frame's
                // demand (no first-frame sizing), so the growth path runs (tests/test_gpu_parity.py)
                if (c->cache_adaptive && std::atoll(v) > 0) {
                    chunks = std::min((size_t)std::atoll(v), c->cache_max_chunks);
                    start_knob = true;
                }
            }
            if (chunks > 0) c->search_blocks = c->num_cus * 8;   // 32 waves per CU; waves that find the queue drained exit
        }
        // the first frame slot (a pipelined context allocates the second one at its first pipelined frame)
        if ((rc = alloc_slot(c, c->slots[0], chunks))) return bail(rc);
        if (chunks > 0 && start_knob) c->slots[0].cache_sized = true;
        if (const char* dbg = std::getenv("INSITU_DEBUG_RAYS")) {   // diagnostics (tools/ray_timing.py)
            if (c->slots[0].queue) {
                c->dbg_entries = (size_t)c->BV * (size_t)c->W * (size_t)c->H;
                if ((rc = c->d_dbg.alloc(c, c->dbg_entries * 4))) return bail(rc);
                c->dbg_path = dbg;
            }
        }
        if (is_root(c)) {
            if ((rc = c->d_gather.alloc(c, (size_t)c->N * c->stripPx)) ||
                (rc = c->d_image.alloc(c, (size_t)c->W * (size_t)c->H)))
                return bail(rc);
        } else if ((rc = c->d_strip.alloc(c, c->stripPx))) {
            return bail(rc);
        }
        if (k.composite_vdi) {
            c->composite_vdi = true;
            c->S_out = k.max_output_supersegments > 0 ? k.max_output_supersegments : c->S;
            c->cblockE = (size_t)c->strip_tiles * (size_t)c->S_out * (size_t)c->H * 8;
            if ((rc = c->d_cpasses.alloc(c, c->stripPx))) return bail(rc);
            // merge cache of the compositor: an eighth of the V*S entries per pixel to start with, grown to
            // a composite's demand when it did not fit (the waves that found no room merge every pass)
            // growth budget: 20 % of the HBM free at create (the simulation and the sample cache share the GPU)
            size_t freeb = 0, totalb = 0;
            if (hipMemGetInfo(&freeb, &totalb) != hipSuccess) freeb = (size_t)32 << 30;
            c->cseq_max = std::max<unsigned long long>(64ull * 64ull, (unsigned long long)(freeb / 5 / (16 * kCompEntryF4)));
            c->cseq_cap = std::min(c->cseq_max, std::max<unsigned long long>(
                64ull * 64ull, (unsigned long long)c->V * c->stripPx * (unsigned long long)c->S / 8));
            if ((rc = c->d_cseq.alloc(c, (size_t)kCompEntryF4 * (size_t)c->cseq_cap)) || (rc = c->d_cseq_cursor.alloc(c, 1)))
                return bail(rc);
            if (c->h_cseq_demand.try_alloc(1) != hipSuccess) {
                c->err = "hipHostMalloc of the compositor demand failed";
                return bail(-5);
            }
            *c->h_cseq_demand = 0;
            if (is_root(c)) {
                if ((rc = c->d_gvdi_col.alloc(c, (size_t)c->N * c->cblockE)) ||
                    (rc = c->d_gvdi_dep.alloc(c, (size_t)c->N * c->cblockE)) ||
                    (rc = c->d_gvdi_cnt.alloc(c, (size_t)c->N * c->stripPx)))
                    return bail(rc);
            } else if ((rc = c->d_cvdi_col.alloc(c, c->cblockE)) || (rc = c->d_cvdi_dep.alloc(c, c->cblockE)) ||
                       (rc = c->d_cvdi_cnt.alloc(c, c->stripPx))) {
                return bail(rc);
            }
        }
    } else {
        if ((rc = create_slot_events(c, c->slots[0]))) return bail(rc);
        c->rows = c->H / c->N;
        c->plainBlock = (size_t)c->rows * (size_t)c->W;
        c->stripPx = c->plainBlock;
        const size_t sendPx = (size_t)c->N * (size_t)c->B * c->plainBlock;
        if ((rc = c->d_pcol_send.alloc(c, sendPx)) || (rc = c->d_pdep_send.alloc(c, sendPx))) return bail(rc);
        if (c->N > 1)
            if ((rc = c->d_pcol_recv.alloc(c, sendPx)) || (rc = c->d_pdep_recv.alloc(c, sendPx))) return bail(rc);
        if (is_root(c)) {
            if ((rc = c->d_gather.alloc(c, (size_t)c->N * c->stripPx))) return bail(rc);
        } else if ((rc = c->d_strip.alloc(c, c->stripPx))) {
            return bail(rc);
        }
    }
    if (k.local_group) {
        c->group = k.local_group;
        c->group->ranks[c->rank] = c;
    } else if (c->N > 1) {
        ncclUniqueId id;
        std::memcpy(&id, k.comm_id, sizeof id);
        ncclResult_t r = ncclCommInitRank(&c->comm, c->N, id, c->rank);
        if (r != ncclSuccess) {
            c->err = std::string("ncclCommInitRank: ") + ncclGetErrorString(r);
            c->comm = nullptr;
            return bail(-4);
        }
    }
    {   // tuning seeds from the environment (tools/knob_sweep.sh); insitu_set_option overrides
        const struct { const char* name; int opt; } names[] = {
            {"INSITU_EXACT_SEARCH", INSITU_OPT_EXACT_SEARCH}, {"INSITU_SEARCH_DEPTH", INSITU_OPT_SEARCH_DEPTH},
            {"INSITU_LONG_SAMPLES", INSITU_OPT_LONG_SAMPLES}, {"INSITU_ROUND_BATCH", INSITU_OPT_ROUND_BATCH},
            {"INSITU_SEARCH_OVERSUB", INSITU_OPT_SEARCH_OVERSUB}, {"INSITU_TILE_ORDER", INSITU_OPT_TILE_ORDER},
            {"INSITU_SUPER_TILE", INSITU_OPT_SUPER_TILE}, {"INSITU_REGROUP", INSITU_OPT_REGROUP},
            {"INSITU_EXACT_TILE_KEYS", INSITU_OPT_EXACT_TILE_KEYS}, {"INSITU_PIPE_TRIGGER", INSITU_OPT_PIPE_TRIGGER},
            {"INSITU_PIPE_OVERSUB", INSITU_OPT_PIPE_OVERSUB}, {"INSITU_PIPE_SEARCH_RAYS", INSITU_OPT_PIPE_SEARCH_RAYS},
            {"INSITU_VIEW_SKIP", INSITU_OPT_VIEW_SKIP}, {"INSITU_VIEW_COMPACT", INSITU_OPT_VIEW_COMPACT}};
        for (const auto& nm : names) {
            if (const char* v = std::getenv(nm.name)) {
                if (insitu_set_option(c, nm.opt, std::atoll(v)) != 0) {
                    c->err = std::string("insitu_create: ") + nm.name + "=" + v + " out of range";
                    return bail(-1);
                }
            }
        }
    }
    *out = c;
    return 0;
}

int insitu_set_option(insitu_ctx* c, int option, long long v) {
    if (!c) return fail(nullptr, -1, "insitu_set_option: null context");
    Tuning& t = c->tune;
    switch (option) {
    case INSITU_OPT_EXACT_SEARCH:
        if (v != 0 && v != 1) break;
        t.exact_search = v;
        return 0;
    case INSITU_OPT_SEARCH_DEPTH:
        if (v < 0 || v > 6) break;
        t.search_depth = v;
        return 0;
    case INSITU_OPT_LONG_SAMPLES:
        if (v < 0 || v > 0xffffffffll) break;
        t.long_samples = v;
        return 0;
    case INSITU_OPT_ROUND_BATCH:
        if (v < 1 || v > 64) break;
        t.round_batch = v;
        return 0;
    case INSITU_OPT_SEARCH_OVERSUB:
        if (v < 1 || v > 64) break;
        t.search_oversub = v;
        return 0;
    case INSITU_OPT_TILE_ORDER:
        if (v != 0 && v != 1) break;
        t.tile_order = v;
        return 0;
    case INSITU_OPT_SUPER_TILE:
        if (v != 1 && v != 2 && v != 4) break;
        if (v > 1 && c->mode == INSITU_MODE_VDI && padded_tiles(c, (int)v) >= ((size_t)1 << 24))
            return fail(c, -1, "insitu_set_option: super-tiles of " + std::to_string(v) +
                                   " tiles pad this frame's tile grid past the sort key's 24 bits of position");
        t.super_tile = v;
        return 0;
    case INSITU_OPT_REGROUP:
        if (v != 0 && v != 1) break;
        t.regroup = v;
        return 0;
    case INSITU_OPT_EXACT_TILE_KEYS:
        if (v != 0 && v != 1) break;
        t.exact_tile_keys = v;
        return 0;
    case INSITU_OPT_PIPE_TRIGGER:
        if (v < 0 || v > 2) break;
        c->pipe_trigger = (int)v;
        return 0;
    case INSITU_OPT_PIPE_OVERSUB:
        if (v < 1 || v > 64) break;
        t.pipe_oversub = v;
        return 0;
    case INSITU_OPT_PIPE_SEARCH_RAYS:
        if (v < 0 || v > (1ll << 24)) break;
        t.pipe_search_rays = v;
        return 0;
    case INSITU_OPT_VIEW_SKIP:
        if (v != 0 && v != 1) break;
        c->view.skip = v;
        return 0;
    case INSITU_OPT_VIEW_COMPACT:   // (the next bind's layout; the bound VDI keeps its own)
        if (v != 0 && v != 1) break;
        c->view.compact_next = v;
        return 0;
    default:
        return fail(c, -1, "insitu_set_option: unknown option " + std::to_string(option));
    }
    return fail(c, -1, "insitu_set_option: value " + std::to_string(v) + " out of range for option " +
                           std::to_string(option));
}

void insitu_destroy(insitu_ctx* ctx) {
    release(ctx);
    delete ctx;
}

void* insitu_stream(insitu_ctx* ctx) { return ctx ? (void*)ctx->stream : nullptr; }

int insitu_set_brick(insitu_ctx* c, int slot, const void* data, int dtype, const int dims[3], const float model[16],
                     int data_on_device) {
    if (!c) return fail(nullptr, -1, "insitu_set_brick: null context");
    if (slot < 0 || slot >= c->B) return fail(c, -1, "insitu_set_brick: slot out of range");
    if (!data || !dims || !model) return fail(c, -1, "insitu_set_brick: null argument");
    if (dtype != INSITU_U8 && dtype != INSITU_U16 && dtype != INSITU_F32) return fail(c, -1, "insitu_set_brick: bad dtype");
    if (dims[0] < 1 || dims[1] < 1 || dims[2] < 1) return fail(c, -1, "insitu_set_brick: bad dims");
    const size_t vox = (size_t)dims[0] * (size_t)dims[1] * (size_t)dims[2];
    if (vox >= (size_t)1 << 32) return fail(c, -1, "insitu_set_brick: brick exceeds 2^32 voxels");
    HIPCHK(c, hipSetDevice(c->cfg.device));
    Brick& b = c->bricks[slot];
    const size_t nb = (size_t)((dims[0] + 7) / 8) * (size_t)((dims[1] + 7) / 8) * (size_t)((dims[2] + 7) / 8);
    if (nb * 729 >= (size_t)1 << 32) return fail(c, -1, "insitu_set_brick: blocked brick exceeds 2^32 voxels");
    const size_t bytes = nb * 729 * dtype_size(dtype);   // blocked layout with halo (insitu_sampling.h)
    if (b.d.count() != bytes)
        if (int rc = b.d.alloc(c, bytes)) return rc;
    if (!mat4_inverse(model, b.im)) return fail(c, -1, "insitu_set_brick: model matrix is singular");
    b.dtype = dtype;
    std::memcpy(b.dims, dims, sizeof b.dims);
    b.valid = false;
    // a pipelined frame in flight may still sample this brick (its first pass, and its search re-samples rays
    // without cache space): the ingest waits for that frame's search
    if (c->pipe_inflight && c->alt->ev_valid[EvSearchEnd]) HIPCHK(c, hipStreamWaitEvent(c->stream, c->alt->ev[EvSearchEnd], 0));
    if (!c->ingest_batch) {   // the first re-ingest since the last render: the batch's GPU time starts here
        HIPCHK(c, hipEventRecord(c->ev_ingest0, c->stream));
        c->ingest_batch = true;
    }
    if (data_on_device) {
        // in-situ: the simulation's device array is read in place by the ingest kernel
        HIPCHK(c, launch_brick_ingest(data, b.d, dtype, dims[0], dims[1], dims[2], c->stream));
        HIPCHK(c, hipEventRecord(c->ev_ingest, c->stream));
    } else {
        // the staging buffer is kept across calls: the reference re-uploads every grid every 20 frames
        // (DistributedVolumeRenderer.kt:521-527); a pinned source makes the copy a DMA at link speed
        const size_t src_bytes = vox * dtype_size(dtype);
        if (c->d_staging.count() < src_bytes) {
            HIPCHK(c, hipStreamSynchronize(c->stream));
            if (int rc = c->d_staging.reserve(c, src_bytes)) return rc;
        }
        hipError_t e = hipMemcpyAsync(c->d_staging, data, src_bytes, hipMemcpyHostToDevice, c->stream);
        if (e == hipSuccess) e = launch_brick_ingest(c->d_staging, b.d, dtype, dims[0], dims[1], dims[2], c->stream);
        if (e == hipSuccess) e = hipEventRecord(c->ev_ingest, c->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(c->stream);   // host buffer may be reused by the caller
        if (e != hipSuccess) return fail(c, -3, std::string("insitu_set_brick: ") + hipGetErrorString(e));
    }
    b.valid = true;
    return 0;
}

int insitu_set_transfer(insitu_ctx* c, const float* tf, int n_tf, const float* cmap, int n_cm, float conv_scale,
                        float conv_offset) {
    if (!c) return fail(nullptr, -1, "insitu_set_transfer: null context");
    if (!tf || !cmap || n_tf < 1 || n_cm < 1 || n_tf > 8192 || n_cm > 4096)
        return fail(c, -1, "insitu_set_transfer: bad LUTs (1..8192 tf texels, 1..4096 colour texels)");
    HIPCHK(c, hipSetDevice(c->cfg.device));
    {   // the generator kernels stage the LUTs in LDS beside their own per-block state: refuse LUTs that would
        // not fit a block here rather than fail at the next kernel launch
        int max_lds = 0;
        HIPCHK(c, hipDeviceGetAttribute(&max_lds, hipDeviceAttributeMaxSharedMemoryPerBlock, c->cfg.device));
        const size_t need = vdi_generator_lds_bytes(n_tf, n_cm);
        if (c->mode == INSITU_MODE_VDI && max_lds > 0 && need > (size_t)max_lds)
            return fail(c, -1, "insitu_set_transfer: LUTs of " + std::to_string(n_tf) + " + " + std::to_string(n_cm) +
                                   " texels need " + std::to_string(need) + " bytes of LDS per block; the device has " +
                                   std::to_string(max_lds));
    }
    // (the LUTs are sized exactly: a size that differs re-allocates; a failure leaves that LUT unset)
    if (c->d_tf.count() != (size_t)n_tf)
        if (int rc = c->d_tf.alloc(c, (size_t)n_tf)) return rc;
    c->n_tf = n_tf;
    if (c->d_cmap.count() != 4 * (size_t)n_cm)
        if (int rc = c->d_cmap.alloc(c, 4 * (size_t)n_cm)) return rc;
    c->n_cm = n_cm;
    // the colour bound of the filtered decisions' margin (vdi_generate.hip, filter_margin)
    double cm_max = 0.0, tf_max = 0.0;
    bool finite = true;
    for (int i = 0; i < n_cm; ++i)
        for (int k = 0; k < 3; ++k) {
            finite = finite && std::isfinite(cmap[4 * i + k]);
            cm_max = std::max(cm_max, (double)std::fabs(cmap[4 * i + k]));
        }
    for (int i = 0; i < n_tf; ++i) {
        finite = finite && std::isfinite(tf[i]);
        tf_max = std::max(tf_max, (double)std::fabs(tf[i]));
    }
    const double cb = std::max({1.0, 2.0 * cm_max, 2.0 * cm_max * tf_max});
    c->cmag = (finite && cb < 1.0e6) ? (float)cb : std::numeric_limits<float>::infinity();   // inf: exact path only
    if (c->pipe_ready)   // a pipelined frame in flight reads the LUTs
        if (int rc = insitu_synchronize(c)) return rc;
    HIPCHK(c, hipMemcpyAsync(c->d_tf, tf, sizeof(float) * n_tf, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(c->d_cmap, cmap, sizeof(float) * 4 * n_cm, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->conv_scale = conv_scale;
    c->conv_offset = conv_offset;
    return 0;
}

static BrickDesc brick_desc(const insitu_ctx* c, const Brick& b) {
    BrickDesc d;
    d.data = b.d;
    d.dtype = b.dtype;
    d.nx = b.dims[0]; d.ny = b.dims[1]; d.nz = b.dims[2];
    d.nbx = (d.nx + 7) / 8; d.nby = (d.ny + 7) / 8; d.nbz = (d.nz + 7) / 8;
    std::memcpy(d.im, b.im, sizeof d.im);
    const float norm = b.dtype == INSITU_U8 ? 1.0f / 255.0f : (b.dtype == INSITU_U16 ? 1.0f / 65535.0f : 1.0f);
    d.conv_k = c->conv_scale * norm;
    d.conv_off = c->conv_offset;
    return d;
}

namespace {

// a checked camera as a frame keeps it: the matrix products the kernels and the compositors take
struct FrameCamera {
    float ipv[16], pv[16], view[16];
    float nw, fwnw, tmax;
};

// the camera set-up of insitu_set_camera and of every render; writes *m only when the camera is accepted
int camera_matrices(insitu_ctx* c, const insitu_camera* cam, FrameCamera* m) {
    if (!cam) return fail(c, -1, "insitu_set_camera: null camera");
    float iv[16], ip[16];
    if (cam->has_inverses) {
        std::memcpy(iv, cam->inv_view, sizeof iv);
        std::memcpy(ip, cam->inv_proj, sizeof ip);
    } else if (!mat4_inverse(cam->view, iv) || !mat4_inverse(cam->proj, ip)) {
        return fail(c, -1, "insitu_set_camera: view or projection matrix is singular");
    }
    mat4_mul_f(iv, ip, m->ipv);                // VDIGenerator.comp:289 (ipvG of accumulateSupseg)
    mat4_mul_f(cam->proj, cam->view, m->pv);   // VDIGenerator.comp:290
    std::memcpy(m->view, cam->view, sizeof m->view);
    m->nw = cam->nw; m->fwnw = cam->fwnw; m->tmax = cam->tmax;
    return 0;
}

void set_slot_camera(insitu_ctx* c, FrameSlot& f, const FrameCamera& m) {
    std::memcpy(f.ipv, m.ipv, sizeof f.ipv);
    std::memcpy(f.pv, m.pv, sizeof f.pv);
    std::memcpy(f.view, m.view, sizeof f.view);
    c->camera_set = true;
}

// everything that rejects a render, pipelined or not, before anything is enqueued or changed: *m is the camera
// render_frame takes
int render_check(insitu_ctx* c, const insitu_camera* cam, FrameCamera* m) {
    if (!cam) return fail(c, -1, "insitu_render: null camera");
    if (!c->d_tf) return fail(c, -1, "insitu_render: transfer function not set");
    for (int b = 0; b < c->B; ++b) {
        if (!c->bricks[b].valid) return fail(c, -1, "insitu_render: brick slot " + std::to_string(b) + " not set");
        if (c->bricks[b].dtype != c->bricks[0].dtype)
            return fail(c, -1, "insitu_render: all bricks of a rank must share one voxel type");
    }
    if (!(cam->nw > 0.0f)) return fail(c, -1, "insitu_render: nw must be > 0");
    return camera_matrices(c, cam, m);
}

// where a render enqueues.  Unpipelined: both streams are the context stream and nothing gates the first pass.
// Pipelined (insitu_frame_pipelined): the first pass on the sampling stream, behind the gate -- placed between
// the frame's prepare (counters, tile keys and their sort: the slot's own buffers) and its sampling kernel, so
// the prepare's launches run ahead of it -- and the search on the slot's search stream.
struct RenderPlan {
    hipStream_t first = nullptr;    // the first pass
    hipStream_t search = nullptr;   // the search and what follows it
    bool pipelined = false;
    unsigned long long* gate_flag = nullptr;         // the first pass waits for *gate_flag >= gate_value (mode 1) ...
    unsigned long long gate_value = 0;
    hipEvent_t gate_event = nullptr;                 // ... or for this event (mode 0), or for neither
};

// the render of a checked camera (render_check) into slot f
int render_frame(insitu_ctx* c, FrameSlot& f, const FrameCamera& cam, const RenderPlan& plan) {
    set_slot_camera(c, f, cam);
    TransferDesc xf{c->d_tf, c->n_tf, c->d_cmap, c->n_cm, c->cmag};
    const hipStream_t ss = plan.first, sr = plan.search;
    const bool pipelined = plan.pipelined;
    HIPCHK(c, wait_peer_reads(c, ss));
    c->ingest_batch = false;
    f.pipelined = pipelined;
    if (!pipelined) record(f, EvRenderStart, ss);   // (pipelined: at the gate, below)
    if (c->mode == INSITU_MODE_VDI) {
        const size_t oct = (size_t)c->BV * (size_t)c->S * (size_t)c->ncx * (size_t)c->ncy;
        if (oct) HIPCHK(c, hipMemsetAsync(f.octree, 0, oct * sizeof(uint32_t), ss));   // GridCellsToZero.comp
        if (f.cache_grow_to > f.cache_chunks) {   // the last frame of this slot's rays did not all fit
            const size_t grow = f.cache_grow_to, old = f.cache_chunks;
            f.cache_grow_to = 0;   // (cleared first: a failure below is not retried every frame)
            HIPCHK(c, hipStreamSynchronize(c->stream));
            HIPCHK(c, hipStreamSynchronize(ss));
            HIPCHK(c, hipStreamSynchronize(sr));
            if (cache_realloc(f, grow) != hipSuccess) {
                // keep what fits (the rest re-samples): half the request, never less than the cache
                // that worked, and at most that from now on
                const size_t keep = std::max(old, grow / 2);
                if (cache_realloc(f, keep) != hipSuccess) HIPCHK(c, cache_realloc(f, old));
                c->cache_max_chunks = f.cache_chunks;
            }
        }
        VdiGenParams p{};
        for (int b = 0; b < c->B; ++b) p.bricks[b] = brick_desc(c, c->bricks[b]);
        p.xfer = xf;
        std::memcpy(p.ipv, f.ipv, sizeof p.ipv);
        std::memcpy(p.pv, f.pv, sizeof p.pv);
        std::memcpy(p.view, f.view, sizeof p.view);
        p.nw = cam.nw;
        p.tmax = cam.tmax;
        p.W = c->W; p.H = c->H; p.S = c->S;
        p.strip_w = c->strip_w; p.strip_tiles = c->strip_tiles; p.nstrips = c->N; p.B = c->BV;
        p.nvolumes = c->BV != c->B ? c->B : 0;
        p.ytiles = (c->H + 7) / 8;
        p.color = f.vcol_send;
        p.depth = f.vdep_send;
        p.octree = f.octree;
        p.octree_stride = (size_t)c->S * (size_t)c->ncx * (size_t)c->ncy;
        p.passes = f.passes;
        p.passes_stride = (size_t)c->W * (size_t)c->H;
        p.seg_pending = f.seg_pending;
        p.seg_steps = f.seg_steps;
        p.ncx = c->ncx; p.ncy = c->ncy;
        p.interval_size = (20.0f - 0.1f) / (float)c->S;   // VDIGenerator.comp:241-247
        p.cache = f.cache;
        p.split_event = f.ev[EvSampleEnd];
        f.ev_valid[EvSampleEnd] = true;
        p.cache_chunks = f.cache_chunks;
        p.ctr = f.counters;
        p.queue = f.queue;
        p.queue_cap = (uint32_t)((size_t)c->BV * (size_t)c->W * (size_t)c->H);
        // longest-first, coarsely: rays with many samples (most work per pass, and the ones with
        // 20+ passes) are searched before the rest, so the frame does not end waiting for a long
        // ray popped late; within each class the queue keeps the sampling kernel's tile order
        p.long_samples = (uint32_t)c->tune.long_samples;
        p.round_batch = (int)c->tune.round_batch;   // (group mode ends rounds at once)
        p.search_blocks = c->search_blocks;
        if (pipelined && c->tune.pipe_search_rays > 0) {
            // the search beside the next frame's first pass: one to two blocks per CU by the queue length, the
            // rest of each CU's wave slots left to that first pass
            p.search_blocks = std::min(c->search_blocks, 2 * c->num_cus);
            p.search_block_rays = (int)c->tune.pipe_search_rays;
            p.search_min_blocks = std::min(p.search_blocks, c->num_cus);
        }
        p.search_oversub = (int)(pipelined ? c->tune.pipe_oversub : c->tune.search_oversub);
        p.search_depth = (int)c->tune.search_depth;
        p.regroup = (int)c->tune.regroup;
        p.exact_search = (int)c->tune.exact_search;
        if (f.cache && (c->search_lanes_tf != c->n_tf || c->search_lanes_cm != c->n_cm)) {
            // lanes the search grid keeps resident on this device with these LUT sizes (LDS)
            HIPCHK(c, vdi_search_resident_lanes(c->n_tf, c->n_cm, c->cfg.device, &c->search_lanes));
            c->search_lanes_tf = c->n_tf;
            c->search_lanes_cm = c->n_cm;
        }
        p.search_lanes = std::min(c->search_lanes, p.search_blocks * 256);
        if (c->tune.tile_order && f.tile_keys) {
            p.tile_keys = f.tile_keys;
            p.super_tile = (int)c->tune.super_tile;
            p.tile_len_exact = (int)c->tune.exact_tile_keys;
            p.tile_ids = f.tile_ids;
            p.sort_tmp = f.sort_tmp;
            p.sort_tmp_bytes = c->sort_tmp_bytes;
        }
        if (pipelined && f.cache && c->pipe_flag && c->pipe_trigger == 1) {
            p.pipe_flag = c->pipe_flag + f.flag_index;   // this search's queue drain starts the next first pass
            p.pipe_seq = f.flag_value + 1;
        }
        // counters zeroed, tile keys (and, on a default cache's first frame, the frame's cache demand) sorted
        p.measure_cache = (c->cache_adaptive && !f.cache_sized && p.nvolumes == 0) ? 1 : 0;
        HIPCHK(c, launch_vdi_prepare(p, ss));
        p.prepared = 1;
        if (p.measure_cache && f.cache && p.tile_ids) {
            // the first frame of a default-sized cache: wait for the demand the tile keys measured and
            // size the cache to it (later frames grow it from their own demand, cache_observe)
            unsigned long long need = 0;
            HIPCHK(c, hipMemcpyAsync(&need, &f.counters->cache_need, sizeof need, hipMemcpyDeviceToHost, ss));
            HIPCHK(c, hipStreamSynchronize(ss));
            f.cache_sized = true;
            const size_t want = std::min((size_t)(need + need / 4 + 64), c->cache_max_chunks);
            if (want > f.cache_chunks) HIPCHK(c, cache_realloc(f, want));
            p.cache = f.cache;
            p.cache_chunks = f.cache_chunks;
        }
        if (pipelined) {
            // the gate (insitu_frame_pipelined): the prepare above only touches this slot's buffers, so its
            // small launches are already queued when the previous frame's search lets the first pass start;
            // the frame's render time and latency count from here
            if (plan.gate_flag)
                HIPCHK(c, hipStreamWaitValue64(ss, plan.gate_flag, plan.gate_value, hipStreamWaitValueGte));
            else if (plan.gate_event)
                HIPCHK(c, hipStreamWaitEvent(ss, plan.gate_event, 0));
            record(f, EvRenderStart, ss);
        }
        if (c->d_dbg && !pipelined) {
            HIPCHK(c, hipMemsetAsync(c->d_dbg, 0, c->dbg_entries * 32, ss));
            p.debug_rays = c->d_dbg;
            p.debug_cap = (uint32_t)std::min(c->dbg_entries, (size_t)0xffffffffu);
            c->dbg_pending = true;   // written to INSITU_DEBUG_RAYS at the next insitu_synchronize
        }
        HIPCHK(c, launch_vdi_sample(p, ss));
        if (ss != sr) HIPCHK(c, hipStreamWaitEvent(sr, f.ev[EvSampleEnd], 0));
        HIPCHK(c, launch_vdi_search(p, sr));
        f.search_launched = f.cache != nullptr;
        if (pipelined) {
            // the next frame's trigger: the search is over (mode 0), or -- the flag's safety net when no wave
            // crossed the trigger point (an empty queue) -- its value is reached (mode 1)
            record(f, EvSearchEnd, sr);
            if (p.pipe_flag) {
                HIPCHK(c, hipStreamWriteValue64(sr, p.pipe_flag, p.pipe_seq, 0));
                f.flag_value = p.pipe_seq;   // what the next frame's gate waits for: its store is enqueued
            }
        }
        HIPCHK(c, launch_vdi_finish(p, sr));
        if (f.h_ctr) {   // the frame's counters, read on the host after the next synchronisation
            HIPCHK(c, hipMemcpyAsync(f.h_ctr, f.counters, sizeof(GenCounters), hipMemcpyDeviceToHost, sr));
            f.h_ctr_pending = true;
            f.h_ctr_valid = false;
        }
        // variable-length exchange: the stored supersegments of the blocks bound for the other
        // ranks are packed as part of producing the send buffers (timed as the exchange); a pipelined frame
        // packs them with its completion, where the compact buffers are free
        if (c->N > 1 && !pipelined) HIPCHK(c, compact_enqueue(c, f, sr));
        c->lists_from_reference = false;
    } else {
        PlainGenParams p{};
        for (int b = 0; b < c->B; ++b) p.bricks[b] = brick_desc(c, c->bricks[b]);
        p.xfer = xf;
        std::memcpy(p.ipv, f.ipv, sizeof p.ipv);
        p.nw = cam.nw; p.fwnw = cam.fwnw; p.tmax = cam.tmax;
        p.dim0 = c->W; p.dim1 = c->H; p.rows = c->rows;
        p.nstrips = c->N; p.B = c->B;
        p.color = c->d_pcol_send;
        p.depth = c->d_pdep_send;
        HIPCHK(c, launch_plain_generate(p, sr));
    }
    record(f, EvRenderEnd, sr);
    f.rendered = true;
    f.composited = false;
    f.exchanged = false;
    return 0;
}

// the exchange of slot f's rendered frame on stream s
int exchange_frame(insitu_ctx* c, FrameSlot& f, hipStream_t st) {
    if (!f.rendered) return fail(c, -1, "insitu_exchange: nothing rendered");
    c->last_exchange_entries = 0;
    c->last_exchange_bytes = 0;
    if (c->N > 1 && c->mode == INSITU_MODE_VDI) {
        // variable-length exchange of the compact messages (VDICompositingTest.kt:251-305, 360-415:
        // counts first, then MPI_Alltoallv): totals to every peer, the host learns the receive sizes,
        // then grouped send/recv of the meta blocks and of exactly the packed entries
        const size_t region = (size_t)c->BV * c->blockE;
        uint32_t* send_tot = c->h_tot;
        uint32_t* recv_tot = c->h_tot + c->N;
        if (c->group) {   // in-process: the peers packed their blocks in their renders (EvRenderEnd)
            for (int p = 0; p < c->N; ++p) {
                if (p == c->rank) continue;
                const insitu_ctx* q = c->group->ranks[p];
                if (!q) return fail(c, -1, "insitu_exchange: local group rank " + std::to_string(p) + " missing");
                if (!q->cur->rendered || !q->cur->ev_valid[EvRenderEnd]) return fail(c, -1, "insitu_exchange: local group rank " + std::to_string(p) + " has not rendered");
                HIPCHK(c, hipStreamWaitEvent(st, q->cur->ev[EvRenderEnd], 0));
                HIPCHK(c, hipMemcpyAsync(recv_tot + p, q->d_cursor + c->rank, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
            }
            HIPCHK(c, hipMemcpyAsync(send_tot, c->d_cursor, sizeof(uint32_t) * (size_t)c->N, hipMemcpyDeviceToHost, st));
            record(f, EvCountsIn, st);
            HIPCHK(c, hipStreamSynchronize(st));
            record(f, EvPayloadStart, st);
            for (int p = 0; p < c->N; ++p) {
                if (p == c->rank) continue;
                const insitu_ctx* q = c->group->ranks[p];
                HIPCHK(c, hipMemcpyAsync(c->d_meta_recv + (size_t)p * c->meta_bytes, q->d_meta_send + (size_t)c->rank * q->meta_bytes,
                                         c->meta_bytes, hipMemcpyDeviceToDevice, st));
                const size_t n = recv_tot[p];
                if (n == 0) continue;
                HIPCHK(c, hipMemcpyAsync(c->d_vcol_recv + (size_t)p * region, q->d_ccol_send + (size_t)c->rank * region,
                                         n * sizeof(float4), hipMemcpyDeviceToDevice, st));
                HIPCHK(c, hipMemcpyAsync(c->d_vdep_recv + (size_t)p * region, q->d_cdep_send + (size_t)c->rank * region,
                                         n * sizeof(float2), hipMemcpyDeviceToDevice, st));
            }
        } else {
            NCCLCHK(c, ncclGroupStart());
            for (int p = 0; p < c->N; ++p) {
                if (p == c->rank) continue;
                NCCLCHK(c, ncclSend(c->d_cursor + p, 1, ncclUint32, p, c->comm, st));
                NCCLCHK(c, ncclRecv(c->d_cursor + c->N + p, 1, ncclUint32, p, c->comm, st));
            }
            NCCLCHK(c, ncclGroupEnd());
            HIPCHK(c, hipMemcpyAsync(c->h_tot, c->d_cursor, 2 * sizeof(uint32_t) * (size_t)c->N, hipMemcpyDeviceToHost,
                                     st));
            // the host learns the receive sizes: the stream idles from here (EvCountsIn) until the payload
            // group is enqueued (EvPayloadStart) -- reported as insitu_stats.ms_exchange_sync
            record(f, EvCountsIn, st);
            HIPCHK(c, hipStreamSynchronize(st));
            record(f, EvPayloadStart, st);
            NCCLCHK(c, ncclGroupStart());
            for (int p = 0; p < c->N; ++p) {
                if (p == c->rank) continue;
                NCCLCHK(c, ncclSend(c->d_meta_send + (size_t)p * c->meta_bytes, c->meta_bytes, ncclUint8, p, c->comm, st));
                NCCLCHK(c, ncclRecv(c->d_meta_recv + (size_t)p * c->meta_bytes, c->meta_bytes, ncclUint8, p, c->comm, st));
                if (send_tot[p]) {
                    NCCLCHK(c, ncclSend(c->d_ccol_send + (size_t)p * region, (size_t)send_tot[p] * 4, ncclFloat32, p, c->comm, st));
                    NCCLCHK(c, ncclSend(c->d_cdep_send + (size_t)p * region, (size_t)send_tot[p] * 2, ncclFloat32, p, c->comm, st));
                }
                if (recv_tot[p]) {
                    NCCLCHK(c, ncclRecv(c->d_vcol_recv + (size_t)p * region, (size_t)recv_tot[p] * 4, ncclFloat32, p, c->comm, st));
                    NCCLCHK(c, ncclRecv(c->d_vdep_recv + (size_t)p * region, (size_t)recv_tot[p] * 2, ncclFloat32, p, c->comm, st));
                }
            }
            NCCLCHK(c, ncclGroupEnd());
        }
        for (int p = 0; p < c->N; ++p) {
            if (p == c->rank) continue;
            c->last_exchange_entries += send_tot[p];
            c->last_exchange_bytes += (long long)c->meta_bytes + (long long)send_tot[p] * (long long)(sizeof(float4) + sizeof(float2));
        }
    } else if (c->N > 1 && c->group) {   // plain mode, in-process: pull the block each peer rendered for my strip
        for (int p = 0; p < c->N; ++p) {
            if (p == c->rank) continue;
            const insitu_ctx* q = c->group->ranks[p];
            if (!q) return fail(c, -1, "insitu_exchange: local group rank " + std::to_string(p) + " missing");
            if (!q->cur->rendered || !q->cur->ev_valid[EvRenderEnd]) return fail(c, -1, "insitu_exchange: local group rank " + std::to_string(p) + " has not rendered");
            // the peer's render runs on its own stream (and maybe device): order my copies after it
            HIPCHK(c, hipStreamWaitEvent(st, q->cur->ev[EvRenderEnd], 0));
            const size_t n = (size_t)c->B * c->plainBlock;
            const size_t src = (size_t)c->rank * n, dst = (size_t)p * n;
            HIPCHK(c, hipMemcpyAsync(c->d_pcol_recv + dst, q->d_pcol_send + src, n * 4, hipMemcpyDeviceToDevice, st));
            HIPCHK(c, hipMemcpyAsync(c->d_pdep_recv + dst, q->d_pdep_send + src, n * 4, hipMemcpyDeviceToDevice, st));
        }
        c->last_exchange_bytes = (long long)(c->N - 1) * (long long)c->B * (long long)c->plainBlock * 8;
    } else if (c->N > 1) {   // plain mode: one rgba8 colour + depth texel per pixel, fixed-size blocks
        NCCLCHK(c, ncclGroupStart());
        for (int p = 0; p < c->N; ++p) {
            if (p == c->rank) continue;
            const size_t e = (size_t)p * (size_t)c->B * c->plainBlock, n = (size_t)c->B * c->plainBlock;
            NCCLCHK(c, ncclSend(c->d_pcol_send + e, n, ncclUint32, p, c->comm, st));
            NCCLCHK(c, ncclRecv(c->d_pcol_recv + e, n, ncclUint32, p, c->comm, st));
            NCCLCHK(c, ncclSend(c->d_pdep_send + e, n, ncclUint32, p, c->comm, st));
            NCCLCHK(c, ncclRecv(c->d_pdep_recv + e, n, ncclUint32, p, c->comm, st));
        }
        NCCLCHK(c, ncclGroupEnd());
        c->last_exchange_bytes = (long long)(c->N - 1) * (long long)c->B * (long long)c->plainBlock * 8;
    }
    if (c->group) record(f, EvPeerReadsDone, st);
    record(f, EvExchangeEnd, st);
    f.exchanged = true;
    return 0;
}

// list v (source s = v / B, brick b = v % B) of this rank's strip, as the compositors read it: this rank's own
// from slot f
VdiList list_of(const insitu_ctx* c, const FrameSlot& f, int v) {
    const int s = v / c->BV, b = v % c->BV;
    VdiList L{};
    if (c->lists_from_reference) {   // host-buffer path: reference layout converted to slots (B == 1)
        const size_t slot = (size_t)s * c->blockE;
        L.col = (s == c->rank ? f.vcol_send : c->d_vcol_recv) + slot;
        L.dep = (s == c->rank ? f.vdep_send : c->d_vdep_recv) + slot;
        L.cnt16 = c->d_ref_cnt + (size_t)s * c->stripPx;
        L.cnt_pitch = c->strip_w;
        L.cnt_x0 = 0;
    } else if (s == c->rank) {       // my own strip: the generator's slots and counts
        const size_t e = ((size_t)c->rank * (size_t)c->BV + (size_t)b) * c->blockE;
        L.col = f.vcol_send + e;
        L.dep = f.vdep_send + e;
        L.cnt16 = f.seg_pending + (size_t)b * (size_t)c->W * (size_t)c->H;
        L.cnt_pitch = c->W;
        L.cnt_x0 = c->rank * c->strip_w;
    } else {                         // the compact message source s sent
        const size_t tiles = (size_t)c->strip_tiles * (size_t)((c->H + 7) / 8);
        const size_t region = (size_t)c->BV * c->blockE;
        L.col = c->d_vcol_recv + (size_t)s * region;
        L.dep = c->d_vdep_recv + (size_t)s * region;
        const uint8_t* meta = c->d_meta_recv + (size_t)s * c->meta_bytes;
        L.cnt8 = meta + (size_t)b * tiles * 64;
        L.toff = reinterpret_cast<const uint32_t*>(meta + (size_t)c->BV * tiles * 64) + (size_t)b * tiles;
    }
    return L;
}

// the composite of slot f's frame into this rank's strip, on stream st
int composite_frame(insitu_ctx* c, FrameSlot& f, hipStream_t st) {
    if (!f.rendered) return fail(c, -1, "insitu_composite: nothing rendered");
    // with N > 1 the peers' lists arrive in insitu_exchange: without it the compact-message offsets
    // of the receive buffers are not this frame's (or never written)
    if (c->N > 1 && !f.exchanged) return fail(c, -1, "insitu_composite: call insitu_exchange first (nranks > 1)");
    HIPCHK(c, wait_peer_reads(c, st));   // (local group: the root's gather of the last strip)
    uint32_t* out = is_root(c) ? c->d_gather + (size_t)c->rank * c->stripPx : c->d_strip;
    if (c->mode == INSITU_MODE_VDI && c->composite_vdi) {
        CompositeParams p{};   // VDICompositor.comp (DistributedVolumes.kt:424-439)
        p.V = c->V; p.S = c->S; p.S_out = c->S_out; p.H = c->H; p.W = c->W;
        p.strip_w = c->strip_w; p.strip_tiles = c->strip_tiles; p.x_offset = c->rank * c->strip_w;
        std::memcpy(p.ipv, f.ipv, sizeof p.ipv);
        for (int v = 0; v < c->V; ++v) p.lists[v] = list_of(c, f, v);
        p.out_color = cvdi_col(c);
        p.out_depth = cvdi_dep(c);
        p.out_count = cvdi_cnt(c);
        p.ndc_local = (c->cfg.faithful & INSITU_FAITHFUL_COMPOSITOR_NDC_X) ? 1 : 0;
        p.passes = c->d_cpasses;
        p.exact = (int)c->tune.exact_search;
        if (c->d_cseq) {
            // the previous composite's demand (observed after that frame's synchronisation) grows the
            // cache, up to the budget taken at create; the waves that find no room merge every pass
            const unsigned long long dem = c->cseq_demand, old = c->cseq_cap;
            if (dem > old && old < c->cseq_max) {
                const unsigned long long want = std::min(dem + dem / 4, c->cseq_max);
                HIPCHK(c, hipStreamSynchronize(st));
                c->d_cseq.reset();
                c->cseq_cap = 0;
                // the request, else half of it, else the cache that worked (and that size from now on)
                for (unsigned long long sz : {want, std::max(old, want / 2), old}) {
                    if (sz && c->d_cseq.try_alloc((size_t)sz * kCompEntryF4) == hipSuccess) {
                        c->cseq_cap = sz;
                        break;
                    }
                }
                if (c->cseq_cap < want) c->cseq_max = c->cseq_cap;
                if (!c->d_cseq) return fail(c, -5, "insitu_composite: re-allocating the merge cache failed");
            }
            if (c->d_cseq) {
                HIPCHK(c, hipMemsetAsync(c->d_cseq_cursor, 0, sizeof(unsigned long long), st));
                p.seq = c->d_cseq;
                p.seq_cursor = c->d_cseq_cursor;
                p.seq_cap = c->cseq_cap;
            }
        }
        HIPCHK(c, launch_vdi_composite(p, st));
        if (p.seq) {
            HIPCHK(c, hipMemcpyAsync(c->h_cseq_demand, c->d_cseq_cursor, sizeof(unsigned long long), hipMemcpyDeviceToHost,
                                     st));
            c->cseq_pending = true;   // observed after the next synchronisation (cache_observe)
        }
    } else if (c->mode == INSITU_MODE_VDI) {
        FlattenParams p{};
        p.V = c->V; p.S = c->S; p.H = c->H; p.W = c->W;
        p.strip_w = c->strip_w; p.strip_tiles = c->strip_tiles; p.x_offset = c->rank * c->strip_w;
        std::memcpy(p.ipv, f.ipv, sizeof p.ipv);
        for (int v = 0; v < c->V; ++v) p.lists[v] = list_of(c, f, v);
        p.out = out;
        HIPCHK(c, launch_vdi_flatten(p, st));
    } else {
        PlainCompParams p{};
        p.V = c->V; p.dim0 = c->W; p.rows = c->rows;
        // PlainImageCompositor.comp:43 as written composites numProcesses = dim0 / rows lists (those past
        // the received ones read as empty): the first min(numProcesses, V)
        if (c->cfg.faithful & INSITU_FAITHFUL_PLAIN_NUM_PROCESSES) p.V = std::min(c->V, c->W / c->rows);
        for (int v = 0; v < c->V; ++v) {
            const int s = v / c->B, b = v % c->B;
            if (s == c->rank) {
                const size_t e = ((size_t)c->rank * (size_t)c->B + (size_t)b) * c->plainBlock;
                p.colors[v] = c->d_pcol_send + e;
                p.depths[v] = c->d_pdep_send + e;
            } else {
                const size_t r = ((size_t)s * (size_t)c->B + (size_t)b) * c->plainBlock;
                p.colors[v] = c->d_pcol_recv + r;
                p.depths[v] = c->d_pdep_recv + r;
            }
        }
        p.out = out;
        HIPCHK(c, launch_plain_composite(p, st));
    }
    record(f, EvCompositeEnd, st);
    f.composited = true;
    return 0;
}

// the gather of slot f's composited frame on stream st (+ the root's image to host_out); blocks until it is done
int gather_frame(insitu_ctx* c, FrameSlot& f, hipStream_t st, void* host_out, size_t cap) {
    if (!f.composited) return fail(c, -1, "insitu_gather: nothing composited");
    if (c->N > 1 && c->group) {   // in-process: the root pulls every peer's strip
        if (is_root(c)) {
            for (int p = 1; p < c->N; ++p) {
                const insitu_ctx* q = c->group->ranks[p];
                if (!q) return fail(c, -1, "insitu_gather: local group rank " + std::to_string(p) + " missing");
                if (!q->cur->composited || !q->cur->ev_valid[EvCompositeEnd]) return fail(c, -1, "insitu_gather: local group rank " + std::to_string(p) + " has not composited");
                HIPCHK(c, hipStreamWaitEvent(st, q->cur->ev[EvCompositeEnd], 0));   // the peer's composite, its stream
                if (c->composite_vdi) {
                    HIPCHK(c, hipMemcpyAsync(c->d_gvdi_col + (size_t)p * c->cblockE, q->d_cvdi_col, c->cblockE * sizeof(float4),
                                             hipMemcpyDeviceToDevice, st));
                    HIPCHK(c, hipMemcpyAsync(c->d_gvdi_dep + (size_t)p * c->cblockE, q->d_cvdi_dep, c->cblockE * sizeof(float2),
                                             hipMemcpyDeviceToDevice, st));
                    HIPCHK(c, hipMemcpyAsync(c->d_gvdi_cnt + (size_t)p * c->stripPx, q->d_cvdi_cnt, c->stripPx * sizeof(uint16_t),
                                             hipMemcpyDeviceToDevice, st));
                } else {
                    HIPCHK(c, hipMemcpyAsync(c->d_gather + (size_t)p * c->stripPx, q->d_strip, c->stripPx * 4,
                                             hipMemcpyDeviceToDevice, st));
                }
            }
        }
    } else if (c->N > 1 && c->composite_vdi) {   // MPI_Gather of the composited VDIs (DistributedVolumes.kt:903)
        NCCLCHK(c, ncclGroupStart());
        if (is_root(c)) {
            for (int p = 1; p < c->N; ++p) {
                NCCLCHK(c, ncclRecv(c->d_gvdi_col + (size_t)p * c->cblockE, c->cblockE * 4, ncclFloat32, p, c->comm,
                                    st));
                NCCLCHK(c, ncclRecv(c->d_gvdi_dep + (size_t)p * c->cblockE, c->cblockE * 2, ncclFloat32, p, c->comm,
                                    st));
                NCCLCHK(c, ncclRecv(c->d_gvdi_cnt + (size_t)p * c->stripPx, c->stripPx * sizeof(uint16_t), ncclUint8, p,
                                    c->comm, st));
            }
        } else {
            NCCLCHK(c, ncclSend(c->d_cvdi_col, c->cblockE * 4, ncclFloat32, 0, c->comm, st));
            NCCLCHK(c, ncclSend(c->d_cvdi_dep, c->cblockE * 2, ncclFloat32, 0, c->comm, st));
            NCCLCHK(c, ncclSend(c->d_cvdi_cnt, c->stripPx * sizeof(uint16_t), ncclUint8, 0, c->comm, st));
        }
        NCCLCHK(c, ncclGroupEnd());
    } else if (c->N > 1) {
        NCCLCHK(c, ncclGroupStart());
        if (is_root(c)) {
            for (int p = 1; p < c->N; ++p)
                NCCLCHK(c, ncclRecv(c->d_gather + (size_t)p * c->stripPx, c->stripPx, ncclUint32, p, c->comm, st));
        } else {
            NCCLCHK(c, ncclSend(c->d_strip, c->stripPx, ncclUint32, 0, c->comm, st));
        }
        NCCLCHK(c, ncclGroupEnd());
    }
    if (is_root(c) && c->composite_vdi) {
        // the root's image: each gathered composited strip flattened front to back (accumulateSupseg)
        for (int p = 0; p < c->N; ++p) {
            FlattenParams fp{};
            fp.V = 1; fp.S = c->S_out; fp.H = c->H; fp.W = c->W;
            fp.strip_w = c->strip_w; fp.strip_tiles = c->strip_tiles; fp.x_offset = p * c->strip_w;
            std::memcpy(fp.ipv, f.ipv, sizeof fp.ipv);
            fp.lists[0].col = c->d_gvdi_col + (size_t)p * c->cblockE;
            fp.lists[0].dep = c->d_gvdi_dep + (size_t)p * c->cblockE;
            fp.lists[0].cnt16 = c->d_gvdi_cnt + (size_t)p * c->stripPx;   // (slots past the count: not written)
            fp.lists[0].cnt_pitch = c->strip_w;
            fp.lists[0].cnt_x0 = 0;
            fp.out = c->d_gather + (size_t)p * c->stripPx;
            HIPCHK(c, launch_vdi_flatten(fp, st));
        }
    }
    if (is_root(c) && c->composite_vdi) {   // what insitu_view_bind(INSITU_VIEW_GATHERED) takes, and its camera
        c->gvdi_valid = true;
        std::memcpy(c->gvdi_pv, f.pv, sizeof c->gvdi_pv);
    }
    if (is_root(c) && c->mode == INSITU_MODE_VDI)
        HIPCHK(c, launch_assemble_columns(c->d_gather, c->N, c->H, c->strip_w, c->d_image, st));
    if (c->group && is_root(c)) record(f, EvPeerReadsDone, st);
    record(f, EvGatherEnd, st);
    if (is_root(c) && host_out) {
        const size_t bytes = (size_t)c->W * (size_t)c->H * 4;
        if (cap < bytes) return fail(c, -1, "insitu_gather: output buffer too small");
        const void* src = c->mode == INSITU_MODE_VDI ? (const void*)c->d_image : (const void*)c->d_gather;
        HIPCHK(c, hipMemcpyAsync(host_out, src, bytes, hipMemcpyDeviceToHost, st));
        record(f, EvImageOnHost, st);
    } else {
        f.ev_valid[EvImageOnHost] = false;
    }
    HIPCHK(c, hipStreamSynchronize(st));
    return check_fault(c, f);
}

// the second frame slot, the sampling and completion streams and the trigger flag (first pipelined frame)
int pipeline_setup(insitu_ctx* c) {
    if (c->pipe_ready) return 0;
    int lo = 0, hi = 0;
    HIPCHK(c, hipDeviceGetStreamPriorityRange(&lo, &hi));   // (greatest priority = numerically smallest)
    // the next frame's first pass fills what the search leaves idle: low priority; the completion of the frame
    // one behind is short and sets the latency: high priority
    HIPCHK(c, hipStreamCreateWithPriority(&c->pipe_sample, hipStreamNonBlocking, lo));
    HIPCHK(c, hipStreamCreateWithPriority(&c->pipe_comp, hipStreamNonBlocking, hi));
    // a search stream per slot: frame k+1's search starts as soon as its first pass is done, beside frame k's
    // search tail and finish (one stream would order it after them)
    for (FrameSlot& f : c->slots) HIPCHK(c, hipStreamCreateWithFlags(&f.search_stream, hipStreamNonBlocking));
    int can_wait = 0;
    if (hipDeviceGetAttribute(&can_wait, hipDeviceAttributeCanUseStreamWaitValue, c->cfg.device) != hipSuccess) can_wait = 0;
    c->pipe_wait_value = can_wait != 0;
    if (c->pipe_wait_value) {
        if (int rc = c->pipe_flag.alloc(c, 2)) return rc;
        HIPCHK(c, hipMemset(c->pipe_flag, 0, 2 * sizeof(unsigned long long)));
    }
    // the second slot starts with the cache size the first one has reached
    if (int rc = alloc_slot(c, c->slots[1], c->slots[0].cache_chunks)) return rc;
    c->slots[1].cache_sized = c->slots[0].cache_sized;
    c->pipe_ready = true;
    return 0;
}

// the stages of slot f's frame after its render, on the completion stream: compaction (N > 1), exchange,
// composite, gather (+ the root's image to host_out); blocks until they are done
int pipeline_complete(insitu_ctx* c, FrameSlot& f, void* host_out, size_t cap) {
    const hipStream_t st = c->pipe_comp;
    if (f.ev_valid[EvRenderEnd] && hipStreamWaitEvent(st, f.ev[EvRenderEnd], 0) != hipSuccess)
        return fail(c, -3, "insitu_frame_pipelined: hipStreamWaitEvent failed");
    if (c->N > 1) {
        hipError_t e = compact_enqueue(c, f, st);
        if (e != hipSuccess) return fail(c, -3, std::string("vdi_compact_kernel: ") + hipGetErrorString(e));
    }
    int rc = exchange_frame(c, f, st);
    if (!rc) rc = composite_frame(c, f, st);
    if (rc) return rc;
    record(f, EvSlotFree, st);   // (recorded before gather's synchronisation: the slot may be rendered into after it)
    return gather_frame(c, f, st, host_out, cap);
}

}  // namespace

// The unpipelined stages work on the completed frame's slot and the context stream, and refuse while a pipelined
// frame is in flight.
int insitu_set_camera(insitu_ctx* c, const insitu_camera* cam) {
    if (!c) return fail(nullptr, -1, "insitu_set_camera: null context");
    FrameCamera m;
    if (int rc = camera_matrices(c, cam, &m)) return rc;
    set_slot_camera(c, *c->cur, m);
    return 0;
}

int insitu_render(insitu_ctx* c, const insitu_camera* cam) {
    if (!c) return fail(nullptr, -1, "insitu_render: null context");
    if (!cam) return fail(c, -1, "insitu_render: null camera");
    if (c->pipe_inflight)
        return fail(c, -1, "insitu_render: a pipelined frame is in flight (insitu_pipeline_flush first)");
    FrameCamera m;
    if (int rc = render_check(c, cam, &m)) return rc;
    HIPCHK(c, hipSetDevice(c->cfg.device));
    RenderPlan plan;
    plan.first = plan.search = c->stream;
    return render_frame(c, *c->cur, m, plan);
}

int insitu_exchange(insitu_ctx* c) {
    if (!c) return fail(nullptr, -1, "insitu_exchange: null context");
    if (c->pipe_inflight)
        return fail(c, -1, "insitu_exchange: a pipelined frame is in flight (insitu_pipeline_flush first)");
    HIPCHK(c, hipSetDevice(c->cfg.device));
    return exchange_frame(c, *c->cur, c->stream);
}

int insitu_composite(insitu_ctx* c) {
    if (!c) return fail(nullptr, -1, "insitu_composite: null context");
    if (c->pipe_inflight)
        return fail(c, -1, "insitu_composite: a pipelined frame is in flight (insitu_pipeline_flush first)");
    HIPCHK(c, hipSetDevice(c->cfg.device));
    return composite_frame(c, *c->cur, c->stream);
}

int insitu_gather(insitu_ctx* c, void* host_out, size_t cap) {
    if (!c) return fail(nullptr, -1, "insitu_gather: null context");
    if (c->pipe_inflight)
        return fail(c, -1, "insitu_gather: a pipelined frame is in flight (insitu_pipeline_flush first)");
    HIPCHK(c, hipSetDevice(c->cfg.device));
    return gather_frame(c, *c->cur, c->stream, host_out, cap);
}

int insitu_frame(insitu_ctx* c, const insitu_camera* cam, void* host_out, size_t cap) {
    int rc;
    if ((rc = insitu_render(c, cam))) return rc;
    if ((rc = insitu_exchange(c))) return rc;
    if ((rc = insitu_composite(c))) return rc;
    return insitu_gather(c, host_out, cap);
}

int insitu_frame_pipelined(insitu_ctx* c, const insitu_camera* cam, void* host_out, size_t cap, long long* done_frame) {
    if (!c) return fail(nullptr, -1, "insitu_frame_pipelined: null context");
    if (done_frame) *done_frame = -1;
    // everything that rejects the call comes first: a rejected call has enqueued and counted nothing, so it
    // leaves the pipeline (the frame in flight, the slots' flags and events) exactly as it was
    if (c->mode != INSITU_MODE_VDI) return fail(c, -1, "insitu_frame_pipelined: VDI mode only");
    if (c->group) return fail(c, -1, "insitu_frame_pipelined: not with a local group (stages run rank by rank)");
    if (!c->cur->cache) return fail(c, -1, "insitu_frame_pipelined: needs the sample cache (sample_cache_mb >= 0)");
    FrameCamera m;
    if (int rc = render_check(c, cam, &m)) return rc;
    HIPCHK(c, hipSetDevice(c->cfg.device));
    if (int rc = pipeline_setup(c)) return rc;
    // 1. frame k into `cur` (its last frame is completed: EvSlotFree was synchronised): the first pass on the
    // sampling stream, the search on the slot's own
    FrameSlot& f = *c->cur;
    RenderPlan plan;
    plan.first = c->pipe_sample;
    plan.search = f.search_stream;
    plan.pipelined = true;
    if (f.ev_valid[EvSlotFree]) HIPCHK(c, hipStreamWaitEvent(plan.first, f.ev[EvSlotFree], 0));
    // everything enqueued on the context stream before this call -- brick ingests (a re-ingest behind the frame
    // in flight waits for that frame's search), LUT uploads, and before the first pipelined frame whatever the
    // context did unpipelined -- is ordered before this frame's first pass, and so before its completion
    HIPCHK(c, hipEventRecord(c->ev_gate, c->stream));
    HIPCHK(c, hipStreamWaitEvent(plan.first, c->ev_gate, 0));
    if (c->pipe_inflight) {
        // the gate of this frame's first pass: the previous frame's search (in `alt`) drains its queue (mode 1:
        // the value that search stores to its slot's flag, kept in the slot; a search that stored none leaves
        // the flag at a value already reached), or ends (mode 0); mode 2 starts it once the previous first pass
        // is done (stream order)
        int mode = c->pipe_trigger;
        if (mode == 1 && !c->pipe_wait_value) mode = 0;
        if (mode == 1) {
            plan.gate_flag = c->pipe_flag + c->alt->flag_index;
            plan.gate_value = c->alt->flag_value;
        } else if (mode == 0 && c->alt->ev_valid[EvSearchEnd]) {
            plan.gate_event = c->alt->ev[EvSearchEnd];
        }
    }
    int rc = render_frame(c, f, m, plan);
    if (rc) return rc;
    const long long k = c->pipe_frames++;
    // 2. frame k is now the one in flight (`alt`); the frame one behind (`cur`): exchange, composite, gather --
    // while frame k renders
    swap_slot(c);
    const bool behind = c->pipe_inflight;
    c->pipe_inflight = true;
    if (!behind) return 0;
    rc = pipeline_complete(c, *c->cur, host_out, cap);
    if (rc) return rc;
    if (done_frame) *done_frame = k - 1;
    return 0;
}

int insitu_pipeline_flush(insitu_ctx* c, void* host_out, size_t cap, long long* done_frame) {
    if (!c) return fail(nullptr, -1, "insitu_pipeline_flush: null context");
    if (done_frame) *done_frame = -1;
    if (!c->pipe_inflight) return 0;
    HIPCHK(c, hipSetDevice(c->cfg.device));
    swap_slot(c);   // the frame in flight becomes the completed one
    int rc = pipeline_complete(c, *c->cur, host_out, cap);
    c->pipe_inflight = false;
    if (rc) return rc;
    if (done_frame) *done_frame = c->pipe_frames - 1;
    return 0;
}

int insitu_synchronize(insitu_ctx* c) {
    if (!c) return fail(nullptr, -1, "insitu_synchronize: null context");
    HIPCHK(c, hipSetDevice(c->cfg.device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    for (hipStream_t st : {c->pipe_sample, c->pipe_comp})
        if (st) HIPCHK(c, hipStreamSynchronize(st));
    for (FrameSlot& f : c->slots)
        if (f.search_stream) HIPCHK(c, hipStreamSynchronize(f.search_stream));
    if (c->dbg_pending) {   // diagnostics: the last render's per-round search timing, all launches
        c->dbg_pending = false;
        std::vector<unsigned long long> h(c->dbg_entries * 4);
        GenCounters gc{};
        HIPCHK(c, hipMemcpy(h.data(), c->d_dbg, h.size() * 8, hipMemcpyDeviceToHost));
        HIPCHK(c, hipMemcpy(&gc, completed_frame(c).f.counters, sizeof gc, hipMemcpyDeviceToHost));
        if (FILE* f = std::fopen(c->dbg_path.c_str(), "wb")) {   // sizeof counters, counters, the non-empty entries
            const uint32_t hdr = (uint32_t)sizeof gc;
            std::fwrite(&hdr, sizeof hdr, 1, f);
            std::fwrite(&gc, sizeof gc, 1, f);
            for (size_t i = 0; i < c->dbg_entries; ++i)
                if (h[4 * i + 1]) std::fwrite(&h[4 * i], 32, 1, f);
            std::fclose(f);
        }
    }
    return check_fault(c, completed_frame(c).f);
}

size_t insitu_buffer_bytes(const insitu_ctx* c, int which) {
    if (!c) return 0;
    const size_t px = (size_t)c->W * (size_t)c->H;
    switch (which) {
    case INSITU_BUF_VDI_COLOR: return c->mode == INSITU_MODE_VDI ? px * (size_t)c->S * 16 : 0;
    case INSITU_BUF_VDI_DEPTH: return c->mode == INSITU_MODE_VDI ? px * (size_t)c->S * 8 : 0;
    case INSITU_BUF_OCTREE: return c->mode == INSITU_MODE_VDI ? (size_t)c->ncx * c->ncy * c->S * 4 : 0;
    case INSITU_BUF_PASSES: return (c->mode == INSITU_MODE_VDI && completed_frame(c).f.passes) ? px : 0;
    case INSITU_BUF_PLAIN_COLOR:
    case INSITU_BUF_PLAIN_DEPTH: return c->mode == INSITU_MODE_PLAIN ? px * 4 : 0;
    case INSITU_BUF_STRIP: return c->stripPx * 4;
    case INSITU_BUF_IMAGE: return is_root(c) ? px * 4 : 0;
    case INSITU_BUF_COMPOSITED_COLOR: return c->composite_vdi ? c->stripPx * (size_t)c->S_out * 16 : 0;
    case INSITU_BUF_COMPOSITED_DEPTH: return c->composite_vdi ? c->stripPx * (size_t)c->S_out * 8 : 0;
    case INSITU_BUF_GATHERED_COLOR: return (c->composite_vdi && is_root(c)) ? px * (size_t)c->S_out * 16 : 0;
    case INSITU_BUF_GATHERED_DEPTH: return (c->composite_vdi && is_root(c)) ? px * (size_t)c->S_out * 8 : 0;
    case INSITU_BUF_COMPOSITE_PASSES: return c->composite_vdi ? c->stripPx : 0;
    case INSITU_BUF_RECEIVED_COLOR: return (c->mode == INSITU_MODE_VDI && completed_frame(c).f.exchanged) ? (size_t)c->V * c->stripPx * c->S * 16 : 0;
    case INSITU_BUF_RECEIVED_DEPTH: return (c->mode == INSITU_MODE_VDI && completed_frame(c).f.exchanged) ? (size_t)c->V * c->stripPx * c->S * 8 : 0;
    case INSITU_BUF_VIEW_COLOR: return (size_t)c->view.out_w * (size_t)c->view.out_h * 16;
    case INSITU_BUF_VIEW_IMAGE: return (size_t)c->view.out_w * (size_t)c->view.out_h * 4;
    default: return 0;
    }
}

int insitu_read(insitu_ctx* c, int which, int slot, void* host_out, size_t cap) {
    if (!c) return fail(nullptr, -1, "insitu_read: null context");
    auto [f, st] = completed_frame(c);
    if (!host_out) return fail(c, -1, "insitu_read: null output");
    const size_t need = insitu_buffer_bytes(c, which);
    if (need == 0) return fail(c, -1, "insitu_read: buffer not available in this mode/rank");
    if (cap < need) return fail(c, -1, "insitu_read: output buffer too small");
    if (which == INSITU_BUF_VIEW_COLOR || which == INSITU_BUF_VIEW_IMAGE) {   // (insitu_view_render blocked: ready)
        HIPCHK(c, hipSetDevice(c->cfg.device));
        HIPCHK(c, hipMemcpy(host_out, which == INSITU_BUF_VIEW_COLOR ? (const void*)c->view.out_color : (const void*)c->view.out_image,
                            need, hipMemcpyDeviceToHost));
        return 0;
    }
    const bool per_brick = which <= INSITU_BUF_PLAIN_DEPTH;
    if (per_brick && (slot < 0 || slot >= (c->mode == INSITU_MODE_VDI ? c->BV : c->B)))
        return fail(c, -1, "insitu_read: slot out of range");
    HIPCHK(c, hipSetDevice(c->cfg.device));
    HIPCHK(c, hipStreamSynchronize(st));
    if (int rc = check_fault(c, f)) return rc;
    switch (which) {
    case INSITU_BUF_VDI_COLOR:
    case INSITU_BUF_VDI_DEPTH: {
        const size_t n = (size_t)c->W * (size_t)c->H * (size_t)c->S;
        DevBuf<float4> rc;   // (the scratch pair is freed at scope exit, after the synchronisation below)
        DevBuf<float> rd;
        HIPCHK(c, rc.try_alloc(n));
        if (rd.try_alloc(n * 2) != hipSuccess) return fail(c, -5, "insitu_read: scratch allocation failed");
        hipError_t e = launch_vdi_to_reference(f.vcol_send, f.vdep_send, f.seg_pending,
                                               (size_t)c->W * (size_t)c->H, (size_t)c->strip_w, (size_t)c->W, c->W, 0, c->W,
                                               c->H, c->S, c->strip_w, c->strip_tiles, c->BV, slot, rc, rd, st);
        if (e == hipSuccess)
            e = hipMemcpyAsync(host_out, which == INSITU_BUF_VDI_COLOR ? (void*)rc : (void*)rd, need,
                               hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        if (e != hipSuccess) return fail(c, -3, std::string("insitu_read: ") + hipGetErrorString(e));
        return 0;
    }
    case INSITU_BUF_OCTREE:
        HIPCHK(c, hipMemcpy(host_out, f.octree + (size_t)slot * (need / 4), need, hipMemcpyDeviceToHost));
        return 0;
    case INSITU_BUF_PASSES:
        HIPCHK(c, hipMemcpy(host_out, f.passes + (size_t)slot * need, need, hipMemcpyDeviceToHost));
        return 0;
    case INSITU_BUF_PLAIN_COLOR:
    case INSITU_BUF_PLAIN_DEPTH: {
        const uint32_t* src = which == INSITU_BUF_PLAIN_COLOR ? c->d_pcol_send : c->d_pdep_send;
        for (int d = 0; d < c->N; ++d)
            HIPCHK(c, hipMemcpy((uint8_t*)host_out + (size_t)d * c->plainBlock * 4,
                                src + ((size_t)d * (size_t)c->B + (size_t)slot) * c->plainBlock, c->plainBlock * 4,
                                hipMemcpyDeviceToHost));
        return 0;
    }
    case INSITU_BUF_STRIP: {
        const uint32_t* src = is_root(c) ? c->d_gather + (size_t)c->rank * c->stripPx : c->d_strip;
        HIPCHK(c, hipMemcpy(host_out, src, need, hipMemcpyDeviceToHost));
        return 0;
    }
    case INSITU_BUF_IMAGE: {
        const void* src = c->mode == INSITU_MODE_VDI ? (const void*)c->d_image : (const void*)c->d_gather;
        HIPCHK(c, hipMemcpy(host_out, src, need, hipMemcpyDeviceToHost));
        return 0;
    }
    case INSITU_BUF_COMPOSITED_COLOR:
    case INSITU_BUF_COMPOSITED_DEPTH:
    case INSITU_BUF_GATHERED_COLOR:
    case INSITU_BUF_GATHERED_DEPTH: {
        const bool gathered = which == INSITU_BUF_GATHERED_COLOR || which == INSITU_BUF_GATHERED_DEPTH;
        const bool colour = which == INSITU_BUF_COMPOSITED_COLOR || which == INSITU_BUF_GATHERED_COLOR;
        const int width = gathered ? c->W : c->strip_w;
        const size_t n = (size_t)width * (size_t)c->H * (size_t)c->S_out;
        DevBuf<float4> rc;
        DevBuf<float> rd;
        HIPCHK(c, rc.try_alloc(n));
        if (rd.try_alloc(n * 2) != hipSuccess) return fail(c, -5, "insitu_read: scratch allocation failed");
        // gathered: N blocks [rank] of one strip each; a single strip: one block
        // (the slots past each pixel's count are not written by the compositor: zeros here)
        hipError_t e = launch_vdi_to_reference(gathered ? c->d_gvdi_col : cvdi_col(c), gathered ? c->d_gvdi_dep : cvdi_dep(c),
                                               gathered ? c->d_gvdi_cnt : cvdi_cnt(c), 0, c->stripPx, (size_t)c->strip_w,
                                               width, 0, width, c->H, c->S_out, c->strip_w, c->strip_tiles, 1, 0, rc, rd,
                                               st);
        if (e == hipSuccess)
            e = hipMemcpyAsync(host_out, colour ? (void*)rc : (void*)rd, need, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        if (e != hipSuccess) return fail(c, -3, std::string("insitu_read: ") + hipGetErrorString(e));
        return 0;
    }
    case INSITU_BUF_COMPOSITE_PASSES:
        HIPCHK(c, hipMemcpy(host_out, c->d_cpasses, need, hipMemcpyDeviceToHost));
        return 0;
    case INSITU_BUF_RECEIVED_COLOR:
    case INSITU_BUF_RECEIVED_DEPTH: {   // block v = list v of the compositor (source-major)
        const size_t n = c->stripPx * (size_t)c->S;
        DevBuf<float4> rc;
        DevBuf<float2> rd;
        HIPCHK(c, rc.try_alloc(n));
        if (rd.try_alloc(n) != hipSuccess) return fail(c, -5, "insitu_read: scratch allocation failed");
        const bool colour = which == INSITU_BUF_RECEIVED_COLOR;
        const size_t blk = colour ? n * sizeof(float4) : n * sizeof(float2);
        hipError_t e = hipSuccess;
        for (int v = 0; v < c->V && e == hipSuccess; ++v) {
            e = launch_vdi_list_to_reference(list_of(c, f, v), c->S, c->H, c->strip_w, c->strip_tiles, rc, rd, st);
            if (e == hipSuccess)
                e = hipMemcpyAsync((uint8_t*)host_out + (size_t)v * blk, colour ? (void*)rc : (void*)rd, blk,
                                   hipMemcpyDeviceToHost, st);
            if (e == hipSuccess) e = hipStreamSynchronize(st);
        }
        if (e != hipSuccess) return fail(c, -3, std::string("insitu_read: ") + hipGetErrorString(e));
        return 0;
    }
    default: return fail(c, -1, "insitu_read: unknown buffer");
    }
}

int insitu_read_region(insitu_ctx* c, int which, int slot, int x0, int x1, void* host_out, size_t cap) {
    if (!c) return fail(nullptr, -1, "insitu_read_region: null context");
    auto [f, st] = completed_frame(c);
    if (!host_out) return fail(c, -1, "insitu_read_region: null output");
    if (c->mode != INSITU_MODE_VDI) return fail(c, -1, "insitu_read_region: VDI mode only");
    if (which != INSITU_BUF_VDI_COLOR && which != INSITU_BUF_VDI_DEPTH && which != INSITU_BUF_PASSES)
        return fail(c, -1, "insitu_read_region: buffer must be VDI colour, VDI depth or passes");
    if (slot < 0 || slot >= c->BV) return fail(c, -1, "insitu_read_region: slot out of range");
    if (x0 < 0 || x1 > c->W || x0 >= x1) return fail(c, -1, "insitu_read_region: bad column range");
    const size_t nx = (size_t)(x1 - x0);
    const size_t n = nx * (size_t)c->H * (size_t)c->S;
    const size_t need = which == INSITU_BUF_VDI_COLOR ? n * 16 : (which == INSITU_BUF_VDI_DEPTH ? n * 8 : nx * (size_t)c->H);
    if (cap < need) return fail(c, -1, "insitu_read_region: output buffer too small");
    if (which == INSITU_BUF_PASSES && !f.passes) return fail(c, -1, "insitu_read_region: context keeps no pass counts");
    HIPCHK(c, hipSetDevice(c->cfg.device));
    HIPCHK(c, hipStreamSynchronize(st));
    if (int rc = check_fault(c, f)) return rc;
    if (which == INSITU_BUF_PASSES) {   // (H, x1-x0) rows of the (H, W) pass counts
        HIPCHK(c, hipMemcpy2D(host_out, nx, f.passes + (size_t)slot * (size_t)c->W * (size_t)c->H + (size_t)x0,
                              (size_t)c->W, nx, (size_t)c->H, hipMemcpyDeviceToHost));
        return 0;
    }
    // the kernel writes both outputs: the one not asked for is a throwaway (both freed at scope exit)
    DevBuf<float4> rc_;
    DevBuf<float> rd_;
    hipError_t e = rc_.try_alloc(n);
    if (e == hipSuccess) e = rd_.try_alloc(n * 2);
    if (e == hipSuccess)
        e = launch_vdi_to_reference(f.vcol_send, f.vdep_send, f.seg_pending, (size_t)c->W * (size_t)c->H,
                                    (size_t)c->strip_w, (size_t)c->W, c->W, x0, (int)nx, c->H, c->S, c->strip_w,
                                    c->strip_tiles, c->BV, slot, rc_, rd_, st);
    if (e == hipSuccess)
        e = hipMemcpyAsync(host_out, which == INSITU_BUF_VDI_COLOR ? (void*)rc_ : (void*)rd_, need, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) return fail(c, -3, std::string("insitu_read_region: ") + hipGetErrorString(e));
    return 0;
}

namespace {

// the view's stream and events (first bind)
int view_stream(insitu_ctx* c) {
    ViewState& v = c->view;
    if (!v.stream) HIPCHK(c, hipStreamCreateWithFlags(&v.stream, hipStreamNonBlocking));
    if (!v.ev0) HIPCHK(c, hipEventCreate(&v.ev0));
    if (!v.ev1) HIPCHK(c, hipEventCreate(&v.ev1));
    return 0;
}

// room for `entries` list entries of the VDI being bound
int view_reserve_entries(insitu_ctx* c, size_t entries) {
    ViewState& v = c->view;
    int rc = 0;
    if ((rc = v.col.reserve(c, entries)) || (rc = v.dep.reserve(c, entries))) return rc;
    v.vdi.col = v.col; v.vdi.dep = v.dep;
    return 0;
}

// ... and room for a VDI of (W, H, S) in the view layout this bind takes (INSITU_OPT_VIEW_COMPACT as it stands now;
// the bound VDI keeps it).  Dense: everything.  Compact: the counts, the tile maxima and the offsets; the entries
// are reserved once the counts are there and add up to E (view_compact_offsets).
int view_reserve(insitu_ctx* c, int W, int H, int S) {
    ViewState& v = c->view;
    if (int rc = view_stream(c)) return rc;
    v.bound = false;
    v.counted = false;
    v.vdi = ViewVdi{};
    const bool compact = v.compact_next != 0;
    ViewLayoutSize sz{};
    if (compact ? !view_compact_size(W, H, S, 0, &sz) : !view_dense_size(W, H, S, &sz))
        return fail(c, -1, "view bind: needs W, H > 0, at most 2^30 pixels and S in [1,255]");
    int rc = 0;
    if ((rc = v.cnt.reserve(c, (size_t)sz.px)) || (rc = v.tmax.reserve(c, (size_t)sz.tiles))) return rc;
    if (compact) {
        if ((rc = v.loc.reserve(c, (size_t)sz.px)) || (rc = v.pk_totals.reserve(c, 1)) ||
            (rc = v.pk_bstat.reserve(c, (size_t)sz.nblocks)) || (rc = v.pk_boff.reserve(c, (size_t)sz.nblocks)))
            return rc;
        v.vdi.loc = v.loc; v.vdi.boff = v.pk_boff;
    }
    v.vdi.cnt = v.cnt; v.vdi.tmax = v.tmax;
    v.vdi.W = W; v.vdi.H = H; v.vdi.S = S; v.vdi.tiles_x = (W + 7) / 8; v.vdi.tiles_y = (H + 7) / 8;
    return compact ? 0 : view_reserve_entries(c, (size_t)sz.entries);
}

int pack_offsets(insitu_ctx* c, int check_E, unsigned long long expect_E, PackTotals* tot, float* ms, const char* who,
                 bool timing_open = false);

// The compact layout once its counts are on the device (after ev0 on the view's stream, which is what *ms counts
// from): the offset passes -- boff, loc and E -- and room for the E entries (at least 1).  Blocks.  With check_E
// the counts are a stream's: *tot tells the caller when they are to be rejected, and nothing is reserved then.
int view_compact_offsets(insitu_ctx* c, int check_E, unsigned long long expect_E, PackTotals* tot, float* ms, const char* who) {
    ViewState& v = c->view;
    if (int rc = pack_offsets(c, check_E, expect_E, tot, ms, who, true)) return rc;
    if (tot->bad) return check_E ? 0 : fail(c, -6, std::string(who) + ": a count of the VDI exceeds S (internal error)");
    v.pk_E = tot->E;
    v.counted = true;
    return view_reserve_entries(c, tot->E > 0 ? (size_t)tot->E : 1);
}

// view_build_kernel over `src` on the view's stream (compact: the count pass, the offsets, the write pass); blocks
// until the snapshot is built
int view_build(insitu_ctx* c, const ViewSource& src, const float* pv_g, const char* who) {
    ViewState& v = c->view;
    float ms_index = 0.0f;
    HIPCHK(c, hipEventRecord(v.ev0, v.stream));
    hipError_t e = hipSuccess;
    if (v.vdi.loc) {
        e = launch_view_build_count(src, v.vdi, v.stream);
        if (e != hipSuccess) return fail(c, -3, std::string(who) + ": view_build_count_kernel: " + hipGetErrorString(e));
        PackTotals tot{};
        if (int rc = view_compact_offsets(c, 0, 0, &tot, &ms_index, who)) return rc;
        HIPCHK(c, hipEventRecord(v.ev0, v.stream));
        e = launch_view_build_fill(src, v.vdi, v.stream);
    } else {
        e = launch_view_build(src, v.vdi, v.stream);
    }
    if (e == hipSuccess) e = hipEventRecord(v.ev1, v.stream);
    if (e == hipSuccess) e = hipStreamSynchronize(v.stream);
    if (e != hipSuccess) return fail(c, -3, std::string(who) + ": view_build_kernel: " + hipGetErrorString(e));
    float ms = 0.0f;
    if (hipEventElapsedTime(&ms, v.ev0, v.ev1) == hipSuccess) v.ms_bind = ms_index + ms;
    std::memcpy(v.pv_g, pv_g, sizeof v.pv_g);
    v.overlaps = 0;
    v.bound = true;
    return 0;
}

// After one of the two merge kernels' launches (e) on the view's stream, behind ev0: the totals on the host; blocks.
// *ms = the kernel's HIP-event time.
int view_merge_done(insitu_ctx* c, hipError_t e, const char* who, const char* kernel, MergeTotals* tot, float* ms) {
    ViewState& v = c->view;
    if (e != hipSuccess) return fail(c, -3, std::string(who) + ": " + kernel + ": " + hipGetErrorString(e));
    HIPCHK(c, hipEventRecord(v.ev1, v.stream));
    HIPCHK(c, hipMemcpyAsync(v.h_mg_totals, v.mg_totals, sizeof(MergeTotals), hipMemcpyDeviceToHost, v.stream));
    HIPCHK(c, hipStreamSynchronize(v.stream));
    *tot = *v.h_mg_totals;
    *ms = 0.0f;
    (void)hipEventElapsedTime(ms, v.ev0, v.ev1);
    return 0;
}

// The merged bind: the src.n lists per pixel of a (W, H) window of S-slot lists, merged by start
// depth into a VDI of S_m = max(1, the longest merged list) slots.  More than 255 is rejected and leaves no VDI
// bound.  Blocks until the snapshot is built.
int view_merge(insitu_ctx* c, const ViewSource& src, int W, int H, int S, const float* pv_g, const char* who) {
    ViewState& v = c->view;
    v.bound = false;
    v.counted = false;
    if (int rc = view_stream(c)) return rc;
    if (int rc = v.mg_totals.reserve(c, 1)) return rc;
    if (!v.h_mg_totals) HIPCHK(c, v.h_mg_totals.try_alloc(1));
    MergeTotals tot{};
    float ms_count = 0.0f, ms_merge = 0.0f, ms_index = 0.0f;
    // compact: the count pass leaves every pixel's merged length as its count (the slots are known after it)
    const bool compact = v.compact_next != 0;
    if (compact)
        if (int rc = view_reserve(c, W, H, 1)) return rc;
    HIPCHK(c, hipEventRecord(v.ev0, v.stream));
    if (int rc = view_merge_done(c, launch_view_merge_count(src, W, H, S, v.mg_totals, compact ? v.vdi.cnt : nullptr, v.stream),
                                 who, "view_merge_count_kernel", &tot, &ms_count))
        return rc;
    if (tot.max_count > 255u)
        return fail(c, -1, std::string(who) + ": the merged lists hold up to " + std::to_string(tot.max_count) +
                               " entries per pixel, at most 255 can be bound");
    const int Sm = tot.max_count > 0u ? (int)tot.max_count : 1;
    if (compact) {
        v.vdi.S = Sm;
        PackTotals ptot{};
        HIPCHK(c, hipEventRecord(v.ev0, v.stream));
        if (int rc = view_compact_offsets(c, 0, 0, &ptot, &ms_index, who)) return rc;
    } else if (int rc = view_reserve(c, W, H, Sm)) {
        return rc;
    }
    HIPCHK(c, hipEventRecord(v.ev0, v.stream));
    if (int rc = view_merge_done(c, launch_view_merge(src, S, v.vdi, v.mg_totals, v.stream), who, "view_merge_kernel", &tot,
                                 &ms_merge))
        return rc;
    v.ms_bind = ms_count + ms_index + ms_merge;
    v.overlaps = (long long)tot.overlaps;
    std::memcpy(v.pv_g, pv_g, sizeof v.pv_g);
    v.bound = true;
    return 0;
}

}  // namespace

int insitu_view_bind(insitu_ctx* c, int source, int slot) {
    if (!c) return fail(nullptr, -1, "insitu_view_bind: null context");
    if (source == INSITU_VIEW_MERGED) {   // (a failed merged bind leaves no VDI bound)
        c->view.bound = false;
        c->view.counted = false;
    }
    if (c->mode != INSITU_MODE_VDI) return fail(c, -1, "insitu_view_bind: VDI mode only");
    auto [f, st] = completed_frame(c);
    ViewSource src{};
    src.n = 1;
    const float* pv = nullptr;
    int S = 0;
    if (source == INSITU_VIEW_GATHERED) {
        if (!c->composite_vdi) return fail(c, -1, "insitu_view_bind: the gathered VDI needs a composite_vdi context");
        if (!is_root(c)) return fail(c, -1, "insitu_view_bind: the gathered VDI is on rank 0 only");
        if (!c->gvdi_valid) return fail(c, -1, "insitu_view_bind: no frame gathered yet");
        src.col = c->d_gvdi_col; src.dep = c->d_gvdi_dep; src.cnt = c->d_gvdi_cnt;
        src.cnt_stride = 0; src.cnt_dstride = c->stripPx; src.cnt_pitch = (size_t)c->strip_w;
        src.B = 1; src.b = 0;
        S = c->S_out;
        pv = c->gvdi_pv;
    } else if (source == INSITU_VIEW_BRICK || source == INSITU_VIEW_MERGED) {
        if (source == INSITU_VIEW_MERGED && slot != 0)
            return fail(c, -1, "insitu_view_bind: INSITU_VIEW_MERGED takes slot 0 (it binds every sub-VDI of the rank)");
        if (slot < 0 || slot >= c->BV) return fail(c, -1, "insitu_view_bind: slot out of range");
        if (!f.rendered || !f.ev_valid[EvRenderEnd]) return fail(c, -1, "insitu_view_bind: no frame rendered yet");
        src.col = f.vcol_send; src.dep = f.vdep_send; src.cnt = f.seg_pending;
        src.cnt_stride = (size_t)c->W * (size_t)c->H; src.cnt_dstride = (size_t)c->strip_w; src.cnt_pitch = (size_t)c->W;
        src.B = c->BV; src.b = slot;
        if (source == INSITU_VIEW_MERGED) src.n = c->BV;   // slots 0..BV-1: the whole window
        S = c->S;
        pv = f.pv;
    } else {
        return fail(c, -1, "insitu_view_bind: unknown source " + std::to_string(source));
    }
    src.strip_w = c->strip_w; src.strip_tiles = c->strip_tiles;
    HIPCHK(c, hipSetDevice(c->cfg.device));
    // the frame's own work is done before the snapshot is taken (its render may still be running when no
    // stage after it has synchronised)
    HIPCHK(c, hipStreamSynchronize(st));
    if (f.search_stream) HIPCHK(c, hipStreamSynchronize(f.search_stream));
    if (int rc = check_fault(c, f)) return rc;
    // (a set of one list is that list: bound with its own S slots, as INSITU_VIEW_BRICK binds it)
    if (src.n > 1) return view_merge(c, src, c->W, c->H, S, pv, "insitu_view_bind");
    if (int rc = view_reserve(c, c->W, c->H, S)) return rc;
    return view_build(c, src, pv, "insitu_view_bind");
}

namespace {

// n dense VDIs in the reference layout, staged on the device and bound: one as it is (view_build_kernel, S slots),
// several merged (view_merge)
int view_bind_host_lists(insitu_ctx* c, const char* who, const void* const* colors, const void* const* depths, int n,
                         int W, int H, int S, const insitu_camera* gen_cam) {
    if (W <= 0 || H <= 0 || S < 1 || S > 255) return fail(c, -1, std::string(who) + ": needs W, H > 0 and S in [1,255]");
    float pv[16];
    mat4_mul_f(gen_cam->proj, gen_cam->view, pv);
    HIPCHK(c, hipSetDevice(c->cfg.device));
    if (n == 1) {
        if (int rc = view_reserve(c, W, H, S)) return rc;
    } else if (int rc = view_stream(c)) {
        return rc;
    }
    const size_t E = (size_t)W * (size_t)H * (size_t)S;
    DevBuf<float4> rc_;   // (the staging pair is freed at scope exit: the view's stream is idle by then)
    DevBuf<float2> rd_;
    HIPCHK(c, rc_.try_alloc(E * (size_t)n));
    if (rd_.try_alloc(E * (size_t)n) != hipSuccess) return fail(c, -5, std::string(who) + ": staging allocation failed");
    hipError_t e = hipSuccess;
    for (int j = 0; j < n && e == hipSuccess; ++j) {
        e = hipMemcpyAsync(rc_ + E * (size_t)j, colors[j], E * sizeof(float4), hipMemcpyHostToDevice, c->view.stream);
        if (e == hipSuccess)
            e = hipMemcpyAsync(rd_ + E * (size_t)j, depths[j], E * sizeof(float2), hipMemcpyHostToDevice, c->view.stream);
    }
    if (e != hipSuccess) {
        (void)hipStreamSynchronize(c->view.stream);
        return fail(c, -3, std::string(who) + ": upload: " + hipGetErrorString(e));
    }
    ViewSource src{};
    src.col = rc_;
    src.dep = rd_;
    src.reference = 1;
    src.ref_stride = E;
    src.n = n;
    // (both block: the staging is free afterwards)
    if (n == 1) return view_build(c, src, pv, who);
    return view_merge(c, src, W, H, S, pv, who);
}

}  // namespace

int insitu_view_bind_host(insitu_ctx* c, const void* color, const void* depth, int W, int H, int S,
                          const insitu_camera* gen_cam) {
    if (!c) return fail(nullptr, -1, "insitu_view_bind_host: null context");
    if (!color || !depth || !gen_cam) return fail(c, -1, "insitu_view_bind_host: null argument");
    return view_bind_host_lists(c, "insitu_view_bind_host", &color, &depth, 1, W, H, S, gen_cam);
}

int insitu_view_bind_host_set(insitu_ctx* c, const void* const* colors, const void* const* depths, int n, int W, int H,
                              int S, const insitu_camera* gen_cam) {
    const char* who = "insitu_view_bind_host_set";
    if (!c) return fail(nullptr, -1, std::string(who) + ": null context");
    c->view.bound = false;   // (a failed bind leaves no VDI bound)
    c->view.counted = false;
    if (!colors || !depths || !gen_cam) return fail(c, -1, std::string(who) + ": null argument");
    if (n < 1 || n > kMaxLists)
        return fail(c, -1, std::string(who) + ": " + std::to_string(n) + " VDIs, needs 1 to " + std::to_string(kMaxLists));
    for (int j = 0; j < n; ++j)
        if (!colors[j] || !depths[j]) return fail(c, -1, std::string(who) + ": null VDI " + std::to_string(j));
    return view_bind_host_lists(c, who, colors, depths, n, W, H, S, gen_cam);
}

// ---- the packed stream of the bound VDI (vdi_pack.hip, vdi_pack_format.h) ----
namespace {

// the offset buffers for the bound dimensions, the totals and their pinned copy; the offset passes
// (pack_count_kernel, pack_scan_kernel) over the view's counts on the view's stream.  Blocks; *tot = what they
// found, *ms = their HIP-event time (timing_open: from the ev0 the caller has recorded, with its own pass over the
// counts behind it).  A compact VDI in the making gets its loc with them.
int pack_offsets(insitu_ctx* c, int check_E, unsigned long long expect_E, PackTotals* tot, float* ms, const char* who,
                 bool timing_open) {
    ViewState& v = c->view;
    const uint64_t px = (uint64_t)v.vdi.W * (uint64_t)v.vdi.H;
    if (px > kPackMaxPixels) return fail(c, -1, std::string(who) + ": more than 2^30 pixels");
    const size_t blocks = (size_t)((px + (uint64_t)kPackBlockPx - 1) / (uint64_t)kPackBlockPx);
    int rc = 0;
    if ((rc = v.pk_totals.reserve(c, 1)) || (rc = v.pk_bstat.reserve(c, blocks)) || (rc = v.pk_boff.reserve(c, blocks)))
        return rc;
    if (!v.h_totals) HIPCHK(c, v.h_totals.try_alloc(1));
    const PackOffsets o{v.vdi.cnt, v.pk_bstat, v.pk_boff, v.pk_totals, (uint32_t)px, (uint32_t)blocks,
                        v.vdi.loc ? v.loc.get() : nullptr};
    if (!timing_open) HIPCHK(c, hipEventRecord(v.ev0, v.stream));
    hipError_t e = launch_pack_offsets(o, v.vdi.S, check_E, expect_E, v.stream);
    if (e != hipSuccess) return fail(c, -3, std::string(who) + ": pack_count_kernel: " + hipGetErrorString(e));
    HIPCHK(c, hipEventRecord(v.ev1, v.stream));
    HIPCHK(c, hipMemcpyAsync(v.h_totals, v.pk_totals, sizeof(PackTotals), hipMemcpyDeviceToHost, v.stream));
    HIPCHK(c, hipStreamSynchronize(v.stream));
    *tot = *v.h_totals;
    *ms = 0.0f;
    (void)hipEventElapsedTime(ms, v.ev0, v.ev1);
    return 0;
}

// E and the block offsets of the bound VDI: counted once per bind
int pack_count_bound(insitu_ctx* c, float* ms, const char* who) {
    ViewState& v = c->view;
    *ms = 0.0f;
    if (v.counted) return 0;
    PackTotals tot{};
    if (int rc = pack_offsets(c, 0, 0, &tot, ms, who)) return rc;
    if (tot.bad) return fail(c, -6, std::string(who) + ": a count of the bound VDI exceeds S (internal error)");
    v.pk_E = tot.E;
    v.counted = true;
    return 0;
}

// room for the two sections on the device: depth at 0, colour at the next multiple of 16 (*colour_at)
int pack_stage_reserve(insitu_ctx* c, const PackLayout& lay, size_t* colour_at) {
    ViewState& v = c->view;
    *colour_at = (lay.depth_bytes + 15) & ~(size_t)15;
    return v.pk_stage.reserve(c, *colour_at + lay.colour_bytes);
}

bool pack_format_ok(int format) { return format == INSITU_PACK_FLOAT || format == INSITU_PACK_HALF; }

}  // namespace

size_t insitu_view_pack_bytes(insitu_ctx* c, int format) {
    const char* err = nullptr;
    PackLayout lay{};
    float ms = 0.0f;
    if (!c) err = "null context";
    else if (!pack_format_ok(format)) err = "bad format";
    else if (!c->view.bound) err = "no VDI bound (insitu_view_bind first)";
    else if (hipSetDevice(c->cfg.device) != hipSuccess) err = "hipSetDevice failed";
    else if (pack_count_bound(c, &ms, "insitu_view_pack_bytes")) return 0;   // (its message stands)
    else if (!pack_layout((uint32_t)format, (uint32_t)c->view.vdi.W, (uint32_t)c->view.vdi.H, (uint32_t)c->view.vdi.S,
                          c->view.pk_E, &lay)) err = "the stream's size does not fit";
    if (err) {
        fail(c, -1, std::string("insitu_view_pack_bytes: ") + err);
        return 0;
    }
    return lay.total;
}

int insitu_view_pack(insitu_ctx* c, int format, void* host_out, size_t cap, size_t* bytes) {
    if (!c) return fail(nullptr, -1, "insitu_view_pack: null context");
    ViewState& v = c->view;
    if (!pack_format_ok(format)) return fail(c, -1, "insitu_view_pack: bad format " + std::to_string(format));
    if (!v.bound) return fail(c, -1, "insitu_view_pack: no VDI bound (insitu_view_bind first)");
    HIPCHK(c, hipSetDevice(c->cfg.device));
    float ms_count = 0.0f;
    if (int rc = pack_count_bound(c, &ms_count, "insitu_view_pack")) return rc;
    PackHeader h{};
    h.format = (uint32_t)format; h.W = (uint32_t)v.vdi.W; h.H = (uint32_t)v.vdi.H; h.S = (uint32_t)v.vdi.S;
    h.E = v.pk_E;
    std::memcpy(h.pv_g, v.pv_g, sizeof h.pv_g);
    PackLayout lay{};
    if (!pack_layout(h.format, h.W, h.H, h.S, h.E, &lay)) return fail(c, -1, "insitu_view_pack: the stream's size does not fit");
    if (bytes) *bytes = lay.total;
    if (!host_out || cap < lay.total)
        return fail(c, -1, "insitu_view_pack: output buffer too small (" + std::to_string(lay.total) + " bytes needed)");
    if (v.vdi.loc) {
        // compact: the bound VDI's arrays are the sections (FLOAT: three copies and no kernel, so ms_pack is 0;
        // HALF: the colours converted element by element)
        unsigned char* out = static_cast<unsigned char*>(host_out);
        const bool half = format == INSITU_PACK_HALF;
        if (half && h.E > 0)
            if (int rc = v.pk_stage.reserve(c, lay.colour_bytes)) return rc;
        HIPCHK(c, hipEventRecord(v.ev0, v.stream));
        if (half && h.E > 0) {
            hipError_t e = launch_pack_convert(v.vdi.col, v.pk_stage, h.E, 1, v.stream);
            if (e != hipSuccess) return fail(c, -3, std::string("pack_convert_kernel: ") + hipGetErrorString(e));
        }
        HIPCHK(c, hipEventRecord(v.ev1, v.stream));
        HIPCHK(c, hipMemcpyAsync(out + kPackHeaderBytes, v.vdi.cnt, (size_t)lay.px, hipMemcpyDeviceToHost, v.stream));
        if (h.E > 0) {
            HIPCHK(c, hipMemcpyAsync(out + lay.depth_off, v.vdi.dep, lay.depth_bytes, hipMemcpyDeviceToHost, v.stream));
            HIPCHK(c, hipMemcpyAsync(out + lay.colour_off, half ? (const void*)v.pk_stage.get() : (const void*)v.vdi.col,
                                     lay.colour_bytes, hipMemcpyDeviceToHost, v.stream));
        }
        HIPCHK(c, hipStreamSynchronize(v.stream));
        pack_write_header(out, h);
        std::memset(out + kPackHeaderBytes + (size_t)lay.px, 0, lay.depth_off - kPackHeaderBytes - (size_t)lay.px);
        float ms = 0.0f;
        v.ms_pack = (half && h.E > 0 && hipEventElapsedTime(&ms, v.ev0, v.ev1) == hipSuccess) ? ms_count + ms : ms_count;
        return 0;
    }
    size_t colour_at = 0;
    if (int rc = pack_stage_reserve(c, lay, &colour_at)) return rc;
    PackParams p{};
    p.vdi = v.vdi;
    p.boff = v.pk_boff;
    p.dep = reinterpret_cast<float2*>(v.pk_stage.get());
    p.col = v.pk_stage + colour_at;
    p.half = format == INSITU_PACK_HALF ? 1 : 0;
    HIPCHK(c, hipEventRecord(v.ev0, v.stream));
    hipError_t e = launch_vdi_pack(p, v.stream);
    if (e != hipSuccess) return fail(c, -3, std::string("vdi_pack_kernel: ") + hipGetErrorString(e));
    HIPCHK(c, hipEventRecord(v.ev1, v.stream));
    unsigned char* out = static_cast<unsigned char*>(host_out);
    HIPCHK(c, hipMemcpyAsync(out + kPackHeaderBytes, v.vdi.cnt, (size_t)lay.px, hipMemcpyDeviceToHost, v.stream));
    if (h.E > 0) {
        HIPCHK(c, hipMemcpyAsync(out + lay.depth_off, v.pk_stage, lay.depth_bytes, hipMemcpyDeviceToHost, v.stream));
        HIPCHK(c, hipMemcpyAsync(out + lay.colour_off, v.pk_stage + colour_at, lay.colour_bytes, hipMemcpyDeviceToHost, v.stream));
    }
    HIPCHK(c, hipStreamSynchronize(v.stream));
    pack_write_header(out, h);
    std::memset(out + kPackHeaderBytes + (size_t)lay.px, 0, lay.depth_off - kPackHeaderBytes - (size_t)lay.px);
    float ms = 0.0f;
    if (hipEventElapsedTime(&ms, v.ev0, v.ev1) == hipSuccess) v.ms_pack = ms_count + ms;
    return 0;
}

int insitu_view_bind_packed(insitu_ctx* c, const void* data, size_t bytes) {
    if (!c) return fail(nullptr, -1, "insitu_view_bind_packed: null context");
    ViewState& v = c->view;
    v.bound = false;   // (a rejected stream leaves no VDI bound)
    v.counted = false;
    PackHeader h{};
    PackLayout lay{};
    if (const char* why = pack_parse(data, bytes, &h, &lay))
        return fail(c, -1, std::string("insitu_view_bind_packed: stream rejected: ") + why);
    HIPCHK(c, hipSetDevice(c->cfg.device));
    if (int rc = view_reserve(c, (int)h.W, (int)h.H, (int)h.S)) return rc;
    const unsigned char* in = static_cast<const unsigned char*>(data);
    if (v.vdi.loc) {
        // compact: the counts, validated by the offset passes as below before anything depends on them; then the
        // sections are the layout's arrays -- copied as they are, the HALF colours widened element by element
        HIPCHK(c, hipMemcpyAsync(v.vdi.cnt, in + kPackHeaderBytes, (size_t)lay.px, hipMemcpyHostToDevice, v.stream));
        PackTotals tot{};
        float ms_count = 0.0f;
        HIPCHK(c, hipEventRecord(v.ev0, v.stream));
        if (int rc = view_compact_offsets(c, 1, h.E, &tot, &ms_count, "insitu_view_bind_packed")) return rc;
        if (tot.bad) {
            if (tot.max_count > h.S)
                return fail(c, -1, "insitu_view_bind_packed: stream rejected: a count of " + std::to_string(tot.max_count) +
                                       " exceeds S = " + std::to_string(h.S));
            return fail(c, -1, "insitu_view_bind_packed: stream rejected: the counts add up to " + std::to_string(tot.E) +
                                   ", the header says " + std::to_string(h.E));
        }
        const bool half = h.format == kPackHalf;
        if (half && h.E > 0)
            if (int rc = v.pk_stage.reserve(c, lay.colour_bytes)) return rc;
        if (h.E > 0) {
            HIPCHK(c, hipMemcpyAsync(v.vdi.dep, in + lay.depth_off, lay.depth_bytes, hipMemcpyHostToDevice, v.stream));
            HIPCHK(c, hipMemcpyAsync(half ? (void*)v.pk_stage.get() : (void*)v.vdi.col, in + lay.colour_off, lay.colour_bytes,
                                     hipMemcpyHostToDevice, v.stream));
        }
        HIPCHK(c, hipEventRecord(v.ev0, v.stream));
        hipError_t e = half ? launch_pack_convert(v.pk_stage, v.vdi.col, h.E, 0, v.stream) : hipSuccess;
        if (e == hipSuccess) e = launch_view_tmax(v.vdi, v.stream);
        if (e != hipSuccess) return fail(c, -3, std::string("pack_convert_kernel: ") + hipGetErrorString(e));
        HIPCHK(c, hipEventRecord(v.ev1, v.stream));
        HIPCHK(c, hipStreamSynchronize(v.stream));
        float ms = 0.0f;
        if (hipEventElapsedTime(&ms, v.ev0, v.ev1) == hipSuccess) v.ms_pack = v.ms_bind = ms_count + ms;
        std::memcpy(v.pv_g, h.pv_g, sizeof v.pv_g);
        v.overlaps = 0;
        v.bound = true;
        return 0;
    }
    size_t colour_at = 0;
    if (int rc = pack_stage_reserve(c, lay, &colour_at)) return rc;
    // the counts go straight into the view layout; nothing reads them as counts until they have been checked
    HIPCHK(c, hipMemcpyAsync(v.vdi.cnt, in + kPackHeaderBytes, (size_t)lay.px, hipMemcpyHostToDevice, v.stream));
    if (h.E > 0) {
        HIPCHK(c, hipMemcpyAsync(v.pk_stage, in + lay.depth_off, lay.depth_bytes, hipMemcpyHostToDevice, v.stream));
        HIPCHK(c, hipMemcpyAsync(v.pk_stage + colour_at, in + lay.colour_off, lay.colour_bytes, hipMemcpyHostToDevice, v.stream));
    }
    // validated on the device before anything is scattered: every count <= S, and the counts add up to E
    PackTotals tot{};
    float ms_count = 0.0f;
    if (int rc = pack_offsets(c, 1, h.E, &tot, &ms_count, "insitu_view_bind_packed")) return rc;
    if (tot.bad) {
        if (tot.max_count > h.S)
            return fail(c, -1, "insitu_view_bind_packed: stream rejected: a count of " + std::to_string(tot.max_count) +
                                   " exceeds S = " + std::to_string(h.S));
        return fail(c, -1, "insitu_view_bind_packed: stream rejected: the counts add up to " + std::to_string(tot.E) +
                               ", the header says " + std::to_string(h.E));
    }
    PackParams p{};
    p.vdi = v.vdi;
    p.boff = v.pk_boff;
    p.dep = reinterpret_cast<float2*>(v.pk_stage.get());
    p.col = v.pk_stage + colour_at;
    p.half = h.format == kPackHalf ? 1 : 0;
    HIPCHK(c, hipEventRecord(v.ev0, v.stream));
    hipError_t e = launch_vdi_unpack(p, v.stream);
    if (e != hipSuccess) return fail(c, -3, std::string("vdi_unpack_kernel: ") + hipGetErrorString(e));
    HIPCHK(c, hipEventRecord(v.ev1, v.stream));
    HIPCHK(c, hipStreamSynchronize(v.stream));
    float ms = 0.0f;
    if (hipEventElapsedTime(&ms, v.ev0, v.ev1) == hipSuccess) v.ms_pack = v.ms_bind = ms_count + ms;
    std::memcpy(v.pv_g, h.pv_g, sizeof v.pv_g);
    v.overlaps = 0;
    v.pk_E = h.E;
    v.counted = true;
    v.bound = true;
    return 0;
}

int insitu_view_render(insitu_ctx* c, const insitu_camera* cam, int out_w, int out_h, void* host_out, size_t cap) {
    if (!c) return fail(nullptr, -1, "insitu_view_render: null context");
    if (!cam) return fail(c, -1, "insitu_view_render: null camera");
    ViewState& v = c->view;
    if (!v.bound) return fail(c, -1, "insitu_view_render: no VDI bound (insitu_view_bind first)");
    if (out_w <= 0 || out_h <= 0 || (long long)out_w * (long long)out_h > (1ll << 30))
        return fail(c, -1, "insitu_view_render: bad output size");
    const size_t px = (size_t)out_w * (size_t)out_h;
    if (host_out && cap < px * 4) return fail(c, -1, "insitu_view_render: output buffer too small");
    ViewParams p{};
    float iv[16], ip[16];
    if (cam->has_inverses) {
        std::memcpy(iv, cam->inv_view, sizeof iv);
        std::memcpy(ip, cam->inv_proj, sizeof ip);
    } else if (!mat4_inverse(cam->view, iv) || !mat4_inverse(cam->proj, ip)) {
        return fail(c, -1, "insitu_view_render: view or projection matrix is singular");
    }
    mat4_mul_f(iv, ip, p.ipv_n);
    std::memcpy(p.pv_g, v.pv_g, sizeof p.pv_g);
    HIPCHK(c, hipSetDevice(c->cfg.device));
    if (px > v.out_color.count() || px > v.out_image.count()) {
        v.out_w = v.out_h = 0;   // (nothing to read until this render is done)
        int rc = 0;
        if ((rc = v.out_color.reserve(c, px)) || (rc = v.out_image.reserve(c, px))) return rc;
    }
    p.vdi = v.vdi;
    p.out_w = out_w; p.out_h = out_h;
    p.skip = (int)v.skip;
    p.out_color = v.out_color;
    p.out_image = v.out_image;
    HIPCHK(c, hipEventRecord(v.ev0, v.stream));
    hipError_t e = launch_vdi_view(p, v.stream);
    if (e != hipSuccess) return fail(c, -3, std::string("vdi_view_kernel: ") + hipGetErrorString(e));
    HIPCHK(c, hipEventRecord(v.ev1, v.stream));
    if (host_out) HIPCHK(c, hipMemcpyAsync(host_out, v.out_image, px * 4, hipMemcpyDeviceToHost, v.stream));
    HIPCHK(c, hipStreamSynchronize(v.stream));
    v.out_w = out_w; v.out_h = out_h;
    float ms = 0.0f;
    if (hipEventElapsedTime(&ms, v.ev0, v.ev1) == hipSuccess) v.ms = ms;
    return 0;
}

int insitu_get_stats(insitu_ctx* c, insitu_stats* out) {
    if (!c || !out) return fail(c, -1, "insitu_get_stats: null argument");
    const CompletedFrame done = completed_frame(c);
    FrameSlot& f = done.f;
    HIPCHK(c, hipSetDevice(c->cfg.device));
    HIPCHK(c, hipStreamSynchronize(done.s));
    cache_observe(c, f);
    std::memset(out, 0, sizeof *out);
    // the time from event a to event b of the slot's frame, when both were recorded
    auto span = [&f](int a, int b, float* ms) {
        return f.ev_valid[a] && f.ev_valid[b] && hipEventElapsedTime(ms, f.ev[a], f.ev[b]) == hipSuccess;
    };
    const bool vdi_ranks = c->mode == INSITU_MODE_VDI && c->N > 1;
    float ms = 0.0f;
    float* stages[4] = {&out->ms_render, &out->ms_exchange, &out->ms_composite, &out->ms_gather};
    for (int i = EvRenderStart; i < EvGatherEnd; ++i)   // (the stage events are consecutive, FrameEvent)
        if (span(i, i + 1, &ms)) *stages[i] = ms;
    if (span(EvGatherEnd, EvImageOnHost, &ms)) out->ms_image_d2h = ms;
    out->cache_bytes = (long long)f.cache_chunks * 32;
    out->exchange_bytes = c->last_exchange_bytes;
    out->exchange_entries = c->last_exchange_entries;
    if (c->mode == INSITU_MODE_VDI && f.counters) {
        // the render's pinned copy when it has arrived: a synchronous copy out of device memory is a blit kernel,
        // and with a pipelined frame's persistent search holding every CU it waited ~2 ms for a slot (the 8-GPU
        // share's trace: the host's next frame call, and so the next first pass, came that much late)
        GenCounters gc{};
        if (f.h_ctr_valid) gc = *f.h_ctr;
        else HIPCHK(c, hipMemcpy(&gc, f.counters, sizeof gc, hipMemcpyDeviceToHost));
        out->rays_searched = (long long)gc.queue_count + (long long)gc.queue_short;
        out->rays_uncached = (long long)gc.march_rays + (long long)gc.cap_overflow;
        out->cache_demand_bytes = (long long)gc.cache_cursor * 32;
        out->search_regroups = (int)gc.regroups;
    }
    if (vdi_ranks && span(EvCountsIn, EvPayloadStart, &ms)) out->ms_exchange_sync = ms;
    if (vdi_ranks && span(EvCompactStart, EvCompactEnd, &ms)) {   // compaction: exchange
        out->ms_compact = ms;
        if (!f.pipelined) {   // (a pipelined frame packs after its render, in its exchange span)
            out->ms_render -= ms;
            out->ms_exchange += ms;
        }
    }
    if (f.pipelined && f.ev_valid[EvRenderEnd] && c->N > 1 && span(EvCompactStart, EvExchangeEnd, &ms))
        out->ms_exchange = ms;   // exchange from its compaction
    // latency: render start to the image on the host (or the gather's end)
    if (span(EvRenderStart, f.ev_valid[EvImageOnHost] ? EvImageOnHost : EvGatherEnd, &ms)) out->ms_latency = ms;
    out->pipelined = f.pipelined ? 1 : 0;
    // the last batch of re-ingests, once it is done (a pipelined loop does not wait for it)
    if (hipEventQuery(c->ev_ingest) == hipSuccess && hipEventElapsedTime(&ms, c->ev_ingest0, c->ev_ingest) == hipSuccess)
        out->ms_ingest = ms;
    (void)hipGetLastError();
    out->ms_view = c->view.ms;
    out->ms_pack = c->view.ms_pack;
    out->view_slots = c->view.bound ? c->view.vdi.S : 0;
    out->view_overlaps = c->view.bound ? c->view.overlaps : 0;
    out->ms_view_bind = c->view.ms_bind;
    if (c->view.bound) {
        ViewState& v = c->view;
        float ms_count = 0.0f;   // (a dense bind counts its entries when they are first asked for)
        if (int rc = pack_count_bound(c, &ms_count, "insitu_get_stats")) return rc;
        ViewLayoutSize sz{};
        const bool ok = v.vdi.loc ? view_compact_size(v.vdi.W, v.vdi.H, v.vdi.S, v.pk_E, &sz)
                                  : view_dense_size(v.vdi.W, v.vdi.H, v.vdi.S, &sz);
        out->view_entries = (long long)v.pk_E;
        out->view_bytes = ok ? (long long)sz.bytes : 0;
        out->view_compact = v.vdi.loc ? 1 : 0;
    }
    out->ms_sample = out->ms_render;
    float a = 0.0f, b = 0.0f;
    if (c->mode == INSITU_MODE_VDI && f.ev_valid[EvRenderEnd] && span(EvRenderStart, EvSampleEnd, &a) &&
        span(EvSampleEnd, EvRenderEnd, &b)) {
        out->ms_sample = a;
        out->ms_search = b - out->ms_compact;
    }
    return 0;
}

int insitu_pass_stats(insitu_ctx* c, double* mean_passes, long long* rays_hit) {
    if (!c || !mean_passes || !rays_hit) return fail(c, -1, "insitu_pass_stats: null argument");
    auto [f, st] = completed_frame(c);
    if (!f.passes || c->mode != INSITU_MODE_VDI) return fail(c, -1, "insitu_pass_stats: needs VDI mode + keep_passes");
    HIPCHK(c, hipSetDevice(c->cfg.device));
    HIPCHK(c, hipStreamSynchronize(st));
    std::vector<uint8_t> h((size_t)c->BV * (size_t)c->W * (size_t)c->H);
    HIPCHK(c, hipMemcpy(h.data(), f.passes, h.size(), hipMemcpyDeviceToHost));
    long long hit = 0, sum = 0;
    for (uint8_t v : h)
        if (v) { ++hit; sum += v; }
    *rays_hit = hit;
    *mean_passes = hit ? (double)sum / (double)hit : 0.0;
    return 0;
}

int insitu_distribute_vdis(insitu_ctx* c, const void* subVDIColor, const void* subVDIDepth, long long sizePerProcess,
                           int commSize, void* recvColor, void* recvDepth) {
    if (!c) return fail(nullptr, -1, "insitu_distribute_vdis: null context");
    if (!subVDIColor || !subVDIDepth) return fail(c, -1, "insitu_distribute_vdis: null sub-VDI buffer");
    if (commSize != c->N) return fail(c, -1, "insitu_distribute_vdis: commSize differs from the context's nranks");
    if (c->BV != 1) return fail(c, -1, "insitu_distribute_vdis: the host-buffer path carries one sub-VDI per rank");
    if (!c->camera_set) return fail(c, -1, "insitu_distribute_vdis: call insitu_set_camera (VDI metadata) first");
    HIPCHK(c, hipSetDevice(c->cfg.device));
    FrameSlot& f = *c->cur;   // (an unpipelined stage of its own: the public exchange and composite follow it)
    if (c->mode == INSITU_MODE_PLAIN) {
        // rgba8 (dim0, dim1) colour + encoded depth; blocks of rows*dim0 texels (DistributedVolumeRenderer.kt:577)
        if (sizePerProcess != (long long)c->plainBlock * 4)
            return fail(c, -1, "insitu_distribute_vdis: plain sizePerProcess must be H*W*4/commSize bytes");
        const size_t bytes = (size_t)c->N * c->plainBlock * 4;
        HIPCHK(c, hipMemcpyAsync(c->d_pcol_send, subVDIColor, bytes, hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipMemcpyAsync(c->d_pdep_send, subVDIDepth, bytes, hipMemcpyHostToDevice, c->stream));
        f.rendered = true;
        int rc = insitu_exchange(c);
        if (rc) return rc;
        for (int s = 0; s < c->N; ++s) {   // the received set, source-major (compositeVDIs' VDISetColour)
            const size_t blk = c->plainBlock;
            const uint32_t* sc = s == c->rank ? c->d_pcol_send + (size_t)c->rank * blk : c->d_pcol_recv + (size_t)s * blk;
            const uint32_t* sd = s == c->rank ? c->d_pdep_send + (size_t)c->rank * blk : c->d_pdep_recv + (size_t)s * blk;
            if (recvColor) HIPCHK(c, hipMemcpyAsync((uint32_t*)recvColor + (size_t)s * blk, sc, blk * 4, hipMemcpyDeviceToHost, c->stream));
            if (recvDepth) HIPCHK(c, hipMemcpyAsync((uint32_t*)recvDepth + (size_t)s * blk, sd, blk * 4, hipMemcpyDeviceToHost, c->stream));
        }
        rc = insitu_composite(c);
        if (rc) return rc;
        HIPCHK(c, hipStreamSynchronize(c->stream));
        return 0;
    }
    // VDI mode: colour (S,H,W) rgba32f + depth (2S,H,W) r32f, x slowest; block j = columns of strip j
    const size_t blkE = (size_t)c->strip_w * (size_t)c->H * (size_t)c->S;   // supersegments per block
    if (sizePerProcess != (long long)(blkE * 4))
        return fail(c, -1, "insitu_distribute_vdis: VDI sizePerProcess must be H*W*S*4/commSize floats");
    const size_t allE = blkE * (size_t)c->N;
    if (int rc = c->d_ref_col.reserve(c, 2 * allE)) return rc;   // (allocated by the first call)
    if (int rc = c->d_ref_dep.reserve(c, 2 * allE * 2)) return rc;
    if (int rc = c->d_ref_cnt.reserve(c, (size_t)c->N * c->stripPx)) return rc;
    float4* send_c = c->d_ref_col;
    float4* recv_c = c->d_ref_col + allE;
    float* send_d = c->d_ref_dep;
    float* recv_d = c->d_ref_dep + 2 * allE;
    HIPCHK(c, hipMemcpyAsync(send_c, subVDIColor, allE * sizeof(float4), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(send_d, subVDIDepth, allE * 2 * sizeof(float), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(recv_c + (size_t)c->rank * blkE, send_c + (size_t)c->rank * blkE, blkE * sizeof(float4),
                             hipMemcpyDeviceToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(recv_d + (size_t)c->rank * 2 * blkE, send_d + (size_t)c->rank * 2 * blkE,
                             blkE * 2 * sizeof(float), hipMemcpyDeviceToDevice, c->stream));
    if (c->N > 1 && c->group) {
        return fail(c, -1, "insitu_distribute_vdis: the host-buffer path needs RCCL ranks (not a local group)");
    } else if (c->N > 1) {   // MPI_Alltoall of InVis.cpp -> grouped RCCL send/recv of contiguous strip blocks
        NCCLCHK(c, ncclGroupStart());
        for (int p = 0; p < c->N; ++p) {
            if (p == c->rank) continue;
            NCCLCHK(c, ncclSend(send_c + (size_t)p * blkE, blkE * 4, ncclFloat32, p, c->comm, c->stream));
            NCCLCHK(c, ncclRecv(recv_c + (size_t)p * blkE, blkE * 4, ncclFloat32, p, c->comm, c->stream));
            NCCLCHK(c, ncclSend(send_d + (size_t)p * 2 * blkE, blkE * 2, ncclFloat32, p, c->comm, c->stream));
            NCCLCHK(c, ncclRecv(recv_d + (size_t)p * 2 * blkE, blkE * 2, ncclFloat32, p, c->comm, c->stream));
        }
        NCCLCHK(c, ncclGroupEnd());
    }
    if (recvColor) HIPCHK(c, hipMemcpyAsync(recvColor, recv_c, allE * sizeof(float4), hipMemcpyDeviceToHost, c->stream));
    if (recvDepth) HIPCHK(c, hipMemcpyAsync(recvDepth, recv_d, allE * 2 * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    // uploadForCompositing (DistributedVolumes.kt:945-998): the received set feeds the compositor
    for (int s = 0; s < c->N; ++s) {
        const size_t slot = s == c->rank ? (size_t)c->rank * c->blockE : (size_t)s * c->blockE;
        float4* dc = (s == c->rank ? f.vcol_send : c->d_vcol_recv) + slot;
        float2* dd = (s == c->rank ? f.vdep_send : c->d_vdep_recv) + slot;
        HIPCHK(c, launch_vdi_from_reference(recv_c + (size_t)s * blkE, recv_d + (size_t)s * 2 * blkE, c->H, c->S,
                                            c->strip_w, c->strip_tiles, dc, dd, c->d_ref_cnt + (size_t)s * c->stripPx,
                                            c->stream));
    }
    f.rendered = true;
    f.exchanged = true;
    c->lists_from_reference = true;
    int rc = insitu_composite(c);
    if (rc) return rc;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return 0;
}

int insitu_gather_composited_vdi_set(insitu_ctx* c, long long compositedVDILen, int root, int myRank, int commSize,
                                     void* gatherColor, void* gatherDepth) {
    if (!c) return fail(nullptr, -1, "insitu_gather_composited_vdi_set: null context");
    if (!c->composite_vdi) return fail(c, -1, "insitu_gather_composited_vdi_set: context has composite_vdi == 0");
    if (root != 0) return fail(c, -1, "insitu_gather_composited_vdi_set: root must be 0");
    if (myRank != c->rank || commSize != c->N)
        return fail(c, -1, "insitu_gather_composited_vdi_set: rank/commSize differ from the context");
    if (compositedVDILen != (long long)(c->stripPx * (size_t)c->S_out * 4))
        return fail(c, -1, "insitu_gather_composited_vdi_set: compositedVDILen must be H*W*S_out*4/commSize floats");
    int rc = insitu_gather(c, nullptr, 0);
    if (rc) return rc;
    if (is_root(c)) {
        const size_t cb = insitu_buffer_bytes(c, INSITU_BUF_GATHERED_COLOR);
        if (gatherColor && (rc = insitu_read(c, INSITU_BUF_GATHERED_COLOR, 0, gatherColor, cb))) return rc;
        if (gatherDepth && (rc = insitu_read(c, INSITU_BUF_GATHERED_DEPTH, 0, gatherDepth, cb / 2))) return rc;
    }
    return 0;
}

int insitu_gather_composited_vdis(insitu_ctx* c, int root, long long subVDILen, int myRank, int commSize,
                                  void* gatherOut, size_t cap) {
    if (!c) return fail(nullptr, -1, "insitu_gather_composited_vdis: null context");
    if (root != 0) return fail(c, -1, "insitu_gather_composited_vdis: root must be 0");
    if (myRank != c->rank || commSize != c->N)
        return fail(c, -1, "insitu_gather_composited_vdis: rank/commSize differ from the context");
    if (subVDILen != (long long)c->stripPx * 4)
        return fail(c, -1, "insitu_gather_composited_vdis: subVDILen must be the rgba8 strip size H*W*4/commSize");
    return insitu_gather(c, gatherOut, cap);
}

}  // extern "C"
