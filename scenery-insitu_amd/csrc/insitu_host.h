// insitu_host.h -- private to the host side of libinsitu_hip.so: what insitu_context.cpp (the context's set-up and
// inputs), insitu_hip.cpp (the frame's stages), insitu_read.cpp (readbacks and statistics) and insitu_view.cpp (the
// novel-view subsystem) share -- the owners of device memory, the error helpers, the matrix helpers, the context
// with its frame slots and view state, and the few functions one of those files defines for another.
#pragma once

#include "insitu_hip.h"
#include "insitu_kernels.h"

#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <cmath>
#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

using namespace insitu;

// records msg as the context's error (no context: the calling thread's, read by insitu_last_error(NULL)); returns code
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

// float mat4 product with the same operation order as the shaders' `A * B` (and the oracle)
inline void mat4_mul_f(const float* a, const float* b, float* out) {
    float t[16];
    for (int c = 0; c < 4; ++c) {
        const float x = b[c * 4 + 0], y = b[c * 4 + 1], z = b[c * 4 + 2], w = b[c * 4 + 3];
        for (int r = 0; r < 4; ++r)
            t[c * 4 + r] = std::fmaf(a[12 + r], w, std::fmaf(a[8 + r], z, std::fmaf(a[4 + r], y, a[r] * x)));
    }
    std::memcpy(out, t, sizeof t);
}

// general 4x4 inverse in double, rounded to float (column-major in and out)
inline bool mat4_inverse(const float* m, float* out) {
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
    DevBuf<SegRecord> seg_rec;          // per sub-VDI entry: the stored supersegment of a deferred ray (32 bytes)
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
    ViewVdi vdi{};                      // ... as the kernels take them, with its dimensions (view_reserve_index, _entries)
    float pv_g[16] = {};                // proj * view of the generating camera
    bool bound = false;
    DevBuf<float4> out_color;           // (out_h, out_w) rgba32f / rgba8 of the last render (grown by a larger one)
    DevBuf<uint32_t> out_image;
    int out_w = 0, out_h = 0;           // of the last render (0: none yet)
    hipStream_t stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    float ms = 0.0f;                    // the last render's kernel
    long long skip = 1;                 // insitu_set_option: the view-skip option
    // the compact view layout: vdi.loc != null says the bound VDI has it
    long long compact_next = 0;         // insitu_set_option: the view layout the next bind takes
    DevBuf<uint16_t> loc;               // a pixel's entries before it in its block (vdi.boff is pk_boff)
    // the packed stream of the bound VDI (insitu_view_pack, insitu_view_bind_packed; vdi_pack.hip)
    bool counted = false;               // pk_boff and pk_E describe the bound VDI (once per bind; view_unbind clears it)
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
    // a set of packed streams (insitu_view_bind_packed_set), kept across calls and grown by a larger set
    DevBuf<unsigned char> ps_stage;     // every stream's counts, depth section and colour section, as they arrive
    DevBuf<unsigned char> ps_index;     // the PackedStream table, the streams' totals, and each stream's own boff, bstat, loc
    PinnedBuf<PackTotals> h_ps_totals;  // kMaxLists: the totals of all streams, read back in one copy
    // the gather of the ranks' bound VDIs on rank 0 (insitu_view_gather_merged)
    DevBuf<unsigned char> gm_ctl;       // headers (the root: one per rank) and the verdict record, as they travel
    PinnedBuf<unsigned char> h_gm_ctl;  // the same on the host: the only bytes of a gather the host reads
    // (local group) what a peer's call leaves for the root's: its header and where its sections lie on its device,
    // ready once `ev` (the view's stream, behind its pack) has completed.  The sections are the peer's own buffers:
    // a bind or a pack of the peer's before the root has pulled them withdraws the offer.
    struct GatherOffer {
        enum { None, Made, Withdrawn } state = None;
        unsigned char header[128] = {};
        const uint8_t* cnt = nullptr;
        const float2* dep = nullptr;
        const void* col = nullptr;
        hipEvent_t ev = nullptr;
    } offer;
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
    // sizes derived from the ones above, once, in insitu_create (VDI mode; plain mode: ytiles and framePx)
    int ytiles = 0;         // 8-row tiles per column of tiles
    size_t framePx = 0;     // pixels of the frame
    size_t stripTiles = 0;  // tiles of one strip
    size_t regionE = 0;     // VDI entries of one source's region: BV blocks
    size_t sendE = 0;       // VDI entries of a slot's send buffers: N regions
    size_t octreeN = 0;     // octree counters of a slot
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
    // the composited strips: N blocks [rank] on the root, one elsewhere.  This rank's own strip is the first block
    // on every rank (the root is rank 0), so every stage writes and reads it at offset 0; the gather fills the
    // root's other blocks
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
    DevBuf<float4> d_gvdi_col;          // the composited VDI strips, as d_gather: [rank][block] on the root, this
    DevBuf<float2> d_gvdi_dep;          // rank's block alone elsewhere
    bool gvdi_valid = false;            // root: a gather has filled them, from the frame of camera gvdi_pv
    float gvdi_pv[16] = {};
    DevBuf<uint16_t> d_gvdi_cnt;        // per pixel of those strips: slots written [rank][y][x_local]
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
    long long pipe_trigger = 2;         // 0: after the previous search; 1: at its queue drain; 2: none (default:
                                        // the search keeps only the blocks its queue needs)
    bool pipe_wait_value = true;        // hipStreamWaitValue64 works here (else mode 1 falls back to 0)
    ViewState view;
    std::string err;
};

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

inline bool is_root(const insitu_ctx* c) { return c->rank == 0; }

// the completed frame's slot and the stream its readbacks run on: with a pipelined frame in flight the completion
// stream (the context stream may be busy with work for the next frame, the completion stream holds nothing of it)
struct CompletedFrame {
    FrameSlot& f;
    hipStream_t s;
};
inline CompletedFrame completed_frame(const insitu_ctx* c) {
    return {*c->cur, c->pipe_inflight ? c->pipe_comp : c->stream};
}

// after a synchronisation of the stream of slot f's last render: did a persistent kernel of that render hit its
// wall-clock bound?
int check_fault(insitu_ctx* c, FrameSlot& f);

// after a synchronisation of the stream of slot f's last render: its cache demand (h_ctr) decides whether a
// default-sized cache grows before the slot's next render (insitu_hip.cpp)
void cache_observe(insitu_ctx* c, FrameSlot& f);

// list v (source s = v / B, brick b = v % B) of this rank's strip, as the compositors read it: this rank's own
// from slot f (insitu_hip.cpp)
VdiList list_of(const insitu_ctx* c, const FrameSlot& f, int v);

// the second frame slot, the sampling and completion streams and the trigger flag (first pipelined frame;
// insitu_context.cpp)
int pipeline_setup(insitu_ctx* c);

// the view fields of insitu_get_stats (insitu_view.cpp)
int view_stats(insitu_ctx* c, insitu_stats* out);
