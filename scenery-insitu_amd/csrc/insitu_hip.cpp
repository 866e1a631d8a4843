// insitu_hip.cpp -- host side of libinsitu_hip.so: the C ABI declared in include/insitu_hip.h.
//
// Owns the per-rank device state of the in-situ frame (bricks, transfer function, sub-VDI
// send/receive blocks, octree counters, composited strip, gathered image; the types: insitu_host.h) and orders
// the four stages of a frame (unpipelined: on one HIP stream; insitu_frame_pipelined: over the sampling, search and
// completion streams):
//   render    -> VDIGenerator.comp+AccumulateVDI.comp / VolumeRaycaster.comp+AccumulatePlainImage.comp
//   exchange  -> distributeVDIs' MPI_Alltoall (DistributedVolumes.kt:860), here RCCL send/recv
//                of contiguous screen-strip blocks over xGMI
//   composite -> PlainImageCompositor.comp / VDI flatten (VDIGenerator.comp:147-185)
//   gather    -> gatherCompositedVDIs' MPI_Gather (DistributedVolumes.kt:903), RCCL to rank 0
// The novel-view subsystem (insitu_view_*) is insitu_view.cpp: its own stream, buffers and blocking calls.  This
// file only frees its state (release), sets its options, reads its output buffers and asks it for its statistics.
#include "insitu_host.h"

#include <cmath>
#include <cstdio>
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#pragma clang fp contract(off)

namespace {

thread_local std::string g_create_error;

size_t dtype_size(int dt) { return dt == INSITU_U8 ? 1 : (dt == INSITU_U16 ? 2 : 4); }

}  // namespace

int fail(insitu_ctx* c, int code, const std::string& msg) {
    if (c) c->err = msg;
    else g_create_error = msg;
    return code;
}

bool is_root(const insitu_ctx* c) { return c->rank == 0; }

CompletedFrame completed_frame(const insitu_ctx* c) { return {*c->cur, c->pipe_inflight ? c->pipe_comp : c->stream}; }

namespace {

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
    for (hipEvent_t e : {c->view.ev0, c->view.ev1, c->view.offer.ev, c->ev_ingest, c->ev_ingest0, c->ev_gate})
        if (e) (void)hipEventDestroy(e);
    for (hipStream_t st : {c->view.stream, c->pipe_sample, c->pipe_comp})
        if (st) (void)hipStreamDestroy(st);
    if (c->comm) ncclCommDestroy(c->comm);
    if (c->group && c->rank < (int)c->group->ranks.size() && c->group->ranks[c->rank] == c) c->group->ranks[c->rank] = nullptr;
    if (c->own_stream && c->stream) (void)hipStreamDestroy(c->stream);
}

// the other frame slot becomes the current one
void swap_slot(insitu_ctx* c) { std::swap(c->cur, c->alt); }

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

}  // namespace

int check_fault(insitu_ctx* c, FrameSlot& f) {
    cache_observe(c, f);   // (a pending copy of the frame's counters reached h_ctr: we are after a synchronisation)
    if (!f.counters || !f.search_launched) return 0;
    uint32_t fault = 0;
    if (f.h_ctr_valid) fault = f.h_ctr->fault;
    else if (hipMemcpy(&fault, &f.counters->fault, sizeof fault, hipMemcpyDeviceToHost) != hipSuccess) fault = 1;
    if (fault) return fail(c, -6, "VDI search kernel exceeded its loop bound (internal error)");
    return 0;
}

namespace {

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
// counts and supersegment records, generator counters, and -- with a sample cache of `chunks` 32-byte units -- the
// cache, the search queue, the pinned counter copy and the tile-order keys; plus the slot's events
int alloc_slot(insitu_ctx* c, FrameSlot& f, size_t chunks) {
    int rc = 0;
    if ((rc = create_slot_events(c, f))) return rc;
    const size_t sendE = (size_t)c->N * (size_t)c->BV * c->blockE;
    const size_t px = (size_t)c->BV * (size_t)c->W * (size_t)c->H;
    if ((rc = f.vcol_send.alloc(c, sendE)) || (rc = f.vdep_send.alloc(c, sendE))) return rc;
    const size_t oct = (size_t)c->BV * (size_t)c->S * (size_t)c->ncx * (size_t)c->ncy;
    if ((rc = f.octree.alloc(c, oct ? oct : 1))) return rc;
    if ((rc = f.seg_pending.alloc(c, px)) || (rc = f.seg_rec.alloc(c, sendE))) return rc;
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
        p.seg_rec = f.seg_rec;
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
    if (int rc = view_stats(c, out)) return rc;
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
