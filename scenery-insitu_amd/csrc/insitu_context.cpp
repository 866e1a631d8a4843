// insitu_context.cpp -- the context of libinsitu_hip.so: everything that is set up once and fed between frames.
//
// Owns the create error and `fail`, the in-process rank group, insitu_create (in steps: config check, buffers by
// mode, transport, environment seeds) with insitu_destroy, the option table of insitu_set_option, the frame slots'
// allocation (alloc_slot, and pipeline_setup for the second slot and the pipeline's streams), and the inputs of a
// frame: insitu_set_brick and insitu_set_transfer.  The frame's stages are insitu_hip.cpp, its readbacks and
// statistics insitu_read.cpp.
#include "insitu_host.h"

#include <array>
#include <cstdlib>
#include <limits>

#pragma clang fp contract(off)

namespace {

thread_local std::string g_create_error;

size_t dtype_size(int dt) { return dt == INSITU_U8 ? 1 : (dt == INSITU_U16 ? 2 : 4); }

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
    const size_t px = (size_t)c->BV * c->framePx;
    if ((rc = f.vcol_send.alloc(c, c->sendE)) || (rc = f.vdep_send.alloc(c, c->sendE))) return rc;
    if ((rc = f.octree.alloc(c, c->octreeN ? c->octreeN : 1))) return rc;
    if ((rc = f.seg_pending.alloc(c, px)) || (rc = f.seg_rec.alloc(c, c->sendE))) return rc;
    // per-pixel supersegment counts: empty until the first render (the slots are not zero-filled)
    if (hipMemset(f.seg_pending, 0, sizeof(uint16_t) * px) != hipSuccess)
        return fail(c, -3, "hipMemset of the supersegment counts failed");
    if (c->cfg.keep_passes && (rc = f.passes.alloc(c, px))) return rc;
    // generator counters, zeroed here so the fault flag reads 0 before any render (the host-buffer path never renders)
    if ((rc = f.counters.alloc(c, 1))) return rc;
    if (hipMemset(f.counters, 0, sizeof(GenCounters)) != hipSuccess)
        return fail(c, -3, "hipMemset of the generator counters failed");
    if (chunks == 0) return 0;
    if ((rc = f.cache.alloc(c, chunks * 8)) || (rc = f.queue.alloc(c, (size_t)c->B * c->framePx))) return rc;
    if (f.h_ctr.try_alloc(1) != hipSuccess) return fail(c, -5, "hipHostMalloc of the generator counters failed");
    std::memset(f.h_ctr, 0, sizeof(GenCounters));
    f.cache_chunks = (uint32_t)chunks;
    // longest-tiles-first order of the sampling kernel: keys, ids and the sort's scratch (the key keeps 24
    // bits of tile position; super-tiles of up to 4x4 tiles pad the grid, so larger frames keep the order
    // only with super_tile 1: insitu_set_option checks that)
    const size_t ntile = (size_t)c->B * (size_t)c->N * c->stripTiles;
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
    return (size_t)c->B * (size_t)((c->ytiles + sup - 1) / sup * sup) *
           (size_t)((c->N * c->strip_tiles + sup - 1) / sup * sup);
}

// One row per option of insitu_set_option: its number, the INSITU_* variable that seeds it at create
// (tools/knob_sweep.sh), the range it accepts and where its value lives.  INSITU_OPT_SUPER_TILE takes the set
// {1, 2, 4} of its range and has a check of its own (insitu_set_option).
struct Option {
    int id;
    const char* env;
    long long lo, hi;
    long long* value;
};

std::array<Option, 14> options(insitu_ctx* c) {
    Tuning& t = c->tune;
    return {{{INSITU_OPT_EXACT_SEARCH, "INSITU_EXACT_SEARCH", 0, 1, &t.exact_search},
             {INSITU_OPT_SEARCH_DEPTH, "INSITU_SEARCH_DEPTH", 0, 6, &t.search_depth},
             {INSITU_OPT_LONG_SAMPLES, "INSITU_LONG_SAMPLES", 0, 0xffffffffll, &t.long_samples},
             {INSITU_OPT_ROUND_BATCH, "INSITU_ROUND_BATCH", 1, 64, &t.round_batch},
             {INSITU_OPT_SEARCH_OVERSUB, "INSITU_SEARCH_OVERSUB", 1, 64, &t.search_oversub},
             {INSITU_OPT_TILE_ORDER, "INSITU_TILE_ORDER", 0, 1, &t.tile_order},
             {INSITU_OPT_SUPER_TILE, "INSITU_SUPER_TILE", 1, 4, &t.super_tile},
             {INSITU_OPT_REGROUP, "INSITU_REGROUP", 0, 1, &t.regroup},
             {INSITU_OPT_EXACT_TILE_KEYS, "INSITU_EXACT_TILE_KEYS", 0, 1, &t.exact_tile_keys},
             {INSITU_OPT_PIPE_TRIGGER, "INSITU_PIPE_TRIGGER", 0, 2, &c->pipe_trigger},
             {INSITU_OPT_PIPE_OVERSUB, "INSITU_PIPE_OVERSUB", 1, 64, &t.pipe_oversub},
             {INSITU_OPT_PIPE_SEARCH_RAYS, "INSITU_PIPE_SEARCH_RAYS", 0, 1ll << 24, &t.pipe_search_rays},
             {INSITU_OPT_VIEW_SKIP, "INSITU_VIEW_SKIP", 0, 1, &c->view.skip},
             // (the next bind's layout; the bound VDI keeps its own)
             {INSITU_OPT_VIEW_COMPACT, "INSITU_VIEW_COMPACT", 0, 1, &c->view.compact_next}}};
}

// insitu_create, step by step.  The config alone: nothing is created before it passes; every later step reports
// through fail() on the half-built context
int check_config(const insitu_config& k) {
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
    return 0;
}

// VDI mode: the strip geometry and the sizes derived from it, the exchange buffers (N > 1), the first frame slot
// with its sample cache, and the root's image.  hbm_free: the device memory free at create.
int create_vdi_buffers(insitu_ctx* c, size_t hbm_free) {
    const insitu_config& k = c->cfg;
    int rc = 0;
    c->strip_w = c->W / c->N;
    c->strip_tiles = (c->strip_w + 7) / 8;
    c->blockE = (size_t)c->strip_tiles * (size_t)c->S * (size_t)c->H * 8;
    c->stripPx = (size_t)c->H * (size_t)c->strip_w;
    c->ncx = c->W / 8; c->ncy = c->H / 8;
    c->stripTiles = (size_t)c->strip_tiles * (size_t)c->ytiles;
    c->regionE = (size_t)c->BV * c->blockE;
    c->sendE = (size_t)c->N * c->regionE;
    c->octreeN = (size_t)c->BV * (size_t)c->S * (size_t)c->ncx * (size_t)c->ncy;
    if (c->N > 1) {
        // compact exchange: send regions per destination, receive regions per source, meta blocks
        c->meta_bytes = compact_meta_bytes(c->BV, c->strip_tiles, c->ytiles);
        if ((rc = c->d_vcol_recv.alloc(c, c->sendE)) || (rc = c->d_vdep_recv.alloc(c, c->sendE)) ||
            (rc = c->d_ccol_send.alloc(c, c->sendE)) || (rc = c->d_cdep_send.alloc(c, c->sendE)) ||
            (rc = c->d_meta_send.alloc(c, (size_t)c->N * c->meta_bytes)) ||
            (rc = c->d_meta_recv.alloc(c, (size_t)c->N * c->meta_bytes)) ||
            (rc = c->d_cursor.alloc(c, 2 * (size_t)c->N)))
            return rc;
        // received counts/offsets read as empty lists until the first exchange fills them
        if (hipMemset(c->d_meta_recv, 0, (size_t)c->N * c->meta_bytes) != hipSuccess)
            return fail(c, -3, "hipMemset of the exchange meta blocks failed");
        if (c->h_tot.try_alloc(2 * (size_t)c->N) != hipSuccess)
            return fail(c, -5, "hipHostMalloc of the exchange totals failed");
    }
    size_t chunks = 0;
    bool start_knob = false;
    if (k.sample_cache_mb >= 0) {
        // default: 512 B (64 samples of 8 B) per pixel per brick to start with (config 2 asks for 4.1 GB = 250 B per
        // pixel per brick), grown after a frame whose rays did not fit to 1.25x that frame's demand, up to 45 % of
        // the HBM free at create (this is an in-situ library: the simulation shares the GPU, so the cache takes
        // what the frames need, not what is free).  Rays that do not fit are searched by re-sampling (same
        // results, slower) and counted (insitu_stats.rays_uncached).  sample_cache_mb > 0 fixes it.
        c->cache_max_chunks = std::min(hbm_free / 20 * 9 / 32, (size_t)0xffffffffu);
        size_t bytes = (size_t)k.sample_cache_mb << 20;
        if (k.sample_cache_mb == 0) {
            bytes = std::min((size_t)c->B * c->framePx * 512, c->cache_max_chunks * 32);
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
    if ((rc = alloc_slot(c, c->slots[0], chunks))) return rc;
    if (chunks > 0 && start_knob) c->slots[0].cache_sized = true;
    if (const char* dbg = std::getenv("INSITU_DEBUG_RAYS")) {   // diagnostics (tools/ray_timing.py)
        if (c->slots[0].queue) {
            c->dbg_entries = (size_t)c->BV * c->framePx;
            if ((rc = c->d_dbg.alloc(c, c->dbg_entries * 4))) return rc;
            c->dbg_path = dbg;
        }
    }
    if (is_root(c) && (rc = c->d_image.alloc(c, c->framePx))) return rc;
    return 0;
}

// composite_vdi: the compositor's pass counts and merge cache, and the composited VDI strips (`blocks` of them)
int create_composited_vdi_buffers(insitu_ctx* c, size_t hbm_free, size_t blocks) {
    const insitu_config& k = c->cfg;
    int rc = 0;
    c->composite_vdi = true;
    c->S_out = k.max_output_supersegments > 0 ? k.max_output_supersegments : c->S;
    c->cblockE = (size_t)c->strip_tiles * (size_t)c->S_out * (size_t)c->H * 8;
    if ((rc = c->d_cpasses.alloc(c, c->stripPx))) return rc;
    // merge cache of the compositor: an eighth of the V*S entries per pixel to start with, grown to
    // a composite's demand when it did not fit (the waves that found no room merge every pass)
    // growth budget: 20 % of the HBM free at create (the simulation and the sample cache share the GPU)
    c->cseq_max = std::max<unsigned long long>(64ull * 64ull, (unsigned long long)(hbm_free / 5 / (16 * kCompEntryF4)));
    c->cseq_cap = std::min(c->cseq_max, std::max<unsigned long long>(
        64ull * 64ull, (unsigned long long)c->V * c->stripPx * (unsigned long long)c->S / 8));
    if ((rc = c->d_cseq.alloc(c, (size_t)kCompEntryF4 * (size_t)c->cseq_cap)) || (rc = c->d_cseq_cursor.alloc(c, 1)))
        return rc;
    if (c->h_cseq_demand.try_alloc(1) != hipSuccess)
        return fail(c, -5, "hipHostMalloc of the compositor demand failed");
    *c->h_cseq_demand = 0;
    if ((rc = c->d_gvdi_col.alloc(c, blocks * c->cblockE)) || (rc = c->d_gvdi_dep.alloc(c, blocks * c->cblockE)) ||
        (rc = c->d_gvdi_cnt.alloc(c, blocks * c->stripPx)))
        return rc;
    return 0;
}

// plain mode: the row-strip geometry, the slot's events and the fixed-size exchange blocks
int create_plain_buffers(insitu_ctx* c) {
    int rc = 0;
    if ((rc = create_slot_events(c, c->slots[0]))) return rc;
    c->rows = c->H / c->N;
    c->plainBlock = (size_t)c->rows * (size_t)c->W;
    c->stripPx = c->plainBlock;
    const size_t sendPx = (size_t)c->N * (size_t)c->B * c->plainBlock;
    if ((rc = c->d_pcol_send.alloc(c, sendPx)) || (rc = c->d_pdep_send.alloc(c, sendPx))) return rc;
    if (c->N > 1)
        if ((rc = c->d_pcol_recv.alloc(c, sendPx)) || (rc = c->d_pdep_recv.alloc(c, sendPx))) return rc;
    return 0;
}

// the ranks' transport: a slot of the in-process group, or an RCCL communicator (N > 1)
int create_transport(insitu_ctx* c, const insitu_config& k) {
    if (k.local_group) {
        c->group = k.local_group;
        c->group->ranks[c->rank] = c;
    } else if (c->N > 1) {
        ncclUniqueId id;
        std::memcpy(&id, k.comm_id, sizeof id);
        ncclResult_t r = ncclCommInitRank(&c->comm, c->N, id, c->rank);
        if (r != ncclSuccess) {
            c->comm = nullptr;
            return fail(c, -4, std::string("ncclCommInitRank: ") + ncclGetErrorString(r));
        }
    }
    return 0;
}

// tuning seeds from the environment; insitu_set_option overrides
int seed_options(insitu_ctx* c) {
    for (const Option& o : options(c))
        if (const char* v = std::getenv(o.env))
            if (insitu_set_option(c, o.id, std::atoll(v)) != 0)
                return fail(c, -1, std::string("insitu_create: ") + o.env + "=" + v + " out of range");
    return 0;
}

// everything of insitu_create that a half-built context can fail in (k: the caller's config, with its comm_id)
int create_steps(insitu_ctx* c, const insitu_config& k) {
    int rc = 0;
    if (k.stream) {
        c->stream = (hipStream_t)k.stream;
    } else {
        if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess)
            return fail(c, -3, "hipStreamCreate failed");
        c->own_stream = true;
    }
    if (hipEventCreate(&c->ev_ingest0) != hipSuccess || hipEventCreate(&c->ev_ingest) != hipSuccess ||
        hipEventCreate(&c->ev_gate) != hipSuccess)
        return fail(c, -3, "hipEventCreate failed");
    // the composited strips: every rank's on the root, this rank's own elsewhere
    const size_t blocks = is_root(c) ? (size_t)c->N : 1;
    if (c->mode == INSITU_MODE_VDI) {
        // the budgets of the sample cache and of the compositor's merge cache are shares of this
        size_t hbm_free = 0, hbm_total = 0;
        if (hipMemGetInfo(&hbm_free, &hbm_total) != hipSuccess) hbm_free = (size_t)32 << 30;
        if ((rc = create_vdi_buffers(c, hbm_free))) return rc;
        if (k.composite_vdi && (rc = create_composited_vdi_buffers(c, hbm_free, blocks))) return rc;
    } else if ((rc = create_plain_buffers(c))) {
        return rc;
    }
    if ((rc = c->d_gather.alloc(c, blocks * c->stripPx))) return rc;
    if ((rc = create_transport(c, k))) return rc;
    return seed_options(c);
}

}  // namespace

int fail(insitu_ctx* c, int code, const std::string& msg) {
    if (c) c->err = msg;
    else g_create_error = msg;
    return code;
}

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
    if (int rc = check_config(k)) return rc;

    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev == 0) return fail(nullptr, -2, "insitu_create: no HIP device available");
    if (k.device < 0 || k.device >= ndev) return fail(nullptr, -2, "insitu_create: device index out of range");
    e = hipSetDevice(k.device);
    if (e != hipSuccess) return fail(nullptr, -2, std::string("hipSetDevice: ") + hipGetErrorString(e));

    insitu_ctx* c = new insitu_ctx();
    c->cfg = k;
    int cus = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, k.device) == hipSuccess && cus > 0)
        c->num_cus = cus;
    c->cfg.comm_id = nullptr;
    c->W = k.width; c->H = k.height; c->N = k.nranks; c->rank = k.rank; c->B = k.bricks_per_rank;
    c->BV = (k.mode == INSITU_MODE_VDI && k.merge_bricks) ? 1 : c->B;
    c->V = c->N * c->BV; c->mode = k.mode;
    c->S = (k.mode == INSITU_MODE_VDI) ? k.max_supersegments : 1;
    c->ytiles = (k.height + 7) / 8;
    c->framePx = (size_t)k.width * (size_t)k.height;
    c->bricks.resize(c->B);
    if (int rc = create_steps(c, k)) {   // the one place a half-built context ends: its message is the create error
        g_create_error = c->err;
        release(c);
        delete c;
        return rc;
    }
    *out = c;
    return 0;
}

int insitu_set_option(insitu_ctx* c, int option, long long v) {
    if (!c) return fail(nullptr, -1, "insitu_set_option: null context");
    for (const Option& o : options(c)) {
        if (o.id != option) continue;
        const bool super_tile = option == INSITU_OPT_SUPER_TILE;
        if (v < o.lo || v > o.hi || (super_tile && v == 3))
            return fail(c, -1, "insitu_set_option: value " + std::to_string(v) + " out of range for option " +
                                   std::to_string(option));
        if (super_tile && v > 1 && c->mode == INSITU_MODE_VDI && padded_tiles(c, (int)v) >= ((size_t)1 << 24))
            return fail(c, -1, "insitu_set_option: super-tiles of " + std::to_string(v) +
                                   " tiles pad this frame's tile grid past the sort key's 24 bits of position");
        *o.value = v;
        return 0;
    }
    return fail(c, -1, "insitu_set_option: unknown option " + std::to_string(option));
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

}  // extern "C"
