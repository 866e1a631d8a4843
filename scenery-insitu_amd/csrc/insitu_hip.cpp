// insitu_hip.cpp -- the frame of libinsitu_hip.so: the stage calls of the C ABI declared in include/insitu_hip.h.
//
// Orders the four stages of a frame over the per-rank device state (bricks, transfer function, sub-VDI
// send/receive blocks, octree counters, composited strips, gathered image; the types: insitu_host.h)
// (unpipelined: on one HIP stream; insitu_frame_pipelined: over the sampling, search and completion streams):
//   render    -> VDIGenerator.comp+AccumulateVDI.comp / VolumeRaycaster.comp+AccumulatePlainImage.comp
//   exchange  -> distributeVDIs' MPI_Alltoall (DistributedVolumes.kt:860), here RCCL send/recv
//                of contiguous screen-strip blocks over xGMI
//   composite -> PlainImageCompositor.comp / VDI flatten (VDIGenerator.comp:147-185)
//   gather    -> gatherCompositedVDIs' MPI_Gather (DistributedVolumes.kt:903), RCCL to rank 0
// and owns the camera, the pipelined frame loop and the host-buffer entry points (insitu_distribute_vdis,
// insitu_gather_composited_vdi*).  The context's set-up, options and inputs are insitu_context.cpp, the readbacks
// and statistics insitu_read.cpp, the novel-view subsystem (insitu_view_*) insitu_view.cpp.
#include "insitu_host.h"

#include <cstdio>

#pragma clang fp contract(off)

// what the other host files call too (insitu_host.h says what each does)
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

int check_fault(insitu_ctx* c, FrameSlot& f) {
    cache_observe(c, f);   // (a pending copy of the frame's counters reached h_ctr: we are after a synchronisation)
    if (!f.counters || !f.search_launched) return 0;
    uint32_t fault = 0;
    if (f.h_ctr_valid) fault = f.h_ctr->fault;
    else if (hipMemcpy(&fault, &f.counters->fault, sizeof fault, hipMemcpyDeviceToHost) != hipSuccess) fault = 1;
    if (fault) return fail(c, -6, "VDI search kernel exceeded its loop bound (internal error)");
    return 0;
}

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
        L.cnt16 = f.seg_pending + (size_t)b * c->framePx;
        L.cnt_pitch = c->W;
        L.cnt_x0 = c->rank * c->strip_w;
    } else {                         // the compact message source s sent
        const size_t tiles = c->stripTiles;
        L.col = c->d_vcol_recv + (size_t)s * c->regionE;
        L.dep = c->d_vdep_recv + (size_t)s * c->regionE;
        const uint8_t* meta = c->d_meta_recv + (size_t)s * c->meta_bytes;
        L.cnt8 = meta + (size_t)b * tiles * 64;
        L.toff = reinterpret_cast<const uint32_t*>(meta + (size_t)c->BV * tiles * 64) + (size_t)b * tiles;
    }
    return L;
}

namespace {

// (re)allocate slot f's sample cache to `chunks` 32-byte units; on failure nothing is left allocated and the
// error is returned
hipError_t cache_realloc(FrameSlot& f, size_t chunks) {
    f.cache_chunks = 0;
    const hipError_t e = f.cache.try_alloc(chunks * 8);
    if (e == hipSuccess) f.cache_chunks = (uint32_t)chunks;
    return e;
}

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
    cp.pend_stride = c->framePx;
    cp.W = c->W; cp.H = c->H; cp.S = c->S; cp.B = c->BV; cp.nstrips = c->N; cp.strip_w = c->strip_w;
    cp.strip_tiles = c->strip_tiles; cp.ytiles = c->ytiles; cp.skip_d = c->rank;
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

BrickDesc brick_desc(const insitu_ctx* c, const Brick& b) {
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

// slot f's sample cache grows to what cache_observe asked for (the last frame of this slot's rays did not all
// fit).  Every stream that may still read the old cache is synchronised before it is reallocated.
int grow_cache(insitu_ctx* c, FrameSlot& f, hipStream_t ss, hipStream_t sr) {
    if (f.cache_grow_to <= f.cache_chunks) return 0;
    const size_t grow = f.cache_grow_to, old = f.cache_chunks;
    f.cache_grow_to = 0;   // (cleared first: a failure below is not retried every frame)
    for (hipStream_t s : {c->stream, ss, sr}) HIPCHK(c, hipStreamSynchronize(s));
    if (cache_realloc(f, grow) != hipSuccess) {
        // keep what fits (the rest re-samples): half the request, never less than the cache
        // that worked, and at most that from now on
        const size_t keep = std::max(old, grow / 2);
        if (cache_realloc(f, keep) != hipSuccess) HIPCHK(c, cache_realloc(f, old));
        c->cache_max_chunks = f.cache_chunks;
    }
    return 0;
}

// what the generator's kernels take for a VDI render of camera `cam` into slot f under `plan`: everything but
// the debug buffer (render_frame).  Queries the search grid's resident lanes when the LUT sizes have changed.
int vdi_gen_params(insitu_ctx* c, FrameSlot& f, const FrameCamera& cam, const RenderPlan& plan, VdiGenParams& p) {
    for (int b = 0; b < c->B; ++b) p.bricks[b] = brick_desc(c, c->bricks[b]);
    p.xfer = TransferDesc{c->d_tf, c->n_tf, c->d_cmap, c->n_cm, c->cmag};
    std::memcpy(p.ipv, f.ipv, sizeof p.ipv);
    std::memcpy(p.pv, f.pv, sizeof p.pv);
    std::memcpy(p.view, f.view, sizeof p.view);
    p.nw = cam.nw;
    p.tmax = cam.tmax;
    p.W = c->W; p.H = c->H; p.S = c->S;
    p.strip_w = c->strip_w; p.strip_tiles = c->strip_tiles; p.nstrips = c->N; p.B = c->BV;
    p.nvolumes = c->BV != c->B ? c->B : 0;
    p.ytiles = c->ytiles;
    p.color = f.vcol_send;
    p.depth = f.vdep_send;
    p.octree = f.octree;
    p.octree_stride = c->octreeN / (size_t)c->BV;
    p.passes = f.passes;
    p.passes_stride = c->framePx;
    p.seg_pending = f.seg_pending;
    p.seg_rec = f.seg_rec;
    p.ncx = c->ncx; p.ncy = c->ncy;
    p.interval_size = (20.0f - 0.1f) / (float)c->S;   // VDIGenerator.comp:241-247
    p.cache = f.cache;
    p.split_event = f.ev[EvSampleEnd];
    p.cache_chunks = f.cache_chunks;
    p.ctr = f.counters;
    p.queue = f.queue;
    p.queue_cap = (uint32_t)((size_t)c->BV * c->framePx);
    // longest-first, coarsely: rays with many samples (most work per pass, and the ones with
    // 20+ passes) are searched before the rest, so the frame does not end waiting for a long
    // ray popped late; within each class the queue keeps the sampling kernel's tile order
    p.long_samples = (uint32_t)c->tune.long_samples;
    p.round_batch = (int)c->tune.round_batch;   // (group mode ends rounds at once)
    p.search_blocks = c->search_blocks;
    if (plan.pipelined && c->tune.pipe_search_rays > 0) {
        // the search beside the next frame's first pass: one to two blocks per CU by the queue length, the
        // rest of each CU's wave slots left to that first pass
        p.search_blocks = std::min(c->search_blocks, 2 * c->num_cus);
        p.search_block_rays = (int)c->tune.pipe_search_rays;
        p.search_min_blocks = std::min(p.search_blocks, c->num_cus);
    }
    p.search_oversub = (int)(plan.pipelined ? c->tune.pipe_oversub : c->tune.search_oversub);
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
    if (plan.pipelined && f.cache && c->pipe_flag && c->pipe_trigger == 1) {
        p.pipe_flag = c->pipe_flag + f.flag_index;   // this search's queue drain starts the next first pass
        p.pipe_seq = f.flag_value + 1;
    }
    // counters zeroed, tile keys (and, on a default cache's first frame, the frame's cache demand) sorted
    p.measure_cache = (c->cache_adaptive && !f.cache_sized && p.nvolumes == 0) ? 1 : 0;
    return 0;
}

// the first frame of a default-sized cache: wait for the demand the tile keys measured (the prepare, on ss) and
// size the cache to it (later frames grow it from their own demand, cache_observe)
int size_cache_to_first_frame(insitu_ctx* c, FrameSlot& f, hipStream_t ss) {
    unsigned long long need = 0;
    HIPCHK(c, hipMemcpyAsync(&need, &f.counters->cache_need, sizeof need, hipMemcpyDeviceToHost, ss));
    HIPCHK(c, hipStreamSynchronize(ss));
    f.cache_sized = true;
    const size_t want = std::min((size_t)(need + need / 4 + 64), c->cache_max_chunks);
    if (want > f.cache_chunks) HIPCHK(c, cache_realloc(f, want));
    return 0;
}

// the render of a checked camera (render_check) into slot f: the enqueue sequence, the first pass on ss and the
// search and what follows it on sr
int render_frame(insitu_ctx* c, FrameSlot& f, const FrameCamera& cam, const RenderPlan& plan) {
    set_slot_camera(c, f, cam);
    const hipStream_t ss = plan.first, sr = plan.search;
    const bool pipelined = plan.pipelined;
    HIPCHK(c, wait_peer_reads(c, ss));
    c->ingest_batch = false;
    f.pipelined = pipelined;
    if (!pipelined) record(f, EvRenderStart, ss);   // (pipelined: at the gate, below)
    if (c->mode == INSITU_MODE_VDI) {
        // GridCellsToZero.comp
        if (c->octreeN) HIPCHK(c, hipMemsetAsync(f.octree, 0, c->octreeN * sizeof(uint32_t), ss));
        if (int rc = grow_cache(c, f, ss, sr)) return rc;
        VdiGenParams p{};
        if (int rc = vdi_gen_params(c, f, cam, plan, p)) return rc;
        f.ev_valid[EvSampleEnd] = true;   // (p.split_event: the first pass records it)
        HIPCHK(c, launch_vdi_prepare(p, ss));
        p.prepared = 1;
        if (p.measure_cache && f.cache && p.tile_ids) {
            if (int rc = size_cache_to_first_frame(c, f, ss)) return rc;
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
        p.xfer = TransferDesc{c->d_tf, c->n_tf, c->d_cmap, c->n_cm, c->cmag};
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
        const size_t region = c->regionE;
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

// the composite of slot f's frame into this rank's strip, on stream st
int composite_frame(insitu_ctx* c, FrameSlot& f, hipStream_t st) {
    if (!f.rendered) return fail(c, -1, "insitu_composite: nothing rendered");
    // with N > 1 the peers' lists arrive in insitu_exchange: without it the compact-message offsets
    // of the receive buffers are not this frame's (or never written)
    if (c->N > 1 && !f.exchanged) return fail(c, -1, "insitu_composite: call insitu_exchange first (nranks > 1)");
    HIPCHK(c, wait_peer_reads(c, st));   // (local group: the root's gather of the last strip)
    if (c->mode == INSITU_MODE_VDI && c->composite_vdi) {
        CompositeParams p{};   // VDICompositor.comp (DistributedVolumes.kt:424-439)
        p.V = c->V; p.S = c->S; p.S_out = c->S_out; p.H = c->H; p.W = c->W;
        p.strip_w = c->strip_w; p.strip_tiles = c->strip_tiles; p.x_offset = c->rank * c->strip_w;
        std::memcpy(p.ipv, f.ipv, sizeof p.ipv);
        for (int v = 0; v < c->V; ++v) p.lists[v] = list_of(c, f, v);
        p.out_color = c->d_gvdi_col;   // (this rank's block of each: the first)
        p.out_depth = c->d_gvdi_dep;
        p.out_count = c->d_gvdi_cnt;
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
        p.out = c->d_gather;   // (this rank's strip: the first block)
        HIPCHK(c, launch_vdi_flatten(p, st));
    } else {
        PlainCompParams p{};
        p.V = c->V; p.dim0 = c->W; p.rows = c->rows;
        // PlainImageCompositor.comp:43 as written composites numProcesses = dim0 / rows lists (those past
        // the received ones read as empty): the first min(numProcesses, V)
        if (c->cfg.faithful & INSITU_FAITHFUL_PLAIN_NUM_PROCESSES) p.V = std::min(c->V, c->W / c->rows);
        for (int v = 0; v < c->V; ++v) {   // list v (source v / B, brick v % B) is block v: my own of the send buffers
            const bool own = v / c->B == c->rank;
            p.colors[v] = (own ? c->d_pcol_send : c->d_pcol_recv) + (size_t)v * c->plainBlock;
            p.depths[v] = (own ? c->d_pdep_send : c->d_pdep_recv) + (size_t)v * c->plainBlock;
        }
        p.out = c->d_gather;   // (this rank's strip: the first block)
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
                    HIPCHK(c, hipMemcpyAsync(c->d_gvdi_col + (size_t)p * c->cblockE, q->d_gvdi_col, c->cblockE * sizeof(float4),
                                             hipMemcpyDeviceToDevice, st));
                    HIPCHK(c, hipMemcpyAsync(c->d_gvdi_dep + (size_t)p * c->cblockE, q->d_gvdi_dep, c->cblockE * sizeof(float2),
                                             hipMemcpyDeviceToDevice, st));
                    HIPCHK(c, hipMemcpyAsync(c->d_gvdi_cnt + (size_t)p * c->stripPx, q->d_gvdi_cnt, c->stripPx * sizeof(uint16_t),
                                             hipMemcpyDeviceToDevice, st));
                } else {
                    HIPCHK(c, hipMemcpyAsync(c->d_gather + (size_t)p * c->stripPx, q->d_gather, c->stripPx * 4,
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
            NCCLCHK(c, ncclSend(c->d_gvdi_col, c->cblockE * 4, ncclFloat32, 0, c->comm, st));
            NCCLCHK(c, ncclSend(c->d_gvdi_dep, c->cblockE * 2, ncclFloat32, 0, c->comm, st));
            NCCLCHK(c, ncclSend(c->d_gvdi_cnt, c->stripPx * sizeof(uint16_t), ncclUint8, 0, c->comm, st));
        }
        NCCLCHK(c, ncclGroupEnd());
    } else if (c->N > 1) {
        NCCLCHK(c, ncclGroupStart());
        if (is_root(c)) {
            for (int p = 1; p < c->N; ++p)
                NCCLCHK(c, ncclRecv(c->d_gather + (size_t)p * c->stripPx, c->stripPx, ncclUint32, p, c->comm, st));
        } else {
            NCCLCHK(c, ncclSend(c->d_gather, c->stripPx, ncclUint32, 0, c->comm, st));
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
        c->gvdi_valid = true;   // what insitu_view_bind(INSITU_VIEW_GATHERED) takes, and its camera
        std::memcpy(c->gvdi_pv, f.pv, sizeof c->gvdi_pv);
    }
    if (is_root(c) && c->mode == INSITU_MODE_VDI)
        HIPCHK(c, launch_assemble_columns(c->d_gather, c->N, c->H, c->strip_w, c->d_image, st));
    if (c->group && is_root(c)) record(f, EvPeerReadsDone, st);
    record(f, EvGatherEnd, st);
    if (is_root(c) && host_out) {
        const size_t bytes = c->framePx * 4;
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

// what the four unpipelined stage calls open with: they work on the completed frame's slot and the context
// stream, and refuse while a pipelined frame is in flight.  fn: the public call, for the message.
int stage_guard(insitu_ctx* c, const char* fn) {
    if (!c) return fail(nullptr, -1, std::string(fn) + ": null context");
    if (c->pipe_inflight)
        return fail(c, -1, std::string(fn) + ": a pipelined frame is in flight (insitu_pipeline_flush first)");
    HIPCHK(c, hipSetDevice(c->cfg.device));
    return 0;
}

}  // namespace

extern "C" {

int insitu_set_camera(insitu_ctx* c, const insitu_camera* cam) {
    if (!c) return fail(nullptr, -1, "insitu_set_camera: null context");
    FrameCamera m;
    if (int rc = camera_matrices(c, cam, &m)) return rc;
    set_slot_camera(c, *c->cur, m);
    return 0;
}

int insitu_render(insitu_ctx* c, const insitu_camera* cam) {
    if (int rc = stage_guard(c, "insitu_render")) return rc;
    FrameCamera m;
    if (int rc = render_check(c, cam, &m)) return rc;
    RenderPlan plan;
    plan.first = plan.search = c->stream;
    return render_frame(c, *c->cur, m, plan);
}

int insitu_exchange(insitu_ctx* c) {
    if (int rc = stage_guard(c, "insitu_exchange")) return rc;
    return exchange_frame(c, *c->cur, c->stream);
}

int insitu_composite(insitu_ctx* c) {
    if (int rc = stage_guard(c, "insitu_composite")) return rc;
    return composite_frame(c, *c->cur, c->stream);
}

int insitu_gather(insitu_ctx* c, void* host_out, size_t cap) {
    if (int rc = stage_guard(c, "insitu_gather")) return rc;
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
    std::swap(c->cur, c->alt);
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
    std::swap(c->cur, c->alt);   // the frame in flight becomes the completed one
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
