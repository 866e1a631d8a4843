// insitu_read.cpp -- what the host reads of a completed frame: insitu_buffer_bytes, insitu_read and
// insitu_read_region (every reference-layout readback goes through read_reference), insitu_get_stats and
// insitu_pass_stats.  All of them work on the completed frame's slot and stream (completed_frame) and enqueue
// nothing a frame depends on.
#include "insitu_host.h"

namespace {

// One reference-layout readback: a scratch pair of n colour entries (rgba32f) and n depth entries (two r32f) is
// allocated, and for each of `blocks` blocks convert(i, colour, depth) -- which writes both, the one not asked for
// being a throwaway -- is enqueued on st, the half asked for copied to block i of host_out, and st synchronised.
// The pair is freed on return, after the last synchronisation.  fn: the public call, for the message.
template <typename Convert>
int read_reference(insitu_ctx* c, const char* fn, hipStream_t st, size_t n, bool colour, int blocks, void* host_out,
                   Convert convert) {
    DevBuf<float4> col;
    DevBuf<float> dep;
    if (col.try_alloc(n) != hipSuccess || dep.try_alloc(n * 2) != hipSuccess)
        return fail(c, -5, std::string(fn) + ": scratch allocation failed");
    const size_t bytes = colour ? n * sizeof(float4) : n * sizeof(float2);
    hipError_t e = hipSuccess;
    for (int i = 0; i < blocks && e == hipSuccess; ++i) {
        e = convert(i, col.get(), dep.get());
        if (e == hipSuccess)
            e = hipMemcpyAsync((uint8_t*)host_out + (size_t)i * bytes, colour ? (void*)col : (void*)dep, bytes,
                               hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);
    }
    if (e != hipSuccess) return fail(c, -3, std::string(fn) + ": " + hipGetErrorString(e));
    return 0;
}

// a VDI in the generator's [d][b][xt][i][y][xx] blocks with its per-pixel counts (the parameters of
// launch_vdi_to_reference): `width` columns of S slots, B bricks per strip
struct SlottedVdi {
    const float4* col;
    const float2* dep;
    const uint16_t* cnt;
    size_t cnt_stride, cnt_dstride, cnt_pitch;
    int width, S, B;
};

// columns [x0, x0 + nx) of brick b of such a VDI in the reference layout: colour (S,H,nx) or depth (2S,H,nx)
int read_columns(insitu_ctx* c, const char* fn, hipStream_t st, const SlottedVdi& v, int b, int x0, int nx, bool colour,
                 void* host_out) {
    auto convert = [&](int, float4* rc, float* rd) {
        return launch_vdi_to_reference(v.col, v.dep, v.cnt, v.cnt_stride, v.cnt_dstride, v.cnt_pitch, v.width, x0, nx,
                                       c->H, v.S, c->strip_w, c->strip_tiles, v.B, b, rc, rd, st);
    };
    return read_reference(c, fn, st, (size_t)nx * (size_t)c->H * (size_t)v.S, colour, 1, host_out, convert);
}

// the sub-VDIs slot f's render left in its send blocks
SlottedVdi rendered_vdi(const insitu_ctx* c, const FrameSlot& f) {
    return {f.vcol_send, f.vdep_send, f.seg_pending, c->framePx, (size_t)c->strip_w, (size_t)c->W, c->W, c->S, c->BV};
}

}  // namespace

extern "C" {

size_t insitu_buffer_bytes(const insitu_ctx* c, int which) {
    if (!c) return 0;
    const size_t px = c->framePx;
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
    const CompletedFrame done = completed_frame(c);
    FrameSlot& f = done.f;
    const hipStream_t st = done.s;
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
    const void* src = nullptr;   // of the buffers that are copied as they lie, below
    switch (which) {
    case INSITU_BUF_VDI_COLOR:
    case INSITU_BUF_VDI_DEPTH:   // (insitu_read_region over every column)
        return read_columns(c, "insitu_read", st, rendered_vdi(c, f), slot, 0, c->W, which == INSITU_BUF_VDI_COLOR,
                            host_out);
    case INSITU_BUF_OCTREE: src = f.octree + (size_t)slot * (need / 4); break;
    case INSITU_BUF_PASSES: src = f.passes + (size_t)slot * need; break;
    case INSITU_BUF_PLAIN_COLOR:
    case INSITU_BUF_PLAIN_DEPTH: {
        const uint32_t* src = which == INSITU_BUF_PLAIN_COLOR ? c->d_pcol_send : c->d_pdep_send;
        for (int d = 0; d < c->N; ++d)
            HIPCHK(c, hipMemcpy((uint8_t*)host_out + (size_t)d * c->plainBlock * 4,
                                src + ((size_t)d * (size_t)c->B + (size_t)slot) * c->plainBlock, c->plainBlock * 4,
                                hipMemcpyDeviceToHost));
        return 0;
    }
    case INSITU_BUF_STRIP: src = c->d_gather; break;   // (this rank's block is the first)
    case INSITU_BUF_IMAGE: src = c->mode == INSITU_MODE_VDI ? c->d_image : c->d_gather; break;
    case INSITU_BUF_COMPOSITED_COLOR:
    case INSITU_BUF_COMPOSITED_DEPTH:
    case INSITU_BUF_GATHERED_COLOR:
    case INSITU_BUF_GATHERED_DEPTH: {
        const bool gathered = which == INSITU_BUF_GATHERED_COLOR || which == INSITU_BUF_GATHERED_DEPTH;
        const bool colour = which == INSITU_BUF_COMPOSITED_COLOR || which == INSITU_BUF_GATHERED_COLOR;
        // gathered: N blocks [rank] of one strip each; a single strip: one block, this rank's (the first)
        // (the slots past each pixel's count are not written by the compositor: zeros here)
        const int width = gathered ? c->W : c->strip_w;
        const SlottedVdi v{c->d_gvdi_col, c->d_gvdi_dep, c->d_gvdi_cnt, 0, c->stripPx,
                           (size_t)c->strip_w, width, c->S_out, 1};
        return read_columns(c, "insitu_read", st, v, 0, 0, width, colour, host_out);
    }
    case INSITU_BUF_COMPOSITE_PASSES: src = c->d_cpasses; break;
    case INSITU_BUF_RECEIVED_COLOR:
    case INSITU_BUF_RECEIVED_DEPTH: {   // block v = list v of the compositor (source-major), a conversion each
        auto convert = [&](int v, float4* rc, float* rd) {
            return launch_vdi_list_to_reference(list_of(c, f, v), c->S, c->H, c->strip_w, c->strip_tiles, rc,
                                                reinterpret_cast<float2*>(rd), st);
        };
        return read_reference(c, "insitu_read", st, c->stripPx * (size_t)c->S, which == INSITU_BUF_RECEIVED_COLOR, c->V,
                              host_out, convert);
    }
    default: return fail(c, -1, "insitu_read: unknown buffer");
    }
    HIPCHK(c, hipMemcpy(host_out, src, need, hipMemcpyDeviceToHost));
    return 0;
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
        HIPCHK(c, hipMemcpy2D(host_out, nx, f.passes + (size_t)slot * c->framePx + (size_t)x0, (size_t)c->W, nx,
                              (size_t)c->H, hipMemcpyDeviceToHost));
        return 0;
    }
    const bool colour = which == INSITU_BUF_VDI_COLOR;
    return read_columns(c, "insitu_read_region", st, rendered_vdi(c, f), slot, x0, (int)nx, colour, host_out);
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
    std::vector<uint8_t> h((size_t)c->BV * c->framePx);
    HIPCHK(c, hipMemcpy(h.data(), f.passes, h.size(), hipMemcpyDeviceToHost));
    long long hit = 0, sum = 0;
    for (uint8_t v : h)
        if (v) { ++hit; sum += v; }
    *rays_hit = hit;
    *mean_passes = hit ? (double)sum / (double)hit : 0.0;
    return 0;
}

}  // extern "C"
