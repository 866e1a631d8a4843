// insitu_view.cpp -- the novel-view subsystem's host side: the insitu_view_* calls of include/insitu_hip.h
// (DESIGN.md section 9).  It shares nothing with the frame's stages but the source insitu_view_bind picks: the
// bound VDI lives in ViewState (insitu_host.h), its work runs on the view's own stream, and every call blocks.
//
// A bind opens with view_unbind, so a bind that fails anywhere leaves no VDI bound; it reserves the per-pixel index
// (view_reserve_index) and, once S or E is known, the entries (view_reserve_entries); its kernels run in timed
// sections (view_timed), whose spans add up to the bind's time; view_commit is the one place it ends.
#include "insitu_host.h"
#include "vdi_pack_format.h"
#include "vdi_view_layout.h"

#include <initializer_list>

#pragma clang fp contract(off)

namespace {

const char* const kBadDimensions = "view bind: needs W, H > 0, at most 2^30 pixels and S in [1,255]";

// a bind or a pack reuses the buffers that a local group's peer has offered to its root (insitu_view_gather_merged)
void offer_withdraw(ViewState& v) {
    if (v.offer.state == ViewState::GatherOffer::Made) v.offer.state = ViewState::GatherOffer::Withdrawn;
}

// every bind's first step: whatever fails after it, no VDI is bound
void view_unbind(ViewState& v) {
    v.bound = v.counted = false;
    offer_withdraw(v);
}

// ... and its last: the generating camera, the kernels' time (the packed bind's is ms_pack as well), the overlaps a
// merge found, and E with the block offsets where the bind ran the offset passes (else counted on demand)
void view_commit(ViewState& v, const float* pv_g, float ms, const PackTotals* counted, long long overlaps = 0,
                 bool packed = false) {
    std::memcpy(v.pv_g, pv_g, sizeof v.pv_g);
    v.overlaps = overlaps;
    v.ms_bind = ms;
    if (packed) v.ms_pack = ms;
    v.counted = counted != nullptr;
    if (counted) v.pk_E = counted->E;
    v.bound = true;
}

// the view's stream and events (first bind)
int view_stream(insitu_ctx* c) {
    ViewState& v = c->view;
    if (!v.stream) HIPCHK(c, hipStreamCreateWithFlags(&v.stream, hipStreamNonBlocking));
    if (!v.ev0) HIPCHK(c, hipEventCreate(&v.ev0));
    if (!v.ev1) HIPCHK(c, hipEventCreate(&v.ev1));
    return 0;
}

// what a timed section enqueued: the first error and the kernel to name with it (null: nothing was launched)
struct Launched {
    hipError_t e;
    const char* kernel;
};
const auto no_launch = []() -> Launched { return {hipSuccess, nullptr}; };

// a device-to-host copy behind a timed section (nothing when bytes == 0)
struct CopyOut {
    void* dst;
    const void* src;
    size_t bytes;
};

// One timed section on the view's stream: ev0, what `enqueue` launches, ev1; behind them the copies of `out`, which
// the span does not cover; one synchronisation.  Adds the span to *ms (nothing when nothing was launched).
template <typename F>
int view_timed(insitu_ctx* c, const char* who, float* ms, F&& enqueue, std::initializer_list<CopyOut> out = {}) {
    ViewState& v = c->view;
    HIPCHK(c, hipEventRecord(v.ev0, v.stream));
    const Launched l = enqueue();
    if (l.e != hipSuccess) return fail(c, -3, std::string(who) + ": " + l.kernel + ": " + hipGetErrorString(l.e));
    HIPCHK(c, hipEventRecord(v.ev1, v.stream));
    for (const CopyOut& o : out)
        if (o.bytes) HIPCHK(c, hipMemcpyAsync(o.dst, o.src, o.bytes, hipMemcpyDeviceToHost, v.stream));
    HIPCHK(c, hipStreamSynchronize(v.stream));
    float span = 0.0f;
    if (l.kernel && hipEventElapsedTime(&span, v.ev0, v.ev1) == hipSuccess) *ms += span;
    return 0;
}

// Room for the per-pixel index of a (W, H) VDI in the view layout this bind takes (INSITU_OPT_VIEW_COMPACT as it
// stands now; the bound VDI keeps it): the counts, the tile maxima and what the offset passes fill (view_count);
// compact: loc.  The slots and the entries follow once they are known (view_reserve_entries).
int view_reserve_index(insitu_ctx* c, int W, int H) {
    ViewState& v = c->view;
    if (int rc = view_stream(c)) return rc;
    v.vdi = ViewVdi{};
    ViewLayoutSize sz{};
    if (!view_pixels(W, H, &sz)) return fail(c, -1, kBadDimensions);
    const size_t blocks = (size_t)view_blocks(sz.px);
    int rc = 0;
    if ((rc = v.cnt.reserve(c, (size_t)sz.px)) || (rc = v.tmax.reserve(c, (size_t)sz.tiles)) ||
        (rc = v.pk_totals.reserve(c, 1)) || (rc = v.pk_bstat.reserve(c, blocks)) || (rc = v.pk_boff.reserve(c, blocks)))
        return rc;
    if (!v.h_totals) HIPCHK(c, v.h_totals.try_alloc(1));
    if (v.compact_next != 0) {
        if ((rc = v.loc.reserve(c, (size_t)sz.px))) return rc;
        v.vdi.loc = v.loc; v.vdi.boff = v.pk_boff;
    }
    v.vdi.cnt = v.cnt; v.vdi.tmax = v.tmax;
    v.vdi.W = W; v.vdi.H = H; v.vdi.tiles_x = (W + 7) / 8; v.vdi.tiles_y = (H + 7) / 8;
    return 0;
}

// The VDI's S slots per list and room for its entries: dense W*H*S; compact the E its counts add up to (at least 1)
int view_reserve_entries(insitu_ctx* c, int S, unsigned long long E) {
    ViewState& v = c->view;
    ViewLayoutSize sz{};
    if (v.vdi.loc ? !view_compact_size(v.vdi.W, v.vdi.H, S, E, &sz) : !view_dense_size(v.vdi.W, v.vdi.H, S, &sz))
        return fail(c, -1, kBadDimensions);
    int rc = 0;
    if ((rc = v.col.reserve(c, (size_t)sz.entries)) || (rc = v.dep.reserve(c, (size_t)sz.entries))) return rc;
    v.vdi.col = v.col; v.vdi.dep = v.dep; v.vdi.S = S;
    return 0;
}

// The offset passes (pack_count_kernel, pack_scan_kernel) over the counts of the view's index, behind what `first`
// launches (a pass that writes those counts), in one timed section: boff, a compact VDI's loc, and *tot = what they
// found.  S bounds every count.  With check_E the counts are a stream's, and *tot tells the caller when they are to
// be rejected.
template <typename F>
int view_count(insitu_ctx* c, const char* who, int S, int check_E, unsigned long long expect_E, PackTotals* tot, float* ms,
               F&& first) {
    ViewState& v = c->view;
    ViewLayoutSize sz{};
    if (!view_compact_size(v.vdi.W, v.vdi.H, S, 0, &sz)) return fail(c, -1, kBadDimensions);
    const PackOffsets o{v.vdi.cnt, v.pk_bstat, v.pk_boff, v.pk_totals, (uint32_t)sz.px, (uint32_t)sz.nblocks,
                        v.vdi.loc ? v.loc.get() : nullptr};
    const auto passes = [&]() -> Launched {
        const Launched l = first();
        if (l.e != hipSuccess) return l;
        return {launch_pack_offsets(o, S, check_E, expect_E, v.stream), "pack_count_kernel"};
    };
    if (int rc = view_timed(c, who, ms, passes, {{v.h_totals.get(), v.pk_totals.get(), sizeof(PackTotals)}})) return rc;
    *tot = *v.h_totals;
    if (tot->bad && !check_E)
        return fail(c, -6, std::string(who) + ": a count of the " + (v.bound ? "bound " : "") + "VDI exceeds S (internal error)");
    return 0;
}

// view_build_kernel over `src`, one list of S slots per pixel, into the reserved index (compact: the count pass with
// the offsets, then the write pass); blocks until the snapshot is built
int view_build(insitu_ctx* c, const ViewSource& src, int S, const float* pv_g, const char* who) {
    ViewState& v = c->view;
    const bool compact = v.vdi.loc != nullptr;
    PackTotals tot{};
    float ms = 0.0f;
    if (compact) {
        ViewVdi lists = v.vdi;   // (the count pass reads S slots per list; the VDI takes its S with its entries)
        lists.S = S;
        const auto count = [&]() -> Launched { return {launch_view_build_count(src, lists, v.stream), "view_build_count_kernel"}; };
        if (int rc = view_count(c, who, S, 0, 0, &tot, &ms, count)) return rc;
    }
    if (int rc = view_reserve_entries(c, S, tot.E)) return rc;
    const auto build = [&]() -> Launched {
        return {compact ? launch_view_build_fill(src, v.vdi, v.stream) : launch_view_build(src, v.vdi, v.stream), "view_build_kernel"};
    };
    if (int rc = view_timed(c, who, &ms, build)) return rc;
    view_commit(v, pv_g, ms, compact ? &tot : nullptr);
    return 0;
}

// The merged bind: the src.n lists per pixel of the reserved index's window, S slots each, merged by
// start depth into a VDI of S_m = max(1, the longest merged list) slots.  More than 255 is rejected.  Blocks until
// the snapshot is built.  SRC: ViewSource, or PackedSource (a set of packed streams, whose offset passes took ms0).
template <class SRC>
int view_merge(insitu_ctx* c, const SRC& src, int S, const float* pv_g, const char* who, float ms0 = 0.0f) {
    ViewState& v = c->view;
    if (int rc = v.mg_totals.reserve(c, 1)) return rc;
    if (!v.h_mg_totals) HIPCHK(c, v.h_mg_totals.try_alloc(1));
    const CopyOut totals{v.h_mg_totals.get(), v.mg_totals.get(), sizeof(MergeTotals)};
    const bool compact = v.vdi.loc != nullptr;
    float ms = ms0;
    // compact: the count pass leaves every pixel's merged length as its count (the slots are known after it)
    const auto count = [&]() -> Launched {
        return {launch_view_merge_count(src, v.vdi.W, v.vdi.H, S, v.mg_totals, compact ? v.vdi.cnt : nullptr, v.stream),
                "view_merge_count_kernel"};
    };
    if (int rc = view_timed(c, who, &ms, count, {totals})) return rc;
    const uint32_t longest = v.h_mg_totals->max_count;
    if (longest > 255u)
        return fail(c, -1, std::string(who) + ": the merged lists hold up to " + std::to_string(longest) +
                               " entries per pixel, at most 255 can be bound");
    const int Sm = longest > 0u ? (int)longest : 1;
    PackTotals tot{};
    if (compact)
        if (int rc = view_count(c, who, Sm, 0, 0, &tot, &ms, no_launch)) return rc;
    if (int rc = view_reserve_entries(c, Sm, tot.E)) return rc;
    const auto merge = [&]() -> Launched { return {launch_view_merge(src, S, v.vdi, v.mg_totals, v.stream), "view_merge_kernel"}; };
    if (int rc = view_timed(c, who, &ms, merge, {totals})) return rc;
    view_commit(v, pv_g, ms, compact ? &tot : nullptr, (long long)v.h_mg_totals->overlaps);
    return 0;
}

// (a set of one list is that list: bound with its own S slots, as INSITU_VIEW_BRICK binds it)
int view_bind_lists(insitu_ctx* c, const ViewSource& src, int S, const float* pv_g, const char* who) {
    return src.n > 1 ? view_merge(c, src, S, pv_g, who) : view_build(c, src, S, pv_g, who);
}

}  // namespace

int insitu_view_bind(insitu_ctx* c, int source, int slot) {
    if (!c) return fail(nullptr, -1, "insitu_view_bind: null context");
    view_unbind(c->view);
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
    if (int rc = view_reserve_index(c, c->W, c->H)) return rc;
    return view_bind_lists(c, src, S, pv, "insitu_view_bind");
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
    if (int rc = view_reserve_index(c, W, H)) return rc;
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
    return view_bind_lists(c, src, S, pv, who);   // (blocks: the staging is free afterwards)
}

}  // namespace

int insitu_view_bind_host(insitu_ctx* c, const void* color, const void* depth, int W, int H, int S,
                          const insitu_camera* gen_cam) {
    if (!c) return fail(nullptr, -1, "insitu_view_bind_host: null context");
    view_unbind(c->view);
    if (!color || !depth || !gen_cam) return fail(c, -1, "insitu_view_bind_host: null argument");
    return view_bind_host_lists(c, "insitu_view_bind_host", &color, &depth, 1, W, H, S, gen_cam);
}

int insitu_view_bind_host_set(insitu_ctx* c, const void* const* colors, const void* const* depths, int n, int W, int H,
                              int S, const insitu_camera* gen_cam) {
    const char* who = "insitu_view_bind_host_set";
    if (!c) return fail(nullptr, -1, std::string(who) + ": null context");
    view_unbind(c->view);
    if (!colors || !depths || !gen_cam) return fail(c, -1, std::string(who) + ": null argument");
    if (n < 1 || n > kMaxLists)
        return fail(c, -1, std::string(who) + ": " + std::to_string(n) + " VDIs, needs 1 to " + std::to_string(kMaxLists));
    for (int j = 0; j < n; ++j)
        if (!colors[j] || !depths[j]) return fail(c, -1, std::string(who) + ": null VDI " + std::to_string(j));
    return view_bind_host_lists(c, who, colors, depths, n, W, H, S, gen_cam);
}

// ---- the packed stream of the bound VDI (vdi_pack.hip, vdi_pack_format.h) ----
namespace {

// E and the block offsets of the bound VDI: counted once per bind
int pack_count_bound(insitu_ctx* c, float* ms, const char* who) {
    ViewState& v = c->view;
    if (v.counted) return 0;
    PackTotals tot{};
    if (int rc = view_count(c, who, v.vdi.S, 0, 0, &tot, ms, no_launch)) return rc;
    v.pk_E = tot.E;
    v.counted = true;
    return 0;
}

// Where the depth and colour sections of a stream of the view's VDI lie on the device, and so which kernel goes
// between them and the view layout (pack_launch):
//   dense          staged, depth at 0 and colour at the next multiple of 16: vdi_pack / vdi_unpack
//   compact FLOAT  the VDI's own arrays are the sections: no kernel (on a bind, the tile maxima)
//   compact HALF   the VDI's depths, and staged colours converted element by element
struct PackSections {
    float2* dep;
    void* col;
};

int pack_sections(insitu_ctx* c, bool half, const PackLayout& lay, PackSections* s) {
    ViewState& v = c->view;
    if (!v.vdi.loc) {
        const size_t colour_at = (lay.depth_bytes + 15) & ~(size_t)15;
        if (int rc = v.pk_stage.reserve(c, colour_at + lay.colour_bytes)) return rc;
        *s = {reinterpret_cast<float2*>(v.pk_stage.get()), v.pk_stage + colour_at};
    } else if (half) {
        if (int rc = v.pk_stage.reserve(c, lay.colour_bytes)) return rc;
        *s = {v.vdi.dep, v.pk_stage.get()};
    } else {
        *s = {v.vdi.dep, v.vdi.col};
    }
    return 0;
}

// the kernel between the view layout and the E entries of the sections: to the stream, or from it
Launched pack_launch(ViewState& v, const PackSections& s, bool half, unsigned long long E, bool to_stream) {
    if (!v.vdi.loc) {
        const PackParams p{v.vdi, v.pk_boff, s.dep, s.col, half ? 1 : 0};
        if (to_stream) return {launch_vdi_pack(p, v.stream), "vdi_pack_kernel"};
        return {launch_vdi_unpack(p, v.stream), "vdi_unpack_kernel"};
    }
    if (to_stream) {
        if (!half || E == 0) return no_launch();
        return {launch_pack_convert(v.vdi.col, s.col, E, 1, v.stream), "pack_convert_kernel"};
    }
    const hipError_t e = half ? launch_pack_convert(s.col, v.vdi.col, E, 0, v.stream) : hipSuccess;
    return {e == hipSuccess ? launch_view_tmax(v.vdi, v.stream) : e, "pack_convert_kernel"};
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
    const char* who = "insitu_view_pack";
    if (!c) return fail(nullptr, -1, "insitu_view_pack: null context");
    ViewState& v = c->view;
    if (!pack_format_ok(format)) return fail(c, -1, "insitu_view_pack: bad format " + std::to_string(format));
    if (!v.bound) return fail(c, -1, "insitu_view_pack: no VDI bound (insitu_view_bind first)");
    HIPCHK(c, hipSetDevice(c->cfg.device));
    float ms = 0.0f;
    if (int rc = pack_count_bound(c, &ms, who)) return rc;
    PackHeader h{};
    h.format = (uint32_t)format; h.W = (uint32_t)v.vdi.W; h.H = (uint32_t)v.vdi.H; h.S = (uint32_t)v.vdi.S;
    h.E = v.pk_E;
    std::memcpy(h.pv_g, v.pv_g, sizeof h.pv_g);
    PackLayout lay{};
    if (!pack_layout(h.format, h.W, h.H, h.S, h.E, &lay)) return fail(c, -1, "insitu_view_pack: the stream's size does not fit");
    if (bytes) *bytes = lay.total;
    if (!host_out || cap < lay.total)
        return fail(c, -1, "insitu_view_pack: output buffer too small (" + std::to_string(lay.total) + " bytes needed)");
    const bool half = format == INSITU_PACK_HALF;
    PackSections s{};
    offer_withdraw(v);
    if (int rc = pack_sections(c, half, lay, &s)) return rc;
    unsigned char* out = static_cast<unsigned char*>(host_out);
    // (E == 0: the sections are empty, and nothing is copied from arrays that may not exist)
    if (int rc = view_timed(c, who, &ms, [&] { return pack_launch(v, s, half, h.E, true); },
                            {{out + kPackHeaderBytes, v.vdi.cnt, (size_t)lay.px},
                             {out + lay.depth_off, s.dep, lay.depth_bytes},
                             {out + lay.colour_off, s.col, lay.colour_bytes}}))
        return rc;
    pack_write_header(out, h);
    std::memset(out + kPackHeaderBytes + (size_t)lay.px, 0, lay.depth_off - kPackHeaderBytes - (size_t)lay.px);
    v.ms_pack = ms;
    return 0;
}

namespace {

// what a rejected stream's message begins with: `who`, and in a set the stream's index
std::string pack_rejected(const char* who, int index) {
    return std::string(who) + (index < 0 ? ": stream rejected: " : ": stream " + std::to_string(index) + " rejected: ");
}
std::string pack_bad_counts(const PackTotals& tot, const PackHeader& h) {
    if (tot.max_count > h.S) return "a count of " + std::to_string(tot.max_count) + " exceeds S = " + std::to_string(h.S);
    return "the counts add up to " + std::to_string(tot.E) + ", the header says " + std::to_string(h.E);
}

// the counts and the two sections of a parsed stream where they lie: behind its header in host memory, or staged on
// the device (insitu_view_gather_merged)
struct PackedBytes {
    const void* cnt;
    const void* dep;
    const void* col;
    hipMemcpyKind kind;
};

// one parsed stream into the view layout; index: see pack_rejected
int view_bind_packed_parsed(insitu_ctx* c, const char* who, int index, const PackHeader& h, const PackLayout& lay,
                            const PackedBytes& in) {
    ViewState& v = c->view;
    HIPCHK(c, hipSetDevice(c->cfg.device));
    if (int rc = view_reserve_index(c, (int)h.W, (int)h.H)) return rc;
    // the counts go straight into the view layout, and are validated on the device before anything depends on
    // them: every count <= S, and the counts add up to E
    HIPCHK(c, hipMemcpyAsync(v.vdi.cnt, in.cnt, (size_t)lay.px, in.kind, v.stream));
    PackTotals tot{};
    float ms = 0.0f;
    if (int rc = view_count(c, who, (int)h.S, 1, h.E, &tot, &ms, no_launch)) return rc;
    if (tot.bad) return fail(c, -1, pack_rejected(who, index) + pack_bad_counts(tot, h));
    const bool half = h.format == kPackHalf;
    PackSections s{};
    if (int rc = view_reserve_entries(c, (int)h.S, h.E)) return rc;
    if (int rc = pack_sections(c, half, lay, &s)) return rc;
    if (h.E > 0) {
        HIPCHK(c, hipMemcpyAsync(s.dep, in.dep, lay.depth_bytes, in.kind, v.stream));
        HIPCHK(c, hipMemcpyAsync(s.col, in.col, lay.colour_bytes, in.kind, v.stream));
    }
    if (int rc = view_timed(c, who, &ms, [&] { return pack_launch(v, s, half, h.E, false); })) return rc;
    view_commit(v, h.pv_g, ms, &tot, 0, true);
    return 0;
}

// one packed stream into the view layout (insitu_view_bind_packed; a set of one)
int view_bind_packed_one(insitu_ctx* c, const char* who, int index, const void* data, size_t bytes) {
    PackHeader h{};
    PackLayout lay{};
    if (const char* why = pack_parse(data, bytes, &h, &lay)) return fail(c, -1, pack_rejected(who, index) + why);
    const unsigned char* in = static_cast<const unsigned char*>(data);
    return view_bind_packed_parsed(c, who, index, h, lay,
                                   {in + kPackHeaderBytes, in + lay.depth_off, in + lay.colour_off, hipMemcpyHostToDevice});
}

// The index of a set's streams, apart from the bound VDI's (ViewState::ps_index): table | totals | per stream boff |
// bstat | loc
struct PackSetIndex {
    size_t px, nb, totals_at, boff_at, bstat_at, loc_at, bytes;
};
PackSetIndex pack_set_index(int n, uint64_t pixels) {
    PackSetIndex x{};
    const size_t N = (size_t)n;
    x.px = (size_t)pixels;
    x.nb = (size_t)view_blocks(pixels);
    x.totals_at = (N * sizeof(PackedStream) + 15) & ~(size_t)15;
    x.boff_at = x.totals_at + N * sizeof(PackTotals);
    x.bstat_at = x.boff_at + N * x.nb * sizeof(unsigned long long);
    x.loc_at = (x.bstat_at + N * x.nb * sizeof(uint32_t) + 15) & ~(size_t)15;
    x.bytes = x.loc_at + N * x.px * sizeof(uint16_t);
    return x;
}

// room for the n parsed streams of a set and their index: at[j] says where stream j is staged in ps_stage
int view_set_reserve(insitu_ctx* c, const char* who, const PackLayout* lay, int n, PackSetStage* at) {
    ViewState& v = c->view;
    size_t stage_bytes = 0;
    if (!pack_set_stage(lay, n, at, &stage_bytes)) return fail(c, -1, std::string(who) + ": the streams' size does not fit");
    int rc = 0;
    if ((rc = v.ps_index.reserve(c, pack_set_index(n, lay[0].px).bytes)) ||
        (rc = v.ps_stage.reserve(c, stage_bytes > 0 ? stage_bytes : 16)))
        return rc;
    if (!v.h_ps_totals) HIPCHK(c, v.h_ps_totals.try_alloc((size_t)kMaxLists));
    return 0;
}

// The bind of n >= 2 staged streams (view_set_reserve; their counts and sections are in ps_stage, or on their way
// there on the view's stream): the PackedStream table, the offset passes over every stream's counts -- which
// validate them before a kernel reads an entry that they place -- and the merge.
int view_set_bind(insitu_ctx* c, const char* who, const PackHeader* h, const PackLayout* lay, const PackSetStage* at, int n) {
    ViewState& v = c->view;
    if (int rc = view_reserve_index(c, (int)h[0].W, (int)h[0].H)) return rc;
    const PackSetIndex x = pack_set_index(n, lay[0].px);
    unsigned char* const ix = v.ps_index.get();
    unsigned char* const sg = v.ps_stage.get();
    PackTotals* const d_totals = reinterpret_cast<PackTotals*>(ix + x.totals_at);
    PackedStream table[kPackSetMax];
    int Smax = 1;
    for (int j = 0; j < n; ++j) {
        PackedStream& t = table[j];
        t.off = PackOffsets{sg + at[j].cnt_at,
                            reinterpret_cast<uint32_t*>(ix + x.bstat_at) + (size_t)j * x.nb,
                            reinterpret_cast<unsigned long long*>(ix + x.boff_at) + (size_t)j * x.nb,
                            d_totals + j, (uint32_t)x.px, (uint32_t)x.nb,
                            reinterpret_cast<uint16_t*>(ix + x.loc_at) + (size_t)j * x.px};
        t.dep = reinterpret_cast<const float2*>(sg + at[j].dep_at);
        t.col = sg + at[j].col_at;
        t.E = h[j].E;
        t.S = h[j].S;
        t.half = h[j].format == kPackHalf ? 1u : 0u;
        Smax = (int)h[j].S > Smax ? (int)h[j].S : Smax;
    }
    HIPCHK(c, hipMemcpyAsync(ix, table, (size_t)n * sizeof(PackedStream), hipMemcpyHostToDevice, v.stream));
    const PackedStream* const d_table = reinterpret_cast<const PackedStream*>(ix);
    float ms = 0.0f;
    const auto offsets = [&]() -> Launched {
        return {launch_pack_offsets_set(d_table, n, (uint32_t)x.px, (uint32_t)x.nb, v.stream), "pack_count_set_kernel"};
    };
    if (int rc = view_timed(c, who, &ms, offsets, {{v.h_ps_totals.get(), d_totals, (size_t)n * sizeof(PackTotals)}})) return rc;
    for (int j = 0; j < n; ++j)
        if (v.h_ps_totals[j].bad) return fail(c, -1, pack_rejected(who, j) + pack_bad_counts(v.h_ps_totals[j], h[j]));
    return view_merge(c, PackedSource{d_table, n, (int)h[0].W}, Smax, h[0].pv_g, who, ms);
}

}  // namespace

int insitu_view_bind_packed(insitu_ctx* c, const void* data, size_t bytes) {
    if (!c) return fail(nullptr, -1, "insitu_view_bind_packed: null context");
    view_unbind(c->view);
    return view_bind_packed_one(c, "insitu_view_bind_packed", -1, data, bytes);
}

// n packed streams of one window and one generating camera, merged per pixel straight from their sections (DESIGN.md
// section 9.8): staged as they arrive, each with an index of its own (boff, loc: the offset passes over its counts,
// which also validate them), read by the merge kernels as a PackedSource.  No stream is expanded to S-slot lists.
int insitu_view_bind_packed_set(insitu_ctx* c, const void* const* streams, const size_t* bytes, int n) {
    const char* who = "insitu_view_bind_packed_set";
    static_assert(kPackSetMax == kMaxLists, "a set holds as many streams as the merge takes lists");
    if (!c) return fail(nullptr, -1, std::string(who) + ": null context");
    ViewState& v = c->view;
    view_unbind(v);
    if (!streams || !bytes) return fail(c, -1, std::string(who) + ": null argument");
    if (n < 1 || n > kMaxLists)
        return fail(c, -1, std::string(who) + ": " + std::to_string(n) + " streams, needs 1 to " + std::to_string(kMaxLists));
    if (n == 1) return view_bind_packed_one(c, who, 0, streams[0], bytes[0]);
    PackHeader h[kPackSetMax];
    PackLayout lay[kPackSetMax];
    PackSetStage at[kPackSetMax];
    int index = -1;
    if (const char* why = pack_set_parse(streams, bytes, n, h, lay, &index))
        return fail(c, -1, index < 0 ? std::string(who) + ": " + why : pack_rejected(who, index) + why);
    HIPCHK(c, hipSetDevice(c->cfg.device));
    if (int rc = view_stream(c)) return rc;
    if (int rc = view_set_reserve(c, who, lay, n, at)) return rc;
    unsigned char* const sg = v.ps_stage.get();
    for (int j = 0; j < n; ++j) {
        // each stream is uploaded once, as it is: its counts and depths lie together in it as they do in the staging
        const unsigned char* in = static_cast<const unsigned char*>(streams[j]);
        HIPCHK(c, hipMemcpyAsync(sg + at[j].cnt_at, in + kPackHeaderBytes, lay[j].colour_off - kPackHeaderBytes,
                                 hipMemcpyHostToDevice, v.stream));
        if (lay[j].colour_bytes)
            HIPCHK(c, hipMemcpyAsync(sg + at[j].col_at, in + lay[j].colour_off, lay[j].colour_bytes, hipMemcpyHostToDevice, v.stream));
    }
    return view_set_bind(c, who, h, lay, at, n);
}

// ---- the ranks' bound VDIs gathered into one merged VDI on rank 0 ----
namespace {

// a rank's part in a gather: its stream's header and layout, and where the sections lie on its device
struct GatherStream {
    PackHeader h{};
    PackLayout lay{};
    PackSections s{};
    uint32_t refusal = kGatherAccepted;   // else why the rank cannot take part (it still has its turn in the protocol)
};

// what travels back from the root: kGatherAccepted, or the rank the gather fails on and why
struct GatherVerdict {
    uint32_t reason;
    int32_t rank;
    uint32_t pad[2];
};

int gather_rejected(insitu_ctx* c, const char* who, int rank, uint32_t reason) {
    return fail(c, -1, std::string(who) + ": rank " + std::to_string(rank) + " rejected: " + pack_gather_reason_text(reason));
}

// insitu_view_pack up to the sections: the bound VDI's stream on the device, nothing of it copied out
int gather_prepare(insitu_ctx* c, int format, const char* who, GatherStream* g) {
    ViewState& v = c->view;
    if (!v.bound) g->refusal = kGatherNothingBound;
    else if (!pack_format_ok(format)) g->refusal = kGatherBadFormatArgument;
    else if (c->N > 1 && c->pipe_inflight) g->refusal = kGatherFrameInFlight;
    if (g->refusal) return 0;
    float ms = 0.0f;
    if (int rc = pack_count_bound(c, &ms, who)) return rc;
    PackHeader& h = g->h;
    h.format = (uint32_t)format; h.W = (uint32_t)v.vdi.W; h.H = (uint32_t)v.vdi.H; h.S = (uint32_t)v.vdi.S;
    h.E = v.pk_E;
    std::memcpy(h.pv_g, v.pv_g, sizeof h.pv_g);
    if (!pack_layout(h.format, h.W, h.H, h.S, h.E, &g->lay)) return fail(c, -1, std::string(who) + ": the stream's size does not fit");
    const bool half = format == INSITU_PACK_HALF;
    offer_withdraw(v);
    if (int rc = pack_sections(c, half, g->lay, &g->s)) {
        if (rc != -5) return rc;
        g->refusal = kGatherAllocationFailed;
        return 0;
    }
    if (int rc = view_timed(c, who, &ms, [&] { return pack_launch(v, g->s, half, h.E, true); })) return rc;
    v.ms_pack = ms;
    return 0;
}

unsigned long long gather_section_bytes(const PackLayout& lay) {
    return (unsigned long long)lay.px + (unsigned long long)lay.depth_bytes + (unsigned long long)lay.colour_bytes;
}

int view_gather(insitu_ctx* c, int format, unsigned long long* wire_bytes, const char* who) {
    ViewState& v = c->view;
    using Offer = ViewState::GatherOffer;
    const int N = c->N;
    const bool root = is_root(c), local = c->group != nullptr, rccl = N > 1 && !local;
    HIPCHK(c, hipSetDevice(c->cfg.device));
    if (int rc = view_stream(c)) return rc;
    // the communicator is used on the view's stream: what the frame's stages left on theirs is done first
    if (rccl && !c->pipe_inflight) HIPCHK(c, hipStreamSynchronize(c->stream));
    GatherStream mine;
    if (int rc = gather_prepare(c, format, who, &mine)) return rc;
    unsigned char head[kPackHeaderBytes];
    if (mine.refusal) pack_write_refusal(head, mine.refusal);
    else pack_write_header(head, mine.h);

    if (local && N > 1 && !root) {   // the offer: the root's call pulls it
        Offer& o = v.offer;
        o.state = Offer::None;
        if (!o.ev) HIPCHK(c, hipEventCreateWithFlags(&o.ev, hipEventDisableTiming));
        std::memcpy(o.header, head, sizeof head);
        o.cnt = mine.refusal ? nullptr : v.vdi.cnt;
        o.dep = mine.s.dep;
        o.col = mine.s.col;
        HIPCHK(c, hipEventRecord(o.ev, v.stream));
        o.state = Offer::Made;
        if (wire_bytes && !mine.refusal) *wire_bytes = gather_section_bytes(mine.lay);
        return 0;
    }

    // 1. the offer: every rank's header
    const size_t verdict_at = (size_t)(root ? N : 1) * kPackHeaderBytes;
    if (rccl) {
        int rc = 0;
        if ((rc = v.gm_ctl.reserve(c, (size_t)kPackSetMax * kPackHeaderBytes + sizeof(GatherVerdict))) ||
            (rc = v.h_gm_ctl.reserve(c, (size_t)kPackSetMax * kPackHeaderBytes + sizeof(GatherVerdict))))
            return rc;
    }
    if (!root) {   // a peer over RCCL
        std::memcpy(v.h_gm_ctl.get(), head, sizeof head);
        HIPCHK(c, hipMemcpyAsync(v.gm_ctl.get(), v.h_gm_ctl.get(), sizeof head, hipMemcpyHostToDevice, v.stream));
        NCCLCHK(c, ncclGroupStart());
        NCCLCHK(c, ncclSend(v.gm_ctl.get(), sizeof head, ncclUint8, 0, c->comm, v.stream));
        NCCLCHK(c, ncclGroupEnd());
        // (the offer has left before the wait for the root's answer is enqueued: nothing that a peer's progress
        // depends on is ever queued behind a wait)
        HIPCHK(c, hipStreamSynchronize(v.stream));
        // 2. the verdict
        NCCLCHK(c, ncclGroupStart());
        NCCLCHK(c, ncclRecv(v.gm_ctl + verdict_at, sizeof(GatherVerdict), ncclUint8, 0, c->comm, v.stream));
        NCCLCHK(c, ncclGroupEnd());
        HIPCHK(c, hipMemcpyAsync(v.h_gm_ctl + verdict_at, v.gm_ctl + verdict_at, sizeof(GatherVerdict), hipMemcpyDeviceToHost, v.stream));
        HIPCHK(c, hipStreamSynchronize(v.stream));
        GatherVerdict verdict;
        std::memcpy(&verdict, v.h_gm_ctl + verdict_at, sizeof verdict);
        if (verdict.reason != kGatherAccepted) return gather_rejected(c, who, verdict.rank, verdict.reason);
        // 3. the payload (an empty section is not sent)
        NCCLCHK(c, ncclGroupStart());
        NCCLCHK(c, ncclSend(v.vdi.cnt, (size_t)mine.lay.px, ncclUint8, 0, c->comm, v.stream));
        if (mine.h.E > 0) {
            NCCLCHK(c, ncclSend(mine.s.dep, mine.lay.depth_bytes, ncclUint8, 0, c->comm, v.stream));
            NCCLCHK(c, ncclSend(mine.s.col, mine.lay.colour_bytes, ncclUint8, 0, c->comm, v.stream));
        }
        NCCLCHK(c, ncclGroupEnd());
        HIPCHK(c, hipStreamSynchronize(v.stream));
        if (wire_bytes) *wire_bytes = gather_section_bytes(mine.lay);
        return 0;
    }

    // the root (N = 1: the only rank)
    unsigned char local_heads[kPackSetMax * kPackHeaderBytes];
    unsigned char* heads = local_heads;
    Offer offers[kPackSetMax];
    if (rccl) {
        heads = v.h_gm_ctl.get();
        NCCLCHK(c, ncclGroupStart());
        for (int p = 1; p < N; ++p)
            NCCLCHK(c, ncclRecv(v.gm_ctl + (size_t)p * kPackHeaderBytes, kPackHeaderBytes, ncclUint8, p, c->comm, v.stream));
        NCCLCHK(c, ncclGroupEnd());
        HIPCHK(c, hipMemcpyAsync(heads, v.gm_ctl.get(), (size_t)N * kPackHeaderBytes, hipMemcpyDeviceToHost, v.stream));
        HIPCHK(c, hipStreamSynchronize(v.stream));
    } else if (N > 1) {
        for (int p = 1; p < N; ++p) {
            const insitu_ctx* q = c->group->ranks[p];
            const std::string rank = std::string(who) + ": local group rank " + std::to_string(p);
            if (!q) return fail(c, -1, rank + " missing");
            if (q->view.offer.state == Offer::None) return fail(c, -1, rank + " has not offered (the peers call first, the root last)");
            if (q->view.offer.state == Offer::Withdrawn) return fail(c, -1, rank + " has bound or packed since its offer");
        }
        for (int p = 1; p < N; ++p) {   // consumed, whatever comes of them
            Offer& o = c->group->ranks[p]->view.offer;
            offers[p] = o;
            o.state = Offer::None;
            std::memcpy(heads + (size_t)p * kPackHeaderBytes, o.header, kPackHeaderBytes);
        }
    }
    std::memcpy(heads, head, sizeof head);

    // 2. the verdict, once the root has room for what an accepted set sends
    PackHeader h[kPackSetMax];
    PackLayout lay[kPackSetMax];
    PackSetStage at[kPackSetMax];
    GatherVerdict verdict{};
    int index = -1;
    verdict.reason = pack_header_set_check(heads, N, h, lay, &index);
    verdict.rank = index;
    if (verdict.reason == kGatherAccepted) {
        if (int rc = view_set_reserve(c, who, lay, N, at)) {
            if (!rccl) return rc;
            verdict.reason = kGatherAllocationFailed;
            verdict.rank = 0;
        }
    }
    if (rccl) {
        std::memcpy(heads + verdict_at, &verdict, sizeof verdict);
        HIPCHK(c, hipMemcpyAsync(v.gm_ctl + verdict_at, heads + verdict_at, sizeof verdict, hipMemcpyHostToDevice, v.stream));
        NCCLCHK(c, ncclGroupStart());
        for (int p = 1; p < N; ++p)
            NCCLCHK(c, ncclSend(v.gm_ctl + verdict_at, sizeof verdict, ncclUint8, p, c->comm, v.stream));
        NCCLCHK(c, ncclGroupEnd());
        if (verdict.reason != kGatherAccepted) HIPCHK(c, hipStreamSynchronize(v.stream));
    }
    if (verdict.reason != kGatherAccepted) return gather_rejected(c, who, verdict.rank, verdict.reason);

    // 3. the payload: the root's own stream into slot 0, before the bind reuses the buffers it lies in ...
    unsigned char* const sg = v.ps_stage.get();
    HIPCHK(c, hipMemcpyAsync(sg + at[0].cnt_at, v.vdi.cnt, (size_t)lay[0].px, hipMemcpyDeviceToDevice, v.stream));
    if (h[0].E > 0) {
        HIPCHK(c, hipMemcpyAsync(sg + at[0].dep_at, mine.s.dep, lay[0].depth_bytes, hipMemcpyDeviceToDevice, v.stream));
        HIPCHK(c, hipMemcpyAsync(sg + at[0].col_at, mine.s.col, lay[0].colour_bytes, hipMemcpyDeviceToDevice, v.stream));
    }
    // ... and every peer's at its place (an empty section is not sent)
    unsigned long long wire = 0;
    if (rccl) NCCLCHK(c, ncclGroupStart());
    for (int p = 1; p < N; ++p) {
        wire += gather_section_bytes(lay[p]);
        if (rccl) {
            NCCLCHK(c, ncclRecv(sg + at[p].cnt_at, (size_t)lay[p].px, ncclUint8, p, c->comm, v.stream));
            if (h[p].E > 0) {
                NCCLCHK(c, ncclRecv(sg + at[p].dep_at, lay[p].depth_bytes, ncclUint8, p, c->comm, v.stream));
                NCCLCHK(c, ncclRecv(sg + at[p].col_at, lay[p].colour_bytes, ncclUint8, p, c->comm, v.stream));
            }
        } else {
            const Offer& o = offers[p];
            HIPCHK(c, hipStreamWaitEvent(v.stream, o.ev, 0));   // the peer's pack, its stream
            HIPCHK(c, hipMemcpyAsync(sg + at[p].cnt_at, o.cnt, (size_t)lay[p].px, hipMemcpyDeviceToDevice, v.stream));
            if (h[p].E > 0) {
                HIPCHK(c, hipMemcpyAsync(sg + at[p].dep_at, o.dep, lay[p].depth_bytes, hipMemcpyDeviceToDevice, v.stream));
                HIPCHK(c, hipMemcpyAsync(sg + at[p].col_at, o.col, lay[p].colour_bytes, hipMemcpyDeviceToDevice, v.stream));
            }
        }
    }
    if (rccl) NCCLCHK(c, ncclGroupEnd());
    HIPCHK(c, hipStreamSynchronize(v.stream));
    if (wire_bytes) *wire_bytes = wire;

    // 4. the bind: from here on the root's own VDI is a stream among the others
    view_unbind(v);
    if (N == 1)
        return view_bind_packed_parsed(c, who, -1, h[0], lay[0],
                                       {sg + at[0].cnt_at, sg + at[0].dep_at, sg + at[0].col_at, hipMemcpyDeviceToDevice});
    return view_set_bind(c, who, h, lay, at, N);
}

}  // namespace

int insitu_view_gather_merged(insitu_ctx* c, int format, unsigned long long* wire_bytes) {
    const char* who = "insitu_view_gather_merged";
    if (!c) return fail(nullptr, -1, std::string(who) + ": null context");
    if (wire_bytes) *wire_bytes = 0;
    const int rc = c->N > kPackSetMax
                       ? fail(c, -1, std::string(who) + ": " + std::to_string(c->N) + " ranks, at most " + std::to_string(kPackSetMax))
                       : view_gather(c, format, wire_bytes, who);
    if (rc != 0 && is_root(c)) view_unbind(c->view);   // (a failed bind leaves no VDI bound)
    return rc;
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
    float ms = 0.0f;
    if (int rc = view_timed(c, "insitu_view_render", &ms, [&]() -> Launched { return {launch_vdi_view(p, v.stream), "vdi_view_kernel"}; },
                            {{host_out, v.out_image.get(), host_out ? px * 4 : 0}}))
        return rc;
    v.out_w = out_w; v.out_h = out_h;
    v.ms = ms;
    return 0;
}

int view_stats(insitu_ctx* c, insitu_stats* out) {
    ViewState& v = c->view;
    out->ms_view = v.ms;
    out->ms_pack = v.ms_pack;
    out->ms_view_bind = v.ms_bind;
    if (!v.bound) return 0;
    out->view_slots = v.vdi.S;
    out->view_overlaps = v.overlaps;
    float ms_count = 0.0f;   // (a dense bind counts its entries when they are first asked for)
    if (int rc = pack_count_bound(c, &ms_count, "insitu_get_stats")) return rc;
    ViewLayoutSize sz{};
    const bool ok = v.vdi.loc ? view_compact_size(v.vdi.W, v.vdi.H, v.vdi.S, v.pk_E, &sz)
                              : view_dense_size(v.vdi.W, v.vdi.H, v.vdi.S, &sz);
    out->view_entries = (long long)v.pk_E;
    out->view_bytes = ok ? (long long)sz.bytes : 0;
    out->view_compact = v.vdi.loc ? 1 : 0;
    return 0;
}
