// vdi_view_source.h -- where the lists of a ViewSource lie (insitu_kernels.h), shared by view_build_kernel
// (vdi_view.hip) and the merge kernels (vdi_view_merge.hip), and where those of a set of packed streams lie
// (PackedSource), which the merge kernels read through the same few functions.  Every product in 64 bits.
#pragma once
#include "insitu_kernels.h"
#include "vdi_pack_format.h"

namespace insitu {

// Entry k of list j of one pixel at col/dep[e0 + j*lstride + k*estride]
struct ViewAt {
    size_t e0, lstride, estride;
};

// (x, y) inside the W x H window of lists of S slots
__device__ __forceinline__ ViewAt view_at(const ViewSource& P, int x, int y, int H, int S) {
    ViewAt a;
    if (P.reference) {
        a.e0 = ((size_t)x * (size_t)H + (size_t)y) * (size_t)S;
        a.lstride = P.ref_stride;
        a.estride = 1;
    } else {
        const int d = x / P.strip_w, xl = x - d * P.strip_w, xt = xl >> 3, xx = xl & 7;
        const size_t blockE = (size_t)P.strip_tiles * (size_t)S * (size_t)H * 8;
        a.e0 = ((size_t)d * (size_t)P.B + (size_t)P.b) * blockE + ((size_t)xt * (size_t)S * (size_t)H + (size_t)y) * 8 + (size_t)xx;
        a.lstride = blockE;
        a.estride = (size_t)H * 8;
    }
    return a;
}

// the slots of list j of the pixel that may hold entries: the stored count, or all S in the reference layout
__device__ __forceinline__ int view_slots(const ViewSource& P, int j, int x, int y, int S) {
    if (P.reference) return S;
    const int d = x / P.strip_w, xl = x - d * P.strip_w;
    const int stored = (int)(P.cnt[(size_t)(P.b + j) * P.cnt_stride + (size_t)d * P.cnt_dstride + (size_t)y * P.cnt_pitch + (size_t)xl] & kPendingCount);
    return stored < S ? stored : S;   // (a corrupt count must not walk past the S slots)
}

// ---- what the merge kernels walk: a ViewSource, or a set of packed streams (PackedSource) ----
// src_at(P, x, y, W, H, S) is the pixel, src_slots(P, at, j, x, y, S) the slots of its list j that may hold entries,
// src_list(P, at, j) that list as a run: entry k at index run.e0 + k * run.estride, read by run_dep and run_col.

struct ViewRun {
    const float2* dep;
    const float4* col;
    size_t e0, estride;
};

__device__ __forceinline__ ViewAt src_at(const ViewSource& P, int x, int y, int, int H, int S) { return view_at(P, x, y, H, S); }
__device__ __forceinline__ int src_slots(const ViewSource& P, const ViewAt&, int j, int x, int y, int S) {
    return view_slots(P, j, x, y, S);
}
__device__ __forceinline__ ViewRun src_list(const ViewSource& P, const ViewAt& at, int j) {
    return {P.dep, P.col, at.e0 + (size_t)j * at.lstride, at.estride};
}
__device__ __forceinline__ float2 run_dep(const ViewRun& r, size_t e) { return r.dep[e]; }
__device__ __forceinline__ float4 run_col(const ViewRun& r, size_t e) { return r.col[e]; }

// A packed stream holds its stored entries alone, so a list is found through the stream's own offsets (the compact
// view layout's addressing, view_list_at) and its entries are neighbours.  Nothing of a stream is kept per lane
// but what the merge keeps of any list: the run is derived again from the table whenever an entry is taken.
struct PackedAt {
    size_t p;   // y*W + x
};
struct PackedRun {
    const float2* dep;
    const void* col;
    size_t e0;
    static constexpr size_t estride = 1;
    uint32_t half;
};

__device__ __forceinline__ PackedAt src_at(const PackedSource& P, int x, int y, int, int, int) {
    return {(size_t)y * (size_t)P.W + (size_t)x};
}
__device__ __forceinline__ int src_slots(const PackedSource& P, const PackedAt& at, int j, int, int, int) {
    const PackedStream& s = P.streams[j];
    const int stored = (int)s.off.cnt[at.p], S = (int)s.S;
    return stored < S ? stored : S;   // (validated before the merge runs; a count must not become an address all the same)
}
__device__ __forceinline__ PackedRun src_list(const PackedSource& P, const PackedAt& at, int j) {
    const PackedStream& s = P.streams[j];
    return {s.dep, s.col, (size_t)s.off.boff[at.p >> 8] + (size_t)s.off.loc[at.p], s.half};
}
__device__ __forceinline__ float2 run_dep(const PackedRun& r, size_t e) { return r.dep[e]; }
__device__ __forceinline__ float4 run_col(const PackedRun& r, size_t e) {
    if (!r.half) return static_cast<const float4*>(r.col)[e];
    const uint2 h = static_cast<const uint2*>(r.col)[e];
    return make_float4(__uint_as_float(float_bits_from_half((uint16_t)(h.x & 0xffffu))),
                       __uint_as_float(float_bits_from_half((uint16_t)(h.x >> 16))),
                       __uint_as_float(float_bits_from_half((uint16_t)(h.y & 0xffffu))),
                       __uint_as_float(float_bits_from_half((uint16_t)(h.y >> 16))));
}

// the start depth of the first entry of list j (which has one)
template <class SRC, class AT>
__device__ __forceinline__ float src_front(const SRC& P, const AT& at, int j) {
    const auto run = src_list(P, at, j);
    return run_dep(run, run.e0).x;
}

}  // namespace insitu
