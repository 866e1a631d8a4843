// vdi_view_merge.hip -- the merged bind of the novel-view renderer for gfx950.
//
// All sub-VDIs of a frame share one generating camera and one pixel grid, and the flatten compositor defines how
// their lists combine: the k-way merge by start depth of determineNextSupseg (VDICompositor.comp:58-91,
// vdi_flatten_kernel in composite.hip).  The merged per-pixel list is itself a VDI, so vdi_view_kernel and the
// packed stream work on it unchanged.  Entries are copied bit for bit: no float arithmetic, only comparisons.
// view_merge_count_kernel: per pixel the sum of the lists' lengths, the largest of them over the window (the
// slots the merged VDI needs).
// view_merge_kernel: the merge into the view layout (ViewVdi) -- entries, counts, the tiles' largest count -- and
// the number of adjacent merged entries that overlap in depth.
// Both: one lane per VDI pixel, one wave per 8x8 tile, as view_build_kernel.
// For the compact view layout the count kernel also stores every pixel's merged length as its
// count, the offset passes of vdi_pack.hip run between the two kernels, and the merge writes each list where
// view_list_at puts it.
// Both kernels take their lists from a ViewSource or, the same loop instantiated again, from a PackedSource: the
// staged streams of insitu_view_bind_packed_set, read in place through each stream's own
// offsets; vdi_view_source.h holds what differs between the two.
#include "insitu_device.h"
#include "insitu_kernels.h"
#include "vdi_view_source.h"

#pragma clang fp contract(off)

namespace insitu {

namespace {

__device__ __forceinline__ int wave_max(int m) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const int v = __shfl_xor(m, o);
        m = v > m ? v : m;
    }
    return m;
}

}  // namespace

// SRC: ViewSource, or PackedSource (the lists of a set of packed streams); vdi_view_source.h has what differs.
template <class SRC>
__global__ __launch_bounds__(256) void view_merge_count_kernel(const SRC P, const int W, const int H, const int S,
                                                               MergeTotals* tot, uint8_t* cnt) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int tiles_x = (W + 7) >> 3, tiles_y = (H + 7) >> 3;
    const int tile = (int)blockIdx.x * 4 + wave;
    if (tile >= tiles_x * tiles_y) return;   // wave-uniform
    const int ty = tile / tiles_x, tx = tile - ty * tiles_x;
    const int x = tx * 8 + (lane & 7), y = ty * 8 + (lane >> 3);
    int m = 0;
    if (x < W && y < H) {
        const auto at = src_at(P, x, y, W, H, S);
        int taken = 0;   // the entries the merge takes: a list also ends at a start the merge never picks (not < 100000)
        for (int j = 0; j < P.n; ++j) {
            const int slots = src_slots(P, at, j, x, y, S);
            const auto run = src_list(P, at, j);
            int c = 0, t = -1;
            for (; c < slots; ++c) {
                const float start = run_dep(run, run.e0 + (size_t)c * run.estride).x;
                if (start == 0.0f) break;
                if (t < 0 && !(start < 100000.0f)) t = c;
            }
            m += c;
            taken += t < 0 ? c : t;
        }
        // the compact bind: the merged list's length is the pixel's count (more than 255 anywhere rejects the bind)
        if (cnt) cnt[(size_t)y * (size_t)W + (size_t)x] = (uint8_t)(taken < 255 ? taken : 255);
    }
    m = wave_max(m);
    if (lane == 0 && m > 0) atomicMax(&tot->max_count, (uint32_t)m);
}

// The fronts, as vdi_flatten_kernel holds them: per list the start depth at its front (0 = exhausted or empty), and
// the entries left in the list (the front included) | the entries taken from it << 16.  Up to 8 lists they live in
// registers (every access unrolled over the lists); beyond that the compiler spills them (VMAX = 32: 2052 bytes
// of scratch per lane), so they live in LDS, one column per lane ([list][lane of the block]: no bank conflicts on
// the scan, no barrier -- a lane touches its own column only), and the scan runs over the n lists there are.
template <int VMAX, class SRC>
__global__ __launch_bounds__(256) void view_merge_kernel(const SRC P, const int S, const ViewVdi V, MergeTotals* tot) {
    constexpr bool kLds = VMAX > 8;
    __shared__ float lfs[kLds ? VMAX * 256 : 1];
    __shared__ uint32_t lst[kLds ? VMAX * 256 : 1];
    const int tid = (int)threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int tile = (int)blockIdx.x * 4 + wave;
    if (tile >= V.tiles_x * V.tiles_y) return;   // wave-uniform
    const int ty = tile / V.tiles_x, tx = tile - ty * V.tiles_x;
    const int x = tx * 8 + (lane & 7), y = ty * 8 + (lane >> 3);
    const int H = V.H, Sm = V.S, n = P.n < VMAX ? P.n : VMAX;
    int m = 0;
    uint32_t overlaps = 0;
    if (x < V.W && y < H) {
        const auto at = src_at(P, x, y, V.W, H, S);
        float fs[kLds ? 1 : VMAX];
        uint32_t st[kLds ? 1 : VMAX];
        auto front_of = [&](int j, float& f, uint32_t& left) {
            const int slots = src_slots(P, at, j, x, y, S);
            left = (uint32_t)slots;
            f = slots > 0 ? src_front(P, at, j) : 0.0f;
        };
        if constexpr (kLds) {
            for (int j = 0; j < n; ++j) front_of(j, lfs[j * 256 + tid], lst[j * 256 + tid]);
        } else {
#pragma unroll
            for (int j = 0; j < VMAX; ++j) {
                fs[j] = 0.0f;
                st[j] = 0u;
                if (j < n) front_of(j, fs[j], st[j]);
            }
        }
        const size_t p = (size_t)y * (size_t)V.W + (size_t)x;
        const size_t o = view_list_at(V, p);
        // (the count kernel sized Sm, and a compact list's own room: the bound never cuts a list short)
        const int room = V.loc ? ((int)V.cnt[p] < Sm ? (int)V.cnt[p] : Sm) : Sm;
        float prev_end = 0.0f;
        while (m < room) {
            // determineNextSupseg (VDICompositor.comp:58-91): smallest non-zero front start, lowest index on ties
            float low = 100000.0f;
            int idx = -1;
            uint32_t s = 0u;
            if constexpr (kLds) {
                for (int j = 0; j < n; ++j) {
                    const float c = lfs[j * 256 + tid];
                    if (c < low && c != 0.0f) { low = c; idx = j; }
                }
                if (idx < 0) break;
                s = lst[idx * 256 + tid];
            } else {
#pragma unroll
                for (int j = 0; j < VMAX; ++j) {
                    const float c = fs[j];
                    if (c < low && c != 0.0f) { low = c; idx = j; }
                }
                if (idx < 0) break;
#pragma unroll
                for (int j = 0; j < VMAX; ++j)
                    if (j == idx) s = st[j];
            }
            const uint32_t left = s & 0xffffu, taken = s >> 16;
            const auto run = src_list(P, at, idx);
            const size_t e = run.e0 + (size_t)taken * run.estride;
            const float2 se = run_dep(run, e);
            const float4 colour = run_col(run, e);
            // advance that list
            const float nxt = left > 1u ? run_dep(run, e + run.estride).x : 0.0f;
            const uint32_t ns = (left - 1u) | ((taken + 1u) << 16);
            if constexpr (kLds) {
                lfs[idx * 256 + tid] = nxt;
                lst[idx * 256 + tid] = ns;
            } else {
#pragma unroll
                for (int j = 0; j < VMAX; ++j)
                    if (j == idx) { st[j] = ns; fs[j] = nxt; }
            }
            if (m > 0 && se.x < prev_end) ++overlaps;
            prev_end = se.y;
            V.col[o + (size_t)m] = colour;
            V.dep[o + (size_t)m] = se;
            ++m;
        }
        if (!V.loc) V.cnt[p] = (uint8_t)m;   // (compact: the offsets stand on the count kernel's counts)
    }
    const int mx = wave_max(m);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) overlaps += __shfl_xor(overlaps, o);
    if (lane == 0) {
        V.tmax[tile] = (uint8_t)mx;
        if (overlaps) atomicAdd(&tot->overlaps, (unsigned long long)overlaps);
    }
}

namespace {

// blocks of 4 waves over the 8x8 tiles of a W x H window; 0 when they do not fit a launch
unsigned merge_blocks(int W, int H) {
    if (W <= 0 || H <= 0) return 0;
    const long long tiles = (long long)((W + 7) / 8) * (long long)((H + 7) / 8);
    if (tiles > 0x7fffffffLL / 4) return 0;
    return (unsigned)((tiles + 3) / 4);
}

template <class SRC>
hipError_t merge_count_launch(const SRC& src, int W, int H, int S, MergeTotals* tot, uint8_t* cnt, hipStream_t s) {
    const unsigned blocks = merge_blocks(W, H);
    if (!blocks || S <= 0 || src.n < 1 || src.n > kMaxLists) return hipErrorInvalidValue;
    hipError_t e = hipMemsetAsync(tot, 0, sizeof(MergeTotals), s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(view_merge_count_kernel<SRC>, dim3(blocks), dim3(256), 0, s, src, W, H, S, tot, cnt);
    return hipGetLastError();
}

template <class SRC>
hipError_t merge_launch(const SRC& src, int S, const ViewVdi& dst, MergeTotals* tot, hipStream_t s) {
    const unsigned blocks = merge_blocks(dst.W, dst.H);
    if (!blocks || S <= 0 || dst.S <= 0 || dst.S > 255 || src.n < 1 || src.n > kMaxLists || (dst.loc && !dst.boff))
        return hipErrorInvalidValue;
    hipError_t e = hipMemsetAsync(&tot->overlaps, 0, sizeof tot->overlaps, s);
    if (e != hipSuccess) return e;
    if (src.n <= 8) hipLaunchKernelGGL((view_merge_kernel<8, SRC>), dim3(blocks), dim3(256), 0, s, src, S, dst, tot);
    else if (src.n <= 16) hipLaunchKernelGGL((view_merge_kernel<16, SRC>), dim3(blocks), dim3(256), 0, s, src, S, dst, tot);
    else hipLaunchKernelGGL((view_merge_kernel<kMaxLists, SRC>), dim3(blocks), dim3(256), 0, s, src, S, dst, tot);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_view_merge_count(const ViewSource& src, int W, int H, int S, MergeTotals* tot, uint8_t* cnt,
                                   hipStream_t s) {
    return merge_count_launch(src, W, H, S, tot, cnt, s);
}
hipError_t launch_view_merge_count(const PackedSource& src, int W, int H, int S, MergeTotals* tot, uint8_t* cnt,
                                   hipStream_t s) {
    if (!src.streams || src.W != W) return hipErrorInvalidValue;
    return merge_count_launch(src, W, H, S, tot, cnt, s);
}

hipError_t launch_view_merge(const ViewSource& src, int S, const ViewVdi& dst, MergeTotals* tot, hipStream_t s) {
    return merge_launch(src, S, dst, tot, s);
}
hipError_t launch_view_merge(const PackedSource& src, int S, const ViewVdi& dst, MergeTotals* tot, hipStream_t s) {
    if (!src.streams || src.W != dst.W) return hipErrorInvalidValue;
    return merge_launch(src, S, dst, tot, s);
}

}  // namespace insitu
