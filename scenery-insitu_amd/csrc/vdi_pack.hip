// vdi_pack.hip -- the packed VDI stream for gfx950 (stands in for the compressed VDI the
// reference publishes to a remote viewer, VolumeFromFileExample.kt:907-1030).
//
// The view layout (ViewVdi: S slots per pixel, a count per pixel) <-> the stream's sections (the stored entries
// alone, pixel by pixel in row-major order, each list first to last; vdi_pack_format.h).  A pixel's first entry
// index is the exclusive prefix sum of the counts:
//   pack_count_kernel  per block of 256 pixels the sum of its counts and the largest one;
//   pack_scan_kernel   one wave scans the block sums, 64 per step with a carry; the carry left over is E;
//   vdi_pack_kernel / vdi_unpack_kernel: a wave owns 64 consecutive pixels, their prefix sums by __shfl_up; the
//     pixels' entries are one contiguous run of the sections, which the wave copies cooperatively -- lane l
//     takes entries l, l + 64, ... of the run and finds each one's pixel by a binary search over the wave's 64
//     prefix values (256 B of LDS) -- so every section access of a wave is one contiguous piece (1 KiB of
//     float colour) and the accesses to one list are contiguous too.
//   pack_count_set_kernel / pack_scan_set_kernel: the two offset passes over every stream of a set of packed
//     streams in one launch each (insitu_view_bind_packed_set).
// No atomics anywhere: the order of the bytes is a function of the counts alone.
// The compact view layout (ViewVdi with loc) holds its entries in the sections' order already:
// pack_count_kernel also leaves every pixel's offset inside its block (loc), the FLOAT stream is copied to and from
// the layout's arrays as it is, and pack_convert_kernel converts the HALF colours element by element.
#include "insitu_device.h"
#include "insitu_kernels.h"
#include "vdi_pack_format.h"

#pragma clang fp contract(off)

namespace insitu {

namespace {

constexpr uint32_t kSumMask = 0x00ffffffu;   // PackOffsets::bstat: the sum (<= 256 * 255) below the largest count

// inclusive prefix sum over the wave's 64 lanes
__device__ __forceinline__ uint32_t wave_scan(uint32_t v, int lane) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t t = __shfl_up(v, d);
        if (lane >= d) v += t;
    }
    return v;
}

__device__ __forceinline__ uint32_t wave_max(uint32_t m) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const uint32_t v = __shfl_xor(m, o);
        m = v > m ? v : m;
    }
    return m;
}

// the two offset passes, over one VDI's counts (pack_count_kernel, pack_scan_kernel) or a stream of a set's
__device__ __forceinline__ void pack_count_block(const PackOffsets& P) {
    __shared__ uint32_t s_sum[4], s_max[4];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const uint32_t p = blockIdx.x * (uint32_t)kPackBlockPx + threadIdx.x;
    const uint32_t n = p < P.px ? (uint32_t)P.cnt[p] : 0u;
    const uint32_t sum = wave_scan(n, lane), mx = wave_max(n);
    if (lane == 63) {
        s_sum[wave] = sum;
        s_max[wave] = mx;
    }
    __syncthreads();
    if (P.loc && p < P.px) {   // the entries of the block before this pixel (at most 255 x 255: 16 bits hold it)
        uint32_t before = sum - n;
        for (int w = 0; w < wave; ++w) before += s_sum[w];
        P.loc[p] = (uint16_t)before;
    }
    if (threadIdx.x == 0) {
        const uint32_t a = s_max[0] > s_max[1] ? s_max[0] : s_max[1], b = s_max[2] > s_max[3] ? s_max[2] : s_max[3];
        P.bstat[blockIdx.x] = (s_sum[0] + s_sum[1] + s_sum[2] + s_sum[3]) | ((a > b ? a : b) << 24);
    }
}

// One wave.  Four steps' block sums are loaded together (their latencies overlap); each step is a 64-wide scan.
__device__ __forceinline__ void pack_scan_wave(const PackOffsets& P, uint32_t S, int check_E, unsigned long long expect_E) {
    const int lane = threadIdx.x;
    unsigned long long carry = 0;
    uint32_t mx = 0;
    for (uint32_t base = 0; base < P.nblocks; base += 256u) {
        uint32_t v[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const uint32_t b = base + 64u * k + lane;
            v[k] = b < P.nblocks ? P.bstat[b] : 0u;
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const uint32_t b = base + 64u * k + lane, sum = v[k] & kSumMask;
            mx = (v[k] >> 24) > mx ? (v[k] >> 24) : mx;
            const uint32_t incl = wave_scan(sum, lane);   // (64 * 256 * 255 fits)
            if (b < P.nblocks) P.boff[b] = carry + (unsigned long long)(incl - sum);
            carry += (unsigned long long)__shfl(incl, 63);
        }
    }
    mx = wave_max(mx);
    if (lane == 0) {
        P.totals->E = carry;
        P.totals->max_count = mx;
        P.totals->bad = (mx > S || (check_E && carry != expect_E)) ? 1u : 0u;
    }
}

}  // namespace

__global__ __launch_bounds__(256) void pack_count_kernel(const PackOffsets P) { pack_count_block(P); }

__global__ __launch_bounds__(64) void pack_scan_kernel(const PackOffsets P, uint32_t S, int check_E,
                                                       unsigned long long expect_E) {
    pack_scan_wave(P, S, check_E, expect_E);
}

// The same over every stream of a set in one launch each: blockIdx.y, and the scan's one wave per block, pick the
// stream; its S and E are the header's, and the counts must add up to E (insitu_view_bind_packed_set).
__global__ __launch_bounds__(256) void pack_count_set_kernel(const PackedStream* set) {
    const PackOffsets P = set[blockIdx.y].off;
    pack_count_block(P);
}

__global__ __launch_bounds__(64) void pack_scan_set_kernel(const PackedStream* set) {
    const PackedStream s = set[blockIdx.x];
    pack_scan_wave(s.off, s.S, 1, s.E);
}

namespace {

// The cooperative copy both directions share: move(e, v) for every stored entry of the wave's 64 pixels, e its
// index in the sections and v its index in the view layout; consecutive lanes get consecutive e.
template <class Move>
__device__ __forceinline__ void for_each_entry(const PackParams& P, uint32_t (*s_incl)[64], uint32_t* s_tot, Move&& move) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const uint32_t S = (uint32_t)P.vdi.S, px = (uint32_t)P.vdi.W * (uint32_t)P.vdi.H;
    const uint32_t p0 = blockIdx.x * (uint32_t)kPackBlockPx + (uint32_t)wave * 64u, p = p0 + (uint32_t)lane;
    uint32_t n = p < px ? (uint32_t)P.vdi.cnt[p] : 0u;
    n = n < S ? n : S;   // (a count is never above S here; should one be, it must not become an address)
    const uint32_t incl = wave_scan(n, lane);
    s_incl[wave][lane] = incl;
    if (lane == 63) s_tot[wave] = incl;
    __syncthreads();   // (every wave of the block gets here: a wave past the last pixel has n = 0)
    unsigned long long base = P.boff[blockIdx.x];
    for (int w = 0; w < wave; ++w) base += (unsigned long long)s_tot[w];
    const uint32_t total = s_tot[wave];
    const uint32_t* pre = s_incl[wave];
    for (uint32_t k = (uint32_t)lane; k < total; k += 64u) {
        uint32_t j = 0;   // the pixel of entry k of the run: the number of prefix values <= k (at most 63, k < total)
#pragma unroll
        for (uint32_t step = 32u; step > 0u; step >>= 1)
            if (pre[j + step - 1u] <= k) j += step;
        const uint32_t i = k - (j ? pre[j - 1u] : 0u);
        move((size_t)(base + k), (size_t)(p0 + j) * (size_t)S + (size_t)i);
    }
}

__device__ __forceinline__ uint32_t half2_of(float a, float b) {
    return (uint32_t)half_from_float_bits(__float_as_uint(a)) | ((uint32_t)half_from_float_bits(__float_as_uint(b)) << 16);
}
__device__ __forceinline__ float float_of_half(uint32_t h) { return __uint_as_float(float_bits_from_half((uint16_t)h)); }

}  // namespace

template <bool HALF>
__global__ __launch_bounds__(256) void vdi_pack_kernel(const PackParams P) {
    __shared__ uint32_t s_incl[4][64], s_tot[4];
    for_each_entry(P, s_incl, s_tot, [&](size_t e, size_t v) {
        P.dep[e] = P.vdi.dep[v];
        const float4 c = P.vdi.col[v];
        if constexpr (HALF) static_cast<uint2*>(P.col)[e] = make_uint2(half2_of(c.x, c.y), half2_of(c.z, c.w));
        else static_cast<float4*>(P.col)[e] = c;
    });
}

template <bool HALF>
__global__ __launch_bounds__(256) void vdi_unpack_kernel(const PackParams P) {
    __shared__ uint32_t s_incl[4][64], s_tot[4];
    for_each_entry(P, s_incl, s_tot, [&](size_t e, size_t v) {
        P.vdi.dep[v] = P.dep[e];
        if constexpr (HALF) {
            const uint2 h = static_cast<const uint2*>(P.col)[e];
            P.vdi.col[v] = make_float4(float_of_half(h.x & 0xffffu), float_of_half(h.x >> 16), float_of_half(h.y & 0xffffu),
                                       float_of_half(h.y >> 16));
        } else {
            P.vdi.col[v] = static_cast<const float4*>(P.col)[e];
        }
    });
}

// per 8x8-pixel tile the largest count, as view_build_kernel leaves it (one wave per tile)
__global__ __launch_bounds__(256) void view_tmax_kernel(const ViewVdi V) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int tile = (int)blockIdx.x * 4 + wave;
    if (tile >= V.tiles_x * V.tiles_y) return;   // wave-uniform
    const int ty = tile / V.tiles_x, tx = tile - ty * V.tiles_x;
    const int x = tx * 8 + (lane & 7), y = ty * 8 + (lane >> 3);
    const uint32_t n = (x < V.W && y < V.H) ? (uint32_t)V.cnt[(size_t)y * (size_t)V.W + (size_t)x] : 0u;
    const uint32_t m = wave_max(n);
    if (lane == 0) V.tmax[tile] = (uint8_t)m;
}

// The compact view layout against the HALF stream: colour e of the one is colour e of the other.
template <bool TO_HALF>
__global__ __launch_bounds__(256) void pack_convert_kernel(const void* src, void* dst, unsigned long long n) {
    const unsigned long long e = (unsigned long long)blockIdx.x * 256ull + (unsigned long long)threadIdx.x;
    if (e >= n) return;
    if constexpr (TO_HALF) {
        const float4 c = static_cast<const float4*>(src)[e];
        static_cast<uint2*>(dst)[e] = make_uint2(half2_of(c.x, c.y), half2_of(c.z, c.w));
    } else {
        const uint2 h = static_cast<const uint2*>(src)[e];
        static_cast<float4*>(dst)[e] = make_float4(float_of_half(h.x & 0xffffu), float_of_half(h.x >> 16),
                                                   float_of_half(h.y & 0xffffu), float_of_half(h.y >> 16));
    }
}

hipError_t launch_pack_convert(const void* src, void* dst, unsigned long long n, int to_half, hipStream_t s) {
    if (n == 0) return hipSuccess;
    const unsigned long long blocks = (n + 255ull) / 256ull;
    if (!src || !dst || blocks > 0x7fffffffull) return hipErrorInvalidValue;
    if (to_half) hipLaunchKernelGGL(pack_convert_kernel<true>, dim3((unsigned)blocks), dim3(256), 0, s, src, dst, n);
    else hipLaunchKernelGGL(pack_convert_kernel<false>, dim3((unsigned)blocks), dim3(256), 0, s, src, dst, n);
    return hipGetLastError();
}

hipError_t launch_view_tmax(const ViewVdi& v, hipStream_t s) {
    const int tiles = v.tiles_x * v.tiles_y;
    if (tiles <= 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(view_tmax_kernel, dim3((unsigned)((tiles + 3) / 4)), dim3(256), 0, s, v);
    return hipGetLastError();
}

hipError_t launch_pack_offsets(const PackOffsets& o, int S, int check_E, unsigned long long expect_E, hipStream_t s) {
    if (o.px == 0 || S < 1 || S > 255 || o.nblocks != (o.px + (uint32_t)kPackBlockPx - 1u) / (uint32_t)kPackBlockPx)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(pack_count_kernel, dim3(o.nblocks), dim3(256), 0, s, o);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(pack_scan_kernel, dim3(1), dim3(64), 0, s, o, (uint32_t)S, check_E, expect_E);
    return hipGetLastError();
}

hipError_t launch_pack_offsets_set(const PackedStream* set, int n, uint32_t px, uint32_t nblocks, hipStream_t s) {
    if (!set || n < 1 || n > kMaxLists || px == 0 || nblocks != (px + (uint32_t)kPackBlockPx - 1u) / (uint32_t)kPackBlockPx)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(pack_count_set_kernel, dim3(nblocks, (unsigned)n), dim3(256), 0, s, set);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(pack_scan_set_kernel, dim3((unsigned)n), dim3(64), 0, s, set);
    return hipGetLastError();
}

namespace {
bool pack_params_ok(const PackParams& p) {
    const ViewVdi& v = p.vdi;
    // (the cooperative copies address the dense layout; a compact one is the sections already)
    return !v.loc && v.W > 0 && v.H > 0 && v.S >= 1 && v.S <= 255 && (uint64_t)v.W * (uint64_t)v.H <= kPackMaxPixels;
}
unsigned pack_blocks(const PackParams& p) {
    const uint32_t px = (uint32_t)p.vdi.W * (uint32_t)p.vdi.H;
    return (px + (uint32_t)kPackBlockPx - 1u) / (uint32_t)kPackBlockPx;
}
}  // namespace

hipError_t launch_vdi_pack(const PackParams& p, hipStream_t s) {
    if (!pack_params_ok(p)) return hipErrorInvalidValue;
    if (p.half) hipLaunchKernelGGL(vdi_pack_kernel<true>, dim3(pack_blocks(p)), dim3(256), 0, s, p);
    else hipLaunchKernelGGL(vdi_pack_kernel<false>, dim3(pack_blocks(p)), dim3(256), 0, s, p);
    return hipGetLastError();
}

hipError_t launch_vdi_unpack(const PackParams& p, hipStream_t s) {
    if (!pack_params_ok(p)) return hipErrorInvalidValue;
    if (p.half) hipLaunchKernelGGL(vdi_unpack_kernel<true>, dim3(pack_blocks(p)), dim3(256), 0, s, p);
    else hipLaunchKernelGGL(vdi_unpack_kernel<false>, dim3(pack_blocks(p)), dim3(256), 0, s, p);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    return launch_view_tmax(p.vdi, s);
}

}  // namespace insitu
