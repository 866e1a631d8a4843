// vdi_view_layout.h -- the size arithmetic of the two view layouts of a bound VDI (ViewVdi, insitu_kernels.h;
// DESIGN.md sections 9 and 9.7).  Plain C++ with no HIP in it (tests/view_compact_host.cpp runs it under the
// sanitizers).  Every product is in 64 bits with its operands bounded first: W, H, S and E may be anything their
// types can hold.
//
// Dense:   S slots per pixel, entry i of pixel p at p*S + i:
//            bytes = 24*W*H*S + W*H + tiles
// Compact: the E stored entries alone, entry i of pixel p at boff[p >> 8] + loc[p] + i:
//            bytes = 24*max(E,1) + 3*W*H + 8*nblocks + tiles
// with 24 = a float4 colour + a float2 depth pair per entry, tiles = ceil(W/8)*ceil(H/8) (one byte each, the
// largest count), nblocks = ceil(W*H/256) (one 64-bit entry offset each), and per pixel a count byte and, compact,
// the 16-bit offset inside its block (at most 255 pixels x 255 entries = 65 025 before a block's last pixel).
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace insitu {

constexpr uint64_t kViewMaxPixels = 1ull << 30;   // kPackMaxPixels: pixel indices stay 32-bit
constexpr uint32_t kViewBlockPx = 256;            // kPackBlockPx: pixels per offset block
constexpr uint32_t kViewMaxSlots = 255;           // counts are bytes
constexpr uint64_t kViewEntryBytes = 24;
constexpr uint32_t kViewMaxLoc = (kViewBlockPx - 1u) * kViewMaxSlots;   // 65 025: fits the u16 of loc

struct ViewLayoutSize {
    uint64_t px;        // W*H
    uint64_t tiles;     // ceil(W/8)*ceil(H/8)
    uint64_t nblocks;   // ceil(px/256); 0 in the dense layout's sizes
    uint64_t entries;   // entries the layout holds room for: W*H*S, or max(E,1)
    uint64_t bytes;     // device bytes of the layout
};

// W, H > 0 and W*H <= 2^30; then px and tiles (no product can overflow: 32 x 32 bits, and tiles <= px)
inline bool view_pixels(int W, int H, ViewLayoutSize* out) {
    if (W <= 0 || H <= 0) return false;
    const uint64_t px = (uint64_t)(uint32_t)W * (uint64_t)(uint32_t)H;   // (< 2^62)
    if (px > kViewMaxPixels) return false;
    out->px = px;
    out->tiles = (((uint64_t)(uint32_t)W + 7u) >> 3) * (((uint64_t)(uint32_t)H + 7u) >> 3);
    out->nblocks = 0;
    return true;
}

// blocks of kViewBlockPx pixels over px <= 2^30 pixels (<= 2^22)
inline uint64_t view_blocks(uint64_t px) { return (px + (uint64_t)kViewBlockPx - 1u) / (uint64_t)kViewBlockPx; }

// the dense layout of (W, H, S); false when a dimension is out of range
inline bool view_dense_size(int W, int H, int S, ViewLayoutSize* out) {
    if (S < 1 || (uint32_t)S > kViewMaxSlots) return false;
    if (!view_pixels(W, H, out)) return false;
    out->entries = out->px * (uint64_t)S;                                    // (< 2^38)
    out->bytes = kViewEntryBytes * out->entries + out->px + out->tiles;      // (< 2^43)
    return true;
}

// the compact layout of E entries over (W, H) lists of at most S entries; false when a dimension is out of range or
// E exceeds what W*H lists of S entries can hold
inline bool view_compact_size(int W, int H, int S, uint64_t E, ViewLayoutSize* out) {
    if (S < 1 || (uint32_t)S > kViewMaxSlots) return false;
    if (!view_pixels(W, H, out)) return false;
    if (E > out->px * (uint64_t)S) return false;                             // (bounds E below 2^38)
    out->nblocks = view_blocks(out->px);
    out->entries = E > 0 ? E : 1;
    out->bytes = kViewEntryBytes * out->entries + 3u * out->px + 8u * out->nblocks + out->tiles;
    return true;
}

}  // namespace insitu
