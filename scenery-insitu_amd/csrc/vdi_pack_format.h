// vdi_pack_format.h -- the packed VDI stream, format version 1: its header, the size
// arithmetic and the binary16 conversions.  Plain C++ with no HIP in it, so that the parsing of bytes that come from
// outside the process compiles for the CPU alone (tests/pack_format_host.cpp runs it under the sanitizers); the
// kernels of vdi_pack.hip use the same conversions on the device.
//
// Stream (little-endian, as the host is): 128-byte header | W*H u8 counts, row-major (y*W + x), zero-padded to a
// multiple of 16 | E x {start, end} float32 | E x rgba (float32, or binary16 in INSITU_PACK_HALF) -- entries pixel
// by pixel in the counts' order, each list first entry to last; nothing follows.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#define INSITU_HD __host__ __device__
#else
#define INSITU_HD
#endif

namespace insitu {

constexpr size_t kPackHeaderBytes = 128;
constexpr uint32_t kPackVersion = 1;
constexpr uint32_t kPackFloat = 0, kPackHalf = 1;   // enum insitu_pack_format
constexpr unsigned char kPackMagic[4] = {'I', 'V', 'D', 'P'};
constexpr uint64_t kPackMaxPixels = 1ull << 30;   // (pixel indices and grid sizes stay 32-bit; entry indices are 64-bit)

struct PackHeader {
    uint32_t format, W, H, S;
    uint64_t E;          // stored entries
    float pv_g[16];      // proj * view of the generating camera, column-major (ViewState::pv_g)
};

// byte offsets of the sections in the stream and its size
struct PackLayout {
    uint64_t px;                            // W*H
    size_t depth_off, colour_off, total;    // (the counts are at kPackHeaderBytes)
    size_t depth_bytes, colour_bytes;
};

// The layout of a stream of these dimensions; false when a dimension is out of range, E exceeds the S slots of
// every pixel, or a size does not fit (every product is checked: W, H and E may be anything a header can hold).
inline bool pack_layout(uint32_t format, uint32_t W, uint32_t H, uint32_t S, uint64_t E, PackLayout* out) {
    if (format != kPackFloat && format != kPackHalf) return false;
    if (W == 0 || H == 0 || S < 1 || S > 255) return false;
    const uint64_t px = (uint64_t)W * (uint64_t)H;   // (32 x 32 bits: no overflow)
    if (px > kPackMaxPixels) return false;
    if (E > px * (uint64_t)S) return false;          // (< 2^38)
    const uint64_t counts = (px + 15u) & ~(uint64_t)15u;
    const uint64_t dep = E * 8u, col = E * (format == kPackHalf ? 8u : 16u);   // (< 2^42)
    const uint64_t total = (uint64_t)kPackHeaderBytes + counts + dep + col;
    if (total > (uint64_t)SIZE_MAX) return false;
    out->px = px;
    out->depth_off = (size_t)(kPackHeaderBytes + counts);
    out->colour_off = (size_t)(kPackHeaderBytes + counts + dep);
    out->total = (size_t)total;
    out->depth_bytes = (size_t)dep;
    out->colour_bytes = (size_t)col;
    return true;
}

inline void pack_write_header(void* out, const PackHeader& h) {
    unsigned char b[kPackHeaderBytes] = {};
    const uint32_t version = kPackVersion;
    memcpy(b, kPackMagic, 4);
    memcpy(b + 4, &version, 4);
    memcpy(b + 8, &h.format, 4);
    memcpy(b + 12, &h.W, 4);
    memcpy(b + 16, &h.H, 4);
    memcpy(b + 20, &h.S, 4);
    memcpy(b + 24, &h.E, 8);
    memcpy(b + 32, h.pv_g, 64);
    memcpy(out, b, sizeof b);
}

// The header of a stream of `bytes` bytes and its layout; null when they are consistent -- magic, version, format,
// W, H > 0, S in 1..255, `bytes` exactly the size the header implies -- else what is wrong.  Reads the first
// kPackHeaderBytes of `data` at most.  The counts are not looked at here: whether each is <= S and they add up to
// E is checked where they are (on the device, before anything is scattered).
inline const char* pack_parse(const void* data, size_t bytes, PackHeader* h, PackLayout* lay) {
    if (!data) return "null stream";
    if (bytes < kPackHeaderBytes) return "shorter than the header";
    const unsigned char* b = static_cast<const unsigned char*>(data);
    if (memcmp(b, kPackMagic, 4) != 0) return "bad magic";
    uint32_t version;
    memcpy(&version, b + 4, 4);
    if (version != kPackVersion) return "unknown version";
    memcpy(&h->format, b + 8, 4);
    memcpy(&h->W, b + 12, 4);
    memcpy(&h->H, b + 16, 4);
    memcpy(&h->S, b + 20, 4);
    memcpy(&h->E, b + 24, 8);
    memcpy(h->pv_g, b + 32, 64);
    if (h->format != kPackFloat && h->format != kPackHalf) return "unknown format";
    if (h->W == 0 || h->H == 0) return "W and H must be > 0";
    if (h->S < 1 || h->S > 255) return "S must be in [1,255]";
    if (!pack_layout(h->format, h->W, h->H, h->S, h->E, lay)) return "dimensions or entry count out of range";
    if (lay->total != bytes) return "size differs from what the header implies";
    return nullptr;
}

// ---- a set of streams, bound as one merged VDI (insitu_view_bind_packed_set) ----
constexpr int kPackSetMax = 32;   // (kMaxLists)

// The headers and layouts of n streams that are to be merged: null when n is 1..kPackSetMax, every stream passes
// pack_parse, and all of them have stream 0's W, H and pv_g (the 64 bytes compared as they are); else what is wrong,
// with *index the stream it is wrong with (-1: the set itself).  S and the format may differ from stream to stream.
// headers and layouts have room for kPackSetMax entries; those before *index are filled in.
inline const char* pack_set_parse(const void* const* streams, const size_t* bytes, int n, PackHeader* headers,
                                  PackLayout* layouts, int* index) {
    *index = -1;
    if (!streams || !bytes) return "null argument";
    if (n < 1 || n > kPackSetMax) return "needs 1 to 32 streams";
    for (int j = 0; j < n; ++j) {
        *index = j;
        if (const char* why = pack_parse(streams[j], bytes[j], &headers[j], &layouts[j])) return why;
        if (headers[j].W != headers[0].W || headers[j].H != headers[0].H) return "W and H differ from stream 0's";
        if (memcmp(headers[j].pv_g, headers[0].pv_g, sizeof headers[j].pv_g) != 0)
            return "the generating camera differs from stream 0's";
    }
    *index = -1;
    return nullptr;
}

// Where the streams of a parsed set lie in their one staging allocation: per stream the counts, the depth section
// and the colour section, each at a multiple of 16 bytes, stream after stream.
struct PackSetStage {
    size_t cnt_at, dep_at, col_at;
};

// false when the staging does not fit a size_t.  (A parsed layout's sections are below 2^43 bytes each, so the sum
// over kPackSetMax streams stays below 2^50: no 64-bit sum wraps.)
inline bool pack_set_stage(const PackLayout* layouts, int n, PackSetStage* at, size_t* total) {
    if (n < 1 || n > kPackSetMax) return false;
    const auto pad16 = [](uint64_t v) { return (v + 15u) & ~(uint64_t)15u; };
    uint64_t off = 0;
    for (int j = 0; j < n; ++j) {
        const uint64_t cnt = pad16(layouts[j].px), dep = pad16((uint64_t)layouts[j].depth_bytes);
        const uint64_t col = pad16((uint64_t)layouts[j].colour_bytes);
        if (off + cnt + dep + col > (uint64_t)SIZE_MAX) return false;
        at[j].cnt_at = (size_t)off;
        at[j].dep_at = (size_t)(off + cnt);
        at[j].col_at = (size_t)(off + cnt + dep);
        off += cnt + dep + col;
    }
    *total = (size_t)off;
    return true;
}

// ---- the headers of a gather (insitu_view_gather_merged) ----
// Before any section moves, the root of a gather holds every rank's header and nothing else of its stream.  A rank
// that cannot take part offers a refusing header instead: zeroed magic, and its reason where the version would be.
// The verdict names one rank and one of these codes on every rank.
enum PackGatherReason : uint32_t {
    kGatherAccepted = 0,
    // a rank's own refusal
    kGatherNothingBound = 1,
    kGatherBadFormatArgument = 2,
    kGatherFrameInFlight = 3,
    kGatherAllocationFailed = 4,
    // what the root finds in a header: pack_parse's reasons ...
    kGatherBadMagic = 5,
    kGatherUnknownVersion = 6,
    kGatherUnknownFormat = 7,
    kGatherZeroWindow = 8,
    kGatherBadSlots = 9,
    kGatherOutOfRange = 10,
    // ... and pack_set_parse's
    kGatherWindowDiffers = 11,
    kGatherCameraDiffers = 12,
    kGatherBadRankCount = 13,
    kGatherRejectedHeader = 14,   // (a reason of pack_parse's that has no code of its own)
    kGatherReasons
};
constexpr uint32_t kGatherLastRefusal = kGatherAllocationFailed;

inline const char* pack_gather_reason_text(uint32_t reason) {
    switch (reason) {
    case kGatherAccepted: return "accepted";
    case kGatherNothingBound: return "no VDI bound (insitu_view_bind first)";
    case kGatherBadFormatArgument: return "bad format argument";
    case kGatherFrameInFlight: return "a pipelined frame is in flight (insitu_pipeline_flush first)";
    case kGatherAllocationFailed: return "a device allocation failed";
    case kGatherBadMagic: return "bad magic";
    case kGatherUnknownVersion: return "unknown version";
    case kGatherUnknownFormat: return "unknown format";
    case kGatherZeroWindow: return "W and H must be > 0";
    case kGatherBadSlots: return "S must be in [1,255]";
    case kGatherOutOfRange: return "dimensions or entry count out of range";
    case kGatherWindowDiffers: return "W and H differ from rank 0's";
    case kGatherCameraDiffers: return "the generating camera differs from rank 0's";
    case kGatherBadRankCount: return "needs 1 to 32 ranks";
    case kGatherRejectedHeader: return "header rejected";
    default: return "unknown reason";
    }
}

inline void pack_write_refusal(void* out, uint32_t reason) {
    unsigned char b[kPackHeaderBytes] = {};
    memcpy(b + 4, &reason, 4);
    memcpy(out, b, sizeof b);
}

// n headers of kPackHeaderBytes each, one behind the other, with no stream bodies: kGatherAccepted when n is
// 1..kPackSetMax, no header refuses, every header passes what pack_parse checks of one -- given the size the header
// itself implies -- and all have header 0's W, H and pv_g (the 64 bytes compared as they are); else the reason, with
// *index the header it lies with (-1: the set itself).  A refusing header is reported with the reason it carries.
// headers_out and layouts have room for kPackSetMax entries; those before *index are filled in.
inline uint32_t pack_header_set_check(const void* headers, int n, PackHeader* headers_out, PackLayout* layouts, int* index) {
    *index = -1;
    if (!headers || n < 1 || n > kPackSetMax) return kGatherBadRankCount;
    const unsigned char* b = static_cast<const unsigned char*>(headers);
    const unsigned char no_magic[4] = {};
    for (int j = 0; j < n; ++j, b += kPackHeaderBytes) {
        *index = j;
        uint32_t word;
        memcpy(&word, b + 4, 4);
        if (memcmp(b, no_magic, 4) == 0 && word >= 1 && word <= kGatherLastRefusal) return word;
        // the size a stream of this header has, where its fields give one (where they do not, pack_parse names the
        // field before it comes to the size)
        PackHeader& h = headers_out[j];
        memcpy(&h.format, b + 8, 4);
        memcpy(&h.W, b + 12, 4);
        memcpy(&h.H, b + 16, 4);
        memcpy(&h.S, b + 20, 4);
        memcpy(&h.E, b + 24, 8);
        const size_t bytes = pack_layout(h.format, h.W, h.H, h.S, h.E, &layouts[j]) ? layouts[j].total : kPackHeaderBytes;
        if (const char* why = pack_parse(b, bytes, &h, &layouts[j])) {
            for (uint32_t r = kGatherBadMagic; r <= kGatherOutOfRange; ++r)
                if (strcmp(why, pack_gather_reason_text(r)) == 0) return r;
            return kGatherRejectedHeader;
        }
        if (h.W != headers_out[0].W || h.H != headers_out[0].H) return kGatherWindowDiffers;
        if (memcmp(h.pv_g, headers_out[0].pv_g, sizeof h.pv_g) != 0) return kGatherCameraDiffers;
    }
    *index = -1;
    return kGatherAccepted;
}

// binary32 -> binary16, round to nearest even, by integer operations (numpy's astype(float16), bit for bit:
// subnormal halves are produced, anything that rounds beyond 65504 is infinity, a NaN keeps its top payload bits
// and stays a NaN).  Independent of the kernel's rounding and denormal modes.  gfx950's own conversion gives the
// same bits for every input that is not a NaN, subnormals included, but quiets the 2^23 - 2 signalling NaNs, whose
// payload numpy keeps (all 2^32 inputs compared on an MI355X): the integer form is what makes the bytes numpy's.
INSITU_HD inline uint16_t half_from_float_bits(uint32_t x) {
    const uint32_t sign = (x >> 16) & 0x8000u, a = x & 0x7fffffffu;
    if (a >= 0x7f800000u) {   // inf, NaN
        if (a == 0x7f800000u) return (uint16_t)(sign | 0x7c00u);
        const uint32_t r = 0x7c00u | ((a & 0x007fffffu) >> 13);
        return (uint16_t)(sign | (r == 0x7c00u ? 0x7c01u : r));
    }
    if (a >= 0x47800000u) return (uint16_t)(sign | 0x7c00u);   // >= 65536
    if (a >= 0x38800000u) {   // normal halves (>= 2^-14); a carry out of the mantissa raises the exponent, up to inf
        const uint32_t r = a - 0x38000000u;
        return (uint16_t)(sign | ((r + 0x0fffu + ((r >> 13) & 1u)) >> 13));
    }
    if (a < 0x33000000u) return (uint16_t)sign;   // <= 2^-25: zero (the tie at 2^-25 goes to even)
    const uint32_t mant = (a & 0x007fffffu) | 0x00800000u, shift = 126u - (a >> 23);   // 14..24
    uint32_t r = mant >> shift;
    const uint32_t rem = mant & ((1u << shift) - 1u), half = 1u << (shift - 1u);
    if (rem > half || (rem == half && (r & 1u))) r += 1u;   // (0x3ff + 1 is the smallest normal half)
    return (uint16_t)(sign | r);
}

// binary16 -> binary32, exact
INSITU_HD inline uint32_t float_bits_from_half(uint16_t h) {
    const uint32_t sign = ((uint32_t)h & 0x8000u) << 16, e = ((uint32_t)h >> 10) & 0x1fu;
    const uint32_t m = (uint32_t)h & 0x3ffu;
    if (e == 0x1fu) return sign | 0x7f800000u | (m << 13);
    if (e != 0u) return sign | ((e + 112u) << 23) | (m << 13);
    if (m == 0u) return sign;
    const uint32_t k = (uint32_t)__builtin_clz(m) - 21u;   // subnormal, m * 2^-24: k shifts bring its top bit to 2^10
    return sign | ((113u - k) << 23) | (((m << k) & 0x3ffu) << 13);
}

}  // namespace insitu
