// Stand-alone host program over pack_header_set_check of scenery-insitu_amd/csrc/vdi_pack_format.h: what the root of
// insitu_view_gather_merged checks before any section moves -- n headers of 128 bytes, no
// stream bodies.  No HIP, no GPU.  The headers lie in a heap block of exactly n * 128 bytes, so a read past the last
// header is a read past the allocation.  Prints "ok <cases>" and returns 0, or names the case that went wrong and
// returns 1.
//
// Built and run by tests/test_view_gather_host.py with -fsanitize=address,undefined -fno-sanitize-recover=all.
#include "vdi_pack_format.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

using namespace insitu;

namespace {

int g_cases = 0, g_failed = 0;

void failed(const std::string& name, const std::string& what) {
    ++g_failed;
    std::printf("FAILED %s: %s\n", name.c_str(), what.c_str());
}

using Head = std::vector<unsigned char>;   // 128 bytes

PackHeader header(uint32_t format, uint32_t W, uint32_t H, uint32_t S, uint64_t E) {
    PackHeader h{};
    h.format = format; h.W = W; h.H = H; h.S = S; h.E = E;
    for (int i = 0; i < 16; ++i) h.pv_g[i] = 0.37f * (float)i - 2.0f;
    return h;
}

Head head_of(const PackHeader& h) {
    Head b(kPackHeaderBytes);
    pack_write_header(b.data(), h);
    return b;
}

Head good(uint32_t format, uint32_t W, uint32_t H, uint32_t S, uint64_t E) { return head_of(header(format, W, H, S, E)); }

Head refusing(uint32_t reason) {
    Head b(kPackHeaderBytes, 0xff);
    pack_write_refusal(b.data(), reason);
    return b;
}

struct Outcome {
    uint32_t reason;
    int index;
    PackHeader h[kPackSetMax];
    PackLayout lay[kPackSetMax];
};

Outcome check(const std::vector<const Head*>& set) {
    const size_t bytes = set.size() * kPackHeaderBytes;
    std::unique_ptr<unsigned char, decltype(&std::free)> p(static_cast<unsigned char*>(std::malloc(bytes ? bytes : 1)), &std::free);
    for (size_t j = 0; j < set.size(); ++j) std::memcpy(p.get() + j * kPackHeaderBytes, set[j]->data(), kPackHeaderBytes);
    Outcome o{};
    o.index = 7;
    o.reason = pack_header_set_check(p.get(), (int)set.size(), o.h, o.lay, &o.index);
    return o;
}

void accept(const char* name, const std::vector<const Head*>& set) {
    ++g_cases;
    const Outcome o = check(set);
    if (o.reason != kGatherAccepted) return failed(name, std::string("rejected: ") + pack_gather_reason_text(o.reason));
    if (o.index != -1) return failed(name, "index set on success");
    for (size_t j = 0; j < set.size(); ++j) {
        // what comes out is the header that went in, and the layout of the stream it describes
        Head again(kPackHeaderBytes);
        pack_write_header(again.data(), o.h[j]);
        if (again != *set[j]) return failed(name, "header " + std::to_string(j) + " read back differently");
        PackLayout lay{};
        if (!pack_layout(o.h[j].format, o.h[j].W, o.h[j].H, o.h[j].S, o.h[j].E, &lay) || lay.total != o.lay[j].total ||
            lay.depth_off != o.lay[j].depth_off || lay.colour_off != o.lay[j].colour_off || lay.px != o.lay[j].px ||
            lay.depth_bytes != o.lay[j].depth_bytes || lay.colour_bytes != o.lay[j].colour_bytes)
            return failed(name, "layout " + std::to_string(j));
    }
}

void reject(const std::string& name, const std::vector<const Head*>& set, int index, uint32_t reason) {
    ++g_cases;
    const Outcome o = check(set);
    if (o.reason == kGatherAccepted) return failed(name, "accepted");
    if (o.index != index) return failed(name, "index " + std::to_string(o.index) + ", expected " + std::to_string(index));
    if (o.reason != reason)
        return failed(name, std::string("reason '") + pack_gather_reason_text(o.reason) + "', expected '" +
                                pack_gather_reason_text(reason) + "'");
}

}  // namespace

int main() {
    static_assert(kPackSetMax == 32, "as many ranks as the merge takes lists");
    const Head a = good(kPackFloat, 16, 8, 6, 300), b = good(kPackHalf, 16, 8, 2, 17), c = good(kPackFloat, 16, 8, 255, 0);
    const Head full = good(kPackHalf, 16, 8, 6, 16 * 8 * 6), odd = good(kPackFloat, 9, 7, 1, 63);

    accept("one header", {&a});
    accept("two headers: S and format differ", {&a, &b});
    accept("three headers, one empty, one full", {&c, &full, &a});
    accept("9x7", {&odd, &odd});
    accept("32 headers", std::vector<const Head*>(32, &b));

    // the set itself
    reject("33 headers", std::vector<const Head*>(33, &b), -1, kGatherBadRankCount);
    reject("no headers", {}, -1, kGatherBadRankCount);
    ++g_cases;
    {
        PackHeader h[kPackSetMax];
        PackLayout lay[kPackSetMax];
        for (int n : {0, -1, 33, 1 << 30}) {
            int index = 7;   // (nothing of the one header is looked at)
            if (pack_header_set_check(a.data(), n, h, lay, &index) != kGatherBadRankCount || index != -1) failed("n out of range", "accepted");
        }
        int index = 7;
        if (pack_header_set_check(nullptr, 1, h, lay, &index) != kGatherBadRankCount || index != -1) failed("null headers", "accepted");
    }

    // a rank that refuses: every reason, at index 0 and at the last index
    for (uint32_t r = kGatherNothingBound; r <= kGatherLastRefusal; ++r) {
        const Head no = refusing(r);
        const std::string name = std::string("refusal '") + pack_gather_reason_text(r) + "'";
        reject(name + " at index 0", {&no, &a, &b}, 0, r);
        reject(name + " at the last index", {&a, &b, &no}, 2, r);
        reject(name + " alone", {&no}, 0, r);
        std::vector<const Head*> many(32, &b);
        many[31] = &no;
        reject(name + " at index 31", many, 31, r);
    }
    {
        // the first refusal is the one reported; zeroed magic with no reason of a rank's is no refusal
        const Head unbound = refusing(kGatherNothingBound), busy = refusing(kGatherFrameInFlight);
        reject("two refusals", {&a, &busy, &unbound}, 1, kGatherFrameInFlight);
        const Head zero = refusing(0), beyond = refusing(kGatherLastRefusal + 1), root_only = refusing(kGatherCameraDiffers);
        reject("zeroed magic, reason 0", {&a, &zero}, 1, kGatherBadMagic);
        reject("zeroed magic, reason 5", {&beyond, &a}, 0, kGatherBadMagic);
        reject("zeroed magic, a reason of the root's", {&a, &root_only}, 1, kGatherBadMagic);
        Head all_zero(kPackHeaderBytes, 0);
        reject("128 zero bytes", {&a, &all_zero}, 1, kGatherBadMagic);
    }

    // a bad header at each position; the reasons are pack_parse's
    {
        Head magic = a, version = a;
        magic[3] = 'Q';
        version[4] = 2;
        reject("bad magic, second of three", {&a, &magic, &b}, 1, kGatherBadMagic);
        reject("bad magic, first", {&magic, &a}, 0, kGatherBadMagic);
        reject("version 2", {&version, &a}, 0, kGatherUnknownVersion);
        reject("version 2, last", {&a, &b, &version}, 2, kGatherUnknownVersion);
        const Head fmt = good(2, 16, 8, 6, 300), s0 = good(kPackFloat, 16, 8, 0, 0), s256 = good(kPackFloat, 16, 8, 256, 300);
        const Head w0 = good(kPackFloat, 0, 8, 6, 0), h0 = good(kPackFloat, 16, 0, 6, 0);
        reject("format 2", {&a, &fmt, &b}, 1, kGatherUnknownFormat);
        reject("S = 0", {&a, &s0, &b}, 1, kGatherBadSlots);
        reject("S = 256", {&a, &b, &s256}, 2, kGatherBadSlots);
        reject("W = 0", {&a, &w0}, 1, kGatherZeroWindow);
        reject("H = 0", {&h0, &a}, 0, kGatherZeroWindow);
        const Head e_over = good(kPackFloat, 16, 8, 6, 16 * 8 * 6 + 1), e_over1 = good(kPackHalf, 16, 8, 1, 129);
        reject("E one above W*H*S", {&a, &e_over, &b}, 1, kGatherOutOfRange);
        reject("E one above W*H, S = 1", {&e_over1}, 0, kGatherOutOfRange);
    }
    // every reason pack_parse can give of a header has a code of its own
    ++g_cases;
    for (uint32_t r = 0; r < kGatherReasons; ++r)
        for (uint32_t q = r + 1; q < kGatherReasons; ++q)
            if (std::strcmp(pack_gather_reason_text(r), pack_gather_reason_text(q)) == 0) failed("reason texts", "two codes share a text");

    // agreement across the set
    const Head wide = good(kPackFloat, 17, 8, 6, 0), tall = good(kPackFloat, 16, 9, 6, 0), swapped = good(kPackFloat, 8, 16, 6, 0);
    reject("W differs", {&a, &wide}, 1, kGatherWindowDiffers);
    reject("H differs", {&a, &b, &tall}, 2, kGatherWindowDiffers);
    reject("W and H swapped: the same pixels", {&a, &swapped}, 1, kGatherWindowDiffers);
    for (int word = 0; word < 16; ++word)
        for (uint32_t bit : {0u, 31u}) {
            PackHeader h = header(kPackFloat, 16, 8, 6, 0);
            uint32_t bits;
            std::memcpy(&bits, &h.pv_g[word], 4);
            bits ^= 1u << bit;
            std::memcpy(&h.pv_g[word], &bits, 4);
            const Head cam = head_of(h);
            const std::string name = "pv_g[" + std::to_string(word) + "] differs in bit " + std::to_string(bit);
            reject(name, {&a, &b, &cam}, 2, kGatherCameraDiffers);
            if (word == 11) reject(name + ", first against second", {&cam, &a}, 1, kGatherCameraDiffers);
        }

    // dimensions whose products wrap 32 or 64 bits, and sizes near the size_t limit
    struct Dims {
        const char* name;
        uint32_t W, H, S;
        uint64_t E;
    };
    for (const Dims& d : {Dims{"W*H = 2^32: 0 in 32 bits", 65536u, 65536u, 1u, 0},
                          Dims{"W*H = 2^32 + 128: 16x8 in 32 bits", 0x80000040u, 2u, 6u, 300},
                          Dims{"W = H = 2^32 - 1", 0xffffffffu, 0xffffffffu, 255u, 0},
                          Dims{"2^30 + 2^15 pixels", 32769u, 32768u, 1u, 0},
                          Dims{"E = 2^64 - 1", 16u, 8u, 6u, ~0ull},
                          Dims{"E = 2^64 - 128: the size wraps to the header's", 16u, 8u, 6u, ~0ull - 127u},
                          Dims{"E = 2^61: 8 E is 0 in 64 bits", 16u, 8u, 6u, 1ull << 61},
                          Dims{"E = 2^60 + 300: 16 E wraps to 4800", 16u, 8u, 6u, (1ull << 60) + 300},
                          Dims{"2^30 pixels, E one above 255 per pixel", 32768u, 32768u, 255u, 273804165121ull}}) {
        const Head big = good(kPackFloat, d.W, d.H, d.S, d.E);
        reject(d.name, {&a, &big, &b}, 1, kGatherOutOfRange);
        reject(std::string(d.name) + ", first", {&big, &a}, 0, kGatherOutOfRange);
    }
    // the largest stream there is: its header alone is accepted, with the size it implies
    {
        const Head big = good(kPackFloat, 32768u, 32768u, 255u, 273804165120ull);
        accept("2^30 pixels of 255 entries", {&big, &big});
        ++g_cases;
        const Outcome o = check({&big});
        const unsigned long long each = 128ull + 1073741824ull + 273804165120ull * 24ull;
        if (o.reason != kGatherAccepted || o.lay[0].total != each) failed("largest header", "size");
        const Head small = good(kPackFloat, 16, 8, 6, 0);
        reject("the largest against 16x8", {&big, &small}, 1, kGatherWindowDiffers);
    }

    if (g_failed) return 1;
    std::printf("ok %d\n", g_cases);
    return 0;
}
