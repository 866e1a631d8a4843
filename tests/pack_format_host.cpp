// Stand-alone host program over scenery-insitu_amd/csrc/vdi_pack_format.h, the part of insitu_view_bind_packed that
// reads bytes from outside the process: header parsing, size arithmetic, binary16 conversion.  No HIP, no GPU.
//
//   pack_format_host            feeds pack_parse good and rejected headers and sizes, every stream in a heap block of
//                               exactly its size (so a read past it is a finding for AddressSanitizer); prints
//                               "ok <cases>" and returns 0, or names the case that went wrong and returns 1
//   pack_format_host half       stdin: binary32 bit patterns in hex, one per line -> their binary16 bits
//   pack_format_host float      stdin: binary16 bit patterns in hex -> their binary32 bits
//
// Built plainly by tests/test_vdi_pack.py; for a sanitizer run:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Iscenery-insitu_amd/csrc
//       tests/pack_format_host.cpp -o pack_format_host && ./pack_format_host
#include "vdi_pack_format.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

using namespace insitu;

namespace {

int g_cases = 0, g_failed = 0;

// a stream of `bytes` bytes in a heap block of that size, its first bytes the header `h` as written (or cut short)
struct Stream {
    unsigned char* p;
    size_t bytes;
    Stream(const PackHeader& h, size_t n) : p(static_cast<unsigned char*>(std::malloc(n ? n : 1))), bytes(n) {
        unsigned char hdr[kPackHeaderBytes];
        pack_write_header(hdr, h);
        std::memset(p, 0, n);
        std::memcpy(p, hdr, n < kPackHeaderBytes ? n : kPackHeaderBytes);
    }
    ~Stream() { std::free(p); }
};

void expect(const char* name, const Stream& s, bool accepted) {
    PackHeader h{};
    PackLayout lay{};
    const char* why = pack_parse(s.p, s.bytes, &h, &lay);
    ++g_cases;
    if ((why == nullptr) != accepted) {
        ++g_failed;
        std::printf("FAILED %s: %s\n", name, why ? why : "accepted");
    } else if (accepted && (lay.total != s.bytes || lay.colour_off + lay.colour_bytes != lay.total ||
                            lay.depth_off + lay.depth_bytes != lay.colour_off)) {
        ++g_failed;
        std::printf("FAILED %s: inconsistent layout\n", name);
    }
}

size_t size_of(const PackHeader& h) {
    return kPackHeaderBytes + (((size_t)h.W * h.H + 15) & ~(size_t)15) + (size_t)h.E * (h.format == kPackHalf ? 16 : 24);
}

int self_check() {
    PackHeader good{};
    good.format = kPackFloat; good.W = 9; good.H = 7; good.S = 3; good.E = 40;
    for (int i = 0; i < 16; ++i) good.pv_g[i] = (float)i;
    expect("good float", Stream(good, size_of(good)), true);
    PackHeader h = good;
    h.format = kPackHalf;
    expect("good half", Stream(h, size_of(h)), true);
    h = good; h.E = 0;
    expect("good empty", Stream(h, size_of(h)), true);
    h = good; h.S = 255; h.E = 9 * 7 * 255;
    expect("good S = 255, every slot stored", Stream(h, size_of(h)), true);

    {
        Stream s(good, size_of(good));
        s.p[0] = 'X';
        expect("bad magic", s, false);
    }
    {
        Stream s(good, size_of(good));
        s.p[4] = 2;
        expect("version 2", s, false);
    }
    h = good; h.format = 2;
    expect("format 2", Stream(h, size_of(good)), false);
    h = good; h.format = 0xffffffffu;
    expect("format 2^32 - 1", Stream(h, size_of(good)), false);
    h = good; h.S = 0;
    expect("S = 0", Stream(h, size_of(good)), false);
    h = good; h.S = 256;
    expect("S = 256", Stream(h, size_of(good)), false);
    h = good; h.W = 0;
    expect("W = 0", Stream(h, size_of(good)), false);
    h = good; h.H = 0;
    expect("H = 0", Stream(h, size_of(good)), false);
    expect("one byte short", Stream(good, size_of(good) - 1), false);
    expect("one byte long", Stream(good, size_of(good) + 1), false);
    expect("header only", Stream(good, kPackHeaderBytes), false);
    expect("shorter than the header", Stream(good, kPackHeaderBytes - 1), false);
    expect("ten bytes", Stream(good, 10), false);
    expect("no bytes", Stream(good, 0), false);
    h = good; h.E = (uint64_t)9 * 7 * 3 + 1;
    expect("E above W*H*S", Stream(h, size_of(h)), false);
    // dimensions whose products overflow 32 and 64 bits, against small and matching-looking sizes
    h = good; h.W = 0xffffffffu; h.H = 0xffffffffu;
    expect("W = H = 2^32 - 1", Stream(h, size_of(good)), false);
    h = good; h.W = 0x10000u; h.H = 0x10000u;   // W*H = 2^32: 0 in 32 bits
    expect("W*H = 2^32", Stream(h, kPackHeaderBytes + 40 * 24), false);
    h = good; h.W = 0x80000000u; h.H = 2;
    expect("W = 2^31", Stream(h, size_of(good)), false);
    h = good; h.E = ~(uint64_t)0;
    expect("E = 2^64 - 1", Stream(h, size_of(good)), false);
    h = good; h.E = ((uint64_t)1 << 61) + 40;   // 8 E wraps to 8 * 40 in 64 bits
    expect("E whose byte count wraps", Stream(h, size_of(good)), false);
    h = good; h.E = (uint64_t)1 << 60;
    expect("E = 2^60", Stream(h, size_of(good)), false);
    {
        PackHeader hh{};
        PackLayout lay{};
        ++g_cases;
        if (pack_parse(nullptr, 1000, &hh, &lay) == nullptr) {
            ++g_failed;
            std::printf("FAILED null stream: accepted\n");
        }
    }
    if (g_failed) return 1;
    std::printf("ok %d\n", g_cases);
    return 0;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc < 2) return self_check();
    const bool to_half = std::strcmp(argv[1], "half") == 0;
    if (!to_half && std::strcmp(argv[1], "float") != 0) return 2;
    unsigned int x;
    while (std::scanf("%x", &x) == 1) {
        if (to_half) std::printf("%04x\n", (unsigned)half_from_float_bits((uint32_t)x));
        else std::printf("%08x\n", (unsigned)float_bits_from_half((uint16_t)x));
    }
    return 0;
}
