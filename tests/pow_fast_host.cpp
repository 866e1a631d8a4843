// Host build of det_pow_normal and its guard (scenery-insitu_amd/csrc/insitu_device.h) for
// tests/test_pow_fast_host.py: over x = every 64th float of [2^-126, 1] and every float within 2^12 ulps of
// 2^-126, 0.5 and 1, crossed with a grid of exponents y and, per x, the exponents that put y * log2(x) on and
// beside both edges of the guard's range,
//   * where the guard holds, det_pow_normal(x, y) must have the bits of det_pow(x, y);
//   * the guard must hold exactly where x is a finite positive normal and y * det_log2(x) lies in
//     [kPowNormalLo, kPowNormalHi] (so never beyond either edge, and never for x = 0, subnormal, negative, inf, NaN).
// Prints one line of counts: "pairs guarded on_edge mismatches guard_wrong special_accepted".
#include <cstdio>
#include <cstdint>
#include <cstring>
#include <thread>
#include <vector>
#include "insitu_device.h"

namespace {

float from_bits(uint32_t u) {
    float f;
    std::memcpy(&f, &u, 4);
    return f;
}
uint32_t bits_of(float f) {
    uint32_t u;
    std::memcpy(&u, &f, 4);
    return u;
}

struct Counts {
    unsigned long long pairs = 0, guarded = 0, on_edge = 0, mismatches = 0, guard_wrong = 0, special = 0;
    void add(const Counts& o) {
        pairs += o.pairs, guarded += o.guarded, on_edge += o.on_edge, mismatches += o.mismatches;
        guard_wrong += o.guard_wrong, special += o.special;
    }
};

const float kGrid[] = {0.0f, 1.0e-30f, 0.01f, 0.5f, 1.0f, 1.00000012f, 1.008f, 3.7f, 127.0f, 1.0e6f};

__attribute__((always_inline)) inline void check(float x, float y, Counts& c) {
    c.pairs++;
    const bool ok = insitu::det_pow_normal_ok(x, y);
    const float t = y * insitu::det_log2(x);   // the general path's exponent
    const bool normal = x >= 1.17549435e-38f && x < __builtin_inff();
    const bool want = normal && t >= insitu::kPowNormalLo && t <= insitu::kPowNormalHi;
    if (ok != want && c.guard_wrong++ < 5) std::fprintf(stderr, "guard(%08x, %08x) = %d\n", bits_of(x), bits_of(y), (int)ok);
    if (!ok) return;
    c.guarded++;
    if (t == insitu::kPowNormalLo || t == insitu::kPowNormalHi) c.on_edge++;
    const float a = insitu::det_pow_normal(x, y), b = insitu::det_pow(x, y);
    if (bits_of(a) != bits_of(b) && c.mismatches++ < 5)
        std::fprintf(stderr, "det_pow_normal(%08x, %08x) = %08x, det_pow %08x\n", bits_of(x), bits_of(y), bits_of(a), bits_of(b));
}

__attribute__((always_inline)) inline void check_x(float x, Counts& c) {
    for (float y : kGrid) {
        check(x, y, c);
        check(x, -y, c);
    }
    // the exponents at both edges of the range and 1 and 2 ulps to either side of them
    const float l = insitu::det_log2(x);
    if (l == 0.0f) return;
    for (float edge : {insitu::kPowNormalLo, insitu::kPowNormalHi}) {
        const uint32_t u = bits_of(edge / l);
        for (int d : {-2, -1, 0, 1, 2}) check(x, from_bits(u + (uint32_t)d), c);
    }
}

void range(uint32_t lo, uint32_t hi, uint32_t stride, Counts& c) {
    for (uint64_t u = lo; u <= hi; u += stride) check_x(from_bits((uint32_t)u), c);
}

}  // namespace

int main() {
    const uint32_t tiny = 0x00800000u, half = 0x3f000000u, one = 0x3f800000u;
    const unsigned nt = 8;
    std::vector<Counts> part(nt);
    std::vector<std::thread> th;
    const uint32_t span = (one - tiny) / nt;   // (a multiple of 64)
    for (unsigned i = 0; i < nt; ++i)
        th.emplace_back([&, i] { range(tiny + i * span, i + 1 == nt ? one : tiny + (i + 1) * span - 1u, 64u, part[i]); });
    Counts c;
    range(tiny, tiny + 4096u, 1u, c);   // (below 2^-126: subnormal, with the special values)
    range(half - 4096u, half + 4096u, 1u, c);
    range(one - 4096u, one + 4096u, 1u, c);
    for (auto& t : th) t.join();
    for (const Counts& p : part) c.add(p);
    // x the guard must refuse whatever the exponent: zeros, subnormals, negatives, inf, NaN
    std::vector<uint32_t> bad = {0x00000000u, 0x80000000u, 0x00000001u, 0x007fffffu, 0x00400000u, 0x80000001u, 0x807fffffu,
                                 0xbf800000u, 0x80800000u, 0xff7fffffu, 0x7f800000u, 0xff800000u, 0x7fc00000u, 0xffc00000u,
                                 0x7f800001u};
    for (uint32_t u = tiny - 4096u; u < tiny; ++u) bad.push_back(u);
    for (uint32_t u : bad) {
        const float x = from_bits(u);
        for (float y : kGrid)
            for (float s : {1.0f, -1.0f})
                if (insitu::det_pow_normal_ok(x, s * y)) c.special++;
        for (float y : {__builtin_inff(), -__builtin_inff(), __builtin_nanf("")})
            if (insitu::det_pow_normal_ok(x, y)) c.special++;
    }
    // non-finite exponents on ordinary x
    for (float x : {0.5f, 0.999f, 1.0f, 1.17549435e-38f, 3.0f})
        for (float y : {__builtin_inff(), -__builtin_inff(), __builtin_nanf("")})
            if (insitu::det_pow_normal_ok(x, y)) c.special++;
    std::printf("%llu %llu %llu %llu %llu %llu\n", c.pairs, c.guarded, c.on_edge, c.mismatches, c.guard_wrong, c.special);
    return 0;
}
