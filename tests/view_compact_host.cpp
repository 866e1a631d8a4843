// Stand-alone host program over scenery-insitu_amd/csrc/vdi_view_layout.h, the size arithmetic of the dense and the
// compact view layout.  No HIP, no GPU.  Every expected value is written out; prints
// "ok <cases>" and returns 0, or names the case that went wrong and returns 1.
//
// Built and run by tests/test_view_compact.py with -fsanitize=address,undefined -fno-sanitize-recover=all: a product
// that overflowed a signed type or a shift out of range would end the run.
#include "vdi_view_layout.h"

#include <climits>
#include <cstdio>

using namespace insitu;

namespace {

int g_cases = 0, g_failed = 0;

void failed(const char* name, const char* what, unsigned long long got, unsigned long long want) {
    ++g_failed;
    std::printf("FAILED %s: %s %llu, expected %llu\n", name, what, got, want);
}

struct Want {
    unsigned long long px, tiles, nblocks, dense_bytes, compact_bytes;
};

// both layouts of (W, H, S) with E stored entries
void expect(const char* name, int W, int H, int S, unsigned long long E, const Want& w) {
    ++g_cases;
    ViewLayoutSize d{}, c{};
    if (!view_dense_size(W, H, S, &d)) return failed(name, "dense rejected", 0, 1);
    if (!view_compact_size(W, H, S, E, &c)) return failed(name, "compact rejected", 0, 1);
    if (d.px != w.px || c.px != w.px) return failed(name, "px", d.px, w.px);
    if (d.tiles != w.tiles || c.tiles != w.tiles) return failed(name, "tiles", d.tiles, w.tiles);
    if (c.nblocks != w.nblocks) return failed(name, "nblocks", c.nblocks, w.nblocks);
    if (d.entries != w.px * (unsigned long long)S) return failed(name, "dense entries", d.entries, w.px * (unsigned long long)S);
    if (c.entries != (E ? E : 1)) return failed(name, "compact entries", c.entries, E ? E : 1);
    if (d.bytes != w.dense_bytes) return failed(name, "dense bytes", d.bytes, w.dense_bytes);
    if (c.bytes != w.compact_bytes) return failed(name, "compact bytes", c.bytes, w.compact_bytes);
}

void reject(const char* name, int W, int H, int S, unsigned long long E, bool dense_too) {
    ++g_cases;
    ViewLayoutSize d{}, c{};
    if (view_compact_size(W, H, S, E, &c)) return failed(name, "compact accepted, bytes", c.bytes, 0);
    if (view_dense_size(W, H, S, &d) == dense_too) return failed(name, "dense accepted", dense_too ? 1 : 0, dense_too ? 0 : 1);
}

}  // namespace

int main() {
    static_assert(kViewMaxLoc == 65025u && kViewMaxLoc < 65536u, "a block's largest in-block offset fits 16 bits");
    static_assert(kViewBlockPx == 256u && kViewEntryBytes == 24u && kViewMaxPixels == 1073741824ull, "constants");

    // the shapes of tests/test_gpu_view_compact.py
    expect("64x48 S=6", 64, 48, 6, 5000, {3072, 48, 12, 445488, 129360});
    expect("50x37 S=5", 50, 37, 5, 1850, {1850, 35, 8, 223885, 50049});
    expect("9x7 S=1, one partial block", 9, 7, 1, 63, {63, 2, 1, 1577, 1711});
    expect("32x8 S=255 full, exactly one block", 32, 8, 255, 65280, {256, 4, 1, 1566980, 1567500});
    expect("20x12 S=255 full, a partial block", 20, 12, 255, 61200, {240, 6, 1, 1469046, 1469534});
    expect("12x5 S=3, E = 0", 12, 5, 3, 0, {60, 2, 1, 4382, 214});
    expect("260x130 S=2, 133 blocks", 260, 130, 2, 33800, {33800, 561, 133, 1656761, 914225});
    expect("400x170 S=1, 266 blocks", 400, 170, 1, 30000, {68000, 1100, 266, 1701100, 927228});
    expect("257 pixels: a second block of one pixel", 257, 1, 1, 1, {257, 33, 2, 6458, 844});
    // the benchmark's frame (995 MB dense)
    expect("1920x1080 S=20", 1920, 1080, 20, 13083333, {2073600, 32400, 8100, 997434000, 320317992});
    // 2^30 pixels of 255 entries: the largest VDI there is
    expect("32768x32768 S=255, every slot", 32768, 32768, 255, 273804165120ull,
           {1073741824ull, 16777216ull, 4194304ull, 6572390481920ull, 6574571520000ull});
    expect("32768x32768 S=255, E = 0", 32768, 32768, 255, 0, {1073741824ull, 16777216ull, 4194304ull, 6572390481920ull, 3271557144ull});
    expect("2^30 x 1", 1 << 30, 1, 1, 7, {1073741824ull, 134217728ull, 4194304ull, 26977763328ull, 3388997800ull});

    reject("E one above W*H*S", 9, 7, 1, 64, false);
    reject("E one above 2^30 * 255", 32768, 32768, 255, 273804165121ull, false);
    reject("E = 2^64 - 1", 64, 48, 6, ~0ull, false);
    reject("2^30 + 2^15 pixels", 32769, 32768, 1, 0, true);
    reject("W*H = 2^32: 0 in 32 bits", 65536, 65536, 1, 0, true);
    reject("W*H = 2^32 + 2^17 + 1: small in 32 bits", 65537, 65537, 1, 0, true);
    reject("W = H = 2^31 - 1", INT_MAX, INT_MAX, 255, 0, true);
    reject("W = 2^31 - 1, H = 2: negative as an int product", INT_MAX, 2, 1, 0, true);
    reject("W = 0", 0, 48, 6, 0, true);
    reject("H = -1", 64, -1, 6, 0, true);
    reject("W = INT_MIN", INT_MIN, 48, 6, 0, true);
    reject("S = 0", 64, 48, 0, 0, true);
    reject("S = 256", 64, 48, 256, 0, true);
    reject("S = -1", 64, 48, -1, 0, true);

    ++g_cases;
    if (view_blocks(0) != 0 || view_blocks(1) != 1 || view_blocks(256) != 1 || view_blocks(257) != 2 ||
        view_blocks(kViewMaxPixels) != 4194304ull)
        failed("view_blocks", "wrong", 0, 0);

    if (g_failed) return 1;
    std::printf("ok %d\n", g_cases);
    return 0;
}
