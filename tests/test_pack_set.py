"""A set of packed streams merged into one VDI without a GPU: vdi_io.merge_packed against a
plain per-pixel merge loop written here (not merge_vdis, not the library) -- byte for byte -- over the oracle scene
sets of section 9.6, streams of different S, mixed formats, a tie, a zero start inside a stream's count, empty sets;
the hierarchy (merging merged streams equals the flat merge) that the multi-rank GPU test rests on; the limit of 255
slots and every rejection; the host half of insitu_view_bind_packed_set (pack_set_parse, pack_set_stage of
csrc/vdi_pack_format.h) through the stand-alone tests/pack_set_host.cpp under AddressSanitizer and
UndefinedBehaviorSanitizer; and the export.  loop_merge_set and the stream builders are shared with
tests/test_gpu_view_pack_set.py."""
from __future__ import annotations

import ctypes
import re
import struct
import subprocess
from pathlib import Path

import numpy as np
import pytest

import view_binding as vb
from insitu_amd import native, vdi_io
from insitu_amd.vdi_io import PACK_FLOAT, PACK_HALF, merge_packed, pack_vdi, unpack_vdi
from test_vdi_pack import PV, random_vdi, rejected_streams
from test_view_merge import SCENE_SETS, oracle_set

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "scenery-insitu_amd" / "csrc"
HEADER = ROOT / "include" / "insitu_hip.h"


def loop_merge_set(cols, deps):
    """The definition, pixel by pixel, over reference-layout VDIs of one window whose S may differ:
    repeatedly the front with the smallest start depth, the lists scanned in ascending order with a strict `<` from
    100000; a list ends at its S slots or at a zero start, and a front that is not below 100000 is never taken.
    -> (colour (W, H, S_m, 4), depth (W, H, 2 S_m), overlaps), S_m = max(1, the longest merged list); ValueError
    above 255."""
    n = len(cols)
    w, h = cols[0].shape[:2]
    slots = [c.shape[2] for c in cols]
    starts = [np.asarray(d, np.float32)[:, :, 0::2].tolist() for d in deps]
    picks = {}
    for x in range(w):
        for y in range(h):
            at = [0] * n
            out = []
            while True:
                low, idx = 100000.0, -1
                for j in range(n):
                    if at[j] < slots[j]:
                        c = starts[j][x][y][at[j]]
                        if c != 0.0 and c < low:
                            low, idx = c, j
                if idx < 0:
                    break
                out.append((idx, at[idx]))
                at[idx] += 1
            picks[(x, y)] = out
    s_m = max(1, max(len(p) for p in picks.values()))
    if s_m > 255:
        raise ValueError(f"{s_m} entries in a merged list")
    col = np.zeros((w, h, s_m, 4), np.float32)
    dep = np.zeros((w, h, 2 * s_m), np.float32)
    overlaps = 0
    for (x, y), out in picks.items():
        for k, (j, i) in enumerate(out):
            col[x, y, k] = cols[j][x, y, i]
            dep[x, y, 2 * k:2 * k + 2] = deps[j][x, y, 2 * i:2 * i + 2]
            if k and dep[x, y, 2 * k] < dep[x, y, 2 * k - 1]:
                overlaps += 1
    return col, dep, overlaps


def merged_stream(streams, pv=None, fmt=PACK_FLOAT):
    """What a bind of `streams` must hold: pack_vdi of the loop's merge of the unpacked streams (a HALF stream's
    colours enter widened, which is what unpack_vdi returns).  -> (stream, (colour, depth, overlaps))."""
    vdis = [unpack_vdi(s) for s in streams]
    merged = loop_merge_set([v[0] for v in vdis], [v[1] for v in vdis])
    return pack_vdi(merged[0], merged[1], vdis[0][2] if pv is None else pv, fmt), merged


def _same(got, want, what):
    assert got.dtype == np.uint8 and got.size == want.size, f"{what}: {got.size} bytes, expected {want.size}"
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, f"{what}: {bad.size} of {want.size} bytes differ, the first at {int(bad[0])}"


def _header(buf):
    magic, version, fmt, W, H, S, E = struct.unpack_from("<4sIIIIIQ", np.asarray(buf).tobytes(), 0)
    return dict(fmt=fmt, W=W, H=H, S=S, E=E)


# ---------------------------------------------------------------- streams the GPU tests bind as well
def tie_streams():
    """Three 16x8 streams (S = 2, 1, 2; the colour of entry i of stream j is (j, i, 0, 0.5)): streams 0 and 2 both
    start at 0.2 -- the merged order is (0,0) (2,0) (1,0) (2,1) (0,1)."""
    out = []
    for j, starts in enumerate(([0.2, 0.5], [0.3], [0.2, 0.4])):
        col = np.zeros((16, 8, len(starts), 4), np.float32)
        dep = np.zeros((16, 8, 2 * len(starts)), np.float32)
        for i, z in enumerate(starts):
            col[:, :, i] = (j, i, 0.0, 0.5)
            dep[:, :, 2 * i:2 * i + 2] = (z, z + 0.05)
        out.append(pack_vdi(col, dep, PV, PACK_FLOAT))
    return out


def zero_inside_count_stream(fmt=PACK_FLOAT):
    """A 16x8, S = 4 stream that pack_vdi cannot write, built with struct: every pixel's count is 4 and its entries
    start at 0.1, 0, 0.3, 0.4 -- the list ends at the zero, inside the count."""
    W, H, S = 16, 8, 4
    E = W * H * S
    head = struct.pack("<4sIIIIIQ16f32x", b"IVDP", 1, fmt, W, H, S, E, *[float(v) for v in PV])
    counts = bytes([S]) * (W * H)
    dep = np.tile(np.array([[0.1, 0.15], [0.0, 0.25], [0.3, 0.35], [0.4, 0.45]], np.float32), (W * H, 1))
    col = np.tile(np.array([[9, i, 0, 0.5] for i in range(S)], np.float32), (W * H, 1))
    col = col.astype(np.float16) if fmt == PACK_HALF else col
    raw = head + counts + dep.tobytes() + col.tobytes()
    assert len(raw) == vdi_io.packed_size(W, H, E, fmt)
    return np.frombuffer(raw, np.uint8).copy()


def random_streams(n, seed, w=16, h=8):
    """n streams of one w x h window with S drawn from 1..4 per stream (every S occurs from n = 9 on), start depths
    from 24 shared values so that lists tie, and alternating FLOAT and HALF."""
    rng = np.random.default_rng(seed)
    grid = np.linspace(0.9, 0.99, 24).astype(np.float32)
    half = np.float32(0.5) * (grid[1] - grid[0])
    out = []
    for j in range(n):
        s = int(rng.integers(1, 5)) if j >= 4 else j + 1
        pick = np.sort(np.argsort(rng.random((w, h, 24)), axis=2)[:, :, :s], axis=2)   # s distinct values, increasing
        live = np.arange(s)[None, None, :] < rng.integers(0, s + 1, size=(w, h))[:, :, None]
        dep = np.zeros((w, h, 2 * s), np.float32)
        dep[:, :, 0::2] = grid[pick] * live
        dep[:, :, 1::2] = (grid[pick] + half) * live
        col = rng.random(size=(w, h, s, 4), dtype=np.float32) * live[..., None]
        out.append(pack_vdi(col, dep, PV, PACK_HALF if j % 2 else PACK_FLOAT))
    return out


def layered_streams(n_a, n_b):
    """Two 16x8 streams of n_a and n_b abutting layers in every list (vb.layered_vdi: the second set behind the
    first)."""
    z0, z1, rgba = vb.SLAB[0]
    z = np.linspace(z0, z1, n_a + n_b + 1).astype(np.float32)
    assert np.all(np.diff(z) > 0)
    a = vb.slab_vdi([(z[i], z[i + 1], rgba) for i in range(n_a)], 16, 8, n_a)
    b = vb.slab_vdi([(z[n_a + i], z[n_a + i + 1], rgba) for i in range(n_b)], 16, 8, n_b)
    return [pack_vdi(*a, PV, PACK_FLOAT), pack_vdi(*b, PV, PACK_FLOAT)]


# ---------------------------------------------------------------- merge_packed against the loop
@pytest.mark.parametrize("name", list(SCENE_SETS))
def test_oracle_scene_sets(name):
    cols, deps, _ = oracle_set(name)
    streams = [pack_vdi(c, d, PV, PACK_FLOAT) for c, d in zip(cols, deps)]
    want, merged = merged_stream(streams)
    _same(merge_packed(streams), want, name)
    assert _header(want)["S"] == merged[0].shape[2] > cols[0].shape[2]
    # ... and in the other format
    _same(merge_packed(streams, PACK_HALF), pack_vdi(merged[0], merged[1], PV, PACK_HALF), name + ", HALF")


def test_streams_of_different_S():
    a, b = random_vdi(37, 21, 2, 31), random_vdi(37, 21, 5, 32)
    streams = [pack_vdi(*a, PV, PACK_FLOAT), pack_vdi(*b, PV, PACK_FLOAT)]
    want, merged = merged_stream(streams)
    _same(merge_packed(streams), want, "S = 2 and S = 5")
    # by definition: the S = 2 VDI zero-padded to 5 slots
    pc, pd = np.zeros((37, 21, 5, 4), np.float32), np.zeros((37, 21, 10), np.float32)
    pc[:, :, :2], pd[:, :, :4] = vb.truncate_lists(*a)
    padded = loop_merge_set([pc, vb.truncate_lists(*b)[0]], [pd, vb.truncate_lists(*b)[1]])
    _same(pack_vdi(padded[0], padded[1], PV, PACK_FLOAT), want, "padded to 5")
    assert 5 < merged[0].shape[2] <= 7


def test_mixed_formats():
    a, b, c = random_vdi(20, 9, 3, 41), random_vdi(20, 9, 3, 42), random_vdi(20, 9, 4, 43)
    streams = [pack_vdi(*a, PV, PACK_HALF), pack_vdi(*b, PV, PACK_FLOAT), pack_vdi(*c, PV, PACK_HALF)]
    cols = [vb.truncate_lists(*a)[0].astype(np.float16).astype(np.float32), vb.truncate_lists(*b)[0],
            vb.truncate_lists(*c)[0].astype(np.float16).astype(np.float32)]
    deps = [vb.truncate_lists(*v)[1] for v in (a, b, c)]
    merged = loop_merge_set(cols, deps)
    assert np.any(cols[0] != vb.truncate_lists(*a)[0])   # (the quantiser does something)
    for fmt in (PACK_FLOAT, PACK_HALF):
        _same(merge_packed(streams, fmt), pack_vdi(merged[0], merged[1], PV, fmt), f"mixed formats to {fmt}")
    _same(merged_stream(streams)[0], pack_vdi(merged[0], merged[1], PV, PACK_FLOAT), "the yardstick itself")


def test_tie_between_streams_0_and_2():
    streams = tie_streams()
    want, merged = merged_stream(streams)
    _same(merge_packed(streams), want, "tie")
    assert merged[0][2, 3, :, :2].tolist() == [[0, 0], [2, 0], [1, 0], [2, 1], [0, 1]]
    assert _header(want) == dict(fmt=PACK_FLOAT, W=16, H=8, S=5, E=16 * 8 * 5)


def test_zero_start_inside_a_count():
    for fmt in (PACK_FLOAT, PACK_HALF):
        streams = [tie_streams()[1], zero_inside_count_stream(fmt)]
        want, merged = merged_stream(streams)
        _same(merge_packed(streams), want, "zero inside the count")
        # stream 1 gives its first entry alone: 0.1 from it, then 0.3 from stream 0
        assert merged[0].shape[2] == 2 and merged[0][5, 5, :, :2].tolist() == [[9, 0], [1, 0]]
        assert _header(want)["E"] == 2 * 16 * 8


def test_all_empty_set():
    empty = [pack_vdi(np.zeros((12, 5, s, 4), np.float32), np.zeros((12, 5, 2 * s), np.float32), PV, f)
             for s, f in ((3, PACK_FLOAT), (1, PACK_HALF), (255, PACK_FLOAT))]
    got = merge_packed(empty)
    _same(got, merged_stream(empty)[0], "all-empty set")
    assert _header(got) == dict(fmt=PACK_FLOAT, W=12, H=5, S=1, E=0) and got.size == 128 + 64
    # one empty stream among others changes nothing
    streams = tie_streams()
    _same(merge_packed([streams[0], pack_vdi(np.zeros((16, 8, 2, 4), np.float32), np.zeros((16, 8, 4), np.float32), PV),
                        streams[1], streams[2]]), merge_packed(streams), "an empty stream in between")
    _same(merge_packed(streams[:1]), streams[0], "a set of one")


def test_hierarchy_equals_the_flat_merge():
    cols, deps, _ = oracle_set("abutting_2x2")
    for d in deps:   # the premise: every list is ordered by start depth
        st = d[:, :, 0::2]
        live = np.cumprod(st != 0.0, axis=2).astype(bool)
        assert np.all((np.diff(st, axis=2) > 0) | ~live[:, :, 1:])
    halves = []
    for pair in ((0, 1), (2, 3)):
        m = loop_merge_set([cols[j] for j in pair], [deps[j] for j in pair])
        halves.append(pack_vdi(m[0], m[1], PV, PACK_FLOAT))
    flat = loop_merge_set(cols, deps)
    _same(merge_packed(halves), pack_vdi(flat[0], flat[1], PV, PACK_FLOAT), "two merged pairs against the flat merge")
    assert flat[0].shape[2] == 13


# ---------------------------------------------------------------- limits and rejections
def test_slot_limit():
    got = merge_packed(layered_streams(128, 127))
    assert _header(got)["S"] == 255 and _header(got)["E"] == 255 * 16 * 8
    _same(got, merged_stream(layered_streams(128, 127))[0], "128 + 127")
    with pytest.raises(ValueError, match="256"):
        merge_packed(layered_streams(128, 128))


def _good():
    col, dep = vb.list_end_vdi()
    return col, dep, pack_vdi(col, dep, PV, PACK_FLOAT)


def test_rejections():
    col, dep, good = _good()
    pv_bit = PV.copy()
    pv_bit.view(np.uint32)[11] ^= 1
    for what, streams in (("W", [good, pack_vdi(*random_vdi(17, 8, 6, 1), PV)]),
                          ("H", [good, good, pack_vdi(*random_vdi(16, 9, 6, 1), PV)]),
                          ("W and H swapped", [good, pack_vdi(*random_vdi(8, 16, 6, 1), PV)]),
                          ("pv_g in one float's last bit", [good, pack_vdi(col, dep, pv_bit)]),
                          ("n = 0", []),
                          ("n = 33", [good] * 33)):
        with pytest.raises(ValueError):
            merge_packed(streams)
        pytest.raises(ValueError, merge_packed, streams, PACK_HALF)
    merge_packed([good] * 32)   # (32 is the most: 32 x 6 slots)
    with pytest.raises(ValueError):
        merge_packed([good, good], 2)


@pytest.mark.parametrize("name", list(rejected_streams()))
def test_bad_stream_second_of_three(name):
    _, _, good = _good()
    with pytest.raises(ValueError, match="stream 1"):
        merge_packed([good, rejected_streams()[name], good])


# ---------------------------------------------------------------- the host half of insitu_view_bind_packed_set
@pytest.fixture(scope="module")
def set_host(tmp_path_factory):
    exe = tmp_path_factory.mktemp("ps") / "pack_set_host"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", str(CSRC), str(ROOT / "tests" / "pack_set_host.cpp"),
                    "-o", str(exe)], check=True)
    return exe


def test_set_parsing_under_the_sanitizers(set_host):
    p = subprocess.run([str(set_host)], capture_output=True, text=True)
    assert p.returncode == 0 and p.stdout.startswith("ok "), p.stdout + p.stderr
    assert int(p.stdout.split()[1]) >= 45


def test_export_and_null_context():
    lib = native.load()
    assert "insitu_view_bind_packed_set" in native.EXPORTED_SYMBOLS
    text = HEADER.read_text()
    assert re.search(r"int\s+insitu_view_bind_packed_set\(insitu_ctx\*\s*ctx,\s*const void\*\s*const\*\s*streams,\s*"
                     r"const size_t\*\s*bytes,\s*int n\);", text)
    assert re.search(r"#define\s+INSITU_ABI_VERSION\s+12\b", text) and "an addition within ABI" in text
    fn = lib.insitu_view_bind_packed_set
    assert fn.restype is ctypes.c_int
    assert list(fn.argtypes) == [ctypes.c_void_p, ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_size_t), ctypes.c_int]
    _, _, good = _good()
    ptrs = (ctypes.c_void_p * 2)(good.ctypes.data, good.ctypes.data)
    sizes = (ctypes.c_size_t * 2)(good.nbytes, good.nbytes)
    assert fn(None, ptrs, sizes, 2) == -1
    assert b"insitu_view_bind_packed_set: null context" in lib.insitu_last_error(None)
    assert fn(None, None, None, 0) == -1
    assert lib.insitu_abi_version() == 12
