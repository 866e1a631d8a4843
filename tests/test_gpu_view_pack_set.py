"""GPU checks of insitu_view_bind_packed_set (csrc/insitu_view.cpp, vdi_view_merge.hip, vdi_pack.hip; DESIGN.md
section 9.8): a set of packed streams bound as one merged VDI straight from their sections.  The bound VDI is read back
through view_pack(PACK_FLOAT), and its bytes must equal vdi_io.pack_vdi of the plain loop's merge
(tests/test_pack_set.py loop_merge_set) of the unpacked streams; renders are compared bit for bit with tests/view_ref.
Covered: the 2x2 abutting bricks against INSITU_VIEW_MERGED of the same frame, both destination layouts, overlapping
bricks, a ragged window, one partial wave, 3, 9 and 32 streams of differing S and format (the merge kernel's three
instantiations), empty streams, 133 blocks per stream, the limit of 255 slots, two ranks' merged streams, a set of
one, every rejection, and a bind with a pipelined frame in flight."""
from __future__ import annotations

import ctypes
import struct

import numpy as np
import pytest
import torch

import view_binding as vb
from insitu_amd import native, scene
from insitu_amd.renderer import InSituContext, LocalGroup
from insitu_amd.vdi_io import PACK_FLOAT, PACK_HALF, pack_vdi
from test_pack_set import (layered_streams, loop_merge_set, merged_stream, random_streams, tie_streams,
                           zero_inside_count_stream)
from test_vdi_pack import PV, random_vdi, rejected_streams
from test_view_merge import scene_set
from view_binding import bits as _bits, fails as _fails, read_all as _read_all, set_bricks as _set_bricks

pytestmark = pytest.mark.gpu

W, H, S = vb.VDI_W, vb.VDI_H, vb.VDI_S
CAMS = vb.view_cameras()
G = vb.gen_camera()
SIZE = vb.OUT_SIZES[1]
FORMATS = (PACK_FLOAT, PACK_HALF)
COMPACT = native.OPT_VIEW_COMPACT
ZERO_STATS = ("view_slots", "view_overlaps", "view_entries", "view_bytes", "view_compact")


def _same_bytes(got, want, what):
    assert got.size == want.size, f"{what}: {got.size} bytes, expected {want.size}"
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, f"{what}: {bad.size} of {want.size} bytes differ, the first at {int(bad[0])}"


def _header(stream):
    """(W, H, S, E) of a packed stream."""
    raw = stream.tobytes()[:32]
    return struct.unpack_from("<3I", raw, 12) + struct.unpack_from("<Q", raw, 24)


def _layout_bytes(w, h, s, e, compact):
    """The formulas of include/insitu_hip.h (insitu_stats.view_bytes)."""
    px, tiles = w * h, ((w + 7) // 8) * ((h + 7) // 8)
    if compact:
        return 24 * max(e, 1) + 3 * px + 8 * ((px + 255) // 256) + tiles
    return 24 * px * s + px + tiles


def _bind_set(ctx, streams, compact=0):
    try:
        ctx.set_option(COMPACT, compact)
        ctx.view_bind_packed_set(streams)
    finally:
        ctx.set_option(COMPACT, 0)


def _check_set(ctx, streams, what, layouts=(0, 1)):
    """Bind `streams` in each layout: the bound VDI's FLOAT stream is the loop's merge of the unpacked streams, and
    the statistics describe it.  -> (that stream, the loop's (colour, depth, overlaps))."""
    want, merged = merged_stream(streams)
    w, h, s, e = _header(want)
    for compact in layouts:
        _bind_set(ctx, streams, compact)
        _same_bytes(ctx.view_pack(PACK_FLOAT), want, f"{what}, compact {compact}")
        st = ctx.stats()
        assert st["view_slots"] == s == merged[0].shape[2] and st["view_overlaps"] == merged[2], (what, compact)
        assert st["view_entries"] == e and st["view_compact"] == compact, (what, compact)
        assert st["view_bytes"] == _layout_bytes(w, h, s, e, compact), (what, compact)
        assert st["ms_view_bind"] > 0.0
    return want, merged


def _nothing_bound(ctx):
    cam = CAMS["yaw20"].native()
    img = np.empty((37, 50, 4), np.uint8)
    _fails(ctx, ctx.lib.insitu_view_render(ctx.h, ctypes.byref(cam), 50, 37, img.ctypes.data, img.nbytes), "no VDI bound")
    st = ctx.stats()
    assert all(st[k] == 0 for k in ZERO_STATS), {k: st[k] for k in ZERO_STATS}


def _brick_streams(ctx, n, fmt=PACK_FLOAT):
    out = []
    for b in range(n):
        ctx.view_bind(native.VIEW_BRICK, b)
        out.append(ctx.view_pack(fmt if not isinstance(fmt, (tuple, list)) else fmt[b]))
    return out


class _Frame:
    """A one-rank context's frame: every brick's sub-VDI as a packed stream, the sub-VDIs read back, and the FLOAT
    stream of INSITU_VIEW_MERGED of the same frame."""

    def __init__(self, ctx, scenes, cam, fmt=PACK_FLOAT):
        self.ctx, self.cam = ctx, cam
        _set_bricks(ctx, scenes)
        ctx.frame(cam)
        self.streams = _brick_streams(ctx, len(scenes), fmt)
        self.cols, self.deps = _read_all(ctx, len(scenes))
        ctx.view_bind(native.VIEW_MERGED)
        self.merged_stream = ctx.view_pack(PACK_FLOAT)
        self.stats = ctx.stats()


@pytest.fixture(scope="module")
def quad():
    """The 2x2 abutting bricks in one context."""
    with InSituContext(W, H, max_supersegments=S, bricks_per_rank=4) as ctx:
        yield _Frame(ctx, scene_set("abutting_2x2"), G)


@pytest.fixture(scope="module")
def other():
    """A context of other dimensions than anything bound into it."""
    with InSituContext(32, 16, max_supersegments=2) as ctx:
        yield ctx


def _renders(ctx, names=("yaw90", "yaw180", "cross"), cams=CAMS, size=SIZE):
    return [ctx.view_render(cams[name], *size, want_float=True) for name in names]


def test_abutting_quad(quad, other):
    _bind_set(other, quad.streams)
    got = other.view_pack(PACK_FLOAT)
    flat = loop_merge_set(quad.cols, quad.deps)
    _same_bytes(got, pack_vdi(flat[0], flat[1], vb.pv_of(G), PACK_FLOAT), "2x2 abutting bricks against the loop")
    _same_bytes(got, merged_stream(quad.streams)[0], "... of the unpacked streams")
    _same_bytes(got, quad.merged_stream, "... and INSITU_VIEW_MERGED of the same frame")
    st = other.stats()
    assert st["view_slots"] == 13 and st["view_overlaps"] == 0 and st["ms_view_bind"] > 0.0
    assert quad.stats["view_slots"] == 13
    seen = 0.0
    for name in ("yaw90", "yaw180", "cross"):
        ref_img, ref_acc = vb.render(flat[0], flat[1], G, CAMS[name], *SIZE)
        try:
            other.set_option(native.OPT_VIEW_SKIP, 0)
            _, walked = other.view_render(CAMS[name], *SIZE, want_float=True)
        finally:
            other.set_option(native.OPT_VIEW_SKIP, 1)
        img, acc = other.view_render(CAMS[name], *SIZE, want_float=True)
        bad = _bits(acc) != _bits(ref_acc)
        assert not bad.any(), f"{name}: {int(bad.sum())} of {bad.size} accumulator words differ"
        assert np.array_equal(img, ref_img), name
        assert np.array_equal(_bits(walked), _bits(acc)), name
        seen += float(ref_acc[..., 3].sum())
    assert seen > 1.0


def test_destination_layouts(quad, other):
    bound = {}
    for compact in (1, 0):
        _bind_set(other, quad.streams, compact)
        st = other.stats()
        packs = {fmt: other.view_pack(fmt) for fmt in FORMATS}
        w, h, s, e = _header(packs[PACK_FLOAT])
        assert (w, h, s) == (W, H, 13) and _header(packs[PACK_HALF]) == (w, h, s, e)
        assert st["view_compact"] == compact and st["view_entries"] == e and st["view_slots"] == s
        assert st["view_bytes"] == _layout_bytes(w, h, s, e, compact)
        bound[compact] = (packs, _renders(other))
    for fmt in FORMATS:
        _same_bytes(bound[1][0][fmt], bound[0][0][fmt], f"compact against dense, format {fmt}")
    _same_bytes(bound[0][0][PACK_FLOAT], quad.merged_stream, "both against INSITU_VIEW_MERGED")
    for (img1, acc1), (img0, acc0) in zip(bound[1][1], bound[0][1]):
        assert np.array_equal(_bits(acc1), _bits(acc0)) and np.array_equal(img1, img0)
    assert sum(float(acc[..., 3].sum()) for _, acc in bound[0][1]) > 1.0


def test_overlapping_pair(other):
    with InSituContext(W, H, max_supersegments=S, bricks_per_rank=2) as ctx:
        f = _Frame(ctx, scene_set("overlapping_pair"), G, fmt=(PACK_FLOAT, PACK_HALF))
        # (the second brick arrives as HALF: what must be bound is the merge of the streams, not of the frame)
        _, merged = _check_set(other, f.streams, "overlapping pair")
        assert other.stats()["view_overlaps"] == merged[2] > 0
        floats = _brick_streams(ctx, 2)
    _check_set(other, floats, "overlapping pair, both FLOAT", layouts=(0,))
    _same_bytes(other.view_pack(PACK_FLOAT), f.merged_stream, "against INSITU_VIEW_MERGED")
    assert other.stats()["view_overlaps"] == f.stats["view_overlaps"] > 0


def test_ragged_window(other):
    """50x37, S = 5: partial tiles on both axes and a partial block of 256 pixels."""
    rw, rh, rs = 50, 37, 5
    cam = scene.orbit_camera(rw, rh, radius=1.4, yaw_deg=30.0, pitch_deg=20.0, voxel_world=1.0 / 32)
    with InSituContext(rw, rh, max_supersegments=rs, bricks_per_rank=2) as ctx:
        f = _Frame(ctx, scene_set("abutting_pair", rw, rh), cam)
    _, merged = _check_set(other, f.streams, "ragged window")
    counts = np.count_nonzero(merged[1][:, :, 0::2], axis=2)
    assert counts.max() > rs and np.count_nonzero(counts[48:]) >= 20 and np.count_nonzero(counts[:, 32:]) >= 20
    _same_bytes(other.view_pack(PACK_FLOAT), f.merged_stream, "against INSITU_VIEW_MERGED")
    cams = vb.view_cameras(rw, rh)
    (img, acc), = _renders(other, ("yaw90",), cams, (41, 29))
    ref_img, ref_acc = vb.render(merged[0], merged[1], cam, cams["yaw90"], 41, 29)
    assert np.array_equal(_bits(acc), _bits(ref_acc)) and np.array_equal(img, ref_img)


def test_one_partial_wave(other):
    """9x7, S = 1 streams: 63 pixels."""
    gen = vb.gen_camera(9, 7)
    slabs = [(0.9760, 0.9799, (0.0, 0.0, 1.0, 0.6)), (0.9715, 0.9760, (1.0, 0.0, 0.0, 0.4)), (0.9800, 0.9810, (0.0, 1.0, 0.0, 0.2))]
    streams = [pack_vdi(*vb.slab_vdi([s], 9, 7, 1), vb.pv_of(gen), f) for s, f in zip(slabs, (PACK_FLOAT, PACK_HALF, PACK_FLOAT))]
    want, merged = _check_set(other, streams, "9x7, S = 1")
    assert _header(want) == (9, 7, 3, 63 * 3)
    assert merged[1][4, 3, 0::2].tolist() == [np.float32(0.9715), np.float32(0.9760), np.float32(0.9800)]
    cam = vb.view_cameras(9, 7)["yaw20"]
    img, acc = other.view_render(cam, 41, 29, want_float=True)
    ref_img, ref_acc = vb.render(merged[0], merged[1], gen, cam, 41, 29)
    assert np.array_equal(_bits(acc), _bits(ref_acc)) and np.array_equal(img, ref_img)
    assert ref_acc[..., 3].sum() > 1.0


@pytest.mark.parametrize("n", [3, 9, 32])
def test_random_sets(other, n):
    streams = random_streams(n, 200 + n)
    slots = [_header(s)[2] for s in streams]
    formats = [struct.unpack_from("<I", s.tobytes()[:16], 8)[0] for s in streams]
    assert set(slots) == ({1, 2, 3} if n == 3 else {1, 2, 3, 4})
    assert set(formats) == {PACK_FLOAT, PACK_HALF}
    _, merged = _check_set(other, streams, f"{n} random streams")
    starts = merged[1][:, :, 0::2]
    assert np.count_nonzero((starts[:, :, 1:] == starts[:, :, :-1]) & (starts[:, :, 1:] != 0)) > 0   # ties between streams
    assert merged[0].shape[2] > 4


def test_crafted_streams(other):
    want, merged = _check_set(other, tie_streams(), "a tie between streams 0 and 2")
    assert merged[0][2, 3, :, :2].tolist() == [[0, 0], [2, 0], [1, 0], [2, 1], [0, 1]]
    for fmt in FORMATS:
        want, merged = _check_set(other, [tie_streams()[1], zero_inside_count_stream(fmt)], "a zero start inside a count")
        assert _header(want) == (16, 8, 2, 2 * 128)


def test_empty_streams(other):
    gen, cam = vb.gen_camera(16, 8), vb.view_cameras(16, 8)["yaw20"]
    pv = vb.pv_of(gen)
    col, dep = vb.list_end_vdi()
    slab = vb.slab_vdi(vb.SLAB, 16, 8, 2)

    def empty(s, fmt):
        return pack_vdi(np.zeros((16, 8, s, 4), np.float32), np.zeros((16, 8, 2 * s), np.float32), pv, fmt)

    streams = [pack_vdi(col, dep, pv, PACK_FLOAT), empty(3, PACK_HALF), pack_vdi(*slab, pv, PACK_HALF)]
    _, merged = _check_set(other, streams, "an empty stream among others")
    img, acc = other.view_render(cam, 41, 29, want_float=True)
    ref_img, ref_acc = vb.render(merged[0], merged[1], gen, cam, 41, 29)
    assert np.array_equal(_bits(acc), _bits(ref_acc)) and np.array_equal(img, ref_img) and ref_acc[..., 3].sum() > 1.0
    _same_bytes(other.view_pack(PACK_FLOAT), merged_stream([streams[0], streams[2]])[0], "without the empty stream")
    want, _ = _check_set(other, [empty(3, PACK_FLOAT), empty(1, PACK_HALF), empty(255, PACK_FLOAT)], "only empty streams")
    assert _header(want) == (16, 8, 1, 0) and want.size == 128 + 128
    img, acc = other.view_render(cam, 41, 29, want_float=True)
    assert not img.any() and not acc.any()


def test_133_blocks_per_stream(other):
    """260x130: the scan's multi-step path, once per stream.  Bytes only."""
    streams = [pack_vdi(*random_vdi(260, 130, 2, 51), PV, PACK_FLOAT), pack_vdi(*random_vdi(260, 130, 2, 52), PV, PACK_HALF)]
    want, merged = _check_set(other, streams, "260x130")
    assert merged[0].shape[2] == 4 and _header(want)[3] > 60000


def test_slot_limit(other):
    want, _ = _check_set(other, layered_streams(128, 127), "128 + 127 entries")
    assert other.stats()["view_slots"] == 255 and _header(want)[2:] == (255, 255 * 128)
    for compact in (0, 1):
        with pytest.raises(RuntimeError, match="256"):
            _bind_set(other, layered_streams(128, 128), compact)
        _nothing_bound(other)
    # a good bind afterwards renders as the restatement does
    gen, cam = vb.gen_camera(16, 8), vb.view_cameras(16, 8)["yaw20"]
    col, dep = vb.list_end_vdi()
    slab = vb.slab_vdi(vb.SLAB, 16, 8, 6)
    streams = [pack_vdi(col, dep, vb.pv_of(gen), PACK_FLOAT), pack_vdi(*slab, vb.pv_of(gen), PACK_FLOAT)]
    _, merged = _check_set(other, streams, "after the rejected bind", layouts=(0,))
    img, acc = other.view_render(cam, 41, 29, want_float=True)
    ref_img, ref_acc = vb.render(merged[0], merged[1], gen, cam, 41, 29)
    assert np.array_equal(_bits(acc), _bits(ref_acc)) and np.array_equal(img, ref_img)
    assert ref_acc[..., 3].sum() > 1.0


def test_two_ranks(other):
    """Each rank of a two-rank group binds INSITU_VIEW_MERGED (its own two bricks) and packs; the two streams bound
    as a set are the flat merge of the four sub-VDIs, rank 0's bricks first (tests/test_pack_set.py:
    test_hierarchy_equals_the_flat_merge)."""
    scenes = scene_set("abutting_2x2")
    group = LocalGroup(2)
    ctxs = []
    try:
        for r in range(2):
            ctx = InSituContext(W, H, max_supersegments=S, bricks_per_rank=2, rank=r, nranks=2, local_group=group)
            ctxs.append(ctx)
            _set_bricks(ctx, scenes[2 * r:2 * r + 2])
        for ctx in ctxs:
            ctx.render(G)
        for ctx in ctxs:
            ctx.exchange()
        for ctx in ctxs:
            ctx.composite()
        for ctx in ctxs[::-1]:
            ctx.gather(want_image=False)
        cols, deps, streams = [], [], []
        for ctx in ctxs:
            c, d = _read_all(ctx, 2)
            cols += c
            deps += d
            ctx.view_bind(native.VIEW_MERGED)
            streams.append(ctx.view_pack(PACK_FLOAT))
    finally:
        for c in ctxs:
            c.close()
        group.close()
    assert _header(streams[1])[2] > S   # (a merged bind has its own S_m: rank 1's two bricks share pixels)
    flat = loop_merge_set(cols, deps)
    assert flat[0].shape[2] == 13
    for compact in (0, 1):
        _bind_set(other, streams, compact)
        _same_bytes(other.view_pack(PACK_FLOAT), pack_vdi(flat[0], flat[1], vb.pv_of(G), PACK_FLOAT), "two ranks' streams")
        assert other.stats()["view_slots"] == 13 and other.stats()["view_overlaps"] == 0


def test_set_of_one_is_bind_packed(quad, other):
    for fmt in FORMATS:
        quad.ctx.view_bind(native.VIEW_BRICK, 1)
        stream = quad.ctx.view_pack(fmt)
        for compact in (0, 1):
            try:
                other.set_option(COMPACT, compact)
                other.view_bind_packed(stream)
            finally:
                other.set_option(COMPACT, 0)
            one = ({f: other.view_pack(f) for f in FORMATS}, _renders(other))
            _bind_set(other, [stream], compact)
            assert other.stats()["view_slots"] == S and other.stats()["view_compact"] == compact
            for f in FORMATS:
                _same_bytes(other.view_pack(f), one[0][f], f"a set of one, format {fmt} to {f}, compact {compact}")
            for (img, acc), (wimg, wacc) in zip(_renders(other), one[1]):
                assert np.array_equal(_bits(acc), _bits(wacc)) and np.array_equal(img, wimg)
            assert sum(float(acc[..., 3].sum()) for _, acc in one[1]) > 1.0


REASONS = {"bad magic": "bad magic", "version 2": "unknown version", "format 2": "unknown format",
           "S = 0": "S must be in [1,255]", "S = 256": "S must be in [1,255]", "one byte short": "size differs",
           "one byte long": "size differs", "a count above S, the sum kept": "a count of 7 exceeds S = 6",
           "counts that add up to less than E": "add up to", "counts that add up to more than E": "add up to"}


def _raw_bind(ctx, streams, n=None):
    arrs = [None if s is None else np.ascontiguousarray(s) for s in streams]
    ptrs = (ctypes.c_void_p * max(len(arrs), 1))(*[None if a is None else a.ctypes.data for a in arrs])
    sizes = (ctypes.c_size_t * max(len(arrs), 1))(*[0 if a is None else a.nbytes for a in arrs])
    return ctx.lib.insitu_view_bind_packed_set(ctx.h, ptrs, sizes, len(arrs) if n is None else n)


def test_rejections(other):
    col, dep = vb.list_end_vdi()
    good = pack_vdi(col, dep, PV, PACK_FLOAT)
    good_set = [good, pack_vdi(*vb.slab_vdi(vb.SLAB, 16, 8, 2), PV, PACK_HALF), good]
    want = merged_stream(good_set)[0]
    bad = rejected_streams()
    assert set(bad) == set(REASONS)
    pv_bit = PV.copy()
    pv_bit.view(np.uint32)[11] ^= 1
    cases = [(name, [good, stream, good], None, ("stream 1 rejected", REASONS[name])) for name, stream in bad.items()]
    cases += [("W differs", [good, pack_vdi(*random_vdi(17, 8, 6, 1), PV), good], None, ("stream 1 rejected", "W and H differ")),
              ("H differs", [good, good, pack_vdi(*random_vdi(16, 9, 6, 1), PV)], None, ("stream 2 rejected", "W and H differ")),
              ("pv_g differs in one bit", [good, pack_vdi(col, dep, pv_bit), good], None, ("stream 1 rejected", "generating camera")),
              ("a null entry", [good, None, good], None, ("stream 1 rejected", "null stream")),
              ("a bad only stream", [bad["bad magic"]], None, ("stream 0 rejected", "bad magic")),
              ("n = 0", [good], 0, ("0 streams", "needs 1 to 32")),
              ("n = 33", [good] * 33, None, ("33 streams", "needs 1 to 32"))]
    for i, (name, streams, n, texts) in enumerate(cases):
        compact = i % 2
        try:
            other.set_option(COMPACT, compact)
            other.view_bind_packed_set(good_set)
            _same_bytes(other.view_pack(PACK_FLOAT), want, f"good bind before '{name}'")
            rc = _raw_bind(other, streams, n)
        finally:
            other.set_option(COMPACT, 0)
        for text in ("insitu_view_bind_packed_set",) + texts:
            _fails(other, rc, text)
        _nothing_bound(other)
    lib = other.lib
    sizes = (ctypes.c_size_t * 2)(good.nbytes, good.nbytes)
    ptrs = (ctypes.c_void_p * 2)(good.ctypes.data, good.ctypes.data)
    other.view_bind_packed_set(good_set)
    _fails(other, lib.insitu_view_bind_packed_set(other.h, None, sizes, 2), "null argument")
    _nothing_bound(other)
    other.view_bind_packed_set(good_set)
    _fails(other, lib.insitu_view_bind_packed_set(other.h, ptrs, None, 2), "null argument")
    _nothing_bound(other)
    other.view_bind_packed_set([good] * 32)   # 32 is the most, and binds
    assert other.stats()["view_slots"] == 32 * 6
    other.view_bind_packed_set(good_set)
    _same_bytes(other.view_pack(PACK_FLOAT), want, "a good bind after them all")


def test_pipelined_frame_in_flight(quad):
    """After a re-ingest and with a pipelined frame in flight, a set is bound on the view's own stream; two more
    frames leave the bound bytes as they are."""
    scenes = scene_set("overlapping_pair")
    want = merged_stream(quad.streams)[0]
    with InSituContext(W, H, max_supersegments=S, bricks_per_rank=2) as ctx:
        _set_bricks(ctx, scenes)
        assert ctx.frame_pipelined(G)[0] == -1
        ctx.set_brick(0, torch.from_numpy(scenes[1]["vol"].view(np.int16)).cuda(), scenes[0]["model"], dtype=native.U16)
        assert ctx.frame_pipelined(CAMS["yaw90"])[0] == 0      # frame 0 is complete, frame 1 in flight
        for compact in (1, 0):
            _bind_set(ctx, quad.streams, compact)
            _same_bytes(ctx.view_pack(PACK_FLOAT), want, f"bound with frame 1 in flight, compact {compact}")
        assert ctx.frame_pipelined(CAMS["yaw180"])[0] == 1
        assert ctx.pipeline_flush()[0] == 2
        _same_bytes(ctx.view_pack(PACK_FLOAT), want, "after two more frames")
        assert ctx.stats()["view_slots"] == 13
