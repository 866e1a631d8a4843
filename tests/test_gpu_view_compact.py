"""GPU checks of the compact view layout (INSITU_OPT_VIEW_COMPACT): a bound VDI held as its
stored entries alone, entry i of pixel p at boff[p >> 8] + loc[p] + i.  The yardsticks are the dense layout of the
same build, the CPU restatement of the viewer (tests/view_ref through view_binding.render) and the numpy codec
(vdi_io.pack_vdi); the bar is equality of bytes and of float bit patterns.  Every bind source is bound dense and
compact and must pack to the same streams and render the same accumulators; the shapes at which an index can go wrong
(one partial block, the 16-bit bound of loc, several steps of the block scan, E = 0); the three statistics; the
option's semantics; every rejected stream; the snapshot under pipelined frames."""
from __future__ import annotations

import ctypes
import struct

import numpy as np
import pytest
import torch

import view_binding as vb
from insitu_amd import native
from insitu_amd.renderer import InSituContext
from insitu_amd.vdi_io import PACK_FLOAT, PACK_HALF, pack_vdi, unpack_vdi
from scenes import make_scene
from test_vdi_pack import empty_vdi, random_vdi, rejected_streams
from test_view_merge import loop_merge, scene_set
from view_binding import bits as _bits, fails as _fails, random_set as _random_set, read_all as _read_all, set_bricks as _set_bricks

pytestmark = pytest.mark.gpu

W, H, S, S_OUT = vb.VDI_W, vb.VDI_H, vb.VDI_S, 4
RW, RH, RS = 50, 37, 5
G = vb.gen_camera()
SIZE = vb.OUT_SIZES[1]
# far cameras and the one behind G's eye at 50x37, and the generating camera at 128x96 (rays in cell planes)
VIEWS = (("yaw90", SIZE), ("yaw180", SIZE), ("cross", SIZE), ("same", (128, 96)))
FORMATS = (PACK_FLOAT, PACK_HALF)
COMPACT = native.OPT_VIEW_COMPACT


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


def _views(ctx, cams):
    return [ctx.view_render(cams[name], *size, want_float=True) for name, size in VIEWS]


def _same_views(got, want, what):
    for (name, size), (img, acc), (wimg, wacc) in zip(VIEWS, got, want):
        bad = _bits(acc) != _bits(wacc)
        assert not bad.any(), f"{what}, {name} at {size}: {int(bad.sum())} of {bad.size} accumulator words differ"
        assert np.array_equal(img, wimg), f"{what}, {name} at {size}: images differ"


def _same_bytes(got, want, what):
    assert got.size == want.size, f"{what}: {got.size} bytes, expected {want.size}"
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, f"{what}: {bad.size} of {want.size} bytes differ, the first at {int(bad[0])}"


def _bound(ctx, compact, cams):
    """What the tests compare of a bound VDI: both streams, the views and the statistics."""
    st = ctx.stats()
    assert st["view_compact"] == compact
    packs = {fmt: ctx.view_pack(fmt) for fmt in FORMATS}
    w, h, s, e = _header(packs[PACK_FLOAT])
    assert _header(packs[PACK_HALF]) == (w, h, s, e)
    assert st["view_slots"] == s and st["view_entries"] == e
    assert st["view_bytes"] == _layout_bytes(w, h, s, e, compact), (st["view_bytes"], w, h, s, e, compact)
    return {"packs": packs, "views": _views(ctx, cams), "stats": st}


def _dense_and_compact(ctx, bind, what, vdi=None, cams=None, merged=False, visible=True):
    """bind() with the option 0, then with the option 1: the same streams, the same views, and both the numpy
    codec's stream and the restatement's views of vdi = (colour, depth, generating camera) when there is one."""
    cams = cams or vb.view_cameras()
    try:
        ctx.set_option(COMPACT, 0)
        bind()
        dense = _bound(ctx, 0, cams)
        ctx.set_option(COMPACT, 1)
        bind()
        compact = _bound(ctx, 1, cams)
        ctx.set_option(native.OPT_VIEW_SKIP, 0)
        walked = _views(ctx, cams)
    finally:
        ctx.set_option(native.OPT_VIEW_SKIP, 1)
        ctx.set_option(COMPACT, 0)
    for fmt in FORMATS:
        _same_bytes(compact["packs"][fmt], dense["packs"][fmt], f"{what}, format {fmt}, compact against dense")
    _same_views(compact["views"], dense["views"], f"{what}, compact against dense")
    _same_views(walked, compact["views"], f"{what}, compact, skip off against on")
    if vdi is not None:
        col, dep, gen = vdi
        _same_bytes(compact["packs"][PACK_FLOAT], pack_vdi(col, dep, vb.pv_of(gen), PACK_FLOAT), f"{what}, numpy codec")
        ref = [vb.render(col, dep, gen, cams[name], *size) for name, size in VIEWS]
        _same_views(compact["views"], ref, f"{what}, compact against view_ref")
    if visible:
        assert sum(float(acc[..., 3].sum()) for _, acc in dense["views"]) > 1.0, what   # (the cameras see something)
    if merged:
        for key in ("view_slots", "view_overlaps"):
            assert compact["stats"][key] == dense["stats"][key], key
    assert compact["stats"]["view_entries"] == dense["stats"]["view_entries"]
    return dense, compact


@pytest.fixture(scope="module")
def other():
    """A context of other dimensions than anything bound into it."""
    with InSituContext(32, 16, max_supersegments=2) as ctx:
        yield ctx


# ---------------------------------------------------------------- every bind source, compact against dense
def test_brick_source():
    sc = make_scene(n=32, W=W, H=H, origin=(-0.5, -0.5, -0.5))
    with InSituContext(W, H, max_supersegments=S) as ctx:
        _set_bricks(ctx, [sc])
        ctx.frame(G)
        vdi = (ctx.read(native.BUF_VDI_COLOR), ctx.read(native.BUF_VDI_DEPTH), G)
        counts = np.count_nonzero(vdi[1][:, :, 0::2], axis=2)
        assert counts.max() == S and counts.min() == 0
        _dense_and_compact(ctx, lambda: ctx.view_bind(native.VIEW_BRICK, 0), "INSITU_VIEW_BRICK", vdi)


def test_gathered_source():
    a = make_scene(n=32, W=W, H=H, origin=(-0.5, -0.5, -0.5))
    b = make_scene(n=32, W=W, H=H, seed=7, origin=(0.0, -0.25, -0.75))
    with InSituContext(W, H, max_supersegments=S, bricks_per_rank=2, composite_vdi=True,
                       max_output_supersegments=S_OUT) as ctx:
        _set_bricks(ctx, [a, b])
        ctx.frame(G)
        vdi = (ctx.read(native.BUF_GATHERED_COLOR), ctx.read(native.BUF_GATHERED_DEPTH), G)
        assert vdi[0].shape[2] == S_OUT
        _dense_and_compact(ctx, lambda: ctx.view_bind(native.VIEW_GATHERED), "INSITU_VIEW_GATHERED", vdi)


def test_host_source_ragged(other):
    col, dep = random_vdi(RW, RH, RS, 22)
    gen = vb.gen_camera(RW, RH)
    _dense_and_compact(other, lambda: other.view_bind_host(col, dep, gen), "insitu_view_bind_host 50x37", (col, dep, gen),
                       vb.view_cameras(RW, RH))


def test_host_source_list_ends(other):
    col, dep = vb.list_end_vdi()
    gen = vb.gen_camera(16, 8)
    _dense_and_compact(other, lambda: other.view_bind_host(col, dep, gen), "list_end_vdi", (col, dep, gen),
                       vb.view_cameras(16, 8))


def test_merged_source_and_its_bytes():
    scenes = scene_set("abutting_2x2")
    with InSituContext(W, H, max_supersegments=S, bricks_per_rank=4) as ctx:
        _set_bricks(ctx, scenes)
        ctx.frame(G)
        cols, deps = _read_all(ctx, 4)
        mc, md, overlaps = loop_merge(cols, deps)
        dense, compact = _dense_and_compact(ctx, lambda: ctx.view_bind(native.VIEW_MERGED), "INSITU_VIEW_MERGED", (mc, md, G),
                                            merged=True)
        assert compact["stats"]["view_slots"] == 13 and compact["stats"]["view_overlaps"] == overlaps == 0
        assert compact["stats"]["ms_view_bind"] > 0.0
        # S_m = 13 is the one longest list, most pixels hold far fewer: compact is smaller by construction
        print(f"merged quad: dense {dense['stats']['view_bytes']} bytes, compact {compact['stats']['view_bytes']} bytes, "
              f"{compact['stats']['view_entries']} entries")
        assert compact["stats"]["view_bytes"] < dense["stats"]["view_bytes"]


@pytest.mark.parametrize("n", [3, 9, 32])
def test_host_set_source(other, n):
    cols, deps = _random_set(n, 100 + n)
    mc, md, overlaps = loop_merge(cols, deps)
    gen = vb.gen_camera(16, 8)
    dense, compact = _dense_and_compact(other, lambda: other.view_bind_host_set(cols, deps, gen), f"host set of {n}",
                                        (mc, md, gen), vb.view_cameras(16, 8), merged=True)
    assert compact["stats"]["view_slots"] == mc.shape[2] > 2 and compact["stats"]["view_overlaps"] == overlaps


@pytest.mark.parametrize("fmt", FORMATS)
def test_packed_source(other, fmt):
    col, dep = random_vdi(RW, RH, RS, 22)
    gen = vb.gen_camera(RW, RH)
    stream = pack_vdi(col, dep, vb.pv_of(gen), fmt)
    ucol, udep, pv, ufmt = unpack_vdi(stream)
    assert ufmt == fmt and np.array_equal(_bits(pv), _bits(vb.pv_of(gen)))
    dense, compact = _dense_and_compact(other, lambda: other.view_bind_packed(stream), f"packed stream, format {fmt}",
                                        (ucol, udep, gen), vb.view_cameras(RW, RH))
    _same_bytes(compact["packs"][fmt], stream, "the stream bound, packed again")
    assert compact["stats"]["ms_pack"] >= 0.0 and compact["stats"]["ms_view_bind"] > 0.0


# ---------------------------------------------------------------- shapes where the index can go wrong
SHAPES = {
    "9x7_S1": lambda: vb.slab_vdi(vb.SLAB, 9, 7, 1),              # one partial wave, one partial block
    "32x8_S255_full": lambda: vb.layered_vdi(255, 32, 8),        # exactly one block; loc reaches 65 025, the u16 bound
    "20x12_S255": lambda: vb.layered_vdi(255, 20, 12),           # large in-block offsets in a partial block
    "empty": empty_vdi,                                          # E = 0
    "random_260x130_S2": lambda: random_vdi(260, 130, 2, 21),    # 133 blocks: three steps of the scan
    "random_400x170_S1": lambda: random_vdi(400, 170, 1, 23),    # 266 blocks: the scan's second batch of loads
}
RENDERED = ("9x7_S1", "32x8_S255_full", "20x12_S255")
LSB = 1.0


@pytest.mark.parametrize("name", list(SHAPES))
def test_shapes(other, name):
    col, dep = SHAPES[name]()
    w, h, s = col.shape[:3]
    gen, cam = vb.gen_camera(w, h), vb.view_cameras(w, h)["yaw90"]
    pv = vb.pv_of(gen)
    want = {fmt: pack_vdi(col, dep, pv, fmt) for fmt in FORMATS}
    entries = _header(want[PACK_FLOAT])[3]
    try:
        other.set_option(COMPACT, 1)
        for how in ("host", "packed"):
            if how == "host":
                other.view_bind_host(col, dep, gen)
            else:
                other.view_bind_packed(want[PACK_FLOAT])
            st = other.stats()
            assert st["view_compact"] == 1 and st["view_entries"] == entries and st["view_slots"] == s
            assert st["view_bytes"] == _layout_bytes(w, h, s, entries, True)
            for fmt in FORMATS:
                assert other.lib.insitu_view_pack_bytes(other.h, fmt) == want[fmt].size
                _same_bytes(other.view_pack(fmt), want[fmt], f"{name} bound from {how}, format {fmt}")
            if name == "empty":
                assert entries == 0 and want[PACK_FLOAT].size == 128 + 64
                img, acc = other.view_render(cam, 41, 29, want_float=True)
                assert not acc.any() and not img.any()
            if name in RENDERED:
                img, acc = other.view_render(cam, 41, 29, want_float=True)
                ref_img, ref_acc = vb.render(col, dep, gen, cam, 41, 29)
                assert np.array_equal(_bits(acc), _bits(ref_acc)) and np.array_equal(img, ref_img), (name, how)
                assert ref_acc[..., 3].sum() > 1.0
                if s == 255:
                    err = vb.lsb_error(img, vb.analytic_slabs(vb.SLAB, gen, cam, 41, 29, w, h))
                    print(f"{name} from {how}: {err:.3f} LSB from the analytic slab")
                    assert err <= LSB
        if name == "32x8_S255_full":
            counts = want[PACK_FLOAT][128:128 + w * h]
            assert np.all(counts == 255) and int(counts[:-1].astype(np.int64).sum()) == 65025
    finally:
        other.set_option(COMPACT, 0)


# ---------------------------------------------------------------- the option
def test_option_values_and_when_it_takes_effect(other):
    lib = other.lib
    col, dep = vb.list_end_vdi()
    gen, cam = vb.gen_camera(16, 8), vb.view_cameras(16, 8)["yaw20"]
    _, want = vb.render(col, dep, gen, cam, 41, 29)
    try:
        for value in (2, -1):
            _fails(other, lib.insitu_set_option(other.h, COMPACT, value), "out of range")
        for first in (0, 1):
            other.set_option(COMPACT, first)
            other.view_bind_host(col, dep, gen)
            stream = other.view_pack(PACK_HALF)
            other.set_option(COMPACT, 1 - first)          # the bound VDI keeps its layout
            assert other.stats()["view_compact"] == first
            _, acc = other.view_render(cam, 41, 29, want_float=True)
            assert np.array_equal(_bits(acc), _bits(want)), first
            assert np.array_equal(other.view_pack(PACK_HALF), stream)
            assert other.stats()["view_compact"] == first
            other.view_bind_host(col, dep, gen)           # the next bind takes the option
            assert other.stats()["view_compact"] == 1 - first
            _, acc = other.view_render(cam, 41, 29, want_float=True)
            assert np.array_equal(_bits(acc), _bits(want)), first
    finally:
        other.set_option(COMPACT, 0)


def test_environment_seeds_the_option(monkeypatch):
    col, dep = vb.list_end_vdi()
    gen = vb.gen_camera(16, 8)
    monkeypatch.setenv("INSITU_VIEW_COMPACT", "1")
    with InSituContext(32, 16, max_supersegments=2) as ctx:
        ctx.view_bind_host(col, dep, gen)
        assert ctx.stats()["view_compact"] == 1
        ctx.set_option(COMPACT, 0)                        # insitu_set_option overrides the seed
        ctx.view_bind_host(col, dep, gen)
        assert ctx.stats()["view_compact"] == 0
    monkeypatch.setenv("INSITU_VIEW_COMPACT", "2")
    with pytest.raises(RuntimeError, match="INSITU_VIEW_COMPACT=2 out of range"):
        InSituContext(32, 16, max_supersegments=2)
    monkeypatch.delenv("INSITU_VIEW_COMPACT")
    with InSituContext(32, 16, max_supersegments=2) as ctx:
        ctx.view_bind_host(col, dep, gen)
        assert ctx.stats()["view_compact"] == 0           # dense is the default


def test_buffers_grow_across_layouts():
    """A dense bind, a smaller compact one and a larger compact one in one context, in that order."""
    small = vb.list_end_vdi()                                       # 16x8, S = 6
    mid = random_vdi(RW, RH, RS, 22)                                # 50x37, S = 5
    big = random_vdi(260, 130, 2, 21)                               # 33 800 pixels
    with InSituContext(32, 16, max_supersegments=2) as ctx:
        for compact, (col, dep) in ((0, mid), (1, small), (1, big), (0, small), (1, mid)):
            w, h = col.shape[:2]
            gen, cam = vb.gen_camera(w, h), vb.view_cameras(w, h)["yaw90"]
            ctx.set_option(COMPACT, compact)
            ctx.view_bind_host(col, dep, gen)
            assert ctx.stats()["view_compact"] == compact
            _, acc = ctx.view_render(cam, 41, 29, want_float=True)
            _, want = vb.render(col, dep, gen, cam, 41, 29)
            assert np.array_equal(_bits(acc), _bits(want)), (compact, w, h)
            _same_bytes(ctx.view_pack(PACK_FLOAT), pack_vdi(col, dep, vb.pv_of(gen), PACK_FLOAT), f"{w}x{h}, compact {compact}")


# ---------------------------------------------------------------- validation
def _nothing_bound(ctx, ncam):
    img = np.empty((29, 41, 4), np.uint8)
    _fails(ctx, ctx.lib.insitu_view_render(ctx.h, ctypes.byref(ncam), 41, 29, img.ctypes.data, img.nbytes), "no VDI bound")
    _fails(ctx, ctx.lib.insitu_view_pack(ctx.h, PACK_FLOAT, img.ctypes.data, img.nbytes, None), "no VDI bound")
    st = ctx.stats()
    assert st["view_entries"] == 0 and st["view_bytes"] == 0 and st["view_compact"] == 0 and st["view_slots"] == 0


def test_rejected_streams_leave_nothing_bound(other):
    lib = other.lib
    col, dep = vb.list_end_vdi()
    gen, cam = vb.gen_camera(16, 8), vb.view_cameras(16, 8)["yaw20"]
    good = pack_vdi(col, dep, vb.pv_of(gen), PACK_FLOAT)
    _, want = vb.render(col, dep, gen, cam, 41, 29)
    assert want[..., 3].sum() > 1.0
    ncam = cam.native()
    on_device = {"a count above S, the sum kept": "exceeds S", "counts that add up to less than E": "add up to",
                 "counts that add up to more than E": "add up to"}
    streams = rejected_streams()
    assert set(on_device) <= set(streams)
    try:
        other.set_option(COMPACT, 1)
        for name, stream in streams.items():
            other.view_bind_packed(good)
            assert other.stats()["view_compact"] == 1
            stream = np.ascontiguousarray(stream)
            _fails(other, lib.insitu_view_bind_packed(other.h, stream.ctypes.data, stream.nbytes), "stream rejected")
            assert on_device.get(name, "") in lib.insitu_last_error(other.h).decode(), name
            _nothing_bound(other, ncam)
        _fails(other, lib.insitu_view_bind_packed(other.h, None, 1000), "stream rejected")
        other.view_bind_packed(good)
        _, acc = other.view_render(cam, 41, 29, want_float=True)
        assert np.array_equal(_bits(acc), _bits(want))
        _same_bytes(other.view_pack(PACK_FLOAT), good, "a good compact bind after the rejected ones")
    finally:
        other.set_option(COMPACT, 0)


def test_slot_limit(other):
    gen, cam = vb.gen_camera(16, 8), vb.view_cameras(16, 8)["yaw20"]
    a = vb.layered_vdi(128, 16, 8)
    b = vb.layered_vdi(127, 16, 8, 128)
    ncam = cam.native()
    try:
        other.set_option(COMPACT, 1)
        other.view_bind_host_set([a[0], b[0]], [a[1], b[1]], gen)
        st = other.stats()
        assert st["view_slots"] == 255 and st["view_compact"] == 1 and st["view_entries"] == 16 * 8 * 255
        merged = loop_merge([a[0], b[0]], [a[1], b[1]])
        _same_bytes(other.view_pack(PACK_FLOAT), pack_vdi(merged[0], merged[1], vb.pv_of(gen), PACK_FLOAT), "128 + 127 entries")
        cp = (ctypes.c_void_p * 2)(a[0].ctypes.data, a[0].ctypes.data)
        dp = (ctypes.c_void_p * 2)(a[1].ctypes.data, a[1].ctypes.data)
        _fails(other, other.lib.insitu_view_bind_host_set(other.h, cp, dp, 2, 16, 8, 128, ctypes.byref(gen.native())), "256")
        _nothing_bound(other, ncam)
        # a good bind afterwards renders as the restatement does
        col, dep = vb.list_end_vdi()
        slab = vb.slab_vdi(vb.SLAB, 16, 8, 6)
        other.view_bind_host_set([col, slab[0]], [dep, slab[1]], gen)
        merged = loop_merge([col, slab[0]], [dep, slab[1]])
        img, acc = other.view_render(cam, 41, 29, want_float=True)
        ref_img, ref_acc = vb.render(merged[0], merged[1], gen, cam, 41, 29)
        assert np.array_equal(_bits(acc), _bits(ref_acc)) and np.array_equal(img, ref_img)
        assert ref_acc[..., 3].sum() > 1.0 and other.stats()["view_compact"] == 1
    finally:
        other.set_option(COMPACT, 0)


# ---------------------------------------------------------------- the snapshot
def test_snapshot_is_independent_of_the_frame_loop():
    """A compact MERGED bind of frame 0 with frame 1 in flight; a re-ingest and two more pipelined frames leave its
    bytes alone; a fresh bind then holds the completed frame's lists and camera."""
    from insitu_amd import scene
    scenes = scene_set("overlapping_pair")
    cams = [scene.orbit_camera(W, H, yaw_deg=30.0 + 41.0 * i, pitch_deg=20.0 - 7.0 * i, voxel_world=1.0 / 32)
            for i in range(4)]
    with InSituContext(W, H, max_supersegments=S, bricks_per_rank=2) as ctx:
        _set_bricks(ctx, scenes)
        ctx.set_option(COMPACT, 1)
        assert ctx.frame_pipelined(cams[0])[0] == -1
        assert ctx.frame_pipelined(cams[1])[0] == 0               # frame 0 is complete, frame 1 in flight
        ctx.view_bind(native.VIEW_MERGED)
        assert ctx.stats()["view_compact"] == 1
        cols, deps = _read_all(ctx, 2)
        merged = loop_merge(cols, deps)
        first = {fmt: ctx.view_pack(fmt) for fmt in FORMATS}
        _same_bytes(first[PACK_FLOAT], pack_vdi(merged[0], merged[1], vb.pv_of(cams[0]), PACK_FLOAT), "frame 0")
        assert ctx.stats()["view_overlaps"] == merged[2] > 0
        assert ctx.frame_pipelined(cams[2])[0] == 1
        ctx.set_brick(0, torch.from_numpy(scenes[1]["vol"].view(np.int16)).cuda(), scenes[0]["model"], dtype=native.U16)
        assert ctx.frame_pipelined(cams[3])[0] == 2               # frame 3, of the re-ingested brick, is in flight
        for fmt in FORMATS:
            assert np.array_equal(ctx.view_pack(fmt), first[fmt]), fmt
        ctx.view_bind(native.VIEW_MERGED)                         # frame 2, the completed one
        cols2, deps2 = _read_all(ctx, 2)
        assert not np.array_equal(deps2[0], deps[0])
        merged2 = loop_merge(cols2, deps2)
        _same_bytes(ctx.view_pack(PACK_FLOAT), pack_vdi(merged2[0], merged2[1], vb.pv_of(cams[2]), PACK_FLOAT), "frame 2")
        assert ctx.stats()["view_compact"] == 1
        assert ctx.pipeline_flush()[0] == 3
