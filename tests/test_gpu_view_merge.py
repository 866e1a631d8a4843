"""GPU checks of the merged bind (INSITU_VIEW_MERGED, insitu_view_bind_host_set; csrc/vdi_view_merge.hip, DESIGN.md
section 9.6).  The bound VDI is read back through view_pack(PACK_FLOAT), and its bytes must equal vdi_io.pack_vdi of
the plain loop's merge (tests/test_view_merge.py loop_merge) of the sub-VDIs insitu_read returns: every count, entry
and slot order, and the generating camera, without going through a render.  On top of that: renders against the CPU
restatement bit for bit, the generating camera against the frame's own flatten, the host set against the device
bind, a ragged window, 3, 9 and 32 lists (the kernel's three instantiations), the limit of 255 slots, merge_bricks
and multi-rank contexts, a pipelined frame in flight, and the error paths."""
from __future__ import annotations

import ctypes

import numpy as np
import pytest
import torch

import view_binding as vb
from insitu_amd import native, scene
from insitu_amd.renderer import InSituContext, LocalGroup
from insitu_amd.vdi_io import PACK_FLOAT, pack_vdi
from test_view_merge import loop_merge, scene_set
from view_binding import bits as _bits, fails as _fails, random_set as _random_set, read_all as _read_all, set_bricks as _set_bricks

pytestmark = pytest.mark.gpu

W, H, S = vb.VDI_W, vb.VDI_H, vb.VDI_S
CAMS = vb.view_cameras()
G = vb.gen_camera()
SIZE = vb.OUT_SIZES[1]


def _nothing_bound(ctx):
    cam = CAMS["yaw20"].native()
    img = np.empty((37, 50, 4), np.uint8)
    _fails(ctx, ctx.lib.insitu_view_render(ctx.h, ctypes.byref(cam), 50, 37, img.ctypes.data, img.nbytes), "no VDI bound")


def _assert_packed(ctx, merged, gen, what):
    """The bound VDI's FLOAT stream equals the numpy codec's of `merged` (colour, depth, ...) with gen's camera."""
    want = pack_vdi(merged[0], merged[1], vb.pv_of(gen), PACK_FLOAT)
    got = ctx.view_pack(PACK_FLOAT)
    assert got.size == want.size, f"{what}: {got.size} bytes, expected {want.size}"
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, f"{what}: {bad.size} of {want.size} bytes differ, the first at {int(bad[0])}"
    return got


class _Merged:
    """A one-rank context whose sub-VDIs are bound with INSITU_VIEW_MERGED: their readback, the loop's merge of it
    and the frame's own image."""

    def __init__(self, ctx, scenes, cam):
        self.ctx, self.cam = ctx, cam
        _set_bricks(ctx, scenes)
        self.image = ctx.frame(cam, want_image=True)
        ctx.view_bind(native.VIEW_MERGED)
        self.stats = ctx.stats()
        self.cols, self.deps = _read_all(ctx, len(scenes))
        self.merged = loop_merge(self.cols, self.deps)


@pytest.fixture(scope="module")
def quad():
    """The 2x2 abutting bricks in one context."""
    scenes = scene_set("abutting_2x2")
    with InSituContext(W, H, max_supersegments=S, bricks_per_rank=4) as ctx:
        yield _Merged(ctx, scenes, G)


@pytest.fixture(scope="module")
def pair():
    """Two bricks that overlap in space."""
    scenes = scene_set("overlapping_pair")
    with InSituContext(W, H, max_supersegments=S, bricks_per_rank=2) as ctx:
        yield _Merged(ctx, scenes, G)


@pytest.fixture(scope="module")
def other():
    """A context of other dimensions than anything bound into it."""
    with InSituContext(32, 16, max_supersegments=2) as ctx:
        yield ctx


def test_abutting_quad(quad):
    ctx = quad.ctx
    _assert_packed(ctx, quad.merged, G, "2x2 abutting bricks")
    assert quad.stats["view_slots"] == 13 and quad.merged[0].shape[2] == 13
    assert quad.stats["view_overlaps"] == 0 and quad.merged[2] == 0
    assert quad.stats["ms_view_bind"] > 0.0
    seen = 0.0
    for name in ("yaw90", "yaw180", "cross"):
        ref_img, ref_acc = vb.render(quad.merged[0], quad.merged[1], G, CAMS[name], *SIZE)
        try:
            ctx.set_option(native.OPT_VIEW_SKIP, 0)
            _, walked = ctx.view_render(CAMS[name], *SIZE, want_float=True)
        finally:
            ctx.set_option(native.OPT_VIEW_SKIP, 1)
        img, acc = ctx.view_render(CAMS[name], *SIZE, want_float=True)
        bad = _bits(acc) != _bits(ref_acc)
        assert not bad.any(), f"{name}: {int(bad.sum())} of {bad.size} accumulator words differ"
        assert np.array_equal(img, ref_img), name
        assert np.array_equal(_bits(walked), _bits(acc)), name
        seen += float(ref_acc[..., 3].sum())
    assert seen > 1.0


def test_overlapping_pair(pair):
    _assert_packed(pair.ctx, pair.merged, G, "overlapping pair")
    assert pair.stats["view_slots"] == pair.merged[0].shape[2]
    assert pair.stats["view_overlaps"] == pair.merged[2] > 0


@pytest.mark.parametrize("source", ["quad", "pair"])
def test_generating_camera_equals_the_frame(request, source):
    """From the generating camera at the VDI's size the merged VDI is the frame's own image (the GPU flatten of the
    same lists) within 1 LSB per channel, the bound of test_same_camera_equals_flatten."""
    m = request.getfixturevalue(source)
    img = m.ctx.view_render(G, W, H)
    diff = np.abs(img.astype(np.int32) - m.image.astype(np.int32))
    print(f"{source}: merged view against the frame's image: at most {int(diff.max())} LSB, "
          f"{int(np.count_nonzero(diff))} channels differ")
    assert m.image[..., 3].max() > 0
    assert diff.max() <= 1


def test_host_set_equals_device_bind(quad, other):
    stream = quad.ctx.view_pack(PACK_FLOAT)
    _, dev_acc = quad.ctx.view_render(CAMS["yaw90"], *SIZE, want_float=True)
    other.view_bind_host_set(quad.cols, quad.deps, G)
    st = other.stats()
    assert st["view_slots"] == 13 and st["view_overlaps"] == 0 and st["ms_view_bind"] > 0.0
    assert np.array_equal(other.view_pack(PACK_FLOAT), stream)
    _, acc = other.view_render(CAMS["yaw90"], *SIZE, want_float=True)
    assert np.array_equal(_bits(acc), _bits(dev_acc))
    # a set of one is the single-VDI bind
    other.view_bind_host(quad.cols[1], quad.deps[1], G)
    one = other.view_pack(PACK_FLOAT)
    other.view_bind_host_set(quad.cols[1:2], quad.deps[1:2], G)
    assert np.array_equal(other.view_pack(PACK_FLOAT), one)
    assert np.array_equal(one, pack_vdi(quad.cols[1], quad.deps[1], vb.pv_of(G), PACK_FLOAT))


def test_ragged_window():
    """50x37, S = 5: partial tiles on both axes, seen from so close that the two abutting bricks reach into them."""
    rw, rh, rs = 50, 37, 5
    scenes = scene_set("abutting_pair", rw, rh)
    cam = scene.orbit_camera(rw, rh, radius=1.4, yaw_deg=30.0, pitch_deg=20.0, voxel_world=1.0 / 32)
    with InSituContext(rw, rh, max_supersegments=rs, bricks_per_rank=2) as ctx:
        m = _Merged(ctx, scenes, cam)
        counts = np.count_nonzero(m.merged[1][:, :, 0::2], axis=2)
        assert counts.max() > rs   # (longer than either list: both bricks reach some pixel)
        assert np.count_nonzero(counts[48:]) >= 20 and np.count_nonzero(counts[:, 32:]) >= 20   # (oracle: 54 and 130)
        _assert_packed(ctx, m.merged, cam, "ragged window")
        assert m.stats["view_slots"] == m.merged[0].shape[2] and m.stats["view_overlaps"] == m.merged[2]


@pytest.mark.parametrize("n", [3, 9, 32])
def test_list_counts_through_the_host_set(other, n):
    cols, deps = _random_set(n, 100 + n)
    for d in deps:
        st = d[:, :, 0::2]
        assert np.all((st[:, :, 1] == 0) | (st[:, :, 1] > st[:, :, 0]))
    merged = loop_merge(cols, deps)
    starts = merged[1][:, :, 0::2]
    assert np.count_nonzero((starts[:, :, 1:] == starts[:, :, :-1]) & (starts[:, :, 1:] != 0)) > 0   # ties between lists
    gen = vb.gen_camera(16, 8)
    other.view_bind_host_set(cols, deps, gen)
    _assert_packed(other, merged, gen, f"{n} random lists")
    st = other.stats()
    assert st["view_slots"] == merged[0].shape[2] > 2 and st["view_overlaps"] == merged[2]


def test_slot_limit(other):
    gen, cam = vb.gen_camera(16, 8), vb.view_cameras(16, 8)["yaw20"]
    a = vb.layered_vdi(128, 16, 8)
    b = vb.layered_vdi(127, 16, 8, 128)
    other.view_bind_host_set([a[0], b[0]], [a[1], b[1]], gen)
    assert other.stats()["view_slots"] == 255
    _assert_packed(other, loop_merge([a[0], b[0]], [a[1], b[1]]), gen, "128 + 127 entries")
    lib = other.lib
    ncam = gen.native()
    cp = (ctypes.c_void_p * 2)(a[0].ctypes.data, a[0].ctypes.data)
    dp = (ctypes.c_void_p * 2)(a[1].ctypes.data, a[1].ctypes.data)
    _fails(other, lib.insitu_view_bind_host_set(other.h, cp, dp, 2, 16, 8, 128, ctypes.byref(ncam)), "256")
    _nothing_bound(other)
    assert other.stats()["view_slots"] == 0
    # a good bind afterwards renders as the restatement does
    col, dep = vb.list_end_vdi()
    slab = vb.slab_vdi(vb.SLAB, 16, 8, 6)
    other.view_bind_host_set([col, slab[0]], [dep, slab[1]], gen)
    merged = loop_merge([col, slab[0]], [dep, slab[1]])
    img, acc = other.view_render(cam, 41, 29, want_float=True)
    ref_img, ref_acc = vb.render(merged[0], merged[1], gen, cam, 41, 29)
    assert np.array_equal(_bits(acc), _bits(ref_acc)) and np.array_equal(img, ref_img)
    assert ref_acc[..., 3].sum() > 1.0


def test_merge_bricks_context_is_brick_0():
    scenes = scene_set("abutting_pair")
    with InSituContext(W, H, max_supersegments=S, bricks_per_rank=2, merge_bricks=True) as ctx:
        _set_bricks(ctx, scenes)
        ctx.frame(G)
        ctx.view_bind(native.VIEW_BRICK, 0)
        brick = ctx.view_pack(PACK_FLOAT)
        ctx.view_bind(native.VIEW_MERGED)
        assert np.array_equal(ctx.view_pack(PACK_FLOAT), brick)
        assert np.array_equal(brick, pack_vdi(ctx.read(native.BUF_VDI_COLOR), ctx.read(native.BUF_VDI_DEPTH), vb.pv_of(G),
                                              PACK_FLOAT))
        assert ctx.stats()["view_overlaps"] == 0


def test_rank_1_of_two_merges_its_own_bricks():
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
        ctx = ctxs[1]
        cols, deps = _read_all(ctx, 2)
        merged = loop_merge(cols, deps)
        assert merged[0].shape[2] > S   # (its two bricks share pixels)
        ctx.view_bind(native.VIEW_MERGED)
        _assert_packed(ctx, merged, G, "rank 1 of two")
    finally:
        for c in ctxs:
            c.close()
        group.close()


def test_pipelined_frame_in_flight():
    """After a re-ingest and with frame 1 in flight, MERGED binds frame 0: its lists and its camera."""
    scenes = scene_set("overlapping_pair")
    cam1 = CAMS["yaw90"]
    with InSituContext(W, H, max_supersegments=S, bricks_per_rank=2) as ctx:
        _set_bricks(ctx, scenes)
        assert ctx.frame_pipelined(G)[0] == -1
        ctx.set_brick(0, torch.from_numpy(scenes[1]["vol"].view(np.int16)).cuda(), scenes[0]["model"], dtype=native.U16)
        assert ctx.frame_pipelined(cam1)[0] == 0              # frame 0 is complete, frame 1 in flight
        ctx.view_bind(native.VIEW_MERGED)
        cols, deps = _read_all(ctx, 2)
        first = _assert_packed(ctx, loop_merge(cols, deps), G, "frame 0, frame 1 in flight")
        assert ctx.pipeline_flush()[0] == 1
        assert np.array_equal(ctx.view_pack(PACK_FLOAT), first)   # the snapshot did not move
        ctx.view_bind(native.VIEW_MERGED)
        cols1, deps1 = _read_all(ctx, 2)
        assert not np.array_equal(deps1[0], deps[0])
        _assert_packed(ctx, loop_merge(cols1, deps1), cam1, "frame 1")


def test_error_paths(quad, other):
    lib = quad.ctx.lib
    slab = vb.slab_vdi(vb.SLAB, 16, 8, 2)
    gen = vb.gen_camera(16, 8)
    ncam = gen.native()
    with InSituContext(W, H, max_supersegments=S, bricks_per_rank=2) as ctx:
        ctx.view_bind_host(*slab, gen)
        _fails(ctx, lib.insitu_view_bind(ctx.h, native.VIEW_MERGED, 0), "no frame rendered")
        _nothing_bound(ctx)
    ctx = quad.ctx
    try:
        _fails(ctx, lib.insitu_view_bind(ctx.h, native.VIEW_MERGED, 1), "slot 0")
        _nothing_bound(ctx)
    finally:
        ctx.view_bind(native.VIEW_MERGED)   # (as the fixture left it)
    cols = (ctypes.c_void_p * 33)(*([slab[0].ctypes.data] * 33))
    deps = (ctypes.c_void_p * 33)(*([slab[1].ctypes.data] * 33))
    holed = (ctypes.c_void_p * 3)(slab[0].ctypes.data, None, slab[0].ctypes.data)
    for what, args, text in (("n = 0", (cols, deps, 0, 16, 8, 2), "needs 1 to 32"),
                             ("n = 33", (cols, deps, 33, 16, 8, 2), "needs 1 to 32"),
                             ("a null entry", (holed, deps, 3, 16, 8, 2), "null VDI 1"),
                             ("S = 0", (cols, deps, 2, 16, 8, 0), "S in [1,255]"),
                             ("no camera", (cols, deps, 2, 16, 8, 2), "null argument")):
        other.view_bind_host(*slab, gen)
        cam_arg = None if what == "no camera" else ctypes.byref(ncam)
        _fails(other, lib.insitu_view_bind_host_set(other.h, *args, cam_arg), text)
        _nothing_bound(other)
    other.view_bind_host_set([slab[0]] * 32, [slab[1]] * 32, gen)   # 32 is the most, and binds
    assert other.stats()["view_slots"] == 32
