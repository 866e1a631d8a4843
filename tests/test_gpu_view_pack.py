"""GPU checks of the packed VDI stream (insitu_view_pack_bytes / insitu_view_pack / insitu_view_bind_packed,
csrc/vdi_pack.hip).  The bar is equality of bytes and of float bit patterns throughout: the
GPU's stream against the numpy codec's (insitu_amd/vdi_io.py) in both formats over every bind source and the sizes
at which the offset passes and the cooperative copy take another path; a FLOAT stream bound in a second context
renders what the first context renders; a HALF stream is exactly the numpy quantiser; packing is idempotent; the
snapshot does not move under pipelined frames; buffers grow and are reused; every rejected stream is rejected
before it is scattered, leaves nothing bound, and a good bind works afterwards."""
from __future__ import annotations

import ctypes

import numpy as np
import pytest
import torch

import view_binding as vb
from insitu_amd import native, scene
from insitu_amd.renderer import InSituContext
from insitu_amd.vdi_io import PACK_FLOAT, PACK_HALF, pack_vdi, unpack_vdi
from scenes import make_scene
from test_vdi_pack import empty_vdi, random_vdi, rejected_streams
from view_binding import bits as _bits, fails as _fails

pytestmark = pytest.mark.gpu

W, H, S, S_OUT = vb.VDI_W, vb.VDI_H, vb.VDI_S, 4
RW, RH, RS = 50, 37, 5
CAMS = vb.view_cameras()
G = vb.gen_camera()
SIZE = vb.OUT_SIZES[1]
# far cameras at 50x37, and the generating camera at twice the VDI's resolution (rays in cell planes)
VIEWS = (("yaw90", SIZE), ("yaw180", SIZE), ("cross", SIZE), ("same", (128, 96)))
FORMATS = (PACK_FLOAT, PACK_HALF)


def _scenes():
    a = make_scene(n=32, W=W, H=H, origin=(-0.5, -0.5, -0.5))
    b = make_scene(n=32, W=W, H=H, seed=7, origin=(0.0, -0.25, -0.75))
    return a, b


class _Source:
    """A VDI in the reference layout with its generating camera, and the context it is bound in (for the device
    sources: the one that generated it)."""

    def __init__(self, ctx, col, dep, gen):
        self.ctx, self.col, self.dep, self.gen = ctx, col, dep, gen
        self.pv = vb.pv_of(gen)
        self._views = None

    def views(self, cams=CAMS):
        """The bound VDI from VIEWS, rendered by the source's own context (once)."""
        if self._views is None:
            self._views = _views(self.ctx, cams)
        return self._views


def _views(ctx, cams=CAMS):
    return [ctx.view_render(cams[name], *size, want_float=True) for name, size in VIEWS]


def _assert_same_views(got, want, what):
    for (name, size), (img, acc), (wimg, wacc) in zip(VIEWS, got, want):
        bad = _bits(acc) != _bits(wacc)
        assert not bad.any(), f"{what}, {name} at {size}: {int(bad.sum())} of {bad.size} accumulator words differ"
        assert np.array_equal(img, wimg), f"{what}, {name} at {size}: images differ"
    assert sum(float(acc[..., 3].sum()) for _, acc in want) > 1.0, what   # (the cameras see something)


@pytest.fixture(scope="module")
def brick():
    """One brick's sub-VDI (64x48, S = 6, counts 0...6), bound with INSITU_VIEW_BRICK."""
    a, _ = _scenes()
    with InSituContext(W, H, max_supersegments=S) as ctx:
        ctx.set_transfer(a["tf"], a["cmap"], a["conv_scale"], a["conv_offset"])
        ctx.set_brick(0, a["vol"], a["model"])
        ctx.frame(G)
        ctx.view_bind(native.VIEW_BRICK, 0)
        yield _Source(ctx, ctx.read(native.BUF_VDI_COLOR), ctx.read(native.BUF_VDI_DEPTH), G)


@pytest.fixture(scope="module")
def gathered():
    """The gathered composited VDI of two bricks, S_out = 4 < S: unwritten slots past the counts."""
    a, b = _scenes()
    with InSituContext(W, H, max_supersegments=S, bricks_per_rank=2, composite_vdi=True,
                       max_output_supersegments=S_OUT) as ctx:
        ctx.set_transfer(a["tf"], a["cmap"], a["conv_scale"], a["conv_offset"])
        ctx.set_brick(0, a["vol"], a["model"])
        ctx.set_brick(1, b["vol"], b["model"])
        ctx.frame(G)
        ctx.view_bind(native.VIEW_GATHERED)
        yield _Source(ctx, ctx.read(native.BUF_GATHERED_COLOR), ctx.read(native.BUF_GATHERED_DEPTH), G)


@pytest.fixture(scope="module")
def ragged():
    """A 50x37, S = 5 brick VDI: ragged in both axes, 1850 pixels = 7 blocks and a partial one."""
    sc = make_scene(n=32, W=RW, H=RH, origin=(-0.5, -0.5, -0.5), world=2.0)
    with InSituContext(RW, RH, max_supersegments=RS) as ctx:
        ctx.set_transfer(sc["tf"], sc["cmap"], sc["conv_scale"], sc["conv_offset"])
        ctx.set_brick(0, sc["vol"], sc["model"])
        ctx.frame(sc["cam"])
        ctx.view_bind(native.VIEW_BRICK, 0)
        yield _Source(ctx, ctx.read(native.BUF_VDI_COLOR), ctx.read(native.BUF_VDI_DEPTH), sc["cam"])


@pytest.fixture(scope="module")
def other():
    """A context of other dimensions than anything bound into it."""
    with InSituContext(32, 16, max_supersegments=2) as ctx:
        yield ctx


HOST_VDIS = {
    "list_ends": vb.list_end_vdi,                           # lists that end at a zero start, run full, or are empty
    "9x7_S1": lambda: vb.slab_vdi(vb.SLAB, 9, 7, 1),        # 63 pixels: one partial wave
    "20x12_S255": lambda: vb.layered_vdi(255, 20, 12),      # the longest lists: 16320 entries per wave
    "empty": empty_vdi,                                     # E = 0
    "random_260x130_S2": lambda: random_vdi(260, 130, 2, 21),   # 33 800 pixels: 133 blocks, 3 steps of the scan
    "random_400x170_S1": lambda: random_vdi(400, 170, 1, 23),   # 266 blocks: the scan loads a second batch of 4 steps
}


def _check_pack(ctx, col, dep, pv, what):
    for fmt in FORMATS:
        want = pack_vdi(col, dep, pv, fmt)
        assert ctx.lib.insitu_view_pack_bytes(ctx.h, fmt) == want.size, (what, fmt)
        got = ctx.view_pack(fmt)
        assert got.size == want.size, (what, fmt)
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, f"{what}, format {fmt}: {bad.size} of {want.size} bytes differ, the first at {int(bad[0])}"
        assert ctx.stats()["ms_pack"] > 0.0


@pytest.mark.parametrize("source", ["brick", "gathered", "ragged"])
def test_pack_of_device_bind_equals_numpy_codec(request, source):
    src = request.getfixturevalue(source)
    counts = np.count_nonzero(src.dep[:, :, 0::2], axis=2)
    assert counts.max() > 0 and counts.min() == 0
    _check_pack(src.ctx, src.col, src.dep, src.pv, source)


@pytest.mark.parametrize("name", list(HOST_VDIS))
def test_pack_of_host_bind_equals_numpy_codec(other, name):
    col, dep = HOST_VDIS[name]()
    gen = vb.gen_camera(col.shape[0], col.shape[1])
    other.view_bind_host(col, dep, gen)
    _check_pack(other, col, dep, vb.pv_of(gen), name)


@pytest.mark.parametrize("source", ["brick", "gathered"])
def test_float_stream_carries_the_view_exactly(request, other, source):
    src = request.getfixturevalue(source)
    other.view_bind_packed(src.ctx.view_pack(PACK_FLOAT))
    assert other.stats()["ms_pack"] > 0.0
    try:
        other.set_option(native.OPT_VIEW_SKIP, 0)
        walked = _views(other)
    finally:
        other.set_option(native.OPT_VIEW_SKIP, 1)
    skipped = _views(other)
    _assert_same_views(skipped, src.views(), f"{source}, packed bind")
    _assert_same_views(walked, skipped, f"{source}, packed bind, skip off")   # (tmax is the unpacker's)


def test_half_stream_is_the_defined_quantiser(brick, other):
    rcol, rdep = random_vdi(RW, RH, RS, 22)
    rgen, rcams = vb.gen_camera(RW, RH), vb.view_cameras(RW, RH)
    other.view_bind_host(rcol, rdep, rgen)
    for what, stream, gen, cams in (("random 50x37x5", other.view_pack(PACK_HALF), rgen, rcams),
                                    ("brick", brick.ctx.view_pack(PACK_HALF), G, CAMS)):
        other.view_bind_packed(stream)
        packed = _views(other, cams)
        col, dep, pv, fmt = unpack_vdi(stream)
        assert fmt == PACK_HALF and np.array_equal(_bits(pv), _bits(vb.pv_of(gen)))
        other.view_bind_host(col, dep, gen)
        _assert_same_views(packed, _views(other, cams), f"{what}, half stream against its unpacked VDI")
    # recorded, not asserted: how far the half image lies from the float one
    other.view_bind_packed(brick.ctx.view_pack(PACK_HALF))
    worst = 0.0
    for name, cam in CAMS.items():
        half = other.view_render(cam, *SIZE).astype(np.float64)
        full = brick.ctx.view_render(cam, *SIZE).astype(np.float64)
        worst = max(worst, float(np.abs(half - full).max()))
    print(f"HALF against FLOAT, brick VDI, six cameras at {SIZE}: at most {worst:.0f} of 255")


@pytest.mark.parametrize("source", ["brick", "gathered"])
def test_packing_is_idempotent(request, other, source):
    src = request.getfixturevalue(source)
    for fmt in FORMATS:
        stream = src.ctx.view_pack(fmt)
        other.view_bind_packed(stream)
        assert np.array_equal(other.view_pack(fmt), stream), (source, fmt)
    # `other` now holds the half stream's VDI
    assert np.array_equal(other.view_pack(PACK_FLOAT), pack_vdi(*unpack_vdi(stream)[:3], PACK_FLOAT)), source


def test_snapshot_is_independent_of_the_frame_loop():
    a, b = _scenes()
    cams = [scene.orbit_camera(W, H, yaw_deg=30.0 + 41.0 * i, pitch_deg=20.0 - 7.0 * i, voxel_world=1.0 / 32)
            for i in range(4)]
    with InSituContext(W, H, max_supersegments=S) as ctx:
        ctx.set_transfer(a["tf"], a["cmap"], a["conv_scale"], a["conv_offset"])
        ctx.set_brick(0, a["vol"], a["model"])
        assert ctx.frame_pipelined(cams[0])[0] == -1
        assert ctx.frame_pipelined(cams[1])[0] == 0
        ctx.view_bind(native.VIEW_BRICK, 0)                   # frame 0, with frame 1 in flight
        col, dep = ctx.read(native.BUF_VDI_COLOR), ctx.read(native.BUF_VDI_DEPTH)
        first = {fmt: ctx.view_pack(fmt) for fmt in FORMATS}
        assert np.array_equal(first[PACK_FLOAT], pack_vdi(col, dep, vb.pv_of(cams[0]), PACK_FLOAT))
        assert ctx.frame_pipelined(cams[2])[0] == 1
        ctx.set_brick(0, torch.from_numpy(b["vol"].view(np.int16)).cuda(), a["model"], dtype=native.U16)
        assert ctx.frame_pipelined(cams[3])[0] == 2           # frame 3, of the re-ingested brick, is in flight
        for fmt in FORMATS:
            assert np.array_equal(ctx.view_pack(fmt), first[fmt]), fmt
        assert ctx.pipeline_flush()[0] == 3


def test_rebinding_grows_and_reuses_buffers(brick):
    """A larger packed VDI after a smaller device bind and the other way round, in one context each: every bind
    renders as its own source does."""
    sc = make_scene(n=32, W=32, H=16, origin=(-0.5, -0.5, -0.5))
    big = brick.ctx.view_pack(PACK_FLOAT)
    with InSituContext(32, 16, max_supersegments=2) as ctx:
        ctx.set_transfer(sc["tf"], sc["cmap"], sc["conv_scale"], sc["conv_offset"])
        ctx.set_brick(0, sc["vol"], sc["model"])
        ctx.frame(sc["cam"])
        ctx.view_bind(native.VIEW_BRICK, 0)
        small_views = _views(ctx)
        small = ctx.view_pack(PACK_HALF)
        small_exact = ctx.view_pack(PACK_FLOAT)
        ctx.view_bind_packed(big)                             # larger: the view's buffers and the staging grow
        _assert_same_views(_views(ctx), brick.views(), "larger packed VDI after a smaller device bind")
        ctx.view_bind(native.VIEW_BRICK, 0)                   # smaller again: the larger buffers are kept
        _assert_same_views(_views(ctx), small_views, "device bind after the larger packed VDI")
        assert np.array_equal(ctx.view_pack(PACK_HALF), small)
    try:
        brick.ctx.view_bind_packed(small_exact)               # a smaller packed VDI after the larger device bind
        _assert_same_views(_views(brick.ctx), small_views, "smaller packed VDI after a larger device bind")
        assert np.array_equal(brick.ctx.view_pack(PACK_FLOAT), small_exact)
    finally:
        brick.ctx.view_bind(native.VIEW_BRICK, 0)             # (as the fixture left it)
    _assert_same_views(_views(brick.ctx), brick.views(), "device bind after the smaller packed VDI")
    assert np.array_equal(brick.ctx.view_pack(PACK_FLOAT), big)


def test_error_paths(brick):
    lib = brick.ctx.lib
    n = ctypes.c_size_t(0)
    with InSituContext(W, H, max_supersegments=S) as ctx:
        buf = np.zeros(1024, np.uint8)
        _fails(ctx, lib.insitu_view_pack(ctx.h, PACK_FLOAT, buf.ctypes.data, buf.nbytes, ctypes.byref(n)), "no VDI bound")
        assert lib.insitu_view_pack_bytes(ctx.h, PACK_FLOAT) == 0
        assert "no VDI bound" in lib.insitu_last_error(ctx.h).decode()
    ctx = brick.ctx
    need = lib.insitu_view_pack_bytes(ctx.h, PACK_FLOAT)
    buf = np.full(need, 0xAB, np.uint8)
    _fails(ctx, lib.insitu_view_pack(ctx.h, 2, buf.ctypes.data, buf.nbytes, ctypes.byref(n)), "bad format")
    _fails(ctx, lib.insitu_view_pack(ctx.h, -1, buf.ctypes.data, buf.nbytes, None), "bad format")
    assert lib.insitu_view_pack_bytes(ctx.h, 2) == 0 and "bad format" in lib.insitu_last_error(ctx.h).decode()
    n.value = 0
    _fails(ctx, lib.insitu_view_pack(ctx.h, PACK_FLOAT, buf.ctypes.data, need - 1, ctypes.byref(n)), "too small")
    assert n.value == need and np.all(buf == 0xAB)            # the size is reported, the buffer untouched
    n.value = 0
    _fails(ctx, lib.insitu_view_pack(ctx.h, PACK_HALF, None, 0, ctypes.byref(n)), "too small")
    assert n.value == lib.insitu_view_pack_bytes(ctx.h, PACK_HALF) < need
    assert lib.insitu_view_pack(ctx.h, PACK_FLOAT, buf.ctypes.data, need, None) == 0   # (*bytes may be NULL)
    assert np.array_equal(buf, pack_vdi(brick.col, brick.dep, brick.pv, PACK_FLOAT))


def test_rejected_streams_leave_nothing_bound(other):
    lib = other.lib
    col, dep = vb.list_end_vdi()
    gen, cam = vb.gen_camera(16, 8), vb.view_cameras(16, 8)["yaw20"]
    good = pack_vdi(col, dep, vb.pv_of(gen), PACK_FLOAT)
    _, want = vb.render(col, dep, gen, cam, 41, 29)
    assert want[..., 3].sum() > 1.0
    ncam = cam.native()
    img = np.empty((29, 41, 4), np.uint8)
    on_device = {"a count above S, the sum kept": "exceeds S", "counts that add up to less than E": "add up to",
                 "counts that add up to more than E": "add up to"}
    streams = rejected_streams()
    assert set(on_device) <= set(streams)
    for name, stream in streams.items():
        other.view_bind_packed(good)
        _, acc = other.view_render(cam, 41, 29, want_float=True)
        assert np.array_equal(_bits(acc), _bits(want)), f"good bind before '{name}'"
        stream = np.ascontiguousarray(stream)
        _fails(other, lib.insitu_view_bind_packed(other.h, stream.ctypes.data, stream.nbytes), "stream rejected")
        assert on_device.get(name, "") in lib.insitu_last_error(other.h).decode(), name
        _fails(other, lib.insitu_view_render(other.h, ctypes.byref(ncam), 41, 29, img.ctypes.data, img.nbytes), "no VDI bound")
        _fails(other, lib.insitu_view_pack(other.h, PACK_FLOAT, img.ctypes.data, img.nbytes, None), "no VDI bound")
    _fails(other, lib.insitu_view_bind_packed(other.h, None, 1000), "stream rejected")
    other.view_bind_packed(good)
    _, acc = other.view_render(cam, 41, 29, want_float=True)
    assert np.array_equal(_bits(acc), _bits(want))
