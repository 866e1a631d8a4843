"""GPU checks of novel-view VDI rendering (insitu_view_bind / insitu_view_bind_host / insitu_view_render,
DESIGN.md section 9): vdi_view_kernel against the CPU restatement tests/view_ref/view_ref.c bit for bit -- the
float accumulator and the rgba8 image -- over a generator sub-VDI and a gathered composited VDI, every test
camera and both output sizes; the host bind against the device bind; the empty-tile skip on and off; the
snapshot under later pipelined frames; the error paths; and a slab VDI against its analytic image, which does
not go through the restatement at all."""
from __future__ import annotations

import ctypes

import numpy as np
import pytest
import torch

import view_binding as vb
from insitu_amd import native, scene
from insitu_amd.renderer import InSituContext, LocalGroup
from scenes import make_scene

pytestmark = pytest.mark.gpu

W, H, S, S_OUT = vb.VDI_W, vb.VDI_H, vb.VDI_S, 4
CAMS = vb.view_cameras()
G = vb.gen_camera()


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _scenes():
    a = make_scene(n=32, W=W, H=H, origin=(-0.5, -0.5, -0.5))
    b = make_scene(n=32, W=W, H=H, seed=7, origin=(0.0, -0.25, -0.75))
    return a, b


class _Bound:
    """A context with a VDI bound from the device, the VDI's readback, and the CPU reference's views of it
    (computed once per camera and size, shared by the tests)."""

    def __init__(self, ctx, col, dep):
        self.ctx, self.col, self.dep = ctx, col, dep
        self._ref = {}

    def ref(self, name, size):
        if (name, size) not in self._ref:
            self._ref[(name, size)] = vb.render(self.col, self.dep, G, CAMS[name], *size)
        return self._ref[(name, size)]


@pytest.fixture(scope="module")
def brick():
    """One brick's sub-VDI, bound with INSITU_VIEW_BRICK."""
    a, _ = _scenes()
    with InSituContext(W, H, max_supersegments=S) as ctx:
        ctx.set_transfer(a["tf"], a["cmap"], a["conv_scale"], a["conv_offset"])
        ctx.set_brick(0, a["vol"], a["model"])
        ctx.frame(G)
        ctx.view_bind(native.VIEW_BRICK, 0)
        yield _Bound(ctx, ctx.read(native.BUF_VDI_COLOR), ctx.read(native.BUF_VDI_DEPTH))


@pytest.fixture(scope="module")
def gathered():
    """The gathered composited VDI of two bricks with S_out = 4 < S: counts below the slot count and slots past
    them that the compositor never wrote."""
    a, b = _scenes()
    with InSituContext(W, H, max_supersegments=S, bricks_per_rank=2, composite_vdi=True,
                       max_output_supersegments=S_OUT) as ctx:
        ctx.set_transfer(a["tf"], a["cmap"], a["conv_scale"], a["conv_offset"])
        ctx.set_brick(0, a["vol"], a["model"])
        ctx.set_brick(1, b["vol"], b["model"])
        ctx.frame(G)
        ctx.view_bind(native.VIEW_GATHERED)
        col, dep = ctx.read(native.BUF_GATHERED_COLOR), ctx.read(native.BUF_GATHERED_DEPTH)
        assert col.shape == (W, H, S_OUT, 4)
        yield _Bound(ctx, col, dep)


@pytest.mark.parametrize("size", vb.OUT_SIZES)
@pytest.mark.parametrize("name", list(CAMS))
@pytest.mark.parametrize("source", ["brick", "gathered"])
def test_view_equals_cpu_reference(request, source, name, size):
    bound = request.getfixturevalue(source)
    img, acc = bound.ctx.view_render(CAMS[name], *size, want_float=True)
    ref_img, ref_acc = bound.ref(name, size)
    bad = np.count_nonzero(_bits(acc) != _bits(ref_acc))
    assert bad == 0, f"{bad} of {acc.size} accumulator words differ, max |d| {np.max(np.abs(acc - ref_acc))}"
    assert np.array_equal(img, ref_img)
    assert ref_acc[..., 3].sum() > 1.0   # (the camera sees the volume)
    out = np.empty((size[1], size[0], 4), np.uint8)
    bound.ctx._check(bound.ctx.lib.insitu_read(bound.ctx.h, native.BUF_VIEW_IMAGE, 0, out.ctypes.data, out.nbytes),
                     "insitu_read")
    assert np.array_equal(out, img)
    assert bound.ctx.stats()["ms_view"] > 0.0


def test_counts_differ_from_slots(gathered, brick):
    """What the two sources are there for: the brick's lists run from empty to full; every gathered list is
    shorter than its S_out slots, and the compositor never wrote the slots past a list's count."""
    counts = np.count_nonzero(brick.dep[:, :, 0::2], axis=2)
    assert counts.max() == S and np.count_nonzero((counts > 0) & (counts < S)) > 50
    counts = np.count_nonzero(gathered.dep[:, :, 0::2], axis=2)
    assert 0 < counts.max() < S_OUT and np.count_nonzero(counts) > 300


@pytest.mark.parametrize("source", ["brick", "gathered"])
def test_host_bind_equals_device_bind(request, source):
    bound = request.getfixturevalue(source)
    name, size = "yaw90", vb.OUT_SIZES[1]
    _, dev_acc = bound.ctx.view_render(CAMS[name], *size, want_float=True)
    with InSituContext(32, 16, max_supersegments=2) as other:   # (W, H, S need not be the context's)
        other.view_bind_host(bound.col, bound.dep, G)
        img, acc = other.view_render(CAMS[name], *size, want_float=True)
    assert np.array_equal(_bits(acc), _bits(dev_acc))
    assert np.array_equal(img, bound.ref(name, size)[0])


@pytest.mark.parametrize("name", list(CAMS))
def test_skip_changes_no_bit(brick, name):
    counts = np.count_nonzero(brick.dep[:, :, 0::2], axis=2)
    tiles = counts.reshape(W // 8, 8, H // 8, 8).max(axis=(1, 3))
    assert (tiles == 0).sum() >= 8 and (tiles > 0).sum() >= 4   # fully empty 8x8 tiles, and others
    size = vb.OUT_SIZES[1]
    try:
        brick.ctx.set_option(native.OPT_VIEW_SKIP, 0)
        _, walked = brick.ctx.view_render(CAMS[name], *size, want_float=True)
    finally:
        brick.ctx.set_option(native.OPT_VIEW_SKIP, 1)
    _, skipped = brick.ctx.view_render(CAMS[name], *size, want_float=True)
    assert np.array_equal(_bits(walked), _bits(skipped))
    assert np.array_equal(_bits(walked), _bits(brick.ref(name, size)[1]))


def test_snapshot_survives_pipelined_frames():
    """Bind after a completed pipelined frame; two more pipelined frames with other cameras and a re-ingest leave
    the bound VDI as it was; a fresh bind then takes the newly completed frame."""
    a, b = _scenes()
    cams = [scene.orbit_camera(W, H, yaw_deg=30.0 + 41.0 * i, pitch_deg=20.0 - 7.0 * i, voxel_world=1.0 / 32)
            for i in range(4)]
    view_cam, size = CAMS["yaw20"], vb.OUT_SIZES[1]
    with InSituContext(W, H, max_supersegments=S) as ctx:
        ctx.set_transfer(a["tf"], a["cmap"], a["conv_scale"], a["conv_offset"])
        ctx.set_brick(0, a["vol"], a["model"])
        assert ctx.frame_pipelined(cams[0])[0] == -1
        assert ctx.frame_pipelined(cams[1])[0] == 0          # frame 0 is complete, frame 1 in flight
        ctx.view_bind(native.VIEW_BRICK, 0)
        col0, dep0 = ctx.read(native.BUF_VDI_COLOR), ctx.read(native.BUF_VDI_DEPTH)
        img0, acc0 = ctx.view_render(view_cam, *size, want_float=True)
        ref0 = vb.render(col0, dep0, cams[0], view_cam, *size)
        assert np.array_equal(_bits(acc0), _bits(ref0[1])) and np.array_equal(img0, ref0[0])
        ctx.set_brick(0, torch.from_numpy(b["vol"].view(np.int16)).cuda(), a["model"], dtype=native.U16)
        assert ctx.frame_pipelined(cams[2])[0] == 1
        assert ctx.frame_pipelined(cams[3])[0] == 2
        img1, acc1 = ctx.view_render(view_cam, *size, want_float=True)
        assert np.array_equal(_bits(acc1), _bits(acc0)) and np.array_equal(img1, img0)
        ctx.view_bind(native.VIEW_BRICK, 0)                   # frame 2: the re-ingested brick, camera 2
        col2, dep2 = ctx.read(native.BUF_VDI_COLOR), ctx.read(native.BUF_VDI_DEPTH)
        assert not np.array_equal(dep2, dep0)
        img2, acc2 = ctx.view_render(view_cam, *size, want_float=True)
        ref2 = vb.render(col2, dep2, cams[2], view_cam, *size)
        assert np.array_equal(_bits(acc2), _bits(ref2[1])) and np.array_equal(img2, ref2[0])
        assert not np.array_equal(acc2, acc0)
        assert ctx.pipeline_flush()[0] == 3


def _fails(ctx, rc, text):
    assert rc == -1
    msg = ctx.lib.insitu_last_error(ctx.h).decode()
    assert text in msg, msg


def test_error_paths(brick):
    lib = brick.ctx.lib
    cam = CAMS["yaw20"].native()
    out = np.empty((37, 50, 4), np.uint8)
    with InSituContext(W, H, max_supersegments=S) as ctx:
        _fails(ctx, lib.insitu_view_render(ctx.h, ctypes.byref(cam), 50, 37, out.ctypes.data, out.nbytes), "no VDI bound")
        _fails(ctx, lib.insitu_view_bind(ctx.h, native.VIEW_GATHERED, 0), "composite_vdi")
        _fails(ctx, lib.insitu_view_bind(ctx.h, native.VIEW_BRICK, 0), "no frame rendered")
        _fails(ctx, lib.insitu_view_bind(ctx.h, 7, 0), "unknown source")
    ctx = brick.ctx
    _fails(ctx, lib.insitu_view_bind(ctx.h, native.VIEW_BRICK, 1), "slot out of range")
    _fails(ctx, lib.insitu_view_bind(ctx.h, native.VIEW_BRICK, -1), "slot out of range")
    ctx.view_bind(native.VIEW_BRICK, 0)   # (a failed bind leaves nothing bound: bind again for the later tests)
    _fails(ctx, lib.insitu_view_render(ctx.h, ctypes.byref(cam), 50, 37, out.ctypes.data, out.nbytes - 1), "too small")
    _fails(ctx, lib.insitu_view_render(ctx.h, ctypes.byref(cam), 0, 37, out.ctypes.data, out.nbytes), "output size")
    _fails(ctx, lib.insitu_view_render(ctx.h, ctypes.byref(cam), 50, -3, out.ctypes.data, out.nbytes), "output size")
    _fails(ctx, lib.insitu_view_bind_host(ctx.h, brick.col.ctypes.data, brick.dep.ctypes.data, W, H, 0,
                                          ctypes.byref(G.native())), "S in [1,255]")
    ctx.view_bind(native.VIEW_BRICK, 0)
    # the gathered VDI lives on rank 0 only
    group = LocalGroup(2)
    ctxs = [InSituContext(W, H, max_supersegments=S, rank=r, nranks=2, local_group=group, composite_vdi=True,
                          max_output_supersegments=S_OUT) for r in range(2)]
    try:
        _fails(ctxs[1], lib.insitu_view_bind(ctxs[1].h, native.VIEW_GATHERED, 0), "rank 0")
        _fails(ctxs[0], lib.insitu_view_bind(ctxs[0].h, native.VIEW_GATHERED, 0), "no frame gathered")
    finally:
        for c in ctxs:
            c.close()
        group.close()


def test_slab_matches_analytic_on_gpu():
    """The homogeneous slab through the GPU at an oblique camera against its analytic image: within 1 LSB
    (the project's image tolerance), without the CPU restatement in between."""
    layers = [(0.9715, 0.9799, (0.5, 0.25, 0.75, 0.3))]
    col, dep = vb.slab_vdi(layers)
    size = vb.OUT_SIZES[1]
    with InSituContext(W, H, max_supersegments=S) as ctx:
        ctx.view_bind_host(col, dep, G)
        img = ctx.view_render(CAMS["yaw20"], *size)
    want = vb.analytic_slabs(layers, G, CAMS["yaw20"], *size)
    err = vb.lsb_error(img, want)
    print(f"GPU slab yaw20 {size}: {err:.3f} LSB")
    assert 0.0 < np.mean(want[..., 3] > 0) < 1.0
    assert err <= 1.0
