"""GPU checks of novel-view VDI rendering (insitu_view_bind / insitu_view_bind_host / insitu_view_render,
DESIGN.md section 9): vdi_view_kernel against the CPU restatement tests/view_ref/view_ref.c bit for bit -- the
float accumulator and the rgba8 image -- over a generator sub-VDI and a gathered composited VDI, every test
camera and both output sizes; the host bind against the device bind; the empty-tile skip on and off; the
snapshot under later pipelined frames; the error paths; and a slab VDI against its analytic image, which does
not go through the restatement at all.  Further down: every bind source (the gathered VDI of 2 and 4 ranks, bricks
beyond rank 0 and slot 0, a merged sub-VDI), VDIs whose size is no multiple of the tile, rays that lie in a cell
plane, S = 1 and S = 255, host lists that end in every way, rebinding, and the gathered VDI between pipelined
frames."""
from __future__ import annotations

import ctypes

import numpy as np
import pytest
import torch

import view_binding as vb
from insitu_amd import native, scene
from insitu_amd.renderer import InSituContext, LocalGroup
from scenes import make_scene
from view_binding import bits as _bits, fails as _fails

pytestmark = pytest.mark.gpu

W, H, S, S_OUT = vb.VDI_W, vb.VDI_H, vb.VDI_S, 4
CAMS = vb.view_cameras()
G = vb.gen_camera()


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
    _fails(ctx, lib.insitu_view_render(ctx.h, ctypes.byref(cam), 50, 37, out.ctypes.data, out.nbytes), "no VDI bound")
    _fails(ctx, lib.insitu_view_bind(ctx.h, native.VIEW_BRICK, -1), "slot out of range")
    _fails(ctx, lib.insitu_view_render(ctx.h, ctypes.byref(cam), 50, 37, out.ctypes.data, out.nbytes), "no VDI bound")
    ctx.view_bind(native.VIEW_BRICK, 0)   # (a failed bind leaves no VDI bound: bind again for the later tests)
    _fails(ctx, lib.insitu_view_render(ctx.h, ctypes.byref(cam), 50, 37, out.ctypes.data, out.nbytes - 1), "too small")
    _fails(ctx, lib.insitu_view_render(ctx.h, ctypes.byref(cam), 0, 37, out.ctypes.data, out.nbytes), "output size")
    _fails(ctx, lib.insitu_view_render(ctx.h, ctypes.byref(cam), 50, -3, out.ctypes.data, out.nbytes), "output size")
    _fails(ctx, lib.insitu_view_bind_host(ctx.h, brick.col.ctypes.data, brick.dep.ctypes.data, W, H, 0,
                                          ctypes.byref(G.native())), "S in [1,255]")
    _fails(ctx, lib.insitu_view_render(ctx.h, ctypes.byref(cam), 50, 37, out.ctypes.data, out.nbytes), "no VDI bound")
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


# ---------------------------------------------------------------- every bind source, ragged sizes, rays in cell planes
SIZE = vb.OUT_SIZES[1]
FAR_CAMS = ("yaw90", "yaw180", "cross")


def _same(ctx, col, dep, gen, cam, size, what):
    """The bound VDI seen from cam equals the restatement's view of (col, dep) bit for bit; returns both."""
    img, acc = ctx.view_render(cam, *size, want_float=True)
    ref_img, ref_acc = vb.render(col, dep, gen, cam, *size)
    bad = _bits(acc) != _bits(ref_acc)
    assert not bad.any(), (f"{what} at {size}: {int(bad.sum())} of {bad.size} accumulator words differ, the first at "
                           f"(y, x, c) = {np.argwhere(bad)[0].tolist()}, max |d| {np.max(np.abs(acc - ref_acc))}")
    assert np.array_equal(img, ref_img), what
    return acc, ref_acc


def _group_scene(w, h):
    """The frame camera and the four bricks of test_multi_rank_data_path_local_group at (w, h)."""
    sc = make_scene(n=24, W=w, H=h, yaw=35.0)
    bricks = []
    for i in range(4):
        s_i = make_scene(n=24, W=w, H=h, yaw=35.0, seed=11 + i, origin=(-1.0 + (i % 2), -1.0 + (i // 2), -0.5))
        bricks.append((s_i["vol"], s_i["model"]))
    return sc, bricks


class _Group:
    """`world` ranks of an in-process group sharing the four bricks, composite_vdi with S_out = 4 < S = 6."""

    def __init__(self, world, w, h):
        self.sc, self.bricks = _group_scene(w, h)
        self.world, self.B = world, 4 // world
        self.group = LocalGroup(world)
        self.ctxs = []

    def __enter__(self):
        try:
            for r in range(self.world):
                ctx = InSituContext(self.sc["W"], self.sc["H"], max_supersegments=S, bricks_per_rank=self.B, rank=r,
                                    nranks=self.world, local_group=self.group, composite_vdi=True,
                                    max_output_supersegments=S_OUT)
                self.ctxs.append(ctx)
                ctx.set_transfer(self.sc["tf"], self.sc["cmap"], self.sc["conv_scale"], self.sc["conv_offset"])
                for b in range(self.B):
                    ctx.set_brick(b, *self.bricks[r * self.B + b])
        except Exception:
            self.__exit__()
            raise
        return self

    def __exit__(self, *a):
        for ctx in self.ctxs:
            ctx.close()
        self.group.close()

    def frame(self, cam):
        for ctx in self.ctxs:
            ctx.render(cam)
        for ctx in self.ctxs:
            ctx.exchange()
        for ctx in self.ctxs:
            ctx.composite()
        for ctx in self.ctxs[1:]:
            ctx.gather(want_image=False)
        self.ctxs[0].gather(want_image=False)


@pytest.mark.parametrize("world,w,h", [(2, 64, 48), (4, 64, 48), (2, 100, 37)])
def test_gathered_vdi_of_several_ranks(world, w, h):
    """view_build_kernel's strip addressing with d > 0 (strips of 32, 16 and 50 columns; 50: 7 tiles, the last one
    padded, over a ragged H): the gathered composited VDI of 2 and 4 ranks, seen from afar, equals the restatement
    on its read-back and, word for word, the view of one rank holding all four bricks."""
    with _Group(world, w, h) as g:
        g.frame(g.sc["cam"])
        root = g.ctxs[0]
        col, dep = root.read(native.BUF_GATHERED_COLOR), root.read(native.BUF_GATHERED_DEPTH)
        assert col.shape == (w, h, S_OUT, 4)
        counts = np.count_nonzero(dep[:, :, 0::2], axis=2)
        sw = w // world
        for d in range(1, world):
            assert np.count_nonzero(counts[d * sw:(d + 1) * sw]) > 20, f"strip {d} holds (almost) nothing"
        root.view_bind(native.VIEW_GATHERED)
        accs = {n: _same(root, col, dep, g.sc["cam"], CAMS[n], SIZE, f"world {world} {n}")[0] for n in FAR_CAMS}
        assert all(a[..., 3].sum() > 1.0 for a in accs.values())
    with InSituContext(w, h, max_supersegments=S, bricks_per_rank=4, composite_vdi=True,
                       max_output_supersegments=S_OUT) as one:
        one.set_transfer(g.sc["tf"], g.sc["cmap"], g.sc["conv_scale"], g.sc["conv_offset"])
        for b in range(4):
            one.set_brick(b, *g.bricks[b])
        one.frame(g.sc["cam"])
        one.view_bind(native.VIEW_GATHERED)
        for n in FAR_CAMS:
            _, acc = one.view_render(CAMS[n], *SIZE, want_float=True)
            assert np.array_equal(_bits(acc), _bits(accs[n])), n


def test_gathered_vdi_after_falling_counts():
    """The second of two frames lowers many pixels' counts; the gathered slots past them still hold the first
    frame's entries.  The view bound after it sees the second frame alone, from the second camera."""
    cam_b = scene.orbit_camera(W, H, yaw_deg=110.0, pitch_deg=-25.0, voxel_world=1.0 / 24)
    with _Group(2, W, H) as g:
        root = g.ctxs[0]
        g.frame(g.sc["cam"])
        first = np.count_nonzero(root.read(native.BUF_GATHERED_DEPTH)[:, :, 0::2], axis=2)
        g.frame(cam_b)
        col, dep = root.read(native.BUF_GATHERED_COLOR), root.read(native.BUF_GATHERED_DEPTH)
        assert np.count_nonzero(np.count_nonzero(dep[:, :, 0::2], axis=2) < first) > 0
        root.view_bind(native.VIEW_GATHERED)
        for n in FAR_CAMS:
            acc, _ = _same(root, col, dep, cam_b, CAMS[n], SIZE, f"falling counts {n}")
            assert acc[..., 3].sum() > 1.0


def test_brick_sources_beyond_rank0_slot0():
    """INSITU_VIEW_BRICK of slot 1 on rank 1 of two (after the exchange and the gather: the generator's slots are
    not the exchange's buffers, so this is supported as it stands), of slot 1 of a one-rank two-brick context,
    and of the one merged sub-VDI of a merge_bricks context."""
    with _Group(2, W, H) as g:
        g.frame(g.sc["cam"])
        ctx = g.ctxs[1]
        col, dep = ctx.read(native.BUF_VDI_COLOR, 1), ctx.read(native.BUF_VDI_DEPTH, 1)
        ctx.view_bind(native.VIEW_BRICK, 1)
        for n in FAR_CAMS:
            acc, _ = _same(ctx, col, dep, g.sc["cam"], CAMS[n], SIZE, f"rank 1 slot 1 {n}")
            assert acc[..., 3].sum() > 1.0
    for merge in (False, True):
        with InSituContext(W, H, max_supersegments=S, bricks_per_rank=2, merge_bricks=merge) as ctx:
            ctx.set_transfer(g.sc["tf"], g.sc["cmap"], g.sc["conv_scale"], g.sc["conv_offset"])
            ctx.set_brick(0, *g.bricks[2])
            ctx.set_brick(1, *g.bricks[3])
            ctx.frame(g.sc["cam"])
            if merge:
                _fails(ctx, ctx.lib.insitu_view_bind(ctx.h, native.VIEW_BRICK, 1), "slot out of range")
                slot = 0
            else:
                slot = 1
                # rank 1's slot 1 above was this brick: the same sub-VDI whichever rank renders it
                assert np.array_equal(_bits(ctx.read(native.BUF_VDI_DEPTH, 1)), _bits(dep))
            c, d = ctx.read(native.BUF_VDI_COLOR, slot), ctx.read(native.BUF_VDI_DEPTH, slot)
            ctx.view_bind(native.VIEW_BRICK, slot)
            for n in FAR_CAMS:
                acc, _ = _same(ctx, c, d, g.sc["cam"], CAMS[n], SIZE, f"merge {merge} slot {slot} {n}")
                assert acc[..., 3].sum() > 1.0


RW, RH, RS = 50, 37, 5
RAGGED_SIZES = ((50, 37), (64, 48), (1, 1), (130, 3))


def test_ragged_vdi_device_and_host_bind():
    """A VDI whose last tile column and row are partial (50x37, S = 5): the walk's clamped last granules, and
    the tile maximum taken over lanes outside the VDI."""
    sc = make_scene(n=32, W=RW, H=RH, origin=(-0.5, -0.5, -0.5), world=2.0)
    cams = vb.view_cameras(RW, RH)
    with InSituContext(RW, RH, max_supersegments=RS) as ctx:
        ctx.set_transfer(sc["tf"], sc["cmap"], sc["conv_scale"], sc["conv_offset"])
        ctx.set_brick(0, sc["vol"], sc["model"])
        ctx.frame(sc["cam"])
        col, dep = ctx.read(native.BUF_VDI_COLOR), ctx.read(native.BUF_VDI_DEPTH)
        counts = np.count_nonzero(dep[:, :, 0::2], axis=2)
        tiles = np.zeros((7, 5), int)
        np.maximum.at(tiles, (np.arange(RW)[:, None] // 8, np.arange(RH)[None, :] // 8), counts)
        assert 1 <= (tiles == 0).sum() <= 20 and np.count_nonzero(counts[:, 32:]) >= 40   # (oracle: 7 and 118)
        ctx.view_bind(native.VIEW_BRICK, 0)
        dev = {(n, size): _same(ctx, col, dep, sc["cam"], cams[n], size, f"ragged device bind {n}")[0]
               for n in ("yaw90", "yaw180", "close") for size in RAGGED_SIZES}
        assert dev[("yaw90", (50, 37))][..., 3].sum() > 1.0
    with InSituContext(32, 16, max_supersegments=2) as other:
        other.view_bind_host(col, dep, sc["cam"])
        for (n, size), acc in dev.items():
            _, host = other.view_render(cams[n], *size, want_float=True)
            assert np.array_equal(_bits(host), _bits(acc)), (n, size)
        # that scene leaves columns 48 and 49 empty: the slab fills every list
        gen = vb.gen_camera(RW, RH)
        scol, sdep = vb.slab_vdi(vb.SLAB, RW, RH, 3)
        other.view_bind_host(scol, sdep, gen)
        for n in ("yaw90", "yaw180", "close"):
            for size in RAGGED_SIZES:
                _same(other, scol, sdep, gen, cams[n], size, f"ragged slab {n}")
        img = other.view_render(cams["yaw90"], RW, RH)
        want = vb.analytic_slabs(vb.SLAB, gen, cams["yaw90"], RW, RH, W=RW, H=RH)
        err = vb.lsb_error(img, want)
        print(f"GPU ragged slab yaw90: {err:.3f} LSB")
        assert np.mean(want[..., 3] > 0) > 0.5 and err <= 1.0


@pytest.mark.parametrize("size", [(128, 96), (128, 48)])
def test_plane_aligned_rays(brick, size):
    """The generating camera at twice the VDI's resolution: every other column (and row) of rays lies in a cell
    plane, and the cell that the plane cuts give such a ray to must be the one the walk visits."""
    acc, _ = _same(brick.ctx, brick.col, brick.dep, G, G, size, "brick, aligned")
    assert acc[..., 3].sum() > 1.0
    col, dep = vb.slab_vdi(vb.SLAB)
    with InSituContext(32, 16, max_supersegments=2) as ctx:
        ctx.view_bind_host(col, dep, G)
        _same(ctx, col, dep, G, G, size, "slab, aligned")
        img = ctx.view_render(G, *size)
    want = vb.analytic_slabs(vb.SLAB, G, G, *size)
    out = vb.on_outer_plane(G, G, *size, W, H)
    assert out.sum() <= size[0] + size[1]
    assert np.mean(want[~out][:, 3] > 0) >= 0.9
    err = np.abs(img.astype(np.float64) - np.clip(want, 0.0, 1.0) * 255.0).max(axis=2)
    print(f"GPU aligned slab {size}: {err[~out].max():.3f} LSB, {int(out.sum())} rays in an outer plane left out")
    assert err[~out].max() <= 1.0


@pytest.mark.parametrize("which", ["S1", "S255", "list_ends"])
def test_host_bind_s_limits_and_list_ends(which):
    """S = 1 and S = 255 (the counts and the tiles' largest count are bytes), and host lists that end at a zero
    start depth in the middle, at S entries without a terminator, or at once."""
    if which == "S1":
        col, dep = vb.slab_vdi(vb.SLAB, 9, 7, 1)
    elif which == "S255":
        col, dep = vb.layered_vdi(255, 20, 12)
        assert np.all(np.count_nonzero(dep[:, :, 0::2], axis=2) == 255)
    else:
        col, dep = vb.list_end_vdi()
    w, h = col.shape[:2]
    gen, cam = vb.gen_camera(w, h), vb.view_cameras(w, h)["yaw20"]
    with InSituContext(32, 16, max_supersegments=2) as ctx:
        ctx.view_bind_host(col, dep, gen)
        acc, _ = _same(ctx, col, dep, gen, cam, (41, 29), which)
        img = ctx.view_render(cam, 41, 29)
    assert acc[..., 3].sum() > 1.0
    if which != "list_ends":   # all 255 entries were blended, or the one: the single slab's image
        err = vb.lsb_error(img, vb.analytic_slabs(vb.SLAB, gen, cam, 41, 29, W=w, H=h))
        print(f"GPU {which} yaw20: {err:.3f} LSB")
        assert err <= 1.0


def test_rebinding_and_resizing(brick):
    """A smaller VDI bound after a larger one keeps the larger buffers, and the output buffers outlive a smaller
    output: every bind and every size renders its own VDI."""
    ctx = brick.ctx
    small = vb.slab_vdi(vb.SLAB, 9, 7, 1)
    small_gen, small_cam = vb.gen_camera(9, 7), vb.view_cameras(9, 7)["yaw20"]
    try:
        ctx.view_bind(native.VIEW_BRICK, 0)
        for size in ((130, 3), (1, 1), (64, 48)):
            acc, _ = _same(ctx, brick.col, brick.dep, G, CAMS["yaw20"], size, "device bind 64x48x6")
        assert acc[..., 3].sum() > 1.0
        ctx.view_bind_host(*small, small_gen)
        for size in ((130, 3), (1, 1), (64, 48)):
            acc, _ = _same(ctx, *small, small_gen, small_cam, size, "host bind 9x7x1")
        assert acc[..., 3].sum() > 1.0
        ctx.view_bind_host(brick.col, brick.dep, G)
        for size in ((130, 3), (1, 1), (64, 48)):
            _same(ctx, brick.col, brick.dep, G, CAMS["yaw20"], size, "host bind 64x48x6")
    finally:
        ctx.view_bind(native.VIEW_BRICK, 0)   # (as the fixture left it)


def test_gathered_vdi_between_pipelined_frames():
    """INSITU_VIEW_GATHERED with a frame in flight: the VDI and its generating camera are the completed
    frame's, not those of the frame being rendered."""
    a, b = _scenes()
    cams = [scene.orbit_camera(W, H, yaw_deg=30.0 + 41.0 * i, pitch_deg=20.0 - 7.0 * i, voxel_world=1.0 / 32)
            for i in range(4)]
    accs = []
    with InSituContext(W, H, max_supersegments=S, bricks_per_rank=2, composite_vdi=True,
                       max_output_supersegments=S_OUT) as ctx:
        ctx.set_transfer(a["tf"], a["cmap"], a["conv_scale"], a["conv_offset"])
        ctx.set_brick(0, a["vol"], a["model"])
        ctx.set_brick(1, b["vol"], b["model"])
        assert ctx.frame_pipelined(cams[0])[0] == -1
        assert ctx.frame_pipelined(cams[1])[0] == 0
        for done in (1, 2):
            assert ctx.frame_pipelined(cams[done + 1])[0] == done   # frame done + 1 is in flight
            assert not np.array_equal(vb.pv_of(cams[done]), vb.pv_of(cams[done + 1]))
            ctx.view_bind(native.VIEW_GATHERED)
            col, dep = ctx.read(native.BUF_GATHERED_COLOR), ctx.read(native.BUF_GATHERED_DEPTH)
            acc, _ = _same(ctx, col, dep, cams[done], CAMS["yaw20"], SIZE, f"gathered, frame {done} done")
            assert acc[..., 3].sum() > 1.0
            # (the camera matters: the same lists taken as the in-flight camera's give another image)
            assert not np.array_equal(vb.render(col, dep, cams[done + 1], CAMS["yaw20"], *SIZE)[1], acc)
            accs.append(acc)
        assert not np.array_equal(accs[0], accs[1])
        assert ctx.pipeline_flush()[0] == 3
