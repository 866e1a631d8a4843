"""CPU checks of novel-view VDI rendering: the C restatement tests/view_ref/view_ref.c
against an analytic double-precision image of slab VDIs, against the oracle's flatten from the generating camera,
and against itself with and without the empty-tile skip and the view-layout repack; that the walk's intervals
partition every ray, rays lying in a cell plane included; ragged VDI sizes, S = 1 and S = 255, and host lists that
end at a zero start depth, at S entries or at once.  The GPU kernel is checked
against this restatement bit for bit in tests/test_gpu_view.py."""
from __future__ import annotations

import numpy as np
import pytest

import oracle_binding as orc
import view_binding as vb
from scenes import make_scene

# NDC depths of the generating camera (near 0.1, far 20, Vulkan z): about 3, 3.5 and 4 world units from its eye,
# around the volume the test scenes hold
Z0, Z1, Z2 = 0.9715, 0.9760, 0.9799
ONE = [(Z0, Z2, (0.5, 0.25, 0.75, 0.3))]
TWO = [(Z0, Z1, (1.0, 0.0, 0.0, 0.4)), (Z1, Z2, (0.0, 0.0, 1.0, 0.6))]
# the project's image tolerance: one 8-bit step
LSB = 1.0

CAMS = vb.view_cameras()
G = vb.gen_camera()


@pytest.fixture(scope="module")
def brick_vdi():
    """The oracle's VDI of tests/scenes.make_scene's default scene at the view tests' size."""
    sc = make_scene(n=32, W=vb.VDI_W, H=vb.VDI_H)
    inp = orc.Inputs(sc["vol"], sc["im"], sc["tf"], sc["cmap"], sc["conv_k"], sc["conv_offset"], sc["cam"])
    col, dep, _, _ = orc.vdi_generate(inp, vb.VDI_W, vb.VDI_H, vb.VDI_S)
    return sc, col, dep


def _clip_w(cam, out_w, out_h):
    """c_w of G's clip space at both ends of every output ray of cam."""
    pv_g = G.proj_rm @ G.view_rm
    ipv = np.linalg.inv(cam.proj_rm @ cam.view_rm)
    ox, oy = np.meshgrid(np.arange(out_w), np.arange(out_h))
    w = []
    for z in (-1.0, 1.0):
        p = np.stack([ox / out_w * 2 - 1, oy / out_h * 2 - 1, np.full(ox.shape, z), np.ones(ox.shape)], -1) @ ipv.T
        p = p / p[..., 3:]
        w.append((p @ pv_g.T)[..., 3])
    return w


@pytest.mark.parametrize("size", vb.OUT_SIZES)
@pytest.mark.parametrize("name", list(CAMS))
def test_homogeneous_slab_matches_analytic(name, size):
    """One supersegment [z0, z2] of one colour and opacity in every list: alpha = 1 - (1 - a)^chord with the
    chord of the ray inside the frustum slab, whatever cells the ray crosses -- a missed, repeated or
    mis-measured cell shows."""
    col, dep = vb.slab_vdi(ONE)
    img, _ = vb.render(col, dep, G, CAMS[name], *size)
    want = vb.analytic_slabs(ONE, G, CAMS[name], *size)
    err = vb.lsb_error(img, want)
    print(f"slab {name} {size}: {err:.3f} LSB, coverage {np.mean(want[..., 3] > 0):.2f}")
    assert err <= LSB


def test_cameras_are_the_cases_they_claim():
    w, h = vb.OUT_SIZES[0]
    cover = {n: np.mean(vb.analytic_slabs(ONE, G, c, w, h)[..., 3] > 0) for n, c in CAMS.items()}
    assert cover["same"] == 1.0
    assert 0.0 < cover["close"] < 1.0          # G's frustum covers only part of the output
    wf, wb = _clip_w(CAMS["cross"], w, h)
    assert np.all(wf < 0) and np.all(wb > 0)   # every ray crosses G's camera plane
    assert cover["cross"] > 0.5
    # yaw90: the rays cross many columns of lists
    pv_g = G.proj_rm @ G.view_rm
    ipv = np.linalg.inv(CAMS["yaw90"].proj_rm @ CAMS["yaw90"].view_rm)
    ends = []
    for z in (0.9, 0.98):   # inside the slab's depth range of the new camera's centre ray
        p = ipv @ np.array([0.0, 0.0, z, 1.0])
        c = pv_g @ (p / p[3])
        ends.append(c[0] / c[3])
    assert abs(ends[1] - ends[0]) * vb.VDI_W / 2 > 8


@pytest.mark.parametrize("name", ["same", "yaw20", "yaw180"])
def test_two_layers_blend_in_ray_order(name):
    """A red layer in front of a blue one (seen from G): the layer the ray meets first is blended first -- red
    from the front, blue from behind.  The image with the layers blended in the other order is farther than the
    tolerance from the analytic one, so a walk that does not flip fails."""
    col, dep = vb.slab_vdi(TWO)
    w, h = vb.OUT_SIZES[0]
    img, _ = vb.render(col, dep, G, CAMS[name], w, h)
    want = vb.analytic_slabs(TWO, G, CAMS[name], w, h)
    wrong = vb.analytic_slabs(TWO, G, CAMS[name], w, h, reverse=True)
    err, err_wrong = vb.lsb_error(img, want), vb.lsb_error(img, wrong)
    print(f"two layers {name}: {err:.3f} LSB (other order: {err_wrong:.1f} LSB)")
    assert err <= LSB
    assert err_wrong > 10 * LSB


def test_two_layers_order_flips_behind():
    """From behind the blue layer is met first: blue keeps its full weight and red is attenuated by it."""
    w, h = vb.OUT_SIZES[0]
    col, dep = vb.slab_vdi(TWO)
    ratio = {}
    for name in ("same", "yaw180"):
        _, acc = vb.render(col, dep, G, CAMS[name], w, h)
        both = (acc[..., 0] > 0.05) & (acc[..., 2] > 0.05)
        assert both.sum() > 100
        ratio[name] = float(np.median(acc[both][:, 2] / acc[both][:, 0]))   # blue over red
    assert ratio["yaw180"] > 1.5 * ratio["same"]


def test_same_camera_equals_flatten(brick_vdi):
    """From the generating camera at the VDI's size every ray stays in its own list, and the view is the
    flatten (orc_vdi_flatten) up to the float route to the segment length: within 1 LSB per channel."""
    sc, col, dep = brick_vdi
    assert np.array_equal(sc["cam"].view, G.view) and np.array_equal(sc["cam"].proj, G.proj)
    flat = orc.vdi_flatten([col], [dep], vb.VDI_W, vb.VDI_H, 0, vb.VDI_W, orc.ipv_of(G))
    img, _ = vb.render(col, dep, G, G, vb.VDI_W, vb.VDI_H)
    diff = np.abs(img.astype(np.int32) - flat.astype(np.int32))
    print(f"same camera vs flatten: max {diff.max()} LSB, {np.count_nonzero(diff)} of {diff.size} channels differ")
    assert np.count_nonzero(flat[..., 3]) > 200
    assert diff.max() <= 1


@pytest.mark.parametrize("size", vb.OUT_SIZES)
@pytest.mark.parametrize("name", list(CAMS))
def test_skip_and_layout_change_no_bit(brick_vdi, name, size):
    """Stepping over empty tiles, and reading the lists from the y-major view layout instead of the reference
    layout, give the same floats."""
    _, col, dep = brick_vdi
    counts = np.count_nonzero(dep[:, :, 0::2], axis=2)
    tiles = counts.reshape(vb.VDI_W // 8, 8, vb.VDI_H // 8, 8).max(axis=(1, 3))
    assert (tiles == 0).sum() >= 8 and (tiles > 0).sum() >= 4
    base_img, base = vb.render(col, dep, G, CAMS[name], *size, skip=False, repack=False)
    for skip, repack in ((True, False), (False, True), (True, True)):
        img, acc = vb.render(col, dep, G, CAMS[name], *size, skip=skip, repack=repack)
        assert np.array_equal(acc.view(np.uint32), base.view(np.uint32)), (skip, repack)
        assert np.array_equal(img, base_img)
    assert base[..., 3].sum() > 1.0


# ---------------------------------------------------------------- every VDI size, rays in cell planes, list ends
VDI_SIZES = ((64, 48), (50, 37), (9, 7))   # whole tiles; a ragged last tile on both axes; less than two tiles


def _aligned_sizes(W, H):
    """Output sizes at which, from the generating camera, whole columns or rows of rays lie in a cell plane."""
    return ((2 * W, 2 * H), (4 * W, 4 * H), (2 * W, H), (W, 2 * H))


@pytest.mark.parametrize("name", list(CAMS))
@pytest.mark.parametrize("vdi_size", VDI_SIZES)
def test_walk_partitions_the_ray(vdi_size, name):
    """Whatever the lists hold: the intervals of the tiles a ray visits, and those of the cells it visits (skip
    off), add up to its range [s0, s1].  Consecutive granules share the plane between them, so the sum
    telescopes and the expected difference is 0; the allowance is one float ulp of 1 for each interval (the
    range itself is one rounded float subtraction).  A ray left out of the walk is off by its whole range."""
    W, H = vdi_size
    gen, cam = vb.gen_camera(W, H), vb.view_cameras(W, H)[name]
    col, dep = vb.slab_vdi(vb.SLAB, W, H, 1)
    sizes = [(W, H), (50, 37), (1, 1)]
    if name == "same":
        sizes += [*_aligned_sizes(W, H), (130, 3)]
    for size in sizes:
        _, _, part = vb.render(col, dep, gen, cam, *size, skip=False, part=True)
        span = part[..., 0]
        assert size != (W, H) or np.count_nonzero(span) > 0   # (the camera sees the VDI)
        for level, (cover, n) in (("tiles", (part[..., 1], part[..., 2])), ("cells", (part[..., 3], part[..., 4]))):
            off = np.abs(cover - span)
            print(f"partition {W}x{H} {name} {size} {level}: max |cover - span| {off.max():.3g}, "
                  f"most intervals {int(n.max())}, rays {np.count_nonzero(span)}")
            bad = off > n * 2.0 ** -24
            assert not bad.any(), (size, level, int(bad.sum()), np.argwhere(bad)[:4].tolist(), float(off.max()))


@pytest.mark.parametrize("vdi_size", VDI_SIZES[:2])
def test_plane_aligned_rays_match_analytic(vdi_size):
    """The generating camera at 2x and 4x the VDI's resolution: every other column and row of rays lies in a
    cell plane (q and n at noise level there).  Only the rays in an outer plane of the extent are left out:
    there the analytic image itself jumps."""
    W, H = vdi_size
    gen = vb.gen_camera(W, H)
    col, dep = vb.slab_vdi(vb.SLAB, W, H, 1)
    for size in _aligned_sizes(W, H):
        img, _ = vb.render(col, dep, gen, gen, *size)
        want = vb.analytic_slabs(vb.SLAB, gen, gen, *size, W=W, H=H)
        out = vb.on_outer_plane(gen, gen, *size, W, H)
        assert out.sum() <= size[0] + size[1]
        assert np.mean(want[~out][:, 3] > 0) >= 0.9
        err = np.abs(img.astype(np.float64) - np.clip(want, 0.0, 1.0) * 255.0).max(axis=2)
        black = np.count_nonzero((err > LSB) & ~out & (img[..., 3] == 0))
        print(f"aligned {W}x{H} at {size}: {err[~out].max():.3f} LSB, {int(out.sum())} rays in an outer plane left out")
        assert err[~out].max() <= LSB, (size, int(((err > LSB) & ~out).sum()), black)


@pytest.fixture(scope="module")
def many_layers():
    """20x12, S = 255: the slab cut into 255 abutting layers."""
    col, dep = vb.layered_vdi(255, 20, 12)
    starts = dep[:, :, 0::2]
    assert starts.shape[2] == 255 and len(np.unique(starts[0, 0])) == 255 and np.all(starts != 0.0)
    return col, dep


RAGGED = [((50, 37), 3, n) for n in ("same", "yaw20", "yaw90", "yaw180", "close")] + \
         [((9, 7), 1, n) for n in ("same", "yaw20", "yaw90", "yaw180", "close")]


@pytest.mark.parametrize("vdi_size,S,name", RAGGED)
def test_ragged_vdi_matches_analytic(vdi_size, S, name):
    """VDIs whose last tile is partial on both axes (and one smaller than two tiles), S = 3 and S = 1."""
    W, H = vdi_size
    gen, cam = vb.gen_camera(W, H), vb.view_cameras(W, H)[name]
    col, dep = vb.slab_vdi(vb.SLAB, W, H, S)
    for size in ((W, H), (41, 29), (130, 3)):
        base_img, base = vb.render(col, dep, gen, cam, *size, skip=False, repack=False)
        want = vb.analytic_slabs(vb.SLAB, gen, cam, *size, W=W, H=H)
        err = vb.lsb_error(base_img, want)
        print(f"ragged {W}x{H} S={S} {name} {size}: {err:.3f} LSB, coverage {np.mean(want[..., 3] > 0):.2f}")
        assert err <= LSB
        for skip, repack in ((True, False), (False, True), (True, True)):
            img, acc = vb.render(col, dep, gen, cam, *size, skip=skip, repack=repack)
            assert np.array_equal(acc.view(np.uint32), base.view(np.uint32)), (skip, repack)
            assert np.array_equal(img, base_img)
    assert np.any(want[..., 3] > 0)


@pytest.mark.parametrize("name", ["yaw20", "yaw180"])
def test_255_layers_match_the_one_slab(many_layers, name):
    """S at its limit (counts and the tiles' largest count are uint8): 255 abutting layers give the single
    slab's image, first to last and last to first."""
    col, dep = many_layers
    W, H = 20, 12
    gen, cam = vb.gen_camera(W, H), vb.view_cameras(W, H)[name]
    for size in ((W, H), (41, 29)):
        base_img, base = vb.render(col, dep, gen, cam, *size, skip=False, repack=False)
        want = vb.analytic_slabs(vb.SLAB, gen, cam, *size, W=W, H=H)
        err = vb.lsb_error(base_img, want)
        print(f"255 layers {name} {size}: {err:.3f} LSB, coverage {np.mean(want[..., 3] > 0):.2f}")
        assert np.mean(want[..., 3] > 0) > 0.2
        assert err <= LSB
        img, acc = vb.render(col, dep, gen, cam, *size, skip=True, repack=True)
        assert np.array_equal(acc.view(np.uint32), base.view(np.uint32)) and np.array_equal(img, base_img)


@pytest.mark.parametrize("repack", [False, True])
def test_list_ends_at_first_zero_start(repack):
    """A list ends at its first entry with start depth 0, whatever lies behind it, or at S entries."""
    col, dep = vb.list_end_vdi()
    W, H, S = col.shape[:3]
    counts = np.cumprod(dep[:, :, 0::2] != 0.0, axis=2).sum(axis=2)
    assert {0, 2, 3, S} == set(np.unique(counts))
    assert np.count_nonzero(dep[2, 1, 0::2]) == 4 and dep[2, 1, 4] == 0.0   # 2 entries, a zero start, 2 more
    tcol, tdep = vb.truncate_lists(col, dep)
    assert not np.array_equal(tdep, dep) and np.array_equal(tdep[9, 3], dep[9, 3])
    gen, cam = vb.gen_camera(W, H), vb.view_cameras(W, H)["yaw20"]
    for size in ((W, H), (41, 29)):
        img, acc = vb.render(col, dep, gen, cam, *size, repack=repack)
        timg, tacc = vb.render(tcol, tdep, gen, cam, *size, repack=repack)
        assert np.array_equal(acc.view(np.uint32), tacc.view(np.uint32)) and np.array_equal(img, timg)
        # the entries behind the zero start would show: the same lists with that entry filled in look different
        fcol, fdep = vb.layered_vdi(6, W, H)
        ucol, udep = col.copy(), dep.copy()
        ucol[2:7, 1:5, 2], udep[2:7, 1:5, 4:6] = fcol[2:7, 1:5, 2], fdep[2:7, 1:5, 4:6]
        _, uacc = vb.render(ucol, udep, gen, cam, *size, repack=repack)
        assert not np.array_equal(uacc, acc)
