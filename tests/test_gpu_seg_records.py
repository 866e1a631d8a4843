"""GPU parity of the search kernel's supersegment records (SegRecord): vdi_search_kernel stores every
supersegment a deferred ray closes as one 32-byte record through a running per-lane pointer, and
vdi_finish_kernel turns the records of a pixel's final count into its colour and depth entries.  Every case is
bit for bit against the CPU oracle, and asserts first -- on the oracle's output -- that the scene does what the
case is there for:

  * rays that close fewer than S, exactly S and more than S supersegments in their write pass (the ones past S
    are not stored: their octree cells are counted by the search itself), at S = 4 and S = 20;
  * rays of 8 and more passes, whose late search passes store speculatively into the records the accepted pass
    or the write pass overwrites, with the filtered and with the exact decisions;
  * two volumes merged into one sub-VDI (the merged-volume search shares the loop);
  * a 52-pixel window on two ranks: 26-pixel strips, so the record pointer's slot stride and the strip offset
    must agree with the send layout off the 8-grid;
  * pipelined frames whose per-pixel counts fall from a slot's frame to its next one: the slot's records past
    the new counts are the older frame's and must not be read.
"""
from __future__ import annotations

import functools

import numpy as np
import pytest

import oracle_binding as orc
import pyref
from insitu_amd import native, scene
from insitu_amd.renderer import InSituContext, LocalGroup
from scenes import make_scene, variant_scene

pytestmark = pytest.mark.gpu

W, H = 64, 48


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _inputs(sc, cam=None):
    return orc.Inputs(sc["vol"], sc["im"], sc["tf"], sc["cmap"], sc["conv_k"], sc["conv_offset"],
                      sc["cam"] if cam is None else cam)


def _counts(depth):
    """Stored supersegments per pixel (x, y) of a reference-layout depth array."""
    return np.count_nonzero(depth[..., 0::2] != 0, axis=-1)


def _frozen(out):
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _oracle_variant(name, S):
    """The oracle's sub-VDI (colour, depth, octree, passes) of scenes.variant_scene(name); shared, never modified."""
    return _frozen(orc.vdi_generate(_inputs(variant_scene(name, W, H)), W, H, S))


def _assert_sub_vdi(got, ref, what=""):
    (col, dep, octree, passes), (rc, rd, ro, rp) = got, ref
    bad = np.count_nonzero(_bits(col) != _bits(rc)) + np.count_nonzero(_bits(dep) != _bits(rd))
    if bad:
        where = np.argwhere(np.any(_bits(dep) != _bits(rd), axis=2) | np.any(_bits(col) != _bits(rc), axis=(2, 3)))
        raise AssertionError(f"{what}{bad} mismatching sub-VDI words; stored counts equal on "
                             f"{np.mean(_counts(dep) == _counts(rd)):.4f} of the pixels; first bad (x, y) {where[:5].tolist()}")
    assert np.array_equal(octree, ro), f"{what}octree cells differ"
    assert np.array_equal(passes.astype(np.int32), rp), f"{what}pass counts differ"


def _render(sc, S, options=()):
    with InSituContext(sc["W"], sc["H"], max_supersegments=S, keep_passes=True) as ctx:
        ctx.set_transfer(sc["tf"], sc["cmap"], sc["conv_scale"], sc["conv_offset"])
        for opt, val in options:
            ctx.set_option(opt, val)
        ctx.set_brick(0, sc["vol"], sc["model"])
        ctx.render(sc["cam"])
        got = (ctx.read(native.BUF_VDI_COLOR), ctx.read(native.BUF_VDI_DEPTH), ctx.read(native.BUF_OCTREE),
               ctx.read(native.BUF_PASSES))
        st = ctx.stats()
    return got, st


def _closed_in_write_pass(sc, x, y, S, ref):
    """Supersegments pixel (x, y) closes in its write pass, stored or not: the oracle keeps the first S only, so the
    count comes from the pure-Python restatement the oracle is pinned to (tests/test_oracle_pin.py), which must
    reproduce the oracle's stored entries and pass count of the pixel."""
    vol, c = sc["vol"], sc["cam"]
    V = pyref.Volume(vol.ravel().tolist(), (vol.shape[2], vol.shape[1], vol.shape[0]), sc["im"].tolist(),
                     sc["tf"].tolist(), sc["cmap"].tolist(), float(sc["conv_k"]), float(sc["conv_offset"]))
    cam = dict(view=c.view.tolist(), proj=c.proj.tolist(), inv_view=c.inv_view.tolist(), inv_proj=c.inv_proj.tolist(),
               nw=float(c.nw), fwnw=float(c.fwnw), tmax=float(c.tmax))
    written, _, passes = pyref.vdi_pixel(V, cam, int(x), int(y), sc["W"], sc["H"], S)
    rc, rd, _, rp = ref
    assert passes == rp[y, x]
    starts = np.asarray([w[0] for w in written[:S]], np.float32)
    assert np.array_equal(_bits(starts), _bits(rd[x, y, 0:2 * len(starts):2]))
    return len(written)


@pytest.mark.parametrize("S", [4, 20])
def test_counts_below_at_and_above_S(S):
    """One 32^3 brick at 64x48 under the `big` colour map (scenes.cmap_variant: rgb up to 4.9e5, so neighbouring
    samples differ by more than any threshold the search can reach): most rays that search end at the largest
    threshold with more than S supersegments in the write pass, the short ones settle with S or fewer."""
    sc = variant_scene("big", W, H)
    ref = _oracle_variant("big", S)
    _, rd, _, rp = ref
    cnt, passes = _counts(rd), rp.T
    # every cached ray has its write pass in the search kernel, the ones found in pass 1 (2 passes) too
    assert np.count_nonzero((cnt > 0) & (cnt < S)) >= 20, "too few rays close fewer than S supersegments"
    full = cnt == S
    # a search that never finds a count <= S ends with the range closed (pass 24): its write pass overflows
    over, at = np.argwhere(full & (passes == passes.max())), np.argwhere(full & (passes < passes.max()))
    assert len(over) and len(at), (len(over), len(at))
    closed_over = _closed_in_write_pass(sc, *over[0], S, ref)
    closed_at = _closed_in_write_pass(sc, *at[0], S, ref)
    assert closed_over > S, f"pixel {over[0].tolist()} closes {closed_over} supersegments, not more than {S}"
    assert closed_at == S, f"pixel {at[0].tolist()} closes {closed_at} supersegments, not {S}"
    got, st = _render(sc, S)
    assert st["rays_searched"] > 0 and st["rays_uncached"] == 0
    _assert_sub_vdi(got, ref)


@pytest.mark.parametrize("exact", [0, 1], ids=["filtered", "exact_search"])
def test_speculative_stores_are_overwritten(exact):
    """The base scene at S = 8: rays of 8 and more passes (up to 24) store the supersegments of their late search
    passes into their own records; what counts is the accepted pass's or the write pass's records alone."""
    S = 8
    sc = variant_scene("base", W, H)
    ref = _oracle_variant("base", S)
    assert np.count_nonzero(ref[3] >= 8) >= 50, "the scene needs rays of 8 and more passes"
    got, st = _render(sc, S, options=((native.OPT_EXACT_SEARCH, exact),))
    assert st["rays_searched"] > 0
    _assert_sub_vdi(got, ref)


def test_merged_bricks_records():
    """Two 16^3 volumes rendered into one sub-VDI (merge_bricks) at S = 8: vdi_search_kernel<., true>."""
    S = 8
    scs = [make_scene(n=16, W=W, H=H, yaw=35.0),
           make_scene(n=16, W=W, H=H, yaw=35.0, seed=7, origin=(0.0, -0.25, -0.75))]
    cam = scs[0]["cam"]
    ref = orc.vdi_generate_multi([_inputs(sc, cam) for sc in scs], W, H, S)
    assert np.count_nonzero(ref[3] > 2) >= 50 and ref[3].max() >= 8, "the merged rays must search, some of them long"
    with InSituContext(W, H, max_supersegments=S, bricks_per_rank=2, keep_passes=True, merge_bricks=True) as ctx:
        ctx.set_transfer(scs[0]["tf"], scs[0]["cmap"], scs[0]["conv_scale"], scs[0]["conv_offset"])
        for b, sc in enumerate(scs):
            ctx.set_brick(b, sc["vol"], sc["model"])
        img = ctx.frame(cam, want_image=True)
        st = ctx.stats()
        got = (ctx.read(native.BUF_VDI_COLOR), ctx.read(native.BUF_VDI_DEPTH), ctx.read(native.BUF_OCTREE),
               ctx.read(native.BUF_PASSES))
    assert st["rays_searched"] > 0
    _assert_sub_vdi(got, ref)
    assert np.array_equal(img, orc.vdi_flatten([ref[0]], [ref[1]], W, H, 0, W, orc.ipv_of(cam)))


def test_ragged_strips_records():
    """A 52x48 window on two local ranks (26-pixel strips: three whole tile columns and a partial one in each), one
    32^3 brick per rank, S = 8: each rank's sub-VDI over the whole width, and rank 0's image of both lists."""
    Wr, S, world = 52, 8, 2
    scs = [make_scene(n=32, W=Wr, H=H, yaw=40.0),
           make_scene(n=32, W=Wr, H=H, yaw=40.0, seed=7)]   # (another field in the same place)
    # (from nearby: at the default radius the outer tile columns of the window are empty)
    cam = scene.orbit_camera(Wr, H, radius=1.2, yaw_deg=40.0, pitch_deg=20.0, voxel_world=1.0 / 32)
    refs = [orc.vdi_generate(_inputs(sc, cam), Wr, H, S) for sc in scs]
    sw = Wr // world
    for r, ref in enumerate(refs):
        deferred = (_counts(ref[1]) > 0) & (ref[3].T > 2)
        per_strip = deferred.reshape(world, sw, H)
        assert np.all(per_strip[:, 24:, :].sum(axis=(1, 2)) > 0), f"brick {r}: a strip's partial tile column stores no searched ray"
    group = LocalGroup(world)
    ctxs = []
    try:
        for r in range(world):
            ctx = InSituContext(Wr, H, max_supersegments=S, keep_passes=True, rank=r, nranks=world, local_group=group)
            ctxs.append(ctx)
            ctx.set_transfer(scs[0]["tf"], scs[0]["cmap"], scs[0]["conv_scale"], scs[0]["conv_offset"])
            ctx.set_brick(0, scs[r]["vol"], scs[r]["model"])
        for stage in ("render", "exchange", "composite"):
            for ctx in ctxs:
                ctx.render(cam) if stage == "render" else getattr(ctx, stage)()
        ctxs[1].gather(want_image=False)
        img = ctxs[0].gather(want_image=True)
        got = [(ctx.read(native.BUF_VDI_COLOR), ctx.read(native.BUF_VDI_DEPTH), ctx.read(native.BUF_OCTREE),
                ctx.read(native.BUF_PASSES)) for ctx in ctxs]
    finally:
        for ctx in ctxs:
            ctx.close()
        group.close()
    for r in range(world):
        _assert_sub_vdi(got[r], refs[r], f"rank {r}: ")
    want = orc.vdi_flatten([r[0] for r in refs], [r[1] for r in refs], Wr, H, 0, Wr, orc.ipv_of(cam))
    assert np.count_nonzero(want[..., 3]) > 0
    assert np.array_equal(img, want)


def test_two_slots_falling_counts():
    """Three pipelined frames and the flush at S = 8, the camera backing away from the brick: frames 0 and 2 share a
    frame slot, frame 1 has the other.  Where a pixel's count falls from one frame to a later one the slot's
    records past the new count are the older frame's; every completed frame equals the oracle's frame of its
    camera alone."""
    S = 8
    sc = make_scene(n=32, W=W, H=H)
    cams = [scene.orbit_camera(W, H, radius=r, yaw_deg=30.0 + 20.0 * i, pitch_deg=20.0, voxel_world=1.0 / 32)
            for i, r in enumerate((2.2, 3.0, 4.0))]
    refs = [orc.vdi_generate(_inputs(sc, cam), W, H, S) for cam in cams]
    cnt = [np.where(r[3].T > 2, _counts(r[1]), 0) for r in refs]   # of searched rays: the deferred pixels
    for a, b in ((0, 1), (1, 2), (0, 2)):
        falls = np.count_nonzero((cnt[b] > 0) & (cnt[b] < cnt[a]))
        assert falls >= 20, f"frame {b} lowers the count of only {falls} searched pixels of frame {a}"
    seen = []
    with InSituContext(W, H, max_supersegments=S, keep_passes=True) as ctx:
        ctx.set_transfer(sc["tf"], sc["cmap"], sc["conv_scale"], sc["conv_offset"])
        ctx.set_brick(0, sc["vol"], sc["model"])
        steps = [functools.partial(ctx.frame_pipelined, cam, want_image=True) for cam in cams]
        steps.append(functools.partial(ctx.pipeline_flush, want_image=True))
        for step in steps:
            done, img = step()
            if done < 0:
                continue
            seen.append(done)
            assert ctx.stats()["pipelined"] == 1
            got = (ctx.read(native.BUF_VDI_COLOR), ctx.read(native.BUF_VDI_DEPTH), ctx.read(native.BUF_OCTREE),
                   ctx.read(native.BUF_PASSES))
            _assert_sub_vdi(got, refs[done], f"frame {done}: ")
            want = orc.vdi_flatten([refs[done][0]], [refs[done][1]], W, H, 0, W, orc.ipv_of(cams[done]))
            assert np.array_equal(img, want), f"frame {done}: image differs"
    assert seen == [0, 1, 2]
