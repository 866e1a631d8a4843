"""N-rank parity on strips that are not whole 8x8 tiles: libinsitu_hip.so's multi-rank data path (in-process
rank group) against the CPU oracle, bit for bit, at windows whose strip width W / N and height are off the
8-grid -- a partial tile column inside the image once per strip, strips narrower than a tile, a partial
last tile row, and peers that get no entry at all.

Scene (scenes.strip_bricks / strip_camera): the 24^3 Gray-Scott bricks of the group tests in
test_gpu_parity.py, seen from radius 2.0 (yaw 35, pitch 20), S = 6.  World 2 and 4 split 4 bricks (2 x 2 x 1),
world 3 the first 6 and world 8 all of 2 x 2 x 2 bricks (one number of bricks per rank: 4 bricks do not
split over 3 ranks).  What the oracle stores there, checked by _conditions() on the oracle's output before
anything is compared:

  W x H x ranks  strip_w  entries per strip                    bricks per strip  (source, destination) pairs
                                                                                  without / with entries
  60 x 37 x 4    15       663 4414 4502 2313                   2 4 4 2            4 / 8
  50 x 37 x 2    25       5077 6656                            4 4                0 / 2
  57 x 41 x 3    19       3168 8329 5704                       4 6 4              0 / 6
  40 x 37 x 8    5        1602 2492 3301 3247 3059 3085        4 6 6 6 6 6 4 4    17 / 39
                          2618 2549
  12 x  9 x 4    3        55 214 236 187                       2 4 4 2            4 / 8
  64 x 48 x 4    16       2077 6535 6384 4711 (aligned control) 2 4 4 2           4 / 8

  - every strip holds entries of at least 2 bricks;
  - every strip's last, partial tile column holds entries (60x37: 663 2623 1792 398; 50x37: 437 107;
    57x41: 1017 1406 426; strips narrower than a tile are that column);
  - the partial last tile row holds entries (60x37: 1069, 50x37: 1069, 57x41: 438, 40x37: 2480, 12x9: 60);
  - world 8 (and world 4) have peers whose whole message is empty, and peers whose message is not.

A second GPU context is no reference here: every expected value is the oracle's.  The whole-frame and the
per-strip oracle composites are interchangeable (test_compositor_oracle.py pins that on the CPU).
"""
from __future__ import annotations

import functools

import numpy as np
import pytest

import oracle_binding as orc
from insitu_amd import native
from insitu_amd.renderer import InSituContext, LocalGroup
from scenes import STRIP_S as S
from scenes import strip_bricks, strip_camera

pytestmark = pytest.mark.gpu

S_OUT = 4
# (W, H, ranks)
GEOMETRIES = [(60, 37, 4), (50, 37, 2), (57, 41, 3), (40, 37, 8), (12, 9, 4), (64, 48, 4)]
NBRICKS = {2: 4, 3: 6, 4: 4, 8: 8}


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _assert_bits(got, ref, what):
    """Bit-for-bit equality of two float32 (or integer) arrays, reporting the count and place of the mismatches."""
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    if got.dtype == np.float32:
        got, ref = _bits(got), _bits(ref)
    bad = got != ref
    if bad.any():
        where = np.argwhere(bad)
        raise AssertionError(f"{what}: {np.count_nonzero(bad)} of {bad.size} words differ; first at {where[:6].tolist()}, "
                             f"index ranges {where.min(axis=0).tolist()} .. {where.max(axis=0).tolist()}")


def _counts(depth):
    """Stored entries per pixel of a reference-layout depth array (..., 2S): the slots with a non-zero start."""
    return np.count_nonzero(depth[..., 0::2] != 0, axis=-1)


@functools.lru_cache(maxsize=None)
def _oracle(W, H, nb, yaw=35.0, pitch=20.0, merged_by=0):
    """The oracle's frame of the strip scene: sub-VDIs (colour, depth, octree, passes) of every list -- one per
    brick, or with merged_by one per group of merged_by bricks rendered into one VDI -- their entry counts
    (lists, W, H), and the whole-width composite and both images.  Computed once and shared; never modified."""
    bricks = strip_bricks(nb)
    cam = strip_camera(W, H, yaw, pitch)
    inps = [orc.Inputs(b["vol"], b["im"], b["tf"], b["cmap"], b["conv_k"], b["conv_offset"], cam) for b in bricks]
    if merged_by:
        subs = [orc.vdi_generate_multi(inps[i:i + merged_by], W, H, S) for i in range(0, nb, merged_by)]
    else:
        subs = [orc.vdi_generate(inp, W, H, S) for inp in inps]
    cols, deps = [s[0] for s in subs], [s[1] for s in subs]
    ipv = orc.ipv_of(cam)
    ref = dict(cam=cam, ipv=ipv, subs=subs, cols=cols, deps=deps, cnt=np.stack([_counts(d) for d in deps]))
    for d in deps:   # compact lists: the entry count is the list length the exchange packs
        assert np.all(np.diff((d[..., 0::2] != 0).astype(np.int8), axis=2) <= 0)
    ref["flat_image"] = orc.vdi_flatten(cols, deps, W, H, 0, W, ipv)
    ref["composited"] = orc.vdi_composite(cols, deps, W, H, 0, W, ipv, S_OUT)
    ref["composited_image"] = orc.vdi_flatten([ref["composited"][0]], [ref["composited"][1]], W, H, 0, W, ipv)
    for a in (*cols, *deps, ref["cnt"], ref["flat_image"], *ref["composited"], ref["composited_image"]):
        a.setflags(write=False)
    return ref


def _conditions(ref, W, H, world, lists_per_rank):
    """The scene does what the geometry is there for (on the oracle's output, so a quiet scene cannot hide a
    failure).  Returns the (source rank, destination) entry totals."""
    sw = W // world
    cnt = ref["cnt"]
    per = cnt.reshape(cnt.shape[0], world, sw, H)             # (list, strip, xl, y)
    per_strip = per.sum(axis=(2, 3))                          # (list, strip)
    assert np.all((per_strip > 0).sum(axis=0) >= 2), f"a strip has entries of fewer than 2 lists: {per_strip.tolist()}"
    if sw % 8:
        edge = per[:, :, (sw // 8) * 8:, :].sum(axis=(0, 2, 3))
        assert np.all(edge > 0), f"a strip's partial tile column is empty: {edge.tolist()}"
    if H % 8:
        assert per[:, :, :, (H // 8) * 8:].sum() > 0, "the partial last tile row is empty"
    pairs = per_strip.reshape(world, lists_per_rank, world).sum(axis=1)   # (source rank, destination)
    if world == 8:
        off = pairs[~np.eye(world, dtype=bool)]
        assert np.any(off == 0) and np.any(off > 0), "world 8 needs empty and non-empty peer messages"
    return pairs


def _open(W, H, world, nb, *, composite_vdi=False, merge=False, mode=native.MODE_VDI, options=()):
    """A local group of `world` contexts holding the strip scene's nb bricks, nb / world each."""
    bricks = strip_bricks(nb)
    B = nb // world
    group = LocalGroup(world)
    ctxs = []
    try:
        for r in range(world):
            ctx = InSituContext(W, H, mode=mode, max_supersegments=S, bricks_per_rank=B, rank=r, nranks=world,
                                local_group=group, composite_vdi=composite_vdi,
                                max_output_supersegments=S_OUT if composite_vdi else 0, merge_bricks=merge)
            ctxs.append(ctx)
            b0 = bricks[0]
            ctx.set_transfer(b0["tf"], b0["cmap"], b0["conv_scale"], b0["conv_offset"])
            for opt, val in options:
                ctx.set_option(opt, val)
            for b in range(B):
                ctx.set_brick(b, bricks[r * B + b]["vol"], bricks[r * B + b]["model"])
    except Exception:
        _close(group, ctxs)
        raise
    return group, ctxs


def _close(group, ctxs):
    for ctx in ctxs:
        ctx.close()
    group.close()


def _frame(ctxs, cam):
    """One frame, stage by stage across the ranks; rank 0's image."""
    for ctx in ctxs:
        ctx.render(cam)
    for ctx in ctxs:
        ctx.exchange()
    for ctx in ctxs:
        ctx.composite()
    for ctx in ctxs[1:]:
        ctx.gather(want_image=False)
    return ctxs[0].gather(want_image=True)


def _read_vdi_frame(ctxs, composite_vdi, lists_per_rank):
    """Everything the checks compare, read back from every rank."""
    got = []
    for ctx in ctxs:
        g = dict(stats=ctx.stats())
        g["subs"] = [(ctx.read(native.BUF_VDI_COLOR, b), ctx.read(native.BUF_VDI_DEPTH, b),
                      ctx.read(native.BUF_OCTREE, b), ctx.read(native.BUF_PASSES, b))
                     for b in range(lists_per_rank)]
        x0, x1 = max(0, ctx.strip_w - 3), min(ctx.width, ctx.strip_w + 5)   # a column band across the first seam
        g["seam"] = (x0, x1, ctx.read_columns(native.BUF_VDI_COLOR, x0, x1), ctx.read_columns(native.BUF_VDI_DEPTH, x0, x1),
                     ctx.read_columns(native.BUF_PASSES, x0, x1))
        g["recv"] = (ctx.read(native.BUF_RECEIVED_COLOR), ctx.read(native.BUF_RECEIVED_DEPTH))
        if composite_vdi:
            g["comp"] = (ctx.read(native.BUF_COMPOSITED_COLOR), ctx.read(native.BUF_COMPOSITED_DEPTH),
                         ctx.read(native.BUF_COMPOSITE_PASSES))
        got.append(g)
    if composite_vdi:
        got[0]["gathered"] = (ctxs[0].read(native.BUF_GATHERED_COLOR), ctxs[0].read(native.BUF_GATHERED_DEPTH))
    return got


def _check_vdi_frame(ref, img, got, W, H, world, composite_vdi, lists_per_rank, pairs):
    sw = W // world
    nl = world * lists_per_rank
    for r, g in enumerate(got):
        # sub-VDIs over the full width: the generator under the N-rank tile grid
        for b, (c, d, o, p) in enumerate(g["subs"]):
            rc, rd, ro, rp = ref["subs"][r * lists_per_rank + b]
            _assert_bits(c, rc, f"rank {r} list {b} sub-VDI colour (x, y, slot, channel)")
            _assert_bits(d, rd, f"rank {r} list {b} sub-VDI depth (x, y, word)")
            _assert_bits(o, ro, f"rank {r} list {b} octree (slot, cell y, cell x)")
            _assert_bits(p.astype(np.int32), rp, f"rank {r} list {b} pass counts (y, x)")
        x0, x1, sc_, sd_, sp_ = g["seam"]   # the region readback of list 0, a band that straddles strips 0 and 1
        rc, rd, _, rp = ref["subs"][r * lists_per_rank]
        _assert_bits(sc_, rc[x0:x1], f"rank {r} columns [{x0}, {x1}) colour (x - {x0}, y, slot, channel)")
        _assert_bits(sd_, rd[x0:x1], f"rank {r} columns [{x0}, {x1}) depth (x - {x0}, y, word)")
        _assert_bits(sp_.astype(np.int32), rp[:, x0:x1], f"rank {r} columns [{x0}, {x1}) pass counts (y, x - {x0})")
        # the received set: strip r of every list, source-major
        rcol, rdep = g["recv"]
        assert rcol.shape == (nl, sw, H, S, 4) and rdep.shape == (nl, sw, H, 2 * S), (rcol.shape, rdep.shape)
        for v in range(nl):
            _assert_bits(rcol[v], ref["cols"][v][r * sw:(r + 1) * sw], f"rank {r} received list {v} colour (xl, y, slot, channel)")
            _assert_bits(rdep[v], ref["deps"][v][r * sw:(r + 1) * sw], f"rank {r} received list {v} depth (xl, y, word)")
        if composite_vdi:
            oc, od, op = orc.vdi_composite(ref["cols"], ref["deps"], W, H, r * sw, sw, ref["ipv"], S_OUT)
            _assert_bits(g["comp"][0], oc, f"rank {r} composited colour (xl, y, slot, channel)")
            _assert_bits(g["comp"][1], od, f"rank {r} composited depth (xl, y, word)")
            _assert_bits(g["comp"][2].astype(np.int32), op, f"rank {r} composite pass counts (y, xl)")
        # the exchange sent the meta block to every peer and exactly the stored entries outside the own strip
        tiles = ((sw + 7) // 8) * ((H + 7) // 8)
        meta_bytes = lists_per_rank * tiles * 68
        sent = int(pairs[r].sum() - pairs[r, r])
        assert g["stats"]["exchange_entries"] == sent, (r, g["stats"]["exchange_entries"], sent)
        assert g["stats"]["exchange_bytes"] == (world - 1) * meta_bytes + 24 * sent, (r, g["stats"]["exchange_bytes"])
    if composite_vdi:
        _assert_bits(got[0]["gathered"][0], ref["composited"][0], "gathered composited colour (x, y, slot, channel)")
        _assert_bits(got[0]["gathered"][1], ref["composited"][1], "gathered composited depth (x, y, word)")
    want = ref["composited_image"] if composite_vdi else ref["flat_image"]
    assert np.count_nonzero(want[..., 3]) > 0
    _assert_bits(img, want, "rank 0's image (y, x, channel)")


def _run_vdi_case(W, H, world, composite_vdi, options=(), frames=1):
    nb = NBRICKS[world]
    ref = _oracle(W, H, nb)
    pairs = _conditions(ref, W, H, world, nb // world)
    group, ctxs = _open(W, H, world, nb, composite_vdi=composite_vdi, options=options)
    try:
        for _ in range(frames):
            img = _frame(ctxs, ref["cam"])
        got = _read_vdi_frame(ctxs, composite_vdi, nb // world)
    finally:
        _close(group, ctxs)
    _check_vdi_frame(ref, img, got, W, H, world, composite_vdi, nb // world, pairs)


@pytest.mark.parametrize("composite_vdi", [False, True], ids=["flatten", "compositor"])
@pytest.mark.parametrize("W,H,world", GEOMETRIES)
def test_ragged_strips_bit_exact(W, H, world, composite_vdi):
    """One frame on `world` ranks: every rank's sub-VDIs (with octree and pass counts; whole, and a column band
    across the first strip seam through insitu_read_region), the lists it received,
    its composited strip and pass counts, the gathered composited VDI, rank 0's image and the exchange's byte
    and entry counts equal the oracle's."""
    _run_vdi_case(W, H, world, composite_vdi)


@pytest.mark.parametrize("option,value", [(native.OPT_SUPER_TILE, 2), (native.OPT_SUPER_TILE, 4),
                                          (native.OPT_TILE_ORDER, 0), (native.OPT_EXACT_TILE_KEYS, 1)],
                         ids=["super_tile2", "super_tile4", "tile_order0", "exact_tile_keys"])
def test_ragged_strips_tile_order_options(option, value):
    """The sampling kernel's tile-order options over the N-rank tile grid with partial tile columns in
    mid-image (60x37 on 4 ranks, compositor path), set on every rank: the second of two frames
    (it reuses the queue, the cache and the tile order of the first) equals the oracle's like any other."""
    _run_vdi_case(60, 37, 4, True, options=((option, value),), frames=2)


def test_ragged_strips_merged_bricks():
    """merge_bricks on 2 ranks at 50x37 (2 bricks each, one list per rank, 25-pixel strips): each rank's one
    sub-VDI equals the oracle's multi-volume VDI, and the lists are exchanged and flattened like any other."""
    W, H, world, nb = 50, 37, 2, 4
    ref = _oracle(W, H, nb, merged_by=2)
    pairs = _conditions(ref, W, H, world, 1)
    group, ctxs = _open(W, H, world, nb, merge=True)
    try:
        img = _frame(ctxs, ref["cam"])
        got = _read_vdi_frame(ctxs, False, 1)
    finally:
        _close(group, ctxs)
    _check_vdi_frame(ref, img, got, W, H, world, False, 1, pairs)


def test_ragged_strips_falling_counts():
    """Two frames through the compositor path at 60x37 on 4 ranks, the second from another camera, so that many
    pixels of the ragged strips get fewer output supersegments than before (the slots past a pixel's new count
    keep the first frame's data): the second frame equals the oracle's frame of its camera alone."""
    W, H, world, nb = 60, 37, 4, 4
    first, second = _oracle(W, H, nb), _oracle(W, H, nb, yaw=35.0, pitch=-40.0)
    falls = _counts(second["composited"][1]) < _counts(first["composited"][1])
    sw = W // world
    per_strip = [int(falls[r * sw:(r + 1) * sw].sum()) for r in range(world)]   # the oracle: 88, 65, 0, 72 pixels
    assert sum(n > 0 for n in per_strip) >= 3, f"counts must fall on most strips: {per_strip}"
    _conditions(first, W, H, world, 1)
    pairs = _conditions(second, W, H, world, 1)
    group, ctxs = _open(W, H, world, nb, composite_vdi=True)
    try:
        counts = []
        for ref in (first, second):
            img = _frame(ctxs, ref["cam"])
            counts.append(_counts(ctxs[0].read(native.BUF_GATHERED_DEPTH)))
        got = _read_vdi_frame(ctxs, True, 1)
    finally:
        _close(group, ctxs)
    assert np.count_nonzero(counts[1] < counts[0]) > 0, "the second frame must lower some pixels' counts"
    _check_vdi_frame(second, img, got, W, H, world, True, 1, pairs)


@pytest.mark.parametrize("W,H,world", [(50, 36, 4), (57, 39, 3)])
def test_plain_ragged_row_strips(W, H, world):
    """Plain mode on N > 1 ranks with row strips off the 8-grid (9 rows of 50 and 13 rows of 57 pixels): each
    rank's plain colour and depth images equal the oracle's plain_raycast of its bricks, rank 0's image the
    oracle's plain_composite of all of them."""
    nb = NBRICKS[world]
    B = nb // world
    bricks = strip_bricks(nb)
    cam = strip_camera(W, H)
    refs = [orc.plain_raycast(orc.Inputs(b["vol"], b["im"], b["tf"], b["cmap"], b["conv_k"], b["conv_offset"], cam), W, H)
            for b in bricks]
    rows = H // world
    hit = np.stack([c[..., 3] != 0 for c, _ in refs]).reshape(nb, world, rows, W).any(axis=(2, 3))   # (brick, strip)
    assert np.all(hit.sum(axis=0) >= 2), f"a row strip shows fewer than 2 bricks: {hit.sum(axis=0).tolist()}"
    group, ctxs = _open(W, H, world, nb, mode=native.MODE_PLAIN)
    try:
        img = _frame(ctxs, cam)
        got = [[(ctx.read(native.BUF_PLAIN_COLOR, b), ctx.read(native.BUF_PLAIN_DEPTH, b)) for b in range(B)]
               for ctx in ctxs]
    finally:
        _close(group, ctxs)
    for r in range(world):
        for b in range(B):
            _assert_bits(got[r][b][0], refs[r * B + b][0], f"rank {r} brick {b} plain colour (y, x, channel)")
            _assert_bits(got[r][b][1], refs[r * B + b][1], f"rank {r} brick {b} plain depth (y, x, channel)")
    want = orc.plain_composite([c for c, _ in refs], [d for _, d in refs], H)
    assert np.count_nonzero(want[..., 3]) > 0
    _assert_bits(img, want, "rank 0's plain image (y, x, channel)")
