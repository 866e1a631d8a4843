"""GPU checks of insitu_view_gather_merged (csrc/insitu_view.cpp): every rank's bound VDI
gathered into one merged VDI bound on rank 0, device to device.  The root's VDI is read back through
view_pack(PACK_FLOAT); what it must hold never comes from the call under test: vdi_io.pack_vdi of the plain loop's merge
(tests/test_pack_set.py loop_merge_set) of the ranks' read-back sub-VDIs, INSITU_VIEW_MERGED of a one-rank context that
holds every brick, and insitu_view_bind_packed_set of the ranks' view_pack streams.  Local groups of 2 and 4 ranks over
the abutting 2x2 bricks at 64x48 and 50x37, both layouts on the root and a peer in the other one, both formats, renders
against tests/view_ref, the peers' bindings, repeated gathers, crafted ranks bound from host memory (differing S, an
empty rank, ties, nine ranks, more than 255 merged entries), every rejection, one rank alone, and the same over RCCL in
separate processes (tests/view_gather_worker.py)."""
from __future__ import annotations

import os
import socket
import struct
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import view_binding as vb
from insitu_amd import native, scene
from insitu_amd.renderer import InSituContext, LocalGroup
from insitu_amd.vdi_io import PACK_FLOAT, PACK_HALF, pack_vdi, unpack_vdi
from test_gpu_view_pack_set import _layout_bytes, _nothing_bound
from test_pack_set import layered_streams, loop_merge_set, merged_stream, tie_streams
from test_vdi_pack import random_vdi
from test_view_merge import scene_set
from view_binding import bits as _bits, fails as _fails, read_all as _read_all, set_bricks as _set_bricks

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
S = vb.VDI_S
FORMATS = (PACK_FLOAT, PACK_HALF)
COMPACT = native.OPT_VIEW_COMPACT
WHO = "insitu_view_gather_merged"


def _same_bytes(got, want, what):
    assert got.size == want.size, f"{what}: {got.size} bytes, expected {want.size}"
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, f"{what}: {bad.size} of {want.size} bytes differ, the first at {int(bad[0])}"


def _header(stream):
    """(W, H, S, E) of a packed stream."""
    raw = stream.tobytes()[:32]
    return struct.unpack_from("<3I", raw, 12) + struct.unpack_from("<Q", raw, 24)


def _wire(streams, fmt):
    """The section bytes of the peers' streams: W*H + 8 E + (16 or 8) E each."""
    per = 24 if fmt == PACK_FLOAT else 16
    return sum(w * h + per * e for w, h, _, e in map(_header, streams[1:]))


def _gather(ctxs, fmt=PACK_FLOAT, root_compact=0):
    """The peers first, the root last.  -> the wire bytes of every rank, the root's first."""
    sent = [ctx.view_gather_merged(fmt) for ctx in ctxs[1:]]
    try:
        ctxs[0].set_option(COMPACT, root_compact)
        got = ctxs[0].view_gather_merged(fmt)
    finally:
        ctxs[0].set_option(COMPACT, 0)
    return [got] + sent


def _bind_in(ctx, compact, bind):
    try:
        ctx.set_option(COMPACT, compact)
        bind()
    finally:
        ctx.set_option(COMPACT, 0)


class _World:
    """A local group of `world` ranks over the abutting 2x2 bricks, 4 / world bricks each."""

    def __init__(self, world, w, h):
        self.world, self.w, self.h, self.B = world, w, h, 4 // world
        self.scenes = scene_set("abutting_2x2", w, h)
        self.group = LocalGroup(world)
        self.ctxs = []
        for r in range(world):
            ctx = InSituContext(w, h, max_supersegments=S, bricks_per_rank=self.B, rank=r, nranks=world, local_group=self.group)
            self.ctxs.append(ctx)
            _set_bricks(ctx, self.scenes[self.B * r:self.B * (r + 1)])

    def frame(self, cam):
        """One frame, stage by stage; the sub-VDIs read back in rank order and the loop's merge of them."""
        for stage in ("render", "exchange", "composite"):
            for ctx in self.ctxs:
                getattr(ctx, stage)(*((cam,) if stage == "render" else ()))
        for ctx in self.ctxs[::-1]:
            ctx.gather(want_image=False)
        self.cam, self.cols, self.deps = cam, [], []
        for ctx in self.ctxs:
            c, d = _read_all(ctx, self.B)
            self.cols += c
            self.deps += d
        self.flat = loop_merge_set(self.cols, self.deps)
        self.want = pack_vdi(self.flat[0], self.flat[1], vb.pv_of(cam), PACK_FLOAT)

    def bind(self, layouts=None):
        """Every rank binds INSITU_VIEW_MERGED in its layout.  -> the ranks' FLOAT and HALF streams."""
        for r, ctx in enumerate(self.ctxs):
            _bind_in(ctx, layouts[r] if layouts else 0, lambda: ctx.view_bind(native.VIEW_MERGED))
        return {fmt: [ctx.view_pack(fmt) for ctx in self.ctxs] for fmt in FORMATS}

    def close(self):
        for ctx in self.ctxs:
            ctx.close()
        self.group.close()


def _world(world, w, h, cam):
    g = _World(world, w, h)
    g.frame(cam)
    return g


@pytest.fixture(scope="module")
def two():
    g = _world(2, vb.VDI_W, vb.VDI_H, vb.gen_camera())
    yield g
    g.close()


@pytest.fixture(scope="module")
def four():
    g = _world(4, vb.VDI_W, vb.VDI_H, vb.gen_camera())
    yield g
    g.close()


@pytest.fixture(scope="module")
def ragged():
    g = _world(2, 50, 37, scene.orbit_camera(50, 37, radius=1.4, yaw_deg=30.0, pitch_deg=20.0, voxel_world=1.0 / 32))
    yield g
    g.close()


@pytest.fixture(scope="module")
def other():
    """A context of other dimensions than anything bound into it."""
    with InSituContext(32, 16, max_supersegments=2) as ctx:
        yield ctx


def _one_rank_merged(g):
    """INSITU_VIEW_MERGED of a one-rank context holding all four bricks, as a FLOAT stream."""
    with InSituContext(g.w, g.h, max_supersegments=S, bricks_per_rank=4) as ctx:
        _set_bricks(ctx, g.scenes)
        ctx.frame(g.cam)
        ctx.view_bind(native.VIEW_MERGED)
        return ctx.view_pack(PACK_FLOAT)


def _check_frame_gather(g, other):
    single = _one_rank_merged(g)
    _same_bytes(single, g.want, "the one-rank merged bind against the loop")
    root = g.ctxs[0]
    for root_compact in (0, 1):
        layouts = [root_compact] * g.world
        layouts[1] = 1 - root_compact
        streams = g.bind(layouts)
        assert [ctx.stats()["view_compact"] for ctx in g.ctxs] == layouts
        other.view_bind_packed_set(streams[PACK_FLOAT])
        from_set = other.view_pack(PACK_FLOAT)
        set_stats = other.stats()
        wires = _gather(g.ctxs, PACK_FLOAT, root_compact)
        got = root.view_pack(PACK_FLOAT)
        what = f"{g.world} ranks at {g.w}x{g.h}, root compact {root_compact}"
        _same_bytes(got, g.want, what + ": against the loop over the read-back sub-VDIs")
        _same_bytes(got, single, what + ": against the one-rank context")
        _same_bytes(got, from_set, what + ": against the set bind of the ranks' streams")
        w, h, s, e = _header(g.want)
        st = root.stats()
        assert st["view_slots"] == s == g.flat[0].shape[2] == set_stats["view_slots"]
        assert st["view_overlaps"] == 0 == g.flat[2] and st["view_compact"] == root_compact
        assert st["view_entries"] == e == sum(_header(x)[3] for x in streams[PACK_FLOAT]) == set_stats["view_entries"]
        assert st["view_bytes"] == _layout_bytes(w, h, s, e, root_compact) and st["ms_view_bind"] > 0.0
        assert wires[0] == _wire(streams[PACK_FLOAT], PACK_FLOAT) == sum(wires[1:])
        assert wires[1:] == [w * h + 24 * _header(x)[3] for x in streams[PACK_FLOAT][1:]]
        assert s > S and e > 0


def test_frame_gather_two_ranks(two, other):
    _check_frame_gather(two, other)


def test_frame_gather_four_ranks(four, other):
    _check_frame_gather(four, other)


def test_frame_gather_ragged_window(ragged, other):
    """50x37 on two ranks: 25-pixel strips, partial tiles on both axes and a partial block of 256 pixels."""
    _check_frame_gather(ragged, other)


@pytest.mark.parametrize("name", ["two", "four"])
def test_half(name, request):
    g = request.getfixturevalue(name)
    for root_compact in (0, 1):
        layouts = [root_compact] * g.world
        layouts[-1] = 1 - root_compact
        streams = g.bind(layouts)
        want = merged_stream(streams[PACK_HALF])[0]
        assert not np.array_equal(want, g.want)   # (the rounding shows)
        wires = _gather(g.ctxs, PACK_HALF, root_compact)
        _same_bytes(g.ctxs[0].view_pack(PACK_FLOAT), want, f"HALF, {g.world} ranks, root compact {root_compact}")
        assert wires[0] == _wire(streams[PACK_HALF], PACK_HALF) == sum(wires[1:])
        assert wires[1:] == [g.w * g.h + 16 * _header(x)[3] for x in streams[PACK_HALF][1:]]


def test_renders(two):
    size = vb.OUT_SIZES[1]
    cams = vb.view_cameras()
    two.bind()
    _gather(two.ctxs)
    seen = 0.0
    for name in ("yaw90", "cross"):
        img, acc = two.ctxs[0].view_render(cams[name], *size, want_float=True)
        ref_img, ref_acc = vb.render(two.flat[0], two.flat[1], two.cam, cams[name], *size)
        bad = _bits(acc) != _bits(ref_acc)
        assert not bad.any(), f"{name}: {int(bad.sum())} of {bad.size} accumulator words differ"
        assert np.array_equal(img, ref_img), name
        seen += float(ref_acc[..., 3].sum())
    assert seen > 1.0


def test_peers_untouched(four):
    for fmt in FORMATS:
        before = four.bind([0, 1, 0, 1])[PACK_FLOAT]
        stats = [ctx.stats() for ctx in four.ctxs[1:]]
        _gather(four.ctxs, fmt)
        for r, ctx in enumerate(four.ctxs[1:], 1):
            _same_bytes(ctx.view_pack(PACK_FLOAT), before[r], f"rank {r} after a gather in format {fmt}")
            st = ctx.stats()
            assert all(st[k] == stats[r - 1][k] for k in ("view_slots", "view_entries", "view_bytes", "view_compact", "view_overlaps"))
        assert four.ctxs[0].stats()["view_entries"] == sum(_header(x)[3] for x in before)


def test_repeated_gather():
    first, second = vb.gen_camera(), vb.view_cameras()["yaw20"]
    g = _world(2, vb.VDI_W, vb.VDI_H, first)
    try:
        g.bind()
        _gather(g.ctxs)
        _same_bytes(g.ctxs[0].view_pack(PACK_FLOAT), g.want, "the first frame")
        old = g.want
        g.frame(second)
        assert not np.array_equal(vb.pv_of(first), vb.pv_of(second))
        assert g.want.size != old.size or not np.array_equal(g.want, old)
        g.bind([1, 0])
        _gather(g.ctxs, root_compact=1)
        got = g.ctxs[0].view_pack(PACK_FLOAT)
        _same_bytes(got, g.want, "the second frame: entries and generating camera")
        assert np.array_equal(unpack_vdi(got)[2], vb.pv_of(second))
        # again, the peer as it stands: the root binds its own bricks anew, the peer offers what it holds
        g.ctxs[0].view_bind(native.VIEW_MERGED)
        _gather(g.ctxs)
        _same_bytes(g.ctxs[0].view_pack(PACK_FLOAT), g.want, "gathered twice in a row")
    finally:
        g.close()


# ---------------------------------------------------------------- crafted ranks, bound from host memory
class _HostRanks:
    """A local group of n ranks that render nothing: each binds a 16x8 VDI from host memory."""

    def __init__(self, n):
        self.group = LocalGroup(n)
        self.ctxs = [InSituContext(8 * n, 8, max_supersegments=2, rank=r, nranks=n, local_group=self.group) for r in range(n)]
        self.gen = vb.gen_camera(16, 8)

    def bind(self, vdis, layouts=None):
        """-> the VDIs as FLOAT streams (what every rank's view_pack gives, by tests/test_gpu_view_pack.py)."""
        for r, (ctx, (col, dep)) in enumerate(zip(self.ctxs, vdis)):
            _bind_in(ctx, layouts[r] if layouts else 0, lambda: ctx.view_bind_host(col, dep, self.gen))
        return [pack_vdi(col, dep, vb.pv_of(self.gen), PACK_FLOAT) for col, dep in vdis]

    def close(self):
        for ctx in self.ctxs:
            ctx.close()
        self.group.close()


def _check_crafted(ranks, vdis, what):
    for root_compact in (0, 1):
        layouts = [(r + root_compact) % 2 for r in range(len(vdis))]
        streams = ranks.bind(vdis, layouts)
        want, merged = merged_stream(streams)
        wires = _gather(ranks.ctxs, PACK_FLOAT, root_compact)
        _same_bytes(ranks.ctxs[0].view_pack(PACK_FLOAT), want, f"{what}, root compact {root_compact}")
        st = ranks.ctxs[0].stats()
        assert st["view_slots"] == merged[0].shape[2] and st["view_overlaps"] == merged[2]
        assert st["view_entries"] == _header(want)[3] and st["view_compact"] == root_compact
        assert wires[0] == _wire(streams, PACK_FLOAT)
    return merged


def test_crafted_three_ranks():
    empty = (np.zeros((16, 8, 4, 4), np.float32), np.zeros((16, 8, 8), np.float32))
    ranks = _HostRanks(3)
    try:
        for order in ([random_vdi(16, 8, 2, 71), empty, random_vdi(16, 8, 7, 72)],     # the empty rank is a peer
                      [empty, random_vdi(16, 8, 4, 73), random_vdi(16, 8, 7, 74)]):    # ... is the root
            merged = _check_crafted(ranks, order, "S = 2, 4, 7 with an empty rank")
            assert merged[0].shape[2] > 7
        _check_crafted(ranks, [empty, empty, empty], "only empty ranks")
        assert ranks.ctxs[0].stats()["view_slots"] == 1 and ranks.ctxs[0].stats()["view_entries"] == 0
        # a tie: the lowest rank first
        ties = [unpack_vdi(s)[:2] for s in tie_streams()]
        merged = _check_crafted(ranks, ties, "a tie between ranks 0 and 2")
        assert merged[0][2, 3, :, :2].tolist() == [[0, 0], [2, 0], [1, 0], [2, 1], [0, 1]]
    finally:
        ranks.close()


def test_crafted_nine_ranks():
    cols, deps = vb.random_set(9, 909)
    ranks = _HostRanks(9)
    try:
        merged = _check_crafted(ranks, list(zip(cols, deps)), "nine ranks")
        assert merged[0].shape[2] > 8
    finally:
        ranks.close()


def test_more_than_255_merged_entries():
    vdis = [unpack_vdi(s)[:2] for s in layered_streams(200, 200)]
    ranks = _HostRanks(2)
    try:
        for root_compact in (0, 1):
            before = ranks.bind(vdis)
            assert ranks.ctxs[1].view_gather_merged() == 16 * 8 * (1 + 24 * 200)
            try:
                ranks.ctxs[0].set_option(COMPACT, root_compact)
                rc = ranks.ctxs[0].lib.insitu_view_gather_merged(ranks.ctxs[0].h, PACK_FLOAT, None)
            finally:
                ranks.ctxs[0].set_option(COMPACT, 0)
            _fails(ranks.ctxs[0], rc, "400 entries per pixel, at most 255")
            _nothing_bound(ranks.ctxs[0])
            _same_bytes(ranks.ctxs[1].view_pack(PACK_FLOAT), before[1], "the peer is still bound")
        # 128 + 127 is the most
        streams = ranks.bind([unpack_vdi(s)[:2] for s in layered_streams(128, 127)])
        _gather(ranks.ctxs)
        _same_bytes(ranks.ctxs[0].view_pack(PACK_FLOAT), merged_stream(streams)[0], "128 + 127 entries")
        assert ranks.ctxs[0].stats()["view_slots"] == 255
    finally:
        ranks.close()


# ---------------------------------------------------------------- rejections
def _raw(ctx, fmt=PACK_FLOAT):
    return ctx.lib.insitu_view_gather_merged(ctx.h, fmt, None)


def test_rejections(two):
    root, peer = two.ctxs
    G = two.cam

    def good(what):
        two.bind()
        _gather(two.ctxs)
        _same_bytes(root.view_pack(PACK_FLOAT), two.want, what)

    def rejected(*texts):
        _fails(root, _raw(root), WHO)
        for text in texts:
            _fails(root, -1, text)
        _nothing_bound(root)

    good("before any rejection")
    # a peer with nothing bound (a failed bind leaves none)
    two.bind()
    assert peer.lib.insitu_view_bind(peer.h, 99, 0) == -1
    assert _raw(peer) == 0   # (in a local group a rejection is the root's to see)
    rejected("rank 1 rejected", "no VDI bound")
    good("after a peer with nothing bound")
    # the root itself
    two.bind()
    assert root.lib.insitu_view_bind(root.h, 99, 0) == -1
    assert _raw(peer) == 0
    rejected("rank 0 rejected", "no VDI bound")
    good("after a root with nothing bound")
    # a peer of another window
    two.bind()
    peer.view_bind_host(*random_vdi(50, 37, 3, 5), G)
    assert _raw(peer) == 0
    rejected("rank 1 rejected", "W and H differ")
    good("after a peer of another window")
    # a peer of another generating camera
    two.bind()
    peer.view_bind_host(*random_vdi(vb.VDI_W, vb.VDI_H, 3, 6), vb.view_cameras()["yaw20"])
    assert _raw(peer) == 0
    rejected("rank 1 rejected", "generating camera differs")
    good("after a peer of another camera")
    # a bad format, on the peer and on the root
    two.bind()
    assert _raw(peer, 2) == 0
    rejected("rank 1 rejected", "bad format")
    two.bind()
    assert _raw(peer) == 0
    _fails(root, _raw(root, 2), "rank 0 rejected")
    _fails(root, -1, "bad format")
    _nothing_bound(root)
    good("after a bad format")
    # the root before its peer: nothing is offered (the rejections above consumed what was)
    two.bind()
    rejected("local group rank 1 has not offered")
    good("after a root that called first")
    # an offer withdrawn by a pack, and by a bind
    for again in (lambda: peer.view_pack(PACK_HALF), lambda: peer.view_bind(native.VIEW_MERGED)):
        two.bind()
        assert _raw(peer) == 0
        again()
        rejected("local group rank 1 has bound or packed since its offer")
        good("after a withdrawn offer")


def test_one_rank(other):
    scenes = scene_set("abutting_2x2")
    with InSituContext(vb.VDI_W, vb.VDI_H, max_supersegments=S, bricks_per_rank=4) as ctx:
        _set_bricks(ctx, scenes)
        ctx.frame(vb.gen_camera())
        for fmt in FORMATS:
            for compact in (0, 1):
                ctx.view_bind(native.VIEW_MERGED)
                stream = ctx.view_pack(fmt)
                _bind_in(other, compact, lambda: other.view_bind_packed(stream))
                want = {f: other.view_pack(f) for f in FORMATS}
                want_stats = other.stats()
                assert _gather([ctx], fmt, compact) == [0]
                for f in FORMATS:
                    _same_bytes(ctx.view_pack(f), want[f], f"one rank, format {fmt} read as {f}, compact {compact}")
                st = ctx.stats()
                assert all(st[k] == want_stats[k] for k in ("view_slots", "view_entries", "view_bytes", "view_compact", "view_overlaps"))
                assert st["view_compact"] == compact and st["view_slots"] == 13
        # with nothing bound, and with a bad format
        assert ctx.lib.insitu_view_bind(ctx.h, 99, 0) == -1
        _fails(ctx, _raw(ctx), "rank 0 rejected: no VDI bound")
        ctx.view_bind(native.VIEW_MERGED)
        _fails(ctx, _raw(ctx, 7), "rank 0 rejected: bad format")
        _nothing_bound(ctx)
    # one rank has no communicator to keep free: legal with a pipelined frame in flight
    with InSituContext(vb.VDI_W, vb.VDI_H, max_supersegments=S, bricks_per_rank=4) as ctx:
        _set_bricks(ctx, scenes)
        assert ctx.frame_pipelined(vb.gen_camera())[0] == -1
        ctx.view_bind_packed(stream)
        assert ctx.view_gather_merged(PACK_FLOAT) == 0
        _same_bytes(ctx.view_pack(fmt), want[fmt], "with a frame in flight")
        assert ctx.pipeline_flush()[0] == 0


# ---------------------------------------------------------------- RCCL, one rank per process
def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _run_worker(world, size, *mode):
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", OMP_NUM_THREADS="2", NCCL_DEBUG="WARN")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={world}",
           "--master-addr=127.0.0.1", f"--master-port={_free_port()}", str(ROOT / "tests" / "view_gather_worker.py"),
           str(size[0]), str(size[1]), *mode]
    p = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=280)
    assert p.returncode == 0 and "GATHER_OK" in p.stdout, p.stdout[-6000:] + "\n--- stderr ---\n" + p.stderr[:6000]
    return p.stdout + p.stderr


@pytest.mark.timeout(300)
@pytest.mark.parametrize("world, size", [(2, (50, 37)), (4, (64, 48))])
def test_rccl(world, size):
    out = _run_worker(world, size)
    for case in ("frame FLOAT", "frame HALF", "crafted", "rejection", "after the rejection"):
        assert f"[gather] {case}: True" in out, (case, out[-4000:])


@pytest.mark.timeout(300)
def test_rccl_frame_in_flight():
    """With nranks > 1 a rank that has a pipelined frame in flight refuses (in a local group there is no such frame)."""
    out = _run_worker(2, (vb.VDI_W, vb.VDI_H), "inflight")
    for case in ("frame in flight", "after the flush"):
        assert f"[gather] {case}: True" in out, (case, out[-4000:])
