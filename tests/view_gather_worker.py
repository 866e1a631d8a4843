"""One rank of the multi-process check of insitu_view_gather_merged over RCCL (launched by
tests/test_gpu_view_gather.py through torch.distributed.run; test infrastructure, in the manner of
tests/rccl_worker.py).

Arguments W H [inflight]: the window, and which cases run.  The 2x2 abutting bricks are split over the ranks; every rank renders a frame, binds
INSITU_VIEW_MERGED and the ranks gather on rank 0.  Rank 0 compares the root's VDI, read back
as a FLOAT stream, with a one-rank context that renders every brick itself and with insitu_view_bind_packed_set of the
ranks' view_pack streams, which travel over gloo:
  frame FLOAT / frame HALF : the frame-based gather in both formats (HALF: the root compact, rank 1 in the other layout)
  crafted                  : 16x8 VDIs bound from host memory, S differing from rank to rank, rank 1 empty
  rejection                : rank 1 has nothing bound: every rank returns -1 and names rank 1
  after the rejection      : the next gather on the same communicator succeeds -- no rank was left waiting
With `inflight` (a run of its own: in a local group no frame can be in flight):
  frame in flight          : a pipelined frame in flight on every rank: every rank returns -1 and names rank 0
  after the flush          : insitu_pipeline_flush, then the gather on the same communicator succeeds
The exit status is the ranks' verdict; nothing is retried.  When the ranks outnumber the GPUs they share one (distinct
NCCL host ids, RCCL's socket transport), as in tests/rccl_worker.py.
"""
import ctypes
import os
import struct
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT / "scenery-insitu_amd"), str(ROOT / "tests")]
rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])

import torch  # noqa: E402

if torch.cuda.device_count() < world:   # before any RCCL call (RCCL reads these at its first init)
    os.environ["NCCL_HOSTID"] = f"insitu-rank-{rank}"
    os.environ.setdefault("NCCL_SOCKET_IFNAME", "lo")
    os.environ.setdefault("NCCL_IB_DISABLE", "1")

import numpy as np  # noqa: E402
import torch.distributed as dist  # noqa: E402

import view_binding as vb  # noqa: E402
from insitu_amd import native  # noqa: E402
from insitu_amd.renderer import InSituContext  # noqa: E402
from insitu_amd.vdi_io import PACK_FLOAT, PACK_HALF, pack_vdi  # noqa: E402
from test_pack_set import merged_stream  # noqa: E402
from test_vdi_pack import random_vdi  # noqa: E402
from test_view_merge import scene_set  # noqa: E402

dev = int(os.environ.get("LOCAL_RANK", "0")) % max(1, torch.cuda.device_count())
torch.cuda.set_device(dev)
dist.init_process_group("gloo")
W, H = int(sys.argv[1]), int(sys.argv[2])
INFLIGHT = sys.argv[3:4] == ["inflight"]
S = vb.VDI_S
B = 4 // world
COMPACT = native.OPT_VIEW_COMPACT
scenes = scene_set("abutting_2x2", W, H)
cam = vb.gen_camera(W, H)
gen = vb.gen_camera(16, 8)


def comm_id() -> bytes:
    """A fresh ncclUniqueId for every communicator (an id serves one ncclCommInitRank)."""
    buf = torch.zeros(native.COMM_ID_BYTES, dtype=torch.uint8)
    if rank == 0:
        raw = ctypes.create_string_buffer(native.COMM_ID_BYTES)
        native.check(native.load().insitu_comm_id(raw, native.COMM_ID_BYTES))
        buf = torch.frombuffer(bytearray(raw.raw), dtype=torch.uint8).clone()
    dist.broadcast(buf, 0)
    return bytes(buf.numpy().tobytes())


def everyone(value):
    out = [None] * world
    dist.all_gather_object(out, value)
    return out


def same(a, b):
    return a.size == b.size and bool(np.array_equal(a, b))


def entries(stream):
    return struct.unpack_from("<Q", stream.tobytes()[:32], 24)[0]


def bind_in(ctx, compact, bind):
    try:
        ctx.set_option(COMPACT, compact)
        bind()
    finally:
        ctx.set_option(COMPACT, 0)


def gather(ctx, fmt, compact=0):
    """-> (return code, wire bytes, the last error)"""
    wire = ctypes.c_ulonglong(0)
    try:
        ctx.set_option(COMPACT, compact)
        rc = ctx.lib.insitu_view_gather_merged(ctx.h, fmt, ctypes.byref(wire))
    finally:
        ctx.set_option(COMPACT, 0)
    return rc, int(wire.value), ctx.lib.insitu_last_error(ctx.h).decode()


def nothing_bound(ctx):
    return ctx.lib.insitu_view_pack_bytes(ctx.h, PACK_FLOAT) == 0 and "no VDI bound" in ctx.lib.insitu_last_error(ctx.h).decode()


def set_bind(streams):
    """insitu_view_bind_packed_set of the streams in a context of its own, read back as a FLOAT stream."""
    with InSituContext(32, 16, max_supersegments=2, device=dev) as ref:
        ref.view_bind_packed_set(streams)
        return ref.view_pack(PACK_FLOAT)


def crafted_vdi(r):
    s = 2 + 2 * r
    if r == 1:
        return np.zeros((16, 8, s, 4), np.float32), np.zeros((16, 8, 2 * s), np.float32)
    return random_vdi(16, 8, s, 300 + r)


def crafted_case(ctx, what):
    """Every rank binds its crafted VDI and the ranks gather: the root holds the loop's merge of them all."""
    bind_in(ctx, rank % 2, lambda: ctx.view_bind_host(*crafted_vdi(rank), gen))
    mine = ctx.view_pack(PACK_FLOAT)
    trace(what + ": bound")
    rc, wire, err = gather(ctx, PACK_FLOAT, 1)
    trace(what + f": gathered, rc {rc}")
    ok = rc == 0 and (rank == 0 or (wire == 16 * 8 + 24 * entries(mine) and same(ctx.view_pack(PACK_FLOAT), mine)))
    if rank == 0:
        streams = [pack_vdi(*crafted_vdi(r), vb.pv_of(gen), PACK_FLOAT) for r in range(world)]
        want, merged = merged_stream(streams)
        ok = ok and same(ctx.view_pack(PACK_FLOAT), want) and same(set_bind(streams), want)
        ok = ok and wire == sum(16 * 8 + 24 * entries(s) for s in streams[1:]) and entries(want) > 0 and merged[0].shape[2] >= 2
        ok = ok and ctx.stats()["view_compact"] == 1 and ctx.stats()["view_entries"] == entries(want)
    if not ok:
        print(f"[gather] rank {rank}, {what}: rc {rc}, wire {wire}, '{err}'", flush=True)
    return ok


def trace(what):
    if os.environ.get("GATHER_WORKER_TRACE"):
        print(f"[trace] rank {rank}: {what}", flush=True)


def main_cases():
    results = {}
    ctx = InSituContext(W, H, max_supersegments=S, bricks_per_rank=B, rank=rank, nranks=world, device=dev, comm_id=comm_id())
    vb.set_bricks(ctx, scenes[B * rank:B * (rank + 1)])
    ctx.frame(cam)
    trace("frame rendered")
    single = None
    if rank == 0:
        with InSituContext(W, H, max_supersegments=S, bricks_per_rank=4, device=dev) as ref:
            vb.set_bricks(ref, scenes)
            ref.frame(cam)
            ref.view_bind(native.VIEW_MERGED)
            single = ref.view_pack(PACK_FLOAT)
    for fmt, name in ((PACK_FLOAT, "frame FLOAT"), (PACK_HALF, "frame HALF")):
        root_compact = 1 if fmt == PACK_HALF else 0
        bind_in(ctx, (root_compact + rank) % 2, lambda: ctx.view_bind(native.VIEW_MERGED))
        mine = ctx.view_pack(fmt)
        before = ctx.view_pack(PACK_FLOAT)
        streams = everyone(mine)
        trace(name + ": bound and packed")
        rc, wire, err = gather(ctx, fmt, root_compact)
        trace(name + f": gathered, rc {rc}")
        per = 24 if fmt == PACK_FLOAT else 16
        ok = rc == 0
        if rank == 0:
            got = ctx.view_pack(PACK_FLOAT)
            ok = ok and same(got, set_bind(streams)) and same(got, merged_stream(streams)[0])
            if fmt == PACK_FLOAT:
                ok = ok and same(got, single)
            ok = ok and wire == sum(W * H + per * entries(s) for s in streams[1:])
            st = ctx.stats()
            ok = ok and st["view_compact"] == root_compact and st["view_entries"] == sum(entries(s) for s in streams) > 0
        else:
            ok = ok and wire == W * H + per * entries(mine) and same(ctx.view_pack(PACK_FLOAT), before)
        if not ok:
            print(f"[gather] rank {rank}, {name}: rc {rc}, wire {wire}, '{err}'", flush=True)
        results[name] = ok

    results["crafted"] = crafted_case(ctx, "crafted")

    # rank 1 has nothing bound (a failed bind leaves none): every rank learns it
    if rank == 1:
        assert ctx.lib.insitu_view_bind(ctx.h, 99, 0) == -1
    mine = ctx.view_pack(PACK_FLOAT) if rank > 1 else None
    rc, wire, err = gather(ctx, PACK_FLOAT)
    ok = rc == -1 and wire == 0 and "insitu_view_gather_merged: rank 1 rejected: no VDI bound" in err
    if rank == 0:
        ok = ok and nothing_bound(ctx)
    elif rank > 1:
        ok = ok and same(ctx.view_pack(PACK_FLOAT), mine)
    if not ok:
        print(f"[gather] rank {rank}, rejection: rc {rc}, wire {wire}, '{err}'", flush=True)
    results["rejection"] = ok
    trace("rejection done")
    results["after the rejection"] = crafted_case(ctx, "after the rejection")
    ctx.close()
    return results


def inflight_cases():
    """A pipelined frame in flight on every rank: the gather is refused, and works after the flush."""
    results = {}
    ctx = InSituContext(W, H, max_supersegments=S, bricks_per_rank=B, rank=rank, nranks=world, device=dev, comm_id=comm_id())
    vb.set_bricks(ctx, scenes[B * rank:B * (rank + 1)])
    assert ctx.frame_pipelined(cam)[0] == -1
    ctx.view_bind_host(*crafted_vdi(rank), gen)
    mine = ctx.view_pack(PACK_FLOAT)
    trace("frame in flight, bound")
    rc, wire, err = gather(ctx, PACK_FLOAT)
    ok = rc == -1 and "insitu_view_gather_merged: rank 0 rejected: a pipelined frame is in flight" in err
    ok = ok and (nothing_bound(ctx) if rank == 0 else same(ctx.view_pack(PACK_FLOAT), mine))
    if not ok:
        print(f"[gather] rank {rank}, frame in flight: rc {rc}, wire {wire}, '{err}'", flush=True)
    results["frame in flight"] = ok
    trace("refused")
    assert ctx.pipeline_flush()[0] == 0
    trace("flushed")
    results["after the flush"] = crafted_case(ctx, "after the flush")
    ctx.close()
    return results


results = inflight_cases() if INFLIGHT else main_cases()
verdicts = everyone(results)
failures = sorted({name for v in verdicts for name, ok in v.items() if not ok})
if rank == 0:
    for name in results:
        print(f"[gather] {name}: {all(v[name] for v in verdicts)}", flush=True)
    print("GATHER_OK" if not failures else f"GATHER_FAILED {failures}", flush=True)
dist.barrier()
dist.destroy_process_group()
sys.exit(1 if failures else 0)
