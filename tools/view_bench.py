#!/usr/bin/env python3
"""Timing of the novel-view renderer (insitu_view_render) on the benchmark's scene.

The scene is config 2 of bench.py on one GPU: 8 Gray-Scott bricks of 512^3 rendered at 1920x1080 with S = 20 and
composited by the VDICompositor into a VDI of S_out = 20, gathered on the root.  That VDI is bound
(INSITU_VIEW_GATHERED) and viewed from 36 cameras on the orbit the frame's camera lies on (10 degrees apart, the first
one the generating camera) at 1920x1080.  Every view's kernel is timed by HIP events (insitu_stats.ms_view); after a
warm-up pass over the orbit per setting, the passes alternate between the empty-tile skip on and off.

The work of a view -- cells visited, list entries examined (24 bytes each: depth pair + colour), entries blended --
is counted by the CPU restatement (tests/view_ref) for a few of the views (--count-views; slow), and gives the
kernel's entry traffic in GB/s against the HBM peak.  Prints one JSON line.

--pack: after the bind, the bound VDI is packed (insitu_view_pack) in both formats and bound
back (insitu_view_bind_packed): the stream sizes, the kernels' HIP-event time of the pack and of the unpack
(insitu_stats.ms_pack) and the wall time of insitu_view_pack with its copy to the host, one warm-up and then the
best of three each, go into the JSON under "pack", beside the size of the dense readback they replace.

--merged: the whole scene without the compositor's loss.  Config 2 in the default (flatten)
context, all eight sub-VDIs bound with INSITU_VIEW_MERGED: the slots S_m, the stored entries, the overlap count, the
bind's kernels (insitu_stats.ms_view_bind, best of three binds), the FLOAT and HALF packed sizes, and ms per view over
the same orbit (skip on).  Then, in the same process, the same bricks in a composite_vdi context and the orbit over its
gathered VDI; per camera the largest and the mean absolute difference of the two rgba8 images, in LSB -- what the
VDICompositor's re-supersegmentation to S_out entries costs a novel view.  Prints one JSON line and nothing else runs.

--compact: every measurement is also taken with INSITU_OPT_VIEW_COMPACT = 1, the same VDI
bound again in the compact view layout: the layout's device bytes (insitu_stats.view_bytes) and the bind's kernels,
the orbit with its passes alternating between the two layouts, with --pack the pack and bind-packed times, with
--merged the merged bind and its orbit.  The compact figures stand beside the dense ones in the JSON.

--packed-set: the whole scene from packed streams.  Config 2 in the default context; each of
the eight sub-VDIs is bound (INSITU_VIEW_BRICK) and packed, FLOAT and HALF; the set is bound with
insitu_view_bind_packed_set, dense and with --compact also compact, and the FLOAT pack of the result must equal the
FLOAT pack of INSITU_VIEW_MERGED of the same frame byte for byte (the HALF set: the HALF packs).  Beside it today's
path, insitu_view_bind_host_set of the same eight sub-VDIs read back dense: for both the bytes uploaded, the device
bytes staged, ms_view_bind and the wall time of the call, one warm-up and the best of three.  Prints one JSON line and
nothing else runs.

--gather-merged: the whole scene on rank 0 without the host.  Config 2 as a local group of 8
one-brick ranks on this one GPU; every rank binds its sub-VDI and insitu_view_gather_merged gathers them on rank 0, in
both formats: the call's wall time on the root (the peers' calls, which pack and offer, beside it), ms_view_bind and
the wire bytes -- on one GPU the "wire" is a device-to-device copy; over xGMI it is unmeasured.  For comparison the
same frame through the host: insitu_view_pack on every rank and insitu_view_bind_packed_set on rank 0.  The FLOAT pack
of both results must be equal byte for byte.  Prints one JSON line and nothing else runs.

usage: python tools/view_bench.py [--brick 512] [--sim-n 512] [--views 36] [--passes 3] [--count-views 2] [--pack] [--compact]
       python tools/view_bench.py --merged [--compact] [--brick 512] [--sim-n 512] [--views 36] [--passes 2]
       python tools/view_bench.py --packed-set [--compact] [--brick 512] [--sim-n 512]
       python tools/view_bench.py --gather-merged [--compact] [--brick 512] [--sim-n 512]
"""
from __future__ import annotations

import argparse
import json
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
for _p in (ROOT / "scenery-insitu_amd", ROOT / "tests", ROOT):
    if str(_p) not in sys.path:
        sys.path.insert(0, str(_p))

import numpy as np  # noqa: E402
import torch  # noqa: E402

W_IMG, H_IMG, S = 1920, 1080, 20
HBM_PEAK_GBS = 8000.0   # MI355X HBM3E, spec
ENTRY_BYTES = 24        # {start, end} depth + rgba colour of one list entry


def log(*a):
    print(*a, file=sys.stderr, flush=True)


def run_merged(args):
    from insitu_amd import native, scene
    from insitu_amd.renderer import InSituContext
    from insitu_amd.vdi_io import PACK_HEADER_BYTES

    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    n = args.brick
    bricks = scene.grid_bricks(n * 2, 2)
    t0 = time.perf_counter()
    flat = InSituContext(W_IMG, H_IMG, max_supersegments=S, bricks_per_rank=len(bricks), keep_passes=False)
    comp = InSituContext(W_IMG, H_IMG, max_supersegments=S, bricks_per_rank=len(bricks), composite_vdi=True,
                         max_output_supersegments=S, keep_passes=False)
    for ctx in (flat, comp):
        ctx.set_transfer(scene.transfer_function(), scene.colormap_hot(), conv_scale=1.0 / 0.5, conv_offset=0.0)
    for bid, (origin, vw, _) in enumerate(bricks):
        v = scene.gray_scott(n, steps=1500, seed=1000 + bid, device=dev, sim_n=min(args.sim_n, n)).contiguous()
        for ctx in (flat, comp):
            ctx.set_brick(bid, v, scene.brick_model(origin, vw), dtype=native.F32)
        del v
    vw = bricks[0][1]
    torch.cuda.synchronize()
    log(f"view_bench: {len(bricks)} bricks of {n}^3 in two contexts in {time.perf_counter() - t0:.1f} s")
    cams = [scene.orbit_camera(W_IMG, H_IMG, yaw_deg=30.0 + 360.0 / args.views * i, pitch_deg=20.0, voxel_world=vw)
            for i in range(args.views)]
    ow, oh = args.out_w, args.out_h

    def orbit(ctx, layouts=(None,), source=None):
        """Per layout (None: as bound; 0 / 1: `source` bound again dense / compact before each of its passes, so
        the layouts alternate): (best ms per camera over the timed passes after one warm-up pass, the images)"""
        ms, imgs = {lay: [] for lay in layouts}, {}
        for k in range(args.passes + 1):
            for lay in layouts:
                if lay is not None:
                    ctx.set_option(native.OPT_VIEW_COMPACT, lay)
                    ctx.view_bind(source)
                row, imgs[lay] = [], []
                for cam in cams:
                    imgs[lay].append(ctx.view_render(cam, ow, oh))
                    row.append(ctx.stats()["ms_view"])
                if k:
                    ms[lay].append(row)
        return {lay: (np.asarray(ms[lay]).min(axis=0), imgs[lay]) for lay in layouts}

    def bind_merged(layout):
        flat.set_option(native.OPT_VIEW_COMPACT, layout)
        ms_bind, wall_bind = [], []
        for _ in range(4):   # one warm-up (it allocates), then the best of three
            t0 = time.perf_counter()
            flat.view_bind(native.VIEW_MERGED)
            wall_bind.append((time.perf_counter() - t0) * 1e3)
            ms_bind.append(flat.stats()["ms_view_bind"])
        st = flat.stats()
        return {"view_slots": int(st["view_slots"]), "entries": int(st["view_entries"]), "view_overlaps": int(st["view_overlaps"]),
                "ms_view_bind": min(ms_bind[1:]), "ms_view_bind_first": ms_bind[0], "ms_bind_wall": min(wall_bind[1:]),
                "view_layout_bytes": int(st["view_bytes"]), "view_compact": int(st["view_compact"])}

    flat.frame(cams[0])
    merged = bind_merged(0)
    px16 = (W_IMG * H_IMG + 15) // 16 * 16
    sizes = {name: int(flat.lib.insitu_view_pack_bytes(flat.h, fmt))
             for name, fmt in (("float", native.PACK_FLOAT), ("half", native.PACK_HALF))}
    assert merged["entries"] == (sizes["float"] - PACK_HEADER_BYTES - px16) // ENTRY_BYTES
    merged.update({"packed_bytes": sizes, "slots_if_sized_by_n_times_S": len(bricks) * S})
    log(f"view_bench: merged bind {json.dumps(merged)}")
    compact = None
    if args.compact:
        compact = bind_merged(1)
        log(f"view_bench: compact merged bind {json.dumps(compact)}")
        runs = orbit(flat, (0, 1), native.VIEW_MERGED)
        ms_m, img_m = runs[0]
        ms_c, img_c = runs[1]
        assert all(np.array_equal(a, b) for a, b in zip(img_m, img_c)), "compact and dense images differ"
        compact.update({"ms_per_view": float(ms_c.mean()), "ms_min_max": [float(ms_c.min()), float(ms_c.max())],
                        "ms_by_view": [round(float(v), 4) for v in ms_c]})
        flat.set_option(native.OPT_VIEW_COMPACT, 0)
    else:
        ms_m, img_m = orbit(flat)[None]
    flat.close()

    comp.frame(cams[0])
    comp.view_bind(native.VIEW_GATHERED)
    g_entries = (int(comp.lib.insitu_view_pack_bytes(comp.h, native.PACK_FLOAT)) - PACK_HEADER_BYTES - px16) // ENTRY_BYTES
    ms_g, img_g = orbit(comp)[None]
    comp.close()
    lsb_max, lsb_mean = [], []
    for a, b in zip(img_m, img_g):
        d = np.abs(a.astype(np.int16) - b.astype(np.int16))
        lsb_max.append(int(d.max()))
        lsb_mean.append(round(float(d.mean()), 4))
    res = {
        "metric": f"INSITU_VIEW_MERGED against INSITU_VIEW_GATHERED, novel views @{ow}x{oh} of config 2 "
                  f"({W_IMG}x{H_IMG}, S = S_out = {S}, 8x{n}^3 volume)",
        "views": args.views, "passes": args.passes,
        "merged": merged, "gathered": {"view_slots": S, "entries": int(g_entries)},
        "merged_compact": compact,   # --compact: the same bind and orbit in the compact layout, alternating with dense
        "ms_per_view": {"merged": float(ms_m.mean()), "gathered": float(ms_g.mean())},
        "ms_min_max": {"merged": [float(ms_m.min()), float(ms_m.max())], "gathered": [float(ms_g.min()), float(ms_g.max())]},
        "ms_by_view_merged": [round(float(v), 4) for v in ms_m],
        "ms_by_view_gathered": [round(float(v), 4) for v in ms_g],
        "lsb_max_by_view": lsb_max, "lsb_mean_by_view": lsb_mean,
        "lsb_max": max(lsb_max), "lsb_mean": float(np.mean(lsb_mean)),
        "timing": "HIP events around the kernels (insitu_stats.ms_view, ms_view_bind), best of the passes per camera, "
                  "skip on",
    }
    print(json.dumps(res))


def run_packed_set(args):
    """--packed-set: the eight sub-VDIs of config 2 as packed streams, bound as one merged VDI."""
    from insitu_amd import native, scene
    from insitu_amd.renderer import InSituContext

    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    n = args.brick
    bricks = scene.grid_bricks(n * 2, 2)
    nb = len(bricks)
    t0 = time.perf_counter()
    ctx = InSituContext(W_IMG, H_IMG, max_supersegments=S, bricks_per_rank=nb, keep_passes=False)
    ctx.set_transfer(scene.transfer_function(), scene.colormap_hot(), conv_scale=1.0 / 0.5, conv_offset=0.0)
    for bid, (origin, vw, _) in enumerate(bricks):
        v = scene.gray_scott(n, steps=1500, seed=1000 + bid, device=dev, sim_n=min(args.sim_n, n)).contiguous()
        ctx.set_brick(bid, v, scene.brick_model(origin, vw), dtype=native.F32)
        del v
    cam = scene.orbit_camera(W_IMG, H_IMG, yaw_deg=30.0, pitch_deg=20.0, voxel_world=bricks[0][1])
    ctx.frame(cam)
    torch.cuda.synchronize()
    log(f"view_bench: {nb} bricks of {n}^3 and their frame in {time.perf_counter() - t0:.1f} s")
    streams = {"float": [], "half": []}
    for b in range(nb):
        ctx.view_bind(native.VIEW_BRICK, b)
        streams["float"].append(ctx.view_pack(native.PACK_FLOAT))
        streams["half"].append(ctx.view_pack(native.PACK_HALF))
    ctx.view_bind(native.VIEW_MERGED)
    merged_float = ctx.view_pack(native.PACK_FLOAT)
    merged_half = ctx.view_pack(native.PACK_HALF)
    px16 = (W_IMG * H_IMG + 15) // 16 * 16

    def timed(bind):
        """one warm-up (it allocates), then the best of three: the bind's kernels and the call's wall time"""
        ms, wall = [], []
        for _ in range(4):
            t0 = time.perf_counter()
            bind()
            wall.append((time.perf_counter() - t0) * 1e3)
            ms.append(ctx.stats()["ms_view_bind"])
        st = ctx.stats()
        return {"ms_view_bind": min(ms[1:]), "ms_view_bind_first": ms[0], "ms_wall": min(wall[1:]), "ms_wall_first": wall[0],
                "view_slots": int(st["view_slots"]), "view_entries": int(st["view_entries"]),
                "view_overlaps": int(st["view_overlaps"]), "view_layout_bytes": int(st["view_bytes"])}

    layouts = {"dense": 0, "compact": 1} if args.compact else {"dense": 0}
    res = {"metric": f"insitu_view_bind_packed_set of the {nb} sub-VDIs of config 2 ({W_IMG}x{H_IMG}, S = {S}, {nb}x{n}^3 "
                     f"volume) against insitu_view_bind_host_set of the same sub-VDIs read back dense",
           "timing": "one warm-up, then the best of three per bind; ms_view_bind: HIP events around the bind's kernels, "
                     "ms_wall: the call with its uploads", "packed_set": {}, "host_set": {}}
    for lname, layout in layouts.items():
        ctx.set_option(native.OPT_VIEW_COMPACT, layout)
        for fname, fmt_streams in streams.items():
            r = timed(lambda: ctx.view_bind_packed_set(fmt_streams))
            up = sum(int(s.size) for s in fmt_streams)
            # staged: every stream without its header, sections padded to 16 bytes (csrc/vdi_pack_format.h
            # pack_set_stage); index: the streams' own boff, bstat and loc, their totals and the table
            r["bytes_uploaded"] = up
            ents = [(int(s.size) - 128 - px16) // (ENTRY_BYTES if fname == "float" else 16) for s in fmt_streams]
            r["device_bytes_staged"] = sum(px16 + (8 * e + 15) // 16 * 16 + ((16 if fname == "float" else 8) * e + 15) // 16 * 16
                                           for e in ents)
            r["device_bytes_index"] = nb * (W_IMG * H_IMG * 2 + (W_IMG * H_IMG + 255) // 256 * 12 + 16 + 80)
            got = ctx.view_pack(native.PACK_FLOAT)
            if fname == "float":
                assert np.array_equal(got, merged_float), "the set bind differs from INSITU_VIEW_MERGED of the same frame"
            else:   # the HALF streams' merge, repacked as HALF, is the HALF pack of the merged bind
                assert np.array_equal(ctx.view_pack(native.PACK_HALF), merged_half), "HALF set bind differs"
            del got
            res["packed_set"][f"{lname}_{fname}"] = r
            log(f"view_bench: packed set {lname} {fname} {json.dumps(r)}")
    del merged_half
    # today's path: the same sub-VDIs read back dense and bound through insitu_view_bind_host_set
    cols = [ctx.read(native.BUF_VDI_COLOR, b) for b in range(nb)]
    deps = [ctx.read(native.BUF_VDI_DEPTH, b) for b in range(nb)]
    for lname, layout in layouts.items():
        ctx.set_option(native.OPT_VIEW_COMPACT, layout)
        r = timed(lambda: ctx.view_bind_host_set(cols, deps, cam))
        r["bytes_uploaded"] = r["device_bytes_staged"] = sum(int(c.nbytes) + int(d.nbytes) for c, d in zip(cols, deps))
        r["device_bytes_index"] = 0
        assert np.array_equal(ctx.view_pack(native.PACK_FLOAT), merged_float), "the host set differs from INSITU_VIEW_MERGED"
        res["host_set"][lname] = r
        log(f"view_bench: host set {lname} {json.dumps(r)}")
    res["merged_packed_bytes"] = int(merged_float.size)
    res["merged_entries"] = (int(merged_float.size) - 128 - px16) // ENTRY_BYTES
    ctx.set_option(native.OPT_VIEW_COMPACT, 0)
    ctx.close()
    print(json.dumps(res))


def run_gather_merged(args):
    """--gather-merged: config 2 as 8 one-brick ranks of a local group, gathered on rank 0 device to device."""
    from insitu_amd import native, scene
    from insitu_amd.renderer import InSituContext, LocalGroup

    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    n = args.brick
    bricks = scene.grid_bricks(n * 2, 2)
    nr = len(bricks)
    t0 = time.perf_counter()
    group = LocalGroup(nr)
    ctxs = []
    for r, (origin, vw, _) in enumerate(bricks):
        ctx = InSituContext(W_IMG, H_IMG, max_supersegments=S, bricks_per_rank=1, rank=r, nranks=nr, local_group=group,
                            keep_passes=False)
        ctx.set_transfer(scene.transfer_function(), scene.colormap_hot(), conv_scale=1.0 / 0.5, conv_offset=0.0)
        v = scene.gray_scott(n, steps=1500, seed=1000 + r, device=dev, sim_n=min(args.sim_n, n)).contiguous()
        ctx.set_brick(0, v, scene.brick_model(origin, vw), dtype=native.F32)
        del v
        ctxs.append(ctx)
    cam = scene.orbit_camera(W_IMG, H_IMG, yaw_deg=30.0, pitch_deg=20.0, voxel_world=bricks[0][1])
    for stage in ("render", "exchange", "composite"):
        for ctx in ctxs:
            getattr(ctx, stage)(*((cam,) if stage == "render" else ()))
    for ctx in ctxs[::-1]:
        ctx.gather(want_image=False)
    torch.cuda.synchronize()
    log(f"view_bench: {nr} ranks of one {n}^3 brick and their frame in {time.perf_counter() - t0:.1f} s")
    root = ctxs[0]
    formats = (("float", native.PACK_FLOAT), ("half", native.PACK_HALF))
    layouts = {"dense": 0, "compact": 1} if args.compact else {"dense": 0}
    res = {"metric": f"insitu_view_gather_merged of config 2 ({W_IMG}x{H_IMG}, S = {S}, {nr}x{n}^3 volume) as a local group of "
                     f"{nr} one-brick ranks on one GPU, against insitu_view_pack on every rank + insitu_view_bind_packed_set",
           "timing": "one warm-up, then the best of three; ms_view_bind: HIP events around the root's bind kernels; wall: the "
                     "calls as the host sees them.  One GPU: the wire is a device-to-device copy; xGMI is unmeasured",
           "gather_merged": {}, "through_the_host": {}}
    for lname, layout in layouts.items():
        for ctx in ctxs:
            ctx.set_option(native.OPT_VIEW_COMPACT, layout)
        for fname, fmt in formats:
            wall_root, wall_peers, ms_bind, wire = [], [], [], 0
            for _ in range(4):
                for ctx in ctxs:
                    ctx.view_bind(native.VIEW_MERGED)
                t0 = time.perf_counter()
                sent = [ctx.view_gather_merged(fmt) for ctx in ctxs[1:]]
                t1 = time.perf_counter()
                wire = root.view_gather_merged(fmt)
                wall_root.append((time.perf_counter() - t1) * 1e3)
                wall_peers.append((t1 - t0) * 1e3)
                ms_bind.append(root.stats()["ms_view_bind"])
                assert wire == sum(sent)
            st = root.stats()
            gathered = {f: root.view_pack(f2) for f, f2 in formats}
            r = {"ms_wall_root": min(wall_root[1:]), "ms_wall_root_first": wall_root[0], "ms_wall_peers": min(wall_peers[1:]),
                 "ms_view_bind": min(ms_bind[1:]), "wire_bytes": int(wire), "view_slots": int(st["view_slots"]),
                 "view_entries": int(st["view_entries"]), "view_overlaps": int(st["view_overlaps"]),
                 "view_layout_bytes": int(st["view_bytes"])}
            res["gather_merged"][f"{lname}_{fname}"] = r
            log(f"view_bench: gather {lname} {fname} {json.dumps(r)}")
            # the same frame through the host: every rank packs, the root binds the set
            wall_pack, wall_set, ms_set = [], [], []
            for _ in range(4):
                for ctx in ctxs:
                    ctx.view_bind(native.VIEW_MERGED)
                t0 = time.perf_counter()
                streams = [ctx.view_pack(fmt) for ctx in ctxs]
                t1 = time.perf_counter()
                root.view_bind_packed_set(streams)
                wall_set.append((time.perf_counter() - t1) * 1e3)
                wall_pack.append((t1 - t0) * 1e3)
                ms_set.append(root.stats()["ms_view_bind"])
            for f, f2 in formats:
                assert np.array_equal(root.view_pack(f2), gathered[f]), "the gather differs from the set bind of the ranks' streams"
            h = {"ms_wall_pack_all_ranks": min(wall_pack[1:]), "ms_wall_bind_packed_set": min(wall_set[1:]),
                 "ms_view_bind": min(ms_set[1:]), "host_bytes": sum(int(x.size) for x in streams)}
            res["through_the_host"][f"{lname}_{fname}"] = h
            log(f"view_bench: through the host {lname} {fname} {json.dumps(h)}")
            del streams, gathered
    for ctx in ctxs:
        ctx.close()
    group.close()
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--brick", type=int, default=512)
    ap.add_argument("--sim-n", type=int, default=512)
    ap.add_argument("--views", type=int, default=36)
    ap.add_argument("--passes", type=int, default=3, help="timed passes over the orbit per skip setting")
    ap.add_argument("--count-views", type=int, default=2,
                    help="views, evenly spaced on the orbit and none of them the generating one, whose work the CPU "
                         "restatement counts")
    ap.add_argument("--out-w", type=int, default=W_IMG)
    ap.add_argument("--out-h", type=int, default=H_IMG)
    ap.add_argument("--pack", action="store_true", help="also time the packed stream of the bound VDI, both formats")
    ap.add_argument("--compact", action="store_true",
                    help="every measurement also in the compact view layout (INSITU_OPT_VIEW_COMPACT), beside dense")
    ap.add_argument("--merged", action="store_true",
                    help="INSITU_VIEW_MERGED of the flatten context against INSITU_VIEW_GATHERED of the composite_vdi one")
    ap.add_argument("--packed-set", action="store_true",
                    help="insitu_view_bind_packed_set of the eight packed sub-VDIs against insitu_view_bind_host_set")
    ap.add_argument("--gather-merged", action="store_true",
                    help="insitu_view_gather_merged over a local group of 8 one-brick ranks against pack + bind_packed_set")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("view_bench: needs a GPU (timings are HIP-event times of the kernel)")
    if args.gather_merged:
        return run_gather_merged(args)
    if args.packed_set:
        return run_packed_set(args)
    if args.merged:
        return run_merged(args)
    from insitu_amd import native, scene
    from insitu_amd.renderer import InSituContext

    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    n = args.brick
    bricks = scene.grid_bricks(n * 2, 2)
    t0 = time.perf_counter()
    ctx = InSituContext(W_IMG, H_IMG, max_supersegments=S, bricks_per_rank=len(bricks), composite_vdi=True,
                        max_output_supersegments=S, keep_passes=False)
    ctx.set_transfer(scene.transfer_function(), scene.colormap_hot(), conv_scale=1.0 / 0.5, conv_offset=0.0)
    for bid, (origin, vw, _) in enumerate(bricks):
        v = scene.gray_scott(n, steps=1500, seed=1000 + bid, device=dev, sim_n=min(args.sim_n, n)).contiguous()
        ctx.set_brick(bid, v, scene.brick_model(origin, vw), dtype=native.F32)
        del v
    vw = bricks[0][1]
    torch.cuda.synchronize()
    log(f"view_bench: {len(bricks)} bricks of {n}^3 in {time.perf_counter() - t0:.1f} s")

    def cam_at(i):
        return scene.orbit_camera(W_IMG, H_IMG, yaw_deg=30.0 + 360.0 / args.views * i, pitch_deg=20.0, voxel_world=vw)

    gen_cam = cam_at(0)
    ctx.frame(gen_cam)
    layouts = (0, 1) if args.compact else (0,)   # INSITU_OPT_VIEW_COMPACT: dense, and beside it compact
    names = {0: "dense", 1: "compact"}
    cams = [cam_at(i) for i in range(args.views)]
    ow, oh = args.out_w, args.out_h

    def bind(layout):
        ctx.set_option(native.OPT_VIEW_COMPACT, layout)
        ctx.view_bind(native.VIEW_GATHERED)

    layout_info = {}
    for layout in layouts:
        ms_bind = []
        for _ in range(4):   # one warm-up (it allocates), then the best of three
            bind(layout)
            ms_bind.append(ctx.stats()["ms_view_bind"])
        st = ctx.stats()
        layout_info[names[layout]] = {"view_bytes": int(st["view_bytes"]), "view_entries": int(st["view_entries"]),
                                      "view_compact": int(st["view_compact"]), "ms_view_bind": min(ms_bind[1:]),
                                      "ms_view_bind_first": ms_bind[0]}
    log(f"view_bench: layouts {json.dumps(layout_info)}")

    def time_pack(layout):
        res = {}
        for name, fmt in (("float", native.PACK_FLOAT), ("half", native.PACK_HALF)):
            bind(layout)
            ms_pack, ms_wall, ms_unpack, ms_bind_wall = [], [], [], []
            for _ in range(4):
                t0 = time.perf_counter()
                stream = ctx.view_pack(fmt)
                ms_wall.append((time.perf_counter() - t0) * 1e3)
                ms_pack.append(ctx.stats()["ms_pack"])
            for _ in range(4):
                t0 = time.perf_counter()
                ctx.view_bind_packed(stream)
                ms_bind_wall.append((time.perf_counter() - t0) * 1e3)
                ms_unpack.append(ctx.stats()["ms_pack"])
            if fmt == native.PACK_FLOAT:   # (the round trip is exact: the same bytes again)
                assert np.array_equal(ctx.view_pack(fmt), stream)
            res[name] = {"bytes": int(stream.size), "ms_pack_kernels_with_count": ms_pack[0], "ms_pack_kernels": min(ms_pack[1:]), "ms_pack_wall": min(ms_wall[1:]),
                         "ms_unpack_kernels": min(ms_unpack[1:]), "ms_bind_packed_wall": min(ms_bind_wall[1:])}
            del stream
        return res

    pack = None
    if args.pack:
        pack = {"dense_readback_bytes": W_IMG * H_IMG * S * 24,
                "timing": "one warm-up, then the best of three; ms_pack: HIP events around the kernels alone"}
        pack.update(time_pack(0))
        if args.compact:
            pack["compact"] = time_pack(1)
        log(f"view_bench: pack {json.dumps(pack)}")

    def orbit(layout, skip):
        bind(layout)   # (the orbit views the exact VDI; with --compact the layouts alternate)
        ctx.set_option(native.OPT_VIEW_SKIP, skip)
        ms = []
        for cam in cams:
            ctx.view_render(cam, ow, oh)
            ms.append(ctx.stats()["ms_view"])
        return ms

    settings = [(layout, skip) for layout in layouts for skip in (1, 0)]
    for layout, skip in settings:   # warm-up: every camera, every setting
        orbit(layout, skip)
    all_times = {k: [] for k in settings}
    for _ in range(args.passes):
        for k in settings:
            all_times[k].append(orbit(*k))
    ctx.set_option(native.OPT_VIEW_SKIP, 1)
    bind(0)
    best = {k: np.asarray(v).min(axis=0) for k, v in all_times.items()}    # best of the passes, per camera
    times = {skip: all_times[(0, skip)] for skip in (1, 0)}
    per_view = {skip: best[(0, skip)] for skip in (1, 0)}
    spread = {k: float(np.max(np.asarray(v).max(axis=0) / np.asarray(v).min(axis=0))) for k, v in times.items()}
    compact = None
    if args.compact:
        compact = {"ms_per_view": {"skip": float(best[(1, 1)].mean()), "walk": float(best[(1, 0)].mean())},
                   "ms_min_max": {"skip": [float(best[(1, 1)].min()), float(best[(1, 1)].max())],
                                  "walk": [float(best[(1, 0)].min()), float(best[(1, 0)].max())]},
                   "ms_by_view_skip": [round(float(v), 4) for v in best[(1, 1)]],
                   "ms_by_view_walk": [round(float(v), 4) for v in best[(1, 0)]]}

    dep = ctx.read(native.BUF_GATHERED_DEPTH)
    counts = np.count_nonzero(dep[:, :, 0::2], axis=2)
    tiles_empty = None
    if W_IMG % 8 == 0 and H_IMG % 8 == 0:
        tiles_empty = float(np.mean(counts.reshape(W_IMG // 8, 8, H_IMG // 8, 8).max(axis=(1, 3)) == 0))
    work = []
    if args.count_views > 0:
        import view_binding
        col = ctx.read(native.BUF_GATHERED_COLOR)
        for i in (np.arange(1, args.count_views + 1) * args.views // (args.count_views + 1)).astype(int):
            t0 = time.perf_counter()
            rec = {"view": int(i)}
            for skip in (1, 0):
                _, _, (cells, examined, blended) = view_binding.render(col, dep, gen_cam, cams[i], ow, oh, skip=bool(skip),
                                                                       work=True)
                ms = float(per_view[skip][i])
                rec["skip" if skip else "walk"] = {
                    "ms": ms, "cells": cells, "entries_examined": examined, "entries_blended": blended,
                    "entry_gb_per_s": examined * ENTRY_BYTES / (ms * 1e-3) / 1e9,
                    "share_of_hbm_peak": examined * ENTRY_BYTES / (ms * 1e-3) / 1e9 / HBM_PEAK_GBS}
            work.append(rec)
            log(f"view_bench: counted view {i} on the CPU in {time.perf_counter() - t0:.1f} s")
    res = {
        "metric": f"ms per novel view @{ow}x{oh} of the composited VDI {W_IMG}x{H_IMG}x{S} (8x{n}^3 volume)",
        "views": args.views, "passes": args.passes,
        "ms_per_view": {"skip": float(per_view[1].mean()), "walk": float(per_view[0].mean())},
        "ms_min_max": {"skip": [float(per_view[1].min()), float(per_view[1].max())],
                       "walk": [float(per_view[0].min()), float(per_view[0].max())]},
        "ms_by_view_skip": [round(float(v), 4) for v in per_view[1]],
        "ms_by_view_walk": [round(float(v), 4) for v in per_view[0]],
        "pass_spread_max_over_min": spread,
        "vdi": {"entries": int(counts.sum()), "nonempty_lists": int(np.count_nonzero(counts)),
                "mean_entries_per_nonempty_list": float(counts.sum() / max(1, np.count_nonzero(counts))),
                "empty_tile_fraction": tiles_empty},
        "work": work,
        "pack": pack,
        "layouts": layout_info,   # view_bytes and the bind's kernels per view layout
        "compact": compact,       # --compact: the orbit in the compact layout, its passes alternating with dense
        "timing": "HIP events around vdi_view_kernel (insitu_stats.ms_view), best of the passes per camera",
    }
    ctx.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
