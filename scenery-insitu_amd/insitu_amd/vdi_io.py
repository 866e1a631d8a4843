"""On-disk VDI dumps in the reference's formats.

The reference dumps raw texture bytes with `SystemHelpers.dumpToFile(buffer, path)`:
  sub-VDIs       `{basePath}{dataset}SubVDI{n}_ndc_col` / `_ndc_depth`         DistributedVolumes.kt:848-849
  received sets  `{basePath}{dataset}SetOfVDI{n}_ndc_col` / `_ndc_depth`       DistributedVolumes.kt:974-975
  composited     `{basePath}{dataset}CompositedVDI{n}_ndc_col` / `_ndc_depth`  DistributedVolumes.kt:894-895
Colour is the rgba32f image3D (S, H, W) -- supersegment fastest, then y, then x -- and depth the r32f
image3D (2S, H, W) (DistributedVolumes.kt:349-368), which is exactly the byte order of the
(W, H, S, 4) / (W, H, 2S) float32 arrays `InSituContext.read` returns.

The octree grid (OctreeCells, r32ui (W/8, H/8, S), x fastest) is dumped next to a VDI as
`{fileName}_octree` (VolumeFromFileExample.kt:1061-1071, fileName
`{dataset}VDI_{W}_{H}_{S}_{vo}_{cnt}_ndc` or `..._world_new`): `volume_file_paths` / `write_octree`.

The frame metadata (`VDIDataIO.write(VDIData(VDIBufferSizes(), VDIMetadata(index, projection, view,
volumeDimensions, model, nw, windowDimensions)))`, DistributedVolumes.kt:706-716, 910-915;
VDIConverter.kt:243-257) is written by scenery's serializer, which is a dependency outside the
reference tree and absent here, so its byte format cannot be reproduced or checked (parity unpinned).
The constructor arguments are written instead, under the reference's file name
`{basePath}{dataset}vdi_{W}_{H}_{S}_0_dump{n}`, as JSON with the VDIMetadata parameter names;
INTEGRATION.md shows the few Kotlin lines that turn it into a VDIDataIO file with scenery on the
classpath.  Matrices are column-major float lists (JOML order); `projection` is the OpenGL projection
as the reference stores it (the Vulkan fix is applied by the consumer, DistributedVolumes.kt:721),
`projection_vulkan` the corrected one the kernels use.

The packed stream (`pack_vdi` / `unpack_vdi` / `write_packed` / `read_packed`) is this
project's own format, what stands in for the compacted VDI the reference streams to a remote viewer
(VolumeFromFileExample.kt:907-1030): a 128-byte header, a count per pixel, and the stored entries alone.  The
functions here are pure numpy on the reference layout, byte for byte what `InSituContext.view_pack` produces on the
GPU, so a client without a GPU or this library's native half can read a stream.

`merge_packed` merges a set of packed streams into one, as
`InSituContext.view_bind_packed_set` binds them on the GPU.

`merge_vdis` is the merged bind in numpy: the VDIs of one frame and camera -- the per-rank
SubVDI dumps, say -- combined per pixel into one lossless VDI, as `InSituContext.view_bind_host_set` combines them on
the GPU.
"""
from __future__ import annotations

import json
import struct
from pathlib import Path

import numpy as np

KINDS = ("SubVDI", "SetOfVDI", "CompositedVDI")


def vdi_paths(base_path: str | Path, dataset: str, kind: str, counter: int) -> tuple[Path, Path]:
    if kind not in KINDS:
        raise ValueError(f"kind must be one of {KINDS}")
    stem = f"{base_path}{dataset}{kind}{counter}_ndc"
    return Path(stem + "_col"), Path(stem + "_depth")


def dump_to_file(array: np.ndarray, path: str | Path) -> None:
    """SystemHelpers.dumpToFile: the buffer's bytes, nothing else."""
    with open(path, "wb") as f:
        f.write(np.ascontiguousarray(array).tobytes())


def write_vdi(base_path: str | Path, dataset: str, kind: str, counter: int, colour: np.ndarray,
              depth: np.ndarray) -> tuple[Path, Path]:
    colour = np.asarray(colour, dtype=np.float32)
    depth = np.asarray(depth, dtype=np.float32)
    if colour.ndim != 4 or colour.shape[3] != 4 or depth.shape != colour.shape[:2] + (2 * colour.shape[2],):
        raise ValueError("expected colour (W, H, S, 4) and depth (W, H, 2S) float32")
    cp, dp = vdi_paths(base_path, dataset, kind, counter)
    dump_to_file(colour, cp)
    dump_to_file(depth, dp)
    return cp, dp


def read_vdi(colour_path: str | Path, depth_path: str | Path, width: int, height: int,
             supersegments: int) -> tuple[np.ndarray, np.ndarray]:
    """Raw dump -> ((W, H, S, 4), (W, H, 2S)) float32; the file sizes must match exactly."""
    n = width * height * supersegments
    c = np.fromfile(colour_path, dtype=np.float32)
    d = np.fromfile(depth_path, dtype=np.float32)
    if c.size != 4 * n or d.size != 2 * n:
        raise ValueError(f"dump sizes {c.size}, {d.size} floats do not match {width}x{height}x{supersegments}")
    return c.reshape(width, height, supersegments, 4), d.reshape(width, height, 2 * supersegments)


def volume_file_paths(dataset: str, width: int, height: int, supersegments: int, vo: int, counter: int,
                      world_abs: bool = False, base_path: str | Path = "") -> tuple[Path, Path, Path]:
    """VolumeFromFileExample.kt:1056-1071: (colour, depth, octree) dump paths of a stored VDI."""
    suffix = "world_new" if world_abs else "ndc"
    stem = f"{base_path}{dataset}VDI_{width}_{height}_{supersegments}_{vo}_{counter}_{suffix}"
    return Path(stem + "_col"), Path(stem + "_depth"), Path(stem + "_octree")


def write_octree(path: str | Path, octree: np.ndarray) -> Path:
    """gridCellsBuff: the (S, H/8, W/8) uint32 cell counts (x fastest), raw."""
    octree = np.asarray(octree)
    if octree.dtype != np.uint32 or octree.ndim != 3:
        raise ValueError("expected a (S, H/8, W/8) uint32 octree grid")
    dump_to_file(octree, path)
    return Path(path)


def read_octree(path: str | Path, width: int, height: int, supersegments: int) -> np.ndarray:
    o = np.fromfile(path, dtype=np.uint32)
    if o.size != supersegments * (height // 8) * (width // 8):
        raise ValueError(f"octree dump has {o.size} cells, expected {supersegments}x{height // 8}x{width // 8}")
    return o.reshape(supersegments, height // 8, width // 8)


def write_received_set(base_path: str | Path, dataset: str, counter: int, colour: np.ndarray,
                       depth: np.ndarray) -> tuple[Path, Path]:
    """SetOfVDI{n}_ndc_col / _ndc_depth (DistributedVolumes.kt:974-975): the received blocks,
    source-major, each (W/P, H, S) -- (V, W/P, H, S, 4) / (V, W/P, H, 2S) float32."""
    colour = np.asarray(colour, dtype=np.float32)
    depth = np.asarray(depth, dtype=np.float32)
    if colour.ndim != 5 or depth.shape != colour.shape[:3] + (2 * colour.shape[3],):
        raise ValueError("expected colour (V, W/P, H, S, 4) and depth (V, W/P, H, 2S) float32")
    cp, dp = vdi_paths(base_path, dataset, "SetOfVDI", counter)
    dump_to_file(colour, cp)
    dump_to_file(depth, dp)
    return cp, dp


def metadata_path(base_path: str | Path, dataset: str, width: int, height: int, supersegments: int,
                  counter: int) -> Path:
    return Path(f"{base_path}{dataset}vdi_{width}_{height}_{supersegments}_0_dump{counter}")


def write_metadata(base_path: str | Path, dataset: str, width: int, height: int, supersegments: int, counter: int,
                   cam, model: np.ndarray, volume_dims, nw: float | None = None) -> Path:
    """VDIMetadata fields of one frame (DistributedVolumes.kt:706-716) as JSON."""
    from .scene import VULKAN_FIX, col_major
    proj_gl = np.linalg.inv(VULKAN_FIX) @ cam.proj_rm
    meta = {
        "format": "scenery-insitu_amd VDIMetadata v2 (constructor arguments of graphics.scenery.volumes.vdi."
                  "VDIData(VDIBufferSizes(), VDIMetadata(...)))",
        "index": int(counter),
        "projection": col_major(proj_gl).tolist(),
        "projection_vulkan": np.asarray(cam.proj, np.float32).tolist(),
        "view": np.asarray(cam.view, np.float32).tolist(),
        "model": np.asarray(model, np.float32).reshape(16).tolist(),
        "volumeDimensions": [float(v) for v in volume_dims],
        "nw": float(cam.nw if nw is None else nw),
        "windowDimensions": [int(width), int(height)],
        "maxSupersegments": int(supersegments),
        "layout": {"colour": "rgba32f image3D (S, H, W), x = supersegment fastest",
                   "depth": "r32f image3D (2S, H, W): start, end per supersegment (NDC z)"},
    }
    p = metadata_path(base_path, dataset, width, height, supersegments, counter)
    p.write_text(json.dumps(meta, indent=1))
    return p


def read_metadata(path: str | Path) -> dict:
    return json.loads(Path(path).read_text())


# ---------------------------------------------------------------- the merged VDI of a set
MERGE_MAX_LISTS = 32     # kMaxLists
MERGE_MAX_SLOTS = 255    # counts are bytes


def merge_vdis(colours, depths) -> tuple[np.ndarray, np.ndarray, int]:
    """Reference-layout VDIs of one size and one generating camera (sequences of colour (W, H, S, 4) and depth
    (W, H, 2S) float32) -> (colour (W, H, S_m, 4), depth (W, H, 2 S_m), overlaps): per pixel the k-way merge of
    the lists by start depth that the flatten compositor walks (determineNextSupseg, VDICompositor.comp:58-91).
    A list ends before its first entry whose start depth is 0; the merged list takes, repeatedly, the front with
    the smallest start depth below 100000, the lowest list on a tie; entries are copied bit for bit.  S_m =
    max(1, the largest sum of a pixel's list lengths); ValueError when it exceeds 255.  overlaps counts the
    adjacent merged entries whose next start lies before the previous end (0 for the bricks of a domain
    decomposition; the novel-view renderer trusts a list not to overlap)."""
    cs = [np.ascontiguousarray(c, dtype=np.float32) for c in colours]
    ds = [np.ascontiguousarray(d, dtype=np.float32) for d in depths]
    n = len(cs)
    if not 1 <= n <= MERGE_MAX_LISTS or len(ds) != n:
        raise ValueError(f"expected 1 to {MERGE_MAX_LISTS} colour / depth pairs")
    W, H, S = cs[0].shape[:3] if cs[0].ndim == 4 else (0, 0, 0)
    for c, d in zip(cs, ds):
        if c.ndim != 4 or c.shape != (W, H, S, 4) or d.shape != (W, H, 2 * S) or min(W, H, S) < 1:
            raise ValueError("expected colour (W, H, S, 4) and depth (W, H, 2S) float32 of one size")
    col = np.stack(cs)                              # (n, W, H, S, 4)
    dep = np.stack(ds).reshape(n, W, H, S, 2)
    start = dep[..., 0]
    lens = np.cumprod(start != 0.0, axis=3).sum(axis=3)      # (n, W, H)
    s_m = max(1, int(lens.sum(axis=0).max()))
    if s_m > MERGE_MAX_SLOTS:
        raise ValueError(f"the merged lists hold up to {s_m} entries per pixel, at most {MERGE_MAX_SLOTS} fit")
    out_col = np.zeros((W, H, s_m, 4), np.float32)
    out_dep = np.zeros((W, H, s_m, 2), np.float32)
    taken = np.zeros((n, W, H), np.intp)
    wi, hi = np.indices((W, H))
    overlaps, prev_end = 0, None
    for k in range(s_m):
        at = np.minimum(taken, S - 1)
        front = np.take_along_axis(start, at[..., None], axis=3)[..., 0]
        ok = (taken < lens) & (front < np.float32(100000.0))
        j = np.argmin(np.where(ok, front, np.inf), axis=0)   # (the first of equal minima: the lowest list)
        has = np.take_along_axis(ok, j[None], axis=0)[0]
        if not has.any():
            break
        e = at[j, wi, hi]
        d = dep[j, wi, hi, e]
        out_col[has, k] = col[j, wi, hi, e][has]
        out_dep[has, k] = d[has]
        if k:
            overlaps += int(np.count_nonzero(has & (d[..., 0] < prev_end)))
        prev_end = d[..., 1]
        taken[j[has], wi[has], hi[has]] += 1
    return out_col, out_dep.reshape(W, H, 2 * s_m), overlaps


# ---------------------------------------------------------------- the packed stream, format version 1
PACK_MAGIC = b"IVDP"
PACK_VERSION = 1
PACK_FLOAT, PACK_HALF = 0, 1          # enum insitu_pack_format
PACK_HEADER_BYTES = 128
PACK_MAX_PIXELS = 1 << 30
_PACK_HEADER = struct.Struct("<4sIIIIIQ16f32x")   # magic, version, format, W, H, S, E, pv_g, zeros


def packed_size(width: int, height: int, entries: int, fmt: int) -> int:
    """128 + pad16(W*H) + 8 E + (16 | 8) E."""
    return PACK_HEADER_BYTES + (width * height + 15) // 16 * 16 + entries * (8 + (8 if fmt == PACK_HALF else 16))


def pack_vdi(colour: np.ndarray, depth: np.ndarray, pv_g, fmt: int = PACK_FLOAT) -> np.ndarray:
    """Reference-layout VDI (colour (W, H, S, 4), depth (W, H, 2S) float32) and the generating camera's
    proj * view (16 floats, column-major) -> the packed stream, uint8.  PACK_HALF rounds the colours to binary16
    (astype(float16): nearest even, subnormals kept, beyond 65504 infinity); depths stay float32."""
    colour = np.ascontiguousarray(colour, dtype=np.float32)
    depth = np.ascontiguousarray(depth, dtype=np.float32)
    if colour.ndim != 4 or colour.shape[3] != 4 or depth.shape != colour.shape[:2] + (2 * colour.shape[2],):
        raise ValueError("expected colour (W, H, S, 4) and depth (W, H, 2S) float32")
    W, H, S = colour.shape[:3]
    if fmt not in (PACK_FLOAT, PACK_HALF):
        raise ValueError(f"unknown format {fmt}")
    if W < 1 or H < 1 or not 1 <= S <= 255 or W * H > PACK_MAX_PIXELS:
        raise ValueError("needs W, H > 0, at most 2^30 pixels and S in [1,255]")
    pv = np.asarray(pv_g, dtype=np.float32).reshape(-1)
    if pv.size != 16:
        raise ValueError("pv_g must hold 16 floats")
    # row-major pixels (y*W + x), each list first entry to last: the boolean mask of (H, W, S) picks them in order
    live = np.cumprod(depth[:, :, 0::2] != 0.0, axis=2).astype(bool).transpose(1, 0, 2)
    counts = live.sum(axis=2).astype(np.uint8)
    dep = depth.reshape(W, H, S, 2).transpose(1, 0, 2, 3)[live]
    col = colour.transpose(1, 0, 2, 3)[live]
    if fmt == PACK_HALF:
        with np.errstate(over="ignore"):
            col = col.astype(np.float16)
    E = int(dep.shape[0])
    out = np.zeros(packed_size(W, H, E, fmt), np.uint8)
    out[:PACK_HEADER_BYTES] = np.frombuffer(_PACK_HEADER.pack(PACK_MAGIC, PACK_VERSION, fmt, W, H, S, E, *pv.tolist()), np.uint8)
    out[PACK_HEADER_BYTES:PACK_HEADER_BYTES + W * H] = counts.reshape(-1)
    d0 = PACK_HEADER_BYTES + (W * H + 15) // 16 * 16
    out[d0:d0 + 8 * E] = np.ascontiguousarray(dep).view(np.uint8).reshape(-1)
    out[d0 + 8 * E:] = np.ascontiguousarray(col).view(np.uint8).reshape(-1)
    return out


def unpack_vdi(buf) -> tuple[np.ndarray, np.ndarray, np.ndarray, int]:
    """Packed stream -> (colour (W, H, S, 4), depth (W, H, 2S), pv_g (16,), format), float32, zero past every
    list's count.  PACK_HALF colours are widened exactly.  ValueError on everything the library rejects: magic,
    version, format, W or H of 0, S outside 1..255, a size that is not exactly what the header implies, a count
    above S, counts that do not add up to the header's entry count."""
    b = np.frombuffer(buf, np.uint8) if isinstance(buf, (bytes, bytearray, memoryview)) else np.asarray(buf)
    if b.dtype != np.uint8 or b.ndim != 1:
        raise ValueError("expected bytes or a one-dimensional uint8 array")
    if b.size < PACK_HEADER_BYTES:
        raise ValueError("stream shorter than its header")
    magic, version, fmt, W, H, S, E, *pv = _PACK_HEADER.unpack(b[:PACK_HEADER_BYTES].tobytes())
    if magic != PACK_MAGIC:
        raise ValueError("bad magic")
    if version != PACK_VERSION:
        raise ValueError(f"unknown version {version}")
    if fmt not in (PACK_FLOAT, PACK_HALF):
        raise ValueError(f"unknown format {fmt}")
    if W == 0 or H == 0:
        raise ValueError("W and H must be > 0")
    if not 1 <= S <= 255:
        raise ValueError("S must be in [1,255]")
    if W * H > PACK_MAX_PIXELS or E > W * H * S:
        raise ValueError("dimensions or entry count out of range")
    if b.size != packed_size(W, H, E, fmt):
        raise ValueError(f"stream of {b.size} bytes, the header implies {packed_size(W, H, E, fmt)}")
    counts = b[PACK_HEADER_BYTES:PACK_HEADER_BYTES + W * H].reshape(H, W)
    if int(counts.max()) > S:
        raise ValueError(f"a count of {int(counts.max())} exceeds S = {S}")
    if int(counts.sum(dtype=np.uint64)) != E:
        raise ValueError(f"the counts add up to {int(counts.sum(dtype=np.uint64))}, the header says {E}")
    d0 = PACK_HEADER_BYTES + (W * H + 15) // 16 * 16
    dep = b[d0:d0 + 8 * E].view(np.float32).reshape(E, 2)
    if fmt == PACK_HALF:
        col = b[d0 + 8 * E:].view(np.float16).reshape(E, 4).astype(np.float32)
    else:
        col = b[d0 + 8 * E:].view(np.float32).reshape(E, 4)
    live = np.arange(S)[None, None, :] < counts[:, :, None]
    colour = np.zeros((H, W, S, 4), np.float32)
    depth = np.zeros((H, W, S, 2), np.float32)
    colour[live] = col
    depth[live] = dep
    return (np.ascontiguousarray(colour.transpose(1, 0, 2, 3)),
            np.ascontiguousarray(depth.transpose(1, 0, 2, 3)).reshape(W, H, 2 * S), np.asarray(pv, np.float32), int(fmt))


def merge_packed(streams, fmt: int = PACK_FLOAT) -> np.ndarray:
    """Packed streams of one window and one generating camera -> the packed stream of their merged VDI, what
    `InSituContext.view_bind_packed_set` binds on the GPU, for a client without one: each stream unpacked,
    zero-padded to the largest S, merged by `merge_vdis` and packed in `fmt` with the common pv_g.  ValueError on
    an empty set or more than 32 streams, on differing W, H or pv_g (compared bit for bit), and on everything
    `unpack_vdi` or `merge_vdis` raises."""
    streams = list(streams)
    if not 1 <= len(streams) <= MERGE_MAX_LISTS:
        raise ValueError(f"expected 1 to {MERGE_MAX_LISTS} streams, got {len(streams)}")
    vdis = []
    for j, b in enumerate(streams):
        try:
            vdis.append(unpack_vdi(b))
        except ValueError as e:
            raise ValueError(f"stream {j}: {e}") from None
    c0, _, pv0, _ = vdis[0]
    for j, (c, _, pv, _) in enumerate(vdis):
        if c.shape[:2] != c0.shape[:2]:
            raise ValueError(f"stream {j}: W and H differ from stream 0's")
        if pv.tobytes() != pv0.tobytes():
            raise ValueError(f"stream {j}: the generating camera differs from stream 0's")
    s_max = max(c.shape[2] for c, _, _, _ in vdis)
    cols, deps = [], []
    for c, d, _, _ in vdis:
        W, H, S = c.shape[:3]
        cp = np.zeros((W, H, s_max, 4), np.float32)
        dp = np.zeros((W, H, s_max, 2), np.float32)
        cp[:, :, :S] = c
        dp[:, :, :S] = d.reshape(W, H, S, 2)
        cols.append(cp)
        deps.append(dp.reshape(W, H, 2 * s_max))
    col, dep, _ = merge_vdis(cols, deps)
    return pack_vdi(col, dep, pv0, fmt)


def write_packed(path: str | Path, colour: np.ndarray, depth: np.ndarray, pv_g, fmt: int = PACK_FLOAT) -> Path:
    dump_to_file(pack_vdi(colour, depth, pv_g, fmt), path)
    return Path(path)


def read_packed(path: str | Path) -> tuple[np.ndarray, np.ndarray, np.ndarray, int]:
    return unpack_vdi(np.fromfile(path, dtype=np.uint8))
