"""CPU reference of novel-view VDI rendering (tests/view_ref/view_ref.c) -- TEST INFRASTRUCTURE.

Builds the C99 restatement of DESIGN.md section 9 with the oracle's flags (oracle/Makefile) against
liboracle.so, which exports the contract's pow (orc_pow), and binds it with ctypes.  Also holds what the view
tests share: the cameras, the slab VDIs and their analytic (double precision) images.
"""
from __future__ import annotations

import ctypes
import math
import subprocess
from pathlib import Path

import numpy as np

import oracle_binding as orc
from insitu_amd import native, scene

ROOT = Path(__file__).resolve().parent.parent
SRC = ROOT / "tests" / "view_ref" / "view_ref.c"
LIB = ROOT / "tests" / "view_ref" / "_build" / "libview_ref.so"
CFLAGS = ["-O3", "-march=x86-64-v3", "-std=c99", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "-fopenmp",
          "-Wall", "-Wextra"]   # oracle/Makefile

_lib = None


def load():
    global _lib
    if _lib is not None:
        return _lib
    orc.load()   # builds liboracle.so when it is missing or stale
    if not LIB.exists() or LIB.stat().st_mtime < max(SRC.stat().st_mtime, orc.LIB.stat().st_mtime):
        LIB.parent.mkdir(parents=True, exist_ok=True)
        # (the run path is relative to the library, so the built tree may be moved or copied)
        subprocess.run(["gcc", *CFLAGS, "-shared", "-o", str(LIB), str(SRC), f"-L{orc.LIB.parent}", "-loracle",
                        "-Wl,-rpath,$ORIGIN/../../../oracle/_build", "-lm"], check=True)
    lib = ctypes.CDLL(str(LIB))
    vp, i = ctypes.c_void_p, ctypes.c_int
    lib.view_ref_render.argtypes = [vp, vp, i, i, i, vp, vp, i, i, i, i, vp, vp, vp, vp]
    _lib = lib
    return lib


def pv_of(cam) -> np.ndarray:
    """proj * view as the library forms it (float, the shaders' operation order)."""
    return orc.mat4_mul(cam.proj, cam.view)


def render(color: np.ndarray, depth: np.ndarray, gen_cam, cam, out_w: int, out_h: int, skip: bool = True,
           repack: bool = False, work: bool = False, part: bool = False):
    """The VDI (colour (W,H,S,4), depth (W,H,2S), generated from gen_cam) seen from cam:
    (rgba8 image (out_h,out_w,4), float accumulator (out_h,out_w,4)); with work also the walk's counts over all
    rays, (cells visited, list entries examined in them, entries blended); with part also, per output pixel,
    (out_h, out_w, 5) doubles: the ray's range s1 - s0 inside the cells' extent (0 when clipped away), the summed
    length and the number of the level-1 (tile) intervals it visited, and the same two of the level-2 (cell)
    intervals -- with skip the cells of empty tiles are not among the latter."""
    lib = load()
    c = np.ascontiguousarray(color, dtype=np.float32)
    d = np.ascontiguousarray(depth, dtype=np.float32)
    W, H, S = c.shape[0], c.shape[1], c.shape[2]
    assert c.shape == (W, H, S, 4) and d.shape == (W, H, 2 * S)
    pv_g = np.ascontiguousarray(pv_of(gen_cam), np.float32)
    ipv_n = np.ascontiguousarray(orc.ipv_of(cam), np.float32)
    acc = np.zeros((out_h, out_w, 4), np.float32)
    img = np.zeros((out_h, out_w, 4), np.uint8)
    counts = np.zeros(3, np.int64)
    parts = np.zeros((out_h, out_w, 5), np.float64) if part else None
    rc = lib.view_ref_render(c.ctypes.data, d.ctypes.data, W, H, S, pv_g.ctypes.data, ipv_n.ctypes.data, out_w, out_h,
                             1 if skip else 0, 1 if repack else 0, acc.ctypes.data, img.ctypes.data, counts.ctypes.data,
                             parts.ctypes.data if part else None)
    assert rc == 0, rc
    res = (img, acc)
    if work:
        res += (tuple(int(v) for v in counts),)
    if part:
        res += (parts,)
    return res


# ---------------------------------------------------------------- shared scenes of the view tests
VDI_W, VDI_H, VDI_S = 64, 48, 6
OUT_SIZES = ((64, 48), (50, 37))   # the VDI's own size; one that is neither a multiple of 8 nor that size


def gen_camera(W=VDI_W, H=VDI_H):
    """The generating camera of the view tests' VDIs (tests/scenes.make_scene's default orbit)."""
    return scene.orbit_camera(W, H, yaw_deg=30.0, pitch_deg=20.0, voxel_world=1.0 / 32)


def view_cameras(W=VDI_W, H=VDI_H) -> dict:
    """The viewing cameras: the generating one; yaw +20, +90 (the ray crosses many columns) and +180 degrees
    (lists walked back to front); one so close that G's frustum covers only part of the output; and one behind
    G's eye, whose rays cross G's camera plane."""
    g = dict(voxel_world=1.0 / 32)
    yaw, pitch = math.radians(30.0), math.radians(20.0)
    eye = 3.5 * np.array([math.cos(pitch) * math.sin(yaw), math.sin(pitch), math.cos(pitch) * math.cos(yaw)])
    fwd = -eye / np.linalg.norm(eye)
    side = np.cross(fwd, [0.0, 1.0, 0.0])
    side /= np.linalg.norm(side)
    # behind G's camera plane and to its side, looking at the volume: every ray starts behind that plane
    # (c_w < 0 at s = 0) and crosses it
    cross_eye = eye - 0.5 * fwd + 1.2 * side
    cross = scene.CameraSpec(scene.look_at(cross_eye, (0.0, 0.0, 0.0)), scene.perspective(50.0, W / H), nw=1.0)
    return {
        "same": gen_camera(W, H),
        "yaw20": scene.orbit_camera(W, H, yaw_deg=50.0, pitch_deg=20.0, **g),
        "yaw90": scene.orbit_camera(W, H, yaw_deg=120.0, pitch_deg=20.0, **g),
        "yaw180": scene.orbit_camera(W, H, yaw_deg=210.0, pitch_deg=20.0, **g),
        "close": scene.orbit_camera(W, H, radius=1.2, yaw_deg=75.0, pitch_deg=-10.0, fov_deg=100.0, **g),
        "cross": cross,
    }


def slab_vdi(layers, W=VDI_W, H=VDI_H, S=VDI_S):
    """A host VDI with the same supersegments in every list: layers = [(z0, z1, (r, g, b, a)), ...] in depth
    order, z in the generating view's NDC, a = opacity per unit world length."""
    col = np.zeros((W, H, S, 4), np.float32)
    dep = np.zeros((W, H, 2 * S), np.float32)
    for i, (z0, z1, rgba) in enumerate(layers):
        col[:, :, i, :] = np.asarray(rgba, np.float32)
        dep[:, :, 2 * i] = np.float32(z0)
        dep[:, :, 2 * i + 1] = np.float32(z1)
    return col, dep


def analytic_slabs(layers, gen_cam, cam, out_w: int, out_h: int, W=VDI_W, H=VDI_H, reverse: bool = False) -> np.ndarray:
    """Double-precision image of slab_vdi(layers) seen from cam, (out_h, out_w, 4) in [0, 1]: per layer the
    chord of the ray inside the frustum slab -- the cells' extent X(0) <= x <= X(W), Y(0) <= y <= Y(H) and
    z0 <= z <= z1, clipped in G's clip space -- gives alpha = 1 - (1 - a)^chord and rgb * alpha; the layers
    blend front to back in the order the ray meets them (reverse: in the opposite order, the image a walk
    that takes the lists the wrong way round would give).  Independent of view_ref.c: no cells, no DDA."""
    pv_g = np.asarray(gen_cam.proj_rm, np.float64) @ np.asarray(gen_cam.view_rm, np.float64)
    ipv_n = np.linalg.inv(np.asarray(cam.proj_rm, np.float64) @ np.asarray(cam.view_rm, np.float64))
    x_lo, x_hi = -1.0 - 1.0 / W, 1.0 - 1.0 / W
    y_lo, y_hi = -1.0 - 1.0 / H, 1.0 - 1.0 / H
    out = np.zeros((out_h, out_w, 4))
    for oy in range(out_h):
        for ox in range(out_w):
            uv = (ox / out_w * 2.0 - 1.0, oy / out_h * 2.0 - 1.0)
            wf = ipv_n @ np.array([uv[0], uv[1], -1.0, 1.0])
            wb = ipv_n @ np.array([uv[0], uv[1], 1.0, 1.0])
            wf, wb = wf / wf[3], wb / wb[3]
            L = float(np.linalg.norm(wb[:3] - wf[:3]))
            cf, cb = pv_g @ wf, pv_g @ wb
            d = cb - cf
            segs = []
            for z0, z1, rgba in layers:
                lo, hi = 0.0, 1.0
                # g(s) = g0 + s*dg >= 0 for each face of the frustum slab
                for axis, P, sign in ((0, x_lo, 1.0), (0, x_hi, -1.0), (1, y_lo, 1.0), (1, y_hi, -1.0),
                                      (2, float(np.float32(z0)), 1.0), (2, float(np.float32(z1)), -1.0)):
                    g0 = sign * (cf[axis] - P * cf[3])
                    dg = sign * (d[axis] - P * d[3])
                    if dg > 0.0:
                        lo = max(lo, -g0 / dg)
                    elif dg < 0.0:
                        hi = min(hi, -g0 / dg)
                    elif g0 < 0.0:
                        hi = -1.0
                if hi > lo:
                    segs.append((lo, (hi - lo) * L, rgba))
            C = np.zeros(4)
            for _, chord, rgba in sorted(segs, key=lambda t: t[0], reverse=reverse):
                a = 1.0 - (1.0 - float(np.float32(rgba[3]))) ** chord
                C[:3] += (1.0 - C[3]) * np.asarray(rgba[:3], np.float32).astype(np.float64) * a
                C[3] += (1.0 - C[3]) * a
            out[oy, ox] = C
    return out


def lsb_error(img: np.ndarray, analytic: np.ndarray) -> float:
    """Largest distance of the rgba8 image from the analytic value, in units of 1/255."""
    return float(np.max(np.abs(img.astype(np.float64) - np.clip(analytic, 0.0, 1.0) * 255.0)))


SLAB = [(0.9715, 0.9799, (0.5, 0.25, 0.75, 0.3))]   # about 3 to 4 world units from the generating eye


def layered_vdi(n: int, W: int, H: int, S: int | None = None):
    """SLAB cut into n abutting layers of its colour in every list (S slots, default n): the same analytic image
    as the one slab, (1 - a)^chord being multiplicative over abutting chords."""
    z0, z1, rgba = SLAB[0]
    z = np.linspace(z0, z1, n + 1).astype(np.float32)
    assert np.all(np.diff(z) > 0)   # the float32 depths are distinct
    return slab_vdi([(z[i], z[i + 1], rgba) for i in range(n)], W, H, n if S is None else S)


def list_end_vdi():
    """A 16x8, S = 6 host VDI of lists that end in every way a host list can: most hold 3 entries and a
    terminator; a block of them holds 2 entries, an entry with start depth 0 and 2 more entries that must not be
    seen; a block is full, 6 entries and no terminator; a block is empty."""
    W, H, S = 16, 8, 6
    col, dep = layered_vdi(6, W, H)
    col[..., 0:3] *= np.linspace(0.4, 1.0, 6, dtype=np.float32)[None, None, :, None]   # (tell the layers apart)
    col[:, :, 3:], dep[:, :, 6:] = 0.0, 0.0
    full_col, full_dep = layered_vdi(6, W, H)
    col[2:7, 1:5], dep[2:7, 1:5] = full_col[2:7, 1:5], full_dep[2:7, 1:5]
    dep[2:7, 1:5, 4], dep[2:7, 1:5, 10:] = 0.0, 0.0             # ends at entry 2; entries 3 and 4 lie behind it
    col[9:13, 3:8], dep[9:13, 3:8] = full_col[9:13, 3:8], full_dep[9:13, 3:8]   # full, no terminator
    col[13:16, 0:3], dep[13:16, 0:3] = 0.0, 0.0                  # empty
    return col, dep


def truncate_lists(col: np.ndarray, dep: np.ndarray):
    """The VDI with everything from each list's first entry with start depth 0 on zeroed out."""
    live = np.cumprod(dep[:, :, 0::2] != 0.0, axis=2).astype(bool)
    return col * live[..., None], dep * np.repeat(live, 2, axis=2)


def on_outer_plane(gen_cam, cam, out_w: int, out_h: int, W: int, H: int, tol: float = 1e-6) -> np.ndarray:
    """(out_h, out_w) bool: the pixels whose ray, in double, has at both ends a G-NDC x or y within tol of one
    outer plane of the cells' extent, X(0), X(W), Y(0) or Y(H) -- the ray lies in that plane, where the analytic
    image is discontinuous."""
    pv_g = np.asarray(gen_cam.proj_rm, np.float64) @ np.asarray(gen_cam.view_rm, np.float64)
    ipv_n = np.linalg.inv(np.asarray(cam.proj_rm, np.float64) @ np.asarray(cam.view_rm, np.float64))
    ox, oy = np.meshgrid(np.arange(out_w), np.arange(out_h))
    ndc = []
    for z in (-1.0, 1.0):
        p = np.stack([ox / out_w * 2.0 - 1.0, oy / out_h * 2.0 - 1.0, np.full(ox.shape, z), np.ones(ox.shape)], -1)
        p = p @ ipv_n.T
        c = (p / p[..., 3:]) @ pv_g.T
        ndc.append(c[..., :2] / c[..., 3:])
    out = np.zeros(ox.shape, bool)
    for axis, planes in ((0, (-1.0 - 1.0 / W, 1.0 - 1.0 / W)), (1, (-1.0 - 1.0 / H, 1.0 - 1.0 / H))):
        for P in planes:
            out |= (np.abs(ndc[0][..., axis] - P) <= tol) & (np.abs(ndc[1][..., axis] - P) <= tol)
    return out


# ---- shared by the GPU tests of the view subsystem (tests/test_gpu_view*.py) ----
def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def fails(ctx, rc, text):
    assert rc == -1
    msg = ctx.lib.insitu_last_error(ctx.h).decode()
    assert text in msg, msg


def set_bricks(ctx, scenes, first=0):
    sc = scenes[0]
    ctx.set_transfer(sc["tf"], sc["cmap"], sc["conv_scale"], sc["conv_offset"])
    for b, s in enumerate(scenes):
        ctx.set_brick(first + b, s["vol"], s["model"])


def read_all(ctx, n):
    return ([ctx.read(native.BUF_VDI_COLOR, b) for b in range(n)], [ctx.read(native.BUF_VDI_DEPTH, b) for b in range(n)])


def random_set(n, seed, w=16, h=8, s=2):
    """n VDIs of 16x8, S = 2: list lengths 0..2, start depths drawn from 24 shared values (so lists tie), sorted
    inside a list, every entry as long as half a step of those values."""
    rng = np.random.default_rng(seed)
    grid = np.linspace(0.9, 0.99, 24).astype(np.float32)
    half = np.float32(0.5) * (grid[1] - grid[0])
    cols, deps = [], []
    for _ in range(n):
        pick = np.sort(rng.integers(0, 12, size=(w, h, s)) * 2 + np.arange(s), axis=2)   # distinct, increasing
        start = grid[pick]
        counts = rng.integers(0, s + 1, size=(w, h))
        live = np.arange(s)[None, None, :] < counts[:, :, None]
        dep = np.zeros((w, h, 2 * s), np.float32)
        dep[:, :, 0::2] = start * live
        dep[:, :, 1::2] = (start + half) * live
        col = rng.random(size=(w, h, s, 4), dtype=np.float32) * live[..., None]
        cols.append(col.astype(np.float32))
        deps.append(dep)
    return cols, deps
