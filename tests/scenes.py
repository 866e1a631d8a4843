"""Small deterministic scenes shared by the CPU and GPU tests (test infrastructure)."""
from __future__ import annotations

import numpy as np

from insitu_amd import native, scene


_CACHE: dict = {}


def gray_scott_u16(n: int = 32, steps: int = 1500, seed: int = 1000) -> np.ndarray:
    key = (n, steps, seed)
    if key not in _CACHE:
        _CACHE[key] = scene.to_uint16(scene.gray_scott(n, steps=steps, seed=seed), vmax=0.5)
    return _CACHE[key]


def make_scene(n=32, W=64, H=48, yaw=30.0, pitch=20.0, samples_per_voxel=1.0, dtype="u16", seed=1000,
               origin=(-0.5, -0.5, -0.5), world=1.0, steps=1500, conv_scale=1.0, conv_offset=0.0):
    """One brick of edge `world` centred at the origin, camera orbiting at radius 3.5."""
    vol16 = gray_scott_u16(n, steps=steps, seed=seed)
    if dtype == "u16":
        vol, dt = vol16, native.U16
    elif dtype == "u8":
        vol, dt = (vol16 >> 8).astype(np.uint8), native.U8
    else:
        vol, dt = (vol16.astype(np.float32) / np.float32(65535.0) * np.float32(0.5)), native.F32
    vw = world / n
    model = scene.brick_model(origin, vw)
    im = scene.inverse_model(model)
    cam = scene.orbit_camera(W, H, yaw_deg=yaw, pitch_deg=pitch, voxel_world=vw,
                             samples_per_voxel=samples_per_voxel)
    tf = scene.transfer_function()
    cmap = scene.colormap_hot()
    conv_k = scene.folded_conv_scale(conv_scale, dt)
    return dict(vol=vol, dtype=dt, model=model, im=im, cam=cam, tf=tf, cmap=cmap, conv_scale=conv_scale,
                conv_offset=conv_offset, conv_k=conv_k, W=W, H=H)


# ---------------------------------------------------------------- the N-rank strip scene
# The bricks of the multi-rank group tests seen from close by (radius 2.0: at the default 3.5 the outer strips
# of a window are empty), shared by the CPU pin (test_compositor_oracle.py) and the GPU strip tests
# (test_gpu_strips.py).  nb == 4: 2 x 2 x 1 unit bricks at z = -0.5 (Gray-Scott seeds 11..14); nb > 4: the
# first nb of 2 x 2 x 2 bricks, the second z layer re-using the four fields rolled by 5 voxels along y.

STRIP_S = 6


def strip_bricks(nb: int) -> list:
    """nb bricks as make_scene dicts (vol, model, im, tf, cmap, conv_*), 24^3 voxels each."""
    out = []
    for i in range(nb):
        origin = (-1.0 + (i % 2), -1.0 + (i // 2), -0.5) if nb == 4 else (-1.0 + (i % 2), -1.0 + (i // 2) % 2, -1.0 + (i // 4))
        b = make_scene(n=24, seed=11 + i % 4, origin=origin)
        if i >= 4:
            b["vol"] = np.roll(b["vol"], 5, axis=1).copy()
        out.append(b)
    return out


def strip_camera(W: int, H: int, yaw: float = 35.0, pitch: float = 20.0):
    return scene.orbit_camera(W, H, radius=2.0, yaw_deg=yaw, pitch_deg=pitch, voxel_world=1.0 / 24)


# ---------------------------------------------------------------- inputs off the one scene
# Named variants of make_scene(n=32, yaw=40): each changes ONE input of the base scene (transfer function,
# colour map, conversion, camera, model matrix or field) and returns the same dict, so the CPU pins
# (test_oracle_pin.py) and the GPU parity tests (test_gpu_inputs.py) share them.

def tf_variant(name: str, n: int = 1024) -> np.ndarray:
    """Alpha LUTs sampled at texel centres t = (i + 0.5) / n."""
    t = (np.arange(n) + 0.5) / n
    if name == "step":            # 0 below t = 0.3, 0.9 above
        a = np.where(t < 0.3, 0.0, 0.9)
    elif name == "opaque":        # alpha exactly 1.0 on half the table: log2(1 - a) = -inf
        a = np.clip(2.0 * t, 0.0, 1.0)
    elif name == "near_opaque":   # the same, capped at the largest float below 1
        a = np.minimum(np.clip(2.0 * t, 0.0, 1.0), 1.0 - 2.0 ** -24)
    elif name == "faint":
        return (scene.transfer_function(n=n) * np.float32(1e-3)).astype(np.float32)
    elif name == "comb":          # non-monotonic
        a = 0.5 * ((16.0 * t) % 1.0)
    elif name == "out_of_range":  # alpha below 0 and above 1: the ABI accepts any finite value
        a = 1.5 * t - 0.25
    elif name == "tf_1texel":
        a = np.array([0.4])
    elif name == "tf_2texel":
        a = np.array([0.0, 0.8])
    else:
        raise ValueError(name)
    return a.astype(np.float32)


TF_VARIANTS = ("step", "opaque", "near_opaque", "faint", "comb", "out_of_range", "tf_1texel", "tf_2texel")


def cmap_variant(name: str) -> np.ndarray:
    """Colour maps (alpha channel 1) with the filter constant c = max(1, 2C, 2CA) they give under the
    default transfer function (A = 0.75) in brackets."""
    hot = scene.colormap_hot().astype(np.float64)
    cm = hot.copy()
    if name == "dark":        # [c = 1]
        cm[:, :3] = hot[:, :3] * 1e-3
    elif name == "hdr":       # [c = 16]
        cm[:, :3] = hot[:, :3] * 8.0
    elif name == "signed":    # [c = 2], rgb in [-1, 1]: red below -0.5 skips samples (AccumulateVDI.comp:12)
        cm[:, :3] = (hot[:, :3] - 0.5) * 2.0
    elif name == "big":       # [c = 9.8e5, just under the 1e6 where the filter turns itself off]
        cm[:, :3] = hot[:, :3] * 4.9e5
    elif name == "huge":      # [c = inf: exact decisions only]
        cm[:, :3] = hot[:, :3] * 2e6
    elif name == "cmap_1texel":
        cm = np.array([[0.9, 0.5, 0.2, 1.0]])
    elif name == "cmap_2texel":
        cm = np.array([[0.0, 0.0, 1.0, 1.0], [1.0, 0.5, 0.0, 1.0]])
    else:
        raise ValueError(name)
    return cm.astype(np.float32)


CMAP_VARIANTS = ("dark", "hdr", "signed", "big", "huge", "cmap_1texel", "cmap_2texel")

# (conv_scale, conv_offset): LUT coordinates below 0 and above 1 (the last one: above only).  The Gray-Scott
# brick spans [0.04, 0.58] of the voxel range, so the pairs are steep enough to push 5 % of it out on each side.
CONV_VARIANTS = {"conv_wide": (4.0, -1.0), "conv_negative": (-4.0, 2.0), "conv_high": (1.0, 0.6)}

CAMERA_VARIANTS = {
    "cam_inside": dict(radius=0.2),                          # the eye inside the brick
    "cam_near_cut": dict(radius=0.55),                       # the near plane cuts the brick
    "cam_wide": dict(radius=1.2, fov_deg=110.0),
    "cam_pitch89": dict(pitch_deg=89.0),
    "cam_offcentre": dict(center=(0.6, 0.3, 0.0), radius=2.0),   # the brick partly off screen
    "cam_spv_half": dict(samples_per_voxel=0.5),
    "cam_spv3": dict(samples_per_voxel=3.0),
    "cam_tmax": dict(),                                      # the default camera with tmax = TMAX_CUT
}
TMAX_CUT = 0.17

MODEL_VARIANTS = ("model_aniso", "model_rot30", "brick_1x1x1", "brick_1x3x2", "brick_slab", "brick_nz1",
                  "brick_nz1_unit")

FIELD_VARIANTS = ("field_noise", "field_const", "field_checker", "field_f32_range", "field_f32_nonfinite")


def _model_rm(scale, origin, rot_y_deg: float = 0.0) -> np.ndarray:
    """Column-major model matrix: world = R_y * (origin + scale * p)."""
    m = np.eye(4)
    m[0, 0], m[1, 1], m[2, 2] = scale
    m[:3, 3] = origin
    a = np.radians(rot_y_deg)
    r = np.eye(4)
    r[0, 0], r[0, 2], r[2, 0], r[2, 2] = np.cos(a), np.sin(a), -np.sin(a), np.cos(a)
    return scene.col_major(r @ m)


def field_variant(name: str, n: int = 32):
    """(volume [z][y][x], native dtype) of the synthetic fields."""
    if name == "field_noise":      # u16 white noise over the full range
        return np.random.default_rng(77).integers(0, 65536, (n, n, n), dtype=np.uint16), native.U16
    if name == "field_const":
        return np.full((n, n, n), 65535, np.uint16), native.U16
    if name == "field_checker":    # 3-D checkerboard of 0 and 65535
        z, y, x = np.indices((n, n, n))
        return (((x + y + z) & 1) * 65535).astype(np.uint16), native.U16
    g = gray_scott_u16(n).astype(np.float32) / np.float32(65535.0)
    if name == "field_f32_range":  # Gray-Scott mapped to [-1, 2]
        return (g * np.float32(3.0) - np.float32(1.0)).astype(np.float32), native.F32
    if name == "field_f32_nonfinite":   # blocks of NaN, +inf and -inf inside the Gray-Scott field
        v = g.copy()
        q = n // 4
        v[q:2 * q, q:2 * q, q:2 * q] = np.nan
        v[2 * q:3 * q, q:2 * q, 2 * q:3 * q] = np.inf
        v[q:2 * q, 2 * q:3 * q, 2 * q:3 * q] = -np.inf
        return v, native.F32
    raise ValueError(name)


def variant_scene(name: str, W: int = 64, H: int = 48, n: int = 32, dtype: str = "u16", yaw: float = 40.0):
    """The base scene make_scene(n, W, H, yaw=40) with the one input `name` changed ("base": nothing)."""
    sc = make_scene(n=n, W=W, H=H, yaw=yaw, dtype=dtype)
    vw = 1.0 / n
    if name == "base":
        pass
    elif name in TF_VARIANTS:
        sc["tf"] = tf_variant(name)
    elif name in CMAP_VARIANTS:
        sc["cmap"] = cmap_variant(name)
    elif name in CONV_VARIANTS:
        sc["conv_scale"], sc["conv_offset"] = CONV_VARIANTS[name]
        sc["conv_k"] = scene.folded_conv_scale(sc["conv_scale"], sc["dtype"])
    elif name in CAMERA_VARIANTS:
        kw = dict(yaw_deg=yaw, pitch_deg=20.0, voxel_world=vw)
        kw.update(CAMERA_VARIANTS[name])
        sc["cam"] = scene.orbit_camera(W, H, **kw)
        if name == "cam_tmax":
            sc["cam"].tmax = np.float32(TMAX_CUT)
    elif name in MODEL_VARIANTS:
        vol = sc["vol"]
        if name == "model_aniso":       # voxel sizes (vw, 2 vw, vw / 2), centred
            model = _model_rm((vw, 2 * vw, vw / 2), (-0.5, -1.0, -0.25))
        elif name == "model_rot30":     # the base brick turned 30 degrees about y
            model = _model_rm((vw, vw, vw), (-0.5, -0.5, -0.5), 30.0)
        elif name == "brick_1x1x1":     # one voxel filling the unit cube
            vol = np.full((1, 1, 1), 40000, vol.dtype)
            model = _model_rm((1.0, 1.0, 1.0), (-0.5, -0.5, -0.5))
        elif name == "brick_1x3x2":     # (z, y, x) = 1 x 3 x 2 voxels of 0.4
            vol = np.array([[[9000, 52000], [30000, 65535], [61000, 20000]]], dtype=vol.dtype)
            model = _model_rm((0.4, 0.4, 0.4), (-0.4, -0.6, -0.2))
        elif name == "brick_slab":      # 2 x 64 x 64: two z planes of the field (each voxel doubled along x and y),
            # stepped at the slab's voxel size and seen at a grazing angle from nearby, so that rays run a dozen
            # steps through the two planes and search (face-on they take two steps and settle in two passes)
            vol = np.ascontiguousarray(np.repeat(np.repeat(gray_scott_u16(n)[n // 2 - 1:n // 2 + 1], 2, axis=1), 2, axis=2))
            model = _model_rm((1.0 / 64, 1.0 / 64, 1.0 / 64), (-0.5, -0.5, -1.0 / 64))
            sc["cam"] = scene.orbit_camera(W, H, yaw_deg=80.0, pitch_deg=20.0, radius=1.0, voxel_world=1.0 / 64)
        elif name == "brick_nz1":       # one z plane at the base voxel size: a ray crosses it in under two steps and
            # its one sample sits at tnear, which AccumulateVDI.comp:1 (step > localNear) leaves out -- an empty VDI
            vol = np.ascontiguousarray(vol[n // 2:n // 2 + 1])
            model = _model_rm((vw, vw, vw), (-0.5, -0.5, -vw / 2))
        else:                           # brick_nz1_unit: one z plane of voxels 1 world unit wide, the eye above it
            vol = np.ascontiguousarray(vol[n // 2:n // 2 + 1])
            model = _model_rm((1.0, 1.0, 1.0), (-n / 2.0, -n / 2.0, -0.5))
        sc["vol"], sc["model"], sc["im"] = vol, model, scene.inverse_model(model)
    elif name in FIELD_VARIANTS:
        sc["vol"], sc["dtype"] = field_variant(name, n)
        sc["conv_k"] = scene.folded_conv_scale(sc["conv_scale"], sc["dtype"])
    else:
        raise ValueError(name)
    return sc


# The oracle on each variant at 64 x 48, S = 8 (u16 unless noted; u8 within one ray of it), as
# hit rays / searched rays (passes > 2) / largest pass count:
#   base 366/259/24
#   step 366/232/24, opaque 366/259/24, near_opaque 366/259/24, faint 366/79/24, comb 366/260/24,
#   out_of_range 366/250/24, tf_1texel 366/259/24, tf_2texel 366/240/16
#   dark 366/80/24, hdr 366/260/24, signed 366/257/24, big 366/260/24, huge 366/260/24, cmap_1texel 366/259/24,
#   cmap_2texel 366/259/24
#   conv_wide 366/234/24, conv_negative 366/232/24, conv_high 366/145/24
#   cam_inside 3072/3072/24, cam_near_cut 3072/3072/24, cam_wide 401/282/24, cam_pitch89 294/241/24,
#   cam_offcentre 763/537/24, cam_spv_half 366/170/24, cam_spv3 366/325/24, cam_tmax 323/171/24
#   model_aniso 485/335/24, model_rot30 312/243/24, brick_1x1x1 366/0/2, brick_1x3x2 236/118/13,
#   brick_slab 672/201/14, brick_nz1 169/0/2 (empty VDI), brick_nz1_unit 3072/3068/20
#   field_noise 366/260/24, field_const 366/0/2, field_checker 366/260/24, field_f32_range (f32) 366/237/24,
#   field_f32_nonfinite (f32) 366/259/24
ALL_VARIANTS = (TF_VARIANTS + CMAP_VARIANTS + tuple(CONV_VARIANTS) + tuple(CAMERA_VARIANTS) + MODEL_VARIANTS +
                FIELD_VARIANTS)


def lut_coordinate_fractions(sc):
    """Fractions of the voxels whose converted value raw = v * conv_k + conv_offset lies below 0 and above 1."""
    raw = sc["vol"].astype(np.float64) * float(sc["conv_k"]) + float(sc["conv_offset"])
    return float(np.mean(raw < 0.0)), float(np.mean(raw > 1.0))


def filter_constant(tf, cmap) -> float:
    """TransferDesc::cmag as insitu_set_transfer computes it: c = max(1, 2C, 2CA), inf from 1e6 on or for a
    non-finite LUT entry (the filtered decisions' error margin scales with it, insitu_filter.h)."""
    rgb = np.asarray(cmap, np.float64).reshape(-1, 4)[:, :3]
    a = np.asarray(tf, np.float64)
    if not (np.all(np.isfinite(rgb)) and np.all(np.isfinite(a))):
        return float("inf")
    C, A = float(np.abs(rgb).max()), float(np.abs(a).max())
    cb = max(1.0, 2.0 * C, 2.0 * C * A)
    return cb if cb < 1.0e6 else float("inf")


# variants whose rays mostly settle in the first two passes (nothing to search): everything else must search
NO_SEARCH_VARIANTS = ("brick_1x1x1", "brick_nz1", "field_const")
EXPECTED_FILTER_CONSTANT = {"base": 2.0, "dark": 1.0, "hdr": 16.0, "signed": 2.0, "big": 980000.0,
                            "huge": float("inf"), "out_of_range": 2.5, "faint": 2.0, "opaque": 2.0}


def check_variant_claims(name: str, sc, oracle_out, generate=None):
    """Assertions on the INPUTS and on the ORACLE's output (colour, depth, octree, passes of the whole frame)
    that variant `name` does what it is there for.  generate(sc) -> the oracle's output for another scene
    dict (only cam_tmax needs it)."""
    rc, rd, _, rp = oracle_out
    hit, searched = rp > 0, rp > 2
    if name in EXPECTED_FILTER_CONSTANT:
        c, want = filter_constant(sc["tf"], sc["cmap"]), EXPECTED_FILTER_CONSTANT[name]
        assert c == want or abs(c - want) <= 2e-3 * want, (name, c, want)   # (LUTs sample texel centres)
    if name not in NO_SEARCH_VARIANTS:
        assert np.count_nonzero(searched) >= 50, f"{name}: only {np.count_nonzero(searched)} rays search"
    if name == "opaque":
        assert np.count_nonzero(sc["tf"] == np.float32(1.0)) >= sc["tf"].size // 2 - 1
    elif name == "near_opaque":
        assert sc["tf"].max() == np.float32(1.0 - 2.0 ** -24) < np.float32(1.0)
    elif name == "out_of_range":
        assert sc["tf"].min() < 0.0 and sc["tf"].max() > 1.0
    elif name in CONV_VARIANTS:
        below, above = lut_coordinate_fractions(sc)
        assert above >= 0.05 and (below >= 0.05 or name == "conv_high"), (below, above)
    elif name in ("cam_inside", "cam_near_cut"):
        assert np.all(searched), "every ray starts inside the brick and searches"
        # the first sample is the ray's front, mix(wfront, wback, 0): NDC z = -1 (VDIGenerator.comp:305-320)
        assert np.all(np.abs(rd[..., 0] + 1.0) < 1e-5), "every list starts at the front of its ray"
    elif name == "cam_tmax":
        full = dict(sc, cam=variant_scene("base", sc["W"], sc["H"], sc["vol"].shape[0]).get("cam"))
        _, fd, _, fp = generate(full)
        both = hit & (fp > 0)
        last_cut, last_full = rd.max(axis=2).T[both], fd.max(axis=2).T[both]
        assert np.count_nonzero(last_cut < last_full) >= 50, "tmax must end rays inside the brick"
        assert np.count_nonzero(hit) < np.count_nonzero(fp > 0)
    elif name == "brick_nz1":
        assert np.count_nonzero(hit) > 0 and not np.any(rd) and not np.any(rc), "the oracle's VDI is empty"
    elif name == "field_const":
        # one supersegment per ray that has an in-brick sample, found in 2 passes.  A hit ray (tnear < tfar) of fewer
        # than two steps has none: its one sample sits at tnear, which AccumulateVDI.comp:1 (step > localNear) leaves
        # out, as for brick_nz1.  Which rays those are does not depend on the field: they are the rays that store
        # nothing under a constant alpha of 0.4 (tf_1texel) either.
        _, sd, _, _ = generate(dict(sc, vol=variant_scene("base", sc["W"], sc["H"])["vol"], tf=tf_variant("tf_1texel")))
        count = np.count_nonzero(rd[..., 0::2], axis=2)
        assert rp.max() == 2 and count.max() == 1 and np.array_equal(count == 1, sd[..., 0] != 0)
        assert 0 < np.count_nonzero(count) <= hit.sum()
    elif name == "field_f32_nonfinite":
        v = sc["vol"]
        assert np.isnan(v).any() and np.isposinf(v).any() and np.isneginf(v).any()
        assert np.all(np.isfinite(rc)) and np.all(np.isfinite(rd)), "the oracle's output is finite: bits compare"
    if name != "brick_nz1":
        assert np.count_nonzero(rd) > 0, "scene produced no supersegments"
