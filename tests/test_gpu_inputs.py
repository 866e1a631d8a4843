"""GPU parity off the default scene: the generator, the plain raymarch, the VDICompositor and the flatten on
inputs the other GPU tests never build (tests/scenes.py variants and synthetic supersegment lists).

Every comparison is bit for bit against the CPU oracle, as in tests/test_gpu_parity.py.  What the variants
exercise in the kernels:
  * the filter constant c = TransferDesc::cmag = max(1, 2C, 2CA) of insitu_filter.h at 1 (dark map), 2, 2.5,
    16 (hdr), 9.8e5 (just under the switch-off) and inf (exact decisions only) -- and the VDICompositor's
    per-pixel cpix at 1, 16 and inf; every case renders with filtered AND with exact decisions, and BOTH must
    equal the oracle (not only each other);
  * LUT coordinates below texel 0, past texel n - 1 and NaN (texel_pair_mm, the padded LDS LUTs), 1- and
    2-texel LUTs;
  * alpha exactly 1 (log2(1 - a) = -inf), one ulp below 1, below 0 and above 1;
  * rays that start inside the brick, rays cut by tmax, other step counts per ray (samples_per_voxel 0.5 and
    3: other chunk counts per ray), bricks of 1, 6 and 2 x 64 x 64 voxels, a brick no sample falls into;
  * general model matrices (anisotropic voxels, a rotation);
  * white noise, constant, checkerboard and non-finite fields;
  * the in-place search of vdi_march (sample_cache_mb = -1) and a cache that holds only some waves.
A test asserts nothing about the kernels' output other than equality with the oracle; what it asserts beyond
that is about its inputs, the oracle's output or which path ran (scenes.check_variant_claims).

Loop bounds for the non-finite and out-of-range inputs (NaN / inf voxels, alpha outside [0, 1], colours of
2e6, inf / NaN entry colours): every loop these values reach ends on an integer count that no float
comparison feeds.  Generator: a pass walks i < numSteps (march_pass) or k < n cached samples with k advanced
by a select on integers (search_loop); numSteps comes from the camera and the model matrix only and is < 65536
for every cached ray; a ray ends after at most 64 passes (q.iter, incremented every pass and every free_walk
step; vdi_march breaks at q.iter > 64).  Compositor: a pass consumes one list entry per step or at most one
gap before it (rem[j] counts down, e runs to nent), the terminal sample (end depth 0) always stops it, and the
search leaves at q.iter > 64; the interval walk increments q.iter per step.  Depths are finite in every case,
so NaN reaches decisions (`diff >= threshold`, false for NaN on both sides) but never a loop condition.
"""
from __future__ import annotations

import numpy as np
import pytest

import oracle_binding as orc
import scenes
from insitu_amd import native
from insitu_amd.renderer import InSituContext

pytestmark = pytest.mark.gpu

W, H, S = 64, 48, 8
_ORACLE: dict = {}


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _inputs(sc):
    return orc.Inputs(sc["vol"], sc["im"], sc["tf"], sc["cmap"], sc["conv_k"], sc["conv_offset"], sc["cam"])


def _generate(sc, S_=S):
    return orc.vdi_generate(_inputs(sc), sc["W"], sc["H"], S_)


def _case(name, dtype="u16", w=W, h=H):
    """The variant's scene and the oracle's VDI of it, computed once per module."""
    key = (name, dtype, w, h)
    if key not in _ORACLE:
        sc = scenes.variant_scene(name, w, h, dtype=dtype)
        _ORACLE[key] = (sc, _generate(sc))
    return _ORACLE[key]


def _assert_vdi_equal(got, ref, what):
    for g, r, part in zip(got, ref, ("colour", "depth", "octree", "passes")):
        g, r = np.ascontiguousarray(g), np.ascontiguousarray(r)
        if g.dtype == np.float32:
            bad = _bits(g) != _bits(r)
        else:
            bad = g.astype(np.int64) != r.astype(np.int64)
        if np.any(bad):
            where = np.argwhere(bad)
            raise AssertionError(f"{what}: {part} differs in {np.count_nonzero(bad)} words, first at "
                                 f"{where[:4].tolist()}: got {g[tuple(where[0])]!r}, oracle {r[tuple(where[0])]!r}")


def _render_both_searches(sc, ref, what, cache_mb=0):
    """Two renders in one context, filtered (OPT_EXACT_SEARCH 0) then exact (1): each equals the oracle."""
    with InSituContext(sc["W"], sc["H"], max_supersegments=S, keep_passes=True, sample_cache_mb=cache_mb) as ctx:
        ctx.set_transfer(sc["tf"], sc["cmap"], sc["conv_scale"], sc["conv_offset"])
        ctx.set_brick(0, sc["vol"], sc["model"])
        stats = []
        for exact in (0, 1):
            ctx.set_option(native.OPT_EXACT_SEARCH, exact)
            ctx.render(sc["cam"])
            got = [ctx.read(b) for b in (native.BUF_VDI_COLOR, native.BUF_VDI_DEPTH, native.BUF_OCTREE, native.BUF_PASSES)]
            stats.append(ctx.stats())
            _assert_vdi_equal(got, ref, f"{what}, exact_search={exact}")
    return stats


_GEN_CASES = [(n, "u16") for n in ("base",) + scenes.ALL_VARIANTS] + [(n, "u8") for n in scenes.CONV_VARIANTS]


@pytest.mark.parametrize("name,dtype", _GEN_CASES, ids=[f"{n}-{d}" for n, d in _GEN_CASES])
def test_vdi_generate_variant_bit_exact(name, dtype):
    """One changed input per case; colour, depth, octree and pass counts of the filtered and of the exact search
    equal the oracle's.  (The f32 field cases carry their own dtype; the conversion cases also run in u8, whose
    conv_k folds in the 1/255.)"""
    sc, ref = _case(name, dtype)
    scenes.check_variant_claims(name, sc, ref, _generate)
    _render_both_searches(sc, ref, f"{name}/{dtype}")


@pytest.mark.parametrize("name", ["cam_inside", "cam_spv3", "opaque", "huge"])
def test_vdi_generate_variant_uncached(name):
    """sample_cache_mb = -1: every ray runs its whole search in the sampling kernel (vdi_march), re-sampling the
    brick every pass; rendered with OPT_EXACT_SEARCH 0 and 1 like every other case (vdi_march itself decides
    exactly either way)."""
    sc, ref = _case(name)
    stats = _render_both_searches(sc, ref, f"{name}, no cache", cache_mb=-1)
    assert all(st["rays_uncached"] > 0 and st["rays_searched"] == 0 for st in stats)


def test_vdi_generate_inside_camera_partial_cache():
    """The inside camera at 96 x 80 with a 1-MiB cache: every ray is long, some waves get cache space and replay,
    the rest search in place."""
    sc, ref = _case("cam_inside", "u16", 96, 80)
    assert np.all(ref[3] > 2)
    stats = _render_both_searches(sc, ref, "cam_inside 96x80, 1 MiB cache", cache_mb=1)
    assert all(st["rays_uncached"] > 0 and st["rays_searched"] > 0 for st in stats)


_PLAIN_CASES = ([(n, "u16") for n in scenes.TF_VARIANTS + scenes.CMAP_VARIANTS + tuple(scenes.CONV_VARIANTS) +
                 scenes.FIELD_VARIANTS + ("fwnw",)] + [(n, "u8") for n in scenes.CONV_VARIANTS])


@pytest.mark.parametrize("name,dtype", _PLAIN_CASES, ids=[f"{n}-{d}" for n, d in _PLAIN_CASES])
def test_plain_variant_bit_exact(name, dtype):
    """MODE_PLAIN at 40 x 40 on the same transfer functions, colour maps, conversions and fields, and with the
    growing step of VolumeRaycaster.comp:132-139 (fwnw = 0.002): rgba8 colour and encoded depth equal the
    oracle's plain raycast."""
    dim = 40
    sc = scenes.variant_scene("base" if name == "fwnw" else name, dim, dim, dtype=dtype)
    if name == "fwnw":
        sc["cam"].fwnw = np.float32(0.002)
    rc, rd = orc.plain_raycast(_inputs(sc), dim, dim)
    assert np.count_nonzero(rc[..., 3]) > 0
    with InSituContext(dim, dim, mode=native.MODE_PLAIN) as ctx:
        ctx.set_transfer(sc["tf"], sc["cmap"], sc["conv_scale"], sc["conv_offset"])
        ctx.set_brick(0, sc["vol"], sc["model"])
        img = ctx.frame(sc["cam"], want_image=True)
        col = ctx.read(native.BUF_PLAIN_COLOR)
        dep = ctx.read(native.BUF_PLAIN_DEPTH)
    assert np.array_equal(col, rc), f"{np.count_nonzero(np.any(col != rc, axis=2))} pixels differ"
    assert np.array_equal(dep, rd)
    assert np.array_equal(img, orc.plain_composite([rc], [rd], dim))


# ---------------------------------------------------------------- VDICompositor and flatten on synthetic lists
LS = 6   # supersegments per input list


def _lists():
    """Two random lists (test_vdi_pack.random_vdi: lengths 0..S, depths in (0.9, 0.99)) and the generating
    camera whose inverse view-projection places them."""
    if "lists" not in _ORACLE:
        from test_vdi_pack import random_vdi
        cam = scenes.variant_scene("base", W, H)["cam"]
        _ORACLE["lists"] = (random_vdi(W, H, LS, 21), random_vdi(W, H, LS, 22), cam, orc.ipv_of(cam))
    return _ORACLE["lists"]


def _list_variant(name):
    """One list of the compositor cases, as (colour (W,H,S,4), depth (W,H,2S)) float32."""
    (col, dep), _, _, _ = _lists()
    col, dep = col.copy(), dep.copy()
    live = dep[..., 0::2] != 0
    rng = np.random.default_rng(5)
    if name == "random":
        pass
    elif name == "zero_length":      # every entry ends where it starts
        dep[..., 1::2] = dep[..., 0::2]
    elif name == "alpha_0_or_1":
        col[..., 3] = np.where(rng.random(live.shape) < 0.5, 0.0, 1.0) * live
    elif name == "rgb_x8":           # cpix = 16; alpha untouched
        col[..., :3] *= np.float32(8.0)
    elif name == "rgb_x3e6":         # cpix = inf: exact decisions only
        col[..., :3] *= np.float32(3e6)
    elif name == "nonfinite":        # a few inf / -inf / NaN colour components (alpha among them)
        idx = np.argwhere(live)
        pick = idx[rng.choice(len(idx), 60, replace=False)]
        vals = np.array([np.inf, -np.inf, np.nan], np.float32)
        for k, (x, y, i) in enumerate(pick):
            col[x, y, i, rng.integers(0, 4)] = vals[k % 3]
    else:
        raise ValueError(name)
    return col, dep


def _assert_lists_equal(got_c, got_d, ref_c, ref_d, what, nan_masks=False):
    for g, r, part in ((got_c, ref_c, "colour"), (got_d, ref_d, "depth")):
        g, r = np.ascontiguousarray(g), np.ascontiguousarray(r)
        bad = _bits(g) != _bits(r)
        if nan_masks:   # NaN payloads are not part of the contract: the masks must agree, the rest bit for bit
            assert np.array_equal(np.isnan(g), np.isnan(r)), f"{what}: {part} NaN masks differ"
            bad &= ~np.isnan(r)
        assert not np.any(bad), f"{what}: {part} differs in {np.count_nonzero(bad)} words, first {np.argwhere(bad)[:4].tolist()}"


@pytest.mark.parametrize("name,S_out", [("random", 4), ("random", 12), ("zero_length", 4), ("alpha_0_or_1", 4),
                                        ("rgb_x8", 4), ("rgb_x3e6", 4), ("nonfinite", 4)])
def test_vdi_compositor_one_list(name, S_out):
    """One host list through distributeVDIs -> VDICompositor -> gatherCompositedVDISet / gatherCompositedVDIs:
    composited colour, depth and pass counts with filtered and with exact decisions equal orc.vdi_composite, the
    image of a third frame (the merge cache grown to the demand) equals the flatten of the composited VDI, and a
    context without the compositor flattens the list itself."""
    _, _, cam, ipv = _lists()
    col, dep = _list_variant(name)
    oc, od, op = orc.vdi_composite([col], [dep], W, H, 0, W, ipv, S_out)
    nanm = name == "nonfinite"
    assert nanm or (np.all(np.isfinite(oc)) and np.all(np.isfinite(od)))
    assert np.count_nonzero(od) > 0 and op.max() > 4
    size = H * W * LS * 4
    with InSituContext(W, H, max_supersegments=LS, composite_vdi=True, max_output_supersegments=S_out,
                       keep_passes=True) as ctx:
        ctx.set_camera(cam)
        for exact in (0, 1):
            ctx.set_option(native.OPT_EXACT_SEARCH, exact)
            ctx.distributeVDIs(col, dep, size, 1, recv=False)
            gc, gd = ctx.gatherCompositedVDISet(H * W * S_out * 4, 0, 0, 1)
            _assert_lists_equal(gc, gd, oc, od, f"{name}, exact_search={exact}", nanm)
            assert np.array_equal(ctx.read(native.BUF_COMPOSITE_PASSES).astype(np.int32), op), f"passes, exact={exact}"
        ctx.set_option(native.OPT_EXACT_SEARCH, 0)
        ctx.distributeVDIs(col, dep, size, 1, recv=False)
        img = ctx.gatherCompositedVDIs(0, H * W * 4, 0, 1)
    assert np.array_equal(img, orc.vdi_flatten([oc], [od], W, H, 0, W, ipv))
    with InSituContext(W, H, max_supersegments=LS) as ctx:
        ctx.set_camera(cam)
        ctx.distributeVDIs(col, dep, size, 1, recv=False)
        img = ctx.gatherCompositedVDIs(0, H * W * 4, 0, 1)
    assert np.array_equal(img, orc.vdi_flatten([col], [dep], W, H, 0, W, ipv))


def _harness(tmp_path, kind, subs, S_out):
    import test_c_harness as th
    th._need_harness()
    _, _, cam, _ = _lists()
    sc = dict(scenes.variant_scene("base", W, H), cam=cam)
    th._write_common(tmp_path, sc, W, H, LS, S_out)
    for r, (c, d) in enumerate(subs):
        (tmp_path / f"sub_col_{r}.bin").write_bytes(np.ascontiguousarray(c, np.float32).tobytes())
        (tmp_path / f"sub_dep_{r}.bin").write_bytes(np.ascontiguousarray(d, np.float32).tobytes())
    th._run(kind, tmp_path, len(subs))


def _harness_lists(name):
    """The lists of a harness case, one per rank: two random ones; a list and its exact copy (every start depth
    ties); both with rgb x 8; a zero-length list and its copy (ties between entries that end where they start);
    four lists -- three random ones and a copy of the first, so ties cross lists 0 and 3 with two others merged
    in between."""
    a, b, _, _ = _lists()
    if name == "two_random":
        return [a, b]
    if name == "copy":
        return [a, (a[0].copy(), a[1].copy())]
    if name == "rgb_x8":
        return [_list_variant("rgb_x8"), (b[0] * np.float32([8, 8, 8, 1]), b[1])]
    if name == "zero_length_copy":
        z = _list_variant("zero_length")
        return [z, (z[0].copy(), z[1].copy())]
    if name == "four_lists":
        from test_vdi_pack import random_vdi
        return [a, b, random_vdi(W, H, LS, 23), (a[0].copy(), a[1].copy())]
    raise ValueError(name)


@pytest.mark.timeout(300)
@pytest.mark.parametrize("name,S_out", [("two_random", 4), ("two_random", 12), ("copy", 4), ("rgb_x8", 4),
                                        ("zero_length_copy", 4), ("four_lists", 4)])
def test_vdi_compositor_lists_c_harness(tmp_path, name, S_out):
    """Two or four lists, one per rank of the C harness (tests/c_harness, unchanged): the gathered composited VDI
    equals orc.vdi_composite of them all.  Where lists tie on a start depth the merge order must be the oracle's
    (lowest list first)."""
    subs = _harness_lists(name)
    ipv = _lists()[3]
    oc, od, op = orc.vdi_composite([c for c, _ in subs], [d for _, d in subs], W, H, 0, W, ipv, S_out)
    assert np.count_nonzero(od) > 0 and op.max() > 8
    if name in ("copy", "zero_length_copy", "four_lists"):
        assert np.array_equal(subs[0][1], subs[-1][1]) and np.count_nonzero(subs[0][1]) > 0
    if name == "zero_length_copy":
        assert np.array_equal(subs[0][1][..., 0::2], subs[0][1][..., 1::2])
    _harness(tmp_path, "cvdi", subs, S_out)
    gc = np.fromfile(tmp_path / "gcol.bin", np.float32).reshape(oc.shape)
    gd = np.fromfile(tmp_path / "gdep.bin", np.float32).reshape(od.shape)
    _assert_lists_equal(gc, gd, oc, od, name)


@pytest.mark.timeout(300)
@pytest.mark.parametrize("name", ["two_random", "copy", "zero_length_copy", "four_lists"])
def test_vdi_flatten_lists_c_harness(tmp_path, name):
    """The same lists flattened by the root (no compositor): the image equals orc.vdi_flatten of them all."""
    subs = _harness_lists(name)
    ipv = _lists()[3]
    want = orc.vdi_flatten([c for c, _ in subs], [d for _, d in subs], W, H, 0, W, ipv)
    # (entries of length zero have adjusted alpha 1 - (1 - a)^0 = 0: their flatten is legitimately empty)
    assert (np.count_nonzero(want[..., 3]) > 0) == (name != "zero_length_copy")
    _harness(tmp_path, "vdi", subs, 0)
    img = np.fromfile(tmp_path / "image.bin", np.uint8).reshape(H, W, 4)
    assert np.array_equal(img, want)
