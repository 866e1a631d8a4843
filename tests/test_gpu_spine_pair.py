"""GPU parity of the paired spine machine and of the fast path of the adjusted opacity.

first_pass_impl counts spine levels 1 and 2 (thresholds 0.866 and 0.433) as ONE state machine while the two levels
decide alike, and splits them at the first sample one of them closes a supersegment on where the other does not
(count_sample_pair); march_pass / march_multi take det_pow_normal for a sample's adjusted opacity when its guard
holds for every lane of the wave.  Every case is one 32^3 brick at 64x48 (the merged cases: two), bit for bit
against the CPU oracle -- colour, depth, octree, pass counts -- and asserts first, on the oracle's output alone,
that the scene does what the case is there for.  What the pass count of a ray says about the levels (the search
walks the tree's "fewer" spine from pass 2 on: pass 2 is level 1, pass 3 level 2, ...):

  * a ray of 6 and more passes went "fewer" at levels 1 to 4: levels 1 and 2 closed alike wherever it mattered;
  * a ray that ends at 4 passes with 2 and more supersegments stored was accepted at level 2's threshold, which
    closed supersegments level 1 did not: its lanes split, in tiles whose other rays (5 and more passes) agree;
  * a ray that ends at 3 passes with 2 and more stored was accepted at level 1's threshold: level 1 closes too;
  * under the `big` colour map every threshold closes more than S: the machines stop at nterm > S, paired or split.
"""
from __future__ import annotations

import functools

import numpy as np
import pytest

import oracle_binding as orc
import scenes
from insitu_amd import native
from insitu_amd.renderer import InSituContext
from scenes import make_scene, variant_scene

pytestmark = pytest.mark.gpu

W, H = 64, 48
SECOND_ORIGIN = (0.0, -0.25, -0.75)   # the second volume of the merged cases, overlapping the first


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
def _oracle(name, S):
    """The oracle's sub-VDI (colour, depth, octree, passes) of scenes.variant_scene(name); shared, never modified."""
    return _frozen(orc.vdi_generate(_inputs(variant_scene(name, W, H)), W, H, S))


def _merged_scenes(name):
    """Two volumes for one sub-VDI: variant_scene(name) and a second brick with the same field, transfer function
    and colour map at SECOND_ORIGIN."""
    a = variant_scene(name, W, H)
    b = make_scene(n=32, W=W, H=H, yaw=40.0, origin=SECOND_ORIGIN)
    b["vol"], b["dtype"], b["conv_k"] = a["vol"], a["dtype"], a["conv_k"]
    return [a, b]


@functools.lru_cache(maxsize=None)
def _oracle_merged(name, S):
    scs = _merged_scenes(name)
    return _frozen(orc.vdi_generate_multi([_inputs(sc, scs[0]["cam"]) for sc in scs], W, H, S))


def _assert_sub_vdi(got, ref, what=""):
    (col, dep, octree, passes), (rc, rd, ro, rp) = got, ref
    bad = np.count_nonzero(_bits(col) != _bits(rc)) + np.count_nonzero(_bits(dep) != _bits(rd))
    if bad:
        where = np.argwhere(np.any(_bits(dep) != _bits(rd), axis=2) | np.any(_bits(col) != _bits(rc), axis=(2, 3)))
        raise AssertionError(f"{what}{bad} mismatching sub-VDI words; stored counts equal on "
                             f"{np.mean(_counts(dep) == _counts(rd)):.4f} of the pixels; first bad (x, y) {where[:5].tolist()}")
    assert np.array_equal(octree, ro), f"{what}octree cells differ"
    assert np.array_equal(passes.astype(np.int32), rp), f"{what}pass counts differ"


def _read_all(ctx):
    return (ctx.read(native.BUF_VDI_COLOR), ctx.read(native.BUF_VDI_DEPTH), ctx.read(native.BUF_OCTREE),
            ctx.read(native.BUF_PASSES))


def _render(sc, S, exact=0):
    with InSituContext(sc["W"], sc["H"], max_supersegments=S, keep_passes=True) as ctx:
        ctx.set_transfer(sc["tf"], sc["cmap"], sc["conv_scale"], sc["conv_offset"])
        ctx.set_option(native.OPT_EXACT_SEARCH, exact)
        ctx.set_brick(0, sc["vol"], sc["model"])
        ctx.render(sc["cam"])
        got, st = _read_all(ctx), ctx.stats()
    assert st["rays_searched"] > 0 and st["rays_uncached"] == 0, "the rays must take the first pass and the search kernel"
    return got


def _render_merged(scs, S):
    with InSituContext(W, H, max_supersegments=S, bricks_per_rank=2, keep_passes=True, merge_bricks=True) as ctx:
        ctx.set_transfer(scs[0]["tf"], scs[0]["cmap"], scs[0]["conv_scale"], scs[0]["conv_offset"])
        for b, sc in enumerate(scs):
            ctx.set_brick(b, sc["vol"], sc["model"])
        ctx.render(scs[0]["cam"])
        got, st = _read_all(ctx), ctx.stats()
    assert st["rays_searched"] > 0
    return got


def _accepted_at(ref, passes):
    """Rays (as a [y][x] mask) that end at `passes` passes with 2 and more supersegments stored."""
    _, rd, _, rp = ref
    return (rp == passes) & (_counts(rd).T >= 2)


def _tiles_with(mask_a, mask_b):
    """8x8 tiles that hold a ray of mask_a together with a ray of mask_b ([y][x] masks)."""
    ta = mask_a.reshape(H // 8, 8, W // 8, 8).any(axis=(1, 3))
    tb = mask_b.reshape(H // 8, 8, W // 8, 8).any(axis=(1, 3))
    return int(np.count_nonzero(ta & tb))


def _claim_level2_only(ref):
    split = _accepted_at(ref, 4)
    assert np.count_nonzero(split) >= 40, f"only {np.count_nonzero(split)} rays are accepted at level 2"
    mixed = _tiles_with(split, ref[3] >= 5)
    assert mixed >= 5, f"only {mixed} tiles hold a splitting ray beside rays that stay paired"


def _claim_level1(ref):
    n = np.count_nonzero(_accepted_at(ref, 3))
    assert n >= 20, f"only {n} rays are accepted at level 1"


LEVEL2_CASES = [("field_checker", 2), ("field_noise", 3)]
LEVEL1_CASES = [("hdr", 2), ("hdr", 4)]


def test_never_split():
    """The base scene at S = 20: every ray that searches takes 6 and more passes, so its levels 1 and 2 each go
    "fewer" with the one supersegment a ray has at those thresholds -- the pair holds from the first sample to the
    last.  (The other hit rays, 2 passes, are accepted at pass 1's threshold: nothing reads their levels.)"""
    S = 20
    ref = _oracle("base", S)
    rp = ref[3]
    assert np.count_nonzero(rp > 2) >= 100 and rp[rp > 2].min() >= 6, "a searching ray settles before level 5"
    _assert_sub_vdi(_render(variant_scene("base", W, H), S), ref)


@pytest.mark.parametrize("exact", [0, 1], ids=["filtered", "exact_search"])
@pytest.mark.parametrize("name,S", LEVEL2_CASES)
def test_level2_closes_where_level1_does_not(name, S, exact):
    ref = _oracle(name, S)
    _claim_level2_only(ref)
    _assert_sub_vdi(_render(variant_scene(name, W, H), S, exact), ref)


@pytest.mark.parametrize("exact", [0, 1], ids=["filtered", "exact_search"])
@pytest.mark.parametrize("name,S", LEVEL1_CASES)
def test_level1_closes_too(name, S, exact):
    ref = _oracle(name, S)
    _claim_level1(ref)
    _assert_sub_vdi(_render(variant_scene(name, W, H), S, exact), ref)


@pytest.mark.parametrize("S", [2, 4])
def test_machines_stopped_past_S(S):
    """The `big` colour map: neighbouring samples differ by more than any threshold, so every threshold closes more
    than S supersegments on a searching ray (it ends at 24 passes, the range closed) and every machine stops at
    nterm > S -- the pair as one, and after a split each level at its own sample."""
    ref = _oracle("big", S)
    rp = ref[3]
    assert np.count_nonzero(rp > 2) >= 50 and np.all(rp[rp > 2] == 24), "a searching ray ends before pass 24"
    _assert_sub_vdi(_render(variant_scene("big", W, H), S), ref)


def test_merged_volumes_split():
    """Two volumes of the checkerboard field in one sub-VDI at S = 2 (vdi_merge_kernel shares first_pass_impl; a step
    inside both volumes feeds two samples, the ray's last step two `last` ones)."""
    S = 2
    ref = _oracle_merged("field_checker", S)
    _claim_level2_only(ref)
    _assert_sub_vdi(_render_merged(_merged_scenes("field_checker"), S), ref)


def test_pipelined_pair_of_frames():
    """The checkerboard case as two pipelined frames and the flush: frame 1's first pass runs beside frame 0's search."""
    S = 2
    sc = variant_scene("field_checker", W, H)
    ref = _oracle("field_checker", S)
    _claim_level2_only(ref)
    seen = []
    with InSituContext(W, H, max_supersegments=S, keep_passes=True) as ctx:
        ctx.set_transfer(sc["tf"], sc["cmap"], sc["conv_scale"], sc["conv_offset"])
        ctx.set_brick(0, sc["vol"], sc["model"])
        for step in (lambda: ctx.frame_pipelined(sc["cam"], want_image=False),
                     lambda: ctx.frame_pipelined(sc["cam"], want_image=False),
                     lambda: ctx.pipeline_flush(want_image=False)):
            done, _ = step()
            if done >= 0:
                seen.append(done)
                _assert_sub_vdi(_read_all(ctx), ref, f"frame {done}: ")
    assert seen == [0, 1]


@pytest.mark.parametrize("name", ["opaque", "near_opaque", "out_of_range"])
def test_pow_guard_far_side_merged(name):
    """Transfer functions whose samples fail det_pow_normal's guard -- alpha exactly 1 (1 - a = 0), the largest
    float below 1 (a normal 1 - a: the guard holds at the edge of the table), alpha above 1 (1 - a < 0) -- through
    march_multi: two merged volumes at S = 4.  (The brick kernel under them: test_gpu_inputs.py.)"""
    S = 4
    scs = _merged_scenes(name)
    scenes.check_variant_claims(name, scs[0], _oracle(name, S))
    ref = _oracle_merged(name, S)
    assert np.count_nonzero(ref[3] > 2) >= 50, "the merged rays must search"
    _assert_sub_vdi(_render_merged(scs, S), ref)
