"""GPU parity of vdi_search_kernel under the two scheduling knobs no other test moves off their defaults:
INSITU_OPT_LONG_SAMPLES (which end of the two-ended search queue a ray is appended to) and INSITU_OPT_ROUND_BATCH
(how many finished lanes end a round of a one-lane-per-ray wave).  Neither changes what a ray computes, so every case
is bit for bit the CPU oracle's sub-VDI, octree cells and pass counts; what the cases add is the proof, from CPU data
alone, that the code they aim at runs.

pr.n and numSteps.  A ray's step count is numSteps = trunc((tfar - tnear) / nw) (ray_setup, vdi_generate.hip:121; the
`num_steps` of pyref.vdi_pixel).  The first pass caches one sample per step i < numSteps whose ray parameter
step_i = tnear + nw + ... + nw (a running binary32 sum) lies strictly inside (localNear, localFar)
(march_pass, :524/:535), counts them in k, and queues the ray with pr.n = k (first_pass_impl, :918/:961).  With the eye
outside the brick tnear == localNear, so step 0 is not inside and pr.n = numSteps - 1; _ray_steps() replays the
running sum with pyref's binary32 arithmetic instead of relying on that, and every scene below asserts
pr.n == numSteps - 1 for all its queued rays.  sample_tile (:1185, :1212) queues every ray with tnear < tfar and
1 <= numSteps < 65536 that found cache space -- also the rays of one step (pr.n = 0) and the rays pass 1 settles --
so rays_searched == count(passes > 0 and numSteps >= 1) whenever rays_uncached == 0, the oracle's pass count being
positive exactly where tnear < tfar.  A ray is "long" when pr.n >= LONG_SAMPLES (:1223).

Class sizes (long + short = queued rays) at the 25th / 50th / 75th percentile of pr.n over the queued rays, from
_ray_steps() (asserted again by the tests, at least 64 = one wave per class):

  deep    make_scene(n=32, 72x56, yaw=120), S=12: 472 queued of 486 hit, pr.n 0..39;
          T=8: 358+114, T=18: 237+235, T=30: 123+349
  ragged  n=24, 50x37, yaw=75, S=5, the camera at radius 2.0 (at the default 3.5 only 192 rays are queued and a
          quartile class is 44 rays, less than a wave): 615 queued of 636 hit, pr.n 0..27;
          T=6: 481+134, T=16: 319+296, T=23: 219+396
  big3    the deep scene under the `big` colour map at S=3: the same 472 rays, 2 or 24 passes each
  trio    three separate bricks (the scenes of test_merged_volumes_one_vdi_bit_exact) at 96x80, S=8: 2381 queued
          of 2485 hit; T=12 (the median): 1231+1150
  pipe    two bricks at 96x80, S=8, three cameras (tests/test_gpu_pipeline.py): T=19 (frame 0's median);
          frame 0: 1009+929, frame 1: 1144+914, frame 2: 1316+698
  merged  the trio merged into one sub-VDI at 64x48 and 50x37: vdi_merge_kernel queues every ray from the front
          (:1062), LONG_SAMPLES is not read; 630 and 373 queued rays
  far     n=32 at 64x48 from radius 14: 23 hit rays, all queued, 18 of them searching -- fewer than one wave
  overflow  n=32 at 96x80, 5 samples per voxel: 985 rays to search, pr.n up to 203; their waves ask for 43648 cache
          chunks of 32 bytes, at most 3264 each, of the 32768 a 1 MiB cache has (at 1 sample per voxel, the scene of
          test_vdi_sample_cache_off_and_overflow, they ask for 9024 and all fit)

Which lines of vdi_generate.hip each group is aimed at:

  test_long_samples_sweep, test_queue_*     the two append indices of sample_tile (:1226-1233: the long rays'
      queue_count from the front, the short rays' queue_cap - 1 - (queue_short + ...) from the back), the search's
      qlong / qlen (:1352-1353) and its pop mapping r < qlong ? r : queue_cap - 1 - (r - qlong) (:1488), with
      queue_cap = BV * W * H for one brick, three bricks and merged volumes (vdi_gen_params, insitu_hip.cpp)
  test_queue_shorter_than_a_wave            the pop's base + cnt >= qlen (:1477) and r < qlen (:1488) inside one claim
  test_round_batch*                         the round-end ballot (:1671-1677) with ROUND_BATCH 1 (a lane never waits),
      28 and 64 (a finished lane waits with k >= n while any lane of its wave replays: the `on = k < n` selects of
      INSITU_REPLAY_SEL (:1620-1638) and the `if (k < n)` of INSITU_REPLAY (:1646) leave its state alone), regroup's
      `hold` lanes (:1552) in the same ballot, and emit's nseg >= S branch (:1603) with the early k = n exit (:1637)
  test_two_renders_*, test_pipelined_*, test_small_cache_*    the counters zeroed per render, the pipelined search's
      block count (:1358-1364) and drain flag (:1477-1483), and waves that queue nothing (:1199-1219)
  test_env_*                                the INSITU_* seeds of insitu_create (seed_options over the option table,
      insitu_context.cpp)
"""
from __future__ import annotations

import functools

import numpy as np
import pytest

import oracle_binding as orc
import pyref
from insitu_amd import native, scene
from insitu_amd.renderer import InSituContext
from scenes import make_scene, variant_scene

# (the search kernel's own guard against a logic error ends a wave after 10 s and raises the fault flag)
pytestmark = [pytest.mark.gpu, pytest.mark.timeout(45)]

ALL_LONG, ALL_SHORT = 0, 0xffffffff
WAVE = 64


# ---------------------------------------------------------------- scenes, shared and never modified
@functools.lru_cache(maxsize=None)
def _scene(name):
    """(bricks as make_scene dicts, camera, S) of the named case; W, H, LUTs and conversion are bricks[0]'s."""
    if name == "deep":       # the tree-depth test's scene: rays of more than 8 passes
        sc = make_scene(n=32, W=72, H=56, yaw=120.0)
        return (sc,), sc["cam"], 12
    if name == "ragged":     # W, H off the 8-grid; from radius 2.0, so that a quartile of the queue is more than a wave
        sc = make_scene(n=24, W=50, H=37, yaw=75.0)
        return (sc,), scene.orbit_camera(50, 37, radius=2.0, yaw_deg=75.0, pitch_deg=20.0, voxel_world=1.0 / 24), 5
    if name == "big3":       # rgb up to 4.9e5: no threshold merges neighbours, write passes close more than S = 3
        sc = variant_scene("big", 72, 56, yaw=120.0)
        return (sc,), sc["cam"], 3
    if name == "far":        # the brick seen from far away: fewer hit pixels than a wave has lanes
        sc = make_scene(n=32, W=64, H=48, yaw=30.0)
        return (sc,), scene.orbit_camera(64, 48, radius=14.0, yaw_deg=30.0, pitch_deg=20.0, voxel_world=1.0 / 32), 8
    if name == "overflow":   # test_vdi_sample_cache_off_and_overflow's at 5 samples per voxel: at 1 its rays need
        # 282 KiB of sample cache, which a 1 MiB cache holds
        sc = make_scene(n=32, W=96, H=80, yaw=30.0, samples_per_voxel=5.0)
        return (sc,), sc["cam"], 8
    if name.startswith("trio"):   # the bricks of test_merged_volumes_one_vdi_bit_exact
        W, H = {"trio": (96, 80), "trio_small": (64, 48), "trio_ragged": (50, 37)}[name]
        scs = (make_scene(n=24, W=W, H=H, yaw=35.0),
               make_scene(n=24, W=W, H=H, yaw=35.0, seed=7, origin=(0.0, -0.25, -0.75)),
               make_scene(n=16, W=W, H=H, yaw=35.0, seed=9, origin=(-0.7, 0.1, 0.2), world=0.6))
        return scs, scs[0]["cam"], 8
    if name.startswith("pipe"):   # tests/test_gpu_pipeline.py's two bricks, under its camera number name[4]
        W, H = 96, 80
        scs = (make_scene(n=32, W=W, H=H, origin=(-0.5, -0.5, -0.5)),
               make_scene(n=32, W=W, H=H, seed=7, origin=(0.0, -0.25, -0.75)))
        i = int(name[4:])
        cam = scene.orbit_camera(W, H, yaw_deg=30.0 + 37.0 * i, pitch_deg=20.0 - 9.0 * i, voxel_world=1.0 / 32)
        return scs, cam, 8
    raise ValueError(name)


def _frozen(arrays):
    for a in arrays:
        a.setflags(write=False)
    return tuple(arrays)


def _inputs(sc, cam):
    return orc.Inputs(sc["vol"], sc["im"], sc["tf"], sc["cmap"], sc["conv_k"], sc["conv_offset"], cam)


@functools.lru_cache(maxsize=None)
def _oracle(name):
    """Per brick the oracle's (colour, depth, octree, passes)."""
    scs, cam, S = _scene(name)
    W, H = scs[0]["W"], scs[0]["H"]
    return tuple(_frozen(orc.vdi_generate(_inputs(sc, cam), W, H, S)) for sc in scs)


@functools.lru_cache(maxsize=None)
def _oracle_merged(name):
    scs, cam, S = _scene(name)
    return _frozen(orc.vdi_generate_multi([_inputs(sc, cam) for sc in scs], scs[0]["W"], scs[0]["H"], S))


# ---------------------------------------------------------------- the rays' step counts, on the CPU
def _ray_steps(sc, cam):
    """Per pixel [y][x] of one brick, in pyref's binary32 arithmetic: tnear < tfar (`hit`), numSteps
    (ray_setup; pyref.vdi_pixel's num_steps), the in-brick samples the first pass caches (pr.n: march_pass's running
    sum step += nw tested against (localNear, localFar)), and the brick's interval (max(0, n), f) of a hit ray."""
    W, H = sc["W"], sc["H"]
    vol = sc["vol"]
    V = pyref.Volume([], (vol.shape[2], vol.shape[1], vol.shape[0]), sc["im"].tolist(), [], [], 1.0, 0.0)
    ipv = pyref.matmul(cam.inv_view.tolist(), cam.inv_proj.tolist())
    nw, tmax = pyref.r32(float(cam.nw)), pyref.r32(float(cam.tmax))
    hit = np.zeros((H, W), bool)
    steps = np.zeros((H, W), np.int64)
    samples = np.zeros((H, W), np.int64)
    near = np.ones((H, W), np.float64)
    far = np.zeros((H, W), np.float64)
    for gy in range(H):
        for gx in range(W):
            _, _, wfront, wback = pyref._ray(ipv, gx, gy, W, H)
            n, f = V.intersect(wfront, wback)
            f = pyref.gmin(tmax, f)
            if not n < f:
                continue
            tnear, tfar = pyref.gmin(1.0, pyref.gmax(0.0, n)), pyref.gmax(0.0, f)
            near[gy, gx], far[gy, gx] = pyref.gmax(0.0, n), f
            if not tnear < tfar:
                continue
            hit[gy, gx] = True
            steps[gy, gx] = int(pyref.div(pyref.sub(tfar, tnear), nw))
            step, k = tnear, 0
            for _ in range(int(steps[gy, gx])):
                k += n < step < f
                step = pyref.add(step, nw)
            samples[gy, gx] = k
    return _frozen((hit, steps, samples, near, far))


@functools.lru_cache(maxsize=None)
def _steps(name):
    """_ray_steps of every brick of the named case."""
    scs, cam, _ = _scene(name)
    return tuple(_ray_steps(sc, cam) for sc in scs)


def _queued(hit, steps):
    """The rays sample_tile / vdi_merge_kernel queue when every ray finds cache space."""
    return hit & (steps >= 1) & (steps < 65536)


def _queue_samples(name):
    """pr.n of every queued ray of the case (all bricks), checked against the oracle's pass counts: a ray has
    passes > 0 exactly where the CPU data says tnear < tfar."""
    out = []
    for (hit, steps, samples, _, _), ref in zip(_steps(name), _oracle(name)):
        assert np.array_equal(hit, ref[3] > 0), "CPU ray setup and the oracle's pass counts disagree on the hit rays"
        q = _queued(hit, steps)
        assert np.array_equal(samples[q], steps[q] - 1), "pr.n == numSteps - 1 with the eye outside the brick"
        out.append(samples[q])
    return np.concatenate(out)


def _classes(n, T):
    """(long, short) rays of a queue with sample counts n under LONG_SAMPLES = T."""
    return int(np.count_nonzero(n >= T)), int(np.count_nonzero(n < T))


def _percentile_thresholds(name, which=(25, 50, 75)):
    """LONG_SAMPLES values at percentiles of pr.n over the queued rays; both classes hold more than one wave."""
    n = _queue_samples(name)
    out = []
    for p in which:
        T = int(np.percentile(n, p))
        lng, sht = _classes(n, T)
        assert lng >= WAVE and sht >= WAVE, f"{name}: LONG_SAMPLES {T} (p{p}) gives {lng} long and {sht} short rays"
        out.append(T)
    return out


def _merged_steps(name):
    """(hit, numSteps) per pixel of the case's bricks merged into one ray (multi_ray_setup: the union of the
    volumes' intervals)."""
    scs, cam, _ = _scene(name)
    per = _steps(name)
    nw = pyref.r32(float(cam.nw))
    near = np.minimum(1.0, np.minimum.reduce([p[3] for p in per]))
    far = np.maximum(0.0, np.maximum.reduce([p[4] for p in per]))
    hit = near < far
    steps = np.zeros(hit.shape, np.int64)
    for y, x in np.argwhere(hit):
        steps[y, x] = int(pyref.div(pyref.sub(float(far[y, x]), float(near[y, x])), nw))
    return hit, steps


# ---------------------------------------------------------------- rendering and comparing
def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _read(ctx, b=0):
    return (ctx.read(native.BUF_VDI_COLOR, b), ctx.read(native.BUF_VDI_DEPTH, b), ctx.read(native.BUF_OCTREE, b),
            ctx.read(native.BUF_PASSES, b))


def _assert_sub_vdi(got, ref, what=""):
    (col, dep, octree, passes), (rc, rd, ro, rp) = got, ref
    bad = np.count_nonzero(_bits(col) != _bits(rc)) + np.count_nonzero(_bits(dep) != _bits(rd))
    if bad:
        where = np.argwhere(np.any(_bits(dep) != _bits(rd), axis=2) | np.any(_bits(col) != _bits(rc), axis=(2, 3)))
        raise AssertionError(f"{what}: {bad} mismatching sub-VDI words; first bad (x, y) {where[:5].tolist()}")
    assert np.array_equal(octree, ro), f"{what}: octree cells differ"
    assert np.array_equal(passes.astype(np.int32), rp), f"{what}: pass counts differ"


def _context(name, merge=False, cache_mb=0):
    scs, _, S = _scene(name)
    sc = scs[0]
    ctx = InSituContext(sc["W"], sc["H"], max_supersegments=S, bricks_per_rank=len(scs), keep_passes=True,
                        merge_bricks=merge, sample_cache_mb=cache_mb)
    ctx.set_transfer(sc["tf"], sc["cmap"], sc["conv_scale"], sc["conv_offset"])
    for b, s in enumerate(scs):
        ctx.set_brick(b, s["vol"], s["model"])
    return ctx


def _render_check(ctx, name, what, merge=False):
    """One render of the case's camera: every sub-VDI equals the oracle's; returns the stats."""
    scs, cam, _ = _scene(name)
    ctx.render(cam)
    if merge:
        _assert_sub_vdi(_read(ctx), _oracle_merged(name), what)
    else:
        for b, ref in enumerate(_oracle(name)):
            _assert_sub_vdi(_read(ctx, b), ref, f"{what}, brick {b}")
    return ctx.stats()


def _run(name, options, what, merge=False, cache_mb=0):
    with _context(name, merge, cache_mb) as ctx:
        for opt, val in options:
            ctx.set_option(opt, val)
        return _render_check(ctx, name, what, merge)


def _assert_all_searched(st, expect, what):
    assert st["rays_uncached"] == 0, f"{what}: {st['rays_uncached']} rays without cache space"
    assert st["rays_searched"] == expect > 0, f"{what}: {st['rays_searched']} rays searched, {expect} queued on the CPU"


# ---------------------------------------------------------------- 1. both queue classes
@pytest.mark.parametrize("depth,regroup", [(0, 1), (1, 0), (1, 1)])
@pytest.mark.parametrize("name", ["deep", "ragged"])
def test_long_samples_sweep(name, depth, regroup):
    """LONG_SAMPLES at 0 (every queued ray long, queue_short stays 0), 0xffffffff (every ray short) and the three
    quartiles of pr.n (both classes larger than a wave, from the CPU's step counts): the same sub-VDI, octree cells
    and pass counts as the oracle, and the same number of searched rays -- the rays the first pass's rule queues.
    depth 0: the kernel's own choice (tree groups); 1: one lane per ray, where ROUND_BATCH and the regroup act."""
    n = _queue_samples(name)
    if name == "deep":
        assert _oracle(name)[0][3].max() > 8, "scene needs rays with a long search"
    for T in [ALL_LONG, ALL_SHORT] + _percentile_thresholds(name):
        what = f"{name}, LONG_SAMPLES {T}"
        st = _run(name, [(native.OPT_LONG_SAMPLES, T), (native.OPT_SEARCH_DEPTH, depth), (native.OPT_REGROUP, regroup)], what)
        _assert_all_searched(st, n.size, what)
        if depth == 1:
            assert (st["search_regroups"] > 0) == bool(regroup), (what, st["search_regroups"])


# ---------------------------------------------------------------- 2. queue_cap beyond one brick
def test_queue_three_bricks():
    """Three separate bricks at 96x80: queue_cap = 3 W H, the short rays of all three descend from the far end of the
    three-brick queue while the long ones ascend from its front."""
    n = _queue_samples("trio")
    for T in [ALL_LONG] + _percentile_thresholds("trio", (50,)):
        what = f"3 bricks, LONG_SAMPLES {T}"
        _assert_all_searched(_run("trio", [(native.OPT_LONG_SAMPLES, T)], what), n.size, what)


@pytest.mark.parametrize("name,depth", [("trio_small", 0), ("trio_small", 1), ("trio_ragged", 1)])
def test_queue_merged_volumes(name, depth):
    """merge_bricks: BV = 1 while B = 3, queue_cap = W H, the search's MERGED instantiation -- against the oracle's
    multi-volume restatement, also at tree depth 1 and on a window off the 8-grid.  vdi_merge_kernel appends every ray
    at the front, whatever LONG_SAMPLES says: the pop must find all of them below qlong."""
    hit, steps = _merged_steps(name)
    rp = _oracle_merged(name)[3]
    assert np.array_equal(hit, rp > 0), "CPU ray setup and the oracle's pass counts disagree on the hit rays"
    q = _queued(hit, steps)
    assert np.count_nonzero(rp > 2) >= WAVE, "the merged rays must search"
    for T in (ALL_LONG, int(np.percentile(steps[q], 50))):
        what = f"{name}, depth {depth}, LONG_SAMPLES {T}"
        st = _run(name, [(native.OPT_LONG_SAMPLES, T), (native.OPT_SEARCH_DEPTH, depth)], what, merge=True)
        _assert_all_searched(st, int(np.count_nonzero(q)), what)


@pytest.mark.parametrize("depth", [0, 1])
@pytest.mark.parametrize("T", [ALL_LONG, ALL_SHORT])
def test_queue_shorter_than_a_wave(T, depth):
    """A brick so far away that fewer pixels hit it than a wave has lanes, all long or all short: with one lane per
    ray (depth 1) the first claim asks for 64 rays of a shorter queue, so base + cnt >= qlen and r < qlen decide
    inside that one claim; with tree groups a few claims drain it."""
    rp = _oracle("far")[0][3]
    n = _queue_samples("far")
    assert 0 < n.size <= np.count_nonzero(rp > 0) < WAVE, np.count_nonzero(rp > 0)
    assert np.count_nonzero(rp > 2) > 0, "some of the rays must search"
    what = f"far brick, depth {depth}, LONG_SAMPLES {T}"
    st = _run("far", [(native.OPT_LONG_SAMPLES, T), (native.OPT_SEARCH_DEPTH, depth)], what)
    _assert_all_searched(st, n.size, what)


# ---------------------------------------------------------------- 3. ROUND_BATCH
def _assert_lanes_finish_apart(name, pass_kinds):
    """The rays of the case differ in length and in passes (at least pass_kinds different counts), so the lanes of a
    wave finish their passes at different trips: with ROUND_BATCH 64 the early ones wait, with 1 none does."""
    n = _queue_samples(name)
    rp = _oracle(name)[0][3]
    assert np.unique(n).size >= 16 and n.size > 4 * WAVE, "the queue needs rays of many different lengths"
    assert np.unique(rp[rp > 0]).size >= pass_kinds, "the rays need different numbers of passes"


@pytest.mark.parametrize("exact", [0, 1])
@pytest.mark.parametrize("regroup", [0, 1])
@pytest.mark.parametrize("batch", [1, 28, 64])
def test_round_batch(batch, regroup, exact):
    """One lane per ray (SEARCH_DEPTH 1), where ROUND_BATCH is read: every finished lane ends its round alone (1),
    the default (28), every finished lane waits until no lane of its wave replays (64) -- with the select form
    (filtered) and the branching form (EXACT_SEARCH) of the replay, with and without the regroup's holding lanes."""
    _assert_lanes_finish_apart("deep", 8)
    what = f"ROUND_BATCH {batch}, regroup {regroup}, exact {exact}"
    st = _run("deep", [(native.OPT_SEARCH_DEPTH, 1), (native.OPT_ROUND_BATCH, batch), (native.OPT_REGROUP, regroup),
                       (native.OPT_EXACT_SEARCH, exact)], what)
    _assert_all_searched(st, _queue_samples("deep").size, what)
    assert (st["search_regroups"] > 0) == bool(regroup), (what, st["search_regroups"])


@pytest.mark.parametrize("exact", [0, 1])
@pytest.mark.parametrize("batch", [1, 64])
def test_round_batch_overflowing_passes(batch, exact):
    """S = 3 under the `big` colour map: search passes close more than S supersegments and leave early (k = n), and
    the write pass of a ray whose search never finds S or fewer closes more than it stores (emit's nseg >= S branch)
    -- while the other lanes of the wave wait (64) or never do (1)."""
    (sc,), cam, S = _scene("big3")
    _assert_lanes_finish_apart("big3", 2)   # (2 passes: settled by pass 1; 24: the range closed)
    _, rd, _, rp = _oracle("big3")[0]
    cnt = np.count_nonzero(rd[..., 0::2] != 0, axis=2).T   # [y][x]
    assert np.count_nonzero(rp > 2) >= WAVE, "pass 1 must close more than S supersegments on many rays"
    over = np.argwhere((cnt == S) & (rp == rp.max()))
    assert len(over) >= WAVE and rp.max() == 24, "rays whose search ends with the range closed"
    y, x = over[0]
    vol = sc["vol"]
    V = pyref.Volume(vol.ravel().tolist(), (vol.shape[2], vol.shape[1], vol.shape[0]), sc["im"].tolist(),
                     sc["tf"].tolist(), sc["cmap"].tolist(), float(sc["conv_k"]), float(sc["conv_offset"]))
    pcam = dict(view=cam.view.tolist(), proj=cam.proj.tolist(), inv_view=cam.inv_view.tolist(),
                inv_proj=cam.inv_proj.tolist(), nw=float(cam.nw), fwnw=float(cam.fwnw), tmax=float(cam.tmax))
    written, _, passes = pyref.vdi_pixel(V, pcam, int(x), int(y), sc["W"], sc["H"], S)
    assert passes == rp[y, x] and len(written) > S, f"pixel ({x}, {y}) closes {len(written)} supersegments"
    what = f"S = 3, ROUND_BATCH {batch}, exact {exact}"
    st = _run("big3", [(native.OPT_SEARCH_DEPTH, 1), (native.OPT_ROUND_BATCH, batch), (native.OPT_EXACT_SEARCH, exact)], what)
    _assert_all_searched(st, _queue_samples("big3").size, what)


def test_round_batch_inert_with_tree_groups():
    """Tree groups (SEARCH_DEPTH 0: the kernel's choice, G > 1) end their rounds by kGroupBatch: ROUND_BATCH 1
    changes neither the result nor the pass counts."""
    what = "depth 0, ROUND_BATCH 1"
    _assert_all_searched(_run("deep", [(native.OPT_ROUND_BATCH, 1)], what), _queue_samples("deep").size, what)


# ---------------------------------------------------------------- 4. with the paths that share the queue
def test_two_renders_changing_long_samples():
    """Renders in one context with LONG_SAMPLES going 0 -> median -> 0xffffffff -> 0: each reuses the queue and
    starts from zeroed counters, so a stale queue_count or queue_short would pop records of the render before."""
    n = _queue_samples("deep")
    (median,) = _percentile_thresholds("deep", (50,))
    with _context("deep") as ctx:
        ctx.set_option(native.OPT_SEARCH_DEPTH, 1)
        for T in (ALL_LONG, median, ALL_SHORT, ALL_LONG):
            ctx.set_option(native.OPT_LONG_SAMPLES, T)
            what = f"render with LONG_SAMPLES {T}"
            _assert_all_searched(_render_check(ctx, "deep", what), n.size, what)


@pytest.mark.parametrize("search_rays", [0, 1 << 24])
def test_pipelined_frames_two_queue_ends(search_rays):
    """Three pipelined frames and the flush, PIPE_TRIGGER 1 (the claim that drains the queue starts the next frame's
    first pass), LONG_SAMPLES at frame 0's median, every frame with both classes larger than a wave; with the full
    search grid (0) and with PIPE_SEARCH_RAYS so large that only the minimum of blocks searches and the others
    return at once (1 << 24).  Every completed frame equals the oracle's."""
    names = ["pipe0", "pipe1", "pipe2"]
    (T,) = _percentile_thresholds(names[0], (50,))
    for name in names:
        lng, sht = _classes(_queue_samples(name), T)
        assert lng >= WAVE and sht >= WAVE, (name, lng, sht)
    seen = []
    with _context(names[0]) as ctx:
        ctx.set_option(native.OPT_PIPE_TRIGGER, 1)
        ctx.set_option(native.OPT_PIPE_SEARCH_RAYS, search_rays)
        ctx.set_option(native.OPT_LONG_SAMPLES, T)
        calls = [functools.partial(ctx.frame_pipelined, _scene(name)[1], want_image=True) for name in names]
        calls.append(functools.partial(ctx.pipeline_flush, want_image=True))
        for call in calls:
            done, img = call()
            if done < 0:
                continue
            seen.append(done)
            refs = _oracle(names[done])
            for b, ref in enumerate(refs):
                _assert_sub_vdi(_read(ctx, b), ref, f"frame {done}, brick {b}")
            cam = _scene(names[done])[1]
            want = orc.vdi_flatten([r[0] for r in refs], [r[1] for r in refs], 96, 80, 0, 96, orc.ipv_of(cam))
            assert np.array_equal(img, want), f"frame {done}: image differs"
            st = ctx.stats()
            assert st["pipelined"] == 1
            _assert_all_searched(st, _queue_samples(names[done]).size, f"frame {done}")
    assert seen == [0, 1, 2]


def test_small_cache_waves_queue_nothing():
    """A 1 MiB cache at 96x80 with LONG_SAMPLES 0: the waves that find no cache space queue nothing and search their
    rays in place, the others append to the front only.  Asserted instead of rays_uncached == 0: both kinds of wave
    occur, and together they account for every ray the first pass's rule names."""
    n = _queue_samples("overflow")
    # sample_tile (:1185-1197): a wave takes 64 x its longest ray's chunks of 4 samples (32 bytes each) with one
    # atomic add, and gets them when they end inside the cache.  The first wave to ask gets its space if any wave's
    # request fits; once the requests add up to more than the cache some wave gets none.
    hit, steps, _, _, _ = _steps("overflow")[0]
    need = np.where(_queued(hit, steps), (steps + 3) >> 2, 0)
    H, W = need.shape
    per_wave = 64 * need.reshape(H // 8, 8, W // 8, 8).max(axis=(1, 3))
    cache_chunks = (1 << 20) // 32
    assert per_wave.sum() > cache_chunks >= per_wave.max(), (per_wave.sum(), per_wave.max())
    st = _run("overflow", [(native.OPT_LONG_SAMPLES, ALL_LONG)], "1 MiB cache", cache_mb=1)
    assert st["cache_bytes"] == 1 << 20
    assert st["rays_uncached"] > 0 and st["rays_searched"] > 0, st
    assert st["rays_uncached"] + st["rays_searched"] == n.size, (st["rays_uncached"], st["rays_searched"], n.size)


# ---------------------------------------------------------------- 5. environment seeds
# every INSITU_* seed of insitu_create with a value outside its option's range (include/insitu_hip.h)
_ENV_OUT_OF_RANGE = [
    ("INSITU_EXACT_SEARCH", "2"), ("INSITU_SEARCH_DEPTH", "7"), ("INSITU_LONG_SAMPLES", "-1"),
    ("INSITU_ROUND_BATCH", "65"), ("INSITU_SEARCH_OVERSUB", "0"), ("INSITU_TILE_ORDER", "2"),
    ("INSITU_SUPER_TILE", "3"), ("INSITU_REGROUP", "-1"), ("INSITU_EXACT_TILE_KEYS", "2"),
    ("INSITU_PIPE_TRIGGER", "3"), ("INSITU_PIPE_OVERSUB", "65"), ("INSITU_PIPE_SEARCH_RAYS", "16777217"),
    ("INSITU_VIEW_SKIP", "2"), ("INSITU_VIEW_COMPACT", "-1")]


@pytest.mark.parametrize("var,value", _ENV_OUT_OF_RANGE)
def test_env_seed_out_of_range(monkeypatch, var, value):
    """insitu_create refuses an out-of-range INSITU_* seed, whichever of the 14 it is, and names the variable and
    the value."""
    monkeypatch.setenv(var, value)
    sc = make_scene(n=16, W=32, H=24)
    with pytest.raises(RuntimeError, match=f"insitu_create: {var}={value} out of range$"):
        InSituContext(sc["W"], sc["H"], max_supersegments=4)


def test_env_seeds_and_override(monkeypatch):
    """INSITU_SEARCH_DEPTH=1 and INSITU_REGROUP=0 seed the options of a new context (one lane per ray, no regroup);
    insitu_set_option afterwards overrides the seed; without the variables the same options, set by hand to depth 1,
    regroup (the default leaves small frames at the deepest tree, where no regroup is possible)."""
    expect = _queue_samples("deep").size
    monkeypatch.setenv("INSITU_REGROUP", "0")
    monkeypatch.setenv("INSITU_SEARCH_DEPTH", "1")
    with _context("deep") as ctx:
        st = _render_check(ctx, "deep", "seeded from the environment")
        _assert_all_searched(st, expect, "seeded from the environment")
        assert st["search_regroups"] == 0
        ctx.set_option(native.OPT_REGROUP, 1)
        st = _render_check(ctx, "deep", "seed overridden")
        _assert_all_searched(st, expect, "seed overridden")
        assert st["search_regroups"] > 0, "insitu_set_option must override INSITU_REGROUP"
    monkeypatch.delenv("INSITU_REGROUP")
    monkeypatch.delenv("INSITU_SEARCH_DEPTH")
    st = _run("deep", [(native.OPT_SEARCH_DEPTH, 1)], "no variables")
    _assert_all_searched(st, expect, "no variables")
    assert st["search_regroups"] > 0
