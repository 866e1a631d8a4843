"""The merged VDI of a set without a GPU: vdi_io.merge_vdis against a plain per-pixel loop
written here -- bit for bit, the overlap count included -- over oracle VDIs of bricks that overlap in space and of
abutting bricks of a domain decomposition; the merged VDI seen from the generating camera against the oracle's
flatten of the same lists; crafted lists (ties, entries behind a zero start, empty pixels, empty sets); slabs against
their analytic image; the limit of 255 slots; and the new entry point with a null context.
loop_merge, SCENE_SETS and scene_set are shared with tests/test_gpu_view_merge.py."""
from __future__ import annotations

import numpy as np
import pytest

import oracle_binding as orc
import view_binding as vb
from insitu_amd import native, vdi_io
from insitu_amd.vdi_io import merge_vdis
from scenes import make_scene

W, H, S = vb.VDI_W, vb.VDI_H, vb.VDI_S
G = vb.gen_camera()
CAMS = vb.view_cameras()
LSB = 1.0   # the project's image tolerance, as tests/test_view_ref.py

# name -> (brick edge in voxels, brick edge in world units, ((origin, seed), ...)); every voxel is 1/32 world units
SCENE_SETS = {
    "overlapping_pair": (32, 1.0, (((-0.5, -0.5, -0.5), 1000), ((0.0, -0.25, -0.75), 7))),   # test_gpu_view's _scenes()
    "abutting_pair": (24, 0.75, (((-0.75, -0.375, -0.375), 1000), ((0.0, -0.375, -0.375), 7))),
    "abutting_2x2": (16, 0.5, (((-0.5, -0.5, -0.25), 1000), ((0.0, -0.5, -0.25), 7), ((-0.5, 0.0, -0.25), 11),
                               ((0.0, 0.0, -0.25), 13))),
}


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def scene_set(name, w=W, h=H):
    n, world, bricks = SCENE_SETS[name]
    return [make_scene(n=n, W=w, H=h, seed=seed, origin=origin, world=world) for origin, seed in bricks]


def loop_merge(cols, deps):
    """The definition, pixel by pixel: repeatedly the front with the smallest start depth, scanning the lists in
    ascending order with a strict `<` from 100000; a list ends at a zero start.  -> (colour (W,H,S_m,4), depth
    (W,H,2 S_m), overlaps)."""
    n = len(cols)
    w, h, s = cols[0].shape[:3]
    starts = [np.asarray(d, np.float32)[:, :, 0::2].tolist() for d in deps]
    picks = {}
    for x in range(w):
        for y in range(h):
            at = [0] * n
            out = []
            while True:
                low, idx = 100000.0, -1
                for j in range(n):
                    if at[j] < s:
                        c = starts[j][x][y][at[j]]
                        if c != 0.0 and c < low:
                            low, idx = c, j
                if idx < 0:
                    break
                out.append((idx, at[idx]))
                at[idx] += 1
            picks[(x, y)] = out
    s_m = max(1, max(len(p) for p in picks.values()))
    col = np.zeros((w, h, s_m, 4), np.float32)
    dep = np.zeros((w, h, 2 * s_m), np.float32)
    overlaps = 0
    for (x, y), out in picks.items():
        for k, (j, i) in enumerate(out):
            col[x, y, k] = cols[j][x, y, i]
            dep[x, y, 2 * k:2 * k + 2] = deps[j][x, y, 2 * i:2 * i + 2]
            if k and dep[x, y, 2 * k] < dep[x, y, 2 * k - 1]:
                overlaps += 1
    return col, dep, overlaps


def _same_vdi(got, want, what):
    assert got[0].shape == want[0].shape and got[1].shape == want[1].shape, what
    assert np.array_equal(_bits(got[0]), _bits(want[0])), what
    assert np.array_equal(_bits(got[1]), _bits(want[1])), what
    assert got[2] == want[2], what


_ORACLE = {}


def oracle_set(name):
    """(colours, depths, the loop's merge) of a scene set from the oracle, once."""
    if name not in _ORACLE:
        cols, deps = [], []
        for sc in scene_set(name):
            inp = orc.Inputs(sc["vol"], sc["im"], sc["tf"], sc["cmap"], sc["conv_k"], sc["conv_offset"], G)
            c, d, _, _ = orc.vdi_generate(inp, W, H, S)
            cols.append(c)
            deps.append(d)
        _ORACLE[name] = (cols, deps, loop_merge(cols, deps))
    return _ORACLE[name]


@pytest.mark.parametrize("name", list(SCENE_SETS))
def test_merge_vdis_equals_the_loop(name):
    cols, deps, want = oracle_set(name)
    got = merge_vdis(cols, deps)
    _same_vdi(got, want, name)
    shared = np.sum([np.any(d[:, :, 0::2] != 0.0, axis=2) for d in deps], axis=0) >= 2
    print(f"{name}: S_m {got[0].shape[2]}, {int(shared.sum())} pixels with two or more non-empty lists, "
          f"{got[2]} overlapping neighbours")
    assert shared.sum() >= 50
    if name.startswith("abutting"):
        assert got[2] == 0
    else:
        assert got[2] > 0


@pytest.mark.parametrize("name", list(SCENE_SETS))
def test_generating_camera_equals_flatten(name):
    """The merged VDI seen from the generating camera at its own size is the flatten of the lists it was merged
    from, within the bound of test_same_camera_equals_flatten: 1 LSB per channel."""
    cols, deps, (mc, md, _) = oracle_set(name)
    img, _ = vb.render(mc, md, G, G, W, H)
    flat = orc.vdi_flatten(cols, deps, W, H, 0, W, orc.ipv_of(G))
    diff = np.abs(img.astype(np.int32) - flat.astype(np.int32))
    print(f"{name}: merged view against the flatten: at most {int(diff.max())} LSB, {int(np.count_nonzero(diff))} "
          f"channels differ")
    assert flat[..., 3].max() > 0
    assert diff.max() <= 1


def _crafted():
    """Three 16x8, S = 4 VDIs; the colour of entry i of list j is (j, i, 0, 0.5).
    x < 6: lists 0 and 2 both start at 0.2 -- expected order (0,0) (2,0) (1,0) (2,1) (0,1).
    6 <= x < 12: list 1 holds 0.1, a zero start, then 0.3 and 0.4 behind it; list 0 holds 0.25.
    x >= 12: empty in every list."""
    cols = [np.zeros((16, 8, 4, 4), np.float32) for _ in range(3)]
    deps = [np.zeros((16, 8, 8), np.float32) for _ in range(3)]

    def put(j, xs, starts):
        for i, z in enumerate(starts):
            if z:
                cols[j][xs, :, i] = (j, i, 0.0, 0.5)
                deps[j][xs, :, 2 * i:2 * i + 2] = (z, z + 0.05)

    put(0, slice(0, 6), [0.2, 0.5])
    put(1, slice(0, 6), [0.3])
    put(2, slice(0, 6), [0.2, 0.4])
    put(0, slice(6, 12), [0.25])
    put(1, slice(6, 12), [0.1, 0.0, 0.3, 0.4])
    return cols, deps


def test_crafted_lists():
    cols, deps = _crafted()
    got = merge_vdis(cols, deps)
    _same_vdi(got, loop_merge(cols, deps), "crafted")
    mc, md, _ = got
    assert mc.shape == (16, 8, 5, 4)
    assert mc[2, 3, :, :2].tolist() == [[0, 0], [2, 0], [1, 0], [2, 1], [0, 1]]    # the tie: list 0 before list 2
    assert md[2, 3, 0::2].tolist() == [np.float32(z) for z in (0.2, 0.2, 0.3, 0.4, 0.5)]
    assert mc[8, 1, :, :2].tolist() == [[1, 0], [0, 0], [0, 0], [0, 0], [0, 0]]    # nothing from behind the zero
    assert md[8, 1, 0::2].tolist() == [np.float32(0.1), np.float32(0.25), 0.0, 0.0, 0.0]
    assert not md[12:].any() and not mc[12:].any()                                   # empty in every list
    # an all-empty set: one slot, nothing in it
    ec, ed = [np.zeros_like(c) for c in cols], [np.zeros_like(d) for d in deps]
    c0, d0, ov = merge_vdis(ec, ed)
    assert c0.shape == (16, 8, 1, 4) and d0.shape == (16, 8, 2) and not c0.any() and not d0.any() and ov == 0
    _same_vdi((c0, d0, ov), loop_merge(ec, ed), "empty set")
    # lists without entries change nothing, wherever they stand
    more = merge_vdis([ec[0], cols[0], cols[1], ec[1], cols[2], ec[2]], [ed[0], deps[0], deps[1], ed[1], deps[2], ed[2]])
    _same_vdi(more, got, "with empty lists in between")
    _same_vdi(merge_vdis(cols[:1], deps[:1]), loop_merge(cols[:1], deps[:1]), "a set of one")


A_SLAB, B_SLAB = [(0.9715, 0.9760, (1.0, 0.0, 0.0, 0.4)), (0.9760, 0.9799, (0.0, 0.0, 1.0, 0.6))]


def test_slabs_merge_to_the_two_layer_vdi():
    both = vb.slab_vdi([A_SLAB, B_SLAB])
    want = (both[0][:, :, :2], both[1][:, :, :4], 0)
    a, b = vb.slab_vdi([A_SLAB]), vb.slab_vdi([B_SLAB])
    ab = merge_vdis([a[0], b[0]], [a[1], b[1]])
    ba = merge_vdis([b[0], a[0]], [b[1], a[1]])
    _same_vdi(ab, want, "A then B")
    _same_vdi(ba, want, "B then A")
    w, h = vb.OUT_SIZES[0]
    for name, cam in CAMS.items():
        img, _ = vb.render(ab[0], ab[1], G, cam, w, h)
        err = vb.lsb_error(img, vb.analytic_slabs([A_SLAB, B_SLAB], G, cam, w, h))
        print(f"merged slabs {name}: {err:.3f} LSB")
        assert err <= LSB


def test_slot_limit():
    a = vb.layered_vdi(128, 16, 8)
    b = vb.layered_vdi(127, 16, 8, 128)
    mc, md, _ = merge_vdis([a[0], b[0]], [a[1], b[1]])
    assert mc.shape == (16, 8, 255, 4) and np.all(md[:, :, 0::2] != 0.0)
    with pytest.raises(ValueError, match="256"):
        merge_vdis([a[0], a[0]], [a[1], a[1]])


def test_null_context_and_export():
    lib = native.load()
    assert "insitu_view_bind_host_set" in native.EXPORTED_SYMBOLS
    assert lib.insitu_view_bind_host_set(None, None, None, 2, 16, 8, 4, None) == -1
    assert native.VIEW_MERGED == 2 and vdi_io.MERGE_MAX_LISTS == 32
