"""The packed VDI stream without a GPU: the numpy codec of insitu_amd/vdi_io.py -- round
trips bit for bit, the size formula, the header, determinism, every rejection -- the host half of
insitu_view_bind_packed (csrc/vdi_pack_format.h through the stand-alone tests/pack_format_host.cpp: header parsing,
size arithmetic, the integer binary16 conversions against numpy), and the new entry points with a null context.
random_vdi and rejected_streams are shared with tests/test_gpu_view_pack.py."""
from __future__ import annotations

import ctypes
import struct
import subprocess
from pathlib import Path

import numpy as np
import pytest

import view_binding as vb
from insitu_amd import native, vdi_io
from insitu_amd.vdi_io import PACK_FLOAT, PACK_HALF, pack_vdi, unpack_vdi

ROOT = Path(__file__).resolve().parent.parent
PV = np.arange(16, dtype=np.float32) * np.float32(0.37) - np.float32(2.0)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def random_vdi(W: int, H: int, S: int, seed: int):
    """A reference-layout VDI with list lengths uniform in 0..S, depths strictly increasing inside (0.9, 0.99) and
    colours in [0, 1), a quarter of them below 6e-5, where binary16 is subnormal."""
    rng = np.random.default_rng(seed)
    counts = rng.integers(0, S + 1, size=(W, H))
    k = np.arange(2 * S, dtype=np.float64)
    dep = (0.9 + 0.09 * (k + rng.uniform(0.05, 0.95, size=(W, H, 2 * S))) / (2 * S + 1)).astype(np.float32)
    assert np.all(np.diff(dep, axis=2) > 0) and dep.min() > 0.9 and dep.max() < 0.99
    col = rng.random(size=(W, H, S, 4), dtype=np.float32)
    col *= np.where(rng.random(size=col.shape) < 0.25, np.float32(6e-5), np.float32(1.0)).astype(np.float32)
    live = np.arange(S)[None, None, :] < counts[:, :, None]
    return col * live[..., None], dep * np.repeat(live, 2, axis=2)


def empty_vdi(W=12, H=5, S=3):
    return np.zeros((W, H, S, 4), np.float32), np.zeros((W, H, 2 * S), np.float32)


def _cases():
    return {
        "list_ends": vb.list_end_vdi(),
        "empty": empty_vdi(),
        "9x7_S1": vb.slab_vdi(vb.SLAB, 9, 7, 1),
        "random": random_vdi(37, 21, 5, 11),
        "random_S2": random_vdi(70, 33, 2, 12),
    }


CASES = _cases()


def _entries(dep):
    return int(np.cumprod(dep[:, :, 0::2] != 0.0, axis=2).sum())


@pytest.mark.parametrize("name", list(CASES))
def test_float_round_trip_is_exact(name):
    col, dep = CASES[name]
    buf = pack_vdi(col, dep, PV, PACK_FLOAT)
    c, d, pv, fmt = unpack_vdi(buf)
    tc, td = vb.truncate_lists(col, dep)
    assert fmt == PACK_FLOAT and c.shape == col.shape and d.shape == dep.shape
    assert np.array_equal(_bits(c), _bits(tc)) and np.array_equal(_bits(d), _bits(td))
    assert np.array_equal(_bits(pv), _bits(PV))
    assert np.array_equal(buf, pack_vdi(col, dep, PV, PACK_FLOAT))   # deterministic
    assert np.array_equal(buf, pack_vdi(c, d, pv, PACK_FLOAT))       # and idempotent
    assert np.array_equal(unpack_vdi(buf.tobytes())[0], c)           # bytes are taken too


@pytest.mark.parametrize("name", list(CASES))
def test_half_round_trip_is_the_quantiser(name):
    col, dep = CASES[name]
    buf = pack_vdi(col, dep, PV, PACK_HALF)
    c, d, _, fmt = unpack_vdi(buf)
    tc, td = vb.truncate_lists(col, dep)
    assert fmt == PACK_HALF
    assert np.array_equal(_bits(d), _bits(td))
    assert np.array_equal(_bits(c), _bits(tc.astype(np.float16).astype(np.float32)))
    assert np.array_equal(pack_vdi(c, d, PV, PACK_HALF), buf)        # a half stream repacked as half is unchanged


def test_random_vdi_reaches_subnormal_halves():
    col, dep = CASES["random"]
    h = col[col > 0].astype(np.float16)
    sub = (h.view(np.uint16) & 0x7c00) == 0
    assert np.count_nonzero(sub) > 100 and np.count_nonzero(~sub) > 100
    counts = np.cumprod(dep[:, :, 0::2] != 0.0, axis=2).sum(axis=2)
    assert set(np.unique(counts)) == set(range(6))


@pytest.mark.parametrize("fmt", [PACK_FLOAT, PACK_HALF])
@pytest.mark.parametrize("name", list(CASES))
def test_size_and_header(name, fmt):
    col, dep = CASES[name]
    W, H, S = col.shape[:3]
    E = _entries(dep)
    buf = pack_vdi(col, dep, PV, fmt)
    assert buf.dtype == np.uint8 and buf.ndim == 1
    assert buf.size == 128 + (W * H + 15) // 16 * 16 + 8 * E + (8 if fmt == PACK_HALF else 16) * E
    raw = buf.tobytes()
    assert raw[:4] == b"IVDP"
    assert struct.unpack_from("<5I", raw, 4) == (1, fmt, W, H, S)
    assert struct.unpack_from("<Q", raw, 24) == (E,)
    assert struct.unpack_from("<16f", raw, 32) == tuple(float(v) for v in PV)
    assert raw[96:128] == bytes(32)
    counts = np.frombuffer(raw, np.uint8, W * H, 128).reshape(H, W)
    assert np.array_equal(counts.T, np.cumprod(dep[:, :, 0::2] != 0.0, axis=2).sum(axis=2))
    assert raw[128 + W * H:128 + (W * H + 15) // 16 * 16] == bytes((-W * H) % 16)
    if name == "empty":
        assert E == 0 and buf.size == 128 + 64


def test_entry_order_is_row_major_lists_first_to_last():
    col, dep = random_vdi(5, 3, 4, 5)
    raw = pack_vdi(col, dep, PV, PACK_FLOAT)
    counts = np.cumprod(dep[:, :, 0::2] != 0.0, axis=2).sum(axis=2)
    want_d, want_c = [], []
    for y in range(3):
        for x in range(5):
            for i in range(counts[x, y]):
                want_d.append(dep[x, y, 2 * i:2 * i + 2])
                want_c.append(col[x, y, i])
    E = len(want_d)
    d0 = 128 + 16
    assert np.array_equal(raw[d0:d0 + 8 * E].view(np.float32).reshape(E, 2), np.array(want_d))
    assert np.array_equal(raw[d0 + 8 * E:].view(np.float32).reshape(E, 4), np.array(want_c))


def test_files(tmp_path):
    col, dep = CASES["random"]
    p = vdi_io.write_packed(tmp_path / "vdi.ivdp", col, dep, PV, PACK_HALF)
    assert p.stat().st_size == pack_vdi(col, dep, PV, PACK_HALF).size
    c, d, pv, fmt = vdi_io.read_packed(p)
    assert fmt == PACK_HALF and np.array_equal(_bits(d), _bits(dep)) and np.array_equal(pv, PV)
    assert np.array_equal(c, col.astype(np.float16).astype(np.float32))


def rejected_streams() -> dict:
    """Streams that must be rejected, each one change away from a good 16x8, S = 6 stream (list_end_vdi: counts 0,
    2, 3 and 6).  The last three pass every host check: only the counts themselves tell."""
    col, dep = vb.list_end_vdi()
    good = pack_vdi(col, dep, PV, PACK_FLOAT)
    W, H, S = col.shape[:3]
    counts = good[128:128 + W * H]
    full, short = int(np.flatnonzero(counts == S)[0]), int(np.flatnonzero(counts == 3)[0])

    def edit(off, fmt, value):
        b = good.copy()
        b[off:off + struct.calcsize(fmt)] = np.frombuffer(struct.pack(fmt, value), np.uint8)
        return b

    def with_counts(changes):
        b = good.copy()
        for p, n in changes:
            b[128 + p] = n
        return b

    return {
        "bad magic": edit(0, "<4s", b"IVDQ"),
        "version 2": edit(4, "<I", 2),
        "format 2": edit(8, "<I", 2),
        "S = 0": edit(20, "<I", 0),
        "S = 256": edit(20, "<I", 256),
        "one byte short": good[:-1].copy(),
        "one byte long": np.concatenate([good, np.zeros(1, np.uint8)]),
        "a count above S, the sum kept": with_counts([(full, S + 1), (short, 2)]),
        "counts that add up to less than E": with_counts([(short, 2)]),
        "counts that add up to more than E": with_counts([(short, 4)]),
    }


@pytest.mark.parametrize("name", list(rejected_streams()))
def test_rejections(name):
    with pytest.raises(ValueError):
        unpack_vdi(rejected_streams()[name])


def test_pack_rejects_bad_arguments():
    col, dep = CASES["random"]
    for args in ((col, dep[:, :, :-1], PV, PACK_FLOAT), (col, dep, PV[:15], PACK_FLOAT), (col, dep, PV, 2),
                 (np.zeros((2, 2, 256, 4), np.float32), np.zeros((2, 2, 512), np.float32), PV, PACK_FLOAT)):
        with pytest.raises(ValueError):
            pack_vdi(*args)


def test_null_context_calls_fail():
    lib = native.load()
    assert native.PACK_FLOAT == PACK_FLOAT == 0 and native.PACK_HALF == PACK_HALF == 1
    assert lib.insitu_view_pack_bytes(None, 0) == 0
    n = ctypes.c_size_t(7)
    buf = np.zeros(16, np.uint8)
    assert lib.insitu_view_pack(None, 0, buf.ctypes.data, buf.nbytes, ctypes.byref(n)) == -1
    assert lib.insitu_view_bind_packed(None, buf.ctypes.data, buf.nbytes) == -1
    assert n.value == 7 and not buf.any()
    assert "ms_pack" in dict(native.Stats._fields_)


# ---------------------------------------------------------------- the host half of insitu_view_bind_packed
@pytest.fixture(scope="module")
def format_host(tmp_path_factory):
    exe = tmp_path_factory.mktemp("pf") / "pack_format_host"
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", str(ROOT / "scenery-insitu_amd" / "csrc"),
                    str(ROOT / "tests" / "pack_format_host.cpp"), "-o", str(exe)], check=True)
    return exe


def test_header_parsing_accepts_and_rejects(format_host):
    p = subprocess.run([str(format_host)], capture_output=True, text=True)
    assert p.returncode == 0 and p.stdout.startswith("ok "), p.stdout + p.stderr


def _convert(exe, mode, values, width):
    inp = "\n".join(f"{int(v):x}" for v in values) + "\n"
    out = subprocess.run([str(exe), mode], input=inp, capture_output=True, text=True, check=True).stdout.split()
    return np.array([int(v, 16) for v in out], dtype=width)


def test_integer_half_conversion_is_numpys(format_host):
    """half_from_float_bits / float_bits_from_half, which the kernels use: every binary16 widens exactly, and floats
    of every class -- random bit patterns, the neighbourhood of every binary16 value and of every tie between two
    of them, the subnormal range, overflow, infinities and NaNs -- round as astype(float16) does."""
    h = np.arange(1 << 16, dtype=np.uint16)
    nan = np.isnan(h.view(np.float16))
    wide = _convert(format_host, "float", h, np.uint32)
    assert np.array_equal(wide[~nan], h.view(np.float16).astype(np.float32).view(np.uint32)[~nan])
    assert np.all(np.isnan(wide[nan].view(np.float32)))
    rng = np.random.default_rng(2)
    exact = h[~nan].view(np.float16).astype(np.float32).view(np.uint32).astype(np.int64)
    ties = (exact[:-1] + exact[1:]) // 2          # (between neighbours of one sign: the midpoint's bit pattern)
    near = np.concatenate([exact + d for d in (-1, 0, 1)] + [ties + d for d in (-1, 0, 1)])
    x = np.concatenate([rng.integers(0, 1 << 32, 40000), near[(near >= 0) & (near < (1 << 32))],
                        [0x33000000, 0x33000001, 0x32ffffff, 0x477fefff, 0x477ff000, 0x47800000, 0x7f7fffff, 0x7f800000,
                         0xff800000, 0x7f800001, 0x7fc00000, 0xffc01234, 0x00000001, 0x80000000]]).astype(np.uint32)
    got = _convert(format_host, "half", x, np.uint16)
    with np.errstate(over="ignore", invalid="ignore"):
        want = x.view(np.float32).astype(np.float16).view(np.uint16)
    isnan = np.isnan(x.view(np.float32))
    assert np.array_equal(got[~isnan], want[~isnan])
    assert np.all(np.isnan(got[isnan].view(np.float16)))
