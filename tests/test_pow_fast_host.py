"""det_pow_normal (insitu_device.h: det_pow without its special-value selects, the adjusted opacity's fast path in
march_pass / march_multi) against det_pow on the host: tests/pow_fast_host.cpp walks every 64th float x of
[2^-126, 1] and every float within 2^12 ulps of 2^-126, 0.5 and 1, crossed with exponents over the guard's whole
range and on and beside both of its edges.  Where the guard holds the two have the same bits; the guard holds exactly
for a finite positive normal x with y * log2(x) in [-125, 127], so never for x = 0, a subnormal, a negative, inf or
NaN, nor for a product beyond either edge."""
from __future__ import annotations

import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent


@pytest.fixture(scope="module")
def counts(tmp_path_factory):
    exe = tmp_path_factory.mktemp("pf") / "pow_fast_host"
    subprocess.run(["/opt/rocm/bin/hipcc", "-O2", "-std=c++17", "-ffp-contract=off", "-pthread",
                    "-I", str(ROOT / "scenery-insitu_amd" / "csrc"), str(ROOT / "tests" / "pow_fast_host.cpp"),
                    "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True)
    pairs, guarded, on_edge, mismatches, guard_wrong, special = (int(v) for v in out.stdout.split())
    return dict(pairs=pairs, guarded=guarded, on_edge=on_edge, mismatches=mismatches, guard_wrong=guard_wrong,
                special=special, stderr=out.stderr)


def test_walk_covers_both_sides_of_the_guard(counts):
    # 16.5 M x, 30 exponents each: a good part inside the guard, a good part outside, some exactly on an edge
    assert counts["pairs"] > 4e8
    assert counts["guarded"] > 0.2 * counts["pairs"]
    assert counts["pairs"] - counts["guarded"] > 0.05 * counts["pairs"]
    assert counts["on_edge"] > 1000


def test_fast_path_has_det_pow_bits(counts):
    assert counts["mismatches"] == 0, counts["stderr"]


def test_guard_is_exact(counts):
    assert counts["guard_wrong"] == 0, counts["stderr"]
    assert counts["special"] == 0, "the guard accepted x = 0, a subnormal, a negative, inf or NaN, or a non-finite exponent"
