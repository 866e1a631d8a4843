"""The compact view layout (INSITU_OPT_VIEW_COMPACT) without a GPU: the export of the option
and of the three statistics, native.Stats against the header, insitu_set_option with a null context, and the
layout's size arithmetic (csrc/vdi_view_layout.h) through the stand-alone tests/view_compact_host.cpp, built with
AddressSanitizer and UndefinedBehaviorSanitizer and run as a program of its own."""
from __future__ import annotations

import ctypes
import re
import subprocess
from pathlib import Path

import pytest

from insitu_amd import native

ROOT = Path(__file__).resolve().parent.parent
HEADER = ROOT / "include" / "insitu_hip.h"
CSRC = ROOT / "scenery-insitu_amd" / "csrc"


def test_option_and_stats_are_exported():
    text = HEADER.read_text()
    assert re.search(r"\bINSITU_OPT_VIEW_COMPACT\s*=\s*15\b", text)
    assert native.OPT_VIEW_COMPACT == 15
    assert re.search(r"#define\s+INSITU_ABI_VERSION\s+12\b", text) and native.ABI_VERSION == 12
    fields = [name for name, _ in native.Stats._fields_]
    assert fields[-4:] == ["ms_view_bind", "view_entries", "view_bytes", "view_compact"]
    kinds = dict(native.Stats._fields_)
    assert kinds["view_entries"] is ctypes.c_longlong and kinds["view_bytes"] is ctypes.c_longlong
    assert kinds["view_compact"] is ctypes.c_int
    # the two formulas stand in the header's comment
    assert "24*W*H*S + W*H + tiles" in text and "24*max(E,1) + 3*W*H + 8*nblocks + tiles" in text


def test_stats_layout_matches_header(tmp_path):
    src = tmp_path / "stats.c"
    src.write_text(r'''
#include <stdio.h>
#include <stddef.h>
#include "insitu_hip.h"
int main(void) {
  printf("%zu %zu %zu %zu %zu\n", sizeof(insitu_stats), offsetof(insitu_stats, ms_view_bind),
         offsetof(insitu_stats, view_entries), offsetof(insitu_stats, view_bytes), offsetof(insitu_stats, view_compact));
  return 0;
}''')
    exe = tmp_path / "stats"
    subprocess.run(["gcc", "-std=c99", "-I", str(ROOT / "include"), str(src), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    S = native.Stats
    assert got == [ctypes.sizeof(S), S.ms_view_bind.offset, S.view_entries.offset, S.view_bytes.offset, S.view_compact.offset]


def test_set_option_with_a_null_context():
    lib = native.load()
    for value in (0, 1, 2, -1):
        assert lib.insitu_set_option(None, native.OPT_VIEW_COMPACT, value) == -1
    assert b"null context" in lib.insitu_last_error(None)
    assert lib.insitu_abi_version() == 12


@pytest.fixture(scope="module")
def layout_host(tmp_path_factory):
    exe = tmp_path_factory.mktemp("vc") / "view_compact_host"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", str(CSRC), str(ROOT / "tests" / "view_compact_host.cpp"),
                    "-o", str(exe)], check=True)
    return exe


def test_size_arithmetic_under_the_sanitizers(layout_host):
    p = subprocess.run([str(layout_host)], capture_output=True, text=True)
    assert p.returncode == 0 and p.stdout.startswith("ok "), p.stdout + p.stderr
    assert int(p.stdout.split()[1]) >= 28


def test_layout_header_needs_no_hip(tmp_path):
    """vdi_view_layout.h compiles for the CPU alone, as C++11 and with every warning an error."""
    src = tmp_path / "t.cpp"
    src.write_text('#include "vdi_view_layout.h"\nint main() { insitu::ViewLayoutSize s{}; '
                   'return insitu::view_compact_size(9, 7, 1, 63, &s) && s.bytes == 1711 ? 0 : 1; }\n')
    exe = tmp_path / "t"
    subprocess.run(["g++", "-std=c++11", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", str(CSRC), str(src), "-o", str(exe)],
                   check=True)
    assert subprocess.run([str(exe)]).returncode == 0
