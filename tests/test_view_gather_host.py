"""insitu_view_gather_merged without a GPU: the header-only check its root runs before any
section moves (pack_header_set_check of csrc/vdi_pack_format.h) through the stand-alone tests/view_gather_host.cpp
under AddressSanitizer and UndefinedBehaviorSanitizer; the declaration, the export and the binding."""
from __future__ import annotations

import ctypes
import re
import subprocess
from pathlib import Path

import pytest

from insitu_amd import native
from insitu_amd.renderer import InSituContext

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "scenery-insitu_amd" / "csrc"
HEADER = ROOT / "include" / "insitu_hip.h"


@pytest.fixture(scope="module")
def gather_host(tmp_path_factory):
    exe = tmp_path_factory.mktemp("vg") / "view_gather_host"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", str(CSRC), str(ROOT / "tests" / "view_gather_host.cpp"),
                    "-o", str(exe)], check=True)
    return exe


def test_header_set_check_under_the_sanitizers(gather_host):
    p = subprocess.run([str(gather_host)], capture_output=True, text=True)
    assert p.returncode == 0 and p.stdout.startswith("ok "), p.stdout + p.stderr
    assert int(p.stdout.split()[1]) == 99   # (every case of the program ran)


def test_declaration_export_and_binding():
    text = HEADER.read_text()
    assert re.search(r"int\s+insitu_view_gather_merged\(insitu_ctx\*\s*ctx,\s*int format,\s*unsigned long long\*\s*wire_bytes\);",
                     text)
    assert re.search(r"#define\s+INSITU_ABI_VERSION\s+12\b", text)
    comment = text[:text.index("int insitu_view_gather_merged")].rsplit("/*", 1)[1]
    for cited in ("DistributedVolumes.kt:903-904", ":848-849", "an addition within ABI 12", "insitu_pipeline_flush"):
        assert cited in comment, cited
    assert "it merges the rank's own bricks only." not in re.sub(r"\s+\*\s+", " ", text)   # (the sentence this closes)
    assert "insitu_view_gather_merged" in native.EXPORTED_SYMBOLS
    lib = native.load()
    fn = lib.insitu_view_gather_merged
    assert fn.restype is ctypes.c_int
    assert list(fn.argtypes) == [ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(ctypes.c_ulonglong)]
    wire = ctypes.c_ulonglong(77)
    assert fn(None, native.PACK_FLOAT, ctypes.byref(wire)) == -1
    assert b"insitu_view_gather_merged: null context" in lib.insitu_last_error(None)
    assert fn(None, native.PACK_FLOAT, None) == -1
    assert lib.insitu_abi_version() == 12
    assert callable(InSituContext.view_gather_merged)
