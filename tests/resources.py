"""What a built library's gfx950 code objects say about its kernels (tools/resource_table.py; CPU only), for the
resource tests of every library and ``test_native_libraries.py``.

This module is a plain helper (no tests, no fixtures).
"""
import importlib.util
import os

import pytest

from tests.conftest import ROOT

CSRC = os.path.join(ROOT, "pydrobert-speech_amd", "csrc")
TEXT_CAP = 65536  # bytes of gfx950 .text of a stages library: a cap, not a measurement
LDS_PER_CU = 160 * 1024


def _resource_table():
    spec = importlib.util.spec_from_file_location("resource_table", os.path.join(ROOT, "tools", "resource_table.py"))
    rt = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(rt)
    return rt


def table(lib_file):
    """({short kernel name: its metadata}, bytes of device code) of ``csrc/<lib_file>`` (or of a path); skips without
    the library or llvm-readelf"""
    rt = _resource_table()
    lib = os.path.join(CSRC, lib_file)
    if not os.path.exists(lib) or not os.path.exists(os.path.join(rt.LLVM, "llvm-readelf")):
        pytest.skip("library or llvm-readelf not available")
    rows, text = [], 0
    for elf in rt.code_objects(lib):
        ks, t = rt.kernels_of(elf)
        rows += ks
        text += t
    return {rt.short(n): k for n, k in rows}, text
