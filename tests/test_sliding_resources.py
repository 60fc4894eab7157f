"""Register and size budget of the stages library, read from its gfx950 code objects (tools/resource_table.py; CPU
only): no kernel of it may use scratch or spill, and its device code is capped so that it does not become a way round
the size bound of libpds_amd.so."""
import importlib.util
import os

import pytest

from tests.conftest import ROOT

LIB = os.path.join(ROOT, "pydrobert-speech_amd", "csrc", "libpds_amd_stages.so")
TEXT_CAP = 65536  # bytes of gfx950 .text: a cap, not a measurement


def _table():
    spec = importlib.util.spec_from_file_location("resource_table", os.path.join(ROOT, "tools", "resource_table.py"))
    rt = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(rt)
    if not os.path.exists(LIB) or not os.path.exists(os.path.join(rt.LLVM, "llvm-readelf")):
        pytest.skip("library or llvm-readelf not available")
    rows, text = [], 0
    for elf in rt.code_objects(LIB):
        ks, t = rt.kernels_of(elf)
        rows += ks
        text += t
    return {rt.short(n): k for n, k in rows}, text


def test_no_kernel_has_scratch_or_spills():
    table, _ = _table()
    offline = [n for n in table if "sliding_rows_kernel" in n]
    streaming = [n for n in table if "multistream_sliding_kernel" in n]
    assert len(offline) == 2 and len(streaming) == 2, sorted(table)  # float32 and float64 of each
    for name, k in table.items():
        assert k.get("private_segment_fixed_size", 0) == 0, (name, k)
        assert k.get("vgpr_spill_count", 0) == 0 and k.get("sgpr_spill_count", 0) == 0, (name, k)


def test_device_code_stays_under_its_cap():
    _, text = _table()
    assert 0 < text <= TEXT_CAP, text
