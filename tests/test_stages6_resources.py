"""Register and size budget of the sixth stages library, read from its gfx950 code objects (tools/resource_table.py;
CPU only): it holds the three families of reverberation kernels with the expected instantiations and no other, none
named like a kernel of the other six libraries, none of them uses scratch or spills, the static LDS of the transform
kernels (eight transposition areas and the twiddle table) leaves room for two blocks per CU in 160 KB, and its device
code is capped at 64 KiB like the other stages libraries' (one capped library per family of stage
kernels)."""
import importlib.util
import os

import pytest

from tests.conftest import ROOT

CSRC = os.path.join(ROOT, "pydrobert-speech_amd", "csrc")
LIB = os.path.join(CSRC, "libpds_amd_stages6.so")
TEXT_CAP = 65536  # bytes of gfx950 .text: a cap, not a measurement
LDS_PER_CU = 160 * 1024
TRANSFORM_LDS = 8 * 32 * 33 * 8 + 32 * 32 * 8  # eight half waves' transposition areas and the twiddle table
# (mangled names have the template arguments as `f`, `d` and `s`, demangled ones spell them out)
TYPES = (("f", "float"), ("d", "double"), ("s", "short"))


def _resource_table():
    spec = importlib.util.spec_from_file_location("resource_table", os.path.join(ROOT, "tools", "resource_table.py"))
    rt = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(rt)
    return rt


def _table(lib=LIB):
    rt = _resource_table()
    if not os.path.exists(lib) or not os.path.exists(os.path.join(rt.LLVM, "llvm-readelf")):
        pytest.skip("library or llvm-readelf not available")
    rows, text = [], 0
    for elf in rt.code_objects(lib):
        ks, t = rt.kernels_of(elf)
        rows += ks
        text += t
    return {rt.short(n): k for n, k in rows}, text


def test_the_library_holds_the_three_kernel_families_and_no_other():
    table, _ = _table()
    spectra = sorted(n for n in table if "reverb_spectra_kernel" in n)
    assert len(spectra) == 3, sorted(table)  # float, double and int16_t samples
    for short, long in TYPES:
        assert any(f"reverb_spectra_kernelI{short}E" in n or f"reverb_spectra_kernel<{long}>" in n for n in spectra), (
            long, spectra)
    assert len([n for n in table if "reverb_convolve_kernel" in n]) == 1, sorted(table)  # the copy's dtype an argument
    assert len([n for n in table if "reverb_scale_kernel" in n]) == 1, sorted(table)
    assert len(table) == 5 and all("reverb_" in n for n in table), sorted(table)
    # none named like a kernel of the other six libraries (their resource tests count kernels by these names)
    for other in ("libpds_amd.so", "libpds_amd_stages.so", "libpds_amd_stages2.so", "libpds_amd_stages3.so",
                  "libpds_amd_stages4.so", "libpds_amd_stages5.so"):
        path = os.path.join(CSRC, other)
        if not os.path.exists(path):
            continue
        theirs, _ = _table(path)
        assert theirs and not set(theirs) & set(table)
        assert not any("reverb_" in n for n in theirs), other
    for word in ("mix_", "sliding", "resample", "pcen", "specaug", "plp_", "dither", "cepstra", "multistream",
                 "stft_wave", "vad_energy", "select_rows"):
        assert not any(word in n for n in table), word


def test_no_kernel_has_scratch_or_spills_and_lds_is_the_transform_areas():
    table, _ = _table()
    assert len(table) == 5
    for name, k in table.items():
        print(name, "vgpr", k.get("vgpr_count"), "agpr", k.get("agpr_count"), "sgpr", k.get("sgpr_count"), "static lds",
              k.get("group_segment_fixed_size"))
        assert k.get("private_segment_fixed_size", 0) == 0, (name, k)
        assert k.get("vgpr_spill_count", 0) == 0 and k.get("sgpr_spill_count", 0) == 0, (name, k)
        lds = k.get("group_segment_fixed_size", 0)
        if "scale" in name:
            assert lds == 0, (name, k)
            assert k.get("vgpr_count", 0) <= 64, (name, k)  # a bandwidth kernel at full occupancy
        else:
            # the transposition areas and the twiddle table and nothing else; two blocks (16 half waves) per CU
            assert lds == TRANSFORM_LDS and 2 * lds <= LDS_PER_CU, (name, k)
            # blocks of four waves, one per SIMD: a wave may use the whole register file of its SIMD
            assert k.get("vgpr_count", 0) <= 512, (name, k)
        if "spectra" in name:
            assert k.get("vgpr_count", 0) <= 128, (name, k)  # two blocks per CU by registers too


def test_device_code_stays_under_its_cap():
    _, text = _table()
    print("device code of the sixth stages library:", text, "bytes")
    assert 0 < text <= TEXT_CAP, text
