"""Register and size budget of the sixth stages library, read from its gfx950 code objects (tools/resource_table.py;
CPU only): it holds the three families of reverberation kernels with the expected instantiations and no other, none
named like a kernel of the other six libraries, none of them uses scratch or spills, the static LDS of the transform
kernels (eight transposition areas and the twiddle table) leaves room for two blocks per CU in 160 KB, and its device
code is capped at 64 KiB like the other stages libraries' (one capped library per family of stage
kernels)."""
from tests import resources
from tests.resources import LDS_PER_CU, TEXT_CAP

LIB = "libpds_amd_stages6.so"
TRANSFORM_LDS = 8 * 32 * 33 * 8 + 32 * 32 * 8  # eight half waves' transposition areas and the twiddle table
# (mangled names have the template arguments as `f`, `d` and `s`, demangled ones spell them out)
TYPES = (("f", "float"), ("d", "double"), ("s", "short"))


def test_the_library_holds_the_three_kernel_families_and_no_other():
    table, _ = resources.table(LIB)
    spectra = sorted(n for n in table if "reverb_spectra_kernel" in n)
    assert len(spectra) == 3, sorted(table)  # float, double and int16_t samples
    for short, long in TYPES:
        assert any(f"reverb_spectra_kernelI{short}E" in n or f"reverb_spectra_kernel<{long}>" in n for n in spectra), (
            long, spectra)
    assert len([n for n in table if "reverb_convolve_kernel" in n]) == 1, sorted(table)  # the copy's dtype an argument
    assert len([n for n in table if "reverb_scale_kernel" in n]) == 1, sorted(table)
    assert len(table) == 5 and all("reverb_" in n for n in table), sorted(table)
    # none named like a kernel of the other libraries (their resource tests count kernels by these names; that no
    # other library holds a kernel of this one's names, or one with "reverb_" in it, is tests/test_native_libraries.py's)
    for word in ("mix_", "sliding", "resample", "pcen", "specaug", "plp_", "dither", "cepstra", "multistream",
                 "stft_wave", "vad_energy", "select_rows"):
        assert not any(word in n for n in table), word


def test_no_kernel_has_scratch_or_spills_and_lds_is_the_transform_areas():
    table, _ = resources.table(LIB)
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
    _, text = resources.table(LIB)
    print("device code of the sixth stages library:", text, "bytes")
    assert 0 < text <= TEXT_CAP, text
