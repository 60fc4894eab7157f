"""Register and size budget of the fourth stages library, read from its gfx950 code objects (tools/resource_table.py;
CPU only): it holds the PLP kernels and none named like a kernel of the other four libraries, float32 and float64 of
each, none of them uses scratch or spills, and its device code is capped at 64 KiB like the other stages libraries'
(one capped library per family of stage kernels)."""
from tests import resources
from tests.resources import TEXT_CAP

LIB = "libpds_amd_stages4.so"
TYPED_KERNELS = ("plp_rows_kernel",)


def test_the_library_holds_the_plp_kernels_and_no_other():
    table, _ = resources.table(LIB)
    for kernel in TYPED_KERNELS:
        names = sorted(n for n in table if kernel in n)
        assert len(names) == 2, (kernel, sorted(table))  # float32 and float64 of each
        # (mangled names have the template argument as `f` or `d`, demangled ones spell it out)
        assert any(kernel + "IfE" in n or kernel + "<float>" in n for n in names), names
        assert any(kernel + "IdE" in n or kernel + "<double>" in n for n in names), names
    assert all("plp_" in n for n in table), sorted(table)
    assert all(any(kernel in n for kernel in TYPED_KERNELS) for n in table), sorted(table)
    # none named like a kernel of the other libraries (their resource tests count kernels by these names; that no
    # other library holds a kernel of this one's names, or one with "plp_" in it, is tests/test_native_libraries.py's)
    for word in ("sliding", "vad_energy", "select_rows", "resample", "stft_wave", "multistream", "pcen", "specaug",
                 "cepstra"):
        assert not any(word in n for n in table), word


def test_no_kernel_has_scratch_or_spills():
    table, _ = resources.table(LIB)
    assert len(table) == 2
    for name, k in table.items():
        print(name, "vgpr", k.get("vgpr_count"), "sgpr", k.get("sgpr_count"), "static lds",
              k.get("group_segment_fixed_size"))
        assert k.get("private_segment_fixed_size", 0) == 0, (name, k)
        assert k.get("vgpr_spill_count", 0) == 0 and k.get("sgpr_spill_count", 0) == 0, (name, k)
        assert k.get("group_segment_fixed_size", 0) == 0, (name, k)  # (the LDS is dynamic, sized per launch from p)


def test_device_code_stays_under_its_cap():
    _, text = resources.table(LIB)
    print("device code of the fourth stages library:", text, "bytes")
    assert 0 < text <= TEXT_CAP, text
