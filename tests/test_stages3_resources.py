"""Register and size budget of the third stages library, read from its gfx950 code objects (tools/resource_table.py;
CPU only): it holds the SpecAugment kernels and none named like a kernel of the other three libraries, none of them
uses scratch or spills, and its device code is capped at 64 KiB like the other stages libraries' (DESIGN.md section
4.3: one capped library per family of stage kernels)."""
from tests import resources
from tests.resources import TEXT_CAP

LIB = "libpds_amd_stages3.so"
TYPED_KERNELS = ("specaug_mean_rows_kernel", "specaug_apply_rows_kernel")
PLAIN_KERNELS = ("specaug_plan_kernel",)  # integers only: no row type


def test_the_library_holds_the_specaug_kernels_and_no_other():
    table, _ = resources.table(LIB)
    for kernel in TYPED_KERNELS:
        names = sorted(n for n in table if kernel in n)
        assert len(names) == 2, (kernel, sorted(table))  # float32 and float64 of each
        # (mangled names: the template argument is `f` or `d`)
        assert any(kernel + "IfE" in n for n in names) and any(kernel + "IdE" in n for n in names), names
    for kernel in PLAIN_KERNELS:
        assert len([n for n in table if kernel in n]) == 1, (kernel, sorted(table))
    assert all("specaug_" in n for n in table), sorted(table)
    assert all(any(kernel in n for kernel in TYPED_KERNELS + PLAIN_KERNELS) for n in table), sorted(table)
    # none named like a kernel of the other libraries (their resource tests count kernels by these names; that no
    # other library holds a kernel of this one's names is tests/test_native_libraries.py's)
    for word in ("sliding", "vad_energy", "select_rows", "resample", "stft_wave", "multistream_cmvn", "pcen"):
        assert not any(word in n for n in table), word


def test_no_kernel_has_scratch_or_spills():
    table, _ = resources.table(LIB)
    assert len(table) == 5
    for name, k in table.items():
        assert k.get("private_segment_fixed_size", 0) == 0, (name, k)
        assert k.get("vgpr_spill_count", 0) == 0 and k.get("sgpr_spill_count", 0) == 0, (name, k)


def test_device_code_stays_under_its_cap():
    _, text = resources.table(LIB)
    print("device code of the third stages library:", text, "bytes")
    assert 0 < text <= TEXT_CAP, text
