"""Register and size budget of the fifth stages library, read from its gfx950 code objects (tools/resource_table.py;
CPU only): it holds the three families of noise-mixing kernels with the expected instantiations and no other, none
named like a kernel of the other five libraries, none of them uses scratch, spills or static LDS, and its device code
is capped at 64 KiB like the other stages libraries' (one capped library per family of stage
kernels)."""
from tests import resources
from tests.resources import TEXT_CAP

LIB = "libpds_amd_stages5.so"
# (mangled names have the template arguments as `f`, `d` and `s`, demangled ones spell them out)
TYPES = (("f", "float"), ("d", "double"), ("s", "short"))


def test_the_library_holds_the_three_kernel_families_and_no_other():
    table, _ = resources.table(LIB)
    energy = sorted(n for n in table if "mix_chunk_energy_kernel" in n)
    assert len(energy) == 3, sorted(table)  # float, double and int16_t segments
    for short, long in TYPES:
        assert any(f"mix_chunk_energy_kernelI{short}E" in n or f"mix_chunk_energy_kernel<{long}>" in n for n in energy), (
            long, energy)
    gain = [n for n in table if "mix_gain_kernel" in n]
    assert len(gain) == 1, sorted(table)  # one kernel, its mode an argument
    apply = sorted(n for n in table if "mix_apply_kernel" in n)
    assert len(apply) == 9, sorted(table)  # signal dtype x bank dtype
    for xs, xl in TYPES:
        for zs, zl in TYPES:
            assert any(f"mix_apply_kernelI{xs}{zs}E" in n or f"mix_apply_kernel<{xl}, {zl}>" in n for n in apply), (
                xl, zl, apply)
    assert len(table) == 13 and all("mix_" in n for n in table), sorted(table)
    # none named like a kernel of the other libraries (their resource tests count kernels by these names; that no
    # other library holds a kernel of this one's names, or one with "mix_" in it, is tests/test_native_libraries.py's)
    for word in ("sliding", "vad_energy", "select_rows", "resample", "stft_wave", "multistream", "pcen", "specaug",
                 "cepstra", "plp_", "dither"):
        assert not any(word in n for n in table), word


def test_no_kernel_has_scratch_spills_or_static_lds():
    table, _ = resources.table(LIB)
    assert len(table) == 13
    for name, k in table.items():
        print(name, "vgpr", k.get("vgpr_count"), "sgpr", k.get("sgpr_count"), "static lds",
              k.get("group_segment_fixed_size"))
        assert k.get("private_segment_fixed_size", 0) == 0, (name, k)
        assert k.get("vgpr_spill_count", 0) == 0 and k.get("sgpr_spill_count", 0) == 0, (name, k)
        assert k.get("group_segment_fixed_size", 0) == 0, (name, k)  # (the tree runs by cross-lane moves: no LDS)
        assert k.get("vgpr_count", 0) <= 64, (name, k)  # every kernel at full occupancy


def test_device_code_stays_under_its_cap():
    _, text = resources.table(LIB)
    print("device code of the fifth stages library:", text, "bytes")
    assert 0 < text <= TEXT_CAP, text
