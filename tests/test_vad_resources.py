"""The energy VAD's kernels in the stages library, read from its gfx950 code objects (tools/resource_table.py; CPU
only): the decision kernel in float32 and float64 and ONE selection kernel (rows are copied as 32-bit words whatever
their type), none with scratch or spills.  The library's size cap is tests/test_sliding_resources.py's."""
from tests import resources

LIB = "libpds_amd_stages.so"


def test_the_library_holds_two_decision_kernels_and_one_selection_kernel():
    table, text = resources.table(LIB)
    decide = sorted(n for n in table if "vad_energy_kernel" in n)
    select = sorted(n for n in table if "select_rows_kernel" in n)
    assert len(decide) == 2 and len(select) == 1, sorted(table)
    # (mangled names: the template argument is `f` or `d`)
    assert any("vad_energy_kernelIfE" in n for n in decide) and any("vad_energy_kernelIdE" in n for n in decide), decide
    # (names that tests/test_sliding_resources.py counts belong to the sliding kernels alone)
    assert not any("sliding_rows_kernel" in n or "multistream_sliding_kernel" in n for n in decide + select)
    for name in decide + select:
        k = table[name]
        assert k.get("private_segment_fixed_size", 0) == 0, (name, k)
        assert k.get("vgpr_spill_count", 0) == 0 and k.get("sgpr_spill_count", 0) == 0, (name, k)
    print("device code of the stages library:", text, "bytes")
    assert text > 0
