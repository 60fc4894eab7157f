"""Register and size budget of the stages library, read from its gfx950 code objects (tools/resource_table.py; CPU
only): no kernel of it may use scratch or spill, and its device code is capped so that it does not become a way round
the size bound of libpds_amd.so."""
from tests import resources
from tests.resources import TEXT_CAP

LIB = "libpds_amd_stages.so"


def test_no_kernel_has_scratch_or_spills():
    table, _ = resources.table(LIB)
    offline = [n for n in table if "sliding_rows_kernel" in n]
    streaming = [n for n in table if "multistream_sliding_kernel" in n]
    assert len(offline) == 2 and len(streaming) == 2, sorted(table)  # float32 and float64 of each
    for name, k in table.items():
        assert k.get("private_segment_fixed_size", 0) == 0, (name, k)
        assert k.get("vgpr_spill_count", 0) == 0 and k.get("sgpr_spill_count", 0) == 0, (name, k)


def test_device_code_stays_under_its_cap():
    _, text = resources.table(LIB)
    assert 0 < text <= TEXT_CAP, text
