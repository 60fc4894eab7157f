"""tests/flow_matrix.py against csrc/stft_geoms.def and the computers' host attributes: no GPU needed.

A PDS_GEOM line added to the .def fails here until the matrix has a row for it, and with the row a parity case in
test_gpu_flow_matrix.py.
"""
import json

import numpy as np
import pytest

from pydrobert_speech_amd.alias import alias_factory_subclass_from_arg
from pydrobert_speech_amd.compute import FrameComputer
from tests import flow_matrix as fm
from tests import structured as st


def geoms():
    with open(fm.GEOMS_DEF) as fh:
        return fm.parse_geoms(fh.read())


def computer(cfg):
    return alias_factory_subclass_from_arg(FrameComputer, json.loads(json.dumps(cfg)))


def test_one_row_per_geometry_line():
    lines = geoms()
    assert len(lines) >= 24 and len(lines) == len(set(lines))
    assert fm.mismatches(lines) == []
    assert list(fm.MATRIX) == lines  # (the .def's order: the dispatch takes the first line that holds the frame)
    assert set(fm.MATRIX.values()) <= set(st.suite_names()) and len(set(fm.MATRIX.values())) == len(fm.MATRIX)


def test_a_new_geometry_line_fails_the_guard(tmp_path):
    """A scratch copy of the .def with one more line (outside the experiments block) is not covered by the matrix;
    one more line inside that block changes nothing"""
    with open(fm.GEOMS_DEF) as fh:
        text = fh.read()
    scratch = tmp_path / "stft_geoms.def"
    scratch.write_text(text.replace("#if PDS_EXPERIMENTS", "PDS_GEOM(64, 32, 50, 3)\n#if PDS_EXPERIMENTS"))
    problems = fm.mismatches(fm.parse_geoms(scratch.read_text()))
    assert len(problems) == 1 and "(64, 32, 50)" in problems[0]
    scratch.write_text(text.replace("#endif", "PDS_GEOM(32, 32, 28, 3)\n#endif"))
    assert fm.mismatches(fm.parse_geoms(scratch.read_text())) == []
    # ... and a row whose line is gone
    scratch.write_text(text.replace("PDS_GEOM(16, 8, 16, 4)\n", ""))
    assert len(fm.mismatches(fm.parse_geoms(scratch.read_text()))) == 1


@pytest.mark.parametrize("row", list(fm.MATRIX), ids=lambda r: "x".join(map(str, r)))
def test_configuration_reaches_its_row(row):
    """The dispatch rule of launch_stft_fast_f32 restated on the host: the smallest ROWS of the transform size that
    holds ceil(L / N2) rows (the GPU test asks the plan itself: plan.geometry)"""
    comp = computer(st.suite_config(fm.MATRIX[row])[1])
    assert comp.dft_size == fm.dft_size(row)
    assert fm.dispatched_row(comp, geoms()) == row, (fm.MATRIX[row], comp.dft_size, comp.frame_length)


def test_every_row_lists_its_flows():
    for row in fm.MATRIX:
        flows = fm.flows(row)
        assert "f32+preemph" in flows and len(set(flows)) == len(flows)
        if fm.dft_size(row) in (256, 512, 1024, 2048):
            assert set(fm.SAMPLE_FLOWS) <= set(flows), row
        else:
            assert not set(flows) & {"f64in", "f64in+preemph", "i16", "i16+preemph"}, row
    fused = [row for row in fm.MATRIX if row[1] == 16 and row[0] in (32, 64)]
    assert sorted(fused) == sorted(fm.FUSED_ROWS) and len(fused) == 6
    for row in fm.MATRIX:
        want = set(fm.DELTAS_FLOWS) | set(fm.RAGGED_FLOWS) | {"cmvn"}
        assert (want <= set(fm.flows(row))) if row in fused else not (want & set(fm.flows(row))), row
        assert fm.plan_flags(row)[2] == (row in fused)
    assert set(fm.CMVN_WALK) == set(fused)
    assert sum(len(fm.flows(row)) for row in fm.MATRIX) == len(fm.cases()) + len(fm.COVERED)
    assert len({(row, flow) for row, _, flow in fm.cases()}) == len(fm.cases())


def test_pairs_left_to_the_structured_suite_are_run_there():
    """A (row, flow) the matrix does not run itself names the test of test_gpu_structured.py that does, on the same
    configuration"""
    from tests import test_gpu_structured as tgs

    for (row, flow), (test, name) in fm.COVERED.items():
        assert flow in fm.flows(row) and callable(getattr(tgs, test)), (row, flow, test)
        ids = [p for mark in getattr(tgs, test).pytestmark if mark.name == "parametrize" for p in mark.args[1]]
        assert name in ids, (test, name, ids)
        mine = st.suite_config(fm.MATRIX[row])[0]
        if name in tgs.DELTAS_CONFIGS:
            assert flow == "deltas:K=2"  # (Deltas(2) is what that test launches)
            theirs = st.params_from_computer(computer(tgs.DELTAS_CONFIGS[name]))
        else:
            theirs = st.suite_config(name)[0]
        assert (theirs.frame_length, theirs.frame_shift, theirs.dft_size, theirs.include_energy, theirs.use_power,
                theirs.use_log, list(theirs.starts)) == (mine.frame_length, mine.frame_shift, mine.dft_size,
                                                         mine.include_energy, mine.use_power, mine.use_log, list(mine.starts))
        # (the fixture's tables come from the reference, the other's from this package: test_host.py pins them together)
        assert all(a.shape == b.shape and np.allclose(a, b, rtol=1e-12, atol=0) for a, b in zip(theirs.taps, mine.taps))
