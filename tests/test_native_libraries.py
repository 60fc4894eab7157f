"""What holds for every shared library of the package alike (``_native.LIBRARIES``; CPU only): a missing file is an
error and never a CPU path, where each is looked for and under which variable, what its return codes raise, and that no
two of them share an exported symbol or a kernel name -- every pair, whichever library came later -- with each stages
library's device code under its 64 KiB cap."""
import itertools
import os
import subprocess
import sys

import pytest

from pydrobert_speech_amd import _native
from tests import resources
from tests.conftest import ROOT

FILES = ("libpds_amd.so", "libpds_amd_stages.so", "libpds_amd_stages2.so", "libpds_amd_stages3.so",
         "libpds_amd_stages4.so", "libpds_amd_stages5.so", "libpds_amd_stages6.so")
# a word that every kernel of a one-family library has in its name, and no kernel of another library may
FAMILY_WORD = {"libpds_amd_stages2.so": "pcen", "libpds_amd_stages3.so": "specaug_", "libpds_amd_stages4.so": "plp_",
               "libpds_amd_stages5.so": "mix_", "libpds_amd_stages6.so": "reverb_"}
each_library = pytest.mark.parametrize("library, file", list(zip(_native.LIBRARIES, FILES)), ids=FILES)


def test_the_libraries_are_the_seven_in_order():
    assert len(_native.LIBRARIES) == len(FILES)
    assert _native.LIBRARIES == (_native.lib, _native.stages_lib, _native.stages2_lib, _native.stages3_lib,
                                 _native.stages4_lib, _native.stages5_lib, _native.stages6_lib)
    assert [library.variable for library in _native.LIBRARIES] == ["PDS_AMD_LIB"] + [
        f"PDS_AMD_STAGES{n}_LIB" for n in ("", 2, 3, 4, 5, 6)]
    assert [library.signatures for library in _native.LIBRARIES] == [_native.SIGNATURES] + [
        getattr(_native, f"STAGES{n}_SIGNATURES") for n in ("", 2, 3, 4, 5, 6)]
    assert (_native.check, _native.check_stages6) == (_native.lib.check, _native.stages6_lib.check)


@each_library
def test_a_missing_library_is_an_error(monkeypatch, tmp_path, library, file):
    monkeypatch.setattr(library, "_handle", None)
    monkeypatch.setattr(library, "path", str(tmp_path / file))
    with pytest.raises(_native.NativeError, match="no CPU fallback") as raised:
        library()
    assert str(raised.value).startswith(f"{tmp_path / file} is missing: build it with")


def _path_constant(library):
    return library.variable[len("PDS_AMD_"):] + "_PATH"  # PDS_AMD_STAGES2_LIB -> STAGES2_LIB_PATH


@each_library
def test_the_library_is_found_at_its_default_place_without_its_variable(library, file):
    assert getattr(_native, _path_constant(library)) == library.path
    if os.environ.get(library.variable):
        assert library.path == os.environ[library.variable]
        return
    assert os.path.basename(library.path) == file
    # the first two beside the package's csrc/, the later stages libraries beside the first library
    csrc = os.path.join(os.path.dirname(os.path.abspath(_native.__file__)), "csrc")
    beside = csrc if library in _native.LIBRARIES[:2] else os.path.dirname(_native.LIB_PATH)
    assert os.path.dirname(library.path) == beside


@each_library
def test_the_variable_of_the_library_is_honoured(tmp_path, library, file):
    made_up = str(tmp_path / "elsewhere" / ("other_" + file))
    env = {k: v for k, v in os.environ.items() if not k.startswith("PDS_AMD_")}
    env[library.variable] = made_up
    code = ("from pydrobert_speech_amd import _native as n\n"
            "for library in n.LIBRARIES:\n"
            "    print(library.path)\n"
            f"print(n.{_path_constant(library)})\n")
    out = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, check=True, capture_output=True,
                         text=True).stdout.split("\n")
    paths, constant = out[:len(FILES)], out[len(FILES)]
    k = FILES.index(file)
    assert paths[k] == made_up and constant == made_up
    # ... and it moves no other library, but that PDS_AMD_LIB takes stages2 .. stages6 with it
    csrc = os.path.join(ROOT, "pydrobert-speech_amd", "csrc")
    for j, other in enumerate(FILES):
        if j != k:
            beside = os.path.dirname(made_up) if k == 0 and j >= 2 else csrc
            assert paths[j] == os.path.join(beside, other), (other, paths[j])


@each_library
def test_return_codes_raise_what_they_always_raised(monkeypatch, library, file):
    monkeypatch.setattr(library, "last_error", lambda: "the message")  # (no need of the built library here)
    library.check(0, "pds_call")
    with pytest.raises(ValueError, match="^pds_call: the message$"):
        library.check(-1, "pds_call")
    with pytest.raises(_native.NativeError, match=r"^pds_call: the message \(code -2\)$"):
        library.check(-2, "pds_call")
    if library is _native.lib:
        with pytest.raises(MemoryError, match="^pds_call: the message$"):
            library.check(-3, "pds_call")
    else:
        with pytest.raises(_native.NativeError, match=r"\(code -3\)$"):
            library.check(-3, "pds_call")


def test_the_signature_tables_are_pairwise_disjoint():
    for a, b in itertools.combinations(_native.LIBRARIES, 2):
        assert not set(a.signatures) & set(b.signatures), (a.variable, b.variable)
    for library in _native.LIBRARIES:  # ... and each names its own error string
        assert library._last_error in library.signatures


def test_the_kernel_names_of_the_built_libraries_are_pairwise_disjoint():
    built = [library for library in _native.LIBRARIES if os.path.exists(library.path)]
    tables = {os.path.basename(library.path): resources.table(library.path)[0] for library in built}
    assert all(tables.values()), {file: len(table) for file, table in tables.items()}
    for a, b in itertools.combinations(tables, 2):
        assert not set(tables[a]) & set(tables[b]), (a, b)
    for file, word in FAMILY_WORD.items():
        for other, table in tables.items():
            assert all(word in n for n in table) if other == file else not any(word in n for n in table), (word, other)


@pytest.mark.parametrize("library, file", list(zip(_native.LIBRARIES, FILES))[1:], ids=FILES[1:])
def test_device_code_of_a_stages_library_stays_under_its_cap(library, file):
    _, text = resources.table(library.path)
    print("device code of", file, text, "bytes")
    assert 0 < text <= resources.TEXT_CAP, text
