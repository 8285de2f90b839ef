"""CPU: the entry points that change a built position index (kh_index_append*, kh_index_erase, kh_index_erase_counts and their
kh_wide_index_ twins) are declared, bound and exported, the Python methods exist on both classes, and the null-handle forms are
refused without touching the out-parameters."""
import ctypes as C
import inspect
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OPS = ["append", "append_from_sequence", "append_from_fastq", "erase", "erase_counts"]
NEW = [pre + s for pre in ("kh_index_", "kh_wide_index_") for s in OPS]


@pytest.fixture(scope="module")
def capi():
    from kmerhash_amd.build import build_library
    build_library()
    from kmerhash_amd import _capi
    return _capi


def test_symbols_declared_bound_and_exported(capi):
    assert len(NEW) == 10
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "kmerhash_amd.h")).read(), flags=re.S)
    L = capi.lib()
    for s in NEW:
        assert re.search(r"\b%s\s*\(" % s, txt), "%s is not declared" % s
        assert s in capi.SYMBOLS
        f = getattr(L, s)                                   # AttributeError: not exported
        assert f.argtypes, s
        assert f.restype is C.c_int
    for s in OPS:                                           # one contract, two key widths
        assert list(getattr(L, "kh_wide_index_" + s).argtypes) == list(getattr(L, "kh_index_" + s).argtypes), s
    # append is build's argument list; the text forms are the build forms plus pos_base
    assert list(L.kh_index_append.argtypes) == list(L.kh_index_build.argtypes)
    assert list(L.kh_index_append_from_sequence.argtypes) == list(L.kh_index_build_from_sequence.argtypes) + [C.c_uint32]
    assert list(L.kh_index_append_from_fastq.argtypes) == list(L.kh_index_build_from_fastq.argtypes) + [C.c_uint32]


def test_header_no_longer_calls_the_index_static():
    txt = open(os.path.join(ROOT, "include", "kmerhash_amd.h")).read()
    assert "Appending to or erasing from a built index" not in txt
    assert "appending to or erasing from a built index" not in txt


def test_python_methods_on_both_classes():
    import kmerhash_amd as kh
    for cls in (kh.KmerPositionIndex, kh.WideKmerPositionIndex):
        for m in ("append", "append_sequences", "append_fastq", "erase", "erase_counts", "drop_above"):
            assert callable(getattr(cls, m, None)), (cls.__name__, m)
        assert inspect.signature(cls.append_sequences).parameters["pos_base"].default == 0
        assert inspect.signature(cls.append_fastq).parameters["pos_base"].default == 0
        assert list(inspect.signature(cls.erase_counts).parameters)[1:] == ["lo", "hi"]
        assert list(inspect.signature(cls.drop_above).parameters)[1:] == ["max_occ"]
    # inherited through PREFIX / _kbuf, not restated
    for m in ("append", "append_sequences", "append_fastq", "erase", "erase_counts", "drop_above"):
        assert m not in kh.WideKmerPositionIndex.__dict__, m


@pytest.mark.parametrize("pre", ["kh_index_", "kh_wide_index_"])
def test_null_handle_forms_are_refused(capi, pre):
    L = capi.lib()
    f = lambda s: getattr(L, pre + s)                       # noqa: E731
    for n in (0, 1, 1 << 32):
        assert f("append")(None, None, None, n, capi.KH_MEM_HOST) == capi.KH_ERR_INVALID
        assert f("append_from_sequence")(None, None, n, 21, 1, capi.KH_MEM_HOST, 0) == capi.KH_ERR_INVALID
        assert f("append_from_fastq")(None, None, n, 21, 1, capi.KH_MEM_HOST, 0xFFFFFFFF) == capi.KH_ERR_INVALID
        nk, npos = C.c_uint64(7), C.c_uint64(9)
        assert f("erase")(None, None, n, capi.KH_MEM_HOST, C.byref(nk), C.byref(npos)) == capi.KH_ERR_INVALID
        assert (nk.value, npos.value) == (0, 0)
        assert f("erase")(None, None, n, capi.KH_MEM_HOST, None, None) == capi.KH_ERR_INVALID
    nk, npos = C.c_uint64(7), C.c_uint64(9)
    assert f("erase_counts")(None, 1, 0xFFFFFFFF, C.byref(nk), C.byref(npos)) == capi.KH_ERR_INVALID
    assert (nk.value, npos.value) == (0, 0)
    assert f("erase_counts")(None, 5, 2, None, None) == capi.KH_ERR_INVALID
