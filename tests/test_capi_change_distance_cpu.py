"""CPU-side checks of the resident change of distance (hny_distance_keeps_links, hny_builder_create_changed_distance,
hny_builder_recode_items): the symbols are exported, the family rule is the reference's rule on the distances' names,
and bad arguments are refused before any device is touched.  No GPU needed."""
import ctypes as C
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ["hny_distance_keeps_links", "hny_builder_create_changed_distance", "hny_builder_recode_items"]


@pytest.fixture(scope="module")
def capi():
    from hannoy_amd import _capi
    _capi.load_library()
    return _capi


def _err(capi):
    return capi.load_library().hny_last_error().decode()


def test_entry_points_are_exported(capi):
    lib = capi.load_library()
    for name in ENTRY_POINTS:
        assert hasattr(lib, name), name
        assert name in capi.EXPORTED


def test_keeps_links_is_the_rule_on_the_names(capi):
    """writer.rs:359-368: links stay iff the new distance's name is "binary quantized " + the old one's"""
    from hannoy_amd.api import Metric
    kept = []
    for old in Metric:
        for new in Metric:
            want = str(new) == "binary quantized " + str(old)
            assert capi.distance_keeps_links(old.value, new.value) == want, (old, new)
            if want:
                kept.append((old, new))
    assert len(list(Metric)) ** 2 == 49 and len(kept) == 3
    assert kept == [(Metric.COSINE, Metric.BQ_COSINE), (Metric.EUCLIDEAN, Metric.BQ_EUCLIDEAN),
                    (Metric.MANHATTAN, Metric.BQ_MANHATTAN)]
    L = capi.load_library()
    for bad in (-1, 7, 1 << 20):
        assert L.hny_distance_keeps_links(bad, capi.BQ_COSINE) == 0 and L.hny_distance_keeps_links(capi.COSINE, bad) == 0


def test_null_arguments_are_refused_without_a_device(capi):
    L = capi.load_library()
    c = capi.ChangeDistance()
    c.new_metric = capi.BQ_COSINE
    out = C.c_void_p(0x1234)  # a refusal leaves *out as it was
    assert c.struct_size == C.sizeof(capi.ChangeDistance)
    assert L.hny_builder_create_changed_distance(None, C.byref(c), C.byref(out)) == capi.ERR_INVALID_ARG
    assert "null source" in _err(capi) and out.value == 0x1234
    assert L.hny_builder_create_changed_distance(None, None, C.byref(out)) == capi.ERR_INVALID_ARG
    assert "null" in _err(capi) and out.value == 0x1234
    assert L.hny_builder_create_changed_distance(None, C.byref(c), None) == capi.ERR_INVALID_ARG
    assert "null" in _err(capi)
    buf = (C.c_uint8 * 16)()
    assert L.hny_builder_recode_items(None, capi.BQ_COSINE, buf, buf) == capi.ERR_INVALID_ARG
    assert "null source" in _err(capi)


@pytest.mark.parametrize("off", [-8, 8])
def test_wrong_struct_size_names_the_field(capi, off):
    L = capi.load_library()
    c = capi.ChangeDistance()
    out = C.c_void_p(0x1234)
    # the size the binding computes is the one the library expects: it gets past the guard, to the NULL source
    assert L.hny_builder_create_changed_distance(None, C.byref(c), C.byref(out)) == capi.ERR_INVALID_ARG
    assert "struct_size" not in _err(capi) and "null source" in _err(capi)
    c.struct_size = C.sizeof(capi.ChangeDistance) + off
    assert L.hny_builder_create_changed_distance(None, C.byref(c), C.byref(out)) == capi.ERR_INVALID_ARG
    msg = _err(capi)
    assert "hny_change_distance.struct_size" in msg and str(C.sizeof(capi.ChangeDistance) + off) in msg
    assert str(C.sizeof(capi.ChangeDistance)) in msg and out.value == 0x1234
    # ... and the guard of the hny_update it points to
    c.struct_size = C.sizeof(capi.ChangeDistance)
    u = capi.Update()
    u.struct_size = C.sizeof(capi.Update) + off
    c.update = C.pointer(u)
    assert L.hny_builder_create_changed_distance(None, C.byref(c), C.byref(out)) == capi.ERR_INVALID_ARG
    assert "hny_update.struct_size" in _err(capi) and out.value == 0x1234


def test_struct_layout_header_vs_binding(capi, tmp_path):
    """sizeof(hny_change_distance) and its field offsets as gcc lays the header out == the ctypes struct; the struct
    did not join hny_abi_sizes (seven entries, as before)"""
    fields = [f for f, _ in capi.ChangeDistance._fields_]
    body = ['printf("%zu\\n", sizeof(hny_change_distance));']
    body += [f'printf("%zu\\n", offsetof(hny_change_distance, {f}));' for f in fields]
    src = tmp_path / "cd_sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "hannoy_amd.h"\nint main(void){' + "".join(body) +
                   "return 0;}\n")
    exe = tmp_path / "cd_sizes"
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)], text=True).split()]
    assert got == [C.sizeof(capi.ChangeDistance)] + [getattr(capi.ChangeDistance, f).offset for f in fields]
    assert capi.load_library().hny_abi_sizes(None, 0) == 7 and len(capi.ABI_STRUCTS) == 7
