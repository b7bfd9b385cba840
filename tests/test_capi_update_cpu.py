"""CPU-side checks of the resident update entry points (hny_builder_create_update, hny_builder_update,
hny_builder_finish_delta, hny_graph_delta_free): they are exported, refuse bad arguments before any device is
touched, and their structs have one layout in the header, the library and the ctypes binding.  No GPU needed."""
import ctypes as C
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ["hny_builder_create_update", "hny_builder_update", "hny_builder_finish_delta", "hny_graph_delta_free"]


@pytest.fixture(scope="module")
def capi():
    from hannoy_amd import _capi
    _capi.load_library()
    return _capi


def _err(capi):
    return capi.load_library().hny_last_error().decode()


def test_update_entry_points_are_exported(capi):
    lib = capi.load_library()
    for name in ENTRY_POINTS:
        assert hasattr(lib, name), name
        assert name in capi.EXPORTED


def test_null_arguments_are_refused_without_a_device(capi):
    L = capi.load_library()
    u = capi.Update()
    out = C.c_void_p()
    assert u.struct_size == C.sizeof(capi.Update)
    assert L.hny_builder_create_update(None, C.byref(u), C.byref(out)) == capi.ERR_INVALID_ARG
    assert "null" in _err(capi) and not out.value
    assert L.hny_builder_create_update(None, None, C.byref(out)) == capi.ERR_INVALID_ARG
    assert "null" in _err(capi)
    assert L.hny_builder_create_update(None, C.byref(u), None) == capi.ERR_INVALID_ARG
    assert "null" in _err(capi)
    gp, dp = C.POINTER(capi.GraphStruct)(), C.POINTER(capi.GraphDeltaStruct)()
    null_b = C.c_void_p()
    assert L.hny_builder_update(None, C.byref(u), C.byref(gp), C.byref(dp)) == capi.ERR_INVALID_ARG
    assert L.hny_builder_update(C.byref(null_b), C.byref(u), C.byref(gp), C.byref(dp)) == capi.ERR_INVALID_ARG
    assert "null" in _err(capi) and not gp and not dp
    assert L.hny_builder_update(C.byref(null_b), None, None, None) == capi.ERR_INVALID_ARG
    assert L.hny_builder_finish_delta(None, C.byref(dp)) == capi.ERR_INVALID_ARG
    assert L.hny_builder_finish_delta(None, None) == capi.ERR_INVALID_ARG
    L.hny_graph_delta_free(None)  # like free(NULL)


@pytest.mark.parametrize("off", [-8, 8])
def test_wrong_struct_size_names_the_field(capi, off):
    L = capi.load_library()
    u = capi.Update()
    u.struct_size = C.sizeof(capi.Update) + off
    out = C.c_void_p()
    assert L.hny_builder_create_update(None, C.byref(u), C.byref(out)) == capi.ERR_INVALID_ARG
    msg = _err(capi)
    assert "struct_size" in msg and str(C.sizeof(capi.Update) + off) in msg and str(C.sizeof(capi.Update)) in msg
    null_b = C.c_void_p()
    assert L.hny_builder_update(C.byref(null_b), C.byref(u), None, None) == capi.ERR_INVALID_ARG
    assert "struct_size" in _err(capi)


def test_struct_sizes_header_vs_binding(capi, tmp_path):
    """sizeof(hny_update) and sizeof(hny_graph_delta) as gcc lays the header out == the ctypes structs, field
    offsets included; the new structs did not join hny_abi_sizes (seven entries, as before)."""
    src = tmp_path / "upd_sizes.c"
    fields_u = [f for f, _ in capi.Update._fields_]
    fields_d = [f for f, _ in capi.GraphDeltaStruct._fields_]
    body = ['printf("%zu %zu\\n", sizeof(hny_update), sizeof(hny_graph_delta));']
    body += [f'printf("%zu\\n", offsetof(hny_update, {f}));' for f in fields_u]
    body += [f'printf("%zu\\n", offsetof(hny_graph_delta, {f}));' for f in fields_d]
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "hannoy_amd.h"\nint main(void){' + "".join(body) +
                   "return 0;}\n")
    exe = tmp_path / "upd_sizes"
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)], text=True).split()]
    assert got[:2] == [C.sizeof(capi.Update), C.sizeof(capi.GraphDeltaStruct)]
    want = [getattr(capi.Update, f).offset for f in fields_u] + [getattr(capi.GraphDeltaStruct, f).offset for f in fields_d]
    assert got[2:] == want
    L = capi.load_library()
    assert L.hny_abi_sizes(None, 0) == 7 and len(capi.ABI_STRUCTS) == 7
