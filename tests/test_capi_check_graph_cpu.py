"""hny_builder_check_graph without a GPU: the symbol and its structs as the header declares them, and what the header
lists as decided before any device work, in its order, with *out untouched.  (A builder is read only by the last of
those checks, so a block of zero bytes stands in for one up to there; the refusal of an unfinished builder needs a
device: test_gpu_check_graph.py.)"""
import ctypes as C
import os
import re

import pytest

from support import hny, param_types  # noqa: F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_symbol_and_structs_are_the_headers(hny):
    from hannoy_amd import _capi
    header = open(os.path.join(ROOT, "include", "hannoy_amd.h")).read()
    fn = hny.load_library().hny_builder_check_graph
    assert "hny_builder_check_graph" in _capi.EXPORTED and fn.restype is C.c_int
    assert param_types(header, "hny_builder_check_graph") == ["hny_builder *", "const hny_check_opts *",
                                                              "hny_graph_report *"]
    for cname, cls in (("hny_check_opts", _capi.CheckOpts), ("hny_graph_report", _capi.GraphReport)):
        body = re.search(r"typedef struct \{([^}]*)\} %s;" % cname, header, re.S).group(1)
        body = re.sub(r"/\*.*?\*/|\[\w+\]", "", body, flags=re.S)
        names = []
        for decl in body.split(";"):
            m = re.search(r"\(\*(\w+)\)\(", decl)
            names += [m.group(1)] if m else [w.strip(" *\n") for w in decl.split(",") if w.strip()]
        assert [n.split()[-1].lstrip("*") for n in names] == [f[0] for f in cls._fields_], cname
    assert C.sizeof(_capi.CheckOpts) == 56 == _capi.CheckOpts().struct_size
    assert C.sizeof(_capi.GraphReport) == 32 + 4 * 15 * 8 + 15 * 4 + 4 + 7 * 8 + 8
    assert (_capi.CHECK_LISTS, _capi.CHECK_REACH, _capi.CHECK_LAYERS) == (1, 2, 15)
    assert all(s in header for s in ("#define HNY_CHECK_LISTS 1u", "#define HNY_CHECK_REACH 2u",
                                     "#define HNY_CHECK_LAYERS 15"))


def test_abi_table_is_the_parents(hny):
    out = (C.c_uint32 * 16)()
    assert hny.load_library().hny_abi_sizes(out, 16) == 7 and len(hny.abi_sizes()) == 7


def _opts(_capi, **kw):
    o = _capi.CheckOpts()
    for k, v in kw.items():
        setattr(o, k, v)
    return o


@pytest.mark.parametrize("case,message", [
    ("no-builder", "null argument"), ("no-opts", "null argument"), ("no-out", "null argument"),
    ("struct-size", "struct_size 55"), ("cap-without-buffer", "cap_unreachable without out_unreachable"),
    ("what-bit-2", "what 4"), ("what-high-bits", "what 2147483651")])
def test_refused_before_any_device_work(hny, case, message):
    from hannoy_amd import _capi
    L = hny.load_library()
    block = C.create_string_buffer(1 << 16)  # never read: every case is decided before the builder is looked at
    b = None if case == "no-builder" else C.cast(block, C.c_void_p)
    o = _opts(_capi, **{"struct-size": dict(struct_size=55), "cap-without-buffer": dict(cap_unreachable=1),
                        "what-bit-2": dict(what=4), "what-high-bits": dict(what=0x80000003)}.get(case, {}))
    out = _capi.GraphReport()
    C.memset(C.byref(out), 0x5A, C.sizeof(out))
    rc = L.hny_builder_check_graph(b, None if case == "no-opts" else C.byref(o), None if case == "no-out" else C.byref(out))
    assert rc == _capi.ERR_INVALID_ARG and message in L.hny_last_error().decode()
    assert bytes(out) == b"\x5a" * C.sizeof(out)
