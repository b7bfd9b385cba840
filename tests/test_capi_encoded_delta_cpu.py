"""The C ABI of the encoded delta export (hny_builder_finish_delta_encoded, hny_encoded_delta_free)
without a GPU: the symbols exist and are declared, bad arguments are refused before any device is touched, the ctypes
struct has the layout a C compiler gives the header's, and hny_encode_kv_encoded on the `links` of a hand-filled
hny_encoded_delta emits the crafted stream (what GraphDelta.encode_kv emits for the matching hny_graph_delta)."""
import ctypes as C
import os
import subprocess

import numpy as np

from support import hny, param_types  # noqa: F401
from test_capi_encoded_cpu import CRAFTED, CRAFTED_IDS, encoded_struct, graph_struct, stream

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "hannoy_amd.h")


def test_symbols_and_declarations(hny):
    from hannoy_amd import _capi
    L = hny.load_library()
    header = open(HEADER).read()
    for name in ("hny_builder_finish_delta_encoded", "hny_encoded_delta_free"):
        assert name in _capi.EXPORTED and hasattr(L, name), name
    assert param_types(header, "hny_builder_finish_delta_encoded") == ["hny_builder *", "hny_encoded_delta **"]
    assert param_types(header, "hny_encoded_delta_free", "void") == ["hny_encoded_delta *"]
    assert hny.EncodedDelta is _capi.EncodedDelta and hny.EncodedDeltaStruct is _capi.EncodedDeltaStruct
    assert callable(hny.Builder.finish_delta_encoded)


def test_refused_on_null(hny):
    from hannoy_amd import _capi
    L = hny.load_library()
    out = C.POINTER(_capi.EncodedDeltaStruct)()
    assert L.hny_builder_finish_delta_encoded(None, C.byref(out)) == hny.ERR_INVALID_ARG and not out
    assert L.hny_builder_finish_delta_encoded(None, None) == hny.ERR_INVALID_ARG
    L.hny_encoded_delta_free(None)  # documented: NULL is fine


def test_struct_layout_is_the_headers(hny, tmp_path):
    from hannoy_amd import _capi
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    fields = ("links", "n_removed", "removed_item", "removed_layer", "n_records_total")
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "hannoy_amd.h"\nint main(void) {\n'
                   '  printf("%zu %zu", sizeof(hny_encoded_delta), sizeof(hny_encoded_links));\n'
                   + "".join('  printf(" %%zu", offsetof(hny_encoded_delta, %s));\n' % f for f in fields)
                   + "  return 0;\n}\n")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    S = _capi.EncodedDeltaStruct
    assert got == [C.sizeof(S), C.sizeof(_capi.EncodedLinksStruct)] + [getattr(S, f).offset for f in fields]
    assert S.links.offset == 0  # (&d->links is d: what hny_encode_kv_encoded is handed)


def test_encode_kv_on_a_hand_filled_delta(hny, orc):
    """the crafted records as the changed records of a delta that also removes two keys: the stream is Metadata,
    Version and the records, the removed keys play no part in it"""
    from hannoy_amd import _capi
    e, _keep, vals = encoded_struct(orc, CRAFTED, [0, 0xFFFFFFFF], 3)
    d = _capi.EncodedDeltaStruct()
    d.links = e
    rm = [np.array([1, 65536], np.uint32), np.array([1, 0], np.uint8)]
    d.n_removed = 2
    d.removed_item = rm[0].ctypes.data_as(C.POINTER(C.c_uint32))
    d.removed_layer = rm[1].ctypes.data_as(C.POINTER(C.c_uint8))
    d.n_records_total = 40
    g, _k = graph_struct(CRAFTED, [0, 0xFFFFFFFF], 3)
    ids = np.array(CRAFTED_IDS, np.uint32)
    it = _capi.Items(len(ids), ids.ctypes.data, None, 0, None, 0, None)  # ids only, as GraphDelta.encode_kv passes them
    opts = hny.make_opts(hny.EUCLIDEAN, 3)
    for index in (0, 513):
        want = stream(hny, "hny_encode_kv", g, opts, it, index, 0)
        got = stream(hny, "hny_encode_kv_encoded", d.links, opts, it, index, 0)
        assert got == want and [v for _, v in got[2:]] == vals and len(got) == 2 + len(CRAFTED)
        assert [k[3:7] + k[7:] for k, _ in got[2:]] == [i.to_bytes(4, "big") + bytes([l]) for i, l, _ in CRAFTED]
