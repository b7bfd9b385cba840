"""Links values written by hand, for the tests of the encoded import (hny_builder_load_encoded and its kin): the
serialiser below shares no code with the library's, and every part of a value can be replaced to make it malformed."""
import struct

import numpy as np

COOKIE = 12346


def containers(ids):
    """[(key, [low-16 values])] of ascending ids, one pair per high-16 group"""
    out = []
    for i in ids:
        i = int(i)
        if not out or out[-1][0] != i >> 16:
            out.append((i >> 16, []))
        out[-1][1].append(i & 0xFFFF)
    return out


def links_value(ids=(), cts=None, tag=1, cookie=COOKIE, nc=None, cards=None, offsets=None):
    """tag | cookie | nc | (key, cardinality - 1) per container | offsets | low-16 values: the value of a Links record
    for ascending `ids` (or the containers `cts`), each header field replaceable"""
    cts = containers(ids) if cts is None else cts
    n = len(cts)
    cards = [len(lows) for _, lows in cts] if cards is None else cards
    if offsets is None:
        offsets = [8 + 8 * n + 2 * sum(len(lows) for _, lows in cts[:k]) for k in range(n)]
    out = bytes([tag]) + struct.pack("<II", cookie, n if nc is None else nc)
    out += b"".join(struct.pack("<HH", key, c - 1) for (key, _), c in zip(cts, cards))
    out += b"".join(struct.pack("<I", o) for o in offsets)
    return out + b"".join(struct.pack("<%dH" % len(lows), *lows) for _, lows in cts)


def decode_value(v):
    """the ids of a well-formed value"""
    assert v[0] == 1 and struct.unpack_from("<I", v, 1)[0] == COOKIE
    n = struct.unpack_from("<I", v, 5)[0]
    at, out = 9 + 8 * n, []
    for k in range(n):
        key, c = struct.unpack_from("<HH", v, 9 + 4 * k)
        out += [key << 16 | x for x in struct.unpack_from("<%dH" % (c + 1), v, at)]
        at += 2 * (c + 1)
    assert at == len(v)
    return out


def values_of(graph):
    """the value of every record of anything with offsets / nbrs"""
    off = np.asarray(graph.offsets).astype(np.int64)
    nb = np.asarray(graph.nbrs)
    return [links_value(nb[a:z]) for a, z in zip(off[:-1], off[1:])]


def encoded(hny, graph, values=None):
    """hny.EncodedLinks of a graph (rec_item / rec_layer / offsets / nbrs / entry_points / max_level), with the values
    given in place of its own"""
    return hny.EncodedLinks.from_records(graph.rec_item, graph.rec_layer, values_of(graph) if values is None else values,
                                         np.asarray(graph.entry_points, np.uint32), graph.max_level)
