"""HNY_WALK_RESIDENT: the tiled layer-0 walks of a build on fewer resident waves than walk_slots.

The switch only changes how many one-wave workgroups a k_walk launch of the XCD-tiled queue has (hny_host.cpp
walk_resident_of): the eight per-XCD counters then hand the same tiles to fewer waves, each wave takes more
members, and a wave whose own counter ran out steals from the next.  Every member is still walked exactly once,
so the graph equals the oracle's edge for edge and the walk evaluations are the oracle's number, whatever the
residency.  The switch is read when a builder is created: every value runs in a fresh child process.
"""
import os
import subprocess
import sys
import types

import numpy as np
import pytest

from conftest import ROOT
from support import same_graph

pytestmark = pytest.mark.gpu

M, M0, EF, DIM = 16, 32, 100, 768

# the child: one build from the item set in argv[1] with the options of argv[3:], graph -> argv[2]
CHILD = r"""
import sys
import numpy as np
sys.path.insert(0, sys.argv[3])
import hannoy_amd as H
H.load_library()
d = np.load(sys.argv[1])
frac, bmax = float(sys.argv[4]), int(sys.argv[5])
items = H.ItemSet(H.COSINE, int(d["dim"]), d["ids"], d["codes"], d["headers"], d["levels"])
g = H.build(items, M=16, M0=32, ef_construction=100, batch_frac=frac, batch_max=bmax)
np.savez(sys.argv[2], entry_points=g.entry_points, max_level=g.max_level, rec_item=g.rec_item,
         rec_layer=g.rec_layer, offsets=g.offsets, nbrs=g.nbrs, n_evals_walk=g.n_evals_walk,
         n_links_added=g.n_links_added, n_batches=g.n_batches)
"""


def _clustered(seed, n):
    rng = np.random.default_rng(seed)
    cent = rng.uniform(-1, 1, (16, DIM)).astype(np.float32)
    return (cent[rng.integers(0, 16, n)] + 0.25 * rng.standard_normal((n, DIM))).astype(np.float32)


def _case(orc, tmp, name, vecs, levels, frac, bmax):
    """the item set as a file for the children, and the oracle's graph with the same schedule"""
    ds = orc.Dataset.from_f32(orc.COSINE, vecs, levels)
    path = os.path.join(str(tmp), name + ".npz")
    np.savez(path, dim=DIM, ids=ds.ids, codes=ds.codes, headers=ds.headers, levels=ds.levels)
    o = orc.build(ds, M=M, M0=M0, ef=EF, order=orc.ORDER_WAVE, threads=8, batch_frac=frac, batch_max=bmax)
    return {"items": path, "oracle": o, "frac": frac, "bmax": bmax, "tmp": str(tmp), "name": name}


def _child_build(case, tag, expect_error=None, **env):
    out = os.path.join(case["tmp"], f"{case['name']}_{tag}.npz")
    e = dict(os.environ)
    for k in ("HNY_WALK_RESIDENT", "HNY_XCD_TILE", "HNY_POOL_FORCE_RETRY", "HNY_WALK_SLOTS"):
        e.pop(k, None)
    e.update({k: str(v) for k, v in env.items()})
    r = subprocess.run([sys.executable, "-c", CHILD, case["items"], out, ROOT, repr(case["frac"]), str(case["bmax"])],
                       env=e, capture_output=True, text=True, timeout=300)
    if expect_error is not None:
        assert r.returncode != 0 and expect_error in r.stderr, r.stderr[-2000:]
        return None
    assert r.returncode == 0, r.stderr[-2000:]
    return types.SimpleNamespace(**np.load(out))


@pytest.fixture(scope="module")
def tiled_case(orc, tmp_path_factory):
    """6 000 x 768 cosine, batch_max 4 096: the level-0 group ends in a batch of about 3 000 members, the only one
    of at least 2 048 (locality order); with HNY_XCD_TILE=64 that is 16 tiles and more (the tiled queue): about
    47 tiles on 8 counters, every counter serves five or six tiles, the last tile is not full.  (ONE tiled batch,
    not several of 64 tiles: 6 000 items with a doubling schedule have no second batch of 2 048 members.)"""
    from conftest import draw_levels
    n = 6000
    return _case(orc, tmp_path_factory.mktemp("walk_resident"), "tiled", _clustered(61, n), draw_levels(n, M, seed=8),
                 1.0, 4096)


@pytest.fixture(scope="module")
def short_case(orc, tmp_path_factory):
    """2 100 items, 40 of them on level 1 and batch_frac 100: the level-0 group is ONE batch of 2 060 members,
    just above the 2 048 the locality order asks for — 32 tiles of 64 and a last one of 12"""
    n = 2100
    levels = np.zeros(n, np.uint8)
    levels[:40] = 1
    return _case(orc, tmp_path_factory.mktemp("walk_resident_short"), "short", _clustered(62, n), levels, 100.0, 4096)


@pytest.mark.parametrize("waves_per_cu", [16, 4, 1])
def test_tiled_walk_equals_oracle_at_every_residency(tiled_case, waves_per_cu):
    """4 096 (= walk_slots), 1 024 and 256 resident waves on the tiled queue of the 3 000-member batch: with 256 waves
    (32 per counter) every wave claims members from several tiles of its XCD"""
    g = _child_build(tiled_case, f"r{waves_per_cu}", HNY_XCD_TILE=64, HNY_WALK_RESIDENT=waves_per_cu)
    same_graph(g, tiled_case["oracle"])


@pytest.mark.parametrize("tile,waves_per_cu", [(64, 1), (64, 4), (256, 1)])
def test_partial_last_tile_and_untiled_fallback(short_case, tile, waves_per_cu):
    """2 060 members: tiles of 64 leave a last tile of 12 members (a counter runs past the end in the middle of a
    tile and its waves steal from the next XCD); tiles of 256 would be fewer than 16, so the launch falls back to
    the single counter on walk_slots waves whatever the residency asked for"""
    g = _child_build(short_case, f"t{tile}r{waves_per_cu}", HNY_XCD_TILE=tile, HNY_WALK_RESIDENT=waves_per_cu)
    same_graph(g, short_case["oracle"])


def test_heap_retry_behind_reduced_residency(tiled_case):
    """HNY_POOL_FORCE_RETRY=3: every third member of every walk launch is handed to k_walk_heap, behind a tiled
    launch of 1 024 waves; the heap kernel's evaluations are the ones counted"""
    g = _child_build(tiled_case, "retry", HNY_XCD_TILE=64, HNY_WALK_RESIDENT=4, HNY_POOL_FORCE_RETRY=3)
    same_graph(g, tiled_case["oracle"])


@pytest.mark.parametrize("value", [-1, 257])
def test_switch_is_read_when_the_builder_is_created(short_case, value):
    """the graph cannot show that the switch was read (it is the same for every value): a value outside 0 .. 256
    waves per CU is refused by the creation of the builder, under the name the other cases set"""
    _child_build(short_case, f"bad{value}", expect_error=f"HNY_WALK_RESIDENT={value}", HNY_WALK_RESIDENT=value)
