"""support.py's comparisons on hand-made inputs: each passes on equal inputs and fails on every difference it is
there to find, and on nothing else."""
import copy
import types

import numpy as np
import pytest

from support import LINKS, NO_COUNTERS, NONE, WALK, identical_hits, param_types, same_graph, same_hits

ARRAYS = ("entry_points", "rec_item", "rec_layer", "offsets", "nbrs")
SCALARS = ("max_level", "n_links_added", "n_evals_walk")


def _graph():
    """three records, five links"""
    return types.SimpleNamespace(entry_points=np.array([2], np.uint32), max_level=1,
                                 rec_item=np.array([0, 1, 2], np.uint32), rec_layer=np.array([0, 0, 1], np.uint8),
                                 offsets=np.array([0, 2, 4, 5], np.uint64), nbrs=np.array([1, 2, 0, 2, 0], np.uint32),
                                 n_links_added=9, n_evals_walk=40)


def _bent(field):
    g = copy.deepcopy(_graph())
    if field in ARRAYS:
        getattr(g, field)[-1] += 1
    else:
        setattr(g, field, getattr(g, field) + 1)
    return g


def test_same_graph_passes_on_equal_graphs_at_every_level():
    for counters in (NO_COUNTERS, LINKS, WALK):
        same_graph(_graph(), _graph(), counters=counters)
    same_graph(_graph(), _graph())


@pytest.mark.parametrize("field", ARRAYS + SCALARS)
def test_same_graph_finds_a_difference_in_each_field(field):
    with pytest.raises(AssertionError):
        same_graph(_bent(field), _graph())
    with pytest.raises(AssertionError):
        same_graph(_graph(), _bent(field), counters=WALK, tag="t")


def test_same_graph_finds_a_longer_array():
    g = _graph()
    g.nbrs = np.append(g.nbrs, np.uint32(1))
    with pytest.raises(AssertionError):
        same_graph(g, _graph(), counters=NO_COUNTERS)


def test_same_graph_counter_levels():
    same_graph(_bent("n_links_added"), _graph(), counters=NO_COUNTERS)
    same_graph(_bent("n_evals_walk"), _graph(), counters=NO_COUNTERS)
    same_graph(_bent("n_evals_walk"), _graph(), counters=LINKS)
    with pytest.raises(AssertionError):
        same_graph(_bent("n_links_added"), _graph(), counters=LINKS)
    for field in ARRAYS + ("max_level",):
        with pytest.raises(AssertionError):
            same_graph(_bent(field), _graph(), counters=NO_COUNTERS)
    with pytest.raises(AssertionError):
        same_graph(_graph(), _graph(), counters=("n_evals_walk",))  # not one of the three levels


def _hits():
    """two queries, k = 3: two results and none at all"""
    return (np.array([[5, 9, 0], [0, 0, 0]], np.uint32), np.array([[0.25, 0.5, 0], [0, 0, 0]], np.float32),
            np.array([2, NONE], np.uint32))


def test_same_hits_passes_on_equal_hits_and_ignores_what_lies_beyond_the_count():
    same_hits(_hits(), _hits())
    ids, dists, counts = _hits()
    ids[0, 2], dists[0, 2] = 1234, np.nan
    ids[1], dists[1] = 77, 7.5
    same_hits((ids, dists, counts), _hits(), tag="garbage")
    same_hits(_hits(), (ids, dists, counts))
    with pytest.raises(AssertionError):
        identical_hits((ids, dists, counts), _hits())
    identical_hits(_hits(), _hits())


def test_same_hits_finds_each_difference():
    ids, dists, counts = _hits()
    counts[0] = 1
    with pytest.raises(AssertionError):
        same_hits((ids, dists, counts), _hits())
    ids, dists, counts = _hits()
    counts[1] = 0  # NONE and 0 both mean no rows to compare, but they are different counts
    with pytest.raises(AssertionError):
        same_hits((ids, dists, counts), _hits())
    ids, dists, counts = _hits()
    ids[0, 1] = 8
    with pytest.raises(AssertionError):
        same_hits((ids, dists, counts), _hits())
    ids, dists, counts = _hits()
    dists.view(np.uint32)[0, 1] ^= 1  # one bit of the mantissa
    with pytest.raises(AssertionError):
        same_hits((ids, dists, counts), _hits())
    ids, dists, counts = _hits()
    dists[0, 0] = -0.0
    zero = _hits()
    zero[1][0, 0] = 0.0
    with pytest.raises(AssertionError):
        same_hits((ids, dists, counts), zero)  # equal as floats, not as bit patterns


def test_same_hits_takes_another_distance_comparison():
    seen = []
    ids, dists, counts = _hits()
    dists[0, 1] = 0.75
    same_hits((ids, dists, counts), _hits(), tag="t", dists=lambda a, b, tag: seen.append((a.tolist(), b.tolist(), tag)))
    assert seen == [([0.25, 0.75], [0.25, 0.5], ("t", 0)), ([], [], ("t", 1))]


def test_param_types_reads_a_declaration():
    header = "int hny_f(const hny_builder *b, uint32_t n,\n          float *out);\nuint64_t hny_g(const hny_builder *b);\n"
    assert param_types(header, "hny_f") == ["const hny_builder *", "uint32_t", "float *"]
    assert param_types(header, "hny_g", "uint64_t") == ["const hny_builder *"]
    with pytest.raises(AssertionError):
        param_types(header, "hny_g")
