"""The evaluation counters of the short-row prune and re-link kernels (k_prune_n8, k_apply_n8), pinned.

n_evals_walk is the reference's count and is compared with the oracle everywhere.  n_evals_prune and
n_evals_apply are what the kernels computed (include/hannoy_amd.h): the prefix filter tests candidates the
reference never reaches, so the oracle cannot say what they should be.  They are integer sums of per-member
values and do not depend on scheduling, so a recording of them pins the S-scan, the filter bounds and the
rule that row j + 1 counts only for the candidates row j did not reject.  The recording
(tests/golden/short_row_eval_counts.json) is made by scripts/record_short_row_eval_counts.py from a library
built at the commit named in it, never from the code under test.
"""
import hashlib
import json
import os

import numpy as np
import pytest

from conftest import draw_levels
from support import NO_COUNTERS, WALK, hny, same_graph  # noqa: F401

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "short_row_eval_counts.json")
RECORDER = "scripts/record_short_row_eval_counts.py"

# (metric, n, dim, M, M0, ef): the smallest builds that reach every branch of the 8-lane row code
CASES = [
    (0, 4000, 128, 16, 32, 100),  # 32 units f32; 12 staged rows against 32 selected: S from L2 too; filter engaged
    (1, 3000, 60, 12, 24, 64),    # 15 units, 16-lane order: p0 + p1
    (2, 3000, 20, 5, 9, 33),      # 5 units, manhattan, odd caps; too few candidates for the filter
    (3, 4000, 1024, 32, 64, 80),  # 8 units of bit codes; 64 selected rows against 48 staged
    (3, 3000, 4096, 16, 32, 64),  # 32 units of bit codes
    (5, 3000, 2000, 16, 64, 64),  # 16 units, binary quantized
]
SCHEDULES = [dict(batch_frac=1.0, batch_max=4096), dict(batch_frac=0.1, batch_max=128)]


def case_key(case):
    return "-".join(str(x) for x in case)


def schedule_key(kw):
    return f"{kw['batch_frac']}/{kw['batch_max']}"


def make_inputs(case):
    """The vectors and levels of test_one_wave_prune_for_short_rows_equals_oracle for this case."""
    _, n, dim, M, _, _ = case
    rng = np.random.default_rng(n + dim)
    cent = rng.uniform(-1, 1, (12, dim)).astype(np.float32)
    vecs = (cent[rng.integers(0, 12, n)] + 0.3 * rng.standard_normal((n, dim))).astype(np.float32)
    return vecs, draw_levels(n, M, seed=7)


def input_sha1(vecs):
    return hashlib.sha1(np.ascontiguousarray(vecs, dtype=np.float32).tobytes()).hexdigest()


@pytest.fixture(scope="module")
def recorded():
    with open(FIXTURE) as f:
        return json.load(f)


@pytest.mark.parametrize("case", CASES, ids=case_key)
def test_short_row_prune_and_apply_counts_equal_the_recording(orc, hny, recorded, monkeypatch, case):
    metric, n, dim, M, M0, ef = case
    vecs, levels = make_inputs(case)
    ds = orc.Dataset.from_f32(metric, vecs, levels)
    items = hny.ItemSet(metric, dim, ds.ids, ds.codes, ds.headers, ds.levels)
    built = []
    for kw in SCHEDULES:
        o = orc.build(ds, M=M, M0=M0, ef=ef, order=orc.ORDER_WAVE, threads=8, **kw)
        g = hny.build(items, M=M, M0=M0, ef_construction=ef, **kw)
        print(case_key(case), schedule_key(kw), "n_evals_prune", g.n_evals_prune, "n_evals_apply", g.n_evals_apply)
        same_graph(g, o, counters=WALK)
        built.append((kw, g))
    rec = recorded["cases"][case_key(case)]
    assert input_sha1(vecs) == rec["input_sha1"], (
        f"numpy draws other vectors here than where {FIXTURE} was recorded: the counts in it belong to other "
        f"data.  Record it again with {RECORDER} (library built at the parent commit, named by HNY_LIB).")
    for kw, g in built:
        want = rec["schedules"][schedule_key(kw)]
        assert (g.n_evals_prune, g.n_evals_apply) == (want["n_evals_prune"], want["n_evals_apply"]), schedule_key(kw)
    if case == CASES[0]:
        # the workgroup kernels serve these rows with HNY_PRUNE_N8=0: their counts are their own and not
        # pinned, their graph is the same
        monkeypatch.setenv("HNY_PRUNE_N8", "0")
        same_graph(hny.build(items, M=M, M0=M0, ef_construction=ef, **kw), o, counters=NO_COUNTERS)
