"""NaN, infinite, zero-norm, tiny and denormal vectors through the distance kernels, the walk, the prune, updates
and the searcher.  The reference takes such rows as they come (Writer::add_item does not look at the values), and
they are what drives the walk's rarest bookkeeping: a NaN distance is neither `>` nor `<` anything (hnsw.rs:485,
505) but sorts last by its bits (ordered_float.rs:25-29), so a full result set whose maximum is a NaN admits
nothing more and the walk drains its candidates; +inf ties by the hundred overflow the 128-slot tie pool; an
all-zero row under Cosine is at distance 0.0 from everything.

Every graph comparison is on a dataset of ONE kind: all its NaN distances then share one bit pattern on each
side, no f32 metric yields a negative distance, so the (bits, id) order is the same on both sides whatever the
pattern is, and the graphs must be identical.  `mixed` (propagated and generated NaNs in one index) builds under
Manhattan (fabs clears the sign) and Cosine (a propagated NaN gives 0.0) only: DESIGN.md §4."""
import functools

import numpy as np
import pytest

from conftest import draw_levels
from support import hny, same_graph, same_hits  # noqa: F401

pytestmark = pytest.mark.gpu

EPS = float(np.finfo(np.float32).eps)       # f32::EPSILON, cosine.rs:45
DENORM_ULP = float(np.float32(2.0 ** -149))  # spacing of the f32 denormals
KINDS = ("nan", "inf", "huge", "zero", "tiny", "denormal", "mixed")


def special_vectors(kind, n, dim, seed):
    """U(-1, 1) f32 rows with one kind of special row applied; returns (vectors, mask of the special rows)"""
    rng = np.random.default_rng(seed)
    v = rng.uniform(-1, 1, (n, dim)).astype(np.float32)
    special = np.zeros(n, bool)
    order = rng.permutation(n)
    used = 0

    def take(k):
        nonlocal used
        rows = order[used:used + k]
        used += k
        special[rows] = True
        return rows
    for k in (("nan", "inf", "zero") if kind == "mixed" else (kind,)):
        if k == "nan":  # one NaN component: NaN under Euclidean / Manhattan, 0.0 under Cosine (the norm is NaN)
            rows = take(40)
            v[rows, rng.integers(0, dim, len(rows))] = np.nan
        elif k == "inf":  # +inf from everything; inf - inf between two of them: a GENERATED NaN
            rows = take(40)
            v[rows, 5 % dim] = np.inf
            v[rows[:10], 7 % dim] = -np.inf
        elif k == "huge":  # every squared term overflows: Euclidean +inf, Cosine norm inf
            rows = take(n * 15 // 100)
            v[rows] *= np.float32(1e20)
        elif k == "zero":  # Cosine: pn * qn <= EPSILON, distance 0.0 to every item
            rows = take(n // 10)
            v[rows] = 0.0
            v[rows[0], ::2] = -0.0
        elif k == "tiny":  # Cosine: far above EPSILON against a normal row, far below between two of them
            rows = take(40)
            v[rows] *= np.float32(1e-6)
        elif k == "denormal":  # f32 denormals: L1 / L2 between two such rows are denormal or underflow
            rows = take(40)
            v[rows] *= np.float32(1e-40)
        else:
            raise ValueError(k)
    return v, special


def _mk(orc, hny, metric, vecs, levels, ids=None):
    ds = orc.Dataset.from_f32(metric, vecs, levels, ids)
    items = hny.ItemSet(metric, vecs.shape[1], ds.ids, ds.codes, ds.headers, ds.levels)
    return ds, items


def _same_dists(got, want, tag=None):
    """bit for bit where the oracle's distance is not a NaN (±inf, 0.0 and denormals included), NaN where it is"""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, tag
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), tag
    assert np.array_equal(got.view(np.uint32)[~nan], want.view(np.uint32)[~nan]), tag


def _nan_patterns(d):
    return sorted(set(int(b) for b in d.view(np.uint32)[np.isnan(d)]))


# ---------------------------------------------------------------------------------------------------------
# 1. pair distances
# ---------------------------------------------------------------------------------------------------------
def _formula(metric, A, B):
    """The reference's formulas in plain numpy: elementwise terms in f32 (overflow and inf - inf happen as in f32),
    sums in f64, finalised in f32 as cosine.rs:40-56 / euclidean.rs:42-44 / manhattan.rs:41-43 do.
    Returns (distances f32, mask of the pairs that took Cosine's EPSILON branch)."""
    with np.errstate(all="ignore"):
        if metric == 0:
            pq = (A * B).sum(1, dtype=np.float64).astype(np.float32)
            pn = np.sqrt((A * A).sum(1, dtype=np.float64).astype(np.float32))
            qn = np.sqrt((B * B).sum(1, dtype=np.float64).astype(np.float32))
            pnqn = pn * qn
            c = pq / pnqn
            c = np.where(c < -1, np.float32(-1), c)  # f32::clamp: a NaN stays a NaN
            c = np.where(c > 1, np.float32(1), c)
            d = ((np.float32(1) - c) / np.float32(2)).astype(np.float32)
            big = pnqn > np.float32(EPS)
            return np.where(big, d, np.float32(0)).astype(np.float32), ~big
        t = A - B
        t = t * t if metric == 1 else np.abs(t)
        return t.sum(1, dtype=np.float64).astype(np.float32), np.zeros(len(A), bool)


def _pairs(rng, metric, vecs, special, npairs=4000):
    """4 000 pairs, 600 of them between two special rows, identical operands (special ones too) among them.  A partner
    is drawn again while pn * qn lies within a factor 2 of f32::EPSILON (which branch of cosine.rs:45 is taken).
    Returns (a, c, pn * qn in f64, mask of the pairs whose CLASS the formula decides).  The mask leaves out the Cosine
    pairs whose dot product has a finite exact value although an intermediate can overflow (sum of the |products|
    beyond f32::MAX — rows x 1e20 in few dimensions): +-inf, NaN or finite depending on the summation order and on
    whether a product is rounded before it is added (fmaf).  The oracle in the same order decides those, and they
    stay in that comparison.  (Squared L2, L1 and the norms add non-negative terms: they overflow in every order or
    in none.)"""
    n = len(vecs)
    a = rng.integers(0, n, npairs).astype(np.uint32)
    c = rng.integers(0, n, npairs).astype(np.uint32)
    sp = np.flatnonzero(special)
    a[:600] = rng.choice(sp, 600)
    c[:600] = rng.choice(sp, 600)
    c[:60] = a[:60]
    c[600:700] = a[600:700]
    v64 = vecs.astype(np.float64)
    fmax = float(np.finfo(np.float32).max)
    with np.errstate(all="ignore"):
        norm = np.sqrt((v64 ** 2).sum(1))
    for _ in range(50):
        with np.errstate(all="ignore"):
            pnqn = norm[a] * norm[c]
        bad = np.flatnonzero((pnqn > EPS / 2) & (pnqn < EPS * 2))
        if not len(bad):
            break
        c[bad] = rng.integers(0, n, len(bad))
    assert not len(bad)
    decided = np.ones(npairs, bool)
    if metric == 0:
        with np.errstate(all="ignore"):
            p = v64[a] * v64[c]
        p = np.where(np.isfinite(p), p, 0.0)
        decided = ~((np.abs(p).sum(1) > fmax) & (np.abs(p.sum(1)) <= fmax))
    return a, c, pnqn, decided


PAIR_DIMS = (3, 20, 48, 100, 768, 2500)  # scalar / SSE / AVX strict paths, 1-chunk and multi-chunk wave shapes


@pytest.mark.parametrize("dim", PAIR_DIMS)
@pytest.mark.parametrize("metric", (0, 1, 2))
def test_pair_distances_of_special_rows(orc, hny, metric, dim):
    """hny_builder_distances on every kind of special row, wave order and strict mode.  Against the oracle in the
    same order: equal bits wherever its result is not a NaN (±inf, 0.0, denormals), NaN where it is.  Against the
    formula in numpy (f32 terms, f64 sums): the same class for every pair — NaN, +inf, exactly 0.0 from Cosine's
    EPSILON branch, finite — and finite values within the suite's bounds (1e-6 absolute on (1 - cos) / 2, 1e-5
    relative on squared L2 and L1; denormal sums: within one denormal ulp per component).  Each side writes at
    most one NaN pattern per single-kind dataset (printed: the table of DESIGN.md §4)."""
    n = 300
    lv = np.zeros(n, np.uint8)
    lv[0] = 1
    for kind in KINDS:
        seed = 1000 * dim + 10 * metric + KINDS.index(kind)
        vecs, special = special_vectors(kind, n, dim, seed)
        a, c, pnqn, decided = _pairs(np.random.default_rng(seed + 1), metric, vecs, special)
        assert int((special[a] & special[c]).sum()) >= 500 and int((a == c).sum()) >= 160
        assert not np.any((pnqn > EPS / 2) & (pnqn < EPS * 2)) and decided.sum() >= 0.9 * len(a)
        ds, items = _mk(orc, hny, metric, vecs, lv)
        ref, eps_branch = _formula(metric, vecs[a], vecs[c])
        for mode, order in (("wave", orc.ORDER_WAVE), ("x86", orc.ORDER_X86)):
            tag = (metric, dim, kind, mode)
            with hny.Builder(items, M=4, M0=8, x86_order=(mode == "x86")) as b:
                got = b.distances(a, c)
            want = orc.distance_pairs(ds, order, a, c, threads=8)
            gp, wp = _nan_patterns(got), _nan_patterns(want)
            print(f"NANPAT metric={metric} dim={dim} kind={kind} mode={mode} "
                  f"device={[hex(p) for p in gp]} oracle={[hex(p) for p in wp]} n_nan={int(np.isnan(want).sum())} "
                  f"n_inf={int(np.isinf(want).sum())} n_zero={int((want == 0).sum())}")
            _same_dists(got, want, tag)
            if kind != "mixed":
                assert len(gp) <= 1 and len(wp) <= 1, tag
            # classes against the formula, where the formula decides them
            assert np.array_equal(np.isnan(got)[decided], np.isnan(ref)[decided]), tag
            assert np.array_equal(np.isposinf(got)[decided], np.isposinf(ref)[decided]), tag
            assert not np.isneginf(got).any() and not np.isneginf(ref).any(), tag
            assert np.all(got.view(np.uint32)[eps_branch & decided] == 0), tag
            fin = np.isfinite(ref) & decided
            err = np.abs(got[fin].astype(np.float64) - ref[fin].astype(np.float64))
            if metric == 0:
                assert err.max() <= 1e-6, tag
            elif kind == "denormal":
                assert np.all(err <= np.maximum(1e-5 * ref[fin], dim * DENORM_ULP)), tag
            else:
                assert np.max(err / np.maximum(ref[fin], 1e-30)) <= 1e-5, tag
            if kind == "denormal" and metric == 2 and dim <= 100:  # contains what it is there for: denormal sums
                assert np.any((want > 0) & (want < np.finfo(np.float32).tiny)), tag


# ---------------------------------------------------------------------------------------------------------
# 2. fresh builds
# ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cache():
    """datasets and oracle graphs, made once per case and shared by the tests of this module that need them"""
    c = {}
    yield c
    c.clear()


def _data(cache, orc, hny, metric, kind, n, dim, M):
    key = ("data", metric, kind, n, dim, M)
    if key not in cache:
        vecs, special = special_vectors(kind, n, dim, seed=7 * n + dim + KINDS.index(kind))
        ds, items = _mk(orc, hny, metric, vecs, draw_levels(n, M, seed=n + dim))
        cache[key] = (vecs, special, ds, items)
    return cache[key]


def _oracle(cache, orc, metric, kind, ds, M, M0, ef, frac, bmax, x86=False):
    """the oracle's graph of a case, checked once for what the case is there for"""
    key = ("oracle", metric, kind, ds.n, ds.dim, M, M0, ef, frac, bmax, x86)
    if key not in cache:
        if x86:  # batch_max 0: the reference's own loop, one thread, its x86 summation order
            o = orc.build(ds, M=M, M0=M0, ef=ef, order=orc.ORDER_X86)
        else:
            o = orc.build(ds, M=M, M0=M0, ef=ef, order=orc.ORDER_WAVE, batch_frac=frac, batch_max=bmax)
        _guard(orc, metric, kind, ds, o, ef, x86)
        cache[key] = o
    return cache[key]


def _guard(orc, metric, kind, ds, o, ef, x86=False):
    """Does the oracle's build contain the distances this kind is there for?  (raw_dists: the distances stored
    with the links of the finished graph, i.e. of candidates that went through walk and prune.)"""
    d = o.raw_dists
    n_nan, n_inf, n_zero = int(np.isnan(d).sum()), int(np.isposinf(d).sum()), int((d == 0).sum())
    expects_nan = kind == "inf" or (kind in ("nan", "mixed") and metric != 0)  # (Cosine: a NaN norm gives 0.0)
    if expects_nan and kind == "inf" and metric != 0:
        # An infinite row is at +inf from every ordinary row and at NaN from its like; the prune takes the +inf
        # candidates first, so no link carries a NaN.  What shows that NaN keys sat next to +inf keys in a beam: the
        # oracle's walk of the finished layer 0 from the infinite rows themselves, with a result set of the build's
        # size (Reader::nns by_item, k = ef_search = ef_construction), returns NaN distances.
        f = ds.codes.view(np.float32)
        sp = ds.ids[np.isinf(f).any(1)]
        _, sd, sc = orc.search(ds, o, None, None, k=ef, ef_search=ef, order=orc.ORDER_X86 if x86 else orc.ORDER_WAVE,
                               query_items=sp)
        hits = np.concatenate([sd[r, :int(sc[r])] for r in range(len(sp))])
        assert np.isnan(hits).any() and np.isposinf(hits).any(), (metric, kind, "no NaN candidate next to +inf ones")
        assert n_inf > 0, (metric, kind, "no +inf link")
    elif expects_nan:
        assert n_nan > 0, (metric, kind, "no NaN-distance link")
    if kind == "huge" and metric == 1:
        # one ordinary row sees all the huge rows at +inf: more ties at the maximum than the 128-slot pool holds
        first = int(np.flatnonzero(np.isfinite(ds.codes.view(np.float32)).all(1) &
                                   (np.abs(ds.codes.view(np.float32)).max(1) <= 1))[0])
        row = orc.distance_pairs(ds, orc.ORDER_X86 if x86 else orc.ORDER_WAVE,
                                 np.full(ds.n, first, np.uint32), np.arange(ds.n, dtype=np.uint32))
        assert int(np.isposinf(row).sum()) > min(128, ds.n // 8) and n_inf > 0, (metric, kind)  # (n = 400: 60 rows)
    if metric == 0 and kind in ("zero", "nan", "denormal", "tiny", "mixed"):
        assert n_zero > 50, (metric, kind, "no ties at 0.0")  # the zero-norm hub
    if kind == "denormal" and metric == 2:
        assert np.any((d > 0) & (d < np.finfo(np.float32).tiny)), "no denormal link distance"


WALK_CASES = [(m, k) for m in (0, 1, 2) for k in KINDS if not (m == 1 and k == "mixed")]
KNOBS = {"default": {},                               # register beam, one-wave prune
         "lds_beam": {"HNY_NO_RB": "1"},              # beam_insert, pool_drop_ties
         "general": {"HNY_NO_FAST": "1"},             # the general kernels
         "heap_walk": {"HNY_POOL_FORCE_RETRY": "1"}}  # k_walk_heap with NaN / inf keys


@pytest.mark.parametrize("knob", list(KNOBS))
@pytest.mark.parametrize("metric,kind", WALK_CASES)
def test_build_with_special_rows_equals_oracle(cache, orc, hny, monkeypatch, metric, kind, knob):
    """dim 48, M 8 / M0 16, ef 40, batched (0.05, 64) and one member at a time: the oracle's graph, link count and
    walk evaluations on the default kernels, the LDS beam, the general kernels and the heap walk"""
    for k, v in KNOBS[knob].items():
        monkeypatch.setenv(k, v)
    M, M0, ef = 8, 16, 40
    for n, frac, bmax in ((1200, 0.05, 64), (400, 0.05, 1)):
        _, _, ds, items = _data(cache, orc, hny, metric, kind, n, 48, M)
        o = _oracle(cache, orc, metric, kind, ds, M, M0, ef, frac, bmax)
        g = hny.build(items, M=M, M0=M0, ef_construction=ef, batch_frac=frac, batch_max=bmax)
        assert g.n_tie_pool_overflow == 0
        same_graph(g, o)


def test_inf_ties_overflow_the_tie_pool_naturally(cache, orc, hny):
    """Euclidean, 15 % of the rows x 1e20: an ordinary query sees 225 candidates at +inf.  M0 = 96 and ef 64 put
    more of them at res.max than the 128-slot pool holds; the walk is repeated on heaps without being told to."""
    metric, kind, n, dim, M, M0, ef = 1, "huge", 1500, 48, 16, 96, 64
    _, _, ds, items = _data(cache, orc, hny, metric, kind, n, dim, M)
    o = _oracle(cache, orc, metric, kind, ds, M, M0, ef, 0.05, 64)
    g = hny.build(items, M=M, M0=M0, ef_construction=ef, batch_frac=0.05, batch_max=64)
    assert g.n_tie_pool_overflow == 0
    same_graph(g, o)


@pytest.mark.parametrize("n8", ["1", "0"])
def test_prune_of_zero_distance_ties(cache, orc, hny, monkeypatch, n8):
    """Cosine with zero rows, 24-d (96-B rows): k_prune_n8 / k_apply_n8 and the workgroup prune on lists whose
    candidates tie at 0.0"""
    monkeypatch.setenv("HNY_PRUNE_N8", n8)
    metric, kind, n, dim, M, M0, ef = 0, "zero", 1500, 24, 8, 16, 40
    _, _, ds, items = _data(cache, orc, hny, metric, kind, n, dim, M)
    o = _oracle(cache, orc, metric, kind, ds, M, M0, ef, 0.05, 64)
    same_graph(hny.build(items, M=M, M0=M0, ef_construction=ef, batch_frac=0.05, batch_max=64), o)


@pytest.mark.parametrize("metric,kind,n,dim,M,M0,ef", [
    (1, "nan", 800, 768, 8, 16, 40),     # k_prune_wg, 3 KB rows
    (0, "inf", 500, 2500, 8, 16, 40),    # multi-chunk walk
    (1, "nan", 1200, 48, 8, 16, 300),    # result sets beyond the register beam
    (1, "nan", 1200, 40, 16, 200, 40),   # paged lists
    (1, "inf", 1200, 40, 16, 200, 40)])
def test_long_rows_wide_beams_and_paged_lists_with_nan_distances(cache, orc, hny, metric, kind, n, dim, M, M0, ef):
    _, _, ds, items = _data(cache, orc, hny, metric, kind, n, dim, M)
    o = _oracle(cache, orc, metric, kind, ds, M, M0, ef, 0.05, 64)
    g = hny.build(items, M=M, M0=M0, ef_construction=ef, batch_frac=0.05, batch_max=64)
    assert g.n_tie_pool_overflow == 0
    same_graph(g, o)


STRICT_KINDS = {0: ("zero", "inf", "tiny"), 1: ("nan", "inf", "huge"), 2: ("nan", "inf", "denormal")}


@pytest.mark.parametrize("dim", (20, 48, 100))
@pytest.mark.parametrize("metric", (0, 1, 2))
def test_strict_mode_with_special_rows_equals_x86_oracle(cache, orc, hny, metric, dim):
    """x86_order, one member at a time, against the oracle's restatement of the reference's own loop in its x86
    summation order (SSE below 16 lanes of 8, AVX above)"""
    M, M0, ef, n = 8, 16, 40, 400
    for kind in STRICT_KINDS[metric]:
        _, _, ds, items = _data(cache, orc, hny, metric, kind, n, dim, M)
        o = _oracle(cache, orc, metric, kind, ds, M, M0, ef, 0.0, 0, x86=True)
        g = hny.build(items, M=M, M0=M0, ef_construction=ef, batch_max=1, x86_order=True)
        same_graph(g, o)


def test_f32_ingest_of_inf_rows_builds_the_same_graph(cache, orc, hny):
    """hny_build_f32: k_ingest's norms of rows with ±inf components (inf) equal the host encoder's, the build on
    device-encoded rows equals the build on host codes and the oracle's"""
    metric, kind, n, dim, M, M0, ef = 0, "inf", 1200, 48, 8, 16, 40
    vecs, _, ds, items = _data(cache, orc, hny, metric, kind, n, dim, M)
    o = _oracle(cache, orc, metric, kind, ds, M, M0, ef, 0.05, 64)
    f32 = hny.ItemSet.from_f32(metric, vecs, levels=ds.levels, device=True)
    g = hny.build(f32, M=M, M0=M0, ef_construction=ef, batch_frac=0.05, batch_max=64)
    same_graph(g, o)
    with hny.Builder(f32, M=M, M0=M0, ef_construction=ef) as b:
        codes, hdrs = b.export_items()
    assert np.array_equal(codes, ds.codes)
    assert np.array_equal(hdrs, ds.headers)  # norms: +inf, bit for bit


# ---------------------------------------------------------------------------------------------------------
# 3. updates
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric,kind", [(1, "nan"), (1, "inf"), (0, "zero")])
def test_update_with_special_rows(orc, hny, metric, kind):
    """From a finished build: half of the special rows deleted, some overwritten with finite vectors, some finite
    rows overwritten with special ones, 100 rows added.  hny_build_incremental == the oracle's incremental build
    (k_fill_gaps, the on-disk-links pass of the walk), and hny_builder_update from the resident builder ==
    hny_build_incremental."""
    n0, dim, M, M0, ef = 1200, 40, 8, 16, 40
    rng = np.random.default_rng(31 + metric)
    allv, special = special_vectors(kind, n0 + 100, dim, seed=5 + KINDS.index(kind))
    donors, dsp = special_vectors(kind, 400, dim, seed=77)
    donors = donors[dsp]
    kw_o = dict(M=M, M0=M0, ef=ef, order=orc.ORDER_WAVE, batch_frac=0.1, batch_max=64)
    kw_g = dict(M=M, M0=M0, ef_construction=ef, batch_frac=0.1, batch_max=64)
    ds, items = _mk(orc, hny, metric, allv[:n0], draw_levels(n0, M, seed=1))
    og = orc.build(ds, **kw_o)
    _guard(orc, metric, kind, ds, og, ef)
    gg = hny.build(items, **kw_g)
    same_graph(gg, og)

    sp = np.flatnonzero(special[:n0])
    sp = sp[rng.permutation(len(sp))]
    to_delete = np.sort(sp[:len(sp) // 2]).astype(np.uint32)
    made_finite = sp[len(sp) // 2:len(sp) // 2 + 8]
    ordinary = np.setdiff1d(np.flatnonzero(~special[:n0]), to_delete)
    made_special = rng.choice(ordinary, 15, replace=False)
    vecs = allv.copy()
    vecs[made_finite] = rng.uniform(-1, 1, (len(made_finite), dim)).astype(np.float32)
    vecs[made_special] = donors[:15]
    vecs[n0:n0 + 6] = donors[15:21]  # special rows among the new ones, whatever the generator drew
    alive = np.setdiff1d(np.arange(n0 + 100, dtype=np.uint32), to_delete)
    to_insert = np.sort(np.concatenate([made_finite, made_special, np.arange(n0, n0 + 100)])).astype(np.uint32)
    lv = draw_levels(len(to_insert), M, seed=9)
    ds2 = orc.Dataset.from_f32(metric, vecs[alive], np.zeros(len(alive), np.uint8), alive)
    items2 = hny.ItemSet(metric, dim, ds2.ids, ds2.codes, ds2.headers, lv)
    og2 = orc.build_incremental(ds2, og, to_insert, lv, to_delete, **kw_o)
    _guard(orc, metric, kind, ds2, og2, ef)
    gg2 = hny.build_incremental(items2, gg, to_insert, to_delete, **kw_g)
    same_graph(gg2, og2)
    d = gg2.as_dict()
    assert all(set(nb) <= set(alive.tolist()) for nb in d.values())
    with hny.Builder(items, **kw_g) as b:
        b.run()
        same_graph(b.finish(), gg)
        c, h = hny.encode_vectors(metric, vecs[to_insert])
        gb = b.update(to_insert, codes=c, headers=h, delete_ids=to_delete, levels=lv)
        same_graph(gb, gg2)
        codes, hdrs = b.export_items()
        assert np.array_equal(codes, ds2.codes) and np.array_equal(hdrs, ds2.headers)


# ---------------------------------------------------------------------------------------------------------
# 4. search
# ---------------------------------------------------------------------------------------------------------
equal_hits = functools.partial(same_hits, dists=_same_dists)  # a NaN is a NaN, whatever its bits


@pytest.mark.parametrize("metric,kind", [(1, "nan"), (1, "inf"), (0, "zero"), (1, "huge"), (0, "inf"), (2, "nan")])
def test_search_on_graphs_with_special_rows(cache, orc, hny, metric, kind):
    """The restated Reader's ids, counts and distances on the graphs of part 2, for 64 queries of which one has a
    NaN component, one an infinite one and one is all zero: k-NN at ef_search 50 and at ef_search = n, a filtered
    search above and one below `linear_below` (k_nns_linear), by_item on special items."""
    n, dim, M, M0, ef = 1200, 48, 8, 16, 40
    vecs, special, ds, items = _data(cache, orc, hny, metric, kind, n, dim, M)
    o = _oracle(cache, orc, metric, kind, ds, M, M0, ef, 0.05, 64)
    rng = np.random.default_rng(50 + metric)
    qs = rng.uniform(-1, 1, (64, dim)).astype(np.float32)
    qs[0, 3] = np.nan
    qs[1, 5] = np.inf
    qs[2] = 0.0
    qc = orc.encode_vectors(metric, qs)
    qh = orc.make_headers(metric, dim, qc)
    sp = np.flatnonzero(special).astype(np.uint32)
    qi = np.concatenate([sp[:24], rng.integers(0, n, 8).astype(np.uint32), [n + 5]]).astype(np.uint32)
    wide = np.flatnonzero(rng.random(n) < 0.5).astype(np.uint32)
    few = np.concatenate([sp[:20], rng.choice(n, 40, replace=False).astype(np.uint32)])
    kw = dict(order=orc.ORDER_WAVE, threads=8)
    with hny.Builder(items, M=M, M0=M0, ef_construction=ef, batch_frac=0.05, batch_max=64) as b:
        b.run()
        same_graph(b.finish(), o)
        for ef_s in (50, n):
            equal_hits(b.search_knn(qc, qh, k=10, ef_search=ef_s),
                       orc.search(ds, o, qc, qh, k=10, ef_search=ef_s, **kw), ("knn", ef_s))
        equal_hits(b.nns(qc, qh, k=10, ef_search=50, candidates=wide, linear_below=100),
                   orc.search(ds, o, qc, qh, k=10, ef_search=50, candidates=wide, linear_below=100, **kw), "filtered")
        equal_hits(b.nns(qc, qh, k=10, ef_search=50, candidates=few, linear_below=1000),
                   orc.search(ds, o, qc, qh, k=10, ef_search=50, candidates=few, linear_below=1000, **kw), "linear")
        equal_hits(b.nns(k=10, ef_search=50, query_items=qi),
                   orc.search(ds, o, None, None, k=10, ef_search=50, query_items=qi, **kw), "by_item")
