"""Which specialised kernel instance a configuration runs, by enumeration ("Which test runs which
instance").  Not a test file: tests/test_kernel_instances_cpu.py holds the table against the rule, and
tests/test_gpu_kernel_instances.py runs every case of it against the oracle.

A configuration is (metric, dim, ef_construction, ef_search, prune_n8) with M = 8, M0 = 16.  The library's own form
functions (hny_internal_launch_forms, as tests/test_capi_forms_cpu.py calls it) and shape_of resolve it to instance keys

  ("walk", L, C, sp, rm, rc)     k_walk<L, C, false, sp, rm, rc>: the build walk (rm 0) and the Reader's walk (rm 1)
  ("prune", kind, L, C, sp)      kind "n8": k_prune_n8<L, sp>; "wg": k_prune_wg<L, C, sp>
  ("apply", kind, L, C, sp)      kind "n8": k_apply_n8<L, sp>; "wg": k_apply_wg<L, C, sp>; "wave": k_apply<L, C, sp>

Only sp != 0 counts: the general kernels (sp 0: strict mode, incremental builders, M0 > 64, and the one-wave k_prune
of rows beyond 8 KB) are what the update, strict and incremental tests run.  CASES is the greedy cover of every key that
the axes below can reach: the configurations in axis order, each kept if it adds a key."""
import ctypes as C

from test_gpu_row_shapes import EDGES, SHAPES, shape_of

M, M0 = 8, 16
METRICS = range(7)
BIT_CODES = 3  # metrics from here on are rows of bits: 128 dimensions per 16-byte unit
# ef_construction -> beam of the build walk: 32 one register chunk (rows <= 512 B), 100 two, 128 the LDS beam (129
# entries need rcap 256); 512 (rcap 1 024 > 512) sends the candidate lists of short rows to k_prune_wg<L, 1, SP>
EF_CONSTRUCTION = (32, 100, 128, 512)
EF_SEARCH = (40, 200)  # rcap 64: two register chunks (the Reader's walk never takes one); rcap 256: the LDS beam
SHORT = [s for s in SHAPES if s[0] <= 32]  # one chunk per lane, at most 32 lanes: rows of at most 512 B
PRUNE_KIND = {0: "n8", 1: "wg", 2: "wave"}
APPLY_KIND = {0: "n8", 1: "wg", 2: "wave"}


def dim_of(metric, shape):
    """f32 metrics: the lower, odd edge of the shape, so the last 16-byte unit is zero padded.  Bit codes: the first
    unit count of the shape with 37 bits in its last unit (27 bits of that word and the whole second word are
    padding); the shortest rows take their last unit count instead, 933 bits, where equal distances are rarer than at
    the 293 bits of their third"""
    s = SHAPES.index(shape)
    if metric < BIT_CODES:
        return EDGES[s][0]
    units = 8 if s == 0 else EDGES[s][0] // 4 + 1  # EDGES[s][0] = 4 * (units of the shape below) + 1
    return (units - 1) * 128 + 37


for _m in METRICS:
    for _s in SHAPES:
        _d = dim_of(_m, _s)
        assert shape_of(_m, _d) == _s, (_m, _s, _d)
        assert _m < BIT_CODES or (_d >= 257 and _d % 64), (_m, _s, _d)


def _load_forms():
    try:
        import hannoy_amd
        fn = hannoy_amd.load_library().hny_internal_launch_forms
    except (OSError, AttributeError, ImportError) as e:
        raise ImportError("tests/kernel_instances.py needs the built library (hny_internal_launch_forms): run "
                          "__graft_entry__.build() first") from e
    fn.restype = C.c_int
    fn.argtypes = [C.POINTER(C.c_int32), C.POINTER(C.c_int32)]

    def call(metric, dim, ef, reader, n8):
        # metric, dim, M, M0, ef, entry points, strict, incremental, reader, HNY_NO_FAST, HNY_NO_RB, HNY_RB_ONE, HNY_PRUNE_N8
        out = (C.c_int32 * 12)()
        rc = fn((C.c_int32 * 13)(metric, dim, M, M0, ef, 1, 0, 0, reader, 0, 0, 1, n8), out)
        if rc != 0:
            raise RuntimeError(f"hny_internal_launch_forms{(metric, dim, ef, reader, n8)} returned {rc}")
        return tuple(out)
    return call


_forms = _load_forms()


def keys_of(config):
    """the specialised instances a configuration runs: its build (walk, prune, apply) and its Reader's walk"""
    metric, dim, efc, efs, n8 = config
    L, Cn = shape_of(metric, dim)
    build = _forms(metric, dim, efc, 0, n8)
    reader = _forms(metric, dim, efs, 1, n8)
    keys = set()
    for sp, _, rm, rc, _ in (build[:5], reader[:5]):
        if sp:
            keys.add(("walk", L, Cn, sp, rm, rc))
    if build[6]:
        keys.add(("prune", PRUNE_KIND[build[5]], L, Cn, build[6]))
    if build[9]:
        keys.add(("apply", APPLY_KIND[build[8]], L, Cn, build[9]))
    return frozenset(keys)


def all_configs():
    """the full product of the axes, then the seven HNY_PRUNE_N8=0 configurations: one short shape per metric"""
    out = []
    for metric in METRICS:
        for shape in SHAPES:
            for efc in EF_CONSTRUCTION:
                if efc == 512 and shape not in SHORT:
                    continue
                for efs in EF_SEARCH:
                    out.append((metric, dim_of(metric, shape), efc, efs, 1))
    for metric in METRICS:
        out.append((metric, dim_of(metric, SHORT[metric % len(SHORT)]), EF_CONSTRUCTION[0], EF_SEARCH[0], 0))
    return out


def greedy_cover(configs):
    seen, cases = set(), []
    for c in configs:
        k = keys_of(c)
        if k - seen:
            seen |= k
            cases.append(c)
    return cases


CASES = greedy_cover(all_configs())


def key_name(key):
    return ".".join(str(x) for x in key)


def case_id(config):
    metric, dim, efc, efs, n8 = config
    head = f"m{metric}-d{dim}-efc{efc}-efs{efs}" + ("" if n8 else "-n8off")
    return head + ":" + "+".join(key_name(k) for k in sorted(keys_of(config), key=str))
