"""The dynamic LDS of every kernel family that has a layout function, without a GPU: hny_internal_lds_layout runs the
function (hny_internal.h) on a null cursor and returns every array's offset and size, the launch's bytes and the
misalignment flag.  The expected figures below are the byte formulas of the launchers and the cast chains of the
kernels of commit 5810c92 (the parent of the layout functions), written out by hand as plain arithmetic; each names the
lines it was read from (K = hny_kernels.hip, H = hny_host.cpp, I = hny_internal.h at that commit).  Nothing here calls
the library to compute an expected value.  k_walk, k_prune_wg, k_apply_wg and k_fill_gaps_wg have no layout function:
they keep the cast chains and formulas of that commit.

The grid, and what of it the host can produce:
  rcap         64 doubling, everywhere (res_capacity H:495-496, linear_rcap H:3867-3868, exact_dense_run H:4444-4445)
  eps_cap      a multiple of 64, at least 64 (eps_cap_of H:472-475)
  n8 kernels   rows of at most 512 bytes (hnyk_short_rows I:319-321: nch 1, lpr <= 32) and 1 .. 64 staged rows
               (plan_launch H:1574), lists of at most 512 entries (hnyk_prune_form I:326)
  k_fill_gaps  lists of at most 64 slots: maxu = cap * (cap + 1) (GapsLauncher K:4699-4700)
The other sizes are crossed in full: the formulas hold for all of them.
"""
import ctypes as C
import itertools

import pytest

POOL, MAX_CAP = 128, 64  # HNY_POOL_CAP I:15, HNY_MAX_CAP I:12
RCAP = (64, 128, 256, 4096)
EPS_CAP = (64, 128, 4096)
VIS_SLOTS = (0, 512, 1472)
CAPMAX = (64, 128, 256, 768)
ROW_STRIDE = (128, 512, 3072, 8192)
MAXU = tuple(cap * (cap + 1) for cap in (2, 32, 64))
QT = (1, 8, 32)
# enum LdsFamily, hny_internal.h; a family's sizes go in the order of its layout function's parameters
HEAP_WALK, NNS, NNS_LINEAR, EXACT_TOPK, EXACT_SCORES, PRUNE, APPLY, FILL_GAPS, PRUNE_N8, APPLY_N8 = range(10)


@pytest.fixture(scope="module")
def layout():
    import hannoy_amd
    fn = hannoy_amd.load_library().hny_internal_lds_layout
    fn.restype = C.c_int
    fn.argtypes = [C.c_int, C.POINTER(C.c_uint32), C.POINTER(C.c_uint64), C.POINTER(C.c_int32), C.POINTER(C.c_uint64)]

    def call(kernel, *params):
        p = (C.c_uint32 * 4)(*[int(x) for x in params])
        spans = (C.c_uint64 * 64)()
        n = C.c_int32(32)
        out2 = (C.c_uint64 * 2)()
        assert fn(kernel, p, spans, C.byref(n), out2) == 0
        return [(spans[2 * i], spans[2 * i + 1]) for i in range(n.value)], out2[0], out2[1]
    return call


def walk_fixed(rcap, eps_cap):
    """hnyk_walk_lds_bytes, K:4763-4765"""
    return rcap * 8 + POOL * 8 + 64 * 4 * 2 + eps_cap * 4


def cases():
    """(kernel, params, bytes of the parent's launch)"""
    for rcap, eps_cap, vis_slots in itertools.product(RCAP, EPS_CAP, VIS_SLOTS):
        # NnsLauncher K:4663, k_nns<.., false>: the table behind eps_cap entry points (K:2648)
        yield NNS, (rcap, eps_cap, vis_slots), walk_fixed(rcap, eps_cap) + vis_slots * 4
    for eps_cap in EPS_CAP:
        yield HEAP_WALK, (eps_cap,), 64 * 4 * 2 + eps_cap * 4  # WalkHeapLauncher K:4672, NnsLauncher K:4660
    for rcap in RCAP:
        yield NNS_LINEAR, (rcap,), rcap * 8 + 64 * 4 * 2  # NnsLinearLauncher K:4680
        yield EXACT_TOPK, (rcap,), rcap * 8               # hnyk_exact_topk K:4786
    for qt, row_stride in itertools.product(QT, ROW_STRIDE):
        yield EXACT_SCORES, (qt, row_stride), qt * row_stride + qt * 4  # ExactScoresLauncher K:4688
    for rcap, capmax in itertools.product(RCAP, CAPMAX):
        yield PRUNE, (rcap, capmax), rcap * 8 + capmax * (8 + 4) + 64 * 4  # Hot<SP>::Prune K:4626
    for capmax in CAPMAX:
        yield APPLY, (capmax,), capmax * (8 + 8 + 8 + 4) + 64 * 4  # Hot<SP>::Apply K:4648
    for maxu in MAXU:
        # fill_gaps_lds_bytes K:4033-4035
        yield FILL_GAPS, (maxu,), maxu * 4 * 2 + (maxu + MAX_CAP) * 8 * 2 + MAX_CAP * (8 + 4) + 64 * 4

    for sl, row_stride in itertools.product((8, 64), (128, 512)):
        for rcap in (64, 128, 256):
            # prune_n8_lds_bytes K:3551-3553
            yield PRUNE_N8, (rcap, row_stride, sl), rcap * 8 + MAX_CAP * (8 + 4 + 4) + (sl + 1) * row_stride
        # apply_n8_lds_bytes K:3554-3556
        yield APPLY_N8, (row_stride, sl), MAX_CAP * (8 + 8 + 8 + 4 + 4) + (sl + 1) * row_stride


CASES = list(cases())


def test_every_family_is_in_the_grid():
    assert {k for k, _, _ in CASES} == set(range(10))


def test_launch_bytes_equal_the_parent_formulas(layout):
    for kernel, params, want in CASES:
        _, total, _ = layout(kernel, *params)
        assert total == want, (kernel, params)


def test_nns_offsets_equal_the_parent_cast_chain(layout):
    """k_nns<.., false> K:2636-2640 (res, pool, nb_ids, nb_d, eps) and the visited table at eps + eps_cap words K:2648;
    with vis_slots = 0 the end of eps is hnyk_walk_lds_bytes K:4763-4765, which the host sizes k_walk's tables against
    (vis_slots_for H:507, vis_buckets_for H:537)"""
    for rcap, eps_cap, vis_slots in itertools.product(RCAP, EPS_CAP, VIS_SLOTS):
        spans, total, _ = layout(NNS, rcap, eps_cap, vis_slots)
        pool = rcap * 8
        nb_ids = pool + POOL * 8
        nb_d = nb_ids + 64 * 4
        eps = nb_d + 64 * 4
        vis = eps + eps_cap * 4
        assert spans == [(0, rcap * 8), (pool, POOL * 8), (nb_ids, 64 * 4), (nb_d, 64 * 4), (eps, eps_cap * 4),
                         (vis, vis_slots * 4)], (rcap, eps_cap, vis_slots)
        assert vis == walk_fixed(rcap, eps_cap) and total == vis + vis_slots * 4


def test_arrays_ascend_without_overlap_inside_the_launch_and_aligned(layout):
    for kernel, params, _ in CASES:
        spans, total, misaligned = layout(kernel, *params)
        end = 0
        for off, size in spans:
            assert off >= end, (kernel, params, spans)  # ascending and disjoint
            end = off + size
        assert end <= total, (kernel, params, spans)
        assert misaligned == 0, (kernel, params, spans)
