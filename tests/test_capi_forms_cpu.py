"""Which kernel a launch gets, without a GPU: hny_internal_launch_forms fills the walk, prune and apply forms and the
default walk_slots for a builder's figures from the arguments alone.  The table below was written out by hand from
the code of commit 87c955e (the parent of the form functions), where the rule lived in five places; each row names
the lines it was read from (K = hny_kernels.hip, H = hny_host.cpp at that commit):

  shape           pick_shape, H:530-544 (f32: dim / 4 units; bit codes: dim / 128 units)
  eps_cap, rcap   eps_cap_of H:442-445, res_capacity H:460-468 (64, 128, 256 .. >= max(ef, entry points) + 1)
  walk            hnyk_walk K:4758-4761 (specialised or general), fast_path K:4738-4742, Hot<SP>::Walk::run
                  K:4518-4560 (big_eps, register beams, reader), rb_one H:1894-1900, __launch_bounds__ K:1979
  prune           launch_prune H:1924-1932, wave_prune_only H:1401, hnyk_prune_n8_ok K:4788-4792, hnyk_prune_wg K:4804-4808
  apply           apply_front H:2050-2057, launch_apply_deferred H:2064-2068, hnyk_apply_n8_ok K:4796-4800,
                  hnyk_apply K:4783-4786, hnyk_apply_wg K:4809-4813
  walk_slots      six_waves H:1375-1377
"""
import ctypes as C

import pytest

N8, WG, WAVE = 0, 1, 2
COS, EUC, MAN, HAM = 0, 1, 2, 3


def case(metric, dim, M=16, M0=32, ef=100, eps=1, strict=0, inc=0, reader=0, no_fast=0, no_rb=0, rb_one=1, n8=1):
    return (metric, dim, M, M0, ef, eps, strict, inc, reader, no_fast, no_rb, rb_one, n8)


# expected: walk (sp, big_eps, reader, rc, waves per SIMD), prune (kind, sp, grid cap), apply (kind, sp, grid cap), walk_slots
SHORT_EUC = (2, 0, 0, 2, 4, N8, 2, 5120, N8, 2, 5120, 4096)
GENERAL_WG = (0, 0, 0, 0, 4, WG, 0, 2048, WG, 0, 2048, 4096)
LONG_LDS_BEAM = (1, 0, 0, 0, 4, WG, 1, 2048, WG, 1, 2048, 4096)
TABLE = {
    # 64-d f32 rows (16 lanes, 1 chunk), ef 100: rcap 128 -> two-chunk beam (K:4530, 4547), 4 waves (SP 2 < 4, K:1979),
    # n8 prune and apply (K:4791, 4799), 4 096 slots (metric < HAMMING, H:1375)
    "euclid_64d": (case(EUC, 64), SHORT_EUC),
    # 1 024-bit codes (8 lanes), ef 40: most = 40 <= 64 -> one-chunk beam (H:1899, K:4539), six waves (K:1979), 6 144 (H:1377)
    "hamming_1024b_ef40": (case(HAM, 1024, ef=40), (4, 0, 0, 1, 6, N8, 4, 5120, N8, 4, 5120, 6144)),
    # most 64 / 65 (H:1897-1899): ef 64 keeps one chunk, ef 65 takes two; both hold six waves (RC 1 or 2, K:1979)
    "hamming_most_64": (case(HAM, 1024, ef=64), (4, 0, 0, 1, 6, N8, 4, 5120, N8, 4, 5120, 6144)),
    "hamming_most_65": (case(HAM, 1024, ef=65), (4, 0, 0, 2, 6, N8, 4, 5120, N8, 4, 5120, 6144)),
    # metric 2 / 3 on 512-B rows (32 lanes): SP 3 < 4 -> 4 waves and 4 096; SP 4 -> 6 and 6 144
    "manhattan_128d_ef40": (case(MAN, 128, ef=40), (3, 0, 0, 1, 4, N8, 3, 5120, N8, 3, 5120, 4096)),
    "hamming_4096b_ef40": (case(HAM, 4096, ef=40), (4, 0, 0, 1, 6, N8, 4, 5120, N8, 4, 5120, 6144)),
    # lpr 64 at nch 1 (1 KB of codes): no one-chunk beam (K:4534), 4 waves (K:1979), workgroup prune / apply
    # (K:4791, 4799: lpr <= 32), 4 096 (H:1375: lpr <= 32)
    "hamming_8192b_ef40": (case(HAM, 8192, ef=40), (4, 0, 0, 2, 4, WG, 4, 2048, WG, 4, 2048, 4096)),
    # nch 3 / 4 (K:4528, HNY_RB_MAX_NCH = 3): 768-d keeps the register beam, 1 024-d takes the LDS beam
    "cosine_768d": (case(COS, 768), (1, 0, 0, 2, 4, WG, 1, 2048, WG, 1, 2048, 4096)),
    "cosine_1024d": (case(COS, 1024), LONG_LDS_BEAM),
    # rcap 128 / 256 (K:4530): ef 127 -> 128 entries, ef 128 -> 129 entries = rcap 256 -> LDS beam
    "cosine_768d_ef127": (case(COS, 768, ef=127), (1, 0, 0, 2, 4, WG, 1, 2048, WG, 1, 2048, 4096)),
    "cosine_768d_ef128": (case(COS, 768, ef=128), LONG_LDS_BEAM),
    # nch 8 / 12 (H:1401, K:4565, 4613): 2 048-d on the workgroup kernels; 3 072-d on the one-wave kernels, the prune
    # general (K:4780-4782) on walk_slots blocks (H:1930), k_apply specialised (K:4784) on up to 8 192 (H:2052)
    "cosine_2048d": (case(COS, 2048), LONG_LDS_BEAM),
    "cosine_3072d": (case(COS, 3072), (1, 0, 0, 0, 4, WAVE, 0, 4096, WAVE, 1, 8192, 4096)),
    # eps_cap 64 / 128 (K:4759, 4522): 64 entry points stay specialised, 65 take the general kernel with BIG_EPS;
    # prune and apply do not look at the entry points
    "euclid_64d_eps64": (case(EUC, 64, eps=64), SHORT_EUC),
    "euclid_64d_eps65": (case(EUC, 64, eps=65), (0, 1, 0, 0, 4, N8, 2, 5120, N8, 2, 5120, 4096)),
    # M0 64 / 65 (K:4741): lists beyond 64 slots take the general kernels; six_waves does not know (H:1375)
    "euclid_64d_M0_64": (case(EUC, 64, M0=64), SHORT_EUC),
    "euclid_64d_M0_65": (case(EUC, 64, M0=65), GENERAL_WG),
    "hamming_1024b_M0_65": (case(HAM, 1024, M0=65, ef=40), (0, 0, 0, 0, 4, WG, 0, 2048, WG, 0, 2048, 6144)),
    # strict mode (K:4741, H:1401): general walk, one-wave prune on walk_slots blocks, k_apply<.., 0>
    "euclid_64d_strict": (case(EUC, 64, strict=1), (0, 0, 0, 0, 4, WAVE, 0, 4096, WAVE, 0, 8192, 4096)),
    "hamming_1024b_strict": (case(HAM, 1024, ef=40, strict=1), (0, 0, 0, 0, 4, WAVE, 0, 6144, WAVE, 0, 8192, 6144)),
    # incremental (K:4741): the general kernels, workgroup prune and apply
    "euclid_64d_incremental": (case(EUC, 64, inc=1), GENERAL_WG),
    # reader mode (K:4539, 4544-4545, 1979): RM compiled in, never the one-chunk beam, 4 waves
    "euclid_64d_reader": (case(EUC, 64, reader=1), (2, 0, 1, 2, 4, N8, 2, 5120, N8, 2, 5120, 4096)),
    "hamming_1024b_reader": (case(HAM, 1024, ef=40, reader=1), (4, 0, 1, 2, 4, N8, 4, 5120, N8, 4, 5120, 6144)),
    # the form switches: HNY_NO_FAST (K:4739; six_waves does not read it), HNY_NO_RB (K:4529, H:1376), HNY_RB_ONE=0
    # (H:1899), HNY_PRUNE_N8=0 (K:4789, 4797)
    "euclid_64d_no_fast": (case(EUC, 64, no_fast=1), GENERAL_WG),
    "hamming_1024b_no_fast": (case(HAM, 1024, ef=40, no_fast=1), (0, 0, 0, 0, 4, WG, 0, 2048, WG, 0, 2048, 6144)),
    "hamming_1024b_no_rb": (case(HAM, 1024, ef=40, no_rb=1), (4, 0, 0, 0, 4, N8, 4, 5120, N8, 4, 5120, 4096)),
    "hamming_1024b_rb_one_0": (case(HAM, 1024, ef=40, rb_one=0), (4, 0, 0, 2, 6, N8, 4, 5120, N8, 4, 5120, 6144)),
    "euclid_64d_prune_n8_0": (case(EUC, 64, n8=0), (2, 0, 0, 2, 4, WG, 2, 2048, WG, 2, 2048, 4096)),
    # candidate lists of 512 / 1 024 entries (K:4791: rcap <= 512): ef 511 on the n8 prune, ef 512 on the workgroup
    # prune; the apply does not depend on ef; both walks on the LDS beam
    "euclid_64d_ef511": (case(EUC, 64, ef=511), (2, 0, 0, 0, 4, N8, 2, 5120, N8, 2, 5120, 4096)),
    "euclid_64d_ef512": (case(EUC, 64, ef=512), (2, 0, 0, 0, 4, WG, 2, 2048, N8, 2, 5120, 4096)),
}


@pytest.fixture(scope="module")
def forms():
    import hannoy_amd
    fn = hannoy_amd.load_library().hny_internal_launch_forms
    fn.restype = C.c_int
    fn.argtypes = [C.POINTER(C.c_int32), C.POINTER(C.c_int32)]

    def call(args):
        out = (C.c_int32 * 12)()
        assert fn((C.c_int32 * 13)(*args), out) == 0
        return tuple(out)
    return call


@pytest.mark.parametrize("name", list(TABLE))
def test_launch_forms_equal_the_parent_rule(forms, name):
    args, want = TABLE[name]
    assert forms(args) == want


def test_waves_per_simd_and_walk_slots_off_the_table(forms):
    """The two rules that size the resident walks, on what the library returns for inputs beyond the table's rows:
    six waves per SIMD only for k_walk<lpr <= 32, 1, ., SP >= 4, false, RC 1 or 2> (K:1979; bit codes of at most 4 096
    bits are the rows of nch 1 and lpr <= 32), and 6 144 walk slots for bit codes of that size with rcap <= 128 unless
    HNY_NO_RB is set, whatever kernel the walk then gets (H:1375-1377)."""
    dims = {COS: (64, 128, 768), EUC: (64, 128, 768), MAN: (64, 128, 768), HAM: (1024, 4096, 8192)}
    for metric, metric_dims in dims.items():
        for dim in metric_dims:
            for ef in (40, 127, 128):
                for M0 in (32, 65):
                    for strict in (0, 1):
                        for reader in (0, 1):
                            for no_rb in (0, 1):
                                args = case(metric, dim, M0=M0, ef=ef, strict=strict, reader=reader, no_rb=no_rb)
                                got = forms(args)
                                sp, _, rm, rc, waves = got[:5]
                                short_codes = metric == HAM and dim <= 4096
                                six = short_codes and sp >= 4 and not rm and rc in (1, 2)
                                assert waves == (6 if six else 4), args
                                assert rm == (reader if sp else 0), args
                                assert got[11] == (6144 if short_codes and ef <= 127 and not no_rb else 4096), args
