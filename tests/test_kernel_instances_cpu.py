"""The case table of tests/kernel_instances.py against the rule of DESIGN.md §3h, without a GPU: the table covers every
specialised instance that the form functions can name over the axes, the reachable set has the counts that follow from
the rule (written out below by hand, next to the condition each comes from), and no case ends on the general kernels."""
import kernel_instances as ki

N_METRICS = 7
# the eleven row shapes (lanes per row, chunks per lane) by what the form functions ask of them
SHORT = 3    # (8, 1) (16, 1) (32, 1): nch = 1 and lpr <= 32, rows of at most 512 B
RB_LONG = 3  # (64, 1) (64, 2) (64, 3): nch <= HNY_RB_MAX_NCH = 3, not short
LDS = 5      # (64, 4) (64, 6) (64, 8) (64, 12) (64, 16): no register beam
WG = 6       # (64, 1) .. (64, 8): not short, nch <= 8 — the workgroup kernels
WAVE = 2     # (64, 12) (64, 16): nch > 8 — the one-wave kernels
assert SHORT + RB_LONG + LDS == SHORT + WG + WAVE == len(ki.SHAPES) == 11

EXPECTED = {
    # hnyk_walk_form, build walks (rm 0).  rc 1: nch = 1, lpr <= 32, rcap <= 128, rb_one (ef 32); rc 2: nch <= 3,
    # rcap <= 128 (short rows at ef 100, where rb_one fails; the other three at ef 32 and 100); rc 0: every shape
    # once rcap > 128 (ef 128, 512), and the five shapes beyond three chunks at any ef
    ("walk", 0): N_METRICS * (SHORT * 3 + RB_LONG * 2 + LDS * 1),  # 7 x 20
    # the Reader's walks (rm 1) never take one chunk: rc 2 on the six shapes of nch <= 3 at ef_search 40 (rcap 64),
    # rc 0 on the same six at ef_search 200 (rcap 256) and on the five others
    ("walk", 1): N_METRICS * ((SHORT + RB_LONG) * 2 + LDS * 1),  # 7 x 17
    # hnyk_prune_form.  PRUNE_N8: short rows while rcap <= 512 (ef 32, 100, 128)
    ("prune", "n8"): N_METRICS * SHORT,
    # PRUNE_WG: the six shapes up to 8 chunks that are not short, and k_prune_wg<L, 1, SP> on the three short ones at
    # ef 512 (rcap 1 024); PRUNE_WAVE (nch > 8) is the general k_prune, sp 0
    ("prune", "wg"): N_METRICS * (WG + SHORT),
    ("prune", "wave"): 0,
    # hnyk_apply_form.  APPLY_APPEND_N8: short rows (M = 8 <= 64); the apply does not look at ef
    ("apply", "n8"): N_METRICS * SHORT,
    # APPLY_APPEND_WG: the six shapes of PRUNE_WG, and k_apply_wg<L, 1, SP> only with HNY_PRUNE_N8=0, which the table
    # sets on ONE short shape per metric (L = 8, 16, 32 in turn), not on every one
    ("apply", "wg"): N_METRICS * WG + N_METRICS,
    # APPLY_WAVE with sp != 0: rows beyond 8 KB
    ("apply", "wave"): N_METRICS * WAVE,
}


def _reachable():
    keys = set()
    for c in ki.all_configs():
        keys |= ki.keys_of(c)
    return keys


def test_the_case_table_covers_every_reachable_instance():
    covered = set()
    for c in ki.CASES:
        covered |= ki.keys_of(c)
    reachable = _reachable()
    missing = sorted(ki.key_name(k) for k in reachable - covered)
    extra = sorted(ki.key_name(k) for k in covered - reachable)
    assert not missing and not extra, f"instances no case runs: {missing}; instances outside the axes: {extra}"
    assert ki.CASES == ki.greedy_cover(ki.all_configs())  # deterministic: the same table at every import
    assert len(set(ki.CASES)) == len(ki.CASES)


def test_reachable_instances_per_family_follow_the_form_rule():
    reachable = _reachable()
    assert all(k[3 if k[0] == "walk" else 4] != 0 for k in reachable)
    got = {fam: 0 for fam in EXPECTED}
    for k in reachable:
        fam = (k[0], k[4]) if k[0] == "walk" else (k[0], k[1])
        assert fam in got, ki.key_name(k)
        got[fam] += 1
    assert got == EXPECTED
    # the same count for every metric, and in every family but apply-wg for every shape the rule names
    for sp in range(1, N_METRICS + 1):
        mine = {k for k in reachable if k[3 if k[0] == "walk" else 4] == sp}
        assert len(mine) == 20 + 17 + 3 + 9 + 3 + 7 + 2, sp
        rcs = {}
        for k in mine:
            if k[0] == "walk":
                rcs.setdefault((k[1], k[2], k[4]), set()).add(k[5])
        for (L, Cn), i in zip(ki.SHAPES, range(11)):
            assert rcs[(L, Cn, 0)] == ({0, 1, 2} if i < SHORT else {0, 2} if i < SHORT + RB_LONG else {0}), (sp, L, Cn)
            assert rcs[(L, Cn, 1)] == ({0, 2} if i < SHORT + RB_LONG else {0}), (sp, L, Cn)
        short_l = ki.SHORT[(sp - 1) % 3][0]
        assert {k[2:4] for k in mine if k[:2] == ("apply", "wg") and k[3] == 1 and k[2] <= 32} == {(short_l, 1)}, sp
    assert len(reachable) == sum(EXPECTED.values()) == 427


def test_every_case_runs_a_specialised_instance():
    for c in ki.CASES:
        keys = ki.keys_of(c)
        assert keys, c
        # a whole build on the specialised kernels: its walk and its apply (the prune of rows beyond 8 KB is general)
        assert any(k[0] == "walk" and k[4] == 0 for k in keys) and any(k[0] == "apply" for k in keys), c
        assert ki.case_id(c).count("+") + 1 == len(keys)
    assert len({ki.case_id(c) for c in ki.CASES}) == len(ki.CASES)
