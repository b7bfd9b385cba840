"""The generator of hand-made selections (tests/crafted_selections.py) against its own contract, on every buffer the GPU
tests of tests/test_gpu_build_phases.py send to the device: the scenarios' buffers depend on the schedule alone, so
stepping the oracle through a scenario here produces them all.  The bounds the scenarios exist for (segments of one
batch beyond one trip of k_apply_append, beyond the block cap of the strict-mode k_apply) are asserted on the buffers
as well, and the checker is shown to refuse a buffer that breaks each rule."""
import numpy as np
import pytest

import crafted_selections as cs


def walk(orc, scen, on_crafted=None):
    """every batch of the scenario on the oracle stepper; crafted buffers are checked, the others are the walk's own"""
    progress, crafted = cs.Progress(scen.ds.n), 0
    with scen.stepper() as st:
        while True:
            b = st.next_batch()
            if b.count == 0:
                break
            sel = scen.select(b, progress)
            if sel is None:
                sel = st.search()
            else:
                cs.check_contract(orc, scen.ds, scen.order, b, scen.cap(b.level), sel, progress)
                crafted += 1
                if on_crafted:
                    on_crafted(b, sel, progress)
            st.apply(sel)
            progress.close(b)
        assert progress.n_done == scen.ds.n and progress.done.all()
    return crafted


@pytest.mark.parametrize("name", sorted(cs.SCENARIOS))
def test_every_crafted_buffer_keeps_the_contract(orc, name):
    scen = cs.SCENARIOS[name](orc)
    crafted = walk(orc, scen)
    assert len(scen.chosen) == 1 and crafted >= 1
    first, segments = scen.chosen[0]
    if name == "append-second-trip":
        assert segments == cs.APPEND_MEMBERS * cs.APPEND_PRIVATE + cs.APPEND_MEMBERS == 1114112 > 4096 * 256
    elif name == "strict-apply-beyond-cap":
        assert segments == cs.WAVE_MEMBERS * cs.WAVE_PRIVATE + cs.WAVE_MEMBERS == 10240 > 8192
    elif name.startswith("hub"):
        assert segments == 1 + 2 * cs.Hub.HUB_BATCH + cs.Hub.HUB_BATCH  # the hub, the private targets, the members
    else:
        assert segments > 0


def test_the_checker_refuses_what_the_contract_forbids(orc):
    """one broken rule at a time on a buffer of the hub scenario (three entries per member on layer 0)"""
    scen = cs.SCENARIOS["hub-32B"](orc)
    seen = []

    def tamper(b, sel, progress):
        cap = scen.cap(b.level)
        good = sel.reshape(b.count, 1, cap + 1)

        def refuses(rule, edit):
            bad = good.copy()
            edit(bad)
            with pytest.raises(AssertionError, match=rule):
                cs.check_contract(orc, scen.ds, scen.order, b, cap, bad.reshape(-1), progress)
        m0, m1 = int(b.slots[0]), int(b.slots[1])
        d01 = orc.distance_pairs(scen.ds, scen.order, [m0], [m1]).view(np.uint32)[0]
        never = int(np.flatnonzero(~progress.done & ~np.isin(np.arange(scen.ds.n), b.slots))[0])
        dn = orc.distance_pairs(scen.ds, scen.order, [m0], [never]).view(np.uint32)[0]

        def one_entry(bits, slot):
            def edit(x):
                x[0, 0, 0] = 1
                x[0, 0, 1] = (np.uint64(bits) << np.uint64(32)) | np.uint64(slot)
            return edit
        refuses("count", lambda x: x.__setitem__((0, 0, 0), cap + 1))
        refuses("earlier|member", one_entry(d01, m1))  # a member is no earlier slot either
        refuses("earlier", one_entry(dn, never))
        refuses("true ones", lambda x: x.__setitem__((0, 0, 1), x[0, 0, 1] ^ np.uint64(1 << 32)))
        refuses("ascend", lambda x: x.__setitem__((0, 0, slice(1, 3)), x[0, 0, 2:0:-1].copy()))
        refuses("distinct|ascend", lambda x: x.__setitem__((0, 0, 2), x[0, 0, 1]))
        seen.append(b.first)
    walk(orc, scen, tamper)
    assert len(seen) == 1


def test_a_level_reaches_the_layer(orc):
    """the empty-layers buffer is full on layers 2 and 0 and empty on layer 1; it is refused once one of its layer-2
    targets is said to be of level 1 (every slot inserted before a level-2 batch has level 2 or more, so the rule is
    shown on edited levels, not on an edited buffer)"""
    import copy
    scen = cs.SCENARIOS["empty-layers"](orc)
    seen = []

    def tamper(b, sel, progress):
        cap = scen.cap(b.level)
        rows = sel.reshape(b.count, 3, cap + 1)
        assert b.level == 2 and (rows[:, 1, 0] == 0).all() and (rows[:, 0, 0] == cap).all() and (rows[:, 2, 0] == cap).all()
        lower = copy.copy(scen.ds)
        lower.levels = scen.ds.levels.copy()
        lower.levels[int(rows[0, 0, 1] & np.uint64(0xFFFFFFFF))] = 1
        with pytest.raises(AssertionError, match="level reaches"):
            cs.check_contract(orc, lower, scen.order, b, cap, sel, progress)
        seen.append(b.first)
    walk(orc, scen, tamper)
    assert len(seen) == 1
