"""The slot state machine of the chunk pipeline (epa_dev_chunk_stage / _launch_begin / _launch_end / _finish and the group
launches): what it refuses, and that a refusal changes nothing.

A slot is free, staged, launch begun, launched, or a member of a group whose launch was begun.  Every call that does not
fit the slot's state must fail with EPA_ERR_INVALID_ARG before anything is queued, and leave every slot as it was: after
each refusal the pipeline is carried to its end, and the rows a slot hands out must equal BIT FOR BIT what
epa_dev_place_chunk returns for the same reads on a context that has done nothing else (history_util.fresh_chunk).

Two recoverable paths as well: a group of three launched with too small a max_pairs fails with EPA_ERR_PAIR_OVERFLOW and
leaves all three members staged; they then launch as a group with room, or one by one.  (The overflow followed by the
second GROUP launch is also asserted, against another reference, at the end of
test_gpu_pipeline.py::test_group_launch_of_small_chunks_equals_per_chunk_launches; the one-by-one continuation only here.)

Reference R4 (40 tips, 77 branches, 260 sites), chunks of 3, 10 and 12 reads."""
import pytest

import epa_ng_amd as epa
import history_util as hu

pytestmark = pytest.mark.gpu

NAME = "R4"
ERR_INVALID_ARG, ERR_PAIR_OVERFLOW = -1, -9
N_SLOTS = 24        # epa_ctx::N_SLOTS
MAX_GROUP = 8       # EPA_MAX_GROUP


def refused(fn, *a, **kw):
    with pytest.raises(epa.EpaError) as ei:
        fn(*a, **kw)
    assert ei.value.code == ERR_INVALID_ARG, ei.value


def chunk(which, form="full"):
    return hu.inputs(NAME)[which][form]


def room(ev, *which):
    return sum(len(chunk(w)[1]) for w in which) * ev.B


def finish_equals_fresh(ev, slot, which, form="full", own_launch=True):
    """finish `slot`: the rows of a fresh place_chunk on the same reads; own_launch: the Newton counters too (a group
    reports ONE launch's counters, with its first member)"""
    p, r = ev.chunk_finish(slot)
    want = hu.fresh_chunk(NAME, which, form)
    if not own_launch:
        want = {k: v for k, v in want.items() if not k.endswith(".counters")}
    hu.assert_same(hu.chunk_rows(p, r, ev if own_launch else None), want, "slot %d, chunk %r" % (slot, which))


def test_slot_index_out_of_range():
    ev = hu.new_context(NAME)
    ev.chunk_stage(0, *chunk("small"))
    for bad in (-1, N_SLOTS):
        refused(ev.chunk_stage, bad, *chunk("small"))
        refused(ev.chunk_launch, bad, max_pairs=room(ev, "small"))
        refused(ev.chunk_launch_begin, bad, max_pairs=room(ev, "small"))
        refused(ev.chunk_launch_end, bad)
        refused(ev.chunk_finish, bad)
        refused(ev.chunk_launch_many, [bad], max_pairs=room(ev, "small"))
        refused(ev.chunk_launch_many, [0, bad], max_pairs=room(ev, "small"))
    ev.chunk_launch(0, max_pairs=room(ev, "small"))
    finish_equals_fresh(ev, 0, "small")
    ev.close()


def test_one_slot_through_its_states():
    """free -> staged -> launch begun -> launched -> free, with every call that does not fit tried on the way"""
    ev = hu.new_context(NAME)
    kw = dict(max_pairs=room(ev, "ten"))
    # free
    refused(ev.chunk_launch, 3, **kw)
    refused(ev.chunk_launch_begin, 3, **kw)
    refused(ev.chunk_launch_end, 3)
    refused(ev.chunk_finish, 3)
    ev.chunk_stage(3, *chunk("ten"))
    # staged
    refused(ev.chunk_launch_end, 3)
    refused(ev.chunk_finish, 3)
    ev.chunk_launch_begin(3, **kw)
    # launch begun
    refused(ev.chunk_launch_begin, 3, **kw)
    refused(ev.chunk_launch, 3, **kw)
    refused(ev.chunk_finish, 3)
    refused(ev.chunk_stage, 3, *chunk("small"))
    ev.chunk_launch_end(3)
    # launched, not finished
    refused(ev.chunk_stage, 3, *chunk("small"))
    refused(ev.chunk_launch_begin, 3, **kw)
    refused(ev.chunk_launch_end, 3)
    finish_equals_fresh(ev, 3, "ten")
    # free again
    refused(ev.chunk_finish, 3)
    refused(ev.chunk_launch_end, 3)
    ev.chunk_stage(3, *chunk("small"))
    ev.chunk_launch(3, max_pairs=room(ev, "small"))
    finish_equals_fresh(ev, 3, "small")
    ev.close()


def test_group_launch_refusals():
    """chunk_launch_many that never starts: no slot, nine slots, a slot twice, a member that is not staged, members
    staged in different query layouts.  The staged slots stay staged"""
    ev = hu.new_context(NAME)
    kw = dict(max_pairs=room(ev, "small", "ten", "mid"))
    ev.chunk_stage(0, *chunk("small"))
    ev.chunk_stage(1, *chunk("ten"))
    ev.chunk_stage(5, *chunk("mid", "compact"))
    refused(ev.chunk_launch_many, [], **kw)
    refused(ev.chunk_launch_many, list(range(MAX_GROUP + 1)), **kw)
    refused(ev.chunk_launch_many, [0, 1, 0], **kw)
    refused(ev.chunk_launch_many, [1, 1], **kw)
    refused(ev.chunk_launch_many, [0, 1, 2], **kw)          # slot 2 is free
    refused(ev.chunk_launch_many, [2, 0], **kw)             # ... as the leader
    refused(ev.chunk_launch_many, [0, 1, 5], **kw)          # full rows and compact rows
    refused(ev.chunk_launch_many, [5, 0], **kw)
    ev.chunk_launch_many([0, 1], **kw)
    ev.chunk_launch(5, **kw)
    finish_equals_fresh(ev, 1, "ten", own_launch=False)
    finish_equals_fresh(ev, 5, "mid", "compact")
    finish_equals_fresh(ev, 0, "small", own_launch=False)
    ev.close()


def test_members_of_a_begun_and_of_an_ended_group():
    ev = hu.new_context(NAME)
    kw = dict(max_pairs=room(ev, "small", "ten", "mid"))
    for slot, which in ((4, "mid"), (0, "small"), (7, "ten")):
        ev.chunk_stage(slot, *chunk(which))
    ev.chunk_launch_many_begin([4, 0, 7], **kw)
    # the group's launch is begun: slot 4 leads, 0 and 7 are members
    for member in (0, 7):
        refused(ev.chunk_launch_end, member)
        refused(ev.chunk_stage, member, *chunk("small"))
        refused(ev.chunk_launch, member, **kw)
        refused(ev.chunk_finish, member)
    refused(ev.chunk_launch_many, [9, 0], **kw)
    refused(ev.chunk_finish, 4)
    refused(ev.chunk_stage, 4, *chunk("small"))
    ev.chunk_launch_end(4)
    finish_equals_fresh(ev, 4, "mid", own_launch=False)
    # ended, only the leader finished: its buffers still hold the members' rows
    ev.chunk_stage(9, *chunk("small"))
    refused(ev.chunk_stage, 4, *chunk("ten"))
    refused(ev.chunk_launch_many, [4, 9], **kw)
    finish_equals_fresh(ev, 7, "ten", own_launch=False)
    refused(ev.chunk_stage, 4, *chunk("ten"))                # member 0 is still out
    finish_equals_fresh(ev, 0, "small", own_launch=False)
    # every member finished: the leader stages and leads again
    ev.chunk_stage(4, *chunk("ten"))
    ev.chunk_launch_many([4, 9], **kw)
    finish_equals_fresh(ev, 9, "small", own_launch=False)
    finish_equals_fresh(ev, 4, "ten", own_launch=False)
    ev.close()


@pytest.mark.parametrize("again", ["as a group", "one by one"])
def test_group_overflow_leaves_every_member_staged(again):
    ev = hu.new_context(NAME)
    members = ((2, "small"), (6, "mid"), (1, "ten"))
    slots = [s for s, _ in members]
    for slot, which in members:
        ev.chunk_stage(slot, *chunk(which))
    with pytest.raises(epa.EpaError) as ei:
        ev.chunk_launch_many(slots, max_pairs=5)
    assert ei.value.code == ERR_PAIR_OVERFLOW, ei.value
    for slot in slots:                                       # staged, not launched: nothing to end or to finish
        refused(ev.chunk_launch_end, slot)
        refused(ev.chunk_finish, slot)
    if again == "as a group":
        ev.chunk_launch_many(slots, max_pairs=room(ev, "small", "mid", "ten"))
    else:
        for slot, which in members:
            ev.chunk_launch(slot, max_pairs=room(ev, which))
    for slot, which in reversed(members):
        finish_equals_fresh(ev, slot, which, own_launch=again == "one by one")
    ev.close()
