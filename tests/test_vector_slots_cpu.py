"""Host bookkeeping of the two vector agents (safevla_amd/vector_slots.py): what is a slot, goal normalisation, the padded goal table of all slots, and the arithmetic
of the KV rings -- ``ring_slot``: step ``age`` of an episode is written to slot age mod W and reads the first min(age + 1, W) slots, the slot just written is always
among the slots read, and once the ring is full every slot is; ``restart_slot``: the RL reference's restart at W steps.  No device, no native library."""
import numpy as np
import pytest
import torch

from safevla_amd.vector_slots import EpisodeSlots, goal_ids, restart_slot, ring_slot

TEXT_OFF = 169
GOALS = {0: (11, 12, 1), 1: (21, 22, 23, 24, 1), 3: (31, 32, 33, 34, 35, 36, 1)}          # 3, 5 and 7 tokens; slot 2 never starts


def _slots(goals=GOALS, n=4, first_action=0):
    sl = EpisodeSlots(n, first_action)
    for s, g in goals.items():
        sl.start(s, g)
    return sl


def test_what_is_a_slot():
    sl = _slots()
    for bad in (True, "0", -1, 4, 2.0):
        for f in (sl.slot, sl.started, sl.age):
            with pytest.raises(KeyError):
                f(bad)
        with pytest.raises(KeyError):
            sl.start(bad, (1,))
        with pytest.raises(KeyError):
            sl.rows([0, bad])
    assert sl.slot(np.int64(1)) == 1 and type(sl.slot(np.int64(1))) is int and sl.started(np.int64(1)) == 1 and sl.age(np.int64(1)) == 0
    assert sl.slot(2) == 2                                  # a slot, but never started
    for f in (sl.age, sl.started):
        with pytest.raises(KeyError):
            f(2)
    with pytest.raises(KeyError):
        sl.rows([2])
    for n in (0, 1025):
        with pytest.raises(ValueError, match=f"num_episodes = {n}: 1 ... 1024 episodes per vector agent"):
            EpisodeSlots(n, 0)
    assert EpisodeSlots(1, 0).num_episodes == 1 and EpisodeSlots(1024, 0).num_episodes == 1024


def test_goal_ids():
    ids = [917, 4033, 88, 1]
    assert goal_ids(dict(input_ids=np.array([ids]))) == tuple(ids)
    assert goal_ids(dict(input_ids=np.array([ids + [0, 0]]), attention_mask=np.array([[1, 1, 1, 1, 0, 0]]))) == tuple(ids)      # right-padded: trimmed
    assert goal_ids(dict(input_ids=torch.tensor([ids + [0]]), attention_mask=torch.tensor([[1, 1, 1, 1, 0]]))) == tuple(ids)
    assert goal_ids(dict(input_ids=np.array([ids + [0, 0]]))) == tuple(ids) + (0, 0)                                          # no mask: every id
    assert goal_ids(ids) == goal_ids(np.array([ids])) == goal_ids(torch.tensor(ids)) == tuple(ids)
    assert all(type(v) is int for v in goal_ids(np.array([ids], np.int32)))
    assert goal_ids([]) == ()


def test_goal_table():
    sl = _slots()
    t = sl.goal_table("cpu", TEXT_OFF)
    assert t.L == 7 and t.lens == [3, 5, 1, 7]
    assert t.ids.shape == (4, 7) and t.ids.dtype == torch.int64
    assert t.ids[2].tolist() == [1, 0, 0, 0, 0, 0, 0]                           # the idle row: one end-of-sequence token
    for s, g in GOALS.items():
        assert t.ids[s].tolist() == list(g) + [0] * (7 - len(g))
    assert t.mask.dtype == torch.int64 and t.mask_u8.dtype == torch.uint8 and t.mask.sum(1).tolist() == t.lens
    assert torch.equal(t.mask, t.mask_u8.long())
    assert all(t.mask[s, :n].all() for s, n in enumerate(t.lens))               # right-padded: the tokens come first
    assert t.kvalid.shape == (4, 176) and t.kvalid.dtype == torch.uint8 and t.kvalid.is_contiguous()
    assert bool((t.kvalid[:, :TEXT_OFF] == 1).all()) and torch.equal(t.kvalid[:, TEXT_OFF:], t.mask_u8)
    # cached until a goal changes
    assert sl.goal_table("cpu", TEXT_OFF) is t
    sl.advance(0, 5)
    sl.start(0, GOALS[0])
    assert sl.goal_table("cpu", TEXT_OFF) is t and sl.age(0) == 0
    sl.start(0, (11, 12, 13, 1))
    t2 = sl.goal_table("cpu", TEXT_OFF)
    assert t2 is not t and t2.key != t.key and t2.lens == [4, 5, 1, 7] and t2.ids[0].tolist() == [11, 12, 13, 1, 0, 0, 0]
    sl.start(2, (41, 1))                                                        # a slot's first goal changes the table too
    assert sl.goal_table("cpu", TEXT_OFF).lens == [4, 5, 2, 7]


def test_goal_table_without_padding():
    same = _slots({s: (10 + s, 20 + s, 1) for s in range(4)})
    t = same.goal_table("cpu", TEXT_OFF)
    assert t.kvalid is None and t.lens == [3] * 4 and t.L == 3 and bool(t.mask.all())
    fixed = _slots()                                                            # the SigLIP case: one fixed context, shorter rows are padded up to it
    t = fixed.goal_table("cpu", TEXT_OFF, padded=False)
    assert t.kvalid is None and t.L == 7 and t.lens == [7] * 4 and bool(t.mask.all()) and bool(t.mask_u8.all())
    assert t.ids.shape == (4, 7) and t.ids[2].tolist() == [1, 0, 0, 0, 0, 0, 0]


@pytest.mark.parametrize("first_action", [0, 21])
def test_start_and_advance(first_action):
    sl = _slots(first_action=first_action)
    assert sl.last(0) == first_action and sl.age(0) == 0
    for age, action in enumerate((7, 3)):
        assert sl.age(0) == age
        sl.advance(0, action)
        assert sl.last(0) == action
    assert sl.age(0) == 2 and sl.age(1) == 0 and sl.last(1) == first_action    # the other slots stand
    assert sl.rows([np.int64(3), 0]) == ([3, 0], [0, 2], [first_action, 3])
    sl.start(0, GOALS[0])
    assert sl.age(0) == 0 and sl.last(0) == first_action


@pytest.mark.parametrize("W", [1, 8, 1000, 1024])
def test_ring_slot(W):
    from safevla_amd import il

    assert il.ring_slot is ring_slot
    held = {}                                            # slot -> age of the step it holds
    for age in range(2 * W + 2):
        pos, klen = ring_slot(age, W)
        assert pos == age % W and klen == min(age + 1, W)
        assert 0 <= pos < klen <= W                      # the written slot lies inside the read range
        held[pos] = age
        # the slots read hold exactly the last min(age + 1, W) steps
        assert sorted(held[s] for s in range(klen)) == list(range(age + 1 - klen, age + 1))


@pytest.mark.parametrize("W", [1, 8, 1000])
def test_restart_slot(W):
    for age in range(3 * W + 1):
        pos, klen = restart_slot(age, W)
        assert pos == age % W and klen == pos + 1 and 0 <= pos < klen <= W
