"""Host arithmetic of the vector agent's KV rings (safevla_amd/il.py: ring_slot): step ``age`` of an episode is written to slot age mod W and reads the first
min(age + 1, W) slots -- the slot just written is always among the slots read, and once the ring is full every slot is."""
import pytest

from safevla_amd.il import ring_slot


@pytest.mark.parametrize("W", [1, 8, 1000, 1024])
def test_ring_slot(W):
    held = {}                                            # slot -> age of the step it holds
    for age in range(2 * W + 2):
        pos, klen = ring_slot(age, W)
        assert pos == age % W and klen == min(age + 1, W)
        assert 0 <= pos < klen <= W                      # the written slot lies inside the read range
        held[pos] = age
        # the slots read hold exactly the last min(age + 1, W) steps
        assert sorted(held[s] for s in range(klen)) == list(range(age + 1 - klen, age + 1))
