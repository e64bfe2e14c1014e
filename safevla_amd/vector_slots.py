"""Host bookkeeping of the vector agents (``il.EarlyFusionCnnTransformerVectorAgent``, ``agent.VectorInferenceAgentVIDA``): which slots hold an episode, how old it
is, its last action and its goal; the padded goal table of all slots; where a step of a given age lies on a slot's KV ring.  An episode's actions must not depend on
which other slots share its batch, and this is the state that rests on.  numpy and torch only: no kernel, no GPU (tests/test_vector_slots_cpu.py)."""
from collections import namedtuple

import numpy as np
import torch


def goal_ids(goal_spec) -> tuple:
    """Already tokenised goal -> its token ids without padding: ``{"input_ids"[, "attention_mask"]}`` (right-padded ids keep their ``attention_mask.sum()`` first
    tokens) or an id sequence, array or tensor of any shape, on any device.  Strings are the agents': their tokenisers differ"""
    if isinstance(goal_spec, dict):
        ids = torch.as_tensor(goal_spec["input_ids"]).reshape(-1)
        if "attention_mask" in goal_spec:
            ids = ids[: int(torch.as_tensor(goal_spec["attention_mask"]).sum())]
    else:
        ids = torch.as_tensor(goal_spec).reshape(-1)
    return tuple(int(v) for v in ids.tolist())


def ring_slot(age: int, window: int):
    """Step ``age`` of an episode on a KV ring of ``window`` slots -> (slot the step is written to, number of slots its query reads).  The llama decoder applies
    no RoPE and the time encoding is added to the input, so a single query does not care in which order its keys lie: slots [0, klen) ARE the last
    min(age + 1, window) steps.  The same slot holds the step's decoder input in the history ring that the sliding window of
    early_fusion_tsfm_models.py:491-497 is decoded from once the episode is older than the window."""
    return age % window, min(age + 1, window)


def restart_slot(age: int, window: int):
    """The RL reference has no sliding window: it restarts its cache when its step counter reaches ``max_steps`` (allenact_dino_transformer.py:376-377).  Step ``age``
    -> (slot the step is written to, number of slots its query reads): the steps since the last restart."""
    return age % window, age % window + 1


GoalTable = namedtuple("GoalTable", "key ids mask mask_u8 kvalid lens L")       # EpisodeSlots.goal_table


class EpisodeSlots:
    """``num_episodes`` slots; ``start`` puts an episode into one, ``advance`` records a step of it.  What is not a slot, or a slot that never started, is a ``KeyError``"""

    def __init__(self, num_episodes: int, first_action: int):
        if not 1 <= int(num_episodes) <= 1024:
            raise ValueError(f"num_episodes = {num_episodes}: 1 ... 1024 episodes per vector agent")
        self.num_episodes, self.first_action = int(num_episodes), first_action
        self._age = [None] * self.num_episodes                 # steps taken in the slot's episode (None: not started)
        self._last = [first_action] * self.num_episodes
        self._goal = [None] * self.num_episodes                # token ids without padding, as tuples
        self._table = None                                     # goal_table() of the current goals; None: a goal changed

    def slot(self, s) -> int:
        if isinstance(s, bool) or not isinstance(s, (int, np.integer)) or not 0 <= s < self.num_episodes:
            raise KeyError(s)
        return int(s)

    def started(self, s) -> int:
        s = self.slot(s)
        if self._age[s] is None:
            raise KeyError(s)
        return s

    def age(self, s) -> int:
        return self._age[self.started(s)]

    def last(self, s) -> int:
        return self._last[s]

    def start(self, s, ids: tuple):
        s = self.slot(s)
        if ids != self._goal[s]:
            self._goal[s], self._table = ids, None
        self._age[s], self._last[s] = 0, self.first_action

    def advance(self, s: int, action: int):
        self._last[s], self._age[s] = action, self._age[s] + 1

    def rows(self, keys):
        """the episodes of one step -> (their slots, ages, last actions), in the order of ``keys``.  One call per step: a vector step is bound by its host (0.9 ms at 32 episodes)"""
        n, age, last = self.num_episodes, self._age, self._last
        slots = [s if type(s) is int and 0 <= s < n and age[s] is not None else self.started(s) for s in keys]      # (started: every key that is not plainly a started slot)
        return slots, [age[s] for s in slots], [last[s] for s in slots]

    def goal_table(self, device, text_off: int, padded: bool = True) -> GoalTable:
        """All slots' goals, row = slot, right-padded to the longest, length L (a slot that never started holds one end-of-sequence token): ``key`` the frozen text
        encoder's output is cached under, ``ids`` [N, L] int64, the padding ``mask`` [N, L] as int64 and uint8, the fusion key mask ``kvalid`` [N, text_off + L] uint8 or
        None where no row is padded, the goal length per slot ``lens``; rebuilt when a goal changed.  ``padded=False``: goals of one fixed context (SigLIP) -- nothing to
        hide, every length is L (slots that never started: pad ids up to it)"""
        if self._table is None:
            rows = [g if g is not None else (1,) for g in self._goal]
            L = max(len(g) for g in rows)
            lens = [len(g) if padded else L for g in rows]
            ids = torch.tensor([list(g) + [0] * (L - len(g)) for g in rows], dtype=torch.int64)
            mask = torch.arange(L)[None, :] < torch.tensor(lens)[:, None]
            kvalid = torch.cat([torch.ones(len(rows), text_off, dtype=torch.uint8), mask.to(torch.uint8)], 1).contiguous().to(device) if min(lens) < L else None
            self._table = GoalTable(("vector", tuple(rows)), ids.to(device), mask.to(torch.int64).to(device), mask.to(torch.uint8).to(device), kvalid, lens, L)
        return self._table
