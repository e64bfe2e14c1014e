#!/usr/bin/env python3
"""A/B of the vector RL agent (safevla_amd/agent.py: VectorInferenceAgentVIDA -- actor tower only, per-row KV rings, csrc/sample.hip), one process, HIP events,
5 warm-up steps and 20 repetitions per figure (``--reps``); median, min and max of the repetitions go to stdout and to ``--out`` (profiles/vector_vida_ab.txt).
  (a) agent   N single ``InferenceAgentVIDA`` steps in turn against ONE vector step of N episodes, N = 8 and 32, on one full-sensor policy in eval mode.  The single
              agent is the agent as it ships: rollout storage, three towers on the recorded, tower-grouped acting path, log_softmax / multinomial / argmax.  Its N
              steps are N consecutive steps of one agent on one model -- N agents in turn do the same work per step, but each would need a model copy of its own
              (the towers' KV caches and step counter belong to the model); one copy keeps its weights warm in the caches, which favours the single agent.  A
              repetition is one episode of 48 steps (reset included); the figures are N x (ms per single step) and ms per vector step of all N.  Neither side runs
              the frozen ViT: both get the same pre-encoded features (the single agent through a preprocessor that hands them over).
  (b) sample  ops.policy_sample_rows against the four framework calls it replaces (log_softmax, exp, multinomial, argmax) at n = 64 rows of 20 actions; a repetition
              is 200 calls, the two alternate repetition by repetition; us per call.
  python tools/ab_vector_vida.py [--reps 20] [--out profiles/vector_vida_ab.txt]"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from safevla_amd import ops

WARMUP, STEPS, CALLS = 5, 48, 200
LINES = []


def say(line):
    print(line, flush=True)
    LINES.append(line)


def timed(fn):
    """one repetition of ``fn`` between two HIP events -> ms"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def stats(ts):
    return statistics.median(ts), min(ts), max(ts)


class _Features:
    """stands where the frozen ViT preprocessor stands in ``InferenceAgentVIDA`` and hands over pre-encoded features [1, 384, 7, 12]"""

    def __init__(self, feat):
        self.feat = feat

    def process(self, obs, *a, **k):
        return self.feat


def agent_ab(model, n, reps):
    from safevla_amd.agent import InferenceAgentVIDA

    rs = np.random.RandomState(n)
    u = model.uuids
    feats = [{u["nav"]: torch.from_numpy(rs.standard_normal((384, 7, 12)).astype(np.float32)).cuda(),
              u["manip"]: torch.from_numpy(rs.standard_normal((384, 7, 12)).astype(np.float32)).cuda(), "an_object_is_in_hand": [0]} for _ in range(n)]
    goals = ["find a mug", "navigate to the red chair and pick up the cup", "go to the kitchen", "pick up the apple on the table"]
    single = InferenceAgentVIDA.build_agent(model, device="cuda", nav_preprocessor=_Features(feats[0][u["nav"]][None]), manip_preprocessor=_Features(feats[0][u["manip"]][None]),
                                            generator=torch.Generator(device="cuda").manual_seed(1))
    raw = {"raw_navigation_camera": np.zeros((2, 2, 3), np.uint8), "raw_manipulation_camera": np.zeros((2, 2, 3), np.uint8), "an_object_is_in_hand": np.array([0])}
    vector = InferenceAgentVIDA.build_vector_agent(model, num_episodes=n, device="cuda", seed=1)

    def single_episode(steps=STEPS):
        single.reset()
        for _ in range(steps):
            single.get_action(raw, goals[0])

    def vector_episode(steps=STEPS):
        for s in range(n):
            vector.reset(s, goals[s % len(goals)])
        obs = dict(enumerate(feats))
        for _ in range(steps):
            vector.get_actions(obs)

    ts = {"single": [], "vector": []}
    for name, fn in (("single", single_episode), ("vector", vector_episode)):      # one kind of agent on the model at a time
        fn(WARMUP)
        torch.cuda.synchronize()
        for _ in range(reps):
            ts[name].append(timed(fn) / STEPS)
    (sm, sl, sh), (vm, vl, vh) = stats(ts["single"]), stats(ts["vector"])
    say(f"agent N={n:2d}: one single step {sm:6.3f} ms (min {sl:.3f}, max {sh:.3f}) -> {n} in turn {n * sm:8.3f} ms; one vector step of {n} episodes {vm:7.3f} ms "
        f"(min {vl:.3f}, max {vh:.3f}); ratio {n * sm / vm:.2f}")


def sample_ab(reps, n=64, A=20):
    g = torch.Generator(device="cuda").manual_seed(0)
    x = torch.randn(n, A, device="cuda", generator=g)
    slot, age = torch.arange(n, device="cuda", dtype=torch.int32), torch.zeros(n, device="cuda", dtype=torch.int32)

    def framework():
        lp = torch.log_softmax(x, -1)
        p = lp.exp()
        return lp, p, torch.multinomial(p, 1, generator=g), torch.argmax(x, -1)

    forms = {"log_softmax + exp + multinomial + argmax": framework, "ops.policy_sample_rows                  ": lambda: ops.policy_sample_rows(x, slot, age, 7)}
    for f in forms.values():
        for _ in range(WARMUP):
            f()
    torch.cuda.synchronize()
    ts = {name: [] for name in forms}
    for _ in range(reps):
        for name, f in forms.items():
            ts[name].append(1e3 * timed(lambda: [f() for _ in range(CALLS)]) / CALLS)
    lp, p, _, gr = framework()
    klp, kp, _, kg = ops.policy_sample_rows(x, slot, age, 7)
    for name in forms:
        med, lo, hi = stats(ts[name])
        say(f"sample n={n} A={A}  {name}: {med:7.2f} us per call (min {lo:.2f}, max {hi:.2f})")
    say(f"sample n={n} A={A}  max |log_probs difference| {float((lp - klp).abs().max()):.2e}, max |probs difference| {float((p - kp).abs().max()):.2e}, "
        f"greedy equal: {bool((gr == kg.long()).all())}")


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "vector_vida_ab.txt"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs an MI355X"
    from safevla_amd.model import SafeDinoLLAMATxNavActorCriticSeparate

    torch.manual_seed(0)
    model = SafeDinoLLAMATxNavActorCriticSeparate(device="cuda").eval()
    say("Vector RL agent (safevla_amd/agent.py: VectorInferenceAgentVIDA; csrc/sample.hip) against the single InferenceAgentVIDA.  One process:\n"
        "  python tools/ab_vector_vida.py\n"
        f"HIP events, {WARMUP} warm-up steps, {a.reps} repetitions per figure; median (min, max) of the repetitions.  Device: {torch.cuda.get_device_name(0)}.\n"
        f"(a) agent: one full-sensor policy, eval mode, pre-encoded features on both sides (no ViT).  A repetition is one episode of {STEPS} steps, reset included.  single: the\n"
        "    agent as it ships (rollout storage, three towers on the recorded, tower-grouped path, framework sampling), N consecutive steps of ONE agent on one model\n"
        "    copy (N agents would need N copies); vector: one step of all N slots, actor tower only, goals of 4 ... 11 tokens padded to the longest.\n"
        f"(b) sample: n = 64 rows of 20 actions, a repetition is {CALLS} calls, the two forms alternate repetition by repetition.\n")
    for n in (32, 8):
        agent_ab(model, n, a.reps)
    sample_ab(a.reps)
    with open(a.out, "w") as fh:
        fh.write("\n".join(LINES) + "\n")
