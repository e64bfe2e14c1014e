#!/usr/bin/env python3
"""What the two vector agents compute and launch on a fixed script, as text that two revisions can be compared by (``diff``): run it on each, one process each.
Weights: oracle.detfill.  Per agent the script is
  staggered  3 slots with goals of 3, 5 and 7 tokens that start at calls 0, 2 and 4; slot 1 sits out calls 5 and 6; slot 0 is reset at call 5 (4 tokens); 12 calls
  window     one slot for 11 steps at a KV window of 8
on ``il.EarlyFusionCnnTransformerVectorAgent`` (small_3; greedy, and ``sample`` under a seeded generator) and ``agent.VectorInferenceAgentVIDA`` (seed 21).  Per call
it prints the returned actions, the SHA-256 of the returned probabilities' bytes (slots in ascending order) and the SHA-256 of the call's launches: the ordered C-ABI
entry names with their non-pointer arguments (``ops.lib().recorder``).  Every distinct launch list is printed in full once, under its hash.
  python tools/vector_agent_digest.py [--out FILE]"""
import argparse
import ctypes
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from oracle.detfill import fill_state_dict
from safevla_amd import ops

DEV = "cuda"
LINES, SEEN = [], set()


def say(line):
    print(line, flush=True)
    LINES.append(line)


def goal(rs, n_tokens):
    ids = np.concatenate([rs.randint(3, 32000, n_tokens - 1), [1]])[None]
    return dict(input_ids=ids, attention_mask=np.ones_like(ids))


def step(name, call, agent, frames):
    lib = ops.lib()
    lib.recorder = []
    try:
        out = agent.get_actions(frames)
        trace = lib.recorder
    finally:
        lib.recorder = None
    launches = [f"{fn.__name__}({','.join(repr(a) for a, ct in zip(args, fn.argtypes) if ct is not ctypes.c_void_p)})" for fn, args in trace]
    lh = hashlib.sha256("\n".join(launches).encode()).hexdigest()[:16]
    if lh not in SEEN:
        SEEN.add(lh)
        say(f"launches {lh} ({len(launches)}): " + " ".join(launches))
    probs = torch.stack([out[s][1] for s in sorted(out)]).contiguous().cpu().numpy()
    say(f"{name} call {call:2d}: actions {({s: out[s][0] for s in sorted(out)})} probs {probs.dtype}{list(probs.shape)} sha256 {hashlib.sha256(probs.tobytes()).hexdigest()} "
        f"launches {lh}")


def staggered(name, agent, frame):
    rs = np.random.RandomState(8)
    start, lengths, live = {0: 0, 1: 2, 2: 4}, {0: 3, 1: 5, 2: 7}, set()
    for call in range(12):
        for s, c0 in start.items():
            if call == c0:
                agent.reset(s, goal(rs, lengths[s]))
                live.add(s)
        if call == 5:
            agent.reset(0, goal(rs, 4))
        step(name, call, agent, {s: frame(rs) for s in sorted(live) if not (s == 1 and call in (5, 6))})
    say(f"{name}: ages {[agent.age(s) for s in range(3)]}")


def window(name, agent, frame):
    rs = np.random.RandomState(9)
    agent.reset(1, goal(rs, 5))
    for call in range(11):
        step(name, call, agent, {1: frame(rs)})
    say(f"{name}: age {agent.age(1)}")


def il_agents():
    from safevla_amd.il import EarlyFusionCnnTransformer, EarlyFusionCnnTransformerVectorAgent

    m = EarlyFusionCnnTransformer.build_model("small_3", device=DEV)
    fill_state_dict(m, seed=17, share_t5=False)
    m.sync_weights()
    frame = lambda rs: {"raw_navigation_camera": rs.standard_normal((m.dino_dim, 7, 12)).astype(np.float32),
                        "raw_manipulation_camera": rs.standard_normal((m.dino_dim, 7, 12)).astype(np.float32), "an_object_is_in_hand": [int(rs.randint(0, 2))]}
    for sampling in ("greedy", "sample"):
        kw = dict(sampling=sampling, generator=torch.Generator(device=DEV).manual_seed(1234) if sampling == "sample" else None)
        staggered(f"il small_3 {sampling} staggered", EarlyFusionCnnTransformerVectorAgent(m.eval(), 3, DEV, **kw), frame)
        window(f"il small_3 {sampling} window 8", EarlyFusionCnnTransformerVectorAgent(m, 2, DEV, max_seq_len=8, **kw), frame)


def rl_agents():
    from safevla_amd.agent import InferenceAgentVIDA
    from safevla_amd.model import SafeDinoLLAMATxNavActorCriticSeparate

    frame = lambda rs: {"rgb_dinov2": rs.standard_normal((384, 7, 12)).astype(np.float32), "manipulation_rgb_dinov2": rs.standard_normal((384, 7, 12)).astype(np.float32),
                        "an_object_is_in_hand": [int(rs.randint(0, 2))]}
    for name, n, kw, script in (("rl seed 21 staggered", 3, {}, staggered), ("rl seed 21 window 8", 2, dict(max_steps=8), window)):
        m = SafeDinoLLAMATxNavActorCriticSeparate(device=DEV, **kw)
        fill_state_dict(m, seed=7)
        m.sync_weights()
        script(name, InferenceAgentVIDA.build_vector_agent(m.eval(), num_episodes=n, device=DEV, seed=21), frame)


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--out", default=None, help="also write the lines to this file")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs an MI355X"
    il_agents()
    rl_agents()
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("\n".join(LINES) + "\n")
