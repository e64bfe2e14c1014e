#!/usr/bin/env python3
"""A/B of the vector IL agent (safevla_amd/il.py: EarlyFusionCnnTransformerVectorAgent on per-row KV rings, csrc/attn_decode.hip), one process, HIP events,
5 warm-up calls and 20 repetitions per figure (``--reps``); median, min and max of the repetitions are printed.
  (a) kernel  ops.attn_decode_rows against ops.attn_fwd with a prefix ``kvalid`` (attn_decode_long_kernel of the same file) at 64 rows x 8 heads, window 1000, with 100 and with
              1000 valid keys.  As in tools/ab_attn_decode_long.py every launch works on one of nine caches in turn (1.2 GB: more than the last-level cache
              holds); a repetition is 45 launches (five rounds over the caches), and the two kernels alternate repetition by repetition.
  (b) agent   N single agents (one model copy each, as the reference's evaluation workers hold) stepped in turn against ONE vector agent of N slots, N = 1, 8, 32:
              ``small_3`` on pre-encoded features, greedy.  A call = one step of all N episodes; a repetition = one episode of 50 steps in all N (reset included);
              the figure is ms per step of all N.
  (c) window  one vector agent of 8 slots whose episodes have outlived their window of W = 100 and W = 1000 steps: a step then decodes the last W steps anew
              (Tower._decoder_window_fwd) instead of one token against the KV ring; ms per step of all 8, next to the same agent's step inside the window.
  python tools/ab_vector_agent.py [--reps 20] [--skip-agent]"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from safevla_amd import ops

H, HD, ROWS, W = 8, 64, 64, 1000
D = H * HD
NBUF, ROUNDS, WARMUP, STEPS = 9, 5, 5, 50


def timed(fn):
    """one repetition of ``fn`` between two HIP events -> ms"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def stats(ts):
    return statistics.median(ts), min(ts), max(ts)


def kernel_ab(valid, reps):
    g = torch.Generator(device="cuda").manual_seed(valid)
    caches = [(torch.randn(ROWS * W, 2 * D, device="cuda", generator=g) * 0.5).to(torch.bfloat16) for _ in range(NBUF)]
    qkv = (torch.randn(ROWS, 3 * D, device="cuda", generator=g) * 0.5).to(torch.bfloat16)
    kvalid = torch.zeros(ROWS, W, device="cuda", dtype=torch.uint8)
    kvalid[:, :valid] = 1
    klen = torch.full((ROWS,), valid, device="cuda", dtype=torch.int32)
    out = torch.empty(ROWS, D, device="cuda", dtype=torch.bfloat16)
    forms = {"attn_fwd + prefix kvalid": lambda c: ops.attn_fwd(qkv, c, c[:, D:], 2 * D, ROWS, W, H, 0.125, kvalid=kvalid, save_lse=False, Sq=1, ldq=3 * D, kv_rows=W, out=out),
             "attn_decode_rows        ": lambda c: ops.attn_decode_rows(qkv, 3 * D, c, c[:, D:], 2 * D, klen, None, ROWS, H, 0.125, W, out=out)}
    outs = {}
    for name, f in forms.items():
        for c in caches[:WARMUP]:
            f(c)
        outs[name] = out.clone()
    torch.cuda.synchronize()
    ts = {name: [] for name in forms}
    for _ in range(reps):
        for name, f in forms.items():
            ts[name].append(1e3 * timed(lambda: [f(c) for _ in range(ROUNDS) for c in caches]) / (ROUNDS * NBUF))
    a, b = outs.values()
    kb = ROWS * H * valid * 2 * HD * 2 / 1024
    for name in forms:
        med, lo, hi = stats(ts[name])
        print(f"kernel rows={ROWS} H={H} window={W} valid={valid:4d}  {name}: {med:7.2f} us per launch (min {lo:.2f}, max {hi:.2f}; {kb:6.0f} KiB of K and V read)")
    print(f"kernel rows={ROWS} H={H} window={W} valid={valid:4d}  max |difference| of the two outputs {float((a.float() - b.float()).abs().max()):.2e}")


def agent_ab(n, reps):
    from safevla_amd.il import EarlyFusionCnnTransformer, EarlyFusionCnnTransformerAgent, EarlyFusionCnnTransformerVectorAgent

    rs = np.random.RandomState(n)
    frame = lambda: {"raw_navigation_camera": rs.standard_normal((384, 7, 12)).astype(np.float32),
                     "raw_manipulation_camera": rs.standard_normal((384, 7, 12)).astype(np.float32), "an_object_is_in_hand": [0]}
    frames = [frame() for _ in range(n)]
    goals = [dict(input_ids=np.concatenate([rs.randint(3, 32000, 3 + s % 5), [1]])[None]) for s in range(n)]          # 4 ... 8 tokens
    for g in goals:
        g["attention_mask"] = np.ones_like(g["input_ids"])
    torch.manual_seed(0)
    singles = [EarlyFusionCnnTransformerAgent(EarlyFusionCnnTransformer.build_model("small_3", device="cuda"), "cuda") for _ in range(n)]
    vector = EarlyFusionCnnTransformerVectorAgent(EarlyFusionCnnTransformer.build_model("small_3", device="cuda"), n, "cuda")

    def single_episode(steps=STEPS):
        for a in singles:
            a.reset()
        for _ in range(steps):
            for a, f, g in zip(singles, frames, goals):
                a.get_action(f, g)

    def vector_episode(steps=STEPS):
        for s, g in enumerate(goals):
            vector.reset(s, g)
        obs = dict(enumerate(frames))
        for _ in range(steps):
            vector.get_actions(obs)

    single_episode(WARMUP); vector_episode(WARMUP)
    torch.cuda.synchronize()
    ts = {"single": [], "vector": []}
    for _ in range(reps):
        ts["single"].append(timed(single_episode) / STEPS)
        ts["vector"].append(timed(vector_episode) / STEPS)
    (sm, sl, sh), (vm, vl, vh) = stats(ts["single"]), stats(ts["vector"])
    print(f"agent small_3 N={n:2d}: {n} single agents in turn {sm:8.3f} ms per step of all N (min {sl:.3f}, max {sh:.3f}); one vector agent {vm:8.3f} ms "
          f"(min {vl:.3f}, max {vh:.3f}); ratio {sm / vm:.2f}")


def window_cost(n, W, reps):
    from safevla_amd.il import EarlyFusionCnnTransformer, EarlyFusionCnnTransformerVectorAgent

    rs = np.random.RandomState(W)
    obs = {s: {"raw_navigation_camera": rs.standard_normal((384, 7, 12)).astype(np.float32),
               "raw_manipulation_camera": rs.standard_normal((384, 7, 12)).astype(np.float32), "an_object_is_in_hand": [0]} for s in range(n)}
    torch.manual_seed(0)
    vector = EarlyFusionCnnTransformerVectorAgent(EarlyFusionCnnTransformer.build_model("small_3", device="cuda"), n, "cuda", max_seq_len=W)
    for s in range(n):
        vector.reset(s, dict(input_ids=np.array([[917, 4033, 88, 21, 1]]), attention_mask=np.ones((1, 5), np.int64)))
    step = lambda: vector.get_actions(obs)
    for _ in range(W - reps - WARMUP):
        step()
    inside = stats([timed(step) for _ in range(reps)])                  # the last steps inside the window: the longest KV rings
    for _ in range(2 * WARMUP):
        step()
    assert vector.age(0) >= W
    beyond = stats([timed(step) for _ in range(reps)])
    print(f"window small_3 N={n} W={W:4d}: a step inside the window {inside[0]:7.3f} ms (min {inside[1]:.3f}, max {inside[2]:.3f}); beyond it, decoded over the "
          f"window {beyond[0]:7.3f} ms (min {beyond[1]:.3f}, max {beyond[2]:.3f})")


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--skip-agent", action="store_true")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs an MI355X"
    for valid in (100, 1000):
        kernel_ab(valid, a.reps)
    if not a.skip_agent:
        for n in (1, 8, 32):
            agent_ab(n, a.reps)
            torch.cuda.empty_cache()
        for W in (100, 1000):
            window_cost(8, W, a.reps)
            torch.cuda.empty_cache()
