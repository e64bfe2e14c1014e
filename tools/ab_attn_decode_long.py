#!/usr/bin/env python3
"""A/B of the single-query ("decode") attention forward over long KV-cache windows (csrc/attn_decode.hip: attn_decode_long_kernel, head_dim 64, 512 < S <= 1024) against the kernel for
S <= 512 (attn_decode_kernel of the same file), per launch at rows = 64 and rows = 1 with H = 8:
  baseline  S = 500, all 500 keys valid, and S = 500 with a 100-key window (run this file on the previous revision for the baseline of record: the S > 512 lines then
            print 'refused');
  long      S = 1000 with 1000 valid keys (twice the bytes of the baseline) and S = 1000 with a 100-key window at slots 850 .. 949 (what the recorded acting path
            issues at step 949 of an episode that began at slot 850: S is the whole window at every step, the mask hides the rest).
Every launch of a case works on one of nine caches in turn (3 towers x 3 decoder layers: 1.2 GB at rows = 64, S = 1000 -- more than the last-level cache holds).
HIP-event timing: 10 warm-up launches, then 31 timed batches of 45 launches; the median batch / 45 is the figure, min and max batch are printed with it.
``--policy-step`` adds the whole KV-cached three-tower policy step at 64 envs (recorded, tower-grouped) for max_steps = 500 and max_steps = 1000."""
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from safevla_amd import ops
from safevla_amd._lib import SvlaError

H, HD = 8, 64
D = H * HD
NBUF, BATCH, NBATCH = 9, 45, 31


def per_launch_us(fns):
    """fns: the launches of one round over the buffers; (median, min, max) us per launch"""
    for _ in range(2):
        for f in fns: f()
    torch.cuda.synchronize()
    reps = BATCH // len(fns)
    ts = []
    for _ in range(NBATCH):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            for f in fns: f()
        e1.record(); torch.cuda.synchronize()
        ts.append(1e3 * e0.elapsed_time(e1) / (reps * len(fns)))
    return statistics.median(ts), min(ts), max(ts)


def case(rows, S, lo, hi):
    g = torch.Generator(device="cuda").manual_seed(rows + S)
    caches = [(torch.randn(rows * S, 2 * D, device="cuda", generator=g) * 0.5).to(torch.bfloat16) for _ in range(NBUF)]
    qkv = (torch.randn(rows, 3 * D, device="cuda", generator=g) * 0.5).to(torch.bfloat16)
    kvalid = torch.zeros(rows, S, device="cuda", dtype=torch.uint8)
    kvalid[:, lo:hi + 1] = 1
    out = torch.empty(rows, D, device="cuda", dtype=torch.bfloat16)
    mk = lambda c: (lambda: ops.attn_fwd(qkv, c, c[:, D:], 2 * D, rows, S, H, 0.125, kvalid=kvalid, save_lse=False, Sq=1, ldq=3 * D, kv_rows=S, out=out))
    try:
        return per_launch_us([mk(c) for c in caches])
    except SvlaError:
        return None


def policy_step(max_steps, n=200):
    from safevla_amd.model import SafeDinoLLAMATxNavActorCriticSeparate
    from safevla_amd.synth_env import SynthSpec, fill_synthetic_rollout
    torch.manual_seed(1234)
    m = SafeDinoLLAMATxNavActorCriticSeparate(device="cuda", max_steps=max_steps)
    B = 64
    st, _, _ = fill_synthetic_rollout(m, SynthSpec(T=24, B=B, L=12, task="PickUp", seed=1234), device="cuda")
    step_in = lambda t: ({k: v[t % 24:t % 24 + 1] for k, v in st.observations.items()}, None, st.prev_actions[t % 24:t % 24 + 1], st.masks[t % 24:t % 24 + 1])
    for t in m.towers:
        t.time_step_counter, t._kv = 0, None
    ts = []
    with torch.no_grad():
        for t in range(8):
            m(*step_in(t))
        torch.cuda.synchronize()
        for b in range(5):                     # five windows of n / 5 steps: the spread between them is printed
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for t in range(n // 5):
                m(*step_in(8 + b * (n // 5) + t))
            e1.record(); torch.cuda.synchronize()
            ts.append(e0.elapsed_time(e1) / (n // 5))
    return statistics.median(ts), min(ts), max(ts)


if __name__ == "__main__":
    base = {}
    for rows in (64, 1):
        for name, S, lo, hi in (("S= 500 full window      ", 500, 0, 499), ("S= 500 100 valid keys   ", 500, 350, 449), ("S=1000 full window      ", 1000, 0, 999),
                                ("S=1000 100 valid keys   ", 1000, 850, 949), ("S=1000 500 valid keys   ", 1000, 450, 949)):
            r = case(rows, S, lo, hi)
            if r is None:
                print(f"rows={rows:2d} {name}: refused")
                continue
            base.setdefault(rows, {})[(S, hi - lo + 1)] = r[0]
            b = base[rows].get((500, 500 if hi - lo + 1 >= 500 else 100))
            kb = rows * H * (hi - lo + 1) * 2 * HD * 2 / 1024
            print(f"rows={rows:2d} {name}: {r[0]:7.2f} us per launch (min {r[1]:.2f}, max {r[2]:.2f}; {kb:8.0f} KiB of K and V read)"
                  + (f" = {r[0] / b:.2f} x this run's S=500 case with {'500' if hi - lo + 1 >= 500 else '100'} valid keys" if b and S > 512 else ""))
    if "--policy-step" in sys.argv:
        for ms in (500, 1000):
            try:
                r = policy_step(ms)
                print(f"policy step, 64 envs, max_steps={ms:4d}: {r[0]:.3f} ms per step (windows of 40 steps: min {r[1]:.3f}, max {r[2]:.3f})")
            except (SvlaError, ValueError) as e:
                print(f"policy step, 64 envs, max_steps={ms:4d}: refused ({type(e).__name__})")
