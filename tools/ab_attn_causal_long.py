#!/usr/bin/env python3
"""A/B of the streaming causal attention forward (csrc/attn_seq_long.hip: ops.attn_causal_fwd) against the route it replaces, one process, HIP events, 5 warm-up
calls and 20 repetitions per figure (``--reps``); median, min and max of the repetitions are printed.
  (a) kernel  rows x H x S = 8 x 8 x 1000, 8 x 8 x 513 and 64 x 8 x 600 on fused qkv rows.  Old: ops.attn_decode_rows with rows * S single-query rows, klen = t + 1
              (what Tower._decoder_window_fwd issued for every window above 512 steps).  New: ops.attn_causal_fwd, traj = None.  Every launch works on one of NBUF
              qkv buffers in turn; a repetition is ROUNDS rounds over the buffers, and the two kernels alternate repetition by repetition.
  (b) agent   one vector agent of 8 ``small_3`` slots on pre-encoded features whose episodes have outlived their window of W = 1000 steps: ms per step of all 8
              with the window on single-query rows (model.WINDOW_DECODE_ROWS = True) and on the streaming kernel, alternating repetition by repetition.
  (c) episode ``forward(batch)`` of ``small_3`` at B = 1, T = 1000 on pre-encoded features under torch.no_grad(): absolute ms (there is no old route: above 512 steps
              the forward used to raise).
  python tools/ab_attn_causal_long.py [--reps 20] [--skip-agent]"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from safevla_amd import ops

H, HD = 8, 64
D = H * HD
NBUF, ROUNDS, WARMUP = 5, 2, 5


def timed(fn):
    """one repetition of ``fn`` between two HIP events -> ms"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def stats(ts):
    return statistics.median(ts), min(ts), max(ts)


def kernel_ab(rows, S, reps):
    g = torch.Generator(device="cuda").manual_seed(S)
    bufs = [(torch.randn(rows * S, 3 * D, device="cuda", generator=g) * 0.5).to(torch.bfloat16) for _ in range(NBUF)]
    crow = torch.arange(rows, device="cuda", dtype=torch.int32).repeat_interleave(S)
    klen = (torch.arange(S, device="cuda") + 1).to(torch.int32).repeat(rows)
    out = torch.empty(rows * S, D, device="cuda", dtype=torch.bfloat16)
    forms = {"attn_decode_rows, rows * S queries": lambda x: ops.attn_decode_rows(x, 3 * D, x[:, D:], x[:, 2 * D:], 3 * D, klen, crow, rows * S, H, 0.125, S, out=out),
             "attn_causal_fwd                   ": lambda x: ops.attn_causal_fwd(x, x[:, D:], x[:, 2 * D:], 3 * D, rows, S, H, 0.125, out=out)}
    outs = {}
    for name, f in forms.items():
        for x in bufs[:WARMUP]:
            f(x)
        outs[name] = out.clone()
    torch.cuda.synchronize()
    ts = {name: [] for name in forms}
    for _ in range(reps):
        for name, f in forms.items():
            ts[name].append(1e3 * timed(lambda: [f(x) for _ in range(ROUNDS) for x in bufs]) / (ROUNDS * NBUF))
    med = {}
    for name in forms:
        med[name], lo, hi = stats(ts[name])
        print(f"kernel rows={rows:2d} H={H} S={S:4d}  {name}: {med[name]:8.2f} us per launch (min {lo:.2f}, max {hi:.2f})")
    a, b = outs.values()
    old, new = med.values()
    print(f"kernel rows={rows:2d} H={H} S={S:4d}  old / new {old / new:.2f}; max |difference| of the two outputs {float((a.float() - b.float()).abs().max()):.2e}")


def window_ab(n, W, reps):
    from safevla_amd import model as M
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
    for _ in range(WARMUP):
        step()
    assert vector.age(0) >= W
    saved = M.WINDOW_DECODE_ROWS
    ts = {True: [], False: []}
    try:
        for old in (True, False):
            M.WINDOW_DECODE_ROWS = old
            for _ in range(WARMUP):
                step()
        for _ in range(reps):
            for old in (True, False):
                M.WINDOW_DECODE_ROWS = old
                ts[old].append(timed(step))
    finally:
        M.WINDOW_DECODE_ROWS = saved
    (om, ol, oh), (nm, nl, nh) = stats(ts[True]), stats(ts[False])
    print(f"window small_3 N={n} W={W:4d}: a step inside the window {inside[0]:7.3f} ms (min {inside[1]:.3f}, max {inside[2]:.3f}); beyond it, on single-query rows "
          f"{om:7.3f} ms (min {ol:.3f}, max {oh:.3f}), on the streaming kernel {nm:7.3f} ms (min {nl:.3f}, max {nh:.3f}); old / new {om / nm:.2f}")


def episode(T, reps):
    from safevla_amd.il import EarlyFusionCnnTransformer

    rs = np.random.RandomState(T)
    torch.manual_seed(0)
    m = EarlyFusionCnnTransformer.build_model("small_3", device="cuda").eval()
    feat = lambda: torch.from_numpy(rs.standard_normal((1, T, 384, 7, 12)).astype(np.float32)).cuda()
    batch = {"raw_navigation_camera": feat(), "raw_manipulation_camera": feat(), "time_ids": torch.arange(T, device="cuda")[None],
             "an_object_is_in_hand": torch.zeros(1, T, dtype=torch.int64, device="cuda"),
             "last_actions": torch.from_numpy(np.concatenate([[20], rs.randint(0, 20, T - 1)])[None]).cuda(),
             "goals": dict(input_ids=torch.tensor([[917, 4033, 88, 21, 1]], device="cuda"), attention_mask=torch.ones(1, 5, dtype=torch.int64, device="cuda"))}
    with torch.no_grad():
        for _ in range(WARMUP):
            out = m(batch)["actions_logits"]
        assert out.shape == (1, T, 20) and torch.isfinite(out).all()
        med, lo, hi = stats([timed(lambda: m(batch)) for _ in range(reps)])
    print(f"episode small_3 B=1 T={T}: forward(batch) {med:8.3f} ms (min {lo:.3f}, max {hi:.3f})")


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--skip-agent", action="store_true")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs an MI355X"
    for rows, S in ((8, 1000), (8, 513), (64, 600)):
        kernel_ab(rows, S, a.reps)
        torch.cuda.empty_cache()
    if not a.skip_agent:
        window_ab(8, 1000, a.reps)
        torch.cuda.empty_cache()
        episode(1000, a.reps)
