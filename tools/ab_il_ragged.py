#!/usr/bin/env python3
"""A/B of ``EarlyFusionCnnTransformer(skip_padded_steps=...)``: one ``ILTrainer.training_step`` and one ``validation_step`` of ``small_3`` with the flag off against
the flag on, on the SAME batch with the same weights (one model; the flag is an attribute), one process.
  batches      pre-encoded DINOv2-S features at B = 16, T = 100 (``--feat_bt``) and raw 224 x 384 frames through the frozen trunk at B = 4, T = 32 (``--raw_bt``);
               0 %, about 30 % and about 60 % of the B * T steps padded: the first trajectory keeps all T steps, the others spread linearly around the length that makes
               the mean 100 %, 70 % and 40 % of T.  Padding as il.Preprocessor writes it; ``lengths`` is a host tensor.
  flag off     every padded step runs (``lengths`` is ignored): the path of a model built without the flag;
  flag on      everything in front of the decoder runs on the valid steps only; at 0 % padding ``prepare`` returns the same Prep (no row table): the same path.
  timing       host clock around a step that ends in a device synchronise (training_step reads its loss; validation_step is followed by torch.cuda.synchronize()),
               3 warm-up steps per form and batch, then ``--reps`` (10) steps per form, the two forms alternating step by step; median (min, max) in ms.
               training_step updates the weights, so the two forms see weights one step apart: the same work.
  python tools/ab_il_ragged.py [--reps 10] [--out profiles/il_ragged_ab.txt]"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from safevla_amd.il import MANIP, NAV, PAD_TOKEN, START_TOKEN, EarlyFusionCnnTransformer, ILTrainer

WARMUP = 3
LINES = []


def say(line):
    print(line, flush=True)
    LINES.append(line)


def lengths_for(B, T, mean_share):
    """the first trajectory keeps T steps; the others spread linearly over +-40 % around the length that makes the batch's mean mean_share * T"""
    if mean_share >= 1.0 or B == 1:
        return [T] * B
    x = (mean_share * B - 1.0) * T / (B - 1)
    return [T] + [int(min(T, max(1, round(v)))) for v in np.linspace(1.4 * x, 0.6 * x, B - 1)]


def make_batch(B, T, lens, raw, dev, seed):
    g = torch.Generator(device=dev).manual_seed(seed)
    ln = torch.tensor(lens, device=dev)
    tt = torch.arange(T, device=dev)[None, :].expand(B, T).clone()
    pad = tt >= ln[:, None]
    actions = torch.randint(0, 20, (B, T), device=dev, generator=g)
    last = torch.cat([torch.full((B, 1), START_TOKEN, device=dev), actions[:, :-1]], 1)
    hand = torch.randint(0, 2, (B, T), device=dev, generator=g)
    last[pad], actions[pad], hand[pad], tt[pad] = PAD_TOKEN, -1, 2, -1
    L = 12
    n_tok = torch.randint(4, L + 1, (B,), device=dev, generator=g)
    am = (torch.arange(L, device=dev)[None, :] < n_tok[:, None]).to(torch.int64)
    ids = torch.randint(3, 32000, (B, L), device=dev, generator=g) * am
    ids[torch.arange(B, device=dev), n_tok - 1] = 1
    batch = {"time_ids": tt, "an_object_is_in_hand": hand, "last_actions": last, "actions": actions, "padding_mask": pad,
             "goals": dict(input_ids=ids, attention_mask=am), "lengths": torch.tensor(lens, dtype=torch.int32)}
    for cam in (NAV, MANIP):
        if raw:
            x = torch.randint(0, 256, (B, T, 224, 384, 3), device=dev, generator=g).to(torch.uint8)
        else:
            x = torch.randn(B, T, 384, 7, 12, device=dev, generator=g)
        x[pad] = 0
        batch[cam] = x
    return batch


def step_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0)


def ab(model, trainer, kind, B, T, reps, dev):
    raw = kind == "raw frames"
    for share in (1.0, 0.7, 0.4):
        lens = lengths_for(B, T, share)
        valid = sum(lens)
        batch = make_batch(B, T, lens, raw, dev, seed=B * T + int(100 * share))
        model.skip_padded_steps = True
        same_path = model.prepare(batch).row_map is None
        steps = {"training_step  ": lambda: trainer.training_step(batch), "validation_step": lambda: trainer.validation_step(batch)}
        for sname, step in steps.items():
            ts = {False: [], True: []}
            for flag in (False, True):
                model.skip_padded_steps = flag
                for _ in range(WARMUP):
                    step_ms(step)
            for _ in range(reps):
                for flag in (False, True):
                    model.skip_padded_steps = flag
                    ts[flag].append(step_ms(step))
            med = {f: statistics.median(v) for f, v in ts.items()}
            say(f"{kind:13s} B={B:2d} T={T:3d} padded {100.0 * (1 - valid / (B * T)):4.1f} % ({valid:4d} of {B * T:4d} steps valid)  {sname}  "
                f"off {med[False]:8.2f} ms ({min(ts[False]):.2f}, {max(ts[False]):.2f})   on {med[True]:8.2f} ms ({min(ts[True]):.2f}, {max(ts[True]):.2f})   "
                f"off / on {med[False] / med[True]:5.2f}" + ("   [same path: no row table]" if same_path else ""))
        trainer.val_metrics.reset()


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--feat_bt", type=int, nargs=2, default=(16, 100))
    ap.add_argument("--raw_bt", type=int, nargs=2, default=(4, 32))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "il_ragged_ab.txt"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs an MI355X"
    dev = torch.device("cuda")
    torch.manual_seed(0)
    model = EarlyFusionCnnTransformer.build_model("small_3", device=dev, skip_padded_steps=True)
    trainer = ILTrainer(model, lr=1e-5)
    say("IL batches of unequal-length trajectories: small_3, one training_step and one validation_step, skip_padded_steps off against on, same batch, same model.\n"
        "  python tools/ab_il_ragged.py\n"
        f"One process; host clock around a step that ends in a device synchronise; {WARMUP} warm-up steps per form and batch, then {a.reps} per form, alternating step by\n"
        f"step; median (min, max) ms.  Device: {torch.cuda.get_device_name(0)}.  Train mode (dropout on) for training_step; validation_step runs in eval mode under no_grad.\n"
        "Flag off = the path of a model built without the flag (every padded step runs).  The share of padded steps is the upper bound of the saving in front of the\n"
        "decoder; the decoder, the heads, the loss and the optimiser step run on all B * T steps either way.\n")
    model.train()
    ab(model, trainer, "features", a.feat_bt[0], a.feat_bt[1], a.reps, dev)
    ab(model, trainer, "raw frames", a.raw_bt[0], a.raw_bt[1], a.reps, dev)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(LINES) + "\n")
