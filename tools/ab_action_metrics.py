#!/usr/bin/env python3
"""A/B of the validation-metrics kernel (csrc/metrics.hip: svla_action_metrics_f32 through ops.action_metrics) against the framework calls it replaces, one process,
HIP events, 5 warm-up repetitions, then 20 (``--reps``); median, min and max go to stdout and to ``--out`` (profiles/action_metrics_ab.txt).
  one launch   ops.action_metrics(logits, target, counts, sums): argmax, confusion counts and summed cross-entropy into accumulators that stay on the device;
  framework    torch.argmax + F.cross_entropy(ignore_index=-1, reduction="sum") + torch.bincount over target * A + pred (ignored rows sent to an extra bin), added
               into the same kind of accumulators.  No explicit host read is timed on this side either, but bincount has one of its own (it sizes its output by the
               largest index) -- the host read per batch that the kernel saves.
at rows = 16 x 50 (one training-sized batch of the default flags) and 16 x 1000 (whole episodes), A = 20, about 30 % of the targets -1.  A repetition is 200 calls;
the two forms alternate repetition by repetition; us per call.  At these sizes both sides are launch and wrapper cost, not kernel time.
  python tools/ab_action_metrics.py [--reps 20] [--out profiles/action_metrics_ab.txt]"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
import torch.nn.functional as F
from safevla_amd import ops

WARMUP, CALLS, A = 5, 200, 20
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


def ab(rows, reps):
    g = torch.Generator(device="cuda").manual_seed(rows)
    x = torch.randn(rows, A, device="cuda", generator=g) * 1.5
    t = torch.randint(0, A, (rows,), device="cuda", generator=g)
    t = torch.where(torch.rand(rows, device="cuda", generator=g) < 0.3, torch.full_like(t, -1), t)
    k_counts, k_sums = torch.zeros(A, A, device="cuda", dtype=torch.int64), torch.zeros(3, device="cuda", dtype=torch.float64)
    f_counts, f_sums = torch.zeros(A * A + 1, device="cuda", dtype=torch.int64), torch.zeros(2, device="cuda", dtype=torch.float64)

    def kernel():
        ops.action_metrics(x, t, k_counts, k_sums)

    def framework():
        pred = torch.argmax(x, -1)
        valid = t != -1
        f_sums[0] += F.cross_entropy(x, t, ignore_index=-1, reduction="sum")
        f_sums[1] += valid.sum()
        f_counts.add_(torch.bincount(torch.where(valid, t * A + pred, A * A), minlength=A * A + 1))

    forms = {"argmax + cross_entropy + bincount": framework, "ops.action_metrics               ": kernel}
    for f in forms.values():
        for _ in range(WARMUP):
            timed(lambda: [f() for _ in range(CALLS)])
    ts = {name: [] for name in forms}
    for _ in range(reps):
        for name, f in forms.items():
            ts[name].append(1e3 * timed(lambda: [f() for _ in range(CALLS)]) / CALLS)
    for name in forms:
        say(f"rows={rows:6d} A={A}  {name}: {statistics.median(ts[name]):7.2f} us per call (min {min(ts[name]):.2f}, max {max(ts[name]):.2f})")
    # both sides saw the same number of calls: the same state
    same_counts = bool((k_counts.reshape(-1) == f_counts[:A * A]).all())
    rel = abs(float(k_sums[0]) - float(f_sums[0])) / max(1.0, abs(float(f_sums[0])))
    say(f"rows={rows:6d} A={A}  counts equal: {same_counts}; frames {int(k_sums[1])} against {int(f_sums[1])}; summed loss differs by {rel:.2e} (relative); refused rows {int(k_sums[2])}")


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "action_metrics_ab.txt"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs an MI355X"
    say("Validation metrics of one batch: one launch of svla_action_metrics_f32 (csrc/metrics.hip) against argmax + F.cross_entropy(reduction='sum') + bincount.\n"
        "  python tools/ab_action_metrics.py\n"
        f"One process, HIP events, {WARMUP} warm-up repetitions, then {a.reps}; median (min, max); a repetition is {CALLS} calls, the two forms alternate repetition by\n"
        f"repetition.  Device: {torch.cuda.get_device_name(0)}.  A = {A}, about 30 % of the targets -1; both sides add into accumulators on the device, neither\n"
        "is read back inside the timed window (bincount synchronises with the host on its own).  No threshold: at these sizes this is launch and wrapper cost.\n")
    for rows in (16 * 50, 16 * 1000):
        ab(rows, a.reps)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(LINES) + "\n")
