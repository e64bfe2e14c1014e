#!/usr/bin/env python3
"""Digests of the host schedule (safevla_amd/model.py, il.py): which C-ABI entry point runs with which arguments on which buffers, for a fixed list of small
configurations of the towers.  The host-side sibling of tools/isa_digest.py: equal digests before and after a change of the Python schedule mean that it issues the
same calls in the same order with the same arguments.  Needs a GPU and a built tree; one process, a few seconds per configuration.
  python tools/schedule_digest.py [--root OTHER_CHECKOUT] [--hold] [--dump-grad FILE.npy]
--root: the same configurations against another checkout's safevla_amd/ (and oracle/) in a child interpreter; a checkout without a built library runs on this
tree's (only valid while both trees have the same csrc/ and include/).  --hold: every tensor handed to a kernel stays alive until its configuration ends (the list
ops.LaunchPlan keeps, ``ops._REC.keep``), so no address is ever reused and the pointer digest shows the wiring alone, whatever the lifetimes.  --dump-grad: the
first configuration's gradient range as an fp32 array, for comparing two runs.

One line per configuration: the number of recorded calls (``lib().recorder``, the hook ops.LaunchPlan uses; for recorded acting steps the plans' own call lists) and
  scalars   sha256 over entry-point name + every non-pointer argument by value (per ``lib().decls``) + null / non-null of every pointer argument; of a dropout
            descriptor (the pointer arguments named ``drop``) its seed, stream, probability and row multiplier by value
  pointers  sha256 over the same trace with every device pointer replaced by the rank of its first appearance: buffer wiring and reuse after free, not addresses
  outputs   sha256 over the bytes of the forward outputs
  grads     sha256 over the bytes of the gradient range (configurations with a backward; the accumulating GEMMs' atomics make it run-dependent: reported only)
The tool hashes and prints; it inspects nothing."""
import argparse
import ctypes
import hashlib
import os
import struct
import subprocess
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda"
T, B, L = 3, 2, 12          # S = 169 + 12 = 181 fusion tokens, M = 1086 token rows, M2 = 1008 patch rows


class Trace:
    """the calls made while it is active (or a given call list), as the three digests"""

    hold = False

    def __init__(self, lib, ops):
        self.lib, self.ops, self.calls, self.keep, self.outputs, self.grads = lib, ops, [], [], hashlib.sha256(), None

    def __enter__(self):
        assert self.lib.recorder is None and self.ops._REC is None
        self.lib.recorder = self.calls
        if self.hold:
            self.ops._REC = self
        return self

    def __exit__(self, *exc):
        self.lib.recorder = self.ops._REC = None

    def out(self, *tensors):
        import torch
        torch.cuda.synchronize()
        for t in tensors:
            self.outputs.update(t.detach().contiguous().cpu().view(torch.uint8).numpy().tobytes())

    def grad(self, flat_g):
        import torch
        torch.cuda.synchronize()
        self.grads = flat_g.detach().cpu().numpy()

    def line(self, name):
        scal, ptrs, rank = hashlib.sha256(), hashlib.sha256(), {}

        def pointer(v):
            v = v.value if isinstance(v, ctypes.c_void_p) else v
            return int(v or 0)

        def both(b):
            scal.update(b); ptrs.update(b)

        def device_pointer(p):
            scal.update(b"n" if p == 0 else b"p")
            ptrs.update(struct.pack("<q", -1 if p == 0 else rank.setdefault(p, len(rank))))

        for fn, args in self.calls:
            both(fn.__name__.encode() + b"(")
            for (an, ct), v in zip(self.lib.decls[fn.__name__], args):
                if ct is ctypes.c_float or ct is ctypes.c_double:
                    both(struct.pack("<d", float(v)))
                elif ct is not ctypes.c_void_p:
                    both(struct.pack("<q", int(v)))
                elif an == "drop" and pointer(v):         # host descriptor: by value
                    d = self.ops._SvlaDropout.from_address(pointer(v))
                    both(struct.pack("<IIfi", d.seed, d.stream, d.p, d.row_mult))
                    device_pointer(int(d.seed_dev or 0))
                else:
                    device_pointer(pointer(v))
            both(b")")
        g = hashlib.sha256(self.grads.tobytes()).hexdigest()[:16] if self.grads is not None else "-" * 16
        print(f"{name:<34} calls {len(self.calls):5d}  scalars {scal.hexdigest()[:16]}  pointers {ptrs.hexdigest()[:16]}  "
              f"outputs {self.outputs.hexdigest()[:16]}  grads {g}", flush=True)


def run(root, dump_grad, hold):
    sys.path.insert(0, root)
    import numpy as np
    import torch

    import safevla_amd._lib as _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.LIB_PATH = os.path.join(HERE, "safevla_amd", "libsvla_hip.so")
    from oracle.detfill import fill_state_dict
    from safevla_amd import ops
    from safevla_amd.il import EarlyFusionCnnTransformer, EarlyFusionCnnTransformerAgent, ILTrainer
    from safevla_amd.model import N_ACTIONS, SafeDinoLLAMATxNavActorCriticSeparate

    lib = _lib.lib()
    Trace.hold = hold
    print(f"# schedule digest of {os.path.relpath(root, HERE)}" + (", every kernel operand held until its configuration ends" if hold else ""))

    def randn(seed, *shape):
        return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)).to(DEV)

    def observations(T, B, dtype, seed=3):
        g = torch.Generator().manual_seed(seed)
        ids = torch.randint(3, 32000, (B, L), generator=g)
        for b in range(B):
            ids[b, L - 2 * (b % 3):] = 0          # padded goals of different lengths
        obs = {"dino_tokens": torch.randn(T, B, 2, 84, 384, generator=g).to(dtype), "goal_token_ids": ids[None].expand(T, B, L).contiguous(),
               "time_step": torch.arange(T)[:, None].expand(T, B).contiguous(), "traj_index": torch.arange(B)[None].expand(T, B).contiguous(),
               "an_object_is_in_hand": torch.randint(0, 2, (T, B, 1), generator=g)}
        pa, mk = torch.randint(0, N_ACTIONS, (T, B), generator=g), torch.ones(T, B, 1)
        return {k: v.to(DEV) for k, v in obs.items()}, pa.to(DEV), mk.to(DEV)

    def three_towers(**kw):
        torch.manual_seed(0)
        m = SafeDinoLLAMATxNavActorCriticSeparate(device=DEV, **kw)
        fill_state_dict(m, seed=7)
        m.sync_weights()
        return m

    def tower_pass(name, m, T=T, train=True, **attrs):
        """forward + backward of the actor tower alone"""
        m.train(train)
        keep = {k: getattr(m, k) for k in attrs}
        for k, v in attrs.items():
            setattr(m, k, v)
        m.zero_grad()
        m._fwd_count = 0
        torch.cuda.empty_cache()
        obs, pa, mk = observations(T, B, m.adt)
        prep = m.prepare(obs, pa, mk)
        dfull = randn(13, T, B, 101) if m.critic_type == "discrete" else None
        with Trace(lib, ops) as tr:
            logits, values, saved = m.run_forward(prep, need_grad=True)
            tr.out(logits, values)
            m.run_backward(prep, saved, randn(11, T, B, N_ACTIONS), randn(12, T, B, 1), dfull)
            a, b = m.arena.tower_ranges[0]
            tr.grad(m.arena.flat_g[a:b])
        tr.line(name)
        for k, v in keep.items():
            setattr(m, k, v)
        return tr

    def acting(name, m, plans, **attrs):
        """three single steps of the three-tower wrapper under no_grad at 4 environments"""
        m.train(True)
        for t in m.towers:
            t.time_step_counter, t._kv, t._fwd_count = 0, None, 0
            for k, v in attrs.items():
                setattr(t, k, v)
        m.enable_acting_graphs(plans, backend="plan")
        torch.cuda.empty_cache()
        obs, pa, mk = observations(3, 4, m.adt, seed=5)
        tr = Trace(lib, ops)
        with torch.no_grad():
            for t in range(3):
                step = ({k: v[t:t + 1] for k, v in obs.items()}, None, pa[t:t + 1], mk[t:t + 1])
                if plans:
                    out, _ = m(*step)
                else:
                    with tr:
                        out, _ = m(*step)
                tr.out(out.distributions.logits, out.values, out.c_values)
        if plans:      # the recording step and two grouped replays: the digest is over the recorded call lists
            st = next(iter(m._acting_graphs.values()))
            tr.calls = [c for p in st.plans for c in p.calls]
        tr.line(name)
        m.enable_acting_graphs(False)

    def il(version, agent_step):
        torch.manual_seed(0)
        m = EarlyFusionCnnTransformer.build_model(version, device=DEV)
        fill_state_dict(m, seed=17, share_t5=False)
        m.sync_weights()
        g = torch.Generator().manual_seed(21)
        Bi, Ti, C = 2, 4, m.dino_dim
        batch = {"raw_navigation_camera": torch.randn(Bi, Ti, C, 7, 12, generator=g), "raw_manipulation_camera": torch.randn(Bi, Ti, C, 7, 12, generator=g),
                 "time_ids": torch.arange(Ti)[None].expand(Bi, Ti).contiguous(), "an_object_is_in_hand": torch.randint(0, 2, (Bi, Ti), generator=g),
                 "actions": torch.randint(0, N_ACTIONS, (Bi, Ti), generator=g), "last_actions": torch.randint(0, N_ACTIONS, (Bi, Ti), generator=g)}
        batch = {k: v.to(DEV) for k, v in batch.items()}
        batch["goals"] = dict(input_ids=torch.tensor([[917, 4033, 88, 21, 1], [55, 1, 0, 0, 0]], device=DEV),
                              attention_mask=torch.tensor([[1, 1, 1, 1, 1], [1, 1, 0, 0, 0]], device=DEV))
        torch.cuda.empty_cache()
        with Trace(lib, ops) as tr:
            info = ILTrainer(m).training_step(batch)
            tr.out(torch.tensor([info["loss"]], dtype=torch.float64))
            tr.grad(m.arena.flat_g)
        tr.line(f"il {version} training_step")
        if agent_step:
            agent = EarlyFusionCnnTransformerAgent(m, DEV)
            rs = np.random.RandomState(8)
            frame = {"raw_navigation_camera": rs.standard_normal((C, 7, 12)).astype(np.float32),
                     "raw_manipulation_camera": rs.standard_normal((C, 7, 12)).astype(np.float32), "an_object_is_in_hand": [1]}
            with Trace(lib, ops) as tr:
                _, probs = agent.get_action(frame, dict(input_ids=np.array([[917, 4033, 88, 21, 1]]), attention_mask=np.ones((1, 5), np.int64)))
                tr.out(probs)
            tr.line(f"il {version} get_action")

    m = three_towers()
    first = tower_pass("tower train defaults", m)
    if dump_grad:
        os.makedirs(os.path.dirname(os.path.abspath(dump_grad)), exist_ok=True)
        np.save(dump_grad, first.grads)
    tower_pass("tower absorb_last=False", m, absorb_last=False)
    tower_pass("tower prune_last=False", m, prune_last=False)
    tower_pass("tower fp8_attention", m, fp8_attention=True)
    tower_pass("tower eval", m, train=False)
    tower_pass("tower T=1 need_grad", m, T=1)
    acting("wrapper eager fused", m, False)
    acting("wrapper eager rms/t5 two-launch", m, False, rms_fused=False, t5_fused=False)
    for t in m.towers:
        t.rms_fused, t.t5_fused = True, None
    acting("wrapper acting plans", m, True)
    del m
    m = three_towers(precision="fp32")
    tower_pass("tower fp32", m)
    tower_pass("tower fp32 prune_last=False", m, prune_last=False)
    del m
    for critic in ("mlp", "discrete"):
        m = three_towers(critic_type=critic)
        tower_pass(f"tower critic {critic}", m)
        del m
    il("small_3", True)
    il("base_6", False)


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--root", default=HERE, help="checkout whose safevla_amd/ package runs the configurations (default: this one)")
    ap.add_argument("--dump-grad", default=None, help="write the first configuration's gradient range to this .npy file")
    ap.add_argument("--hold", action="store_true", help="keep every kernel operand alive until its configuration ends: the pointer digest then shows the wiring alone")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    root = os.path.abspath(a.root)
    if root != HERE and not a.child:      # another checkout's package: a fresh interpreter that never imported this tree's
        cmd = [sys.executable, os.path.abspath(__file__), "--root", root, "--child"] + (["--hold"] if a.hold else []) + (["--dump-grad", a.dump_grad] if a.dump_grad else [])
        sys.exit(subprocess.run(cmd).returncode)
    run(root, a.dump_grad, a.hold)


if __name__ == "__main__":
    main()
