"""The dynamic-LDS opt-in is lazy and per kernel (csrc/launch.h: svla_lds_optin): a kernel that needs more than 64 KiB must work when its launch is the first
thing a process does with it, whatever ran -- or did not run -- before.  Each group below runs in a fresh child process (nothing has cleared any kernel there),
at the smallest size at which the kernel still asks for more than 64 KiB, through the cases of the kernels' own tests: their references, their tolerances.

  attn64    64-wide backward at S = 250 (16 key tiles: 66 KiB and more), one row, one head: the dQ + dK/dV pair, the generic-mask pair, the single-pass kernel
  attn      96-wide backward at S = 129 (12 key tiles: 73 KiB; 8 tiles take 49 KiB), long-window backward at S = 260, fp8 forward + backward at S = 193
            (the backward's 16-tile image is 68 KiB; its 12-tile image 52 KiB)
  gemm_tn   weight gradient at M = 8192 + 40, N = K = 256 under force mode 2 (the ragged split: 256-tile kernel + the 64 KiB small-tile kernel on the last 40
            rows), the 8-phase 256-tile kernel (128 KiB); the split leaves the force mode as it found it
  gemm_nt   M = 256 + 40, N = 256, K = 512 under force modes 1 and 2 (the 128-tile kernel, 66 KiB, as the main launch and as the tail behind an assembly
            launch), the 160 KiB 256-tile flavours behind both launch paths
A C-ABI call that does not return 0 raises in the binding, so every call below is checked for it.

Not yet run on an MI355X: no GPU could be had while this file was written (see the commit message)."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


def _attn64(ops):
    import torch
    import test_kernels_gpu as K

    ops.attn_bwd_two_pass(True)
    try:
        K._attn_case(ops, 1, 250, 1)                                   # attn_bwd_dq_exact / attn_bwd_dkv_exact
    finally:
        ops.attn_bwd_two_pass(False)
    g = torch.Generator().manual_seed(250)
    traj = torch.cumsum((torch.rand(1, 250, generator=g) < 0.05).long(), dim=1) + 3
    K._attn_case(ops, 1, 250, 1, mask_mode=1, traj=traj)               # attn_bwd_dq / attn_bwd_dkv <generic>
    K._attn_case(ops, 1, 250, 1)                                       # attn_bwd_fused_exact


def _attn(ops):
    import test_attn_hd96_gpu as A96
    import test_attn_long_bwd_gpu as AL
    import test_fp8_attention_gpu as F8

    A96.run_case(ops, 129, name="hd96 S=129")
    AL.run_case(ops, 260, seed=260, name="long S=260")
    F8.test_fp8_forward_backward_tolerance_ladder_vs_fp32(ops, 193, 0.0)


def _gemm_tn(ops):
    import torch
    import test_kernels_gpu as K

    M, N, Kd = 8192 + 40, 256, 256
    dY, X = K.bf(K.rnd(M, N, seed=1)), K.bf(K.rnd(M, Kd, seed=2))
    dW = torch.ones(N, Kd, device=K.DEV)
    ops.gemm_force_small_tile(2)
    try:
        ops.gemm_tn_acc(dY.to(K.DEV).bfloat16(), X.to(K.DEV).bfloat16(), dW, M, N, Kd)
        # still mode 2, neither the 1 of the split's second half nor 0: 45 panels x N = 512 go to the assembly kernel only when forced
        A = torch.zeros(11584, 512, device=K.DEV, dtype=torch.bfloat16); B = torch.zeros(512, 512, device=K.DEV, dtype=torch.bfloat16)
        ops.gemm_nt(A, B, 11584, 512, 512, bias=torch.zeros(512, device=K.DEV))
        torch.cuda.synchronize()
        assert ops.gemm_last_kernel()[0] == "svla_nt_as_f0", ops.gemm_last_kernel()
    finally:
        ops.gemm_force_small_tile(0)
    K.close(dW, 1 + dY.double().t() @ X.double(), 2e-4, 2e-4 * (M ** 0.5), "ragged dW")      # = test_gemm_tn's gate
    K.test_gemm_nt_mid_m_cost_model_dispatch(ops)                      # default mode: the kernels the cost model picks
    K.test_gemm_tn(ops, M, N, Kd, 2)                                   # the same split with the fused bias gradient, test_gemm_tn's own checks
    K.test_gemm_tn_assembly_kernel(ops, 512, 512)                      # gemm_tn8p (assembly off)


def _gemm_nt(ops):
    import test_kernels_gpu as K

    K.test_gemm_nt_plain(ops, 256 + 40, 256, 512, 2)                   # assembly panel + gemm_nt_bf16 as the tail launch
    assert ops.gemm_last_kernel() == ("svla_nt_as_f0", (256, 256, 512)), ops.gemm_last_kernel()
    K.test_gemm_nt_plain(ops, 256 + 40, 256, 512, 1)
    assert ops.gemm_last_kernel()[0] == "gemm_nt_bf16_kernel", ops.gemm_last_kernel()
    K.test_gemm_nt_epilogues(ops, 17000, 1024)                         # gemm_nt8p flavours behind SVLA_LAUNCH and behind svla_launch


GROUPS = {"attn64": _attn64, "attn": _attn, "gemm_tn": _gemm_tn, "gemm_nt": _gemm_nt}


@pytest.mark.parametrize("group", sorted(GROUPS))
def test_first_launch_in_a_fresh_process(group):
    r = subprocess.run([sys.executable, os.path.abspath(__file__), group], cwd=os.path.dirname(HERE), capture_output=True, text=True, timeout=600)
    print(r.stdout[-3000:])
    assert r.returncode == 0 and f"ok {group}" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(HERE))
    from safevla_amd import ops as _ops

    GROUPS[sys.argv[1]](_ops)
    import torch

    torch.cuda.synchronize()
    print(f"ok {sys.argv[1]}")
