"""The plan query and the launch read ONE plan: after a small GEMM under each dispatch hook, svla_gemm_last_kernel shows the kernel and the rows of the main
launch that ops.gemm_nt_plan / ops.gemm_tn_plan return for the same arguments, hook and the device's CU count.  (What the plans must be: test_gemm_plan_cpu.py;
that every path computes the right thing: test_gemm_ld_gpu.py, whose shapes and hooks these are.)"""
import pytest
import torch

from test_gemm_ld_gpu import BF16, DEV, F32, MARKER, drnd, hooked, launch_marker, ops      # noqa: F401  (ops: fixture)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def n_cu():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _nt(ops, n_cu, hook, M, N, K, want_kernel):
    A, B, bias = drnd(M, K, seed=1).to(BF16), drnd(N, K, seed=2, scale=K ** -0.5).to(BF16), drnd(N, seed=3)
    with hooked(hook):
        kernel, plan = ops.gemm_nt_plan(M, N, K, n_cu, bias=True)
        out = ops.gemm_nt(A, B, M, N, K, bias=bias)
        torch.cuda.synchronize()
        assert ops.gemm_last_kernel() == (kernel, (plan[1], N, K))
    assert kernel == want_kernel and plan[1] + plan[2] == M
    assert torch.isfinite(out.float()).all()


@pytest.mark.parametrize("hook,M,want", [("big", 2085, "svla_nt_as_f0"), ("big", 512, "svla_nt_as_f0"), ("big", 100, "gemm_nt8p_bf16_kernel"),
                                         ("small", 2085, "gemm_nt_bf16_kernel"), (None, 2085, "gemm_nt_bf16_kernel")])
def test_nt_launch_follows_the_plan(ops, n_cu, hook, M, want):
    _nt(ops, n_cu, hook, M, 512, 512, want)


@pytest.mark.parametrize("hook,want", [("asm_off", "gemm_nt8p_bf16_kernel"), ("asm_off_2buf", "gemm_nt256k64_bf16_kernel")])
def test_nt_256_tile_launch_follows_the_plan(ops, n_cu, hook, want):
    """the dbg hooks clear the force hook, so the 256-tile kernels are reached by size: 41 x 4 = 164 tiles (test_gemm_ld_gpu.py: test_nt_256_tile_hip_kernels)"""
    _nt(ops, n_cu, hook, 256 * 40 + 77, 1024, 192, want)


@pytest.mark.parametrize("M,want,rows", [(1000, "svla_tn_os+gemm_tn_bf16_kernel", 960), (64, "svla_tn_os", 64)])
def test_tn_launch_follows_the_plan(ops, n_cu, M, want, rows):
    N = K = 512
    dY, X = drnd(M, N, seed=1).to(BF16), drnd(M, K, seed=2).to(BF16)
    dW, db = torch.zeros(N, K, device=DEV, dtype=F32), torch.zeros(N, device=DEV, dtype=F32)
    with hooked("big"):
        kernel, plan = ops.gemm_tn_plan(M, N, K, n_cu, db=True)
        launch_marker(ops)
        ops.gemm_tn_acc(dY, X, dW, M, N, K, db=db)
        torch.cuda.synchronize()
        assert ops.gemm_last_kernel() == (kernel.split("+")[0], (plan[1], N, K)) != MARKER      # the record keeps the main launch
    assert kernel == want and plan[1] == rows and plan[1] + plan[7] == M
    assert torch.isfinite(dW).all() and torch.isfinite(db).all()
