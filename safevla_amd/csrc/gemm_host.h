// Host side of the bf16 GEMM entry points (include/svla.h: svla_gemm_nt_bf16 / svla_gemm_tn_f32acc, defined in gemm.hip): WHICH kernel carries a problem, and
// with what grid, as a pure function of (problem, knobs, CU count).  Nothing of HIP is included: a plain C++17 host compiler compiles this file, and
// svla_gemm_nt_plan / svla_gemm_tn_plan return its answers on a machine without a GPU (tests/test_gemm_plan_cpu.py pins them).  The entry points check their
// arguments, ask nt_plan / tn_plan once and launch what the plan says; the kernel name in the plan is the one string both the log and the launch use.
#pragma once
#include <cstdio>
#include <cstdlib>

enum { ACT_NONE = 0, ACT_RELU = 1, ACT_GELU = 2 };
// bits of GemmKnobs::dbg (svla_gemm_force_small_tile(10 + bits)).  The timing-only ones are read by the kernels out of their argument structs:
enum {
    GEMM_DBG_NO_STORES = 1, GEMM_DBG_NO_EPILOGUE = 2,       // NT 256-tile kernels: no C stores / no epilogue
    GEMM_DBG_PHASE_CYCLES = 4, GEMM_DBG_TN_NT_LOADS = 16,   // gemm_tn8p only: shader cycles per phase instead of the gradient / nt loads
    GEMM_DBG_NT_CYCLES = 16, GEMM_DBG_KTILE_CYCLES = 4096,  // gemm_nt8p only: main-loop and epilogue cycles / cycles by K-tile position into the first floats of C
    GEMM_DBG_L2_OPERANDS = 8, GEMM_DBG_NO_DMA = 32,         // 8-phase kernels: re-read the first operand tile (served by the L2) / no operand DMA at all
    GEMM_DBG_DMA_ONLY = 64,                                 // 256-tile kernels: operand DMA stream + barriers alone
    // and the ones the dispatch reads (A/B comparisons, tools/ab_*.py):
    GEMM_DBG_2BUF = 128, GEMM_DBG_8P = 256,                 // the 2-buffer 256-tile kernels (gemm_nt256k64 / gemm_tn256) / the 8-phase ones (chosen anyway)
    GEMM_DBG_ASM_OFF = 8192, GEMM_DBG_NT_OS_OFF = 16384,    // every assembly kernel off / the output-stationary NT ones off
};
// The test hook and the environment thresholds.  force = 0 / 1 / 2: normal dispatch / the 128-tile kernels / the 256-tile and assembly kernels wherever their
// shape constraints hold.  svla_gemm_force_small_tile(on) fills force (on < 10) or dbg (on - 10), never both.
struct GemmKnobs {
    int force = 0, dbg = 0;
    int nt_as_min_panels = 8;       // SVLA_NT_AS_MIN_PANELS: floor of the mid-M launch in 256-row panels (sweeps of tools/ab_midm.py; the cost model decides above it)
    int nt256_min_tiles = 160;      // SVLA_NT256_MIN_TILES: fewest 256x256 tiles for which a 256-tile kernel is chosen over the 128-tile one (tools/acting_force_probe.py)
};
inline GemmKnobs gemm_knobs_from_env() {
    const char *panels = getenv("SVLA_NT_AS_MIN_PANELS"), *tiles = getenv("SVLA_NT256_MIN_TILES");
    return GemmKnobs{0, 0, panels ? atoi(panels) : 8, tiles ? atoi(tiles) : 160};
}
inline void gemm_knobs_set(GemmKnobs& k, int on) { k.force = on >= 10 ? 0 : on; k.dbg = on >= 10 ? on - 10 : 0; }
typedef int (*GemmHas)(const char* name);      // is this assembly kernel in the code object?  (the library: svla_asm_has)
inline const char* gemm_asm_variant(const char* name, [[maybe_unused]] const char* env) {
#ifdef SVLA_ASM_DEBUG      // instrumented builds of tools/ only (SVLA_EXTRA_FLAGS=-DSVLA_ASM_DEBUG): <kernel>_<$env> (tools/time_nt_as.py, tools/var_nt_os.py)
    static char buf[96];
    if (name && getenv(env)) { snprintf(buf, sizeof(buf), "%s_%s", name, getenv(env)); return buf; }
#endif
    return name;
}

// ================================================================================================= NT: C = epi(alpha A B^T)
// What the choice depends on, and nothing else (no pointers: has-bias, not the bias)
struct NtProblem {
    int M, N, K, act;
    bool out_f32, alpha_one, bias, residual, relu_mask, bits_in, bits_out;      // bits_out: the ReLU sign-bit output; bits_in: the ReLU mask given as such bits
    bool drop; int row_mult;                                                    // train-mode dropout and its counter's row stride
};
enum NtPath { NT_AS = 0, NT_OS = 1, NT_8P = 2, NT_2BUF = 3, NT_128 = 4 };      // A-stationary asm, output-stationary asm, 8-phase, 2-buffer, 128-tile
// kernel: what gemm_log records and what is launched; main_rows / tail_rows: rows of the main launch / the M % 256 rows behind an assembly launch, which run on the
// 128-tile kernel; nr, flags, cmask (A-stationary only): columns per n-range, 1 = the mid-M launch, phase mask; log_extra: bytes per output row beyond the A and C rows
// (residual 2 N, sign bits N / 8, bf16 mask 2 N); log_joinable false: remembered by name only (128-tile dispatches also run the unlogged tails: no join by index)
struct NtPlan { NtPath path; const char* kernel; int main_rows, tail_rows, grid_x, grid_y, nr, flags, cmask, log_extra; bool log_joinable; };

// ---- A-stationary assembly kernels (asmgen/nt_as_gen.py): K = 512 or 384, bf16 output, no residual, full 256-row panels.  One row per flavour:
// K = 512: bias / bias + ReLU + sign bits [+ dropout] / the input gradient under the sign bits (+ dropout scale as alpha: no bias);
// K = 384 (the ViT-S / DINOv2-feature width): bias (qkv), bias + ReLU + sign bits (the policy's visual compressor), bias + erf-GELU (fc1)
struct NtAsFlavour { int K, act; bool bits_in, bits_out, drop, bias_ok, any_alpha; const char* name; };
constexpr NtAsFlavour NT_AS_FLAVOURS[] = {
    {512, ACT_NONE, false, false, false, true,  false, "svla_nt_as_f0"},
    {512, ACT_RELU, false, true,  false, true,  false, "svla_nt_as_f1"},
    {512, ACT_RELU, false, true,  true,  true,  false, "svla_nt_as_f1d"},
    {512, ACT_NONE, true,  false, false, false, true,  "svla_nt_as_f3"},
    {384, ACT_NONE, false, false, false, true,  false, "svla_nt_as_k384_f0"},
    {384, ACT_RELU, false, true,  false, true,  false, "svla_nt_as_k384_f1"},
    {384, ACT_GELU, false, false, false, true,  false, "svla_nt_as_k384_f2"},
};
inline bool nt_as_plan(const NtProblem& q, const GemmKnobs& kn, int n_cu, GemmHas has, NtPlan& p) {
    if (q.out_f32 || (q.N % 128) || q.N > 4096 || q.N < 128 || (kn.dbg & GEMM_DBG_ASM_OFF) || kn.force == 1 || q.relu_mask || q.residual) return false;
    const int npanels = q.M / 256;
    if ((npanels < kn.nt_as_min_panels && kn.force != 2) || npanels < 1) return false;
    const char* name = nullptr;
    for (const NtAsFlavour& f : NT_AS_FLAVOURS)
        if (f.K == q.K && f.act == q.act && f.bits_in == q.bits_in && f.bits_out == q.bits_out && f.drop == q.drop && (f.bias_ok || !q.bias) && (f.any_alpha || q.alpha_one)) name = f.name;
    name = gemm_asm_variant(name, "SVLA_NT_AS_VARIANT");
    if (!name || !has(name)) return false;
    // the dropout counter of the assembly kernel is 32 bits wide: element pairs of the whole logical tensor must fit
    if (q.drop && (unsigned long long)q.M * (unsigned long long)q.row_mult * (unsigned long long)q.N / 2 >= 0xffffffffull) return false;
    // the sign-bit offset of a panel (panel * N * 32 bytes) is 32-bit scalar arithmetic in the kernel (asmgen/nt_as_gen.py bits_srd)
    if ((q.bits_in || q.bits_out) && (unsigned long long)q.M * (unsigned long long)q.N / 8 >= 0xffffffffull) return false;
    int cmask = 0;      // phase spread over workgroups: (workgroup & cmask) < NS/4 extra steps, cmask + 1 = the largest power of two <= NS/4
    while ((cmask + 1) * 2 <= q.N / 256) cmask = cmask * 2 + 1;
    // >= 2 panels per CU: the row-streaming launch (one persistent workgroup per CU, phases); fewer: the mid-M launch below
    int grid_x = npanels < n_cu ? npanels : n_cu, grid_y = 1, nr = q.N, flags = 0;
    if (npanels < 2 * n_cu) {
        // mid-M (an acting step's 45 panels, the 233 of the batch-256 probe, the ViT's 216): too few panels to give every CU two sweeps.  The grid becomes
        // (panel slots) x (n-ranges): workgroup (x, y) sweeps columns [y nr, (y + 1) nr) of panels x, x + slots, ...; no phases (a workgroup that holds one
        // panel has nothing to de-phase).  nsplit minimises rounds * (steps per sweep + ~2.5 steps of prologue / drain) over the divisors of N / 128.
        // Cost model, calibrated on profiles/r05_midm_sweep.txt (asm side within ~10 % of the measurements): one n-step (64 columns of a 256-row panel) takes
        // ~2.76 us * K/512; a workgroup pays ~5 steps per panel it loads (the fragment-shaped A gather runs at ~13 B/clk) + its sweep; the tile kernels take
        // ~(6.2 + 11.6 K/512) us per round of 256 tiles.  The assembly launch is taken when it is at least 5 % ahead (a ragged M adds the tail launch).
        const int ns = q.N / 64;
        double best = 1e30;
        int best_d = 1, best_slots = grid_x;
        for (int d = 1; d <= q.N / 128; ++d) {
            if ((q.N / 128) % d) continue;
            int slots = npanels * d <= n_cu ? npanels : n_cu / d;
            if (slots < 1) break;
            const int rounds = (npanels + slots - 1) / slots;
            const double cost = rounds * ((double)ns / d + 5.0);
            if (cost < best - 1e-9) { best = cost; best_d = d; best_slots = slots; }
        }
        if (kn.force != 2) {
            const long tiles = (long)((q.M + 255) / 256) * ((q.N + 255) / 256);
            const double hip = (double)((tiles + n_cu - 1) / n_cu) * (6.2 + 11.6 * q.K / 512.0);
            const double asm_cost = best * 2.76 * q.K / 512.0 + ((q.M % 256) ? 15.0 : 0.0);      // a ragged M: + the tail launch behind it (~15 us in a stream, r05_vit_kernel_stats.txt)
            if (asm_cost > 0.95 * hip) return false;
        }
        grid_x = best_slots; grid_y = best_d; nr = q.N / best_d; flags = 1; cmask = 0;
    }
    p = NtPlan{NT_AS, name, npanels * 256, q.M - npanels * 256, grid_x, grid_y, nr, flags, cmask, (q.bits_in || q.bits_out) ? q.N / 8 : 0, true};
    return true;
}
// ---- output-stationary assembly kernels (asmgen/nt_os_gen.py): K > 512 (or K = 512 with a residual), bias / residual epilogues without dropout, N % 256 == 0,
// K % 128 == 0, full 256-row tiles.  GEMM_DBG_NT_OS_OFF = off (A/B: tools/ab_nt_os.py).
inline bool nt_os_plan(const NtProblem& q, const GemmKnobs& kn, int n_cu, GemmHas has, NtPlan& p) {
    if (q.out_f32 || (q.N % 256) || q.N > 4096 || (q.K % 128) || q.K < 384 || (kn.dbg & (GEMM_DBG_ASM_OFF | GEMM_DBG_NT_OS_OFF)) || kn.force == 1) return false;
    if (q.relu_mask || q.bits_in || q.bits_out || q.drop || q.act != ACT_NONE || !q.alpha_one) return false;
    const int mtiles = q.M / 256, ntiles = mtiles * (q.N / 256);
    if ((ntiles < 1024 && kn.force != 2) || mtiles < 1) return false;      // fewer than four tiles per CU: the two-workgroup-per-CU tile kernel balances better
    const char* name = gemm_asm_variant(q.bias ? (q.residual ? "svla_nt_os_br" : "svla_nt_os_b") : (q.residual ? "svla_nt_os_r" : "svla_nt_os_p"), "SVLA_NT_OS_VARIANT");
    if (!has(name)) return false;
    p = NtPlan{NT_OS, name, mtiles * 256, q.M - mtiles * 256, ntiles < n_cu ? ntiles : n_cu, 1, 0, 0, 0, q.residual ? 2 * q.N : 0, true};
    return true;
}
// The assembly families first (K = 512 / 384 row-streaming GEMMs, then K >= 384 without dropout), then the HIP kernels.  Among the 256-tile ones (measured,
// tools/ab_gemm.py, profiles/r03_nt_ab.txt): with the trimmed epilogue the 8-phase kernel wins on every shape of the update (+2 ... +7 %); the 2-buffer kernel
// stays for N > 8192 (the LDS bias table) and as the A/B partner (GEMM_DBG_2BUF).
inline NtPlan nt_plan(const NtProblem& q, const GemmKnobs& kn, int n_cu, GemmHas has) {
    NtPlan p{};
    if (nt_as_plan(q, kn, n_cu, has, p) || nt_os_plan(q, kn, n_cu, has, p)) return p;
    const long tiles = (long)((q.M + 255) / 256) * ((q.N + 255) / 256);
    // N % 256 == 128 with N >= 384 (the ViT-S widths 384 and 1152): the last n-tile is a half tile (75 % / 90 % of the MFMA work useful) --
    // still well ahead of the 128-tile kernel
    if (!q.out_f32 && ((q.N % 256) == 0 || ((q.N % 128) == 0 && q.N >= 384)) && (q.K % 64) == 0 && q.K >= 128 && (tiles >= kn.nt256_min_tiles || kn.force == 2) && kn.force != 1) {
        const bool p8 = q.N <= 8192 && !(kn.dbg & GEMM_DBG_2BUF);
        int grid = n_cu / 8 * 8 < 8 ? 8 : n_cu / 8 * 8;      // persistent: one 512-thread workgroup (160 KiB LDS) per CU, in whole groups of 8, no more than there are tiles
        while (grid > 8 && grid > tiles) grid -= 8;
        const int extra = (q.residual ? 2 * q.N : 0) + ((q.bits_in || q.bits_out) ? q.N / 8 : 0) + (q.relu_mask ? 2 * q.N : 0);
        return NtPlan{p8 ? NT_8P : NT_2BUF, p8 ? "gemm_nt8p_bf16_kernel" : "gemm_nt256k64_bf16_kernel", q.M, 0, grid, 1, 0, 0, 0, extra, true};
    }
    return NtPlan{NT_128, "gemm_nt_bf16_kernel", q.M, 0, (q.M + 127) / 128 * (q.N / 128), 1, 0, 0, 0, 0, false};      // one workgroup per 128 x 128 output tile
}

// ================================================================================================= TN: dW += dY^T X
constexpr int TN_GROUP_ROWS = 64;      // reduction rows per stage of the 256-tile TN kernels (TN256_ROWS of gemm.hip)
enum TnPath { TN_OS = 0, TN_8P = 1, TN_2BUF = 2, TN_128 = 3 };      // svla_tn_os, gemm_tn8p, gemm_tn256, gemm_tn_bf16_kernel
// One launch: every workgroup reduces chunk_rows rows of one output tile (rows == 0: no such part).  colsum: the 128-tile kernel has no fused bias gradient,
// svla_colsum_bf16 runs in front; recorded: gemm_log / svla_gemm_last_kernel see the launch (the 2-buffer and the 128-tile kernel: not)
struct TnPart { TnPath path; const char* kernel; int rows, chunk_rows, grid; bool colsum, recorded; };
struct TnPlan { TnPart main, tail; };      // tail: the ragged rows of a forced (force == 2) 256-tile call, on the 128-tile kernel
inline TnPart tn_part(int M, int N, int K, bool has_db, int force, int dbg, bool det_on, GemmHas has) {
    // measured (r03): at 16 k rows the 256-tile kernel is 1.0x (512 x 512) to 2.0x (1536 x 512) the 128-tile one, at 8 k rows 0.7x / 1.2-1.9x
    if ((N % 256) == 0 && (K % 256) == 0 && (M % TN_GROUP_ROWS) == 0 && (M >= 16384 || (M >= 8192 && (long)N * K >= 1024L * 512) || force == 2) && force != 1) {
        const int ntile256 = (N / 256) * (K / 256);
        const int chunks = 256 / ntile256 < 1 ? 1 : 256 / ntile256;                                  // <= one workgroup per CU (no second dispatch wave)
        const int chunk_rows = ((M + chunks - 1) / chunks + TN_GROUP_ROWS - 1) / TN_GROUP_ROWS * TN_GROUP_ROWS, grid = ntile256 * ((M + chunk_rows - 1) / chunk_rows);
        // output-stationary assembly kernel (asmgen/tn_os_gen.py): 4 waves x 128 x 128 accumulators, 4-slot LDS-DMA ring
        if (!(dbg & (GEMM_DBG_2BUF | GEMM_DBG_ASM_OFF)) && !det_on && has("svla_tn_os")) return TnPart{TN_OS, "svla_tn_os", M, chunk_rows, grid, false, true};
        if (!(dbg & GEMM_DBG_2BUF)) return TnPart{TN_8P, "gemm_tn8p_bf16_kernel", M, chunk_rows, grid, false, true};
        return TnPart{TN_2BUF, "gemm_tn256_bf16_kernel", M, chunk_rows, grid, false, false};
    }
    const int ntile = (N / 128) * (K / 128), chunks = (2048 + ntile - 1) / ntile;      // aim for ~2048 workgroups; chunk is a multiple of the 64-row reduction tile
    int chunk_rows = ((M + chunks - 1) / chunks + 63) / 64 * 64;
    if (chunk_rows < 256) chunk_rows = 256;
    return TnPart{TN_128, "gemm_tn_bf16_kernel", M, chunk_rows, ntile * ((M + chunk_rows - 1) / chunk_rows), has_db, false};
}
inline TnPlan tn_plan(int M, int N, int K, bool has_db, const GemmKnobs& kn, bool det_on, GemmHas has) {
    // forced big-tile mode (tests: the reference goldens through the kernels that carry the update): whole 64-row groups on the 256-tile kernel, the ragged tail on the small one
    const bool split = kn.force == 2 && (N % 256) == 0 && (K % 256) == 0 && M >= 2 * TN_GROUP_ROWS && (M % TN_GROUP_ROWS) != 0;
    const int mb = split ? M / TN_GROUP_ROWS * TN_GROUP_ROWS : M;
    return TnPlan{tn_part(mb, N, K, has_db, kn.force, kn.dbg, det_on, has), split ? tn_part(M - mb, N, K, has_db, 1, kn.dbg, det_on, has) : TnPart{}};
}
