// tests/test_gemm_plan_cpu.py: nt_plan / tn_plan (safevla_amd/csrc/gemm_host.h) when an assembly kernel is missing from the code object -- the entry points of the
// library count every kernel as present, so the predicate is exercised here.  Plain C++17, no HIP.  argv[1]: the missing kernel, "*" = all, "-" = none.
#include <cstring>
#include "gemm_host.h"

static const char* g_missing = "-";
static int has(const char* name) { return strcmp(g_missing, "*") != 0 && strcmp(g_missing, name) != 0; }

static void nt(int M, int N, int K, bool bias, bool residual) {
    const NtProblem q{M, N, K, ACT_NONE, false, true, bias, residual, false, false, false, false, 1};
    const NtPlan p = nt_plan(q, GemmKnobs{}, 256, has);
    printf("%s %d %d %d %dx%d %d %d %d %d %d\n", p.kernel, (int)p.path, p.main_rows, p.tail_rows, p.grid_x, p.grid_y, p.nr, p.flags, p.cmask, p.log_extra, (int)p.log_joinable);
}

int main(int argc, char** argv) {
    if (argc > 1) g_missing = argv[1];
    nt(741376, 512, 512, true, false);
    nt(741476, 512, 2048, true, true);
    const TnPlan t = tn_plan(741376, 512, 512, true, GemmKnobs{}, false, has);
    printf("%s %d %d %d %d %d %d\n", t.main.kernel, (int)t.main.path, t.main.rows, t.main.chunk_rows, t.main.grid, (int)t.main.colsum, (int)t.main.recorded);
    return 0;
}
