// Tower-grouped launches (round 6) and THE launch path of csrc/: every kernel launch, memset and copy of the library goes through this file.
//
// The three towers of the actor-critic (actor, reward critic, cost critic: separate_actor_critic.py:27-37) execute the SAME kernel
// sequence on the same shapes with different weights.  At an acting step every one of those kernels is small (64 ... 11 584 rows): three
// streams of ~100 dependent launches each, where a chip-filling kernel of one tower holds up the other two (profiles/r05_policy_step_kernel_stats.txt).
// With a capture open (svla_group_begin), a launch site that goes through SVLA_LAUNCH / SVLA_LAUNCH_TWIN does not launch: it stores the kernel's arguments.
// svla_group_end then issues, for launch j of the call, ONE grid whose blockIdx.z selects the member's argument block -- three times the
// workgroups per dispatch, one dependency chain instead of three.  Anything that is not identical across the members (kernel, grid, block,
// LDS bytes) falls back to one launch per member, in member order, on the same stream: always correct, only slower.
//
// What a capture decides is host logic without HIP, in launch_group.h (the rules are written out there): a member's launches keep the order of its calls --
// svla_launch, svla_asm_launch2, svla_memset_async and svla_memcpy_async issue the member's pending launches before their own, as does a deferral into a full queue --
// and a capture has ONE stream, that of its first launch; a site or an end that names another is SVLA_EINVAL.  This file is the HIP side: the opt-in for dynamic
// LDS, the launchers and the grouped twin.
//
// A kernel takes part by being written as  __device__ body(args...)  +  __global__ kernel(args...) { body(args...); }  (the single-launch kernel keeps
// its name, signature and code); its grouped twin is svla_grouped<&body, ...>, generated here.
#pragma once
#include <hip/hip_runtime.h>
#include <string.h>
#include <atomic>
#include <mutex>
#include <utility>
#include "launch_group.h"

template <typename... Ts> struct ArgPack;
template <> struct ArgPack<> {};
template <typename T, typename... Ts> struct ArgPack<T, Ts...> { T head; ArgPack<Ts...> tail; };

template <size_t I, typename T, typename... Ts>
__host__ __device__ __forceinline__ const auto& pack_get(const ArgPack<T, Ts...>& p) {
    if constexpr (I == 0) return p.head;
    else return pack_get<I - 1>(p.tail);
}
template <typename T, typename... Ts> inline ArgPack<T, Ts...> pack_make(const T& h, const Ts&... t) {
    if constexpr (sizeof...(Ts) == 0) return ArgPack<T>{h, ArgPack<>{}};
    else return ArgPack<T, Ts...>{h, pack_make<Ts...>(t...)};
}

template <typename P> struct GroupedArgs { P a[SVLA_MAXG]; };

template <auto Body, typename... Ts, size_t... I>
__device__ __forceinline__ void svla_call_body(const ArgPack<Ts...>& p, std::index_sequence<I...>) { Body(pack_get<I>(p)...); }

// the grouped twin: blockIdx.z = member (the argument block is read from the kernarg segment at a wave-uniform offset)
template <auto Body, int MAXT, int MINB, typename... Ts>
__global__ void __launch_bounds__(MAXT, MINB) svla_grouped(GroupedArgs<ArgPack<Ts...>> g) {
    svla_call_body<Body, Ts...>(g.a[blockIdx.z], std::index_sequence_for<Ts...>{});
}

GroupCapture* svla_group_capture();    // misc.hip: this thread's open capture, or nullptr
int svla_group_size();                 // members of the open capture (1: none) -- dispatchers size persistent grids / choose kernels for the GROUP's work
int svla_cu_count();                   // misc.hip: compute units of the current device, cached (0: the query failed); never refuses inside a stream capture

static inline int svla_launch_status() { return (int)hipGetLastError(); }
static inline dim3 svla_dim3(LaunchDim d) { return dim3(d.x, d.y, d.z); }

// Dynamic LDS beyond 64 KiB has to be asked for, per kernel: raises Kern's limit when `bytes` exceeds what this process has already cleared for it (a high-water
// mark that starts at 0: sizes below the default limit are asked for too, once, rather than trusting where exactly that default lies).  THE one place that
// does it -- every launch path below calls it, so no launch site carries a flag of its own -- and so the one place to change if the state ever has to be kept
// per device (today: once per kernel per process).  Returns the HIP error.
inline std::mutex& svla_lds_optin_mutex() { static std::mutex m; return m; }
template <auto Kern> inline int svla_lds_optin(size_t bytes) {
    static std::atomic<unsigned> cleared{0};
    if (bytes <= cleared.load(std::memory_order_acquire)) return 0;
    std::lock_guard<std::mutex> lock(svla_lds_optin_mutex());      // first launches only: two threads must not set the limit in one order and record it in the other
    if (bytes <= cleared.load(std::memory_order_relaxed)) return 0;
    const hipError_t e = hipFuncSetAttribute((const void*)Kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
    if (e != hipSuccess) return (int)e;
    cleared.store((unsigned)bytes, std::memory_order_release);
    return 0;
}
// opt in when needed, launch, report: what a flush function and svla_launch end in.  Asks no capture.
template <auto Kern, typename... As> inline int svla_issue(dim3 grid, dim3 block, size_t lds, hipStream_t s, const As&... a) {
    if (const int rc = svla_lds_optin<Kern>(lds)) return rc;
    hipLaunchKernelGGL(Kern, grid, block, lds, s, a...);
    return svla_launch_status();
}
// Whatever is issued at once -- a kernel without a grouped twin, an assembly kernel, a memset, a copy -- asks the thread's open capture first (launch_group.h:
// group_direct): the member's pending launches go ahead of it, and another stream than the capture's is refused.  One thread-local read when none is open.
inline int svla_direct(hipStream_t s) {
    GroupCapture* gc = svla_group_capture();
    return gc ? group_direct(*gc, (void*)s) : 0;
}
// THE launch of a kernel without a grouped twin.  (Kern may be a template-id with commas: this is a function template, not a macro.)
template <auto Kern, typename... As> inline int svla_launch(dim3 grid, dim3 block, size_t lds, hipStream_t s, const As&... a) {
    if (const int rc = svla_direct(s)) return rc;
    return svla_issue<Kern>(grid, block, lds, s, a...);
}
inline int svla_memset_async(void* p, int value, size_t bytes, hipStream_t s) {
    if (const int rc = svla_direct(s)) return rc;
    return (int)hipMemsetAsync(p, value, bytes, s);
}
inline int svla_memcpy_async(void* dst, const void* src, size_t bytes, hipMemcpyKind kind, hipStream_t s) {
    if (const int rc = svla_direct(s)) return rc;
    return (int)hipMemcpyAsync(dst, src, bytes, kind, s);
}

// issue n >= 1 members' argument blocks as ONE grid of the grouped twin (grid.z = n)
template <auto Body, int MAXT, int MINB, typename... Ts>
inline int svla_twin_launch(const DeferredLaunch* const* m, int n, void* s) {
    using Pack = ArgPack<Ts...>;
    GroupedArgs<Pack> g;
    for (int i = 0; i < SVLA_MAXG; ++i) memcpy((void*)&g.a[i], m[i < n ? i : 0]->args, sizeof(Pack));
    if (const int rc = svla_lds_optin<svla_grouped<Body, MAXT, MINB, Ts...>>(m[0]->smem)) return rc;      // the twin is a kernel of its own: cleared apart from the single-launch kernel
    dim3 grid = svla_dim3(m[0]->grid);
    grid.z = (unsigned)n;
    hipLaunchKernelGGL((svla_grouped<Body, MAXT, MINB, Ts...>), grid, svla_dim3(m[0]->block), m[0]->smem, (hipStream_t)s, g);
    return svla_launch_status();
}
// A deferral site: inside a capture the launch is stored in the member's queue (0, or why it was refused), outside it is issued through the same flush as a
// group of one.  `flush` is all that tells a kernel with a single-launch form from one without.
typedef int (*SvlaFlush)(const DeferredLaunch* const*, int, void*);
template <typename... Ts> inline int svla_defer_or_issue(SvlaFlush flush, dim3 grid, dim3 block, size_t smem, hipStream_t s, const Ts&... a) {
    static_assert(sizeof(ArgPack<Ts...>) <= SVLA_DEFER_ARG_BYTES, "deferred argument block too small");
    GroupCapture* gc = svla_group_capture();
    DeferredLaunch now, *d = &now;
    int rc = 0;
    if (gc && !(d = group_defer(*gc, (void*)s, &rc))) return rc;
    d->flush = flush;
    d->grid = LaunchDim{grid.x, grid.y, grid.z}; d->block = LaunchDim{block.x, block.y, block.z}; d->smem = (unsigned)smem;
    const ArgPack<Ts...> p = pack_make<Ts...>(a...);
    memcpy(d->args, (const void*)&p, sizeof(p));
    return gc ? 0 : flush(&d, 1, (void*)s);
}

// A kernel with a same-named single-launch __global__ (Kern) and a grouped twin generated from its body
template <auto Kern, auto Body, int MAXT, int MINB> struct Launch;
template <typename... Ts, void (*Kern)(Ts...), void (*Body)(Ts...), int MAXT, int MINB>
struct Launch<Kern, Body, MAXT, MINB> {
    using Pack = ArgPack<Ts...>;
    template <size_t... I>
    static int single(const DeferredLaunch& d, void* s, std::index_sequence<I...>) {
        Pack p;
        memcpy((void*)&p, d.args, sizeof(Pack));
        return svla_issue<Kern>(svla_dim3(d.grid), svla_dim3(d.block), d.smem, (hipStream_t)s, pack_get<I>(p)...);
    }
    static int flush(const DeferredLaunch* const* m, int n, void* s) {
        if (n == 1) return single(*m[0], s, std::index_sequence_for<Ts...>{});
        return svla_twin_launch<Body, MAXT, MINB, Ts...>(m, n, s);
    }
    static int go(dim3 grid, dim3 block, size_t smem, hipStream_t s, Ts... a) { return svla_defer_or_issue<Ts...>(&flush, grid, block, smem, s, a...); }
};
// A kernel that exists ONLY as the grouped form: a single launch is a group of one (grid.z = 1).  For the attention forward kernels: their bodies inlined into a
// plain same-named __global__ compiled worse than the original kernels did (attn_fwd_persist_kernel<12>: 109 spilled VGPRs against 6, 2.99 -> 5.97 ms per launch
// in the update -- caught by an A/B against the round-5 tree on one box), while the same body inside svla_grouped<> compiles like the original
template <auto Body, int MAXT, int MINB> struct LaunchTwin;
template <typename... Ts, void (*Body)(Ts...), int MAXT, int MINB>
struct LaunchTwin<Body, MAXT, MINB> {
    static int flush(const DeferredLaunch* const* m, int n, void* s) { return svla_twin_launch<Body, MAXT, MINB, Ts...>(m, n, s); }
    static int go(dim3 grid, dim3 block, size_t smem, hipStream_t s, Ts... a) { return svla_defer_or_issue<Ts...>(&flush, grid, block, smem, s, a...); }
};
// kern / body may be template-ids with commas: pass them in parentheses
#define SVLA_LAUNCH(kern, body, maxt, minb, grid, block, smem, stream, ...) \
    Launch<&kern, &body, maxt, minb>::go(grid, block, smem, stream, __VA_ARGS__)
#define SVLA_LAUNCH_TWIN(body, maxt, minb, grid, block, smem, stream, ...) \
    LaunchTwin<&body, maxt, minb>::go(grid, block, smem, stream, __VA_ARGS__)
