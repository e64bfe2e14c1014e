// Host logic of a launch-group capture (include/svla.h: svla_group_begin / _member / _end / _stats; csrc/launch.h is the HIP side): the per-member queues of
// deferred launches and WHAT a capture decides -- on a deferral, on a launch that cannot be deferred, on a full queue and at the end.  Nothing of HIP is included:
// a plain C++17 host compiler compiles this file, and a launch is issued only through the `flush` function a deferred launch carries, so
// tests/test_launch_group_cpu.py drives captures with flush functions that record instead of launching.
//
// The rules:
//   order    the launches of ONE member reach the stream in the order its calls made them.  A deferred launch waits for svla_group_end; before a launch
//            that cannot wait (a kernel without a grouped twin, an assembly kernel, a memset, a copy: group_direct) and before a deferral that finds the
//            member's queue full, the member's pending launches are issued singly, in order.  Such a capture is no longer in lockstep: the end issues what is
//            left member by member.  With nothing pending there is nothing to do and lockstep is kept (an assembly main launch followed by its deferred row
//            tail still groups the tail).  Members are independent of each other: nothing orders member 0's launches against member 1's.
//   stream   the first launch made inside a capture, deferred or not, fixes the capture's stream; a launch site or an end that names another one is
//            SVLA_EINVAL (the site neither launches nor defers; the end issues nothing and closes the capture).  An empty capture ends on any stream.
//   stats    every launch that passed a deferral site is counted once: as part of a grouped issue, or as a single one (also when it was issued early).
#pragma once
#include <stddef.h>

#define SVLA_OK 0
#define SVLA_EINVAL (-1)

#define SVLA_MAXG 3             // towers
#define SVLA_MAXQ 8             // launches one member can have pending at a time; one more deferral issues them first (group_defer)
#define SVLA_DEFER_ARG_BYTES 512

struct LaunchDim { unsigned x, y, z; };
struct DeferredLaunch {
    // issues members m[0..n): grouped when n > 1 (the caller has checked that they are identical in everything but the arguments)
    int (*flush)(const DeferredLaunch* const* m, int n, void* stream);
    LaunchDim grid, block;
    unsigned smem;
    alignas(16) unsigned char args[SVLA_DEFER_ARG_BYTES];
};
struct GroupCapture {
    int size = 0, member = 0;
    int n[SVLA_MAXG] = {0, 0, 0};
    bool lockstep = true;              // no member's pending launches were issued ahead of the end
    bool has_stream = false;
    void* stream = nullptr;            // of the capture's first launch
    DeferredLaunch q[SVLA_MAXG][SVLA_MAXQ];
    long grouped = 0, single = 0;      // statistics since group_stats was last read
};
// One per thread (misc.hip): `store` is allocated at the first begin (~13 KiB of argument blocks) and kept, `open` is it while a capture is open
struct GroupState { GroupCapture *open = nullptr, *store = nullptr; };

inline int group_begin(GroupState& g, int members) {
    if (g.open || members < 1 || members > SVLA_MAXG) return SVLA_EINVAL;
    if (!g.store) g.store = new GroupCapture();
    GroupCapture* gc = g.store;
    gc->size = members;
    gc->member = 0;
    gc->lockstep = true;
    gc->has_stream = false;
    gc->stream = nullptr;
    for (int m = 0; m < SVLA_MAXG; ++m) gc->n[m] = 0;
    g.open = gc;
    return SVLA_OK;
}
inline int group_member(GroupState& g, int member) {
    GroupCapture* gc = g.open;
    if (!gc || member < 0 || member >= gc->size) return SVLA_EINVAL;
    gc->member = member;
    return SVLA_OK;
}
inline int group_stats(GroupState& g, long* grouped, long* single) {
    GroupCapture* gc = g.store;
    if (grouped) *grouped = gc ? gc->grouped : 0;
    if (single) *single = gc ? gc->single : 0;
    if (gc) gc->grouped = gc->single = 0;
    return SVLA_OK;
}

// every launch site inside a capture names the capture's stream
inline int group_stream(GroupCapture& gc, void* stream) {
    if (!gc.has_stream) { gc.stream = stream; gc.has_stream = true; }
    return gc.stream == stream ? SVLA_OK : SVLA_EINVAL;
}
// member m's pending launches, singly and in call order
inline int group_issue_member(GroupCapture& gc, int m) {
    int rc = SVLA_OK;
    for (int j = 0; j < gc.n[m] && rc == SVLA_OK; ++j) {
        const DeferredLaunch* one = &gc.q[m][j];
        rc = one->flush(&one, 1, gc.stream);
        gc.single += 1;
    }
    gc.n[m] = 0;
    return rc;
}
// the current member's pending launches go first: before a launch that is issued at once, and when its queue is full
inline int group_issue_pending(GroupCapture& gc) {
    if (gc.n[gc.member] == 0) return SVLA_OK;
    gc.lockstep = false;
    return group_issue_member(gc, gc.member);
}
// A launch that cannot be deferred asks here first; SVLA_OK: issue it now, on `stream`
inline int group_direct(GroupCapture& gc, void* stream) {
    if (const int rc = group_stream(gc, stream)) return rc;
    return group_issue_pending(gc);
}
// A deferral site: the slot to fill (flush, grid, block, smem, args), or nullptr with *rc set
inline DeferredLaunch* group_defer(GroupCapture& gc, void* stream, int* rc) {
    *rc = group_stream(gc, stream);
    if (*rc == SVLA_OK && gc.n[gc.member] == SVLA_MAXQ) *rc = group_issue_pending(gc);
    if (*rc != SVLA_OK) return nullptr;
    return &gc.q[gc.member][gc.n[gc.member]++];
}

inline bool group_same_launch(const DeferredLaunch& a, const DeferredLaunch& b) {
    return a.flush == b.flush && a.smem == b.smem && a.grid.x == b.grid.x && a.grid.y == b.grid.y && a.grid.z == 1 && b.grid.z == 1 &&
           a.block.x == b.block.x && a.block.y == b.block.y && a.block.z == b.block.z;
}
// Closes the capture, then issues what it holds: launch j of all members as one grouped issue where the members are in lockstep and launch j is the same for
// all of them, else singly
inline int group_end(GroupState& g, void* stream) {
    GroupCapture* gc = g.open;
    if (!gc) return SVLA_EINVAL;
    g.open = nullptr;                            // the launches below are real
    if (gc->has_stream && gc->stream != stream) return SVLA_EINVAL;
    bool lockstep = gc->lockstep;
    for (int m = 1; m < gc->size; ++m) lockstep = lockstep && gc->n[m] == gc->n[0];
    int rc = SVLA_OK;
    if (lockstep) {
        for (int j = 0; j < gc->n[0] && rc == SVLA_OK; ++j) {
            const DeferredLaunch* ms[SVLA_MAXG];
            bool same = gc->size > 1;
            for (int m = 0; m < gc->size; ++m) {
                ms[m] = &gc->q[m][j];
                same = same && group_same_launch(gc->q[0][j], gc->q[m][j]);
            }
            if (same) { rc = ms[0]->flush(ms, gc->size, stream); gc->grouped += 1; }
            else for (int m = 0; m < gc->size && rc == SVLA_OK; ++m) { rc = ms[m]->flush(&ms[m], 1, stream); gc->single += 1; }
        }
    } else {        // a member issued launches early, or the members did not make the same number (e.g. one of them has a ragged row tail): member by member, in call order
        for (int m = 0; m < gc->size && rc == SVLA_OK; ++m) rc = group_issue_member(*gc, m);
    }
    return rc;
}
