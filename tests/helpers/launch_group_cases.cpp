// tests/test_launch_group_cpu.py: the capture logic of safevla_amd/csrc/launch_group.h driven with flush functions that print instead of launching.  Plain C++17, no HIP.
// A launch is named by a tag ("m1.a": member 1, launch a) kept in its argument block; one line per issue, in the order the stream would see them.
#include <cstdio>
#include <cstring>
#include "launch_group.h"

static GroupState g;
static int s1_, s2_;
static void *const S1 = &s1_, *const S2 = &s2_;

static int rec(const DeferredLaunch* const* m, int n, void*) {
    printf("%s", n > 1 ? "grouped" : "single");
    for (int i = 0; i < n; ++i) printf(" %s", (const char*)m[i]->args);
    printf("\n");
    return 0;
}
// what a deferral site does inside a capture (csrc/launch.h: svla_defer_or_issue)
static void defer(const char* tag, unsigned grid_x = 1, void* stream = S1) {
    int rc = 0;
    DeferredLaunch* d = group_defer(*g.open, stream, &rc);
    if (!d) { printf("refused %s %d\n", tag, rc); return; }
    d->flush = rec;
    d->grid = LaunchDim{grid_x, 1, 1}; d->block = LaunchDim{256, 1, 1}; d->smem = 0;
    strcpy((char*)d->args, tag);
}
// and a launch that cannot be deferred (svla_launch, an assembly kernel, a memset, a copy)
static void direct(const char* tag, void* stream = S1) {
    const int rc = group_direct(*g.open, stream);
    if (rc) printf("refused %s %d\n", tag, rc);
    else printf("direct %s\n", tag);
}
static void begin(int no, int members) { printf("case %d\n", no); group_begin(g, members); }
static void end(void* stream = S1) {
    printf("ending\n");
    printf("end %d\n", group_end(g, stream));
    long grouped = -1, single = -1;
    group_stats(g, &grouped, &single);
    printf("stats %ld %ld\n", grouped, single);
}
static const char* tag(char* buf, int m, const char* name) { sprintf(buf, "m%d.%s", m, name); return buf; }

int main() {
    char t[16];
    begin(1, 3);
    for (int m = 0; m < 3; ++m) { group_member(g, m); defer(tag(t, m, "a")); defer(tag(t, m, "b")); }
    end();
    begin(2, 3);
    for (int m = 0; m < 3; ++m) { group_member(g, m); defer(tag(t, m, "a")); defer(tag(t, m, "b"), m == 1 ? 2 : 1); }
    end();
    begin(3, 3);
    for (int m = 0; m < 3; ++m) { group_member(g, m); defer(tag(t, m, "a")); if (m != 1) defer(tag(t, m, "b")); }
    end();
    begin(4, 3);
    group_member(g, 0); defer("m0.a");
    group_member(g, 1); defer("m1.a"); direct("m1.x"); defer("m1.b");
    group_member(g, 2); defer("m2.a");
    end();
    begin(5, 3);
    for (int m = 0; m < 3; ++m) { group_member(g, m); direct(tag(t, m, "x")); defer(tag(t, m, "a")); }
    end();
    begin(6, 1);
    for (int j = 0; j < SVLA_MAXQ + 1; ++j) { sprintf(t, "m0.l%d", j); defer(t); }
    end();
    begin(7, 2);
    defer("m0.a"); defer("m0.b", 1, S2); direct("m0.x", S2);
    end(S2);
    printf("begin %d\n", group_begin(g, 2));
    end(nullptr);
    printf("case 8\n");
    const int rc[] = {group_end(g, nullptr), group_begin(g, 0), group_begin(g, 4), group_begin(g, 3), group_begin(g, 3),      // (a braced list is evaluated left to right)
                      group_member(g, 3), group_member(g, -1), group_member(g, 2), group_end(g, nullptr)};
    printf("protocol");
    for (int r : rc) printf(" %d", r);
    printf("\n");
    long grouped = -1, single = -1;
    group_stats(g, &grouped, &single);
    printf("stats %ld %ld\n", grouped, single);
    delete g.store;
    return 0;
}
