// What the stand-alone check programs (tests/*_check.cpp) share: a counter of failed checks, expect() and main's exit status.
#pragma once
#include <cstdio>

static int g_failures = 0;

static inline void expect(bool ok, const char* what) {
    if (!ok) {
        ++g_failures;
        std::fprintf(stderr, "FAIL %s\n", what);
    }
}

// what main returns: 1, with the count on stderr, where a check failed
static inline int exit_status() {
    if (g_failures) std::fprintf(stderr, "%d checks failed\n", g_failures);
    return g_failures ? 1 : 0;
}
