// cli_check.hpp -- what the check programs of raft_amd/host/cli_plan.hpp share (tests/cli_plan_*_check.cpp, tests/min_anchor_check.cpp;
// each is built under the address and undefined-behaviour sanitizers and run as a process of its own by raft_testlib.build_and_run_check):
// CHECK, which counts and goes on, the exit that reports the count, the exact-size heap copy of an option's text, and the
// cross-option decisions (raft_cli::usage_ok, raft_cli::request) over the few values each of them reads.
#pragma once
#include "../raft_amd/host/cli_plan.hpp"

#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

namespace cli_check {

inline int g_failed = 0;

// the first twenty failures are shown: where, the condition, and the message where the check has one
inline void failed(const char *file, int line, const char *cond, const char *fmt, ...)
{
    if (++g_failed > 20) return;
    fprintf(stderr, "%s:%d: %s", file, line, cond);
    if (*fmt) {
        fputs(" -- ", stderr);
        va_list ap;
        va_start(ap, fmt);
        vfprintf(stderr, fmt, ap);
        va_end(ap);
    }
    fputc('\n', stderr);
}

// `NAME: ok` on stdout and 0, or the count on stderr and 1: what main() returns
inline int finish(const char *name)
{
    if (g_failed) { fprintf(stderr, "%s: %d checks failed\n", name, g_failed); return 1; }
    printf("%s: ok\n", name);
    return 0;
}

// parse(text, v) with the text in a heap block of exactly its size, so that a read behind its end is the sanitizer's
template <class F> bool parsed(F parse, const char *text, int32_t *v)
{
    char *copy = (char *)malloc(strlen(text) + 1);
    strcpy(copy, text);
    const bool ok = parse(copy, v);
    free(copy);
    return ok;
}

// usage_ok over the values its four rules read (the options not named are as the command line leaves them without them)
inline bool usage(int32_t overlap_ends, bool ratio_given, bool best_overlaps, bool unitigs, bool fragment_paf, bool min_given)
{
    raft_cli::Options o;
    o.overlap_ends = overlap_ends; o.ends_ratio_given = ratio_given; o.best_overlaps = best_overlaps; o.unitigs = unitigs;
    o.fragment_paf = fragment_paf; o.fragment_paf_min_given = min_given;
    return raft_cli::usage_ok(o);
}

// Request::paf_columns of a job with or without the filter (--min-overlap 1), --overlap-ends H (-1: without) and --fragment-paf
inline int columns(bool filter, int32_t overlap_ends, bool fragment_paf)
{
    raft_cli::Options o;
    o.min_overlap = filter ? 1 : 0; o.overlap_ends = overlap_ends; o.fragment_paf = fragment_paf;
    return raft_cli::request(o, false).paf_columns;
}

// Request::keep_query_ids
inline bool keeps(bool prepare, int32_t min_anchor, bool fragment_overlaps, bool fragment_paf)
{
    raft_cli::Options o;
    o.min_anchor = min_anchor; o.fragment_overlaps = fragment_overlaps; o.fragment_paf = fragment_paf;
    return raft_cli::request(o, prepare).keep_query_ids;
}

} // namespace cli_check

// CHECK(cond) or CHECK(cond, "printf format", args...)
#define CHECK(cond, ...)                                                                          \
    do {                                                                                          \
        if (!(cond)) cli_check::failed(__FILE__, __LINE__, #cond, "" __VA_ARGS__);                \
    } while (0)
