// query_args.hpp -- what the queries about a record stream (census, repeat_overlaps, fragment_overlaps, repeat_stats) decide about
// their arguments before anything is staged or launched, as plain functions: which record columns must be there, what the three
// arrays of a CSR table say, which load path the columns allow.  No HIP call and no HIP header: a host compiler alone builds it
// (tests/query_args_check.cpp does).  What is a query's own -- its size limits, min_anchor, threshold, whether a table may be left
// out, the state of the context -- stays in its check_call.
#pragma once
#include <cstdint>

namespace raft {

struct RecordCols {                   // qid, qs, qe, tid, ts, te
    int64_t n_rec;
    const int32_t *col[6];
};

struct CsrArg {                       // a count and the three arrays of a CSR table by read: offsets [n_reads + 1], two row arrays
    int64_t count;
    const int64_t *off;
    const int32_t *x, *y;
};

// When ts / te may be NULL beside records.
enum class TargetCols {
    always,                           // never: all six columns (fragment_overlaps)
    unless_symmetric,                 // both or neither, neither only under symmetric (repeat_overlaps, repeat_stats)
    unread_if_symmetric,              // under symmetric they are not looked at, not even as a pair (census)
};

// n_rec >= 0 is the caller's check.  Without a record no column is needed; ts / te are a pair even then where the rule pairs them.
inline bool record_cols_ok(const RecordCols &r, bool symmetric, TargetCols rule)
{
    if (rule == TargetCols::unless_symmetric && (r.col[4] == nullptr) != (r.col[5] == nullptr)) return false;
    if (r.n_rec <= 0) return true;
    for (int k = 0; k < 4; ++k)
        if (!r.col[k]) return false;
    if (rule != TargetCols::always && symmetric) return true;
    return r.col[4] && r.col[5];
}

// What count and arrays say together (include/raft_hip_ovl.h, raft_hip_frag.h, raft_hip_rst.h):
//   own    count -1, no array: the table of the context's finished pass
//   none   count 0, no array: no table at all (only fragment_overlaps' repeats may be left out)
//   given  count >= 0, the offsets, and both row arrays -- or, with count 0, neither: they have nothing to point at
enum class CsrKind { own, given, none, bad };

inline CsrKind csr_arg_kind(const CsrArg &a)
{
    const bool rows = a.x && a.y, no_rows = !a.x && !a.y;
    if (!a.off && no_rows) return a.count == -1 ? CsrKind::own : a.count == 0 ? CsrKind::none : CsrKind::bad;
    if (a.count < 0 || !a.off) return CsrKind::bad;
    return rows || (no_rows && a.count == 0) ? CsrKind::given : CsrKind::bad;
}

// every column that is there begins on a 16-byte line: the kernels' four-record loads (NULL counts as aligned)
inline bool aligned16(const RecordCols &r)
{
    uintptr_t bits = 0;
    for (int k = 0; k < 6; ++k) bits |= reinterpret_cast<uintptr_t>(r.col[k]);
    return (bits & 15) == 0;
}
// ... and two columns beside the six (filter_overlaps: matches, block)
inline bool aligned16(const RecordCols &r, const void *a, const void *b)
{
    return aligned16(r) && ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b)) & 15) == 0;
}

} // namespace raft
