// query_args_check.cpp -- the argument decisions of the record-stream queries (raft_amd/csrc/query_args.hpp) on the CPU: built by the
// host compiler under the address and undefined-behaviour sanitizers and run as a process of its own (tests/test_query_args.py).
// The expected answers are written out here from the contracts of include/raft_hip_ovl.h, raft_hip_frag.h and raft_hip_rst.h, not
// computed with the header's own expressions.
#include "../raft_amd/csrc/query_args.hpp"

#include <cstdio>

using namespace raft;

static int failures = 0;

static const char *name(CsrKind k)
{
    return k == CsrKind::own ? "own" : k == CsrKind::given ? "given" : k == CsrKind::none ? "none" : "bad";
}

// count x (off, x, y set or NULL): 32 rows.  The contracts: "all three NULL with n == -1: the context's own finished pass"; "all NULL
// with n_rep == 0 for none"; explicit arrays with a count >= 0 need the offsets and the row arrays, and "with n == 0 the row arrays may
// be NULL" -- both of them, they are one table; everything else is an error.
static void check_csr()
{
    static int64_t off[2];
    static int32_t x[1], y[1];
    const CsrKind B = CsrKind::bad, G = CsrKind::given;
    struct Row { int64_t count; bool off, x, y; CsrKind want; };
    const Row table[] = {
        // count -2: never
        {-2, false, false, false, B}, {-2, false, false, true, B}, {-2, false, true, false, B}, {-2, false, true, true, B},
        {-2, true, false, false, B},  {-2, true, false, true, B},  {-2, true, true, false, B},  {-2, true, true, true, B},
        // count -1: the own pass, and only without any array
        {-1, false, false, false, CsrKind::own}, {-1, false, false, true, B}, {-1, false, true, false, B}, {-1, false, true, true, B},
        {-1, true, false, false, B},  {-1, true, false, true, B},  {-1, true, true, false, B},  {-1, true, true, true, B},
        // count 0: no table at all, or the offsets with both row arrays or neither
        {0, false, false, false, CsrKind::none}, {0, false, false, true, B}, {0, false, true, false, B}, {0, false, true, true, B},
        {0, true, false, false, G},   {0, true, false, true, B},   {0, true, true, false, B},   {0, true, true, true, G},
        // count 1: all three
        {1, false, false, false, B},  {1, false, false, true, B},  {1, false, true, false, B},  {1, false, true, true, B},
        {1, true, false, false, B},   {1, true, false, true, B},   {1, true, true, false, B},   {1, true, true, true, G},
    };
    int rows = 0;
    for (const Row &r : table) {
        const CsrArg a{r.count, r.off ? off : nullptr, r.x ? x : nullptr, r.y ? y : nullptr};
        const CsrKind got = csr_arg_kind(a);
        if (got != r.want) {
            printf("FAIL: count %lld off %d x %d y %d: %s, want %s\n", (long long)r.count, r.off, r.x, r.y, name(got), name(r.want));
            ++failures;
        }
        ++rows;
    }
    if (rows != 4 * 8) { printf("FAIL: %d rows\n", rows); ++failures; }
}

// n_rec in {0, 1} x symmetric x every subset of NULL columns, under the three rules.  Expected, from the headers: with records qid, qs,
// qe, tid are needed; ts / te are needed unless symmetric (fragment_overlaps: always); repeat_overlaps and repeat_stats take ts / te
// as a pair, both or neither, whatever n_rec; the census does not look at them under symmetric; without a record nothing else is asked.
static void check_columns()
{
    static int32_t data[6][4];
    int cases = 0;
    for (int64_t n_rec = 0; n_rec <= 1; ++n_rec)
        for (int sym = 0; sym <= 1; ++sym)
            for (int null_mask = 0; null_mask < 64; ++null_mask) {
                RecordCols r{n_rec, {}};
                for (int k = 0; k < 6; ++k) r.col[k] = (null_mask >> k) & 1 ? nullptr : data[k];
                const bool first4 = (null_mask & 15) == 0, ts = !(null_mask & 16), te = !(null_mask & 32);
                const bool want_always = n_rec == 0 || (first4 && ts && te);
                const bool want_pair = ts == te && (n_rec == 0 || (first4 && (sym || ts)));
                const bool want_unread = n_rec == 0 || (first4 && (sym || (ts && te)));
                const struct { TargetCols rule; bool want; const char *what; } rules[] = {
                    {TargetCols::always, want_always, "always"}, {TargetCols::unless_symmetric, want_pair, "unless_symmetric"},
                    {TargetCols::unread_if_symmetric, want_unread, "unread_if_symmetric"}};
                for (const auto &q : rules) {
                    if (record_cols_ok(r, sym != 0, q.rule) != q.want) {
                        printf("FAIL: n_rec %lld symmetric %d NULL mask %d rule %s: want %d\n", (long long)n_rec, sym, null_mask, q.what, q.want);
                        ++failures;
                    }
                    ++cases;
                }
            }
    if (cases != 2 * 2 * 64 * 3) { printf("FAIL: %d cases\n", cases); ++failures; }
}

static void check_alignment()
{
    alignas(16) static int32_t data[6][8];
    RecordCols r{4, {data[0], data[1], data[2], data[3], data[4], data[5]}};
    if (!aligned16(r)) { printf("FAIL: six aligned columns\n"); ++failures; }
    for (int k = 0; k < 6; ++k) {                       // one column 4 bytes on: the four-record loads are off
        RecordCols s = r;
        s.col[k] = data[k] + 1;
        if (aligned16(s)) { printf("FAIL: column %d offset by 4 bytes\n", k); ++failures; }
        s.col[k] = data[k] + 4;                         // ... and 16 bytes on: aligned again
        if (!aligned16(s)) { printf("FAIL: column %d offset by 16 bytes\n", k); ++failures; }
    }
    r.col[4] = r.col[5] = nullptr;                      // columns that are not there do not count
    if (!aligned16(r)) { printf("FAIL: NULL target columns\n"); ++failures; }
    r.col[5] = data[5] + 1;
    if (aligned16(r)) { printf("FAIL: te offset by 4 bytes beside a NULL ts\n"); ++failures; }
}

int main()
{
    check_csr();
    check_columns();
    check_alignment();
    if (failures) return 1;
    printf("query_args_check: ok\n");
    return 0;
}
