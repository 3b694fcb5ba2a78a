// min_anchor_check.cpp -- raft_cli::parse_min_anchor (raft_amd/host/cli_plan.hpp), the argument of `raft --repeat-overlaps A`, on the
// CPU: built by the host compiler under the address and undefined-behaviour sanitizers and run as a process of its own
// (tests/test_min_anchor_parse.py).
#include "cli_check.hpp"

// (the text in a heap block of exactly its size: a read past the terminator is the sanitizer's to see)
static void good(const char *text, int32_t want)
{
    int32_t v = -77;
    CHECK(cli_check::parsed(raft_cli::parse_min_anchor, text, &v) && v == want, "\"%s\" should give %d, gave %d", text, want, v);
}

static void bad(const char *text)
{
    int32_t v = -77;
    CHECK(!cli_check::parsed(raft_cli::parse_min_anchor, text, &v) && v == -77, "\"%s\" should be refused and leave the value alone (%d)", text, v);
}

int main()
{
    good("1", 1); good("1000", 1000); good("0001", 1); good("2147483647", 2147483647); good("999999999", 999999999);
    for (const char *t : {"0", "00", "", "-1", "+1", " 1", "1 ", "1.5", "1e3", "x", "12x", "0x10", "2147483648", "4294967297", "99999999999999999999",
                          "18446744073709551617", "\t5", "5\n"})
        bad(t);
    int32_t v = 5;
    CHECK(!raft_cli::parse_min_anchor(nullptr, &v) && v == 5, "NULL");
    return cli_check::finish("min_anchor_check");
}
