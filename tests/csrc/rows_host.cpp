// Host harness of tests/test_rows.py: the row-range check of the resident blocks (soc_amd/csrc/soc_rows.h: soc_rows_ok) behind a C
// interface, and -- with -DROWS_HOST_MAIN -- a program of its own that the test builds with -fsanitize=undefined and runs.
#include "../../soc_amd/csrc/soc_rows.h"

extern "C" int rows_ok(long long c0, long long n, long long cells) { return soc_rows_ok(c0, n, cells) ? 1 : 0; }

#ifdef ROWS_HOST_MAIN
#include <stdio.h>

int main()
{
    const struct { int64_t c0, n; int ok; } t[] = { { 0, 10, 1 }, { 9, 1, 1 }, { 10, 1, 0 }, { 0, 11, 0 }, { -1, 1, 0 }, { 0, 0, 0 },
                                                    { INT64_MAX, 1, 0 }, { 1, INT64_MAX, 0 } };
    int bad = 0;
    for (const auto &r : t) {
        if (rows_ok(r.c0, r.n, 10) != r.ok) {
            printf("rows [%lld, +%lld) of 10: expected %d\n", (long long)r.c0, (long long)r.n, r.ok);
            bad++;
        }
    }
    if (!bad) printf("rows ok\n");
    return bad ? 1 : 0;
}
#endif
