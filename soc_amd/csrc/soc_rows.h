// soc_rows.h -- THE check of a row range of a resident block: rows [c0, c0 + n) of `cells`.  No HIP in it: the host units use it through
// SOC_ROWS (soc_host.h), tests/test_rows.py compiles it with g++.  No sum is formed, so no c0 or n can overflow it.
#pragma once
#include <stdint.h>

static inline bool soc_rows_ok(int64_t c0, int64_t n, int64_t cells)
{
    return c0 >= 0 && n >= 1 && c0 <= cells && n <= cells - c0;
}
