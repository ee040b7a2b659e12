"""The row-range check of the resident blocks (soc_amd/csrc/soc_rows.h: soc_rows_ok), which every transfer call of the C ABI makes
through SOC_ROWS, on the host: the harness tests/csrc/rows_host.cpp compiles the product header with g++ -- as a library, and as a
program of its own with -fsanitize=undefined, which a sum c0 + n near the int64 limits would stop."""
import ctypes as C
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
SRC = os.path.join(HERE, "csrc", "rows_host.cpp")
INT64_MAX = 2 ** 63 - 1
CASES = [(0, 10, True), (9, 1, True), (10, 1, False), (0, 11, False), (-1, 1, False), (0, 0, False), (INT64_MAX, 1, False),
         (1, INT64_MAX, False)]


@pytest.fixture(scope="module")
def lib():
    out = os.path.join(REPO, "oracle", "_build", "librows_host.so")
    deps = [SRC, os.path.join(REPO, "soc_amd", "csrc", "soc_rows.h")]
    if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps):
        os.makedirs(os.path.dirname(out), exist_ok=True)
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fPIC", "-shared", "-Wall", "-o", out, SRC])
    L = C.CDLL(out)
    L.rows_ok.argtypes = [C.c_longlong] * 3
    return L


@pytest.mark.parametrize("c0, n, ok", CASES)
def test_rows_of_ten_cells(lib, c0, n, ok):
    assert bool(lib.rows_ok(c0, n, 10)) == ok


def test_no_range_overflows_the_check(tmp_path):
    exe = str(tmp_path / "rows_host")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-DROWS_HOST_MAIN", "-fsanitize=undefined", "-fno-sanitize-recover",
                           SRC, "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "rows ok" in out.stdout
