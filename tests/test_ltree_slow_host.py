"""The slow-step test of soc_lt_aim (soc_ltree.h) as straight-line code, against the expression it replaced, on the host:
tests/csrc/ltree_slow_host.cpp, a stand-alone program built with -fsanitize=address,undefined and run as a program."""
import os
import subprocess

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_slow_equals_the_old_expression(tmp_path):
    exe = str(tmp_path / "ltree_slow_host")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-mfma", "-Wall", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-I", os.path.join(REPO, "soc_amd", "csrc"),
                           os.path.join(REPO, "tests", "csrc", "ltree_slow_host.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "ltree slow ok" in out.stdout
