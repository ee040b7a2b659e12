"""The integer forms of soc_ltree.h that replaced longer expressions (the sibling slot of soc_lt_aim), new against old, on the host:
tests/csrc/ltree_diet_host.cpp, a stand-alone program built with -fsanitize=address,undefined and run as a program."""
import os
import subprocess

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_new_forms_equal_the_old_expressions(tmp_path):
    exe = str(tmp_path / "ltree_diet_host")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-mfma", "-Wall", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-I", os.path.join(REPO, "soc_amd", "csrc"),
                           os.path.join(REPO, "tests", "csrc", "ltree_diet_host.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "ltree diet ok" in out.stdout
