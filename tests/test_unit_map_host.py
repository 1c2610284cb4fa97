"""CPU: the map of a layer's units to the columns of its padded rows (lstm-rnn_amd/csrc/cn_unit_map.h), which host code and every
feature kernel read, walked by the stand-alone program tests/unit_map_main.cpp against a brute-force table of each layout:
unit(col(u)) == u, pad columns map to -1, the columns of the units ascend, and the units among an aligned group of 4 or 8
columns are counted right and come first.  The header must build with the plain host compiler, without HIP."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no C++ compiler"
    out = str(tmp_path_factory.mktemp("unit_map") / "unit_map_check")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "lstm-rnn_amd", "csrc"),
                           os.path.join(ROOT, "tests", "unit_map_main.cpp"), "-o", out])
    return out


def test_unit_map_holds_on_every_layout(program):
    r = subprocess.run([program], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "unit_map: ok", r.stdout + r.stderr
