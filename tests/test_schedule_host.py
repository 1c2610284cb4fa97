"""CPU: the learning-rate schedule class of the driver (lstm-rnn_amd/host/optimizers/LearningRateSchedule.hpp), driven by the
stand-alone program tests/schedule_main.cpp, against a Python restatement of the rule:

    update k = U + 1 runs at f = s * (N > 0 ? min(1, k / N) : 1) and at rate (float)(rate * f)
    epoch end with error e:  e < lowest: lowest = e, bad = 0;  else bad += 1;  bad >= E: s = max(s * F, M / rate), bad = 0

Python floats are the doubles the class computes in, so every printed number must be equal, digit for digit."""
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DBL_MAX = float(np.finfo(np.float64).max)


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no C++ compiler"
    out = str(tmp_path_factory.mktemp("schedule") / "schedule_check")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "lstm-rnn_amd", "host", "optimizers"),
                           os.path.join(ROOT, "tests", "schedule_main.cpp"), "-o", out])
    return out


class Restatement:
    def __init__(self, N, F, E, M, rate):
        self.N, self.F, self.E, self.M = N, F, E, M
        self.rate = float(np.float32(rate))
        self.U, self.s, self.bad, self.lowest = 0, 1.0, 0, DBL_MAX

    def factor(self):
        return self.s * (min(1.0, (self.U + 1) / self.N) if self.N > 0 else 1.0)

    def lr(self):
        return float(np.float32(self.rate * self.factor()))

    def epoch_end(self, e):
        if e < self.lowest:
            self.lowest, self.bad = e, 0
            return
        self.bad += 1
        if self.bad >= self.E:
            self.s = max(self.s * self.F, self.M / self.rate)
            self.bad = 0


def expected(N, F, E, M, rate, script):
    r = Restatement(N, F, E, M, rate)
    lines = ["on %d" % (1 if (N > 0 or F < 1.0) else 0)]
    for item in script:
        if item == "x":
            continue                                        # (an export / import changes nothing)
        k, e = item.split(":")
        for _ in range(int(k)):
            lines.append("u %.17g %.9g" % (r.factor(), r.lr()))
            r.U += 1
        if e != "-":
            r.epoch_end(float(e))
        lines.append("e %.17g %.9g %d %.17g %d %.17g" % (r.factor(), r.lr(), r.U, r.s, r.bad, r.lowest))
    return lines, r


def run(program, N, F, E, M, rate, script):
    out = subprocess.check_output([program, str(N), repr(F), str(E), repr(M), repr(rate)] + script, text=True)
    return out.strip().split("\n")


SCRIPTS = {
    # warm-up alone: N = 7 is no multiple of the 3 updates per epoch; the factor reaches 1 inside the third epoch
    "warm-up": (7, 1.0, 1, 0.0, 1e-3, ["3:2.0", "3:1.9", "3:1.8", "3:1.7"]),
    # decay alone, patience 1: improving, stalling, EQUAL (no improvement), improving again
    "decay, patience 1": (0, 0.5, 1, 0.0, 1e-3, ["2:2.0", "2:1.5", "2:1.6", "2:1.5", "2:1.4", "2:1.4"]),
    # patience 3: three bad epochs in a row before a decay; an improvement in between resets the count
    "decay, patience 3": (0, 0.7, 3, 0.0, 1e-2, ["1:2.0", "1:2.1", "1:2.1", "1:1.9", "1:1.9", "1:2.0", "1:1.95", "1:1.8", "1:1.8"]),
    # the floor: M a quarter of the rate
    "floor": (0, 0.5, 1, 2.5e-4, 1e-3, ["1:1.0", "1:1.0", "1:1.0", "1:1.0", "1:1.0"]),
    # a floor that is no power of F below the rate: the scale lands on M / rate itself
    "floor between": (0, 0.5, 1, 3e-4, 1e-3, ["1:1.0", "1:1.0", "1:1.0", "1:1.0"]),
    # the two combined, an epoch without a monitored error in between
    "combined": (5, 0.5, 2, 1e-5, 3e-3, ["2:3.0", "2:3.0", "2:3.0", "2:-", "2:2.5", "2:2.6", "2:2.7"]),
    # a state export / import in the middle
    "export": (5, 0.5, 2, 1e-5, 3e-3, ["2:3.0", "2:3.0", "x", "2:3.0", "2:-", "x", "2:2.5", "2:2.6", "2:2.7"]),
    # everything at its default: off, factor 1, the rate itself
    "off": (0, 1.0, 1, 0.0, 1e-3, ["2:1.0", "2:1.0"]),
}


@pytest.mark.parametrize("which", list(SCRIPTS))
def test_schedule_equals_the_restatement(program, which):
    N, F, E, M, rate, script = SCRIPTS[which]
    want, r = expected(N, F, E, M, rate, script)
    got = run(program, N, F, E, M, rate, script)
    assert got == want, [(a, b) for a, b in zip(got, want) if a != b][:3]


def test_the_scripts_exercise_what_they_name(program):
    """the restatement itself: the warm-up factors, equal-is-no-improvement, the patience count and the floor"""
    N, F, E, M, rate, script = SCRIPTS["warm-up"]
    lines, r = expected(N, F, E, M, rate, script)
    factors = [float(l.split()[1]) for l in lines if l.startswith("u ")]
    assert factors[:7] == [k / 7 for k in range(1, 8)] and factors[7:] == [1.0] * 5 and r.s == 1.0
    assert lines[1].split()[2] == "%.9g" % float(np.float32(float(np.float32(1e-3)) * (1 / 7)))      # rounded once to float
    _, r = expected(*SCRIPTS["decay, patience 1"][:5], SCRIPTS["decay, patience 1"][5])
    assert r.s == 0.5 ** 3 and r.lowest == 1.4                     # 1.6, the equal 1.5 and the equal 1.4 each decay
    _, r = expected(*SCRIPTS["decay, patience 3"][:5], SCRIPTS["decay, patience 3"][5])
    assert r.s == 0.7 and r.bad == 1 and r.lowest == 1.8           # one decay (2.1, 2.1 do not reach 3; 1.9, 2.0, 1.95 do)
    _, r = expected(*SCRIPTS["floor"][:5], SCRIPTS["floor"][5])
    assert r.s == 2.5e-4 / float(np.float32(1e-3)) and 0.2499999 < r.s < 0.25      # (the rate is the float the option holds)
    _, r = expected(*SCRIPTS["floor between"][:5], SCRIPTS["floor between"][5])
    assert r.s == 3e-4 / float(np.float32(1e-3))
    a = run(program, *SCRIPTS["combined"][:5], SCRIPTS["combined"][5])
    b = run(program, *SCRIPTS["export"][:5], SCRIPTS["export"][5])
    assert a == b
    assert run(program, *SCRIPTS["off"][:5], SCRIPTS["off"][5])[0] == "on 0"
