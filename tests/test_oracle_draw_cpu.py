"""oracle/linearham_oracle.discrete_distribution_draw against the real std::discrete_distribution<int> over a std::mt19937
whose next outputs are given words (tests/discrete_draw_main.cpp, compiled here with the system compiler): the index drawn
and the engine outputs consumed, on the weight vectors where the restatement could part from libstdc++ -- no positive
weight (0 / 0 in every quotient), zero blocks at either end, inf and NaN weights, subnormals, a single weight (no draw) --
and on random ones, each with a uniform of exactly 0, the largest below 1 (two word pairs reach it) and the smallest above
0, and with random word pairs.  No GPU."""
import math
import os
import shutil
import subprocess
import warnings

import numpy as np
import pytest

from oracle import linearham_oracle as orc

HERE = os.path.dirname(os.path.abspath(__file__))
FIXED_WORDS = [(0, 0), (0xFFFFFFFF, 0xFFFFFFFF), (1, 0), (0xFFFFF800, 0xFFFFFFFF)]
N_RANDOM_WORDS = 4
SUB = 5e-324


def vectors():
    rng = np.random.default_rng(20)
    out = [("all zeros", [0.0] * 7), ("all zeros, two", [0.0, 0.0])]
    for n in (2, 9, 40):
        for name, at in (("first", 0), ("middle", n // 2), ("last", n - 1)):
            v = [0.0] * n
            v[at] = 0.37
            out.append(("one positive weight, %s of %d" % (name, n), v))
    body = list(rng.uniform(0.01, 1.0, size=11))
    out.append(("leading zero block", [0.0] * 17 + body))
    out.append(("trailing zero block", body + [0.0] * 17))
    out.append(("zero blocks at both ends", [0.0] * 16 + body + [0.0] * 16))
    for at in (0, 5, 10):
        v = list(body)
        v[at] = math.inf
        out.append(("inf at %d" % at, v))
        v = list(body)
        v[at] = math.nan
        out.append(("NaN at %d" % at, v))
    out.append(("two infs", [0.5, math.inf, 0.25, math.inf, 0.125]))
    out.append(("all NaN", [math.nan] * 6))
    out.append(("subnormals beside normal weights", [SUB, 0.5, 3 * SUB, 2.0 ** -1030, 0.25, SUB]))
    out.append(("subnormals only", [SUB, 3 * SUB, 2.0 ** -1060, 0.0, SUB]))
    out.append(("huge weights: the sum overflows", [1e308, 1e308, 1e308]))
    out.append(("length 1", [0.7]))
    out.append(("length 1, zero", [0.0]))
    out.append(("length 0", []))
    for i in range(200):
        n = int(rng.integers(2, 301))
        v = rng.uniform(0.0, 1.0, size=n) * np.ldexp(1.0, rng.integers(-300, 1, size=n) if i % 4 == 0 else 0)
        if i % 3 == 0:   # the zero structure of a junction row: most states have no predecessor
            v[rng.uniform(size=n) < 0.7] = 0.0
        out.append(("random %d" % i, [float(x) for x in v]))
    return out


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no C++ compiler"
    exe = str(tmp_path_factory.mktemp("discrete_draw") / "discrete_draw")
    subprocess.run([cxx, "-O1", "-std=c++17", os.path.join(HERE, "discrete_draw_main.cpp"), "-o", exe], check=True,
                   capture_output=True, text=True)
    return exe


def _fmt(x):
    return "nan" if x != x else "inf" if x == math.inf else float(x).hex()


def test_draw_equals_libstdcxx(program):
    rng = np.random.default_rng(21)
    jobs = []
    for name, v in vectors():
        pairs = FIXED_WORDS + [tuple(int(x) for x in rng.integers(0, 2 ** 32, size=2)) for _ in range(N_RANDOM_WORDS)]
        jobs += [(name, v, p) for p in pairs]
    text = "".join("%d %d %d %s\n" % (p[0], p[1], len(v), " ".join(_fmt(x) for x in v)) for _, v, p in jobs)
    r = subprocess.run([program], input=text, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.split("\n")[:-1]
    assert len(lines) == len(jobs)
    seen = dict(first_by_nan=0, last=0, words=set())
    with warnings.catch_warnings():
        warnings.simplefilter("error")        # (no NumPy or Python warning may leak out of the draw)
        for (name, v, p), line in zip(jobs, lines):
            want_k, want_used = (int(x) for x in line.split())
            assert want_used >= 0, (name, "the program could not tell how many outputs the draw consumed")
            used = []

            def engine():
                used.append(1)
                return p[len(used) - 1] if len(used) <= 2 else len(used) - 1
            k = orc.discrete_distribution_draw(np.array(v, dtype=float), engine)
            assert (k, len(used)) == (want_k, want_used), (name, p, (k, len(used)), (want_k, want_used))
            seen["words"].add(want_used)
            if len(v) > 1 and not sum(v) > 0:
                assert k == 0, (name, p, k)
                seen["first_by_nan"] += 1
            if len(v) > 1 and k == len(v) - 1 and v[-1] == 0.0:
                seen["last"] += 1
    # the vectors reach what they are for: draws without a positive weight, draws beyond the last partial sum that
    # return a trailing zero-weight element, vectors that take no words
    assert seen["first_by_nan"] >= 16 and seen["last"] >= 2 and seen["words"] == {0, 2}, seen


def test_draw_of_zeros_raises_nothing():
    """what the oracle met before: ZeroDivisionError on a vector of zeros"""
    words = iter([0, 0])
    assert orc.discrete_distribution_draw(np.zeros(5), lambda: next(words)) == 0
    assert orc._ieee_div(1.0, 0.0) == math.inf and orc._ieee_div(-1.0, 0.0) == -math.inf
    assert orc._ieee_div(1.0, -0.0) == -math.inf and math.isnan(orc._ieee_div(0.0, 0.0))
    assert math.isnan(orc._ieee_div(math.nan, 0.0)) and orc._ieee_div(math.inf, 0.0) == math.inf
