"""K1's cherry-table kernels (prune_kernel_ct6 / ct5 / ct4, linearham_amd/csrc/lh_prune.hip) outside their walk: no scalar
registers parked in vector lanes beyond a remainder, no vector registers in scratch memory, fewer vector instructions.

The kernels are bound by vector-instruction issue, and a scalar register the compiler cannot keep costs a v_writelane_b32
and a v_readlane_b32 each time.  They used to take 21 parameters that lived from entry to exit beside the 56 scalar
registers of the eigen-system and across a walk statement that leaves a dozen; now each phase of the kernel reads what it
needs from one argument block.  This test compiles the kernel file to gfx950 assembly (as test_k1_scalar_readback.py
does) and counts, per kernel and outside the ASMSTART / ASMEND regions (the generated walk):
  lane moves   v_readlane_b32 + v_writelane_b32
  scratch ops  scratch_* instructions (the walk's result and deep-stack area are read back with 8; the rest are spills)
  vector       v_* instructions, and those among them that name f64
PARENT holds the counts of the kernels before the change; every instantiation must stay at or below them on every count,
the two default kernels (configs[2] without and with N in the alignment) at most at half the lane moves.  REACHED pins
what the change arrived at, with about 10 % allowance for compiler noise, so that the spills cannot return unnoticed."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "linearham_amd", "csrc", "lh_prune.hip")

# (waves per SIMD, N-aware, fused, assembly walk) -> (lane moves, scratch ops, vector instructions, of which f64);
# the stack depths 4 and 16 compile to the same counts
PARENT = {
    (6, True, True, True): (215, 10, 1347, 664), (5, True, True, True): (221, 12, 1353, 664),
    (4, True, True, True): (219, 8, 1351, 664),
    (6, True, False, True): (199, 8, 1148, 632), (5, True, False, True): (199, 12, 1148, 632),
    (4, True, False, True): (199, 8, 1148, 632),
    (6, True, True, False): (159, 24, 1583, 736), (5, True, True, False): (159, 16, 1583, 736),
    (4, True, True, False): (159, 12, 1583, 736),
    (6, True, False, False): (116, 22, 1371, 704), (5, True, False, False): (116, 16, 1371, 704),
    (4, True, False, False): (116, 12, 1371, 704),
    (6, False, True, True): (248, 19, 1296, 592), (5, False, True, True): (248, 22, 1295, 592),
    (4, False, True, True): (248, 8, 1295, 592),
    (6, False, False, True): (224, 19, 1080, 560), (5, False, False, True): (224, 15, 1080, 560),
    (4, False, False, True): (224, 8, 1080, 560),
    (6, False, True, False): (177, 37, 1484, 664), (5, False, True, False): (177, 26, 1485, 664),
    (4, False, True, False): (177, 12, 1485, 664),
    (6, False, False, False): (128, 31, 1259, 632), (5, False, False, False): (128, 19, 1259, 632),
    (4, False, False, False): (128, 12, 1259, 632),
}
DEFAULTS = [(6, False, True, True), (6, True, True, True)]
# what the change reached for the two default kernels (lane moves, scratch ops, vector instructions)
REACHED = {(6, False, True, True): (81, 8, 995), (6, True, True, True): (78, 8, 1068)}


def kernel_counts(text):
    """{(waves, kN, kFused, kAsm, depth): (lane moves, scratch ops, vector instructions, f64 ones)} of an assembly listing"""
    out = {}
    for name, body in re.findall(r"^(_ZN2lh\w*prune_kernel_ct\w*):[^\n]*\n(.*?)^\.Lfunc_end", text, flags=re.S | re.M):
        # ...prune_kernel_ct6ILi4ELb0ELb1ELb1EEv...: the budget and the template arguments from the mangled name
        m = re.search(r"prune_kernel_ct(\d)ILi(\d+)ELb([01])ELb([01])ELb([01])E", name)
        assert m, name
        key = (int(m.group(1)), m.group(3) == "1", m.group(4) == "1", m.group(5) == "1", int(m.group(2)))
        lane = scratch = vec = f64 = 0
        inside = False
        for line in body.splitlines():
            s = line.strip()
            if "#ASMSTART" in s:
                inside = True
            elif "#ASMEND" in s:
                inside = False
            elif not inside and s:
                op = s.split()[0]
                if op.startswith("scratch_"):
                    scratch += 1
                if op.startswith("v_"):
                    vec += 1
                    lane += op in ("v_readlane_b32", "v_writelane_b32")
                    f64 += "f64" in op
        out[key] = (lane, scratch, vec, f64)
    return out


@pytest.fixture(scope="module")
def counts(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    out = str(tmp_path_factory.mktemp("k1_spills") / "lh_prune.s")
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "-S",
                           "-I", os.path.join(ROOT, "include"), "-I", os.path.dirname(SRC), SRC, "-o", out],
                          stderr=subprocess.DEVNULL)
    got = kernel_counts(open(out).read())
    for key, c in sorted(got.items()):
        print("ct%d<%d,%s,%s,%s>: lane moves %d, scratch ops %d, vector %d (f64 %d)" % (key[0], key[4], *key[1:4], *c))
    return got


def test_every_instantiation_is_there(counts):
    assert {k[:4] for k in counts} == set(PARENT)
    assert {k[4] for k in counts} == {4, 16}


def test_default_kernels_halve_the_lane_moves(counts):
    for key in DEFAULTS:
        parent = PARENT[key]
        for depth in (4, 16):
            lane, scratch, vec, f64 = counts[key + (depth,)]
            assert lane <= parent[0] // 2, (key, depth, lane)          # <= 124 and <= 107
            assert scratch <= parent[1], (key, depth, scratch)
            assert vec < parent[2], (key, depth, vec)
            assert f64 <= parent[3], (key, depth, f64)


def test_no_instantiation_is_worse_than_its_parent(counts):
    for key, got in sorted(counts.items()):
        parent = PARENT[key[:4]]
        for what, g, p in zip(("lane moves", "scratch ops", "vector instructions", "f64 instructions"), got, parent):
            assert g <= p, (key, what, g, p)


def test_the_counts_reached_stay(counts):
    for key, reached in REACHED.items():
        for depth in (4, 16):
            got = counts[key + (depth,)]
            for what, g, r in zip(("lane moves", "scratch ops", "vector instructions"), got, reached):
                assert g <= r + (r + 9) // 10, (key, depth, what, g, r)
