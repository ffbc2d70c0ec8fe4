"""K2a (emission_kernel, linearham_amd/csrc/lh_forward.hip) keeps its register budget.

The kernel is bound by vector-instruction issue and runs eight workgroups of four waves per CU: that takes at most 64 vector
registers for the instantiation configs[2] runs and at most 80 scalar registers for every one (the kernel's
amdgpu_num_sgpr).  fill_consensus' rounds of eight departures are tested once per round instead of once per factor; the
round keeps eight factors, their high words' extremes and two copies of the multiplication chain in flight, and the function
is inlined into every instantiation so that no call's register convention applies.  This test compiles the file to gfx950
assembly (as test_k1_scalar_spills.py does for K1) and reads every instantiation's counts from the code object's metadata:
  vector registers   at most the count before that change (PARENT_VGPR), no spills
  scalar registers   at most 80
"""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "linearham_amd", "csrc", "lh_forward.hip")

# emission_kernel<kG, kFromSiteLik, kByteOff, kExt, kLem>: (kG, kFromSiteLik, kExt, kLem) -> vector registers before the change
# (kByteOff does not move the count)
PARENT_VGPR = {
    (1, False, False, False): 58, (1, False, True, False): 26, (1, True, False, False): 59, (1, True, False, True): 59,
    (1, True, True, False): 42, (1, True, True, True): 44,
    (2, False, False, False): 148, (2, False, True, False): 30, (2, True, False, False): 148, (2, True, False, True): 148,
    (2, True, True, False): 43, (2, True, True, True): 45,
    (4, False, False, False): 152, (4, False, True, False): 47, (4, True, False, False): 152, (4, True, False, True): 152,
    (4, True, True, False): 48, (4, True, True, True): 48,
}
MAX_SGPR = 80            # eight workgroups of four waves per CU


def kernel_registers(text):
    """{(kG, kFromSiteLik, kByteOff, kExt, kLem): (vgpr, sgpr, vgpr spills, sgpr spills)} from the metadata of a listing"""
    out = {}
    for name, body in re.findall(r"\.name:\s+(_ZN2lh15emission_kernel\w+)\n(.*?)\.wavefront_size", text, flags=re.S):
        m = re.search(r"emission_kernelILi(\d)ELb([01])ELb([01])ELb([01])ELb([01])E", name)
        assert m, name
        key = (int(m.group(1)),) + tuple(g == "1" for g in m.groups()[1:])
        field = lambda f: int(re.search(r"\.%s:\s+(\d+)" % f, body).group(1))
        out[key] = (field("vgpr_count"), field("sgpr_count"), field("vgpr_spill_count"), field("sgpr_spill_count"))
    return out


@pytest.fixture(scope="module")
def registers(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    out = str(tmp_path_factory.mktemp("k2a_registers") / "lh_forward.s")
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "-S",
                           "-I", os.path.join(ROOT, "include"), "-I", os.path.dirname(SRC), SRC, "-o", out],
                          stderr=subprocess.DEVNULL)
    got = kernel_registers(open(out).read())
    for key, c in sorted(got.items()):
        print("emission_kernel<%d,%s,%s,%s,%s>: vgpr %d, sgpr %d, spills %d + %d" % (key + c))
    return got


def test_every_instantiation_is_there(registers):
    assert {(k[0], k[1], k[3], k[4]) for k in registers} == set(PARENT_VGPR)
    assert {k[2] for k in registers} == {False, True}


def test_vector_registers_do_not_rise(registers):
    for key, (vgpr, _, vspill, _) in sorted(registers.items()):
        parent = PARENT_VGPR[(key[0], key[1], key[3], key[4])]
        assert vgpr <= parent, (key, vgpr, parent)
        assert vspill == 0, (key, vspill)


def test_scalar_registers_leave_eight_workgroups_per_cu(registers):
    for key, (_, sgpr, _, _) in sorted(registers.items()):
        assert sgpr <= MAX_SGPR, (key, sgpr)


def test_the_benchmarked_instantiation_keeps_eight_waves_per_simd(registers):
    """configs[2]: one gene slot per thread, emissions from K1's site likelihoods, byte offsets"""
    vgpr, sgpr, _, _ = registers[(1, True, True, False, False)]
    assert vgpr <= 64 and sgpr <= MAX_SGPR, (vgpr, sgpr)
