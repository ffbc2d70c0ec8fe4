"""K2b's D-J kernels (junction_dj4_kernel: four samples per wave; junction_dj_kernel: two;
linearham_amd/csrc/lh_forward.hip) keep their register budget.

The launcher sizes the four-sample kernel's workgroups (dj4_waves) on the footing that both kernels hold four waves per SIMD
by registers: at most 128 vector registers, nothing spilled, no scratch.  This test compiles the file to gfx950 assembly and
reads the code object's metadata, the way tests/test_k2a_registers.py does for K2a: junction_dj4_kernel for both left-gene
slot counts (GL = 1: at most 16 D alleles; GL = 2: at most 32), and both kernels in both range modes."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "linearham_amd", "csrc", "lh_forward.hip")
MAX_VGPR = 128           # four waves per SIMD


def _counts(body):
    field = lambda f: int(re.search(r"\.%s:\s+(\d+)" % f, body).group(1))
    return (field("vgpr_count"), field("vgpr_spill_count"), field("sgpr_spill_count"), field("private_segment_fixed_size"))


def kernel_registers(text):
    """{(GL, kExt): (vgpr, vgpr spills, sgpr spills, scratch bytes)} from the metadata of a listing"""
    out = {}
    for name, body in re.findall(r"\.name:\s+(_ZN2lh19junction_dj4_kernel\w+)\n(.*?)\.wavefront_size", text, flags=re.S):
        m = re.search(r"junction_dj4_kernelILi(\d)ELb([01])E", name)
        assert m, name
        out[(int(m.group(1)), m.group(2) == "1")] = _counts(body)
    return out


def pair_kernel_registers(text):
    """{kExt: (vgpr, vgpr spills, sgpr spills, scratch bytes)} of junction_dj_kernel"""
    out = {}
    for name, body in re.findall(r"\.name:\s+(_ZN2lh18junction_dj_kernel\w+)\n(.*?)\.wavefront_size", text, flags=re.S):
        m = re.search(r"junction_dj_kernelILb([01])E", name)
        assert m, name
        out[m.group(1) == "1"] = _counts(body)
    return out


@pytest.fixture(scope="module")
def listing(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    out = str(tmp_path_factory.mktemp("k2b_dj_registers") / "lh_forward.s")
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "-S",
                           "-I", os.path.join(ROOT, "include"), "-I", os.path.dirname(SRC), SRC, "-o", out],
                          stderr=subprocess.DEVNULL)
    return open(out).read()


@pytest.fixture(scope="module")
def registers(listing):
    got = kernel_registers(listing)
    for key, c in sorted(got.items()):
        print("junction_dj4_kernel<%d,%s>: vgpr %d, spills %d + %d, scratch %d bytes" % (key + c))
    return got


@pytest.fixture(scope="module")
def pair_registers(listing):
    got = pair_kernel_registers(listing)
    for key, c in sorted(got.items()):
        print("junction_dj_kernel<%s>: vgpr %d, spills %d + %d, scratch %d bytes" % ((key,) + c))
    return got


def test_every_instantiation_is_there(registers):
    assert set(registers) == {(1, False), (1, True), (2, False), (2, True)}


def test_four_waves_per_simd_and_no_scratch(registers):
    for key, (vgpr, vspill, sspill, scratch) in sorted(registers.items()):
        assert vgpr <= MAX_VGPR, (key, vgpr)
        assert vspill == 0 and sspill == 0 and scratch == 0, (key, vspill, sspill, scratch)


def test_pair_kernel_four_waves_per_simd_and_no_scratch(pair_registers):
    assert set(pair_registers) == {False, True}
    for key, (vgpr, vspill, sspill, scratch) in sorted(pair_registers.items()):
        assert vgpr <= MAX_VGPR, (key, vgpr)
        assert vspill == 0 and sspill == 0 and scratch == 0, (key, vspill, sspill, scratch)
