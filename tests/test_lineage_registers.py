"""The kernels along a seed's lineage (K3b, K11b, K12b, K13b, K14, K15b, K15; linearham_amd/csrc/lh_asr.hip, lh_ancestral.hip,
lh_substitutions.hip, lh_ancestral_probs.hip, lh_node_codon.hip, lh_codon_edges.hip) keep their register budget.

They share their tree pass (lh_treepass.h), and a step that moves into the shared header can cost one of them a wave per SIMD
without changing a bit of its output: K15b (cond_edge_kernel) lies at the edge of its tier and declares it.  This test
compiles the files to gfx950 assembly and reads the code objects' metadata, the way tests/test_k2b_dj_registers.py does for
K2b: every instantiation is there, every kernel stays under the vector-register ceiling of its tier (512 registers a SIMD,
allocated in eights: 128 for four waves, 168 for three, 256 for two, 64 for eight), nothing is spilled, no scratch.

cond_edge_kernel stands at 168, its ceiling: a compiler or a source change that costs it one more register fails this test,
which is meant -- the launcher and lh_codon_edges.hip's comments rely on three waves per SIMD."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "linearham_amd", "csrc")
SOURCES = ["lh_ancestral.hip", "lh_substitutions.hip", "lh_ancestral_probs.hip", "lh_codon_edges.hip", "lh_node_codon.hip",
           "lh_asr.hip"]
# kernel (its name in the mangled symbol, template arguments included) -> the VGPR ceiling of its tier
CEILING = {
    "10anc_kernelE": 128,
    "10asr_kernelE": 128,
    "10sub_kernelILb0EE": 168,
    "10sub_kernelILb1EE": 168,
    "11cond_kernelILi0EE": 168,
    "11cond_kernelILi1EE": 168,
    "11cond_kernelILi2EE": 168,
    "16cond_edge_kernelE": 168,
    "17codon_edge_kernelE": 256,
    "17node_codon_kernelE": 64,
}


def kernel_registers(text):
    """{mangled name: (vgpr, vgpr spills, sgpr spills, scratch bytes)} from the metadata of a listing"""
    out = {}
    for entry in re.split(r"\n  - \.agpr_count:", text[text.index("amdhsa.kernels:"):])[1:]:
        field = lambda f: int(re.search(r"\.%s:\s+(\d+)" % f, entry).group(1))
        name = re.search(r"\.name:\s+(\S+)", entry).group(1)
        out[name] = (field("vgpr_count"), field("vgpr_spill_count"), field("sgpr_spill_count"), field("private_segment_fixed_size"))
    return out


@pytest.fixture(scope="module")
def registers(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    tmp = tmp_path_factory.mktemp("lineage_registers")
    jobs = []
    for src in SOURCES:
        out = str(tmp / (src + ".s"))
        jobs.append((out, subprocess.Popen([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "-S",
                                            "-I", os.path.join(ROOT, "include"), "-I", CSRC, os.path.join(CSRC, src), "-o", out],
                                           stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, text=True)))
    got = {}
    for out, job in jobs:
        _, err = job.communicate()
        assert job.returncode == 0, "%s did not compile:\n%s" % (out, err)
        got.update(kernel_registers(open(out).read()))
    # the budgeted kernels, by the key of CEILING their symbol holds
    found = {}
    for name, counts in sorted(got.items()):
        for key in CEILING:
            if key in name:
                assert key not in found, name
                found[key] = counts
                print("%s: vgpr %d, spills %d + %d, scratch %d bytes" % ((key,) + counts))
    return got, found


def test_every_instantiation_is_there(registers):
    assert set(registers[1]) == set(CEILING)


def test_waves_per_simd(registers):
    for key, (vgpr, _, _, _) in sorted(registers[1].items()):
        assert vgpr <= CEILING[key], (key, vgpr)


def test_no_vgpr_spills_and_no_scratch(registers):
    # every kernel of the six files, the small ones included
    for name, (_, vspill, _, scratch) in sorted(registers[0].items()):
        assert vspill == 0 and scratch == 0, (name, vspill, scratch)
