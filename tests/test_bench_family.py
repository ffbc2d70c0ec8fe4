"""bench.py generates its synthetic family with the rows of the tree table built by several processes; the files must
be those tools/synth_family.generate() writes, byte for byte, or the benchmark would measure other inputs."""
import os

import pytest

import bench
from tools import synth_family as sf


def _files(d):
    out = {}
    for root, _, names in os.walk(d):
        for name in names:
            p = os.path.join(root, name)
            with open(p, "rb") as f:
                out[os.path.relpath(p, d)] = f.read()
    return out


@pytest.mark.parametrize("spec,workers", [
    (sf.Spec(n_samples=601), 3),                                       # configs[2] shape, an uneven last chunk
    (sf.Spec.small(n_samples=97, ragged=4, ambiguous=0.02), 2),        # N inside columns
    (sf.Spec(n_leaves=40, n_samples=200, tree_shape="balanced", brlen_mean=0.002, n_nni=6), 4),
], ids=["config2", "small_ragged", "balanced"])
def test_parallel_family_is_generate_byte_for_byte(tmp_path, spec, workers):
    sf.generate(spec, str(tmp_path / "serial"))
    bench.generate_family(spec, str(tmp_path / "parallel"), workers)
    want, got = _files(tmp_path / "serial"), _files(tmp_path / "parallel")
    assert sorted(got) == sorted(want)
    for name in want:
        assert got[name] == want[name], name
