"""lh_eval_codons_batch across its launch-group boundaries: tests/test_gpu_batch_boundaries.py's scheme.

1. Anchor: 23 distinct tree samples as one 23-row call, windows and genes checked against tests/codon_oracle.py.
2. Position independence: in a large call row i is anchor row (7 i + i // G) % 23 and carries that row's bits in every
   per-row output; the weighted sums and weight_stats against a long-double host sum of the call's own rows.  The groups are
   shrunk with the hooks the other module uses (LH_CHUNK, LH_HOST_SUB), read once per process: one child per case."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import batch_boundaries_worker as bw
from tests import codon_boundaries_worker as cw

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOOKS = {"LH_HOST_SUB": "1536", "LH_CHUNK": "1024"}
SLABS = "2053,2304,2305"     # 2 x 1024 + 5, 2048 + 256 (group and slab edges coincide), 2048 + 257


@pytest.fixture(scope="module")
def work(tmp_path_factory):
    import linearham_amd
    assert linearham_amd.load_library().device_count() >= 1, "no HIP device visible: the GPU tests need an MI355X"
    d = str(tmp_path_factory.mktemp("codon_boundaries"))
    return d, cw.build_anchors(d)


def test_anchor_rows_match_the_oracle(work):
    from linearham_amd import posterior as lp
    from tests import codon_oracle as co
    from tests.test_gpu_posterior import BOUND
    d, (A, lay) = work
    F = bw.Fam(d, "igh")
    o = F.o
    assert len({r["tree"] for r in F.rows}) == bw.N_SETS
    for i, s in enumerate(F.rows):
        o.initialize_phylo_parameters(s["tree"], s["er"], s["pi"], s["alpha"], 4, is_path=False)
        o.initialize_phylo_emission()
        ll = o.log_likelihood()
        assert abs(A["loglik"][i] - ll) <= 1e-12 * abs(ll)
        table, post = co.dense(o, cw.FRAME)
        w, g, olay = co.window_inputs(o, table, post, cw.FRAME)
        assert olay == lay
        assert np.max(np.abs(A["windows"][i] - w)) < BOUND and np.max(np.abs(A["genes"][i] - g)) < BOUND, i
    assert len({float(x) for x in A["loglik"]}) == bw.N_SETS
    F.close()


@pytest.mark.parametrize("extra", [{}, {"LH_CODON_BLOCKS": "8"}], ids=["groups-and-slabs", "capped-grid"])
def test_codons_batch_across_groups_and_slabs(work, extra):
    """capped-grid: K9's workgroup cap (2048 in the product) lowered to 8, i.e. 128 sample slots, so that every group of
    lanes walks eight or more samples of a 1024-row launch group over the same scratch vectors."""
    e = {k: v for k, v in os.environ.items() if k not in HOOKS and k != "LH_CODON_BLOCKS"}
    e.update(HOOKS)
    e.update(extra)
    r = subprocess.run([sys.executable, "-m", "tests.codon_boundaries_worker", "codons", work[0], "ns=" + SLABS, "G=1024"],
                       cwd=ROOT, env=e, capture_output=True, text=True, timeout=180)
    assert r.returncode == 0, "worker exited %d\n" % r.returncode + r.stdout[-2000:] + r.stderr[-3000:]
    res = json.loads(r.stdout.strip().splitlines()[-1])
    print(json.dumps(res["info"]))
    assert res["failures"] == [], "\n".join(res["failures"])
