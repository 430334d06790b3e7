"""The branch of the shared Arnoldi step that one GPU never takes by itself: k_reduce_partials + the all-reduce of the slots + k_givens
(csrc/knp_krylov.inc, arnoldi_step_finish), which distributed runs use and KNP_FIN=0 forces on one GPU, against the default single-block
k_reduce_fin.  Same algorithm, other summation order of the partial sums: the same iteration counts and read-backs, and the fields
agree to 1e-10 of their max norm after 3 steps at rtol 1e-10 (the bound of test_gpu_fused_reductions.py and
test_gpu_fgmres.py::test_fold_equivalence for exactly this kind of difference).  With KNP_FIN=0 no first stage may be folded into a
neighbouring kernel (k_reduce_partials takes no row stride): both fold counters stay 0, which shows that the other branch ran.

The switch is read once per process, so each leg is a fresh interpreter that runs all four cases; the legs run one after the other
and the second is not started when the first ends abnormally.

Largest |x(KNP_FIN=0) - x(default)| / max|x(default)| over the four fields, measured on MI355X before the two drivers shared their core:
square 32x32 hypre: gmres 5.3e-12, fgmres 5.7e-12; cube 8^3 btcc: gmres 0 (bit for bit), fgmres 5.8e-13."""
from __future__ import annotations

import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEFT = {"ksp_type": "gmres", "norm_type": "preconditioned"}
FLEX = {"ksp_type": "fgmres", "norm_type": "unpreconditioned"}
# the smallest shapes at which both reduction paths and both cycle lengths (up to 8 vectors, and longer) occur
CASES = {
    "square32-hypre-gmres": (32, "square", "hypre", LEFT),
    "square32-hypre-fgmres": (32, "square", "hypre", FLEX),
    "cube8-btcc-gmres": (8, "cube", "btcc", LEFT),
    "cube8-btcc-fgmres": (8, "cube", "btcc", FLEX),
}
CHILD = """
import sys; sys.path[:0] = ['tests', 'oracle', 'knp-emi-cgx_amd']; import conftest, json, numpy as np
from parity_utils import ci_config, run_native
cases, path = json.loads(sys.argv[1]), sys.argv[2]
meta, xs = {}, {}
for name, (N, kind, pc, ksp) in cases.items():
    c = ci_config(N=N, steps=3, rtol=1e-10, kind=kind, pc=pc)
    c['solver']['ksp_settings'].update(ksp)
    s = run_native(c)
    xs[name] = s.backend.x.cpu().numpy()
    meta[name] = {'its': list(s.iterations), 'stats': s.backend.stats(), 'flexible': bool(s._flexible)}
np.savez(path, **xs)
print('RESULT' + json.dumps(meta))
"""


def _leg(path, env_extra):
    env = {k: v for k, v in os.environ.items() if k != "KNP_FIN"}
    out = subprocess.run([sys.executable, "-c", CHILD, json.dumps(CASES), path], cwd=ROOT, env=dict(env, **env_extra),
                         capture_output=True, text=True, timeout=300)
    line = [ln for ln in out.stdout.splitlines() if ln.startswith("RESULT")]
    assert out.returncode == 0 and line, f"exit status {out.returncode}\n" + out.stdout[-2000:] + out.stderr[-2000:]
    return json.loads(line[0][6:]), dict(np.load(path))


@pytest.fixture(scope="module")
def legs(tmp_path_factory):
    d = tmp_path_factory.mktemp("krylov_paths")
    fin = _leg(str(d / "fin.npz"), {})
    nofin = _leg(str(d / "nofin.npz"), {"KNP_FIN": "0"})
    return fin, nofin


@pytest.mark.parametrize("name", list(CASES))
def test_allreduce_branch_matches_the_single_block_finish(legs, name):
    (m1, x1), (m0, x0) = legs
    a, b = m1[name], m0[name]
    x1, x0 = x1[name], x0[name]
    ratios = [float(np.max(np.abs(x0[f::4] - x1[f::4])) / np.max(np.abs(x1[f::4]))) for f in range(4)]
    print(name, "its", a["its"], b["its"], "stats", a["stats"], b["stats"], "ratios", ratios)
    assert a["flexible"] == b["flexible"] == (CASES[name][3] is FLEX)
    assert len(a["its"]) == 3 and a["its"] == b["its"]
    assert a["stats"]["readbacks"] == b["stats"]["readbacks"]
    assert b["stats"]["spmv_dots"] == 0 and b["stats"]["fused_dots"] == 0, b["stats"]
    assert not a["flexible"] or a["stats"]["spmv_dots"] > 0, a["stats"]   # the default leg did take the single-block finish
    assert max(ratios) <= 1e-10, ratios
