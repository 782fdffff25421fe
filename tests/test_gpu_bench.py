"""bench.py's plain run and --dump-outputs on a small cohort: the dumped state is the chain after
exactly warmup + steps sweeps (identical to a session driven here with the same arguments), the
result line carries ms_per_step, and what --full measures is absent from a plain run."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import CVA, HYP, REPO

pytestmark = pytest.mark.gpu
N, P, WARM, STEPS = 1000, 1300, 2, 3  # P: 10 full blocks of 128 and one of 20


@pytest.fixture(scope="module")
def bench_run(require_gpu, tmp_path_factory):
    out = tmp_path_factory.mktemp("bench") / "dump"
    r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--steps", str(STEPS),
                        "--warmup", str(WARM), "--config", "c1", "--N", str(N), "--P", str(P),
                        "--dump-outputs", str(out)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads(r.stdout.strip().splitlines()[-1]), out


def test_plain_result_line(bench_run):
    d, _ = bench_run
    assert d["steps"] == STEPS and d["warmup"] == WARM and d["n_gpus"] == 1
    assert d["unit"] == "sweeps/s" and d["higher_is_better"] is True and d["dtype"] == "f64"
    assert d["ms_per_step"] > 0
    # value = 1 / (s per step); ms_per_step is printed to 3 decimals, value to 4
    assert abs(d["value"] * d["ms_per_step"] / 1e3 - 1.0) < 0.0006 / d["ms_per_step"] + 1e-4
    assert d["roofline"] is None and d["cpu_baseline"] is None  # --full only
    assert d["config"]["census_failures"] == 0


def test_dump_is_the_chain_after_the_timed_steps(brr, bench_run):
    _, out = bench_run
    from bayesrrcpp_amd import _lib as L
    with brr.Session(L.MODEL_V2, N, P, K=len(CVA) + 1, block_size=128) as s:
        s.synthesize(20261015, 0.5, -1)
        s.set_bayesr(cva=CVA, **HYP)
        s.init(1)
        s.sweep(WARM + STEPS)
        want = s.state()
    assert sorted(os.listdir(out)) == sorted(f"{k}.npy" for k in want)
    for k, v in want.items():
        got = np.load(out / f"{k}.npy")
        assert got.dtype == np.float64
        assert np.array_equal(got, np.atleast_1d(v)), k
    assert np.load(out / "beta.npy").shape == (P,) and np.load(out / "eps.npy").shape == (N,)
    assert np.count_nonzero(np.load(out / "beta.npy")) > 0
