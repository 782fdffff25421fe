#!/usr/bin/env python3
"""Time one prediction fold (brr_session_predict_accumulate) at the C2 size.

A synthetic C2 training session (N = 100,000 x P = 500,000, 2-bit storage), a random .bed target of
N2 = 8,192 rows with an explicit value table, and the fold's two kernels timed by HIP events on the
session stream (brr_session_set_timing / brr_session_predict_timing), one fold at a time, in two
states: a BayesR state after 10 sweeps (sparse beta) and a dense beta set through set_vector.  The
median over --folds folds is reported beside the sweep time of the same session on the same device
and the dense fold's bytes/s (codes + value tables) against the measured HBM copy rate.

  python scripts/predict_measure.py [--N 100000] [--P 500000] [--N2 8192] [--folds 31] [--f32-target]

Prints one JSON line.  Needs an MI355X; there is no CPU path.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

HBM_COPY_TBS = 6.29  # measured float4 copy rate of the MI355X (79 % of the 8.0 TB/s specification)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=int, default=100_000)
    ap.add_argument("--P", type=int, default=500_000)
    ap.add_argument("--N2", type=int, default=8192)
    ap.add_argument("--folds", type=int, default=31)
    ap.add_argument("--sweeps", type=int, default=10)
    ap.add_argument("--f32-target", action="store_true", help="the target decoded and attached as dense f32")
    a = ap.parse_args()
    import numpy as np
    import bayesrrcpp_amd as B
    from bayesrrcpp_amd import _lib as L
    from bayesrrcpp_amd.predict import ReferencePredictor

    N, P, N2 = a.N, a.P, a.N2
    s = B.Session(L.MODEL_V2, N, P, K=4, x_storage=L.X_2BIT)
    s.synthesize(20261015, 0.5, -1)
    s.set_bayesr(sigma0=0.01, v0E=1e-4, s02E=1e-3, v0G=1e-4, s02G=1e-3, cva=[1e-4, 1e-3, 1e-2]).init(1)
    rng = np.random.default_rng(0)
    bed = rng.integers(0, 256, size=(P, (N2 + 3) // 4), dtype=np.uint8)
    table = rng.normal(size=(P, 4)).astype(np.float32)
    table[:, 1] = 0.0
    t0 = time.perf_counter()
    if a.f32_target:
        s.predict_upload_x(ReferencePredictor.decode_bed(bed, N2, table))
    else:
        s.predict_upload_bed(bed, N2, table=table)
    t_attach = time.perf_counter() - t0
    s.predict_set_y(rng.normal(size=N2))
    s.sweep(a.sweeps)
    s.synchronize()
    t0 = time.perf_counter()
    s.sweep(5)
    s.synchronize()
    sweep_ms = (time.perf_counter() - t0) / 5 * 1e3

    def folds():
        s.predict_begin()
        for _ in range(3):  # warm: code objects, the first touch of the target
            s.predict_accumulate()
        s.synchronize()
        s.set_timing(True)
        times, last = [], 0.0
        for _ in range(a.folds):
            s.predict_accumulate()
            t = s.predict_timing()["fold_ms"]
            times.append(t - last)
            last = t
        s.set_timing(False)
        s.predict_end()
        return float(np.median(times)), float(np.min(times)), float(np.max(times))

    nnz_sparse = int(np.count_nonzero(s.vector(L.BETA)))
    sparse = folds()
    # spot check of the device's score against the numpy specification on the first rows
    rows = min(N2, 4)
    want = ReferencePredictor(ReferencePredictor.decode_bed(bed[:, :1], rows, table)).score(s.vector(L.BETA))
    assert np.array_equal(s.predict_score()[:rows], want), "device score differs from the specification"
    s.set_vector(L.BETA, rng.normal(size=P) * 1e-3)
    dense = folds()
    gbytes = (P * ((N2 + 3) // 4) + 16 * P) if not a.f32_target else 4 * P * N2
    print(json.dumps({
        "N": N, "P": P, "N2": N2, "target_storage": "f32" if a.f32_target else "2bit", "attach_s": round(t_attach, 2),
        "sweep_ms": round(sweep_ms, 3), "nnz_sparse": nnz_sparse,
        "fold_ms_sparse": {"median": round(sparse[0], 4), "min": round(sparse[1], 4), "max": round(sparse[2], 4)},
        "fold_ms_dense": {"median": round(dense[0], 4), "min": round(dense[1], 4), "max": round(dense[2], 4)},
        "dense_genotype_bytes": gbytes, "dense_tb_per_s": round(gbytes / (dense[0] * 1e-3) / 1e12, 3),
        "dense_frac_of_copy_rate": round(gbytes / (dense[0] * 1e-3) / 1e12 / HBM_COPY_TBS, 3),
        "folds": a.folds}), flush=True)
    s.close()


if __name__ == "__main__":
    main()
