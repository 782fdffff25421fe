"""CPU tests of ReferencePredictor (bayesrrcpp_amd/predict.py), the numpy specification of the
device's out-of-sample prediction: the score against exact rational arithmetic, the .bed decode
against a per-code computation, and the Welford / trace definitions against numpy's own moments."""
from fractions import Fraction

import numpy as np
import pytest

from bayesrrcpp_amd import _lib as L
from bayesrrcpp_amd.predict import ReferencePredictor

C = L.PREDICT_CHUNK


def _bed(rng, n_rows, n_markers, extra_bytes=0):
    """Random .bed body with missing codes; every bit of the last byte (rows >= n_rows) and of the
    extra bytes is random too."""
    return rng.integers(0, 256, size=(n_markers, (n_rows + 3) // 4 + extra_bytes), dtype=np.uint8)


@pytest.mark.parametrize("kind", ["dense", "sparse", "zero"])
def test_score_against_exact_sums(kind):
    """One rounding per product and one per add: the score of a row is within
    nnz * 2^-52 * sum_j |x_ij b_j| of the exact sum (formed in rational arithmetic).  M = C + 77 spans
    two chunks, so the chunk fold is part of it."""
    rng = np.random.default_rng(11)
    n2, m = 5, C + 77
    X = rng.normal(size=(n2, m)).astype(np.float32)
    beta = np.zeros(m)
    if kind == "dense":
        beta = rng.normal(size=m) * 0.01
    elif kind == "sparse":
        idx = np.array([0, 5, C - 1, C, m - 1])
        beta[idx] = rng.normal(size=idx.size)
        beta[7] = -0.0
    g = ReferencePredictor(X).score(beta)
    nnz = int(np.count_nonzero(beta))
    assert nnz == {"dense": m, "sparse": 5, "zero": 0}[kind]
    for i in range(n2):
        exact = sum((Fraction(float(X[i, j])) * Fraction(float(beta[j])) for j in np.flatnonzero(beta)), Fraction(0))
        mag = sum((abs(Fraction(float(X[i, j])) * Fraction(float(beta[j]))) for j in np.flatnonzero(beta)), Fraction(0))
        bound = nnz * Fraction(1, 2 ** 52) * mag
        assert abs(Fraction(float(g[i])) - exact) <= bound, f"{kind} row {i}"
    if kind == "zero":
        assert np.array_equal(g, np.zeros(n2)) and not np.signbit(g).any()


def test_score_order_is_chunked():
    """The specification's order, restated with python floats: chunk sums from 0, ascending markers,
    zeros skipped, chunk sums added to 0 in order."""
    rng = np.random.default_rng(12)
    n2, m = 3, 2 * C + 9
    X = rng.normal(size=(n2, m)).astype(np.float32)
    beta = rng.normal(size=m)
    beta[rng.random(m) < 0.5] = 0.0
    g = ReferencePredictor(X).score(beta)
    for i in range(n2):
        tot = 0.0
        for c0 in range(0, m, C):
            acc = 0.0
            for j in range(c0, min(c0 + C, m)):
                if beta[j] != 0.0:
                    acc = acc + float(X[i, j]) * float(beta[j])
            tot = tot + acc
        assert tot == g[i]


def test_bed_decode_and_training_table():
    rng = np.random.default_rng(13)
    n, n2, m = 23, 9, 12  # neither a multiple of 4: the last bytes carry random padding bits
    table = rng.normal(size=(m, 4)).astype(np.float32)
    bed = _bed(rng, n2, m, extra_bytes=2)
    X = ReferencePredictor.decode_bed(bed, n2, table)
    assert X.shape == (n2, m) and X.dtype == np.float32
    codes_seen = set()
    for j in range(m):
        for i in range(n2):
            code = (int(bed[j, i // 4]) >> (2 * (i % 4))) & 3
            codes_seen.add(code)
            assert X[i, j] == table[j, code]
    assert codes_seen == {0, 1, 2, 3}  # missing genotypes included
    # other padding bits, same decode
    bed2 = bed.copy()
    bed2[:, (n2 + 3) // 4 - 1] ^= np.uint8(0xFF & ~((1 << (2 * (n2 % 4))) - 1))
    bed2[:, (n2 + 3) // 4:] ^= np.uint8(0xFF)
    assert np.array_equal(ReferencePredictor.decode_bed(bed2, n2, table), X)
    # the training table: scale() after mean imputation, missing -> 0, a monomorphic column all 0
    tb = _bed(rng, n, m)
    tb[3] = 0xFF  # every sample 11: no variation
    t = ReferencePredictor.training_table(tb, n)
    assert t.shape == (m, 4) and t.dtype == np.float32
    geno = np.array([2.0, np.nan, 1.0, 0.0])
    for j in range(m):
        g = np.array([geno[(int(tb[j, i // 4]) >> (2 * (i % 4))) & 3] for i in range(n)])
        obs = ~np.isnan(g)
        if j == 3:
            assert not t[j].any()
            continue
        mean = g[obs].mean()
        sd = np.sqrt(np.sum((g[obs] - mean) ** 2) / (n - 1))
        want = (np.array([2.0, 0.0, 1.0, 0.0]) - mean) / sd
        want[1] = 0.0
        assert np.allclose(t[j], want, rtol=1e-6, atol=0)
    Xt = ReferencePredictor.decode_bed(tb, n, t)
    assert np.all(np.abs(Xt.sum(axis=0)) < 1e-4)  # mean-imputed columns are centred
    with pytest.raises(ValueError):
        ReferencePredictor.decode_bed(bed, n2, table, bytes_per_col=1)


def _folded(n2, with_y=True, sweeps=5, seed=14):
    rng = np.random.default_rng(seed)
    m = 40
    X = rng.normal(size=(n2, m)).astype(np.float32)
    Y = rng.normal(size=n2) if with_y else None
    ref = ReferencePredictor(X, Y)
    gs, mus = [], []
    for it in range(sweeps):
        beta = rng.normal(size=m) * (rng.random(m) < 0.3)
        mu = rng.normal()
        ref.add(10 + 2 * it, beta, mu)
        gs.append(ref.score(beta))
        mus.append(mu)
    return ref, np.array(gs), np.array(mus), Y


def _close(a, b, tol=1e-12):
    a, b = np.asarray(a, float), np.asarray(b, float)
    return np.all(np.abs(a - b) <= tol * np.maximum(1.0, np.abs(b)))


def test_welford_and_trace_against_numpy():
    ref, gs, mus, Y = _folded(37)
    assert _close(ref.get(L.PRED_G_MEAN), gs.mean(axis=0))
    assert _close(ref.get(L.PRED_G_SD), gs.std(axis=0, ddof=1))
    assert _close(ref.get(L.PRED_G_M2), gs.var(axis=0, ddof=1) * (len(gs) - 1))
    tr = ref.get(L.PRED_TRACE)
    assert tr.shape == (5, 8) and len(L.PRED_TRACE_HEADER) == 8
    assert np.array_equal(tr[:, 0], 10 + 2 * np.arange(5))
    for k, g in enumerate(gs):
        want = [g.mean(), g.var(ddof=1), Y.mean(), Y.var(ddof=1), np.cov(Y, g, ddof=1)[0, 1],
                np.corrcoef(Y, g)[0, 1], np.mean((Y - mus[k] - g) ** 2)]
        assert _close(tr[k, 1:], want), (k, tr[k, 1:], want)
    assert set(ref.posterior()) == set(L.PRED_NAMES)


def test_trace_without_y_and_single_row():
    ref, gs, _, _ = _folded(37, with_y=False)
    tr = ref.get(L.PRED_TRACE)
    assert _close(tr[:, 1], gs.mean(axis=1)) and _close(tr[:, 2], gs.var(axis=1, ddof=1))
    assert np.isnan(tr[:, 3:]).all()
    # N2 = 1: variances and covariance 0 (no division by zero), cor 0, mse the one squared residual
    ref, gs, mus, Y = _folded(1)
    tr = ref.get(L.PRED_TRACE)
    assert np.isfinite(tr).all()
    assert np.array_equal(tr[:, 1], gs[:, 0]) and np.array_equal(tr[:, 3], np.full(5, Y[0]))
    assert not tr[:, [2, 4, 5, 6]].any()
    assert _close(tr[:, 7], (Y[0] - mus - gs[:, 0]) ** 2)
    # one kept sweep: SD 0
    one = ReferencePredictor(np.ones((3, 2), dtype=np.float32)).add(0, [1.0, 2.0], 0.0)
    assert np.array_equal(one.get(L.PRED_G_SD), np.zeros(3)) and np.array_equal(one.get(L.PRED_G_MEAN), np.full(3, 3.0))
