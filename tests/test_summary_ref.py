"""CPU tests of the posterior summaries: ReferenceSummary (bayesrrcpp_amd/summary.py, the executable
specification of the device accumulator) against direct numpy over the stacked samples, over a short
oracle chain, and the brr_session_summary_* C ABI without a device."""
import ctypes as C

import numpy as np
import pytest

from conftest import CVA, HYP

S, M, N, K, G = 7, 37, 29, 4, 3


def _rel(a, b):
    a, b = np.asarray(a, float), np.asarray(b, float)
    return float(np.max(np.abs(a - b) / np.maximum(np.abs(b), np.max(np.abs(b)) * 1e-3 + 1e-300))) if a.size else 0.0


def _samples(seed=5):
    rng = np.random.default_rng(seed)
    comp = rng.integers(0, K, size=(S, M))
    beta = rng.normal(size=(S, M)) * (comp > 0)
    beta[3] = 0.0  # a sweep with an empty model: every window's share is 0 there
    comp[3] = 0
    eps = rng.normal(size=(S, N))
    mu = rng.normal(size=S)
    alpha = rng.normal(size=(S, 2))
    sigmaE = rng.uniform(0.5, 1.5, size=S)
    Y = rng.normal(size=N)
    fixed = rng.normal(size=(N, 2))
    gA = rng.integers(0, G, size=M)
    return dict(comp=comp, beta=beta, eps=eps, mu=mu, alpha=alpha, sigmaE=sigmaE, Y=Y, fixed=fixed, gA=gA)


@pytest.mark.parametrize("W", [5, 1])
def test_reference_summary_against_direct_numpy(W):
    from bayesrrcpp_amd import _lib as L
    from bayesrrcpp_amd.summary import ReferenceSummary
    d = _samples()
    r = ReferenceSummary(M, N, K=K, G=G, gAssign=d["gA"], Y=d["Y"], fixed=d["fixed"], window=W)
    for s in range(S):
        r.add(10 + s, d["beta"][s], d["comp"][s], d["eps"][s], d["mu"][s], d["alpha"][s], sigmaE=d["sigmaE"][s])
    beta, comp = d["beta"], d["comp"]
    assert _rel(r.get(L.SUM_BETA_MEAN), beta.mean(axis=0)) < 1e-13
    assert _rel(r.get(L.SUM_BETA_M2) / (S - 1), beta.var(axis=0, ddof=1)) < 1e-13
    assert _rel(r.get(L.SUM_BETA_SD), beta.std(axis=0, ddof=1)) < 1e-13
    # class frequencies and PIPs: exact
    cnt = np.stack([(comp == k).sum(axis=0) for k in range(K)], axis=1)
    assert np.array_equal(r.get(L.SUM_COMP_COUNT), cnt)
    assert np.array_equal(r.get(L.SUM_COMP_FREQ), cnt / S)
    assert np.array_equal(r.get(L.SUM_PIP), 1.0 - cnt[:, 0] / S)
    # genetic values
    g = (d["Y"][None, :] - d["mu"][:, None]) - d["eps"] - d["alpha"] @ d["fixed"].T
    assert _rel(r.get(L.SUM_G_MEAN), g.mean(axis=0)) < 1e-13
    assert _rel(r.get(L.SUM_G_M2) / (S - 1), g.var(axis=0, ddof=1)) < 1e-13
    # windows of W consecutive markers (the last one shorter: 37 = 7 * 5 + 2)
    nW = -(-M // W)
    assert r.get(L.SUM_WINDOW_COUNT).shape == (nW,)
    b2 = beta * beta
    ssq = np.stack([b2[:, w * W:(w + 1) * W].sum(axis=1) for w in range(nW)], axis=1)
    wany = np.stack([(comp[:, w * W:(w + 1) * W] > 0).any(axis=1) for w in range(nW)], axis=1)
    tot = b2.sum(axis=1)
    share = np.where(tot[:, None] > 0, ssq / np.where(tot > 0, tot, 1.0)[:, None], 0.0)
    assert np.array_equal(r.get(L.SUM_WINDOW_COUNT), wany.sum(axis=0))
    assert np.array_equal(r.get(L.SUM_WINDOW_PIP), wany.sum(axis=0) / S)
    assert _rel(r.get(L.SUM_WINDOW_SSQ), ssq.mean(axis=0)) < 1e-13
    assert _rel(r.get(L.SUM_WINDOW_SHARE), share.mean(axis=0)) < 1e-13
    if W == 1:  # a window per marker: the same counts (PIP = 1 - c0 / n rounds differently from c / n at n = 7)
        assert np.array_equal(r.get(L.SUM_WINDOW_COUNT), S - cnt[:, 0])
        assert np.max(np.abs(r.get(L.SUM_WINDOW_PIP) - r.get(L.SUM_PIP))) < 1e-15
    # trace: header, var_g / h2, counts and sums of squares per (group, class)
    tr = r.get(L.SUM_TRACE)
    assert tr.shape == (S, 12 + 2 * G * K)
    assert np.array_equal(tr[:, 0], 10 + np.arange(S))
    var_g = g.var(axis=1, ddof=1)
    assert _rel(tr[:, 9], var_g) < 1e-13
    assert _rel(tr[:, 10], var_g / (var_g + d["sigmaE"])) < 1e-13
    assert np.array_equal(tr[:, 11], (comp > 0).sum(axis=1))
    for gg in range(G):
        for k in range(K):
            sel = (d["gA"][None, :] == gg) & (comp == k)
            assert np.array_equal(tr[:, 12 + gg * K + k], sel.sum(axis=1))
            assert _rel(tr[:, 12 + G * K + gg * K + k], (b2 * sel).sum(axis=1)) < 1e-13
    assert np.array_equal(tr[:, 12:12 + G * K].sum(axis=1), np.full(S, M))
    assert set(r.posterior()) == set(L.SUM_NAMES)


def test_reference_summary_horseshoe_and_item_errors():
    from bayesrrcpp_amd import _lib as L
    from bayesrrcpp_amd.summary import ReferenceSummary
    d = _samples()
    r = ReferenceSummary(M, N, horseshoe=True, Y=d["Y"])
    for s in range(S):
        r.add(s, d["beta"][s], None, d["eps"][s], d["mu"][s], sigmaE=1.0)
    tr = r.get(L.SUM_TRACE)
    assert tr.shape == (S, 14)
    assert np.array_equal(tr[:, 12], np.full(S, M)) and np.array_equal(tr[:, 11], (d["beta"] != 0).sum(axis=1))
    assert _rel(tr[:, 13], (d["beta"] ** 2).sum(axis=1)) < 1e-13
    with pytest.raises(ValueError):
        r.get(L.SUM_PIP)
    with pytest.raises(ValueError):
        r.get(L.SUM_WINDOW_PIP)
    assert "pip" not in r.posterior() and "window_pip" not in r.posterior()
    one = ReferenceSummary(M, N, K=K).add(0, d["beta"][0], d["comp"][0], d["eps"][0], 0.0)
    assert not one.get(L.SUM_BETA_SD).any()  # SD is 0 below two kept sweeps


def test_reference_summary_of_an_oracle_chain(oracle_mod):
    from bayesrrcpp_amd import _lib as L
    from bayesrrcpp_amd.summary import ReferenceSummary
    O = oracle_mod
    n, p = 120, 90
    X, Y, _ = O.synth_cohort(20261015, n, p, h2=0.5, n_causal=9)
    orc = O.Oracle(O.V2, X, Y, cva=CVA, seed=3, order_mode=O.ORDER_BLOCKED, block_size=64, **HYP)
    r = ReferenceSummary(p, n, K=4, Y=Y, window=8)
    kept = []
    for it in range(10):
        orc.sweep(1)
        if it >= 2 and it % 2 == 0:
            r.add_chain(it, orc)
            kept.append(it)
    assert kept == [2, 4, 6, 8] and r.n == 4
    pip, freq, tr = r.get(L.SUM_PIP), r.get(L.SUM_COMP_FREQ), r.get(L.SUM_TRACE)
    assert ((pip >= 0) & (pip <= 1)).all()
    assert np.array_equal(freq.sum(axis=1), np.ones(p))
    assert np.array_equal(tr[:, 12:16].sum(axis=1), np.full(4, p))
    assert np.array_equal(tr[:, 0], kept)
    # g = Y - mu - eps is the fitted X beta: the chain explains part of Y's unit variance
    assert ((tr[:, 10] > 0) & (tr[:, 10] < 1)).all()
    wp = r.get(L.SUM_WINDOW_PIP)
    assert wp.shape == (12,) and ((wp >= 0) & (wp <= 1)).all()
    assert abs(r.get(L.SUM_WINDOW_SHARE).sum() - 1.0) < 1e-12


def test_summary_abi_without_a_device(brr):
    from bayesrrcpp_amd import _lib
    assert _lib.ABI_VERSION == 4
    lib = brr.lib()
    new = [s for s in _lib.EXPORTED if s.startswith("brr_session_summary_")]
    assert len(new) == 8
    for name in new:
        assert getattr(lib, name) is not None
    out = np.zeros(4)
    calls = {
        "begin": lambda: lib.brr_session_summary_begin(None, 0),
        "accumulate": lambda: lib.brr_session_summary_accumulate(None),
        "run": lambda: lib.brr_session_summary_run(None, 10, 2, 1),
        "count": lambda: lib.brr_session_summary_count(None),
        "trace_width": lambda: lib.brr_session_summary_trace_width(None),
        "get": lambda: lib.brr_session_summary_get(None, _lib.SUM_BETA_MEAN, out.ctypes.data_as(_lib.D)),
        "get_size": lambda: lib.brr_session_summary_get(None, _lib.SUM_TRACE, None),
        "write": lambda: lib.brr_session_summary_write(None, b"/nonexistent/prefix"),
        "end": lambda: lib.brr_session_summary_end(None),
    }
    for name, call in calls.items():
        rc = call()
        assert rc < 0, name
        assert _lib.last_error() == f"summary_{name.replace('_size', '')}: null session", name
    assert not out.any()
    assert C.sizeof(C.c_int64) == 8 and lib.brr_session_summary_get.restype is C.c_int64
