"""GPU tests of the posterior summaries (brr_session_summary_*, csrc/brr_summary.hpp): the device
accumulator against ReferenceSummary (bayesrrcpp_amd/summary.py) fed from the CPU oracle and from a
second GPU session, the window forms, determinism / reset / refusals, and the one-shots'
BRR_SUMMARY_PREFIX files.

Shape: N = 257 rows (no multiple of 4, 64 or 256), P = 333 markers (no multiple of the block, of 256
or of the window: two k_summary_markers workgroups, the second with 77 markers), B = 64; 12
iterations, burn-in 3, thinning 2: iterations 4, 6, 8 and 10 are kept.  Cohort seed 20261015,
n_causal = 20 (the M2 filter of test_against_oracle covers >= 90 % of the entries there: see
_m2_check; measured with the oracle alone before the first GPU run).
"""
import numpy as np
import pytest

from conftest import CVA, HYP

pytestmark = pytest.mark.gpu

RTOL = 1e-9
N, P, B = 257, 333, 64
N_CAUSAL = 20
ITER, BURN, THIN = 12, 3, 2
KEPT = [4, 6, 8, 10]
WINDOW = 10
CVA5 = np.array([1e-4, 1e-3, 3e-3, 1e-2])  # K = 5
HS = dict(A=(1 / np.sqrt(N)) * 150 / (P - 150), v0E=1e-3, s02E=1e-3, vL=1.0, vT=1.0, c2=1.0, vC=10.0, sC=10.0)


def _cohort(O, n=N, p=P, seed=20261015, n_causal=N_CAUSAL):
    X, Y, _ = O.synth_cohort(seed, n, p, h2=0.5, n_causal=n_causal)
    return X, Y


def _rel(a, b):
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    nf = ~np.isfinite(b)
    if nf.any():  # degenerate draws (sigmaG = inf): the same non-finite value on both sides
        if not np.array_equal(a[nf], b[nf], equal_nan=True):
            return float("inf")
        a, b = a[~nf], b[~nf]
        if not a.size:
            return 0.0
    scale = np.maximum(np.abs(b), np.max(np.abs(b)) * 1e-3 + 1e-300)
    return float(np.max(np.abs(a - b) / scale)) if a.size else 0.0


def _keep(it):
    return it >= BURN and it % THIN == 0


def _make(brr, O, model, X, Y, G=1, gAssign=None, fixed=None, cva=CVA, seed=7, restart=None, hs=None,
          xs="f32", oracle=True):
    """A session and (oracle=True) the CPU oracle on the same inputs, seed and visit order."""
    from bayesrrcpp_amd import _lib as L
    n, p = X.shape
    K = 1 if model == L.MODEL_HORSESHOE else np.atleast_2d(cva).shape[-1] + 1
    F = 0 if fixed is None else np.asarray(fixed).reshape(n, -1).shape[1]
    s = brr.Session(model, n, p, K=K, groups=G, F=F, block_size=B, order_mode=L.ORDER_BLOCKED,
                    x_storage=L.X_2BIT if xs == "2bit" else L.X_F32)
    s.upload_x(X)
    okw = {}
    if model != L.MODEL_RESTART:
        s.set_y(Y)
    if model == L.MODEL_HORSESHOE:
        s.set_horseshoe(**hs)
        okw.update(hs)
    else:
        cva2 = np.tile(np.asarray(cva, float), (G, 1)) if np.ndim(cva) == 1 else np.asarray(cva)
        s.set_bayesr(HYP["sigma0"], HYP["v0E"], HYP["s02E"], HYP["v0G"], HYP["s02G"], cva2, gAssign)
        okw.update(HYP)
        okw.update(cva=cva2, G=G)
        if gAssign is not None:
            okw["gAssign"] = gAssign
    if fixed is not None:
        s.set_fixed(fixed)
        okw["fixed"] = fixed
    if restart is not None:
        s.set_restart(restart["mu0"], restart["beta0"], restart["sigmaE0"], restart["sigmaGG0"],
                      restart["eps0"], restart["comp0"])
        okw.update(restart)
    s.init(seed)
    orc = None
    if oracle:
        orc = O.Oracle(model, X, None if model == L.MODEL_RESTART else Y, seed=seed, order_mode=O.ORDER_BLOCKED,
                       block_size=B, N=n, **okw)
    return s, orc


def _case(O, name):
    """model, _make's keywords and ReferenceSummary's keywords of a test_against_oracle case"""
    from bayesrrcpp_amd import _lib as L
    X, Y = _cohort(O)
    if name in ("v2", "v2-2bit"):
        return L.MODEL_V2, X, Y, dict(xs="2bit" if name == "v2-2bit" else "f32"), dict(K=4, Y=Y)
    if name == "horseshoe":
        return L.MODEL_HORSESHOE, X, Y, dict(hs=HS), dict(horseshoe=True, Y=Y)
    G = 3
    if name == "groups":
        gA = (np.arange(P) * G // P).astype(np.int32)
        fixed = np.random.default_rng(3).normal(size=(N, 2))
        cva = np.array([[1e-4, 1e-3, 1e-2]] * G) * (1 + np.arange(G))[:, None]
        return (L.MODEL_GROUPS, X, Y, dict(G=G, gAssign=gA, fixed=fixed, cva=cva),
                dict(K=4, G=G, gAssign=gA, fixed=fixed, Y=Y))
    assert name == "restart"
    # one group: the state a one-group Groups chain has reached after 4 sweeps.  (Several groups
    # under these hyper-parameters drive every sigmaG to 1e-9 within ten sweeps; g = Y - mu - eps is
    # then the rounding noise of a cancellation, and with group-scaled variances, which keep the
    # chain alive, the M2 filter below keeps only 35-65 % of the entries: measured with the oracle.)
    prev = O.Oracle(O.GROUPS, X, Y, cva=np.tile(CVA, (1, 1)), G=1, seed=3, order_mode=0, block_size=B, **HYP)
    prev.sweep(4)
    st = dict(mu0=prev.scalar(O.S_MU), beta0=prev.vector(O.V_BETA), sigmaE0=prev.scalar(O.S_SIGMAE),
              sigmaGG0=prev.vector(O.V_SIGMAGG), eps0=prev.vector(O.V_EPS), comp0=prev.vector(O.V_COMP))
    # a restart chain has no Y: the summaries use mu + X beta + eps of the state it starts from
    yrec = (st["mu0"] + X @ st["beta0"]) + st["eps0"]
    return L.MODEL_RESTART, X, None, dict(restart=st), dict(K=4, Y=yrec)


def _m2_check(got, want, tag):
    """M2 within RTOL where the reference M2 > 1e-6 max(M2) (below, the difference of near-equal
    samples loses the tolerance by cancellation); the filter must keep >= 90 % of the entries
    with a positive reference M2, so that it cannot hide a failure."""
    pos = want > 0
    keep = want > 1e-6 * want.max()
    share = keep.sum() / max(pos.sum(), 1)
    err = _rel(got[keep], want[keep])
    print(f"{tag}: M2 > 0 in {pos.sum()} entries, compared {keep.sum()} ({share:.3f}), rel err {err:.3g}")
    assert share >= 0.9, f"{tag}: the M2 filter keeps only {share:.3f} of the positive entries"
    assert err < RTOL, f"{tag} rel err {err}"


def _float_columns(model, L, GK):
    cols = {"mu": 1, "sigmaE": 2, "sumsq_beta": 8, "var_g": 9, "h2": 10}
    if model == L.MODEL_HORSESHOE:
        cols.update(tau=5, eta=6, c2=7)
    else:
        cols.update(sigmaG=3)
    if model == L.MODEL_GROUPS:
        cols.update(sigmaF=4)
    cols.update({f"ssq[{q}]": 12 + GK + q for q in range(GK)})
    return cols


@pytest.mark.parametrize("case", ["v2", "groups", "horseshoe", "restart", "v2-2bit"])
def test_against_oracle(brr, oracle_mod, require_gpu, case):
    """summary_run on the device against ReferenceSummary fed the oracle's state at every kept
    iteration: counts exact, means / window means / trace within the parity tolerance (the
    summaries are linear in states that agree to it), M2 within it under _m2_check's filter."""
    from bayesrrcpp_amd import _lib as L
    from bayesrrcpp_amd.summary import ReferenceSummary
    O = oracle_mod
    model, X, Y, mkw, rkw = _case(O, case)
    s, orc = _make(brr, O, model, X, Y, **mkw)
    ref = ReferenceSummary(P, N, window=WINDOW, **rkw)
    for it in range(ITER):
        orc.sweep(1)
        if _keep(it):
            ref.add_chain(it, orc)
    s.summary_begin(WINDOW)
    s.summary_run(ITER, BURN, THIN)
    assert s.summary_count == ref.n == len(KEPT)
    hs = model == L.MODEL_HORSESHOE
    GK = ref.G * ref.K
    tr, tref = s.summary(L.SUM_TRACE), ref.get(L.SUM_TRACE)
    assert tr.shape == tref.shape == (len(KEPT), 12 + 2 * GK)
    # exact: iterations, counts
    assert np.array_equal(tr[:, 0], KEPT)
    assert np.array_equal(tr[:, 11], tref[:, 11]), "nnz"
    assert np.array_equal(tr[:, 12:12 + GK], tref[:, 12:12 + GK]), "count[g][k]"
    assert np.array_equal(tr[:, 12:12 + GK].sum(axis=1), np.full(len(KEPT), P))
    assert np.array_equal(s.summary(L.SUM_WINDOW_COUNT), ref.get(L.SUM_WINDOW_COUNT))
    if hs:
        for w in L.SUM_CLASS_ITEMS:
            with pytest.raises(brr.BrrError, match="Horseshoe"):
                s.summary(w)
    else:
        assert np.array_equal(s.summary(L.SUM_COMP_COUNT), ref.get(L.SUM_COMP_COUNT))
        assert np.array_equal(s.summary(L.SUM_COMP_FREQ), ref.get(L.SUM_COMP_FREQ))
        assert np.array_equal(s.summary(L.SUM_PIP), ref.get(L.SUM_PIP))
    # parity tolerance
    for w in (L.SUM_BETA_MEAN, L.SUM_G_MEAN, L.SUM_WINDOW_SSQ, L.SUM_WINDOW_SHARE):
        err = _rel(s.summary(w), ref.get(w))
        print(f"{case} {L.SUM_NAMES[w]} rel err {err:.3g}")
        assert err < RTOL, f"{case} {L.SUM_NAMES[w]} rel err {err}"
    for name, col in _float_columns(model, L, GK).items():
        if name == "mu":
            assert np.all(np.abs(tr[:, col] - tref[:, col]) <= RTOL * (1 + np.abs(tref[:, col]))), f"{case} mu"
        else:
            err = _rel(tr[:, col], tref[:, col])
            assert err < RTOL, f"{case} trace {name} rel err {err}"
    # second moments
    bm2, gm2 = s.summary(L.SUM_BETA_M2), s.summary(L.SUM_G_M2)
    _m2_check(bm2, ref.get(L.SUM_BETA_M2), f"{case} beta")
    _m2_check(gm2, ref.get(L.SUM_G_M2), f"{case} g")
    assert np.array_equal(s.summary(L.SUM_BETA_SD), np.sqrt(bm2 / (len(KEPT) - 1)))
    assert np.array_equal(s.summary(L.SUM_G_SD), np.sqrt(gm2 / (len(KEPT) - 1)))
    s.close()


def _snapshot(s, L):
    return dict(beta=s.vector(L.BETA), comp=s.vector(L.COMP), eps=s.vector(L.EPS), mu=s.scalar(L.MU),
                sigmaE=s.scalar(L.SIGMAE), sigmaG=s.scalar(L.SIGMAG), sumsq_beta=s.scalar(L.SUMSQ_BETA))


@pytest.fixture(scope="module")
def chains(brr, oracle_mod, require_gpu):
    """The V2 chain of the accumulator tests, run once per K by a session that sweeps one iteration at
    a time and reads its state back at every kept one (the reference the summaries are checked
    against), with its final state."""
    from bayesrrcpp_amd import _lib as L
    X, Y = _cohort(oracle_mod)
    out = {"X": X, "Y": Y}
    for K, cva in ((4, CVA), (5, CVA5)):
        a, _ = _make(brr, oracle_mod, L.MODEL_V2, X, Y, cva=cva, oracle=False)
        states = []
        for it in range(ITER):
            a.sweep(1)
            if _keep(it):
                states.append((it, _snapshot(a, L)))
        out[K] = dict(cva=cva, states=states, final=a.state())
        a.close()
    return out


def _reference(chains, K, window):
    from bayesrrcpp_amd.summary import ReferenceSummary
    ref = ReferenceSummary(P, N, K=K, Y=chains["Y"], window=window)
    for it, st in chains[K]["states"]:
        st = dict(st)
        ref.add(it, st.pop("beta"), st.pop("comp"), st.pop("eps"), st.pop("mu"), **st)
    return ref


def _summarised(brr, oracle_mod, chains, K, window):
    from bayesrrcpp_amd import _lib as L
    s, _ = _make(brr, oracle_mod, L.MODEL_V2, chains["X"], chains["Y"], cva=chains[K]["cva"], oracle=False)
    s.summary_begin(window)
    s.summary_run(ITER, BURN, THIN)
    return s


@pytest.mark.parametrize("K", [4, 5])
def test_accumulator_exactness(brr, oracle_mod, require_gpu, chains, K):
    """The accumulator alone: session A's states read back at the kept iterations and folded by
    ReferenceSummary, against session B (same seed) folding on the device.  At most 4 Welford
    updates, each operation correctly rounded and uncontracted on both sides: 1e-12 leaves three
    orders of margin over 1e-15.  Folding does not disturb the chain: B ends in A's state, bit for bit."""
    from bayesrrcpp_amd import _lib as L
    ref = _reference(chains, K, WINDOW)
    s = _summarised(brr, oracle_mod, chains, K, WINDOW)
    assert s.summary_count == len(KEPT)
    for w in (L.SUM_BETA_M2, L.SUM_G_M2, L.SUM_BETA_MEAN, L.SUM_G_MEAN):
        err = _rel(s.summary(w), ref.get(w))
        print(f"K={K} {L.SUM_NAMES[w]} rel err {err:.3g}")
        assert err < 1e-12, f"K={K} {L.SUM_NAMES[w]} rel err {err}"
    for w in (L.SUM_COMP_COUNT, L.SUM_WINDOW_COUNT):
        assert np.array_equal(s.summary(w), ref.get(w)), L.SUM_NAMES[w]
    tr, tref = s.summary(L.SUM_TRACE), ref.get(L.SUM_TRACE)
    assert np.array_equal(tr[:, 0], KEPT)
    assert np.array_equal(tr[:, 11:12 + K], tref[:, 11:12 + K])  # nnz, count[k]
    assert np.array_equal(tr[:, 1:4], tref[:, 1:4]) and np.array_equal(tr[:, 8], tref[:, 8])  # the scalars
    assert _rel(tr[:, 12 + K:], tref[:, 12 + K:]) < 1e-12  # ssq[k]: sums of at most 333 squares
    err = _rel(tr[:, 9], tref[:, 9])
    print(f"K={K} var_g rel err {err:.3g}")
    assert err < 1e-11
    final, want = s.state(), chains[K]["final"]
    assert set(final) == set(want)
    for k in want:
        assert np.array_equal(final[k], want[k]), f"state {k} differs after summary_run"
    s.close()


@pytest.mark.parametrize("W", [1, 7, 64, 300, 1000])
def test_window_edges(brr, oracle_mod, require_gpu, chains, W):
    """Every form of k_summary_windows -- a thread (W = 1, 7), a wave (64) and a workgroup (300: the
    last window has 33 markers; 1000: one window) per window -- against ReferenceSummary.  The sums of
    at most 333 squares differ from numpy's in order only: 1e-12 is 30 times 333 ulps."""
    from bayesrrcpp_amd import _lib as L
    ref = _reference(chains, 4, W)
    s = _summarised(brr, oracle_mod, chains, 4, W)
    nW = -(-P // W)
    assert s.summary(L.SUM_WINDOW_COUNT).shape == (nW,)
    assert np.array_equal(s.summary(L.SUM_WINDOW_COUNT), ref.get(L.SUM_WINDOW_COUNT))
    assert np.array_equal(s.summary(L.SUM_WINDOW_PIP), ref.get(L.SUM_WINDOW_PIP))
    for w in (L.SUM_WINDOW_SSQ, L.SUM_WINDOW_SHARE):
        err = _rel(s.summary(w), ref.get(w))
        print(f"W={W} {L.SUM_NAMES[w]} rel err {err:.3g}")
        assert err < 1e-12, f"W={W} {L.SUM_NAMES[w]} rel err {err}"
    assert abs(s.summary(L.SUM_WINDOW_SHARE).sum() - 1.0) < 1e-12  # shares of every sweep sum to 1
    if W == 1:
        assert np.array_equal(s.summary(L.SUM_WINDOW_PIP), s.summary(L.SUM_PIP))
    s.close()


def test_determinism_reset_and_refusals(brr, oracle_mod, require_gpu, chains):
    from bayesrrcpp_amd import _lib as L
    a = _summarised(brr, oracle_mod, chains, 4, WINDOW)
    b = _summarised(brr, oracle_mod, chains, 4, WINDOW)
    pa, pb = a.posterior(), b.posterior()
    assert set(pa) == set(pb) == set(L.SUM_NAMES)
    for k in pa:
        assert np.array_equal(pa[k], pb[k], equal_nan=True), f"{k} differs between two runs"
    assert pa["trace"].shape == (len(KEPT), 20) and pa["comp_freq"].shape == (P, 4)
    # a second begin resets; without windows the window items are refused
    a.summary_begin(0)
    assert a.summary_count == 0
    assert a.summary(L.SUM_TRACE).shape == (0, 20) and not a.summary(L.SUM_BETA_MEAN).any()
    with pytest.raises(brr.BrrError, match="window"):
        a.summary(L.SUM_WINDOW_PIP)
    assert "window_pip" not in a.posterior()
    a.summary_accumulate()  # the current state, as kept sweep 1: iteration = sweeps so far - 1
    assert a.summary_count == 1 and a.summary(L.SUM_TRACE)[0, 0] == ITER - 1
    assert np.array_equal(a.summary(L.SUM_BETA_MEAN), a.vector(L.BETA))
    with pytest.raises(brr.BrrError, match="burn_in"):
        a.summary_run(5, 10, 1)
    with pytest.raises(brr.BrrError, match="window"):
        a.summary_begin(-1)
    # after end, and before begin: errors, not device work
    a.summary_end()
    for call in (a.summary_accumulate, a.summary_end, lambda: a.summary(L.SUM_PIP), lambda: a.summary_count,
                 lambda: a.summary_run(ITER, BURN, THIN), lambda: a.summary_write("unused")):
        with pytest.raises(brr.BrrError, match="summary_begin first"):
            call()
    a.sweep(1)  # the session goes on
    a.close()
    b.close()
    fresh = brr.Session(L.MODEL_V2, N, P, K=4, block_size=B)
    with pytest.raises(brr.BrrError, match="not initialised"):
        fresh.summary_begin()
    fresh.close()
    # a column shard: refused, and the session continues (one round of the hand-driven protocol)
    X, Y = chains["X"], chains["Y"]
    sh = brr.Session(L.MODEL_V2, N, 192, K=4, M_total=P, col_offset=0, block_size=B, shard_rank=0, shard_count=2,
                     exchanges_per_sweep=1)
    sh.upload_x(X[:, :192])
    sh.set_y(Y)
    sh.set_bayesr(**HYP, cva=CVA)
    sh.init(9)
    with pytest.raises(brr.BrrError, match="sharded"):
        sh.summary_begin(WINDOW)
    sh.exchange_buffers()
    sh.sweep_local()
    e, st = sh.exchange_get()
    sh.exchange_set(e, st)
    sh.sweep_finish()
    assert sh.iteration == 1 and np.isfinite(sh.vector(L.BETA)).all()
    sh.close()


def test_oneshot_summary_files(brr, oracle_mod, require_gpu, tmp_path, monkeypatch):
    """brr_BayesRSamplerV2 with BRR_SUMMARY_PREFIX writes the four files; their values equal a
    session's summary_run (same seed) to all 17 digits, and the CSV is the one it writes without
    the variable, byte for byte."""
    from bayesrrcpp_amd import _lib as L
    n, p, seed = 120, 90, 5
    X, Y = _cohort(oracle_mod, n, p, n_causal=9)
    args = (seed, ITER, BURN, THIN, X, Y, HYP["sigma0"], HYP["v0E"], HYP["s02E"], HYP["v0G"], HYP["s02G"], CVA)
    plain = tmp_path / "plain.csv"
    brr.BayesRSamplerV2(str(plain), *args, log=lambda m: None)
    assert sorted(f.name for f in tmp_path.iterdir()) == ["plain.csv"]
    prefix = tmp_path / "post"
    monkeypatch.setenv("BRR_SUMMARY_PREFIX", str(prefix))
    monkeypatch.setenv("BRR_SUMMARY_WINDOW", "10")
    with_sum = tmp_path / "with.csv"
    brr.BayesRSamplerV2(str(with_sum), *args, log=lambda m: None)
    monkeypatch.delenv("BRR_SUMMARY_PREFIX")
    assert with_sum.read_bytes() == plain.read_bytes()
    s = brr.Session(L.MODEL_V2, n, p, K=4)
    s.upload_x(X).set_y(Y).set_bayesr(**HYP, cva=CVA).init(seed)
    s.summary_begin(10).summary_run(ITER, BURN, THIN)
    post = s.posterior()

    def table(ext):
        path = f"{prefix}.{ext}.csv"
        header = open(path).readline().strip().split(",")
        return header, np.loadtxt(path, delimiter=",", skiprows=1, ndmin=2)

    h, t = table("markers")
    assert h == ["marker", "mean", "sd", "pip", "freq_0", "freq_1", "freq_2", "freq_3"]
    assert np.array_equal(t[:, 0], np.arange(p))
    assert np.array_equal(t[:, 1], post["beta_mean"]) and np.array_equal(t[:, 2], post["beta_sd"])
    assert np.array_equal(t[:, 3], post["pip"]) and np.array_equal(t[:, 4:], post["comp_freq"])
    h, t = table("rows")
    assert h == ["row", "g_mean", "g_sd"] and np.array_equal(t[:, 0], np.arange(n))
    assert np.array_equal(t[:, 1], post["g_mean"]) and np.array_equal(t[:, 2], post["g_sd"])
    h, t = table("windows")
    assert h == ["first_marker", "pip", "ssq", "share"] and np.array_equal(t[:, 0], np.arange(0, p, 10))
    assert np.array_equal(t[:, 1], post["window_pip"]) and np.array_equal(t[:, 2], post["window_ssq"])
    assert np.array_equal(t[:, 3], post["window_share"])
    h, t = table("trace")
    assert h == list(L.TRACE_HEADER) + [f"{a}_0_{k}" for a in ("count", "ssq") for k in range(4)]
    assert np.array_equal(t, post["trace"], equal_nan=True) and np.array_equal(t[:, 0], KEPT)
    # the session's own writer gives the same files
    s.summary_write(tmp_path / "again")
    for ext in ("markers", "rows", "windows", "trace"):
        assert open(f"{prefix}.{ext}.csv").read() == open(tmp_path / f"again.{ext}.csv").read()
    s.close()
