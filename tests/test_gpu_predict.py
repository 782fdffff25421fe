"""GPU tests of the out-of-sample prediction (brr_session_predict_*, csrc/brr_predict.hpp): the
device's scores against ReferencePredictor (bayesrrcpp_amd/predict.py) bit for bit in both target
storages, the chunk fold, the accumulators over kept sweeps against a second session whose states
are read back, the shared run loop, determinism / reset / refusals and the written files.

Training shape as test_gpu_summary.py: N = 257, P = 333, B = 64, cohort seed 20261015; 12 iterations,
burn-in 3, thinning 2: iterations 4, 6, 8 and 10 are kept.  Target cohorts: N2 = 1, 3, 257 and one row
tile of the score kernel + 5 (a second workgroup along the rows in 2-bit storage, a fifth in f32), all
prefixes of one random genotype matrix with missing genotypes and a monomorphic column, packed with
random bits in the padding of the last byte.
"""
import ctypes as C

import numpy as np
import pytest

from conftest import CVA, HYP

pytestmark = pytest.mark.gpu

N, P, B = 257, 333, 64
ITER, BURN, THIN = 12, 3, 2
KEPT = [4, 6, 8, 10]
N2_ACC = 131
HS = dict(A=(1 / np.sqrt(N)) * 150 / (P - 150), v0E=1e-3, s02E=1e-3, vL=1.0, vT=1.0, c2=1.0, vC=10.0, sC=10.0)


def _pack(codes, rng):
    """(M, n) codes 0..3 -> .bed body (M, ceil(n / 4)); the rows beyond n in the last byte are random."""
    m, n = codes.shape
    nb = (n + 3) // 4
    full = rng.integers(0, 4, size=(m, 4 * nb)).astype(np.uint8)
    full[:, :n] = codes
    q = full.reshape(m, nb, 4)
    return (q[:, :, 0] | (q[:, :, 1] << 2) | (q[:, :, 2] << 4) | (q[:, :, 3] << 6)).astype(np.uint8)


def _genotypes(seed, n, m):
    """(M, n) .bed codes: Binomial(2, f) genotypes, 3 % missing, column 17 monomorphic."""
    rng = np.random.default_rng(seed)
    f = rng.uniform(0.05, 0.5, size=m)
    g = rng.binomial(2, f[:, None], size=(m, n))
    codes = np.array([3, 2, 0], dtype=np.uint8)[g]  # copies of allele 1: 0 -> 11, 1 -> 10, 2 -> 00
    codes[rng.random((m, n)) < 0.03] = 1
    codes[17] = 3
    return codes


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).tobytes()


def _rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    scale = np.maximum(np.abs(b), np.max(np.abs(b)) * 1e-3 + 1e-300)
    return float(np.max(np.abs(a - b) / scale)) if a.size else 0.0


@pytest.fixture(scope="module")
def data(brr, oracle_mod, require_gpu):
    """The training cohorts (the synthetic X / Y of test_gpu_summary.py and a .bed of the same shape),
    the target genotypes and the value table the targets are decoded through."""
    from bayesrrcpp_amd import _lib as L
    from bayesrrcpp_amd.predict import ReferencePredictor
    assert L.PREDICT_CHUNK == brr.lib().brr_predict_chunk()
    assert L.PREDICT_ROW_TILE == brr.lib().brr_predict_row_tile()
    X, Y, _ = oracle_mod.synth_cohort(20261015, N, P, h2=0.5, n_causal=20)
    rng = np.random.default_rng(5)
    train_bed = _pack(_genotypes(1, N, P), rng)
    table = ReferencePredictor.training_table(train_bed, N)
    assert not table[17].any() and table[:, 1].max() == 0.0 and np.abs(table).max() > 1.0
    # a phenotype for the .bed-trained sessions: 20 causal markers of that cohort, h2 = 0.5
    Xb = ReferencePredictor.decode_bed(train_bed, N, table).astype(np.float64)
    causal = np.random.default_rng(4).choice(P, 20, replace=False)
    yb = Xb[:, causal] @ np.random.default_rng(4).normal(size=20) * np.sqrt(0.5 / 20)
    yb = yb + np.random.default_rng(3).normal(size=N) * np.sqrt(0.5)
    Ybed = (yb - yb.mean()) / yb.std(ddof=1)
    codes = _genotypes(2, L.PREDICT_ROW_TILE + 5, P)
    return dict(X=X, Y=Y, Ybed=Ybed, train_bed=train_bed, table=table, codes=codes, rng=rng,
                Y2=np.random.default_rng(6).normal(size=N2_ACC))


def _target(data, n2):
    """.bed body and decoded f32 matrix of the first n2 target rows"""
    from bayesrrcpp_amd.predict import ReferencePredictor
    bed = _pack(data["codes"][:, :n2], data["rng"])
    return bed, ReferencePredictor.decode_bed(bed, n2, data["table"])


def _betas(p, seed=8):
    rng = np.random.default_rng(seed)
    dense = rng.normal(size=p) * 0.05
    sparse = np.zeros(p)
    sparse[[0, 17, 100, 256, p - 1]] = rng.normal(size=5)
    negzero = np.zeros(p)
    negzero[40] = -0.0
    negzero[41] = 0.25
    return {"dense": dense, "sparse": sparse, "zero": np.zeros(p), "negzero": negzero}


def _scores(s, betas):
    return {k: s.predict_score(b) for k, b in betas.items()}


@pytest.fixture(scope="module")
def scored(brr, data):
    """predict_score of every beta, N2 and target storage, and the reference's"""
    from bayesrrcpp_amd import _lib as L
    from bayesrrcpp_amd.predict import ReferencePredictor
    betas = _betas(P)
    out = {}
    with brr.Session(L.MODEL_V2, N, P, K=4, block_size=B) as s:
        for n2 in (1, 3, N, L.PREDICT_ROW_TILE + 5):
            bed, X2 = _target(data, n2)
            ref = ReferencePredictor(X2)
            s.predict_upload_bed(bed, n2, table=data["table"])
            assert s.predict_rows == n2
            two = _scores(s, betas)
            s.predict_upload_x(X2)  # a second attach replaces the first
            assert s.predict_rows == n2
            f32 = _scores(s, betas)
            out[n2] = dict(two=two, f32=f32, ref={k: ref.score(b) for k, b in betas.items()})
        s.predict_detach()
    return out


@pytest.mark.parametrize("n2", [1, 3, N, "tile+5"])
def test_score_bit_equal(brr, require_gpu, scored, n2):
    """Explicit betas (dense; 5 non-zeros including markers 0 and P - 1; all zero; one entry -0.0):
    the 2-bit and the f32 target give the reference's bits, and each other's."""
    from bayesrrcpp_amd import _lib as L
    n2 = L.PREDICT_ROW_TILE + 5 if n2 == "tile+5" else n2
    r = scored[n2]
    for k, want in r["ref"].items():
        assert want.shape == (n2,)
        assert _bits(r["two"][k]) == _bits(want), f"N2={n2} {k}: 2-bit storage differs from the reference"
        assert _bits(r["f32"][k]) == _bits(want), f"N2={n2} {k}: f32 storage differs from the reference"
        assert _bits(r["two"][k]) == _bits(r["f32"][k])
    assert np.abs(r["ref"]["dense"]).max() > 0.1 and not r["ref"]["zero"].any()


def test_rows_do_not_depend_on_n2(brr, require_gpu, scored):
    """The targets are prefixes of one genotype matrix: a row scores the same in every cohort size
    (another grid, another column pitch)."""
    big = max(scored)
    for n2, r in scored.items():
        for k in r["two"]:
            assert _bits(r["two"][k]) == _bits(scored[big]["two"][k][:n2]), f"N2={n2} {k}"


def test_multi_chunk(brr, require_gpu):
    """P = 2 C + 77 markers: three chunks, the last with 77 markers -- the one case with a chunk fold.
    A dense beta through predict_score, no sweeps, both storages, bit-equal to the reference."""
    from bayesrrcpp_amd import _lib as L
    from bayesrrcpp_amd.predict import ReferencePredictor
    n, p, n2 = 96, 2 * L.PREDICT_CHUNK + 77, 50
    rng = np.random.default_rng(21)
    codes = _genotypes(22, n2, p)
    bed = _pack(codes, rng)
    table = ReferencePredictor.training_table(_pack(_genotypes(23, n, p), rng), n)
    X2 = ReferencePredictor.decode_bed(bed, n2, table)
    beta = rng.normal(size=p) * 0.02
    want = ReferencePredictor(X2).score(beta)
    one_chunk = ReferencePredictor(X2[:, :L.PREDICT_CHUNK]).score(beta[:L.PREDICT_CHUNK])
    assert not np.array_equal(want, one_chunk)
    with brr.Session(L.MODEL_V2, n, p, K=4, block_size=B) as s:
        s.predict_upload_bed(bed, n2, table=table)
        two = s.predict_score(beta)
        s.predict_upload_x(X2)
        f32 = s.predict_score(beta)
    assert _bits(two) == _bits(want) and _bits(f32) == _bits(want)


def _session(brr, data, case, seed=7):
    """An initialised training session: V2 on the synthetic X ("v2"), the Horseshoe on it
    ("horseshoe"), or V2 trained from the .bed in 2-bit ("bed-2bit") or f32 ("bed-f32") storage."""
    from bayesrrcpp_amd import _lib as L
    hs = case == "horseshoe"
    s = brr.Session(L.MODEL_HORSESHOE if hs else L.MODEL_V2, N, P, K=1 if hs else 4, block_size=B,
                    x_storage=L.X_2BIT if case == "bed-2bit" else L.X_F32)
    if case.startswith("bed"):
        s.upload_bed(data["train_bed"]).set_y(data["Ybed"])
    else:
        s.upload_x(data["X"]).set_y(data["Y"])
    if hs:
        s.set_horseshoe(**HS)
    else:
        s.set_bayesr(**HYP, cva=CVA)
    return s.init(seed)


def _attach(s, data, case):
    """The accumulator tests' target of N2_ACC rows: f32 ("v2"), 2-bit with an explicit table
    ("horseshoe"), 2-bit with table = NULL (the .bed-trained sessions); returns the f32 values."""
    bed, X2 = _target(data, N2_ACC)
    if case == "v2":
        s.predict_upload_x(X2)
    else:
        s.predict_upload_bed(bed, N2_ACC, table=data["table"] if case == "horseshoe" else None)
    return X2


@pytest.mark.parametrize("case", ["v2", "horseshoe", "bed-2bit", "bed-f32"])
def test_accumulators(brr, require_gpu, data, case):
    """Session A sweeps one iteration at a time and its beta and mu, read back at the kept
    iterations, go through ReferencePredictor; session B (same seed) folds on the device in
    predict_run.  The scores are the reference's bit for bit and the Welford updates the same
    correctly rounded operations; the trace moments differ in summation order only (131 terms): the
    margins of the summary's accumulator test.  Folding does not disturb the chain."""
    from bayesrrcpp_amd import _lib as L
    from bayesrrcpp_amd.predict import ReferencePredictor
    a = _session(brr, data, case)
    b = _session(brr, data, case)
    X2 = _attach(b, data, case)
    ref = ReferencePredictor(X2, data["Y2"])
    for it in range(ITER):
        a.sweep(1)
        if it >= BURN and it % THIN == 0:
            ref.add(it, a.vector(L.BETA), a.scalar(L.MU))
    b.predict_set_y(data["Y2"]).predict_begin().predict_run(ITER, BURN, THIN)
    assert b.predict_count == ref.n == len(KEPT)
    if case == "horseshoe":
        assert np.count_nonzero(a.vector(L.BETA)) == P  # the dense case
    tr, tref = b.predict(L.PRED_TRACE), ref.get(L.PRED_TRACE)
    assert tr.shape == tref.shape == (len(KEPT), 8)
    assert np.array_equal(tr[:, 0], KEPT)
    err = {"g_mean": _rel(b.predict(L.PRED_G_MEAN), ref.get(L.PRED_G_MEAN)),
           "g_m2": _rel(b.predict(L.PRED_G_M2), ref.get(L.PRED_G_M2))}
    err.update({name: _rel(tr[:, c], tref[:, c]) for c, name in enumerate(L.PRED_TRACE_HEADER) if c})
    print(f"{case}: " + ", ".join(f"{k} {v:.3g}" for k, v in err.items()))
    for k in ("g_mean", "g_m2", "mean_g", "mean_y", "mse"):
        assert err[k] < 1e-12, f"{case} {k} rel err {err[k]}"
    for k in ("var_g", "var_y", "cov_yg", "cor_yg"):
        assert err[k] < 1e-11, f"{case} {k} rel err {err[k]}"
    assert np.array_equal(b.predict(L.PRED_G_SD), np.sqrt(b.predict(L.PRED_G_M2) / (len(KEPT) - 1)))
    assert np.abs(tr[:, 2]).min() > 0 and np.abs(tr[:, 6]).max() <= 1.0
    # predict_score(None) is the chain's current beta, and changes nothing
    assert _bits(b.predict_score()) == _bits(ref.score(a.vector(L.BETA)))
    assert b.predict_count == len(KEPT)
    final, want = b.state(), a.state()
    assert set(final) == set(want)
    for k in want:
        assert np.array_equal(final[k], want[k]), f"state {k} differs after predict_run"
    a.close()
    b.close()


def test_shared_run_loop_determinism_and_reset(brr, require_gpu, data):
    """summary_begin + predict_begin + summary_run fills both accumulators from one chain; the summary
    items equal a run with no target attached bit for bit, the prediction items a predict_run's; a
    second predict_begin resets; without Y2 the y columns are NaN."""
    from bayesrrcpp_amd import _lib as L
    plain = _session(brr, data, "v2")
    plain.summary_begin(10).summary_run(ITER, BURN, THIN)
    want = plain.posterior()
    plain.close()
    only = _session(brr, data, "v2")
    _attach(only, data, "v2")
    only.predict_begin().predict_run(ITER, BURN, THIN)
    both = _session(brr, data, "v2")
    _attach(both, data, "v2")
    both.summary_begin(10).predict_begin().summary_run(ITER, BURN, THIN)
    assert both.summary_count == both.predict_count == len(KEPT)
    got = both.posterior()
    assert set(got) == set(want)
    for k in want:
        assert np.array_equal(got[k], want[k], equal_nan=True), f"summary item {k} changed with a target attached"
    for w, name in enumerate(L.PRED_NAMES):  # two runs, bit-identical
        assert _bits(both.predict(w)) == _bits(only.predict(w)), name
    tr = only.predict(L.PRED_TRACE)
    assert np.array_equal(tr[:, 0], KEPT) and np.isfinite(tr[:, :3]).all() and np.isnan(tr[:, 3:]).all()
    # a second begin resets; accumulate folds the current state as kept sweep 1
    only.predict_begin()
    assert only.predict_count == 0 and only.predict(L.PRED_TRACE).shape == (0, 8)
    assert not only.predict(L.PRED_G_MEAN).any()
    only.set_timing(True)  # the fold's two kernels between HIP events
    only.predict_accumulate()
    timed = only.predict_timing()
    only.set_timing(False)
    assert timed["folds"] == 1 and 0 < timed["fold_ms"] < 1000
    assert only.predict_count == 1 and only.predict(L.PRED_TRACE)[0, 0] == ITER - 1
    assert _bits(only.predict(L.PRED_G_MEAN)) == _bits(only.predict_score())
    assert not only.predict(L.PRED_G_SD).any()
    with pytest.raises(brr.BrrError, match="burn_in"):
        only.predict_run(5, 10, 1)
    only.predict_end()
    with pytest.raises(brr.BrrError, match="predict_begin first"):
        only.predict_count
    assert only.predict_rows == N2_ACC  # the target stays attached
    only.close()
    both.close()


def test_refusals(brr, require_gpu, data):
    from bayesrrcpp_amd import _lib as L
    s = _session(brr, data, "v2")
    calls = [s.predict_begin, s.predict_accumulate, s.predict_end, s.predict_detach, s.predict_score,
             lambda: s.predict_set_y(data["Y2"]), lambda: s.predict_run(ITER, BURN, THIN), lambda: s.predict_count,
             lambda: s.predict(L.PRED_G_MEAN), lambda: s.predict_write("unused"), lambda: s.predict_rows]
    for call in calls:  # before attach: errors, not device work
        with pytest.raises(brr.BrrError, match="no target cohort attached"):
            call()
    bed, X2 = _target(data, N2_ACC)
    with pytest.raises(brr.BrrError, match=r"did not\s+come from a \.bed"):  # training came from upload_x
        s.predict_upload_bed(bed, N2_ACC, table=None)
    s.predict_upload_x(X2)
    for call in (s.predict_accumulate, s.predict_end, lambda: s.predict_run(ITER, BURN, THIN),
                 lambda: s.predict_count, lambda: s.predict(L.PRED_TRACE), lambda: s.predict_write("unused")):
        with pytest.raises(brr.BrrError, match="predict_begin first"):
            call()
    with pytest.raises(brr.BrrError, match="summary_begin first"):  # summary_run still needs its own begin
        s.predict_begin().summary_run(ITER, BURN, THIN)
    with pytest.raises(brr.BrrError, match="unknown item"):
        s.predict(9)
    s.predict_detach()
    with pytest.raises(brr.BrrError, match="no target cohort attached"):
        s.predict_score()
    # N2 = 2^40 is refused by the size check before anything is read or allocated; the session goes on
    lib, small = brr.lib(), np.zeros(16, dtype=np.uint8)
    n2 = 2 ** 40
    tab = np.ascontiguousarray(data["table"])
    rc = lib.brr_session_predict_upload_bed(s.h, small.ctypes.data_as(C.POINTER(C.c_uint8)), n2, n2 // 4,
                                            tab.ctypes.data_as(C.POINTER(C.c_float)))
    assert rc != 0 and "does not fit" in L.last_error() and str(n2) in L.last_error()
    rc = lib.brr_session_predict_upload_x_f32(s.h, small.ctypes.data_as(C.POINTER(C.c_float)), n2, n2)
    assert rc != 0 and "does not fit" in L.last_error() and "bytes free" in L.last_error()
    with pytest.raises(brr.BrrError, match="no target cohort attached"):
        s.predict_rows
    s.sweep(1)
    assert s.iteration == 1 and np.isfinite(s.vector(L.BETA)).all()
    s.predict_upload_x(X2)  # and still takes a target that fits
    assert np.isfinite(s.predict_score()).all()
    s.close()
    # a column shard: refused, and the session continues (one round of the hand-driven protocol)
    sh = brr.Session(L.MODEL_V2, N, 192, K=4, M_total=P, col_offset=0, block_size=B, shard_rank=0, shard_count=2,
                     exchanges_per_sweep=1)
    sh.upload_x(data["X"][:, :192])
    sh.set_y(data["Y"])
    sh.set_bayesr(**HYP, cva=CVA)
    sh.init(9)
    with pytest.raises(brr.BrrError, match="sharded"):
        sh.predict_upload_x(X2[:, :192])
    with pytest.raises(brr.BrrError, match="sharded"):
        sh.predict_upload_bed(bed[:192], N2_ACC, table=data["table"][:192])
    sh.exchange_buffers()
    sh.sweep_local()
    e, st = sh.exchange_get()
    sh.exchange_set(e, st)
    sh.sweep_finish()
    assert sh.iteration == 1 and np.isfinite(sh.vector(L.BETA)).all()
    sh.close()


def test_written_files(brr, require_gpu, data, tmp_path):
    """predict_write's files, re-read, equal predict() to all 17 digits."""
    from bayesrrcpp_amd import _lib as L
    s = _session(brr, data, "bed-2bit")
    _attach(s, data, "bed-2bit")
    s.predict_set_y(data["Y2"]).predict_begin().predict_run(ITER, BURN, THIN)
    s.predict_write(tmp_path / "post")
    assert sorted(f.name for f in tmp_path.iterdir()) == ["post.target.csv", "post.target_trace.csv"]

    def table(name):
        path = tmp_path / name
        return open(path).readline().strip().split(","), np.loadtxt(path, delimiter=",", skiprows=1, ndmin=2)

    h, t = table("post.target.csv")
    assert h == ["row", "g_mean", "g_sd"] and np.array_equal(t[:, 0], np.arange(N2_ACC))
    assert np.array_equal(t[:, 1], s.predict(L.PRED_G_MEAN)) and np.array_equal(t[:, 2], s.predict(L.PRED_G_SD))
    assert t[:, 2].min() >= 0 and t[:, 2].max() > 0
    h, t = table("post.target_trace.csv")
    assert h == list(L.PRED_TRACE_HEADER)
    assert np.array_equal(t, s.predict(L.PRED_TRACE)) and np.array_equal(t[:, 0], KEPT)
    s.close()
