"""GPU parity in the 700-guard / no-selection regime (BayesRv2.cpp:216-242, BayesRv2Groups.cpp:268-295,
BRv2Grstart.cpp:219-246): the device's exact decision path (decide_bayesr, reached from the fast softmax
when the spread of logL nears the guards) and its no-selection arms -- beta and component kept, the marker
not counted in v nor in Groups' betaAcum -- against the oracle, sweep by sweep, on the cohorts of
guard_cases.py.  tests/test_oracle.py::test_guard_cohorts_are_in_regime shows on the CPU that every chain
used here is in the regime and that the oracle's own sensitivity leaves nine tenths of the 1e-9 tolerance.

Every sweep: visit order, components and v identical (hence the same markers selecting nothing); beta,
epsilon, mu, sigmaE, sigmaG, pi (Groups: alpha, sigmaF, betaAcum) within 1e-9 -- test_gpu_parity's _compare.
At the end: the session evaluated decisions exactly (diagnostics scalar 100: the positions whose first
decision of a sweep the fast softmax handed to decide_bayesr, and the chain steps decided exactly) and, for
K >= 3, at least three marker visits selected nothing.  The chains' own exact steps, which no sampled state
reaches, are run from a forced state (test_guard_windowless_exact_step)."""
import numpy as np
import pytest

import guard_cases as GC
from conftest import HYP
from test_gpu_parity import RTOL, _compare, _rel

pytestmark = pytest.mark.gpu


def _session(brr, O, c, xs="f32"):
    from bayesrrcpp_amd import _lib as L
    X, Y, kw = GC.inputs(O, c)
    cva = np.atleast_2d(kw["cva"])
    G = kw.get("G", 1)
    fixed = kw.get("fixed")
    s = brr.Session(c.model, c.N, c.P, K=c.K, groups=G, F=0 if fixed is None else fixed.shape[1], block_size=c.B,
                    order_mode=c.order, x_storage=L.X_2BIT if xs == "2bit" else L.X_F32)
    s.upload_x(X)
    if c.model != L.MODEL_RESTART:
        s.set_y(Y)
    s.set_bayesr(HYP["sigma0"], HYP["v0E"], HYP["s02E"], HYP["v0G"], HYP["s02G"], cva, kw.get("gAssign"))
    if fixed is not None:
        s.set_fixed(fixed)
    if "restart" in kw:
        r = kw["restart"]
        s.set_restart(r["mu0"], r["beta0"], r["sigmaE0"], r["sigmaGG0"], r["eps0"], r["comp0"])
    s.init(GC.ORACLE_SEED)
    return s


def _follow(s, O, c, tag, each_sweep=None):
    """The session against the oracle's chain, sweep by sweep; the end-of-run regime assertions.
    Prints the worst relative error (the figures of DESIGN.md's parity section)."""
    from bayesrrcpp_amd import _lib as L
    ref = GC.reference(O, c)
    assert _rel(s.vector(L.PI), ref[0].vector(O.V_PI)) < RTOL, f"{tag} initial pi"
    worst, nosel = 0.0, 0
    for it in range(1, c.sweeps + 1):
        s.sweep(1)
        o = ref[it]
        if each_sweep:
            each_sweep()
        assert np.array_equal(s.vector(L.ORDER), o.vector(O.V_ORDER)), f"{tag} visit order, sweep {it}"
        worst = max([worst, _rel(s.vector(L.BETA), o.vector(O.V_BETA)), _rel(s.vector(L.EPS), o.vector(O.V_EPS)),
                     _rel([s.scalar(L.SIGMAE)], [o.scalar(O.S_SIGMAE)]),
                     _rel(s.vector(L.SIGMAGG), o.vector(O.V_SIGMAGG)), _rel(s.vector(L.PI), o.vector(O.V_PI))])
        print(f"{tag} sweep {it}: worst relative error so far {worst:.2e}, "
              f"no selection {int(c.P - s.vector(L.VCOUNT).sum())} (oracle {int(o.vector(O.V_REGIME)[O.R_NO_SELECTION])})")
        _compare(s, o, O, L, c.model, tag=f"{tag} sweep {it}")
        if c.model == L.MODEL_GROUPS:
            assert _rel(s.vector(L.ALPHA), o.vector(O.V_ALPHA)) < RTOL, f"{tag} alpha, sweep {it}"
            assert _rel([s.scalar(L.SIGMAF)], [o.scalar(O.S_SIGMAF)]) < RTOL, f"{tag} sigmaF, sweep {it}"
        if c.model != L.MODEL_V2:
            assert _rel(s.vector(L.BETAACUM), o.vector(O.V_BETAACUM)) < RTOL, f"{tag} betaAcum, sweep {it}"
        nosel += int(c.P - s.vector(L.VCOUNT).sum())
    print(f"{tag}: worst relative error {worst:.2e}, exact evaluations {int(s.scalar(100))}, no selection {nosel}")
    assert s.scalar(100) > 0, f"{tag}: no decision was evaluated exactly"
    if c.K >= 3:
        assert nosel >= 3, f"{tag}: {nosel} marker visits selected nothing"
    else:
        assert nosel == 0


class Case:
    """One device configuration on one of guard_cases' chains"""
    def __init__(self, chain, xs="f32", fused=None, **env):
        self.chain, self.xs, self.fused, self.env = chain, xs, fused, env
        self.id = "-".join([chain.id, xs] + [f"{k[4:].lower()}={v}" for k, v in env.items() if k != "BRR_STREAM_WG"])

    def open(self, brr, O, monkeypatch):
        for k, v in self.env.items():
            monkeypatch.setenv(k, str(v))
        s = _session(brr, O, self.chain, self.xs)
        if self.fused is True:
            assert s.scalar(104) > 1  # the fused sweep, several streaming workgroups
        elif self.fused is False:
            assert s.scalar(104) == 0  # the per-block kernels
        return s


# Small (257 x 333, 12 causal): B = 128 in every visit order -- K = 4 decides through decide_fast_quad, K = 2
# and 5 through the runtime-K form; B = 64, the per-block kernels (k_stream / k_solve), in both storages;
# REFERENCE order on 2-bit storage, the per-block kernels reading member columns by index
SMALL = ([Case(c) for c in GC.SMALL] + [Case(GC.SMALL_B64, xs, fused=False) for xs in ("f32", "2bit")] +
         [Case(GC.SMALL_REF, "2bit", fused=False)])
# Fused (1500 x 1100, 30 causal, B = 128, 5 streaming workgroups): V2, Groups (G = 3, one fixed effect) and
# restart x the round-5 solver and the overlapped one (brr_ovsolve.hpp: its own copies of the decision and of
# the no-selection arms) x pipeline lag 1 and 2 x both storages.  The restart chain starts where the Groups
# (G = 1) oracle chain stands after 5 sweeps on this cohort: sigmaE has collapsed, so its first sweep is
# already in the regime.
FUSED = [Case(GC.FUSED[model], xs, fused=True, BRR_OVS=ovs, BRR_LAG=lag, BRR_STREAM_WG=5)
         for model in (0, 1, 2) for ovs in (0, 1) for lag in (1, 2) for xs in ("f32", "2bit")]
# Row chain: V2 at B = 512 (both storages) and B = 256 (2-bit) on the fused sweep
ROW_CHAIN = [Case(GC.ROW_CHAIN[B], xs, fused=True, BRR_STREAM_WG=5) for B, xs in ((512, "f32"), (512, "2bit"), (256, "2bit"))]
CASES = SMALL + FUSED + ROW_CHAIN


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.id)
def test_guard_parity(brr, oracle_mod, require_gpu, monkeypatch, case):
    with case.open(brr, oracle_mod, monkeypatch) as s:
        each = None
        if "BRR_OVS" in case.env:
            def each():
                assert s.scalar(132) == case.env["BRR_OVS"]  # the solver form this sweep ran
        _follow(s, oracle_mod, case.chain, case.id, each_sweep=each)


# the chains' exact steps (`exf`): a position still flagged `ex` when the serial chain reaches it, decided
# there by decide_bayesr with no window.  An exact evaluation leaves the flag only when it has no window to
# give -- p within 1e-12 of a cumulative sum, or no non-zero slope -- which no sampled state reaches, so the
# state is forced: sigmaG = 0 makes every denominator infinite and every slope 0, logL = log(pi), and pi alone
# decides whether the guards fire.
WINDOWLESS = [Case(GC.SMALL[4]), Case(GC.SMALL[5]), Case(GC.SMALL_B64, fused=False),
              Case(GC.FUSED[0], fused=True, BRR_OVS=0, BRR_STREAM_WG=5),
              Case(GC.FUSED[0], fused=True, BRR_OVS=1, BRR_STREAM_WG=5),
              Case(GC.ROW_CHAIN[512], fused=True, BRR_STREAM_WG=5)]


@pytest.mark.parametrize("guards", [True, False], ids=["every-guard", "no-guard"])
@pytest.mark.parametrize("case", WINDOWLESS, ids=lambda c: c.id)
def test_guard_windowless_exact_step(brr, oracle_mod, require_gpu, monkeypatch, case, guards):
    """One sweep from a forced state in which every visit is an exact step of the serial chain (diagnostics
    scalar 100 counts them), against the oracle from the same state.  every-guard: the two small entries of
    pi lie more than 700 below the others in log, every guard of BayesRv2.cpp:216-240 is true, every
    cumulative sum stays 0 and no marker selects anything -- beta and the components come back bit for bit
    and v is all zero.  no-guard: the same state with a spread of 460: every marker selects a component
    through the same exact step (infinite denominators: the new beta is 0 whatever the component).  Scalar
    100 counts every position once at its first decision and once more for its exact chain step."""
    from bayesrrcpp_amd import _lib as L
    O = oracle_mod
    c = case.chain
    X, Y, kw = GC.inputs(O, c)
    small = 1e-310 if guards else 1e-200
    pi = np.array([0.25, 0.75 - (c.K - 2) * small] + [small] * (c.K - 2))
    rng = np.random.default_rng(11)
    beta = np.where(rng.random(c.P) < 0.3, rng.normal(0, 0.05, c.P), 0.0)
    comp = np.where(beta != 0, rng.integers(1, c.K, c.P), 0).astype(float)
    eps = Y - X @ beta
    o = O.Oracle(c.model, X, Y, seed=GC.ORACLE_SEED, order_mode=c.order, block_size=c.B, N=c.N, **HYP, **kw)
    with case.open(brr, O, monkeypatch) as s:
        for sv, ov, a in ((L.BETA, O.V_BETA, beta), (L.COMP, O.V_COMP, comp), (L.PI, O.V_PI, pi), (L.EPS, O.V_EPS, eps)):
            s.set_vector(sv, a)
            o.set_vector(ov, a)
        s.set_scalar(L.SIGMAE, 0.6)
        o.set_scalar(O.S_SIGMAE, 0.6)
        s.set_scalar(L.SIGMAG, 0.0)
        o.set_scalar(O.S_SIGMAG, 0.0)
        s.sweep(1)
        o.sweep(1)
        nosel = int(o.vector(O.V_REGIME)[O.R_NO_SELECTION])
        assert nosel == (c.P if guards else 0)
        _compare(s, o, O, L, c.model, tag=case.id)
        if guards:
            assert s.vector(L.VCOUNT).sum() == 0
            assert np.array_equal(s.vector(L.BETA).view(np.uint64), beta.view(np.uint64))
            assert np.array_equal(s.vector(L.COMP), comp)
        else:
            assert s.vector(L.VCOUNT).sum() == c.P and not s.vector(L.BETA).any()
        assert s.scalar(100) > c.P  # more than the first decisions alone: the chain's exact steps ran
