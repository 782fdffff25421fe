"""The 700-guard / no-selection regime (BayesRv2.cpp:216-242): the cohort that reaches it and the
chains that test_oracle.py (is the oracle in the regime, and stable enough to compare against?) and
test_gpu_guard.py (does the device follow it there?) both run.  A plain module, imported by both.

The regime needs sigmaE to collapse: a few strong causal markers, almost no noise and a standardised
Y.  The spread of logL then passes 700, the reference zeroes whole cumulative sums, and a marker
whose uniform p lies above the last one selects no component (beta and component kept, not counted).
synth_cohort(h2 = 0.5) never gets there: its logL spreads stay in the tens."""
import functools
from dataclasses import dataclass

import numpy as np

from conftest import CVA, HYP
from test_gpu_parity import _rel as rel  # noqa: F401  (the parity tests' relative error)

V2, GROUPS, RESTART = 0, 1, 2
BLOCKED, REFERENCE, IDENTITY = 0, 1, 2
ORACLE_SEED = 7
CVA_K = {2: [1e-2], 4: list(CVA), 5: [1e-4, 1e-3, 3e-3, 1e-2]}


def guard_cohort(seed, N, P, n_causal):
    """Genotype cohort (at most three values per column: valid in 2-bit storage), strong signal."""
    rng = np.random.default_rng(seed)
    f = rng.uniform(0.1, 0.5, P)
    g = (rng.random((N, P)) < f).astype(np.float64) + (rng.random((N, P)) < f)
    X = (g - g.mean(0)) / np.maximum(g.std(0, ddof=1), 1e-3)
    X = np.asfortranarray(X.astype(np.float32).astype(np.float64))
    idx = rng.choice(P, n_causal, replace=False)
    y = X[:, idx] @ rng.normal(0, 1, n_causal) + 0.02 * rng.normal(size=N)
    return X, (y - y.mean()) / y.std(ddof=1)


@dataclass(frozen=True)
class Chain:
    """What the oracle's chain depends on (solver form, pipeline lag and storage do not change it)."""
    model: int
    N: int
    P: int
    n_causal: int
    K: int
    B: int
    order: int
    sweeps: int
    cohort_seed: int = 1

    @property
    def id(self):
        return (f"{('v2', 'groups', 'restart')[self.model]}-{self.N}x{self.P}-K{self.K}-B{self.B}-"
                f"{('blocked', 'reference', 'identity')[self.order]}-{self.sweeps}sw")


# sweeps: 12, but the K = 2 chains only while five twins of the oracle (Y moved by two ulps) stay within 1e-10
# of it, a tenth of the parity tolerance (test_oracle.py::test_guard_cohorts_are_in_regime): with one
# non-zero component every causal marker is redrawn in every sweep, which amplifies faster
def _sweeps(K, order):
    return 12 if K != 2 else (6 if order == IDENTITY else 7)


SMALL = [Chain(V2, 257, 333, 12, K, 128, order, _sweeps(K, order)) for order in (IDENTITY, BLOCKED, REFERENCE)
         for K in (2, 4, 5)]
SMALL_B64 = Chain(V2, 257, 333, 12, 4, 64, BLOCKED, 12)
SMALL_REF = Chain(V2, 257, 333, 12, 4, 128, REFERENCE, 12)
FUSED = {m: Chain(m, 1500, 1100, 30, 4, 128, BLOCKED, 12) for m in (V2, GROUPS, RESTART)}
ROW_CHAIN = {B: Chain(V2, 1500, 1100, 30, 4, B, BLOCKED, 12) for B in (512, 256)}
CHAINS = list(dict.fromkeys(SMALL + [SMALL_B64, SMALL_REF] + list(FUSED.values()) + list(ROW_CHAIN.values())))

RESTART_AFTER = 5  # sweeps of the Groups (G = 1) chain whose state the restart chain starts from


def _oracle_kwargs(O, c, X, Y):
    """(model inputs shared by the oracle and the session, the oracle's Y)"""
    kw = dict(cva=np.asarray(CVA_K[c.K], float))
    if c.model == GROUPS:
        G = 3
        kw.update(G=G, gAssign=(np.arange(c.P) * G // c.P).astype(np.int32), cva=np.tile(kw["cva"], (G, 1)),
                  fixed=np.linspace(-1, 1, c.N).reshape(c.N, 1))
    elif c.model == RESTART:
        # sigmaE has collapsed by then: the first restarted sweep is already in the regime
        prev = O.Oracle(O.GROUPS, X, Y, cva=kw["cva"], G=1, seed=ORACLE_SEED, order_mode=c.order,
                        block_size=c.B, **HYP)
        prev.sweep(RESTART_AFTER)
        kw.update(G=1, cva=kw["cva"].reshape(1, -1),
                  restart=dict(mu0=prev.scalar(O.S_MU), beta0=prev.vector(O.V_BETA), sigmaE0=prev.scalar(O.S_SIGMAE),
                               sigmaGG0=prev.vector(O.V_SIGMAGG), eps0=prev.vector(O.V_EPS),
                               comp0=prev.vector(O.V_COMP)))
    return kw


@functools.lru_cache(maxsize=None)
def inputs(O, c):
    """X, Y and the model's further inputs of a chain, computed once"""
    X, Y = guard_cohort(c.cohort_seed, c.N, c.P, c.n_causal)
    return X, Y, _oracle_kwargs(O, c, X, Y)


class Snapshot:
    """The oracle's state after one sweep, read like the oracle itself (vector / scalar)"""
    def __init__(self, O, o):
        vecs = [O.V_BETA, O.V_COMP, O.V_EPS, O.V_SIGMAGG, O.V_PI, O.V_ALPHA, O.V_ORDER, O.V_VCOUNT, O.V_BETAACUM,
                O.V_REGIME]
        self._v = {w: o.vector(w) for w in vecs}
        for a in self._v.values():
            a.setflags(write=False)
        self._s = {w: o.scalar(w) for w in (O.S_MU, O.S_SIGMAE, O.S_SIGMAG, O.S_SIGMAF)}

    def vector(self, w):
        return self._v[w]

    def scalar(self, w):
        return self._s[w]


def run_chain(O, c, y_factor=None):
    """[state before the first sweep, state after sweep 1, ...] of the oracle's chain; y_factor
    multiplies Y elementwise (the twins of test_guard_cohorts_are_in_regime)"""
    X, Y, kw = inputs(O, c)
    if y_factor is not None:
        Y = Y * y_factor
        kw = _oracle_kwargs(O, c, X, Y)
    kw = dict(kw)
    kw.update(kw.pop("restart", {}))
    o = O.Oracle(c.model, X, None if c.model == RESTART else Y, seed=ORACLE_SEED, order_mode=c.order,
                 block_size=c.B, N=c.N, **HYP, **kw)
    out = [Snapshot(O, o)]
    for _ in range(c.sweeps):
        o.sweep(1)
        out.append(Snapshot(O, o))
    return out


@functools.lru_cache(maxsize=None)
def reference(O, c):
    """The unperturbed chain, computed once per process and shared, read-only"""
    return run_chain(O, c)


def regime_counts(O, snaps):
    """[first guard, later guard, no selection, spread in [600, 800)] visits summed over the sweeps"""
    return np.sum([s.vector(O.V_REGIME) for s in snaps[1:]], axis=0).astype(int)
