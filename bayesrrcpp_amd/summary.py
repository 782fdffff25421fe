"""Posterior summaries over kept sweeps, in plain numpy.

`ReferenceSummary` is the executable specification of the device accumulator behind
brr_session_summary_* (include/brr.h, csrc/brr_summary.hpp): the same definitions and the same
Welford recurrence, one `add()` per kept sweep.  The GPU tests compare the device against it, and
it summarises a chain that did not run on a GPU (a CSV read back, the CPU oracle): it needs numpy
only and never loads libbrr.so.

    d = x - mean;  mean += d / n;  M2 += d * (x - mean)          (beta per marker, g per row)
    g_i = ((Y_i - mu) - eps_i) - sum_c fixed[i, c] * alpha_c      (c ascending)
    window w = markers [w W, (w + 1) W): any marker in the model, running means of its
               sum beta^2 and of its share of the sweep's total (0 when the total is 0)
    trace row = [iteration, mu, sigmaE, sigmaG, sigmaF, tau, eta, c2, sumsq_beta, var_g, h2, nnz,
                 count[g][k] ..., ssq[g][k] ...]
"""
from __future__ import annotations

import numpy as np

from ._lib import (ALPHA, BETA, C2, COMP, EPS, ETA, MU, SIGMAE, SIGMAF, SIGMAG, SUM_BETA_M2,
                   SUM_BETA_MEAN, SUM_BETA_SD, SUM_CLASS_ITEMS, SUM_COMP_COUNT, SUM_COMP_FREQ, SUM_G_M2, SUM_G_MEAN,
                   SUM_G_SD, SUM_NAMES, SUM_PIP, SUM_TRACE, SUM_WINDOW_COUNT, SUM_WINDOW_ITEMS, SUM_WINDOW_PIP,
                   SUM_WINDOW_SHARE, SUM_WINDOW_SSQ, SUMSQ_BETA, TAU)


class ReferenceSummary:
    """Running summaries of a chain of M markers and N rows.

    K = mixture classes including the zero one, G = groups (gAssign: group of each marker);
    horseshoe=True: no classes (G = K = 1 in the trace, a marker is in the model when beta != 0).
    Y: the phenotype (a restart chain: mu + X beta + eps of its first state); fixed: N x F.
    """

    def __init__(self, M, N, K=1, G=1, gAssign=None, Y=None, fixed=None, window=0, horseshoe=False):
        if window < 0:
            raise ValueError("window < 0")
        self.M, self.N, self.hs = M, N, bool(horseshoe)
        self.K, self.G = (1, 1) if self.hs else (K, G)
        self.gAssign = np.zeros(M, dtype=np.int64) if gAssign is None or self.hs else np.asarray(gAssign, dtype=np.int64)
        self.Y = np.zeros(N) if Y is None else np.asarray(Y, dtype=np.float64)
        self.fixed = None if fixed is None else np.asarray(fixed, dtype=np.float64).reshape(N, -1)
        self.window = window
        self.nW = -(-M // window) if window else 0
        self.width = 12 + 2 * self.G * self.K
        self.n = 0
        self.bmean, self.bM2 = np.zeros(M), np.zeros(M)
        self.gmean, self.gM2 = np.zeros(N), np.zeros(N)
        self.cfreq = np.zeros((M, self.K), dtype=np.int64)
        self.wany = np.zeros(self.nW, dtype=np.int64)
        self.wssq, self.wshare = np.zeros(self.nW), np.zeros(self.nW)
        self.rows = []

    # -- one kept sweep -------------------------------------------------------------------------
    def add(self, iteration, beta, comp, eps, mu, alpha=None, *, sigmaE=0.0, sigmaG=0.0, sigmaF=0.0,
            tau=0.0, eta=0.0, c2=0.0, sumsq_beta=None):
        beta = np.asarray(beta, dtype=np.float64)
        eps = np.asarray(eps, dtype=np.float64)
        b2 = beta * beta
        if self.hs:
            comp = np.zeros(self.M, dtype=np.int64)
            inmodel = beta != 0.0
        else:
            comp = np.asarray(comp).astype(np.int64)
            inmodel = comp > 0
        self.n += 1
        n = float(self.n)
        d = beta - self.bmean
        self.bmean = self.bmean + d / n
        self.bM2 = self.bM2 + d * (beta - self.bmean)
        if not self.hs:
            self.cfreq[np.arange(self.M), comp] += 1
        # genetic values
        fa = np.zeros(self.N)
        if self.fixed is not None and alpha is not None:
            alpha = np.asarray(alpha, dtype=np.float64)
            for c in range(self.fixed.shape[1]):
                fa = fa + self.fixed[:, c] * alpha[c]
        g = ((self.Y - mu) - eps) - fa
        d = g - self.gmean
        self.gmean = self.gmean + d / n
        self.gM2 = self.gM2 + d * (g - self.gmean)
        var_g = float(np.sum((g - np.mean(g)) ** 2) / (self.N - 1)) if self.N > 1 else 0.0
        h2 = var_g / (var_g + sigmaE) if var_g + sigmaE > 0 else 0.0
        total = float(np.sum(b2))
        if self.window:
            starts = np.arange(0, self.M, self.window)
            ssq = np.add.reduceat(b2, starts)
            self.wany += np.maximum.reduceat(inmodel.astype(np.int64), starts)
            share = ssq / total if total > 0 else np.zeros(self.nW)
            self.wssq = self.wssq + (ssq - self.wssq) / n
            self.wshare = self.wshare + (share - self.wshare) / n
        key = self.gAssign * self.K + comp
        GK = self.G * self.K
        count = np.bincount(key, minlength=GK).astype(np.float64)
        ssq_gk = np.bincount(key, weights=b2, minlength=GK)
        head = [float(iteration), mu, sigmaE, sigmaG, sigmaF, tau, eta, c2,
                total if sumsq_beta is None else sumsq_beta, var_g, h2, float(np.count_nonzero(inmodel))]
        self.rows.append(np.concatenate([head, count, ssq_gk]))
        return self

    def add_chain(self, iteration, chain):
        """The current state of a chain object with scalar(which) / vector(which) in the library's
        numbering: a Session, or the CPU oracle's Oracle (whose S_* / V_* constants share it)."""
        vec, sc = chain.vector, chain.scalar
        alpha = vec(ALPHA) if self.fixed is not None else None
        extra = dict(tau=sc(TAU), eta=sc(ETA), c2=sc(C2)) if self.hs else dict(sigmaG=sc(SIGMAG))
        if alpha is not None:
            extra["sigmaF"] = sc(SIGMAF)
        return self.add(iteration, vec(BETA), None if self.hs else vec(COMP), vec(EPS), sc(MU), alpha,
                        sigmaE=sc(SIGMAE), sumsq_beta=sc(SUMSQ_BETA), **extra)

    # -- results (brr_session_summary_get's items) ------------------------------------------------
    def _sd(self, M2):
        return np.sqrt(M2 / (self.n - 1)) if self.n >= 2 else np.zeros_like(M2)

    def get(self, which):
        if self.hs and which in SUM_CLASS_ITEMS:
            raise ValueError(f"{SUM_NAMES[which]} is class-based: the Horseshoe has no mixture classes")
        if not self.window and which in SUM_WINDOW_ITEMS:
            raise ValueError(f"{SUM_NAMES[which]} needs window > 0")
        n = max(self.n, 1)
        return {
            SUM_BETA_MEAN: lambda: self.bmean, SUM_BETA_SD: lambda: self._sd(self.bM2),
            SUM_PIP: lambda: 1.0 - self.cfreq[:, 0] / n if self.n else np.zeros(self.M),
            SUM_COMP_FREQ: lambda: self.cfreq / n,
            SUM_G_MEAN: lambda: self.gmean, SUM_G_SD: lambda: self._sd(self.gM2),
            SUM_WINDOW_PIP: lambda: self.wany / n, SUM_WINDOW_SSQ: lambda: self.wssq,
            SUM_WINDOW_SHARE: lambda: self.wshare,
            SUM_TRACE: lambda: np.array(self.rows).reshape(self.n, self.width),
            SUM_BETA_M2: lambda: self.bM2, SUM_G_M2: lambda: self.gM2,
            SUM_COMP_COUNT: lambda: self.cfreq.astype(np.float64),
            SUM_WINDOW_COUNT: lambda: self.wany.astype(np.float64),
        }[which]()

    def posterior(self):
        skip = set(SUM_CLASS_ITEMS if self.hs else ())
        if not self.window:
            skip.update(SUM_WINDOW_ITEMS)
        return {name: self.get(w) for w, name in enumerate(SUM_NAMES) if w not in skip}
