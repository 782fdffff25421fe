"""Out-of-sample prediction, in plain numpy.

`ReferencePredictor` is the executable specification of the device path behind
brr_session_predict_* (include/brr.h, csrc/brr_predict.hpp): the same decode of a PLINK .bed through
a value table, the same order of every sum of a score, and the same Welford and trace definitions,
one `add()` per kept sweep.  The GPU tests compare the device against it bit for bit (scores) and to
rounding (accumulators), and it scores a chain that did not run on a GPU: it needs numpy only and
never loads libbrr.so.

    chunk c = markers [c C, (c + 1) C), C = PREDICT_CHUNK
    acc_c = 0;  acc_c = acc_c + f64(x_ij) * beta_j   for j in the chunk, ascending, beta_j != 0
    g_i   = 0;  g_i = g_i + acc_c                      for c ascending
    d = g - mean;  mean += d / n;  M2 += d * (g - mean)              (per target row)
    trace row = [iteration, mean_g, var_g, mean_y, var_y, cov_yg, cor_yg, mse]
"""
from __future__ import annotations

import numpy as np

from ._lib import PRED_G_M2, PRED_G_MEAN, PRED_G_SD, PRED_NAMES, PRED_TRACE, PRED_TRACE_HEADER, PREDICT_CHUNK

_GENOTYPE = np.array([2.0, 0.0, 1.0, 0.0])  # copies of allele 1 of codes 00, 01 (missing), 10, 11


def _codes(bed, n_rows, n_markers=None, bytes_per_col=None):
    """(M, n_rows) codes 0..3 of a .bed body; bits beyond n_rows in the last byte are not read."""
    b = np.ascontiguousarray(bed, dtype=np.uint8)
    if bytes_per_col is None:
        bytes_per_col = b.shape[1] if b.ndim == 2 else (n_rows + 3) // 4
    if bytes_per_col < (n_rows + 3) // 4:
        raise ValueError("bytes_per_col < ceil(rows / 4)")
    if n_markers is None:
        n_markers = b.size // bytes_per_col
    if b.size < n_markers * bytes_per_col:
        raise ValueError("bed holds fewer than M * bytes_per_col bytes")
    b = b.ravel()[:n_markers * bytes_per_col].reshape(n_markers, bytes_per_col)
    i = np.arange(n_rows)
    return (b[:, i >> 2] >> (2 * (i & 3)).astype(np.uint8)) & 3


class ReferencePredictor:
    """Scores and running prediction summaries of a target cohort of N2 rows and M markers.

    X2: the target genotypes as the device stores them, N2 x M float32 (a float64 matrix is rounded to
    float32 as the upload rounds it); or use `from_bed`.  Y2: optional validation phenotypes.
    """

    def __init__(self, X2, Y2=None):
        X2 = np.asarray(X2)
        if X2.ndim != 2:
            raise ValueError("X2 must be N2 x M")
        self.X = np.asfortranarray(X2, dtype=np.float32)
        self.N2, self.M = self.X.shape
        self.Y = None if Y2 is None else np.asarray(Y2, dtype=np.float64).reshape(self.N2)
        self.n = 0
        self.gmean, self.gM2 = np.zeros(self.N2), np.zeros(self.N2)
        self.rows = []

    # -- .bed input -------------------------------------------------------------------------------
    @staticmethod
    def training_table(bed, N, bytes_per_col=None):
        """The (M, 4) float32 value table brr_session_upload_bed gives a training .bed of N rows:
        genotype = copies of allele 1, standardised per column as R's scale() after mean imputation
        (sd over N - 1), missing -> 0, a column without variation all 0."""
        codes = _codes(bed, N, None, bytes_per_col)
        cnt = np.stack([(codes == c).sum(axis=1) for c in range(4)], axis=1).astype(np.float64)
        nobs = cnt[:, 0] + cnt[:, 2] + cnt[:, 3]
        S = 2.0 * cnt[:, 0] + cnt[:, 2]
        Q = 4.0 * cnt[:, 0] + cnt[:, 2]
        mean = np.where(nobs > 0, S / np.maximum(nobs, 1.0), 0.0)
        ss = Q - S * mean
        flat = (nobs < 2) | ~(ss > 0.0) | (N < 2)
        sd = np.where(flat, 1.0, np.sqrt(np.where(flat, 1.0, ss) / max(N - 1, 1)))
        table = ((_GENOTYPE[None, :] - mean[:, None]) / sd[:, None]).astype(np.float32)
        table[:, 1] = 0.0
        table[flat] = 0.0
        return table

    @staticmethod
    def decode_bed(bed, N2, table, bytes_per_col=None):
        """N2 x M float32: row i of marker j is table[j, code], the code in bits 2(i&3).. of byte i>>2
        of the marker's column.  Bits of rows >= N2 take no part."""
        table = np.asarray(table, dtype=np.float32)
        codes = _codes(bed, N2, table.shape[0], bytes_per_col)
        return np.asfortranarray(np.take_along_axis(table, codes, axis=1).T)

    @classmethod
    def from_bed(cls, bed, N2, table, bytes_per_col=None, Y2=None):
        return cls(cls.decode_bed(bed, N2, table, bytes_per_col), Y2)

    # -- the score, in the device's order -----------------------------------------------------------
    def score(self, beta):
        beta = np.asarray(beta, dtype=np.float64).reshape(self.M)
        g = np.zeros(self.N2)
        for c0 in range(0, self.M, PREDICT_CHUNK):
            acc = np.zeros(self.N2)
            for j in c0 + np.flatnonzero(beta[c0:c0 + PREDICT_CHUNK] != 0.0):
                acc = acc + self.X[:, j].astype(np.float64) * beta[j]
            g = g + acc
        return g

    # -- one kept sweep -------------------------------------------------------------------------
    def add(self, iteration, beta, mu):
        g = self.score(beta)
        self.n += 1
        n = float(self.n)
        d = g - self.gmean
        self.gmean = self.gmean + d / n
        self.gM2 = self.gM2 + d * (g - self.gmean)
        N2 = self.N2
        gbar = float(np.sum(g) / N2)
        var_g = float(np.sum((g - gbar) ** 2) / (N2 - 1)) if N2 > 1 else 0.0
        row = [float(iteration), gbar, var_g] + [np.nan] * 5
        if self.Y is not None:
            y = self.Y
            ybar = float(np.sum(y) / N2)
            var_y = float(np.sum((y - ybar) ** 2) / (N2 - 1)) if N2 > 1 else 0.0
            cov = float(np.sum((y - ybar) * (g - gbar)) / (N2 - 1)) if N2 > 1 else 0.0
            cor = cov / np.sqrt(var_y * var_g) if var_y > 0.0 and var_g > 0.0 else 0.0
            mse = float(np.sum(((y - mu) - g) ** 2) / N2)
            row[3:] = [ybar, var_y, cov, float(cor), mse]
        self.rows.append(row)
        return self

    # -- results (brr_session_predict_get's items) ---------------------------------------------------
    def get(self, which):
        if which == PRED_G_MEAN:
            return self.gmean
        if which == PRED_G_M2:
            return self.gM2
        if which == PRED_G_SD:
            return np.sqrt(self.gM2 / (self.n - 1)) if self.n >= 2 else np.zeros(self.N2)
        if which == PRED_TRACE:
            return np.array(self.rows, dtype=np.float64).reshape(self.n, len(PRED_TRACE_HEADER))
        raise ValueError(f"unknown item {which}")

    def posterior(self):
        return {name: self.get(w) for w, name in enumerate(PRED_NAMES)}
