// brr_summary.hpp -- posterior summaries folded on the device (brr_session_summary_*, include/brr.h).
//
// Included by brr_kernels.hip inside namespace brr (it uses block_sum / wave_sum / last_arriver and
// x-free state only: beta, comp, eps, mu, alpha).  One kept sweep is three small launches on the
// session stream, after the sweep's k_hyper:
//
//   k_summary_markers  one thread per marker: Welford update of beta's mean / M2, the class
//                      frequencies, and the trace row's count[g][k] / ssq[g][k] / nnz / total
//                      sum beta^2 through per-workgroup slabs summed by the last arriving workgroup.
//   k_summary_windows  (W > 0) per window of W consecutive markers: any marker in the model, the
//                      running means of its sum beta^2 and of its share of the sweep's total.
//   k_summary_rows     one thread per row: g_i = ((Y_i - mu) - eps_i) - sum_c fixed[i,c] alpha_c, its
//                      Welford update, and var_g as the exact many-way Chan merge of the
//                      workgroups' (rows, mean, centred M2).
//
// Every sum runs in a fixed order (no floating-point atomics; the LDS counters are integers), so the
// summaries are bit-identical from run to run.  Nothing here writes chain state.
#pragma once

// thresholds of k_summary_windows' three forms: a thread, a wave or a workgroup per window
constexpr int SUM_W_THREAD = 8;
constexpr int SUM_W_WAVE = 256;

__global__ __launch_bounds__(256) void k_summary_markers(Dev d, SumDev q, double n, double iteration) {
#pragma clang fp contract(off)
  __shared__ double red[8];
  __shared__ int cnt[MAXG * MAXK];
  __shared__ double s_b2[256];
  __shared__ int s_key[256];
  __shared__ int s_last;
  const bool hs = d.model == MODEL_HORSESHOE;
  const int GK = hs ? 1 : d.G * d.K;
  const int SW = 2 * GK + 2;  // slab: count[GK], ssq[GK], total sum beta^2, nnz
  const int64_t m = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const bool valid = m < d.M;
  for (int k = threadIdx.x; k < GK; k += 256) cnt[k] = 0;
  __syncthreads();
  double b2 = 0.0, nz = 0.0;
  int key = -1;
  if (valid) {
    const double b = d.beta[m];
    b2 = b * b;
    double mean = q.bmean[m];
    const double dl = b - mean;
    mean += dl / n;
    q.bM2[m] += dl * (b - mean);
    q.bmean[m] = mean;
    if (hs) {
      key = 0;
      nz = b != 0.0 ? 1.0 : 0.0;
    } else {
      const int c = d.comp[m];
      const int g = d.gAssign ? d.gAssign[m] : 0;
      if (c >= 0 && c < d.K && g >= 0 && g < d.G) {
        key = g * d.K + c;
        q.cfreq[m * d.K + c] += 1u;
      }
      nz = c > 0 ? 1.0 : 0.0;
    }
    if (key >= 0) atomicAdd(&cnt[key], 1);
  }
  s_key[threadIdx.x] = key;
  s_b2[threadIdx.x] = b2;
  const double tot = block_sum<256>(b2, red);  // (its barriers publish s_key / s_b2 / cnt)
  const double nnz = block_sum<256>(nz, red);
  double *out = q.mslab + (int64_t)blockIdx.x * SW;
  // sum beta^2 of each (group, class): the workgroup's markers in index order
  for (int k = threadIdx.x; k < GK; k += 256) {
    double a = 0.0;
    for (int j = 0; j < 256; ++j)
      if (s_key[j] == k) a += s_b2[j];
    out[k] = (double)cnt[k];
    out[GK + k] = a;
  }
  if (threadIdx.x == 0) { out[2 * GK] = tot; out[2 * GK + 1] = nnz; }
  if (last_arriver(q.cnt, gridDim.x, &s_last)) {
    const int nw = (int)gridDim.x;
    // slab entry k -> trace row: counts and ssq follow the 12 header values, nnz is header value
    // 11, the total goes behind the row
    auto dst = [&](int k) { return k < 2 * GK ? 12 + k : (k == 2 * GK ? q.width : 11); };
    if (SW <= 64) {
      const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
      for (int k = wv; k < SW; k += 4) {
        double acc = 0.0;
        for (int w = lane; w < nw; w += 64) acc += q.mslab[(int64_t)w * SW + k];
        acc = wave_sum(acc);
        if (lane == 0) q.row[dst(k)] = acc;
      }
    } else {
      for (int k = threadIdx.x; k < SW; k += 256) {
        double acc = 0.0;
        for (int w = 0; w < nw; ++w) acc += q.mslab[(int64_t)w * SW + k];
        q.row[dst(k)] = acc;
      }
    }
    if (threadIdx.x == 0) {
      const Scal *sc = d.sc;
      q.row[0] = iteration;
      q.row[1] = sc->mu;
      q.row[2] = sc->sigmaE;
      q.row[3] = hs ? 0.0 : d.sigmaGG[0];  // (the Horseshoe has no sigmaG: its buffer is never written)
      q.row[4] = sc->sigmaF;
      q.row[5] = sc->tau;
      q.row[6] = sc->eta;
      q.row[7] = sc->c2;
      q.row[8] = d.stats[0];
      *q.cnt = 0;
    }
  }
}

// one window's update from its sum beta^2 and "a marker is in the model" (one thread)
__device__ __forceinline__ void summary_window_update(const SumDev &q, int64_t w, double ssq, bool any, double total,
                                                      double n) {
#pragma clang fp contract(off)
  if (any) q.wany[w] += 1u;
  const double share = total > 0.0 ? ssq / total : 0.0;
  const double a = q.wssq[w], b = q.wshare[w];
  q.wssq[w] = a + (ssq - a) / n;
  q.wshare[w] = b + (share - b) / n;
}

// FORM 0: a thread per window (W <= SUM_W_THREAD), grid cdiv(nW, 256); 1: a wave per window
// (W <= SUM_W_WAVE), grid cdiv(nW, 4); 2: a workgroup per window, grid nW.  Runs after
// k_summary_markers on the same stream: q.row[q.width] is this sweep's total sum beta^2.
template <int FORM>
__global__ __launch_bounds__(256) void k_summary_windows(Dev d, SumDev q, double n) {
#pragma clang fp contract(off)
  __shared__ double red[8];
  const bool hs = d.model == MODEL_HORSESHOE;
  const double total = q.row[q.width];
  const int lane = threadIdx.x & 63;
  int64_t w;
  int first, step;
  if (FORM == 0) { w = (int64_t)blockIdx.x * 256 + threadIdx.x; first = 0; step = 1; }
  else if (FORM == 1) { w = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); first = lane; step = 64; }
  else { w = blockIdx.x; first = threadIdx.x; step = 256; }
  const bool live = w < q.nW;  // (uniform over a wave in form 1, over the workgroup in form 2)
  double ssq = 0.0, in = 0.0;
  if (live) {
    const int64_t m0 = w * q.W, m1 = m0 + q.W < d.M ? m0 + q.W : d.M;
    for (int64_t m = m0 + first; m < m1; m += step) {
      const double b = d.beta[m];
      ssq += b * b;
      if (hs ? b != 0.0 : d.comp[m] > 0) in = 1.0;
    }
  }
  if (FORM == 1) { ssq = wave_sum(ssq); in = wave_sum(in); }
  if (FORM == 2) { ssq = block_sum<256>(ssq, red); in = block_sum<256>(in, red); }
  const bool writer = FORM == 0 ? true : (FORM == 1 ? lane == 0 : threadIdx.x == 0);
  if (live && writer) summary_window_update(q, w, ssq, in > 0.0, total, n);
}

__global__ __launch_bounds__(256) void k_summary_rows(Dev d, SumDev q, double n) {
#pragma clang fp contract(off)
  __shared__ double red[8];
  __shared__ int s_last;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const bool valid = i < d.N;  // rows of the padded ld beyond N take no part
  double g = 0.0;
  if (valid) {
    double fa = 0.0;
    for (int c = 0; c < d.F; ++c) fa += d.fixed[(int64_t)c * d.N + i] * d.alpha[c];
    g = ((q.Y[i] - d.sc->mu) - d.eps[i]) - fa;
    double mean = q.gmean[i];
    const double dl = g - mean;
    mean += dl / n;
    q.gM2[i] += dl * (g - mean);
    q.gmean[i] = mean;
  }
  // this workgroup's (rows, mean, centred M2)
  const int64_t left = d.N - (int64_t)blockIdx.x * 256;
  const double nv = (double)(left < 256 ? left : 256);
  const double mw = block_sum<256>(g, red) / nv;
  const double dv = valid ? g - mw : 0.0;
  const double m2w = block_sum<256>(dv * dv, red);
  if (threadIdx.x == 0) {
    double *o = q.rslab + (int64_t)blockIdx.x * 3;
    o[0] = nv; o[1] = mw; o[2] = m2w;
  }
  if (last_arriver(q.cnt + 1, gridDim.x, &s_last)) {
    // the many-way Chan merge in a fixed order: gbar = sum n_w mean_w / N, then
    // M2 = sum (M2_w + n_w (mean_w - gbar)^2) -- centred, no sum g^2 - N gbar^2
    const int nw = (int)gridDim.x;
    double a = 0.0;
    for (int w = threadIdx.x; w < nw; w += 256) a += q.rslab[(int64_t)w * 3] * q.rslab[(int64_t)w * 3 + 1];
    const double gbar = block_sum<256>(a, red) / (double)d.N;
    double b = 0.0;
    for (int w = threadIdx.x; w < nw; w += 256) {
      const double dm = q.rslab[(int64_t)w * 3 + 1] - gbar;
      b += q.rslab[(int64_t)w * 3 + 2] + q.rslab[(int64_t)w * 3] * (dm * dm);
    }
    const double M2 = block_sum<256>(b, red);
    if (threadIdx.x == 0) {
      const double var = d.N > 1 ? M2 / (double)(d.N - 1) : 0.0;
      const double den = var + d.sc->sigmaE;
      q.row[9] = var;
      q.row[10] = den > 0.0 ? var / den : 0.0;
      q.cnt[1] = 0;
    }
  }
}

// restart sessions hold no Y: Yrec = (mu + (X beta + F alpha)) + eps from the state at summary_begin
// (y holds k_linpred's output on entry)
__global__ __launch_bounds__(256) void k_summary_yrec(Dev d, double *y) {
#pragma clang fp contract(off)
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < d.N) y[i] = (d.sc->mu + y[i]) + d.eps[i];
}
