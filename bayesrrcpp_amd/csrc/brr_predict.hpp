// brr_predict.hpp -- out-of-sample prediction on the device (brr_session_predict_*, include/brr.h).
//
// Included by brr_kernels.hip inside namespace brr (it uses block_sum / last_arriver).  A
// target cohort of N2 rows is scored against a beta of the session's M markers, g2 = X2 beta, by two
// launches on the session stream:
//
//   k_predict_score  a workgroup owns a row tile and a chunk of PRED_CHUNK consecutive markers.  It
//                    loads the chunk's beta, compacts the non-zero entries into LDS in index order
//                    (index, beta, the column's value table) and walks that list: per listed column a
//                    thread reads its rows as one word (2-bit codes: 4 bytes = 16 rows, a wave 256
//                    contiguous bytes) or one float4 (f32 storage) and accumulates
//                    acc = acc + (double)x * b, product and sum rounded separately.  The chunk's
//                    partial sums go to part[chunk][row].
//   k_predict_rows   one thread per target row: the chunk partials left-folded in chunk order give g2;
//                    folding a kept sweep adds the Welford update of g2's mean / M2 and the trace
//                    row's moments as the many-way Chan merge of the workgroups' (rows, mean, centred
//                    M2, co-moment) -- never sum g^2 - N gbar^2.
//
// The order of every sum of a row's score is a function of M and PRED_CHUNK only: columns ascending
// inside a chunk, zeros of beta skipped, chunks ascending.  So two runs, the two target storages of the
// same values, and any N2 or launch shape give a row the same bits.  No floating-point atomics;
// nothing here writes chain state.
#pragma once

// rows of one thread: a 4-byte word of 2-bit codes, or a float4
template <bool BITS2>
struct PredTile {
  static constexpr int R = BITS2 ? 16 : 4;
  static constexpr int ROWS = 256 * R;  // rows per workgroup (BITS2: PRED_ROWS)
};

template <bool BITS2>
__global__ __launch_bounds__(256) void k_predict_score(PredDev p, const double *beta) {
#pragma clang fp contract(off)
  constexpr int R = PredTile<BITS2>::R;
  constexpr int NP8 = PRED_CHUNK / 256;  // chunk entries per thread
  __shared__ double s_b[PRED_CHUNK];
  __shared__ float4 s_tab[BITS2 ? PRED_CHUNK : 1];
  __shared__ unsigned short s_idx[PRED_CHUNK];
  __shared__ int s_wn[NP8][4];
  __shared__ double s_t[8][4];  // 2-bit codes: the current eight columns' products f64(table[code]) * beta
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  const int64_t m0 = (int64_t)blockIdx.y * PRED_CHUNK;
  // the chunk's beta; its non-zero entries compacted in index order: entry e = k 256 + t lies behind
  // every non-zero entry of an earlier (k, wave) and of the lower lanes of its own wave
  double b[NP8];
  unsigned long long mask[NP8];
#pragma unroll
  for (int k = 0; k < NP8; ++k) {
    const int64_t m = m0 + k * 256 + t;
    b[k] = m < p.M ? beta[m] : 0.0;
    mask[k] = __ballot(b[k] != 0.0);
    if (lane == 0) s_wn[k][wv] = __popcll(mask[k]);
  }
  __syncthreads();
  int off[NP8] = {}, n = 0;
#pragma unroll
  for (int k = 0; k < NP8; ++k)
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      if (w == wv) off[k] = n;
      n += s_wn[k][w];
    }
#pragma unroll
  for (int k = 0; k < NP8; ++k)
    if (b[k] != 0.0) {
      const int pos = off[k] + __popcll(mask[k] & ((1ull << lane) - 1ull));
      s_idx[pos] = (unsigned short)(k * 256 + t);
      s_b[pos] = b[k];
      if (BITS2) s_tab[pos] = *reinterpret_cast<const float4 *>(p.table + 4 * (m0 + k * 256 + t));
    }
  __syncthreads();
  const int64_t row0 = (int64_t)blockIdx.x * PredTile<BITS2>::ROWS + (int64_t)R * t;
  const bool live = row0 < p.NP;  // (NP is a multiple of 16: a thread's rows are all inside or all outside)
  if (!BITS2 && !live) return;    // (the 2-bit walk has workgroup barriers)
  double acc[R];
#pragma unroll
  for (int r = 0; r < R; ++r) acc[r] = 0.0;
  // the listed columns in ascending order, eight loads in flight
  for (int i = 0; i < n; i += 8) {
    if (BITS2) {
      // A column has four values, so it has four products x * b: 32 threads form the eight columns'
      // (the same correctly rounded f64(x) * b a row would form) and a row's term is an LDS read
      // indexed by its code, all lanes on the same four addresses of a column (broadcast reads).
      uint32_t w[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        w[u] = 0u;
        if (live && i + u < n)
          w[u] = *reinterpret_cast<const uint32_t *>(p.codes + (m0 + s_idx[i + u]) * p.ldc + (row0 >> 2));
      }
      __syncthreads();  // the previous eight columns' products have been read
      if (t < 32 && i + (t >> 2) < n)
        s_t[t >> 2][t & 3] = (double)reinterpret_cast<const float *>(&s_tab[i + (t >> 2)])[t & 3] * s_b[i + (t >> 2)];
      __syncthreads();
      if (live) {
#pragma unroll
        for (int u = 0; u < 8; ++u)
          if (i + u < n) {
#pragma unroll
            for (int r = 0; r < R; ++r) acc[r] = acc[r] + s_t[u][(w[u] >> (2 * r)) & 3u];
          }
      }
    } else {
      float4 x[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        x[u] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (i + u < n) x[u] = *reinterpret_cast<const float4 *>(p.X + (m0 + s_idx[i + u]) * p.ld + row0);
      }
#pragma unroll
      for (int u = 0; u < 8; ++u)
        if (i + u < n) {
          const double bb = s_b[i + u];
          acc[0] = acc[0] + (double)x[u].x * bb;
          acc[1] = acc[1] + (double)x[u].y * bb;
          acc[2] = acc[2] + (double)x[u].z * bb;
          acc[3] = acc[3] + (double)x[u].w * bb;
        }
    }
  }
  if (!live) return;
  double *out = p.part + (int64_t)blockIdx.y * p.NP + row0;
#pragma unroll
  for (int r = 0; r < R; r += 2) *reinterpret_cast<double2 *>(out + r) = make_double2(acc[r], acc[r + 1]);
}

// FOLD = false: the scores only (brr_session_predict_score).  FOLD = true: kept sweep number n
// (1-based) into the accumulators, and the trace row of `iteration`.
template <bool FOLD>
__global__ __launch_bounds__(256) void k_predict_rows(PredDev p, Dev d, double n, double iteration) {
#pragma clang fp contract(off)
  __shared__ double red[8];
  __shared__ int s_last;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const bool valid = i < p.N2;
  double g = 0.0;
  if (valid) {
    for (int c = 0; c < p.nchunk; ++c) g = g + p.part[(int64_t)c * p.NP + i];
    p.g[i] = g;
  }
  if (!FOLD) return;
  const bool hasy = p.Y2 != nullptr;
  const double mu = d.sc->mu;
  double y = 0.0, res = 0.0;
  if (valid) {
    double mean = p.gmean[i];
    const double dl = g - mean;
    mean += dl / n;
    p.gM2[i] += dl * (g - mean);
    p.gmean[i] = mean;
    if (hasy) {
      y = p.Y2[i];
      res = (y - mu) - g;
    }
  }
  // this workgroup's rows, means, centred second moments and co-moment
  const int64_t left = p.N2 - (int64_t)blockIdx.x * 256;
  const double nv = (double)(left < 256 ? left : 256);
  const double mg = block_sum<256>(g, red) / nv;
  const double my = block_sum<256>(y, red) / nv;
  const double dg = valid ? g - mg : 0.0, dy = valid ? y - my : 0.0;
  const double m2g = block_sum<256>(dg * dg, red);
  const double m2y = block_sum<256>(dy * dy, red);
  const double cyg = block_sum<256>(dy * dg, red);
  const double sse = block_sum<256>(res * res, red);
  if (threadIdx.x == 0) {
    double *o = p.rslab + (int64_t)blockIdx.x * PRED_SLAB;
    o[0] = nv; o[1] = mg; o[2] = m2g; o[3] = my; o[4] = m2y; o[5] = cyg; o[6] = sse;
  }
  if (last_arriver(p.cnt, gridDim.x, &s_last)) {
    // the many-way Chan merge in a fixed order: the grand means, then the centred moments about them
    const int nw = (int)gridDim.x;
    double a = 0.0, b = 0.0;
    for (int w = threadIdx.x; w < nw; w += 256) {
      const double *o = p.rslab + (int64_t)w * PRED_SLAB;
      a += o[0] * o[1];
      b += o[0] * o[3];
    }
    const double gbar = block_sum<256>(a, red) / (double)p.N2;
    const double ybar = block_sum<256>(b, red) / (double)p.N2;
    double sg = 0.0, sy = 0.0, sc = 0.0, se = 0.0;
    for (int w = threadIdx.x; w < nw; w += 256) {
      const double *o = p.rslab + (int64_t)w * PRED_SLAB;
      const double eg = o[1] - gbar, ey = o[3] - ybar;
      sg += o[2] + o[0] * (eg * eg);
      sy += o[4] + o[0] * (ey * ey);
      sc += o[5] + o[0] * (ey * eg);
      se += o[6];
    }
    const double M2g = block_sum<256>(sg, red);
    const double M2y = block_sum<256>(sy, red);
    const double Cyg = block_sum<256>(sc, red);
    const double SSE = block_sum<256>(se, red);
    if (threadIdx.x == 0) {
      const double dof = (double)(p.N2 - 1);
      const double vg = p.N2 > 1 ? M2g / dof : 0.0;
      const double vy = p.N2 > 1 ? M2y / dof : 0.0;
      const double cov = p.N2 > 1 ? Cyg / dof : 0.0;
      const double nan = __longlong_as_double(0x7ff8000000000000ll);
      p.row[0] = iteration;
      p.row[1] = gbar;
      p.row[2] = vg;
      p.row[3] = hasy ? ybar : nan;
      p.row[4] = hasy ? vy : nan;
      p.row[5] = hasy ? cov : nan;
      p.row[6] = hasy ? ((vy > 0.0 && vg > 0.0) ? cov / sqrt(vy * vg) : 0.0) : nan;
      p.row[7] = hasy ? SSE / (double)p.N2 : nan;
      *p.cnt = 0;
    }
  }
}
