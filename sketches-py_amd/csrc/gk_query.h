// gk_query.h -- the table query shared by the kernel units: numpy's linear
// percentile (small n) and wave_quantiles.  Consumers: k_ingest / k_ingest_big
// (gk_kernels.hip, the <1, 1> instance over the split arrays; small_quantiles
// there uses percentile_linear_at) and k_query_list / k_select_query
// (gk_ops.hip, the <2, 4> instance over GKRec tables).  wave_quantiles is
// noinline: each instance must be one function of one unit, which is why the
// two kernels that share <2, 4> sit in the same unit.
#pragma once
#include "gk_dev.h"

// ===========================================================================
// Quantiles of one stream from its table (gk:156-232), wave-parallel.
//   large n: the reference walks i = 0.. while prefix_g(i) + d_i - 1 <=
//   rank + spread; the first i that breaks is the number of i whose RUNNING
//   MAX of prefix_g + d - 1 is <= rank + spread (the running max is
//   monotone), so each q is one count over the table.
//   small n (n < 1/eps, gk:169): numpy.percentile(values, q*100), linear.
// qmode 0 (quantiles, sorted qs): no break -> _max (gk:225-230)
// qmode 1 (quantile / unsorted qs): no break -> entries[-1].val (gk:185)
// ===========================================================================
__device__ __forceinline__ double gk_nan() { return __longlong_as_double(0x7ff8000000000000LL); }

// SV / SI: element strides of the value / g,d arrays (1 for the split
// arrays of the large classes, 2 / 4 for the GKRec table of the 256 class)
template <typename At>
__device__ __forceinline__ double percentile_linear_at(int E, double q, At at) {
  // numpy 2.2.6 _function_base_impl.py: q/100 (l.4257), (n-1)*q (l.107),
  // bounds (l.4748-4750), gamma (l.4632), _lerp (l.4653-4657)
  const double qq = (q * 100.0) / 100.0;
  const double vi = (double)(E - 1) * qq;
  double prev;
  double a, b;
  if (vi >= (double)(E - 1)) {
    prev = -1.0;
    a = at(E - 1);
    b = a;
  } else if (vi < 0.0) {
    prev = 0.0;
    a = at(0);
    b = a;
  } else {
    prev = floor(vi);
    const int pi = (int)prev;
    a = at(pi);
    b = at(pi + 1);
  }
  const double gamma = vi - prev;
  const double diff = b - a;
  if (gamma >= 0.5) return b - diff * (1.0 - gamma);
  return a + diff * gamma;
}

template <int SV>
__device__ double percentile_linear_arr(const double* __restrict__ tv, int E, double q) {
  return percentile_linear_at(E, q, [&](int i) { return tv[i * SV]; });
}

template <int SV, int SI>
__device__ __attribute__((noinline)) void wave_quantiles(const double* __restrict__ tv, const int32_t* __restrict__ tg,
                               const int32_t* __restrict__ td, int E, int64_t n, double mn, double mx,
                               const GKState& st, const double* __restrict__ qs, int nq, int qmode,
                               double* __restrict__ out, int lane) {
  if (n == 0 || E == 0) {
    for (int q = lane; q < nq; q += 64) out[q] = gk_nan();
    return;
  }
  if ((double)n < st.inv_eps) {  // gk:169 / gk:200
    for (int q = lane; q < nq; q += 64) {
      const double qv = qs[q];
      out[q] = (qv >= 0.0 && qv <= 1.0) ? percentile_linear_arr<SV>(tv, E, qv) : gk_nan();
    }
    return;
  }
  const int K = (E + 63) >> 6;
  const int j0 = lane * K;
  const int jend = min(j0 + K, E);
  int64_t bsum = 0;
  for (int j = j0; j < jend; ++j) bsum += tg[j * SI];
  const int64_t bex = wave_incl_scan_i64(bsum, lane) - bsum;
  int64_t acc = bex, bmax = INT64_MIN;
  for (int j = j0; j < jend; ++j) {
    acc += tg[j * SI];
    const int64_t a = acc + td[j * SI] - 1;
    if (a > bmax) bmax = a;
  }
  const int64_t pmax_incl = wave_incl_max_i64(bmax, lane);
  int64_t pmax_ex = __shfl_up(pmax_incl, 1, 64);
  if (lane == 0) pmax_ex = INT64_MIN;
  const int64_t spread = (int64_t)(st.eps * (double)(n - 1));  // gk:174 / gk:210
  for (int q = 0; q < nq; ++q) {
    const double qv = qs[q];
    const bool valid = (qv >= 0.0 && qv <= 1.0);
    const int64_t rank = valid ? (int64_t)(qv * (double)(n - 1) + 1.0) : 0;  // gk:173
    const int64_t th = rank + spread;
    int c = 0;
    int64_t run = pmax_ex, a2 = bex;
    for (int j = j0; j < jend; ++j) {
      a2 += tg[j * SI];
      const int64_t a = a2 + td[j * SI] - 1;
      if (a > run) run = a;
      c += (run <= th) ? 1 : 0;
    }
    const int i = wave_sum_i32(c);
    if (lane == 0) {
      double r;
      if (!valid) r = gk_nan();
      else if (i == 0) r = mn;                          // gk:182-183 / gk:220
      else if (i < E) r = tv[(i - 1) * SV];                    // gk:185 / gk:220
      else r = (qmode == 0) ? mx : tv[(E - 1) * SV];           // gk:229 / gk:185
      out[q] = r;
    }
  }
}
