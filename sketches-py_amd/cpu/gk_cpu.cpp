// gk_cpu.cpp -- the host (CPU) engine of the batched GKArray: every entry
// point of include/gk_capi.h on host memory (include/gk_cpu.h), streams in
// parallel on host threads, each stream strictly in insertion order.
//
// Reference: githomin/sketches-py gkarray/gkarray.py ("gk:N" = line N).  It is
// an independent implementation (not the test oracle): the add-driven flush
// uses the closed form of the four-rule walk (SURVEY.md 3.2 -- gap counts
// against the old table, one integer carry per entry), merges use the
// general walk (gk:76-106).  Built with -ffp-contract=off, no fast-math: the
// reference's float64 expressions (gk:54, gk:70, numpy's linear percentile)
// are evaluated exactly as written.
#include <math.h>
#include <sched.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <limits>
#include <set>
#include <string>
#include <thread>

#include "gk_host_stats.h"
#include <vector>

#include "gk_cpu.h"
#include "gk_checks.h"
#include "gk_dirhash.h"
#include "gk_format.h"
#include "gk_pack.h"

namespace {

// one (v, g, delta) tuple of a table (gk:8-16)
struct Rec {
  double v;
  int64_t g;
  int64_t d;
};

struct Stream {
  int64_t n = 0;                                        // _n (gk:27)
  double mn = std::numeric_limits<double>::infinity();  // _min (gk:25)
  double mx = -std::numeric_limits<double>::infinity(); // _max (gk:26)
  double sum = 0.0, avg = 0.0;                          // _sum, _avg (gk:28-29)
  std::vector<Rec> tab;                                 // entries (gk:23)
  std::vector<double> pend;                             // incoming (gk:24)
};

int default_threads() {
  if (const char* e = getenv("GK_CPU_THREADS")) {
    const int t = atoi(e);
    if (t > 0) return t;
  }
  cpu_set_t cs;
  if (sched_getaffinity(0, sizeof(cs), &cs) == 0) {
    const int n = CPU_COUNT(&cs);
    if (n > 0) return n;
  }
  const unsigned hc = std::thread::hardware_concurrency();
  return hc ? (int)hc : 1;
}

// Run fn(s) for s in [0, S): dynamic chunks of streams over `threads` threads.
template <typename F>
void parallel_for(int64_t S, int threads, F&& fn) {
  constexpr int64_t kChunk = 64;
  const int64_t chunks = (S + kChunk - 1) / kChunk;
  const int T = (int)std::max<int64_t>(1, std::min<int64_t>(threads, chunks));
  if (T <= 1) {
    for (int64_t s = 0; s < S; ++s) fn(s);
    return;
  }
  std::atomic<int64_t> next{0};
  auto worker = [&]() {
    for (;;) {
      const int64_t c = next.fetch_add(1, std::memory_order_relaxed);
      if (c >= chunks) break;
      const int64_t e = std::min(S, (c + 1) * kChunk);
      for (int64_t s = c * kChunk; s < e; ++s) fn(s);
    }
  };
  std::vector<std::thread> pool;
  pool.reserve(T - 1);
  for (int t = 1; t < T; ++t) pool.emplace_back(worker);
  worker();
  for (auto& t : pool) t.join();
}

}  // namespace

struct gk_set {
  int64_t S = 0;
  double eps = 0;
  int64_t P = 0;  // int(1.0/eps) + 1 (gk:60)
  int threads = 1;
  std::vector<Stream> st;
  bool timing = false;
  double ingest_ms = 0;
  int64_t launches = 0;
  gk_set* fold_scratch = nullptr;  // gk_fold_packed (made on first use)
  // gk_ingest_keyed: the grouped batch (only grows)
  std::vector<double> key_vals;
  std::vector<int64_t> key_offs;
  // gk_rank_ingest_keyed: the sample index of every grouped position (only grows)
  std::vector<int64_t> key_idx;
};

namespace {

// ---- float64 control arithmetic, exactly the reference's expressions -------
int64_t threshold(const gk_set* h, int64_t n) {
  return (int64_t)floor(2.0 * h->eps * (double)(n - 1));  // gk:70: (2.0*eps)*(n-1)
}

// gk:52-59 for one value
inline void add_stats(Stream& s, double v) { gk_host_stat_step(s.n, s.sum, s.avg, s.mn, s.mx, v); }

// Stable order of the pending values by value (gk:71-72: Python's sorted();
// -0.0 == +0.0, so equal keys keep insertion order): sorted by (value,
// insertion index), which is the stable order, with no allocation.
struct Keyed {
  double v;
  uint32_t i;
};
inline bool keyed_less(const Keyed& a, const Keyed& b) { return a.v < b.v || (!(b.v < a.v) && a.i < b.i); }

void sorted_pending(const std::vector<double>& pend, std::vector<Keyed>& key, std::vector<double>& out) {
  const size_t n = pend.size();
  out.resize(n);
  if (n <= 24) {  // insertion sort is stable
    for (size_t i = 0; i < n; ++i) {
      const double x = pend[i];
      size_t j = i;
      while (j > 0 && x < out[j - 1]) {
        out[j] = out[j - 1];
        --j;
      }
      out[j] = x;
    }
    return;
  }
  key.resize(n);
  for (size_t i = 0; i < n; ++i) key[i] = Keyed{pend[i], (uint32_t)i};
  std::sort(key.begin(), key.end(), keyed_less);
  for (size_t i = 0; i < n; ++i) out[i] = key[i].v;
}

// merge_compress() of an add-driven flush (gk:63-109 with every incoming record
// (x, 1, 0)), in closed form: entry j, with carry c from a removed
// predecessor, absorbs the k = clamp(T - d_j - (g_j + c), 0, m_j) smallest of
// the m_j values of its gap [v_{j-1}, v_j) (gk:93-95); the others are kept as
// (x, 1, G + d_j - 1), G = g_j + c + k (gk:96-98); entry j is removed into j+1
// iff G + g_{j+1} + d_{j+1} <= T (gk:100-103), else kept as (v_j, G, d_j).  The
// values past the last entry chain in runs of max(T, 1) (gk:85-92).
void flush_add(Stream& s, int64_t T, std::vector<Keyed>& key, std::vector<double>& xs, std::vector<Rec>& out) {
  sorted_pending(s.pend, key, xs);
  const std::vector<Rec>& E = s.tab;
  const size_t ne = E.size(), nx = xs.size();
  out.clear();
  out.reserve(ne + nx);
  size_t i = 0;
  int64_t carry = 0;
  for (size_t j = 0; j < ne; ++j) {
    const double vj = E[j].v;
    size_t m = 0;
    while (i + m < nx && xs[i + m] < vj) ++m;  // gk:93: strict, ties go after the entry
    const int64_t Gp = E[j].g + carry;
    const int64_t k = std::min<int64_t>((int64_t)m, std::max<int64_t>(0, T - E[j].d - Gp));
    const int64_t G = Gp + k;
    for (size_t t = i + (size_t)k; t < i + m; ++t) out.push_back(Rec{xs[t], 1, G + E[j].d - 1});
    i += m;
    if (j + 1 < ne && G + E[j + 1].g + E[j + 1].d <= T) {
      carry = G;
    } else {
      out.push_back(Rec{vj, G, E[j].d});
      carry = 0;
    }
  }
  int64_t c = 0;
  for (; i < nx; ++i) {
    c += 1;
    if (i + 1 == nx || c + 1 > T) {
      out.push_back(Rec{xs[i], c, 0});
      c = 0;
    }
  }
  s.tab.swap(out);
  s.pend.clear();
}

// merge_compress(entries) with explicit records (gk:63-109): the general
// four-rule walk over the stable order of incoming (pending values as
// (x, 1, 0), then the records, gk:71) and the table.
void flush_general(Stream& s, int64_t T, const Rec* recs, size_t nrec, std::vector<Keyed>& key, std::vector<Rec>& inc,
                   std::vector<Rec>& out) {
  // incoming = pending (x, 1, 0) + records, in that order (gk:71), stably sorted
  const size_t np = s.pend.size(), ntot = np + nrec;
  key.resize(ntot);
  for (size_t i = 0; i < ntot; ++i) key[i] = Keyed{i < np ? s.pend[i] : recs[i - np].v, (uint32_t)i};
  std::sort(key.begin(), key.end(), keyed_less);
  inc.resize(ntot);
  for (size_t k = 0; k < ntot; ++k) {
    const uint32_t i = key[k].i;
    inc[k] = i < np ? Rec{s.pend[i], 1, 0} : recs[i - np];
  }
  std::vector<Rec>& E = s.tab;
  const size_t ni = inc.size(), ne = E.size();
  out.clear();
  out.reserve(ni + ne);
  size_t i = 0, j = 0;
  while (i < ni || j < ne) {
    if (i == ni || (j < ne && !(inc[i].v < E[j].v))) {  // gk:77-84, gk:100-106
      if (j + 1 < ne && E[j].g + E[j + 1].g + E[j + 1].d <= T) E[j + 1].g += E[j].g;
      else out.push_back(E[j]);
      ++j;
    } else if (j == ne) {  // gk:85-92
      if (i + 1 < ni && inc[i].g + inc[i + 1].g + inc[i + 1].d <= T) inc[i + 1].g += inc[i].g;
      else out.push_back(inc[i]);
      ++i;
    } else {  // gk:93-99: inc[i].v < E[j].v
      if (inc[i].g + E[j].g + E[j].d <= T) {
        E[j].g += inc[i].g;
      } else {
        Rec r = inc[i];
        r.d = E[j].g + E[j].d - r.g;
        out.push_back(r);
      }
      ++i;
    }
  }
  s.tab.swap(out);
  s.pend.clear();
}

struct Scratch {
  std::vector<Keyed> key;
  std::vector<double> xs;
  std::vector<Rec> out, inc;
};
thread_local Scratch tl_scratch;

// GKArray.add for a run of values (gk:49-61): a flush whenever n reaches a
// multiple of P (counted down instead of a modulo per value).
void ingest_stream(const gk_set* h, Stream& s, const double* x, int64_t L) {
  Scratch& sc = tl_scratch;
  int64_t k = 0;
  while (k < L) {
    const int64_t need = h->P - s.n % h->P;  // adds until the next flush point (gk:60)
    const int64_t take = std::min(need, L - k);
    for (int64_t t = 0; t < take; ++t) {
      const double v = x[k + t];
      add_stats(s, v);
      s.pend.push_back(v);
    }
    k += take;
    if (take == need) flush_add(s, threshold(h, s.n), sc.key, sc.xs, sc.out);
  }
}

// merge_compress() where values are pending (size/quantile, gk:45-46, 166, 197)
void flush_if_pending(const gk_set* h, Stream& s) {
  if (!s.pend.empty()) flush_add(s, threshold(h, s.n), tl_scratch.key, tl_scratch.xs, tl_scratch.out);
}

// numpy 2.2.6 percentile(values, q*100), method 'linear' (gk:171, gk:202):
// q/100 (np:4257), virtual index (n-1)*q (np:107), bounds (np:4748-4750),
// gamma (np:4632), _lerp with its gamma >= 0.5 branch (np:4653-4657)
double percentile_linear(const std::vector<Rec>& E, double q) {
  const int64_t n = (int64_t)E.size();
  const double qq = (q * 100.0) / 100.0;
  const double vi = (double)(n - 1) * qq;
  double prev, a, b;
  if (vi >= (double)(n - 1)) {
    prev = -1.0;
    a = b = E[n - 1].v;
  } else if (vi < 0.0) {
    prev = 0.0;
    a = b = E[0].v;
  } else {
    prev = floor(vi);
    const int64_t pi = (int64_t)prev;
    a = E[pi].v;
    b = E[pi + 1].v;
  }
  const double gamma = vi - prev;
  const double diff = b - a;
  if (gamma >= 0.5) return b - diff * (1.0 - gamma);
  return a + diff * gamma;
}

double nan_value() { return std::numeric_limits<double>::quiet_NaN(); }

// GKArray.quantile(q) (gk:156-185) after the flush
double quantile_one(const gk_set* h, const Stream& s, double q) {
  if (q < 0 || q > 1 || s.n == 0) return nan_value();
  if ((double)s.n < 1.0 / h->eps) return percentile_linear(s.tab, q);
  const int64_t rank = (int64_t)(q * (double)(s.n - 1) + 1);  // gk:173
  const int64_t spread = (int64_t)(h->eps * (double)(s.n - 1));  // gk:174
  double g_sum = 0.0;
  size_t i = 0;
  for (; i < s.tab.size(); ++i) {
    g_sum += (double)s.tab[i].g;
    if (g_sum + (double)s.tab[i].d - 1 > (double)(rank + spread)) break;
  }
  if (i == 0) return s.mn;
  return s.tab[i - 1].v;
}

// GKArray.quantiles(qs) (gk:187-232) after the flush, qs sorted
void quantiles_list(const gk_set* h, const Stream& s, const double* qs, int nq, double* out) {
  if (s.n == 0) {
    for (int k = 0; k < nq; ++k) out[k] = nan_value();
    return;
  }
  if ((double)s.n < 1.0 / h->eps) {  // gk:200-202
    for (int k = 0; k < nq; ++k) out[k] = (qs[k] >= 0 && qs[k] <= 1) ? percentile_linear(s.tab, qs[k]) : nan_value();
    return;
  }
  const int64_t spread = (int64_t)(h->eps * (double)(s.n - 1));  // gk:210
  double g_sum = 0.0;
  size_t i = 0;
  int j = 0;
  while (i < s.tab.size() && j < nq) {  // gk:213-224
    g_sum += (double)s.tab[i].g;
    while (j < nq) {
      if (qs[j] < 0 || qs[j] > 1) {
        out[j++] = nan_value();
      } else if (g_sum + (double)s.tab[i].d - 1 > (double)((int64_t)(qs[j] * (double)(s.n - 1) + 1) + spread)) {
        out[j++] = i == 0 ? s.mn : s.tab[i - 1].v;
      } else {
        break;
      }
    }
    ++i;
  }
  for (; j < nq; ++j) out[j] = (qs[j] < 0 || qs[j] > 1) ? nan_value() : s.mx;  // gk:225-230
}

// gk:205: an unsorted list is answered q by q with quantile()
int effective_mode(const double* qs, int nq, int mode) {
  if (mode == GK_Q_LIST)
    for (int i = 1; i < nq; ++i)
      if (qs[i] < qs[i - 1]) return GK_Q_SINGLE;
  return mode;
}

void answer(const gk_set* h, const Stream& s, const double* qs, int nq, int mode, double* out) {
  if (mode == GK_Q_SINGLE) {
    for (int k = 0; k < nq; ++k) out[k] = quantile_one(h, s, qs[k]);
  } else {
    quantiles_list(h, s, qs, nq, out);
  }
}

int ingest_impl(gk_set* h, const double* values, const int64_t* offsets, const double* qs, int nq, double* out,
                int mode) {
  if (!offsets) return fail(GK_E_ARG, "offsets is null");
  if (!values) return fail(GK_E_ARG, "values is null");
  for (int64_t s = 0; s < h->S; ++s)
    if (offsets[s + 1] < offsets[s]) return fail(GK_E_ARG, "offsets must be non-decreasing");
  const auto t0 = std::chrono::steady_clock::now();
  parallel_for(h->S, h->threads, [&](int64_t s) {
    Stream& st = h->st[s];
    ingest_stream(h, st, values + offsets[s], offsets[s + 1] - offsets[s]);
    if (qs) {
      if (nq > 0 && st.n > 0) flush_if_pending(h, st);  // gk:166-167 / gk:197-198
      answer(h, st, qs, nq, mode, out + s * (int64_t)nq);
    }
  });
  if (h->timing) {
    h->ingest_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    h->launches += 1;
  }
  return GK_OK;
}

// GKArray.merge(other) (gk:111-154) for one stream
void merge_stream(const gk_set* h, Stream& a, Stream& b, std::vector<Rec>& conv) {
  Scratch& sc = tl_scratch;
  if (b.n == 0) {  // gk:121-123: unconditional flush of self
    flush_general(a, threshold(h, a.n), nullptr, 0, sc.key, sc.inc, sc.out);
    return;
  }
  if (a.n == 0) {  // gk:125-133: other flushed, self takes a copy of its state
    flush_general(b, threshold(h, b.n), nullptr, 0, sc.key, sc.inc, sc.out);
    a.tab = b.tab;
    a.mn = b.mn;
    a.mx = b.mx;
    a.n = b.n;
    a.sum = b.sum;
    a.avg = b.avg;
    return;
  }
  const int64_t spread = (int64_t)(h->eps * (double)(b.n - 1));  // gk:136 (before the flush)
  flush_general(b, threshold(h, b.n), nullptr, 0, sc.key, sc.inc, sc.out);  // gk:137
  conv.clear();
  const std::vector<Rec>& E = b.tab;
  const size_t L = E.size();
  int64_t g = E[0].g + E[0].d - spread - 1;  // gk:138-140
  if (g > 0) conv.push_back(Rec{b.mn, g, 0});
  for (size_t i = 0; i + 1 < L; ++i) {  // gk:141-144
    g = E[i + 1].g + E[i + 1].d - E[i].d;
    if (g > 0) conv.push_back(Rec{E[i].v, g, 0});
  }
  g = spread + 1 - E[L - 1].d;  // gk:145-147
  if (g > 0) conv.push_back(Rec{E[L - 1].v, g, 0});
  a.n += b.n;                    // gk:149 (_sum/_avg are not merged)
  if (b.mn < a.mn) a.mn = b.mn;  // gk:151: Python min() keeps the first on ties
  if (b.mx > a.mx) a.mx = b.mx;  // gk:152
  flush_general(a, threshold(h, a.n), conv.data(), conv.size(), sc.key, sc.inc, sc.out);  // gk:154
}

}  // namespace

extern "C" {

int gk_version(void) { return 100; }

const char* gk_last_error(void) { return g_err.c_str(); }

int gk_create(int64_t num_streams, double eps, int64_t cap_hint, int device, gk_set** out) {
  (void)cap_hint;
  (void)device;
  if (!out) return fail(GK_E_ARG, "out is null");
  *out = nullptr;
  if (num_streams < 0 || num_streams > INT32_MAX) return fail(GK_E_ARG, "num_streams out of range");
  // any finite eps > 0, as the reference (gk:21); eps > 1 gives P = 1 (gk:60)
  if (!std::isfinite(eps) || !(eps > 0.0)) return fail(GK_E_ARG, "eps must be finite and > 0");
  const double inv = 1.0 / eps;
  if (inv >= 9.0e18) return fail(GK_E_UNSUPPORTED, "eps=%g: flush period beyond int64", eps);
  gk_set* h = new (std::nothrow) gk_set();
  if (!h) return fail(GK_E_NOMEM, "set allocation failed");
  h->S = num_streams;
  h->eps = eps;
  h->P = (int64_t)inv + 1;  // gk:60
  h->threads = default_threads();
  try {
    h->st.resize((size_t)num_streams);
  } catch (...) {
    delete h;
    return fail(GK_E_NOMEM, "state for %lld streams failed", (long long)num_streams);
  }
  *out = h;
  return GK_OK;
}

int gk_destroy(gk_set* h) {
  if (h && h->fold_scratch) gk_destroy(h->fold_scratch);
  delete h;
  return GK_OK;
}

int gk_cpu_set_threads(gk_set* h, int threads) {
  int rc = check_set(h);
  if (rc) return rc;
  if (threads < 0) return fail(GK_E_ARG, "threads must be >= 0");
  h->threads = threads ? threads : default_threads();
  return GK_OK;
}

int gk_cpu_threads(const gk_set* h) { return h ? h->threads : -1; }

int gk_reset(gk_set* h, void* stream) {
  (void)stream;
  int rc = check_set(h);
  if (rc) return rc;
  parallel_for(h->S, h->threads, [&](int64_t s) { h->st[s] = Stream(); });
  return GK_OK;
}

int gk_ingest(gk_set* h, const double* values, const int64_t* offsets, void* stream) {
  (void)stream;
  int rc = check_set(h);
  if (rc) return rc;
  return ingest_impl(h, values, offsets, nullptr, 0, nullptr, GK_Q_LIST);
}

// Stable group-by of (id, value) samples by a counting sort: histogram, scan,
// in-order scatter.  A bad id (>= S) leaves out_offsets all zero.
static int group_impl(const gk_set* h, const int32_t* ids, const double* values, int64_t count, double* out_values,
                      int64_t* out_offsets) {
  int rc = check_count(count);
  if (rc) return rc;
  if (!out_offsets) return fail(GK_E_ARG, "out_offsets is null");
  if (count > 0 && (!ids || !values || !out_values)) return fail(GK_E_ARG, "ids, values or out_values is null");
  const int64_t S = h->S;
  std::fill(out_offsets, out_offsets + S + 1, (int64_t)0);
  for (int64_t i = 0; i < count; ++i) {
    const int64_t id = ids[i];
    if (id < 0) continue;  // "not for this set"
    if (id >= S) {
      std::fill(out_offsets, out_offsets + S + 1, (int64_t)0);
      return fail(GK_E_ARG, "sample %lld has stream id %lld outside [0, %lld)", (long long)i, (long long)id,
                  (long long)S);
    }
    ++out_offsets[id + 1];
  }
  for (int64_t s = 0; s < S; ++s) out_offsets[s + 1] += out_offsets[s];
  // out_offsets[s] is the next free position of stream s while scattering,
  // and ends as the start of stream s + 1: shifted back afterwards
  for (int64_t i = 0; i < count; ++i)
    if (ids[i] >= 0) out_values[out_offsets[ids[i]]++] = values[i];
  for (int64_t s = S; s > 0; --s) out_offsets[s] = out_offsets[s - 1];
  out_offsets[0] = 0;
  return GK_OK;
}

int gk_group_by_key(gk_set* h, const int32_t* ids, const double* values, int64_t count, double* out_values,
                    int64_t* out_offsets, void* stream) {
  (void)stream;
  int rc = check_set(h);
  if (rc) return rc;
  return group_impl(h, ids, values, count, out_values, out_offsets);
}

int gk_ingest_keyed(gk_set* h, const int32_t* ids, const double* values, int64_t count, const double* qs, int nq,
                    double* out, int mode, void* stream) {
  int rc = check_set(h);
  if (!rc) rc = check_query_args(qs, nq, out, mode);
  if (!rc) rc = check_count(count);
  if (rc) return rc;
  if (h->S == 0) return GK_OK;
  try {
    if ((int64_t)h->key_vals.size() < std::max<int64_t>(count, 1)) h->key_vals.resize((size_t)std::max<int64_t>(count, 1));
    h->key_offs.resize((size_t)h->S + 1);
  } catch (...) {
    return fail(GK_E_NOMEM, "grouped batch of %lld samples failed", (long long)count);
  }
  // a bad id is returned here: nothing has been mutated
  rc = group_impl(h, ids, values, count, h->key_vals.data(), h->key_offs.data());
  if (rc) return rc;
  if (nq == 0) return gk_ingest(h, h->key_vals.data(), h->key_offs.data(), stream);
  return gk_ingest_quantiles(h, h->key_vals.data(), h->key_offs.data(), qs, nq, out, mode, stream);
}

int gk_flush(gk_set* h, void* stream) {
  (void)stream;
  int rc = check_set(h);
  if (rc) return rc;
  parallel_for(h->S, h->threads, [&](int64_t s) { flush_if_pending(h, h->st[s]); });
  return GK_OK;
}

int gk_sync(gk_set* h, void* stream) {
  (void)stream;
  return check_set(h);
}

int gk_quantiles(gk_set* h, const double* qs, int nq, double* out, int mode, void* stream) {
  (void)stream;
  int rc = check_set(h);
  if (!rc) rc = check_query_args(qs, nq, out, mode);
  if (rc) return rc;
  if (nq == 0) return GK_OK;
  mode = effective_mode(qs, nq, mode);
  parallel_for(h->S, h->threads, [&](int64_t s) {
    Stream& st = h->st[s];
    if (st.n > 0) flush_if_pending(h, st);
    answer(h, st, qs, nq, mode, out + s * (int64_t)nq);
  });
  return GK_OK;
}

int gk_ingest_quantiles(gk_set* h, const double* values, const int64_t* offsets, const double* qs, int nq,
                        double* out, int mode, void* stream) {
  (void)stream;
  int rc = check_set(h);
  if (!rc) rc = check_query_args(qs, nq, out, mode);
  if (rc) return rc;
  if (nq == 0) return ingest_impl(h, values, offsets, nullptr, 0, nullptr, mode);
  return ingest_impl(h, values, offsets, qs, nq, out, effective_mode(qs, nq, mode));
}

int gk_stats(gk_set* h, int64_t* n, double* mn, double* mx, double* sum, double* avg, int32_t* table_size,
             int32_t* pending, void* stream) {
  (void)stream;
  int rc = check_set(h);
  if (rc) return rc;
  for (int64_t s = 0; s < h->S; ++s) {
    const Stream& st = h->st[s];
    if (n) n[s] = st.n;
    if (mn) mn[s] = st.mn;
    if (mx) mx[s] = st.mx;
    if (sum) sum[s] = st.sum;
    if (avg) avg[s] = st.avg;
    if (table_size) table_size[s] = (int32_t)st.tab.size();
    if (pending) pending[s] = (int32_t)st.pend.size();
  }
  return GK_OK;
}

// ---- per-stream selection: query, flush, reset and stats of a list of streams

// count and ids checked (every id in [0, S)) before anything is mutated
static int check_select(const gk_set* h, const int32_t* ids, int64_t count) {
  int rc = check_select_args(ids, count);
  if (rc) return rc;
  for (int64_t k = 0; k < count; ++k)
    if (ids[k] < 0 || ids[k] >= h->S)
      return fail(GK_E_ARG, "ids[%lld] = %d lies outside [0, %lld)", (long long)k, ids[k], (long long)h->S);
  return GK_OK;
}

// the DISTINCT listed streams (two threads never work on one Stream)
static int distinct_ids(const gk_set* h, const int32_t* ids, int64_t count, std::vector<int32_t>& out) {
  try {
    std::vector<bool> seen((size_t)h->S, false);
    out.clear();
    for (int64_t k = 0; k < count; ++k) {
      if (seen[(size_t)ids[k]]) continue;
      seen[(size_t)ids[k]] = true;
      out.push_back(ids[k]);
    }
  } catch (...) {
    return fail(GK_E_NOMEM, "selection scratch for %lld streams failed", (long long)h->S);
  }
  return GK_OK;
}

// merge_compress() of the listed streams with n > 0 and pending values
// (gk:45-46, 166-167, 197-198), each once
static int flush_selected(gk_set* h, const int32_t* ids, int64_t count) {
  std::vector<int32_t> uniq;
  int rc = distinct_ids(h, ids, count, uniq);
  if (rc) return rc;
  parallel_for((int64_t)uniq.size(), h->threads, [&](int64_t k) {
    Stream& st = h->st[uniq[k]];
    if (st.n > 0) flush_if_pending(h, st);
  });
  return GK_OK;
}

int gk_flush_select(gk_set* h, const int32_t* ids, int64_t count, void* stream) {
  (void)stream;
  int rc = check_set(h);
  if (!rc) rc = check_select(h, ids, count);
  if (rc || count == 0) return rc;
  return flush_selected(h, ids, count);
}

int gk_quantiles_select(gk_set* h, const int32_t* ids, int64_t count, const double* qs, int nq, double* out, int mode,
                        void* stream) {
  (void)stream;
  int rc = check_set(h);
  if (!rc) rc = check_query_args(qs, nq, out, mode);
  if (!rc) rc = check_select(h, ids, count);
  if (rc || count == 0 || nq == 0) return rc;
  mode = effective_mode(qs, nq, mode);
  rc = flush_selected(h, ids, count);
  if (rc) return rc;
  // (read-only from here: rows of a repeated stream may be answered in parallel)
  parallel_for(count, h->threads,
               [&](int64_t k) { answer(h, h->st[ids[k]], qs, nq, mode, out + k * (int64_t)nq); });
  return GK_OK;
}

int gk_reset_select(gk_set* h, const int32_t* ids, int64_t count, void* stream) {
  (void)stream;
  int rc = check_set(h);
  if (!rc) rc = check_select(h, ids, count);
  if (rc || count == 0) return rc;
  std::vector<int32_t> uniq;
  rc = distinct_ids(h, ids, count, uniq);
  if (rc) return rc;
  parallel_for((int64_t)uniq.size(), h->threads, [&](int64_t k) { h->st[uniq[k]] = Stream(); });
  return GK_OK;
}

int gk_stats_select(gk_set* h, const int32_t* ids, int64_t count, int64_t* n, double* mn, double* mx, double* sum,
                    double* avg, int32_t* table_size, int32_t* pending, void* stream) {
  (void)stream;
  int rc = check_set(h);
  if (!rc) rc = check_select(h, ids, count);
  if (rc) return rc;
  for (int64_t k = 0; k < count; ++k) {
    const Stream& st = h->st[ids[k]];
    if (n) n[k] = st.n;
    if (mn) mn[k] = st.mn;
    if (mx) mx[k] = st.mx;
    if (sum) sum[k] = st.sum;
    if (avg) avg[k] = st.avg;
    if (table_size) table_size[k] = (int32_t)st.tab.size();
    if (pending) pending[k] = (int32_t)st.pend.size();
  }
  return GK_OK;
}

// ---- rank queries: bounds on each stream's count of values <= x (gk_capi.h)

// one row: the four rules of gk_capi.h on a flushed stream (read-only).  The
// table is ascending: the walk stops at entry i, the first with v > x, holding
// G(i) -- then G(i+1) + d_i - 1 = G(i) + g_i + d_i - 1.
static void rank_row(const Stream& st, const double* xs, int nx, int64_t* lo, int64_t* hi) {
  const int64_t E = (int64_t)st.tab.size();
  for (int t = 0; t < nx; ++t) {
    const double x = xs[t];
    int64_t l, u;
    if (st.n == 0 || x < st.mn) {
      l = u = 0;
    } else if (x >= st.mx) {
      l = u = st.n;
    } else {
      int64_t i = 0, G = 0;
      for (; i < E && st.tab[(size_t)i].v <= x; ++i) G += st.tab[(size_t)i].g;
      l = std::max<int64_t>(G, 1);
      u = std::min<int64_t>(i < E ? G + st.tab[(size_t)i].g + st.tab[(size_t)i].d - 1 : st.n, st.n - 1);
    }
    if (lo) lo[t] = l;
    if (hi) hi[t] = u;
  }
}

int gk_ranks(gk_set* h, const double* xs, int nx, int64_t* lo, int64_t* hi, void* stream) {
  (void)stream;
  int rc = check_set(h);
  if (!rc) rc = check_rank_args(xs, nx, lo, hi);
  if (rc || nx == 0) return rc;
  parallel_for(h->S, h->threads, [&](int64_t s) {
    Stream& st = h->st[s];
    if (st.n > 0) flush_if_pending(h, st);  // gk:166-167
    rank_row(st, xs, nx, lo ? lo + s * (int64_t)nx : nullptr, hi ? hi + s * (int64_t)nx : nullptr);
  });
  return GK_OK;
}

int gk_ranks_select(gk_set* h, const int32_t* ids, int64_t count, const double* xs, int nx, int64_t* lo, int64_t* hi,
                    void* stream) {
  (void)stream;
  int rc = check_set(h);
  if (!rc) rc = check_rank_args(xs, nx, lo, hi);
  if (!rc) rc = check_select(h, ids, count);
  if (rc || count == 0 || nx == 0) return rc;
  rc = flush_selected(h, ids, count);
  if (rc) return rc;
  // (read-only from here: rows of a repeated stream may be answered in parallel)
  parallel_for(count, h->threads, [&](int64_t k) {
    rank_row(h->st[ids[k]], xs, nx, lo ? lo + k * (int64_t)nx : nullptr, hi ? hi + k * (int64_t)nx : nullptr);
  });
  return GK_OK;
}

// rank bounds per (stream id, value) sample: the checks in sample order, the
// flush over the distinct occurring streams, then every row read-only
int gk_ranks_keyed(gk_set* h, const int32_t* ids, const double* xs, int64_t count, int64_t* lo, int64_t* hi, int64_t* n,
                   void* stream) {
  (void)stream;
  int rc = check_set(h);
  if (!rc) rc = check_rank_keyed_args(ids, xs, count, lo, hi, n);
  if (rc || count == 0) return rc;
  for (int64_t k = 0; k < count; ++k)
    if (ids[k] >= h->S || (ids[k] >= 0 && std::isnan(xs[k]))) return fail_rank_keyed_sample(k, ids[k], h->S);
  std::vector<int32_t> uniq;
  try {
    std::vector<bool> seen((size_t)h->S, false);
    for (int64_t k = 0; k < count; ++k) {
      if (ids[k] < 0 || seen[(size_t)ids[k]]) continue;  // (negative: "no stream")
      seen[(size_t)ids[k]] = true;
      uniq.push_back(ids[k]);
    }
  } catch (...) {
    return fail(GK_E_NOMEM, "selection scratch for %lld streams failed", (long long)h->S);
  }
  parallel_for((int64_t)uniq.size(), h->threads, [&](int64_t k) {
    Stream& st = h->st[uniq[k]];
    if (st.n > 0) flush_if_pending(h, st);  // gk:166-167
  });
  // (read-only from here: rows of a repeated stream may be answered in parallel)
  parallel_for(count, h->threads, [&](int64_t k) {
    int64_t l = 0, u = 0, cnt = 0;
    if (ids[k] >= 0) {
      const Stream& st = h->st[ids[k]];
      rank_row(st, xs + k, 1, &l, &u);
      cnt = st.n;
    }
    if (lo) lo[k] = l;
    if (hi) hi[k] = u;
    if (n) n[k] = cnt;
  });
  return GK_OK;
}

// gk_ranks_keyed, then gk_ingest_keyed, on ONE group-by: the samples are
// grouped by id once, with their values and their indices; each occurring
// stream is flushed and answers its run from the grouped order; the grouped
// values are then the batch the ingest takes.
int gk_rank_ingest_keyed(gk_set* h, const int32_t* ids, const double* xs, int64_t count, int64_t* lo, int64_t* hi,
                         int64_t* n, const double* qs, int nq, double* out, int mode, void* stream) {
  int rc = check_set(h);
  if (!rc) rc = check_rank_ingest_keyed_args(ids, xs, count);
  if (!rc) rc = check_query_args(qs, nq, out, mode);
  if (rc) return rc;
  for (int64_t k = 0; k < count; ++k)
    if (ids[k] >= h->S || (ids[k] >= 0 && std::isnan(xs[k]))) return fail_rank_keyed_sample(k, ids[k], h->S);
  if (count == 0) return gk_ingest_keyed(h, ids, xs, 0, qs, nq, out, mode, stream);
  if (h->S == 0) {  // (every id is negative)
    for (int64_t* o : {lo, hi, n})
      if (o) std::fill(o, o + count, (int64_t)0);
    return GK_OK;
  }
  try {
    if ((int64_t)h->key_vals.size() < count) h->key_vals.resize((size_t)count);
    if ((int64_t)h->key_idx.size() < count) h->key_idx.resize((size_t)count);
    h->key_offs.resize((size_t)h->S + 1);
  } catch (...) {
    return fail(GK_E_NOMEM, "grouped batch of %lld samples failed", (long long)count);
  }
  // group_impl's counting sort, carrying the sample index beside the value
  double* const gv = h->key_vals.data();
  int64_t* const gi = h->key_idx.data();
  int64_t* const offs = h->key_offs.data();
  const int64_t S = h->S;
  std::fill(offs, offs + S + 1, (int64_t)0);
  for (int64_t i = 0; i < count; ++i)
    if (ids[i] >= 0) ++offs[ids[i] + 1];
  for (int64_t s = 0; s < S; ++s) offs[s + 1] += offs[s];
  for (int64_t i = 0; i < count; ++i) {
    if (ids[i] < 0) continue;
    const int64_t p = offs[ids[i]]++;
    gv[p] = xs[i];
    gi[p] = i;
  }
  for (int64_t s = S; s > 0; --s) offs[s] = offs[s - 1];
  offs[0] = 0;
  // every sample is ranked before any value of the batch is added
  parallel_for(S, h->threads, [&](int64_t s) {
    if (offs[s] == offs[s + 1]) return;
    if (!lo && !hi && !n) return;  // (no rank output: gk_ingest_keyed, no flush)
    Stream& st = h->st[s];
    if (st.n > 0) flush_if_pending(h, st);  // gk:166-167
    for (int64_t p = offs[s]; p < offs[s + 1]; ++p) {
      int64_t l = 0, u = 0;
      rank_row(st, gv + p, 1, &l, &u);
      if (lo) lo[gi[p]] = l;
      if (hi) hi[gi[p]] = u;
      if (n) n[gi[p]] = st.n;
    }
  });
  for (int64_t k = 0; k < count; ++k) {
    if (ids[k] >= 0) continue;  // "no stream": the answer of an empty sketch
    if (lo) lo[k] = 0;
    if (hi) hi[k] = 0;
    if (n) n[k] = 0;
  }
  if (nq == 0) return gk_ingest(h, gv, offs, stream);
  return gk_ingest_quantiles(h, gv, offs, qs, nq, out, mode, stream);
}

int gk_merge(gk_set* dst, gk_set* const* srcs, int nsrcs, void* stream) {
  (void)stream;
  int rc = check_merge_args(dst, srcs, nsrcs);
  if (rc) return rc;
  // the fold runs per stream: dst.merge(srcs[0]); dst.merge(srcs[1]); ...
  // A source may be dst itself (gk:111-154 accepts other is self: the flush
  // of gk:137 empties dst's own incoming, the conversion reads the flushed
  // table into `conv` before gk:154 rewrites it, gk:149 doubles n) or repeat
  // (flushed again at each merge, as the reference does).
  parallel_for(dst->S, dst->threads, [&](int64_t s) {
    std::vector<Rec> conv;
    for (int k = 0; k < nsrcs; ++k) merge_stream(dst, dst->st[s], srcs[k]->st[s], conv);
  });
  return GK_OK;
}

int gk_rollup(gk_set* dst, gk_set* src, const int64_t* group_offsets, const int64_t* members, void* stream) {
  (void)stream;
  int rc = check_rollup_args(dst, src, group_offsets);
  if (rc) return rc;
  const int64_t G = dst->S, S = src->S;
  if (group_offsets[0] != 0) return fail(GK_E_ARG, "group_offsets must start at 0");
  for (int64_t j = 0; j < G; ++j)
    if (group_offsets[j + 1] < group_offsets[j])
      return fail(GK_E_ARG, "group_offsets decrease at group %lld", (long long)j);
  const int64_t M = group_offsets[G];
  if (M > 0 && !members) return fail(GK_E_ARG, "members is null");
  // every member in [0, S) and listed once: nothing is mutated before this holds
  std::vector<bool> seen((size_t)S, false);
  for (int64_t k = 0; k < M; ++k) {
    const int64_t m = members[k];
    if (m < 0 || m >= S)
      return fail(GK_E_ARG, "member %lld (position %lld) outside [0, %lld)", (long long)m, (long long)k, (long long)S);
    if (seen[(size_t)m]) return fail(GK_E_ARG, "source stream %lld is listed more than once", (long long)m);
    seen[(size_t)m] = true;
  }
  // per destination stream the left fold dst[j].merge(src[members[k]]) in
  // order of k (gk:111-154); an empty group leaves its destination untouched
  parallel_for(G, dst->threads, [&](int64_t j) {
    std::vector<Rec> conv;
    for (int64_t k = group_offsets[j]; k < group_offsets[j + 1]; ++k)
      merge_stream(dst, dst->st[j], src->st[members[k]], conv);
  });
  return GK_OK;
}

int gk_merge_compress(gk_set* h, const double* v, const int32_t* g, const int32_t* d, const int64_t* eoffs,
                      void* stream) {
  (void)stream;
  int rc = check_set(h);
  if (!rc) rc = check_record_args(v, g, d, eoffs);
  if (rc) return rc;
  parallel_for(h->S, h->threads, [&](int64_t s) {
    std::vector<Rec> recs;
    for (int64_t k = eoffs[s]; k < eoffs[s + 1]; ++k) recs.push_back(Rec{v[k], g[k], d[k]});
    Stream& st = h->st[s];
    flush_general(st, threshold(h, st.n), recs.data(), recs.size(), tl_scratch.key, tl_scratch.inc, tl_scratch.out);
  });
  return GK_OK;
}

int gk_export_sizes(gk_set* h, int32_t* sizes, void* stream) {
  (void)stream;
  int rc = check_set(h);
  if (rc) return rc;
  if (!sizes) return fail(GK_E_ARG, "sizes is null");
  for (int64_t s = 0; s < h->S; ++s) sizes[s] = (int32_t)h->st[s].tab.size();
  return GK_OK;
}

int gk_export(gk_set* h, const int64_t* offs, double* v, int32_t* g, int32_t* d, void* stream) {
  (void)stream;
  int rc = check_set(h);
  if (rc) return rc;
  if (!offs) return fail(GK_E_ARG, "offs is null");
  parallel_for(h->S, h->threads, [&](int64_t s) {
    const std::vector<Rec>& t = h->st[s].tab;
    const int64_t o = offs[s];
    for (size_t j = 0; j < t.size(); ++j) {
      if (v) v[o + j] = t[j].v;
      if (g) g[o + j] = (int32_t)t[j].g;
      if (d) d[o + j] = (int32_t)t[j].d;
    }
  });
  return GK_OK;
}

int gk_export_pending_sizes(gk_set* h, int32_t* sizes, void* stream) {
  (void)stream;
  int rc = check_set(h);
  if (rc) return rc;
  if (!sizes) return fail(GK_E_ARG, "sizes is null");
  for (int64_t s = 0; s < h->S; ++s) sizes[s] = (int32_t)h->st[s].pend.size();
  return GK_OK;
}

int gk_export_pending(gk_set* h, const int64_t* poffs, double* pv, void* stream) {
  (void)stream;
  int rc = check_set(h);
  if (rc) return rc;
  if (!poffs || !pv) return fail(GK_E_ARG, "null pointer");
  for (int64_t s = 0; s < h->S; ++s) std::copy(h->st[s].pend.begin(), h->st[s].pend.end(), pv + poffs[s]);
  return GK_OK;
}

int gk_import(gk_set* h, const int64_t* offs, const double* v, const int32_t* g, const int32_t* d,
              const int64_t* poffs, const double* pv, const int64_t* n, const double* mn, const double* mx,
              const double* sum, const double* avg, void* stream) {
  (void)stream;
  int rc = check_set(h);
  if (rc) return rc;
  if (!offs || !poffs || !n || !mn || !mx || !sum || !avg) return fail(GK_E_ARG, "null pointer");
  for (int64_t s = 0; s < h->S; ++s)
    if (offs[s + 1] < offs[s] || poffs[s + 1] < poffs[s] || n[s] < 0 || poffs[s + 1] - poffs[s] > n[s] % h->P)
      return fail(GK_E_ARG, "stream %lld: bad table / pending sizes (pending <= n %% %d)", (long long)s, h->P);
  parallel_for(h->S, h->threads, [&](int64_t s) {
    Stream& st = h->st[s];
    st.n = n[s];
    st.mn = mn[s];
    st.mx = mx[s];
    st.sum = sum[s];
    st.avg = avg[s];
    st.tab.clear();
    for (int64_t k = offs[s]; k < offs[s + 1]; ++k) st.tab.push_back(Rec{v[k], g[k], d[k]});
    st.pend.assign(pv + poffs[s], pv + poffs[s + 1]);
  });
  return GK_OK;
}

// ---- versioned state files (gk_format.h) ------------------------------------
static int fmt_error(int rc, const char* path) {
  switch (rc) {
    case gkfmt::E_IO: return fail(GK_E_IO, "cannot read/write state file %s", path);
    case gkfmt::E_VERSION: return fail(GK_E_FORMAT, "%s: unsupported state format version", path);
    case gkfmt::E_CHECKSUM: return fail(GK_E_FORMAT, "%s: checksum mismatch (corrupt state file)", path);
    default: return fail(GK_E_FORMAT, "%s: not a GKSTATE file or truncated", path);
  }
}

int gk_save(gk_set* h, const char* path, void* stream) {
  (void)stream;
  int rc = check_set(h);
  if (rc) return rc;
  if (!path) return fail(GK_E_ARG, "path is null");
  gkfmt::State f;
  f.eps = h->eps;
  f.resize_streams(h->S);
  for (int64_t s = 0; s < h->S; ++s) {
    const Stream& st = h->st[s];
    f.sizes[s] = (int32_t)st.tab.size();
    f.psizes[s] = (int32_t)st.pend.size();
    f.n[s] = st.n;
    f.mn[s] = st.mn;
    f.mx[s] = st.mx;
    f.sum[s] = st.sum;
    f.avg[s] = st.avg;
    for (const Rec& r : st.tab) {
      f.v.push_back(r.v);
      f.g.push_back((int32_t)r.g);
      f.d.push_back((int32_t)r.d);
    }
    f.pv.insert(f.pv.end(), st.pend.begin(), st.pend.end());
  }
  rc = gkfmt::write(path, f);
  return rc ? fmt_error(rc, path) : GK_OK;
}

int gk_peek(const char* path, double* eps, int64_t* num_streams) {
  if (!path) return fail(GK_E_ARG, "path is null");
  gkfmt::Header hd;
  const int rc = gkfmt::peek(path, &hd);
  if (rc) return fmt_error(rc, path);
  if (eps) *eps = hd.eps;
  if (num_streams) *num_streams = hd.S;
  return GK_OK;
}

int gk_load(gk_set* h, const char* path, void* stream) {
  int rc = check_set(h);
  if (rc) return rc;
  if (!path) return fail(GK_E_ARG, "path is null");
  gkfmt::State f;
  rc = gkfmt::read(path, &f);
  if (rc) return fmt_error(rc, path);
  if (f.S != h->S)
    return fail(GK_E_ARG, "%s holds %lld streams, the set has %lld", path, (long long)f.S, (long long)h->S);
  if (f.eps != h->eps)
    return fail(GK_E_EPS_MISMATCH, "%s was saved with eps=%.17g, the set has eps=%.17g", path, f.eps, h->eps);
  std::vector<int64_t> offs(f.S + 1, 0), poffs(f.S + 1, 0);
  for (int64_t s = 0; s < f.S; ++s) {
    offs[s + 1] = offs[s] + f.sizes[s];
    poffs[s + 1] = poffs[s] + f.psizes[s];
  }
  return gk_import(h, offs.data(), f.v.data(), f.g.data(), f.d.data(), poffs.data(), f.pv.data(), f.n.data(),
                   f.mn.data(), f.mx.data(), f.sum.data(), f.avg.data(), stream);
}

int64_t gk_num_streams(const gk_set* h) { return h ? h->S : -1; }
double gk_eps(const gk_set* h) { return h ? h->eps : 0.0; }
// ---- packed state (gk_pack.h): host buffers --------------------------------
namespace {
struct HostMem {
  static int to_host(void* host, const void* src, size_t n, void*) {
    memcpy(host, src, n);
    return GK_OK;
  }
  static int from_host(void* dst, const void* host, size_t n, void*) {
    memcpy(dst, host, n);
    return GK_OK;
  }
};
}  // namespace

int gk_pack_bytes(gk_set* h, int64_t* bytes, void* stream) {
  int rc = check_set(h);
  if (rc) return rc;
  if (!bytes) return fail(GK_E_ARG, "bytes is null");
  std::vector<int32_t> e(std::max<int64_t>(h->S, 1)), p(std::max<int64_t>(h->S, 1));
  return gkpack::pack_bytes<HostMem>(h, e.data(), p.data(), bytes, stream);
}

int gk_pack(gk_set* h, void* buf, int64_t bytes, void* stream) {
  int rc = check_set(h);
  if (rc) return rc;
  if (!buf) return fail(GK_E_ARG, "buf is null");
  std::vector<int32_t> e(std::max<int64_t>(h->S, 1)), p(std::max<int64_t>(h->S, 1));
  std::string err;
  rc = gkpack::pack<HostMem>(h, e.data(), p.data(), buf, bytes, stream, err);
  return (rc && !err.empty()) ? fail(rc, "%s", err.c_str()) : rc;
}

int gk_fold_packed(gk_set* dst, const void* const* bufs, int nbufs, void* stream) {
  int rc = check_set(dst);
  if (rc) return rc;
  std::string err;
  auto make = [&](gk_set** out) {
    const int r = gk_create(dst->S, dst->eps, 0, 0, out);
    if (!r) (*out)->threads = dst->threads;
    return r;
  };
  rc = gkpack::fold<HostMem>(dst, bufs, nbufs, &dst->fold_scratch, make, stream, err);
  return (rc && !err.empty()) ? fail(rc, "%s", err.c_str()) : rc;
}

// ---- stream transfer: listed streams to and from a packed state (gk_capi.h) --
static gkpack::Layout select_layout(const gk_set* h, const int32_t* ids, int64_t count) {
  int64_t E = 0, P = 0;
  for (int64_t k = 0; k < count; ++k) {
    E += (int64_t)h->st[ids[k]].tab.size();
    P += (int64_t)h->st[ids[k]].pend.size();
  }
  return gkpack::layout(count, E, P);
}

int gk_pack_select_bytes(gk_set* h, const int32_t* ids, int64_t count, int64_t* bytes, void* stream) {
  (void)stream;
  if (!bytes) return fail(GK_E_ARG, "bytes is null");
  int rc = check_set(h);
  if (!rc) rc = check_select(h, ids, count);
  if (rc) return rc;
  *bytes = (int64_t)select_layout(h, ids, count).total;
  return GK_OK;
}

int gk_pack_select(gk_set* h, const int32_t* ids, int64_t count, void* buf, int64_t bytes, void* stream) {
  (void)stream;
  if (!buf) return fail(GK_E_ARG, "buf is null");
  int rc = check_set(h);
  if (!rc) rc = check_select(h, ids, count);
  if (rc) return rc;
  const gkpack::Layout L = select_layout(h, ids, count);
  if (bytes < (int64_t)L.total)
    return fail(GK_E_ARG, "packed state needs %lld bytes, the buffer has %lld", (long long)L.total, (long long)bytes);
  gkpack::Header hd{};
  hd.magic = gkpack::kMagic;
  hd.version = gkpack::kVersion;
  hd.header_bytes = sizeof(gkpack::Header);
  hd.eps = h->eps;
  hd.S = count;
  hd.E = L.E;
  hd.P = L.P;
  hd.bytes = (int64_t)L.total;
  memcpy(buf, &hd, sizeof(hd));
  int64_t* const eo = gkpack::at<int64_t>(buf, L.eoffs);
  int64_t* const po = gkpack::at<int64_t>(buf, L.poffs);
  eo[0] = po[0] = 0;
  for (int64_t k = 0; k < count; ++k) {
    eo[k + 1] = eo[k] + (int64_t)h->st[ids[k]].tab.size();
    po[k + 1] = po[k] + (int64_t)h->st[ids[k]].pend.size();
  }
  int64_t* const n = gkpack::at<int64_t>(buf, L.n);
  double* const mn = gkpack::at<double>(buf, L.mn);
  double* const mx = gkpack::at<double>(buf, L.mx);
  double* const sum = gkpack::at<double>(buf, L.sum);
  double* const avg = gkpack::at<double>(buf, L.avg);
  double* const v = gkpack::at<double>(buf, L.v);
  int32_t* const g = gkpack::at<int32_t>(buf, L.g);
  int32_t* const d = gkpack::at<int32_t>(buf, L.d);
  double* const pv = gkpack::at<double>(buf, L.pv);
  // (read-only: rows of a repeated stream may be written in parallel)
  parallel_for(count, h->threads, [&](int64_t k) {
    const Stream& st = h->st[ids[k]];
    n[k] = st.n;
    mn[k] = st.mn;
    mx[k] = st.mx;
    sum[k] = st.sum;
    avg[k] = st.avg;
    for (size_t j = 0; j < st.tab.size(); ++j) {
      v[eo[k] + (int64_t)j] = st.tab[j].v;
      g[eo[k] + (int64_t)j] = (int32_t)st.tab[j].g;
      d[eo[k] + (int64_t)j] = (int32_t)st.tab[j].d;
    }
    std::copy(st.pend.begin(), st.pend.end(), pv + po[k]);
  });
  return GK_OK;
}

int gk_unpack_select(gk_set* h, const int32_t* ids, int64_t count, const void* buf, void* stream) {
  int rc = check_set(h);
  if (!rc) rc = check_select_args(ids, count);
  if (rc) return rc;
  if (!buf) return fail(GK_E_ARG, "buf is null");
  gkpack::Header hd{};
  std::string err;
  rc = gkpack::read_header<HostMem>(h, buf, &hd, stream, err, count);
  if (rc) return err.empty() ? rc : fail(rc, "%s", err.c_str());
  rc = check_select(h, ids, count);
  if (rc) return rc;
  std::vector<int32_t> uniq;
  rc = distinct_ids(h, ids, count, uniq);
  if (rc) return rc;
  if ((int64_t)uniq.size() != count)
    return fail(GK_E_ARG, "a stream id is listed more than once (two rows for one stream)");
  const gkpack::Layout L = gkpack::layout(hd.S, hd.E, hd.P);
  const int64_t* const eo = gkpack::at<int64_t>(buf, L.eoffs);
  const int64_t* const po = gkpack::at<int64_t>(buf, L.poffs);
  const int64_t* const n = gkpack::at<int64_t>(buf, L.n);
  for (int64_t k = 0; k < count; ++k)
    if (n[k] < 0 || po[k + 1] - po[k] > n[k] % h->P)
      return fail(GK_E_ARG, "a packed stream holds more pending values than add() leaves (pending <= n %% %lld)",
                  (long long)h->P);
  const double* const mn = gkpack::at<double>(buf, L.mn);
  const double* const mx = gkpack::at<double>(buf, L.mx);
  const double* const sum = gkpack::at<double>(buf, L.sum);
  const double* const avg = gkpack::at<double>(buf, L.avg);
  const double* const v = gkpack::at<double>(buf, L.v);
  const int32_t* const g = gkpack::at<int32_t>(buf, L.g);
  const int32_t* const d = gkpack::at<int32_t>(buf, L.d);
  const double* const pv = gkpack::at<double>(buf, L.pv);
  // the new states are built beside the set and moved in whole: a stream
  // never holds header words of one state and the table of the other
  std::vector<Stream> fresh;
  try {
    fresh.resize((size_t)count);
    parallel_for(count, h->threads, [&](int64_t k) {
      Stream& st = fresh[(size_t)k];
      st.n = n[k];
      st.mn = mn[k];
      st.mx = mx[k];
      st.sum = sum[k];
      st.avg = avg[k];
      st.tab.reserve((size_t)(eo[k + 1] - eo[k]));
      for (int64_t j = eo[k]; j < eo[k + 1]; ++j) st.tab.push_back(Rec{v[j], g[j], d[j]});
      st.pend.assign(pv + po[k], pv + po[k + 1]);
    });
  } catch (...) {
    return fail(GK_E_NOMEM, "unpack of %lld stream(s) failed", (long long)count);
  }
  for (int64_t k = 0; k < count; ++k) h->st[ids[k]] = std::move(fresh[(size_t)k]);
  return GK_OK;
}

// ---- compaction: one unbounded class, so only unused vector capacity goes back
static int64_t capacity_bytes(const gk_set* h) {
  int64_t b = 0;
  for (const Stream& st : h->st)
    b += (int64_t)(st.tab.capacity() * sizeof(Rec)) + (int64_t)(st.pend.capacity() * sizeof(double));
  return b;
}

int gk_compact(gk_set* h, int64_t* demoted, int64_t* bytes_freed, void* stream) {
  (void)stream;
  int rc = check_set(h);
  if (rc) return rc;
  const int64_t before = capacity_bytes(h);
  // (a shrink that finds no memory for the smaller copy keeps the vector as it is)
  parallel_for(h->S, h->threads, [&](int64_t s) {
    Stream& st = h->st[(size_t)s];
    try {
      st.tab.shrink_to_fit();
      st.pend.shrink_to_fit();
    } catch (...) {
    }
  });
  if (demoted) *demoted = 0;
  if (bytes_freed) *bytes_freed = before - capacity_bytes(h);
  return GK_OK;
}

int gk_class_usage(gk_set* h, int cls, int64_t* streams, int64_t* slots_used, int64_t* slots_alloc,
                   int64_t* arena_bytes, int64_t* workspace_bytes, void* stream) {
  (void)stream;
  int rc = check_set(h);
  if (rc) return rc;
  if (cls != 0) return fail(GK_E_ARG, "class %d outside [0, 1)", cls);
  if (streams) *streams = h->S;
  if (slots_used) *slots_used = h->S;
  if (slots_alloc) *slots_alloc = h->S;
  if (arena_bytes) *arena_bytes = capacity_bytes(h);
  if (workspace_bytes) *workspace_bytes = 0;
  return GK_OK;
}

// ---- key directory: the loop of gk_capi.h over an open-addressing table -------
}  // extern "C"

namespace {
// linear probing over T slots (gk_dirhash.h: geometry, hash and the
// GK_DIR_HASH_BITS switch are the device engine's).  A removed key stays in
// its slot with id -1, its own tombstone: probes walk over it, and the key
// finds the slot again when it comes back.
struct DirTable {
  std::vector<int64_t> keys;  // GK_DIR_NONE = empty
  std::vector<int32_t> ids;   // -1: empty slot, or a removed key's
  std::vector<int64_t> key_of_id;  // [0, bound): GK_DIR_NONE at free ids
  std::set<int32_t> free;          // the ids below bound that no key holds
  int64_t dead = 0;                // upper bound on slots that hold a removed key
  uint32_t T = 0;
  GKDirHome home = {};

  void clear(int64_t slots) {
    T = (uint32_t)slots;
    keys.assign((size_t)slots, GK_DIR_NONE);
    ids.assign((size_t)slots, -1);
    key_of_id.clear();
    free.clear();
    dead = 0;
  }
  int64_t bound() const { return (int64_t)key_of_id.size(); }
  int64_t size() const { return bound() - (int64_t)free.size(); }
  // the slot of k, or the empty slot where its probe ends (T full slots: -1)
  int64_t find(int64_t k) const {
    uint32_t slot = gk_dir_home(home, gk_dir_mix((uint64_t)k));
    for (uint32_t it = 0; it < T; ++it) {
      if (keys[slot] == k || keys[slot] == GK_DIR_NONE) return slot;
      slot = (slot + 1) & (T - 1);
    }
    return -1;
  }
  bool holds(int64_t slot, int64_t k) const {
    return slot >= 0 && keys[(size_t)slot] == k && ids[(size_t)slot] >= 0;
  }
  // d[k] = id for a key the table does not hold (slot: find's answer; id: a hole of key_of_id or its end)
  void bind(int64_t slot, int64_t k, int32_t id) {
    keys[(size_t)slot] = k;
    ids[(size_t)slot] = id;
    if ((int64_t)id == bound())
      key_of_id.push_back(k);
    else
      key_of_id[(size_t)id] = k;
  }
  // every slot again from key_of_id (free ids skipped): no tombstones, no slots of a void call
  void rebuild() {
    keys.assign((size_t)T, GK_DIR_NONE);
    ids.assign((size_t)T, -1);
    for (int64_t id = 0; id < bound(); ++id) {
      const int64_t k = key_of_id[(size_t)id];
      if (k == GK_DIR_NONE) continue;
      const int64_t slot = find(k);
      keys[(size_t)slot] = k;
      ids[(size_t)slot] = (int32_t)id;
    }
    dead = 0;
  }
};
}  // namespace

struct gk_dir {
  int64_t capacity = 0;
  DirTable t;
};

namespace {
// gk_dir_import (sparse false: a GK_DIR_NONE entry is refused) and gk_dir_import_sparse
int dir_import(gk_dir* d, const int64_t* keys, int64_t count, bool sparse) {
  if (count > d->capacity) return fail_dir_import_count(count, d->capacity);
  if (!sparse)
    for (int64_t i = 0; i < count; ++i)
      if (keys[i] == GK_DIR_NONE) return fail_dir_import_none(i);
  // built in a second table that replaces the first on success
  DirTable nt;
  nt.home = d->t.home;
  try {
    nt.clear(d->t.T);
    nt.key_of_id.reserve((size_t)count);
  } catch (...) {
    return fail(GK_E_NOMEM, "directory: no memory for a second table");
  }
  for (int64_t i = 0; i < count; ++i) {
    if (keys[i] == GK_DIR_NONE) {
      nt.key_of_id.push_back(GK_DIR_NONE);
      nt.free.insert((int32_t)i);
      continue;
    }
    const int64_t slot = nt.find(keys[i]);
    if (nt.keys[(size_t)slot] == keys[i]) return fail_dir_import_repeat(i, keys[i]);
    nt.bind(slot, keys[i], (int32_t)i);
  }
  d->t = std::move(nt);
  return GK_OK;
}
}  // namespace

extern "C" {

int gk_dir_create(int64_t capacity, int device, gk_dir** out) {
  (void)device;
  int rc = check_dir_create(capacity, out);
  if (rc) return rc;
  GKDirHome home;
  const int64_t T = gk_dir_slots(capacity);
  if (!gk_dir_home_from_env(T, &home))
    return fail(GK_E_ARG, "GK_DIR_HASH_BITS=%s: a number >= 0", getenv("GK_DIR_HASH_BITS"));
  try {
    gk_dir* d = new gk_dir();
    d->capacity = capacity;
    d->t.home = home;
    d->t.clear(T);
    *out = d;
  } catch (...) {
    return fail(GK_E_NOMEM, "directory: no memory for a table of %lld slots", (long long)T);
  }
  return GK_OK;
}

int gk_dir_destroy(gk_dir* d) {
  delete d;
  return GK_OK;
}

int64_t gk_dir_capacity(const gk_dir* d) { return d ? d->capacity : -1; }
int64_t gk_dir_size(const gk_dir* d) { return d ? d->t.size() : -1; }
int64_t gk_dir_bound(const gk_dir* d) { return d ? d->t.bound() : -1; }

int gk_dir_assign(gk_dir* d, const int64_t* keys, int64_t count, int32_t* out_ids, int64_t* num_new, void* stream) {
  (void)stream;
  int rc = check_dir_args(d, keys, count, out_ids, true);
  if (rc) return rc;
  DirTable& t = d->t;
  const int64_t bound0 = t.bound(), size0 = t.size();
  std::vector<int32_t> fresh;  // the ids this call has handed out, to take back if it turns out void
  for (int64_t i = 0; i < count; ++i) {
    const int64_t k = keys[i];
    if (k == GK_DIR_NONE) {
      out_ids[i] = -1;
      continue;
    }
    const int64_t slot = t.find(k);
    if (t.holds(slot, k)) {
      out_ids[i] = t.ids[(size_t)slot];
      continue;
    }
    int32_t id;
    if (!t.free.empty()) {
      id = *t.free.begin();
      t.free.erase(t.free.begin());
    } else if (t.bound() < d->capacity) {
      id = (int32_t)t.bound();
    } else {
      // void call: the ids go back (holes stay holes) and the table is rebuilt from the ids it held before
      for (int32_t f : fresh) {
        if ((int64_t)f >= bound0) continue;
        t.key_of_id[(size_t)f] = GK_DIR_NONE;
        t.free.insert(f);
      }
      t.key_of_id.resize((size_t)bound0);
      t.rebuild();
      return fail_dir_overflow(d->capacity, size0);
    }
    // (size < capacity <= T / 2 and at most T / 4 removed keys in place: find met the key's or an empty slot)
    t.bind(slot, k, id);
    fresh.push_back(id);
    out_ids[i] = id;
  }
  if (num_new) *num_new = (int64_t)fresh.size();
  return GK_OK;
}

int gk_dir_remove(gk_dir* d, const int64_t* keys, int64_t count, int32_t* out_ids, int64_t* num_removed,
                  void* stream) {
  (void)stream;
  int rc = check_dir_args(d, keys, count, out_ids, true);
  if (rc) return rc;
  DirTable& t = d->t;
  int64_t removed = 0;
  for (int64_t i = 0; i < count; ++i) {
    const int64_t k = keys[i];
    const int64_t slot = k == GK_DIR_NONE ? -1 : t.find(k);
    if (!t.holds(slot, k)) {
      out_ids[i] = -1;
      continue;
    }
    const int32_t id = t.ids[(size_t)slot];
    out_ids[i] = id;
    t.ids[(size_t)slot] = -1;  // the key stays: its own tombstone
    t.key_of_id[(size_t)id] = GK_DIR_NONE;
    t.free.insert(id);
    ++removed;
  }
  // as the device engine: at most T/4 removed keys keep a slot, so used slots stay <= 3T/4
  t.dead += removed;
  if (t.dead > (int64_t)t.T / 4) t.rebuild();
  if (num_removed) *num_removed = removed;
  return GK_OK;
}

int gk_dir_lookup(gk_dir* d, const int64_t* keys, int64_t count, int32_t* out_ids, void* stream) {
  (void)stream;
  int rc = check_dir_args(d, keys, count, out_ids, true);
  if (rc) return rc;
  const DirTable& t = d->t;
  for (int64_t i = 0; i < count; ++i) {
    const int64_t k = keys[i];
    const int64_t slot = k == GK_DIR_NONE ? -1 : t.find(k);
    out_ids[i] = t.holds(slot, k) ? t.ids[(size_t)slot] : -1;
  }
  return GK_OK;
}

int gk_dir_keys(gk_dir* d, int64_t* out_keys, void* stream) {
  (void)stream;
  int rc = check_dir(d);
  if (rc) return rc;
  if (d->t.key_of_id.empty()) return GK_OK;
  if (!out_keys) return fail(GK_E_ARG, "out_keys is null");
  std::copy(d->t.key_of_id.begin(), d->t.key_of_id.end(), out_keys);
  return GK_OK;
}

int gk_dir_import(gk_dir* d, const int64_t* keys, int64_t count, void* stream) {
  (void)stream;
  int rc = check_dir_args(d, keys, count, nullptr, false);
  if (rc) return rc;
  return dir_import(d, keys, count, false);
}

int gk_dir_import_sparse(gk_dir* d, const int64_t* keys, int64_t count, void* stream) {
  (void)stream;
  int rc = check_dir_args(d, keys, count, nullptr, false);
  if (rc) return rc;
  return dir_import(d, keys, count, true);
}

int gk_flush_period(const gk_set* h) { return h ? (int)std::min<int64_t>(h->P, INT32_MAX) : -1; }
int gk_capacity(const gk_set* h, int cls) { return (h && cls == 0) ? INT32_MAX : -1; }  // unbounded, one class
int64_t gk_num_promoted(const gk_set* h) { return h ? 0 : -1; }

int gk_timing_enable(gk_set* h, int on) {
  int rc = check_set(h);
  if (rc) return rc;
  h->timing = on != 0;
  return GK_OK;
}

int gk_timing_read(gk_set* h, double* flush_ms, double* stats_ms, int64_t* launches) {
  int rc = check_set(h);
  if (rc) return rc;
  if (flush_ms) *flush_ms = h->ingest_ms;
  if (stats_ms) *stats_ms = 0;
  if (launches) *launches = h->launches;
  h->ingest_ms = 0;
  h->launches = 0;
  return GK_OK;
}

}  // extern "C"
