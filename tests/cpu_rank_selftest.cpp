// cpu_rank_selftest.cpp -- TEST INFRASTRUCTURE: gk_ranks and gk_ranks_select of
// the host engine (sketches-py_amd/cpu/gk_cpu.cpp, through include/gk_capi.h +
// gk_cpu.h) against the contract of gk_capi.h applied to the C oracle's
// tables (oracle/gk_oracle.c: one one-stream set per stream, on which only the
// covered streams are flushed): the argument errors first (nothing mutated,
// nothing written), a selection with unsorted ids, a repeat and an empty
// stream, lo only / hi only, more values into every stream, the set-wide call,
// and a merged set.  After every call every stream is compared bit for bit.
// Built with ASan + UBSan by `make -C sketches-py_amd/cpu sanitize-rank`;
// tests/test_cpu_rank.py runs it.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <limits>
#include <random>
#include <vector>

#include "gk_cpu.h"

extern "C" {
typedef struct gko_set gko_set;
gko_set* gko_create(int64_t S, double eps);
void gko_destroy(gko_set* h);
int gko_ingest(gko_set* h, const double* values, const int64_t* offs, int nthreads);
int gko_flush(gko_set* h, int force, int nthreads);
int gko_merge(gko_set* dst, gko_set* src, int nthreads);
void gko_stats(const gko_set* h, int64_t* n, double* mn, double* mx, double* sum, double* avg, int32_t* E,
               int32_t* p);
void gko_export(const gko_set* h, const int64_t* offs, double* v, int64_t* g, int64_t* d);
void gko_export_pending(const gko_set* h, const int64_t* offs, double* v);
}

static int failures = 0;
#define CHECK(c, ...)                   \
  do {                                  \
    if (!(c)) {                         \
      fprintf(stderr, __VA_ARGS__);     \
      fprintf(stderr, "\n");            \
      ++failures;                       \
      return;                           \
    }                                   \
  } while (0)

static bool same_bits(double a, double b) { return memcmp(&a, &b, 8) == 0; }

// full state of a host-engine set
struct State {
  std::vector<int64_t> n, off, poff;
  std::vector<double> f;  // mn, mx, sum, avg: 4 x S
  std::vector<int32_t> E, p, g, d;
  std::vector<double> v, pv;
};

static State state_of(gk_set* a, int64_t S) {
  State st;
  st.n.resize(S);
  st.f.resize(4 * S);
  st.E.resize(S);
  st.p.resize(S);
  gk_stats(a, st.n.data(), st.f.data(), st.f.data() + S, st.f.data() + 2 * S, st.f.data() + 3 * S, st.E.data(),
           st.p.data(), nullptr);
  st.off.assign(S + 1, 0);
  st.poff.assign(S + 1, 0);
  for (int64_t s = 0; s < S; ++s) {
    st.off[s + 1] = st.off[s] + st.E[s];
    st.poff[s + 1] = st.poff[s] + st.p[s];
  }
  st.v.resize(st.off[S] + 1);
  st.g.resize(st.off[S] + 1);
  st.d.resize(st.off[S] + 1);
  st.pv.resize(st.poff[S] + 1);
  gk_export(a, st.off.data(), st.v.data(), st.g.data(), st.d.data(), nullptr);
  gk_export_pending(a, st.poff.data(), st.pv.data(), nullptr);
  return st;
}

static bool same_state(const State& a, const State& b) {
  if (a.n != b.n || a.E != b.E || a.p != b.p || a.g != b.g || a.d != b.d) return false;
  return memcmp(a.f.data(), b.f.data(), a.f.size() * 8) == 0 && memcmp(a.v.data(), b.v.data(), (a.v.size() - 1) * 8) == 0 &&
         memcmp(a.pv.data(), b.pv.data(), (a.pv.size() - 1) * 8) == 0;
}

// one oracle stream's state
struct OStream {
  int64_t n = 0;
  double f[4] = {0, 0, 0, 0};  // mn, mx, sum, avg
  int32_t E = 0, p = 0;
  std::vector<double> v, pv;
  std::vector<int64_t> g, d;
};

static OStream ostream_of(gko_set* o) {
  OStream r;
  gko_stats(o, &r.n, &r.f[0], &r.f[1], &r.f[2], &r.f[3], &r.E, &r.p);
  const int64_t zero[2] = {0, 0};
  r.v.resize(r.E + 1);
  r.g.resize(r.E + 1);
  r.d.resize(r.E + 1);
  r.pv.resize(r.p + 1);
  gko_export(o, zero, r.v.data(), r.g.data(), r.d.data());
  gko_export_pending(o, zero, r.pv.data());
  return r;
}

// stream s of the engine's state against a one-stream oracle set
static void compare_stream(const State& st, int64_t S, int64_t s, gko_set* o, const char* what) {
  const OStream r = ostream_of(o);
  CHECK(st.n[s] == r.n && st.E[s] == r.E && st.p[s] == r.p, "%s stream %lld: n %lld/%lld table %d/%d pending %d/%d",
        what, (long long)s, (long long)st.n[s], (long long)r.n, st.E[s], r.E, st.p[s], r.p);
  for (int k = 0; k < 4; ++k) CHECK(same_bits(st.f[k * S + s], r.f[k]), "%s stream %lld: stat %d", what, (long long)s, k);
  for (int32_t k = 0; k < r.E; ++k)
    CHECK(same_bits(st.v[st.off[s] + k], r.v[k]) && st.g[st.off[s] + k] == r.g[k] && st.d[st.off[s] + k] == r.d[k],
          "%s stream %lld: record %d", what, (long long)s, k);
  for (int32_t k = 0; k < r.p; ++k)
    CHECK(same_bits(st.pv[st.poff[s] + k], r.pv[k]), "%s stream %lld: pending %d", what, (long long)s, k);
}

// the four rules of gk_capi.h on a flushed oracle stream: a plain linear loop
static void formula(const OStream& r, double x, int64_t* lo, int64_t* hi) {
  if (r.n == 0 || x < r.f[0]) {
    *lo = *hi = 0;
    return;
  }
  if (x >= r.f[1]) {
    *lo = *hi = r.n;
    return;
  }
  int32_t i = 0;
  for (int32_t k = 0; k < r.E; ++k)
    if (r.v[k] <= x) ++i;
  int64_t G = 0;
  for (int32_t k = 0; k < i; ++k) G += r.g[k];
  *lo = std::max<int64_t>(G, 1);
  *hi = std::min<int64_t>(i < r.E ? G + r.g[i] + r.d[i] - 1 : r.n, r.n - 1);
}

static std::vector<double> gen(std::mt19937_64& rng, int dist, int64_t L) {
  std::vector<double> x(L);
  std::uniform_real_distribution<double> u(0, 1);
  std::lognormal_distribution<double> ln(0, 1);
  std::uniform_int_distribution<int> small(0, 4);
  for (int64_t i = 0; i < L; ++i) {
    switch (dist) {
      case 0: x[i] = u(rng); break;
      case 1: x[i] = ln(rng); break;
      case 2: x[i] = (double)(L - i); break;  // descending
      case 3: x[i] = (double)i; break;        // ascending
      case 4: x[i] = (double)small(rng); break;  // ties
      default: x[i] = (small(rng) & 1) ? 0.0 : -0.0; break;  // signed zeros
    }
  }
  return x;
}

struct Sets {
  gk_set* eng = nullptr;
  std::vector<gko_set*> orc;
  int64_t S = 0;
  std::mt19937_64 rng;
};

// lens[s] more values into every stream of the engine and of the oracles
static void feed(Sets& z, const std::vector<int64_t>& lens) {
  std::vector<double> flat;
  std::vector<int64_t> offs(z.S + 1, 0);
  for (int64_t s = 0; s < z.S; ++s) {
    auto x = gen(z.rng, (int)(s % 6), lens[s]);
    x.push_back(0);  // (never an empty buffer)
    const int64_t one[2] = {0, lens[s]};
    gko_ingest(z.orc[s], x.data(), one, 1);
    flat.insert(flat.end(), x.begin(), x.end() - 1);
    offs[s + 1] = (int64_t)flat.size();
  }
  flat.push_back(0);
  if (gk_ingest(z.eng, flat.data(), offs.data(), nullptr) != GK_OK) ++failures;
}

static bool make(Sets& z, double eps, const std::vector<int64_t>& lens, uint64_t seed) {
  z.S = (int64_t)lens.size();
  z.rng.seed(seed);
  if (gk_create(z.S, eps, 0, -1, &z.eng) != GK_OK) {
    ++failures;
    return false;
  }
  gk_cpu_set_threads(z.eng, 4);
  for (int64_t s = 0; s < z.S; ++s) z.orc.push_back(gko_create(1, eps));
  feed(z, lens);
  return true;
}

static void drop(Sets& z) {
  gk_destroy(z.eng);
  for (gko_set* o : z.orc) gko_destroy(o);
}

static void compare_all(Sets& z, const char* what) {
  const State st = state_of(z.eng, z.S);
  for (int64_t s = 0; s < z.S; ++s) compare_stream(st, z.S, s, z.orc[s], what);
}

// thresholds from the (flushed copies of the) tables: ends, entries, midpoints
static std::vector<double> thresholds(Sets& z) {
  const double inf = std::numeric_limits<double>::infinity();
  std::vector<double> xs = {inf, -inf, -0.0, 0.0, -3.5, 1e12, 0.5, 2.0};
  for (int64_t s = 0; s < z.S; ++s) {
    const OStream r = ostream_of(z.orc[s]);
    if (r.n == 0) continue;
    xs.push_back(r.f[0]);
    xs.push_back(r.f[1]);
    if (r.E > 0) {
      xs.push_back(r.v[0]);
      xs.push_back(r.v[r.E / 2]);
      xs.push_back(r.v[r.E - 1]);
    }
    if (r.E > 1) xs.push_back((r.v[r.E / 3] + r.v[r.E / 3 + 1]) / 2);
  }
  std::shuffle(xs.begin(), xs.end(), z.rng);
  return xs;
}

// gk_ranks (ids empty) / gk_ranks_select against flush-if-pending + the formula on the covered oracles
static void query(Sets& z, const std::vector<int32_t>& ids, const std::vector<double>& xs, bool want_lo, bool want_hi,
                  const char* what) {
  const bool all = ids.empty();
  const int nx = (int)xs.size();
  const int64_t K = all ? z.S : (int64_t)ids.size();
  std::vector<int64_t> lo(K * nx + 1, -7), hi(K * nx + 1, -7);
  int64_t* plo = want_lo ? lo.data() : nullptr;
  int64_t* phi = want_hi ? hi.data() : nullptr;
  const int rc = all ? gk_ranks(z.eng, xs.data(), nx, plo, phi, nullptr)
                     : gk_ranks_select(z.eng, ids.data(), K, xs.data(), nx, plo, phi, nullptr);
  CHECK(rc == GK_OK, "%s: failed: %s", what, gk_last_error());
  for (int64_t k = 0; k < K; ++k) {
    gko_set* o = z.orc[all ? k : ids[k]];
    gko_flush(o, 1, 1);  // (merge_compress() where values are pending: such a stream has n > 0)
    const OStream r = ostream_of(o);
    for (int j = 0; j < nx; ++j) {
      int64_t el, eh;
      formula(r, xs[j], &el, &eh);
      CHECK(lo[k * nx + j] == (want_lo ? el : -7) && hi[k * nx + j] == (want_hi ? eh : -7),
            "%s: row %lld x %d (%.17g): (%lld, %lld) vs (%lld, %lld)", what, (long long)k, j, xs[j],
            (long long)lo[k * nx + j], (long long)hi[k * nx + j], (long long)el, (long long)eh);
      CHECK(el <= eh, "%s: row %lld x %d: lo > hi", what, (long long)k, j);
    }
  }
  CHECK(lo[K * nx] == -7 && hi[K * nx] == -7, "%s: wrote past the last row", what);
  compare_all(z, what);
}

static void run() {
  const double eps = 0.01;
  const std::vector<int64_t> lens = {0, 1, 50, 99, 100, 101, 150, 202, 1000, 1500, 190, 150, 150, 57, 1313, 0, 707, 303};
  Sets z;
  if (!make(z, eps, lens, 23)) return;
  const int64_t S = z.S;
  const std::vector<double> xs = {0.5, -0.0, 3.0, 1e12, -1e12, 0.25, 100.0};
  const std::vector<int32_t> ids = {10, 3, 11, 8, 0, 6, 3, 9, 5, 1};
  const int64_t K = (int64_t)ids.size();
  const int nx = (int)xs.size();
  // ---- argument errors first: GK_E_ARG, nothing mutated, nothing written
  {
    const State s0 = state_of(z.eng, S);
    std::vector<int64_t> lo(S * nx, -7), hi(S * nx, -7);
    std::vector<int32_t> big = ids, neg = ids;
    big[4] = (int32_t)S;
    neg[7] = -1;
    std::vector<double> nanx = xs;
    nanx[2] = std::numeric_limits<double>::quiet_NaN();
    CHECK(gk_ranks(z.eng, xs.data(), -1, lo.data(), hi.data(), nullptr) == GK_E_ARG, "ranks: nx -1 accepted");
    CHECK(gk_ranks(z.eng, nullptr, nx, lo.data(), hi.data(), nullptr) == GK_E_ARG, "ranks: null xs accepted");
    CHECK(gk_ranks(z.eng, xs.data(), nx, nullptr, nullptr, nullptr) == GK_E_ARG, "ranks: no output accepted");
    CHECK(gk_ranks(z.eng, nanx.data(), nx, lo.data(), hi.data(), nullptr) == GK_E_ARG, "ranks: NaN accepted");
    CHECK(strstr(gk_last_error(), "NaN") != nullptr, "ranks: message without NaN: %s", gk_last_error());
    CHECK(gk_ranks_select(z.eng, big.data(), K, xs.data(), nx, lo.data(), hi.data(), nullptr) == GK_E_ARG,
          "select: id == S accepted");
    CHECK(strstr(gk_last_error(), "ids[4]") != nullptr, "select: message without the first bad index: %s",
          gk_last_error());
    CHECK(gk_ranks_select(z.eng, neg.data(), K, xs.data(), nx, lo.data(), hi.data(), nullptr) == GK_E_ARG,
          "select: id == -1 accepted");
    CHECK(gk_ranks_select(z.eng, ids.data(), K, nanx.data(), nx, lo.data(), hi.data(), nullptr) == GK_E_ARG,
          "select: NaN accepted");
    CHECK(gk_ranks_select(z.eng, ids.data(), K, xs.data(), -1, lo.data(), hi.data(), nullptr) == GK_E_ARG,
          "select: nx -1 accepted");
    CHECK(gk_ranks_select(z.eng, ids.data(), K, xs.data(), nx, nullptr, nullptr, nullptr) == GK_E_ARG,
          "select: no output accepted");
    CHECK(gk_ranks_select(z.eng, nullptr, K, xs.data(), nx, lo.data(), hi.data(), nullptr) == GK_E_ARG,
          "select: null ids accepted");
    CHECK(gk_ranks_select(z.eng, ids.data(), -1, xs.data(), nx, lo.data(), hi.data(), nullptr) == GK_E_ARG,
          "select: count -1 accepted");
    CHECK(gk_ranks_select(z.eng, ids.data(), (int64_t)1 << 31, xs.data(), nx, lo.data(), hi.data(), nullptr) ==
              GK_E_ARG, "select: count 2^31 accepted");
    // count == 0 (ids may be NULL) and nx == 0: GK_OK, nothing touched
    CHECK(gk_ranks_select(z.eng, nullptr, 0, xs.data(), nx, lo.data(), hi.data(), nullptr) == GK_OK, "select: count 0");
    CHECK(gk_ranks_select(z.eng, ids.data(), K, nullptr, 0, nullptr, nullptr, nullptr) == GK_OK, "select: nx 0");
    CHECK(gk_ranks(z.eng, nullptr, 0, nullptr, nullptr, nullptr) == GK_OK, "ranks: nx 0");
    CHECK(same_state(state_of(z.eng, S), s0), "a refused or empty call changed the set");
    for (int64_t x : lo) CHECK(x == -7, "a refused or empty call wrote lo");
    for (int64_t x : hi) CHECK(x == -7, "a refused or empty call wrote hi");
  }
  // ---- a selection (unsorted ids, a repeat, the empty stream), then lo only / hi only
  query(z, ids, xs, true, true, "selection");
  query(z, {12, 2, 12, 15, 14}, thresholds(z), true, false, "lo only");
  query(z, {13, 16, 4}, thresholds(z), false, true, "hi only");
  // ---- more values into every stream, then the set-wide call, twice
  feed(z, std::vector<int64_t>(S, 253));
  compare_all(z, "continued");
  query(z, {17, 0, 9, 17, 7}, {1.0}, true, true, "nx = 1");
  query(z, {}, thresholds(z), true, true, "set-wide");
  {
    const State s1 = state_of(z.eng, S);
    query(z, {}, thresholds(z), true, true, "set-wide again");
    CHECK(same_state(state_of(z.eng, S), s1), "a second gk_ranks changed the set");
  }
  // ---- a merged history: the set merged with a second one, stream by stream
  {
    Sets y;
    if (!make(y, eps, std::vector<int64_t>(S, 333), 29)) return;
    gk_set* srcs[1] = {y.eng};
    CHECK(gk_merge(z.eng, srcs, 1, nullptr) == GK_OK, "merge failed: %s", gk_last_error());
    for (int64_t s = 0; s < S; ++s) gko_merge(z.orc[s], y.orc[s], 1);
    compare_all(z, "merged");
    query(z, {}, thresholds(z), true, true, "merged, set-wide");
    query(z, {4, 4, 0, 15}, thresholds(z), true, true, "merged, selection");
    drop(y);
  }
  drop(z);
}

int main() {
  run();
  if (failures) {
    fprintf(stderr, "cpu_rank_selftest: %d failure(s)\n", failures);
    return 1;
  }
  printf("cpu_rank_selftest: ok\n");
  return 0;
}
