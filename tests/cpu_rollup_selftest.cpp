// cpu_rollup_selftest.cpp -- TEST INFRASTRUCTURE: gk_rollup of the host engine
// (sketches-py_amd/cpu/gk_cpu.cpp, through include/gk_capi.h + gk_cpu.h)
// against the C oracle (oracle/gk_oracle.c: one one-stream set per source and
// destination stream, gko_merge in member order) on the shapes of the mixed
// roll-up case of tests/rollup_cases.py: a 17-member group, groups of 0, 1, 2
// and 5, empty members first, only empty members, non-members with pending
// values; a fresh and a pre-ingested destination; then the argument errors.
// Built with ASan + UBSan by `make -C sketches-py_amd/cpu sanitize-rollup`;
// tests/test_cpu_rollup.py runs it.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <random>
#include <vector>

#include "gk_cpu.h"

extern "C" {
typedef struct gko_set gko_set;
gko_set* gko_create(int64_t S, double eps);
void gko_destroy(gko_set* h);
int gko_ingest(gko_set* h, const double* values, const int64_t* offs, int nthreads);
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

// stream s of the engine's state against a one-stream oracle set
static void compare_stream(const State& st, int64_t S, int64_t s, gko_set* o, const char* what) {
  int64_t n = 0;
  double f[4];
  int32_t E = 0, p = 0;
  gko_stats(o, &n, &f[0], &f[1], &f[2], &f[3], &E, &p);
  CHECK(st.n[s] == n && st.E[s] == E && st.p[s] == p, "%s stream %lld: n %lld/%lld table %d/%d pending %d/%d", what,
        (long long)s, (long long)st.n[s], (long long)n, st.E[s], E, st.p[s], p);
  for (int k = 0; k < 4; ++k) CHECK(same_bits(st.f[k * S + s], f[k]), "%s stream %lld: stat %d", what, (long long)s, k);
  const int64_t zero[2] = {0, 0};
  std::vector<double> v(E + 1), pv(p + 1);
  std::vector<int64_t> g(E + 1), d(E + 1);
  gko_export(o, zero, v.data(), g.data(), d.data());
  gko_export_pending(o, zero, pv.data());
  for (int32_t k = 0; k < E; ++k)
    CHECK(same_bits(st.v[st.off[s] + k], v[k]) && st.g[st.off[s] + k] == g[k] && st.d[st.off[s] + k] == d[k],
          "%s stream %lld: record %d", what, (long long)s, k);
  for (int32_t k = 0; k < p; ++k) CHECK(same_bits(st.pv[st.poff[s] + k], pv[k]), "%s stream %lld: pending %d", what,
                                        (long long)s, k);
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
};

static Sets make(double eps, const std::vector<int64_t>& lens, uint64_t seed) {
  Sets z;
  z.S = (int64_t)lens.size();
  std::mt19937_64 rng(seed);
  if (gk_create(z.S, eps, 0, -1, &z.eng) != GK_OK) {
    ++failures;
    return z;
  }
  gk_cpu_set_threads(z.eng, 4);
  std::vector<double> flat;
  std::vector<int64_t> offs(z.S + 1, 0);
  for (int64_t s = 0; s < z.S; ++s) {
    auto x = gen(rng, (int)(s % 6), lens[s]);
    x.push_back(0);  // (never an empty buffer)
    const int64_t one[2] = {0, lens[s]};
    gko_set* o = gko_create(1, eps);
    gko_ingest(o, x.data(), one, 1);
    z.orc.push_back(o);
    flat.insert(flat.end(), x.begin(), x.end() - 1);
    offs[s + 1] = (int64_t)flat.size();
  }
  flat.push_back(0);
  gk_ingest(z.eng, flat.data(), offs.data(), nullptr);
  return z;
}

static void drop(Sets& z) {
  gk_destroy(z.eng);
  for (gko_set* o : z.orc) gko_destroy(o);
}

static void run(bool pre) {
  const double eps = 0.01;
  std::vector<int64_t> lens = {1000, 0, 1, 100, 101, 102, 1500, 999, 202, 303, 1000, 1000, 50, 707, 1313, 1000, 1000,
                               450, 1000, 57, 300, 0, 1212, 99, 101, 0, 0, 640, 0, 0,
                               57, 157, 1033, 5, 250, 99};
  const std::vector<std::vector<int64_t>> groups = {{0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16}, {}, {17},
                                                    {19, 18}, {20, 21, 22, 23, 24}, {25, 26, 27}, {28, 29}};
  const int64_t G = (int64_t)groups.size();
  std::vector<int64_t> dlens = {1000, 57, 57, 0, 1000, 0, 57};
  if (!pre) dlens.assign(G, 0);
  Sets src = make(eps, lens, 11), dst = make(eps, dlens, 12);
  if (!src.eng || !dst.eng) return;
  std::vector<int64_t> go(G + 1, 0), mem;
  std::vector<char> is_member(src.S, 0);
  for (int64_t j = 0; j < G; ++j) {
    for (int64_t m : groups[j]) {
      mem.push_back(m);
      is_member[m] = 1;
    }
    go[j + 1] = (int64_t)mem.size();
  }
  const char* what = pre ? "pre-ingested dst" : "fresh dst";
  // ---- argument errors first: GK_E_ARG, nothing mutated
  const State s0 = state_of(src.eng, src.S), d0 = state_of(dst.eng, dst.S);
  {
    std::vector<int64_t> dup = mem, hi = mem, neg = mem, dec = go, first = go;
    dup[3] = dup[0];
    hi[5] = src.S;
    neg[7] = -1;
    dec[2] = dec[3] + 1;
    first[0] = 1;
    CHECK(gk_rollup(dst.eng, src.eng, go.data(), dup.data(), nullptr) == GK_E_ARG, "%s: duplicate member accepted", what);
    CHECK(gk_rollup(dst.eng, src.eng, go.data(), hi.data(), nullptr) == GK_E_ARG, "%s: member == S accepted", what);
    CHECK(gk_rollup(dst.eng, src.eng, go.data(), neg.data(), nullptr) == GK_E_ARG, "%s: member -1 accepted", what);
    CHECK(gk_rollup(dst.eng, src.eng, dec.data(), mem.data(), nullptr) == GK_E_ARG, "%s: decreasing offsets accepted", what);
    CHECK(gk_rollup(dst.eng, src.eng, first.data(), mem.data(), nullptr) == GK_E_ARG, "%s: offsets from 1 accepted", what);
    CHECK(gk_rollup(dst.eng, dst.eng, go.data(), mem.data(), nullptr) == GK_E_ARG, "%s: dst == src accepted", what);
    CHECK(gk_rollup(dst.eng, src.eng, nullptr, mem.data(), nullptr) == GK_E_ARG, "%s: null offsets accepted", what);
    CHECK(gk_rollup(dst.eng, src.eng, go.data(), nullptr, nullptr) == GK_E_ARG, "%s: null members accepted", what);
    CHECK(same_state(state_of(src.eng, src.S), s0) && same_state(state_of(dst.eng, dst.S), d0),
          "%s: a refused call changed a set", what);
  }
  // ---- the roll-up and the oracle's loop of merges
  CHECK(gk_rollup(dst.eng, src.eng, go.data(), mem.data(), nullptr) == GK_OK, "%s: gk_rollup failed: %s", what,
        gk_last_error());
  for (int64_t j = 0; j < G; ++j)
    for (int64_t m : groups[j]) gko_merge(dst.orc[j], src.orc[m], 1);
  const State s1 = state_of(src.eng, src.S), d1 = state_of(dst.eng, dst.S);
  for (int64_t j = 0; j < G; ++j) compare_stream(d1, dst.S, j, dst.orc[j], what);
  for (int64_t s = 0; s < src.S; ++s) compare_stream(s1, src.S, s, src.orc[s], is_member[s] ? "member" : "non-member");
  drop(src);
  drop(dst);
}

int main() {
  run(false);
  run(true);
  if (failures) {
    fprintf(stderr, "cpu_rollup_selftest: %d failure(s)\n", failures);
    return 1;
  }
  printf("cpu_rollup_selftest: ok\n");
  return 0;
}
