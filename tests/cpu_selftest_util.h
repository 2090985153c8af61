// cpu_selftest_util.h -- TEST INFRASTRUCTURE shared by the stand-alone
// self-tests of the host engine (tests/cpu_*selftest.cpp, built with ASan +
// UBSan by sketches-py_amd/cpu/Makefile): the C oracle's prototypes
// (oracle/gk_oracle.c), CHECK and the failure count, bit-for-bit comparison of
// an engine set's full state with itself (State) and with one-stream oracle
// sets (OStream, compare_stream), the seeded value generator, and a set with
// one oracle per stream (Sets).  Each program keeps only its own cases.
#pragma once

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
int gko_flush(gko_set* h, int force, int nthreads);
int gko_quantiles(gko_set* h, const double* qs, int nq, double* out, int mode, int nthreads);
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

// the tail of every main(): the program's verdict line and exit status
static inline int selftest_result(const char* name) {
  if (failures) {
    fprintf(stderr, "%s: %d failure(s)\n", name, failures);
    return 1;
  }
  printf("%s: ok\n", name);
  return 0;
}

static inline bool same_bits(double a, double b) { return memcmp(&a, &b, 8) == 0; }

// full state of a host-engine set
struct State {
  std::vector<int64_t> n, off, poff;
  std::vector<double> f;  // mn, mx, sum, avg: 4 x S
  std::vector<int32_t> E, p, g, d;
  std::vector<double> v, pv;
};

static inline State state_of(gk_set* a, int64_t S) {
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

static inline bool same_state(const State& a, const State& b) {
  if (a.n != b.n || a.E != b.E || a.p != b.p || a.g != b.g || a.d != b.d) return false;
  return memcmp(a.f.data(), b.f.data(), a.f.size() * 8) == 0 &&
         memcmp(a.v.data(), b.v.data(), (a.v.size() - 1) * 8) == 0 &&
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

static inline OStream ostream_of(gko_set* o) {
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
static inline void compare_stream(const State& st, int64_t S, int64_t s, gko_set* o, const char* what) {
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

static inline std::vector<double> gen(std::mt19937_64& rng, int dist, int64_t L) {
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

// an engine set and one one-stream oracle set per stream, fed the same values
struct Sets {
  gk_set* eng = nullptr;
  std::vector<gko_set*> orc;
  int64_t S = 0;
  std::mt19937_64 rng;
};

// lens[s] more values into every stream of the engine and of the oracles
static inline void feed(Sets& z, const std::vector<int64_t>& lens) {
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

static inline bool make(Sets& z, double eps, const std::vector<int64_t>& lens, uint64_t seed) {
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

static inline void drop(Sets& z) {
  gk_destroy(z.eng);
  for (gko_set* o : z.orc) gko_destroy(o);
}

static inline void compare_all(Sets& z, const char* what) {
  const State st = state_of(z.eng, z.S);
  for (int64_t s = 0; s < z.S; ++s) compare_stream(st, z.S, s, z.orc[s], what);
}
