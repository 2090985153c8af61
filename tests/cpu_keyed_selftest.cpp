// cpu_keyed_selftest.cpp -- TEST INFRASTRUCTURE: gk_group_by_key and
// gk_ingest_keyed of the host engine (sketches-py_amd/cpu/gk_cpu.cpp, through
// include/gk_capi.h + gk_cpu.h) at reduced size:
//  1. the grouping shapes of tests/keyed_cases.py against std::stable_sort of
//     the kept sample indices by id (values bit for bit, special values kept);
//  2. keyed ingest against the C oracle (oracle/gk_oracle.c) fed one sample at
//     a time in arrival order: three keyed calls with a CSR ingest between
//     them, skewed ids, Pareto values, eps 0.1 and 0.01;
// then the argument errors (nothing mutated, out_offsets all zero).
// Built with ASan + UBSan by `make -C sketches-py_amd/cpu sanitize-keyed`;
// tests/test_cpu_keyed.py runs it.
#include <algorithm>
#include <limits>
#include <numeric>

#include "cpu_selftest_util.h"

static double from_bits(uint64_t b) {
  double d;
  memcpy(&d, &b, 8);
  return d;
}

// ---- 1. grouping -----------------------------------------------------------
static void group_case(const char* what, int64_t S, const std::vector<int32_t>& ids) {
  const int64_t N = (int64_t)ids.size();
  std::vector<double> vals(N + 1);
  for (int64_t i = 0; i < N; ++i) vals[i] = (double)i;
  const double special[] = {-0.0, std::numeric_limits<double>::infinity(), -std::numeric_limits<double>::infinity(),
                            4.9406564584124654e-324, from_bits(0x7ff8000000000001ull), from_bits(0xfff4000000000bedull)};
  for (int k = 0; k < 6 && N > 0; ++k) vals[(int64_t)(k * 7919) % N] = special[k];
  gk_set* h = nullptr;
  CHECK(gk_create(S, 0.01, 0, -1, &h) == GK_OK, "%s: create", what);
  std::vector<double> out(N + 1, -1.0);
  std::vector<int64_t> offs(S + 1, -1);
  const int rc = gk_group_by_key(h, N ? ids.data() : nullptr, N ? vals.data() : nullptr, N, N ? out.data() : nullptr,
                                 offs.data(), nullptr);
  gk_destroy(h);
  CHECK(rc == GK_OK, "%s: gk_group_by_key failed: %s", what, gk_last_error());
  std::vector<int64_t> order;
  for (int64_t i = 0; i < N; ++i)
    if (ids[i] >= 0) order.push_back(i);
  std::stable_sort(order.begin(), order.end(), [&](int64_t a, int64_t b) { return ids[a] < ids[b]; });
  std::vector<int64_t> exp(S + 1, 0);
  for (int64_t i : order) ++exp[ids[i] + 1];
  for (int64_t s = 0; s < S; ++s) exp[s + 1] += exp[s];
  CHECK(exp == offs, "%s: offsets differ", what);
  for (size_t k = 0; k < order.size(); ++k)
    CHECK(memcmp(&out[k], &vals[order[k]], 8) == 0, "%s: value %zu differs", what, k);
}

static void group_cases() {
  std::mt19937_64 rng(5);
  auto uniform = [&](int64_t S, int64_t N, int32_t lo) {
    std::uniform_int_distribution<int32_t> u(lo, (int32_t)S - 1);
    std::vector<int32_t> ids(N);
    for (auto& x : ids) x = u(rng);
    return ids;
  };
  group_case("S=1", 1, std::vector<int32_t>(2011, 0));
  for (int64_t N : {0, 1, 63, 64, 65}) group_case("S=1000 small N", 1000, uniform(1000, N, -1));
  group_case("S=257 with skips", 257, uniform(257, 2011, -1));
  {
    std::vector<int32_t> pick = uniform(65537, 300, 0), ids(1500);
    pick[0] = 0;
    pick[1] = 65536;
    for (size_t i = 0; i < ids.size(); ++i) ids[i] = pick[i < 2 ? i : rng() % pick.size()];
    group_case("S=65537 sparse", 65537, ids);
  }
  {
    const int64_t S = 419;
    std::vector<int32_t> ids(10 * S + 3);
    for (size_t i = 0; i < ids.size(); ++i) ids[i] = (int32_t)(i % S);
    group_case("round robin", S, ids);
    std::vector<int32_t> asc = uniform(S, 3011, 0);
    std::sort(asc.begin(), asc.end());
    group_case("ascending", S, asc);
    std::reverse(asc.begin(), asc.end());
    group_case("descending", S, asc);
  }
  {
    std::vector<int32_t> ids = uniform(1000003, 20000, 0);
    for (size_t i = 0; i < ids.size(); i += 2) ids[i] = 777777;
    group_case("hot key", 1000003, ids);
  }
}

// ---- 2. keyed ingest vs the oracle's per-sample loop ------------------------
static void compare_with_oracle(gk_set* h, gko_set* o, int64_t S, const char* what) {
  const State st = state_of(h, S);
  std::vector<int64_t> n(S);
  std::vector<double> f(4 * S);
  std::vector<int32_t> E(S), p(S);
  gko_stats(o, n.data(), f.data(), f.data() + S, f.data() + 2 * S, f.data() + 3 * S, E.data(), p.data());
  CHECK(n == st.n && E == st.E && p == st.p, "%s: n / table sizes / pending counts differ", what);
  CHECK(memcmp(f.data(), st.f.data(), f.size() * 8) == 0, "%s: min/max/sum/avg differ", what);
  std::vector<double> v(st.off[S] + 1), pv(st.poff[S] + 1);
  std::vector<int64_t> g(st.off[S] + 1), d(st.off[S] + 1);
  gko_export(o, st.off.data(), v.data(), g.data(), d.data());
  gko_export_pending(o, st.poff.data(), pv.data());
  CHECK(memcmp(v.data(), st.v.data(), st.off[S] * 8) == 0, "%s: table values differ", what);
  for (int64_t k = 0; k < st.off[S]; ++k) CHECK(g[k] == st.g[k] && d[k] == st.d[k], "%s: record %lld", what, (long long)k);
  CHECK(memcmp(pv.data(), st.pv.data(), st.poff[S] * 8) == 0, "%s: pending values differ", what);
}

static void ingest_case(double eps) {
  const int64_t S = 37, N = 1500;
  char what[64];
  snprintf(what, sizeof(what), "keyed ingest eps=%g", eps);
  std::mt19937_64 rng(77);
  std::uniform_real_distribution<double> u(0, 1);
  gk_set* h = nullptr;
  CHECK(gk_create(S, eps, 0, -1, &h) == GK_OK, "%s: create", what);
  gk_cpu_set_threads(h, 4);
  gko_set* o = gko_create(S, eps);
  auto oracle_add = [&](int32_t id, double v) {
    std::vector<int64_t> offs(S + 1, 0);
    for (int64_t s = id + 1; s <= S; ++s) offs[s] = 1;
    gko_ingest(o, &v, offs.data(), 1);
  };
  for (int call = 0; call < 3; ++call) {
    std::vector<int32_t> ids(N);
    std::vector<double> vals(N);
    for (int64_t i = 0; i < N; ++i) {
      const double r = u(rng);
      ids[i] = r < 0.4 ? 5 : (r < 0.45 ? -1 : (int32_t)(rng() % S));  // stream 5 gets ~40 %, some skipped
      vals[i] = pow(1.0 - u(rng), -1.0 / 1.5);                        // Pareto
    }
    CHECK(gk_ingest_keyed(h, ids.data(), vals.data(), N, nullptr, 0, nullptr, GK_Q_LIST, nullptr) == GK_OK,
          "%s: gk_ingest_keyed failed: %s", what, gk_last_error());
    for (int64_t i = 0; i < N; ++i)
      if (ids[i] >= 0) oracle_add(ids[i], vals[i]);
    if (call == 0) {  // a plain CSR ingest between the keyed calls: pending values carry across
      std::vector<double> flat;
      std::vector<int64_t> offs(S + 1, 0);
      for (int64_t s = 0; s < S; ++s) {
        for (int64_t k = 0; k < s % 7; ++k) flat.push_back(pow(1.0 - u(rng), -1.0 / 1.5));
        offs[s + 1] = (int64_t)flat.size();
      }
      flat.push_back(0);
      CHECK(gk_ingest(h, flat.data(), offs.data(), nullptr) == GK_OK, "%s: gk_ingest", what);
      gko_ingest(o, flat.data(), offs.data(), 1);
    }
    compare_with_oracle(h, o, S, what);
  }
  // errors: id == S among valid ones, bad count; nothing mutated, offsets zero
  {
    const State before = state_of(h, S);
    std::vector<int32_t> ids = {0, 3, (int32_t)S, 4};
    std::vector<double> vals = {1, 2, 3, 4}, out(4);
    std::vector<int64_t> offs(S + 1, 7);
    CHECK(gk_ingest_keyed(h, ids.data(), vals.data(), 4, nullptr, 0, nullptr, GK_Q_LIST, nullptr) == GK_E_ARG,
          "%s: id == S accepted", what);
    CHECK(gk_group_by_key(h, ids.data(), vals.data(), 4, out.data(), offs.data(), nullptr) == GK_E_ARG,
          "%s: id == S grouped", what);
    CHECK(std::count(offs.begin(), offs.end(), 0) == S + 1, "%s: offsets not zero after a bad id", what);
    CHECK(gk_ingest_keyed(h, ids.data(), vals.data(), -1, nullptr, 0, nullptr, GK_Q_LIST, nullptr) == GK_E_ARG,
          "%s: count -1 accepted", what);
    CHECK(gk_ingest_keyed(h, ids.data(), vals.data(), (int64_t)1 << 31, nullptr, 0, nullptr, GK_Q_LIST, nullptr) ==
              GK_E_ARG, "%s: count 2^31 accepted", what);
    CHECK(gk_ingest_keyed(h, nullptr, nullptr, 0, nullptr, 0, nullptr, GK_Q_LIST, nullptr) == GK_OK,
          "%s: empty keyed call refused", what);
    CHECK(same_state(state_of(h, S), before), "%s: a refused or empty call changed the set", what);
  }
  gk_destroy(h);
  gko_destroy(o);
}

int main() {
  group_cases();
  ingest_case(0.1);
  ingest_case(0.01);
  return selftest_result("cpu_keyed_selftest");
}
