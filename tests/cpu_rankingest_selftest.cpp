// cpu_rankingest_selftest.cpp -- TEST INFRASTRUCTURE: gk_rank_ingest_keyed of
// the host engine (sketches-py_amd/cpu/gk_cpu.cpp, through include/gk_capi.h +
// gk_cpu.h) against its definition, the two-call composition: two engine sets
// are fed the same values; one gets the fused call, its twin gk_ranks_keyed and
// then gk_ingest_keyed.  The three rank outputs, the fused quantiles and the
// complete state of every stream must agree bit for bit; the fused set is also
// compared with the C oracle (oracle/gk_oracle.c: the occurring streams flushed,
// then the batch added sample by sample in arrival order).  Every refusal comes
// first (nothing mutated, nothing written); then random batches with repeats,
// negative ids carrying NaN, signed zeros, infinities and denormals, each
// subset of the outputs (none included), an all-negative batch, the empty call.
// Built with ASan + UBSan by `make -C sketches-py_amd/cpu sanitize-rankingest`;
// tests/test_cpu_rank_ingest.py runs it.
#include <algorithm>
#include <limits>

#include "cpu_selftest_util.h"

static const double kNaN = std::numeric_limits<double>::quiet_NaN();
static const double kInf = std::numeric_limits<double>::infinity();

struct Pair {
  Sets a, b;  // a: the fused call (and the oracles); b: the two calls
  std::mt19937_64 rng;
};

static bool make_pair(Pair& z, double eps, const std::vector<int64_t>& lens, uint64_t seed) {
  z.rng.seed(seed + 1000);
  return make(z.a, eps, lens, seed) && make(z.b, eps, lens, seed);
}

static void feed_pair(Pair& z, const std::vector<int64_t>& lens) {
  feed(z.a, lens);
  feed(z.b, lens);
}

// one fused call on a, the two calls on b, the definition on a's oracles
static void step(Pair& z, const std::vector<int32_t>& ids, const std::vector<double>& xs, int outs, int nq, int mode,
                 const char* what) {
  const int64_t K = (int64_t)ids.size(), S = z.a.S;
  const double qs[3] = {0.5, 0.9, 0.99};
  std::vector<int64_t> lo(K + 1, -7), hi(K + 1, -7), n(K + 1, -7), lo2(K + 1, -7), hi2(K + 1, -7), n2(K + 1, -7);
  std::vector<double> q(S * 3 + 1, -7.0), q2(S * 3 + 1, -7.0);
  int rc = gk_rank_ingest_keyed(z.a.eng, ids.data(), xs.data(), K, (outs & 1) ? lo.data() : nullptr,
                                (outs & 2) ? hi.data() : nullptr, (outs & 4) ? n.data() : nullptr, qs, nq, q.data(), mode,
                                nullptr);
  CHECK(rc == GK_OK, "%s: fused call failed: %s", what, gk_last_error());
  if (outs) {
    rc = gk_ranks_keyed(z.b.eng, ids.data(), xs.data(), K, (outs & 1) ? lo2.data() : nullptr,
                        (outs & 2) ? hi2.data() : nullptr, (outs & 4) ? n2.data() : nullptr, nullptr);
    CHECK(rc == GK_OK, "%s: gk_ranks_keyed failed: %s", what, gk_last_error());
  }
  rc = gk_ingest_keyed(z.b.eng, ids.data(), xs.data(), K, qs, nq, q2.data(), mode, nullptr);
  CHECK(rc == GK_OK, "%s: gk_ingest_keyed failed: %s", what, gk_last_error());
  CHECK(lo == lo2 && hi == hi2 && n == n2, "%s: rank outputs differ from the two calls", what);
  CHECK(memcmp(q.data(), q2.data(), q.size() * 8) == 0, "%s: fused quantiles differ from the two calls", what);
  CHECK(same_state(state_of(z.a.eng, S), state_of(z.b.eng, S)), "%s: states differ from the two calls", what);
  for (int64_t k = 0; k < K; ++k)
    if (ids[k] < 0 && outs)
      CHECK(lo[k] == ((outs & 1) ? 0 : -7) && hi[k] == ((outs & 2) ? 0 : -7) && n[k] == ((outs & 4) ? 0 : -7),
            "%s: row %lld of a negative id", what, (long long)k);
  // the oracles: flush where a rank was taken, the batch in arrival order, the query's flush
  for (int64_t k = 0; k < K; ++k)
    if (ids[k] >= 0 && outs) gko_flush(z.a.orc[ids[k]], 1, 1);
  const int64_t one[2] = {0, 1};
  for (int64_t k = 0; k < K; ++k)
    if (ids[k] >= 0) gko_ingest(z.a.orc[ids[k]], &xs[k], one, 1);
  if (nq > 0)
    for (int64_t s = 0; s < S; ++s) {
      double eq[3];
      gko_flush(z.a.orc[s], 1, 1);  // (quantiles() flushes first)
      gko_quantiles(z.a.orc[s], qs, nq, eq, mode, 1);
      for (int j = 0; j < nq; ++j)
        CHECK(same_bits(eq[j], q[s * nq + j]) || (eq[j] != eq[j] && q[s * nq + j] != q[s * nq + j]),
              "%s: stream %lld quantile %d", what, (long long)s, j);
    }
  compare_all(z.a, what);
}

static void random_batch(Pair& z, int64_t K, int outs, int nq, int mode, const char* what) {
  std::vector<int32_t> ids(K);
  std::vector<double> xs(K);
  const int32_t negs[] = {-1, -7, INT32_MIN};
  const double fixed[] = {-0.0, 0.0, 5e-324, -5e-324, 2.2250738585072009e-308, 0.5, 2.0, -3.5};
  std::lognormal_distribution<double> ln(0, 1);
  for (int64_t k = 0; k < K; ++k) {
    if (z.rng() % 6 == 0) {
      ids[k] = negs[z.rng() % 3];
      xs[k] = (z.rng() & 1) ? kNaN : 1.0;
    } else {
      // (a few hot streams: runs longer than a flush period)
      ids[k] = (int32_t)((z.rng() % 3 == 0) ? z.rng() % 3 : z.rng() % (uint64_t)z.a.S);
      xs[k] = (z.rng() % 4 == 0) ? fixed[z.rng() % 8] : ln(z.rng);
    }
  }
  step(z, ids, xs, outs, nq, mode, what);
}

static void refusals(Pair& z) {
  Sets& a = z.a;
  const int64_t S = a.S;
  const State s0 = state_of(a.eng, S);
  const std::vector<int32_t> ids = {3, -1, 0, 5, 3, 1, -7, 2};
  const std::vector<double> xs = {0.5, kNaN, 1.0, 2.0, -1.0, 0.0, kNaN, 3.0};
  const int64_t K = (int64_t)ids.size();
  std::vector<int64_t> lo(K, -7), hi(K, -7), n(K, -7);
  std::vector<double> q(S * 3, -7.0);
  const double qs[3] = {0.5, 0.9, 0.99}, qnan[3] = {0.5, kNaN, 0.9};
  auto call = [&](const int32_t* i, const double* x, int64_t c, const double* qq = nullptr, int nq = 0,
                  double* out = nullptr, int mode = GK_Q_LIST) {
    return gk_rank_ingest_keyed(a.eng, i, x, c, lo.data(), hi.data(), n.data(), qq, nq, out, mode, nullptr);
  };
  CHECK(call(ids.data(), xs.data(), -1) == GK_E_ARG, "count -1 accepted");
  CHECK(call(ids.data(), xs.data(), (int64_t)1 << 31) == GK_E_ARG, "count 2^31 accepted");
  CHECK(call(nullptr, xs.data(), K) == GK_E_ARG, "null ids accepted");
  CHECK(call(ids.data(), nullptr, K) == GK_E_ARG, "null xs accepted");
  CHECK(call(ids.data(), xs.data(), K, qs, 3, nullptr) == GK_E_ARG, "nq > 0 with a null out accepted");
  CHECK(call(ids.data(), xs.data(), K, nullptr, 3, q.data()) == GK_E_ARG, "nq > 0 with a null qs accepted");
  CHECK(call(ids.data(), xs.data(), K, qnan, 3, q.data()) == GK_E_ARG, "a NaN in qs accepted");
  CHECK(call(ids.data(), xs.data(), K, qs, -1, q.data()) == GK_E_ARG, "nq -1 accepted");
  CHECK(call(ids.data(), xs.data(), K, qs, 3, q.data(), 7) == GK_E_ARG, "mode 7 accepted");
  CHECK(call(nullptr, nullptr, 0, qnan, 3, q.data()) == GK_E_ARG, "a NaN in qs accepted at count 0");
  {
    std::vector<int32_t> big = ids;
    big[3] = (int32_t)S;
    CHECK(call(big.data(), xs.data(), K) == GK_E_ARG, "id == S accepted");
    CHECK(strstr(gk_last_error(), "ids[3]") != nullptr, "id == S: message without the index: %s", gk_last_error());
  }
  {
    std::vector<double> nanx = xs;
    nanx[5] = kNaN;
    CHECK(call(ids.data(), nanx.data(), K, qs, 3, q.data()) == GK_E_ARG, "NaN on a live row accepted");
    CHECK(strstr(gk_last_error(), "xs[5]") != nullptr && strstr(gk_last_error(), "NaN") != nullptr,
          "NaN: message without index or NaN: %s", gk_last_error());
    // the NaN refusal holds without any rank output too
    CHECK(gk_rank_ingest_keyed(a.eng, ids.data(), nanx.data(), K, nullptr, nullptr, nullptr, nullptr, 0, nullptr,
                               GK_Q_LIST, nullptr) == GK_E_ARG,
          "NaN on a live row accepted without rank outputs");
    // both faults at different indices: the smallest index decides
    std::vector<int32_t> big = ids;
    big[7] = (int32_t)S + 4;
    CHECK(call(big.data(), nanx.data(), K) == GK_E_ARG, "NaN then bad id accepted");
    CHECK(strstr(gk_last_error(), "xs[5]") != nullptr, "NaN first: %s", gk_last_error());
    big[2] = (int32_t)S;
    CHECK(call(big.data(), nanx.data(), K) == GK_E_ARG, "bad id then NaN accepted");
    CHECK(strstr(gk_last_error(), "ids[2]") != nullptr, "bad id first: %s", gk_last_error());
    // both at one index: the id is reported
    big = ids;
    big[5] = (int32_t)S;
    CHECK(call(big.data(), nanx.data(), K) == GK_E_ARG, "bad id with NaN accepted");
    CHECK(strstr(gk_last_error(), "ids[5]") != nullptr && strstr(gk_last_error(), "xs[") == nullptr,
          "same index: the id wins: %s", gk_last_error());
  }
  // the empty call without a query: GK_OK, nothing touched (arrays may be NULL)
  CHECK(call(nullptr, nullptr, 0) == GK_OK, "count 0 refused");
  CHECK(same_state(state_of(a.eng, S), s0), "a refused or empty call changed the set");
  for (int64_t k = 0; k < K; ++k) CHECK(lo[k] == -7 && hi[k] == -7 && n[k] == -7, "a refused or empty call wrote a row");
  for (double x : q) CHECK(x == -7.0, "a refused or empty call wrote a quantile");
}

static void run() {
  const double eps = 0.01;
  const std::vector<int64_t> lens = {0, 1, 50, 99, 100, 101, 150, 202, 1000, 1500, 190, 150, 150, 57, 1313, 0, 707, 303};
  Pair z;
  if (!make_pair(z, eps, lens, 41)) return;
  refusals(z);
  {
    const State s0 = state_of(z.a.eng, z.a.S);
    step(z, {-1, INT32_MIN, -7}, {kNaN, 1.0, kNaN}, 7, 0, GK_Q_LIST, "all negative");
    CHECK(same_state(state_of(z.a.eng, z.a.S), s0), "an all-negative batch changed the set");
  }
  step(z, {}, {}, 7, 3, GK_Q_LIST, "count 0 with a query");
  step(z, {9}, {0.5}, 7, 0, GK_Q_LIST, "one sample");
  // infinities last in their streams (no inf - inf in _sum / _avg); streams 0 and 15 are empty
  step(z, {0, 15, 0, 15, 0, 15}, {-0.0, -5e-324, 5e-324, 0.0, kInf, -kInf}, 7, 0, GK_Q_LIST, "special values");
  random_batch(z, 300, 7, 0, GK_Q_LIST, "batch");
  random_batch(z, 300, 7, 0, GK_Q_LIST, "batch again");
  random_batch(z, 64, 1, 0, GK_Q_LIST, "lo only");
  random_batch(z, 65, 2, 3, GK_Q_LIST, "hi only, quantiles");
  random_batch(z, 63, 4, 3, GK_Q_SINGLE, "n only, single");
  random_batch(z, 129, 0, 0, GK_Q_LIST, "no rank output");
  random_batch(z, 200, 0, 3, GK_Q_LIST, "no rank output, quantiles");
  for (int round = 0; round < 4; ++round) {
    std::vector<int64_t> more(z.a.S);
    for (auto& m : more) m = (int64_t)(z.rng() % 260);
    feed_pair(z, more);
    random_batch(z, 500 + 37 * round, 3 + 4 * (round & 1), 3 * (round & 1), GK_Q_LIST, "round");
  }
  // other eps: the period-1 set (eps > 1) and a fine one
  for (double e : {2.0, 0.001}) {
    Pair y;
    if (!make_pair(y, e, {0, 3, 700, 1, 2500, 64}, 43)) return;
    random_batch(y, 257, 7, 3, GK_Q_LIST, "other eps");
    feed_pair(y, std::vector<int64_t>(y.a.S, 129));
    random_batch(y, 129, 7, 0, GK_Q_LIST, "other eps, continued");
    drop(y.a);
    drop(y.b);
  }
  // a set without streams: every id is negative
  {
    gk_set* none = nullptr;
    CHECK(gk_create(0, eps, 0, -1, &none) == GK_OK, "S = 0: create");
    const int32_t ids[2] = {-1, -7};
    const double xs[2] = {kNaN, 1.0};
    int64_t lo[2] = {-7, -7}, n[2] = {-7, -7};
    CHECK(gk_rank_ingest_keyed(none, ids, xs, 2, lo, nullptr, n, nullptr, 0, nullptr, GK_Q_LIST, nullptr) == GK_OK,
          "S = 0 refused: %s", gk_last_error());
    CHECK(lo[0] == 0 && lo[1] == 0 && n[0] == 0 && n[1] == 0, "S = 0: rows not zero");
    const int32_t zero[1] = {0};
    CHECK(gk_rank_ingest_keyed(none, zero, xs + 1, 1, lo, nullptr, n, nullptr, 0, nullptr, GK_Q_LIST, nullptr) == GK_E_ARG,
          "S = 0: id 0 accepted");
    gk_destroy(none);
  }
  drop(z.a);
  drop(z.b);
}

int main() {
  run();
  return selftest_result("cpu_rankingest_selftest");
}
