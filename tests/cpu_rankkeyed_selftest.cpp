// cpu_rankkeyed_selftest.cpp -- TEST INFRASTRUCTURE: gk_ranks_keyed of the host
// engine (sketches-py_amd/cpu/gk_cpu.cpp, through include/gk_capi.h + gk_cpu.h)
// against the contract of gk_capi.h applied to the C oracle's tables
// (oracle/gk_oracle.c: one one-stream set per stream, on which only the
// occurring streams are flushed): every refusal first (nothing mutated,
// nothing written), then random sets and random batches of (id, x) samples
// with repeats, negative ids carrying NaN, thresholds taken from the tables,
// each subset of the three outputs, an all-negative batch and the empty call.
// After every call every stream is compared bit for bit.
// Built with ASan + UBSan by `make -C sketches-py_amd/cpu sanitize-rankkeyed`;
// tests/test_cpu_rank_keyed.py runs it.
#include <algorithm>
#include <limits>

#include "cpu_selftest_util.h"

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

static const double kNaN = std::numeric_limits<double>::quiet_NaN();
static const double kInf = std::numeric_limits<double>::infinity();

// a threshold for stream s: an end, an entry, a midpoint or a constant
static double pick_x(Sets& z, int64_t s) {
  const OStream r = ostream_of(z.orc[s]);
  const double fixed[] = {kInf, -kInf, -0.0, 0.0, -3.5, 1e12, 0.5, 2.0};
  const int what = (int)(z.rng() % 8);
  if (r.n == 0 || what >= 5) return fixed[z.rng() % 8];
  if (what == 0) return r.f[0];
  if (what == 1) return r.f[1];
  if (r.E == 0) return r.pv[z.rng() % (uint64_t)r.p];
  const int32_t k = (int32_t)(z.rng() % (uint64_t)r.E);
  if (what == 2) return r.v[k];
  if (what == 3) return k + 1 < r.E ? (r.v[k] + r.v[k + 1]) / 2 : r.v[k] + 1.0;
  return nextafter(r.v[k], -kInf);
}

// one call against flush-if-pending of the occurring streams + the formula
static void query(Sets& z, const std::vector<int32_t>& ids, const std::vector<double>& xs, int outs, const char* what) {
  const int64_t K = (int64_t)ids.size();
  std::vector<int64_t> lo(K + 1, -7), hi(K + 1, -7), n(K + 1, -7);
  const int rc = gk_ranks_keyed(z.eng, ids.data(), xs.data(), K, (outs & 1) ? lo.data() : nullptr,
                                (outs & 2) ? hi.data() : nullptr, (outs & 4) ? n.data() : nullptr, nullptr);
  CHECK(rc == GK_OK, "%s: failed: %s", what, gk_last_error());
  for (int64_t k = 0; k < K; ++k)
    if (ids[k] >= 0) gko_flush(z.orc[ids[k]], 1, 1);  // (merge_compress() where values are pending)
  for (int64_t k = 0; k < K; ++k) {
    int64_t el = 0, eh = 0, en = 0;
    if (ids[k] >= 0) {
      const OStream r = ostream_of(z.orc[ids[k]]);
      formula(r, xs[k], &el, &eh);
      en = r.n;
    }
    CHECK(lo[k] == ((outs & 1) ? el : -7) && hi[k] == ((outs & 2) ? eh : -7) && n[k] == ((outs & 4) ? en : -7),
          "%s: row %lld (id %d, x %.17g): (%lld, %lld, %lld) vs (%lld, %lld, %lld)", what, (long long)k, ids[k], xs[k],
          (long long)lo[k], (long long)hi[k], (long long)n[k], (long long)el, (long long)eh, (long long)en);
  }
  CHECK(lo[K] == -7 && hi[K] == -7 && n[K] == -7, "%s: wrote past the last row", what);
  compare_all(z, what);
}

static void random_batch(Sets& z, int64_t K, int outs, const char* what) {
  std::vector<int32_t> ids(K);
  std::vector<double> xs(K);
  const int32_t negs[] = {-1, -7, INT32_MIN};
  for (int64_t k = 0; k < K; ++k) {
    if (z.rng() % 6 == 0) {
      ids[k] = negs[z.rng() % 3];
      xs[k] = (z.rng() & 1) ? kNaN : 1.0;
    } else {
      // (a few hot streams: many repeats)
      ids[k] = (int32_t)((z.rng() % 3 == 0) ? z.rng() % 3 : z.rng() % (uint64_t)z.S);
      xs[k] = pick_x(z, ids[k]);
    }
  }
  query(z, ids, xs, outs, what);
}

static void refusals(Sets& z) {
  const int64_t S = z.S;
  const State s0 = state_of(z.eng, S);
  const std::vector<int32_t> ids = {3, -1, 0, 5, 3, 1, -7, 2};
  const std::vector<double> xs = {0.5, kNaN, 1.0, 2.0, -1.0, 0.0, kNaN, 3.0};
  const int64_t K = (int64_t)ids.size();
  std::vector<int64_t> lo(K, -7), hi(K, -7), n(K, -7);
  auto call = [&](const int32_t* i, const double* x, int64_t c, int64_t* l, int64_t* h, int64_t* m) {
    return gk_ranks_keyed(z.eng, i, x, c, l, h, m, nullptr);
  };
  CHECK(call(ids.data(), xs.data(), -1, lo.data(), hi.data(), n.data()) == GK_E_ARG, "count -1 accepted");
  CHECK(call(ids.data(), xs.data(), (int64_t)1 << 31, lo.data(), hi.data(), n.data()) == GK_E_ARG, "count 2^31 accepted");
  CHECK(call(nullptr, xs.data(), K, lo.data(), hi.data(), n.data()) == GK_E_ARG, "null ids accepted");
  CHECK(call(ids.data(), nullptr, K, lo.data(), hi.data(), n.data()) == GK_E_ARG, "null xs accepted");
  CHECK(call(ids.data(), xs.data(), K, nullptr, nullptr, nullptr) == GK_E_ARG, "no output accepted");
  CHECK(call(nullptr, nullptr, 0, nullptr, nullptr, nullptr) == GK_E_ARG, "no output accepted with count 0");
  {
    std::vector<int32_t> big = ids;
    big[3] = (int32_t)S;
    CHECK(call(big.data(), xs.data(), K, lo.data(), hi.data(), n.data()) == GK_E_ARG, "id == S accepted");
    CHECK(strstr(gk_last_error(), "ids[3]") != nullptr, "id == S: message without the index: %s", gk_last_error());
  }
  {
    std::vector<double> nanx = xs;
    nanx[5] = kNaN;
    CHECK(call(ids.data(), nanx.data(), K, lo.data(), hi.data(), n.data()) == GK_E_ARG, "NaN on a live row accepted");
    CHECK(strstr(gk_last_error(), "xs[5]") != nullptr && strstr(gk_last_error(), "NaN") != nullptr,
          "NaN: message without index or NaN: %s", gk_last_error());
    // both faults at different indices: the smallest index decides
    std::vector<int32_t> big = ids;
    big[7] = (int32_t)S + 4;
    CHECK(call(big.data(), nanx.data(), K, lo.data(), hi.data(), n.data()) == GK_E_ARG, "NaN then bad id accepted");
    CHECK(strstr(gk_last_error(), "xs[5]") != nullptr, "NaN first: %s", gk_last_error());
    big[2] = (int32_t)S;
    CHECK(call(big.data(), nanx.data(), K, lo.data(), hi.data(), n.data()) == GK_E_ARG, "bad id then NaN accepted");
    CHECK(strstr(gk_last_error(), "ids[2]") != nullptr, "bad id first: %s", gk_last_error());
    // both at one index: the id is reported
    big = ids;
    big[5] = (int32_t)S;
    CHECK(call(big.data(), nanx.data(), K, lo.data(), hi.data(), n.data()) == GK_E_ARG, "bad id with NaN accepted");
    CHECK(strstr(gk_last_error(), "ids[5]") != nullptr && strstr(gk_last_error(), "xs[") == nullptr,
          "same index: the id wins: %s", gk_last_error());
  }
  // the empty call: GK_OK, nothing touched (arrays may be NULL)
  CHECK(call(nullptr, nullptr, 0, lo.data(), nullptr, nullptr) == GK_OK, "count 0 refused");
  CHECK(same_state(state_of(z.eng, S), s0), "a refused or empty call changed the set");
  for (int64_t k = 0; k < K; ++k)
    CHECK(lo[k] == -7 && hi[k] == -7 && n[k] == -7, "a refused or empty call wrote an output");
}

static void run() {
  const double eps = 0.01;
  const std::vector<int64_t> lens = {0, 1, 50, 99, 100, 101, 150, 202, 1000, 1500, 190, 150, 150, 57, 1313, 0, 707, 303};
  Sets z;
  if (!make(z, eps, lens, 31)) return;
  refusals(z);
  // an all-negative batch touches no stream; one sample
  {
    const State s0 = state_of(z.eng, z.S);
    query(z, {-1, INT32_MIN, -7}, {kNaN, 1.0, kNaN}, 7, "all negative");
    CHECK(same_state(state_of(z.eng, z.S), s0), "an all-negative batch changed the set");
  }
  query(z, {9}, {0.5}, 7, "one sample");
  random_batch(z, 300, 7, "batch");
  random_batch(z, 64, 1, "lo only");
  random_batch(z, 65, 2, "hi only");
  random_batch(z, 63, 4, "n only");
  for (int round = 0; round < 4; ++round) {
    std::vector<int64_t> more(z.S);
    for (auto& m : more) m = (int64_t)(z.rng() % 260);
    feed(z, more);
    compare_all(z, "continued");
    random_batch(z, 500 + 37 * round, 3 + 4 * (round & 1), "round");
  }
  {
    const State s1 = state_of(z.eng, z.S);
    random_batch(z, 200, 7, "again");
    random_batch(z, 200, 7, "again");
    (void)s1;
  }
  // other eps: the period-1 set (eps > 1) and a fine one
  for (double e : {2.0, 0.001}) {
    Sets y;
    if (!make(y, e, {0, 3, 700, 1, 2500, 64}, 37)) return;
    random_batch(y, 257, 7, "other eps");
    feed(y, std::vector<int64_t>(y.S, 129));
    random_batch(y, 129, 7, "other eps, continued");
    drop(y);
  }
  drop(z);
}

int main() {
  run();
  return selftest_result("cpu_rankkeyed_selftest");
}
