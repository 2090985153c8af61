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
  return selftest_result("cpu_rank_selftest");
}
