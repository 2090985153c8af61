// cpu_rollup_selftest.cpp -- TEST INFRASTRUCTURE: gk_rollup of the host engine
// (sketches-py_amd/cpu/gk_cpu.cpp, through include/gk_capi.h + gk_cpu.h)
// against the C oracle (oracle/gk_oracle.c: one one-stream set per source and
// destination stream, gko_merge in member order) on the shapes of the mixed
// roll-up case of tests/rollup_cases.py: a 17-member group, groups of 0, 1, 2
// and 5, empty members first, only empty members, non-members with pending
// values; a fresh and a pre-ingested destination; then the argument errors.
// Built with ASan + UBSan by `make -C sketches-py_amd/cpu sanitize-rollup`;
// tests/test_cpu_rollup.py runs it.
#include "cpu_selftest_util.h"

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
  Sets src, dst;
  if (!make(src, eps, lens, 11) || !make(dst, eps, dlens, 12)) return;
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
  return selftest_result("cpu_rollup_selftest");
}
