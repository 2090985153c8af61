// cpu_compact_selftest.cpp -- TEST INFRASTRUCTURE: gk_compact and
// gk_class_usage of the host engine (sketches-py_amd/cpu/gk_cpu.cpp, through
// include/gk_capi.h + gk_cpu.h) against the C oracle (oracle/gk_oracle.c: one
// one-stream set per stream).  Random sequences of ingest / reset_select /
// compact: a compaction changes no bit of any stream (state before == state
// after == the oracles'), demotes nothing, never reports more capacity than
// before, and the streams go on exactly as the oracles do.  Then the arguments.
// Built with ASan + UBSan by `make -C sketches-py_amd/cpu sanitize-compact`;
// tests/test_cpu_compact.py runs it.
#include <algorithm>
#include <numeric>

#include "cpu_selftest_util.h"

static int64_t arena_of(gk_set* set) {
  int64_t streams = -1, used = -1, alloc = -1, arena = -1, ws = -1;
  if (gk_class_usage(set, 0, &streams, &used, &alloc, &arena, &ws, nullptr) != GK_OK) ++failures;
  const int64_t S = gk_num_streams(set);
  if (streams != S || used != S || alloc != S || ws != 0 || arena < 0) ++failures;
  return arena;
}

static void sequences(uint64_t seed) {
  const double eps = 0.01;
  Sets z;
  if (!make(z, eps, {0, 1, 50, 99, 100, 101, 150, 202, 1000, 1500, 190, 150, 57, 1313, 707, 0, 640}, seed)) return;
  std::mt19937_64 rng(seed * 7 + 1);
  int compactions = 0;
  for (int step = 0; step < 60; ++step) {
    const int op = (int)(rng() % 4);
    if (op == 0 || op == 1) {
      std::vector<int64_t> lens(z.S);
      for (auto& x : lens) x = (rng() % 3) ? (int64_t)(rng() % 260) : 0;
      feed(z, lens);
    } else if (op == 2) {
      std::vector<int32_t> all((size_t)z.S);
      std::iota(all.begin(), all.end(), 0);
      std::shuffle(all.begin(), all.end(), rng);
      const int64_t cnt = 1 + (int64_t)(rng() % 6);
      CHECK(gk_reset_select(z.eng, all.data(), cnt, nullptr) == GK_OK, "step %d: reset failed", step);
      for (int64_t k = 0; k < cnt; ++k) {
        gko_destroy(z.orc[all[k]]);
        z.orc[all[k]] = gko_create(1, eps);
      }
    } else {
      const State before = state_of(z.eng, z.S);
      const int64_t a0 = arena_of(z.eng);
      int64_t demoted = -1, freed = -1;
      CHECK(gk_compact(z.eng, &demoted, &freed, nullptr) == GK_OK, "step %d: compact failed: %s", step, gk_last_error());
      const int64_t a1 = arena_of(z.eng);
      CHECK(demoted == 0, "step %d: the host engine demoted %lld stream(s)", step, (long long)demoted);
      CHECK(freed >= 0 && freed == a0 - a1, "step %d: bytes_freed %lld, usage %lld -> %lld", step, (long long)freed,
            (long long)a0, (long long)a1);
      CHECK(same_state(state_of(z.eng, z.S), before), "step %d: compact changed a stream", step);
      // straight after one, a second compaction finds nothing
      CHECK(gk_compact(z.eng, &demoted, &freed, nullptr) == GK_OK && demoted == 0 && freed == 0,
            "step %d: a second compact freed %lld bytes", step, (long long)freed);
      ++compactions;
    }
    compare_all(z, "sequence");
    if (failures) return;
  }
  CHECK(compactions > 0, "seed %llu drew no compaction", (unsigned long long)seed);
  drop(z);
}

static void arguments() {
  Sets z;
  if (!make(z, 0.01, {150, 0, 1000}, 5)) return;
  int64_t x = 0;
  CHECK(gk_class_usage(z.eng, 1, &x, nullptr, nullptr, nullptr, nullptr, nullptr) == GK_E_ARG, "cls 1 accepted");
  CHECK(gk_class_usage(z.eng, -1, &x, nullptr, nullptr, nullptr, nullptr, nullptr) == GK_E_ARG, "cls -1 accepted");
  CHECK(gk_class_usage(z.eng, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == GK_OK, "NULL outputs refused");
  CHECK(gk_class_usage(nullptr, 0, &x, nullptr, nullptr, nullptr, nullptr, nullptr) == GK_E_ARG, "NULL set accepted");
  CHECK(gk_compact(nullptr, nullptr, nullptr, nullptr) == GK_E_ARG, "compact: NULL set accepted");
  CHECK(gk_compact(z.eng, nullptr, nullptr, nullptr) == GK_OK, "compact: NULL outputs refused");
  compare_all(z, "after the argument checks");
  drop(z);
  // no stream at all
  gk_set* none = nullptr;
  CHECK(gk_create(0, 0.01, 0, -1, &none) == GK_OK, "create of an empty set failed");
  int64_t demoted = -1, freed = -1;
  CHECK(gk_compact(none, &demoted, &freed, nullptr) == GK_OK && demoted == 0 && freed == 0, "S == 0: compact");
  CHECK(gk_class_usage(none, 0, &x, nullptr, nullptr, &freed, nullptr, nullptr) == GK_OK && x == 0 && freed == 0,
        "S == 0: class_usage");
  gk_destroy(none);
}

int main() {
  for (uint64_t seed : {51, 52, 53}) sequences(seed);
  arguments();
  return selftest_result("cpu_compact_selftest");
}
