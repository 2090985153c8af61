// cpu_dir_selftest.cpp -- TEST INFRASTRUCTURE: the key directory (gk_dir_*) of
// the host engine (sketches-py_amd/cpu/gk_cpu.cpp, through include/gk_capi.h)
// against a std::map that runs the loop of gk_capi.h.  Random batches (many
// repeats, GK_DIR_NONE entries), a void overflow, the refusals of
// gk_dir_import (nothing mutated) and the whole again under
// GK_DIR_HASH_BITS=0 and =2 (one probe chain that wraps round the table end).
// Built with ASan + UBSan by `make -C sketches-py_amd/cpu sanitize-dir`;
// tests/test_cpu_dir.py runs it.
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <map>
#include <random>
#include <vector>

#include "gk_capi.h"

static int failures = 0;
#define CHECK(cond, ...)                \
  do {                                  \
    if (!(cond)) {                      \
      ++failures;                       \
      fprintf(stderr, "FAIL: ");        \
      fprintf(stderr, __VA_ARGS__);     \
      fprintf(stderr, "\n");            \
    }                                   \
  } while (0)

struct Model {
  std::map<int64_t, int32_t> d;
  std::vector<int64_t> keys;
  int64_t capacity;
  // false: overflow (the model is left as it was)
  bool assign(const std::vector<int64_t>& ks, std::vector<int32_t>* out) {
    const std::map<int64_t, int32_t> d0 = d;
    const std::vector<int64_t> k0 = keys;
    out->assign(ks.size(), -2);
    for (size_t i = 0; i < ks.size(); ++i) {
      if (ks[i] == GK_DIR_NONE) {
        (*out)[i] = -1;
        continue;
      }
      auto it = d.find(ks[i]);
      if (it == d.end()) {
        if ((int64_t)keys.size() == capacity) {
          d = d0;
          keys = k0;
          return false;
        }
        it = d.emplace(ks[i], (int32_t)keys.size()).first;
        keys.push_back(ks[i]);
      }
      (*out)[i] = it->second;
    }
    return true;
  }
};

// directory and model answer alike: size, keys, lookups of every key and of strangers
static void same(gk_dir* dir, const Model& m, const char* what) {
  CHECK(gk_dir_size(dir) == (int64_t)m.keys.size(), "%s: size %lld vs %zu", what, (long long)gk_dir_size(dir),
        m.keys.size());
  std::vector<int64_t> ks(m.keys.size() + 1, 0);
  CHECK(gk_dir_keys(dir, ks.data(), nullptr) == GK_OK, "%s: keys failed: %s", what, gk_last_error());
  ks.resize(m.keys.size());
  CHECK(ks == m.keys, "%s: keys differ", what);
  std::vector<int64_t> probe = m.keys;
  for (int64_t j = 0; j < 40; ++j) probe.push_back(INT64_MAX - 1000 - j);  // (never drawn below)
  probe.push_back(GK_DIR_NONE);
  std::vector<int32_t> got(probe.size(), -7);
  CHECK(gk_dir_lookup(dir, probe.data(), (int64_t)probe.size(), got.data(), nullptr) == GK_OK, "%s: lookup failed", what);
  for (size_t i = 0; i < probe.size(); ++i) {
    const int32_t exp = i < m.keys.size() ? (int32_t)i : -1;
    if (got[i] != exp) {
      CHECK(false, "%s: lookup[%zu] = %d, expected %d", what, i, got[i], exp);
      break;
    }
  }
}

static void random_batches(int64_t capacity, uint64_t seed, int64_t pool) {
  gk_dir* dir = nullptr;
  if (gk_dir_create(capacity, 0, &dir) != GK_OK) {
    CHECK(false, "create(%lld) failed: %s", (long long)capacity, gk_last_error());
    return;
  }
  CHECK(gk_dir_capacity(dir) == capacity, "capacity");
  Model m;
  m.capacity = capacity;
  std::mt19937_64 rng(seed);
  for (int round = 0; round < 30; ++round) {
    const int64_t count = (int64_t)(rng() % 300);
    std::vector<int64_t> ks((size_t)count);
    for (auto& k : ks) {
      const uint64_t r = rng() % (uint64_t)(pool + 3);
      // a multiplicative spread of the pool, both signs; now and then "no key"
      k = r == 0 ? GK_DIR_NONE : (int64_t)(r * 0x9E3779B97F4A7C15ull) >> (r & 7);
      if (k >= INT64_MAX - 2000) k = 1;
    }
    std::vector<int32_t> exp, got((size_t)count + 1, -9);
    const bool fits = m.assign(ks, &exp);
    int64_t num_new = -5;
    const int64_t before = gk_dir_size(dir);
    const int rc = gk_dir_assign(dir, count ? ks.data() : nullptr, count, count ? got.data() : nullptr, &num_new, nullptr);
    if (fits) {
      CHECK(rc == GK_OK, "round %d: assign failed: %s", round, gk_last_error());
      got.resize((size_t)count);
      CHECK(got == exp, "round %d: ids differ", round);
      CHECK(num_new == (int64_t)m.keys.size() - before, "round %d: num_new %lld", round, (long long)num_new);
    } else {
      CHECK(rc == GK_E_OVERFLOW, "round %d: expected GK_E_OVERFLOW, got %d", round, rc);
    }
    same(dir, m, "after a batch");
  }
  // a batch of known keys on whatever the directory holds now succeeds
  if (!m.keys.empty()) {
    std::vector<int32_t> got(m.keys.size(), -9);
    int64_t num_new = -5;
    CHECK(gk_dir_assign(dir, m.keys.data(), (int64_t)m.keys.size(), got.data(), &num_new, nullptr) == GK_OK && num_new == 0,
          "known keys: %s", gk_last_error());
    for (size_t i = 0; i < got.size(); ++i)
      if (got[i] != (int32_t)i) {
        CHECK(false, "known keys: id[%zu] = %d", i, got[i]);
        break;
      }
  }
  // import refusals leave the contents alone
  {
    std::vector<int64_t> bad = {5, 6, 7, 6, 5};
    if (capacity >= 5) {
      CHECK(gk_dir_import(dir, bad.data(), 5, nullptr) == GK_E_ARG, "import of a repeated key accepted");
      same(dir, m, "after a refused import (repeat)");
    }
    bad = {5, GK_DIR_NONE};
    if (capacity >= 2) {
      CHECK(gk_dir_import(dir, bad.data(), 2, nullptr) == GK_E_ARG, "import of GK_DIR_NONE accepted");
      same(dir, m, "after a refused import (none)");
    }
    std::vector<int64_t> many((size_t)capacity + 1);
    for (size_t i = 0; i < many.size(); ++i) many[i] = (int64_t)i;
    CHECK(gk_dir_import(dir, many.data(), capacity + 1, nullptr) == GK_E_ARG, "import beyond capacity accepted");
    same(dir, m, "after a refused import (count)");
  }
  // round trip into a second directory, and a reversed import
  {
    gk_dir* other = nullptr;
    CHECK(gk_dir_create(capacity, 0, &other) == GK_OK, "create other");
    if (other) {
      CHECK(gk_dir_import(other, m.keys.data(), (int64_t)m.keys.size(), nullptr) == GK_OK, "import: %s", gk_last_error());
      same(other, m, "imported copy");
      Model r;
      r.capacity = capacity;
      r.keys.assign(m.keys.rbegin(), m.keys.rend());
      for (size_t i = 0; i < r.keys.size(); ++i) r.d[r.keys[i]] = (int32_t)i;
      CHECK(gk_dir_import(other, r.keys.data(), (int64_t)r.keys.size(), nullptr) == GK_OK, "import reversed");
      same(other, r, "reversed import");
      CHECK(gk_dir_import(other, nullptr, 0, nullptr) == GK_OK, "import of nothing");
      CHECK(gk_dir_size(other) == 0, "import of nothing leaves keys");
      gk_dir_destroy(other);
    }
  }
  gk_dir_destroy(dir);
}

static void arguments() {
  gk_dir* dir = nullptr;
  CHECK(gk_dir_create(0, 0, &dir) == GK_E_ARG && !dir, "capacity 0");
  CHECK(gk_dir_create(((int64_t)1 << 30) + 1, 0, &dir) == GK_E_ARG && !dir, "capacity 2^30 + 1");
  CHECK(gk_dir_create(4, 0, nullptr) == GK_E_ARG, "null out");
  CHECK(gk_dir_create(4, 0, &dir) == GK_OK, "create");
  if (!dir) return;
  int64_t k = 1;
  int32_t id = 0;
  CHECK(gk_dir_assign(dir, &k, -1, &id, nullptr, nullptr) == GK_E_ARG, "negative count");
  CHECK(gk_dir_assign(dir, nullptr, 1, &id, nullptr, nullptr) == GK_E_ARG, "null keys");
  CHECK(gk_dir_assign(dir, &k, 1, nullptr, nullptr, nullptr) == GK_E_ARG, "null out_ids");
  CHECK(gk_dir_lookup(dir, nullptr, 1, &id, nullptr) == GK_E_ARG, "lookup: null keys");
  CHECK(gk_dir_import(dir, nullptr, 1, nullptr) == GK_E_ARG, "import: null keys");
  CHECK(gk_dir_assign(nullptr, &k, 1, &id, nullptr, nullptr) == GK_E_ARG, "null directory");
  CHECK(gk_dir_assign(dir, nullptr, 0, nullptr, nullptr, nullptr) == GK_OK, "empty batch");
  CHECK(gk_dir_keys(dir, nullptr, nullptr) == GK_OK, "keys of an empty directory");
  CHECK(gk_dir_size(dir) == 0, "size after refusals");
  gk_dir_destroy(dir);
  CHECK(gk_dir_destroy(nullptr) == GK_OK, "destroy(null)");
}

int main() {
  arguments();
  const char* bits[] = {nullptr, "0", "2"};
  for (const char* b : bits) {
    if (b) setenv("GK_DIR_HASH_BITS", b, 1);
    else unsetenv("GK_DIR_HASH_BITS");
    random_batches(1, 1, 4);
    random_batches(32, 2, 40);     // fills up: overflows, then known keys only
    random_batches(32, 3, 20);     // never fills
    random_batches(700, 4, 5000);  // mostly new keys until full
    random_batches(4096, 5, 600);  // many repeats
  }
  setenv("GK_DIR_HASH_BITS", "x", 1);
  gk_dir* dir = nullptr;
  CHECK(gk_dir_create(4, 0, &dir) == GK_E_ARG && !dir, "GK_DIR_HASH_BITS=x accepted");
  if (failures) {
    fprintf(stderr, "cpu_dir_selftest: %d failure(s)\n", failures);
    return 1;
  }
  printf("cpu_dir_selftest: ok\n");
  return 0;
}
