// cpu_dirremove_selftest.cpp -- TEST INFRASTRUCTURE: key removal and id
// recycling (gk_dir_remove, gk_dir_bound, gk_dir_import_sparse, gk_dir_assign
// with free ids) of the host engine (sketches-py_amd/cpu/gk_cpu.cpp, through
// include/gk_capi.h) against a std::map plus a std::set of free ids that run
// the loops of gk_capi.h.  Random assign / remove / sparse-import sequences,
// void calls on a directory with holes, generations of keys through a table of
// 64 slots (the tombstone chains), and the whole again under
// GK_DIR_HASH_BITS=0 and =2.
// Built with ASan + UBSan by `make -C sketches-py_amd/cpu sanitize-dirremove`;
// tests/test_cpu_dir_remove.py runs it.
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <map>
#include <random>
#include <set>
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
  std::vector<int64_t> keys;  // keys[id], GK_DIR_NONE at free ids; keys.size() is bound
  std::set<int32_t> free;
  int64_t capacity = 0;

  // false: overflow (the model is left as it was)
  bool assign(const std::vector<int64_t>& ks, std::vector<int32_t>* out) {
    const Model before = *this;
    out->assign(ks.size(), -2);
    for (size_t i = 0; i < ks.size(); ++i) {
      if (ks[i] == GK_DIR_NONE) {
        (*out)[i] = -1;
        continue;
      }
      auto it = d.find(ks[i]);
      if (it == d.end()) {
        int32_t id;
        if (!free.empty()) {
          id = *free.begin();
          free.erase(free.begin());
          keys[(size_t)id] = ks[i];
        } else if ((int64_t)keys.size() < capacity) {
          id = (int32_t)keys.size();
          keys.push_back(ks[i]);
        } else {
          *this = before;
          return false;
        }
        it = d.emplace(ks[i], id).first;
      }
      (*out)[i] = it->second;
    }
    return true;
  }
  void remove(const std::vector<int64_t>& ks, std::vector<int32_t>* out) {
    out->assign(ks.size(), -2);
    for (size_t i = 0; i < ks.size(); ++i) {
      auto it = ks[i] == GK_DIR_NONE ? d.end() : d.find(ks[i]);
      if (it == d.end()) {
        (*out)[i] = -1;
        continue;
      }
      (*out)[i] = it->second;
      keys[(size_t)it->second] = GK_DIR_NONE;
      free.insert(it->second);
      d.erase(it);
    }
  }
  void import_sparse(const std::vector<int64_t>& ks) {
    d.clear();
    free.clear();
    keys = ks;
    for (size_t i = 0; i < ks.size(); ++i) {
      if (ks[i] == GK_DIR_NONE) free.insert((int32_t)i);
      else d[ks[i]] = (int32_t)i;
    }
  }
};

// directory and model answer alike: size, bound, keys, lookups of every id's key and of strangers
static void same(gk_dir* dir, const Model& m, const char* what) {
  CHECK(gk_dir_size(dir) == (int64_t)m.d.size(), "%s: size %lld vs %zu", what, (long long)gk_dir_size(dir), m.d.size());
  CHECK(gk_dir_bound(dir) == (int64_t)m.keys.size(), "%s: bound %lld vs %zu", what, (long long)gk_dir_bound(dir),
        m.keys.size());
  CHECK(m.d.size() + m.free.size() == m.keys.size(), "%s: the model lost an id", what);
  std::vector<int64_t> ks(m.keys.size() + 1, 0);
  CHECK(gk_dir_keys(dir, ks.data(), nullptr) == GK_OK, "%s: keys failed: %s", what, gk_last_error());
  ks.resize(m.keys.size());
  CHECK(ks == m.keys, "%s: keys differ", what);
  std::vector<int64_t> probe = m.keys;  // (GK_DIR_NONE at free ids answers -1)
  for (int64_t j = 0; j < 40; ++j) probe.push_back(INT64_MAX - 1000 - j);  // (never drawn below)
  std::vector<int32_t> got(probe.size(), -7);
  CHECK(gk_dir_lookup(dir, probe.data(), (int64_t)probe.size(), got.data(), nullptr) == GK_OK, "%s: lookup failed", what);
  for (size_t i = 0; i < probe.size(); ++i) {
    const int32_t exp = i < m.keys.size() && m.keys[i] != GK_DIR_NONE ? (int32_t)i : -1;
    if (got[i] != exp) {
      CHECK(false, "%s: lookup[%zu] = %d, expected %d", what, i, got[i], exp);
      break;
    }
  }
}

static std::vector<int64_t> batch(std::mt19937_64& rng, int64_t pool, int64_t most) {
  std::vector<int64_t> ks((size_t)(rng() % (uint64_t)(most + 1)));
  const uint64_t lo = rng() % (uint64_t)pool, width = 1 + rng() % (uint64_t)pool;
  for (auto& k : ks) {
    const uint64_t r = (lo + rng() % width) % (uint64_t)(pool + 2);
    // a multiplicative spread of the pool, both signs; now and then "no key"
    k = r == 0 ? GK_DIR_NONE : (int64_t)(r * 0x9E3779B97F4A7C15ull) >> (r & 7);
    if (k >= INT64_MAX - 10000) k = 1;  // (the strangers of same() and of the void calls)
  }
  return ks;
}

static void check_assign(gk_dir* dir, Model& m, const std::vector<int64_t>& ks, int step, bool must_fit = false) {
  const int64_t count = (int64_t)ks.size();
  std::vector<int32_t> exp, got((size_t)count + 1, -9);
  const size_t before = m.d.size();
  const bool fits = m.assign(ks, &exp);
  int64_t num_new = -5;
  const int rc = gk_dir_assign(dir, count ? ks.data() : nullptr, count, count ? got.data() : nullptr, &num_new, nullptr);
  CHECK(fits || !must_fit, "step %d: the model refuses a batch that must fit", step);
  if (fits) {
    CHECK(rc == GK_OK, "step %d: assign failed: %s", step, gk_last_error());
    got.resize((size_t)count);
    CHECK(got == exp, "step %d: assigned ids differ", step);
    CHECK(num_new == (int64_t)(m.d.size() - before), "step %d: num_new %lld", step, (long long)num_new);
  } else {
    CHECK(rc == GK_E_OVERFLOW, "step %d: expected GK_E_OVERFLOW, got %d", step, rc);
  }
  same(dir, m, "after an assign");
}

static void check_remove(gk_dir* dir, Model& m, const std::vector<int64_t>& ks, int step) {
  const int64_t count = (int64_t)ks.size();
  std::vector<int32_t> exp, got((size_t)count + 1, -9);
  const size_t before = m.d.size();
  m.remove(ks, &exp);
  int64_t gone = -5;
  const int rc = gk_dir_remove(dir, count ? ks.data() : nullptr, count, count ? got.data() : nullptr, &gone, nullptr);
  CHECK(rc == GK_OK, "step %d: remove failed: %s", step, gk_last_error());
  got.resize((size_t)count);
  CHECK(got == exp, "step %d: removed ids differ", step);
  CHECK(gone == (int64_t)(before - m.d.size()), "step %d: num_removed %lld", step, (long long)gone);
  same(dir, m, "after a remove");
}

static void random_sequence(int64_t capacity, uint64_t seed, int64_t pool) {
  gk_dir* dir = nullptr;
  if (gk_dir_create(capacity, 0, &dir) != GK_OK) {
    CHECK(false, "create(%lld) failed: %s", (long long)capacity, gk_last_error());
    return;
  }
  Model m;
  m.capacity = capacity;
  std::mt19937_64 rng(seed);
  for (int step = 0; step < 120; ++step) {
    switch (rng() % 6) {
      case 0:
      case 1:
        check_assign(dir, m, batch(rng, pool, 300), step);
        break;
      case 2:
      case 3:
        check_remove(dir, m, batch(rng, pool, 300), step);
        break;
      case 4: {  // more strangers than ids are left, after a few old keys: void, holes kept
        std::vector<int64_t> ks;
        for (const auto& kv : m.d) {
          if (ks.size() == 3) break;
          ks.push_back(kv.first);
        }
        const int64_t left = capacity - (int64_t)m.d.size();
        for (int64_t j = 0; j <= left; ++j) ks.push_back(INT64_MAX - 3000 - j);
        const Model before = m;
        check_assign(dir, m, ks, step);
        CHECK(m.keys == before.keys && m.free == before.free, "step %d: the model took a void call", step);
        break;
      }
      default: {  // its own keys() through the sparse import, into a second directory and back
        gk_dir* other = nullptr;
        CHECK(gk_dir_create(capacity, 0, &other) == GK_OK, "create other");
        if (!other) break;
        CHECK(gk_dir_import_sparse(other, m.keys.data(), (int64_t)m.keys.size(), nullptr) == GK_OK, "sparse import: %s",
              gk_last_error());
        same(other, m, "sparse copy");
        if (m.keys.size() >= 2 && m.keys[0] != GK_DIR_NONE) {
          std::vector<int64_t> bad = m.keys;
          bad.back() = bad[0];
          CHECK(gk_dir_import_sparse(other, bad.data(), (int64_t)bad.size(), nullptr) == GK_E_ARG,
                "sparse import of a repeated key accepted");
          same(other, m, "after a refused sparse import");
        }
        if (!m.free.empty()) {
          CHECK(gk_dir_import(other, m.keys.data(), (int64_t)m.keys.size(), nullptr) == GK_E_ARG,
                "dense import of GK_DIR_NONE accepted");
          same(other, m, "after a refused dense import");
        }
        gk_dir_destroy(dir);
        dir = other;
        break;
      }
    }
  }
  std::vector<int64_t> many((size_t)capacity + 1, GK_DIR_NONE);
  CHECK(gk_dir_import_sparse(dir, many.data(), capacity + 1, nullptr) == GK_E_ARG, "sparse import beyond capacity accepted");
  same(dir, m, "after a refused sparse import (count)");
  many.resize((size_t)capacity);
  CHECK(gk_dir_import_sparse(dir, many.data(), capacity, nullptr) == GK_OK, "sparse import of free ids only");
  m.import_sparse(many);
  same(dir, m, "free ids only");
  check_assign(dir, m, batch(rng, pool, 300), 1000);
  gk_dir_destroy(dir);
}

// capacity 32, 64 slots: whole generations (step 32) or half ones (step 16) come and go
static void chains(int64_t step) {
  gk_dir* dir = nullptr;
  CHECK(gk_dir_create(32, 0, &dir) == GK_OK, "create");
  if (!dir) return;
  Model m;
  m.capacity = 32;
  std::vector<int64_t> ks;
  for (int64_t j = 0; j < 32; ++j) ks.push_back(j * 0x9E3779B97F4A7C15ll);
  check_assign(dir, m, ks, -1, true);
  for (int round = 0; round < 10; ++round) {
    std::vector<int64_t> out, in;
    for (int64_t j = 0; j < step; ++j) {
      out.push_back((round * step + j) * 0x9E3779B97F4A7C15ll);
      in.push_back((round * step + 32 + j) * 0x9E3779B97F4A7C15ll);
    }
    check_remove(dir, m, out, round);
    check_assign(dir, m, in, round, true);
    CHECK(gk_dir_size(dir) == 32 && gk_dir_bound(dir) == 32, "round %d: size %lld bound %lld", round,
          (long long)gk_dir_size(dir), (long long)gk_dir_bound(dir));
  }
  gk_dir_destroy(dir);
}

static void arguments() {
  gk_dir* dir = nullptr;
  CHECK(gk_dir_create(4, 0, &dir) == GK_OK, "create");
  if (!dir) return;
  int64_t k = 1, gone = -5;
  int32_t id = 0;
  CHECK(gk_dir_bound(nullptr) == -1 && gk_dir_bound(dir) == 0, "bound");
  CHECK(gk_dir_remove(dir, &k, -1, &id, nullptr, nullptr) == GK_E_ARG, "negative count");
  CHECK(gk_dir_remove(dir, &k, (int64_t)1 << 31, &id, nullptr, nullptr) == GK_E_ARG, "count 2^31");
  CHECK(gk_dir_remove(dir, nullptr, 1, &id, nullptr, nullptr) == GK_E_ARG, "null keys");
  CHECK(gk_dir_remove(dir, &k, 1, nullptr, nullptr, nullptr) == GK_E_ARG, "null out_ids");
  CHECK(gk_dir_remove(nullptr, &k, 1, &id, nullptr, nullptr) == GK_E_ARG, "null directory");
  CHECK(gk_dir_import_sparse(dir, nullptr, 1, nullptr) == GK_E_ARG, "sparse import: null keys");
  CHECK(gk_dir_import_sparse(nullptr, &k, 1, nullptr) == GK_E_ARG, "sparse import: null directory");
  CHECK(gk_dir_remove(dir, nullptr, 0, nullptr, &gone, nullptr) == GK_OK && gone == 0, "empty batch");
  CHECK(gk_dir_remove(dir, &k, 1, &id, &gone, nullptr) == GK_OK && gone == 0 && id == -1, "a stranger");
  CHECK(gk_dir_assign(dir, &k, 1, &id, nullptr, nullptr) == GK_OK && id == 0, "assign");
  CHECK(gk_dir_remove(dir, &k, 1, &id, nullptr, nullptr) == GK_OK && id == 0, "remove without num_removed");
  CHECK(gk_dir_size(dir) == 0 && gk_dir_bound(dir) == 1, "size 0, bound 1");
  CHECK(gk_dir_import_sparse(dir, nullptr, 0, nullptr) == GK_OK && gk_dir_bound(dir) == 0, "sparse import of nothing");
  gk_dir_destroy(dir);
}

int main() {
  arguments();
  const char* bits[] = {nullptr, "0", "2"};
  for (const char* b : bits) {
    if (b) setenv("GK_DIR_HASH_BITS", b, 1);
    else unsetenv("GK_DIR_HASH_BITS");
    random_sequence(1, 1, 4);
    random_sequence(32, 2, 90);     // three times the capacity: full most of the time
    random_sequence(32, 3, 20);     // never fills
    random_sequence(700, 4, 2100);
    random_sequence(4096, 5, 600);  // many repeats
    chains(32);
    chains(16);
  }
  if (failures) {
    fprintf(stderr, "cpu_dirremove_selftest: %d failure(s)\n", failures);
    return 1;
  }
  printf("cpu_dirremove_selftest: ok\n");
  return 0;
}
