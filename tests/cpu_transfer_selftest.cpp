// cpu_transfer_selftest.cpp -- TEST INFRASTRUCTURE: gk_pack_select_bytes,
// gk_pack_select and gk_unpack_select of the host engine
// (sketches-py_amd/cpu/gk_cpu.cpp, through include/gk_capi.h + gk_cpu.h)
// against the C oracle (oracle/gk_oracle.c: one one-stream set per stream).
// Random workloads: streams are packed out of one set and unpacked into
// another, the oracle streams change owner the same way (the source streams
// are reset, so every oracle still belongs to exactly one engine stream),
// both sets go on ingesting and every stream of both is compared bit for bit
// after every step.  Then the refusals (nothing mutated), pack_select of
// every stream against gk_pack byte for byte, and a fold of a packed subset.
// Built with ASan + UBSan by `make -C sketches-py_amd/cpu sanitize-transfer`;
// tests/test_cpu_transfer.py runs it.
#include <algorithm>
#include <numeric>

#include "cpu_selftest_util.h"
#include "gk_pack.h"

static std::vector<unsigned char> pack_of(gk_set* set, const std::vector<int32_t>& ids, int64_t slack = 0) {
  int64_t bytes = -1;
  std::vector<unsigned char> buf;
  if (gk_pack_select_bytes(set, ids.data(), (int64_t)ids.size(), &bytes, nullptr) != GK_OK || bytes < 0) {
    ++failures;
    return buf;
  }
  buf.assign((size_t)(bytes + slack), 0xAB);
  if (gk_pack_select(set, ids.data(), (int64_t)ids.size(), buf.data(), bytes + slack, nullptr) != GK_OK) ++failures;
  for (int64_t k = bytes; k < bytes + slack; ++k)
    if (buf[(size_t)k] != 0xAB) ++failures;  // bytes past the packed size stay untouched
  return buf;
}

// `cnt` distinct streams of a set of S, in random order
static std::vector<int32_t> pick(std::mt19937_64& rng, int64_t S, int64_t cnt) {
  std::vector<int32_t> all((size_t)S);
  std::iota(all.begin(), all.end(), 0);
  std::shuffle(all.begin(), all.end(), rng);
  all.resize((size_t)cnt);
  return all;
}

static void moves() {
  const double eps = 0.01;
  Sets a, b;
  if (!make(a, eps, {0, 1, 50, 99, 100, 101, 150, 202, 1000, 1500, 190, 150, 57, 1313, 707}, 31)) return;
  if (!make(b, eps, {303, 0, 640, 101, 5, 1000, 250, 99, 1212, 57, 0}, 32)) return;
  std::mt19937_64 rng(33);
  for (int round = 0; round < 8; ++round) {
    Sets& src = (round & 1) ? b : a;
    Sets& dst = (round & 1) ? a : b;
    const int64_t cnt = 1 + (int64_t)(rng() % 5);
    const std::vector<int32_t> from = pick(rng, src.S, cnt), to = pick(rng, dst.S, cnt);
    const State before = state_of(src.eng, src.S);
    const std::vector<unsigned char> buf = pack_of(src.eng, from, 64);
    CHECK(same_state(state_of(src.eng, src.S), before), "round %d: pack_select changed the source", round);
    CHECK(gk_unpack_select(dst.eng, to.data(), cnt, buf.data(), nullptr) == GK_OK, "round %d: unpack failed: %s", round,
          gk_last_error());
    CHECK(gk_reset_select(src.eng, from.data(), cnt, nullptr) == GK_OK, "round %d: reset failed", round);
    for (int64_t k = 0; k < cnt; ++k) {
      gko_destroy(dst.orc[to[k]]);
      dst.orc[to[k]] = src.orc[from[k]];
      src.orc[from[k]] = gko_create(1, eps);
    }
    compare_all(a, "after a move (a)");
    compare_all(b, "after a move (b)");
    if (failures) return;
    std::vector<int64_t> la(a.S), lb(b.S);
    for (auto& x : la) x = (int64_t)(rng() % 260);
    for (auto& x : lb) x = (int64_t)(rng() % 260);
    feed(a, la);
    feed(b, lb);
    compare_all(a, "continued (a)");
    compare_all(b, "continued (b)");
    if (failures) return;
  }
  // pack_select of every stream in order is gk_pack, byte for byte
  {
    std::vector<int32_t> all((size_t)a.S);
    std::iota(all.begin(), all.end(), 0);
    int64_t bytes = 0;
    CHECK(gk_pack_bytes(a.eng, &bytes, nullptr) == GK_OK, "pack_bytes failed");
    std::vector<unsigned char> whole((size_t)bytes, 0), sel((size_t)bytes, 0);
    CHECK(gk_pack(a.eng, whole.data(), bytes, nullptr) == GK_OK, "pack failed");
    int64_t sb = 0;
    CHECK(gk_pack_select_bytes(a.eng, all.data(), a.S, &sb, nullptr) == GK_OK && sb == bytes, "pack_select_bytes");
    CHECK(gk_pack_select(a.eng, all.data(), a.S, sel.data(), bytes, nullptr) == GK_OK, "pack_select failed");
    CHECK(whole == sel, "pack_select(all ids) differs from gk_pack");
  }
  // a packed subset with a repeated id folds into a set holding those streams
  {
    const std::vector<int32_t> ids = {3, 0, 3, 7};
    const std::vector<unsigned char> buf = pack_of(a.eng, ids);
    gk_set* t = nullptr;
    CHECK(gk_create(4, eps, 0, -1, &t) == GK_OK, "create failed");
    const void* bufs[1] = {buf.data()};
    CHECK(gk_fold_packed(t, bufs, 1, nullptr) == GK_OK, "fold of a packed subset failed: %s", gk_last_error());
    const State st = state_of(t, 4);
    for (int64_t k = 0; k < 4; ++k) compare_stream(st, 4, k, a.orc[ids[k]], "take");
    gk_destroy(t);
  }
  drop(a);
  drop(b);
}

template <typename T>
static std::vector<unsigned char> patched(std::vector<unsigned char> buf, size_t off, T value) {
  memcpy(buf.data() + off, &value, sizeof(T));
  return buf;
}

static void refusals() {
  const double eps = 0.01;
  Sets z;
  if (!make(z, eps, {150, 99, 1000, 0, 202, 57, 101, 640}, 41)) return;
  const int64_t S = z.S;
  const std::vector<int32_t> ids = {0, 2, 4};
  const std::vector<unsigned char> good = pack_of(z.eng, ids);
  gkpack::Header hd;
  memcpy(&hd, good.data(), sizeof(hd));
  CHECK(hd.magic == gkpack::kMagic && hd.version == 1 && hd.S == 3 && hd.bytes == (int64_t)good.size(), "header");
  const gkpack::Layout L = gkpack::layout(hd.S, hd.E, hd.P);
  const int64_t* eo = gkpack::at<int64_t>((const void*)good.data(), L.eoffs);
  const int64_t* n = gkpack::at<int64_t>((const void*)good.data(), L.n);
  CHECK(eo[1] > 0 && n[0] == 150, "unexpected packed sizes");
  const State s0 = state_of(z.eng, S);
  const std::vector<int32_t> to = {5, 1, 7}, hi = {5, (int32_t)S, 7}, neg = {-1, 1, 7}, dup = {5, 1, 5};
  int64_t bytes = 0;
  std::vector<unsigned char> small(good.size() - 1, 0);
  CHECK(gk_pack_select_bytes(z.eng, hi.data(), 3, &bytes, nullptr) == GK_E_ARG, "bytes: id == S accepted");
  CHECK(strstr(gk_last_error(), "ids[1]") != nullptr, "bytes: message without the first bad index: %s", gk_last_error());
  CHECK(gk_pack_select(z.eng, neg.data(), 3, small.data(), (int64_t)small.size(), nullptr) == GK_E_ARG,
        "pack: id == -1 accepted");
  CHECK(gk_pack_select(z.eng, nullptr, 3, small.data(), (int64_t)small.size(), nullptr) == GK_E_ARG, "pack: null ids");
  CHECK(gk_pack_select(z.eng, ids.data(), -1, small.data(), (int64_t)small.size(), nullptr) == GK_E_ARG, "pack: count -1");
  CHECK(gk_pack_select(z.eng, ids.data(), 3, small.data(), (int64_t)small.size(), nullptr) == GK_E_ARG,
        "pack: a short buffer accepted");
  CHECK(strstr(gk_last_error(), std::to_string(good.size()).c_str()) != nullptr, "pack: message without the size: %s",
        gk_last_error());
  CHECK(gk_unpack_select(z.eng, hi.data(), 3, good.data(), nullptr) == GK_E_ARG, "unpack: id == S accepted");
  CHECK(strstr(gk_last_error(), "ids[1]") != nullptr, "unpack: message without the first bad index");
  CHECK(gk_unpack_select(z.eng, neg.data(), 3, good.data(), nullptr) == GK_E_ARG, "unpack: id == -1 accepted");
  CHECK(gk_unpack_select(z.eng, dup.data(), 3, good.data(), nullptr) == GK_E_ARG, "unpack: a duplicate id accepted");
  CHECK(gk_unpack_select(z.eng, to.data(), 2, good.data(), nullptr) == GK_E_ARG, "unpack: S != count accepted");
  CHECK(gk_unpack_select(z.eng, to.data(), 3, nullptr, nullptr) == GK_E_ARG, "unpack: null buffer accepted");
  CHECK(gk_unpack_select(z.eng, to.data(), 3, patched<unsigned char>(good, 3, 0).data(), nullptr) == GK_E_FORMAT,
        "unpack: a flipped magic byte accepted");
  CHECK(gk_unpack_select(z.eng, to.data(), 3, patched<uint32_t>(good, 8, 2).data(), nullptr) == GK_E_FORMAT,
        "unpack: version 2 accepted");
  CHECK(gk_unpack_select(z.eng, to.data(), 3, patched<int64_t>(good, 48, hd.bytes + 256).data(), nullptr) == GK_E_FORMAT,
        "unpack: a wrong byte count accepted");
  CHECK(gk_unpack_select(z.eng, to.data(), 3, patched<int64_t>(good, L.eoffs + 8, eo[2] + 1).data(), nullptr) ==
            GK_E_FORMAT, "unpack: a decreasing offset accepted");
  CHECK(gk_unpack_select(z.eng, to.data(), 3, patched<double>(good, 16, 0.02).data(), nullptr) == GK_E_EPS_MISMATCH,
        "unpack: another eps accepted");
  CHECK(gk_unpack_select(z.eng, to.data(), 3, patched<int64_t>(good, L.n, n[0] - 1).data(), nullptr) == GK_E_ARG,
        "unpack: pending beyond n mod P accepted");
  CHECK(gk_unpack_select(z.eng, to.data(), 3, patched<int64_t>(good, L.n + 8, -5).data(), nullptr) == GK_E_ARG,
        "unpack: n < 0 accepted");
  // count == 0: a packed state of zero streams, validated on the way in
  const std::vector<unsigned char> none = pack_of(z.eng, {});
  CHECK(none.size() == gkpack::layout(0, 0, 0).total, "count 0: size");
  CHECK(gk_unpack_select(z.eng, nullptr, 0, none.data(), nullptr) == GK_OK, "unpack: count 0 refused: %s", gk_last_error());
  CHECK(gk_unpack_select(z.eng, nullptr, 0, good.data(), nullptr) == GK_E_ARG, "unpack: count 0 with S == 3 accepted");
  CHECK(same_state(state_of(z.eng, S), s0), "a refused or empty call changed the set");
  compare_all(z, "after the refusals");
  drop(z);
}

int main() {
  moves();
  refusals();
  return selftest_result("cpu_transfer_selftest");
}
