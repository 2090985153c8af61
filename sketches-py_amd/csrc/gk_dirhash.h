// gk_dirhash.h -- what the two engines' key directories (gk_dir_*) share: the
// table geometry, the key hash and the GK_DIR_HASH_BITS switch.  Included by
// gk_dir.hip / gk_capi.cpp (device engine) and ../cpu/gk_cpu.cpp (host engine).
// None of it is part of the ABI: ids never depend on the hash (gk_capi.h).
#pragma once

#include <stdint.h>
#include <stdlib.h>

#ifdef __HIPCC__
#define GK_DIR_HD __host__ __device__ __forceinline__
#else
#define GK_DIR_HD inline
#endif

#define GK_DIR_MAX_CAPACITY ((int64_t)1 << 30)
#define GK_DIR_MIN_SLOTS 64

// Slots of a directory of `capacity` keys: the power of two >= 2 * capacity,
// at least 64 (load factor <= 1/2 when full).
inline int64_t gk_dir_slots(int64_t capacity) {
  int64_t T = GK_DIR_MIN_SLOTS;
  while (T < 2 * capacity) T <<= 1;
  return T;
}

// The key hash: the finaliser of splitmix64 (Steele, Lea, Flood 2014), a
// fixed bijective 64-bit mixer.
GK_DIR_HD uint64_t gk_dir_mix(uint64_t x) {
  x ^= x >> 30;
  x *= 0xbf58476d1ce4e5b9ull;
  x ^= x >> 27;
  x *= 0x94d049bb133111ebull;
  x ^= x >> 31;
  return x;
}

// Home slots: home = base + (hash & mask).  By default base = 0 and mask =
// T - 1.  GK_DIR_HASH_BITS=b (tests) confines them to the LAST 2^b slots, base
// = T - 2^b, mask = 2^b - 1: with b = 0 every key starts at slot T - 1 and the
// table is one probe chain that wraps round its end.
struct GKDirHome {
  uint32_t base;
  uint32_t mask;
};

GK_DIR_HD uint32_t gk_dir_home(const GKDirHome& hm, uint64_t hash) { return hm.base + ((uint32_t)hash & hm.mask); }

// false: GK_DIR_HASH_BITS is set and is not a number >= 0 (b >= log2 T: the whole table)
inline bool gk_dir_home_from_env(int64_t T, GKDirHome* hm) {
  hm->base = 0;
  hm->mask = (uint32_t)(T - 1);
  const char* e = getenv("GK_DIR_HASH_BITS");
  if (!e || !*e) return true;
  char* end = nullptr;
  const long b = strtol(e, &end, 10);
  if (end == e || *end || b < 0) return false;
  if (b < 62 && ((int64_t)1 << b) < T) {
    hm->mask = (uint32_t)(((int64_t)1 << b) - 1);
    hm->base = (uint32_t)(T - ((int64_t)1 << b));
  }
  return true;
}
