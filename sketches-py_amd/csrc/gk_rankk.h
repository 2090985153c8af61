// gk_rankk.h -- what the walks of k_rank_keyed (gk_rankkeyed.hip) and
// k_rank_ingest_keyed (gk_rankingest.hip) share: the per-wave table tile, its
// load and the two searches.  Everything here is a constant or
// __forceinline__: no unit gets code of its own from it.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gk_dev.h"

namespace {

// Entries of a stream's table a wave holds in LDS at once: v, the exclusive
// prefix G of g (int64) and (g, d), 24 bytes per entry -- 6 KiB per wave, 24 KiB
// per workgroup of four waves, six workgroups (24 waves) per CU.  Tables at
// eps = 0.01 stay below it; a longer table is taken tile after tile.
constexpr int RKK_TILE = 256;
constexpr int RKK_WAVES = 4;

struct RkkTile {
  double v[RKK_TILE];
  int64_t G[RKK_TILE];
  int2 gd[RKK_TILE];
};

// the wave's LDS writes are ordered before its later LDS reads (and the other
// way round before a tile is overwritten): one wave, in-order LDS pipeline --
// this only keeps the compiler from moving accesses across
__device__ __forceinline__ void rkk_lds_order() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// Entries tab[0 .. len) (len <= RKK_TILE) into the wave's tile: coalesced
// 16-byte records, G[k] = carry + g_0 + .. + g_{k-1} by the wave scan, 64 entries
// per step.  Returns carry + the sum of g.  Every lane of the wave is active.
__device__ __forceinline__ int64_t rkk_load_tile(RkkTile& t, const GKRec* __restrict__ tab, int len, int64_t carry,
                                                 int lane) {
  for (int k0 = 0; k0 < len; k0 += 64) {
    const int k = k0 + lane;
    int4 w = make_int4(0, 0, 0, 0);
    if (k < len) w = *reinterpret_cast<const int4*>(tab + k);
    const int64_t g = (int64_t)w.z;
    const int64_t incl = wave_incl_scan_i64(g, lane);
    if (k < len) {
      t.v[k] = __hiloint2double(w.y, w.x);
      t.G[k] = carry + incl - g;
      t.gd[k] = make_int2(w.z, w.w);
    }
    carry += gk_readlane_i64(incl, 63);
  }
  return carry;
}

// #{k < len : v[k] <= x} of the ascending tile (IEEE comparison)
__device__ __forceinline__ int rkk_count_le(const RkkTile& t, int len, double x) {
  int lo = 0, hi = len;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (t.v[mid] <= x) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

// the largest s with goffs[s] <= pos, given goffs[0] <= pos < goffs[S]
__device__ __forceinline__ int64_t rkk_stream_at(const int64_t* __restrict__ goffs, int64_t S, int64_t pos) {
  int64_t lo = 0, hi = S;
  while (hi - lo > 1) {
    const int64_t mid = lo + ((hi - lo) >> 1);
    if (goffs[mid] <= pos) lo = mid;
    else hi = mid;
  }
  return lo;
}

}  // namespace
