// gk_dev.h -- the device-side helpers that both gk_kernels.hip and gk_ops.hip
// (or gk_query.h, which both include) use: the query markers, the per-stream
// count limit, the wave64 DPP scans, GK_STATS_LONG.  A helper with one
// consumer stays in its unit.  Everything here is a macro or __forceinline__:
// no unit gets code of its own from it.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>

#include "gk_state.h"

// quantile answers that are the stream's _min / _max while the stats role of
// the launch may still be writing them (the join, k_query_list, replaces them)
#define GK_QMARK_MIN 0x7ff4000000000001LL  // quantile = _min of the stream (gk:182-183, 220)
#define GK_QMARK_MAX 0x7ff4000000000002LL  // quantile = _max of the stream (gk:229)

// Largest T handled in int32 fields: T = floor(2 eps (n-1)) <= 2^30, i.e.
// n <= 2^29/eps values in ONE stream (5.4e10 at eps = 0.01).  No result is
// ever computed with a clamped T: the ingest kernels check the stream's count
// after the call first (gk_count_ok) and refuse a stream that would pass it
// (overflow -> promotion -> the unbounded class reports it, GK_E_OVERFLOW).
#define GK_T_CLAMP (1 << 30)

// T of every flush up to count `n_final` fits GK_T_CLAMP
__device__ __forceinline__ bool gk_count_ok(const GKState& st, int64_t n_final) {
  return st.two_eps * (double)(n_final - 1) < (double)GK_T_CLAMP + 1.0;
}

// ---------------------------------------------------------------------------
// wave helpers (wave64)
// ---------------------------------------------------------------------------
// DPP controls (GFX9 family, gfx950 included)
#define DPP_ROW_SHR(n) (0x110 + (n))
#define DPP_ROW_BCAST15 0x142
#define DPP_ROW_BCAST31 0x143

// Inclusive wave64 prefix sum in 12 VALU ops: Hillis-Steele inside each row
// of 16 lanes, then the row_bcast15/31 carries across rows.  Lanes whose DPP
// source is outside the row (or rows masked off) receive 0.
__device__ __forceinline__ uint32_t wave_incl_scan_u32(uint32_t v, int /*lane*/) {
  v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, DPP_ROW_SHR(1), 0xf, 0xf, false);
  v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, DPP_ROW_SHR(2), 0xf, 0xf, false);
  v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, DPP_ROW_SHR(4), 0xf, 0xf, false);
  v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, DPP_ROW_SHR(8), 0xf, 0xf, false);
  v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, DPP_ROW_BCAST15, 0xa, 0xf, false);
  v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, DPP_ROW_BCAST31, 0xc, 0xf, false);
  return v;
}

// 64-bit DPP move: both halves through the same control; lanes whose
// source is masked off or outside the row receive `old`
template <int CTRL, int ROWMASK>
__device__ __forceinline__ int64_t dpp64(int64_t v, int64_t old) {
  const int lo = __builtin_amdgcn_update_dpp((int)(uint32_t)(uint64_t)old, (int)(uint32_t)(uint64_t)v, CTRL,
                                             ROWMASK, 0xf, false);
  const int hi = __builtin_amdgcn_update_dpp((int)(uint32_t)((uint64_t)old >> 32),
                                             (int)(uint32_t)((uint64_t)v >> 32), CTRL, ROWMASK, 0xf, false);
  return (int64_t)(((uint64_t)(uint32_t)hi << 32) | (uint32_t)lo);
}

// inclusive wave64 prefix sum / running max of int64 on DPP (no LDS-pipe
// instruction: the flush's table traffic bounds the LDS)
__device__ __forceinline__ int64_t wave_incl_scan_i64(int64_t v, int /*lane*/) {
  v += dpp64<DPP_ROW_SHR(1), 0xf>(v, 0);
  v += dpp64<DPP_ROW_SHR(2), 0xf>(v, 0);
  v += dpp64<DPP_ROW_SHR(4), 0xf>(v, 0);
  v += dpp64<DPP_ROW_SHR(8), 0xf>(v, 0);
  v += dpp64<DPP_ROW_BCAST15, 0xa>(v, 0);
  v += dpp64<DPP_ROW_BCAST31, 0xc>(v, 0);
  return v;
}

__device__ __forceinline__ int64_t wave_incl_max_i64(int64_t v, int /*lane*/) {
  v = max(v, dpp64<DPP_ROW_SHR(1), 0xf>(v, INT64_MIN));
  v = max(v, dpp64<DPP_ROW_SHR(2), 0xf>(v, INT64_MIN));
  v = max(v, dpp64<DPP_ROW_SHR(4), 0xf>(v, INT64_MIN));
  v = max(v, dpp64<DPP_ROW_SHR(8), 0xf>(v, INT64_MIN));
  v = max(v, dpp64<DPP_ROW_BCAST15, 0xa>(v, INT64_MIN));
  v = max(v, dpp64<DPP_ROW_BCAST31, 0xc>(v, INT64_MIN));
  return v;
}

// lane l's int64 in every lane (two v_readlane; l wave-uniform)
__device__ __forceinline__ int64_t gk_readlane_i64(int64_t v, int l) {
  const int lo = __builtin_amdgcn_readlane((int)(uint32_t)(uint64_t)v, l);
  const int hi = __builtin_amdgcn_readlane((int)(uint32_t)((uint64_t)v >> 32), l);
  return (int64_t)(((uint64_t)(uint32_t)hi << 32) | (uint32_t)lo);
}

__device__ __forceinline__ int wave_sum_i32(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// Streams up to GK_STATS_LONG values have their gk:52-59 chains walked by the
// stats role of the small-class launch (P <= 128) or by k_stats_short;
// longer ones by k_stats_long, beside the ingest.
#ifndef GK_STATS_LONG
#define GK_STATS_LONG 16384  // longer streams go to k_stats_long (64 per wave, on a second HIP stream)
#endif

