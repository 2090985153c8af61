// gk_compact.hip -- k_compact_plan / k_compact_move: the kernels of gk_compact,
// "every stream into the smallest capacity class that holds its table"
// (gfx950, wave64).  DESIGN.md section 5, "k_compact".
//
// Both kernels walk the S streams in groups of 64, one stream per lane, so that
// cls[] and E[] are read coalesced, and decide each stream's placement with the
// same rule (compact_target): a stream of class c whose table has E entries
// goes to t = min(c, fit(E)), fit(E) the smallest class with E <= cap - 1
// (unpack_target's rule, gk_ops.hip).  Nothing is mutated between the two, so
// the move finds exactly the streams the plan counted.
//
// The host (gk_capi.cpp gk_compact) runs the move once per destination class,
// ascending, into an arena of its own: old and new arenas are different
// allocations, no copy overlaps its source, and the old arena of a class is
// freed only after every stream that lived in it has been moved.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "gk_launch.h"

// The class a stream of class c with a table of E entries is compacted into:
// never above c (compaction does not promote).
__device__ __forceinline__ int compact_target(const GKState& st, int c, int E) {
  int t = 0;
  while (t < c && E > st.cap[t] - 1) ++t;
  return t;
}

// k_compact_plan: per class k > 0, into ctl (GK_CMP_WORDS zeroed words):
//   ctl[GK_CMP_FINAL + k]   streams whose class after the compaction is k
//   ctl[GK_CMP_LEAVE + k]   streams of class k that move down (the demoted)
//   ctl[GK_CMP_ARRIVE + k]  streams that move down INTO class k
// One atomic per wave and counter (ballot + popcount), not one per stream: a
// million streams meet in the same few words.  Mutates no stream state.
__global__ __launch_bounds__(256) void k_compact_plan(GKState st, int32_t* __restrict__ ctl) {
  const int lane = threadIdx.x & 63;
  const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int64_t nw = ((int64_t)gridDim.x * blockDim.x) >> 6;
  for (int64_t base = wave * 64; base < st.S; base += nw * 64) {  // (wave-uniform: every lane ballots)
    const int64_t s = base + lane;
    const bool live = s < st.S;
    const int c = live ? st.cls[s] : 0;
    const int t = live ? compact_target(st, c, st.E[s]) : 0;
    for (int k = 1; k < st.nclass; ++k) {
      const int fin = __popcll(__ballot(live && t == k));
      const int out = __popcll(__ballot(live && c == k && t != k));
      const int in = __popcll(__ballot(live && t == k && c != k));
      if (lane == 0) {
        if (fin) atomicAdd(&ctl[GK_CMP_FINAL + k], fin);
        if (out) atomicAdd(&ctl[GK_CMP_LEAVE + k], out);
        if (in) atomicAdd(&ctl[GK_CMP_ARRIVE + k], in);
      }
    }
  }
}

// k_compact_move: every stream above class 0 whose class after the compaction
// is t -- the ones that stay in t as well as the ones that come down into it --
// moves its table to its new place: its class-0 home tab[0] + s * cap[0]
// (t == 0), or a fresh slot of the new arena ntab of nalloc slots (t > 0).
//  * One atomic per group of 64 streams takes the group's slots from
//    ctl[GK_CMP_TAKEN + t]; the streams are appended to the rebuilt member list
//    nlist at their slot, so the list is dense and holds each member once.
//  * The whole wave copies one stream after the other, 16 bytes per lane and
//    access (a GKRec is one int4): 1 KiB per wave instruction, coalesced.
//  * A wave barrier follows the copy, then lane 0 writes cls and slot.
// st holds the OLD arenas.  A slot beyond nalloc (the host sized the arena from
// the plan: never) is not written; the stream stays put and is counted in
// ctl[GK_CMP_STUCK].
__global__ __launch_bounds__(256) void k_compact_move(GKState st, int t, GKRec* __restrict__ ntab, int32_t nalloc,
                                                      int32_t* __restrict__ nlist, int32_t* __restrict__ ctl) {
  const int lane = threadIdx.x & 63;
  const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int64_t nw = ((int64_t)gridDim.x * blockDim.x) >> 6;
  for (int64_t base = wave * 64; base < st.S; base += nw * 64) {
    const int64_t s = base + lane;
    const bool live = s < st.S;
    const int c = live ? st.cls[s] : 0;
    const int E = live ? st.E[s] : 0;
    const int32_t old = live ? st.slot[s] : 0;
    unsigned long long todo = __ballot(live && c > 0 && compact_target(st, c, E) == t);
    if (!todo) continue;  // (the whole wave)
    int32_t slot0 = 0;
    if (t > 0) {
      if (lane == 0) slot0 = atomicAdd(&ctl[GK_CMP_TAKEN + t], __popcll(todo));
      slot0 = __shfl(slot0, 0, 64);
    }
    for (int k = 0; todo; ++k) {
      const int l = __ffsll((long long)todo) - 1;
      todo &= todo - 1;
      const int cc = __shfl(c, l, 64);
      const int32_t oslot = __shfl(old, l, 64);
      const int64_t ss = base + l;
      const int32_t slot = slot0 + k;
      if (t > 0 && slot >= nalloc) {
        if (lane == 0) atomicAdd(&ctl[GK_CMP_STUCK], 1);
        continue;
      }
      const int4* __restrict__ src = (const int4*)(st.tab[cc] + (int64_t)oslot * st.cap[cc]);
      int4* __restrict__ dst =
          (int4*)(t == 0 ? st.tab[0] + ss * (int64_t)st.cap[0] : ntab + (int64_t)slot * st.cap[t]);
      const int n = min(min(__shfl(E, l, 64), st.cap[cc]), st.cap[t]);
      for (int j = lane; j < n; j += 64) dst[j] = src[j];
      __builtin_amdgcn_wave_barrier();
      if (lane == 0) {
        if (t > 0) nlist[slot] = (int32_t)ss;
        st.slot[ss] = t > 0 ? slot : 0;
        st.cls[ss] = t;
      }
    }
  }
}

// one lane per stream in groups of 64; at most 16 blocks of 4 waves per CU
static unsigned compact_grid(int64_t S) {
  const int64_t groups = (S + 63) / 64;
  return (unsigned)std::max<int64_t>(1, std::min<int64_t>((groups + 3) / 4, (int64_t)gk_num_cu() * 16));
}

hipError_t gk_launch_compact_plan(const GKState& st, int32_t* ctl, hipStream_t stream) {
  if (st.S <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_compact_plan, dim3(compact_grid(st.S)), dim3(256), 0, stream, st, ctl);
  return hipGetLastError();
}

hipError_t gk_launch_compact_move(const GKState& st, int t, GKRec* ntab, int64_t nalloc, int32_t* nlist, int32_t* ctl,
                                  hipStream_t stream) {
  if (st.S <= 0) return hipSuccess;
  if (t < 0 || t >= st.nclass || (t > 0 && (!ntab || !nlist || nalloc <= 0 || nalloc > INT32_MAX)))
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_compact_move, dim3(compact_grid(st.S)), dim3(256), 0, stream, st, t, ntab, (int32_t)nalloc,
                     nlist, ctl);
  return hipGetLastError();
}
