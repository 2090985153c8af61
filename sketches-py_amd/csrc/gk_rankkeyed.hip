// gk_rankkeyed.hip -- k_rank_keyed*: rank bounds per (stream id, value) sample
// behind gk_ranks_keyed (gfx950, wave64).  DESIGN.md section 5, "k_rank_keyed".
//
// Kernels of one call, in stream order (host sequence: gk_capi.cpp):
//   k_rank_keyed_check  one thread per sample: id range (negative ids pass),
//                       NaN on live rows, the flush list through the bitmap,
//                       and the sample's index as the group-by's payload.
//                       Mutates no stream state.
//   (flush of the listed streams; k_group_* of gk_keyed.hip: the samples'
//    indices grouped by id, stable, with the CSR offsets of the S streams)
//   k_rank_keyed        one wave per `chunk` grouped samples: the wave walks
//                       the streams whose runs meet its chunk, holds a stream's
//                       table on chip and answers that stream's samples of
//                       the chunk, one lane per sample.
// The work is balanced by samples, not by streams: a stream with 10^7 samples is
// shared by 10^7 / chunk waves, a chunk of one-sample streams is one wave's
// work.  No wave waits on another; nothing is written but the outputs' rows.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "gk_launch.h"
#include "gk_rankk.h"

__global__ __launch_bounds__(256) void k_rank_keyed_check(GKState st, const int32_t* __restrict__ ids,
                                                          const double* __restrict__ xs, int64_t count,
                                                          int32_t* __restrict__ ctl, uint32_t* __restrict__ bitmap,
                                                          int32_t* __restrict__ list, double* __restrict__ payload) {
  const int64_t step = (int64_t)gridDim.x * blockDim.x;
  for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k < count; k += step) {
    const int64_t s = ids[k];
    payload[k] = __longlong_as_double((long long)k);
    if (s < 0) continue;  // "no stream": xs[k] is not examined
    bool bad = s >= st.S;
    if (!bad) {
      const double x = xs[k];
      bad = x != x;
    }
    if (bad) {
      atomicOr(&ctl[GK_SEL_BAD], 1);
      atomicMax(reinterpret_cast<uint32_t*>(&ctl[GK_SEL_FIRST]), (uint32_t)(count - k));
      continue;
    }
    if (st.n[s] <= 0 || st.pend[s] <= 0) continue;
    const uint32_t bit = 1u << (s & 31);
    // a plain look first: a hot stream's 10^7 samples would otherwise queue up
    // on one word (measured: 0.5 s of same-address atomics at Zipf(1.1)); a
    // stale zero only costs the atomic, whose answer decides
    if (__hip_atomic_load(&bitmap[s >> 5], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & bit) continue;
    if (!(atomicOr(&bitmap[s >> 5], bit) & bit)) list[atomicAdd(&ctl[GK_SEL_COUNT], 1)] = (int32_t)s;
  }
}

// Wave w of the grid takes the grouped samples [w * chunk, (w + 1) * chunk)
// below `kept` = goffs[S] -- gidx[p] is the sample index (int64, bit-cast) of
// grouped position p, goffs[s] .. goffs[s+1] the run of stream s -- and, of the
// caller's samples with the same positions, zeroes the rows of the negative
// ids (kept <= count: the grid covers both).  The call has flushed and
// synchronised: tables and n / _min / _max are final.  Per stream of the chunk:
//  * a table of at most RKK_TILE entries is loaded ONCE for all the stream's
//    samples of the chunk; then, 64 samples per step, lane l finds
//    i = #{v_k <= x} by binary search in LDS and applies the four rules of
//    gk_capi.h with G(i), g_i, d_i from LDS, summed in int64;
//  * a longer table is streamed tile after tile once per 64 samples, the
//    prefix carried from tile to tile: a lane is done at the first tile that
//    holds an entry > x (i, G(i), g_i, d_i are all in that tile), the pass ends
//    when every lane is done; a lane no tile stops has i = E, G(E) = the carry.
// Nothing past entry E-1 and no sample outside the run is read.
__global__ __launch_bounds__(RKK_WAVES * 64) void k_rank_keyed(GKState st, const int32_t* __restrict__ ids,
                                                               const double* __restrict__ xs, int64_t count,
                                                               const double* __restrict__ gidx,
                                                               const int64_t* __restrict__ goffs, int chunk,
                                                               int64_t* __restrict__ lo, int64_t* __restrict__ hi,
                                                               int64_t* __restrict__ nout) {
  __shared__ RkkTile tiles[RKK_WAVES];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  RkkTile& t = tiles[w];
  const int64_t c0 = ((int64_t)blockIdx.x * RKK_WAVES + w) * (int64_t)chunk;
  if (c0 >= count) return;  // (the whole wave)
  {
    const int64_t cend = min(c0 + chunk, count);
    for (int64_t i = c0 + lane; i < cend; i += 64) {
      if (ids[i] < 0) {
        if (lo) lo[i] = 0;
        if (hi) hi[i] = 0;
        if (nout) nout[i] = 0;
      }
    }
  }
  const int64_t kept = goffs[st.S];
  if (c0 >= kept) return;
  const int64_t cend = min(c0 + chunk, kept);
  int64_t s = rkk_stream_at(goffs, st.S, c0);
  int64_t pos = c0;
  while (pos < cend) {
    // goffs[s] <= pos < goffs[s + 1]: samples [pos, run_end) belong to stream s
    const int64_t run_end = min(goffs[s + 1], cend);
    const int64_t n = st.n[s];
    const int E = n != 0 ? st.E[s] : 0;
    const double mn = st.mn[s], mx = st.mx[s];
    const GKRec* tab = gk_table_ptr(st, s);
    const bool single = E <= RKK_TILE;
    int64_t total = 0;
    if (single && E > 0) {
      rkk_lds_order();  // (the last stream's reads of the tile)
      total = rkk_load_tile(t, tab, E, 0, lane);
      rkk_lds_order();
    }
    for (int64_t b = pos; b < run_end; b += 64) {
      const int64_t p = b + lane;
      const bool act = p < run_end;
      int64_t idx = 0;
      double x = 0.0;
      if (act) {
        idx = (int64_t)__double_as_longlong(gidx[p]);
        x = xs[idx];
      }
      // i < E: Gi = G(i), gd = (g_i, d_i); else Gi = G(E)
      bool below = false;
      int64_t Gi = 0;
      int2 gd = make_int2(0, 0);
      if (single) {
        const int c = act ? rkk_count_le(t, E, x) : 0;
        below = c < E;
        Gi = total;
        if (below) {
          Gi = t.G[c];
          gd = t.gd[c];
        }
      } else {
        int64_t carry = 0;
        bool open = act;  // no entry > x seen yet
        for (int k0 = 0; k0 < E; k0 += RKK_TILE) {
          const int len = min(RKK_TILE, E - k0);
          rkk_lds_order();
          carry = rkk_load_tile(t, tab + k0, len, carry, lane);
          rkk_lds_order();
          if (open) {
            const int c = rkk_count_le(t, len, x);
            if (c < len) {
              open = false;
              below = true;
              Gi = t.G[c];
              gd = t.gd[c];
            }
          }
          if (__ballot(open) == 0) break;  // (wave-uniform)
        }
        if (open) Gi = carry;
      }
      if (act) {
        int64_t l, h;
        if (n == 0 || x < mn) {
          l = 0;
          h = 0;
        } else if (x >= mx) {
          l = n;
          h = n;
        } else {
          l = Gi > 1 ? Gi : 1;
          const int64_t up = below ? Gi + (int64_t)gd.x + (int64_t)gd.y - 1 : n;
          h = up < n - 1 ? up : n - 1;
        }
        if (lo) lo[idx] = l;
        if (hi) hi[idx] = h;
        if (nout) nout[idx] = n;
      }
    }
    pos = run_end;
    if (pos >= cend) break;
    // the next stream with samples: usually s + 1
    ++s;
    if (goffs[s + 1] <= pos) s = rkk_stream_at(goffs, st.S, pos);
  }
}

hipError_t gk_launch_rank_keyed_check(const GKState& st, const int32_t* ids, const double* xs, int64_t count,
                                      int32_t* ctl, uint32_t* bitmap, int32_t* list, double* payload,
                                      hipStream_t stream) {
  if (count <= 0) return hipSuccess;
  const unsigned grid = (unsigned)std::min<int64_t>((count + 255) / 256, 65536);
  hipLaunchKernelGGL(k_rank_keyed_check, dim3(grid), dim3(256), 0, stream, st, ids, xs, count, ctl, bitmap, list,
                     payload);
  return hipGetLastError();
}

hipError_t gk_launch_rank_keyed(const GKState& st, const int32_t* ids, const double* xs, int64_t count,
                                const double* gidx, const int64_t* goffs, int chunk, int64_t* lo, int64_t* hi,
                                int64_t* n, hipStream_t stream) {
  if (count <= 0 || (!lo && !hi && !n)) return hipSuccess;
  if (chunk < 64 || chunk % 64) return hipErrorInvalidValue;
  const int64_t waves = (count + chunk - 1) / chunk;
  hipLaunchKernelGGL(k_rank_keyed, dim3((unsigned)((waves + RKK_WAVES - 1) / RKK_WAVES)), dim3(RKK_WAVES * 64), 0,
                     stream, st, ids, xs, count, gidx, goffs, chunk, lo, hi, n);
  return hipGetLastError();
}
