// gk_rankingest.hip -- k_rank_ingest_keyed: the rank kernel of
// gk_rank_ingest_keyed, "rank each sample against its stream, then add it"
// (gfx950, wave64).  DESIGN.md section 5, "k_rank_ingest_keyed".
//
// The call runs k_rank_keyed_check, the flush of the listed streams and ONE
// group-by of the samples' indices, as gk_ranks_keyed does (gk_rankkeyed.hip),
// then this kernel in k_rank_keyed's place: the same walk, in which every lane
// also stores the value it has loaded for its sample at the sample's grouped
// position.  The stable group-by gives ascending sample index within a
// stream's run -- arrival order -- so (gvals, goffs) is the CSR batch the
// ingest takes, and the second group-by of the two-call spelling, with the
// value as its payload, is not run.
//
// The walk is k_rank_keyed's, statement for statement, over the helpers of
// gk_rankk.h.  It is a second copy on purpose: k_rank_keyed keeps the machine
// code it was measured with (one walk shared through a template moved its
// register allocation).  A change to the rank rules goes into both.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gk_launch.h"
#include "gk_rankk.h"

// Wave w of the grid takes the grouped samples [w * chunk, (w + 1) * chunk)
// below `kept` = goffs[S], as in k_rank_keyed: gidx[p] is the sample index of
// grouped position p, the rows of negative ids are zeroed, a stream's table is
// held in the wave's tile (a longer one streamed tile after tile) and lane l
// answers one sample.  In addition gvals[p] = xs[gidx[p]] for every p < kept,
// the double copied bit for bit (-0.0, infinities, denormals); gvals is none of
// the other buffers.  With lo, hi and nout all NULL that copy is all a wave
// does: no stream is looked up and no table loaded.
__global__ __launch_bounds__(RKK_WAVES * 64) void k_rank_ingest_keyed(
    GKState st, const int32_t* __restrict__ ids, const double* __restrict__ xs, int64_t count,
    const double* __restrict__ gidx, const int64_t* __restrict__ goffs, int chunk, int64_t* __restrict__ lo,
    int64_t* __restrict__ hi, int64_t* __restrict__ nout, double* __restrict__ gvals) {
  __shared__ RkkTile tiles[RKK_WAVES];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  RkkTile& t = tiles[w];
  const int64_t c0 = ((int64_t)blockIdx.x * RKK_WAVES + w) * (int64_t)chunk;
  if (c0 >= count) return;  // (the whole wave)
  const int64_t kept = goffs[st.S];
  if (!lo && !hi && !nout) {
    const int64_t cend = min(c0 + chunk, kept);
    for (int64_t p = c0 + lane; p < cend; p += 64) gvals[p] = xs[(int64_t)__double_as_longlong(gidx[p])];
    return;
  }
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
        gvals[p] = x;  // the grouped batch of the ingest
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

hipError_t gk_launch_rank_ingest_keyed(const GKState& st, const int32_t* ids, const double* xs, int64_t count,
                                       const double* gidx, const int64_t* goffs, int chunk, int64_t* lo, int64_t* hi,
                                       int64_t* n, double* gvals, hipStream_t stream) {
  if (count <= 0) return hipSuccess;
  if (chunk < 64 || chunk % 64) return hipErrorInvalidValue;
  const int64_t waves = (count + chunk - 1) / chunk;
  hipLaunchKernelGGL(k_rank_ingest_keyed, dim3((unsigned)((waves + RKK_WAVES - 1) / RKK_WAVES)),
                     dim3(RKK_WAVES * 64), 0, stream, st, ids, xs, count, gidx, goffs, chunk, lo, hi, n, gvals);
  return hipGetLastError();
}
