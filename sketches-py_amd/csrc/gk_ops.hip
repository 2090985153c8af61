// gk_ops.hip -- the operations on a set's committed state, batched GKArray
// engine (CDNA4, gfx950): everything that is not an ingest (the ingests and
// the long-stream machinery: gk_kernels.hip).  Shared device helpers:
// gk_dev.h, the table query: gk_query.h.
//
// Kernels
//   k_lengths / k_query_list  the two ends of an ingest call: the long-stream
//                           list + pre-call n; the join's answers (gk:156-232)
//                           for the listed streams and the _min/_max markers
//   k_fold       gk:111-154 wave per stream, per step (merge, roll-up member,
//                           merge_compress(entries)): convert `other`, stable merge of
//                           the incoming list, general four-rule walk (gk:76-106)
//   k_rollup_*   checks of a roll-up's group offsets and members, the flush list
//   k_select_*   gk:156-232, 45-46, 21-29  a list of stream ids: id check + flush
//                           list, wave per row query, reset, stats gather
//   k_rank       (no gk line: the reference has no rank())  wave per row: bounds on
//                           the count of values <= x from the flushed table
//   k_export* / k_import / k_check_pending / k_reset / k_rtab: state movement
//   k_pack_* / k_unpack_*   (gk:21-29, the whole state)  listed streams to and from a
//                           packed state: sizes + totals, wave per row gather; one
//                           checking pass, wave per row install (no flush)
//   k_promote / k_promote_dev  streams moved to the next capacity class
// Host: their launchers (gk_launch.h); the CU count comes from gk_num_cu()
// (gk_kernels.hip).  Timeline builds: gk_tl_call and gk_tl_call_read.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>

#include <algorithm>

#include "gk_dev.h"
#include "gk_launch.h"
#include "gk_query.h"

// The long-stream list (streams past GK_STATS_LONG values, for k_long_prep /
// k_stats_long) and the pre-call n snapshot st.n0 (read by the small-class
// launch's stats role while its ingest waves rewrite st.n): one stream per
// thread, no LDS (~6 us per 10^6 streams; as part of the former k_stats, whose 35 KiB
// chain tile holds it to 4 blocks per CU, it took 28 us).
#ifdef GK_TIMELINE
// timeline builds only: s_memrealtime when the call's first kernel starts
// (k_lengths) and when its join answers (k_query_list)
__device__ unsigned long long gk_tl_call[2];
#endif
__global__ __launch_bounds__(256) void k_lengths(GKState st, const int64_t* __restrict__ offs,
                                                 int32_t* __restrict__ long_list, int32_t* __restrict__ long_count) {
#ifdef GK_TIMELINE
  if (blockIdx.x == 0 && threadIdx.x == 0) gk_tl_call[0] = __builtin_amdgcn_s_memrealtime();
#endif
  const int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (s >= st.S) return;
  st.n0[s] = st.n[s];
  if (offs[s + 1] - offs[s] > GK_STATS_LONG) long_list[atomicAdd(long_count, 1)] = (int32_t)s;
}

// ===========================================================================
// Rank bounds of one stream from its flushed table (DESIGN.md section 5,
// "k_rank"; the reference has no rank()): for every threshold x the pair
//   n == 0 or x < _min : (0, 0)        x >= _max : (n, n)        otherwise
//   lo = max(G(i), 1),  hi = min(i < E ? G(i+1) + d_i - 1 : n, n - 1)
// with i = #{k : v_k <= x} and G(k) = g_0 + .. + g_{k-1}, all int64.
// The table is ascending, so the entries with v_k <= x ARE the first i: G(i)
// is the sum of g over them and G(i+1) + d_i - 1 = G(i) + g_i + d_i - 1.  Both
// i and G(i) are order-free sums over the table: lane l takes entries l,
// l + 64, ... (each wave access one coalesced run of records; no prefix scan)
// and ONE pass serves RK thresholds held in registers (thresholds beyond RK:
// one more pass per RK).  The lane that owns threshold u of the pass then
// loads entry i (only if i < E: nothing past entry E-1 is read) and stores
// the pair.  Comparisons are IEEE (-0.0 == 0.0, +-inf ordinary).  lo or hi
// may be NULL.  Every lane of the wave must be active (DPP reductions).
// ===========================================================================
#define GK_RANK_RK 8
template <int SV, int SI>
__device__ __forceinline__ void wave_ranks(const double* __restrict__ tv, const int32_t* __restrict__ tg,
                                                     const int32_t* __restrict__ td, int E, int64_t n, double mn,
                                                     double mx, const double* __restrict__ xs, int nx,
                                                     int64_t* __restrict__ lo, int64_t* __restrict__ hi, int lane) {
  for (int t0 = 0; t0 < nx; t0 += GK_RANK_RK) {
    const int nt = min(GK_RANK_RK, nx - t0);
    int my_i = 0;
    int64_t my_G = 0;
    if (n != 0) {
      double x[GK_RANK_RK];
      int cnt[GK_RANK_RK];
      int64_t gs[GK_RANK_RK];
#pragma unroll
      for (int u = 0; u < GK_RANK_RK; ++u) {
        x[u] = xs[t0 + min(u, nt - 1)];  // (wave-uniform; the tail repeats the last threshold)
        cnt[u] = 0;
        gs[u] = 0;
      }
#pragma unroll 4
      for (int j = lane; j < E; j += 64) {  // (long tables: four records per lane in flight)
        const double v = tv[(int64_t)j * SV];
        const int64_t g = tg[(int64_t)j * SI];
#pragma unroll
        for (int u = 0; u < GK_RANK_RK; ++u) {
          const bool le = v <= x[u];
          cnt[u] += le ? 1 : 0;
          gs[u] += le ? g : 0;
        }
      }
#pragma unroll
      for (int u = 0; u < GK_RANK_RK; ++u) {
        if (u < nt) {  // (wave-uniform)
          const int i = __builtin_amdgcn_readlane((int)wave_incl_scan_u32((uint32_t)cnt[u], lane), 63);
          const int64_t Gi = gk_readlane_i64(wave_incl_scan_i64(gs[u], lane), 63);
          if (lane == u) {
            my_i = i;
            my_G = Gi;
          }
        }
      }
    }
    if (lane < nt) {
      const double x = xs[t0 + lane];
      int64_t l, h;
      if (n == 0 || x < mn) {
        l = 0;
        h = 0;
      } else if (x >= mx) {
        l = n;
        h = n;
      } else {
        l = my_G > 1 ? my_G : 1;
        int64_t up = n;
        if (my_i < E) up = my_G + (int64_t)tg[(int64_t)my_i * SI] + (int64_t)td[(int64_t)my_i * SI] - 1;
        h = up < n - 1 ? up : n - 1;
      }
      if (lo) lo[t0 + lane] = l;
      if (hi) hi[t0 + lane] = h;
    }
  }
}

// k_query_list: quantiles (gk:156-232) of the listed streams from their
// committed tables in HBM, one wave per stream.  The fused ingest+query
// launch answers every stream before k_stats_long (running beside it) has
// produced the final _min/_max of the long streams (gk:183, 220, 229); this
// launch re-answers exactly those streams once it has joined.
// The join of a fused ingest + query (one wave per block):
//  * qfix (the small-class launch carried the stats role): an answer that is
//    _min or _max (gk:182-183, gk:229) was written as a marker NaN while the
//    stats role could still be writing them; now they are final.  One answer
//    per thread (the grid covers S*nq; no loop: every load in flight at once).
//  * the long streams (`list`), answered again from their final _min/_max
//    (k_stats_long ran beside the ingest), one per wave.  (A long stream
//    whose answer the qfix part also resolves gets the same bits from both.)
__global__ __launch_bounds__(256) void k_query_list(GKState st, const int32_t* __restrict__ list,
                                                    const int32_t* __restrict__ count,
                                                    const double* __restrict__ qs, int nq, int qmode,
                                                    double* __restrict__ qout, int qfix) {
  const int lane = threadIdx.x & 63;
#ifdef GK_TIMELINE
  if (blockIdx.x == 0 && threadIdx.x == 0) gk_tl_call[1] = __builtin_amdgcn_s_memrealtime();
#endif
  if (qfix) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < st.S * (int64_t)nq) {
      const long long b = __double_as_longlong(qout[i]);
      if (b == GK_QMARK_MIN || b == GK_QMARK_MAX) {
        const int64_t s = i / nq;
        qout[i] = b == GK_QMARK_MIN ? st.mn[s] : st.mx[s];
      }
    }
  }
  const int cnt = *count;
  const int wid = (int)(blockIdx.x * 4 + (threadIdx.x >> 6)), nwv = (int)(gridDim.x * 4);
  for (int w = wid; w < cnt; w += nwv) {
    const int64_t s = list[w];
    const GKRec* tab = gk_table_ptr(st, s);
    wave_quantiles<2, 4>(&tab->v, &tab->g, &tab->d, st.E[s], st.n[s], st.mn[s], st.mx[s], st, qs, nq, qmode,
                         qout + s * (int64_t)nq, lane);
  }
}

// ===========================================================================
// The merge steps of k_fold: GKArray.merge (gk:111-154) and
// merge_compress(entries), stream by stream.  The incoming list (self's raw
// pending values, then the converted records of `other` or the caller's
// records) is stably ordered by value and the four-rule walk of gk:76-106 runs
// wave-parallel over LDS: incoming records carry g > 1 here, so the add-path
// closed form does not apply; each lane re-walks its block of entries from its
// neighbour's carry until no carry-in changes (k_fold).
// `other` has already been flushed by the caller (gk:126, gk:137).
// ===========================================================================
struct MergeLDS {
  double *tv, *rv, *sp, *iv, *ov;
  int32_t *tg, *td, *rg, *rd, *ig, *id, *og, *od;
};

__device__ __forceinline__ MergeLDS merge_carve(unsigned char* smem, int cap, int pm) {
  const int MR = cap + 1, MI = cap + 1 + pm;
  MergeLDS m;
  double* dp = (double*)smem;
  m.tv = dp; dp += cap;
  m.rv = dp; dp += MR;
  m.sp = dp; dp += pm;
  m.iv = dp; dp += MI;
  m.ov = dp; dp += cap;
  int32_t* ip = (int32_t*)dp;
  m.tg = ip; ip += cap;
  m.td = ip; ip += cap;
  m.rg = ip; ip += MR;
  m.rd = ip; ip += MR;
  m.ig = ip; ip += MI;
  m.id = ip; ip += MI;
  m.og = ip; ip += cap;
  m.od = ip; ip += cap;
  return m;
}

__device__ __forceinline__ void flag_overflow(int32_t* cnt, int32_t* list, int64_t s, int lane) {
  if (lane == 0) {
    const int k = atomicAdd(cnt, 1);
    list[k] = (int32_t)s;
  }
}

#define GK_MERGE_RANK_MAX 256  // pending values ranked by comparison up to this many; bitonic above

// The steps of one merge.  All of them work on
// the arrays of a MergeLDS carve (LDS or a block's global workspace).

// gk:136-147: the converted records of a flushed `other` table into rv/rg/rd
//   (other._min, g0+d0-spread-1), (v_k, g_{k+1}+d_{k+1}-d_k),
//   (v_{L-1}, spread+1-d_{L-1}); only g > 0 is kept.  Returns their number
//   (at most oE + 1, which the caller has checked against the carve).
__device__ __forceinline__ int merge_convert(const MergeLDS& m, const GKRec* __restrict__ otab, int oE,
                                             int64_t spread, double omn, int lane) {
  const int ncand = oE + 1;
  int base = 0;
  for (int c0 = 0; c0 < ncand; c0 += 64) {
    const int c = c0 + lane;
    int64_t gv = 0;
    double vv = 0.0;
    if (c < ncand) {
      if (c == 0) {
        gv = (int64_t)otab[0].g + otab[0].d - spread - 1;
        vv = omn;
      } else if (c < oE) {
        gv = (int64_t)otab[c].g + otab[c].d - otab[c - 1].d;
        vv = otab[c - 1].v;
      } else {
        gv = spread + 1 - otab[oE - 1].d;
        vv = otab[oE - 1].v;
      }
    }
    const bool keep = (c < ncand) && gv > 0;
    const unsigned long long bal = __ballot(keep);
    const int before = __popcll(bal & ((1ull << lane) - 1ull));
    if (keep) {
      m.rv[base + before] = vv;
      m.rg[base + before] = (int32_t)gv;
      m.rd[base + before] = 0;
    }
    base += __popcll(bal);
  }
  // The list above is sorted by value while other._min <= v_0.  A table whose
  // first value lies below _min (explicit records below the minimum,
  // gk_merge_compress) leaves the first record out of place: the stable sort
  // of gk:72 moves it behind the records of smaller values, ahead of equal
  // ones.  Those form a prefix of records 1.. (the table is sorted).
  if (oE > 0 && omn > otab[0].v && (int64_t)otab[0].g + otab[0].d - spread - 1 > 0 && base > 1) {  // (wave-uniform)
    __syncthreads();
    int cnt = 0;
    for (int i0 = 1; i0 < base; i0 += 64) {
      const int i = i0 + lane;
      cnt += __popcll(__ballot(i < base && m.rv[i] < omn));
    }
    if (cnt > 0) {
      const int32_t g0 = m.rg[0];
      for (int i0 = 0; i0 < cnt; i0 += 64) {
        const int i = i0 + lane;
        double v1 = 0.0;
        int32_t g1 = 0;
        if (i < cnt) {
          v1 = m.rv[i + 1];
          g1 = m.rg[i + 1];
        }
        __syncthreads();
        if (i < cnt) {
          m.rv[i] = v1;
          m.rg[i] = g1;
        }
        __syncthreads();
      }
      if (lane == 0) {
        m.rv[cnt] = omn;
        m.rg[cnt] = g0;
      }
      __syncthreads();
    }
  }
  return base;
}

// stable order of self's raw pending values (gk:72) into sp; ov/og are scratch
__device__ __forceinline__ void merge_sort_pending(const MergeLDS& m, const double* __restrict__ pb, int p, int lane) {
  if (p <= GK_MERGE_RANK_MAX) {
    // few values: each lane ranks its values against all of them
    for (int i = lane; i < p; i += 64) m.ov[i] = pb[i];
    __syncthreads();
    for (int i = lane; i < p; i += 64) {
      const double x = m.ov[i];
      int rk = 0;
      for (int t = 0; t < p; ++t) {
        const double y = m.ov[t];
        rk += (y < x) || (y == x && t < i);
      }
      m.sp[rk] = x;
    }
  } else {
    // a large flush period (eps < 1/256): bitonic sort of (value, index)
    // in the output arrays (free here; cap >= pow2 above p for every class)
    int N = 1;
    while (N < p) N <<= 1;
    for (int i = lane; i < N; i += 64) {
      m.ov[i] = i < p ? pb[i] : __longlong_as_double(0x7ff0000000000000LL);
      m.og[i] = i < p ? i : INT32_MAX;
    }
    __syncthreads();
    for (int k = 2; k <= N; k <<= 1) {
      for (int j = k >> 1; j > 0; j >>= 1) {
        for (int pp = lane; pp < N / 2; pp += 64) {
          const int i = ((pp & ~(j - 1)) << 1) | (pp & (j - 1));
          const int l = i + j;
          const double a = m.ov[i], b = m.ov[l];
          const int ia = m.og[i], ib = m.og[l];
          const bool a_gt = (a > b) || (a == b && ia > ib);
          if (a_gt == ((i & k) == 0)) {
            m.ov[i] = b;
            m.ov[l] = a;
            m.og[i] = ib;
            m.og[l] = ia;
          }
        }
        __syncthreads();
      }
    }
    for (int i = lane; i < p; i += 64) m.sp[i] = m.ov[i];
  }
  __syncthreads();
}

// merged incoming list: `self.incoming + entries` sorted stably, so on equal
// values the raw pending values come first (gk:71-72); sp + rv/rg/rd -> iv/ig/id
__device__ __forceinline__ void merge_incoming(const MergeLDS& m, int p, int nrec, int lane) {
  for (int r = lane; r < p; r += 64) {
    const double x = m.sp[r];
    int lo = 0, hi = nrec;  // records strictly below x
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (m.rv[mid] < x) lo = mid + 1; else hi = mid;
    }
    m.iv[r + lo] = x;
    m.ig[r + lo] = 1;
    m.id[r + lo] = 0;
  }
  for (int t = lane; t < nrec; t += 64) {
    const double y = m.rv[t];
    int lo = 0, hi = p;  // pending values <= y
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (m.sp[mid] <= y) lo = mid + 1; else hi = mid;
    }
    m.iv[t + lo] = y;
    m.ig[t + lo] = m.rg[t];
    m.id[t + lo] = m.rd[t];
  }
}

// The four-rule walk of gk:76-106, wave-parallel: table tv/tg/td (E entries)
// and incoming iv/ig/id (M records) into ov/og/od; *sh_out = the number of
// output records, or -1 when they exceed outcap (nothing usable written).
// Incoming records (sorted) fall into gaps: record i precedes entry j iff
// iv[i] < tv[j] (gk:93), so gap j holds [a_{j-1}, a_j) with a_j = #{i :
// iv[i] < tv[j]}, and the tail [a_{E-1}, M) follows the last entry.  Entry
// j with carry-in c (the g of removed predecessors, gk:80/102) starts at
// G = g_j + c and walks its gap in order: record i is absorbed iff
// g_i + G + d_j <= T (G += g_i), else emitted as (v_i, g_i, G + d_j - g_i)
// (gk:94-99); the entry is then removed (carry G) iff j+1 < E and
// G + g_{j+1} + d_{j+1} <= T (gk:79/101), else emitted as (v_j, G, d_j).
// The tail chains records (gk:86-92).  Lane l owns entries [lK, lK+K); the
// carries are resolved by rounds (each lane re-walks its block from its
// left neighbour's last carry-out) until no carry-in changes -- lane 0's is
// fixed, so the fixpoint is the sequential walk.  Then counts, a wave scan
// and a second walk write the records in order.
__device__ __forceinline__ void merge_walk(const MergeLDS& m, int E, int M, int64_t T, int outcap, int lane,
                                           int* sh_out) {
  int32_t* ga = m.rg;  // a_j (records are in iv/ig/id by now)
  for (int j = lane; j < E; j += 64) {
    const double tvj = m.tv[j];
    int lo = 0, hi = M;
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (m.iv[mid] < tvj) lo = mid + 1; else hi = mid;
    }
    ga[j] = lo;
  }
  __syncthreads();
  const int K = (E + 63) >> 6;
  const int j0 = lane * K;
  const int jend = min(j0 + K, E);
  // walk of the lane's block from carry-in c; returns the carry-out and
  // the number of records it emits (out != NULL: also writes them)
  auto walk = [&](int64_t c, int& cnt_out, int obase, bool write) -> int64_t {
    int no_l = 0;
    for (int j = j0; j < jend; ++j) {
      int64_t G = (int64_t)m.tg[j] + c;
      const int64_t dj = m.td[j];
      const int ib = j == 0 ? 0 : ga[j - 1];
      const int ie = ga[j];
      for (int i = ib; i < ie; ++i) {
        const int64_t gi = m.ig[i];
        if (gi + G + dj <= T) {
          G += gi;
        } else {
          if (write) {
            m.ov[obase + no_l] = m.iv[i];
            m.og[obase + no_l] = (int32_t)gi;
            m.od[obase + no_l] = (int32_t)(G + dj - gi);
          }
          ++no_l;
        }
      }
      const bool rem = (j + 1 < E) && (G + m.tg[j + 1] + m.td[j + 1] <= T);
      if (rem) {
        c = G;
      } else {
        if (write) {
          m.ov[obase + no_l] = m.tv[j];
          m.og[obase + no_l] = (int32_t)G;
          m.od[obase + no_l] = (int32_t)dj;
        }
        ++no_l;
        c = 0;
      }
    }
    cnt_out = no_l;
    return c;
  };
  int64_t cin = 0;
  int cnt_blk = 0;
  for (int round = 0; round <= 64; ++round) {
    const int64_t cout = walk(cin, cnt_blk, 0, false);
    int64_t ncin = __shfl_up(cout, 1, 64);
    if (lane == 0) ncin = 0;
    if (__ballot(ncin != cin) == 0) break;
    cin = ncin;
  }
  // the tail (gk:85-92), on the lane owning the last entry
  const int tail_lane = E == 0 ? 0 : (E - 1) / K;
  const int t0 = E == 0 ? 0 : ga[E - 1];
  int cnt_tail = 0;
  if (lane == tail_lane) {
    int64_t acc = 0;
    for (int i = t0; i < M; ++i) {
      acc += m.ig[i];
      if (i + 1 < M && acc + m.ig[i + 1] + m.id[i + 1] <= T) continue;  // into record i+1
      ++cnt_tail;
      acc = 0;
    }
  }
  const int mine = (j0 < E ? cnt_blk : 0) + cnt_tail;
  const uint32_t incl = wave_incl_scan_u32((uint32_t)mine, lane);
  const int total = __builtin_amdgcn_readlane((int)incl, 63);
  if (total > outcap) {
    if (lane == 0) *sh_out = -1;
  } else {
    const int obase = (int)incl - mine;
    int wrote = 0;
    if (j0 < E) walk(cin, wrote, obase, true);
    if (lane == tail_lane) {
      int o = obase + wrote;
      int64_t acc = 0;
      for (int i = t0; i < M; ++i) {
        acc += m.ig[i];
        if (i + 1 < M && acc + m.ig[i + 1] + m.id[i + 1] <= T) continue;
        m.ov[o] = m.iv[i];
        m.og[o] = (int32_t)acc;
        m.od[o] = m.id[i];
        ++o;
        acc = 0;
      }
    }
    if (lane == 0) *sh_out = total;
  }
}

// ===========================================================================
// k_fold: dst[j].merge(step) over the steps of destination j (gk:111-154 per
// step), one wave per destination.  gk_rollup, gk_merge and
// gk_merge_compress(entries) all run it (FoldArgs, gk_launch.h): the steps are
// the members src[members[k]], k in [goffs[j], goffs[j+1]), or without groups
// the one member src[j], or with eoffs the caller's records (one step).
// The destination's table is loaded into the carve once and stays there: each
// member is converted (gk:136-147), merged with the destination's pending
// values (first step only, gk:71-72) and walked (gk:76-106), and the walk's
// output arrays become the table arrays of the next step by a pointer swap.
// Table and header go back to global memory once, after the last step.
// Members have been flushed by the caller (gk:126 / gk:137; a member with
// n == 0 is not: gk:121-123).
// A step that does not fit this launch's capacity level ends the fold there:
// the state after the step before it is committed (table, n, _min, _max
// together, so nothing of the failed step is applied twice; nothing at all
// when no step fitted), its position goes to progress[j] and j to the overflow
// list; the host raises j's class and re-launches on the list with resume = 1.
// ===========================================================================
template <bool GLOBAL>
__global__ __launch_bounds__(64) void k_fold(FoldArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  __shared__ int sh_out;
  const int lane = threadIdx.x;
  const int CAPL = a.cap;
  unsigned char* base = GLOBAL ? a.ws + (size_t)blockIdx.x * a.ws_bytes : smem;
  const MergeLDS m0 = merge_carve(base, CAPL, a.dst.pmax);
  const GKState& st = a.dst;
  const GKState& os = a.src;
  const bool recs = a.eoffs != nullptr;  // the step is the caller's records, not a member
  for (int64_t w = blockIdx.x; w < a.count; w += gridDim.x) {
    const int64_t j = a.list ? (int64_t)a.list[w] : w;
    // steps [k, kend): positions in members, or without groups the one member j
    int64_t k = j, kend = j + 1;
    if (a.goffs) {
      kend = a.goffs[j + 1];
      k = a.resume ? a.progress[j] : a.goffs[j];
    }
    if (k >= kend) continue;  // an empty group: the destination is not touched (not flushed)
    const int64_t k0 = k;
    GKRec* __restrict__ tab = gk_table_ptr(st, j);
    const int outcap = min(st.cap[st.cls[j]], CAPL) - 1;  // k_ingest keeps one slot for padding
    const double* __restrict__ pb = st.pbuf + j * (int64_t)st.pmax;
    int64_t n = st.n[j];
    int E = st.E[j];
    int p = st.pend[j];
    double mn = st.mn[j], mx = st.mx[j], sum = st.sum[j], avg = st.avg[j];
    // the next member's id, n, table size and table address are loaded one
    // member ahead (no merge of this fold writes src), off the chain of
    // dependent steps -- the first one's beside the destination's header,
    // ahead of the table load
    int64_t ms_nx = 0, on_nx = 0;
    int oE_nx = 0;
    const GKRec* otab_nx = nullptr;
    if (!recs) {
      ms_nx = a.goffs ? a.members[k] : k;
      on_nx = os.n[ms_nx];
      oE_nx = os.E[ms_nx];
      otab_nx = gk_table_ptr(os, ms_nx);
    }
    MergeLDS m = m0;
    bool ovf = E > CAPL;  // the table itself needs a larger level: nothing done yet
    if (!ovf) {
      for (int i = lane; i < E; i += 64) {
        const GKRec rc = tab[i];
        m.tv[i] = rc.v;
        m.tg[i] = rc.g;
        m.td[i] = rc.d;
      }
      __syncthreads();
    }
    for (; !ovf && k < kend; ++k) {
      int nrec = 0;
      int64_t n2 = n;
      double mn2 = mn, mx2 = mx;
      if (recs) {  // gk:63-109 with explicit entries
        const int64_t eo = a.eoffs[j];
        nrec = (int)(a.eoffs[j + 1] - eo);
        if (nrec > CAPL + 1) {
          ovf = true;
          break;
        }
        for (int c = lane; c < nrec; c += 64) {
          m.rv[c] = a.ev[eo + c];
          m.rg[c] = a.eg[eo + c];
          m.rd[c] = a.ed[eo + c];
        }
      } else {
        const int64_t ms = ms_nx;
        const int64_t on = on_nx;
        const int oE = oE_nx;
        const GKRec* __restrict__ otab = otab_nx;
        if (k + 1 < kend) {
          ms_nx = a.members[k + 1];
          on_nx = os.n[ms_nx];
          oE_nx = os.E[ms_nx];
          otab_nx = gk_table_ptr(os, ms_nx);
        }
        if (on != 0 && n == 0) {  // gk:125-133: take a copy of (flushed) other; E == p == 0 here
          if (oE > outcap) {
            ovf = true;
            break;
          }
          for (int i = lane; i < oE; i += 64) {
            const GKRec rc = otab[i];
            m.tv[i] = rc.v;
            m.tg[i] = rc.g;
            m.td[i] = rc.d;
          }
          n = on;
          E = oE;
          p = 0;
          mn = os.mn[ms];
          mx = os.mx[ms];
          sum = os.sum[ms];
          avg = os.avg[ms];
          __syncthreads();
          continue;
        }
        if (on != 0) {
          if (oE > CAPL) {  // (oE + 1 candidate records, rv holds CAPL + 1)
            ovf = true;
            break;
          }
          const int64_t spread = (int64_t)(os.eps * (double)(on - 1));  // gk:136
          const double omn = os.mn[ms], omx = os.mx[ms];
          nrec = merge_convert(m, otab, oE, spread, omn, lane);
          n2 = n + on;  // gk:149
          if (omn < mn2) mn2 = omn;  // gk:151-152: min()/max() keep self's value on ties
          if (omx > mx2) mx2 = omx;
        }
        // on == 0: gk:121-123, self.merge_compress() with no records
      }
      if (!gk_count_ok(st, n2)) {
        ovf = true;
        break;
      }
      merge_sort_pending(m, pb, p, lane);
      merge_incoming(m, p, nrec, lane);
      __syncthreads();
      merge_walk(m, E, p + nrec, (int64_t)floor(st.two_eps * (double)(n2 - 1)) /* gk:70 */, outcap, lane, &sh_out);
      __syncthreads();
      const int no = sh_out;
      if (no < 0) {
        ovf = true;
        break;
      }
      // the output is the next step's table
      { double* t = m.tv; m.tv = m.ov; m.ov = t; }
      { int32_t* t = m.tg; m.tg = m.og; m.og = t; }
      { int32_t* t = m.td; m.td = m.od; m.od = t; }
      E = no;
      n = n2;
      p = 0;
      mn = mn2;
      mx = mx2;
    }
    // commit: the fold up to (not including) step k
    if (k != k0) {
      for (int i = lane; i < E; i += 64) {
        GKRec rc;
        rc.v = m.tv[i];
        rc.g = m.tg[i];
        rc.d = m.td[i];
        tab[i] = rc;
      }
      if (lane == 0) {
        st.n[j] = n;
        st.E[j] = E;
        st.pend[j] = p;
        st.mn[j] = mn;
        st.mx[j] = mx;
        st.sum[j] = sum;
        st.avg[j] = avg;
      }
    }
    if (ovf) {
      if (lane == 0 && a.progress) a.progress[j] = k;
      flag_overflow(a.ovf_count, a.ovf_list, j, lane);
    }
    __syncthreads();
  }
}

// Roll-up argument checks, before anything is mutated.  bad bit 0: the
// offsets do not start at 0 or decrease; bit 1: a member outside [0, S);
// bit 2: a source stream listed more than once (bitmap: one bit per source
// stream, zeroed by the caller).
__global__ void k_rollup_check_offsets(const int64_t* __restrict__ goffs, int64_t G, int32_t* __restrict__ bad) {
  const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j == 0 && goffs[0] != 0) atomicOr(bad, 1);
  if (j < G && goffs[j + 1] < goffs[j]) atomicOr(bad, 1);
}

__global__ void k_rollup_check_members(const int64_t* __restrict__ members, int64_t M, int64_t S,
                                       uint32_t* __restrict__ bitmap, int32_t* __restrict__ bad) {
  const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= M) return;
  const int64_t ms = members[k];
  if (ms < 0 || ms >= S) {
    atomicOr(bad, 2);
    return;
  }
  const uint32_t bit = 1u << (ms & 31);
  if (atomicOr(&bitmap[ms >> 5], bit) & bit) atomicOr(bad, 4);
}

// the members that the reference flushes (gk:126 / gk:137: every `other` with n != 0)
__global__ void k_rollup_flush_list(GKState src, const int64_t* __restrict__ members, int64_t M,
                                    int32_t* __restrict__ count, int32_t* __restrict__ list) {
  const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= M) return;
  const int64_t ms = members[k];
  if (src.n[ms] != 0) list[atomicAdd(count, 1)] = (int32_t)ms;
}

// ===========================================================================
// Per-stream selection (gk_quantiles_select / gk_flush_select /
// gk_reset_select / gk_stats_select): the calls take a list `ids` of `count`
// stream ids, in any order, repeats allowed.
// ===========================================================================
// k_select_check: the id check and, list != NULL (flush / query), the flush
// list, in one pass over ids that mutates no stream state -- one readback of
// ctl gives the verdict and the list length before anything is changed.
//  * an id outside [0, S): ctl[GK_SEL_BAD] is set and ctl[GK_SEL_FIRST] takes
//    the maximum of count - k over the bad positions k (count minus the FIRST
//    bad index: an atomicMax over words the caller zeroed);
//  * a listed stream with n > 0 and pending values -- the streams that
//    quantile() / quantiles() / size() flush first, gk:45-46, 166-167, 197-198
//    -- joins `list` ONCE (bitmap: one bit per stream, zeroed by the caller),
//    ctl[GK_SEL_COUNT] of them.  A stream without pending values is not
//    listed: it is not compressed again.
__global__ void k_select_check(GKState st, const int32_t* __restrict__ ids, int64_t count, int32_t* __restrict__ ctl,
                               uint32_t* __restrict__ bitmap, int32_t* __restrict__ list) {
  const int64_t step = (int64_t)gridDim.x * blockDim.x;
  for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k < count; k += step) {
    const int64_t s = ids[k];
    if (s < 0 || s >= st.S) {
      atomicOr(&ctl[GK_SEL_BAD], 1);
      atomicMax(reinterpret_cast<uint32_t*>(&ctl[GK_SEL_FIRST]), (uint32_t)(count - k));
      continue;
    }
    if (!list || st.n[s] <= 0 || st.pend[s] <= 0) continue;
    const uint32_t bit = 1u << (s & 31);
    if (!(atomicOr(&bitmap[s >> 5], bit) & bit)) list[atomicAdd(&ctl[GK_SEL_COUNT], 1)] = (int32_t)s;
  }
}

// k_select_query: row k of out = quantiles (gk:156-232) of stream ids[k] from
// its committed table, one wave per row (a stream listed twice is answered
// twice from the same table).  The call has synchronised after its flush:
// _min/_max are final, so no marker pass as in k_query_list.
__global__ __launch_bounds__(256) void k_select_query(GKState st, const int32_t* __restrict__ ids, int64_t count,
                                                      const double* __restrict__ qs, int nq, int qmode,
                                                      double* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int64_t wid = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6), nwv = (int64_t)gridDim.x * 4;
  for (int64_t k = wid; k < count; k += nwv) {
    const int64_t s = ids[k];
    const GKRec* tab = gk_table_ptr(st, s);
    wave_quantiles<2, 4>(&tab->v, &tab->g, &tab->d, st.E[s], st.n[s], st.mn[s], st.mx[s], st, qs, nq, qmode,
                         out + k * (int64_t)nq, lane);
  }
}

// k_rank: row k of lo / hi = the rank bounds (wave_ranks) of stream ids[k] --
// ids == NULL: of stream k -- for the nx thresholds xs, from its committed
// table, one wave per row.  The call has flushed and synchronised: the table
// and n / _min / _max are final.  Reads only; lo or hi may be NULL.
__global__ __launch_bounds__(256, 6) void k_rank(GKState st, const int32_t* __restrict__ ids, int64_t count,
                                              const double* __restrict__ xs, int nx, int64_t* __restrict__ lo,
                                              int64_t* __restrict__ hi) {
  const int lane = threadIdx.x & 63;
  const int64_t wid = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6), nwv = (int64_t)gridDim.x * 4;
  for (int64_t k = wid; k < count; k += nwv) {
    const int64_t s = ids ? (int64_t)ids[k] : k;
    const GKRec* tab = gk_table_ptr(st, s);
    wave_ranks<2, 4>(&tab->v, &tab->g, &tab->d, st.E[s], st.n[s], st.mn[s], st.mx[s], xs, nx,
                     lo ? lo + k * (int64_t)nx : nullptr, hi ? hi + k * (int64_t)nx : nullptr, lane);
  }
}

// k_select_reset: every listed stream back to GKArray(eps) (gk:21-29), the
// header values of k_reset -- but cls and slot stay: arenas are bump-allocated
// and the class member lists have no removal, so a stream put back in class 0
// would be listed twice after its next promotion.  (A repeated id writes the
// same values twice.)
__global__ void k_select_reset(GKState st, const int32_t* __restrict__ ids, int64_t count) {
  const int64_t step = (int64_t)gridDim.x * blockDim.x;
  for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k < count; k += step) {
    const int64_t s = ids[k];
    st.n[s] = 0;
    st.E[s] = 0;
    st.pend[s] = 0;
    st.mn[s] = __longlong_as_double(0x7ff0000000000000LL);   // +inf (gk:25)
    st.mx[s] = __longlong_as_double((long long)0xfff0000000000000ULL);  // -inf (gk:26)
    st.sum[s] = 0.0;
    st.avg[s] = 0.0;
  }
}

// k_select_stats: gk_stats' arrays gathered at ids (any output may be NULL)
__global__ void k_select_stats(GKState st, const int32_t* __restrict__ ids, int64_t count, GKSelectStats o) {
  const int64_t step = (int64_t)gridDim.x * blockDim.x;
  for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k < count; k += step) {
    const int64_t s = ids[k];
    if (o.n) o.n[k] = st.n[s];
    if (o.mn) o.mn[k] = st.mn[s];
    if (o.mx) o.mx[k] = st.mx[s];
    if (o.sum) o.sum[k] = st.sum[s];
    if (o.avg) o.avg[k] = st.avg[s];
    if (o.table_size) o.table_size[k] = st.E[s];
    if (o.pending) o.pending[k] = st.pend[s];
  }
}

// ===========================================================================
// state movement
// ===========================================================================
// ctr (gk_reset): the set's slot and member-list counters start over too
// (words [0, GK_CTR_FATAL); FATAL stays cumulative)
__global__ void k_reset(GKState st, int32_t* __restrict__ ctr) {
  const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  // (+ the per-call block [GK_CTR_CALL, GK_CALL_BYTES): the next call's
  // begin_call then skips its memset -- one dispatch fewer per step)
  if (ctr && (s < GK_CTR_FATAL || (s >= GK_CTR_CALL && s < GK_CALL_BYTES / 4))) ctr[s] = 0;
  if (s >= st.S) return;
  st.n[s] = 0;
  st.E[s] = 0;
  st.pend[s] = 0;
  st.mn[s] = __longlong_as_double(0x7ff0000000000000LL);   // +inf (gk:25)
  st.mx[s] = __longlong_as_double((long long)0xfff0000000000000ULL);  // -inf (gk:26)
  st.sum[s] = 0.0;
  st.avg[s] = 0.0;
  st.cls[s] = 0;  // every stream back in class 0
  st.slot[s] = 0;
}

__global__ void k_export(GKState st, const int64_t* __restrict__ offs, double* __restrict__ v,
                         int32_t* __restrict__ g, int32_t* __restrict__ d) {
  const int lane = threadIdx.x & 63;
  const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int64_t nw = ((int64_t)gridDim.x * blockDim.x) >> 6;
  for (int64_t s = wave; s < st.S; s += nw) {
    const GKRec* tab = gk_table_ptr(st, s);
    const int E = st.E[s];
    const int64_t o = offs[s];
    for (int j = lane; j < E; j += 64) {
      const GKRec rc = tab[j];
      if (v) v[o + j] = rc.v;
      if (g) g[o + j] = rc.g;
      if (d) d[o + j] = rc.d;
    }
  }
}

__global__ void k_export_pending(GKState st, const int64_t* __restrict__ offs, double* __restrict__ v) {
  const int lane = threadIdx.x & 63;
  const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int64_t nw = ((int64_t)gridDim.x * blockDim.x) >> 6;
  for (int64_t s = wave; s < st.S; s += nw) {
    const int p = st.pend[s];
    const double* pb = st.pbuf + s * (int64_t)st.pmax;
    const int64_t o = offs[s];
    for (int j = lane; j < p; j += 64) v[o + j] = pb[j];
  }
}

// gk_import's argument check, before any state is written: a stream's
// pending count p must be one that add() can leave behind -- the values added
// since n last crossed a multiple of P (gk:60), so p <= n mod P (and p = 0
// when n mod P = 0).  A flush batch is then at most P values.
__global__ void k_check_pending(int64_t S, int P, const int64_t* __restrict__ n, const int64_t* __restrict__ poffs,
                                int32_t* __restrict__ bad) {
  const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= S) return;
  const int64_t p = poffs[s + 1] - poffs[s];
  const int64_t ns = n[s];
  if (p < 0 || ns < 0 || p > ns % P) atomicAdd(bad, 1);
}

__global__ void k_import(GKState st, const int64_t* __restrict__ offs, const double* __restrict__ v,
                         const int32_t* __restrict__ g, const int32_t* __restrict__ d,
                         const int64_t* __restrict__ poffs, const double* __restrict__ pv,
                         int32_t* __restrict__ ovf_count, int32_t* __restrict__ ovf_list) {
  const int lane = threadIdx.x & 63;
  const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int64_t nw = ((int64_t)gridDim.x * blockDim.x) >> 6;
  for (int64_t s = wave; s < st.S; s += nw) {
    const int cap = st.cap[st.cls[s]] - 1;  // k_ingest keeps one slot for padding
    const int64_t o = offs[s];
    const int E = (int)(offs[s + 1] - o);
    const int64_t po = poffs[s];
    const int p = (int)(poffs[s + 1] - po);
    if (E > cap || p > st.pmax) {
      if (lane == 0) {
        const int k = atomicAdd(ovf_count, 1);
        ovf_list[k] = (int32_t)s;
      }
      continue;
    }
    GKRec* tab = gk_table_ptr(st, s);
    for (int j = lane; j < E; j += 64) {
      GKRec rc;
      rc.v = v[o + j];
      rc.g = g[o + j];
      rc.d = d[o + j];
      tab[j] = rc;
    }
    double* pb = st.pbuf + s * (int64_t)st.pmax;
    for (int j = lane; j < p; j += 64) pb[j] = pv[po + j];
    if (lane == 0) {
      st.E[s] = E;
      st.pend[s] = p;
    }
  }
}

// ---- stream transfer (gk_pack_select / gk_unpack_select): a LIST of streams
// to and from a GKPACK01 buffer (gk_pack.h), row k of the buffer = stream
// ids[k].  Neither direction flushes.
//
// k_pack_sizes: the two totals (sum of E and of pend over the rows, added to
// totals[0] / totals[1], zeroed by the caller) and, eoffs != NULL, the sizes as
// int64 into eoffs / poffs[0 .. count) with a 0 at [count] -- the input of the
// in-place exclusive scan (gk_launch_scan_i64) that turns them into offsets.
__global__ __launch_bounds__(256) void k_pack_sizes(GKState st, const int32_t* __restrict__ ids, int64_t count,
                                                    int64_t* __restrict__ eoffs, int64_t* __restrict__ poffs,
                                                    unsigned long long* __restrict__ totals) {
  const int lane = threadIdx.x & 63;
  const int64_t step = (int64_t)gridDim.x * blockDim.x;
  unsigned long long te = 0, tp = 0;
  for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k <= count; k += step) {  // ([count]: the 0)
    int64_t e = 0, p = 0;
    if (k < count) {
      const int64_t s = ids[k];
      e = st.E[s];
      p = st.pend[s];
    }
    if (eoffs) {
      eoffs[k] = e;
      poffs[k] = p;
    }
    te += (unsigned long long)e;
    tp += (unsigned long long)p;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    te += __shfl_xor(te, o, 64);
    tp += __shfl_xor(tp, o, 64);
  }
  if (lane == 0 && (te | tp)) {
    if (te) atomicAdd(&totals[0], te);
    if (tp) atomicAdd(&totals[1], tp);
  }
}

// k_pack_select: one wave per row; the table leaves as 16-byte records
// (int4: v low, v high, g, delta) into v / g / d at eoffs[k], the pending
// values in insertion order into pv at poffs[k].  Reads the set only.  (A row
// with a very long table is walked by its one wave.)
__global__ __launch_bounds__(256) void k_pack_select(GKState st, const int32_t* __restrict__ ids, int64_t count,
                                                     const int64_t* __restrict__ eoffs,
                                                     const int64_t* __restrict__ poffs, double* __restrict__ v,
                                                     int32_t* __restrict__ g, int32_t* __restrict__ d,
                                                     double* __restrict__ pv) {
  const int lane = threadIdx.x & 63;
  const int64_t wid = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6), nwv = (int64_t)gridDim.x * 4;
  for (int64_t k = wid; k < count; k += nwv) {
    const int64_t s = ids[k];
    const int4* __restrict__ t4 = (const int4*)gk_table_ptr(st, s);
    const int E = st.E[s];
    const int p = st.pend[s];
    const int64_t o = eoffs[k], po = poffs[k];
    for (int j = lane; j < E; j += 64) {
      const int4 rc = t4[j];
      v[o + j] = __hiloint2double(rc.y, rc.x);
      g[o + j] = rc.z;
      d[o + j] = rc.w;
    }
    const double* __restrict__ pb = st.pbuf + s * (int64_t)st.pmax;
    for (int j = lane; j < p; j += 64) pv[po + j] = pb[j];
  }
}

// The class a stream in class c moves to for a table of E entries: the first
// above c that holds it (a class keeps one slot for padding, as k_import's
// rule); nclass when none does.
__device__ __forceinline__ int unpack_target(const GKState& st, int c, int64_t E) {
  int t = c + 1;
  while (t < st.nclass && E > (int64_t)st.cap[t] - 1) ++t;
  return t;
}

// k_unpack_check: every refusal of gk_unpack_select that needs the device, in
// one pass that mutates no stream state; ctl (GK_UNP_WORDS words) and the
// bitmap ((S + 31) / 32 words) are zeroed by the caller, who reads ctl back
// before anything is written.  Row k:
//  * ids[k] outside [0, S): bit 1 of ctl[GK_UNP_BAD], count - k into the max
//    ctl[GK_UNP_FIRST] (k_select_check's encoding of the FIRST bad index);
//  * ids[k] listed before (bitmap): bit 2;
//  * offsets not monotone from 0 to the header's totals: bit 4;
//  * a pending count that add() cannot leave (k_check_pending's rule): bit 8;
//  * its table size into the max ctl[GK_UNP_MAXE], and, when the table does
//    not fit the stream's class, one more slot needed in the class it moves to
//    (ctl[GK_UNP_NEED + t]) -- the host grows the arenas from these before the
//    first write.
__global__ void k_unpack_check(GKState st, const int32_t* __restrict__ ids, int64_t count, GKPacked pk,
                               int32_t* __restrict__ ctl, uint32_t* __restrict__ bitmap) {
  const int64_t step = (int64_t)gridDim.x * blockDim.x;
  for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k < count; k += step) {
    int bad = 0;
    const int64_t e0 = pk.eoffs[k], e1 = pk.eoffs[k + 1], p0 = pk.poffs[k], p1 = pk.poffs[k + 1];
    if (e1 < e0 || p1 < p0 || (k == 0 && (e0 != 0 || p0 != 0)) || (k == count - 1 && (e1 != pk.E || p1 != pk.P)))
      bad |= 4;
    const int64_t ns = pk.n[k], p = p1 - p0, E = e1 - e0;
    if (!(bad & 4) && (ns < 0 || p > ns % st.P)) bad |= 8;
    const int64_t s = ids[k];
    if (s < 0 || s >= st.S) {
      bad |= 1;
      atomicMax(reinterpret_cast<uint32_t*>(&ctl[GK_UNP_FIRST]), (uint32_t)(count - k));
    } else {
      const uint32_t bit = 1u << (s & 31);
      if (atomicOr(&bitmap[s >> 5], bit) & bit) bad |= 2;
      if (!(bad & 4)) {
        atomicMax(&ctl[GK_UNP_MAXE], (int32_t)(E > INT32_MAX ? INT32_MAX : E));
        const int c = st.cls[s];
        if (E > (int64_t)st.cap[c] - 1) {
          const int t = unpack_target(st, c, E);
          if (t < st.nclass) atomicAdd(&ctl[GK_UNP_NEED + t], 1);
        }
      }
    }
    if (bad) atomicOr(&ctl[GK_UNP_BAD], bad);
  }
}

// k_unpack_select: one wave per row k (rows == NULL: every row of the buffer;
// else rows[0 .. nrows)).  A row whose table fits its stream's class installs
// the table, the pending values and ALL header words in this one pass -- a
// stream therefore holds its complete old or its complete new state, whatever
// happens to other rows.  A row that does not fit joins the overflow list of
// the class t it moves to: its stream id into ov.list[t] (k_promote_dev's
// input) and the row into ov.rows[t] at the same position, ov.count[t] of
// them; the host promotes the listed streams and launches again over
// ov.rows[t].  (On the relaunch every row fits; one that still does not --
// its promotion found no slot -- is counted in *ov.stuck and left alone.)
__global__ __launch_bounds__(256) void k_unpack_select(GKState st, const int32_t* __restrict__ ids,
                                                       const int32_t* __restrict__ rows, int64_t nrows, GKPacked pk,
                                                       GKUnpackOvf ov) {
  const int lane = threadIdx.x & 63;
  const int64_t wid = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6), nwv = (int64_t)gridDim.x * 4;
  for (int64_t w = wid; w < nrows; w += nwv) {
    const int64_t k = rows ? (int64_t)rows[w] : w;
    const int64_t s = ids[k];
    const int64_t o = pk.eoffs[k], po = pk.poffs[k];
    const int64_t E = pk.eoffs[k + 1] - o;
    const int p = (int)(pk.poffs[k + 1] - po);
    const int c = st.cls[s];
    if (E > (int64_t)st.cap[c] - 1) {
      if (lane == 0) {
        const int t = unpack_target(st, c, E);
        if (rows || t >= st.nclass) {
          atomicAdd(ov.stuck, 1);
        } else {
          const int i = atomicAdd(&ov.count[t], 1);
          ov.list[t][i] = (int32_t)s;
          ov.rows[t][i] = (int32_t)k;
        }
      }
      continue;
    }
    int4* __restrict__ t4 = (int4*)gk_table_ptr(st, s);
    for (int j = lane; j < (int)E; j += 64) {
      const double x = pk.v[o + j];
      t4[j] = make_int4(__double2loint(x), __double2hiint(x), pk.g[o + j], pk.d[o + j]);
    }
    double* __restrict__ pb = st.pbuf + s * (int64_t)st.pmax;
    for (int j = lane; j < p; j += 64) pb[j] = pk.pv[po + j];
    if (lane == 0) {
      st.E[s] = (int32_t)E;
      st.pend[s] = p;
      st.n[s] = pk.n[k];
      st.mn[s] = pk.mn[k];
      st.mx[s] = pk.mx[k];
      st.sum[s] = pk.sum[k];
      st.avg[s] = pk.avg[k];
    }
  }
}

// move each listed stream's table into its (already assigned) slot of class `ncls`
__global__ void k_promote(GKState st, const int32_t* __restrict__ list, int64_t count,
                          const int32_t* __restrict__ slots, int ncls) {
  const int lane = threadIdx.x & 63;
  const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int64_t nw = ((int64_t)gridDim.x * blockDim.x) >> 6;
  for (int64_t w = wave; w < count; w += nw) {
    const int64_t s = list[w];
    const int32_t slot = slots[w];
    const GKRec* src = gk_table_ptr(st, s);
    GKRec* dst = st.tab[ncls] + (int64_t)slot * st.cap[ncls];
    const int E = st.E[s];
    for (int j = lane; j < E; j += 64) dst[j] = src[j];
    __builtin_amdgcn_wave_barrier();
    if (lane == 0) {
      st.cls[s] = ncls;
      st.slot[s] = slot;
    }
  }
}

// Device-side promotion (no host round trip): every stream on the list
// (count from the device) moves to class t = cls+1 (level < 0: an ingest
// overflow) or t = level when it is below that class (level >= 0: a merge at
// capacity level `level`).  Its slot comes from the class's device counter;
// the table is copied over, the stream joins the class member list and, for
// ingest, the re-run list of this round.  The stream's state was not
// committed, so it stays as it is when it cannot move: no free slot in its
// next class -> the defer list (the host grows the arena and re-runs it before
// the set's next call); no class above -> ctr[GK_CTR_FATAL], reported as a
// (sticky) GK_E_OVERFLOW.
__global__ void k_promote_dev(GKState st, const int32_t* __restrict__ count, const int32_t* __restrict__ list,
                              int level, GKPoolDev pool) {
  const int lane = threadIdx.x & 63;
  const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int64_t nw = ((int64_t)gridDim.x * blockDim.x) >> 6;
  const int64_t cnt = *count;
  for (int64_t w = wave; w < cnt; w += nw) {
    const int64_t s = list[w];
    const int c = st.cls[s];
    const int t = level < 0 ? c + 1 : level;  // -1: ingest overflow, -2: import overflow
    if (level >= 0 && c >= t) continue;      // already large enough
    int slot = -1;
    if (lane == 0) {
      if (t < st.nclass) {
        slot = atomicAdd(&pool.ctr[GK_CTR_USED + t], 1);
        if (slot >= st.alloc[t]) {
          atomicSub(&pool.ctr[GK_CTR_USED + t], 1);
          slot = -1;
          if (level == -1) pool.defer[atomicAdd(&pool.ctr[GK_CTR_DEFER], 1)] = (int32_t)s;
          else atomicAdd(&pool.ctr[GK_CTR_FATAL], 1);  // (merge / import grow the arena first)
        }
      } else {
        atomicAdd(&pool.ctr[GK_CTR_FATAL], 1);
        atomicMax(&pool.ctr[GK_CTR_FATAL + 1], (int)s);
      }
    }
    slot = __shfl(slot, 0, 64);
    if (slot < 0) continue;
    const GKRec* src = gk_table_ptr(st, s);
    GKRec* dst = st.tab[t] + (int64_t)slot * st.cap[t];
    const int E = min(st.E[s], st.cap[c]);
    for (int j = lane; j < E; j += 64) dst[j] = src[j];
    __builtin_amdgcn_wave_barrier();
    if (lane == 0) {
      st.cls[s] = t;
      st.slot[s] = slot;
      pool.list[t][atomicAdd(&pool.ctr[GK_CTR_LCNT + t], 1)] = (int32_t)s;
      if (level == -1) pool.rerun[t][atomicAdd(&pool.rcnt[t], 1)] = (int32_t)s;
    }
  }
}

// ===========================================================================
// host-side launchers (called from gk_capi.cpp)
// ===========================================================================
hipError_t gk_launch_stats(const GKState& st, const int64_t* offs, int32_t* long_list, int32_t* long_count,
                           hipStream_t stream) {
  if (st.S <= 0) return hipSuccess;
  const int64_t grid = (st.S + 255) / 256;
  // the long-stream list first (k_lengths, a few us), so that the caller can
  // fork k_stats_long -- the sequential chains of the longest streams, the
  // critical path of a Zipf batch -- before the short streams' chains
  // (gk_launch_stats_short) run on this stream
  hipLaunchKernelGGL(k_lengths, dim3((unsigned)grid), dim3(256), 0, stream, st, offs, long_list, long_count);
  return hipGetLastError();
}

hipError_t gk_launch_query_list(const GKState& st, const int32_t* list, const int32_t* count, const GKQuery& q,
                                bool qfix, hipStream_t stream) {
  if (st.S <= 0 || !q.qs || q.nq <= 0) return hipSuccess;
  // (4 waves per block: gk_num_cu() blocks = 4 waves per CU for the list; the
  // marker fix needs one thread per answer)
  const int64_t grid = std::max<int64_t>(gk_num_cu(), qfix ? (st.S * (int64_t)q.nq + 255) / 256 : 0);
  hipLaunchKernelGGL(k_query_list, dim3((unsigned)grid), dim3(256), 0, stream, st, list, count, q.qs, q.nq,
                     q.mode, q.out, qfix ? 1 : 0);
  return hipGetLastError();
}

size_t gk_merge_lds_bytes(int cap, int pmax) {
  const size_t MR = (size_t)cap + 1, MI = (size_t)cap + 1 + pmax;
  size_t b = 8 * ((size_t)cap + MR + pmax + MI + cap) + 4 * (2 * (size_t)cap + 2 * MR + 2 * MI + 2 * (size_t)cap) + 16;
  return (b + 255) & ~(size_t)255;
}

hipError_t gk_launch_fold(const FoldArgs& a, hipStream_t stream) {
  if (a.count <= 0) return hipSuccess;
  if (a.goffs && a.eoffs) return hipErrorInvalidValue;  // explicit records are one step
  const size_t lds = gk_merge_lds_bytes(a.cap, a.dst.pmax);
  if (a.ws) {
    if (a.ws_bytes < lds || a.ws_blocks <= 0) return hipErrorInvalidValue;
    const int64_t grid = std::min(a.ws_blocks, a.count);
    hipLaunchKernelGGL(k_fold<true>, dim3((unsigned)grid), dim3(64), 0, stream, a);
    return hipGetLastError();
  }
  if (lds > 160 * 1024 - 64) return hipErrorInvalidValue;
  if (lds > 48 * 1024)
    (void)hipFuncSetAttribute((const void*)k_fold<false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  // groups: one block per destination (up to 2^20; the kernel's loop takes the
  // rest) -- a fold is a long chain of dependent steps, so every wave the LDS
  // carve lets a CU hold should be resident, and folds of uneven length are
  // handed out as blocks retire.  One step each: 8 blocks per CU over the loop.
  const int64_t grid = std::min(a.goffs ? (int64_t)1 << 20 : (int64_t)gk_num_cu() * 8, a.count);
  hipLaunchKernelGGL(k_fold<false>, dim3((unsigned)grid), dim3(64), lds, stream, a);
  return hipGetLastError();
}

hipError_t gk_launch_rollup_check_offsets(const int64_t* goffs, int64_t G, int32_t* bad, hipStream_t stream) {
  const int64_t nthr = G > 0 ? G : 1;  // (thread 0 checks goffs[0] also when there is no group)
  hipLaunchKernelGGL(k_rollup_check_offsets, dim3((unsigned)((nthr + 255) / 256)), dim3(256), 0, stream, goffs, G, bad);
  return hipGetLastError();
}

hipError_t gk_launch_rollup_check_members(const int64_t* members, int64_t M, int64_t S, uint32_t* bitmap, int32_t* bad,
                                          hipStream_t stream) {
  if (M <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_rollup_check_members, dim3((unsigned)((M + 255) / 256)), dim3(256), 0, stream, members, M, S,
                     bitmap, bad);
  return hipGetLastError();
}

hipError_t gk_launch_rollup_flush_list(const GKState& src, const int64_t* members, int64_t M, int32_t* count,
                                       int32_t* list, hipStream_t stream) {
  if (M <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_rollup_flush_list, dim3((unsigned)((M + 255) / 256)), dim3(256), 0, stream, src, members, M,
                     count, list);
  return hipGetLastError();
}

__global__ void k_rtab(GKState st) {
  const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k < st.rtab_n) st.rtab[k] = k == 0 ? 0.0 : 1.0 / (double)k;  // same IEEE division as gk_stat_step
}

hipError_t gk_launch_rtab(const GKState& st, hipStream_t stream) {
  if (!st.rtab || st.rtab_n <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_rtab, dim3((unsigned)((st.rtab_n + 255) / 256)), dim3(256), 0, stream, st);
  return hipGetLastError();
}

hipError_t gk_launch_reset(const GKState& st, hipStream_t stream, int32_t* ctr) {
  if (st.S <= 0 && !ctr) return hipSuccess;
  const int64_t grid = (std::max<int64_t>(st.S, GK_CALL_BYTES / 4) + 255) / 256;
  hipLaunchKernelGGL(k_reset, dim3((unsigned)grid), dim3(256), 0, stream, st, ctr);
  return hipGetLastError();
}

static int64_t wave_grid(int64_t S) {
  int64_t g = (S + 3) / 4;
  const int64_t cap = (int64_t)gk_num_cu() * 16;
  if (g > cap) g = cap;
  if (g < 1) g = 1;
  return g;
}

// one thread per listed id, at most 2^16 blocks (the kernels loop)
static unsigned select_grid(int64_t count) { return (unsigned)std::min<int64_t>((count + 255) / 256, 65536); }

hipError_t gk_launch_select_check(const GKState& st, const int32_t* ids, int64_t count, int32_t* ctl, uint32_t* bitmap,
                                  int32_t* list, hipStream_t stream) {
  if (count <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_select_check, dim3(select_grid(count)), dim3(256), 0, stream, st, ids, count, ctl, bitmap, list);
  return hipGetLastError();
}

hipError_t gk_launch_select_query(const GKState& st, const int32_t* ids, int64_t count, const GKQuery& q,
                                  hipStream_t stream) {
  if (count <= 0 || !q.qs || q.nq <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_select_query, dim3((unsigned)wave_grid(count)), dim3(256), 0, stream, st, ids, count, q.qs,
                     q.nq, q.mode, q.out);
  return hipGetLastError();
}

hipError_t gk_launch_rank(const GKState& st, const int32_t* ids, int64_t count, const double* xs, int nx, int64_t* lo,
                          int64_t* hi, hipStream_t stream) {
  if (count <= 0 || !xs || nx <= 0 || (!lo && !hi)) return hipSuccess;
  hipLaunchKernelGGL(k_rank, dim3((unsigned)wave_grid(count)), dim3(256), 0, stream, st, ids, count, xs, nx, lo, hi);
  return hipGetLastError();
}

hipError_t gk_launch_select_reset(const GKState& st, const int32_t* ids, int64_t count, hipStream_t stream) {
  if (count <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_select_reset, dim3(select_grid(count)), dim3(256), 0, stream, st, ids, count);
  return hipGetLastError();
}

hipError_t gk_launch_select_stats(const GKState& st, const int32_t* ids, int64_t count, const GKSelectStats& o,
                                  hipStream_t stream) {
  if (count <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_select_stats, dim3(select_grid(count)), dim3(256), 0, stream, st, ids, count, o);
  return hipGetLastError();
}

hipError_t gk_launch_export(const GKState& st, const int64_t* offs, double* v, int32_t* g, int32_t* d,
                            hipStream_t stream) {
  if (st.S <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_export, dim3((unsigned)wave_grid(st.S)), dim3(256), 0, stream, st, offs, v, g, d);
  return hipGetLastError();
}

hipError_t gk_launch_export_pending(const GKState& st, const int64_t* offs, double* v, hipStream_t stream) {
  if (st.S <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_export_pending, dim3((unsigned)wave_grid(st.S)), dim3(256), 0, stream, st, offs, v);
  return hipGetLastError();
}

hipError_t gk_launch_check_pending(int64_t S, int P, const int64_t* n, const int64_t* poffs, int32_t* bad,
                                  hipStream_t stream) {
  if (S <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_check_pending, dim3((unsigned)((S + 255) / 256)), dim3(256), 0, stream, S, P, n, poffs, bad);
  return hipGetLastError();
}

hipError_t gk_launch_import(const GKState& st, const int64_t* offs, const double* v, const int32_t* g,
                            const int32_t* d, const int64_t* poffs, const double* pv, int32_t* ovf_count,
                            int32_t* ovf_list, hipStream_t stream) {
  if (st.S <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_import, dim3((unsigned)wave_grid(st.S)), dim3(256), 0, stream, st, offs, v, g, d,
                     poffs, pv, ovf_count, ovf_list);
  return hipGetLastError();
}

hipError_t gk_launch_pack_sizes(const GKState& st, const int32_t* ids, int64_t count, int64_t* eoffs, int64_t* poffs,
                                unsigned long long* totals, hipStream_t stream) {
  if (count < 0) return hipSuccess;
  hipLaunchKernelGGL(k_pack_sizes, dim3(select_grid(count + 1)), dim3(256), 0, stream, st, ids, count, eoffs, poffs,
                     totals);
  return hipGetLastError();
}

hipError_t gk_launch_pack_select(const GKState& st, const int32_t* ids, int64_t count, const int64_t* eoffs,
                                 const int64_t* poffs, double* v, int32_t* g, int32_t* d, double* pv,
                                 hipStream_t stream) {
  if (count <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_pack_select, dim3((unsigned)wave_grid(count)), dim3(256), 0, stream, st, ids, count, eoffs,
                     poffs, v, g, d, pv);
  return hipGetLastError();
}

hipError_t gk_launch_unpack_check(const GKState& st, const int32_t* ids, int64_t count, const GKPacked& pk,
                                  int32_t* ctl, uint32_t* bitmap, hipStream_t stream) {
  if (count <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_unpack_check, dim3(select_grid(count)), dim3(256), 0, stream, st, ids, count, pk, ctl, bitmap);
  return hipGetLastError();
}

hipError_t gk_launch_unpack_select(const GKState& st, const int32_t* ids, const int32_t* rows, int64_t nrows,
                                   const GKPacked& pk, const GKUnpackOvf& ov, hipStream_t stream) {
  if (nrows <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_unpack_select, dim3((unsigned)wave_grid(nrows)), dim3(256), 0, stream, st, ids, rows, nrows,
                     pk, ov);
  return hipGetLastError();
}

hipError_t gk_launch_promote_dev(const GKState& st, const int32_t* count, const int32_t* list, int level,
                                 const GKPoolDev& pool, hipStream_t stream) {
  hipLaunchKernelGGL(k_promote_dev, dim3((unsigned)(gk_num_cu() * 2)), dim3(256), 0, stream, st, count, list, level,
                     pool);
  return hipGetLastError();
}

hipError_t gk_launch_promote(const GKState& st, const int32_t* list, int64_t count, const int32_t* slots, int ncls,
                             hipStream_t stream) {
  if (count <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_promote, dim3((unsigned)wave_grid(count)), dim3(256), 0, stream, st, list, count, slots,
                     ncls);
  return hipGetLastError();
}

#ifdef GK_TIMELINE
// timeline builds only (tools/launch_timeline.py; not part of include/gk_capi.h)
extern "C" int gk_tl_call_read(unsigned long long* c) {
  if (hipDeviceSynchronize() != hipSuccess) return -4;
  return hipMemcpyFromSymbol(c, HIP_SYMBOL(gk_tl_call), sizeof(unsigned long long) * 2) == hipSuccess ? 0 : -4;
}
#endif
