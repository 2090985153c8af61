// gk_keyed.hip -- k_group_*: the stable group-by of (stream id, value) samples
// behind gk_group_by_key / gk_ingest_keyed (gfx950, wave64).
//
// A least-significant-digit radix partition of the pairs by stream id, 8 bits
// per pass, written by hand (no rocPRIM / hipCUB).  Kernels of one call, in
// stream order:
//   per pass:  k_group_tilehist  digit counts of every 4096-sample tile (the
//                                first pass also finds ids >= S and leaves
//                                out the negative, skipped ones)
//              k_scan_*          exclusive scan over [digit][tile]; its total
//                                is the number of kept samples
//              k_group_scatter   rank inside the tile + scanned base -> position
//                                (the tile is ordered in LDS first, so that
//                                each digit's samples leave as one run)
//   k_group_verdict   after the first tile counts, one thread: a bad id makes
//                     the call void (every later kernel returns at once) and is
//                     recorded in the set's cumulative block for the host
//   k_group_offsets   out_offsets[s] = lower bound of s in the sorted ids (no
//                     per-stream counters: global atomics took 8x the time of
//                     everything else on random ids, 100x with a hot stream)
// Only kernel boundaries synchronise workgroups.  Every position is a pure
// function of the input: a sample's rank among equal digits of its tile comes
// from wave match masks (ballots) and per-wave LDS counters that one leader
// lane per digit advances, combined in wave order, then lane order; no position
// is taken from the return value of an atomic.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gk_launch.h"

namespace {

constexpr int KG_BITS = GK_GROUP_BITS;          // digit width
constexpr int KG_BINS = 1 << KG_BITS;           // 256
constexpr int KG_THREADS = 256;                 // 4 waves
constexpr int KG_WAVES = KG_THREADS / 64;
constexpr int KG_ITEMS = GK_GROUP_TILE / KG_THREADS;  // 16 samples per lane
constexpr int KG_WAVE_SPAN = 64 * KG_ITEMS;     // 1024 consecutive samples per wave
static_assert(KG_BINS == KG_THREADS, "one thread per digit combines the waves' counts");

constexpr int SC_THREADS = 256;
constexpr int SC_ITEMS = 8;
constexpr int SC_TILE = SC_THREADS * SC_ITEMS;  // == GK_GROUP_SCAN_TILE
static_assert(SC_TILE == GK_GROUP_SCAN_TILE, "scan tile");

typedef unsigned long long u64;

__device__ __forceinline__ u64 wave_sum(u64 v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ u64 wave_max(u64 v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const u64 w = __shfl_xor(v, o, 64);
    v = w > v ? w : v;
  }
  return v;
}

// cum: [0] void calls so far, [1] the first bad sample index of the last one, [2] its id
__global__ void k_group_verdict(const int32_t* __restrict__ ids, int64_t count, const u64* __restrict__ call,
                                u64* __restrict__ cum) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  if (call[GK_KG_BAD] == 0) return;
  const int64_t first = count - (int64_t)call[GK_KG_BADKEY];
  cum[0] += 1;
  cum[1] = (u64)first;
  cum[2] = (u64)(int64_t)ids[first];
}

// ---- exclusive scan of a[0..n) in place: tile sums, scan of the sums by one
// workgroup, tile scan + base.  T = uint32_t (digit counts: every partial sum
// is at most count < 2^31) or int64_t (gk_launch_scan_i64: non-negative sizes).
// call: the keyed call's control words (a void call's scan does nothing), or
// NULL.
template <typename T>
__device__ __forceinline__ void load_tile(const T* a, int64_t n, int64_t base, T (&v)[SC_ITEMS]) {
#pragma unroll
  for (int k = 0; k < SC_ITEMS; ++k) {
    const int64_t i = base + k;
    v[k] = i < n ? a[i] : (T)0;
  }
}

// inclusive scan of one value per thread over the workgroup; returns the exclusive prefix, *total the sum
__device__ __forceinline__ u64 block_exclusive(u64 x, u64* lds, u64* total) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, nw = blockDim.x >> 6;
  u64 inc = x;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const u64 y = __shfl_up(inc, o, 64);
    if (lane >= o) inc += y;
  }
  if (lane == 63) lds[w] = inc;
  __syncthreads();
  u64 pre = 0, tot = 0;
  for (int k = 0; k < nw; ++k) {
    const u64 t = lds[k];
    if (k < w) pre += t;
    tot += t;
  }
  __syncthreads();
  *total = tot;
  return pre + inc - x;
}

template <typename T>
__global__ __launch_bounds__(SC_THREADS) void k_scan_sums(const T* __restrict__ a, int64_t n, u64* __restrict__ sums,
                                                          const u64* __restrict__ call) {
  __shared__ u64 lds[SC_THREADS / 64];
  if (call && call[GK_KG_BAD]) return;
  T v[SC_ITEMS];
  load_tile(a, n, (int64_t)blockIdx.x * SC_TILE + (int64_t)threadIdx.x * SC_ITEMS, v);
  u64 x = 0;
#pragma unroll
  for (int k = 0; k < SC_ITEMS; ++k) x += (u64)v[k];
  u64 tot;
  (void)block_exclusive(x, lds, &tot);
  if (threadIdx.x == 0) sums[blockIdx.x] = tot;
}

// total_out (may be NULL): the sum of the whole array
__global__ __launch_bounds__(1024) void k_scan_mid(u64* __restrict__ sums, int64_t nb, const u64* __restrict__ call,
                                                   u64* __restrict__ total_out) {
  __shared__ u64 lds[1024 / 64];
  if (call && call[GK_KG_BAD]) return;
  u64 carry = 0;
  for (int64_t base = 0; base < nb; base += 1024) {
    const int64_t i = base + threadIdx.x;
    const u64 x = i < nb ? sums[i] : 0;
    u64 tot;
    const u64 pre = block_exclusive(x, lds, &tot);
    if (i < nb) sums[i] = carry + pre;
    carry += tot;
  }
  if (total_out && threadIdx.x == 0) *total_out = carry;
}

template <typename T>
__global__ __launch_bounds__(SC_THREADS) void k_scan_apply(T* __restrict__ a, int64_t n, const u64* __restrict__ sums,
                                                           const u64* __restrict__ call) {
  __shared__ u64 lds[SC_THREADS / 64];
  const int64_t base = (int64_t)blockIdx.x * SC_TILE + (int64_t)threadIdx.x * SC_ITEMS;
  if (call && call[GK_KG_BAD]) return;
  T v[SC_ITEMS];
  load_tile(a, n, base, v);
  u64 x = 0;
#pragma unroll
  for (int k = 0; k < SC_ITEMS; ++k) x += (u64)v[k];
  u64 tot;
  u64 run = sums[blockIdx.x] + block_exclusive(x, lds, &tot);
#pragma unroll
  for (int k = 0; k < SC_ITEMS; ++k) {
    if (base + k < n) a[base + k] = (T)run;
    run += (u64)v[k];
  }
}

// Samples of a pass: the caller's `count` in the first pass (negative ids are
// dropped there), the kept ones afterwards.
template <bool FIRST>
__device__ __forceinline__ int64_t pass_n(int64_t count, const u64* call) {
  return FIRST ? count : (int64_t)call[GK_KG_KEPT];
}

// Digit counts of tile blockIdx.x into hist[digit * tiles + tile] (every tile
// writes all its 256 words: the table is not zeroed).  The first pass sees the
// caller's ids: negative ones are left out, ids >= S are counted in
// call[GK_KG_BAD] with the max of (count - i) over them in call[GK_KG_BADKEY]
// (the first bad index is count minus it); it does not read the verdict it is
// making.
template <bool FIRST>
__global__ __launch_bounds__(KG_THREADS) void k_group_tilehist(const int32_t* __restrict__ ids, int64_t count,
                                                               int64_t S, u64* call, int shift,
                                                               uint32_t* __restrict__ hist, int64_t tiles) {
  __shared__ uint32_t cnt[KG_BINS];
  if (!FIRST && call[GK_KG_BAD]) return;
  const int64_t n = pass_n<FIRST>(count, call);
  cnt[threadIdx.x] = 0;
  __syncthreads();
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int64_t base = (int64_t)blockIdx.x * GK_GROUP_TILE + (int64_t)w * KG_WAVE_SPAN + lane;
  u64 nbad = 0, badkey = 0;
#pragma unroll
  for (int k = 0; k < KG_ITEMS; ++k) {
    const int64_t i = base + k * 64;
    if (i < n) {
      const int32_t id = ids[i];
      if (FIRST && id >= S) {
        ++nbad;
        const u64 key = (u64)(count - i);
        badkey = key > badkey ? key : badkey;
      } else if (!FIRST || id >= 0) {
        atomicAdd(&cnt[((uint32_t)id >> shift) & (KG_BINS - 1)], 1u);
      }
    }
  }
  if (FIRST) {
    nbad = wave_sum(nbad);
    badkey = wave_max(badkey);
    if (lane == 0 && nbad) {
      atomicAdd(&call[GK_KG_BAD], nbad);
      atomicMax(&call[GK_KG_BADKEY], badkey);
    }
  }
  __syncthreads();
  hist[(size_t)threadIdx.x * (size_t)tiles + blockIdx.x] = cnt[threadIdx.x];
}

// The scatter of one pass.  base[digit * tiles + tile] is the scanned table:
// the position of the tile's first sample with that digit.  Wave w of the
// workgroup owns samples [w * 1024, (w + 1) * 1024) of the tile, 64 consecutive
// ones per step, so (wave, step, lane) is ascending sample index.
template <bool FIRST>
__global__ __launch_bounds__(KG_THREADS) void k_group_scatter(const int32_t* __restrict__ ids,
                                                              const double* __restrict__ vals, int64_t count,
                                                              const u64* __restrict__ call, int shift, int nbits,
                                                              const uint32_t* __restrict__ base, int64_t tiles,
                                                              int32_t* __restrict__ out_ids,
                                                              double* __restrict__ out_vals) {
  // 37 KiB of LDS: four workgroups per CU.  cnt_raw holds the per-wave digit
  // counters while the ranks are made, then (they are dead by then) the digit
  // of every slot of the ordered tile, one byte each.
  __shared__ uint32_t cnt_raw[KG_WAVES * KG_BINS];
  __shared__ uint32_t gdelta[KG_BINS];
  __shared__ u64 scan_lds[KG_WAVES];
  __shared__ uint32_t tile_n;
  __shared__ u64 stage[GK_GROUP_TILE];  // the ordered tile: value bits, then ids
  static_assert(sizeof(cnt_raw) >= GK_GROUP_TILE, "one digit byte per slot fits the counters");
  uint32_t(*cnt)[KG_BINS] = (uint32_t(*)[KG_BINS])cnt_raw;
  unsigned char* slot_digit = (unsigned char*)cnt_raw;
  if (call[GK_KG_BAD]) return;
  const int64_t n = pass_n<FIRST>(count, call);
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  // (loaded ahead of its use: thread t combines digit t below)
  const uint32_t gbase = base[(size_t)threadIdx.x * (size_t)tiles + blockIdx.x];
#pragma unroll
  for (int k = 0; k < KG_WAVES; ++k) cnt[k][threadIdx.x] = 0;
  __syncthreads();
  const int64_t first = (int64_t)blockIdx.x * GK_GROUP_TILE + (int64_t)w * KG_WAVE_SPAN + lane;
  const u64 below = ((u64)1 << lane) - 1;
  int32_t id[KG_ITEMS];
  uint32_t rank[KG_ITEMS];  // among the wave's earlier samples with the same digit; then the slot
#pragma unroll
  for (int k = 0; k < KG_ITEMS; ++k) {
    const int64_t i = first + k * 64;
    int32_t v = -1;
    if (i < n) v = ids[i];
    id[k] = v;
  }
#pragma unroll
  for (int k = 0; k < KG_ITEMS; ++k) {
    const int32_t v = id[k];
    const bool valid = v >= 0;  // (later passes hold no negative id)
    const uint32_t d = ((uint32_t)v >> shift) & (KG_BINS - 1);
    // match mask: the valid lanes whose digit equals this lane's
    u64 m = __ballot(valid);
    for (int b = 0; b < nbits; ++b) {
      const bool bit = (d >> b) & 1;
      const u64 bb = __ballot(bit);
      m &= bit ? bb : ~bb;
    }
    rank[k] = 0;
    if (valid) {
      const uint32_t before = cnt[w][d];
      const uint32_t r = (uint32_t)__popcll(m & below);
      rank[k] = before + r;
      // the highest lane of the group advances the wave's counter: one writer
      // per digit and step, after every lane of the group has read it
      if (lane == 63 - __clzll(m)) cnt[w][d] = before + r + 1;
    }
  }
  __syncthreads();
  // Thread t owns digit t.  The tile's samples are first put in order in LDS
  // (digit, then wave, then rank: slot `excl + earlier waves + rank`), so that
  // the global writes of one digit are consecutive addresses; slot j of digit
  // d then goes to base[d] + (j - excl[d]).
  {
    uint32_t c[KG_WAVES], total = 0;
#pragma unroll
    for (int k = 0; k < KG_WAVES; ++k) {
      c[k] = cnt[k][threadIdx.x];
      total += c[k];
    }
    u64 all;
    const uint32_t excl = (uint32_t)block_exclusive((u64)total, scan_lds, &all);
    uint32_t run = excl;
#pragma unroll
    for (int k = 0; k < KG_WAVES; ++k) {
      cnt[k][threadIdx.x] = run;
      run += c[k];
    }
    gdelta[threadIdx.x] = gbase - excl;  // (mod 2^32)
    if (threadIdx.x == 0) tile_n = (uint32_t)all;
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < KG_ITEMS; ++k)
    if (id[k] >= 0) rank[k] += cnt[w][((uint32_t)id[k] >> shift) & (KG_BINS - 1)];
  __syncthreads();  // the counters are dead: their words become slot_digit
#pragma unroll
  for (int k = 0; k < KG_ITEMS; ++k) {
    if (id[k] >= 0) {
      stage[rank[k]] = (u64)__double_as_longlong(vals[first + k * 64]);
      slot_digit[rank[k]] = (unsigned char)(((uint32_t)id[k] >> shift) & (KG_BINS - 1));
    }
  }
  __syncthreads();
  const uint32_t kept = tile_n;
#pragma unroll
  for (int k = 0; k < KG_ITEMS; ++k) {
    const uint32_t j = (uint32_t)k * KG_THREADS + threadIdx.x;
    if (j < kept) out_vals[(size_t)(uint32_t)(gdelta[slot_digit[j]] + j)] = __longlong_as_double((long long)stage[j]);
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < KG_ITEMS; ++k)
    if (id[k] >= 0) stage[rank[k]] = (u64)(uint32_t)id[k];
  __syncthreads();
#pragma unroll
  for (int k = 0; k < KG_ITEMS; ++k) {
    const uint32_t j = (uint32_t)k * KG_THREADS + threadIdx.x;
    if (j < kept) out_ids[(size_t)(uint32_t)(gdelta[slot_digit[j]] + j)] = (int32_t)(uint32_t)stage[j];
  }
}

// out_offsets[s] = the number of kept samples with an id below s: the lower
// bound of s in the sorted ids (the last pass's id output), s in [0, S].  A
// void call leaves the zeros the launcher wrote.
__global__ __launch_bounds__(256) void k_group_offsets(const int32_t* __restrict__ sorted, const u64* __restrict__ call,
                                                       int64_t S, int64_t* __restrict__ out_offsets) {
  if (call[GK_KG_BAD]) return;
  const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (s > S) return;
  int64_t lo = 0, hi = (int64_t)call[GK_KG_KEPT];
  while (lo < hi) {
    const int64_t mid = lo + ((hi - lo) >> 1);
    if ((int64_t)sorted[mid] < s) lo = mid + 1;
    else hi = mid;
  }
  out_offsets[s] = lo;
}

// total_out (may be NULL): where the array's sum goes
template <typename T>
hipError_t scan_in_place(T* a, int64_t n, u64* sums, const u64* call, u64* total_out, hipStream_t s) {
  const int64_t nb = (n + SC_TILE - 1) / SC_TILE;
  if (nb <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_scan_sums<T>, dim3((unsigned)nb), dim3(SC_THREADS), 0, s, a, n, sums, call);
  hipLaunchKernelGGL(k_scan_mid, dim3(1), dim3(1024), 0, s, sums, nb, call, total_out);
  hipLaunchKernelGGL(k_scan_apply<T>, dim3((unsigned)nb), dim3(SC_THREADS), 0, s, a, n, sums, call);
  return hipGetLastError();
}

}  // namespace

hipError_t gk_launch_scan_i64(int64_t* a, int64_t n, unsigned long long* sums, hipStream_t stream) {
  return scan_in_place<int64_t>(a, n, sums, nullptr, nullptr, stream);
}

hipError_t gk_launch_scan_u32(uint32_t* a, int64_t n, unsigned long long* sums, const unsigned long long* skip,
                              unsigned long long* total_out, hipStream_t stream) {
  return scan_in_place<uint32_t>(a, n, sums, skip, total_out, stream);
}

int gk_group_passes(int64_t S) {
  int bits = 0;
  while (bits < 31 && ((int64_t)1 << bits) < S) ++bits;  // bits of S - 1
  const int p = (bits + KG_BITS - 1) / KG_BITS;
  return p < 1 ? 1 : p;  // (S == 1: one zero-bit pass, the filtered copy)
}

hipError_t gk_launch_group_by_key(const GKGroupScratch& sc, const int32_t* ids, const double* values, int64_t count,
                                  int64_t S, double* out_values, int64_t* out_offsets, hipStream_t s) {
  hipError_t e = hipMemsetAsync(out_offsets, 0, (size_t)(S + 1) * sizeof(int64_t), s);
  if (e != hipSuccess || count <= 0) return e;
  e = hipMemsetAsync(sc.call, 0, GK_KG_CALL_WORDS * sizeof(u64), s);
  if (e != hipSuccess) return e;
  const int passes = gk_group_passes(S);
  int bits = 0;
  while (bits < 31 && ((int64_t)1 << bits) < S) ++bits;
  const int64_t tiles = gk_group_tiles(count);
  const int32_t* in_ids = ids;
  const double* in_vals = values;
  for (int p = 0; p < passes; ++p) {
    const bool first = p == 0, last = p == passes - 1;
    const int shift = p * KG_BITS;
    const int nbits = bits - shift < KG_BITS ? (bits - shift < 0 ? 0 : bits - shift) : KG_BITS;
    int32_t* o_ids = sc.ids[p & 1];
    double* o_vals = last ? out_values : sc.vals[p & 1];
    if (first) {
      hipLaunchKernelGGL(k_group_tilehist<true>, dim3((unsigned)tiles), dim3(KG_THREADS), 0, s, in_ids, count, S,
                         sc.call, shift, sc.hist, tiles);
      hipLaunchKernelGGL(k_group_verdict, dim3(1), dim3(64), 0, s, ids, count, sc.call, sc.cum);
    } else {
      hipLaunchKernelGGL(k_group_tilehist<false>, dim3((unsigned)tiles), dim3(KG_THREADS), 0, s, in_ids, count, S,
                         sc.call, shift, sc.hist, tiles);
    }
    // (the first scan's total is the number of kept samples: the later passes' n)
    e = scan_in_place(sc.hist, tiles * KG_BINS, sc.sums, sc.call, first ? sc.call + GK_KG_KEPT : nullptr, s);
    if (e != hipSuccess) return e;
    if (first)
      hipLaunchKernelGGL(k_group_scatter<true>, dim3((unsigned)tiles), dim3(KG_THREADS), 0, s, in_ids, in_vals, count,
                         sc.call, shift, nbits, sc.hist, tiles, o_ids, o_vals);
    else
      hipLaunchKernelGGL(k_group_scatter<false>, dim3((unsigned)tiles), dim3(KG_THREADS), 0, s, in_ids, in_vals, count,
                         sc.call, shift, nbits, sc.hist, tiles, o_ids, o_vals);
    in_ids = o_ids;
    in_vals = o_vals;
  }
  hipLaunchKernelGGL(k_group_offsets, dim3((unsigned)((S + 1 + 255) / 256)), dim3(256), 0, s, in_ids, sc.call, S,
                     out_offsets);
  return hipGetLastError();
}
