// gk_dir.hip -- k_dir_*: the key directory behind gk_dir_assign / gk_dir_lookup
// / gk_dir_remove / gk_dir_import (gfx950, wave64): a persistent hash table from
// int64 keys to int32 stream ids, open addressing with linear probing.
//
// Table (gk_dirhash.h: T slots, a power of two >= 2 * capacity): keys[T]
// (GK_DIR_NONE = empty) and meta[T] = {id, first}: the slot's id (-1 while
// unassigned) and its first-occurrence word (GK_DIR_NO_FIRST when idle).  The
// hash is gk_dir_mix, the finaliser of splitmix64; home slots come from
// GKDirHome (GK_DIR_HASH_BITS confines them for the tests).
//
// Kernels of one gk_dir_assign, in stream order; only kernel boundaries
// synchronise workgroups, and no thread ever waits on another one:
//   k_dir_insert  sample i probes from its key's home slot.  An empty slot is
//                 claimed with one 64-bit atomicCAS from GK_DIR_NONE to the
//                 key; the sentinel or the key itself coming back both mean
//                 "this is the key's slot".  The loop is bounded by T steps;
//                 running out of slots raises the overflow word.  On a slot
//                 whose id is unassigned, atomicMin(first, i).  The slot is
//                 kept per sample in scratch (slot_of[i]), not re-probed.
//   k_dir_flag    flag[i] = (first[slot_of[i]] == i): the sample is its key's
//                 first occurrence; the exclusive scan of the flags
//                 (gk_keyed.hip's k_scan_*) is the key's rank among the call's
//                 new keys, its total the number of new keys.
//   k_dir_number  a first occurrence writes {id, idle} into its slot's meta
//                 word and the key into key_of_id; id = free_ids[rank] while
//                 free ids last, then bound + rank - nfree.  A batch whose
//                 new keys pass the ids left writes nothing (void call).
//                 A call that met no unassigned slot -- every key known, the
//                 steady state -- leaves GK_DIR_CTL_IDLE set: k_dir_flag, the
//                 scan and k_dir_number then return at once.
//   k_dir_lookup  out_ids[i] = id of slot_of[i].  Without slot_of (gk_dir_lookup)
//                 the same kernel finds the slot with a read-only probe.
// gk_dir_import and the rebuild after a void call are k_dir_clear +
// k_dir_insert + k_dir_number with rank == NULL (id = i): a sample that is not
// its key's first occurrence is then a repeated key.
//
// gk_dir_remove is k_dir_remove_mark + k_dir_remove_release: a removed key
// stays in keys[slot] with its id unassigned, its own tombstone -- probes walk
// over it, lookup answers -1, and an assign of the same key finds the slot and
// numbers it as a new key.  No key value is reserved for it.  The ascending
// list of free ids is rebuilt after every remove (k_dir_free_flag, k_scan_*,
// k_dir_free_compact over the inverse array); assign consumes it from the front.
//
// Determinism.  Which slot a key lands in depends on which thread wins a CAS,
// but nothing the caller sees does: first[slot] is the MINIMUM sample index of
// the key (atomicMin, order-free), the rank is a scan over sample indices, so
// a new key's id is a function of #{new keys whose first occurrence is earlier}
// and of the sorted free ids: the loop of gk_capi.h.
//
// Contended keys.  Before any global access a workgroup matches equal keys in
// LDS: every sample hashes its key to one of DIR_CELLS cells and the lowest
// thread index wins the cell (ds_min).  A sample whose key equals its cell
// winner's does not probe: it takes the winner's slot, and the winner's i is
// the smaller one, so the atomicMin is the winner's alone.  A hot key costs
// one probe and one atomic per workgroup, not per sample.  Correctness does
// not rest on it: a sample that loses its cell to another key probes itself.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gk_launch.h"

namespace {

typedef unsigned long long u64;

constexpr int DIR_THREADS = 512;             // 8 waves: one LDS match per workgroup
constexpr int DIR_CELLS = 4 * DIR_THREADS;   // match cells (4 per sample)
constexpr u64 DIR_NONE = 0x8000000000000000ull;  // GK_DIR_NONE as stored

// word = max(word, v).  Control words only rise during a kernel, so a value
// read first, however stale, that already reaches v makes the atomic a no-op:
// a batch full of GK_DIR_NONE pays loads from L2, not atomics on one address.
__device__ __forceinline__ void raise(u64* word, u64 v) {
  if (__hip_atomic_load(word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < v) atomicMax(word, v);
}

// Claims or finds the slot of key k; GK_DIR_SLOT_FULL when T probes found neither.
__device__ __forceinline__ uint32_t probe_insert(u64* keys, uint32_t T, GKDirHome hm, u64 k) {
  uint32_t slot = gk_dir_home(hm, gk_dir_mix(k));
  for (uint32_t it = 0; it < T; ++it) {
    // (agent-scope load: a slot claimed by another CU in this kernel is seen at L2;
    // a stale GK_DIR_NONE would only send us to the CAS, which answers the truth)
    u64 cur = __hip_atomic_load(keys + slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (cur == DIR_NONE) {
      cur = atomicCAS(keys + slot, DIR_NONE, k);
      if (cur == DIR_NONE) return slot;
    }
    if (cur == k) return slot;
    slot = (slot + 1) & (T - 1);
  }
  return GK_DIR_SLOT_FULL;
}

// The slot of key k, GK_DIR_SLOT_NONE if the directory does not hold it.
__device__ __forceinline__ uint32_t probe_find(const u64* __restrict__ keys, uint32_t T, GKDirHome hm, u64 k) {
  uint32_t slot = gk_dir_home(hm, gk_dir_mix(k));
  for (uint32_t it = 0; it < T; ++it) {
    const u64 cur = keys[slot];
    if (cur == k) return slot;
    if (cur == DIR_NONE) break;
    slot = (slot + 1) & (T - 1);
  }
  return GK_DIR_SLOT_NONE;
}

__global__ __launch_bounds__(256) void k_dir_clear(GKDirTable t) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; s < (int64_t)t.T; s += stride) {
    t.keys[s] = DIR_NONE;
    t.meta[s] = make_uint2(0xFFFFFFFFu, GK_DIR_NO_FIRST);
  }
}

__global__ __launch_bounds__(DIR_THREADS) void k_dir_insert(GKDirTable t, const int64_t* __restrict__ keys,
                                                            int64_t count, uint32_t* __restrict__ slot_of,
                                                            u64* __restrict__ ctl) {
  __shared__ uint32_t cell[DIR_CELLS];
  __shared__ u64 skey[DIR_THREADS];
  __shared__ uint32_t sslot[DIR_THREADS];
  const int tid = threadIdx.x;
  const int64_t i = (int64_t)blockIdx.x * DIR_THREADS + tid;
  for (int c = tid; c < DIR_CELLS; c += DIR_THREADS) cell[c] = 0xFFFFFFFFu;
  const bool live = i < count;
  const u64 k = live ? (u64)keys[i] : DIR_NONE;
  const bool keyed = k != DIR_NONE;
  const uint32_t c = (uint32_t)(gk_dir_mix(k) >> 40) & (DIR_CELLS - 1);
  skey[tid] = k;
  __syncthreads();
  if (keyed) atomicMin(&cell[c], (uint32_t)tid);
  __syncthreads();
  const uint32_t w = keyed ? cell[c] : (uint32_t)tid;  // (w <= tid)
  const bool follows = keyed && w != (uint32_t)tid && skey[w] == k;
  uint32_t slot = GK_DIR_SLOT_NONE;
  if (keyed && !follows) {
    slot = probe_insert(t.keys, t.T, t.home, k);
    if (slot == GK_DIR_SLOT_FULL) {
      raise(ctl + GK_DIR_CTL_OVF, 1);
    } else if ((int32_t)t.meta[slot].x < 0) {
      // (the word only falls during this kernel: a value read here, however
      // stale, bounds it from above, so one that is already below i makes the
      // atomic a no-op.  Workgroups run roughly in index order, and a hot key's
      // later ones then pay a load from L2 instead of an atomic on one address.)
      uint32_t* first = &t.meta[slot].y;
      if (__hip_atomic_load(first, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > (uint32_t)i)
        atomicMin(first, (uint32_t)i);
      // the call has keys to number (every writer stores the same 0; read first, for the same reason)
      if (__hip_atomic_load(ctl + GK_DIR_CTL_IDLE, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0)
        __hip_atomic_store(ctl + GK_DIR_CTL_IDLE, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
  sslot[tid] = slot;
  __syncthreads();
  if (follows) slot = sslot[w];
  if (live) {
    slot_of[i] = slot;
    if (!keyed) raise(ctl + GK_DIR_CTL_NONE, (u64)(count - i));
  }
}

__global__ __launch_bounds__(256) void k_dir_flag(GKDirTable t, const uint32_t* __restrict__ slot_of, int64_t count,
                                                  uint32_t* __restrict__ flag, const u64* __restrict__ ctl) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= count || ctl[GK_DIR_CTL_IDLE]) return;
  const uint32_t slot = slot_of[i];
  flag[i] = slot < t.T && t.meta[slot].y == (uint32_t)i;
}

// rank == NULL (import, rebuild): id = i, a GK_DIR_NONE entry is a free id, and
// a sample that is not its key's first occurrence is a repeat (GK_DIR_CTL_DUP:
// count minus the first such index).
// rank != NULL (assign): the r-th new key takes free_ids[r], and bound + r -
// nfree once those run out.  The call is void when the table ran out of slots
// (k_dir_insert raised GK_DIR_CTL_OVF) or when the scan's total, on the device
// since the kernel before this one, passes the ids left; a void call writes
// NOTHING here: an id it numbered could be a free one below bound, and the
// rebuild that follows reads the inverse array.
// (A thread compares first[slot] with its own i while the first occurrence may
// be restoring the word: both values differ from every other thread's i.)
// (keys is key_of_id itself in a rebuild: no __restrict__)
__global__ __launch_bounds__(256) void k_dir_number(GKDirTable t, const int64_t* keys,
                                                    const uint32_t* __restrict__ slot_of,
                                                    const uint32_t* __restrict__ rank, int64_t count,
                                                    const int32_t* __restrict__ free_ids, int64_t nfree, int64_t bound,
                                                    u64* __restrict__ ctl) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= count) return;
  if (rank && (ctl[GK_DIR_CTL_IDLE] || ctl[GK_DIR_CTL_OVF] ||
               (int64_t)ctl[GK_DIR_CTL_NEW] > nfree + t.capacity - bound))
    return;
  const uint32_t slot = slot_of[i];
  if (slot >= t.T) {
    if (!rank && slot == GK_DIR_SLOT_NONE) t.key_of_id[i] = (int64_t)DIR_NONE;
    return;
  }
  if (t.meta[slot].y != (uint32_t)i) {
    if (!rank) raise(ctl + GK_DIR_CTL_DUP, (u64)(count - i));
    return;
  }
  int64_t id = i;
  if (rank) {
    const int64_t r = (int64_t)rank[i];
    id = r < nfree ? (int64_t)free_ids[r] : bound + r - nfree;
  }
  if (id >= t.capacity) {  // (import: count <= capacity; assign: checked above.  Never.)
    raise(ctl + GK_DIR_CTL_OVF, 1);
    return;
  }
  t.meta[slot] = make_uint2((uint32_t)id, GK_DIR_NO_FIRST);
  t.key_of_id[id] = keys[i];
}

// gk_dir_remove, first kernel: slot_of[i] = the slot of keys[i] if the key holds
// an id (GK_DIR_SLOT_NONE otherwise), and first[slot] = the minimum such i.
// (The first-occurrence word is idle between calls; it only falls during this
// kernel, so the read-before-atomic argument of k_dir_insert holds: a batch of
// one hot key pays loads from L2, not atomics on one address.)
__global__ __launch_bounds__(256) void k_dir_remove_mark(GKDirTable t, const int64_t* __restrict__ keys, int64_t count,
                                                         uint32_t* __restrict__ slot_of) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= count) return;
  const u64 k = (u64)keys[i];
  uint32_t slot = k == DIR_NONE ? GK_DIR_SLOT_NONE : probe_find(t.keys, t.T, t.home, k);
  if (slot < t.T) {
    if ((int32_t)t.meta[slot].x < 0) {
      slot = GK_DIR_SLOT_NONE;  // a removed key's slot
    } else {
      uint32_t* first = &t.meta[slot].y;
      if (__hip_atomic_load(first, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > (uint32_t)i)
        atomicMin(first, (uint32_t)i);
    }
  }
  slot_of[i] = slot;
}

// gk_dir_remove, second kernel: the first occurrence of a key releases it: its
// id goes to out_ids, the id's entry of the inverse array becomes GK_DIR_NONE
// and the slot goes back to "claimed, no id", the key staying in place as its
// own tombstone (the state k_dir_insert / k_dir_flag / k_dir_number / k_dir_lookup
// handle already).  Every other sample answers -1.  ctl[GK_DIR_CTL_NEW] += the
// keys removed, one atomic per workgroup.
// (A loser compares first[slot] with its own i while the winner may be
// restoring the word: the winner's i and the idle word both differ from it.)
__global__ __launch_bounds__(256) void k_dir_remove_release(GKDirTable t, const uint32_t* __restrict__ slot_of,
                                                            int64_t count, int32_t* __restrict__ out_ids,
                                                            u64* __restrict__ ctl) {
  __shared__ uint32_t removed;
  if (threadIdx.x == 0) removed = 0;
  __syncthreads();
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < count) {
    const uint32_t slot = slot_of[i];
    int32_t id = -1;
    if (slot < t.T && t.meta[slot].y == (uint32_t)i) {
      id = (int32_t)t.meta[slot].x;
      t.key_of_id[id] = (int64_t)DIR_NONE;
      t.meta[slot] = make_uint2(0xFFFFFFFFu, GK_DIR_NO_FIRST);
      atomicAdd(&removed, 1u);
    }
    out_ids[i] = id;
  }
  __syncthreads();
  if (threadIdx.x == 0 && removed) atomicAdd(ctl + GK_DIR_CTL_NEW, (u64)removed);
}

// The list of free ids, ascending: flag[id] = (no key holds id), for id in
// [0, bound); after the exclusive scan of the flags, free_ids[rank[id]] = id.
__global__ __launch_bounds__(256) void k_dir_free_flag(const int64_t* __restrict__ key_of_id, int64_t bound,
                                                       uint32_t* __restrict__ flag) {
  const int64_t id = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (id < bound) flag[id] = (u64)key_of_id[id] == DIR_NONE;
}

__global__ __launch_bounds__(256) void k_dir_free_compact(const int64_t* __restrict__ key_of_id, int64_t bound,
                                                          const uint32_t* __restrict__ rank,
                                                          int32_t* __restrict__ free_ids) {
  const int64_t id = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (id < bound && (u64)key_of_id[id] == DIR_NONE) free_ids[rank[id]] = (int32_t)id;
}

__global__ __launch_bounds__(256) void k_dir_lookup(GKDirTable t, const int64_t* __restrict__ keys,
                                                    const uint32_t* __restrict__ slot_of, int64_t count,
                                                    int32_t* __restrict__ out_ids) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= count) return;
  uint32_t slot;
  if (slot_of) {
    slot = slot_of[i];
  } else {
    const u64 k = (u64)keys[i];
    slot = k == DIR_NONE ? GK_DIR_SLOT_NONE : probe_find(t.keys, t.T, t.home, k);
  }
  out_ids[i] = slot < t.T ? (int32_t)t.meta[slot].x : -1;
}

inline unsigned blocks_of(int64_t n, int threads) { return (unsigned)((n + threads - 1) / threads); }

}  // namespace

hipError_t gk_launch_dir_clear(const GKDirTable& t, hipStream_t s) {
  const int64_t want = ((int64_t)t.T + 255) / 256;
  hipLaunchKernelGGL(k_dir_clear, dim3((unsigned)(want < 65536 ? want : 65536)), dim3(256), 0, s, t);
  return hipGetLastError();
}

hipError_t gk_launch_dir_insert(const GKDirTable& t, const int64_t* keys, int64_t count, uint32_t* slot_of,
                                unsigned long long* ctl, hipStream_t s) {
  if (count <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_dir_insert, dim3(blocks_of(count, DIR_THREADS)), dim3(DIR_THREADS), 0, s, t, keys, count,
                     slot_of, ctl);
  return hipGetLastError();
}

hipError_t gk_launch_dir_flag(const GKDirTable& t, const uint32_t* slot_of, int64_t count, uint32_t* flag,
                              const unsigned long long* ctl, hipStream_t s) {
  if (count <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_dir_flag, dim3(blocks_of(count, 256)), dim3(256), 0, s, t, slot_of, count, flag, ctl);
  return hipGetLastError();
}

hipError_t gk_launch_dir_number(const GKDirTable& t, const int64_t* keys, const uint32_t* slot_of,
                                const uint32_t* rank, int64_t count, const int32_t* free_ids, int64_t nfree,
                                int64_t bound, unsigned long long* ctl, hipStream_t s) {
  if (count <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_dir_number, dim3(blocks_of(count, 256)), dim3(256), 0, s, t, keys, slot_of, rank, count,
                     free_ids, nfree, bound, ctl);
  return hipGetLastError();
}

hipError_t gk_launch_dir_remove(const GKDirTable& t, const int64_t* keys, int64_t count, uint32_t* slot_of,
                                int32_t* out_ids, unsigned long long* ctl, hipStream_t s) {
  if (count <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_dir_remove_mark, dim3(blocks_of(count, 256)), dim3(256), 0, s, t, keys, count, slot_of);
  hipLaunchKernelGGL(k_dir_remove_release, dim3(blocks_of(count, 256)), dim3(256), 0, s, t, slot_of, count, out_ids,
                     ctl);
  return hipGetLastError();
}

hipError_t gk_launch_dir_free_list(const GKDirTable& t, int64_t bound, uint32_t* flag, unsigned long long* sums,
                                   int32_t* free_ids, unsigned long long* total_out, hipStream_t s) {
  if (bound <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_dir_free_flag, dim3(blocks_of(bound, 256)), dim3(256), 0, s, t.key_of_id, bound, flag);
  hipError_t e = gk_launch_scan_u32(flag, bound, sums, nullptr, total_out, s);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_dir_free_compact, dim3(blocks_of(bound, 256)), dim3(256), 0, s, t.key_of_id, bound, flag,
                     free_ids);
  return hipGetLastError();
}

hipError_t gk_launch_dir_lookup(const GKDirTable& t, const int64_t* keys, const uint32_t* slot_of, int64_t count,
                                int32_t* out_ids, hipStream_t s) {
  if (count <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_dir_lookup, dim3(blocks_of(count, 256)), dim3(256), 0, s, t, keys, slot_of, count, out_ids);
  return hipGetLastError();
}
