// gk_dir.hip -- k_dir_*: the key directory behind gk_dir_assign / gk_dir_lookup
// / gk_dir_import (gfx950, wave64): a persistent, insert-only hash table from
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
//   k_dir_number  a first occurrence writes {size + rank, idle} into its
//                 slot's meta word and the key into key_of_id; an id >=
//                 capacity raises the overflow word instead.
//                 A call that met no unassigned slot -- every key known, the
//                 steady state -- leaves GK_DIR_CTL_IDLE set: k_dir_flag, the
//                 scan and k_dir_number then return at once.
//   k_dir_lookup  out_ids[i] = id of slot_of[i].  Without slot_of (gk_dir_lookup)
//                 the same kernel finds the slot with a read-only probe.
// gk_dir_import and the rebuild after a void call are k_dir_clear +
// k_dir_insert + k_dir_number with rank == NULL (id = i): a sample that is not
// its key's first occurrence is then a repeated key.
//
// Determinism.  Which slot a key lands in depends on which thread wins a CAS,
// but nothing the caller sees does: first[slot] is the MINIMUM sample index of
// the key (atomicMin, order-free), the rank is a scan over sample indices, so
// id = size + #{new keys whose first occurrence is earlier}: the loop of
// gk_capi.h.
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

// rank == NULL (import, rebuild): id = i, and a sample that is not its key's
// first occurrence is a repeat (GK_DIR_CTL_DUP: count minus the first such index).
// (A thread compares first[slot] with its own i while the first occurrence may
// be restoring the word: both values differ from every other thread's i.)
// (keys is key_of_id itself in a rebuild: no __restrict__)
__global__ __launch_bounds__(256) void k_dir_number(GKDirTable t, const int64_t* keys,
                                                    const uint32_t* __restrict__ slot_of,
                                                    const uint32_t* __restrict__ rank, int64_t count, int64_t size,
                                                    u64* __restrict__ ctl) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= count || (rank && ctl[GK_DIR_CTL_IDLE])) return;
  const uint32_t slot = slot_of[i];
  if (slot >= t.T) return;
  if (t.meta[slot].y != (uint32_t)i) {
    if (!rank) raise(ctl + GK_DIR_CTL_DUP, (u64)(count - i));
    return;
  }
  const int64_t id = rank ? size + (int64_t)rank[i] : i;
  if (id >= t.capacity) {
    raise(ctl + GK_DIR_CTL_OVF, 1);
    return;
  }
  t.meta[slot] = make_uint2((uint32_t)id, GK_DIR_NO_FIRST);
  t.key_of_id[id] = keys[i];
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
                                const uint32_t* rank, int64_t count, int64_t size, unsigned long long* ctl,
                                hipStream_t s) {
  if (count <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_dir_number, dim3(blocks_of(count, 256)), dim3(256), 0, s, t, keys, slot_of, rank, count, size,
                     ctl);
  return hipGetLastError();
}

hipError_t gk_launch_dir_lookup(const GKDirTable& t, const int64_t* keys, const uint32_t* slot_of, int64_t count,
                                int32_t* out_ids, hipStream_t s) {
  if (count <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_dir_lookup, dim3(blocks_of(count, 256)), dim3(256), 0, s, t, keys, slot_of, count, out_ids);
  return hipGetLastError();
}
