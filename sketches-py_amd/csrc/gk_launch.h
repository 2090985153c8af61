// gk_launch.h -- host-side launchers of the HIP kernels (the gk_*.hip units),
// used by the C ABI runtime (gk_capi.cpp).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "gk_dirhash.h"
#include "gk_state.h"

// Capacity of the fast LDS class (every stream starts there when P <= 128).
#ifndef GK_SMALL_CAP
#define GK_SMALL_CAP 128
#endif

// optional query fused into an ingest/flush launch (gk:187-232 after the flush)
struct GKQuery {
  const double* qs = nullptr;  // device, nq values (NULL: no query)
  int nq = 0;
  double* out = nullptr;       // device [S * nq]
  int mode = 0;                // 0 quantiles() list semantics, 1 quantile() per q
};

int gk_num_cu();
// the device has CUs to spare for k_long_prep beside an early k_ingest_wg grid
int gk_wg_early_ok();
size_t gk_ingest_ws_bytes(int cap, int vpl);
// k_ingest_big (any capacity, any flush period): bytes of one block's workspace
size_t gk_big_ws_bytes(int cap, int P);
#define GK_WORK_BYTES 2048  // 8 hand-out counters + 8 stats-role batch counters, one 128-byte line each
// the set's counter block and the classes' lists (GK_CTR_* below)
struct GKPoolDev {
  int32_t* ctr;
  int32_t* rcnt;  // this round's re-run list lengths (one per class)
  int32_t* list[GK_MAX_CLASSES];
  int32_t* rerun[GK_MAX_CLASSES];
  int32_t* defer;  // S entries
};
// What every launch of one ingest / flush call shares
struct GKBatch {
  const double* x = nullptr;      // the batch: offs = S + 1 offsets into x (x NULL: flush only, zero offsets)
  const int64_t* offs = nullptr;
  int force = 0;  // flush mode: 0 automatic flushes only, 1 also the pending rest, 2 merge_compress() of every stream
  GKQuery q;
};
// One ingest / flush launch of one capacity class: the host fills this struct
// (gk_capi.cpp launch_class) and the launchers unpack it at the kernel launch.
struct GKIngestLaunch : GKBatch {
  // list/count (host count) or list/count_ptr (device count): the streams of a class-lcls launch
  // (list NULL: every stream, class 0); listed streams no longer in class lcls are skipped.
  const int32_t* list = nullptr;
  int64_t count = 0;
  const int32_t* count_ptr = nullptr;
  int lcls = 0;
  // cap GK_SMALL_CAP / 2048: LDS kernels; any other cap: global workspace ws (ws_bytes per block, ws_blocks
  // blocks).  The unbounded class (k_ingest_big: tables beyond 32768 entries; every class when P > 1024):
  // one wave per stream over ws, ws_bytes >= gk_big_ws_bytes(cap, P).
  int cap = 0;
  int vpl = 0;  // (k_ingest_big ignores it)
  unsigned char* ws = nullptr;
  size_t ws_bytes = 0;
  int64_t ws_blocks = 0;
  // the streams that outgrew the class
  int32_t* ovf_count = nullptr;
  int32_t* ovf_list = nullptr;
  // device counters of the launch's dynamic stream hand-out, ZEROED BY THE
  // CALLER (GK_WORK_BYTES for the small-class launch, 8 bytes for the others;
  // gk_capi.cpp zeroes every counter of a call with one memset, GK_CALL_* below)
  unsigned long long* work = nullptr;
  // prio / prio_count (device, may be NULL): streams handed out first by the
  // capacity-class kernels (the long streams of the batch, longest first);
  // psort / prio_ws: their presorted flush batches (GKPresort), or NULL;
  // prio_skip: the head of that list k_ingest_wg takes (the launch skips it).
  // For gk_launch_ingest_wg: list = the long list, count_ptr = its stream count.
  const int32_t* prio = nullptr;
  const int32_t* prio_count = nullptr;
  const double* psort = nullptr;
  const int64_t* prio_ws = nullptr;
  const int32_t* prio_skip = nullptr;
  // > 0: the small-class batch launch (x given, no list) also walks the
  // gk:52-59 stats of every stream of at most GK_STATS_LONG values, in that
  // many eighths of a wave per CU (then requires the lengths-only k_lengths before)
  int fused_stats = 0;
  // the small-class launch records them as part of its dispatch (hipExtLaunchKernel, the kernel's own
  // start and end) instead of two marker packets around it; other classes ignore them
  hipEvent_t ev_start = nullptr;
  hipEvent_t ev_stop = nullptr;
  // the promotion rounds' fused steps (k_ingest's pmode); pmode != 0 needs pool
  const GKPoolDev* pool = nullptr;
  int pmode = 0;
  // k_ingest_big only: the set's GK_CTR_* counters (GK_CTR_FATAL: per-stream count limit)
  int32_t* ctr = nullptr;
};
hipError_t gk_launch_ingest(const GKState& st, const GKIngestLaunch& a, hipStream_t stream);
hipError_t gk_launch_ingest_big(const GKState& st, const GKIngestLaunch& a, hipStream_t stream);
// k_stats over every stream; streams longer than GK_STATS_LONG values are put
// on long_list (S entries), sorted longest first, with their pre-call n in
// long_n, for gk_launch_stats_long, which may run on another HIP stream beside
// the ingest launches (it writes only _min/_max/_sum/_avg of listed streams).
// Presort of the long streams' automatic-flush batches (sets whose class 0 is
// a capacity-class kernel): per list slot the workspace offset (-1: none)
// and first global batch, the workspace (ws_cap doubles) and the size this
// call needed (host grows the workspace from it after the call).
struct GKPresort {
  int64_t* list_ws = nullptr;  // [S]
  int64_t* list_b0 = nullptr;  // [S + 1]
  double* ws = nullptr;
  int64_t ws_cap = 0;
  int64_t* ws_need = nullptr;  // device, 1 value
  int32_t* wg_count = nullptr; // device, 1 value: k_ingest_wg's streams (the head of the long list); NULL: none
  int wg_presort = 1;          // with wg_count: presort as without it (1) or nothing (0: k_ingest_wg ranks)
  int32_t* done = nullptr;     // device, 1 value: k_presort_reg's finished waves (k_ingest_wg runs beside
                               // the presort and takes presorted batches once all are done); NULL: after it
};
// one workgroup per stream for the first *a.count_ptr streams of the long list
// a.list (class lcls = 0 of the 2048 class only); the prio k_ingest launch
// skips them.  go (device, may be NULL): the word the workgroups wait for
// before they start their streams (k_long_prep sets it)
hipError_t gk_launch_ingest_wg(const GKState& st, const GKIngestLaunch& a, const GKPresort& ps, const int32_t* go,
                               hipStream_t stream);
// the long-stream list + every stream's pre-call n (k_lengths)
hipError_t gk_launch_stats(const GKState& st, const int64_t* offs, int32_t* long_list, int32_t* long_count,
                           hipStream_t stream);
// the long list sorted longest first, the listed streams' pre-call n, the
// presort plan and k_ingest_wg's stream count (k_long_prep)
hipError_t gk_launch_long_prep(const GKState& st, const int64_t* offs, int32_t* long_list, int64_t* long_n,
                               int32_t* long_count, const GKPresort& ps, hipStream_t stream, int32_t* go = nullptr);
// gk:52-59 chains of the streams up to GK_STATS_LONG values (k_stats_short; the
// long ones are k_stats_long's), when class 0 is not the small class
hipError_t gk_launch_stats_short(const GKState& st, const double* x, const int64_t* offs, hipStream_t stream);
// the presort (k_presort_reg) over the plan k_long_prep wrote (no-op without
// a workspace), and its grid (waves); k_ingest_wg compares *ps.done with it
int gk_presort_reg_grid(const GKState& st);
hipError_t gk_launch_presort(const GKState& st, const double* x, const int64_t* offs, const int32_t* long_list,
                             const int64_t* long_n, const int32_t* long_count, const GKPresort& ps,
                             hipStream_t stream);
hipError_t gk_launch_stats_long(const GKState& st, const double* x, const int64_t* offs, const int32_t* long_list,
                                const int64_t* long_n, const int32_t* long_count, hipStream_t stream);
// quantiles of the listed streams from their committed tables (after the
// join); qfix: also resolve the _min/_max markers of a small-class launch
// that carried the stats role (every stream's answers)
hipError_t gk_launch_query_list(const GKState& st, const int32_t* list, const int32_t* count, const GKQuery& q,
                                bool qfix, hipStream_t stream);
size_t gk_merge_lds_bytes(int cap, int pmax);
// k_fold: dst[j].merge(...) over the steps of destination j, one wave per
// destination with its table on chip across the steps (gk:111-154 per step).
// The host fills this struct and the kernel takes it as it is.
//  * goffs given (roll-up): the steps are src[members[k]], k in [goffs[j],
//    goffs[j+1]); an empty group leaves j untouched.  One block per destination.
//  * goffs NULL: the one step src[j] (gk_merge), or with eoffs given the
//    caller's records ev/eg/ed[eoffs[j] .. eoffs[j+1]) (merge_compress(entries),
//    gk:63-109; src is not read).  num_cu * 8 blocks; progress may be NULL.
// A step that does not fit `cap` ends the fold there: the state after the step
// before it is committed (nothing when it was the first), its position goes to
// progress[j] and j to the overflow list; resume = 1 starts each listed
// destination at progress[j].
struct FoldArgs {
  GKState dst;
  GKState src;             // its members already flushed (gk:126 / gk:137)
  const int64_t* goffs;    // device [G + 1], or NULL
  const int64_t* members;  // device [goffs[G]] streams of src, each at most once
  int64_t* progress;       // device [G] position of the first step not yet merged (listed destinations)
  int resume;              // 0: start at goffs[j]; 1: at progress[j]
  const double* ev;        // explicit records (v, g, d) in CSR by eoffs (NULL: none)
  const int32_t* eg;
  const int32_t* ed;
  const int64_t* eoffs;
  int cap;                 // capacity of the carve for tables / records
  const int32_t* list;     // destinations to process (NULL = all)
  int64_t count;
  int32_t* ovf_count;
  int32_t* ovf_list;
  unsigned char* ws;  // global workspace for capacities beyond LDS (NULL = LDS)
  size_t ws_bytes;    // per block
  int64_t ws_blocks;
};
hipError_t gk_launch_fold(const FoldArgs& a, hipStream_t stream);
// roll-up argument checks into *bad (zeroed by the caller): bit 0 offsets not
// starting at 0 or decreasing, bit 1 a member outside [0, S), bit 2 a source
// stream listed twice (bitmap: (S + 31) / 32 zeroed words)
hipError_t gk_launch_rollup_check_offsets(const int64_t* goffs, int64_t G, int32_t* bad, hipStream_t stream);
hipError_t gk_launch_rollup_check_members(const int64_t* members, int64_t M, int64_t S, uint32_t* bitmap, int32_t* bad,
                                          hipStream_t stream);
// the members with n != 0 (those the reference flushes) into list, *count of them (zeroed by the caller)
hipError_t gk_launch_rollup_flush_list(const GKState& src, const int64_t* members, int64_t M, int32_t* count,
                                       int32_t* list, hipStream_t stream);
// ---- per-stream selection (gk_*_select): ids = `count` stream ids (device) ----
// Control words of k_select_check (zeroed by the caller with the bitmap):
#define GK_SEL_BAD 0    // an id outside [0, S)
#define GK_SEL_FIRST 1  // max of (count - index) over them: count minus the first bad index
#define GK_SEL_COUNT 2  // entries of the flush list
#define GK_SEL_WORDS 4
// the id check and, list != NULL, the listed streams with n > 0 and pending
// values into list, each once (bitmap: (S + 31) / 32 zeroed words; list: room
// for min(count, S) entries).  Mutates no stream state.
hipError_t gk_launch_select_check(const GKState& st, const int32_t* ids, int64_t count, int32_t* ctl, uint32_t* bitmap,
                                  int32_t* list, hipStream_t stream);
// q.out[k * nq ..] = the quantiles of stream ids[k] from its committed table
hipError_t gk_launch_select_query(const GKState& st, const int32_t* ids, int64_t count, const GKQuery& q,
                                  hipStream_t stream);
// rank bounds (gk_ranks / gk_ranks_select): lo / hi[k * nx ..] = the bounds of
// stream ids[k] (ids == NULL: of stream k, count == S) for the thresholds
// xs[0 .. nx) (device), from its committed table; lo or hi may be NULL
hipError_t gk_launch_rank(const GKState& st, const int32_t* ids, int64_t count, const double* xs, int nx, int64_t* lo,
                          int64_t* hi, hipStream_t stream);
// the listed streams back to empty sketches; class and slot stay as they are
hipError_t gk_launch_select_reset(const GKState& st, const int32_t* ids, int64_t count, hipStream_t stream);
// gk_stats' arrays gathered at ids (device arrays of `count` entries, any may be NULL)
struct GKSelectStats {
  int64_t* n;
  double* mn;
  double* mx;
  double* sum;
  double* avg;
  int32_t* table_size;
  int32_t* pending;
};
hipError_t gk_launch_select_stats(const GKState& st, const int32_t* ids, int64_t count, const GKSelectStats& o,
                                  hipStream_t stream);
// ---- stream transfer (gk_pack_select / gk_unpack_select): listed streams to
// and from a GKPACK01 buffer (gk_pack.h); row k of the buffer = stream ids[k] ----
// Exclusive scan in place of n non-negative int64 values (gk_keyed.hip's
// k_scan_sums / k_scan_mid / k_scan_apply); sums: gk_scan_sums(n) words.
inline int64_t gk_scan_sums(int64_t n) { return (n + 2047) / 2048; }
hipError_t gk_launch_scan_i64(int64_t* a, int64_t n, unsigned long long* sums, hipStream_t stream);
// totals[0] += the rows' table sizes, totals[1] += their pending counts (zeroed
// by the caller); eoffs != NULL: the sizes as int64 into eoffs / poffs[0 .. count)
// and a 0 into [count] (count + 1 entries each), for the scan above
hipError_t gk_launch_pack_sizes(const GKState& st, const int32_t* ids, int64_t count, int64_t* eoffs, int64_t* poffs,
                                unsigned long long* totals, hipStream_t stream);
// tables to v / g / d at eoffs[k], pending values to pv at poffs[k] (k_pack_select)
hipError_t gk_launch_pack_select(const GKState& st, const int32_t* ids, int64_t count, const int64_t* eoffs,
                                 const int64_t* poffs, double* v, int32_t* g, int32_t* d, double* pv,
                                 hipStream_t stream);
// the sections of a packed buffer (device) and its header's totals
struct GKPacked {
  const int64_t* n;
  const double* mn;
  const double* mx;
  const double* sum;
  const double* avg;
  const int64_t* eoffs;
  const int64_t* poffs;
  const double* v;
  const int32_t* g;
  const int32_t* d;
  const double* pv;
  int64_t E, P;
};
// Control words of k_unpack_check (zeroed by the caller with the bitmap):
#define GK_UNP_BAD 0    // bit 1 an id outside [0, S), 2 an id listed twice, 4 offsets not monotone, 8 pending rule
#define GK_UNP_FIRST 1  // count minus the first bad index (as GK_SEL_FIRST)
#define GK_UNP_MAXE 2   // the largest table of the buffer
#define GK_UNP_STUCK 3  // k_unpack_select: rows that found no class (none after a successful check)
#define GK_UNP_NEED 4   // [4 + t]: rows that move to class t (t = 1 .. GK_MAX_CLASSES - 1)
#define GK_UNP_WORDS 8
static_assert(GK_UNP_NEED + GK_MAX_CLASSES <= GK_UNP_WORDS, "one need count per class");
// every device-side refusal of gk_unpack_select in one pass that mutates
// nothing (bitmap: (S + 31) / 32 zeroed words)
hipError_t gk_launch_unpack_check(const GKState& st, const int32_t* ids, int64_t count, const GKPacked& pk,
                                  int32_t* ctl, uint32_t* bitmap, hipStream_t stream);
// overflow lists of k_unpack_select by the class t a row moves to: count[t]
// rows, their stream ids in list[t] (k_promote_dev's input) and the rows
// themselves in rows[t], same positions; stuck: ctl + GK_UNP_STUCK
struct GKUnpackOvf {
  int32_t* count;
  int32_t* list[GK_MAX_CLASSES];
  int32_t* rows[GK_MAX_CLASSES];
  int32_t* stuck;
};
// installs the rows that fit their stream's class (table, pending values and
// header words in one pass); rows NULL: every row of the buffer (nrows = count),
// the others go to `ov`; rows given: those rows (after their promotion)
hipError_t gk_launch_unpack_select(const GKState& st, const int32_t* ids, const int32_t* rows, int64_t nrows,
                                   const GKPacked& pk, const GKUnpackOvf& ov, hipStream_t stream);
// ---- keyed ingest (gk_keyed.hip): stable group-by of (id, value) samples ----
// An LSD radix partition by stream id, GK_GROUP_BITS per pass over tiles of
// GK_GROUP_TILE samples (one workgroup each).  The set owns the scratch:
struct GKGroupScratch {
  int32_t* ids[2] = {};   // ping-pong pair buffers, `count` entries each: pass p writes ids[p & 1]
  double* vals[2] = {};   //   and (not the last pass, which writes the caller's values) vals[p & 1]
  uint32_t* hist = nullptr;            // [2^GK_GROUP_BITS][tiles] digit counts, scanned in place
  unsigned long long* sums = nullptr;  // tile sums of the scan (gk_group_sums entries)
  unsigned long long* call = nullptr;  // GK_KG_CALL_WORDS words of this call (zeroed by the launcher)
  unsigned long long* cum = nullptr;   // cumulative: [0] calls voided by an id >= S, [1] the last one's
                                       //   first bad sample index, [2] its id
};
#define GK_GROUP_BITS 8
#define GK_GROUP_TILE 4096
#define GK_GROUP_SCAN_TILE 2048
static_assert(GK_GROUP_SCAN_TILE == 2048, "gk_scan_sums counts tiles of 2048");
#define GK_KG_BAD 0     // ids >= S in this call
#define GK_KG_BADKEY 1  // max of (count - index) over them
#define GK_KG_KEPT 2    // samples with an id in [0, S)
#define GK_KG_CALL_WORDS 4
#define GK_KG_CUM_WORDS 3
int gk_group_passes(int64_t S);  // ceil(bits(S - 1) / GK_GROUP_BITS), at least 1
inline int64_t gk_group_tiles(int64_t count) { return (count + GK_GROUP_TILE - 1) / GK_GROUP_TILE; }
inline int64_t gk_group_sums(int64_t count) {
  return ((gk_group_tiles(count) << GK_GROUP_BITS) + GK_GROUP_SCAN_TILE - 1) / GK_GROUP_SCAN_TILE;
}
// out_offsets (int64[S + 1]) and out_values (count doubles) from ids / values
// (count samples, 0 <= count < 2^31); every kernel of a call that met an
// id >= S leaves its outputs alone, except that out_offsets becomes all zero.
hipError_t gk_launch_group_by_key(const GKGroupScratch& sc, const int32_t* ids, const double* values, int64_t count,
                                  int64_t S, double* out_values, int64_t* out_offsets, hipStream_t stream);
// ---- keyed rank queries (gk_rankkeyed.hip): bounds per (stream id, value) sample ----
// k_rank_keyed_check over the samples, mutating no stream state: ctl as
// k_select_check's (GK_SEL_*; zeroed by the caller with the bitmap) -- GK_SEL_BAD
// for an id >= S or a NaN xs[i] on a row with id >= 0, GK_SEL_FIRST count minus
// the first such index; negative ids pass; the occurring streams with n > 0 and
// pending values into list, each once.  payload[i] = the int64 i, bit-cast:
// what the group-by carries beside ids[i].
hipError_t gk_launch_rank_keyed_check(const GKState& st, const int32_t* ids, const double* xs, int64_t count,
                                      int32_t* ctl, uint32_t* bitmap, int32_t* list, double* payload,
                                      hipStream_t stream);
// k_rank_keyed: gidx / goffs = gk_launch_group_by_key's outputs for (ids,
// payload); row i of lo / hi / n (any may be NULL) = the rank bounds of xs[i]
// in stream ids[i] and its n, zeros for a negative id.  One wave per `chunk`
// grouped samples (a multiple of 64).
#define GK_RANKK_CHUNK_DEFAULT 1024
hipError_t gk_launch_rank_keyed(const GKState& st, const int32_t* ids, const double* xs, int64_t count,
                                const double* gidx, const int64_t* goffs, int chunk, int64_t* lo, int64_t* hi,
                                int64_t* n, hipStream_t stream);
// ---- keyed score-and-ingest (gk_rankingest.hip) ----
// k_rank_ingest_keyed: k_rank_keyed, and gvals[p] = xs[gidx[p]] (bit for bit)
// for every grouped position p < goffs[S] -- the grouped values, in arrival
// order per stream: (gvals, goffs) is the CSR batch of the samples.  gvals has
// room for `count` doubles and is none of the other buffers.  lo, hi and n may
// all be NULL: only gvals is written then.
hipError_t gk_launch_rank_ingest_keyed(const GKState& st, const int32_t* ids, const double* xs, int64_t count,
                                       const double* gidx, const int64_t* goffs, int chunk, int64_t* lo, int64_t* hi,
                                       int64_t* n, double* gvals, hipStream_t stream);
// ---- key directory (gk_dir.hip): int64 keys -> int32 ids, a device hash table ----
// Exclusive scan in place of n uint32 values whose sum stays below 2^32 (the
// same k_scan_* kernels); *total_out (device, may be NULL) = the sum.  skip
// (device, may be NULL): a non-zero word makes the scan do nothing.
hipError_t gk_launch_scan_u32(uint32_t* a, int64_t n, unsigned long long* sums, const unsigned long long* skip,
                              unsigned long long* total_out, hipStream_t stream);
struct GKDirTable {
  unsigned long long* keys;  // [T] GK_DIR_NONE = empty
  uint2* meta;               // [T] x: id (0xFFFFFFFF unassigned), y: first-occurrence word
  int64_t* key_of_id;        // [capacity]
  uint32_t T;                // slots, a power of two (gk_dir_slots)
  int64_t capacity;
  GKDirHome home;
};
#define GK_DIR_NO_FIRST 0xFFFFFFFFu    // idle first-occurrence word (sample indices are < 2^31)
#define GK_DIR_SLOT_NONE 0xFFFFFFFFu   // slot_of: GK_DIR_NONE sample / unknown key
#define GK_DIR_SLOT_FULL 0xFFFFFFFEu   // slot_of: the probe ran out of slots
// Control words of a directory call (zeroed by the caller, but for the last):
#define GK_DIR_CTL_OVF 0    // the table or the id space ran out
#define GK_DIR_CTL_NEW 1    // the scan's total: keys added by this call (gk_dir_remove: keys removed)
#define GK_DIR_CTL_NONE 2   // count minus the first index of a GK_DIR_NONE key (as GK_SEL_FIRST)
#define GK_DIR_CTL_DUP 3    // import: count minus the first index of a repeated key
#define GK_DIR_CTL_IDLE 4   // SET by the caller, cleared by k_dir_insert on meeting a slot without an id:
                            //   while set, k_dir_flag, the scan and k_dir_number (assign) return at once
#define GK_DIR_CTL_WORDS 5
// every slot empty, unassigned and idle
hipError_t gk_launch_dir_clear(const GKDirTable& t, hipStream_t stream);
// slot_of[i] = the slot of keys[i], claimed if the key is new; first-occurrence words of unassigned slots
hipError_t gk_launch_dir_insert(const GKDirTable& t, const int64_t* keys, int64_t count, uint32_t* slot_of,
                                unsigned long long* ctl, hipStream_t stream);
// flag[i] = sample i is the first occurrence of a key without an id
hipError_t gk_launch_dir_flag(const GKDirTable& t, const uint32_t* slot_of, int64_t count, uint32_t* flag,
                              const unsigned long long* ctl, hipStream_t stream);
// first occurrences take id = free_ids[rank[i]] while rank[i] < nfree, then bound + rank[i] - nfree; nothing is
// written when GK_DIR_CTL_OVF is set or GK_DIR_CTL_NEW passes nfree + capacity - bound (void call).
// rank NULL: id = i, a GK_DIR_NONE entry leaves GK_DIR_NONE in key_of_id[i], and any other sample is a repeat
hipError_t gk_launch_dir_number(const GKDirTable& t, const int64_t* keys, const uint32_t* slot_of,
                                const uint32_t* rank, int64_t count, const int32_t* free_ids, int64_t nfree,
                                int64_t bound, unsigned long long* ctl, hipStream_t stream);
// gk_dir_remove: out_ids[i] = the id keys[i] held, if sample i is the first of its key in the batch, else -1;
// the key's slot loses its id, key_of_id[id] = GK_DIR_NONE; ctl[GK_DIR_CTL_NEW] (zeroed by the caller) += keys removed
hipError_t gk_launch_dir_remove(const GKDirTable& t, const int64_t* keys, int64_t count, uint32_t* slot_of,
                                int32_t* out_ids, unsigned long long* ctl, hipStream_t stream);
// free_ids[0 ..) = the ids of [0, bound) that no key holds, ascending; *total_out (device, may be NULL) = how many.
// flag: bound words, sums: gk_scan_sums(bound) words of scratch
hipError_t gk_launch_dir_free_list(const GKDirTable& t, int64_t bound, uint32_t* flag, unsigned long long* sums,
                                   int32_t* free_ids, unsigned long long* total_out, hipStream_t stream);
// out_ids[i] = id of slot_of[i], or (slot_of NULL) of keys[i] by a read-only probe; -1 if none
hipError_t gk_launch_dir_lookup(const GKDirTable& t, const int64_t* keys, const uint32_t* slot_of, int64_t count,
                                int32_t* out_ids, hipStream_t stream);
// every stream back to an empty sketch in class 0; ctr: also zero the set's
// counter words [0, GK_CTR_FATAL) (slots used, member-list lengths) and the
// per-call block [GK_CTR_CALL, GK_CALL_BYTES) (what begin_call's memset zeroes)
hipError_t gk_launch_reset(const GKState& st, hipStream_t stream, int32_t* ctr = nullptr);
// fills st.rtab (reciprocals 1.0/k, k < st.rtab_n)
hipError_t gk_launch_rtab(const GKState& st, hipStream_t stream);
hipError_t gk_launch_export(const GKState& st, const int64_t* offs, double* v, int32_t* g, int32_t* d,
                            hipStream_t stream);
hipError_t gk_launch_export_pending(const GKState& st, const int64_t* offs, double* v, hipStream_t stream);
// counts into *bad the streams whose pending count p is not one add() can leave (p > n mod P)
hipError_t gk_launch_check_pending(int64_t S, int P, const int64_t* n, const int64_t* poffs, int32_t* bad,
                                  hipStream_t stream);
hipError_t gk_launch_import(const GKState& st, const int64_t* offs, const double* v, const int32_t* g,
                            const int32_t* d, const int64_t* poffs, const double* pv, int32_t* ovf_count,
                            int32_t* ovf_list, hipStream_t stream);
hipError_t gk_launch_promote(const GKState& st, const int32_t* list, int64_t count, const int32_t* slots, int ncls,
                             hipStream_t stream);

// Device-side capacity-class bookkeeping: counters (slots used, member list
// lengths, re-run list lengths, streams that found no class / slot) and, per
// class c > 0, its member list and this round's re-run list (S entries each).
// Layout of the set's counter block (int32 words; one allocation):
//   persistent:  [0..3] slots used per class, [4..7] member-list lengths,
//                [12] streams with no class left, [13] the largest such id
//   per call (zeroed by ONE memset at the start of every call, from word
//   GK_CTR_CALL -- 16, a 64-byte boundary: one fill -- to GK_CALL_BYTES):
//   [16] deferred streams, [17] long-stream list length, [20 + 4r + c] round
//   r's re-run list length of class c, [40 + r] round r's overflow count,
//   then (byte GK_CALL_WORK) the launches' stream hand-out counters.
// The host reads words [0, GK_CTR_WORDS) back after every call.
#define GK_CTR_USED 0
#define GK_CTR_LCNT 4
#define GK_CTR_FATAL 12   // [12] count, [13] largest such stream id
#define GK_CTR_DEFER 16   // streams whose class had no free slot this call (re-run by the host later)
#define GK_CTR_LONG 17    // streams longer than GK_STATS_LONG values (k_stats)
#define GK_CTR_RCNT 20    // [20 + 4*round + class]
#define GK_CTR_OVFC 40    // [40 + round]
#define GK_CTR_BADPEND 48 // gk_import: streams with an unreachable pending count
#define GK_CTR_WG 50      // k_ingest_wg's stream count this call (k_long_prep)
#define GK_CTR_WGGO 53    // k_long_prep done: k_ingest_wg, launched ahead of it, starts its streams
#define GK_CTR_PSDONE 51  // k_presort_reg's finished waves this call (k_ingest_wg beside it)
#define GK_CTR_WORDS 18
#define GK_CTR_CALL 16
#define GK_CALL_WORK 256                          // bytes: the small-class launch's GK_WORK_BYTES, then
#define GK_CALL_SLOTS 16                          //   16 counters of 128 bytes for the other launches
#define GK_CALL_BYTES (GK_CALL_WORK + GK_WORK_BYTES + GK_CALL_SLOTS * 128)
static_assert(GK_CTR_RCNT + 4 * (GK_MAX_CLASSES + 1) <= GK_CTR_OVFC, "re-run counts fit below the overflow counts");
static_assert(GK_CTR_PSDONE < GK_CALL_WORK / 4, "counters fit below the hand-out block");
static_assert((GK_CTR_CALL * 4) % 64 == 0 && (GK_CALL_BYTES - GK_CTR_CALL * 4) % 16 == 0, "aligned per-call memset");
// k_promote_dev over list[0 .. *count): level -1 -> class cls+1 (ingest
// overflow: joins the re-run list, or the defer list when that class has no
// free slot), -2 -> class cls+1 (import), level >= 0 -> class `level` if below it
hipError_t gk_launch_promote_dev(const GKState& st, const int32_t* count, const int32_t* list, int level,
                                 const GKPoolDev& pool, hipStream_t stream);
// ---- compaction (gk_compact.hip): every stream into the smallest class that holds its table ----
// Control words of a gk_compact call (zeroed by the caller), per class k > 0:
#define GK_CMP_FINAL 0    // [k] streams whose class after the compaction is k
#define GK_CMP_LEAVE 4    // [4 + k] streams of class k that move down (the demoted)
#define GK_CMP_ARRIVE 8   // [8 + k] streams that move down into class k
#define GK_CMP_TAKEN 12   // [12 + k] slots of the new arena of class k handed out by k_compact_move
#define GK_CMP_STUCK 12   // (class 0 has no arena counter) streams k_compact_move found no slot for: never
#define GK_CMP_WORDS 16
static_assert(GK_CMP_TAKEN + GK_MAX_CLASSES <= GK_CMP_WORDS, "one counter per class");
// the counts above; mutates no stream state
hipError_t gk_launch_compact_plan(const GKState& st, int32_t* ctl, hipStream_t stream);
// the streams above class 0 whose class after the compaction is t move their tables: t == 0 to their class-0
// home, t > 0 into slots [0, ctl[GK_CMP_TAKEN + t]) of the new arena ntab (nalloc slots; st holds the old
// arenas) with nlist[slot] = the stream -- the class's rebuilt member list
hipError_t gk_launch_compact_move(const GKState& st, int t, GKRec* ntab, int64_t nalloc, int32_t* nlist, int32_t* ctl,
                                  hipStream_t stream);
