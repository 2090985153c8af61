// gk_capi.cpp -- C ABI runtime of the MI355X batched GKArray engine.
//
// Owns the per-set device state (header arrays, table arenas, pending
// buffers), decides flush modes and table-capacity classes, and launches the
// kernels of the gk_*.hip units (gk_launch.h) on the caller's HIP stream and
// the set's aux streams.  Every entry point is declared in include/gk_capi.h
// with the reference method it replaces.  (Ingest / flush: ingest_call.)
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <string>
#include <vector>

#include "gk_capi.h"
#include "gk_checks.h"
#include "gk_pack.h"
#include "gk_format.h"
#include "gk_launch.h"
#include "gk_state.h"

namespace {

#define HIP_TRY(expr)                                                                  \
  do {                                                                                 \
    hipError_t e_ = (expr);                                                            \
    if (e_ != hipSuccess) return fail(GK_E_HIP, "%s: %s", #expr, hipGetErrorString(e_)); \
  } while (0)

constexpr int kCapSmall = GK_SMALL_CAP;  // LDS class (gk_launch.h)
constexpr int kCapLarge = 2048;  // LDS class, ~92 KB per wave
constexpr int kCapHuge = 32768;  // global-workspace class (k_ingest)
constexpr int kCapBig = 1 << 20;  // first unbounded class (k_ingest_big) after kCapHuge
constexpr int kCapMax = 1 << 27;  // largest class (2 GiB per table)
constexpr int kPMax = 1 << 24;    // largest flush period (eps >= 6e-8)
constexpr int64_t kRecipTable = (int64_t)1 << 17;  // entries of st.rtab (1 MiB)
constexpr int kMaxLdsCap = 2048;
constexpr int kRounds = GK_MAX_CLASSES + 1;  // overflow lists: launch round 0 + one per promotion level

// Renew a device buffer: the old one is freed (the caller has synchronised
// whatever may still use it) and `bytes` are allocated in its place.  On
// failure *p is null and the HIP error is cleared.
template <typename T>
bool renew_dev(T** p, size_t bytes) {
  if (*p) (void)hipFree(*p);
  *p = nullptr;
  if (hipMalloc((void**)p, bytes) == hipSuccess) return true;
  *p = nullptr;
  (void)hipGetLastError();
  return false;
}

int vpl_for(int P) {
  int v = 1;
  while (v * 64 < P) v <<= 1;
  return v;
}

}  // namespace

struct gk_set {
  // no stream is in a class above 0 (creation, gk_reset; cleared by every
  // enqueued promotion): the member-list launches of run_ingest are skipped
  bool no_members = true;
  int64_t S = 0;
  double eps = 0;
  int P = 0;
  int device = 0;
  int vpl = 1;
  GKState st{};
  // Capacity classes c > 0 live entirely on the device: slot counters, member
  // lists and re-run lists (GKPoolDev, k_promote_dev).  The host only sizes
  // the arenas (st.alloc) ahead of need, from counters read back
  // asynchronously at the end of each call (h_ctr, ev_done).
  int32_t* d_ctr = nullptr;                                  // GK_CTR_WORDS counters
  int32_t* d_list[GK_MAX_CLASSES] = {};
  int32_t* d_rerun[GK_MAX_CLASSES] = {};
  // kernel of each class: the unbounded k_ingest_big (classes beyond 32768
  // entries; every class when P > 1024) or the capacity-class kernels
  bool big[GK_MAX_CLASSES] = {};
  int32_t* d_defer = nullptr;  // streams whose next class had no free slot (S entries)
  int32_t* h_ctr = nullptr;  // pinned: the counters as of the end of the last call
  hipEvent_t ev_done = nullptr;
  bool done_pending = false;
  // the last ingest / flush call: its inputs, kept to re-run deferred streams
  // (the caller keeps them valid until the set's next call or gk_sync)
  struct : GKBatch {
    bool may_defer = false;  // some class could run out of slots in it
  } last;
  // a gk_reset came after the call whose counters are still in flight: its
  // deferred streams are void (every stream was reset; nothing to re-run)
  bool void_defer = false;
  // the per-call counter block is known zero: gk_reset's k_reset zeroed it and
  // nothing has written it since (begin_call then skips its memset; cleared by
  // begin_call and by the paths that write the block without it: run_levels,
  // gk_import)
  bool ctr_clean = false;
  int32_t fatal_seen = 0;  // device FATAL count already reported
  int sticky = GK_OK;      // asynchronous error reported by the next call / gk_sync
  std::string sticky_msg;
  // global workspace of each class beyond LDS (allocated with its first slots)
  unsigned char* d_ws[GK_MAX_CLASSES] = {};
  size_t ws_bytes[GK_MAX_CLASSES] = {};
  int64_t ws_blocks[GK_MAX_CLASSES] = {};
  // overflow lists of the launch rounds (device); counts in one array
  int32_t* d_ovfc = nullptr;              // kRounds counts (words of d_ctr)
  int32_t* d_ovfl[kRounds] = {};
  int32_t* h_ovf = nullptr;               // pinned readback of a count (+ list) for merge / import
  int64_t* d_zero_offs = nullptr;  // S+1 zeros: offsets of flush-only launches
  unsigned long long* d_work = nullptr;  // the call's hand-out counters (bytes of d_ctr from GK_CALL_WORK)
  int next_work = 0;                     // next free 128-byte counter of this call
  int32_t* d_long_list = nullptr;        // streams k_stats hands to k_stats_long (longest first)
  int64_t* d_long_n = nullptr;           //   and their pre-call n
  int32_t* d_long_count = nullptr;       // (a word of d_ctr)
  // k_stats_long (the sequential _sum/_avg chains of long streams) runs on
  // this stream beside the ingest launches; ev_fork / ev_join order it
  hipStream_t aux = nullptr;
  hipEvent_t ev_fork = nullptr, ev_join = nullptr;
  hipEvent_t ev_slgo = nullptr;  // aux has passed the fork: k_stats_long is next there
  // presorted flush batches of long streams (sets whose class 0 is the 2048
  // class): plan arrays, workspace, and the size the last call needed
  GKPresort ps;
  int64_t* h_ws_need = nullptr;  // pinned host copy of *ps.ws_need (valid once ev_done completed)
  // query scratch: pinned host copy of qs (the async H2D reads it), device copy
  double* h_qs = nullptr;
  double* d_qs = nullptr;
  int qs_alloc = 0;
  hipEvent_t ev_qs = nullptr;  // the last H2D copy out of h_qs
  int qs_n = 0;                // entries of the list last uploaded to d_qs (h_qs holds it)
  // eighths of a wave per CU of the small-class batch launch that walk the gk:52-59
  // stats chains first (0: separate k_stats launch); GK_FUSED_STATS overrides
  int fused_stats = 8;  // eighths of a wave per CU that start with the stats role (DESIGN 5 Stats)
  // gk_fold_packed: receives the packed states merged into this set (made on first use)
  gk_set* fold_scratch = nullptr;
  gk_set* self_scratch = nullptr;  // snapshot source of dst.merge(dst), only during that merge
  int64_t* d_roll_prog = nullptr;  // gk_rollup into this set: the member a resumed fold starts at (first use)
  // Keyed ingest (gk_group_by_key / gk_ingest_keyed; all made on first use,
  // only grown, freed in gk_destroy): the grouping scratch, the grouped batch
  // gk_ingest_keyed ingests from -- h->last.x / h->last.offs of such a call,
  // so the next call's grouping is enqueued only after its settle -- and the
  // pinned copy of the cumulative bad-id block (kg.cum), read back with the
  // counters before ev_done.
  GKGroupScratch kg;
  int64_t kg_cap = 0;       // samples the pair buffers hold
  int kg_pairs = 0;         // id buffers allocated (1 or 2; one value buffer fewer)
  int64_t kg_tiles = 0;     // tiles kg.hist holds
  int64_t kg_sums = 0;      // entries of kg.sums
  double* kg_vals = nullptr;  // grouped values (kg_vals_cap doubles) and offsets (S + 1)
  int64_t kg_vals_cap = 0;
  int64_t* kg_offs = nullptr;
  unsigned long long* h_kg = nullptr;  // pinned GK_KG_CUM_WORDS words
  unsigned long long kg_bad_seen = 0;  // voided keyed calls already reported
  // Per-stream selection (gk_*_select; made on first use, only grown, freed in
  // gk_destroy): GK_SEL_WORDS control words, the bitmap of listed streams and
  // the flush list (k_select_check)
  int32_t* d_sel = nullptr;
  int64_t sel_words = 0;
  // gk_ranks_keyed: the sample indices the group-by carries as its payload
  // (rk_idx_cap doubles, bit-cast int64; made on first use, only grown).
  // gk_rank_ingest_keyed: the same, and once the group-by has consumed them the
  // buffer takes the grouped VALUES its ingest reads (k_rank_ingest_keyed) --
  // h->last.x of that call, with kg_offs as h->last.offs: like kg_vals it is
  // rewritten only by calls that have settled the last one (gk_sync first).
  double* rk_idx = nullptr;
  int64_t rk_idx_cap = 0;
  // What the call in progress still has to join on the caller's stream: set
  // next to the launch that makes the debt (stats_fork, launch_wg), settled
  // and cleared by join_owed alone -- on every path, errors included: the
  // next call's begin_call zeroes counters those kernels add to.
  struct {
    bool wg = false;         // k_ingest_wg on aux2 (ev_wg)
    bool aux = false;        // k_stats_long forked to aux (ev_join)
    bool presort = false;    // the presort on aux2 / aux3 (ev_presort)
    bool sl_inline = false;  // no fork: k_stats_long on the call's own stream, behind the ingest
    const double* sl_x = nullptr;  // (its arguments)
    const int64_t* sl_offs = nullptr;
  } owed;
  // the presort of the long streams' flush batches runs here beside the short
  // streams' chains (k_stats on the caller's stream); the ingest waits for it
  hipStream_t aux2 = nullptr;
  hipStream_t aux3 = nullptr;    // the presort when k_ingest_wg runs beside it (ps.done)
  hipEvent_t ev_presort = nullptr;
  hipEvent_t ev_wg = nullptr;  // k_ingest_wg (on aux2, after the presort) done
  hipEvent_t ev_go = nullptr;  // the call's counters zeroed: k_ingest_wg may be launched (GK_WG_EARLY)
  bool wg_trace = false;       // GK_WG_TRACE=1 at creation: its stream count per completed call on stderr (tests)
  // timing: event pairs recorded around the timed launches, summed at read
  bool timing = false;        // events around the class-0 ingest launch (gk_timing_enable bit 0)
  bool timing_stats = false;  // and around stats_fork's launches (bit 1: two more markers per call)
  std::vector<hipEvent_t> tev_flush, tev_stats;
  size_t n_flush = 0, n_stats = 0;
};

namespace {

// Every launch of the last class counts the streams that outgrow it as fatal
// itself (k_ingest pmode bit 1), so no promotion round is needed past it --
// unless that class runs k_ingest_big (or there is a single class).
bool fatal_direct(const gk_set* h) { return h->st.nclass >= 2 && !h->big[h->st.nclass - 1]; }

// What a launch of class c >= 1 (k_ingest) does itself with the streams that
// outgrow it, instead of listing them for the next promotion round: 2 =
// count them fatal (the last class), 4 = defer them (the next class has no
// slot during this call: the round would defer every one), 0 = list them.
int overflow_direct(const gk_set* h, int c) {
  const int R = h->st.nclass;
  if (c < 1 || c >= R || h->big[c]) return 0;
  if (c == R - 1) return fatal_direct(h) ? 2 : 0;
  return h->st.alloc[c + 1] == 0 ? 4 : 0;
}

GKPoolDev pool_args(const gk_set* h) {
  GKPoolDev p;
  p.ctr = h->d_ctr;
  p.rcnt = h->d_ctr + GK_CTR_RCNT;
  p.defer = h->d_defer;
  for (int c = 0; c < GK_MAX_CLASSES; ++c) {
    p.list[c] = h->d_list[c];
    p.rerun[c] = h->d_rerun[c];
  }
  return p;
}

// Global workspace of class c (ingest and merge share it), for classes beyond
// LDS; allocated when the class gets its first slots.
int ensure_ws(gk_set* h, int c) {
  const int cap = h->st.cap[c];
  if (h->d_ws[c] || (cap <= kMaxLdsCap && !h->big[c])) return GK_OK;
  size_t b = std::max(h->big[c] ? gk_big_ws_bytes(cap, h->P) : gk_ingest_ws_bytes(cap, h->vpl),
                      gk_merge_lds_bytes(cap, h->st.pmax));
  b = (b + 4095) & ~(size_t)4095;
  // class 0 holds every stream: many waves; a larger class only the rare
  // streams that outgrew the ones below, so a few blocks per 4096 streams.
  // At most ~2 GiB of workspace per class.
  const int64_t S = std::max<int64_t>(h->S, 1);
  int64_t blocks = c == 0 ? std::min<int64_t>(S, (int64_t)gk_num_cu() * 8)
                          : std::min<int64_t>(gk_num_cu(), std::max<int64_t>(8, S / 4096));
  blocks = std::max<int64_t>(1, std::min<int64_t>(blocks, ((int64_t)2 << 30) / (int64_t)b));
  if (hipMalloc(&h->d_ws[c], b * blocks) != hipSuccess) {
    h->d_ws[c] = nullptr;
    return fail(GK_E_NOMEM, "class-%d workspace of %lld x %zu bytes failed", c, (long long)blocks, b);
  }
  h->ws_bytes[c] = b;
  h->ws_blocks[c] = blocks;
  return GK_OK;
}

// Slots a class starts with (grown on demand, see grow_pools): every stream
// while that costs at most 1 GiB (then no call can run out of slots), else a
// share of the streams.
int64_t initial_slots(const gk_set* h, int c) {
  const int64_t S = std::max<int64_t>(h->S, 1);
  if (c > 0 && h->st.cap[c] > kCapHuge) return 0;  // unbounded classes: on first use
  if (const char* e = getenv("GK_POOL_SLOTS"))  // tests: force tiny arenas (deferral / growth paths)
    return std::max<int64_t>(1, std::min<int64_t>(S, atoll(e)));
  const int64_t slot_bytes = (int64_t)h->st.cap[c] * (int64_t)sizeof(GKRec);
  if (S * slot_bytes <= ((int64_t)1 << 30)) return S;
  const int64_t n = h->st.cap[c] <= kCapLarge ? std::max<int64_t>(4096, S / 16) : std::max<int64_t>(64, S / 1024);
  return std::min<int64_t>(n, S);
}

// Grow class c's arena to `want` slots, keeping the slots handed out so far.
// Synchronises `s` (the arena may be in use by earlier launches).
int grow_class(gk_set* h, int c, int64_t want, hipStream_t s) {
  want = std::min<int64_t>(want, std::max<int64_t>(h->S, 1));
  if (want <= h->st.alloc[c]) return GK_OK;
  HIP_TRY(hipStreamSynchronize(s));
  if (ensure_ws(h, c) != GK_OK) return GK_E_NOMEM;
  int32_t used = 0;
  HIP_TRY(hipMemcpy(&used, h->d_ctr + GK_CTR_USED + c, sizeof(int32_t), hipMemcpyDeviceToHost));
  const int64_t keep = std::min<int64_t>(std::max(used, 0), h->st.alloc[c]);
  GKRec* nt = nullptr;
  if (hipMalloc(&nt, (size_t)want * h->st.cap[c] * sizeof(GKRec)) != hipSuccess)
    return fail(GK_E_NOMEM, "class-%d arena of %lld slots failed", c, (long long)want);
  if (h->st.tab[c] && keep) {
    HIP_TRY(hipMemcpy(nt, h->st.tab[c], (size_t)keep * h->st.cap[c] * sizeof(GKRec), hipMemcpyDeviceToDevice));
  }
  if (h->st.tab[c]) (void)hipFree(h->st.tab[c]);
  h->st.tab[c] = nt;
  h->st.alloc[c] = (int32_t)want;
  return GK_OK;
}

// gk_compact: the slots class c > 0 keeps for `members` streams -- what a set
// would start with (initial_slots) or twice the members, so that the next
// call's grow_pools (2 * used > alloc) does not regrow an arena no stream has
// entered; never more than it has, unless the streams that come down into it
// need more.
int64_t compact_slots(const gk_set* h, int c, int64_t members) {
  int64_t want = std::min<int64_t>(std::max<int64_t>(h->S, 1), std::max<int64_t>(initial_slots(h, c), 2 * members));
  want = std::min<int64_t>(want, h->st.alloc[c]);
  return std::max<int64_t>(want, members);
}

// Bytes of class c's arena and of its workspace (gk_class_usage).
int64_t arena_bytes(const gk_set* h, int c) {
  return (c == 0 ? h->S : (int64_t)h->st.alloc[c]) * h->st.cap[c] * (int64_t)sizeof(GKRec);
}
int64_t workspace_bytes(const gk_set* h, int c) {
  return h->d_ws[c] ? (int64_t)h->ws_bytes[c] * h->ws_blocks[c] : 0;
}

// The device and arena work of gk_compact on a settled, synchronised set; ctl:
// GK_CMP_WORDS words of device scratch.  Destination classes ascending: class
// 0 first (the streams that go home, no allocation), then each class t > 0
// gets a new arena beside the old ones, its members -- the ones that stay and
// the ones that come down from the classes above, whose old arenas are all
// still there -- move into dense slots of it, and the old arena of t, which no
// stream lives in any more, is freed before class t + 1 is looked at: one new
// arena at a time.  GK_E_NOMEM leaves the classes below t compacted and every
// stream of t and above where it was, header and table together.
int compact_classes(gk_set* h, int32_t* ctl, hipStream_t s, int64_t* demoted) {
  GKState& st = h->st;
  const int R = st.nclass;
  int32_t plan[GK_CMP_WORDS], ctr[2 * GK_MAX_CLASSES];
  static_assert(GK_CTR_LCNT == GK_CTR_USED + GK_MAX_CLASSES, "slots used and list lengths are read back together");
  HIP_TRY(hipMemsetAsync(ctl, 0, GK_CMP_WORDS * sizeof(int32_t), s));
  HIP_TRY(gk_launch_compact_plan(st, ctl, s));
  HIP_TRY(hipStreamSynchronize(s));
  HIP_TRY(hipMemcpy(plan, ctl, sizeof(plan), hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(ctr, h->d_ctr + GK_CTR_USED, sizeof(ctr), hipMemcpyDeviceToHost));
  int64_t home = 0;  // streams that go back to class 0
  for (int c = 1; c < R; ++c) {
    *demoted += plan[GK_CMP_LEAVE + c];
    home += plan[GK_CMP_LEAVE + c] - plan[GK_CMP_ARRIVE + c];
  }
  if (home > 0) HIP_TRY(gk_launch_compact_move(st, 0, nullptr, 0, nullptr, ctl, s));
  int64_t promoted = 0;
  for (int t = 1; t < R; ++t) {
    const int32_t members = plan[GK_CMP_FINAL + t];
    const int64_t want = compact_slots(h, t, members);
    promoted += members;
    // nothing leaves or enters, slots and list already dense, arena at its size: not copied
    if (plan[GK_CMP_LEAVE + t] == 0 && plan[GK_CMP_ARRIVE + t] == 0 && ctr[t] == members &&
        ctr[GK_MAX_CLASSES + t] == members && want == st.alloc[t])
      continue;
    GKRec* nt = nullptr;
    // (streams may come down into a class that had no slots yet: slots > 0 implies a workspace)
    if (want > 0 && ensure_ws(h, t) != GK_OK) {
      (void)hipStreamSynchronize(s);
      return GK_E_NOMEM;
    }
    if (want > 0 && hipMalloc(&nt, (size_t)want * st.cap[t] * sizeof(GKRec)) != hipSuccess) {
      (void)hipGetLastError();
      (void)hipStreamSynchronize(s);
      return fail(GK_E_NOMEM, "compaction: class-%d arena of %lld slots failed (classes below it are compacted)", t,
                  (long long)want);
    }
    if (members > 0) HIP_TRY(gk_launch_compact_move(st, t, nt, want, h->d_list[t], ctl, s));
    const int32_t cnt[2] = {members, members};
    HIP_TRY(hipMemcpyAsync(h->d_ctr + GK_CTR_USED + t, &cnt[0], sizeof(int32_t), hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(h->d_ctr + GK_CTR_LCNT + t, &cnt[1], sizeof(int32_t), hipMemcpyHostToDevice, s));
    HIP_TRY(hipStreamSynchronize(s));  // (cnt is read; the old arena is read no more)
    if (st.tab[t]) (void)hipFree(st.tab[t]);
    st.tab[t] = nt;
    st.alloc[t] = (int32_t)want;
    // a class back at no slots is the not-yet-used class of gk_create: no workspace either
    // (grow_class makes both again when a stream is deferred for want of a slot)
    if (want == 0 && h->d_ws[t]) {
      (void)hipFree(h->d_ws[t]);
      h->d_ws[t] = nullptr;
      h->ws_bytes[t] = 0;
      h->ws_blocks[t] = 0;
    }
  }
  HIP_TRY(hipMemcpy(plan, ctl, sizeof(plan), hipMemcpyDeviceToHost));
  if (plan[GK_CMP_STUCK] != 0) return fail(GK_E_HIP, "compaction: %d stream(s) found no slot", plan[GK_CMP_STUCK]);
  h->no_members = promoted == 0;
  return GK_OK;
}

// Consume the counters read back at the end of the last call: report streams
// that found no class / slot (sticky GK_E_OVERFLOW), learn the presort
// workspace the last call needed.  block: wait for that call to finish.
void poll(gk_set* h, bool block) {
  if (!h->done_pending) return;
  if (block) {
    if (hipEventSynchronize(h->ev_done) != hipSuccess) return;
  } else if (hipEventQuery(h->ev_done) != hipSuccess) {
    return;
  }
  h->done_pending = false;
  if (h->void_defer) {
    h->h_ctr[GK_CTR_DEFER] = 0;
    h->void_defer = false;
  }
  if (h->ps.wg_count && h->wg_trace && h->h_ctr[GK_CTR_WORDS] > 0)
    fprintf(stderr, "[gk] k_ingest_wg: %d stream(s)\n", h->h_ctr[GK_CTR_WORDS]);
  const int32_t fatal = h->h_ctr[GK_CTR_FATAL];
  if (fatal > h->fatal_seen && h->sticky == GK_OK) {
    char buf[512];
    snprintf(buf, sizeof(buf),
             "%d stream(s) (largest id %d) outgrew every table capacity class (largest %d entries), found no "
             "free slot, or passed the per-stream count limit 2*eps*(n-1) <= 2^30: their values of that call "
             "were not added (past the last flush that fitted the smallest class, if one did)",
             fatal - h->fatal_seen, h->h_ctr[GK_CTR_FATAL + 1], h->st.cap[h->st.nclass - 1]);
    h->sticky = GK_E_OVERFLOW;
    h->sticky_msg = buf;
  }
  h->fatal_seen = fatal;
  // a keyed call that met an id >= S (it added nothing): reported the same way
  if (h->h_kg && h->h_kg[0] > h->kg_bad_seen) {
    if (h->sticky == GK_OK) {
      char buf[256];
      snprintf(buf, sizeof(buf),
               "keyed ingest: sample %lld has stream id %lld outside [0, %lld): no value of that call was added",
               (long long)h->h_kg[1], (long long)h->h_kg[2], (long long)h->S);
      h->sticky = GK_E_ARG;
      h->sticky_msg = buf;
    }
    h->kg_bad_seen = h->h_kg[0];
  }
}

int promote_rounds(gk_set* h, const GKBatch& a, hipStream_t s, bool fresh = false);
int mark_done(gk_set* h, hipStream_t s, bool ingest = false);

// Start of a call's device work: ONE memset zeroes every per-call counter
// (deferred / long-stream counts, re-run and overflow list lengths, the
// launches' stream hand-out counters; gk_launch.h GK_CTR_*).
int begin_call(gk_set* h, hipStream_t s) {
  if (!h->ctr_clean)
    HIP_TRY(hipMemsetAsync(h->d_ctr + GK_CTR_CALL, 0, GK_CALL_BYTES - GK_CTR_CALL * sizeof(int32_t), s));
  h->ctr_clean = false;
  h->next_work = 0;
  return GK_OK;
}

// The zeroed hand-out counter of the call's next launch (the small-class
// launch has its own GK_WORK_BYTES block).
unsigned long long* work_counter(gk_set* h, bool small) {
  if (small) return h->d_work;
  if (h->next_work >= GK_CALL_SLOTS) return nullptr;  // (launches per call are bounded: 1 + R-1 + R(R-1)/2)
  return (unsigned long long*)((char*)h->d_work + GK_WORK_BYTES + 128 * (h->next_work++));
}

// GK_TRACE=1: the host runtime's slow-path decisions on stderr (debugging)
bool g_trace = getenv("GK_TRACE") != nullptr;
#define GK_TR(...)                      \
  do {                                  \
    if (g_trace) {                      \
      fprintf(stderr, "[gk] " __VA_ARGS__); \
      fputc('\n', stderr);              \
      fflush(stderr);                   \
    }                                   \
  } while (0)

// Grow the arenas for the `count` streams of device list `list`, each moving
// one class up (deferred ingest streams, import overflows): the target class
// of each is read back (synchronises), so only the classes they go to grow --
// the unbounded classes (MiB..GiB per slot) are allocated only when used.
int grow_targets(gk_set* h, const int32_t* list, int64_t count, hipStream_t s) {
  if (count <= 0) return GK_OK;
  std::vector<int32_t> ids(count), cls(std::max<int64_t>(h->S, 1));
  HIP_TRY(hipStreamSynchronize(s));
  HIP_TRY(hipMemcpy(ids.data(), list, count * sizeof(int32_t), hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(cls.data(), h->st.cls, h->S * sizeof(int32_t), hipMemcpyDeviceToHost));
  int64_t need[GK_MAX_CLASSES] = {};
  for (int32_t id : ids) {
    const int t = cls[id] + 1;
    if (t < h->st.nclass) ++need[t];
  }
  for (int c = 1; c < h->st.nclass; ++c) {
    if (!need[c]) continue;
    int32_t used = 0;
    HIP_TRY(hipMemcpy(&used, h->d_ctr + GK_CTR_USED + c, sizeof(int32_t), hipMemcpyDeviceToHost));
    int64_t want = (int64_t)used + 2 * need[c];
    if (h->st.cap[c] <= kCapHuge) want = std::max<int64_t>(want, 2 * (int64_t)h->st.alloc[c]);
    GK_TR("grow_targets: class %d used %d need %lld -> want %lld", c, used, (long long)need[c], (long long)want);
    int rc = grow_class(h, c, want, s);
    if (rc) return rc;
  }
  return GK_OK;
}

// Streams the last call deferred (their next class had no free slot): grow
// the arenas and run them again, from that call's inputs, before anything
// else touches the set.
int replay_deferred(gk_set* h, hipStream_t s) {
  for (int guard = 0; guard < 2 * GK_MAX_CLASSES + 2; ++guard) {
    const int32_t nd = h->h_ctr[GK_CTR_DEFER];
    if (nd <= 0) return GK_OK;
    h->h_ctr[GK_CTR_DEFER] = 0;
    GK_TR("replay: %d deferred stream(s), round %d", nd, guard);
    int rc = grow_targets(h, h->d_defer, nd, s);
    GK_TR("replay: grown rc=%d", rc);
    if (rc) return rc;
    // the deferred list becomes round 0's overflow list of a fresh call
    HIP_TRY(hipMemcpyAsync(h->d_ovfl[0], h->d_defer, (size_t)nd * sizeof(int32_t), hipMemcpyDeviceToDevice, s));
    int rb = begin_call(h, s);
    if (rb) return rb;
    h->h_ovf[0] = nd;  // pinned; the stream is synchronised below before it is reused
    HIP_TRY(hipMemcpyAsync(h->d_ovfc, h->h_ovf, sizeof(int32_t), hipMemcpyHostToDevice, s));
    rc = promote_rounds(h, h->last, s);
    GK_TR("replay: enqueued rc=%d", rc);
    if (!rc) rc = mark_done(h, s);
    if (rc) return rc;
    HIP_TRY(hipStreamSynchronize(s));
    GK_TR("replay: done");
    poll(h, true);
  }
  return fail(GK_E_OVERFLOW, "deferred streams could not be placed in a capacity class");
}

// Before a call (and in gk_sync): settle the previous call -- wait for it when
// it may have deferred streams (some class could run out of slots), re-run
// those, report its asynchronous errors.
int settle(gk_set* h, hipStream_t s, bool block) {
  poll(h, block || h->last.may_defer);
  if (h->done_pending) return GK_OK;  // still running, and it cannot have deferred anything
  const int rc = replay_deferred(h, s);
  // settled: nothing is re-run from that call any more, so its fused query is
  // forgotten (gk_reset waits only for a query whose call is not settled yet)
  if (!rc) h->last.q = GKQuery();
  return rc;
}

// Before a call: keep every class's arena at least twice what is in use, so
// that the device-side promotions of the call find free slots.
int grow_pools(gk_set* h, hipStream_t s) {
  int rc = settle(h, s, false);
  if (rc) return rc;
  for (int c = 1; c < h->st.nclass; ++c) {
    const int64_t used = h->h_ctr ? h->h_ctr[GK_CTR_USED + c] : 0;
    if (2 * used > h->st.alloc[c]) {
      int rc = grow_class(h, c, std::max<int64_t>(4 * used, 2 * (int64_t)h->st.alloc[c]), s);
      if (rc) return rc;
    }
  }
  // presort workspace: what the last completed call needed (its long streams
  // flushed unsorted if it did not fit -- same results, slower)
  if (h->ps.ws_need && h->h_ws_need && *h->h_ws_need > h->ps.ws_cap) {
    const int64_t need = *h->h_ws_need;
    const int64_t cap = std::max<int64_t>(need + need / 8, 1 << 20);
    HIP_TRY(hipStreamSynchronize(s));
    HIP_TRY(hipStreamSynchronize(h->aux));
    if (h->aux2) HIP_TRY(hipStreamSynchronize(h->aux2));
    if (h->aux3) HIP_TRY(hipStreamSynchronize(h->aux3));
    // (a failure is not fatal: long streams flush unsorted)
    h->ps.ws_cap = renew_dev(&h->ps.ws, (size_t)cap * sizeof(double)) ? cap : 0;
  }
  return GK_OK;
}

// Return (and clear) an asynchronous error of an earlier call.
int take_sticky(gk_set* h) {
  if (h->sticky == GK_OK) return GK_OK;
  const int rc = h->sticky;
  g_err = h->sticky_msg;
  h->sticky = GK_OK;
  h->sticky_msg.clear();
  return rc;
}

// End of a call's device work on `s`: counters -> pinned host memory.
// (ingest: the call listed the long streams -- word GK_CTR_LONG comes back
// too; every other call leaves the host copy of the last ingest's count, which
// stats_fork's fork decision reads)
static_assert(GK_CTR_LONG == GK_CTR_WORDS - 1, "the long-stream count is the last word read back");
int mark_done(gk_set* h, hipStream_t s, bool ingest) {
  HIP_TRY(hipMemcpyAsync(h->h_ctr, h->d_ctr, (GK_CTR_WORDS - (ingest ? 0 : 1)) * sizeof(int32_t),
                         hipMemcpyDeviceToHost, s));
  if (h->ps.wg_count && h->wg_trace)
    HIP_TRY(hipMemcpyAsync(h->h_ctr + GK_CTR_WORDS, h->ps.wg_count, sizeof(int32_t), hipMemcpyDeviceToHost, s));
  if (h->kg.cum)
    HIP_TRY(hipMemcpyAsync(h->h_kg, h->kg.cum, GK_KG_CUM_WORDS * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
  HIP_TRY(hipEventRecord(h->ev_done, s));
  h->done_pending = true;
  h->void_defer = false;  // (the readback in flight is now this call's)
  return GK_OK;
}

int32_t* ovf_count(gk_set* h, int r) { return h->d_ovfc + r; }
int32_t* ovf_list(gk_set* h, int r) { return h->d_ovfl[r]; }

// Read back round r's overflow count and list (synchronises; merge / import only).
int64_t read_overflow(gk_set* h, int r, hipStream_t stream) {
  if (hipMemcpyAsync(h->h_ovf, h->d_ovfc + r, sizeof(int32_t), hipMemcpyDeviceToHost, stream) != hipSuccess ||
      hipStreamSynchronize(stream) != hipSuccess)
    return fail(GK_E_HIP, "overflow readback failed: %s", hipGetErrorString(hipGetLastError()));
  return h->h_ovf[0];
}

hipEvent_t timing_event(std::vector<hipEvent_t>& v, size_t& n) {
  if (n == v.size()) {
    hipEvent_t e = nullptr;
    if (hipEventCreate(&e) != hipSuccess) return nullptr;
    v.push_back(e);
  }
  return v[n++];
}

// One launch of class c: every stream (c == 0) or the streams of `list`
// whose length is *count_ptr (device).  Overflowing streams go to round r's
// list.  L: what the caller has set already (run_ingest's class-0 launch: the
// priority list, the presort, the stats role, the timing events; pmode of a
// fused promotion round); the rest of the descriptor is filled here.
hipError_t launch_class(gk_set* h, const GKBatch& a, int c, const int32_t* list, const int32_t* count_ptr, int r,
                        hipStream_t stream, GKIngestLaunch L = GKIngestLaunch()) {
  if (c > 0 && h->st.alloc[c] == 0) return hipSuccess;  // no slot yet: no member
  L.work = work_counter(h, c == 0 && h->st.cap[0] == GK_SMALL_CAP && !h->big[0]);
  if (!L.work) return hipErrorInvalidValue;
  const GKPoolDev pool = pool_args(h);
  static_cast<GKBatch&>(L) = a;
  L.list = list;
  L.count = list ? 0 : h->S;
  L.count_ptr = count_ptr;
  L.lcls = c;
  L.cap = h->st.cap[c];
  L.vpl = h->vpl;
  L.ws = h->d_ws[c];
  L.ws_bytes = h->ws_bytes[c];
  L.ws_blocks = h->ws_blocks[c];
  L.ovf_count = ovf_count(h, r);
  L.ovf_list = ovf_list(h, r);
  if (h->big[c]) {
    L.ctr = h->d_ctr;
    return gk_launch_ingest_big(h->st, L, stream);
  }
  L.pool = &pool;
  L.pmode |= overflow_direct(h, c);
  return gk_launch_ingest(h->st, L, stream);
}

// gk:52-59 for a batch: k_stats over every stream on `s` (it lists the
// streams longer than GK_STATS_LONG values, longest first), then the long
// streams' sequential _sum/_avg chains on h->aux, beside the ingest launches
// that follow on `s` (they touch neither _sum nor _avg).  stats_join makes
// `s` wait for them and, for a fused query, re-answers the long streams with
// their final _min/_max.
// the small-class batch launch walks the stats chains itself (k_stats then
// only lists the long streams)
bool stats_fused(const gk_set* h) { return h->fused_stats > 0 && h->st.cap[0] == GK_SMALL_CAP; }

// The one place that settles gk_set::owed: `s` waits for what the call
// launched on the aux streams and gets the k_stats_long owed to it, each
// entry cleared as it is settled; in this order: k_ingest_wg, k_stats_long
// (inline or forked), the presort.  strict: stop at the first HIP failure and
// report it; else best effort, errors ignored.  wg_only: that entry alone.
int join_owed(gk_set* h, hipStream_t s, bool strict, bool wg_only = false) {
#define OWED_TRY(flag, expr)   \
  if (h->owed.flag) {          \
    h->owed.flag = false;      \
    if (strict) HIP_TRY(expr); \
    else (void)(expr);         \
  }
  OWED_TRY(wg, hipStreamWaitEvent(s, h->ev_wg, 0));
  if (wg_only) return GK_OK;
  OWED_TRY(sl_inline,
           gk_launch_stats_long(h->st, h->owed.sl_x, h->owed.sl_offs, h->d_long_list, nullptr, h->d_long_count, s));
  OWED_TRY(aux, hipStreamWaitEvent(s, h->ev_join, 0));
  OWED_TRY(presort, hipStreamWaitEvent(s, h->ev_presort, 0));
#undef OWED_TRY
  return GK_OK;
}

// A call that fails between stats_fork and stats_join: best effort, `s` still
// waits for the aux work.
void stats_abort(gk_set* h, hipStream_t s) { (void)join_owed(h, s, false); }

// k_ingest_wg on aux2 behind wait_ev, over the head of the long list (the
// longest streams: one workgroup each); go: the device word its workgroups
// wait for (the early launch), or NULL.  The call owes its join from here on.
int launch_wg(gk_set* h, const double* x, const int64_t* offs, int force, unsigned long long* work,
              hipEvent_t wait_ev, const int32_t* go) {
  GKIngestLaunch L;
  static_cast<GKBatch&>(L) = GKBatch{x, offs, force};
  L.list = h->d_long_list;
  L.count_ptr = h->ps.wg_count;
  L.ovf_count = ovf_count(h, 0);
  L.ovf_list = ovf_list(h, 0);
  L.work = work;
  HIP_TRY(hipStreamWaitEvent(h->aux2, wait_ev, 0));
  HIP_TRY(gk_launch_ingest_wg(h->st, L, h->ps, go, h->aux2));
  HIP_TRY(hipEventRecord(h->ev_wg, h->aux2));
  h->owed.wg = true;
  return GK_OK;
}

int stats_fork(gk_set* h, const double* x, const int64_t* offs, hipStream_t s, int force) {
  hipEvent_t t0 = h->timing_stats ? timing_event(h->tev_stats, h->n_stats) : nullptr;
  if (t0) HIP_TRY(hipEventRecord(t0, s));
  // k_ingest_wg ahead of everything else of the call (GK_WG_EARLY, default
  // 1): launched behind the call's counter reset only, its workgroups take
  // their CUs (128 KiB of LDS and 8 waves each) while the chip is still
  // empty and wait on the device for k_long_prep's word; queued behind it,
  // they found the CUs held by the chain walks and the presort and started
  // 3.1-4.2 ms into a 38.9 ms cfg5 call (profiles/r05/r05AF3_*).  Launched
  // only after k_long_prep is enqueued, so that the word is always written.
  // The early workgroups spin on the device until k_long_prep has run, so
  // they are launched early only when the device keeps CUs free for it
  // (gk_wg_early_ok: at least 2 x GK_WG_MAX CUs; a partitioned device or
  // several sets sharing one could otherwise fill every CU with spinning
  // workgroups).  Read per call, like the other GK_WG switches.
  const char* early_s = getenv("GK_WG_EARLY");
  const int early_env = early_s ? atoi(early_s) : 1;
  const bool early = early_env && x && h->ps.done && h->ps.wg_count && h->aux2 && h->ps.list_ws && gk_wg_early_ok();
  if (early) HIP_TRY(hipEventRecord(h->ev_go, s));
  // the long-stream list (k_lengths) + k_long_prep, then the fork
  // (k_stats_long needs only the sorted list and the pre-call n: the longest
  // chains start at once), then on `s` the short streams' chains (k_stats,
  // unless the small-class launch walks them) and the presort of the long
  // streams' flush batches
  HIP_TRY(gk_launch_stats(h->st, offs, h->d_long_list, h->d_long_count, s));
  // k_long_prep sorts the list (longest first) and plans the presort /
  // workgroups -- unless the small-class launch carries the stats role
  // (P <= 128: no presort, no workgroups): then it is not needed at all
  // (k_stats_long reads the list in k_lengths' order and the pre-call n from
  // k_lengths' snapshot).
  // k_stats_long must be the first work on `aux` after the fork: queued behind
  // anything, its waves reach the CUs after the persistent ingest grid and run
  // ~3x longer beside it (round 5's k_long_prep on aux: cfg4 x 8 shards
  // 84 -> 118 ms per step, profiles/r05/r05E_*)
  const bool prep = !stats_fused(h);
  if (prep)
    HIP_TRY(gk_launch_long_prep(h->st, offs, h->d_long_list, h->d_long_n, h->d_long_count, h->ps, s,
                                early ? h->d_ctr + GK_CTR_WGGO : nullptr));
  unsigned long long* wwork_early = nullptr;
  if (early && prep) {
    wwork_early = work_counter(h, false);
    if (!wwork_early) return fail(GK_E_HIP, "no hand-out counter left for k_ingest_wg");
    const int rw = launch_wg(h, x, offs, force, wwork_early, h->ev_go, h->d_ctr + GK_CTR_WGGO);
    if (rw) return rw;
  }
  const bool presort = h->ps.list_ws && h->ps.ws && h->ps.ws_cap > 0;
  // No fork when nothing but k_stats_long would go to the aux streams and the
  // set's last ingest call listed no long stream (its count comes back with
  // that call's counters): k_stats_long then runs on `s` behind the ingest
  // (stats_join).  Forked, its workgroups must reach the CUs before the
  // persistent ingest grid -- the fork's cross-queue wake-up (~13 us) is then
  // on the step's critical path, and a k_stats_long dispatched beside the
  // ingest grid cost the cfg3 launch 8 % (profiles/r06/r06q_*).  A wrong
  // guess costs time only: the walk is the same on either stream.
  const bool sl_inline = stats_fused(h) && !prep && !early && !presort && !h->aux2 && h->h_ctr &&
                        h->h_ctr[GK_CTR_LONG] == 0 && !getenv("GK_SL_FORK");
  if (sl_inline) {
    h->owed.sl_inline = true;
    h->owed.sl_x = x;
    h->owed.sl_offs = offs;
  } else {
    HIP_TRY(hipEventRecord(h->ev_fork, s));
  }
  if (wwork_early) {
    // behind k_long_prep, on the same hand-out counter: the streams of any
    // early workgroup that gave up waiting for k_long_prep's word (bounded
    // spin, GK_WG_GO_TICKS); normally none are left and its workgroups leave
    // at once
    const int rw = launch_wg(h, x, offs, force, wwork_early, h->ev_fork, nullptr);
    if (rw) return rw;
  }
  // Forked ahead of the small-class launch (nothing else between them on
  // `s`): `s` waits until aux has passed the fork, so that k_stats_long's
  // waves reach the CUs before the persistent ingest grid -- dispatched beside
  // it they ran 2x longer and slowed the ingest (cfg4 x 8 shards 79 -> 84 ms
  // per step, profiles/r06/r07i_*).  Costs one cross-queue wake-up (~13 us)
  // on calls that fork (long streams: steps of tens of ms).
  const bool sl_order = !sl_inline && stats_fused(h) && !presort && !h->aux2;
  if (!sl_inline) {
    HIP_TRY(hipStreamWaitEvent(h->aux, h->ev_fork, 0));
    h->owed.aux = true;
    if (sl_order) HIP_TRY(hipEventRecord(h->ev_slgo, h->aux));
    HIP_TRY(gk_launch_stats_long(h->st, x, offs, h->d_long_list, prep ? h->d_long_n : nullptr, h->d_long_count,
                                 h->aux));
    HIP_TRY(hipEventRecord(h->ev_join, h->aux));
  }
  if (sl_order) HIP_TRY(hipStreamWaitEvent(s, h->ev_slgo, 0));
  if (presort) {
    // with k_ingest_wg beside it (ps.done): on its own stream, joined by
    // stats_join; else on aux2 ahead of k_ingest_wg
    hipStream_t ps_s = h->ps.done ? h->aux3 : h->aux2;
    HIP_TRY(hipStreamWaitEvent(ps_s, h->ev_fork, 0));
    HIP_TRY(gk_launch_presort(h->st, x, offs, h->d_long_list, h->d_long_n, h->d_long_count, h->ps, ps_s));
    HIP_TRY(hipEventRecord(h->ev_presort, ps_s));
    h->owed.presort = true;
  }
  if (!stats_fused(h)) HIP_TRY(gk_launch_stats_short(h->st, x, offs, s));
  // (with k_ingest_wg every presorted stream is one of its streams: the
  // one-wave launch runs beside the presort; k_ingest_wg is ordered after it
  // on aux2)
  if (presort && !h->ps.wg_count) HIP_TRY(hipStreamWaitEvent(s, h->ev_presort, 0));
  if (h->ps.ws_need) HIP_TRY(hipMemcpyAsync(h->h_ws_need, h->ps.ws_need, sizeof(int64_t), hipMemcpyDeviceToHost, s));
  hipEvent_t t1 = h->timing_stats ? timing_event(h->tev_stats, h->n_stats) : nullptr;
  if (t1) HIP_TRY(hipEventRecord(t1, s));
  return GK_OK;
}

int stats_join(gk_set* h, hipStream_t s, const GKQuery& q) {
  // (run_ingest may have returned before joining the early k_ingest_wg)
  const int rc = join_owed(h, s, true);
  if (rc) return rc;
  // (+ the _min/_max markers of the small-class launch's answers when it
  // carried the stats role: its chains are final here)
  HIP_TRY(gk_launch_query_list(h->st, h->d_long_list, h->d_long_count, q, stats_fused(h), s));
  return GK_OK;
}

// The ingest / flush launches of one call, with no host round trip: class 0
// over every stream and each larger class over its member list; a stream
// that outgrows its class is not committed, moves one class up on the device
// (k_promote_dev) and runs again there, at most once per class; a stream
// with no class left is counted as fatal (reported by a later call).
// Promotion rounds of a call: round r-1's overflow list moves one class up
// on the device and runs again in its new class (round r).  fresh: every
// stream started the call in class 0 (gk_create / gk_reset, nothing promoted
// since), so after r rounds no stream is above class r: round r re-runs
// class r only (the launches of the classes above would find their re-run
// lists empty).
int promote_rounds(gk_set* h, const GKBatch& a, hipStream_t stream, bool fresh) {
  const int R = h->st.nclass;
  GKPoolDev pool = pool_args(h);
  bool ran = true;  // a launch ran in the previous round (round 0: class 0)
  for (int r = 1; r <= R; ++r) {
    // (fresh: round r-1 re-ran class r-1 only; a class with no slots has no
    // launch, and then round r has nothing to promote)
    if (fresh && !ran) break;
    // (past the last class only fatal streams are left to count, and with
    // fatal_direct its launches counted them; fresh: round r-1 re-ran class
    // r-1 only, which counted or deferred its overflows itself)
    if (r == R && fatal_direct(h)) break;
    if (fresh && overflow_direct(h, r - 1)) break;
    int32_t* rcnt = h->d_ctr + GK_CTR_RCNT + GK_MAX_CLASSES * r;  // zeroed at the start of the call
    pool.rcnt = rcnt;
    h->no_members = false;
    // Fused round: every class launched this round has slots and runs
    // k_ingest, so each launch promotes the streams of round r-1's overflow
    // list whose next class is its own (k_ingest pmode bit 0) -- no
    // k_promote_dev launch and no re-run list.  GK_PROMOTE_FUSE=0: always the
    // separate promotion.
    const int c_end = fresh ? std::min(r + 1, R) : R;
    const bool fuse_env = !getenv("GK_PROMOTE_FUSE") || atoi(getenv("GK_PROMOTE_FUSE")) != 0;  // (per call: A/B, tests)
    bool fuse = fuse_env && r < R;
    for (int c = r; c < c_end; ++c) fuse = fuse && h->st.alloc[c] > 0 && !h->big[c];
    if (fuse) {
      ran = false;
      GKIngestLaunch promote;
      promote.pmode = 1;
      for (int c = r; c < c_end; ++c) {
        ran = true;
        HIP_TRY(launch_class(h, a, c, ovf_list(h, r - 1), ovf_count(h, r - 1), r, stream, promote));
        if (g_trace) {
          HIP_TRY(hipStreamSynchronize(stream));
          GK_TR("round %d: class %d promoted + re-run (fused)", r, c);
        }
      }
      continue;
    }
    HIP_TRY(gk_launch_promote_dev(h->st, ovf_count(h, r - 1), ovf_list(h, r - 1), -1, pool, stream));
    if (g_trace) {
      HIP_TRY(hipStreamSynchronize(stream));
      GK_TR("round %d: promoted", r);
    }
    if (r == R) break;  // the last promotion only counts what no class can hold
    ran = false;
    for (int c = r; c < (fresh ? r + 1 : R); ++c) {
      ran |= h->st.alloc[c] > 0;  // (launch_class launches nothing without slots)
      HIP_TRY(launch_class(h, a, c, h->d_rerun[c], rcnt + c, r, stream));
      if (g_trace) {
        HIP_TRY(hipStreamSynchronize(stream));
        GK_TR("round %d: class %d re-run done", r, c);
      }
    }
  }
  return GK_OK;
}

int run_ingest(gk_set* h, const GKBatch& call, hipStream_t stream, bool prio) {
  const int R = h->st.nclass;
  const bool fresh = h->no_members;  // (promote_rounds clears it)
  GKBatch& a = h->last;
  a = call;
  if (!a.offs) a.offs = h->d_zero_offs;
  h->last.may_defer = false;
  for (int c = 1; c < R; ++c) h->last.may_defer |= h->st.alloc[c] < h->S;
  // (the call's counters were zeroed by begin_call)
  // timing covers the class-0 batch launch of gk_ingest (x given) only
  const bool timed = h->timing && a.x != nullptr;
  // the longest presorted streams of an ingest: one workgroup each, on aux2
  // right behind their presort, beside the class-0 launch (which skips them)
  // (a stream whose batches are not presorted -- no workspace yet, or it did
  // not fit -- is ranked unsorted there)
  const bool wg = prio && a.x != nullptr && h->ps.wg_count && h->aux2 && h->ps.list_ws;
  // The small-class launch alone records the pair as part of its dispatch
  // (the kernel's own start and end; two marker packets around it cost the
  // step ~12 us of dispatch gaps); with k_ingest_wg beside it the markers
  // span both launches.
  bool ext = timed && !wg && h->st.cap[0] == GK_SMALL_CAP && !h->big[0];
  hipEvent_t t0 = timed ? timing_event(h->tev_flush, h->n_flush) : nullptr;
  hipEvent_t t1x = (ext && t0) ? timing_event(h->tev_flush, h->n_flush) : nullptr;
  if (ext && !t1x) {  // (no second event: markers, paired as before)
    ext = false;
    if (t0) --h->n_flush;
    t0 = timed ? timing_event(h->tev_flush, h->n_flush) : nullptr;
  }
  if (t0 && !ext) HIP_TRY(hipEventRecord(t0, stream));
  if (wg && !h->owed.wg) {  // (not launched early by stats_fork)
    unsigned long long* wwork = work_counter(h, false);
    if (!wwork) return fail(GK_E_HIP, "no hand-out counter left for k_ingest_wg");
    // (behind k_long_prep, which counts its streams, and the call's counter
    // reset: the fork point; the presort, when there is one, is already
    // ordered after it on aux2)
    const int rl = launch_wg(h, a.x, a.offs, a.force, wwork, h->ev_fork, nullptr);
    if (rl) return rl;
  }
  // class 0; an ingest's batch: the long streams first (presorted batches;
  // not k_ingest_wg's streams), the stats role in the small class
  GKIngestLaunch L0;
  if (prio && a.x != nullptr) {
    L0.prio = h->d_long_list;
    L0.prio_count = h->d_long_count;
    if (h->ps.ws) {
      L0.psort = h->ps.ws;
      L0.prio_ws = h->ps.list_ws;
    }
    if (wg) L0.prio_skip = h->ps.wg_count;
    if (stats_fused(h)) L0.fused_stats = h->fused_stats;
  }
  if (ext) {
    L0.ev_start = t0;
    L0.ev_stop = t1x;
  }
  const hipError_t lc = launch_class(h, a, 0, nullptr, nullptr, 0, stream, L0);
  // (its overflow entries feed the promotion rounds below).  k_ingest_wg is
  // joined on every path once launched: the next call's begin_call zeroes the
  // counter block it adds to
  const int rw = join_owed(h, stream, true, true);
  if (rw) return rw;
  HIP_TRY(lc);
  // (with k_ingest_wg beside it, the timed span is both: the call's batch ingest)
  hipEvent_t t1 = (timed && !ext) ? timing_event(h->tev_flush, h->n_flush) : nullptr;
  if (t1) HIP_TRY(hipEventRecord(t1, stream));
  if (!h->no_members)
    for (int c = 1; c < R; ++c) HIP_TRY(launch_class(h, a, c, h->d_list[c], h->d_ctr + GK_CTR_LCNT + c, 0, stream));
  return promote_rounds(h, a, stream, fresh);
}

// The capacity-level ladder of the synchronous folds (merge, merge_compress,
// roll-up): `launch` runs at level 0 over every stream of dst, then at each
// further level over the streams that did not fit the level before -- their
// class is raised on the device first (the arena grown for them), so that
// their output may grow.  One overflow readback per level.
// launch(level, cap, list, count, ovf_count, ovf_list, ws, ws_bytes,
// ws_blocks) -> hipError_t: list is NULL at level 0 (count = dst->S), ws NULL
// for an LDS capacity; it reads dst->st at the call (the arenas move).
// overflow_fmt: the GK_E_OVERFLOW message past the last level, taking the
// stream count (%lld) and the largest capacity (%d).
template <typename Launch>
int run_levels(gk_set* dst, hipStream_t s, Launch&& launch, const char* overflow_fmt) {
  const GKPoolDev pool = pool_args(dst);
  int64_t todo = 0;
  dst->ctr_clean = false;
  HIP_TRY(hipMemsetAsync(dst->d_ovfc, 0, kRounds * sizeof(int32_t), s));
  for (int level = 0; level < dst->st.nclass; ++level) {
    const int cap = dst->st.cap[level];
    if (level > 0) {
      if (todo == 0) return GK_OK;
      int rc = grow_class(dst, level, (int64_t)dst->st.alloc[level] + todo, s);
      if (rc) return rc;
      dst->no_members = false;
      HIP_TRY(gk_launch_promote_dev(dst->st, ovf_count(dst, level - 1), ovf_list(dst, level - 1), level, pool, s));
    }
    const bool lds = cap <= kMaxLdsCap;
    if (!lds) {
      int rc = ensure_ws(dst, level);
      if (rc) return rc;
    }
    HIP_TRY(launch(level, cap, level == 0 ? nullptr : ovf_list(dst, level - 1), level == 0 ? dst->S : todo,
                   ovf_count(dst, level), ovf_list(dst, level), lds ? nullptr : dst->d_ws[level],
                   lds ? 0 : dst->ws_bytes[level], lds ? 0 : dst->ws_blocks[level]));
    todo = read_overflow(dst, level, s);
    if (todo < 0) return (int)todo;
    if (todo == 0) return GK_OK;
  }
  return fail(GK_E_OVERFLOW, overflow_fmt, (long long)todo, dst->st.cap[dst->st.nclass - 1]);
}

const char* const kMergeOverflow =
    "%lld stream(s) exceed %d table entries in merge, or the per-stream count limit "
    "2*eps*(n-1) <= 2^30";
const char* const kRollupOverflow =
    "%lld destination stream(s) exceed %d table entries in roll-up, or the per-stream count "
    "limit 2*eps*(n-1) <= 2^30: they hold the fold of the members before the one that did not fit";

// A fold (k_fold: merge, explicit merge_compress, roll-up) up the ladder; base
// holds what stays the same at every level.  base.list / base.count
// (optional): only these streams at level 0 instead of every stream.  A
// destination whose fold stopped at a step that did not fit resumes at the
// recorded step one level up.
int run_fold(gk_set* dst, const FoldArgs& base, const char* overflow_fmt, hipStream_t s) {
  FoldArgs a = base;
  return run_levels(
      dst, s,
      [&](int level, int cap, const int32_t* list, int64_t count, int32_t* ovf_count, int32_t* ovf_list,
          unsigned char* ws, size_t ws_bytes, int64_t ws_blocks) {
        const bool own = level == 0 && base.list;
        a.dst = dst->st;
        a.resume = level > 0;
        a.cap = cap;
        a.list = own ? base.list : list;
        a.count = own ? base.count : count;
        a.ovf_count = ovf_count;
        a.ovf_list = ovf_list;
        a.ws = ws;
        a.ws_bytes = ws_bytes;
        a.ws_blocks = ws_blocks;
        return gk_launch_fold(a, s);
      },
      overflow_fmt);
}

// k_fold's explicit-record step with no records over the n streams of `list`
// (device): merge_compress() of each; a stream that needs a larger class for
// it climbs the ladder.
int flush_listed(gk_set* h, const int32_t* list, int64_t n, hipStream_t s) {
  if (n <= 0) return GK_OK;
  FoldArgs a{};
  a.eoffs = h->d_zero_offs;
  a.list = list;
  a.count = n;
  return run_fold(h, a, kMergeOverflow, s);
}

// The device work of one ingest / flush call on `s`: the one body of gk_ingest,
// gk_ingest_quantiles, gk_flush, gk_quantiles and flush_source, which keep
// their checks, early returns, grow_pools and query staging (their order is
// the error precedence).  with_stats: the call adds values -- the gk:52-59
// chains run beside the ingest, the long streams go first, the long-stream
// count comes back with the counters.  The join and the readback are enqueued
// whatever the ingest returned; the first failure of the three is returned.
int ingest_call(gk_set* h, const double* x, const int64_t* offs, int force, const GKQuery& q, bool with_stats,
                hipStream_t s, bool sticky = true) {
  int rc = sticky ? take_sticky(h) : GK_OK;
  if (!rc) rc = begin_call(h, s);
  if (rc) return rc;
  if (with_stats) {
    rc = stats_fork(h, x, offs, s, force);
    if (rc) {
      stats_abort(h, s);
      return rc;
    }
  }
  rc = run_ingest(h, GKBatch{x, offs, force, q}, s, with_stats);
  const int rj = with_stats ? stats_join(h, s, q) : GK_OK;  // joined on every path
  const int rd = mark_done(h, s, with_stats);
  return rc ? rc : (rj ? rj : rd);
}

// other.merge_compress() of every stream of a fold's source -- unconditional
// in the reference (gk:126, 137) -- as one batch flush, settled on return.
int flush_source(gk_set* src, hipStream_t s, void* stream) {
  int rc = ingest_call(src, nullptr, nullptr, 2, GKQuery(), false, s, false);
  if (!rc) rc = gk_sync(src, stream);
  return rc;
}

}  // namespace

extern "C" {

int gk_version(void) { return 100; }

const char* gk_last_error(void) { return g_err.c_str(); }

int gk_create(int64_t num_streams, double eps, int64_t cap_hint, int device, gk_set** out) {
  if (!out) return fail(GK_E_ARG, "out is null");
  *out = nullptr;
  if (num_streams < 0 || num_streams > INT32_MAX) return fail(GK_E_ARG, "num_streams out of range");
  // any finite eps > 0, as the reference (gk:21); eps > 1 gives P = 1 (gk:60)
  if (!std::isfinite(eps) || !(eps > 0.0)) return fail(GK_E_ARG, "eps must be finite and > 0");
  const double inv = 1.0 / eps;
  if (inv >= (double)kPMax)
    return fail(GK_E_UNSUPPORTED, "eps=%g: flush period int(1/eps)+1 beyond %d is not supported", eps, kPMax);
  if (cap_hint < 0 || cap_hint >= kCapMax) return fail(GK_E_UNSUPPORTED, "cap_hint %lld out of range", (long long)cap_hint);
  std::vector<int> caps;
  std::vector<bool> force_big;
  if (const char* e = getenv("GK_CAPS")) {  // tests: an explicit ladder, "128,2048,4096b" (b: k_ingest_big)
    for (const char* t = e; *t;) {
      char* end = nullptr;
      const long v = strtol(t, &end, 10);
      if (end == t) return fail(GK_E_ARG, "GK_CAPS=%s: bad list", e);
      caps.push_back((int)v);
      force_big.push_back(*end == 'b');
      t = end + (*end == 'b');
      if (*t == ',') ++t;
    }
    const double P0 = (double)((int)inv + 1);
    bool okc = !caps.empty() && (int)caps.size() <= GK_MAX_CLASSES;
    for (size_t c = 0; okc && c < caps.size(); ++c) {
      okc = caps[c] >= 64 && caps[c] <= kCapMax && (c == 0 || caps[c] > caps[c - 1]);
      if (caps[c] == kCapSmall) okc = okc && c == 0 && P0 <= 128;
    }
    if (!okc) return fail(GK_E_ARG, "GK_CAPS=%s: increasing capacities in [64, %d], 128 only first", e, kCapMax);
  }
  int dev_count = 0;
  if (hipGetDeviceCount(&dev_count) != hipSuccess || dev_count <= 0)
    return fail(GK_E_HIP, "no HIP device available");
  if (device < 0 || device >= dev_count) return fail(GK_E_ARG, "device %d out of range", device);
  HIP_TRY(hipSetDevice(device));

  gk_set* h = new gk_set();
  h->S = num_streams;
  h->eps = eps;
  h->P = (int)inv + 1;  // gk:60
  h->device = device;
  h->vpl = h->P <= 1024 ? vpl_for(h->P) : 0;  // (registers of the capacity-class kernels)
  if (const char* fs = getenv("GK_FUSED_STATS")) h->fused_stats = std::max(0, std::min(64, atoi(fs)));
  GKState& st = h->st;
  st.S = num_streams;
  st.eps = eps;
  st.two_eps = 2.0 * eps;
  st.inv_eps = inv;
  st.P = h->P;
  st.pmax = h->P;
  // Capacity ladder.  Class 0 (every stream) is the 128-entry LDS class when
  // a flush period fits two values per lane (iid tables at eps=0.01 stay at
  // <= ~106 entries); adversarial streams are promoted to 2048
  // (LDS), 32768 (global workspace) and then the unbounded classes of
  // k_ingest_big.  With P > 1024 (eps < 1/1023) every class is k_ingest_big:
  // class 0 of 2P entries (iid tables hold ~P/2..P), then x16 steps.
  auto pow2_at_least = [](int64_t v) {
    int64_t c = 1;
    while (c < v) c <<= 1;
    return c;
  };
  if (caps.empty()) {
    if (h->P <= 1024) {
      if (h->P <= 128 && cap_hint <= kCapSmall) caps = {kCapSmall, kCapLarge, kCapHuge, kCapBig};
      else if (cap_hint <= kCapLarge) caps = {kCapLarge, kCapHuge, kCapBig};
      else if (cap_hint < kCapHuge) caps = {kCapHuge, kCapBig};
    }
    if (caps.empty()) {
      int64_t c = std::max<int64_t>({4096, pow2_at_least(2 * (int64_t)h->P), pow2_at_least(cap_hint + 1)});
      for (; (int)caps.size() < GK_MAX_CLASSES && c <= kCapMax; c *= 16) caps.push_back((int)c);
      if (caps.back() < kCapMax && (int)caps.size() < GK_MAX_CLASSES) caps.push_back(kCapMax);
    }
  }
  st.nclass = (int)caps.size();
  for (int c = 0; c < GK_MAX_CLASSES; ++c) {
    st.cap[c] = c < st.nclass ? caps[c] : 0;
    const bool lds = (st.cap[c] == kCapSmall && c == 0) || st.cap[c] == kCapLarge;
    h->big[c] = c < st.nclass && (h->P > 1024 || st.cap[c] > kCapHuge || (!force_big.empty() && force_big[c]) ||
                                  (st.cap[c] <= kMaxLdsCap && !lds));
  }
  const int64_t S = std::max<int64_t>(num_streams, 1);
  bool okm = true;
  okm &= hipMalloc(&st.n, S * sizeof(int64_t)) == hipSuccess;
  okm &= hipMalloc(&st.E, S * sizeof(int32_t)) == hipSuccess;
  okm &= hipMalloc(&st.pend, S * sizeof(int32_t)) == hipSuccess;
  okm &= hipMalloc(&st.mn, S * sizeof(double)) == hipSuccess;
  okm &= hipMalloc(&st.mx, S * sizeof(double)) == hipSuccess;
  okm &= hipMalloc(&st.sum, S * sizeof(double)) == hipSuccess;
  okm &= hipMalloc(&st.avg, S * sizeof(double)) == hipSuccess;
  okm &= hipMalloc(&st.cls, S * sizeof(int32_t)) == hipSuccess;
  okm &= hipMalloc(&st.slot, S * sizeof(int32_t)) == hipSuccess;
  okm &= hipMalloc(&st.tab[0], (size_t)S * st.cap[0] * sizeof(GKRec)) == hipSuccess;
  okm &= hipMalloc(&st.pbuf, (size_t)S * st.pmax * sizeof(double)) == hipSuccess;
  st.rtab_n = kRecipTable;
  okm &= hipMalloc(&st.rtab, (size_t)st.rtab_n * sizeof(double)) == hipSuccess;
  okm &= hipMalloc(&st.n0, S * sizeof(int64_t)) == hipSuccess;

  for (int r = 0; r < kRounds; ++r) okm &= hipMalloc(&h->d_ovfl[r], S * sizeof(int32_t)) == hipSuccess;
  okm &= hipHostMalloc(&h->h_ovf, 16 * sizeof(int32_t)) == hipSuccess;
  okm &= hipMalloc(&h->d_ctr, GK_CALL_BYTES) == hipSuccess;
  if (h->d_ctr) {
    h->d_ovfc = h->d_ctr + GK_CTR_OVFC;
    h->d_long_count = h->d_ctr + GK_CTR_LONG;
    h->d_work = (unsigned long long*)((char*)h->d_ctr + GK_CALL_WORK);
  }
  okm &= hipHostMalloc(&h->h_ctr, (GK_CTR_WORDS + 1) * sizeof(int32_t)) == hipSuccess;  // + the call's wg count
  okm &= hipMalloc(&h->d_defer, S * sizeof(int32_t)) == hipSuccess;
  if (h->h_ctr) memset(h->h_ctr, 0, GK_CTR_WORDS * sizeof(int32_t));
  okm &= hipEventCreateWithFlags(&h->ev_done, hipEventDisableTiming) == hipSuccess;
  okm &= hipEventCreateWithFlags(&h->ev_qs, hipEventDisableTiming) == hipSuccess;
  st.alloc[0] = (int32_t)S;
  for (int c = 1; c < st.nclass; ++c) {
    okm &= hipMalloc(&h->d_list[c], S * sizeof(int32_t)) == hipSuccess;
    okm &= hipMalloc(&h->d_rerun[c], S * sizeof(int32_t)) == hipSuccess;
    const int64_t n = initial_slots(h, c);
    if (n > 0) okm &= hipMalloc(&st.tab[c], (size_t)n * st.cap[c] * sizeof(GKRec)) == hipSuccess;
    st.alloc[c] = (int32_t)n;
  }
  okm &= hipMalloc(&h->d_zero_offs, (S + 1) * sizeof(int64_t)) == hipSuccess;

  okm &= hipMalloc(&h->d_long_list, S * sizeof(int32_t)) == hipSuccess;
  okm &= hipMalloc(&h->d_long_n, S * sizeof(int64_t)) == hipSuccess;

  okm &= hipStreamCreateWithFlags(&h->aux, hipStreamNonBlocking) == hipSuccess;
  // (aux2 only where the presort runs: every stream of a process shares the
  // box's 4 hardware queues, and a set's idle stream still takes a slot in
  // their round-robin -- with 8 sets of 3 streams the cfg4 shards' long
  // chains landed behind the next shard's ingest)
  if (h->P > 128 && !h->big[0]) okm &= hipStreamCreateWithFlags(&h->aux2, hipStreamNonBlocking) == hipSuccess;
  okm &= hipEventCreateWithFlags(&h->ev_presort, hipEventDisableTiming) == hipSuccess;
  okm &= hipEventCreateWithFlags(&h->ev_fork, hipEventDisableTiming) == hipSuccess;
  okm &= hipEventCreateWithFlags(&h->ev_slgo, hipEventDisableTiming) == hipSuccess;
  okm &= hipEventCreateWithFlags(&h->ev_join, hipEventDisableTiming) == hipSuccess;
  if (h->P > 128 && !h->big[0]) {  // class 0 is a capacity-class kernel: presort long streams' batches
    okm &= hipMalloc(&h->ps.list_ws, S * sizeof(int64_t)) == hipSuccess;
    okm &= hipMalloc(&h->ps.list_b0, (S + 1) * sizeof(int64_t)) == hipSuccess;
    okm &= hipMalloc(&h->ps.ws_need, sizeof(int64_t)) == hipSuccess;
    okm &= hipHostMalloc(&h->h_ws_need, sizeof(int64_t)) == hipSuccess;
    if (h->h_ws_need) *h->h_ws_need = 0;
    // the longest streams: one workgroup each (k_ingest_wg, 2048 class,
    // P <= 1024; GK_WG=0 turns it off); their count is a per-call word.
    // Their batches are presorted (GK_WG_PRESORT=0: not; k_ingest_wg then
    // ranks each value among its gap's members)
    bool wg = st.cap[0] == 2048 && h->P <= 1024;
    if (const char* e = getenv("GK_WG")) wg = wg && atoi(e) != 0;
    if (wg) h->ps.wg_count = h->d_ctr + GK_CTR_WG;
    h->ps.wg_presort = 1;
    if (const char* e = getenv("GK_WG_PRESORT")) h->ps.wg_presort = atoi(e) != 0;
    // the register presort beside k_ingest_wg (which takes presorted batches
    // once it is done and ranks unsorted ones until then); GK_WG_CONC=0: the
    // workgroups wait for the presort
    bool conc = wg && h->ps.wg_presort && gk_presort_reg_grid(st) > 0;
    if (const char* e = getenv("GK_WG_CONC")) conc = conc && atoi(e) != 0;
    if (conc) {
      h->ps.done = h->d_ctr + GK_CTR_PSDONE;
      okm &= hipStreamCreateWithFlags(&h->aux3, hipStreamNonBlocking) == hipSuccess;
    }
    h->wg_trace = getenv("GK_WG_TRACE") != nullptr;
    okm &= hipEventCreateWithFlags(&h->ev_wg, hipEventDisableTiming) == hipSuccess;
    okm &= hipEventCreateWithFlags(&h->ev_go, hipEventDisableTiming) == hipSuccess;
  }
  if (!okm) {
    gk_destroy(h);
    return fail(GK_E_NOMEM, "device allocation for %lld streams failed", (long long)num_streams);
  }
  for (int c = 0; c < st.nclass; ++c) {  // classes with slots: their workspace (entered inside any call)
    if (st.alloc[c] > 0 && ensure_ws(h, c) != GK_OK) {
      gk_destroy(h);
      return GK_E_NOMEM;
    }
  }
  if (hipMemset(st.cls, 0, S * sizeof(int32_t)) != hipSuccess ||
      hipMemset(h->d_ctr, 0, GK_CALL_BYTES) != hipSuccess ||
      hipMemset(h->d_zero_offs, 0, (S + 1) * sizeof(int64_t)) != hipSuccess ||
      hipMemset(st.slot, 0, S * sizeof(int32_t)) != hipSuccess || gk_launch_reset(st, nullptr) != hipSuccess ||
      gk_launch_rtab(st, nullptr) != hipSuccess ||
      hipDeviceSynchronize() != hipSuccess) {
    gk_destroy(h);
    return fail(GK_E_HIP, "state initialisation failed");
  }
  *out = h;
  return GK_OK;
}

int gk_destroy(gk_set* h) {
  if (!h) return GK_OK;
  (void)hipDeviceSynchronize();  // launches of this set may still be running on the caller's stream
  if (h->fold_scratch) gk_destroy(h->fold_scratch);
  if (h->self_scratch) gk_destroy(h->self_scratch);
  GKState& st = h->st;
  void* ptrs[] = {st.n,       st.E,          st.pend,        st.mn,          st.mx,          st.sum,
                  st.avg,     st.cls,        st.slot,        st.pbuf,        h->d_qs,
                  h->d_ctr,   h->d_zero_offs, h->d_long_list, h->d_long_n,
                  h->ps.list_ws, h->ps.list_b0, h->ps.ws,    h->ps.ws_need,  st.rtab,        st.n0,
                  h->d_defer, h->d_roll_prog,
                  h->kg.ids[0], h->kg.ids[1], h->kg.vals[0], h->kg.vals[1],  h->kg.hist,     h->kg.sums,
                  h->kg.call, h->kg_vals,    h->kg_offs,     h->d_sel,       h->rk_idx};
  for (void* p : ptrs)
    if (p) (void)hipFree(p);
  for (int c = 0; c < GK_MAX_CLASSES; ++c)
    for (void* p : {(void*)st.tab[c], (void*)h->d_list[c], (void*)h->d_rerun[c], (void*)h->d_ws[c]})
      if (p) (void)hipFree(p);
  for (int r = 0; r < kRounds; ++r)
    if (h->d_ovfl[r]) (void)hipFree(h->d_ovfl[r]);
  for (auto* v : {&h->tev_flush, &h->tev_stats})
    for (hipEvent_t e : *v) (void)hipEventDestroy(e);
  for (hipEvent_t e : {h->ev_fork, h->ev_join, h->ev_slgo, h->ev_done, h->ev_qs})
    if (e) (void)hipEventDestroy(e);
  if (h->aux2) (void)hipStreamDestroy(h->aux2);
  if (h->aux3) (void)hipStreamDestroy(h->aux3);
  if (h->ev_presort) (void)hipEventDestroy(h->ev_presort);
  if (h->ev_wg) (void)hipEventDestroy(h->ev_wg);
  if (h->ev_go) (void)hipEventDestroy(h->ev_go);
  if (h->aux) (void)hipStreamDestroy(h->aux);
  for (void* p : {(void*)h->h_ws_need, (void*)h->h_ovf, (void*)h->h_ctr, (void*)h->h_qs, (void*)h->h_kg})
    if (p) (void)hipHostFree(p);
  delete h;
  return GK_OK;
}

int gk_reset(gk_set* h, void* stream) {
  int rc = check_set(h);
  if (rc) return rc;
  hipStream_t s = (hipStream_t)stream;
  // No wait for the last call: streams it deferred for
  // want of a slot would only be re-run to be reset; their re-run is void.
  // (Waiting here put the host's enqueueing of every step on the GPU's
  // critical path: ~90 us of idle GPU per step, 10 % of a 125k-stream rank
  // share.)  The last call's counters are consumed when they arrive: its
  // sticky errors are still reported, its deferred list is dropped.
  // The exception is a call with a fused query (gk_ingest_quantiles,
  // gk_ingest_keyed with qs): the answers of a stream it deferred are written
  // by the re-run alone, so that call is settled first, as before any other
  // call.  (A plain gk_ingest, the rank share's step, never takes this wait,
  // nor does a fused-query call that a later call or gk_sync has settled.)
  if (h->last.q.out && h->last.may_defer) {
    rc = settle(h, s, false);
    if (rc) return rc;
  }
  poll(h, false);
  if (h->done_pending) h->void_defer = true;
  else h->h_ctr[GK_CTR_DEFER] = 0;
  h->last.may_defer = false;
  // (k_reset puts every stream back in class 0: cls = slot = 0)
  // slots, member lists and re-run lists start over (FATAL stays cumulative:
  // a readback still in flight carries it)
  // (+ counter words [0, GK_CTR_FATAL) and the per-call block: no separate
  // memset, and none at the next call's begin_call)
  HIP_TRY(gk_launch_reset(h->st, s, h->d_ctr));
  h->no_members = true;
  h->ctr_clean = true;
  return GK_OK;
}

int gk_ingest(gk_set* h, const double* values, const int64_t* offsets, void* stream) {
  int rc = check_set(h);
  if (rc) return rc;
  if (!offsets) return fail(GK_E_ARG, "offsets is null");
  if (!values) return fail(GK_E_ARG, "values is null");
  if (h->S == 0) return GK_OK;
  hipStream_t s = (hipStream_t)stream;
  rc = grow_pools(h, s);
  return rc ? rc : ingest_call(h, values, offsets, 0, GKQuery(), true, s);
}

// The grouping scratch for `count` samples (and, grouped: the set-owned
// grouped batch).  Growing synchronises `s` first: earlier launches may still
// use the buffers (the caller has settled the last call: nothing is re-run
// from them any more).
static int ensure_group_scratch(gk_set* h, int64_t count, bool grouped, hipStream_t s) {
  const int64_t n = std::max<int64_t>(count, 1);
  // pass p writes ids[p & 1] and, unless it is the last, vals[p & 1]
  const int passes = gk_group_passes(h->S), pairs = std::min(passes, 2), vbufs = std::min(passes - 1, 2);
  const int64_t tiles = std::max<int64_t>(gk_group_tiles(n), 1), sums = gk_group_sums(n);
  const bool first = !h->kg.call;
  const bool grow_pairs = pairs > 0 && (n > h->kg_cap || pairs > h->kg_pairs), grow_hist = tiles > h->kg_tiles,
             grow_sums = sums > h->kg_sums, grow_vals = grouped && (n > h->kg_vals_cap || !h->kg_offs);
  if (!(first || grow_pairs || grow_hist || grow_sums || grow_vals)) return GK_OK;
  HIP_TRY(hipStreamSynchronize(s));
  bool ok = true;
  if (first) {
    // per-call words and, behind them, the cumulative block: one allocation
    ok = renew_dev(&h->kg.call, (GK_KG_CALL_WORDS + GK_KG_CUM_WORDS) * sizeof(unsigned long long)) &&
         hipMemset(h->kg.call, 0, (GK_KG_CALL_WORDS + GK_KG_CUM_WORDS) * sizeof(unsigned long long)) == hipSuccess &&
         hipHostMalloc(&h->h_kg, GK_KG_CUM_WORDS * sizeof(unsigned long long)) == hipSuccess;
    if (ok) {
      memset(h->h_kg, 0, GK_KG_CUM_WORDS * sizeof(unsigned long long));
      h->kg.cum = h->kg.call + GK_KG_CALL_WORDS;
    } else {
      if (h->kg.call) (void)hipFree(h->kg.call);
      h->kg.call = nullptr;
    }
  }
  if (ok && grow_pairs) {
    const int64_t cap = std::max(n, h->kg_cap);
    h->kg_cap = 0;
    h->kg_pairs = 0;
    for (int k = 0; k < 2 && ok; ++k) {
      if (k < pairs) ok = renew_dev(&h->kg.ids[k], (size_t)cap * sizeof(int32_t));
      if (ok && k < vbufs) ok = renew_dev(&h->kg.vals[k], (size_t)cap * sizeof(double));
    }
    if (ok) {
      h->kg_cap = cap;
      h->kg_pairs = pairs;
    }
  }
  if (ok && grow_hist) {
    h->kg_tiles = 0;
    ok = renew_dev(&h->kg.hist, ((size_t)tiles << GK_GROUP_BITS) * sizeof(uint32_t));
    if (ok) h->kg_tiles = tiles;
  }
  if (ok && grow_sums) {
    h->kg_sums = 0;
    ok = renew_dev(&h->kg.sums, (size_t)sums * sizeof(unsigned long long));
    if (ok) h->kg_sums = sums;
  }
  if (ok && grow_vals) {
    const int64_t cap = std::max(n, h->kg_vals_cap);
    h->kg_vals_cap = 0;
    ok = renew_dev(&h->kg_vals, (size_t)cap * sizeof(double)) &&
         (h->kg_offs || renew_dev(&h->kg_offs, (size_t)(h->S + 1) * sizeof(int64_t)));
    if (ok) h->kg_vals_cap = cap;
  }
  if (!ok) return fail(GK_E_NOMEM, "grouping scratch for %lld samples failed", (long long)count);
  return GK_OK;
}

static int check_keyed_args(const int32_t* ids, const double* values, int64_t count) {
  int rc = check_count(count);
  if (rc) return rc;
  if (count > 0 && (!ids || !values)) return fail(GK_E_ARG, "ids or values is null");
  return GK_OK;
}

int gk_group_by_key(gk_set* h, const int32_t* ids, const double* values, int64_t count, double* out_values,
                    int64_t* out_offsets, void* stream) {
  int rc = check_set(h);
  if (!rc) rc = check_keyed_args(ids, values, count);
  if (rc) return rc;
  if (!out_offsets) return fail(GK_E_ARG, "out_offsets is null");
  if (count > 0 && !out_values) return fail(GK_E_ARG, "out_values is null");
  hipStream_t s = (hipStream_t)stream;
  rc = settle(h, s, false);
  if (!rc) rc = take_sticky(h);
  if (!rc) rc = ensure_group_scratch(h, count, false, s);
  if (rc) return rc;
  HIP_TRY(gk_launch_group_by_key(h->kg, ids, values, count, h->S, out_values, out_offsets, s));
  return mark_done(h, s);  // (the bad-id block comes back with the counters)
}

int gk_ingest_keyed(gk_set* h, const int32_t* ids, const double* values, int64_t count, const double* qs, int nq,
                    double* out, int mode, void* stream) {
  int rc = check_set(h);
  if (!rc) rc = check_query_args(qs, nq, out, mode);  // (ahead of the grouping)
  if (!rc) rc = check_keyed_args(ids, values, count);
  if (rc) return rc;
  if (h->S == 0) return GK_OK;
  hipStream_t s = (hipStream_t)stream;
  // The last call is settled BEFORE the grouping is enqueued: its deferred
  // streams are re-run from its inputs, which for a keyed call are kg_vals /
  // kg_offs -- the buffers this grouping rewrites.
  rc = grow_pools(h, s);
  if (!rc) rc = take_sticky(h);
  if (!rc) rc = ensure_group_scratch(h, count, true, s);
  if (rc) return rc;
  HIP_TRY(gk_launch_group_by_key(h->kg, ids, values, count, h->S, h->kg_vals, h->kg_offs, s));
  // exactly the CSR path on the grouped batch (its own settle finds the last
  // call settled; a bad id left kg_offs all zero: an empty batch)
  if (nq == 0) return gk_ingest(h, h->kg_vals, h->kg_offs, stream);
  return gk_ingest_quantiles(h, h->kg_vals, h->kg_offs, qs, nq, out, mode, stream);
}

int gk_flush(gk_set* h, void* stream) {
  int rc = check_set(h);
  if (rc) return rc;
  if (h->S == 0) return GK_OK;
  hipStream_t s = (hipStream_t)stream;
  rc = grow_pools(h, s);
  return rc ? rc : ingest_call(h, nullptr, nullptr, 1, GKQuery(), false, s);
}

int gk_sync(gk_set* h, void* stream) {
  int rc = check_set(h);
  if (rc) return rc;
  HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
  rc = settle(h, (hipStream_t)stream, true);
  return rc ? rc : take_sticky(h);
}

static int stage_qs(gk_set* h, const double* qs, int nq, hipStream_t s);

// quantile arguments -> device copy of qs and the effective mode
static int prepare_query(gk_set* h, const double* qs, int nq, double* out, int mode, hipStream_t s, GKQuery* q) {
  int rc = check_query_args(qs, nq, out, mode);
  if (rc) return rc;
  // gk:205-206: an unsorted list is answered q by q with quantile()
  int eff_mode = mode;
  if (mode == GK_Q_LIST) {
    for (int i = 1; i < nq; ++i)
      if (qs[i] < qs[i - 1]) {
        eff_mode = GK_Q_SINGLE;
        break;
      }
  }
  rc = stage_qs(h, qs, nq, s);
  if (rc) return rc;
  q->qs = nq ? h->d_qs : nullptr;
  q->nq = nq;
  q->out = out;
  q->mode = eff_mode;
  return GK_OK;
}

// nq host doubles (quantiles, or the thresholds of a rank query) into the
// set's device copy d_qs
static int stage_qs(gk_set* h, const double* qs, int nq, hipStream_t s) {
  // the previous call's copy out of h_qs (and its kernels' reads of d_qs,
  // ordered on the same stream) must not see the new values
  HIP_TRY(hipEventSynchronize(h->ev_qs));
  if (nq > h->qs_alloc) {
    HIP_TRY(hipStreamSynchronize(s));
    if (h->h_qs) (void)hipHostFree(h->h_qs);
    h->h_qs = nullptr;
    const int cap = std::max(nq, 64);
    if (!renew_dev(&h->d_qs, cap * sizeof(double)) || hipHostMalloc(&h->h_qs, cap * sizeof(double)) != hipSuccess)
      return fail(GK_E_NOMEM, "qs allocation failed");
    h->qs_alloc = cap;
    h->qs_n = 0;
  }
  // (the same list as the last upload -- every step of a serving loop --
  // is already on the device: no copy, no blit launch)
  if (nq && !(nq == h->qs_n && memcmp(h->h_qs, qs, nq * sizeof(double)) == 0)) {
    memcpy(h->h_qs, qs, nq * sizeof(double));
    HIP_TRY(hipMemcpyAsync(h->d_qs, h->h_qs, nq * sizeof(double), hipMemcpyHostToDevice, s));
    HIP_TRY(hipEventRecord(h->ev_qs, s));
    h->qs_n = nq;
  }
  return GK_OK;
}

int gk_quantiles(gk_set* h, const double* qs, int nq, double* out, int mode, void* stream) {
  int rc = check_set(h);
  if (rc) return rc;
  hipStream_t s = (hipStream_t)stream;
  // settle the previous call first: a deferred stream of it is re-run with
  // that call's query (h->last.q reads d_qs), which the upload below replaces
  rc = grow_pools(h, s);
  if (rc) return rc;
  GKQuery q;
  rc = prepare_query(h, qs, nq, out, mode, s, &q);
  if (rc) return rc;
  if (nq == 0 || h->S == 0) return GK_OK;
  // gk:197-198: pending values are flushed first (state mutation); the
  // quantiles are answered in the same launch from the flushed table
  return ingest_call(h, nullptr, nullptr, 1, q, false, s);
}

int gk_ingest_quantiles(gk_set* h, const double* values, const int64_t* offsets, const double* qs, int nq,
                        double* out, int mode, void* stream) {
  int rc = check_set(h);
  if (rc) return rc;
  if (!offsets) return fail(GK_E_ARG, "offsets is null");
  if (!values) return fail(GK_E_ARG, "values is null");
  hipStream_t s = (hipStream_t)stream;
  rc = grow_pools(h, s);  // before d_qs is rewritten (see gk_quantiles)
  if (rc) return rc;
  GKQuery q;
  rc = prepare_query(h, qs, nq, out, mode, s, &q);
  if (rc) return rc;
  if (h->S == 0) return GK_OK;
  if (nq == 0) return gk_ingest(h, values, offsets, stream);
  // add every value (gk:49-61), then quantiles() (gk:187-232): flush the
  // leftover pending values and answer from the LDS-resident table
  return ingest_call(h, values, offsets, 1, q, true, s);
}

int gk_stats(gk_set* h, int64_t* n, double* mn, double* mx, double* sum, double* avg, int32_t* table_size,
             int32_t* pending, void* stream) {
  int rc = check_set(h);
  if (rc) return rc;
  rc = settle(h, (hipStream_t)stream, false);  // a deferred stream of the last call is re-run first
  if (rc) return rc;
  hipStream_t s = (hipStream_t)stream;
  const int64_t S = h->S;
  if (S == 0) return GK_OK;
  if (n) HIP_TRY(hipMemcpyAsync(n, h->st.n, S * sizeof(int64_t), hipMemcpyDeviceToDevice, s));
  if (mn) HIP_TRY(hipMemcpyAsync(mn, h->st.mn, S * sizeof(double), hipMemcpyDeviceToDevice, s));
  if (mx) HIP_TRY(hipMemcpyAsync(mx, h->st.mx, S * sizeof(double), hipMemcpyDeviceToDevice, s));
  if (sum) HIP_TRY(hipMemcpyAsync(sum, h->st.sum, S * sizeof(double), hipMemcpyDeviceToDevice, s));
  if (avg) HIP_TRY(hipMemcpyAsync(avg, h->st.avg, S * sizeof(double), hipMemcpyDeviceToDevice, s));
  if (table_size) HIP_TRY(hipMemcpyAsync(table_size, h->st.E, S * sizeof(int32_t), hipMemcpyDeviceToDevice, s));
  if (pending) HIP_TRY(hipMemcpyAsync(pending, h->st.pend, S * sizeof(int32_t), hipMemcpyDeviceToDevice, s));
  return GK_OK;
}

// ---- per-stream selection: query, flush, reset and stats of a list of streams

static int64_t select_bitmap_words(const gk_set* h, bool want_list) { return want_list ? (h->S + 31) / 32 : 0; }

// The selection scratch: k_select_check's control words, then (want_list) the
// bitmap of listed streams and the flush list, both live at once, then `extra`
// words of the call's own (8-byte aligned: select_extra_at).  Only grows; the
// caller has synchronised `s` (nothing enqueued uses the old buffer).
static int64_t select_extra_at(const gk_set* h, int64_t count, bool want_list) {
  const int64_t at =
      GK_SEL_WORDS + select_bitmap_words(h, want_list) + (want_list ? std::min<int64_t>(count, h->S) : 0);
  return (at + 1) & ~(int64_t)1;
}

static int ensure_select_words(gk_set* h, int64_t words) {
  if (words <= h->sel_words) return GK_OK;
  h->sel_words = 0;
  if (!renew_dev(&h->d_sel, (size_t)words * sizeof(int32_t)))
    return fail(GK_E_NOMEM, "selection scratch of %lld words failed", (long long)words);
  h->sel_words = words;
  return GK_OK;
}

static int ensure_select_scratch(gk_set* h, int64_t count, bool want_list, int64_t extra) {
  return ensure_select_words(h, select_extra_at(h, count, want_list) + extra);
}

// what select_begin found: the listed streams with n > 0 and pending values (device; want_list)
struct Selection {
  int32_t* list = nullptr;
  int64_t nflush = 0;
  int32_t* extra = nullptr;  // the `extra` words asked of select_begin (8-byte aligned)
};

// Head of every selection call: the set and the id list are checked, then the
// call's other arguments (`more`, if any); the set's earlier work is settled (gk_sync:
// deferred streams re-run, sticky errors returned); and, count > 0, ONE kernel
// over ids checks their range and (want_list) lists the streams to flush --
// nothing is mutated before its verdict has been read back.  The caller
// returns at once on an error or count == 0.
static int select_begin(gk_set* h, const int32_t* ids, int64_t count, bool want_list, void* stream, Selection* sel,
                        const std::function<int()>& more = nullptr, int64_t extra = 0) {
  int rc = check_set(h);
  if (!rc) rc = check_select_args(ids, count);
  if (!rc && more) rc = more();
  if (!rc) rc = gk_sync(h, stream);
  if (rc || count == 0) return rc;
  hipStream_t s = (hipStream_t)stream;
  rc = ensure_select_scratch(h, count, want_list, extra);
  if (rc) return rc;
  const int64_t bm = select_bitmap_words(h, want_list);
  int32_t* const ctl = h->d_sel;
  sel->extra = ctl + select_extra_at(h, count, want_list);
  uint32_t* const bitmap = reinterpret_cast<uint32_t*>(ctl + GK_SEL_WORDS);
  sel->list = want_list ? ctl + GK_SEL_WORDS + bm : nullptr;
  HIP_TRY(hipMemsetAsync(ctl, 0, (size_t)(GK_SEL_WORDS + bm) * sizeof(int32_t), s));
  HIP_TRY(gk_launch_select_check(h->st, ids, count, ctl, bitmap, sel->list, s));
  HIP_TRY(hipMemcpyAsync(h->h_ovf, ctl, GK_SEL_WORDS * sizeof(int32_t), hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  if (h->h_ovf[GK_SEL_BAD]) {
    const int64_t first = count - (int64_t)(uint32_t)h->h_ovf[GK_SEL_FIRST];
    int32_t id = 0;
    HIP_TRY(hipMemcpy(&id, ids + first, sizeof(int32_t), hipMemcpyDeviceToHost));
    return fail(GK_E_ARG, "ids[%lld] = %d lies outside [0, %lld)", (long long)first, id, (long long)h->S);
  }
  sel->nflush = h->h_ovf[GK_SEL_COUNT];
  return GK_OK;
}

// End of a selection call that may have promoted streams: the counters (slots
// in use) come back for the next call's grow_pools, and the call synchronises.
static int select_end(gk_set* h, hipStream_t s) {
  int rc = mark_done(h, s);
  if (rc) return rc;
  HIP_TRY(hipStreamSynchronize(s));
  poll(h, true);
  return GK_OK;
}

int gk_flush_select(gk_set* h, const int32_t* ids, int64_t count, void* stream) {
  Selection sel;
  int rc = select_begin(h, ids, count, true, stream, &sel);
  if (rc || count == 0 || sel.nflush == 0) return rc;
  hipStream_t s = (hipStream_t)stream;
  rc = flush_listed(h, sel.list, sel.nflush, s);
  return rc ? rc : select_end(h, s);
}

int gk_quantiles_select(gk_set* h, const int32_t* ids, int64_t count, const double* qs, int nq, double* out, int mode,
                        void* stream) {
  Selection sel;
  int rc = select_begin(h, ids, count, true, stream, &sel, [&] { return check_query_args(qs, nq, out, mode); });
  if (rc || count == 0 || nq == 0) return rc;
  hipStream_t s = (hipStream_t)stream;
  GKQuery q;
  rc = prepare_query(h, qs, nq, out, mode, s, &q);  // (before the flush: its GK_E_NOMEM mutates nothing)
  if (rc) return rc;
  // gk:166-167 / gk:197-198: the listed streams with pending values are
  // flushed first (state mutation); then every row from its committed table
  rc = flush_listed(h, sel.list, sel.nflush, s);
  if (rc) return rc;  // (GK_E_OVERFLOW: out is not written)
  HIP_TRY(gk_launch_select_query(h->st, ids, count, q, s));
  return select_end(h, s);
}

int gk_reset_select(gk_set* h, const int32_t* ids, int64_t count, void* stream) {
  Selection sel;
  int rc = select_begin(h, ids, count, false, stream, &sel);
  if (rc || count == 0) return rc;
  hipStream_t s = (hipStream_t)stream;
  // (class and slot stay: the stream's next ingest runs in its class's launch,
  // from an empty table)
  HIP_TRY(gk_launch_select_reset(h->st, ids, count, s));
  HIP_TRY(hipStreamSynchronize(s));
  return GK_OK;
}

int gk_stats_select(gk_set* h, const int32_t* ids, int64_t count, int64_t* n, double* mn, double* mx, double* sum,
                    double* avg, int32_t* table_size, int32_t* pending, void* stream) {
  Selection sel;
  int rc = select_begin(h, ids, count, false, stream, &sel);
  if (rc || count == 0) return rc;
  hipStream_t s = (hipStream_t)stream;
  const GKSelectStats o{n, mn, mx, sum, avg, table_size, pending};
  HIP_TRY(gk_launch_select_stats(h->st, ids, count, o, s));
  HIP_TRY(hipStreamSynchronize(s));
  return GK_OK;
}

// ---- rank queries: bounds on each stream's count of values <= x (k_rank)

int gk_ranks(gk_set* h, const double* xs, int nx, int64_t* lo, int64_t* hi, void* stream) {
  int rc = check_set(h);
  if (!rc) rc = check_rank_args(xs, nx, lo, hi);
  if (!rc) rc = gk_sync(h, stream);
  if (rc || nx == 0 || h->S == 0) return rc;
  hipStream_t s = (hipStream_t)stream;
  rc = stage_qs(h, xs, nx, s);  // (before the flush: its GK_E_NOMEM mutates nothing)
  if (rc) return rc;
  // gk_quantiles' flush (gk:166-167 / gk:197-198), settled: deferred streams
  // are re-run and a stream that outgrew the last class is reported
  rc = gk_flush(h, stream);
  if (!rc) rc = gk_sync(h, stream);
  if (rc) return rc;  // (GK_E_OVERFLOW: lo and hi are not written)
  HIP_TRY(gk_launch_rank(h->st, nullptr, h->S, h->d_qs, nx, lo, hi, s));
  HIP_TRY(hipStreamSynchronize(s));
  return GK_OK;
}

int gk_ranks_select(gk_set* h, const int32_t* ids, int64_t count, const double* xs, int nx, int64_t* lo, int64_t* hi,
                    void* stream) {
  Selection sel;
  int rc = select_begin(h, ids, count, true, stream, &sel, [&] { return check_rank_args(xs, nx, lo, hi); });
  if (rc || count == 0 || nx == 0) return rc;
  hipStream_t s = (hipStream_t)stream;
  rc = stage_qs(h, xs, nx, s);  // (before the flush, as in gk_quantiles_select)
  if (rc) return rc;
  rc = flush_listed(h, sel.list, sel.nflush, s);
  if (rc) return rc;  // (GK_E_OVERFLOW: lo and hi are not written)
  HIP_TRY(gk_launch_rank(h->st, ids, count, h->d_qs, nx, lo, hi, s));
  return select_end(h, s);
}

// ---- keyed rank queries: bounds per (stream id, value) sample (k_rank_keyed)

// GK_RANKK_CHUNK (tests): the grouped samples one wave takes
static int rank_keyed_chunk(int* chunk) {
  *chunk = GK_RANKK_CHUNK_DEFAULT;
  const char* e = getenv("GK_RANKK_CHUNK");
  if (!e) return GK_OK;
  char* end = nullptr;
  const long c = strtol(e, &end, 10);
  if (end == e || *end || c < 64 || c % 64 || c > INT32_MAX - 63)
    return fail(GK_E_ARG, "GK_RANKK_CHUNK=%s is not a multiple of 64 >= 64 (below 2^31)", e);
  *chunk = (int)c;
  return GK_OK;
}

// The head of gk_ranks_keyed and gk_rank_ingest_keyed, after their argument
// checks and gk_sync (count > 0): the scratch, the check kernel and its verdict,
// the flush of the occurring streams (*nflush of them; none when S == 0 or
// when the caller wants no rank: `flush` false).
static int rank_keyed_begin(gk_set* h, const int32_t* ids, const double* xs, int64_t count, bool flush, hipStream_t s,
                            int64_t* nflush) {
  *nflush = 0;
  // every scratch before the first launch: GK_E_NOMEM mutates nothing.  (The
  // stream is idle after gk_sync and an in-flight keyed ingest is settled:
  // its grouped batch in kg_vals / kg_offs -- rk_idx / kg_offs after a
  // gk_rank_ingest_keyed -- is free.)
  int rc = ensure_group_scratch(h, count, true, s);
  if (!rc && count > h->rk_idx_cap) {
    h->rk_idx_cap = 0;
    if (!renew_dev(&h->rk_idx, (size_t)count * sizeof(double)))
      return fail(GK_E_NOMEM, "index payload for %lld samples failed", (long long)count);
    h->rk_idx_cap = count;
  }
  if (!rc) rc = ensure_select_scratch(h, count, true, 0);
  if (rc) return rc;
  // ONE kernel over the samples: id range (negative ids pass), NaN on live
  // rows, the flush list -- nothing is mutated before its verdict is read back
  const int64_t bm = select_bitmap_words(h, true);
  int32_t* const ctl = h->d_sel;
  int32_t* const list = ctl + GK_SEL_WORDS + bm;
  HIP_TRY(hipMemsetAsync(ctl, 0, (size_t)(GK_SEL_WORDS + bm) * sizeof(int32_t), s));
  HIP_TRY(gk_launch_rank_keyed_check(h->st, ids, xs, count, ctl, reinterpret_cast<uint32_t*>(ctl + GK_SEL_WORDS), list,
                                     h->rk_idx, s));
  HIP_TRY(hipMemcpyAsync(h->h_ovf, ctl, GK_SEL_WORDS * sizeof(int32_t), hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  if (h->h_ovf[GK_SEL_BAD]) {
    const int64_t first = count - (int64_t)(uint32_t)h->h_ovf[GK_SEL_FIRST];
    int32_t id = 0;
    HIP_TRY(hipMemcpy(&id, ids + first, sizeof(int32_t), hipMemcpyDeviceToHost));
    return fail_rank_keyed_sample(first, id, h->S);
  }
  if (h->S == 0 || !flush) return GK_OK;  // (S == 0: every id is negative)
  *nflush = h->h_ovf[GK_SEL_COUNT];
  return flush_listed(h, list, *nflush, s);  // (GK_E_OVERFLOW: no output is written)
}

// S == 0: every id is negative, every row (0, 0, 0)
static int rank_keyed_zero_rows(int64_t* lo, int64_t* hi, int64_t* n, int64_t count, hipStream_t s) {
  for (int64_t* o : {lo, hi, n})
    if (o) HIP_TRY(hipMemsetAsync(o, 0, (size_t)count * sizeof(int64_t), s));
  HIP_TRY(hipStreamSynchronize(s));
  return GK_OK;
}

int gk_ranks_keyed(gk_set* h, const int32_t* ids, const double* xs, int64_t count, int64_t* lo, int64_t* hi, int64_t* n,
                   void* stream) {
  int chunk = 0;
  int rc = check_set(h);
  if (!rc) rc = check_rank_keyed_args(ids, xs, count, lo, hi, n);
  if (!rc) rc = rank_keyed_chunk(&chunk);
  if (!rc) rc = gk_sync(h, stream);
  if (rc || count == 0) return rc;
  hipStream_t s = (hipStream_t)stream;
  int64_t nflush = 0;
  rc = rank_keyed_begin(h, ids, xs, count, true, s, &nflush);
  if (rc) return rc;
  if (h->S == 0) return rank_keyed_zero_rows(lo, hi, n, count, s);
  // the stable group-by of the samples by id, payload = sample index
  HIP_TRY(gk_launch_group_by_key(h->kg, ids, h->rk_idx, count, h->S, h->kg_vals, h->kg_offs, s));
  HIP_TRY(gk_launch_rank_keyed(h->st, ids, xs, count, h->kg_vals, h->kg_offs, chunk, lo, hi, n, s));
  return select_end(h, s);
}

// ---- keyed score-and-ingest: gk_ranks_keyed, then gk_ingest_keyed, one group-by

int gk_rank_ingest_keyed(gk_set* h, const int32_t* ids, const double* xs, int64_t count, int64_t* lo, int64_t* hi,
                         int64_t* n, const double* qs, int nq, double* out, int mode, void* stream) {
  int chunk = 0;
  int rc = check_set(h);
  if (!rc) rc = check_rank_ingest_keyed_args(ids, xs, count);
  if (!rc) rc = check_query_args(qs, nq, out, mode);
  if (!rc) rc = rank_keyed_chunk(&chunk);
  if (!rc) rc = gk_sync(h, stream);
  if (rc) return rc;
  if (count == 0) return gk_ingest_keyed(h, ids, xs, 0, qs, nq, out, mode, stream);
  hipStream_t s = (hipStream_t)stream;
  int64_t nflush = 0;
  // (no rank output: gk_ingest_keyed behind the sample check -- no rank, no flush)
  rc = rank_keyed_begin(h, ids, xs, count, lo || hi || n, s, &nflush);
  if (rc) return rc;
  if (h->S == 0) return rank_keyed_zero_rows(lo, hi, n, count, s);
  // what gk_ranks_keyed ends with, ahead of the ingest: the flush may have
  // promoted streams, and the ingest's grow_pools reads the slots in use
  if (nflush > 0) {
    rc = select_end(h, s);
    if (rc) return rc;
  }
  // ONE group-by, payload = sample index; k_rank_ingest_keyed then turns the
  // consumed payload buffer into the grouped values: (rk_idx, kg_offs) is the
  // batch gk_ingest_keyed's own group-by would have made.  Only enqueued from here.
  HIP_TRY(gk_launch_group_by_key(h->kg, ids, h->rk_idx, count, h->S, h->kg_vals, h->kg_offs, s));
  HIP_TRY(gk_launch_rank_ingest_keyed(h->st, ids, xs, count, h->kg_vals, h->kg_offs, chunk, lo, hi, n, h->rk_idx, s));
  if (nq == 0) return gk_ingest(h, h->rk_idx, h->kg_offs, stream);
  return gk_ingest_quantiles(h, h->rk_idx, h->kg_offs, qs, nq, out, mode, stream);
}

static int merge_self(gk_set* dst, hipStream_t s, void* stream);

int gk_merge(gk_set* dst, gk_set* const* srcs, int nsrcs, void* stream) {
  int rc = check_merge_args(dst, srcs, nsrcs);
  if (rc) return rc;
  hipStream_t s = (hipStream_t)stream;
  rc = gk_sync(dst, stream);
  if (rc) return rc;
  for (int k = 0; k < nsrcs; ++k) {
    gk_set* src = srcs[k];
    if (src == dst) {  // dst.merge(dst): the reference accepts it (gk:111-154)
      rc = merge_self(dst, s, stream);
      if (rc) return rc;
      continue;
    }
    // a repeated source is flushed again at each of its merges (gk:137)
    rc = gk_sync(src, stream);
    if (!rc) rc = flush_source(src, s, stream);
    if (rc) return rc;
    FoldArgs a{};
    a.src = src->st;
    rc = run_fold(dst, a, kMergeOverflow, s);
    if (rc) return rc;
  }
  HIP_TRY(hipStreamSynchronize(s));
  return GK_OK;
}

int gk_rollup(gk_set* dst, gk_set* src, const int64_t* group_offsets, const int64_t* members, void* stream) {
  int rc = check_rollup_args(dst, src, group_offsets);
  if (rc) return rc;
  if (src->device != dst->device) return fail(GK_E_ARG, "the sets live on different devices");
  hipStream_t s = (hipStream_t)stream;
  rc = gk_sync(dst, stream);
  if (!rc) rc = gk_sync(src, stream);
  if (rc) return rc;
  const int64_t G = dst->S, S = src->S;
  // ---- argument checks on the device, read back before anything is mutated.
  // Scratch of src that no launch of this call uses otherwise: the last
  // overflow list (S words) holds the bitmap, then the flush list; its count
  // word the error bits, then the flush count.
  int32_t* const word = ovf_count(src, kRounds - 1);
  int32_t* const scratch = ovf_list(src, kRounds - 1);
  src->ctr_clean = false;
  HIP_TRY(hipMemsetAsync(word, 0, sizeof(int32_t), s));
  HIP_TRY(gk_launch_rollup_check_offsets(group_offsets, G, word, s));
  int64_t* const h_total = reinterpret_cast<int64_t*>(src->h_ovf + 2);
  HIP_TRY(hipMemcpyAsync(h_total, group_offsets + G, sizeof(int64_t), hipMemcpyDeviceToHost, s));
  rc = (int)read_overflow(src, kRounds - 1, s);
  if (rc < 0) return rc;
  if (rc != 0) return fail(GK_E_ARG, "group_offsets must start at 0 and not decrease");
  const int64_t M = *h_total;
  if (M == 0) return GK_OK;  // every group is empty: nothing is touched
  if (!members) return fail(GK_E_ARG, "members is null");
  if (M > S)
    return fail(GK_E_ARG, "%lld members of %lld source streams: a stream is listed more than once or out of range",
                (long long)M, (long long)S);
  HIP_TRY(hipMemsetAsync(scratch, 0, (size_t)((S + 31) / 32) * sizeof(uint32_t), s));
  HIP_TRY(gk_launch_rollup_check_members(members, M, S, reinterpret_cast<uint32_t*>(scratch), word, s));
  rc = (int)read_overflow(src, kRounds - 1, s);
  if (rc < 0) return rc;
  if (rc & 2) return fail(GK_E_ARG, "a member lies outside [0, %lld)", (long long)S);
  if (rc & 4) return fail(GK_E_ARG, "a source stream is listed more than once");
  // ---- other.merge_compress() of every member with n != 0 (gk:126 / gk:137;
  // unconditional there, pending values or not)
  if (M == S) {
    // every source stream is a member (the plain group-by): the batch flush
    // that gk_merge gives its sources; on a stream with n == 0 it changes nothing
    rc = flush_source(src, s, stream);
  } else {
    // the list of those members; each climbs the ladder as far as its flush needs
    HIP_TRY(gk_launch_rollup_flush_list(src->st, members, M, word, scratch, s));
    const int64_t nflush = read_overflow(src, kRounds - 1, s);
    if (nflush < 0) return (int)nflush;
    rc = flush_listed(src, scratch, nflush, s);
  }
  if (rc) return rc;
  if (!dst->d_roll_prog && !renew_dev(&dst->d_roll_prog, (size_t)std::max<int64_t>(dst->S, 1) * sizeof(int64_t)))
    return fail(GK_E_NOMEM, "roll-up progress array of %lld entries failed", (long long)dst->S);
  FoldArgs a{};
  a.src = src->st;
  a.goffs = group_offsets;
  a.members = members;
  a.progress = dst->d_roll_prog;
  rc = run_fold(dst, a, kRollupOverflow, s);
  if (rc) return rc;
  HIP_TRY(hipStreamSynchronize(s));
  return GK_OK;
}

int gk_merge_compress(gk_set* h, const double* v, const int32_t* g, const int32_t* d, const int64_t* eoffs,
                      void* stream) {
  int rc = check_set(h);
  if (!rc) rc = check_record_args(v, g, d, eoffs);
  if (rc) return rc;
  hipStream_t s = (hipStream_t)stream;
  rc = gk_sync(h, stream);
  if (rc) return rc;
  FoldArgs a{};
  a.ev = v;
  a.eg = g;
  a.ed = d;
  a.eoffs = eoffs;
  rc = run_fold(h, a, kMergeOverflow, s);
  if (rc) return rc;
  HIP_TRY(hipStreamSynchronize(s));
  return GK_OK;
}

int gk_export_sizes(gk_set* h, int32_t* sizes, void* stream) {
  int rc = check_set(h);
  if (rc) return rc;
  rc = settle(h, (hipStream_t)stream, false);  // a deferred stream of the last call is re-run first
  if (rc) return rc;
  if (!sizes) return fail(GK_E_ARG, "sizes is null");
  if (h->S)
    HIP_TRY(hipMemcpyAsync(sizes, h->st.E, h->S * sizeof(int32_t), hipMemcpyDeviceToDevice, (hipStream_t)stream));
  return GK_OK;
}

int gk_export(gk_set* h, const int64_t* offs, double* v, int32_t* g, int32_t* d, void* stream) {
  int rc = check_set(h);
  if (rc) return rc;
  rc = settle(h, (hipStream_t)stream, false);  // a deferred stream of the last call is re-run first
  if (rc) return rc;
  if (!offs) return fail(GK_E_ARG, "offs is null");
  HIP_TRY(gk_launch_export(h->st, offs, v, g, d, (hipStream_t)stream));
  return GK_OK;
}

int gk_export_pending_sizes(gk_set* h, int32_t* sizes, void* stream) {
  int rc = check_set(h);
  if (rc) return rc;
  rc = settle(h, (hipStream_t)stream, false);  // a deferred stream of the last call is re-run first
  if (rc) return rc;
  if (!sizes) return fail(GK_E_ARG, "sizes is null");
  if (h->S)
    HIP_TRY(hipMemcpyAsync(sizes, h->st.pend, h->S * sizeof(int32_t), hipMemcpyDeviceToDevice, (hipStream_t)stream));
  return GK_OK;
}

int gk_export_pending(gk_set* h, const int64_t* poffs, double* pv, void* stream) {
  int rc = check_set(h);
  if (rc) return rc;
  rc = settle(h, (hipStream_t)stream, false);  // a deferred stream of the last call is re-run first
  if (rc) return rc;
  if (!poffs || !pv) return fail(GK_E_ARG, "null pointer");
  HIP_TRY(gk_launch_export_pending(h->st, poffs, pv, (hipStream_t)stream));
  return GK_OK;
}

int gk_import(gk_set* h, const int64_t* offs, const double* v, const int32_t* g, const int32_t* d,
              const int64_t* poffs, const double* pv, const int64_t* n, const double* mn, const double* mx,
              const double* sum, const double* avg, void* stream) {
  int rc = check_set(h);
  if (rc) return rc;
  if (!offs || !poffs || !n || !mn || !mx || !sum || !avg) return fail(GK_E_ARG, "null pointer");
  hipStream_t s = (hipStream_t)stream;
  const int64_t S = h->S;
  if (S == 0) return GK_OK;
  rc = gk_sync(h, stream);
  if (rc) return rc;
  h->ctr_clean = false;  // (writes words of the per-call block below)
  {
    int32_t* bad = h->d_ctr + GK_CTR_BADPEND;
    HIP_TRY(hipMemsetAsync(bad, 0, sizeof(int32_t), s));
    HIP_TRY(gk_launch_check_pending(S, h->P, n, poffs, bad, s));
    HIP_TRY(hipMemcpyAsync(h->h_ovf, bad, sizeof(int32_t), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (h->h_ovf[0] != 0)
      return fail(GK_E_ARG, "%d stream(s) hold more pending values than add() leaves (pending <= n %% %d)",
                  h->h_ovf[0], h->P);
  }
  HIP_TRY(hipMemcpyAsync(h->st.n, n, S * sizeof(int64_t), hipMemcpyDeviceToDevice, s));
  HIP_TRY(hipMemcpyAsync(h->st.mn, mn, S * sizeof(double), hipMemcpyDeviceToDevice, s));
  HIP_TRY(hipMemcpyAsync(h->st.mx, mx, S * sizeof(double), hipMemcpyDeviceToDevice, s));
  HIP_TRY(hipMemcpyAsync(h->st.sum, sum, S * sizeof(double), hipMemcpyDeviceToDevice, s));
  HIP_TRY(hipMemcpyAsync(h->st.avg, avg, S * sizeof(double), hipMemcpyDeviceToDevice, s));
  // tables that do not fit their stream's class: one class up (on the
  // device) and import again, until every table fits
  const GKPoolDev pool = pool_args(h);
  for (int round = 0; round <= h->st.nclass; ++round) {
    HIP_TRY(hipMemsetAsync(h->d_ovfc, 0, sizeof(int32_t), s));
    HIP_TRY(gk_launch_import(h->st, offs, v, g, d, poffs, pv, ovf_count(h, 0), ovf_list(h, 0), s));
    const int64_t c = read_overflow(h, 0, s);
    if (c < 0) return (int)c;
    if (c == 0) return GK_OK;
    rc = grow_targets(h, ovf_list(h, 0), c, s);
    if (rc) return rc;
    h->no_members = false;
    HIP_TRY(gk_launch_promote_dev(h->st, ovf_count(h, 0), ovf_list(h, 0), -2, pool, s));
    rc = mark_done(h, s);
    if (!rc) rc = gk_sync(h, stream);
    if (rc) return rc;
  }
  return fail(GK_E_OVERFLOW, "import did not converge");
}

// ---- versioned state files (gk_format.h) ------------------------------------
namespace {

int fmt_error(int rc, const char* path) {
  switch (rc) {
    case gkfmt::E_IO: return fail(GK_E_IO, "cannot read/write state file %s", path);
    case gkfmt::E_VERSION: return fail(GK_E_FORMAT, "%s: unsupported state format version", path);
    case gkfmt::E_CHECKSUM: return fail(GK_E_FORMAT, "%s: checksum mismatch (corrupt state file)", path);
    default: return fail(GK_E_FORMAT, "%s: not a GKSTATE file or truncated", path);
  }
}

// device scratch freed on scope exit (after the stream was synchronised)
struct DevBuf {
  void* p = nullptr;
  ~DevBuf() {
    if (p) (void)hipFree(p);
  }
  bool alloc(size_t bytes) { return hipMalloc(&p, bytes ? bytes : 8) == hipSuccess; }
};

}  // namespace

int gk_save(gk_set* h, const char* path, void* stream) {
  int rc = check_set(h);
  if (rc) return rc;
  if (!path) return fail(GK_E_ARG, "path is null");
  rc = gk_sync(h, stream);
  if (rc) return rc;
  hipStream_t s = (hipStream_t)stream;
  const int64_t S = h->S;
  gkfmt::State st;
  st.eps = h->eps;
  st.resize_streams(S);
  if (S) {
    HIP_TRY(hipMemcpyAsync(st.sizes.data(), h->st.E, S * 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(st.psizes.data(), h->st.pend, S * 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(st.n.data(), h->st.n, S * 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(st.mn.data(), h->st.mn, S * 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(st.mx.data(), h->st.mx, S * 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(st.sum.data(), h->st.sum, S * 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(st.avg.data(), h->st.avg, S * 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
  }
  std::vector<int64_t> offs(S + 1, 0), poffs(S + 1, 0);
  for (int64_t k = 0; k < S; ++k) {
    offs[k + 1] = offs[k] + st.sizes[k];
    poffs[k + 1] = poffs[k] + st.psizes[k];
  }
  const int64_t E = offs[S], P = poffs[S];
  st.v.resize(E);
  st.g.resize(E);
  st.d.resize(E);
  st.pv.resize(P);
  if (S) {
    DevBuf d_offs, d_poffs, d_v, d_g, d_d, d_pv;
    if (!d_offs.alloc((S + 1) * 8) || !d_poffs.alloc((S + 1) * 8) || !d_v.alloc(E * 8) || !d_g.alloc(E * 4) ||
        !d_d.alloc(E * 4) || !d_pv.alloc(P * 8))
      return fail(GK_E_NOMEM, "save: device scratch of %lld records failed", (long long)E);
    HIP_TRY(hipMemcpyAsync(d_offs.p, offs.data(), (S + 1) * 8, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(d_poffs.p, poffs.data(), (S + 1) * 8, hipMemcpyHostToDevice, s));
    HIP_TRY(gk_launch_export(h->st, (const int64_t*)d_offs.p, (double*)d_v.p, (int32_t*)d_g.p, (int32_t*)d_d.p, s));
    HIP_TRY(gk_launch_export_pending(h->st, (const int64_t*)d_poffs.p, (double*)d_pv.p, s));
    if (E) {
      HIP_TRY(hipMemcpyAsync(st.v.data(), d_v.p, E * 8, hipMemcpyDeviceToHost, s));
      HIP_TRY(hipMemcpyAsync(st.g.data(), d_g.p, E * 4, hipMemcpyDeviceToHost, s));
      HIP_TRY(hipMemcpyAsync(st.d.data(), d_d.p, E * 4, hipMemcpyDeviceToHost, s));
    }
    if (P) HIP_TRY(hipMemcpyAsync(st.pv.data(), d_pv.p, P * 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
  }
  rc = gkfmt::write(path, st);
  return rc ? fmt_error(rc, path) : GK_OK;
}

int gk_peek(const char* path, double* eps, int64_t* num_streams) {
  if (!path) return fail(GK_E_ARG, "path is null");
  gkfmt::Header hd;
  const int rc = gkfmt::peek(path, &hd);
  if (rc) return fmt_error(rc, path);
  if (eps) *eps = hd.eps;
  if (num_streams) *num_streams = hd.S;
  return GK_OK;
}

int gk_load(gk_set* h, const char* path, void* stream) {
  int rc = check_set(h);
  if (rc) return rc;
  if (!path) return fail(GK_E_ARG, "path is null");
  gkfmt::State st;
  rc = gkfmt::read(path, &st);
  if (rc) return fmt_error(rc, path);
  if (st.S != h->S)
    return fail(GK_E_ARG, "%s holds %lld streams, the set has %lld", path, (long long)st.S, (long long)h->S);
  if (st.eps != h->eps) return fail(GK_E_EPS_MISMATCH, "%s was saved with eps=%.17g, the set has eps=%.17g", path,
                                   st.eps, h->eps);
  const int64_t S = st.S;
  if (S == 0) return GK_OK;
  hipStream_t s = (hipStream_t)stream;
  std::vector<int64_t> offs(S + 1, 0), poffs(S + 1, 0);
  for (int64_t k = 0; k < S; ++k) {
    offs[k + 1] = offs[k] + st.sizes[k];
    poffs[k + 1] = poffs[k] + st.psizes[k];
    if (st.psizes[k] < 0 || st.n[k] < 0 || st.psizes[k] > st.n[k] % h->P)
      return fail(GK_E_FORMAT, "%s: stream %lld holds %d pending values at n=%lld (at most n mod %d)", path,
                  (long long)k, st.psizes[k], (long long)st.n[k], h->P);
  }
  const int64_t E = offs[S], P = poffs[S];
  DevBuf d_offs, d_poffs, d_v, d_g, d_d, d_pv, d_hdr;
  if (!d_offs.alloc((S + 1) * 8) || !d_poffs.alloc((S + 1) * 8) || !d_v.alloc(E * 8) || !d_g.alloc(E * 4) ||
      !d_d.alloc(E * 4) || !d_pv.alloc(P * 8) || !d_hdr.alloc(5 * S * 8))
    return fail(GK_E_NOMEM, "load: device scratch of %lld records failed", (long long)E);
  int64_t* d_n = (int64_t*)d_hdr.p;
  double* d_f = (double*)d_hdr.p + S;
  HIP_TRY(hipMemcpyAsync(d_offs.p, offs.data(), (S + 1) * 8, hipMemcpyHostToDevice, s));
  HIP_TRY(hipMemcpyAsync(d_poffs.p, poffs.data(), (S + 1) * 8, hipMemcpyHostToDevice, s));
  if (E) {
    HIP_TRY(hipMemcpyAsync(d_v.p, st.v.data(), E * 8, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(d_g.p, st.g.data(), E * 4, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(d_d.p, st.d.data(), E * 4, hipMemcpyHostToDevice, s));
  }
  if (P) HIP_TRY(hipMemcpyAsync(d_pv.p, st.pv.data(), P * 8, hipMemcpyHostToDevice, s));
  HIP_TRY(hipMemcpyAsync(d_n, st.n.data(), S * 8, hipMemcpyHostToDevice, s));
  HIP_TRY(hipMemcpyAsync(d_f, st.mn.data(), S * 8, hipMemcpyHostToDevice, s));
  HIP_TRY(hipMemcpyAsync(d_f + S, st.mx.data(), S * 8, hipMemcpyHostToDevice, s));
  HIP_TRY(hipMemcpyAsync(d_f + 2 * S, st.sum.data(), S * 8, hipMemcpyHostToDevice, s));
  HIP_TRY(hipMemcpyAsync(d_f + 3 * S, st.avg.data(), S * 8, hipMemcpyHostToDevice, s));
  rc = gk_import(h, (const int64_t*)d_offs.p, (const double*)d_v.p, (const int32_t*)d_g.p, (const int32_t*)d_d.p,
                 (const int64_t*)d_poffs.p, (const double*)d_pv.p, d_n, d_f, d_f + S, d_f + 2 * S, d_f + 3 * S,
                 stream);
  const hipError_t e = hipStreamSynchronize(s);  // the scratch above is freed on return
  if (rc) return rc;
  if (e != hipSuccess) return fail(GK_E_HIP, "load: %s", hipGetErrorString(e));
  return GK_OK;
}

// ---- packed state (gk_pack.h): device buffers ------------------------------
namespace {
struct DevMem {
  static int to_host(void* host, const void* src, size_t n, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    if (hipMemcpyAsync(host, src, n, hipMemcpyDeviceToHost, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess)
      return fail(GK_E_HIP, "packed state: device-to-host copy failed");
    return GK_OK;
  }
  static int from_host(void* dst, const void* host, size_t n, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    if (hipMemcpyAsync(dst, host, n, hipMemcpyHostToDevice, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess)
      return fail(GK_E_HIP, "packed state: host-to-device copy failed");
    return GK_OK;
  }
};
}  // namespace

// The size arrays borrow two of the set's S-entry overflow lists (idle
// outside an ingest call; the calls below synchronise first).
int gk_pack_bytes(gk_set* h, int64_t* bytes, void* stream) {
  int rc = check_set(h);
  if (rc) return rc;
  if (!bytes) return fail(GK_E_ARG, "bytes is null");
  rc = gk_sync(h, stream);
  if (rc) return rc;
  return gkpack::pack_bytes<DevMem>(h, h->d_ovfl[1], h->d_ovfl[2], bytes, stream);
}

int gk_pack(gk_set* h, void* buf, int64_t bytes, void* stream) {
  int rc = check_set(h);
  if (rc) return rc;
  if (!buf) return fail(GK_E_ARG, "buf is null");
  rc = gk_sync(h, stream);
  if (rc) return rc;
  std::string err;
  rc = gkpack::pack<DevMem>(h, h->d_ovfl[1], h->d_ovfl[2], buf, bytes, stream, err);
  return (rc && !err.empty()) ? fail(rc, "%s", err.c_str()) : rc;
}

// dst.merge(dst), gk:111-154 with `other` IS self: gk:137 flushes dst itself
// (emptying its incoming), gk:138-147 convert that flushed table, gk:149
// doubles n, and gk:154 merges the converted records back.  k_fold reads the
// source table while it rewrites the destination's, so the source is a
// snapshot of the flushed dst: packed into a device buffer and imported into
// a scratch set that is NOT flushed again (a second compress at the same
// threshold is not a no-op).  Its pending count is 0 and its n equals dst's,
// so k_fold takes the general branch (n > 0) or, for an empty stream, the
// "other empty" branch whose flush of an empty stream changes nothing.
static int merge_self(gk_set* dst, hipStream_t s, void* stream) {
  int rc = gk_sync(dst, stream);
  if (!rc) rc = flush_source(dst, s, stream);  // other.merge_compress() (gk:137)
  if (rc) return rc;
  int64_t bytes = 0;
  rc = gk_pack_bytes(dst, &bytes, stream);
  if (rc) return rc;
  DevBuf buf;
  if (!buf.alloc((size_t)bytes)) return fail(GK_E_NOMEM, "self-merge: snapshot of %lld bytes", (long long)bytes);
  rc = gk_pack(dst, buf.p, bytes, stream);
  if (!rc && !dst->self_scratch) rc = gk_create(dst->S, dst->eps, 0, dst->device, &dst->self_scratch);
  if (rc) return rc;
  std::string err;
  gkpack::Header hd{};
  rc = gkpack::read_header<DevMem>(dst->self_scratch, buf.p, &hd, stream, err, dst->S);
  if (!rc) rc = gkpack::import_packed<DevMem>(dst->self_scratch, buf.p, hd, stream);
  if (!rc) rc = gk_sync(dst->self_scratch, stream);
  if (rc) return (!err.empty()) ? fail(rc, "%s", err.c_str()) : rc;
  FoldArgs a{};
  a.src = dst->self_scratch->st;
  rc = run_fold(dst, a, kMergeOverflow, s);
  // the snapshot set (a full copy of dst's state) is not kept beyond the
  // merge: the set's memory stays what it was before
  const int rs = gk_sync(dst, stream);
  gk_destroy(dst->self_scratch);
  dst->self_scratch = nullptr;
  return rc ? rc : rs;
}

int gk_fold_packed(gk_set* dst, const void* const* bufs, int nbufs, void* stream) {
  int rc = check_set(dst);
  if (rc) return rc;
  rc = gk_sync(dst, stream);
  if (rc) return rc;
  std::string err;
  auto make = [&](gk_set** out) { return gk_create(dst->S, dst->eps, 0, dst->device, out); };
  rc = gkpack::fold<DevMem>(dst, bufs, nbufs, &dst->fold_scratch, make, stream, err);
  return (rc && !err.empty()) ? fail(rc, "%s", err.c_str()) : rc;
}

// ---- stream transfer: listed streams to and from a packed state -------------
// (k_pack_sizes / k_pack_select / k_unpack_check / k_unpack_select)

// gk_pack_select_bytes (need_out given: only the size) and gk_pack_select.
// The sizes go straight into the buffer's eoffs / poffs sections -- their
// positions depend only on `count` -- and are scanned there on the device;
// the host reads back the two totals only (layout and header need them).
static int pack_select_impl(gk_set* h, const int32_t* ids, int64_t count, void* buf, int64_t bytes, int64_t* need_out,
                            void* stream) {
  Selection sel;
  const int64_t nsum = gk_scan_sums(std::max<int64_t>(count, 0) + 1);
  int rc = select_begin(h, ids, count, false, stream, &sel, nullptr, 4 + 2 * nsum);
  if (rc) return rc;
  hipStream_t s = (hipStream_t)stream;
  const gkpack::Layout L0 = gkpack::layout(count, 0, 0);
  const bool sized = !need_out && bytes >= (int64_t)L0.total;  // the offset sections lie inside the buffer
  unsigned long long* const totals = reinterpret_cast<unsigned long long*>(sel.extra);
  int64_t E = 0, P = 0;
  if (count > 0) {
    HIP_TRY(hipMemsetAsync(totals, 0, 2 * sizeof(unsigned long long), s));
    HIP_TRY(gk_launch_pack_sizes(h->st, ids, count, sized ? gkpack::at<int64_t>(buf, L0.eoffs) : nullptr,
                                 sized ? gkpack::at<int64_t>(buf, L0.poffs) : nullptr, totals, s));
    HIP_TRY(hipMemcpyAsync(h->h_ovf, totals, 2 * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    E = reinterpret_cast<const int64_t*>(h->h_ovf)[0];
    P = reinterpret_cast<const int64_t*>(h->h_ovf)[1];
  }
  const gkpack::Layout L = gkpack::layout(count, E, P);
  if (need_out) {
    *need_out = (int64_t)L.total;
    return GK_OK;
  }
  if (bytes < (int64_t)L.total)
    return fail(GK_E_ARG, "packed state needs %lld bytes, the buffer has %lld", (long long)L.total, (long long)bytes);
  gkpack::Header hd{};
  hd.magic = gkpack::kMagic;
  hd.version = gkpack::kVersion;
  hd.header_bytes = sizeof(gkpack::Header);
  hd.eps = h->eps;
  hd.S = count;
  hd.E = E;
  hd.P = P;
  hd.bytes = (int64_t)L.total;
  rc = DevMem::from_host(buf, &hd, sizeof(hd), stream);
  if (rc) return rc;
  if (count == 0) {
    HIP_TRY(hipMemsetAsync(gkpack::at<int64_t>(buf, L.eoffs), 0, sizeof(int64_t), s));
    HIP_TRY(hipMemsetAsync(gkpack::at<int64_t>(buf, L.poffs), 0, sizeof(int64_t), s));
    HIP_TRY(hipStreamSynchronize(s));
    return GK_OK;
  }
  int64_t* const eo = gkpack::at<int64_t>(buf, L.eoffs);
  int64_t* const po = gkpack::at<int64_t>(buf, L.poffs);
  HIP_TRY(gk_launch_scan_i64(eo, count + 1, totals + 2, s));
  HIP_TRY(gk_launch_scan_i64(po, count + 1, totals + 2, s));
  const GKSelectStats o{gkpack::at<int64_t>(buf, L.n),    gkpack::at<double>(buf, L.mn), gkpack::at<double>(buf, L.mx),
                        gkpack::at<double>(buf, L.sum), gkpack::at<double>(buf, L.avg), nullptr,
                        nullptr};
  HIP_TRY(gk_launch_select_stats(h->st, ids, count, o, s));
  HIP_TRY(gk_launch_pack_select(h->st, ids, count, eo, po, gkpack::at<double>(buf, L.v), gkpack::at<int32_t>(buf, L.g),
                                gkpack::at<int32_t>(buf, L.d), gkpack::at<double>(buf, L.pv), s));
  HIP_TRY(hipStreamSynchronize(s));
  return GK_OK;
}

int gk_pack_select_bytes(gk_set* h, const int32_t* ids, int64_t count, int64_t* bytes, void* stream) {
  if (!bytes) return fail(GK_E_ARG, "bytes is null");
  return pack_select_impl(h, ids, count, nullptr, 0, bytes, stream);
}

int gk_pack_select(gk_set* h, const int32_t* ids, int64_t count, void* buf, int64_t bytes, void* stream) {
  if (!buf) return fail(GK_E_ARG, "buf is null");
  return pack_select_impl(h, ids, count, buf, bytes, nullptr, stream);
}

int gk_unpack_select(gk_set* h, const int32_t* ids, int64_t count, const void* buf, void* stream) {
  int rc = check_set(h);
  if (!rc) rc = check_select_args(ids, count);
  if (rc) return rc;
  if (!buf) return fail(GK_E_ARG, "buf is null");
  rc = gk_sync(h, stream);
  if (rc) return rc;
  hipStream_t s = (hipStream_t)stream;
  gkpack::Header hd{};
  std::string err;
  if (count == 0) {  // the buffer is still validated (header and its one-entry offset tables)
    rc = gkpack::read_header<DevMem>(h, buf, &hd, stream, err, 0);
    return (rc && !err.empty()) ? fail(rc, "%s", err.c_str()) : rc;
  }
  rc = DevMem::to_host(&hd, buf, sizeof(hd), stream);
  if (rc) return rc;
  rc = gkpack::check_header(hd, h->eps, count, err);
  if (rc) return fail(rc, "%s", err.c_str());
  const gkpack::Layout L = gkpack::layout(hd.S, hd.E, hd.P);
  const GKPacked pk{gkpack::at<int64_t>(buf, L.n),     gkpack::at<double>(buf, L.mn),    gkpack::at<double>(buf, L.mx),
                    gkpack::at<double>(buf, L.sum),    gkpack::at<double>(buf, L.avg),   gkpack::at<int64_t>(buf, L.eoffs),
                    gkpack::at<int64_t>(buf, L.poffs), gkpack::at<double>(buf, L.v),     gkpack::at<int32_t>(buf, L.g),
                    gkpack::at<int32_t>(buf, L.d),     gkpack::at<double>(buf, L.pv),    hd.E,
                    hd.P};
  // scratch: control words, the bitmap of listed streams, the overflow rows
  const int64_t bm = (h->S + 31) / 32;
  rc = ensure_select_words(h, GK_UNP_WORDS + bm + std::min<int64_t>(count, h->S));
  if (rc) return rc;
  int32_t* const ctl = h->d_sel;
  uint32_t* const bitmap = reinterpret_cast<uint32_t*>(ctl + GK_UNP_WORDS);
  int32_t* const rows = ctl + GK_UNP_WORDS + bm;
  HIP_TRY(hipMemsetAsync(ctl, 0, (size_t)(GK_UNP_WORDS + bm) * sizeof(int32_t), s));
  HIP_TRY(gk_launch_unpack_check(h->st, ids, count, pk, ctl, bitmap, s));
  HIP_TRY(hipMemcpyAsync(h->h_ovf, ctl, GK_UNP_WORDS * sizeof(int32_t), hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  const int bad = h->h_ovf[GK_UNP_BAD];
  if (bad & 4) return fail(GK_E_FORMAT, "%s", gkpack::kBadOffsets);
  if (bad & 1) {
    const int64_t first = count - (int64_t)(uint32_t)h->h_ovf[GK_UNP_FIRST];
    int32_t id = 0;
    HIP_TRY(hipMemcpy(&id, ids + first, sizeof(int32_t), hipMemcpyDeviceToHost));
    return fail(GK_E_ARG, "ids[%lld] = %d lies outside [0, %lld)", (long long)first, id, (long long)h->S);
  }
  if (bad & 2) return fail(GK_E_ARG, "a stream id is listed more than once (two rows for one stream)");
  if (bad & 8)
    return fail(GK_E_ARG, "a packed stream holds more pending values than add() leaves (pending <= n %% %d)", h->P);
  const int last = h->st.nclass - 1;
  if (h->h_ovf[GK_UNP_MAXE] > h->st.cap[last] - 1)
    return fail(GK_E_OVERFLOW, "a packed table of %d entries exceeds the last capacity class (%d entries)",
                h->h_ovf[GK_UNP_MAXE], h->st.cap[last] - 1);
  // the arenas grow BEFORE the first write: GK_E_NOMEM leaves every stream as it was
  int64_t need[GK_MAX_CLASSES] = {}, moving = 0;
  for (int t = 1; t <= last; ++t) moving += need[t] = h->h_ovf[GK_UNP_NEED + t];
  for (int t = 1; t <= last; ++t) {
    if (!need[t]) continue;
    rc = grow_class(h, t, (int64_t)h->st.alloc[t] + need[t], s);
    if (rc) return rc;
  }
  GKUnpackOvf ov{};
  ov.count = h->d_ovfc;
  ov.stuck = ctl + GK_UNP_STUCK;
  int64_t at = 0;
  for (int t = 1; t <= last; ++t) {
    ov.list[t] = ovf_list(h, t);
    ov.rows[t] = rows + at;
    at += need[t];
  }
  h->ctr_clean = false;  // (the overflow counts are words of the per-call block)
  HIP_TRY(hipMemsetAsync(h->d_ovfc, 0, kRounds * sizeof(int32_t), s));
  HIP_TRY(gk_launch_unpack_select(h->st, ids, nullptr, count, pk, ov, s));
  if (moving == 0) {
    HIP_TRY(hipStreamSynchronize(s));
    return GK_OK;
  }
  // the rows whose table outgrew their stream's class: the streams move to
  // the class that holds it (k_promote_dev copies the old table, about to be
  // overwritten), then their rows are installed
  const GKPoolDev pool = pool_args(h);
  h->no_members = false;
  for (int t = 1; t <= last; ++t) {
    if (!need[t]) continue;
    HIP_TRY(gk_launch_promote_dev(h->st, ovf_count(h, t), ovf_list(h, t), t, pool, s));
    HIP_TRY(gk_launch_unpack_select(h->st, ids, ov.rows[t], need[t], pk, ov, s));
  }
  HIP_TRY(hipMemcpyAsync(h->h_ovf, ov.stuck, sizeof(int32_t), hipMemcpyDeviceToHost, s));
  rc = select_end(h, s);
  if (rc) return rc;
  if (h->h_ovf[0] != 0)
    return fail(GK_E_OVERFLOW, "%d packed stream(s) found no slot in a capacity class and keep their state", h->h_ovf[0]);
  return GK_OK;
}

// ---- compaction (gk_compact.hip) ------------------------------------------------
int gk_compact(gk_set* h, int64_t* demoted, int64_t* bytes_freed, void* stream) {
  int rc = check_set(h);
  if (!rc) rc = gk_sync(h, stream);
  if (rc) return rc;
  if (demoted) *demoted = 0;
  if (bytes_freed) *bytes_freed = 0;
  if (h->S == 0 || h->no_members) return GK_OK;  // nothing promoted: nothing to place
  hipStream_t s = (hipStream_t)stream;
  rc = ensure_select_words(h, GK_CMP_WORDS);  // (before anything is mutated)
  if (rc) return rc;
  int64_t before = 0, after = 0, dem = 0;
  for (int c = 0; c < h->st.nclass; ++c) before += arena_bytes(h, c) + workspace_bytes(h, c);
  rc = compact_classes(h, h->d_sel, s, &dem);
  // (also after GK_E_NOMEM: the classes done so far have new counters)
  const int re = select_end(h, s);
  for (int c = 0; c < h->st.nclass; ++c) after += arena_bytes(h, c) + workspace_bytes(h, c);
  if (demoted) *demoted = dem;
  if (bytes_freed) *bytes_freed = before - after;
  return rc ? rc : re;
}

int gk_class_usage(gk_set* h, int cls, int64_t* streams, int64_t* slots_used, int64_t* slots_alloc,
                   int64_t* arena_bytes_out, int64_t* workspace_bytes_out, void* stream) {
  int rc = check_set(h);
  if (rc) return rc;
  if (cls < 0 || cls >= h->st.nclass) return fail(GK_E_ARG, "class %d outside [0, %d)", cls, h->st.nclass);
  hipStream_t s = (hipStream_t)stream;
  // settled as gk_num_promoted settles: deferred streams are placed first; a
  // sticky error stays for the next call that reports one
  HIP_TRY(hipStreamSynchronize(s));
  rc = settle(h, s, true);
  if (rc) return rc;
  int64_t members = 0;
  int32_t used = 0;
  if (h->S > 0) {
    std::vector<int32_t> c(h->S);
    HIP_TRY(hipMemcpy(c.data(), h->st.cls, h->S * sizeof(int32_t), hipMemcpyDeviceToHost));
    for (int32_t v : c) members += v == cls;
    if (cls > 0) HIP_TRY(hipMemcpy(&used, h->d_ctr + GK_CTR_USED + cls, sizeof(int32_t), hipMemcpyDeviceToHost));
  }
  if (streams) *streams = members;
  if (slots_used) *slots_used = cls == 0 ? h->S : used;
  if (slots_alloc) *slots_alloc = cls == 0 ? h->S : h->st.alloc[cls];
  if (arena_bytes_out) *arena_bytes_out = arena_bytes(h, cls);
  if (workspace_bytes_out) *workspace_bytes_out = workspace_bytes(h, cls);
  return GK_OK;
}

// ---- key directory (gk_dir.hip) ----------------------------------------------
}  // extern "C"

struct gk_dir {
  int64_t capacity = 0;
  int64_t size = 0;   // keys held
  int64_t bound = 0;  // one past the largest id handed out; size + nfree == bound
  int device = 0;
  GKDirTable t = {};
  // the ids of [0, bound) that no key holds: d_free[head .. head + nfree), ascending
  int32_t* d_free = nullptr;  // [capacity]
  int64_t head = 0;
  int64_t nfree = 0;
  int64_t dead = 0;  // upper bound on slots that hold a removed key (zero after a rebuild or an import)
  // scratch of assign / import (only grows): per sample its slot and its flag,
  // scanned in place into its rank; the scan's tile sums; the control words
  uint32_t* d_slot = nullptr;
  uint32_t* d_flag = nullptr;
  unsigned long long* d_sums = nullptr;
  int64_t scratch_n = 0;
  unsigned long long* d_ctl = nullptr;  // GK_DIR_CTL_WORDS
};

namespace {

void dir_free_table(GKDirTable* t) {
  for (void* p : {(void*)t->keys, (void*)t->meta, (void*)t->key_of_id})
    if (p) (void)hipFree(p);
  t->keys = nullptr;
  t->meta = nullptr;
  t->key_of_id = nullptr;
}

// a cleared table of the geometry of `like` (pointers of *t are overwritten)
int dir_new_table(const GKDirTable& like, GKDirTable* t, hipStream_t s) {
  *t = like;
  t->keys = nullptr;
  t->meta = nullptr;
  t->key_of_id = nullptr;
  const size_t T = (size_t)like.T;
  if (!renew_dev(&t->keys, T * sizeof(unsigned long long)) || !renew_dev(&t->meta, T * sizeof(uint2)) ||
      !renew_dev(&t->key_of_id, (size_t)like.capacity * sizeof(int64_t))) {
    dir_free_table(t);
    return fail(GK_E_NOMEM, "directory: no device memory for a table of %zu slots", T);
  }
  HIP_TRY(gk_launch_dir_clear(*t, s));
  return GK_OK;
}

int dir_ensure_scratch(gk_dir* d, int64_t n) {
  if (n <= d->scratch_n) return GK_OK;
  HIP_TRY(hipDeviceSynchronize());  // (nothing of this directory is in flight: its calls synchronise)
  d->scratch_n = 0;
  if (!renew_dev(&d->d_slot, (size_t)n * sizeof(uint32_t)) || !renew_dev(&d->d_flag, (size_t)n * sizeof(uint32_t)) ||
      !renew_dev(&d->d_sums, (size_t)gk_scan_sums(n) * sizeof(unsigned long long)))
    return fail(GK_E_NOMEM, "directory: no device memory for the scratch of %lld samples", (long long)n);
  d->scratch_n = n;
  return GK_OK;
}

// The control words of the call that just ran on s, after a synchronise.
int dir_read_ctl(gk_dir* d, unsigned long long* ctl, hipStream_t s) {
  HIP_TRY(hipMemcpyAsync(ctl, d->d_ctl, GK_DIR_CTL_WORDS * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  return GK_OK;
}

// keys[i] -> i into the cleared table t, GK_DIR_NONE entries skipped (import, and the rebuilds)
int dir_fill(gk_dir* d, const GKDirTable& t, const int64_t* keys, int64_t count, hipStream_t s) {
  HIP_TRY(hipMemsetAsync(d->d_ctl, 0, GK_DIR_CTL_WORDS * sizeof(unsigned long long), s));
  HIP_TRY(gk_launch_dir_insert(t, keys, count, d->d_slot, d->d_ctl, s));
  HIP_TRY(gk_launch_dir_number(t, keys, d->d_slot, nullptr, count, nullptr, 0, 0, d->d_ctl, s));
  return GK_OK;
}

// The table again from the inverse array, which holds GK_DIR_NONE at free ids:
// every slot a void call claimed or a removed key kept is empty afterwards.
int dir_rebuild(gk_dir* d, hipStream_t s) {
  HIP_TRY(gk_launch_dir_clear(d->t, s));
  int rc = dir_fill(d, d->t, d->t.key_of_id, d->bound, s);  // (GK_DIR_CTL_NONE: the free ids, no error here)
  if (rc) return rc;
  d->dead = 0;
  return GK_OK;
}

// d_free = the free ids of [0, bound), from the inverse array (nfree is known: bound - size)
int dir_refresh_free(gk_dir* d, hipStream_t s) {
  d->head = 0;
  d->nfree = d->bound - d->size;
  if (d->nfree > 0)
    HIP_TRY(gk_launch_dir_free_list(d->t, d->bound, d->d_flag, d->d_sums, d->d_free, nullptr, s));
  return GK_OK;
}

// gk_dir_import (sparse false: a GK_DIR_NONE entry is refused) and gk_dir_import_sparse
int dir_import(gk_dir* d, const int64_t* keys, int64_t count, bool sparse, hipStream_t s) {
  if (count > d->capacity) return fail_dir_import_count(count, d->capacity);
  int rc = dir_ensure_scratch(d, std::max(count, d->bound));
  if (rc) return rc;
  GKDirTable nt;
  rc = dir_new_table(d->t, &nt, s);
  unsigned long long ctl[GK_DIR_CTL_WORDS] = {};
  if (!rc) rc = dir_fill(d, nt, keys, count, s);
  if (!rc) rc = dir_read_ctl(d, ctl, s);
  if (!rc && !sparse && ctl[GK_DIR_CTL_NONE]) rc = fail_dir_import_none(count - (int64_t)ctl[GK_DIR_CTL_NONE]);
  if (!rc && ctl[GK_DIR_CTL_DUP]) {
    const int64_t idx = count - (int64_t)ctl[GK_DIR_CTL_DUP];
    int64_t key = 0;
    if (hipMemcpy(&key, keys + idx, sizeof(key), hipMemcpyDeviceToHost) != hipSuccess)
      rc = fail(GK_E_HIP, "directory: device-to-host copy failed");
    else
      rc = fail_dir_import_repeat(idx, key);
  }
  if (!rc && ctl[GK_DIR_CTL_OVF]) rc = fail(GK_E_HIP, "directory: import ran out of slots");  // (count <= capacity: never)
  if (rc) {
    (void)hipStreamSynchronize(s);
    dir_free_table(&nt);
    return rc;
  }
  dir_free_table(&d->t);
  d->t = nt;
  d->bound = count;
  d->size = count;
  d->head = d->nfree = d->dead = 0;
  if (sparse && ctl[GK_DIR_CTL_NONE]) {
    // the free ids, counted by the scan
    HIP_TRY(hipMemsetAsync(d->d_ctl, 0, GK_DIR_CTL_WORDS * sizeof(unsigned long long), s));
    HIP_TRY(gk_launch_dir_free_list(d->t, count, d->d_flag, d->d_sums, d->d_free, d->d_ctl + GK_DIR_CTL_NEW, s));
    rc = dir_read_ctl(d, ctl, s);
    if (rc) return rc;
    d->nfree = (int64_t)ctl[GK_DIR_CTL_NEW];
    d->size = count - d->nfree;
  }
  return GK_OK;
}

}  // namespace

extern "C" {

int gk_dir_create(int64_t capacity, int device, gk_dir** out) {
  int rc = check_dir_create(capacity, out);
  if (rc) return rc;
  GKDirTable like = {};
  like.T = (uint32_t)gk_dir_slots(capacity);
  like.capacity = capacity;
  if (!gk_dir_home_from_env((int64_t)like.T, &like.home))
    return fail(GK_E_ARG, "GK_DIR_HASH_BITS=%s: a number >= 0", getenv("GK_DIR_HASH_BITS"));
  int dev_count = 0;
  if (hipGetDeviceCount(&dev_count) != hipSuccess || dev_count <= 0) return fail(GK_E_HIP, "no HIP device available");
  if (device < 0 || device >= dev_count) return fail(GK_E_ARG, "device %d out of range", device);
  HIP_TRY(hipSetDevice(device));
  gk_dir* d = new gk_dir();
  d->capacity = capacity;
  d->device = device;
  rc = dir_new_table(like, &d->t, nullptr);
  if (!rc && (!renew_dev(&d->d_ctl, GK_DIR_CTL_WORDS * sizeof(unsigned long long)) ||
              !renew_dev(&d->d_free, (size_t)capacity * sizeof(int32_t))))
    rc = fail(GK_E_NOMEM, "directory: no device memory for the control words and the free ids");
  if (!rc && hipStreamSynchronize(nullptr) != hipSuccess) rc = fail(GK_E_HIP, "directory: clearing the table failed");
  if (rc) {
    gk_dir_destroy(d);
    return rc;
  }
  *out = d;
  return GK_OK;
}

int gk_dir_destroy(gk_dir* d) {
  if (!d) return GK_OK;
  (void)hipDeviceSynchronize();
  dir_free_table(&d->t);
  for (void* p : {(void*)d->d_slot, (void*)d->d_flag, (void*)d->d_sums, (void*)d->d_ctl, (void*)d->d_free})
    if (p) (void)hipFree(p);
  delete d;
  return GK_OK;
}

int64_t gk_dir_capacity(const gk_dir* d) { return d ? d->capacity : -1; }
int64_t gk_dir_size(const gk_dir* d) { return d ? d->size : -1; }
int64_t gk_dir_bound(const gk_dir* d) { return d ? d->bound : -1; }

int gk_dir_assign(gk_dir* d, const int64_t* keys, int64_t count, int32_t* out_ids, int64_t* num_new, void* stream) {
  int rc = check_dir_args(d, keys, count, out_ids, true);
  if (rc) return rc;
  hipStream_t s = (hipStream_t)stream;
  if (count == 0) {
    HIP_TRY(hipStreamSynchronize(s));
    if (num_new) *num_new = 0;
    return GK_OK;
  }
  rc = dir_ensure_scratch(d, std::max(count, d->bound));
  if (rc) return rc;
  HIP_TRY(hipMemsetAsync(d->d_ctl, 0, GK_DIR_CTL_WORDS * sizeof(unsigned long long), s));
  HIP_TRY(hipMemsetAsync(d->d_ctl + GK_DIR_CTL_IDLE, 1, sizeof(unsigned long long), s));  // (any non-zero word)
  HIP_TRY(gk_launch_dir_insert(d->t, keys, count, d->d_slot, d->d_ctl, s));
  HIP_TRY(gk_launch_dir_flag(d->t, d->d_slot, count, d->d_flag, d->d_ctl, s));
  static_assert(GK_KG_BAD == 0, "the scan reads its skip word at index GK_KG_BAD");
  HIP_TRY(gk_launch_scan_u32(d->d_flag, count, d->d_sums, d->d_ctl + GK_DIR_CTL_IDLE, d->d_ctl + GK_DIR_CTL_NEW, s));
  HIP_TRY(gk_launch_dir_number(d->t, keys, d->d_slot, d->d_flag, count, d->d_free + d->head, d->nfree, d->bound,
                               d->d_ctl, s));
  HIP_TRY(gk_launch_dir_lookup(d->t, keys, d->d_slot, count, out_ids, s));
  unsigned long long ctl[GK_DIR_CTL_WORDS];
  rc = dir_read_ctl(d, ctl, s);
  if (rc) return rc;
  const int64_t fresh = (int64_t)ctl[GK_DIR_CTL_NEW];
  if (ctl[GK_DIR_CTL_OVF] || fresh > d->capacity - d->size) {
    // void call (k_dir_number wrote nothing): the slots it claimed go with a
    // rebuild of the table from the inverse array, which no void call touches
    rc = dir_rebuild(d, s);
    if (rc) return rc;
    HIP_TRY(hipStreamSynchronize(s));
    return fail_dir_overflow(d->capacity, d->size);
  }
  const int64_t recycled = std::min(fresh, d->nfree);
  d->head += recycled;
  d->nfree -= recycled;
  d->bound += fresh - recycled;
  d->size += fresh;
  if (num_new) *num_new = fresh;
  return GK_OK;
}

// Removed keys keep their slots.  The table is rebuilt once `dead`, an upper
// bound on such slots, passes T/4: used slots <= capacity + T/4 <= 3T/4, so a
// batch that fits `capacity` always finds slots, and every rebuild is paid for
// by more than T/4 removals.
int gk_dir_remove(gk_dir* d, const int64_t* keys, int64_t count, int32_t* out_ids, int64_t* num_removed,
                  void* stream) {
  int rc = check_dir_args(d, keys, count, out_ids, true);
  if (rc) return rc;
  hipStream_t s = (hipStream_t)stream;
  if (count == 0) {
    HIP_TRY(hipStreamSynchronize(s));
    if (num_removed) *num_removed = 0;
    return GK_OK;
  }
  rc = dir_ensure_scratch(d, std::max(count, d->bound));
  if (rc) return rc;
  HIP_TRY(hipMemsetAsync(d->d_ctl, 0, GK_DIR_CTL_WORDS * sizeof(unsigned long long), s));
  HIP_TRY(gk_launch_dir_remove(d->t, keys, count, d->d_slot, out_ids, d->d_ctl, s));
  unsigned long long ctl[GK_DIR_CTL_WORDS];
  rc = dir_read_ctl(d, ctl, s);
  if (rc) return rc;
  const int64_t removed = (int64_t)ctl[GK_DIR_CTL_NEW];
  if (removed > 0) {
    d->size -= removed;
    d->dead += removed;
    rc = dir_refresh_free(d, s);
    if (!rc && d->dead > (int64_t)d->t.T / 4) rc = dir_rebuild(d, s);
    if (rc) return rc;
    HIP_TRY(hipStreamSynchronize(s));
  }
  if (num_removed) *num_removed = removed;
  return GK_OK;
}

int gk_dir_lookup(gk_dir* d, const int64_t* keys, int64_t count, int32_t* out_ids, void* stream) {
  int rc = check_dir_args(d, keys, count, out_ids, true);
  if (rc) return rc;
  hipStream_t s = (hipStream_t)stream;
  HIP_TRY(gk_launch_dir_lookup(d->t, keys, nullptr, count, out_ids, s));
  HIP_TRY(hipStreamSynchronize(s));
  return GK_OK;
}

int gk_dir_keys(gk_dir* d, int64_t* out_keys, void* stream) {
  int rc = check_dir(d);
  if (rc) return rc;
  hipStream_t s = (hipStream_t)stream;
  if (d->bound > 0) {
    if (!out_keys) return fail(GK_E_ARG, "out_keys is null");
    HIP_TRY(hipMemcpyAsync(out_keys, d->t.key_of_id, (size_t)d->bound * sizeof(int64_t), hipMemcpyDeviceToDevice, s));
  }
  HIP_TRY(hipStreamSynchronize(s));
  return GK_OK;
}

int gk_dir_import(gk_dir* d, const int64_t* keys, int64_t count, void* stream) {
  int rc = check_dir_args(d, keys, count, nullptr, false);
  if (rc) return rc;
  return dir_import(d, keys, count, false, (hipStream_t)stream);
}

int gk_dir_import_sparse(gk_dir* d, const int64_t* keys, int64_t count, void* stream) {
  int rc = check_dir_args(d, keys, count, nullptr, false);
  if (rc) return rc;
  return dir_import(d, keys, count, true, (hipStream_t)stream);
}

int64_t gk_num_streams(const gk_set* h) { return h ? h->S : -1; }
double gk_eps(const gk_set* h) { return h ? h->eps : 0.0; }
int gk_flush_period(const gk_set* h) { return h ? h->P : -1; }
int gk_capacity(const gk_set* h, int cls) {
  return (h && cls >= 0 && cls < h->st.nclass) ? h->st.cap[cls] : -1;
}

int64_t gk_num_promoted(const gk_set* h) {
  if (!h) return -1;
  if (h->S == 0) return 0;
  if (hipDeviceSynchronize() != hipSuccess) return -1;
  if (settle(const_cast<gk_set*>(h), nullptr, true) != GK_OK) return -1;  // deferred streams placed first
  std::vector<int32_t> cls(h->S);
  if (hipMemcpy(cls.data(), h->st.cls, h->S * sizeof(int32_t), hipMemcpyDeviceToHost) != hipSuccess) return -1;
  int64_t n = 0;
  for (int32_t c : cls) n += c > 0;
  return n;
}

int gk_timing_enable(gk_set* h, int on) {
  int rc = check_set(h);
  if (rc) return rc;
  h->timing = (on & 1) != 0;
  h->timing_stats = (on & 2) != 0;
  return GK_OK;
}

int gk_timing_read(gk_set* h, double* flush_ms, double* stats_ms, int64_t* launches) {
  int rc = check_set(h);
  if (rc) return rc;
  double f = 0, st = 0;
  for (size_t k = 0; k + 1 < h->n_flush; k += 2) {
    float ms = 0;
    HIP_TRY(hipEventSynchronize(h->tev_flush[k + 1]));
    HIP_TRY(hipEventElapsedTime(&ms, h->tev_flush[k], h->tev_flush[k + 1]));
    f += ms;
  }
  for (size_t k = 0; k + 1 < h->n_stats; k += 2) {
    float ms = 0;
    HIP_TRY(hipEventSynchronize(h->tev_stats[k + 1]));
    HIP_TRY(hipEventElapsedTime(&ms, h->tev_stats[k], h->tev_stats[k + 1]));
    st += ms;
  }
  if (flush_ms) *flush_ms = f;
  if (stats_ms) *stats_ms = st;
  if (launches) *launches = (int64_t)(h->n_flush / 2);
  h->n_flush = h->n_stats = 0;
  return GK_OK;
}

}  // extern "C"
