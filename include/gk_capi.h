/*
 * gk_capi.h -- C ABI of the MI355X-native batched GKArray engine.
 *
 * The reference (githomin/sketches-py, gkarray/gkarray.py, "gk:N" = line N) is a
 * pure-Python class with no FFI.  This header is the boundary a ctypes (or cgo /
 * JNI) binding binds; each entry point names the reference method it replaces.
 * A "set" holds S independent GKArray streams that share one epsilon; every
 * stream behaves exactly like one reference ``GKArray`` object fed the same
 * values in the same order (tables and quantiles bit-exact).
 *
 * Conventions
 *  - Every call returns an int status: GK_OK (0) or a negative GK_E_* code;
 *    gk_last_error() returns a thread-local message for the last failure.
 *  - Pointers documented "device" must be device memory on the set's GPU
 *    (e.g. a torch tensor's data_ptr()); "host" pointers are host memory.
 *  - `stream` is a hipStream_t passed as void* (NULL = the default stream).
 *    All calls on one set must be ordered on one stream.  gk_ingest,
 *    gk_ingest_quantiles, gk_flush, gk_quantiles, gk_stats and the exports
 *    only ENQUEUE their work and return (no host synchronisation): a stream
 *    whose table outgrows its capacity class is moved to the next class and
 *    re-run by the device itself.  Part of an ingest (the sequential
 *    _sum/_avg chains of streams longer than 16384 values) runs on a stream
 *    the set owns; `stream` is made to wait for it, so every later call
 *    enqueued on `stream` sees the finished state.  The caller keeps input
 *    buffers alive and unchanged until the set's next call or gk_sync: a
 *    stream that needs a class whose arena has no free slot yet is deferred
 *    and re-run from them by the host runtime before the next call proceeds.
 *    gk_merge, gk_rollup, gk_quantiles_select, gk_flush_select,
 *    gk_reset_select, gk_stats_select, gk_ranks, gk_ranks_select,
 *    gk_ranks_keyed, gk_merge_compress, gk_import, gk_save / gk_load, gk_pack_select_bytes,
 *    gk_pack_select, gk_unpack_select, gk_compact, gk_class_usage and
 *    gk_num_promoted synchronise before
 *    returning; so do the key directory's calls (gk_dir_*, an object of its
 *    own).  gk_rank_ingest_keyed synchronises for its rank half's checks and
 *    flush and then only enqueues (see there).
 *  - Limits.  Any finite eps > 0 with int(1/eps)+1 < 2^24 is accepted (the
 *    reference: any eps; eps > 1 gives a flush period of 1, gk:60); tables grow through capacity classes up to 2^27 entries per
 *    stream (the last classes are allocated on first use).  One stream may
 *    hold n values while 2*eps*(n-1) <= 2^30 (5.4e10 values at eps=0.01):
 *    its tuples' g and delta are int32 (GKRec).
 *  - Asynchronous errors: a stream that would pass a limit above (or finds no
 *    memory for its class) is refused: its table, pending values and n keep
 *    their pre-call state (_min/_max/_sum/_avg, computed beside the tables,
 *    include the call's values), and GK_E_OVERFLOW is reported by a later
 *    call on the set, at the latest by gk_sync.
 *  - A set is not thread-safe.  The library owns the set's device state;
 *    callers own their input and output buffers.
 */
#ifndef GK_CAPI_H
#define GK_CAPI_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GK_OK 0
#define GK_E_ARG (-1)          /* bad argument (size, pointer, NaN quantile ...)   */
#define GK_E_EPS_MISMATCH (-2) /* merge of sets with different eps: gk:118-119     */
#define GK_E_OVERFLOW (-3)     /* a stream passed a limit (table size, count)     */
#define GK_E_HIP (-4)          /* HIP runtime failure                              */
#define GK_E_NOMEM (-5)        /* device allocation failed                          */
#define GK_E_UNSUPPORTED (-6)  /* eps below ~6e-8 (flush period beyond 2^24)       */
#define GK_E_IO (-7)           /* state file cannot be opened / written            */
#define GK_E_FORMAT (-8)       /* state file malformed, wrong version or checksum  */

typedef struct gk_set gk_set;

/* Library / ABI version (major*10000 + minor*100 + patch). */
int gk_version(void);

/* Message for the last failed call on this thread ("" if none). */
const char* gk_last_error(void);

/* GKArray(eps) for `num_streams` streams (gk:21-29): empty tables, n=0,
 * min=+inf, max=-inf, sum=avg=0.  `device` is the HIP device ordinal.
 * `cap_hint` (0 = default, < 2^27) is the per-stream table capacity the set
 * starts with; streams whose table outgrows it are promoted to a larger class
 * automatically. */
int gk_create(int64_t num_streams, double eps, int64_t cap_hint, int device,
              gk_set** out);
int gk_destroy(gk_set* set);

/* Reset every stream to the freshly constructed state (gk:21-29).  Does not
 * wait for the set's last call: streams that call deferred are not re-run,
 * their state being void -- unless that call carried a fused query and has not
 * been settled yet (by gk_sync or any later call): the re-run writes those
 * streams' rows of the query's output, so it is settled first. */
int gk_reset(gk_set* set, void* stream);

/* Batched GKArray.add (gk:49-61): stream s receives, in order,
 * values[offsets[s] .. offsets[s+1]).  `values` (float64, device) and
 * `offsets` (int64[num_streams+1], device, non-decreasing) describe a CSR
 * batch over ALL streams of the set.  Flushes (merge_compress, gk:63-109)
 * happen at exactly the reference's flush points (n % (int(1/eps)+1) == 0). */
int gk_ingest(gk_set* set, const double* values, const int64_t* offsets,
              void* stream);

/* Keyed ingest: samples in arrival order, (ids[i], values[i]) for i in
 * [0, count), instead of a CSR batch.
 *
 * gk_group_by_key is the stable group-by of the samples into a CSR batch over
 * the set's S streams; gk_ingest_keyed is
 *     for i in [0, count): stream ids[i] .add(values[i])        (gk:49-61)
 * and then, nq > 0, quantiles(qs) of every stream as gk_ingest_quantiles does.
 *  - Memory and sizes.  `ids` (int32), `values` (float64), `out_values` (room
 *    for `count` doubles) and `out_offsets` (int64[S+1]) are device memory for
 *    the GPU engine, host memory for the CPU engine.  0 <= count <= 2^31-1,
 *    anything else is GK_E_ARG.  count == 0 is valid (an ingest of an empty
 *    batch; with nq > 0 exactly gk_quantiles), and `ids`, `values` and
 *    `out_values` may then be NULL.
 *  - Grouping rule.  Stream s receives the values whose id is s in ascending
 *    sample index (the grouping is a STABLE sort by id).  Values are copied
 *    bit for bit (-0.0, NaN payloads, infinities, denormals).
 *    out_offsets[s+1] - out_offsets[s] is the number of samples with id s,
 *    out_offsets[0] == 0; out_values[0 .. out_offsets[S]) is written.
 *  - Negative ids are skipped ("not for this set").
 *  - An id >= S is an error.  The GPU engine finds it on the device and reports
 *    it as it reports GK_E_OVERFLOW: GK_E_ARG from a later call on the set, at
 *    the latest from gk_sync, with the first bad sample index and its id in
 *    the message (the host engine returns GK_E_ARG from the call itself).  The
 *    call then adds no value to any stream: gk_group_by_key leaves out_offsets
 *    all zero, and a query fused into gk_ingest_keyed answers as gk_quantiles
 *    would from the pre-call state (which flushes pending values).
 *  - Both calls only enqueue, as gk_ingest does.  The caller keeps `ids`,
 *    `values` and the outputs alive and unchanged until the set's next call or
 *    gk_sync.  A call that has to grow the set's grouping scratch synchronises
 *    first; GK_E_NOMEM is returned before anything is mutated.
 *  - gk_ingest_keyed is gk_group_by_key into buffers the set owns, followed by
 *    exactly gk_ingest (nq == 0) or gk_ingest_quantiles on those buffers; qs,
 *    nq, out and mode are checked as gk_ingest_quantiles checks them.  S == 0
 *    returns GK_OK.
 *  - Scratch (GPU engine; owned by the set, only grows, freed by gk_destroy):
 *    two (int32 id, float64 value) pair buffers of `count` entries, 24 bytes
 *    per sample (S > 65536, three or more radix passes; 16 bytes for
 *    256 < S <= 65536, 4 bytes for S <= 256), 0.25 byte per sample of
 *    per-workgroup digit counts, and for gk_ingest_keyed the grouped batch:
 *    8 bytes per sample + 8 (S+1) bytes. */
int gk_group_by_key(gk_set* set, const int32_t* ids, const double* values, int64_t count,
                    double* out_values, int64_t* out_offsets, void* stream);
int gk_ingest_keyed(gk_set* set, const int32_t* ids, const double* values, int64_t count,
                    const double* qs, int nq, double* out, int mode, void* stream);

/* Wait for the set's work on `stream`; return (and clear) an asynchronous
 * error of an earlier call (GK_E_OVERFLOW, see Conventions; GK_E_ARG for an
 * id >= S of a keyed call) or GK_OK. */
int gk_sync(gk_set* set, void* stream);

/* GKArray.merge_compress() with no argument (gk:63-109) on every stream that
 * has pending values -- what size()/quantile()/quantiles() do first
 * (gk:45-46, 166-167, 197-198). */
int gk_flush(gk_set* set, void* stream);

/* Batched GKArray.quantiles(qs) (gk:187-232) for every stream.
 * `qs` (host, nq float64 values, no NaN); `out` (device, float64[S*nq],
 * row-major [stream][q]).  Pending values are flushed first (mutation, as in
 * the reference).  mode GK_Q_LIST = quantiles() semantics (the caller passes
 * qs as given; if they are not sorted the per-q quantile() result is used,
 * exactly as gk:205-206 does); mode GK_Q_SINGLE = quantile(q) semantics for
 * every q (gk:156-185). */
#define GK_Q_LIST 0
#define GK_Q_SINGLE 1
int gk_quantiles(gk_set* set, const double* qs, int nq, double* out, int mode,
                 void* stream);

/* gk_ingest followed by gk_quantiles, fused: every stream adds its values
 * (gk:49-61), then answers quantiles(qs) (gk:187-232) -- the leftover pending
 * values are flushed first, as the reference does -- from the table while it
 * is still on chip.  Same arguments and semantics as the two calls. */
int gk_ingest_quantiles(gk_set* set, const double* values, const int64_t* offsets,
                        const double* qs, int nq, double* out, int mode, void* stream);

/* Per-stream accessors num_values/_min/_max/sum/avg (gk:35-42, 25-29) and the
 * table size len(entries) / pending count len(incoming) WITHOUT flushing.
 * Any pointer may be NULL.  All outputs are device arrays of length S. */
int gk_stats(gk_set* set, int64_t* n, double* mn, double* mx, double* sum,
             double* avg, int32_t* table_size, int32_t* pending, void* stream);

/* Per-stream selection: query, flush, reset and stats of a LIST of streams,
 * what the reference's user does on a dict of GKArray objects one key at a
 * time (sketches[k].quantiles(qs); sketches[k] = GKArray(eps); sketches[k]._n).
 * gk_quantiles / gk_flush / gk_reset / gk_stats work on every stream of the
 * set; these touch only the streams listed in ids[0 .. count).
 *  - Memory.  `ids` (int32), `out` and the stats outputs are device memory
 *    for the GPU engine, host memory for the CPU engine.  `qs` is host memory,
 *    as in gk_quantiles.
 *  - Count.  0 <= count <= 2^31-1, anything else is GK_E_ARG.  count == 0
 *    returns GK_OK and touches no stream (`ids` may then be NULL); a NULL `ids`
 *    with count > 0 is GK_E_ARG.
 *  - Bad ids.  An id outside [0, S) -- negative ids included: a query has no
 *    "not for this set" row -- is GK_E_ARG, returned by the call itself BEFORE
 *    anything is mutated or written, with the first bad index and its id in
 *    the message.
 *  - Duplicates.  Ids may repeat and come in any order.  Row k of an output
 *    always belongs to ids[k]; a stream listed twice is flushed or reset once
 *    and answered twice with the same bits.
 *  - Synchronisation.  All four calls synchronise before returning, after
 *    settling the set's earlier asynchronous work and errors (gk_sync first,
 *    as gk_rollup does: deferred streams of the previous call are re-run, a
 *    sticky error of it is returned instead of doing the work).
 *  - Unlisted streams stay bit-identical: table, pending values and
 *    n/_min/_max/_sum/_avg (GPU engine: also capacity class and slot).
 *
 * gk_quantiles_select: `out` is float64[count*nq], row-major [k][q]; row k is
 *   GKArray.quantiles(qs) (GK_Q_LIST) or quantile(q) for every q (GK_Q_SINGLE)
 *   of stream ids[k], with the argument checks and the effective mode of
 *   gk_quantiles (NaN in qs: GK_E_ARG; an unsorted list is answered per q).
 *   nq == 0 returns GK_OK after the id check and touches nothing.  Flush rule:
 *   gk_quantiles' rule restricted to the listed streams -- a listed stream
 *   with n > 0 and pending values runs merge_compress() first (gk:166-167,
 *   gk:197-198); a listed stream without pending values is NOT compressed
 *   again (gk_rollup, by contrast, flushes its members unconditionally).  A
 *   listed stream whose flush outgrows its capacity class moves up, as
 *   roll-up members do; one that outgrows the last class makes the call
 *   return GK_E_OVERFLOW: that stream keeps its pre-call state, the other
 *   listed streams have been flushed, `out` is not written.
 * gk_flush_select: that flush and nothing else -- what size() does first
 *   (gk:45-46).
 * gk_reset_select: each listed stream goes back to GKArray(eps) (gk:21-29):
 *   empty table, no pending values, n = 0, min = +inf, max = -inf, sum = avg
 *   = 0.  On the GPU engine a reset stream KEEPS its capacity class and slot
 *   (arenas are bump-allocated and the class member lists have no removal):
 *   memory is not returned and gk_num_promoted does not drop until gk_compact
 *   re-places the streams; gk_reset gives everything back at once.
 * gk_stats_select: gk_stats' seven arrays gathered at ids into outputs of
 *   length `count`; any output pointer may be NULL.  Does not flush.
 *  - Scratch (GPU engine; owned by the set, only grows, freed by gk_destroy):
 *    S/8 bytes + 4 bytes per listed id (at most 4 S).  GK_E_NOMEM is returned
 *    before anything is mutated. */
int gk_quantiles_select(gk_set* set, const int32_t* ids, int64_t count,
                        const double* qs, int nq, double* out, int mode, void* stream);
int gk_flush_select(gk_set* set, const int32_t* ids, int64_t count, void* stream);
int gk_reset_select(gk_set* set, const int32_t* ids, int64_t count, void* stream);
int gk_stats_select(gk_set* set, const int32_t* ids, int64_t count,
                    int64_t* n, double* mn, double* mx, double* sum, double* avg,
                    int32_t* table_size, int32_t* pending, void* stream);

/* Rank queries: bounds on each stream's count of values <= x, the inverse of
 * gk_quantiles.  The reference has no rank(); the answer is defined on the
 * reference's state (entries, _n, _min, _max) and is integer-exact.
 *  - Contract.  A stream, after the flush below, has the table (v_k, g_k, d_k),
 *    k = 0..E-1 (ascending in v), and n, _min, _max.  G(k) = g_0 + .. + g_{k-1},
 *    G(0) = 0.  rank(x) is the int64 pair (lo, hi), rules applied in this order:
 *        n == 0     ->  (0, 0)
 *        x <  _min  ->  (0, 0)
 *        x >= _max  ->  (n, n)
 *        otherwise, with i = #{k : v_k <= x}:
 *            lo = max(G(i), 1)
 *            hi = min(i < E ? G(i+1) + d_i - 1 : n,  n - 1)
 *    Comparisons are IEEE (-0.0 == 0.0; +-inf are ordinary thresholds).
 *    Thresholds are answered independently: any order, repeats allowed.  A
 *    stream that was fed NaN values is outside the contract (the reference's
 *    own _min/_max then depend on the order of the values).
 *  - Meaning.  For a stream built by adds alone, lo <= #{values <= x} <= hi
 *    and hi - lo <= 2 eps n.  After gk_merge, gk_rollup or gk_fold_packed the
 *    reference's conversion (gk:135-147) no longer keeps the invariants the
 *    bracket rests on: lo <= hi still holds, the true count may lie outside.
 *    The pair is the formula on the table in every case, never "repaired".
 *  - Memory.  `xs` (nx float64 values, no NaN) is host memory, as `qs` is.
 *    `lo` and `hi` are int64[rows*nx], row-major [row][x], device memory for
 *    the GPU engine, host memory for the CPU engine; rows are the S streams
 *    (gk_ranks) or ids[k], k in [0, count) (gk_ranks_select).  One of `lo` and
 *    `hi` may be NULL.
 *  - GK_E_ARG, before anything is mutated or written: nx < 0; nx > 0 with
 *    `xs` NULL or with both outputs NULL; a NaN in xs; count and ids as
 *    gk_quantiles_select reports them (the first bad index and its id in the
 *    message).  nx == 0 returns GK_OK after the argument and id checks and
 *    touches no stream; so does count == 0.
 *  - Flush rule: gk_quantiles' rule.  A covered stream (every stream; the
 *    listed ones) with n > 0 and pending values runs merge_compress() first
 *    (gk:166-167); one with nothing pending is NOT compressed again.  Ranks and
 *    quantiles are then answered from the same table.  Unlisted streams stay
 *    bit-identical, as for the other _select calls.
 *  - GK_E_OVERFLOW: a covered stream whose flush outgrows the last capacity
 *    class keeps its pre-call state, the other covered streams have been
 *    flushed, `lo` and `hi` are not written.
 *  - Synchronisation.  Both calls synchronise before returning, after settling
 *    the set's earlier asynchronous work and errors (gk_sync first).  The
 *    device copy of xs is made before the flush: its GK_E_NOMEM mutates
 *    nothing. */
int gk_ranks(gk_set* set, const double* xs, int nx, int64_t* lo, int64_t* hi, void* stream);
int gk_ranks_select(gk_set* set, const int32_t* ids, int64_t count,
                    const double* xs, int nx, int64_t* lo, int64_t* hi, void* stream);

/* Keyed rank queries: rank bounds per (stream id, value) sample -- "where does
 * this value sit in the distribution of the series it belongs to?", for every
 * sample of a batch in one call (the query-side counterpart of
 * gk_ingest_keyed; ids as the key directory hands them out).
 *  - Rows.  Row i belongs to the sample (ids[i], xs[i]), i in [0, count).  `lo`,
 *    `hi` and `n` are int64[count].
 *  - Memory.  `ids` (int32), `xs` (float64), `lo`, `hi` and `n` are device
 *    memory for the GPU engine, host memory for the CPU engine.  Any of the
 *    three outputs may be NULL, but not all three.
 *  - Answer.  For ids[i] in [0, S), (lo[i], hi[i]) is exactly what
 *    gk_ranks_select(set, &ids[i], 1, &xs[i], 1, ...) answers on the state after
 *    the flush below: the four rules of the rank contract above,
 *    integer-exact.  n[i] is that stream's _n.  Ids may repeat any number of
 *    times and come in any order.
 *  - Negative ids.  A negative id is "no stream", as in gk_ingest_keyed and as
 *    gk_dir_lookup answers for an unknown key: the row gets lo = hi = n = 0,
 *    the answer of an empty sketch.  xs[i] of such a row is not examined and
 *    may be NaN.
 *  - GK_E_ARG, from the call itself, before anything is mutated or written:
 *    count outside [0, 2^31-1]; a NULL `ids` or `xs` with count > 0; all three
 *    outputs NULL; an id >= S; a NaN xs[i] on a row whose id is >= 0.  The
 *    message names the smallest offending sample index and its id or the word
 *    NaN; a sample with both faults is reported by its id.
 *  - count == 0 returns GK_OK after the argument checks and touches nothing.
 *  - Flush rule: gk_ranks_select's rule, applied to the streams that occur in
 *    ids.  Such a stream with n > 0 and pending values runs merge_compress()
 *    first, once; one with nothing pending is NOT compressed again.  Streams
 *    that do not occur stay bit-identical (GPU engine: class and slot too).
 *  - GK_E_OVERFLOW as for gk_ranks_select: the stream that outgrew the last
 *    capacity class keeps its pre-call state, the other occurring streams have
 *    been flushed, no output is written.
 *  - Synchronisation.  gk_sync first (deferred streams of the previous call are
 *    re-run, a sticky error of it is returned instead of doing the work); the
 *    call synchronises before returning.
 *  - Scratch (GPU engine; owned by the set, only grows, freed by gk_destroy):
 *    the grouping scratch of gk_ingest_keyed, its grouped-batch buffers
 *    included (free once the leading gk_sync has settled an in-flight keyed
 *    ingest) -- the samples are grouped by id with their sample index as the
 *    payload -- plus the index payload itself and the selection scratch.  Per
 *    sample: 8 bytes of index payload + 8 bytes grouped + the pair buffers of
 *    gk_group_by_key (24 bytes for S > 65536, 16 for 256 < S <= 65536, 4 for
 *    S <= 256) + 0.25 byte of digit counts, 40.25 bytes at most; per set:
 *    8 (S+1) bytes of offsets, S/8 bytes of bitmap and 4 bytes per distinct
 *    occurring stream (at most 4 min(count, S)).  GK_E_NOMEM is returned
 *    before anything is mutated.
 *  - GK_RANKK_CHUNK=c (environment, read per call; tests) sets the number of
 *    grouped samples one wave of the GPU engine's kernel takes (default 1024):
 *    a multiple of 64, >= 64, anything else is GK_E_ARG.  The answers do not
 *    depend on it. */
int gk_ranks_keyed(gk_set* set, const int32_t* ids, const double* xs, int64_t count,
                   int64_t* lo, int64_t* hi, int64_t* n, void* stream);

/* Keyed score-and-ingest: rank each sample against the history of its stream,
 * then add it -- the scoring loop "s = score(batch); add(batch)" in one call.
 *  - Definition.  Exactly gk_ranks_keyed(set, ids, xs, count, lo, hi, n, stream)
 *    followed by gk_ingest_keyed(set, ids, xs, count, qs, nq, out, mode, stream):
 *    every sample is ranked against its stream's state BEFORE any value of this
 *    batch is added (the state after gk_ranks_keyed's flush of the occurring
 *    streams); then the batch is added, in arrival order per stream; then,
 *    nq > 0, quantiles(qs) of every stream as gk_ingest_quantiles answers them.
 *    lo / hi / n, out and the complete state of every stream -- table, pending
 *    values, n/_min/_max/_sum/_avg (GPU engine: capacity class and slot too) --
 *    are bit-identical to what the two calls give.  The samples are grouped by
 *    id ONCE, not once per half.
 *  - Memory and rows as gk_ranks_keyed (ids, xs, lo, hi, n) and gk_ingest_keyed
 *    (qs host, out float64[S*nq]).  Unlike gk_ranks_keyed, lo, hi and n may ALL
 *    be NULL: the call is then gk_ingest_keyed with the refusals below -- no
 *    rank is taken, so no stream is flushed ahead of the ingest.
 *  - Negative ids get the rows lo = hi = n = 0, are not ingested, and their
 *    xs[i] is not examined.
 *  - GK_E_ARG, from the call itself, before anything is mutated or written:
 *    count outside [0, 2^31-1]; a NULL `ids` or `xs` with count > 0; an id >= S;
 *    a NaN xs[i] on a row whose id is >= 0 (message and smallest offending
 *    index as gk_ranks_keyed; a sample with both faults is reported by its id);
 *    qs, nq, out and mode as gk_ingest_quantiles checks them; a bad
 *    GK_RANKK_CHUNK.  A NaN value therefore CANNOT be added through this call
 *    (gk_ingest_keyed adds it as the reference does): a rank of NaN has no
 *    meaning.  An id >= S is never the asynchronous error it is for
 *    gk_ingest_keyed.
 *  - count == 0 runs the argument checks and gk_sync and then is
 *    gk_ingest_keyed with count == 0 (nq > 0: exactly gk_quantiles).  S == 0:
 *    the rows are zero, nothing else happens.
 *  - GK_E_OVERFLOW of the rank half's flush: gk_ranks_keyed's rule -- no output
 *    is written and NOTHING is ingested; the stream that outgrew the last
 *    capacity class keeps its pre-call state, the other occurring streams have
 *    been flushed.  Errors of the ingest half are asynchronous, exactly as for
 *    gk_ingest_keyed (GK_E_OVERFLOW from a later call, at the latest gk_sync).
 *  - Synchronisation.  gk_sync first, as gk_ranks_keyed; the call then
 *    synchronises for the verdict of the sample check and for the flush.  After
 *    that the rank kernel and the ingest are only ENQUEUED and the call returns
 *    as gk_ingest does: lo / hi / n / out are ordered on `stream`, and the
 *    caller keeps ids, xs and the outputs alive and unchanged until the set's
 *    next call or gk_sync.  A stream the ingest defers is re-run from buffers
 *    the set owns, never from the caller's.
 *  - Scratch (GPU engine): exactly gk_ranks_keyed's, at most 40.25 bytes per
 *    sample and the same per-set part -- no second grouped-batch buffer: the
 *    8 bytes per sample of index payload, dead once the group-by has read
 *    them, take the grouped values the ingest reads, the 8 bytes "grouped" hold
 *    the grouped indices.  GK_E_NOMEM is returned before anything is mutated.
 *  - GK_RANKK_CHUNK is honoured as by gk_ranks_keyed; answers and states do
 *    not depend on it. */
int gk_rank_ingest_keyed(gk_set* set, const int32_t* ids, const double* xs, int64_t count,
                         int64_t* lo, int64_t* hi, int64_t* n,
                         const double* qs, int nq, double* out, int mode, void* stream);

/* GKArray.merge(other) (gk:111-154), stream by stream, as the left fold
 * dst.merge(srcs[0]); dst.merge(srcs[1]); ...  Like the reference it mutates
 * each source (flushes its pending values, gk:126, 137).  A source may be dst
 * itself (dst.merge(dst): dst is flushed, then merged with a snapshot of its
 * flushed state, as gk:137-154 do) and may repeat (flushed again at each of
 * its merges).  Returns GK_E_EPS_MISMATCH if any eps differs (gk:118-119) or
 * GK_E_ARG if the stream counts differ.  On GK_E_OVERFLOW (a merge outgrows
 * the last capacity class or the count limit; the fold stops at that source)
 * a stream that did not fit keeps its state from before that merge -- table,
 * pending values, n, _min, _max, _sum, _avg -- the other streams are complete
 * and the source has been flushed: gk_rollup's rule for a one-member group. */
int gk_merge(gk_set* dst, gk_set* const* srcs, int nsrcs, void* stream);

/* Group-by roll-up: GKArray.merge (gk:111-154) of groups of `src`'s streams
 * into the streams of `dst`, a DIFFERENT set with the same eps (stream counts
 * may differ: dst has G streams, src has S).  `group_offsets` (int64[G+1],
 * non-decreasing, starting at 0) and `members` (int64[group_offsets[G]],
 * indices into src) give the groups in CSR form; the arrays are device memory
 * for the GPU engine, host memory for the CPU engine.  For every destination
 * stream j, in order of k:
 *     for k in group_offsets[j] .. group_offsets[j+1]-1:
 *         dst[j].merge(src[members[k]])
 *  - dst keeps its state from before the call (a roll-up can be continued by
 *    a later call); pending values of dst join the first merge's incoming
 *    list (gk:71-72).  A destination with an empty group is not touched at
 *    all (not flushed).
 *  - Members are mutated as the reference mutates `other`: a member with
 *    n == 0 is left alone and the destination runs merge_compress()
 *    (gk:121-123); any other member is flushed unconditionally (gk:126 /
 *    gk:137) before it is converted, and spread uses its n (gk:136).  Source
 *    streams that are no member stay bit-identical.
 *  - _sum/_avg are not merged, except by the copy branch of a destination
 *    with n == 0 (gk:125-133), which may be taken mid-fold when the earlier
 *    members were all empty.
 *  - GK_E_ARG, before anything is mutated: dst == src, NULL arrays,
 *    group_offsets not starting at 0 or decreasing, a member outside [0, S),
 *    a source stream listed more than once (a repeated `other` would need a
 *    re-flush between its merges).  GK_E_EPS_MISMATCH if eps differs
 *    (gk:118-119).
 *  - GK_E_OVERFLOW, two cases.  A member whose own flush outgrows the last
 *    capacity class: that member keeps its state, the other members have been
 *    flushed, no destination is touched.  A destination that outgrows the
 *    last class or the count limit: every member has been flushed, such a
 *    destination holds the fold of the members before the one that did not
 *    fit (table, n, _min, _max consistent with each other), every other
 *    destination is complete.
 * Synchronises before returning, after settling earlier asynchronous work
 * (and errors) of both sets. */
int gk_rollup(gk_set* dst, gk_set* src, const int64_t* group_offsets,
              const int64_t* members, void* stream);

/* GKArray.merge_compress(entries) with an explicit entry list (gk:63-109,
 * gk:71): stream s merges extra records [eoffs[s], eoffs[s+1]) given as
 * (v, g, d) device arrays, each list sorted by v as the reference requires of
 * its Entry lists.  On GK_E_OVERFLOW a stream that did not fit keeps its
 * pre-call state (table, pending values, n, _min, _max, _sum, _avg) and the
 * other streams are complete. */
int gk_merge_compress(gk_set* set, const double* v, const int32_t* g,
                      const int32_t* d, const int64_t* eoffs, void* stream);

/* Table export (the reference's `entries`, gk:23): writes per-stream table
 * sizes to `sizes` (device int32[S]); then gk_export copies stream s's table
 * to v/g/d[offs[s] ..] where offs (device int64[S+1]) is the caller's
 * exclusive scan of those sizes.  Pending values (`incoming`, gk:24) go the
 * same way with gk_export_pending_sizes / gk_export_pending. */
int gk_export_sizes(gk_set* set, int32_t* sizes, void* stream);
int gk_export(gk_set* set, const int64_t* offs, double* v, int32_t* g,
              int32_t* d, void* stream);
int gk_export_pending_sizes(gk_set* set, int32_t* sizes, void* stream);
int gk_export_pending(gk_set* set, const int64_t* poffs, double* pv,
                      void* stream);

/* Import full per-stream state (checkpoint / RCCL payload): tables in CSR
 * (offs, v, g, d), pending values in CSR (poffs, pv) and the header arrays
 * (n, mn, mx, sum, avg), all device arrays of the set's S streams. */
int gk_import(gk_set* set, const int64_t* offs, const double* v,
              const int32_t* g, const int32_t* d, const int64_t* poffs,
              const double* pv, const int64_t* n, const double* mn,
              const double* mx, const double* sum, const double* avg,
              void* stream);

/* Versioned state files (format: sketches-py_amd/csrc/gk_format.h, "GKSTATE"
 * version 1: header with magic, version, eps, S, record totals and a
 * checksum; then sizes, pending counts, n/min/max/sum/avg, the tables and the
 * pending values).  The reference has no serialization: its state is the
 * Python object (gk:21-29 -- entries, incoming, _n, _min, _max, _sum, _avg),
 * and this is that state per stream, saved WITHOUT flushing, so a set loaded
 * from a file continues exactly like the saved one.
 * gk_save writes the set's state to `path`.  gk_peek reads eps and the stream
 * count from a file's header (to create a matching set).  gk_load replaces
 * the state of every stream of `set`, which must have the file's stream count
 * (GK_E_ARG) and eps (GK_E_EPS_MISMATCH).  GK_E_IO / GK_E_FORMAT on
 * unreadable, malformed, wrong-version or corrupt files. */
int gk_save(gk_set* set, const char* path, void* stream);
int gk_peek(const char* path, double* eps, int64_t* num_streams);
int gk_load(gk_set* set, const char* path, void* stream);

/* ---- row-shard exchange ----------------------------------
 * A set's whole state as one contiguous, self-describing "packed state"
 * buffer (layout: sketches-py_amd/csrc/gk_pack.h) that any transport moves as
 * bytes -- rcclAllGather / MPI_Allgather of device buffers, a socket, a file --
 * and the rank-ordered fold of such buffers: for every stream, the
 * reference's left fold sk0.merge(sk1).merge(sk2)... (gk:111-154; each merge
 * flushes `other` first, gk:126/137).  Buffers are device memory on the
 * set's GPU (host memory for the CPU engine).  All three calls synchronise.
 *
 * gk_pack_bytes: size of the set's packed state (read back from the device).
 * gk_pack:       writes it into `buf` (`bytes` >= gk_pack_bytes; trailing
 *                bytes untouched, so equal-sized padded buffers work for an
 *                all-gather).
 * gk_fold_packed: dst := bufs[0], then dst.merge(bufs[r]) for r = 1..n-1.
 *                Every buffer must hold dst's stream count and eps
 *                (GK_E_EPS_MISMATCH otherwise, as gk_merge).  The previous
 *                state of dst is replaced. */
int gk_pack_bytes(gk_set* set, int64_t* bytes, void* stream);
int gk_pack(gk_set* set, void* buf, int64_t bytes, void* stream);
/* Each bufs[r] must hold the whole packed state its header describes (the
 * header's byte count, as gk_pack_bytes returned it for the packing set):
 * headers and offset tables are checked for consistency, but the buffers'
 * own lengths are not known to this call. */
int gk_fold_packed(gk_set* dst, const void* const* bufs, int nbufs, void* stream);

/* ---- stream transfer: a LIST of streams to and from a packed state ----------
 * What the reference's user does with a dict of GKArray objects -- pickle
 * sketches[k] and hand it to another process, delete cold keys, add new ones
 * -- for the streams ids[0 .. count) of a set.  The carrier is the packed state
 * above (GKPACK01 version 1, sketches-py_amd/csrc/gk_pack.h), identical for
 * both engines.  Neither call flushes: after gk_pack_select -> any byte
 * transport -> gk_unpack_select the destination stream answers every later
 * call (ingest, flush, quantiles, ranks, merge, roll-up) with the bits the
 * source stream would have given, across sets, devices and the two engines.
 *  - Memory.  `ids` (int32) and `buf` are device memory for the GPU engine,
 *    host memory for the CPU engine.
 *  - Count and ids as gk_quantiles_select checks them: 0 <= count <= 2^31-1;
 *    an id outside [0, S), negative ids included, is GK_E_ARG, returned BEFORE
 *    anything is mutated or written, with the first bad index and its id in
 *    the message.
 *  - Synchronisation.  All three calls settle the set's earlier asynchronous
 *    work and errors first (gk_sync: deferred streams are re-run, a sticky
 *    error is returned instead of doing the work) and synchronise before
 *    returning.
 *
 * gk_pack_select_bytes: the size gk_pack_select needs for these ids.
 * gk_pack_select: writes a packed state whose header has S == count and whose
 *   stream k is the complete state of stream ids[k] -- table, pending values
 *   in insertion order, n/_min/_max/_sum/_avg -- exactly what gk_pack would
 *   write for a set made of those streams; gk_fold_packed of this one buffer
 *   into a set of `count` streams with the same eps therefore gives a set
 *   holding the listed streams.
 *    - No flush, no mutation: the set is bit-identical after the call (GPU
 *      engine: capacity class and slot too).
 *    - Ids may repeat and come in any order; row k always belongs to ids[k].
 *    - count == 0 is valid (`ids` may be NULL): a packed state of zero streams.
 *    - `bytes` below the needed size is GK_E_ARG with the needed size in the
 *      message; nothing beyond `bytes` is written and the buffer's contents
 *      are then unspecified.  Bytes past the packed size stay untouched, as
 *      with gk_pack.
 * gk_unpack_select: replaces the complete state of stream ids[k] with the
 *   buffer's stream k.  Refused BEFORE anything is mutated:
 *    - GK_E_ARG: an id outside [0, S); an id listed more than once (two rows
 *      for one stream); the header's S != count; a stream whose pending count
 *      p is not one add() can leave (p > n mod P, or n < 0: gk_import's rule);
 *    - GK_E_EPS_MISMATCH: the buffer's eps differs from the set's;
 *    - GK_E_FORMAT: bad magic, version or header size; inconsistent totals or
 *      byte count; offsets not monotone from 0 to the header's totals;
 *    - GK_E_OVERFLOW (GPU engine): a table with more entries than the last
 *      capacity class holds (a GK_CAPS ladder shorter than the packing set's).
 *   Table contents (order of v, values of g and delta) are not checked, as
 *   gk_import does not check them; the buffer's own length is not known, as
 *   for gk_fold_packed.  count == 0: the buffer is still validated (its S
 *   must be 0) and nothing is touched.
 *    - Unlisted streams stay bit-identical, including class and slot.
 *    - Capacity class (GPU engine).  A listed stream whose new table fits its
 *      class keeps class and slot; it is never demoted (gk_reset_select's
 *      reasons; gk_compact is the call that demotes); one whose table does not fit moves up to the first class
 *      that holds it, and gk_num_promoted may rise.
 *    - GK_E_NOMEM while growing a class arena is returned before the first
 *      write: every listed stream then holds its complete old state.  At any
 *      point a stream holds either its complete old or its complete new
 *      state, never header words of one and the table of the other.
 *  - Scratch (GPU engine; the selection scratch, owned by the set, only grows,
 *    freed by gk_destroy).  gk_pack_select*: 32 bytes + 8 bytes per 2048
 *    listed ids (the scan's tile sums).  gk_unpack_select: 32 bytes + S/8
 *    bytes + 4 bytes per listed id (at most 4 S). */
int gk_pack_select_bytes(gk_set* set, const int32_t* ids, int64_t count, int64_t* bytes, void* stream);
int gk_pack_select(gk_set* set, const int32_t* ids, int64_t count, void* buf, int64_t bytes, void* stream);
int gk_unpack_select(gk_set* set, const int32_t* ids, int64_t count, const void* buf, void* stream);

/* ---- compaction: streams back into the smallest capacity class that holds them --
 * What the reference's user gets for free when a key is dropped and its
 * GKArray collected: the memory.  On the GPU engine classes only grow (an
 * ingest, gk_unpack_select, a merge move a stream up; gk_reset_select and
 * gk_unpack_select never move one down), so a set that churns streams -- a
 * KeyedStreamSet whose removed keys' ids are recycled -- ratchets its promoted
 * population, its member lists and its arenas upwards.  gk_compact re-places
 * every stream; gk_class_usage shows what a set holds per class.  Nothing calls
 * gk_compact implicitly: when to compact is the caller's decision.
 *
 * gk_compact
 *  - Synchronisation.  gk_sync first (deferred streams of the previous call are
 *    re-run, a sticky error of it is returned instead of doing the work: nothing
 *    is compacted then, and the outputs are not written); the call synchronises
 *    before returning.
 *  - Placement.  A stream whose table has E entries fits class t when
 *    E <= capacity(t) - 1 (gk_unpack_select's rule).  With fit(E) the smallest
 *    such class, the stream's class after the call is min(old class, fit(E)):
 *    compaction never promotes.  Pending values live beside the tables and
 *    play no part.
 *  - State.  Every stream's table, pending values in insertion order and
 *    n/_min/_max/_sum/_avg are bit-identical before and after, and every later
 *    call (ingest, flush, quantiles, ranks, merge, roll-up, pack) answers with
 *    the bits it would have given without the compaction.  Only class, slot,
 *    member lists and arena sizes change.
 *  - Bookkeeping (GPU engine).  Afterwards the member list of every class c > 0
 *    holds exactly the streams of class c, each once, in unspecified order; the
 *    slots of those streams are a permutation of [0, slots_used) and slots_used
 *    equals their number; and an ingest into a set with no promoted stream
 *    takes the path of a fresh set again.
 *  - Arenas.  Class c > 0 keeps min(slots_alloc, min(S, max(the slots a new set
 *    starts the class with, 2 * slots_used))) slots -- twice what is in use, so
 *    that the next call does not regrow an arena no stream has entered -- or
 *    slots_used if the streams that came down into c need more than that.  A
 *    class left at 0 slots (the classes beyond 32768 entries, which a new set
 *    allocates on first use) returns its arena AND its workspace: it is the
 *    not-yet-used class of gk_create again.  A class that keeps slots keeps its
 *    workspace: the device moves streams into such a class in the middle of a
 *    call, with no host step that could allocate one.  A class in which nothing
 *    changes (no stream leaves or enters, slots dense, size at target) is not
 *    copied.
 *  - *demoted (may be NULL): streams whose class dropped.  *bytes_freed (may be
 *    NULL): arena plus workspace bytes before the call minus those after it,
 *    >= 0 unless arrivals made an arena grow; exactly what summing
 *    gk_class_usage over the classes before and after gives.
 *  - GK_E_NOMEM.  HIP has no realloc: a class's new arena is allocated beside
 *    the old ones.  The work goes by destination class ascending and the old
 *    arena of a class is freed as soon as that class is done, so the peak
 *    extra memory is ONE new arena (at most the size of the old one of that
 *    class, or of its arrivals).  On failure the classes below the failing one
 *    are compacted, the others are as before; every stream holds its complete
 *    state bit for bit -- header and table of one placement, never of two --
 *    and the set stays fully usable.  *demoted then counts the streams the plan
 *    found, moved or not.
 *  - S == 0 and a set with nothing promoted return GK_OK with *demoted =
 *    *bytes_freed = 0 and touch nothing; so does a second gk_compact straight
 *    after one.
 *  - Scratch (GPU engine; the selection scratch, owned by the set, only grows,
 *    freed by gk_destroy): 64 bytes of counters.  Its GK_E_NOMEM is returned
 *    before anything is mutated.
 *  - Host engine: one unbounded class, nothing to demote; the call returns the
 *    unused capacity of every stream's table and pending vectors
 *    (shrink_to_fit).  *demoted = 0, *bytes_freed = capacity bytes before minus
 *    after.
 *
 * gk_class_usage: one capacity class of the set, after settling the set as
 *   gk_num_promoted does (deferred streams are placed first; a sticky error is
 *   left for the next call that reports one).  cls outside [0, number of
 *   classes) is GK_E_ARG (the host engine has class 0 only); any output
 *   pointer may be NULL.  *streams: the streams whose class is cls -- summed
 *   over the classes S, over cls > 0 gk_num_promoted.  *slots_used,
 *   *slots_alloc: slots handed out and allocated in the class's arena (class
 *   0: both S).  *arena_bytes = slots_alloc * capacity * 16 (host engine: the
 *   summed capacities of the streams' table and pending vectors in bytes).
 *   *workspace_bytes: the class's global workspace, 0 when it has none. */
int gk_compact(gk_set* set, int64_t* demoted, int64_t* bytes_freed, void* stream);
int gk_class_usage(gk_set* set, int cls, int64_t* streams, int64_t* slots_used,
                   int64_t* slots_alloc, int64_t* arena_bytes, int64_t* workspace_bytes,
                   void* stream);

/* ---- key directory: int64 keys to stream ids, assigned by the engine ---------
 * The dict of the reference's user (sketches[key] = GKArray(eps) on a key
 * not seen before): a persistent table from int64 keys to int32 ids that
 * looks up or inserts a whole batch of sample keys in one call.  Its ids are
 * what gk_ingest_keyed, the gk_*_select calls, gk_pack_select and roll-up
 * member lists take.  A directory is an object of its own, not part of a
 * set: one directory may serve several sets.  Keys can be removed
 * (gk_dir_remove); the ids they held are handed out again, smallest first.
 *  - State.  Besides its keys a directory holds `bound`, one past the
 *    largest id handed out since the last import (gk_dir_bound), and `free`,
 *    the ids below `bound` that no key holds.  len(d) (gk_dir_size) is the
 *    number of keys held; always len(d) + |free| == bound <= capacity.  With
 *    no removal `free` is empty and bound == len(d).  The id space only
 *    shrinks by gk_dir_keys -> filter -> gk_dir_import.
 *  - Memory.  `keys` (int64), `out_ids` (int32) and `out_keys` (int64) are
 *    device memory on the directory's GPU for the GPU engine, host memory
 *    for the CPU engine.  `num_new` is host memory.
 *  - Count.  0 <= count <= 2^31-1, anything else is GK_E_ARG.  count == 0 is
 *    valid with NULL arrays; a NULL array with count > 0 is GK_E_ARG.
 *  - GK_DIR_NONE is "no key": it is never stored and always answers id -1,
 *    gk_ingest_keyed's "not for this set".  Every other int64 value is a key.
 *  - Synchronisation.  gk_dir_assign, gk_dir_remove, gk_dir_lookup,
 *    gk_dir_keys, gk_dir_import and gk_dir_import_sparse synchronise before
 *    returning.  A directory is not
 *    thread-safe; its calls must be ordered on one stream.
 *
 * gk_dir_create: an empty directory of at most `capacity` keys, 1 <= capacity
 *   <= 2^30 (GK_E_ARG otherwise), on HIP device `device`.
 * gk_dir_assign is this loop over the directory d:
 *       for i in 0 .. count-1:
 *           k = keys[i]
 *           if k == GK_DIR_NONE:   out_ids[i] = -1
 *           elif k in d:           out_ids[i] = d[k]
 *           elif free:             d[k] = min(free); free.remove(d[k]); out_ids[i] = d[k]
 *           else:                  d[k] = bound; bound += 1; out_ids[i] = d[k]
 *   The r-th new key of the batch, in order of FIRST OCCURRENCE, gets the
 *   r-th smallest id that was free when the call began and, once those run
 *   out, bound, bound + 1, ...: every output is a function of the directory's
 *   contents and the batch alone -- not of which gk_dir_remove freed an id or
 *   in what order, nor of the hash, the probe order or the scheduling of the
 *   device's threads -- and the two engines give identical ids.  A removed
 *   key that comes back is a new key: it takes the smallest free id, which
 *   need not be its old one.  *num_new (may be NULL) receives the number of
 *   keys added.  GK_E_OVERFLOW exactly when len(d) + new keys > capacity: the
 *   call is then void and the directory exactly as before it (gk_dir_size,
 *   gk_dir_bound, the free ids, gk_dir_keys and every later answer are as if
 *   it had not happened); out_ids is unspecified and *num_new is not written.
 * gk_dir_remove is this loop:
 *       for i in 0 .. count-1:
 *           k = keys[i]
 *           if k == GK_DIR_NONE or k not in d:  out_ids[i] = -1
 *           else:  out_ids[i] = d.pop(k); free.add(out_ids[i])
 *   A key listed twice is removed by its first occurrence; the later ones
 *   answer -1.  *num_removed (may be NULL) receives the number of keys
 *   removed.  "Not found" is an answer, never an error.  out_ids is required
 *   when count > 0.  The directory does not touch any set: the caller must
 *   reset the stream of a removed id (gk_reset_select) before a new key
 *   inherits it.
 * gk_dir_lookup: read-only; out_ids[i] = d[keys[i]], or -1 for a key the
 *   directory does not hold and for GK_DIR_NONE.
 * gk_dir_bound: one past the largest id handed out; -1 for NULL.
 * gk_dir_keys: the inverse array, out_keys[id] = the key that holds id, or
 *   GK_DIR_NONE for a free id, for id in [0, gk_dir_bound); out_keys may be
 *   NULL while gk_dir_bound is 0.
 * gk_dir_import: replaces the contents with keys[i] -> i, i in [0, count)
 *   (restore, a copy of another capacity, a compacted id space); afterwards
 *   bound == size == count and no id is free.  GK_E_ARG for
 *   count > capacity, for a GK_DIR_NONE entry (its first index in the
 *   message) and for a key listed twice (the first index that repeats an
 *   earlier entry, and the key, in the message): refused BEFORE anything is
 *   mutated -- the new contents are built in a second table that replaces the
 *   first on success.
 * gk_dir_import_sparse: gk_dir_import, except that a GK_DIR_NONE entry is a
 *   free id: keys[i] -> i for the other entries and bound = count (what
 *   gk_dir_keys wrote for a directory with free ids; restore and copies of
 *   such a directory).  The other two refusals are gk_dir_import's.
 *  - Memory (per capacity).  The table has T slots, T the power of two >=
 *    2 * capacity and at least 64; a slot holds an 8-byte key, a 4-byte id and
 *    a 4-byte first-occurrence word (16 T bytes); the inverse array adds 8
 *    bytes per id of `capacity` and the list of free ids 4 bytes per id of
 *    `capacity`.  A removed key keeps its slot until the table is rebuilt
 *    from the inverse array, which gk_dir_remove does once removals since
 *    the last rebuild pass T/4 slots (on the stream, no second table).  The
 *    imports hold two tables while they run.  GK_E_NOMEM is returned before
 *    anything is mutated.
 *  - Scratch (GPU engine; owned by the directory, only grows, freed by
 *    gk_dir_destroy).  gk_dir_assign, gk_dir_remove and the imports: 8 bytes
 *    per sample (the sample's slot and its first-occurrence flag, scanned in
 *    place into its rank) + 8 bytes per 2048 samples (the scan's tile sums),
 *    sized for max(count, gk_dir_bound) samples so that a void call can
 *    always rebuild the table and a remove the list of free ids.
 *    gk_dir_lookup and gk_dir_keys need none.
 *  - GK_DIR_HASH_BITS=b (environment, read by gk_dir_create; tests) confines
 *    the keys' home slots to the last 2^b slots of the table: b = 0 makes the
 *    table one probe chain that wraps round its end.  Not a number >= 0:
 *    GK_E_ARG.  The hash itself is not part of the ABI. */
typedef struct gk_dir gk_dir;
#define GK_DIR_NONE INT64_MIN
int gk_dir_create(int64_t capacity, int device, gk_dir** out);
int gk_dir_destroy(gk_dir* dir);
int64_t gk_dir_capacity(const gk_dir* dir);
int64_t gk_dir_size(const gk_dir* dir);  /* keys held */
int64_t gk_dir_bound(const gk_dir* dir); /* one past the largest id handed out */
int gk_dir_assign(gk_dir* dir, const int64_t* keys, int64_t count, int32_t* out_ids, int64_t* num_new,
                  void* stream);
int gk_dir_remove(gk_dir* dir, const int64_t* keys, int64_t count, int32_t* out_ids, int64_t* num_removed,
                  void* stream);
int gk_dir_lookup(gk_dir* dir, const int64_t* keys, int64_t count, int32_t* out_ids, void* stream);
int gk_dir_keys(gk_dir* dir, int64_t* out_keys, void* stream);
int gk_dir_import(gk_dir* dir, const int64_t* keys, int64_t count, void* stream);
int gk_dir_import_sparse(gk_dir* dir, const int64_t* keys, int64_t count, void* stream);

/* Introspection for tests and benchmarks. */
int64_t gk_num_streams(const gk_set* set);
double gk_eps(const gk_set* set);
int gk_flush_period(const gk_set* set);       /* int(1.0/eps) + 1 (gk:60)  */
int gk_capacity(const gk_set* set, int cls);  /* table capacity of a class */
int64_t gk_num_promoted(const gk_set* set);   /* streams in the large class */

/* Kernel timing: `on` bit 0 -- gk_ingest records HIP events around the
 * flush kernel it launches on `stream`; bit 1 -- also around the call's
 * stats fork (stats_ms; two more event markers per call).  gk_timing_read
 * returns the summed milliseconds and the number of launches since the last
 * read. */
int gk_timing_enable(gk_set* set, int on);
int gk_timing_read(gk_set* set, double* flush_ms, double* stats_ms,
                   int64_t* launches);

#ifdef __cplusplus
}
#endif

#endif /* GK_CAPI_H */
