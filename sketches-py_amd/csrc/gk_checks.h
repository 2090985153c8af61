// gk_checks.h -- the error slot of gk_last_error() and the argument checks
// whose condition and message are the same in both engines (gk_capi.cpp on
// the device, ../cpu/gk_cpu.cpp on the host): one source, so that the two
// engines' error contract cannot drift.  A check whose text or condition
// differs between the engines (id and member ranges, out_values, ...) stays
// in its engine.  Included once per library (everything here is file-local).
#pragma once

#include <cmath>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <string>

#include "gk_capi.h"

namespace {

thread_local std::string g_err;

int fail(int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  g_err = buf;
  return code;
}

int check_set(const gk_set* h) {
  if (!h) return fail(GK_E_ARG, "null set");
  return GK_OK;
}

// quantile arguments (gk_quantiles, gk_ingest_quantiles, gk_ingest_keyed, gk_quantiles_select)
int check_query_args(const double* qs, int nq, const double* out, int mode) {
  if (nq < 0 || (nq > 0 && (!qs || !out))) return fail(GK_E_ARG, "bad quantile arguments");
  if (mode != GK_Q_LIST && mode != GK_Q_SINGLE) return fail(GK_E_ARG, "bad mode %d", mode);
  for (int i = 0; i < nq; ++i)
    if (std::isnan(qs[i])) return fail(GK_E_ARG, "cannot convert float NaN to integer");
  return GK_OK;
}

// rank arguments (gk_ranks, gk_ranks_select)
int check_rank_args(const double* xs, int nx, const int64_t* lo, const int64_t* hi) {
  if (nx < 0 || (nx > 0 && (!xs || (!lo && !hi)))) return fail(GK_E_ARG, "bad rank arguments");
  for (int i = 0; i < nx; ++i)
    if (std::isnan(xs[i])) return fail(GK_E_ARG, "xs[%d] is NaN", i);
  return GK_OK;
}

// sample / id count of the keyed and selection calls
int check_count(int64_t count) {
  if (count < 0 || count > INT32_MAX) return fail(GK_E_ARG, "count %lld outside [0, 2^31-1]", (long long)count);
  return GK_OK;
}

// id list of the selection calls (the ids' range is checked by each engine)
int check_select_args(const int32_t* ids, int64_t count) {
  int rc = check_count(count);
  if (rc) return rc;
  if (count > 0 && !ids) return fail(GK_E_ARG, "ids is null");
  return GK_OK;
}

// keyed rank arguments (gk_ranks_keyed), ahead of the per-sample checks
int check_rank_keyed_args(const int32_t* ids, const double* xs, int64_t count, const int64_t* lo, const int64_t* hi,
                          const int64_t* n) {
  int rc = check_count(count);
  if (rc) return rc;
  if (count > 0 && (!ids || !xs)) return fail(GK_E_ARG, "ids or xs is null");
  if (!lo && !hi && !n) return fail(GK_E_ARG, "lo, hi and n are all null");
  return GK_OK;
}

// gk_rank_ingest_keyed: the same, but lo, hi and n may all be NULL
int check_rank_ingest_keyed_args(const int32_t* ids, const double* xs, int64_t count) {
  int rc = check_count(count);
  if (rc) return rc;
  if (count > 0 && (!ids || !xs)) return fail(GK_E_ARG, "ids or xs is null");
  return GK_OK;
}

// the first offending sample of gk_ranks_keyed: its id if that is >= S, else its NaN
int fail_rank_keyed_sample(int64_t index, int32_t id, int64_t S) {
  if (id >= S)
    return fail(GK_E_ARG, "ids[%lld] = %d lies outside [0, %lld) (negative ids are skipped)", (long long)index, id,
                (long long)S);
  return fail(GK_E_ARG, "xs[%lld] is NaN (ids[%lld] = %d)", (long long)index, (long long)index, id);
}

// gk_merge: the source list, and every source's eps and stream count against dst's
template <typename Set>
int check_merge_args(const Set* dst, Set* const* srcs, int nsrcs) {
  int rc = check_set(dst);
  if (rc) return rc;
  if (nsrcs < 0 || (nsrcs > 0 && !srcs)) return fail(GK_E_ARG, "bad source list");
  for (int k = 0; k < nsrcs; ++k) {
    if (!srcs[k]) return fail(GK_E_ARG, "null source %d", k);
    if (srcs[k]->eps != dst->eps)  // gk:118-119
      return fail(GK_E_EPS_MISMATCH, "Cannot merge two GKArrays with different epsilon values");
    if (srcs[k]->S != dst->S)
      return fail(GK_E_ARG, "stream counts differ (%lld vs %lld)", (long long)srcs[k]->S, (long long)dst->S);
  }
  return GK_OK;
}

// gk_rollup, ahead of the offsets' and members' own checks
template <typename Set>
int check_rollup_args(const Set* dst, const Set* src, const int64_t* group_offsets) {
  int rc = check_set(dst);
  if (!rc) rc = check_set(src);
  if (rc) return rc;
  if (dst == src) return fail(GK_E_ARG, "roll-up of a set into itself");
  if (!group_offsets) return fail(GK_E_ARG, "group_offsets is null");
  if (src->eps != dst->eps)  // gk:118-119
    return fail(GK_E_EPS_MISMATCH, "Cannot merge two GKArrays with different epsilon values");
  return GK_OK;
}

// gk_merge_compress
int check_record_args(const double* v, const int32_t* g, const int32_t* d, const int64_t* eoffs) {
  if (!eoffs || !v || !g || !d) return fail(GK_E_ARG, "null record arrays");
  return GK_OK;
}

// ---- key directory (gk_dir_*) ----
int check_dir(const gk_dir* d) {
  if (!d) return fail(GK_E_ARG, "null directory");
  return GK_OK;
}

int check_dir_create(int64_t capacity, gk_dir** out) {
  if (!out) return fail(GK_E_ARG, "out is null");
  *out = nullptr;
  if (capacity < 1 || capacity > ((int64_t)1 << 30))
    return fail(GK_E_ARG, "capacity %lld outside [1, 2^30]", (long long)capacity);
  return GK_OK;
}

// gk_dir_assign / gk_dir_lookup (out_ids wanted) and gk_dir_import
int check_dir_args(const gk_dir* d, const int64_t* keys, int64_t count, const int32_t* out_ids, bool want_out) {
  int rc = check_dir(d);
  if (!rc) rc = check_count(count);
  if (rc) return rc;
  if (count > 0 && !keys) return fail(GK_E_ARG, "keys is null");
  if (count > 0 && want_out && !out_ids) return fail(GK_E_ARG, "out_ids is null");
  return GK_OK;
}

int fail_dir_overflow(int64_t capacity, int64_t size) {
  return fail(GK_E_OVERFLOW, "the batch's new keys do not fit the directory (capacity %lld, %lld assigned): call void",
              (long long)capacity, (long long)size);
}

int fail_dir_import_count(int64_t count, int64_t capacity) {
  return fail(GK_E_ARG, "import of %lld keys into a directory of capacity %lld", (long long)count, (long long)capacity);
}

int fail_dir_import_none(int64_t index) {
  return fail(GK_E_ARG, "keys[%lld] is GK_DIR_NONE", (long long)index);
}

int fail_dir_import_repeat(int64_t index, int64_t key) {
  return fail(GK_E_ARG, "keys[%lld] repeats key %lld", (long long)index, (long long)key);
}

}  // namespace
