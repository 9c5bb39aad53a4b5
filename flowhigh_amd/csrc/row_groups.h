// Rows in groups, a scalar per group (include/flowhigh_hip.h: fh_row_groups): how a kernel body that serves a one-time entry
// and a grouped entry finds the scalar of a row.  The clips of a ragged sequence are sorted by step count, so the clips of one
// count are one contiguous range of rows, a group.  The groups and every per-group scalar travel BY VALUE as kernel arguments:
// no device table, no upload, no sync, and a captured graph holds them.  A wave works on one row: it finds the row's group by
// scalar compares against the row ends and selects its scalar by scalar selects (no dynamic index into the argument block,
// which would go through scratch).
#pragma once
#include "fh_common.h"

namespace {

struct GroupVals {
  float v[FH_MAX_GROUPS];
};

// group of a wave-uniform row: the number of row ends at or below it (the last end is the row count: not compared)
__device__ __forceinline__ int group_of(const fh_row_groups& g, int row) {
  int k = 0;
#pragma unroll
  for (int i = 0; i < FH_MAX_GROUPS - 1; ++i) k += (i < g.n - 1 && row >= g.row_end[i]) ? 1 : 0;
  return k;
}

__device__ __forceinline__ float pick(const GroupVals& s, int k) {
  float r = s.v[0];
#pragma unroll
  for (int i = 1; i < FH_MAX_GROUPS; ++i) r = k == i ? s.v[i] : r;
  return r;
}

// the row of this wave, in an SGPR (threadIdx.x >> 6 is uniform in a wave, which the compiler cannot see)
__device__ __forceinline__ int wave_row() { return uni((int)(blockIdx.x * 4 + (threadIdx.x >> 6))); }

// The two selectors a templated body takes.  OneGroup: one scalar for all rows, which is group 0 at compile time, so the
// one-time entry's kernel carries no compare and no select.  RowGroups: the row's group's scalar.
struct OneGroup {
  __device__ __forceinline__ int row() const { return (int)(blockIdx.x * 4 + (threadIdx.x >> 6)); }
  __device__ __forceinline__ int group(int) const { return 0; }
};

struct RowGroups {
  fh_row_groups g;
  __device__ __forceinline__ int row() const { return wave_row(); }
  __device__ __forceinline__ int group(int row) const { return group_of(g, row); }
};

bool groups_ok(const fh_row_groups* g) {
  if (!g || g->n < 1 || g->n > FH_MAX_GROUPS) return false;
  int prev = 0;
  for (int i = 0; i < g->n; ++i) {
    if (g->row_end[i] <= prev) return false;
    prev = g->row_end[i];
  }
  return true;
}

// the groups as a kernel argument: the entries behind n filled with the last end (never compared)
fh_row_groups groups_arg(const fh_row_groups* g) {
  fh_row_groups a;
  a.n = g->n;
  for (int i = 0; i < FH_MAX_GROUPS; ++i) a.row_end[i] = g->row_end[i < g->n ? i : g->n - 1];
  return a;
}

GroupVals vals_arg(const float* v, int n) {
  GroupVals a;
  for (int i = 0; i < FH_MAX_GROUPS; ++i) a.v[i] = v[i < n ? i : n - 1];
  return a;
}

}  // namespace

#define FH_CHECK_GROUPS(entry, g, rows)                                                                                    \
  do {                                                                                                                     \
    FH_CHECK_ARG((g) != nullptr, entry ": the groups must be given");                                                      \
    FH_CHECK_ARG((g)->n >= 1 && (g)->n <= FH_MAX_GROUPS, entry ": %d groups (1..%d)", (g)->n, FH_MAX_GROUPS);              \
    FH_CHECK_ARG(groups_ok(g), entry ": the groups' row ends must be positive and strictly increasing");                   \
    FH_CHECK_ARG((g)->row_end[(g)->n - 1] == (rows), entry ": the last group ends at row %d, the call has %d rows",       \
                 (g)->row_end[(g)->n - 1], (rows));                                                                        \
  } while (0)
