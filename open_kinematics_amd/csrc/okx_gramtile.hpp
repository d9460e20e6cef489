// okx_gramtile.hpp — what the two passes that sum outer products over the geometries in 64-wide tiles share (okx_covariance.hip:
// sum d d^T; okx_surface.hip: Phi^T Phi and Phi^T D): the walk over the lower triangle's tile pairs, the slab length of the launch
// plan and the host check of an entry list.  The tile kernels themselves stay in their units: okx_cov_gram is held to its
// instruction text (tools/kernel_text_digest.py), and okx_surf_tile stages a second operand.
#pragma once

#include <stdint.h>

#include <algorithm>
#include <utility>
#include <vector>

#include "../../include/okx.h"
#include "okx_program.hpp"

namespace okx {
namespace gramtile {

// Geometries per slab for `items` work items (tile pairs, tiles) per slab: enough slabs for want_groups workgroups, a multiple
// of the staged panel (`block` geometries), none shorter than min_slab - from the sizes alone.
inline long long slab_length(long long n_geom, long long items, long long want_groups, int block, long long min_slab) {
  long long want = want_groups / (items > 0 ? items : 1);
  if (want < 1) want = 1;
  long long len = (n_geom + want - 1) / want;
  len = (len + block - 1) / block * block;
  return len < min_slab ? min_slab : len;
}

// A HOST copy of an entry list [n_entries] (or null: all n_table_entries in natural order) for the pass `who` that takes 1 to
// `limit` entries: the count, every index inside [0, n_table_entries), and the first position that repeats an earlier one.
inline int check_entry_list(const char* who, const int32_t* entries, int32_t n_entries, int64_t n_table_entries, int limit) {
  if (n_entries < 1 || n_entries > limit)
    return fail(OKX_ERR_INVALID, "%s: %lld entries selected, 1 to %d allowed", who, (long long)n_entries, limit);
  if (!entries) {
    if (n_entries != n_table_entries)
      return fail(OKX_ERR_INVALID, "%s: without an entry list all %lld entries are selected, not %lld", who, (long long)n_table_entries, (long long)n_entries);
    return OKX_OK;
  }
  for (int32_t i = 0; i < n_entries; ++i)
    if (entries[i] < 0 || entries[i] >= n_table_entries)
      return fail(OKX_ERR_INVALID, "%s: entry %lld is %lld, outside [0, %lld)", who, (long long)i, (long long)entries[i], (long long)n_table_entries);
  // the first position that repeats an earlier one
  std::vector<std::pair<int32_t, int32_t>> order((size_t)n_entries);
  for (int32_t i = 0; i < n_entries; ++i) order[(size_t)i] = {entries[i], i};
  std::sort(order.begin(), order.end());
  int32_t at = -1, before = -1;
  for (size_t i = 1; i < order.size(); ++i)
    if (order[i].first == order[i - 1].first && (at < 0 || order[i].second < at)) {
      at = order[i].second;
      size_t j = i;
      while (j > 0 && order[j - 1].first == order[i].first) --j;
      before = order[j].second;
    }
  if (at >= 0)
    return fail(OKX_ERR_INVALID, "%s: entry %lld repeats entry %lld (index %lld)", who, (long long)at, (long long)before, (long long)entries[at]);
  return OKX_OK;
}

#if defined(__HIPCC__)

// pair p of the lower triangle, row by row: (0,0) (1,0) (1,1) (2,0) ...
__device__ inline void pair_of(long long p, int* ti, int* tj) {
  int i = 0;
  while ((long long)(i + 1) * (i + 2) / 2 <= p) ++i;
  *ti = i;
  *tj = (int)(p - (long long)i * (i + 1) / 2);
}

#endif  // __HIPCC__

}  // namespace gramtile
}  // namespace okx
