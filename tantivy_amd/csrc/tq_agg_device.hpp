// tq_agg_device.hpp — the device helpers the kernels over a doc set and a fast-field column share (tq_sort.hip, tq_agg.hip,
// tq_agg_sub.hip, tq_agg_terms.hip, tq_agg_terms_sub.hip, tq_agg_range.hip, tq_agg_terms_hist.hip), all in this one header:
//   col_value / col_key_index   a row's value, and its key index (value - min) / gcd, by the column's codec
//   wave_sum64 / add128         a wavefront's sum; the 128-bit atomic add
//   AggStatsLane, agg_stats_*   the top-level 64-byte stats record: per lane, per wavefront, per workgroup, published
//   BucketTable                 the workgroup's LDS table of 40-byte bucket records, and the same update on global memory
//   bucket_records_init         a row of bucket records: zeros with min_value = ~0
// Integer atomics only: whatever order the adders come in, the result is the same.  Internal linkage, like
// tq_docset_word.hpp: every kernel file gets its own copy.
#pragma once
#include "tq_agg_value.hpp"
#include "tq_column_read.hpp"
#include "tq_common.hpp"
#include "tq_docset_walk.hpp"
#include "tq_launch.h"

namespace {

// the value of `row`: min + gcd * packed; Linear holds the value itself
__device__ __forceinline__ uint64_t col_value(const TqkColumn &col, uint64_t min_value, uint64_t gcd, uint32_t row) {
  const uint32_t codec = col.codec;  // (uniform)
  if (codec == TQK_COL_LINEAR) return rg_value<TQK_COL_LINEAR>(col, row);
  const uint64_t n = codec == TQK_COL_BITPACKED ? rg_value<TQK_COL_BITPACKED>(col, row) : rg_value<TQK_COL_BLOCKWISE>(col, row);
  return min_value + gcd * n;
}

// (value - min) / gcd of `row`: what the packed codecs store; Linear: computed (a value below min wraps to a huge index)
__device__ __forceinline__ uint64_t col_key_index(const TqkColumn &col, uint64_t min_value, uint64_t gcd, uint32_t row) {
  const uint32_t codec = col.codec;  // (uniform)
  if (codec == TQK_COL_LINEAR) {
    const uint64_t idx = rg_value<TQK_COL_LINEAR>(col, row) - min_value;
    return gcd > 1ull ? idx / gcd : idx;  // (uniform)
  }
  return codec == TQK_COL_BITPACKED ? rg_value<TQK_COL_BITPACKED>(col, row) : rg_value<TQK_COL_BLOCKWISE>(col, row);
}

__device__ __forceinline__ unsigned long long wave_sum64(unsigned long long v) {
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  return v;
}

// *sum_lo / *sum_hi (128 bits) += lo + hi * 2^32 (lo, hi < 2^63), low word first: a wrapped add carries into the high word;
// the number of wraps does not depend on the order of the adders
__device__ __forceinline__ void add128(unsigned long long *sum_lo, unsigned long long *sum_hi, unsigned long long lo,
                                       unsigned long long hi) {
  const unsigned long long add_lo = lo + (hi << 32);
  const unsigned long long add_hi = (hi >> 32) + (add_lo < lo ? 1ull : 0ull);
  const unsigned long long old = atomicAdd(sum_lo, add_lo);
  const unsigned long long carry = old + add_lo < old ? 1ull : 0ull;
  if (add_hi + carry) atomicAdd(sum_hi, add_hi + carry);
}

// ---- the top-level stats record (TqkAggStats).  A lane's share: count, min and max of the u64-space values and their sum
// as TWO accumulators of the values' 32-bit halves (a segment has fewer than 2^31 docs: neither can overflow, no carries in
// the walk); the histogram's in-bounds and out-of-range docs.
struct AggStatsLane {
  uint32_t valued = 0, inb = 0, oor = 0;
  uint64_t mn = ~0ull, mx = 0ull, s_lo = 0ull, s_hi = 0ull;
  __device__ __forceinline__ void add(uint64_t v) {
    ++valued;
    mn = v < mn ? v : mn;
    mx = v > mx ? v : mx;
    s_lo += v & 0xFFFFFFFFull;
    s_hi += v >> 32;
  }
};
constexpr uint32_t AGG_STATS_PART = 8;  // words of a wavefront's part; a kernel's own two counts may go behind them

// the wavefront's part: shuffles reduce the lanes (cnt: docset_walk's return), lane 0 writes words [0, AGG_STATS_PART) and,
// where the part has room for them, the sums of the kernel's own two per-lane counts
template <uint32_t N>
__device__ __forceinline__ void agg_stats_wave_part(unsigned long long (&part)[N], uint32_t cnt, AggStatsLane a, int lane,
                                                    uint32_t own0 = 0, uint32_t own1 = 0) {
  static_assert(N == AGG_STATS_PART || N == AGG_STATS_PART + 2, "the shared words, with or without the kernel's two");
  const unsigned long long t_cnt = wave_sum64(cnt), t_val = wave_sum64(a.valued), t_lo = wave_sum64(a.s_lo), t_hi = wave_sum64(a.s_hi);
  const unsigned long long t_inb = wave_sum64(a.inb), t_oor = wave_sum64(a.oor);
  const unsigned long long t_own0 = wave_sum64(own0), t_own1 = wave_sum64(own1);
  for (int off = 32; off > 0; off >>= 1) {
    const uint64_t x = __shfl_down(a.mn, off, 64), y = __shfl_down(a.mx, off, 64);
    a.mn = x < a.mn ? x : a.mn;
    a.mx = y > a.mx ? y : a.mx;
  }
  if (lane == 0) {
    part[0] = t_cnt;
    part[1] = t_val;
    part[2] = a.mn;
    part[3] = a.mx;
    part[4] = t_lo;
    part[5] = t_hi;
    part[6] = t_inb;
    part[7] = t_oor;
    if (N > AGG_STATS_PART) {
      part[AGG_STATS_PART] = t_own0;
      part[AGG_STATS_PART + 1] = t_own1;
    }
  }
}

// ONE lane, behind the barrier that follows the parts: the workgroup's part is added to query q's record, query_sizes and
// totals[0..1] with vector atomics (a workgroup without a match adds nothing; an F64 column: a sum in u64 space means
// nothing, both words stay 0)
template <bool HIST, uint32_t N>
__device__ __forceinline__ void agg_stats_publish(const unsigned long long (&part)[WALK_WAVES][N], const TqkAggParams &p, uint32_t q) {
  unsigned long long matches = 0, count = 0, lo = 0, hi = 0, in_bounds = 0, out_of_range = 0;
  uint64_t wmn = ~0ull, wmx = 0ull;
  for (uint32_t v = 0; v < WALK_WAVES; ++v) {
    matches += part[v][0];
    count += part[v][1];
    wmn = part[v][2] < wmn ? part[v][2] : wmn;
    wmx = part[v][3] > wmx ? part[v][3] : wmx;
    lo += part[v][4];
    hi += part[v][5];
    in_bounds += part[v][6];
    out_of_range += part[v][7];
  }
  if (matches == 0ull) return;  // (nothing to add: an empty slice, or a query without a match in it)
  TqkAggStats *const S = p.stats + q;
  atomicAdd(&S->matches, matches);
  atomicAdd(p.query_sizes + q, (uint32_t)matches);
  atomicAdd(p.totals + 0, matches);
  if (count == 0ull) return;
  atomicAdd(p.totals + 1, count);
  atomicAdd(&S->count, count);
  atomicMin(&S->min_value, (unsigned long long)wmn);
  atomicMax(&S->max_value, (unsigned long long)wmx);
  if (p.value_type != TQ_AGGV_F64) add128(&S->sum_lo, &S->sum_hi, lo, hi);
  if (HIST) {
    if (in_bounds) atomicAdd(&S->in_bounds, in_bounds);
    if (out_of_range) atomicAdd(&S->out_of_range, out_of_range);
  }
}

// ---- the table of 40-byte bucket records (TqkAggBucketStats) of a metric column B, one per bucket or key.  In LDS it is
// five arrays the KERNEL declares with its capacity, one per field: {doc count | value count << 32}, min, max, the sums of
// the values' low and high halves.  A doc costs ONE 64-bit add on the counts (each below 2^31: the low word cannot carry)
// and, with a value, ds min / max and two 64-bit adds; sum_b == false (an F64 column): both sum words stay 0.
struct BucketTable {
  unsigned long long *cv, *mn, *mx, *lo, *hi;
  // entries [0, n) by the whole workgroup; a barrier follows
  __device__ __forceinline__ void zero(uint32_t n) const {
    for (uint32_t i = threadIdx.x; i < n; i += WALK_THREADS) {
      cv[i] = 0ull;
      mn[i] = ~0ull;
      mx[i] = 0ull;
      lo[i] = 0ull;
      hi[i] = 0ull;
    }
  }
  // one doc of entry idx, with value vb in B or without one
  __device__ __forceinline__ void add(uint32_t idx, bool has_b, uint64_t vb, bool sum_b) const {
    atomicAdd(&cv[idx], has_b ? 0x100000001ull : 1ull);
    if (has_b) {
      atomicMin(&mn[idx], (unsigned long long)vb);
      atomicMax(&mx[idx], (unsigned long long)vb);
      if (sum_b) {
        atomicAdd(&lo[idx], (unsigned long long)(vb & 0xFFFFFFFFull));
        atomicAdd(&hi[idx], (unsigned long long)(vb >> 32));
      }
    }
  }
  // the same doc above the table's capacity: straight to the query's count row and record row
  __device__ static __forceinline__ void add_global(uint32_t *row, TqkAggBucketStats *recs, uint32_t idx, bool has_b, uint64_t vb,
                                                    bool sum_b) {
    atomicAdd(row + idx, 1u);
    if (has_b) {
      TqkAggBucketStats *const R = recs + idx;
      atomicAdd(&R->count, 1ull);
      atomicMin(&R->min_value, (unsigned long long)vb);
      atomicMax(&R->max_value, (unsigned long long)vb);
      if (sum_b) add128(&R->sum_lo, &R->sum_hi, vb & 0xFFFFFFFFull, vb >> 32);
    }
  }
  // entries [0, n) into the rows, by the whole workgroup behind a barrier: one pass over the non-empty entries
  __device__ __forceinline__ void flush(uint32_t n, uint32_t *row, TqkAggBucketStats *recs, bool sum_b) const {
    for (uint32_t i = threadIdx.x; i < n; i += WALK_THREADS) {
      const unsigned long long c = cv[i];
      const uint32_t docs = (uint32_t)c;
      const unsigned long long vals = c >> 32;
      if (docs) atomicAdd(row + i, docs);
      if (vals) {
        TqkAggBucketStats *const R = recs + i;
        atomicAdd(&R->count, vals);
        atomicMin(&R->min_value, mn[i]);
        atomicMax(&R->max_value, mx[i]);
        if (sum_b) add128(&R->sum_lo, &R->sum_hi, lo[i], hi[i]);
      }
    }
  }
};

// records [0, n) of a record row = zeros with min_value = ~0, by the whole workgroup
__device__ __forceinline__ void bucket_records_init(TqkAggBucketStats *recs, uint32_t n) {
  static_assert(sizeof(TqkAggBucketStats) == 40, "five 64-bit words, min_value the second");
  unsigned long long *const words = reinterpret_cast<unsigned long long *>(recs);
  for (uint32_t w = threadIdx.x; w < n * 5u; w += WALK_THREADS) words[w] = w % 5u == 1u ? ~0ull : 0ull;
}

}  // namespace
