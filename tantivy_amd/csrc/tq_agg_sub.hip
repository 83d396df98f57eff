// tq_agg_sub.hip — sub-aggregations (tq_agg_sub_batch*): a histogram over a bucket column A with a stats record of a metric
// column B per bucket (src/aggregation/bucket/histogram/histogram.rs:489-505, the nested path of collect;
// src/aggregation/metric/stats.rs:282-306 SegmentStatsCollector::collect with a parent_bucket_id, :164
// IntermediateStats::collect), for every query of a batch in ONE pass over its match bits.  What tq_agg.hip's agg_kernel
// leaves of A — the 64-byte record and the dense row of doc counts — comes out bit for bit the same; beside it, per bucket
// of the row, count / min / max / 128-bit sum of B's u64-space values over exactly the docs counted in that bucket.
//
// agg_sub  workgroup = (query, slice of the bitmap words).  Assembled from the shared walk (docset_walk,
//          tq_docset_walk.hpp), agg_kernel's pieces for A (col_value, AggStatsLane, agg_stats_*: tq_agg_device.hpp; the
//          f64 conversions: tq_agg_value.hpp) and the bucket-record table (BucketTable, tq_agg_device.hpp).  Its own: a
//          doc that is bucketed — a value in A inside the bounds, its bucket inside the row — takes rg_row + col_value of
//          B (a doc that is not bucketed, or has no value in B, loads nothing of B) and adds to the bucket's entry of the
//          workgroup's LDS table (n_buckets <= lds_buckets; a SMALL and a LARGE table, two instantiations), flushed in one
//          pass over its non-empty buckets, or, above the capacity, to the query's row and record in global memory.
// init     the bucket records [0, n_buckets) of every query (bucket_records_init).
// Integer atomics only: the result is deterministic.  Plain vector stores and vector atomics; nothing is written at or
// past n_buckets of a row.  HBM model: agg_kernel's for A + 8 per bucketed doc with a value in B + 8 per bucketed doc of an
// Optional B (its presence word) + 40 x n_buckets per query.
#include <algorithm>

#include "tq_agg_device.hpp"
#include "tq_agg_value.hpp"
#include "tq_column_read.hpp"
#include "tq_common.hpp"
#include "tq_docset_walk.hpp"
#include "tq_launch.h"

namespace {

// the LDS table: 40 bytes per bucket beside the slabs' 16 KB.  The capacities were chosen from an A/B of table sizes
// (profiles/agg_sub_lds_ab.txt)
#ifndef TQ_AGG_SUB_LDS_LARGE
#define TQ_AGG_SUB_LDS_LARGE 1024
#endif
#ifndef TQ_AGG_SUB_LDS_SMALL
#define TQ_AGG_SUB_LDS_SMALL 128
#endif
constexpr uint32_t AS_LDS_LARGE = TQ_AGG_SUB_LDS_LARGE;
constexpr uint32_t AS_LDS_SMALL = TQ_AGG_SUB_LDS_SMALL;
constexpr uint32_t AS_PART = AGG_STATS_PART + 2;  // words of a wavefront's part: the record's, bucketed docs, those with a value in B
static_assert(AS_LDS_SMALL >= 1u && AS_LDS_SMALL <= AS_LDS_LARGE, "two tables");
static_assert(AS_LDS_LARGE * 40u + WALK_SLAB_ENTRIES * 2u + WALK_WAVES * AS_PART * 8u <= 65536u, "the static LDS of a workgroup");

template <bool OPTIONAL_A, bool OPTIONAL_B, uint32_t CAP>
__global__ __launch_bounds__(WALK_THREADS) void agg_sub_kernel(TqkAggSubParams p) {
  __shared__ uint16_t slabs[WALK_SLAB_ENTRIES];
  __shared__ unsigned long long t_cv[CAP], t_mn[CAP], t_mx[CAP], t_lo[CAP], t_hi[CAP];  // BucketTable's fields
  __shared__ unsigned long long part[WALK_WAVES][AS_PART];
  const BucketTable table{t_cv, t_mn, t_mx, t_lo, t_hi};
  const int lane = (int)__lane_id();
  const uint32_t wave = threadIdx.x >> 6;
  const uint32_t q = blockIdx.x % p.a.ds.n_queries, slice = blockIdx.x / p.a.ds.n_queries;
  const uint32_t n_buckets = p.a.n_buckets;
  const bool in_lds = n_buckets <= p.a.lds_buckets && n_buckets <= CAP;  // (uniform)
  const bool sum_b = p.value_type_b != TQ_AGGV_F64;                       // (uniform; F64: both sum words stay 0)
  uint32_t *const row = p.a.buckets + (size_t)q * p.a.bucket_stride;
  TqkAggBucketStats *const recs = p.bucket_stats + (size_t)q * p.a.bucket_stride;
  if (in_lds) {
    table.zero(n_buckets);
    __syncthreads();
  }
  AggStatsLane acc;
  uint32_t bucketed = 0, valued_b = 0;  // per lane
  const uint32_t cnt = docset_walk(p.a.ds, p.a.ds.queries + q, slice, p.a.words_per_slice, slabs, wave, lane, [&](bool has, uint32_t doc) {
    uint32_t r = 0;
    if (!(has && rg_row<OPTIONAL_A>(p.a.col, doc, r))) return;
    const uint64_t v = col_value(p.a.col, p.a.min_value, p.a.gcd, r);
    acc.add(v);
    const double val = tq_agg_f64(v, p.a.value_type);
    if (!(p.a.bounds_min <= val && val <= p.a.bounds_max)) return;  // (HistogramBounds::contains: never true for NaN, +-inf)
    ++acc.inb;
    const int64_t pos = tq_agg_sat_i64(floor((val - p.a.offset) / p.a.interval));
    const uint64_t idx64 = (uint64_t)pos - (uint64_t)p.a.base_pos;  // (a pos below base_pos wraps to a huge index)
    if (idx64 >= (uint64_t)n_buckets) {
      ++acc.oor;
      return;
    }
    const uint32_t idx = (uint32_t)idx64;
    ++bucketed;
    uint32_t rb = 0;
    const bool has_b = rg_row<OPTIONAL_B>(p.col_b, doc, rb);
    const uint64_t vb = has_b ? col_value(p.col_b, p.min_value_b, p.gcd_b, rb) : 0ull;
    valued_b += has_b ? 1u : 0u;
    if (in_lds)
      table.add(idx, has_b, vb, sum_b);
    else
      BucketTable::add_global(row, recs, idx, has_b, vb, sum_b);
  });
  agg_stats_wave_part(part[wave], cnt, acc, lane, bucketed, valued_b);
  __syncthreads();  // (also: every wavefront's LDS table updates are done)
  if (in_lds) table.flush(n_buckets, row, recs, sum_b);
  if (threadIdx.x != 0u) return;
  agg_stats_publish<true>(part, p.a, q);
  unsigned long long in_buckets = 0, with_b = 0;  // (non-zero only where the record had matches with a value to publish)
  for (uint32_t v = 0; v < WALK_WAVES; ++v) {
    in_buckets += part[v][AGG_STATS_PART];
    with_b += part[v][AGG_STATS_PART + 1];
  }
  if (with_b) atomicAdd(p.a.totals + 3, with_b);
  if (in_buckets) atomicAdd(p.a.totals + 4, in_buckets);
}

// bucket record i < n_buckets of query q = zeros with min_value = ~0.  grid = n_queries
__global__ __launch_bounds__(WALK_THREADS) void agg_sub_init_kernel(TqkAggBucketStats *bucket_stats, uint32_t n_buckets,
                                                                  uint32_t bucket_stride) {
  bucket_records_init(bucket_stats + (size_t)blockIdx.x * bucket_stride, n_buckets);
}

template <uint32_t CAP>
void agg_sub_launch(const TqkAggSubParams &p, hipStream_t st) {
  const dim3 grid(p.a.ds.n_queries * p.a.n_slices), block(WALK_THREADS);
  if (p.a.col.present) {
    if (p.col_b.present)
      agg_sub_kernel<true, true, CAP><<<grid, block, 0, st>>>(p);
    else
      agg_sub_kernel<true, false, CAP><<<grid, block, 0, st>>>(p);
  } else {
    if (p.col_b.present)
      agg_sub_kernel<false, true, CAP><<<grid, block, 0, st>>>(p);
    else
      agg_sub_kernel<false, false, CAP><<<grid, block, 0, st>>>(p);
  }
}

}  // namespace

void tqk_agg_sub_lds_capacities(uint32_t out[2]) {
  out[0] = AS_LDS_SMALL;
  out[1] = AS_LDS_LARGE;
}

hipError_t tqk_launch_agg_sub_init(TqkAggBucketStats *bucket_stats, uint32_t n_queries, uint32_t n_buckets, uint32_t bucket_stride,
                                   hipStream_t st) {
  if (!n_queries || !n_buckets) return hipSuccess;
  if (n_buckets > bucket_stride || !bucket_stats) return hipErrorInvalidValue;
  agg_sub_init_kernel<<<dim3(n_queries), dim3(WALK_THREADS), 0, st>>>(bucket_stats, n_buckets, bucket_stride);
  return hipGetLastError();
}

hipError_t tqk_launch_agg_sub(const TqkAggSubParams &p, hipStream_t st) {
  if (!p.a.ds.n_queries || !p.a.n_slices) return hipSuccess;
  if (p.a.col.codec > TQK_COL_BLOCKWISE || p.col_b.codec > TQK_COL_BLOCKWISE) return hipErrorInvalidValue;
  if (!p.a.n_buckets || p.a.n_buckets > p.a.bucket_stride || !p.a.buckets || !p.bucket_stats) return hipErrorInvalidValue;
  if (p.a.n_buckets <= std::min(p.a.lds_buckets, AS_LDS_SMALL))
    agg_sub_launch<AS_LDS_SMALL>(p, st);
  else  // (the large table, or past "agg_lds_buckets" straight to the row and the records)
    agg_sub_launch<AS_LDS_LARGE>(p, st);
  return hipGetLastError();
}
