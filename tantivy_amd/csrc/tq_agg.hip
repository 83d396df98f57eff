// tq_agg.hip — aggregations over a fast field (tq_agg_batch*): what a stats metric (src/aggregation/metric/stats.rs:86-176,
// IntermediateStats::collect) and a histogram bucket aggregation (src/aggregation/bucket/histogram/histogram.rs:468-518
// collect, :738-741 get_bucket_pos_f64; src/aggregation/mod.rs:351-383 f64_from_fastfield_u64) leave of a segment, for
// every query of a batch in ONE pass over its match bits.  No doc set is written: the match bits (docset_word,
// tq_docset_word.hpp) and the column readers (rg_row / rg_value, tq_column_read.hpp) meet as in tq_sort.hip, with
// accumulators in place of the top-k heap.
//
// agg      workgroup = (query, slice of the bitmap words), query fastest in the grid.  Assembled from the shared walk
//          (docset_walk, tq_docset_walk.hpp: a lane per matching doc), col_value and the top-level record's accumulators,
//          reduction and publication (AggStatsLane, agg_stats_*: tq_agg_device.hpp), and the f64 conversions of
//          tq_agg_value.hpp.  Its own: per doc with a value, val = the value as the reference's f64, the contains test,
//          pos = floor((val - offset) / interval) saturated to i64, one atomic add on bucket pos - base_pos — of the
//          workgroup's LDS table (n_buckets <= lds_buckets; a table of 2 048 or of 8 192 buckets, two instantiations),
//          flushed with one atomic add per non-zero bucket, or of the query's row.  Integer atomics: deterministic.
// init     the records (zeros, min_value = ~0) and entries [0, n_buckets) of every row, in front of the launch.
// Plain vector stores and vector atomics only; nothing is written at or past a row's n_buckets: a doc whose bucket is
// outside [0, n_buckets) — none, by the monotonicity of the dense range — is counted in out_of_range and dropped.
// HBM model: lists x bitmap words x 4 + 8 per matching doc with a value + 8 per matching doc of an Optional column
// (its presence word) + 64 + 4 x n_buckets per query.
#include <algorithm>

#include "tq_agg_device.hpp"
#include "tq_agg_value.hpp"
#include "tq_column_read.hpp"
#include "tq_common.hpp"
#include "tq_docset_walk.hpp"
#include "tq_launch.h"

namespace {

// the LDS table's capacity is a template argument: 0 (stats alone), a SMALL table that leaves six wavefronts per SIMD, the
// LARGE one that leaves three (the walk is bound by the latency of its gathers: measured)
#ifndef TQ_AGG_LDS_BUCKETS
#define TQ_AGG_LDS_BUCKETS 8192
#endif
#ifndef TQ_AGG_LDS_SMALL
#define TQ_AGG_LDS_SMALL 2048
#endif
constexpr uint32_t AG_LDS_BUCKETS = TQ_AGG_LDS_BUCKETS;  // 32 KB beside the slabs' 16 KB: three workgroups per CU
constexpr uint32_t AG_LDS_SMALL = TQ_AGG_LDS_SMALL;      //  8 KB: six
static_assert(AG_LDS_SMALL <= AG_LDS_BUCKETS && AG_LDS_BUCKETS * 4u + 16640u <= 65536u, "the static LDS of a workgroup");

template <bool OPTIONAL, uint32_t CAP>
__global__ __launch_bounds__(WALK_THREADS) void agg_kernel(TqkAggParams p) {
  constexpr bool HIST = CAP != 0u;
  __shared__ uint16_t slabs[WALK_SLAB_ENTRIES];
  __shared__ uint32_t hist[HIST ? CAP : 1u];
  __shared__ unsigned long long part[WALK_WAVES][AGG_STATS_PART];
  const int lane = (int)__lane_id();
  const uint32_t wave = threadIdx.x >> 6;
  const uint32_t q = blockIdx.x % p.ds.n_queries, slice = blockIdx.x / p.ds.n_queries;
  const uint32_t n_buckets = HIST ? p.n_buckets : 0u;
  const bool in_lds = HIST && n_buckets <= p.lds_buckets && n_buckets <= CAP;  // (uniform)
  uint32_t *const row = HIST ? p.buckets + (size_t)q * p.bucket_stride : nullptr;
  if (HIST && in_lds) {
    for (uint32_t i = threadIdx.x; i < n_buckets; i += WALK_THREADS) hist[i] = 0u;
    __syncthreads();
  }
  AggStatsLane acc;
  const uint32_t cnt = docset_walk(p.ds, p.ds.queries + q, slice, p.words_per_slice, slabs, wave, lane, [&](bool has, uint32_t doc) {
    uint32_t r = 0;
    if (!(has && rg_row<OPTIONAL>(p.col, doc, r))) return;
    const uint64_t v = col_value(p.col, p.min_value, p.gcd, r);
    acc.add(v);
    if (!HIST) return;
    const double val = tq_agg_f64(v, p.value_type);
    if (!(p.bounds_min <= val && val <= p.bounds_max)) return;  // (HistogramBounds::contains: never true for NaN, +-inf)
    ++acc.inb;
    const int64_t pos = tq_agg_sat_i64(floor((val - p.offset) / p.interval));
    const uint64_t idx = (uint64_t)pos - (uint64_t)p.base_pos;  // (a pos below base_pos wraps to a huge index)
    if (idx >= (uint64_t)n_buckets)
      ++acc.oor;
    else if (in_lds)
      atomicAdd(&hist[(uint32_t)idx], 1u);
    else
      atomicAdd(row + (uint32_t)idx, 1u);
  });
  agg_stats_wave_part(part[wave], cnt, acc, lane);
  __syncthreads();  // (also: every wavefront's LDS bucket adds are done)
  if (HIST && in_lds) {
    for (uint32_t i = threadIdx.x; i < n_buckets; i += WALK_THREADS) {
      const uint32_t c = hist[i];
      if (c) atomicAdd(row + i, c);
    }
  }
  if (threadIdx.x == 0u) agg_stats_publish<HIST>(part, p, q);
}

// record q = zeros with min_value = ~0; entries [0, n_buckets) of row q = 0.  grid = n_queries
__global__ __launch_bounds__(WALK_THREADS) void agg_init_kernel(TqkAggStats *stats, uint32_t *buckets, uint32_t n_buckets,
                                                              uint32_t bucket_stride) {
  const uint32_t q = blockIdx.x;
  if (threadIdx.x < 8u)
    reinterpret_cast<unsigned long long *>(stats + q)[threadIdx.x] = threadIdx.x == 2u ? ~0ull : 0ull;
  uint32_t *const row = buckets + (size_t)q * bucket_stride;
  for (uint32_t i = threadIdx.x; i < n_buckets; i += WALK_THREADS) row[i] = 0u;
}

template <uint32_t CAP>
void agg_launch(const TqkAggParams &p, hipStream_t st) {
  const dim3 grid(p.ds.n_queries * p.n_slices), block(WALK_THREADS);
  if (p.col.present)
    agg_kernel<true, CAP><<<grid, block, 0, st>>>(p);
  else
    agg_kernel<false, CAP><<<grid, block, 0, st>>>(p);
}

}  // namespace

uint32_t tqk_agg_step_words() { return WALK_STEP_WORDS; }
uint32_t tqk_agg_lds_buckets() { return AG_LDS_BUCKETS; }

hipError_t tqk_launch_agg_init(TqkAggStats *stats, uint32_t *buckets, uint32_t n_queries, uint32_t n_buckets,
                               uint32_t bucket_stride, hipStream_t st) {
  if (!n_queries) return hipSuccess;
  if (n_buckets > bucket_stride || (n_buckets && !buckets)) return hipErrorInvalidValue;
  agg_init_kernel<<<dim3(n_queries), dim3(WALK_THREADS), 0, st>>>(stats, buckets, n_buckets, bucket_stride);
  return hipGetLastError();
}

hipError_t tqk_launch_agg(const TqkAggParams &p, hipStream_t st) {
  if (!p.ds.n_queries || !p.n_slices) return hipSuccess;
  if (p.col.codec > TQK_COL_BLOCKWISE) return hipErrorInvalidValue;
  if (p.n_buckets > p.bucket_stride || (p.n_buckets && !p.buckets)) return hipErrorInvalidValue;
  if (!p.n_buckets)
    agg_launch<0u>(p, st);
  else if (p.n_buckets <= std::min(p.lds_buckets, AG_LDS_SMALL))
    agg_launch<AG_LDS_SMALL>(p, st);
  else  // (the large table, or past "agg_lds_buckets" straight to the row)
    agg_launch<AG_LDS_BUCKETS>(p, st);
  return hipGetLastError();
}
