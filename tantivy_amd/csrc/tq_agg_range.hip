// tq_agg_range.hip — range aggregation (tq_agg_range_batch*): doc counts per range of a bucket column A and, with a metric,
// a stats record of a metric column B per range (src/aggregation/bucket/range.rs:276-305 collect, :431-437 get_bucket_pos;
// src/aggregation/metric/stats.rs:282-306 under a parent_bucket_id), for every query of a batch in ONE pass over its match
// bits.  The buckets are the host plan's (tq_agg_range_plan, tq_agg_range.cpp): they cover the whole u64 space, so every doc
// with a value in A is counted in exactly one of them.  No f64 in this file: the request's bounds were converted into the
// column's u64 space once, on the host, and the kernel compares u64 values.
//
// agg_range  workgroup = (query, slice of the bitmap words), query fastest in the grid.  Assembled from the shared walk
//            (docset_walk, tq_docset_walk.hpp), col_value and the top-level record (AggStatsLane, agg_stats_*), and — with
//            a metric — the bucket-record table (BucketTable: zero / add / add_global / flush), all of tq_agg_device.hpp;
//            the records and rows are initialised by tq_agg.hip's and tq_agg_sub.hip's init launches, shared as well.  Its
//            own: the buckets' starts, copied into LDS by every workgroup in front of the walk (always: <= 8 KB), and per
//            doc with a value in A the search of tq_agg_range_search.hpp over them, then ONE update of that bucket —
//            counts only: a uint32_t LDS table flushed with one vector atomic per non-zero entry, or (n_buckets above
//            "agg_lds_buckets") an atomic on the query's row; with a metric: BucketTable in LDS, or the query's row and
//            records above "agg_lds_buckets".  A SMALL and a LARGE instantiation of each; the small one also holds fewer
//            starts.  The wavefronts' parts of the record alias the slabs behind the walk (the LDS budget below).
// Integer atomics only: the result is deterministic.  Plain vector stores and vector atomics; nothing is written at or
// past n_buckets of a row: a search result >= n_buckets cannot occur, is checked anyway, and drops the doc.
// HBM model: agg_kernel's for A + 8 x n_buckets per launch group (the starts) + with a metric agg_sub_kernel's terms for B.
#include <algorithm>

#include "tq_agg_device.hpp"
#include "tq_agg_range_search.hpp"
#include "tq_column_read.hpp"
#include "tq_common.hpp"
#include "tq_docset_walk.hpp"
#include "tq_launch.h"

namespace {

// LDS of a workgroup: the slabs' 16 KB, the starts (8 B each) and the table — 4 B per bucket (counts only) or 40 B (with a
// metric).  1 024 forty-byte entries + 1 024 starts + the slabs are exactly the static 64 KB, with no room for the
// wavefronts' parts (320 B): the parts therefore ALIAS the head of the slabs, which nobody reads once every wavefront has
// left the walk — one more barrier per workgroup.  SMALL carries agg_sub_kernel's choice (profiles/agg_sub_lds_ab.txt: the
// largest record table that cost nothing there); it was NOT measured again for this kernel.
constexpr uint32_t AR_MAX_BUCKETS = 1024;  // TQ_AGG_RANGE_MAX_BUCKETS
#ifndef TQ_AGG_RANGE_LDS_LARGE
#define TQ_AGG_RANGE_LDS_LARGE 1024
#endif
#ifndef TQ_AGG_RANGE_LDS_SMALL
#define TQ_AGG_RANGE_LDS_SMALL 128
#endif
constexpr uint32_t AR_LDS_LARGE = TQ_AGG_RANGE_LDS_LARGE;
constexpr uint32_t AR_LDS_SMALL = TQ_AGG_RANGE_LDS_SMALL;
constexpr uint32_t AR_PART = AGG_STATS_PART + 2;  // words of a wavefront's part: the record's, bucketed docs, those with a value in B
static_assert(AR_LDS_SMALL >= 1u && AR_LDS_SMALL <= AR_LDS_LARGE && AR_LDS_LARGE <= AR_MAX_BUCKETS, "two tables");
static_assert(AR_LDS_LARGE * 40u + AR_MAX_BUCKETS * 8u + WALK_SLAB_ENTRIES * 2u <= 65536u, "the static LDS of a workgroup, with a metric");
static_assert(AR_MAX_BUCKETS * 4u + AR_MAX_BUCKETS * 8u + WALK_SLAB_ENTRIES * 2u <= 65536u, "the static LDS of a workgroup, counts only");
static_assert(WALK_WAVES * AR_PART * 8u <= WALK_SLAB_ENTRIES * 2u && WALK_SLAB_ENTRIES % 4u == 0u, "the parts fit the slabs they alias");

// CAP: the table's capacity in buckets.  CAP == AR_LDS_SMALL is launched for n_buckets <= AR_LDS_SMALL alone, so it holds
// that many starts; any other instantiation holds AR_MAX_BUCKETS of them.
template <bool OPTIONAL_A, bool OPTIONAL_B, bool METRIC, uint32_t CAP>
__global__ __launch_bounds__(WALK_THREADS) void agg_range_kernel(TqkAggRangeParams p) {
  constexpr uint32_t N_STARTS = CAP == AR_LDS_SMALL ? AR_LDS_SMALL : AR_MAX_BUCKETS;
  constexpr uint32_t REC_CAP = METRIC ? CAP : 1u, CNT_CAP = METRIC ? 1u : CAP;
  __shared__ unsigned long long slab_words[WALK_SLAB_ENTRIES / 4u];  // the walk's slabs; behind the walk, the parts
  __shared__ uint64_t starts[N_STARTS];
  __shared__ unsigned long long t_cv[REC_CAP], t_mn[REC_CAP], t_mx[REC_CAP], t_lo[REC_CAP], t_hi[REC_CAP];  // BucketTable's fields
  __shared__ uint32_t hist[CNT_CAP];
  uint16_t *const slabs = reinterpret_cast<uint16_t *>(slab_words);
  unsigned long long(&part)[WALK_WAVES][AR_PART] = *reinterpret_cast<unsigned long long(*)[WALK_WAVES][AR_PART]>(slab_words);
  const TqkAggParams &a = p.s.a;
  const BucketTable table{t_cv, t_mn, t_mx, t_lo, t_hi};
  const int lane = (int)__lane_id();
  const uint32_t wave = threadIdx.x >> 6;
  const uint32_t q = blockIdx.x % a.ds.n_queries, slice = blockIdx.x / a.ds.n_queries;
  const uint32_t n_buckets = a.n_buckets <= N_STARTS ? a.n_buckets : 0u;  // (uniform; the launch refuses more: nothing is bucketed)
  const bool in_lds = n_buckets <= a.lds_buckets && n_buckets <= CAP;     // (uniform)
  const bool sum_b = p.s.value_type_b != TQ_AGGV_F64;                       // (uniform; F64: both sum words stay 0)
  uint32_t *const row = a.buckets + (size_t)q * a.bucket_stride;
  TqkAggBucketStats *const recs = METRIC ? p.s.bucket_stats + (size_t)q * a.bucket_stride : nullptr;
  for (uint32_t i = threadIdx.x; i < n_buckets; i += WALK_THREADS) starts[i] = p.starts[i];
  if (in_lds) {
    if (METRIC)
      table.zero(n_buckets);
    else
      for (uint32_t i = threadIdx.x; i < n_buckets; i += WALK_THREADS) hist[i] = 0u;
  }
  __syncthreads();
  AggStatsLane acc;
  uint32_t bucketed = 0, valued_b = 0;  // per lane
  const uint32_t cnt = docset_walk(a.ds, a.ds.queries + q, slice, a.words_per_slice, slabs, wave, lane, [&](bool has, uint32_t doc) {
    uint32_t r = 0;
    if (!(has && rg_row<OPTIONAL_A>(a.col, doc, r))) return;
    const uint64_t v = col_value(a.col, a.min_value, a.gcd, r);
    acc.add(v);
    ++acc.inb;  // every doc with a value has a bucket: in_bounds == count
    const uint32_t idx = tq_range_bucket_of(starts, n_buckets, v);
    if (idx >= n_buckets) {  // (not reached with a plan's starts; n_buckets == 0 comes here)
      ++acc.oor;
      return;
    }
    ++bucketed;
    if (!METRIC) {
      if (in_lds)
        atomicAdd(&hist[idx], 1u);
      else
        atomicAdd(row + idx, 1u);
      return;
    }
    uint32_t rb = 0;
    const bool has_b = rg_row<OPTIONAL_B>(p.s.col_b, doc, rb);
    const uint64_t vb = has_b ? col_value(p.s.col_b, p.s.min_value_b, p.s.gcd_b, rb) : 0ull;
    valued_b += has_b ? 1u : 0u;
    if (in_lds)
      table.add(idx, has_b, vb, sum_b);
    else
      BucketTable::add_global(row, recs, idx, has_b, vb, sum_b);
  });
  __syncthreads();  // every wavefront has left the walk: the slabs are free for the parts, and the LDS table updates are done
  agg_stats_wave_part(part[wave], cnt, acc, lane, bucketed, valued_b);
  __syncthreads();
  if (in_lds) {
    if (METRIC) {
      table.flush(n_buckets, row, recs, sum_b);
    } else {
      for (uint32_t i = threadIdx.x; i < n_buckets; i += WALK_THREADS) {
        const uint32_t c = hist[i];
        if (c) atomicAdd(row + i, c);
      }
    }
  }
  if (threadIdx.x != 0u) return;
  agg_stats_publish<true>(part, a, q);
  if (!METRIC) return;
  unsigned long long in_buckets = 0, with_b = 0;  // (non-zero only where the record had matches with a value to publish)
  for (uint32_t v = 0; v < WALK_WAVES; ++v) {
    in_buckets += part[v][AGG_STATS_PART];
    with_b += part[v][AGG_STATS_PART + 1];
  }
  if (with_b) atomicAdd(a.totals + 3, with_b);
  if (in_buckets) atomicAdd(a.totals + 4, in_buckets);
}

template <bool METRIC, uint32_t CAP>
void agg_range_launch(const TqkAggRangeParams &p, hipStream_t st) {
  const dim3 grid(p.s.a.ds.n_queries * p.s.a.n_slices), block(WALK_THREADS);
  const bool opt_a = p.s.a.col.present != nullptr, opt_b = METRIC && p.s.col_b.present != nullptr;
  if (opt_a) {
    if (opt_b)
      agg_range_kernel<true, METRIC, METRIC, CAP><<<grid, block, 0, st>>>(p);
    else
      agg_range_kernel<true, false, METRIC, CAP><<<grid, block, 0, st>>>(p);
  } else {
    if (opt_b)
      agg_range_kernel<false, METRIC, METRIC, CAP><<<grid, block, 0, st>>>(p);
    else
      agg_range_kernel<false, false, METRIC, CAP><<<grid, block, 0, st>>>(p);
  }
}

}  // namespace

void tqk_agg_range_lds_capacities(uint32_t out[2]) {
  out[0] = AR_LDS_SMALL;
  out[1] = AR_LDS_LARGE;
}

hipError_t tqk_launch_agg_range(const TqkAggRangeParams &p, bool metric, hipStream_t st) {
  const TqkAggParams &a = p.s.a;
  if (!a.ds.n_queries || !a.n_slices) return hipSuccess;
  if (a.col.codec > TQK_COL_BLOCKWISE || (metric && p.s.col_b.codec > TQK_COL_BLOCKWISE)) return hipErrorInvalidValue;
  if (!a.n_buckets || a.n_buckets > AR_MAX_BUCKETS || a.n_buckets > a.bucket_stride || !a.buckets || !p.starts)
    return hipErrorInvalidValue;
  if (metric && !p.s.bucket_stats) return hipErrorInvalidValue;
  const bool small = a.n_buckets <= std::min(a.lds_buckets, AR_LDS_SMALL);
  if (metric) {
    if (small)
      agg_range_launch<true, AR_LDS_SMALL>(p, st);
    else  // (the large table, or past "agg_lds_buckets" straight to the row and the records)
      agg_range_launch<true, AR_LDS_LARGE>(p, st);
  } else {
    if (small)
      agg_range_launch<false, AR_LDS_SMALL>(p, st);
    else  // (the table of every bucket, or past "agg_lds_buckets" straight to the row)
      agg_range_launch<false, AR_MAX_BUCKETS>(p, st);
  }
  return hipGetLastError();
}
