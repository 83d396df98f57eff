// tq_agg_sub.hip — sub-aggregations (tq_agg_sub_batch*): a histogram over a bucket column A with a stats record of a metric
// column B per bucket (src/aggregation/bucket/histogram/histogram.rs:489-505, the nested path of collect;
// src/aggregation/metric/stats.rs:282-306 SegmentStatsCollector::collect with a parent_bucket_id, :164
// IntermediateStats::collect), for every query of a batch in ONE pass over its match bits.  What tq_agg.hip's agg_kernel
// leaves of A — the 64-byte record and the dense row of doc counts — comes out bit for bit the same; beside it, per bucket
// of the row, count / min / max / 128-bit sum of B's u64-space values over exactly the docs counted in that bucket.
//
// agg_sub  agg_kernel's walk (its own copy: tq_agg.hip and tq_sort.hip keep their code objects byte for byte, and with them
//          the register tables of DESIGN.md 3.4h / 3.4i): workgroup = (query, slice of the bitmap words), four wavefronts,
//          docset_word per lane, the popcount prefix sum, the LDS slab, one lane per matching doc for rg_row + rg_value of
//          A.  A doc that is bucketed — a value in A inside the bounds, its bucket inside the row — then takes rg_row +
//          rg_value of B (a doc that is not bucketed, or has no value in B, loads nothing of B) and adds to
//            - the bucket's entry of the workgroup's LDS table (n_buckets <= lds_buckets; a SMALL and a LARGE table, two
//              instantiations): ONE 64-bit add on {doc count, value count} (each below 2^31: the low word cannot carry),
//              and for a doc with a value ds min / max and two 64-bit adds on the sums of the value's 32-bit halves;
//            - or, above the capacity, the query's row and record in global memory, per doc.
//          The table is flushed in one pass over its non-empty buckets: vector atomics on the row and the record, the
//          128-bit sum low word first, carrying where the add wrapped — as agg_kernel does for the top-level record.
// init     the bucket records [0, n_buckets) of every query: zeros with min_value = ~0.
// Integer atomics only: the result is deterministic.  Plain vector stores and vector atomics; nothing is written at or
// past n_buckets of a row.  HBM model: agg_kernel's for A + 8 per bucketed doc with a value in B + 8 per bucketed doc of an
// Optional B (its presence word) + 40 x n_buckets per query.
#include <algorithm>

#include "tq_column_read.hpp"
#include "tq_common.hpp"
#include "tq_docset_word.hpp"
#include "tq_launch.h"

namespace {

constexpr uint32_t AS_THREADS = 256;
constexpr uint32_t AS_WAVES = AS_THREADS / 64;
constexpr uint32_t AS_CHUNK_WORDS = 64;                  // one word per lane
constexpr uint32_t AS_CHUNK_DOCS = AS_CHUNK_WORDS * 32;  // slab entries per wavefront
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
constexpr uint32_t AS_PART = 10;  // words of a wavefront's part
static_assert(AS_LDS_SMALL >= 1u && AS_LDS_SMALL <= AS_LDS_LARGE, "two tables");
static_assert(AS_LDS_LARGE * 40u + AS_WAVES * AS_CHUNK_DOCS * 2u + AS_WAVES * AS_PART * 8u <= 65536u, "the static LDS of a workgroup");
constexpr uint32_t AS_VALUE_I64 = 1, AS_VALUE_F64 = 2;  // TQ_VALUE_* (U64 = 0)

__device__ __forceinline__ uint64_t as_value(const TqkColumn &col, uint64_t min_value, uint64_t gcd, uint32_t row) {
  const uint32_t codec = col.codec;  // (uniform)
  if (codec == TQK_COL_LINEAR) return rg_value<TQK_COL_LINEAR>(col, row);
  const uint64_t n = codec == TQK_COL_BITPACKED ? rg_value<TQK_COL_BITPACKED>(col, row) : rg_value<TQK_COL_BLOCKWISE>(col, row);
  return min_value + gcd * n;
}

// f64_from_fastfield_u64 (src/aggregation/mod.rs:351-383; common/src/lib.rs:108-114 u64_to_f64)
__device__ __forceinline__ double as_f64(uint64_t v, uint32_t value_type) {
  const uint64_t high = 1ull << 63;
  if (value_type == AS_VALUE_I64) return (double)(int64_t)(v ^ high);
  if (value_type == AS_VALUE_F64) return __longlong_as_double((long long)((v & high) ? v ^ high : ~v));
  return (double)v;
}

// Rust's `f64 as i64`: saturating, NaN is 0 (a plain C++ cast is undefined out of range)
__device__ __forceinline__ int64_t as_sat_i64(double x) {
  if (x != x) return 0;
  if (x >= 9223372036854775808.0) return INT64_MAX;
  if (x <= -9223372036854775808.0) return INT64_MIN;
  return (int64_t)x;
}

__device__ __forceinline__ unsigned long long as_wave_sum64(unsigned long long v) {
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  return v;
}

// *sum_lo / *sum_hi (128 bits) += lo + hi * 2^32 (lo, hi < 2^63), low word first: a wrapped add carries into the high word;
// the number of wraps does not depend on the order of the adders
__device__ __forceinline__ void as_add128(unsigned long long *sum_lo, unsigned long long *sum_hi, unsigned long long lo,
                                          unsigned long long hi) {
  const unsigned long long add_lo = lo + (hi << 32);
  const unsigned long long add_hi = (hi >> 32) + (add_lo < lo ? 1ull : 0ull);
  const unsigned long long old = atomicAdd(sum_lo, add_lo);
  const unsigned long long carry = old + add_lo < old ? 1ull : 0ull;
  if (add_hi + carry) atomicAdd(sum_hi, add_hi + carry);
}

template <bool OPTIONAL_A, bool OPTIONAL_B, uint32_t CAP>
__global__ __launch_bounds__(AS_THREADS) void agg_sub_kernel(TqkAggSubParams p) {
  __shared__ uint16_t slabs[AS_WAVES * AS_CHUNK_DOCS];
  // the table, one array per field: {doc count | value count << 32}, min, max, the sums of the low and of the high halves
  __shared__ unsigned long long t_cv[CAP], t_mn[CAP], t_mx[CAP], t_lo[CAP], t_hi[CAP];
  __shared__ unsigned long long part[AS_WAVES][AS_PART];
  const int lane = (int)__lane_id();
  const uint32_t wave = threadIdx.x >> 6;
  const uint32_t q = blockIdx.x % p.a.ds.n_queries, slice = blockIdx.x / p.a.ds.n_queries;
  const TqkDocsetQuery *Q = p.a.ds.queries + q;
  const DocsetHead h = docset_head(Q);
  uint16_t *const slab = slabs + wave * AS_CHUNK_DOCS;
  const uint64_t w0_64 = (uint64_t)slice * p.a.words_per_slice;
  const uint64_t w1_64 = w0_64 + p.a.words_per_slice;
  const uint32_t w0 = w0_64 < p.a.ds.n_words ? (uint32_t)w0_64 : p.a.ds.n_words;  // (a slice past the end: empty)
  const uint32_t w1 = w1_64 < p.a.ds.n_words ? (uint32_t)w1_64 : p.a.ds.n_words;
  const uint32_t n_buckets = p.a.n_buckets;
  const bool in_lds = n_buckets <= p.a.lds_buckets && n_buckets <= CAP;  // (uniform)
  const bool sum_b = p.value_type_b != AS_VALUE_F64;                      // (uniform; F64: both sum words stay 0)
  uint32_t *const row = p.a.buckets + (size_t)q * p.a.bucket_stride;
  TqkAggBucketStats *const recs = p.bucket_stats + (size_t)q * p.a.bucket_stride;
  if (in_lds) {
    for (uint32_t i = threadIdx.x; i < n_buckets; i += AS_THREADS) {
      t_cv[i] = 0ull;
      t_mn[i] = ~0ull;
      t_mx[i] = 0ull;
      t_lo[i] = 0ull;
      t_hi[i] = 0ull;
    }
    __syncthreads();
  }
  uint32_t cnt = 0, valued = 0, inb = 0, oor = 0, bucketed = 0, valued_b = 0;  // per lane
  uint64_t mn = ~0ull, mx = 0ull, s_lo = 0ull, s_hi = 0ull;
  for (uint32_t base = w0 + wave * AS_CHUNK_WORDS; base < w1; base += AS_WAVES * AS_CHUNK_WORDS) {
    const uint32_t w = base + (uint32_t)lane;
    uint32_t res = w < w1 ? docset_word(Q, h, p.a.ds, w) : 0u;
    const uint32_t pc = (uint32_t)__popc(res);
    cnt += pc;
    const uint32_t incl = wave_incl_sum(pc, lane);
    const uint32_t total = (uint32_t)__shfl(incl, 63, 64);  // <= AS_CHUNK_DOCS
    uint32_t at = incl - pc;
    while (res) {
      slab[at++] = (uint16_t)(((uint32_t)lane << 5) | (uint32_t)__builtin_ctz(res));
      res &= res - 1u;
    }
    wave_mem_fence();
    for (uint32_t j = 0; j < total; j += 64u) {
      const bool has = j + (uint32_t)lane < total;
      const uint32_t e = has ? slab[j + (uint32_t)lane] : 0u;
      const uint32_t doc = ((base + (e >> 5)) << 5) | (e & 31u);
      uint32_t r = 0;
      if (has && rg_row<OPTIONAL_A>(p.a.col, doc, r)) {
        const uint64_t v = as_value(p.a.col, p.a.min_value, p.a.gcd, r);
        ++valued;
        mn = v < mn ? v : mn;
        mx = v > mx ? v : mx;
        s_lo += v & 0xFFFFFFFFull;
        s_hi += v >> 32;
        const double val = as_f64(v, p.a.value_type);
        if (p.a.bounds_min <= val && val <= p.a.bounds_max) {  // (HistogramBounds::contains: never true for NaN, +-inf)
          ++inb;
          const int64_t pos = as_sat_i64(floor((val - p.a.offset) / p.a.interval));
          const uint64_t idx64 = (uint64_t)pos - (uint64_t)p.a.base_pos;  // (a pos below base_pos wraps to a huge index)
          if (idx64 < (uint64_t)n_buckets) {
            const uint32_t idx = (uint32_t)idx64;
            ++bucketed;
            uint32_t rb = 0;
            const bool has_b = rg_row<OPTIONAL_B>(p.col_b, doc, rb);
            const uint64_t vb = has_b ? as_value(p.col_b, p.min_value_b, p.gcd_b, rb) : 0ull;
            valued_b += has_b ? 1u : 0u;
            if (in_lds) {
              atomicAdd(&t_cv[idx], has_b ? 0x100000001ull : 1ull);
              if (has_b) {
                atomicMin(&t_mn[idx], (unsigned long long)vb);
                atomicMax(&t_mx[idx], (unsigned long long)vb);
                if (sum_b) {
                  atomicAdd(&t_lo[idx], (unsigned long long)(vb & 0xFFFFFFFFull));
                  atomicAdd(&t_hi[idx], (unsigned long long)(vb >> 32));
                }
              }
            } else {
              atomicAdd(row + idx, 1u);
              if (has_b) {
                TqkAggBucketStats *const R = recs + idx;
                atomicAdd(&R->count, 1ull);
                atomicMin(&R->min_value, (unsigned long long)vb);
                atomicMax(&R->max_value, (unsigned long long)vb);
                if (sum_b) as_add128(&R->sum_lo, &R->sum_hi, vb & 0xFFFFFFFFull, vb >> 32);
              }
            }
          } else {
            ++oor;
          }
        }
      }
    }
    wave_mem_fence();  // (the next chunk's expansion writes the slab again)
  }
  // the wavefront's part, then the workgroup's
  unsigned long long t_cnt = as_wave_sum64(cnt), t_val = as_wave_sum64(valued), s0 = as_wave_sum64(s_lo), s1 = as_wave_sum64(s_hi);
  unsigned long long t_inb = as_wave_sum64(inb), t_oor = as_wave_sum64(oor);
  unsigned long long t_bkt = as_wave_sum64(bucketed), t_vb = as_wave_sum64(valued_b);
  for (int off = 32; off > 0; off >>= 1) {
    const uint64_t a = __shfl_down(mn, off, 64), b = __shfl_down(mx, off, 64);
    mn = a < mn ? a : mn;
    mx = b > mx ? b : mx;
  }
  if (lane == 0) {
    part[wave][0] = t_cnt;
    part[wave][1] = t_val;
    part[wave][2] = mn;
    part[wave][3] = mx;
    part[wave][4] = s0;
    part[wave][5] = s1;
    part[wave][6] = t_inb;
    part[wave][7] = t_oor;
    part[wave][8] = t_bkt;
    part[wave][9] = t_vb;
  }
  __syncthreads();  // (also: every wavefront's LDS table updates are done)
  if (in_lds) {
    for (uint32_t i = threadIdx.x; i < n_buckets; i += AS_THREADS) {
      const unsigned long long cv = t_cv[i];
      const uint32_t docs = (uint32_t)cv;
      const unsigned long long vals = cv >> 32;
      if (docs) atomicAdd(row + i, docs);
      if (vals) {
        TqkAggBucketStats *const R = recs + i;
        atomicAdd(&R->count, vals);
        atomicMin(&R->min_value, t_mn[i]);
        atomicMax(&R->max_value, t_mx[i]);
        if (sum_b) as_add128(&R->sum_lo, &R->sum_hi, t_lo[i], t_hi[i]);
      }
    }
  }
  if (threadIdx.x != 0u) return;
  unsigned long long matches = 0, count = 0, lo = 0, hi = 0, in_bounds = 0, out_of_range = 0, in_buckets = 0, with_b = 0;
  uint64_t wmn = ~0ull, wmx = 0ull;
  for (uint32_t v = 0; v < AS_WAVES; ++v) {
    matches += part[v][0];
    count += part[v][1];
    wmn = part[v][2] < wmn ? part[v][2] : wmn;
    wmx = part[v][3] > wmx ? part[v][3] : wmx;
    lo += part[v][4];
    hi += part[v][5];
    in_bounds += part[v][6];
    out_of_range += part[v][7];
    in_buckets += part[v][8];
    with_b += part[v][9];
  }
  if (matches == 0ull) return;  // (nothing to add: an empty slice, or a query without a match in it)
  TqkAggStats *const S = p.a.stats + q;
  atomicAdd(&S->matches, matches);
  atomicAdd(p.a.query_sizes + q, (uint32_t)matches);
  atomicAdd(p.a.totals + 0, matches);
  if (count == 0ull) return;
  atomicAdd(p.a.totals + 1, count);
  atomicAdd(&S->count, count);
  atomicMin(&S->min_value, (unsigned long long)wmn);
  atomicMax(&S->max_value, (unsigned long long)wmx);
  if (p.a.value_type != AS_VALUE_F64) as_add128(&S->sum_lo, &S->sum_hi, lo, hi);
  if (in_bounds) atomicAdd(&S->in_bounds, in_bounds);
  if (out_of_range) atomicAdd(&S->out_of_range, out_of_range);
  if (with_b) atomicAdd(p.a.totals + 3, with_b);
  if (in_buckets) atomicAdd(p.a.totals + 4, in_buckets);
}

// bucket record i < n_buckets of query q = zeros with min_value = ~0.  grid = n_queries
__global__ __launch_bounds__(AS_THREADS) void agg_sub_init_kernel(TqkAggBucketStats *bucket_stats, uint32_t n_buckets,
                                                                  uint32_t bucket_stride) {
  unsigned long long *const words = reinterpret_cast<unsigned long long *>(bucket_stats + (size_t)blockIdx.x * bucket_stride);
  for (uint32_t w = threadIdx.x; w < n_buckets * 5u; w += AS_THREADS) words[w] = w % 5u == 1u ? ~0ull : 0ull;
}

template <uint32_t CAP>
void agg_sub_launch(const TqkAggSubParams &p, hipStream_t st) {
  const dim3 grid(p.a.ds.n_queries * p.a.n_slices), block(AS_THREADS);
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
  agg_sub_init_kernel<<<dim3(n_queries), dim3(AS_THREADS), 0, st>>>(bucket_stats, n_buckets, bucket_stride);
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
