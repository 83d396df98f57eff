// tq_agg.hip — aggregations over a fast field (tq_agg_batch*): what a stats metric (src/aggregation/metric/stats.rs:86-176,
// IntermediateStats::collect) and a histogram bucket aggregation (src/aggregation/bucket/histogram/histogram.rs:468-518
// collect, :738-741 get_bucket_pos_f64; src/aggregation/mod.rs:351-383 f64_from_fastfield_u64) leave of a segment, for
// every query of a batch in ONE pass over its match bits.  No doc set is written: the match bits (docset_word,
// tq_docset_word.hpp) and the column readers (rg_row / rg_value, tq_column_read.hpp) meet as in tq_sort.hip, with
// accumulators in place of the top-k heap.
//
// agg      workgroup = (query, slice of the bitmap words), query fastest in the grid; four wavefronts, each walking every
//          fourth 64-word chunk of the slice on its own (tq_sort.hip's walk, its own copy):
//            1. a lane evaluates one word (docset_word), the popcounts are prefix-summed over the wavefront
//            2. every lane expands its word's bits into the wavefront's LDS slab (13 bits per doc: word of the chunk, bit)
//            3. the slab is read back 64 docs at a time — a lane per matching doc — rg_row + rg_value per doc (a doc
//               without a value loads nothing)
//            4. per lane: min, max and count of the u64-space values, and their sum as TWO u64 accumulators of the
//               values' 32-bit halves (a segment has fewer than 2^31 docs: neither can overflow, no carries in the loop);
//               histogram: val = the value as the reference's f64, the contains test, pos = floor((val - offset) /
//               interval) saturated to i64, one atomic add on bucket pos - base_pos — of the workgroup's LDS table
//               (n_buckets <= lds_buckets; a table of 2 048 or of 8 192 buckets, two instantiations) or of the query's row
//          then shuffles reduce a wavefront, LDS the four wavefronts, and ONE lane adds the workgroup's part to the query's
//          64-byte record with vector atomics (add / min / max; the 128-bit sum: add the low word, carry into the high
//          one where the add wrapped — the number of wraps does not depend on the order).  The LDS table is flushed with
//          one atomic add per non-zero bucket.  Integer atomics are order-free: the result is deterministic.
// init     the records (zeros, min_value = ~0) and entries [0, n_buckets) of every row, in front of the launch.
// Plain vector stores and vector atomics only; nothing is written at or past a row's n_buckets: a doc whose bucket is
// outside [0, n_buckets) — none, by the monotonicity of the dense range — is counted in out_of_range and dropped.
// HBM model: lists x bitmap words x 4 + 8 per matching doc with a value + 8 per matching doc of an Optional column
// (its presence word) + 64 + 4 x n_buckets per query.
#include <algorithm>

#include "tq_column_read.hpp"
#include "tq_common.hpp"
#include "tq_docset_word.hpp"
#include "tq_launch.h"

namespace {

constexpr uint32_t AG_THREADS = 256;
constexpr uint32_t AG_WAVES = AG_THREADS / 64;
constexpr uint32_t AG_CHUNK_WORDS = 64;                  // one word per lane
constexpr uint32_t AG_CHUNK_DOCS = AG_CHUNK_WORDS * 32;  // slab entries per wavefront
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
constexpr uint32_t AG_VALUE_I64 = 1, AG_VALUE_F64 = 2;   // TQ_VALUE_* (U64 = 0)

__device__ __forceinline__ uint64_t agg_value(const TqkAggParams &p, uint32_t row) {
  const uint32_t codec = p.col.codec;  // (uniform)
  if (codec == TQK_COL_LINEAR) return rg_value<TQK_COL_LINEAR>(p.col, row);
  const uint64_t n = codec == TQK_COL_BITPACKED ? rg_value<TQK_COL_BITPACKED>(p.col, row) : rg_value<TQK_COL_BLOCKWISE>(p.col, row);
  return p.min_value + p.gcd * n;
}

// f64_from_fastfield_u64 (src/aggregation/mod.rs:351-383; common/src/lib.rs:108-114 u64_to_f64)
__device__ __forceinline__ double agg_f64(uint64_t v, uint32_t value_type) {
  const uint64_t high = 1ull << 63;
  if (value_type == AG_VALUE_I64) return (double)(int64_t)(v ^ high);
  if (value_type == AG_VALUE_F64) return __longlong_as_double((long long)((v & high) ? v ^ high : ~v));
  return (double)v;
}

// Rust's `f64 as i64`: saturating, NaN is 0 (a plain C++ cast is undefined out of range)
__device__ __forceinline__ int64_t agg_sat_i64(double x) {
  if (x != x) return 0;
  if (x >= 9223372036854775808.0) return INT64_MAX;
  if (x <= -9223372036854775808.0) return INT64_MIN;
  return (int64_t)x;
}

__device__ __forceinline__ unsigned long long wave_sum64(unsigned long long v) {
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  return v;
}

template <bool OPTIONAL, uint32_t CAP>
__global__ __launch_bounds__(AG_THREADS) void agg_kernel(TqkAggParams p) {
  constexpr bool HIST = CAP != 0u;
  __shared__ uint16_t slabs[AG_WAVES * AG_CHUNK_DOCS];
  __shared__ uint32_t hist[HIST ? CAP : 1u];
  __shared__ unsigned long long part[AG_WAVES][8];
  const int lane = (int)__lane_id();
  const uint32_t wave = threadIdx.x >> 6;
  const uint32_t q = blockIdx.x % p.ds.n_queries, slice = blockIdx.x / p.ds.n_queries;
  const TqkDocsetQuery *Q = p.ds.queries + q;
  const DocsetHead h = docset_head(Q);
  uint16_t *const slab = slabs + wave * AG_CHUNK_DOCS;
  const uint64_t w0_64 = (uint64_t)slice * p.words_per_slice;
  const uint64_t w1_64 = w0_64 + p.words_per_slice;
  const uint32_t w0 = w0_64 < p.ds.n_words ? (uint32_t)w0_64 : p.ds.n_words;  // (a slice past the end: empty)
  const uint32_t w1 = w1_64 < p.ds.n_words ? (uint32_t)w1_64 : p.ds.n_words;
  const uint32_t n_buckets = HIST ? p.n_buckets : 0u;
  const bool in_lds = HIST && n_buckets <= p.lds_buckets && n_buckets <= CAP;  // (uniform)
  uint32_t *const row = HIST ? p.buckets + (size_t)q * p.bucket_stride : nullptr;
  if (HIST && in_lds) {
    for (uint32_t i = threadIdx.x; i < n_buckets; i += AG_THREADS) hist[i] = 0u;
    __syncthreads();
  }
  uint32_t cnt = 0, valued = 0, inb = 0, oor = 0;  // per lane
  uint64_t mn = ~0ull, mx = 0ull, s_lo = 0ull, s_hi = 0ull;
  for (uint32_t base = w0 + wave * AG_CHUNK_WORDS; base < w1; base += AG_WAVES * AG_CHUNK_WORDS) {
    const uint32_t w = base + (uint32_t)lane;
    uint32_t res = w < w1 ? docset_word(Q, h, p.ds, w) : 0u;
    const uint32_t pc = (uint32_t)__popc(res);
    cnt += pc;
    const uint32_t incl = wave_incl_sum(pc, lane);
    const uint32_t total = (uint32_t)__shfl(incl, 63, 64);  // <= AG_CHUNK_DOCS
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
      if (has && rg_row<OPTIONAL>(p.col, doc, r)) {
        const uint64_t v = agg_value(p, r);
        ++valued;
        mn = v < mn ? v : mn;
        mx = v > mx ? v : mx;
        s_lo += v & 0xFFFFFFFFull;
        s_hi += v >> 32;
        if (HIST) {
          const double val = agg_f64(v, p.value_type);
          if (p.bounds_min <= val && val <= p.bounds_max) {  // (HistogramBounds::contains: never true for NaN, +-inf)
            ++inb;
            const int64_t pos = agg_sat_i64(floor((val - p.offset) / p.interval));
            const uint64_t idx = (uint64_t)pos - (uint64_t)p.base_pos;  // (a pos below base_pos wraps to a huge index)
            if (idx < (uint64_t)n_buckets) {
              if (in_lds)
                atomicAdd(&hist[(uint32_t)idx], 1u);
              else
                atomicAdd(row + (uint32_t)idx, 1u);
            } else {
              ++oor;
            }
          }
        }
      }
    }
    wave_mem_fence();  // (the next chunk's expansion writes the slab again)
  }
  // the wavefront's part, then the workgroup's
  unsigned long long t_cnt = wave_sum64(cnt), t_val = wave_sum64(valued), t_lo = wave_sum64(s_lo), t_hi = wave_sum64(s_hi);
  unsigned long long t_inb = wave_sum64(inb), t_oor = wave_sum64(oor);
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
    part[wave][4] = t_lo;
    part[wave][5] = t_hi;
    part[wave][6] = t_inb;
    part[wave][7] = t_oor;
  }
  __syncthreads();  // (also: every wavefront's LDS bucket adds are done)
  if (HIST && in_lds) {
    for (uint32_t i = threadIdx.x; i < n_buckets; i += AG_THREADS) {
      const uint32_t c = hist[i];
      if (c) atomicAdd(row + i, c);
    }
  }
  if (threadIdx.x != 0u) return;
  unsigned long long matches = 0, count = 0, lo = 0, hi = 0, in_bounds = 0, out_of_range = 0;
  uint64_t wmn = ~0ull, wmx = 0ull;
  for (uint32_t v = 0; v < AG_WAVES; ++v) {
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
  // sum = lo + hi * 2^32 as 128 bits (lo, hi < 2^63), added low word first: a wrapped add carries into the high word
  // (an F64 column: a sum in u64 space means nothing, both words stay 0)
  if (p.value_type != AG_VALUE_F64) {
    const unsigned long long add_lo = lo + (hi << 32);
    const unsigned long long add_hi = (hi >> 32) + (add_lo < lo ? 1ull : 0ull);
    const unsigned long long old = atomicAdd(&S->sum_lo, add_lo);
    const unsigned long long carry = old + add_lo < old ? 1ull : 0ull;
    if (add_hi + carry) atomicAdd(&S->sum_hi, add_hi + carry);
  }
  if (HIST) {
    if (in_bounds) atomicAdd(&S->in_bounds, in_bounds);
    if (out_of_range) atomicAdd(&S->out_of_range, out_of_range);
  }
}

// record q = zeros with min_value = ~0; entries [0, n_buckets) of row q = 0.  grid = n_queries
__global__ __launch_bounds__(AG_THREADS) void agg_init_kernel(TqkAggStats *stats, uint32_t *buckets, uint32_t n_buckets,
                                                              uint32_t bucket_stride) {
  const uint32_t q = blockIdx.x;
  if (threadIdx.x < 8u)
    reinterpret_cast<unsigned long long *>(stats + q)[threadIdx.x] = threadIdx.x == 2u ? ~0ull : 0ull;
  uint32_t *const row = buckets + (size_t)q * bucket_stride;
  for (uint32_t i = threadIdx.x; i < n_buckets; i += AG_THREADS) row[i] = 0u;
}

template <uint32_t CAP>
void agg_launch(const TqkAggParams &p, hipStream_t st) {
  const dim3 grid(p.ds.n_queries * p.n_slices), block(AG_THREADS);
  if (p.col.present)
    agg_kernel<true, CAP><<<grid, block, 0, st>>>(p);
  else
    agg_kernel<false, CAP><<<grid, block, 0, st>>>(p);
}

}  // namespace

uint32_t tqk_agg_step_words() { return AG_WAVES * AG_CHUNK_WORDS; }
uint32_t tqk_agg_lds_buckets() { return AG_LDS_BUCKETS; }

hipError_t tqk_launch_agg_init(TqkAggStats *stats, uint32_t *buckets, uint32_t n_queries, uint32_t n_buckets,
                               uint32_t bucket_stride, hipStream_t st) {
  if (!n_queries) return hipSuccess;
  if (n_buckets > bucket_stride || (n_buckets && !buckets)) return hipErrorInvalidValue;
  agg_init_kernel<<<dim3(n_queries), dim3(AG_THREADS), 0, st>>>(stats, buckets, n_buckets, bucket_stride);
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
