// tq_agg_terms_sub.hip — terms aggregation with a metric (tq_agg_terms_sub_batch*): per key of a column A its doc count and
// a stats record of a metric column B, and the top `segment_size` entries by doc count, by key, or by one metric of the
// record (src/aggregation/bucket/term_agg/mod.rs:836-899 SegmentTermCollector::collect with a sub-aggregation, :1040-1111
// the order by a sub-aggregation and cut_off_buckets; src/aggregation/metric/stats.rs:282-306, :325-357).  Joins the integer
// key index and the exact selection of tq_agg_terms.hip with the 40-byte record and its LDS table of tq_agg_sub.hip.
//
// count    workgroup = (query, slice of the bitmap words).  Assembled from the shared walk (docset_walk,
//          tq_docset_walk.hpp), col_key_index / col_value and the bucket-record table (BucketTable: tq_agg_device.hpp).
//          Its own: a counted doc — a value in A, its index inside [0, n_keys) — takes rg_row + col_value of B (a doc that
//          is not counted, or has no value in B, loads nothing of B) and adds to the key's entry of the workgroup's LDS
//          table (n_keys <= min(lds_buckets, CAP); a SMALL and a LARGE table), flushed once, or, above the capacity, to
//          the query's count row and record row in global memory.
// select   one workgroup per query, once behind the last sub-batch: the shared selection (terms_select,
//          tq_agg_terms_select.hpp) under a key policy of up to 113 bits held as two 64-bit words.  The count and key
//          orders use terms_key64.  The metric orders: (image, or its complement for ASC) << 17 | (0x1FFFF - idx), the
//          image of tq_agg_metric_image.hpp — unique per entry, so nothing ties, and ties of the metric go to the
//          ascending key.  The radix select walks the image's width (32 / 64 / 96) plus the 17 index bits; the survivors'
//          records are written beside key and doc count.
// init     the records (zeros), the count rows (zeros) and the record rows (bucket_records_init), [0, n_keys) each.
// Integer arithmetic and integer atomics only: deterministic.  Plain vector stores and vector atomics; nothing is written at
// or past n_keys of a scratch row, nor at or past n_returned of an output row.  HBM model: tq_agg_terms.hip's + 8 per
// counted doc with a value in B + 8 per counted doc of an Optional B (its presence word) + 40 x n_keys per query + 40 per
// entry returned.
#include <algorithm>

#include "tq_agg_device.hpp"
#include "tq_agg_metric_image.hpp"
#include "tq_agg_terms_select.hpp"
#include "tq_column_read.hpp"
#include "tq_common.hpp"
#include "tq_docset_walk.hpp"
#include "tq_launch.h"

namespace {

// the LDS table: 40 bytes per key beside the slabs' 16 KB.  The capacities are agg_sub_kernel's (same
// entry size), carried over and not measured for this kernel
#ifndef TQ_AGG_TERMS_SUB_LDS_LARGE
#define TQ_AGG_TERMS_SUB_LDS_LARGE 1024
#endif
#ifndef TQ_AGG_TERMS_SUB_LDS_SMALL
#define TQ_AGG_TERMS_SUB_LDS_SMALL 128
#endif
// the instantiation the global path runs in, by its table's capacity: it never touches the table, which only sets the
// wavefronts per SIMD — and fewer of them was faster wherever the atomics on the rows are the bound
#ifndef TQ_AGG_TERMS_SUB_GLOBAL_TABLE
#define TQ_AGG_TERMS_SUB_GLOBAL_TABLE TQ_AGG_TERMS_SUB_LDS_LARGE
#endif
constexpr uint32_t TS_GLOBAL_TABLE = TQ_AGG_TERMS_SUB_GLOBAL_TABLE;
static_assert(TS_GLOBAL_TABLE == TQ_AGG_TERMS_SUB_LDS_LARGE || TS_GLOBAL_TABLE == TQ_AGG_TERMS_SUB_LDS_SMALL, "one of the two tables");
constexpr uint32_t TS_LDS_LARGE = TQ_AGG_TERMS_SUB_LDS_LARGE;
constexpr uint32_t TS_LDS_SMALL = TQ_AGG_TERMS_SUB_LDS_SMALL;
constexpr uint32_t TS_PART = 5;  // words of a wavefront's part
static_assert(TS_LDS_SMALL >= 1u && TS_LDS_SMALL <= TS_LDS_LARGE, "two tables");
static_assert(TS_LDS_LARGE * 40u + WALK_SLAB_ENTRIES * 2u + WALK_WAVES * TS_PART * 8u <= 65536u, "the static LDS of a workgroup");
constexpr uint32_t TS_METRIC_DESC = 4, TS_METRIC_ASC = 5;  // TQ_TERMS_*, behind TERMS_KEY_DESC

template <bool OPTIONAL_A, bool OPTIONAL_B, uint32_t CAP>
__global__ __launch_bounds__(WALK_THREADS) void agg_terms_sub_count_kernel(TqkAggTermsSubParams p) {
  __shared__ uint16_t slabs[WALK_SLAB_ENTRIES];
  __shared__ unsigned long long t_cv[CAP], t_mn[CAP], t_mx[CAP], t_lo[CAP], t_hi[CAP];  // BucketTable's fields
  __shared__ unsigned long long part[WALK_WAVES][TS_PART];
  const BucketTable table{t_cv, t_mn, t_mx, t_lo, t_hi};
  const int lane = (int)__lane_id();
  const uint32_t wave = threadIdx.x >> 6;
  const uint32_t q = blockIdx.x % p.t.ds.n_queries, slice = blockIdx.x / p.t.ds.n_queries;
  const uint32_t n_keys = p.t.n_keys;
  const bool in_lds = n_keys <= p.t.lds_buckets && n_keys <= CAP;  // (uniform)
  const bool sum_b = p.value_type_b != TQ_IMG_F64;                  // (uniform; F64: both sum words stay 0)
  uint32_t *const row = p.t.rows + (size_t)q * n_keys;
  TqkAggBucketStats *const recs = p.stats + (size_t)q * n_keys;
  if (in_lds) {
    table.zero(n_keys);
    __syncthreads();
  }
  uint32_t valued = 0, oor = 0, counted = 0, valued_b = 0;  // per lane
  const uint32_t cnt = docset_walk(p.t.ds, p.t.ds.queries + q, slice, p.t.words_per_slice, slabs, wave, lane, [&](bool has, uint32_t doc) {
    uint32_t r = 0;
    if (!(has && rg_row<OPTIONAL_A>(p.t.col, doc, r))) return;
    ++valued;
    const uint64_t idx64 = col_key_index(p.t.col, p.t.min_value, p.t.gcd, r);
    if (idx64 >= (uint64_t)n_keys) {
      ++oor;
      return;
    }
    const uint32_t idx = (uint32_t)idx64;
    ++counted;
    uint32_t rb = 0;
    const bool has_b = rg_row<OPTIONAL_B>(p.col_b, doc, rb);
    const uint64_t vb = has_b ? col_value(p.col_b, p.min_value_b, p.gcd_b, rb) : 0ull;
    valued_b += has_b ? 1u : 0u;
    if (in_lds)
      table.add(idx, has_b, vb, sum_b);
    else
      BucketTable::add_global(row, recs, idx, has_b, vb, sum_b);
  });
  // the wavefront's part, then the workgroup's
  const unsigned long long t_cnt = wave_sum64(cnt), t_val = wave_sum64(valued), t_oor = wave_sum64(oor);
  const unsigned long long t_ctd = wave_sum64(counted), t_vb = wave_sum64(valued_b);
  if (lane == 0) {
    part[wave][0] = t_cnt;
    part[wave][1] = t_val;
    part[wave][2] = t_oor;
    part[wave][3] = t_ctd;
    part[wave][4] = t_vb;
  }
  __syncthreads();  // (also: every wavefront's LDS table updates are done)
  if (in_lds) table.flush(n_keys, row, recs, sum_b);
  if (threadIdx.x != 0u) return;
  unsigned long long matches = 0, count = 0, out_of_range = 0, in_keys = 0, with_b = 0;
  for (uint32_t v = 0; v < WALK_WAVES; ++v) {
    matches += part[v][0];
    count += part[v][1];
    out_of_range += part[v][2];
    in_keys += part[v][3];
    with_b += part[v][4];
  }
  if (matches == 0ull) return;  // (nothing to add: an empty slice, or a query without a match in it)
  TqkAggTerms *const R = p.t.records + q;
  atomicAdd(&R->matches, matches);
  atomicAdd(p.t.query_sizes + q, (uint32_t)matches);
  atomicAdd(p.t.totals + 0, matches);
  if (count == 0ull) return;
  atomicAdd(p.t.totals + 1, count);
  atomicAdd(&R->count, count);
  if (out_of_range) atomicAdd(&R->out_of_range, (uint32_t)out_of_range);
  if (with_b) atomicAdd(p.t.totals + 4, with_b);
  if (in_keys) atomicAdd(p.t.totals + 5, in_keys);
}

// ---- the selection's key (tq_agg_terms_select.hpp).  128 bits: never 0, unique per entry, the order's first entry the largest.
struct TsKey {
  unsigned long long hi, lo;
};
__device__ __forceinline__ bool operator<(const TsKey &a, const TsKey &b) { return a.hi < b.hi || (a.hi == b.hi && a.lo < b.lo); }
__device__ __forceinline__ bool operator==(const TsKey &a, const TsKey &b) { return a.hi == b.hi && a.lo == b.lo; }
__device__ __forceinline__ TsKey operator&(const TsKey &a, const TsKey &b) { return TsKey{a.hi & b.hi, a.lo & b.lo}; }
__device__ __forceinline__ TsKey operator|(const TsKey &a, const TsKey &b) { return TsKey{a.hi | b.hi, a.lo | b.lo}; }

// the key policy: the count and key orders use terms_key64 in the low word; a metric order reads the entry's record
struct TermsKey128 {
  using Key = TsKey;
  static constexpr uint32_t WORDS = 2;
  uint32_t order, metric, value_type;
  const TqkAggBucketStats *recs;  // the query's record row
  TqkAggBucketStats *out_stats;
  // entry idx (< TERMS_MAX_KEYS) with doc count c (1 .. 2^31 - 1)
  __device__ __forceinline__ Key make(uint32_t idx, uint32_t c) const {
    if (order <= TERMS_KEY_DESC) return TsKey{0ull, terms_key64(order, idx, c)};
    const TqkAggBucketStats *const R = recs + idx;
    TqImage im = tq_metric_image(R->count, R->min_value, R->max_value, R->sum_lo, R->sum_hi, value_type, metric);
    if (order == TS_METRIC_ASC) {  // the complement inside the image's width: the smallest image the largest key
      const uint32_t bits = tq_image_bits(metric);
      im.lo = bits == 32u ? 0xFFFFFFFFull - im.lo : ~im.lo;
      im.hi = bits == 96u ? 0xFFFFFFFFull - im.hi : 0ull;
    }
    return TsKey{(im.hi << 17) | (im.lo >> 47), (im.lo << 17) | (0x1FFFFull - idx)};  // ties of the metric: ascending key
  }
  __device__ __forceinline__ uint32_t idx(const Key &k) const { return terms_idx(order, k.lo); }
  // the key's bits, rounded up to whole digits: 48 / 24 for the old orders, the image's width + 17 for a metric order
  __device__ __forceinline__ int top_shift() const {
    return order <= TERMS_COUNT_ASC ? 40 : order <= TERMS_KEY_DESC ? 16 : (int)((tq_image_bits(metric) + 17u + 7u) & ~7u) - 8;
  }
  __device__ static __forceinline__ Key at(uint32_t v, int shift) {
    return shift >= 64 ? TsKey{(unsigned long long)v << (shift - 64), 0ull} : TsKey{0ull, (unsigned long long)v << shift};
  }
  __device__ static __forceinline__ uint32_t digit(const Key &k, int shift) {
    return (uint32_t)(shift >= 64 ? k.hi >> (shift - 64) : k.lo >> shift) & 255u;
  }
  template <uint32_t N>
  __device__ static __forceinline__ Key get(const unsigned long long (&a)[2][N], uint32_t i) { return TsKey{a[0][i], a[1][i]}; }
  template <uint32_t N>
  __device__ static __forceinline__ void put(unsigned long long (&a)[2][N], uint32_t i, const Key &k) {
    a[0][i] = k.hi;
    a[1][i] = k.lo;
  }
  __device__ static __forceinline__ Key shfl_down(const Key &k, int off) { return TsKey{__shfl_down(k.hi, off, 64), __shfl_down(k.lo, off, 64)}; }
  __device__ __forceinline__ void write(size_t o, uint32_t idx) const { out_stats[o] = recs[idx]; }
};

// grid = n_queries
__global__ __launch_bounds__(TSEL_THREADS) void agg_terms_sub_select_kernel(TqkAggTermsSubSelectParams p) {
  const size_t row0 = (size_t)blockIdx.x * p.s.n_keys;
  terms_select(p.s, TermsKey128{p.s.order, p.metric, p.value_type_b, p.stats + row0, p.out_stats});
}

// record q = zeros; entries [0, n_keys) of count row q = 0, of record row q = zeros with min_value = ~0.  grid = n_queries
__global__ __launch_bounds__(WALK_THREADS) void agg_terms_sub_init_kernel(TqkAggTerms *records, uint32_t *rows, TqkAggBucketStats *stats,
                                                                        uint32_t n_keys) {
  const uint32_t q = blockIdx.x;
  if (threadIdx.x < 5u) reinterpret_cast<unsigned long long *>(records + q)[threadIdx.x] = 0ull;
  uint32_t *const row = rows + (size_t)q * n_keys;
  for (uint32_t i = threadIdx.x; i < n_keys; i += WALK_THREADS) row[i] = 0u;
  bucket_records_init(stats + (size_t)q * n_keys, n_keys);
}

template <uint32_t CAP>
void agg_terms_sub_launch(const TqkAggTermsSubParams &p, hipStream_t st) {
  const dim3 grid(p.t.ds.n_queries * p.t.n_slices), block(WALK_THREADS);
  if (p.t.col.present) {
    if (p.col_b.present)
      agg_terms_sub_count_kernel<true, true, CAP><<<grid, block, 0, st>>>(p);
    else
      agg_terms_sub_count_kernel<true, false, CAP><<<grid, block, 0, st>>>(p);
  } else {
    if (p.col_b.present)
      agg_terms_sub_count_kernel<false, true, CAP><<<grid, block, 0, st>>>(p);
    else
      agg_terms_sub_count_kernel<false, false, CAP><<<grid, block, 0, st>>>(p);
  }
}

}  // namespace

static_assert(sizeof(TqkAggTerms) == 40 && sizeof(TqkAggBucketStats) == 40, "five 64-bit words each: agg_terms_sub_init_kernel");

void tqk_agg_terms_sub_lds_capacities(uint32_t out[2]) {
  out[0] = TS_LDS_SMALL;
  out[1] = TS_LDS_LARGE;
}

hipError_t tqk_launch_agg_terms_sub_init(TqkAggTerms *records, uint32_t *rows, TqkAggBucketStats *stats, uint32_t n_queries,
                                         uint32_t n_keys, hipStream_t st) {
  if (!n_queries) return hipSuccess;
  if (!records || (n_keys && (!rows || !stats)) || n_keys > TERMS_MAX_KEYS) return hipErrorInvalidValue;
  agg_terms_sub_init_kernel<<<dim3(n_queries), dim3(WALK_THREADS), 0, st>>>(records, rows, stats, n_keys);
  return hipGetLastError();
}

hipError_t tqk_launch_agg_terms_sub_count(const TqkAggTermsSubParams &p, hipStream_t st) {
  if (!p.t.ds.n_queries || !p.t.n_slices) return hipSuccess;
  if (p.t.col.codec > TQK_COL_BLOCKWISE || p.col_b.codec > TQK_COL_BLOCKWISE || p.t.gcd == 0ull) return hipErrorInvalidValue;
  if (p.t.n_keys > TERMS_MAX_KEYS || (p.t.n_keys && (!p.t.rows || !p.stats)) || !p.t.records) return hipErrorInvalidValue;
  const bool global = p.t.n_keys > std::min(p.t.lds_buckets, TS_LDS_LARGE);  // past "agg_lds_buckets" or the large table: straight to the rows
  if (global ? TS_GLOBAL_TABLE == TS_LDS_SMALL : p.t.n_keys <= TS_LDS_SMALL)
    agg_terms_sub_launch<TS_LDS_SMALL>(p, st);
  else
    agg_terms_sub_launch<TS_LDS_LARGE>(p, st);
  return hipGetLastError();
}

hipError_t tqk_launch_agg_terms_sub_select(const TqkAggTermsSubSelectParams &p, hipStream_t st) {
  if (!p.s.n_queries) return hipSuccess;
  if (p.s.n_keys > TERMS_MAX_KEYS || (p.s.n_keys && (!p.s.rows || !p.stats)) || !p.s.records) return hipErrorInvalidValue;
  if (p.s.order > TS_METRIC_ASC || p.value_type_b > TQ_IMG_F64) return hipErrorInvalidValue;
  if (p.s.order >= TS_METRIC_DESC && (p.metric > TQ_IMG_AVG || (p.metric >= TQ_IMG_SUM && p.value_type_b == TQ_IMG_F64))) return hipErrorInvalidValue;
  if (p.s.segment_size == 0u || p.s.segment_size > TERMS_MAX_SIZE) return hipErrorInvalidValue;
  if (p.s.out_stride < std::min(p.s.segment_size, p.s.n_keys) || (p.s.n_keys && (!p.s.out_keys || !p.s.out_counts || !p.out_stats)))
    return hipErrorInvalidValue;
  agg_terms_sub_select_kernel<<<dim3(p.s.n_queries), dim3(TSEL_THREADS), 0, st>>>(p);
  return hipGetLastError();
}
