// tq_agg_terms.hip — terms aggregation (tq_agg_terms_batch*): the top `segment_size` values of a fast-field column by doc
// count or by key, per query of a batch (src/aggregation/bucket/term_agg/mod.rs:836-899 SegmentTermCollector::collect,
// :1000-1111 into_intermediate_bucket_result, :1328-1353 cut_off_buckets).  The keys are exact integers: a value's index is
// (value - min) / gcd, the number the Bitpacked and BlockwiseLinear readers return as it stands; no f64 anywhere.
//
// count    workgroup = (query, slice of the bitmap words).  Assembled from the shared walk (docset_walk,
//          tq_docset_walk.hpp) and col_key_index (tq_agg_device.hpp).  Its own: a doc with a value adds one to its key's
//          entry of the workgroup's uint32 LDS table (n_keys <= min(lds_buckets, CAP); a table of 2 048 or of 8 192
//          entries, two instantiations), flushed with one vector atomic add per non-zero entry, or above the capacity to
//          the query's scratch row directly.  Per-lane matches / valued / out-of-range counts are reduced by shuffles and
//          LDS and published by one lane.
// select   one workgroup per query, once behind the last sub-batch: the shared selection (terms_select,
//          tq_agg_terms_select.hpp) under the 64-bit key policy — COUNT_DESC (count << 17) | (0x1FFFF - idx), COUNT_ASC
//          the same with 0x7FFFFFFF - count, KEY_ASC 0x1FFFF - idx, KEY_DESC idx + 1 (terms_key64).
// init     the records (zeros) and entries [0, n_keys) of every scratch row, in front of the first count launch.
// Plain vector stores and vector atomics only.  Nothing is written at or past n_keys of a scratch row (an index outside
// [0, n_keys) — none, by the column's own min / max / gcd — is counted in out_of_range and dropped), nor at or past
// n_returned of an output row.  HBM model: agg_kernel's bitmap-word and per-valued-doc terms + per query 4 x n_keys (the row
// the selection reads) + 12 x n_returned + the 40-byte record.
#include <algorithm>

#include "tq_agg_device.hpp"
#include "tq_agg_terms_select.hpp"
#include "tq_column_read.hpp"
#include "tq_common.hpp"
#include "tq_docset_walk.hpp"
#include "tq_launch.h"

namespace {

// the LDS table: 4 bytes per key beside the slabs' 16 KB, the capacities of agg_kernel's table carried
// over — same entry size, same walk
#ifndef TQ_AGG_TERMS_LDS_LARGE
#define TQ_AGG_TERMS_LDS_LARGE 8192
#endif
#ifndef TQ_AGG_TERMS_LDS_SMALL
#define TQ_AGG_TERMS_LDS_SMALL 2048
#endif
// the instantiation the global path runs in, by its table's capacity: it never touches the table, which only costs it
// wavefronts per SIMD
#ifndef TQ_AGG_TERMS_GLOBAL_TABLE
#define TQ_AGG_TERMS_GLOBAL_TABLE TQ_AGG_TERMS_LDS_LARGE
#endif
constexpr uint32_t AT_LDS_LARGE = TQ_AGG_TERMS_LDS_LARGE;
constexpr uint32_t AT_LDS_SMALL = TQ_AGG_TERMS_LDS_SMALL;
constexpr uint32_t AT_GLOBAL_TABLE = TQ_AGG_TERMS_GLOBAL_TABLE;
static_assert(AT_GLOBAL_TABLE >= 1u && AT_GLOBAL_TABLE <= AT_LDS_LARGE, "one of the tables, or a one-entry stub");
static_assert(AT_LDS_SMALL >= 1u && AT_LDS_SMALL <= AT_LDS_LARGE && AT_LDS_LARGE * 4u + 16640u <= 65536u, "the static LDS of a workgroup");

template <bool OPTIONAL, uint32_t CAP>
__global__ __launch_bounds__(WALK_THREADS) void agg_terms_count_kernel(TqkAggTermsParams p) {
  __shared__ uint16_t slabs[WALK_SLAB_ENTRIES];
  __shared__ uint32_t table[CAP];
  __shared__ unsigned long long part[WALK_WAVES][3];
  const int lane = (int)__lane_id();
  const uint32_t wave = threadIdx.x >> 6;
  const uint32_t q = blockIdx.x % p.ds.n_queries, slice = blockIdx.x / p.ds.n_queries;
  const uint32_t n_keys = p.n_keys;
  const bool in_lds = n_keys <= p.lds_buckets && n_keys <= CAP;  // (uniform)
  uint32_t *const row = p.rows + (size_t)q * n_keys;
  if (in_lds) {
    for (uint32_t i = threadIdx.x; i < n_keys; i += WALK_THREADS) table[i] = 0u;
    __syncthreads();
  }
  uint32_t valued = 0, oor = 0;  // per lane
  const uint32_t cnt = docset_walk(p.ds, p.ds.queries + q, slice, p.words_per_slice, slabs, wave, lane, [&](bool has, uint32_t doc) {
    uint32_t r = 0;
    if (!(has && rg_row<OPTIONAL>(p.col, doc, r))) return;
    ++valued;
    const uint64_t idx = col_key_index(p.col, p.min_value, p.gcd, r);
    if (idx >= (uint64_t)n_keys)
      ++oor;
    else if (in_lds)
      atomicAdd(&table[(uint32_t)idx], 1u);
    else
      atomicAdd(row + (uint32_t)idx, 1u);
  });
  // the wavefront's part, then the workgroup's
  const unsigned long long t_cnt = wave_sum64(cnt), t_val = wave_sum64(valued), t_oor = wave_sum64(oor);
  if (lane == 0) {
    part[wave][0] = t_cnt;
    part[wave][1] = t_val;
    part[wave][2] = t_oor;
  }
  __syncthreads();  // (also: every wavefront's LDS table adds are done)
  if (in_lds) {
    for (uint32_t i = threadIdx.x; i < n_keys; i += WALK_THREADS) {
      const uint32_t c = table[i];
      if (c) atomicAdd(row + i, c);
    }
  }
  if (threadIdx.x != 0u) return;
  unsigned long long matches = 0, count = 0, out_of_range = 0;
  for (uint32_t v = 0; v < WALK_WAVES; ++v) {
    matches += part[v][0];
    count += part[v][1];
    out_of_range += part[v][2];
  }
  if (matches == 0ull) return;  // (nothing to add: an empty slice, or a query without a match in it)
  TqkAggTerms *const R = p.records + q;
  atomicAdd(&R->matches, matches);
  atomicAdd(p.query_sizes + q, (uint32_t)matches);
  atomicAdd(p.totals + 0, matches);
  if (count == 0ull) return;
  atomicAdd(p.totals + 1, count);
  atomicAdd(&R->count, count);
  if (out_of_range) atomicAdd(&R->out_of_range, (uint32_t)out_of_range);
}

// the selection's key policy (tq_agg_terms_select.hpp): the 64-bit key of the count and key orders, no record row
struct TermsKey64 {
  using Key = unsigned long long;
  static constexpr uint32_t WORDS = 1;
  uint32_t order;
  __device__ __forceinline__ Key make(uint32_t idx, uint32_t c) const { return terms_key64(order, idx, c); }
  __device__ __forceinline__ uint32_t idx(Key k) const { return terms_idx(order, k); }
  __device__ __forceinline__ int top_shift() const { return order <= TERMS_COUNT_ASC ? 40 : 16; }  // 48 / 24 bits
  __device__ static __forceinline__ Key at(uint32_t v, int shift) { return (Key)v << shift; }
  __device__ static __forceinline__ uint32_t digit(Key k, int shift) { return (uint32_t)(k >> shift) & 255u; }
  template <uint32_t N>
  __device__ static __forceinline__ Key get(const unsigned long long (&a)[1][N], uint32_t i) { return a[0][i]; }
  template <uint32_t N>
  __device__ static __forceinline__ void put(unsigned long long (&a)[1][N], uint32_t i, Key k) { a[0][i] = k; }
  __device__ static __forceinline__ Key shfl_down(Key k, int off) { return __shfl_down(k, off, 64); }
  __device__ __forceinline__ void write(size_t, uint32_t) const {}
};

// grid = n_queries
__global__ __launch_bounds__(TSEL_THREADS) void agg_terms_select_kernel(TqkAggTermsSelectParams p) {
  terms_select(p, TermsKey64{p.order});
}

// record q = zeros; entries [0, n_keys) of scratch row q = 0.  grid = n_queries
__global__ __launch_bounds__(WALK_THREADS) void agg_terms_init_kernel(TqkAggTerms *records, uint32_t *rows, uint32_t n_keys) {
  const uint32_t q = blockIdx.x;
  if (threadIdx.x < 5u) reinterpret_cast<unsigned long long *>(records + q)[threadIdx.x] = 0ull;
  uint32_t *const row = rows + (size_t)q * n_keys;
  for (uint32_t i = threadIdx.x; i < n_keys; i += WALK_THREADS) row[i] = 0u;
}

template <uint32_t CAP>
void agg_terms_launch(const TqkAggTermsParams &p, hipStream_t st) {
  const dim3 grid(p.ds.n_queries * p.n_slices), block(WALK_THREADS);
  if (p.col.present)
    agg_terms_count_kernel<true, CAP><<<grid, block, 0, st>>>(p);
  else
    agg_terms_count_kernel<false, CAP><<<grid, block, 0, st>>>(p);
}

}  // namespace

static_assert(sizeof(TqkAggTerms) == 40, "five 64-bit words: agg_terms_init_kernel");

void tqk_agg_terms_lds_capacities(uint32_t out[2]) {
  out[0] = AT_LDS_SMALL;
  out[1] = AT_LDS_LARGE;
}

uint32_t tqk_agg_terms_max_size() { return TERMS_MAX_SIZE; }

hipError_t tqk_launch_agg_terms_init(TqkAggTerms *records, uint32_t *rows, uint32_t n_queries, uint32_t n_keys, hipStream_t st) {
  if (!n_queries) return hipSuccess;
  if (!records || (n_keys && !rows)) return hipErrorInvalidValue;
  agg_terms_init_kernel<<<dim3(n_queries), dim3(WALK_THREADS), 0, st>>>(records, rows, n_keys);
  return hipGetLastError();
}

hipError_t tqk_launch_agg_terms_count(const TqkAggTermsParams &p, hipStream_t st) {
  if (!p.ds.n_queries || !p.n_slices) return hipSuccess;
  if (p.col.codec > TQK_COL_BLOCKWISE || p.gcd == 0ull) return hipErrorInvalidValue;
  if (p.n_keys > TERMS_MAX_KEYS || (p.n_keys && !p.rows) || !p.records) return hipErrorInvalidValue;
  if (p.n_keys > std::min(p.lds_buckets, AT_LDS_LARGE))  // past "agg_lds_buckets" or the large table: straight to the row
    agg_terms_launch<AT_GLOBAL_TABLE>(p, st);
  else if (p.n_keys <= AT_LDS_SMALL)
    agg_terms_launch<AT_LDS_SMALL>(p, st);
  else
    agg_terms_launch<AT_LDS_LARGE>(p, st);
  return hipGetLastError();
}

hipError_t tqk_launch_agg_terms_select(const TqkAggTermsSelectParams &p, hipStream_t st) {
  if (!p.n_queries) return hipSuccess;
  if (p.n_keys > TERMS_MAX_KEYS || (p.n_keys && !p.rows) || !p.records || p.order > TERMS_KEY_DESC) return hipErrorInvalidValue;
  if (p.segment_size == 0u || p.segment_size > TERMS_MAX_SIZE) return hipErrorInvalidValue;
  if (p.out_stride < std::min(p.segment_size, p.n_keys) || (p.n_keys && (!p.out_keys || !p.out_counts))) return hipErrorInvalidValue;
  agg_terms_select_kernel<<<dim3(p.n_queries), dim3(TSEL_THREADS), 0, st>>>(p);
  return hipGetLastError();
}
