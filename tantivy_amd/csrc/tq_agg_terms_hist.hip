// tq_agg_terms_hist.hip — terms x histogram (tq_agg_terms_hist_batch*): a dense histogram of a column H per key of a terms
// aggregation over a column T, per query of a batch (src/aggregation/bucket/term_agg/term_histogram.rs, the fused
// collector: counts[term * num_time_buckets + bucket] and per term the docs outside hard_bounds).  The grid of a query is
// n_keys rows of n_buckets + 1 entries, the last of a row the key's OUTSIDE entry (no value in H, or out of bounds): one
// index serves every doc, and a key's doc count is one row sum.
//
// count    workgroup = (query, slice of the bitmap words).  Assembled from the shared walk (docset_walk,
//          tq_docset_walk.hpp), col_key_index / col_value (tq_agg_device.hpp) and the f64 bucket arithmetic of agg_kernel
//          (tq_agg_value.hpp).  Its own: a doc with a value in T takes rg_row + col_value of H and adds one to cell
//          i x (n_buckets + 1) + b, b = n_buckets for outside — of the workgroup's uint32 LDS table (n_cells <=
//          min(lds_buckets, CAP); a table of 2 048 or of 8 192 entries, two instantiations), flushed with one vector atomic
//          add per non-zero cell, or above the capacity of the query's grid row directly.  Per-lane counts are reduced by
//          shuffles and LDS and published by one lane.
// rowsum   behind the last sub-batch: every key's row sum into the query's totals row; G = 1 .. 64 lanes a key.
// (select) tqk_launch_agg_terms_select of tq_agg_terms.hip over the totals rows: the terms call's own selection.
// gather   a wavefront per (query, returned entry): the entry's index from its key, its n_buckets cells into out_hist.
// init     the records (zeros) and every grid and totals row, in front of the first count launch.
// Plain vector stores and integer vector atomics only.  Nothing is written at or past n_cells of a grid row (a key index
// outside [0, n_keys) or a bucket outside [0, n_buckets) of an in-bounds value — none, by the columns' own min / max / gcd
// and the dense range — is counted in out_of_range and dropped), nor at or past n_returned of an output row set or n_buckets
// of a histogram row.  HBM model: agg_terms_count_kernel's + 8 per counted doc with a value in H + 8 per counted doc of an
// Optional H + per query 4 x n_cells + 4 x n_buckets per entry returned.
#include <algorithm>

#include "tq_agg_device.hpp"
#include "tq_agg_value.hpp"
#include "tq_column_read.hpp"
#include "tq_common.hpp"
#include "tq_docset_walk.hpp"
#include "tq_launch.h"

namespace {

// the LDS table: 4 bytes per cell beside the slabs' 16 KB — agg_terms_count_kernel's capacities (same entry size, same
// walk: six and three workgroups per CU)
#ifndef TQ_AGG_TERMS_HIST_LDS_LARGE
#define TQ_AGG_TERMS_HIST_LDS_LARGE 8192
#endif
#ifndef TQ_AGG_TERMS_HIST_LDS_SMALL
#define TQ_AGG_TERMS_HIST_LDS_SMALL 2048
#endif
// the instantiation the global path runs in, by its table's capacity (it never touches the table)
#ifndef TQ_AGG_TERMS_HIST_GLOBAL_TABLE
#define TQ_AGG_TERMS_HIST_GLOBAL_TABLE TQ_AGG_TERMS_HIST_LDS_LARGE
#endif
constexpr uint32_t TH_LDS_LARGE = TQ_AGG_TERMS_HIST_LDS_LARGE;
constexpr uint32_t TH_LDS_SMALL = TQ_AGG_TERMS_HIST_LDS_SMALL;
constexpr uint32_t TH_GLOBAL_TABLE = TQ_AGG_TERMS_HIST_GLOBAL_TABLE;
constexpr uint32_t TH_MAX_CELLS = 65536;  // TQ_AGG_MAX_BUCKETS
constexpr uint32_t TH_PART = 5;
constexpr uint32_t TH_ROWSUM_BLOCKS = 64;  // at most, per query
static_assert(TH_GLOBAL_TABLE >= 1u && TH_GLOBAL_TABLE <= TH_LDS_LARGE, "one of the tables, or a one-entry stub");
static_assert(TH_LDS_SMALL >= 1u && TH_LDS_SMALL <= TH_LDS_LARGE && TH_LDS_LARGE * 4u + 16640u <= 65536u, "the static LDS of a workgroup");

template <bool OPT_T, bool OPT_H, uint32_t CAP>
__global__ __launch_bounds__(WALK_THREADS) void agg_terms_hist_count_kernel(TqkAggTermsHistParams p) {
  __shared__ uint16_t slabs[WALK_SLAB_ENTRIES];
  __shared__ uint32_t table[CAP];
  __shared__ unsigned long long part[WALK_WAVES][TH_PART];
  const int lane = (int)__lane_id();
  const uint32_t wave = threadIdx.x >> 6;
  const uint32_t q = blockIdx.x % p.t.ds.n_queries, slice = blockIdx.x / p.t.ds.n_queries;
  const uint32_t n_keys = p.t.n_keys, n_buckets = p.n_buckets;
  const uint32_t row_len = n_buckets + 1u, n_cells = n_keys * row_len;  // (the host checked: <= TH_MAX_CELLS)
  const bool in_lds = n_cells <= p.t.lds_buckets && n_cells <= CAP;  // (uniform)
  uint32_t *const grid = p.t.rows + (size_t)q * n_cells;
  if (in_lds) {
    for (uint32_t i = threadIdx.x; i < n_cells; i += WALK_THREADS) table[i] = 0u;
    __syncthreads();
  }
  uint32_t valued = 0, oor = 0, counted = 0, valued_h = 0;  // per lane
  const uint32_t cnt = docset_walk(p.t.ds, p.t.ds.queries + q, slice, p.t.words_per_slice, slabs, wave, lane, [&](bool has, uint32_t doc) {
    uint32_t r = 0;
    if (!(has && rg_row<OPT_T>(p.t.col, doc, r))) return;
    ++valued;
    const uint64_t idx = col_key_index(p.t.col, p.t.min_value, p.t.gcd, r);
    if (idx >= (uint64_t)n_keys) {
      ++oor;
      return;
    }
    ++counted;
    uint64_t b = n_buckets;  // outside: no value in H, or out of bounds
    uint32_t rh = 0;
    if (rg_row<OPT_H>(p.col_h, doc, rh)) {
      ++valued_h;
      const double val = tq_agg_f64(col_value(p.col_h, p.min_value_h, p.gcd_h, rh), p.value_type_h);
      if (p.bounds_min <= val && val <= p.bounds_max) {  // (HistogramBounds::contains: never true for NaN, +-inf)
        const int64_t pos = tq_agg_sat_i64(floor((val - p.offset) / p.interval));
        b = (uint64_t)pos - (uint64_t)p.base_pos;  // (a pos below base_pos wraps to a huge index)
        if (b >= (uint64_t)n_buckets) {
          ++oor;
          return;
        }
      }
    }
    const uint32_t cell = (uint32_t)idx * row_len + (uint32_t)b;  // < n_cells
    if (in_lds)
      atomicAdd(&table[cell], 1u);
    else
      atomicAdd(grid + cell, 1u);
  });
  // the wavefront's part, then the workgroup's
  const unsigned long long t_cnt = wave_sum64(cnt), t_val = wave_sum64(valued), t_oor = wave_sum64(oor);
  const unsigned long long t_ctd = wave_sum64(counted), t_vh = wave_sum64(valued_h);
  if (lane == 0) {
    part[wave][0] = t_cnt;
    part[wave][1] = t_val;
    part[wave][2] = t_oor;
    part[wave][3] = t_ctd;
    part[wave][4] = t_vh;
  }
  __syncthreads();  // (also: every wavefront's LDS table adds are done)
  if (in_lds) {
    for (uint32_t i = threadIdx.x; i < n_cells; i += WALK_THREADS) {
      const uint32_t c = table[i];
      if (c) atomicAdd(grid + i, c);
    }
  }
  if (threadIdx.x != 0u) return;
  unsigned long long matches = 0, count = 0, out_of_range = 0, in_keys = 0, with_h = 0;
  for (uint32_t v = 0; v < WALK_WAVES; ++v) {
    matches += part[v][0];
    count += part[v][1];
    out_of_range += part[v][2];
    in_keys += part[v][3];
    with_h += part[v][4];
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
  if (with_h) atomicAdd(p.t.totals + 4, with_h);
  if (in_keys) atomicAdd(p.t.totals + 5, in_keys);
}

// totals row q, entry i = the sum of grid row q's entries [i x row_len, (i + 1) x row_len).  G lanes a key (a power of two,
// 1 .. 64: the smallest that covers row_len, so that short rows do not idle a wavefront); grid = (n_queries, blocks)
__global__ __launch_bounds__(WALK_THREADS) void agg_terms_hist_rowsum_kernel(TqkAggTermsHistFinishParams p, uint32_t g_log2) {
  const uint32_t q = blockIdx.x, n_keys = p.n_keys, row_len = p.n_buckets + 1u;
  const uint32_t G = 1u << g_log2, keys_per_block = WALK_THREADS >> g_log2;
  const uint32_t sub = threadIdx.x & (G - 1u), slot = threadIdx.x >> g_log2;
  const uint32_t *const grid = p.grid + (size_t)q * n_keys * row_len;
  uint32_t *const totals = p.totals_rows + (size_t)q * n_keys;
  // (k0 is the workgroup's: every lane takes every trip, so the shuffles below are converged)
  for (uint32_t k0 = blockIdx.y * keys_per_block; k0 < n_keys; k0 += gridDim.y * keys_per_block) {
    const uint32_t i = k0 + slot;
    uint32_t sum = 0;
    if (i < n_keys) {
      const uint32_t *const row = grid + (size_t)i * row_len;
      for (uint32_t b = sub; b < row_len; b += G) sum += row[b];
    }
    for (uint32_t off = G >> 1; off > 0u; off >>= 1) sum += __shfl_xor(sum, (int)off, 64);
    if (sub == 0u && i < n_keys) totals[i] = sum;
  }
}

// out_hist row (q, j), entries [0, n_buckets) = the cells of the key at out_keys[q][j], for j < n_returned: a wavefront per
// entry, coalesced on both sides.  grid = (n_queries, ceil(width / WALK_WAVES))
__global__ __launch_bounds__(WALK_THREADS) void agg_terms_hist_gather_kernel(TqkAggTermsHistFinishParams p) {
  const uint32_t q = blockIdx.x, j = blockIdx.y * WALK_WAVES + (threadIdx.x >> 6);
  const uint32_t lane = threadIdx.x & 63u;
  uint32_t n_ret = p.records[q].n_returned;
  n_ret = n_ret < p.out_stride ? n_ret : p.out_stride;
  if (j >= n_ret) return;
  const size_t o = (size_t)q * p.out_stride + j;
  const uint64_t off = p.out_keys[o] - p.min_value;
  const uint64_t idx = p.gcd > 1ull ? off / p.gcd : off;
  if (idx >= (uint64_t)p.n_keys) return;  // (none: the selection made the key from an index below n_keys)
  const uint32_t row_len = p.n_buckets + 1u;
  const uint32_t *const src = p.grid + ((size_t)q * p.n_keys + (size_t)idx) * row_len;
  uint32_t *const dst = p.out_hist + o * p.hist_stride;
  for (uint32_t b = lane; b < p.n_buckets; b += 64u) dst[b] = src[b];
}

// record q = zeros; grid row q and totals row q = 0.  grid = n_queries
__global__ __launch_bounds__(WALK_THREADS) void agg_terms_hist_init_kernel(TqkAggTerms *records, uint32_t *grid, uint32_t *totals_rows,
                                                                         uint32_t n_cells, uint32_t n_keys) {
  const uint32_t q = blockIdx.x;
  if (threadIdx.x < 5u) reinterpret_cast<unsigned long long *>(records + q)[threadIdx.x] = 0ull;
  uint32_t *const row = grid + (size_t)q * n_cells;
  for (uint32_t i = threadIdx.x; i < n_cells; i += WALK_THREADS) row[i] = 0u;
  uint32_t *const tot = totals_rows + (size_t)q * n_keys;
  for (uint32_t i = threadIdx.x; i < n_keys; i += WALK_THREADS) tot[i] = 0u;
}

template <uint32_t CAP>
void agg_terms_hist_launch(const TqkAggTermsHistParams &p, hipStream_t st) {
  const dim3 grid(p.t.ds.n_queries * p.t.n_slices), block(WALK_THREADS);
  const bool opt_t = p.t.col.present != nullptr, opt_h = p.col_h.present != nullptr;
  if (opt_t && opt_h)
    agg_terms_hist_count_kernel<true, true, CAP><<<grid, block, 0, st>>>(p);
  else if (opt_t)
    agg_terms_hist_count_kernel<true, false, CAP><<<grid, block, 0, st>>>(p);
  else if (opt_h)
    agg_terms_hist_count_kernel<false, true, CAP><<<grid, block, 0, st>>>(p);
  else
    agg_terms_hist_count_kernel<false, false, CAP><<<grid, block, 0, st>>>(p);
}

bool finish_params_ok(const TqkAggTermsHistFinishParams &p) {
  if (p.n_keys > TH_MAX_CELLS || p.n_buckets > TH_MAX_CELLS) return false;
  return (uint64_t)p.n_keys * ((uint64_t)p.n_buckets + 1u) <= (uint64_t)TH_MAX_CELLS && p.grid && p.totals_rows;
}

}  // namespace

static_assert(sizeof(TqkAggTerms) == 40, "five 64-bit words: agg_terms_hist_init_kernel");

void tqk_agg_terms_hist_lds_capacities(uint32_t out[2]) {
  out[0] = TH_LDS_SMALL;
  out[1] = TH_LDS_LARGE;
}

hipError_t tqk_launch_agg_terms_hist_init(TqkAggTerms *records, uint32_t *grid, uint32_t *totals_rows, uint32_t n_queries, uint32_t n_cells,
                                          uint32_t n_keys, hipStream_t st) {
  if (!n_queries) return hipSuccess;
  if (!records || n_cells > TH_MAX_CELLS || n_keys > n_cells || (n_cells && (!grid || !totals_rows))) return hipErrorInvalidValue;
  agg_terms_hist_init_kernel<<<dim3(n_queries), dim3(WALK_THREADS), 0, st>>>(records, grid, totals_rows, n_cells, n_keys);
  return hipGetLastError();
}

hipError_t tqk_launch_agg_terms_hist_count(const TqkAggTermsHistParams &p, hipStream_t st) {
  if (!p.t.ds.n_queries || !p.t.n_slices) return hipSuccess;
  if (p.t.col.codec > TQK_COL_BLOCKWISE || p.col_h.codec > TQK_COL_BLOCKWISE || p.t.gcd == 0ull) return hipErrorInvalidValue;
  if (p.t.n_keys > TH_MAX_CELLS || p.n_buckets > TH_MAX_CELLS || !p.t.records) return hipErrorInvalidValue;
  const uint64_t n_cells = (uint64_t)p.t.n_keys * ((uint64_t)p.n_buckets + 1u);
  if (n_cells > (uint64_t)TH_MAX_CELLS || (n_cells && !p.t.rows)) return hipErrorInvalidValue;
  if (n_cells > (uint64_t)std::min(p.t.lds_buckets, TH_LDS_LARGE))  // past "agg_lds_buckets" or the large table: straight to the row
    agg_terms_hist_launch<TH_GLOBAL_TABLE>(p, st);
  else if (n_cells <= (uint64_t)TH_LDS_SMALL)
    agg_terms_hist_launch<TH_LDS_SMALL>(p, st);
  else
    agg_terms_hist_launch<TH_LDS_LARGE>(p, st);
  return hipGetLastError();
}

hipError_t tqk_launch_agg_terms_hist_rowsum(const TqkAggTermsHistFinishParams &p, hipStream_t st) {
  if (!p.n_queries || !p.n_keys) return hipSuccess;
  if (!finish_params_ok(p)) return hipErrorInvalidValue;
  uint32_t g_log2 = 0;
  while (g_log2 < 6u && (1u << g_log2) < p.n_buckets + 1u) ++g_log2;
  const uint32_t keys_per_block = WALK_THREADS >> g_log2;
  const uint32_t blocks = std::min((p.n_keys + keys_per_block - 1u) / keys_per_block, TH_ROWSUM_BLOCKS);
  agg_terms_hist_rowsum_kernel<<<dim3(p.n_queries, blocks), dim3(WALK_THREADS), 0, st>>>(p, g_log2);
  return hipGetLastError();
}

hipError_t tqk_launch_agg_terms_hist_gather(const TqkAggTermsHistFinishParams &p, hipStream_t st) {
  if (!p.n_queries || !p.n_keys || !p.n_buckets || !p.width) return hipSuccess;
  if (!finish_params_ok(p) || !p.records || !p.out_keys || !p.out_hist || p.gcd == 0ull) return hipErrorInvalidValue;
  if (p.hist_stride < p.n_buckets || p.out_stride < p.width || p.width > p.n_keys) return hipErrorInvalidValue;
  agg_terms_hist_gather_kernel<<<dim3(p.n_queries, (p.width + WALK_WAVES - 1u) / WALK_WAVES), dim3(WALK_THREADS), 0, st>>>(p);
  return hipGetLastError();
}
