// tq_range.hip — fast-field range clauses (tq_range_prepare): what RangeDocSet over a Column<u64> finds for
// FastFieldRangeWeight::scorer (src/query/range_query/range_query_fastfield.rs:414-450, fast_field_range_doc_set.rs) —
// the docs whose column value lies in a range — as the {32 doc bits, docs before the word} table of a term set, and the
// codec access of tq_column_decode.  The column is tantivy's own u64_based byte format, resident as the file holds it
// (columnar/src/column_values/u64_based/{bitpacked,linear,blockwise_linear,line}.rs, bitpacker/src/bitpacker.rs).
//
// One build is the fill below over every word of the table, then the rank stage of tq_termset.hip:
//   fill     a lane per doc, a 64-lane wavefront per two bitmap words: the lane reads its row's packed value n — num_bits
//            bits at bit row * num_bits of a little-endian LSB-first stream, assembled from up to three aligned dwords —
//            and compares it with the range IN THE PACKED DOMAIN (the host has divided the bounds by the gcd:
//            transform_range_before_linear_transformation, bitpacked.rs:37-49; Linear stores the value itself); the two
//            halves of the wavefront's 64-bit ballot are the two words, stored by lanes 0 and 32.  The 64 rows of a
//            wavefront are consecutive (an Optional column: the present docs' rows are), so its loads fall into
//            64 * num_bits / 8 consecutive bytes — at most 512, 56 for a 7-bit column: the coalescer's case, no LDS staging
//   rank     tqk_launch_bitmap_rank
// HBM model: the payload once + 8 B per 32 docs written and read once by the scan (+ 8 B per 32 docs of presence table).
#include <algorithm>

#include "tq_column_read.hpp"  // rg_bits / rg_line / rg_value / rg_row
#include "tq_common.hpp"
#include "tq_launch.h"

namespace {

constexpr uint32_t RG_THREADS = 256;

template <uint32_t CODEC, bool OPTIONAL>
__global__ __launch_bounds__(RG_THREADS) void range_fill_kernel(TqkColumn c, uint64_t lo, uint64_t hi, uint2 *__restrict__ tab,
                                                                uint32_t n_words) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t n_pairs = (n_words + 1u) >> 1;
  const uint32_t waves = gridDim.x * (RG_THREADS / 64u);
  for (uint32_t pair = blockIdx.x * (RG_THREADS / 64u) + (threadIdx.x >> 6); pair < n_pairs; pair += waves) {
    const uint64_t doc64 = (uint64_t)pair * 64u + lane;
    bool hit = false;
    if (doc64 < c.max_doc) {
      uint32_t row;
      if (rg_row<OPTIONAL>(c, (uint32_t)doc64, row)) {  // (a doc without a value loads nothing)
        const uint64_t n = rg_value<CODEC>(c, row);
        hit = n >= lo && n <= hi;
      }
    }
    const unsigned long long m = __ballot(hit);
    const uint32_t w = pair * 2u + (lane >> 5);
    if ((lane & 31u) == 0u && w < n_words) tab[w].x = lane ? (uint32_t)(m >> 32) : (uint32_t)m;
  }
}

template <uint32_t CODEC>
__global__ __launch_bounds__(RG_THREADS) void column_decode_kernel(TqkColumn c, uint64_t min_value, uint64_t gcd, uint32_t first_row,
                                                                   uint32_t n, uint64_t *__restrict__ out) {
  for (uint32_t i = blockIdx.x * RG_THREADS + threadIdx.x; i < n; i += gridDim.x * RG_THREADS) {
    const uint32_t row = first_row + i;
    if (row >= c.num_rows) continue;
    const uint64_t v = rg_value<CODEC>(c, row);
    out[i] = CODEC == TQK_COL_LINEAR ? v : min_value + gcd * v;
  }
}

template <uint32_t CODEC>
void fill_launch(const TqkColumn &c, uint64_t lo, uint64_t hi, uint2 *tab, uint32_t n_words, uint32_t grid, hipStream_t st) {
  if (c.present)
    range_fill_kernel<CODEC, true><<<dim3(grid), dim3(RG_THREADS), 0, st>>>(c, lo, hi, tab, n_words);
  else
    range_fill_kernel<CODEC, false><<<dim3(grid), dim3(RG_THREADS), 0, st>>>(c, lo, hi, tab, n_words);
}

}  // namespace

hipError_t tqk_launch_range_fill(const TqkColumn &col, uint64_t lo, uint64_t hi, uint2 *tab, uint32_t n_words, hipStream_t st) {
  if (!n_words) return hipSuccess;
  const uint32_t n_pairs = (n_words + 1u) / 2u;
  const uint32_t per_wg = RG_THREADS / 64u;
  const uint32_t grid = std::min<uint32_t>((n_pairs + per_wg - 1u) / per_wg, 1u << 16);
  switch (col.codec) {
    case TQK_COL_BITPACKED: fill_launch<TQK_COL_BITPACKED>(col, lo, hi, tab, n_words, grid, st); break;
    case TQK_COL_LINEAR: fill_launch<TQK_COL_LINEAR>(col, lo, hi, tab, n_words, grid, st); break;
    case TQK_COL_BLOCKWISE: fill_launch<TQK_COL_BLOCKWISE>(col, lo, hi, tab, n_words, grid, st); break;
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

hipError_t tqk_launch_column_decode(const TqkColumn &col, uint64_t min_value, uint64_t gcd, uint32_t first_row, uint32_t n,
                                    uint64_t *out, hipStream_t st) {
  if (!n) return hipSuccess;
  const uint32_t grid = std::min<uint32_t>((n + RG_THREADS - 1u) / RG_THREADS, 1u << 16);
  switch (col.codec) {
    case TQK_COL_BITPACKED:
      column_decode_kernel<TQK_COL_BITPACKED><<<dim3(grid), dim3(RG_THREADS), 0, st>>>(col, min_value, gcd, first_row, n, out);
      break;
    case TQK_COL_LINEAR:
      column_decode_kernel<TQK_COL_LINEAR><<<dim3(grid), dim3(RG_THREADS), 0, st>>>(col, min_value, gcd, first_row, n, out);
      break;
    case TQK_COL_BLOCKWISE:
      column_decode_kernel<TQK_COL_BLOCKWISE><<<dim3(grid), dim3(RG_THREADS), 0, st>>>(col, min_value, gcd, first_row, n, out);
      break;
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}
