// tq_column_read.hpp — the device-side readers of a resident u64_based column (TqkColumn, tq_column.cpp): the three codecs'
// packed values and the Optional row lookup.  Shared by tq_range.hip (range fill, column decode) and tq_sort.hip (the sort
// key of TopDocs::order_by_fast_field).  Internal linkage: every kernel file gets its own copy.
#pragma once
#include "tq_common.hpp"
#include "tq_launch.h"

namespace {

// num_bits bits at bit `bit` of the stream starting at dword `base` of p: aligned dword loads only (the 16 zero bytes
// behind the payload keep the last value's second and third dword in bounds)
__device__ __forceinline__ uint64_t rg_bits(const uint32_t *__restrict__ p, uint64_t base, uint64_t bit, uint32_t num_bits) {
  if (num_bits == 0u) return 0ull;
  const uint64_t i = base + (bit >> 5);
  const uint32_t sh = (uint32_t)bit & 31u;
  const uint32_t need = sh + num_bits;  // <= 95
  uint64_t v = (uint64_t)(p[i] >> sh);
  if (need > 32u) v |= (uint64_t)p[i + 1] << (32u - sh);
  if (need > 64u) v |= (uint64_t)p[i + 2] << (64u - sh);  // (sh >= 1 here)
  return num_bits >= 64u ? v : v & ((1ull << num_bits) - 1ull);
}
// Line::eval (line.rs:65-68): the product's bits 32..63, truncated to 32 bits and sign-extended — a falling line's slope is
// the complement of its magnitude
__device__ __forceinline__ uint64_t rg_line(uint64_t slope, uint64_t intercept, uint32_t x) {
  return intercept + (uint64_t)(int64_t)(int32_t)(uint32_t)(((uint64_t)x * slope) >> 32);
}
// the packed value of `row` (< num_rows): Bitpacked (value - min) / gcd, Linear the value, BlockwiseLinear (value - min) / gcd
template <uint32_t CODEC>
__device__ __forceinline__ uint64_t rg_value(const TqkColumn &c, uint32_t row) {
  if (CODEC == TQK_COL_BITPACKED) return rg_bits(c.payload, 0ull, (uint64_t)row * c.num_bits, c.num_bits);
  if (CODEC == TQK_COL_LINEAR)
    return rg_line(c.slope, c.intercept, row) + rg_bits(c.payload, 0ull, (uint64_t)row * c.num_bits, c.num_bits);
  const TqkColBlock b = c.blocks[row >> 9];
  const uint32_t x = row & 511u;
  return rg_line(b.slope, b.intercept, x) + rg_bits(c.payload, b.data_off >> 2, (uint64_t)x * b.bit_width, b.bit_width);
}

// the row of `doc` (< max_doc), or false: the doc has no value
template <bool OPTIONAL>
__device__ __forceinline__ bool rg_row(const TqkColumn &c, uint32_t doc, uint32_t &row) {
  if (!OPTIONAL) {
    row = doc;
    return doc < c.num_rows;
  }
  const uint2 w = c.present[doc >> 5];
  const uint32_t bit = 1u << (doc & 31u);
  row = w.y + (uint32_t)__popc(w.x & (bit - 1u));
  return (w.x & bit) != 0u && row < c.num_rows;
}

}  // namespace
