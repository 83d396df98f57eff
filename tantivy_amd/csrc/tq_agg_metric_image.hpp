// tq_agg_metric_image.hpp — the ORDER VALUE of a terms entry under a metric order (tq_agg_terms_sub_batch*): a fixed-width
// unsigned integer image of one metric of a 40-byte bucket record, monotone in the metric's typed value.  One piece of
// code for the selection kernel (tq_agg_terms_sub.hip) and for the host-only tq_agg_terms_metric_image
// (tq_agg_terms_sub.cpp): integer arithmetic alone, so both compute the same bits.
//   VALUE_COUNT  the record's count                                                         (32 bits)
//   MIN / MAX    the u64-space value: tantivy's mapping is monotone for U64 / I64 / F64      (64 bits)
//   SUM          the exact typed sum, biased: U64 the sum; I64 sum - count * 2^63 + 2^95      (96 bits)
//   AVG          the monotone u64 image of the f64 that is the correctly rounded (half to even) quotient of the exact typed
//                sum by count — integer long division, never f64 arithmetic on a rounded sum  (64 bits)
// A record with count == 0 orders as typed 0 under MIN / MAX / AVG (the reference's compute_metric_value(..).unwrap_or(0.0),
// src/aggregation/metric/stats.rs:325-357, bucket/term_agg/mod.rs:1058-1065); its sum and count are 0 anyway.
// SUM and AVG of an F64 column are not served (F64 sums are not): the callers refuse the pair before they come here.
#pragma once
#include <cstdint>

#if defined(__HIP__) || defined(__HIPCC__)
#define TQ_IMG_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define TQ_IMG_HD inline
#endif

constexpr uint32_t TQ_IMG_VALUE_COUNT = 0, TQ_IMG_MIN = 1, TQ_IMG_MAX = 2, TQ_IMG_SUM = 3, TQ_IMG_AVG = 4;  // tq_terms_metric
constexpr uint32_t TQ_IMG_U64 = 0, TQ_IMG_I64 = 1, TQ_IMG_F64 = 2;                                            // tq_value_type

struct TqImage {  // a 128-bit unsigned integer
  uint64_t lo, hi;
};

// bits of an image under a metric: what the radix select walks
TQ_IMG_HD uint32_t tq_image_bits(uint32_t metric) { return metric == TQ_IMG_VALUE_COUNT ? 32u : metric == TQ_IMG_SUM ? 96u : 64u; }

// f64 bits -> the u64 whose unsigned order is the f64 order (common/src/lib.rs f64_to_u64)
TQ_IMG_HD uint64_t tq_image_of_f64_bits(uint64_t bits) { return (bits >> 63) ? ~bits : bits ^ (1ull << 63); }

// one step of a long division by a 32-bit divisor: r (< c) and the next 32-bit limb -> the quotient's limb, r the rest
TQ_IMG_HD uint64_t tq_image_div_step(uint64_t &r, uint32_t limb, uint32_t c) {
  const uint64_t cur = (r << 32) | limb;  // r < c: cur / c < 2^32
  const uint64_t qd = cur / c;
  r = cur - qd * c;
  return qd;
}

// the low 64 bits of (w2 : w1 : w0) >> s, 0 <= s < 192
TQ_IMG_HD uint64_t tq_image_shr192(uint64_t w2, uint64_t w1, uint64_t w0, int s) {
  const uint64_t a = s >= 128 ? w2 : s >= 64 ? w1 : w0;    // the word that holds bit s
  const uint64_t b = s >= 128 ? 0ull : s >= 64 ? w2 : w1;  // the one above it
  const int bit = s & 63;
  return bit ? (a >> bit) | (b << (64 - bit)) : a;
}

// The f64 bits of (neg ? -1 : 1) * n / c, correctly rounded, half to even; n = n_hi * 2^64 + n_lo < 2^96, 1 <= c < 2^32.
// n * 2^96 is divided by c limb by limb (six 64 / 32-bit steps): the quotient has at least 65 bits, so the 53 bits of the
// significand, the guard bit and the sticky rest are all inside it; the result is a normal f64 (2^-32 < |n / c| < 2^96).
TQ_IMG_HD uint64_t tq_image_div_f64(uint64_t n_hi, uint64_t n_lo, uint32_t c, bool neg) {
  if (!(n_hi | n_lo)) return 0ull;  // +0.0
  // the 192-bit quotient in three words, w0 the least significant (no array: nothing is indexed by a run-time value)
  uint64_t r = 0ull;
  uint64_t w2 = tq_image_div_step(r, (uint32_t)n_hi, c) << 32;
  w2 |= tq_image_div_step(r, (uint32_t)(n_lo >> 32), c);
  uint64_t w1 = tq_image_div_step(r, (uint32_t)n_lo, c) << 32;
  w1 |= tq_image_div_step(r, 0u, c);
  uint64_t w0 = tq_image_div_step(r, 0u, c) << 32;
  w0 |= tq_image_div_step(r, 0u, c);
  const int nb = w2 ? 192 - __builtin_clzll(w2) : 128 - __builtin_clzll(w1);  // bit length of the quotient, >= 65
  const int shift = nb - 53;                                                   // 12 .. 139
  uint64_t m = tq_image_shr192(w2, w1, w0, shift) & ((1ull << 53) - 1ull);     // 53 bits, the top one set
  // the guard bit, and whether anything is set below it or left over
  const int g = shift - 1, gbit = g & 63;
  const bool guard = tq_image_shr192(w2, w1, w0, g) & 1ull;
  const uint64_t gmask = (1ull << gbit) - 1ull;
  const uint64_t below = g >= 128 ? (w0 | w1 | (w2 & gmask)) : g >= 64 ? (w0 | (w1 & gmask)) : (w0 & gmask);
  const bool sticky = r != 0ull || below != 0ull;
  if (guard && (sticky || (m & 1ull))) ++m;  // (m == 2^53: the add below carries into the exponent)
  const uint64_t biased = (uint64_t)(1023 + 52 + shift - 96);
  return ((biased - 1ull) << 52) + m + (neg ? 1ull << 63 : 0ull);
}

// the exact typed sum of a record as sign and magnitude (< 2^96): U64 the 128-bit sum; I64 minus count * 2^63
TQ_IMG_HD void tq_image_typed_sum(uint64_t count, uint64_t sum_lo, uint64_t sum_hi, uint32_t value_type, uint64_t &mag_hi,
                                  uint64_t &mag_lo, bool &neg) {
  neg = false;
  mag_hi = sum_hi;
  mag_lo = sum_lo;
  if (value_type != TQ_IMG_I64) return;
  const uint64_t sub_lo = count << 63, sub_hi = count >> 1;
  const uint64_t lo = sum_lo - sub_lo;
  const uint64_t hi = sum_hi - sub_hi - (sum_lo < sub_lo ? 1ull : 0ull);
  if (hi >> 63) {  // negative: two's complement
    neg = true;
    mag_lo = ~lo + 1ull;
    mag_hi = ~hi + (mag_lo == 0ull ? 1ull : 0ull);
  } else {
    mag_lo = lo;
    mag_hi = hi;
  }
}

// the image of `metric` (<= TQ_IMG_AVG) of a record of a value_type (<= TQ_IMG_F64) column; SUM / AVG with F64: not served,
// the callers refuse it (here: the image of 0)
TQ_IMG_HD TqImage tq_metric_image(uint64_t count, uint64_t min_value, uint64_t max_value, uint64_t sum_lo, uint64_t sum_hi,
                                  uint32_t value_type, uint32_t metric) {
  const uint64_t typed_zero = value_type == TQ_IMG_U64 ? 0ull : 1ull << 63;  // 0, 0i64, +0.0 in u64 space
  if (metric == TQ_IMG_VALUE_COUNT) return TqImage{count, 0ull};
  if (metric == TQ_IMG_MIN) return TqImage{count ? min_value : typed_zero, 0ull};
  if (metric == TQ_IMG_MAX) return TqImage{count ? max_value : typed_zero, 0ull};
  if (value_type == TQ_IMG_F64) return metric == TQ_IMG_SUM ? TqImage{0ull, 0ull} : TqImage{1ull << 63, 0ull};
  if (metric == TQ_IMG_SUM) {
    if (value_type != TQ_IMG_I64) return TqImage{sum_lo, sum_hi};
    const uint64_t sub_lo = count << 63, sub_hi = count >> 1;  // sum - count * 2^63 + 2^95, never negative
    const uint64_t lo = sum_lo - sub_lo;
    const uint64_t hi = sum_hi - sub_hi - (sum_lo < sub_lo ? 1ull : 0ull) + (1ull << 31);
    return TqImage{lo, hi};
  }
  if (!count) return TqImage{1ull << 63, 0ull};  // +0.0
  uint64_t mag_hi, mag_lo;
  bool neg;
  tq_image_typed_sum(count, sum_lo, sum_hi, value_type, mag_hi, mag_lo, neg);
  return TqImage{tq_image_of_f64_bits(tq_image_div_f64(mag_hi, mag_lo, (uint32_t)count, neg)), 0ull};
}
