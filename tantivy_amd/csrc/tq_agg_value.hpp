// tq_agg_value.hpp — how a u64-space column value becomes the f64 a histogram buckets, and how that f64's bucket
// position becomes an integer.  One piece of code for the kernels (tq_agg.hip, tq_agg_sub.hip, tq_agg_terms_hist.hip) and the host plan
// (tq_agg.cpp), which must agree bit for bit with each other and with the reference's f64_from_fastfield_u64
// (src/aggregation/mod.rs:351-383; common/src/lib.rs:108-114 u64_to_f64) and `f64 as i64`.  Built with -ffp-contract=off.
#pragma once
#include <cstdint>

#if defined(__HIP__) || defined(__HIPCC__)
#define TQ_AGGV_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define TQ_AGGV_HD inline
#endif

constexpr uint32_t TQ_AGGV_U64 = 0, TQ_AGGV_I64 = 1, TQ_AGGV_F64 = 2;  // tq_value_type

TQ_AGGV_HD double tq_agg_f64(uint64_t v, uint32_t value_type) {
  const uint64_t high = 1ull << 63;
  if (value_type == TQ_AGGV_I64) return (double)(int64_t)(v ^ high);
  if (value_type == TQ_AGGV_F64) {
    const uint64_t bits = (v & high) ? v ^ high : ~v;
    double d;
    __builtin_memcpy(&d, &bits, sizeof d);
    return d;
  }
  return (double)v;
}

// Rust's `f64 as i64`: saturating, NaN is 0 (a plain C++ cast is undefined out of range)
TQ_AGGV_HD int64_t tq_agg_sat_i64(double x) {
  if (x != x) return 0;
  if (x >= 9223372036854775808.0) return INT64_MAX;
  if (x <= -9223372036854775808.0) return INT64_MIN;
  return (int64_t)x;
}
