// tq_agg_range_search.hpp — which bucket of a range aggregation a u64-space value falls in (tq_agg_range_batch*): THE LAST
// BUCKET WHOSE START IS <= THE VALUE.  One piece of code for the kernel (tq_agg_range.hip, over the starts in LDS) and for the
// host-only tq_agg_range_bucket_of (tq_agg_range.cpp): integer compares alone, so both give the same index.
//   starts   the buckets' starts in bucket order: non-decreasing, starts[0] == 0 (tq_agg_range_plan's: the plan covers the
//            whole u64 space, so every value has a bucket and UINT64_MAX falls into the last one)
//   strictly increasing starts: the reference's binary_search_by_key(..).unwrap_or_else(|p| p - 1)
//            (src/aggregation/bucket/range.rs:431-437)
//   equal starts (an empty range [s, s) in front of its successor): the LAST of them, so the empty range counts nothing —
//            what [s, s) contains; the reference's result there depends on which equal element its binary search meets
// Branch-free, and the trip count depends on n alone (ceil(log2 n) steps): a wavefront's lanes run in step.
#pragma once
#include <cstdint>

#if defined(__HIP__) || defined(__HIPCC__)
#define TQ_RNG_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define TQ_RNG_HD inline
#endif

// the answer stays inside [base, base + len), and starts[base] <= value (base == 0: by starts[0] == 0); n == 0: 0
TQ_RNG_HD uint32_t tq_range_bucket_of(const uint64_t *starts, uint32_t n, uint64_t value) {
  uint32_t base = 0u;
  for (uint32_t len = n; len > 1u;) {
    const uint32_t half = len >> 1;
    base = starts[base + half] <= value ? base + half : base;
    len -= half;
  }
  return base;
}
