// tq_agg_terms_sub.hip — terms aggregation with a metric (tq_agg_terms_sub_batch*): per key of a column A its doc count and
// a stats record of a metric column B, and the top `segment_size` entries by doc count, by key, or by one metric of the
// record (src/aggregation/bucket/term_agg/mod.rs:836-899 SegmentTermCollector::collect with a sub-aggregation, :1040-1111
// the order by a sub-aggregation and cut_off_buckets; src/aggregation/metric/stats.rs:282-306, :325-357).  Joins the integer
// key index and the exact selection of tq_agg_terms.hip with the 40-byte record and its LDS table of tq_agg_sub.hip.
//
// count    agg_terms_count_kernel's walk and key index (a fifth copy: tq_agg.hip, tq_agg_sub.hip, tq_agg_terms.hip and
//          tq_sort.hip keep their code objects byte for byte, and with them their register tables).  A counted doc — a value
//          in A, its index inside [0, n_keys) — then takes rg_row + rg_value of B (a doc that is not counted, or has no
//          value in B, loads nothing of B) and adds to
//            - the key's entry of the workgroup's LDS table (n_keys <= min(lds_buckets, CAP); a SMALL and a LARGE table):
//              ONE 64-bit add on {doc count | value count << 32} (each below 2^31: the low word cannot carry), and for a
//              doc with a value ds min / max and two 64-bit adds on the sums of the value's 32-bit halves;
//            - or, above the capacity, the query's count row and record row in global memory, per doc.
//          The table is flushed once: vector atomics on the rows, the 128-bit sum low word first, carrying where it wrapped.
// select   one workgroup per query, once behind the last sub-batch: agg_terms_select_kernel's selection over a composite
//          key of up to 113 bits held as two 64-bit words.  The four old orders use that kernel's keys.  The metric orders:
//          (image, or its complement for ASC) << 17 | (0x1FFFF - idx), the image of tq_agg_metric_image.hpp — unique per
//          entry, so nothing ties, and ties of the metric go to the ascending key.  The radix select walks 8 bits a pass
//          over the image's width (32 / 64 / 96) plus the 17 index bits; the bitonic sort runs over at most 1 024 16-byte
//          keys in LDS; the survivors' key, doc count and record are written with plain stores.
// init     the records (zeros), the count rows (zeros) and the record rows (zeros with min_value = ~0), [0, n_keys) each.
// Integer arithmetic and integer atomics only: deterministic.  Plain vector stores and vector atomics; nothing is written at
// or past n_keys of a scratch row, nor at or past n_returned of an output row.  HBM model: tq_agg_terms.hip's + 8 per
// counted doc with a value in B + 8 per counted doc of an Optional B (its presence word) + 40 x n_keys per query + 40 per
// entry returned.
#include <algorithm>

#include "tq_agg_metric_image.hpp"
#include "tq_column_read.hpp"
#include "tq_common.hpp"
#include "tq_docset_word.hpp"
#include "tq_launch.h"

namespace {

constexpr uint32_t TS_THREADS = 256;
constexpr uint32_t TS_WAVES = TS_THREADS / 64;
constexpr uint32_t TS_CHUNK_WORDS = 64;                  // one word per lane
constexpr uint32_t TS_CHUNK_DOCS = TS_CHUNK_WORDS * 32;  // slab entries per wavefront
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
static_assert(TS_LDS_LARGE * 40u + TS_WAVES * TS_CHUNK_DOCS * 2u + TS_WAVES * TS_PART * 8u <= 65536u, "the static LDS of a workgroup");
constexpr uint32_t TS_MAX_SIZE = 1024;   // TQ_AGG_TERMS_MAX_SIZE: survivors sorted in LDS
constexpr uint32_t TS_MAX_KEYS = 65536;  // TQ_AGG_MAX_BUCKETS: an index fits the composite key's 17 low bits
constexpr uint32_t TS_COUNT_DESC = 0, TS_COUNT_ASC = 1, TS_KEY_ASC = 2, TS_KEY_DESC = 3, TS_METRIC_DESC = 4, TS_METRIC_ASC = 5;  // TQ_TERMS_*
constexpr uint32_t TS_VALUE_F64 = 2;  // TQ_VALUE_F64

__device__ __forceinline__ uint64_t ts_value(const TqkColumn &col, uint64_t min_value, uint64_t gcd, uint32_t row) {
  const uint32_t codec = col.codec;  // (uniform)
  if (codec == TQK_COL_LINEAR) return rg_value<TQK_COL_LINEAR>(col, row);
  const uint64_t n = codec == TQK_COL_BITPACKED ? rg_value<TQK_COL_BITPACKED>(col, row) : rg_value<TQK_COL_BLOCKWISE>(col, row);
  return min_value + gcd * n;
}

__device__ __forceinline__ unsigned long long ts_wave_sum64(unsigned long long v) {
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  return v;
}

// *sum_lo / *sum_hi (128 bits) += lo + hi * 2^32 (lo, hi < 2^63), low word first: a wrapped add carries into the high word;
// the number of wraps does not depend on the order of the adders
__device__ __forceinline__ void ts_add128(unsigned long long *sum_lo, unsigned long long *sum_hi, unsigned long long lo,
                                          unsigned long long hi) {
  const unsigned long long add_lo = lo + (hi << 32);
  const unsigned long long add_hi = (hi >> 32) + (add_lo < lo ? 1ull : 0ull);
  const unsigned long long old = atomicAdd(sum_lo, add_lo);
  const unsigned long long carry = old + add_lo < old ? 1ull : 0ull;
  if (add_hi + carry) atomicAdd(sum_hi, add_hi + carry);
}

template <bool OPTIONAL_A, bool OPTIONAL_B, uint32_t CAP>
__global__ __launch_bounds__(TS_THREADS) void agg_terms_sub_count_kernel(TqkAggTermsSubParams p) {
  __shared__ uint16_t slabs[TS_WAVES * TS_CHUNK_DOCS];
  // the table, one array per field: {doc count | value count << 32}, min, max, the sums of the low and of the high halves
  __shared__ unsigned long long t_cv[CAP], t_mn[CAP], t_mx[CAP], t_lo[CAP], t_hi[CAP];
  __shared__ unsigned long long part[TS_WAVES][TS_PART];
  const int lane = (int)__lane_id();
  const uint32_t wave = threadIdx.x >> 6;
  const uint32_t q = blockIdx.x % p.t.ds.n_queries, slice = blockIdx.x / p.t.ds.n_queries;
  const TqkDocsetQuery *Q = p.t.ds.queries + q;
  const DocsetHead h = docset_head(Q);
  uint16_t *const slab = slabs + wave * TS_CHUNK_DOCS;
  const uint64_t w0_64 = (uint64_t)slice * p.t.words_per_slice;
  const uint64_t w1_64 = w0_64 + p.t.words_per_slice;
  const uint32_t w0 = w0_64 < p.t.ds.n_words ? (uint32_t)w0_64 : p.t.ds.n_words;  // (a slice past the end: empty)
  const uint32_t w1 = w1_64 < p.t.ds.n_words ? (uint32_t)w1_64 : p.t.ds.n_words;
  const uint32_t n_keys = p.t.n_keys;
  const bool in_lds = n_keys <= p.t.lds_buckets && n_keys <= CAP;  // (uniform)
  const uint32_t codec = p.t.col.codec;                             // (uniform)
  const bool divide = p.t.gcd > 1ull;                               // (uniform; Linear alone)
  const bool sum_b = p.value_type_b != TS_VALUE_F64;                // (uniform; F64: both sum words stay 0)
  uint32_t *const row = p.t.rows + (size_t)q * n_keys;
  TqkAggBucketStats *const recs = p.stats + (size_t)q * n_keys;
  if (in_lds) {
    for (uint32_t i = threadIdx.x; i < n_keys; i += TS_THREADS) {
      t_cv[i] = 0ull;
      t_mn[i] = ~0ull;
      t_mx[i] = 0ull;
      t_lo[i] = 0ull;
      t_hi[i] = 0ull;
    }
    __syncthreads();
  }
  uint32_t cnt = 0, valued = 0, oor = 0, counted = 0, valued_b = 0;  // per lane
  for (uint32_t base = w0 + wave * TS_CHUNK_WORDS; base < w1; base += TS_WAVES * TS_CHUNK_WORDS) {
    const uint32_t w = base + (uint32_t)lane;
    uint32_t res = w < w1 ? docset_word(Q, h, p.t.ds, w) : 0u;
    const uint32_t pc = (uint32_t)__popc(res);
    cnt += pc;
    const uint32_t incl = wave_incl_sum(pc, lane);
    const uint32_t total = (uint32_t)__shfl(incl, 63, 64);  // <= TS_CHUNK_DOCS
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
      if (has && rg_row<OPTIONAL_A>(p.t.col, doc, r)) {
        ++valued;
        uint64_t idx64;  // (value - min) / gcd: what the packed codecs store; Linear holds the value itself
        if (codec == TQK_COL_LINEAR) {
          idx64 = rg_value<TQK_COL_LINEAR>(p.t.col, r) - p.t.min_value;  // (a value below min wraps to a huge index)
          if (divide) idx64 /= p.t.gcd;
        } else {
          idx64 = codec == TQK_COL_BITPACKED ? rg_value<TQK_COL_BITPACKED>(p.t.col, r) : rg_value<TQK_COL_BLOCKWISE>(p.t.col, r);
        }
        if (idx64 < (uint64_t)n_keys) {
          const uint32_t idx = (uint32_t)idx64;
          ++counted;
          uint32_t rb = 0;
          const bool has_b = rg_row<OPTIONAL_B>(p.col_b, doc, rb);
          const uint64_t vb = has_b ? ts_value(p.col_b, p.min_value_b, p.gcd_b, rb) : 0ull;
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
              if (sum_b) ts_add128(&R->sum_lo, &R->sum_hi, vb & 0xFFFFFFFFull, vb >> 32);
            }
          }
        } else {
          ++oor;
        }
      }
    }
    wave_mem_fence();  // (the next chunk's expansion writes the slab again)
  }
  // the wavefront's part, then the workgroup's
  const unsigned long long t_cnt = ts_wave_sum64(cnt), t_val = ts_wave_sum64(valued), t_oor = ts_wave_sum64(oor);
  const unsigned long long t_ctd = ts_wave_sum64(counted), t_vb = ts_wave_sum64(valued_b);
  if (lane == 0) {
    part[wave][0] = t_cnt;
    part[wave][1] = t_val;
    part[wave][2] = t_oor;
    part[wave][3] = t_ctd;
    part[wave][4] = t_vb;
  }
  __syncthreads();  // (also: every wavefront's LDS table updates are done)
  if (in_lds) {
    for (uint32_t i = threadIdx.x; i < n_keys; i += TS_THREADS) {
      const unsigned long long cv = t_cv[i];
      const uint32_t docs = (uint32_t)cv;
      const unsigned long long vals = cv >> 32;
      if (docs) atomicAdd(row + i, docs);
      if (vals) {
        TqkAggBucketStats *const R = recs + i;
        atomicAdd(&R->count, vals);
        atomicMin(&R->min_value, t_mn[i]);
        atomicMax(&R->max_value, t_mx[i]);
        if (sum_b) ts_add128(&R->sum_lo, &R->sum_hi, t_lo[i], t_hi[i]);
      }
    }
  }
  if (threadIdx.x != 0u) return;
  unsigned long long matches = 0, count = 0, out_of_range = 0, in_keys = 0, with_b = 0;
  for (uint32_t v = 0; v < TS_WAVES; ++v) {
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

// ---- the selection.  A composite key, 128 bits: never 0, unique per entry, the order's first entry the largest.
struct TsKey {
  unsigned long long hi, lo;
};

__device__ __forceinline__ bool ts_less(const TsKey &a, const TsKey &b) { return a.hi < b.hi || (a.hi == b.hi && a.lo < b.lo); }

// entry idx (< TS_MAX_KEYS) with doc count c (1 .. 2^31 - 1) and record R (read under a metric order alone)
__device__ __forceinline__ TsKey ts_key(uint32_t order, uint32_t metric, uint32_t value_type, uint32_t idx, uint32_t c,
                                        const TqkAggBucketStats *R) {
  const unsigned long long up = 0x1FFFFull - idx;  // ascending key: the smaller index the larger
  if (order == TS_COUNT_DESC) return TsKey{0ull, ((unsigned long long)c << 17) | up};
  if (order == TS_COUNT_ASC) return TsKey{0ull, ((unsigned long long)(0x7FFFFFFFu - c) << 17) | up};
  if (order == TS_KEY_ASC) return TsKey{0ull, up};
  if (order == TS_KEY_DESC) return TsKey{0ull, (unsigned long long)idx + 1ull};
  TqImage im = tq_metric_image(R->count, R->min_value, R->max_value, R->sum_lo, R->sum_hi, value_type, metric);
  if (order == TS_METRIC_ASC) {  // the complement inside the image's width: the smallest image the largest key
    const uint32_t bits = tq_image_bits(metric);
    im.lo = bits == 32u ? 0xFFFFFFFFull - im.lo : ~im.lo;
    im.hi = bits == 96u ? 0xFFFFFFFFull - im.hi : 0ull;
  }
  return TsKey{(im.hi << 17) | (im.lo >> 47), (im.lo << 17) | up};
}

__device__ __forceinline__ uint32_t ts_idx(uint32_t order, const TsKey &key) {
  const uint32_t low = (uint32_t)key.lo & 0x1FFFFu;
  return order == TS_KEY_DESC ? low - 1u : 0x1FFFFu - low;
}

// the 8-bit digit at `shift` (a multiple of 8: no digit straddles the words)
__device__ __forceinline__ uint32_t ts_digit(const TsKey &k, int shift) {
  return (uint32_t)(shift >= 64 ? k.hi >> (shift - 64) : k.lo >> shift) & 255u;
}

// grid = n_queries
__global__ __launch_bounds__(TS_THREADS) void agg_terms_sub_select_kernel(TqkAggTermsSubSelectParams p) {
  __shared__ uint32_t hist[256];
  __shared__ unsigned long long skeys_hi[TS_MAX_SIZE], skeys_lo[TS_MAX_SIZE];
  __shared__ unsigned long long red[TS_WAVES][5];
  __shared__ uint32_t sel[2];  // the pass's digit, what remains to be taken inside it
  __shared__ uint32_t n_out;
  const uint32_t tid = threadIdx.x, wave = tid >> 6;
  const int lane = (int)__lane_id();
  const uint32_t q = blockIdx.x, n_keys = p.s.n_keys, order = p.s.order, metric = p.metric, vt = p.value_type_b;
  const uint32_t *const row = p.s.rows + (size_t)q * n_keys;
  const TqkAggBucketStats *const recs = p.stats + (size_t)q * n_keys;
  // pass 0: the entries and the docs they hold
  uint32_t d = 0;
  unsigned long long tot = 0ull;
  for (uint32_t i = tid; i < n_keys; i += TS_THREADS) {
    const uint32_t c = row[i];
    d += c ? 1u : 0u;
    tot += c;
  }
  const unsigned long long w_d = ts_wave_sum64(d), w_tot = ts_wave_sum64(tot);
  if (lane == 0) {
    red[wave][0] = w_d;
    red[wave][1] = w_tot;
  }
  if (tid == 0u) n_out = 0u;
  __syncthreads();
  uint32_t distinct = 0;
  unsigned long long total = 0ull;
  for (uint32_t v = 0; v < TS_WAVES; ++v) {
    distinct += (uint32_t)red[v][0];
    total += red[v][1];
  }
  const uint32_t S = p.s.segment_size;  // 1 .. TS_MAX_SIZE
  const uint32_t n_ret = distinct < S ? distinct : S;
  TsKey cut{0ull, 1ull};  // entries whose key is >= cut survive (distinct <= S: every entry, keys are >= 1)
  if (distinct > S) {
    // the S-th largest key, MSB first: the entries that share the digits chosen so far are counted by their next digit
    TsKey prefix{0ull, 0ull}, mask{0ull, 0ull};
    uint32_t remaining = S;
    // the key's bits, rounded up to whole digits: 48 / 24 for the old orders, the image's width + 17 for a metric order
    const int top = order <= TS_COUNT_ASC ? 40 : order <= TS_KEY_DESC ? 16 : (int)((tq_image_bits(metric) + 17u + 7u) & ~7u) - 8;
    for (int shift = top; shift >= 0; shift -= 8) {
      hist[tid] = 0u;
      __syncthreads();
      for (uint32_t i = tid; i < n_keys; i += TS_THREADS) {
        const uint32_t c = row[i];
        if (c) {
          const TsKey k = ts_key(order, metric, vt, i, c, recs + i);
          if ((k.hi & mask.hi) == prefix.hi && (k.lo & mask.lo) == prefix.lo) atomicAdd(&hist[ts_digit(k, shift)], 1u);
        }
      }
      __syncthreads();
      if (wave == 0u) {  // lane l holds bins 255 - 4l .. 252 - 4l: a prefix sum from the top bin down
        const uint32_t b0 = 255u - 4u * (uint32_t)lane;
        const uint32_t c0 = hist[b0], c1 = hist[b0 - 1u], c2 = hist[b0 - 2u], c3 = hist[b0 - 3u];
        const uint32_t mine = c0 + c1 + c2 + c3;
        const uint32_t incl = wave_incl_sum(mine, lane);
        const uint32_t excl = incl - mine;
        if (excl < remaining && remaining <= incl) {  // (one lane: remaining <= the entries under the prefix)
          uint32_t r = remaining - excl, digit = b0;
          if (r > c0) {
            r -= c0;
            digit = b0 - 1u;
            if (r > c1) {
              r -= c1;
              digit = b0 - 2u;
              if (r > c2) {
                r -= c2;
                digit = b0 - 3u;
              }
            }
          }
          sel[0] = digit;
          sel[1] = r;
        }
      }
      __syncthreads();
      if (shift >= 64) {
        prefix.hi |= (unsigned long long)sel[0] << (shift - 64);
        mask.hi |= 255ull << (shift - 64);
      } else {
        prefix.lo |= (unsigned long long)sel[0] << shift;
        mask.lo |= 255ull << shift;
      }
      remaining = sel[1];
    }
    cut = prefix;  // (keys are unique: exactly S of them are >= it)
  }
  // the survivors into LDS, their docs, and the largest key below the cut
  unsigned long long kept = 0ull;
  TsKey next{0ull, 0ull};
  for (uint32_t i = tid; i < n_keys; i += TS_THREADS) {
    const uint32_t c = row[i];
    if (c) {
      const TsKey k = ts_key(order, metric, vt, i, c, recs + i);
      if (!ts_less(k, cut)) {
        const uint32_t at = atomicAdd(&n_out, 1u);
        if (at < TS_MAX_SIZE) {
          skeys_hi[at] = k.hi;
          skeys_lo[at] = k.lo;
        }
        kept += c;
      } else if (ts_less(next, k)) {
        next = k;
      }
    }
  }
  uint32_t pow2 = 1u;
  while (pow2 < n_ret) pow2 <<= 1;  // <= TS_MAX_SIZE
  const unsigned long long w_kept = ts_wave_sum64(kept);
  for (int off = 32; off > 0; off >>= 1) {
    const TsKey o{__shfl_down(next.hi, off, 64), __shfl_down(next.lo, off, 64)};
    if (ts_less(next, o)) next = o;
  }
  if (lane == 0) {
    red[wave][2] = w_kept;
    red[wave][3] = next.hi;
    red[wave][4] = next.lo;
  }
  __syncthreads();  // (n_out == n_ret entries of skeys are written)
  for (uint32_t i = n_ret + tid; i < pow2; i += TS_THREADS) {  // (below every key)
    skeys_hi[i] = 0ull;
    skeys_lo[i] = 0ull;
  }
  __syncthreads();
  // bitonic sort, descending
  for (uint32_t k = 2u; k <= pow2; k <<= 1) {
    for (uint32_t j = k >> 1; j > 0u; j >>= 1) {
      for (uint32_t t = tid; t < (pow2 >> 1); t += TS_THREADS) {
        const uint32_t i = ((t & ~(j - 1u)) << 1) | (t & (j - 1u)), l = i | j;
        const TsKey a{skeys_hi[i], skeys_lo[i]}, b{skeys_hi[l], skeys_lo[l]};
        const bool desc = (i & k) == 0u;
        if (desc ? ts_less(a, b) : ts_less(b, a)) {
          skeys_hi[i] = b.hi;
          skeys_lo[i] = b.lo;
          skeys_hi[l] = a.hi;
          skeys_lo[l] = a.lo;
        }
      }
      __syncthreads();
    }
  }
  const uint32_t n_write = n_ret < p.s.out_stride ? n_ret : p.s.out_stride;  // (the host checked: n_ret <= out_stride)
  for (uint32_t j = tid; j < n_write; j += TS_THREADS) {
    const uint32_t idx = ts_idx(order, TsKey{skeys_hi[j], skeys_lo[j]});
    const size_t o = (size_t)q * p.s.out_stride + j;
    p.s.out_keys[o] = p.s.min_value + p.s.gcd * (unsigned long long)idx;
    p.s.out_counts[o] = row[idx];
    p.out_stats[o] = recs[idx];
  }
  if (tid != 0u) return;
  unsigned long long kept_all = 0ull;
  TsKey next_all{0ull, 0ull};
  for (uint32_t v = 0; v < TS_WAVES; ++v) {
    kept_all += red[v][2];
    const TsKey o{red[v][3], red[v][4]};
    if (ts_less(next_all, o)) next_all = o;
  }
  TqkAggTerms *const R = p.s.records + q;
  R->sum_other_doc_count = total - kept_all;
  R->distinct = distinct;
  R->n_returned = n_ret;
  R->doc_count_error_upper_bound = (next_all.hi | next_all.lo) ? row[ts_idx(order, next_all)] : 0u;
  if (n_ret) atomicAdd(p.s.totals + 3, (unsigned long long)n_ret);
}

// record q = zeros; entries [0, n_keys) of count row q = 0, of record row q = zeros with min_value = ~0.  grid = n_queries
__global__ __launch_bounds__(TS_THREADS) void agg_terms_sub_init_kernel(TqkAggTerms *records, uint32_t *rows, TqkAggBucketStats *stats,
                                                                        uint32_t n_keys) {
  const uint32_t q = blockIdx.x;
  if (threadIdx.x < 5u) reinterpret_cast<unsigned long long *>(records + q)[threadIdx.x] = 0ull;
  uint32_t *const row = rows + (size_t)q * n_keys;
  for (uint32_t i = threadIdx.x; i < n_keys; i += TS_THREADS) row[i] = 0u;
  unsigned long long *const words = reinterpret_cast<unsigned long long *>(stats + (size_t)q * n_keys);
  for (uint32_t w = threadIdx.x; w < n_keys * 5u; w += TS_THREADS) words[w] = w % 5u == 1u ? ~0ull : 0ull;
}

template <uint32_t CAP>
void agg_terms_sub_launch(const TqkAggTermsSubParams &p, hipStream_t st) {
  const dim3 grid(p.t.ds.n_queries * p.t.n_slices), block(TS_THREADS);
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
  if (!records || (n_keys && (!rows || !stats)) || n_keys > TS_MAX_KEYS) return hipErrorInvalidValue;
  agg_terms_sub_init_kernel<<<dim3(n_queries), dim3(TS_THREADS), 0, st>>>(records, rows, stats, n_keys);
  return hipGetLastError();
}

hipError_t tqk_launch_agg_terms_sub_count(const TqkAggTermsSubParams &p, hipStream_t st) {
  if (!p.t.ds.n_queries || !p.t.n_slices) return hipSuccess;
  if (p.t.col.codec > TQK_COL_BLOCKWISE || p.col_b.codec > TQK_COL_BLOCKWISE || p.t.gcd == 0ull) return hipErrorInvalidValue;
  if (p.t.n_keys > TS_MAX_KEYS || (p.t.n_keys && (!p.t.rows || !p.stats)) || !p.t.records) return hipErrorInvalidValue;
  const bool global = p.t.n_keys > std::min(p.t.lds_buckets, TS_LDS_LARGE);  // past "agg_lds_buckets" or the large table: straight to the rows
  if (global ? TS_GLOBAL_TABLE == TS_LDS_SMALL : p.t.n_keys <= TS_LDS_SMALL)
    agg_terms_sub_launch<TS_LDS_SMALL>(p, st);
  else
    agg_terms_sub_launch<TS_LDS_LARGE>(p, st);
  return hipGetLastError();
}

hipError_t tqk_launch_agg_terms_sub_select(const TqkAggTermsSubSelectParams &p, hipStream_t st) {
  if (!p.s.n_queries) return hipSuccess;
  if (p.s.n_keys > TS_MAX_KEYS || (p.s.n_keys && (!p.s.rows || !p.stats)) || !p.s.records) return hipErrorInvalidValue;
  if (p.s.order > TS_METRIC_ASC || p.value_type_b > TS_VALUE_F64) return hipErrorInvalidValue;
  if (p.s.order >= TS_METRIC_DESC && (p.metric > TQ_IMG_AVG || (p.metric >= TQ_IMG_SUM && p.value_type_b == TS_VALUE_F64))) return hipErrorInvalidValue;
  if (p.s.segment_size == 0u || p.s.segment_size > TS_MAX_SIZE) return hipErrorInvalidValue;
  if (p.s.out_stride < std::min(p.s.segment_size, p.s.n_keys) || (p.s.n_keys && (!p.s.out_keys || !p.s.out_counts || !p.out_stats)))
    return hipErrorInvalidValue;
  agg_terms_sub_select_kernel<<<dim3(p.s.n_queries), dim3(TS_THREADS), 0, st>>>(p);
  return hipGetLastError();
}
