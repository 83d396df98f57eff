// tq_agg_terms.hip — terms aggregation (tq_agg_terms_batch*): the top `segment_size` values of a fast-field column by doc
// count or by key, per query of a batch (src/aggregation/bucket/term_agg/mod.rs:836-899 SegmentTermCollector::collect,
// :1000-1111 into_intermediate_bucket_result, :1328-1353 cut_off_buckets).  The keys are exact integers: a value's index is
// (value - min) / gcd, the number the Bitpacked and BlockwiseLinear readers return as it stands; no f64 anywhere.
//
// count    agg_kernel's walk (a fourth copy: tq_agg.hip, tq_agg_sub.hip and tq_sort.hip keep their code objects byte for
//          byte, and with them the register tables of DESIGN.md 3.4h-j): workgroup = (query, slice of the bitmap words),
//          four wavefronts, docset_word per lane, the popcount prefix sum, the LDS slab, one lane per matching doc for
//          rg_row + rg_value.  A doc with a value adds one to its key's entry of the workgroup's uint32 LDS table
//          (n_keys <= min(lds_buckets, CAP); a table of 2 048 or of 8 192 entries, two instantiations), flushed with one
//          vector atomic add per non-zero entry, or above the capacity to the query's scratch row directly.  Per-lane
//          matches / valued / out-of-range counts are reduced by shuffles and LDS and published by one lane.
// select   one workgroup per query, once behind the last sub-batch: over the query's scratch row a composite key per
//          non-empty entry — unique per entry, so nothing ties: COUNT_DESC (count << 17) | (0x1FFFF - idx), COUNT_ASC the
//          same with 0x7FFFFFFF - count, KEY_ASC 0x1FFFF - idx, KEY_DESC idx + 1 — of which the segment_size LARGEST
//          survive.  The segment_size-th largest key is found exactly by an MSB-first radix select, 8 bits a pass with a
//          256-bin LDS histogram; one more pass compacts the survivors into LDS, sums their counts and finds the largest
//          key below the cut (entry number segment_size: its count is the error bound); a bitonic sort in LDS orders the
//          survivors; rows and record are written with plain vector stores.  Integer arithmetic only: deterministic.
// init     the records (zeros) and entries [0, n_keys) of every scratch row, in front of the first count launch.
// Plain vector stores and vector atomics only.  Nothing is written at or past n_keys of a scratch row (an index outside
// [0, n_keys) — none, by the column's own min / max / gcd — is counted in out_of_range and dropped), nor at or past
// n_returned of an output row.  HBM model: agg_kernel's bitmap-word and per-valued-doc terms + per query 4 x n_keys (the row
// the selection reads) + 12 x n_returned + the 40-byte record.
#include <algorithm>

#include "tq_column_read.hpp"
#include "tq_common.hpp"
#include "tq_docset_word.hpp"
#include "tq_launch.h"

namespace {

constexpr uint32_t AT_THREADS = 256;
constexpr uint32_t AT_WAVES = AT_THREADS / 64;
constexpr uint32_t AT_CHUNK_WORDS = 64;                  // one word per lane
constexpr uint32_t AT_CHUNK_DOCS = AT_CHUNK_WORDS * 32;  // slab entries per wavefront
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
constexpr uint32_t AT_MAX_SIZE = 1024;  // TQ_AGG_TERMS_MAX_SIZE: survivors sorted in LDS
constexpr uint32_t AT_MAX_KEYS = 65536;  // TQ_AGG_MAX_BUCKETS: an index fits the composite key's 17 low bits
constexpr uint32_t AT_COUNT_DESC = 0, AT_COUNT_ASC = 1, AT_KEY_ASC = 2, AT_KEY_DESC = 3;  // TQ_TERMS_ORDER_*

__device__ __forceinline__ unsigned long long at_wave_sum64(unsigned long long v) {
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  return v;
}

__device__ __forceinline__ unsigned long long at_wave_max64(unsigned long long v) {
  for (int off = 32; off > 0; off >>= 1) {
    const unsigned long long u = __shfl_down(v, off, 64);
    v = u > v ? u : v;
  }
  return v;
}

template <bool OPTIONAL, uint32_t CAP>
__global__ __launch_bounds__(AT_THREADS) void agg_terms_count_kernel(TqkAggTermsParams p) {
  __shared__ uint16_t slabs[AT_WAVES * AT_CHUNK_DOCS];
  __shared__ uint32_t table[CAP];
  __shared__ unsigned long long part[AT_WAVES][3];
  const int lane = (int)__lane_id();
  const uint32_t wave = threadIdx.x >> 6;
  const uint32_t q = blockIdx.x % p.ds.n_queries, slice = blockIdx.x / p.ds.n_queries;
  const TqkDocsetQuery *Q = p.ds.queries + q;
  const DocsetHead h = docset_head(Q);
  uint16_t *const slab = slabs + wave * AT_CHUNK_DOCS;
  const uint64_t w0_64 = (uint64_t)slice * p.words_per_slice;
  const uint64_t w1_64 = w0_64 + p.words_per_slice;
  const uint32_t w0 = w0_64 < p.ds.n_words ? (uint32_t)w0_64 : p.ds.n_words;  // (a slice past the end: empty)
  const uint32_t w1 = w1_64 < p.ds.n_words ? (uint32_t)w1_64 : p.ds.n_words;
  const uint32_t n_keys = p.n_keys;
  const bool in_lds = n_keys <= p.lds_buckets && n_keys <= CAP;  // (uniform)
  const uint32_t codec = p.col.codec;                             // (uniform)
  const bool divide = p.gcd > 1ull;                               // (uniform; Linear alone)
  uint32_t *const row = p.rows + (size_t)q * n_keys;
  if (in_lds) {
    for (uint32_t i = threadIdx.x; i < n_keys; i += AT_THREADS) table[i] = 0u;
    __syncthreads();
  }
  uint32_t cnt = 0, valued = 0, oor = 0;  // per lane
  for (uint32_t base = w0 + wave * AT_CHUNK_WORDS; base < w1; base += AT_WAVES * AT_CHUNK_WORDS) {
    const uint32_t w = base + (uint32_t)lane;
    uint32_t res = w < w1 ? docset_word(Q, h, p.ds, w) : 0u;
    const uint32_t pc = (uint32_t)__popc(res);
    cnt += pc;
    const uint32_t incl = wave_incl_sum(pc, lane);
    const uint32_t total = (uint32_t)__shfl(incl, 63, 64);  // <= AT_CHUNK_DOCS
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
        ++valued;
        uint64_t idx;  // (value - min) / gcd: what the packed codecs store; Linear holds the value itself
        if (codec == TQK_COL_LINEAR) {
          idx = rg_value<TQK_COL_LINEAR>(p.col, r) - p.min_value;  // (a value below min wraps to a huge index)
          if (divide) idx /= p.gcd;
        } else {
          idx = codec == TQK_COL_BITPACKED ? rg_value<TQK_COL_BITPACKED>(p.col, r) : rg_value<TQK_COL_BLOCKWISE>(p.col, r);
        }
        if (idx < (uint64_t)n_keys) {
          if (in_lds)
            atomicAdd(&table[(uint32_t)idx], 1u);
          else
            atomicAdd(row + (uint32_t)idx, 1u);
        } else {
          ++oor;
        }
      }
    }
    wave_mem_fence();  // (the next chunk's expansion writes the slab again)
  }
  // the wavefront's part, then the workgroup's
  const unsigned long long t_cnt = at_wave_sum64(cnt), t_val = at_wave_sum64(valued), t_oor = at_wave_sum64(oor);
  if (lane == 0) {
    part[wave][0] = t_cnt;
    part[wave][1] = t_val;
    part[wave][2] = t_oor;
  }
  __syncthreads();  // (also: every wavefront's LDS table adds are done)
  if (in_lds) {
    for (uint32_t i = threadIdx.x; i < n_keys; i += AT_THREADS) {
      const uint32_t c = table[i];
      if (c) atomicAdd(row + i, c);
    }
  }
  if (threadIdx.x != 0u) return;
  unsigned long long matches = 0, count = 0, out_of_range = 0;
  for (uint32_t v = 0; v < AT_WAVES; ++v) {
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

// the composite key of entry idx (< AT_MAX_KEYS) with count c (1 .. 2^31 - 1): never 0, unique per entry, the order's first
// entry the largest
__device__ __forceinline__ unsigned long long at_key(uint32_t order, uint32_t idx, uint32_t c) {
  const unsigned long long up = 0x1FFFFull - idx;  // ascending key: the smaller index the larger
  if (order == AT_COUNT_DESC) return ((unsigned long long)c << 17) | up;
  if (order == AT_COUNT_ASC) return ((unsigned long long)(0x7FFFFFFFu - c) << 17) | up;
  if (order == AT_KEY_ASC) return up;
  return (unsigned long long)idx + 1ull;
}

__device__ __forceinline__ uint32_t at_idx(uint32_t order, unsigned long long key) {
  const uint32_t low = (uint32_t)key & 0x1FFFFu;
  return order == AT_KEY_DESC ? low - 1u : 0x1FFFFu - low;
}

// grid = n_queries
__global__ __launch_bounds__(AT_THREADS) void agg_terms_select_kernel(TqkAggTermsSelectParams p) {
  __shared__ uint32_t hist[256];
  __shared__ unsigned long long skeys[AT_MAX_SIZE];
  __shared__ unsigned long long red[AT_WAVES][4];
  __shared__ uint32_t sel[2];  // the pass's digit, what remains to be taken inside it
  __shared__ uint32_t n_out;
  const uint32_t tid = threadIdx.x, wave = tid >> 6;
  const int lane = (int)__lane_id();
  const uint32_t q = blockIdx.x, n_keys = p.n_keys, order = p.order;
  const uint32_t *const row = p.rows + (size_t)q * n_keys;
  // pass 0: the entries and the docs they hold
  uint32_t d = 0;
  unsigned long long tot = 0ull;
  for (uint32_t i = tid; i < n_keys; i += AT_THREADS) {
    const uint32_t c = row[i];
    d += c ? 1u : 0u;
    tot += c;
  }
  const unsigned long long w_d = at_wave_sum64(d), w_tot = at_wave_sum64(tot);
  if (lane == 0) {
    red[wave][0] = w_d;
    red[wave][1] = w_tot;
  }
  if (tid == 0u) n_out = 0u;
  __syncthreads();
  uint32_t distinct = 0;
  unsigned long long total = 0ull;
  for (uint32_t v = 0; v < AT_WAVES; ++v) {
    distinct += (uint32_t)red[v][0];
    total += red[v][1];
  }
  const uint32_t S = p.segment_size;  // 1 .. AT_MAX_SIZE
  const uint32_t n_ret = distinct < S ? distinct : S;
  unsigned long long cut = 1ull;  // entries whose key is >= cut survive (distinct <= S: every entry, keys are >= 1)
  if (distinct > S) {
    // the S-th largest key, MSB first: the entries that share the digits chosen so far are counted by their next digit
    unsigned long long prefix = 0ull, mask = 0ull;
    uint32_t remaining = S;
    for (int shift = order <= AT_COUNT_ASC ? 40 : 16; shift >= 0; shift -= 8) {
      hist[tid] = 0u;
      __syncthreads();
      for (uint32_t i = tid; i < n_keys; i += AT_THREADS) {
        const uint32_t c = row[i];
        if (c) {
          const unsigned long long k = at_key(order, i, c);
          if ((k & mask) == prefix) atomicAdd(&hist[(uint32_t)(k >> shift) & 255u], 1u);
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
      prefix |= (unsigned long long)sel[0] << shift;
      mask |= 255ull << shift;
      remaining = sel[1];
    }
    cut = prefix;  // (keys are unique: exactly S of them are >= it)
  }
  // the survivors into LDS, their docs, and the largest key below the cut
  unsigned long long kept = 0ull, next = 0ull;
  for (uint32_t i = tid; i < n_keys; i += AT_THREADS) {
    const uint32_t c = row[i];
    if (c) {
      const unsigned long long k = at_key(order, i, c);
      if (k >= cut) {
        const uint32_t at = atomicAdd(&n_out, 1u);
        if (at < AT_MAX_SIZE) skeys[at] = k;
        kept += c;
      } else {
        next = k > next ? k : next;
      }
    }
  }
  uint32_t pow2 = 1u;
  while (pow2 < n_ret) pow2 <<= 1;  // <= AT_MAX_SIZE
  const unsigned long long w_kept = at_wave_sum64(kept), w_next = at_wave_max64(next);
  if (lane == 0) {
    red[wave][2] = w_kept;
    red[wave][3] = w_next;
  }
  __syncthreads();  // (n_out == n_ret entries of skeys are written)
  for (uint32_t i = n_ret + tid; i < pow2; i += AT_THREADS) skeys[i] = 0ull;  // (below every key)
  __syncthreads();
  // bitonic sort, descending
  for (uint32_t k = 2u; k <= pow2; k <<= 1) {
    for (uint32_t j = k >> 1; j > 0u; j >>= 1) {
      for (uint32_t t = tid; t < (pow2 >> 1); t += AT_THREADS) {
        const uint32_t i = ((t & ~(j - 1u)) << 1) | (t & (j - 1u)), l = i | j;
        const unsigned long long a = skeys[i], b = skeys[l];
        const bool desc = (i & k) == 0u;
        if (desc ? a < b : a > b) {
          skeys[i] = b;
          skeys[l] = a;
        }
      }
      __syncthreads();
    }
  }
  const uint32_t n_write = n_ret < p.out_stride ? n_ret : p.out_stride;  // (the host checked: n_ret <= out_stride)
  for (uint32_t j = tid; j < n_write; j += AT_THREADS) {
    const uint32_t idx = at_idx(order, skeys[j]);
    p.out_keys[(size_t)q * p.out_stride + j] = p.min_value + p.gcd * (unsigned long long)idx;
    p.out_counts[(size_t)q * p.out_stride + j] = row[idx];
  }
  if (tid != 0u) return;
  unsigned long long kept_all = 0ull, next_all = 0ull;
  for (uint32_t v = 0; v < AT_WAVES; ++v) {
    kept_all += red[v][2];
    next_all = red[v][3] > next_all ? red[v][3] : next_all;
  }
  TqkAggTerms *const R = p.records + q;
  R->sum_other_doc_count = total - kept_all;
  R->distinct = distinct;
  R->n_returned = n_ret;
  R->doc_count_error_upper_bound = next_all ? row[at_idx(order, next_all)] : 0u;
  if (n_ret) atomicAdd(p.totals + 3, (unsigned long long)n_ret);
}

// record q = zeros; entries [0, n_keys) of scratch row q = 0.  grid = n_queries
__global__ __launch_bounds__(AT_THREADS) void agg_terms_init_kernel(TqkAggTerms *records, uint32_t *rows, uint32_t n_keys) {
  const uint32_t q = blockIdx.x;
  if (threadIdx.x < 5u) reinterpret_cast<unsigned long long *>(records + q)[threadIdx.x] = 0ull;
  uint32_t *const row = rows + (size_t)q * n_keys;
  for (uint32_t i = threadIdx.x; i < n_keys; i += AT_THREADS) row[i] = 0u;
}

template <uint32_t CAP>
void agg_terms_launch(const TqkAggTermsParams &p, hipStream_t st) {
  const dim3 grid(p.ds.n_queries * p.n_slices), block(AT_THREADS);
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

uint32_t tqk_agg_terms_max_size() { return AT_MAX_SIZE; }

hipError_t tqk_launch_agg_terms_init(TqkAggTerms *records, uint32_t *rows, uint32_t n_queries, uint32_t n_keys, hipStream_t st) {
  if (!n_queries) return hipSuccess;
  if (!records || (n_keys && !rows)) return hipErrorInvalidValue;
  agg_terms_init_kernel<<<dim3(n_queries), dim3(AT_THREADS), 0, st>>>(records, rows, n_keys);
  return hipGetLastError();
}

hipError_t tqk_launch_agg_terms_count(const TqkAggTermsParams &p, hipStream_t st) {
  if (!p.ds.n_queries || !p.n_slices) return hipSuccess;
  if (p.col.codec > TQK_COL_BLOCKWISE || p.gcd == 0ull) return hipErrorInvalidValue;
  if (p.n_keys > AT_MAX_KEYS || (p.n_keys && !p.rows) || !p.records) return hipErrorInvalidValue;
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
  if (p.n_keys > AT_MAX_KEYS || (p.n_keys && !p.rows) || !p.records || p.order > AT_KEY_DESC) return hipErrorInvalidValue;
  if (p.segment_size == 0u || p.segment_size > AT_MAX_SIZE) return hipErrorInvalidValue;
  if (p.out_stride < std::min(p.segment_size, p.n_keys) || (p.n_keys && (!p.out_keys || !p.out_counts))) return hipErrorInvalidValue;
  agg_terms_select_kernel<<<dim3(p.n_queries), dim3(AT_THREADS), 0, st>>>(p);
  return hipGetLastError();
}
