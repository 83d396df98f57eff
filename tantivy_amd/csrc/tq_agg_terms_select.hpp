// tq_agg_terms_select.hpp — the exact top-N selection of a terms aggregation: the body of agg_terms_select_kernel
// (tq_agg_terms.hip, a 64-bit key; tq_agg_terms_hist.cpp launches it over its totals rows) and agg_terms_sub_select_kernel
// (tq_agg_terms_sub.hip, a 128-bit key).  One workgroup
// per query over the query's count row: a composite key per non-empty entry — never 0, unique per entry, so nothing ties,
// the order's first entry the largest — of which the segment_size LARGEST survive.  The segment_size-th largest key is
// found exactly by an MSB-first radix select, 8 bits a pass with a 256-bin LDS histogram; one more pass compacts the
// survivors into LDS, sums their counts and finds the largest key below the cut (entry number segment_size: its count is
// the error bound); a bitonic sort in LDS orders the survivors; rows and record are written with plain vector stores.
// Integer arithmetic only: deterministic.
//
// The key policy KP (an object: it carries what its keys are made from):
//   KP::Key, KP::WORDS                 the key — with &, |, ==, < and Key{} == 0 — and its 64-bit words in LDS
//   make(idx, c)                       the key of entry idx with doc count c >= 1
//   idx(key)                           the entry of a key
//   top_shift()                        the shift of the key's most significant digit, a multiple of 8
//   KP::at(v, shift), KP::digit(k, shift)   an 8-bit value placed at / read from `shift` (no digit straddles a word)
//   KP::get(a, i), KP::put(a, i, k)    a key in unsigned long long a[WORDS][N], KP::shfl_down(k, off)
//   write(o, idx)                      what a survivor's output slot o takes beside key and doc count
// Internal linkage, like tq_docset_word.hpp.
#pragma once
#include "tq_agg_device.hpp"
#include "tq_common.hpp"
#include "tq_launch.h"

namespace {

constexpr uint32_t TSEL_THREADS = 256;
constexpr uint32_t TSEL_WAVES = TSEL_THREADS / 64;
constexpr uint32_t TERMS_MAX_SIZE = 1024;   // TQ_AGG_TERMS_MAX_SIZE: survivors sorted in LDS
constexpr uint32_t TERMS_MAX_KEYS = 65536;  // TQ_AGG_MAX_BUCKETS: an index fits the composite key's 17 low bits
constexpr uint32_t TERMS_COUNT_DESC = 0, TERMS_COUNT_ASC = 1, TERMS_KEY_ASC = 2, TERMS_KEY_DESC = 3;  // TQ_TERMS_ORDER_*

// the 64-bit composite key of entry idx (< TERMS_MAX_KEYS) with count c (1 .. 2^31 - 1) under the count and key orders
__device__ __forceinline__ unsigned long long terms_key64(uint32_t order, uint32_t idx, uint32_t c) {
  const unsigned long long up = 0x1FFFFull - idx;  // ascending key: the smaller index the larger
  if (order == TERMS_COUNT_DESC) return ((unsigned long long)c << 17) | up;
  if (order == TERMS_COUNT_ASC) return ((unsigned long long)(0x7FFFFFFFu - c) << 17) | up;
  if (order == TERMS_KEY_ASC) return up;
  return (unsigned long long)idx + 1ull;
}

// the entry of a key from its low word: every order but KEY_DESC keeps 0x1FFFF - idx in the 17 low bits
__device__ __forceinline__ uint32_t terms_idx(uint32_t order, unsigned long long key_lo) {
  const uint32_t low = (uint32_t)key_lo & 0x1FFFFu;
  return order == TERMS_KEY_DESC ? low - 1u : 0x1FFFFu - low;
}

// grid = n_queries, TSEL_THREADS threads.  LDS: 1 024 + 8 192 * WORDS + 32 * (3 + WORDS) + 12 bytes.
template <class KP>
__device__ __forceinline__ void terms_select(const TqkAggTermsSelectParams &p, const KP &kp) {
  using Key = typename KP::Key;
  __shared__ uint32_t hist[256];
  __shared__ unsigned long long skeys[KP::WORDS][TERMS_MAX_SIZE];
  __shared__ unsigned long long red[TSEL_WAVES][3];  // entries, their docs; the survivors' docs
  __shared__ unsigned long long red_next[KP::WORDS][TSEL_WAVES];
  __shared__ uint32_t sel[2];  // the pass's digit, what remains to be taken inside it
  __shared__ uint32_t n_out;
  const uint32_t tid = threadIdx.x, wave = tid >> 6;
  const int lane = (int)__lane_id();
  const uint32_t q = blockIdx.x, n_keys = p.n_keys;
  const uint32_t *const row = p.rows + (size_t)q * n_keys;
  // pass 0: the entries and the docs they hold
  uint32_t d = 0;
  unsigned long long tot = 0ull;
  for (uint32_t i = tid; i < n_keys; i += TSEL_THREADS) {
    const uint32_t c = row[i];
    d += c ? 1u : 0u;
    tot += c;
  }
  const unsigned long long w_d = wave_sum64(d), w_tot = wave_sum64(tot);
  if (lane == 0) {
    red[wave][0] = w_d;
    red[wave][1] = w_tot;
  }
  if (tid == 0u) n_out = 0u;
  __syncthreads();
  uint32_t distinct = 0;
  unsigned long long total = 0ull;
  for (uint32_t v = 0; v < TSEL_WAVES; ++v) {
    distinct += (uint32_t)red[v][0];
    total += red[v][1];
  }
  const uint32_t S = p.segment_size;  // 1 .. TERMS_MAX_SIZE
  const uint32_t n_ret = distinct < S ? distinct : S;
  Key cut = KP::at(1u, 0);  // entries whose key is >= cut survive (distinct <= S: every entry, keys are >= 1)
  if (distinct > S) {
    // the S-th largest key, MSB first: the entries that share the digits chosen so far are counted by their next digit
    Key prefix{}, mask{};
    uint32_t remaining = S;
    for (int shift = kp.top_shift(); shift >= 0; shift -= 8) {
      hist[tid] = 0u;
      __syncthreads();
      for (uint32_t i = tid; i < n_keys; i += TSEL_THREADS) {
        const uint32_t c = row[i];
        if (c) {
          const Key k = kp.make(i, c);
          if ((k & mask) == prefix) atomicAdd(&hist[KP::digit(k, shift)], 1u);
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
      prefix = prefix | KP::at(sel[0], shift);
      mask = mask | KP::at(255u, shift);
      remaining = sel[1];
    }
    cut = prefix;  // (keys are unique: exactly S of them are >= it)
  }
  // the survivors into LDS, their docs, and the largest key below the cut
  unsigned long long kept = 0ull;
  Key next{};
  for (uint32_t i = tid; i < n_keys; i += TSEL_THREADS) {
    const uint32_t c = row[i];
    if (c) {
      const Key k = kp.make(i, c);
      if (!(k < cut)) {
        const uint32_t at = atomicAdd(&n_out, 1u);
        if (at < TERMS_MAX_SIZE) KP::put(skeys, at, k);
        kept += c;
      } else if (next < k) {
        next = k;
      }
    }
  }
  uint32_t pow2 = 1u;
  while (pow2 < n_ret) pow2 <<= 1;  // <= TERMS_MAX_SIZE
  const unsigned long long w_kept = wave_sum64(kept);
  for (int off = 32; off > 0; off >>= 1) {
    const Key o = KP::shfl_down(next, off);
    if (next < o) next = o;
  }
  if (lane == 0) {
    red[wave][2] = w_kept;
    KP::put(red_next, wave, next);
  }
  __syncthreads();  // (n_out == n_ret entries of skeys are written)
  for (uint32_t i = n_ret + tid; i < pow2; i += TSEL_THREADS) KP::put(skeys, i, Key{});  // (below every key)
  __syncthreads();
  // bitonic sort, descending
  for (uint32_t k = 2u; k <= pow2; k <<= 1) {
    for (uint32_t j = k >> 1; j > 0u; j >>= 1) {
      for (uint32_t t = tid; t < (pow2 >> 1); t += TSEL_THREADS) {
        const uint32_t i = ((t & ~(j - 1u)) << 1) | (t & (j - 1u)), l = i | j;
        const Key a = KP::get(skeys, i), b = KP::get(skeys, l);
        const bool desc = (i & k) == 0u;
        if (desc ? a < b : b < a) {
          KP::put(skeys, i, b);
          KP::put(skeys, l, a);
        }
      }
      __syncthreads();
    }
  }
  const uint32_t n_write = n_ret < p.out_stride ? n_ret : p.out_stride;  // (the host checked: n_ret <= out_stride)
  for (uint32_t j = tid; j < n_write; j += TSEL_THREADS) {
    const uint32_t idx = kp.idx(KP::get(skeys, j));
    const size_t o = (size_t)q * p.out_stride + j;
    p.out_keys[o] = p.min_value + p.gcd * (unsigned long long)idx;
    p.out_counts[o] = row[idx];
    kp.write(o, idx);
  }
  if (tid != 0u) return;
  unsigned long long kept_all = 0ull;
  Key next_all{};
  for (uint32_t v = 0; v < TSEL_WAVES; ++v) {
    kept_all += red[v][2];
    const Key o = KP::get(red_next, v);
    if (next_all < o) next_all = o;
  }
  TqkAggTerms *const R = p.records + q;
  R->sum_other_doc_count = total - kept_all;
  R->distinct = distinct;
  R->n_returned = n_ret;
  R->doc_count_error_upper_bound = next_all == Key{} ? 0u : row[kp.idx(next_all)];
  if (n_ret) atomicAdd(p.totals + 3, (unsigned long long)n_ret);
}

}  // namespace
