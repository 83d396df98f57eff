// Full doc sets over bitmaps (Weight::for_each_no_score -> SegmentCollector::collect_block, src/query/weight.rs:23-35,
// 101-121; boolean_weight.rs:536-560; term_weight.rs:88-116; the alive filter of default_collect_segment_impl,
// src/collector/mod.rs:186-221): what DocSetCollector, FilterCollector, facets and aggregations ask a Weight for —
// every alive matching doc of the segment, ascending.  The query is the bitwise expression tq_count.hip evaluates
// (AND over the Must clauses of (OR over the clause's lists), AND NOT the MustNot lists, AND "at least m Should
// clauses", AND the alive bits); here the bits are kept and turned into doc ids.  No postings are decoded.
//
// Two passes over the same words, so that no result bits are stored (n_queries x max_doc / 8 bytes would be 12.5 GB
// for 10 000 queries on 10 M docs):
//   count   workgroup = (query, tile of 65 536 docs), query fastest as in count_bitmap_kernel: one u32 per
//           (query, tile) into a query-major table, no atomics;
//   scan    exclusive 64-bit prefix sum of the table (partials / top / apply): entry (q, tile 0) is out_starts[q],
//           the total out_starts[n];
//   write   the tile's words again, a workgroup-wide exclusive prefix of their popcounts in word order, every lane
//           expands its words to doc ids at start + prefix — straight to memory for a tile with few docs, through an
//           LDS slab (consecutive lanes then store consecutive docs) for a tile with at least stage_min_docs
//           (TQ_DOCSET_STAGE_MIN, 2048 of 65 536: measured in DESIGN.md 3.4a).  Every store is guarded by pos < out_cap.
// HBM model: 2 x lists x 8 (4 for scattered lists) bytes per 32 docs read, 4 bytes per doc written.
#include "tq_common.hpp"
#include "tq_docset_word.hpp"  // SlicedCount / docset_head / docset_word / wave_incl_sum
#include "tq_launch.h"

namespace {

constexpr uint32_t DS_THREADS = 256;
constexpr uint32_t DS_WAVES = DS_THREADS / 64;
constexpr uint32_t DS_WORDS_PER_THREAD = 8;
constexpr uint32_t DS_TILE_WORDS = DS_THREADS * DS_WORDS_PER_THREAD;  // 2048 words = 65 536 docs
constexpr uint32_t DS_SCAN_PER_THREAD = 8;
constexpr uint32_t DS_SCAN_TILE = DS_THREADS * DS_SCAN_PER_THREAD;  // table entries per scan workgroup

__global__ __launch_bounds__(DS_THREADS) void docset_count_kernel(TqkDocsetParams p) {
  __shared__ uint32_t wave_cnt[DS_WAVES];
  const uint32_t q = blockIdx.x % p.n_queries, tile = blockIdx.x / p.n_queries;
  const TqkDocsetQuery *Q = p.queries + q;
  const DocsetHead h = docset_head(Q);
  uint32_t cnt = 0;
#pragma unroll 2
  for (uint32_t i = 0; i < DS_WORDS_PER_THREAD; ++i) {
    const uint32_t w = tile * DS_TILE_WORDS + i * DS_THREADS + threadIdx.x;
    if (w >= p.n_words) break;
    cnt += (uint32_t)__popc(docset_word(Q, h, p, w));
  }
  for (int off = 32; off > 0; off >>= 1) cnt += __shfl_down(cnt, off, 64);
  if ((threadIdx.x & 63u) == 0u) wave_cnt[threadIdx.x >> 6] = cnt;
  __syncthreads();
  if (threadIdx.x == 0u) {
    uint32_t t = 0;
    for (uint32_t i = 0; i < DS_WAVES; ++i) t += wave_cnt[i];
    p.tile_counts[(size_t)q * p.n_tiles + tile] = t;
  }
}

// ---- exclusive scan of tile_counts (u32) into tile_offs (u64); tile 0 of every query -> out_starts
__device__ __forceinline__ uint64_t block_excl_scan64(uint64_t v, uint64_t *sh, uint64_t *total) {
  sh[threadIdx.x] = v;
  __syncthreads();
  for (uint32_t o = 1; o < DS_THREADS; o <<= 1) {
    const uint64_t u = threadIdx.x >= o ? sh[threadIdx.x - o] : 0ull;
    __syncthreads();
    sh[threadIdx.x] += u;
    __syncthreads();
  }
  const uint64_t incl = sh[threadIdx.x];
  *total = sh[DS_THREADS - 1];
  __syncthreads();
  return incl - v;
}

__global__ __launch_bounds__(DS_THREADS) void docset_scan_partials_kernel(TqkDocsetParams p, uint32_t n_entries) {
  __shared__ uint64_t sh[DS_THREADS];
  const uint32_t base = blockIdx.x * DS_SCAN_TILE + threadIdx.x * DS_SCAN_PER_THREAD;
  uint64_t s = 0;
  for (uint32_t i = 0; i < DS_SCAN_PER_THREAD; ++i)
    if (base + i < n_entries) s += p.tile_counts[base + i];
  uint64_t total;
  (void)block_excl_scan64(s, sh, &total);
  if (threadIdx.x == 0u) p.partials[blockIdx.x] = total;
}

// one workgroup: the partials become exclusive offsets (from *base_in: the docs of the sub-batches before this one);
// the total goes to out_starts[n_queries]
__global__ __launch_bounds__(DS_THREADS) void docset_scan_top_kernel(TqkDocsetParams p, uint32_t n_partials) {
  __shared__ uint64_t sh[DS_THREADS];
  uint64_t carry = p.base_in ? *p.base_in : 0ull;
  for (uint32_t base = 0; base < n_partials; base += DS_THREADS) {
    const uint32_t i = base + threadIdx.x;
    const uint64_t v = i < n_partials ? p.partials[i] : 0ull;
    uint64_t total;
    const uint64_t excl = block_excl_scan64(v, sh, &total);
    if (i < n_partials) p.partials[i] = carry + excl;
    carry += total;
  }
  if (threadIdx.x == 0u) p.out_starts[p.n_queries] = carry;
}

__global__ __launch_bounds__(DS_THREADS) void docset_scan_apply_kernel(TqkDocsetParams p, uint32_t n_entries) {
  __shared__ uint64_t sh[DS_THREADS];
  const uint32_t base = blockIdx.x * DS_SCAN_TILE + threadIdx.x * DS_SCAN_PER_THREAD;
  uint32_t c[DS_SCAN_PER_THREAD];
  uint64_t s = 0;
  for (uint32_t i = 0; i < DS_SCAN_PER_THREAD; ++i) {
    c[i] = base + i < n_entries ? p.tile_counts[base + i] : 0u;
    s += c[i];
  }
  uint64_t total;
  uint64_t run = p.partials[blockIdx.x] + block_excl_scan64(s, sh, &total);
  for (uint32_t i = 0; i < DS_SCAN_PER_THREAD; ++i) {
    const uint32_t e = base + i;
    if (e < n_entries) {
      p.tile_offs[e] = run;
      if (e % p.n_tiles == 0u) p.out_starts[e / p.n_tiles] = run;
      run += c[i];
    }
  }
}

// per-query sizes (tq_last_batch_match_counts) and the running total (tq_batch_stats.matches)
__global__ __launch_bounds__(DS_THREADS) void docset_sizes_kernel(TqkDocsetParams p) {
  const uint32_t q = blockIdx.x * DS_THREADS + threadIdx.x;
  if (q >= p.n_queries) return;
  const uint64_t n = p.out_starts[q + 1u] - p.out_starts[q];
  p.query_sizes[q] = (uint32_t)n;
  if (q == p.n_queries - 1u) *p.total_out = p.out_starts[p.n_queries];
}

__global__ __launch_bounds__(DS_THREADS) void docset_write_kernel(TqkDocsetParams p) {
  __shared__ uint32_t wave_tot[DS_WORDS_PER_THREAD / 2][DS_WAVES];  // two 16-bit sums per word: iterations 2j and 2j + 1
  const int lane = (int)__lane_id();
  const uint32_t wave = threadIdx.x >> 6;
  const uint32_t q = blockIdx.x % p.n_queries, tile = blockIdx.x / p.n_queries;
  const size_t entry = (size_t)q * p.n_tiles + tile;
  const uint32_t tile_docs = p.tile_counts[entry];
  if (tile_docs == 0u) return;  // (uniform for the workgroup)
  const uint64_t start = p.tile_offs[entry];
  if (start >= p.out_cap) return;  // nothing of this tile fits
  const TqkDocsetQuery *Q = p.queries + q;
  const DocsetHead h = docset_head(Q);
  uint32_t res[DS_WORDS_PER_THREAD];
#pragma unroll
  for (uint32_t i = 0; i < DS_WORDS_PER_THREAD; ++i) {
    const uint32_t w = tile * DS_TILE_WORDS + i * DS_THREADS + threadIdx.x;
    res[i] = w < p.n_words ? docset_word(Q, h, p, w) : 0u;
  }
  // inclusive sums of the popcounts over the wave, two iterations per scan (a wave holds at most 2048 docs of one)
  uint32_t incl[DS_WORDS_PER_THREAD / 2];
#pragma unroll
  for (uint32_t j = 0; j < DS_WORDS_PER_THREAD / 2; ++j) {
    incl[j] = wave_incl_sum((uint32_t)__popc(res[2 * j]) | ((uint32_t)__popc(res[2 * j + 1]) << 16), lane);
    if (lane == 63) wave_tot[j][wave] = incl[j];
  }
  __syncthreads();
  // word order = iteration, then wave, then lane
  uint32_t run = 0;
  if (tile_docs >= p.stage_min_docs) {
    // a tile with many docs: the docs of 256 words are laid out in LDS first and leave as full lines — consecutive
    // lanes store consecutive docs — instead of every lane storing its own word's docs at a stride of the popcounts.
    // The slab holds the docs' 13 bits within the 256 words: 16 KB, so that the tiles that do not use it keep their
    // occupancy (with 32 KB of full doc ids the and2 batch of tools/bench_docset.py took 2.43 ms instead of 1.84).
    __shared__ uint16_t slab[DS_THREADS * 32];
#pragma unroll
    for (uint32_t i = 0; i < DS_WORDS_PER_THREAD; ++i) {
      uint32_t before = 0, tot = 0;
      for (uint32_t v = 0; v < DS_WAVES; ++v) {
        const uint32_t t = (wave_tot[i >> 1][v] >> (16u * (i & 1u))) & 0xFFFFu;
        if (v < wave) before += t;
        tot += t;
      }
      uint32_t r = res[i];
      const uint32_t mine = (incl[i >> 1] >> (16u * (i & 1u))) & 0xFFFFu;
      uint32_t at = before + (mine - (uint32_t)__popc(r));  // < tot <= 8192
      while (r) {
        slab[at++] = (uint16_t)((threadIdx.x << 5) | (uint32_t)__builtin_ctz(r));
        r &= r - 1u;
      }
      __syncthreads();
      const uint64_t base = start + run;
      const uint32_t doc0 = (tile * DS_TILE_WORDS + i * DS_THREADS) << 5;
      for (uint32_t j = threadIdx.x; j < tot; j += DS_THREADS)
        if (base + j < p.out_cap) p.out_docs[base + j] = doc0 | slab[j];
      __syncthreads();
      run += tot;
    }
  } else {
#pragma unroll
    for (uint32_t i = 0; i < DS_WORDS_PER_THREAD; ++i) {
      uint32_t before = run;
      for (uint32_t v = 0; v < DS_WAVES; ++v) {
        const uint32_t t = (wave_tot[i >> 1][v] >> (16u * (i & 1u))) & 0xFFFFu;
        if (v < wave) before += t;
        run += t;
      }
      uint32_t r = res[i];
      if (!r) continue;
      const uint32_t mine = (incl[i >> 1] >> (16u * (i & 1u))) & 0xFFFFu;
      uint64_t pos = start + before + (mine - (uint32_t)__popc(r));
      const uint32_t doc0 = (tile * DS_TILE_WORDS + i * DS_THREADS + threadIdx.x) << 5;
      while (r) {
        if (pos < p.out_cap) p.out_docs[pos] = doc0 | (uint32_t)__builtin_ctz(r);
        r &= r - 1u;
        ++pos;
      }
    }
  }
}

}  // namespace

uint32_t tqk_docset_tile_words() { return DS_TILE_WORDS; }
uint32_t tqk_docset_scan_tile() { return DS_SCAN_TILE; }

hipError_t tqk_launch_docset_count(const TqkDocsetParams &p, hipStream_t st) {
  if (!p.n_tiles || !p.n_queries) return hipSuccess;
  docset_count_kernel<<<dim3(p.n_tiles * p.n_queries), dim3(DS_THREADS), 0, st>>>(p);
  return hipGetLastError();
}

hipError_t tqk_launch_docset_scan(const TqkDocsetParams &p, hipStream_t st) {
  if (!p.n_tiles || !p.n_queries) return hipSuccess;
  const uint32_t n_entries = p.n_tiles * p.n_queries;
  const uint32_t n_partials = (n_entries + DS_SCAN_TILE - 1) / DS_SCAN_TILE;
  docset_scan_partials_kernel<<<dim3(n_partials), dim3(DS_THREADS), 0, st>>>(p, n_entries);
  docset_scan_top_kernel<<<dim3(1), dim3(DS_THREADS), 0, st>>>(p, n_partials);
  docset_scan_apply_kernel<<<dim3(n_partials), dim3(DS_THREADS), 0, st>>>(p, n_entries);
  docset_sizes_kernel<<<dim3((p.n_queries + DS_THREADS - 1) / DS_THREADS), dim3(DS_THREADS), 0, st>>>(p);
  return hipGetLastError();
}

hipError_t tqk_launch_docset_write(const TqkDocsetParams &p, hipStream_t st) {
  if (!p.n_tiles || !p.n_queries) return hipSuccess;
  docset_write_kernel<<<dim3(p.n_tiles * p.n_queries), dim3(DS_THREADS), 0, st>>>(p);
  return hipGetLastError();
}
