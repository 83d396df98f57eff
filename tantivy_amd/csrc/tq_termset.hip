// tq_termset.hip — the bitmap of a TERM SET (tq_term_set_prepare): what AutomatonWeight::scorer builds for FuzzyTermQuery,
// RegexQuery and TermSetQuery (src/query/automaton_weight.rs:87-111: every matching term's docs OR-ed into a
// BitSet(max_doc), wrapped in ConstScorer(BitSetDocSet), src/query/const_score_query.rs:95-148) — as a {32 doc bits,
// docs before the word} table with the layout of TqdTermHead::dense, so that every bitmap reader takes it unchanged.
//
// One preparation is three stages on the segment's stream, over a zeroed table:
//   OR       the members that have a bitmap of their own, word-wise: a lane per word, every such member of the set in ONE
//            launch (consecutive lanes read consecutive words of one member: coalesced; the member pointers are
//            wave-uniform scalar loads)
//   scatter  the members without one: a wavefront per 128-doc block (the decode count_scatter_kernel uses, vint tails
//            included), atomicOr per doc; a work item = (member, first of four blocks), the grid strides over any number
//            of them.  The docs of a block ascend, so the 128 atomics of a wavefront fall into few cache lines
//   rank     tab[w].y = docs before word w: the project's three-launch device scan (per-tile sums, one workgroup over the
//            sums, every tile again on top of its offset); the first launch also masks the bits at and past max_doc in the
//            last word, the last one stores the sentinel entry and the set's doc count
// HBM model: the scattered members' posting bytes + 4 B per 32 docs per bitmap member (its rank half rides along) + 8 B
// per 32 docs written and read once by the scan.
#include <algorithm>

#include "tq_common.hpp"
#include "tq_launch.h"

namespace {

constexpr uint32_t TS_THREADS = 256;
constexpr uint32_t TS_PER_THREAD = 8;
constexpr uint32_t TS_TILE = TS_THREADS * TS_PER_THREAD;  // 2048 words = 65 536 docs per scan tile

// the members with a bitmap, OR-ed word by word: plain stores into the zeroed table (the scatter follows in stream order)
__global__ __launch_bounds__(TS_THREADS) void termset_or_kernel(const uint2 *const *members, uint32_t n_members, uint2 *tab,
                                                                uint32_t n_words) {
  for (uint32_t w = blockIdx.x * TS_THREADS + threadIdx.x; w < n_words; w += gridDim.x * TS_THREADS) {
    uint32_t bits = 0u;
    for (uint32_t m = 0; m < n_members; ++m) {
      const uint2 *bm = reinterpret_cast<const uint2 *>(sload(reinterpret_cast<const uint64_t *>(members) + m));
      bits |= bm[w].x;
    }
    tab[w].x = bits;
  }
}

// the members without a bitmap: items[i] = {member's term handle, first block}; four blocks per item, one per wavefront
__global__ __launch_bounds__(256) void termset_scatter_kernel(TqdSegment seg, const TqdTerm *terms, const uint2 *items,
                                                              uint32_t n_items, uint2 *tab) {
  const int lane = (int)__lane_id();
  const uint32_t wave = uni(threadIdx.x >> 6);
  for (uint32_t it = blockIdx.x; it < n_items; it += gridDim.x) {
    const uint2 w = sload(items + it);
    const TermRef t = load_term(terms, w.x);
    const uint32_t j = w.y + wave;
    if (j >= t.n_blocks) continue;
    const Dec d = decode_block<true, false>(uni_ptr(seg.idx), t, j, lane);
    if (d.d0 < seg.max_doc) atomicOr(&tab[d.d0 >> 5].x, 1u << (d.d0 & 31u));
    if (d.d1 < seg.max_doc) atomicOr(&tab[d.d1 >> 5].x, 1u << (d.d1 & 31u));
  }
}

__device__ __forceinline__ uint32_t ts_wave_incl_scan(uint32_t x, int lane) {
#pragma unroll
  for (int d = 1; d < WAVE; d <<= 1) {
    const uint32_t y = (uint32_t)__shfl_up((int)x, d, WAVE);
    if (lane >= d) x += y;
  }
  return x;
}
// exclusive prefix of `mine` over the workgroup's 256 threads + the workgroup's total
__device__ __forceinline__ uint32_t ts_wg_excl_scan(uint32_t mine, uint32_t &total) {
  __shared__ uint32_t wsum[TS_THREADS / WAVE];
  const int lane = (int)__lane_id();
  const uint32_t wv = threadIdx.x >> 6;
  const uint32_t incl = ts_wave_incl_scan(mine, lane);
  if (lane == WAVE - 1) wsum[wv] = incl;
  __syncthreads();
  uint32_t before = 0, all = 0;
#pragma unroll
  for (uint32_t w = 0; w < TS_THREADS / WAVE; ++w) {
    const uint32_t v = wsum[w];
    before += w < wv ? v : 0u;
    all += v;
  }
  total = all;
  return before + incl - mine;
}

// per-tile popcount sums; the thread that owns the segment's last word first clears its bits at and past max_doc
__global__ __launch_bounds__(TS_THREADS) void termset_sums_kernel(uint2 *tab, uint32_t n_words, uint32_t max_doc, uint32_t *tile_sums) {
  const uint32_t i0 = blockIdx.x * TS_TILE + threadIdx.x * TS_PER_THREAD;
  uint32_t mine = 0;
#pragma unroll
  for (uint32_t e = 0; e < TS_PER_THREAD; ++e) {
    const uint32_t w = i0 + e;
    if (w >= n_words) continue;
    uint32_t x = tab[w].x;
    if (w == n_words - 1u && (max_doc & 31u)) {
      x &= (1u << (max_doc & 31u)) - 1u;
      tab[w].x = x;
    }
    mine += (uint32_t)__popc(x);
  }
  uint32_t total;
  (void)ts_wg_excl_scan(mine, total);
  if (threadIdx.x == 0) tile_sums[blockIdx.x] = total;
}
// one workgroup: tile_sums -> exclusive prefix, in place; tile_sums[n_tiles] = the grand total
__global__ __launch_bounds__(TS_THREADS) void termset_tiles_kernel(uint32_t *tile_sums, uint32_t n_tiles) {
  uint32_t carry = 0;
  for (uint32_t base = 0; base < n_tiles; base += TS_THREADS) {
    const uint32_t i = base + threadIdx.x;
    const uint32_t v = i < n_tiles ? tile_sums[i] : 0u;
    uint32_t total;
    const uint32_t ex = ts_wg_excl_scan(v, total);
    if (i < n_tiles) tile_sums[i] = carry + ex;
    carry += total;
    __syncthreads();  // (the scan's LDS words are reused by the next chunk)
  }
  if (threadIdx.x == 0) tile_sums[n_tiles] = carry;
}
// tab[w].y = docs before word w; tab[n_words] = {0, the set's doc count} (the sentinel every dense table ends with)
__global__ __launch_bounds__(TS_THREADS) void termset_rank_kernel(uint2 *tab, uint32_t n_words, const uint32_t *tile_off, uint32_t n_tiles) {
  const uint32_t i0 = blockIdx.x * TS_TILE + threadIdx.x * TS_PER_THREAD;
  uint32_t v[TS_PER_THREAD], mine = 0;
#pragma unroll
  for (uint32_t e = 0; e < TS_PER_THREAD; ++e) {
    v[e] = i0 + e < n_words ? (uint32_t)__popc(tab[i0 + e].x) : 0u;
    mine += v[e];
  }
  uint32_t total;
  uint32_t run = tile_off[blockIdx.x] + ts_wg_excl_scan(mine, total);
#pragma unroll
  for (uint32_t e = 0; e < TS_PER_THREAD; ++e) {
    if (i0 + e < n_words) tab[i0 + e].y = run;
    run += v[e];
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) tab[n_words] = make_uint2(0u, tile_off[n_tiles]);
}

}  // namespace

uint32_t tqk_termset_scan_tile() { return TS_TILE; }
uint32_t tqk_termset_scratch_words(uint32_t n_words) { return (n_words + TS_TILE - 1u) / TS_TILE + 2u; }

hipError_t tqk_launch_termset_build(const TqdSegment &seg, const TqdTerm *terms, const uint2 *const *d_members, uint32_t n_members,
                                    const uint2 *d_items, uint32_t n_items, uint2 *tab, uint32_t n_words, uint32_t *scan_scratch,
                                    hipStream_t st) {
  if (n_members && n_words) {
    const uint32_t grid = std::min<uint32_t>((n_words + TS_THREADS - 1u) / TS_THREADS, 1u << 16);
    termset_or_kernel<<<dim3(grid), dim3(TS_THREADS), 0, st>>>(d_members, n_members, tab, n_words);
  }
  if (n_items) {
    termset_scatter_kernel<<<dim3(std::min<uint32_t>(n_items, 1u << 16)), dim3(256), 0, st>>>(seg, terms, d_items, n_items, tab);
  }
  return tqk_launch_bitmap_rank(tab, n_words, seg.max_doc, scan_scratch, st);
}

// the rank stage alone, over a table whose .x words are written: what a term set's build ends with, and what the
// fast-field columns (tq_column.cpp) run over a presence bitmap and over the bits range_fill_kernel leaves
hipError_t tqk_launch_bitmap_rank(uint2 *tab, uint32_t n_words, uint32_t max_doc, uint32_t *scan_scratch, hipStream_t st) {
  const uint32_t n_tiles = (n_words + TS_TILE - 1u) / TS_TILE;
  // (a segment without docs: one launch for the sentinel and the count, over no word)
  termset_sums_kernel<<<dim3(std::max(n_tiles, 1u)), dim3(TS_THREADS), 0, st>>>(tab, n_words, max_doc, scan_scratch);
  termset_tiles_kernel<<<dim3(1), dim3(TS_THREADS), 0, st>>>(scan_scratch, std::max(n_tiles, 1u));
  termset_rank_kernel<<<dim3(std::max(n_tiles, 1u)), dim3(TS_THREADS), 0, st>>>(tab, n_words, scan_scratch, std::max(n_tiles, 1u));
  return hipGetLastError();
}
