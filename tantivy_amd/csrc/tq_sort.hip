// tq_sort.hip — sort by fast field (tq_search_sorted_batch*): what TopDocs::order_by_fast_field / order_by_u64_field /
// order_by((SortByStaticFastValue, ComparatorEnum)) leave of a segment (src/collector/top_score_collector.rs:217-223,
// 299-330, 503-683; sort_key/sort_by_static_fast_value.rs:62-96; sort_key/order.rs) — the first min(k, matches) alive
// matching docs under compare_for_top_k: the comparator on Option<u64> = Column<u64>::first(doc), then ascending doc id.
// No doc set is written: the match bits (docset_word, tq_docset_word.hpp), the column readers (rg_row / rg_value,
// tq_column_read.hpp) and a wavefront top-k (TopKW, tq_common.hpp) meet in one selection kernel.
//
// Key: larger is better, (0, 0) is the empty slot; from the most significant bit
//   class   2 bits   nulls last: a doc with a value 2, without 1; nulls first: without 3, with 2
//   value'  64 bits  the VALUE (min + gcd * packed; Linear: the packed value) descending, its complement ascending,
//                    0 without a value — values, not packed numbers: Linear's and BlockwiseLinear's are not monotonic
//   ~doc    32 bits  ties: ascending doc id whatever the order
// = 98 bits in two words: hi = class << 34 | value' >> 30, lo = (value' & (2^30 - 1)) << 32 | ~doc.
//
// select   workgroup = (query, slice of the bitmap words), query fastest in the grid.  Assembled from the shared walk
//          (docset_walk, tq_docset_walk.hpp: a lane per matching doc) and col_value (tq_agg_device.hpp); per doc
//          rg_row + the value (a doc without a value loads nothing), the key, offered to the wavefront's TopKW: once the
//          heap is full a losing doc costs its decode and one compare.
//          Then wavefronts 1..3 hand their lists to wavefront 0 through LDS (the slab's bytes), which writes the row
//          (one slice) or the slice's sorted list and {matches, valued matches}.
// merge    one wavefront per query over its slices' lists; writes the row.
// Match counts are sums of popcounts.  Plain vector stores only; nothing is written at or past a row's out_stride.
// HBM model: lists x bitmap words x 4 + 8 per matching doc with a value + 8 per matching doc of an Optional column
// (its presence word) + 13 per row entry written (doc, value, flag).
#include <algorithm>

#include "tq_agg_device.hpp"
#include "tq_column_read.hpp"
#include "tq_common.hpp"
#include "tq_docset_walk.hpp"
#include "tq_launch.h"

namespace {

constexpr uint32_t SO_LDS_WORDS = WALK_SLAB_ENTRIES * 2u / 8u;  // the slabs' 16 KB as 64-bit words
static_assert(SO_LDS_WORDS >= 16u * 64u * 2u, "a wavefront's list of 1024 two-word keys fits the slab's bytes");

// the row of one query from its sorted list: entries, padding (TQD_TERMINATED, 0, 0) up to out_stride, the count
template <int KPL>
__device__ __forceinline__ void sort_write_row(const TqkSortParams &p, const TopKW<KPL> &tk, uint32_t q, uint32_t matches,
                                               uint32_t valued, int lane) {
  const uint64_t row = (uint64_t)q * p.out_stride;
  uint32_t count = 0;
#pragma unroll
  for (int r = 0; r < KPL; ++r) {
    const uint32_t rank = (uint32_t)r * 64u + (uint32_t)lane;
    const bool real = rank < tk.k && tk.hi[r] != 0ull;
    count += (uint32_t)__popcll(__ballot(real));
    if (rank < p.out_stride) {
      const bool has = real && (tk.hi[r] >> 34) == 2ull;
      const uint64_t vp = ((tk.hi[r] & ((1ull << 34) - 1ull)) << 30) | (tk.lo[r] >> 32);
      p.out_docs[row + rank] = real ? ~(uint32_t)tk.lo[r] : TQD_TERMINATED;
      p.out_values[row + rank] = has ? (p.ascending ? ~vp : vp) : 0ull;
      p.out_has_value[row + rank] = has ? (uint8_t)1 : (uint8_t)0;
    }
  }
  for (uint32_t rank = (uint32_t)(KPL * 64) + (uint32_t)lane; rank < p.out_stride; rank += 64u) {
    p.out_docs[row + rank] = TQD_TERMINATED;
    p.out_values[row + rank] = 0ull;
    p.out_has_value[row + rank] = (uint8_t)0;
  }
  if (lane == 0) {
    p.out_counts[q] = count;
    p.query_sizes[q] = matches;
    atomicAdd(p.totals + 0, (unsigned long long)matches);
    atomicAdd(p.totals + 1, (unsigned long long)valued);
    atomicAdd(p.totals + 2, (unsigned long long)count);
  }
}

template <int KPL, bool OPTIONAL>
__global__ __launch_bounds__(WALK_THREADS) void sort_select_kernel(TqkSortParams p) {
  __shared__ uint64_t lds[SO_LDS_WORDS];
  __shared__ uint32_t wave_cnt[WALK_WAVES][2];
  const int lane = (int)__lane_id();
  const uint32_t wave = threadIdx.x >> 6;
  const uint32_t q = blockIdx.x % p.ds.n_queries, slice = blockIdx.x / p.ds.n_queries;
  const uint32_t k = sload(p.ks + q);
  TopKW<KPL> tk;
  tk.reset(k);
  uint32_t valued = 0;  // per wavefront
  uint32_t cnt = docset_walk(p.ds, p.ds.queries + q, slice, p.words_per_slice, reinterpret_cast<uint16_t *>(lds), wave, lane,
                             [&](bool has, uint32_t doc) {
    uint32_t row = 0;
    const bool hv = has && rg_row<OPTIONAL>(p.col, doc, row);
    uint64_t vp = 0;
    if (hv) {
      const uint64_t v = col_value(p.col, p.min_value, p.gcd, row);
      vp = p.ascending ? ~v : v;
    }
    valued += (uint32_t)__popcll(__ballot(hv));
    const uint64_t cls = hv ? 2ull : (p.nulls_first ? 3ull : 1ull);
    tk.offer(has, (cls << 34) | (vp >> 30), ((vp & ((1ull << 30) - 1ull)) << 32) | (uint64_t)(~doc), lane);
  });
  for (int off = 32; off > 0; off >>= 1) cnt += __shfl_down(cnt, off, 64);
  if (lane == 0) {
    wave_cnt[wave][0] = cnt;
    wave_cnt[wave][1] = valued;
  }
  // wavefronts 1..3 hand their lists to wavefront 0, one after the other, through the slab's bytes
  uint64_t *const mh = lds, *const ml = lds + KPL * 64;
  for (uint32_t wv = 1; wv < WALK_WAVES; ++wv) {
    __syncthreads();
    if (wave == wv) {
#pragma unroll
      for (int r = 0; r < KPL; ++r) {
        const uint32_t rank = (uint32_t)r * 64u + (uint32_t)lane;
        mh[rank] = rank < k ? tk.hi[r] : 0ull;
        ml[rank] = rank < k ? tk.lo[r] : 0ull;
      }
    }
    __syncthreads();
    if (wave == 0u) {
#pragma unroll
      for (int r = 0; r < KPL; ++r) {
        const uint32_t rank = (uint32_t)r * 64u + (uint32_t)lane;
        const uint64_t a = mh[rank], b = ml[rank];
        tk.offer(a != 0ull, a, b, lane);
      }
    }
  }
  if (wave != 0u) return;
  uint32_t matches = 0, with_value = 0;
  for (uint32_t v = 0; v < WALK_WAVES; ++v) {
    matches += wave_cnt[v][0];
    with_value += wave_cnt[v][1];
  }
  if (p.n_slices == 1u) {
    sort_write_row<KPL>(p, tk, q, matches, with_value, lane);
    return;
  }
  const size_t part = (size_t)q * p.n_slices + slice;
  uint64_t *const dst = p.partials + part * (size_t)(KPL * 64 * 2);
#pragma unroll
  for (int r = 0; r < KPL; ++r) {
    const uint32_t rank = (uint32_t)r * 64u + (uint32_t)lane;
    dst[rank] = rank < k ? tk.hi[r] : 0ull;
    dst[KPL * 64 + rank] = rank < k ? tk.lo[r] : 0ull;
  }
  if (lane == 0) p.slice_counts[part] = make_uint2(matches, with_value);
}

template <int KPL>
__global__ __launch_bounds__(64) void sort_merge_kernel(TqkSortParams p) {
  const int lane = (int)__lane_id();
  const uint32_t q = blockIdx.x;
  const uint32_t k = sload(p.ks + q);
  TopKW<KPL> tk;
  tk.reset(k);
  uint32_t matches = 0, with_value = 0;
  for (uint32_t s = 0; s < p.n_slices; ++s) {
    const size_t part = (size_t)q * p.n_slices + s;
    const uint2 c = p.slice_counts[part];
    matches += c.x;
    with_value += c.y;
    if (c.x == 0u) continue;  // (uniform: an empty slice's list is all zeros)
    const uint64_t *const src = p.partials + part * (size_t)(KPL * 64 * 2);
#pragma unroll
    for (int r = 0; r < KPL; ++r) {
      const uint32_t rank = (uint32_t)r * 64u + (uint32_t)lane;
      const uint64_t a = src[rank], b = src[KPL * 64 + rank];
      tk.offer(a != 0ull, a, b, lane);
    }
  }
  sort_write_row<KPL>(p, tk, q, matches, with_value, lane);
}

template <int KPL>
void select_launch(const TqkSortParams &p, hipStream_t st) {
  const dim3 grid(p.ds.n_queries * p.n_slices), block(WALK_THREADS);
  if (p.col.present)
    sort_select_kernel<KPL, true><<<grid, block, 0, st>>>(p);
  else
    sort_select_kernel<KPL, false><<<grid, block, 0, st>>>(p);
}

}  // namespace

uint32_t tqk_sort_step_words() { return WALK_STEP_WORDS; }

hipError_t tqk_launch_sort_select(const TqkSortParams &p, int kpl, hipStream_t st) {
  if (!p.ds.n_queries || !p.n_slices) return hipSuccess;
  if (p.col.codec > TQK_COL_BLOCKWISE) return hipErrorInvalidValue;
  switch (kpl) {
    case 1: select_launch<1>(p, st); break;
    case 4: select_launch<4>(p, st); break;
    case 16: select_launch<16>(p, st); break;
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

hipError_t tqk_launch_sort_merge(const TqkSortParams &p, int kpl, hipStream_t st) {
  if (!p.ds.n_queries || p.n_slices <= 1u) return hipSuccess;
  switch (kpl) {
    case 1: sort_merge_kernel<1><<<dim3(p.ds.n_queries), dim3(64), 0, st>>>(p); break;
    case 4: sort_merge_kernel<4><<<dim3(p.ds.n_queries), dim3(64), 0, st>>>(p); break;
    case 16: sort_merge_kernel<16><<<dim3(p.ds.n_queries), dim3(64), 0, st>>>(p); break;
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}
