// tq_term_arena.cpp — where term preparation's device memory comes from: the 4 MB slabs of the terms' table blobs, the
// segment's arena of side tables (one hipMalloc, or a reserved address range mapped chunk by chunk) and the range
// directories' chunks inside it.
// Part of the C ABI library of include/tantivy_amd.h (internal declarations: tq_internal.hpp).
#include "tq_internal.hpp"

namespace tqi {

// A term's table blob (block records, coarse table, tail, position-block table): carved out of 4 MB slabs — one
// hipMalloc per prepared term was most of the 40 us a sparse term cost to prepare, i.e. most of a batch that names
// two thousand new terms (the 65 536-term stream of bench.py).  Slabs live as long as the segment; a blob handed
// back by a failed preparation is simply not reused.  Large blobs get an allocation of their own.
int term_alloc(tq_segment *s, size_t bytes, uint8_t **out) {
  constexpr size_t kSlab = (size_t)4 << 20;
  const size_t need = (bytes + 255) & ~(size_t)255;
  if (need > kSlab / 4) {
    HIP_TRY(hipMalloc((void **)out, bytes));
    s->term_slabs.push_back(*out);
    return TQ_OK;
  }
  if (need > s->term_slab_left) {
    void *slab = nullptr;
    HIP_TRY(hipMalloc(&slab, kSlab));
    s->term_slabs.push_back(slab);
    s->term_slab_cur = (uint8_t *)slab;
    s->term_slab_left = kSlab;
  }
  *out = s->term_slab_cur;
  s->term_slab_cur += need;
  s->term_slab_left -= need;
  return TQ_OK;
}

// A failed preparation hands its blob back (a caller retrying a term that keeps failing — a corrupt list —
// allocated again on every attempt until tq_segment_free).  The slab's LAST allocation is rolled back (failures are
// reported before anything else is allocated, so that is the common case); a blob with an allocation of its own is
// freed; anything else stays in its slab.  The device may still be writing to it: the caller has synchronised.
void term_release(tq_segment *s, uint8_t *blob, size_t bytes) {
  if (!blob) return;
  constexpr size_t kSlab = (size_t)4 << 20;
  const size_t need = (bytes + 255) & ~(size_t)255;
  if (s->bytes_term_tables >= bytes) s->bytes_term_tables -= bytes;
  if (need > kSlab / 4) {
    for (size_t i = s->term_slabs.size(); i-- > 0;)
      if (s->term_slabs[i] == blob) {
        s->term_slabs.erase(s->term_slabs.begin() + (ptrdiff_t)i);
        (void)hipFree(blob);
        break;
      }
    return;
  }
  if (s->term_slab_cur == blob + need) {
    s->term_slab_cur = blob;
    s->term_slab_left += need;
  }
}

// ---- the arena as a reserved address range (tq_internal.hpp: dense_arena_vmm)
constexpr size_t kVmmChunk = (size_t)32 << 20;
static bool vmm_map_more(tq_segment *s, size_t bytes) {
  hipMemAllocationProp prop{};
  prop.type = hipMemAllocationTypePinned;
  prop.location.type = hipMemLocationTypeDevice;
  prop.location.id = s->device;
  size_t gran = 0;
  if (hipMemGetAllocationGranularity(&gran, &prop, hipMemAllocationGranularityRecommended) != hipSuccess || !gran) {
    (void)hipGetLastError();
    gran = (size_t)2 << 20;
  }
  // (the driver reported 4 KB and then refused hipMemSetAccess on a chunk that started 47 MB into the range: chunks are
  // multiples of 2 MB — the device's large page — whatever it reports)
  // (and hipMemSetAccess refused 32 MB chunks at 2-, 4- and 16-MB-aligned addresses while it took one at a 64-MB-aligned
  // address: every chunk is a multiple of kVmmChunk at a multiple of kVmmChunk from a kVmmChunk-aligned base, and access
  // is set over the whole mapped prefix)
  gran = std::max<size_t>(gran, kVmmChunk);
  bytes = (bytes + gran - 1) / gran * gran;
  if (s->dense_arena_mapped + bytes > s->dense_arena_cap) return false;
  static const bool trace = getenv("TQ_TRACE") != nullptr;
  auto why = [&](const char *what, hipError_t e) {
    if (trace) fprintf(stderr, "[tq] arena: %s of %zu MB at +%zu MB failed: %s\n", what, bytes >> 20, s->dense_arena_mapped >> 20, hipGetErrorString(e));
    (void)hipGetLastError();
  };
  hipMemGenericAllocationHandle_t h{};
  hipError_t e = hipMemCreate(&h, bytes, &prop, 0);
  if (e != hipSuccess) {
    why("hipMemCreate", e);
    return false;
  }
  uint8_t *at = s->dense_arena + s->dense_arena_mapped;
  e = hipMemMap(at, bytes, 0, h, 0);
  if (e != hipSuccess) {
    why("hipMemMap", e);
    (void)hipMemRelease(h);
    return false;
  }
  hipMemAccessDesc ad{};
  ad.location = prop.location;
  ad.flags = hipMemAccessFlagsProtReadWrite;
  // (the whole mapped prefix, not the new chunk alone: the driver refused the third chunk's own range — "invalid argument")
  e = hipMemSetAccess(s->dense_arena, s->dense_arena_mapped + bytes, &ad, 1);
  if (e != hipSuccess) e = hipMemSetAccess(at, bytes, &ad, 1);
  if (e != hipSuccess) {
    why("hipMemSetAccess", e);
    (void)hipMemUnmap(at, bytes);
    (void)hipMemRelease(h);
    return false;
  }
  s->dense_arena_chunks.emplace_back(h, bytes);
  s->dense_arena_mapped += bytes;
  return true;
}
static bool vmm_reserve(tq_segment *s, size_t first_bytes) {
  static const bool kVmm = tune_u32("TQ_VMM_ARENA", 1) != 0;  // 0: one hipMalloc of the budgets' size + overflow allocations (rounds 3-5)
  if (!kVmm) return false;
  constexpr size_t kReserve = (size_t)24 << 30;  // (the table offsets reach 32 GB)
  void *va = nullptr;
  // (the alignment argument is not honoured — 2 MB-aligned addresses came back for a 1 GB request: the range is a
  // chunk longer and the arena starts at its first multiple of kVmmChunk)
  const hipError_t re = hipMemAddressReserve(&va, kReserve + kVmmChunk, 0, nullptr, 0);
  if (re != hipSuccess || !va) {
    if (getenv("TQ_TRACE")) fprintf(stderr, "[tq] arena: hipMemAddressReserve of %zu GB: %s, address %p\n", kReserve >> 30, hipGetErrorString(re), va);
    (void)hipGetLastError();
    return false;
  }
  s->dense_arena_va = va;
  va = (void *)(((uintptr_t)va + kVmmChunk - 1) & ~(uintptr_t)(kVmmChunk - 1));
  s->dense_arena = (uint8_t *)va;
  s->dense_arena_cap = kReserve;
  s->dense_arena_mapped = 0;
  s->dense_arena_first = first_bytes;
  s->dense_arena_vmm = true;
  if (!vmm_map_more(s, first_bytes)) {  // (nothing mapped: hand the range back, the old arena takes over)
    if (getenv("TQ_TRACE")) fprintf(stderr, "[tq] arena: first chunk of %zu MB not mapped\n", first_bytes >> 20);
    (void)hipMemAddressFree(s->dense_arena_va, kReserve + kVmmChunk);
    s->dense_arena_va = nullptr;
    s->dense_arena = nullptr;
    s->dense_arena_cap = 0;
    s->dense_arena_vmm = false;
    return false;
  }
  return true;
}
void dense_arena_free(tq_segment *s) {
  if (!s->dense_arena) return;
  if (!s->dense_arena_vmm) {
    (void)hipFree(s->dense_arena);
  } else {
    size_t off = 0;
    for (auto &ch : s->dense_arena_chunks) {
      (void)hipMemUnmap(s->dense_arena + off, ch.second);
      (void)hipMemRelease(ch.first);
      off += ch.second;
    }
    s->dense_arena_chunks.clear();
    (void)hipMemAddressFree(s->dense_arena_va, s->dense_arena_cap + kVmmChunk);
    s->dense_arena_va = nullptr;
  }
  s->dense_arena = nullptr;
  s->dense_arena_cap = s->dense_arena_used = s->dense_arena_mapped = 0;
  s->dense_arena_vmm = false;
}

// a side table of a dense list: from the segment's arena, else a device allocation of its own
int dense_alloc(tq_segment *s, size_t bytes, void **out) {
  const size_t need = (bytes + 255) & ~(size_t)255;
  if (!s->dense_arena && s->dense_arena_cap == 0) {
    const size_t cap = std::max<size_t>(s->dense_budget() + s->probe_budget() + s->rdir_budget(), (size_t)1 << 20) + PAD;
    void *base = nullptr;
    if (vmm_reserve(s, cap)) {
      // (the first chunk is what the old arena was: the budgets' worth in one piece)
    } else if (hipMalloc(&base, cap) == hipSuccess) {
      s->dense_arena = (uint8_t *)base;
      s->dense_arena_cap = cap;
    } else {
      (void)hipGetLastError();
      s->dense_arena_cap = 1;  // (tried once: every table gets its own allocation)
    }
  }
  if (s->dense_arena && s->dense_arena_vmm) {
    // growth beyond the budgets (a probe pool grown by a batch that names more lists than it holds, tables of a
    // segment whose options were raised): in multiples of 32 MB
    const size_t want = s->dense_arena_used + need + PAD;
    bool ok = want <= s->dense_arena_cap;
    // (a quarter of what is mapped at a time: a stream discovering a large vocabulary adds hundreds of MB of range
    // directories, and a mapping is three driver calls)
    while (ok && want > s->dense_arena_mapped)
      ok = vmm_map_more(s, std::max<size_t>({want - s->dense_arena_mapped, s->dense_arena_mapped / 4, kVmmChunk}));
    if (ok) {
      *out = s->dense_arena + s->dense_arena_used;
      s->dense_arena_used += need;
      return TQ_OK;
    }
  } else if (s->dense_arena && s->dense_arena_used + need + PAD <= s->dense_arena_cap) {
    *out = s->dense_arena + s->dense_arena_used;
    s->dense_arena_used += need;
    return TQ_OK;
  }
  void *ptr = nullptr;
  HIP_TRY(hipMalloc(&ptr, bytes));
  s->dense_extra.push_back(ptr);
  *out = ptr;
  return TQ_OK;
}
// (tables are only ever released with the segment; a failed build leaves its bytes unused)
void dense_release(tq_segment *s, void *ptr) {
  for (size_t i = 0; i < s->dense_extra.size(); ++i)
    if (s->dense_extra[i] == ptr) {
      (void)hipFree(ptr);
      s->dense_extra.erase(s->dense_extra.begin() + (long)i);
      return;
    }
}

// Range directories (rdir_plan, tq_term_tables.cpp) are carved out of 32 MB chunks of the segment's arena, kept until
// the segment is closed.
int rdir_alloc(tq_segment *s, size_t bytes, void **out) {
  constexpr size_t kChunk = (size_t)32 << 20;
  const size_t need = (bytes + 255) & ~(size_t)255;
  // (chunks come out of the segment's arena of side tables — dense_alloc — so that they lie within the 32 GB the
  // shared launches' table offsets span; a process with several indexes open hands out distant addresses otherwise)
  if (need > kChunk / 2) {
    void *own = nullptr;
    const int arc = dense_alloc(s, need, &own);
    if (arc != TQ_OK) return arc;
    s->rdir_chunks.push_back({own, need});
    *out = own;
  } else {
    if (need > s->rdir_chunk_left) {
      void *chunk = nullptr;
      const int arc = dense_alloc(s, kChunk, &chunk);
      if (arc != TQ_OK) return arc;
      s->rdir_chunks.push_back({chunk, kChunk});
      s->rdir_chunk_cur = (uint8_t *)chunk;
      s->rdir_chunk_left = kChunk;
    }
    *out = s->rdir_chunk_cur;
    s->rdir_chunk_cur += need;
    s->rdir_chunk_left -= need;
  }
  s->rdir_bytes_total += bytes;
  s->bytes_term_tables += bytes;
  s->share_span_terms = ~(size_t)0;  // (the tables' address span is taken again: tq_search.cpp)
  return TQ_OK;
}

}  // namespace tqi
