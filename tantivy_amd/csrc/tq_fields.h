// tq_fields.h — what tree_fields_kernel (tq_tree_fields.hip) and docset_score_fields_kernel
// (tq_docset_score_fields.hip) share (multi-field segments: tq_fields.cpp): per-LIST norms in place of the per-doc norm.
// List m of field f scores under caches[(cache_idx + f) * 256 + fn_f[doc]], or the constant id where the field has no
// fieldnorm file.  Field ids come from the query's descriptor through scalar loads, so every select is wave-uniform.
#pragma once
#include "tq_launch.h"

// A doc's norm under every field the query names: one register per field, held in eight plain locals of the kernel
// (a struct or an array of them is turned into an indexed load from private memory — and from there into LDS — by the
// optimiser, which recognises the chain of selects below), picked per list with wave-uniform selects.
__device__ __forceinline__ float pick_field_norm(uint32_t f, float v0, float v1, float v2, float v3, float v4, float v5, float v6, float v7) {
  float r = v0;  // f wave-uniform
  r = f == 1u ? v1 : r;
  r = f == 2u ? v2 : r;
  r = f == 3u ? v3 : r;
  r = f == 4u ? v4 : r;
  r = f == 5u ? v5 : r;
  r = f == 6u ? v6 : r;
  r = f == 7u ? v7 : r;
  return r;
}
static_assert(TQK_MAX_FIELDS == 8, "one norm per field");

// The gathers of one doc — a fieldnorm byte, then its cache entry, per field in `fmask` (wave-uniform) — are independent
// of each other and of the lists' bitmap gathers: they are requested together, in front of the lists, not one dependent
// round trip per list (the SC_CHUNK comment in tq_docset_score.hip).  fn0 = the segment's own fieldnorms; `cache` = row
// 0 of the query's F rows; a lane without a doc (`has` false) reads entry 0.
__device__ __forceinline__ float field_norm(const float *cache, uint32_t f, const uint8_t *fp, uint32_t const_id, bool has, uint32_t doc) {
  const uint32_t id = fp ? (has ? (uint32_t)fp[doc] : 0u) : const_id;
  return cache[f * 256u + id];
}
// declares the eight locals fnorm0 .. fnorm7 of the enclosing scope
#define TQ_FIELD_NORMS(cache, fmask, fn0, fn, const_id, has, doc)                                  \
  float fnorm0 = 0.0f, fnorm1 = 0.0f, fnorm2 = 0.0f, fnorm3 = 0.0f, fnorm4 = 0.0f, fnorm5 = 0.0f, fnorm6 = 0.0f, fnorm7 = 0.0f; \
  if ((fmask)&1u) fnorm0 = field_norm(cache, 0u, fn0, const_id, has, doc);                         \
  if ((fmask)&2u) fnorm1 = field_norm(cache, 1u, (fn)[1], const_id, has, doc);                     \
  if ((fmask)&4u) fnorm2 = field_norm(cache, 2u, (fn)[2], const_id, has, doc);                     \
  if ((fmask)&8u) fnorm3 = field_norm(cache, 3u, (fn)[3], const_id, has, doc);                     \
  if ((fmask)&16u) fnorm4 = field_norm(cache, 4u, (fn)[4], const_id, has, doc);                    \
  if ((fmask)&32u) fnorm5 = field_norm(cache, 5u, (fn)[5], const_id, has, doc);                    \
  if ((fmask)&64u) fnorm6 = field_norm(cache, 6u, (fn)[6], const_id, has, doc);                    \
  if ((fmask)&128u) fnorm7 = field_norm(cache, 7u, (fn)[7], const_id, has, doc)
#define TQ_FIELD_NORM_OF(f) pick_field_norm(f, fnorm0, fnorm1, fnorm2, fnorm3, fnorm4, fnorm5, fnorm6, fnorm7)
