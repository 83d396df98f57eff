// tq_term_walk.cpp — the host walk of one posting list: its skip list, vint tail and positions header unrolled into
// the term's blob (block records, coarse table, tails, position tables).  Pure host code over a WalkSource: no HIP
// call, so tools/planbench/walk_check.cpp runs it without a GPU (tests/test_term_walk_cpu.py).
//
// Restates (file:line under the tantivy checkout):
//   skip entries        src/postings/skip.rs:205-253,275-302
//   list framing        src/postings/block_segment_postings.rs:78-88,107-116
//   vint tail           src/postings/compression/vint.rs:44-108
//   positions framing   src/positions/reader.rs:43-56,84-101
// Part of the C ABI library of include/tantivy_amd.h (internal declarations: tq_internal.hpp).
#include "tq_internal.hpp"

namespace tqi {

TermBlobLayout term_blob_layout(uint32_t n_blocks, uint32_t n_buckets, uint32_t n_tail, uint32_t n_pos_blocks,
                                uint32_t n_pos_tail) {
  TermBlobLayout l;
  auto place = [&](size_t bytes) {
    const size_t o = l.total;
    l.total = align16(l.total + bytes);
    return o;
  };
  l.o_rec = place(16 * (size_t)(n_blocks + 1));
  l.o_coarse = place(4 * (size_t)(n_buckets + 1));
  l.o_tdocs = place(4 * (size_t)n_tail);
  l.o_ttfs = place(4 * (size_t)n_tail);
  l.o_pboff = place(8 * (size_t)n_pos_blocks);
  l.o_ptail = place(4 * (size_t)n_pos_tail);
  l.o_self = place(sizeof(TqdTerm));  // the term's own record: what the table-building kernels of its
  l.total += PAD;                     // preparation read (the segment's term table is synced per batch)
  return l;
}

uint32_t coarse_shift(uint32_t max_doc, uint32_t n_blocks, uint32_t *n_buckets) {
  uint32_t shift = 7;
  while (shift < 31 && ((uint64_t)(max_doc - 1) >> shift) + 1 > 2ull * n_blocks + 2) ++shift;
  *n_buckets = (uint32_t)(((uint64_t)(max_doc - 1)) >> shift) + 1;
  return shift;
}

// The caller has checked the postings range (postings_range_ok).
int host_walk_term(const WalkSource &src, uint64_t postings_off, uint32_t postings_len, uint64_t positions_off,
                   uint32_t positions_len, uint32_t doc_freq, WalkedTerm &w) {
  const uint8_t *data = src.idx + 8 + postings_off;
  const size_t len = postings_len;
  const uint64_t abs0 = 8 + postings_off;  // offset of `data` inside the uploaded sub-file

  int record = src.record_option;
  const uint32_t n_full = doc_freq / 128u, n_tail = doc_freq % 128u;
  size_t at = 0;
  const uint8_t *skip = nullptr;
  size_t skip_len = 0;
  if (doc_freq >= 128u) {  // block_segment_postings.rs:78-88
    uint64_t sl;
    if (!read_vint(data, len, at, sl) || sl > len - at)
      return fail(TQ_ERR_FORMAT, "bad skip_len for term at %llu", (unsigned long long)postings_off);
    skip = data + at;
    skip_len = (size_t)sl;
    at += skip_len;
    if (skip_len < 8ull * n_full) record = TQ_BASIC;  // :107-116 (JSON terms without freqs)
  }
  const size_t entry = record == TQ_BASIC ? 5 : (record == TQ_WITH_FREQS ? 8 : 12);
  if (skip_len < entry * n_full)
    return fail(TQ_ERR_FORMAT, "skip data too short: %zu < %zu", skip_len, entry * n_full);
  const bool has_freq = record != TQ_BASIC;
  const size_t payload = at;

  const uint32_t n_blocks = n_full + (n_tail ? 1u : 0u);
  // (scratch kept per thread: eight allocations per term were a third of a sparse term's walk)
  static thread_local std::vector<uint32_t> b_last, b_meta, b_off, block_pos, tail_docs, tail_tfs, coarse;
  b_last.assign(n_blocks, 0u);
  b_meta.assign(n_blocks, 0u);
  b_off.assign(n_blocks, 0u);
  block_pos.assign(n_blocks + 1, 0u);
  size_t running = 0;
  uint64_t running_pos = 0;
  uint32_t last_doc = 0;
  for (uint32_t i = 0; i < n_full; ++i) {  // skip.rs:205-253,275-302
    const uint8_t *e = skip + entry * i;
    const uint32_t ld = rd32(e);
    const uint32_t doc_bits = e[4] & 0x1Fu, strict = (e[4] >> 6) & 1u;
    uint32_t tf_bits = 0, tf_sum = 0, bm_fn = 0, bm_tf = 0;
    if (record == TQ_WITH_FREQS) {
      tf_bits = e[5];
      bm_fn = e[6];
      bm_tf = e[7];
    } else if (record == TQ_WITH_FREQS_AND_POSITIONS) {
      tf_bits = e[5];
      tf_sum = rd32(e + 6);
      bm_fn = e[10];
      bm_tf = e[11];
    }
    if (tf_bits > 32u) return fail(TQ_ERR_FORMAT, "tf bit width %u > 32", tf_bits);
    if (i && ld <= last_doc) return fail(TQ_ERR_FORMAT, "skip last_doc not increasing");
    if (running_pos > 0xFFFFFFFFull)
      return fail(TQ_ERR_UNSUPPORTED, "term with more than 2^32 positions");
    b_last[i] = ld;
    b_meta[i] = doc_bits | (strict << 6) | (tf_bits << 8) | (bm_fn << 16) | (bm_tf << 24);
    b_off[i] = (uint32_t)running;  // < postings_len, a u32 (term_info.rs:10-17)
    block_pos[i] = (uint32_t)running_pos;
    running += 16u * (size_t)(doc_bits + tf_bits);
    running_pos += tf_sum;
    last_doc = ld;
  }
  if (payload + running > len) return fail(TQ_ERR_FORMAT, "bitpacked payload exceeds the list");
  tail_docs.assign(n_tail, 0u);
  tail_tfs.assign(n_tail, 1u);
  if (n_tail) {  // vint.rs:44-108; docs delta from the last full block (0 if none)
    size_t t = payload + running;
    uint32_t prev = n_full ? last_doc : 0u;
    for (uint32_t i = 0; i < n_tail; ++i) {
      uint32_t d;
      if (!read_vint32_block(data, len, t, d)) return fail(TQ_ERR_FORMAT, "truncated vint docs");
      prev += d;
      tail_docs[i] = prev;
    }
    if (has_freq && t < len) {
      for (uint32_t i = 0; i < n_tail; ++i)
        if (!read_vint32_block(data, len, t, tail_tfs[i]))
          return fail(TQ_ERR_FORMAT, "truncated vint term freqs");
    }
    if (running_pos > 0xFFFFFFFFull)
      return fail(TQ_ERR_UNSUPPORTED, "term with more than 2^32 positions");
    b_last[n_full] = tail_docs[n_tail - 1];
    b_meta[n_full] = 0xFFFFFFFFu;
    b_off[n_full] = 0;
    block_pos[n_full] = (uint32_t)running_pos;
    if (record == TQ_WITH_FREQS_AND_POSITIONS)  // tf sums only index a positions stream
      for (uint32_t i = 0; i < n_tail; ++i) running_pos += tail_tfs[i];
    last_doc = tail_docs[n_tail - 1];
  }
  if (running_pos > 0xFFFFFFFFull)
    return fail(TQ_ERR_UNSUPPORTED, "term with more than 2^32 positions");
  block_pos[n_blocks] = (uint32_t)running_pos;
  if (last_doc >= TQ_TERMINATED) return fail(TQ_ERR_FORMAT, "doc id >= TERMINATED");
  if (last_doc >= src.max_doc)
    return fail(TQ_ERR_FORMAT, "doc id %u >= max_doc %u", last_doc, src.max_doc);

  // coarse[b] = first block j with last_doc[j] >= b << shift, about one block per bucket
  uint32_t n_buckets = 0;
  const uint32_t shift = coarse_shift(src.max_doc, n_blocks, &n_buckets);
  coarse.assign(n_buckets + 1, 0u);
  {
    uint32_t j = 0;
    for (uint32_t b = 0; b <= n_buckets; ++b) {
      const uint64_t lo = (uint64_t)b << shift;
      while (j < n_blocks && (uint64_t)b_last[j] < lo) ++j;
      coarse[b] = j;
    }
  }

  // positions stream (positions/reader.rs:43-56,84-101)
  std::vector<uint64_t> pos_block_off;
  std::vector<uint8_t> pos_widths;
  std::vector<uint32_t> pos_tail;
  const bool want_pos = src.record_option == TQ_WITH_FREQS_AND_POSITIONS && src.pos_len != 0 &&
                        record == TQ_WITH_FREQS_AND_POSITIONS;
  if (want_pos) {
    if (positions_off > src.pos_len || (uint64_t)positions_len > src.pos_len - positions_off)
      return fail(TQ_ERR_FORMAT, "positions_range outside the pos file");
    const uint8_t *pd = src.pos + positions_off;
    size_t pa = 0;
    uint64_t nb;
    if (!read_vint(pd, positions_len, pa, nb) || nb > positions_len - pa)
      return fail(TQ_ERR_FORMAT, "bad positions header");
    pos_widths.assign(pd + pa, pd + pa + nb);
    pa += (size_t)nb;
    size_t prun = 0;
    pos_block_off.resize((size_t)nb);
    for (size_t i = 0; i < nb; ++i) {
      if (pos_widths[i] > 32) return fail(TQ_ERR_FORMAT, "position bit width > 32");
      pos_block_off[i] = (uint64_t)(positions_off + pa + prun) | ((uint64_t)pos_widths[i] << 56);
      prun += 16u * (size_t)pos_widths[i];
    }
    size_t t = pa + prun;
    if (t > positions_len) return fail(TQ_ERR_FORMAT, "bitpacked positions exceed the range");
    while (t < positions_len) {  // uncompress_vint_unsorted_until_end
      uint32_t v;
      if (!read_vint32_block(pd, positions_len, t, v))
        return fail(TQ_ERR_FORMAT, "truncated vint positions");
      pos_tail.push_back(v);
    }
    const uint64_t n_pos = (uint64_t)nb * 128u + pos_tail.size();
    if (n_pos != running_pos)
      return fail(TQ_ERR_FORMAT, "positions stream holds %llu values, postings say %llu",
                  (unsigned long long)n_pos, (unsigned long long)running_pos);
  }

  // one blob holding every per-term array
  const TermBlobLayout lay = term_blob_layout(n_blocks, n_buckets, n_tail, (uint32_t)pos_block_off.size(), (uint32_t)pos_tail.size());
  std::vector<uint8_t> &hb = w.hb;
  hb.assign(lay.total, 0);
  for (uint32_t i = 0; i <= n_blocks; ++i) {
    const uint32_t r[4] = {i < n_blocks ? b_last[i] : TQ_TERMINATED, i < n_blocks ? b_meta[i] : 0u,
                           i < n_blocks ? b_off[i] : 0u, block_pos[i]};
    memcpy(hb.data() + lay.o_rec + 16 * (size_t)i, r, 16);
  }
  memcpy(hb.data() + lay.o_coarse, coarse.data(), 4 * coarse.size());
  if (n_tail) {
    memcpy(hb.data() + lay.o_tdocs, tail_docs.data(), 4 * (size_t)n_tail);
    memcpy(hb.data() + lay.o_ttfs, tail_tfs.data(), 4 * (size_t)n_tail);
  }
  if (!pos_block_off.empty()) memcpy(hb.data() + lay.o_pboff, pos_block_off.data(), 8 * pos_block_off.size());
  if (!pos_tail.empty()) memcpy(hb.data() + lay.o_ptail, pos_tail.data(), 4 * pos_tail.size());
  w.lay = lay;
  w.postings_off = postings_off;
  TqdTerm &dt = w.dt;
  dt = TqdTerm{};
  dt.payload_base = abs0 + payload;
  dt.n_full = n_full;
  dt.n_tail = n_tail;
  dt.n_blocks = n_blocks;
  dt.doc_freq = doc_freq;
  dt.n_pos_blocks = (uint32_t)pos_block_off.size();
  dt.n_pos_tail = (uint32_t)pos_tail.size();
  dt.has_freq = has_freq ? 1u : 0u;
  dt.coarse_shift = shift;
  TermHost &th = w.th;
  th = TermHost{};
  th.doc_freq = doc_freq;
  th.n_blocks = n_blocks;
  th.n_full = n_full;
  th.n_tail = n_tail;
  th.last_doc = last_doc;
  th.postings_len = postings_len;
  th.positions_len = want_pos ? positions_len : 0;
  th.n_positions = want_pos ? running_pos : 0;
  return TQ_OK;
}
// the device pointers of a walked term whose blob lives at `blob` (its own record goes into the blob's last slot)
void place_walked_term(WalkedTerm &w, uint8_t *blob) {
  TqdTerm &dt = w.dt;
  dt.rec = (const uint4 *)(blob + w.lay.o_rec);
  dt.coarse = (const uint32_t *)(blob + w.lay.o_coarse);
  dt.tail_docs = (const uint32_t *)(blob + w.lay.o_tdocs);
  dt.tail_tfs = (const uint32_t *)(blob + w.lay.o_ttfs);
  dt.pos_blk = (const uint64_t *)(blob + w.lay.o_pboff);
  dt.pos_tail = (const uint32_t *)(blob + w.lay.o_ptail);
  memcpy(w.hb.data() + w.lay.o_self, &dt, sizeof dt);
  w.th.blob = blob;
  w.th.d_self = (const TqdTerm *)(blob + w.lay.o_self);
}

// what the device walk's status words (tq_prepare.h) say
const char *tqp_message(uint32_t st) {
  switch (st) {
    case TQP_BAD_SKIP_LEN: return "bad skip_len";
    case TQP_SKIP_TOO_SHORT: return "skip data too short";
    case TQP_NOT_INCREASING: return "skip last_doc not increasing";
    case TQP_BAD_TF_WIDTH: return "tf bit width > 32";
    case TQP_TOO_MANY_POSITIONS: return "term with more than 2^32 positions";
    case TQP_PAYLOAD_TOO_LONG: return "bitpacked payload exceeds the list";
    case TQP_TRUNCATED_TAIL: return "truncated vint tail";
    case TQP_DOC_OUT_OF_RANGE: return "doc id >= max_doc / TERMINATED";
    case TQP_BAD_POS_HEADER: return "bad positions header";
    case TQP_POS_COUNT_MISMATCH: return "positions stream and postings disagree on the number of positions";
    case TQP_BAD_POS_WIDTH: return "position bit width > 32";
    case TQP_POS_PAYLOAD_TOO_LONG: return "bitpacked positions exceed the range";
    default: return "unknown";
  }
}

}  // namespace tqi
