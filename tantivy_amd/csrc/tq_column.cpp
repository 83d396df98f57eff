// tq_column.cpp — fast-field columns and range clauses: tq_column_parse / _upload / _info / _release / _decode and
// tq_range_prepare.  A column is one u64_based column-values blob of the reference (columnar/src/column_values/u64_based/
// mod.rs:79-110: codec byte, ColumnStats, payload), parsed on the host and kept in HBM as the file holds it; a range over
// it is what search_on_u64_ff decides (src/query/range_query/range_query_fastfield.rs:414-450, bound_to_value_range
// :483-503) — restated here on the host — and, where a doc set remains, a term-set slot whose bitmap tq_range.hip fills.
// Part of the C ABI library of include/tantivy_amd.h (internal declarations: tq_internal.hpp).
#include "tq_internal.hpp"

namespace tqi {

namespace {

constexpr uint32_t kBlockRows = 512;  // blockwise_linear.rs:14
constexpr size_t kPayloadPad = 16;    // zero bytes behind the payload: the last value's second and third dword

struct ColumnParsed {
  tq_column_info_t info{};
  size_t payload_at = 0, payload_len = 0;  // the bytes the readers address from bit 0
  uint64_t slope = 0, intercept = 0;       // Linear
  uint32_t width = 0;                      // the readers' bit width (Bitpacked, Linear)
  std::vector<TqkColBlock> blocks;         // BlockwiseLinear
};

// compute_num_bits (bitpacker/src/lib.rs:34-37)
inline uint32_t compute_num_bits(uint64_t n) {
  const uint32_t bits = n ? 64u - (uint32_t)__builtin_clzll(n) : 0u;
  return bits <= 56u ? bits : 64u;
}
inline bool width_ok(uint32_t w) { return w <= 56u || w == 64u; }  // BitUnpacker::new (bitpacker.rs:78-79)
inline uint64_t packed_bytes(uint64_t rows, uint32_t width) { return (rows * width + 7u) / 8u; }

int parse_column(const uint8_t *d, size_t len, ColumnParsed &c) {
  const char *fn = "column-values bytes";
  if (!len) return fail(TQ_ERR_FORMAT, "%s: empty", fn);
  const uint32_t codec = d[0];
  if (codec > TQ_CODEC_BLOCKWISE_LINEAR) return fail(TQ_ERR_FORMAT, "%s: unknown codec byte %u", fn, codec);
  size_t at = 1;
  uint64_t vmin, gcd, amp, rows;
  if (!read_vint(d, len, at, vmin) || !read_vint(d, len, at, gcd) || !read_vint(d, len, at, amp) || !read_vint(d, len, at, rows))
    return fail(TQ_ERR_FORMAT, "%s: truncated ColumnStats", fn);
  if (!gcd) return fail(TQ_ERR_FORMAT, "%s: gcd 0", fn);
  if (rows > 0xFFFFFFFFull) return fail(TQ_ERR_FORMAT, "%s: %llu rows", fn, (unsigned long long)rows);
  uint64_t span, vmax;
  if (__builtin_mul_overflow(amp, gcd, &span) || __builtin_add_overflow(vmin, span, &vmax))
    return fail(TQ_ERR_FORMAT, "%s: min + amplitude does not fit 64 bits", fn);
  c.info.codec = codec;
  c.info.min_value = vmin;
  c.info.max_value = vmax;
  c.info.gcd = gcd;
  c.info.num_rows = (uint32_t)rows;
  if (codec == TQ_CODEC_BITPACKED) {
    c.width = c.info.num_bits = compute_num_bits(amp);
    c.payload_at = at;
    c.payload_len = len - at;
    if (c.payload_len < packed_bytes(rows, c.width))
      return fail(TQ_ERR_FORMAT, "%s: Bitpacked payload of %zu bytes, %llu rows of %u bits", fn, c.payload_len,
                  (unsigned long long)rows, c.width);
  } else if (codec == TQ_CODEC_LINEAR) {
    if (!read_vint(d, len, at, c.slope) || !read_vint(d, len, at, c.intercept) || at >= len)
      return fail(TQ_ERR_FORMAT, "%s: truncated Linear parameters", fn);
    c.width = d[at++];
    if (!width_ok(c.width)) return fail(TQ_ERR_FORMAT, "%s: Linear bit width %u", fn, c.width);
    c.payload_at = at;
    c.payload_len = len - at;
    if (c.payload_len < packed_bytes(rows, c.width))
      return fail(TQ_ERR_FORMAT, "%s: Linear payload of %zu bytes, %llu rows of %u bits", fn, c.payload_len,
                  (unsigned long long)rows, c.width);
  } else {
    // data | footer: ceil(rows / 512) x (Line, bit width) | u32 footer_len (blockwise_linear.rs:157-194)
    if (len - at < 4u) return fail(TQ_ERR_FORMAT, "%s: truncated BlockwiseLinear footer length", fn);
    const uint64_t footer_len = rd32(d + len - 4);
    if (footer_len > len - at - 4u) return fail(TQ_ERR_FORMAT, "%s: BlockwiseLinear footer of %llu bytes does not fit", fn,
                                                 (unsigned long long)footer_len);
    const size_t footer_at = len - 4u - (size_t)footer_len, footer_end = len - 4u;
    c.payload_at = at;
    c.payload_len = footer_at - at;
    const uint64_t n_blocks = (rows + kBlockRows - 1u) / kBlockRows;
    if (n_blocks * 3u > footer_len)  // (a block is at least three bytes: no allocation beyond what the bytes can hold)
      return fail(TQ_ERR_FORMAT, "%s: BlockwiseLinear footer of %llu bytes, %llu blocks", fn, (unsigned long long)footer_len,
                  (unsigned long long)n_blocks);
    c.blocks.resize((size_t)n_blocks);
    size_t fat = footer_at;
    uint64_t data_off = 0;
    for (uint64_t b = 0; b < n_blocks; ++b) {
      TqkColBlock &blk = c.blocks[(size_t)b];
      if (!read_vint(d, footer_end, fat, blk.slope) || !read_vint(d, footer_end, fat, blk.intercept) || fat >= footer_end)
        return fail(TQ_ERR_FORMAT, "%s: truncated BlockwiseLinear footer (block %llu)", fn, (unsigned long long)b);
      blk.bit_width = d[fat++];
      blk.pad_ = 0;
      if (!width_ok(blk.bit_width)) return fail(TQ_ERR_FORMAT, "%s: block %llu: bit width %u", fn, (unsigned long long)b, blk.bit_width);
      blk.data_off = data_off;
      const uint64_t in_block = std::min<uint64_t>(kBlockRows, rows - b * kBlockRows);
      if (data_off + packed_bytes(in_block, blk.bit_width) > c.payload_len)
        return fail(TQ_ERR_FORMAT, "%s: block %llu: its %llu rows of %u bits end past the %zu data bytes", fn, (unsigned long long)b,
                    (unsigned long long)in_block, blk.bit_width, c.payload_len);
      data_off += (uint64_t)blk.bit_width * kBlockRows / 8u;
    }
  }
  c.info.resident_bytes = ((c.payload_len + 3u) & ~(size_t)3) + kPayloadPad + c.blocks.size() * sizeof(TqkColBlock);
  return TQ_OK;
}

void free_column(tq_segment::ColumnHost &c) {
  if (c.d_payload) (void)hipFree(c.d_payload);
  if (c.d_blocks) (void)hipFree(c.d_blocks);
  if (c.d_present) (void)hipFree(c.d_present);
  c = tq_segment::ColumnHost{};
}

inline size_t table_words(const tq_segment *s) { return ((size_t)s->max_doc + 31u) / 32u; }
inline uint32_t total_word_at(size_t n_words) {
  return std::max<uint32_t>(1u, (uint32_t)((n_words + tqk_termset_scan_tile() - 1u) / tqk_termset_scan_tile()));
}

int live_column(tq_segment *s, uint32_t column, const char *fn) {
  if (column >= TQ_MAX_COLUMNS || !s->columns[column].live)
    return fail(TQ_ERR_INVALID, "%s: column %u is not a live column of the segment", fn, column);
  return TQ_OK;
}

}  // namespace

void free_columns(tq_segment *s) {
  for (tq_segment::ColumnHost &c : s->columns) free_column(c);
}

}  // namespace tqi

extern "C" {

int tq_column_parse(const uint8_t *values, size_t values_len, tq_column_info_t *out) {
  if (!values || !out) return fail(TQ_ERR_INVALID, "tq_column_parse: null argument");
  try {
    ColumnParsed c;
    const int rc = parse_column(values, values_len, c);
    if (rc != TQ_OK) return rc;
    *out = c.info;
    return TQ_OK;
  } catch (const std::exception &e) {
    return fail(TQ_ERR_INVALID, "tq_column_parse: %s", e.what());
  }
}

int tq_column_upload(tq_segment *s, const uint8_t *values, size_t values_len, uint8_t cardinality, const uint32_t *present_words,
                     uint32_t *out_column) {
  if (!s || !values || !out_column) return fail(TQ_ERR_INVALID, "tq_column_upload: null argument");
  if (cardinality == TQ_CARD_MULTIVALUED)
    return fail(TQ_ERR_UNSUPPORTED, "tq_column_upload: a multivalued column stays on the CPU");
  if (cardinality > TQ_CARD_MULTIVALUED) return fail(TQ_ERR_INVALID, "tq_column_upload: cardinality %u", cardinality);
  try {
    TQ_SEGMENT_LOCK(s);
    ColumnParsed c;
    int rc = parse_column(values, values_len, c);
    if (rc != TQ_OK) return rc;
    const size_t n_words = table_words(s);
    std::vector<uint2> present;
    if (cardinality == TQ_CARD_FULL) {
      if (present_words) return fail(TQ_ERR_FORMAT, "tq_column_upload: a TQ_CARD_FULL column takes no presence words");
      if (c.info.num_rows != s->max_doc)
        return fail(TQ_ERR_FORMAT, "tq_column_upload: a TQ_CARD_FULL column of %u rows on a segment of %u docs", c.info.num_rows, s->max_doc);
    } else {
      if (!present_words && n_words) return fail(TQ_ERR_INVALID, "tq_column_upload: a TQ_CARD_OPTIONAL column needs its presence words");
      present.resize(n_words + 1u);
      uint64_t pop = 0;
      for (size_t w = 0; w < n_words; ++w) {
        uint32_t x = present_words[w];
        if (w == n_words - 1u && (s->max_doc & 31u)) x &= (1u << (s->max_doc & 31u)) - 1u;  // (bits at or above max_doc)
        present[w] = make_uint2(x, 0u);
        pop += (uint32_t)__builtin_popcount(x);
      }
      present[n_words] = make_uint2(0u, 0u);
      if (pop != c.info.num_rows)
        return fail(TQ_ERR_FORMAT, "tq_column_upload: %llu docs have a value, the column has %u rows", (unsigned long long)pop, c.info.num_rows);
    }
    uint32_t slot = 0;
    while (slot < TQ_MAX_COLUMNS && s->columns[slot].live) ++slot;
    if (slot == TQ_MAX_COLUMNS) return fail(TQ_ERR_INVALID, "tq_column_upload: the segment holds %u columns already", TQ_MAX_COLUMNS);
    HIP_TRY(hipSetDevice(s->device));
    tq_segment::ColumnHost col;
    col.info = c.info;
    col.info.cardinality = cardinality;
    col.payload_len = c.payload_len;
    const size_t padded = ((c.payload_len + 3u) & ~(size_t)3) + kPayloadPad;
    hipError_t e = hipMalloc(&col.d_payload, padded);
    if (e == hipSuccess) e = hipMemsetAsync(col.d_payload, 0, padded, s->stream);
    if (e == hipSuccess && c.payload_len)
      e = hipMemcpyAsync(col.d_payload, values + c.payload_at, c.payload_len, hipMemcpyHostToDevice, s->stream);
    if (e == hipSuccess && !c.blocks.empty()) {
      e = hipMalloc(&col.d_blocks, c.blocks.size() * sizeof(TqkColBlock));
      if (e == hipSuccess)
        e = hipMemcpyAsync(col.d_blocks, c.blocks.data(), c.blocks.size() * sizeof(TqkColBlock), hipMemcpyHostToDevice, s->stream);
    }
    if (e == hipSuccess && cardinality == TQ_CARD_OPTIONAL) {
      // the presence bits get their rank directory from the term sets' scan: row = rank before the word + bits below
      rc = s->d_set_work.ensure(tqk_termset_scratch_words((uint32_t)n_words) * sizeof(uint32_t));
      if (rc != TQ_OK) {
        free_column(col);
        return rc;
      }
      e = hipMalloc(&col.d_present, present.size() * sizeof(uint2));
      if (e == hipSuccess) e = hipMemcpyAsync(col.d_present, present.data(), present.size() * sizeof(uint2), hipMemcpyHostToDevice, s->stream);
      if (e == hipSuccess) e = tqk_launch_bitmap_rank((uint2 *)col.d_present, (uint32_t)n_words, s->max_doc, (uint32_t *)s->d_set_work.p, s->stream);
      col.info.resident_bytes += present.size() * sizeof(uint2);
    }
    if (e == hipSuccess) e = hipStreamSynchronize(s->stream);  // (the host buffers above live until here)
    if (e != hipSuccess) {
      (void)hipStreamSynchronize(s->stream);
      free_column(col);
      return fail(TQ_ERR_HIP, "tq_column_upload: %s", hipGetErrorString(e));
    }
    col.dev.payload = (const uint32_t *)col.d_payload;
    col.dev.blocks = (const TqkColBlock *)col.d_blocks;
    col.dev.present = (const uint2 *)col.d_present;
    col.dev.slope = c.slope;
    col.dev.intercept = c.intercept;
    col.dev.codec = c.info.codec;
    col.dev.num_bits = c.width;
    col.dev.num_rows = c.info.num_rows;
    col.dev.max_doc = s->max_doc;
    col.live = true;
    s->columns[slot] = col;
    *out_column = slot;
    return TQ_OK;
  } catch (const std::exception &e) {
    return fail(TQ_ERR_HIP, "tq_column_upload: %s", e.what());
  }
}

int tq_column_info(tq_segment *s, uint32_t column, tq_column_info_t *out) {
  if (!s || !out) return fail(TQ_ERR_INVALID, "tq_column_info: null argument");
  TQ_SEGMENT_LOCK(s);
  const int rc = live_column(s, column, "tq_column_info");
  if (rc != TQ_OK) return rc;
  *out = s->columns[column].info;
  return TQ_OK;
}

int tq_column_release(tq_segment *s, uint32_t column) {
  if (!s) return fail(TQ_ERR_INVALID, "tq_column_release: null segment");
  TQ_SEGMENT_LOCK(s);
  const int rc = live_column(s, column, "tq_column_release");
  if (rc != TQ_OK) return rc;
  HIP_TRY(hipSetDevice(s->device));
  {
    const int wrc = wait_segment_idle(s);
    if (wrc != TQ_OK) return wrc;
  }
  free_column(s->columns[column]);
  return TQ_OK;
}

int tq_column_decode(tq_segment *s, uint32_t column, uint32_t first_row, uint32_t n, uint64_t *out_host) {
  if (!s || (!out_host && n)) return fail(TQ_ERR_INVALID, "tq_column_decode: null argument");
  TQ_SEGMENT_LOCK(s);
  int rc = live_column(s, column, "tq_column_decode");
  if (rc != TQ_OK) return rc;
  const tq_segment::ColumnHost &col = s->columns[column];
  if ((uint64_t)first_row + n > col.info.num_rows)
    return fail(TQ_ERR_INVALID, "tq_column_decode: rows [%u, %llu) of a column of %u rows", first_row,
                (unsigned long long)first_row + n, col.info.num_rows);
  if (!n) return TQ_OK;
  HIP_TRY(hipSetDevice(s->device));
  uint64_t *d_out = nullptr;
  HIP_TRY(hipMalloc((void **)&d_out, (size_t)n * sizeof(uint64_t)));
  hipError_t e = tqk_launch_column_decode(col.dev, col.info.min_value, col.info.gcd, first_row, n, d_out, s->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(out_host, d_out, (size_t)n * sizeof(uint64_t), hipMemcpyDeviceToHost, s->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(s->stream);
  if (e != hipSuccess) (void)hipStreamSynchronize(s->stream);
  (void)hipFree(d_out);
  return e == hipSuccess ? TQ_OK : fail(TQ_ERR_HIP, "tq_column_decode: %s", hipGetErrorString(e));
}

int tq_range_prepare(tq_segment *s, uint32_t column, uint8_t lower_kind, uint64_t lower, uint8_t upper_kind, uint64_t upper, float boost,
                     tq_term_handle *out, float *out_weight) {
  if (!s || !out || !out_weight) return fail(TQ_ERR_INVALID, "tq_range_prepare: null argument");
  if (lower_kind > TQ_BOUND_EXCLUDED || upper_kind > TQ_BOUND_EXCLUDED)
    return fail(TQ_ERR_INVALID, "tq_range_prepare: bound kinds %u, %u", lower_kind, upper_kind);
  if (lower_kind == TQ_BOUND_UNBOUNDED && upper_kind == TQ_BOUND_UNBOUNDED) {  // AllScorer, before the column is opened
    *out = TQ_TERM_ALL;
    *out_weight = 1.0f;
    return TQ_OK;
  }
  try {
    TQ_SEGMENT_LOCK(s);
    int rc = live_column(s, column, "tq_range_prepare");
    if (rc != TQ_OK) return rc;
    const tq_segment::ColumnHost &col = s->columns[column];
    const uint64_t vmin = col.info.min_value, vmax = col.info.max_value, gcd = col.info.gcd;
    // bound_to_value_range (:483-503), then the column's own bounds
    bool empty = col.info.num_rows == 0;
    uint64_t start = vmin, end = vmax;
    if (lower_kind == TQ_BOUND_INCLUDED) start = lower;
    if (lower_kind == TQ_BOUND_EXCLUDED) {
      if (lower == ~0ull) empty = true;
      start = lower + 1u;
    }
    if (start < vmin) start = vmin;
    if (upper_kind == TQ_BOUND_INCLUDED) end = upper;
    if (upper_kind == TQ_BOUND_EXCLUDED) {
      if (upper == 0ull) empty = true;
      end = upper - 1u;
    }
    if (start > end || start > vmax || end < vmin) empty = true;
    if (!empty && col.info.cardinality == TQ_CARD_FULL && vmin >= start && vmax <= end && boost == 1.0f) {
      *out = TQ_TERM_ALL;  // every value lies in the range: an AllScorer to the boolean weight
      *out_weight = 1.0f;
      return TQ_OK;
    }
    // the packed domain: Bitpacked and BlockwiseLinear store (value - min) / gcd (start, end >= min here); Linear the value
    uint64_t lo = start, hi = end;
    if (!empty && col.info.codec != TQ_CODEC_LINEAR) {
      lo = (start - vmin) / gcd + ((start - vmin) % gcd ? 1u : 0u);
      hi = (end - vmin) / gcd;
    }
    HIP_TRY(hipSetDevice(s->device));
    const size_t n_words = table_words(s);
    void *tab = nullptr;
    rc = set_table_acquire(s, &tab);
    if (rc != TQ_OK) return rc;
    rc = s->d_set_work.ensure(tqk_termset_scratch_words((uint32_t)n_words) * sizeof(uint32_t));
    if (rc != TQ_OK) {
      set_table_release(s, tab);
      return rc;
    }
    uint32_t *const scratch = (uint32_t *)s->d_set_work.p;
    uint32_t n_docs = 0;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    hipError_t e = hipSuccess;
    if (s->opt.timing) {
      e = hipEventCreate(&ev0);
      if (e == hipSuccess) e = hipEventCreate(&ev1);
    }
    if (e == hipSuccess && ev0) e = hipEventRecord(ev0, s->stream);
    if (e == hipSuccess) e = hipMemsetAsync(tab, 0, (n_words + 1u) * sizeof(uint2), s->stream);
    if (e == hipSuccess && !empty) {
      e = tqk_launch_range_fill(col.dev, lo, hi, (uint2 *)tab, (uint32_t)n_words, s->stream);
      if (e == hipSuccess) e = tqk_launch_bitmap_rank((uint2 *)tab, (uint32_t)n_words, s->max_doc, scratch, s->stream);
    }
    if (e == hipSuccess && ev1) e = hipEventRecord(ev1, s->stream);
    if (e == hipSuccess && !empty)
      e = hipMemcpyAsync(&n_docs, scratch + total_word_at(n_words), sizeof n_docs, hipMemcpyDeviceToHost, s->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(s->stream);
    float build_ms = 0.0f;
    if (e == hipSuccess && ev0 && ev1) e = hipEventElapsedTime(&build_ms, ev0, ev1);
    if (ev0) (void)hipEventDestroy(ev0);
    if (ev1) (void)hipEventDestroy(ev1);
    if (e != hipSuccess) {
      (void)hipStreamSynchronize(s->stream);
      set_table_release(s, tab);
      return fail(TQ_ERR_HIP, "tq_range_prepare: %s", hipGetErrorString(e));
    }
    if (s->opt.timing) {  // (the last call's figures, as after tq_term_set_prepare)
      s->stats = tq_batch_stats{};
      s->stats_pending = false;
      s->stats.kernel_ms = s->stats.total_ms = build_ms;
      s->stats.batches_averaged = 1;
      // the HBM model of the build: the payload once + 8 B per 32 docs written and read once by the scan + 8 B per 32 docs
      // of presence table
      s->stats.algorithmic_bytes =
          empty ? 0ull : col.payload_len + 2ull * n_words * sizeof(uint2) + (col.d_present ? (uint64_t)n_words * sizeof(uint2) : 0ull);
    }
    *out = set_slot_commit(s, tab, n_docs);
    *out_weight = boost;
    return TQ_OK;
  } catch (const std::exception &e) {
    return fail(TQ_ERR_HIP, "tq_range_prepare: %s", e.what());
  }
}

}  // extern "C"
