// tq_fields.cpp — multi-field segments (include/tantivy_amd.h "multi-field segments"; the upload: tq_api.cpp): the
// field entry points of term preparation — a term's offsets are relative to ITS field's sub-files, the library adds the
// field's bases and everything behind works on the shifted offsets —, the handle's field, the statistics, and the one
// check of a query's fields (a phrase over two fields).
// Part of the C ABI library of include/tantivy_amd.h (internal declarations: tq_internal.hpp).
#include "tq_internal.hpp"

namespace tqi {
namespace {
// field f's TermInfo ranges inside field f's sub-files, then shifted into the concatenation
int shift_term_info(const tq_segment *s, uint32_t field, const tq_term_info &in, tq_term_info &out, const char *fn) {
  if (field >= s->n_fields) return fail(TQ_ERR_INVALID, "%s: field %u of a segment with %u field(s)", fn, field, s->n_fields);
  out = in;
  if (s->n_fields == 1) return TQ_OK;
  if (!postings_range_ok((size_t)s->field_idx_len[field], in.postings_off, in.postings_len))
    return bad_postings_range((size_t)s->field_idx_len[field], in.postings_off, in.postings_len);
  if (s->field_pos_len[field] &&
      (in.positions_off > s->field_pos_len[field] || (uint64_t)in.positions_len > s->field_pos_len[field] - in.positions_off))
    return fail(TQ_ERR_FORMAT, "positions_range outside field %u's pos file", field);
  out.postings_off = in.postings_off + s->field_idx_base[field];
  if (s->field_pos_len[field])
    out.positions_off = in.positions_off + s->field_pos_base[field];
  else  // a field without positions on a segment where another field has them: the list has none
    out.positions_off = 0, out.positions_len = 0;
  return TQ_OK;
}
}  // namespace

int check_field_query(const tq_segment *s, const tq_query &q, uint32_t qi, const char *fn) {
  if (!q.terms || q.n_terms > TQ_MAX_TERMS) return TQ_OK;  // (reported by the planner)
  if (q.mode == TQ_MODE_PHRASE) {
    uint32_t f0 = 0xFFFFFFFFu;
    for (uint32_t i = 0; i < q.n_terms; ++i) {
      if (q.terms[i] >= s->terms.size()) continue;
      const uint32_t f = s->terms[q.terms[i]].field;
      if (f0 != 0xFFFFFFFFu && f != f0)
        return fail(TQ_ERR_INVALID, "%s: query %u: a phrase over terms of different fields (%u and %u)", fn, qi, f0, f);
      f0 = f;
    }
    return TQ_OK;
  }
  if (q.mode != TQ_MODE_BOOL || !q.nested_occurs || !q.atom_of) return TQ_OK;
  for (uint32_t i = 0; i < q.n_terms; ++i) {
    if (q.nested_occurs[i] == 255u || !(q.nested_occurs[i] & TQ_NESTED_PHRASE) || q.terms[i] >= s->terms.size()) continue;
    for (uint32_t j = 0; j < i; ++j) {
      if (q.nested_occurs[j] == 255u || !(q.nested_occurs[j] & TQ_NESTED_PHRASE) || q.terms[j] >= s->terms.size()) continue;
      if (q.atom_of[i] != q.atom_of[j] || (q.clause_of ? q.clause_of[i] != q.clause_of[j] : true)) continue;
      if (s->terms[q.terms[i]].field != s->terms[q.terms[j]].field)
        return fail(TQ_ERR_INVALID, "%s: query %u: a phrase over terms of different fields (%u and %u)", fn, qi,
                    (uint32_t)s->terms[q.terms[j]].field, (uint32_t)s->terms[q.terms[i]].field);
    }
  }
  return TQ_OK;
}
}  // namespace tqi

extern "C" {

int tq_term_prepare_field(tq_segment *s, uint32_t field, uint64_t postings_off, uint32_t postings_len,
                          uint64_t positions_off, uint32_t positions_len, uint32_t doc_freq, tq_term_handle *out) {
  if (!s || !out) return fail(TQ_ERR_INVALID, "tq_term_prepare_field: null argument");
  TQ_SEGMENT_LOCK(s);
  tq_term_info in{}, sh{};
  in.postings_off = postings_off;
  in.positions_off = positions_off;
  in.postings_len = postings_len;
  in.positions_len = positions_len;
  in.doc_freq = doc_freq;
  const int rc = shift_term_info(s, field, in, sh, "tq_term_prepare_field");
  if (rc != TQ_OK) return rc;
  FieldScope scope(s, (uint8_t)field);
  return term_prepare_shifted(s, sh.postings_off, sh.postings_len, sh.positions_off, sh.positions_len, sh.doc_freq, out);
}

int tq_term_prepare_batch_fields(tq_segment *s, const tq_term_info *infos, const uint8_t *fields, uint32_t n,
                                 tq_term_handle *out) {
  if (!s || (!infos && n) || (!out && n)) return fail(TQ_ERR_INVALID, "tq_term_prepare_batch_fields: null argument");
  if (s->n_fields == 1) {
    for (uint32_t i = 0; fields && i < n; ++i)
      if (fields[i]) return fail(TQ_ERR_INVALID, "tq_term_prepare_batch_fields: field %u of a segment with 1 field(s)", (uint32_t)fields[i]);
    return term_prepare_batch_shifted(s, infos, n, out, 0);
  }
  // one staged call per field that is named (the terms of one call are tagged together)
  std::vector<tq_term_info> shifted;
  std::vector<uint32_t> at;
  std::vector<tq_term_handle> handles;
  for (uint32_t f = 0; f < TQ_MAX_FIELDS; ++f) {
    shifted.clear();
    at.clear();
    for (uint32_t i = 0; i < n; ++i) {
      const uint32_t fi = fields ? fields[i] : 0u;
      if (fi >= s->n_fields)
        return fail(TQ_ERR_INVALID, "tq_term_prepare_batch_fields: field %u of a segment with %u field(s)", fi, s->n_fields);
      if (fi != f) continue;
      tq_term_info sh;
      const int rc = shift_term_info(s, f, infos[i], sh, "tq_term_prepare_batch_fields");
      if (rc != TQ_OK) return rc;
      shifted.push_back(sh);
      at.push_back(i);
    }
    if (shifted.empty()) continue;
    handles.assign(shifted.size(), TQ_TERM_ABSENT);
    const int rc = term_prepare_batch_shifted(s, shifted.data(), (uint32_t)shifted.size(), handles.data(), (uint8_t)f);
    if (rc != TQ_OK) return rc;
    for (size_t k = 0; k < at.size(); ++k) out[at[k]] = handles[k];
  }
  return TQ_OK;
}

int tq_term_field(tq_segment *s, tq_term_handle term, uint32_t *field) {
  if (!s || !field) return fail(TQ_ERR_INVALID, "tq_term_field: null argument");
  TQ_SEGMENT_LOCK(s);
  if (term >= s->terms.size()) return fail(TQ_ERR_INVALID, "unknown term handle %u", term);
  *field = s->terms[term].field;
  return TQ_OK;
}

int tq_segment_get_fields_stats(tq_segment *s, tq_fields_stats *out) {
  if (!s || !out) return fail(TQ_ERR_INVALID, "tq_segment_get_fields_stats: null argument");
  TQ_SEGMENT_LOCK(s);
  tq_fields_stats r{};
  r.n_fields = s->n_fields;
  r.n_field_terms = s->n_field_terms;
  for (uint32_t f = 1; f < s->n_fields; ++f)
    if (s->d_fn_field[f]) r.extra_fieldnorm_bytes += s->max_doc;
  *out = r;
  return TQ_OK;
}

}  // extern "C"
