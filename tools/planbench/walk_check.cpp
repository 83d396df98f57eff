// The host format walker (host_walk_term of tq_term_walk.cpp) without a GPU, driven by tests/test_term_walk_cpu.py:
//   walk_check IDX POS TERMS RECORD_OPTION MAX_DOC
// IDX / POS: the segment's idx and pos sub-files ("-": no pos file); TERMS: one term per line,
// "postings_off postings_len positions_off positions_len doc_freq".  Printed per term, from the blob the walk leaves:
//   term K ok n_blocks N last_doc D n_positions P shift S
//   rec LAST_DOC META PAYLOAD_OFF POSITIONS_BEFORE      (one per block)
//   tail_docs ... / tail_tfs ... / coarse ...
// or, for a walk that fails:  term K error CODE MESSAGE
#include "../../tantivy_amd/csrc/tq_internal.hpp"

static bool slurp(const char *path, std::vector<uint8_t> &out) {
  FILE *f = fopen(path, "rb");
  if (!f) return false;
  uint8_t buf[65536];
  for (size_t n; (n = fread(buf, 1, sizeof buf, f)) > 0;) out.insert(out.end(), buf, buf + n);
  fclose(f);
  return true;
}

static void print_u32s(const char *name, const uint8_t *p, size_t n) {
  printf("%s", name);
  for (size_t i = 0; i < n; ++i) printf(" %u", rd32(p + 4 * i));
  printf("\n");
}

int main(int argc, char **argv) {
  if (argc != 6) {
    fprintf(stderr, "usage: walk_check IDX POS TERMS RECORD_OPTION MAX_DOC\n");
    return 2;
  }
  std::vector<uint8_t> idx, pos;
  if (!slurp(argv[1], idx) || idx.size() < 8 || (strcmp(argv[2], "-") != 0 && !slurp(argv[2], pos))) {
    fprintf(stderr, "walk_check: cannot read the segment\n");
    return 2;
  }
  FILE *tf = fopen(argv[3], "r");
  if (!tf) return 2;
  const WalkSource src{idx.data(), idx.size(), pos.data(), pos.size(), (uint8_t)atoi(argv[4]), (uint32_t)strtoul(argv[5], nullptr, 10)};
  unsigned long long po, pl, qo, ql, df;
  for (unsigned k = 0; fscanf(tf, "%llu %llu %llu %llu %llu", &po, &pl, &qo, &ql, &df) == 5; ++k) {
    WalkedTerm w;
    int rc = df == 0 ? fail(TQ_ERR_INVALID, "doc_freq 0 (term absent)") : TQ_OK;
    if (rc == TQ_OK && !postings_range_ok(src.idx_len, po, (uint32_t)pl)) rc = bad_postings_range(src.idx_len, po, (uint32_t)pl);
    if (rc == TQ_OK) rc = host_walk_term(src, po, (uint32_t)pl, qo, (uint32_t)ql, (uint32_t)df, w);
    if (rc != TQ_OK) {
      printf("term %u error %d %s\n", k, rc, tq_last_error());
      continue;
    }
    const uint8_t *hb = w.hb.data();
    uint32_t n_buckets = 0;
    coarse_shift(src.max_doc, w.th.n_blocks, &n_buckets);
    printf("term %u ok n_blocks %u last_doc %u n_positions %llu shift %u\n", k, w.th.n_blocks, w.th.last_doc,
           (unsigned long long)w.th.n_positions, w.dt.coarse_shift);
    for (uint32_t i = 0; i < w.th.n_blocks; ++i) print_u32s("rec", hb + w.lay.o_rec + 16 * (size_t)i, 4);
    print_u32s("tail_docs", hb + w.lay.o_tdocs, w.th.n_tail);
    print_u32s("tail_tfs", hb + w.lay.o_ttfs, w.th.n_tail);
    print_u32s("coarse", hb + w.lay.o_coarse, (size_t)n_buckets + 1);
  }
  fclose(tf);
  return 0;
}
