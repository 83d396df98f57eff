// Host-only check of the launch ORDER build_ashare_plan gives the shared intersections' tasks (option
// "ashare_inline_warm"), driven by tests/test_ashare_order_cpu.py; built like plan_check.cpp.
//   order_check <max_doc> <n_queries> <resident wavefronts>
// plans one group — 2-term ANDs over 256 Zipf lists whose other list has a bitmap, the group of plan_bench.cpp's
// bench_ashare (10 000 000 docs, 10 000 queries: the headline) — with the option at 0, 1 and 2 and checks:
//   * every (leader, lead group) covers the leader's blocks exactly once, in every mode;
//   * band 1, tasks [0, a_warm_tasks), is exactly the warm-up tasks (the first 2 permille of a leader's blocks);
//   * with one dispatch (a_inline) band 2, tasks [a_warm_tasks, a_dep_tasks), holds only tasks of leaders WITHOUT warm-up
//     tasks: those of the first doc slices, as few slices as give every resident wavefront that finds no warm-up task
//     one; no task of a leader that has warm-up tasks stands before a_dep_tasks; bands 2 and 3 are each in
//     non-decreasing doc-slice order;
//   * the recorded boundaries (a_warm_tasks, a_dep_tasks) and a_inline are what the tasks and the rule say;
//   * with the option at 0 the table is, byte for byte, the same tasks under the ordering rule of before the option:
//     warm-up tasks first, then 4 096 doc slices, stable in (leader run, first block, lead group).
#include "../../tantivy_amd/csrc/tq_internal.hpp"

#include <map>
#include <random>

static int fail_msg(const char *m, long a = 0, long b = 0) {
  fprintf(stderr, "order_check: %s (%ld, %ld)\n", m, a, b);
  return 1;
}

static uint32_t slice_of(uint32_t j0, uint32_t n_blocks) {  // the planner's (j0 << 12) / n_blocks
  return std::min<uint32_t>(4095u, (uint32_t)((j0 * (((uint64_t)1 << 44) / n_blocks)) >> 32));
}

int main(int argc, char **argv) {
  const uint32_t max_doc = argc > 1 ? (uint32_t)atol(argv[1]) : 10000000u;
  const int n_queries = argc > 2 ? atoi(argv[2]) : 10000;
  const uint32_t resident = argc > 3 ? (uint32_t)atol(argv[3]) : 1280u;
  const uint32_t n_terms = 256;
  const uint32_t warm_permille = getenv("TQ_AS_WARM_PERMILLE") ? (uint32_t)atoi(getenv("TQ_AS_WARM_PERMILLE")) : 2u;
  tq_segment seg;
  static uint8_t arena[1 << 21];
  for (uint32_t t = 0; t < n_terms; ++t) {
    TermHost th;
    th.doc_freq = max_doc / 2 / (t + 1);
    th.n_blocks = (th.doc_freq + 127) / 128;
    TqdTerm dt{};
    dt.has_freq = 1u;
    if (t < 64) {
      th.dense_blob = arena + 4096u * t + 8u;
      th.tf8_blob = arena + 4096u * t + 2048u;
    }
    if (t < TQD_MAT_SLOTS) dt.has_freq |= (t + 1u) << 8;
    else dt.has_freq |= ((t * 7u) % TQD_SIG_BITS + 1u) << 16;
    seg.terms.push_back(th);
    seg.h_dterms.push_back(dt);
  }
  seg.max_doc = max_doc;
  seg.share_table_lo = (uint64_t)arena;
  std::vector<double> cdf(n_terms);
  double acc = 0;
  for (uint32_t r = 0; r < n_terms; ++r) cdf[r] = (acc += 1.0 / (r + 1));
  auto nb_warm = [&](uint32_t term) { return (uint32_t)((uint64_t)seg.terms[term].n_blocks * warm_permille / 1000u); };

  std::vector<uint4> table[3];
  std::vector<TqdALead> leads0;
  for (int mode = 0; mode < 3; ++mode) {
    PlanScratch ps;
    Group &g = ps.groups[kGAShare];
    g.reset();
    g.mode = TQ_MODE_AND;
    std::mt19937 rng(7);
    for (int q = 0; q < n_queries; ++q) {
      TqdQuery dq{};
      uint32_t a, b;
      do {
        a = (uint32_t)(std::lower_bound(cdf.begin(), cdf.end(), std::uniform_real_distribution<double>(0, acc)(rng)) - cdf.begin());
        b = (uint32_t)(std::lower_bound(cdf.begin(), cdf.end(), std::uniform_real_distribution<double>(0, acc)(rng)) - cdf.begin());
      } while (a == b || std::min(a, b) >= 64);
      dq.n_terms = 2;
      dq.k = 10;
      dq.flags = TQD_QF_PRUNE;
      dq.thr_index = (uint32_t)q;
      dq.term[0] = std::max(a, b);
      dq.term[1] = std::min(a, b);
      for (int i = 0; i < 2; ++i)
        dq.weight[i] = 2.2f * logf(1.0f + (max_doc - seg.terms[dq.term[i]].doc_freq + 0.5f) / (seg.terms[dq.term[i]].doc_freq + 0.5f));
      g.queries.push_back(dq);
      g.tile_cost.push_back(1);
      g.out_index.push_back((uint32_t)q);
      g.max_k = 10;
    }
    seg.opt.ashare_inline_warm = mode;
    if (build_ashare_plan(&seg, g, ps, false, resident) != TQ_OK) return fail_msg("build_ashare_plan failed", mode);
    const PlanScratch::ASharePlan &A = ps.ap[0];
    const std::vector<uint4> &tasks = A.atasks;
    table[mode] = tasks;
    if (mode == 0) leads0 = A.aleads;
    else if (leads0.size() != A.aleads.size() || memcmp(leads0.data(), A.aleads.data(), leads0.size() * sizeof(TqdALead)))
      return fail_msg("the leads depend on the option", mode);

    // coverage: the runs of every (first lead, leads) pair tile the leader's blocks exactly once
    std::map<std::pair<uint32_t, uint32_t>, std::vector<std::pair<uint32_t, uint32_t>>> runs_of;
    uint64_t n_warm = 0, n_indep = 0;
    uint32_t leaders_with = 0, leaders_without = 0;
    std::map<uint32_t, bool> seen_leader;
    for (size_t ti = 0; ti < tasks.size(); ++ti) {
      const uint4 t = tasks[ti];
      const uint32_t nb = t.z & 0xFFFFu, nl = (t.z >> 16) & 0xFFu;
      if (!nb || !nl || t.x >= n_terms || t.w + nl > A.aleads.size()) return fail_msg("task shape", mode, (long)ti);
      runs_of[{t.w, nl}].push_back({t.y, nb});
      const uint32_t w = nb_warm(t.x);
      const bool warm = t.y < w;
      if (warm && t.y + nb > w) return fail_msg("a warm-up task runs into the main blocks", mode, (long)ti);
      n_warm += warm;
      n_indep += !warm && w == 0;
      if (!seen_leader.count(t.x)) {
        seen_leader[t.x] = true;
        (w ? leaders_with : leaders_without)++;
      }
      // band 1 is exactly the warm-up tasks
      if ((ti < A.a_warm_tasks) != warm) return fail_msg("band 1 is not the warm-up tasks", mode, (long)ti);
    }
    for (auto &kv : runs_of) {
      std::sort(kv.second.begin(), kv.second.end());
      uint32_t at = 0;
      for (auto &r : kv.second) {
        if (r.first != at) return fail_msg("runs do not tile the list", mode, (long)kv.first.first);
        at += r.second;
      }
      if (at != seg.terms[g.queries[A.aleads[kv.first.first].query].term[0]].n_blocks)
        return fail_msg("list not covered", mode, (long)kv.first.first);
    }
    if (A.a_warm_tasks != n_warm) return fail_msg("a_warm_tasks", mode, (long)A.a_warm_tasks);
    // the rule: one dispatch when band 2 gives every resident wavefront that finds no warm-up task a task to take
    const uint64_t grid = std::min<uint64_t>(tasks.size(), resident);
    const bool want_inline = n_warm != 0 && (mode == 2 || (mode == 1 && resident != 0 && n_indep >= grid - std::min(grid, n_warm)));
    if (A.a_inline != want_inline) return fail_msg("a_inline", mode, (long)A.a_inline);
    const uint64_t band2 = A.a_dep_tasks - A.a_warm_tasks, want2 = std::min<uint64_t>(n_indep, grid - std::min(grid, n_warm));
    if (A.a_dep_tasks < A.a_warm_tasks || A.a_dep_tasks > tasks.size()) return fail_msg("a_dep_tasks", mode, (long)A.a_dep_tasks);
    if (A.a_inline ? band2 < want2 : band2 != 0) return fail_msg("band 2 is shorter than the rule wants", mode, (long)band2);
    uint32_t last = 0, band2_last = 0;
    for (size_t ti = A.a_warm_tasks; ti < tasks.size(); ++ti) {
      const uint4 t = tasks[ti];
      const bool dep = nb_warm(t.x) != 0;
      if (ti < A.a_dep_tasks && dep) return fail_msg("a task of a leader with warm-up tasks in band 2", mode, (long)ti);
      if (ti == A.a_dep_tasks) {  // (band 3 sweeps the doc-id space again)
        band2_last = last;
        last = 0;
      }
      const uint32_t sl = A.a_inline ? slice_of(t.y, seg.terms[t.x].n_blocks) >> 1 : slice_of(t.y, seg.terms[t.x].n_blocks);
      if (sl < last) return fail_msg("a band is not in doc-slice order", mode, (long)ti);
      last = sl;
      // band 2 is a PREFIX of the independent tasks in slice order: those left to band 3 come from later slices
      if (A.a_inline && ti >= A.a_dep_tasks && !dep && band2 && sl <= band2_last) return fail_msg("an independent task of band 2's slices in band 3", mode, (long)ti);
    }
    if (A.a_inline && band2) {  // minimal: the tasks before band 2's last slice are fewer than wanted
      uint64_t before_last = 0;
      for (size_t ti = A.a_warm_tasks; ti < A.a_dep_tasks; ++ti)
        before_last += (slice_of(tasks[ti].y, seg.terms[tasks[ti].x].n_blocks) >> 1) < band2_last;
      if (before_last >= want2 && !getenv("TQ_AS_BAND2_ALL")) return fail_msg("band 2 is longer than the rule wants", mode, (long)band2);
    }
    printf("mode %d: %zu tasks, warm %llu, independent %llu, leaders with / without warm-up tasks %u / %u, bands [0, %u, %u, %zu) %s\n",
           mode, tasks.size(), (unsigned long long)n_warm, (unsigned long long)n_indep, leaders_with, leaders_without,
           A.a_warm_tasks, A.a_dep_tasks, tasks.size(), A.a_inline ? "one dispatch" : "two dispatches");
  }
  // option 0 == the ordering rule of before the option, over the same tasks: sort mode 2's tasks by it
  {
    std::vector<uint4> want = table[2];
    if (want.size() != table[0].size()) return fail_msg("the task count depends on the option");
    std::map<std::pair<uint32_t, uint32_t>, uint32_t> run_first;  // (leader, cache) -> its first lead
    for (const uint4 &t : want) {
      auto it = run_first.emplace(std::make_pair(t.x, t.z >> 24), t.w).first;
      it->second = std::min(it->second, t.w);
    }
    auto key = [&](const uint4 &t) {
      const uint32_t n_blocks = seg.terms[t.x].n_blocks;
      return t.y < nb_warm(t.x) ? 0u : 1u + slice_of(t.y, n_blocks);
    };
    std::sort(want.begin(), want.end(), [&](const uint4 &a, const uint4 &b) {
      const uint32_t ka = key(a), kb = key(b);
      if (ka != kb) return ka < kb;
      const uint32_t ra = run_first[{a.x, a.z >> 24}], rb = run_first[{b.x, b.z >> 24}];
      if (ra != rb) return ra < rb;
      if (a.y != b.y) return a.y < b.y;
      return a.w < b.w;
    });
    if (memcmp(want.data(), table[0].data(), want.size() * sizeof(uint4))) return fail_msg("option 0 is not the former order");
  }
  printf("order ok\n");
  return 0;
}
