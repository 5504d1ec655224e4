// CPU sanitizer program for the host side of g3_gp_cv (g3py_amd/csrc/g3_host.h): the fold validation g3h_args_folds, whose
// refusals are the entry point's (arguments 13 idx, 14 ptr, 15 nfold), and the launch groups g3h_fold_groups.  Built with
// g++ -fsanitize=address,undefined by tests/test_cv_host.py; no GPU, no HIP.
#include <stdio.h>

#include <vector>

#include "g3_host.h"

#define CHECK(c)                                                        \
  do {                                                                  \
    if (!(c)) {                                                         \
      printf("FAILED %s:%d %s\n", __FILE__, __LINE__, #c);              \
      return 1;                                                         \
    }                                                                   \
  } while (0)

int main() {
  const int64_t N = 300;
  // ---- one valid input of three folds: out of order inside a fold, one fold empty, not covering
  {
    const std::vector<int32_t> idx = {7, 3, 299, 0, 150, 151};
    const std::vector<int64_t> ptr = {0, 3, 3, 6};
    CHECK(g3h_args_folds(idx.data(), ptr.data(), 3, N, 13) == 0);
  }
  // ---- the refusals of tests/test_gpu_fold_cv.py::test_argument_checks
  std::vector<int32_t> idx(300);
  for (int i = 0; i < 300; ++i) idx[i] = i;
  const std::vector<int64_t> ptr = {0, 75, 150, 225, 300};
  CHECK(g3h_args_folds(idx.data(), ptr.data(), 4, N, 13) == 0);
  {
    std::vector<int32_t> bad = idx;
    bad[200] = 10;                                     // overlapping folds
    CHECK(g3h_args_folds(bad.data(), ptr.data(), 4, N, 13) == -13);
    bad = idx;
    bad[299] = (int32_t)N;                             // an index equal to N
    CHECK(g3h_args_folds(bad.data(), ptr.data(), 4, N, 13) == -13);
    bad[299] = -1;
    CHECK(g3h_args_folds(bad.data(), ptr.data(), 4, N, 13) == -13);
    bad[299] = 0x7fffffff;
    CHECK(g3h_args_folds(bad.data(), ptr.data(), 4, N, 13) == -13);
  }
  {
    const std::vector<int64_t> down = {0, 150, 75, 225, 300};   // a decreasing pointer
    CHECK(g3h_args_folds(idx.data(), down.data(), 4, N, 13) == -14);
    const std::vector<int64_t> late = {1, 75, 150, 225, 300};   // ptr[0] != 0
    CHECK(g3h_args_folds(idx.data(), late.data(), 4, N, 13) == -14);
    CHECK(g3h_args_folds(idx.data(), nullptr, 4, N, 13) == -14);
  }
  CHECK(g3h_args_folds(idx.data(), ptr.data(), 0, N, 13) == -15);
  CHECK(g3h_args_folds(idx.data(), ptr.data(), G3_MAX_BATCH + 1, N, 13) == -15);     // refused before any pointer is read
  CHECK(g3h_args_folds(idx.data(), ptr.data(), -1, N, 13) == -15);
  CHECK(g3h_args_folds(nullptr, ptr.data(), 4, N, 13) == -13);
  {
    // more indices than observations: some index is there twice, found without reading past the N marks
    std::vector<int32_t> many(2 * 300);
    for (int i = 0; i < 600; ++i) many[i] = i % 300;
    const std::vector<int64_t> p2 = {0, 600};
    CHECK(g3h_args_folds(many.data(), p2.data(), 1, N, 13) == -13);
    const std::vector<int64_t> none = {0, 0, 0};        // folds that hold nothing need no index list
    CHECK(g3h_args_folds(nullptr, none.data(), 2, N, 13) == 0);
  }
  // ---- the most folds there can be, every one a single point
  {
    std::vector<int32_t> all(G3_MAX_BATCH);
    std::vector<int64_t> p(G3_MAX_BATCH + 1);
    for (int i = 0; i < G3_MAX_BATCH; ++i) all[i] = G3_MAX_BATCH - 1 - i;
    for (int i = 0; i <= G3_MAX_BATCH; ++i) p[i] = i;
    CHECK(g3h_args_folds(all.data(), p.data(), G3_MAX_BATCH, G3_MAX_BATCH, 13) == 0);
  }
  // ---- launch groups: every fold in exactly one group, in order; a group's Sp covers its largest fold; a group of more than
  //      one fold fits the cap
  {
    auto per = [](int64_t sp) { return (size_t)((sp + 128) * sp + sp * 128 + 3 * sp) * 8; };
    const std::vector<std::vector<int64_t>> cases = {
        {0, 75, 150, 225, 300}, {0, 1, 51, 180, 300}, {0, 257, 600}, {0, 300}, {0, 0, 0}, {0, 5000, 5001, 9000, 9100, 9100, 20000}};
    const size_t caps[3] = {(size_t)256 << 20, (size_t)1 << 20, (size_t)1};
    for (const auto& p : cases)
      for (const size_t cap : caps) {
        const int nfold = (int)p.size() - 1;
        std::vector<int> first;
        std::vector<int64_t> sp;
        g3h_fold_groups(p.data(), nfold, cap, per, &first, &sp);
        CHECK(first.size() == sp.size() + 1 && first.front() == 0 && first.back() == nfold);
        for (size_t g = 0; g < sp.size(); ++g) {
          CHECK(first[g + 1] > first[g] && sp[g] >= 128 && sp[g] % 128 == 0);
          int64_t largest = 0;
          for (int f = first[g]; f < first[g + 1]; ++f) largest = p[f + 1] - p[f] > largest ? p[f + 1] - p[f] : largest;
          CHECK(sp[g] == g3h_roundup(largest > 128 ? largest : 128, 128));
          if (first[g + 1] - first[g] > 1) CHECK((size_t)(first[g + 1] - first[g]) * per(sp[g]) <= cap);
        }
        if (cap == 1) CHECK((int)sp.size() == nfold);          // nothing fits: every fold on its own
      }
    std::vector<int> first;
    std::vector<int64_t> sp;
    g3h_fold_groups(cases[1].data(), 4, caps[0], per, &first, &sp);
    CHECK(sp.size() == 1 && sp[0] == 256);                     // 1, 50, 129, 120: one group of 256 padded rows
  }
  printf("cv_folds ok\n");
  return 0;
}
