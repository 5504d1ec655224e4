// CPU sanitizer program for the host side of g3_gp_append / g3_gp_cross_append (g3py_amd/csrc/g3_host.h): the plan
// g3h_append_plan -- n0, Np1, r and every offset the entry points add to a pointer -- walked over model buffers of exactly the
// size the header asks for, the argument check g3h_args_append and the capacity rule g3h_append_capacity.  Built with
// g++ -fsanitize=address,undefined by tests/test_append_host.py; no GPU, no HIP.
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
  // ---- the cases of tests/test_gpu_append.py and a few around them
  const int64_t cases[][2] = {{1, 1},   {100, 20}, {100, 28},  {100, 29},   {128, 1}, {128, 128}, {300, 1},
                              {300, 300}, {256, 3200}, {4224, 5}, {127, 1}, {129, 127}, {120, 30}};
  for (const auto& c : cases) {
    const int64_t N0 = c[0], N1 = c[0] + c[1];
    CHECK(g3h_args_append(N0, N1, 4) == 0);
    for (const int64_t slack : {(int64_t)0, (int64_t)128, (int64_t)640}) {
      const int64_t ld = g3h_roundup(N1, 128) + slack;
      const G3hAppendPlan p = g3h_append_plan(N0, N1, ld);
      CHECK(p.n0 % 128 == 0 && p.n0 <= N0 && N0 - p.n0 < 128);
      CHECK(p.Np1 % 128 == 0 && p.Np1 >= N1 && p.Np1 - N1 < 128);
      CHECK(p.r == p.Np1 - p.n0 && p.r >= 128 && p.r % 128 == 0);
      CHECK(p.k_rows == p.Np1 + 128 && p.w_blocks * 128 == p.Np1 && p.w_first * 128 == p.n0);
      // the tall buffer as the header sizes it: every element the call may touch lies inside, none of a row below n0
      std::vector<unsigned char> K((size_t)p.k_rows * ld, 0);
      for (int64_t i = 0; i < p.r; ++i)                                // the new block row, columns [0, Np1)
        for (int64_t j = 0; j < p.Np1; ++j) K[(size_t)(p.rows_off + i * ld + j)] |= 1;
      for (int64_t i = 0; i < p.r + 128; ++i)                          // the corner with the right-hand-side rows below it
        for (int64_t j = 0; j < p.r; ++j) K[(size_t)(p.corner_off + i * ld + j)] |= 2;
      for (int64_t i = 0; i < 128; ++i)                                // the right-hand-side block
        for (int64_t j = 0; j < p.Np1; ++j) K[(size_t)(p.rhs_off + i * ld + j)] |= 4;
      for (int64_t i = 0; i < p.n0; ++i)
        for (int64_t j = 0; j < ld; ++j) CHECK(K[(size_t)(i * ld + j)] == 0);
      CHECK(p.corner_off == p.n0 * ld + p.n0 && p.rhs_off == p.Np1 * ld);
      CHECK((K[(size_t)p.corner_off] & 3) == 3 && (K[(size_t)(p.rhs_off + p.n0)] & 6) == 6);
      // the block inverses: blocks [w_first, w_blocks) of 128 x 128
      std::vector<unsigned char> W((size_t)p.w_blocks * 128 * 128, 0);
      for (int64_t b = 0; b < p.r / 128; ++b) W[(size_t)(p.w_off + b * 128 * 128 + 128 * 128 - 1)] = 1;
      CHECK(p.w_off == p.n0 * 128 && W.back() == 1);
    }
  }
  // ---- refusals: N0 at `at`, N1 at at + 1
  CHECK(g3h_args_append(0, 5, 4) == -4);
  CHECK(g3h_args_append(-3, 5, 4) == -4);
  CHECK(g3h_args_append(5, 5, 4) == -5);
  CHECK(g3h_args_append(5, 4, 7) == -8);
  // ---- capacity: never below the need, a multiple of 128, unchanged while it fits, else at least 1.5 x
  for (int64_t have = 128; have <= 40000; have += 128 * 7)
    for (int64_t need = 1; need <= have + 4000; need += 97) {
      const int64_t cap = g3h_append_capacity(have, need);
      CHECK(cap >= need && cap >= have);
      if (need <= have) CHECK(cap == have);
      else CHECK(cap % 128 == 0 && 2 * cap >= 3 * have);
    }
  {
    // forty one-row appends from N = 100: the 128-row buffer grows once
    int64_t cap = 128, grown = 0;
    for (int64_t n = 101; n <= 140; ++n) {
      const int64_t next = g3h_append_capacity(cap, g3h_roundup(n, 128));
      grown += next != cap;
      cap = next;
    }
    CHECK(grown == 1 && cap == 256);
    // and one-row appends up to 32768 rows: O(log) of them
    cap = 128, grown = 0;
    for (int64_t n = 129; n <= 32768; n += 128) {
      const int64_t next = g3h_append_capacity(cap, n);
      grown += next != cap;
      cap = next;
    }
    CHECK(grown <= 15);
  }
  printf("append_plan ok\n");
  return 0;
}
