// Stand-alone sweep of the grouped weight-gradient planner (csrc/dw_plan.hpp)
// for AddressSanitizer / UBSan runs: the planner writes fixed-size stack arrays
// whose bounds rest on an interplay of its limits (bands, entries, GEMMs), so
// test_cpu_dw_plan_sanitized.py builds this file with -fsanitize=address,
// undefined and runs it.  Every launch parameter takes every value of its list;
// the GEMM shapes are drawn per combination from a fixed-seed generator.
#include <cstdio>
#include <cstdlib>
#include "../surreal_amd/csrc/dw_plan.hpp"

using namespace smi;

// the lists of test_cpu_dw_plan.py, then the edges of the 16- and 64-wide tiles
// and of the grouped kernel's range
static const int MS[] = {1, 8, 16, 17, 64, 72, 90, 108, 128, 200, 300, 400, 15, 63, 65, 511, 512};
static const int NS[] = {16, 79, 91, 101, 128, 143, 201, 301, 1, 15, 17, 63, 64, 65, 511, 512};
static const int KS[] = {513, 1100, 21504, 1, 63, 64, 65};
static const int WAVES[] = {4, 8};
static const int SLOTS[] = {1, 32, 224, 768, 1536};
static const int64_t CAPS[] = {0, 1, 4096, (int64_t)1 << 26};
static const int TARGETS[] = {0, 1, 224};
constexpr int kDraws = 3;          // shape draws per combination (a few seconds under the sanitizers)

static uint32_t g_rng = 20240607u;
static uint32_t rnd(uint32_t n) {
  g_rng = g_rng * 1664525u + 1013904223u;
  return (g_rng >> 8) % n;
}
template <typename T, size_t L>
static T pick(const T (&a)[L]) { return a[rnd((uint32_t)L)]; }

#define REQUIRE(c)                                                                              \
  do {                                                                                          \
    if (!(c)) {                                                                                 \
      std::printf("FAILED %s: ng %d waves %d slots %d cap %lld max_ent %d target %d\n", #c, ng, \
                  wv, slots, (long long)cap, max_ent, target);                                  \
      for (int i_ = 0; i_ < ng; ++i_)                                                           \
        std::printf("  gemm %d: %d x %d x %d vec %d ones %d split %d\n", i_, g[i_].M, g[i_].N,  \
                    g[i_].K, g[i_].vec, g[i_].ones, g[i_].split_col);                           \
      return 1;                                                                                 \
    }                                                                                           \
  } while (0)

int main() {
  long made = 0, tried = 0;
  for (int ng = 1; ng <= kDwGemmMax; ++ng)
    for (int wv : WAVES)
      for (int slots : SLOTS)
        for (int max_ent = 1; max_ent <= 16; ++max_ent)
          for (int64_t cap : CAPS)
            for (int target : TARGETS)
              for (int d = 0; d < kDraws; ++d) {
                DwPlanGemm g[kDwGemmMax];
                for (int i = 0; i < ng; ++i) {
                  const int M = pick(MS), N = pick(NS);
                  g[i] = DwPlanGemm{M, N, pick(KS), (int)rnd(16), (int)rnd(2),
                                    rnd(2) ? -1 : (int)rnd((uint32_t)N)};
                  REQUIRE(dw_group_takes(M, N));
                }
                DwPlan P;
                const int rc = dw_plan(g, ng, wv, slots, cap, max_ent, target, P);
                ++tried;
                REQUIRE(rc == 0 || rc == -1);
                if (rc != 0) continue;
                ++made;
                REQUIRE(P.n >= 1 && P.n <= std::min(max_ent, kDwSplitMax));
                REQUIRE(P.wg0[0] == 0 && P.rb0[0] == 0);
                for (int i = 0; i < P.n; ++i) {
                  REQUIRE(P.e[i].gi >= 0 && P.e[i].gi < ng);
                  REQUIRE(P.wg0[i + 1] >= P.wg0[i] && P.rb0[i + 1] >= P.rb0[i]);
                }
                REQUIRE(P.need <= cap);
              }
  std::printf("%ld plans made of %ld tried\n", made, tried);
  return 0;
}
