// Stand-alone sweep of the fused head chains' launch planner (head_plan,
// csrc/smi_shapes.hpp: host-only arithmetic, no device or runtime call) for
// AddressSanitizer / UBSan runs: test_cpu_head_plan.py builds this file with
// -fsanitize=address,undefined and runs it.  Rows 1 .. 70,000 (the row-tile
// threshold, the grid) and every width 4 .. 512 of the three layers on both
// sides of the threshold; the expected values are restated here from the
// kernels' layout, not taken from the planner.
#include <cstdio>
#include <cstdlib>
#include "../surreal_amd/csrc/smi_shapes.hpp"

using namespace smi;

static int imax(int a, int b) { return a > b ? a : b; }
static int ld16(int k) { return (k + 15) / 16 * 16 + 4; }
static int wgs(int bytes) { const int n = 163840 / bytes; return n < 8 ? n : 8; }

#define REQUIRE(c)                                                                           \
  do {                                                                                       \
    if (!(c)) {                                                                              \
      std::printf("FAILED %s: rows %lld in %d h1 %d h2 %d dxn %d\n", #c, (long long)rows,    \
                  in, h1, h2, dxn);                                                          \
      return 1;                                                                              \
    }                                                                                        \
  } while (0)

static int check(int64_t rows, int in, int h1, int h2, int dxn, long* shared) {
  const HeadPlan p = head_plan(rows, in, h1, h2, dxn);
  const int rt = rows >= 16384 ? 2 : 1, R = 16 * rt;
  REQUIRE(hc_rt(rows) == rt && p.rt == rt);
  REQUIRE(head_bwd_blocks(rows) == (int)((rows + R - 1) / R) && p.grid == head_bwd_blocks(rows));
  const int l0 = ld16(in), l1 = ld16(h1), l2 = ld16(h2);
  REQUIRE(p.ld0 == l0 && p.ld1 == l1 && p.ld2 == l2);
  const int sr = imax(rt * 1024, 32 * 33 + 32);
  // the separate carve (every tile beside its successor) and the shared one
  const int fsep = (R * (imax(l0, l2) + l1) + sr) * 4, fsh = (R * imax(imax(l0, l1), l2) + sr) * 4;
  const int bsep = (R * (l2 + l1) + R * 16) * 4;
  REQUIRE(p.fwd_lds == (p.fwd_shared ? fsh : fsep));
  REQUIRE(p.bwd_lds == bsep);     // (the backward keeps its tiles apart)
  // the flag only where it raises the workgroups per CU, never at one row tile
  REQUIRE(p.fwd_shared == (rt == 2 && wgs(fsh) > wgs(fsep)));
  REQUIRE(p.fwd_wgs >= 1 && p.fwd_wgs <= 8 && (int64_t)p.fwd_lds * p.fwd_wgs <= 163840);
  REQUIRE(p.bwd_wgs >= 1 && p.bwd_wgs <= 8 && (int64_t)(p.bwd_lds + HC_PG_LDS) * p.bwd_wgs <= 163840);
  REQUIRE(p.fwd_wgs == wgs(p.fwd_lds) && p.bwd_wgs == wgs(p.bwd_lds + HC_PG_LDS));
  // the tiles fit the carve and do not overlap unless they take turns
  REQUIRE(p.fwd_oR * 4 + sr * 4 == p.fwd_lds);
  REQUIRE(R * l0 <= p.fwd_oR && R * l2 <= p.fwd_oR && p.fwd_o1 + R * l1 <= p.fwd_oR);
  REQUIRE(p.fwd_shared ? p.fwd_o1 == 0 : p.fwd_o1 >= R * imax(l0, l2));
  REQUIRE(p.fwd_o1 % 4 == 0 && p.fwd_oR % 4 == 0);
  // the forms cover the layers: 4 waves x n tiles x 16 columns
  REQUIRE(64 * p.fwd_n1 >= h1 && 64 * p.fwd_n2 >= h2 && 64 * p.bwd_na >= h1 && 64 * p.bwd_nb >= dxn);
  REQUIRE(p.fwd_n1 == 2 || p.fwd_n1 == 5 || p.fwd_n1 == 8);
  REQUIRE(p.fwd_n2 == 2 || p.fwd_n2 == 3 || p.fwd_n2 == 4 || p.fwd_n2 == 5 || p.fwd_n2 == 8);
  REQUIRE(p.bwd_na == p.fwd_n1 && (p.bwd_nb == 2 || p.bwd_nb == 5));
  *shared += p.fwd_shared;
  return 0;
}

int main() {
  long made = 0, shared = 0;
  for (int64_t rows = 1; rows <= 70000; ++rows, ++made)
    if (check(rows, 100, 300, 200, 100, &shared)) return 1;
  static const int64_t ROWS[] = {16383, 16384};
  for (int64_t rows : ROWS)
    for (int in = 4; in <= 512; in += 4)
      for (int h1 = 4; h1 <= 512; h1 += 4)
        for (int h2 = 4; h2 <= 512; h2 += 4, ++made)
          // (dX spans at most 320 columns: the chains' input limit, head_fused_ok)
          if (check(rows, in, h1, h2, (h1 + h2) % 3 == 0 ? 0 : in <= 320 ? in : 320, &shared)) return 1;
  {   // the headline shape: the forward three workgroups per CU, one resident
      // round; the backward, kept on its separate carve, two
    const int64_t rows = 21504;
    const int in = 100, h1 = 300, h2 = 200, dxn = 100;
    const HeadPlan p = head_plan(rows, in, h1, h2, dxn);
    REQUIRE(p.rt == 2 && p.grid == 672 && p.fwd_shared);
    REQUIRE(p.fwd_lds == 47616 && p.bwd_lds == 68608);
    REQUIRE(p.fwd_wgs == 3 && p.bwd_wgs == 2 && p.grid <= 256 * 3);
    REQUIRE(p.fwd_n1 == 5 && p.fwd_n2 == 4 && p.bwd_na == 5 && p.bwd_nb == 2);
  }
  {   // a rank's share keeps the one-row-tile carve
    const int64_t rows = 2688;
    const int in = 100, h1 = 300, h2 = 200, dxn = 100;
    const HeadPlan p = head_plan(rows, in, h1, h2, dxn);
    REQUIRE(p.rt == 1 && !p.fwd_shared && p.fwd_lds == (16 * (212 + 308) + 1088) * 4);
  }
  std::printf("plans made: %ld (shared carves: %ld)\n", made, shared);
  return 0;
}
