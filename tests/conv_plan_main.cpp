// Stand-alone sweep of csrc/conv_plan.hpp (host-only arithmetic of the general
// convolution layer) for tests/test_cpu_conv_plan_sanitized.py, which builds it
// with AddressSanitizer and UBSan.  Every index the kernels derive from the plan
// is replayed here against real arrays of the planned size: the LDS staging
// maps, the stride-parity classes of the input gradient, and the partial-sum
// slabs of the weight gradient.
#include <stdio.h>
#include <stdlib.h>
#include <vector>

#include "../surreal_amd/csrc/conv_plan.hpp"

using namespace smi;

static long g_plans = 0;

#define CHECK(c)                                                                   \
  do {                                                                             \
    if (!(c)) {                                                                    \
      fprintf(stderr, "%s:%d: check failed: %s\n", __FILE__, __LINE__, #c);        \
      exit(1);                                                                     \
    }                                                                              \
  } while (0)

// the staging maps of conv_kernels.hip: 256 threads, 8 elements each, into a
// 64 x 32 slice with row stride kConvLd; each cell written exactly once
static void check_lds_maps() {
  const int cells = kConvTile * kConvLd;
  CHECK(conv_lds_bytes() == 2 * cells * 4);
  for (int map = 0; map < 3; ++map) {
    std::vector<int> lds(cells, 0);
    for (int tid = 0; tid < 256; ++tid)
      for (int j = 0; j < 8; ++j) {
        int idx;
        if (map == 0) idx = ((tid >> 5) + 8 * j) * kConvLd + (tid & 31);              // row block
        else if (map == 1) idx = ((tid >> 3) + 32 * (j >> 2)) * kConvLd + 4 * (tid & 7) + (j & 3);
        else idx = (tid & 63) * kConvLd + (tid >> 6) + 4 * j;                         // pixel rows
        lds.at(idx) += 1;
      }
    for (int r = 0; r < kConvTile; ++r)
      for (int z = 0; z < kConvLd; ++z) CHECK(lds[r * kConvLd + z] == (z < kConvChunk ? 1 : 0));
  }
  // MFMA operand reads of wave w, lane l
  std::vector<int> lds(cells, 0);
  for (int w = 0; w < 4; ++w)
    for (int l = 0; l < 64; ++l)
      for (int kk = 0; kk < kConvChunk / 4; ++kk)
        for (int half = 0; half < 2; ++half) {
          lds.at(((w >> 1) * 32 + (l & 15) + 16 * half) * kConvLd + (l >> 4) + kk * 4) += 1;
          lds.at(((w & 1) * 32 + (l & 15) + 16 * half) * kConvLd + (l >> 4) + kk * 4) += 1;
        }
}

static void check_geometry(int cin, int h, int w, int cout, int k, int s, int p, int64_t n) {
  if (!conv_geom_ok(cin, h, w, cout, k, s, p)) return;
  const ConvGeom g = conv_geom(cin, h, w, cout, k, s, p);
  ++g_plans;
  CHECK(g.ho >= 1 && g.wo >= 1 && g.K == cin * k * k && g.P == g.ho * g.wo);
  // the last window starts inside the padded image
  CHECK((g.ho - 1) * s + k <= h + 2 * p && (g.wo - 1) * s + k <= w + 2 * p);
  // ---- parity classes: every input row in exactly one class, at first + s j
  int taps = 0;
  std::vector<int> seen(h, 0);
  for (int r = 0; r < s; ++r) {
    const int f = conv_class_first(r, s, p), c = conv_class_count(h, r, s, p);
    CHECK(f >= 0 && f < s);
    for (int j = 0; j < c; ++j) {
      const int iy = f + s * j;
      CHECK((iy + p) % s == r);
      seen.at(iy) += 1;
      // tap a of the class reads output row (iy + p - r) / s - a: the forward's relation
      const int t = conv_class_taps(k, r, s);
      for (int a = 0; a < t; ++a) {
        const int ky = r + s * a, oy = (iy + p - r) / s - a;
        CHECK(ky < k);
        CHECK(oy * s + ky - p == iy);
      }
    }
    if (f + s * c < h) CHECK(false);
    taps += conv_class_taps(k, r, s);
  }
  for (int iy = 0; iy < h; ++iy) CHECK(seen[iy] == 1);
  CHECK(taps == k);                                       // every tap in exactly one class
  // ---- tiles
  CHECK(conv_fwd_tiles(g, n) * kConvTile * kConvTile >= n * g.P * (int64_t)cout || n == 0);
  int64_t q = 0;
  for (int ry = 0; ry < s; ++ry)
    for (int rx = 0; rx < s; ++rx) {
      q += (int64_t)conv_class_count(h, ry, s, p) * conv_class_count(w, rx, s, p);
      CHECK(conv_dx_class_tiles(g, n, ry, rx) <= conv_dx_max_tiles(g, n));
    }
  CHECK(q == (int64_t)h * w);
  // ---- weight gradient plan
  const ConvDwPlan pl = conv_dw_plan(g, n);
  CHECK(pl.slab == (int64_t)cout * g.K + cout);
  CHECK(conv_scratch_bytes(g, n) == 4 * pl.splits * pl.slab);
  if (n == 0) {
    CHECK(pl.splits == 0 && conv_scratch_bytes(g, n) == 0);
    return;
  }
  CHECK(pl.tiles * kConvTile * kConvTile >= cout * g.K);
  CHECK(pl.chunks * kConvChunk >= n * g.P && (pl.chunks - 1) * kConvChunk < n * g.P);
  CHECK(pl.splits >= 1 && pl.splits <= kConvMaxSplits && pl.per >= 1);
  CHECK(pl.per * pl.splits >= pl.chunks);                 // every chunk in a split
  CHECK(pl.per * (pl.splits - 1) < pl.chunks);            // no empty split
  // the partial-sum slabs: replay the epilogue's stores on a small plan
  if ((int64_t)pl.splits * pl.slab <= (1 << 12)) {
    std::vector<int> part((size_t)(conv_scratch_bytes(g, n) / 4), 0);
    const int rT = (cout + kConvTile - 1) / kConvTile;
    for (int sp = 0; sp < pl.splits; ++sp)
      for (int bx = 0; bx < pl.tiles; ++bx) {
        const int r0 = (bx % rT) * kConvTile, k0 = (bx / rT) * kConvTile;
        for (int r = 0; r < kConvTile; ++r)
          for (int c = 0; c < kConvTile; ++c)
            if (r0 + r < cout && k0 + c < g.K)
              part.at((size_t)sp * pl.slab + (size_t)(r0 + r) * g.K + k0 + c) += 1;
        if (k0 == 0)
          for (int r = 0; r < kConvTile; ++r)
            if (r0 + r < cout) part.at((size_t)sp * pl.slab + (size_t)cout * g.K + r0 + r) += 1;
      }
    for (size_t i = 0; i < part.size(); ++i) CHECK(part[i] == 1);
  }
}

int main() {
  check_lds_maps();
  // rejected arguments
  CHECK(!conv_geom_ok(1, 8, 8, 1, 9, 1, 0) && !conv_geom_ok(1, 8, 8, 1, 0, 1, 0));
  CHECK(!conv_geom_ok(1, 8, 8, 1, 8, 5, 0) && !conv_geom_ok(1, 8, 8, 1, 3, 4, 0));
  CHECK(!conv_geom_ok(1, 8, 8, 1, 3, 1, 3) && !conv_geom_ok(1, 8, 8, 1, 3, 1, -1));
  CHECK(!conv_geom_ok(129, 8, 8, 1, 3, 1, 1) && !conv_geom_ok(1, 8, 8, 129, 3, 1, 1));
  CHECK(!conv_geom_ok(0, 8, 8, 1, 3, 1, 1) && !conv_geom_ok(1, 8, 8, 0, 3, 1, 1));
  CHECK(!conv_geom_ok(1, 1, 1, 1, 8, 1, 0) && !conv_geom_ok(1, 0, 8, 1, 3, 1, 1));
  CHECK(!conv_geom_ok(1, 1 << 15, 8, 1, 3, 1, 1));
  const int hs[] = {1, 3, 8, 9, 20, 84};
  const int ws[] = {1, 7, 13};
  const int cs[] = {1, 3, 65, 128};
  const int64_t ns[] = {0, 1, 5, 100000};
  for (int k = 1; k <= 8; ++k)
    for (int s = 1; s <= 5; ++s)
      for (int p = 0; p <= k; ++p)
        for (int h : hs)
          for (int w : ws)
            for (int cin : cs)
              for (int cout : cs)
                for (int64_t n : ns) check_geometry(cin, h, w, cout, k, s, p, n);
  // the largest accepted layer at a large batch: no overflow in the byte count
  CHECK(!conv_geom_ok(128, 4096, 4096, 1, 3, 1, 1) && conv_geom_ok(128, 4000, 4000, 128, 8, 1, 7));
  const ConvGeom big = conv_geom(128, 4000, 4000, 128, 8, 1, 7);
  CHECK(conv_scratch_bytes(big, (int64_t)1 << 20) > 0);
  CHECK(conv_fwd_tiles(big, (int64_t)1 << 20) > 0);
  printf("plans made %ld\n", g_plans);
  return 0;
}
