// Stand-alone sweep of csrc/stem_plan.hpp (host-only arithmetic of the pixel
// stem of free shape) for tests/test_cpu_stem_plan_sanitized.py, which builds
// it with AddressSanitizer and UBSan.  Specs of 1 to 4 layers with k, stride
// and channels at their range ends, frames from 1 x 8 x 8 over odd sizes to
// 256 x 256, and row counts: the parameter, activation and scratch regions are
// painted into arrays of the planned size (each float owned exactly once: no
// overlap, no gap), the default spec reproduces cnn_geom's offsets, the
// time-major row map stays inside pix / pix_next, and stem_fused_ok equals the
// fused kernels' conditions restated here.
#include <stdio.h>
#include <stdlib.h>
#include <vector>

#include "../surreal_amd/csrc/stem_plan.hpp"

using namespace smi;

static long g_plans = 0, g_fused = 0, g_refused = 0;

#define CHECK(c)                                                                   \
  do {                                                                             \
    if (!(c)) {                                                                    \
      fprintf(stderr, "%s:%d: check failed: %s\n", __FILE__, __LINE__, #c);        \
      exit(1);                                                                     \
    }                                                                              \
  } while (0)

static void paint(std::vector<unsigned char>& a, int64_t off, int64_t n) {
  CHECK(off >= 0 && n >= 0 && off + n <= (int64_t)a.size());
  for (int64_t i = 0; i < n; ++i) a.at(off + i) += 1;
}
static void all_once(const std::vector<unsigned char>& a) {
  for (size_t i = 0; i < a.size(); ++i) CHECK(a[i] == 1);
}

// the fused kernels' acceptance (cnn_check and the two LDS limits of
// cnn_kernels.hip), restated from the frame arithmetic
static bool fused_expected(const StemSpec& s, int C, int H, int W) {
  if (s.n != 2 || s.cout[0] != 16 || s.cout[1] != 32 || s.k[0] != 8 || s.k[1] != 4 ||
      s.stride[0] != 4 || s.stride[1] != 2)
    return false;
  if (C != 3 && C != 9) return false;
  if (H < 8 || W < 8) return false;
  const int64_t H1 = (H - 8) / 4 + 1, W1 = (W - 8) / 4 + 1;
  if (H1 < 4 || W1 < 4) return false;
  const int64_t H2 = (H1 - 4) / 2 + 1, W2 = (W1 - 4) / 2 + 1, P1 = H1 * W1, P2 = H2 * W2;
  const int64_t img = (int64_t)C * H * W;
  if ((P2 + 15) / 16 > 6) return false;
  if (W % 4 || img % 16 || P1 % 4 || W1 % 2) return false;
  if (s.F < 1) return false;
  const int64_t fwd = (img + 15) / 16 * 16 + 64 * P1;
  const int64_t bwd = fwd + 4 * 32 * P2 + 4 * 256 + 4 * (P1 + P2);
  return fwd <= 160 * 1024 && bwd <= 160 * 1024;
}

static void check_plan(const StemSpec& s, int C, int H, int W, int64_t rows) {
  const int bad = stem_check(s, C, H, W);
  if (bad) {
    ++g_refused;
    CHECK(bad == -1 || (bad >= 1 && bad <= s.n));
    CHECK(!fused_expected(s, C, H, W));
    return;
  }
  const StemPlan p = stem_plan(s, C, H, W);
  ++g_plans;
  CHECK(p.n == s.n && p.F == s.F && p.img == (int64_t)C * H * W);
  // geometry: each layer reads the previous layer's output, the last window inside the frame
  int c = C, h = H, w = W;
  int64_t row = 0;
  for (int i = 0; i < p.n; ++i) {
    const ConvGeom& g = p.g[i];
    CHECK(g.cin == c && g.h == h && g.w == w && g.cout == s.cout[i] && g.k == s.k[i] &&
          g.s == s.stride[i] && g.p == 0);
    CHECK(g.ho == (h - g.k) / g.s + 1 && g.wo == (w - g.k) / g.s + 1 && g.ho >= 1 && g.wo >= 1);
    CHECK((g.ho - 1) * g.s + g.k <= h && (g.wo - 1) * g.s + g.k <= w);
    CHECK(p.act[i] == (int64_t)g.cout * g.ho * g.wo);
    row += p.act[i];
    c = g.cout; h = g.ho; w = g.wo;
  }
  CHECK(p.act_row == row && p.flat == p.act[p.n - 1]);
  // parameters: module order, no overlap, no gap
  int64_t o = 0;
  for (int i = 0; i < p.n; ++i) {
    CHECK(p.oW[i] == o);
    o += (int64_t)p.g[i].cout * p.g[i].cin * p.g[i].k * p.g[i].k;
    CHECK(p.ob[i] == o);
    o += p.g[i].cout;
  }
  CHECK(p.oWf == o && p.nconv == o);
  o += (int64_t)p.F * p.flat;
  CHECK(p.obf == o && p.total == o + p.F);
  if (p.total <= (1 << 19)) {
    std::vector<unsigned char> prm((size_t)p.total, 0);
    for (int i = 0; i < p.n; ++i) {
      paint(prm, p.oW[i], (int64_t)p.g[i].cout * p.g[i].K);
      paint(prm, p.ob[i], p.g[i].cout);
    }
    paint(prm, p.oWf, (int64_t)p.F * p.flat);
    paint(prm, p.obf, p.F);
    all_once(prm);
  }
  // the default spec is cnn_geom's layout
  if (stem_is_default(s)) {
    const CnnGeom g = cnn_geom(C, H, W, s.F);
    CHECK(p.oW[0] == g.oW1 && p.ob[0] == g.ob1 && p.oW[1] == g.oW2 && p.ob[1] == g.ob2 &&
          p.oWf == g.oWf && p.obf == g.obf && p.total == g.total && p.nconv == g.nconv);
    CHECK(p.flat == g.flat && p.act[0] == 16 * (int64_t)g.P1 && p.img == g.img);
  }
  // dispatch
  CHECK(p.fused == stem_fused_ok(s, C, H, W));
  CHECK(p.fused == fused_expected(s, C, H, W));
  g_fused += p.fused;
  // activations: the layers one behind the other
  const int64_t na = stem_act_floats(p, rows);
  CHECK(na == rows * row);
  const bool small = na <= (1 << 19);
  if (small) {
    std::vector<unsigned char> act((size_t)na, 0);
    for (int i = 0; i < p.n; ++i) paint(act, stem_act_off(p, rows, i), rows * p.act[i]);
    all_once(act);
  }
  // backward scratch: dA_n first ... then the partials
  const StemScratch sc = stem_scratch(p, rows);
  CHECK(sc.part_floats == stem_part_floats(p, rows));
  CHECK(sc.total == sc.part + sc.part_floats);
  CHECK(stem_scratch_bytes(p, rows) >= 4 * sc.total);
  CHECK(stem_scratch_bytes(p, rows) >= 4 * stem_fwd_scratch_floats(p, rows));
  CHECK(stem_scratch_bytes(p, rows) % 4 == 0);
  if (p.fused) {
    // the carve of smi_cnn_backward: [dA2 | cnn_bwd_grid(rows) slabs]
    CHECK(sc.dA[0] == -1 && sc.dA[1] == 0 && sc.part == rows * p.flat);
    CHECK(sc.part_floats == (int64_t)cnn_bwd_grid(rows) * p.nconv);
    CHECK(stem_fwd_scratch_floats(p, rows) == rows * p.flat);
  } else {
    int64_t need = 0;
    for (int i = 0; i < p.n; ++i) {
      CHECK(sc.dA[i] >= 0);
      const int64_t b = conv_scratch_bytes(p.g[i], rows);
      CHECK(b % 4 == 0);
      need = b / 4 > need ? b / 4 : need;
    }
    CHECK(sc.part_floats == need);
    CHECK(sc.dA[p.n - 1] == 0);
    CHECK(stem_fwd_scratch_floats(p, rows) == na);
  }
  for (int i = p.n; i < kStemMaxLayers; ++i) CHECK(sc.dA[i] == -1);
  if (sc.total <= (1 << 19)) {
    std::vector<unsigned char> scr((size_t)sc.total, 0);
    for (int i = 0; i < p.n; ++i)
      if (sc.dA[i] >= 0) paint(scr, sc.dA[i], rows * p.act[i]);
    paint(scr, sc.part, sc.part_floats);
    all_once(scr);
    // every layer's partial slabs fit the shared region
    if (!p.fused)
      for (int i = 0; i < p.n; ++i) {
        const ConvDwPlan q = conv_dw_plan(p.g[i], rows);
        CHECK((int64_t)q.splits * q.slab <= sc.part_floats);
      }
  }
}

// row n = t B + b reads pix[b][t] (t < T) or pix_next[b]: inside the buffers
static void check_row_map(int64_t B, int64_t T, int64_t rows, int64_t img) {
  std::vector<unsigned char> pix((size_t)(B * T * img), 0), nxt((size_t)(B * img), 0);
  for (int64_t n = 0; n < rows; ++n) {
    const int64_t t = n / B, b = n - t * B;
    CHECK(t <= T);
    if (t < T) paint(pix, (b * T + t) * img, img);
    else paint(nxt, b * img, img);
  }
  int64_t seen = 0;
  for (unsigned char v : pix) { CHECK(v <= 1); seen += v; }
  for (unsigned char v : nxt) { CHECK(v <= 1); seen += v; }
  CHECK(seen == rows * img);
}

int main() {
  const int ks[] = {1, 2, 3, 4, 5, 8, 9}, ss[] = {0, 1, 2, 3, 4, 5}, cs[] = {0, 1, 4, 16, 72, 128, 129};
  const int frames[][3] = {{1, 8, 8}, {1, 21, 23}, {2, 9, 11}, {3, 12, 12}, {3, 20, 20}, {3, 30, 26},
                           {3, 32, 22}, {3, 36, 52}, {3, 84, 84}, {3, 84, 100}, {3, 96, 96},
                           {4, 20, 20}, {5, 19, 16}, {6, 84, 84}, {9, 84, 84}, {9, 40, 212},
                           {3, 128, 128}, {3, 256, 256}, {9, 20, 668}, {9, 20, 780}, {3, 7, 84},
                           {128, 33, 17}, {129, 20, 20}, {3, 16385, 8}};
  const int64_t rowss[] = {0, 1, 3, 7, 9, 512, 513, 2688};
  for (const auto& f : frames) {
    // the default spec and its neighbours
    for (int F : {0, 1, 8, 200})
      for (int64_t rows : rowss) check_plan(stem_spec_default(F), f[0], f[1], f[2], rows);
    // one layer over the range ends
    for (int k : ks)
      for (int s : ss)
        for (int c : cs) {
          const int co[4] = {c, 0, 0, 0}, kk[4] = {k, 0, 0, 0}, st[4] = {s, 0, 0, 0};
          for (int64_t rows : {1, 5, 600}) check_plan(stem_spec(1, co, kk, st, 8), f[0], f[1], f[2], rows);
        }
    // two to four layers: shrinking windows, mixed strides
    const int co[4] = {8, 12, 20, 4}, kk[4] = {5, 3, 2, 1}, st[4] = {2, 1, 2, 1};
    const int co2[4] = {4, 4, 4, 4}, kk2[4] = {2, 2, 2, 2}, st2[4] = {1, 1, 1, 1};
    const int co3[4] = {128, 1, 128, 7}, kk3[4] = {8, 4, 3, 3}, st3[4] = {4, 3, 1, 2};
    for (int n = 0; n <= 5; ++n)
      for (int64_t rows : {2, 8, 515}) {
        check_plan(stem_spec(n, co, kk, st, 16), f[0], f[1], f[2], rows);
        check_plan(stem_spec(n, co2, kk2, st2, 8), f[0], f[1], f[2], rows);
        check_plan(stem_spec(n, co3, kk3, st3, 3), f[0], f[1], f[2], rows);
      }
  }
  // stem_check names the layer
  {
    const int co[4] = {8, 12, 20, 4}, kk[4] = {5, 3, 9, 1}, st[4] = {2, 1, 2, 1};
    CHECK(stem_check(stem_spec(3, co, kk, st, 16), 3, 30, 26) == 3);
    CHECK(stem_check(stem_spec(2, co, kk, st, 16), 3, 30, 26) == 0);
    CHECK(stem_check(stem_spec(2, co, kk, st, 16), 3, 4, 26) == 1);
    CHECK(stem_check(stem_spec(2, co, kk, st, 16), 3, 6, 26) == 2);      // 1 x 11 into k = 3
    CHECK(stem_check(stem_spec(0, co, kk, st, 16), 3, 30, 26) == -1);
    CHECK(stem_check(stem_spec(5, co, kk, st, 16), 3, 30, 26) == -1);
    CHECK(stem_check(stem_spec(2, co, kk, st, 0), 3, 30, 26) == -1);
    CHECK(stem_check(stem_spec(1, nullptr, nullptr, nullptr, 4), 3, 30, 26) == 1);
  }
  for (int64_t B : {1, 2, 5})
    for (int64_t T : {1, 2, 3})
      for (int64_t rows = 0; rows <= B * (T + 1); ++rows) check_row_map(B, T, rows, 37);
  CHECK(g_plans > 1000 && g_fused > 10 && g_refused > 1000);
  printf("%ld plans made, %ld fused, %ld specs refused\n", g_plans, g_fused, g_refused);
  return 0;
}
