// Stand-alone sweep of the LSTM learner's shapes and scratch carve
// (surreal_amd/csrc/rnn_layout.hpp: plain C++, no device or runtime call), for
// tests/test_cpu_rnn_layout_sanitized.py: built with AddressSanitizer and
// UBSan and run as a child process.  For every shape smi_ppo_rnn_phase accepts
// it checks the carve with a null base (sizes only) and with a base address
// (never dereferenced): order, alignment, no overlap, and that each region
// holds every use ppo_rnn.hip makes of it.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include "../surreal_amd/csrc/rnn_layout.hpp"

using namespace smi;

static long long g_checks = 0;
#define CHECK(cond, ...)                                              \
  do {                                                                \
    ++g_checks;                                                       \
    if (!(cond)) {                                                    \
      std::printf("FAILED %s:%d: %s\n  ", __FILE__, __LINE__, #cond); \
      std::printf(__VA_ARGS__);                                       \
      std::printf("\n");                                              \
      std::exit(1);                                                   \
    }                                                                 \
  } while (0)

struct Region { const char* name; const void* p; int64_t need; };   // need: floats

static int64_t imax(int64_t a, int64_t b) { return a > b ? a : b; }

// the regions in carve order with the floats their uses in ppo_rnn.hip need
static int regions(const RnnDims& d, const RnnScratch& s, Region* r) {
  const int64_t hm1 = imax(d.h1, d.c1), hm2 = imax(d.h2, d.c2), A1 = imax(d.A, 1);
  const int64_t BH = (int64_t)d.B * d.H;
  const bool px = d.F > 0;
  // s.part (doubles): the policy statistics' [<= 4096][8] partials, the value
  // rows' [<= 4096][5] or the head forward's five per workgroup, ZSTATS's
  // [256][2][D], the Adam norm's <= 1024
  int64_t part = imax(65536, 5 * (int64_t)head_bwd_blocks(d.NE));
  part = imax(part, (int64_t)256 * 2 * d.D);
  part = imax(part, (int64_t)4096 * 8);
  int n = 0;
  r[n++] = {"Xz", s.Xz, d.NG * d.ldx};
  r[n++] = {"Xr", s.Xr, d.NE * d.ldx};
  r[n++] = {"xproj", s.xproj, d.NG * d.G4};                        // a layer's S1 steps (GAE)
  r[n++] = {"hbuf", s.hbuf, d.L * (d.S1 + 1) * BH};
  r[n++] = {"cbuf", s.cbuf, d.L * (d.E + 1) * BH};
  r[n++] = {"gates", s.gates, d.L * d.NE * d.G4};
  r[n++] = {"HA1", s.HA1, imax(d.NG * d.c1, d.NE * hm1)};          // GAE critic over NG rows
  r[n++] = {"HA2", s.HA2, imax(d.NG * d.c2, d.NE * hm2)};
  r[n++] = {"OUT", s.OUT, imax(d.NG, d.NE * A1)};
  r[n++] = {"dOUT", s.dOUT, d.NE * A1};
  r[n++] = {"dH1", s.dH1, d.NE * hm1};
  r[n++] = {"dH2", s.dH2, d.NE * hm2};
  r[n++] = {"dh", s.dh, d.NE * d.H};
  r[n++] = {"dgates", s.dgates, d.L * d.NE * d.G4};
  r[n++] = {"values", s.values, (int64_t)d.B * d.S1};
  r[n++] = {"adv", s.adv, d.NE};
  r[n++] = {"ret", s.ret, d.NE};
  r[n++] = {"refmu", s.refmu, d.NE * d.A};
  r[n++] = {"rowin", s.rowin, ((d.NE + 63) / 64 * 64) * row_w(d.A)};
  r[n++] = {"ret_tm", s.ret_tm, d.NE};
  r[n++] = {"lvpart", s.lvpart, (int64_t)4096 * d.A};
  r[n++] = {"A1", s.A1, px ? d.NE * 16 * d.G.P1 : 0};
  r[n++] = {"A2", s.A2, px ? d.NG * d.G.flat : 0};
  r[n++] = {"xprojR", s.xprojR, d.NE * d.G4};
  r[n++] = {"hbufR", s.hbufR, d.L * (d.S1 + 1) * BH};              // hbuf_of's stride, E steps used
  r[n++] = {"HA1R", s.HA1R, d.NE * d.h1};
  r[n++] = {"HA2R", s.HA2R, d.NE * d.h2};
  r[n++] = {"A2R", s.A2R, px ? d.NE * d.G.flat : 0};
  r[n++] = {"wT", s.wT, imax((int64_t)d.Hin * d.h1 + (int64_t)d.h1 * d.h2,
                             (int64_t)d.Hin * d.c1 + (int64_t)d.c1 * d.c2)};
  r[n++] = {"dA2", s.dA2, px ? d.NE * d.G.flat : 0};
  r[n++] = {"dF", s.dF, px ? d.NE * d.F : 0};
  r[n++] = {"cpart", s.cpart, px ? (int64_t)cnn_bwd_grid(d.NE) * d.G.nconv : 0};
  r[n++] = {"part", s.part, 2 * part};
  r[n++] = {"gaepart", s.gaepart, 2 * 2 * 2048};
  r[n++] = {"ci", s.ci, CI_COUNT};
  r[n++] = {"cf", s.cf, CF_COUNT};
  return n;
}

static void check_shape(int B, int T, int Hz, int D, int H, int L, int h1, int h2, int c1, int c2,
                        int A, int pc, int ph, int pw, int F) {
  const RnnDims d = rnn_dims(B, T, Hz, D, H, h1, h2, A, c1, c2, pc, ph, pw, F, L);
#define SF "B %d T %d Hz %d D %d H %d L %d heads %d,%d/%d,%d A %d F %d"
#define SA B, T, Hz, D, H, L, h1, h2, c1, c2, A, F
  CHECK(d.nA_head == mlp_layout(d.Hin, h1, h2, A, 1).fcount && d.nS == d.nL + d.nCnn, SF, SA);
  Region r0[40], r[40];
  // null base: sizes only, every pointer null
  const RnnScratch s0 = rnn_scratch(d, nullptr);
  const int n = regions(d, s0, r0);
  int64_t sum = 0;
  for (int i = 0; i < n; ++i) {
    CHECK(r0[i].p == nullptr, "%s not null; " SF, r0[i].name, SA);
    CHECK(r0[i].need >= 0, "%s; " SF, r0[i].name, SA);
  }
  // a base address that is never dereferenced
  const uintptr_t base = (uintptr_t)1 << 32;
  const RnnScratch s = rnn_scratch(d, reinterpret_cast<void*>(base));
  CHECK(s.total_floats == s0.total_floats, SF, SA);
  regions(d, s, r);
  uintptr_t at = base;                                   // end of the regions so far
  for (int i = 0; i < n; ++i) {
    const uintptr_t p = reinterpret_cast<uintptr_t>(r[i].p);
    const uintptr_t next = i + 1 < n ? reinterpret_cast<uintptr_t>(r[i + 1].p)
                                     : base + 4 * (uintptr_t)s.total_floats;
    CHECK(p == at, "%s out of order or overlapping; " SF, r[i].name, SA);
    CHECK((p - base) % (64 * 4) == 0, "%s not on a 64-float boundary; " SF, r[i].name, SA);
    CHECK(next >= p && (int64_t)(next - p) >= 4 * r[i].need,
          "%s holds %lld floats, its uses need %lld; " SF, r[i].name,
          (long long)((next - p) / 4), (long long)r[i].need, SA);
    CHECK((int64_t)(next - p) == 4 * al64((int64_t)(next - p) / 4), "%s; " SF, r[i].name, SA);
    sum += (int64_t)(next - p) / 4;
    at = next;
  }
  CHECK(sum == s0.total_floats, "total_floats %lld, regions %lld; " SF,
        (long long)s0.total_floats, (long long)sum, SA);
  // the per-layer accessors stay inside their region for the last layer
  const int64_t BH = (int64_t)B * H, l = d.L - 1;
  CHECK(hbuf_of(d, s, l) + (d.S1 + 1) * BH <= s.cbuf, "hbuf_of; " SF, SA);
  CHECK(cbuf_of(d, s, l) + (d.E + 1) * BH <= s.gates, "cbuf_of; " SF, SA);
  CHECK(gates_of(d, s, l) + d.NE * d.G4 <= s.HA1, "gates_of; " SF, SA);
  CHECK(dgates_of(d, s, l) + d.NE * d.G4 <= s.values, "dgates_of; " SF, SA);
  CHECK(hbuf_of(d, s, 0) == s.hbuf && gates_of(d, s, 0) == s.gates, SF, SA);
  // the stem's parameter image [layer 0 | layer 1 | ...] ends at nL
  if (H > 0) {
    const float* P = reinterpret_cast<const float*>(base);
    const LstmP lp = lstm_layer(d, P, l);
    CHECK(lp.bhh + 4 * H == P + d.nL, "lstm_layer; " SF, SA);
  }
#undef SF
#undef SA
}

int main() {
  const int Bs[] = {1, 9, 19, 128, 1024}, Ts[] = {1, 6, 25}, Ds[] = {0, 1, 11, 42, 128};
  const int Hs[] = {0, 16, 100, 256}, Ls[] = {1, 2, 3}, As[] = {1, 4, 8, 32}, Fs[] = {0, 64};
  const int heads[][2] = {{1, 1}, {30, 18}, {32, 32}, {300, 200}, {520, 32}};
  long long shapes = 0;
  for (int B : Bs) for (int T : Ts) for (int hz = 0; hz < (T > 1 ? 2 : 1); ++hz)
  for (int D : Ds) for (int H : Hs) for (int L : Ls) for (auto& hd : heads) for (int A : As)
  for (int F : Fs) {
    const int Hz = hz ? T : 1;
    // what smi_ppo_rnn_phase rejects: layers without an LSTM, no input at all,
    // the MLP policy with more than one window
    if (L > 1 && H == 0) continue;
    if (D == 0 && F == 0) continue;
    if (H == 0 && Hz != T) continue;
    // the camera of tests/test_gpu_cnn.py; actor and critic heads alike, and
    // once per shape the critic narrower than the actor
    check_shape(B, T, Hz, D, H, L, hd[0], hd[1], hd[0], hd[1], A, F ? 3 : 0, F ? 84 : 0,
                F ? 84 : 0, F);
    if (A == 4) check_shape(B, T, Hz, D, H, L, hd[0], hd[1], 32, 32, A, F ? 3 : 0, F ? 84 : 0,
                            F ? 84 : 0, F);
    ++shapes;
  }
  std::printf("%lld shapes carved, %lld checks\n", shapes, g_checks);
  return 0;
}
