// r2l_bn_settings_lockstep.cpp -- driver `bn_settings` of r2l_lockstep_drivers.cpp (stand-alone, no Python): train-mode BatchNorm off
// its defaults on the kernels' DEVICE forms on the CPU -- the streaming statistics kernel, whose last workgroup runs its own copy of
// the bookkeeping's argument block, fetches the running statistics early and writes num_batches_tracked itself, never runs on the
// serial emulation -- under -fsanitize=address,undefined.  TEST INFRASTRUCTURE: run by tests/test_bn_settings.py.
// Per case and step two calls of r2l_isp_step_fwd in a malloc workspace of exactly the queried size: R2L_BN_NONE gives the
// pre-normalisation x (the library's own float32, so only the normalisation is under test), R2L_BN_TRAIN with the case's eps /
// momentum / buffers (possibly NULL) the normalised output -- as one call, and as phase A + r2l_bn_finalize (the launch inside phase
// B) over the statistics phase A left.  Three steps in a row on new frames against the statistics of x accumulated in long double on
// the host: the output within 1e-5 * max(1, istd), running mean / variance within rtol 1e-5 + atol 1e-6, the counter equal.
//   usage: r2l_lockstep_drivers bn_settings
#include <math.h>

namespace r2l_drv::bn_settings {

static Lcg lcg01{24680u};

struct Setting {
  int id;
  double eps, momentum;  // momentum < 0: nn.BatchNorm2d(momentum=None), the cumulative average
  bool track;
};

static int run_case(const float* P, int B, int H, int W, int raw_u16, const Setting& s, bool phases) {
  const size_t px = (size_t)B * H * W, nws = r2l_isp_workspace_bytes(B, H, W);
  const float* table[9];
  param_table(P, table);
  Block rawb(px * raw_bytes(raw_u16)), ws(nws);
  Buf<float> x(3 * px), y(3 * px);
  Buf<double> gathered(7);
  // setting 3 (momentum 0) starts from uneven statistics, which must stay as they are bit for bit
  const bool frozen = s.momentum == 0.0;
  float rm[3] = {0.f, 0.f, 0.f}, rv[3] = {1.f, 1.f, 1.f};
  if (frozen) rm[0] = 0.4f, rm[1] = 0.45f, rm[2] = 0.35f, rv[0] = 0.03f, rv[1] = 0.05f, rv[2] = 0.04f;
  const float rm0[3] = {rm[0], rm[1], rm[2]}, rv0[3] = {rv[0], rv[1], rv[2]};
  long double hm[3] = {rm[0], rm[1], rm[2]}, hv[3] = {rv[0], rv[1], rv[2]};
  long long nbt = 0;
  long bad = 0;
  double worst_out = 0.0, worst_stats = 0.0;
  for (int step = 0; step < 3; ++step) {
    fill_raw(lcg01, rawb.p, px, raw_u16, 0.15f, 0.7f);
    CHECK(r2l_isp_step_fwd(rawb.p, raw_u16, 65535.f, table, nullptr, R2L_BN_NONE, nullptr, nullptr, nullptr, s.eps, s.momentum, x.p,
                           ws.p, nws, B, H, W, 1, R2L_STEP_ALL | R2L_STEP_KEEP_LUMA, nullptr, nullptr));
    float *prm = s.track ? rm : nullptr, *prv = s.track ? rv : nullptr;
    long long* pnbt = s.track ? &nbt : nullptr;
    record_begin();
    if (!phases) {
      CHECK(r2l_isp_step_fwd(rawb.p, raw_u16, 65535.f, table, nullptr, R2L_BN_TRAIN, prm, prv, pnbt, s.eps, s.momentum, y.p, ws.p, nws, B,
                             H, W, 1, R2L_STEP_ALL | R2L_STEP_KEEP_LUMA, nullptr, nullptr));
    } else {
      CHECK(r2l_isp_step_fwd(rawb.p, raw_u16, 65535.f, table, nullptr, R2L_BN_TRAIN, prm, prv, pnbt, s.eps, s.momentum, y.p, ws.p, nws, B,
                             H, W, 1, R2L_STEP_A | R2L_STEP_KEEP_LUMA, nullptr, nullptr));
      memcpy(gathered.p, ws.p + r2l_isp_step_offset(R2L_STEP_STATS, B, H, W), 7 * sizeof(double));
      if (gathered.p[6] != (double)px) ++bad, fprintf(stderr, "phase A left a pixel count of %g\n", gathered.p[6]);
      CHECK(r2l_isp_step_fwd(rawb.p, raw_u16, 65535.f, table, nullptr, R2L_BN_TRAIN, prm, prv, pnbt, s.eps, s.momentum, y.p, ws.p, nws, B,
                             H, W, 1, R2L_STEP_B | R2L_STEP_KEEP_LUMA, gathered.p, nullptr));
    }
    {  // the route: W >= 260 takes the streaming statistics kernel (its own finalization in a whole step), phase B the finalize launch
      std::lock_guard<std::mutex> g(r2l_ls_record_mutex);
      bool streamed = false, finalized = false;
      for (const auto& kv : r2l_ls_record) {
        streamed |= kv.first.find("fwd_stream_stats") != std::string::npos;
        finalized |= kv.first.find("bn_finalize") != std::string::npos;
      }
      r2l_ls_record_on = false;
      if (streamed != (W >= 260) || finalized != phases) ++bad, fprintf(stderr, "route: streaming statistics %d, finalize launch %d\n", streamed, finalized);
    }
    const long double n = (long double)px;
    for (int c = 0; c < 3; ++c) {
      long double s1 = 0, s2 = 0;
      for (int b = 0; b < B; ++b)
        for (size_t i = 0; i < (size_t)H * W; ++i) s1 += x.p[((size_t)b * 3 + c) * H * W + i];
      const long double mean = s1 / n;
      for (int b = 0; b < B; ++b)
        for (size_t i = 0; i < (size_t)H * W; ++i) {
          const long double d = x.p[((size_t)b * 3 + c) * H * W + i] - mean;
          s2 += d * d;
        }
      const long double var = s2 / n, istd = 1 / sqrtl(var + s.eps);
      const double lim = 1e-5 * (istd > 1 ? (double)istd : 1.0);
      for (int b = 0; b < B; ++b)
        for (size_t i = 0; i < (size_t)H * W; ++i) {
          const size_t k = ((size_t)b * 3 + c) * H * W + i;
          const double e = fabs((double)y.p[k] - (double)((x.p[k] - mean) * istd));
          if (e / lim > worst_out) worst_out = e / lim;
          if (!(e <= lim) && bad++ < 5) fprintf(stderr, "step %d out[%zu]: %.9g, want %.9g (limit %.3g)\n", step, k, y.p[k], (double)((x.p[k] - mean) * istd), lim);
        }
      if (s.track) {
        const long double f = s.momentum < 0 ? 1.0L / (long double)(step + 1) : (long double)s.momentum;
        hm[c] = (1 - f) * hm[c] + f * mean;
        hv[c] = (1 - f) * hv[c] + f * var * (n / (n > 1 ? n - 1 : 1));
        const double em = fabs((double)rm[c] - (double)hm[c]) / (1e-6 + 1e-5 * fabs((double)hm[c]));
        const double ev = fabs((double)rv[c] - (double)hv[c]) / (1e-6 + 1e-5 * fabs((double)hv[c]));
        if (em > worst_stats) worst_stats = em;
        if (ev > worst_stats) worst_stats = ev;
        if (!(em <= 1 && ev <= 1) && bad++ < 5)
          fprintf(stderr, "step %d channel %d: running mean %.9g (want %.9Lg), running variance %.9g (want %.9Lg)\n", step, c, rm[c], hm[c], rv[c], hv[c]);
      }
    }
    if (s.track && nbt != step + 1) ++bad, fprintf(stderr, "step %d: num_batches_tracked %lld\n", step, nbt);
    if (frozen && (memcmp(rm, rm0, sizeof rm) || memcmp(rv, rv0, sizeof rv))) ++bad, fprintf(stderr, "step %d: momentum 0 moved the running statistics\n", step);
  }
  // without buffers nothing of the kind is written
  if (!s.track && (nbt != 0 || memcmp(rm, rm0, sizeof rm) || memcmp(rv, rv0, sizeof rv))) ++bad, fprintf(stderr, "buffers written without being given\n");
  printf("case %dx%dx%d raw_u16 %d setting %d %s: out %.3f of its limit, running statistics %.3f of theirs, %ld mismatches%s\n", B, H, W,
         raw_u16, s.id, phases ? "phases" : "whole", worst_out, worst_stats, bad, bad ? "" : " ok");
  return bad ? 1 : 0;
}

int run(int argc, char** argv) {
  (void)argv;
  if (argc != 1) return 2;
  // the drone camera, a bilinear debayer, the reference's sharpening and blur kernels, the YUV matrices: R2L_P_* order
  float P[R2L_P_COUNT];
  memset(P, 0, sizeof P);
  for (int i = 0; i < 4; ++i) P[R2L_P_BLACK_LEVEL + i] = (float)CAMERA[i];
  for (int i = 0; i < 3; ++i) P[R2L_P_WHITE_BALANCE + i] = (float)CAMERA[4 + i];
  for (int i = 0; i < 9; ++i) P[R2L_P_CCM + i] = (float)CAMERA[7 + i];
  P[R2L_P_GAMMA] = 2.2f;
  static const float RB[9] = {.25f, .5f, .25f, .5f, 1.f, .5f, .25f, .5f, .25f}, G[9] = {0.f, .25f, 0.f, .25f, 1.f, .25f, 0.f, .25f, 0.f};
  for (int k = 0; k < 3; ++k)
    for (int i = 0; i < 9; ++i) P[R2L_P_DEBAYER + (k * 3 + k) * 9 + i] = k == 1 ? G[i] : RB[i];
  static const float SHARP[9] = {0, -1, 0, -1, 5, -1, 0, -1, 0}, B1[5] = {1, 4, 6, 4, 1};
  for (int i = 0; i < 9; ++i) P[R2L_P_SHARPEN + i] = SHARP[i];
  for (int i = 0; i < 5; ++i)
    for (int j = 0; j < 5; ++j) P[R2L_P_BLUR + i * 5 + j] = B1[i] * B1[j] / 256.f;
  static const float RGB2YUV[9] = {0.299f, 0.587f, 0.114f, -0.14714119f, -0.28886916f, 0.43601035f, 0.61497538f, -0.51496512f, -0.10001026f};
  static const float YUV2RGB[9] = {1.f, 0.f, 1.13988303f, 1.f, -0.394642334f, -0.58062185f, 1.f, 2.03206185f, 0.f};
  for (int i = 0; i < 9; ++i) P[R2L_P_M_RGB2YUV + i] = RGB2YUV[i], P[R2L_P_M_YUV2RGB + i] = YUV2RGB[i];

  // one / two wavefronts per row, four on 16-bit frames (the stats_apply route), the ragged tile kernel
  static const int SHAPES[4][4] = {{1, 8, 8, 0}, {1, 8, 260, 0}, {1, 8, 516, 1}, {1, 8, 10, 0}};
  static const Setting SETTINGS[3] = {{1, 1e-3, -1.0, true}, {3, 1e-5, 0.0, true}, {4, 1e-3, 0.1, false}};
  int rc = 0;
  for (const auto& sh : SHAPES)
    for (const auto& s : SETTINGS)
      for (int phases = 0; phases < 2; ++phases) rc |= run_case(P, sh[0], sh[1], sh[2], sh[3], s, phases != 0);
  return rc;
}

}  // namespace r2l_drv::bn_settings
