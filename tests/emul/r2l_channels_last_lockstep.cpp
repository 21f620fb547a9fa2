// r2l_channels_last_lockstep.cpp -- driver `channels_last` of r2l_lockstep_drivers.cpp (stand-alone, no Python) of the channels-last
// output / cotangent kernels in their DEVICE forms on the CPU: the lock-step emulation's sources (r2l_lockstep.cpp, unchanged) under
// -fsanitize=address,undefined.  TEST INFRASTRUCTURE: run by tests/test_channels_last.py.
// `out` and `grad_out` are heap blocks of exactly 3 B H W elements, so an interleaved access that strays lands in a redzone.  The
// R2L_LAYOUT_NHWC calls are compared bit for bit with the R2L_LAYOUT_NCHW calls of the same element type and build: out_nhwc is
// out_nchw permuted, and the gradients are those of the permuted cotangent on the plane route (R2L_BWD_PLANES: the planar float32
// calls take the plane passes at these sizes too).
//   usage: r2l_lockstep_drivers channels_last params.bin     (150 float32: the packed parameter block, R2L_P_* order)
namespace r2l_drv::channels_last {

static Lcg lcg01{4321u};

// element (b, k, y, x) of a (B,3,H,W) tensor: planar and channels-last
static size_t at_nchw(int H, int W, int b, int k, int y, int x) { return (((size_t)b * 3 + k) * H + y) * W + x; }
static size_t at_nhwc(int H, int W, int b, int k, int y, int x) { return (((size_t)b * H + y) * W + x) * 3 + k; }

static int run_case(const float* P, int B, int H, int W, int bn_mode, int io, int raw_u16) {
  const size_t px = (size_t)B * H * W, nws = r2l_isp_workspace_bytes(B, H, W), esz = io == R2L_IO_F32 ? 4 : 2;
  const int phase = R2L_STEP_ALL | R2L_STEP_KEEP_LUMA;
  const float* table[9];
  param_table(P, table);
  Block rawb(px * raw_bytes(raw_u16));
  fill_raw(lcg01, rawb.p, px, raw_u16, 0.15f, 0.7f);
  const void* raw = rawb.p;
  if (r2l_isp_layout_supported(io, R2L_LAYOUT_NHWC, raw_u16, 0, B, H, W, phase) != 1) return fprintf(stderr, "not supported?\n"), 1;
  Buf<char> wsp(nws), wsl(nws);
  Buf<char> outp(3 * px * esz), outl(3 * px * esz), cotp(3 * px * esz), cotl(3 * px * esz);  // exactly 3 B H W elements each
  Buf<float> gpp(R2L_P_NTRAIN), gpl(R2L_P_NTRAIN), grp(raw_u16 ? 0 : px), grl(raw_u16 ? 0 : px);
  Buf<char> scr(r2l_isp_raw_grad_scratch_bytes(B, H, W));
  float rm[2][3] = {{0.4f, 0.45f, 0.35f}, {0.4f, 0.45f, 0.35f}}, rv[2][3] = {{0.03f, 0.05f, 0.04f}, {0.03f, 0.05f, 0.04f}};
  long long nbt[2] = {0, 0};
  CHECK(r2l_isp_step_fwd_layout(raw, raw_u16, 65535.f, table, nullptr, bn_mode, rm[0], rv[0], &nbt[0], 1e-5, 0.1, outp.p, io,
                                R2L_LAYOUT_NCHW, wsp.p, nws, B, H, W, 1, phase, nullptr, nullptr));
  CHECK(r2l_isp_step_fwd_layout(raw, raw_u16, 65535.f, table, nullptr, bn_mode, rm[1], rv[1], &nbt[1], 1e-5, 0.1, outl.p, io,
                                R2L_LAYOUT_NHWC, wsl.p, nws, B, H, W, 1, phase, nullptr, nullptr));
  long bad = 0;
  for (int b = 0; b < B; ++b)
    for (int k = 0; k < 3; ++k)
      for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x)
          if (memcmp(outp.p + at_nchw(H, W, b, k, y, x) * esz, outl.p + at_nhwc(H, W, b, k, y, x) * esz, esz) && bad++ < 5)
            fprintf(stderr, "out[%d,%d,%d,%d] differs from the planar call\n", b, k, y, x);
  if (memcmp(rm[0], rm[1], sizeof rm[0]) || memcmp(rv[0], rv[1], sizeof rv[0]) || nbt[0] != nbt[1]) bad += 1000;
  for (int b = 0; b < B; ++b)
    for (int k = 0; k < 3; ++k)
      for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x) {
          const float g = 2.f * lcg01() - 1.f;
          const unsigned short h = (unsigned short)(io == R2L_IO_BF16 ? r2l_f32_to_bf16_bits(g) : r2l_f32_to_f16_bits(g));
          const void* e = io == R2L_IO_F32 ? (const void*)&g : (const void*)&h;
          memcpy(cotp.p + at_nchw(H, W, b, k, y, x) * esz, e, esz);
          memcpy(cotl.p + at_nhwc(H, W, b, k, y, x) * esz, e, esz);
        }
  const unsigned mask = R2L_GRAD_ALL_PARAMS | (raw_u16 ? 0u : (unsigned)R2L_GRAD_RAW);
  CHECK(r2l_isp_step_bwd_layout(raw, raw_u16, 65535.f, nullptr, cotp.p, io, R2L_LAYOUT_NCHW, outp.p, gpp.p, nullptr, bn_mode, wsp.p,
                                nws, B, H, W, 1, phase, nullptr, nullptr, raw_u16 ? nullptr : grp.p, raw_u16 ? nullptr : scr.p, scr.n,
                                mask));
  // (a mask of GAMMA [+ RAW] alone: the channels-last call still runs the full route and fills every element; `out` is not read)
  const unsigned maskl = R2L_GRAD_GAMMA | (raw_u16 ? 0u : (unsigned)R2L_GRAD_RAW);
  CHECK(r2l_isp_step_bwd_layout(raw, raw_u16, 65535.f, nullptr, cotl.p, io, R2L_LAYOUT_NHWC, nullptr, gpl.p, nullptr, bn_mode, wsl.p,
                                nws, B, H, W, 1, phase, nullptr, nullptr, raw_u16 ? nullptr : grl.p, raw_u16 ? nullptr : scr.p, scr.n,
                                maskl));
  if (memcmp(gpp.p, gpl.p, sizeof(float) * R2L_P_NTRAIN)) {
    ++bad;
    for (int i = 0; i < R2L_P_NTRAIN; ++i)
      if (memcmp(gpp.p + i, gpl.p + i, 4)) {
        fprintf(stderr, "grad_params[%d]: %.9g, planar call %.9g\n", i, gpl.p[i], gpp.p[i]);
        break;
      }
  }
  if (!raw_u16 && memcmp(grp.p, grl.p, sizeof(float) * px)) ++bad, fprintf(stderr, "grad_raw differs\n");
  printf("%dx%dx%d bn_mode %d io %d raw_u16 %d: %ld mismatches\n", B, H, W, bn_mode, io, raw_u16, bad);
  return bad ? 1 : 0;
}

int run(int argc, char** argv) {
  float P[R2L_P_COUNT];
  if (argc != 2 || !read_params(argv[1], P)) return 2;
  setenv("R2L_BWD_PLANES", "1", 1);
  static const int shapes[2][3] = {{2, 6, 80}, {1, 4, 260}};  // (the second: a last strip of one lane)
  int rc = 0, n = 0;
  for (const auto& s : shapes)
    for (int io = R2L_IO_F32; io <= R2L_IO_F16; ++io) {
      // BatchNorm train (apply pass, recomputing sums) and none / eval (the row-streaming forward) in turn, both frame types
      const int bn_mode = (n % 3 == 0) ? R2L_BN_TRAIN : (n % 3 == 1 ? R2L_BN_NONE : R2L_BN_EVAL), raw_u16 = (n >> 1) & 1;
      rc |= run_case(P, s[0], s[1], s[2], bn_mode, io, raw_u16);
      rc |= run_case(P, s[0], s[1], s[2], bn_mode == R2L_BN_TRAIN ? R2L_BN_NONE : R2L_BN_TRAIN, io, !raw_u16);
      ++n;
    }
  // what the calls refuse
  {
    alignas(16) float o[64];
    const int K = R2L_STEP_KEEP_LUMA;
    if (r2l_isp_layout_supported(R2L_IO_F32, R2L_LAYOUT_NHWC, 0, 0, 1, 4, 4, 0) != 0 ||
        r2l_isp_layout_supported(R2L_IO_F32, R2L_LAYOUT_NHWC, 0, 0, 1, 4, 6, K) != 0 ||
        r2l_isp_layout_supported(R2L_IO_F32, R2L_LAYOUT_NCHW, 0, 1, 1, 4, 6, 0) != 1 ||
        r2l_isp_layout_supported(R2L_IO_F32, 2, 0, 0, 1, 4, 4, K) != 0 || r2l_isp_layout_supported(R2L_IO_BF16, R2L_LAYOUT_NHWC, 0, 0, 1, 4, 4, K) != 1)
      rc |= 1, fprintf(stderr, "r2l_isp_layout_supported\n");
    const float* table[9] = {P, P, P, P, P, P, P, P, P};
    if (r2l_isp_step_fwd_layout(o, 0, 1.f, table, nullptr, R2L_BN_NONE, nullptr, nullptr, nullptr, 1e-5, 0.1, o, R2L_IO_F32,
                                R2L_LAYOUT_NHWC, o, 0, 1, 4, 4, 1, 0, nullptr, nullptr) != -3)
      rc |= 1, fprintf(stderr, "fwd_layout without KEEP_LUMA must return -3\n");
    if (r2l_isp_step_fwd_layout(o, 0, 1.f, table, nullptr, R2L_BN_NONE, nullptr, nullptr, nullptr, 1e-5, 0.1, o, R2L_IO_F32, 2, o, 0,
                                1, 4, 4, 1, K, nullptr, nullptr) != -1)
      rc |= 1, fprintf(stderr, "a layout outside the enum must return -1\n");
    if (r2l_isp_step_fwd_layout(o, 0, 1.f, table, nullptr, R2L_BN_NONE, nullptr, nullptr, nullptr, 1e-5, 0.1, o + 2, R2L_IO_F32,
                                R2L_LAYOUT_NHWC, o, 0, 1, 4, 4, 1, K, nullptr, nullptr) != -1)
      rc |= 1, fprintf(stderr, "a float32 NHWC out at 8-byte alignment must return -1\n");
    if (r2l_isp_step_bwd_layout(o, 0, 1.f, nullptr, (char*)o + 4, R2L_IO_BF16, R2L_LAYOUT_NHWC, nullptr, o, nullptr, R2L_BN_NONE, o, 0,
                                1, 4, 4, 1, K, nullptr, nullptr, nullptr, nullptr, 0, 0) != -1)
      rc |= 1, fprintf(stderr, "a 16-bit NHWC grad_out at 4-byte alignment must return -1\n");
  }
  return rc;
}

}  // namespace r2l_drv::channels_last
