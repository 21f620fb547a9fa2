// r2l_half_io_lockstep.cpp -- driver `half_io` of r2l_lockstep_drivers.cpp (stand-alone, no Python) of the 16-bit output / cotangent
// kernels in their DEVICE forms on the CPU: the lock-step emulation's sources (r2l_lockstep.cpp, unchanged) under
// -fsanitize=address,undefined.  TEST INFRASTRUCTURE: run by tests/test_half_io.py.
// Every buffer is a heap block of exactly the size the C ABI asks for, so an access past a 2-byte tensor is an ASan report.  The
// 16-bit calls are compared bit for bit with the io = R2L_IO_F32 calls of the same build: out16 = narrow(out32), and the gradients of
// the widened cotangent on the plane route (R2L_BWD_PLANES: the float32 calls take the plane passes at these sizes too).
//   usage: r2l_lockstep_drivers half_io params.bin     (150 float32: the packed parameter block, R2L_P_* order)
namespace r2l_drv::half_io {

static Lcg lcg01{12345u};

static int run_case(const float* P, int B, int H, int W, int bn_mode, int io, int raw_u16) {
  const size_t px = (size_t)B * H * W, nws = r2l_isp_workspace_bytes(B, H, W);
  const int phase = R2L_STEP_ALL | R2L_STEP_KEEP_LUMA;
  const float* table[9];
  param_table(P, table);
  Block rawb(px * raw_bytes(raw_u16));
  fill_raw(lcg01, rawb.p, px, raw_u16, 0.15f, 0.7f);
  const void* raw = rawb.p;
  if (r2l_isp_io_supported(io, raw_u16, 0, B, H, W, phase) != 1) return fprintf(stderr, "not supported?\n"), 1;
  Buf<char> ws32(nws), ws16(nws);
  Buf<float> out32(3 * px), cot32(3 * px), gp32(R2L_P_NTRAIN), gp16(R2L_P_NTRAIN), gr32(raw_u16 ? 0 : px), gr16(raw_u16 ? 0 : px);
  Buf<unsigned short> out16(3 * px), cot16(3 * px);
  Buf<char> scr(r2l_isp_raw_grad_scratch_bytes(B, H, W));
  float rm[2][3] = {{0.4f, 0.45f, 0.35f}, {0.4f, 0.45f, 0.35f}}, rv[2][3] = {{0.03f, 0.05f, 0.04f}, {0.03f, 0.05f, 0.04f}};
  long long nbt[2] = {0, 0};
  CHECK(r2l_isp_step_fwd_io(raw, raw_u16, 65535.f, table, nullptr, bn_mode, rm[0], rv[0], &nbt[0], 1e-5, 0.1, out32.p, R2L_IO_F32,
                            ws32.p, nws, B, H, W, 1, phase, nullptr, nullptr));
  CHECK(r2l_isp_step_fwd_io(raw, raw_u16, 65535.f, table, nullptr, bn_mode, rm[1], rv[1], &nbt[1], 1e-5, 0.1, out16.p, io, ws16.p,
                            nws, B, H, W, 1, phase, nullptr, nullptr));
  long bad = 0;
  for (size_t i = 0; i < 3 * px; ++i) {
    const unsigned want = io == R2L_IO_BF16 ? r2l_f32_to_bf16_bits(out32.p[i]) : r2l_f32_to_f16_bits(out32.p[i]);
    if (out16.p[i] != want && bad++ < 5) fprintf(stderr, "out[%zu]: %04x, float32 call narrowed %04x\n", i, out16.p[i], want);
  }
  if (memcmp(rm[0], rm[1], sizeof rm[0]) || memcmp(rv[0], rv[1], sizeof rv[0]) || nbt[0] != nbt[1]) bad += 1000;
  for (size_t i = 0; i < 3 * px; ++i) {
    const float g = 2.f * lcg01() - 1.f;
    cot16.p[i] = (unsigned short)(io == R2L_IO_BF16 ? r2l_f32_to_bf16_bits(g) : r2l_f32_to_f16_bits(g));
    cot32.p[i] = io == R2L_IO_BF16 ? r2l_bf16_bits_to_f32(cot16.p[i]) : r2l_f16_bits_to_f32(cot16.p[i]);
  }
  const unsigned mask = R2L_GRAD_ALL_PARAMS | (raw_u16 ? 0u : (unsigned)R2L_GRAD_RAW);
  CHECK(r2l_isp_step_bwd_io(raw, raw_u16, 65535.f, nullptr, cot32.p, R2L_IO_F32, out32.p, gp32.p, nullptr, bn_mode, ws32.p, nws, B,
                            H, W, 1, phase, nullptr, nullptr, raw_u16 ? nullptr : gr32.p, raw_u16 ? nullptr : scr.p, scr.n, mask));
  // (a mask of GAMMA [+ RAW] alone: the 16-bit call still runs the full route and fills every element)
  const unsigned mask16 = R2L_GRAD_GAMMA | (raw_u16 ? 0u : (unsigned)R2L_GRAD_RAW);
  CHECK(r2l_isp_step_bwd_io(raw, raw_u16, 65535.f, nullptr, cot16.p, io, nullptr, gp16.p, nullptr, bn_mode, ws16.p, nws, B, H, W, 1,
                            phase, nullptr, nullptr, raw_u16 ? nullptr : gr16.p, raw_u16 ? nullptr : scr.p, scr.n, mask16));
  if (memcmp(gp32.p, gp16.p, sizeof(float) * R2L_P_NTRAIN)) {
    ++bad;
    for (int i = 0; i < R2L_P_NTRAIN; ++i)
      if (memcmp(gp32.p + i, gp16.p + i, 4)) {
        fprintf(stderr, "grad_params[%d]: %.9g, float32 call %.9g\n", i, gp16.p[i], gp32.p[i]);
        break;
      }
  }
  if (!raw_u16 && memcmp(gr32.p, gr16.p, sizeof(float) * px)) ++bad, fprintf(stderr, "grad_raw differs\n");
  printf("%dx%dx%d bn_mode %d io %d raw_u16 %d: %ld mismatches\n", B, H, W, bn_mode, io, raw_u16, bad);
  return bad ? 1 : 0;
}

int run(int argc, char** argv) {
  float P[R2L_P_COUNT];
  if (argc != 2 || !read_params(argv[1], P)) return 2;
  setenv("R2L_BWD_PLANES", "1", 1);
  static const int shapes[3][3] = {{2, 4, 4}, {2, 4, 260}, {1, 70, 260}};
  int rc = 0, n = 0;
  for (const auto& s : shapes)
    for (int io = R2L_IO_BF16; io <= R2L_IO_F16; ++io) {
      // BatchNorm train (apply pass, recomputing sums) and none / eval (the row-streaming forward) in turn, both frame types
      const int bn_mode = (n % 3 == 0) ? R2L_BN_TRAIN : (n % 3 == 1 ? R2L_BN_NONE : R2L_BN_EVAL), raw_u16 = (n >> 1) & 1;
      rc |= run_case(P, s[0], s[1], s[2], bn_mode, io, raw_u16);
      rc |= run_case(P, s[0], s[1], s[2], bn_mode == R2L_BN_TRAIN ? R2L_BN_NONE : R2L_BN_TRAIN, io, !raw_u16);
      ++n;
    }
  // what the calls refuse
  {
    float o[64];
    if (r2l_isp_io_supported(R2L_IO_BF16, 0, 0, 1, 4, 4, 0) != 0 || r2l_isp_io_supported(R2L_IO_F16, 0, 0, 1, 4, 6, R2L_STEP_KEEP_LUMA) != 0 ||
        r2l_isp_io_supported(R2L_IO_F32, 0, 1, 1, 4, 6, 0) != 1 || r2l_isp_io_supported(7, 0, 0, 1, 4, 4, R2L_STEP_KEEP_LUMA) != 0)
      rc |= 1, fprintf(stderr, "r2l_isp_io_supported\n");
    const float* table[9] = {P, P, P, P, P, P, P, P, P};
    if (r2l_isp_step_fwd_io(o, 0, 1.f, table, nullptr, R2L_BN_NONE, nullptr, nullptr, nullptr, 1e-5, 0.1, o, R2L_IO_BF16, o, 0, 1, 4, 4, 1,
                            0, nullptr, nullptr) != -3)
      rc |= 1, fprintf(stderr, "fwd_io without KEEP_LUMA must return -3\n");
  }
  return rc;
}

}  // namespace r2l_drv::half_io
