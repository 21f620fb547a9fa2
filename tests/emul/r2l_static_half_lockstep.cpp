// r2l_static_half_lockstep.cpp -- driver `static_half` of r2l_lockstep_drivers.cpp (stand-alone, no Python) of the static chains'
// 16-bit-output kernels in their DEVICE forms on the CPU: the lock-step emulation's sources (r2l_lockstep.cpp, unchanged) under
// -fsanitize=address,undefined.  TEST INFRASTRUCTURE: run by tests/test_static_half_io.py.
// Every buffer is a heap block of exactly the size the C ABI asks for: the 16-bit output is half the float32 one, so a store
// that is too wide, or lands at a float32 offset, is an ASan report.  Each 16-bit call (r2l_static_fwd_io, R2L_IO_BF16 / _F16) is
// compared bit for bit with the out_io = R2L_IO_F32 call of the same build narrowed by the host helpers of r2l_common.h.
//   usage: r2l_lockstep_drivers static_half
namespace r2l_drv::static_half {

static Lcg lcg01{2468u};

static const char* const launched_suffix[3] = {"", "_bf16_kernel", "_f16_kernel"};

static int run_case(int B, int H, int W, int debayer, int sharpening, int denoising, int frames, int io, bool norm) {
  const size_t px = (size_t)B * H * W;
  Block rawb(px * raw_bytes(frames));
  // values below the black level, inside, and (after white balance) above the clip
  fill_raw(lcg01, rawb.p, px, frames, 0.02f, 0.9f);
  const void* raw = rawb.p;
  const char* why = r2l_static_io_supported(frames, H, W, debayer, sharpening, denoising, nullptr);
  if (why) return fprintf(stderr, "not served: %s\n", why), 1;
  if (r2l_static_workspace_bytes(B, H, W, debayer, sharpening, denoising) != 0) return fprintf(stderr, "workspace?\n"), 1;
  Buf<float> out32(3 * px);
  Buf<unsigned short> out16(3 * px);
  const float* ms = norm ? MEAN_STD : nullptr;
  int e = r2l_static_fwd_io(raw, frames, 65535.f, out32.p, R2L_IO_F32, B, H, W, CAMERA, debayer, sharpening, denoising, 2.2, nullptr, ms,
                            nullptr, 0, nullptr);
  if (e) return fprintf(stderr, "float32 call -> %d: %s\n", e, r2l_last_error()), 1;
  record_begin();
  e = r2l_static_fwd_io(raw, frames, 65535.f, out16.p, io, B, H, W, CAMERA, debayer, sharpening, denoising, 2.2, nullptr, ms, nullptr, 0,
                        nullptr);
  r2l_ls_record_on = false;
  if (e) return fprintf(stderr, "16-bit call -> %d: %s\n", e, r2l_last_error()), 1;
  long bad = 0;
  // exactly one launch, of a 16-bit instantiation
  if (r2l_ls_record.size() != 1 || r2l_ls_record.begin()->second != 1) bad += 1000;
  for (const auto& kv : r2l_ls_record) {
    const std::string sfx = launched_suffix[io];
    if (kv.first.size() < sfx.size() || kv.first.compare(kv.first.size() - sfx.size(), sfx.size(), sfx)) {
      bad += 1000;
      fprintf(stderr, "launched %s\n", kv.first.c_str());
    }
  }
  bool inside = false, clipped = false;
  for (size_t i = 0; i < 3 * px; ++i) {
    const unsigned want = io == R2L_IO_BF16 ? r2l_f32_to_bf16_bits(out32.p[i]) : r2l_f32_to_f16_bits(out32.p[i]);
    if (out16.p[i] != want && bad++ < 5) fprintf(stderr, "out[%zu]: %04x, float32 call narrowed %04x\n", i, out16.p[i], want);
    if (!norm) {
      inside |= out32.p[i] > 0.f && out32.p[i] < 1.f;
      clipped |= out32.p[i] == 0.f || out32.p[i] == 1.f;
    }
  }
  if (!norm && !(inside && clipped)) ++bad, fprintf(stderr, "the frames must reach both sides of the clip\n");
  printf("%dx%dx%d debayer %d sharpening %d denoising %d frames %d io %d norm %d: %ld mismatches\n", B, H, W, debayer, sharpening,
         denoising, frames, io, (int)norm, bad);
  return bad ? 1 : 0;
}

int run(int, char**) {
  static const int shapes[3][3] = {{1, 6, 80}, {1, 10, 260}, {1, 4, 4}};
  // the short chain (r2l_static_stream.h) and the luma chain (r2l_static_chain.h: Gaussian and median outputs) x both demosaics
  static const int chains[3][2] = {{R2L_SHARPEN_NONE, R2L_DENOISE_NONE}, {R2L_SHARPEN_FILTER, R2L_DENOISE_GAUSSIAN},
                                   {R2L_SHARPEN_FILTER, R2L_DENOISE_MEDIAN}};
  int rc = 0, n = 0;
  for (const auto& s : shapes)
    for (const auto& c : chains)
      for (int deb = R2L_DEBAYER_BILINEAR; deb <= R2L_DEBAYER_MALVAR2004; ++deb)
        for (int frames = R2L_FRAMES_F32; frames <= R2L_FRAMES_U16; ++frames)
          for (int io = R2L_IO_BF16; io <= R2L_IO_F16; ++io, ++n)
            rc |= run_case(s[0], s[1], s[2], deb, c[0], c[1], frames, io, (n % 3) == 1);
  // unsharp_masking (the 7-row chroma ring) once per 16-bit type, float64 frames on the short chain once per demosaic
  rc |= run_case(1, 10, 260, R2L_DEBAYER_BILINEAR, R2L_SHARPEN_UNSHARP, R2L_DENOISE_GAUSSIAN, R2L_FRAMES_F32, R2L_IO_BF16, false);
  rc |= run_case(1, 10, 260, R2L_DEBAYER_MALVAR2004, R2L_SHARPEN_UNSHARP, R2L_DENOISE_MEDIAN, R2L_FRAMES_U16, R2L_IO_F16, true);
  {
    const size_t px = 10 * 260;
    Buf<double> raw(px);
    for (size_t i = 0; i < px; ++i) raw.p[i] = 0.02 + 0.9 * lcg01();
    for (int deb = R2L_DEBAYER_BILINEAR; deb <= R2L_DEBAYER_MALVAR2004; ++deb) {
      Buf<float> out32(3 * px);
      Buf<unsigned short> out16(3 * px);
      const int io = deb ? R2L_IO_F16 : R2L_IO_BF16;
      int e = r2l_static_fwd_io(raw.p, R2L_FRAMES_F64, 1.f, out32.p, R2L_IO_F32, 1, 10, 260, CAMERA, deb, 0, 0, 2.2, nullptr, MEAN_STD,
                                nullptr, 0, nullptr);
      e |= r2l_static_fwd_io(raw.p, R2L_FRAMES_F64, 1.f, out16.p, io, 1, 10, 260, CAMERA, deb, 0, 0, 2.2, nullptr, MEAN_STD, nullptr, 0,
                             nullptr);
      long bad = e ? 1 : 0;
      for (size_t i = 0; i < 3 * px; ++i)
        bad += out16.p[i] != (io == R2L_IO_BF16 ? r2l_f32_to_bf16_bits(out32.p[i]) : r2l_f32_to_f16_bits(out32.p[i]));
      printf("1x10x260 float64 frames debayer %d io %d: %ld mismatches\n", deb, io, bad);
      rc |= bad != 0;
    }
  }
  // what the calls refuse: -3 with the reason, nothing written
  {
    Buf<float> raw(4 * 8);
    Buf<unsigned short> o(3 * 4 * 8);
    for (size_t i = 0; i < raw.n; ++i) raw.p[i] = 0.5f;
    struct { int frames, W, deb, sh, dn; } no[] = {{R2L_FRAMES_F32, 8, R2L_DEBAYER_MENON2007, 0, 0},
                                                   {R2L_FRAMES_F32, 8, 0, R2L_SHARPEN_FILTER, R2L_DENOISE_FFT},
                                                   {R2L_FRAMES_F32, 6, 0, 0, 0},
                                                   {R2L_FRAMES_F32, 2052, 0, 0, 0},
                                                   {R2L_FRAMES_F32, 1028, 0, R2L_SHARPEN_UNSHARP, 0},
                                                   {R2L_FRAMES_F64, 8, 0, R2L_SHARPEN_FILTER, R2L_DENOISE_GAUSSIAN}};
    for (const auto& q : no) {
      const char* why = r2l_static_io_supported(q.frames, 4, q.W, q.deb, q.sh, q.dn, nullptr);
      if (!why || !*why) rc |= 1, fprintf(stderr, "W %d debayer %d sharpening %d denoising %d must not be served\n", q.W, q.deb, q.sh, q.dn);
    }
    const double med5[R2L_SOPT_COUNT] = {1.0, 1.0, 0.5, 0.3, 5.0};
    if (!r2l_static_io_supported(R2L_FRAMES_F32, 4, 8, 0, R2L_SHARPEN_FILTER, R2L_DENOISE_MEDIAN, med5)) rc |= 1, fprintf(stderr, "5x5 median\n");
    if (r2l_static_io_supported(R2L_FRAMES_F32, 4, 8, 0, R2L_SHARPEN_FILTER, R2L_DENOISE_MEDIAN, nullptr)) rc |= 1, fprintf(stderr, "3x3 median\n");
    const int e = r2l_static_fwd_io(raw.p, R2L_FRAMES_F32, 1.f, o.p, R2L_IO_BF16, 1, 4, 8, CAMERA, R2L_DEBAYER_MENON2007, 0, 0, 2.2, nullptr,
                                    nullptr, nullptr, 0, nullptr);
    if (e != -3 || !strstr(r2l_last_error(), "menon2007")) rc |= 1, fprintf(stderr, "Menon2007 must return -3 with the reason\n");
    for (size_t i = 0; i < o.n; ++i)
      if (o.p[i] != 0xffffu) rc |= 1;
    if (r2l_static_fwd_io(raw.p, R2L_FRAMES_F32, 1.f, o.p, 7, 1, 4, 8, CAMERA, 0, 0, 0, 2.2, nullptr, nullptr, nullptr, 0, nullptr) != -1)
      rc |= 1, fprintf(stderr, "an unknown out_io must return -1\n");
  }
  return rc;
}

}  // namespace r2l_drv::static_half
