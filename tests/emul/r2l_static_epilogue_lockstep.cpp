// r2l_static_epilogue_lockstep.cpp -- stand-alone program (own main, no Python) of the static chains' epilogue kernels
// (r2l_static_fwd_epilogue: the weak augmentation in the stores) in their DEVICE forms on the CPU: the lock-step emulation's sources
// (r2l_lockstep.cpp, unchanged) under -fsanitize=address,undefined.  TEST INFRASTRUCTURE: built and run by
// tests/test_static_epilogue.py with the flags and the dependency list of tests/lockstep_driver.py.
// Every buffer is a heap block of exactly the size the C ABI names, so that a store based one group off under sc = -1, or a
// float32-wide store into a 16-bit output, is an ASan report.  Each epilogue call is compared element by element with the plain
// call of the same build (r2l_static_fwd_io, the same out_io) permuted by a host loop over r2l_aug_map -- the definition the
// permutation kernel uses.
#define R2L_TEST_HOOKS 1
#include "r2l_lockstep.cpp"

#include "r2l_driver_util.h"

using namespace r2l_drv;

static Lcg lcg01{13579u};

static int epi_bits(int hflip, int vflip, int k) {
  return (hflip ? R2L_STEP_EPI_HFLIP : 0) | (vflip ? R2L_STEP_EPI_VFLIP : 0) | (k << R2L_STEP_EPI_ROT_SHIFT);
}

// one launch, of an epilogue instantiation
static long record_is_one_epi_launch() {
  long bad = (r2l_ls_record.size() != 1 || r2l_ls_record.begin()->second != 1) ? 1000 : 0;
  for (const auto& kv : r2l_ls_record) {
    const std::string sfx = "_epi_kernel";
    if (kv.first.size() < sfx.size() || kv.first.compare(kv.first.size() - sfx.size(), sfx.size(), sfx)) {
      bad += 1000;
      fprintf(stderr, "launched %s x %d\n", kv.first.c_str(), kv.second);
    }
  }
  return bad;
}

// the plain call once, then the three moves (hflip, vflip, both; every other case spells one of them with k = 2)
static int run_case(int B, int H, int W, int debayer, int sharpening, int denoising, int frames, int io, bool norm, int n) {
  const size_t px = (size_t)B * H * W, esz = io == R2L_IO_F32 ? 4 : 2;
  Block rawb(px * raw_bytes(frames));
  fill_raw(lcg01, rawb.p, px, frames, 0.02f, 0.9f);
  const float* ms = norm ? MEAN_STD : nullptr;
  Block plain(3 * px * esz);
  int e = r2l_static_fwd_io(rawb.p, frames, 65535.f, plain.p, io, B, H, W, CAMERA, debayer, sharpening, denoising, 2.2, nullptr, ms, nullptr, 0,
                            nullptr);
  if (e) return fprintf(stderr, "plain call -> %d: %s\n", e, r2l_last_error()), 1;
  static const int moves[3][2] = {{1, 0}, {0, 1}, {1, 1}};
  int rc = 0;
  for (int m = 0; m < 3; ++m) {
    const int hflip = moves[m][0], vflip = moves[m][1];
    // rot90^2 = both flips: the same permutation spelt with k = 2 on every other case
    const bool k2 = ((n + m) & 1) != 0;
    const int bits = k2 ? epi_bits(!hflip, !vflip, 2) : epi_bits(hflip, vflip, 0);
    if (const char* why = r2l_static_epilogue_supported(frames, H, W, debayer, sharpening, denoising, nullptr, io, bits))
      return fprintf(stderr, "not served: %s\n", why), 1;
    Block out(3 * px * esz);
    record_begin();
    e = r2l_static_fwd_epilogue(rawb.p, frames, 65535.f, out.p, io, B, H, W, CAMERA, debayer, sharpening, denoising, 2.2, nullptr, ms, nullptr, 0,
                                nullptr, bits);
    r2l_ls_record_on = false;
    if (e) return fprintf(stderr, "epilogue call -> %d: %s\n", e, r2l_last_error()), 1;
    long bad = record_is_one_epi_launch();
    for (int p = 0; p < 3 * B; ++p)
      for (int r = 0; r < H; ++r)
        for (int c = 0; c < W; ++c) {
          int r2, c2;
          r2l_aug_map(H, W, hflip, vflip, 0, r, c, r2, c2);
          const size_t src = ((size_t)p * H + r) * W + c, dst = ((size_t)p * H + r2) * W + c2;
          if (memcmp(out.p + dst * esz, plain.p + src * esz, esz) && bad++ < 5)
            fprintf(stderr, "plane %d: pixel (%d, %d) is not at (%d, %d)\n", p, r, c, r2, c2);
        }
    printf("%dx%dx%d debayer %d sharpening %d denoising %d frames %d io %d norm %d hflip %d vflip %d%s: %ld mismatches\n", B, H, W, debayer,
           sharpening, denoising, frames, io, (int)norm, hflip, vflip, k2 ? " (k = 2)" : "", bad);
    rc |= bad != 0;
  }
  return rc;
}

int main() {
  static const int shapes[3][3] = {{1, 6, 80}, {1, 10, 260}, {1, 4, 4}};
  // the short chain (r2l_static_stream.h) and the luma chain (r2l_static_chain.h: its Gaussian and its median store site)
  static const int chains[3][2] = {{R2L_SHARPEN_NONE, R2L_DENOISE_NONE}, {R2L_SHARPEN_FILTER, R2L_DENOISE_GAUSSIAN},
                                   {R2L_SHARPEN_FILTER, R2L_DENOISE_MEDIAN}};
  int rc = 0, n = 0;
  for (const auto& s : shapes)
    for (const auto& c : chains)
      for (int deb = R2L_DEBAYER_BILINEAR; deb <= R2L_DEBAYER_MALVAR2004; ++deb)
        for (int frames = R2L_FRAMES_F32; frames <= R2L_FRAMES_U16; ++frames)
          for (int io = R2L_IO_F32; io <= R2L_IO_F16; ++io, ++n) rc |= run_case(s[0], s[1], s[2], deb, c[0], c[1], frames, io, (n % 3) == 1, n);
  // two images (the batch stride), and behind unsharp_masking (the 7-row chroma ring)
  rc |= run_case(2, 10, 260, R2L_DEBAYER_MALVAR2004, R2L_SHARPEN_NONE, R2L_DENOISE_NONE, R2L_FRAMES_F32, R2L_IO_F32, false, 0);
  rc |= run_case(2, 10, 260, R2L_DEBAYER_BILINEAR, R2L_SHARPEN_FILTER, R2L_DENOISE_GAUSSIAN, R2L_FRAMES_U16, R2L_IO_BF16, true, 1);
  rc |= run_case(1, 10, 260, R2L_DEBAYER_BILINEAR, R2L_SHARPEN_UNSHARP, R2L_DENOISE_GAUSSIAN, R2L_FRAMES_F32, R2L_IO_F16, false, 0);
  // what the call refuses: -3 with the reason, nothing written; unknown bits -1; no epilogue: r2l_static_fwd_io
  {
    const int B = 1, H = 8, W = 8;
    Buf<float> raw((size_t)H * W);
    for (size_t i = 0; i < raw.n; ++i) raw.p[i] = 0.02f + 0.9f * lcg01();
    Buf<double> raw64((size_t)H * W);
    for (size_t i = 0; i < raw64.n; ++i) raw64.p[i] = raw.p[i];
    Buf<float> o((size_t)3 * H * W), want((size_t)3 * H * W);
    struct { int frames, deb, sh, dn, bits; const char* word; } no[] = {
        {R2L_FRAMES_F32, 0, 0, 0, epi_bits(0, 0, 1), "k odd"},
        {R2L_FRAMES_F32, 0, R2L_SHARPEN_FILTER, R2L_DENOISE_GAUSSIAN, epi_bits(1, 1, 3), "k odd"},
        {R2L_FRAMES_F64, 0, 0, 0, epi_bits(1, 0, 0), "float64"},
        {R2L_FRAMES_F32, R2L_DEBAYER_MENON2007, 0, 0, epi_bits(0, 1, 0), "menon2007"},
        {R2L_FRAMES_F32, 0, R2L_SHARPEN_FILTER, R2L_DENOISE_FFT, epi_bits(1, 0, 0), "fft_denoising"}};
    for (const auto& q : no) {
      const void* r = q.frames == R2L_FRAMES_F64 ? (const void*)raw64.p : (const void*)raw.p;
      const char* why = r2l_static_epilogue_supported(q.frames, H, W, q.deb, q.sh, q.dn, nullptr, R2L_IO_F32, q.bits);
      if (!why || !strstr(why, q.word)) rc |= 1, fprintf(stderr, "%s: the predicate says %s\n", q.word, why ? why : "(served)");
      Block ws(1 << 16);
      const int e = r2l_static_fwd_epilogue(r, q.frames, 1.f, o.p, R2L_IO_F32, B, H, W, CAMERA, q.deb, q.sh, q.dn, 2.2, nullptr, nullptr, ws.p,
                                            1 << 16, nullptr, q.bits);
      if (e != -3 || !strstr(r2l_last_error(), q.word)) rc |= 1, fprintf(stderr, "%s must return -3 with the reason, got %d\n", q.word, e);
      for (size_t i = 0; i < o.n; ++i)
        if (r2l_f2u(o.p[i]) != 0xffffffffu) rc |= 1;
    }
    if (r2l_static_fwd_epilogue(raw.p, R2L_FRAMES_F32, 1.f, o.p, R2L_IO_F32, B, H, W, CAMERA, 0, 0, 0, 2.2, nullptr, nullptr, nullptr, 0, nullptr,
                                R2L_STEP_EPI_HFLIP | 8) != -1)
      rc |= 1, fprintf(stderr, "bits outside R2L_STEP_EPI_* must return -1\n");
    record_begin();
    int e = r2l_static_fwd_epilogue(raw.p, R2L_FRAMES_F32, 1.f, o.p, R2L_IO_F32, B, H, W, CAMERA, 0, R2L_SHARPEN_FILTER, R2L_DENOISE_GAUSSIAN, 2.2,
                                    nullptr, nullptr, nullptr, 0, nullptr, 0);
    r2l_ls_record_on = false;
    e |= r2l_static_fwd_io(raw.p, R2L_FRAMES_F32, 1.f, want.p, R2L_IO_F32, B, H, W, CAMERA, 0, R2L_SHARPEN_FILTER, R2L_DENOISE_GAUSSIAN, 2.2, nullptr,
                           nullptr, nullptr, 0, nullptr);
    if (e || memcmp(o.p, want.p, o.n * sizeof(float)) || r2l_ls_record.size() != 1 || !r2l_ls_record.count("r2l_launch_static_chain_kernel"))
      rc |= 1, fprintf(stderr, "epilogue = 0 must be r2l_static_fwd_io\n");
  }
  return rc;
}
