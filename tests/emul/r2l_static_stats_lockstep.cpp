// r2l_static_stats_lockstep.cpp -- stand-alone program (own main, no Python) of the static chains' statistics kernels
// (r2l_static_stats) and of r2l_channel_sums in their DEVICE forms on the CPU: the lock-step emulation's sources (r2l_lockstep.cpp,
// unchanged) under -fsanitize=address,undefined.  TEST INFRASTRUCTURE: built and run by tests/test_static_stats.py with the flags
// and the dependency list of tests/lockstep_driver.py.  (A second build of the emulation's sources beside r2l_lockstep_drivers:
// to be folded into that program.)
// Every buffer is a heap block of exactly the size the C ABI names -- the frames, sums[7], the workspace of
// r2l_static_stats_workspace_bytes -- so that a load or a partial that strays is an ASan report.
//   check 1: constant frames (8.0; full containers read as 12-bit) under the identity camera: every output value is exactly 1.0,
//            all seven sums must equal B * H * W exactly;
//   check 2: random frames under the Drone camera: sums against long-double sums of the float32 call's output, within
//            (n - 1) * 2^-53 * sum|t| (any summation order of exactly representable terms);
//   routes : the launch record holds one ..._stats kernel and the finishing launch; unserved calls return -3 and write nothing.
#define R2L_TEST_HOOKS 1
#include "r2l_lockstep.cpp"

#include "r2l_driver_util.h"

#include <math.h>

using namespace r2l_drv;

static Lcg lcg01{97531u};
// black level 0, white balance 1, identity colour matrix (oracle/isp_oracle.py: DEFAULT_CAMERA_PARAMS)
static const double IDENTITY[16] = {0, 0, 0, 0, 1, 1, 1, 1, 0, 0, 0, 1, 0, 0, 0, 1};

static bool record_is_stats_and_finish() {
  bool stats = false, finish = false;
  for (const auto& kv : r2l_ls_record) {
    const std::string sfx = "_stats_kernel";
    if (kv.first == "r2l_launch_sums_finish_kernel" && kv.second == 1) finish = true;
    else if (kv.first.size() > sfx.size() && !kv.first.compare(kv.first.size() - sfx.size(), sfx.size(), sfx) && kv.second == 1) stats = true;
    else fprintf(stderr, "launched %s x %d\n", kv.first.c_str(), kv.second);
  }
  return stats && finish && r2l_ls_record.size() == 2;
}

static int stats_call(const void* raw, int frames, float denom, double* sums, int B, int H, int W, const double* cam, int deb, int sh, int dn) {
  if (const char* why = r2l_static_stats_supported(frames, H, W, deb, sh, dn, nullptr)) return fprintf(stderr, "not served: %s\n", why), 1;
  const size_t nws = r2l_static_stats_workspace_bytes(frames, B, H, W, deb, sh, dn, nullptr);
  if (!nws) return fprintf(stderr, "no workspace?\n"), 1;
  Block ws(nws);
  // one byte short: -2, nothing launched
  if (r2l_static_stats(raw, frames, denom, sums, B, H, W, cam, deb, sh, dn, 2.2, nullptr, ws.p, nws - 1, nullptr) != -2)
    return fprintf(stderr, "a workspace one byte short must return -2\n"), 1;
  record_begin();
  const int e = r2l_static_stats(raw, frames, denom, sums, B, H, W, cam, deb, sh, dn, 2.2, nullptr, ws.p, nws, nullptr);
  r2l_ls_record_on = false;
  if (e) return fprintf(stderr, "r2l_static_stats -> %d: %s\n", e, r2l_last_error()), 1;
  return record_is_stats_and_finish() ? 0 : (fprintf(stderr, "launch record\n"), 1);
}

static int run_case(int B, int H, int W, int deb, int sh, int dn, int frames) {
  const size_t px = (size_t)B * H * W;
  long bad = 0;
  Buf<double> sums(7);
  {  // check 1
    Block rawb(px * raw_bytes(frames));
    for (size_t i = 0; i < px; ++i) {
      if (frames == R2L_FRAMES_U16) ((unsigned short*)rawb.p)[i] = 65535;
      else if (frames == R2L_FRAMES_F64) ((double*)rawb.p)[i] = 8.0;
      else ((float*)rawb.p)[i] = 8.0f;
    }
    if (stats_call(rawb.p, frames, 4095.f, sums.p, B, H, W, IDENTITY, deb, sh, dn)) return 1;
    for (int k = 0; k < 7; ++k)
      if (sums.p[k] != (double)px && bad++ < 7) fprintf(stderr, "constant frames: sums[%d] = %.17g, want %zu\n", k, sums.p[k], px);
  }
  {  // check 2
    Block rawb(px * raw_bytes(frames));
    fill_raw(lcg01, rawb.p, px, frames, 0.02f, 0.9f);
    Buf<float> out(3 * px);
    const int e = r2l_static_fwd_io(rawb.p, frames, 65535.f, out.p, R2L_IO_F32, B, H, W, CAMERA, deb, sh, dn, 2.2, nullptr, nullptr, nullptr, 0,
                                    nullptr);
    if (e) return fprintf(stderr, "float32 call -> %d: %s\n", e, r2l_last_error()), 1;
    if (stats_call(rawb.p, frames, 65535.f, sums.p, B, H, W, CAMERA, deb, sh, dn)) return 1;
    if (sums.p[6] != (double)px) ++bad, fprintf(stderr, "sums[6] = %.17g\n", sums.p[6]);
    const long double u = (long double)(px - 1) * ldexpl(1.0L, -53);
    bool inside = false, clipped = false;
    for (int k = 0; k < 3; ++k) {
      long double s1 = 0, s2 = 0, sa = 0;
      for (size_t b = 0; b < (size_t)B; ++b)
        for (size_t i = 0; i < (size_t)H * W; ++i) {
          const long double v = out.p[(b * 3 + k) * (size_t)H * W + i];
          s1 += v, s2 += v * v, sa += fabsl(v);
          inside |= v > 0 && v < 1;
          clipped |= v == 0 || v == 1;
        }
      // (the long-double reference sums carry their own rounding, 2^-64 per addition: 2^-11 of the limit)
      const long double slack = (long double)px * ldexpl(1.0L, -64);
      if (fabsl((long double)sums.p[k] - s1) > u * sa + slack * sa && bad++ < 7) fprintf(stderr, "sum[%d] %.17g, want %.17Lg\n", k, sums.p[k], s1);
      if (fabsl((long double)sums.p[3 + k] - s2) > u * s2 + slack * s2 && bad++ < 7) fprintf(stderr, "sumsq[%d] %.17g, want %.17Lg\n", k, sums.p[3 + k], s2);
    }
    if (!(inside && clipped)) ++bad, fprintf(stderr, "the frames must reach both sides of the clip\n");
    // check 5: a second call, the same 56 bytes
    Buf<double> again(7);
    if (stats_call(rawb.p, frames, 65535.f, again.p, B, H, W, CAMERA, deb, sh, dn)) return 1;
    if (memcmp(again.p, sums.p, 56)) ++bad, fprintf(stderr, "a second call gave other bits\n");
  }
  printf("%dx%dx%d debayer %d sharpening %d denoising %d frames %d: %ld mismatches\n", B, H, W, deb, sh, dn, frames, bad);
  return bad ? 1 : 0;
}

// r2l_channel_sums on a tensor that starts `shift` floats behind a 16-byte boundary
static int run_channel_sums(int B, int C, int H, int W, int shift) {
  const size_t n = (size_t)B * C * H * W;
  float* block = nullptr;
  if (posix_memalign((void**)&block, 16, (n + shift) * sizeof(float))) return 1;
  float* x = block + shift;
  for (size_t i = 0; i < n; ++i) x[i] = 2.f * lcg01() - 0.5f;
  const size_t nws = r2l_channel_sums_workspace_bytes(B, C, H, W);
  Block ws(nws);
  Buf<double> sums(2 * C + 1);
  long bad = 0;
  if (r2l_channel_sums(x, sums.p, B, C, H, W, ws.p, nws - 1, nullptr) != -2) ++bad, fprintf(stderr, "workspace one byte short must return -2\n");
  const int e = r2l_channel_sums(x, sums.p, B, C, H, W, ws.p, nws, nullptr);
  if (e) return fprintf(stderr, "r2l_channel_sums -> %d: %s\n", e, r2l_last_error()), free(block), 1;
  const size_t hw = (size_t)H * W, px = (size_t)B * hw;
  const long double u = (long double)(px - 1) * ldexpl(1.0L, -53) + (long double)px * ldexpl(1.0L, -64);
  for (int c = 0; c < C; ++c) {
    long double s1 = 0, s2 = 0, sa = 0;
    for (size_t b = 0; b < (size_t)B; ++b)
      for (size_t i = 0; i < hw; ++i) {
        const long double v = x[(b * C + c) * hw + i];
        s1 += v, s2 += v * v, sa += fabsl(v);
      }
    if (fabsl((long double)sums.p[c] - s1) > u * sa && bad++ < 7) fprintf(stderr, "sum[%d] %.17g, want %.17Lg\n", c, sums.p[c], s1);
    if (fabsl((long double)sums.p[C + c] - s2) > u * s2 && bad++ < 7) fprintf(stderr, "sumsq[%d] %.17g, want %.17Lg\n", c, sums.p[C + c], s2);
  }
  if (sums.p[2 * C] != (double)px) ++bad;
  printf("channel_sums %dx%dx%dx%d shift %d: %ld mismatches\n", B, C, H, W, shift, bad);
  free(block);
  return bad ? 1 : 0;
}

int main() {
  static const int shapes[3][3] = {{1, 6, 80}, {1, 10, 260}, {1, 4, 4}};
  static const int chains[3][2] = {{R2L_SHARPEN_NONE, R2L_DENOISE_NONE}, {R2L_SHARPEN_FILTER, R2L_DENOISE_GAUSSIAN},
                                   {R2L_SHARPEN_FILTER, R2L_DENOISE_MEDIAN}};
  int rc = 0;
  for (const auto& s : shapes)
    for (const auto& c : chains)
      for (int deb = R2L_DEBAYER_BILINEAR; deb <= R2L_DEBAYER_MALVAR2004; ++deb)
        for (int frames = R2L_FRAMES_F32; frames <= R2L_FRAMES_F64; ++frames) {
          if (frames == R2L_FRAMES_F64 && c[0] != R2L_SHARPEN_NONE) continue;  // float64 frames: the short chain only
          rc |= run_case(s[0], s[1], s[2], deb, c[0], c[1], frames);
        }
  // two batches of bands per workgroup and a batch of 2 (R2L_GRID_STATIC caps the statistics launches of this diagnostic build)
  setenv("R2L_GRID_STATIC", "1", 1);
  rc |= run_case(2, 10, 260, R2L_DEBAYER_BILINEAR, R2L_SHARPEN_NONE, R2L_DENOISE_NONE, R2L_FRAMES_F32);
  rc |= run_case(2, 10, 260, R2L_DEBAYER_MALVAR2004, R2L_SHARPEN_FILTER, R2L_DENOISE_GAUSSIAN, R2L_FRAMES_U16);
  unsetenv("R2L_GRID_STATIC");
  // behind unsharp_masking (bilinear: the statistics form's float32 raw window)
  rc |= run_case(1, 10, 260, R2L_DEBAYER_BILINEAR, R2L_SHARPEN_UNSHARP, R2L_DENOISE_GAUSSIAN, R2L_FRAMES_F32);
  rc |= run_case(1, 10, 260, R2L_DEBAYER_BILINEAR, R2L_SHARPEN_UNSHARP, R2L_DENOISE_MEDIAN, R2L_FRAMES_U16);
  rc |= run_channel_sums(3, 1, 1, 1, 0);
  rc |= run_channel_sums(2, 3, 35, 67, 0);
  rc |= run_channel_sums(1, 4, 35, 66, 1);
  rc |= run_channel_sums(2, 3, 70, 260, 3);
  // what the call refuses: -3 with the reason, nothing written; null pointers -1
  {
    Buf<float> raw(4 * 8);
    for (size_t i = 0; i < raw.n; ++i) raw.p[i] = 0.5f;
    Buf<double> sums(7);
    Block ws(1024);
    for (int k = 0; k < 7; ++k) sums.p[k] = 7.0;
    const int e = r2l_static_stats(raw.p, R2L_FRAMES_F32, 1.f, sums.p, 1, 4, 8, CAMERA, R2L_DEBAYER_MENON2007, 0, 0, 2.2, nullptr, ws.p, 1024, nullptr);
    if (e != -3 || !strstr(r2l_last_error(), "menon2007")) rc |= 1, fprintf(stderr, "Menon2007 must return -3 with the reason\n");
    for (int k = 0; k < 7; ++k)
      if (sums.p[k] != 7.0) rc |= 1;
    if (r2l_static_stats(raw.p, R2L_FRAMES_F32, 1.f, nullptr, 1, 4, 8, CAMERA, 0, 0, 0, 2.2, nullptr, ws.p, 1024, nullptr) != -1)
      rc |= 1, fprintf(stderr, "sums = NULL must return -1\n");
    if (r2l_static_stats(raw.p, R2L_FRAMES_F32, 1.f, sums.p, 1, 4, 8, CAMERA, 0, 0, R2L_DENOISE_FFT + 1, 2.2, nullptr, ws.p, 1024, nullptr) != -4)
      rc |= 1, fprintf(stderr, "an unknown denoising must return -4\n");
  }
  return rc;
}
