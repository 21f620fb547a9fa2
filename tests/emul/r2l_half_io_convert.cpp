// r2l_half_io_convert.cpp -- stand-alone check of the 16-bit conversion helpers of raw2logit_amd/csrc/r2l_common.h in their
// HOST forms (the emulation builds' integer arithmetic).  TEST INFRASTRUCTURE: built and run by tests/test_half_io.py, which
// writes the expected values from torch's Tensor.to(dtype) into the file this program reads.
//   file layout (little endian): uint32 n, then n records of (uint32 float32 pattern, uint16 bfloat16 pattern, uint16 float16
//   pattern) for the narrowings; then 65536 uint32 float32 patterns of the widened bfloat16 values, then 65536 of the float16 ones.
// NaN: a NaN must stay a NaN (of any payload); everything else is compared bit for bit.
#define R2L_EMUL 1
#ifdef R2L_CONVERT_LOCKSTEP
#define R2L_LOCKSTEP 1
#endif
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../../raw2logit_amd/csrc/r2l_common.h"

static bool is_nan32(unsigned u) { return (u & 0x7fffffffu) > 0x7f800000u; }
static bool is_nan_bf16(unsigned h) { return (h & 0x7fffu) > 0x7f80u; }
static bool is_nan_f16(unsigned h) { return (h & 0x7fffu) > 0x7c00u; }

int main(int argc, char** argv) {
  if (argc != 2) {
    fprintf(stderr, "usage: %s expected.bin\n", argv[0]);
    return 2;
  }
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  unsigned n = 0;
  if (fread(&n, 4, 1, f) != 1) return 2;
  struct Rec {
    unsigned f32;
    unsigned short bf16, f16;
  };
  static_assert(sizeof(Rec) == 8, "record layout");
  std::vector<Rec> recs(n);
  if (fread(recs.data(), sizeof(Rec), n, f) != n) return 2;
  std::vector<unsigned> wb(65536), wh(65536);
  if (fread(wb.data(), 4, 65536, f) != 65536 || fread(wh.data(), 4, 65536, f) != 65536) return 2;
  fclose(f);
  long bad = 0;
  for (unsigned i = 0; i < n; ++i) {
    const float x = r2l_u2f(recs[i].f32);
    const unsigned b = r2l_f32_to_bf16_bits(x), h = r2l_f32_to_f16_bits(x);
    const bool okb = is_nan32(recs[i].f32) ? (is_nan_bf16(b) && is_nan_bf16(recs[i].bf16)) : b == recs[i].bf16;
    const bool okh = is_nan32(recs[i].f32) ? (is_nan_f16(h) && is_nan_f16(recs[i].f16)) : h == recs[i].f16;
    if ((!okb || !okh) && bad++ < 10)
      fprintf(stderr, "narrow %08x: bf16 %04x (torch %04x) f16 %04x (torch %04x)\n", recs[i].f32, b, recs[i].bf16, h, recs[i].f16);
    // the packed form is the scalar one, four times
    if ((i & 3) == 3) {
      r2l_f4 v;
      v.x = r2l_u2f(recs[i - 3].f32);
      v.y = r2l_u2f(recs[i - 2].f32);
      v.z = r2l_u2f(recs[i - 1].f32);
      v.w = x;
      const r2l_h4 pb = r2l_io_narrow4<R2L_IO_BF16>(v), ph = r2l_io_narrow4<R2L_IO_F16>(v);
      const bool okp = pb.lo == (r2l_f32_to_bf16_bits(v.x) | (r2l_f32_to_bf16_bits(v.y) << 16)) &&
                       pb.hi == (r2l_f32_to_bf16_bits(v.z) | (b << 16)) &&
                       ph.lo == (r2l_f32_to_f16_bits(v.x) | (r2l_f32_to_f16_bits(v.y) << 16)) &&
                       ph.hi == (r2l_f32_to_f16_bits(v.z) | (h << 16));
      const r2l_f4 back = r2l_io_widen4<R2L_IO_F16>(ph);
      const bool okw = r2l_f2u(back.w) == r2l_f2u(r2l_f16_bits_to_f32(h)) && r2l_f2u(back.x) == r2l_f2u(r2l_f16_bits_to_f32(ph.lo & 0xffffu));
      if ((!okp || !okw) && bad++ < 10) fprintf(stderr, "packed form differs at record %u\n", i);
    }
  }
  for (unsigned p = 0; p < 65536; ++p) {
    const unsigned a = r2l_f2u(r2l_bf16_bits_to_f32(p)), c = r2l_f2u(r2l_f16_bits_to_f32(p));
    const bool oka = is_nan_bf16(p) ? (is_nan32(a) && is_nan32(wb[p])) : a == wb[p];
    const bool okc = is_nan_f16(p) ? (is_nan32(c) && is_nan32(wh[p])) : c == wh[p];
    if ((!oka || !okc) && bad++ < 10) fprintf(stderr, "widen %04x: bf16 %08x (torch %08x) f16 %08x (torch %08x)\n", p, a, wb[p], c, wh[p]);
    // a 16-bit value survives the round trip
    if (!is_nan_bf16(p) && r2l_f32_to_bf16_bits(r2l_u2f(a)) != p && bad++ < 10) fprintf(stderr, "bf16 round trip %04x\n", p);
    if (!is_nan_f16(p) && r2l_f32_to_f16_bits(r2l_u2f(c)) != p && bad++ < 10) fprintf(stderr, "f16 round trip %04x\n", p);
  }
  printf("checked %u narrowings, 2 x 65536 widenings: %ld mismatches\n", n, bad);
  return bad ? 1 : 0;
}
