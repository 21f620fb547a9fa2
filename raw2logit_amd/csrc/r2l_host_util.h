// r2l_host_util.h -- host helpers that both the step and the static chains use: grid sizing, the environment overrides of
// diagnostic builds, the workspace carve, the checks of shapes and frames, the output epilogue's map.
#pragma once
#include <stdlib.h>

#include <string>

#include "r2l_launch.h"
#include "r2l_param_kernels.h"
#include "r2l_staged_kernels.h"

// ---- grid sizing ------------------------------------------------------------------------------
static_assert(R2L_MAX_BLOCKS == 2048 && 1 + R2L_MAX_GROUPS <= R2L_NT, "partials / arrival counters are laid out for at most 2048 workgroups");
// Launch shapes are compile-time choices of the product build.  Diagnostic builds (-DR2L_TEST_HOOKS: the host
// emulation and tests/_build/libr2l_isp_hooks.so, never the shipped libr2l_isp.so) can override them through the
// environment -- that is how the tests show that no result depends on the workgroup count, and how A/B runs sweep
// band heights.
#ifdef R2L_TEST_HOOKS
static int r2l_env_int(const char* name, int dflt) {
  const char* s = getenv(name);
  if (!s || !*s) return dflt;
  const int v = atoi(s);
  return v > 0 ? v : dflt;
}
#else
static inline int r2l_env_int(const char*, int dflt) { return dflt; }
#endif
// the flat grid-stride kernels (staged path, raw2rgb, the weak augmentation's permutation): min(computed grid, R2L_GRID_FLAT)
// in diagnostic builds, so that their second and later passes run at small shapes; the computed grid in the product build
static int r2l_flat_grid(size_t g) {
  const size_t cap = (size_t)r2l_env_int("R2L_GRID_FLAT", 0x7fffffff);
  if (g > cap) g = cap;
  return g < 1 ? 1 : (int)g;
}
// persistent tile-walking kernels: at most `cap` workgroups (256 CUs x resident workgroups per CU),
// a multiple of 8 when possible so that the XCD-grouped walk applies
static int r2l_tile_grid(int ntiles, int cap) {
  if (cap > R2L_MAX_BLOCKS) cap = R2L_MAX_BLOCKS;
  int g = ntiles < cap ? ntiles : cap;
  if (g >= 8) g -= g % 8;
  return g < 1 ? 1 : g;
}

// Band height of the plane passes (r2l_param_stream.h, r2l_param_plane_bwd.h): a multiple of 6 rows (bands start on
// multiples of 6: the ring slot of a row is the unroll position of its step), the one that needs the fewest rounds of
// `slots` resident wavefronts x the rows a wavefront walks (+ 4 load-only warm-up steps + its start) -- 64x512x512 apply
// pass: 24 rows = 2,816 wavefronts, one round at 3 per SIMD (65 us; 18 rows: 68.5; 12: 67.5; 36: 71.5,
// profiles/r03_apply_kept.txt; re-swept under the progress-priority build, profiles/r04_bands.txt); 64x256x256: 6 rows.
// `env`: override of diagnostic builds.
static int r2l_band_rows(int B, int H, int W, long slots, const char* env) {
  const long nstrip = (W + 255) / 256;
  int bh = 6;
  long best = -1;
  for (int c = 6; c <= 48; c += 6) {
    const long items = (long)B * nstrip * ((H + c - 1) / c);
    const long cost = ((items + slots - 1) / slots) * (10L * c + 32);
    if (best < 0 || cost < best) {
      best = cost;
      bh = c;
    }
  }
  return (r2l_env_int(env, bh) + 5) / 6 * 6;
}
// Work items of a plane pass -- one per (image, 256-column strip, band of band_h rows) -- and its workgroups: nwv items in
// flight per workgroup, at most `cap` workgroups and R2L_MAX_BLOCKS (the partials of the reduction trees); cap = 0: a pass
// without partials, one workgroup per nwv items
static long r2l_plane_items(int B, int H, int W, int band_h) {
  return (long)B * ((W + 255) / 256) * ((H + band_h - 1) / band_h);
}
static int r2l_plane_grid(int B, int H, int W, int band_h, int nwv, long cap) {
  long g = (r2l_plane_items(B, H, W, band_h) + nwv - 1) / nwv;
  if (cap && g > cap) g = cap;
  if (cap && g > R2L_MAX_BLOCKS) g = R2L_MAX_BLOCKS;
  return (int)g;
}

// ---- workspace ----------------------------------------------------------------------------------
struct R2LWorkspace {
  R2LFolded* folded;
  float* part_b1;
  float* part_b2;
  float* part_small;
  double* sums;
  double* gpartial;    // [R2L_MAX_GROUPS][R2L_NSUMS] group partials of the in-kernel final reductions
  unsigned* counters;  // [1 + R2L_MAX_GROUPS] arrival counters: zeroed by the fold kernel, zero after every launch
  float* gypp;
  float* yp;     // (B,H,W): the sharpened luma Y' of the forward, for kernel B1 (R2L_F_KEEP_LUMA)
  float* hp;     // (B,H,W): the blur's adjoint of dL/dY'' (plane passes of kernel B2, r2l_param_plane_bwd.h)
  float* debug;  // 3 x [R2L_MAX_BLOCKS][8] floats: per-phase cycle stamps of diagnostic builds (fwd, bwd1, bwd2)
  // step block (r2l_isp_step_fwd / _bwd): what one training step keeps between its launches
  float* packed;    // [R2L_P_COUNT] the parameter values the forward saw
  float* bn;        // [6] mean, istd
  float* bn_bwd;    // [6] mean(g), mean(g * xhat)
  double* stats;    // [7] this rank's statistics sums (+ pixel count)
  double* moments;  // [7] mean, biased var, pixel count of the global batch
  double* bsums;    // [6] this rank's BatchNorm backward sums
  size_t total;
};
static size_t r2l_align_up(size_t x) { return (x + 255) & ~(size_t)255; }
static R2LWorkspace r2l_carve(void* base, int B, int H, int W) {
  R2LWorkspace w;
  size_t off = 0;
  char* p = (char*)base;
  w.folded = (R2LFolded*)(p + off);
  off += r2l_align_up(sizeof(R2LFolded));
  w.part_b1 = (float*)(p + off);
  off += r2l_align_up(sizeof(float) * R2L_B1_NACC * R2L_MAX_BLOCKS);
  w.part_b2 = (float*)(p + off);
  off += r2l_align_up(sizeof(float) * R2L_B2_NACC * R2L_MAX_BLOCKS);
  w.part_small = (float*)(p + off);
  off += r2l_align_up(sizeof(float) * 12 * R2L_MAX_BLOCKS);
  w.sums = (double*)(p + off);
  off += r2l_align_up(sizeof(double) * R2L_NSUMS);
  w.gpartial = (double*)(p + off);
  off += r2l_align_up(sizeof(double) * R2L_NSUMS * R2L_MAX_GROUPS);
  w.counters = (unsigned*)(p + off);
  off += r2l_align_up(sizeof(unsigned) * (1 + R2L_MAX_GROUPS));
  w.debug = (float*)(p + off);
#ifdef R2L_EXP_STAMPS
  off += r2l_align_up(sizeof(float) * 4 * 8 * R2L_MAX_BLOCKS);  // + the wavefront placement records (tests/timeline_fwd.py)
#else
  off += r2l_align_up(sizeof(float) * 3 * 8 * R2L_MAX_BLOCKS);
#endif
  w.packed = (float*)(p + off);
  off += r2l_align_up(sizeof(float) * R2L_P_COUNT);
  w.bn = (float*)(p + off);
  w.bn_bwd = w.bn + 8;
  off += r2l_align_up(sizeof(float) * 16);
  w.stats = (double*)(p + off);
  w.moments = w.stats + 8;
  w.bsums = w.stats + 16;
  off += r2l_align_up(sizeof(double) * 24);
  w.gypp = (float*)(p + off);
  off += r2l_align_up(sizeof(float) * (size_t)B * H * W);
  w.yp = (float*)(p + off);
  off += r2l_align_up(sizeof(float) * (size_t)B * H * W);
  w.hp = (float*)(p + off);
  off += r2l_align_up(sizeof(float) * (size_t)B * H * W);
  w.total = off;
  return w;
}

static int r2l_check_dims(int B, int H, int W) {
  if (B < 1) return r2l_fail(-1, "B must be >= 1");
  if (H < 4 || W < 4 || (H & 1) || (W & 1))
    return r2l_fail(-1, "H and W must be even and >= 4 (Bayer quads; 5x5 mirror padding)");
  if ((size_t)H * W > ((size_t)1 << 29)) return r2l_fail(-1, "frames above 2^29 pixels are not supported");
  if ((size_t)B * H * W > ((size_t)1 << 40)) return r2l_fail(-1, "batch too large");
  return 0;
}

static int r2l_check_raw(const R2LRaw& raw, int W, const char* who) {
  if (!raw.f32 && !raw.u16 && !raw.f64) return r2l_fail(-1, std::string(who) + ": null pointer");
  if (raw.f64 && (W & 3)) return r2l_fail(-4, std::string(who) + ": float64 frames need W % 4 == 0");
  if (raw.u16 && !(raw.denom >= 1.f)) return r2l_fail(-1, std::string(who) + ": denom must be >= 1 (2**bits - 1)");
  if (raw.u16 && (W & 3)) return r2l_fail(-1, std::string(who) + ": 16-bit frames need W % 4 == 0");
  return 0;
}

// the output epilogue travels in the bits of `phase` above R2L_STEP_KEEP_LUMA (R2L_STEP_EPI_*); the affine map of
// R2LEpi follows from r2l_aug_map, the definition the stand-alone permutation kernel (r2l_augment) uses
#define R2L_STEP_EPI_MASK (R2L_STEP_EPI_HFLIP | R2L_STEP_EPI_VFLIP | (3 << R2L_STEP_EPI_ROT_SHIFT))
static int r2l_epi_from_phase(int phase, int H, int W, R2LEpi& ep) {
  const int hflip = (phase & R2L_STEP_EPI_HFLIP) != 0, vflip = (phase & R2L_STEP_EPI_VFLIP) != 0;
  const int k = (phase >> R2L_STEP_EPI_ROT_SHIFT) & 3;
  ep = R2LEpi{0, 0, 0, 0};
  if (!(hflip || vflip || k)) return 0;
  if ((k & 1) && H != W) return r2l_fail(-1, "output epilogue: a rotation by 90 degrees needs square frames");
  const int Wo = (k & 1) ? H : W;
  int r0, c0, r1, c1, r2, c2;
  r2l_aug_map(H, W, hflip, vflip, k, 0, 0, r0, c0);
  r2l_aug_map(H, W, hflip, vflip, k, 1, 0, r1, c1);
  r2l_aug_map(H, W, hflip, vflip, k, 0, 1, r2, c2);
  ep.on = 1;
  ep.s0 = r0 * Wo + c0;
  ep.sr = (r1 * Wo + c1) - ep.s0;
  ep.sc = (r2 * Wo + c2) - ep.s0;
  return 0;
}
static R2LRaw r2l_raw_any(const void* raw, int raw_u16, float denom) {
  return raw_u16 ? r2l_raw_u16((const unsigned short*)raw, denom) : r2l_raw_f32((const float*)raw);
}
