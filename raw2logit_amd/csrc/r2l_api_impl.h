// r2l_api_impl.h -- the C ABI of include/r2l_isp.h, written once.
//
// Included by r2l_api.hip (hipcc, gfx950: launches real kernels on a HIP stream) and by
// tests/emul/r2l_emul.cpp (g++, R2L_EMUL: runs the same workgroup programs on host memory, for the
// CPU-only test suite).
#pragma once
#include "r2l_launch.h"
#include "r2l_kernels_step.h"
#include "r2l_kernels_static.h"
#include "r2l_kernels_rest.h"
#include "r2l_host_util.h"

extern "C" {

size_t r2l_isp_workspace_bytes(int B, int H, int W) {
  if (B < 1 || H < 1 || W < 1) return 0;
  return r2l_carve(nullptr, B, H, W).total;
}

// ---- the forward: one plan, one launcher ----------------------------------------------------------------------------------
// where the row-streaming forward (r2l_param_stream.h) runs -- and with R2L_F_KEEP_LUMA leaves Y' for kernel B1
static bool r2l_fwd_streams(bool additive, int W) {
  return R2L_PLANE_PASSES && !additive && (W & 3) == 0 && W <= 2048 && !r2l_env_int("R2L_FWD_TILED", 0);
}
// which pass of a step a forward is: a whole forward (every public r2l_isp_fwd*; the step's without train-mode BatchNorm), the
// statistics pass of train mode, or its apply pass -- the workspace's Y' plane is then this batch's, left by the statistics pass
enum { R2L_FWD_WHOLE, R2L_FWD_STATS_PASS, R2L_FWD_APPLY_PASS };
// what a forward works on
struct R2LFwdCall {
  R2LRaw raw;
  const float *params, *additive, *bn;
  float* out;     // elements of type io; null: the statistics alone
  double* stats;  // or null
  const R2LBnFinalizeArgs* fin;  // or null; one rank: the last workgroup also does the BatchNorm bookkeeping
  R2LEpi ep;
  int io;    // what `out` really holds (R2L_IO_* | R2L_IO_NHWC; r2l_io_check has seen that the streaming kernels serve the call)
  int pass;  // R2L_FWD_*
  int B, H, W;
  void* stream;
};
enum { R2L_FWD_STREAM, R2L_FWD_STREAM_STATS, R2L_FWD_SPLIT_STATS, R2L_FWD_APPLY, R2L_FWD_TILES };
enum { R2L_FWD_TILE_EXACT, R2L_FWD_TILE_RAGGED, R2L_FWD_TILE_ADD };
enum { R2L_YP_NONE, R2L_YP_WRITE, R2L_YP_READ };
// the work items of one launch: bands of band_h rows (0: a tile kernel), nitems of them in all, on `grid` workgroups
struct R2LPass {
  int band_h, nband, nitems, grid;
};
// What a forward launches, decided from the shape of the call alone (r2l_fwd_plan): r2l_fwd_launch walks it
struct R2LFwdPlan {
  int route;       // R2L_FWD_STREAM: the row-streaming kernel; _STREAM_STATS: its statistics-only instantiation; _SPLIT_STATS: luma
                   // pass + statistics from the plane; _APPLY: the apply pass on the kept Y'; _TILES: the tile kernels
  int tile;        // R2L_FWD_TILE_*
  int nw;          // wavefronts side by side per row: 1 << nw (the column of r2l_fwd_stream_table)
  int yp;          // R2L_YP_*: what the route's (last) launch does with the workspace's Y' plane
  bool epi;        // the output goes through the epilogue
  bool too_large;  // a pass counts more work items than an int holds
  R2LPass luma, main;  // the luma pass of R2L_FWD_SPLIT_STATS; the route's one or last launch
};
// a plane pass (r2l_param_stream.h, r2l_param_plane_bwd.h): independent wavefronts, one per (image, band, 256-column strip); band
// height: r2l_band_rows for `slots` resident wavefronts; nwv items in flight per workgroup, at most `cap` workgroups (r2l_plane_grid)
static R2LPass r2l_plane_pass(int B, int H, int W, long slots, const char* band_env, int nwv, long cap, bool& too_large) {
  R2LPass p;
  p.band_h = r2l_band_rows(B, H, W, slots, band_env);
  p.nband = (H + p.band_h - 1) / p.band_h;
  const long items = r2l_plane_items(B, H, W, p.band_h);
  too_large = too_large || items > (1L << 30);
  p.nitems = (int)items;
  p.grid = r2l_plane_grid(B, H, W, p.band_h, nwv, cap);
  return p;
}
// The only reader of the forward's overrides of diagnostic builds (R2L_FORCE_SPLIT, R2L_FWD_*, R2L_GRID_FWD, the band heights;
// R2L_FWD_TILED: r2l_fwd_streams).  has_out: after R2L_F_STATS_ONLY
static R2LFwdPlan r2l_fwd_plan(int pass, bool has_out, bool has_stats, bool additive, bool keep_luma, bool epi_on, int B, int H,
                               int W) {
  R2LFwdPlan p = {};
  p.epi = epi_on && has_out;
#ifndef R2L_SERIAL
  if (r2l_fwd_streams(additive, W)) {
    // (diagnostic builds, tests/timeline_fwd.py: every call as both passes of a step)
    const bool force = r2l_env_int("R2L_FORCE_SPLIT", 0) != 0;
    const bool stats_pass = force || pass == R2L_FWD_STATS_PASS, apply_pass = force || pass == R2L_FWD_APPLY_PASS;
    // row-streaming forward: work item = (image, band of rows); short bands are cheap here (the 8 halo rows of a
    // band only compute their luma), so aim at ~2048 items (three wavefronts per SIMD: the kernel's row step is a
    // chain of scalar-load waits, which only other wavefronts can fill), bands of >= 16 rows
    p.nw = W <= 256 ? 0 : (W <= 512 ? 1 : (W <= 1024 ? 2 : 3));
    // one round of resident workgroups: 256 CUs x 12 wavefronts (three per SIMD) / wavefronts per workgroup
    const long resident = 256L * (12 >> p.nw);
    const int fs_band = r2l_env_int("R2L_FS_BAND", 0);
    long nband = fs_band ? (H + fs_band - 1) / fs_band : resident / B;
    if (nband > H / R2L_FS_MINBAND) nband = H / R2L_FS_MINBAND;
    if (nband < 1) nband = 1;
    R2LPass fs;
    fs.band_h = (int)((H + nband - 1) / nband);
    fs.band_h += fs.band_h & 1;
    fs.nband = (H + fs.band_h - 1) / fs.band_h;
    const long nitems = (long)B * fs.nband;
    p.too_large = nitems > (1L << 30);  // (counted on every route of a frame that streams)
    fs.nitems = (int)nitems;
    long cap = r2l_env_int("R2L_GRID_FWD", (int)(resident < R2L_MAX_BLOCKS ? resident : R2L_MAX_BLOCKS));
    if (cap > R2L_MAX_BLOCKS) cap = R2L_MAX_BLOCKS;
    fs.grid = (int)(nitems < cap ? nitems : cap);
    // The passes on the kept luma plane (r2l_fwd_luma_block, r2l_fwd_apply_block): r2l_plane_pass
    const bool kept_ok = !r2l_env_int("R2L_FWD_APPLY_RECOMPUTE", 0);
    // statistics pass = luma pass + statistics from the plane, where that is faster than the streaming forward without
    // output: frames one strip wide (64x256x256: 12 + 26 us against 46; 128x256x256: 17 + 36 against 61).  On 512-wide
    // frames the two kernels issue as many vector instructions as the one (7.1 M + 15.9 M against 23.9 M at 64x512x512)
    // and take as long (28.5 + 55 us against 79.7): profiles/r03_split_stats.txt
    const bool split = r2l_env_int("R2L_FWD_STATS_SPLIT", 0) || (W <= 256 && !r2l_env_int("R2L_FWD_STATS_STREAM", 0));
    if (!has_out && has_stats && stats_pass && kept_ok && split) {
      p.route = R2L_FWD_SPLIT_STATS;
      p.yp = R2L_YP_READ;
      p.luma = r2l_plane_pass(B, H, W, 256L * 4 * R2L_FL_OCC, "R2L_FL_BAND", R2L_FA_NWV, 0, p.too_large);
      // (<= R2L_MAX_BLOCKS workgroups = partials of the reduction tree)
      p.main = r2l_plane_pass(B, H, W, 256L * 4 * R2L_FA_STATS_OCC, "R2L_FST_BAND", R2L_FA_STATS_NWV,
                              r2l_env_int("R2L_GRID_FWD", R2L_MAX_BLOCKS), p.too_large);
    } else if (has_out && !has_stats && apply_pass && kept_ok) {
      p.route = R2L_FWD_APPLY;
      p.yp = R2L_YP_READ;
      p.main = r2l_plane_pass(B, H, W, 256L * 4 * R2L_FA_OCC, "R2L_FA_BAND", R2L_FA_NWV, 0, p.too_large);
    } else {
      // the statistics alone: the kernel's own instantiation (no output code, fewer live scalars)
      p.route = (!has_out && has_stats) ? R2L_FWD_STREAM_STATS : R2L_FWD_STREAM;
      // (a statistics pass of the streaming kernel keeps Y' too: for kernel B1 and for the apply pass)
      p.yp = (keep_luma || stats_pass) ? R2L_YP_WRITE : R2L_YP_NONE;
      p.main = fs;
    }
    return p;
  }
#endif
  p.route = R2L_FWD_TILES;
  // (an additive layer means 256 x 256 frames: they tile exactly)
  const bool exact = (H % GFwd::TH == 0) && (W % GFwd::TW == 0);
  p.tile = additive ? R2L_FWD_TILE_ADD : (exact ? R2L_FWD_TILE_EXACT : R2L_FWD_TILE_RAGGED);
  const int ntiles = B * ((H + GFwd::TH - 1) / GFwd::TH) * ((W + GFwd::TW - 1) / GFwd::TW);
  p.main.grid = r2l_tile_grid(ntiles, r2l_env_int("R2L_GRID_FWD", 512));
  return p;
}
#ifndef R2L_SERIAL
// the argument block of the streaming kernel and of every plane pass (luma, statistics from the plane, apply; the backward's
// BatchNorm sums) over `pass`: no output, no Y' plane, no epilogue; sums: its partials go through the workspace's reduction tree
// (the arrival counters are valid: this call or an earlier one on this workspace ran the fold kernel)
static R2LFwdStreamArgs r2l_fwd_stream_args(const R2LRaw& raw, const R2LWorkspace& ws, const float* bn, int B, int H, int W,
                                            const R2LPass& pass, bool sums) {
  R2LFwdStreamArgs a;
  a.raw = raw;
  a.F = ws.folded;
  a.bn = bn;
  a.out = nullptr;
  a.yp_out = nullptr;
  a.yp_in = nullptr;
#ifdef R2L_EXP_STAMPS
  a.tl = nullptr;
#endif
  a.stat_partial = sums ? ws.part_small : nullptr;
  a.B = B;
  a.H = H;
  a.W = W;
  a.band_h = pass.band_h;
  a.nband = pass.nband;
  a.nitems = pass.nitems;
  a.tree = R2LTree{ws.part_small, nullptr, ws.gpartial, sums ? ws.counters : nullptr, 12, 0};
  a.stats_out = nullptr;
  a.fin.bn = nullptr;
  a.ep = R2LEpi{0, 0, 0, 0};
  return a;
}
#endif
// The launches of plan `p` = r2l_fwd_plan(this call), in order.  The workspace's folded weights and arrival counters are valid
static int r2l_fwd_launch(const R2LFwdCall& c, const R2LWorkspace& ws, const R2LFwdPlan& p) {
  const int u16 = c.raw.u16 ? 1 : 0;
  const R2LEpi ep = p.epi ? c.ep : R2LEpi{0, 0, 0, 0};
#ifndef R2L_SERIAL
  if (p.route != R2L_FWD_TILES) {
    R2LFwdStreamArgs fa = r2l_fwd_stream_args(c.raw, ws, c.bn, c.B, c.H, c.W, p.main, c.stats != nullptr);
    fa.out = c.out;
    fa.yp_out = p.yp == R2L_YP_WRITE ? ws.yp : nullptr;
    fa.yp_in = p.yp == R2L_YP_READ ? ws.yp : nullptr;
    fa.stats_out = c.stats;
    if (c.fin) fa.fin = *c.fin;
    fa.ep = ep;
#ifdef R2L_EXP_STAMPS  // (tests/timeline_fwd.py: the streaming kernel on request, each plane pass in its own third)
    if (p.route == R2L_FWD_APPLY) fa.tl = (unsigned long long*)ws.debug + 16384;
    else if (p.route == R2L_FWD_SPLIT_STATS) fa.tl = (unsigned long long*)ws.debug + 8192;
    else if (r2l_env_int("R2L_TL_STREAM", 0)) fa.tl = (unsigned long long*)ws.debug;
#endif
    switch (p.route) {
      case R2L_FWD_SPLIT_STATS: {
        R2LFwdStreamArgs la = fa;  // raw -> Y'
        la.yp_out = ws.yp;
        la.yp_in = nullptr;
        la.stat_partial = nullptr;
        la.band_h = p.luma.band_h;
        la.nband = p.luma.nband;
        la.nitems = p.luma.nitems;
#ifdef R2L_EXP_STAMPS
        la.tl = (unsigned long long*)ws.debug;
#endif
        if (int e = u16 ? r2l_launch_fwd_luma_u16(la, p.luma.grid, c.stream) : r2l_launch_fwd_luma(la, p.luma.grid, c.stream)) return e;
        return u16 ? r2l_launch_fwd_stats_u16(fa, p.main.grid, c.stream) : r2l_launch_fwd_stats(fa, p.main.grid, c.stream);
      }
      case R2L_FWD_APPLY:
        return r2l_fwd_apply_table[c.io != R2L_IO_F32 ? R2L_PAIR_IO + r2l_io_slot(c.io) : (p.epi ? R2L_PAIR_EPI : R2L_PAIR_PLAIN)][u16](
            fa, p.main.grid, c.stream);
      case R2L_FWD_STREAM_STATS:
        return r2l_fwd_stream_table[R2L_FS_STATS][u16][p.nw](fa, p.main.grid, c.stream);
      default:
        return r2l_fwd_stream_table[c.io != R2L_IO_F32 ? R2L_FS_IO + r2l_io_slot(c.io) : (p.epi ? R2L_FS_EPI : R2L_FS_PLAIN)][u16][p.nw](
            fa, p.main.grid, c.stream);
    }
  }
#endif
  // the tile kernels
  if (p.epi && c.additive) return r2l_fail(-3, "r2l_isp_fwd: no output epilogue with an additive layer");
  R2LFwdArgs a;
  a.raw = c.raw;
  a.additive = c.additive;
  a.F = ws.folded;
  a.bn = c.bn;
  a.out = c.out;
  a.stat_partial = c.stats ? ws.part_small : nullptr;
  a.B = c.B;
  a.H = c.H;
  a.W = c.W;
  a.debug = ws.debug;
  // the statistics are reduced by the last workgroups of the same launch
  a.tree = R2LTree{ws.part_small, nullptr, ws.gpartial, c.stats ? ws.counters : nullptr, 12, 0};
  a.stats_out = c.stats;
  if (c.fin)
    a.fin = *c.fin;
  else
    a.fin.bn = nullptr;
  a.ep = ep;
  typedef int (*launch_t)(const R2LFwdArgs&, int, void*);
  static const launch_t tile[3][2] = {{r2l_launch_fwd, r2l_launch_fwd_u16},
                                      {r2l_launch_fwd_ragged, r2l_launch_fwd_ragged_u16},
                                      {r2l_launch_fwd_add_exact, r2l_launch_fwd_add_exact_u16}};
  return tile[p.tile][u16](a, p.main.grid, c.stream);
}
// validate, carve, fold if needed, plan, launch.  flags: the public R2L_F_* bits (others are ignored)
static int r2l_isp_fwd_impl(R2LFwdCall c, int flags, void* workspace, size_t workspace_bytes) {
  const int B = c.B, H = c.H, W = c.W;
  if (int e = r2l_check_dims(B, H, W)) return e;
  if (int e = r2l_check_raw(c.raw, W, "r2l_isp_fwd")) return e;
  if (c.io != R2L_IO_F32 && (!r2l_fwd_streams(c.additive, W) || c.ep.on))
    return r2l_fail(-3, "r2l_isp_fwd: internal: a 16-bit / channels-last output needs the row-streaming forward without an epilogue");
  if (!c.params || !workspace) return r2l_fail(-1, "r2l_isp_fwd: null pointer");
  if (c.additive && (H != 256 || W != 256))
    return r2l_fail(-1, "additive_layer is (1,3,256,256): needs 256x256 frames");
  if (flags & R2L_F_STATS_ONLY) c.out = nullptr;
  if (!c.out && !c.stats) return r2l_fail(-1, "r2l_isp_fwd: nothing to compute (no out, no stats)");
  const R2LWorkspace ws = r2l_carve(workspace, B, H, W);
  if (workspace_bytes < ws.total) return r2l_fail(-2, "r2l_isp_fwd: workspace too small");
  if (!(flags & R2L_F_FOLDED_VALID)) {
    R2LFoldArgs fa{c.params, ws.folded, ws.counters};
    if (int e = r2l_launch_fold(fa, 1, c.stream)) return e;
  }
  const R2LFwdPlan p = r2l_fwd_plan(c.pass, c.out != nullptr, c.stats != nullptr, c.additive != nullptr,
                                    (flags & R2L_F_KEEP_LUMA) != 0, c.ep.on != 0, B, H, W);
  if (p.too_large) return r2l_fail(-1, "r2l_isp_fwd: batch too large");
  return r2l_fwd_launch(c, ws, p);
}

int r2l_bn_finalize(const double* stats, int nranks, float* bn_mean_istd, double* moments, float* running_mean,
                    float* running_var, long long* num_batches_tracked, double eps, double momentum,
                    void* stream) {
  const double* totals = stats;
  if (!totals || !bn_mean_istd || nranks < 1) return r2l_fail(-1, "r2l_bn_finalize: null pointer / nranks < 1");
  if ((running_mean == nullptr) != (running_var == nullptr))
    return r2l_fail(-1, "r2l_bn_finalize: running_mean and running_var go together");
  R2LBnFinalizeArgs a{totals, nranks, bn_mean_istd, moments, running_mean, running_var, eps, momentum,
                      num_batches_tracked};
  return r2l_launch_bn_finalize(a, 1, stream);
}

int r2l_bn_bwd_means(const double* gathered_sums, int nranks, const double* n, float* bn_bwd, void* stream) {
  if (!gathered_sums || !n || !bn_bwd || nranks < 1) return r2l_fail(-1, "r2l_bn_bwd_means: null pointer / nranks < 1");
  R2LBnBwdMeansArgs a{gathered_sums, nranks, n, bn_bwd};
  return r2l_launch_bn_bwd_means(a, 1, stream);
}

int r2l_bn_bwd_reduce(const float* grad_out, const float* out, const double* totals, double* sums,
                      float* bn_bwd, void* workspace, size_t workspace_bytes, int B, int H, int W, int flags,
                      void* stream) {
  if (int e = r2l_check_dims(B, H, W)) return e;
  if (!grad_out || !out || !sums || !workspace) return r2l_fail(-1, "r2l_bn_bwd_reduce: null pointer");
  if (bn_bwd && !totals) return r2l_fail(-1, "r2l_bn_bwd_reduce: bn_bwd needs totals (the pixel count)");
  const R2LWorkspace ws = r2l_carve(workspace, B, H, W);
  if (workspace_bytes < ws.total) return r2l_fail(-2, "r2l_bn_bwd_reduce: workspace too small");
  const size_t hw = (size_t)H * W;
  const size_t nitems = (size_t)3 * B * ((hw + R2L_SEG - 1) / R2L_SEG);
  const int cap = r2l_tile_grid(R2L_MAX_BLOCKS, r2l_env_int("R2L_GRID_BNR", 512));
  int grid = nitems < (size_t)cap ? (int)nitems : cap;
  // a workspace that went through r2l_isp_fwd / r2l_isp_bwd has valid arrival counters: the last workgroups
  // of the launch finish the reduction; otherwise a second, tiny launch does
  const bool in_kernel = (flags & R2L_F_FOLDED_VALID) != 0;
  R2LBnReduceArgs a{grad_out, out, ws.part_small, B, H, W,
                    R2LTree{ws.part_small, nullptr, ws.gpartial, in_kernel ? ws.counters : nullptr, 6, 0},
                    sums, totals, bn_bwd};
  if (int e = r2l_launch_bn_reduce(a, grid, stream)) return e;
  if (in_kernel) return 0;
  R2LReduceRowsArgs r{ws.part_small, sums, grid, 1.0, bn_bwd, nullptr, 0.0, bn_bwd ? totals + 6 : nullptr};
  return r2l_launch_reduce_rows(r, 6, stream);
}

// ---- the backward: one plan, one launcher ---------------------------------------------------------------------------------
// kernel B1 as a tile kernel (which instantiation), as the plane passes, or as a reduced plane pass (R2LBwdPlan::select)
enum { R2L_B1_TILE_SAVED, R2L_B1_TILE_ADD, R2L_B1_TILE_EXACT, R2L_B1_TILE_RAGGED, R2L_B1_PLANES };
// What a backward launches, decided from the shape of the call alone (r2l_bwd_plan): r2l_bwd_launch walks it, and
// r2l_isp_step_bwd_select_passes reports its `select`
struct R2LBwdPlan {
  int select;           // R2L_SELECT_FULL: every sum; else the R2L_SELECT_* bits of the reduced passes that run
  int b1;               // R2L_B1_*
  bool saved;           // kernel B1 reads the Y' the forward kept
  bool b2_planes;       // kernel B2 as plane passes (the blur's adjoint HP, then the sums) instead of the tile kernel
  bool blur_hp;         // the blur-weight sums and HP in one pass (r2l_bwd1_blur_hp_block)
  bool in_kernel;       // the last workgroups of kernel B2 reduce and unfold; else three tiny launches do
  int b1_grid, b1_band;  // kernel B1 (band heights: 0 for a tile kernel); b1_grid workgroups write its partials
  int hb_band;           // the blur / blur + HP pass, on kernel B1's grid
  int hp_grid, hp_band;  // the HP pass alone
  int b2_grid, b2_band, b2_nmain;  // kernel B2: the tile kernel, or the sums pass (b2_nmain workgroups + R2L_B2S_HELPERS)
  int raw_grid, raw_band;          // the d/d raw gather pass
  bool bnr;                        // train-mode BatchNorm's backward sums are recomputed from raw + Y' (r2l_bnr_planes_block)
  int bnr_grid, bnr_band;          // ... instead of read back from the saved output (r2l_bn_bwd_reduce)
};
// grad_mask: the R2L_GRAD_* bits a caller of r2l_isp_step_bwd_select asks for, 0 = every parameter gradient; want_raw: d/d raw too.
// The only reader of the backward's overrides of diagnostic builds (R2L_BWD_*, R2L_GRID_BWD*, the band heights).
// io16: grad_out is bfloat16 / float16 or channels-last (r2l_isp_step_bwd_io, _layout) -- read by the plane passes only, which such
// a call therefore takes at every size, on the full route whatever the mask
static R2LBwdPlan r2l_bwd_plan(unsigned grad_mask, bool want_raw, int raw_u16, bool has_additive, bool epi_on,
                               bool keep_luma, int B, int H, int W, bool io16 = false) {
  R2LBwdPlan p = {};
  if (io16) grad_mask = 0;
  const bool want_raw_mask = want_raw;  // (the reduced routes' own condition below)
  want_raw = want_raw || io16;          // "the plane passes at every size, no diagnostic override"
  // (the serial emulation has no row-streaming forward, so nothing is ever saved there and every plan is tile kernels)
  p.saved = keep_luma && r2l_fwd_streams(has_additive, W) && (want_raw || !r2l_env_int("R2L_BWD1_RECOMPUTE", 0));
  // frames that do not tile by 64: Y' recomputed in LDS, kept or not; an additive layer means 256 x 256 frames, which tile exactly
  const bool exact = (H % GBwd1::TH == 0) && (W % GBwd1::TW == 0);
  p.b1 = (p.saved && exact) ? R2L_B1_TILE_SAVED
                            : (has_additive ? R2L_B1_TILE_ADD : (exact ? R2L_B1_TILE_EXACT : R2L_B1_TILE_RAGGED));
#ifndef R2L_SERIAL
  // The plane passes where there is enough work for their launch tails: 128x256x256 (8.4 Mpx) 102 us against the tile kernels'
  // 110+, 64x256x256 (4.2 Mpx) 77.7 against 80.5 since the tails were shortened (profiles/r04_small.txt; round 3: 99 against 85,
  // and the threshold was 6 Mi px)
  // (d/d raw: the plane passes at every size -- the gather pass reads the planes they leave)
  // (R2L_BWD_PLANES of diagnostic builds: the plane passes, and the recomputing BatchNorm sums, below their pixel thresholds too)
  const bool forced = r2l_env_int("R2L_BWD_PLANES", 0) != 0;
  const bool planes = want_raw || forced || (size_t)B * H * W >= ((size_t)4 << 20);
  const bool b1_planes = p.saved && planes && (want_raw || !r2l_env_int("R2L_BWD1_TILED", 0));
  p.b2_planes = b1_planes && (want_raw || !r2l_env_int("R2L_BWD2_TILED", 0));
  // The reduced passes: the sums of the black level, white balance, colour matrix, debayer and sharpen gradients need the whole
  // chain; the reduced forms exist as plane passes only
  // (16-bit frames and an output epilogue have no d/d raw -- r2l_raw_grad_preconditions refuses them before a call gets here, the
  // query reports the full route for them)
  const unsigned cheap = R2L_GRAD_GAMMA | R2L_GRAD_BLUR | R2L_GRAD_RAW;
  const bool gam = (grad_mask & R2L_GRAD_GAMMA) != 0, blur = (grad_mask & R2L_GRAD_BLUR) != 0;
  if (grad_mask && !(grad_mask & ~cheap) && p.b2_planes && !(want_raw && (raw_u16 || epi_on))) {
    p.select = R2L_SELECT_B1 | (want_raw ? R2L_SELECT_RAW : 0);
    if (blur) p.select |= want_raw ? R2L_SELECT_BLUR_HP : R2L_SELECT_BLUR;
    else if (want_raw) p.select |= R2L_SELECT_HP;
  }
  auto band_rows = [&](long slots, const char* env) { return r2l_band_rows(B, H, W, slots, env); };
  if (b1_planes) {
    // persistent workgroups of 4 independent wavefronts, `occ` per CU (the full pass: two, <= 256 VGPRs), not more workgroups
    // than kernel B2 runs (its last workgroups reduce both kernels' partials); band height as for the forward's plane passes
    const int occ = !p.select ? 2 : ((want_raw && !gam) ? R2L_BPS_OCC_RAW : R2L_BPS_OCC);
    p.b1 = R2L_B1_PLANES;
    p.b1_band = band_rows(256L * 4 * occ, "R2L_BP_BAND");
    p.b1_grid = r2l_plane_grid(B, H, W, p.b1_band, R2L_BP_NWV, r2l_env_int("R2L_GRID_BWD1", 256 * occ));
    // its second pass (the blur-weight sums) and kernel B2's first (the blur's adjoint) read the same plane: one pass when B2
    // runs as plane passes too.  Its own band height: R2L_HB_OCC wavefronts per SIMD; not more workgroups than wrote the first
    // pass's partials
    p.blur_hp = p.select ? (p.select & R2L_SELECT_BLUR_HP) != 0 : (p.b2_planes && !r2l_env_int("R2L_BWD_SPLIT_BLUR", 0));
    p.hb_band = band_rows(256L * 4 * R2L_HB_OCC, "R2L_HB_BAND");
  }
  if (p.select ? (p.select & R2L_SELECT_HP) != 0 : (p.b2_planes && !p.blur_hp)) {
    p.hp_band = band_rows(256L * 4 * 4, "R2L_HP_BAND");
    p.hp_grid = r2l_plane_grid(B, H, W, p.hp_band, R2L_BP_NWV, 0);
  }
  if (p.b2_planes && !p.select) {
    // the sums pass: its last workgroups reduce B2's partials; R2L_B2S_HELPERS more workgroups (the grid leaves room for them
    // beside one round of the others) add B1's meanwhile; the last arrival of all unfolds the 155 totals into the 132 gradients
    p.b2_band = band_rows(256L * 4 * 3, "R2L_B2S_BAND");
    p.b2_nmain = r2l_plane_grid(B, H, W, p.b2_band, R2L_B2S_NWV, r2l_env_int("R2L_GRID_BWD2", 768));  // 3 workgroups per CU
    p.b2_grid = p.b2_nmain + R2L_B2S_HELPERS;
    p.in_kernel = true;
  }
  if (want_raw_mask && p.b2_planes) {  // d/d raw from HP and the chroma gradient planes: one item per wavefront
    p.raw_band = band_rows(256L * 4 * R2L_BR_OCC, "R2L_BR_BAND");
    p.raw_grid = r2l_plane_grid(B, H, W, p.raw_band, R2L_BR_NWV, 0);
  }
  // BatchNorm's backward sums of a step whose forward kept Y' (R2L_F_KEEP_LUMA on the row-streaming path): recomputed from the raw
  // frame and Y' on batches of >= 6 Mi px -- the forward's output is then not read at all by the backward
  // (from 6 Mi px: at 64x256x256 = 4 Mi px the whole step, output included, lives in the memory-side cache and reading the output back
  //  is cheaper than recomputing it -- bn_reduce 22.4-23.8 us against 27.1; at 128x256x256 37.2 against 37.5, the step 2 % faster)
  // A 16-bit / channels-last cotangent is read by this pass only, at every size (without an epilogue)
  p.bnr = keep_luma && r2l_fwd_streams(has_additive, W) && (io16 ? !epi_on : (forced || (size_t)B * H * W >= ((size_t)6 << 20)));
  if (p.bnr) {
    // (band height as kernel B1's: 36 rows at 64x512x512 -- 61.4 us against 63.2 at 24 rows, 71-73 at 12 / 18 / 30, 68.4 at 48)
    p.bnr_band = band_rows(256L * 4 * 2, "R2L_BNR_BAND");
    p.bnr_grid = r2l_plane_grid(B, H, W, p.bnr_band, R2L_BNR_NWV, r2l_env_int("R2L_GRID_BNR", R2L_MAX_BLOCKS));
  }
#endif
  if (p.b1 != R2L_B1_PLANES) {
    const int ntiles = B * ((H + GBwd1::TH - 1) / GBwd1::TH) * ((W + GBwd1::TW - 1) / GBwd1::TW);
    p.b1_grid = r2l_tile_grid(ntiles, r2l_env_int("R2L_GRID_BWD1", 256));
  }
  if (!p.b2_planes) {
    // bwd2 fits two workgroups per CU (<= 128 VGPRs, 68 KB of LDS): 512 workgroups.  Its last workgroups reduce both kernels'
    // partials (B1's were written by b1_grid workgroups: every level-1 group of B2's grid adds the B1 partials of its own 16
    // workgroup ids, as far as they exist) and unfold them into the 132 gradients; if B1 ran MORE workgroups than B2 (R2L_GRID_*
    // overrides of diagnostic builds) three tiny launches do it
    const int ntiles = B * ((H + GBwd2::TH - 1) / GBwd2::TH) * ((W + GBwd2::TW - 1) / GBwd2::TW);
    p.b2_grid = r2l_tile_grid(ntiles, r2l_env_int("R2L_GRID_BWD2", R2L_OCC_BWD2 >= 4 ? 512 : 256));
    p.in_kernel = p.b1_grid <= p.b2_grid;
  }
  return p;
}
int r2l_isp_step_bwd_select_passes(unsigned grad_mask, int raw_u16, int has_additive, int B, int H, int W, int phase) {
  if (B < 1 || H < 1 || W < 1) return R2L_SELECT_FULL;
  return r2l_bwd_plan(grad_mask, (grad_mask & R2L_GRAD_RAW) != 0, raw_u16, has_additive != 0, (phase & R2L_STEP_EPI_MASK) != 0,
                      (phase & R2L_STEP_KEEP_LUMA) != 0, B, H, W)
      .select;
}
// what a backward works on; the workspace holds the folded weights of `params` (and, behind a step's forward, Y')
struct R2LBwdCall {
  R2LRaw raw;
  const float *params, *additive, *bn, *bn_bwd, *gout;
  float *grad_params, *grad_raw, *guv;  // guv: the chroma gradient planes, with grad_raw
  R2LEpi ep;
  unsigned grad_mask;  // r2l_bwd_plan's
  int B, H, W;
  void* stream;
  int io;  // the type behind gout (R2L_IO_*)
};
static R2LBwd1Args r2l_bwd1_args(const R2LBwdCall& c, const R2LWorkspace& ws, const R2LBwdPlan& p) {
  R2LBwd1Args a;
  a.raw = c.raw;
  a.additive = c.additive;
  a.F = ws.folded;
  a.bn = c.bn;
  a.bn_bwd = c.bn_bwd;
  a.gout = c.gout;
  a.gypp = ws.gypp;
  a.partial = ws.part_b1;
  a.B = c.B;
  a.H = c.H;
  a.W = c.W;
  a.debug = ws.debug + 8 * R2L_MAX_BLOCKS;
  a.yp = p.saved ? ws.yp : nullptr;
  a.ep = c.ep;
  a.band_h = p.b1_band;
  a.hp = p.b1 == R2L_B1_PLANES ? ws.hp : nullptr;
  a.band_hb = p.hb_band;
  return a;
}
// (as the HP pass takes them: no sums, no reduction)
static R2LBwd2Args r2l_bwd2_args(const R2LBwdCall& c, const R2LWorkspace& ws, const R2LBwdPlan& p) {
  R2LBwd2Args a;
  a.raw = c.raw;
  a.F = ws.folded;
  a.gypp = ws.gypp;
  a.partial = ws.part_b2;
  a.B = c.B;
  a.H = c.H;
  a.W = c.W;
  a.debug = ws.debug + 16 * R2L_MAX_BLOCKS;
  a.tree = R2LTree{nullptr, nullptr, nullptr, nullptr, 0, 0};
  a.params = nullptr;
  a.grad_params = nullptr;
  a.hp = p.b2_planes ? ws.hp : nullptr;
  a.band_h = p.hp_band;
  a.nmain = 0;
  a.b1_partial = nullptr;
  a.b1_n = 0;
  a.b1_tot = nullptr;
  return a;
}
#ifndef R2L_SERIAL
static int r2l_bwd_hp_pass(const R2LBwdCall& c, const R2LWorkspace& ws, const R2LBwdPlan& p) {
  return r2l_launch_bwd2_hp(r2l_bwd2_args(c, ws, p), p.hp_grid, c.stream);
}
static int r2l_bwd_raw_pass(const R2LBwdCall& c, const R2LWorkspace& ws, const R2LBwdPlan& p) {
  if (r2l_plane_items(c.B, c.H, c.W, p.raw_band) > (1L << 30)) return r2l_fail(-1, "r2l_isp_step_bwd_raw: batch too large");
  const R2LRawGradArgs a{ws.folded, ws.hp, c.guv, c.grad_raw, c.B, c.H, c.W, p.raw_band};
  return r2l_launch_bwd_raw_plane(a, p.raw_grid, c.stream);
}
// phase A of a step's backward where p.bnr: the BatchNorm sums from raw + Y' + grad_out into the workspace (means: and their means)
static int r2l_bwd_bnr_pass(const R2LBwdCall& c, const R2LWorkspace& ws, const R2LBwdPlan& p, float* means) {
  if (r2l_plane_items(c.B, c.H, c.W, p.bnr_band) > (1L << 30)) return r2l_fail(-1, "r2l_isp_step_bwd: batch too large");
  const R2LPass pass{p.bnr_band, (c.H + p.bnr_band - 1) / p.bnr_band, (int)r2l_plane_items(c.B, c.H, c.W, p.bnr_band), p.bnr_grid};
  R2LBnrArgs a;
  a.s = r2l_fwd_stream_args(c.raw, ws, ws.bn, c.B, c.H, c.W, pass, true);
  a.s.yp_in = ws.yp;
  a.s.ep = c.ep.on ? c.ep : R2LEpi{0, 0, 0, 0};
  a.gout = c.gout;
  a.sums = ws.bsums;
  a.totals = ws.moments;
  a.bn_bwd = means;
  return r2l_bnr_table[c.io != R2L_IO_F32 ? R2L_PAIR_IO + r2l_io_slot(c.io) : (c.ep.on ? R2L_PAIR_EPI : R2L_PAIR_PLAIN)][c.raw.u16 ? 1 : 0](
      a, p.bnr_grid, c.stream);
}
#endif
// The launches of plan `p` = r2l_bwd_plan(this call), in order.  The workspace's folded weights and arrival counters are valid
// (this call's fold kernel, or the step's forward)
static int r2l_bwd_launch(const R2LBwdCall& c, const R2LWorkspace& ws, const R2LBwdPlan& p) {
  if (c.ep.on && c.additive) return r2l_fail(-3, "r2l_isp_bwd: no output epilogue with an additive layer");
  // (the plane passes count their work items -- B x strips x bands -- in an int, like the forward's: the same 2^30 limit, before any launch)
  for (const int band : {p.b1_band, p.hb_band, p.hp_band, p.b2_band, p.raw_band})
    if (band > 0 && r2l_plane_items(c.B, c.H, c.W, band) > (1L << 30)) return r2l_fail(-1, "r2l_isp_step_bwd: batch too large");
  const int u16 = c.raw.u16 ? 1 : 0, g1 = p.b1_grid;
  void* const stream = c.stream;
  const R2LBwd1Args a1 = r2l_bwd1_args(c, ws, p);
  if (c.io != R2L_IO_F32 && (p.b1 != R2L_B1_PLANES || p.select || c.ep.on))
    return r2l_fail(-3, "r2l_isp_step_bwd_io: internal: a 16-bit cotangent needs the full plane route without an epilogue");
  if (p.b1 != R2L_B1_PLANES) {
    typedef int (*launch_t)(const R2LBwd1Args&, int, void*);
    static const launch_t tile[4][2] = {{r2l_launch_bwd1_saved, r2l_launch_bwd1_saved_u16},
                                        {r2l_launch_bwd1_add_exact, r2l_launch_bwd1_add_exact_u16},
                                        {r2l_launch_bwd1, r2l_launch_bwd1_u16},
                                        {r2l_launch_bwd1_ragged, r2l_launch_bwd1_ragged_u16}};
    if (int e = tile[p.b1][u16](a1, g1, stream)) return e;
  }
#ifndef R2L_SERIAL
  else if (p.select) {  // the reduced passes: behind a step's forward only (packed parameters, Y')
    const bool gam = (c.grad_mask & R2L_GRAD_GAMMA) != 0, blur = (c.grad_mask & R2L_GRAD_BLUR) != 0;
    // the gamma sum: slot R2L_B1_GGAM of kernel B1's partials, one slot through the shared tree
    R2LBwd1SelArgs sa{a1, c.guv,
                      R2LBpSelect{R2LTree{ws.part_b1 + (size_t)R2L_B1_GGAM * g1, nullptr, ws.gpartial, ws.counters, 1, 0},
                                  c.params, c.grad_params, blur}};
    typedef int (*launch_t)(const R2LBwd1SelArgs&, int, void*);
#define R2L_BPS_ROW(name) {{name, name##_u16}, {name##_epi, name##_epi_u16}}
    static const launch_t sel[3][2][2] = {R2L_BPS_ROW(r2l_launch_bwd1_sel_gamma), R2L_BPS_ROW(r2l_launch_bwd1_sel_gypp),
                                          R2L_BPS_ROW(r2l_launch_bwd1_sel_gypp_gamma)};
#undef R2L_BPS_ROW
    if (int e = c.grad_raw ? (gam ? r2l_launch_bwd1_sel_raw_gamma(sa, g1, stream) : r2l_launch_bwd1_sel_raw(sa, g1, stream))
                           : sel[!blur ? 0 : (gam ? 2 : 1)][c.ep.on ? 1 : 0][u16](sa, g1, stream))
      return e;
    if (blur) {  // the 25 sums (and HP, for d/d raw) on kernel B1's grid; its last workgroup writes the blur gradient
      sa.s.tree = R2LTree{ws.part_b1, nullptr, ws.gpartial, ws.counters, R2L_B1_GAU, 0};
      if (int e = p.blur_hp ? r2l_launch_bwd1_blur_hp_fin(sa, g1, stream) : r2l_launch_bwd1_blur_fin(sa, g1, stream)) return e;
    }
    if (!c.grad_raw) return 0;
    if (p.select & R2L_SELECT_HP)
      if (int e = r2l_bwd_hp_pass(c, ws, p)) return e;
    return r2l_bwd_raw_pass(c, ws, p);
  } else {  // kernel B1 as two passes over planes
    typedef int (*launch_t)(const R2LBwd1Args&, int, void*);
    static const launch_t plane[2][2] = {{r2l_launch_bwd1_plane, r2l_launch_bwd1_plane_u16},
                                         {r2l_launch_bwd1_plane_epi, r2l_launch_bwd1_plane_epi_u16}};
    static const launch_t plane_io[R2L_IO_SLOTS][2] = {{r2l_launch_bwd1_plane_bf16, r2l_launch_bwd1_plane_u16_bf16},
                                                       {r2l_launch_bwd1_plane_f16, r2l_launch_bwd1_plane_u16_f16},
                                                       {r2l_launch_bwd1_plane_nhwc, r2l_launch_bwd1_plane_u16_nhwc},
                                                       {r2l_launch_bwd1_plane_bf16_nhwc, r2l_launch_bwd1_plane_u16_bf16_nhwc},
                                                       {r2l_launch_bwd1_plane_f16_nhwc, r2l_launch_bwd1_plane_u16_f16_nhwc}};
    typedef int (*launch_guv_t)(const R2LBwd1GuvArgs&, int, void*);
    static const launch_guv_t guv_io[R2L_IO_SLOTS] = {r2l_launch_bwd1_plane_guv_bf16, r2l_launch_bwd1_plane_guv_f16,
                                                      r2l_launch_bwd1_plane_guv_nhwc, r2l_launch_bwd1_plane_guv_bf16_nhwc,
                                                      r2l_launch_bwd1_plane_guv_f16_nhwc};
    // (d/d raw: float32 frames, no epilogue -- r2l_raw_grad_preconditions)
    int e;
    if (c.io != R2L_IO_F32)
      e = c.grad_raw ? guv_io[r2l_io_slot(c.io)](R2LBwd1GuvArgs{a1, c.guv}, g1, stream)
                     : plane_io[r2l_io_slot(c.io)][u16](a1, g1, stream);
    else
      e = c.grad_raw ? r2l_launch_bwd1_plane_guv(R2LBwd1GuvArgs{a1, c.guv}, g1, stream)
                     : plane[c.ep.on ? 1 : 0][u16](a1, g1, stream);
    if (e) return e;
    if (int e = p.blur_hp ? r2l_launch_bwd1_blur_hp(a1, g1, stream) : r2l_launch_bwd1_blur(a1, g1, stream)) return e;
  }
#endif
  R2LBwd2Args a2 = r2l_bwd2_args(c, ws, p);
  a2.params = c.params;
  a2.grad_params = c.grad_params;
#ifndef R2L_SERIAL
  if (p.b2_planes) {  // kernel B2 as two passes over planes (r2l_param_plane_bwd.h)
    if (!p.blur_hp)
      if (int e = r2l_bwd_hp_pass(c, ws, p)) return e;
    a2.band_h = p.b2_band;
    a2.tree = R2LTree{nullptr, ws.part_b2, ws.gpartial, ws.counters, 0, 0};
    a2.nmain = p.b2_nmain;
    a2.b1_partial = ws.part_b1;
    a2.b1_n = g1;
    a2.b1_tot = ws.sums;
    if (int e = u16 ? r2l_launch_bwd2_sums_u16(a2, p.b2_grid, stream) : r2l_launch_bwd2_sums(a2, p.b2_grid, stream)) return e;
    return c.grad_raw ? r2l_bwd_raw_pass(c, ws, p) : 0;
  }
#endif
  if (c.grad_raw) return r2l_fail(-3, "r2l_isp_step_bwd_raw: internal: the plane passes did not run");
  const int g2 = p.b2_grid;
  a2.tree = R2LTree{ws.part_b1, ws.part_b2, ws.gpartial, p.in_kernel ? ws.counters : nullptr, R2L_B1_NACC, g1};
  // (even tile shares: uneven ones for the two workgroups of a CU measured no gain, profiles/r03_bwd2_tile_shares.txt)
  if (int e = u16 ? r2l_launch_bwd2_u16(a2, g2, stream) : r2l_launch_bwd2(a2, g2, stream)) return e;
  if (p.in_kernel) return 0;
  R2LReduceRowsArgs r1{ws.part_b1, ws.sums, g1, 1.0, nullptr};
  if (int e = r2l_launch_reduce_rows(r1, R2L_B1_NACC, stream)) return e;
  R2LReduceRowsArgs r2{ws.part_b2, ws.sums + R2L_B1_NACC, g2, 1.0, nullptr};
  if (int e = r2l_launch_reduce_rows(r2, R2L_B2_NACC, stream)) return e;
  R2LUnfoldArgs ua{c.params, ws.sums, c.grad_params, 1.0f};
  return r2l_launch_unfold(ua, 1, stream);
}
// r2l_isp_bwd / r2l_isp_bwd_u16: no step behind them -- the call folds the parameters itself -- and no d/d raw
static int r2l_isp_bwd_impl(const R2LRaw& raw, const float* params, const float* additive, const float* bn_mean_istd,
                            const float* bn_bwd, const float* grad_out, float* grad_params, float* grad_raw, void* workspace,
                            size_t workspace_bytes, int B, int H, int W, int flags, void* stream) {
  if (int e = r2l_check_dims(B, H, W)) return e;
  if (int e = r2l_check_raw(raw, W, "r2l_isp_bwd")) return e;
  if (!params || !grad_out || !grad_params || !workspace)
    return r2l_fail(-1, "r2l_isp_bwd: null pointer");
  if (bn_bwd && !bn_mean_istd) return r2l_fail(-1, "r2l_isp_bwd: bn_bwd given without bn_mean_istd");
  if (additive && (H != 256 || W != 256))
    return r2l_fail(-1, "additive_layer is (1,3,256,256): needs 256x256 frames");
  if (grad_raw)
    return r2l_fail(-3, "r2l_isp_bwd: grad_raw is produced by the staged path or r2l_isp_step_bwd_raw, not this call");
  const R2LWorkspace ws = r2l_carve(workspace, B, H, W);
  if (workspace_bytes < ws.total) return r2l_fail(-2, "r2l_isp_bwd: workspace too small");
  if (!(flags & R2L_F_FOLDED_VALID)) {
    R2LFoldArgs fa{params, ws.folded, ws.counters};
    if (int e = r2l_launch_fold(fa, 1, stream)) return e;
  }
  const R2LBwdCall c{raw, params, additive, bn_mean_istd, bn_bwd, grad_out, grad_params, nullptr, nullptr,
                     R2LEpi{0, 0, 0, 0}, 0, B, H, W, stream, R2L_IO_F32};
  return r2l_bwd_launch(c, ws, r2l_bwd_plan(0, false, raw.u16 != nullptr, additive != nullptr, false,
                                            (flags & R2L_F_KEEP_LUMA) != 0, B, H, W));
}

int r2l_additive_bwd(const float* grad_out, const float* out, const float* bn_mean_istd,
                     const float* bn_bwd, float* grad_additive, int B, int H, int W, void* stream) {
  if (int e = r2l_check_dims(B, H, W)) return e;
  if (!grad_out || !grad_additive) return r2l_fail(-1, "r2l_additive_bwd: null pointer");
  if (bn_mean_istd && !out) return r2l_fail(-1, "r2l_additive_bwd: BatchNorm needs the saved output");
  R2LAddBwdArgs a{grad_out, out, bn_mean_istd, bn_bwd, grad_additive, B, H, W};
  const size_t nchunk = (size_t)3 * H * W / 4;
  int grid = (int)((nchunk + R2L_NT - 1) / R2L_NT);
  if (grid > R2L_MAX_BLOCKS) grid = R2L_MAX_BLOCKS;
  return r2l_launch_add_bwd(a, grid, stream);
}

// ---- one training step in two calls (r2l_isp_step_fwd / r2l_isp_step_bwd) --------------------------------
size_t r2l_isp_step_offset(int which, int B, int H, int W) {
  if (B < 1 || H < 1 || W < 1) return 0;
  const R2LWorkspace ws = r2l_carve(nullptr, B, H, W);
  switch (which) {
    case R2L_STEP_STATS: return (size_t)((char*)ws.stats - (char*)nullptr);
    case R2L_STEP_MOMENTS: return (size_t)((char*)ws.moments - (char*)nullptr);
    case R2L_STEP_BN_SUMS: return (size_t)((char*)ws.bsums - (char*)nullptr);
    case R2L_STEP_PACKED: return (size_t)((char*)ws.packed - (char*)nullptr);
    case R2L_STEP_BN: return (size_t)((char*)ws.bn - (char*)nullptr);
    case R2L_STEP_LUMA: return (size_t)((char*)ws.yp - (char*)nullptr);
    default: return 0;
  }
}
// 16-bit and channels-last output / cotangent (include/r2l_isp.h: R2L_IO_*, R2L_LAYOUT_*)
// why a 16-bit or channels-last call is not served, or null: the ONE predicate of r2l_isp_io_supported, r2l_isp_layout_supported and
// the r2l_isp_step_{fwd,bwd}_{io,layout} calls
static const char* r2l_io_why(int raw_u16, bool has_additive, int B, int H, int W, int phase) {
  (void)raw_u16;  // (both frame types are served)
  if (!R2L_PLANE_PASSES) return "the serial emulation has no row-streaming forward and no plane passes";
  if (B < 1 || H < 4 || W < 4 || (H & 1) || (W & 1)) return "H and W must be even and >= 4, B >= 1";
  if (has_additive) return "not with an additive layer";
  if ((W & 3) || W > 2048) return "needs W % 4 == 0 and W <= 2048";
  if (r2l_env_int("R2L_FWD_TILED", 0)) return "needs the row-streaming forward (R2L_FWD_TILED is set)";
  if (phase & R2L_STEP_EPI_MASK) return "not with an output epilogue";
  if (!(phase & R2L_STEP_KEEP_LUMA)) return "needs R2L_STEP_KEEP_LUMA in `phase` of both calls";
  return nullptr;
}
// 0, or the error of a call whose `out` / `grad_out` is not planar float32.  layout = R2L_LAYOUT_NHWC is served where a 16-bit call
// is, float32 included (r2l_isp_layout_supported)
static int r2l_io_check(const char* who, int io, int layout, const void* tensor, int raw_u16, bool has_additive, int B, int H,
                        int W, int phase) {
  if (io != R2L_IO_F32 && io != R2L_IO_BF16 && io != R2L_IO_F16) return r2l_fail(-1, std::string(who) + ": io must be one of R2L_IO_*");
  if (layout != R2L_LAYOUT_NCHW && layout != R2L_LAYOUT_NHWC)
    return r2l_fail(-1, std::string(who) + ": layout must be one of R2L_LAYOUT_*");
  if (io == R2L_IO_F32 && layout == R2L_LAYOUT_NCHW) return 0;
  const bool nhwc = layout == R2L_LAYOUT_NHWC;
  if (const char* why = r2l_io_why(raw_u16, has_additive, B, H, W, phase))
    return r2l_fail(-3, std::string(who) + (nhwc ? ": a channels-last output / cotangent is not served here: "
                                                 : ": a 16-bit output / cotangent is not served here: ") + why);
  if (nhwc && io == R2L_IO_F32) {
    if ((uintptr_t)tensor % 16) return r2l_fail(-1, std::string(who) + ": the channels-last float32 tensor must be 16-byte aligned");
  } else if ((uintptr_t)tensor % 8) {
    return r2l_fail(-1, std::string(who) + ": the 16-bit tensor must be 8-byte aligned");
  }
  return 0;
}
// r2l_isp_step_fwd, r2l_isp_step_fwd_io and r2l_isp_step_fwd_layout: one implementation, what they ask of it
struct R2LStepFwd {
  const void* raw;
  int raw_u16;
  float denom;
  const float* const* params_host;
  const float* additive;
  int bn_mode;
  float *running_mean, *running_var;
  long long* num_batches_tracked;
  double eps, momentum;
  float* out;
  int io, layout;  // R2L_IO_*, R2L_LAYOUT_* as the entry got them; behind r2l_step_fwd's check io carries R2L_IO_NHWC too
  void* workspace;
  size_t workspace_bytes;
  int B, H, W, nranks, phase;
  const double* gathered_stats;
  void* stream;
};
// `who`: the entry point r2l_last_error() names where io / layout are refused
static int r2l_step_fwd(const char* who, R2LStepFwd q) {
  if (int e = r2l_io_check(who, q.io, q.layout, q.out, q.raw_u16, q.additive != nullptr, q.B, q.H, q.W, q.phase)) return e;
  if (q.layout == R2L_LAYOUT_NHWC) q.io |= R2L_IO_NHWC;
  const int B = q.B, H = q.H, W = q.W;
  const int keep = (q.phase & R2L_STEP_KEEP_LUMA) ? R2L_F_KEEP_LUMA : 0;
  R2LEpi ep;
  if (int e = r2l_check_dims(B, H, W)) return e;
  if (int e = r2l_epi_from_phase(q.phase, H, W, ep)) return e;
  const int phase = q.phase & ~(R2L_STEP_KEEP_LUMA | R2L_STEP_EPI_MASK);
  if (!q.raw || !q.out || !q.workspace) return r2l_fail(-1, "r2l_isp_step_fwd: null pointer");
  if (q.bn_mode != R2L_BN_NONE && q.bn_mode != R2L_BN_TRAIN && q.bn_mode != R2L_BN_EVAL)
    return r2l_fail(-1, "r2l_isp_step_fwd: bn_mode must be R2L_BN_NONE, R2L_BN_TRAIN or R2L_BN_EVAL");
  if (phase != R2L_STEP_ALL && phase != R2L_STEP_A && phase != R2L_STEP_B)
    return r2l_fail(-1, "r2l_isp_step_fwd: unknown phase");
  if (q.nranks < 1 || (q.nranks > 1 && phase == R2L_STEP_ALL && q.bn_mode == R2L_BN_TRAIN))
    return r2l_fail(-1, "r2l_isp_step_fwd: several ranks exchange the statistics between phase A and phase B");
  if (phase != R2L_STEP_ALL && q.bn_mode != R2L_BN_TRAIN)
    return r2l_fail(-1, "r2l_isp_step_fwd: only train-mode BatchNorm has two phases");
  if (phase == R2L_STEP_B && !q.gathered_stats) return r2l_fail(-1, "r2l_isp_step_fwd: phase B needs the gathered statistics");
  if (q.bn_mode == R2L_BN_EVAL && (!q.running_mean || !q.running_var))
    return r2l_fail(-1, "r2l_isp_step_fwd: eval-mode BatchNorm needs the running statistics");
  if ((q.running_mean == nullptr) != (q.running_var == nullptr))
    return r2l_fail(-1, "r2l_isp_step_fwd: running_mean and running_var go together");
  const R2LRaw rw = r2l_raw_any(q.raw, q.raw_u16, q.denom);
  const R2LWorkspace ws = r2l_carve(q.workspace, B, H, W);
  if (q.workspace_bytes < ws.total) return r2l_fail(-2, "r2l_isp_step_fwd: workspace too small (r2l_isp_workspace_bytes)");
  if (phase != R2L_STEP_B) {
    if (!q.params_host) return r2l_fail(-1, "r2l_isp_step_fwd: null parameter table");
    R2LPackFoldArgs pa;
    for (int i = 0; i < 9; ++i) {
      if (!q.params_host[i]) return r2l_fail(-1, "r2l_isp_step_fwd: null parameter pointer");
      pa.src[i] = q.params_host[i];
    }
    pa.packed = ws.packed;
    pa.F = ws.folded;
    pa.counters = ws.counters;
    pa.running_mean = q.bn_mode == R2L_BN_EVAL ? q.running_mean : nullptr;
    pa.running_var = q.running_var;
    pa.bn = ws.bn;
    pa.eps = q.eps;
    if (int e = r2l_launch_pack_fold(pa, 1, q.stream)) return e;
  }
  if (q.bn_mode == R2L_BN_TRAIN && phase != R2L_STEP_B) {
    // statistics pass; one rank: the last workgroup also does the BatchNorm bookkeeping
    R2LBnFinalizeArgs f{ws.stats, 1, ws.bn, ws.moments, q.running_mean, q.running_var, q.eps, q.momentum, q.num_batches_tracked};
    const R2LFwdCall c{rw, ws.packed, q.additive, nullptr, nullptr, ws.stats, phase == R2L_STEP_ALL ? &f : nullptr,
                       R2LEpi{0, 0, 0, 0}, R2L_IO_F32, R2L_FWD_STATS_PASS, B, H, W, q.stream};
    if (int e = r2l_isp_fwd_impl(c, R2L_F_STATS_ONLY | R2L_F_FOLDED_VALID | keep, q.workspace, q.workspace_bytes)) return e;
    if (phase == R2L_STEP_A) return 0;
  }
  if (phase == R2L_STEP_B) {
    R2LBnFinalizeArgs f{q.gathered_stats, q.nranks, ws.bn, ws.moments, q.running_mean, q.running_var, q.eps, q.momentum,
                        q.num_batches_tracked};
    if (int e = r2l_launch_bn_finalize(f, 1, q.stream)) return e;
  }
  // (train mode: the statistics pass of this call -- or of phase A of this step -- has left Y' in the workspace wherever the
  // row-streaming forward runs, and the apply pass reads it)
  const R2LFwdCall c{rw, ws.packed, q.additive, q.bn_mode == R2L_BN_NONE ? nullptr : ws.bn, q.out, nullptr, nullptr, ep, q.io,
                     q.bn_mode == R2L_BN_TRAIN ? R2L_FWD_APPLY_PASS : R2L_FWD_WHOLE, B, H, W, q.stream};
  return r2l_isp_fwd_impl(c, R2L_F_FOLDED_VALID | keep, q.workspace, q.workspace_bytes);
}
int r2l_isp_step_fwd(const void* raw, int raw_u16, float denom, const float* const* params_host,
                     const float* additive, int bn_mode, float* running_mean, float* running_var,
                     long long* num_batches_tracked, double eps, double momentum, float* out, void* workspace,
                     size_t workspace_bytes, int B, int H, int W, int nranks, int phase,
                     const double* gathered_stats, void* stream) {
  return r2l_step_fwd("r2l_isp_step_fwd",
                      R2LStepFwd{raw, raw_u16, denom, params_host, additive, bn_mode, running_mean, running_var, num_batches_tracked,
                                 eps, momentum, out, R2L_IO_F32, R2L_LAYOUT_NCHW, workspace, workspace_bytes, B, H, W, nranks, phase,
                                 gathered_stats, stream});
}
// r2l_isp_step_bwd and its _raw, _select, _io and _layout forms: one implementation, what they ask of it
struct R2LStepBwd {
  const void* raw;
  int raw_u16;
  float denom;
  const float *additive, *grad_out, *out;
  float *grad_params, *grad_additive;
  int bn_mode;
  void* workspace;
  size_t workspace_bytes;
  int B, H, W, nranks, phase;
  const double* gathered_sums;
  void* stream;
  float *grad_raw, *guv;  // d/d raw and its scratch (the chroma gradient planes), or null
  unsigned grad_mask;     // R2L_GRAD_* bits (r2l_isp_step_bwd_select), 0 = every parameter gradient
  int io, layout;         // of grad_out, R2L_IO_*, R2L_LAYOUT_* as the entry got them; behind r2l_step_bwd's check io carries
                          // R2L_IO_NHWC too (not planar float32: `out` is not read)
};
static int r2l_isp_step_bwd_impl(const R2LStepBwd& q) {
  const int B = q.B, H = q.H, W = q.W;
  const int keep = (q.phase & R2L_STEP_KEEP_LUMA) ? R2L_F_KEEP_LUMA : 0;
  R2LEpi ep;
  if (int e = r2l_check_dims(B, H, W)) return e;
  if (int e = r2l_epi_from_phase(q.phase, H, W, ep)) return e;
  const int phase = q.phase & ~(R2L_STEP_KEEP_LUMA | R2L_STEP_EPI_MASK);
  if (ep.on && q.grad_additive) return r2l_fail(-3, "r2l_isp_step_bwd: no output epilogue with an additive layer");
  if (!q.raw || !q.grad_out || !q.workspace) return r2l_fail(-1, "r2l_isp_step_bwd: null pointer");
  if (phase != R2L_STEP_ALL && phase != R2L_STEP_A && phase != R2L_STEP_B)
    return r2l_fail(-1, "r2l_isp_step_bwd: unknown phase");
  if (q.nranks < 1 || (q.nranks > 1 && phase == R2L_STEP_ALL && q.bn_mode == R2L_BN_TRAIN))
    return r2l_fail(-1, "r2l_isp_step_bwd: several ranks exchange the BatchNorm sums between phase A and phase B");
  if (phase != R2L_STEP_ALL && q.bn_mode != R2L_BN_TRAIN)
    return r2l_fail(-1, "r2l_isp_step_bwd: only train-mode BatchNorm has two phases");
  if (phase == R2L_STEP_B && !q.gathered_sums) return r2l_fail(-1, "r2l_isp_step_bwd: phase B needs the gathered sums");
  if (q.bn_mode == R2L_BN_TRAIN && !q.out && q.io == R2L_IO_F32)
    return r2l_fail(-1, "r2l_isp_step_bwd: train-mode BatchNorm needs the saved output");
  if (q.io != R2L_IO_F32 && q.grad_additive)
    return r2l_fail(-3, "r2l_isp_step_bwd_io: a 16-bit / channels-last cotangent is not served with an additive layer");
  const R2LRaw rw = r2l_raw_any(q.raw, q.raw_u16, q.denom);
  // (before ANY launch: the recomputing BatchNorm sums below read the raw frames)
  if (int e = r2l_check_raw(rw, W, "r2l_isp_step_bwd")) return e;
  const R2LWorkspace ws = r2l_carve(q.workspace, B, H, W);
  if (q.workspace_bytes < ws.total) return r2l_fail(-2, "r2l_isp_step_bwd: workspace too small (r2l_isp_workspace_bytes)");
  const float* bn = q.bn_mode == R2L_BN_NONE ? nullptr : ws.bn;
  const float* bn_bwd = q.bn_mode == R2L_BN_TRAIN ? ws.bn_bwd : nullptr;
  // the step's forward has folded the parameters (and kept Y', with R2L_STEP_KEEP_LUMA)
  const R2LBwdCall c{rw, ws.packed, q.additive, bn, bn_bwd, q.grad_out, q.grad_params, q.grad_raw, q.guv, ep, q.grad_mask,
                     B, H, W, q.stream, q.io};
  const R2LBwdPlan p = r2l_bwd_plan(q.grad_mask, q.grad_raw != nullptr, q.raw_u16, q.additive != nullptr, ep.on != 0,
                                    keep != 0, B, H, W, q.io != R2L_IO_F32);
  if (q.bn_mode == R2L_BN_TRAIN && phase != R2L_STEP_B) {
    float* means = phase == R2L_STEP_ALL ? ws.bn_bwd : nullptr;
    if (!p.bnr && q.io != R2L_IO_F32)
      return r2l_fail(-3, "r2l_isp_step_bwd_io: internal: the BatchNorm sums of a 16-bit cotangent need the plane pass");
    int e;
#ifndef R2L_SERIAL
    if (p.bnr)
      e = r2l_bwd_bnr_pass(c, ws, p, means);
    else
#endif
      e = r2l_bn_bwd_reduce(q.grad_out, q.out, ws.moments, ws.bsums, means, q.workspace, q.workspace_bytes, B, H, W,
                            R2L_F_FOLDED_VALID, q.stream);
    if (e) return e;
    if (phase == R2L_STEP_A) return 0;
  }
  if (phase == R2L_STEP_B) {
    R2LBnBwdMeansArgs m{q.gathered_sums, q.nranks, ws.moments + 6, ws.bn_bwd};
    if (int e = r2l_launch_bn_bwd_means(m, 1, q.stream)) return e;
  }
  if (q.grad_params) {
    if (q.additive && (H != 256 || W != 256))
      return r2l_fail(-1, "additive_layer is (1,3,256,256): needs 256x256 frames");
    if (int e = r2l_bwd_launch(c, ws, p)) return e;
  }
  if (q.grad_additive) return r2l_additive_bwd(q.grad_out, q.out, bn, bn_bwd, q.grad_additive, B, H, W, q.stream);
  return 0;
}
size_t r2l_isp_raw_grad_scratch_bytes(int B, int H, int W) {
  if (B < 1 || H < 1 || W < 1) return 0;
  return (size_t)2 * B * H * W * sizeof(float);  // gU, gV
}
// what d/d raw needs of a call (r2l_isp_step_bwd_raw, r2l_isp_step_bwd_select): 0, or the error
static int r2l_raw_grad_preconditions(const R2LStepBwd& q, size_t raw_grad_scratch_bytes) {
  if (!R2L_PLANE_PASSES)
    return r2l_fail(-3, "r2l_isp_step_bwd_raw: grad_raw needs the plane passes, which the serial emulation does not have");
  if (int e = r2l_check_dims(q.B, q.H, q.W)) return e;
  if (q.raw_u16) return r2l_fail(-3, "r2l_isp_step_bwd_raw: grad_raw needs float32 frames (16-bit containers have no gradient)");
  if (q.additive) return r2l_fail(-3, "r2l_isp_step_bwd_raw: grad_raw is not produced with an additive layer");
  if ((q.W & 3) || q.W > 2048) return r2l_fail(-3, "r2l_isp_step_bwd_raw: grad_raw needs W % 4 == 0 and W <= 2048");
  if (r2l_env_int("R2L_FWD_TILED", 0))
    return r2l_fail(-3, "r2l_isp_step_bwd_raw: grad_raw needs the row-streaming forward (R2L_FWD_TILED is set)");
  if (q.phase & R2L_STEP_EPI_MASK) return r2l_fail(-3, "r2l_isp_step_bwd_raw: grad_raw is not produced with an output epilogue");
  if (!(q.phase & R2L_STEP_KEEP_LUMA))
    return r2l_fail(-3, "r2l_isp_step_bwd_raw: grad_raw needs a forward that kept Y' (R2L_STEP_KEEP_LUMA in both calls)");
  if (!q.grad_params) return r2l_fail(-1, "r2l_isp_step_bwd_raw: grad_raw needs grad_params (the parameter sums run with it)");
  if (!q.guv) return r2l_fail(-1, "r2l_isp_step_bwd_raw: null raw_grad_scratch");
  if (raw_grad_scratch_bytes < r2l_isp_raw_grad_scratch_bytes(q.B, q.H, q.W))
    return r2l_fail(-2, "r2l_isp_step_bwd_raw: raw_grad_scratch too small (r2l_isp_raw_grad_scratch_bytes)");
  if ((uintptr_t)q.guv % 16 || (uintptr_t)q.grad_raw % 16)
    return r2l_fail(-1, "r2l_isp_step_bwd_raw: grad_raw and raw_grad_scratch must be 16-byte aligned");
  return 0;
}
// the one way into r2l_isp_step_bwd_impl.  `who`: the entry point r2l_last_error() names; masked: the entry takes a grad_mask (a
// planar float32 call words what it refuses of the mask as r2l_isp_step_bwd_select)
static int r2l_step_bwd(const char* who, bool masked, R2LStepBwd q, size_t raw_grad_scratch_bytes) {
  if (int e = r2l_io_check(who, q.io, q.layout, q.grad_out, q.raw_u16, q.additive != nullptr, q.B, q.H, q.W, q.phase)) return e;
  if (q.layout == R2L_LAYOUT_NHWC) q.io |= R2L_IO_NHWC;
  if (masked) {
    const char* w = q.io == R2L_IO_F32 ? "r2l_isp_step_bwd_select" : who;
    if (q.grad_mask & ~(unsigned)(R2L_GRAD_ALL_PARAMS | R2L_GRAD_RAW))
      return r2l_fail(-1, std::string(w) + ": unknown bits in grad_mask");
    if ((q.grad_raw != nullptr) != ((q.grad_mask & R2L_GRAD_RAW) != 0))
      return r2l_fail(-1, std::string(w) + ": grad_raw goes with R2L_GRAD_RAW in grad_mask");
    if (q.grad_mask && !q.grad_params) return r2l_fail(-1, std::string(w) + ": a gradient is asked for but grad_params is null");
  }
  if (int e = q.grad_raw ? r2l_raw_grad_preconditions(q, raw_grad_scratch_bytes) : 0) return e;
  // (phase A computes the BatchNorm sums only: the gradient kernels, and with them d/d raw, run in phase B / ALL.  A mask without
  // a reduced route runs exactly r2l_isp_step_bwd / r2l_isp_step_bwd_raw: r2l_bwd_plan)
  return r2l_isp_step_bwd_impl(q);
}
int r2l_isp_step_bwd(const void* raw, int raw_u16, float denom, const float* additive, const float* grad_out,
                     const float* out, float* grad_params, float* grad_additive, int bn_mode, void* workspace,
                     size_t workspace_bytes, int B, int H, int W, int nranks, int phase,
                     const double* gathered_sums, void* stream) {
  return r2l_step_bwd("r2l_isp_step_bwd", false,
                      R2LStepBwd{raw, raw_u16, denom, additive, grad_out, out, grad_params, grad_additive, bn_mode, workspace,
                                 workspace_bytes, B, H, W, nranks, phase, gathered_sums, stream, nullptr, nullptr, 0, R2L_IO_F32,
                                 R2L_LAYOUT_NCHW},
                      0);
}
int r2l_isp_step_bwd_raw(const void* raw, int raw_u16, float denom, const float* additive, const float* grad_out,
                         const float* out, float* grad_params, float* grad_additive, int bn_mode, void* workspace,
                         size_t workspace_bytes, int B, int H, int W, int nranks, int phase,
                         const double* gathered_sums, void* stream, float* grad_raw, void* raw_grad_scratch,
                         size_t raw_grad_scratch_bytes) {
  // (without grad_raw: r2l_isp_step_bwd, the scratch is not looked at)
  return r2l_step_bwd("r2l_isp_step_bwd_raw", false,
                      R2LStepBwd{raw, raw_u16, denom, additive, grad_out, out, grad_params, grad_additive, bn_mode, workspace,
                                 workspace_bytes, B, H, W, nranks, phase, gathered_sums, stream, grad_raw,
                                 grad_raw ? (float*)raw_grad_scratch : nullptr, 0, R2L_IO_F32, R2L_LAYOUT_NCHW},
                      raw_grad_scratch_bytes);
}
int r2l_isp_step_bwd_select(const void* raw, int raw_u16, float denom, const float* additive, const float* grad_out,
                            const float* out, float* grad_params, float* grad_additive, int bn_mode, void* workspace,
                            size_t workspace_bytes, int B, int H, int W, int nranks, int phase,
                            const double* gathered_sums, void* stream, float* grad_raw, void* raw_grad_scratch,
                            size_t raw_grad_scratch_bytes, unsigned grad_mask) {
  return r2l_step_bwd("r2l_isp_step_bwd_select", true,
                      R2LStepBwd{raw, raw_u16, denom, additive, grad_out, out, grad_params, grad_additive, bn_mode, workspace,
                                 workspace_bytes, B, H, W, nranks, phase, gathered_sums, stream, grad_raw,
                                 (float*)raw_grad_scratch, grad_mask, R2L_IO_F32, R2L_LAYOUT_NCHW},
                      raw_grad_scratch_bytes);
}

// ---- 16-bit and channels-last output / cotangent (include/r2l_isp.h: R2L_IO_*, R2L_LAYOUT_*) -----------------------------------
int r2l_isp_layout_supported(int io, int layout, int raw_u16, int has_additive, int B, int H, int W, int phase) {
  if (io != R2L_IO_F32 && io != R2L_IO_BF16 && io != R2L_IO_F16) return 0;
  if (layout != R2L_LAYOUT_NCHW && layout != R2L_LAYOUT_NHWC) return 0;
  if (io == R2L_IO_F32 && layout == R2L_LAYOUT_NCHW) return 1;
  return r2l_io_why(raw_u16, has_additive != 0, B, H, W, phase) ? 0 : 1;
}
int r2l_isp_io_supported(int io, int raw_u16, int has_additive, int B, int H, int W, int phase) {
  return r2l_isp_layout_supported(io, R2L_LAYOUT_NCHW, raw_u16, has_additive, B, H, W, phase);
}
// the forwards and backwards that take io [and layout]: r2l_step_fwd / r2l_step_bwd above, like the planar float32 entries
int r2l_isp_step_fwd_layout(const void* raw, int raw_u16, float denom, const float* const* params_host,
                            const float* additive, int bn_mode, float* running_mean, float* running_var,
                            long long* num_batches_tracked, double eps, double momentum, void* out, int io, int layout,
                            void* workspace, size_t workspace_bytes, int B, int H, int W, int nranks, int phase,
                            const double* gathered_stats, void* stream) {
  return r2l_step_fwd("r2l_isp_step_fwd_layout",
                      R2LStepFwd{raw, raw_u16, denom, params_host, additive, bn_mode, running_mean, running_var, num_batches_tracked,
                                 eps, momentum, (float*)out, io, layout, workspace, workspace_bytes, B, H, W, nranks, phase,
                                 gathered_stats, stream});
}
int r2l_isp_step_fwd_io(const void* raw, int raw_u16, float denom, const float* const* params_host,
                        const float* additive, int bn_mode, float* running_mean, float* running_var,
                        long long* num_batches_tracked, double eps, double momentum, void* out, int io, void* workspace,
                        size_t workspace_bytes, int B, int H, int W, int nranks, int phase,
                        const double* gathered_stats, void* stream) {
  return r2l_step_fwd("r2l_isp_step_fwd_io",
                      R2LStepFwd{raw, raw_u16, denom, params_host, additive, bn_mode, running_mean, running_var, num_batches_tracked,
                                 eps, momentum, (float*)out, io, R2L_LAYOUT_NCHW, workspace, workspace_bytes, B, H, W, nranks, phase,
                                 gathered_stats, stream});
}
int r2l_isp_step_bwd_layout(const void* raw, int raw_u16, float denom, const float* additive, const void* grad_out, int io,
                            int layout, const void* out, float* grad_params, float* grad_additive, int bn_mode,
                            void* workspace, size_t workspace_bytes, int B, int H, int W, int nranks, int phase,
                            const double* gathered_sums, void* stream, float* grad_raw, void* raw_grad_scratch,
                            size_t raw_grad_scratch_bytes, unsigned grad_mask) {
  return r2l_step_bwd("r2l_isp_step_bwd_layout", true,
                      R2LStepBwd{raw, raw_u16, denom, additive, (const float*)grad_out, (const float*)out, grad_params,
                                 grad_additive, bn_mode, workspace, workspace_bytes, B, H, W, nranks, phase, gathered_sums, stream,
                                 grad_raw, (float*)raw_grad_scratch, grad_mask, io, layout},
                      raw_grad_scratch_bytes);
}
int r2l_isp_step_bwd_io(const void* raw, int raw_u16, float denom, const float* additive, const void* grad_out, int io,
                        const void* out, float* grad_params, float* grad_additive, int bn_mode, void* workspace,
                        size_t workspace_bytes, int B, int H, int W, int nranks, int phase,
                        const double* gathered_sums, void* stream, float* grad_raw, void* raw_grad_scratch,
                        size_t raw_grad_scratch_bytes, unsigned grad_mask) {
  return r2l_step_bwd("r2l_isp_step_bwd_io", true,
                      R2LStepBwd{raw, raw_u16, denom, additive, (const float*)grad_out, (const float*)out, grad_params,
                                 grad_additive, bn_mode, workspace, workspace_bytes, B, H, W, nranks, phase, gathered_sums, stream,
                                 grad_raw, (float*)raw_grad_scratch, grad_mask, io, R2L_LAYOUT_NCHW},
                      raw_grad_scratch_bytes);
}

// ---- the whole forward and backward as single calls (every r2l_isp_fwd* / r2l_isp_bwd*) -----------------------------------------
int r2l_isp_fwd(const float* raw, const float* params, const float* additive,
                const float* bn_mean_istd, float* out, double* stats, void* workspace,
                size_t workspace_bytes, int B, int H, int W, int flags, void* stream) {
  return r2l_isp_fwd_impl(R2LFwdCall{r2l_raw_f32(raw), params, additive, bn_mean_istd, out, stats, nullptr, R2LEpi{0, 0, 0, 0},
                                     R2L_IO_F32, R2L_FWD_WHOLE, B, H, W, stream},
                          flags, workspace, workspace_bytes);
}
// statistics pass + BatchNorm bookkeeping in one launch (one rank: no exchange between the two)
static int r2l_isp_fwd_stats_bn_impl(const R2LRaw& raw, const float* params, const float* additive, double* stats,
                                     float* bn_mean_istd, double* moments, float* running_mean, float* running_var,
                                     long long* num_batches_tracked, double eps, double momentum, void* workspace,
                                     size_t workspace_bytes, int B, int H, int W, void* stream) {
  if (!stats || !bn_mean_istd) return r2l_fail(-1, "r2l_isp_fwd_stats_bn: null pointer");
  if ((running_mean == nullptr) != (running_var == nullptr))
    return r2l_fail(-1, "r2l_isp_fwd_stats_bn: running_mean and running_var go together");
  R2LBnFinalizeArgs f{stats, 1, bn_mean_istd, moments, running_mean, running_var, eps, momentum, num_batches_tracked};
  return r2l_isp_fwd_impl(R2LFwdCall{raw, params, additive, nullptr, nullptr, stats, &f, R2LEpi{0, 0, 0, 0}, R2L_IO_F32,
                                     R2L_FWD_WHOLE, B, H, W, stream},
                          R2L_F_STATS_ONLY, workspace, workspace_bytes);
}
int r2l_isp_fwd_stats_bn(const float* raw, const float* params, const float* additive, double* stats,
                         float* bn_mean_istd, double* moments, float* running_mean, float* running_var,
                         long long* num_batches_tracked, double eps, double momentum, void* workspace,
                         size_t workspace_bytes, int B, int H, int W, void* stream) {
  return r2l_isp_fwd_stats_bn_impl(r2l_raw_f32(raw), params, additive, stats, bn_mean_istd, moments, running_mean,
                                   running_var, num_batches_tracked, eps, momentum, workspace, workspace_bytes, B,
                                   H, W, stream);
}
int r2l_isp_fwd_stats_bn_u16(const unsigned short* raw, float denom, const float* params, const float* additive,
                             double* stats, float* bn_mean_istd, double* moments, float* running_mean,
                             float* running_var, long long* num_batches_tracked, double eps, double momentum,
                             void* workspace, size_t workspace_bytes, int B, int H, int W, void* stream) {
  return r2l_isp_fwd_stats_bn_impl(r2l_raw_u16(raw, denom), params, additive, stats, bn_mean_istd, moments,
                                   running_mean, running_var, num_batches_tracked, eps, momentum, workspace,
                                   workspace_bytes, B, H, W, stream);
}
int r2l_isp_fwd_u16(const unsigned short* raw, float denom, const float* params, const float* additive,
                    const float* bn_mean_istd, float* out, double* stats, void* workspace,
                    size_t workspace_bytes, int B, int H, int W, int flags, void* stream) {
  return r2l_isp_fwd_impl(R2LFwdCall{r2l_raw_u16(raw, denom), params, additive, bn_mean_istd, out, stats, nullptr,
                                     R2LEpi{0, 0, 0, 0}, R2L_IO_F32, R2L_FWD_WHOLE, B, H, W, stream},
                          flags, workspace, workspace_bytes);
}
int r2l_isp_bwd(const float* raw, const float* params, const float* additive,
                const float* bn_mean_istd, const float* bn_bwd, const float* grad_out,
                float* grad_params, float* grad_raw, void* workspace, size_t workspace_bytes, int B,
                int H, int W, int flags, void* stream) {
  return r2l_isp_bwd_impl(r2l_raw_f32(raw), params, additive, bn_mean_istd, bn_bwd, grad_out, grad_params, grad_raw,
                          workspace, workspace_bytes, B, H, W, flags, stream);
}
int r2l_isp_bwd_u16(const unsigned short* raw, float denom, const float* params, const float* additive,
                    const float* bn_mean_istd, const float* bn_bwd, const float* grad_out,
                    float* grad_params, void* workspace, size_t workspace_bytes, int B, int H, int W, int flags,
                    void* stream) {
  return r2l_isp_bwd_impl(r2l_raw_u16(raw, denom), params, additive, bn_mean_istd, bn_bwd, grad_out, grad_params,
                          nullptr, workspace, workspace_bytes, B, H, W, flags, stream);
}

static int r2l_raw2rgb_fwd_impl(const R2LRaw& raw, const float* black_level, float* out, int B, int H, int W,
                                int reduce_size, int out_channels, void* stream) {
  if (B < 1 || H < 2 || W < 2 || (H & 1) || (W & 1)) return r2l_fail(-1, "raw2rgb: H and W must be even");
  if (out_channels != 3 && out_channels != 4) return r2l_fail(-1, "raw2rgb: out_channels in {3,4}");
  if (int e = r2l_check_raw(raw, 4, "raw2rgb")) return e;
  if (!out) return r2l_fail(-1, "raw2rgb: null pointer");
  R2LRaw2RgbArgs a{raw, black_level, out, nullptr, nullptr, nullptr, B, H, W, reduce_size, out_channels};
  const size_t nitems = (size_t)B * (H / 2) * ((W + 3) / 4);
  size_t grid = (nitems + R2L_NT - 1) / R2L_NT;
  if (grid > 4096) grid = 4096;
  return r2l_launch_raw2rgb_fwd(a, r2l_flat_grid(grid), stream);
}

size_t r2l_raw2rgb_bwd_workspace_bytes(int B, int H, int W) {
  (void)B;
  (void)H;
  (void)W;
  return sizeof(float) * 4 * R2L_MAX_BLOCKS;
}

int r2l_raw2rgb_bwd(const float* grad_out, float* grad_raw, double* grad_black_level, void* workspace,
                    size_t workspace_bytes, int B, int H, int W, int reduce_size, int out_channels,
                    void* stream) {
  if (B < 1 || H < 2 || W < 2 || (H & 1) || (W & 1)) return r2l_fail(-1, "raw2rgb: H and W must be even");
  if (out_channels != 3 && out_channels != 4) return r2l_fail(-1, "raw2rgb: out_channels in {3,4}");
  if (!grad_out) return r2l_fail(-1, "raw2rgb_bwd: null pointer");
  if (grad_black_level && (!workspace || workspace_bytes < r2l_raw2rgb_bwd_workspace_bytes(B, H, W)))
    return r2l_fail(-2, "raw2rgb_bwd: workspace too small");
  R2LRaw2RgbArgs a{r2l_raw_f32(nullptr), nullptr, nullptr, grad_out, grad_raw,
                   grad_black_level ? (float*)workspace : nullptr, B, H, W, reduce_size, out_channels};
  const size_t nitems = (size_t)B * (H / 2) * ((W + 3) / 4);
  size_t grid = (nitems + R2L_NT - 1) / R2L_NT;
  if (grid > R2L_MAX_BLOCKS) grid = R2L_MAX_BLOCKS;
  grid = (size_t)r2l_flat_grid(grid);
  if (int e = r2l_launch_raw2rgb_bwd(a, (int)grid, stream)) return e;
  if (grad_black_level) {
    R2LReduceRowsArgs r{(const float*)workspace, grad_black_level, (int)grid, 1.0, nullptr};
    return r2l_launch_reduce_rows(r, 4, stream);
  }
  return 0;
}

// ---- fft_denoising: the two transforms.  Device build: rocFFT plans (real <-> Hermitian, float64, rows of length W),
// cached per (W, rows); the work buffer comes out of the caller's workspace like everything else.
struct R2LFftPlans {
#ifndef R2L_EMUL
  rocfft_plan fwd = nullptr, inv = nullptr;
#endif
  size_t work_bytes = 0;
};
#ifndef R2L_EMUL
// rocFFT is NOT a link-time dependency of this library (round 6): fft_denoising is the one stage of the path that is a library
// call, and an alternate the reference's defaults never take (train.py:100-101 offers it).  The library is opened the first time
// an fft_denoising chain is asked for; every other entry point works on a box without it.
#include <dlfcn.h>
struct R2LRocfft {
  decltype(&rocfft_setup) setup = nullptr;
  decltype(&rocfft_plan_create) plan_create = nullptr;
  decltype(&rocfft_plan_get_work_buffer_size) plan_get_work_buffer_size = nullptr;
  decltype(&rocfft_execution_info_create) execution_info_create = nullptr;
  decltype(&rocfft_execution_info_set_stream) execution_info_set_stream = nullptr;
  decltype(&rocfft_execution_info_set_work_buffer) execution_info_set_work_buffer = nullptr;
  decltype(&rocfft_execute) execute = nullptr;
  decltype(&rocfft_execution_info_destroy) execution_info_destroy = nullptr;
  bool ok = false;
};
static const R2LRocfft* r2l_rocfft() {
  static R2LRocfft api;
  static std::once_flag once;
  std::call_once(once, [] {
    void* h = nullptr;
    for (const char* name : {"librocfft.so.0", "librocfft.so", "/opt/rocm/lib/librocfft.so.0", "/opt/rocm/lib/librocfft.so"})
      if ((h = dlopen(name, RTLD_NOW | RTLD_LOCAL))) break;
    if (!h) return;
#define R2L_FFT_SYM(field, sym) api.field = (decltype(api.field))dlsym(h, #sym)
    R2L_FFT_SYM(setup, rocfft_setup);
    R2L_FFT_SYM(plan_create, rocfft_plan_create);
    R2L_FFT_SYM(plan_get_work_buffer_size, rocfft_plan_get_work_buffer_size);
    R2L_FFT_SYM(execution_info_create, rocfft_execution_info_create);
    R2L_FFT_SYM(execution_info_set_stream, rocfft_execution_info_set_stream);
    R2L_FFT_SYM(execution_info_set_work_buffer, rocfft_execution_info_set_work_buffer);
    R2L_FFT_SYM(execute, rocfft_execute);
    R2L_FFT_SYM(execution_info_destroy, rocfft_execution_info_destroy);
#undef R2L_FFT_SYM
    api.ok = api.setup && api.plan_create && api.plan_get_work_buffer_size && api.execution_info_create &&
             api.execution_info_set_stream && api.execution_info_set_work_buffer && api.execute && api.execution_info_destroy;
  });
  return api.ok ? &api : nullptr;
}
static int r2l_fft_plans(int W, size_t rows, R2LFftPlans& out) {
  const R2LRocfft* fft = r2l_rocfft();
  if (!fft) return r2l_fail(-10, "fft_denoising needs librocfft.so (ROCm), which could not be opened; every other chain works without it");
  static std::mutex mu;
  static std::map<std::pair<int, std::pair<int, size_t>>, R2LFftPlans> cache;  // (device, (W, rows))
  static bool setup = false;
  std::lock_guard<std::mutex> lk(mu);
  if (!setup) {
    if (fft->setup() != rocfft_status_success) return r2l_fail(-10, "rocfft_setup failed");
    setup = true;
  }
  int dev = 0;
  (void)hipGetDevice(&dev);
  const std::pair<int, std::pair<int, size_t>> key{dev, {W, rows}};
  auto it = cache.find(key);
  if (it == cache.end()) {
    // (plans live as long as the process: a caller on another thread may be executing one, so none is destroyed here)
    R2LFftPlans p;
    const size_t len = (size_t)W;
    if (fft->plan_create(&p.fwd, rocfft_placement_notinplace, rocfft_transform_type_real_forward,
                           rocfft_precision_double, 1, &len, rows, nullptr) != rocfft_status_success ||
        fft->plan_create(&p.inv, rocfft_placement_notinplace, rocfft_transform_type_real_inverse,
                           rocfft_precision_double, 1, &len, rows, nullptr) != rocfft_status_success)
      return r2l_fail(-10, "rocfft_plan_create failed");
    size_t w0 = 0, w1 = 0;
    fft->plan_get_work_buffer_size(p.fwd, &w0);
    fft->plan_get_work_buffer_size(p.inv, &w1);
    p.work_bytes = w0 > w1 ? w0 : w1;
    it = cache.emplace(key, p).first;
  }
  out = it->second;
  return 0;
}
static int r2l_fft_exec(rocfft_plan plan, void* in, void* outp, void* work, size_t work_bytes, void* stream) {
  const R2LRocfft* fft = r2l_rocfft();
  if (!fft) return r2l_fail(-10, "librocfft.so could not be opened");
  rocfft_execution_info info = nullptr;
  if (fft->execution_info_create(&info) != rocfft_status_success) return r2l_fail(-10, "rocfft_execution_info_create failed");
  rocfft_status st = fft->execution_info_set_stream(info, stream);
  if (st == rocfft_status_success && work_bytes) st = fft->execution_info_set_work_buffer(info, work, work_bytes);
  void* ins[1] = {in};
  void* outs[1] = {outp};
  if (st == rocfft_status_success) st = fft->execute(plan, ins, outs, info);
  fft->execution_info_destroy(info);
  return st == rocfft_status_success ? 0 : r2l_fail(-10, "rocfft_execute failed");
}
#endif
// ---- the static chains: one plan (r2l_static_plan), one launcher (r2l_static_launch) ------------------------------------------
// processing()'s numeric arguments out of the C ABI's array (NULL: the reference's defaults).  A median size that is no integer
// becomes `bad_median`: -1, which r2l_static_opts_problem refuses -- but for r2l_static_workspace_bytes_opts, which sizes it as 3
static R2LStaticOpts r2l_static_opts(const double* options_host, int bad_median = -1) {
  R2LStaticOpts o;
  if (!options_host) return o;
  o.sharp_radius = options_host[R2L_SOPT_SHARP_RADIUS];
  o.sharp_amount = options_host[R2L_SOPT_SHARP_AMOUNT];
  o.gaussian_sigma = options_host[R2L_SOPT_GAUSSIAN_SIGMA];
  o.fft_fraction = options_host[R2L_SOPT_FFT_FRACTION];
  const double m = options_host[R2L_SOPT_MEDIAN_SIZE];
  o.median_kernel_size = (m == (double)(int)m) ? (int)m : bad_median;
  return o;
}

// the kernels that serve a call
enum {
  R2L_ROUTE_MENON,   // Menon2007: plane passes (r2l_static_menon.h) on a float64 image + five planes of workspace
  R2L_ROUTE_CHAIN,   // one launch of the row-streaming luma-chain kernel (r2l_static_chain.h)
  R2L_ROUTE_PLANES,  // luma-plane passes: raw -> Y | sharpen | denoise | raw + Y'' -> RGB, on two float64 planes of workspace
  R2L_ROUTE_FULL,    // the tile kernel of the default chain (bilinear + sharpening_filter + gaussian_denoising)
  R2L_ROUTE_STREAM,  // the short chain, row-streaming (r2l_static_stream.h)
  R2L_ROUTE_SHORT    // the short chain's tile kernel
};

// What a static call launches and what it needs, decided from the shape of the call alone: r2l_static_fwd_impl hands it to
// r2l_static_launch, the workspace queries report `workspace_bytes`, r2l_static_io_supported reports `no_io`
struct R2LStaticPlan {
  int route;               // R2L_ROUTE_*
  bool fft;                // fft_denoising behind MENON / PLANES: the linear image low-passed along its rows, then clip and gamma
  int ops[2];              // MENON / PLANES: the plane filter (r2l_static_planes.h) of the sharpening and of the denoising stage, 0: none
  double fft_fraction;
  const char* refused;     // why the call cannot run at all (-4), or null
  const char* no_io;       // why a 16-bit output is not served (-3), or null
  const char* no_stats;    // why r2l_static_stats is not served (-3), or null: the same kernels in their statistics form
  const char* no_epi;      // why an output epilogue is not served (-3), or null (also without one): the same kernels in their epilogue form
  int nparts;              // io = R2L_IO_STATS: the partials double[6] the launch leaves in the workspace, one per wavefront
  int err;                 // rocFFT could not plan the transforms (its text is in r2l_err)
  bool too_large;          // more workgroups than a launch takes
  // workspace of MENON: the (B,3,H,W) float64 image + five (B,H,W) planes; of PLANES: two planes, for fft_denoising the image
  // behind them; behind either, for fft_denoising, the spectrum and rocFFT's work buffer
  size_t rgb_off, spec_off, work_off, rows, workspace_bytes;
  R2LFftPlans fft_plans;
  // bands of `band_h` rows in `nseg` 256-column strips (CHAIN: the wavefronts of a workgroup), work items, workgroups
  int nseg, nband, band_h, nitems, grid;
  R2LStreamLaunch stream;  // STREAM: the whole chain; PLANES: its LUMA instantiation
#ifndef R2L_SERIAL
  R2LChainLaunch chain;
#endif
};
// frames: R2L_FRAMES_*; io: R2L_IO_* of the output, or R2L_IO_STATS: none, the channel sums (r2l_static_stats).  The only reader of the static chains' overrides of diagnostic builds
// (R2L_STATIC_TILED, R2L_CHAIN_BAND, R2L_STREAM_BANDS, R2L_GRID_STATIC*).  sized = false: without rocFFT's work buffer in
// `workspace_bytes` -- for callers that ask for `no_io` alone and must not open the library.  epilogue: R2L_STEP_EPI_* bits (r2l_static_fwd_epilogue),
// 0: none -- the plan of every other entry
static R2LStaticPlan r2l_static_plan(int frames, int B, int H, int W, int debayer, int sharpening, int denoising,
                                     const R2LStaticOpts& opt, int io, bool sized = true, int epilogue = 0) {
  R2LStaticPlan p = {};
  const bool f64 = frames == R2L_FRAMES_F64, menon = debayer == R2L_DEBAYER_MENON2007, malvar = debayer == R2L_DEBAYER_MALVAR2004;
  const bool unsharp = sharpening == R2L_SHARPEN_UNSHARP, median = denoising == R2L_DENOISE_MEDIAN;
  const bool luma = sharpening != R2L_SHARPEN_NONE || denoising != R2L_DENOISE_NONE;  // (R2LStaticArgs::full)
  const bool med5 = median && opt.median_kernel_size != 3;  // the 5x5 median runs as a luma-plane pass
  const bool quads = (W & 3) == 0;
  const bool tiled = r2l_env_int("R2L_STATIC_TILED", 0) != 0;
  p.fft = denoising == R2L_DENOISE_FFT;
  p.fft_fraction = opt.fft_fraction;
  p.ops[0] = sharpening == R2L_SHARPEN_FILTER ? 1 : (unsharp ? 4 : 0);
  p.ops[1] = denoising == R2L_DENOISE_GAUSSIAN ? 2 : (median ? (opt.median_kernel_size == 5 ? 5 : 3) : 0);
#ifdef R2L_SERIAL
  const bool chain = false;  // (lane shifts and wave-level exchange: not expressible in the one-lane-at-a-time emulation)
#else
  // the luma-chain kernel: every demosaic but Menon2007, every sharpening and denoising but fft_denoising and the 5x5 median, at
  // least one of them; W % 4 == 0, frames up to 2048 columns (behind unsharp_masking the chroma waits 7 rows for its luma: 28 KB
  // of LDS per 256-column strip, 4 strips at most)
  const bool chain = !menon && !med5 && !tiled && quads && W <= (unsharp ? 1024 : 2048) && !p.fft && luma;
#endif
  // the tile kernel of the default chain stages float32 frames in LDS
  const bool full = !f64 && debayer == R2L_DEBAYER_BILINEAR && sharpening == R2L_SHARPEN_FILTER && denoising == R2L_DENOISE_GAUSSIAN;
  p.route = menon                               ? R2L_ROUTE_MENON
            : chain                             ? R2L_ROUTE_CHAIN
            : (p.fft || med5 || (luma && !full)) ? R2L_ROUTE_PLANES
            : luma                              ? R2L_ROUTE_FULL
            : (quads && (f64 || !tiled))        ? R2L_ROUTE_STREAM
                                                : R2L_ROUTE_SHORT;
  if (menon && (!quads || H < 4 || W < 4))
    p.refused = "r2l_static_fwd: menon2007 runs as plane passes, which need W % 4 == 0 (and frames of at least 4 x 4)";
  if (p.route == R2L_ROUTE_PLANES && !quads) p.refused = "r2l_static_fwd: this chain runs as plane passes, which need W % 4 == 0";

  // a 16-bit output (form 0), none (1: the statistics form) or an output epilogue (2): what runs as one launch of a row-streaming
  // kernel on frames up to 2048 columns
  const auto one_launch = [&](int form) -> const char* {
    const bool stats = form == 1, epi = form == 2;
    if (frames != R2L_FRAMES_F32 && frames != R2L_FRAMES_U16 && frames != R2L_FRAMES_F64) return "frames must be one of R2L_FRAMES_*";
    if (H < 4 || W < 4 || (H & 1) || (W & 1)) return "H and W must be even and >= 4";
    if (epi && f64) return "float64 frames have no epilogue form of the static kernels";
#ifdef R2L_SERIAL
    return epi     ? "the serial emulation has no epilogue form of the static kernels"
           : stats ? "the serial emulation has no statistics form of the static kernels (not expressible one lane at a time)"
                   : "the serial emulation has no 16-bit form of the static kernels";
#else
    if (menon)
      return epi     ? "menon2007 runs as plane passes, which have no epilogue form"
             : stats ? "menon2007 runs as plane passes, which have no statistics form"
                     : "menon2007 runs as plane passes, which store float32";
    if (debayer != R2L_DEBAYER_BILINEAR && !malvar) return "unknown debayer";
    if (sharpening != R2L_SHARPEN_NONE && sharpening != R2L_SHARPEN_FILTER && !unsharp) return "unknown sharpening";
    if (denoising != R2L_DENOISE_NONE && denoising != R2L_DENOISE_GAUSSIAN && !median && !p.fft) return "unknown denoising";
    if (p.fft)
      return epi     ? "fft_denoising runs as plane passes, which have no epilogue form"
             : stats ? "fft_denoising runs as plane passes, which have no statistics form"
                     : "fft_denoising runs as plane passes, which store float32";
    if (med5)
      return epi     ? "the 5x5 median runs as a plane pass, which has no epilogue form"
             : stats ? "the 5x5 median runs as a plane pass, which has no statistics form"
                     : "the 5x5 median runs as a plane pass, which stores float32";
    if (!quads) return "needs W % 4 == 0 (the row-streaming kernels)";
    if (W > 2048) return "needs W <= 2048";
    if (p.route == R2L_ROUTE_STREAM) return nullptr;
    if (p.route != R2L_ROUTE_CHAIN)
      return unsharp && W > 1024 ? "behind unsharp_masking the luma-chain kernel needs W <= 1024"
                                 : "needs the row-streaming kernels (R2L_STATIC_TILED is set)";
    if (f64) return stats ? "float64 frames on a luma chain have no statistics form" : "float64 frames on a luma chain store float32";
    return nullptr;
#endif
  };
  p.no_io = one_launch(0);
  p.no_stats = one_launch(1);
  // an output epilogue: k even only -- a row-walking kernel's stores under a rotation by 90 degrees land one element per row of
  // the rotated tensor, which the permutation kernel does better
  const bool want_epi = (epilogue & R2L_STEP_EPI_MASK) != 0;
  p.no_epi = !want_epi ? nullptr
             : ((epilogue >> R2L_STEP_EPI_ROT_SHIFT) & 1)
                 ? "a rotation by 90 or 270 degrees (k odd) is not part of the row-streaming kernels' stores"
                 : one_launch(2);
  const bool epi = want_epi && !p.no_epi;
  if (B < 1 || H < 1 || W < 1) return p;

  const size_t px = (size_t)B * H * W;
  if (p.route == R2L_ROUTE_MENON || p.route == R2L_ROUTE_PLANES) {
    p.rows = (size_t)3 * B * H;
    p.rgb_off = menon ? 0 : r2l_align_up(2 * sizeof(double) * px);
    p.spec_off = menon ? r2l_align_up(8 * sizeof(double) * px) : p.rgb_off + r2l_align_up(3 * sizeof(double) * px);
    p.workspace_bytes = menon ? p.spec_off : 2 * sizeof(double) * px;
    if (p.fft) {
      p.work_off = p.spec_off + r2l_align_up(2 * sizeof(double) * p.rows * (size_t)(W / 2 + 1));
#ifndef R2L_EMUL
      if (sized) p.err = r2l_fft_plans(W, p.rows, p.fft_plans);
#else
      (void)sized;
#endif
      p.workspace_bytes = p.err ? 0 : p.work_off + r2l_align_up(p.fft_plans.work_bytes);
    }
  }
  // (the launch shape: of frames r2l_check_dims lets through, whose counts fit the arithmetic below)
  if ((size_t)H * W > ((size_t)1 << 29) || px > ((size_t)1 << 40)) return p;

  const bool stats = io == R2L_IO_STATS && !p.no_stats;
  const int kind = frames == R2L_FRAMES_U16 ? 1 : (f64 ? 2 : 0), out = stats ? R2L_IO_STATS : ((p.no_io || io == R2L_IO_STATS) ? R2L_IO_F32 : io);
  // the statistics forms: a workgroup walks the work items bid, bid + grid, ...; as many workgroups as the reduction trees take
  long stats_cap = r2l_env_int("R2L_GRID_STATIC", R2L_MAX_BLOCKS);
  if (stats_cap > R2L_MAX_BLOCKS) stats_cap = R2L_MAX_BLOCKS;
  long grid = 0;
  switch (p.route) {
    case R2L_ROUTE_MENON: {
      const size_t g = (px + R2L_NT - 1) / R2L_NT;
      grid = g > 16384 ? 16384 : (long)g;
      break;
    }
    case R2L_ROUTE_CHAIN: {
#ifndef R2L_SERIAL
      // Bands: every band re-computes 7 rows of halo, so tall bands are cheaper (256x1024x1024: 64 rows 1134 us,
      // 128 rows 1112, 256 rows 1086; profiles/r02_f_chain_bands.txt) -- as tall as leaves ~1024 workgroups (two
      // rounds of two per CU), but not below 64 rows
      long nband = (1024 + B - 1) / B;
      if (nband > H / 64) nband = H / 64;
      if (const int rows = r2l_env_int("R2L_CHAIN_BAND", 0)) nband = (H + rows - 1) / rows;
      if (nband < 1) nband = 1;
      p.band_h = (int)((H + nband - 1) / nband);
      p.band_h += p.band_h & 1;  // bands start on even rows
      p.nband = (H + p.band_h - 1) / p.band_h;
      p.nseg = W <= 256 ? 1 : (W <= 512 ? 2 : (W <= 1024 ? 4 : 8));
      grid = (long)B * p.nband;
      if (stats) {
        p.too_large = grid > (1L << 30);
        grid = grid < stats_cap ? grid : stats_cap;
        p.nparts = (int)grid * p.nseg;
        p.workspace_bytes = sizeof(double) * 6 * (size_t)p.nparts;
      }
      p.chain = r2l_static_chain_table[epi][out][kind][malvar][unsharp][median];
#endif
      break;
    }
    case R2L_ROUTE_PLANES:
    case R2L_ROUTE_STREAM: {
      // One wavefront per (image, 256-column strip, row band), dealt in that order, so the ~3,000 wavefronts resident
      // at any moment work on ADJACENT bands.  Short bands keep that active region of the frames and of the output
      // compact in HBM (a few tens of MiB instead of a slice of every image of the batch), which is worth far more
      // than the halo rows every band re-reads (they come from L2): same-buffer A/B on 256x1024x1024, bilinear,
      // 128 rows per band 862 us, 32 rows 830, 16 rows 800, 8 rows 735-756, 5 rows 754, 4 rows 778, 2 rows 1012.
      // Malvar (4 halo rows, 5-row window) is flat between 24 and 48 rows per band -- and, round 5, 6 % FASTER at 10 rows (two
      // full groups of its 5-step unrolled loop): 883 -> 826 us on 256x1024x1024, same buffers (profiles/r05_static_ab.txt;
      // 9 rows 835, 13 rows 848, 15 rows 836, 5 rows 867, 6 rows -- 4 wasted steps of 10 -- 1000): the same compactness, at
      // 40 % more fetched rows.  Rounds 1-4 had only swept 24 .. 48.
      // Round 2, other frame widths (profiles/r02_j_stream_bands.txt): 6-row bands are as good on 1024-wide frames
      // (0.711 vs 0.709 of the HBM peak) and better on 512- and 256-wide ones (0.718 vs 0.692, 0.724 vs 0.700).
      p.nseg = (W + 255) / 256;
      const int rows = malvar ? 10 : 6;
      long nband = r2l_env_int("R2L_STREAM_BANDS", (H + rows - 1) / rows);
      if (nband > H / 2) nband = H / 2;
      if (nband < 1) nband = 1;
      p.band_h = (int)((H + nband - 1) / nband);
      p.nband = (H + p.band_h - 1) / p.band_h;
      const long nitems = (long)B * p.nseg * p.nband;
      const int wpb = R2L_STREAM_NT / 64;
      p.nitems = (int)nitems;
      grid = (nitems + wpb - 1) / wpb;
      p.too_large = nitems > (1L << 30);
      if (stats) {
        grid = grid < stats_cap ? grid : stats_cap;
        p.nparts = (int)grid * wpb;
        p.workspace_bytes = sizeof(double) * 6 * (size_t)p.nparts;
      }
      p.stream = p.route == R2L_ROUTE_PLANES ? r2l_static_luma_table[kind][malvar] : r2l_static_stream_table[epi][out][kind][malvar];
      break;
    }
    default: {  // persistent 64 x 64 tile walkers
      const long ntiles = (long)B * ((H + GStatic::TH - 1) / GStatic::TH) * ((W + GStatic::TW - 1) / GStatic::TW);
      grid = r2l_tile_grid(ntiles > R2L_MAX_BLOCKS ? R2L_MAX_BLOCKS : (int)ntiles,
                           p.route == R2L_ROUTE_FULL ? r2l_env_int("R2L_GRID_STATIC_FULL", 256) : r2l_env_int("R2L_GRID_STATIC", 1024));
    }
  }
  p.too_large = p.too_large || grid > (1L << 30);
  p.grid = (int)grid;
  return p;
}

// ---- what the launcher's routes share -----------------------------------------------------------------------------------------
static int r2l_static_grid(size_t items) {  // the flat kernels: R2L_NT items per workgroup, grid-stride beyond 16384 workgroups
  const size_t g = (items + R2L_NT - 1) / R2L_NT;
  return g > 16384 ? 16384 : (int)g;
}
// the luma plane `cur` through the plan's plane filters, each into the other plane of the pair; `cur` names the result
static int r2l_static_plane_filters(const R2LStaticPlan& p, const R2LStaticArgs& a, double*& cur, double* other, void* stream) {
  for (int i = 0; i < 2; ++i) {
    if (!p.ops[i]) continue;
    R2LPlaneArgs pa;
    pa.src = cur;
    pa.dst = other;
    pa.B = a.B;
    pa.H = a.H;
    pa.W = a.W;
    pa.op = p.ops[i];
    for (int k = 0; k < 5; ++k) pa.gk[k] = a.gk[k];
    for (int k = 0; k < 5; ++k) pa.uk[k] = a.uk[k];
    pa.amount = a.amount;
    if (int e = r2l_launch_plane_filter(pa, r2l_static_grid((size_t)a.B * a.H * a.W / 2), stream)) return e;
    other = cur;
    cur = pa.dst;
  }
  return 0;
}
// fft_denoising, then the rest of the chain: the linear image at rgb_off low-passed along its rows -- bins
// int(c * keep_fraction) <= k < int(c * (1 - keep_fraction)) zeroed (pipeline_numpy.py:229-230; default 0.3) -- then clip, gamma
static int r2l_static_lowpass_finish(const R2LStaticPlan& p, const R2LStaticArgs& a, void* workspace, void* stream) {
  double* rgb = (double*)((char*)workspace + p.rgb_off);
  if (p.fft) {
    const int cut0 = (int)(a.W * p.fft_fraction), cut1 = (int)(a.W * (1 - p.fft_fraction));
#ifdef R2L_EMUL
    r2l_fft_lowpass_rows_host(rgb, p.rows, a.W, cut0, cut1);
#else
    double* spec = (double*)((char*)workspace + p.spec_off);
    void* work = (char*)workspace + p.work_off;
    if (int e = r2l_fft_exec(p.fft_plans.fwd, rgb, spec, work, p.fft_plans.work_bytes, stream)) return e;
    R2LSpecMaskArgs sm{spec, p.rows, a.W, cut0, cut1};
    if (int e = r2l_launch_spec_mask(sm, r2l_static_grid(p.rows * (size_t)(a.W / 2 + 1)), stream)) return e;
    if (int e = r2l_fft_exec(p.fft_plans.inv, spec, rgb, work, p.fft_plans.work_bytes, stream)) return e;
#endif
  }
  R2LStaticFinishArgs fa{a, rgb};
  return r2l_launch_static_finish(fa, r2l_static_grid((size_t)a.B * a.H * a.W / 4), stream);
}

// a plan that is neither refused nor too large, and a workspace of its workspace_bytes
// ep: the map of an epilogue form the plan chose (STREAM / CHAIN), otherwise off
static int r2l_static_launch(const R2LStaticPlan& p, const R2LStaticArgs& a, void* workspace, void* stream,
                             const R2LEpi& ep = R2LEpi{0, 0, 0, 0}) {
  const size_t px = (size_t)a.B * a.H * a.W;
  switch (p.route) {
    case R2L_ROUTE_MENON: {
      R2LMenonArgs ma;
      ma.s = a;
      ma.rgb = (double*)workspace;
      ma.gh = ma.rgb + 3 * px;
      ma.gv = ma.gh + px;
      ma.ch = ma.gv + px;
      ma.cv = ma.ch + px;
      ma.m = ma.cv + px;
      ma.luma = ma.gh;
      ma.want_luma = (p.ops[0] || p.ops[1]) ? 1 : 0;
      for (int i = 0; i < 9; ++i) ma.M1[i] = R2L_YUV_FROM_RGB[i];
      for (int st = 0; st <= 7; ++st) {
        ma.stage = st;
        if (int e = r2l_launch_static_menon(ma, p.grid, stream)) return e;
      }
      if (ma.want_luma) {
        double* cur = ma.gh;  // G_H / G_V are dead behind stage 1: the luma plane and its ping-pong partner
        if (int e = r2l_static_plane_filters(p, a, cur, ma.gv, stream)) return e;
        ma.stage = 8;
        ma.luma = cur;
        if (int e = r2l_launch_static_menon(ma, p.grid, stream)) return e;
      }
      return r2l_static_lowpass_finish(p, a, workspace, stream);
    }
#ifndef R2L_SERIAL
    case R2L_ROUTE_CHAIN: {
      R2LStaticChainArgs ca;
      ca.s = a;
      ca.nband = p.nband;
      ca.band_h = p.band_h;
      ca.nw = p.nseg;
      ca.ep = ep;
      return p.chain(ca, p.grid, stream);
    }
#endif
    case R2L_ROUTE_PLANES:
    case R2L_ROUTE_STREAM: {
      R2LStaticStreamArgs sa;
      sa.s = a;
      sa.nseg = p.nseg;
      sa.nband = p.nband;
      sa.band_h = p.band_h;
      sa.nitems = p.nitems;
      sa.luma_out = nullptr;
      sa.luma_in = nullptr;
      sa.lin_out = nullptr;
      sa.ep = ep;
      if (p.route == R2L_ROUTE_STREAM) return p.stream(sa, p.grid, stream);
      double* cur = (double*)workspace;
      sa.luma_out = cur;
      if (int e = p.stream(sa, p.grid, stream)) return e;
      if (int e = r2l_static_plane_filters(p, a, cur, (double*)workspace + px, stream)) return e;
      sa.luma_out = nullptr;
      sa.luma_in = cur;
      if (!p.fft) return p.stream(sa, p.grid, stream);
      // fft_denoising: the sharpened RGB as float64 planes instead of the output
      sa.lin_out = (double*)((char*)workspace + p.rgb_off);
      if (int e = p.stream(sa, p.grid, stream)) return e;
      return r2l_static_lowpass_finish(p, a, workspace, stream);
    }
    case R2L_ROUTE_FULL:
      return r2l_launch_static_full(a, p.grid, stream);
    default:
      return r2l_launch_static_short(a, p.grid, stream);
  }
}

// the six r2l_static_fwd* entries: one implementation, what they ask of it
struct R2LStaticCall {
  const void* raw;  // the frames as the entries take them: pointer, R2L_FRAMES_*, denom (read for 16-bit containers)
  int frames;
  float denom;
  float* out;  // (io != R2L_IO_F32: 2-byte elements, and r2l_static_io_why has said that a 16-bit kernel serves the call)
  int io, B, H, W;
  const double* camera_host;
  int debayer, sharpening, denoising;
  double gamma;
  const float* mean_std_host;  // or null
  R2LStaticOpts opt;
  void* workspace;
  size_t workspace_bytes;
  void* stream;
  double* sums = nullptr;  // r2l_static_stats (io = R2L_IO_STATS, out = null): double[7], instead of an output
  // r2l_static_fwd_epilogue: where the output goes, as R2L_STEP_EPI_* bits; the affine map R2LEpi follows from them and the frame
  // size (r2l_epi_from_phase) once the plan has said that an epilogue form serves the call.  0: none
  int epilogue = 0;
};
// the partials a statistics launch left in the workspace -> sums[0..5], the pixel count -> sums[6]
static int r2l_static_sums_finish(const R2LStaticPlan& p, const R2LStaticCall& c) {
  R2LSumsFinishArgs f{(const double*)c.workspace, p.nparts, 6, (double)c.B * (double)c.H * (double)c.W, c.sums};
  return r2l_launch_sums_finish(f, 1, c.stream);
}
static int r2l_static_fwd_impl(const R2LStaticCall& c) {
  if (c.frames != R2L_FRAMES_F32 && c.frames != R2L_FRAMES_U16 && c.frames != R2L_FRAMES_F64)
    return r2l_fail(-1, "r2l_static_fwd_norm: frames must be R2L_FRAMES_F32, _U16 or _F64");
  const R2LRaw raw = c.frames == R2L_FRAMES_F64 ? r2l_raw_f64((const double*)c.raw)
                                                : r2l_raw_any(c.raw, c.frames == R2L_FRAMES_U16, c.denom);
  if (int e = r2l_check_dims(c.B, c.H, c.W)) return e;
  if (int e = r2l_check_raw(raw, c.W, "r2l_static_fwd")) return e;
  if (c.mean_std_host)
    for (int k = 0; k < 3; ++k)
      if (!(c.mean_std_host[3 + k] != 0.f)) return r2l_fail(-1, "r2l_static_fwd_norm: std must be non-zero");
  if (!(c.io == R2L_IO_STATS ? (void*)c.sums : (void*)c.out) || !c.camera_host) return r2l_fail(-1, "r2l_static_fwd: null pointer");
  if (c.debayer != R2L_DEBAYER_BILINEAR && c.debayer != R2L_DEBAYER_MALVAR2004 && c.debayer != R2L_DEBAYER_MENON2007)
    return r2l_fail(-1, "r2l_static_fwd: unknown debayer");
  if (c.sharpening != R2L_SHARPEN_NONE && c.sharpening != R2L_SHARPEN_FILTER && c.sharpening != R2L_SHARPEN_UNSHARP)
    return r2l_fail(-1, "r2l_static_fwd: unknown sharpening");
  if (c.denoising != R2L_DENOISE_NONE && c.denoising != R2L_DENOISE_GAUSSIAN && c.denoising != R2L_DENOISE_MEDIAN &&
      c.denoising != R2L_DENOISE_FFT)
    return r2l_fail(-4, "r2l_static_fwd: denoising must be none, gaussian_denoising, median_denoising or fft_denoising");
  if (!(c.gamma > 0)) return r2l_fail(-1, "r2l_static_fwd: gamma must be > 0");
  if (const char* why = r2l_static_opts_problem(c.opt, c.sharpening, c.denoising))
    return r2l_fail(-4, std::string("r2l_static_fwd: ") + why);
  R2LStaticArgs a;
  // (the statistics forms store nothing: their `out` is where each wavefront leaves its partial, the workspace)
  r2l_static_setup(a, raw, c.io == R2L_IO_STATS ? (float*)c.workspace : c.out, c.B, c.H, c.W, c.camera_host, c.debayer, c.sharpening,
                   c.denoising, c.gamma, c.mean_std_host, c.opt);
  const R2LStaticPlan p = r2l_static_plan(c.frames, c.B, c.H, c.W, c.debayer, c.sharpening, c.denoising, c.opt, c.io, true, c.epilogue);
  if (p.no_epi) return r2l_fail(-3, std::string("r2l_static_fwd_epilogue: an output epilogue is not served here: ") + p.no_epi);
  R2LEpi ep = R2LEpi{0, 0, 0, 0};
  if (c.epilogue)
    if (int e = r2l_epi_from_phase(c.epilogue, c.H, c.W, ep)) return e;
  if (c.io == R2L_IO_STATS && p.no_stats)
    return r2l_fail(-3, std::string("r2l_static_stats: not served here: ") + p.no_stats);
  if (c.io != R2L_IO_F32 && c.io != R2L_IO_STATS && p.no_io)
    return r2l_fail(-3, "r2l_static_fwd_io: no 16-bit form of the kernels this call takes (r2l_static_io_supported)");
  if (p.refused) return r2l_fail(-4, p.refused);
  if (p.err) return p.err;
  if (p.workspace_bytes && (!c.workspace || c.workspace_bytes < p.workspace_bytes))
    return r2l_fail(-2, "r2l_static_fwd: workspace too small (r2l_static_workspace_bytes)");
  if (p.too_large) return r2l_fail(-1, "r2l_static_fwd: batch too large");
  if (int e = r2l_static_launch(p, a, c.workspace, c.stream, ep)) return e;
  return c.io == R2L_IO_STATS ? r2l_static_sums_finish(p, c) : 0;
}

int r2l_raw2rgb_fwd(const float* raw, const float* black_level, float* out, int B, int H, int W,
                    int reduce_size, int out_channels, void* stream) {
  return r2l_raw2rgb_fwd_impl(r2l_raw_f32(raw), black_level, out, B, H, W, reduce_size, out_channels, stream);
}
int r2l_raw2rgb_fwd_u16(const unsigned short* raw, float denom, const float* black_level, float* out, int B,
                        int H, int W, int reduce_size, int out_channels, void* stream) {
  return r2l_raw2rgb_fwd_impl(r2l_raw_u16(raw, denom), black_level, out, B, H, W, reduce_size, out_channels,
                              stream);
}
size_t r2l_static_workspace_bytes(int B, int H, int W, int debayer, int sharpening, int denoising) {
  return r2l_static_plan(R2L_FRAMES_F32, B, H, W, debayer, sharpening, denoising, R2LStaticOpts(), R2L_IO_F32)
      .workspace_bytes;
}
size_t r2l_static_workspace_bytes_f64(int B, int H, int W, int debayer, int sharpening, int denoising) {
  return r2l_static_plan(R2L_FRAMES_F64, B, H, W, debayer, sharpening, denoising, R2LStaticOpts(), R2L_IO_F32)
      .workspace_bytes;
}
size_t r2l_static_workspace_bytes_opts(int frames, int B, int H, int W, int debayer, int sharpening, int denoising,
                                       const double* options_host) {
  return r2l_static_plan(frames, B, H, W, debayer, sharpening, denoising, r2l_static_opts(options_host, 3), R2L_IO_F32)
      .workspace_bytes;
}
int r2l_static_fwd_f64(const double* raw, float* out, int B, int H, int W, const double* camera_host,
                       int debayer, int sharpening, int denoising, double gamma, void* workspace,
                       size_t workspace_bytes, void* stream) {
  return r2l_static_fwd_impl(R2LStaticCall{raw, R2L_FRAMES_F64, 1.f, out, R2L_IO_F32, B, H, W, camera_host, debayer, sharpening,
                                           denoising, gamma, nullptr, R2LStaticOpts(), workspace, workspace_bytes, stream});
}
int r2l_static_fwd(const float* raw, float* out, int B, int H, int W, const double* camera_host,
                   int debayer, int sharpening, int denoising, double gamma, void* workspace,
                   size_t workspace_bytes, void* stream) {
  return r2l_static_fwd_impl(R2LStaticCall{raw, R2L_FRAMES_F32, 1.f, out, R2L_IO_F32, B, H, W, camera_host, debayer, sharpening,
                                           denoising, gamma, nullptr, R2LStaticOpts(), workspace, workspace_bytes, stream});
}
int r2l_static_fwd_u16(const unsigned short* raw, float denom, float* out, int B, int H, int W,
                       const double* camera_host, int debayer, int sharpening, int denoising, double gamma,
                       void* workspace, size_t workspace_bytes, void* stream) {
  return r2l_static_fwd_impl(R2LStaticCall{raw, R2L_FRAMES_U16, denom, out, R2L_IO_F32, B, H, W, camera_host, debayer, sharpening,
                                           denoising, gamma, nullptr, R2LStaticOpts(), workspace, workspace_bytes, stream});
}
int r2l_static_fwd_norm(const void* raw, int frames, float denom, float* out, int B, int H, int W,
                        const double* camera_host, int debayer, int sharpening, int denoising, double gamma,
                        const float* mean_std_host, void* workspace, size_t workspace_bytes, void* stream) {
  return r2l_static_fwd_impl(R2LStaticCall{raw, frames, denom, out, R2L_IO_F32, B, H, W, camera_host, debayer, sharpening, denoising,
                                           gamma, mean_std_host, R2LStaticOpts(), workspace, workspace_bytes, stream});
}
int r2l_static_fwd_opts(const void* raw, int frames, float denom, float* out, int B, int H, int W,
                        const double* camera_host, int debayer, int sharpening, int denoising, double gamma,
                        const double* options_host, const float* mean_std_host, void* workspace, size_t workspace_bytes,
                        void* stream) {
  return r2l_static_fwd_impl(R2LStaticCall{raw, frames, denom, out, R2L_IO_F32, B, H, W, camera_host, debayer, sharpening, denoising,
                                           gamma, mean_std_host, r2l_static_opts(options_host), workspace, workspace_bytes, stream});
}

// ---- 16-bit output of the static chains (include/r2l_isp.h: r2l_static_fwd_io) -------------------------------------------------
// why a 16-bit call is not served, or null: the plan's answer, for r2l_static_io_supported and r2l_static_fwd_io alike
static const char* r2l_static_io_why(int frames, int H, int W, int debayer, int sharpening, int denoising, const R2LStaticOpts& opt) {
  return r2l_static_plan(frames, 1, H, W, debayer, sharpening, denoising, opt, R2L_IO_BF16, false).no_io;
}
const char* r2l_static_io_supported(int frames, int H, int W, int debayer, int sharpening, int denoising, const double* options_host) {
  return r2l_static_io_why(frames, H, W, debayer, sharpening, denoising, r2l_static_opts(options_host));
}
// r2l_static_fwd_io and r2l_static_fwd_epilogue (epilogue: R2L_STEP_EPI_* bits, 0 for the former)
static int r2l_static_fwd_io_impl(const void* raw, int frames, float denom, void* out, int out_io, int B, int H, int W,
                                  const double* camera_host, int debayer, int sharpening, int denoising, double gamma,
                                  const double* options_host, const float* mean_std_host, void* workspace, size_t workspace_bytes,
                                  void* stream, int epilogue) {
  if (out_io != R2L_IO_F32 && out_io != R2L_IO_BF16 && out_io != R2L_IO_F16)
    return r2l_fail(-1, "r2l_static_fwd_io: out_io must be one of R2L_IO_*");
  R2LStaticCall c{raw, frames, denom, (float*)out, out_io, B, H, W, camera_host, debayer, sharpening, denoising, gamma, mean_std_host,
                  r2l_static_opts(options_host), workspace, workspace_bytes, stream};
  c.epilogue = epilogue;
  if (epilogue)
    if (const char* why = r2l_static_plan(frames, 1, H, W, debayer, sharpening, denoising, c.opt, out_io, false, epilogue).no_epi)
      return r2l_fail(-3, std::string("r2l_static_fwd_epilogue: an output epilogue is not served here: ") + why);
  if (out_io != R2L_IO_F32) {
    if (const char* why = r2l_static_io_why(frames, H, W, debayer, sharpening, denoising, c.opt))
      return r2l_fail(-3, std::string("r2l_static_fwd_io: a 16-bit output is not served here: ") + why);
    if ((uintptr_t)out % 8) return r2l_fail(-1, "r2l_static_fwd_io: the 16-bit output must be 8-byte aligned");
  }
  if (epilogue && out_io == R2L_IO_F32 && (uintptr_t)out % 16)
    return r2l_fail(-1, "r2l_static_fwd_epilogue: the float32 output must be 16-byte aligned");
  return r2l_static_fwd_impl(c);
}
int r2l_static_fwd_io(const void* raw, int frames, float denom, void* out, int out_io, int B, int H, int W,
                      const double* camera_host, int debayer, int sharpening, int denoising, double gamma,
                      const double* options_host, const float* mean_std_host, void* workspace, size_t workspace_bytes,
                      void* stream) {
  return r2l_static_fwd_io_impl(raw, frames, denom, out, out_io, B, H, W, camera_host, debayer, sharpening, denoising, gamma, options_host,
                                mean_std_host, workspace, workspace_bytes, stream, 0);
}

// ---- output epilogue of the static chains (include/r2l_isp.h: r2l_static_fwd_epilogue) ---------------------------------------------
const char* r2l_static_epilogue_supported(int frames, int H, int W, int debayer, int sharpening, int denoising, const double* options_host,
                                          int out_io, int epilogue) {
  if (out_io != R2L_IO_F32 && out_io != R2L_IO_BF16 && out_io != R2L_IO_F16) return "out_io must be one of R2L_IO_*";
  if (epilogue & ~R2L_STEP_EPI_MASK) return "epilogue holds bits outside R2L_STEP_EPI_*";
  const R2LStaticPlan p = r2l_static_plan(frames, 1, H, W, debayer, sharpening, denoising, r2l_static_opts(options_host), out_io, false, epilogue);
  return (epilogue & R2L_STEP_EPI_MASK) ? p.no_epi : (out_io != R2L_IO_F32 ? p.no_io : nullptr);
}
int r2l_static_fwd_epilogue(const void* raw, int frames, float denom, void* out, int out_io, int B, int H, int W,
                            const double* camera_host, int debayer, int sharpening, int denoising, double gamma,
                            const double* options_host, const float* mean_std_host, void* workspace, size_t workspace_bytes,
                            void* stream, int epilogue) {
  if (epilogue & ~R2L_STEP_EPI_MASK) return r2l_fail(-1, "r2l_static_fwd_epilogue: epilogue holds bits outside R2L_STEP_EPI_*");
  return r2l_static_fwd_io_impl(raw, frames, denom, out, out_io, B, H, W, camera_host, debayer, sharpening, denoising, gamma, options_host,
                                mean_std_host, workspace, workspace_bytes, stream, epilogue);
}

// ---- channel statistics (include/r2l_isp.h: r2l_static_stats, r2l_channel_sums) ---------------------------------------------------
const char* r2l_static_stats_supported(int frames, int H, int W, int debayer, int sharpening, int denoising, const double* options_host) {
  return r2l_static_plan(frames, 1, H, W, debayer, sharpening, denoising, r2l_static_opts(options_host), R2L_IO_STATS, false).no_stats;
}
size_t r2l_static_stats_workspace_bytes(int frames, int B, int H, int W, int debayer, int sharpening, int denoising,
                                        const double* options_host) {
  const R2LStaticPlan p = r2l_static_plan(frames, B, H, W, debayer, sharpening, denoising, r2l_static_opts(options_host, 3), R2L_IO_STATS, false);
  return p.no_stats ? 0 : p.workspace_bytes;
}
int r2l_static_stats(const void* raw, int frames, float denom, double* sums, int B, int H, int W, const double* camera_host, int debayer,
                     int sharpening, int denoising, double gamma, const double* options_host, void* workspace, size_t workspace_bytes,
                     void* stream) {
  R2LStaticCall c{raw, frames, denom, nullptr, R2L_IO_STATS, B, H, W, camera_host, debayer, sharpening, denoising, gamma, nullptr,
                  r2l_static_opts(options_host), workspace, workspace_bytes, stream};
  c.sums = sums;
  return r2l_static_fwd_impl(c);
}
// the shares of r2l_channel_sums and where its 16-byte vectors start, from the shape and the pointer's alignment alone
static R2LChannelSumsArgs r2l_channel_sums_args(const float* x, int B, int C, int H, int W) {
  R2LChannelSumsArgs a = {};
  a.x = x;
  a.hw = (size_t)H * W;
  a.n = (size_t)B * C * a.hw;
  a.C = C;
  a.head = (size_t)((16 - (uintptr_t)x % 16) % 16) / 4;
  if (a.head > a.n) a.head = a.n;
  a.nvec = (a.n - a.head) / 4;
  const size_t nv = (a.nvec + R2L_NT - 1) / R2L_NT;
  a.nv = nv > R2L_SUMS_MAX_SHARES ? R2L_SUMS_MAX_SHARES : (nv < 1 ? 1 : (int)nv);
  return a;
}
size_t r2l_channel_sums_workspace_bytes(int B, int C, int H, int W) {
  if (B < 1 || C < 1 || C > 4 || H < 1 || W < 1) return 0;
  // (an unaligned tensor has at most one vector less than an aligned one: the aligned count bounds the shares)
  return sizeof(double) * 2 * C * (size_t)r2l_channel_sums_args(nullptr, B, C, H, W).nv;
}
int r2l_channel_sums(const float* x, double* sums, int B, int C, int H, int W, void* workspace, size_t workspace_bytes, void* stream) {
  if (!x || !sums) return r2l_fail(-1, "r2l_channel_sums: null pointer");
  if (B < 1 || C < 1 || C > 4 || H < 1 || W < 1) return r2l_fail(-1, "r2l_channel_sums: needs B, H, W >= 1 and 1 <= C <= 4");
  if ((uintptr_t)x % 4) return r2l_fail(-1, "r2l_channel_sums: x must be 4-byte aligned");
  if ((double)B * C * H * W > 1099511627776.0) return r2l_fail(-1, "r2l_channel_sums: tensor too large");
  R2LChannelSumsArgs a = r2l_channel_sums_args(x, B, C, H, W);
  if (!workspace || workspace_bytes < r2l_channel_sums_workspace_bytes(B, C, H, W))
    return r2l_fail(-2, "r2l_channel_sums: workspace too small (r2l_channel_sums_workspace_bytes)");
  a.partial = (double*)workspace;
  if (int e = r2l_launch_channel_sums(a, r2l_flat_grid((size_t)a.nv), stream)) return e;
  R2LSumsFinishArgs f{a.partial, a.nv, 2 * C, (double)B * (double)H * (double)W, sums};
  return r2l_launch_sums_finish(f, 1, stream);
}

// ---- staged (track_stages=True) entry points -------------------------------------------------------
size_t r2l_stage_workspace_bytes(void) { return sizeof(float) * 81 * R2L_MAX_BLOCKS + 256; }

static int r2l_stage_shares(int B, int H, int W, int per_thread) {  // the grid the shape asks for
  const size_t n = (size_t)B * H * W / per_thread;
  size_t g = (n + R2L_NT - 1) / R2L_NT;
  if (g > R2L_MAX_BLOCKS) g = R2L_MAX_BLOCKS;
  return g < 1 ? 1 : (int)g;
}
static int r2l_stage_grid(int B, int H, int W, int per_thread) {
  return r2l_flat_grid((size_t)r2l_stage_shares(B, H, W, per_thread));
}
static int r2l_stage_finish(const float* partial, int nslots, int grid, float* out, void* stream) {
  R2LReduceRowsArgs r{partial, nullptr, grid, 1.0, out};
  return r2l_launch_reduce_rows(r, nslots, stream);
}

int r2l_stage_conv33_fwd(const float* x, const float* w, float* y, int B, int H, int W, void* stream) {
  if (int e = r2l_check_dims(B, H, W)) return e;
  if (!x || !w || !y) return r2l_fail(-1, "r2l_stage_conv33_fwd: null pointer");
  R2LStageArgs a{x, nullptr, w, nullptr, y, nullptr, B, H, W, 3, 1};
  return r2l_launch_conv33_fwd(a, r2l_stage_grid(B, H, W, 1), stream);
}
int r2l_stage_conv33_bwd(const float* x, const float* w, const float* g, float* gx, float* gw, void* workspace,
                         size_t workspace_bytes, int B, int H, int W, void* stream) {
  if (int e = r2l_check_dims(B, H, W)) return e;
  if (!x || !w || !g || !gw || !workspace) return r2l_fail(-1, "r2l_stage_conv33_bwd: null pointer");
  if (workspace_bytes < r2l_stage_workspace_bytes()) return r2l_fail(-2, "r2l_stage: workspace too small");
  const int grid = r2l_stage_grid(B, H, W, 1);
  R2LStageArgs a{x, g, w, nullptr, gx, (float*)workspace, B, H, W, 3, 1};
  if (int e = r2l_launch_conv33_bwd(a, grid, stream)) return e;
  return r2l_stage_finish((const float*)workspace, 81, grid, gw, stream);
}
int r2l_stage_mix3_fwd(const float* x, const float* m, float* y, int B, int H, int W, void* stream) {
  if (int e = r2l_check_dims(B, H, W)) return e;
  if (!x || !m || !y) return r2l_fail(-1, "r2l_stage_mix3_fwd: null pointer");
  R2LStageArgs a{x, nullptr, m, nullptr, y, nullptr, B, H, W, 0, 0};
  return r2l_launch_mix3_fwd(a, r2l_stage_grid(B, H, W, 1), stream);
}
int r2l_stage_mix3_bwd(const float* x, const float* m, const float* g, float* gx, float* gm, void* workspace,
                       size_t workspace_bytes, int B, int H, int W, void* stream) {
  if (int e = r2l_check_dims(B, H, W)) return e;
  if (!m || !g || !workspace) return r2l_fail(-1, "r2l_stage_mix3_bwd: null pointer");
  if (gm && !x) return r2l_fail(-1, "r2l_stage_mix3_bwd: the matrix gradient needs the forward input");
  if (workspace_bytes < r2l_stage_workspace_bytes()) return r2l_fail(-2, "r2l_stage: workspace too small");
  const int grid = r2l_stage_grid(B, H, W, 1);
  R2LStageArgs a{gm ? x : nullptr, g, m, nullptr, gx, (float*)workspace, B, H, W, 0, 0};
  if (int e = r2l_launch_mix3_bwd(a, grid, stream)) return e;
  return gm ? r2l_stage_finish((const float*)workspace, 9, grid, gm, stream) : 0;
}
int r2l_stage_pconv_fwd(const float* x, const float* k, float* y, int K, int mirror, int B, int H, int W,
                        void* stream) {
  if (int e = r2l_check_dims(B, H, W)) return e;
  if (!x || !k || !y || (K != 3 && K != 5)) return r2l_fail(-1, "r2l_stage_pconv_fwd: bad argument");
  R2LStageArgs a{x, nullptr, k, nullptr, y, nullptr, B, H, W, K, mirror};
  return r2l_launch_pconv_fwd(a, r2l_stage_grid(B, H, W, 1), stream);
}
int r2l_stage_pconv_bwd(const float* x, const float* k, const float* g, float* gx, float* gk25, int K,
                        int mirror, void* workspace, size_t workspace_bytes, int B, int H, int W,
                        void* stream) {
  if (int e = r2l_check_dims(B, H, W)) return e;
  if (!x || !k || !g || !gk25 || !workspace || (K != 3 && K != 5))
    return r2l_fail(-1, "r2l_stage_pconv_bwd: bad argument");
  if (workspace_bytes < r2l_stage_workspace_bytes()) return r2l_fail(-2, "r2l_stage: workspace too small");
  const int grid = r2l_stage_grid(B, H, W, 1);
  R2LStageArgs a{x, g, k, nullptr, gx, (float*)workspace, B, H, W, K, mirror};
  if (int e = r2l_launch_pconv_bwd(a, grid, stream)) return e;
  return r2l_stage_finish((const float*)workspace, 25, grid, gk25, stream);
}
int r2l_stage_point(int op, const float* x, const float* g, const float* w, const float* aux,
                    const float* aux2, float* y, float* sums6, void* workspace, size_t workspace_bytes,
                    int B, int H, int W, void* stream) {
  if (int e = r2l_check_dims(B, H, W)) return e;
  if (op < 0 || op > 8) return r2l_fail(-1, "r2l_stage_point: unknown op");
  const bool reduces = (op == 3 || op == 7);
  if (reduces && (!sums6 || !workspace || workspace_bytes < r2l_stage_workspace_bytes()))
    return r2l_fail(-2, "r2l_stage_point: reduction needs sums + workspace");
  const int shares = r2l_stage_shares(B, H, W * 3, 4), grid = r2l_stage_grid(B, H, W * 3, 4);
  R2LPointArgs a{x, g, w, aux, aux2, y, reduces ? (float*)workspace : nullptr, B, H, W, op, shares};
  if (int e = r2l_launch_point(a, grid, stream)) return e;
  return reduces ? r2l_stage_finish((const float*)workspace, 6, shares, sums6, stream) : 0;
}

// ---- augmentation after the ISP (utils/augmentation.py) -------------------------------------------------
int r2l_augment(const float* x, float* y, int N, int H, int W, int hflip, int vflip, int k, int inverse,
                void* stream) {
  if (!x || !y || N < 1 || H < 1 || W < 1) return r2l_fail(-1, "r2l_augment: null pointer / bad dimensions");
  if ((H & 3) == 0 && (W & 3) == 0 && (hflip || vflip || (k & 3))) {
    // 16 bytes at a time, transposes through LDS tiles (r2l_aug_tiled_block)
    const int Wo = (k & 1) ? H : W;
    int r0, c0, r1, c1, r2, c2;
    r2l_aug_map(H, W, hflip != 0, vflip != 0, k & 3, 0, 0, r0, c0);
    r2l_aug_map(H, W, hflip != 0, vflip != 0, k & 3, 1, 0, r1, c1);
    r2l_aug_map(H, W, hflip != 0, vflip != 0, k & 3, 0, 1, r2, c2);
    R2LAugTiledArgs t;
    t.x = x;
    t.y = y;
    t.N = N;
    t.H = H;
    t.W = W;
    t.s0 = r0 * Wo + c0;
    t.sr = (r1 * Wo + c1) - t.s0;
    t.sc = (r2 * Wo + c2) - t.s0;
    t.odd = k & 1;
    t.inverse = inverse != 0;
    t.ntr = (H + R2L_AUG_TS - 1) / R2L_AUG_TS;
    t.ntc = (W + R2L_AUG_TS - 1) / R2L_AUG_TS;
    size_t nt = (size_t)N * t.ntr * t.ntc;
    if (nt > (size_t)1 << 30) return r2l_fail(-1, "r2l_augment: batch too large");
    return r2l_launch_aug_tiled(t, r2l_flat_grid(nt < 4096 ? nt : 4096), stream);
  }
  R2LAugArgs a{x, y, N, H, W, hflip != 0, vflip != 0, k & 3, inverse != 0};
  size_t g = ((size_t)N * H * W + R2L_NT - 1) / R2L_NT;
  if (g > 8192) g = 8192;
  return r2l_launch_aug(a, r2l_flat_grid(g), stream);
}
int r2l_add_noise(const float* x, const float* noise, float std, float* y, size_t n, void* stream) {
  if (!x || !noise || !y || n == 0) return r2l_fail(-1, "r2l_add_noise: null pointer / empty");
  R2LAxpyArgs a{x, noise, y, std, n};
  size_t g = (n + R2L_NT - 1) / R2L_NT;
  if (g > 8192) g = 8192;
  return r2l_launch_axpy(a, (int)g, stream);
}
int r2l_add_noise_philox(const float* x, float* y, float std, unsigned long long seed, unsigned long long offset,
                         size_t n, void* stream) {
  if (!x || !y || n == 0) return r2l_fail(-1, "r2l_add_noise_philox: null pointer / empty");
  R2LPhiloxArgs a{x, y, std, seed, offset, n};
  size_t g = ((n + 3) / 4 + R2L_NT - 1) / R2L_NT;
  if (g > 8192) g = 8192;
  return r2l_launch_philox_noise(a, (int)g, stream);
}

// ---- strong augmentation (utils/augmentation.py:77-84; r2l_augment_strong.h) ------------------------------------
static_assert(R2L_NT == (R2L_AUGS_TW / 4) * R2L_AUGS_TH, "one lane per 4 output pixels of the sharpness tile");
static int r2l_strong_geom(const char* who, int N, int C, int H, int W, int hflip, int vflip, int rotate, float txx,
                           float txy, float tyx, float tyy, R2LStrongGeom& g) {
  if (N < 1 || C < 1 || H < 1 || W < 1 || N % C || (size_t)N > ((size_t)1 << 24) || (size_t)H * W > ((size_t)1 << 29))
    return r2l_fail(-1, std::string(who) + ": bad dimensions (N planes, a multiple of C, of H x W)");
  if (rotate && !(isfinite(txx) && isfinite(txy) && isfinite(tyx) && isfinite(tyy)))
    return r2l_fail(-1, std::string(who) + ": non-finite rotation coefficients");
  g = R2LStrongGeom{N, H, W, hflip != 0, vflip != 0, rotate != 0, txx, txy, tyx, tyy};
  return 0;
}
// sharpness in effect?  (adjust_sharpness: C in {1, 3} is checked first, frames of H or W <= 2 come back unchanged)
static int r2l_strong_sharp(const char* who, double sharpness, int C, int H, int W, bool& on) {
  on = false;
  if (sharpness != sharpness) return r2l_fail(-1, std::string(who) + ": sharpness factor is NaN");
  if (sharpness < 0) return 0;
  if (C != 1 && C != 3) return r2l_fail(-1, std::string(who) + ": the sharpness adjustment needs 1 or 3 channels");
  on = H > 2 && W > 2;
  return 0;
}
static int r2l_strong_flat_grid(const R2LStrongGeom& g) {
  const size_t nch = (size_t)g.N * g.H * ((g.W + 3) / 4);
  size_t n = (nch + R2L_NT - 1) / R2L_NT;
  if (n > 8192) n = 8192;
  return r2l_env_int("R2L_GRID_AUGS", (int)n);
}
int r2l_augment_strong_fwd(const float* x, float* y, unsigned char* clamp_mask, int N, int C, int H, int W, int hflip,
                           int vflip, int rotate, float txx, float txy, float tyx, float tyy, float fill, float noise_std,
                           const long long* noise_key, unsigned long long noise_offset, double sharpness, void* stream) {
  const char* who = "r2l_augment_strong_fwd";
  if (!x || !y) return r2l_fail(-1, std::string(who) + ": null pointer");
  R2LStrongArgs a;
  if (int e = r2l_strong_geom(who, N, C, H, W, hflip, vflip, rotate, txx, txy, tyx, tyy, a.g)) return e;
  bool sharp;
  if (int e = r2l_strong_sharp(who, sharpness, C, H, W, sharp)) return e;
  if (!isfinite(fill) || (noise_key && !isfinite(noise_std)))
    return r2l_fail(-1, std::string(who) + ": non-finite fill / noise std");
  a.x = x;
  a.y = y;
  a.mask = sharp ? clamp_mask : nullptr;
  a.key = noise_key;
  a.fill = fill;
  a.std = noise_std;
  a.r = (float)sharpness;
  a.s = (float)(1.0 - sharpness);
  a.offset = noise_offset;
  if (!sharp) return r2l_launch_strong_fwd_flat(a, r2l_strong_flat_grid(a.g), stream);
  const long ntiles = (long)N * ((H + R2L_AUGS_TH - 1) / R2L_AUGS_TH) * ((W + R2L_AUGS_TW - 1) / R2L_AUGS_TW);
  return r2l_launch_strong_fwd_sharp(a, r2l_env_int("R2L_GRID_AUGS", (int)(ntiles < R2L_MAX_BLOCKS ? ntiles : R2L_MAX_BLOCKS)),
                                     stream);
}
int r2l_augment_strong_bwd(const float* grad_y, float* grad_x, const unsigned char* clamp_mask, float* work, int N, int C,
                           int H, int W, int hflip, int vflip, int rotate, float txx, float txy, float tyx, float tyy,
                           double sharpness, void* stream) {
  const char* who = "r2l_augment_strong_bwd";
  if (!grad_y || !grad_x) return r2l_fail(-1, std::string(who) + ": null pointer");
  R2LStrongBwdArgs a;
  if (int e = r2l_strong_geom(who, N, C, H, W, hflip, vflip, rotate, txx, txy, tyx, tyy, a.g)) return e;
  bool sharp;
  if (int e = r2l_strong_sharp(who, sharpness, C, H, W, sharp)) return e;
  if (sharp && (!clamp_mask || !work))
    return r2l_fail(-1, std::string(who) + ": the sharpness adjoint needs the forward's clamp mask and an N*H*W work plane");
  a.gy = grad_y;
  a.mask = clamp_mask;
  a.gv = sharp ? work : (float*)grad_y;
  a.gx = grad_x;
  a.r = (float)sharpness;
  a.s = (float)(1.0 - sharpness);
  const int grid = r2l_strong_flat_grid(a.g);
  if (sharp)
    if (int e = r2l_launch_strong_bwd_sharp(a, grid, stream)) return e;
  return r2l_launch_strong_bwd_rot(a, grid, stream);
}

// ---- common corruptions (utils/hendrycks_robustness.py: Distortions; r2l_corruptions.h) ----------------------------
static_assert(R2L_NT == (R2L_CBLUR_TW / 4) * R2L_CBLUR_TH, "one lane per 4 output pixels of the blur tile");
static const char* const r2l_corrupt_names[R2L_CORRUPT_KINDS] = {"identity",      "gaussian_noise", "shot_noise", "impulse_noise",
                                                                "speckle_noise", "gaussian_blur",  "zoom_blur",  "contrast",
                                                                "brightness",    "saturate"};
size_t r2l_corrupt_workspace_bytes(int kind, int N, int C, int H, int W) {
  if (kind != R2L_CORRUPT_CONTRAST || N < 1 || C != 3 || H < 1 || W < 1) return 0;
  return r2l_align_up(sizeof(float) * 3 * (size_t)N);
}
// workgroups of a pass over `items` work items of one lane each (diagnostic builds: R2L_GRID_CORRUPT)
static int r2l_corrupt_grid(size_t items, size_t per_block, size_t cap) {
  size_t n = (items + per_block - 1) / per_block;
  if (n > cap) n = cap;
  return r2l_env_int("R2L_GRID_CORRUPT", (int)(n < 1 ? 1 : n));
}
int r2l_corrupt(const float* x, float* y, int N, int C, int H, int W, int kind, const double* params_host, int nparams,
                unsigned long long noise_key, unsigned long long noise_offset, const float* mean3, const float* std3,
                void* workspace, size_t workspace_bytes, void* stream) {
  const std::string who = "r2l_corrupt";
  if (kind < 0 || kind >= R2L_CORRUPT_KINDS)
    return r2l_fail(R2L_CORRUPT_E_KIND, who + ": unknown kind " + std::to_string(kind));
  const std::string what = who + "(" + r2l_corrupt_names[kind] + ")";
  if (!x || !y || x == y) return r2l_fail(R2L_CORRUPT_E_ARGS, what + ": null pointer, or y aliases x");
  if (C != 3) return r2l_fail(R2L_CORRUPT_E_CHANNELS, what + ": needs 3 channels (RGB), got C = " + std::to_string(C));
  if (N < 1 || H < 1 || W < 1 || (size_t)H * W > ((size_t)1 << 29) || (size_t)N * 3 * H * W >= ((size_t)1 << 40))
    return r2l_fail(R2L_CORRUPT_E_ARGS, what + ": bad dimensions");
  if ((mean3 == nullptr) != (std3 == nullptr)) return r2l_fail(R2L_CORRUPT_E_ARGS, what + ": mean3 and std3 go together");
  if (nparams < 0 || (nparams > 0 && !params_host)) return r2l_fail(R2L_CORRUPT_E_PARAMS, what + ": params_host is null");
  for (int k = 0; k < nparams; ++k)
    if (!isfinite(params_host[k])) return r2l_fail(R2L_CORRUPT_E_PARAMS, what + ": non-finite parameter");
  R2LCorruptIO io;
  io.x = x;
  io.y = y;
  io.N = N;
  io.H = H;
  io.W = W;
  io.norm = mean3 != nullptr;
  for (int c = 0; c < 3; ++c) {
    io.mean[c] = mean3 ? mean3[c] : 0.0f;
    io.std[c] = std3 ? std3[c] : 1.0f;
  }
  const size_t chunks = (size_t)N * H * ((W + 3) / 4);  // 4 pixels of a row, three channels
  if (kind == R2L_CORRUPT_ZOOM_BLUR) {
    if (H != W)
      return r2l_fail(R2L_CORRUPT_E_NOT_SQUARE, what + ": needs square frames (the reference crops both axes by the height), got " +
                                                    std::to_string(H) + " x " + std::to_string(W));
    if (nparams < 5 || nparams % 5 || nparams / 5 > R2L_CZOOM_MAXF)
      return r2l_fail(R2L_CORRUPT_E_PARAMS, what + ": 5 numbers per zoom factor, 1 to " + std::to_string(R2L_CZOOM_MAXF) + " factors");
    R2LCorruptZoomArgs z;
    z.io = io;
    z.nf = nparams / 5;
    z.denom = (float)(z.nf + 1);
    for (int f = 0; f < R2L_CZOOM_MAXF; ++f) {
      if (f >= z.nf) {
        z.ch[f] = 1;
        z.top[f] = z.trim[f] = 0;
        z.scale[f] = 0.0;
        continue;
      }
      const double* p = params_host + 5 * f;
      const long ch = (long)p[0], top = (long)p[1], out = (long)p[2], trim = (long)p[3];
      const double sc = p[4];
      // the crop lies in the frame, the trimmed window in the zoomed crop, and the largest coordinate at most one step past the crop
      if (ch < 1 || top < 0 || top + ch > H || out < H || trim < 0 || trim + H > out || sc < 0.0 ||
          (double)(out - 1) * sc > (double)ch)
        return r2l_fail(R2L_CORRUPT_E_PARAMS, what + ": zoom factor " + std::to_string(f) + " does not fit the frame");
      z.ch[f] = (int)ch;
      z.top[f] = (int)top;
      z.trim[f] = (int)trim;
      z.scale[f] = sc;
    }
    return r2l_launch_corrupt_zoom(z, r2l_corrupt_grid(3 * chunks, R2L_NT, 8192), stream);
  }
  R2LCorruptArgs a;
  memset(&a, 0, sizeof(a));
  a.io = io;
  a.seed = noise_key;
  a.offset = noise_offset;
  if (kind == R2L_CORRUPT_GAUSSIAN_BLUR) {
    if (nparams < 1 || nparams > R2L_CBLUR_R + 1)
      return r2l_fail(R2L_CORRUPT_E_PARAMS, what + ": 1 to " + std::to_string(R2L_CBLUR_R + 1) + " taps (radius <= " +
                                                std::to_string(R2L_CBLUR_R) + ")");
    a.radius = nparams - 1;
    for (int k = 0; k < nparams; ++k) a.taps[k] = (float)params_host[k];
    const size_t ntiles = (size_t)N * 3 * ((H + R2L_CBLUR_TH - 1) / R2L_CBLUR_TH) * ((W + R2L_CBLUR_TW - 1) / R2L_CBLUR_TW);
    return r2l_launch_corrupt_blur(a, r2l_corrupt_grid(ntiles, 1, 8192), stream);
  }
  const int want = kind == R2L_CORRUPT_IDENTITY ? 0 : (kind == R2L_CORRUPT_SATURATE ? 2 : 1);
  if (nparams != want) return r2l_fail(R2L_CORRUPT_E_PARAMS, what + ": takes " + std::to_string(want) + " parameter(s)");
  a.c0 = want > 0 ? (float)params_host[0] : 0.0f;
  a.c1 = want > 1 ? (float)params_host[1] : 0.0f;
  const int grid = r2l_corrupt_grid(chunks, R2L_NT, 8192);
  switch (kind) {
    case R2L_CORRUPT_IDENTITY:
      return r2l_launch_corrupt_identity(a, grid, stream);
    case R2L_CORRUPT_GAUSSIAN_NOISE:
      return r2l_launch_corrupt_gaussian_noise(a, grid, stream);
    case R2L_CORRUPT_SPECKLE_NOISE:
      return r2l_launch_corrupt_speckle_noise(a, grid, stream);
    case R2L_CORRUPT_SHOT_NOISE:
      if (!(params_host[0] > 0.0)) return r2l_fail(R2L_CORRUPT_E_PARAMS, what + ": c must be positive");
      return r2l_launch_corrupt_shot_noise(a, grid, stream);
    case R2L_CORRUPT_IMPULSE_NOISE: {
      const double c = params_host[0];
      if (c < 0.0 || c > 1.0) return r2l_fail(R2L_CORRUPT_E_PARAMS, what + ": the amount is a probability");
      const double t = c * 4294967296.0 + 0.5;
      a.thresh = t >= 4294967295.0 ? 0xFFFFFFFFu : (unsigned)t;
      return r2l_launch_corrupt_impulse_noise(a, grid, stream);
    }
    case R2L_CORRUPT_BRIGHTNESS:
      return r2l_launch_corrupt_brightness(a, grid, stream);
    case R2L_CORRUPT_SATURATE:
      return r2l_launch_corrupt_saturate(a, grid, stream);
    default:  // R2L_CORRUPT_CONTRAST: the plane means into the workspace, then the apply pass
      if (!workspace || workspace_bytes < r2l_corrupt_workspace_bytes(kind, N, C, H, W))
        return r2l_fail(R2L_CORRUPT_E_WORKSPACE, what + ": workspace null or smaller than r2l_corrupt_workspace_bytes()");
      a.means = (float*)workspace;
      if (int e = r2l_launch_corrupt_mean(a, r2l_corrupt_grid((size_t)N * 3, 1, R2L_MAX_BLOCKS), stream)) return e;
      return r2l_launch_corrupt_contrast(a, grid, stream);
  }
}

// ---- adversarial auxiliary losses (utils/ssim.py, utils/base.py:342-358) -------------------------------
static void r2l_ssim_gauss(float* g) {  // utils/ssim.py:9-11, float32 like torch.Tensor([...]) / sum
  float w[R2L_SSIM_K], sum = 0.f;
  for (int x = 0; x < R2L_SSIM_K; ++x) {
    const double d = x - R2L_SSIM_K / 2;
    w[x] = (float)exp(-(d * d) / (2.0 * 1.5 * 1.5));
    sum += w[x];
  }
  for (int x = 0; x < R2L_SSIM_K; ++x) g[x] = w[x] / sum;
}
size_t r2l_aux_workspace_bytes(int B, int C, int H, int W) {
  if (B < 1 || C < 1 || H < 1 || W < 1) return 0;
  return r2l_align_up(sizeof(float) * R2L_MAX_BLOCKS) + sizeof(float) * 3 * (size_t)B * C * H * W;
}
static int r2l_aux_check(const void* a, const void* b, int B, int C, int H, int W, const char* who) {
  if (!a || !b) return r2l_fail(-1, std::string(who) + ": null pointer");
  if (B < 1 || C < 1 || H < 1 || W < 1 || (size_t)B * C > (1u << 24) || (size_t)H * W > ((size_t)1 << 29))
    return r2l_fail(-1, std::string(who) + ": bad dimensions");
  return 0;
}
// workgroups of the two persistent SSIM kernels: one per 64x64 tile up to 512, which then walk the rest.  Diagnostic builds
// take R2L_GRID_AUX instead (at most R2L_MAX_BLOCKS: the partials), so that tests can run the walk on a few dozen tiles.
static int r2l_ssim_grid(int B, int C, int H, int W) {
  const int ntiles = B * C * ((H + R2L_SSIM_T - 1) / R2L_SSIM_T) * ((W + R2L_SSIM_T - 1) / R2L_SSIM_T);
  const int g = r2l_env_int("R2L_GRID_AUX", ntiles < 512 ? ntiles : 512);
  return g < R2L_MAX_BLOCKS ? g : R2L_MAX_BLOCKS;
}
// workgroups of the grid-stride L2 kernel: one per 512 lanes x 4 floats up to `cap` (R2L_GRID_AUX: as above)
static int r2l_l2_grid(size_t n, size_t cap) {
  size_t g = (n / 4 + R2L_NT - 1) / R2L_NT;
  if (g > cap) g = cap;
  g = (size_t)r2l_env_int("R2L_GRID_AUX", (int)g);
  return (int)(g < cap ? g : cap);
}
static int r2l_ssim_launch(const float* img1, const float* img2, float* partial, float* dmaps, int mode, int B,
                           int C, int H, int W, void* stream, int* grid_out) {
  R2LSsimArgs a;
  a.img1 = img1;
  a.img2 = img2;
  r2l_ssim_gauss(a.g);
  a.partial = partial;
  a.dmaps = dmaps;
  a.nplanes = B * C;
  a.H = H;
  a.W = W;
  a.mode = mode;
  *grid_out = r2l_ssim_grid(B, C, H, W);
  return r2l_launch_ssim(a, *grid_out, stream);
}
int r2l_ssim_fwd(const float* img1, const float* img2, double* ssim_mean, void* workspace, size_t workspace_bytes,
                 int keep_for_backward, int B, int C, int H, int W, void* stream) {
  if (int e = r2l_aux_check(img1, img2, B, C, H, W, "r2l_ssim_fwd")) return e;
  if (!ssim_mean || !workspace || workspace_bytes < r2l_aux_workspace_bytes(B, C, H, W))
    return r2l_fail(-2, "r2l_ssim_fwd: workspace too small / null output");
  float* partial = (float*)workspace;
  float* dmaps = (float*)((char*)workspace + r2l_align_up(sizeof(float) * R2L_MAX_BLOCKS));
  int grid = 0;
  if (int e = r2l_ssim_launch(img1, img2, partial, dmaps, keep_for_backward ? 3 : 1, B, C, H, W, stream, &grid))
    return e;
  R2LReduceRowsArgs r{partial, ssim_mean, grid, 1.0 / ((double)B * C * H * W), nullptr};
  return r2l_launch_reduce_rows(r, 1, stream);
}
int r2l_ssim_bwd(const float* img1, const float* img2, const float* grad_ssim, float* grad_img2, void* workspace,
                 size_t workspace_bytes, int workspace_has_dmaps, int B, int C, int H, int W, void* stream) {
  if (int e = r2l_aux_check(img1, img2, B, C, H, W, "r2l_ssim_bwd")) return e;
  if (!grad_ssim || !grad_img2 || !workspace || workspace_bytes < r2l_aux_workspace_bytes(B, C, H, W))
    return r2l_fail(-2, "r2l_ssim_bwd: workspace too small / null pointer");
  float* dmaps = (float*)((char*)workspace + r2l_align_up(sizeof(float) * R2L_MAX_BLOCKS));
  int grid = 0;
  if (!workspace_has_dmaps) {
    if (int e = r2l_ssim_launch(img1, img2, nullptr, dmaps, 2, B, C, H, W, stream, &grid)) return e;
  } else {
    grid = r2l_ssim_grid(B, C, H, W);
  }
  R2LSsimBwdArgs b;
  b.img1 = img1;
  b.img2 = img2;
  b.dmaps = dmaps;
  b.gup = grad_ssim;
  b.scale = (float)(1.0 / ((double)B * C * H * W));
  b.grad = grad_img2;
  r2l_ssim_gauss(b.g);
  b.nplanes = B * C;
  b.H = H;
  b.W = W;
  return r2l_launch_ssim_bwd(b, grid, stream);
}
int r2l_l2_fwd(const float* x, const float* y, double* sum, void* workspace, size_t workspace_bytes, size_t n,
               void* stream) {
  if (!x || !y || !sum || !workspace) return r2l_fail(-1, "r2l_l2_fwd: null pointer");
  if (n == 0 || (n & 3)) return r2l_fail(-1, "r2l_l2_fwd: the element count must be a positive multiple of 4");
  if (workspace_bytes < sizeof(float) * R2L_MAX_BLOCKS) return r2l_fail(-2, "r2l_l2_fwd: workspace too small");
  const int g = r2l_l2_grid(n, R2L_MAX_BLOCKS);
  R2LL2Args a{x, y, nullptr, nullptr, (float*)workspace, n};
  if (int e = r2l_launch_l2(a, g, stream)) return e;
  R2LReduceRowsArgs r{a.partial, sum, g, 1.0, nullptr};
  return r2l_launch_reduce_rows(r, 1, stream);
}
int r2l_l2_bwd(const float* x, const float* y, const float* grad_sum, float* grad_y, size_t n, void* stream) {
  if (!x || !y || !grad_sum || !grad_y) return r2l_fail(-1, "r2l_l2_bwd: null pointer");
  if (n == 0 || (n & 3)) return r2l_fail(-1, "r2l_l2_bwd: the element count must be a positive multiple of 4");
  R2LL2Args a{x, y, grad_sum, grad_y, nullptr, n};
  return r2l_launch_l2(a, r2l_l2_grid(n, 4096), stream);
}

#ifdef R2L_TEST_HOOKS
// diagnostic builds: where the per-phase cycle stamps of -DR2L_EXP_STAMPS builds land in the workspace (tests/stamps.py)
#if defined(R2L_EXP_STAMPS) && !defined(R2L_EMUL)
int r2l_test_tail_stamps(unsigned long long* out32) {  // (tests/tail_timeline.py)
  return (int)hipMemcpyFromSymbol(out32, HIP_SYMBOL(r2l_tail_ts), sizeof(unsigned long long) * 32);
}
#endif
size_t r2l_test_debug_offset(int B, int H, int W) {
  const R2LWorkspace ws = r2l_carve((void*)0, B, H, W);
  return (size_t)((char*)ws.debug - (char*)0);
}
#ifdef R2L_EMUL
// the Poisson sampler of shot_noise on chosen Philox outputs (tests feed it the smallest and the largest): below lambda = 10 the
// inversion walk's k from `ou`; from 10 on one PTRS candidate from (ou, ov): its k when accepted, else -1
float r2l_test_corrupt_poisson(float lam, unsigned ou, unsigned ov) {
  if (!(lam > 0.0f)) return 0.0f;
  if (lam < 10.0f) return r2l_corrupt_poisson_walk(lam, ou);
  float k;
  return r2l_corrupt_ptrs_try(r2l_corrupt_ptrs_setup(lam), ou, ov, k) ? k : -1.0f;
}
// the tile walk of the persistent kernels, replayed on the host: owner[tile] = workgroup id that visits it (or -1), and
// the number of visits per tile in visits[tile]; returns the largest number of tiles any workgroup takes
int r2l_test_tile_walk(int B, int H, int W, int nblk, int* owner, int* visits) {
  const int ntx = (W + 63) / 64, nty = (H + 63) / 64, ntiles = B * ntx * nty;
  for (int i = 0; i < ntiles; ++i) {
    owner[i] = -1;
    visits[i] = 0;
  }
  int most = 0;
  for (int bid = 0; bid < nblk; ++bid) {
    R2LTileWalk w = r2l_walk_init(B, H, W, 64, 64, bid, nblk);
    R2LTile t;
    int n = 0;
    while (r2l_walk_next(w, H, W, 64, 64, t)) {
      const int tile = (t.b * nty + t.oy / 64) * ntx + t.ox / 64;
      owner[tile] = bid;
      visits[tile] += 1;
      n += 1;
    }
    most = n > most ? n : most;
  }
  return most;
}
#endif
#endif
}  // extern "C"
