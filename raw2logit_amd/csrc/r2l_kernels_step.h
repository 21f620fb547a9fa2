// r2l_kernels_step.h -- the kernels of the parametrised ISP (the training step's forward and backward, BatchNorm, raw2rgb), each
// launch table beside the kernels it lists.
#pragma once
#include "r2l_launch.h"
#include "r2l_simple_kernels.h"
#include "r2l_param_stream.h"
#include "r2l_param_plane_bwd.h"

// the serial emulation compiles the tile forms of the kernels only (r2l_common.h): no row-streaming forward, no plane passes
#ifdef R2L_SERIAL
#define R2L_PLANE_PASSES 0
#else
#define R2L_PLANE_PASSES 1
#endif

typedef R2LGeom<64, 64> GFwd;
typedef R2LGeom<64, 64> GBwd1;
typedef R2LGeom<64, 64> GBwd2;

#define R2L_LDS3(G) (R2L_FOLDED_FLOATS + 2 * G::PAD + 3 * G::PLANE)
#define R2L_LDS4(G) (R2L_FOLDED_FLOATS + 2 * G::PAD + 4 * G::PLANE)
static_assert(R2L_LDS3(GFwd) >= R2L_RED_FLOATS, "reduction scratch must fit");
static_assert(R2L_LDS3(GBwd2) >= R2L_RED_FLOATS, "reduction scratch must fit");

R2L_KERNEL(r2l_launch_fold, R2LFoldArgs, r2l_fold_block, 4)
R2L_KERNEL(r2l_launch_unfold, R2LUnfoldArgs, r2l_unfold_block, 4 + 2 * R2L_NSUMS + 2 * R2L_UNFOLD_TG + R2L_P_COUNT + 4)
R2L_KERNEL(r2l_launch_bn_finalize, R2LBnFinalizeArgs, r2l_bn_finalize_block, 4)
R2L_KERNEL(r2l_launch_bn_bwd_means, R2LBnBwdMeansArgs, r2l_bn_bwd_means_block, 4)
R2L_KERNEL(r2l_launch_reduce_rows, R2LReduceRowsArgs, r2l_reduce_rows_block, 2 * R2L_NT + 64)
#ifndef R2L_OCC_FWD
#define R2L_OCC_FWD 4
#endif
#ifndef R2L_OCC_BWD1
#define R2L_OCC_BWD1 2
#endif
#ifndef R2L_OCC_BWD2
#define R2L_OCC_BWD2 4
#endif
// hot instantiation (frames that tile exactly, no additive layer) + the general ones; each again for 16-bit
// container frames (compile-time, so that the float32 kernels carry no decode code)
R2L_KERNEL_V(r2l_launch_fwd, R2LFwdArgs, R2L_LDS3(GFwd), R2L_OCC_FWD, r2l_fwd_block<GFwd, false, false, false>)
R2L_KERNEL_V(r2l_launch_fwd_ragged, R2LFwdArgs, R2L_LDS3(GFwd), 2, r2l_fwd_block<GFwd, false, true, false>)
// the additive layer on frames that tile exactly -- the reference's only case: its layer is 256 x 256 (pipeline_torch.py:130)
R2L_KERNEL_V(r2l_launch_fwd_add_exact, R2LFwdArgs, R2L_LDS3(GFwd), R2L_OCC_FWD, r2l_fwd_block<GFwd, true, false, false>)
#ifndef R2L_SERIAL
// the forward as a row-streaming kernel (r2l_param_stream.h): NW wavefronts side by side cover 256 * NW columns
#ifndef R2L_FS_OCC
#define R2L_FS_OCC 3
#endif
#ifndef R2L_FS_MINBAND
#define R2L_FS_MINBAND 16  // rows: shortest band of the row-streaming forward (7 halo rows of luma per band)
#endif
// (8 wavefronts side by side -- frames 1024 < W <= 2048 -- need 99 KB of LDS: one workgroup per CU, 2 wavefronts per SIMD)
#define R2L_FS_OCC_NW(NW) ((NW) == 8 ? 2 : R2L_FS_OCC)
// One spelling per family.  R2L_FS_KERNELS(pre, sfx, EPI, SONLY, IO) emits the eight kernels r2l_launch_fwd_stream<pre>_w{1,2,4,8}[_u16]<sfx>,
// R2L_FS_ROW(pre, sfx) their row of r2l_fwd_stream_table: [16-bit container frames][wavefronts per row: 1, 2, 4, 8]
#define R2L_FS_KERNEL(pre, NW, u16, sfx, ...)                                                                              \
  R2L_KERNEL_NT_LDS(r2l_launch_fwd_stream##pre##_w##NW##u16##sfx, R2LFwdStreamArgs, (NW) * 64, R2L_FS_LDS_FLOATS(NW),     \
                    R2L_FS_OCC_NW(NW), r2l_fwd_stream_block<NW, __VA_ARGS__>)
#define R2L_FS_KERNELS(pre, sfx, ...)                  \
  R2L_FS_KERNEL(pre, 1, , sfx, false, __VA_ARGS__)     \
  R2L_FS_KERNEL(pre, 2, , sfx, false, __VA_ARGS__)     \
  R2L_FS_KERNEL(pre, 4, , sfx, false, __VA_ARGS__)     \
  R2L_FS_KERNEL(pre, 8, , sfx, false, __VA_ARGS__)     \
  R2L_FS_KERNEL(pre, 1, _u16, sfx, true, __VA_ARGS__)  \
  R2L_FS_KERNEL(pre, 2, _u16, sfx, true, __VA_ARGS__)  \
  R2L_FS_KERNEL(pre, 4, _u16, sfx, true, __VA_ARGS__)  \
  R2L_FS_KERNEL(pre, 8, _u16, sfx, true, __VA_ARGS__)
#define R2L_FS_ROW(pre, sfx)                                                                                            \
  {{r2l_launch_fwd_stream##pre##_w1##sfx, r2l_launch_fwd_stream##pre##_w2##sfx, r2l_launch_fwd_stream##pre##_w4##sfx,    \
    r2l_launch_fwd_stream##pre##_w8##sfx},                                                                              \
   {r2l_launch_fwd_stream##pre##_w1_u16##sfx, r2l_launch_fwd_stream##pre##_w2_u16##sfx,                                 \
    r2l_launch_fwd_stream##pre##_w4_u16##sfx, r2l_launch_fwd_stream##pre##_w8_u16##sfx}}
R2L_FS_KERNELS(, , false, false, R2L_IO_F32)
// ... the statistics pass of train-mode BatchNorm (no output; keeps Y' when asked): its own instantiation
R2L_FS_KERNELS(_stats, , false, true, R2L_IO_F32)
// ... with the output epilogue (flip / flip / rot90 of the output planes as part of the stores, R2LEpi)
R2L_FS_KERNELS(_epi, , true, false, R2L_IO_F32)
// ... writing the output as bfloat16 / float16 (r2l_isp_step_fwd_io: R2L_IO_*; no epilogue)
R2L_FS_KERNELS(, _bf16, false, false, R2L_IO_BF16)
R2L_FS_KERNELS(, _f16, false, false, R2L_IO_F16)
// ... writing it channels-last (r2l_isp_step_fwd_layout: R2L_LAYOUT_NHWC; float32 and 16 bits, no epilogue)
R2L_FS_KERNELS(, _nhwc, false, false, R2L_IO_F32 | R2L_IO_NHWC)
R2L_FS_KERNELS(, _bf16_nhwc, false, false, R2L_IO_BF16 | R2L_IO_NHWC)
R2L_FS_KERNELS(, _f16_nhwc, false, false, R2L_IO_F16 | R2L_IO_NHWC)
// The implementations' `io` = element type (R2L_IO_*) | R2L_IO_NHWC for a channels-last tensor (r2l_common.h).  Every value but
// R2L_IO_F32 takes the routes a 16-bit call takes; its rows in their launch tables (r2l_io_check has seen the value):
#define R2L_IO_SLOTS 5
static int r2l_io_slot(int io) { return (io & R2L_IO_NHWC) ? 2 + R2L_IO_ELEM(io) : io - 1; }
typedef int (*r2l_fwd_stream_launch_t)(const R2LFwdStreamArgs&, int, void*);
enum { R2L_FS_PLAIN, R2L_FS_STATS, R2L_FS_EPI, R2L_FS_IO /* + r2l_io_slot */ };
static const r2l_fwd_stream_launch_t r2l_fwd_stream_table[R2L_FS_IO + R2L_IO_SLOTS][2][4] = {
    R2L_FS_ROW(, ),      R2L_FS_ROW(_stats, ), R2L_FS_ROW(_epi, ),      R2L_FS_ROW(, _bf16),
    R2L_FS_ROW(, _f16),  R2L_FS_ROW(, _nhwc),  R2L_FS_ROW(, _bf16_nhwc), R2L_FS_ROW(, _f16_nhwc)};
// A family of [_u16] pairs -- plain, with the output epilogue (<pre> = _epi), one per io slot (<sfx>): the kernels base<pre>[_u16]<sfx>
// and their row of a launch table, [16-bit container frames]
#define R2L_PAIR_KERNELS(KERNEL, base, pre, sfx, ...) \
  KERNEL(base##pre##sfx, false, __VA_ARGS__)          \
  KERNEL(base##pre##_u16##sfx, true, __VA_ARGS__)
#define R2L_PAIR_ROW(base, pre, sfx) {base##pre##sfx, base##pre##_u16##sfx}
#define R2L_PAIR_FAMILY(KERNEL, base)                                             \
  R2L_PAIR_KERNELS(KERNEL, base, , , false, R2L_IO_F32)                           \
  R2L_PAIR_KERNELS(KERNEL, base, _epi, , true, R2L_IO_F32)                        \
  R2L_PAIR_KERNELS(KERNEL, base, , _bf16, false, R2L_IO_BF16)                     \
  R2L_PAIR_KERNELS(KERNEL, base, , _f16, false, R2L_IO_F16)                       \
  R2L_PAIR_KERNELS(KERNEL, base, , _nhwc, false, R2L_IO_F32 | R2L_IO_NHWC)        \
  R2L_PAIR_KERNELS(KERNEL, base, , _bf16_nhwc, false, R2L_IO_BF16 | R2L_IO_NHWC)  \
  R2L_PAIR_KERNELS(KERNEL, base, , _f16_nhwc, false, R2L_IO_F16 | R2L_IO_NHWC)
#define R2L_PAIR_TABLE(base)                                                                                             \
  {R2L_PAIR_ROW(base, , ),      R2L_PAIR_ROW(base, _epi, ),       R2L_PAIR_ROW(base, , _bf16),     R2L_PAIR_ROW(base, , _f16), \
   R2L_PAIR_ROW(base, , _nhwc), R2L_PAIR_ROW(base, , _bf16_nhwc), R2L_PAIR_ROW(base, , _f16_nhwc)}
enum { R2L_PAIR_PLAIN, R2L_PAIR_EPI, R2L_PAIR_IO /* + r2l_io_slot */ };
// the apply pass of train-mode BatchNorm on the Y' plane the statistics pass kept: independent wavefronts, no LDS
#ifndef R2L_FA_OCC
#define R2L_FA_OCC 3
#endif
#ifndef R2L_FA_NWV
#define R2L_FA_NWV 4  // wavefronts (= work items) per workgroup of the apply and luma passes
#endif
#define R2L_FA_KERNEL(name, U16, EPI, IO) \
  R2L_KERNEL_NT_LDS(name, R2LFwdStreamArgs, 64 * R2L_FA_NWV, 4, R2L_FA_OCC, r2l_fwd_apply_block<U16, EPI, false, R2L_FA_NWV, IO>)
R2L_PAIR_FAMILY(R2L_FA_KERNEL, r2l_launch_fwd_apply)
static const r2l_fwd_stream_launch_t r2l_fwd_apply_table[R2L_PAIR_IO + R2L_IO_SLOTS][2] = R2L_PAIR_TABLE(r2l_launch_fwd_apply);
// ... the same walk without output: the BatchNorm statistics from the kept plane (2 wavefronts per workgroup, each with
// its own work items; <= R2L_MAX_BLOCKS workgroups = partials of the reduction tree)
#define R2L_FA_STATS_NWV 4
#ifndef R2L_FA_STATS_OCC
#define R2L_FA_STATS_OCC 3
#endif
R2L_KERNEL_NT_LDS(r2l_launch_fwd_stats, R2LFwdStreamArgs, 64 * R2L_FA_STATS_NWV, R2L_FA_LDS_FLOATS(R2L_FA_STATS_NWV, true),
                  R2L_FA_STATS_OCC, r2l_fwd_apply_block<false, false, true, R2L_FA_STATS_NWV>)
R2L_KERNEL_NT_LDS(r2l_launch_fwd_stats_u16, R2LFwdStreamArgs, 64 * R2L_FA_STATS_NWV,
                  R2L_FA_LDS_FLOATS(R2L_FA_STATS_NWV, true), R2L_FA_STATS_OCC,
                  r2l_fwd_apply_block<true, false, true, R2L_FA_STATS_NWV>)
// the luma pass in front of them: raw -> Y' (independent wavefronts, no LDS)
#ifndef R2L_FL_OCC
#define R2L_FL_OCC 4
#endif
R2L_KERNEL_NT_LDS(r2l_launch_fwd_luma, R2LFwdStreamArgs, 64 * R2L_FA_NWV, 4, R2L_FL_OCC, r2l_fwd_luma_block<false, R2L_FA_NWV>)
R2L_KERNEL_NT_LDS(r2l_launch_fwd_luma_u16, R2LFwdStreamArgs, 64 * R2L_FA_NWV, 4, R2L_FL_OCC, r2l_fwd_luma_block<true, R2L_FA_NWV>)
#endif
R2L_KERNEL_V(r2l_launch_bwd1, R2LBwd1Args, R2L_LDS3(GBwd1), R2L_OCC_BWD1, r2l_bwd1_block<GBwd1, false, false, false>)
R2L_KERNEL_V(r2l_launch_bwd1_ragged, R2LBwd1Args, R2L_LDS3(GBwd1), 2, r2l_bwd1_block<GBwd1, false, true, false>)
// ... with Y' taken from the plane the streaming forward kept (one workgroup per CU: the second prefetch frame
// takes the kernel past 256 VGPRs)
#ifndef R2L_OCC_BWD1S
#define R2L_OCC_BWD1S 1
#endif
R2L_KERNEL_V(r2l_launch_bwd1_saved, R2LBwd1Args, R2L_LDS3(GBwd1) + GBwd1::PAD + R2L_B1_FRAME_FLOATS, R2L_OCC_BWD1S, r2l_bwd1_block<GBwd1, false, false, false, true>)
R2L_KERNEL_V(r2l_launch_bwd1_saved_u16, R2LBwd1Args, R2L_LDS3(GBwd1) + GBwd1::PAD + R2L_B1_FRAME_FLOATS, R2L_OCC_BWD1S, r2l_bwd1_block<GBwd1, false, false, true, true>)
// (frames that do not tile by 64 below 4 Mi px take r2l_launch_bwd1_ragged -- Y' recomputed in LDS -- also when the forward kept
// Y': the kept-plane form of the general instantiation needed 76 B of scratch per lane, round 6)
R2L_KERNEL_V(r2l_launch_bwd1_add_exact, R2LBwd1Args, R2L_LDS3(GBwd1), 2, r2l_bwd1_block<GBwd1, true, false, false>)
#ifndef R2L_SERIAL
// kernel B1 as two passes over planes (r2l_param_plane_bwd.h): where the forward kept Y' and no epilogue / additive layer
R2L_KERNEL_NT_LDS(r2l_launch_bwd1_plane, R2LBwd1Args, R2L_BP_NT, R2L_BP_LDS_FLOATS, 2, r2l_bwd1_plane_block<false, false>)
R2L_KERNEL_NT_LDS(r2l_launch_bwd1_plane_u16, R2LBwd1Args, R2L_BP_NT, R2L_BP_LDS_FLOATS, 2, r2l_bwd1_plane_block<true, false>)
R2L_KERNEL_NT_LDS(r2l_launch_bwd1_plane_epi, R2LBwd1Args, R2L_BP_NT, R2L_BP_LDS_FLOATS, 2, r2l_bwd1_plane_block<false, true>)
R2L_KERNEL_NT_LDS(r2l_launch_bwd1_plane_epi_u16, R2LBwd1Args, R2L_BP_NT, R2L_BP_LDS_FLOATS, 2, r2l_bwd1_plane_block<true, true>)
// ... storing the chroma gradient planes gU, gV as well, for the d/d raw pass (float32 frames, no epilogue)
struct R2LBwd1GuvArgs {
  R2LBwd1Args b;
  float* guv;  // gU (B,H,W), then gV (B,H,W)
};
R2L_BLOCKFN void r2l_bwd1_plane_guv_block(const R2LBwd1GuvArgs& a, int bid, int nblk, float* lds) {
  r2l_bwd1_plane_block<false, false, true>(a.b, bid, nblk, lds, a.guv);
}
R2L_KERNEL_NT_LDS(r2l_launch_bwd1_plane_guv, R2LBwd1GuvArgs, R2L_BP_NT, R2L_BP_LDS_FLOATS, 2, r2l_bwd1_plane_guv_block)
// ... reading grad_out as bfloat16 / float16 (r2l_isp_step_bwd_io: the full route, no epilogue)
template <int IO>
R2L_BLOCKFN void r2l_bwd1_plane_guv_io_block(const R2LBwd1GuvArgs& a, int bid, int nblk, float* lds) {
  r2l_bwd1_plane_block<false, false, true, R2L_BPS_FULL, R2L_BPS_PF, IO>(a.b, bid, nblk, lds, a.guv);
}
// (16-bit container frames and the gU / gV stores: ONE row of raw / Y' in flight like the reduced routes (R2L_BPS_PF, 10 registers
// less) -- with two, hipcc took 214 and 226 registers where the float32 siblings take 208 and 222, whatever the place of the
// widening; the cotangent these forms wait for is half as many bytes.  profiles/half_io_resources.txt)
#define R2L_BP_KERNELS_IO(sfx, IO)                                                                          \
  R2L_KERNEL_NT_LDS(r2l_launch_bwd1_plane##sfx, R2LBwd1Args, R2L_BP_NT, R2L_BP_LDS_FLOATS, 2,               \
                    r2l_bwd1_plane_block<false, false, false, R2L_BPS_FULL, R2L_BP_PF, IO>)                 \
  R2L_KERNEL_NT_LDS(r2l_launch_bwd1_plane_u16##sfx, R2LBwd1Args, R2L_BP_NT, R2L_BP_LDS_FLOATS, 2,           \
                    r2l_bwd1_plane_block<true, false, false, R2L_BPS_FULL, R2L_BPS_PF, IO>)                 \
  R2L_KERNEL_NT_LDS(r2l_launch_bwd1_plane_guv##sfx, R2LBwd1GuvArgs, R2L_BP_NT, R2L_BP_LDS_FLOATS, 2,        \
                    r2l_bwd1_plane_guv_io_block<IO>)
R2L_BP_KERNELS_IO(_bf16, R2L_IO_BF16)
R2L_BP_KERNELS_IO(_f16, R2L_IO_F16)
R2L_BP_KERNELS_IO(_nhwc, R2L_IO_F32 | R2L_IO_NHWC)
R2L_BP_KERNELS_IO(_bf16_nhwc, R2L_IO_BF16 | R2L_IO_NHWC)
R2L_BP_KERNELS_IO(_f16_nhwc, R2L_IO_F16 | R2L_IO_NHWC)
R2L_KERNEL_NT_LDS(r2l_launch_bwd1_blur, R2LBwd1Args, R2L_BP_NT, R2L_BP_RED_FLOATS, 3, r2l_bwd1_blur_block)
R2L_KERNEL_NT_LDS(r2l_launch_bwd1_blur_hp, R2LBwd1Args, R2L_BP_NT, R2L_BP_RED_FLOATS, R2L_HB_OCC, r2l_bwd1_blur_hp_block)
// the reduced forms r2l_isp_step_bwd_select routes to (R2L_BPS_*: what each keeps).  Without the 38 stencil accumulator pairs
// and with one row of raw / Y' in flight instead of two the pass fits three wavefronts per SIMD (133 .. 164 VGPRs, no scratch)
// -- except the pure map with the gU / gV stores: hipcc keeps ~250 folded weights live in scalar registers there and spills
// them into vector lanes (3 VGPRs over at one row in flight, 17 at two), so that one stays at two wavefronts (184 VGPRs)
#define R2L_BPS_OCC 3
#define R2L_BPS_OCC_RAW 2
struct R2LBwd1SelArgs {
  R2LBwd1Args b;
  float* guv;  // gU, gV planes (the GUV forms), else null
  R2LBpSelect s;
};
template <bool U16, bool EPI, bool GUV, int SEL, int PF = R2L_BPS_PF>
R2L_BLOCKFN void r2l_bwd1_sel_block(const R2LBwd1SelArgs& a, int bid, int nblk, float* lds) {
  r2l_bwd1_plane_block<U16, EPI, GUV, SEL, PF>(a.b, bid, nblk, lds, a.guv, &a.s);
}
R2L_BLOCKFN void r2l_bwd1_blur_fin_block(const R2LBwd1SelArgs& a, int bid, int nblk, float* lds) {
  r2l_bwd1_blur_block<true>(a.b, bid, nblk, lds, &a.s);
}
R2L_BLOCKFN void r2l_bwd1_blur_hp_fin_block(const R2LBwd1SelArgs& a, int bid, int nblk, float* lds) {
  r2l_bwd1_blur_hp_block<true>(a.b, bid, nblk, lds, &a.s);
}
// d/d raw alone: a pure map raw + Y' + grad_out -> dL/dY'', gU, gV (no accumulator, no LDS, no tail); ... with the gamma sum
R2L_KERNEL_NT_LDS(r2l_launch_bwd1_sel_raw, R2LBwd1SelArgs, R2L_BP_NT, 4, R2L_BPS_OCC_RAW,
                  r2l_bwd1_sel_block<false, false, true, R2L_BPS_GYPP, R2L_BP_PF>)
R2L_KERNEL_NT_LDS(r2l_launch_bwd1_sel_raw_gamma, R2LBwd1SelArgs, R2L_BP_NT, R2L_BPS_LDS_FLOATS, R2L_BPS_OCC,
                  r2l_bwd1_sel_block<false, false, true, R2L_BPS_GYPP | R2L_BPS_GAMMA>)
// gamma alone (no plane written); dL/dY'' for the blur pass; both -- float32 / 16-bit frames, with / without the output epilogue
#define R2L_BPS_KERNELS(name, LDSF, SEL)                                                                                       \
  R2L_KERNEL_NT_LDS(name, R2LBwd1SelArgs, R2L_BP_NT, LDSF, R2L_BPS_OCC, r2l_bwd1_sel_block<false, false, false, SEL>)         \
  R2L_KERNEL_NT_LDS(name##_u16, R2LBwd1SelArgs, R2L_BP_NT, LDSF, R2L_BPS_OCC, r2l_bwd1_sel_block<true, false, false, SEL>)    \
  R2L_KERNEL_NT_LDS(name##_epi, R2LBwd1SelArgs, R2L_BP_NT, LDSF, R2L_BPS_OCC, r2l_bwd1_sel_block<false, true, false, SEL>)    \
  R2L_KERNEL_NT_LDS(name##_epi_u16, R2LBwd1SelArgs, R2L_BP_NT, LDSF, R2L_BPS_OCC, r2l_bwd1_sel_block<true, true, false, SEL>)
R2L_BPS_KERNELS(r2l_launch_bwd1_sel_gamma, R2L_BPS_LDS_FLOATS, R2L_BPS_GAMMA)
R2L_BPS_KERNELS(r2l_launch_bwd1_sel_gypp, 4, R2L_BPS_GYPP)
R2L_BPS_KERNELS(r2l_launch_bwd1_sel_gypp_gamma, R2L_BPS_LDS_FLOATS, R2L_BPS_GYPP | R2L_BPS_GAMMA)
// the blur passes whose last workgroup finishes the 25 sums into the blur gradient
R2L_KERNEL_NT_LDS(r2l_launch_bwd1_blur_fin, R2LBwd1SelArgs, R2L_BP_NT, R2L_BP_RED_FLOATS, 3, r2l_bwd1_blur_fin_block)
R2L_KERNEL_NT_LDS(r2l_launch_bwd1_blur_hp_fin, R2LBwd1SelArgs, R2L_BP_NT, R2L_BP_RED_FLOATS, R2L_HB_OCC, r2l_bwd1_blur_hp_fin_block)
// kernel B2 likewise: the blur's adjoint into a plane, then the sums + the final reduction and unfold
R2L_KERNEL_NT_LDS(r2l_launch_bwd2_hp, R2LBwd2Args, R2L_BP_NT, 4, 4, r2l_bwd2_hp_block)
R2L_KERNEL_NT_LDS(r2l_launch_bwd2_sums, R2LBwd2Args, R2L_B2S_NT, R2L_B2S_LDS_FLOATS, 3, r2l_bwd2_sums_block<false>)
R2L_KERNEL_NT_LDS(r2l_launch_bwd2_sums_u16, R2LBwd2Args, R2L_B2S_NT, R2L_B2S_LDS_FLOATS, 3, r2l_bwd2_sums_block<true>)
// d/d raw: HP + gU + gV -> grad_raw (independent wavefronts, no LDS)
#ifndef R2L_BR_OCC
#define R2L_BR_OCC 3
#endif
R2L_KERNEL_NT_LDS(r2l_launch_bwd_raw_plane, R2LRawGradArgs, 64 * R2L_BR_NWV, 4, R2L_BR_OCC, r2l_bwd_raw_plane_block)
// BatchNorm's backward sums from the raw frame, Y' and grad_out (xhat recomputed, the output not read back): r2l_bnr_planes_block
#ifndef R2L_BNR_OCC
#define R2L_BNR_OCC 3
#endif
#define R2L_BNR_NWV 4
#define R2L_BNR_KERNEL(name, U16, EPI, IO)                                                                      \
  R2L_KERNEL_NT_LDS(name, R2LBnrArgs, 64 * R2L_BNR_NWV, R2L_FA_LDS_FLOATS(R2L_BNR_NWV, true), R2L_BNR_OCC,      \
                    r2l_bnr_planes_block<U16, EPI, R2L_BNR_NWV, IO>)
R2L_PAIR_FAMILY(R2L_BNR_KERNEL, r2l_launch_bnr_planes)
typedef int (*r2l_bnr_launch_t)(const R2LBnrArgs&, int, void*);
static const r2l_bnr_launch_t r2l_bnr_table[R2L_PAIR_IO + R2L_IO_SLOTS][2] = R2L_PAIR_TABLE(r2l_launch_bnr_planes);
#endif
R2L_KERNEL_V(r2l_launch_bwd2, R2LBwd2Args, R2L_LDS3(GBwd2), R2L_OCC_BWD2, r2l_bwd2_block<GBwd2, false>)
R2L_KERNEL_V(r2l_launch_fwd_u16, R2LFwdArgs, R2L_LDS3(GFwd), R2L_OCC_FWD, r2l_fwd_block<GFwd, false, false, true>)
R2L_KERNEL_V(r2l_launch_fwd_ragged_u16, R2LFwdArgs, R2L_LDS3(GFwd), 2, r2l_fwd_block<GFwd, false, true, true>)
R2L_KERNEL_V(r2l_launch_fwd_add_exact_u16, R2LFwdArgs, R2L_LDS3(GFwd), R2L_OCC_FWD, r2l_fwd_block<GFwd, true, false, true>)
R2L_KERNEL_V(r2l_launch_bwd1_u16, R2LBwd1Args, R2L_LDS3(GBwd1), R2L_OCC_BWD1, r2l_bwd1_block<GBwd1, false, false, true>)
R2L_KERNEL_V(r2l_launch_bwd1_ragged_u16, R2LBwd1Args, R2L_LDS3(GBwd1), 2, r2l_bwd1_block<GBwd1, false, true, true>)
R2L_KERNEL_V(r2l_launch_bwd1_add_exact_u16, R2LBwd1Args, R2L_LDS3(GBwd1), 2, r2l_bwd1_block<GBwd1, true, false, true>)
R2L_KERNEL_V(r2l_launch_bwd2_u16, R2LBwd2Args, R2L_LDS3(GBwd2), R2L_OCC_BWD2, r2l_bwd2_block<GBwd2, true>)
// 14 KB of LDS instead of 68 KB: 8 workgroups' worth of loads in flight per CU instead of 2
R2L_KERNEL_OCC(r2l_launch_bn_reduce, R2LBnReduceArgs, r2l_bn_reduce_block, R2L_RED_FLOATS_N(6), 8)
R2L_KERNEL(r2l_launch_add_bwd, R2LAddBwdArgs, r2l_add_bwd_block, 4)
// (raw2rgb: here, in front of the static chains' kernels, where the device code has them)
R2L_KERNEL(r2l_launch_raw2rgb_fwd, R2LRaw2RgbArgs, r2l_raw2rgb_fwd_block, 4)
R2L_KERNEL(r2l_launch_raw2rgb_bwd, R2LRaw2RgbArgs, r2l_raw2rgb_bwd_block, R2L_RED_FLOATS)
