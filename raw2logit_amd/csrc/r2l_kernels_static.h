// r2l_kernels_static.h -- the kernels of the static chains (processing() with fixed settings), each launch table beside the
// kernels it lists.
#pragma once
#include "r2l_launch.h"
#include "r2l_static_kernels.h"
#include "r2l_static_stream.h"
#include "r2l_static_chain.h"
#include "r2l_static_planes.h"
#include "r2l_static_menon.h"

R2L_KERNEL(r2l_launch_static_full, R2LStaticArgs, r2l_static_block<GStatic>, R2L_STATIC_LDS_FLOATS)
// 3 wavefronts per SIMD with 5 rows in flight each beat 4 with 3 by 1 % (same-buffer A/B): the depth is what counts
#ifndef R2L_STREAM_OCC_BILINEAR
#define R2L_STREAM_OCC_BILINEAR 3
#endif
#ifndef R2L_STREAM_OCC_MALVAR
#define R2L_STREAM_OCC_MALVAR 3
#endif
// One spelling per form of the row-streaming kernels (r2l_static_stream.h).  A form is base<sfx>: whether it is the luma-plane pass
// (LUMA), what it stores (IO: float32 | bfloat16 | float16 | R2L_IO_STATS: nothing, the channel sums) and whether every row goes to
// its augmented position (EPI).  R2L_STREAM_FORM(base, sfx, LUMA, IO, EPI) emits its kernels base_{bilinear,malvar}[_u16]<sfx> --
// demosaic x frame container (float32 | 16-bit), at the occupancy of the demosaic --, R2L_STREAM_FORM_F64 those and the two of
// float64 frames (3 / 2 wavefronts per SIMD); R2L_STREAM_ROW / _ROW_F64(base, sfx) is their row of a launch table,
// [frames: float32 | 16-bit | float64][bilinear | Malvar2004], null for the float64 frames of a form that has none
#define R2L_STREAM_KERNEL(name, DEB, RAWK, LUMA, IO, EPI, OCC)                                           \
  R2L_BLOCKFN void name##_block(const R2LStaticStreamArgs& sa, int bid, int nblk, float* lds) {          \
    r2l_static_stream_block<DEB, RAWK, LUMA, IO, EPI>(sa, bid, nblk, lds);                               \
  }                                                                                                      \
  R2L_KERNEL_NT(name, R2LStaticStreamArgs, name##_block, R2L_STREAM_NT, OCC)
#define R2L_STREAM_PAIR(base, knd, sfx, RAWK, LUMA, IO, EPI, OCC_BILINEAR, OCC_MALVAR)  \
  R2L_STREAM_KERNEL(base##_bilinear##knd##sfx, 0, RAWK, LUMA, IO, EPI, OCC_BILINEAR)    \
  R2L_STREAM_KERNEL(base##_malvar##knd##sfx, 1, RAWK, LUMA, IO, EPI, OCC_MALVAR)
#define R2L_STREAM_FORM(base, sfx, LUMA, IO, EPI)                                                                   \
  R2L_STREAM_PAIR(base, , sfx, R2L_RAW_F32, LUMA, IO, EPI, R2L_STREAM_OCC_BILINEAR, R2L_STREAM_OCC_MALVAR)          \
  R2L_STREAM_PAIR(base, _u16, sfx, R2L_RAW_U16, LUMA, IO, EPI, R2L_STREAM_OCC_BILINEAR, R2L_STREAM_OCC_MALVAR)
#define R2L_STREAM_FORM_F64(base, sfx, LUMA, IO, EPI) \
  R2L_STREAM_FORM(base, sfx, LUMA, IO, EPI)           \
  R2L_STREAM_PAIR(base, _f64, sfx, R2L_RAW_F64, LUMA, IO, EPI, 3, 2)
#define R2L_STREAM_PAIR_ROW(base, knd, sfx) {base##_bilinear##knd##sfx, base##_malvar##knd##sfx}
#define R2L_STREAM_ROW(base, sfx) {R2L_STREAM_PAIR_ROW(base, , sfx), R2L_STREAM_PAIR_ROW(base, _u16, sfx)}
#define R2L_STREAM_ROW_F64(base, sfx) \
  {R2L_STREAM_PAIR_ROW(base, , sfx), R2L_STREAM_PAIR_ROW(base, _u16, sfx), R2L_STREAM_PAIR_ROW(base, _f64, sfx)}
typedef int (*R2LStreamLaunch)(const R2LStaticStreamArgs&, int, void*);
// the whole short chain; the luma-plane passes
R2L_STREAM_FORM_F64(r2l_launch_static_stream, , false, R2L_IO_F32, false)
R2L_STREAM_FORM_F64(r2l_launch_static_luma, , true, R2L_IO_F32, false)
static const R2LStreamLaunch r2l_static_luma_table[3][2] = R2L_STREAM_ROW_F64(r2l_launch_static_luma, );
// r2l_static_stream_table[epilogue][output: float32 | bfloat16 | float16 | none, statistics][frames][bilinear | Malvar2004].
// Null where no form exists: float64 frames with an epilogue, statistics with one.  r2l_static_plan never hands such an entry out:
// it indexes with an output other than float32 only where its `no_io` (16-bit) resp. `no_stats` is null, with the epilogue only
// where its `no_epi` is null -- which refuses float64 frames --, and no entry asks for statistics and an epilogue at once.
#ifdef R2L_SERIAL
// (the serial emulation: the float32 forms alone -- `no_io`, `no_stats` and `no_epi` are never null there --, in a table of the
// full size: an index the plan should not have used finds a null launcher, not the memory behind the table)
static const R2LStreamLaunch r2l_static_stream_table[2][4][3][2] = {{R2L_STREAM_ROW_F64(r2l_launch_static_stream, )}};
#else
// ... the whole short chain writing bfloat16 / float16 (r2l_static_fwd_io: R2L_IO_*), at their float32 siblings' occupancy
R2L_STREAM_FORM_F64(r2l_launch_static_stream, _bf16, false, R2L_IO_BF16, false)
R2L_STREAM_FORM_F64(r2l_launch_static_stream, _f16, false, R2L_IO_F16, false)
// ... and storing nothing: the channel sums of what the float32 siblings store (r2l_static_stats)
R2L_STREAM_FORM_F64(r2l_launch_static_stream, _stats, false, R2L_IO_STATS, false)
// ... and storing every row at its augmented position (r2l_static_fwd_epilogue: R2LEpi with sc = +-1, launch arguments): float32 and
// 16-bit-container frames x the three output types, at their siblings' occupancy
R2L_STREAM_FORM(r2l_launch_static_stream, _epi, false, R2L_IO_F32, true)
R2L_STREAM_FORM(r2l_launch_static_stream, _bf16_epi, false, R2L_IO_BF16, true)
R2L_STREAM_FORM(r2l_launch_static_stream, _f16_epi, false, R2L_IO_F16, true)
static const R2LStreamLaunch r2l_static_stream_table[2][4][3][2] = {
    {R2L_STREAM_ROW_F64(r2l_launch_static_stream, ), R2L_STREAM_ROW_F64(r2l_launch_static_stream, _bf16),
     R2L_STREAM_ROW_F64(r2l_launch_static_stream, _f16), R2L_STREAM_ROW_F64(r2l_launch_static_stream, _stats)},
    {R2L_STREAM_ROW(r2l_launch_static_stream, _epi), R2L_STREAM_ROW(r2l_launch_static_stream, _bf16_epi),
     R2L_STREAM_ROW(r2l_launch_static_stream, _f16_epi)}};
#endif
R2L_KERNEL(r2l_launch_plane_filter, R2LPlaneArgs, r2l_plane_filter_block, 4)
R2L_KERNEL(r2l_launch_spec_mask, R2LSpecMaskArgs, r2l_spec_mask_block, 4)
R2L_KERNEL(r2l_launch_static_finish, R2LStaticFinishArgs, r2l_static_finish_block, 4)
R2L_KERNEL(r2l_launch_static_menon, R2LMenonArgs, r2l_static_menon_block, 4)
#ifndef R2L_SERIAL
// row-streaming luma chains (r2l_static_chain.h): NW wavefronts side by side cover frames up to 256 * NW columns
#ifndef R2L_CHAIN_OCC
#define R2L_CHAIN_OCC 2
#endif
// behind unsharp_masking the 28 KB chroma ring per strip leaves one wavefront per SIMD on 1024-wide frames anyway:
// 512 registers instead of spills
#ifndef R2L_CHAIN_OCC_SH
#define R2L_CHAIN_OCC_SH 1
#endif
// (the workgroup size and the LDS size follow the frame width at launch time: 64 threads and 16.1 KB per strip)
#define R2L_CHAIN_KERNEL_IO(name, RAWK, DEB, SH, DN, IO, EPI)                                                        \
  R2L_KERNEL_DYN_LDS(name, R2LStaticChainArgs, (SH) ? 256 : 512, (SH) ? R2L_CHAIN_OCC_SH : R2L_CHAIN_OCC, a.nw * 64, \
                     2 * (size_t)R2L_CHAIN_LDS_DOUBLES(a.nw, SH), r2l_static_chain_block<RAWK, DEB, SH, DN, IO, EPI>)
// One spelling per form here too: a form is <sfx> = the frame container (RAWK) x what it stores (IO) x the output epilogue (EPI,
// r2l_static_fwd_epilogue).  R2L_CHAIN_KERNELS_IO_EPI emits its kernels [Malvar2004] x [unsharp_masking] x [median_denoising],
// R2L_CHAIN_ROW(sfx) is their block of the launch table
#define R2L_CHAIN_KERNELS_IO_EPI(sfx, RAWK, IO, EPI)                                               \
  R2L_CHAIN_KERNEL_IO(r2l_launch_static_chain##sfx, RAWK, 0, 0, 0, IO, EPI)                        \
  R2L_CHAIN_KERNEL_IO(r2l_launch_static_chain_median##sfx, RAWK, 0, 0, 1, IO, EPI)                 \
  R2L_CHAIN_KERNEL_IO(r2l_launch_static_chain_unsharp##sfx, RAWK, 0, 1, 0, IO, EPI)                \
  R2L_CHAIN_KERNEL_IO(r2l_launch_static_chain_unsharp_median##sfx, RAWK, 0, 1, 1, IO, EPI)         \
  R2L_CHAIN_KERNEL_IO(r2l_launch_static_chain_malvar##sfx, RAWK, 1, 0, 0, IO, EPI)                 \
  R2L_CHAIN_KERNEL_IO(r2l_launch_static_chain_malvar_median##sfx, RAWK, 1, 0, 1, IO, EPI)          \
  R2L_CHAIN_KERNEL_IO(r2l_launch_static_chain_malvar_unsharp##sfx, RAWK, 1, 1, 0, IO, EPI)         \
  R2L_CHAIN_KERNEL_IO(r2l_launch_static_chain_malvar_unsharp_median##sfx, RAWK, 1, 1, 1, IO, EPI)
#define R2L_CHAIN_ROW(sfx)                                                                                          \
  {{{r2l_launch_static_chain##sfx, r2l_launch_static_chain_median##sfx},                                            \
    {r2l_launch_static_chain_unsharp##sfx, r2l_launch_static_chain_unsharp_median##sfx}},                           \
   {{r2l_launch_static_chain_malvar##sfx, r2l_launch_static_chain_malvar_median##sfx},                              \
    {r2l_launch_static_chain_malvar_unsharp##sfx, r2l_launch_static_chain_malvar_unsharp_median##sfx}}}
R2L_CHAIN_KERNELS_IO_EPI(, R2L_RAW_F32, R2L_IO_F32, false)
R2L_CHAIN_KERNELS_IO_EPI(_u16, R2L_RAW_U16, R2L_IO_F32, false)
R2L_CHAIN_KERNELS_IO_EPI(_f64, R2L_RAW_F64, R2L_IO_F32, false)
R2L_CHAIN_KERNELS_IO_EPI(_bf16, R2L_RAW_F32, R2L_IO_BF16, false)
R2L_CHAIN_KERNELS_IO_EPI(_u16_bf16, R2L_RAW_U16, R2L_IO_BF16, false)
R2L_CHAIN_KERNELS_IO_EPI(_f16, R2L_RAW_F32, R2L_IO_F16, false)
R2L_CHAIN_KERNELS_IO_EPI(_u16_f16, R2L_RAW_U16, R2L_IO_F16, false)
R2L_CHAIN_KERNELS_IO_EPI(_stats, R2L_RAW_F32, R2L_IO_STATS, false)
R2L_CHAIN_KERNELS_IO_EPI(_u16_stats, R2L_RAW_U16, R2L_IO_STATS, false)
R2L_CHAIN_KERNELS_IO_EPI(_epi, R2L_RAW_F32, R2L_IO_F32, true)
R2L_CHAIN_KERNELS_IO_EPI(_u16_epi, R2L_RAW_U16, R2L_IO_F32, true)
R2L_CHAIN_KERNELS_IO_EPI(_bf16_epi, R2L_RAW_F32, R2L_IO_BF16, true)
R2L_CHAIN_KERNELS_IO_EPI(_u16_bf16_epi, R2L_RAW_U16, R2L_IO_BF16, true)
R2L_CHAIN_KERNELS_IO_EPI(_f16_epi, R2L_RAW_F32, R2L_IO_F16, true)
R2L_CHAIN_KERNELS_IO_EPI(_u16_f16_epi, R2L_RAW_U16, R2L_IO_F16, true)
typedef int (*R2LChainLaunch)(const R2LStaticChainArgs&, int, void*);
// r2l_static_chain_table[epilogue][output][frames][Malvar2004][unsharp_masking][median_denoising].  Null where no form exists:
// float64 frames with a 16-bit output, statistics or an epilogue; statistics with an epilogue.  As for r2l_static_stream_table,
// r2l_static_plan never hands one out: on this route `no_io` and `no_stats` refuse float64 frames as `no_epi` does everywhere.
static const R2LChainLaunch r2l_static_chain_table[2][4][3][2][2][2] = {
    {{R2L_CHAIN_ROW(), R2L_CHAIN_ROW(_u16), R2L_CHAIN_ROW(_f64)},
     {R2L_CHAIN_ROW(_bf16), R2L_CHAIN_ROW(_u16_bf16)},
     {R2L_CHAIN_ROW(_f16), R2L_CHAIN_ROW(_u16_f16)},
     {R2L_CHAIN_ROW(_stats), R2L_CHAIN_ROW(_u16_stats)}},
    {{R2L_CHAIN_ROW(_epi), R2L_CHAIN_ROW(_u16_epi)},
     {R2L_CHAIN_ROW(_bf16_epi), R2L_CHAIN_ROW(_u16_bf16_epi)},
     {R2L_CHAIN_ROW(_f16_epi), R2L_CHAIN_ROW(_u16_f16_epi)}}};
#endif
R2L_KERNEL(r2l_launch_static_short, R2LStaticArgs, r2l_static_short_block<GStatic>,
           R2L_STATIC_SHORT_LDS_FLOATS)
