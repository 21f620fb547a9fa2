// r2l_sums_kernels.h -- per-channel sums and sums of squares in float64: what torch.mean / torch.std over (0, 2, 3) need
// (get_statistics, pipeline_numpy.py:306-329), without reading anything twice.
//
//   r2l_channel_sums_block   any (B,C,H,W) float32 tensor, C <= 4 -> one partial double[2 C] per SHARE of the elements
//   r2l_sums_finish_block    the partials of that kernel, or of the static chains' statistics forms (r2l_static_stream.h,
//                            r2l_static_chain.h: one double[6] per wavefront) -> sum[C], sum of squares[C], pixel count
//
// Every term (double)v and (double)v * (double)v is exact; the additions run in an order the shape of the call fixes: a lane's
// elements in address order, the 512 lanes of a workgroup through a pairwise tree in LDS (stride 256, 128, ... 1), the partials
// strided over the lanes of ONE workgroup (lane t: partials t, t + 512, ...) and through the same tree.  No atomics: the same bits
// on every run.  Written in phases without lane-to-lane operations, so the serial emulation runs them too.
#pragma once
#include "r2l_common.h"

#define R2L_SUMS_SLOTS 8  // 2 C, C <= 4
#define R2L_SUMS_LDS_FLOATS (2 * R2L_SUMS_SLOTS * R2L_NT)
#define R2L_SUMS_MAX_SHARES 2048

// red[k * R2L_NT + tid], k < nslots: the workgroup's sum of slot k to out[k]
R2L_BLOCKFN void r2l_sums_tree(double* red, int nslots, double* out) {
  for (int s = R2L_NT / 2; s >= 1; s >>= 1) {
    R2L_PHASE_BEGIN
    if (tid < s)
      for (int k = 0; k < nslots; ++k) red[k * R2L_NT + tid] += red[k * R2L_NT + tid + s];
    R2L_PHASE_END
  }
  R2L_PHASE_BEGIN
  if (tid < nslots) out[tid] = red[tid * R2L_NT];
  R2L_PHASE_END
}

struct R2LChannelSumsArgs {
  const float* x;   // n = B C H W elements, 4-byte aligned
  double* partial;  // [nv][2 C]
  size_t n, hw;
  size_t head, nvec;  // elements in front of the first 16-byte boundary; 16-byte vectors behind them (the rest: a tail of < 4)
  int C;
  int nv;  // shares of the vectors = rows of `partial`, from the shape (and the alignment) alone: workgroup bid takes shares bid, bid + nblk, ...
};
// plane (b, c) and offset inside it of element e (32-bit division where the tensor allows it)
R2L_HD void r2l_sums_locate(const R2LChannelSumsArgs& a, size_t e, int& c, size_t& rem) {
  size_t pl;
  if (a.n <= 0xffffffffu) {
    const unsigned p = (unsigned)e / (unsigned)a.hw;
    pl = p;
    rem = (unsigned)e - p * (unsigned)a.hw;
  } else {
    pl = e / a.hw;
    rem = e - pl * a.hw;
  }
  c = (int)(pl % (size_t)a.C);
}
R2L_HD void r2l_sums_add(double* s, float v, int c) {
  const double d = (double)v;
  R2L_PRAGMA_UNROLL
  for (int k = 0; k < 4; ++k) {
    const double t = (c == k) ? d : 0.0;
    s[k] += t;
    s[4 + k] = fma(t, t, s[4 + k]);
  }
}
R2L_BLOCKFN void r2l_channel_sums_block(const R2LChannelSumsArgs& a, int bid, int nblk, float* lds) {
  double* red = (double*)lds;
  for (int share = bid; share < a.nv; share += nblk) {
    R2L_PHASE_BEGIN
    double s[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};  // sums [0..3], sums of squares [4..7] by channel
    for (size_t i4 = (size_t)share * R2L_NT + tid; i4 < a.nvec; i4 += (size_t)a.nv * R2L_NT) {
      const size_t e = a.head + 4 * i4;
      const r2l_f4 v4 = r2l_load_f4_nt(a.x + e);
      const float v[4] = {v4.x, v4.y, v4.z, v4.w};
      int c;
      size_t rem;
      r2l_sums_locate(a, e, c, rem);
      R2L_PRAGMA_UNROLL
      for (int q = 0; q < 4; ++q) {  // (a vector may cross into the next plane, or -- planes of 1 .. 3 elements -- several)
        r2l_sums_add(s, v[q], c);
        if (++rem == a.hw) {
          rem = 0;
          c = (c + 1 == a.C) ? 0 : c + 1;
        }
      }
    }
    if (share == 0) {  // the scalar head and tail: lanes 0 .. 2 and 64 .. 66 of the first share
      const size_t tail0 = a.head + 4 * a.nvec;
      const bool is_head = (size_t)tid < a.head, is_tail = tid >= 64 && tail0 + (size_t)(tid - 64) < a.n;
      if (is_head || is_tail) {
        const size_t e = is_head ? (size_t)tid : tail0 + (size_t)(tid - 64);
        int c;
        size_t rem;
        r2l_sums_locate(a, e, c, rem);
        r2l_sums_add(s, a.x[e], c);
      }
    }
    R2L_PRAGMA_UNROLL
    for (int k = 0; k < 4; ++k)
      if (k < a.C) {
        red[k * R2L_NT + tid] = s[k];
        red[(a.C + k) * R2L_NT + tid] = s[4 + k];
      }
    R2L_PHASE_END
    r2l_sums_tree(red, 2 * a.C, a.partial + (size_t)share * 2 * a.C);
  }
}

struct R2LSumsFinishArgs {
  const double* partial;  // [n][nslots]
  int n, nslots;          // nslots = 2 C <= 8
  double count;           // B H W, to out[nslots]
  double* out;            // [nslots + 1]
};
// one workgroup
R2L_BLOCKFN void r2l_sums_finish_block(const R2LSumsFinishArgs& a, int bid, int nblk, float* lds) {
  (void)bid;
  (void)nblk;
  double* red = (double*)lds;
  R2L_PHASE_BEGIN
  for (int k = 0; k < a.nslots; ++k) {
    double s = 0.0;
    for (int i = tid; i < a.n; i += R2L_NT) s += a.partial[(size_t)i * a.nslots + k];
    red[k * R2L_NT + tid] = s;
  }
  R2L_PHASE_END
  r2l_sums_tree(red, a.nslots, a.out);
  R2L_PHASE_BEGIN
  if (tid == 0) a.out[a.nslots] = a.count;
  R2L_PHASE_END
}
