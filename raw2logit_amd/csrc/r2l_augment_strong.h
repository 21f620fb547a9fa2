// r2l_augment_strong.h -- the strong augmentation set (utils/augmentation.py:77-84) as fused kernels.
//
// torchvision 0.10's RandomHorizontalFlip, RandomVerticalFlip, RandomApply([RandomRotation(90)]) (NEAREST, expand=False,
// fill), RandomApply([AddGaussianNoise]) and RandomAdjustSharpness(0.5), applied to N planes of H x W float32 in ONE
// forward launch:
//   v(q)  = x[flip(src(q))], or `fill` where the rotated sample falls outside the frame, (+ std * n(key, offset, q))
//   y(q)  = clamp(r v(q) + (1 - r) D(v)(q), 0, 1)   if sharpness was drawn, else v(q)
// D = the 3x3 blur (weights 1/13, centre 5/13) on the interior, the identity on the border rows and columns.
// The backward is at most two launches and has no atomics: the sharpness adjoint (r m g + (1 - r) D^T(m g), m = the clamp
// mask the forward saved as a byte plane), then the rotation adjoint as a GATHER: every source pixel tests the 3 x 3 output
// pixels around its inverse-rotated position with the same source function the forward uses and adds, in a fixed order,
// those whose source it is.  Results are bit-identical across runs and grid sizes.
#pragma once
#include "r2l_staged_kernels.h"

// The source coordinate is torchvision's float32 expression, evaluated in its order and rounded at every step (no fma)
#pragma clang fp contract(off)

#define R2L_AUGS_TW 64  // forward tile with sharpness: 64 x 32 output pixels, v staged on (32 + 2) x (64 + 8) in LDS
#define R2L_AUGS_TH 32
#define R2L_AUGS_EW (R2L_AUGS_TW + 8)  // 4 columns of halo each side keep the Philox groups (4 elements) aligned
#define R2L_AUGS_EH (R2L_AUGS_TH + 2)
#define R2L_AUGS_LDS_FLOATS (R2L_AUGS_EW * R2L_AUGS_EH)
#define R2L_AUGS_W1 (1.0f / 13.0f)  // torch.ones(3, 3), [1, 1] = 5, / its float32 sum 13
#define R2L_AUGS_W5 (5.0f / 13.0f)

struct R2LStrongGeom {
  int N, H, W;
  int hflip, vflip, rot;
  float txx, txy, tyx, tyy;  // theta^T / [W/2, H/2] of torchvision's _gen_affine_grid, float32, computed by the host
};
struct R2LStrongArgs {
  R2LStrongGeom g;
  const float* x;
  float* y;
  unsigned char* mask;        // clamp mask (0 <= pre <= 1) for the backward, or null
  const long long* key;       // Philox key (device memory), or null: no noise
  float fill, std, r, s;      // s = 1 - r; sharp off: r < 0
  unsigned long long offset;
};
struct R2LStrongBwdArgs {
  R2LStrongGeom g;
  const float* gy;            // gradient of y
  const unsigned char* mask;  // clamp mask of the forward (sharpness adjoint)
  float* gv;                  // sharpness adjoint out / rotation adjoint in
  float* gx;
  float r, s;
};

// output pixel (i, j) -> its nearest source pixel (si, sj) in the flipped frame; 0 where it falls outside (fill).
// grid = base @ theta^T / [W/2, H/2] with base = (linspace(-W/2 + 0.5, W/2 - 0.5, W), linspace(..H..), 1), then
// grid_sample(nearest, zeros, align_corners=False): ix = ((gx + 1) W - 1) / 2, round half to even.
R2L_HOSTDEV int r2l_strong_src(const R2LStrongGeom& g, int i, int j, int& si, int& sj) {
  if (!g.rot) {
    si = i;
    sj = j;
    return 1;
  }
  const float bx = (float)j + (0.5f - 0.5f * (float)g.W), by = (float)i + (0.5f - 0.5f * (float)g.H);
  const float px = bx * g.txx, py = by * g.txy, qx = bx * g.tyx, qy = by * g.tyy;
  const float gx = px + py, gy = qx + qy;
  const float ix = ((gx + 1.0f) * (float)g.W - 1.0f) * 0.5f, iy = ((gy + 1.0f) * (float)g.H - 1.0f) * 0.5f;
  const float rx = rintf(ix), ry = rintf(iy);
  if (!(rx >= 0.0f && rx <= (float)(g.W - 1) && ry >= 0.0f && ry <= (float)(g.H - 1))) return 0;
  si = (int)ry;
  sj = (int)rx;
  return 1;
}
// the rotated (+ noisy) value of the output pixels e, e + 1, .., e + 3 of plane `pl` at row i, columns j0 .. j0 + 3
// (only those with lo <= j <= hi are computed; the others are left alone)
R2L_HD void r2l_strong_v4(const R2LStrongArgs& a, int pl, int i, int j0, int lo, int hi, float v[4]) {
  const size_t hw = (size_t)a.g.H * a.g.W;
  const float* xp = a.x + (size_t)pl * hw;
  R2L_PRAGMA_UNROLL
  for (int k = 0; k < 4; ++k) {
    const int j = j0 + k;
    if (j < lo || j > hi) continue;
    int si, sj;
    float t = a.fill;
    if (r2l_strong_src(a.g, i, j, si, sj)) {
      if (a.g.vflip) si = a.g.H - 1 - si;
      if (a.g.hflip) sj = a.g.W - 1 - sj;
      t = xp[(size_t)si * a.g.W + sj];
    }
    v[k] = t;
  }
  if (!a.key) return;
  // r2l_philox_noise_block's deviates of the flat output index: 4 consecutive columns span at most 2 Philox groups
  const unsigned long long seed = (unsigned long long)*a.key;
  const size_t e0 = (size_t)pl * hw + (size_t)i * a.g.W;
  size_t have = ~(size_t)0;
  float nz[4] = {0.f, 0.f, 0.f, 0.f};
  for (int k = 0; k < 4; ++k) {
    const int j = j0 + k;
    if (j < lo || j > hi) continue;
    const size_t e = e0 + j, grp = e >> 2;
    if (grp != have) {
      unsigned o[4];
      r2l_philox4x32_10((unsigned)grp, (unsigned)(grp >> 32), (unsigned)a.offset, (unsigned)(a.offset >> 32),
                        (unsigned)seed, (unsigned)(seed >> 32), o);
      r2l_box_muller(o[0], o[1], nz[0], nz[1]);
      r2l_box_muller(o[2], o[3], nz[2], nz[3]);
      have = grp;
    }
    v[k] = fmaf(nz[e & 3], a.std, v[k]);
  }
}
R2L_HD void r2l_strong_store4(float* p, int j0, int W, const float v[4]) {
  if (j0 + 3 < W && ((uintptr_t)p & 15) == 0) {
    r2l_f4 w;
    w.x = v[0];
    w.y = v[1];
    w.z = v[2];
    w.w = v[3];
    *(r2l_f4*)p = w;
  } else {
    for (int k = 0; k < 4 && j0 + k < W; ++k) p[k] = v[k];
  }
}
// forward without sharpness (rotation / flips / noise; the mask planes): 4 output columns per lane, no LDS
R2L_BLOCKFN void r2l_strong_fwd_flat_block(const R2LStrongArgs& a, int bid, int nblk, float* lds) {
  (void)lds;
  const int cw = (a.g.W + 3) >> 2;
  const size_t nch = (size_t)a.g.N * a.g.H * cw;
  R2L_PHASE_BEGIN
  for (size_t c = (size_t)bid * R2L_NT + tid; c < nch; c += (size_t)nblk * R2L_NT) {
    const size_t row = c / cw;
    const int j0 = (int)(c - row * cw) * 4, pl = (int)(row / a.g.H), i = (int)(row - (size_t)pl * a.g.H);
    float v[4] = {0.f, 0.f, 0.f, 0.f};
    r2l_strong_v4(a, pl, i, j0, 0, a.g.W - 1, v);
    r2l_strong_store4(a.y + row * a.g.W + j0, j0, a.g.W, v);
  }
  R2L_PHASE_END
}
// forward with sharpness: per 64 x 32 tile, v on the tile + 1-pixel halo into LDS, then the 3 x 3 blend and the clamp
R2L_BLOCKFN void r2l_strong_fwd_sharp_block(const R2LStrongArgs& a, int bid, int nblk, float* lds) {
  const int H = a.g.H, W = a.g.W;
  const int ntx = (W + R2L_AUGS_TW - 1) / R2L_AUGS_TW, nty = (H + R2L_AUGS_TH - 1) / R2L_AUGS_TH;
  const long ntiles = (long)a.g.N * ntx * nty;
  for (long t = bid; t < ntiles; t += nblk) {
    const int pl = (int)(t / ((long)ntx * nty)), rem = (int)(t - (long)pl * ntx * nty);
    const int y0 = (rem / ntx) * R2L_AUGS_TH, x0 = (rem % ntx) * R2L_AUGS_TW;
    R2L_PHASE_BEGIN
    for (int c = tid; c < R2L_AUGS_EH * (R2L_AUGS_EW / 4); c += R2L_NT) {
      const int er = c / (R2L_AUGS_EW / 4), ec = c - er * (R2L_AUGS_EW / 4);
      const int i = y0 - 1 + er, j0 = x0 - 4 + 4 * ec;
      float v[4] = {0.f, 0.f, 0.f, 0.f};
      if (i >= 0 && i < H) {
        const int lo = x0 - 1 > 0 ? x0 - 1 : 0, hi = x0 + R2L_AUGS_TW < W - 1 ? x0 + R2L_AUGS_TW : W - 1;
        r2l_strong_v4(a, pl, i, j0, lo, hi, v);
      }
      float* d = lds + er * R2L_AUGS_EW + 4 * ec;
      d[0] = v[0];
      d[1] = v[1];
      d[2] = v[2];
      d[3] = v[3];
    }
    R2L_PHASE_END
    R2L_PHASE_BEGIN
    {
      const int tr = tid / (R2L_AUGS_TW / 4), tc = tid - tr * (R2L_AUGS_TW / 4);
      const int i = y0 + tr, j0 = x0 + 4 * tc;
      if (i < H && j0 < W) {
        float o[4];
        unsigned char m[4];
        for (int k = 0; k < 4; ++k) {
          const int j = j0 + k;
          const float* c = lds + (tr + 1) * R2L_AUGS_EW + 4 + 4 * tc + k;
          const float v = c[0];
          float dg = v;
          if (i > 0 && i < H - 1 && j > 0 && j < W - 1) {  // conv2d(ones(3,3) / 13, centre 5 / 13), valid, row-major taps
            dg = c[-R2L_AUGS_EW - 1] * R2L_AUGS_W1;
            dg = dg + c[-R2L_AUGS_EW] * R2L_AUGS_W1;
            dg = dg + c[-R2L_AUGS_EW + 1] * R2L_AUGS_W1;
            dg = dg + c[-1] * R2L_AUGS_W1;
            dg = dg + v * R2L_AUGS_W5;
            dg = dg + c[1] * R2L_AUGS_W1;
            dg = dg + c[R2L_AUGS_EW - 1] * R2L_AUGS_W1;
            dg = dg + c[R2L_AUGS_EW] * R2L_AUGS_W1;
            dg = dg + c[R2L_AUGS_EW + 1] * R2L_AUGS_W1;
          }
          const float pre = a.r * v + a.s * dg;
          m[k] = (pre >= 0.0f && pre <= 1.0f) ? 1 : 0;
          o[k] = pre < 0.0f ? 0.0f : (pre > 1.0f ? 1.0f : pre);  // torch.clamp(0, 1); (a NaN passes through)
        }
        const size_t base = ((size_t)pl * H + i) * W + j0;
        r2l_strong_store4(a.y + base, j0, W, o);
        if (a.mask)
          for (int k = 0; k < 4 && j0 + k < W; ++k) a.mask[base + k] = m[k];
      }
    }
    R2L_PHASE_END
  }
}
// backward 1 (sharpness drawn): gv = r h + (1 - r) D^T h, h = m * gy; D^T: identity on the border, the (symmetric) 3 x 3
// weights over the INTERIOR neighbours (the pixels whose blur reads this one)
R2L_BLOCKFN void r2l_strong_bwd_sharp_block(const R2LStrongBwdArgs& a, int bid, int nblk, float* lds) {
  (void)lds;
  const int H = a.g.H, W = a.g.W, cw = (W + 3) >> 2;
  const size_t nch = (size_t)a.g.N * H * cw;
  R2L_PHASE_BEGIN
  for (size_t c = (size_t)bid * R2L_NT + tid; c < nch; c += (size_t)nblk * R2L_NT) {
    const size_t row = c / cw;
    const int j0 = (int)(c - row * cw) * 4, pl = (int)(row / H), i = (int)(row - (size_t)pl * H);
    const size_t pb = (size_t)pl * H * W;
    float o[4] = {0.f, 0.f, 0.f, 0.f};
    for (int k = 0; k < 4 && j0 + k < W; ++k) {
      const int j = j0 + k;
      const size_t e = pb + (size_t)i * W + j;
      const float h = a.mask[e] ? a.gy[e] : 0.0f;
      const bool border = i == 0 || i == H - 1 || j == 0 || j == W - 1;
      float dt = border ? h : 0.0f;
      for (int di = -1; di <= 1; ++di) {
        const int ii = i + di;
        if (ii < 1 || ii > H - 2) continue;
        for (int dj = -1; dj <= 1; ++dj) {
          const int jj = j + dj;
          if (jj < 1 || jj > W - 2) continue;
          const size_t q = pb + (size_t)ii * W + jj;
          const float hq = a.mask[q] ? a.gy[q] : 0.0f;
          dt = dt + hq * ((di | dj) ? R2L_AUGS_W1 : R2L_AUGS_W5);
        }
      }
      o[k] = a.r * h + a.s * dt;
    }
    r2l_strong_store4(a.gv + row * W + j0, j0, W, o);
  }
  R2L_PHASE_END
}
// backward 2: rotation (+ flips) adjoint as a gather.  Source pixel s of the flipped frame collects gv[q] of every output
// q with src(q) == s.  The cell that rounds to s is a unit square around s; its preimage is a unit square (rotated) around
// the inverse-rotated position c of s, whose points are within sqrt(2)/2 of c in each axis -- so every such q lies among
// the 3 x 3 pixels around round(c), each confirmed with r2l_strong_src itself (tests/test_strong_augmentation.py checks the
// search exhaustively)
R2L_BLOCKFN void r2l_strong_bwd_rot_block(const R2LStrongBwdArgs& a, int bid, int nblk, float* lds) {
  (void)lds;
  const int H = a.g.H, W = a.g.W, cw = (W + 3) >> 2;
  const size_t nch = (size_t)a.g.N * H * cw;
  // inverse of the sampling map in pixel units: ix - (W-1)/2 = (W/2 txx) bx + (W/2 txy) by (likewise iy), approximately
  const float m00 = 0.5f * W * a.g.txx, m01 = 0.5f * W * a.g.txy, m10 = 0.5f * H * a.g.tyx, m11 = 0.5f * H * a.g.tyy;
  const float det = m00 * m11 - m01 * m10;
  const float i00 = det != 0.0f ? m11 / det : 0.0f, i01 = det != 0.0f ? -m01 / det : 0.0f;
  const float i10 = det != 0.0f ? -m10 / det : 0.0f, i11 = det != 0.0f ? m00 / det : 0.0f;
  R2L_PHASE_BEGIN
  for (size_t c = (size_t)bid * R2L_NT + tid; c < nch; c += (size_t)nblk * R2L_NT) {
    const size_t row = c / cw;
    const int j0 = (int)(c - row * cw) * 4, pl = (int)(row / H), r = (int)(row - (size_t)pl * H);
    const float* gp = a.gv + (size_t)pl * H * W;
    float o[4] = {0.f, 0.f, 0.f, 0.f};
    for (int k = 0; k < 4 && j0 + k < W; ++k) {
      const int si = a.g.vflip ? H - 1 - r : r, sj = a.g.hflip ? W - 1 - (j0 + k) : j0 + k;  // flips are involutions
      float acc = 0.0f;
      if (!a.g.rot) {
        acc = gp[(size_t)si * W + sj];
      } else {
        const float sx = (float)sj - 0.5f * (float)(W - 1), sy = (float)si - 0.5f * (float)(H - 1);
        const float cx = i00 * sx + i01 * sy + 0.5f * (float)(W - 1), cy = i10 * sx + i11 * sy + 0.5f * (float)(H - 1);
        const int qi0 = (int)rintf(cy), qj0 = (int)rintf(cx);
        for (int qi = qi0 - 1; qi <= qi0 + 1; ++qi) {
          if (qi < 0 || qi >= H) continue;
          for (int qj = qj0 - 1; qj <= qj0 + 1; ++qj) {
            if (qj < 0 || qj >= W) continue;
            int ti, tj;
            if (r2l_strong_src(a.g, qi, qj, ti, tj) && ti == si && tj == sj) acc = acc + gp[(size_t)qi * W + qj];
          }
        }
      }
      o[k] = acc;
    }
    r2l_strong_store4(a.gx + row * W + j0, j0, W, o);
  }
  R2L_PHASE_END
}

#pragma clang fp contract(fast)
