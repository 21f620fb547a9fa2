// r2l_corruptions.h -- the common-corruption set (utils/hendrycks_robustness.py: Distortions) as fused kernels.
//
// The eleven transforms of the reference's C-testing sweep (figures/ABtesting.py) minus elastic_transform, on a whole
// (N,3,H,W) float32 batch, with the T.Normalize(mean, std) that follows them in the reference's Compose optionally
// folded into the stores ((y - mean[c]) / std[c]: subtract, then divide).  Four kernels:
//   point   4 pixels of a row per lane, all three channels in registers: identity (for the Normalize alone), the HSV pair
//           (brightness, saturate: scikit-image 0.18's rgb2hsv / hsv2rgb), the four noises (in-kernel Philox4x32-10) and
//           the apply pass of contrast;
//   mean    contrast's per-plane means: one workgroup per plane, a summation order fixed by R2L_NT alone, float64;
//   blur    gaussian_blur: both passes of the separable filter in one launch through an LDS tile with a halo
//           (scipy.ndimage.gaussian_filter over H then W, mode='nearest', radius <= 4, taps from the host);
//   zoom    zoom_blur: every output pixel accumulates one bilinear sample per zoom factor (scipy.ndimage.zoom(order=1) of
//           the centred crop, trimmed back), coordinates in float64 like scipy's so that the last row and column -- where
//           the coordinate reaches the crop's edge and rounding decides between the edge pixel and scipy's cval 0 -- agree.
// Every kernel walks its work items with a grid stride and no value depends on the walk: results are bit-identical for
// every launch shape.  No atomics, no global state; the caller owns all memory.
#pragma once
#include "r2l_augment_strong.h"

// the reference's expressions, rounded at every step (no fma), so that a batch and its images one by one give the same bits
#pragma clang fp contract(off)

#define R2L_CBLUR_R 4     // largest radius: int(4 sigma + .5) for sigma <= 1.124
#define R2L_CBLUR_TW 64   // output tile 64 x 32: one lane per 4 pixels of a row
#define R2L_CBLUR_TH 32
#define R2L_CBLUR_EW (R2L_CBLUR_TW + 2 * R2L_CBLUR_R)
#define R2L_CBLUR_EH (R2L_CBLUR_TH + 2 * R2L_CBLUR_R)
#define R2L_CBLUR_LDS_FLOATS (R2L_CBLUR_EH * R2L_CBLUR_EW + R2L_CBLUR_TH * R2L_CBLUR_EW)
#define R2L_CMEAN_LDS_FLOATS (2 * R2L_NT)  // R2L_NT doubles
#define R2L_CZOOM_MAXF 32                  // zoom factors of one call (severity 5: 26)

struct R2LCorruptIO {
  const float* x;
  float* y;
  int N, H, W;  // N images of 3 planes of H x W
  int norm;     // store (y - mean[c]) / std[c]
  float mean[3], std[3];
};
struct R2LCorruptArgs {
  R2LCorruptIO io;
  float c0, c1;                        // the severity's constants
  unsigned thresh;                     // impulse_noise: an element flips when its first Philox output is below this
  unsigned long long seed, offset;     // Philox key / counter offset
  float* means;                        // contrast: [3 N] plane means (workspace)
  int radius;                          // gaussian_blur
  float taps[R2L_CBLUR_R + 1];         // taps[|t|], float64 on the host, rounded once
};
struct R2LCorruptZoomArgs {
  R2LCorruptIO io;
  int nf;
  float denom;                         // nf + 1
  int ch[R2L_CZOOM_MAXF], top[R2L_CZOOM_MAXF], trim[R2L_CZOOM_MAXF];
  double scale[R2L_CZOOM_MAXF];        // (ch - 1) / (out_size - 1)
};

R2L_HD float r2l_corrupt_clip(float v) { return v < 0.0f ? 0.0f : (v > 1.0f ? 1.0f : v); }  // np.clip(., 0, 1); a NaN passes
R2L_HD void r2l_corrupt_load4(const float* p, int j0, int W, float v[4]) {
  if (j0 + 3 < W && ((uintptr_t)p & 15) == 0) {
    const r2l_f4 t = *(const r2l_f4*)p;
    v[0] = t.x;
    v[1] = t.y;
    v[2] = t.z;
    v[3] = t.w;
  } else {
    for (int k = 0; k < 4; ++k) v[k] = j0 + k < W ? p[k] : 0.0f;
  }
}
// the clipped values of channel c -> y, normalised when asked
R2L_HD void r2l_corrupt_store4(const R2LCorruptIO& io, int c, float* p, int j0, float v[4]) {
  if (io.norm) {
    const float m = io.mean[c], s = io.std[c];
    R2L_PRAGMA_UNROLL
    for (int k = 0; k < 4; ++k) v[k] = (v[k] - m) / s;
  }
  r2l_strong_store4(p, j0, io.W, v);
}
// r2l_add_noise_philox's deviates of the flat elements e .. e + 3 (4 consecutive elements span at most 2 Philox groups)
R2L_HD void r2l_corrupt_normal4(unsigned long long seed, unsigned long long offset, size_t e, float n[4]) {
  size_t have = ~(size_t)0;
  float nz[4] = {0.f, 0.f, 0.f, 0.f};
  for (int k = 0; k < 4; ++k) {
    const size_t grp = (e + k) >> 2;
    if (grp != have) {
      unsigned o[4];
      r2l_philox4x32_10((unsigned)grp, (unsigned)(grp >> 32), (unsigned)offset, (unsigned)(offset >> 32), (unsigned)seed,
                        (unsigned)(seed >> 32), o);
      r2l_box_muller(o[0], o[1], nz[0], nz[1]);
      r2l_box_muller(o[2], o[3], nz[2], nz[3]);
      have = grp;
    }
    n[k] = nz[(e + k) & 3];
  }
}
// Block `blk` of element e's OWN Philox sub-sequence: counter = (e low, e high | blk << 8, offset), e < 2^40.  What one
// element consumes never moves a neighbour's draws.
R2L_HD void r2l_corrupt_element_draws(unsigned long long seed, unsigned long long offset, size_t e, unsigned blk, unsigned o[4]) {
  r2l_philox4x32_10((unsigned)e, (unsigned)(e >> 32) | (blk << 8), (unsigned)offset, (unsigned)(offset >> 32), (unsigned)seed,
                    (unsigned)(seed >> 32), o);
}
// a Philox output -> a uniform strictly inside (0, 1): (o >> 9) + 1/2 has 24 significant bits, so it and its product with 2^-23
// are exact in float32; smallest value 2^-24, largest 1 - 2^-24
R2L_HD float r2l_corrupt_u23(unsigned o) { return ((float)(o >> 9) + 0.5f) * 1.1920928955078125e-7f; }
// ln k!, k < 10
R2L_HD float r2l_corrupt_lnfact(int k) {
  const float t[10] = {0.0f,          0.0f,          0.6931471806f, 1.7917594692f, 3.1780538303f,
                       4.7874917428f, 6.5792512120f, 8.5251613611f, 10.604602903f, 12.801827480f};
  return t[k];
}
// Poisson(lam), lam < 10, by inversion: the sequential search for the first k whose cumulative probability reaches u.  The
// probabilities and their sum are float64 (a float32 sum is off by a few 1e-7 after 30 terms and moves the top quantiles by one
// or two k, or stalls under the largest u), so the only discretisation is u's own 2^-23 grid and the largest u gives the k
// whose upper tail is 2^-24.  The walk ends at that k; should the sum ever stop growing first, it ends there, not at a bound on k.
R2L_HD float r2l_corrupt_poisson_walk(float lam, unsigned o) {
  const double u = (double)r2l_corrupt_u23(o), l = (double)lam;
  double p = exp(-l), s = p;
  int k = 0;
  while (u > s) {
    ++k;
    p *= l / (double)k;
    const double t = s + p;
    if (t == s) break;
    s = t;
  }
  return (float)k;
}
// Poisson(lam), lam >= 10: Hoermann's transformed rejection with squeeze (PTRS, 1993).  One candidate from two Philox
// outputs; true when it is accepted.  us >= 2^-24 > 0 for every output.  The acceptance test's right-hand side
// k ln(lam) - lam - ln k! is taken through Stirling's series as (k - lam) + k log1p(-(k - lam) / k) - ln(2 pi k) / 2 - 1/(12 k)
// + 1/(360 k^3): the terms that cancel to ~ -d^2 / 2k are of size |d| instead of k ln k, so float32 decides it to ~ 1e-5
// (series error at k >= 10: 8e-9).
struct R2LPtrs {
  float lam, b, a, invalpha, vr;
};
R2L_HD R2LPtrs r2l_corrupt_ptrs_setup(float lam) {
  R2LPtrs c;
  c.lam = lam;
  c.b = 0.931f + 2.53f * sqrtf(lam);
  c.a = -0.059f + 0.02483f * c.b;
  c.invalpha = 1.1239f + 1.1328f / (c.b - 3.4f);
  c.vr = 0.9277f - 3.6224f / (c.b - 2.0f);
  return c;
}
R2L_HD bool r2l_corrupt_ptrs_try(const R2LPtrs& c, unsigned ou, unsigned ov, float& k) {
  const float U = r2l_corrupt_u23(ou) - 0.5f, V = r2l_corrupt_u23(ov);
  const float us = 0.5f - fabsf(U);
  k = floorf((2.0f * c.a / us + c.b) * U + c.lam + 0.43f);
  if (us >= 0.07f && V <= c.vr) return true;
  if (k < 0.0f || (us < 0.013f && V > us)) return false;
  const float lhs = logf(V * c.invalpha / (c.a / (us * us) + c.b));
  float rhs;
  if (k < 10.0f) {
    rhs = k * logf(c.lam) - c.lam - r2l_corrupt_lnfact((int)k);
  } else {
    const float d = k - c.lam, ik = 1.0f / k;
    rhs = (d + k * log1pf(-d * ik)) - 0.5f * logf(6.2831853071795865f * k) - ik * (1.0f / 12.0f) + ik * ik * ik * (1.0f / 360.0f);
  }
  return lhs <= rhs;
}
// Poisson(lam) for element e from its own Philox sub-sequence: one output below lam = 10, two per PTRS candidate above
R2L_HD float r2l_corrupt_poisson(float lam, unsigned long long seed, unsigned long long offset, size_t e) {
  if (!(lam > 0.0f)) return 0.0f;
  unsigned o[4];
  if (lam < 10.0f) {
    r2l_corrupt_element_draws(seed, offset, e, 0, o);
    return r2l_corrupt_poisson_walk(lam, o[0]);
  }
  const R2LPtrs c = r2l_corrupt_ptrs_setup(lam);
  float k;
  for (unsigned blk = 0; blk < 64; ++blk) {  // two candidates per block; a candidate is rejected with probability < 0.3
    r2l_corrupt_element_draws(seed, offset, e, blk, o);
    if (r2l_corrupt_ptrs_try(c, o[0], o[1], k)) return k;
    if (r2l_corrupt_ptrs_try(c, o[2], o[3], k)) return k;
  }
  return floorf(lam);
}
// scikit-image 0.18: rgb2hsv, the edit of V (brightness: clip(V + c0)) or S (saturate: clip(S c0 + c1)), hsv2rgb
template <int SAT>
R2L_HD void r2l_corrupt_hsv(float c0, float c1, float& r, float& g, float& b) {
  const float v = fmaxf(r, fmaxf(g, b)), delta = v - fminf(r, fminf(g, b));
  float h = 0.0f, s = 0.0f;
  if (delta != 0.0f) {
    s = delta / v;
    float h6 = (g - b) / delta;                 // red is the maximum
    if (g == v) h6 = 2.0f + (b - r) / delta;    // green (assigned later: wins a tie with red)
    if (b == v) h6 = 4.0f + (r - g) / delta;    // blue (wins every tie)
    h = h6 / 6.0f;
    h = h - floorf(h);                          // % 1.
  }
  float vv = v;
  if (SAT)
    s = r2l_corrupt_clip(s * c0 + c1);
  else
    vv = r2l_corrupt_clip(v + c0);
  const float hs = h * 6.0f, hi = floorf(hs), f = hs - hi;
  const float p = vv * (1.0f - s), q = vv * (1.0f - f * s), t = vv * (1.0f - (1.0f - f) * s);
  switch ((int)hi % 6) {  // (hi = 6 when h rounded up to 1: sector 0 with f = 0, the same colour)
    case 0: r = vv; g = t; b = p; break;
    case 1: r = q; g = vv; b = p; break;
    case 2: r = p; g = vv; b = t; break;
    case 3: r = p; g = q; b = vv; break;
    case 4: r = t; g = p; b = vv; break;
    default: r = vv; g = p; b = q; break;
  }
}

// ---- point: identity / noises / HSV pair / contrast's apply pass ------------------------------------------------------
template <int KIND>
R2L_BLOCKFN void r2l_corrupt_point_block(const R2LCorruptArgs& a, int bid, int nblk, float* lds) {
  (void)lds;
  const int H = a.io.H, W = a.io.W, cw = (W + 3) >> 2;
  const size_t hw = (size_t)H * W, nch = (size_t)a.io.N * H * cw;
  R2L_PHASE_BEGIN
  for (size_t c = (size_t)bid * R2L_NT + tid; c < nch; c += (size_t)nblk * R2L_NT) {
    const size_t row = c / cw;
    const int j0 = (int)(c - row * cw) * 4, n = (int)(row / H), i = (int)(row - (size_t)n * H);
    const size_t e0 = (size_t)n * 3 * hw + (size_t)i * W + j0;  // flat index of the first pixel in channel 0
    float v[3][4];
    R2L_PRAGMA_UNROLL
    for (int ch = 0; ch < 3; ++ch) r2l_corrupt_load4(a.io.x + e0 + ch * hw, j0, W, v[ch]);
    if (KIND == R2L_CORRUPT_BRIGHTNESS || KIND == R2L_CORRUPT_SATURATE) {
      R2L_PRAGMA_UNROLL
      for (int k = 0; k < 4; ++k) r2l_corrupt_hsv<KIND == R2L_CORRUPT_SATURATE>(a.c0, a.c1, v[0][k], v[1][k], v[2][k]);
    }
    R2L_PRAGMA_UNROLL
    for (int ch = 0; ch < 3; ++ch) {
      const size_t e = e0 + ch * hw;
      if (KIND == R2L_CORRUPT_GAUSSIAN_NOISE || KIND == R2L_CORRUPT_SPECKLE_NOISE) {
        float nz[4];
        r2l_corrupt_normal4(a.seed, a.offset, e, nz);
        R2L_PRAGMA_UNROLL
        for (int k = 0; k < 4; ++k)
          v[ch][k] = KIND == R2L_CORRUPT_GAUSSIAN_NOISE ? fmaf(nz[k], a.c0, v[ch][k]) : fmaf(v[ch][k], a.c0 * nz[k], v[ch][k]);
      } else if (KIND == R2L_CORRUPT_IMPULSE_NOISE) {
        for (int k = 0; k < 4 && j0 + k < W; ++k) {
          unsigned o[4];
          r2l_corrupt_element_draws(a.seed, a.offset, e + k, 0, o);
          if (o[0] < a.thresh) v[ch][k] = (o[1] >> 31) ? 1.0f : 0.0f;  // flip: output 0; salt or pepper: output 1
        }
      } else if (KIND == R2L_CORRUPT_SHOT_NOISE) {
        for (int k = 0; k < 4 && j0 + k < W; ++k)
          v[ch][k] = r2l_corrupt_poisson(v[ch][k] * a.c0, a.seed, a.offset, e + k) / a.c0;
      } else if (KIND == R2L_CORRUPT_CONTRAST) {
        const float m = a.means[n * 3 + ch];
        R2L_PRAGMA_UNROLL
        for (int k = 0; k < 4; ++k) v[ch][k] = (v[ch][k] - m) * a.c0 + m;
      }
      if (KIND != R2L_CORRUPT_IDENTITY) {
        R2L_PRAGMA_UNROLL
        for (int k = 0; k < 4; ++k) v[ch][k] = r2l_corrupt_clip(v[ch][k]);
      }
      r2l_corrupt_store4(a.io, ch, a.io.y + e, j0, v[ch]);
    }
  }
  R2L_PHASE_END
}

// ---- mean: contrast's per-plane means ---------------------------------------------------------------------------------
// One workgroup per plane.  Lane t adds the groups q = t, t + R2L_NT, .. of 4 consecutive pixels into four float64 sums (one per
// position in the group), the tail pixels hw - hw % 4 .. go to lane 0; then 64 lanes add 8 partial sums each, lane 0 the 64.
// The order is a function of R2L_NT alone -- not of the grid, and not of the plane's alignment (which only picks the load width).
R2L_BLOCKFN void r2l_corrupt_mean_block(const R2LCorruptArgs& a, int bid, int nblk, float* lds) {
  double* red = (double*)lds;
  const size_t hw = (size_t)a.io.H * a.io.W, ng = hw >> 2;
  const int nplanes = a.io.N * 3;
  for (int pl = bid; pl < nplanes; pl += nblk) {
    const float* p = a.io.x + (size_t)pl * hw;
    R2L_PHASE_BEGIN
    double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
    const bool vec = ((uintptr_t)p & 15) == 0;
    for (size_t q = tid; q < ng; q += R2L_NT) {
      float t[4];
      if (vec) {
        const r2l_f4 f = r2l_load_f4_nt(p + 4 * q);
        t[0] = f.x;
        t[1] = f.y;
        t[2] = f.z;
        t[3] = f.w;
      } else {
        for (int k = 0; k < 4; ++k) t[k] = p[4 * q + k];
      }
      s0 += (double)t[0];
      s1 += (double)t[1];
      s2 += (double)t[2];
      s3 += (double)t[3];
    }
    double s = (s0 + s1) + (s2 + s3);
    if (tid == 0)
      for (size_t e = ng << 2; e < hw; ++e) s += (double)p[e];
    red[tid] = s;
    R2L_PHASE_END
    R2L_PHASE_BEGIN
    if (tid < 64) {
      double s = red[tid];
      for (int k = 1; k < R2L_NT / 64; ++k) s += red[tid + 64 * k];
      red[tid] = s;
    }
    R2L_PHASE_END
    R2L_PHASE_BEGIN
    if (tid == 0) {
      double s = red[0];
      for (int k = 1; k < 64; ++k) s += red[k];
      a.means[pl] = (float)(s / (double)hw);
    }
    R2L_PHASE_END
  }
}

// ---- blur: separable Gaussian, both passes through LDS ---------------------------------------------------------------------
// Per 64 x 32 tile: the tile + R2L_CBLUR_R pixels of halo, read at coordinates clamped to the frame (mode='nearest'), the pass
// over H on every column of the extended tile (a halo column holds the clamped column, i.e. what the pass over W reads there),
// then the pass over W, clip, store.  Symmetric taps are applied to the sum of their two pixels, like scipy's correlate1d -- which adds the pairs from the outermost
// inward, in float64; here from the centre outward, in float32.
R2L_BLOCKFN void r2l_corrupt_blur_block(const R2LCorruptArgs& a, int bid, int nblk, float* lds) {
  const int H = a.io.H, W = a.io.W, R = R2L_CBLUR_R, rad = a.radius;
  const int ntx = (W + R2L_CBLUR_TW - 1) / R2L_CBLUR_TW, nty = (H + R2L_CBLUR_TH - 1) / R2L_CBLUR_TH;
  const long ntiles = (long)a.io.N * 3 * ntx * nty;
  float* mid = lds + R2L_CBLUR_EH * R2L_CBLUR_EW;
  for (long t = bid; t < ntiles; t += nblk) {
    const int pl = (int)(t / ((long)ntx * nty)), rem = (int)(t - (long)pl * ntx * nty);
    const int y0 = (rem / ntx) * R2L_CBLUR_TH, x0 = (rem % ntx) * R2L_CBLUR_TW;
    const float* xp = a.io.x + (size_t)pl * H * W;
    R2L_PHASE_BEGIN
    for (int c = tid; c < R2L_CBLUR_EH * R2L_CBLUR_EW; c += R2L_NT) {
      const int er = c / R2L_CBLUR_EW, ec = c - er * R2L_CBLUR_EW;
      int i = y0 - R + er, j = x0 - R + ec;
      i = i < 0 ? 0 : (i > H - 1 ? H - 1 : i);
      j = j < 0 ? 0 : (j > W - 1 ? W - 1 : j);
      lds[c] = xp[(size_t)i * W + j];
    }
    R2L_PHASE_END
    R2L_PHASE_BEGIN
    for (int c = tid; c < R2L_CBLUR_TH * R2L_CBLUR_EW; c += R2L_NT) {
      const float* s = lds + c + R * R2L_CBLUR_EW;
      float acc = s[0] * a.taps[0];
      for (int k = 1; k <= rad; ++k) acc = acc + (s[-k * R2L_CBLUR_EW] + s[k * R2L_CBLUR_EW]) * a.taps[k];
      mid[c] = acc;
    }
    R2L_PHASE_END
    R2L_PHASE_BEGIN
    {
      const int tr = tid / (R2L_CBLUR_TW / 4), tc = tid - tr * (R2L_CBLUR_TW / 4);
      const int i = y0 + tr, j0 = x0 + 4 * tc;
      if (i < H && j0 < W) {
        float o[4];
        for (int k = 0; k < 4; ++k) {
          const float* s = mid + tr * R2L_CBLUR_EW + R + 4 * tc + k;
          float acc = s[0] * a.taps[0];
          for (int q = 1; q <= rad; ++q) acc = acc + (s[-q] + s[q]) * a.taps[q];
          o[k] = r2l_corrupt_clip(acc);
        }
        r2l_corrupt_store4(a.io, pl % 3, a.io.y + ((size_t)pl * H + i) * W + j0, j0, o);
      }
    }
    R2L_PHASE_END
  }
}

// ---- zoom: one bilinear sample per factor ------------------------------------------------------------------------------------
// Factor f: the crop x[top .. top + ch) squared, zoomed to out_size squared by scipy.ndimage.zoom(order=1) (output index o reads
// the crop at o (ch - 1) / (out_size - 1), float64; mode='constant': a coordinate above ch - 1 -- which rounding can give at the
// last index -- reads cval 0), of which the output takes rows and columns trim .. trim + H.  Accumulated in the factors' order in
// float32 like the reference's `out +=`, then (x + sum) / (nf + 1), clip.  Lanes of a wavefront read neighbouring columns of
// two source rows per factor: whole cache lines, like the unrotated gather of section 3.6.
R2L_BLOCKFN void r2l_corrupt_zoom_block(const R2LCorruptZoomArgs& a, int bid, int nblk, float* lds) {
  (void)lds;
  const int H = a.io.H, W = a.io.W, cw = (W + 3) >> 2;
  const size_t nch = (size_t)a.io.N * 3 * H * cw;
  R2L_PHASE_BEGIN
  for (size_t c = (size_t)bid * R2L_NT + tid; c < nch; c += (size_t)nblk * R2L_NT) {
    const size_t row = c / cw;
    const int j0 = (int)(c - row * cw) * 4, pl = (int)(row / H), i = (int)(row - (size_t)pl * H);
    const float* xp = a.io.x + (size_t)pl * H * W;
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    for (int f = 0; f < a.nf; ++f) {
      const int ch = a.ch[f], top = a.top[f], trim = a.trim[f];
      const double sc = a.scale[f], edge = (double)(ch - 1);
      const double cr = (double)(trim + i) * sc;
      const bool rin = cr <= edge;
      const int r0 = rin ? (int)cr : 0, r1 = r0 + 1 < ch ? r0 + 1 : ch - 1;
      const float tr = (float)(cr - (double)r0);
      const float* p0 = xp + (size_t)(top + r0) * W + top;
      const float* p1 = xp + (size_t)(top + r1) * W + top;
      for (int k = 0; k < 4 && j0 + k < W; ++k) {
        const double cc = (double)(trim + j0 + k) * sc;
        float val = 0.0f;
        if (rin && cc <= edge) {
          const int q0 = (int)cc, q1 = q0 + 1 < ch ? q0 + 1 : ch - 1;
          const float tc = (float)(cc - (double)q0);
          const float u0 = (1.0f - tc) * p0[q0] + tc * p0[q1], u1 = (1.0f - tc) * p1[q0] + tc * p1[q1];
          val = (1.0f - tr) * u0 + tr * u1;
        }
        acc[k] = acc[k] + val;
      }
    }
    float v[4];
    r2l_corrupt_load4(xp + (size_t)i * W + j0, j0, W, v);
    for (int k = 0; k < 4; ++k) v[k] = r2l_corrupt_clip((v[k] + acc[k]) / a.denom);
    r2l_corrupt_store4(a.io, pl % 3, a.io.y + row * W + j0, j0, v);
  }
  R2L_PHASE_END
}

#pragma clang fp contract(fast)
