// r2l_driver_util.h -- what the stand-alone drivers of r2l_lockstep_drivers.cpp share.  TEST INFRASTRUCTURE: included once, behind
// r2l_lockstep.cpp (it uses the C ABI's enums and the launch record of r2l_launch.h), in front of the drivers.
#pragma once

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <map>
#include <mutex>
#include <string>
#include <vector>

namespace r2l_drv {

// The drivers' random numbers: `static Lcg lcg01{seed};` then `lcg01()`, uniform in [0, 1).  Every driver has a seed and an order
// of draws of its own; the FNV-1a hashes in tests/golden/*_routes.txt depend on both.
struct Lcg {
  unsigned state;
  float operator()() {
    state = state * 1664525u + 1013904223u;
    return (float)(state >> 8) * (1.0f / 16777216.0f);
  }
};

// A heap block of exactly n elements (malloc, not new[]: no cookie in front, no rounding, the block ends at its last element), so
// that an access which strays past it is an ASan report.
template <class T>
struct Buf {
  T* p;
  size_t n;
  explicit Buf(size_t n_, int fill = 0xff) : p((T*)malloc(n_ ? n_ * sizeof(T) : 1)), n(n_) { memset(p, fill, n_ * sizeof(T)); }
  ~Buf() { free(p); }
  Buf(const Buf&) = delete;
};
typedef Buf<char> Block;

#define CHECK(call)                                                   \
  do {                                                                \
    const int e_ = (call);                                            \
    if (e_) {                                                         \
      fprintf(stderr, "%s -> %d: %s\n", #call, e_, r2l_last_error()); \
      return 1;                                                       \
    }                                                                 \
  } while (0)

inline unsigned long long fnv1a(const void* p, size_t n) {  // FNV-1a 64
  unsigned long long h = 1469598103934665603ull;
  for (size_t i = 0; i < n; ++i) h = (h ^ ((const unsigned char*)p)[i]) * 1099511628211ull;
  return h;
}

// The nine parameter pointers of r2l_isp_step_fwd / _bwd, into a packed block in R2L_P_* order
inline void param_table(const float* P, const float* table[9]) {
  static const int off[9] = {R2L_P_BLACK_LEVEL, R2L_P_WHITE_BALANCE, R2L_P_CCM, R2L_P_GAMMA, R2L_P_DEBAYER, R2L_P_SHARPEN,
                             R2L_P_BLUR, R2L_P_M_RGB2YUV, R2L_P_M_YUV2RGB};
  for (int i = 0; i < 9; ++i) table[i] = P + off[i];
}
// params.bin: 150 float32, the packed parameter block
inline bool read_params(const char* path, float P[R2L_P_COUNT]) {
  FILE* f = fopen(path, "rb");
  const bool ok = f && fread(P, sizeof(float), R2L_P_COUNT, f) == R2L_P_COUNT;
  if (f) fclose(f);
  return ok;
}

// Drone camera: black level, white balance, colour matrix (oracle/isp_oracle.py: DRONE_CAMERA_PARAMS)
static const double CAMERA[16] = {0.0625,      0.0626,      0.0625,      0.0626,     2.86653646,  1.,          1.73079425, 1.50768983,
                                  -0.33571374, -0.17197604, -0.23048614, 1.70698738, -0.47650126, -0.03119153, -0.32803956, 1.35923111};
static const float MEAN_STD[6] = {0.35f, 0.36f, 0.35f, 0.12f, 0.11f, 0.12f};  // train.py:157-158

// px raw values lo + span * lcg() in the container `frames` names (R2L_FRAMES_*; 16-bit containers: of 65535), one draw per pixel
inline size_t raw_bytes(int frames) { return frames == R2L_FRAMES_F64 ? 8 : (frames == R2L_FRAMES_U16 ? 2 : 4); }
inline void fill_raw(Lcg& lcg, void* raw, size_t px, int frames, float lo, float span) {
  for (size_t i = 0; i < px; ++i) {
    const float v = lo + span * lcg();
    if (frames == R2L_FRAMES_U16) ((unsigned short*)raw)[i] = (unsigned short)(v * 65535.f);
    else if (frames == R2L_FRAMES_F64) ((double*)raw)[i] = (double)v;
    else ((float*)raw)[i] = v;
  }
}

// The launch record of r2l_launch.h (kernel -> launches), emptied and switched on
inline void record_begin() {
  std::lock_guard<std::mutex> g(r2l_ls_record_mutex);
  r2l_ls_record.clear();
  r2l_ls_record_on = true;
}

}  // namespace r2l_drv
