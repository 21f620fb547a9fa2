// r2l_entries_lockstep.cpp -- driver `entries` of r2l_lockstep_drivers.cpp (stand-alone, no Python): what every public step and
// static entry point of the C ABI answers, on the lock-step emulation's sources (r2l_lockstep.cpp, unchanged) under
// -fsanitize=address,undefined.  It uses the public C ABI only (and the parameter block of the fwd_routes driver), so the same source
// compiles against an earlier commit.  TEST INFRASTRUCTURE: run by tests/test_entry_points.py, which compares the output byte for
// byte with tests/golden/entry_points.txt (tests/entry_points_record.py: how that file is regenerated).
//   X  a call that is refused, through every entry that takes the argument: return code and r2l_last_error(), so that which check
//      runs for which entry, in which order and under which name is on record
//   F  the flavours of one call through every entry that can express it, at 1x16x16 and 2x16x24: FNV-1a 64 of every result.  The
//      lines of one group must carry the same digests (the driver fails where they do not)
//   usage: r2l_lockstep_drivers entries
#include <array>

namespace r2l_drv::entries {

static Lcg lcg01{97531u};
static int failures = 0;
static const int K = R2L_STEP_KEEP_LUMA;

// ---- the calls, by entry -------------------------------------------------------------------------------------------------------
static const char* const FWD_NAMES[3] = {"step_fwd", "step_fwd_io", "step_fwd_layout"};
struct Fwd {
  int entry = 0;
  const void* raw = nullptr;
  int u16 = 0;
  float denom = 65535.f;
  const float* const* table = nullptr;
  const float* additive = nullptr;
  int bn_mode = R2L_BN_NONE;
  float *rm = nullptr, *rv = nullptr;
  long long* nbt = nullptr;
  void* out = nullptr;
  int io = R2L_IO_F32, layout = R2L_LAYOUT_NCHW;
  void* ws = nullptr;
  size_t nws = 0;
  int B = 1, H = 8, W = 8, nranks = 1, phase = K;
  const double* gathered = nullptr;
};
static int call(const Fwd& q) {
  if (q.entry == 0)
    return r2l_isp_step_fwd(q.raw, q.u16, q.denom, q.table, q.additive, q.bn_mode, q.rm, q.rv, q.nbt, 1e-5, 0.1, (float*)q.out, q.ws, q.nws, q.B,
                            q.H, q.W, q.nranks, q.phase, q.gathered, nullptr);
  if (q.entry == 1)
    return r2l_isp_step_fwd_io(q.raw, q.u16, q.denom, q.table, q.additive, q.bn_mode, q.rm, q.rv, q.nbt, 1e-5, 0.1, q.out, q.io, q.ws, q.nws, q.B,
                               q.H, q.W, q.nranks, q.phase, q.gathered, nullptr);
  return r2l_isp_step_fwd_layout(q.raw, q.u16, q.denom, q.table, q.additive, q.bn_mode, q.rm, q.rv, q.nbt, 1e-5, 0.1, q.out, q.io, q.layout, q.ws,
                                 q.nws, q.B, q.H, q.W, q.nranks, q.phase, q.gathered, nullptr);
}
static const char* const BWD_NAMES[5] = {"step_bwd", "step_bwd_raw", "step_bwd_select", "step_bwd_io", "step_bwd_layout"};
struct Bwd {
  int entry = 0;
  const void* raw = nullptr;
  int u16 = 0;
  float denom = 65535.f;
  const float* additive = nullptr;
  const void* gout = nullptr;
  int io = R2L_IO_F32, layout = R2L_LAYOUT_NCHW;
  const void* out = nullptr;
  float *gp = nullptr, *gadd = nullptr;
  int bn_mode = R2L_BN_NONE;
  void* ws = nullptr;
  size_t nws = 0;
  int B = 1, H = 8, W = 8, nranks = 1, phase = K;
  const double* gathered = nullptr;
  float* graw = nullptr;
  void* scr = nullptr;
  size_t nscr = 0;
  unsigned mask = 0;
};
static int call(const Bwd& q) {
  const float *go = (const float*)q.gout, *o = (const float*)q.out;
  switch (q.entry) {
    case 0:
      return r2l_isp_step_bwd(q.raw, q.u16, q.denom, q.additive, go, o, q.gp, q.gadd, q.bn_mode, q.ws, q.nws, q.B, q.H, q.W, q.nranks, q.phase,
                              q.gathered, nullptr);
    case 1:
      return r2l_isp_step_bwd_raw(q.raw, q.u16, q.denom, q.additive, go, o, q.gp, q.gadd, q.bn_mode, q.ws, q.nws, q.B, q.H, q.W, q.nranks, q.phase,
                                  q.gathered, nullptr, q.graw, q.scr, q.nscr);
    case 2:
      return r2l_isp_step_bwd_select(q.raw, q.u16, q.denom, q.additive, go, o, q.gp, q.gadd, q.bn_mode, q.ws, q.nws, q.B, q.H, q.W, q.nranks,
                                     q.phase, q.gathered, nullptr, q.graw, q.scr, q.nscr, q.mask);
    case 3:
      return r2l_isp_step_bwd_io(q.raw, q.u16, q.denom, q.additive, q.gout, q.io, q.out, q.gp, q.gadd, q.bn_mode, q.ws, q.nws, q.B, q.H, q.W,
                                 q.nranks, q.phase, q.gathered, nullptr, q.graw, q.scr, q.nscr, q.mask);
    default:
      return r2l_isp_step_bwd_layout(q.raw, q.u16, q.denom, q.additive, q.gout, q.io, q.layout, q.out, q.gp, q.gadd, q.bn_mode, q.ws, q.nws, q.B,
                                     q.H, q.W, q.nranks, q.phase, q.gathered, nullptr, q.graw, q.scr, q.nscr, q.mask);
  }
}
static const char* const STA_NAMES[6] = {"static_fwd", "static_fwd_u16", "static_fwd_f64", "static_fwd_norm", "static_fwd_opts", "static_fwd_io"};
static const int STA_FRAMES[3] = {R2L_FRAMES_F32, R2L_FRAMES_U16, R2L_FRAMES_F64};  // what entries 0, 1, 2 read
struct Sta {
  int entry = 0;
  const void* raw = nullptr;
  int frames = R2L_FRAMES_F32;  // entries 3, 4, 5
  void* out = nullptr;
  int out_io = R2L_IO_F32;  // entry 5
  int B = 1, H = 8, W = 8;
  const double* cam = CAMERA;
  int deb = R2L_DEBAYER_BILINEAR, sha = R2L_SHARPEN_FILTER, den = R2L_DENOISE_GAUSSIAN;
  double gamma = 2.2;
  const double* opts = nullptr;  // entries 4, 5
  const float* ms = nullptr;     // entries 3, 4, 5
  void* ws = nullptr;
  size_t nws = 0;
};
static int call(const Sta& q) {
  float* o = (float*)q.out;
  switch (q.entry) {
    case 0:
      return r2l_static_fwd((const float*)q.raw, o, q.B, q.H, q.W, q.cam, q.deb, q.sha, q.den, q.gamma, q.ws, q.nws, nullptr);
    case 1:
      return r2l_static_fwd_u16((const unsigned short*)q.raw, 65535.f, o, q.B, q.H, q.W, q.cam, q.deb, q.sha, q.den, q.gamma, q.ws, q.nws, nullptr);
    case 2:
      return r2l_static_fwd_f64((const double*)q.raw, o, q.B, q.H, q.W, q.cam, q.deb, q.sha, q.den, q.gamma, q.ws, q.nws, nullptr);
    case 3:
      return r2l_static_fwd_norm(q.raw, q.frames, 65535.f, o, q.B, q.H, q.W, q.cam, q.deb, q.sha, q.den, q.gamma, q.ms, q.ws, q.nws, nullptr);
    case 4:
      return r2l_static_fwd_opts(q.raw, q.frames, 65535.f, o, q.B, q.H, q.W, q.cam, q.deb, q.sha, q.den, q.gamma, q.opts, q.ms, q.ws, q.nws,
                                 nullptr);
    default:
      return r2l_static_fwd_io(q.raw, q.frames, 65535.f, q.out, q.out_io, q.B, q.H, q.W, q.cam, q.deb, q.sha, q.den, q.gamma, q.opts, q.ms, q.ws,
                               q.nws, nullptr);
  }
}

// ---- X lines -------------------------------------------------------------------------------------------------------------------
// the tensors of a call of up to 2 x 16 x 16 that would run if it were not refused (the backward's workspace: behind a forward)
struct World {
  Block raw{512 * 8, 0x3c}, out{3 * 512 * 4 + 16}, gout{3 * 512 * 4 + 16, 0x3c}, ws{r2l_isp_workspace_bytes(2, 16, 16)}, scr{2 * 512 * 4 + 16};
  Block sws{1 << 20};
  Buf<float> gp{R2L_P_NTRAIN}, graw{512 + 4}, gadd{3 * 256 * 256};
  float rm[3] = {0.4f, 0.45f, 0.35f}, rv[3] = {0.03f, 0.05f, 0.04f};
  long long nbt = 0;
  double gathered[7] = {1, 1, 1, 2, 2, 2, 64};
};
static World* world;
static Fwd fwd_base() {
  World& w = *world;
  Fwd q;
  q.raw = w.raw.p, q.table = fwd_routes::TABLE, q.rm = w.rm, q.rv = w.rv, q.nbt = &w.nbt, q.out = w.out.p, q.ws = w.ws.p;
  q.nws = w.ws.n;
  return q;
}
static Bwd bwd_base() {
  World& w = *world;
  Bwd q;
  q.raw = w.raw.p, q.gout = w.gout.p, q.out = w.out.p, q.gp = w.gp.p, q.ws = w.ws.p;
  q.nws = w.ws.n;
  return q;
}
static Sta sta_base() {
  World& w = *world;
  Sta q;
  q.raw = w.raw.p, q.out = w.out.p, q.ws = w.sws.p, q.nws = w.sws.n;
  return q;
}
template <class Q, class M>
static void refused(const char* const* names, std::initializer_list<int> entries, const char* tag, Q base, M mutate) {
  for (int entry : entries) {
    Q q = base;
    q.entry = entry;
    mutate(q);
    const int e = call(q);
    printf("X %s: %s -> %d [%s]\n", names[entry], tag, e, e ? r2l_last_error() : "");
  }
}
#define ALL_FWD {0, 1, 2}
#define ALL_BWD {0, 1, 2, 3, 4}
#define MASKED {2, 3, 4}
#define ALL_STA {0, 1, 2, 3, 4, 5}
#define FRAMED {3, 4, 5}
#define IO_FWD {1, 2}
#define IO_BWD {3, 4}
#define RAW_BWD {1, 2, 3, 4}
#define OPT_STA {4, 5}
#define BADF(entries, tag, ...) refused(FWD_NAMES, entries, tag, fwd_base(), [&](Fwd& q) { __VA_ARGS__; });
#define BADB(entries, tag, ...) refused(BWD_NAMES, entries, tag, bwd_base(), [&](Bwd& q) { __VA_ARGS__; });
#define BADS(entries, tag, ...) refused(STA_NAMES, entries, tag, sta_base(), [&](Sta& q) { __VA_ARGS__; });

static void refusals_fwd() {
  World& w = *world;
  BADF(ALL_FWD, "null raw", q.raw = nullptr)
  BADF(ALL_FWD, "null out", q.out = nullptr)
  BADF(ALL_FWD, "null workspace", q.ws = nullptr)
  BADF(ALL_FWD, "bn_mode 3", q.bn_mode = 3)
  BADF(ALL_FWD, "phase 3", q.phase = 3 | K)
  BADF(ALL_FWD, "nranks 0", q.nranks = 0)
  BADF(ALL_FWD, "two ranks, ALL, train", q.nranks = 2; q.bn_mode = R2L_BN_TRAIN)
  BADF(ALL_FWD, "phase B without gathered", q.phase = R2L_STEP_B | K; q.bn_mode = R2L_BN_TRAIN)
  BADF(ALL_FWD, "eval without running statistics", q.bn_mode = R2L_BN_EVAL; q.rm = q.rv = nullptr)
  BADF(ALL_FWD, "running_mean alone", q.rv = nullptr)
  BADF(ALL_FWD, "workspace one byte short", q.nws = r2l_isp_workspace_bytes(q.B, q.H, q.W) - 1)
  BADF(ALL_FWD, "rot90 on 8 x 12", q.W = 12; q.phase = 1 << R2L_STEP_EPI_ROT_SHIFT)
  BADF(ALL_FWD, "B = 0", q.B = 0)
  BADF(ALL_FWD, "null parameter table", q.table = nullptr)
  for (int io : {R2L_IO_F32, R2L_IO_BF16}) {  // (the same refusals where r2l_io_check has looked at the call)
    const std::string s = io ? "bf16: " : "f32: ";
    BADF(IO_FWD, (s + "io 7").c_str(), q.io = 7)
    BADF({2}, (s + "layout 5").c_str(), q.io = io; q.layout = 5)
    BADF(IO_FWD, (s + "null out").c_str(), q.io = io; q.out = nullptr)
    BADF(IO_FWD, (s + "bn_mode 3").c_str(), q.io = io; q.bn_mode = 3)
    BADF(IO_FWD, (s + "workspace one byte short").c_str(), q.io = io; q.nws = r2l_isp_workspace_bytes(q.B, q.H, q.W) - 1)
    BADF(IO_FWD, (s + "no KEEP_LUMA").c_str(), q.io = io; q.phase = 0)
    BADF(IO_FWD, (s + "additive layer").c_str(), q.io = io; q.additive = w.gadd.p)
    BADF(IO_FWD, (s + "W % 4").c_str(), q.io = io; q.W = 10)
    BADF(IO_FWD, (s + "epilogue").c_str(), q.io = io; q.phase = K | R2L_STEP_EPI_HFLIP)
    if (io) BADF(IO_FWD, (s + "out 4 bytes off").c_str(), q.io = io; q.out = w.out.p + 4)
    BADF({2}, (s + "channels-last, out 8 bytes off").c_str(), q.io = io; q.layout = R2L_LAYOUT_NHWC; q.out = w.out.p + 8)
    BADF({2}, (s + "channels-last, out 4 bytes off").c_str(), q.io = io; q.layout = R2L_LAYOUT_NHWC; q.out = w.out.p + 4)
    BADF({2}, (s + "channels-last, no KEEP_LUMA").c_str(), q.io = io; q.layout = R2L_LAYOUT_NHWC; q.phase = 0)
  }
}
static void refusals_bwd() {
  World& w = *world;
  BADB(ALL_BWD, "null raw", q.raw = nullptr)
  BADB(ALL_BWD, "null grad_out", q.gout = nullptr)
  BADB(ALL_BWD, "null workspace", q.ws = nullptr)
  BADB(ALL_BWD, "bn_mode 3", q.bn_mode = 3)  // (the backward does not look: the call runs, as in eval mode)
  BADB(ALL_BWD, "phase 3", q.phase = 3 | K)
  BADB(ALL_BWD, "nranks 0", q.nranks = 0)
  BADB(ALL_BWD, "two ranks, ALL, train", q.nranks = 2; q.bn_mode = R2L_BN_TRAIN)
  BADB(ALL_BWD, "phase A without train", q.phase = R2L_STEP_A | K)
  BADB(ALL_BWD, "phase B without gathered", q.phase = R2L_STEP_B | K; q.bn_mode = R2L_BN_TRAIN)
  BADB(ALL_BWD, "train without the saved output", q.bn_mode = R2L_BN_TRAIN; q.out = nullptr)
  BADB(ALL_BWD, "workspace one byte short", q.nws = r2l_isp_workspace_bytes(q.B, q.H, q.W) - 1)
  BADB(ALL_BWD, "epilogue with an additive gradient", q.phase = K | R2L_STEP_EPI_HFLIP; q.additive = w.gadd.p; q.gadd = w.gadd.p)
  BADB(ALL_BWD, "rot90 on 8 x 12", q.W = 12; q.phase = 1 << R2L_STEP_EPI_ROT_SHIFT)
  BADB(ALL_BWD, "B = 0", q.B = 0)
  BADB(ALL_BWD, "16-bit frames, W % 4", q.u16 = 1; q.W = 10)
  // the mask: through a planar float32 call, a 16-bit one and a channels-last one
  struct Form {
    const char* name;
    int io, layout;
  };
  for (const Form& f : {Form{"f32", R2L_IO_F32, R2L_LAYOUT_NCHW}, Form{"bf16", R2L_IO_BF16, R2L_LAYOUT_NCHW}, Form{"f32 nhwc", R2L_IO_F32, R2L_LAYOUT_NHWC}}) {
    const std::string s = std::string(f.name) + ": ";
    const bool plain = f.io == R2L_IO_F32 && f.layout == R2L_LAYOUT_NCHW;
#define FORM q.io = f.io; q.layout = f.layout
#define ENTRIES_OF_FORM (plain ? std::initializer_list<int>MASKED : (f.layout ? std::initializer_list<int>{4} : std::initializer_list<int>IO_BWD))
    BADB(ENTRIES_OF_FORM, (s + "unknown bits in the mask").c_str(), FORM; q.mask = 256 | 1)
    BADB(ENTRIES_OF_FORM, (s + "grad_raw without R2L_GRAD_RAW").c_str(), FORM; q.graw = w.graw.p; q.scr = w.scr.p; q.nscr = w.scr.n; q.mask = 127)
    BADB(ENTRIES_OF_FORM, (s + "R2L_GRAD_RAW without grad_raw").c_str(), FORM; q.mask = 255)
    BADB(ENTRIES_OF_FORM, (s + "a mask without grad_params").c_str(), FORM; q.mask = R2L_GRAD_GAMMA; q.gp = nullptr)
    // two ways: the order of the checks
    BADB(ENTRIES_OF_FORM, (s + "unknown bits + R2L_GRAD_RAW without grad_raw").c_str(), FORM; q.mask = 256 | 128)
    BADB(ENTRIES_OF_FORM, (s + "R2L_GRAD_RAW without grad_raw + no grad_params").c_str(), FORM; q.mask = 128; q.gp = nullptr)
    BADB(ENTRIES_OF_FORM, (s + "unknown bits + no KEEP_LUMA").c_str(), FORM; q.mask = 256; q.phase = 0)
    BADB(ENTRIES_OF_FORM, (s + "unknown bits + null grad_out").c_str(), FORM; q.mask = 256; q.gout = nullptr)
    BADB(ENTRIES_OF_FORM, (s + "unknown bits + workspace one byte short").c_str(), FORM; q.mask = 256; q.nws = r2l_isp_workspace_bytes(q.B, q.H, q.W) - 1)
    if (!plain) {
      BADB(ENTRIES_OF_FORM, (s + "no KEEP_LUMA").c_str(), FORM; q.phase = 0)
      BADB(ENTRIES_OF_FORM, (s + "additive layer").c_str(), FORM; q.additive = w.gadd.p; q.gadd = w.gadd.p)
      BADB(ENTRIES_OF_FORM, (s + "W % 4").c_str(), FORM; q.W = 10)
      BADB(ENTRIES_OF_FORM, (s + "epilogue").c_str(), FORM; q.phase = K | R2L_STEP_EPI_VFLIP)
      BADB(ENTRIES_OF_FORM, (s + "grad_out 4 bytes off").c_str(), FORM; q.gout = w.gout.p + 4)
      BADB(ENTRIES_OF_FORM, (s + "grad_out 8 bytes off").c_str(), FORM; q.gout = w.gout.p + 8)
      BADB(ENTRIES_OF_FORM, (s + "null grad_out").c_str(), FORM; q.gout = nullptr)
    }
    // d/d raw: every precondition, through every entry that takes grad_raw
#define ENTRIES_RAW (plain ? std::initializer_list<int>RAW_BWD : ENTRIES_OF_FORM)
#define RAWGRAD FORM; q.graw = w.graw.p; q.scr = w.scr.p; q.nscr = r2l_isp_raw_grad_scratch_bytes(q.B, q.H, q.W); q.mask = 255
    BADB(ENTRIES_RAW, (s + "grad_raw, B = 0").c_str(), RAWGRAD; q.B = 0)
    BADB(ENTRIES_RAW, (s + "grad_raw, 16-bit frames").c_str(), RAWGRAD; q.u16 = 1)
    BADB(ENTRIES_RAW, (s + "grad_raw, additive layer").c_str(), RAWGRAD; q.additive = w.gadd.p)
    BADB(ENTRIES_RAW, (s + "grad_raw, W % 4").c_str(), RAWGRAD; q.W = 10)
    setenv("R2L_FWD_TILED", "1", 1);
    BADB(ENTRIES_RAW, (s + "grad_raw, R2L_FWD_TILED").c_str(), RAWGRAD)
    unsetenv("R2L_FWD_TILED");
    BADB(ENTRIES_RAW, (s + "grad_raw, epilogue").c_str(), RAWGRAD; q.phase = K | R2L_STEP_EPI_HFLIP)
    BADB(ENTRIES_RAW, (s + "grad_raw, no KEEP_LUMA").c_str(), RAWGRAD; q.phase = 0)
    BADB(ENTRIES_RAW, (s + "grad_raw, no grad_params").c_str(), RAWGRAD; q.gp = nullptr)
    BADB(ENTRIES_RAW, (s + "grad_raw, null scratch").c_str(), RAWGRAD; q.scr = nullptr)
    BADB(ENTRIES_RAW, (s + "grad_raw, scratch one byte short").c_str(), RAWGRAD; q.nscr -= 1)
    BADB(ENTRIES_RAW, (s + "grad_raw 4 bytes off").c_str(), RAWGRAD; q.graw = w.graw.p + 1)
    BADB(ENTRIES_RAW, (s + "grad_raw, scratch 4 bytes off").c_str(), RAWGRAD; q.scr = w.scr.p + 4)
    BADB(ENTRIES_RAW, (s + "grad_raw, 16-bit frames + null scratch + phase 3").c_str(), RAWGRAD; q.u16 = 1; q.scr = nullptr; q.phase = 3 | K)
#undef RAWGRAD
#undef ENTRIES_RAW
#undef ENTRIES_OF_FORM
#undef FORM
  }
  // r2l_isp_step_bwd_raw without grad_raw: the scratch is not looked at
  BADB({1}, "no grad_raw, a scratch of 1 byte, workspace one byte short", q.scr = w.scr.p; q.nscr = 1; q.nws = r2l_isp_workspace_bytes(q.B, q.H, q.W) - 1)
  BADB(IO_BWD, "io 7", q.io = 7)
  BADB({4}, "layout 5", q.layout = 5)
  BADB({4}, "bf16, layout 5", q.io = R2L_IO_BF16; q.layout = 5)
  BADB(IO_BWD, "io 7 + unknown bits in the mask", q.io = 7; q.mask = 256)
}
static void refusals_static() {
  World& w = *world;
  static const float ms0[6] = {0.35f, 0.36f, 0.35f, 0.12f, 0.f, 0.12f};
  static const double sigma2[5] = {1.0, 1.0, 2.0, 0.3, 3.0}, median5[5] = {1.0, 1.0, 0.5, 0.3, 5.0};
  // (entries 0, 1, 2 read the frames their name says; the others R2L_FRAMES_F32 unless the case sets them)
  BADS(ALL_STA, "null raw", q.raw = nullptr)
  BADS(ALL_STA, "null out", q.out = nullptr)
  BADS(ALL_STA, "null camera", q.cam = nullptr)
  BADS(ALL_STA, "B = 0", q.B = 0)
  BADS(ALL_STA, "debayer 7", q.deb = 7)
  BADS(ALL_STA, "sharpening 7", q.sha = 7)
  BADS(ALL_STA, "denoising 9", q.den = 9)
  BADS(ALL_STA, "gamma 0", q.gamma = 0)
  BADS(ALL_STA, "debayer 7 + gamma 0", q.deb = 7; q.gamma = 0)
  BADS(ALL_STA, "Menon2007, workspace too small", q.deb = R2L_DEBAYER_MENON2007; q.nws = 64)
  BADS(ALL_STA, "Menon2007, no workspace", q.deb = R2L_DEBAYER_MENON2007; q.ws = nullptr)
  BADS(ALL_STA, "fft_denoising, workspace one byte short", q.den = R2L_DENOISE_FFT;
       q.nws = r2l_static_workspace_bytes_opts(q.entry < 3 ? STA_FRAMES[q.entry] : q.frames, q.B, q.H, q.W, q.deb, q.sha, q.den, nullptr) - 1)
  BADS(FRAMED, "std 0", q.ms = ms0)
  BADS(FRAMED, "std 0 + null out", q.ms = ms0; q.out = nullptr)
  BADS(FRAMED, "frames 9", q.frames = 9)
  BADS(FRAMED, "frames 9 + B = 0", q.frames = 9; q.B = 0)
  BADS(OPT_STA, "gaussian_sigma 2", q.opts = sigma2)
  BADS(OPT_STA, "5 x 5 median, workspace one byte short", q.opts = median5; q.den = R2L_DENOISE_MEDIAN;
       q.nws = r2l_static_workspace_bytes_opts(q.frames, q.B, q.H, q.W, q.deb, q.sha, q.den, median5) - 1)
  BADS({5}, "out_io 7", q.out_io = 7)
  BADS({5}, "out_io 7 + frames 9", q.out_io = 7; q.frames = 9)
  BADS({5}, "bf16: fft_denoising", q.out_io = R2L_IO_BF16; q.den = R2L_DENOISE_FFT)
  BADS({5}, "bf16: Menon2007", q.out_io = R2L_IO_BF16; q.deb = R2L_DEBAYER_MENON2007)
  BADS({5}, "bf16: 5 x 5 median", q.out_io = R2L_IO_BF16; q.den = R2L_DENOISE_MEDIAN; q.opts = median5)
  BADS({5}, "bf16: W % 4", q.out_io = R2L_IO_BF16; q.W = 10)
  BADS({5}, "bf16: out 4 bytes off", q.out_io = R2L_IO_BF16; q.out = w.out.p + 4)
  BADS({5}, "bf16: gaussian_sigma 2", q.out_io = R2L_IO_BF16; q.opts = sigma2)
  BADS({5}, "bf16: std 0", q.out_io = R2L_IO_BF16; q.ms = ms0)
  BADS({5}, "bf16: debayer 7", q.out_io = R2L_IO_BF16; q.deb = 7)
  BADS({5}, "bf16: gamma 0 + out 4 bytes off", q.out_io = R2L_IO_BF16; q.gamma = 0; q.out = w.out.p + 4)
}

// ---- F lines -------------------------------------------------------------------------------------------------------------------
static std::map<std::string, std::string> groups;  // group -> the digests of its first flavour
static void flavour(const std::string& group, const char* name, const std::string& digests) {
  printf("F %s | %s | %s\n", group.c_str(), name, digests.c_str());
  const auto it = groups.emplace(group, digests).first;
  if (it->second != digests) ++failures, fprintf(stderr, "%s: %s differs from the group's first flavour\n", group.c_str(), name);
}
static std::string hex(const void* p, size_t n) {
  char s[24];
  snprintf(s, sizeof s, "%016llx", fnv1a(p, n));
  return s;
}
static std::string code(int e) { return "-> " + std::to_string(e) + " [" + (e ? r2l_last_error() : "") + "]"; }
struct Slots {
  size_t stats, moments, bn, sums;
  Slots(int B, int H, int W)
      : stats(r2l_isp_step_offset(R2L_STEP_STATS, B, H, W)), moments(r2l_isp_step_offset(R2L_STEP_MOMENTS, B, H, W)),
        bn(r2l_isp_step_offset(R2L_STEP_BN, B, H, W)), sums(r2l_isp_step_offset(R2L_STEP_BN_SUMS, B, H, W)) {}
};
// one forward, whole (split = false) or as phase A + phase B: the digests of everything it leaves
static std::string fwd_run(Fwd q, bool split, size_t out_bytes, Block* keep_ws = nullptr, Block* keep_out = nullptr) {
  const Slots at(q.B, q.H, q.W);
  Block ws(q.nws), out(out_bytes);
  float rm[3] = {0.4f, 0.45f, 0.35f}, rv[3] = {0.03f, 0.05f, 0.04f};
  long long nbt = 3;
  q.ws = ws.p, q.out = out.p, q.rm = rm, q.rv = rv, q.nbt = &nbt;
  int e;
  if (!split) {
    e = call(q);
  } else {
    const int rest = q.phase & ~3;
    q.phase = rest | R2L_STEP_A;
    e = call(q);
    double gathered[7];
    memcpy(gathered, ws.p + at.stats, sizeof gathered);
    q.phase = rest | R2L_STEP_B, q.gathered = gathered;
    if (!e) e = call(q);
  }
  if (keep_ws) memcpy(keep_ws->p, ws.p, ws.n);
  if (keep_out) memcpy(keep_out->p, out.p, out.n);
  if (e) return code(e);
  return "out " + hex(out.p, out.n) + " stats " + hex(ws.p + at.stats, 56) + " moments " + hex(ws.p + at.moments, 56) + " bn " +
         hex(ws.p + at.bn, 24) + " rm " + hex(rm, sizeof rm) + " rv " + hex(rv, sizeof rv) + " nbt " + std::to_string(nbt);
}
// one backward on a copy of the workspace its forward left
static std::string bwd_run(Bwd q, bool split, const Block& ws0, size_t px) {
  const Slots at(q.B, q.H, q.W);
  Block ws(ws0.n), scr(q.graw ? r2l_isp_raw_grad_scratch_bytes(q.B, q.H, q.W) : 0);
  Buf<float> gp(R2L_P_NTRAIN), graw(q.graw ? px : 0);
  memcpy(ws.p, ws0.p, ws0.n);
  q.ws = ws.p, q.gp = gp.p;
  if (q.graw) q.graw = graw.p, q.scr = scr.p, q.nscr = scr.n;
  int e;
  if (!split) {
    e = call(q);
  } else {
    const int rest = q.phase & ~3;
    q.phase = rest | R2L_STEP_A;
    e = call(q);
    double gathered[6];
    memcpy(gathered, ws.p + at.sums, sizeof gathered);
    q.phase = rest | R2L_STEP_B, q.gathered = gathered;
    if (!e) e = call(q);
  }
  if (e) return code(e);
  return "gp " + hex(gp.p, gp.n * 4) + (q.graw ? " graw " + hex(graw.p, px * 4) : std::string());
}
static void step_flavours(int B, int H, int W) {
  const size_t px = (size_t)B * H * W, nws = r2l_isp_workspace_bytes(B, H, W);
  char shape[32];
  snprintf(shape, sizeof shape, "%dx%dx%d", B, H, W);
  Block raw32(px * 4), raw16(px * 2), cot32(3 * px * 4), cot16(3 * px * 2);
  fill_raw(lcg01, raw32.p, px, 0, 0.05f, 0.9f);
  fill_raw(lcg01, raw16.p, px, 1, 0.05f, 0.9f);
  for (size_t i = 0; i < 3 * px; ++i) {
    const float g = 2.f * lcg01() - 1.f;
    ((float*)cot32.p)[i] = g;
    ((unsigned short*)cot16.p)[i] = (unsigned short)r2l_f32_to_bf16_bits(g);
  }
  for (int u16 = 0; u16 < 2; ++u16)
    for (int bn_mode : {R2L_BN_NONE, R2L_BN_TRAIN, R2L_BN_EVAL}) {
      Fwd f;
      f.raw = u16 ? raw16.p : raw32.p, f.u16 = u16, f.table = fwd_routes::TABLE, f.bn_mode = bn_mode, f.nws = nws, f.B = B, f.H = H, f.W = W;
      const std::string what = std::string(shape) + " u" + std::to_string(u16) + " bn" + std::to_string(bn_mode);
      for (int keep = 0; keep < 2; ++keep) {
        f.phase = keep ? K : 0, f.io = R2L_IO_F32;
        for (int split = 0; split <= (bn_mode == R2L_BN_TRAIN); ++split)  // (phase A + phase B in the group of the whole call)
          for (int entry = 0; entry < 3; ++entry) {
            f.entry = entry;
            flavour("fwd " + what + " keep" + std::to_string(keep), split ? (std::string(FWD_NAMES[entry]) + " A+B").c_str() : FWD_NAMES[entry],
                    fwd_run(f, split != 0, 3 * px * 4));
          }
      }
      f.phase = K, f.io = R2L_IO_BF16;
      for (int split = 0; split <= (bn_mode == R2L_BN_TRAIN); ++split)
        for (int entry = 1; entry < 3; ++entry) {
          f.entry = entry;
          flavour("fwd bf16 " + what, split ? (std::string(FWD_NAMES[entry]) + " A+B").c_str() : FWD_NAMES[entry], fwd_run(f, split != 0, 3 * px * 2));
        }
      // the backwards, behind a forward that kept Y'
      for (int io : {R2L_IO_F32, R2L_IO_BF16}) {
        Block ws0(nws), out0(3 * px * (io ? 2 : 4));
        f.entry = 2, f.io = io, f.phase = K;
        fwd_run(f, false, out0.n, &ws0, &out0);
        Bwd b;
        b.raw = f.raw, b.u16 = u16, b.gout = io ? cot16.p : cot32.p, b.io = io, b.out = out0.p, b.bn_mode = bn_mode, b.nws = nws;
        b.B = B, b.H = H, b.W = W;
        float dummy;
        for (int split = 0; split <= (bn_mode == R2L_BN_TRAIN); ++split) {
          auto run = [&](const std::string& group, int entry, unsigned mask, bool want_raw, const char* name) {
            b.entry = entry, b.mask = mask, b.graw = want_raw ? &dummy : nullptr;
            flavour("bwd " + group + " " + what, split ? (std::string(name) + " A+B").c_str() : name, bwd_run(b, split != 0, ws0, px));
          };
          if (io == R2L_IO_F32) {
            run("params", 0, 0, false, "step_bwd");
            run("params", 1, 0, false, "step_bwd_raw(no grad_raw)");
            run("params", 2, 0, false, "step_bwd_select(0)");
            run("params", 3, 0, false, "step_bwd_io(f32, 0)");
            run("params", 4, 0, false, "step_bwd_layout(f32, nchw, 0)");
            run("params", 2, 127, false, "step_bwd_select(127)");
            run("params", 4, 127, false, "step_bwd_layout(f32, nchw, 127)");
            if (!u16) {
              run("params+raw", 1, 0, true, "step_bwd_raw");
              run("params+raw", 2, 255, true, "step_bwd_select(255)");
              run("params+raw", 3, 255, true, "step_bwd_io(f32, 255)");
              run("params+raw", 4, 255, true, "step_bwd_layout(f32, nchw, 255)");
            }
          } else {
            run("bf16 params", 3, 127, false, "step_bwd_io(bf16, 127)");
            run("bf16 params", 4, 127, false, "step_bwd_layout(bf16, nchw, 127)");
            run("bf16 params", 3, 0, false, "step_bwd_io(bf16, 0)");
            run("bf16 params", 4, 0, false, "step_bwd_layout(bf16, nchw, 0)");
            if (!u16) {
              run("bf16 params+raw", 3, 255, true, "step_bwd_io(bf16, 255)");
              run("bf16 params+raw", 4, 255, true, "step_bwd_layout(bf16, nchw, 255)");
            }
          }
        }
      }
    }
}
static void static_flavours(int B, int H, int W) {
  const size_t px = (size_t)B * H * W;
  static const double median5[5] = {1.0, 1.0, 0.5, 0.3, 5.0};
  struct Chain {
    const char* name;
    int deb, sha, den;
    const double* opts;
  };
  static const Chain CHAINS[5] = {{"default", R2L_DEBAYER_BILINEAR, R2L_SHARPEN_FILTER, R2L_DENOISE_GAUSSIAN, nullptr},
                                  {"short", R2L_DEBAYER_BILINEAR, R2L_SHARPEN_NONE, R2L_DENOISE_NONE, nullptr},
                                  {"malvar", R2L_DEBAYER_MALVAR2004, R2L_SHARPEN_UNSHARP, R2L_DENOISE_MEDIAN, nullptr},
                                  {"menon", R2L_DEBAYER_MENON2007, R2L_SHARPEN_FILTER, R2L_DENOISE_NONE, nullptr},
                                  {"median5", R2L_DEBAYER_BILINEAR, R2L_SHARPEN_FILTER, R2L_DENOISE_MEDIAN, median5}};
  Block raws[3] = {Block(px * 4), Block(px * 2), Block(px * 8)};
  for (int frames = 0; frames < 3; ++frames) fill_raw(lcg01, raws[frames].p, px, frames, 0.05f, 0.9f);
  for (const Chain& c : CHAINS) {
    char what[64];
    snprintf(what, sizeof what, "%dx%dx%d %s", B, H, W, c.name);
    // the workspace queries
    size_t nws[3];
    for (int frames = 0; frames < 3; ++frames) nws[frames] = r2l_static_workspace_bytes_opts(frames, B, H, W, c.deb, c.sha, c.den, c.opts);
    if (!c.opts) {
      const size_t plain = r2l_static_workspace_bytes(B, H, W, c.deb, c.sha, c.den), f64 = r2l_static_workspace_bytes_f64(B, H, W, c.deb, c.sha, c.den);
      printf("F workspace %s | workspace_bytes %zu _opts(0) %zu _opts(1) %zu | _f64 %zu _opts(2) %zu\n", what, plain, nws[0], nws[1], f64, nws[2]);
      if (plain != nws[0] || plain != nws[1] || f64 != nws[2]) ++failures, fprintf(stderr, "%s: the workspace queries differ\n", what);
    } else {
      printf("F workspace %s | _opts(0) %zu _opts(1) %zu _opts(2) %zu\n", what, nws[0], nws[1], nws[2]);
    }
    for (int frames = 0; frames < 3; ++frames) {
      Sta q;
      q.raw = raws[frames].p, q.frames = frames, q.B = B, q.H = H, q.W = W, q.deb = c.deb, q.sha = c.sha, q.den = c.den;
      auto run = [&](const std::string& group, int entry, const char* name) {
        Block out(3 * px * (q.out_io ? 2 : 4)), ws(nws[frames]);  // exactly what the query says
        q.entry = entry, q.out = out.p, q.ws = ws.n ? ws.p : nullptr, q.nws = ws.n;
        const int e = call(q);
        flavour("static " + group + " " + what + " frames" + std::to_string(frames), name, e ? code(e) : "out " + hex(out.p, out.n));
      };
      if (!c.opts) {
        run("plain", frames, STA_NAMES[frames]);
        run("plain", 3, "static_fwd_norm(NULL)");
        run("plain", 4, "static_fwd_opts(NULL, NULL)");
        run("plain", 5, "static_fwd_io(f32)");
      }
      q.opts = c.opts, q.ms = MEAN_STD;
      if (!c.opts) run("normalized", 3, "static_fwd_norm");
      run("normalized", 4, "static_fwd_opts");
      run("normalized", 5, "static_fwd_io(f32)");
      q.out_io = R2L_IO_BF16;  // (one line: what the 16-bit call answers for this chain)
      run("bf16", 5, "static_fwd_io(bf16)");
    }
  }
}

int run(int, char**) {
  for (const char* v : {"R2L_FWD_TILED", "R2L_BWD_PLANES", "R2L_BWD1_RECOMPUTE", "R2L_BWD1_TILED", "R2L_BWD2_TILED", "R2L_BWD_SPLIT_BLUR"}) unsetenv(v);
  setvbuf(stdout, nullptr, _IOLBF, 0);  // (what was answered before a sanitizer report stays on record)
  fwd_routes::make_params();
  World w;
  world = &w;
  {  // (so that a backward that is not refused after all reads a workspace a forward has left, BatchNorm constants included)
    Fwd q = fwd_base();
    q.bn_mode = R2L_BN_EVAL;
    CHECK(call(q));
  }
  puts("# X entry: what is wrong with the call -> code [r2l_last_error()]");
  refusals_fwd();
  refusals_bwd();
  refusals_static();
  puts("# F group | flavour | FNV-1a 64 of each result (or -> code [error]): one group, one answer");
  for (const auto& s : {std::array<int, 3>{1, 16, 16}, std::array<int, 3>{2, 16, 24}}) {
    step_flavours(s[0], s[1], s[2]);
    static_flavours(s[0], s[1], s[2]);
  }
  fflush(stdout);
  world = nullptr;
  return failures ? 1 : 0;
}
#undef ALL_FWD
#undef ALL_BWD
#undef MASKED
#undef ALL_STA
#undef FRAMED
#undef IO_FWD
#undef IO_BWD
#undef RAW_BWD
#undef OPT_STA
#undef BADF
#undef BADB
#undef BADS

}  // namespace r2l_drv::entries
