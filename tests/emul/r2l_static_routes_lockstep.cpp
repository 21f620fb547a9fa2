// r2l_static_routes_lockstep.cpp -- driver `static_routes` of r2l_lockstep_drivers.cpp (stand-alone, no Python) that writes down what
// the static chains' host route does: one text line per call of the C ABI, on the lock-step emulation's sources (r2l_lockstep.cpp,
// unchanged) under -fsanitize=address,undefined.  TEST INFRASTRUCTURE: run by tests/test_static_routes.py, which compares
// the output line by line with tests/golden/static_routes.txt (tests/README.md: how that file is regenerated).
//   Q  what the workspace and 16-bit queries answer, over the full product of frame kind x chain x median size x shape
//   R  a call that runs: return code, error text, launch record (kernel*count, sorted), FNV-1a 64 of the output bytes.  Its
//      workspace is a malloc block of EXACTLY the size the matching query returned: a write past it is an ASan report
//   S  the same call with one byte less of workspace
//   X  calls that fail before a launch
//   usage: r2l_lockstep_drivers static_routes
namespace r2l_drv::static_routes {

static Lcg lcg01{97531u};
static const double MEDIANS[3] = {3.0, 5.0, 2.5};

struct Chain {
  int deb, sh, dn;
  double med;  // 3: options_host = NULL
};
static void options(double med, double* o) {
  o[R2L_SOPT_SHARP_RADIUS] = 1.0, o[R2L_SOPT_SHARP_AMOUNT] = 1.0, o[R2L_SOPT_GAUSSIAN_SIGMA] = 0.5, o[R2L_SOPT_FFT_FRACTION] = 0.3;
  o[R2L_SOPT_MEDIAN_SIZE] = med;
}

// ---- Q lines: every reason is printed in full once ("W k: text"), lines name it by k ("-": served) ------------------------------
static std::vector<std::string> reasons;
static int reason_id(const char* why) {
  if (!why) return -1;
  for (size_t i = 0; i < reasons.size(); ++i)
    if (reasons[i] == why) return (int)i;
  reasons.push_back(why);
  printf("W %zu: %s\n", reasons.size() - 1, why);
  return (int)reasons.size() - 1;
}
static void queries(int tiled) {
  static const int widths[5] = {8, 10, 260, 1028, 2052};
  static const int bh[2][2] = {{1, 8}, {2, 12}};
  for (int frames = R2L_FRAMES_F32; frames <= R2L_FRAMES_F64; ++frames)
    for (int deb = 0; deb < 3; ++deb)
      for (int sh = 0; sh < 3; ++sh)
        for (int dn = 0; dn < 4; ++dn)
          for (double med : MEDIANS) {
            double o[R2L_SOPT_COUNT];
            options(med, o);
            std::string line;
            for (int W : widths)
              for (const auto& s : bh) {
                const int B = s[0], H = s[1];
                const int why = reason_id(r2l_static_io_supported(frames, H, W, deb, sh, dn, o));
                const size_t ws = r2l_static_workspace_bytes(B, H, W, deb, sh, dn), ws64 = r2l_static_workspace_bytes_f64(B, H, W, deb, sh, dn),
                             wso = r2l_static_workspace_bytes_opts(frames, B, H, W, deb, sh, dn, o);
                line += " " + std::to_string(ws) + "," + (ws64 == ws ? "=" : std::to_string(ws64)) + "," + (wso == ws ? "=" : std::to_string(wso)) +
                        "," + (why < 0 ? "-" : std::to_string(why));
              }
            printf("Q%d %d %d%d%d %g:%s\n", tiled, frames, deb, sh, dn, med, line.c_str());
          }
}

// ---- R / S lines ------------------------------------------------------------------------------------------------------------
static int failures = 0;
static void run(const char* tag, int frames, int io, int B, int H, int W, const Chain& c, bool norm = false) {
  const size_t px = (size_t)B * H * W;
  Block raw(px * raw_bytes(frames));
  // values below the black level, inside, and (after white balance) above the clip
  fill_raw(lcg01, raw.p, px, frames, 0.02f, 0.9f);
  double o[R2L_SOPT_COUNT];
  options(c.med, o);
  const double* opts = c.med == 3.0 ? nullptr : o;
  const size_t ws_bytes = r2l_static_workspace_bytes_opts(frames, B, H, W, c.deb, c.sh, c.dn, opts);
  for (int less = 0; less <= (ws_bytes ? 1 : 0); ++less) {
    Block ws(ws_bytes - less), out(3 * px * (io == R2L_IO_F32 ? 4 : 2));
    record_begin();
    const int e = r2l_static_fwd_io(raw.p, frames, 65535.f, out.p, io, B, H, W, CAMERA, c.deb, c.sh, c.dn, 2.2, opts, norm ? MEAN_STD : nullptr,
                                    ws.n ? ws.p : nullptr, ws.n, nullptr);
    r2l_ls_record_on = false;
    std::string rec;
    for (const auto& kv : r2l_ls_record) rec += (rec.empty() ? "" : ",") + kv.first + "*" + std::to_string(kv.second);
    printf("%c %s f%d io%d %dx%dx%d %d%d%d %g n%d ws %zu -> %d [%s] [%s] %016llx\n", less ? 'S' : 'R', tag, frames, io, B, H, W, c.deb, c.sh,
           c.dn, c.med, (int)norm, ws.n, e, e ? r2l_last_error() : "", rec.c_str(), fnv1a(out.p, out.n));
    if (less && e != -2) ++failures, fprintf(stderr, "one byte less of workspace must return -2\n");
  }
}

static void runs() {
  const Chain none{0, 0, 0, 3.0}, dflt{0, 1, 1, 3.0};
  // row-streaming short chain: both demosaics x every frame kind x every io, one strip and two (H = 8: two bands)
  for (int W : {8, 260})
    for (int deb = 0; deb < 2; ++deb)
      for (int frames = 0; frames < 3; ++frames)
        for (int io = 0; io < 3; ++io) run("stream", frames, io, 1, 8, W, Chain{deb, 0, 0, 3.0}, io == 1);
  // short tile kernel: W % 4 != 0 (float32 frames only), and 64 x 64 tiles in more than one workgroup
  for (int deb = 0; deb < 2; ++deb) run("short", R2L_FRAMES_F32, R2L_IO_F32, 1, 8, 10, Chain{deb, 0, 0, 3.0});
  run("short", R2L_FRAMES_F32, R2L_IO_F32, 2, 12, 70, none, true);
  // full-chain tile kernel: the default chain where the luma-chain kernel does not go
  run("full", R2L_FRAMES_F32, R2L_IO_F32, 1, 8, 10, dflt);
  run("full", R2L_FRAMES_F32, R2L_IO_F32, 2, 12, 70, dflt, true);
  run("full", R2L_FRAMES_F32, R2L_IO_F32, 1, 8, 2052, dflt);
  run("full", R2L_FRAMES_U16, R2L_IO_F32, 1, 8, 2052, dflt);
  // luma-chain kernel: all 16 instantiations of every frame kind at every io on one strip; on two strips a walk through them
  int n = 0;
  for (int W : {8, 260})
    for (int deb = 0; deb < 2; ++deb)
      for (int sh = 0; sh < 3; ++sh)
        for (int dn = 0; dn < 3; ++dn) {
          if (!sh && !dn) continue;
          for (int frames = 0; frames < 3; ++frames)
            for (int io = 0; io < (frames == R2L_FRAMES_F64 ? 1 : 3); ++io, ++n)
              if (W == 8 || n % 8 == 0) run("chain", frames, io, 1, 8, W, Chain{deb, sh, dn, 3.0}, n % 3 == 1);
        }
  run("chain", R2L_FRAMES_F32, R2L_IO_F32, 1, 8, 1028, dflt);                    // 8 wavefronts side by side
  run("chain", R2L_FRAMES_U16, R2L_IO_BF16, 1, 128, 8, dflt);                    // the smallest H with two bands
  run("chain", R2L_FRAMES_F32, R2L_IO_F32, 1, 130, 8, Chain{1, 2, 2, 3.0});      // ... and a ragged second band
  // luma-plane passes: the 5 x 5 median, fft_denoising, past the luma-chain kernel's widths, every frame kind
  for (int frames = 0; frames < 3; ++frames) {
    run("planes", frames, R2L_IO_F32, 1, 8, 8, Chain{0, 1, 2, 5.0});
    run("planes", frames, R2L_IO_F32, 1, 8, 260, Chain{1, 0, 2, 5.0}, true);
    run("planes", frames, R2L_IO_F32, 1, 8, 8, Chain{1, 0, 3, 3.0});
    run("planes", frames, R2L_IO_F32, 2, 12, 260, Chain{0, 2, 3, 3.0});
    run("planes", frames, R2L_IO_F32, 1, 8, 1028, Chain{0, 2, 1, 3.0});
    run("planes", frames, R2L_IO_F32, 1, 8, 2052, Chain{1, 1, 1, 3.0});
  }
  run("planes", R2L_FRAMES_F64, R2L_IO_F32, 1, 8, 2052, dflt);                   // (float32 frames: the full-chain tile kernel)
  // Menon2007: every frame kind, without a luma stage, with one, with two, with fft_denoising behind either
  for (int frames = 0; frames < 3; ++frames) {
    run("menon", frames, R2L_IO_F32, 1, 8, 8, Chain{2, 0, 0, 3.0});
    run("menon", frames, R2L_IO_F32, 1, 8, 260, Chain{2, 1, 1, 3.0}, true);
    run("menon", frames, R2L_IO_F32, 1, 8, 8, Chain{2, 2, 2, 5.0});
    run("menon", frames, R2L_IO_F32, 1, 8, 260, Chain{2, 0, 3, 3.0});
    run("menon", frames, R2L_IO_F32, 2, 12, 8, Chain{2, 1, 3, 3.0});
    run("menon", frames, R2L_IO_F32, 1, 8, 260, Chain{2, 0, 2, 3.0});
  }
  // the older entry points, once each, on 1x8x8
  {
    Block raw(64 * 8, 0x3c), out(3 * 64 * 4);
    const int e[4] = {r2l_static_fwd((const float*)raw.p, (float*)out.p, 1, 8, 8, CAMERA, 0, 1, 1, 2.2, nullptr, 0, nullptr),
                      r2l_static_fwd_u16((const unsigned short*)raw.p, 65535.f, (float*)out.p, 1, 8, 8, CAMERA, 1, 1, 1, 2.2, nullptr, 0, nullptr),
                      r2l_static_fwd_f64((const double*)raw.p, (float*)out.p, 1, 8, 8, CAMERA, 0, 0, 0, 2.2, nullptr, 0, nullptr),
                      r2l_static_fwd_norm(raw.p, R2L_FRAMES_U16, 65535.f, (float*)out.p, 1, 8, 8, CAMERA, 0, 0, 2, 2.2, MEAN_STD, nullptr, 0, nullptr)};
    printf("R older entry points -> %d %d %d %d %016llx\n", e[0], e[1], e[2], e[3], fnv1a(out.p, out.n));
  }
  // the overrides of the diagnostic build
  setenv("R2L_CHAIN_BAND", "2", 1);
  run("chain_band2", R2L_FRAMES_F32, R2L_IO_F16, 1, 8, 8, dflt);
  unsetenv("R2L_CHAIN_BAND");
  setenv("R2L_STREAM_BANDS", "4", 1);
  run("stream_bands4", R2L_FRAMES_F32, R2L_IO_F32, 1, 8, 8, none);
  run("stream_bands4", R2L_FRAMES_F32, R2L_IO_F32, 1, 8, 8, Chain{0, 1, 2, 5.0});
  unsetenv("R2L_STREAM_BANDS");
  setenv("R2L_GRID_STATIC", "1", 1);
  setenv("R2L_GRID_STATIC_FULL", "1", 1);
  run("grid1", R2L_FRAMES_F32, R2L_IO_F32, 2, 12, 70, none);
  run("grid1", R2L_FRAMES_F32, R2L_IO_F32, 2, 12, 70, dflt);
  unsetenv("R2L_GRID_STATIC");
  unsetenv("R2L_GRID_STATIC_FULL");
  setenv("R2L_STATIC_TILED", "1", 1);
  for (int frames = 0; frames < 3; ++frames) {
    run("tiled", frames, R2L_IO_F32, 1, 8, 8, none);                // tile kernel; float64 frames: the streaming kernel
    run("tiled", frames, R2L_IO_F32, 1, 8, 8, dflt);                // tile kernel; float64 frames: plane passes
    run("tiled", frames, R2L_IO_F32, 1, 8, 260, Chain{1, 1, 2, 3.0});  // plane passes
  }
  run("tiled", R2L_FRAMES_F64, R2L_IO_BF16, 1, 8, 8, none);
  unsetenv("R2L_STATIC_TILED");
}

// ---- X lines ----------------------------------------------------------------------------------------------------------------
struct Call {
  int frames = R2L_FRAMES_F32, io = R2L_IO_F32, B = 1, H = 8, W = 8;
  Chain c{0, 0, 0, 3.0};
  double gamma = 2.2;
  bool null_raw = false, null_out = false, null_camera = false, misaligned = false, workspace = true;
  const double* opts = nullptr;
  const float* mean_std = nullptr;
};
static void refused(const char* tag, const Call& q) {
  const size_t px = (size_t)(q.B > 0 ? q.B : 1) * q.H * q.W;
  Block raw(px * 8, 0x3c), out(3 * px * 4 + 8), ws(q.workspace ? 64 * px * 8 + 4096 : 0);
  const unsigned long long before = fnv1a(out.p, out.n);
  const int e = r2l_static_fwd_io(q.null_raw ? nullptr : raw.p, q.frames, 65535.f, q.null_out ? nullptr : out.p + (q.misaligned ? 2 : 0), q.io,
                                  q.B, q.H, q.W, q.null_camera ? nullptr : CAMERA, q.c.deb, q.c.sh, q.c.dn, q.gamma, q.opts, q.mean_std,
                                  ws.n ? ws.p : nullptr, ws.n, nullptr);
  printf("X %s -> %d [%s]\n", tag, e, e ? r2l_last_error() : "");
  if (!e || fnv1a(out.p, out.n) != before) ++failures, fprintf(stderr, "%s: must fail, and write nothing\n", tag);
}
static void refusals() {
  Call d;
  { Call q = d; q.null_out = true; refused("null out", q); }
  { Call q = d; q.null_camera = true; refused("null camera_host", q); }
  { Call q = d; q.null_raw = true; refused("null raw", q); }
  for (int code : {-1, 3, 7}) {
    { Call q = d; q.c.deb = code; refused("unknown debayer", q); }
    { Call q = d; q.c.sh = code; refused("unknown sharpening", q); }
    { Call q = d; q.c.dn = code == 3 ? 4 : code; refused("unknown denoising", q); }
    { Call q = d; q.frames = code; refused("unknown frames", q); }
    { Call q = d; q.io = code; refused("out_io outside R2L_IO_*", q); }
  }
  for (double g : {0.0, -1.0, (double)NAN}) { Call q = d; q.gamma = g; refused("gamma <= 0", q); }
  for (int k = 0; k < 3; ++k) {
    float ms[6] = {0.35f, 0.36f, 0.35f, 0.12f, 0.11f, 0.12f};
    ms[3 + k] = 0.f;
    Call q = d; q.mean_std = ms; refused("zero std", q);
  }
  { Call q = d; q.B = 0; refused("B = 0", q); }
  { Call q = d; q.H = 6; q.W = 2; refused("W = 2", q); }
  { Call q = d; q.H = 7; refused("odd H", q); }
  { Call q = d; q.frames = R2L_FRAMES_U16; q.W = 10; refused("16-bit frames, W % 4", q); }
  { Call q = d; q.frames = R2L_FRAMES_F64; q.W = 10; refused("float64 frames, W % 4", q); }
  // every out-of-range option, with the stage that reads it: bilinear and Menon2007, float32 and bfloat16 output
  struct { int slot; double v; int sh, dn; } bad[] = {
      {R2L_SOPT_GAUSSIAN_SIGMA, 0.0, 1, 1},  {R2L_SOPT_GAUSSIAN_SIGMA, 0.625, 1, 1}, {R2L_SOPT_GAUSSIAN_SIGMA, -1.0, 0, 1},
      {R2L_SOPT_GAUSSIAN_SIGMA, NAN, 1, 1},  {R2L_SOPT_SHARP_RADIUS, 0.0, 2, 1},     {R2L_SOPT_SHARP_RADIUS, 1.125, 2, 0},
      {R2L_SOPT_SHARP_RADIUS, NAN, 2, 2},    {R2L_SOPT_SHARP_AMOUNT, NAN, 2, 1},     {R2L_SOPT_MEDIAN_SIZE, 4.0, 1, 2},
      {R2L_SOPT_MEDIAN_SIZE, 7.0, 1, 2},     {R2L_SOPT_MEDIAN_SIZE, 2.5, 1, 2},      {R2L_SOPT_MEDIAN_SIZE, 1.0, 0, 2},
      {R2L_SOPT_MEDIAN_SIZE, -3.0, 0, 2},    {R2L_SOPT_FFT_FRACTION, -0.01, 0, 3},   {R2L_SOPT_FFT_FRACTION, 0.51, 1, 3},
      {R2L_SOPT_FFT_FRACTION, NAN, 0, 3}};
  for (const auto& b : bad)
    for (int deb = 0; deb < 3; deb += 2)
      for (int io = 0; io < 2; ++io) {
        double o[R2L_SOPT_COUNT];
        options(3.0, o);
        o[b.slot] = b.v;
        char tag[96];
        snprintf(tag, sizeof tag, "option %d = %g, chain %d%d%d, io %d", b.slot, b.v, deb, b.sh, b.dn, io);
        Call q = d; q.c = Chain{deb, b.sh, b.dn, 3.0}; q.opts = o; q.io = io; refused(tag, q);
      }
  // plane passes need W % 4 == 0; Menon2007 too
  double med5[R2L_SOPT_COUNT];
  options(5.0, med5);
  { Call q = d; q.W = 10; q.c = Chain{1, 1, 1, 3.0}; refused("planes, W % 4", q); }
  { Call q = d; q.W = 10; q.c = Chain{0, 1, 2, 5.0}; q.opts = med5; refused("planes (5x5 median), W % 4", q); }
  { Call q = d; q.W = 10; q.c = Chain{0, 0, 3, 3.0}; refused("planes (fft), W % 4", q); }
  { Call q = d; q.W = 10; q.c = Chain{2, 0, 0, 3.0}; refused("menon2007, W % 4", q); }
  { Call q = d; q.W = 6; q.H = 4; q.c = Chain{2, 1, 1, 3.0}; refused("menon2007, 4 x 6", q); }
  { Call q = d; q.W = 2; q.H = 2; q.c = Chain{2, 0, 0, 3.0}; refused("menon2007 below 4 x 4", q); }
  // no workspace at all where one is needed
  { Call q = d; q.workspace = false; q.c = Chain{2, 0, 0, 3.0}; refused("menon2007, no workspace", q); }
  { Call q = d; q.workspace = false; q.c = Chain{0, 0, 3, 3.0}; refused("planes (fft), no workspace", q); }
  { Call q = d; q.workspace = false; q.c = Chain{0, 1, 2, 5.0}; q.opts = med5; refused("planes (5x5 median), no workspace", q); }
  // 16-bit output: misaligned, and each reason r2l_static_io_supported knows
  { Call q = d; q.io = R2L_IO_BF16; q.misaligned = true; refused("misaligned 16-bit output", q); }
  { Call q = d; q.io = R2L_IO_F16; q.c = Chain{0, 1, 1, 3.0}; q.misaligned = true; refused("misaligned 16-bit output", q); }
  for (int io = R2L_IO_BF16; io <= R2L_IO_F16; ++io) {
    Call h = d; h.io = io;
    { Call q = h; q.frames = 3; refused("io: frames", q); }
    { Call q = h; q.H = 7; refused("io: odd H", q); }
    { Call q = h; q.H = 2; refused("io: H = 2", q); }
    { Call q = h; q.c.deb = 2; refused("io: menon2007", q); }
    { Call q = h; q.c.deb = 3; refused("io: unknown debayer", q); }
    { Call q = h; q.c.sh = 3; refused("io: unknown sharpening", q); }
    { Call q = h; q.c.dn = 4; refused("io: unknown denoising", q); }
    { Call q = h; q.c.dn = 3; refused("io: fft_denoising", q); }
    { Call q = h; q.c = Chain{0, 1, 2, 5.0}; q.opts = med5; refused("io: 5x5 median", q); }
    { Call q = h; q.W = 10; refused("io: W % 4", q); }
    { Call q = h; q.W = 2052; refused("io: W > 2048", q); }
    { Call q = h; q.W = 2052; q.c = Chain{1, 1, 1, 3.0}; refused("io: W > 2048, luma chain", q); }
    { Call q = h; q.W = 1028; q.c = Chain{0, 2, 0, 3.0}; refused("io: unsharp_masking, W > 1024", q); }
    { Call q = h; q.frames = R2L_FRAMES_F64; q.c = Chain{0, 1, 1, 3.0}; refused("io: float64 frames on a luma chain", q); }
    setenv("R2L_STATIC_TILED", "1", 1);
    { Call q = h; refused("io: R2L_STATIC_TILED, short chain", q); }
    { Call q = h; q.c = Chain{0, 1, 1, 3.0}; refused("io: R2L_STATIC_TILED, luma chain", q); }
    { Call q = h; q.c = Chain{1, 2, 2, 3.0}; q.frames = R2L_FRAMES_U16; refused("io: R2L_STATIC_TILED, luma chain", q); }
    unsetenv("R2L_STATIC_TILED");
  }
}

int run(int, char**) {
  for (const char* v : {"R2L_STATIC_TILED", "R2L_CHAIN_BAND", "R2L_STREAM_BANDS", "R2L_GRID_STATIC", "R2L_GRID_STATIC_FULL"}) unsetenv(v);
  puts("# Q<R2L_STATIC_TILED> frames debayer|sharpening|denoising median: for W in 8 10 260 1028 2052, for BxH in 1x8 2x12:");
  puts("#   r2l_static_workspace_bytes,_f64,_opts (=: as the first),r2l_static_io_supported (k: the text of line 'W k', -: served)");
  queries(0);
  setenv("R2L_STATIC_TILED", "1", 1);
  queries(1);
  unsetenv("R2L_STATIC_TILED");
  puts("# R|S tag frames io BxHxW debayer|sharpening|denoising median normalize workspace -> code [error] [launches] fnv1a64(out)");
  runs();
  puts("# X what -> code [error]");
  refusals();
  fflush(stdout);
  return failures ? 1 : 0;
}

}  // namespace r2l_drv::static_routes
