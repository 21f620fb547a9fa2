// r2l_fwd_routes_lockstep.cpp -- driver `fwd_routes` of r2l_lockstep_drivers.cpp (stand-alone, no Python) that writes down what the
// host route of the training step's forward (and of the backward's recomputing BatchNorm-sums pass) does: one text line per call
// of the C ABI, on the lock-step emulation's sources (r2l_lockstep.cpp, unchanged) under -fsanitize=address,undefined.
// TEST INFRASTRUCTURE: run by tests/test_fwd_routes.py, which compares the output line by line with
// tests/golden/fwd_routes.txt (tests/README.md: how that file is regenerated).  Every launch is seen through the observer of
// r2l_ls::launch, which decodes the kernel's argument block:
//   P  plans, dry (the observer lets no workgroup run; every pointer is a made-up address that nothing dereferences): the full
//      product of entry x frame type x BatchNorm mode / phase x KEEP_LUMA x epilogue x io / layout x additive over small shapes
//      and the shapes training runs, then again under every override of diagnostic builds.  "P <override> <key>: a/g ...": one
//      answer per combination of the key's last dimensions; its kernels and arguments per shape are line "VA a", their launch
//      shapes line "VG g".  Under an override "=" is the answer without it, and only lines with another one are printed
//   R  a call that runs: return code, error text, launch record (kernel*count, sorted), the launches, FNV-1a 64 of each result.
//      Its workspace is a malloc block of EXACTLY r2l_isp_workspace_bytes, `out` EXACTLY 3 B H W elements
//   S  the same call with one byte less of workspace
//   X  calls that fail before a launch
//   usage: r2l_lockstep_drivers fwd_routes
namespace r2l_drv::fwd_routes {

static Lcg lcg01{24680u};
static int failures = 0;

// ---- the packed parameters: the drone camera, a bilinear debayer, the reference's sharpening and blur kernels ----------------
static float PARAMS[R2L_P_COUNT];
static const float* TABLE[9];
static void make_params() {
  float* P = PARAMS;
  for (int i = 0; i < 4; ++i) P[R2L_P_BLACK_LEVEL + i] = 0.0625f;
  const float wb[3] = {2.86653646f, 1.f, 1.73079425f};
  const float ccm[9] = {1.50768983f, -0.33571374f, -0.17197604f, -0.23048614f, 1.70698738f, -0.47650126f, -0.03119153f, -0.32803956f, 1.35923111f};
  memcpy(P + R2L_P_WHITE_BALANCE, wb, sizeof wb);
  memcpy(P + R2L_P_CCM, ccm, sizeof ccm);
  P[R2L_P_GAMMA] = 2.2f;
  const float rb[9] = {.25f, .5f, .25f, .5f, 1.f, .5f, .25f, .5f, .25f}, g[9] = {0.f, .25f, 0.f, .25f, 1.f, .25f, 0.f, .25f, 0.f};
  for (int k = 0; k < 3; ++k) memcpy(P + R2L_P_DEBAYER + (k * 3 + k) * 9, k == 1 ? g : rb, sizeof rb);
  const float sh[9] = {0.f, -1.f, 0.f, -1.f, 5.f, -1.f, 0.f, -1.f, 0.f}, b1[5] = {1.f, 4.f, 6.f, 4.f, 1.f};
  memcpy(P + R2L_P_SHARPEN, sh, sizeof sh);
  for (int i = 0; i < 25; ++i) P[R2L_P_BLUR + i] = b1[i / 5] * b1[i % 5] / 256.f;
  const float m1[9] = {0.299f, 0.587f, 0.114f, -0.14714119f, -0.28886916f, 0.43601035f, 0.61497538f, -0.51496512f, -0.10001026f};
  const float m2[9] = {1.f, 0.f, 1.13988303f, 1.f, -0.394642334f, -0.58062185f, 1.f, 2.03206185f, 0.f};
  memcpy(P + R2L_P_M_RGB2YUV, m1, sizeof m1);
  memcpy(P + R2L_P_M_YUV2RGB, m2, sizeof m2);
  param_table(P, TABLE);
}

// ---- the observer: every launch as text -------------------------------------------------------------------------------------
struct Range {
  const char* base;
  size_t n;
  const char* name;
};
static std::vector<Range> ranges;   // what the pointers of the call under observation are called
static size_t luma_offset = 0;      // r2l_isp_step_offset(R2L_STEP_LUMA) of that call: printed as ws+Y
static bool dry = false;
static std::vector<std::pair<std::string, std::string>> launches;  // (who and on what, shape) of every launch of the call

static std::string role(const void* p) {
  if (!p) return "-";
  for (const Range& r : ranges)
    if ((const char*)p >= r.base && (const char*)p < r.base + r.n) {
      const size_t off = (size_t)((const char*)p - r.base);
      if (!strcmp(r.name, "ws")) return off == luma_offset ? std::string("ws+Y") : "ws+" + std::to_string(off);
      return off ? std::string(r.name) + "+" + std::to_string(off) : std::string(r.name);
    }
  return "?";
}
static std::string raw_role(const R2LRaw& r) {
  return r.u16 ? "u16:" + role(r.u16) : (r.f64 ? "f64:" + role(r.f64) : "f32:" + role(r.f32));
}
static std::string tree_role(const R2LTree& t) {
  return "tree(" + role(t.partial) + "," + role(t.partial2) + "," + role(t.gpartial) + "," + role(t.counters) + "," + std::to_string(t.split) +
         "," + std::to_string(t.nblk1) + ")";
}
static std::string fin_role(const R2LBnFinalizeArgs& f) {  // (without fin.bn the callers leave the rest unset)
  if (!f.bn) return "fin-";
  return "fin(" + role(f.tot) + "," + std::to_string(f.nranks) + "," + role(f.bn) + "," + role(f.moments) + "," + role(f.running_mean) + "," +
         role(f.running_var) + "," + role(f.num_batches_tracked) + ")";
}
static std::string epi(const R2LEpi& e) {
  return " e" + std::to_string(e.on) + "," + std::to_string(e.s0) + "," + std::to_string(e.sr) + "," + std::to_string(e.sc);
}
static int call_B, call_H, call_W;
static std::string stream_roles(const R2LFwdStreamArgs& a) {
  std::string s = " " + raw_role(a.raw) + " " + role(a.F) + " " + role(a.bn) + " " + role(a.out) + " " + role(a.yp_out) + " " + role(a.yp_in) +
                  " " + role(a.stat_partial) + " " + tree_role(a.tree) + " " + role(a.stats_out) + " " + fin_role(a.fin);
  if (a.B != call_B || a.H != call_H || a.W != call_W) s += " BHW!";
  return s;
}
static bool starts(const char* s, const char* prefix) { return !strncmp(s, prefix, strlen(prefix)); }
static bool observe(const char* name, int grid, int nt, size_t lds_floats, const void* kernarg) {
  const char* n = starts(name, "r2l_launch_") ? name + 11 : name;
  std::string who = n, shape = "g" + std::to_string(grid) + " t" + std::to_string(nt) + " l" + std::to_string(lds_floats);
  if (starts(n, "fwd_stream")) {  // (the wavefronts per row go with the shape: the rest of the name does not depend on it)
    const size_t at = who.find("_w");
    shape = who.substr(at + 1, 2) + " " + shape;
    who.erase(at, 3);
  }
  if (starts(n, "fwd_stream") || starts(n, "fwd_apply") || starts(n, "fwd_stats") || starts(n, "fwd_luma")) {
    const R2LFwdStreamArgs& a = *(const R2LFwdStreamArgs*)kernarg;
    who += stream_roles(a);
    shape += " b" + std::to_string(a.band_h) + "x" + std::to_string(a.nband) + "=" + std::to_string(a.nitems) + epi(a.ep);
  } else if (starts(n, "bnr_planes")) {
    const R2LBnrArgs& a = *(const R2LBnrArgs*)kernarg;
    who += stream_roles(a.s) + " " + role(a.gout) + " " + role(a.sums) + " " + role(a.totals) + " " + role(a.bn_bwd);
    shape += " b" + std::to_string(a.s.band_h) + "x" + std::to_string(a.s.nband) + "=" + std::to_string(a.s.nitems) + epi(a.s.ep);
  } else if (!strcmp(n, "fwd") || starts(n, "fwd_u16") || starts(n, "fwd_ragged") || starts(n, "fwd_add_exact")) {
    const R2LFwdArgs& a = *(const R2LFwdArgs*)kernarg;
    who += " " + raw_role(a.raw) + " " + role(a.additive) + " " + role(a.F) + " " + role(a.bn) + " " + role(a.out) + " " + role(a.stat_partial) +
           " " + role(a.debug) + " " + tree_role(a.tree) + " " + role(a.stats_out) + " " + fin_role(a.fin);
    if (a.B != call_B || a.H != call_H || a.W != call_W) who += " BHW!";
    shape += " b-" + epi(a.ep);
  }
  launches.emplace_back(who, shape);
  return !dry;
}
static void begin_call(int B, int H, int W) {
  call_B = B, call_H = H, call_W = W;
  luma_offset = r2l_isp_step_offset(R2L_STEP_LUMA, B, H, W);
  launches.clear();
  record_begin();
}
static std::string end_call_record() {
  r2l_ls_record_on = false;
  std::string rec;
  for (const auto& kv : r2l_ls_record)  // ("r2l_launch_<name>_kernel": <name>)
    rec += (rec.empty() ? "" : ",") + kv.first.substr(11, kv.first.size() - 18) + "*" + std::to_string(kv.second);
  return rec;
}

// ---- P lines ----------------------------------------------------------------------------------------------------------------
typedef std::map<std::string, int> Table;  // every distinct text is printed once ("<kind> k: text"), lines name it by k
static int intern(Table& table, const char* kind, const std::string& s) {
  const auto it = table.find(s);
  if (it != table.end()) return it->second;
  const int k = (int)table.size();
  table.emplace(s, k);
  printf("%s %d: %s\n", kind, k, s.c_str());
  return k;
}
static Table whos, shapes, errors, vectors;
// made-up addresses of a dry call (2^44 apart: every tensor of every shape fits)
static char* fake(int k) { return (char*)(((uintptr_t)(k + 1)) << 44); }
enum { FK_RAW, FK_OUT, FK_WS, FK_STATS, FK_BN, FK_ADD, FK_RM, FK_RV, FK_NBT, FK_GOUT, FK_MOM, FK_GP, FK_GATHER, FK_COUNT };
static const char* const FK_NAMES[FK_COUNT] = {"raw", "out", "ws", "stats", "bn", "add", "rm", "rv", "nbt", "gout", "mom", "gp", "gather"};
static const float* FAKE_TABLE[9];
static void dry_ranges() {
  ranges.clear();
  for (int k = 0; k < FK_COUNT; ++k) ranges.push_back(Range{fake(k), (size_t)1 << 43, FK_NAMES[k]});
  ranges.push_back(Range{fake(FK_COUNT), (size_t)1 << 43, "params"});
  for (int i = 0; i < 9; ++i) FAKE_TABLE[i] = (const float*)(fake(FK_COUNT) + 1024 * i);
}
struct Answer {
  std::string who, shape;  // "+"-joined A resp. G numbers of the call's launches; a refusal: its code and E number, twice
};
static Answer answer(int e) {  // of the call that has just returned
  end_call_record();
  if (e) {
    const std::string s = "e" + std::to_string(e) + "." + std::to_string(intern(errors, "E", r2l_last_error()));
    return Answer{s, s};
  }
  Answer a;
  for (const auto& l : launches) {
    a.who += (a.who.empty() ? "" : "+") + std::to_string(intern(whos, "A", l.first));
    a.shape += (a.shape.empty() ? "" : "+") + std::to_string(intern(shapes, "G", l.second));
  }
  return a;
}
struct Shape {
  int B, H, W;
};
static const Shape FWD_SHAPES[] = {{1, 8, 8},       {1, 8, 10},      {2, 14, 260},     {1, 8, 516},     {1, 8, 1028},     {1, 64, 64},    {1, 256, 256},
                                   {64, 512, 512},  {64, 256, 256},  {128, 256, 256},  {8, 1024, 1024}, {2, 2048, 2048},  {1, 1024, 2052}};
// (the recomputing BatchNorm sums: both sides of their 6 Mi px threshold and of the plane passes' 4 Mi px one)
static const Shape BWD_SHAPES[] = {{1, 8, 8},       {1, 8, 10},      {2, 14, 260},     {1, 256, 256},    {63, 256, 256},  {64, 256, 256}, {95, 256, 256},
                                   {96, 256, 256},  {64, 512, 512},  {128, 256, 256},  {2, 2048, 2048},  {1, 1024, 2052}};
static const int EPIS[3] = {0, R2L_STEP_EPI_HFLIP, R2L_STEP_EPI_VFLIP | (1 << R2L_STEP_EPI_ROT_SHIFT)};
static std::string run_lengths(const std::vector<std::string>& v) {  // "x*n"
  std::string out;
  for (size_t i = 0; i < v.size();) {
    size_t j = i;
    while (j < v.size() && v[j] == v[i]) ++j;
    out += (out.empty() ? "" : " ") + v[i] + (j - i > 1 ? "*" + std::to_string(j - i) : "");
    i = j;
  }
  return out;
}
static Table who_vectors, shape_vectors;
static std::string p_token(const std::vector<Answer>& per_shape) {
  std::vector<std::string> w, g;
  for (const Answer& a : per_shape) w.push_back(a.who), g.push_back(a.shape);
  return std::to_string(intern(who_vectors, "VA", run_lengths(w))) + "/" + std::to_string(intern(shape_vectors, "VG", run_lengths(g)));
}
static std::map<std::string, std::vector<std::string>> baseline;  // key -> tokens of the pass without an override
static long p_same = 0, p_differ = 0;
static void p_line(const char* override_name, const std::string& key, std::vector<std::string> tokens) {
  if (!override_name) {
    baseline[key] = tokens;
  } else {
    const std::vector<std::string>& base = baseline.at(key);
    long differ = 0;
    for (size_t i = 0; i < tokens.size(); ++i) {
      const size_t cut = tokens[i].find('/'), bcut = base[i].find('/');
      if (tokens[i] == base[i]) tokens[i] = "=";
      else if (++differ && tokens[i].substr(0, cut) == base[i].substr(0, bcut)) tokens[i] = "=" + tokens[i].substr(cut);
      else if (tokens[i].substr(cut) == base[i].substr(bcut)) tokens[i] = tokens[i].substr(0, cut + 1) + "=";
    }
    p_differ += differ, p_same += (long)tokens.size() - differ;
    if (!differ) return;
  }
  printf("P %s %s: %s\n", override_name ? override_name + 4 : "-", key.c_str(), run_lengths(tokens).c_str());
}
static void plans(const char* ov) {
  dry = true;
  dry_ranges();
  char key[96];
  void* const ws = fake(FK_WS);
  // r2l_isp_fwd[_u16]: with out, with stats, with both, with both and R2L_F_STATS_ONLY
  for (int mode = 0; mode < 4; ++mode)
    for (int u16 = 0; u16 < 2; ++u16) {
      std::vector<std::string> tokens;
      for (int bn = 0; bn < 2; ++bn)
        for (int keep = 0; keep < 2; ++keep)
          for (int add = 0; add < 2; ++add) {
            std::vector<Answer> per;
            for (const Shape& s : FWD_SHAPES) {
              begin_call(s.B, s.H, s.W);
              float* out = mode == 1 ? nullptr : (float*)fake(FK_OUT);
              double* stats = mode == 0 ? nullptr : (double*)fake(FK_STATS);
              const float* bnp = bn ? (const float*)fake(FK_BN) : nullptr;
              const float* addp = add ? (const float*)fake(FK_ADD) : nullptr;
              const int flags = (mode == 3 ? R2L_F_STATS_ONLY : 0) | (keep ? R2L_F_KEEP_LUMA : 0);
              const size_t n = r2l_isp_workspace_bytes(s.B, s.H, s.W);
              const int e = u16 ? r2l_isp_fwd_u16((const unsigned short*)fake(FK_RAW), 65535.f, (const float*)fake(FK_COUNT), addp, bnp, out, stats,
                                                  ws, n, s.B, s.H, s.W, flags, nullptr)
                                : r2l_isp_fwd((const float*)fake(FK_RAW), (const float*)fake(FK_COUNT), addp, bnp, out, stats, ws, n, s.B, s.H, s.W,
                                              flags, nullptr);
              per.push_back(answer(e));
            }
            tokens.push_back(p_token(per));
          }
      snprintf(key, sizeof key, "fwd m%d u%d", mode, u16);
      p_line(ov, key, tokens);
    }
  // r2l_isp_fwd_stats_bn[_u16]
  for (int u16 = 0; u16 < 2; ++u16) {
    std::vector<std::string> tokens;
    for (int add = 0; add < 2; ++add) {
      std::vector<Answer> per;
      for (const Shape& s : FWD_SHAPES) {
        begin_call(s.B, s.H, s.W);
        const float* addp = add ? (const float*)fake(FK_ADD) : nullptr;
        const size_t n = r2l_isp_workspace_bytes(s.B, s.H, s.W);
        const int e = u16 ? r2l_isp_fwd_stats_bn_u16((const unsigned short*)fake(FK_RAW), 65535.f, (const float*)fake(FK_COUNT), addp,
                                                     (double*)fake(FK_STATS), (float*)fake(FK_BN), (double*)fake(FK_MOM), (float*)fake(FK_RM),
                                                     (float*)fake(FK_RV), (long long*)fake(FK_NBT), 1e-5, 0.1, ws, n, s.B, s.H, s.W, nullptr)
                          : r2l_isp_fwd_stats_bn((const float*)fake(FK_RAW), (const float*)fake(FK_COUNT), addp, (double*)fake(FK_STATS),
                                                 (float*)fake(FK_BN), (double*)fake(FK_MOM), (float*)fake(FK_RM), (float*)fake(FK_RV),
                                                 (long long*)fake(FK_NBT), 1e-5, 0.1, ws, n, s.B, s.H, s.W, nullptr);
        per.push_back(answer(e));
      }
      tokens.push_back(p_token(per));
    }
    snprintf(key, sizeof key, "stats_bn u%d", u16);
    p_line(ov, key, tokens);
  }
  // r2l_isp_step_fwd (entry 0), _io (1: io = float32, bfloat16, float16), _layout (2: planar float32, channels-last x 3)
  static const int ENTRIES[8][3] = {{0, 0, 0}, {1, 0, 0}, {1, 1, 0}, {1, 2, 0}, {2, 0, 0}, {2, 0, 1}, {2, 1, 1}, {2, 2, 1}};
  static const int BNPHASE[5][2] = {{R2L_BN_NONE, R2L_STEP_ALL}, {R2L_BN_EVAL, R2L_STEP_ALL}, {R2L_BN_TRAIN, R2L_STEP_ALL},
                                    {R2L_BN_TRAIN, R2L_STEP_A}, {R2L_BN_TRAIN, R2L_STEP_B}};
  for (const auto& en : ENTRIES)
    for (int u16 = 0; u16 < 2; ++u16)
      for (const auto& bp : BNPHASE) {
        std::vector<std::string> tokens;
        for (int keep = 0; keep < 2; ++keep)
          for (int ep = 0; ep < 3; ++ep)
            for (int add = 0; add < 2; ++add) {
              std::vector<Answer> per;
              for (const Shape& s : FWD_SHAPES) {
                begin_call(s.B, s.H, s.W);
                const float* addp = add ? (const float*)fake(FK_ADD) : nullptr;
                const int phase = bp[1] | (keep ? R2L_STEP_KEEP_LUMA : 0) | EPIS[ep];
                const size_t n = r2l_isp_workspace_bytes(s.B, s.H, s.W);
                const double* gathered = bp[1] == R2L_STEP_B ? (const double*)fake(FK_GATHER) : nullptr;
                float *rm = (float*)fake(FK_RM), *rv = (float*)fake(FK_RV);
                long long* nbt = (long long*)fake(FK_NBT);
                int e;
                if (en[0] == 0)
                  e = r2l_isp_step_fwd(fake(FK_RAW), u16, 65535.f, FAKE_TABLE, addp, bp[0], rm, rv, nbt, 1e-5, 0.1, (float*)fake(FK_OUT), ws, n,
                                       s.B, s.H, s.W, 1, phase, gathered, nullptr);
                else if (en[0] == 1)
                  e = r2l_isp_step_fwd_io(fake(FK_RAW), u16, 65535.f, FAKE_TABLE, addp, bp[0], rm, rv, nbt, 1e-5, 0.1, fake(FK_OUT), en[1], ws, n,
                                          s.B, s.H, s.W, 1, phase, gathered, nullptr);
                else
                  e = r2l_isp_step_fwd_layout(fake(FK_RAW), u16, 65535.f, FAKE_TABLE, addp, bp[0], rm, rv, nbt, 1e-5, 0.1, fake(FK_OUT), en[1],
                                              en[2], ws, n, s.B, s.H, s.W, 1, phase, gathered, nullptr);
                per.push_back(answer(e));
              }
              tokens.push_back(p_token(per));
            }
        snprintf(key, sizeof key, "step_fwd n%d io%d l%d u%d bn%d p%d", en[0], en[1], en[2], u16, bp[0], bp[1]);
        p_line(ov, key, tokens);
      }
  // r2l_isp_step_bwd (entry 0), _io (1), _layout (2): phase A (the BatchNorm sums alone) and ALL (then the gradient kernels)
  static const int BENTRIES[6][3] = {{0, 0, 0}, {1, 1, 0}, {1, 2, 0}, {2, 0, 1}, {2, 1, 1}, {2, 2, 1}};
  static const int BBNPHASE[3][2] = {{R2L_BN_TRAIN, R2L_STEP_A}, {R2L_BN_TRAIN, R2L_STEP_ALL}, {R2L_BN_NONE, R2L_STEP_ALL}};
  for (const auto& en : BENTRIES)
    for (int u16 = 0; u16 < 2; ++u16)
      for (const auto& bp : BBNPHASE) {
        std::vector<std::string> tokens;
        for (int keep = 0; keep < 2; ++keep)
          for (int ep = 0; ep < 3; ++ep)
            for (int add = 0; add < 2; ++add) {
              std::vector<Answer> per;
              for (const Shape& s : BWD_SHAPES) {
                begin_call(s.B, s.H, s.W);
                const float* addp = add ? (const float*)fake(FK_ADD) : nullptr;
                const int phase = bp[1] | (keep ? R2L_STEP_KEEP_LUMA : 0) | EPIS[ep];
                const size_t n = r2l_isp_workspace_bytes(s.B, s.H, s.W);
                float* gp = bp[1] == R2L_STEP_ALL ? (float*)fake(FK_GP) : nullptr;
                int e;
                if (en[0] == 0)
                  e = r2l_isp_step_bwd(fake(FK_RAW), u16, 65535.f, addp, (const float*)fake(FK_GOUT), (const float*)fake(FK_OUT), gp, nullptr, bp[0],
                                       ws, n, s.B, s.H, s.W, 1, phase, nullptr, nullptr);
                else if (en[0] == 1)
                  e = r2l_isp_step_bwd_io(fake(FK_RAW), u16, 65535.f, addp, fake(FK_GOUT), en[1], fake(FK_OUT), gp, nullptr, bp[0], ws, n, s.B, s.H,
                                          s.W, 1, phase, nullptr, nullptr, nullptr, nullptr, 0, 0);
                else
                  e = r2l_isp_step_bwd_layout(fake(FK_RAW), u16, 65535.f, addp, fake(FK_GOUT), en[1], en[2], fake(FK_OUT), gp, nullptr, bp[0], ws, n,
                                              s.B, s.H, s.W, 1, phase, nullptr, nullptr, nullptr, nullptr, 0, 0);
                per.push_back(answer(e));
              }
              tokens.push_back(p_token(per));
            }
        snprintf(key, sizeof key, "step_bwd n%d io%d l%d u%d bn%d p%d", en[0], en[1], en[2], u16, bp[0], bp[1]);
        p_line(ov, key, tokens);
      }
  dry = false;
}

// ---- R / S lines ------------------------------------------------------------------------------------------------------------
struct Run {
  const char* tag;
  int entry;  // 0: r2l_isp_fwd[_u16] (out + stats); 1: r2l_isp_step_fwd_layout; 2: ... then r2l_isp_step_bwd_layout
  int u16, B, H, W;
  int bn_mode = R2L_BN_NONE, phase = R2L_STEP_ALL, io = R2L_IO_F32, layout = R2L_LAYOUT_NCHW;
  bool additive = false, grads = false;
  int flags = 0;  // entry 0
};
static std::string full_launches() {  // "A.G" of every launch, in order
  std::string s;
  for (const auto& l : launches) {
    const int a = intern(whos, "A", l.first), g = intern(shapes, "G", l.second);
    s += (s.empty() ? "" : " ") + std::to_string(a) + "." + std::to_string(g);
  }
  return s;
}
static void run(const Run& q) {
  const int B = q.B, H = q.H, W = q.W;
  const size_t px = (size_t)B * H * W, esz = q.io == R2L_IO_F32 ? 4 : 2, nws = r2l_isp_workspace_bytes(B, H, W);
  Block raw(px * (q.u16 ? 2 : 4)), add(q.additive ? 3 * 256 * 256 * 4 : 0), cot(3 * px * esz);
  fill_raw(lcg01, raw.p, px, q.u16, 0.02f, 0.9f);  // values below the black level, inside, and (after white balance) above the clip
  for (size_t i = 0; i < add.n / 4; ++i) ((float*)add.p)[i] = 0.1f * (lcg01() - 0.5f);
  for (size_t i = 0; i < 3 * px; ++i) {
    const float g = 2.f * lcg01() - 1.f;
    if (q.io == R2L_IO_F32) ((float*)cot.p)[i] = g;
    else ((unsigned short*)cot.p)[i] = (unsigned short)(q.io == R2L_IO_BF16 ? r2l_f32_to_bf16_bits(g) : r2l_f32_to_f16_bits(g));
  }
  const float* addp = q.additive ? (const float*)add.p : nullptr;
  const float bnv[6] = {0.4f, 0.45f, 0.35f, 4.f, 3.5f, 4.5f};
  for (int less = 0; less <= 1; ++less) {
    Block ws(nws - less), out(3 * px * esz);
    float rm[3] = {0.4f, 0.45f, 0.35f}, rv[3] = {0.03f, 0.05f, 0.04f}, gp[R2L_P_NTRAIN];
    long long nbt = 0;
    double stats[7];
    memset(stats, 0xff, sizeof stats);
    memset(gp, 0xff, sizeof gp);
    ranges = {Range{raw.p, raw.n, "raw"}, Range{out.p, out.n, "out"}, Range{ws.p, ws.n, "ws"}, Range{(char*)stats, sizeof stats, "stats"},
              Range{(const char*)bnv, sizeof bnv, "bn"}, Range{add.p, add.n, "add"}, Range{(char*)rm, sizeof rm, "rm"},
              Range{(char*)rv, sizeof rv, "rv"}, Range{(char*)&nbt, sizeof nbt, "nbt"}, Range{cot.p, cot.n, "gout"},
              Range{(char*)gp, sizeof gp, "gp"}, Range{(const char*)PARAMS, sizeof PARAMS, "params"}};
    begin_call(B, H, W);
    int e;
    if (q.entry == 0)
      e = q.u16 ? r2l_isp_fwd_u16((const unsigned short*)raw.p, 65535.f, PARAMS, addp, bnv, (float*)out.p, stats, ws.p, ws.n, B, H, W, q.flags, nullptr)
                : r2l_isp_fwd((const float*)raw.p, PARAMS, addp, bnv, (float*)out.p, stats, ws.p, ws.n, B, H, W, q.flags, nullptr);
    else {
      const int fphase = q.entry == 2 ? (q.phase & ~3) | R2L_STEP_ALL : q.phase;
      e = r2l_isp_step_fwd_layout(raw.p, q.u16, 65535.f, TABLE, addp, q.bn_mode, rm, rv, &nbt, 1e-5, 0.1, out.p, q.io, q.layout, ws.p, ws.n, B, H,
                                  W, 1, fphase, nullptr, nullptr);
      if (q.entry == 2 && !e) {  // (the record of the backward alone)
        begin_call(B, H, W);
        e = r2l_isp_step_bwd_layout(raw.p, q.u16, 65535.f, addp, cot.p, q.io, q.layout, out.p, q.grads ? gp : nullptr, nullptr, q.bn_mode, ws.p,
                                    ws.n, B, H, W, 1, q.phase, nullptr, nullptr, nullptr, nullptr, 0, 0);
      }
    }
    const std::string rec = end_call_record();
    const std::string ls = less ? "" : full_launches();  // (numbers a text the first time it is seen: before the line)
    printf("%c %s n%d u%d %dx%dx%d bn%d p%d io%d l%d a%d f%d ws %zu -> %d [%s] [%s]", less ? 'S' : 'R', q.tag, q.entry, q.u16, B, H, W, q.bn_mode,
           q.phase, q.io, q.layout, (int)q.additive, q.flags, ws.n, e, e ? r2l_last_error() : "", rec.c_str());
    if (less) {
      printf("\n");
      if (e != -2 || !launches.empty()) ++failures, fprintf(stderr, "one byte less of workspace must return -2 before any launch\n");
      continue;
    }
    printf(" {%s} out %016llx", ls.c_str(), fnv1a(out.p, out.n));
    if (q.entry == 0) printf(" stats %016llx", fnv1a(stats, sizeof stats));
    else {
      printf(" stats %016llx rm %016llx rv %016llx nbt %lld", fnv1a(ws.p + r2l_isp_step_offset(R2L_STEP_STATS, B, H, W), 7 * sizeof(double)),
             fnv1a(rm, sizeof rm), fnv1a(rv, sizeof rv), nbt);
    }
    if ((q.entry == 0 && (q.flags & R2L_F_KEEP_LUMA)) || (q.entry && (q.phase & R2L_STEP_KEEP_LUMA)))
      printf(" yp %016llx", fnv1a(ws.p + r2l_isp_step_offset(R2L_STEP_LUMA, B, H, W), px * 4));
    if (q.entry == 2) {
      printf(" bsums %016llx", fnv1a(ws.p + r2l_isp_step_offset(R2L_STEP_BN_SUMS, B, H, W), 6 * sizeof(double)));
      if ((q.phase & 3) == R2L_STEP_ALL) printf(" bn_bwd %016llx", fnv1a(ws.p + r2l_isp_step_offset(R2L_STEP_BN, B, H, W) + 32, 6 * sizeof(float)));
      if (q.grads) printf(" gp %016llx", fnv1a(gp, sizeof gp));
    }
    printf("\n");
  }
}
static Run mk(const char* tag, int entry, int u16, int B, int H, int W, int bn_mode = R2L_BN_NONE, int phase = R2L_STEP_ALL, int io = R2L_IO_F32,
              int layout = R2L_LAYOUT_NCHW) {
  Run q{tag, entry, u16, B, H, W};
  q.bn_mode = bn_mode, q.phase = phase, q.io = io, q.layout = layout;
  return q;
}
static void runs() {
  const int K = R2L_STEP_KEEP_LUMA, TR = R2L_BN_TRAIN;
  static const int widths[4] = {8, 260, 516, 1028};  // 1, 2, 4, 8 wavefronts per row
  int n = 0;
  // the row-streaming kernel: r2l_isp_fwd with out and stats (one launch), the step without BatchNorm, with an epilogue, in eval mode
  for (int W : widths) {
    Run q = mk("stream", 0, n++ & 1, 1, 8, W);
    q.flags = W == 260 ? R2L_F_KEEP_LUMA : 0;
    run(q);
    run(mk("stream", 1, n++ & 1, W == 8 ? 2 : 1, W == 260 ? 14 : 8, W, R2L_BN_NONE, K));
  }
  for (int u16 = 0; u16 < 2; ++u16) {
    run(mk("stream_epi", 1, u16, 1, 8, 8, R2L_BN_EVAL, R2L_STEP_EPI_VFLIP | (1 << R2L_STEP_EPI_ROT_SHIFT)));
    run(mk("stream_epi", 1, u16, 2, 14, 260, R2L_BN_NONE, K | R2L_STEP_EPI_HFLIP));
  }
  // train mode: luma pass + statistics from the plane + apply (one strip), streaming statistics + apply (wider); phases A and B
  for (int W : widths)
    for (int u16 = 0; u16 < 2; ++u16)
      if (W <= 260 || u16 == (W == 516)) run(mk(W <= 256 ? "split_apply" : "stats_apply", 1, u16, W == 8 ? 2 : 1, W == 260 ? 14 : 8, W, TR, K));
  for (int u16 = 0; u16 < 2; ++u16) {
    run(mk("split_apply_epi", 1, u16, 1, 8, 8, TR, R2L_STEP_EPI_HFLIP | R2L_STEP_EPI_VFLIP));
    run(mk("stats_apply_epi", 1, u16, 1, 14, 260, TR, K | R2L_STEP_EPI_VFLIP));
    run(mk("phase_a", 1, u16, 1, 8, u16 ? 260 : 8, TR, R2L_STEP_A | K));
  }
  // r2l_isp_fwd: statistics alone (the streaming kernel's statistics instantiation)
  for (int u16 = 0; u16 < 2; ++u16) {
    Run q = mk("stats_only", 0, u16, 1, 8, u16 ? 8 : 260);
    q.flags = R2L_F_STATS_ONLY | (u16 ? R2L_F_KEEP_LUMA : 0);
    run(q);
  }
  // every io slot, both frame types: the streaming kernel (no BatchNorm) and the apply pass (train)
  for (int layout = 0; layout < 2; ++layout)
    for (int io = 0; io < 3; ++io) {
      if (!layout && !io) continue;
      for (int u16 = 0; u16 < 2; ++u16) {
        run(mk("stream_io", 1, u16, 1, 8, 8, R2L_BN_NONE, K, io, layout));
        run(mk("apply_io", 1, u16, 1, 8, 8, TR, K, io, layout));
      }
    }
  run(mk("stream_io", 1, 0, 1, 8, 516, R2L_BN_EVAL, K, R2L_IO_BF16, R2L_LAYOUT_NHWC));
  run(mk("apply_io", 1, 1, 2, 14, 260, TR, K, R2L_IO_F16, R2L_LAYOUT_NCHW));
  // the tile kernels: ragged (W % 4 != 0), exact (past 2048 columns), additive (256 x 256)
  for (int u16 = 0; u16 < 2; ++u16) {
    if (!u16) run(mk("tile_ragged", 0, 0, 1, 8, 10));
    if (!u16) run(mk("tile_ragged", 1, 0, 2, 14, 10, TR, K | R2L_STEP_EPI_HFLIP));
    run(mk("tile_exact", 1, u16, 1, 64, 2112, u16 ? TR : R2L_BN_NONE, K));
  }
  for (int u16 = 0; u16 < 2; ++u16) {
    Run q = mk("tile_additive", 1, u16, 1, 256, 256, u16 ? R2L_BN_EVAL : TR, K);
    q.additive = true;
    run(q);
  }
  // the backward's BatchNorm sums from raw + Y' (r2l_bnr_planes_block): a 16-bit / channels-last cotangent takes it at every size
  for (int layout = 0; layout < 2; ++layout)
    for (int io = 0; io < 3; ++io) {
      if (!layout && !io) continue;
      for (int u16 = 0; u16 < 2; ++u16) run(mk("bnr_io", 2, u16, 1, 8, 8, TR, ((io + u16) & 1 ? R2L_STEP_A : R2L_STEP_ALL) | K, io, layout));
    }
  {
    Run q = mk("bnr_io_grads", 2, 0, 1, 8, 260, TR, K, R2L_IO_BF16, R2L_LAYOUT_NCHW);
    q.grads = true;
    run(q);
  }
  // ... float32 below 6 Mi px: r2l_bn_bwd_reduce; with R2L_BWD_PLANES of diagnostic builds the plane pass, with and without epilogue
  run(mk("bn_reduce", 2, 0, 1, 8, 8, TR, K));
  setenv("R2L_BWD_PLANES", "1", 1);
  for (int u16 = 0; u16 < 2; ++u16) {
    run(mk("bnr", 2, u16, 1, 8, u16 ? 260 : 8, TR, (u16 ? R2L_STEP_A : R2L_STEP_ALL) | K));
    run(mk("bnr_epi", 2, u16, 1, 8, 8, TR, (u16 ? R2L_STEP_ALL : R2L_STEP_A) | K | R2L_STEP_EPI_HFLIP));
  }
  run(mk("bnr_no_luma", 2, 0, 1, 8, 8, TR, 0));
  unsetenv("R2L_BWD_PLANES");
  // the overrides of diagnostic builds
  setenv("R2L_FWD_TILED", "1", 1);
  run(mk("tiled", 1, 0, 1, 64, 64, TR, K));
  run(mk("tiled", 1, 1, 1, 8, 8, R2L_BN_NONE, 0));
  unsetenv("R2L_FWD_TILED");
  setenv("R2L_FORCE_SPLIT", "1", 1);
  {
    Run q = mk("force_split", 0, 0, 1, 8, 8);
    q.flags = R2L_F_STATS_ONLY;
    run(q);
    Run r = mk("force_split", 0, 1, 1, 8, 8);
    run(r);
  }
  unsetenv("R2L_FORCE_SPLIT");
  setenv("R2L_FWD_APPLY_RECOMPUTE", "1", 1);
  run(mk("apply_recompute", 1, 0, 1, 8, 8, TR, K));
  unsetenv("R2L_FWD_APPLY_RECOMPUTE");
  setenv("R2L_FWD_STATS_SPLIT", "1", 1);
  run(mk("stats_split", 1, 0, 1, 8, 260, TR, K));
  unsetenv("R2L_FWD_STATS_SPLIT");
  setenv("R2L_FWD_STATS_STREAM", "1", 1);
  run(mk("stats_stream", 1, 1, 1, 8, 8, TR, K));
  unsetenv("R2L_FWD_STATS_STREAM");
  for (const char* v : {"R2L_FS_BAND", "R2L_FL_BAND", "R2L_FST_BAND", "R2L_FA_BAND"}) setenv(v, "6", 1);
  setenv("R2L_GRID_FWD", "1", 1);
  run(mk("bands6_grid1", 1, 0, 2, 14, 8, TR, K));
  run(mk("bands6_grid1", 1, 0, 2, 14, 260, TR, K));
  run(mk("bands6_grid1", 1, 0, 2, 14, 10, TR, K));
  for (const char* v : {"R2L_FS_BAND", "R2L_FL_BAND", "R2L_FST_BAND", "R2L_FA_BAND", "R2L_GRID_FWD"}) unsetenv(v);
  setenv("R2L_BNR_BAND", "6", 1);
  setenv("R2L_GRID_BNR", "1", 1);
  run(mk("bnr_band6_grid1", 2, 0, 2, 14, 8, TR, K, R2L_IO_F16));
  run(mk("bnr_band6_grid1", 2, 0, 2, 14, 8, TR, K));
  unsetenv("R2L_BNR_BAND");
  unsetenv("R2L_GRID_BNR");
}

// ---- X lines ----------------------------------------------------------------------------------------------------------------
struct Bad {
  int u16 = 0, B = 1, H = 8, W = 8, flags = 0, bn_mode = R2L_BN_NONE, phase = 0, nranks = 1, io = 0, layout = 0;
  float denom = 65535.f;
  bool null_raw = false, null_params = false, null_out = false, null_stats = true, null_ws = false, additive = false, small_ws = false;
  bool null_table = false, null_entry = false, null_rm = false, null_rv = false, gathered = false, misaligned = false;
};
static void refused_fwd(const char* tag, const Bad& q) {
  const size_t px = (size_t)(q.B > 0 ? q.B : 1) * q.H * q.W;
  Block raw(px * 4, 0x3c), out(3 * px * 4), ws(r2l_isp_workspace_bytes(q.B > 0 ? q.B : 1, q.H, q.W) + 4096), add(3 * 256 * 256 * 4, 0);
  double stats[7];
  const unsigned long long before = fnv1a(out.p, out.n);
  begin_call(q.B, q.H, q.W);
  float* o = q.null_out ? nullptr : (float*)out.p;
  double* st = q.null_stats ? nullptr : stats;
  const float* P = q.null_params ? nullptr : PARAMS;
  const float* a = q.additive ? (const float*)add.p : nullptr;
  void* w = q.null_ws ? nullptr : ws.p;
  const size_t wn = q.small_ws ? 1024 : ws.n;
  const int e = q.u16 ? r2l_isp_fwd_u16(q.null_raw ? nullptr : (const unsigned short*)raw.p, q.denom, P, a, nullptr, o, st, w, wn, q.B, q.H, q.W,
                                        q.flags, nullptr)
                      : r2l_isp_fwd(q.null_raw ? nullptr : (const float*)raw.p, P, a, nullptr, o, st, w, wn, q.B, q.H, q.W, q.flags, nullptr);
  const std::string rec = end_call_record();
  printf("X fwd %s -> %d [%s] [%s]\n", tag, e, e ? r2l_last_error() : "", rec.c_str());
  if (!e || fnv1a(out.p, out.n) != before || !rec.empty()) ++failures, fprintf(stderr, "%s: must fail before any launch\n", tag);
}
static void refused_step(const char* tag, const Bad& q) {
  const size_t px = (size_t)(q.B > 0 ? q.B : 1) * q.H * q.W;
  Block raw(px * 4, 0x3c), out(3 * px * 4 + 8), ws(r2l_isp_workspace_bytes(q.B > 0 ? q.B : 1, q.H, q.W) + 4096), add(3 * 256 * 256 * 4, 0);
  float rm[3] = {0.4f, 0.45f, 0.35f}, rv[3] = {0.03f, 0.05f, 0.04f};
  long long nbt = 0;
  double gathered[7] = {1, 1, 1, 2, 2, 2, 64};
  const float* table[9];
  for (int i = 0; i < 9; ++i) table[i] = TABLE[i];
  if (q.null_entry) table[4] = nullptr;
  const unsigned long long before = fnv1a(out.p, out.n);
  begin_call(q.B, q.H, q.W);
  const int e = r2l_isp_step_fwd_layout(q.null_raw ? nullptr : raw.p, q.u16, q.denom, q.null_table ? nullptr : table, q.additive ? (const float*)add.p : nullptr,
                                        q.bn_mode, q.null_rm ? nullptr : rm, q.null_rv ? nullptr : rv, &nbt, 1e-5, 0.1,
                                        q.null_out ? nullptr : out.p + (q.misaligned ? 4 : 0), q.io, q.layout, q.null_ws ? nullptr : ws.p,
                                        q.small_ws ? 1024 : ws.n, q.B, q.H, q.W, q.nranks, q.phase, q.gathered ? gathered : nullptr, nullptr);
  const std::string rec = end_call_record();
  printf("X step_fwd %s -> %d [%s] [%s]\n", tag, e, e ? r2l_last_error() : "", rec.c_str());
  // (a refusal of the forward behind the step comes after the step's own launches: the record pins which)
  if (!e || fnv1a(out.p, out.n) != before) ++failures, fprintf(stderr, "%s: must fail, and write nothing\n", tag);
}
// more work items than an int counts: refused after the fold launch, before any other (dry: nothing is dereferenced)
static void too_large() {
  dry = true;
  dry_ranges();
  const int B = (1 << 30) + 2, H = 4, W = 4;
  const size_t n = r2l_isp_workspace_bytes(B, H, W);
  begin_call(B, H, W);
  int e = r2l_isp_fwd((const float*)fake(FK_RAW), (const float*)fake(FK_COUNT), nullptr, nullptr, (float*)fake(FK_OUT), nullptr, fake(FK_WS), n, B, H,
                      W, 0, nullptr);
  std::string rec = end_call_record();
  printf("X fwd too large -> %d [%s] [%s]\n", e, e ? r2l_last_error() : "", rec.c_str());
  for (int bn_mode : {R2L_BN_NONE, R2L_BN_TRAIN}) {
    begin_call(B, H, W);
    e = r2l_isp_step_fwd(fake(FK_RAW), 0, 1.f, FAKE_TABLE, nullptr, bn_mode, nullptr, nullptr, nullptr, 1e-5, 0.1, (float*)fake(FK_OUT), fake(FK_WS),
                         n, B, H, W, 1, R2L_STEP_KEEP_LUMA, nullptr, nullptr);
    rec = end_call_record();
    printf("X step_fwd too large, bn %d -> %d [%s] [%s]\n", bn_mode, e, e ? r2l_last_error() : "", rec.c_str());
  }
  setenv("R2L_FWD_STATS_STREAM", "1", 1);  // (so that the apply pass is the first to count too many)
  begin_call(B / 2, H, W);
  e = r2l_isp_step_fwd(fake(FK_RAW), 0, 1.f, FAKE_TABLE, nullptr, R2L_BN_TRAIN, nullptr, nullptr, nullptr, 1e-5, 0.1, (float*)fake(FK_OUT),
                       fake(FK_WS), r2l_isp_workspace_bytes(B / 2, H, W), B / 2, H, W, 1, R2L_STEP_KEEP_LUMA, nullptr, nullptr);
  rec = end_call_record();
  printf("X step_fwd not too large -> %d [%s] [%s]\n", e, e ? r2l_last_error() : "", rec.c_str());
  unsetenv("R2L_FWD_STATS_STREAM");
  begin_call(B, H, W);
  e = r2l_isp_step_bwd_io(fake(FK_RAW), 0, 1.f, nullptr, fake(FK_GOUT), R2L_IO_BF16, nullptr, nullptr, nullptr, R2L_BN_TRAIN, fake(FK_WS), n, B, H, W,
                          1, R2L_STEP_A | R2L_STEP_KEEP_LUMA, nullptr, nullptr, nullptr, nullptr, 0, 0);
  rec = end_call_record();
  printf("X step_bwd_io too large -> %d [%s] [%s]\n", e, e ? r2l_last_error() : "", rec.c_str());
  dry = false;
}
#define BAD(fn, tag, ...)  \
  {                        \
    Bad q;                 \
    __VA_ARGS__;           \
    fn(tag, q);            \
  }
static void refusals() {
  const int K = R2L_STEP_KEEP_LUMA;
  BAD(refused_fwd, "B = 0", q.B = 0)
  BAD(refused_fwd, "odd H", q.H = 7)
  BAD(refused_fwd, "W = 2", q.W = 2)
  BAD(refused_fwd, "null raw", q.null_raw = true)
  BAD(refused_fwd, "null raw, 16-bit", q.null_raw = true; q.u16 = 1)
  BAD(refused_fwd, "16-bit, denom 0", q.u16 = 1; q.denom = 0.f)
  BAD(refused_fwd, "16-bit, W % 4", q.u16 = 1; q.W = 10)
  BAD(refused_fwd, "null params", q.null_params = true)
  BAD(refused_fwd, "null workspace", q.null_ws = true)
  BAD(refused_fwd, "additive, 8 x 8", q.additive = true)
  BAD(refused_fwd, "nothing to compute", q.null_out = true)
  BAD(refused_fwd, "STATS_ONLY without stats", q.flags = R2L_F_STATS_ONLY)
  BAD(refused_fwd, "workspace too small", q.small_ws = true)
  // wrong in two ways: the order of the checks
  BAD(refused_fwd, "odd H + null raw", q.H = 7; q.null_raw = true)
  BAD(refused_fwd, "null raw + null params", q.null_raw = true; q.null_params = true)
  BAD(refused_fwd, "16-bit W % 4 + null params", q.u16 = 1; q.W = 10; q.null_params = true)
  BAD(refused_fwd, "null params + additive 8 x 8", q.null_params = true; q.additive = true)
  BAD(refused_fwd, "additive 8 x 8 + nothing to compute", q.additive = true; q.null_out = true)
  BAD(refused_fwd, "nothing to compute + workspace too small", q.null_out = true; q.small_ws = true)
  BAD(refused_fwd, "null workspace + workspace too small", q.null_ws = true; q.small_ws = true)
  for (const char* ov : {"", "R2L_FWD_TILED", "R2L_FORCE_SPLIT"}) {
    if (*ov) setenv(ov, "1", 1);
    BAD(refused_fwd, *ov ? ov : "internal flag bits are ignored: nothing to compute", q.null_out = true; q.flags = 1024 | 2048)
    if (*ov) unsetenv(ov);
  }
  BAD(refused_step, "B = 0", q.B = 0)
  BAD(refused_step, "odd W", q.W = 9)
  BAD(refused_step, "rot90 on 8 x 12", q.W = 12; q.phase = 1 << R2L_STEP_EPI_ROT_SHIFT)
  BAD(refused_step, "null raw", q.null_raw = true)
  BAD(refused_step, "null out", q.null_out = true)
  BAD(refused_step, "null workspace", q.null_ws = true)
  BAD(refused_step, "bn_mode 3", q.bn_mode = 3)
  BAD(refused_step, "phase 3", q.phase = 3)
  BAD(refused_step, "nranks 0", q.nranks = 0)
  BAD(refused_step, "two ranks, ALL, train", q.nranks = 2; q.bn_mode = R2L_BN_TRAIN)
  BAD(refused_step, "phase A without train", q.phase = R2L_STEP_A)
  BAD(refused_step, "phase B without gathered", q.phase = R2L_STEP_B; q.bn_mode = R2L_BN_TRAIN)
  BAD(refused_step, "eval without running statistics", q.bn_mode = R2L_BN_EVAL; q.null_rm = q.null_rv = true)
  BAD(refused_step, "running_mean alone", q.null_rv = true)
  BAD(refused_step, "workspace too small", q.small_ws = true)
  BAD(refused_step, "null parameter table", q.null_table = true)
  BAD(refused_step, "null parameter pointer", q.null_entry = true)
  BAD(refused_step, "16-bit, denom 0", q.u16 = 1; q.denom = 0.f)
  BAD(refused_step, "16-bit, W % 4", q.u16 = 1; q.W = 10)
  BAD(refused_step, "additive, 8 x 8", q.additive = true)
  BAD(refused_step, "additive 256 x 256 with an epilogue", q.additive = true; q.H = q.W = 256; q.phase = R2L_STEP_EPI_HFLIP)
  BAD(refused_step, "additive 256 x 256 with an epilogue, train", q.additive = true; q.H = q.W = 256; q.phase = R2L_STEP_EPI_HFLIP; q.bn_mode = R2L_BN_TRAIN)
  // two ways
  BAD(refused_step, "rot90 on 8 x 12 + null raw", q.W = 12; q.phase = 1 << R2L_STEP_EPI_ROT_SHIFT; q.null_raw = true)
  BAD(refused_step, "null out + bn_mode 3", q.null_out = true; q.bn_mode = 3)
  BAD(refused_step, "bn_mode 3 + phase 3", q.bn_mode = 3; q.phase = 3)
  BAD(refused_step, "phase 3 + nranks 0", q.phase = 3; q.nranks = 0)
  BAD(refused_step, "phase B without gathered + workspace too small", q.phase = R2L_STEP_B; q.bn_mode = R2L_BN_TRAIN; q.small_ws = true)
  BAD(refused_step, "workspace too small + null parameter table", q.small_ws = true; q.null_table = true)
  BAD(refused_step, "workspace too small + 16-bit W % 4", q.small_ws = true; q.u16 = 1; q.W = 10)
  BAD(refused_step, "null parameter table + additive 8 x 8", q.null_table = true; q.additive = true)
  // 16-bit / channels-last output
  for (int layout = 0; layout < 2; ++layout)
    for (int io = 0; io < 3; ++io) {
      if (!layout && !io) continue;
      char tag[96];
#define IOBAD(what, ...)                                            \
  {                                                                 \
    snprintf(tag, sizeof tag, "io%d l%d %s", io, layout, what);     \
    Bad q;                                                          \
    q.io = io, q.layout = layout, q.phase = K;                      \
    __VA_ARGS__;                                                    \
    refused_step(tag, q);                                           \
  }
      IOBAD("odd H", q.H = 7)
      IOBAD("additive", q.additive = true; q.H = q.W = 256)
      IOBAD("W % 4", q.W = 10)
      IOBAD("W > 2048", q.W = 2052)
      IOBAD("epilogue", q.phase = K | R2L_STEP_EPI_HFLIP)
      IOBAD("no KEEP_LUMA", q.phase = 0)
      IOBAD("misaligned", q.misaligned = true)
      IOBAD("W % 4 + null out", q.W = 10; q.null_out = true)
      IOBAD("null out", q.null_out = true)
      setenv("R2L_FWD_TILED", "1", 1);
      IOBAD("R2L_FWD_TILED", )
      unsetenv("R2L_FWD_TILED");
#undef IOBAD
    }
  BAD(refused_step, "io 3", q.io = 3; q.phase = K)
  BAD(refused_step, "layout 2", q.layout = 2; q.phase = K)
  too_large();
}

int run(int, char**) {
  static const char* const OVERRIDES[13][2] = {{"R2L_FWD_TILED", "1"},        {"R2L_FORCE_SPLIT", "1"},      {"R2L_FWD_APPLY_RECOMPUTE", "1"},
                                               {"R2L_FWD_STATS_SPLIT", "1"},  {"R2L_FWD_STATS_STREAM", "1"}, {"R2L_FS_BAND", "32"},
                                               {"R2L_FL_BAND", "12"},         {"R2L_FST_BAND", "12"},        {"R2L_FA_BAND", "12"},
                                               {"R2L_GRID_FWD", "8"},         {"R2L_BNR_BAND", "12"},        {"R2L_GRID_BNR", "8"},
                                               {"R2L_BWD_PLANES", "1"}};
  for (const auto& ov : OVERRIDES) unsetenv(ov[0]);
  for (const char* v : {"R2L_BWD1_RECOMPUTE", "R2L_BWD1_TILED", "R2L_BWD2_TILED", "R2L_BWD_SPLIT_BLUR", "R2L_GRID_BWD1", "R2L_GRID_BWD2"}) unsetenv(v);
  make_params();
  r2l_ls::g_observer = observe;
  puts("# a launch = A (kernel, then its arguments by role: raw F bn out yp_out yp_in stat_partial tree stats_out fin [bnr_planes: gout sums");
  puts("#   totals bn_bwd]; tile kernels: raw additive F bn out stat_partial debug tree stats_out fin; -: null, ws+Y: the Y' plane)");
  puts("#   and G ([wavefronts per row,] grid, threads, LDS floats, band_h x nband = nitems, epilogue on,s0,sr,sc); E: an error text");
  puts("# P <override> <key>: VA/VG for every combination of the key's inner dimensions -- fwd: bn_mean_istd x KEEP_LUMA x additive; stats_bn:");
  puts("#   additive; step_fwd, step_bwd: KEEP_LUMA x epilogue (none, hflip, vflip + rot90) x additive.  VA, VG: per shape, launches");
  puts("#   joined by +, e<code>.<E>: refused.  fwd m: out, stats, both, both + STATS_ONLY; n: entry (0 plain, 1 _io, 2 _layout)");
  puts("#   fwd / stats_bn / step_fwd shapes 1x8x8 1x8x10 2x14x260 1x8x516 1x8x1028 1x64x64 1x256x256 64x512x512");
  puts("#   64x256x256 128x256x256 8x1024x1024 2x2048x2048 1x1024x2052; step_bwd shapes 1x8x8 1x8x10 2x14x260 1x256x256 63x256x256");
  puts("#   64x256x256 95x256x256 96x256x256 64x512x512 128x256x256 2x2048x2048 1x1024x2052; under an override: the keys that differ");
  plans(nullptr);
  for (const auto& ov : OVERRIDES) {
    setenv(ov[0], ov[1], 1);
    p_same = p_differ = 0;
    plans(ov[0]);
    printf("P %s=%s: %ld answers as without, %ld differ\n", ov[0] + 4, ov[1], p_same, p_differ);
    unsetenv(ov[0]);
  }
  puts("# R|S tag entry u16 BxHxW bn_mode phase io layout additive flags workspace -> code [error] [launch record: r2l_launch_<name>_kernel*count] {launches} results");
  runs();
  puts("# X what -> code [error] [launch record]");
  refusals();
  fflush(stdout);
  return failures ? 1 : 0;
}
#undef BAD

}  // namespace r2l_drv::fwd_routes
