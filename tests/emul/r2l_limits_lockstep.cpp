// r2l_limits_lockstep.cpp -- driver `limits` of r2l_lockstep_drivers.cpp (stand-alone, no Python): the refusals at the documented
// size limits, on the lock-step emulation's sources (r2l_lockstep.cpp, unchanged: the device's host route) under
// -fsanitize=address,undefined.  TEST INFRASTRUCTURE: run by tests/test_large_index.py, which reads the lines
//   <tag> -> <code> [<error text>]
// Every call here must fail BEFORE the launch that would use the sizes it names: the frames, outputs and cotangents are blocks of a
// few bytes and the workspace holds only its fixed head (the parameter fold of a step's forward runs, in that head), so a missed
// refusal is an ASan report, not a pass.  Never run these shapes on a GPU.
//   usage: r2l_lockstep_drivers limits
namespace r2l_drv::limits {

static void line(const char* tag, int e) { printf("%s -> %d [%s]\n", tag, e, e ? r2l_last_error() : ""); }

int run(int, char**) {
  const size_t head = r2l_isp_workspace_bytes(1, 4, 4);  // more than the shape-independent head of any workspace
  std::vector<char> ws(head, 0), small(4096, 0);
  std::vector<float> params(256, 0.5f), grad(R2L_P_NTRAIN, 0.f), rm(3, 0.f), rv(3, 1.f);
  long long nbt = 0;
  const float* table[9];
  param_table(params.data(), table);
  void* raw = small.data();
  float* out = (float*)small.data();
  const size_t all = ~(size_t)0;  // "the workspace is large enough": the calls below must fail before they believe it
  struct Shape { const char* tag; int B, H, W; } dims[] = {{"frame 2^29 + 2 * 2048 px", 1, 262146, 2048},
                                                           {"batch 4097x16384x16384", 4097, 16384, 16384}};
  char tag[128];
  for (const Shape& s : dims) {
    snprintf(tag, sizeof tag, "step_fwd %s", s.tag);
    line(tag, r2l_isp_step_fwd(raw, 0, 1.f, table, nullptr, R2L_BN_NONE, nullptr, nullptr, nullptr, 1e-5, 0.1, out, ws.data(), all, s.B,
                               s.H, s.W, 1, R2L_STEP_ALL | R2L_STEP_KEEP_LUMA, nullptr, nullptr));
    snprintf(tag, sizeof tag, "step_bwd %s", s.tag);
    line(tag, r2l_isp_step_bwd(raw, 0, 1.f, nullptr, out, out, grad.data(), nullptr, R2L_BN_NONE, ws.data(), all, s.B, s.H, s.W, 1,
                               R2L_STEP_ALL | R2L_STEP_KEEP_LUMA, nullptr, nullptr));
    snprintf(tag, sizeof tag, "static_fwd %s", s.tag);
    line(tag, r2l_static_fwd((const float*)raw, out, s.B, s.H, s.W, CAMERA, 0, 0, 0, 2.2, nullptr, 0, nullptr));
  }
  // a frame of exactly 2^29 px passes r2l_check_dims: the call fails at the NEXT check, its workspace of 0 bytes
  line("step_fwd frame 2^29 px, workspace of 0 bytes",
       r2l_isp_step_fwd(raw, 0, 1.f, table, nullptr, R2L_BN_NONE, nullptr, nullptr, nullptr, 1e-5, 0.1, out, ws.data(), 0, 1, 262144, 2048, 1,
                        R2L_STEP_ALL, nullptr, nullptr));
  line("static_fwd frame 2^29 px (Menon2007), workspace of 0 bytes",
       r2l_static_fwd((const float*)raw, out, 1, 262144, 2048, CAMERA, 2, 0, 0, 2.2, ws.data(), 0, nullptr));
  // 2^30 + 2 frames of 4 x 4: one work item per frame in every pass
  const int B = (1 << 30) + 2;
  const int modes[3] = {R2L_BN_NONE, R2L_BN_TRAIN, R2L_BN_EVAL};
  const char* names[3] = {"bn none", "bn train", "bn eval"};
  for (int k = 0; k < 3; ++k) {
    float* m = modes[k] == R2L_BN_NONE ? nullptr : rm.data();
    float* v = modes[k] == R2L_BN_NONE ? nullptr : rv.data();
    snprintf(tag, sizeof tag, "step_fwd 2^30 + 2 frames of 4x4, %s", names[k]);
    line(tag, r2l_isp_step_fwd(raw, 0, 1.f, table, nullptr, modes[k], m, v, modes[k] == R2L_BN_TRAIN ? &nbt : nullptr, 1e-5, 0.1, out,
                               ws.data(), all, B, 4, 4, 1, R2L_STEP_ALL | R2L_STEP_KEEP_LUMA, nullptr, nullptr));
    snprintf(tag, sizeof tag, "step_bwd 2^30 + 2 frames of 4x4, %s", names[k]);
    line(tag, r2l_isp_step_bwd(raw, 0, 1.f, nullptr, out, out, grad.data(), nullptr, modes[k], ws.data(), all, B, 4, 4, 1,
                               R2L_STEP_ALL | R2L_STEP_KEEP_LUMA, nullptr, nullptr));
  }
  for (int chain = 0; chain < 2; ++chain) {  // the row-streaming kernel, the luma-chain kernel
    snprintf(tag, sizeof tag, "static_fwd 2^30 + 2 frames of 4x4, chain %d%d%d", 0, chain, chain);
    line(tag, r2l_static_fwd((const float*)raw, out, B, 4, 4, CAMERA, 0, chain, chain, 2.2, nullptr, 0, nullptr));
  }
  return 0;
}

}  // namespace r2l_drv::limits
