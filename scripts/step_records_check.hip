// Host-only check of the loss steps' launch records, for an address/undefined-behaviour sanitizer build.  Launches nothing and
// needs no device: it fills the fused-sweep records of the teacher, the student and every scale, the shared builders of
// mal_march.h, and runs the argument checks with null and aliased operands.
//
//   python -m mal_amd.build                     # the other translation units' objects (mal_amd/lib/*.o)
//   F="-O1 -g --offload-arch=gfx950 -std=c++17 -fPIC -fno-gpu-rdc -I mal_amd/csrc -Xarch_host -fsanitize=address,undefined"
//   hipcc $F -c scripts/step_records_check.hip -o /tmp/step_records_check.o
//   hipcc --offload-arch=gfx950 -fsanitize=address,undefined /tmp/step_records_check.o \
//         $(ls mal_amd/lib/*.o | grep -v -e mal_photo_march.o -e mal_step.o -e mal_step_ms.o) -o /tmp/step_records_check
//   /tmp/step_records_check                     # prints "step records: N checks passed", exit status 0
//
// The three sources under test are included, not linked, so that their file-local builders and checks are reachable.
#include "../mal_amd/csrc/mal_photo_march.hip"
#include "../mal_amd/csrc/mal_step.hip"
#include "../mal_amd/csrc/mal_step_ms.hip"
#include <cstdio>
#include <vector>

static int g_checks = 0, g_failed = 0;
#define CHECK(c) do { ++g_checks; if (!(c)) { ++g_failed; std::printf("FAILED line %d: %s\n", __LINE__, #c); } } while (0)

int main() {
  const int B = 2, H = 32, W = 64, S = 2;
  CHECK(mal_set_option("device_cus", 256) == MAL_OK);  // the decompositions without a device query
  // every operand a distinct address inside one host buffer: the records and checks compare pointers, nothing is dereferenced
  std::vector<float> pool((size_t)256 * B * 3 * H * W);
  size_t next = 0;
  auto buf = [&]() { float* p = pool.data() + next; next += (size_t)B * 3 * H * W; return p; };
  std::vector<char> ws(mal_step_workspace_bytes(B, H, W)), ws_ms(mal_ms_workspace_bytes(B, H, W, S - 1));
  float losses[64] = {};

  mal_step_args a = {};
  a.B = B; a.H = H; a.W = W; a.min_depth = 0.1f; a.max_depth = 100.f; a.w_main = 0.7f; a.w_distil = 0.3f;
  a.color0 = buf(); a.color_m1 = buf(); a.color_p1 = buf(); a.K = buf(); a.inv_K = buf();
  a.disp_teacher = buf(); a.disp_student = buf(); a.axisangle_m1 = buf(); a.translation_m1 = buf(); a.axisangle_p1 = buf();
  a.translation_p1 = buf(); a.consistency_mask = buf(); a.augmentation_keep = buf(); a.lowest_cost = buf(); a.losses = losses;
  a.ws = ws.data(); a.ws_bytes = ws.size();
  a.flags = MAL_STEP_TEMPORAL | MAL_STEP_MAIN_TEMPORAL | MAL_STEP_SYN_SPARSE;
  a.noise = buf(); a.warp_m1 = buf(); a.warp_p1 = buf(); a.warp_s_m1 = buf(); a.warp_s_p1 = buf();
  a.syn_m1 = buf(); a.syn_p1 = buf(); a.g_syn_m1 = buf(); a.g_syn_p1 = buf();
  a.syn_s_m1 = buf(); a.syn_s_p1 = buf(); a.g_syn_s_m1 = buf(); a.g_syn_s_p1 = buf();
  a.syn_region = (const uint8_t*)buf(); a.syn_s_region = (const uint8_t*)buf();
  CHECK(step_check(&a) == MAL_OK);
  const StepWs w = step_ws(&a);

  // ---- the teacher's and the student's sweep
  PhotoMarchParams p = {};
  const FusedMoreArgs t = teacher_sweep(&a, w, w.mono_reproj), s = student_sweep(&a, w);
  CHECK(sweep_check(t, true) == MAL_OK && sweep_check(s, false) == MAL_OK);
  CHECK(t.cand0 == a.syn_m1 && t.g_cand1 == a.g_syn_p1 && t.orig0 == a.warp_m1 && t.orig1 == a.warp_p1 && !t.weight_given);
  CHECK(s.ident == w.w_s && s.weight_given == 1 && !s.noise && !s.orig0 && !s.orig1 && s.min_reproj == w.multi_reproj);
  CHECK(fused_more_params(p, t, B, H, W) == MAL_OK && p.target_texels == 1 && p.idx[0] == 2 && p.idx[1] == 3);
  CHECK(p.orig_stride == (size_t)3 * H * W && p.region == a.syn_region && !p.g_region[0] && p.ntasks == B * p.strips * p.segs);
  CHECK(fused_more_params(p, s, B, H, W) == MAL_OK && p.weight_given == 1 && p.ident == w.w_s);
  // ... refused: missing and aliased operands, a shape beyond the 32-bit byte offsets
  FusedMoreArgs x = t;
  x.cand1 = nullptr;
  CHECK(sweep_check(x, true) == MAL_EINVAL);
  x = t; x.region = nullptr;
  CHECK(sweep_check(x, true) == MAL_EINVAL && sweep_check(x, false) == MAL_OK && fused_more_params(p, x, B, H, W) == MAL_EINVAL);
  x = t; x.orig1 = nullptr;
  CHECK(sweep_check(x, true) == MAL_EINVAL && fused_more_params(p, x, B, H, W) == MAL_EINVAL);
  x = t; x.prev_min = x.min_reproj;
  CHECK(fused_more_params(p, x, B, H, W) == MAL_EINVAL);
  x = t; x.prev_arg = x.argmin;
  CHECK(fused_more_params(p, x, B, H, W) == MAL_EINVAL);
  x = s; x.noise = a.noise;
  CHECK(fused_more_params(p, x, B, H, W) == MAL_EINVAL);
  CHECK(fused_more_params(p, t, 4096, 1024, 1024) == MAL_ESHAPE);
  x = t; x.orig_stride = (size_t)1 << 30;
  CHECK(fused_more_params(p, x, B, H, W) == MAL_ESHAPE);
  int per = -1;
  CHECK(photo_march_fused_more_n(0, &t, B, H, W, &per, nullptr) == MAL_EINVAL && per == -1);
  CHECK(photo_march_fused_more_n(MAL_MS_MAX_SCALES + 1, &t, B, H, W, &per, nullptr) == MAL_EINVAL);
  x = t; x.prev_min = x.min_reproj;
  CHECK(photo_march_fused_more(x, B, H, W, &per, nullptr) == MAL_EINVAL && per == -1);
  const FusedMoreArgs pair[2] = {t, x};
  CHECK(photo_march_fused_more_n(2, pair, B, H, W, &per, nullptr) == MAL_EINVAL && per == -1);  // (refused before any launch)
  const SmoothMapArgs sm = {a.disp_teacher, a.color0, H, W, w.gn_t, w.bs_p};
  CHECK(smooth_march_sweep_batch(0, &sm, B, nullptr, &per) == MAL_EINVAL && smooth_march_sweep_batch(9, &sm, B, nullptr, &per) == MAL_EINVAL);

  // ---- one sweep per scale
  mal_ms_args m = {};
  m.B = B; m.H = H; m.W = W; m.sclm = S - 1; m.min_depth = 0.1f; m.max_depth = 100.f; m.flags = MAL_STEP_TEMPORAL;
  m.color0 = a.color0; m.color_m1 = a.color_m1; m.color_p1 = a.color_p1; m.K = a.K; m.inv_K = a.inv_K;
  m.axisangle_m1 = a.axisangle_m1; m.translation_m1 = a.translation_m1; m.axisangle_p1 = a.axisangle_p1;
  m.translation_p1 = a.translation_p1; m.consistency_mask = a.consistency_mask; m.augmentation_keep = a.augmentation_keep;
  m.losses = losses; m.ws = ws_ms.data(); m.ws_bytes = ws_ms.size(); m.syn_sparse = 2;  // scale 1 sparse
  for (int k = 0; k < S; ++k) {
    m.disp_teacher[k] = buf(); m.disp_student[k] = buf(); m.color0_s[k] = buf(); m.noise[k] = buf();
    m.warp_m1[k] = buf(); m.warp_p1[k] = buf(); m.syn_m1[k] = buf(); m.syn_p1[k] = buf(); m.g_syn_m1[k] = buf(); m.g_syn_p1[k] = buf();
    m.syn_region[k] = (const uint8_t*)buf();
  }
  CHECK(ms_check(&m) == MAL_OK);
  const MsWs mw = carve_ms(m.ws, B, H, W, m.sclm);
  for (int k = 0; k < S; ++k) {
    const FusedMoreArgs q = ms_sweep(&m, mw, k);
    CHECK(q.cand0 == m.syn_m1[k] && q.noise == m.noise[k] && q.prev_min == mw.rp_warp[k] && q.min_reproj == mw.rp4[k]);
    CHECK((q.orig0 == m.warp_m1[k]) == (k == 1) && (q.orig1 == m.warp_p1[k]) == (k == 1) && !q.weight_given);
    CHECK(fused_more_params(p, q, B, H, W) == MAL_OK && p.block_sums == mw.bs_ph[k]);
  }
  m.flags |= MAL_STEP_NOISE_PHILOX;
  CHECK(ms_sweep(&m, mw, 1).noise == mw.noise[1]);

  // ---- the shared builders
  const MarchParams mp = pass_params(&a, w), mq = step_march_params(&m, 1, mw.T[0], mw.T[1], mw.packed, mw.cam);
  CHECK(mp.K == a.K && mp.invK == a.inv_K && mp.T[1] == w.T[1] && mp.target == w.packed[0] && mp.src[0] == w.packed[1]);
  CHECK(mp.src[1] == w.packed[2] && mp.cam == w.cam && mp.cam_ready == 1 && mp.convention == 0 && mp.B == B && mp.W == W);
  CHECK(mq.convention == 1 && mq.cam == mw.cam && mq.src[1] == mw.packed[2] && mq.min_disp == mp.min_disp);
  const StepPoses sp = step_poses(&a, w.T, w.cam, w.ticket);
  CHECK(sp.pose.F == 2 && sp.pose.invert[0] == 1 && sp.pose.invert[1] == 0 && sp.pose.T[0] == w.T[0] && sp.ticket == w.ticket);
  CHECK(sp.pose.axisangle[1] == a.axisangle_p1 && sp.pose.translation[0] == a.translation_m1 && sp.K == a.K && sp.cam == w.cam);
  int pose_bwd = -1;
  PoseParams pb = step_pose_bwd(&a, w.gTs, &pose_bwd);
  CHECK(pose_bwd == 0 && pb.gT[1] == w.gTs[1] && !pb.g_axisangle[0] && !pb.T[0]);
  m.g_translation_p1 = buf();
  pb = step_pose_bwd(&m, mw.gTs, &pose_bwd);
  CHECK(pose_bwd == 1 && pb.g_translation[1] == m.g_translation_p1 && pb.invert[0] == 1);
  CHECK(halo_bnd(w.bnd_t) == w.bnd_t && mal_set_option("march_halo1", 0) == MAL_OK && halo_bnd(w.bnd_t) == nullptr);
  CHECK(mal_set_option("march_halo1", 1) == MAL_OK);

  std::printf("step records: %d checks %s\n", g_checks, g_failed ? "FAILED" : "passed");
  return g_failed ? 1 : 0;
}
