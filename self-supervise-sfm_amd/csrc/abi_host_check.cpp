// Host-side check of the C ABI, built by `make debug` against an AddressSanitizer +
// UndefinedBehaviorSanitizer build of the library (host code only: -Xarch_host -fsanitize=...;
// SURVEY §5 "race detection / sanitizers").  Needs no GPU: it drives every entry point's argument
// validation and dispatch planning up to the launch (which fails without a device, SR_ELAUNCH),
// so ASan / UBSan see the host paths the Python mirror takes.
//
//   abi_host_check layout   JSON: size and field offsets of every ABI struct (tests/test_abi.py
//                           compares them with the ctypes mirror in sailrecon_amd/_lib.py)
//   abi_host_check layout corres   the same for the structs of sr_corres_sample (ABI 1.6), apart:
//                           tests/test_debug_build.py pins the set the plain mode prints
//   abi_host_check layout pose_eval   the same for the structs of sr_pose_pair_errors / sr_pose_align (ABI 1.9)
//   abi_host_check layout imc_stats   the same for sr_imc_stats_desc (ABI 1.10)
//   abi_host_check layout cloud_eval   the same for sr_cloud_nn_desc (ABI 1.11)
//   abi_host_check layout depth_eval   the same for sr_select_desc and sr_depth_eval_desc (ABI 1.12)
//   abi_host_check layout cloud_voxel   the same for sr_sort_desc and sr_cloud_voxel_desc (ABI 1.13)
//   abi_host_check layout sparsify   the same for sr_sparsify_desc (ABI 1.14)
//   abi_host_check layout cloud_render   the same for sr_cloud_render_desc (ABI 1.15)
//   abi_host_check layout two_view   the same for sr_two_view_desc (ABI 1.16)
//   abi_host_check check    the validation sweep; exit 0 iff every call returned what it should
#include <cstddef>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/sfm_amd.h"

namespace {

int g_fail = 0;

void expect(const char* what, int rc, bool ok_launch_fail) {
  // rc < 0 always (no device: a call that passes validation fails at its launch, SR_ELAUNCH);
  // a validation failure must say why
  const char* msg = sr_last_error();
  bool good = rc < 0 && msg && *msg;
  if (!ok_launch_fail && rc == SR_ELAUNCH) good = false;  // should have been rejected before launching
  std::printf("%-44s rc=%d  %s%s\n", what, rc, good ? "" : "UNEXPECTED  ", msg ? msg : "(null)");
  if (!good) ++g_fail;
}

// fake, suitably aligned device addresses: validation never dereferences them
template <typename T = void>
T* fake(uintptr_t i) { return reinterpret_cast<T*>(0x7f0000000000ull + (i << 12)); }

#define FIELD(S, F) std::printf("%s\"%s\": %zu", first ? "" : ", ", #F, offsetof(S, F)), first = false
#define STRUCT(S, BODY)                                                 \
  do {                                                                  \
    bool first = true;                                                  \
    std::printf("%s\"%s\": {\"size\": %zu, \"fields\": {", sep, #S, sizeof(S)); \
    BODY;                                                               \
    std::printf("}}");                                                  \
    sep = ", ";                                                         \
  } while (0)

void layout() {
  const char* sep = "";
  std::printf("{");
  STRUCT(sr_gemm_epi, (FIELD(sr_gemm_epi, bias), FIELD(sr_gemm_epi, gamma), FIELD(sr_gemm_epi, qn_w),
                       FIELD(sr_gemm_epi, qn_b), FIELD(sr_gemm_epi, kn_w), FIELD(sr_gemm_epi, kn_b),
                       FIELD(sr_gemm_epi, qk_eps), FIELD(sr_gemm_epi, rope_cos), FIELD(sr_gemm_epi, rope_sin),
                       FIELD(sr_gemm_epi, rope_npos), FIELD(sr_gemm_epi, col_offset), FIELD(sr_gemm_epi, head_dim),
                       FIELD(sr_gemm_epi, embed_dim), FIELD(sr_gemm_epi, pos_yx), FIELD(sr_gemm_epi, pos_rowmap),
                       FIELD(sr_gemm_epi, pos_row_base), FIELD(sr_gemm_epi, tokens_per_frame),
                       FIELD(sr_gemm_epi, patch_start), FIELD(sr_gemm_epi, grid_w), FIELD(sr_gemm_epi, seg_rows),
                       FIELD(sr_gemm_epi, seg_stride), FIELD(sr_gemm_epi, seg_offset), FIELD(sr_gemm_epi, row_add),
                       FIELD(sr_gemm_epi, aux), FIELD(sr_gemm_epi, ld_aux), FIELD(sr_gemm_epi, q_scale),
                       FIELD(sr_gemm_epi, q_cols), FIELD(sr_gemm_epi, colsum)));
  STRUCT(sr_gemm_problem, (FIELD(sr_gemm_problem, A), FIELD(sr_gemm_problem, lda), FIELD(sr_gemm_problem, W),
                           FIELD(sr_gemm_problem, ldw), FIELD(sr_gemm_problem, out), FIELD(sr_gemm_problem, ldo),
                           FIELD(sr_gemm_problem, M), FIELD(sr_gemm_problem, N), FIELD(sr_gemm_problem, K),
                           FIELD(sr_gemm_problem, ep)));
  STRUCT(sr_wgrad_problem,
         (FIELD(sr_wgrad_problem, A), FIELD(sr_wgrad_problem, lda), FIELD(sr_wgrad_problem, B),
          FIELD(sr_wgrad_problem, ldb), FIELD(sr_wgrad_problem, dW), FIELD(sr_wgrad_problem, lddw),
          FIELD(sr_wgrad_problem, M), FIELD(sr_wgrad_problem, N), FIELD(sr_wgrad_problem, K),
          FIELD(sr_wgrad_problem, accumulate), FIELD(sr_wgrad_problem, rowscale), FIELD(sr_wgrad_problem, wdot),
          FIELD(sr_wgrad_problem, ldwd), FIELD(sr_wgrad_problem, rowdot), FIELD(sr_wgrad_problem, splits),
          FIELD(sr_wgrad_problem, workspace)));
  STRUCT(sr_attn_desc,
         (FIELD(sr_attn_desc, q), FIELD(sr_attn_desc, ldq), FIELD(sr_attn_desc, k0), FIELD(sr_attn_desc, v0),
          FIELD(sr_attn_desc, ldk0), FIELD(sr_attn_desc, ldv0), FIELD(sr_attn_desc, k1), FIELD(sr_attn_desc, v1),
          FIELD(sr_attn_desc, ldk1), FIELD(sr_attn_desc, ldv1), FIELD(sr_attn_desc, o), FIELD(sr_attn_desc, ldo),
          FIELD(sr_attn_desc, batch), FIELD(sr_attn_desc, heads), FIELD(sr_attn_desc, head_dim),
          FIELD(sr_attn_desc, lq), FIELD(sr_attn_desc, q_bstride), FIELD(sr_attn_desc, l0),
          FIELD(sr_attn_desc, k0_bstride), FIELD(sr_attn_desc, l1), FIELD(sr_attn_desc, k1_bstride),
          FIELD(sr_attn_desc, mask_mode), FIELD(sr_attn_desc, n_anchor), FIELD(sr_attn_desc, scale),
          FIELD(sr_attn_desc, lse), FIELD(sr_attn_desc, key_bound), FIELD(sr_attn_desc, key_norm_max),
          FIELD(sr_attn_desc, o_bstride), FIELD(sr_attn_desc, mask), FIELD(sr_attn_desc, mask_bstride),
          FIELD(sr_attn_desc, mask_hstride), FIELD(sr_attn_desc, mask_ld), FIELD(sr_attn_desc, tail_rows_readable),
          FIELD(sr_attn_desc, merge_o), FIELD(sr_attn_desc, ld_merge_o), FIELD(sr_attn_desc, merge_lse),
          FIELD(sr_attn_desc, merge_rows), FIELD(sr_attn_desc, sweep_stats),
          FIELD(sr_attn_desc, key_box), FIELD(sr_attn_desc, value_box), FIELD(sr_attn_desc, key_norm2),
          FIELD(sr_attn_desc, q_scaled)));
  STRUCT(sr_attn_bwd_desc,
         (FIELD(sr_attn_bwd_desc, f), FIELD(sr_attn_bwd_desc, dout), FIELD(sr_attn_bwd_desc, lddo),
          FIELD(sr_attn_bwd_desc, delta), FIELD(sr_attn_bwd_desc, dq), FIELD(sr_attn_bwd_desc, lddq),
          FIELD(sr_attn_bwd_desc, dk0), FIELD(sr_attn_bwd_desc, dv0), FIELD(sr_attn_bwd_desc, lddk0),
          FIELD(sr_attn_bwd_desc, lddv0), FIELD(sr_attn_bwd_desc, dk1), FIELD(sr_attn_bwd_desc, dv1),
          FIELD(sr_attn_bwd_desc, lddk1), FIELD(sr_attn_bwd_desc, lddv1)));
  STRUCT(sr_imc_loss_desc,
         (FIELD(sr_imc_loss_desc, enc), FIELD(sr_imc_loss_desc, n_views), FIELD(sr_imc_loss_desc, H),
          FIELD(sr_imc_loss_desc, W), FIELD(sr_imc_loss_desc, kp2k), FIELD(sr_imc_loss_desc, shared_focal),
          FIELD(sr_imc_loss_desc, n_pairs), FIELD(sr_imc_loss_desc, n_points), FIELD(sr_imc_loss_desc, src_idx),
          FIELD(sr_imc_loss_desc, dst_idx), FIELD(sr_imc_loss_desc, src_coords), FIELD(sr_imc_loss_desc, dst_coords),
          FIELD(sr_imc_loss_desc, src_depth), FIELD(sr_imc_loss_desc, dst_depth), FIELD(sr_imc_loss_desc, node_src),
          FIELD(sr_imc_loss_desc, node_dst), FIELD(sr_imc_loss_desc, n_nodes), FIELD(sr_imc_loss_desc, min_val),
          FIELD(sr_imc_loss_desc, max_val), FIELD(sr_imc_loss_desc, num_bins), FIELD(sr_imc_loss_desc, smooth_w),
          FIELD(sr_imc_loss_desc, smooth_radius), FIELD(sr_imc_loss_desc, grad_scale), FIELD(sr_imc_loss_desc, loss),
          FIELD(sr_imc_loss_desc, d_enc), FIELD(sr_imc_loss_desc, workspace)));
  STRUCT(sr_weight_item,
         (FIELD(sr_weight_item, src), FIELD(sr_weight_item, lds), FIELD(sr_weight_item, rows),
          FIELD(sr_weight_item, cols), FIELD(sr_weight_item, rowscale), FIELD(sr_weight_item, cast),
          FIELD(sr_weight_item, ldc), FIELD(sr_weight_item, trans), FIELD(sr_weight_item, ldt)));
  std::printf("}\n");
}

void layout_corres() {
  const char* sep = "";
  std::printf("{");
  STRUCT(sr_corres_pair,
         (FIELD(sr_corres_pair, src), FIELD(sr_corres_pair, dst), FIELD(sr_corres_pair, dst_y),
          FIELD(sr_corres_pair, conf), FIELD(sr_corres_pair, depth_src), FIELD(sr_corres_pair, depth_dst),
          FIELD(sr_corres_pair, format), FIELD(sr_corres_pair, m), FIELD(sr_corres_pair, hs), FIELD(sr_corres_pair, ws),
          FIELD(sr_corres_pair, h1), FIELD(sr_corres_pair, w1), FIELD(sr_corres_pair, h2), FIELD(sr_corres_pair, w2)));
  STRUCT(sr_corres_desc,
         (FIELD(sr_corres_desc, n_pairs), FIELD(sr_corres_desc, n_points), FIELD(sr_corres_desc, pairs),
          FIELD(sr_corres_desc, max_m), FIELD(sr_corres_desc, uniforms), FIELD(sr_corres_desc, min_conf),
          FIELD(sr_corres_desc, src_coords), FIELD(sr_corres_desc, dst_coords), FIELD(sr_corres_desc, src_depth),
          FIELD(sr_corres_desc, dst_depth), FIELD(sr_corres_desc, index), FIELD(sr_corres_desc, total),
          FIELD(sr_corres_desc, n_valid), FIELD(sr_corres_desc, workspace), FIELD(sr_corres_desc, workspace_doubles)));
  std::printf("}\n");
}

void layout_pose_eval() {
  const char* sep = "";
  std::printf("{");
  STRUCT(sr_pose_pairs_desc,
         (FIELD(sr_pose_pairs_desc, pred), FIELD(sr_pose_pairs_desc, gt), FIELD(sr_pose_pairs_desc, pred_stride),
          FIELD(sr_pose_pairs_desc, gt_stride), FIELD(sr_pose_pairs_desc, n_views), FIELD(sr_pose_pairs_desc, n_pairs),
          FIELD(sr_pose_pairs_desc, pair_i), FIELD(sr_pose_pairs_desc, pair_j),
          FIELD(sr_pose_pairs_desc, trans_ambiguity), FIELD(sr_pose_pairs_desc, n_bins),
          FIELD(sr_pose_pairs_desc, bin_deg), FIELD(sr_pose_pairs_desc, hist), FIELD(sr_pose_pairs_desc, rot_err),
          FIELD(sr_pose_pairs_desc, trans_err)));
  STRUCT(sr_pose_align_desc,
         (FIELD(sr_pose_align_desc, pred), FIELD(sr_pose_align_desc, gt), FIELD(sr_pose_align_desc, pred_stride),
          FIELD(sr_pose_align_desc, gt_stride), FIELD(sr_pose_align_desc, n_views),
          FIELD(sr_pose_align_desc, with_scale), FIELD(sr_pose_align_desc, out), FIELD(sr_pose_align_desc, status),
          FIELD(sr_pose_align_desc, err)));
  std::printf("}\n");
}

void layout_imc_stats() {
  const char* sep = "";
  std::printf("{");
  STRUCT(sr_imc_stats_desc,
         (FIELD(sr_imc_stats_desc, residuals), FIELD(sr_imc_stats_desc, frame_pmf), FIELD(sr_imc_stats_desc, frame_cdf),
          FIELD(sr_imc_stats_desc, frame_pdf), FIELD(sr_imc_stats_desc, thresh), FIELD(sr_imc_stats_desc, n_thresh),
          FIELD(sr_imc_stats_desc, pair_counts), FIELD(sr_imc_stats_desc, pair_stats),
          FIELD(sr_imc_stats_desc, workspace), FIELD(sr_imc_stats_desc, workspace_floats)));
  std::printf("}\n");
}

void layout_cloud_eval() {
  const char* sep = "";
  std::printf("{");
  STRUCT(sr_cloud_nn_desc,
         (FIELD(sr_cloud_nn_desc, query), FIELD(sr_cloud_nn_desc, target), FIELD(sr_cloud_nn_desc, n_query),
          FIELD(sr_cloud_nn_desc, n_target), FIELD(sr_cloud_nn_desc, query_xform), FIELD(sr_cloud_nn_desc, target_xform),
          FIELD(sr_cloud_nn_desc, target_chunk), FIELD(sr_cloud_nn_desc, dist), FIELD(sr_cloud_nn_desc, index),
          FIELD(sr_cloud_nn_desc, n_bins), FIELD(sr_cloud_nn_desc, bin_len), FIELD(sr_cloud_nn_desc, hist),
          FIELD(sr_cloud_nn_desc, stats), FIELD(sr_cloud_nn_desc, workspace), FIELD(sr_cloud_nn_desc, workspace_bytes)));
  std::printf("}\n");
}

void layout_depth_eval() {
  const char* sep = "";
  std::printf("{");
  STRUCT(sr_select_desc,
         (FIELD(sr_select_desc, x), FIELD(sr_select_desc, mask), FIELD(sr_select_desc, group), FIELD(sr_select_desc, n_rows),
          FIELD(sr_select_desc, row_len), FIELD(sr_select_desc, row_stride), FIELD(sr_select_desc, n_groups),
          FIELD(sr_select_desc, n_ranks), FIELD(sr_select_desc, rank_num), FIELD(sr_select_desc, rank_den),
          FIELD(sr_select_desc, blocks_per_row), FIELD(sr_select_desc, value), FIELD(sr_select_desc, count),
          FIELD(sr_select_desc, workspace), FIELD(sr_select_desc, workspace_bytes)));
  STRUCT(sr_depth_eval_desc,
         (FIELD(sr_depth_eval_desc, pred), FIELD(sr_depth_eval_desc, gt), FIELD(sr_depth_eval_desc, mask),
          FIELD(sr_depth_eval_desc, conf), FIELD(sr_depth_eval_desc, conf_min), FIELD(sr_depth_eval_desc, group),
          FIELD(sr_depth_eval_desc, n_pix), FIELD(sr_depth_eval_desc, stride), FIELD(sr_depth_eval_desc, n_views),
          FIELD(sr_depth_eval_desc, n_groups), FIELD(sr_depth_eval_desc, gt_min), FIELD(sr_depth_eval_desc, gt_max),
          FIELD(sr_depth_eval_desc, align), FIELD(sr_depth_eval_desc, n_bins), FIELD(sr_depth_eval_desc, bin_len),
          FIELD(sr_depth_eval_desc, xform), FIELD(sr_depth_eval_desc, status), FIELD(sr_depth_eval_desc, stats),
          FIELD(sr_depth_eval_desc, hist), FIELD(sr_depth_eval_desc, aligned), FIELD(sr_depth_eval_desc, rel_err),
          FIELD(sr_depth_eval_desc, rel_q), FIELD(sr_depth_eval_desc, workspace), FIELD(sr_depth_eval_desc, workspace_bytes)));
  std::printf("}\n");
}

void layout_cloud_voxel() {
  const char* sep = "";
  std::printf("{");
  STRUCT(sr_sort_desc,
         (FIELD(sr_sort_desc, keys_in), FIELD(sr_sort_desc, vals_in), FIELD(sr_sort_desc, keys_out),
          FIELD(sr_sort_desc, vals_out), FIELD(sr_sort_desc, n), FIELD(sr_sort_desc, key_bits),
          FIELD(sr_sort_desc, workspace), FIELD(sr_sort_desc, workspace_bytes)));
  STRUCT(sr_cloud_voxel_desc,
         (FIELD(sr_cloud_voxel_desc, points), FIELD(sr_cloud_voxel_desc, attr), FIELD(sr_cloud_voxel_desc, mask),
          FIELD(sr_cloud_voxel_desc, weight), FIELD(sr_cloud_voxel_desc, xform), FIELD(sr_cloud_voxel_desc, n),
          FIELD(sr_cloud_voxel_desc, ldp), FIELD(sr_cloud_voxel_desc, lda), FIELD(sr_cloud_voxel_desc, n_attr),
          FIELD(sr_cloud_voxel_desc, axis_bits), FIELD(sr_cloud_voxel_desc, mode), FIELD(sr_cloud_voxel_desc, origin),
          FIELD(sr_cloud_voxel_desc, voxel), FIELD(sr_cloud_voxel_desc, capacity), FIELD(sr_cloud_voxel_desc, out_points),
          FIELD(sr_cloud_voxel_desc, out_attr), FIELD(sr_cloud_voxel_desc, out_count), FIELD(sr_cloud_voxel_desc, out_index),
          FIELD(sr_cloud_voxel_desc, out_key), FIELD(sr_cloud_voxel_desc, voxel_of), FIELD(sr_cloud_voxel_desc, counts),
          FIELD(sr_cloud_voxel_desc, workspace), FIELD(sr_cloud_voxel_desc, workspace_bytes)));
  std::printf("}\n");
}

void layout_sparsify() {
  const char* sep = "";
  std::printf("{");
  STRUCT(sr_sparsify_desc,
         (FIELD(sr_sparsify_desc, err), FIELD(sr_sparsify_desc, conf), FIELD(sr_sparsify_desc, mask),
          FIELD(sr_sparsify_desc, group), FIELD(sr_sparsify_desc, n_rows), FIELD(sr_sparsify_desc, row_len),
          FIELD(sr_sparsify_desc, row_stride), FIELD(sr_sparsify_desc, n_groups), FIELD(sr_sparsify_desc, n_steps),
          FIELD(sr_sparsify_desc, order), FIELD(sr_sparsify_desc, bin_sum), FIELD(sr_sparsify_desc, cut),
          FIELD(sr_sparsify_desc, count), FIELD(sr_sparsify_desc, workspace), FIELD(sr_sparsify_desc, workspace_bytes)));
  std::printf("}\n");
}

void layout_cloud_render() {
  const char* sep = "";
  std::printf("{");
  STRUCT(sr_cloud_render_desc,
         (FIELD(sr_cloud_render_desc, points), FIELD(sr_cloud_render_desc, attr), FIELD(sr_cloud_render_desc, mask),
          FIELD(sr_cloud_render_desc, view_id), FIELD(sr_cloud_render_desc, exclude), FIELD(sr_cloud_render_desc, xform),
          FIELD(sr_cloud_render_desc, extrinsic), FIELD(sr_cloud_render_desc, intrinsic), FIELD(sr_cloud_render_desc, n),
          FIELD(sr_cloud_render_desc, ldp), FIELD(sr_cloud_render_desc, lda), FIELD(sr_cloud_render_desc, n_attr),
          FIELD(sr_cloud_render_desc, n_views), FIELD(sr_cloud_render_desc, height), FIELD(sr_cloud_render_desc, width),
          FIELD(sr_cloud_render_desc, radius), FIELD(sr_cloud_render_desc, z_near), FIELD(sr_cloud_render_desc, z_far),
          FIELD(sr_cloud_render_desc, attr_fill), FIELD(sr_cloud_render_desc, depth), FIELD(sr_cloud_render_desc, index),
          FIELD(sr_cloud_render_desc, out_attr), FIELD(sr_cloud_render_desc, counts), FIELD(sr_cloud_render_desc, workspace),
          FIELD(sr_cloud_render_desc, workspace_bytes)));
  std::printf("}\n");
}

void layout_two_view() {
  const char* sep = "";
  std::printf("{");
  STRUCT(sr_two_view_desc,
         (FIELD(sr_two_view_desc, src_coords), FIELD(sr_two_view_desc, dst_coords), FIELD(sr_two_view_desc, mask),
          FIELD(sr_two_view_desc, intrinsic), FIELD(sr_two_view_desc, src_idx), FIELD(sr_two_view_desc, dst_idx),
          FIELD(sr_two_view_desc, given_E), FIELD(sr_two_view_desc, ref_extrinsic), FIELD(sr_two_view_desc, n_views),
          FIELD(sr_two_view_desc, n_pairs), FIELD(sr_two_view_desc, n_points), FIELD(sr_two_view_desc, n_given),
          FIELD(sr_two_view_desc, n_hyp), FIELD(sr_two_view_desc, refine_iters), FIELD(sr_two_view_desc, threshold_px),
          FIELD(sr_two_view_desc, seed), FIELD(sr_two_view_desc, E), FIELD(sr_two_view_desc, R),
          FIELD(sr_two_view_desc, t), FIELD(sr_two_view_desc, cost), FIELD(sr_two_view_desc, n_inliers),
          FIELD(sr_two_view_desc, n_front), FIELD(sr_two_view_desc, best), FIELD(sr_two_view_desc, refined),
          FIELD(sr_two_view_desc, status), FIELD(sr_two_view_desc, inlier_mask), FIELD(sr_two_view_desc, pose_err),
          FIELD(sr_two_view_desc, hyp_idx), FIELD(sr_two_view_desc, hyp_E), FIELD(sr_two_view_desc, hyp_cost),
          FIELD(sr_two_view_desc, hyp_inliers), FIELD(sr_two_view_desc, workspace), FIELD(sr_two_view_desc, workspace_bytes)));
  std::printf("}\n");
}

sr_attn_desc attn(int batch, int heads, int lq, int l0, int l1) {
  sr_attn_desc d;
  std::memset(&d, 0, sizeof(d));
  d.q = fake(1);
  d.k0 = fake(2);
  d.v0 = fake(3);
  d.o = fake(4);
  d.ldq = d.ldk0 = d.ldv0 = d.ldo = heads * 64 * 3;
  d.batch = batch;
  d.heads = heads;
  d.head_dim = 64;
  d.lq = lq;
  d.q_bstride = lq;
  d.l0 = l0;
  d.l1 = l1;
  if (l1) {
    d.k1 = fake(5);
    d.v1 = fake(6);
    d.ldk1 = d.ldv1 = d.ldk0;
    d.k1_bstride = l1;
  }
  d.scale = 0.125f;
  return d;
}

void check() {
  // ---- tuning table and strings
  if (sr_version() < (1 << 16)) ++g_fail;
  for (int k = 0; k < SR_TUNE_COUNT; ++k) {
    const char* n = sr_tuning_name(k);
    const int v = sr_get_tuning(k);
    if (!n || sr_set_tuning(k, v + 1) != v || sr_get_tuning(k) != v + 1 || sr_set_tuning(k, v) != v + 1) ++g_fail;
  }
  if (sr_tuning_name(SR_TUNE_COUNT) || sr_set_tuning(SR_TUNE_COUNT, 0) != SR_EINVAL || sr_get_tuning(-1) != SR_EINVAL)
    ++g_fail;
  std::printf("tuning table: %d switches\n", (int)SR_TUNE_COUNT);

  sr_gemm_epi ep;
  std::memset(&ep, 0, sizeof(ep));
  // ---- GEMM: rejected shapes, then the planned paths of every epilogue / size class
  expect("sr_gemm null A", sr_gemm(nullptr, SR_BF16, SR_EPI_BIAS, nullptr, 64, fake(1), 64, fake(2), 64, 8, 64, 64, &ep), false);
  expect("sr_gemm N % 4", sr_gemm(nullptr, SR_BF16, SR_EPI_BIAS, fake(0), 64, fake(1), 64, fake(2), 66, 8, 66, 64, &ep), false);
  expect("sr_gemm K % 64", sr_gemm(nullptr, SR_BF16, SR_EPI_BIAS, fake(0), 96, fake(1), 96, fake(2), 64, 8, 64, 96, &ep), false);
  expect("sr_gemm RESID without gamma", sr_gemm(nullptr, SR_BF16, SR_EPI_BIAS_RESID, fake(0), 64, fake(1), 64, fake(2), 64, 8, 64, 64, &ep), false);
  expect("sr_gemm bad epilogue", sr_gemm(nullptr, SR_BF16, 42, fake(0), 64, fake(1), 64, fake(2), 64, 8, 64, 64, &ep), true);
  ep.gamma = fake<float>(9);
  const int Ms[] = {1, 64, 300, 87936};
  const int Ns[] = {256, 1024, 3072, 4096};
  for (int M : Ms)
    for (int N : Ns)
      for (int epi : {SR_EPI_BIAS, SR_EPI_BIAS_GELU, SR_EPI_BIAS_RESID, SR_EPI_F32}) {
        char what[96];
        std::snprintf(what, sizeof(what), "sr_gemm bf16 epi %d M %d N %d", epi, M, N);
        expect(what, sr_gemm(nullptr, SR_BF16, epi, fake(0), 1024, fake(1), 1024, fake(2), N, M, N, 1024, &ep), true);
        std::snprintf(what, sizeof(what), "sr_gemm f32 epi %d M %d N %d", epi, M, N);
        expect(what, sr_gemm(nullptr, SR_F32, epi, fake(0), 1024, fake(1), 1024, fake(2), N, M, N, 1024, &ep), true);
      }
  ep.q_scale = 0.18f;  // ABI 1.0: the Q block of a BIAS / QKV output leaves scaled
  ep.q_cols = 1024;
  expect("sr_gemm BIAS q_scale", sr_gemm(nullptr, SR_BF16, SR_EPI_BIAS, fake(0), 1024, fake(1), 1024, fake(2), 3072, 87936, 3072, 1024, &ep), true);
  expect("sr_gemm RESID q_scale", sr_gemm(nullptr, SR_BF16, SR_EPI_BIAS_RESID, fake(0), 1024, fake(1), 1024, fake(2), 3072, 87936, 3072, 1024, &ep), false);
  ep.q_cols = 100;
  expect("sr_gemm q_cols not a multiple of 64", sr_gemm(nullptr, SR_BF16, SR_EPI_BIAS, fake(0), 1024, fake(1), 1024, fake(2), 3072, 87936, 3072, 1024, &ep), false);
  ep.q_scale = 0.f;
  ep.q_cols = 0;
  expect("sr_gemm_splitk 3 slices of 16 tiles", sr_gemm_splitk(nullptr, SR_BF16, SR_EPI_BIAS, fake(0), 1024, fake(1), 1024, fake(2), 1024, 64, 1024, 1024, 3, fake<float>(3), &ep), false);
  expect("sr_gemm_splitk 4 slices", sr_gemm_splitk(nullptr, SR_BF16, SR_EPI_BIAS, fake(0), 1024, fake(1), 1024, fake(2), 1024, 64, 1024, 1024, 4, fake<float>(3), &ep), true);
  std::vector<sr_gemm_problem> pr(5);
  for (auto& p : pr) {
    std::memset(&p, 0, sizeof(p));
    p.A = fake(0);
    p.W = fake(1);
    p.out = fake(2);
    p.lda = p.ldw = 1024;
    p.ldo = 3072;
    p.M = 43968;
    p.N = 3072;
    p.K = 1024;
    p.ep = ep;
  }
  expect("sr_gemm_group 5 problems", sr_gemm_group(nullptr, SR_BF16, SR_EPI_BIAS, 5, pr.data()), false);
  expect("sr_gemm_group 3 problems", sr_gemm_group(nullptr, SR_BF16, SR_EPI_BIAS, 3, pr.data()), true);
  pr[1].N = 1000;
  pr[1].ldo = 1000;
  expect("sr_gemm_group N % 256", sr_gemm_group(nullptr, SR_BF16, SR_EPI_BIAS, 3, pr.data()), false);

  // ---- attention: every dispatch class of the bf16 and f32 paths
  sr_attn_desc d = attn(1, 16, 43968, 43968, 0);
  expect("sr_attention null desc", sr_attention(nullptr, SR_BF16, nullptr), false);
  d.k0 = nullptr;
  expect("sr_attention null k0", sr_attention(nullptr, SR_BF16, &d), false);
  d = attn(1, 16, 43968, 43968, 0);
  d.head_dim = 128;
  expect("sr_attention bf16 head_dim 128", sr_attention(nullptr, SR_BF16, &d), false);
  d = attn(1, 16, 43968, 43968, 0);
  d.key_norm_max = 40.f;
  expect("sr_attention global (asm sweep)", sr_attention(nullptr, SR_BF16, &d), true);
  d.key_norm_max = 0.f;
  d.key_bound = fake<float>(7);
  expect("sr_attention global, key scan", sr_attention(nullptr, SR_BF16, &d), true);
  // ABI 1.0: the caller-filled norms have their own field; boxes need a bound and 16-B alignment
  d = attn(1, 16, 43968, 43968, 0);
  d.key_norm_max = 40.f;
  d.key_norm2 = fake<float>(10);
  d.key_box = fake<float>(11);
  d.value_box = fake<float>(12);
  d.q_scaled = 1;
  expect("sr_attention global, key_norm2 + boxes + q_scaled", sr_attention(nullptr, SR_BF16, &d), true);
  d.key_box = (const float*)((const char*)fake<float>(11) + 4);
  expect("sr_attention misaligned key_box", sr_attention(nullptr, SR_BF16, &d), false);
  d.key_box = fake<float>(11);
  d.key_norm_max = 0.f;
  d.key_norm2 = nullptr;
  expect("sr_attention boxes without a bound", sr_attention(nullptr, SR_BF16, &d), false);
  d = attn(4, 16, 300, 300, 0);
  d.q_scaled = 1;
  expect("sr_attention f32 q_scaled", sr_attention(nullptr, SR_F32, &d), false);
  d.q_scaled = 2;
  expect("sr_attention bf16 q_scaled 2", sr_attention(nullptr, SR_BF16, &d), false);
  d = attn(64, 16, 1374, 1374, 0);
  d.k0_bstride = 1374;
  expect("sr_attention frame", sr_attention(nullptr, SR_BF16, &d), true);
  d = attn(32, 16, 1374, 9760, 1374);
  d.tail_rows_readable = 64;
  expect("sr_attention reloc (two segments)", sr_attention(nullptr, SR_BF16, &d), true);
  d.merge_o = fake(8);
  d.merge_lse = fake<float>(9);
  d.merge_rows = 32 * 1374;
  d.ld_merge_o = 1024;
  expect("sr_attention reloc merge-in", sr_attention(nullptr, SR_BF16, &d), true);
  d.merge_rows = 0;
  expect("sr_attention merge-in without rows", sr_attention(nullptr, SR_BF16, &d), false);
  d = attn(4, 16, 300, 300, 0);
  expect("sr_attention f32 short", sr_attention(nullptr, SR_F32, &d), true);
  d = attn(1, 16, 64, 64, 0);
  d.head_dim = 128;
  d.mask_mode = SR_MASK_CAMERA;
  d.n_anchor = 32;
  expect("sr_attention f32 camera mask", sr_attention(nullptr, SR_F32, &d), true);
  d.mask_mode = SR_MASK_DENSE;
  expect("sr_attention dense mask without mask", sr_attention(nullptr, SR_F32, &d), false);
  d.mask_mode = 7;
  expect("sr_attention bad mask mode", sr_attention(nullptr, SR_F32, &d), false);
  sr_attn_desc a = attn(1, 16, 43968, 43968, 0), b = attn(1, 16, 43968, 9728, 0);
  a.key_norm_max = b.key_norm_max = 40.f;
  expect("sr_attention_pair", sr_attention_pair(nullptr, SR_BF16, &a, &b), true);
  expect("sr_attention_pair_vt null tiles", sr_attention_pair_vt(nullptr, SR_BF16, &a, &b, fake(0), nullptr), false);
  expect("sr_vt_tiles null", sr_vt_tiles(nullptr, nullptr, 3072, 64, 16, nullptr), false);
  b.l0 = 9760;
  expect("sr_attention_pair ragged keys", sr_attention_pair(nullptr, SR_BF16, &a, &b), false);
  b = attn(1, 8, 43968, 9728, 0);
  b.key_norm_max = 40.f;
  expect("sr_attention_pair head counts", sr_attention_pair(nullptr, SR_BF16, &a, &b), false);
  // ---- few query rows, key-split (ABI 1.7): rejections, then the chunk plan of the C3 camera-row
  // shapes and of ragged / two-segment / many-item ones (the launch itself fails without a device)
  expect("sr_attention_rows null desc", sr_attention_rows(nullptr, SR_BF16, nullptr, fake(20), 1 << 30), false);
  d = attn(1, 16, 65, 43968, 0);
  expect("sr_attention_rows 65 rows", sr_attention_rows(nullptr, SR_BF16, &d, fake(20), 1 << 30), false);
  if (sr_attention_rows_chunks(&d) != 0 || sr_attention_rows_workspace(&d) != 0) ++g_fail;
  d = attn(1, 16, 32, 43968, 0);
  d.head_dim = 128;
  expect("sr_attention_rows head_dim 128", sr_attention_rows(nullptr, SR_BF16, &d, fake(20), 1 << 30), false);
  d.head_dim = 64;
  expect("sr_attention_rows f32", sr_attention_rows(nullptr, SR_F32, &d, fake(20), 1 << 30), false);
  d.mask_mode = SR_MASK_CAMERA;
  expect("sr_attention_rows mask", sr_attention_rows(nullptr, SR_BF16, &d, fake(20), 1 << 30), false);
  d.mask_mode = SR_MASK_NONE;
  d.merge_o = fake(8);
  expect("sr_attention_rows merge_o", sr_attention_rows(nullptr, SR_BF16, &d, fake(20), 1 << 30), false);
  d.merge_o = nullptr;
  d.ldq = 3076;
  expect("sr_attention_rows ldq % 8", sr_attention_rows(nullptr, SR_BF16, &d, fake(20), 1 << 30), false);
  d.ldq = 1374 * 3072;  // camera rows read in place: one row per frame of a packed q|k|v buffer
  d.k1 = (const char*)fake(5) + 2;  // a stale, unaligned segment-1 pointer is ignored while l1 == 0 ...
  expect("sr_attention_rows stale k1 with l1 = 0", sr_attention_rows(nullptr, SR_BF16, &d, fake(20), 1 << 30), true);
  d.v1 = fake(6);
  d.ldk1 = d.ldv1 = d.ldk0;
  d.l1 = 64;                        // ... and rejected once the segment is used
  expect("sr_attention_rows unaligned k1", sr_attention_rows(nullptr, SR_BF16, &d, fake(20), 1 << 30), false);
  d.l1 = 0;
  d.k1 = d.v1 = nullptr;
  expect("sr_attention_rows workspace too small",
         sr_attention_rows(nullptr, SR_BF16, &d, fake(20), sr_attention_rows_workspace(&d) - 1), false);
  expect("sr_attention_rows null workspace", sr_attention_rows(nullptr, SR_BF16, &d, nullptr, 1 << 30), false);
  {
    struct { int batch, heads, lq, l0, l1, chunks; } cases[] = {
        {1, 16, 32, 43968, 0, 128}, {1, 16, 32, 9760, 0, 38}, {32, 16, 1, 1374, 0, 4}, {1, 16, 64, 4100, 0, 16},
        {3, 6, 33, 1000, 64, 4},    {1, 1, 1, 1, 0, 1},       {3, 1, 2, 63, 21, 1},    {64, 16, 1, 1 << 20, 1 << 20, 2}};
    for (const auto& c : cases) {
      d = attn(c.batch, c.heads, c.lq, c.l0, c.l1);
      const int n = sr_attention_rows_chunks(&d);
      const int64_t ws = sr_attention_rows_workspace(&d);
      std::printf("sr_attention_rows plan batch %d heads %d lq %d keys %d + %d: %d chunks, %lld workspace bytes\n", c.batch,
                  c.heads, c.lq, c.l0, c.l1, n, (long long)ws);
      if (n != c.chunks || ws != (int64_t)c.batch * c.heads * n * c.lq * 66 * 4) ++g_fail;
      expect("sr_attention_rows launch", sr_attention_rows(nullptr, SR_BF16, &d, fake(20), ws), true);
    }
  }
  d = attn(1, 16, 43968, 43968, 0);
  std::printf("bound floats: %d\n", sr_attention_bound_floats(&d));
  std::printf("key box scratch floats: %d\n", sr_attention_key_box_scratch(43968, 1, 16));
  expect("sr_attention_key_box", sr_attention_key_box(nullptr, fake(0), 3072, 43968, 0, 1, 16, fake<float>(1),
                                                      fake<float>(2), fake<float>(3)), true);
  expect("sr_attention_key_box null scratch", sr_attention_key_box(nullptr, fake(0), 3072, 43968, 0, 1, 16,
                                                                   fake<float>(1), nullptr, nullptr), false);
  expect("sr_attention_key_box 33 heads", sr_attention_key_box(nullptr, fake(0), 3072, 100, 0, 1, 33, fake<float>(1),
                                                               nullptr, fake<float>(3)), false);
  expect("sr_attention_key_box overlapping instances", sr_attention_key_box(nullptr, fake(0), 1024, 1374, 1000, 64,
                                                                             16, fake<float>(1), nullptr,
                                                                             fake<float>(3)), false);

  // ---- merges
  const int seg[SR_ATTN_MERGE_MAX_PARTS] = {43968, 1374};
  expect("sr_attn_merge_n", sr_attn_merge_n(nullptr, SR_BF16, 2, 43968, 16, 64, fake(0), 1024, 43968, fake<float>(1), seg, fake(2), 1024, nullptr), true);
  expect("sr_attn_merge_n 17 parts", sr_attn_merge_n(nullptr, SR_BF16, 17, 43968, 16, 64, fake(0), 1024, 43968, fake<float>(1), nullptr, fake(2), 1024, nullptr), false);
  const int bad_seg[SR_ATTN_MERGE_MAX_PARTS] = {43968, 1000};
  expect("sr_attn_merge_n seg rows", sr_attn_merge_n(nullptr, SR_BF16, 2, 43968, 16, 64, fake(0), 1024, 43968, fake<float>(1), bad_seg, fake(2), 1024, nullptr), false);
  expect("sr_attn_merge", sr_attn_merge(nullptr, SR_BF16, 100, 16, 64, fake(0), 1024, fake<float>(1), fake(2), 1024, fake<float>(3), fake(4), 1024, nullptr), true);

  // ---- the rest of the ABI: null / empty arguments are rejected, never dereferenced
  expect("sr_layernorm null", sr_layernorm(nullptr, SR_BF16, nullptr, 1024, nullptr, nullptr, nullptr, 1e-5f, nullptr, 1024, 0, 1024), false);
  expect("sr_layernorm", sr_layernorm(nullptr, SR_BF16, fake<float>(0), 1024, nullptr, fake<float>(1), fake<float>(2), 1e-5f, fake(3), 1024, 87936, 1024), true);
  expect("sr_quant_fp8 null", sr_quant_fp8(nullptr, nullptr, 8, 8, 8, 1.f, nullptr, 8, nullptr, nullptr), false);
  expect("sr_attention_qk8 null", sr_attention_qk8(nullptr, nullptr, nullptr, 0, nullptr, 0, nullptr), false);
  expect("sr_attention_qkv8 null", sr_attention_qkv8(nullptr, nullptr, nullptr, 0, nullptr, 0, nullptr, nullptr), false);
  expect("sr_colsum_fma no pair", sr_colsum_fma(nullptr, SR_F32, fake(0), 8, 8, 8, nullptr, nullptr, nullptr, nullptr,
                                                   fake<float>(1), 1 << 20), false);
  expect("sr_vec_fma2_f32 null", sr_vec_fma2_f32(nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 8), false);
  expect("sr_quant_fp8_vt null", sr_quant_fp8_vt(nullptr, nullptr, 8, 8, 1, nullptr, nullptr, nullptr), false);
  expect("sr_attention_bwd null", sr_attention_bwd(nullptr, nullptr), false);
  expect("sr_attention_bwd_f32 null", sr_attention_bwd_f32(nullptr, nullptr), false);
  if (sr_qk_bwd_workspace_floats(43968, 3072) < 1024LL * 3072 || sr_qk_bwd_workspace_floats(0, 3072) != 0) ++g_fail;
  expect("sr_gemm_wgrad null", sr_gemm_wgrad(nullptr, nullptr, 0, nullptr, 0, nullptr, 0, 0, 0, 0, 0, nullptr, nullptr, 0, nullptr, 0, nullptr), false);
  expect("sr_colsum null", sr_colsum(nullptr, SR_F32, nullptr, 0, 0, 0, nullptr, 0, 1.f, nullptr, 0), false);
  {  // ABI 1.0: the workspace size is checked against sr_colsum_workspace_floats
    const int64_t need = sr_colsum_workspace_floats(87936, 1024);
    if (need <= 0 || need > 1024LL * 1024) ++g_fail;
    expect("sr_colsum workspace one float short",
           sr_colsum(nullptr, SR_F32, fake(1), 1024, 87936, 1024, fake<float>(2), 0, 1.f, fake<float>(3), need - 1), false);
    expect("sr_colsum sized workspace",
           sr_colsum(nullptr, SR_F32, fake(1), 1024, 87936, 1024, fake<float>(2), 0, 1.f, fake<float>(3), need), true);
  }
  expect("sr_imc_loss null", sr_imc_loss(nullptr, nullptr), false);
  std::printf("imc workspace floats: %lld\n", (long long)sr_imc_loss_workspace(4, 3, 1024, 1, 100));
  {  // the sizes its fixed arrays hold (kr[64] / gKr[64], raw[1024], one reflection) are refused before any launch
    sr_imc_loss_desc ld{};
    ld.enc = fake<float>(0), ld.kp2k = fake<float>(1), ld.src_coords = fake<float>(2), ld.dst_coords = fake<float>(3);
    ld.src_depth = fake<float>(4), ld.dst_depth = fake<float>(5), ld.smooth_w = fake<float>(6);
    ld.src_idx = fake<int32_t>(7), ld.dst_idx = fake<int32_t>(8), ld.node_src = fake<int32_t>(9);
    ld.node_dst = fake<int32_t>(10), ld.loss = fake<float>(11), ld.d_enc = fake<float>(12), ld.workspace = fake<float>(13);
    ld.n_views = 64, ld.H = 392, ld.W = 518, ld.n_pairs = 70, ld.n_points = 130, ld.n_nodes = 64;
    ld.min_val = 0.f, ld.max_val = 15.f, ld.num_bins = 1024, ld.smooth_radius = 13, ld.grad_scale = 1.f;
    expect("sr_imc_loss 64 views 1024 bins", sr_imc_loss(nullptr, &ld), true);
    sr_imc_loss_desc b = ld;
    b.n_views = 65;
    expect("sr_imc_loss 65 views", sr_imc_loss(nullptr, &b), false);
    b = ld, b.num_bins = 1025;
    expect("sr_imc_loss 1025 bins", sr_imc_loss(nullptr, &b), false);
    b = ld, b.num_bins = 2, b.smooth_radius = 0;
    expect("sr_imc_loss 2 bins", sr_imc_loss(nullptr, &b), false);
    b = ld, b.num_bins = 3, b.smooth_radius = 2;
    expect("sr_imc_loss 5 taps over 3 bins", sr_imc_loss(nullptr, &b), false);
    b = ld, b.node_src = nullptr;
    expect("sr_imc_loss null node_src", sr_imc_loss(nullptr, &b), false);
    b = ld, b.max_val = 0.f;
    expect("sr_imc_loss empty range", sr_imc_loss(nullptr, &b), false);

    // ABI 1.10: the same geometry with the loss's own outputs absent, and every rejection the header lists
    sr_imc_loss_desc g = ld;
    g.loss = nullptr, g.d_enc = nullptr, g.workspace = nullptr, g.n_points = 10000;
    const int64_t need = sr_imc_stats_workspace(g.n_views, g.n_pairs, g.n_points, g.n_nodes, g.num_bins);
    std::printf("imc stats workspace floats: %lld\n", (long long)need);
    if (need < 4LL * 70 * 10000 || sr_imc_stats_workspace(0, 70, 10000, 64, 1024) != 0 ||
        sr_imc_stats_workspace(64, 70, 0, 64, 1024) != 0)
      ++g_fail;
    sr_imc_stats_desc sd{};
    sd.residuals = fake<float>(14), sd.frame_pmf = fake<float>(15), sd.frame_cdf = fake<float>(16);
    sd.frame_pdf = fake<float>(17), sd.thresh = fake<float>(18), sd.n_thresh = 8, sd.pair_counts = fake<uint32_t>(19);
    sd.pair_stats = fake<float>(20), sd.workspace = fake<float>(21), sd.workspace_floats = need;
    expect("sr_imc_residual_stats every output", sr_imc_residual_stats(nullptr, &g, &sd), true);
    sr_imc_stats_desc c{};
    c.pair_stats = fake<float>(20), c.workspace = fake<float>(21), c.workspace_floats = need;
    expect("sr_imc_residual_stats pair_stats only", sr_imc_residual_stats(nullptr, &g, &c), true);
    expect("sr_imc_residual_stats null g", sr_imc_residual_stats(nullptr, nullptr, &sd), false);
    expect("sr_imc_residual_stats null s", sr_imc_residual_stats(nullptr, &g, nullptr), false);
    c = sd, c.n_thresh = 9;
    expect("sr_imc_residual_stats 9 thresholds", sr_imc_residual_stats(nullptr, &g, &c), false);
    c = sd, c.n_thresh = -1;
    expect("sr_imc_residual_stats -1 thresholds", sr_imc_residual_stats(nullptr, &g, &c), false);
    c = sd, c.thresh = nullptr;
    expect("sr_imc_residual_stats null thresh", sr_imc_residual_stats(nullptr, &g, &c), false);
    c = sd, c.pair_counts = nullptr;
    expect("sr_imc_residual_stats thresholds without counts", sr_imc_residual_stats(nullptr, &g, &c), false);
    c = sd, c.workspace = nullptr;
    expect("sr_imc_residual_stats null workspace", sr_imc_residual_stats(nullptr, &g, &c), false);
    c = sd, c.workspace_floats = need - 1;
    expect("sr_imc_residual_stats workspace one float short", sr_imc_residual_stats(nullptr, &g, &c), false);
    c = sr_imc_stats_desc{}, c.workspace = fake<float>(21), c.workspace_floats = need;
    expect("sr_imc_residual_stats every output NULL", sr_imc_residual_stats(nullptr, &g, &c), false);
    b = g, b.n_views = 65;
    expect("sr_imc_residual_stats 65 views", sr_imc_residual_stats(nullptr, &b, &sd), false);
    b = g, b.num_bins = 1025;
    expect("sr_imc_residual_stats 1025 bins", sr_imc_residual_stats(nullptr, &b, &sd), false);
    b = g, b.n_points = 0;
    expect("sr_imc_residual_stats 0 points", sr_imc_residual_stats(nullptr, &b, &sd), false);
    b = g, b.dst_coords = nullptr;
    expect("sr_imc_residual_stats null dst_coords", sr_imc_residual_stats(nullptr, &b, &sd), false);
    b = g, b.n_pairs = 65536;
    c = sd, c.workspace_floats = sr_imc_stats_workspace(b.n_views, b.n_pairs, b.n_points, b.n_nodes, b.num_bins);
    expect("sr_imc_residual_stats 65536 pairs", sr_imc_residual_stats(nullptr, &b, &c), false);
  }
  expect("sr_corres_sample null", sr_corres_sample(nullptr, nullptr), false);
  {  // ABI 1.6: null pointers, empty sizes and an undersized workspace are refused before any launch
    const int64_t need = sr_corres_sample_workspace(240, 313600);
    if (need < 240LL * 313600 || sr_corres_sample_workspace(0, 100) != 0 || sr_corres_sample_workspace(3, 0) != 0) ++g_fail;
    std::printf("corres workspace doubles: %lld\n", (long long)need);
    sr_corres_desc cd{};
    cd.n_pairs = 240, cd.n_points = 10000, cd.max_m = 313600, cd.min_conf = 0.1f;
    cd.pairs = fake<sr_corres_pair>(0), cd.uniforms = fake<double>(1);
    cd.src_coords = fake<float>(2), cd.dst_coords = fake<float>(3), cd.src_depth = fake<float>(4), cd.dst_depth = fake<float>(5);
    cd.total = fake<double>(6), cd.n_valid = fake<int32_t>(7), cd.workspace = fake<double>(8), cd.workspace_doubles = need;
    expect("sr_corres_sample 240 pairs, no index", sr_corres_sample(nullptr, &cd), true);
    sr_corres_desc b = cd;
    b.workspace_doubles = need - 1;
    expect("sr_corres_sample workspace one double short", sr_corres_sample(nullptr, &b), false);
    b = cd, b.n_points = 0;
    expect("sr_corres_sample 0 points", sr_corres_sample(nullptr, &b), false);
    b = cd, b.n_pairs = 0;
    expect("sr_corres_sample 0 pairs", sr_corres_sample(nullptr, &b), false);
    b = cd, b.max_m = 0;
    expect("sr_corres_sample max_m 0", sr_corres_sample(nullptr, &b), false);
    b = cd, b.pairs = nullptr;
    expect("sr_corres_sample null table", sr_corres_sample(nullptr, &b), false);
    b = cd, b.uniforms = nullptr;
    expect("sr_corres_sample null uniforms", sr_corres_sample(nullptr, &b), false);
    b = cd, b.total = nullptr;
    expect("sr_corres_sample null total", sr_corres_sample(nullptr, &b), false);
    b = cd, b.dst_depth = nullptr;
    expect("sr_corres_sample null output", sr_corres_sample(nullptr, &b), false);
    b = cd, b.workspace = nullptr;
    expect("sr_corres_sample null workspace", sr_corres_sample(nullptr, &b), false);
    b = cd, b.n_pairs = 70000, b.workspace_doubles = sr_corres_sample_workspace(70000, 313600);
    expect("sr_corres_sample 70000 pairs", sr_corres_sample(nullptr, &b), false);
  }
  expect("sr_pose_pair_errors null", sr_pose_pair_errors(nullptr, nullptr), false);
  expect("sr_pose_align null", sr_pose_align(nullptr, nullptr), false);
  {  // ABI 1.9: every rejection the header lists, then the two pair sets and both strides up to the launch
    sr_pose_pairs_desc pd{};
    pd.pred = fake<float>(0), pd.gt = fake<float>(1), pd.pred_stride = 12, pd.gt_stride = 16, pd.n_views = 4096;
    pd.trans_ambiguity = 1, pd.n_bins = 180, pd.bin_deg = 1.f, pd.hist = fake<uint32_t>(2);
    expect("sr_pose_pair_errors all pairs, histogram only", sr_pose_pair_errors(nullptr, &pd), true);
    sr_pose_pairs_desc b = pd;
    b.rot_err = fake<float>(3), b.trans_err = fake<float>(4), b.n_views = 65535, b.n_bins = 1024;
    expect("sr_pose_pair_errors 65535 views, 1024 bins", sr_pose_pair_errors(nullptr, &b), true);
    b = pd, b.pair_i = fake<int32_t>(5), b.pair_j = fake<int32_t>(6), b.n_pairs = 2147483647;
    expect("sr_pose_pair_errors list of 2^31 - 1", sr_pose_pair_errors(nullptr, &b), true);
    b.n_pairs = 0;
    expect("sr_pose_pair_errors empty list", sr_pose_pair_errors(nullptr, &b), false);
    b = pd, b.pair_i = fake<int32_t>(5), b.n_pairs = 7;
    expect("sr_pose_pair_errors pair_i without pair_j", sr_pose_pair_errors(nullptr, &b), false);
    b = pd, b.pair_j = fake<int32_t>(6), b.n_pairs = 7;
    expect("sr_pose_pair_errors pair_j without pair_i", sr_pose_pair_errors(nullptr, &b), false);
    b = pd, b.pred = nullptr;
    expect("sr_pose_pair_errors null pred", sr_pose_pair_errors(nullptr, &b), false);
    b = pd, b.gt = nullptr;
    expect("sr_pose_pair_errors null gt", sr_pose_pair_errors(nullptr, &b), false);
    b = pd, b.hist = nullptr;
    expect("sr_pose_pair_errors null hist", sr_pose_pair_errors(nullptr, &b), false);
    b = pd, b.n_views = 0;
    expect("sr_pose_pair_errors 0 views", sr_pose_pair_errors(nullptr, &b), false);
    b = pd, b.n_views = 65536;
    expect("sr_pose_pair_errors 65536 views", sr_pose_pair_errors(nullptr, &b), false);
    b = pd, b.pred_stride = 9;
    expect("sr_pose_pair_errors stride 9", sr_pose_pair_errors(nullptr, &b), false);
    b = pd, b.gt_stride = 0;
    expect("sr_pose_pair_errors stride 0", sr_pose_pair_errors(nullptr, &b), false);
    b = pd, b.n_bins = 0;
    expect("sr_pose_pair_errors 0 bins", sr_pose_pair_errors(nullptr, &b), false);
    b = pd, b.n_bins = 1025;
    expect("sr_pose_pair_errors 1025 bins", sr_pose_pair_errors(nullptr, &b), false);
    b = pd, b.bin_deg = 0.f;
    expect("sr_pose_pair_errors bin_deg 0", sr_pose_pair_errors(nullptr, &b), false);
    b = pd, b.bin_deg = -1.f;
    expect("sr_pose_pair_errors bin_deg -1", sr_pose_pair_errors(nullptr, &b), false);
    const uint32_t nan_bits = 0x7fc00000u;
    b = pd, std::memcpy(&b.bin_deg, &nan_bits, sizeof(nan_bits));
    expect("sr_pose_pair_errors bin_deg NaN", sr_pose_pair_errors(nullptr, &b), false);

    sr_pose_align_desc ad{};
    ad.pred = fake<float>(0), ad.gt = fake<float>(1), ad.pred_stride = 16, ad.gt_stride = 12, ad.n_views = 65535;
    ad.with_scale = 1, ad.out = fake<double>(2), ad.status = fake<int32_t>(3);
    expect("sr_pose_align 65535 views", sr_pose_align(nullptr, &ad), true);
    sr_pose_align_desc c = ad;
    c.err = fake<double>(4), c.n_views = 1, c.with_scale = 0;
    expect("sr_pose_align one view, per-view errors", sr_pose_align(nullptr, &c), true);
    c = ad, c.pred = nullptr;
    expect("sr_pose_align null pred", sr_pose_align(nullptr, &c), false);
    c = ad, c.gt = nullptr;
    expect("sr_pose_align null gt", sr_pose_align(nullptr, &c), false);
    c = ad, c.out = nullptr;
    expect("sr_pose_align null out", sr_pose_align(nullptr, &c), false);
    c = ad, c.status = nullptr;
    expect("sr_pose_align null status", sr_pose_align(nullptr, &c), false);
    c = ad, c.n_views = 0;
    expect("sr_pose_align 0 views", sr_pose_align(nullptr, &c), false);
    c = ad, c.n_views = 65536;
    expect("sr_pose_align 65536 views", sr_pose_align(nullptr, &c), false);
    c = ad, c.gt_stride = 13;
    expect("sr_pose_align stride 13", sr_pose_align(nullptr, &c), false);
    c = ad, c.out = (double*)((char*)fake(2) + 4);
    expect("sr_pose_align out % 8", sr_pose_align(nullptr, &c), false);
  }
  expect("sr_cloud_nn null", sr_cloud_nn(nullptr, nullptr), false);
  {  // ABI 1.11: every rejection the header lists, then the planned shapes up to the launch
    const int64_t nq = 8600000, nt = 8600000;
    const int64_t need = sr_cloud_nn_workspace(nq, nt, 0, 1);
    std::printf("cloud workspace bytes: %lld\n", (long long)need);
    if (need < 16 * nt + 8 * nq || sr_cloud_nn_workspace(0, nt, 0, 0) != 0 || sr_cloud_nn_workspace(nq, 0, 0, 0) != 0 ||
        sr_cloud_nn_workspace(int64_t(1) << 31, nt, 0, 0) != 0 || sr_cloud_nn_workspace(nq, int64_t(1) << 31, 0, 0) != 0 ||
        sr_cloud_nn_workspace(nq, nt, -64, 0) != 0 || sr_cloud_nn_workspace(nq, nt, 100, 0) != 0 ||
        sr_cloud_nn_workspace(nq, nt, 64, 0) != 0 || sr_cloud_nn_workspace(nq, nt, 0, 0) != need)
      ++g_fail;
    {  // the size never shrinks when a count grows, nor when an explicit chunk shrinks
      const int64_t ns[] = {1, 63, 1024, 1025, 4096, 1 << 20, (1 << 20) + 1, 8600000, 2147483647LL};
      for (int chunk : {0, 65536, 1 << 20})
        for (int64_t fixed : ns) {
          int64_t prev_q = 0, prev_t = 0;
          for (int64_t n : ns) {
            const int64_t wq = sr_cloud_nn_workspace(n, fixed, chunk, 0), wt = sr_cloud_nn_workspace(fixed, n, chunk, 0);
            if (wq < prev_q || wt < prev_t || wq <= 0 || wt <= 0) ++g_fail;
            prev_q = wq, prev_t = wt;
          }
        }
      if (sr_cloud_nn_workspace(4096, 1 << 20, 128, 0) < sr_cloud_nn_workspace(4096, 1 << 20, 256, 0)) ++g_fail;
    }
    sr_cloud_nn_desc cd{};
    cd.query = fake<float>(0), cd.target = fake<float>(1), cd.n_query = nq, cd.n_target = nt;
    cd.query_xform = fake<double>(2), cd.dist = fake<float>(3), cd.index = fake<int32_t>(4), cd.n_bins = 1024;
    cd.bin_len = 0.01f, cd.hist = fake<uint32_t>(5), cd.stats = fake<double>(6), cd.workspace = fake(7);
    cd.workspace_bytes = need;
    expect("sr_cloud_nn 8.6 M x 8.6 M, every output", sr_cloud_nn(nullptr, &cd), true);
    sr_cloud_nn_desc b = cd;
    b.n_query = 4096, b.query_xform = nullptr, b.target_xform = fake<double>(2), b.dist = nullptr, b.index = nullptr;
    b.stats = nullptr;
    expect("sr_cloud_nn 4096-point probe, histogram only", sr_cloud_nn(nullptr, &b), true);
    b = cd, b.n_query = 1, b.n_target = 1, b.hist = nullptr, b.n_bins = 0, b.bin_len = 0.f, b.target_chunk = 64;
    expect("sr_cloud_nn 1 x 1 without a histogram", sr_cloud_nn(nullptr, &b), true);
    b = cd, b.n_query = 2147483647, b.n_target = 2147483647, b.target_chunk = 1 << 20;
    b.workspace_bytes = sr_cloud_nn_workspace(b.n_query, b.n_target, b.target_chunk, 0);
    expect("sr_cloud_nn 2^31 - 1 points a side", sr_cloud_nn(nullptr, &b), true);
    b = cd, b.query = nullptr;
    expect("sr_cloud_nn null query", sr_cloud_nn(nullptr, &b), false);
    b = cd, b.target = nullptr;
    expect("sr_cloud_nn null target", sr_cloud_nn(nullptr, &b), false);
    b = cd, b.workspace = nullptr;
    expect("sr_cloud_nn null workspace", sr_cloud_nn(nullptr, &b), false);
    b = cd, b.n_query = 0;
    expect("sr_cloud_nn 0 queries", sr_cloud_nn(nullptr, &b), false);
    b = cd, b.n_query = int64_t(1) << 31;
    expect("sr_cloud_nn 2^31 queries", sr_cloud_nn(nullptr, &b), false);
    b = cd, b.n_target = 0;
    expect("sr_cloud_nn 0 targets", sr_cloud_nn(nullptr, &b), false);
    b = cd, b.n_target = int64_t(1) << 31;
    expect("sr_cloud_nn 2^31 targets", sr_cloud_nn(nullptr, &b), false);
    b = cd, b.dist = nullptr, b.index = nullptr, b.hist = nullptr, b.stats = nullptr;
    expect("sr_cloud_nn every output NULL", sr_cloud_nn(nullptr, &b), false);
    b = cd, b.n_bins = 0;
    expect("sr_cloud_nn 0 bins", sr_cloud_nn(nullptr, &b), false);
    b = cd, b.n_bins = 1025;
    expect("sr_cloud_nn 1025 bins", sr_cloud_nn(nullptr, &b), false);
    b = cd, b.bin_len = 0.f;
    expect("sr_cloud_nn bin_len 0", sr_cloud_nn(nullptr, &b), false);
    b = cd, b.bin_len = -1.f;
    expect("sr_cloud_nn bin_len -1", sr_cloud_nn(nullptr, &b), false);
    const uint32_t inf_bits = 0x7f800000u, nan_bits = 0x7fc00000u;
    b = cd, std::memcpy(&b.bin_len, &inf_bits, sizeof(inf_bits));
    expect("sr_cloud_nn bin_len Inf", sr_cloud_nn(nullptr, &b), false);
    b = cd, std::memcpy(&b.bin_len, &nan_bits, sizeof(nan_bits));
    expect("sr_cloud_nn bin_len NaN", sr_cloud_nn(nullptr, &b), false);
    b = cd, b.target_chunk = -64;
    expect("sr_cloud_nn target_chunk -64", sr_cloud_nn(nullptr, &b), false);
    b = cd, b.target_chunk = 100;
    expect("sr_cloud_nn target_chunk 100", sr_cloud_nn(nullptr, &b), false);
    b = cd, b.target_chunk = 64, b.workspace_bytes = int64_t(1) << 62;
    expect("sr_cloud_nn more than 65535 slices", sr_cloud_nn(nullptr, &b), false);
    b = cd, b.workspace_bytes = need - 1;
    expect("sr_cloud_nn workspace one byte short", sr_cloud_nn(nullptr, &b), false);
    b = cd, b.workspace = (char*)fake(7) + 8;
    expect("sr_cloud_nn workspace % 16", sr_cloud_nn(nullptr, &b), false);
    b = cd, b.query_xform = (const double*)((const char*)fake(2) + 4);
    expect("sr_cloud_nn query_xform % 8", sr_cloud_nn(nullptr, &b), false);
    b = cd, b.target_xform = (const double*)((const char*)fake(2) + 4);
    expect("sr_cloud_nn target_xform % 8", sr_cloud_nn(nullptr, &b), false);
    b = cd, b.stats = (double*)((char*)fake(6) + 4);
    expect("sr_cloud_nn stats % 8", sr_cloud_nn(nullptr, &b), false);
  }
  expect("sr_select_ranks null", sr_select_ranks(nullptr, nullptr), false);
  expect("sr_depth_eval null", sr_depth_eval(nullptr, nullptr), false);
  {  // ABI 1.12: every rejection the header lists, then the planned shapes up to the launch
    const int64_t pix = 518 * 518;
    const int64_t need = sr_select_workspace(64, 2);
    std::printf("select workspace bytes: %lld\n", (long long)need);
    if (need < 64 * 2 * 256 * 4 || sr_select_workspace(0, 1) != 0 || sr_select_workspace(1, 0) != 0 ||
        sr_select_workspace(1, 5) != 0 || sr_select_workspace(-1, 1) != 0)
      ++g_fail;
    {  // never shrinks when a count grows
      int64_t prev_g = 0;
      for (int g : {1, 2, 63, 64, 65, 4096, 65535, 1 << 20, 2147483647}) {
        int64_t prev_r = 0;
        for (int r = 1; r <= SR_SELECT_MAX_RANKS; ++r) {
          const int64_t w = sr_select_workspace(g, r);
          if (w <= 0 || w < prev_r || (w & 15)) ++g_fail;
          prev_r = w;
        }
        if (sr_select_workspace(g, 1) < prev_g) ++g_fail;
        prev_g = sr_select_workspace(g, 1);
      }
    }
    sr_select_desc sd{};
    sd.x = fake<float>(0), sd.mask = fake<uint8_t>(1), sd.group = fake<int32_t>(2), sd.n_rows = 64, sd.row_len = pix;
    sd.row_stride = pix, sd.n_groups = 64, sd.n_ranks = 2, sd.rank_num[0] = 1, sd.rank_den[0] = 2, sd.rank_num[1] = 9;
    sd.rank_den[1] = 10, sd.value = fake<float>(3), sd.count = fake<uint32_t>(4), sd.workspace = fake(5);
    sd.workspace_bytes = need;
    expect("sr_select_ranks 64 x 518 x 518, two ranks", sr_select_ranks(nullptr, &sd), true);
    sr_select_desc b = sd;
    b.mask = nullptr, b.group = nullptr, b.count = nullptr, b.blocks_per_row = 7;
    expect("sr_select_ranks bare, 7 workgroups a row", sr_select_ranks(nullptr, &b), true);
    b = sd, b.n_rows = 1, b.row_len = int64_t(1) << 31, b.row_stride = b.row_len, b.n_groups = 1, b.n_ranks = 4;
    b.rank_num[2] = 0, b.rank_den[2] = 1, b.rank_num[3] = 1 << 20, b.rank_den[3] = 1 << 20;
    b.workspace_bytes = sr_select_workspace(1, 4);
    expect("sr_select_ranks one row of 2^31, four ranks", sr_select_ranks(nullptr, &b), true);
    b = sd, b.n_rows = 1, b.row_len = 1, b.row_stride = 1, b.n_groups = 1;
    expect("sr_select_ranks 1 x 1", sr_select_ranks(nullptr, &b), true);
    b = sd, b.n_groups = 1, b.row_stride = pix + 3;
    expect("sr_select_ranks one group, padded rows", sr_select_ranks(nullptr, &b), true);
    b = sd, b.x = nullptr;
    expect("sr_select_ranks null x", sr_select_ranks(nullptr, &b), false);
    b = sd, b.value = nullptr;
    expect("sr_select_ranks null value", sr_select_ranks(nullptr, &b), false);
    b = sd, b.workspace = nullptr;
    expect("sr_select_ranks null workspace", sr_select_ranks(nullptr, &b), false);
    b = sd, b.n_ranks = 0;
    expect("sr_select_ranks 0 ranks", sr_select_ranks(nullptr, &b), false);
    b = sd, b.n_ranks = 5;
    expect("sr_select_ranks 5 ranks", sr_select_ranks(nullptr, &b), false);
    b = sd, b.rank_num[1] = -1;
    expect("sr_select_ranks num -1", sr_select_ranks(nullptr, &b), false);
    b = sd, b.rank_den[1] = 0;
    expect("sr_select_ranks den 0", sr_select_ranks(nullptr, &b), false);
    b = sd, b.rank_num[0] = 3;
    expect("sr_select_ranks num > den", sr_select_ranks(nullptr, &b), false);
    b = sd, b.rank_den[0] = (1 << 20) + 1;
    expect("sr_select_ranks den 2^20 + 1", sr_select_ranks(nullptr, &b), false);
    b = sd, b.n_rows = 0;
    expect("sr_select_ranks 0 rows", sr_select_ranks(nullptr, &b), false);
    b = sd, b.row_len = 0;
    expect("sr_select_ranks row_len 0", sr_select_ranks(nullptr, &b), false);
    b = sd, b.row_stride = pix - 1;
    expect("sr_select_ranks stride < row_len", sr_select_ranks(nullptr, &b), false);
    b = sd, b.n_rows = 8192, b.n_groups = 64;  // 8192 x 268,324 > 2^31
    expect("sr_select_ranks more than 2^31 elements", sr_select_ranks(nullptr, &b), false);
    b = sd, b.n_groups = 0;
    expect("sr_select_ranks 0 groups", sr_select_ranks(nullptr, &b), false);
    b = sd, b.n_groups = 65, b.workspace_bytes = int64_t(1) << 40;
    expect("sr_select_ranks more groups than rows", sr_select_ranks(nullptr, &b), false);
    b = sd, b.group = nullptr, b.n_groups = 3;
    expect("sr_select_ranks no group, 3 groups", sr_select_ranks(nullptr, &b), false);
    b = sd, b.blocks_per_row = -1;
    expect("sr_select_ranks blocks_per_row -1", sr_select_ranks(nullptr, &b), false);
    b = sd, b.blocks_per_row = 65536;
    expect("sr_select_ranks blocks_per_row 65536", sr_select_ranks(nullptr, &b), false);
    b = sd, b.n_rows = 1 << 20, b.row_len = 1, b.row_stride = 1, b.n_groups = 1, b.blocks_per_row = 4096;
    expect("sr_select_ranks 2^32 workgroups", sr_select_ranks(nullptr, &b), false);
    b = sd, b.workspace_bytes = need - 1;
    expect("sr_select_ranks workspace one byte short", sr_select_ranks(nullptr, &b), false);
    b = sd, b.workspace = (char*)fake(5) + 8;
    expect("sr_select_ranks workspace % 16", sr_select_ranks(nullptr, &b), false);

    const int64_t dneed = sr_depth_eval_workspace(64, pix, pix, 64, 1);
    std::printf("depth workspace bytes: %lld\n", (long long)dneed);
    if (dneed < 64 * pix * 5 || sr_depth_eval_workspace(64, pix, pix, 64, 0) > dneed - 64 * pix * 4 ||
        sr_depth_eval_workspace(0, pix, pix, 1, 0) != 0 || sr_depth_eval_workspace(65536, 1, 1, 1, 0) != 0 ||
        sr_depth_eval_workspace(64, 0, pix, 64, 0) != 0 || sr_depth_eval_workspace(64, pix, pix - 1, 64, 0) != 0 ||
        sr_depth_eval_workspace(64, pix, pix, 0, 0) != 0 || sr_depth_eval_workspace(64, pix, pix, 65, 0) != 0 ||
        sr_depth_eval_workspace(8192, pix, pix, 1, 0) != 0)
      ++g_fail;
    {  // never shrinks when a count grows
      const int64_t ps[] = {1, 2047, 2048, 2049, 4900, pix, pix + 1, 1 << 20};
      const int vs[] = {1, 2, 5, 64, 65, 2000};
      for (int scratch : {0, 1}) {
        for (int64_t n : ps) {
          int64_t prev = 0;
          for (int v : vs) {
            const int64_t w = sr_depth_eval_workspace(v, n, n, 1, scratch), wg = sr_depth_eval_workspace(v, n, n, v, scratch);
            if (w <= 0 || w < prev || wg < w || sr_depth_eval_workspace(v, n, n + 5, 1, scratch) < w) ++g_fail;
            prev = w;
          }
        }
        for (int v : vs) {
          int64_t prev = 0;
          for (int64_t n : ps) {
            const int64_t w = sr_depth_eval_workspace(v, n, 1 << 20, 1, scratch);
            if (w <= 0 || w < prev) ++g_fail;
            prev = w;
          }
        }
      }
    }
    sr_depth_eval_desc dd{};
    dd.pred = fake<float>(0), dd.gt = fake<float>(1), dd.mask = fake<uint8_t>(2), dd.conf = fake<float>(3);
    dd.conf_min = fake<float>(4), dd.group = fake<int32_t>(5), dd.n_pix = pix, dd.stride = pix, dd.n_views = 64;
    dd.n_groups = 64, dd.gt_min = 0.f, dd.gt_max = 1e30f, dd.align = SR_DEPTH_ALIGN_MEDIAN, dd.n_bins = 1024;
    dd.bin_len = 0.005f, dd.xform = fake<double>(6), dd.status = fake<int32_t>(7), dd.stats = fake<double>(8);
    dd.hist = fake<uint32_t>(9), dd.aligned = fake<float>(10), dd.rel_err = fake<float>(11), dd.rel_q = fake<float>(12);
    dd.workspace = fake(13), dd.workspace_bytes = dneed;
    expect("sr_depth_eval 64 x 518 x 518 MEDIAN, every output", sr_depth_eval(nullptr, &dd), true);
    sr_depth_eval_desc c = dd;
    for (int align : {SR_DEPTH_ALIGN_NONE, SR_DEPTH_ALIGN_SCALE, SR_DEPTH_ALIGN_SCALE_SHIFT, SR_DEPTH_ALIGN_GIVEN}) {
      c = dd, c.align = align, c.n_views = 5, c.n_groups = 2;
      expect("sr_depth_eval 5 views in 2 groups", sr_depth_eval(nullptr, &c), true);
    }
    c = dd, c.mask = nullptr, c.conf = nullptr, c.conf_min = nullptr, c.group = nullptr, c.aligned = nullptr;
    c.rel_err = nullptr;
    expect("sr_depth_eval bare, rel_q through the scratch", sr_depth_eval(nullptr, &c), true);
    c.rel_q = nullptr, c.workspace_bytes = sr_depth_eval_workspace(64, pix, pix, 64, 0);
    expect("sr_depth_eval bare, no quantiles", sr_depth_eval(nullptr, &c), true);
    c = dd, c.n_views = 1, c.n_groups = 1, c.n_pix = 1, c.stride = 1, c.n_bins = 1;
    expect("sr_depth_eval 1 x 1", sr_depth_eval(nullptr, &c), true);
    const uint32_t inf_bits = 0x7f800000u, nan_bits = 0x7fc00000u;
    c = dd, std::memcpy(&c.gt_max, &inf_bits, sizeof(inf_bits));
    expect("sr_depth_eval gt_max Inf", sr_depth_eval(nullptr, &c), true);
    c = dd, c.pred = nullptr;
    expect("sr_depth_eval null pred", sr_depth_eval(nullptr, &c), false);
    c = dd, c.gt = nullptr;
    expect("sr_depth_eval null gt", sr_depth_eval(nullptr, &c), false);
    c = dd, c.xform = nullptr;
    expect("sr_depth_eval null xform", sr_depth_eval(nullptr, &c), false);
    c = dd, c.status = nullptr;
    expect("sr_depth_eval null status", sr_depth_eval(nullptr, &c), false);
    c = dd, c.stats = nullptr;
    expect("sr_depth_eval null stats", sr_depth_eval(nullptr, &c), false);
    c = dd, c.hist = nullptr;
    expect("sr_depth_eval null hist", sr_depth_eval(nullptr, &c), false);
    c = dd, c.workspace = nullptr;
    expect("sr_depth_eval null workspace", sr_depth_eval(nullptr, &c), false);
    c = dd, c.n_views = 0;
    expect("sr_depth_eval 0 views", sr_depth_eval(nullptr, &c), false);
    c = dd, c.n_views = 65536, c.n_pix = 1, c.stride = 1;
    expect("sr_depth_eval 65536 views", sr_depth_eval(nullptr, &c), false);
    c = dd, c.n_pix = 0;
    expect("sr_depth_eval 0 pixels", sr_depth_eval(nullptr, &c), false);
    c = dd, c.stride = pix - 1;
    expect("sr_depth_eval stride < n_pix", sr_depth_eval(nullptr, &c), false);
    c = dd, c.n_views = 8192, c.workspace_bytes = int64_t(1) << 50;
    expect("sr_depth_eval more than 2^31 floats", sr_depth_eval(nullptr, &c), false);
    c = dd, c.n_groups = 0;
    expect("sr_depth_eval 0 groups", sr_depth_eval(nullptr, &c), false);
    c = dd, c.n_groups = 65, c.workspace_bytes = int64_t(1) << 50;
    expect("sr_depth_eval more groups than views", sr_depth_eval(nullptr, &c), false);
    c = dd, c.group = nullptr, c.n_groups = 1;
    expect("sr_depth_eval no group, 1 group", sr_depth_eval(nullptr, &c), false);
    c = dd, c.conf_min = nullptr;
    expect("sr_depth_eval conf without conf_min", sr_depth_eval(nullptr, &c), false);
    c = dd, c.conf = nullptr;
    expect("sr_depth_eval conf_min without conf", sr_depth_eval(nullptr, &c), false);
    c = dd, std::memcpy(&c.gt_min, &nan_bits, sizeof(nan_bits));
    expect("sr_depth_eval gt_min NaN", sr_depth_eval(nullptr, &c), false);
    c = dd, std::memcpy(&c.gt_max, &nan_bits, sizeof(nan_bits));
    expect("sr_depth_eval gt_max NaN", sr_depth_eval(nullptr, &c), false);
    c = dd, c.gt_min = 2.f, c.gt_max = 2.f;
    expect("sr_depth_eval gt_min == gt_max", sr_depth_eval(nullptr, &c), false);
    c = dd, c.align = -1;
    expect("sr_depth_eval align -1", sr_depth_eval(nullptr, &c), false);
    c = dd, c.align = 5;
    expect("sr_depth_eval align 5", sr_depth_eval(nullptr, &c), false);
    c = dd, c.n_bins = 0;
    expect("sr_depth_eval 0 bins", sr_depth_eval(nullptr, &c), false);
    c = dd, c.n_bins = 1025;
    expect("sr_depth_eval 1025 bins", sr_depth_eval(nullptr, &c), false);
    c = dd, c.bin_len = 0.f;
    expect("sr_depth_eval bin_len 0", sr_depth_eval(nullptr, &c), false);
    c = dd, c.bin_len = -1.f;
    expect("sr_depth_eval bin_len -1", sr_depth_eval(nullptr, &c), false);
    c = dd, std::memcpy(&c.bin_len, &inf_bits, sizeof(inf_bits));
    expect("sr_depth_eval bin_len Inf", sr_depth_eval(nullptr, &c), false);
    c = dd, std::memcpy(&c.bin_len, &nan_bits, sizeof(nan_bits));
    expect("sr_depth_eval bin_len NaN", sr_depth_eval(nullptr, &c), false);
    c = dd, c.workspace_bytes = dneed - 64 * pix * 4;
    c.rel_err = nullptr;
    expect("sr_depth_eval workspace without the scratch", sr_depth_eval(nullptr, &c), false);
    c = dd, c.workspace_bytes = sr_depth_eval_workspace(64, pix, pix, 64, 0) - 1;
    expect("sr_depth_eval workspace one byte short", sr_depth_eval(nullptr, &c), false);
    c = dd, c.workspace = (char*)fake(13) + 8;
    expect("sr_depth_eval workspace % 16", sr_depth_eval(nullptr, &c), false);
    c = dd, c.xform = (double*)((char*)fake(6) + 4);
    expect("sr_depth_eval xform % 8", sr_depth_eval(nullptr, &c), false);
    c = dd, c.stats = (double*)((char*)fake(8) + 4);
    expect("sr_depth_eval stats % 8", sr_depth_eval(nullptr, &c), false);
  }
  {
    // ---- sr_sort_pairs / sr_cloud_voxel (ABI 1.13)
    const int64_t big = 32LL * 518 * 518, most = 2147483647LL;
    {  // never shrinks when n grows; 0 outside the range
      const int64_t ns[] = {1, 2, 63, 64, 65, 2047, 2048, 2049, 4097, 70001, 5LL * 518 * 518, big, 1LL << 30, most};
      int64_t ps = 0, pv = 0;
      for (int64_t n : ns) {
        const int64_t s = sr_sort_workspace(n), v = sr_cloud_voxel_workspace(n);
        if (s <= 0 || s % 16 || s < ps || s < 24 * n || v < s + 24 * n || v % 16 || v < pv) ++g_fail;
        ps = s, pv = v;
      }
      for (int64_t n : {int64_t(0), int64_t(-1), most + 1, int64_t(1) << 40})
        if (sr_sort_workspace(n) != 0 || sr_cloud_voxel_workspace(n) != 0) ++g_fail;
      std::printf("sort / voxel workspace bytes at 32 x 518 x 518: %lld / %lld\n", (long long)sr_sort_workspace(big),
                  (long long)sr_cloud_voxel_workspace(big));
    }
    sr_sort_desc so{};
    so.keys_in = fake<uint64_t>(0), so.vals_in = fake<uint32_t>(1), so.keys_out = fake<uint64_t>(2);
    so.vals_out = fake<uint32_t>(3), so.n = big, so.key_bits = 64, so.workspace = fake(4);
    so.workspace_bytes = sr_sort_workspace(big);
    expect("sr_sort_pairs 32 x 518 x 518, 64 bits", sr_sort_pairs(nullptr, &so), true);
    sr_sort_desc t = so;
    for (int bits : {1, 7, 8, 9, 16, 31, 33, 63}) {
      t = so, t.key_bits = bits;
      expect("sr_sort_pairs key_bits sweep", sr_sort_pairs(nullptr, &t), true);
    }
    for (int64_t n : {int64_t(1), int64_t(2), int64_t(2048), int64_t(2049), int64_t(70001)}) {
      t = so, t.n = n;
      expect("sr_sort_pairs n sweep", sr_sort_pairs(nullptr, &t), true);
    }
    t = so, t.vals_in = nullptr, t.keys_out = nullptr;
    expect("sr_sort_pairs permutation only", sr_sort_pairs(nullptr, &t), true);
    t = so, t.n = most, t.workspace_bytes = sr_sort_workspace(most);
    expect("sr_sort_pairs 2^31 - 1", sr_sort_pairs(nullptr, &t), true);
    expect("sr_sort_pairs null desc", sr_sort_pairs(nullptr, nullptr), false);
    t = so, t.keys_in = nullptr;
    expect("sr_sort_pairs null keys_in", sr_sort_pairs(nullptr, &t), false);
    t = so, t.vals_out = nullptr;
    expect("sr_sort_pairs null vals_out", sr_sort_pairs(nullptr, &t), false);
    t = so, t.workspace = nullptr;
    expect("sr_sort_pairs null workspace", sr_sort_pairs(nullptr, &t), false);
    t = so, t.n = 0;
    expect("sr_sort_pairs n 0", sr_sort_pairs(nullptr, &t), false);
    t = so, t.n = most + 1, t.workspace_bytes = int64_t(1) << 50;
    expect("sr_sort_pairs n 2^31", sr_sort_pairs(nullptr, &t), false);
    t = so, t.key_bits = 0;
    expect("sr_sort_pairs key_bits 0", sr_sort_pairs(nullptr, &t), false);
    t = so, t.key_bits = 65;
    expect("sr_sort_pairs key_bits 65", sr_sort_pairs(nullptr, &t), false);
    t = so, t.keys_out = fake<uint64_t>(0);
    expect("sr_sort_pairs keys_out == keys_in", sr_sort_pairs(nullptr, &t), false);
    t = so, t.vals_out = fake<uint32_t>(1);
    expect("sr_sort_pairs vals_out == vals_in", sr_sort_pairs(nullptr, &t), false);
    t = so, t.keys_in = (const uint64_t*)((const char*)fake(0) + 4);
    expect("sr_sort_pairs keys_in % 8", sr_sort_pairs(nullptr, &t), false);
    t = so, t.vals_out = (uint32_t*)((char*)fake(3) + 2);
    expect("sr_sort_pairs vals_out % 4", sr_sort_pairs(nullptr, &t), false);
    t = so, t.workspace_bytes -= 1;
    expect("sr_sort_pairs workspace one byte short", sr_sort_pairs(nullptr, &t), false);
    t = so, t.workspace = (char*)fake(4) + 8;
    expect("sr_sort_pairs workspace % 16", sr_sort_pairs(nullptr, &t), false);

    sr_cloud_voxel_desc vd{};
    vd.points = fake<float>(0), vd.attr = fake<float>(1), vd.mask = fake<uint8_t>(2), vd.weight = fake<float>(3);
    vd.xform = fake<double>(4), vd.n = big, vd.ldp = 3, vd.lda = 4, vd.n_attr = 4, vd.axis_bits = 21;
    vd.mode = SR_VOXEL_BEST, vd.origin[0] = 0.1, vd.origin[1] = -0.2, vd.origin[2] = 0.3, vd.voxel = 0.01;
    vd.capacity = big, vd.out_points = fake<float>(5), vd.out_attr = fake<float>(6), vd.out_count = fake<uint32_t>(7);
    vd.out_index = fake<uint32_t>(8), vd.out_key = fake<uint64_t>(9), vd.voxel_of = fake<int32_t>(10);
    vd.counts = fake<uint32_t>(11), vd.workspace = fake(12), vd.workspace_bytes = sr_cloud_voxel_workspace(big);
    expect("sr_cloud_voxel 32 x 518 x 518 BEST, every output", sr_cloud_voxel(nullptr, &vd), true);
    sr_cloud_voxel_desc u = vd;
    u = vd, u.mode = SR_VOXEL_MEAN, u.weight = nullptr;
    expect("sr_cloud_voxel MEAN", sr_cloud_voxel(nullptr, &u), true);
    u = vd, u.attr = nullptr, u.n_attr = 0, u.mask = nullptr, u.weight = nullptr, u.xform = nullptr, u.out_attr = nullptr;
    u.out_count = nullptr, u.out_index = nullptr, u.out_key = nullptr, u.voxel_of = nullptr, u.counts = nullptr;
    expect("sr_cloud_voxel bare", sr_cloud_voxel(nullptr, &u), true);
    for (int b : {1, 4, 20}) {
      u = vd, u.axis_bits = b, u.ldp = 4, u.lda = 9, u.n_attr = 8, u.capacity = 1;
      expect("sr_cloud_voxel axis_bits sweep, padded rows, capacity 1", sr_cloud_voxel(nullptr, &u), true);
    }
    u = vd, u.n = 1, u.capacity = 1;
    expect("sr_cloud_voxel one point", sr_cloud_voxel(nullptr, &u), true);
    u = vd, u.n = most, u.capacity = 5, u.workspace_bytes = sr_cloud_voxel_workspace(most);
    expect("sr_cloud_voxel 2^31 - 1 points", sr_cloud_voxel(nullptr, &u), true);
    expect("sr_cloud_voxel null desc", sr_cloud_voxel(nullptr, nullptr), false);
    u = vd, u.points = nullptr;
    expect("sr_cloud_voxel null points", sr_cloud_voxel(nullptr, &u), false);
    u = vd, u.out_points = nullptr;
    expect("sr_cloud_voxel null out_points", sr_cloud_voxel(nullptr, &u), false);
    u = vd, u.workspace = nullptr;
    expect("sr_cloud_voxel null workspace", sr_cloud_voxel(nullptr, &u), false);
    u = vd, u.n = 0;
    expect("sr_cloud_voxel n 0", sr_cloud_voxel(nullptr, &u), false);
    u = vd, u.n = most + 1, u.workspace_bytes = int64_t(1) << 50;
    expect("sr_cloud_voxel n 2^31", sr_cloud_voxel(nullptr, &u), false);
    u = vd, u.ldp = 2;
    expect("sr_cloud_voxel ldp 2", sr_cloud_voxel(nullptr, &u), false);
    u = vd, u.n_attr = -1;
    expect("sr_cloud_voxel n_attr -1", sr_cloud_voxel(nullptr, &u), false);
    u = vd, u.n_attr = 9, u.lda = 9;
    expect("sr_cloud_voxel n_attr 9", sr_cloud_voxel(nullptr, &u), false);
    u = vd, u.attr = nullptr;
    expect("sr_cloud_voxel n_attr without attr", sr_cloud_voxel(nullptr, &u), false);
    u = vd, u.lda = 3;
    expect("sr_cloud_voxel lda < n_attr", sr_cloud_voxel(nullptr, &u), false);
    u = vd, u.mode = SR_VOXEL_MEAN;
    expect("sr_cloud_voxel weight under MEAN", sr_cloud_voxel(nullptr, &u), false);
    u = vd, u.mode = 2;
    expect("sr_cloud_voxel mode 2", sr_cloud_voxel(nullptr, &u), false);
    u = vd, u.mode = -1;
    expect("sr_cloud_voxel mode -1", sr_cloud_voxel(nullptr, &u), false);
    u = vd, u.axis_bits = 0;
    expect("sr_cloud_voxel axis_bits 0", sr_cloud_voxel(nullptr, &u), false);
    u = vd, u.axis_bits = 22;
    expect("sr_cloud_voxel axis_bits 22", sr_cloud_voxel(nullptr, &u), false);
    const uint64_t inf64 = 0x7ff0000000000000ull, nan64 = 0x7ff8000000000000ull;
    u = vd, std::memcpy(&u.origin[1], &nan64, 8);
    expect("sr_cloud_voxel origin NaN", sr_cloud_voxel(nullptr, &u), false);
    u = vd, std::memcpy(&u.origin[2], &inf64, 8);
    expect("sr_cloud_voxel origin Inf", sr_cloud_voxel(nullptr, &u), false);
    u = vd, u.voxel = 0.0;
    expect("sr_cloud_voxel voxel 0", sr_cloud_voxel(nullptr, &u), false);
    u = vd, u.voxel = -1.0;
    expect("sr_cloud_voxel voxel -1", sr_cloud_voxel(nullptr, &u), false);
    u = vd, std::memcpy(&u.voxel, &inf64, 8);
    expect("sr_cloud_voxel voxel Inf", sr_cloud_voxel(nullptr, &u), false);
    u = vd, std::memcpy(&u.voxel, &nan64, 8);
    expect("sr_cloud_voxel voxel NaN", sr_cloud_voxel(nullptr, &u), false);
    u = vd, u.capacity = 0;
    expect("sr_cloud_voxel capacity 0", sr_cloud_voxel(nullptr, &u), false);
    u = vd, u.capacity = big + 1;
    expect("sr_cloud_voxel capacity n + 1", sr_cloud_voxel(nullptr, &u), false);
    u = vd, u.workspace_bytes -= 1;
    expect("sr_cloud_voxel workspace one byte short", sr_cloud_voxel(nullptr, &u), false);
    u = vd, u.workspace = (char*)fake(12) + 8;
    expect("sr_cloud_voxel workspace % 16", sr_cloud_voxel(nullptr, &u), false);
    u = vd, u.xform = (const double*)((const char*)fake(4) + 4);
    expect("sr_cloud_voxel xform % 8", sr_cloud_voxel(nullptr, &u), false);
    u = vd, u.out_key = (uint64_t*)((char*)fake(9) + 4);
    expect("sr_cloud_voxel out_key % 8", sr_cloud_voxel(nullptr, &u), false);
  }
  {
    // ---- sr_sparsify (ABI 1.14): the workspace sweep, the planned shapes up to the launch, every rejection
    const int64_t pix = 518LL * 518, most = 2147483647LL;
    {  // never shrinks when an argument grows; 0 for what the call rejects
      const int64_t rows[] = {1, 2, 3, 5, 32, 64, 65535, 70001}, lens[] = {1, 2, 63, 64, 65, 2047, 2048, 2049, 6149, 30000};
      const int groups[] = {1, 2, 3, 5, 32, 65535}, steps[] = {1, 2, 3, 7, 100, 1024};
      for (int64_t r : rows)
        for (int64_t l : lens)
          for (int g : groups)
            for (int k : steps) {
              if (g > r) continue;
              const int64_t w = sr_sparsify_workspace(r, l, g, k);
              if (w <= 0 || w % 16 || w < 32 * r * l + sr_sort_workspace(r * l) + 16 * (int64_t)g * k) ++g_fail;
              if (sr_sparsify_workspace(r + 1, l, g, k) < w || sr_sparsify_workspace(r, l + 1, g, k) < w) ++g_fail;
              if (g + 1 <= r && g + 1 <= 65535 && sr_sparsify_workspace(r, l, g + 1, k) < w) ++g_fail;
              if (k + 1 <= 1024 && sr_sparsify_workspace(r, l, g, k + 1) < w) ++g_fail;
            }
      if (sr_sparsify_workspace(0, 5, 1, 1) || sr_sparsify_workspace(5, 0, 1, 1) || sr_sparsify_workspace(-1, 5, 1, 1) ||
          sr_sparsify_workspace(5, 5, 0, 1) || sr_sparsify_workspace(5, 5, 6, 1) || sr_sparsify_workspace(70000, 5, 65536, 1) ||
          sr_sparsify_workspace(5, 5, 1, 0) || sr_sparsify_workspace(5, 5, 1, 1025) || sr_sparsify_workspace(2, 1LL << 30, 1, 1) ||
          sr_sparsify_workspace(1LL << 31, 1, 1, 1) || sr_sparsify_workspace(1LL << 62, 4, 1, 1) ||
          sr_sparsify_workspace(most, 1, 1, 1) <= 0 || sr_sparsify_workspace(1, most, 1, 1) <= 0)
        ++g_fail;
      std::printf("sparsify workspace bytes at 32 x 518 x 518, K = 100, view / scene: %lld / %lld\n",
                  (long long)sr_sparsify_workspace(32, pix, 32, 100), (long long)sr_sparsify_workspace(32, pix, 1, 100));
    }
    sr_sparsify_desc sd{};
    sd.err = fake<float>(0), sd.conf = fake<float>(1), sd.mask = fake<uint8_t>(2), sd.group = fake<int32_t>(3);
    sd.n_rows = 32, sd.row_len = pix, sd.row_stride = pix, sd.n_groups = 4, sd.n_steps = 100;
    sd.order = SR_SPARSIFY_CONFIDENCE, sd.bin_sum = fake<double>(4), sd.cut = fake<float>(5), sd.count = fake<uint32_t>(6);
    sd.workspace = fake(7), sd.workspace_bytes = sr_sparsify_workspace(32, pix, 4, 100);
    expect("sr_sparsify 32 x 518 x 518 in 4 groups, every output", sr_sparsify(nullptr, &sd), true);
    sr_sparsify_desc v = sd;
    v = sd, v.order = SR_SPARSIFY_UNCERTAINTY, v.mask = nullptr, v.cut = nullptr, v.count = nullptr;
    expect("sr_sparsify uncertainty, bare", sr_sparsify(nullptr, &v), true);
    v = sd, v.group = nullptr, v.n_groups = 32, v.workspace_bytes = sr_sparsify_workspace(32, pix, 32, 100);
    expect("sr_sparsify by view", sr_sparsify(nullptr, &v), true);
    v = sd, v.n_groups = 1, v.row_stride = pix + 3;
    expect("sr_sparsify by scene, padded rows", sr_sparsify(nullptr, &v), true);
    for (int k : {1, 2, 3, 7, 1024}) {
      v = sd, v.n_steps = k, v.workspace_bytes = sr_sparsify_workspace(32, pix, 4, k);
      expect("sr_sparsify n_steps sweep", sr_sparsify(nullptr, &v), true);
    }
    for (int64_t l : {int64_t(1), int64_t(2), int64_t(255), int64_t(256), int64_t(257), int64_t(4097), int64_t(70001)}) {
      v = sd, v.n_rows = 3, v.row_len = v.row_stride = l, v.n_groups = 3, v.group = nullptr;
      expect("sr_sparsify row_len sweep", sr_sparsify(nullptr, &v), true);
    }
    v = sd, v.n_rows = 70000, v.row_len = v.row_stride = 3, v.n_groups = 65535, v.n_steps = 1024;
    v.workspace_bytes = sr_sparsify_workspace(70000, 3, 65535, 1024);
    expect("sr_sparsify 65535 groups of 1024 steps", sr_sparsify(nullptr, &v), true);
    v = sd, v.n_rows = 1, v.row_len = v.row_stride = most, v.n_groups = 1, v.n_steps = 1;
    v.workspace_bytes = sr_sparsify_workspace(1, most, 1, 1);
    expect("sr_sparsify 2^31 - 1 elements", sr_sparsify(nullptr, &v), true);
    expect("sr_sparsify null desc", sr_sparsify(nullptr, nullptr), false);
    v = sd, v.err = nullptr;
    expect("sr_sparsify null err", sr_sparsify(nullptr, &v), false);
    v = sd, v.conf = nullptr;
    expect("sr_sparsify null conf", sr_sparsify(nullptr, &v), false);
    v = sd, v.bin_sum = nullptr;
    expect("sr_sparsify null bin_sum", sr_sparsify(nullptr, &v), false);
    v = sd, v.workspace = nullptr;
    expect("sr_sparsify null workspace", sr_sparsify(nullptr, &v), false);
    v = sd, v.n_rows = 0;
    expect("sr_sparsify n_rows 0", sr_sparsify(nullptr, &v), false);
    v = sd, v.row_len = 0, v.row_stride = 0;
    expect("sr_sparsify row_len 0", sr_sparsify(nullptr, &v), false);
    v = sd, v.row_stride = pix - 1;
    expect("sr_sparsify row_stride < row_len", sr_sparsify(nullptr, &v), false);
    v = sd, v.n_rows = 8004, v.workspace_bytes = int64_t(1) << 50;
    expect("sr_sparsify 2^31 elements and more", sr_sparsify(nullptr, &v), false);
    v = sd, v.n_rows = int64_t(1) << 62, v.row_len = v.row_stride = 4, v.workspace_bytes = int64_t(1) << 50;
    expect("sr_sparsify a product that overflows", sr_sparsify(nullptr, &v), false);
    v = sd, v.n_groups = 0;
    expect("sr_sparsify n_groups 0", sr_sparsify(nullptr, &v), false);
    v = sd, v.n_groups = 33;
    expect("sr_sparsify n_groups above n_rows", sr_sparsify(nullptr, &v), false);
    v = sd, v.n_rows = 70000, v.row_len = v.row_stride = 3, v.n_groups = 65536, v.workspace_bytes = int64_t(1) << 50;
    expect("sr_sparsify n_groups 65536", sr_sparsify(nullptr, &v), false);
    v = sd, v.group = nullptr;
    expect("sr_sparsify no group, n_groups != n_rows", sr_sparsify(nullptr, &v), false);
    v = sd, v.n_steps = 0;
    expect("sr_sparsify n_steps 0", sr_sparsify(nullptr, &v), false);
    v = sd, v.n_steps = 1025, v.workspace_bytes = int64_t(1) << 50;
    expect("sr_sparsify n_steps 1025", sr_sparsify(nullptr, &v), false);
    v = sd, v.order = 2;
    expect("sr_sparsify order 2", sr_sparsify(nullptr, &v), false);
    v = sd, v.order = -1;
    expect("sr_sparsify order -1", sr_sparsify(nullptr, &v), false);
    v = sd, v.workspace_bytes -= 1;
    expect("sr_sparsify workspace one byte short", sr_sparsify(nullptr, &v), false);
    v = sd, v.workspace = (char*)fake(7) + 8;
    expect("sr_sparsify workspace % 16", sr_sparsify(nullptr, &v), false);
    v = sd, v.bin_sum = (double*)((char*)fake(4) + 4);
    expect("sr_sparsify bin_sum % 8", sr_sparsify(nullptr, &v), false);
  }
  {
    // ---- sr_cloud_render (ABI 1.15): the workspace sweep, the planned shapes up to the launch, every rejection
    const int64_t big = 32LL * 518 * 518, most = 2147483647LL;
    const uint64_t inf_bits = 0x7ff0000000000000ull, nan_bits = 0x7ff8000000000000ull;
    double inf64, nan64;
    std::memcpy(&inf64, &inf_bits, 8), std::memcpy(&nan64, &nan_bits, 8);
    {  // never shrinks when an argument grows; 0 for what the call rejects
      const int vs[] = {1, 2, 3, 32, 65535}, hs[] = {1, 2, 37, 518, 1024}, ws[] = {1, 2, 53, 518, 2047};
      for (int v : vs)
        for (int h : hs)
          for (int w : ws) {
            const int64_t pix = (int64_t)v * h * w;
            const int64_t b = sr_cloud_render_workspace(v, h, w);
            if (pix > most) {
              if (b != 0) ++g_fail;
              continue;
            }
            if (b <= 0 || b % 16 || b < 8 * pix + 16 * (int64_t)v) ++g_fail;
            if (pix + (int64_t)h * w <= most && v < 65535 && sr_cloud_render_workspace(v + 1, h, w) < b) ++g_fail;
            if (pix + (int64_t)v * w <= most && sr_cloud_render_workspace(v, h + 1, w) < b) ++g_fail;
            if (pix + (int64_t)v * h <= most && sr_cloud_render_workspace(v, h, w + 1) < b) ++g_fail;
          }
      if (sr_cloud_render_workspace(0, 5, 5) || sr_cloud_render_workspace(-1, 5, 5) || sr_cloud_render_workspace(65536, 1, 1) ||
          sr_cloud_render_workspace(1, 0, 5) || sr_cloud_render_workspace(1, 5, 0) || sr_cloud_render_workspace(1, -3, 5) ||
          sr_cloud_render_workspace(1, 1 << 16, 1 << 15) || sr_cloud_render_workspace(2, 1 << 15, 1 << 15) ||
          sr_cloud_render_workspace(65535, 2147483647, 2147483647) || sr_cloud_render_workspace(1, 2147483647, 1) <= 0 ||
          sr_cloud_render_workspace(1, 1, 2147483647) <= 0 || sr_cloud_render_workspace(65535, 1, 1) <= 0)
        ++g_fail;
      std::printf("render workspace bytes at 32 x 518 x 518: %lld\n", (long long)sr_cloud_render_workspace(32, 518, 518));
    }
    sr_cloud_render_desc rd{};
    rd.points = fake<float>(0), rd.attr = fake<float>(1), rd.mask = fake<uint8_t>(2), rd.view_id = fake<int32_t>(3);
    rd.exclude = fake<int32_t>(4), rd.xform = fake<double>(5), rd.extrinsic = fake<float>(6), rd.intrinsic = fake<float>(7);
    rd.n = big, rd.ldp = 3, rd.lda = 4, rd.n_attr = 4, rd.n_views = 32, rd.height = 518, rd.width = 518, rd.radius = 1;
    rd.z_near = 1e-6, rd.z_far = inf64, rd.attr_fill = 0.5f;
    rd.depth = fake<float>(8), rd.index = fake<int32_t>(9), rd.out_attr = fake<float>(10), rd.counts = fake<uint32_t>(11);
    rd.workspace = fake(12), rd.workspace_bytes = sr_cloud_render_workspace(32, 518, 518);
    expect("sr_cloud_render 32 x 518 x 518, every output", sr_cloud_render(nullptr, &rd), true);
    sr_cloud_render_desc u = rd;
    u.attr = nullptr, u.out_attr = nullptr, u.n_attr = 0, u.lda = 0, u.mask = nullptr, u.view_id = nullptr, u.exclude = nullptr;
    u.xform = nullptr, u.index = nullptr, u.counts = nullptr, u.radius = 0;
    expect("sr_cloud_render bare, depth only", sr_cloud_render(nullptr, &u), true);
    u = rd, u.depth = nullptr, u.index = nullptr, u.out_attr = nullptr, u.attr = nullptr, u.n_attr = 0;
    expect("sr_cloud_render counts only", sr_cloud_render(nullptr, &u), true);
    for (int r = 0; r <= 3; ++r) {
      u = rd, u.radius = r, u.ldp = 5, u.lda = 9, u.n_attr = 8, u.z_far = u.z_near;
      expect("sr_cloud_render radius sweep, padded rows", sr_cloud_render(nullptr, &u), true);
    }
    u = rd, u.n = 1, u.n_views = 1, u.height = 1, u.width = 1;
    expect("sr_cloud_render one point, one pixel", sr_cloud_render(nullptr, &u), true);
    u = rd, u.n = most, u.n_views = 65535, u.height = 1, u.width = 1, u.workspace_bytes = sr_cloud_render_workspace(65535, 1, 1);
    expect("sr_cloud_render 2^31 - 1 points, 65535 views", sr_cloud_render(nullptr, &u), true);
    u = rd, u.n_views = 1, u.height = 1, u.width = 2147483647, u.workspace_bytes = sr_cloud_render_workspace(1, 1, 2147483647);
    expect("sr_cloud_render 2^31 - 1 pixels", sr_cloud_render(nullptr, &u), true);
    expect("sr_cloud_render null desc", sr_cloud_render(nullptr, nullptr), false);
    u = rd, u.points = nullptr;
    expect("sr_cloud_render null points", sr_cloud_render(nullptr, &u), false);
    u = rd, u.extrinsic = nullptr;
    expect("sr_cloud_render null extrinsic", sr_cloud_render(nullptr, &u), false);
    u = rd, u.intrinsic = nullptr;
    expect("sr_cloud_render null intrinsic", sr_cloud_render(nullptr, &u), false);
    u = rd, u.workspace = nullptr;
    expect("sr_cloud_render null workspace", sr_cloud_render(nullptr, &u), false);
    u = rd, u.n = 0;
    expect("sr_cloud_render n 0", sr_cloud_render(nullptr, &u), false);
    u = rd, u.n = most + 1;
    expect("sr_cloud_render n 2^31", sr_cloud_render(nullptr, &u), false);
    u = rd, u.ldp = 2;
    expect("sr_cloud_render ldp 2", sr_cloud_render(nullptr, &u), false);
    u = rd, u.n_attr = -1;
    expect("sr_cloud_render n_attr -1", sr_cloud_render(nullptr, &u), false);
    u = rd, u.n_attr = 9, u.lda = 9;
    expect("sr_cloud_render n_attr 9", sr_cloud_render(nullptr, &u), false);
    u = rd, u.attr = nullptr;
    expect("sr_cloud_render n_attr without attr", sr_cloud_render(nullptr, &u), false);
    u = rd, u.out_attr = nullptr;
    expect("sr_cloud_render n_attr without out_attr", sr_cloud_render(nullptr, &u), false);
    u = rd, u.lda = 3;
    expect("sr_cloud_render lda < n_attr", sr_cloud_render(nullptr, &u), false);
    u = rd, u.exclude = nullptr;
    expect("sr_cloud_render view_id without exclude", sr_cloud_render(nullptr, &u), false);
    u = rd, u.view_id = nullptr;
    expect("sr_cloud_render exclude without view_id", sr_cloud_render(nullptr, &u), false);
    u = rd, u.n_views = 0;
    expect("sr_cloud_render n_views 0", sr_cloud_render(nullptr, &u), false);
    u = rd, u.n_views = 65536, u.height = 1, u.width = 1, u.workspace_bytes = int64_t(1) << 50;
    expect("sr_cloud_render n_views 65536", sr_cloud_render(nullptr, &u), false);
    u = rd, u.height = 0;
    expect("sr_cloud_render height 0", sr_cloud_render(nullptr, &u), false);
    u = rd, u.width = -4;
    expect("sr_cloud_render width -4", sr_cloud_render(nullptr, &u), false);
    u = rd, u.n_views = 8004, u.workspace_bytes = int64_t(1) << 50;
    expect("sr_cloud_render 2^31 pixels and more", sr_cloud_render(nullptr, &u), false);
    u = rd, u.n_views = 65535, u.height = 2147483647, u.width = 2147483647, u.workspace_bytes = int64_t(1) << 50;
    expect("sr_cloud_render a product that overflows", sr_cloud_render(nullptr, &u), false);
    u = rd, u.radius = -1;
    expect("sr_cloud_render radius -1", sr_cloud_render(nullptr, &u), false);
    u = rd, u.radius = 4;
    expect("sr_cloud_render radius 4", sr_cloud_render(nullptr, &u), false);
    u = rd, u.z_near = 0.0;
    expect("sr_cloud_render z_near 0", sr_cloud_render(nullptr, &u), false);
    u = rd, u.z_near = -1.0;
    expect("sr_cloud_render z_near -1", sr_cloud_render(nullptr, &u), false);
    u = rd, u.z_near = nan64;
    expect("sr_cloud_render z_near NaN", sr_cloud_render(nullptr, &u), false);
    u = rd, u.z_near = inf64;
    expect("sr_cloud_render z_near Inf", sr_cloud_render(nullptr, &u), false);
    u = rd, u.z_far = nan64;
    expect("sr_cloud_render z_far NaN", sr_cloud_render(nullptr, &u), false);
    u = rd, u.z_near = 2.0, u.z_far = 1.0;
    expect("sr_cloud_render z_far < z_near", sr_cloud_render(nullptr, &u), false);
    u = rd, u.depth = nullptr, u.index = nullptr, u.counts = nullptr, u.attr = nullptr, u.out_attr = nullptr, u.n_attr = 0;
    expect("sr_cloud_render no output", sr_cloud_render(nullptr, &u), false);
    u = rd, u.workspace_bytes -= 1;
    expect("sr_cloud_render workspace one byte short", sr_cloud_render(nullptr, &u), false);
    u = rd, u.workspace = (char*)fake(12) + 8;
    expect("sr_cloud_render workspace % 16", sr_cloud_render(nullptr, &u), false);
    u = rd, u.xform = (const double*)((const char*)fake(5) + 4);
    expect("sr_cloud_render xform % 8", sr_cloud_render(nullptr, &u), false);
  }
  {
    // ---- sr_two_view (ABI 1.16): the workspace sweep, the planned shapes up to the launch, every rejection
    const uint64_t inf_bits = 0x7ff0000000000000ull, nan_bits = 0x7ff8000000000000ull;
    double inf64, nan64;
    std::memcpy(&inf64, &inf_bits, 8), std::memcpy(&nan64, &nan_bits, 8);
    {  // never shrinks when an argument grows; 0 for what the call rejects
      const int ps[] = {1, 3, 70, 240, 65535}, ks[] = {1, 8, 256, 257, 10000}, gs[] = {0, 1, 5}, hs[] = {0, 1, 65, 1024};
      for (int p : ps)
        for (int k : ks)
          for (int g : gs)
            for (int h : hs) {
              const int64_t b = sr_two_view_workspace(p, k, g, h);
              if (g + h == 0) {
                if (b != 0) ++g_fail;
                continue;
              }
              if (b <= 0 || b % 16 || b < 44 * (int64_t)p * k + 84 * (int64_t)p * (g + h)) ++g_fail;
              if (p < 65535 && sr_two_view_workspace(p + 1, k, g, h) < b) ++g_fail;
              if (sr_two_view_workspace(p, k + 1, g, h) < b || sr_two_view_workspace(p, k, g + 1, h) < b ||
                  sr_two_view_workspace(p, k, g, h + 1) < b)
                ++g_fail;
            }
      if (sr_two_view_workspace(0, 8, 0, 1) || sr_two_view_workspace(65536, 8, 0, 1) || sr_two_view_workspace(1, 0, 0, 1) ||
          sr_two_view_workspace(1, (1 << 24) + 1, 0, 1) || sr_two_view_workspace(65535, 1 << 16, 0, 1) ||
          sr_two_view_workspace(1, 8, -1, 1) || sr_two_view_workspace(1, 8, 0, -1) || sr_two_view_workspace(1, 8, 0, (1 << 20) + 1) ||
          sr_two_view_workspace(1, 8, (1 << 20) + 1, 0) || sr_two_view_workspace(65535, 32767, 1 << 20, 1 << 20) ||
          sr_two_view_workspace(1, 1 << 24, 0, 1) <= 0 || sr_two_view_workspace(65535, 1, 1 << 20, 0) <= 0)
        ++g_fail;
      std::printf("two-view workspace bytes at 240 x 10000, 1024 models: %lld\n", (long long)sr_two_view_workspace(240, 10000, 0, 1024));
    }
    sr_two_view_desc td{};
    td.src_coords = fake<float>(0), td.dst_coords = fake<float>(1), td.mask = fake<uint8_t>(2), td.intrinsic = fake<float>(3);
    td.src_idx = fake<int32_t>(4), td.dst_idx = fake<int32_t>(5), td.given_E = fake<double>(6), td.ref_extrinsic = fake<float>(7);
    td.n_views = 16, td.n_pairs = 240, td.n_points = 10000, td.n_given = 1, td.n_hyp = 1024, td.refine_iters = 8;
    td.threshold_px = 2.0, td.seed = 0x123456789abcdef0ull;
    td.E = fake<double>(8), td.R = fake<double>(9), td.t = fake<double>(10), td.cost = fake<double>(11);
    td.n_inliers = fake<uint32_t>(12), td.n_front = fake<uint32_t>(13), td.best = fake<int32_t>(14), td.refined = fake<int32_t>(15);
    td.status = fake<int32_t>(16), td.inlier_mask = fake<uint8_t>(17), td.pose_err = fake<double>(18), td.hyp_idx = fake<int32_t>(19);
    td.hyp_E = fake<double>(20), td.hyp_cost = fake<double>(21), td.hyp_inliers = fake<uint32_t>(22);
    td.workspace = fake(23), td.workspace_bytes = sr_two_view_workspace(240, 10000, 1, 1024);
    expect("sr_two_view 240 x 10000, every output", sr_two_view(nullptr, &td), true);
    sr_two_view_desc bare = td;
    bare.mask = nullptr, bare.given_E = nullptr, bare.n_given = 0, bare.ref_extrinsic = nullptr, bare.pose_err = nullptr;
    bare.R = nullptr, bare.t = nullptr, bare.cost = nullptr, bare.n_inliers = nullptr, bare.n_front = nullptr, bare.best = nullptr;
    bare.refined = nullptr, bare.status = nullptr, bare.inlier_mask = nullptr, bare.hyp_idx = nullptr, bare.hyp_E = nullptr;
    bare.hyp_cost = nullptr, bare.hyp_inliers = nullptr;
    expect("sr_two_view bare, E only", sr_two_view(nullptr, &bare), true);
    sr_two_view_desc u = bare;
    u.E = nullptr, u.status = td.status;
    expect("sr_two_view status only", sr_two_view(nullptr, &u), true);
    u = td, u.n_hyp = 0, u.n_given = 5, u.refine_iters = 0, u.workspace_bytes = sr_two_view_workspace(240, 10000, 5, 0);
    expect("sr_two_view given models only", sr_two_view(nullptr, &u), true);
    u = td, u.n_pairs = 1, u.n_points = 1, u.n_hyp = 1, u.n_given = 0, u.refine_iters = 32;
    expect("sr_two_view one pair, one point, one model", sr_two_view(nullptr, &u), true);
    u = td, u.n_pairs = 65535, u.n_points = 8, u.n_hyp = 1 << 20, u.n_given = 0, u.workspace_bytes = sr_two_view_workspace(65535, 8, 0, 1 << 20);
    expect("sr_two_view 65535 pairs, 2^20 hypotheses", sr_two_view(nullptr, &u), true);
    u = td, u.n_pairs = 1, u.n_points = 1 << 24, u.n_hyp = 64, u.workspace_bytes = sr_two_view_workspace(1, 1 << 24, 1, 64);
    expect("sr_two_view 2^24 correspondences", sr_two_view(nullptr, &u), true);
    u = td, u.threshold_px = 1e-300;
    expect("sr_two_view tiny threshold", sr_two_view(nullptr, &u), true);
    expect("sr_two_view null desc", sr_two_view(nullptr, nullptr), false);
    u = td, u.src_coords = nullptr;
    expect("sr_two_view null src_coords", sr_two_view(nullptr, &u), false);
    u = td, u.dst_coords = nullptr;
    expect("sr_two_view null dst_coords", sr_two_view(nullptr, &u), false);
    u = td, u.intrinsic = nullptr;
    expect("sr_two_view null intrinsic", sr_two_view(nullptr, &u), false);
    u = td, u.src_idx = nullptr;
    expect("sr_two_view null src_idx", sr_two_view(nullptr, &u), false);
    u = td, u.dst_idx = nullptr;
    expect("sr_two_view null dst_idx", sr_two_view(nullptr, &u), false);
    u = td, u.workspace = nullptr;
    expect("sr_two_view null workspace", sr_two_view(nullptr, &u), false);
    u = td, u.n_views = 0;
    expect("sr_two_view n_views 0", sr_two_view(nullptr, &u), false);
    u = td, u.n_pairs = 0;
    expect("sr_two_view n_pairs 0", sr_two_view(nullptr, &u), false);
    u = td, u.n_pairs = 65536, u.n_points = 8, u.workspace_bytes = int64_t(1) << 50;
    expect("sr_two_view n_pairs 65536", sr_two_view(nullptr, &u), false);
    u = td, u.n_points = 0;
    expect("sr_two_view n_points 0", sr_two_view(nullptr, &u), false);
    u = td, u.n_pairs = 1, u.n_points = (1 << 24) + 1, u.workspace_bytes = int64_t(1) << 50;
    expect("sr_two_view n_points 2^24 + 1", sr_two_view(nullptr, &u), false);
    u = td, u.n_pairs = 65535, u.n_points = 1 << 16, u.workspace_bytes = int64_t(1) << 50;
    expect("sr_two_view 2^31 correspondences and more", sr_two_view(nullptr, &u), false);
    u = td, u.n_given = -1;
    expect("sr_two_view n_given -1", sr_two_view(nullptr, &u), false);
    u = td, u.n_given = (1 << 20) + 1, u.workspace_bytes = int64_t(1) << 50;
    expect("sr_two_view n_given 2^20 + 1", sr_two_view(nullptr, &u), false);
    u = td, u.n_hyp = -1;
    expect("sr_two_view n_hyp -1", sr_two_view(nullptr, &u), false);
    u = td, u.n_hyp = (1 << 20) + 1, u.workspace_bytes = int64_t(1) << 50;
    expect("sr_two_view n_hyp 2^20 + 1", sr_two_view(nullptr, &u), false);
    u = td, u.n_given = 0, u.n_hyp = 0;
    expect("sr_two_view no model", sr_two_view(nullptr, &u), false);
    u = td, u.given_E = nullptr;
    expect("sr_two_view n_given without given_E", sr_two_view(nullptr, &u), false);
    u = td, u.refine_iters = -1;
    expect("sr_two_view refine_iters -1", sr_two_view(nullptr, &u), false);
    u = td, u.refine_iters = 33;
    expect("sr_two_view refine_iters 33", sr_two_view(nullptr, &u), false);
    u = td, u.threshold_px = 0.0;
    expect("sr_two_view threshold 0", sr_two_view(nullptr, &u), false);
    u = td, u.threshold_px = -2.0;
    expect("sr_two_view threshold -2", sr_two_view(nullptr, &u), false);
    u = td, u.threshold_px = nan64;
    expect("sr_two_view threshold NaN", sr_two_view(nullptr, &u), false);
    u = td, u.threshold_px = inf64;
    expect("sr_two_view threshold Inf", sr_two_view(nullptr, &u), false);
    u = td, u.n_pairs = 65535, u.n_points = 32767, u.n_given = 1 << 20, u.n_hyp = 1 << 20, u.workspace_bytes = int64_t(1) << 62;
    expect("sr_two_view partial sums beyond 2^36", sr_two_view(nullptr, &u), false);
    u = td, u.ref_extrinsic = nullptr;
    expect("sr_two_view pose_err without ref_extrinsic", sr_two_view(nullptr, &u), false);
    u = bare, u.E = nullptr;
    expect("sr_two_view no output", sr_two_view(nullptr, &u), false);
    u = bare, u.E = nullptr, u.hyp_idx = td.hyp_idx, u.n_hyp = 0, u.n_given = 1, u.given_E = td.given_E;
    expect("sr_two_view no output, hyp_idx without hypotheses", sr_two_view(nullptr, &u), false);
    u = td, u.workspace_bytes -= 1;
    expect("sr_two_view workspace one byte short", sr_two_view(nullptr, &u), false);
    u = td, u.workspace = (char*)fake(23) + 8;
    expect("sr_two_view workspace % 16", sr_two_view(nullptr, &u), false);
    u = td, u.given_E = (const double*)((const char*)fake(6) + 4);
    expect("sr_two_view given_E % 8", sr_two_view(nullptr, &u), false);
    u = td, u.hyp_cost = (double*)((char*)fake(21) + 4);
    expect("sr_two_view hyp_cost % 8", sr_two_view(nullptr, &u), false);
  }
  expect("sr_pose_decode_f32 null", sr_pose_decode_f32(nullptr, nullptr, 9, 0, 518, 518, nullptr, nullptr), false);
  expect("sr_copy_rows_f32 null", sr_copy_rows_f32(nullptr, nullptr, 0, nullptr, 0, nullptr, 0, 0), false);
  expect("sr_conv3x3_f32 null", sr_conv3x3_f32(nullptr, nullptr, 1, 8, 8, 32, 1, 0, nullptr, 32, SR_EPI_BIAS, &ep, nullptr, 32, nullptr), false);
  sr_weight_item wi{};
  expect("sr_weight_refresh_bf16 0 items", sr_weight_refresh_bf16(nullptr, 0, &wi), false);
  expect("sr_weight_refresh_bf16 no outputs", sr_weight_refresh_bf16(nullptr, 1, &wi), false);
  wi.src = fake<float>(0);
  wi.lds = 1024;
  wi.rows = 3072;
  wi.cols = 1024;
  wi.cast = fake(1);
  wi.ldc = 1024;
  wi.trans = fake(2);
  wi.ldt = 3072;
  expect("sr_weight_refresh_bf16", sr_weight_refresh_bf16(nullptr, 1, &wi), true);
  {
    sr_weight_item two[2] = {wi, wi};
    int start[3] = {-1, -1, -1};
    const int rc = sr_weight_refresh_plan(2, two, start);  // host-only: SR_OK
    const bool ok = rc == SR_OK && start[0] == 0 && start[1] == 768 && start[2] == 1536;
    std::printf("%-44s rc=%d  %sprefix %d %d %d\n", "sr_weight_refresh_plan", rc, ok ? "" : "UNEXPECTED  ", start[0],
                start[1], start[2]);
    if (!ok) ++g_fail;
    two[1].trans = nullptr;
    two[1].cast = nullptr;
    expect("sr_weight_refresh_plan no outputs", sr_weight_refresh_plan(2, two, start), false);
    expect("sr_weight_refresh_list_bf16 empty", sr_weight_refresh_list_bf16(nullptr, 0, nullptr, nullptr, 0), false);
  }
  expect("sr_im2col_normalize null", sr_im2col_normalize(nullptr, SR_BF16, nullptr, 0, 518, 518, 14, nullptr, nullptr, nullptr, 0), false);
  {
    // ---- sr_im2col_normalize_map / sr_frame_groups (ABI 1.8)
    const float m3[3] = {0.f, 0.f, 0.f}, s3[3] = {1.f, 1.f, 1.f};
    expect("sr_im2col_normalize_map null", sr_im2col_normalize_map(nullptr, SR_BF16, nullptr, fake<int32_t>(2), 2, 56, 56, 14, m3, s3, fake(3), 640), false);
    expect("sr_im2col_normalize_map H % patch", sr_im2col_normalize_map(nullptr, SR_BF16, fake<float>(1), fake<int32_t>(2), 2, 57, 56, 14, m3, s3, fake(3), 640), false);
    expect("sr_im2col_normalize_map kpad", sr_im2col_normalize_map(nullptr, SR_F32, fake<float>(1), fake<int32_t>(2), 2, 56, 56, 14, m3, s3, fake(3), 512), false);
    expect("sr_im2col_normalize_map dtype", sr_im2col_normalize_map(nullptr, 7, fake<float>(1), fake<int32_t>(2), 2, 56, 56, 14, m3, s3, fake(3), 640), false);
    expect("sr_im2col_normalize_map", sr_im2col_normalize_map(nullptr, SR_BF16, fake<float>(1), fake<int32_t>(2), 2, 56, 56, 14, m3, s3, fake(3), 640), true);
    const int64_t fw = 3 * 518 * 518;
    const int64_t need = sr_frame_groups_workspace(fw, 64);
    // 50 chunks of 16,384 words: 64 * (50 * 16 + 16 + 8) bytes
    const bool ws_ok = need == 64 * (50 * 16 + 24) && sr_frame_groups_workspace(1, 1) == 48 &&
                       sr_frame_groups_workspace(0, 4) == 0 && sr_frame_groups_workspace(fw, 0) == 0 &&
                       sr_frame_groups_workspace(fw, 65536) == 0 && sr_frame_groups_workspace(int64_t(1) << 31, 2) == 0;
    std::printf("%-44s %sbytes %lld\n", "sr_frame_groups_workspace", ws_ok ? "" : "UNEXPECTED  ", (long long)need);
    if (!ws_ok) ++g_fail;
    int32_t* rep = fake<int32_t>(5);
    expect("sr_frame_groups null frames", sr_frame_groups(nullptr, nullptr, fw, fw, 64, nullptr, rep, fake(6)), false);
    expect("sr_frame_groups null out", sr_frame_groups(nullptr, fake(4), fw, fw, 64, nullptr, nullptr, fake(6)), false);
    expect("sr_frame_groups null workspace", sr_frame_groups(nullptr, fake(4), fw, fw, 64, nullptr, rep, nullptr), false);
    expect("sr_frame_groups no frames", sr_frame_groups(nullptr, fake(4), fw, fw, 0, nullptr, rep, fake(6)), false);
    expect("sr_frame_groups too many frames", sr_frame_groups(nullptr, fake(4), fw, fw, 65536, nullptr, rep, fake(6)), false);
    expect("sr_frame_groups no words", sr_frame_groups(nullptr, fake(4), 0, fw, 2, nullptr, rep, fake(6)), false);
    expect("sr_frame_groups 2^31 words", sr_frame_groups(nullptr, fake(4), int64_t(1) << 31, int64_t(1) << 31, 2, nullptr, rep, fake(6)), false);
    expect("sr_frame_groups stride < words", sr_frame_groups(nullptr, fake(4), fw, fw - 1, 2, nullptr, rep, fake(6)), false);
    expect("sr_frame_groups frames % 4", sr_frame_groups(nullptr, (const char*)fake(4) + 2, fw, fw, 2, nullptr, rep, fake(6)), false);
    expect("sr_frame_groups workspace % 8", sr_frame_groups(nullptr, fake(4), fw, fw, 2, nullptr, rep, (char*)fake(6) + 4), false);
    expect("sr_frame_groups fp_override % 8", sr_frame_groups(nullptr, fake(4), fw, fw, 2, (const uint64_t*)((char*)fake(7) + 4), rep, fake(6)), false);
    expect("sr_frame_groups", sr_frame_groups(nullptr, (const char*)fake(4) + 4, fw, fw + 1, 64, nullptr, rep, fake(6)), true);
    expect("sr_frame_groups one frame, override", sr_frame_groups(nullptr, fake(4), 5, 0, 1, fake<uint64_t>(7), rep, fake(6)), true);
  }
}

}  // namespace

int main(int argc, char** argv) {
  const std::string mode = argc > 1 ? argv[1] : "check";
  if (mode == "layout") {
    if (argc > 2 && std::string(argv[2]) == "corres")
      layout_corres();
    else if (argc > 2 && std::string(argv[2]) == "pose_eval")
      layout_pose_eval();
    else if (argc > 2 && std::string(argv[2]) == "imc_stats")
      layout_imc_stats();
    else if (argc > 2 && std::string(argv[2]) == "cloud_eval")
      layout_cloud_eval();
    else if (argc > 2 && std::string(argv[2]) == "depth_eval")
      layout_depth_eval();
    else if (argc > 2 && std::string(argv[2]) == "cloud_voxel")
      layout_cloud_voxel();
    else if (argc > 2 && std::string(argv[2]) == "sparsify")
      layout_sparsify();
    else if (argc > 2 && std::string(argv[2]) == "cloud_render")
      layout_cloud_render();
    else if (argc > 2 && std::string(argv[2]) == "two_view")
      layout_two_view();
    else
      layout();
    return 0;
  }
  check();
  std::printf("%s: %d unexpected result(s)\n", g_fail ? "FAIL" : "OK", g_fail);
  return g_fail ? 1 : 0;
}
