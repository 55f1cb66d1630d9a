// Scoring predicted camera poses against ground truth on gfx950: pairwise relative rotation /
// translation errors with their histograms (RRA, RTA and AUC are read off the histogram on the host)
// and the similarity alignment of the camera centres (ATE).  The relative pose follows
// compute_relative_pose (train/utils/geometry.py:240-282) in closed form; the metrics are what the
// reference's demos hand to their `eval` package (train/demo_imc_forward.py:109-128), which is absent
// from the reference tree.
//
// Contract (DESIGN.md "Scoring poses"; poses are world-to-camera [R|t], 3x4 or 4x4 fp32 row-major, a
// view every `stride` = 12 or 16 floats, the R block used as given):
//   relative pose   R_ij = R_j R_i^T, t_ij = t_j - R_ij t_i
//   rotation error  E = (R^gt_ij)^T R^pr_ij, rot = atan2(|(E21-E12, E02-E20, E10-E01)| / 2, (tr E - 1) / 2)
//                   (never acos((tr E - 1) / 2): its fp32 error is 3e-2 degrees at errors <= 0.1 degrees)
//   translation     a = t^gt_ij, b = t^pr_ij, trans = atan2(|a x b|, a.b), |a.b| with trans_ambiguity;
//                   0 if a.a == 0 and b.b == 0; the worst case (180, or 90 with ambiguity) if exactly
//                   one of them is 0
//   histogram       uint32 hist[3][n_bins + 2], rows rot / trans / max(rot, trans): slot k < n_bins counts
//                   k <= fl32(err / bin_deg) < k + 1, slot n_bins the rest, slot n_bins + 1 the non-finite
//                   pairs: one of the four poses holds a NaN or an Inf (tested on the bits: the build
//                   compiles with -fno-honor-nans), an index outside [0, n_views) (nothing is loaded
//                   through it), or an error that itself evaluates to a non-finite value.  Their
//                   per-pair outputs are NaN.  Integer atomics only: independent of execution order.
//   pair sets       all i < j in lexicographic order, p = i (2N - i - 1) / 2 + (j - i - 1), or an explicit
//                   (pair_i, pair_j) list (any order, repeats allowed; i == j scores 0 / 0: T_i T_i^-1 is
//                   the identity, whatever rounding makes of R_i R_i^T)
//   alignment       centres c_k = -R_k^T t_k; Umeyama fit gt ~ s R pred + t over all views; everything in
//                   fp64 from the fp32 inputs, sums in a fixed order (a lane's views in ascending order,
//                   then a fixed tree), deviations taken from view 0's centre so that coincident centres
//                   give a variance of exactly 0; SVD of the 3x3 covariance by one-sided Jacobi
//                   rotations, the third left singular vector always u1 x u2 (never a column divided by
//                   its singular value), the second completed to a unit vector orthogonal to u1 when
//                   sigma_2 <= 1e-12 sigma_1
//
//   pose_hist_zero_kernel    clears hist
//   pose_pairs_tri_kernel    one workgroup per 64 x 64 tile of the pair triangle: both tiles' pred and gt
//                            poses staged in LDS, lane b of wave w keeps column b's poses in registers
//                            and walks rows w, w + 4, ...; LDS histogram, one global atomic per used slot
//   pose_pairs_list_kernel   the explicit list, 8 pairs per lane, poses gathered from global memory
//   pose_align_kernel        one workgroup, three passes over the views (means, covariance, residuals), each
//                            summed by sr::block_reduce (sr_eval.h)
#include "sr_common.h"
#include "sr_eval.h"

namespace {

using sr::bits_nonfinite;

constexpr int PE_T = 256;           // threads of every workgroup here
constexpr int TILE = 64;            // views per tile side
constexpr int PSTR = 13;            // LDS floats per staged pose (12 + 1: odd stride, conflict-free)
constexpr int MAX_BINS = 1024;
constexpr int HROW = MAX_BINS + 2;  // LDS histogram row
constexpr int LIST_RUN = 8;         // pairs per lane of the list kernel

struct Pose {
  float r[9], t[3];
};

__device__ inline Pose load_pose(const float* p) {
  Pose q;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
#pragma unroll
    for (int b = 0; b < 3; ++b) q.r[3 * a + b] = p[4 * a + b];
    q.t[a] = p[4 * a + 3];
  }
  return q;
}

__device__ inline Pose lds_pose(const float* p) {  // staged as r[9] | t[3]
  Pose q;
#pragma unroll
  for (int e = 0; e < 9; ++e) q.r[e] = p[e];
#pragma unroll
  for (int e = 0; e < 3; ++e) q.t[e] = p[9 + e];
  return q;
}

__device__ inline bool pose_nonfinite(const Pose& q) {
  bool bad = false;
#pragma unroll
  for (int e = 0; e < 9; ++e) bad |= bits_nonfinite(q.r[e]);
#pragma unroll
  for (int e = 0; e < 3; ++e) bad |= bits_nonfinite(q.t[e]);
  return bad;
}

// R_ij = R_j R_i^T, t_ij = t_j - R_ij t_i
__device__ inline Pose relative(const Pose& pi, const Pose& pj) {
  Pose o;
#pragma unroll
  for (int a = 0; a < 3; ++a)
#pragma unroll
    for (int c = 0; c < 3; ++c)
      o.r[3 * a + c] = pj.r[3 * a] * pi.r[3 * c] + pj.r[3 * a + 1] * pi.r[3 * c + 1] + pj.r[3 * a + 2] * pi.r[3 * c + 2];
#pragma unroll
  for (int a = 0; a < 3; ++a)
    o.t[a] = pj.t[a] - (o.r[3 * a] * pi.t[0] + o.r[3 * a + 1] * pi.t[1] + o.r[3 * a + 2] * pi.t[2]);
  return o;
}

// atan2 in degrees, rounded to fp32 once: the angle and the unit conversion in fp64 (an ulp of fp32 at
// 180 degrees is 1.5e-5 degrees, the size of the whole error budget of a pair)
__device__ inline float to_degrees(float y, float x) { return (float)(atan2((double)y, (double)x) * 57.29577951308232); }

// (rot, trans) in degrees of one pair; the four poses are finite
__device__ inline void pair_errors(const Pose& pr_i, const Pose& pr_j, const Pose& gt_i, const Pose& gt_j, bool ambiguity,
                                   float& rot, float& trans) {
  const Pose g = relative(gt_i, gt_j), p = relative(pr_i, pr_j);
  float E[9];  // E = Rg^T Rp
#pragma unroll
  for (int a = 0; a < 3; ++a)
#pragma unroll
    for (int c = 0; c < 3; ++c) E[3 * a + c] = g.r[a] * p.r[c] + g.r[3 + a] * p.r[3 + c] + g.r[6 + a] * p.r[6 + c];
  const float vx = E[7] - E[5], vy = E[2] - E[6], vz = E[3] - E[1];
  const float s = 0.5f * sqrtf(vx * vx + vy * vy + vz * vz);
  const float c = 0.5f * (E[0] + E[4] + E[8] - 1.0f);
  rot = to_degrees(s, c);
  const float* a = g.t;
  const float* b = p.t;
  const float aa = a[0] * a[0] + a[1] * a[1] + a[2] * a[2], bb = b[0] * b[0] + b[1] * b[1] + b[2] * b[2];
  if (aa == 0.0f || bb == 0.0f) {
    trans = (aa == 0.0f && bb == 0.0f) ? 0.0f : (ambiguity ? 90.0f : 180.0f);
    return;
  }
  const float cx = a[1] * b[2] - a[2] * b[1], cy = a[2] * b[0] - a[0] * b[2], cz = a[0] * b[1] - a[1] * b[0];
  const float d = a[0] * b[0] + a[1] * b[1] + a[2] * b[2];
  trans = to_degrees(sqrtf(cx * cx + cy * cy + cz * cz), ambiguity ? fabsf(d) : d);
}

// Run-length front of one lane's LDS histogram adds: consecutive pairs mostly share a slot.
struct SlotRun {
  int slot = -1;
  uint32_t n = 0;
  __device__ inline void add(uint32_t* row, int s) {
    if (s == slot) {
      ++n;
      return;
    }
    flush(row);
    slot = s;
    n = 1;
  }
  __device__ inline void flush(uint32_t* row) {
    if (n) atomicAdd(&row[slot], n);
    n = 0;
  }
};

struct PairOut {
  float rot, trans;
  int s_rot, s_trans, s_max;
};

// errors and the three slots of one pair; `bad`: a pose is non-finite or an index out of range
__device__ inline PairOut score(bool bad, const Pose& pr_i, const Pose& pr_j, const Pose& gt_i, const Pose& gt_j,
                                const sr_pose_pairs_desc& d) {
  PairOut o;
  if (!bad) {
    pair_errors(pr_i, pr_j, gt_i, gt_j, d.trans_ambiguity != 0, o.rot, o.trans);
    bad = bits_nonfinite(o.rot) || bits_nonfinite(o.trans);
  }
  if (bad) {
    o.rot = o.trans = sr::quiet_nan();
    o.s_rot = o.s_trans = o.s_max = d.n_bins + 1;
    return o;
  }
  o.s_rot = sr::hist_slot(o.rot, d.bin_deg, d.n_bins);
  o.s_trans = sr::hist_slot(o.trans, d.bin_deg, d.n_bins);
  o.s_max = max(o.s_rot, o.s_trans);  // the slot is monotone in the error
  return o;
}

// sr::hist_flush for three rows at once: HROW apart in LDS, packed in the global histogram
__device__ inline void hist_flush(const uint32_t* s_hist, uint32_t* hist, int n_slots) {
  for (int e = threadIdx.x; e < 3 * n_slots; e += PE_T) {
    const int row = e / n_slots, k = e - row * n_slots;
    const uint32_t v = s_hist[row * HROW + k];
    if (v) atomicAdd(&hist[e], v);
  }
}

__global__ __launch_bounds__(PE_T) void pose_hist_zero_kernel(uint32_t* hist, int n) {
  const int e = blockIdx.x * PE_T + threadIdx.x;
  if (e < n) hist[e] = 0;
}

// ---------------------------------------------------------------- all pairs i < j
__global__ __launch_bounds__(PE_T) void pose_pairs_tri_kernel(sr_pose_pairs_desc d) {
  const int ti = blockIdx.y, tj = blockIdx.x;
  if (ti > tj) return;  // below the diagonal: uniform per workgroup
  __shared__ float s_pose[4][TILE * PSTR];  // pred i-tile, gt i-tile, pred j-tile, gt j-tile
  __shared__ int s_bad[2][TILE];            // per view of the i-tile / j-tile: a non-finite pose
  __shared__ uint32_t s_hist[3 * HROW];
  const int t = threadIdx.x, N = d.n_views, n_slots = d.n_bins + 2;
  sr::hist_clear<PE_T>(s_hist, 3 * HROW);
  for (int e = t; e < 4 * TILE * 12; e += PE_T) {
    const int arr = e / (TILE * 12), rem = e - arr * (TILE * 12), v = rem / 12, c = rem - v * 12;
    const int view = ((arr & 2) ? tj : ti) * TILE + v;
    float x = 0.0f;
    if (view < N) {
      const float* base = (arr & 1) ? d.gt + (int64_t)view * d.gt_stride : d.pred + (int64_t)view * d.pred_stride;
      x = base[c];
    }
    // [R|t] row-major -> r[9] | t[3]
    const int row = c >> 2, col = c & 3;
    s_pose[arr][v * PSTR + (col == 3 ? 9 + row : 3 * row + col)] = x;
  }
  __syncthreads();
  if (t < 2 * TILE) {
    const int side = t / TILE, v = t - side * TILE;
    bool bad = false;
    for (int c = 0; c < 12; ++c)
      bad |= bits_nonfinite(s_pose[2 * side][v * PSTR + c]) || bits_nonfinite(s_pose[2 * side + 1][v * PSTR + c]);
    s_bad[side][v] = bad;
  }
  __syncthreads();
  const int b = t & (TILE - 1), w = t / TILE;  // column of the j-tile; first row of the i-tile
  const int j = tj * TILE + b;
  const Pose pr_j = lds_pose(&s_pose[2][b * PSTR]), gt_j = lds_pose(&s_pose[3][b * PSTR]);
  const bool bad_j = s_bad[1][b] != 0;
  SlotRun run_rot, run_trans, run_max;
  for (int a = w; a < TILE; a += PE_T / TILE) {
    const int i = ti * TILE + a;
    if (i >= N) break;            // uniform per wave
    if (j >= N || i >= j) continue;
    const Pose pr_i = lds_pose(&s_pose[0][a * PSTR]), gt_i = lds_pose(&s_pose[1][a * PSTR]);  // broadcast reads
    const PairOut o = score(bad_j || s_bad[0][a] != 0, pr_i, pr_j, gt_i, gt_j, d);
    run_rot.add(s_hist, o.s_rot);
    run_trans.add(s_hist + HROW, o.s_trans);
    run_max.add(s_hist + 2 * HROW, o.s_max);
    if (d.rot_err || d.trans_err) {
      const int64_t p = (int64_t)i * (2 * (int64_t)N - i - 1) / 2 + (j - i - 1);
      if (d.rot_err) d.rot_err[p] = o.rot;
      if (d.trans_err) d.trans_err[p] = o.trans;
    }
  }
  run_rot.flush(s_hist);
  run_trans.flush(s_hist + HROW);
  run_max.flush(s_hist + 2 * HROW);
  __syncthreads();
  hist_flush(s_hist, d.hist, n_slots);
}

// ---------------------------------------------------------------- an explicit pair list
__global__ __launch_bounds__(PE_T) void pose_pairs_list_kernel(sr_pose_pairs_desc d) {
  __shared__ uint32_t s_hist[3 * HROW];
  const int t = threadIdx.x, N = d.n_views, n_slots = d.n_bins + 2;
  sr::hist_clear<PE_T>(s_hist, 3 * HROW);
  __syncthreads();
  SlotRun run_rot, run_trans, run_max;
  const int64_t base = (int64_t)blockIdx.x * (LIST_RUN * PE_T);
#pragma unroll 1
  for (int k = 0; k < LIST_RUN; ++k) {
    const int64_t p = base + (int64_t)k * PE_T + t;
    if (p >= d.n_pairs) break;
    const int i = d.pair_i[p], j = d.pair_j[p];
    bool bad = i < 0 || i >= N || j < 0 || j >= N;
    Pose pr_i = {}, pr_j = {}, gt_i = {}, gt_j = {};
    if (!bad) {  // nothing is loaded through an index out of range
      pr_i = load_pose(d.pred + (int64_t)i * d.pred_stride);
      pr_j = load_pose(d.pred + (int64_t)j * d.pred_stride);
      gt_i = load_pose(d.gt + (int64_t)i * d.gt_stride);
      gt_j = load_pose(d.gt + (int64_t)j * d.gt_stride);
      bad = pose_nonfinite(pr_i) || pose_nonfinite(pr_j) || pose_nonfinite(gt_i) || pose_nonfinite(gt_j);
    }
    PairOut o = score(bad, pr_i, pr_j, gt_i, gt_j, d);
    if (i == j && !bad) {  // T_i T_i^-1 is the identity, whatever rounding makes of R R^T
      o.rot = o.trans = 0.0f;
      o.s_rot = o.s_trans = o.s_max = 0;
    }
    run_rot.add(s_hist, o.s_rot);
    run_trans.add(s_hist + HROW, o.s_trans);
    run_max.add(s_hist + 2 * HROW, o.s_max);
    if (d.rot_err) d.rot_err[p] = o.rot;
    if (d.trans_err) d.trans_err[p] = o.trans;
  }
  run_rot.flush(s_hist);
  run_trans.flush(s_hist + HROW);
  run_max.flush(s_hist + 2 * HROW);
  __syncthreads();
  hist_flush(s_hist, d.hist, n_slots);
}

// ---------------------------------------------------------------- alignment
// c = -R^T t in fp64 (the products of fp32 values are exact)
__device__ inline void centre(const float* p, double c[3]) {
#pragma unroll
  for (int a = 0; a < 3; ++a)
    c[a] = -((double)p[a] * (double)p[3] + (double)p[4 + a] * (double)p[7] + (double)p[8 + a] * (double)p[11]);
}

__device__ inline double dot3(const double* a, const double* b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }
__device__ inline void cross3(const double* a, const double* b, double* o) {
  o[0] = a[1] * b[2] - a[2] * b[1];
  o[1] = a[2] * b[0] - a[0] * b[2];
  o[2] = a[0] * b[1] - a[1] * b[0];
}

// Rotation R (row-major) and sum of the sign-fixed singular values of the Umeyama fit for the
// covariance S = mean (g - mg)(p - mp)^T (row-major); returns the rank class: 0 (S == 0), 1 or 2 (>= 2).
__device__ int umeyama_rotation(const double S[9], double R[9], double& sigma_sum) {
  double A[3][3], V[3][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}};  // columns A[c], V[c]: S V = A
  double big = 0.0;
  for (int e = 0; e < 9; ++e) big = fmax(big, fabs(S[e]));
  for (int e = 0; e < 9; ++e) R[e] = (e % 4 == 0) ? 1.0 : 0.0;
  sigma_sum = 0.0;
  if (!(big > 0.0)) return 0;
  for (int c = 0; c < 3; ++c)
    for (int r = 0; r < 3; ++r) A[c][r] = S[3 * r + c] / big;
  for (int sweep = 0; sweep < 30; ++sweep) {  // one-sided Jacobi: rotate column pairs until orthogonal
    bool rotated = false;
    for (int p = 0; p < 2; ++p)
      for (int q = p + 1; q < 3; ++q) {
        const double alpha = dot3(A[p], A[p]), beta = dot3(A[q], A[q]), gamma = dot3(A[p], A[q]);
        if (!(fabs(gamma) > 1e-16 * sqrt(alpha * beta))) continue;
        rotated = true;
        const double zeta = (beta - alpha) / (2.0 * gamma);
        const double tn = (zeta >= 0.0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
        const double cs = 1.0 / sqrt(1.0 + tn * tn), sn = cs * tn;
        for (int r = 0; r < 3; ++r) {
          const double ap = A[p][r], aq = A[q][r], vp = V[p][r], vq = V[q][r];
          A[p][r] = cs * ap - sn * aq;
          A[q][r] = sn * ap + cs * aq;
          V[p][r] = cs * vp - sn * vq;
          V[q][r] = sn * vp + cs * vq;
        }
      }
    if (!rotated) break;
  }
  double sig[3];
  int ord[3] = {0, 1, 2};
  for (int c = 0; c < 3; ++c) sig[c] = sqrt(dot3(A[c], A[c]));
  for (int a = 0; a < 2; ++a)  // descending
    for (int b = 0; b < 2 - a; ++b)
      if (sig[ord[b]] < sig[ord[b + 1]]) {
        const int tmp = ord[b];
        ord[b] = ord[b + 1];
        ord[b + 1] = tmp;
      }
  const double *a1 = A[ord[0]], *a2 = A[ord[1]], *a3 = A[ord[2]];
  const double *v1 = V[ord[0]], *v2 = V[ord[1]], *v3 = V[ord[2]];
  const double s1 = sig[ord[0]], s2 = sig[ord[1]], s3 = sig[ord[2]];
  if (!(s1 > 0.0)) return 0;
  double u1[3], u2[3], u3[3], vx[3];
  for (int r = 0; r < 3; ++r) u1[r] = a1[r] / s1;
  const int rank = s2 > 1e-12 * s1 ? 2 : 1;
  if (rank == 2) {
    for (int r = 0; r < 3; ++r) u2[r] = a2[r];
  } else {  // complete u1 to a basis: the axis least aligned with it
    int ax = fabs(u1[0]) <= fabs(u1[1]) ? 0 : 1;
    if (fabs(u1[2]) < fabs(u1[ax])) ax = 2;
    for (int r = 0; r < 3; ++r) u2[r] = (r == ax ? 1.0 : 0.0);
  }
  const double along = dot3(u1, u2);  // Gram-Schmidt against u1 (a rounding-sized step for rank 2)
  for (int r = 0; r < 3; ++r) u2[r] -= along * u1[r];
  const double n2 = sqrt(dot3(u2, u2));
  for (int r = 0; r < 3; ++r) u2[r] /= n2;
  cross3(u1, u2, u3);
  const double n3 = sqrt(dot3(u3, u3));
  for (int r = 0; r < 3; ++r) u3[r] /= n3;
  cross3(v1, v2, vx);
  const double det_v = dot3(vx, v3) >= 0.0 ? 1.0 : -1.0;
  // the true third left vector is +-u3 with the sign of u3 . a3 (= det U); d = det U det V multiplies
  // it in R, so R needs det V alone and only the singular-value sum needs det U
  const double det_u = dot3(u3, a3) >= 0.0 ? 1.0 : -1.0;
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) R[3 * r + c] = u1[r] * v1[c] + u2[r] * v2[c] + det_v * u3[r] * v3[c];
  sigma_sum = (s1 + s2 + det_u * det_v * s3) * big;
  return rank;
}

__global__ __launch_bounds__(PE_T) void pose_align_kernel(sr_pose_align_desc d) {
  __shared__ double s_red[10 * PE_T];
  __shared__ double s_fit[13];  // scale, R[9], t[3]
  const int t = threadIdx.x, N = d.n_views;
  double p0[3], g0[3];  // view 0's centres: the origin the deviations are taken from
  centre(d.pred, p0);
  centre(d.gt, g0);
  // ---- means
  double acc[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (int k = t; k < N; k += PE_T) {
    double p[3], g[3];
    centre(d.pred + (int64_t)k * d.pred_stride, p);
    centre(d.gt + (int64_t)k * d.gt_stride, g);
    for (int a = 0; a < 3; ++a) {
      acc[a] += p[a] - p0[a];
      acc[3 + a] += g[a] - g0[a];
    }
  }
  sr::block_reduce<PE_T>(acc, s_red);
  for (int e = 0; e < 6; ++e) acc[e] /= (double)N;
  double mp[3], mg[3];
  for (int a = 0; a < 3; ++a) {
    mp[a] = p0[a] + acc[a];
    mg[a] = g0[a] + acc[3 + a];
  }
  // ---- variance of the predicted centres and the covariance
  double cov[10];
  for (int e = 0; e < 10; ++e) cov[e] = 0.0;
  for (int k = t; k < N; k += PE_T) {
    double p[3], g[3];
    centre(d.pred + (int64_t)k * d.pred_stride, p);
    centre(d.gt + (int64_t)k * d.gt_stride, g);
    for (int a = 0; a < 3; ++a) {
      p[a] -= mp[a];
      g[a] -= mg[a];
    }
    for (int r = 0; r < 3; ++r)
      for (int c = 0; c < 3; ++c) cov[3 * r + c] += g[r] * p[c];
    cov[9] += dot3(p, p);
  }
  sr::block_reduce<PE_T>(cov, s_red);
  for (int e = 0; e < 10; ++e) cov[e] /= (double)N;
  if (t == 0) {
    double R[9], sigma_sum, scale = 1.0;
    int status = 0;
    if (!(cov[9] > 0.0)) {  // coincident predicted centres
      status = 3;
      for (int e = 0; e < 9; ++e) R[e] = (e % 4 == 0) ? 1.0 : 0.0;
    } else {
      const int rank = umeyama_rotation(cov, R, sigma_sum);
      if (rank < 2) status = 2;
      if (d.with_scale) scale = sigma_sum / cov[9];
    }
    s_fit[0] = scale;
    for (int e = 0; e < 9; ++e) s_fit[1 + e] = R[e];
    for (int r = 0; r < 3; ++r) s_fit[10 + r] = mg[r] - scale * dot3(&R[3 * r], mp);
    for (int e = 0; e < 13; ++e) d.out[e] = s_fit[e];
    *d.status = status;
  }
  __syncthreads();
  // ---- residuals
  double sq[1] = {0.0};
  for (int k = t; k < N; k += PE_T) {
    double p[3], g[3], e2 = 0.0;
    centre(d.pred + (int64_t)k * d.pred_stride, p);
    centre(d.gt + (int64_t)k * d.gt_stride, g);
    for (int r = 0; r < 3; ++r) {
      const double diff = g[r] - (s_fit[0] * dot3(&s_fit[1 + 3 * r], p) + s_fit[10 + r]);
      e2 += diff * diff;
    }
    sq[0] += e2;
    if (d.err) d.err[k] = sqrt(e2);
  }
  sr::block_reduce<PE_T>(sq, s_red);
  if (t == 0) d.out[13] = sqrt(sq[0] / (double)N);
}

bool stride_ok(int s) { return s == 12 || s == 16; }

}  // namespace

extern "C" int sr_pose_pair_errors(sr_stream_t stream, const sr_pose_pairs_desc* desc) {
  SR_CHECK(desc, SR_EINVAL, "sr_pose_pair_errors: null desc");
  const sr_pose_pairs_desc& d = *desc;
  SR_CHECK(d.pred && d.gt && d.hist, SR_EINVAL, "sr_pose_pair_errors: null pointer");
  SR_CHECK(d.n_views > 0 && d.n_views <= 65535, SR_EINVAL, "sr_pose_pair_errors: n_views %d outside [1, 65535]",
           d.n_views);
  SR_CHECK(stride_ok(d.pred_stride) && stride_ok(d.gt_stride), SR_EINVAL,
           "sr_pose_pair_errors: strides %d / %d must be 12 or 16 floats", d.pred_stride, d.gt_stride);
  SR_CHECK(d.n_bins > 0 && d.n_bins <= MAX_BINS, SR_EINVAL, "sr_pose_pair_errors: n_bins %d outside [1, %d]", d.n_bins,
           MAX_BINS);
  SR_CHECK(sr::positive_finite(d.bin_deg), SR_EINVAL, "sr_pose_pair_errors: bin_deg must be positive and finite");
  SR_CHECK((d.pair_i != nullptr) == (d.pair_j != nullptr), SR_EINVAL,
           "sr_pose_pair_errors: pair_i and pair_j go together");
  SR_CHECK(!d.pair_i || d.n_pairs > 0, SR_EINVAL, "sr_pose_pair_errors: a pair list of %d entries", d.n_pairs);
  hipStream_t s = (hipStream_t)stream;
  const int n_hist = 3 * (d.n_bins + 2);
  hipLaunchKernelGGL(pose_hist_zero_kernel, dim3((n_hist + PE_T - 1) / PE_T), dim3(PE_T), 0, s, d.hist, n_hist);
  if (d.pair_i) {
    const int per_block = LIST_RUN * PE_T;
    hipLaunchKernelGGL(pose_pairs_list_kernel, dim3((unsigned)(((int64_t)d.n_pairs + per_block - 1) / per_block)), dim3(PE_T), 0, s, d);
    sr::note_kernel("pose_pairs_list_kernel");
  } else {
    const int nt = (d.n_views + TILE - 1) / TILE;
    hipLaunchKernelGGL(pose_pairs_tri_kernel, dim3(nt, nt), dim3(PE_T), 0, s, d);
    sr::note_kernel("pose_pairs_tri_kernel");
  }
  return sr::check_launch("sr_pose_pair_errors");
}

extern "C" int sr_pose_align(sr_stream_t stream, const sr_pose_align_desc* desc) {
  SR_CHECK(desc, SR_EINVAL, "sr_pose_align: null desc");
  const sr_pose_align_desc& d = *desc;
  SR_CHECK(d.pred && d.gt && d.out && d.status, SR_EINVAL, "sr_pose_align: null pointer");
  SR_CHECK(d.n_views > 0 && d.n_views <= 65535, SR_EINVAL, "sr_pose_align: n_views %d outside [1, 65535]", d.n_views);
  SR_CHECK(stride_ok(d.pred_stride) && stride_ok(d.gt_stride), SR_EINVAL,
           "sr_pose_align: strides %d / %d must be 12 or 16 floats", d.pred_stride, d.gt_stride);
  SR_CHECK(((uintptr_t)d.out & 7) == 0 && ((uintptr_t)d.err & 7) == 0, SR_EINVAL,
           "sr_pose_align: fp64 buffers must be 8-byte aligned");
  hipLaunchKernelGGL(pose_align_kernel, dim3(1), dim3(PE_T), 0, (hipStream_t)stream, d);
  sr::note_kernel("pose_align_kernel");
  return sr::check_launch("sr_pose_align");
}
