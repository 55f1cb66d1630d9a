// Two-view relative poses from correspondences on gfx950: per pair of views a robust essential matrix (8-point
// hypotheses scored by a truncated pixel Sampson cost), its inliers, a reweighted refinement, and (R, t) by
// cheirality.  No ground truth is read; ref_extrinsic only feeds the optional pose_err.
//
// Contract (DESIGN.md "Two-view geometry", include/sfm_amd.h).  Everything is fp64 on fp32 inputs widened exactly,
// nothing is contracted, and everything that decides a result "to the bit" is an integer, a test on the bits or an
// IEEE fp64 operation in the order written here.
//   valid       mask byte non-zero and the four coordinates finite (on the bits); compacted per pair in index order
//   status      3: src_idx == dst_idx or an index outside [0, n_views) (tested first, nothing is loaded through it);
//               1: fewer than 8 valid; 2: no model with a finite cost; 0 otherwise
//   x^          x = (u - cx) / fx, y = (v - cy) / fy, true divisions; fx, fy, cx, cy = K[0], K[4], K[2], K[5]
//   sampling    mix = the splitmix64 finaliser; attempt a = 0, 1, ... of hypothesis h of pair p:
//               u = mix(seed + 0x9E3779B97F4A7C15 (((p 2^20 + h) 64 + a) + 1)) mod 2^64, j = ((u >> 32) n_valid) >> 32,
//               accepted if it differs from the slots already filled; void after 64 attempts
//   solve       S = A^T A of the 8 rows a = (x'x, x'y, x', y'x, y'y, y', x, y, 1); cyclic Jacobi; the eigenvector
//               of the smallest eigenvalue; projected to the essential manifold by essential_frames
//   score       ex_r = (E[3r] x + E[3r+1] y) + E[3r+2];  e = (x' ex_0 + y' ex_1) + ex_2;
//               et_c = (E[c] x' + E[3+c] y') + E[6+c] for c = 0, 1;
//               g = (((ex_0 ex_0) a_0 + (ex_1 ex_1) a_1) + (et_0 et_0) a_2) + (et_1 et_1) a_3 with
//               a = 1 / (fx_d fx_d), 1 / (fy_d fy_d), 1 / (fx_s fx_s), 1 / (fy_s fy_s);  r2 = (e e) / g
//   inlier      r2 < tau2 = tau tau (false for a NaN); the term of the cost is r2 for an inlier, tau2 otherwise
//   cost        chunks of TV_CHUNK = 256 consecutive valid correspondences: a chunk's terms are added to 0 one by
//               one in index order, the chunks' sums are added to 0 one by one in chunk order.  A model with a
//               non-finite entry has cost +Inf and 0 inliers.
//   selection   the minimum cost, ties to the lowest model index (given models first)
//   refinement  round k = 1 .. iters from the current iterate: w = (1 / (t t)) / g', t = 1 + r2 / s2, g' = g with
//               a = 1, s2 = 4 tau2 for k <= iters / 2 else tau2, w = 0 where it is not finite; M = sum w a a^T
//               (lane t adds i = t, t + 256, ... in order, then the fixed tree of sr::block_reduce); Jacobi, the
//               smallest eigenvector, projected; rescored.  The iterate moves on when the new model is finite.
//               The output is the first iterate with the lowest cost that is strictly below the selected model's.
//   decompose   essential_frames(E) gives U = (u1 u2 u3), V = (v1 v2 v3), both proper; W = rot_z(90 degrees);
//               candidates 0: (U W V^T, +u3), 1: (U W V^T, -u3), 2: (U W^T V^T, +u3), 3: (U W^T V^T, -u3);
//               a = R x^, b = x^', depths lambda = ((a.b)(b.t) - (b.b)(a.t)) / D, mu = ((a.a)(b.t) - (a.b)(a.t)) / D,
//               D = (a.a)(b.b) - (a.b)(a.b); in front: D > 0, lambda > 0 and mu > 0; counted over the inliers;
//               the largest count wins, ties to the lowest candidate.  X_dst = R X_src + t.
//   pose_err    R_ref = R_d R_s^T, t_ref = t_d - R_ref t_s; sr_pose_eval's atan2 formulas in fp64, degrees; the
//               translation angle is signed (no ambiguity) and a NaN when t_ref . t_ref == 0
//
//   tv_prep_kernel    one workgroup per pair: the status, the scan of the valid flags (sr::scan_row), the compacted
//                     indices and x^, the pair's four constants
//   tv_hyp_kernel     one lane per model: copies a given model, or draws, solves and projects
//   tv_score_kernel   the hot path.  grid (chunks, tiles of 256 models, pairs): the chunk's 256 (x, y, x', y') go
//                     through LDS (8 KiB), every lane keeps one model's 9 entries and the 4 constants in registers and
//                     walks the chunk by broadcast reads (all lanes read one address: two ds_read_b128, no
//                     conflict), one partial sum and count per (chunk, model).  Splitting K by chunks keeps P = 1
//                     busy (K = 10,000, 1,024 models: 160 workgroups) and P = 240 at 38,400.
//   tv_select_kernel  one workgroup per pair: the chunks' partial sums in chunk order, the argmin
//   tv_final_kernel   one workgroup per pair: refinement, the inlier mask, decomposition, pose error, the
//                     outputs of a pair without a result
// Integer atomics on LDS counters only, no float atomics, no workgroup waits on another; inputs are never written.
#include "sr_common.h"
#include "sr_eval.h"

namespace {

constexpr int TV_T = 256;      // threads of every workgroup but tv_hyp_kernel's
constexpr int TV_CHUNK = 256;  // valid correspondences per chunk of the cost (the contract's summation order)
constexpr int TV_HT = 64;      // lanes (models) per workgroup of tv_hyp_kernel: one wave, up to 512 VGPRs
constexpr int TV_MAX_PAIRS = 65535;
constexpr int TV_MAX_HYP = 1 << 20;
constexpr int TV_MAX_ITERS = 32;
constexpr int TV_MAX_K = 1 << 24;                // keeps every index sum here inside an int
constexpr int64_t TV_MAX_PK = 2147483647LL;      // P K
constexpr int64_t TV_MAX_PART = 1LL << 36;       // P (G + H) chunks: the partial sums, 12 bytes each

using sr::bits_nonfinite;
using sr::bits_nonfinite64;
using sr::finite64;

struct TvPlan {
  int n_models, n_chunks;
  int64_t off_st, off_nv, off_best, off_pc, off_idx, off_xn, off_rs, off_he, off_hc, off_hi, off_pcost, off_pinl, bytes;
};

bool tv_plan(int P, int K, int G, int H, TvPlan& p) {
  if (P < 1 || P > TV_MAX_PAIRS || K < 1 || K > TV_MAX_K || G < 0 || G > TV_MAX_HYP || H < 0 || H > TV_MAX_HYP || G + H < 1) return false;
  if ((int64_t)P * K > TV_MAX_PK) return false;
  p.n_models = G + H;
  p.n_chunks = (K + TV_CHUNK - 1) / TV_CHUNK;
  const int64_t pm = (int64_t)P * p.n_models;  // < 2^37
  if (pm > TV_MAX_PART / p.n_chunks) return false;
  const int64_t pk = (int64_t)P * K;
  int64_t o = 0;
  p.off_st = o, o += sr::align16(4 * (int64_t)P);
  p.off_nv = o, o += sr::align16(4 * (int64_t)P);
  p.off_best = o, o += sr::align16(4 * (int64_t)P);
  p.off_pc = o, o += 32 * (int64_t)P;
  p.off_idx = o, o += sr::align16(4 * pk);
  p.off_xn = o, o += 32 * pk;
  p.off_rs = o, o += sr::align16(8 * pk);
  p.off_he = o, o += sr::align16(72 * pm);
  p.off_hc = o, o += sr::align16(8 * pm);
  p.off_hi = o, o += sr::align16(4 * pm);
  p.off_pcost = o, o += sr::align16(8 * pm * p.n_chunks);
  p.off_pinl = o, o += sr::align16(4 * pm * p.n_chunks);
  p.bytes = o;
  return true;
}

struct TvArgs {
  sr_two_view_desc d;
  int n_models, n_chunks;
  double tau2;
  int32_t* st;       // [P]
  uint32_t* nv;      // [P] valid correspondences
  int32_t* best;     // [P]
  double* pc;        // [P][4] 1 / fx_d^2, 1 / fy_d^2, 1 / fx_s^2, 1 / fy_s^2
  int32_t* idx;      // [P][K] the valid correspondences, compacted
  double* xn;        // [P][K][4] x, y, x', y' of the compacted correspondences
  double* rs;        // [P][K] the cost's terms of the model being rescored
  double* he;        // [P][M][9] the caller's hyp_E, or the workspace's
  double* hc;        // [P][M] likewise hyp_cost
  uint32_t* hi;      // [P][M] likewise hyp_inliers
  double* pcost;     // [P][chunks][M]
  uint32_t* pinl;    // [P][chunks][M]
};

__device__ inline double qnan64() { return __longlong_as_double(0x7ff8000000000000LL); }
__device__ inline double pinf64() { return __longlong_as_double(0x7ff0000000000000LL); }

__device__ inline bool all_finite9(const double (&E)[9]) {
  bool ok = true;
#pragma unroll
  for (int k = 0; k < 9; ++k) ok = ok && !bits_nonfinite64(E[k]);
  return ok;
}

__device__ inline uint64_t mix64(uint64_t z) {
  z ^= z >> 30, z *= 0xBF58476D1CE4E5B9ull;
  z ^= z >> 27, z *= 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

// The contract's r2 of one correspondence under one model; gp is g with every focal length 1.
__device__ inline double sampson2(const double (&E)[9], double x, double y, double xp, double yp, const double (&a)[4],
                                  double& gp) {
  const double ex0 = (E[0] * x + E[1] * y) + E[2];
  const double ex1 = (E[3] * x + E[4] * y) + E[5];
  const double ex2 = (E[6] * x + E[7] * y) + E[8];
  const double e = (xp * ex0 + yp * ex1) + ex2;
  const double et0 = (E[0] * xp + E[3] * yp) + E[6];
  const double et1 = (E[1] * xp + E[4] * yp) + E[7];
  const double q0 = ex0 * ex0, q1 = ex1 * ex1, q2 = et0 * et0, q3 = et1 * et1;
  const double g = ((q0 * a[0] + q1 * a[1]) + q2 * a[2]) + q3 * a[3];
  gp = ((q0 + q1) + q2) + q3;
  return (e * e) / g;
}

// Cyclic Jacobi on the symmetric N x N matrix A (destroyed: its diagonal ends as the eigenvalues); V's columns are
// the eigenvectors.  Every index is a compile-time constant after unrolling, so A and V stay in registers.
template <int N>
__device__ inline void jacobi(double (&A)[N * N], double (&V)[N * N]) {
#pragma unroll
  for (int i = 0; i < N * N; ++i) V[i] = (i / N == i % N) ? 1.0 : 0.0;
  for (int sweep = 0; sweep < 16; ++sweep) {
    double off = 0.0, diag = 0.0;
#pragma unroll
    for (int p = 0; p < N; ++p) {
      diag += A[p * N + p] * A[p * N + p];
#pragma unroll
      for (int q = p + 1; q < N; ++q) off += A[p * N + q] * A[p * N + q];
    }
    if (!(off > 1e-40 * diag)) break;  // also leaves on a NaN
#pragma unroll
    for (int p = 0; p < N - 1; ++p) {
#pragma unroll
      for (int q = p + 1; q < N; ++q) {
        const double apq = A[p * N + q];
        if (apq != 0.0) {
          const double theta = (A[q * N + q] - A[p * N + p]) / (2.0 * apq);
          const double tt = (theta < 0.0 ? -1.0 : 1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
          const double c = 1.0 / sqrt(tt * tt + 1.0), s = tt * c;
#pragma unroll
          for (int k = 0; k < N; ++k) {
            const double akp = A[k * N + p], akq = A[k * N + q];
            A[k * N + p] = c * akp - s * akq, A[k * N + q] = s * akp + c * akq;
          }
#pragma unroll
          for (int k = 0; k < N; ++k) {
            const double apk = A[p * N + k], aqk = A[q * N + k];
            A[p * N + k] = c * apk - s * aqk, A[q * N + k] = s * apk + c * aqk;
          }
          A[p * N + q] = 0.0, A[q * N + p] = 0.0;
#pragma unroll
          for (int k = 0; k < N; ++k) {
            const double vkp = V[k * N + p], vkq = V[k * N + q];
            V[k * N + p] = c * vkp - s * vkq, V[k * N + q] = s * vkp + c * vkq;
          }
        }
      }
    }
  }
}

// The eigenvector of the smallest eigenvalue of the symmetric 9 x 9 S (destroyed), ties to the lowest column.
__device__ inline void smallest_eigenvector9(double (&S)[81], double (&e)[9]) {
  double V[81];
  jacobi<9>(S, V);
  int k = 0;
  double lo = S[0];
#pragma unroll
  for (int c = 1; c < 9; ++c)
    if (S[c * 9 + c] < lo) lo = S[c * 9 + c], k = c;
#pragma unroll
  for (int r = 0; r < 9; ++r) {
    double v = V[r * 9];
#pragma unroll
    for (int c = 1; c < 9; ++c) v = (c == k) ? V[r * 9 + c] : v;
    e[r] = v;
  }
}

__device__ inline void cross3(const double (&a)[3], const double (&b)[3], double (&o)[3]) {
  o[0] = a[1] * b[2] - a[2] * b[1], o[1] = a[2] * b[0] - a[0] * b[2], o[2] = a[0] * b[1] - a[1] * b[0];
}

// U = (u1 u2 u3) and V = (v1 v2 v3), as arrays of columns, of the 3 x 3 E: v1, v2 the eigenvectors of the two
// largest eigenvalues of E^T E (Jacobi), v3 = v1 x v2, u1 = E v1 / |E v1|, u2 = E v2 made orthogonal to u1 and
// scaled to length 1, u3 = u1 x u2.  u1 v1^T + u2 v2^T is E's nearest essential matrix of Frobenius norm sqrt 2.
__device__ inline void essential_frames(const double (&E)[9], double (&U)[3][3], double (&V)[3][3]) {
  double B[9], Q[9];
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int c = 0; c < 3; ++c) B[3 * r + c] = (E[r] * E[c] + E[3 + r] * E[3 + c]) + E[6 + r] * E[6 + c];
  jacobi<3>(B, Q);
  const double d0 = B[0], d1 = B[4], d2 = B[8];
  // the column of the smallest eigenvalue (ties to the highest column), the other two in column order
  const int lo = (d2 <= d0 && d2 <= d1) ? 2 : (d1 <= d0 ? 1 : 0);
  const int c1 = lo == 0 ? 1 : 0, c2 = lo == 2 ? 1 : 2;
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    V[0][r] = c1 == 0 ? Q[3 * r] : Q[3 * r + 1];
    V[1][r] = c2 == 1 ? Q[3 * r + 1] : Q[3 * r + 2];
  }
  cross3(V[0], V[1], V[2]);
  double w[3];
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    U[0][r] = (E[3 * r] * V[0][0] + E[3 * r + 1] * V[0][1]) + E[3 * r + 2] * V[0][2];
    w[r] = (E[3 * r] * V[1][0] + E[3 * r + 1] * V[1][1]) + E[3 * r + 2] * V[1][2];
  }
  const double n1 = sqrt((U[0][0] * U[0][0] + U[0][1] * U[0][1]) + U[0][2] * U[0][2]);
#pragma unroll
  for (int r = 0; r < 3; ++r) U[0][r] = U[0][r] / n1;
  const double dot = (U[0][0] * w[0] + U[0][1] * w[1]) + U[0][2] * w[2];
#pragma unroll
  for (int r = 0; r < 3; ++r) w[r] = w[r] - dot * U[0][r];
  const double n2 = sqrt((w[0] * w[0] + w[1] * w[1]) + w[2] * w[2]);
#pragma unroll
  for (int r = 0; r < 3; ++r) U[1][r] = w[r] / n2;
  cross3(U[0], U[1], U[2]);
}

// e (any 3 x 3) to the essential manifold; NaN in every entry if the result is not finite
__device__ inline void project_essential(const double (&e)[9], double (&E)[9]) {
  double U[3][3], V[3][3];
  essential_frames(e, U, V);
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int c = 0; c < 3; ++c) E[3 * r + c] = U[0][r] * V[0][c] + U[1][r] * V[1][c];
  if (!all_finite9(E)) {
#pragma unroll
    for (int k = 0; k < 9; ++k) E[k] = qnan64();
  }
}

// ---------------------------------------------------------------- valid correspondences, x^, the pair's constants
__global__ __launch_bounds__(TV_T) void tv_prep_kernel(TvArgs a) {
  __shared__ uint32_t s_scan[TV_T];
  const sr_two_view_desc& d = a.d;
  const int p = blockIdx.x, t = threadIdx.x, K = d.n_points;
  const int si = d.src_idx[p], di = d.dst_idx[p];
  if (si == di || si < 0 || si >= d.n_views || di < 0 || di >= d.n_views) {  // uniform
    if (t == 0) a.st[p] = 3, a.nv[p] = 0, a.best[p] = -1;
    return;
  }
  const float* Ks = d.intrinsic + 9 * (int64_t)si;
  const float* Kd = d.intrinsic + 9 * (int64_t)di;
  const double fxs = (double)Ks[0], fys = (double)Ks[4], cxs = (double)Ks[2], cys = (double)Ks[5];
  const double fxd = (double)Kd[0], fyd = (double)Kd[4], cxd = (double)Kd[2], cyd = (double)Kd[5];
  const int64_t row = (int64_t)p * K;
  const float* sc = d.src_coords + 2 * row;
  const float* dc = d.dst_coords + 2 * row;
  const uint8_t* mk = d.mask ? d.mask + row : nullptr;
  auto valid = [&](int i) -> uint32_t {
    if (mk && mk[i] == 0) return 0u;
    return (bits_nonfinite(sc[2 * i]) || bits_nonfinite(sc[2 * i + 1]) || bits_nonfinite(dc[2 * i]) ||
            bits_nonfinite(dc[2 * i + 1]))
               ? 0u
               : 1u;
  };
  int32_t* idx = a.idx + row;
  double* xn = a.xn + 4 * row;
  const uint32_t n = sr::scan_row<TV_T>(K, 0u, s_scan, valid, [&](int i, uint32_t at) {
    if (!valid(i)) return;  // at < K: the number of valid correspondences before i
    idx[at] = i;
    double* o = xn + 4 * (int64_t)at;
    o[0] = ((double)sc[2 * i] - cxs) / fxs, o[1] = ((double)sc[2 * i + 1] - cys) / fys;
    o[2] = ((double)dc[2 * i] - cxd) / fxd, o[3] = ((double)dc[2 * i + 1] - cyd) / fyd;
  });
  if (t == 0) {
    a.nv[p] = n, a.st[p] = n < 8u ? 1 : 0, a.best[p] = -1;
    double* pc = a.pc + 4 * (int64_t)p;
    pc[0] = 1.0 / (fxd * fxd), pc[1] = 1.0 / (fyd * fyd), pc[2] = 1.0 / (fxs * fxs), pc[3] = 1.0 / (fys * fys);
  }
}

// ---------------------------------------------------------------- models: given ones copied, the others drawn and solved
// grid (tiles of TV_HT models, pairs)
__global__ __launch_bounds__(TV_HT) void tv_hyp_kernel(TvArgs a) {
  const sr_two_view_desc& d = a.d;
  const int p = blockIdx.y, m = blockIdx.x * TV_HT + threadIdx.x, M = a.n_models, G = d.n_given;
  if (m >= M) return;
  double* out = a.he + 9 * ((int64_t)p * M + m);
  int32_t* hidx = (d.hyp_idx && m >= G) ? d.hyp_idx + 8 * ((int64_t)p * d.n_hyp + (m - G)) : nullptr;
  if (a.st[p] != 0) {  // no result for this pair: NaN / 0 / -1
    for (int k = 0; k < 9; ++k) out[k] = qnan64();
    a.hc[(int64_t)p * M + m] = qnan64(), a.hi[(int64_t)p * M + m] = 0u;
    if (hidx)
      for (int s = 0; s < 8; ++s) hidx[s] = -1;
    return;
  }
  if (m < G) {
    const double* src = d.given_E + 9 * ((int64_t)p * G + m);
    for (int k = 0; k < 9; ++k) out[k] = src[k];
    return;
  }
  const uint32_t nv = a.nv[p];  // >= 8
  const uint64_t base = (((uint64_t)p << 20) + (uint64_t)(m - G)) * 64ull;
  int32_t j[8] = {-1, -1, -1, -1, -1, -1, -1, -1};
  int filled = 0;
  for (int at = 0; at < 64 && filled < 8; ++at) {
    const uint64_t u = mix64(d.seed + 0x9E3779B97F4A7C15ull * (base + (uint64_t)at + 1ull));
    const int32_t c = (int32_t)(((u >> 32) * (uint64_t)nv) >> 32);  // in [0, nv)
    bool dup = false;
#pragma unroll
    for (int s = 0; s < 8; ++s) dup = dup || (s < filled && j[s] == c);
    if (!dup) {
#pragma unroll
      for (int s = 0; s < 8; ++s)
        if (s == filled) j[s] = c;
      ++filled;
    }
  }
  double E[9];
  if (filled < 8) {
#pragma unroll
    for (int k = 0; k < 9; ++k) E[k] = qnan64();
    if (hidx)
      for (int s = 0; s < 8; ++s) hidx[s] = -1;
  } else {
    const int64_t row = (int64_t)p * d.n_points;
    double S[81];
#pragma unroll
    for (int k = 0; k < 81; ++k) S[k] = 0.0;
#pragma unroll
    for (int s = 0; s < 8; ++s) {
      if (hidx) hidx[s] = a.idx[row + j[s]];
      const double* q = a.xn + 4 * (row + j[s]);
      const double x = q[0], y = q[1], xp = q[2], yp = q[3];
      const double r[9] = {xp * x, xp * y, xp, yp * x, yp * y, yp, x, y, 1.0};
#pragma unroll
      for (int b = 0; b < 9; ++b)
#pragma unroll
        for (int c = b; c < 9; ++c) S[9 * b + c] += r[b] * r[c];
    }
#pragma unroll
    for (int b = 1; b < 9; ++b)
#pragma unroll
      for (int c = 0; c < b; ++c) S[9 * b + c] = S[9 * c + b];
    double e[9];
    smallest_eigenvector9(S, e);
    project_essential(e, E);
  }
#pragma unroll
  for (int k = 0; k < 9; ++k) out[k] = E[k];
}

// ---------------------------------------------------------------- the hot path: every model against every correspondence
// grid (chunks, tiles of TV_T models, pairs)
__global__ __launch_bounds__(TV_T) void tv_score_kernel(TvArgs a) {
  __shared__ double4 s_x[TV_CHUNK];
  const int p = blockIdx.z, t = threadIdx.x, M = a.n_models;
  if (a.st[p] != 0) return;  // uniform
  const int nv = (int)a.nv[p], c0 = blockIdx.x * TV_CHUNK;
  if (c0 >= nv) return;  // uniform
  const int cnt = min(TV_CHUNK, nv - c0);
  const int64_t row = (int64_t)p * a.d.n_points;
  if (t < cnt) s_x[t] = reinterpret_cast<const double4*>(a.xn)[row + c0 + t];
  __syncthreads();
  const int m = blockIdx.y * TV_T + t;
  if (m >= M) return;
  const double* src = a.he + 9 * ((int64_t)p * M + m);
  double E[9];
#pragma unroll
  for (int k = 0; k < 9; ++k) E[k] = src[k];
  const double* pc = a.pc + 4 * (int64_t)p;
  const double f[4] = {pc[0], pc[1], pc[2], pc[3]};
  const double tau2 = a.tau2;
  double sum = 0.0;
  uint32_t inl = 0;
#pragma unroll 4
  for (int i = 0; i < cnt; ++i) {
    const double4 q = s_x[i];
    double gp;
    const double r2 = sampson2(E, q.x, q.y, q.z, q.w, f, gp);
    const bool in = r2 < tau2;
    sum += in ? r2 : tau2;
    inl += in ? 1u : 0u;
  }
  const int64_t o = ((int64_t)p * a.n_chunks + blockIdx.x) * M + m;
  a.pcost[o] = sum, a.pinl[o] = inl;
}

// ---------------------------------------------------------------- the chunks' sums in chunk order, the argmin
__global__ __launch_bounds__(TV_T) void tv_select_kernel(TvArgs a) {
  __shared__ double s_c[TV_T];
  __shared__ int s_m[TV_T];
  const int p = blockIdx.x, t = threadIdx.x, M = a.n_models;
  if (a.st[p] != 0) return;  // uniform
  const int nch = ((int)a.nv[p] + TV_CHUNK - 1) / TV_CHUNK;
  double bc = pinf64();
  int bm = -1;
  for (int m = t; m < M; m += TV_T) {
    const double* src = a.he + 9 * ((int64_t)p * M + m);
    double E[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) E[k] = src[k];
    double cost = 0.0;
    uint32_t inl = 0;
    for (int c = 0; c < nch; ++c) {
      const int64_t o = ((int64_t)p * a.n_chunks + c) * M + m;
      cost += a.pcost[o], inl += a.pinl[o];
    }
    if (!all_finite9(E)) cost = pinf64(), inl = 0u;
    a.hc[(int64_t)p * M + m] = cost, a.hi[(int64_t)p * M + m] = inl;
    if (cost < bc) bc = cost, bm = m;  // ascending m: the first of equal costs stays
  }
  s_c[t] = bc, s_m[t] = bm;
  __syncthreads();
  for (int s = TV_T / 2; s > 0; s >>= 1) {
    if (t < s) {
      const double oc = s_c[t + s];
      const int om = s_m[t + s];
      if (om >= 0 && (s_m[t] < 0 || oc < s_c[t] || (oc == s_c[t] && om < s_m[t]))) s_c[t] = oc, s_m[t] = om;
    }
    __syncthreads();
  }
  if (t == 0) {
    a.best[p] = s_m[0];
    if (s_m[0] < 0) a.st[p] = 2;
  }
}

// ---------------------------------------------------------------- refinement, mask, decomposition, pose error
// The contract's cost and inlier count of the model s_E over the pair's valid correspondences, in every thread;
// mask, if given, gets the inliers' bytes (the row is zero before).  s_red: TV_T doubles.
__device__ inline double rescore(const TvArgs& a, int p, int nv, const double* s_E, const double (&f)[4], double* s_red,
                                 uint32_t* s_cnt, uint8_t* mask, uint32_t& inliers) {
  const int t = threadIdx.x;
  const int64_t row = (int64_t)p * a.d.n_points;
  double E[9];
#pragma unroll
  for (int k = 0; k < 9; ++k) E[k] = s_E[k];
  __syncthreads();
  if (t == 0) *s_cnt = 0u;
  __syncthreads();
  uint32_t mine = 0;
  for (int i = t; i < nv; i += TV_T) {
    const double4 q = reinterpret_cast<const double4*>(a.xn)[row + i];
    double gp;
    const double r2 = sampson2(E, q.x, q.y, q.z, q.w, f, gp);
    const bool in = r2 < a.tau2;
    a.rs[row + i] = in ? r2 : a.tau2;
    mine += in ? 1u : 0u;
    if (mask && in) mask[a.idx[row + i]] = 1;
  }
  if (mine) atomicAdd(s_cnt, mine);
  __syncthreads();  // a workgroup's own global writes are visible to it after the barrier
  const int nch = (nv + TV_CHUNK - 1) / TV_CHUNK;
  double total = 0.0;  // thread 0's: chunk sums in chunk order, TV_T chunks per pass
  for (int c0 = 0; c0 < nch; c0 += TV_T) {
    const int c = c0 + t;
    double sum = 0.0;
    if (c < nch) {
      const int lo = c * TV_CHUNK, hi = min(nv, lo + TV_CHUNK);
      for (int i = lo; i < hi; ++i) sum += a.rs[row + i];
    }
    s_red[t] = sum;
    __syncthreads();
    if (t == 0)
      for (int k = 0; k < min(TV_T, nch - c0); ++k) total += s_red[k];
    __syncthreads();
  }
  if (t == 0) s_red[0] = total;
  __syncthreads();
  total = s_red[0];
  inliers = *s_cnt;
  __syncthreads();
  return total;
}

__device__ inline void store_nan(double* o, int n) {
  if (o)
    for (int k = 0; k < n; ++k) o[k] = qnan64();
}

__global__ __launch_bounds__(TV_T) void tv_final_kernel(TvArgs a) {
  __shared__ double s_red[15 * TV_T];
  __shared__ double s_M[45];
  __shared__ double s_E[9], s_best[9], s_R[2][9], s_t[3];
  __shared__ uint32_t s_cnt, s_front[4];
  const sr_two_view_desc& d = a.d;
  const int p = blockIdx.x, t = threadIdx.x, M = a.n_models, K = d.n_points;
  const int64_t row = (int64_t)p * K;
  uint8_t* mask = d.inlier_mask ? d.inlier_mask + row : nullptr;
  if (mask)
    for (int i = t; i < K; i += TV_T) mask[i] = 0;
  const int st = a.st[p];
  if (st != 0) {  // uniform: no result
    if (t == 0) {
      store_nan(d.E ? d.E + 9 * (int64_t)p : nullptr, 9), store_nan(d.R ? d.R + 9 * (int64_t)p : nullptr, 9);
      store_nan(d.t ? d.t + 3 * (int64_t)p : nullptr, 3), store_nan(d.cost ? d.cost + p : nullptr, 1);
      store_nan(d.pose_err ? d.pose_err + 2 * (int64_t)p : nullptr, 2);
      if (d.n_inliers) d.n_inliers[p] = 0u;
      if (d.n_front) d.n_front[p] = 0u;
      if (d.best) d.best[p] = -1;
      if (d.refined) d.refined[p] = -1;
      if (d.status) d.status[p] = st;
    }
    return;
  }
  const int nv = (int)a.nv[p], best = a.best[p];
  const double* pc = a.pc + 4 * (int64_t)p;
  const double f[4] = {pc[0], pc[1], pc[2], pc[3]};
  if (t < 9) s_E[t] = s_best[t] = a.he[9 * ((int64_t)p * M + best) + t];
  __syncthreads();
  uint32_t inl;
  double best_cost = rescore(a, p, nv, s_E, f, s_red, &s_cnt, nullptr, inl);  // = hyp_cost[best], bit for bit
  int refined = 0;
  for (int round = 1; round <= d.refine_iters; ++round) {
    const double s2 = round <= d.refine_iters / 2 ? 4.0 * a.tau2 : a.tau2;
    double E[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) E[k] = s_E[k];
    double acc[45];
#pragma unroll
    for (int k = 0; k < 45; ++k) acc[k] = 0.0;
    for (int i = t; i < nv; i += TV_T) {
      const double4 q = reinterpret_cast<const double4*>(a.xn)[row + i];
      double gp;
      const double r2 = sampson2(E, q.x, q.y, q.z, q.w, f, gp);
      const double tt = 1.0 + r2 / s2;
      double w = (1.0 / (tt * tt)) / gp;
      if (bits_nonfinite64(w)) w = 0.0;
      const double r[9] = {q.z * q.x, q.z * q.y, q.z, q.w * q.x, q.w * q.y, q.w, q.x, q.y, 1.0};
      int k = 0;
#pragma unroll
      for (int b = 0; b < 9; ++b) {
        const double wb = w * r[b];
#pragma unroll
        for (int c = b; c < 9; ++c) acc[k++] += wb * r[c];
      }
    }
#pragma unroll
    for (int pass = 0; pass < 3; ++pass) {
      double v[15];
#pragma unroll
      for (int k = 0; k < 15; ++k) v[k] = acc[15 * pass + k];
      sr::block_reduce<TV_T, 15>(v, s_red);
      if (t == 0)
#pragma unroll
        for (int k = 0; k < 15; ++k) s_M[15 * pass + k] = v[k];
    }
    __syncthreads();
    if (t == 0) {
      double S[81], e[9], En[9];
      int k = 0;
#pragma unroll
      for (int b = 0; b < 9; ++b)
#pragma unroll
        for (int c = b; c < 9; ++c) S[9 * b + c] = S[9 * c + b] = s_M[k++];
      smallest_eigenvector9(S, e);
      project_essential(e, En);
      const bool ok = all_finite9(En);
      s_cnt = ok ? 1u : 0u;
      if (ok)
#pragma unroll
        for (int c = 0; c < 9; ++c) s_E[c] = En[c];
    }
    __syncthreads();
    const bool ok = s_cnt != 0u;  // uniform
    __syncthreads();
    if (ok) {
      const double cost = rescore(a, p, nv, s_E, f, s_red, &s_cnt, nullptr, inl);
      if (cost < best_cost) {  // uniform
        best_cost = cost, refined = round;
        if (t < 9) s_best[t] = s_E[t];
      }
    }
    __syncthreads();
  }
  const double cost = rescore(a, p, nv, s_best, f, s_red, &s_cnt, mask, inl);
  // decomposition: thread 0 makes the two rotations and u3, every thread counts its inliers in front
  if (t == 0) {
    double E[9], U[3][3], V[3][3];
#pragma unroll
    for (int k = 0; k < 9; ++k) E[k] = s_best[k];
    essential_frames(E, U, V);
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        // U W V^T = -u2 v1^T + u1 v2^T + u3 v3^T;  U W^T V^T = u2 v1^T - u1 v2^T + u3 v3^T
        const double x = U[0][r] * V[1][c] - U[1][r] * V[0][c], z = U[2][r] * V[2][c];
        s_R[0][3 * r + c] = z + x, s_R[1][3 * r + c] = z - x;
      }
#pragma unroll
    for (int r = 0; r < 3; ++r) s_t[r] = U[2][r];
  }
  if (t < 4) s_front[t] = 0u;
  __syncthreads();
  {
    uint32_t front[4] = {0u, 0u, 0u, 0u};
    for (int i = t; i < nv; i += TV_T) {
      if (!(a.rs[row + i] < a.tau2)) continue;  // the terms of the last rescoring: an inlier's is r2 < tau2
      const double4 q = reinterpret_cast<const double4*>(a.xn)[row + i];
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const double* R = s_R[c >> 1];
        const double sg = (c & 1) ? -1.0 : 1.0;
        const double tv[3] = {sg * s_t[0], sg * s_t[1], sg * s_t[2]};
        double av[3];
#pragma unroll
        for (int r = 0; r < 3; ++r) av[r] = (R[3 * r] * q.x + R[3 * r + 1] * q.y) + R[3 * r + 2];
        const double aa = (av[0] * av[0] + av[1] * av[1]) + av[2] * av[2];
        const double bb = (q.z * q.z + q.w * q.w) + 1.0;
        const double ab = (av[0] * q.z + av[1] * q.w) + av[2];
        const double at = (av[0] * tv[0] + av[1] * tv[1]) + av[2] * tv[2];
        const double bt = (q.z * tv[0] + q.w * tv[1]) + tv[2];
        const double D = aa * bb - ab * ab;
        const double lam = (ab * bt - bb * at) / D, mu = (aa * bt - ab * at) / D;
        if (D > 0.0 && lam > 0.0 && mu > 0.0) ++front[c];
      }
    }
#pragma unroll
    for (int c = 0; c < 4; ++c)
      if (front[c]) atomicAdd(&s_front[c], front[c]);
  }
  __syncthreads();
  if (t == 0) {
    int win = 0;
    for (int c = 1; c < 4; ++c)
      if (s_front[c] > s_front[win]) win = c;
    const double* R = s_R[win >> 1];
    const double sg = (win & 1) ? -1.0 : 1.0;
    const double tv[3] = {sg * s_t[0], sg * s_t[1], sg * s_t[2]};
    if (d.E)
      for (int k = 0; k < 9; ++k) d.E[9 * (int64_t)p + k] = s_best[k];
    if (d.R)
      for (int k = 0; k < 9; ++k) d.R[9 * (int64_t)p + k] = R[k];
    if (d.t)
      for (int k = 0; k < 3; ++k) d.t[3 * (int64_t)p + k] = tv[k];
    if (d.cost) d.cost[p] = cost;
    if (d.n_inliers) d.n_inliers[p] = inl;
    if (d.n_front) d.n_front[p] = s_front[win];
    if (d.best) d.best[p] = best;
    if (d.refined) d.refined[p] = refined;
    if (d.status) d.status[p] = 0;
    if (d.pose_err) {
      const float* Es = d.ref_extrinsic + 12 * (int64_t)d.src_idx[p];
      const float* Ed = d.ref_extrinsic + 12 * (int64_t)d.dst_idx[p];
      double Rr[9], tr[3];
      for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c)
          Rr[3 * r + c] = ((double)Ed[4 * r] * (double)Es[4 * c] + (double)Ed[4 * r + 1] * (double)Es[4 * c + 1]) +
                          (double)Ed[4 * r + 2] * (double)Es[4 * c + 2];
      for (int r = 0; r < 3; ++r)
        tr[r] = (double)Ed[4 * r + 3] -
                ((Rr[3 * r] * (double)Es[3] + Rr[3 * r + 1] * (double)Es[7]) + Rr[3 * r + 2] * (double)Es[11]);
      double Q[9];  // R_ref^T R
      for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) Q[3 * r + c] = (Rr[r] * R[c] + Rr[3 + r] * R[3 + c]) + Rr[6 + r] * R[6 + c];
      const double vx = Q[7] - Q[5], vy = Q[2] - Q[6], vz = Q[3] - Q[1];
      const double sn = 0.5 * sqrt((vx * vx + vy * vy) + vz * vz), cs = 0.5 * (((Q[0] + Q[4]) + Q[8]) - 1.0);
      const double deg = 57.29577951308232;
      d.pose_err[2 * (int64_t)p] = atan2(sn, cs) * deg;
      double cr[3];
      cross3(tr, tv, cr);
      const double nn = (tr[0] * tr[0] + tr[1] * tr[1]) + tr[2] * tr[2];
      const double dt = (tr[0] * tv[0] + tr[1] * tv[1]) + tr[2] * tv[2];
      const double cn = sqrt((cr[0] * cr[0] + cr[1] * cr[1]) + cr[2] * cr[2]);
      d.pose_err[2 * (int64_t)p + 1] = nn == 0.0 ? qnan64() : atan2(cn, dt) * deg;
    }
  }
}

}  // namespace

extern "C" int64_t sr_two_view_workspace(int n_pairs, int n_points, int n_given, int n_hyp) {
  TvPlan p;
  return tv_plan(n_pairs, n_points, n_given, n_hyp, p) ? p.bytes : 0;
}

extern "C" int sr_two_view(sr_stream_t stream, const sr_two_view_desc* desc) {
  SR_CHECK(desc, SR_EINVAL, "sr_two_view: null desc");
  TvArgs a{};
  a.d = *desc;
  const sr_two_view_desc& d = a.d;
  SR_CHECK(d.src_coords && d.dst_coords && d.intrinsic && d.src_idx && d.dst_idx && d.workspace, SR_EINVAL,
           "sr_two_view: null src_coords, dst_coords, intrinsic, src_idx, dst_idx or workspace");
  SR_CHECK(d.n_views >= 1, SR_EINVAL, "sr_two_view: n_views %d below 1", d.n_views);
  SR_CHECK(d.n_pairs >= 1 && d.n_pairs <= TV_MAX_PAIRS, SR_EINVAL, "sr_two_view: n_pairs %d outside [1, %d]", d.n_pairs,
           TV_MAX_PAIRS);
  SR_CHECK(d.n_points >= 1 && d.n_points <= TV_MAX_K, SR_EINVAL, "sr_two_view: n_points %d outside [1, 2^24]", d.n_points);
  SR_CHECK((int64_t)d.n_pairs * d.n_points <= TV_MAX_PK, SR_EINVAL, "sr_two_view: %d x %d correspondences exceed 2^31 - 1",
           d.n_pairs, d.n_points);
  SR_CHECK(d.n_given >= 0 && d.n_given <= TV_MAX_HYP, SR_EINVAL, "sr_two_view: n_given %d outside [0, 2^20]", d.n_given);
  SR_CHECK(d.n_hyp >= 0 && d.n_hyp <= TV_MAX_HYP, SR_EINVAL, "sr_two_view: n_hyp %d outside [0, 2^20]", d.n_hyp);
  SR_CHECK(d.n_given + d.n_hyp >= 1, SR_EINVAL, "sr_two_view: no model (n_given + n_hyp is 0)");
  SR_CHECK(d.n_given == 0 || d.given_E, SR_EINVAL, "sr_two_view: n_given %d without given_E", d.n_given);
  SR_CHECK(d.refine_iters >= 0 && d.refine_iters <= TV_MAX_ITERS, SR_EINVAL, "sr_two_view: refine_iters %d outside [0, %d]",
           d.refine_iters, TV_MAX_ITERS);
  SR_CHECK(finite64(d.threshold_px) && d.threshold_px > 0.0, SR_EINVAL, "sr_two_view: threshold_px must be positive and finite");
  TvPlan p;
  SR_CHECK(tv_plan(d.n_pairs, d.n_points, d.n_given, d.n_hyp, p), SR_EINVAL,
           "sr_two_view: %d pairs x %d models x %d chunks of partial sums exceed 2^36", d.n_pairs, d.n_given + d.n_hyp,
           (d.n_points + TV_CHUNK - 1) / TV_CHUNK);
  SR_CHECK(!d.pose_err || d.ref_extrinsic, SR_EINVAL, "sr_two_view: pose_err without ref_extrinsic");
  SR_CHECK(d.E || d.R || d.t || d.cost || d.n_inliers || d.n_front || d.best || d.refined || d.status || d.inlier_mask ||
               d.pose_err || (d.hyp_idx && d.n_hyp > 0) || d.hyp_E || d.hyp_cost || d.hyp_inliers,
           SR_EINVAL, "sr_two_view: no output (every output pointer is null)");
  SR_CHECK_WORKSPACE("sr_two_view", d.workspace, d.workspace_bytes, p.bytes);
  SR_CHECK((((uintptr_t)d.given_E | (uintptr_t)d.E | (uintptr_t)d.R | (uintptr_t)d.t | (uintptr_t)d.cost | (uintptr_t)d.pose_err |
             (uintptr_t)d.hyp_E | (uintptr_t)d.hyp_cost) & 7) == 0,
           SR_EINVAL, "sr_two_view: given_E and the fp64 outputs must be 8-byte aligned");
  if (d.n_given == 0) a.d.given_E = nullptr;
  if (d.n_hyp == 0) a.d.hyp_idx = nullptr;
  a.n_models = p.n_models, a.n_chunks = p.n_chunks;
  a.tau2 = d.threshold_px * d.threshold_px;
  char* ws = (char*)d.workspace;
  a.st = (int32_t*)(ws + p.off_st), a.nv = (uint32_t*)(ws + p.off_nv), a.best = (int32_t*)(ws + p.off_best);
  a.pc = (double*)(ws + p.off_pc), a.idx = (int32_t*)(ws + p.off_idx), a.xn = (double*)(ws + p.off_xn);
  a.rs = (double*)(ws + p.off_rs);
  a.he = d.hyp_E ? d.hyp_E : (double*)(ws + p.off_he);
  a.hc = d.hyp_cost ? d.hyp_cost : (double*)(ws + p.off_hc);
  a.hi = d.hyp_inliers ? d.hyp_inliers : (uint32_t*)(ws + p.off_hi);
  a.pcost = (double*)(ws + p.off_pcost), a.pinl = (uint32_t*)(ws + p.off_pinl);
  hipStream_t s = (hipStream_t)stream;
  const unsigned P = (unsigned)d.n_pairs, M = (unsigned)p.n_models;
  hipLaunchKernelGGL(tv_prep_kernel, dim3(P), dim3(TV_T), 0, s, a);
  hipLaunchKernelGGL(tv_hyp_kernel, dim3((M + TV_HT - 1) / TV_HT, P), dim3(TV_HT), 0, s, a);
  hipLaunchKernelGGL(tv_score_kernel, dim3((unsigned)p.n_chunks, (M + TV_T - 1) / TV_T, P), dim3(TV_T), 0, s, a);
  hipLaunchKernelGGL(tv_select_kernel, dim3(P), dim3(TV_T), 0, s, a);
  hipLaunchKernelGGL(tv_final_kernel, dim3(P), dim3(TV_T), 0, s, a);
  sr::note_kernel("tv_score_kernel");
  return sr::check_launch("sr_two_view");
}
