// Self-supervised IMC training loss on gfx950: compute_loss
// (train/train_imc.py:141-246) = pose decode (pose_enc.py:68-135) -> K' -> K recovery (+ shared
// focal averaging) -> relative poses -> backproject / reproject (exact and fixed-depth variants,
// train/utils/geometry.py:89-303) -> log1p residuals -> CDFLossIndexPytorch (per-node weighted
// histograms, CDF, Sobel + Gaussian PDF, lookup; train/losses/cdf_loss.py:88-242), forward value
// AND its gradient with respect to the pose encodings, in one call:
//
//   imc_views_kernel   per view: K (FoV), Kr = K'K, E = [R(q) | T]             (1 workgroup)
//   imc_pairs_kernel   per pair: Ks^-1, Kd, T = Ed Es^-1 (4x4, general inverse)
//   imc_points_kernel  per point: residuals of both variants + histogram atomics (counts are
//                      sums of 1.0: exact, order-independent)
//   imc_cdf_kernel     per (variant, node): pmf, cumsum CDF, reflect-padded Sobel + Gaussian PDF
//   imc_back_kernel    per point: CDF lookup (loss terms) and the chain rule down to per-pair
//                      dKd, dT, dKs^-1, reduced per workgroup into fixed partial slots
//   imc_final_kernel   partials summed in fixed order -> per-pair -> per-view grads -> shared
//                      focal / K' / FoV / quaternion backward -> d enc; the loss value
// Points are float32 like the reference; the 3x3 / 4x4 algebra runs in double.
//
// sr_imc_residual_stats (ABI 1.10) reports what the loss bins, through the same kernels: views,
// pairs (+ the fundamental matrix), points (+ the three residuals in pixels), cdf, then
//   imc_frames_kernel  per (variant, node): pmf / cdf / pdf copied out of the workspace
//   imc_select_kernel  per (variant, pair): counts, fp64 mean, max and the exact median / p90 by a
//                      radix select on the fp32 bit patterns (4 digits of 8 bits, histograms in LDS)
#include <cmath>

#include "sr_common.h"

namespace {

constexpr int PTB = 256;  // points per workgroup in the per-point kernels
constexpr int NPG = 30;   // per-pair gradient slots: dKd 9 | dT 12 | dKsinv 9
constexpr int VIEW_SLOTS = 21;  // Kr 9 | E 12
constexpr int PAIR_SLOTS = 9 + 9 + 12 + 16 + 16;  // Ksinv | Kd | T (3x4) | Es^-1 (4x4) | Ed (4x4)

struct Ws {  // workspace carve-up (floats unless noted)
  float* views;   // [n_views][21]
  float* pairs;   // [n_pairs][62]
  float* hist;    // [2][n_nodes][bins]
  float* tot;     // [2][n_nodes]
  float* cdf;     // [2][n_nodes][bins]
  float* pdf;     // [2][n_nodes][bins]
  float* part;    // [n_pairs][chunks][NPG + 1]  (+1: loss partial)
};

__host__ __device__ inline int64_t ws_floats(int nv, int np, int nn, int bins, int chunks) {
  return (int64_t)nv * VIEW_SLOTS + (int64_t)np * PAIR_SLOTS + 2ll * nn * bins + 2ll * nn + 4ll * nn * bins +
         (int64_t)np * chunks * (NPG + 1);
}

__device__ inline Ws carve(float* w, int nv, int np, int nn, int bins) {
  Ws s;
  s.views = w;
  s.pairs = s.views + (int64_t)nv * VIEW_SLOTS;
  s.hist = s.pairs + (int64_t)np * PAIR_SLOTS;
  s.tot = s.hist + 2ll * nn * bins;
  s.cdf = s.tot + 2ll * nn;
  s.pdf = s.cdf + 2ll * nn * bins;
  s.part = s.pdf + 2ll * nn * bins;
  return s;
}

// ---------------------------------------------------------------- small dense algebra (double)
__device__ inline void mat3_inv(const double* a, double* o) {
  const double c00 = a[4] * a[8] - a[5] * a[7], c01 = a[5] * a[6] - a[3] * a[8], c02 = a[3] * a[7] - a[4] * a[6];
  const double det = a[0] * c00 + a[1] * c01 + a[2] * c02;
  const double id = 1.0 / det;
  o[0] = c00 * id;
  o[1] = (a[2] * a[7] - a[1] * a[8]) * id;
  o[2] = (a[1] * a[5] - a[2] * a[4]) * id;
  o[3] = c01 * id;
  o[4] = (a[0] * a[8] - a[2] * a[6]) * id;
  o[5] = (a[2] * a[3] - a[0] * a[5]) * id;
  o[6] = c02 * id;
  o[7] = (a[1] * a[6] - a[0] * a[7]) * id;
  o[8] = (a[0] * a[4] - a[1] * a[3]) * id;
}

// general 4x4 inverse, Gauss-Jordan with partial pivoting (torch.inverse on [R|t;0 0 0 1])
__device__ inline void mat4_inv(const double* a, double* o) {
  double m[4][8];
  for (int i = 0; i < 4; ++i)
    for (int j = 0; j < 4; ++j) {
      m[i][j] = a[i * 4 + j];
      m[i][4 + j] = i == j ? 1.0 : 0.0;
    }
  for (int c = 0; c < 4; ++c) {
    int p = c;
    for (int r = c + 1; r < 4; ++r)
      if (fabs(m[r][c]) > fabs(m[p][c])) p = r;
    if (p != c)
      for (int j = 0; j < 8; ++j) {
        const double t = m[c][j];
        m[c][j] = m[p][j];
        m[p][j] = t;
      }
    const double iv = 1.0 / m[c][c];
    for (int j = 0; j < 8; ++j) m[c][j] *= iv;
    for (int r = 0; r < 4; ++r)
      if (r != c) {
        const double f = m[r][c];
        for (int j = 0; j < 8; ++j) m[r][j] -= f * m[c][j];
      }
  }
  for (int i = 0; i < 4; ++i)
    for (int j = 0; j < 4; ++j) o[i * 4 + j] = m[i][4 + j];
}

// ---------------------------------------------------------------- views
__global__ void imc_views_kernel(sr_imc_loss_desc d, float* wsp) {
  const Ws w = carve(wsp, d.n_views, d.n_pairs, d.n_nodes, d.num_bins);
  __shared__ double kr[64][9];
  const int n = d.n_views;
  for (int v = threadIdx.x; v < n; v += blockDim.x) {
    const float* e = d.enc + v * 9;
    // K (pose_enc.py:116-130): fy = (H/2)/tan(fov_h/2), fx = (W/2)/tan(fov_w/2), pp = (W/2, H/2)
    const float fy = (d.H / 2.0f) / tanf(e[7] / 2.0f), fx = (d.W / 2.0f) / tanf(e[8] / 2.0f);
    const double K[9] = {fx, 0, d.W / 2.0, 0, fy, d.H / 2.0, 0, 0, 1};
    const float* kp = d.kp2k + v * 9;
    for (int i = 0; i < 3; ++i)
      for (int j = 0; j < 3; ++j) {
        double s = 0;
        for (int t = 0; t < 3; ++t) s += (double)kp[i * 3 + t] * K[t * 3 + j];
        if (v < 64) kr[v][i * 3 + j] = s;
        w.views[v * VIEW_SLOTS + i * 3 + j] = (float)s;
      }
    // E = [quat_to_mat(q) | T] (rotation.py:14-44, xyzw)
    const float i_ = e[3], j_ = e[4], k_ = e[5], r_ = e[6];
    const float s2 = 2.0f / (i_ * i_ + j_ * j_ + k_ * k_ + r_ * r_);
    const float R[9] = {1 - s2 * (j_ * j_ + k_ * k_), s2 * (i_ * j_ - k_ * r_), s2 * (i_ * k_ + j_ * r_),
                        s2 * (i_ * j_ + k_ * r_), 1 - s2 * (i_ * i_ + k_ * k_), s2 * (j_ * k_ - i_ * r_),
                        s2 * (i_ * k_ - j_ * r_), s2 * (j_ * k_ + i_ * r_), 1 - s2 * (i_ * i_ + j_ * j_)};
    float* E = w.views + v * VIEW_SLOTS + 9;
    for (int i = 0; i < 3; ++i) {
      E[i * 4 + 0] = R[i * 3 + 0];
      E[i * 4 + 1] = R[i * 3 + 1];
      E[i * 4 + 2] = R[i * 3 + 2];
      E[i * 4 + 3] = e[i];
    }
  }
  __syncthreads();
  if (d.shared_focal && threadIdx.x == 0) {  // Kr_i = mean_j Kr_j (train_imc.py:169-174)
    for (int t = 0; t < 9; ++t) {
      double s = 0;
      for (int v = 0; v < n; ++v) s += (float)kr[v][t];
      const float m = (float)(s / n);
      for (int v = 0; v < n; ++v) w.views[v * VIEW_SLOTS + t] = m;
    }
  }
}

// ---------------------------------------------------------------- pairs
// fmat (stats only, else NULL): [n_pairs][9] F = Kd^-T [t]x R Ks^-1 of T = (R | t), unit Frobenius norm
__global__ void imc_pairs_kernel(sr_imc_loss_desc d, float* wsp, float* fmat) {
  const Ws w = carve(wsp, d.n_views, d.n_pairs, d.n_nodes, d.num_bins);
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= d.n_pairs) return;
  const float* vs = w.views + d.src_idx[p] * VIEW_SLOTS;
  const float* vd = w.views + d.dst_idx[p] * VIEW_SLOTS;
  double Ks[9], Ksi[9], Es[16], Esi[16], Ed[16];
  for (int t = 0; t < 9; ++t) Ks[t] = vs[t];
  mat3_inv(Ks, Ksi);
  for (int i = 0; i < 4; ++i)
    for (int j = 0; j < 4; ++j) {
      Es[i * 4 + j] = i < 3 ? vs[9 + i * 4 + j] : (j == 3 ? 1.0 : 0.0);
      Ed[i * 4 + j] = i < 3 ? vd[9 + i * 4 + j] : (j == 3 ? 1.0 : 0.0);
    }
  mat4_inv(Es, Esi);
  float* o = w.pairs + (int64_t)p * PAIR_SLOTS;
  for (int t = 0; t < 9; ++t) {
    o[t] = (float)Ksi[t];
    o[9 + t] = vd[t];
  }
  double T[12];
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 4; ++j) {
      double s = 0;
      for (int t = 0; t < 4; ++t) s += Ed[i * 4 + t] * Esi[t * 4 + j];
      T[i * 4 + j] = s;
      o[18 + i * 4 + j] = (float)s;
    }
  for (int t = 0; t < 16; ++t) {
    o[30 + t] = (float)Esi[t];
    o[46 + t] = (float)Ed[t];
  }
  if (fmat) {
    double Kd[9], Kdi[9], E[9], A[9], F[9];
    for (int t = 0; t < 9; ++t) Kd[t] = vd[t];
    mat3_inv(Kd, Kdi);
    const double tx = T[3], ty = T[7], tz = T[11];
    for (int j = 0; j < 3; ++j) {  // [t]x R
      E[j] = ty * T[8 + j] - tz * T[4 + j];
      E[3 + j] = tz * T[j] - tx * T[8 + j];
      E[6 + j] = tx * T[4 + j] - ty * T[j];
    }
    for (int i = 0; i < 3; ++i)
      for (int j = 0; j < 3; ++j) {
        double a = 0;
        for (int t = 0; t < 3; ++t) a += Kdi[t * 3 + i] * E[t * 3 + j];  // Kd^-T E
        A[i * 3 + j] = a;
      }
    double n2 = 0;
    for (int i = 0; i < 3; ++i)
      for (int j = 0; j < 3; ++j) {
        double a = 0;
        for (int t = 0; t < 3; ++t) a += A[i * 3 + t] * Ksi[t * 3 + j];
        F[i * 3 + j] = a;
        n2 += a * a;
      }
    const double inv = 1.0 / sqrt(n2);
    for (int t = 0; t < 9; ++t) fmat[(int64_t)p * 9 + t] = (float)(F[t] * inv);
  }
}

// forward geometry of one point: returns X (3), Y (3), p (3) and both predictions
struct PointGeo {
  float X[3], Y[3], p[3], pred[2][2], r[2];
};

__device__ inline PointGeo point_geo(const sr_imc_loss_desc& d, const float* pr, int p, int k) {
  PointGeo g;
  const int64_t e = (int64_t)p * d.n_points + k;
  const float u = d.src_coords[2 * e], v = d.src_coords[2 * e + 1];
  const float ds = d.src_depth[e], dd = d.dst_depth[e];
  const float* Ksi = pr;
  const float* Kd = pr + 9;
  const float* T = pr + 18;
  for (int i = 0; i < 3; ++i) g.X[i] = (Ksi[i * 3] * u + Ksi[i * 3 + 1] * v + Ksi[i * 3 + 2]) * ds;
  for (int i = 0; i < 3; ++i) g.Y[i] = T[i * 4] * g.X[0] + T[i * 4 + 1] * g.X[1] + T[i * 4 + 2] * g.X[2] + T[i * 4 + 3];
  for (int i = 0; i < 3; ++i) g.p[i] = Kd[i * 3] * g.Y[0] + Kd[i * 3 + 1] * g.Y[1] + Kd[i * 3 + 2] * g.Y[2];
  const float ox = d.dst_coords[2 * e], oy = d.dst_coords[2 * e + 1];
  const float den[2] = {g.p[2] + 1e-6f, dd + 1e-6f};  // from_homogeneous / fixed-depth variant
  for (int vv = 0; vv < 2; ++vv) {
    g.pred[vv][0] = g.p[0] / den[vv];
    g.pred[vv][1] = g.p[1] / den[vv];
    const float a = g.pred[vv][0] - ox, b = g.pred[vv][1] - oy;
    g.r[vv] = sqrtf(a * a + b * b);
  }
  return g;
}

// a test on the bits: the library builds with -fno-honor-nans
__device__ inline bool finite_bits(uint32_t b) { return (b & 0x7f800000u) != 0x7f800000u; }
constexpr uint32_t QNAN_BITS = 0x7fc00000u;

struct StatsOut {  // sr_imc_residual_stats only
  const float* fmat;  // [n_pairs][9]
  float* resid;       // [3][n_pairs][n_points] pixels: exact, fixed depth, Sampson
  float* behind;      // [n_pairs][n_points] 1 where the exact residual is finite and p_z <= 0, else 0
};

// ---------------------------------------------------------------- residuals + histograms
template <bool kStats>
__global__ __launch_bounds__(PTB) void imc_points_kernel(sr_imc_loss_desc d, float* wsp, StatsOut so) {
  const Ws w = carve(wsp, d.n_views, d.n_pairs, d.n_nodes, d.num_bins);
  const int p = blockIdx.y, k = blockIdx.x * PTB + threadIdx.x;
  if (k >= d.n_points) return;
  const PointGeo g = point_geo(d, w.pairs + (int64_t)p * PAIR_SLOTS, p, k);
  if constexpr (kStats) {
    const int64_t e = (int64_t)p * d.n_points + k, pk = (int64_t)d.n_pairs * d.n_points;
    so.resid[e] = g.r[0];
    so.resid[pk + e] = g.r[1];
    so.behind[e] = finite_bits(__float_as_uint(g.r[0])) && g.p[2] <= 0.f ? 1.f : 0.f;
    float r2 = __uint_as_float(QNAN_BITS);  // src == dst: no epipolar geometry (a rule on the indices)
    if (d.src_idx[p] != d.dst_idx[p]) {
      // Sampson distance of x = (u, v, 1), x' = (u', v', 1) under the pair's F; sums in double
      const float* F = so.fmat + (int64_t)p * 9;
      const double u = d.src_coords[2 * e], v = d.src_coords[2 * e + 1];
      const double ox = d.dst_coords[2 * e], oy = d.dst_coords[2 * e + 1];
      double Fx[3], Ft[2];
      for (int i = 0; i < 3; ++i) Fx[i] = (double)F[i * 3] * u + (double)F[i * 3 + 1] * v + (double)F[i * 3 + 2];
      for (int j = 0; j < 2; ++j) Ft[j] = (double)F[j] * ox + (double)F[3 + j] * oy + (double)F[6 + j];
      const double num = ox * Fx[0] + oy * Fx[1] + Fx[2];
      r2 = (float)(fabs(num) / sqrt(Fx[0] * Fx[0] + Fx[1] * Fx[1] + Ft[0] * Ft[0] + Ft[1] * Ft[1]));
    }
    so.resid[2 * pk + e] = r2;
  }
  const float bw = (d.max_val - d.min_val) / d.num_bins;
  const int ns = d.node_src[p], nd = d.node_dst[p];
  for (int vv = 0; vv < 2; ++vv) {
    const float rl = log1pf(g.r[vv]);
    const long b = (long)((rl - d.min_val) / bw);  // .long(): truncation (cdf_loss.py:137)
    float* h = w.hist + (int64_t)vv * d.n_nodes * d.num_bins;
    if (b >= 0 && b < d.num_bins) {  // weights are the all-ones validity masks
      atomicAdd(h + (int64_t)ns * d.num_bins + b, 1.0f);
      atomicAdd(h + (int64_t)nd * d.num_bins + b, 1.0f);
    }
    atomicAdd(w.tot + vv * d.n_nodes + ns, 1.0f);
    atomicAdd(w.tot + vv * d.n_nodes + nd, 1.0f);
  }
}

// ---------------------------------------------------------------- per-node CDF / PDF
__global__ void imc_cdf_kernel(sr_imc_loss_desc d, float* wsp) {
  const Ws w = carve(wsp, d.n_views, d.n_pairs, d.n_nodes, d.num_bins);
  const int vv = blockIdx.y, node = blockIdx.x, nb = d.num_bins;
  const int64_t o = ((int64_t)vv * d.n_nodes + node) * nb;
  float* cdf = w.cdf + o;
  float* pdf = w.pdf + o;
  __shared__ float raw[1024];
  if (threadIdx.x == 0) {  // pmf = hist / (total + 1e-10); cumsum in bin order (cdf_loss.py:177-178)
    const float t = w.tot[vv * d.n_nodes + node] + 1e-10f;
    float s = 0.f;
    for (int i = 0; i < nb; ++i) {
      s += w.hist[o + i] / t;
      cdf[i] = s;
    }
  }
  __syncthreads();
  const float bw = (d.max_val - d.min_val) / nb;
  auto refl = [nb](int i) { return i < 0 ? -i : (i >= nb ? 2 * (nb - 1) - i : i); };
  for (int i = threadIdx.x; i < nb; i += blockDim.x)  // Sobel [-1, 0, 1] / (2 bw), reflect padding
    raw[i] = (-cdf[refl(i - 1)] + cdf[refl(i + 1)]) / (2.0f * bw);
  __syncthreads();
  const int R = d.smooth_radius;
  for (int i = threadIdx.x; i < nb; i += blockDim.x) {
    float s = 0.f;
    for (int t = -R; t <= R; ++t) s += d.smooth_w[t + R] * raw[refl(i + t)];
    pdf[i] = s;
  }
}

// ---------------------------------------------------------------- lookup + chain rule per point
__global__ __launch_bounds__(PTB) void imc_back_kernel(sr_imc_loss_desc d, float* wsp, int chunks) {
  const Ws w = carve(wsp, d.n_views, d.n_pairs, d.n_nodes, d.num_bins);
  __shared__ float red[PTB / 64][NPG + 1];
  const int p = blockIdx.y, k = blockIdx.x * PTB + threadIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  float acc[NPG + 1];
#pragma unroll
  for (int t = 0; t <= NPG; ++t) acc[t] = 0.f;
  if (k < d.n_points) {
    const float* pr = w.pairs + (int64_t)p * PAIR_SLOTS;
    const PointGeo g = point_geo(d, pr, p, k);
    const int64_t e = (int64_t)p * d.n_points + k;
    const float ox = d.dst_coords[2 * e], oy = d.dst_coords[2 * e + 1];
    const float u = d.src_coords[2 * e], v = d.src_coords[2 * e + 1];
    const float ds = d.src_depth[e], dd = d.dst_depth[e];
    const float bw = (d.max_val - d.min_val) / d.num_bins;
    const int ns = d.node_src[p], nd = d.node_dst[p];
    const float inv4 = d.grad_scale / (4.0f * (float)d.n_pairs * (float)d.n_points);
    float gp[3] = {0.f, 0.f, 0.f};
    for (int vv = 0; vv < 2; ++vv) {
      const float rl = log1pf(g.r[vv]);
      const long b = (long)((rl - d.min_val) / bw + 0.5f);  // lookup bin (cdf_loss.py:207-210)
      const bool ok = b >= 0 && b < d.num_bins;
      const int64_t base = (int64_t)vv * d.n_nodes * d.num_bins;
      const float cs = ok ? w.cdf[base + (int64_t)ns * d.num_bins + b] : 2.0f;
      const float cd = ok ? w.cdf[base + (int64_t)nd * d.num_bins + b] : 2.0f;
      acc[NPG] += cs + cd;  // loss = sum over both variants / (4 P K)
      const float grl = ok ? (w.pdf[base + (int64_t)ns * d.num_bins + b] + w.pdf[base + (int64_t)nd * d.num_bins + b]) *
                                 inv4
                           : 0.f;
      const float gr = grl / (1.f + g.r[vv]);
      if (g.r[vv] > 0.f && gr != 0.f) {
        const float gx = gr * (g.pred[vv][0] - ox) / g.r[vv], gy = gr * (g.pred[vv][1] - oy) / g.r[vv];
        const float den = vv == 0 ? g.p[2] + 1e-6f : dd + 1e-6f;
        gp[0] += gx / den;
        gp[1] += gy / den;
        if (vv == 0) gp[2] -= (gx * g.p[0] + gy * g.p[1]) / (den * den);
      }
    }
    const float* Ksi = pr;
    const float* Kd = pr + 9;
    const float* T = pr + 18;
    float gY[3], gX[3];
    for (int i = 0; i < 3; ++i)
      for (int j = 0; j < 3; ++j) acc[i * 3 + j] += gp[i] * g.Y[j];  // dKd
    for (int j = 0; j < 3; ++j) gY[j] = Kd[j] * gp[0] + Kd[3 + j] * gp[1] + Kd[6 + j] * gp[2];
    for (int i = 0; i < 3; ++i) {  // dT
      for (int j = 0; j < 3; ++j) acc[9 + i * 4 + j] += gY[i] * g.X[j];
      acc[9 + i * 4 + 3] += gY[i];
    }
    for (int j = 0; j < 3; ++j) gX[j] = T[j] * gY[0] + T[4 + j] * gY[1] + T[8 + j] * gY[2];
    const float h[3] = {u * ds, v * ds, ds};
    for (int i = 0; i < 3; ++i)
      for (int j = 0; j < 3; ++j) acc[21 + i * 3 + j] += gX[i] * h[j];  // dKs^-1
    (void)Ksi;
  }
#pragma unroll
  for (int t = 0; t <= NPG; ++t) {
    const float s = sr::wave_sum(acc[t]);
    if (lane == 0) red[wave][t] = s;
  }
  __syncthreads();
  if (threadIdx.x <= NPG) {
    float s = 0.f;
    for (int q = 0; q < PTB / 64; ++q) s += red[q][threadIdx.x];
    w.part[((int64_t)p * chunks + blockIdx.x) * (NPG + 1) + threadIdx.x] = s;
  }
}

// ---------------------------------------------------------------- per-pair -> per-view -> d enc
__global__ void imc_final_kernel(sr_imc_loss_desc d, float* wsp, int chunks) {
  const Ws w = carve(wsp, d.n_views, d.n_pairs, d.n_nodes, d.num_bins);
  if (threadIdx.x != 0) return;
  const int nv = d.n_views;
  double gKr[64][9], gE[64][12];
  for (int v = 0; v < nv; ++v) {
    for (int t = 0; t < 9; ++t) gKr[v][t] = 0;
    for (int t = 0; t < 12; ++t) gE[v][t] = 0;
  }
  double loss = 0;
  for (int p = 0; p < d.n_pairs; ++p) {
    double g[NPG + 1];
    for (int t = 0; t <= NPG; ++t) g[t] = 0;
    for (int c = 0; c < chunks; ++c)
      for (int t = 0; t <= NPG; ++t) g[t] += w.part[((int64_t)p * chunks + c) * (NPG + 1) + t];
    loss += g[NPG];
    const float* pr = w.pairs + (int64_t)p * PAIR_SLOTS;
    const int s = d.src_idx[p], dv = d.dst_idx[p];
    // dKs = -Ks^-T dKsinv Ks^-T
    double Ksi[9], tmp[9];
    for (int t = 0; t < 9; ++t) Ksi[t] = pr[t];
    for (int i = 0; i < 3; ++i)
      for (int j = 0; j < 3; ++j) {
        double a = 0;
        for (int t = 0; t < 3; ++t) a += Ksi[t * 3 + i] * g[21 + t * 3 + j];  // Ksi^T dKsinv
        tmp[i * 3 + j] = a;
      }
    for (int i = 0; i < 3; ++i)
      for (int j = 0; j < 3; ++j) {
        double a = 0;
        for (int t = 0; t < 3; ++t) a += tmp[i * 3 + t] * Ksi[j * 3 + t];  // (.) Ksi^T
        gKr[s][i * 3 + j] -= a;
      }
    for (int t = 0; t < 9; ++t) gKr[dv][t] += g[t];
    // T = Ed Es^-1:  dEd = dT Es^-T;  dEs^-1 = Ed^T dT;  dEs = -Es^-T dEs^-1 Es^-T  (4x4, dT row 3 = 0)
    double dT[16], Esi[16], Ed[16], dEsi[16], t2[16];
    for (int i = 0; i < 4; ++i)
      for (int j = 0; j < 4; ++j) dT[i * 4 + j] = i < 3 ? g[9 + i * 4 + j] : 0.0;
    for (int t = 0; t < 16; ++t) {
      Esi[t] = pr[30 + t];
      Ed[t] = pr[46 + t];
    }
    for (int i = 0; i < 3; ++i)
      for (int j = 0; j < 4; ++j) {
        double a = 0;
        for (int t = 0; t < 4; ++t) a += dT[i * 4 + t] * Esi[j * 4 + t];
        gE[dv][i * 4 + j] += a;
      }
    for (int i = 0; i < 4; ++i)
      for (int j = 0; j < 4; ++j) {
        double a = 0;
        for (int t = 0; t < 4; ++t) a += Ed[t * 4 + i] * dT[t * 4 + j];
        dEsi[i * 4 + j] = a;
      }
    for (int i = 0; i < 4; ++i)
      for (int j = 0; j < 4; ++j) {
        double a = 0;
        for (int t = 0; t < 4; ++t) a += Esi[t * 4 + i] * dEsi[t * 4 + j];
        t2[i * 4 + j] = a;
      }
    for (int i = 0; i < 3; ++i)
      for (int j = 0; j < 4; ++j) {
        double a = 0;
        for (int t = 0; t < 4; ++t) a += t2[i * 4 + t] * Esi[j * 4 + t];
        gE[s][i * 4 + j] -= a;
      }
  }
  if (d.loss) d.loss[0] = (float)(loss / (4.0 * (double)d.n_pairs * (double)d.n_points));
  if (d.shared_focal) {  // every Kr_i is the mean of all: dKr'_j = (1/N) sum_i dKr_i
    for (int t = 0; t < 9; ++t) {
      double s = 0;
      for (int v = 0; v < nv; ++v) s += gKr[v][t];
      for (int v = 0; v < nv; ++v) gKr[v][t] = s / nv;
    }
  }
  for (int v = 0; v < nv; ++v) {
    const float* e = d.enc + v * 9;
    const float* kp = d.kp2k + v * 9;
    double gK[9];
    for (int i = 0; i < 3; ++i)
      for (int j = 0; j < 3; ++j) {
        double a = 0;
        for (int t = 0; t < 3; ++t) a += (double)kp[t * 3 + i] * gKr[v][t * 3 + j];  // K'^T dKr
        gK[i * 3 + j] = a;
      }
    float* o = d.d_enc + v * 9;
    // f = (S/2) / tan(fov/2):  df/dfov = -(S/4) / sin^2(fov/2)
    const double sh = sin(e[7] / 2.0), sw = sin(e[8] / 2.0);
    o[7] = (float)(gK[4] * (-(d.H / 4.0) / (sh * sh)));
    o[8] = (float)(gK[0] * (-(d.W / 4.0) / (sw * sw)));
    for (int i = 0; i < 3; ++i) o[i] = (float)gE[v][i * 4 + 3];
    // quat_to_mat backward: R = I + s A(q), s = 2 / |q|^2
    const double qi = e[3], qj = e[4], qk = e[5], qr = e[6];
    const double nq = qi * qi + qj * qj + qk * qk + qr * qr, s2 = 2.0 / nq;
    double gR[9];
    for (int i = 0; i < 3; ++i)
      for (int j = 0; j < 3; ++j) gR[i * 3 + j] = gE[v][i * 4 + j];
    const double A[9] = {-(qj * qj + qk * qk), qi * qj - qk * qr, qi * qk + qj * qr, qi * qj + qk * qr,
                         -(qi * qi + qk * qk), qj * qk - qi * qr, qi * qk - qj * qr, qj * qk + qi * qr,
                         -(qi * qi + qj * qj)};
    const double dAi[9] = {0, qj, qk, qj, -2 * qi, -qr, qk, qr, -2 * qi};
    const double dAj[9] = {-2 * qj, qi, qr, qi, 0, qk, -qr, qk, -2 * qj};
    const double dAk[9] = {-2 * qk, -qr, qi, qr, -2 * qk, qj, qi, qj, 0};
    const double dAr[9] = {0, -qk, qj, qk, 0, -qi, -qj, qi, 0};
    double gA = 0, gi = 0, gj = 0, gk = 0, gr = 0;
    for (int t = 0; t < 9; ++t) {
      gA += gR[t] * A[t];
      gi += gR[t] * dAi[t];
      gj += gR[t] * dAj[t];
      gk += gR[t] * dAk[t];
      gr += gR[t] * dAr[t];
    }
    const double ds_coef = -s2 * 2.0 / nq * gA;  // d s / d q = -s * 2 q / |q|^2
    o[3] = (float)(s2 * gi + ds_coef * qi);
    o[4] = (float)(s2 * gj + ds_coef * qj);
    o[5] = (float)(s2 * gk + ds_coef * qk);
    o[6] = (float)(s2 * gr + ds_coef * qr);
  }
}

// ---------------------------------------------------------------- stats: per-frame arrays
__global__ void imc_frames_kernel(sr_imc_loss_desc d, float* wsp, float* pmf, float* cdf, float* pdf) {
  const Ws w = carve(wsp, d.n_views, d.n_pairs, d.n_nodes, d.num_bins);
  const int vv = blockIdx.y, node = blockIdx.x, nb = d.num_bins;
  const int64_t o = ((int64_t)vv * d.n_nodes + node) * nb;
  const float t = w.tot[vv * d.n_nodes + node] + 1e-10f;  // as imc_cdf_kernel
  for (int i = threadIdx.x; i < nb; i += blockDim.x) {
    if (pmf) pmf[o + i] = w.hist[o + i] / t;
    if (cdf) cdf[o + i] = w.cdf[o + i];
    if (pdf) pdf[o + i] = w.pdf[o + i];
  }
}

// ---------------------------------------------------------------- stats: per-pair selection
constexpr int SEL_T = 1024;       // threads of the one workgroup per (variant, pair)
constexpr int SEL_CACHE = 12288;  // residuals of a pair kept in LDS (48 KiB); more are re-read from global memory

__device__ inline double wave_sum_f64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// Non-negative floats order as their bit patterns, so rank k of the finite values is found digit by
// digit: a 256-bin histogram of the digit among the values that share the digits found so far, a
// scan for the bin that holds rank k, four times.  Both ranks (median, p90) ride the same passes,
// each with its own prefix and histogram; the first pass also takes the counts, the max and the sum.
__global__ __launch_bounds__(SEL_T) void imc_select_kernel(const float* resid, const float* behind, int n_pairs,
                                                           int n_points, const float* thresh, int n_thresh,
                                                           uint32_t* counts, float* stats) {
  __shared__ uint32_t cache[SEL_CACHE];
  __shared__ uint32_t hist[2][256];
  __shared__ double wsum[SEL_T / 64];
  __shared__ uint32_t cnt[2 + 8];
  __shared__ uint32_t smax;
  __shared__ uint32_t prefix[2];
  __shared__ uint64_t rank[2];
  const int p = blockIdx.x, v = blockIdx.y, tid = threadIdx.x;
  const uint32_t* x = reinterpret_cast<const uint32_t*>(resid) + ((int64_t)v * n_pairs + p) * n_points;
  const float* bh = behind + (int64_t)p * n_points;
  const bool cached = n_points <= SEL_CACHE;
  if (tid < 512) hist[tid >> 8][tid & 255] = 0;
  if (tid < 10) cnt[tid] = 0;
  if (tid == 0) smax = 0;
  __syncthreads();
  float th[8];
#pragma unroll
  for (int t = 0; t < 8; ++t) th[t] = t < n_thresh ? thresh[t] : 0.f;
  uint32_t c_fin = 0, c_beh = 0, c_th[8] = {0, 0, 0, 0, 0, 0, 0, 0}, mx = 0;
  double s = 0;
  for (int k = tid; k < n_points; k += SEL_T) {  // a fixed assignment of points to threads: a fixed sum
    const uint32_t b = x[k];
    if (cached) cache[k] = b;
    if (finite_bits(b)) {
      const float f = __uint_as_float(b);
      ++c_fin;
      s += (double)f;
      mx = b > mx ? b : mx;
#pragma unroll
      for (int t = 0; t < 8; ++t) c_th[t] += (t < n_thresh && f < th[t]) ? 1u : 0u;
      atomicAdd(&hist[0][b >> 24], 1u);
    }
    c_beh += bh[k] != 0.f ? 1u : 0u;
  }
  if (c_fin) atomicAdd(&cnt[0], c_fin);
  if (c_beh) atomicAdd(&cnt[1], c_beh);
#pragma unroll
  for (int t = 0; t < 8; ++t)
    if (c_th[t]) atomicAdd(&cnt[2 + t], c_th[t]);
  if (mx) atomicMax(&smax, mx);
  s = wave_sum_f64(s);
  if ((tid & 63) == 0) wsum[tid >> 6] = s;
  __syncthreads();
  const uint32_t n = cnt[0];
  const int64_t slot = (int64_t)v * n_pairs + p;
  if (tid == 0 && counts) {
    uint32_t* c = counts + slot * (2 + n_thresh);
    c[0] = n;
    c[1] = cnt[1];
    for (int t = 0; t < n_thresh; ++t) c[2 + t] = cnt[2 + t];
  }
  if (!stats) return;
  float* out = stats + slot * 4;
  if (n == 0) {  // uniform: n comes from LDS after the barrier
    if (tid < 4) out[tid] = __uint_as_float(QNAN_BITS);
    return;
  }
  if (tid == 0) {
    double tot = 0;
    for (int q = 0; q < SEL_T / 64; ++q) tot += wsum[q];
    out[0] = (float)(tot / (double)n);
    out[3] = __uint_as_float(smax);
  }
  if (tid < 2) {
    prefix[tid] = 0;
    rank[tid] = tid == 0 ? ((uint64_t)n - 1) / 2 : (9ull * n + 9) / 10 - 1;  // lower median; p90
  }
  __syncthreads();
  for (int dgt = 0; dgt < 4; ++dgt) {
    if (tid < 2) {  // the bin of this rank among the values that share its prefix
      const uint32_t* h = hist[dgt == 0 ? 0 : tid];
      uint64_t r = rank[tid];
      int b = 0;
      for (; b < 255; ++b) {
        const uint32_t c = h[b];
        if (r < c) break;
        r -= c;
      }
      rank[tid] = r;
      prefix[tid] = (prefix[tid] << 8) | (uint32_t)b;
    }
    __syncthreads();
    if (dgt == 3) break;
    if (tid < 512) hist[tid >> 8][tid & 255] = 0;
    __syncthreads();
    const int hi = 24 - 8 * dgt, lo = hi - 8;  // digits found so far: bits >= hi; this pass: bits [lo, hi)
    const uint32_t p0 = prefix[0], p1 = prefix[1];
    for (int k = tid; k < n_points; k += SEL_T) {
      const uint32_t b = cached ? cache[k] : x[k];
      if (!finite_bits(b)) continue;
      const uint32_t top = b >> hi, d8 = (b >> lo) & 255u;
      if (top == p0) atomicAdd(&hist[0][d8], 1u);
      if (top == p1) atomicAdd(&hist[1][d8], 1u);
    }
    __syncthreads();
  }
  if (tid < 2) out[1 + tid] = __uint_as_float(prefix[tid]);
}

}  // namespace

extern "C" int64_t sr_imc_loss_workspace(int n_views, int n_pairs, int n_points, int n_nodes, int num_bins) {
  const int chunks = (n_points + PTB - 1) / PTB;
  return ws_floats(n_views, n_pairs, n_nodes, num_bins, chunks);
}

extern "C" int sr_imc_loss(sr_stream_t stream, const sr_imc_loss_desc* desc) {
  SR_CHECK(desc, SR_EINVAL, "sr_imc_loss: null desc");
  const sr_imc_loss_desc& d = *desc;
  SR_CHECK(d.enc && d.kp2k && d.src_idx && d.dst_idx && d.src_coords && d.dst_coords && d.src_depth && d.dst_depth &&
               d.node_src && d.node_dst && d.d_enc && d.workspace && d.smooth_w,
           SR_EINVAL, "sr_imc_loss: null pointer");
  SR_CHECK(d.n_views > 0 && d.n_views <= 64 && d.n_pairs > 0 && d.n_points > 0 && d.n_nodes > 0 &&
               d.num_bins > 2 && d.num_bins <= 1024 && d.smooth_radius >= 0 && 2 * d.smooth_radius + 1 <= d.num_bins &&
               d.max_val > d.min_val && d.H > 0 && d.W > 0,
           SR_EUNSUPPORTED, "sr_imc_loss: bad sizes (views <= 64, bins <= 1024)");
  hipStream_t s = (hipStream_t)stream;
  const int chunks = (d.n_points + PTB - 1) / PTB;
  float* w = d.workspace;
  const int64_t nn = d.n_nodes, nb = d.num_bins;
  // histograms / totals start at zero (one memset of their contiguous range)
  const int64_t hist_off = (int64_t)d.n_views * VIEW_SLOTS + (int64_t)d.n_pairs * PAIR_SLOTS;
  SR_CHECK(hipMemsetAsync(w + hist_off, 0, (2 * nn * nb + 2 * nn) * sizeof(float), s) == hipSuccess, SR_ELAUNCH,
           "sr_imc_loss: memset");
  hipLaunchKernelGGL(imc_views_kernel, dim3(1), dim3(64), 0, s, d, w);
  hipLaunchKernelGGL(imc_pairs_kernel, dim3((d.n_pairs + 63) / 64), dim3(64), 0, s, d, w, (float*)nullptr);
  hipLaunchKernelGGL(imc_points_kernel<false>, dim3(chunks, d.n_pairs), dim3(PTB), 0, s, d, w, StatsOut{});
  hipLaunchKernelGGL(imc_cdf_kernel, dim3(d.n_nodes, 2), dim3(256), 0, s, d, w);
  hipLaunchKernelGGL(imc_back_kernel, dim3(chunks, d.n_pairs), dim3(PTB), 0, s, d, w, chunks);
  hipLaunchKernelGGL(imc_final_kernel, dim3(1), dim3(64), 0, s, d, w, chunks);
  return sr::check_launch("sr_imc_loss");
}

extern "C" int64_t sr_imc_stats_workspace(int n_views, int n_pairs, int n_points, int n_nodes, int num_bins) {
  if (n_views <= 0 || n_pairs <= 0 || n_points <= 0 || n_nodes <= 0 || num_bins <= 0) return 0;
  // the loss's carve-up without partial slots, then F, three residual planes and the behind flags
  return ws_floats(n_views, n_pairs, n_nodes, num_bins, 0) + 9ll * n_pairs + 4ll * n_pairs * n_points;
}

extern "C" int sr_imc_residual_stats(sr_stream_t stream, const sr_imc_loss_desc* desc, const sr_imc_stats_desc* out) {
  SR_CHECK(desc && out, SR_EINVAL, "sr_imc_residual_stats: null desc");
  sr_imc_loss_desc d = *desc;
  const sr_imc_stats_desc& o = *out;
  SR_CHECK(d.enc && d.kp2k && d.src_idx && d.dst_idx && d.src_coords && d.dst_coords && d.src_depth && d.dst_depth &&
               d.node_src && d.node_dst && d.smooth_w,
           SR_EINVAL, "sr_imc_residual_stats: null pointer");
  SR_CHECK(d.n_views > 0 && d.n_views <= 64 && d.n_pairs > 0 && d.n_points > 0 && d.n_nodes > 0 &&
               d.num_bins > 2 && d.num_bins <= 1024 && d.smooth_radius >= 0 && 2 * d.smooth_radius + 1 <= d.num_bins &&
               d.max_val > d.min_val && d.H > 0 && d.W > 0,
           SR_EINVAL, "sr_imc_residual_stats: bad sizes (views <= 64, bins <= 1024)");
  SR_CHECK(o.n_thresh >= 0 && o.n_thresh <= 8, SR_EINVAL, "sr_imc_residual_stats: n_thresh outside [0, 8]");
  SR_CHECK(o.n_thresh == 0 || (o.thresh && o.pair_counts), SR_EINVAL,
           "sr_imc_residual_stats: thresholds need thresh and pair_counts");
  const bool frames = o.frame_pmf || o.frame_cdf || o.frame_pdf, select = o.pair_counts || o.pair_stats;
  SR_CHECK(frames || select || o.residuals, SR_EINVAL, "sr_imc_residual_stats: every output is NULL");
  const int64_t base = ws_floats(d.n_views, d.n_pairs, d.n_nodes, d.num_bins, 0);
  const int64_t pk = (int64_t)d.n_pairs * d.n_points;
  SR_CHECK(o.workspace && o.workspace_floats >= base + 9ll * d.n_pairs + 4 * pk, SR_EINVAL,
           "sr_imc_residual_stats: workspace missing or smaller than sr_imc_stats_workspace");
  SR_CHECK(d.n_pairs <= 65535, SR_EINVAL, "sr_imc_residual_stats: more than 65535 pairs");
  hipStream_t s = (hipStream_t)stream;
  const int chunks = (d.n_points + PTB - 1) / PTB;
  float* w = o.workspace;
  d.loss = nullptr, d.d_enc = nullptr, d.workspace = w, d.grad_scale = 0.f;  // ignored fields: nothing reads them
  float* fmat = w + base;
  float* resid = o.residuals ? o.residuals : fmat + 9ll * d.n_pairs;
  float* behind = fmat + 9ll * d.n_pairs + 3 * pk;
  const int64_t nn = d.n_nodes, nb = d.num_bins;
  const int64_t hist_off = (int64_t)d.n_views * VIEW_SLOTS + (int64_t)d.n_pairs * PAIR_SLOTS;
  SR_CHECK(hipMemsetAsync(w + hist_off, 0, (2 * nn * nb + 2 * nn) * sizeof(float), s) == hipSuccess, SR_ELAUNCH,
           "sr_imc_residual_stats: memset");
  hipLaunchKernelGGL(imc_views_kernel, dim3(1), dim3(64), 0, s, d, w);
  hipLaunchKernelGGL(imc_pairs_kernel, dim3((d.n_pairs + 63) / 64), dim3(64), 0, s, d, w, fmat);
  hipLaunchKernelGGL(imc_points_kernel<true>, dim3(chunks, d.n_pairs), dim3(PTB), 0, s, d, w,
                     StatsOut{fmat, resid, behind});
  if (frames) {
    hipLaunchKernelGGL(imc_cdf_kernel, dim3(d.n_nodes, 2), dim3(256), 0, s, d, w);
    hipLaunchKernelGGL(imc_frames_kernel, dim3(d.n_nodes, 2), dim3(256), 0, s, d, w, o.frame_pmf, o.frame_cdf,
                       o.frame_pdf);
  }
  if (select)
    hipLaunchKernelGGL(imc_select_kernel, dim3(d.n_pairs, 3), dim3(SEL_T), 0, s, resid, behind, d.n_pairs, d.n_points,
                       o.thresh, o.n_thresh, o.pair_counts, o.pair_stats);
  return sr::check_launch("sr_imc_residual_stats");
}
