// Scoring a predicted point cloud against a ground-truth one on gfx950: the nearest-neighbour distance
// of every query point to a target set, by brute force, with the distance histogram and the moments the
// reconstruction metrics (accuracy, completeness, Chamfer distance, precision / recall / F-score at a
// threshold) are read off on the host.  One call scores one direction; the metrics are what the
// reference hands to its `eval` package (train/train_imc.py:301-317), which is absent from its tree.
//
// Contract (DESIGN.md "Scoring point clouds"; points are packed [n][3] fp32):
//   transform   p' = fl32(s (R p) + t): every product and sum in fp64, left to right, none contracted,
//               from the fp32 point and the fp64 [13] = scale, R row-major, t that sr_pose_align leaves in
//               out[0..12]; rounded to fp32 once.  sr::load_point (sr_eval.h) serves queries and targets.
//   distance    d(q) = sqrt(min_t d2(q, t)), d2 = dx dx + dy dy + dz dz in fp32 from the direct
//               differences dx = q.x - t.x, ... (never |q|^2 + |t|^2 - 2 q.t, which cancels for a cloud far
//               from the origin); sqrt correctly rounded
//   non-finite  a target with a NaN or Inf component before or after its transform (a test on the bits:
//               the build compiles with -fno-honor-nans) is staged as (+Inf, +Inf, +Inf): its d2 is +Inf
//               for every query and never wins the strict comparison.  A query that is non-finite, whose
//               minimum d2 overflows or that has no finite target gets dist = NaN, index = -1, and counts
//               in hist[n_bins + 1] and stats[4].
//   index       the lowest target index attaining the fp32 minimum of d2: every lane walks its slice in
//               ascending order and replaces on d2 < best only, and the slices are merged in ascending
//               order on the same strict comparison.  Nothing depends on execution order: two runs and
//               any target_chunk give the same bits.
//   histogram   slot k < n_bins counts k <= fl32(d / bin_len) < k + 1, slot n_bins the larger distances,
//               slot n_bins + 1 the non-finite queries; integer atomics only
//   stats       n_finite, sum d, sum d^2, max d, n_nonfinite, 0: fp64 from the fp32 d; a lane's queries in
//               ascending order, sr::block_reduce's fixed LDS tree per workgroup, one partial per workgroup in the
//               workspace, then one workgroup sums the partials (each lane a contiguous ascending run, then the
//               same tree).  No floating-point atomics.
//
//   cloud_hist_zero_kernel   clears hist
//   cloud_prep_kernel        targets -> float4 (x, y, z, 0) in the workspace, transformed, non-finite ones
//                            replaced by +Inf
//   cloud_sweep_kernel       grid (query tiles x target slices); a workgroup keeps QPL queries per lane
//                            in registers and walks its slice in tiles of TT targets staged in LDS; every
//                            lane reads the same float4 at the same time (a broadcast ds_read_b128), one
//                            fetch per QPL distance evaluations.  Writes (d2, index) per (slice, query).
//   cloud_finish_kernel      per query tile: merges the slices, writes dist / index, LDS histogram,
//                            workgroup partial of the stats
//   cloud_stats_kernel       one workgroup: sums the partials
#include "sr_common.h"
#include "sr_eval.h"

namespace {

constexpr int CE_T = 256;             // threads of every workgroup here
constexpr int QPL = 4;                // queries per lane
constexpr int QTILE = CE_T * QPL;     // queries per workgroup
constexpr int TT = 1024;              // targets per LDS tile
constexpr int MAX_BINS = 1024;
constexpr int64_t MAX_POINTS = 2147483647LL;
constexpr int MAX_SLICES = 65535;     // grid.y
constexpr int AUTO_BLOCKS = 1024;     // workgroups the automatic slice count aims for: 4 per CU
constexpr int AUTO_MIN_CHUNK = 2048;  // fewest targets of an automatic slice

using sr::pos_inf;

struct Plan {
  int64_t chunk;    // targets per slice, a multiple of 64
  int slices;       // ceil(n_target / chunk), 1 .. MAX_SLICES
  int64_t n_tiles;  // query tiles
  int64_t off_part, off_stat, bytes;  // workspace: float4 targets | (d2, index) partials | stats partials
};

// Automatic slice count: one slice once the query tiles alone give AUTO_BLOCKS workgroups; otherwise
// enough slices to reach AUTO_BLOCKS, each of at least AUTO_MIN_CHUNK targets.
bool make_plan(int64_t n_query, int64_t n_target, int target_chunk, Plan& p) {
  if (n_query < 1 || n_query > MAX_POINTS || n_target < 1 || n_target > MAX_POINTS) return false;
  if (target_chunk < 0 || target_chunk % 64 != 0) return false;
  p.n_tiles = (n_query + QTILE - 1) / QTILE;
  const int64_t max_auto = (n_target + AUTO_MIN_CHUNK - 1) / AUTO_MIN_CHUNK;
  int64_t chunk = target_chunk, part_pairs;
  if (chunk == 0) {
    int64_t want = (AUTO_BLOCKS + p.n_tiles - 1) / p.n_tiles;
    if (want > max_auto) want = max_auto;
    chunk = ((n_target + want - 1) / want + 63) / 64 * 64;
  }
  const int64_t slices = (n_target + chunk - 1) / chunk;
  if (slices > MAX_SLICES) return false;
  p.chunk = chunk;
  p.slices = (int)slices;
  if (target_chunk == 0) {
    // a bound of n_query * slices that does not shrink when n_query or n_target grows:
    // slices <= AUTO_BLOCKS / n_tiles + 1 and n_query / n_tiles <= QTILE; slices <= max_auto
    const int64_t a = (int64_t)AUTO_BLOCKS * QTILE, b = n_query > a / max_auto ? a : n_query * max_auto;
    part_pairs = n_query + (a < b ? a : b);
  } else {
    part_pairs = n_query * slices;
  }
  p.off_part = 16 * n_target;
  p.off_stat = p.off_part + 8 * part_pairs;
  p.bytes = p.off_stat + 5 * 8 * p.n_tiles;
  return true;
}

struct Args {
  sr_cloud_nn_desc d;
  float4* tgt4;      // [n_target]
  uint2* part;       // [slices][n_query]: d2 bits, index
  double* stat;      // [n_tiles][5]
  int64_t chunk, n_tiles;
  int slices;
};

__global__ __launch_bounds__(CE_T) void cloud_hist_zero_kernel(uint32_t* hist, int n) {
  const int e = blockIdx.x * CE_T + threadIdx.x;
  if (e < n) hist[e] = 0;
}

__global__ __launch_bounds__(CE_T) void cloud_prep_kernel(Args a) {
  const int64_t i = (int64_t)blockIdx.x * CE_T + threadIdx.x;
  if (i >= a.d.n_target) return;
  float x, y, z;
  if (sr::load_point(a.d.target + 3 * i, a.d.target_xform, x, y, z)) x = y = z = pos_inf();
  a.tgt4[i] = make_float4(x, y, z, 0.0f);
}

__global__ __launch_bounds__(CE_T) void cloud_sweep_kernel(Args a) {
  __shared__ float4 s_t[TT];
  const int t = threadIdx.x;
  const int64_t nq = a.d.n_query, nt = a.d.n_target;
  const int64_t q0 = (int64_t)blockIdx.x * QTILE;
  float qx[QPL], qy[QPL], qz[QPL], best[QPL];
  int bi[QPL];
  bool bad[QPL];
#pragma unroll
  for (int k = 0; k < QPL; ++k) {
    const int64_t q = q0 + k * CE_T + t;
    qx[k] = qy[k] = qz[k] = 0.0f;
    bad[k] = true;
    if (q < nq) bad[k] = sr::load_point(a.d.query + 3 * q, a.d.query_xform, qx[k], qy[k], qz[k]);
    if (bad[k]) qx[k] = qy[k] = qz[k] = 0.0f;  // the sweep runs on finite numbers; the result is discarded
    best[k] = pos_inf();
    bi[k] = -1;
  }
  const int64_t t_begin = (int64_t)blockIdx.y * a.chunk;
  const int64_t t_end = t_begin + a.chunk < nt ? t_begin + a.chunk : nt;
  for (int64_t base = t_begin; base < t_end; base += TT) {
    __syncthreads();  // the previous tile has been read
#pragma unroll
    for (int e = 0; e < TT / CE_T; ++e) {
      const int64_t j = base + e * CE_T + t;
      float4 v = make_float4(pos_inf(), pos_inf(), pos_inf(), 0.0f);  // past the slice: never selected
      if (j < t_end) v = a.tgt4[j];
      s_t[e * CE_T + t] = v;
    }
    __syncthreads();
    const int n = (int)(t_end - base < TT ? t_end - base : TT);
    const int n8 = (n + 7) & ~7;  // <= TT; the slots past n hold +Inf
    const uint32_t ib = (uint32_t)base;
#pragma unroll 1
    for (int j = 0; j < n8; j += 8) {
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const float4 tv = s_t[j + u];  // every lane the same address: a broadcast read
#pragma unroll
        for (int k = 0; k < QPL; ++k) {
          const float dx = qx[k] - tv.x, dy = qy[k] - tv.y, dz = qz[k] - tv.z;
          const float d2 = fmaf(dz, dz, fmaf(dy, dy, dx * dx));
          const bool lt = d2 < best[k];
          best[k] = lt ? d2 : best[k];
          bi[k] = lt ? (int)(ib + j + u) : bi[k];
        }
      }
    }
  }
#pragma unroll
  for (int k = 0; k < QPL; ++k) {
    const int64_t q = q0 + k * CE_T + t;
    if (q < nq) {
      uint2 o = make_uint2(__float_as_uint(best[k]), (uint32_t)bi[k]);
      if (bad[k]) o = make_uint2(sr::PINF_BITS, 0xffffffffu);
      a.part[(int64_t)blockIdx.y * nq + q] = o;
    }
  }
}

__global__ __launch_bounds__(CE_T) void cloud_finish_kernel(Args a) {
  __shared__ uint32_t s_hist[MAX_BINS + 2];
  __shared__ double s_red[5 * CE_T];
  const int t = threadIdx.x, n_slots = a.d.n_bins + 2;
  const int64_t nq = a.d.n_query, q0 = (int64_t)blockIdx.x * QTILE;
  if (a.d.hist) {
    sr::hist_clear<CE_T>(s_hist, n_slots);
    __syncthreads();
  }
  double acc[5] = {0.0, 0.0, 0.0, 0.0, 0.0};  // n_finite, sum d, sum d^2, n_nonfinite, max d
#pragma unroll 1
  for (int k = 0; k < QPL; ++k) {
    const int64_t q = q0 + k * CE_T + t;
    if (q >= nq) break;
    float best = pos_inf();
    int bi = -1;
    for (int s = 0; s < a.slices; ++s) {  // ascending slices, strict comparison: the lowest index wins
      const uint2 p = a.part[(int64_t)s * nq + q];
      const float d2 = __uint_as_float(p.x);
      if (d2 < best) {
        best = d2;
        bi = (int)p.y;
      }
    }
    const bool bad = bi < 0;
    const float d = __fsqrt_rn(bad ? 0.0f : best);
    // the NaN leaves as bits: under -fno-honor-nans a float select may drop it
    if (a.d.dist) reinterpret_cast<uint32_t*>(a.d.dist)[q] = bad ? sr::QNAN_BITS : __float_as_uint(d);
    if (a.d.index) a.d.index[q] = bi;
    if (a.d.hist) atomicAdd(&s_hist[bad ? a.d.n_bins + 1 : sr::hist_slot(d, a.d.bin_len, a.d.n_bins)], 1u);
    if (bad) {
      acc[3] += 1.0;
    } else {
      const double dd = (double)d;
      acc[0] += 1.0;
      acc[1] += dd;
      acc[2] += dd * dd;
      if (dd > acc[4]) acc[4] = dd;
    }
  }
  if (a.d.hist) {
    __syncthreads();
    sr::hist_flush<CE_T>(s_hist, a.d.hist, n_slots);
  }
  if (a.d.stats) {
    sr::block_reduce<CE_T, 5, true>(acc, s_red);
    if (t == 0) {
      double* o = a.stat + 5 * (int64_t)blockIdx.x;
      o[0] = acc[0], o[1] = acc[1], o[2] = acc[2], o[3] = acc[4], o[4] = acc[3];
    }
  }
}

__global__ __launch_bounds__(CE_T) void cloud_stats_kernel(Args a) {
  __shared__ double s_red[5 * CE_T];
  const int t = threadIdx.x;
  const int64_t run = (a.n_tiles + CE_T - 1) / CE_T;
  const int64_t lo = run * t, hi = lo + run < a.n_tiles ? lo + run : a.n_tiles;
  double acc[5] = {0.0, 0.0, 0.0, 0.0, 0.0};  // as in cloud_finish_kernel
  for (int64_t b = lo; b < hi; ++b) {  // ascending workgroups
    const double* p = a.stat + 5 * b;
    acc[0] += p[0];
    acc[1] += p[1];
    acc[2] += p[2];
    acc[3] += p[4];
    if (p[3] > acc[4]) acc[4] = p[3];
  }
  sr::block_reduce<CE_T, 5, true>(acc, s_red);
  if (t == 0) {
    double* o = a.d.stats;
    o[0] = acc[0], o[1] = acc[1], o[2] = acc[2], o[3] = acc[4], o[4] = acc[3], o[5] = 0.0;
  }
}

}  // namespace

extern "C" int64_t sr_cloud_nn_workspace(int64_t n_query, int64_t n_target, int target_chunk, int has_xform) {
  (void)has_xform;  // the targets are staged through the workspace with or without a transform
  Plan p;
  return make_plan(n_query, n_target, target_chunk, p) ? p.bytes : 0;
}

extern "C" int sr_cloud_nn(sr_stream_t stream, const sr_cloud_nn_desc* desc) {
  SR_CHECK(desc, SR_EINVAL, "sr_cloud_nn: null desc");
  Args a;
  a.d = *desc;
  const sr_cloud_nn_desc& d = a.d;
  SR_CHECK(d.query && d.target && d.workspace, SR_EINVAL, "sr_cloud_nn: null query, target or workspace");
  SR_CHECK(d.n_query >= 1 && d.n_query <= MAX_POINTS && d.n_target >= 1 && d.n_target <= MAX_POINTS, SR_EINVAL,
           "sr_cloud_nn: n_query %lld / n_target %lld outside [1, 2^31 - 1]", (long long)d.n_query, (long long)d.n_target);
  SR_CHECK(d.dist || d.index || d.hist || d.stats, SR_EINVAL, "sr_cloud_nn: every output is NULL");
  if (d.hist) {
    SR_CHECK(d.n_bins > 0 && d.n_bins <= MAX_BINS, SR_EINVAL, "sr_cloud_nn: n_bins %d outside [1, %d]", d.n_bins, MAX_BINS);
    SR_CHECK(sr::positive_finite(d.bin_len), SR_EINVAL, "sr_cloud_nn: bin_len must be positive and finite");
  }
  SR_CHECK(d.target_chunk >= 0 && d.target_chunk % 64 == 0, SR_EINVAL,
           "sr_cloud_nn: target_chunk %d must be 0 or a positive multiple of 64", d.target_chunk);
  Plan p;
  SR_CHECK(make_plan(d.n_query, d.n_target, d.target_chunk, p), SR_EINVAL,
           "sr_cloud_nn: target_chunk %d cuts %lld targets into more than %d slices", d.target_chunk, (long long)d.n_target,
           MAX_SLICES);
  SR_CHECK_WORKSPACE("sr_cloud_nn", d.workspace, d.workspace_bytes, p.bytes);
  SR_CHECK(((uintptr_t)d.query_xform & 7) == 0 && ((uintptr_t)d.target_xform & 7) == 0 && ((uintptr_t)d.stats & 7) == 0,
           SR_EINVAL, "sr_cloud_nn: fp64 buffers must be 8-byte aligned");
  char* ws = (char*)d.workspace;
  a.tgt4 = (float4*)ws;
  a.part = (uint2*)(ws + p.off_part);
  a.stat = (double*)(ws + p.off_stat);
  a.chunk = p.chunk, a.slices = p.slices, a.n_tiles = p.n_tiles;
  hipStream_t s = (hipStream_t)stream;
  if (d.hist) {
    const int n_hist = d.n_bins + 2;
    hipLaunchKernelGGL(cloud_hist_zero_kernel, dim3((n_hist + CE_T - 1) / CE_T), dim3(CE_T), 0, s, d.hist, n_hist);
  }
  hipLaunchKernelGGL(cloud_prep_kernel, dim3((unsigned)((d.n_target + CE_T - 1) / CE_T)), dim3(CE_T), 0, s, a);
  hipLaunchKernelGGL(cloud_sweep_kernel, dim3((unsigned)p.n_tiles, (unsigned)p.slices), dim3(CE_T), 0, s, a);
  hipLaunchKernelGGL(cloud_finish_kernel, dim3((unsigned)p.n_tiles), dim3(CE_T), 0, s, a);
  if (d.stats) hipLaunchKernelGGL(cloud_stats_kernel, dim3(1), dim3(CE_T), 0, s, a);
  sr::note_kernel("cloud_sweep_kernel");
  return sr::check_launch("sr_cloud_nn");
}
