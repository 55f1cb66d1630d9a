// Rendering a point cloud into camera views on gfx950: n points and V cameras in, per camera one z-buffered
// depth image, one index image and optional attribute images out.
//
// Contract (DESIGN.md "Rendering point clouds", include/sfm_amd.h).  Everything that decides a result is a
// test on the bits, an integer, or an IEEE fp64 operation that is not contracted.
//   skipped     (for view v) mask byte 0; a non-finite coordinate; a non-finite transformed point; view_id and
//               exclude both given and view_id[i] == exclude[v]
//   q           p, or fl32(s (R p) + t) by sr::xform_point (sr_eval.h; sr_cloud_nn's transform)
//   camera      E = extrinsic[v], fp32 [3][4], camera from world, OpenCV, widened exactly;
//               c_r = ((E[r][0] q_x + E[r][1] q_y) + E[r][2] q_z) + E[r][3] in fp64
//   clipped     a non-finite c_r (on the bits), c_z < z_near or c_z > z_far, compared in fp64
//   pixel       u = fx (c_x / c_z) + cx, v = fy (c_y / c_z) + cy with true fp64 divisions; fx, fy, cx, cy =
//               K[0][0], K[1][1], K[0][2], K[1][2] of the fp32 intrinsic[v]; ix = floor(u + 0.5),
//               iy = floor(v + 0.5): pixel centres at integers
//   outside     not (0 <= ix < W and 0 <= iy < H), compared in fp64 before any conversion to an integer;
//               every other point that is neither skipped nor clipped is drawn
//   footprint   the (2 radius + 1)^2 pixels around the centre, those outside the frame dropped
//   z-buffer    key (bits(fl32(c_z)) << 32) | i, minimum per pixel; the empty key is all ones (z_near > 0 makes
//               the depth's bit pattern order like its value, and i < 2^31 keeps a key below all ones)
//   outputs     depth: the winner's fl32(c_z), 0x7fc00000 when empty; index: its i, -1 when empty; out_attr:
//               its attribute row by its bits, attr_fill when empty; counts[v]: covered, drawn, clipped, outside
//
//   render_clear_kernel    the key image to all ones, 16 bytes per lane, and the counts to 0 (the caller's, or
//                          the workspace's when counts is NULL) with the workspace's partial counts
//   render_draw_kernel     grid (point tiles, views), 4 points per lane, consecutive lanes on consecutive
//                          points: a cloud that comes from raster-ordered maps sends a wave's atomics to
//                          neighbouring pixels.  One 64-bit unsigned atomic minimum per footprint pixel
//                          (global_atomic_umin_x2, no compare-and-swap loop).  The camera's 12 + 4 numbers are
//                          workgroup-uniform: scalar loads.  The three counts: ballot, popcount, one LDS atomic
//                          per wave, one global integer atomic per workgroup and count -- into one of 64 slots
//                          per view: with one word per count and view the (tiles x views) workgroups queued on
//                          it and the kernel ran at the rate of those atomics (measurements).
//   render_resolve_kernel  one lane per pixel: decodes the key, writes depth and index, gathers the attribute
//                          row through the index, counts covered pixels the same way; the first workgroup of
//                          every view sums the draw kernel's slots.
//
// Integer atomics only, no workgroup waits on another, and a minimum does not depend on arrival order: any two
// runs give the same bits.  Inputs are never written.
//
// The pre-test (template parameter of the draw kernel): an ordinary load of the pixel's key before the atomic,
// which is skipped when the loaded key is already <= the lane's.  Safe, because within the draw kernel a key
// only decreases, so a stale value is never below the current one and the worst outcome is a redundant atomic.
// SR_RENDER_PRETEST=0 at compile time builds the draw kernel without it.  With it the call is 1.5 to 4.6 times
// faster at every shape and radius measured (measurements): most points lose at their pixel.
//
// The Makefile builds this file with -ffp-contract=off -fhonor-nans, for sr_cloud_voxel.hip's two reasons: the
// shared transform's products and sums are header code, and the tests on the exponent bits must see NaNs.
#include "sr_common.h"
#include "sr_eval.h"

#ifndef SR_RENDER_PRETEST
#define SR_RENDER_PRETEST 1
#endif

namespace {

constexpr int RD_T = 256;      // threads of every workgroup here
constexpr int RD_PER = 4;      // points per lane of the draw kernel, RD_T apart: consecutive lanes, consecutive points
constexpr int RD_SLOTS = 64;   // partial counts per view: a workgroup adds to slot blockIdx.x % 64, so that the
                               // (point tiles x views) workgroups do not queue on three words per view
constexpr int64_t RD_MAX_N = 2147483647LL;
constexpr int RD_MAX_VIEWS = 65535;

using sr::bits_nonfinite;
using sr::bits_nonfinite64;
using sr::finite64;

struct RenderPlan {
  int64_t pixels;    // V H W
  int64_t key_bytes; // the key image, padded to 16 bytes
  int64_t off_cnt, off_slots, bytes;
};

bool render_plan(int n_views, int height, int width, RenderPlan& p) {
  if (n_views < 1 || n_views > RD_MAX_VIEWS || height < 1 || width < 1) return false;
  const int64_t hw = (int64_t)height * width;  // < 2^62
  if (hw > RD_MAX_N || hw * n_views > RD_MAX_N) return false;
  p.pixels = hw * n_views;
  p.key_bytes = sr::align16(8 * p.pixels);
  p.off_cnt = p.key_bytes;
  p.off_slots = p.off_cnt + 16 * (int64_t)n_views;
  p.bytes = p.off_slots + 16 * (int64_t)RD_SLOTS * n_views;
  return true;
}

struct RenderArgs {
  sr_cloud_render_desc d;
  uint64_t* keys;  // [V][H][W]
  uint32_t* cnt;   // [V][4] covered, drawn, clipped, outside: the caller's counts, or the workspace's
  uint32_t* slots; // [V][RD_SLOTS][4] partial drawn, clipped, outside in words 1 .. 3
  int64_t key_chunks;  // 16-byte pieces of the key image
};

__global__ __launch_bounds__(RD_T) void render_clear_kernel(RenderArgs a) {
  const int64_t j = (int64_t)blockIdx.x * RD_T + threadIdx.x;
  if (j < a.key_chunks) reinterpret_cast<uint4*>(a.keys)[j] = make_uint4(0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu);
  if (j < 4 * (int64_t)a.d.n_views) a.cnt[j] = 0u;
  if (j < 4 * (int64_t)RD_SLOTS * a.d.n_views) a.slots[j] = 0u;
}

template <bool PRETEST>
__global__ __launch_bounds__(RD_T) void render_draw_kernel(RenderArgs a) {
  __shared__ uint32_t s_cnt[3];
  const sr_cloud_render_desc& d = a.d;
  const int t = threadIdx.x, v = blockIdx.y;
  if (t < 3) s_cnt[t] = 0;
  __syncthreads();
  uint32_t n_drawn = 0, n_clipped = 0, n_outside = 0;  // of the wave, in every lane
  for (int k = 0; k < RD_PER; ++k) {
  const int64_t i = ((int64_t)blockIdx.x * RD_PER + k) * RD_T + t;
  bool drawn = false, clipped = false, outside = false;
  if (i < d.n) {
    const float* p = d.points + i * d.ldp;
    float x = p[0], y = p[1], z = p[2];
    bool skipped = bits_nonfinite(x) || bits_nonfinite(y) || bits_nonfinite(z);
    if (d.mask && d.mask[i] == 0) skipped = true;
    if (d.view_id && d.view_id[i] == d.exclude[v]) skipped = true;
    if (!skipped && d.xform) {
      sr::xform_point(d.xform, x, y, z);
      skipped = bits_nonfinite(x) || bits_nonfinite(y) || bits_nonfinite(z);
    }
    if (!skipped) {
      const float* E = d.extrinsic + 12 * (int64_t)v;
      const float* K = d.intrinsic + 9 * (int64_t)v;
      const double qx = (double)x, qy = (double)y, qz = (double)z;
      double c[3];
#pragma unroll
      for (int r = 0; r < 3; ++r)
        c[r] = __dadd_rn(__dadd_rn(__dadd_rn(__dmul_rn((double)E[4 * r], qx), __dmul_rn((double)E[4 * r + 1], qy)),
                                   __dmul_rn((double)E[4 * r + 2], qz)),
                         (double)E[4 * r + 3]);
      clipped = bits_nonfinite64(c[0]) || bits_nonfinite64(c[1]) || bits_nonfinite64(c[2]) || c[2] < d.z_near ||
                c[2] > d.z_far;
      if (!clipped) {
        const double u = __dadd_rn(__dmul_rn((double)K[0], __ddiv_rn(c[0], c[2])), (double)K[2]);
        const double w = __dadd_rn(__dmul_rn((double)K[4], __ddiv_rn(c[1], c[2])), (double)K[5]);
        const double fx = floor(__dadd_rn(u, 0.5)), fy = floor(__dadd_rn(w, 0.5));
        drawn = fx >= 0.0 && fx < (double)d.width && fy >= 0.0 && fy < (double)d.height;  // a NaN is outside
        outside = !drawn;
        if (drawn) {
          const int ix = (int)fx, iy = (int)fy, r = d.radius;
          const uint64_t key = ((uint64_t)__float_as_uint((float)c[2]) << 32) | (uint64_t)i;
          uint64_t* img = a.keys + (int64_t)v * d.height * d.width;
          const int y0 = iy - r < 0 ? 0 : iy - r, y1 = iy + r >= d.height ? d.height - 1 : iy + r;
          const int x0 = ix - r < 0 ? 0 : ix - r, x1 = ix + r >= d.width ? d.width - 1 : ix + r;
          for (int yy = y0; yy <= y1; ++yy)
            for (int xx = x0; xx <= x1; ++xx) {
              uint64_t* cell = img + (int64_t)yy * d.width + xx;  // in [0, H W) of view v's image
              if (PRETEST && __hip_atomic_load(cell, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) <= key) continue;
              __hip_atomic_fetch_min(cell, key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        }
      }
    }
  }
  n_drawn += (uint32_t)__popcll(__ballot(drawn));
  n_clipped += (uint32_t)__popcll(__ballot(clipped));
  n_outside += (uint32_t)__popcll(__ballot(outside));
  }
  if ((t & 63) == 0) {
    if (n_drawn) atomicAdd(&s_cnt[0], n_drawn);
    if (n_clipped) atomicAdd(&s_cnt[1], n_clipped);
    if (n_outside) atomicAdd(&s_cnt[2], n_outside);
  }
  __syncthreads();
  if (t < 3 && s_cnt[t]) atomicAdd(&a.slots[4 * ((int64_t)v * RD_SLOTS + (blockIdx.x & (RD_SLOTS - 1))) + 1 + t], s_cnt[t]);
}

// grid (pixel tiles of one view, views)
__global__ __launch_bounds__(RD_T) void render_resolve_kernel(RenderArgs a) {
  __shared__ uint32_t s_cov;
  const sr_cloud_render_desc& d = a.d;
  const int t = threadIdx.x, v = blockIdx.y;
  if (t == 0) s_cov = 0;
  __syncthreads();
  const int64_t hw = (int64_t)d.height * d.width, j = (int64_t)blockIdx.x * RD_T + t;
  bool covered = false;
  if (j < hw) {
    const int64_t px = (int64_t)v * hw + j;
    const uint64_t key = a.keys[px];
    covered = key != ~uint64_t(0);
    const uint32_t i = (uint32_t)key;
    if (d.depth) reinterpret_cast<uint32_t*>(d.depth)[px] = covered ? (uint32_t)(key >> 32) : sr::QNAN_BITS;
    if (d.index) d.index[px] = covered ? (int32_t)i : -1;
    if (d.out_attr) {
      uint32_t* o = reinterpret_cast<uint32_t*>(d.out_attr) + px * d.n_attr;  // as bits: a float select may not keep them
      const uint32_t* src = reinterpret_cast<const uint32_t*>(d.attr) + (int64_t)i * d.lda;
      const uint32_t fill = __float_as_uint(d.attr_fill);
      const bool ok = covered && (int64_t)i < d.n;  // always, for a covered pixel: the key's low word is an input index
#pragma unroll
      for (int c = 0; c < SR_RENDER_MAX_ATTR; ++c)
        if (c < d.n_attr) o[c] = ok ? src[c] : fill;
    }
  }
  const uint64_t b = __ballot(covered);
  if ((t & 63) == 0 && b) atomicAdd(&s_cov, (uint32_t)__popcll(b));
  __syncthreads();
  if (t == 0 && s_cov) atomicAdd(&a.cnt[4 * v], s_cov);
  if (blockIdx.x == 0 && t >= 1 && t < 4) {  // the draw kernel is over: its partial counts, in slot order
    uint32_t sum = 0;
    for (int s = 0; s < RD_SLOTS; ++s) sum += a.slots[4 * ((int64_t)v * RD_SLOTS + s) + t];
    a.cnt[4 * v + t] = sum;  // words 1 .. 3; the covered count in word 0 is the other workgroups' atomics
  }
}

}  // namespace

extern "C" int64_t sr_cloud_render_workspace(int n_views, int height, int width) {
  RenderPlan p;
  return render_plan(n_views, height, width, p) ? p.bytes : 0;
}

extern "C" int sr_cloud_render(sr_stream_t stream, const sr_cloud_render_desc* desc) {
  SR_CHECK(desc, SR_EINVAL, "sr_cloud_render: null desc");
  RenderArgs a{};
  a.d = *desc;
  const sr_cloud_render_desc& d = a.d;
  SR_CHECK(d.points && d.extrinsic && d.intrinsic && d.workspace, SR_EINVAL,
           "sr_cloud_render: null points, extrinsic, intrinsic or workspace");
  SR_CHECK(d.n >= 1 && d.n <= RD_MAX_N, SR_EINVAL, "sr_cloud_render: n %lld outside [1, 2^31 - 1]", (long long)d.n);
  SR_CHECK(d.ldp >= 3, SR_EINVAL, "sr_cloud_render: ldp %lld below 3", (long long)d.ldp);
  SR_CHECK(d.n_attr >= 0 && d.n_attr <= SR_RENDER_MAX_ATTR, SR_EINVAL, "sr_cloud_render: n_attr %d outside [0, %d]", d.n_attr,
           SR_RENDER_MAX_ATTR);
  SR_CHECK(d.n_attr == 0 || (d.attr && d.out_attr && d.lda >= d.n_attr), SR_EINVAL,
           "sr_cloud_render: %d attribute columns need attr, out_attr and lda >= n_attr (lda %lld)", d.n_attr, (long long)d.lda);
  SR_CHECK(!d.view_id == !d.exclude, SR_EINVAL, "sr_cloud_render: view_id and exclude are given together or not at all");
  SR_CHECK(d.n_views >= 1 && d.n_views <= RD_MAX_VIEWS, SR_EINVAL, "sr_cloud_render: n_views %d outside [1, %d]", d.n_views,
           RD_MAX_VIEWS);
  SR_CHECK(d.height >= 1 && d.width >= 1, SR_EINVAL, "sr_cloud_render: height %d or width %d below 1", d.height, d.width);
  RenderPlan p;
  SR_CHECK(render_plan(d.n_views, d.height, d.width, p), SR_EINVAL, "sr_cloud_render: %d x %d x %d pixels exceed 2^31 - 1",
           d.n_views, d.height, d.width);
  SR_CHECK(d.radius >= 0 && d.radius <= SR_RENDER_MAX_RADIUS, SR_EINVAL, "sr_cloud_render: radius %d outside [0, %d]", d.radius,
           SR_RENDER_MAX_RADIUS);
  SR_CHECK(finite64(d.z_near) && d.z_near > 0.0, SR_EINVAL, "sr_cloud_render: z_near must be positive and finite");
  SR_CHECK(d.z_far >= d.z_near, SR_EINVAL, "sr_cloud_render: z_far must be no NaN and at least z_near");
  SR_CHECK(d.depth || d.index || (d.out_attr && d.n_attr > 0) || d.counts, SR_EINVAL,
           "sr_cloud_render: no output (depth, index, out_attr and counts are all null)");
  SR_CHECK_WORKSPACE("sr_cloud_render", d.workspace, d.workspace_bytes, p.bytes);
  SR_CHECK(((uintptr_t)d.xform & 7) == 0, SR_EINVAL, "sr_cloud_render: xform must be 8-byte aligned");
  if (d.n_attr == 0) a.d.out_attr = nullptr, a.d.attr = nullptr;
  char* ws = (char*)d.workspace;
  a.keys = (uint64_t*)ws;
  a.cnt = d.counts ? d.counts : (uint32_t*)(ws + p.off_cnt);
  a.slots = (uint32_t*)(ws + p.off_slots);
  a.key_chunks = p.key_bytes / 16;
  const int64_t n_slots = 4 * (int64_t)RD_SLOTS * d.n_views;
  const int64_t clear = a.key_chunks > n_slots ? a.key_chunks : n_slots;
  const int64_t tile = (int64_t)RD_T * RD_PER;
  hipStream_t s = (hipStream_t)stream;
  const dim3 block(RD_T);
  const int64_t hw = (int64_t)d.height * d.width;
  hipLaunchKernelGGL(render_clear_kernel, dim3((unsigned)((clear + RD_T - 1) / RD_T)), block, 0, s, a);
  const dim3 draw_grid((unsigned)((d.n + tile - 1) / tile), (unsigned)d.n_views);
  hipLaunchKernelGGL(render_draw_kernel<SR_RENDER_PRETEST != 0>, draw_grid, block, 0, s, a);
  hipLaunchKernelGGL(render_resolve_kernel, dim3((unsigned)((hw + RD_T - 1) / RD_T), (unsigned)d.n_views), block, 0, s, a);
  sr::note_kernel("render_draw_kernel");
  return sr::check_launch("sr_cloud_render");
}
