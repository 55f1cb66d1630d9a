// Downsampling a point cloud to a voxel grid on gfx950: points in, one point per occupied voxel out, in a
// fixed order, with the mean or the best member of every voxel.
//
// Contract (DESIGN.md "Downsampling point clouds", include/sfm_amd.h).  Everything that decides a result
// is a test on the bits, an integer, or an IEEE fp64 operation that is not contracted.
//   skipped     mask byte 0; a non-finite coordinate; under BEST a NaN weight; a non-finite transformed point
//   q           p, or fl32(s (R p) + t) by sr::load_point / sr::xform_point (sr_eval.h; sr_cloud_nn's transform)
//   cell        f = floor(((double)q - origin) / voxel) per axis; considered when -2^(b-1) <= f < 2^(b-1) on
//               all three, compared in fp64; outside otherwise
//   key         (u_z << 2b) | (u_y << b) | u_x, u = f + 2^(b-1); 2^(3b) for what is not considered
//   rows        ascending key; members in ascending input index (the sort is stable and carries the index)
//
//   voxel_key_kernel     keys, and the considered / skipped / outside counts (ballots, then one integer
//                        atomic per workgroup and counter)
//   sr::sort_launch      sr_sort_pairs' passes on 3b + 1 bits: sorted keys and the permutation
//   voxel_head_count_kernel   heads (a sorted key that differs from its predecessor and is no sentinel)
//                        per tile of 2048 sorted positions
//   voxel_head_scan_kernel    one workgroup: exclusive scan of the tile counts (sr::scan_row); the total is the voxel count
//   voxel_head_local_kernel   the row of every sorted position: tile base + sr::block_exclusive inside the workgroup.
//                        Writes the start of every voxel and voxel_of.
//   voxel_reduce_kernel  one lane per voxel walks its members from its start while the key stays: the
//                        left-to-right fp64 sum the contract asks for.  A cloud with everything in one
//                        voxel is walked by one lane: slow and still correct.
//
// The Makefile builds this file with -ffp-contract=off -fhonor-nans.  Without the first, sr::xform_point's
// products and sums, which live in headers, are fused into FMAs whatever a pragma here says; without the
// second the compiler reads the test on the exponent bits as a float classification, assumes that no
// float is a NaN and reduces it to |x| == Inf, so that a NaN coordinate would count as finite.
#include "sr_common.h"
#include "sr_eval.h"

namespace {

constexpr int VX_T = 256;                  // threads of every workgroup here
constexpr int VX_PER = 8;                  // sorted positions per lane of the head kernels
constexpr int VX_TILE = VX_T * VX_PER;     // 2048
constexpr int64_t VX_MAX_N = 2147483647LL;
constexpr int VX_MAX_BITS = 21;

using sr::align16;
using sr::finite64;

struct VoxPlan {
  int64_t tiles;
  int64_t off_keys, off_skeys, off_perm, off_start, off_tile, off_cnt, off_sort, bytes;
};

bool vox_plan(int64_t n, VoxPlan& p) {
  if (n < 1 || n > VX_MAX_N) return false;
  p.tiles = (n + VX_TILE - 1) / VX_TILE;
  int64_t o = 0;
  p.off_keys = o, o = align16(o + 8 * n);
  p.off_skeys = o, o = align16(o + 8 * n);
  p.off_perm = o, o = align16(o + 4 * n);
  p.off_start = o, o = align16(o + 4 * n);
  p.off_tile = o, o = align16(o + 4 * p.tiles);
  p.off_cnt = o, o += 16;
  p.off_sort = o, o += sr::sort_workspace(n);
  p.bytes = o;
  return true;
}

struct VoxArgs {
  sr_cloud_voxel_desc d;
  uint64_t* keys;     // [n] in input order
  uint64_t* skeys;    // [n] sorted
  uint32_t* perm;     // [n] input index of every sorted position
  uint32_t* start;    // [n] sorted position of every voxel's first member
  uint32_t* tilecnt;  // [tiles] heads per tile, then their exclusive scan
  uint32_t* cnt;      // [4] voxels, considered, skipped, outside
  int64_t tiles;
  double lo, hi;      // -2^(b-1), 2^(b-1)
  uint64_t sentinel;  // 2^(3b)
};

// the transformed point of element i; true if it is to be skipped for its coordinates
__device__ inline bool load_q(const VoxArgs& a, int64_t i, float& x, float& y, float& z) {
  return sr::load_point(a.d.points + i * a.d.ldp, a.d.xform, x, y, z);
}

__device__ inline double cell_of(float q, double origin, double voxel) {
  return floor(__ddiv_rn(__dsub_rn((double)q, origin), voxel));
}

__global__ __launch_bounds__(VX_T) void voxel_key_kernel(VoxArgs a) {
  __shared__ uint32_t s_cnt[3];
  const int t = threadIdx.x;
  const sr_cloud_voxel_desc& d = a.d;
  if (t < 3) s_cnt[t] = 0;
  __syncthreads();
  const int64_t i = (int64_t)blockIdx.x * VX_T + t;
  bool considered = false, skipped = false, outside = false;
  if (i < d.n) {
    float x, y, z;
    skipped = load_q(a, i, x, y, z);
    if (d.mask && d.mask[i] == 0) skipped = true;
    if (d.mode == SR_VOXEL_BEST && d.weight && sr::bits_nan(d.weight[i])) skipped = true;
    uint64_t key = a.sentinel;
    if (!skipped) {
      const double fx = cell_of(x, d.origin[0], d.voxel), fy = cell_of(y, d.origin[1], d.voxel),
                   fz = cell_of(z, d.origin[2], d.voxel);
      considered = fx >= a.lo && fx < a.hi && fy >= a.lo && fy < a.hi && fz >= a.lo && fz < a.hi;
      outside = !considered;
      if (considered) {
        const int64_t half = (int64_t)a.hi;
        const uint64_t ux = (uint64_t)((int64_t)fx + half), uy = (uint64_t)((int64_t)fy + half),
                       uz = (uint64_t)((int64_t)fz + half);
        key = (uz << (2 * d.axis_bits)) | (uy << d.axis_bits) | ux;
      }
    }
    a.keys[i] = key;
  }
  const uint64_t bc = __ballot(considered), bs = __ballot(skipped), bo = __ballot(outside);
  if ((t & 63) == 0) {
    if (bc) atomicAdd(&s_cnt[0], (uint32_t)__popcll(bc));
    if (bs) atomicAdd(&s_cnt[1], (uint32_t)__popcll(bs));
    if (bo) atomicAdd(&s_cnt[2], (uint32_t)__popcll(bo));
  }
  __syncthreads();
  if (t < 3 && s_cnt[t]) atomicAdd(&a.cnt[1 + t], s_cnt[t]);
}

// heads among the VX_PER sorted positions from j0; bit u set: position j0 + u starts a voxel
__device__ inline uint32_t head_bits(const VoxArgs& a, int64_t j0, uint64_t (&k)[VX_PER]) {
  const int64_t n = a.d.n;
  uint64_t prev = j0 > 0 && j0 < n ? a.skeys[j0 - 1] : 0u;
  uint32_t bits = 0;
#pragma unroll
  for (int u = 0; u < VX_PER; ++u) {
    const int64_t j = j0 + u;
    k[u] = j < n ? a.skeys[j] : a.sentinel;
    if (j < n && k[u] != a.sentinel && (j == 0 || k[u] != prev)) bits |= 1u << u;
    prev = k[u];
  }
  return bits;
}

__global__ __launch_bounds__(VX_T) void voxel_head_count_kernel(VoxArgs a) {
  __shared__ uint32_t s_scan[VX_T];
  const int t = threadIdx.x;
  uint64_t k[VX_PER];
  const uint32_t bits = head_bits(a, (int64_t)blockIdx.x * VX_TILE + (int64_t)t * VX_PER, k);
  uint32_t total;
  sr::block_exclusive<VX_T>((uint32_t)__popc(bits), s_scan, total);
  if (t == 0) a.tilecnt[blockIdx.x] = total;
}

__global__ __launch_bounds__(VX_T) void voxel_head_scan_kernel(VoxArgs a) {
  __shared__ uint32_t s_scan[VX_T];
  const uint32_t heads = sr::scan_row<VX_T>(a.tiles, 0u, s_scan, [&](int64_t e) { return a.tilecnt[e]; },
                                            [&](int64_t e, uint32_t x) { a.tilecnt[e] = x; });
  if (threadIdx.x == 0) a.cnt[0] = heads;
}

__global__ __launch_bounds__(VX_T) void voxel_head_local_kernel(VoxArgs a) {
  __shared__ uint32_t s_scan[VX_T];
  const int t = threadIdx.x;
  const int64_t n = a.d.n, j0 = (int64_t)blockIdx.x * VX_TILE + (int64_t)t * VX_PER;
  uint64_t k[VX_PER];
  const uint32_t bits = head_bits(a, j0, k);
  uint32_t total;
  uint32_t row = a.tilecnt[blockIdx.x] + sr::block_exclusive<VX_T>((uint32_t)__popc(bits), s_scan, total);  // heads before j0
#pragma unroll
  for (int u = 0; u < VX_PER; ++u) {
    const int64_t j = j0 + u;
    if (j >= n) break;
    if ((bits >> u) & 1u) {
      if ((int64_t)row < n) a.start[row] = (uint32_t)j;  // always: row < the number of heads <= n
      ++row;
    }
    if (a.d.voxel_of) {
      const uint32_t i = a.perm[j];
      if ((int64_t)i < n) a.d.voxel_of[i] = k[u] != a.sentinel ? (int32_t)(row - 1) : -1;
    }
  }
}

__global__ __launch_bounds__(VX_T) void voxel_reduce_kernel(VoxArgs a) {
  const sr_cloud_voxel_desc& d = a.d;
  const int t = threadIdx.x;
  if (blockIdx.x == 0 && t < 4 && d.counts) d.counts[t] = a.cnt[t];
  const int64_t v = (int64_t)blockIdx.x * VX_T + t, n = d.n;
  const int64_t rows = (int64_t)a.cnt[0] < d.capacity ? (int64_t)a.cnt[0] : d.capacity;
  if (v >= rows) return;
  const int64_t j0 = a.start[v];
  const uint64_t key = a.skeys[j0];
  uint32_t count = 0, pick = 0;
  float ox, oy, oz;
  uint32_t oa[SR_VOXEL_MAX_ATTR];
  if (d.mode == SR_VOXEL_MEAN) {
    double sx = 0.0, sy = 0.0, sz = 0.0, sa[SR_VOXEL_MAX_ATTR];
#pragma unroll
    for (int c = 0; c < SR_VOXEL_MAX_ATTR; ++c) sa[c] = 0.0;
    for (int64_t j = j0; j < n && a.skeys[j] == key; ++j) {  // ascending input index
      const int64_t i = a.perm[j];
      if (i >= n) break;
      if (count == 0) pick = (uint32_t)i;
      float x, y, z;
      load_q(a, i, x, y, z);
      sx = __dadd_rn(sx, (double)x), sy = __dadd_rn(sy, (double)y), sz = __dadd_rn(sz, (double)z);
#pragma unroll
      for (int c = 0; c < SR_VOXEL_MAX_ATTR; ++c)
        if (c < d.n_attr) sa[c] = __dadd_rn(sa[c], (double)d.attr[i * d.lda + c]);
      ++count;
    }
    const double cd = (double)count;
    ox = (float)__ddiv_rn(sx, cd), oy = (float)__ddiv_rn(sy, cd), oz = (float)__ddiv_rn(sz, cd);
#pragma unroll
    for (int c = 0; c < SR_VOXEL_MAX_ATTR; ++c) oa[c] = c < d.n_attr ? __float_as_uint((float)__ddiv_rn(sa[c], cd)) : 0u;
  } else {
    float best = 0.0f;
    for (int64_t j = j0; j < n && a.skeys[j] == key; ++j) {
      const int64_t i = a.perm[j];
      if (i >= n) break;
      const float w = d.weight ? d.weight[i] : 0.0f;
      if (count == 0 || w > best) best = w, pick = (uint32_t)i;  // strict: equal weights keep the lowest index
      ++count;
    }
    load_q(a, pick, ox, oy, oz);
#pragma unroll
    for (int c = 0; c < SR_VOXEL_MAX_ATTR; ++c)
      oa[c] = c < d.n_attr ? __float_as_uint(d.attr[(int64_t)pick * d.lda + c]) : 0u;
  }
  uint32_t* op = reinterpret_cast<uint32_t*>(d.out_points) + 3 * v;  // as bits: a float select may not keep them
  op[0] = __float_as_uint(ox), op[1] = __float_as_uint(oy), op[2] = __float_as_uint(oz);
  if (d.out_attr) {
    uint32_t* o = reinterpret_cast<uint32_t*>(d.out_attr) + v * d.n_attr;
#pragma unroll
    for (int c = 0; c < SR_VOXEL_MAX_ATTR; ++c)
      if (c < d.n_attr) o[c] = oa[c];
  }
  if (d.out_count) d.out_count[v] = count;
  if (d.out_index) d.out_index[v] = pick;
  if (d.out_key) d.out_key[v] = key;
}

}  // namespace

extern "C" int64_t sr_cloud_voxel_workspace(int64_t n) {
  VoxPlan p;
  return vox_plan(n, p) ? p.bytes : 0;
}

extern "C" int sr_cloud_voxel(sr_stream_t stream, const sr_cloud_voxel_desc* desc) {
  SR_CHECK(desc, SR_EINVAL, "sr_cloud_voxel: null desc");
  VoxArgs a{};
  a.d = *desc;
  const sr_cloud_voxel_desc& d = a.d;
  SR_CHECK(d.points && d.out_points && d.workspace, SR_EINVAL, "sr_cloud_voxel: null points, out_points or workspace");
  SR_CHECK(d.n >= 1 && d.n <= VX_MAX_N, SR_EINVAL, "sr_cloud_voxel: n %lld outside [1, 2^31 - 1]", (long long)d.n);
  SR_CHECK(d.ldp >= 3, SR_EINVAL, "sr_cloud_voxel: ldp %lld below 3", (long long)d.ldp);
  SR_CHECK(d.n_attr >= 0 && d.n_attr <= SR_VOXEL_MAX_ATTR, SR_EINVAL, "sr_cloud_voxel: n_attr %d outside [0, %d]", d.n_attr,
           SR_VOXEL_MAX_ATTR);
  SR_CHECK(d.n_attr == 0 || (d.attr && d.lda >= d.n_attr), SR_EINVAL,
           "sr_cloud_voxel: %d attribute columns need attr and lda >= n_attr (lda %lld)", d.n_attr, (long long)d.lda);
  SR_CHECK(d.mode == SR_VOXEL_MEAN || d.mode == SR_VOXEL_BEST, SR_EINVAL, "sr_cloud_voxel: unknown mode %d", d.mode);
  SR_CHECK(d.mode == SR_VOXEL_BEST || !d.weight, SR_EINVAL, "sr_cloud_voxel: a weight is read under SR_VOXEL_BEST only");
  SR_CHECK(d.axis_bits >= 1 && d.axis_bits <= VX_MAX_BITS, SR_EINVAL, "sr_cloud_voxel: axis_bits %d outside [1, %d]",
           d.axis_bits, VX_MAX_BITS);
  SR_CHECK(finite64(d.origin[0]) && finite64(d.origin[1]) && finite64(d.origin[2]), SR_EINVAL,
           "sr_cloud_voxel: the origin must be finite");
  SR_CHECK(finite64(d.voxel) && d.voxel > 0.0, SR_EINVAL, "sr_cloud_voxel: voxel must be positive and finite");
  SR_CHECK(d.capacity >= 1 && d.capacity <= d.n, SR_EINVAL, "sr_cloud_voxel: capacity %lld outside [1, %lld]",
           (long long)d.capacity, (long long)d.n);
  VoxPlan p;
  vox_plan(d.n, p);
  SR_CHECK_WORKSPACE("sr_cloud_voxel", d.workspace, d.workspace_bytes, p.bytes);
  SR_CHECK(((uintptr_t)d.xform & 7) == 0 && ((uintptr_t)d.out_key & 7) == 0, SR_EINVAL,
           "sr_cloud_voxel: xform and out_key must be 8-byte aligned");
  char* ws = (char*)d.workspace;
  a.keys = (uint64_t*)(ws + p.off_keys);
  a.skeys = (uint64_t*)(ws + p.off_skeys);
  a.perm = (uint32_t*)(ws + p.off_perm);
  a.start = (uint32_t*)(ws + p.off_start);
  a.tilecnt = (uint32_t*)(ws + p.off_tile);
  a.cnt = (uint32_t*)(ws + p.off_cnt);
  a.tiles = p.tiles;
  a.hi = (double)(int64_t(1) << (d.axis_bits - 1)), a.lo = -a.hi;
  a.sentinel = uint64_t(1) << (3 * d.axis_bits);
  hipStream_t s = (hipStream_t)stream;
  const dim3 block(VX_T), tile_grid((unsigned)p.tiles);
  (void)hipMemsetAsync(a.cnt, 0, 16, s);
  hipLaunchKernelGGL(voxel_key_kernel, dim3((unsigned)((d.n + VX_T - 1) / VX_T)), block, 0, s, a);
  sr::sort_launch(s, a.keys, nullptr, a.skeys, a.perm, d.n, 3 * d.axis_bits + 1, ws + p.off_sort);
  hipLaunchKernelGGL(voxel_head_count_kernel, tile_grid, block, 0, s, a);
  hipLaunchKernelGGL(voxel_head_scan_kernel, dim3(1), block, 0, s, a);
  hipLaunchKernelGGL(voxel_head_local_kernel, tile_grid, block, 0, s, a);
  hipLaunchKernelGGL(voxel_reduce_kernel, dim3((unsigned)((d.capacity + VX_T - 1) / VX_T)), block, 0, s, a);
  sr::note_kernel("voxel_reduce_kernel");
  return sr::check_launch("sr_cloud_voxel");
}
