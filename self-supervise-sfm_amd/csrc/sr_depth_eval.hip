// Scoring a predicted depth map against a reference one on gfx950, and the grid-wide exact select the
// scorer needs for its median alignment and its error quantiles.
//
// Contract (DESIGN.md "Scoring depth maps", include/sfm_amd.h).  Everything that decides a result is a
// test on the bits (the build compiles with -fno-honor-nans), an integer count, or an fp64 operation
// that is written with the uncontracted intrinsics where the bits are part of the contract.
//
// sr_select_ranks: four passes, one per 8-bit digit of the order-preserving key, most significant first
//   select_hist_kernel   grid (rows x blocks_per_row).  A lane walks its slice of the row four elements
//                        at a time (one 16-byte load where the row is aligned), keeps a run of equal
//                        digits in registers and adds the run to the workgroup's LDS histogram when the
//                        digit changes: depth values share their top digit, so the first pass would
//                        otherwise serialise 64 lanes on one LDS word.  An element counts for rank r
//                        when its higher digits equal r's prefix.  Non-zero bins are flushed with
//                        integer atomics.  In the first pass the ranks share histogram 0.
//   select_scan_kernel   one workgroup per group: sr::block_exclusive over the 256 bins of every rank finds the
//                        bin holding the remaining rank, appends it to the prefix, subtracts the bins
//                        below, clears the counters for the next pass; the last pass writes the values.
//   Rows are re-read from global memory in every pass (4 x 4 bytes per element): staging a row once
//   does not fit (268,324 pixels are 1 MiB per view) and a compacted copy would cost a fifth pass.
//
// sr_depth_eval
//   depth_valid_kernel     validity bytes; partials of n, sum p, sum g, sum g p, sum p p over valid pixels
//   depth_fit_kernel       one workgroup per group: sums the partials of its views in ascending order
//                          (stage 0), then (s, t) and the status from the sums, the medians or the
//                          centred sums (stage 1)
//   depth_centred_kernel   SCALE_SHIFT only: partials of sum (p - pm)(g - gm), sum (p - pm)^2
//   depth_error_kernel     a, the error terms, LDS histogram, 13 partials per workgroup
//   depth_group_kernel     one workgroup per group: sums the 13 partials of its views
//   depth_pool_kernel      row n_groups of stats and hist from the group rows, ascending
#include "sr_common.h"
#include "sr_eval.h"

#pragma clang fp contract(off)

namespace {

constexpr int DE_T = 256;                      // threads of every workgroup here
constexpr int64_t SEL_MAX_TOTAL = 2147483648LL;
constexpr int SEL_MAX_DEN = 1 << 20;
constexpr int SEL_MAX_BPR = 65535;
constexpr int SEL_AUTO_BLOCKS = 2048;          // workgroups the automatic split aims for: 8 per CU
constexpr int SEL_MIN_CHUNK = 4096;            // fewest elements of an automatic slice: 16 per lane
constexpr int MAX_BINS = 1024;
constexpr int MAX_VIEWS = 65535;
constexpr int PPL = 8;                         // pixels per lane of the depth kernels
constexpr int DTILE = DE_T * PPL;              // pixels per workgroup
constexpr int NE = 13;                         // partials of the error kernel: 12 sums and the maximum

using sr::align16;
using sr::bits_finite;
using sr::bits_nan;
using sr::bits_positive_finite;
using sr::QNAN_BITS;

// ------------------------------------------------------------------------------------------ select
struct SelArgs {
  const float* x;
  const uint8_t* mask;
  const int32_t* group;
  int64_t n_rows, row_len, row_stride;
  int n_groups, n_ranks;
  int32_t num[SR_SELECT_MAX_RANKS], den[SR_SELECT_MAX_RANKS];
  float* value;
  uint32_t* count;
  uint32_t* hist;   // [n_groups][n_ranks][256]
  uint32_t* state;  // [n_groups][n_ranks][2]: prefix, remaining rank
  uint32_t* cnt;    // [n_groups][2]: considered (written by the first scan), skipped
  int64_t chunk;    // elements per workgroup, a multiple of 4
  int bpr;          // workgroups per row
  int vec;          // rows and masks allow 16-byte / 4-byte loads
};

struct SelPlan {
  int bpr;
  int64_t chunk;
};

int64_t sel_workspace(int n_groups, int n_ranks) {
  if (n_groups < 1 || n_ranks < 1 || n_ranks > SR_SELECT_MAX_RANKS) return 0;
  return align16(((int64_t)n_groups * n_ranks * (256 + 2) + (int64_t)n_groups * 2) * 4);
}

bool sel_plan(int64_t n_rows, int64_t row_len, int blocks_per_row, SelPlan& p) {
  if (n_rows < 1 || row_len < 1 || blocks_per_row < 0 || blocks_per_row > SEL_MAX_BPR) return false;
  if (row_len > SEL_MAX_TOTAL / n_rows) return false;
  int64_t bpr = blocks_per_row;
  if (bpr == 0) {
    const int64_t most = (row_len + SEL_MIN_CHUNK - 1) / SEL_MIN_CHUNK;
    bpr = (SEL_AUTO_BLOCKS + n_rows - 1) / n_rows;
    if (bpr > most) bpr = most;
    if (bpr > SEL_MAX_BPR) bpr = SEL_MAX_BPR;
  }
  if (n_rows * bpr > 2147483647LL) return false;
  p.bpr = (int)bpr;
  p.chunk = ((row_len + bpr - 1) / bpr + 3) / 4 * 4;
  return true;
}

__global__ __launch_bounds__(DE_T) void select_hist_kernel(SelArgs a, int pass) {
  __shared__ uint32_t s_hist[SR_SELECT_MAX_RANKS * 256];
  __shared__ uint32_t s_skip;
  const int t = threadIdx.x;
  const int64_t row = blockIdx.x / (uint32_t)a.bpr;
  const int part = (int)(blockIdx.x % (uint32_t)a.bpr);
  const int g = a.group ? a.group[row] : (int)row;
  if (g < 0 || g >= a.n_groups) return;  // the whole workgroup: nothing is indexed through a bad group
  const int nr = pass == 0 ? 1 : a.n_ranks;
  for (int e = t; e < nr * 256; e += DE_T) s_hist[e] = 0;
  if (t == 0) s_skip = 0;
  uint32_t prefix[SR_SELECT_MAX_RANKS];
#pragma unroll
  for (int r = 0; r < SR_SELECT_MAX_RANKS; ++r)
    prefix[r] = (pass > 0 && r < nr) ? a.state[((int64_t)g * a.n_ranks + r) * 2] : 0u;
  __syncthreads();
  const int shift = 24 - 8 * pass;
  const int hi = pass > 0 ? shift + 8 : 0;  // pass 0 never shifts by it
  const int64_t begin = (int64_t)part * a.chunk;
  const int64_t end = begin + a.chunk < a.row_len ? begin + a.chunk : a.row_len;
  const float* xr = a.x + row * a.row_stride;
  const uint8_t* mr = a.mask ? a.mask + row * a.row_stride : nullptr;
  int cur[SR_SELECT_MAX_RANKS];
  uint32_t run[SR_SELECT_MAX_RANKS];
#pragma unroll
  for (int r = 0; r < SR_SELECT_MAX_RANKS; ++r) cur[r] = 0, run[r] = 0u;
  uint32_t skipped = 0;
  for (int64_t q = begin + 4 * t; q < end; q += 4 * DE_T) {
    const int n = end - q < 4 ? (int)(end - q) : 4;
    uint32_t b[4] = {0u, 0u, 0u, 0u};
    uint32_t m = 0x01010101u;
    if (a.vec && n == 4) {
      const uint4 v = *reinterpret_cast<const uint4*>(xr + q);
      b[0] = v.x, b[1] = v.y, b[2] = v.z, b[3] = v.w;
      if (mr) m = *reinterpret_cast<const uint32_t*>(mr + q);
    } else {
      if (mr) m = 0u;
#pragma unroll
      for (int u = 0; u < 4; ++u)
        if (u < n) {
          b[u] = __float_as_uint(xr[q + u]);
          if (mr) m |= (uint32_t)mr[q + u] << (8 * u);
        }
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      if (u >= n) continue;
      if (((m >> (8 * u)) & 255u) == 0u || !bits_finite(b[u])) {
        ++skipped;
        continue;
      }
      const uint32_t key = sr::key32(b[u]);
      const int digit = (int)((key >> shift) & 255u);
#pragma unroll
      for (int r = 0; r < SR_SELECT_MAX_RANKS; ++r) {
        if (r >= nr) continue;
        if (pass > 0 && (key >> hi) != prefix[r]) continue;
        if (digit == cur[r]) {
          ++run[r];
        } else {
          if (run[r]) atomicAdd(&s_hist[r * 256 + cur[r]], run[r]);
          cur[r] = digit, run[r] = 1u;
        }
      }
    }
  }
#pragma unroll
  for (int r = 0; r < SR_SELECT_MAX_RANKS; ++r)
    if (r < nr && run[r]) atomicAdd(&s_hist[r * 256 + cur[r]], run[r]);
  if (pass == 0 && skipped) atomicAdd(&s_skip, skipped);
  __syncthreads();
  for (int e = t; e < nr * 256; e += DE_T) {
    const uint32_t v = s_hist[e];
    if (v) atomicAdd(&a.hist[(int64_t)g * a.n_ranks * 256 + e], v);
  }
  if (pass == 0 && t == 0 && s_skip) atomicAdd(&a.cnt[2 * (int64_t)g + 1], s_skip);
}

__global__ __launch_bounds__(DE_T) void select_scan_kernel(SelArgs a, int pass) {
  __shared__ uint32_t s_scan[DE_T];
  const int t = threadIdx.x;
  const int64_t g = blockIdx.x;
  uint32_t* hist = a.hist + g * a.n_ranks * 256;
  for (int r = 0; r < a.n_ranks; ++r) {
    const uint32_t c = hist[(pass == 0 ? 0 : r) * 256 + t];
    uint32_t n;
    const uint32_t excl = sr::block_exclusive<DE_T>(c, s_scan, n), incl = excl + c;
    uint32_t* st = a.state + (g * a.n_ranks + r) * 2;
    uint32_t rem;
    if (pass == 0) {
      int64_t k = ((int64_t)a.num[r] * n + a.den[r] - 1) / a.den[r] - 1;
      rem = (uint32_t)(k < 0 ? 0 : k);
      if (r == 0 && t == 0) a.cnt[2 * g] = n;
    } else {
      rem = st[1];
    }
    __syncthreads();  // every lane has read the remaining rank and the scan
    if (c > 0u && excl <= rem && rem < incl) {  // exactly one lane of a non-empty group
      st[0] = pass == 0 ? (uint32_t)t : ((st[0] << 8) | (uint32_t)t);
      st[1] = rem - excl;
    }
    __syncthreads();
  }
  for (int r = 0; r < a.n_ranks; ++r) hist[r * 256 + t] = 0u;
  if (pass == 3) {
    const uint32_t n = a.cnt[2 * g];
    if (t < a.n_ranks)
      reinterpret_cast<uint32_t*>(a.value)[g * a.n_ranks + t] = n ? sr::unkey32(a.state[(g * a.n_ranks + t) * 2]) : QNAN_BITS;
    if (a.count && t < 2) a.count[2 * g + t] = a.cnt[2 * g + t];
  }
}

// validated arguments -> the clearing node and the eight launches
void select_launch(hipStream_t s, SelArgs a, const SelPlan& p, void* workspace) {
  const int64_t n_hist = (int64_t)a.n_groups * a.n_ranks * 256;
  a.hist = (uint32_t*)workspace;
  a.state = a.hist + n_hist;
  a.cnt = a.state + (int64_t)a.n_groups * a.n_ranks * 2;
  a.bpr = p.bpr, a.chunk = p.chunk;
  a.vec = ((uintptr_t)a.x & 15) == 0 && a.row_stride % 4 == 0 && (!a.mask || ((uintptr_t)a.mask & 3) == 0);
  (void)hipMemsetAsync(workspace, 0, (size_t)sel_workspace(a.n_groups, a.n_ranks), s);
  for (int pass = 0; pass < 4; ++pass) {
    hipLaunchKernelGGL(select_hist_kernel, dim3((unsigned)(a.n_rows * a.bpr)), dim3(DE_T), 0, s, a, pass);
    hipLaunchKernelGGL(select_scan_kernel, dim3((unsigned)a.n_groups), dim3(DE_T), 0, s, a, pass);
  }
}

// ------------------------------------------------------------------------------------------ depth
struct DepArgs {
  sr_depth_eval_desc d;
  uint8_t* valid;  // [n_views][stride]
  double* part1;   // [n_views][wpv][5]: n, sum p, sum g, sum g p, sum p p
  double* part2;   // [n_views][wpv][2]: sum (p - pm)(g - gm), sum (p - pm)^2
  double* part_e;  // [n_views][wpv][NE]
  double* gsum;    // [n_groups][8]: the five sums of part1, pm, gm, 0
  float* med;      // [2][n_groups]: med(gt), med(pred)
  float* rel;      // [n_views][n_pix] r32: d.rel_err or the scratch
  int wpv;         // workgroups per view
};

// the partials [view][workgroup][NV] of group g's views: views ascending, a lane's workgroups ascending,
// then sr::block_reduce's tree
template <int NV, bool LAST_MAX>
__device__ inline void group_reduce(const DepArgs& a, const double* part, int g, double (&acc)[NV], double* smem) {
  const int t = threadIdx.x;
#pragma unroll
  for (int e = 0; e < NV; ++e) acc[e] = 0.0;
  const int v0 = a.d.group ? 0 : g, v1 = a.d.group ? a.d.n_views : g + 1;
  for (int v = v0; v < v1; ++v) {
    if (a.d.group && a.d.group[v] != g) continue;
    for (int w = t; w < a.wpv; w += DE_T) {
      const double* p = part + ((int64_t)v * a.wpv + w) * NV;
#pragma unroll
      for (int e = 0; e < NV; ++e) {
        if (LAST_MAX && e == NV - 1) {
          if (p[e] > acc[e]) acc[e] = p[e];
        } else {
          acc[e] += p[e];
        }
      }
    }
  }
  sr::block_reduce<DE_T, NV, LAST_MAX>(acc, smem);
}

__global__ __launch_bounds__(DE_T) void depth_valid_kernel(DepArgs a) {
  __shared__ double s_red[5 * DE_T];
  const int t = threadIdx.x;
  const int v = blockIdx.x / a.wpv, w = blockIdx.x % a.wpv;
  const sr_depth_eval_desc& d = a.d;
  const int64_t base = (int64_t)v * d.stride;
  const float cmin = d.conf ? d.conf_min[v] : 0.0f;
  double acc[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll 1
  for (int k = 0; k < PPL; ++k) {
    const int64_t i = (int64_t)w * DTILE + k * DE_T + t;
    if (i >= d.n_pix) break;
    const float p = d.pred[base + i], g = d.gt[base + i];
    bool ok = bits_finite(__float_as_uint(p)) && bits_finite(__float_as_uint(g)) && g > d.gt_min && g <= d.gt_max;
    if (d.mask) ok = ok && d.mask[base + i] != 0;
    if (d.conf) {
      const float c = d.conf[base + i];
      ok = ok && !bits_nan(__float_as_uint(c)) && !bits_nan(__float_as_uint(cmin)) && c >= cmin;
    }
    a.valid[base + i] = ok ? 1 : 0;
    if (ok) {
      const double pd = (double)p, gd = (double)g;
      acc[0] += 1.0;
      acc[1] += pd;
      acc[2] += gd;
      acc[3] += __dmul_rn(gd, pd);
      acc[4] += __dmul_rn(pd, pd);
    }
  }
  sr::block_reduce<DE_T>(acc, s_red);
  if (t == 0) {
    double* o = a.part1 + (int64_t)blockIdx.x * 5;
#pragma unroll
    for (int e = 0; e < 5; ++e) o[e] = acc[e];
  }
}

__global__ __launch_bounds__(DE_T) void depth_centred_kernel(DepArgs a) {
  __shared__ double s_red[2 * DE_T];
  const int t = threadIdx.x;
  const int v = blockIdx.x / a.wpv, w = blockIdx.x % a.wpv;
  const sr_depth_eval_desc& d = a.d;
  const int64_t base = (int64_t)v * d.stride;
  const int g = d.group ? d.group[v] : v;
  double acc[2] = {0.0, 0.0};
  if (g >= 0 && g < d.n_groups) {
    const double pm = a.gsum[8 * (int64_t)g + 5], gm = a.gsum[8 * (int64_t)g + 6];
#pragma unroll 1
    for (int k = 0; k < PPL; ++k) {
      const int64_t i = (int64_t)w * DTILE + k * DE_T + t;
      if (i >= d.n_pix) break;
      if (!a.valid[base + i]) continue;
      const double dp = __dsub_rn((double)d.pred[base + i], pm), dg = __dsub_rn((double)d.gt[base + i], gm);
      acc[0] += __dmul_rn(dp, dg);
      acc[1] += __dmul_rn(dp, dp);
    }
  }
  sr::block_reduce<DE_T>(acc, s_red);
  if (t == 0) {
    double* o = a.part2 + (int64_t)blockIdx.x * 2;
    o[0] = acc[0], o[1] = acc[1];
  }
}

// stage 0: the sums of part1 and the means; (s, t) where they need nothing more.  stage 1: (s, t) from
// the medians (MEDIAN) or the centred sums (SCALE_SHIFT).
__global__ __launch_bounds__(DE_T) void depth_fit_kernel(DepArgs a, int stage) {
  __shared__ double s_red[5 * DE_T];
  const int t = threadIdx.x, g = blockIdx.x;
  const sr_depth_eval_desc& d = a.d;
  double* gs = a.gsum + 8 * (int64_t)g;
  const bool two_stage = d.align == SR_DEPTH_ALIGN_MEDIAN || d.align == SR_DEPTH_ALIGN_SCALE_SHIFT;
  double c2[2] = {0.0, 0.0};
  if (stage == 0) {
    double acc[5];
    group_reduce<5, false>(a, a.part1, g, acc, s_red);
    if (t == 0) {
      const bool any = acc[0] > 0.0;
#pragma unroll
      for (int e = 0; e < 5; ++e) gs[e] = acc[e];
      gs[5] = any ? acc[1] / acc[0] : 0.0;
      gs[6] = any ? acc[2] / acc[0] : 0.0;
      gs[7] = 0.0;
    }
    if (two_stage) return;
  } else if (d.align == SR_DEPTH_ALIGN_SCALE_SHIFT) {
    group_reduce<2, false>(a, a.part2, g, c2, s_red);
  }
  if (t != 0) return;
  double s = 1.0, sh = 0.0;
  int status = 0;
  if (!(gs[0] > 0.0)) {
    status = 2;
  } else if (d.align == SR_DEPTH_ALIGN_MEDIAN) {
    const float mg = a.med[g], mp = a.med[d.n_groups + g];
    if (bits_positive_finite(__float_as_uint(mp)))
      s = (double)mg / (double)mp;
    else
      status = 1;
  } else if (d.align == SR_DEPTH_ALIGN_SCALE) {
    if (gs[4] > 0.0)
      s = gs[3] / gs[4];
    else
      status = 1;
  } else if (d.align == SR_DEPTH_ALIGN_SCALE_SHIFT) {
    if (c2[1] > 0.0) {
      s = c2[0] / c2[1];
      sh = __dsub_rn(gs[6], __dmul_rn(s, gs[5]));
    } else {
      status = 1;
      sh = __dsub_rn(gs[6], gs[5]);
    }
  }
  d.status[g] = status;
  if (d.align != SR_DEPTH_ALIGN_GIVEN) d.xform[2 * g] = s, d.xform[2 * g + 1] = sh;
}

__global__ __launch_bounds__(DE_T) void depth_error_kernel(DepArgs a) {
  __shared__ uint32_t s_hist[MAX_BINS + 2];
  __shared__ double s_red[NE * DE_T];
  const int t = threadIdx.x;
  const int v = blockIdx.x / a.wpv, w = blockIdx.x % a.wpv;
  const sr_depth_eval_desc& d = a.d;
  const int64_t base = (int64_t)v * d.stride, obase = (int64_t)v * d.n_pix;
  const int n_slots = d.n_bins + 2;
  int g = d.group ? d.group[v] : v;
  const bool group_ok = g >= 0 && g < d.n_groups;  // a view outside every group scores nothing
  if (!group_ok) g = 0;
  const double s = d.xform[2 * g], sh = d.xform[2 * g + 1];
  sr::hist_clear<DE_T>(s_hist, n_slots);
  __syncthreads();
  // n_valid, n_nonpos, n_invalid, rel, sq / g, sq, d, d^2, |d| / ln 10, delta 1..3, max rel
  double acc[NE];
#pragma unroll
  for (int e = 0; e < NE; ++e) acc[e] = 0.0;
  const double inv_ln10 = 0.43429448190325182765;
#pragma unroll 1
  for (int k = 0; k < PPL; ++k) {
    const int64_t i = (int64_t)w * DTILE + k * DE_T + t;
    if (i >= d.n_pix) break;
    uint32_t a_bits = QNAN_BITS, r_bits = QNAN_BITS;
    if (group_ok && a.valid[base + i]) {
      const float p = d.pred[base + i], gf = d.gt[base + i];
      const float af = (float)__dadd_rn(__dmul_rn(s, (double)p), sh);
      a_bits = __float_as_uint(af);
      const double ad = (double)af, gd = (double)gf;
      const double e = __dsub_rn(ad, gd), sq = __dmul_rn(e, e);
      const double rel = fabs(e) / gd;
      const float r32 = (float)rel;
      r_bits = __float_as_uint(r32);
      acc[0] += 1.0;
      acc[3] += rel;
      acc[4] += sq / gd;
      acc[5] += sq;
      if (bits_finite(r_bits)) {
        if (rel > acc[12]) acc[12] = rel;
        atomicAdd(&s_hist[sr::hist_slot(r32, d.bin_len, d.n_bins)], 1u);
      } else {
        atomicAdd(&s_hist[d.n_bins + 1], 1u);
      }
      if (bits_positive_finite(a_bits)) {
        const double dl = __dsub_rn(log(ad), log(gd));
        acc[6] += dl;
        acc[7] += __dmul_rn(dl, dl);
        acc[8] += __dmul_rn(fabs(dl), inv_ln10);
        if (ad < __dmul_rn(1.25, gd) && gd < __dmul_rn(1.25, ad)) acc[9] += 1.0;
        if (ad < __dmul_rn(1.5625, gd) && gd < __dmul_rn(1.5625, ad)) acc[10] += 1.0;
        if (ad < __dmul_rn(1.953125, gd) && gd < __dmul_rn(1.953125, ad)) acc[11] += 1.0;
      } else {
        acc[1] += 1.0;
      }
    } else {
      acc[2] += 1.0;
    }
    if (d.aligned) reinterpret_cast<uint32_t*>(d.aligned)[obase + i] = a_bits;
    if (a.rel) reinterpret_cast<uint32_t*>(a.rel)[obase + i] = r_bits;
  }
  __syncthreads();
  if (group_ok) sr::hist_flush<DE_T>(s_hist, d.hist + (int64_t)g * n_slots, n_slots);
  sr::block_reduce<DE_T, NE, true>(acc, s_red);
  if (t == 0) {
    double* o = a.part_e + (int64_t)blockIdx.x * NE;
#pragma unroll
    for (int e = 0; e < NE; ++e) o[e] = acc[e];
  }
}

__global__ __launch_bounds__(DE_T) void depth_group_kernel(DepArgs a) {
  __shared__ double s_red[NE * DE_T];
  const int g = blockIdx.x;
  double acc[NE];
  group_reduce<NE, true>(a, a.part_e, g, acc, s_red);
  if (threadIdx.x == 0) {
    double* o = a.d.stats + 16 * (int64_t)g;
#pragma unroll
    for (int e = 0; e < NE; ++e) o[e] = acc[e];
    o[13] = o[14] = o[15] = 0.0;
  }
}

// grid: one workgroup per 256 histogram slots; workgroup 0 also pools the stats
__global__ __launch_bounds__(DE_T) void depth_pool_kernel(DepArgs a) {
  const int t = threadIdx.x, ng = a.d.n_groups, n_slots = a.d.n_bins + 2;
  if (blockIdx.x == 0 && t < 16) {
    double v = 0.0;
    for (int g = 0; g < ng; ++g) {  // ascending groups
      const double o = a.d.stats[16 * (int64_t)g + t];
      if (t == NE - 1) {
        if (o > v) v = o;
      } else {
        v += o;
      }
    }
    a.d.stats[16 * (int64_t)ng + t] = v;
  }
  const int e = blockIdx.x * DE_T + t;
  if (e < n_slots) {
    uint32_t c = 0;
#pragma unroll 8
    for (int g = 0; g < ng; ++g) c += a.d.hist[(int64_t)g * n_slots + e];
    a.d.hist[(int64_t)ng * n_slots + e] = c;
  }
}

struct DepPlan {
  int wpv;
  int64_t off_part1, off_part2, off_part_e, off_gsum, off_med, off_zero, off_sel, off_rel, bytes;
};

bool dep_plan(int n_views, int64_t n_pix, int64_t stride, int n_groups, int rel_q_scratch, DepPlan& p) {
  if (n_views < 1 || n_views > MAX_VIEWS || n_pix < 1 || stride < n_pix) return false;
  if (stride > SEL_MAX_TOTAL / n_views) return false;
  if (n_groups < 1 || n_groups > n_views) return false;
  p.wpv = (int)((n_pix + DTILE - 1) / DTILE);
  const int64_t wgs = (int64_t)n_views * p.wpv;
  int64_t o = align16((int64_t)n_views * stride);
  p.off_part1 = o, o += wgs * 5 * 8;
  p.off_part2 = o, o += wgs * 2 * 8;
  p.off_part_e = o, o += wgs * NE * 8;
  p.off_gsum = o, o += (int64_t)n_groups * 8 * 8;
  p.off_med = o, o = align16(o + (int64_t)n_groups * 2 * 4);
  p.off_zero = o, o = align16(o + (int64_t)n_views * 4);
  p.off_sel = o, o += sel_workspace(n_groups, 2);
  p.off_rel = o;
  if (rel_q_scratch) o = align16(o + (int64_t)n_views * n_pix * 4);
  p.bytes = o;
  return true;
}

}  // namespace

extern "C" int64_t sr_select_workspace(int n_groups, int n_ranks) { return sel_workspace(n_groups, n_ranks); }

extern "C" int sr_select_ranks(sr_stream_t stream, const sr_select_desc* desc) {
  SR_CHECK(desc, SR_EINVAL, "sr_select_ranks: null desc");
  const sr_select_desc& d = *desc;
  SR_CHECK(d.x && d.value && d.workspace, SR_EINVAL, "sr_select_ranks: null x, value or workspace");
  SR_CHECK(d.n_ranks >= 1 && d.n_ranks <= SR_SELECT_MAX_RANKS, SR_EINVAL, "sr_select_ranks: n_ranks %d outside [1, %d]",
           d.n_ranks, SR_SELECT_MAX_RANKS);
  for (int r = 0; r < d.n_ranks; ++r)
    SR_CHECK(d.rank_den[r] >= 1 && d.rank_den[r] <= SEL_MAX_DEN && d.rank_num[r] >= 0 && d.rank_num[r] <= d.rank_den[r],
             SR_EINVAL, "sr_select_ranks: rank %d is %d / %d, need 0 <= num <= den <= 2^20", r, d.rank_num[r], d.rank_den[r]);
  SR_CHECK(d.n_rows >= 1 && d.row_len >= 1, SR_EINVAL, "sr_select_ranks: n_rows %lld / row_len %lld below 1",
           (long long)d.n_rows, (long long)d.row_len);
  SR_CHECK(d.row_stride >= d.row_len, SR_EINVAL, "sr_select_ranks: row_stride %lld below row_len %lld",
           (long long)d.row_stride, (long long)d.row_len);
  SR_CHECK(d.row_len <= SEL_MAX_TOTAL / d.n_rows, SR_EINVAL, "sr_select_ranks: %lld x %lld elements, more than 2^31",
           (long long)d.n_rows, (long long)d.row_len);
  SR_CHECK(d.n_groups >= 1 && d.n_groups <= d.n_rows, SR_EINVAL, "sr_select_ranks: n_groups %d outside [1, %lld]",
           d.n_groups, (long long)d.n_rows);
  SR_CHECK(d.group || d.n_groups == d.n_rows, SR_EINVAL, "sr_select_ranks: without group, n_groups must be n_rows");
  SelPlan p;
  SR_CHECK(sel_plan(d.n_rows, d.row_len, d.blocks_per_row, p), SR_EINVAL,
           "sr_select_ranks: blocks_per_row %d outside [0, %d], or more than 2^31 - 1 workgroups", d.blocks_per_row,
           SEL_MAX_BPR);
  const int64_t need = sel_workspace(d.n_groups, d.n_ranks);
  SR_CHECK_WORKSPACE("sr_select_ranks", d.workspace, d.workspace_bytes, need);
  SelArgs a{};
  a.x = d.x, a.mask = d.mask, a.group = d.group;
  a.n_rows = d.n_rows, a.row_len = d.row_len, a.row_stride = d.row_stride;
  a.n_groups = d.n_groups, a.n_ranks = d.n_ranks;
  for (int r = 0; r < d.n_ranks; ++r) a.num[r] = d.rank_num[r], a.den[r] = d.rank_den[r];
  a.value = d.value, a.count = d.count;
  select_launch((hipStream_t)stream, a, p, d.workspace);
  sr::note_kernel("select_hist_kernel");
  return sr::check_launch("sr_select_ranks");
}

extern "C" int64_t sr_depth_eval_workspace(int n_views, int64_t n_pix, int64_t stride, int n_groups, int rel_q_scratch) {
  DepPlan p;
  return dep_plan(n_views, n_pix, stride, n_groups, rel_q_scratch, p) ? p.bytes : 0;
}

extern "C" int sr_depth_eval(sr_stream_t stream, const sr_depth_eval_desc* desc) {
  SR_CHECK(desc, SR_EINVAL, "sr_depth_eval: null desc");
  DepArgs a{};
  a.d = *desc;
  const sr_depth_eval_desc& d = a.d;
  SR_CHECK(d.pred && d.gt && d.xform && d.status && d.stats && d.hist && d.workspace, SR_EINVAL,
           "sr_depth_eval: null pred, gt, xform, status, stats, hist or workspace");
  SR_CHECK(d.n_views >= 1 && d.n_views <= MAX_VIEWS, SR_EINVAL, "sr_depth_eval: n_views %d outside [1, %d]", d.n_views,
           MAX_VIEWS);
  SR_CHECK(d.n_pix >= 1 && d.stride >= d.n_pix, SR_EINVAL, "sr_depth_eval: n_pix %lld below 1 or above the stride %lld",
           (long long)d.n_pix, (long long)d.stride);
  SR_CHECK(d.stride <= SEL_MAX_TOTAL / d.n_views, SR_EINVAL, "sr_depth_eval: %d x %lld floats, more than 2^31", d.n_views,
           (long long)d.stride);
  SR_CHECK(d.n_groups >= 1 && d.n_groups <= d.n_views, SR_EINVAL, "sr_depth_eval: n_groups %d outside [1, %d]", d.n_groups,
           d.n_views);
  SR_CHECK(d.group || d.n_groups == d.n_views, SR_EINVAL, "sr_depth_eval: without group, n_groups must be n_views");
  SR_CHECK((d.conf != nullptr) == (d.conf_min != nullptr), SR_EINVAL, "sr_depth_eval: conf and conf_min go together");
  SR_CHECK(!sr::is_nan(d.gt_min) && !sr::is_nan(d.gt_max) && d.gt_min < d.gt_max, SR_EINVAL,
           "sr_depth_eval: need gt_min < gt_max, neither a NaN");
  SR_CHECK(d.align >= SR_DEPTH_ALIGN_NONE && d.align <= SR_DEPTH_ALIGN_GIVEN, SR_EINVAL, "sr_depth_eval: unknown align %d",
           d.align);
  SR_CHECK(d.n_bins > 0 && d.n_bins <= MAX_BINS, SR_EINVAL, "sr_depth_eval: n_bins %d outside [1, %d]", d.n_bins, MAX_BINS);
  SR_CHECK(sr::positive_finite(d.bin_len), SR_EINVAL, "sr_depth_eval: bin_len must be positive and finite");
  DepPlan p;
  const int scratch = d.rel_q && !d.rel_err;
  SR_CHECK(dep_plan(d.n_views, d.n_pix, d.stride, d.n_groups, scratch, p), SR_EINVAL, "sr_depth_eval: no plan");
  SR_CHECK_WORKSPACE("sr_depth_eval", d.workspace, d.workspace_bytes, p.bytes);
  SR_CHECK(((uintptr_t)d.xform & 7) == 0 && ((uintptr_t)d.stats & 7) == 0, SR_EINVAL,
           "sr_depth_eval: fp64 buffers must be 8-byte aligned");
  char* ws = (char*)d.workspace;
  a.valid = (uint8_t*)ws;
  a.part1 = (double*)(ws + p.off_part1);
  a.part2 = (double*)(ws + p.off_part2);
  a.part_e = (double*)(ws + p.off_part_e);
  a.gsum = (double*)(ws + p.off_gsum);
  a.med = (float*)(ws + p.off_med);
  int32_t* zero_group = (int32_t*)(ws + p.off_zero);
  void* sel_ws = ws + p.off_sel;
  a.rel = d.rel_err ? d.rel_err : (scratch ? (float*)(ws + p.off_rel) : nullptr);
  a.wpv = p.wpv;
  hipStream_t s = (hipStream_t)stream;
  const dim3 pix_grid((unsigned)((int64_t)d.n_views * p.wpv)), grp_grid((unsigned)d.n_groups), block(DE_T);
  (void)hipMemsetAsync(d.hist, 0, (size_t)(d.n_groups + 1) * (d.n_bins + 2) * sizeof(uint32_t), s);
  hipLaunchKernelGGL(depth_valid_kernel, pix_grid, block, 0, s, a);
  hipLaunchKernelGGL(depth_fit_kernel, grp_grid, block, 0, s, a, 0);
  SelArgs sa{};
  sa.group = d.group;
  sa.n_rows = d.n_views, sa.n_groups = d.n_groups;
  if (d.align == SR_DEPTH_ALIGN_MEDIAN) {
    sa.mask = a.valid, sa.row_len = d.n_pix, sa.row_stride = d.stride, sa.n_ranks = 1;
    sa.num[0] = 1, sa.den[0] = 2;
    SelPlan sp;
    sel_plan(sa.n_rows, sa.row_len, 0, sp);
    sa.x = d.gt, sa.value = a.med;
    select_launch(s, sa, sp, sel_ws);
    sa.x = d.pred, sa.value = a.med + d.n_groups;
    select_launch(s, sa, sp, sel_ws);
    hipLaunchKernelGGL(depth_fit_kernel, grp_grid, block, 0, s, a, 1);
  } else if (d.align == SR_DEPTH_ALIGN_SCALE_SHIFT) {
    hipLaunchKernelGGL(depth_centred_kernel, pix_grid, block, 0, s, a);
    hipLaunchKernelGGL(depth_fit_kernel, grp_grid, block, 0, s, a, 1);
  }
  hipLaunchKernelGGL(depth_error_kernel, pix_grid, block, 0, s, a);
  hipLaunchKernelGGL(depth_group_kernel, grp_grid, block, 0, s, a);
  hipLaunchKernelGGL(depth_pool_kernel, dim3((unsigned)((d.n_bins + 2 + DE_T - 1) / DE_T)), block, 0, s, a);
  if (d.rel_q) {
    sa.x = a.rel, sa.mask = nullptr, sa.row_len = d.n_pix, sa.row_stride = d.n_pix, sa.n_ranks = 2;
    sa.num[0] = 1, sa.den[0] = 2, sa.num[1] = 9, sa.den[1] = 10;
    SelPlan sp;
    sel_plan(sa.n_rows, sa.row_len, 0, sp);
    sa.value = d.rel_q;
    select_launch(s, sa, sp, sel_ws);
    (void)hipMemsetAsync(zero_group, 0, (size_t)d.n_views * sizeof(int32_t), s);
    sa.group = zero_group, sa.n_groups = 1, sa.value = d.rel_q + 2 * (int64_t)d.n_groups;
    select_launch(s, sa, sp, sel_ws);
  }
  sr::note_kernel("depth_error_kernel");
  return sr::check_launch("sr_depth_eval");
}
