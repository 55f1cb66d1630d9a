// Sparsification curves on gfx950: per group of rows, the fp64 sums of a per-element error over the K bins
// of two orders of the group's elements, the order of a confidence and the oracle order of the error itself.
// AUSE, AURG and the curves are read off these sums on the host (utils/conf_eval.py).
//
// Contract (DESIGN.md "Scoring confidence maps", include/sfm_amd.h).  Everything that decides a membership is
// a test on the bits or an integer; the sums are IEEE fp64 additions in a fixed order.
//   considered  an element of [0, row_len) of a row whose group lies in [0, n_groups), whose mask byte is
//               non-zero and whose err and conf both have exponent bits that are not all ones
//   key32(x)    bits ^ (sign ? 0xffffffff : 0x80000000): sr_select_ranks' order, -0 before +0
//   order C     (group << 32) | key32(conf), the low word complemented under SR_SPARSIFY_UNCERTAINTY
//   order O     (group << 32) | ~key32(err)
//   sentinel    group n_groups for whatever is not considered: it sorts behind every group
//   bins        b_k = k n / K in 64-bit integers; bin k of a group is [start + b_k, start + b_{k+1}) of the
//               sorted order, start = the considered counts of the groups below
//
//   sparsify_key_kernel     err, conf and mask once, 2048 elements per workgroup: both keys, the err bits as
//                           order C's value, and the considered / skipped counts by group (ballots, then one
//                           integer atomic per workgroup and counter for the group of the workgroup's first
//                           element; behind a row boundary, one per wave, round, group and counter)
//   sr::sort_launch         twice, on 32 + bit_length(n_groups) bits.  Order C carries the err bits as its
//                           value; order O's err is read back from the low word of its sorted key.  Both
//                           reductions stream contiguous memory.
//   sparsify_scan_kernel    one workgroup: the exclusive scans (sr::scan_row) of the considered counts (group
//                           starts) and of K split_g (the first reduction workgroup of every group)
//   sparsify_reduce_kernel  workgroup w of order c finds its group by bisection of the second scan, then its
//                           bin and its chunk of 4096 positions: a lane's elements ascending (stride 256),
//                           sr::block_reduce's fixed tree, one partial.  split_g = max(1, ceil(ceil(n / K) / 4096))
//                           chunks per bin, the same for every bin of a group, so a long bin is spread over many
//                           workgroups and the grid is known on the host: at most N / 4096 + 2 G K.
//   sparsify_finish_kernel  one wave per (group, bin): the partials of the bin, a lane's ascending (stride
//                           64), then a fixed shuffle tree; cut from the sorted key of order C; the counts.
//
// The Makefile builds this file with -ffp-contract=off -fhonor-nans: under -fno-honor-nans the compiler reads
// the test on the exponent bits as a float classification and reduces it to |x| == Inf, which a NaN fails.
#include "sr_common.h"
#include "sr_eval.h"

namespace {

constexpr int SP_T = 256;                   // threads of every workgroup here
constexpr int SP_KEY_PER = 8;               // elements per lane of the key kernel
constexpr int SP_KEY_TILE = SP_T * SP_KEY_PER;  // 2048
constexpr int SP_CHUNK = 4096;              // sorted positions per reduction workgroup: 16 per lane
constexpr int64_t SP_MAX_N = 2147483647LL;
constexpr int SP_MAX_GROUPS = 65535;
constexpr int SP_MAX_STEPS = 1024;

using sr::align16;
using sr::bits_nonfinite;
using sr::key32;
using sr::unkey32;

struct SpPlan {
  int64_t n;        // n_rows * row_len
  int64_t wgs;      // reduction workgroups per order, an upper bound
  int key_bits;
  int64_t off_keyc, off_keyo, off_err, off_skeyc, off_sval, off_gcnt, off_gstart, off_wstart, off_part, off_sort, bytes;
};

bool sp_plan(int64_t n_rows, int64_t row_len, int n_groups, int n_steps, SpPlan& p) {
  if (n_rows < 1 || row_len < 1 || n_rows > SP_MAX_N || row_len > SP_MAX_N / n_rows) return false;
  if (n_groups < 1 || n_groups > SP_MAX_GROUPS || n_groups > n_rows) return false;
  if (n_steps < 1 || n_steps > SP_MAX_STEPS) return false;
  const int64_t n = n_rows * row_len;
  p.n = n;
  p.wgs = n / SP_CHUNK + 2 * (int64_t)n_groups * n_steps + 1;
  p.key_bits = 32;
  for (int g = n_groups; g; g >>= 1) ++p.key_bits;
  int64_t o = 0;
  p.off_keyc = o, o = align16(o + 8 * n);    // order C keys; later order O's sorted keys
  p.off_keyo = o, o = align16(o + 8 * n);    // order O keys
  p.off_err = o, o = align16(o + 4 * n);     // err bits in flat order; later order O's unused sorted values
  p.off_skeyc = o, o = align16(o + 8 * n);   // order C's sorted keys
  p.off_sval = o, o = align16(o + 4 * n);    // order C's sorted values: err bits
  p.off_gcnt = o, o = align16(o + 8 * (int64_t)n_groups);
  p.off_gstart = o, o = align16(o + 4 * (int64_t)n_groups);
  p.off_wstart = o, o = align16(o + 4 * ((int64_t)n_groups + 1));
  p.off_part = o, o = align16(o + 2 * 8 * p.wgs);
  p.off_sort = o, o += sr::sort_workspace(n);
  p.bytes = o;
  return true;
}

struct SpArgs {
  sr_sparsify_desc d;
  uint64_t* keyc;     // [n] order C keys in flat order; after the first sort, order O's sorted keys
  uint64_t* keyo;     // [n] order O keys in flat order
  uint32_t* errbits;  // [n] err bits in flat order
  uint64_t* skeyc;    // [n] order C sorted keys
  uint32_t* sval;     // [n] err bits in order C
  uint32_t* gcnt;     // [n_groups][2] considered, skipped
  uint32_t* gstart;   // [n_groups] sorted position of the group's first element
  uint32_t* wstart;   // [n_groups + 1] first reduction workgroup of the group; the total
  double* part;       // [2][wgs]
  int64_t n, wgs;
};

// reduction workgroups per bin of a group with n considered elements
__device__ inline uint32_t split_of(uint32_t n, int K) {
  const uint32_t longest = (uint32_t)(((uint64_t)n + K - 1) / K);
  const uint32_t s = (longest + SP_CHUNK - 1) / SP_CHUNK;
  return s ? s : 1u;
}

__global__ __launch_bounds__(SP_T) void sparsify_key_kernel(SpArgs a) {
  __shared__ uint32_t s_cnt[2];
  const sr_sparsify_desc& d = a.d;
  const int t = threadIdx.x;
  if (t < 2) s_cnt[t] = 0;
  __syncthreads();
  // flat indices fit 32 bits (n <= 2^31 - 1): the row of an element is a 32-bit division
  const uint32_t n = (uint32_t)a.n, row_len = (uint32_t)d.row_len;
  const int64_t i0 = (int64_t)blockIdx.x * SP_KEY_TILE;
  const uint32_t r0 = (uint32_t)i0 / row_len;
  const int64_t g0 = d.group ? (int64_t)d.group[r0] : (int64_t)r0;  // i0 < n: r0 is a row
  uint32_t mine_c = 0, mine_s = 0;  // in lane 0 of a wave: its elements of group g0
#pragma unroll
  for (int u = 0; u < SP_KEY_PER; ++u) {
    const int64_t i64 = i0 + u * SP_T + t;  // round u, lane t: every load and store is contiguous
    bool of_g0_c = false, of_g0_s = false, other = false, other_c = false;  // other: in range, not of g0
    int other_g = 0;
    if (i64 < (int64_t)n) {
      const uint32_t i = (uint32_t)i64, r = i / row_len, c = i - r * row_len;
      const int64_t g = d.group ? (int64_t)d.group[r] : (int64_t)r;
      const bool in_range = g >= 0 && g < d.n_groups;
      const int64_t e = (int64_t)r * d.row_stride + c;
      const uint32_t eb = __float_as_uint(d.err[e]), cb = __float_as_uint(d.conf[e]);
      const bool considered = in_range && !(d.mask && d.mask[e] == 0) && !bits_nonfinite(eb) && !bits_nonfinite(cb);
      uint64_t kc = (uint64_t)d.n_groups << 32, ko = kc;
      if (considered) {
        const uint32_t k = key32(cb);
        kc = ((uint64_t)g << 32) | (d.order == SR_SPARSIFY_UNCERTAINTY ? ~k : k);
        ko = ((uint64_t)g << 32) | (uint32_t)~key32(eb);
      }
      a.keyc[i] = kc, a.keyo[i] = ko, a.errbits[i] = eb;
      if (in_range) {
        if (g == g0) of_g0_c = considered, of_g0_s = !considered;
        else other = true, other_c = considered, other_g = (int)g;
      }
    }
    mine_c += (uint32_t)__popcll(__ballot(of_g0_c)), mine_s += (uint32_t)__popcll(__ballot(of_g0_s));
    // the lanes behind a row boundary: one pair of atomics per wave and group, from the lowest lane of the group
    // (a lane-by-lane add of 1 to one address set this kernel's time at 32 x 518^2 by view: 261 us against 54)
    for (uint64_t pend = __ballot(other); pend;) {
      const int leader = __ffsll((unsigned long long)pend) - 1;
      const int lg = __shfl(other_g, leader, 64);
      const bool same = other && other_g == lg;
      const uint64_t m = __ballot(same), mc = __ballot(same && other_c);
      if ((t & 63) == leader) {
        if (mc) atomicAdd(&a.gcnt[2 * lg], (uint32_t)__popcll(mc));
        if (m & ~mc) atomicAdd(&a.gcnt[2 * lg + 1], (uint32_t)__popcll(m & ~mc));
      }
      pend &= ~m;
    }
  }
  if ((t & 63) == 0) {
    if (mine_c) atomicAdd(&s_cnt[0], mine_c);
    if (mine_s) atomicAdd(&s_cnt[1], mine_s);
  }
  __syncthreads();
  if (t < 2 && s_cnt[t]) atomicAdd(&a.gcnt[2 * g0 + t], s_cnt[t]);  // s_cnt != 0: g0 is in range
}

__global__ __launch_bounds__(SP_T) void sparsify_scan_kernel(SpArgs a) {
  __shared__ uint32_t s_scan[SP_T];
  const int G = a.d.n_groups, K = a.d.n_steps;
  sr::scan_row<SP_T>(G, 0u, s_scan, [&](int g) { return a.gcnt[2 * g]; }, [&](int g, uint32_t x) { a.gstart[g] = x; });
  const uint32_t wgs = sr::scan_row<SP_T>(G, 0u, s_scan, [&](int g) { return (uint32_t)K * split_of(a.gcnt[2 * g], K); },
                                          [&](int g, uint32_t x) { a.wstart[g] = x; });
  if (threadIdx.x == 0) a.wstart[G] = wgs;
}

// grid (wgs, 2): workgroup w of order c sums one chunk of one bin
__global__ __launch_bounds__(SP_T) void sparsify_reduce_kernel(SpArgs a) {
  __shared__ double s_sum[SP_T];
  const int t = threadIdx.x, G = a.d.n_groups, K = a.d.n_steps, order = blockIdx.y;
  const uint32_t w = blockIdx.x;
  if (w >= a.wstart[G]) return;
  int lo = 0, hi = G;  // the last group whose first workgroup is at or before w: wstart ascends strictly
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (a.wstart[mid] <= w) lo = mid; else hi = mid;
  }
  const int g = lo;
  const uint32_t n = a.gcnt[2 * g], split = split_of(n, K), local = w - a.wstart[g];
  const uint32_t k = local / split, s = local - k * split;
  const int64_t b0 = (int64_t)k * n / K, b1 = (int64_t)(k + 1) * n / K;
  const int64_t p0 = (int64_t)a.gstart[g] + b0 + (int64_t)s * SP_CHUNK;
  int64_t p1 = (int64_t)a.gstart[g] + b1;
  if (p1 > p0 + SP_CHUNK) p1 = p0 + SP_CHUNK;
  if (p1 > a.n) p1 = a.n;  // always: start + n <= the element count
  double sum[1] = {0.0};
  for (int64_t p = p0 + t; p < p1; p += SP_T) {
    const uint32_t eb = order == 0 ? a.sval[p] : unkey32(~(uint32_t)a.keyc[p]);
    sum[0] += (double)__uint_as_float(eb);
  }
  sr::block_reduce<SP_T>(sum, s_sum);
  if (t == 0) a.part[(int64_t)order * a.wgs + w] = sum[0];
}

// one wave per (group, bin)
__global__ __launch_bounds__(SP_T) void sparsify_finish_kernel(SpArgs a) {
  const sr_sparsify_desc& d = a.d;
  const int t = threadIdx.x, lane = t & 63, K = d.n_steps;
  const int64_t item = (int64_t)blockIdx.x * (SP_T / 64) + (t >> 6);
  if (item >= (int64_t)d.n_groups * K) return;
  const int g = (int)(item / K), k = (int)(item - (int64_t)g * K);
  const uint32_t n = a.gcnt[2 * g], split = split_of(n, K);
  const int64_t w0 = (int64_t)a.wstart[g] + (int64_t)k * split;
#pragma unroll
  for (int c = 0; c < 2; ++c) {
    const double* part = a.part + (int64_t)c * a.wgs + w0;
    double sum = 0.0;
    for (uint32_t s = lane; s < split; s += 64) sum += part[s];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) sum += __shfl_down(sum, off, 64);
    if (lane == 0) d.bin_sum[((int64_t)g * 2 + c) * K + k] = sum;
  }
  if (lane != 0) return;
  if (d.cut) {
    uint32_t bits = sr::QNAN_BITS;
    const int64_t p = (int64_t)a.gstart[g] + (int64_t)k * n / K;
    if (n > 0 && p < a.n) {
      const uint32_t low = (uint32_t)a.skeyc[p];
      bits = unkey32(d.order == SR_SPARSIFY_UNCERTAINTY ? ~low : low);
    }
    reinterpret_cast<uint32_t*>(d.cut)[(int64_t)g * K + k] = bits;  // as bits: a float move may not keep them
  }
  if (d.count && k == 0) d.count[2 * g] = n, d.count[2 * g + 1] = a.gcnt[2 * g + 1];
}

}  // namespace

extern "C" int64_t sr_sparsify_workspace(int64_t n_rows, int64_t row_len, int n_groups, int n_steps) {
  SpPlan p;
  return sp_plan(n_rows, row_len, n_groups, n_steps, p) ? p.bytes : 0;
}

extern "C" int sr_sparsify(sr_stream_t stream, const sr_sparsify_desc* desc) {
  SR_CHECK(desc, SR_EINVAL, "sr_sparsify: null desc");
  SpArgs a{};
  a.d = *desc;
  const sr_sparsify_desc& d = a.d;
  SR_CHECK(d.err && d.conf && d.bin_sum && d.workspace, SR_EINVAL, "sr_sparsify: null err, conf, bin_sum or workspace");
  SR_CHECK(d.n_rows >= 1 && d.row_len >= 1, SR_EINVAL, "sr_sparsify: n_rows %lld and row_len %lld must be positive",
           (long long)d.n_rows, (long long)d.row_len);
  SR_CHECK(d.row_stride >= d.row_len, SR_EINVAL, "sr_sparsify: row_stride %lld below row_len %lld", (long long)d.row_stride,
           (long long)d.row_len);
  SR_CHECK(d.n_rows <= SP_MAX_N && d.row_len <= SP_MAX_N / d.n_rows, SR_EINVAL,
           "sr_sparsify: %lld rows of %lld elements exceed 2^31 - 1", (long long)d.n_rows, (long long)d.row_len);
  SR_CHECK(d.n_groups >= 1 && d.n_groups <= SP_MAX_GROUPS && d.n_groups <= d.n_rows, SR_EINVAL,
           "sr_sparsify: n_groups %d outside [1, min(n_rows, %d)]", d.n_groups, SP_MAX_GROUPS);
  SR_CHECK(d.group || d.n_groups == d.n_rows, SR_EINVAL, "sr_sparsify: without group, n_groups must equal n_rows");
  SR_CHECK(d.n_steps >= 1 && d.n_steps <= SP_MAX_STEPS, SR_EINVAL, "sr_sparsify: n_steps %d outside [1, %d]", d.n_steps,
           SP_MAX_STEPS);
  SR_CHECK(d.order == SR_SPARSIFY_CONFIDENCE || d.order == SR_SPARSIFY_UNCERTAINTY, SR_EINVAL,
           "sr_sparsify: unknown order %d", d.order);
  SpPlan p;
  sp_plan(d.n_rows, d.row_len, d.n_groups, d.n_steps, p);
  SR_CHECK_WORKSPACE("sr_sparsify", d.workspace, d.workspace_bytes, p.bytes);
  SR_CHECK(((uintptr_t)d.bin_sum & 7) == 0, SR_EINVAL, "sr_sparsify: bin_sum must be 8-byte aligned");
  char* ws = (char*)d.workspace;
  a.keyc = (uint64_t*)(ws + p.off_keyc);
  a.keyo = (uint64_t*)(ws + p.off_keyo);
  a.errbits = (uint32_t*)(ws + p.off_err);
  a.skeyc = (uint64_t*)(ws + p.off_skeyc);
  a.sval = (uint32_t*)(ws + p.off_sval);
  a.gcnt = (uint32_t*)(ws + p.off_gcnt);
  a.gstart = (uint32_t*)(ws + p.off_gstart);
  a.wstart = (uint32_t*)(ws + p.off_wstart);
  a.part = (double*)(ws + p.off_part);
  a.n = p.n, a.wgs = p.wgs;
  hipStream_t s = (hipStream_t)stream;
  const dim3 block(SP_T);
  (void)hipMemsetAsync(a.gcnt, 0, 8 * (size_t)d.n_groups, s);
  hipLaunchKernelGGL(sparsify_key_kernel, dim3((unsigned)((p.n + SP_KEY_TILE - 1) / SP_KEY_TILE)), block, 0, s, a);
  // order C: the err bits ride along.  Order O: its sorted keys land where order C's keys were, which the first
  // sort has finished reading; its values (the permutation) are not used and land on the err bits, likewise.
  sr::sort_launch(s, a.keyc, a.errbits, a.skeyc, a.sval, p.n, p.key_bits, ws + p.off_sort);
  sr::sort_launch(s, a.keyo, nullptr, a.keyc, a.errbits, p.n, p.key_bits, ws + p.off_sort);
  hipLaunchKernelGGL(sparsify_scan_kernel, dim3(1), block, 0, s, a);
  hipLaunchKernelGGL(sparsify_reduce_kernel, dim3((unsigned)p.wgs, 2), block, 0, s, a);
  const int64_t items = (int64_t)d.n_groups * d.n_steps;
  hipLaunchKernelGGL(sparsify_finish_kernel, dim3((unsigned)((items + SP_T / 64 - 1) / (SP_T / 64))), block, 0, s, a);
  sr::note_kernel("sparsify_finish_kernel");
  return sr::check_launch("sr_sparsify");
}
