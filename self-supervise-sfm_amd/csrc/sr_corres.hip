// Training correspondences and depths on gfx950: sample_correspondence_and_depth
// (train/utils/io.py:280-360), called once per ordered pair by IMC2021._create_downsampled_arrays
// (train/datasets/imc2021.py:317-390), for every pair of a scene in one launch sequence.
//
// Contract (per pair: coords_src / coords_dst [M][2] fp32 in [-1, 1], certainty [M] fp32, depth maps
// [H1][W1] / [H2][W2] fp32, K uniforms u in [0, 1) fp64, min_conf):
//   1. weight   w_i = certainty_i > (float)min_conf ? certainty_i : 0   (strict, fp32, like numpy's
//               comparison of an fp32 array with a Python float).  No compaction: a zero-weight entry
//               has a zero-width CDF step and is never selected.
//   2. scan     cdf = inclusive prefix sum of w in fp64, T = cdf[M - 1]: chunks of CHUNK entries, each
//               lane a serial run of RUN, a wave64 shuffle scan, an LDS step across the waves, one wave
//               over the chunk totals -- a fixed partition and order, so bit-stable from run to run.
//               The CDF is written once (chunk-local); a lookup adds the chunk's exclusive prefix.
//   3. sample   idx = first i with cdf[i] > u * T (binary search: chunk ends, then inside the chunk);
//               if rounding puts u * T >= T, the last positive-weight index.  Never idx >= M.
//   4. outputs  idx in the unfiltered numbering; coords[idx] rescaled (c + 1) * (w - 1) / 2 (x) and
//               (c + 1) * (h - 1) / 2 (y) with the pair's own depth-map sizes, fp32 and bit-equal to
//               numpy (explicit unfused operations: device code compiles with fp contraction on);
//               depth by grid_sample(bilinear, zeros, align_corners=False): x = ((gx + 1) W - 1) / 2 in
//               fp32, four taps, taps outside the map contribute 0.  Tap indices are clamped before any
//               load: a non-finite coordinate reads nothing outside the map (its value is unspecified).
//   5. T == 0   (no eligible correspondence): zeros for that pair; total[p] and n_valid[p] report it and
//               the Python layer raises the reference's ValueError (io.py:319-322).
// Where this differs from numpy's choice(p = fl32(c / S)): S cancels in cdf / cdf[-1] and each p_i keeps
// a relative error <= 2^-24, so an edge of numpy's CDF and the exact-weight edge differ by < 2^-22 (CDF
// units); every uniform at least that far from every edge gives the reference's index.
//
// Second input form (SR_CORRES_PNG16): the matcher's stored uint16 maps x / y / conf [hs][ws], decoded
// like IMC2021._png2coords (v / 65535 * 2 - 1) and _png2certainty (v / 1000) in fp32, coords_src the
// implicit np.linspace(-1 + 1/ws, 1 - 1/ws, ws) x linspace(..hs..) grid (imc2021.py:126-131) computed in
// fp64 as numpy does (i * step + start unfused, last element = stop) and rounded to fp32: 6 bytes per
// correspondence instead of 20, bit-identical to the fp32 form fed the decoded arrays.
//
//   corres_scan_kernel     one workgroup per chunk of a pair: weights -> chunk-local fp64 CDF, chunk
//                          total, eligible count, last positive-weight index
//   corres_chunks_kernel   one wave per pair: exclusive scan of the chunk totals, T, n_valid
//   corres_sample_kernel   one lane per (pair, k): search, gather, rescale, two bilinear depth reads
// Plain vector loads and stores only; bandwidth- and latency-bound.
#include "sr_common.h"

namespace {

constexpr int SCAN_T = 256;            // threads of a scan workgroup
constexpr int RUN = 8;                 // serial entries per lane
constexpr int CHUNK = SCAN_T * RUN;    // entries per workgroup
constexpr int SAMPLE_T = 256;

__host__ __device__ inline int n_chunks(int m) { return (m + CHUNK - 1) / CHUNK; }

// workspace of one pair (doubles): cdf [max_m] | cexcl [maxc] | cend [maxc] | {count, last} int32 [maxc][2]
// | {last positive index, pad} int32 [2]
__host__ __device__ inline int64_t pair_stride(int max_m) { return (int64_t)max_m + 3ll * n_chunks(max_m) + 1; }

struct PairWs {
  double* cdf;
  double* cexcl;
  double* cend;
  int32_t* cinfo;
  int32_t* last;
};

__device__ inline PairWs carve(double* ws, int p, int max_m) {
  const int maxc = n_chunks(max_m);
  PairWs w;
  w.cdf = ws + (int64_t)p * pair_stride(max_m);
  w.cexcl = w.cdf + max_m;
  w.cend = w.cexcl + maxc;
  w.cinfo = (int32_t*)(w.cend + maxc);
  w.last = w.cinfo + 2 * maxc;
  return w;
}

// entries of a pair; 0 for a record this launch cannot hold (reported as n_valid = -1)
__device__ inline int pair_m(const sr_corres_pair& r, int max_m) {
  int64_t m;
  if (r.format == SR_CORRES_PNG16)
    m = (r.hs > 0 && r.ws > 0) ? (int64_t)r.hs * r.ws : 0;
  else
    m = r.format == SR_CORRES_F32 ? r.m : 0;
  const bool maps = r.h1 > 0 && r.w1 > 0 && r.h2 > 0 && r.w2 > 0 && r.conf && r.dst && r.depth_src && r.depth_dst &&
                    (r.format == SR_CORRES_PNG16 ? r.dst_y != nullptr : r.src != nullptr);
  return (m > 0 && m <= max_m && maps) ? (int)m : 0;
}

__device__ inline float certainty_at(const sr_corres_pair& r, int i) {
  if (r.format == SR_CORRES_PNG16)  // _png2certainty: astype(float32) / 1000
    return __fdiv_rn((float)((const uint16_t*)r.conf)[i], 1000.0f);
  return ((const float*)r.conf)[i];
}

// np.linspace(-1 + 1/n, 1 - 1/n, n)[i] in fp64 as numpy computes it, then .astype(float32)
__device__ inline float linspace_at(int i, int n) {
  const double inv = __ddiv_rn(1.0, (double)n);
  const double start = __dadd_rn(-1.0, inv), stop = __dsub_rn(1.0, inv);
  if (n == 1) return (float)start;
  if (i == n - 1) return (float)stop;
  const double step = __ddiv_rn(__dsub_rn(stop, start), (double)(n - 1));
  return (float)__dadd_rn(__dmul_rn((double)i, step), start);
}

__device__ inline float png_coord(const void* map, int i) {  // _png2coords: astype(float32) / 65535.0 * 2 - 1
  const float v = (float)((const uint16_t*)map)[i];
  return __fsub_rn(__fmul_rn(__fdiv_rn(v, 65535.0f), 2.0f), 1.0f);
}

// torchncoords2coordinates (io.py:262-277): (c + 1) * (size - 1) / 2, fp32 like numpy
__device__ inline float to_pixel(float c, int size) {
  return __fdiv_rn(__fmul_rn(__fadd_rn(c, 1.0f), (float)(size - 1)), 2.0f);
}

// F.grid_sample(bilinear, padding_mode='zeros', align_corners=False) of one point
__device__ inline float bilinear_zeros(const float* map, int h, int w, float gx, float gy) {
  const float x = ((gx + 1.0f) * (float)w - 1.0f) / 2.0f, y = ((gy + 1.0f) * (float)h - 1.0f) / 2.0f;
  // at x <= -1 or x >= w every tap is off the map or has weight 0, so the position is clamped to
  // [-1, w] first (the same value, and the float -> int conversion stays in range) ...
  const float xc = fminf(fmaxf(x, -1.0f), (float)w), yc = fminf(fmaxf(y, -1.0f), (float)h);
  const float fx = floorf(xc), fy = floorf(yc);
  const int x0 = (int)fx, y0 = (int)fy, x1 = x0 + 1, y1 = y0 + 1;
  const float ax = xc - fx, ay = yc - fy;
  // ... and every tap index is clamped into the map before its load, whatever the coordinate was
  const int cx0 = min(max(x0, 0), w - 1), cx1 = min(max(x1, 0), w - 1);
  const int cy0 = min(max(y0, 0), h - 1), cy1 = min(max(y1, 0), h - 1);
  const float nw = map[(int64_t)cy0 * w + cx0], ne = map[(int64_t)cy0 * w + cx1];
  const float sw = map[(int64_t)cy1 * w + cx0], se = map[(int64_t)cy1 * w + cx1];
  const bool okx0 = x0 == cx0, okx1 = x1 == cx1, oky0 = y0 == cy0, oky1 = y1 == cy1;  // tap on the map
  float acc = 0.0f;
  if (okx0 && oky0) acc += nw * ((1.0f - ax) * (1.0f - ay));
  if (okx1 && oky0) acc += ne * (ax * (1.0f - ay));
  if (okx0 && oky1) acc += sw * ((1.0f - ax) * ay);
  if (okx1 && oky1) acc += se * (ax * ay);
  return acc;
}

// ---------------------------------------------------------------- chunk-local CDF
__global__ __launch_bounds__(SCAN_T) void corres_scan_kernel(sr_corres_desc d) {
  __shared__ float s_w[CHUNK];
  __shared__ double s_cdf[CHUNK];
  __shared__ double s_wave[SCAN_T / 64];
  __shared__ int s_cnt[SCAN_T / 64], s_last[SCAN_T / 64];
  const int p = blockIdx.y, c = blockIdx.x, t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const sr_corres_pair r = d.pairs[p];
  const int m = pair_m(r, d.max_m);
  const int base = c * CHUNK;
  if (base >= m) return;  // uniform per workgroup
  const PairWs w = carve(d.workspace, p, d.max_m);
  const float minc = d.min_conf;
  int cnt = 0, last = -1;
#pragma unroll
  for (int j = 0; j < RUN; ++j) {  // coalesced loads
    const int i = base + j * SCAN_T + t;
    float wt = 0.0f;
    if (i < m) {
      const float cv = certainty_at(r, i);
      if (cv > minc) {
        ++cnt;
        wt = cv;
        if (cv > 0.0f) last = i;
      }
    }
    s_w[j * SCAN_T + t] = wt;
  }
  __syncthreads();
  double run[RUN];
  double s = 0.0;
#pragma unroll
  for (int j = 0; j < RUN; ++j) {  // the lane's serial run
    s = __dadd_rn(s, (double)s_w[t * RUN + j]);
    run[j] = s;
  }
  double incl = s;  // wave64 inclusive scan of the lane totals
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const double up = __shfl_up(incl, o, 64);
    if (lane >= o) incl = __dadd_rn(up, incl);
  }
  double excl = __shfl_up(incl, 1, 64);
  if (lane == 0) excl = 0.0;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    cnt += __shfl_xor(cnt, o, 64);
    last = max(last, __shfl_xor(last, o, 64));
  }
  if (lane == 63) s_wave[wave] = incl;
  if (lane == 0) {
    s_cnt[wave] = cnt;
    s_last[wave] = last;
  }
  __syncthreads();
  double off = 0.0;  // the waves before this one, in order
  for (int q = 0; q < wave; ++q) off = __dadd_rn(off, s_wave[q]);
  off = __dadd_rn(off, excl);
#pragma unroll
  for (int j = 0; j < RUN; ++j) s_cdf[t * RUN + j] = __dadd_rn(off, run[j]);
  __syncthreads();
#pragma unroll
  for (int j = 0; j < RUN; ++j) {  // coalesced stores
    const int i = base + j * SCAN_T + t;
    if (i < m) w.cdf[i] = s_cdf[j * SCAN_T + t];
  }
  if (t == 0) {
    const int len = min(CHUNK, m - base);
    w.cend[c] = s_cdf[len - 1];  // the chunk total, bit-equal to the chunk's last CDF entry
    int n = 0, l = -1;
    for (int q = 0; q < SCAN_T / 64; ++q) {
      n += s_cnt[q];
      l = max(l, s_last[q]);
    }
    w.cinfo[2 * c] = n;
    w.cinfo[2 * c + 1] = l;
  }
}

// ---------------------------------------------------------------- chunk prefixes, T, n_valid
__global__ __launch_bounds__(64) void corres_chunks_kernel(sr_corres_desc d) {
  const int p = blockIdx.x, lane = threadIdx.x;
  const sr_corres_pair r = d.pairs[p];
  const int m = pair_m(r, d.max_m);
  const PairWs w = carve(d.workspace, p, d.max_m);
  if (m == 0) {
    if (lane == 0) {
      d.total[p] = 0.0;
      d.n_valid[p] = -1;  // a record the launch could not hold
      w.last[0] = -1;
    }
    return;
  }
  const int nc = n_chunks(m);
  double carry = 0.0, tlast = 0.0;
  int cnt = 0, last = -1;
  for (int c0 = 0; c0 < nc; c0 += 64) {
    const int c = c0 + lane;
    const double tot = c < nc ? w.cend[c] : 0.0;
    double incl = tot;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const double up = __shfl_up(incl, o, 64);
      if (lane >= o) incl = __dadd_rn(up, incl);
    }
    incl = __dadd_rn(carry, incl);
    double excl = __shfl_up(incl, 1, 64);
    if (lane == 0) excl = carry;
    if (c < nc) {
      w.cexcl[c] = excl;
      const double end = __dadd_rn(excl, tot);  // the CDF at the chunk's last entry, as a lookup forms it
      w.cend[c] = end;
      if (c == nc - 1) tlast = end;
      cnt += w.cinfo[2 * c];
      last = max(last, w.cinfo[2 * c + 1]);
    }
    carry = __shfl(incl, 63, 64);
  }
  const double T = __shfl(tlast, (nc - 1) & 63, 64);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    cnt += __shfl_xor(cnt, o, 64);
    last = max(last, __shfl_xor(last, o, 64));
  }
  if (lane == 0) {
    d.total[p] = T;
    d.n_valid[p] = cnt;
    w.last[0] = last;
  }
}

// first i in [0, n) with base + v[i] > x on (nearly) sorted v; n if there is none.  Whatever the
// data, the result is n or an index whose entry was tested and passed.
__device__ inline int first_above(const double* v, int n, double base, double x) {
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (__dadd_rn(base, v[mid]) > x)
      hi = mid;
    else
      lo = mid + 1;
  }
  return hi;
}

// ---------------------------------------------------------------- search + gather + depth
__global__ __launch_bounds__(SAMPLE_T) void corres_sample_kernel(sr_corres_desc d) {
  const int p = blockIdx.y, k = blockIdx.x * SAMPLE_T + threadIdx.x;
  if (k >= d.n_points) return;
  const sr_corres_pair r = d.pairs[p];
  const int m = pair_m(r, d.max_m);
  const PairWs w = carve(d.workspace, p, d.max_m);
  const int64_t e = (int64_t)p * d.n_points + k;
  const double T = d.total[p];
  const int lastpos = w.last[0];
  if (m == 0 || !(T > 0.0) || lastpos < 0) {  // no eligible correspondence: zeros (the caller raises)
    d.src_coords[2 * e] = d.src_coords[2 * e + 1] = 0.0f;
    d.dst_coords[2 * e] = d.dst_coords[2 * e + 1] = 0.0f;
    d.src_depth[e] = d.dst_depth[e] = 0.0f;
    if (d.index) d.index[e] = 0;
    return;
  }
  const double x = __dmul_rn(d.uniforms[e], T);
  const int nc = n_chunks(m);
  const int c = first_above(w.cend, nc, 0.0, x);
  int idx;
  if (c >= nc) {
    idx = lastpos;  // rounding put u * T >= T
  } else {
    const int base = c * CHUNK, len = min(CHUNK, m - base);
    // base_c + cdf[len - 1] is cend[c] bit for bit, so the search finds an entry
    idx = base + min(first_above(w.cdf + base, len, w.cexcl[c], x), len - 1);
    // a zero-weight entry is reachable only where two lanes' partial sums round apart by an ulp:
    // its step belongs to the next positive weight
    const float minc = d.min_conf;
    while (idx < lastpos) {
      const float cv = certainty_at(r, idx);
      if (cv > minc && cv > 0.0f) break;
      ++idx;
    }
    idx = min(idx, lastpos);
  }
  float sx, sy, dx, dy;
  if (r.format == SR_CORRES_PNG16) {
    const int iy = idx / r.ws, ix = idx - iy * r.ws;
    sx = linspace_at(ix, r.ws);
    sy = linspace_at(iy, r.hs);
    dx = png_coord(r.dst, idx);
    dy = png_coord(r.dst_y, idx);
  } else {
    const float* cs = (const float*)r.src;
    const float* cd = (const float*)r.dst;
    sx = cs[2 * (int64_t)idx];
    sy = cs[2 * (int64_t)idx + 1];
    dx = cd[2 * (int64_t)idx];
    dy = cd[2 * (int64_t)idx + 1];
  }
  d.src_coords[2 * e] = to_pixel(sx, r.w1);
  d.src_coords[2 * e + 1] = to_pixel(sy, r.h1);
  d.dst_coords[2 * e] = to_pixel(dx, r.w2);
  d.dst_coords[2 * e + 1] = to_pixel(dy, r.h2);
  d.src_depth[e] = bilinear_zeros(r.depth_src, r.h1, r.w1, sx, sy);
  d.dst_depth[e] = bilinear_zeros(r.depth_dst, r.h2, r.w2, dx, dy);
  if (d.index) d.index[e] = idx;
}

}  // namespace

extern "C" int64_t sr_corres_sample_workspace(int n_pairs, int max_m) {
  if (n_pairs <= 0 || max_m <= 0) return 0;
  return (int64_t)n_pairs * pair_stride(max_m);
}

extern "C" int sr_corres_sample(sr_stream_t stream, const sr_corres_desc* desc) {
  SR_CHECK(desc, SR_EINVAL, "sr_corres_sample: null desc");
  const sr_corres_desc& d = *desc;
  SR_CHECK(d.n_pairs > 0 && d.n_points > 0 && d.max_m > 0, SR_EINVAL,
           "sr_corres_sample: n_pairs %d, n_points %d and max_m %d must be positive", d.n_pairs, d.n_points, d.max_m);
  SR_CHECK(d.pairs && d.uniforms && d.src_coords && d.dst_coords && d.src_depth && d.dst_depth && d.total &&
               d.n_valid && d.workspace,
           SR_EINVAL, "sr_corres_sample: null pointer");
  SR_CHECK(d.n_pairs <= 65535, SR_EUNSUPPORTED, "sr_corres_sample: more than 65535 pairs in one call");
  SR_CHECK(d.workspace_doubles >= sr_corres_sample_workspace(d.n_pairs, d.max_m), SR_EINVAL,
           "sr_corres_sample: workspace of %lld doubles, needs %lld", (long long)d.workspace_doubles,
           (long long)sr_corres_sample_workspace(d.n_pairs, d.max_m));
  SR_CHECK(((uintptr_t)d.workspace & 7) == 0 && ((uintptr_t)d.uniforms & 7) == 0 && ((uintptr_t)d.total & 7) == 0,
           SR_EINVAL, "sr_corres_sample: fp64 buffers must be 8-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(corres_scan_kernel, dim3(n_chunks(d.max_m), d.n_pairs), dim3(SCAN_T), 0, s, d);
  hipLaunchKernelGGL(corres_chunks_kernel, dim3(d.n_pairs), dim3(64), 0, s, d);
  hipLaunchKernelGGL(corres_sample_kernel, dim3((d.n_points + SAMPLE_T - 1) / SAMPLE_T, d.n_pairs), dim3(SAMPLE_T), 0, s,
                     d);
  sr::note_kernel("corres_scan_kernel");
  return sr::check_launch("sr_corres_sample");
}
