// A stable device-wide sort of (64-bit key, 32-bit value) pairs on gfx950: least significant digit first,
// 8 bits per pass.  sr_cloud_voxel sorts its voxel keys with it; it is exported on its own
// (sr_sort_pairs) for whatever else needs an order: sparsification curves, cell lists.
//
// Contract (DESIGN.md "Downsampling point clouds", include/sfm_amd.h): the result is
// np.argsort(keys & mask, kind="stable"); bits above key_bits ride along in keys_out; inputs are not
// written.  Nothing depends on execution order: no kernel waits on another workgroup, no position
// comes from the arrival order of an atomic, and two runs give the same bits.
//
// The tile plan, restated in numpy by tests/cloud_voxel_ref.py (sort_plan_model):
//   tile      2048 consecutive elements, one workgroup of four waves.  Wave w owns the 512 elements
//             [512 w, 512 w + 512) of the tile and reads them in eight rounds of 64 (round k, lane l is
//             element 512 w + 64 k + l): every load is contiguous, and ascending (wave, round, lane) is
//             ascending input position.
//   sort_hist_kernel     table[digit][tile] = the tile's count of the digit.  A wave finds the lanes
//                        that share its digit with eight ballots; the lowest of them adds their number
//                        to the LDS histogram (an integer count: the order of the adds is immaterial).
//                        Each workgroup then adds its 256 counts to the pass's digit totals.
//   sort_scan_kernel     one workgroup per digit d: base = the sum of the totals of the digits below d,
//                        then the exclusive scan of row d of the table, in place (sr::scan_row).  The table is
//                        digit-major, so this is the exclusive scan of the whole [256][tiles] table.
//                        Every workgroup works from the totals alone: none waits for another.
//   sort_scatter_kernel  a lane's rank among its tile's equal digits = (the count of the digit in the
//                        waves before it) + (its wave's count in earlier rounds, a per-wave LDS counter
//                        that only this wave touches) + (the lanes below it in its ballot group).
//                        position = table[digit][tile] + rank; the store is guarded by position < n.
//   Passes ping-pong between two buffers of the workspace; the first reads the inputs, the last writes
//   the outputs.
#include "sr_common.h"
#include "sr_eval.h"

namespace {

constexpr int ST_T = 256;                 // threads of every workgroup here
constexpr int ST_WAVES = ST_T / 64;
constexpr int ST_ROUNDS = 8;              // elements per lane
constexpr int ST_WAVE_ELEMS = 64 * ST_ROUNDS;
constexpr int ST_TILE = ST_T * ST_ROUNDS;  // 2048
constexpr int ST_MAX_PASSES = 8;
constexpr int64_t ST_MAX_N = 2147483647LL;

using sr::align16;

struct SortPlan {
  int64_t tiles;
  int64_t off_keys[2], off_vals[2], off_table, off_totals, bytes;
};

bool sort_plan(int64_t n, SortPlan& p) {
  if (n < 1 || n > ST_MAX_N) return false;
  p.tiles = (n + ST_TILE - 1) / ST_TILE;
  int64_t o = 0;
  p.off_keys[0] = o, o = align16(o + 8 * n);
  p.off_keys[1] = o, o = align16(o + 8 * n);
  p.off_vals[0] = o, o = align16(o + 4 * n);
  p.off_vals[1] = o, o = align16(o + 4 * n);
  p.off_table = o, o = align16(o + 256 * p.tiles * 4);
  p.off_totals = o, o += ST_MAX_PASSES * 256 * 4;
  p.bytes = o;
  return true;
}

struct SortArgs {
  const uint64_t* keys_in;
  const uint32_t* vals_in;  // NULL: the element's own index
  uint64_t* keys_out;       // NULL: not written
  uint32_t* vals_out;
  uint32_t* table;          // [256][tiles]
  uint32_t* totals;         // [256] of this pass
  int64_t n, tiles;
  uint64_t key_mask;
  int shift;
};

__device__ inline int sort_digit(uint64_t key, const SortArgs& a) { return (int)(((key & a.key_mask) >> a.shift) & 255u); }

// the lanes of the wave that are live and hold the same digit as this one (garbage in a lane that is not live)
__device__ inline uint64_t match_digit(int digit, bool live) {
  uint64_t m = __ballot(live);
#pragma unroll
  for (int b = 0; b < 8; ++b) {
    const bool bit = (digit >> b) & 1;
    const uint64_t v = __ballot(bit);
    m &= bit ? v : ~v;
  }
  return m;
}

__device__ inline uint64_t lanes_below(int lane) { return (uint64_t(1) << lane) - 1; }

__global__ __launch_bounds__(ST_T) void sort_hist_kernel(SortArgs a) {
  __shared__ uint32_t s_hist[256];
  const int t = threadIdx.x, wave = t >> 6, lane = t & 63;
  const int64_t tile = blockIdx.x;
  s_hist[t] = 0;
  __syncthreads();
  const int64_t base = tile * ST_TILE + wave * ST_WAVE_ELEMS + lane;
#pragma unroll
  for (int k = 0; k < ST_ROUNDS; ++k) {
    const int64_t i = base + 64 * k;
    const bool live = i < a.n;
    const int digit = live ? sort_digit(a.keys_in[i], a) : 0;
    const uint64_t m = match_digit(digit, live);
    if (live && (m & lanes_below(lane)) == 0) atomicAdd(&s_hist[digit], (uint32_t)__popcll(m));
  }
  __syncthreads();
  const uint32_t c = s_hist[t];
  a.table[(int64_t)t * a.tiles + tile] = c;
  if (c) atomicAdd(&a.totals[t], c);
}

// grid 256: workgroup d scans row d of the table in place, starting from the totals of the digits below d
__global__ __launch_bounds__(ST_T) void sort_scan_kernel(SortArgs a) {
  __shared__ uint32_t s_scan[ST_T];
  const int t = threadIdx.x, d = blockIdx.x;
  s_scan[t] = t < d ? a.totals[t] : 0u;
  __syncthreads();
  for (int s = ST_T / 2; s > 0; s >>= 1) {
    if (t < s) s_scan[t] += s_scan[t + s];
    __syncthreads();
  }
  const uint32_t base = s_scan[0];  // read by every lane before scan_row's first barrier lets s_scan be written
  uint32_t* row = a.table + (int64_t)d * a.tiles;
  sr::scan_row<ST_T>(a.tiles, base, s_scan, [&](int64_t e) { return row[e]; }, [&](int64_t e, uint32_t x) { row[e] = x; });
}

__global__ __launch_bounds__(ST_T) void sort_scatter_kernel(SortArgs a) {
  __shared__ uint32_t s_wave[ST_WAVES][256];  // a wave's running count of every digit, then its base position
  const int t = threadIdx.x, wave = t >> 6, lane = t & 63;
  const int64_t tile = blockIdx.x;
#pragma unroll
  for (int w = 0; w < ST_WAVES; ++w) s_wave[w][t] = 0;
  __syncthreads();
  const int64_t base = tile * ST_TILE + wave * ST_WAVE_ELEMS + lane;
  uint64_t key[ST_ROUNDS];
  uint32_t val[ST_ROUNDS], rank[ST_ROUNDS];
  int digit[ST_ROUNDS];
#pragma unroll
  for (int k = 0; k < ST_ROUNDS; ++k) {
    const int64_t i = base + 64 * k;
    const bool live = i < a.n;
    key[k] = live ? a.keys_in[i] : 0u;
    val[k] = live ? (a.vals_in ? a.vals_in[i] : (uint32_t)i) : 0u;
    digit[k] = live ? sort_digit(key[k], a) : -1;
  }
  uint32_t* mine = s_wave[wave];  // only this wave reads and writes it before the barrier
#pragma unroll
  for (int k = 0; k < ST_ROUNDS; ++k) {
    const bool live = digit[k] >= 0;
    const int dg = live ? digit[k] : 0;
    const uint64_t m = match_digit(dg, live);
    const uint64_t below = m & lanes_below(lane);
    const uint32_t seen = mine[dg];  // every lane of a group reads the count of the earlier rounds ...
    __builtin_amdgcn_wave_barrier();
    if (live && below == 0) mine[dg] = seen + (uint32_t)__popcll(m);  // ... before its lowest lane advances it
    __builtin_amdgcn_wave_barrier();
    rank[k] = seen + (uint32_t)__popcll(below);
  }
  __syncthreads();
  {  // digit t: the waves' counts become their base positions, in wave order
    uint32_t run = a.table[(int64_t)t * a.tiles + tile];
#pragma unroll
    for (int w = 0; w < ST_WAVES; ++w) {
      const uint32_t c = s_wave[w][t];
      s_wave[w][t] = run;
      run += c;
    }
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < ST_ROUNDS; ++k) {
    if (digit[k] < 0) continue;
    const uint32_t pos = mine[digit[k]] + rank[k];
    if ((int64_t)pos < a.n) {
      if (a.keys_out) a.keys_out[pos] = key[k];
      a.vals_out[pos] = val[k];
    }
  }
}

}  // namespace

namespace sr {

int64_t sort_workspace(int64_t n) {
  SortPlan p;
  return sort_plan(n, p) ? p.bytes : 0;
}

// validated arguments -> the clearing node and three launches per pass (also sr_cloud_voxel's sort)
void sort_launch(hipStream_t s, const uint64_t* keys_in, const uint32_t* vals_in, uint64_t* keys_out, uint32_t* vals_out,
                 int64_t n, int key_bits, void* workspace) {
  SortPlan p;
  sort_plan(n, p);
  char* ws = (char*)workspace;
  uint64_t* kbuf[2] = {(uint64_t*)(ws + p.off_keys[0]), (uint64_t*)(ws + p.off_keys[1])};
  uint32_t* vbuf[2] = {(uint32_t*)(ws + p.off_vals[0]), (uint32_t*)(ws + p.off_vals[1])};
  uint32_t* totals = (uint32_t*)(ws + p.off_totals);
  const int passes = (key_bits + 7) / 8;
  (void)hipMemsetAsync(totals, 0, ST_MAX_PASSES * 256 * 4, s);
  SortArgs a{};
  a.table = (uint32_t*)(ws + p.off_table);
  a.n = n, a.tiles = p.tiles;
  a.key_mask = key_bits >= 64 ? ~uint64_t(0) : (uint64_t(1) << key_bits) - 1;
  for (int pass = 0; pass < passes; ++pass) {
    const bool first = pass == 0, last = pass == passes - 1;
    a.keys_in = first ? keys_in : kbuf[(pass - 1) & 1];
    a.vals_in = first ? vals_in : vbuf[(pass - 1) & 1];
    a.keys_out = last ? keys_out : kbuf[pass & 1];
    a.vals_out = last ? vals_out : vbuf[pass & 1];
    a.totals = totals + 256 * pass;
    a.shift = 8 * pass;
    const dim3 grid((unsigned)p.tiles), block(ST_T);
    hipLaunchKernelGGL(sort_hist_kernel, grid, block, 0, s, a);
    hipLaunchKernelGGL(sort_scan_kernel, dim3(256), block, 0, s, a);
    hipLaunchKernelGGL(sort_scatter_kernel, grid, block, 0, s, a);
  }
}

}  // namespace sr

extern "C" int64_t sr_sort_workspace(int64_t n) { return sr::sort_workspace(n); }

extern "C" int sr_sort_pairs(sr_stream_t stream, const sr_sort_desc* desc) {
  SR_CHECK(desc, SR_EINVAL, "sr_sort_pairs: null desc");
  const sr_sort_desc& d = *desc;
  SR_CHECK(d.keys_in && d.vals_out && d.workspace, SR_EINVAL, "sr_sort_pairs: null keys_in, vals_out or workspace");
  SR_CHECK(d.n >= 1 && d.n <= ST_MAX_N, SR_EINVAL, "sr_sort_pairs: n %lld outside [1, 2^31 - 1]", (long long)d.n);
  SR_CHECK(d.key_bits >= 1 && d.key_bits <= 64, SR_EINVAL, "sr_sort_pairs: key_bits %d outside [1, 64]", d.key_bits);
  SR_CHECK(d.keys_out != d.keys_in && (!d.vals_in || d.vals_out != d.vals_in), SR_EINVAL,
           "sr_sort_pairs: an output may not be its own input");
  SR_CHECK(((uintptr_t)d.keys_in & 7) == 0 && ((uintptr_t)d.keys_out & 7) == 0, SR_EINVAL,
           "sr_sort_pairs: keys must be 8-byte aligned");
  SR_CHECK(((uintptr_t)d.vals_in & 3) == 0 && ((uintptr_t)d.vals_out & 3) == 0, SR_EINVAL,
           "sr_sort_pairs: values must be 4-byte aligned");
  const int64_t need = sr::sort_workspace(d.n);
  SR_CHECK_WORKSPACE("sr_sort_pairs", d.workspace, d.workspace_bytes, need);
  sr::sort_launch((hipStream_t)stream, d.keys_in, d.vals_in, d.keys_out, d.vals_out, d.n, d.key_bits, d.workspace);
  sr::note_kernel("sort_scatter_kernel");
  return sr::check_launch("sr_sort_pairs");
}
