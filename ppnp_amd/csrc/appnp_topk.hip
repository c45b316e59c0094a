// appnp_topk.hip -- top-k selection along the columns of a row-major block (gfx950).
//
// appnp_topk_columns turns X = Pi[:, idx] (n x b, what appnp_solve / appnp_propagate write) into
// b sparse rows of exactly k entries each, sorted by index: the rows of a canonical CSR whose row
// pointer is k * arange(b + 1).  It replaces the transposed copy + torch.topk + sort + nonzero of
// the dense route (batch-main.py:115-116, 140-142) and reads nothing back.  DESIGN.md 4.6.
//
// Order.  The candidate of (row r, column c) is v = (X[r, c] * row_scale[r]) * col_scale[c] in
// fp32.  Its key is the order-preserving uint32 image of v with -0 folded onto +0 and every NaN
// mapped to 0, below the image of -inf; larger key = better, equal keys go by the smaller row.
//
// Shape.  One thread mapping serves every pass: a workgroup of 256 threads owns a tile of 32
// adjacent columns (lane & 31: a half wave reads one 128-B line of a row) and 8 SUB-BLOCKS of
// kSubRows contiguous rows, one per half wave.  A thread therefore walks the rows of one column
// of one sub-block in increasing order, so ranks inside a sub-block are plain running counters;
// across sub-blocks they come from an exclusive scan.  The chain on `stream`:
//
//   memset                 the four 256-bin histograms of every column
//   4 x (hist, pick)       radix select, 8 bits per pass from the top: hist counts the digit of
//                          the keys that match the prefix found so far (LDS histograms laid out
//                          [bin][column], merged into the workspace by integer atomics, empty bins
//                          skipped); pick (a wave per column) finds the digit in which the k-th
//                          largest key lies and how many keys are still wanted inside it
//   count                  per (sub-block, column): keys above the threshold key T and equal to it
//   scan                   exclusive scan of both counts over the sub-blocks of a column
//   emit                   a thread places its entries at (scanned offset + running count): every
//                          key > T, and the first `need` keys == T in row order
//
// X is read 6 times (4 hist + count + emit).  Only integer atomics are used and every output
// position is a pure function of the input, so results are bitwise reproducible.  The phases are
// separate launches: no workgroup ever waits for another one.
#include <algorithm>

#include "appnp_internal.h"
#include "appnp_topk_key.h"  // order_key, digit_search
#include "../../include/ppnp_amd.h"

namespace appnp {
namespace {

constexpr int kTileCols = 32;                 // one 128-B line of fp32 per row
constexpr int kSlots = kBlock / kTileCols;    // sub-blocks per workgroup (one per half wave)
constexpr int kSubRows = 128;                 // rows of a sub-block
constexpr int kBins = 256;
constexpr int kUnroll = 8;                    // rows in flight per thread
constexpr int kScanThreads = 1024;
constexpr int kScanSlots = kScanThreads / kTileCols;

struct TopkArgs {
  const float* x;
  const float* row_scale;
  const float* col_scale;
  int64_t ld_x, n, b;
  int64_t n_sub;    // sub-blocks of kSubRows rows
  int64_t tiles;    // column tiles
  uint32_t* hist;   // [4][b][kBins]
  uint32_t* state;  // [b][2]: key prefix found so far, entries still wanted inside it
  uint32_t* cnt;    // [2][n_sub][b]: keys > T, keys == T (after the scan: exclusive offsets)
  int32_t* out_idx;
  float* out_val;
  int64_t ld_out;
  int32_t k;
};

// The thread's place: column c of sub-block sb (rows [r0, r1)); false when it has none.
__device__ __forceinline__ bool my_place(const TopkArgs& a, int64_t& sb, int64_t& c, int64_t& r0,
                                         int64_t& r1) {
  const int64_t tile = (int64_t)blockIdx.x % a.tiles;
  const int64_t rb = (int64_t)blockIdx.x / a.tiles;
  c = tile * kTileCols + (threadIdx.x & (kTileCols - 1));
  sb = rb * kSlots + (threadIdx.x / kTileCols);
  r0 = sb * kSubRows;
  r1 = std::min<int64_t>(a.n, r0 + kSubRows);
  return c < a.b && sb < a.n_sub;
}

// f(row, v) for the rows [r0, r1) of column c in increasing order, kUnroll loads in flight.
template <typename F>
__device__ __forceinline__ void for_rows(const TopkArgs& a, int64_t c, int64_t r0, int64_t r1,
                                         F&& f) {
  const float* p = a.x + r0 * a.ld_x + c;
  const bool has_cs = a.col_scale != nullptr;
  const float cs = has_cs ? a.col_scale[c] : 1.0f;
  int64_t r = r0;
  for (; r + kUnroll <= r1; r += kUnroll, p += kUnroll * a.ld_x) {
    float v[kUnroll];
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) v[u] = p[u * a.ld_x];
    if (a.row_scale) {
#pragma unroll
      for (int u = 0; u < kUnroll; ++u) v[u] = v[u] * a.row_scale[r + u];
    }
    if (has_cs) {
#pragma unroll
      for (int u = 0; u < kUnroll; ++u) v[u] = v[u] * cs;
    }
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) f(r + u, v[u]);
  }
  for (; r < r1; ++r, p += a.ld_x) {
    float v = *p;
    if (a.row_scale) v = v * a.row_scale[r];
    if (has_cs) v = v * cs;
    f(r, v);
  }
}

// Pass `pass` of the radix select: digit (key >> shift) & 255 of the keys whose higher bits equal
// the column's prefix.
__global__ __launch_bounds__(kBlock) void k_topk_hist(TopkArgs a, int pass) {
  __shared__ uint32_t lh[kBins * kTileCols];  // [bin][column]: a half wave hits 32 banks
  for (int i = threadIdx.x; i < kBins * kTileCols; i += kBlock) lh[i] = 0u;
  __syncthreads();
  int64_t sb, c, r0, r1;
  const int lc = threadIdx.x & (kTileCols - 1);
  if (my_place(a, sb, c, r0, r1)) {
    const int shift = 24 - 8 * pass;
    const uint32_t prefix = pass ? a.state[2 * c] : 0u;
    // pass 0 has no higher bits: both sides shift to 0
    const int hs = pass ? shift + 8 : 31;
    const uint32_t want = pass ? (prefix >> hs) : 0u;
    for_rows(a, c, r0, r1, [&](int64_t, float v) {
      const uint32_t key = order_key(v);
      const uint32_t hi = pass ? (key >> hs) : 0u;
      if (hi == want) atomicAdd(&lh[((key >> shift) & 255u) * kTileCols + lc], 1u);
    });
  }
  __syncthreads();
  const int64_t tile = (int64_t)blockIdx.x % a.tiles;
  uint32_t* gh = a.hist + (int64_t)pass * a.b * kBins;
  for (int i = threadIdx.x; i < kBins * kTileCols; i += kBlock) {
    // LDS order (conflict-free); most bins are empty, so few atomics leave the workgroup
    const int bin = i / kTileCols, col = i % kTileCols;
    const int64_t gc = tile * kTileCols + col;
    const uint32_t x = lh[i];
    if (x != 0u && gc < a.b) atomicAdd(&gh[gc * kBins + bin], x);
  }
}

// One wave per column: the digit in which the (wanted)-th largest matching key lies.
__global__ __launch_bounds__(kBlock) void k_topk_pick(TopkArgs a, int pass) {
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t c = (int64_t)blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6);
  if (c >= a.b) return;  // whole wave
  const uint32_t* h = a.hist + ((int64_t)pass * a.b + c) * kBins + 4 * lane;
  const uint32_t want = pass ? a.state[2 * c + 1] : (uint32_t)a.k;
  const uint32_t prefix = pass ? a.state[2 * c] : 0u;
  uint32_t digit, above, in;
  if (digit_search(h[0], h[1], h[2], h[3], want, lane, digit, above, in)) {  // exactly one lane
    a.state[2 * c] = prefix | (digit << (24 - 8 * pass));
    a.state[2 * c + 1] = want - above;
  }
}

__global__ __launch_bounds__(kBlock) void k_topk_count(TopkArgs a) {
  int64_t sb, c, r0, r1;
  if (!my_place(a, sb, c, r0, r1)) return;
  const uint32_t T = a.state[2 * c];
  uint32_t gt = 0, eq = 0;
  for_rows(a, c, r0, r1, [&](int64_t, float v) {
    const uint32_t key = order_key(v);
    gt += key > T ? 1u : 0u;
    eq += key == T ? 1u : 0u;
  });
  a.cnt[sb * a.b + c] = gt;
  a.cnt[(a.n_sub + sb) * a.b + c] = eq;
}

// Exclusive scan of both counts over the sub-blocks of each column; one workgroup per column
// tile, kScanSlots contiguous chunks of sub-blocks per column.
__global__ __launch_bounds__(kScanThreads) void k_topk_scan(TopkArgs a) {
  __shared__ uint32_t part[2][kScanSlots][kTileCols];
  const int lc = threadIdx.x & (kTileCols - 1), slot = threadIdx.x / kTileCols;
  const int64_t c = (int64_t)blockIdx.x * kTileCols + lc;
  const int64_t chunk = (a.n_sub + kScanSlots - 1) / kScanSlots;
  const int64_t s0 = std::min<int64_t>(a.n_sub, slot * chunk);
  const int64_t s1 = std::min<int64_t>(a.n_sub, s0 + chunk);
  uint32_t* gt = a.cnt;
  uint32_t* eq = a.cnt + a.n_sub * a.b;
  uint32_t sg = 0, se = 0;
  if (c < a.b)
    for (int64_t s = s0; s < s1; ++s) {
      sg += gt[s * a.b + c];
      se += eq[s * a.b + c];
    }
  part[0][slot][lc] = sg;
  part[1][slot][lc] = se;
  __syncthreads();
  if (c >= a.b) return;
  uint32_t og = 0, oe = 0;
  for (int j = 0; j < slot; ++j) {
    og += part[0][j][lc];
    oe += part[1][j][lc];
  }
  for (int64_t s = s0; s < s1; ++s) {
    const uint32_t g = gt[s * a.b + c], e = eq[s * a.b + c];
    gt[s * a.b + c] = og;
    eq[s * a.b + c] = oe;
    og += g;
    oe += e;
  }
}

__global__ __launch_bounds__(kBlock) void k_topk_emit(TopkArgs a) {
  int64_t sb, c, r0, r1;
  if (!my_place(a, sb, c, r0, r1)) return;
  const uint32_t T = a.state[2 * c];
  const uint32_t need = a.state[2 * c + 1];  // keys == T to take, lowest rows first
  uint32_t e = a.cnt[(a.n_sub + sb) * a.b + c];
  uint32_t pos = a.cnt[sb * a.b + c] + std::min(e, need);
  if (pos >= (uint32_t)a.k) return;  // this column's k entries all lie in earlier sub-blocks
  int32_t* oi = a.out_idx + c * a.ld_out;
  float* ov = a.out_val + c * a.ld_out;
  const uint32_t k = (uint32_t)a.k;
  for_rows(a, c, r0, r1, [&](int64_t r, float v) {
    const uint32_t key = order_key(v);
    const bool tie = key == T;
    const bool take = key > T || (tie && e < need);
    e += tie ? 1u : 0u;
    if (take && pos < k) {  // pos < k holds by construction; the guard keeps a store in bounds
      oi[pos] = (int32_t)r;
      ov[pos] = v;
    }
    pos += take ? 1u : 0u;
  });
}

inline int64_t sub_blocks(int64_t n) { return (n + kSubRows - 1) / kSubRows; }

// words of the three workspace parts
inline size_t hist_words(int64_t b) { return (size_t)4 * (size_t)b * kBins; }
inline size_t state_words(int64_t b) { return (size_t)2 * (size_t)b; }
inline size_t cnt_words(int64_t n, int64_t b) { return (size_t)2 * (size_t)sub_blocks(n) * (size_t)b; }

}  // namespace
}  // namespace appnp

extern "C" size_t appnp_topk_workspace_bytes(int64_t n, int64_t b, int k) {
  using namespace appnp;
  (void)k;
  if (n <= 0 || b <= 0 || n > INT32_MAX) return 0;
  return round_up((hist_words(b) + state_words(b) + cnt_words(n, b)) * sizeof(uint32_t), 256);
}

extern "C" int appnp_topk_columns(const float* X, int64_t ld_x, int64_t n, int64_t b, int k,
                                  const float* row_scale, const float* col_scale,
                                  int32_t* out_idx, float* out_val, int64_t ld_out, void* ws,
                                  size_t ws_bytes, void* stream) {
  using namespace appnp;
  if (n < 0 || b < 0 || ld_x < b || k < 1 || ld_out < k || n > INT32_MAX) return APPNP_EINVAL;
  if (n == 0 || b == 0) return APPNP_OK;
  if (k > n || !X || !out_idx || !out_val || !ws) return APPNP_EINVAL;
  if (ws_bytes < appnp_topk_workspace_bytes(n, b, k)) return APPNP_EINVAL;
  if (reinterpret_cast<uintptr_t>(ws) % sizeof(uint32_t) != 0) return APPNP_EINVAL;

  TopkArgs a{};
  a.x = X;
  a.row_scale = row_scale;
  a.col_scale = col_scale;
  a.ld_x = ld_x;
  a.n = n;
  a.b = b;
  a.n_sub = sub_blocks(n);
  a.tiles = (b + kTileCols - 1) / kTileCols;
  a.hist = static_cast<uint32_t*>(ws);
  a.state = a.hist + hist_words(b);
  a.cnt = a.state + state_words(b);
  a.out_idx = out_idx;
  a.out_val = out_val;
  a.ld_out = ld_out;
  a.k = k;
  const int64_t row_blocks = (a.n_sub + kSlots - 1) / kSlots;
  // a 1-D grid of (row block, column tile) pairs; HIP bounds a grid's threads by 2^32
  if (a.tiles > ((int64_t)1 << 24) - 1 || row_blocks > (((int64_t)1 << 24) - 1) / a.tiles)
    return APPNP_ERANGE;
  const dim3 grid((unsigned)(row_blocks * a.tiles)), block(kBlock);
  const dim3 pick_grid((unsigned)((b + kWavesPerBlock - 1) / kWavesPerBlock));
  hipStream_t s = static_cast<hipStream_t>(stream);

  ktimer_begin(s);
  const hipError_t me = hipMemsetAsync(a.hist, 0, hist_words(b) * sizeof(uint32_t), s);
  ktimer_mark(s, APPNP_KT_COPY);
  if (me != hipSuccess) return APPNP_EDEVICE;
  int rc = APPNP_OK;
  for (int pass = 0; pass < 4 && rc == APPNP_OK; ++pass) {
    rc = timed_launch(s, APPNP_KT_COPY,
                      [&] { hipLaunchKernelGGL(k_topk_hist, grid, block, 0, s, a, pass); });
    if (rc == APPNP_OK)
      rc = timed_launch(s, APPNP_KT_COPY,
                        [&] { hipLaunchKernelGGL(k_topk_pick, pick_grid, block, 0, s, a, pass); });
  }
  if (rc == APPNP_OK)
    rc = timed_launch(s, APPNP_KT_COPY,
                      [&] { hipLaunchKernelGGL(k_topk_count, grid, block, 0, s, a); });
  if (rc == APPNP_OK)
    rc = timed_launch(s, APPNP_KT_COPY, [&] {
      hipLaunchKernelGGL(k_topk_scan, dim3((unsigned)a.tiles), dim3(kScanThreads), 0, s, a);
    });
  if (rc == APPNP_OK)
    rc = timed_launch(s, APPNP_KT_COPY,
                      [&] { hipLaunchKernelGGL(k_topk_emit, grid, block, 0, s, a); });
  return rc;
}
