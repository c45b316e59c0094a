// appnp_push.hip -- PPR columns by local forward push (Andersen-Chung-Lang), gfx950.
//
// appnp_push_columns writes X = Pi[:, sources] (n x b, the block appnp_topk_columns reads) like
// appnp_solve does for one-hot columns, but a source's work follows its residual, not n: with
// T = (1-alpha) A_hat it keeps an estimate p and a residual r (p = 0, r = e_s at the start) and
// moves r_i to alpha r_i in p_i and T[:, i] r_i in r, for the nodes i whose residual has reached
// the threshold eps * w_i only.  DESIGN.md 4.7.
//
// Fixed point.  p and r are int64 in units of 2^-44.  A round is synchronous: its frontier is
// F = { j : r_j >= thr_j }, thr_j = max(1, ceil(eps w_j 2^44)) (w_j = 1 / dinv_j for sym, 1 for
// rw); every i in F is TAKEN first (t_i = r_i, r_i = 0), then pushed:
//   p_i += (int64)((double)t_i * alpha)
//   r_j += (int64)(((double)t_i * val) * (1 - alpha))   for every entry (j, i) of column i
// Every sum is an integer sum and a round is a pure function of the state before it, so X does
// not depend on the schedule: it is bitwise reproducible (tests/push_ref.py replays it in numpy).
//
// Shape.  One workgroup of kPushBlock threads per source, the whole round loop (push_rounds)
// inside the kernel, workgroup barriers only: a workgroup touches nothing but its own source's
// slices of the workspace, so no workgroup ever waits for (or reads from) another one.  Per round:
//   take   a thread per frontier entry q: t = exchange(r_i, 0) into take[q]; p_i += alpha t
//   push   a wave per frontier entry, lanes over the entries of row i of A_hat^T (coalesced col /
//          val loads): old = fetch_add(r_j, c); the one add that carries r_j over thr_j appends j
//          to the next frontier list (LDS counter; the store is clamped to the list's capacity).
//          A frontier shorter than the workgroup's wave count is pushed by all waves together,
//          each on every kPushWaves-th chunk of 64 entries of a row (walk_rows).
// A_hat >= 0 is assumed: residuals then only grow between takes, so a node is appended once per
// round.  r is accessed by 64-bit integer atomics only; the lists and takes are plain stores read
// after a workgroup barrier.  The launches on `stream`: clear of r and p, thresholds (sym),
// push, emit (p -> X through an LDS transpose, coalesced on both sides).
//
// appnp_push_topk (further down) runs the same push on a grid of reusable slots
// and selects each source's top k straight from the nodes it took: no dense block.  Both entry
// points share the round loop, the workspace layout (push_layout) and the host side up to the
// push launch (push_call).
#include <algorithm>

#include "appnp_internal.h"
#include "appnp_topk_key.h"  // order_key, digit_search
#include "../../include/ppnp_amd.h"

namespace appnp {
namespace {

constexpr int kPushBlock = 1024;
constexpr int kPushWaves = kPushBlock / kWave;
constexpr int64_t kOne = (int64_t)1 << 44;  // 1.0 in fixed point
constexpr double kUnit = 1.0 / 17592186044416.0;  // 2^-44
constexpr int kEmitTile = 32;
constexpr int kPushLists = 2;  // int32 lists per source of appnp_push_columns: the two frontiers
constexpr int kTopkLists = 3;  // ... per slot of appnp_push_topk: and the taken list

// What the round loop reads: the arguments both kernels share.  A SLAB is the slice of r, p, take
// and lists one workgroup works on: a source's (appnp_push_columns) or a slot's (appnp_push_topk).
struct PushCore {
  const int32_t* row_ptr;  // A_hat^T: row i holds the entries (j, i) of column i of A_hat
  const int32_t* col;
  const float* val;
  const int64_t* thr;      // [n] (sym); null for rw (every threshold is threshold(eps, 1))
  const int64_t* sources;  // [b]
  int64_t n, b;
  float alpha, beta;       // beta = 1.0f - alpha, in fp32
  float eps;
  int max_rounds;
  int64_t* r;              // [slabs][n]
  int64_t* p;              // [slabs][n]
  int64_t* take;           // [slabs][n] the takes of a round, by frontier position
  int32_t* lists;          // [slabs][lists][n]
  int32_t* rounds;
  int32_t* left;
};

struct PushArgs {
  PushCore core;
  float* x;
  int64_t ld_x;
};

__host__ __device__ __forceinline__ int64_t threshold(float eps, double w) {
  const double t = ceil(((double)eps * w) * 17592186044416.0);
  return t < 1.0 ? (int64_t)1 : (int64_t)t;
}

// sym: w_j = 1 / dinv_j
__global__ __launch_bounds__(kBlock) void k_push_thr(const double* dinv, int64_t n, float eps,
                                                     int64_t* thr) {
  const int64_t j = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (j < n) thr[j] = threshold(eps, 1.0 / dinv[j]);
}

// r and p of every slab to zero: 16-byte stores, grid-stride
__global__ __launch_bounds__(kBlock) void k_push_clear(ulonglong2* dst, int64_t n16) {
  const int64_t stride = (int64_t)gridDim.x * kBlock;
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n16; i += stride)
    dst[i] = make_ulonglong2(0ull, 0ull);
}

__device__ __forceinline__ int64_t fetch_add(int64_t* p, int64_t v) {
  return __hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__device__ __forceinline__ int64_t load_i64(const int64_t* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__device__ __forceinline__ void store_i64(int64_t* p, int64_t v) {
  __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

struct PushSlab {
  int64_t* r;
  int64_t* p;
  int64_t* take;
  int32_t* list;  // `lists` lists of capacity n
};

__device__ __forceinline__ PushSlab slab(const PushCore& a, int64_t w, int lists) {
  return {a.r + w * a.n, a.p + w * a.n, a.take + w * a.n, a.lists + lists * w * a.n};
}

__device__ __forceinline__ void report(const PushCore& a, int64_t c, int rounds, int64_t left) {
  if (threadIdx.x == 0) {
    if (a.rounds) a.rounds[c] = rounds;
    if (a.left) a.left[c] = (int32_t)left;
  }
}

// The workgroup's walk of the rows i = nodes[q], q < m, of A_hat^T: per row v = row(q), then
// entry(v, e) for the thread's entries e of the row.  A list shorter than the workgroup's wave
// count is walked by all waves together, each on every kPushWaves-th chunk of 64 entries of a
// row; a longer one by a wave per row.
template <typename Row, typename Entry>
__device__ __forceinline__ void walk_rows(const PushCore& a, const int32_t* nodes, int64_t m,
                                          Row&& row, Entry&& entry) {
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x >> 6;
  // entries [off, off + kWave) of every `step` entries of the rows q0, q0 + dq, ...
  const bool together = m < kPushWaves;
  const int64_t q0 = together ? 0 : wave, dq = together ? 1 : kPushWaves;
  const int off = (together ? wave * kWave : 0) + lane;
  const int step = together ? kPushBlock : kWave;
  for (int64_t q = q0; q < m; q += dq) {
    const int64_t i = nodes[q];
    const auto v = row(q);
    const int64_t e1 = a.row_ptr[i + 1];
    for (int64_t e = (int64_t)a.row_ptr[i] + off; e < e1; e += step) entry(v, e);
  }
}

struct PushEnd {
  int rounds;
  int64_t left;  // the size of the frontier the loop ended on
};

// The push of source s on the slab w, by the whole workgroup: the set-up (r_s = 1 and, if that
// reaches its threshold, the frontier {s}; an empty frontier for a source outside [0, n)) and the
// synchronous rounds, until the frontier is empty or max_rounds have run.  taken(i) runs once per
// take of a node i, between the exchange on r_i and the add to p_i.  What the caller wrote to LDS
// before the call is ordered by the barrier that ends the set-up; every append of the rounds, and
// of `taken`, by the last barrier passed before the return.
template <typename Taken>
__device__ __forceinline__ PushEnd push_rounds(const PushCore& a, int64_t s, const PushSlab& w,
                                               Taken&& taken) {
  __shared__ int cnt[2];  // the lengths of the two frontier lists
  const int64_t n = a.n;
  const int tid = threadIdx.x;
  const int64_t thr_rw = threshold(a.eps, 1.0);
  const double alpha = (double)a.alpha, beta = (double)a.beta;
  if (tid == 0) {
    cnt[0] = 0;
    cnt[1] = 0;
    if (s >= 0 && s < n) {
      const int64_t thr_s = a.thr ? a.thr[s] : thr_rw;
      store_i64(w.r + s, kOne);
      w.list[0] = (int32_t)s;
      cnt[0] = kOne >= thr_s ? 1 : 0;
    }
  }
  __syncthreads();
  int cur = 0, round = 0;
  int64_t m = 0;  // frontier size
  for (;;) {
    m = std::min<int64_t>((int64_t)cnt[cur], n);  // an append past the capacity was not stored
    if (m == 0 || round == a.max_rounds) break;
    if (tid == 0) cnt[cur ^ 1] = 0;  // last read a round ago, two barriers back
    const int32_t* fl = w.list + (int64_t)cur * n;
    int32_t* nl = w.list + (int64_t)(cur ^ 1) * n;
    for (int64_t q = tid; q < m; q += kPushBlock) {
      const int64_t i = fl[q];
      const int64_t t =
          __hip_atomic_exchange(w.r + i, (int64_t)0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      w.take[q] = t;
      taken(i);
      fetch_add(w.p + i, (int64_t)((double)t * alpha));
    }
    __syncthreads();  // every take before every add
    walk_rows(
        a, fl, m, [&](int64_t q) { return (double)w.take[q]; },
        [&](double t, int64_t e) {
          const int64_t j = a.col[e];
          const int64_t add = (int64_t)((t * (double)a.val[e]) * beta);
          if (j < 0 || j >= n) return;  // never with a graph this library built
          const int64_t old = fetch_add(w.r + j, add);
          const int64_t th = a.thr ? a.thr[j] : thr_rw;
          if (old < th && old + add >= th) {
            const int pos = atomicAdd(&cnt[cur ^ 1], 1);
            if (pos < n) nl[pos] = (int32_t)j;
          }
        });
    __syncthreads();
    cur ^= 1;
    ++round;
  }
  return {round, m};
}

__global__ __launch_bounds__(kPushBlock) void k_push(PushArgs a) {
  const int64_t c = blockIdx.x;
  const int64_t s = a.core.sources[c];
  if (s < 0 || s >= a.core.n) {  // whole workgroup: the column stays zero
    report(a.core, c, 0, -1);
    return;
  }
  const PushEnd end = push_rounds(a.core, s, slab(a.core, c, kPushLists), [](int64_t) {});
  report(a.core, c, end.rounds, end.left);
}

// X[j, c] = (float)(p[c][j] 2^-44): a 32 x 32 tile through LDS, reads along j, writes along c
__global__ __launch_bounds__(kBlock) void k_push_emit(PushArgs a) {
  __shared__ int64_t tile[kEmitTile][kEmitTile + 1];
  const int64_t n = a.core.n, b = a.core.b;
  const int64_t jt = (int64_t)blockIdx.x * kEmitTile, ct = (int64_t)blockIdx.y * kEmitTile;
  const int lx = threadIdx.x & (kEmitTile - 1), ly = threadIdx.x / kEmitTile;
  for (int y = ly; y < kEmitTile; y += kBlock / kEmitTile) {
    const int64_t c = ct + y, j = jt + lx;
    if (c < b && j < n) tile[y][lx] = a.core.p[c * n + j];
  }
  __syncthreads();
  for (int y = ly; y < kEmitTile; y += kBlock / kEmitTile) {
    const int64_t j = jt + y, c = ct + lx;
    if (c < b && j < n) a.x[j * a.ld_x + c] = (float)((double)tile[lx][y] * kUnit);
  }
}

// ---- appnp_push_topk: the push, then the top k straight from the list of taken nodes ----------
//
// A grid of SLOTS: workgroup w runs the sources w, w + slots, ... one after another on its own
// slab of the workspace (r, p, take as int64 [n], two frontier lists and the list of the distinct
// nodes taken so far as int32 [n]).  Per source:
//   push     push_rounds; the take phase also sets kSeen in p_i (fetch_or) and the one thread that
//            found it unset appends i to the taken list: once per node, whatever the increments
//            of p_i truncate to
//   keys     per taken node the candidate v = ((float)(p 2^-44) * row_scale) * col_scale and, when
//            v > 0, the composite key order_key(v) << 32 | ~i (all distinct: the tie rule is part
//            of the key), written over the take slab; 0 otherwise
//   select   with more than k positive candidates, a radix select in LDS (8 bits per pass from the
//            top; it stops at the first digit whose bin holds exactly what is still wanted) finds
//            T with exactly k keys >= T; otherwise every positive candidate wins (T = 1)
//   emit     winners compacted into LDS; a short row is filled with +0.0 at the smallest indices
//            of [0, k) that hold no winner (flags over [0, k) and a scan); every entry's place is
//            the number of entries with a smaller index
//   clean    r_j = 0 over the rows of the taken nodes, p_i = r_i = 0 of those nodes (a thread per
//            node, after the walk: a store ahead of a row's loads would be waited for with them,
//            vmcnt counts both), r_s = 0: every
//            nonzero of the slot, at the cost of one more walk of what the push walked (skipped
//            after a slot's last source: every call starts with a clear of r and p)
// r and p are accessed by relaxed agent-scope atomics only (a slot is reused inside one launch; a
// plain load could hit a line cached from the source before).  Lists, takes and keys are plain
// stores read after a workgroup barrier.  No workgroup waits for or reads from another one.

constexpr int kTopkCap = kPushBlock;          // k <= 1024: a thread per output entry
constexpr int64_t kSeen = (int64_t)1 << 62;   // in p_i: node i is on the taken list (p < 2^45)

struct PushTopkArgs {
  PushCore core;
  const float* row_scale;  // [n] or null
  const float* col_scale;  // [b] or null
  int k;
  int32_t* out_idx;
  float* out_val;
  int64_t ld_out;
};

__global__ __launch_bounds__(kPushBlock) void k_push_topk(PushTopkArgs a) {
  __shared__ int ntaken, npos, nwin;
  __shared__ uint32_t hist[256];
  __shared__ uint32_t pick[3];  // the digit found, the keys above its bin, the keys in its bin
  __shared__ int wsum[kPushWaves];
  __shared__ int32_t widx[kTopkCap];
  __shared__ float wval[kTopkCap];
  __shared__ int flag[kTopkCap];
  const PushCore& core = a.core;
  const int64_t n = core.n;
  const int k = a.k;
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid >> 6;
  const PushSlab w = slab(core, blockIdx.x, kTopkLists);
  int32_t* taken = w.list + 2 * n;
  uint64_t* keys = reinterpret_cast<uint64_t*>(w.take);

  for (int64_t c = blockIdx.x; c < core.b; c += gridDim.x) {
    const int64_t s = core.sources[c];
    const bool valid = s >= 0 && s < n;
    if (tid == 0) {
      ntaken = 0;
      npos = 0;
      nwin = 0;
    }
    if (tid < k) flag[tid] = 0;

    // ---- push: the take phase records a node the first time it is taken
    const PushEnd end = push_rounds(core, s, w, [&](int64_t i) {
      const int64_t seen =
          __hip_atomic_fetch_or(w.p + i, kSeen, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (!(seen & kSeen)) {  // exactly one thread per node, ever: at most n appends
        const int pos = atomicAdd(&ntaken, 1);
        if (pos < n) taken[pos] = (int32_t)i;
      }
    });
    report(core, c, end.rounds, valid ? end.left : -1);
    const int64_t L = std::min<int64_t>((int64_t)ntaken, n);

    // ---- keys: over the take slab, which the push no longer reads
    {
      const bool has_cs = a.col_scale != nullptr;
      const float cs = has_cs ? a.col_scale[c] : 1.0f;
      for (int64_t q0 = 0; q0 < L; q0 += kPushBlock) {  // whole waves: the ballot below
        const int64_t q = q0 + tid;
        bool positive = false;
        if (q < L) {
          const int64_t i = taken[q];
          const int64_t pv = load_i64(w.p + i) & ~kSeen;
          float v = (float)((double)pv * kUnit);
          if (a.row_scale) v = v * a.row_scale[i];
          if (has_cs) v = v * cs;
          const uint32_t key = order_key(v);
          positive = key > kOrderKeyZero;
          keys[q] = positive ? ((uint64_t)key << 32) | (uint64_t)(~(uint32_t)i) : 0ull;
        }
        const unsigned long long mask = __ballot(positive);
        if (lane == 0 && mask) atomicAdd(&npos, __popcll(mask));
      }
    }
    __syncthreads();

    // ---- select: T with exactly min(k, positives) keys >= T
    uint64_t T = 1ull;
    if (npos > k) {
      uint64_t prefix = 0ull;
      uint32_t want = (uint32_t)k;
      for (int pass = 0; pass < 8; ++pass) {
        const int shift = 56 - 8 * pass;
        if (tid < 256) hist[tid] = 0u;
        __syncthreads();
        for (int64_t q = tid; q < L; q += kPushBlock) {
          const uint64_t key = keys[q];
          const bool match = pass == 0 || ((key ^ prefix) >> ((shift + 8) & 63)) == 0ull;
          if (match) atomicAdd(&hist[(uint32_t)(key >> shift) & 255u], 1u);
        }
        __syncthreads();
        if (wave == 0) {  // the digit in which the want-th largest matching key lies
          uint32_t digit, above, in;
          if (digit_search(hist[4 * lane], hist[4 * lane + 1], hist[4 * lane + 2],
                           hist[4 * lane + 3], want, lane, digit, above, in)) {  // exactly one lane
            pick[0] = digit;
            pick[1] = above;
            pick[2] = in;
          }
        }
        __syncthreads();
        prefix |= (uint64_t)pick[0] << shift;
        want -= pick[1];
        // keys are distinct: by the last pass the bin holds one key and one is wanted
        if (pick[2] == want) break;  // the whole bin wins
      }
      T = prefix;
    }

    // ---- emit: winners into LDS, the padding of a short row, places by index
    for (int64_t q = tid; q < L; q += kPushBlock) {
      const uint64_t key = keys[q];
      if (key >= T) {
        const int pos = atomicAdd(&nwin, 1);
        if (pos < k) {  // holds by construction; the guard keeps the store in bounds
          const uint32_t j = ~(uint32_t)key;
          widx[pos] = (int32_t)j;
          wval[pos] = __uint_as_float((uint32_t)(key >> 32) & 0x7fffffffu);  // v > 0
          if (j < (uint32_t)k) flag[j] = 1;
        }
      }
    }
    __syncthreads();
    const int nw = std::min(nwin, k);
    if (nw < k) {  // the k - nw smallest indices of [0, k) without a winner, value +0.0
      const bool free_j = tid < k && flag[tid] == 0;
      const unsigned long long mask = __ballot(free_j);
      if (lane == 0) wsum[wave] = __popcll(mask);
      __syncthreads();
      int zr = __popcll(mask & ((1ull << lane) - 1ull));
      for (int u = 0; u < wave; ++u) zr += wsum[u];
      if (free_j && zr < k - nw) {
        widx[nw + zr] = tid;
        wval[nw + zr] = 0.0f;
      }
      __syncthreads();
    }
    if (tid < k) {
      const int32_t mine = widx[tid];
      int rank = 0;
      for (int u = 0; u < k; ++u) rank += widx[u] < mine ? 1 : 0;
      a.out_idx[c * a.ld_out + rank] = mine;
      a.out_val[c * a.ld_out + rank] = wval[tid];
    }

    // ---- clean the slot: the rows of the taken nodes hold every nonzero of r.  Not after the
    // slot's last source: the next call clears r and p itself
    if (c + gridDim.x < core.b) {
      walk_rows(
          core, taken, L, [](int64_t) { return 0; },
          [&](int, int64_t e) {
            const int64_t j = core.col[e];
            if (j >= 0 && j < n) store_i64(w.r + j, 0);
          });
      for (int64_t q = tid; q < L; q += kPushBlock) {  // p_i, and r_i of a row without a self loop
        const int64_t i = taken[q];
        store_i64(w.p + i, 0);
        store_i64(w.r + i, 0);
      }
      if (tid == 0 && valid) store_i64(w.r + s, 0);  // a source that ran no round
    }
    __syncthreads();  // the slot and the LDS state are free for the next source
  }
}

// The workspace of both entry points, as byte offsets: the n thresholds at 0, then r, p and take
// as int64 [slabs][n] and `lists` int32 lists of capacity n per slab.  r starts 256-byte aligned
// and p follows it directly: one clear covers both.
struct PushLayout {
  size_t r, p, take, lists, bytes;
};

inline PushLayout push_layout(int64_t n, int64_t slabs, int lists) {
  const size_t cells = (size_t)n * (size_t)slabs;
  PushLayout l;
  l.r = round_up((size_t)n * sizeof(int64_t), 256);
  l.p = l.r + cells * sizeof(int64_t);
  l.take = l.p + cells * sizeof(int64_t);
  l.lists = l.take + cells * sizeof(int64_t);
  l.bytes = round_up(l.lists + (size_t)lists * cells * sizeof(int32_t), 256);
  return l;
}

inline size_t push_bytes(int64_t n, int64_t slabs, int lists) {
  if (n <= 0 || slabs <= 0 || n > INT32_MAX) return 0;
  return push_layout(n, slabs, lists).bytes;
}

// A call of either entry point up to its own launches: the checks (in the order of refusals
// include/ppnp_amd.h states), A_hat or A_hat^T, the workspace, the clear and the thresholds.
//   a          the core as the entry point filled it: sources, b, alpha, eps, max_rounds, rounds,
//              left; the rest is set here
//   args_ok    its own argument checks that precede the return for an empty call
//   outs_ok    ... and those that follow it, with n >= min_n (all APPNP_EINVAL)
//   ws_slabs   the slabs `ws` must hold; `slabs` of them are used, of `lists` lists each
//   last(n)    its refusal after the graph checks, or APPNP_OK
//   run(s)     its launches
template <typename Last, typename Run>
int push_call(const appnp_graph* g, PushCore& a, bool args_ok, bool outs_ok, int64_t min_n,
              void* ws, size_t ws_bytes, int64_t ws_slabs, int64_t slabs, int lists, void* stream,
              Last last, Run run) {
  if (!g || a.b < 0 || a.max_rounds < 1 || !args_ok) return APPNP_EINVAL;
  if (!(a.alpha > 0.0f && a.alpha <= 1.0f) || !(a.eps > 0.0f && a.eps < 1.0f)) return APPNP_EINVAL;
  if (a.b == 0 || g->n == 0) return APPNP_OK;
  const int64_t n = g->n;
  if (n < min_n || !a.sources || !outs_ok || !ws || n > INT32_MAX) return APPNP_EINVAL;
  if (ws_bytes < push_bytes(n, ws_slabs, lists)) return APPNP_EINVAL;
  if (reinterpret_cast<uintptr_t>(ws) % 16 != 0) return APPNP_EINVAL;
  if (g->row_lo != 0 || g->row_hi != n) return APPNP_ENOTSUP;  // needs the whole graph
  if (!g->symmetric) return APPNP_ENOTSUP;
  const bool sym = g->mode == APPNP_NORM_SYM;
  if (!sym && !g->t_row_ptr) return APPNP_ENOTSUP;  // rw: the columns of A_hat are rows of A_hat^T
  int rc = last(n);
  if (rc != APPNP_OK) return rc;

  a.row_ptr = sym ? g->row_ptr : g->t_row_ptr;
  a.col = sym ? g->col : g->t_col;
  a.val = sym ? g->val : g->t_val;
  a.n = n;
  a.beta = 1.0f - a.alpha;
  char* base = static_cast<char*>(ws);
  const PushLayout l = push_layout(n, slabs, lists);
  int64_t* thr = reinterpret_cast<int64_t*>(base);
  a.thr = sym ? thr : nullptr;
  a.r = reinterpret_cast<int64_t*>(base + l.r);
  a.p = reinterpret_cast<int64_t*>(base + l.p);
  a.take = reinterpret_cast<int64_t*>(base + l.take);
  a.lists = reinterpret_cast<int32_t*>(base + l.lists);
  hipStream_t s = static_cast<hipStream_t>(stream);

  // one clear of r and p per call, by a kernel (a captured memset node is not relied on,
  // DESIGN.md 4.7): 2 n slabs int64 = n slabs 16-byte stores
  const int64_t n16 = n * slabs;
  const unsigned clear_grid = (unsigned)std::min<int64_t>((n16 + kBlock - 1) / kBlock, 1 << 16);
  rc = timed_launch(s, APPNP_KT_COPY, [&] {
    hipLaunchKernelGGL(k_push_clear, dim3(clear_grid), dim3(kBlock), 0, s,
                       reinterpret_cast<ulonglong2*>(a.r), n16);
  });
  if (rc == APPNP_OK && sym)
    rc = timed_launch(s, APPNP_KT_COPY, [&] {
      hipLaunchKernelGGL(k_push_thr, dim3((unsigned)((n + kBlock - 1) / kBlock)), dim3(kBlock), 0,
                         s, g->dinv, n, a.eps, thr);
    });
  return rc == APPNP_OK ? run(s) : rc;
}

inline PushCore push_core(const int64_t* sources, int64_t b, float alpha, float eps,
                          int max_rounds, int32_t* rounds, int32_t* left) {
  PushCore c{};
  c.sources = sources;
  c.b = b;
  c.alpha = alpha;
  c.eps = eps;
  c.max_rounds = max_rounds;
  c.rounds = rounds;
  c.left = left;
  return c;
}

}  // namespace
}  // namespace appnp

extern "C" size_t appnp_push_workspace_bytes(int64_t n, int64_t b) {
  return appnp::push_bytes(n, b, appnp::kPushLists);
}

extern "C" int appnp_push_columns(const appnp_graph* g, const int64_t* sources, int64_t b,
                                  float alpha, float eps, int max_rounds, float* X, int64_t ld_x,
                                  int32_t* rounds, int32_t* left, void* ws, size_t ws_bytes,
                                  void* stream) {
  using namespace appnp;
  PushArgs a{push_core(sources, b, alpha, eps, max_rounds, rounds, left), X, ld_x};
  int64_t jt = 0, ct = 0;  // the tiles of the emit launch
  return push_call(
      g, a.core, ld_x >= b, X && b <= INT32_MAX, 0, ws, ws_bytes, b, b, kPushLists, stream,
      [&](int64_t n) {
        jt = (n + kEmitTile - 1) / kEmitTile;
        ct = (b + kEmitTile - 1) / kEmitTile;
        // grid.y, and HIP bounds a grid's threads by 2^32
        const bool fits = ct <= 65535 && jt * ct <= (((int64_t)1 << 32) - 1) / kBlock;
        return fits ? APPNP_OK : APPNP_ERANGE;
      },
      [&](hipStream_t s) {
        int rc = timed_launch(s, APPNP_KT_PUSH, [&] {
          hipLaunchKernelGGL(k_push, dim3((unsigned)b), dim3(kPushBlock), 0, s, a);
        });
        if (rc == APPNP_OK)
          rc = timed_launch(s, APPNP_KT_COPY, [&] {
            hipLaunchKernelGGL(k_push_emit, dim3((unsigned)jt, (unsigned)ct), dim3(kBlock), 0, s,
                               a);
          });
        return rc;
      });
}

extern "C" size_t appnp_push_topk_workspace_bytes(int64_t n, int slots) {
  return appnp::push_bytes(n, slots, appnp::kTopkLists);
}

extern "C" int appnp_push_topk(const appnp_graph* g, const int64_t* sources, int64_t b,
                               float alpha, float eps, int max_rounds, int k,
                               const float* row_scale, const float* col_scale, int32_t* out_idx,
                               float* out_val, int64_t ld_out, int32_t* rounds, int32_t* left,
                               int slots, void* ws, size_t ws_bytes, void* stream) {
  using namespace appnp;
  static_assert(APPNP_PUSH_TOPK_MAX_K == kTopkCap, "the header states the kernel's cap");
  PushTopkArgs a{push_core(sources, b, alpha, eps, max_rounds, rounds, left),
                 row_scale, col_scale, k, out_idx, out_val, ld_out};
  // more slots than sources would only be cleared: the grid is what the sources can fill, and
  // every source leaves its slot clean
  const int64_t used = std::min<int64_t>(slots, b);
  return push_call(
      g, a.core, k >= 1 && ld_out >= k && slots >= 1, out_idx && out_val, k, ws, ws_bytes, slots,
      used, kTopkLists, stream,
      [&](int64_t) { return k > APPNP_PUSH_TOPK_MAX_K ? APPNP_ENOTSUP : APPNP_OK; },
      [&](hipStream_t s) {
        return timed_launch(s, APPNP_KT_PUSH, [&] {
          hipLaunchKernelGGL(k_push_topk, dim3((unsigned)used), dim3(kPushBlock), 0, s, a);
        });
      });
}
