// appnp_batch.hip -- the per-minibatch slice of a sparse PPR matrix, transpose included (gfx950).
//
// batch-main.py:140-142 on a CSR P: ppr_sub = ppr[idx]; sel = (ppr_sub > 0).any(dim=0);
// ppr_sub[:, sel].  appnp_csr_batch_count / appnp_csr_batch_emit produce the [b x |sel|] CSR with
// its columns relabelled into sel, sel itself, and the canonical CSR of the transpose (what
// appnp_csr_transpose returns for the sub-matrix, bit for bit), with ONE read-back between the
// two calls: the 24 bytes of `counts`, from which the caller sizes the outputs.  DESIGN.md 4.9.
//
// The chains on `stream` (a wave per taken row wherever rows are walked):
//
//   count:  memset    the cols-bit bitmap and the out-of-range counter
//           mark      atomicOr of the column bit of every taken entry with val > 0 (up to
//                     APPNP_CSR_BATCH_LDS_COLS columns: gathered in LDS per workgroup first)
//           rows      per taken row: entries whose column bit is set
//           scan      one workgroup: exclusive scan of popcount over the bitmap words (each word's
//                     base rank, |sel|), exclusive scan of the row counts (out_indptr), counts[]
//   emit:   sel       per bitmap word: the set bits' column ids at base + popcount(lower bits);
//                     clears t_indptr
//           emit      stable in-row compaction (ballot + mbcnt) into out_indices / out_vals, the new
//                     column = base[word] + popcount(word & lower mask); counts each new column
//                     into t_indptr by integer atomics
//           tscan     one workgroup: t_indptr from the column counts; clears the cursors
//           scatter   every kept entry e (its index in out_indices) to its column's segment
//                     through an atomic cursor, with its row p
//           sort      each segment into ascending e: rank by counting, a wave per short segment
//                     (shuffles), the workgroup per long one (keys staged in LDS)
//
// e ascends with (p, position in the row), and it is unique, so the sorted segment does not depend
// on the order the cursor atomics took: integer atomics only, two runs give the same bits.  The
// phases are separate launches and the scans single-workgroup loops: no workgroup ever waits for
// another.  Per batch the work follows the taken entries plus cols / 32 words.
//
// Every index the kernels form is checked before it is used: a row outside [0, rows) is an empty
// row (and counted), a column outside [0, cols) is never selected, and every store is guarded by
// the size of its output, so a caller that passes sizes other than those `counts` reported gets
// unspecified values, never an access outside its buffers.
//
// appnp_csr_rows_count / appnp_csr_rows_emit take whole rows of a CSR, M[idx],
// with no column selected or relabelled: count is ONE single-workgroup launch (lengths from indptr,
// their scan, the out-of-range count: no workspace, nothing to clear), emit a wave-per-row copy
// and, for the transpose, a clear of t_indptr before it and tscan, scatter and sort after it, over
// all cols columns.
#include <algorithm>

#include "appnp_internal.h"
#include "../../include/ppnp_amd.h"

namespace appnp {
namespace {

constexpr int kScanThreads = 1024;
constexpr int kScanItems = APPNP_CSR_BATCH_SCAN_PASS / kScanThreads;  // per thread and pass
constexpr int kScanWaves = kScanThreads / kWave;
static_assert(kScanItems * kScanThreads == APPNP_CSR_BATCH_SCAN_PASS, "whole items per thread");
constexpr int kMarkLdsWords = APPNP_CSR_BATCH_LDS_COLS / 32;  // mark: the bitmap gathered in LDS
constexpr int kMarkRows = 8;                   // ... of this many taken rows per wave
constexpr int kSegsPerBlock = kWavesPerBlock;  // sort: a wave per segment
constexpr int kSortOwn = 4;                    // long segments: keys a thread ranks per chunk
constexpr int kSortTile = kSortOwn * kBlock;   // ... and keys staged in LDS at a time

struct BatchArgs {
  const int32_t* indptr;
  const int32_t* indices;
  const float* vals;
  int64_t rows, cols;
  const int64_t* idx;
  int64_t b;
  int64_t words;       // bitmap words
  int64_t nnz_out, n_sel;
  // workspace
  unsigned long long* oob;  // indices outside [0, rows)
  uint32_t* bitmap;    // [words]
  uint32_t* rank;      // [words] selected columns below the word
  uint32_t* rowcnt;    // [b] kept entries per taken row
  uint32_t* cursor;    // [n_sel]
  int32_t* tkey;       // [nnz_out] the entry e of each transpose slot, unsorted inside a segment
  int32_t* trow;       // [nnz_out] ... and its row p
  // outputs
  int32_t* out_indptr;
  int64_t* counts;
  int32_t* out_indices;
  float* out_vals;
  int64_t* sel;
  int32_t* t_indptr;
  int32_t* t_indices;
  float* t_vals;
};

// Entries [s, e) of taken row p; false (an empty row) for an index outside [0, rows).
__device__ __forceinline__ bool taken_row(const BatchArgs& a, int64_t p, int32_t& s, int32_t& e,
                                          bool& in_range) {
  const int64_t r = a.idx[p];
  in_range = r >= 0 && r < a.rows;
  if (!in_range || !a.indices || !a.vals) return false;
  s = a.indptr[r];
  e = a.indptr[r + 1];
  return s >= 0 && e > s;
}

__device__ __forceinline__ bool col_selected(const BatchArgs& a, int32_t j) {
  return j >= 0 && j < a.cols && ((a.bitmap[j >> 5] >> (j & 31)) & 1u) != 0u;
}

// kLds: the bitmap fits kMarkLdsWords words, and the taken rows share most of their columns (a
// small matrix has few words for all of them: atomics from every wave on the same few lines).  A
// workgroup then gathers the bits of kMarkRows rows per wave in LDS and merges the words that are
// not empty; otherwise a wave per row marks the global bitmap directly.
template <bool kLds>
__global__ __launch_bounds__(kBlock) void k_batch_mark(BatchArgs a) {
  __shared__ uint32_t lbits[kLds ? kMarkLdsWords : 1];
  const int lane = threadIdx.x & (kWave - 1);
  constexpr int per = kLds ? kMarkRows : 1;
  if (kLds) {
    for (int i = threadIdx.x; i < a.words; i += kBlock) lbits[i] = 0u;
    __syncthreads();
  }
  const int64_t p0 = ((int64_t)blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6)) * per;
  for (int64_t p = p0; p < std::min<int64_t>(a.b, p0 + per); ++p) {  // wave-uniform
    int32_t s = 0, e = 0;
    bool in_range;
    const bool any = taken_row(a, p, s, e, in_range);
    if (!in_range && lane == 0) atomicAdd(a.oob, 1ull);
    if (!any) continue;
    for (int64_t q = (int64_t)s + lane; q < e; q += kWave) {
      const int32_t j = a.indices[q];
      if (!(a.vals[q] > 0.0f) || j < 0 || j >= a.cols) continue;
      const uint32_t bit = 1u << (j & 31);
      if (kLds) {
        atomicOr(&lbits[j >> 5], bit);
      } else {
        // a bit that is seen set needs no atomic; a stale word only costs the atomic it would
        // have saved
        uint32_t* word = &a.bitmap[j >> 5];
        if ((*word & bit) == 0u) atomicOr(word, bit);
      }
    }
  }
  if (kLds) {
    __syncthreads();
    for (int i = threadIdx.x; i < a.words; i += kBlock) {
      const uint32_t x = lbits[i];
      if (x != 0u && (x & ~a.bitmap[i]) != 0u) atomicOr(&a.bitmap[i], x);
    }
  }
}

__global__ __launch_bounds__(kBlock) void k_batch_rows(BatchArgs a) {
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t p = (int64_t)blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6);
  if (p >= a.b) return;  // whole wave
  int32_t s = 0, e = 0;
  bool in_range;
  uint32_t cnt = 0;
  if (taken_row(a, p, s, e, in_range)) {
    for (int64_t q0 = s; q0 < e; q0 += kWave) {  // wave-uniform trip count
      const int64_t q = q0 + lane;
      const bool keep = q < e && col_selected(a, a.indices[q]);
      cnt += (uint32_t)__popcll(__ballot(keep));
    }
  }
  if (lane == 0) a.rowcnt[p] = cnt;
}

// Exclusive scan of load(i), i < n, by one workgroup of kScanThreads threads, a pass of
// APPNP_CSR_BATCH_SCAN_PASS items at a time: store(i, sum of the items before i, item i).  Returns
// the total (to every thread).  wsum: kScanWaves words of LDS.
template <typename Load, typename Store>
__device__ __forceinline__ unsigned long long scan_loop(int64_t n, unsigned long long* wsum,
                                                        Load load, Store store) {
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x >> 6;
  unsigned long long carry = 0;
  for (int64_t base = 0; base < n; base += APPNP_CSR_BATCH_SCAN_PASS) {  // uniform trip count
    const int64_t i0 = base + (int64_t)threadIdx.x * kScanItems;
    uint32_t v[kScanItems];
    unsigned long long own = 0;
#pragma unroll
    for (int u = 0; u < kScanItems; ++u) {
      v[u] = i0 + u < n ? load(i0 + u) : 0u;
      own += v[u];
    }
    unsigned long long inc = own;  // inclusive over the wave's lanes
#pragma unroll
    for (int off = 1; off < kWave; off <<= 1) {
      const unsigned long long t = __shfl_up(inc, off, kWave);
      if (lane >= off) inc += t;
    }
    if (lane == kWave - 1) wsum[wave] = inc;
    __syncthreads();
    unsigned long long before = 0, total = 0;
#pragma unroll
    for (int w = 0; w < kScanWaves; ++w) {
      const unsigned long long x = wsum[w];
      total += x;
      before += w < wave ? x : 0ull;
    }
    unsigned long long ex = carry + before + (inc - own);
#pragma unroll
    for (int u = 0; u < kScanItems; ++u)
      if (i0 + u < n) {
        store(i0 + u, ex, v[u]);
        ex += v[u];
      }
    carry += total;
    __syncthreads();  // wsum is rewritten by the next pass
  }
  return carry;
}

__global__ __launch_bounds__(kScanThreads) void k_batch_scan(BatchArgs a) {
  __shared__ unsigned long long wsum[kScanWaves];
  const unsigned long long n_sel = scan_loop(
      a.words, wsum, [&](int64_t i) { return (uint32_t)__popc(a.bitmap[i]); },
      [&](int64_t i, unsigned long long ex, uint32_t) { a.rank[i] = (uint32_t)ex; });
  const unsigned long long nnz = scan_loop(
      a.b, wsum, [&](int64_t i) { return a.rowcnt[i]; },
      [&](int64_t i, unsigned long long ex, uint32_t) { a.out_indptr[i] = (int32_t)ex; });
  if (threadIdx.x == 0) {
    a.out_indptr[a.b] = (int32_t)nnz;  // the caller refuses nnz >= 2^31 from counts[0]
    a.counts[0] = (int64_t)nnz;
    a.counts[1] = (int64_t)n_sel;
    a.counts[2] = (int64_t)*a.oob;
  }
}

__global__ __launch_bounds__(kBlock) void k_batch_sel(BatchArgs a) {
  const int64_t w = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  const int64_t stride = (int64_t)gridDim.x * kBlock;
  for (int64_t i = w; i <= a.n_sel; i += stride) a.t_indptr[i] = 0;  // the column counts
  if (w >= a.words) return;
  uint32_t bits = a.bitmap[w];
  int64_t r = a.rank[w];
  while (bits != 0u && r < a.n_sel) {
    const int bit = __ffs(bits) - 1;
    a.sel[r++] = w * 32 + bit;
    bits &= bits - 1u;
  }
}

__global__ __launch_bounds__(kBlock) void k_batch_emit(BatchArgs a) {
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t p = (int64_t)blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6);
  if (p >= a.b) return;  // whole wave
  int32_t s = 0, e = 0;
  bool in_range;
  if (!taken_row(a, p, s, e, in_range)) return;
  int64_t base = a.out_indptr[p];
  for (int64_t q0 = s; q0 < e; q0 += kWave) {  // wave-uniform trip count
    const int64_t q = q0 + lane;
    int32_t j = -1;
    if (q < e) j = a.indices[q];
    const bool keep = q < e && col_selected(a, j);
    const unsigned long long m = __ballot(keep);
    const uint32_t before = __builtin_amdgcn_mbcnt_hi(
        (uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
    if (keep) {
      const uint32_t word = a.bitmap[j >> 5];
      const int64_t c = (int64_t)a.rank[j >> 5] + __popc(word & ((1u << (j & 31)) - 1u));
      const int64_t pos = base + before;
      if (pos >= 0 && pos < a.nnz_out && c < a.n_sel) {
        a.out_indices[pos] = (int32_t)c;
        a.out_vals[pos] = a.vals[q];
        atomicAdd(reinterpret_cast<uint32_t*>(&a.t_indptr[c + 1]), 1u);
      }
    }
    base += __popcll(m);
  }
}

__global__ __launch_bounds__(kScanThreads) void k_batch_tscan(BatchArgs a) {
  __shared__ unsigned long long wsum[kScanWaves];
  // in place: a thread reads the counts of its own items, then writes the same elements
  scan_loop(
      a.n_sel, wsum, [&](int64_t i) { return (uint32_t)a.t_indptr[i + 1]; },
      [&](int64_t i, unsigned long long ex, uint32_t v) {
        a.t_indptr[i + 1] = (int32_t)(ex + v);
        a.cursor[i] = 0u;
      });
}

__global__ __launch_bounds__(kBlock) void k_batch_scatter(BatchArgs a) {
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t p = (int64_t)blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6);
  if (p >= a.b) return;  // whole wave
  const int64_t s = std::max<int64_t>(0, a.out_indptr[p]);
  const int64_t e = std::min<int64_t>(a.nnz_out, a.out_indptr[p + 1]);
  for (int64_t q = s + lane; q < e; q += kWave) {
    const int64_t c = a.out_indices[q];
    if (c < 0 || c >= a.n_sel) continue;
    const int64_t slot = (int64_t)a.t_indptr[c] + atomicAdd(&a.cursor[c], 1u);
    if (slot >= 0 && slot < a.t_indptr[c + 1] && slot < a.nnz_out) {
      a.tkey[slot] = (int32_t)q;
      a.trow[slot] = (int32_t)p;
    }
  }
}

// Segment c of the transpose: slots [s, s + len); false when it is empty or does not fit.
__device__ __forceinline__ bool segment(const BatchArgs& a, int64_t c, int64_t& s, int64_t& len) {
  if (c >= a.n_sel) return false;
  s = a.t_indptr[c];
  len = (int64_t)a.t_indptr[c + 1] - s;
  return s >= 0 && len > 0 && s + len <= a.nnz_out;
}

__device__ __forceinline__ void put_sorted(const BatchArgs& a, int64_t slot, int32_t key,
                                           int32_t row) {
  a.t_indices[slot] = row;
  a.t_vals[slot] = key >= 0 && key < a.nnz_out ? a.out_vals[key] : 0.0f;
}

__global__ __launch_bounds__(kBlock) void k_batch_sort(BatchArgs a) {
  __shared__ __attribute__((aligned(16))) int32_t tile[kSortTile];
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x >> 6;
  const int64_t c0 = (int64_t)blockIdx.x * kSegsPerBlock;
  {  // segments of up to a wave's length: the rank of a key is the number of smaller keys
    int64_t s, len;
    if (segment(a, c0 + wave, s, len) && len <= kWave) {  // wave-uniform
      const bool mine = lane < len;
      const int32_t key = mine ? a.tkey[s + lane] : INT32_MAX;
      const int32_t row = mine ? a.trow[s + lane] : 0;
      int rank = 0;
      for (int j = 0; j < (int)len; ++j) rank += __shfl(key, j, kWave) < key ? 1 : 0;
      if (mine) put_sorted(a, s + rank, key, row);
    }
  }
  for (int g = 0; g < kSegsPerBlock; ++g) {  // longer ones: the whole workgroup, keys through LDS
    int64_t s, len;
    if (!segment(a, c0 + g, s, len) || len <= kWave) continue;  // workgroup-uniform
    for (int64_t own0 = 0; own0 < len; own0 += kSortTile) {
      int32_t key[kSortOwn], row[kSortOwn];
      int rank[kSortOwn];
#pragma unroll
      for (int u = 0; u < kSortOwn; ++u) {
        const int64_t i = own0 + u * kBlock + threadIdx.x;
        key[u] = i < len ? a.tkey[s + i] : INT32_MAX;
        row[u] = i < len ? a.trow[s + i] : 0;
        rank[u] = 0;
      }
      for (int64_t t0 = 0; t0 < len; t0 += kSortTile) {
        __syncthreads();  // the tile of the step before has been read
#pragma unroll
        for (int u = 0; u < kSortOwn; ++u) {
          const int64_t i = t0 + u * kBlock + threadIdx.x;
          tile[u * kBlock + threadIdx.x] = i < len ? a.tkey[s + i] : INT32_MAX;
        }
        __syncthreads();
        const int n4 = (int)((std::min<int64_t>(kSortTile, len - t0) + 3) / 4);
        const int4* t4 = reinterpret_cast<const int4*>(tile);
        for (int j = 0; j < n4; ++j) {  // every lane reads the same 16 bytes: a broadcast
          const int4 k = t4[j];
#pragma unroll
          for (int u = 0; u < kSortOwn; ++u)
            rank[u] += (k.x < key[u] ? 1 : 0) + (k.y < key[u] ? 1 : 0) + (k.z < key[u] ? 1 : 0) +
                       (k.w < key[u] ? 1 : 0);
        }
      }
#pragma unroll
      for (int u = 0; u < kSortOwn; ++u) {
        const int64_t i = own0 + u * kBlock + threadIdx.x;
        if (i < len && rank[u] < len) put_sorted(a, s + rank[u], key[u], row[u]);
      }
    }
    __syncthreads();  // before the next segment restages the tile
  }
}

// ---- whole rows of a CSR (appnp_csr_rows_count / _emit) ----------------------
// The same BatchArgs with n_sel = cols (no column is relabelled), so that tscan, scatter and sort
// above serve its transpose unchanged.

// Entries of taken row p as indptr gives them; an index outside [0, rows) adds to `oob`.
__device__ __forceinline__ uint32_t taken_len(const BatchArgs& a, int64_t p,
                                              unsigned long long& oob) {
  int32_t s = 0, e = 0;
  bool in_range;
  const bool any = taken_row(a, p, s, e, in_range);
  oob += in_range ? 0ull : 1ull;
  return any ? (uint32_t)((int64_t)e - s) : 0u;
}

// One workgroup: the row lengths from indptr, their exclusive scan (out_indptr) and the indices
// outside [0, rows), with no state in memory before it: nothing to clear.
__global__ __launch_bounds__(kScanThreads) void k_rows_count(BatchArgs a) {
  __shared__ unsigned long long wsum[kScanWaves];
  __shared__ unsigned long long oob_all;
  if (threadIdx.x == 0) oob_all = 0ull;
  unsigned long long oob = 0;  // of the rows this thread loads
  const unsigned long long nnz = scan_loop(
      a.b, wsum, [&](int64_t i) { return taken_len(a, i, oob); },
      [&](int64_t i, unsigned long long ex, uint32_t) {
        a.out_indptr[i] = (int32_t)std::min<unsigned long long>(ex, INT32_MAX);
      });
  if (oob != 0ull) atomicAdd(&oob_all, oob);  // after scan_loop's barriers: oob_all is zero
  __syncthreads();
  if (threadIdx.x == 0) {
    a.out_indptr[a.b] = (int32_t)std::min<unsigned long long>(nnz, INT32_MAX);
    a.counts[0] = (int64_t)nnz;  // the caller refuses nnz >= 2^31
    a.counts[1] = (int64_t)oob_all;
  }
}

__global__ __launch_bounds__(kBlock) void k_rows_clear(BatchArgs a) {
  const int64_t stride = (int64_t)gridDim.x * kBlock;
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i <= a.cols; i += stride)
    a.t_indptr[i] = 0;  // the column counts
}

// A wave per taken row: the row as it is.  kT: also counts each entry's column into t_indptr; an
// entry whose column lies outside [0, cols) is copied and not counted (scatter skips it too).
template <bool kT>
__global__ __launch_bounds__(kBlock) void k_rows_copy(BatchArgs a) {
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t p = (int64_t)blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6);
  if (p >= a.b) return;  // whole wave
  int32_t s = 0, e = 0;
  bool in_range;
  if (!taken_row(a, p, s, e, in_range)) return;
  const int64_t base = a.out_indptr[p];
  for (int64_t q = (int64_t)s + lane; q < e; q += kWave) {
    const int64_t pos = base + (q - s);
    if (pos < 0 || pos >= a.nnz_out) continue;
    const int32_t j = a.indices[q];
    a.out_indices[pos] = j;
    a.out_vals[pos] = a.vals[q];
    if (kT && j >= 0 && j < a.cols) atomicAdd(reinterpret_cast<uint32_t*>(&a.t_indptr[j + 1]), 1u);
  }
}

inline size_t rows_ws_words(int64_t cols, int64_t nnz) { return (size_t)cols + 2 * (size_t)nnz; }

inline int64_t bitmap_words(int64_t cols) { return (cols + 31) / 32; }

// words of the workspace parts, in their order
inline size_t head_words(int64_t cols) { return 2 + (size_t)bitmap_words(cols); }  // oob, bitmap
inline size_t cursor_words(int64_t cols, int64_t nnz) { return (size_t)std::min(cols, nnz); }
inline size_t ws_words(int64_t cols, int64_t b, int64_t nnz) {
  return head_words(cols) + (size_t)bitmap_words(cols) + (size_t)b + cursor_words(cols, nnz) +
         2 * (size_t)nnz;
}

inline void place(BatchArgs& a, void* ws, int64_t nnz_cap) {
  uint32_t* w = static_cast<uint32_t*>(ws);
  a.oob = reinterpret_cast<unsigned long long*>(w);
  a.bitmap = w + 2;
  a.rank = a.bitmap + a.words;
  a.rowcnt = a.rank + a.words;
  a.cursor = a.rowcnt + a.b;
  a.tkey = reinterpret_cast<int32_t*>(a.cursor + cursor_words(a.cols, nnz_cap));
  a.trow = a.tkey + nnz_cap;
}

inline bool bad_shape(int64_t rows, int64_t cols, int64_t b) {
  return rows < 0 || cols < 0 || b < 0 || cols > INT32_MAX || b > INT32_MAX;
}

inline unsigned grid_rows(int64_t b) { return (unsigned)((b + kWavesPerBlock - 1) / kWavesPerBlock); }

}  // namespace
}  // namespace appnp

extern "C" size_t appnp_csr_batch_workspace_bytes(int64_t cols, int64_t b, int64_t nnz_cap) {
  using namespace appnp;
  if (cols <= 0 || b <= 0 || nnz_cap < 0 || cols > INT32_MAX || b > INT32_MAX ||
      nnz_cap > INT32_MAX)
    return 0;
  return round_up(ws_words(cols, b, nnz_cap) * sizeof(uint32_t), 256);
}

extern "C" int appnp_csr_batch_count(const int32_t* indptr, const int32_t* indices,
                                     const float* vals, int64_t rows, int64_t cols,
                                     const int64_t* idx, int64_t b, int32_t* out_indptr,
                                     int64_t* counts, void* ws, size_t ws_bytes, void* stream) {
  using namespace appnp;
  if (bad_shape(rows, cols, b)) return APPNP_EINVAL;
  if (b == 0 || cols == 0) return APPNP_OK;
  if (!indptr || !idx || !out_indptr || !counts || !ws) return APPNP_EINVAL;
  if (ws_bytes < appnp_csr_batch_workspace_bytes(cols, b, 0)) return APPNP_EINVAL;
  if (reinterpret_cast<uintptr_t>(ws) % sizeof(unsigned long long) != 0) return APPNP_EINVAL;

  BatchArgs a{};
  a.indptr = indptr;
  a.indices = indices;
  a.vals = vals;
  a.rows = rows;
  a.cols = cols;
  a.idx = idx;
  a.b = b;
  a.words = bitmap_words(cols);
  a.out_indptr = out_indptr;
  a.counts = counts;
  place(a, ws, 0);
  hipStream_t s = static_cast<hipStream_t>(stream);
  const dim3 block(kBlock), grid(grid_rows(b));

  ktimer_begin(s);
  const hipError_t me = hipMemsetAsync(ws, 0, head_words(cols) * sizeof(uint32_t), s);
  ktimer_mark(s, APPNP_KT_COPY);
  if (me != hipSuccess) return APPNP_EDEVICE;
  int rc = timed_launch(s, APPNP_KT_COPY, [&] {
    if (a.words <= kMarkLdsWords) {
      const int64_t per_block = (int64_t)kWavesPerBlock * kMarkRows;
      const dim3 lds_grid((unsigned)((b + per_block - 1) / per_block));
      hipLaunchKernelGGL(k_batch_mark<true>, lds_grid, block, 0, s, a);
    } else {
      hipLaunchKernelGGL(k_batch_mark<false>, grid, block, 0, s, a);
    }
  });
  if (rc == APPNP_OK)
    rc = timed_launch(s, APPNP_KT_COPY,
                      [&] { hipLaunchKernelGGL(k_batch_rows, grid, block, 0, s, a); });
  if (rc == APPNP_OK)
    rc = timed_launch(s, APPNP_KT_COPY, [&] {
      hipLaunchKernelGGL(k_batch_scan, dim3(1), dim3(kScanThreads), 0, s, a);
    });
  return rc;
}

extern "C" int appnp_csr_batch_emit(const int32_t* indptr, const int32_t* indices,
                                    const float* vals, int64_t rows, int64_t cols,
                                    const int64_t* idx, int64_t b, const int32_t* out_indptr,
                                    int64_t nnz_out, int64_t n_sel, int32_t* out_indices,
                                    float* out_vals, int64_t* sel, int32_t* t_indptr,
                                    int32_t* t_indices, float* t_vals, void* ws, size_t ws_bytes,
                                    void* stream) {
  using namespace appnp;
  if (bad_shape(rows, cols, b) || nnz_out < 0 || n_sel < 0 || nnz_out > INT32_MAX ||
      n_sel > cols || n_sel > nnz_out)
    return APPNP_EINVAL;
  if (b == 0 || cols == 0) return APPNP_OK;
  if (!indptr || !idx || !out_indptr || !t_indptr || !ws) return APPNP_EINVAL;
  if (nnz_out > 0 && (!indices || !vals || !out_indices || !out_vals || !t_indices || !t_vals))
    return APPNP_EINVAL;
  if (n_sel > 0 && !sel) return APPNP_EINVAL;
  if (ws_bytes < appnp_csr_batch_workspace_bytes(cols, b, nnz_out)) return APPNP_EINVAL;
  if (reinterpret_cast<uintptr_t>(ws) % sizeof(unsigned long long) != 0) return APPNP_EINVAL;

  BatchArgs a{};
  a.indptr = indptr;
  a.indices = indices;
  a.vals = vals;
  a.rows = rows;
  a.cols = cols;
  a.idx = idx;
  a.b = b;
  a.words = bitmap_words(cols);
  a.nnz_out = nnz_out;
  a.n_sel = n_sel;
  a.out_indptr = const_cast<int32_t*>(out_indptr);  // read only from here on
  a.out_indices = out_indices;
  a.out_vals = out_vals;
  a.sel = sel;
  a.t_indptr = t_indptr;
  a.t_indices = t_indices;
  a.t_vals = t_vals;
  place(a, ws, nnz_out);
  hipStream_t s = static_cast<hipStream_t>(stream);
  const dim3 block(kBlock), grid(grid_rows(b));
  const dim3 word_grid((unsigned)((a.words + kBlock - 1) / kBlock));

  int rc = timed_launch(s, APPNP_KT_COPY,
                        [&] { hipLaunchKernelGGL(k_batch_sel, word_grid, block, 0, s, a); });
  if (nnz_out == 0 || rc != APPNP_OK) return rc;  // t_indptr = {0}: nothing was selected
  rc = timed_launch(s, APPNP_KT_COPY,
                    [&] { hipLaunchKernelGGL(k_batch_emit, grid, block, 0, s, a); });
  if (rc == APPNP_OK)
    rc = timed_launch(s, APPNP_KT_COPY, [&] {
      hipLaunchKernelGGL(k_batch_tscan, dim3(1), dim3(kScanThreads), 0, s, a);
    });
  if (rc == APPNP_OK)
    rc = timed_launch(s, APPNP_KT_COPY,
                      [&] { hipLaunchKernelGGL(k_batch_scatter, grid, block, 0, s, a); });
  if (rc == APPNP_OK) {
    const dim3 seg_grid((unsigned)((n_sel + kSegsPerBlock - 1) / kSegsPerBlock));
    rc = timed_launch(s, APPNP_KT_COPY,
                      [&] { hipLaunchKernelGGL(k_batch_sort, seg_grid, block, 0, s, a); });
  }
  return rc;
}

extern "C" size_t appnp_csr_rows_workspace_bytes(int64_t cols, int64_t nnz_cap) {
  using namespace appnp;
  if (cols <= 0 || nnz_cap <= 0 || cols > INT32_MAX || nnz_cap > INT32_MAX) return 0;
  return round_up(rows_ws_words(cols, nnz_cap) * sizeof(uint32_t), 256);
}

extern "C" int appnp_csr_rows_count(const int32_t* indptr, const int32_t* indices,
                                    const float* vals, int64_t rows, int64_t cols,
                                    const int64_t* idx, int64_t b, int32_t* out_indptr,
                                    int64_t* counts, void* stream) {
  using namespace appnp;
  if (bad_shape(rows, cols, b)) return APPNP_EINVAL;
  if (b == 0) return APPNP_OK;
  if (!indptr || !idx || !out_indptr || !counts) return APPNP_EINVAL;

  BatchArgs a{};
  a.indptr = indptr;
  a.indices = indices;
  a.vals = vals;
  a.rows = rows;
  a.cols = cols;
  a.idx = idx;
  a.b = b;
  a.out_indptr = out_indptr;
  a.counts = counts;
  hipStream_t s = static_cast<hipStream_t>(stream);
  return timed_launch(s, APPNP_KT_COPY, [&] {
    hipLaunchKernelGGL(k_rows_count, dim3(1), dim3(kScanThreads), 0, s, a);
  });
}

extern "C" int appnp_csr_rows_emit(const int32_t* indptr, const int32_t* indices,
                                   const float* vals, int64_t rows, int64_t cols,
                                   const int64_t* idx, int64_t b, const int32_t* out_indptr,
                                   int64_t nnz_out, int32_t* out_indices, float* out_vals,
                                   int32_t* t_indptr, int32_t* t_indices, float* t_vals, void* ws,
                                   size_t ws_bytes, void* stream) {
  using namespace appnp;
  if (bad_shape(rows, cols, b) || nnz_out < 0 || nnz_out > INT32_MAX) return APPNP_EINVAL;
  if (b == 0) return APPNP_OK;
  if (!indptr || !idx || !out_indptr) return APPNP_EINVAL;
  if (nnz_out > 0 && (!indices || !vals || !out_indices || !out_vals)) return APPNP_EINVAL;
  const bool chain = t_indptr && nnz_out > 0 && cols > 0;  // the transpose holds entries
  if (chain) {
    if (!t_indices || !t_vals || !ws) return APPNP_EINVAL;
    if (ws_bytes < appnp_csr_rows_workspace_bytes(cols, nnz_out)) return APPNP_EINVAL;
    if (reinterpret_cast<uintptr_t>(ws) % sizeof(uint32_t) != 0) return APPNP_EINVAL;
  }

  BatchArgs a{};
  a.indptr = indptr;
  a.indices = indices;
  a.vals = vals;
  a.rows = rows;
  a.cols = cols;
  a.idx = idx;
  a.b = b;
  a.nnz_out = nnz_out;
  a.n_sel = cols;  // every column keeps its id: tscan, scatter and sort run over all of them
  a.out_indptr = const_cast<int32_t*>(out_indptr);  // read only
  a.out_indices = out_indices;
  a.out_vals = out_vals;
  a.t_indptr = t_indptr;
  a.t_indices = t_indices;
  a.t_vals = t_vals;
  if (chain) {
    a.cursor = static_cast<uint32_t*>(ws);
    a.tkey = reinterpret_cast<int32_t*>(a.cursor + cols);
    a.trow = a.tkey + nnz_out;
  }
  hipStream_t s = static_cast<hipStream_t>(stream);
  const dim3 block(kBlock), grid(grid_rows(b));

  int rc = APPNP_OK;
  if (t_indptr) {
    const int64_t blocks = std::min<int64_t>((cols + kBlock) / kBlock, 65536);
    rc = timed_launch(s, APPNP_KT_COPY, [&] {
      hipLaunchKernelGGL(k_rows_clear, dim3((unsigned)blocks), block, 0, s, a);
    });
  }
  if (nnz_out == 0 || rc != APPNP_OK) return rc;
  rc = timed_launch(s, APPNP_KT_COPY, [&] {
    if (chain)
      hipLaunchKernelGGL(k_rows_copy<true>, grid, block, 0, s, a);
    else
      hipLaunchKernelGGL(k_rows_copy<false>, grid, block, 0, s, a);
  });
  if (!chain || rc != APPNP_OK) return rc;
  rc = timed_launch(s, APPNP_KT_COPY, [&] {
    hipLaunchKernelGGL(k_batch_tscan, dim3(1), dim3(kScanThreads), 0, s, a);
  });
  if (rc == APPNP_OK)
    rc = timed_launch(s, APPNP_KT_COPY,
                      [&] { hipLaunchKernelGGL(k_batch_scatter, grid, block, 0, s, a); });
  if (rc == APPNP_OK) {
    const dim3 seg_grid((unsigned)((cols + kSegsPerBlock - 1) / kSegsPerBlock));
    rc = timed_launch(s, APPNP_KT_COPY,
                      [&] { hipLaunchKernelGGL(k_batch_sort, seg_grid, block, 0, s, a); });
  }
  return rc;
}
