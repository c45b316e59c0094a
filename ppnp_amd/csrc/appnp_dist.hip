// appnp_dist.hip -- row-partitioned multi-GPU propagation behind the C ABI
// (include/ppnp_amd.h appnp_dist_*; SURVEY.md 8(b) "appnp_dist_create").
//
// Host orchestration only: every iteration is a few appnp_step* launches on the held rows
// (appnp_capi.hip), and the row shards travel through the caller's exchange callbacks.  There is
// one schedule (Schedule::run; ppnp_amd/dist.py PartitionedAPPNP.run for a pure row layout):
//
//   Z_0: seed iterate 0 with H's held rows, publish it (every rank needs all of Z_0)
//   k = 0 .. K-1:  iterate k&1 (all P S rows) -> the held rows of iterate (k+1)&1
//                  -- or Z itself on the last iteration (nothing is published after it)
//     the early product, on what this rank already holds         -> fp32 partial
//     wait for the exchange of iterate k&1 (internal stream xs)
//     the finishing product + partial + alpha H                   -> the held rows
//     k < K-1:     publish iterate (k+1)&1
//
// It varies in two ways, both fixed per call.
//
// The layout of an iterate.  Whole rows: one [P S, ld] buffer.  Split rows (fp32 F = 32q + r on
// a graph with a source-blocked copy of the held rows, appnp_step_split): two full-height
// parts, main [P S, 32q] (whole cache lines per gathered row) and remainder [P S, width of the
// copy]; both are exchanged, the main part runs the SpMM kernel and the remainder part the
// persistent L2-blocked pass, inside the finishing product, once its exchange has landed.
//
// The exchange.
//   in stream order (no overlap): all-gather each part on `stream`; no early product, the
//     finishing product is ALL.
//   overlapped: the all-gathers run on xs behind the event `produced` and end in `exchanged`,
//     which `stream` waits for between the early product LOCAL (columns in [lo, hi): the own
//     shard, complete) and the finishing product REMOTE.  Z_0 is still exchanged in stream
//     order, nothing could overlap it; rows without main columns (fs = 0) run ALL.
//   pipelined (appnp_dist_set_broadcast): one broadcast per row shard on xs, each followed by
//     its `arrived` event; the early product is FIRST on the own shard, the finishing product
//     ACC per group of arrived shards and LAST on the last group.  A remainder part is
//     all-gathered on xs before the broadcasts (it is small and lands first); LAST waits for it.
//
// The two iterates alternate, and each exchange is waited for before its buffers are written
// again.  So the only concurrent accesses are the exchange of the source iterate, which writes
// the other ranks' shards, and the early product, which reads this rank's shard.
//
// tests/test_dist_trace.py pins every launch, record, wait and exchange of this unit on the CPU.
#include <dlfcn.h>

#include <algorithm>
#include <cstdlib>
#include <new>
#include <vector>

#include "../../include/ppnp_amd.h"
#include "appnp_internal.h"

struct appnp_dist {
  appnp_graph* g = nullptr;
  int64_t n = 0, lo = 0, hi = 0, shard = 0;
  int rank = 0, nranks = 1, overlap = 0;
  appnp_allgather_fn allgather = nullptr;
  void* ctx = nullptr;
  int sb_requested = 0;                // `mode` asked for the source-blocked copy (all ranks)
  int split_agreed = 0;                // the ranks have agreed on split_ok (first propagation)
  int split_ok = 0;                    // every rank holds its rows' source-blocked copy
  int poisoned = APPNP_OK;             // the split agreement failed on this rank: every later
                                       // call returns this code (the ranks may disagree now)
  hipStream_t xs = nullptr;            // exchange stream (overlap)
  hipEvent_t produced = nullptr;       // dst rows written on the caller's stream
  hipEvent_t exchanged = nullptr;      // exchange finished on xs
  // pipelined exchange (appnp_dist_set_broadcast): one broadcast per row shard on xs, each
  // followed by its event, and the groups of remote shards the product waits for in turn
  appnp_bcast_fn bcast = nullptr;
  void* bctx = nullptr;
  std::vector<hipEvent_t> arrived;     // [nranks]: shard r has landed (on xs)
  std::vector<std::pair<int, int>> groups;
};

namespace {

using appnp::as_stream;
using appnp::dev_err;
using appnp::round_up;

constexpr size_t kAlign = 256;

struct WsLayout {
  int64_t ld = 0;          // elements per row of the iterate buffers
  size_t buf_bytes = 0;    // one full-height iterate
  size_t partial_off = 0;  // fp32 partial (overlap)
  size_t total = 0;
  // split rows: main [P S, fs] and remainder [P S, rw] parts of each iterate
  int64_t fs = 0, rw = 0;
  size_t main_bytes = 0, part_bytes = 0;  // one main part; one iterate (main + remainder)
  // staging of a held-rows H or Z whose base or leading dimension does not allow 16-B vectors:
  // [S, f4] fp32 each (f4 = f rounded up to 4), after the iterates and the partial
  int64_t f4 = 0;
  size_t stage_off = 0, stage_bytes = 0;
  size_t split_total = 0;
};

WsLayout ws_layout(const appnp_dist* d, int64_t f, int dtype) {
  WsLayout w;
  const int64_t es = appnp::elem_size(dtype);
  const size_t rows_pad = (size_t)(d->shard * d->nranks);
  w.ld = appnp::line_ld(f, dtype);
  w.buf_bytes = round_up(rows_pad * (size_t)(w.ld * es), kAlign);
  w.partial_off = 2 * w.buf_bytes;
  const size_t partial = d->overlap ? round_up((size_t)d->shard * (size_t)w.ld * 4, kAlign) : 0;
  w.total = w.partial_off + partial;
  if (dtype == APPNP_F32 && appnp_split_layout(d->g, f, &w.fs, &w.rw) == APPNP_OK) {
    w.main_bytes = round_up(rows_pad * (size_t)w.fs * 4, kAlign);
    w.part_bytes = w.main_bytes + round_up(rows_pad * (size_t)w.rw * 4, kAlign);
    w.f4 = (f + 3) / 4 * 4;
    w.stage_off =
        2 * w.part_bytes + (d->overlap ? round_up((size_t)d->shard * w.fs * 4, kAlign) : 0);
    w.stage_bytes = round_up((size_t)d->shard * (size_t)w.f4 * 4, kAlign);
    w.split_total = w.stage_off + 2 * w.stage_bytes;
  }
  return w;
}

// The split layout exchanges two parts per iterate, so every rank must take it or none.  The
// rule is the same on every rank (its locality measure is the whole graph's), but the
// regrouped copy is best-effort: at the first fp32 propagation with K >= 2 of an engine whose
// `mode` asked for the copy, the ranks agree through the exchange itself -- each sets one byte
// of its slot of a small in-place all-gather in the workspace, and the copy is used only if
// every rank built it.  Synchronises the stream once.  If the agreement itself fails on this
// rank (exchange or copy error), its peers may have completed it and decided differently, so
// the handle is poisoned: this and every later call returns the error instead of running a
// loop that exchanges a different number of parts than the peers' (ADVICE r3).
int agree_split(appnp_dist* d, void* ws, hipStream_t s) {
  constexpr size_t kSlot = 256;
  d->split_ok = d->g->rb_off != nullptr;
  if (d->nranks <= 1) {
    d->split_agreed = 1;
    return APPNP_OK;
  }
  char* flags = static_cast<char*>(ws);
  std::vector<unsigned char> host((size_t)d->nranks, 0);
  int rc = dev_err(hipMemsetAsync(flags, 0, kSlot * d->nranks, s));
  if (rc == APPNP_OK && d->split_ok)
    rc = dev_err(hipMemsetAsync(flags + kSlot * d->rank, 1, 1, s));
  if (rc == APPNP_OK) rc = d->allgather(flags, kSlot, d->rank, d->nranks, s, d->ctx);
#ifdef APPNP_TESTING
  // APPNP_DIST_TEST_AGREE_FAIL (test library): a failure on this rank after the exchange, so
  // the poisoned handle can be observed
  const char* inj = std::getenv("APPNP_DIST_TEST_AGREE_FAIL");
  if (rc == APPNP_OK && inj && *inj && std::atoi(inj)) rc = APPNP_EDEVICE;
#endif
  for (int p = 0; p < d->nranks && rc == APPNP_OK; ++p)
    rc = dev_err(hipMemcpyAsync(&host[p], flags + kSlot * p, 1, hipMemcpyDeviceToHost, s));
  if (rc == APPNP_OK) rc = dev_err(hipStreamSynchronize(s));
  for (int p = 0; p < d->nranks; ++p)
    if (rc != APPNP_OK || host[p] != 1) d->split_ok = 0;
  if (rc != APPNP_OK) d->poisoned = rc;
  d->split_agreed = 1;
  return rc;
}

// One exchange through the caller's all-gather on stream s, bracketed for the per-launch timer
// (APPNP_KT_XCHG), so the time it takes is never counted in the launch that waits for it
int exchange_on(appnp_dist* d, void* buf, size_t shard_bytes, hipStream_t s) {
  appnp::ktimer_begin(s);
  const int rc = d->allgather(buf, shard_bytes, d->rank, d->nranks, s, d->ctx);
  appnp::ktimer_mark(s, APPNP_KT_XCHG);
  return rc;
}

// Groups of remote shards in arrival order (ppnp_amd/dist.py shard_groups): sized 1, 2, 4, ...
// from the last to arrive backwards, cut where a group would span the own shard, then adjacent
// groups merged, front first, down to ceil(log2 R) groups.
std::vector<std::pair<int, int>> shard_groups(int R, int ri) {
  std::vector<int> arrival;
  for (int s = 0; s < R; ++s)
    if (s != ri) arrival.push_back(s);
  std::vector<int> sizes;
  for (int left = (int)arrival.size(), sz = 1; left > 0; sz *= 2) {
    const int take = std::min(sz, left);
    sizes.push_back(take);
    left -= take;
  }
  std::vector<std::pair<int, int>> groups;
  size_t pos = 0;
  for (auto it = sizes.rbegin(); it != sizes.rend(); ++it) {
    int start = arrival[pos];
    for (int j = 0; j < *it; ++j) {
      const int a = arrival[pos + j];
      const bool end = j + 1 == *it || arrival[pos + j + 1] != a + 1;
      if (end) {
        groups.emplace_back(start, a + 1);
        if (j + 1 < *it) start = arrival[pos + j + 1];
      }
    }
    pos += *it;
  }
  int cap = 1;
  while ((1 << cap) < R) ++cap;  // ceil(log2 R)
  for (size_t i = 0; groups.size() > (size_t)cap && i + 2 < groups.size();) {  // not the last
    if (groups[i].second == groups[i + 1].first) {
      groups[i].second = groups[i + 1].second;
      groups.erase(groups.begin() + (long)i + 1);
    } else {
      ++i;
    }
  }
  return groups;
}

// rows x (f elements) between two row-major matrices with leading dimensions in elements
hipError_t copy_rows(void* dst, int64_t ld_dst, const void* src, int64_t ld_src, int64_t rows,
                     int64_t f, int64_t es, hipStream_t s) {
  if (rows <= 0 || f <= 0) return hipSuccess;
  return hipMemcpy2DAsync(dst, (size_t)(ld_dst * es), src, (size_t)(ld_src * es),
                          (size_t)(f * es), (size_t)rows, hipMemcpyDeviceToDevice, s);
}

// What a step contributes to the held rows: appnp_part, then appnp_shard_mode
enum Role {
  ALL = APPNP_PART_ALL,
  LOCAL = APPNP_PART_LOCAL,
  REMOTE = APPNP_PART_REMOTE,
  FIRST,  // over a range of source shards: FIRST + its appnp_shard_mode
  ACC = FIRST + APPNP_SHARDS_ACC,
  LAST = FIRST + APPNP_SHARDS_LAST
};
static_assert(APPNP_SHARDS_FIRST == 0 && FIRST > REMOTE, "appnp_part, then appnp_shard_mode");
// the step writes the output rows (+ alpha H); the others write the partial
constexpr bool finishes(Role r) { return r == ALL || r == REMOTE || r == LAST; }

// One propagation (see the file comment): the call's operands, where the two iterates and the
// partial live in the workspace, which parts of an iterate are exchanged and how, and the loop.
struct Schedule {
  appnp_dist* d;
  hipStream_t s;
  const void* H;
  int64_t ld_h;
  void* Z;
  int64_t ld_z;
  int64_t f;
  int dtype, K;
  float alpha, p_drop;
  uint64_t seed;
  // the layout, from WsLayout: iterate b is main[b] (whole rows: all of it, [P S, ld]) and, in
  // the split layout, rem[b]; *_shard are the bytes of one rank's rows of a part, 0: no such part
  bool split;
  int64_t ld, fs;
  char* main[2];
  char* rem[2];
  size_t main_shard, rem_shard;
  float* partial;  // [S, ld_partial] fp32 (overlap)
  int64_t ld_partial;
  bool pipelined;        // the main part travels by broadcasts (d->bcast, which implies overlap and
                         // so fp32: appnp_dist_propagate rejects bf16 with overlap)
  bool pending = false;  // an all-gather on xs that `s` has not waited for yet

  // H / Z: set by the caller, which may have staged them
  Schedule(appnp_dist* d_, const WsLayout& w, bool split_, char* base, int64_t f_, int dtype_,
           int K_, float alpha_, float p_drop_, uint64_t seed_, hipStream_t s_)
      : d(d_), s(s_), H(nullptr), ld_h(0), Z(nullptr), ld_z(0), f(f_), dtype(dtype_), K(K_),
        alpha(alpha_), p_drop(p_drop_), seed(seed_), split(split_), ld(w.ld), fs(w.fs) {
    const size_t stride = split ? w.part_bytes : w.buf_bytes;
    for (int b = 0; b < 2; ++b) {
      main[b] = base + b * stride;
      rem[b] = split ? main[b] + w.main_bytes : nullptr;
    }
    const size_t S = (size_t)d->shard;
    main_shard = S * (size_t)(split ? fs * 4 : ld * appnp::elem_size(dtype));
    rem_shard = split ? S * (size_t)w.rw * 4 : 0;
    partial = d->overlap ? reinterpret_cast<float*>(base + 2 * stride) : nullptr;
    ld_partial = split ? fs : ld;
    pipelined = d->bcast && main_shard > 0;
  }

  static float* f32(char* p) { return reinterpret_cast<float*>(p); }
  // the held rows of whole-row iterate b
  char* own(int b) const { return main[b] + (size_t)(d->lo * ld * appnp::elem_size(dtype)); }

  // Z_0's held rows
  int seed_rows() const {
    if (split)
      return appnp_split_copy(d->g, static_cast<const float*>(H), ld_h, f,
                              fs ? f32(main[0]) : nullptr, f32(rem[0]), s);
    return dev_err(
        copy_rows(own(0), ld, H, ld_h, d->hi - d->lo, f, appnp::elem_size(dtype), s));
  }

  // The step of iteration k in `role` (FIRST / ACC / LAST: over the source shards [s_lo, s_hi)):
  // from iterate k&1; a finishing step writes the held rows of the other iterate, or Z on the
  // last iteration.  A step is handed only what its role reads and writes.
  int step(Role role, int s_lo, int s_hi, int k) const {
    const bool fin = finishes(role), last = k == K - 1;
    const int cur = k & 1, nxt = cur ^ 1;
    const float* h = fin ? static_cast<const float*>(H) : nullptr;
    const int64_t lh = fin ? ld_h : 0;
    if (split) {
      const float* zin_rem = fin ? f32(rem[cur]) : nullptr;
      float* out_main = fin && !last ? f32(main[nxt]) : nullptr;
      float* out_rem = fin && !last ? f32(rem[nxt]) : nullptr;
      float* z = fin && last ? static_cast<float*>(Z) : nullptr;
      const int64_t lz = fin ? ld_z : 0;
      float* part = role == ALL ? nullptr : partial;
      const int64_t ld_part = role == ALL ? 0 : ld_partial;
      if (role < FIRST)
        return appnp_step_split(d->g, role, f32(main[cur]), zin_rem, h, lh, out_main, out_rem, z,
                                lz, part, ld_part, f, k, alpha, p_drop, seed, s);
      return appnp_step_split_shards(d->g, s_lo, s_hi, role - FIRST, f32(main[cur]), zin_rem, h,
                                     lh, out_main, out_rem, z, lz, part, ld_part, f, k, alpha,
                                     p_drop, seed, s);
    }
    void* out = !fin ? nullptr : last ? Z : own(nxt);
    const int64_t ld_out = !fin ? 0 : last ? ld_z : ld;
    if (role >= FIRST)
      return appnp_step_shards(d->g, s_lo, s_hi, role - FIRST, f32(main[cur]), ld, h, lh,
                               static_cast<float*>(out), ld_out, partial, ld_partial, f, k, alpha,
                               p_drop, seed, s);
    // appnp_step takes LOCAL's partial as its output rows, and another one only to read it
    const bool reads = role == REMOTE;
    return appnp_step(d->g, role, main[cur], ld, h, lh, role == LOCAL ? partial : out,
                      role == LOCAL ? ld_partial : ld_out, reads ? partial : nullptr,
                      reads ? ld_partial : 0, f, dtype, k, alpha, p_drop, seed, s);
  }

  // All-gather the parts of iterate b on stream `on`: the main part unless it travels by
  // broadcasts, then the remainder part
  int all_gather(int b, hipStream_t on) const {
    int rc = APPNP_OK;
    if (main_shard && !pipelined) rc = exchange_on(d, main[b], main_shard, on);
    if (rc == APPNP_OK && rem_shard) rc = exchange_on(d, rem[b], rem_shard, on);
    return rc;
  }

  // xs goes on behind what `s` holds now
  int xs_follows() const {
    const int rc = dev_err(hipEventRecord(d->produced, s));
    return rc == APPNP_OK ? dev_err(hipStreamWaitEvent(d->xs, d->produced, 0)) : rc;
  }

  // `s` goes on behind the all-gather on xs
  int wait_exchanged() {
    pending = false;
    return dev_err(hipStreamWaitEvent(s, d->exchanged, 0));
  }

  // Hand the held rows of iterate b, written on `s`, to every rank.  Z_0 (`first`) has nothing to
  // overlap with, so the all-gather loops exchange it in stream order even with overlap.
  int publish(int b, bool first) {
    if (d->nranks == 1) return APPNP_OK;
    if (!pipelined && (first || !d->overlap)) return all_gather(b, s);
    int rc = APPNP_OK;
    if (!pipelined || rem_shard) {
      // the all-gathered parts on xs; pipelined, that is the remainder part (small: it lands
      // before the main shards), which LAST waits for -- otherwise the next iteration does
      rc = xs_follows();
      if (rc == APPNP_OK) rc = all_gather(b, d->xs);
      if (rc == APPNP_OK) rc = dev_err(hipEventRecord(d->exchanged, d->xs));
      pending = rc == APPNP_OK && !pipelined;
    }
    if (!pipelined) return rc;
    // row shard r from rank r, r = 0 .. P-1 in turn (the same order on every rank), each bracketed
    // for the timer and followed by its arrival event
    if (rc == APPNP_OK) rc = xs_follows();
    for (int r = 0; r < d->nranks && rc == APPNP_OK; ++r) {
      appnp::ktimer_begin(d->xs);
      rc = d->bcast(main[b] + (size_t)r * main_shard, main_shard, r, d->nranks, d->xs, d->bctx);
      appnp::ktimer_mark(d->xs, APPNP_KT_XCHG);
      if (rc == APPNP_OK) rc = dev_err(hipEventRecord(d->arrived[r], d->xs));
    }
    return rc;
  }

  // The finishing product of iteration k, with the waits it needs
  int finish(int k, bool early) {
    int rc = APPNP_OK;
    if (!pipelined) {
      if (pending) rc = wait_exchanged();
      return rc == APPNP_OK ? step(early ? REMOTE : ALL, 0, 0, k) : rc;
    }
    // ACC per group of arrived shards, LAST (and with it the remainder pass) on the last group
    for (size_t i = 0; i < d->groups.size() && rc == APPNP_OK; ++i) {
      const int a = d->groups[i].first, b = d->groups[i].second;
      const bool last_group = i + 1 == d->groups.size();
      rc = dev_err(hipStreamWaitEvent(s, d->arrived[b - 1], 0));
      if (rc == APPNP_OK && last_group && rem_shard) rc = wait_exchanged();
      if (rc == APPNP_OK) rc = step(last_group ? LAST : ACC, a, b, k);
    }
    // the own shard's send: the last thing on xs of this exchange (s waits for it before the
    // next exchange reuses the buffer, at no cost: it precedes that exchange on xs anyway)
    if (rc == APPNP_OK) rc = dev_err(hipStreamWaitEvent(s, d->arrived[d->nranks - 1], 0));
    return rc;
  }

  int run() {
    // the early product needs main columns of its own: LOCAL on the own columns, FIRST on the
    // own shard
    const bool early = pipelined || (d->overlap && main_shard > 0);
    int rc = seed_rows();
    if (rc == APPNP_OK) rc = publish(0, true);
    for (int k = 0; k < K && rc == APPNP_OK; ++k) {
      if (early) rc = step(pipelined ? FIRST : LOCAL, d->rank, d->rank + 1, k);
      if (rc == APPNP_OK) rc = finish(k, early);
      if (rc == APPNP_OK && k < K - 1) rc = publish((k + 1) & 1, false);
    }
    if (pending) (void)wait_exchanged();  // never leave xs running ahead
    return rc;
  }
};

// RCCL, resolved at first use (appnp_allgather_rccl, appnp_bcast_rccl)
typedef int (*nccl_allgather_t)(const void*, void*, size_t, int, void*, hipStream_t);
typedef int (*nccl_bcast_t)(const void*, void*, size_t, int, int, void*, hipStream_t);

void* rccl_handle() {
  static void* h = [] {
    const char* env = std::getenv("APPNP_RCCL_LIB");
    void* x = nullptr;
    if (env && *env) {
      x = dlopen(env, RTLD_NOW | RTLD_LOCAL);
    } else {
      // the copy already in the process (PyTorch's), so its communicators are valid here
      x = dlopen("librccl.so.1", RTLD_NOW | RTLD_NOLOAD);
      if (!x) x = dlopen("librccl.so.1", RTLD_NOW | RTLD_LOCAL);
    }
    return x;
  }();
  return h;
}

nccl_allgather_t rccl_allgather() {
  static nccl_allgather_t fn = rccl_handle() ? reinterpret_cast<nccl_allgather_t>(
                                                   dlsym(rccl_handle(), "ncclAllGather"))
                                             : nullptr;
  return fn;
}

nccl_bcast_t rccl_bcast() {
  static nccl_bcast_t fn =
      rccl_handle() ? reinterpret_cast<nccl_bcast_t>(dlsym(rccl_handle(), "ncclBroadcast"))
                    : nullptr;
  return fn;
}

}  // namespace

extern "C" {

int appnp_dist_create(const int32_t* indptr, const int32_t* indices, const float* vals,
                      int64_t n, int64_t nnz, int mode, int rank, int nranks, int overlap,
                      appnp_allgather_fn allgather, void* ctx, void* stream, appnp_dist** out) {
  if (!out) return APPNP_EINVAL;
  *out = nullptr;
  if (n <= 0 || nranks < 1 || rank < 0 || rank >= nranks || (nranks > 1 && !allgather))
    return APPNP_EINVAL;
  appnp_dist* d = new (std::nothrow) appnp_dist();
  if (!d) return APPNP_ENOMEM;
  d->n = n;
  d->rank = rank;
  d->nranks = nranks;
  d->overlap = (overlap && nranks > 1) ? 1 : 0;
  d->allgather = allgather;
  d->ctx = ctx;
  d->shard = (n + nranks - 1) / nranks;
  d->lo = std::min<int64_t>(n, (int64_t)rank * d->shard);
  d->hi = std::min<int64_t>(n, d->lo + d->shard);
  int rc = appnp_graph_create_rows(indptr, indices, vals, n, nnz, mode, d->lo, d->hi,
                                   d->overlap, stream, &d->g);
  d->sb_requested = (mode & (APPNP_GRAPH_SOURCE_BLOCKS | APPNP_GRAPH_SB_W8 |
                             APPNP_GRAPH_SB_W16)) != 0;
  if (rc == APPNP_OK && d->overlap) {
    rc = dev_err(hipStreamCreateWithFlags(&d->xs, hipStreamNonBlocking));
    if (rc == APPNP_OK) rc = dev_err(hipEventCreateWithFlags(&d->produced, hipEventDisableTiming));
    if (rc == APPNP_OK)
      rc = dev_err(hipEventCreateWithFlags(&d->exchanged, hipEventDisableTiming));
  }
  if (rc != APPNP_OK) {
    appnp_dist_destroy(d);
    return rc;
  }
  *out = d;
  return APPNP_OK;
}

int appnp_dist_rows(const appnp_dist* d, int64_t* row_lo, int64_t* row_hi, int64_t* shard) {
  if (!d) return APPNP_EINVAL;
  if (row_lo) *row_lo = d->lo;
  if (row_hi) *row_hi = d->hi;
  if (shard) *shard = d->shard;
  return APPNP_OK;
}

const appnp_graph* appnp_dist_graph(const appnp_dist* d) { return d ? d->g : nullptr; }

size_t appnp_dist_workspace_bytes(const appnp_dist* d, int64_t f, int dtype) {
  if (!d || f <= 0 || !appnp::valid_dtype(dtype)) return 0;
  const WsLayout w = ws_layout(d, f, dtype);
  return std::max(w.total, w.split_total);
}

int appnp_dist_propagate(appnp_dist* d, const void* H, int64_t ld_h, void* Z, int64_t ld_z,
                         int64_t f, int dtype, int K, float alpha, float p_drop, uint64_t seed,
                         void* ws, size_t ws_bytes, void* stream) {
  if (!d || f < 0 || K < 0 || !appnp::valid_dtype(dtype)) return APPNP_EINVAL;
  if (d->overlap && dtype != APPNP_F32) return APPNP_ENOTSUP;
  if (!(alpha >= 0.0f && alpha <= 1.0f) || !(p_drop >= 0.0f && p_drop < 1.0f))
    return APPNP_EINVAL;
  if (d->poisoned != APPNP_OK) return d->poisoned;
  const int64_t rows = d->hi - d->lo;
  if (f == 0) return APPNP_OK;
  if (rows > 0 && (!H || !Z || ld_h < f || ld_z < f)) return APPNP_EINVAL;
  hipStream_t s = as_stream(stream);
  if (K == 0) return dev_err(copy_rows(Z, ld_z, H, ld_h, rows, f, appnp::elem_size(dtype), s));
  const WsLayout w = ws_layout(d, f, dtype);
  if (d->sb_requested && !d->split_agreed && dtype == APPNP_F32 && K >= 2) {
    if (!ws || ws_bytes < w.total || ws_bytes < 256 * (size_t)d->nranks) return APPNP_EINVAL;
    const int arc = agree_split(d, ws, s);
    if (arc != APPNP_OK) return arc;
  }
  // split rows whenever every rank's copy allows it (K >= 2: one iteration gains nothing from
  // the split layout).  The decision depends only on what the ranks agreed on, so every rank
  // exchanges the same parts: an H or Z whose base pointer or leading dimension does not allow
  // 16-B vectors is this rank's alone, and it is staged through the workspace ([S, f4] fp32,
  // copied in before the loop and out after it) rather than changing this rank's path (ADVICE
  // r4: round 4 returned APPNP_EINVAL there while the peers waited in the split loop's exchange)
  const bool split = d->split_ok && w.split_total && K >= 2;
  if (!ws || ws_bytes < (split ? w.split_total : w.total)) return APPNP_EINVAL;
  // the base stays as the caller passes it: every buffer shares its alignment
  char* base = static_cast<char*>(ws);
  Schedule run(d, w, split, base, f, dtype, K, alpha, p_drop, seed, s);
  run.H = H, run.ld_h = ld_h, run.Z = Z, run.ld_z = ld_z;
  auto vec16 = [](const void* p, int64_t ld) { return appnp::vec16(&ld, 1, &p, 1); };
  const bool stage_h = split && rows > 0 && !vec16(H, ld_h);
  const bool stage_z = split && rows > 0 && !vec16(Z, ld_z);
  int rc = APPNP_OK;
  if (stage_h) {
    run.H = base + w.stage_off;
    run.ld_h = w.f4;
    rc = dev_err(copy_rows(base + w.stage_off, w.f4, H, ld_h, rows, f, 4, s));
  }
  if (stage_z) {
    run.Z = base + w.stage_off + w.stage_bytes;
    run.ld_z = w.f4;
  }
  if (rc == APPNP_OK) rc = run.run();
  if (rc == APPNP_OK && stage_z) rc = dev_err(copy_rows(Z, ld_z, run.Z, w.f4, rows, f, 4, s));
  return rc;
}

int appnp_dist_set_broadcast(appnp_dist* d, appnp_bcast_fn fn, void* ctx, void* stream) {
  if (!d || !fn) return APPNP_EINVAL;
  if (!d->overlap || d->nranks < 3) return APPNP_ENOTSUP;  // nothing to pipeline
  if (d->poisoned != APPNP_OK) return d->poisoned;
  int rc = appnp_graph_shard_offsets(d->g, d->nranks, d->shard, stream);
  std::vector<hipEvent_t> ev((size_t)d->nranks, nullptr);
  for (size_t r = 0; r < ev.size() && rc == APPNP_OK; ++r)
    rc = dev_err(hipEventCreateWithFlags(&ev[r], hipEventDisableTiming));
  if (rc != APPNP_OK) {
    for (hipEvent_t e : ev)
      if (e) (void)hipEventDestroy(e);
    return rc;
  }
  for (hipEvent_t e : d->arrived) (void)hipEventDestroy(e);
  d->arrived = ev;
  d->groups = shard_groups(d->nranks, d->rank);
  d->bcast = fn;
  d->bctx = ctx;
  return APPNP_OK;
}

int appnp_dist_pipeline_groups(const appnp_dist* d, int* lo, int* hi, int max, int* n_out) {
  if (!d || !n_out) return APPNP_EINVAL;
  *n_out = d->bcast ? (int)d->groups.size() : 0;
  for (int i = 0; i < *n_out && i < max; ++i) {
    if (lo) lo[i] = d->groups[i].first;
    if (hi) hi[i] = d->groups[i].second;
  }
  return APPNP_OK;
}

void appnp_dist_destroy(appnp_dist* d) {
  if (!d) return;
  if (d->xs) (void)hipStreamSynchronize(d->xs);
  for (hipEvent_t e : d->arrived) (void)hipEventDestroy(e);
  if (d->produced) (void)hipEventDestroy(d->produced);
  if (d->exchanged) (void)hipEventDestroy(d->exchanged);
  if (d->xs) (void)hipStreamDestroy(d->xs);
  appnp_graph_destroy(d->g);
  delete d;
}

int appnp_bcast_rccl(void* buf, size_t bytes, int root, int nranks, void* stream, void* ctx) {
  if (!buf || !ctx || root < 0 || root >= nranks) return APPNP_EINVAL;
  const nccl_bcast_t fn = rccl_bcast();
  if (!fn) return APPNP_ENOTSUP;
  // ncclChar = 0; in place (sendbuff == recvbuff); ncclSuccess = 0
  return fn(buf, buf, bytes, 0, root, ctx, as_stream(stream)) == 0 ? APPNP_OK : APPNP_EDEVICE;
}

int appnp_allgather_rccl(void* buf, size_t shard_bytes, int rank, int nranks, void* stream,
                         void* ctx) {
  if (!buf || !ctx || rank < 0 || rank >= nranks) return APPNP_EINVAL;
  const nccl_allgather_t fn = rccl_allgather();
  if (!fn) return APPNP_ENOTSUP;
  char* b = static_cast<char*>(buf);
  // ncclChar = 0; ncclSuccess = 0
  return fn(b + (size_t)rank * shard_bytes, b, shard_bytes, 0, ctx, as_stream(stream)) == 0
             ? APPNP_OK
             : APPNP_EDEVICE;
}

}  // extern "C"
