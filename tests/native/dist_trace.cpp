// dist_trace.cpp -- the launch trace of ppnp_amd/csrc/appnp_dist.hip, recorded on a CPU.
//
// The row-partition engine holds no kernel: it requests appnp_step* launches, calls the caller's
// exchange callbacks, and orders two streams with events.  This program links its host-only
// object (built with -DAPPNP_TESTING) with those of appnp_capi.hip and appnp_propagate.hip
// against the recording stand-ins of capi_trace.cpp, drives every appnp_dist_* entry point on
// fabricated row partitions, and prints what reaches the device boundary -- every launch with
// every argument, every event record and wait with its stream, every exchange -- plus each
// return code.  tests/test_dist_trace.py compares the output with tests/golden/dist_trace.txt
// byte for byte.  A mistake in this unit is a race or a deadlock between ranks, which a GPU run
// would usually survive; here a missing wait is a missing line.
//
// To keep the golden file small, each kind of run is recorded once with every argument and its
// variations (other ranks, P, K) in a brief form: one short line per call with its name, stream,
// role, shard range and buffers.  What creating and destroying an engine requests is shown by the
// teardown cases only, and a failure run is printed from the failing call on.
//
// Run it with every APPNP_* variable removed from the environment.
#include <unistd.h>

#include <cstdlib>
#include <functional>
#include <memory>
#include <string>

#define TRACE_STANDINS_ONLY  // the stand-ins and operands of capi_trace.cpp, not its cases
#include "capi_trace.cpp"

namespace {

constexpr int64_t kN = 10007;    // no P of the cases divides it: the last rank's shard is short
constexpr int64_t kNs = 100003;  // the same for the split layout, which needs n > 2^16

int g_xchg = 0;       // exchange callbacks called so far
int g_fail_xchg = 0;  // the callback (1-based count) that fails; 0: none
void* const kCtx = at<void>(0xc7c0);
void* const kBctx = at<void>(0xbc70);

int exchange_cb(const char* name, const char* who, void* buf, size_t bytes, int r, int nranks,
                void* stream, void* ctx) {
  const bool fails = ++g_xchg == g_fail_xchg;
  if (g_brief)
    printf("%s s=%#llx buf=%#llx bytes=%zu %s=%d", name, X(stream), X(buf), bytes, who, r);
  else
    printf("%s buf=%#llx bytes=%zu %s=%d nranks=%d s=%#llx ctx=%#llx", name, X(buf), bytes, who, r,
           nranks, X(stream), X(ctx));
  printf(fails ? " -> fails\n" : "\n");
  return fails ? APPNP_EDEVICE : APPNP_OK;
}
int allgather_cb(void* buf, size_t bytes, int rank, int nranks, void* stream, void* ctx) {
  return exchange_cb("allgather", "rank", buf, bytes, rank, nranks, stream, ctx);
}
int bcast_cb(void* buf, size_t bytes, int root, int nranks, void* stream, void* ctx) {
  return exchange_cb("bcast", "root", buf, bytes, root, nranks, stream, ctx);
}

constexpr int W4 = APPNP_GRAPH_SOURCE_BLOCKS, W8 = APPNP_GRAPH_SB_W8, W16 = APPNP_GRAPH_SB_W16;

// What is printed while one of these lives is kept, not shown: the set-up of a query case
// (dropped), the part of a failure run before the failure
struct Mute {
  int saved;
  FILE* kept;
  Mute() : kept(tmpfile()) {
    fflush(stdout);
    saved = dup(1);
    dup2(fileno(kept), 1);
  }
  std::string text() {
    fflush(stdout);
    std::string t((size_t)ftell(kept), '\0');
    rewind(kept);
    t.resize(fread(&t[0], 1, t.size(), kept));
    return t;
  }
  ~Mute() {
    fflush(stdout);
    dup2(saved, 1);
    close(saved);
    fclose(kept);
  }
};

// what creating and destroying an engine requests is the same for every case of a kind: only
// the teardown cases show it
bool g_show_setup = false;

// appnp_dist_create (+ appnp_dist_set_broadcast) of rank `rank` of P
appnp_dist* engine(int rank, int P, int overlap, bool bcast = false, int mode = APPNP_NORM_SYM,
                   int64_t n = kN) {
  appnp_dist* d = nullptr;
  int rc, rc_bcast = 1;
  {
    std::unique_ptr<Mute> quiet(g_show_setup ? nullptr : new Mute);
    rc = appnp_dist_create(at<int32_t>(0x70000000), at<int32_t>(0x71000000), nullptr, n, 25 * n,
                           mode, rank, P, overlap, allgather_cb, kCtx, kStream, &d);
    if (d && bcast) rc_bcast = appnp_dist_set_broadcast(d, bcast_cb, kBctx, kStream);
  }
  printf("create rank=%d P=%d overlap=%d mode=%#x n=%" PRId64 " -> %d\n", rank, P, overlap, mode,
         n, rc);
  if (rc_bcast != 1) printf("set_broadcast -> %d\n", rc_bcast);
  return d;
}
void destroy(appnp_dist* d) {
  std::unique_ptr<Mute> quiet(g_show_setup ? nullptr : new Mute);
  appnp_dist_destroy(d);
}
appnp_dist* split_engine(int rank, int P, int overlap, bool bcast = false, int mode = W4) {
  return engine(rank, P, overlap, bcast, mode, kNs);
}

struct Run {
  appnp_dist* d;
  const void* H = kH;
  int64_t ld_h;
  void* Z = kZ;
  int64_t ld_z;
  int64_t f;
  int dtype;
  int K;
  float alpha = 0.1f, p_drop = 0.0f;
  uint64_t seed = 42;
  void* ws = kWs;
  size_t ws_bytes;

  Run(appnp_dist* d_, int64_t f_, int K_ = 3, int dtype_ = APPNP_F32)
      : d(d_), ld_h(f_), ld_z(f_), f(f_), dtype(dtype_), K(K_),
        ws_bytes(appnp_dist_workspace_bytes(d_, f_, dtype_)) {}
  int go() const {
    const int rc = appnp_dist_propagate(d, H, ld_h, Z, ld_z, f, dtype, K, alpha, p_drop, seed, ws,
                                        ws_bytes, kStream);
    printf("propagate f=%" PRId64 " dtype=%d K=%d ws_bytes=%zu -> %d\n", f, dtype, K, ws_bytes, rc);
    return rc;
  }
};

// the same in the brief form (a call another case records in full)
int brief(const Run& r) {
  g_brief = true;
  const int rc = r.go();
  g_brief = false;
  return rc;
}

// propagate once for each K of `ks` (-K: K iterations in the brief form), destroy
int runs(appnp_dist* d, int64_t f, std::initializer_list<int> ks, int dtype = APPNP_F32) {
  int rc = APPNP_OK;
  for (int K : ks) rc = K < 0 ? brief(Run(d, f, -K, dtype)) : Run(d, f, K, dtype).go();
  destroy(d);
  return rc;
}

// the pending agreement bytes of the next appnp_dist_propagate: every peer built the copy
// unless `missing` names one
unsigned char g_flags[8];
void peers_say(int missing = -1) {
  for (int p = 0; p < 8; ++p) g_flags[p] = p == missing ? 0 : 1;
  g_peer_flags = g_flags;
  g_peer_next = 0;
}

// Run `r` under the per-launch timer and print the kinds it recorded, nothing else
int timed(const Run& r) {
  float ms[64];
  int kinds[64], n = -1, rc_begin, rc_run, rc;
  {
    Mute m;
    rc_begin = appnp_kernel_timer_begin(32, kStream);
    rc_run = r.go();
    rc = appnp_kernel_timer_end(ms, kinds, 64, &n);
    destroy(r.d);
  }
  printf("timer_begin -> %d, propagate -> %d, kinds n=%d:", rc_begin, rc_run, n);
  for (int i = 0; i < n && i < 64 && rc == APPNP_OK; ++i) printf(" %d", kinds[i]);
  printf("\n");
  return rc;
}

// one run of `r` in which a call fails: print it from the failing call on (up to there it is the
// clean run), which is what still runs after the error
void failing_run(const Run& r) {
  std::string t;
  {
    Mute m;
    r.go();
    t = m.text();
  }
  const size_t at = t.find(" -> fails\n");
  const size_t line = at == std::string::npos ? 0 : t.rfind('\n', at) + 1;
  fputs(t.c_str() + line, stdout);
}

// The failure paths of one loop, in the brief form: after one clean run (and an unrecorded one
// before it, which settles the split agreement), fail the i-th exchange callback for every i,
// then the i-th launch for every i, one per run.  What is printed after "-> fails" is what still
// runs after the error.
int failures(appnp_dist* d, int64_t f) {
  g_brief = true;
  Run r(d, f, 2);
  {
    Mute m;
    r.go();
  }
  g_xchg = g_launches = 0;
  printf("clean:\n");
  r.go();
  const int n_xchg = g_xchg, n_launch = g_launches;
  for (int i = 1; i <= n_xchg; ++i) {
    printf("exchange %d of %d:\n", i, n_xchg);
    g_xchg = 0;
    g_fail_xchg = i;
    failing_run(r);
  }
  g_fail_xchg = 0;
  for (int i = 1; i <= n_launch; ++i) {
    printf("launch %d of %d:\n", i, n_launch);
    g_launches = 0;
    g_fail_launch = i;
    failing_run(r);
  }
  g_fail_launch = 0;
  g_brief = false;
  destroy(d);
  return APPNP_OK;
}

// "rejected-begin" .. "rejected-end": every line between the two is a return code, nothing else
// (a rejected call requests nothing); tests/test_dist_trace.py asserts it
void rc_line(const char* what, long long rc) { printf("rc %s -> %lld\n", what, rc); }

struct Case {
  const char* name;
  std::function<int()> run;
};

#define CASE(name, ...) {name, []() -> int { __VA_ARGS__ }},

const Case kCases[] = {
    // ---- whole rows, all-gather ------------------------------------------------------------
    CASE("rows P=1 K=0,1,3", return runs(engine(0, 1, 0), 64, {0, 1, 3});)
    CASE("rows P=1 with overlap asked for (there is none)", return runs(engine(0, 1, 1), 64, {-2});)
    CASE("rows P=2 rank 0 f32 K=2", return runs(engine(0, 2, 0), 64, {2});)
    CASE("rows P=2 rank 1 bf16 K=0,2", return runs(engine(1, 2, 0), 64, {0, 2}, APPNP_BF16);)
    CASE("rows P=2 rank 0 overlap K=1,2,3", return runs(engine(0, 2, 1), 64, {-1, 2, -3});)
    CASE("rows P=4 rank 3 overlap K=1,2,3", return runs(engine(3, 4, 1), 64, {-1, -2, -3});)
    CASE("rows P=2 rank 1 overlap dropout", appnp_dist* d = engine(1, 2, 1); Run r(d, 64, 2);
         r.p_drop = 0.5f; r.seed = 0x1234567; const int rc = r.go(); destroy(d); return rc;)
    CASE("rows P=2 rank 0 dropout, no overlap", appnp_dist* d = engine(0, 2, 0); Run r(d, 64, 2);
         r.p_drop = 0.25f; const int rc = r.go(); destroy(d); return rc;)
    CASE("rows bf16 with overlap", return runs(engine(0, 2, 1), 64, {2}, APPNP_BF16);)
    CASE("rows F=20 P=2 rank 1 K=2", return runs(engine(1, 2, 0), 20, {2});)
    CASE("rows F=20 P=2 rank 1 overlap K=2", return runs(engine(1, 2, 1), 20, {-2});)
    CASE("rows F=20 bf16 ld=24 P=2 rank 0", appnp_dist* d = engine(0, 2, 0); Run r(d, 20, 2, APPNP_BF16);
         r.ld_h = r.ld_z = 24; const int rc = r.go(); destroy(d); return rc;)
    CASE("rows f = 0 is a no-op", return runs(engine(0, 2, 1), 0, {3});)
    CASE("rows unaligned ws keeps its base", appnp_dist* d = engine(1, 2, 1); Run r(d, 64, 2);
         r.ws = off(kWs, 16); const int rc = brief(r); destroy(d); return rc;)
    // ---- whole rows, pipelined -------------------------------------------------------------
    CASE("pipelined P=3 rank 0 K=1,3", return runs(engine(0, 3, 1, true), 64, {-1, 3});)
    CASE("pipelined P=3 rank 1 K=2", return runs(engine(1, 3, 1, true), 64, {-2});)
    CASE("pipelined P=3 rank 2 K=2", return runs(engine(2, 3, 1, true), 64, {-2});)
    CASE("pipelined P=5 rank 2 K=1,3", return runs(engine(2, 5, 1, true), 64, {-1, -3});)
    CASE("pipelined P=8 rank 0 K=1", return runs(engine(0, 8, 1, true), 64, {-1});)
    CASE("pipelined P=8 rank 3 K=1,3", return runs(engine(3, 8, 1, true), 64, {-1, -3});)
    CASE("pipelined P=8 rank 7 K=2", return runs(engine(7, 8, 1, true), 64, {-2});)
    CASE("pipelined F=20 P=3 rank 1 K=2", return runs(engine(1, 3, 1, true), 20, {2});)
    CASE("pipelined K=0 copies", return runs(engine(1, 3, 1, true), 64, {0});)
    // ---- split layout, all-gather ----------------------------------------------------------
    CASE("split F=100 W4 P=2 rank 0 overlap K=1,2,3", peers_say(); return runs(split_engine(0, 2, 1), 100, {-1, -2, 3});)
    CASE("split F=100 W4 P=2 rank 1 K=3", peers_say(); return runs(split_engine(1, 2, 0), 100, {3});)
    CASE("split F=100 W4 P=1 K=1,2", return runs(split_engine(0, 1, 0), 100, {1, 2});)
    CASE("split F=100 W4 P=4 rank 3 overlap K=3", peers_say(); return runs(split_engine(3, 4, 1), 100, {-3});)
    CASE("split F=40 W8 P=4 rank 1 overlap K=2", peers_say(); return runs(split_engine(1, 4, 1, false, W8), 40, {2});)
    CASE("split F=40 W8 P=2 rank 0 K=2", peers_say(); return runs(split_engine(0, 2, 0, false, W8), 40, {-2});)
    CASE("split F=13 W16 P=2 rank 1 overlap K=2", peers_say(); return runs(split_engine(1, 2, 1, false, W16), 13, {2});)
    CASE("split F=13 W16 P=1 K=3", return runs(split_engine(0, 1, 0, false, W16), 13, {-3});)
    CASE("split F=100 on W16 stays whole rows", peers_say(); return runs(split_engine(0, 2, 1, false, W16), 100, {-2});)
    CASE("split F=3 (fs=0) P=2 rank 0 overlap K=3", peers_say(); return runs(split_engine(0, 2, 1), 3, {3});)
    CASE("split F=3 (fs=0) P=4 rank 3 K=2", peers_say(); return runs(split_engine(3, 4, 0), 3, {-2});)
    CASE("split F=100 dropout P=2 rank 0 overlap", peers_say(); appnp_dist* d = split_engine(0, 2, 1); Run r(d, 100, 2);
         r.p_drop = 0.5f; const int rc = r.go(); destroy(d); return rc;)
    CASE("split H misaligned (staged in)", peers_say(); appnp_dist* d = split_engine(0, 2, 1); Run r(d, 100, 2);
         r.H = off(kH, 8); const int rc = r.go(); destroy(d); return rc;)
    CASE("split ld_z misaligned (staged out)", peers_say(); appnp_dist* d = split_engine(1, 2, 1); Run r(d, 100, 2);
         r.ld_z = 101; const int rc = r.go(); destroy(d); return rc;)
    CASE("split H and ld_z misaligned, no overlap", peers_say(); appnp_dist* d = split_engine(1, 2, 0); Run r(d, 100, 3);
         r.ld_h = 102; r.ld_z = 101; const int rc = brief(r); destroy(d); return rc;)
    CASE("split bf16 on a graph with a copy: whole rows", peers_say(); return runs(split_engine(0, 2, 0), 100, {-2}, APPNP_BF16);)
    // ---- split layout, pipelined -----------------------------------------------------------
    CASE("split pipelined F=100 P=3 rank 1 K=3", peers_say(); return runs(split_engine(1, 3, 1, true), 100, {3});)
    CASE("split pipelined F=100 P=5 rank 4 K=2", peers_say(); return runs(split_engine(4, 5, 1, true), 100, {-2});)
    CASE("split pipelined F=100 P=5 rank 0 K=1 (whole rows, pipelined)", peers_say(); return runs(split_engine(0, 5, 1, true), 100, {-1});)
    CASE("split F=3 with a broadcast set takes the all-gather loop", peers_say(); return runs(split_engine(2, 3, 1, true), 3, {-3});)
    CASE("split pipelined, H and ld_z misaligned", peers_say(); appnp_dist* d = split_engine(0, 3, 1, true); Run r(d, 100, 2);
         r.H = off(kH, 4); r.ld_z = 103; const int rc = brief(r); destroy(d); return rc;)
    // ---- the agreement ---------------------------------------------------------------------
    CASE("agreement: every peer built the copy; the second call does not agree again", peers_say();
         appnp_dist* d = split_engine(1, 4, 1); brief(Run(d, 100, 2)); brief(Run(d, 100, 2)); destroy(d); return APPNP_OK;)
    CASE("agreement: one peer did not", peers_say(2);
         appnp_dist* d = split_engine(1, 4, 1); brief(Run(d, 100, 2)); brief(Run(d, 100, 2)); destroy(d); return APPNP_OK;)
    CASE("agreement: this rank did not", g_show_setup = true; peers_say(1); appnp::g_build_rc = APPNP_ENOMEM; appnp_dist* d = split_engine(1, 4, 1);
         appnp::g_build_rc = APPNP_OK; brief(Run(d, 100, 2)); brief(Run(d, 100, 2)); destroy(d); return APPNP_OK;)
    CASE("agreement: bf16 and K=1 calls first, then the fp32 K=3 call agrees", peers_say(); appnp_dist* d = split_engine(0, 2, 0);
         brief(Run(d, 100, 2, APPNP_BF16)); brief(Run(d, 100, 1)); return runs(d, 100, {-3});)
    CASE("agreement: workspace too small", peers_say(); appnp_dist* d = engine(0, 8, 0, false, W4, 5); Run r(d, 3, 2);
         r.go(); r.ws_bytes = 1; r.go(); r.ws_bytes = 8 * 256 - 1; r.go(); r.ws_bytes = 8 * 256; const int rc = r.go(); destroy(d); return rc;)
    CASE("agreement: null workspace", peers_say(); appnp_dist* d = split_engine(0, 2, 0); Run r(d, 100, 2);
         r.ws = nullptr; const int rc = r.go(); destroy(d); return rc;)
    CASE("agreement: the callback fails inside it", peers_say(); appnp_dist* d = split_engine(0, 2, 1); g_xchg = 0; g_fail_xchg = 1;
         Run(d, 100, 2).go(); g_fail_xchg = 0; return runs(d, 100, {2});)
    CASE("agreement: injected failure poisons the handle", peers_say(); appnp_dist* d = split_engine(0, 3, 1);
         setenv("APPNP_DIST_TEST_AGREE_FAIL", "1", 1); Run(d, 100, 2).go(); unsetenv("APPNP_DIST_TEST_AGREE_FAIL");
         Run(d, 100, 2).go(); Run(d, 64, 0).go();
         printf("set_broadcast -> %d\n", appnp_dist_set_broadcast(d, bcast_cb, kBctx, kStream));
         destroy(d); return APPNP_OK;)
    CASE("agreement: injection variable set to 0 does nothing", peers_say(); appnp_dist* d = split_engine(0, 2, 0);
         setenv("APPNP_DIST_TEST_AGREE_FAIL", "0", 1); const int rc = Run(d, 100, 2).go(); unsetenv("APPNP_DIST_TEST_AGREE_FAIL");
         destroy(d); return rc;)
    // ---- queries ---------------------------------------------------------------------------
    CASE("workspace_bytes",
         for (int P : {1, 3}) for (int overlap : {0, 1}) for (int mode : {0, W4, W8, W16}) for (int built : {1, 0}) {
           if (!mode && !built) continue;
           appnp_dist* d = nullptr;
           {
             Mute m;
             appnp::g_build_rc = built ? APPNP_OK : APPNP_ENOMEM;
             d = engine(P - 1, P, overlap, false, mode, kNs);
             appnp::g_build_rc = APPNP_OK;
           }
           printf("P=%d overlap=%d mode=%#x built=%d f32/bf16 at F=3,13,20,40,64,100:", P, overlap, mode, built);
           for (int64_t f : {3, 13, 20, 40, 64, 100})
             printf(" %zu/%zu", appnp_dist_workspace_bytes(d, f, APPNP_F32), appnp_dist_workspace_bytes(d, f, APPNP_BF16));
           printf("\n");
           Mute m;
           destroy(d);
         }
         return APPNP_OK;)
    CASE("rows",
         for (int P : {1, 2, 3, 8}) for (int r = 0; r < P; ++r) {
           int64_t lo = -1, hi = -1, shard = -1;
           Mute* m = new Mute;
           appnp_dist* d = engine(r, P, 0);
           const int rc = appnp_dist_rows(d, &lo, &hi, &shard);
           const bool graph = appnp_dist_graph(d) != nullptr;
           destroy(d);
           delete m;
           printf("rows P=%d rank=%d -> %d [%" PRId64 ", %" PRId64 ") shard=%" PRId64 " graph=%d\n", P, r, rc, lo, hi,
                  shard, (int)graph);
         }
         appnp_dist* d = engine(7, 8, 0, false, 0, 5);  // more ranks than rows: an empty shard
         int64_t lo = -1, hi = -1, shard = -1;
         printf("rows -> %d", appnp_dist_rows(d, &lo, &hi, &shard));
         printf(" [%" PRId64 ", %" PRId64 ") shard=%" PRId64 "\n", lo, hi, shard);
         printf("rows with null outs -> %d\n", appnp_dist_rows(d, nullptr, nullptr, nullptr));
         return runs(d, 64, {2});)
    CASE("pipeline_groups",
         for (int R = 3; R <= 17; ++R) {
          printf("pipeline_groups R=%d:", R);
          for (int ri = 0; ri < R; ++ri) {
           int lo[8], hi[8], n = -1, rc;
           {
             Mute m;
             appnp_dist* d = engine(ri, R, 1, true);
             rc = appnp_dist_pipeline_groups(d, lo, hi, 8, &n);
             destroy(d);
           }
           if (rc != APPNP_OK) return rc;
           for (int i = 0; i < n && i < 8; ++i) printf("%s%d-%d", i ? "," : " ", lo[i], hi[i]);  // rank ri
          }
          printf("\n");
         }
         return APPNP_OK;)
    CASE("pipeline_groups: max smaller than the count, null arrays",
         appnp_dist* d = engine(3, 8, 1, true); int lo[2] = {-1, -1}, hi[2] = {-1, -1}, n = -1;
         int rc = appnp_dist_pipeline_groups(d, lo, hi, 2, &n);
         printf("max=2 -> %d n=%d %d-%d %d-%d\n", rc, n, lo[0], hi[0], lo[1], hi[1]);
         rc = appnp_dist_pipeline_groups(d, nullptr, nullptr, 8, &n);
         printf("null arrays -> %d n=%d\n", rc, n);
         destroy(d); return rc;)
    // ---- rejected arguments ----------------------------------------------------------------
    CASE("rejected: create",
         appnp_dist* d = at<appnp_dist>(0xbad0);
         const int32_t* ip = at<int32_t>(0x70000000); const int32_t* ix = at<int32_t>(0x71000000);
         printf("rejected-begin\n");
         rc_line("null out", appnp_dist_create(ip, ix, nullptr, kN, 25 * kN, 0, 0, 2, 0, allgather_cb, kCtx, kStream, nullptr));
         rc_line("n = 0", appnp_dist_create(ip, ix, nullptr, 0, 0, 0, 0, 2, 0, allgather_cb, kCtx, kStream, &d));
         rc_line("out after a rejection is null", d == nullptr);
         rc_line("n < 0", appnp_dist_create(ip, ix, nullptr, -1, 0, 0, 0, 2, 0, allgather_cb, kCtx, kStream, &d));
         rc_line("nranks = 0", appnp_dist_create(ip, ix, nullptr, kN, 25 * kN, 0, 0, 0, 0, allgather_cb, kCtx, kStream, &d));
         rc_line("rank < 0", appnp_dist_create(ip, ix, nullptr, kN, 25 * kN, 0, -1, 2, 0, allgather_cb, kCtx, kStream, &d));
         rc_line("rank = nranks", appnp_dist_create(ip, ix, nullptr, kN, 25 * kN, 0, 2, 2, 0, allgather_cb, kCtx, kStream, &d));
         rc_line("P = 2 without a callback", appnp_dist_create(ip, ix, nullptr, kN, 25 * kN, 0, 0, 2, 0, nullptr, kCtx, kStream, &d));
         rc_line("nnz < 0", appnp_dist_create(ip, ix, nullptr, kN, -1, 0, 0, 2, 0, allgather_cb, kCtx, kStream, &d));
         rc_line("n > INT32_MAX", appnp_dist_create(ip, ix, nullptr, (int64_t)INT32_MAX + 1, 8, 0, 0, 2, 0, allgather_cb, kCtx, kStream, &d));
         rc_line("bad norm", appnp_dist_create(ip, ix, nullptr, kN, 25 * kN, 2, 0, 2, 0, allgather_cb, kCtx, kStream, &d));
         rc_line("transpose of held rows", appnp_dist_create(ip, ix, nullptr, kN, 25 * kN, APPNP_GRAPH_TRANSPOSE, 1, 2, 0, allgather_cb, kCtx, kStream, &d));
         rc_line("null indptr", appnp_dist_create(nullptr, ix, nullptr, kN, 25 * kN, 0, 0, 2, 0, allgather_cb, kCtx, kStream, &d));
         rc_line("null indices", appnp_dist_create(ip, nullptr, nullptr, kN, 25 * kN, 0, 0, 2, 0, allgather_cb, kCtx, kStream, &d));
         rc_line("out is null", d == nullptr);
         printf("rejected-end\n");
         // one rank needs no callback
         const int rc = appnp_dist_create(ip, ix, nullptr, kN, 25 * kN, 0, 0, 1, 0, nullptr, nullptr, kStream, &d);
         destroy(d); return rc;)
    CASE("rejected: a device error in the blocked copy fails the creation", appnp::g_build_rc = APPNP_EDEVICE;
         appnp_dist* d = split_engine(0, 2, 1); appnp::g_build_rc = APPNP_OK; return d == nullptr ? APPNP_OK : APPNP_EDEVICE;)
    CASE("rejected: propagate",
         appnp_dist* d = engine(0, 2, 0); appnp_dist* o = engine(0, 2, 1);
         const size_t need = appnp_dist_workspace_bytes(d, 64, APPNP_F32);
         printf("rejected-begin\n");
         rc_line("null engine", appnp_dist_propagate(nullptr, kH, 64, kZ, 64, 64, 0, 3, .1f, 0.f, 42, kWs, need, kStream));
         rc_line("f < 0", appnp_dist_propagate(d, kH, 64, kZ, 64, -1, 0, 3, .1f, 0.f, 42, kWs, need, kStream));
         rc_line("K < 0", appnp_dist_propagate(d, kH, 64, kZ, 64, 64, 0, -1, .1f, 0.f, 42, kWs, need, kStream));
         rc_line("bad dtype", appnp_dist_propagate(d, kH, 64, kZ, 64, 64, 2, 3, .1f, 0.f, 42, kWs, need, kStream));
         rc_line("bf16 with overlap", appnp_dist_propagate(o, kH, 64, kZ, 64, 64, APPNP_BF16, 3, .1f, 0.f, 42, kWs, need, kStream));
         rc_line("alpha < 0", appnp_dist_propagate(d, kH, 64, kZ, 64, 64, 0, 3, -.1f, 0.f, 42, kWs, need, kStream));
         rc_line("alpha > 1", appnp_dist_propagate(d, kH, 64, kZ, 64, 64, 0, 3, 1.5f, 0.f, 42, kWs, need, kStream));
         rc_line("alpha NaN", appnp_dist_propagate(d, kH, 64, kZ, 64, 64, 0, 3, std::numeric_limits<float>::quiet_NaN(), 0.f, 42, kWs, need, kStream));
         rc_line("p_drop < 0", appnp_dist_propagate(d, kH, 64, kZ, 64, 64, 0, 3, .1f, -.1f, 42, kWs, need, kStream));
         rc_line("p_drop = 1", appnp_dist_propagate(d, kH, 64, kZ, 64, 64, 0, 3, .1f, 1.f, 42, kWs, need, kStream));
         rc_line("p_drop NaN", appnp_dist_propagate(d, kH, 64, kZ, 64, 64, 0, 3, .1f, std::numeric_limits<float>::quiet_NaN(), 42, kWs, need, kStream));
         rc_line("f = 0 with null operands is a no-op", appnp_dist_propagate(d, nullptr, 0, nullptr, 0, 0, 0, 3, .1f, 0.f, 42, nullptr, 0, kStream));
         rc_line("null H", appnp_dist_propagate(d, nullptr, 64, kZ, 64, 64, 0, 3, .1f, 0.f, 42, kWs, need, kStream));
         rc_line("null Z", appnp_dist_propagate(d, kH, 64, nullptr, 64, 64, 0, 3, .1f, 0.f, 42, kWs, need, kStream));
         rc_line("ld_h < f", appnp_dist_propagate(d, kH, 63, kZ, 64, 64, 0, 3, .1f, 0.f, 42, kWs, need, kStream));
         rc_line("ld_z < f", appnp_dist_propagate(d, kH, 64, kZ, 63, 64, 0, 3, .1f, 0.f, 42, kWs, need, kStream));
         rc_line("null ws", appnp_dist_propagate(d, kH, 64, kZ, 64, 64, 0, 3, .1f, 0.f, 42, nullptr, need, kStream));
         rc_line("ws one byte short", appnp_dist_propagate(d, kH, 64, kZ, 64, 64, 0, 3, .1f, 0.f, 42, kWs, need - 1, kStream));
         rc_line("ws one byte short, overlap", appnp_dist_propagate(o, kH, 64, kZ, 64, 64, 0, 3, .1f, 0.f, 42, kWs, appnp_dist_workspace_bytes(o, 64, 0) - 1, kStream));
         printf("rejected-end\n");
         // exactly enough
         const int rc = appnp_dist_propagate(d, kH, 64, kZ, 64, 64, 0, 1, .1f, 0.f, 42, kWs, need, kStream);
         destroy(o); destroy(d); return rc;)
    CASE("rejected: propagate on the split layout", peers_say();
         appnp_dist* d = split_engine(0, 2, 1); Run r(d, 100, 2); brief(r);  // agrees
         const size_t need = appnp_dist_workspace_bytes(d, 100, APPNP_F32);
         printf("rejected-begin\n");
         rc_line("null ws", appnp_dist_propagate(d, kH, 100, kZ, 100, 100, 0, 2, .1f, 0.f, 42, nullptr, need, kStream));
         rc_line("ws one byte short", appnp_dist_propagate(d, kH, 100, kZ, 100, 100, 0, 2, .1f, 0.f, 42, kWs, need - 1, kStream));
         rc_line("K = 1: whole rows need theirs too", appnp_dist_propagate(d, kH, 100, kZ, 100, 100, 0, 1, .1f, 0.f, 42, kWs, 0, kStream));
         printf("rejected-end\n");
         destroy(d); return APPNP_OK;)
    CASE("rejected: set_broadcast, pipeline_groups, workspace_bytes",
         appnp_dist* d = engine(0, 3, 1); appnp_dist* two = engine(0, 2, 1); appnp_dist* plain = engine(0, 3, 0);
         int n = -1;
         printf("rejected-begin\n");
         rc_line("set_broadcast null engine", appnp_dist_set_broadcast(nullptr, bcast_cb, kBctx, kStream));
         rc_line("set_broadcast null callback", appnp_dist_set_broadcast(d, nullptr, kBctx, kStream));
         rc_line("set_broadcast without overlap", appnp_dist_set_broadcast(plain, bcast_cb, kBctx, kStream));
         rc_line("set_broadcast P = 2", appnp_dist_set_broadcast(two, bcast_cb, kBctx, kStream));
         rc_line("pipeline_groups null engine", appnp_dist_pipeline_groups(nullptr, nullptr, nullptr, 0, &n));
         rc_line("pipeline_groups null count", appnp_dist_pipeline_groups(d, nullptr, nullptr, 0, nullptr));
         rc_line("pipeline_groups before a broadcast is set", appnp_dist_pipeline_groups(d, nullptr, nullptr, 0, &n));
         rc_line("its count", n);
         rc_line("workspace_bytes null engine", (long long)appnp_dist_workspace_bytes(nullptr, 64, 0));
         rc_line("workspace_bytes f = 0", (long long)appnp_dist_workspace_bytes(d, 0, 0));
         rc_line("workspace_bytes f < 0", (long long)appnp_dist_workspace_bytes(d, -1, 0));
         rc_line("workspace_bytes bad dtype", (long long)appnp_dist_workspace_bytes(d, 64, 2));
         rc_line("rows null engine", appnp_dist_rows(nullptr, nullptr, nullptr, nullptr));
         rc_line("graph null engine", appnp_dist_graph(nullptr) != nullptr);
         printf("rejected-end\n");
         appnp_dist_destroy(nullptr);
         destroy(plain); destroy(two); destroy(d); return APPNP_OK;)
    // ---- timer and teardown ----------------------------------------------------------------
    CASE("timer: rows, all-gather with overlap", return timed(Run(engine(1, 3, 1), 64, 2));)
    CASE("timer: rows, pipelined", return timed(Run(engine(1, 3, 1, true), 64, 2));)
    CASE("timer: split, all-gather with overlap", peers_say(); appnp_dist* d = split_engine(1, 3, 1);
         { Mute m; Run(d, 100, 2).go(); } return timed(Run(d, 100, 2));)
    CASE("timer: split, pipelined", peers_say(); appnp_dist* d = split_engine(1, 3, 1, true);
         { Mute m; Run(d, 100, 2).go(); } return timed(Run(d, 100, 2));)
    CASE("set_broadcast twice replaces the events", g_show_setup = true; appnp_dist* d = engine(0, 3, 1, true);
         printf("set_broadcast -> %d\n", appnp_dist_set_broadcast(d, bcast_cb, kCtx, kStream));
         destroy(d); return APPNP_OK;)
    CASE("create and destroy: W8 copy, broadcast set", g_show_setup = true; destroy(split_engine(1, 3, 1, true, W8)); return APPNP_OK;)
    CASE("destroy without a broadcast set", g_show_setup = true; destroy(engine(0, 3, 1)); return APPNP_OK;)
    CASE("destroy without overlap", g_show_setup = true; destroy(engine(0, 3, 0)); return APPNP_OK;)
    // ---- failure paths (brief form) --------------------------------------------------------
    CASE("failures: rows, all-gather, P=3 rank 1 K=2", return failures(engine(1, 3, 1), 64);)
    CASE("failures: rows, all-gather without overlap, P=3 rank 1 K=2", return failures(engine(1, 3, 0), 64);)
    CASE("failures: rows, pipelined, P=3 rank 1 K=2", return failures(engine(1, 3, 1, true), 64);)
    CASE("failures: split, all-gather, P=3 rank 1 K=2", peers_say(); return failures(split_engine(1, 3, 1), 100);)
    CASE("failures: split, pipelined, P=3 rank 1 K=2", peers_say(); return failures(split_engine(1, 3, 1, true), 100);)
};

}  // namespace

int main() {
  for (const Case& c : kCases) {
    printf("# %s\n", c.name);
    g_next_handle = 0xe0000000u;
    g_peer_flags = nullptr;
    g_show_setup = false;
    const int rc = c.run();
    printf("-> %d\n", rc);
  }
  return 0;
}
