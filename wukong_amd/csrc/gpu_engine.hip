/*
 * gpu_engine.hip — the MI355X-native per-pattern graph-exploration engine.
 *
 * Hand-written CDNA4 HIP kernels (gfx950) replacing the reference's CUDA
 * pipeline (core/gpu/gpu_hash.cu, gpu_engine_cuda.hpp) with an
 * HBM-resident full store (no segment cache / block mapping).  Operator
 * semantics restate core/engine/sparql.hpp:80-549.
 *
 * Execution model: a query is ONE asynchronous launch chain — row counts
 * live in device memory (d_state) and every kernel reads its bounds from
 * there, so the host never synchronizes between patterns (the reference's
 * GPU pipeline synced per step, gpu_engine_cuda.hpp:168-197).  Scratch is
 * sized to a grow-only row capacity; expansion overflow raises a device
 * flag and the query is re-run at the larger capacity (replaces the
 * reference's hard 32 MB rbuf assert, gpu_engine_cuda.hpp:185).
 *
 * Kernel inventory (device code lives in the wk_kernels_*.h headers,
 * included below: one translation unit):
 *  wk_kernels_common.h
 *   probe_one/probe_chain, bsearch_u32, tbm_has, csr_entry,
 *   typeof_nodrop_ok — lookup helpers; d_state words and categories;
 *   chain_eval (row-major, early exit) and chain_eval_batch (op-major,
 *   K candidates of compile-time width W, no early exit) — the per-row
 *   op chain evaluators
 *  wk_kernels_expand.h
 *   k_probe_scan      — fused gen-keys + thread-per-row cluster-hash
 *                       probe + in-kernel prefix scan (2-deep bucket
 *                       prefetch); replaces gpu_hash.cu:94-324
 *   k_csr_gather      — 24-B rank-compressed CSR probes for
 *                       non-functional segments (vs 128-B bucket walks)
 *   k_csr_gather_tf, k_expand_tf[_big] — EXACT fused k2u + typeof
 *                       compaction over the CSR index (count pass ->
 *                       scan -> filtered write)
 *   k_csr_gather_chain, k_expand_chain[_big] — the same exact pipeline
 *                       with a per-row op chain (chain_t: fn-map
 *                       lookups, bitmap type tests, equality tests of
 *                       the FOLLOWING patterns) as the per-edge predicate;
 *                       the count pass evaluates it op-major on 2 rows x
 *                       4 edges per thread (chain_eval_batch, clamped
 *                       unconditional loads) and leaves a 32-bit pass
 *                       mask per row, from which the writer emits
 *   k_row_chain       — a run of >= 2 per-row patterns with no expansion
 *                       in front as ONE pass over the table: op-major
 *                       evaluation of 4 rows per thread + ballot
 *                       compaction at the widened width (Q1's body)
 *                       (k_row_chain, k_csr_gather_chain, k_expand_chain
 *                       are instantiated <NC, W>: candidate rows are 4
 *                       columns wide when the plan's widened row fits,
 *                       else 8; WK_CHAIN_WIDTH=8 forces 8)
 *   k_scan_local/mid  — chunked exclusive scan with DEVICE-side length
 *                       (replaces the thrust scans, gpu_hash.cu:587-596):
 *                       several elements per thread, wave scan, one
 *                       barrier per tile; k_scan_mid also commits the
 *                       step (S_INROWS snapshot for the scatter side)
 *   k_expand_in/big   — input-centric expansion + wave-per-big-row pass
 *                       (replaces gpu_hash.cu:762-834; no 20-col cap),
 *                       optional inline no-drop typeof verify in graphs
 *   k_fn_gather/k_fn_scatter — functional-predicate rank-compressed
 *                       map k2u (deg==1 segments; page+value gathers);
 *                       k_expand_fn_map = optimistic 1:1 inside graphs
 *   k_commit, k_set_state, k_begin_state, k_zero_words,
 *   k_publish_state, k_publish_begin, k_project — 1-thread state
 *                       kernels, projection.
 *                       A query's begin zeroing rides on its first state
 *                       write (k_begin_state); the optimistic kernels
 *                       count guard misses into the sticky S_DONE word,
 *                       which k_publish_state alone turns into S_ERR —
 *                       no per-step commit for steps that keep the row
 *                       count
 *  wk_kernels_filter.h
 *   k_filter_tpr      — fused probe/typeof filter + block compaction
 *                       (replaces gpu_hash.cu:326-445,523-585);
 *                       per-type bitmaps: rdf:type filters read
 *                       1 bit/vid (LLC-resident); the bitmap, PM_EQ and
 *                       functional-map paths evaluate a thread's 4 rows
 *                       op-major (filter_keep_batch; WK_FILTER_BATCH=0:
 *                       row after row)
 *   k_filter_expr     — FILTER expressions (=, !=, bound, &&, ||, !) as a
 *                       postfix program with a register bit-stack, same
 *                       compaction; pushed down behind the pattern that
 *                       binds a conjunct's last variable (§3 5j)
 *   k_vu              — VERSATILE predicate-variable ops over the dense
 *                       vp CSR (sparql.hpp:556-744)
 *   k_expand_opt / k_filter_opt — OPTIONAL-group ops (BLANK fill,
 *                       matched flags; sparql.hpp:100-170,316-375)
 *  wk_kernels_batch.h
 *   k_dst_count/scan2/scatter2 — fork-join radix split by vid % ndst
 *                       (replaces gpu_hash.cu:600-760)
 *   k_light2          — whole-query single-kernel path for 2-pattern
 *                       light templates (emulator A1/A2/A3/A5)
 *   k_light_batch     — batched light-query window (one wavefront
 *                       workgroup per query; proxy.hpp:477-525 window)
 *   k_plan_batch      — LDS plan interpreter: whole multi-pattern
 *                       const-start templates, binding table in LDS
 *   k_peer_step       — xGMI peer-probe small-table step
 *  wk_kernels_final.h
 *   k_fin_live/hist/scan/scatter — DISTINCT as a stable LSD radix sort of
 *                       a row-index permutation (8-bit digits, constant
 *                       digits skipped on the device); k_fin_flag/emit —
 *                       adjacent dedup + OFFSET/LIMIT window + projection
 *                       in one compaction; k_fin_window — the window
 *                       alone (replaces the host final_process,
 *                       sparql.hpp:1424-1551; captured into graphs)
 *  host side (this file)
 *   zero-copy i2u/c2u — the 1-col start table IS the stored edge list
 *                       (read-only view, no copy kernel)
 *   hipGraph replay   — wk_engine_graph_build/run/launch: a fixed plan
 *                       replays as ONE launch, with warm-pass-derived
 *                       no-drop specialization verified on every replay;
 *                       patterns the warm pass saw run on an empty
 *                       table are host bookkeeping only (empty-tail
 *                       truncation, guarded by the publish)
 */
#include "wk_store.h"
#include "../../include/wukong_abi.h"

#include <hip/hip_runtime.h>

#include <vector>
#include <algorithm>
#include <cstring>
#include <cstdio>
#include <cstdlib>
#include <chrono>
#include <type_traits>

static double now_us() {
    return std::chrono::duration<double, std::micro>(
               std::chrono::steady_clock::now().time_since_epoch()).count();
}
static int wk_verbose_lvl() {
    static int v = -1;
    if (v < 0) { const char *e = getenv("WK_VERBOSE"); v = e ? atoi(e) : 0; }
    return v;
}

using namespace wk;

#define HIP_CHECK(x)                                                        \
    do {                                                                    \
        hipError_t err_ = (x);                                              \
        if (err_ != hipSuccess) {                                           \
            fprintf(stderr, "HIP error %s at %s:%d: %s\n", #x, __FILE__,    \
                    __LINE__, hipGetErrorString(err_));                     \
            return WK_ERR_HIP;                                              \
        }                                                                   \
    } while (0)

enum {
    WK_OK = 0,
    WK_ERR_HIP = -2,
    WK_ERR_PLAN = -3,
    WK_ERR_STATE = -4,
    WK_ERR_CAP = -5,
};

#include "wk_kernels_common.h"
#include "wk_kernels_expand.h"
#include "wk_kernels_filter.h"
#include "wk_kernels_batch.h"
#include "wk_kernels_final.h"

// ---------------------------------------------------------------------
// engine
// ---------------------------------------------------------------------

namespace {

struct devbuf {
    void *p = nullptr;
    size_t cap = 0;
    devbuf() = default;
    devbuf(const devbuf &) = delete;
    devbuf &operator=(const devbuf &) = delete;
    ~devbuf() { release(); }  // locals (e.g. run_union's snapshot) free
                              // on every early-return path
    int ensure(size_t bytes) {
        if (bytes <= cap) return WK_OK;
        if (p) (void)hipFree(p);
        p = nullptr; cap = 0;
        if (hipMalloc(&p, bytes) != hipSuccess) return WK_ERR_HIP;
        cap = bytes;
        return WK_OK;
    }
    void release() { if (p) (void)hipFree(p); p = nullptr; cap = 0; }
};

struct timed_launch {
    hipEvent_t start, stop;
    int cat;
};

}  // namespace

// device-resident store image, shared by any number of engines on one
// GPU (one upload; engines add only their scratch — replaces the
// reference's per-agent GPUCache, core/gpu/gpu_cache.hpp)
struct wk_gpu_store {
    const wk_store *st = nullptr;
    int device = 0;
    vertex_t *d_verts = nullptr;
    sid_t *d_edges = nullptr;
    uint16_t *d_type_of = nullptr;
    // VERSATILE dense CSR (per-vertex predicate lists) + the per-
    // (pid,dir) segment table the predicate-variable ops probe through
    uint32_t *d_vp_off[2] = {nullptr, nullptr};
    sid_t *d_vp_edges[2] = {nullptr, nullptr};
    seg_t *d_segtab = nullptr;
    // functional-predicate rank-compressed maps, indexed [pid*2+dir]
    // (host vectors of device pointers; null = absent): presence-bitmap
    // pages + packed values (wk_types.h fnpage_t)
    std::vector<fnpage_t *> d_fn_pages;
    std::vector<sid_t *> d_fn_vals;
    // rank-compressed CSR side index for non-functional segments:
    // pages + u64 {edge_off:40|len:24} entries (24-B probes)
    std::vector<fnpage_t *> d_csr_pages;
    std::vector<uint64_t *> d_csr_entries;
    // per-type membership bitmaps (LLC-resident typeof filters)
    std::vector<uint64_t *> d_tbm;
    // xGMI peer mappings of the other ranks' stores (HIP IPC) — the
    // small-table remote-read path (k_peer_step); empty = not imported
    std::vector<wk_peer_desc> peers;            // host copy, [nsrv]
    std::vector<std::vector<seg_t>> peer_nseg;  // [nsrv][pid*2+dir]
    wk_peer_desc *d_peers = nullptr;            // device array [nsrv]
    std::vector<void *> ipc_opened;             // to close on destroy
    int refs = 0;     // engines attached
    bool owned = false;  // created implicitly by wk_engine_create
};

struct wk_engine {
    const wk_store *st = nullptr;
    wk_gpu_store *gs = nullptr;
    int device = 0;
    hipStream_t stream = nullptr;

    // device store (borrowed from gs)
    vertex_t *d_verts = nullptr;
    sid_t *d_edges = nullptr;
    uint16_t *d_type_of = nullptr;

    // dual result buffer (gpu_mem.hpp:116-124) + scratch, all sized by
    // cap_rows (grow-only; overflow -> re-run)
    devbuf tbl[2];
    devbuf eoff, cnt, pmask, prefix, bsums, misc, ovf;
    devbuf fhist;  // final ops: block x digit histograms (by cap_rows)
    int64_t cap_rows = 0;
    int cap_cols = 0;

    uint64_t *d_state = nullptr;  // S_WORDS words
    uint64_t *d_stats = nullptr;  // CAT_COUNT words (algorithmic bytes)
    uint64_t *d_fin = nullptr;    // F_WORDS words (final-ops state)
    uint64_t *h_pin = nullptr;    // pinned: state + stats snapshot
    void *h_stage = nullptr;      // pinned staging for result downloads
    size_t h_stage_cap = 0;

    int cur = 0;
    int64_t nrows = 0;   // valid only after a sync point
    int ncols = 0;
    int64_t bound = 0;   // host-side upper bound on rows (grid sizing)

    bool light = false;  // single-kernel fast path ran (h_pin self-published)
    // begin_query's d_state zeroing, deferred so the query's first state
    // write (k_begin_state) performs it; any other first launch flushes
    // it with k_zero_words (flush_begin)
    bool zero_pending = false;
    // suite capture: the previous query's publish (value = its
    // expect_empty; -1 = none), held back so the next query's
    // k_begin_state can take it along (k_publish_begin)
    int publish_pending = -1;
    bool hinting = false;  // graph-build hint pass: per-PATTERN row counts
                           // needed, so multi-step fusions are disabled
    int remote_step_idx = -1;  // pattern to run via the xGMI peer path
    // a WHOLE plan is being run (wk_engine_submit / wk_engine_run_query,
    // captures included): the only place multi-pattern op chains apply —
    // the step API and UNION/OPTIONAL continuations keep per-pattern steps
    bool whole_plan = false;
    // zero-copy i2u/c2u: the 1-col start table IS the (immutable) edge
    // list in the store — later steps read it in place instead of
    // replaying a 25-MB k_copy_list per query.  Cleared on every table
    // flip/load; materialised before any in-place writer (OPT groups).
    const sid_t *tbl_view = nullptr;

    // final ops of the CURRENT table.  fin_count: the
    // post-final row count of the last non-blind fetch or final-op replay
    // (-1 = none); fin_table: the finalized, projected table for fin_sig
    // sits in tbl[cur ^ 1].  Both are dropped by whatever changes the
    // current table (fin_invalidate).
    struct fin_sig_t {
        int32_t distinct = 0, nrequired = 0;
        int64_t limit = -1, offset = 0;
        int32_t req[8] = {0};
        bool operator==(const fin_sig_t &o) const {
            return distinct == o.distinct && nrequired == o.nrequired &&
                   limit == o.limit && offset == o.offset &&
                   !memcmp(req, o.req, sizeof(req));
        }
    };
    int64_t fin_count = -1;
    bool fin_table = false;
    fin_sig_t fin_sig;

    // OPTIONAL group execution state (wk_engine_run_query only)
    devbuf oflag[2];          // per-row matched flags (u8), ping-pong
    int opt_mode = 0;         // inside an OPTIONAL pattern group
    int ocur = 0;             // which oflag is current
    uint32_t opt_mask = 0;    // columns first bound inside the group

    // batched light-query window (wk_engine_submit_light_batch)
    devbuf lbd;               // device light_desc array
    devbuf lbcnt;             // device per-query counts
    uint64_t *h_lb = nullptr; // pinned: descs/consts staging, then counts
    size_t h_lb_cap = 0;
    size_t lb_coff = 0;       // byte offset of the counts region in h_lb
    int lb_n = -1;            // queries in flight in the batch (-1 = none)

    // query state (host mirror of SPARQLQuery, query.hpp:560-594)
    std::vector<wk_pattern_t> pats;
    std::vector<int32_t> v2c;  // idx -> col (query.hpp:352-374)
    int nvars = 0;
    int step = 0;
    // FILTER program of the current plan (validated by begin_query) and
    // its top-level conjuncts.  after = index of the main-BGP pattern the
    // conjunct runs behind (pushdown); -1 = the
    // reference position, once after UNION/OPTIONAL (run_query only)
    struct fconj { std::vector<wk_fnode_t> prog; int after; };
    std::vector<wk_fnode_t> filt;
    std::vector<fconj> conj;

    // hipGraph replay of whole fixed plans (wk_engine_graph_build/run)
    struct wk_graph {
        hipGraphExec_t exec = nullptr;
        std::vector<int32_t> v2c;
        int ncols = 0, cur = 0, nvars = 0;
        int64_t bound = 0;
        bool light = false;
        const sid_t *view = nullptr;  // final table is a zero-copy view
        bool fin = false;  // the chain ends with the final pass (fin_sig)
        fin_sig_t fin_sig;
    };
    std::vector<wk_graph> graphs;
    int capturing = 0;
    // per-pattern-step no-drop hints from the graph build's warm pass
    // (consulted ONLY while capturing)
    std::vector<uint8_t> capture_hint;
    // last pattern to execute while capturing: the warm pass saw the
    // table empty from there to the end of the plan (-1 = run them all)
    int capture_empty_after = -1;

    // timing (WK_KERNEL_TIMING=1)
    bool timing = false;
    std::vector<timed_launch> pending;
    double cat_usec[CAT_COUNT] = {0};
    double cat_bytes[CAT_COUNT] = {0};
    int64_t cat_n[CAT_COUNT] = {0};

    int var2col(ssid_t v) const { return v < 0 ? v2c[-(v + 1)] : -1; }
    int var_stat(ssid_t v) const { return v >= 0 ? 2 : (var2col(v) >= 0 ? 1 : 0); }
};

static const int BLOCK = 256;
static_assert(BLOCK == SCAN_T, "kernels declare __launch_bounds__(SCAN_T)");
static inline const sid_t *cur_table(wk_engine *e);
static int grid_for(int64_t work) {
    int64_t g = (work + BLOCK - 1) / BLOCK;
    return (int)(g < 1 ? 1 : (g > 2048 ? 2048 : g));
}
static inline const sid_t *cur_table(wk_engine *e) {
    return e->tbl_view ? e->tbl_view : (const sid_t *)e->tbl[e->cur].p;
}
// copy a zero-copy i2u view into the owned table buffer (needed before
// any in-place writer, e.g. the OPTIONAL-group BLANK fill)
static int32_t materialize_view(wk_engine *e) {
    if (!e->tbl_view) return WK_OK;
    size_t bytes = (size_t)std::max<int64_t>(e->nrows, 0) *
                   std::max(e->ncols, 1) * 4;
    if (bytes &&
        hipMemcpyAsync(e->tbl[e->cur].p, e->tbl_view, bytes,
                       hipMemcpyDeviceToDevice, e->stream) != hipSuccess)
        return WK_ERR_HIP;
    e->tbl_view = nullptr;
    return WK_OK;
}
static inline void fin_invalidate(wk_engine *e) {
    e->fin_count = -1;
    e->fin_table = false;
}
// blocks of the final-ops histogram/scatter grid: fixed by the capacity
static int fin_grid(int64_t cap_rows) {
    int64_t g = (cap_rows + BLOCK - 1) / BLOCK;
    return (int)(g < 1 ? 1 : (g > FIN_MAXB ? FIN_MAXB : g));
}
static int scan_grid(int64_t bound) {
    int64_t g = (bound + SCAN_T) / SCAN_T + 1;
    return (int)(g < 1 ? 1 : (g > 2048 ? 2048 : g));
}

static hipEvent_t ev_get() { hipEvent_t e; (void)hipEventCreate(&e); return e; }

// WK_FN_DISPATCH=0: route around the functional-predicate dense maps at
// dispatch time (diagnostic / roofline probe of the classic pipeline).
// Read per call — bench.py flips it mid-process.
static bool wk_fn_dispatch() {
    const char *v = getenv("WK_FN_DISPATCH");
    return !(v && !atoi(v));
}

// WK_CHAIN=0: run every pattern as a step of its own (no per-row op
// chain fused into an expansion).  Read per call, like
// WK_FN_DISPATCH.
static bool wk_row_chain() {  // WK_ROW_CHAIN=0: expansion tails only
    const char *v = getenv("WK_ROW_CHAIN");
    return !(v && v[0] == '0');
}
static bool wk_chain() {
    const char *v = getenv("WK_CHAIN");
    return !(v && !atoi(v));
}
// Width bucket of the batched chain kernels: candidate
// rows are carried as sid_t[ROW_NARROW] when the plan's widened row fits,
// else as sid_t[ROW_MAX].  WK_CHAIN_WIDTH=8 forces the wide instantiation
// (A/B arm and fallback).  Read per call, like WK_CHAIN.
static bool chain_narrow(int out_cols) {
    const char *v = getenv("WK_CHAIN_WIDTH");
    return out_cols <= ROW_NARROW && !(v && atoi(v) == ROW_MAX);
}
// WK_CHAIN_SCHED=0: one chain op per round in plan order and no wave
// early-out, i.e. the plain op loop through the same kernels (A/B arm of
// the round schedule).  Read per call, like WK_CHAIN.
static bool wk_chain_sched() {
    const char *v = getenv("WK_CHAIN_SCHED");
    return !(v && !atoi(v));
}
// Grid of the three batched chain kernels: grid_for's, but never more
// blocks than are resident at once at the kernel's compiled occupancy
// (queried once per instantiation), so that the grid-stride loops run as
// one batch; every instantiation at 8 waves per SIMD keeps 2048.
// WK_CHAIN_GRID=<n> caps it further, so that a test table of a few
// thousand rows makes one block walk several tiles / iterations.  Read
// per call, like WK_MIN_CAP.
template <auto Kern>
static int chain_grid(int64_t work) {
    static const int resident = [] {
        int nb = 0, dev = 0, cus = 0;
        if (hipGetDevice(&dev) != hipSuccess ||
            hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount,
                                  dev) != hipSuccess ||
            hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, Kern, BLOCK,
                                                         0) != hipSuccess ||
            nb < 1 || cus < 1)
            return 2048;
        return std::min(2048, nb * cus);
    }();
    int g = std::min(grid_for(work), resident);
    const char *v = getenv("WK_CHAIN_GRID");
    const int cap = v ? atoi(v) : 0;
    return cap > 0 && cap < g ? cap : g;
}
// WK_FILTER_BATCH=0: k_filter_tpr evaluates its rows one after another
// (filter_keep) on every path.  Read per call, like WK_CHAIN.
static bool wk_filter_batch() {
    const char *v = getenv("WK_FILTER_BATCH");
    return !(v && !atoi(v));
}
// WK_SCAN=0: the barrier-ladder k_scan_local/k_scan_mid (DESIGN.md §3
// 5g(vi)) in place of the wave-scan ones.  Read per call, like WK_CHAIN.
static bool wk_wave_scan() {
    const char *v = getenv("WK_SCAN");
    return !(v && !atoi(v));
}

// WK_FILTER_PUSHDOWN=0: run every FILTER conjunct at the reference's
// position (after the whole plan) instead of right behind the pattern
// that binds its last variable.  Read per call, like WK_CHAIN.
static bool wk_filter_pushdown() {
    const char *v = getenv("WK_FILTER_PUSHDOWN");
    return !(v && !atoi(v));
}

// WK_SPIN_SYNC=1: poll instead of blocking (diagnostic)
static bool wk_spin_sync() {
    static int v = -1;
    if (v < 0) { const char *e = getenv("WK_SPIN_SYNC"); v = e ? atoi(e) : 0; }
    return v;
}
static hipError_t stream_sync(hipStream_t s) {
    if (!wk_spin_sync()) return hipStreamSynchronize(s);
    hipError_t rc;
    while ((rc = hipStreamQuery(s)) == hipErrorNotReady) {}
    return rc;
}

#define TIME_BEGIN(eng)                                                     \
    hipEvent_t t_s_ = nullptr, t_e_ = nullptr;                              \
    if ((eng)->timing && !(eng)->capturing) {                               \
        t_s_ = ev_get(); t_e_ = ev_get();                                   \
        (void)hipEventRecord(t_s_, (eng)->stream); }

#define TIME_END(eng, category)                                             \
    if ((eng)->timing && !(eng)->capturing) {                               \
        (void)hipEventRecord(t_e_, (eng)->stream);                          \
        (eng)->pending.push_back({t_s_, t_e_, (category)}); }

static const char *CAT_NAMES[CAT_COUNT] = {"probe", "scan", "expand", "filter",
                                           "copy", "split", "other"};

static void resolve_timing(wk_engine *e) {
    for (auto &t : e->pending) {
        float ms = 0;
        (void)hipEventElapsedTime(&ms, t.start, t.stop);
        if (wk_verbose_lvl() >= 3)
            fprintf(stderr, "[launch] %s %.0fus\n", CAT_NAMES[t.cat], ms * 1e3);
        e->cat_usec[t.cat] += ms * 1000.0;
        e->cat_n[t.cat]++;
        (void)hipEventDestroy(t.start);
        (void)hipEventDestroy(t.stop);
    }
    e->pending.clear();
}

// grow scratch + rbufs to hold `rows` rows of up to `cols` columns.
// Preserves the CURRENT table's contents (e->nrows x e->ncols, valid at
// every sync point) so a mid-plan overflow re-run can resume from the
// intact input table (dual-buffer invariant).
static int64_t min_cap_rows() {
    const char *v = getenv("WK_MIN_CAP");  // tests force tiny caps to
    return v ? atoll(v) : (1 << 20);       // exercise the overflow re-run
}

static int32_t grow_caps(wk_engine *e, int64_t rows, int cols) {
    rows = std::max<int64_t>(rows, min_cap_rows());
    cols = std::max(cols, std::max(e->cap_cols, 1));
    if (rows <= e->cap_rows && cols <= e->cap_cols) return WK_OK;
    if (e->capturing) return WK_ERR_STATE;  // no alloc/sync inside capture
    rows = std::max(rows, e->cap_rows);
    // one sync before freeing buffers that in-flight kernels may use
    HIP_CHECK(stream_sync(e->stream));
    fin_invalidate(e);  // the finalized table lives in the old buffers
    size_t keep = (size_t)std::max<int64_t>(e->nrows, 0) * std::max(e->ncols, 0) * 4;
    keep = std::min(keep, e->tbl[e->cur].cap);
    void *saved = nullptr;
    if (keep) {
        if (hipMalloc(&saved, keep) != hipSuccess) return WK_ERR_HIP;
        HIP_CHECK(hipMemcpy(saved, e->tbl[e->cur].p, keep, hipMemcpyDeviceToDevice));
    }
    if (e->tbl[0].ensure((size_t)rows * cols * 4)) return WK_ERR_HIP;
    if (e->tbl[1].ensure((size_t)rows * cols * 4)) return WK_ERR_HIP;
    if (saved) {
        HIP_CHECK(hipMemcpy(e->tbl[e->cur].p, saved, keep, hipMemcpyDeviceToDevice));
        (void)hipFree(saved);
    }
    if (e->cnt.ensure((size_t)(rows + 1) * 4)) return WK_ERR_HIP;   // u32 degs
    // u32 per-row pass masks of the chain-fused expansion
    if (e->pmask.ensure((size_t)(rows + 1) * 4)) return WK_ERR_HIP;
    if (e->eoff.ensure((size_t)(rows + 1) * 8)) return WK_ERR_HIP;
    if (e->prefix.ensure((size_t)(rows + 1) * 8)) return WK_ERR_HIP;
    if (e->ovf.ensure((size_t)(rows + 1) * 4)) return WK_ERR_HIP;
    if (e->bsums.ensure(2056 * 8)) return WK_ERR_HIP;
    if (e->fhist.ensure((size_t)fin_grid(rows) * 256 * 4)) return WK_ERR_HIP;
    e->cap_rows = rows;
    e->cap_cols = cols;
    return WK_OK;
}

extern "C" void wk_gpu_store_destroy(wk_gpu_store_t *g);

extern "C" wk_gpu_store_t *wk_gpu_store_create(const wk_store_t *st, int32_t device) {
    if (!st) return nullptr;
    if (hipSetDevice(device) != hipSuccess) return nullptr;
    wk_gpu_store *g = new wk_gpu_store();
    g->st = st;
    g->device = device;
    size_t vb = st->vertices.size() * sizeof(vertex_t);
    size_t eb = st->edges.size() * sizeof(sid_t);
    if (hipMalloc(&g->d_verts, vb ? vb : 16) != hipSuccess ||
        hipMalloc(&g->d_edges, eb ? eb : 16) != hipSuccess) {
        wk_gpu_store_destroy(g);
        return nullptr;
    }
    if (hipMemcpy(g->d_verts, st->vertices.data(), vb, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(g->d_edges, st->edges.data(), eb, hipMemcpyHostToDevice) != hipSuccess) {
        wk_gpu_store_destroy(g);
        return nullptr;
    }
    if (st->type_n) {
        if (hipMalloc(&g->d_type_of, st->type_n * 2) != hipSuccess ||
            hipMemcpy(g->d_type_of, st->type_of.data(), st->type_n * 2,
                      hipMemcpyHostToDevice) != hipSuccess) {
            wk_gpu_store_destroy(g);
            return nullptr;
        }
    }
    if (st->vp_n) {
        for (int d = 0; d < 2; d++) {
            size_t ob = (st->vp_n + 1) * 4;
            size_t eb = st->vp_edges[d].size() * 4;
            if (hipMalloc(&g->d_vp_off[d], ob) != hipSuccess ||
                hipMalloc(&g->d_vp_edges[d], eb ? eb : 16) != hipSuccess ||
                hipMemcpy(g->d_vp_off[d], st->vp_off[d].data(), ob,
                          hipMemcpyHostToDevice) != hipSuccess ||
                (eb && hipMemcpy(g->d_vp_edges[d], st->vp_edges[d].data(), eb,
                                 hipMemcpyHostToDevice) != hipSuccess)) {
                wk_gpu_store_destroy(g);
                return nullptr;
            }
        }
        size_t sb = st->nseg.size() * sizeof(seg_t);
        if (hipMalloc(&g->d_segtab, sb) != hipSuccess ||
            hipMemcpy(g->d_segtab, st->nseg.data(), sb,
                      hipMemcpyHostToDevice) != hipSuccess) {
            wk_gpu_store_destroy(g);
            return nullptr;
        }
    }
    if (st->fn_n) {
        g->d_fn_pages.assign(st->fn.size(), nullptr);
        g->d_fn_vals.assign(st->fn.size(), nullptr);
        for (size_t w = 0; w < st->fn.size(); w++) {
            if (!st->fn[w].present()) continue;
            size_t pb = st->fn[w].pages.size() * sizeof(fnpage_t);
            size_t vb = std::max<size_t>(st->fn[w].vals.size() * 4, 4);
            if (hipMalloc(&g->d_fn_pages[w], pb) != hipSuccess ||
                hipMemcpy(g->d_fn_pages[w], st->fn[w].pages.data(), pb,
                          hipMemcpyHostToDevice) != hipSuccess ||
                hipMalloc(&g->d_fn_vals[w], vb) != hipSuccess ||
                hipMemcpy(g->d_fn_vals[w], st->fn[w].vals.data(),
                          st->fn[w].vals.size() * 4,
                          hipMemcpyHostToDevice) != hipSuccess) {
                wk_gpu_store_destroy(g);
                return nullptr;
            }
        }
    }
    if (!st->csr.empty()) {
        g->d_csr_pages.assign(st->csr.size(), nullptr);
        g->d_csr_entries.assign(st->csr.size(), nullptr);
        for (size_t w = 0; w < st->csr.size(); w++) {
            if (!st->csr[w].present()) continue;
            size_t pb = st->csr[w].pages.size() * sizeof(fnpage_t);
            size_t eb = std::max<size_t>(st->csr[w].entries.size() * 8, 8);
            if (hipMalloc(&g->d_csr_pages[w], pb) != hipSuccess ||
                hipMemcpy(g->d_csr_pages[w], st->csr[w].pages.data(), pb,
                          hipMemcpyHostToDevice) != hipSuccess ||
                hipMalloc(&g->d_csr_entries[w], eb) != hipSuccess ||
                hipMemcpy(g->d_csr_entries[w], st->csr[w].entries.data(),
                          st->csr[w].entries.size() * 8,
                          hipMemcpyHostToDevice) != hipSuccess) {
                wk_gpu_store_destroy(g);
                return nullptr;
            }
        }
    }
    if (!st->tbm.empty()) {
        g->d_tbm.assign(st->tbm.size(), nullptr);
        for (size_t t = 0; t < st->tbm.size(); t++) {
            if (st->tbm[t].empty()) continue;
            size_t tb = st->tbm[t].size() * 8;
            if (hipMalloc(&g->d_tbm[t], tb) != hipSuccess ||
                hipMemcpy(g->d_tbm[t], st->tbm[t].data(), tb,
                          hipMemcpyHostToDevice) != hipSuccess) {
                wk_gpu_store_destroy(g);
                return nullptr;
            }
        }
    }
    return g;
}

extern "C" void wk_gpu_store_destroy(wk_gpu_store_t *g) {
    if (!g) return;
    if (g->refs > 0) { g->owned = false; return; }  // last engine frees
    if (g->d_verts) (void)hipFree(g->d_verts);
    if (g->d_edges) (void)hipFree(g->d_edges);
    if (g->d_type_of) (void)hipFree(g->d_type_of);
    for (int d = 0; d < 2; d++) {
        if (g->d_vp_off[d]) (void)hipFree(g->d_vp_off[d]);
        if (g->d_vp_edges[d]) (void)hipFree(g->d_vp_edges[d]);
    }
    if (g->d_segtab) (void)hipFree(g->d_segtab);
    for (fnpage_t *p : g->d_fn_pages)
        if (p) (void)hipFree(p);
    for (sid_t *p : g->d_fn_vals)
        if (p) (void)hipFree(p);
    for (fnpage_t *p : g->d_csr_pages)
        if (p) (void)hipFree(p);
    for (uint64_t *p : g->d_csr_entries)
        if (p) (void)hipFree(p);
    for (uint64_t *p : g->d_tbm)
        if (p) (void)hipFree(p);
    for (void *p : g->ipc_opened)
        if (p) (void)hipIpcCloseMemHandle(p);
    if (g->d_peers) (void)hipFree(g->d_peers);
    delete g;
}

// ---- xGMI peer-mapping export/import (small-table remote reads) ------
extern "C" int32_t wk_gpu_store_export(wk_gpu_store_t *g,
                                       wk_peer_blob_t *out) {
    if (!g || !out) return WK_ERR_STATE;
    memset(out, 0, sizeof(*out));
    out->device = g->device;
    out->sid = g->st->sid;
    out->nsrv = g->st->nsrv;
    out->type_base = g->st->type_base;
    out->type_n = g->st->type_n;
    out->nseg = (int64_t)g->st->nseg.size();
    static_assert(sizeof(hipIpcMemHandle_t) <= WK_IPC_HANDLE_BYTES,
                  "ipc handle size");
    if (hipIpcGetMemHandle((hipIpcMemHandle_t *)out->verts_h, g->d_verts) !=
            hipSuccess ||
        hipIpcGetMemHandle((hipIpcMemHandle_t *)out->edges_h, g->d_edges) !=
            hipSuccess)
        return WK_ERR_HIP;
    if (g->d_type_of) {
        if (hipIpcGetMemHandle((hipIpcMemHandle_t *)out->type_of_h,
                               g->d_type_of) != hipSuccess)
            return WK_ERR_HIP;
        out->has_type_of = 1;
    }
    return WK_OK;
}

extern "C" int64_t wk_store_seg_table(const wk_store_t *st, uint64_t *out,
                                      int64_t cap_entries) {
    if (!st) return -1;
    int64_t n = (int64_t)st->nseg.size();
    if (!out) return n;
    if (cap_entries < n) return -1;
    for (int64_t w = 0; w < n; w++) {
        out[2 * w] = st->nseg[w].bucket_start;
        out[2 * w + 1] = st->nseg[w].num_buckets;
    }
    return n;
}

extern "C" int32_t wk_gpu_store_import_peers(wk_gpu_store_t *g,
                                             const wk_peer_blob_t *blobs,
                                             const uint64_t *segtabs,
                                             int64_t nseg, int32_t nsrv) {
    if (!g || !blobs || !segtabs || nsrv <= 0 || nsrv > 8) return WK_ERR_STATE;
    if (hipSetDevice(g->device) != hipSuccess) return WK_ERR_HIP;
    g->peers.assign(nsrv, wk_peer_desc{});
    g->peer_nseg.assign(nsrv, {});
    const int me = g->st->sid;
    for (int r = 0; r < nsrv; r++) {
        const wk_peer_blob_t &b = blobs[r];
        if (b.nseg != nseg) return WK_ERR_STATE;
        wk_peer_desc &P = g->peers[r];
        P.type_base = b.type_base;
        P.type_n = b.type_n;
        if (r == me) {
            P.verts = g->d_verts;
            P.edges = g->d_edges;
            P.type_of = g->d_type_of;
        } else {
            void *pv = nullptr, *pe = nullptr, *pt = nullptr;
            if (hipIpcOpenMemHandle(&pv, *(const hipIpcMemHandle_t *)b.verts_h,
                                    hipIpcMemLazyEnablePeerAccess) != hipSuccess)
                return WK_ERR_HIP;
            g->ipc_opened.push_back(pv);
            if (hipIpcOpenMemHandle(&pe, *(const hipIpcMemHandle_t *)b.edges_h,
                                    hipIpcMemLazyEnablePeerAccess) != hipSuccess)
                return WK_ERR_HIP;
            g->ipc_opened.push_back(pe);
            if (b.has_type_of) {
                if (hipIpcOpenMemHandle(&pt,
                                        *(const hipIpcMemHandle_t *)b.type_of_h,
                                        hipIpcMemLazyEnablePeerAccess) !=
                    hipSuccess)
                    return WK_ERR_HIP;
                g->ipc_opened.push_back(pt);
            }
            P.verts = (const vertex_t *)pv;
            P.edges = (const sid_t *)pe;
            P.type_of = (const uint16_t *)pt;
        }
        g->peer_nseg[r].resize((size_t)nseg);
        const uint64_t *tab = segtabs + (size_t)r * nseg * 2;
        for (int64_t w = 0; w < nseg; w++) {
            g->peer_nseg[r][w].bucket_start = tab[2 * w];
            g->peer_nseg[r][w].num_buckets = tab[2 * w + 1];
        }
    }
    if (hipMalloc(&g->d_peers, nsrv * sizeof(wk_peer_desc)) != hipSuccess ||
        hipMemcpy(g->d_peers, g->peers.data(), nsrv * sizeof(wk_peer_desc),
                  hipMemcpyHostToDevice) != hipSuccess)
        return WK_ERR_HIP;
    return WK_OK;
}

extern "C" wk_engine_t *wk_engine_create_on(wk_gpu_store_t *g) {
    if (!g) return nullptr;
    if (hipSetDevice(g->device) != hipSuccess) return nullptr;
    wk_engine *e = new wk_engine();
    e->st = g->st;
    e->gs = g;
    g->refs++;
    e->device = g->device;
    e->d_verts = g->d_verts;
    e->d_edges = g->d_edges;
    e->d_type_of = g->d_type_of;
    if (hipStreamCreate(&e->stream) != hipSuccess) { delete e; return nullptr; }
    if (hipMalloc(&e->d_state, (S_WORDS + CAT_COUNT + 2) * 8) != hipSuccess ||
        hipHostMalloc(&e->h_pin, 64 * sizeof(uint64_t)) != hipSuccess) {
        wk_engine_destroy(e);
        return nullptr;
    }
    e->d_stats = e->d_state + S_WORDS;
    if (hipMalloc(&e->d_fin, F_WORDS * 8) != hipSuccess ||
        hipMemset(e->d_fin, 0, F_WORDS * 8) != hipSuccess ||
        hipMemset(e->d_state, 0, (S_WORDS + CAT_COUNT + 2) * 8) != hipSuccess) {
        wk_engine_destroy(e);
        return nullptr;
    }
    if (const char *t = getenv("WK_KERNEL_TIMING")) e->timing = atoi(t) != 0;
    if (grow_caps(e, min_cap_rows(), 4) != WK_OK) { wk_engine_destroy(e); return nullptr; }
    return e;
}

extern "C" wk_engine_t *wk_engine_create(const wk_store_t *st, int32_t device) {
    wk_gpu_store *g = wk_gpu_store_create(st, device);
    if (!g) return nullptr;
    g->owned = true;
    wk_engine *e = wk_engine_create_on(g);
    if (!e) { g->owned = false; wk_gpu_store_destroy(g); return nullptr; }
    return e;
}

extern "C" void wk_engine_destroy(wk_engine_t *e) {
    if (!e) return;
    resolve_timing(e);
    for (int i = 0; i < 2; i++) e->tbl[i].release();
    e->eoff.release(); e->cnt.release(); e->pmask.release();
    e->prefix.release();
    e->bsums.release(); e->misc.release(); e->ovf.release();
    e->fhist.release();
    e->oflag[0].release(); e->oflag[1].release();
    for (auto &g : e->graphs)
        if (g.exec) (void)hipGraphExecDestroy(g.exec);
    e->lbd.release(); e->lbcnt.release();
    if (e->h_lb) (void)hipHostFree(e->h_lb);
    if (e->d_state) (void)hipFree(e->d_state);
    if (e->d_fin) (void)hipFree(e->d_fin);
    if (e->h_pin) (void)hipHostFree(e->h_pin);
    if (e->h_stage) (void)hipHostFree(e->h_stage);
    if (e->stream) (void)hipStreamDestroy(e->stream);
    if (e->gs) {
        e->gs->refs--;
        if (e->gs->refs == 0 && e->gs->owned) {
            e->gs->owned = false;
            wk_gpu_store_destroy(e->gs);
        }
    }
    delete e;
}

// Validate the plan's FILTER program and split it into top-level
// conjuncts (across clauses and through top-level AND nodes — the clauses
// are ANDed into the one program), each with its placement.  A conjunct
// whose variables are all bound by main-BGP patterns runs right behind
// the earliest pattern that binds the last of them: exact, because main-
// BGP columns are never rewritten later and every later operator acts
// row by row.  The others wait for the reference position.
static int32_t plan_filter(wk_engine *e, const wk_plan_t *plan) {
    e->filt.clear();
    e->conj.clear();
    const int n = plan->nfilter;
    if (n <= 0 || !plan->filter) return n > 0 ? WK_ERR_PLAN : WK_OK;
    if (n > WK_FILTER_MAX) return WK_ERR_PLAN;
    const int nv = plan->nvars, np = std::max(plan->npatterns, 0);
    // first main pattern a variable appears in (every variable of a
    // pattern has a column once the pattern ran); elsewhere = union/opt
    std::vector<int> first_main((size_t)nv, -1);
    std::vector<uint8_t> elsewhere((size_t)nv, 0);
    auto note = [&](ssid_t v, int k) {
        if (v >= 0 || -(v + 1) >= nv) return;
        if (k < 0) elsewhere[-(v + 1)] = 1;
        else if (first_main[-(v + 1)] < 0) first_main[-(v + 1)] = k;
    };
    auto note_pat = [&](const wk_pattern_t &pt, int k) {
        note(pt.subject, k); note(pt.predicate, k); note(pt.object, k);
    };
    for (int k = 0; k < np; k++) note_pat(plan->patterns[k], k);
    for (int k = 0; k < plan->nopt && plan->opt_patterns; k++)
        note_pat(plan->opt_patterns[k], -1);
    int nu = 0;
    for (int b = 0; b < plan->nunion && plan->union_sizes; b++)
        nu += plan->union_sizes[b];
    for (int k = 0; k < nu && plan->union_pats; k++)
        note_pat(plan->union_pats[k], -1);
    // start[i]: first node of the subtree that ends at node i
    int start[WK_FILTER_MAX];
    auto operand_ok = [&](int32_t x) {
        if (x == 0 || x < -nv) return false;
        return x > 0 || first_main[-(x + 1)] >= 0 || elsewhere[-(x + 1)];
    };
    for (int i = 0; i < n; i++) {
        const wk_fnode_t &f = plan->filter[i];
        switch (f.op) {
        case WK_F_EQ: case WK_F_NE:
            if (!operand_ok(f.a) || !operand_ok(f.b)) return WK_ERR_PLAN;
            start[i] = i;
            break;
        case WK_F_BOUND:
            if (f.a >= 0 || !operand_ok(f.a)) return WK_ERR_PLAN;
            start[i] = i;
            break;
        case WK_F_NOT:
            if (i < 1) return WK_ERR_PLAN;  // stack underflow
            start[i] = start[i - 1];
            break;
        case WK_F_AND: case WK_F_OR:
            if (i < 1 || start[i - 1] < 1) return WK_ERR_PLAN;  // underflow
            start[i] = start[start[i - 1] - 1];
            break;
        default:
            return WK_ERR_PLAN;
        }
    }
    if (start[n - 1] != 0) return WK_ERR_PLAN;  // final stack depth != 1
    e->filt.assign(plan->filter, plan->filter + n);
    const bool groups = plan->nunion > 0 || plan->nopt > 0;
    const bool push = wk_filter_pushdown();
    // explicit stack instead of recursion: subtree end indexes
    std::vector<int> todo{n - 1};
    while (!todo.empty()) {
        const int hi = todo.back();
        todo.pop_back();
        if (e->filt[hi].op == WK_F_AND) {
            todo.push_back(hi - 1);
            todo.push_back(start[hi - 1] - 1);
            continue;
        }
        wk_engine::fconj cj;
        cj.prog.assign(e->filt.begin() + start[hi], e->filt.begin() + hi + 1);
        int after = 0;
        bool main_only = true;
        for (const wk_fnode_t &f : cj.prog) {
            if (f.op > WK_F_BOUND) continue;
            for (int32_t x : {f.a, f.op == WK_F_BOUND ? f.a : f.b}) {
                if (x >= 0) continue;
                if (first_main[-(x + 1)] < 0) main_only = false;
                after = std::max(after, first_main[-(x + 1)]);
            }
        }
        if (!main_only || np == 0) cj.after = -1;
        else if (push) cj.after = after;
        else cj.after = groups ? -1 : np - 1;
        e->conj.push_back(std::move(cj));
    }
    return WK_OK;
}

extern "C" int32_t wk_engine_begin_query(wk_engine_t *e, const wk_plan_t *plan) {
    if (!e || !plan || plan->nvars <= 0) return WK_ERR_PLAN;
    if (plan->npatterns <= 0 && plan->nunion <= 0) return WK_ERR_PLAN;
    if (plan->nvars > 8) return WK_ERR_PLAN;  // col count cap (templated kernels)
    {
        int32_t rcf = plan_filter(e, plan);
        if (rcf) return rcf;
    }
    if (plan->npatterns > 0)
        e->pats.assign(plan->patterns, plan->patterns + plan->npatterns);
    else
        e->pats.clear();
    e->v2c.assign(plan->nvars, -1);
    e->nvars = plan->nvars;
    e->step = 0;
    e->nrows = 0;
    e->ncols = 0;
    e->cur = 0;
    e->tbl_view = nullptr;
    e->bound = 0;
    e->light = false;
    fin_invalidate(e);
    int32_t rc = grow_caps(e, e->cap_rows, plan->nvars);
    if (rc) return rc;
    // reset nrows + overflow flags on device: deferred to the query's
    // first launch (k_begin_state in step_start / load_common, else
    // flush_begin)
    e->zero_pending = true;
    return WK_OK;
}

// Perform a still-pending begin_query zeroing on its own: called ahead
// of every launch that reads or publishes d_state and is not itself a
// begin-aware state write (launch_set_rows).
// A publish held back by the suite capture goes out on its own when the
// next query does not open with k_begin_state.
static void flush_publish(wk_engine *e) {
    if (e->publish_pending < 0) return;
    hipLaunchKernelGGL(k_publish_state, dim3(1), dim3(1), 0, e->stream,
                       e->d_state, e->d_stats, e->h_pin, e->publish_pending);
    e->publish_pending = -1;
}
static void flush_begin(wk_engine *e) {
    flush_publish(e);
    if (!e->zero_pending) return;
    e->zero_pending = false;
    hipLaunchKernelGGL(k_zero_words, dim3(1), dim3(64), 0, e->stream, e->d_state,
                       S_WORDS);
}

// Set the row count of a fresh table.  As the first launch of a query it
// also does begin_query's zeroing (one kernel); later it keeps
// k_set_state's meaning and leaves S_ERR/S_REQ/S_DONE alone.
static void launch_set_rows(wk_engine *e, uint64_t nrows) {
    if (e->zero_pending && e->publish_pending >= 0) {
        e->zero_pending = false;
        hipLaunchKernelGGL(k_publish_begin, dim3(1), dim3(1), 0, e->stream,
                           e->d_state, e->d_stats, e->h_pin,
                           e->publish_pending, nrows);
        e->publish_pending = -1;
    } else if (e->zero_pending) {
        e->zero_pending = false;
        hipLaunchKernelGGL(k_begin_state, dim3(1), dim3(1), 0, e->stream,
                           e->d_state, nrows);
    } else {
        flush_publish(e);
        hipLaunchKernelGGL(k_set_state, dim3(1), dim3(1), 0, e->stream,
                           e->d_state, nrows);
    }
}

// begin without the device-state zeroing kernel (the light fast path's
// kernel writes NROWS/ERR itself and publishes to pinned memory)
static int32_t begin_light(wk_engine *e, const wk_plan_t *plan) {
    if (!e || !plan || plan->npatterns <= 0 || plan->nvars <= 0) return WK_ERR_PLAN;
    e->pats.assign(plan->patterns, plan->patterns + plan->npatterns);
    e->filt.clear();  // light2_eligible: no filter on this path
    e->conj.clear();
    e->v2c.assign(plan->nvars, -1);
    e->nvars = plan->nvars;
    e->step = 0;
    e->nrows = 0;
    e->ncols = 0;
    e->cur = 0;
    e->tbl_view = nullptr;
    e->bound = 0;
    e->light = true;
    fin_invalidate(e);
    e->zero_pending = false;  // k_light2 writes S_NROWS/S_ERR itself
    return grow_caps(e, e->cap_rows, plan->nvars);
}

static int32_t load_common(wk_engine *e, int64_t nrows, int32_t ncols,
                           const int32_t *v2c_map, int32_t pattern_step) {
    e->cur = 0;
    e->tbl_view = nullptr;
    fin_invalidate(e);
    e->nrows = nrows;
    e->bound = nrows;
    e->ncols = ncols;
    if (v2c_map) e->v2c.assign(v2c_map, v2c_map + e->nvars);
    e->step = pattern_step;
    launch_set_rows(e, (uint64_t)nrows);
    return WK_OK;
}

extern "C" int32_t wk_engine_load_rbuf(wk_engine_t *e, const sid_t *table,
                                       int64_t nrows, int32_t ncols,
                                       const int32_t *v2c_map, int32_t pattern_step) {
    if (!e) return WK_ERR_STATE;
    int32_t rc = grow_caps(e, nrows, std::max(ncols, 1));
    if (rc) return rc;
    size_t bytes = (size_t)nrows * ncols * sizeof(sid_t);
    if (bytes)
        HIP_CHECK(hipMemcpyAsync(e->tbl[0].p, table, bytes, hipMemcpyHostToDevice,
                                 e->stream));
    return load_common(e, nrows, ncols, v2c_map, pattern_step);
}

extern "C" int32_t wk_engine_load_rbuf_device(wk_engine_t *e, const sid_t *dev_table,
                                              int64_t nrows, int32_t ncols,
                                              const int32_t *v2c_map, int32_t pattern_step) {
    if (!e) return WK_ERR_STATE;
    int32_t rc = grow_caps(e, nrows, std::max(ncols, 1));
    if (rc) return rc;
    size_t bytes = (size_t)nrows * ncols * sizeof(sid_t);
    if (bytes)
        HIP_CHECK(hipMemcpyAsync(e->tbl[0].p, dev_table, bytes,
                                 hipMemcpyDeviceToDevice, e->stream));
    return load_common(e, nrows, ncols, v2c_map, pattern_step);
}

// publish device state to pinned memory + sync; refresh host nrows/stats
static void launch_publish(wk_engine *e, int expect_empty) {
    flush_begin(e);
    hipLaunchKernelGGL(k_publish_state, dim3(1), dim3(1), 0, e->stream,
                       e->d_state, e->d_stats, e->h_pin, expect_empty);
}

static int32_t sync_state(wk_engine *e) {
    if (!e->light) launch_publish(e, 0);
    HIP_CHECK(stream_sync(e->stream));
    resolve_timing(e);
    e->nrows = (int64_t)e->h_pin[S_NROWS];
    e->bound = e->nrows;
    for (int i = 0; i < CAT_COUNT; i++) e->cat_bytes[i] = (double)e->h_pin[8 + i];
    if (e->h_pin[S_ERR]) {
        // reported here: the sticky slot belongs to the pipelined
        // graph_launch window and must not fail a later wk_engine_sync
        e->h_pin[7] = 0;
        return WK_ERR_CAP;
    }
    return WK_OK;
}

// fetch-path variant: on overflow, grow and reset flags so the caller can
// simply resubmit the whole plan (table contents are irrelevant then)
static int32_t sync_state_grow(wk_engine *e) {
    int32_t rc = sync_state(e);
    if (rc != WK_ERR_CAP) return rc;
    int64_t need = (int64_t)e->h_pin[S_REQ];
    e->nrows = 0;  // nothing worth preserving across the re-run
    int32_t rc2 = grow_caps(e, need + need / 4, e->cap_cols);
    if (rc2) return rc2;
    e->zero_pending = true;  // the next launch clears the flags
    return WK_ERR_CAP;
}

// expansion dispatch, specialised on the input column count so the row
// copy unrolls/vectorises (runtime-indexed local arrays spill to scratch
// — cdna_hip_programming.md §5.4 rule 20)
//
// with_ncols is the ONE place a runtime column count (1..8) picks a
// compile-time NC: it calls f(std::integral_constant<int, NC>{}).  The
// `default -> 8` arm is safe because wk_engine_begin_query rejects
// nvars > 8, so no binding table is ever wider than 8 columns.
template <class F>
static void with_ncols(int ncols, F &&f) {
    switch (ncols) {
    case 1: f(std::integral_constant<int, 1>{}); break;
    case 2: f(std::integral_constant<int, 2>{}); break;
    case 3: f(std::integral_constant<int, 3>{}); break;
    case 4: f(std::integral_constant<int, 4>{}); break;
    case 5: f(std::integral_constant<int, 5>{}); break;
    case 6: f(std::integral_constant<int, 6>{}); break;
    case 7: f(std::integral_constant<int, 7>{}); break;
    default: f(std::integral_constant<int, 8>{}); break;
    }
}

// ---- pieces shared by the step_* operators ---------------------------

// warm-pass hint: pattern `step` dropped no rows (consulted ONLY while
// capturing a graph)
static bool hint_nodrop(const wk_engine *e, int step) {
    return e->capturing && step < (int)e->capture_hint.size() &&
           e->capture_hint[step];
}

// Const type id of a following `?o rdf:type CONST` pattern on this
// step's output variable o, or 0.  Pattern shape only: every caller adds
// its own guards (nsrv == 1, hints, !hinting, bitmap present, ...).
static sid_t typeof_lookahead(const wk_engine *e, ssid_t o) {
    if (e->step + 1 >= (int)e->pats.size()) return 0;
    const wk_pattern_t &nx = e->pats[e->step + 1];
    if (nx.subject == o && nx.predicate == (ssid_t)TYPE_ID &&
        nx.direction == DIR_OUT && nx.object > 0)
        return (sid_t)nx.object;
    return 0;
}

// per-type membership bitmap of a type id (null = not built)
static const uint64_t *type_bitmap(const wk_engine *e, sid_t type_id) {
    return (e->gs && (size_t)type_id < e->gs->d_tbm.size())
               ? e->gs->d_tbm[type_id]
               : nullptr;
}

// functional map of (p, dir): pages (null = absent) and packed values
static const fnpage_t *fn_map(const wk_engine *e, ssid_t p, int dir,
                              const sid_t **vals) {
    const size_t w = (size_t)p * 2 + dir;
    if (!e->gs || w >= e->gs->d_fn_pages.size() || !e->gs->d_fn_pages[w])
        return nullptr;
    *vals = e->gs->d_fn_vals[w];
    return e->gs->d_fn_pages[w];
}

// ---- per-row op chains -----------------------------
struct chain_plan {
    chain_t C{};
    int npat = 0;             // patterns consumed (one op each)
    int nfilter = 0;          // ops other than FN_APPEND
    int out_cols = 0;         // column count after the chain
    int nnew = 0;             // appended variables, in column order
    ssid_t new_vars[CHAIN_MAX];
    bool lone_typeof(int col) const {
        return npat == 1 && C.op[0].kind == CH_TYPE && C.op[0].a == col;
    }
};

// chains apply to whole-plan runs on the local, single-step-at-a-time
// path only; off while the hint pass needs per-pattern row counts
static bool chain_enabled(const wk_engine *e) {
    return e->whole_plan && !e->hinting && !e->opt_mode &&
           e->remote_step_idx < 0 && e->gs && wk_fn_dispatch() && wk_chain();
}

// Greedily collect the patterns from index `from` on that are per-row
// ops over the layout (v2c, ncols): known subject, fixed predicate,
// PK_NORMAL key, and the functional map / type bitmap the op reads is
// built — the eligibility rules of step_filter / step_k2u_fn, one op per
// pattern.  Stops at the first pattern that does not fit.  In a capture
// with a truncated empty tail the chain never reaches into the tail.
static void collect_chain(const wk_engine *e, int from,
                          std::vector<int32_t> v2c, int ncols,
                          chain_plan &cp) {
    const wk_store *st = e->st;
    const int nc_in = ncols;
    cp.C.fn_base = st->fn_base;
    cp.C.fn_n = st->fn_n;
    cp.C.t_base = st->type_base;
    cp.C.t_n = st->type_n;
    int end = (int)e->pats.size();
    if (e->capturing && e->capture_empty_after >= 0)
        end = std::min(end, e->capture_empty_after + 1);
    auto col_of = [&](ssid_t v) {
        const int i = -(v + 1);
        return (v < 0 && i < (int)v2c.size()) ? v2c[i] : -1;
    };
    for (int i = from; i < end && cp.npat < CHAIN_MAX; i++) {
        const wk_pattern_t &pt = e->pats[i];
        const ssid_t p = pt.predicate;
        const int dir = pt.direction;
        const int a = col_of(pt.subject);
        if (a < 0 || p < 1) break;
        if ((sid_t)p == TYPE_ID && dir == DIR_IN) break;  // PK_INDEX
        chain_op op{nullptr, nullptr, 0, a, 0, 0, -1};
        const sid_t *vals = nullptr;
        if (pt.object >= 0) {
            if ((sid_t)p == TYPE_ID && dir == DIR_OUT) {
                const uint64_t *tbm = type_bitmap(e, (sid_t)pt.object);
                if (!tbm) break;
                op.kind = CH_TYPE;
                op.data = tbm;
            } else {
                // k2c: only the reversed-map form (host-resolved PM_EQ)
                if (fn_map(e, p, dir, &vals) || st->nsrv != 1 ||
                    !fn_map(e, p, dir ^ 1, &vals))
                    break;
                op.kind = CH_EQ;
                op.cval = st->fn_get((size_t)p * 2 + (dir ^ 1),
                                     (sid_t)pt.object);
            }
            cp.nfilter++;
        } else if (col_of(pt.object) >= 0) {  // k2k
            op.kind = CH_FN_EQ;
            op.b = col_of(pt.object);
            op.pg = fn_map(e, p, dir, &vals);
            if (!op.pg && st->nsrv == 1) {  // reversed map: swap the roles
                op.pg = fn_map(e, p, dir ^ 1, &vals);
                std::swap(op.a, op.b);
            }
            if (!op.pg) break;
            op.data = vals;
            cp.nfilter++;
        } else {  // functional k2u
            const int oi = -(pt.object + 1);
            if (oi >= (int)v2c.size() || ncols + 1 > e->cap_cols ||
                ncols + 1 > ROW_MAX)
                break;
            op.pg = fn_map(e, p, dir, &vals);
            if (!op.pg) break;
            op.kind = CH_FN_APPEND;
            op.data = vals;
            v2c[oi] = ncols++;
            cp.new_vars[cp.nnew++] = pt.object;
        }
        cp.C.op[cp.npat++] = op;
    }
    cp.C.nops = cp.npat;
    cp.out_cols = ncols;
    // dependency rounds and the appends' destination columns
    chain_sched_op sop[CHAIN_MAX];
    for (int i = 0; i < cp.npat; i++)
        sop[i] = {cp.C.op[i].kind, cp.C.op[i].a, cp.C.op[i].b};
    chain_sched S;
    chain_schedule(sop, cp.npat, nc_in, wk_chain_sched(), S);
    cp.C.nrounds = S.nrounds;
    cp.C.early_out = S.early_out;
    for (int i = 0; i < CHAIN_MAX; i++) {
        cp.C.op[i].dst = S.dst[i];
        for (int s2 = 0; s2 < CHAIN_SLOTS; s2++)
            cp.C.slot[i][s2] = S.slot[i][s2];
    }
}

// bind a chain's appended variables to the columns from `first_col` on
static void bind_chain_vars(wk_engine *e, const chain_plan &cp, int first_col) {
    for (int j = 0; j < cp.nnew; j++)
        e->v2c[-(cp.new_vars[j] + 1)] = first_col + j;
}

// End-of-step bookkeeping: bind new_var (a variable, < 0; 0 = none) to
// the appended column, set the column count and the host row bound, and
// consume `consumed` patterns.  finish_step is for steps that wrote the
// OTHER table buffer (flip, drop any zero-copy view);
// finish_step_in_place is for the steps that leave the current table
// where it is (OPTIONAL filter, verify-only filter, absent segment).
static void finish_step_in_place(wk_engine *e, ssid_t new_var, int out_cols,
                                 int64_t bound, int consumed) {
    if (new_var < 0) e->v2c[-(new_var + 1)] = e->ncols;
    fin_invalidate(e);
    e->ncols = out_cols;
    e->bound = bound;
    e->step += consumed;
}
static void finish_step(wk_engine *e, ssid_t new_var, int out_cols,
                        int64_t bound, int consumed) {
    finish_step_in_place(e, new_var, out_cols, bound, consumed);
    e->cur ^= 1;
    e->tbl_view = nullptr;
}

static void launch_commit(wk_engine *e) {
    hipLaunchKernelGGL(k_commit, dim3(1), dim3(1), 0, e->stream, e->d_state,
                       (uint64_t)e->cap_rows);
}

// fparams of a fixed-list membership filter (c2k/i2k): keep the rows
// whose `col` value is in the sorted list edges[off, off+sz)
static fparams fparams_list(const wk_engine *e, const sid_t *edges,
                            const sid_t *cur_tbl, int col, int dir,
                            uint64_t off, uint64_t sz) {
    return fparams{e->d_verts, edges, 0, 1, cur_tbl, e->ncols, col, 0u,
                   dir, PK_NORMAL, PM_LIST, 0, 0u, off, sz, e->d_type_of,
                   0, 0, 0, nullptr, nullptr, nullptr, 0, 0, 0};
}
static void launch_filter_tpr(wk_engine *e, const fparams &P, int verify_only,
                              sid_t *out_tbl) {
    hipLaunchKernelGGL(k_filter_tpr, dim3(grid_for(e->bound)), dim3(BLOCK), 0,
                       e->stream, P, verify_only, (int)wk_filter_batch(),
                       e->d_state, e->d_stats, out_tbl);
}

static void launch_scan_mid(wk_engine *e, int G) {
    hipLaunchKernelGGL(wk_wave_scan() ? k_scan_mid : k_scan_mid_ladder,
                       dim3(1), dim3(SCAN_T), 0, e->stream,
                       (uint64_t *)e->bsums.p, G, (uint64_t)e->cap_rows,
                       e->d_state);
}
// Front half of a scan-pipeline step: gather() launches the 1:1 kernel
// that fills cnt, then k_scan_local + k_scan_mid turn the counts into
// output positions (k_scan_mid also commits the step).  `timed`
// attributes gather + scan_local to CAT_PROBE and scan_mid to CAT_SCAN
// (the CSR paths); the fn pipeline passes false because its caller
// times the whole chain as CAT_EXPAND.
template <class Gather>
static void launch_gather_scan(wk_engine *e, int G, bool timed,
                               Gather &&gather) {
    auto front = [&] {
        gather();
        hipLaunchKernelGGL(wk_wave_scan() ? k_scan_local : k_scan_local_ladder,
                           dim3(G), dim3(SCAN_T), 0, e->stream,
                           (const uint32_t *)e->cnt.p, e->d_state,
                           (uint64_t *)e->prefix.p, (uint64_t *)e->bsums.p);
    };
    if (!timed) {
        front();
        launch_scan_mid(e, G);
        return;
    }
    {
        TIME_BEGIN(e);
        front();
        TIME_END(e, CAT_PROBE);
    }
    {
        TIME_BEGIN(e);
        launch_scan_mid(e, G);
        TIME_END(e, CAT_SCAN);
    }
}

struct expand_verify {  // fused no-drop typeof check (captured graphs)
    const uint64_t *tbm = nullptr;
    const uint16_t *type_of = nullptr;
    uint64_t base = 0, n = 0;
    sid_t cval = 0;
    int on = 0;
};

template <int NC>
static void launch_expand_t(wk_engine *e, const sid_t *cur_tbl, sid_t *out_tbl,
                            int G, const expand_verify &vf) {
    hipLaunchKernelGGL(k_expand_in<NC>, dim3(grid_for(e->bound)), dim3(BLOCK), 0,
                       e->stream, cur_tbl, e->ncols, e->d_edges,
                       (uint64_t *)e->eoff.p, (uint32_t *)e->cnt.p,
                       (uint64_t *)e->prefix.p, (uint64_t *)e->bsums.p, G,
                       e->d_state, (uint64_t)e->cap_rows, e->d_stats,
                       (uint32_t *)e->ovf.p, vf.tbm, vf.type_of, vf.base,
                       vf.n, vf.cval, vf.on, out_tbl);
    hipLaunchKernelGGL(k_expand_big<NC>, dim3(512), dim3(BLOCK), 0, e->stream,
                       cur_tbl, e->ncols, e->d_edges, (uint64_t *)e->eoff.p,
                       (uint32_t *)e->cnt.p, (uint64_t *)e->prefix.p,
                       (uint64_t *)e->bsums.p, G, e->d_state,
                       (uint64_t)e->cap_rows,
                       (uint32_t *)e->ovf.p, vf.tbm, vf.type_of, vf.base,
                       vf.n, vf.cval, vf.on, out_tbl);
    // a fused verify's misses sit in the sticky S_DONE word until the
    // publish: no epilogue launch
}

template <int NC>
static void launch_expand_fn_t(wk_engine *e, const sid_t *cur_tbl,
                               sid_t *out_tbl, const fnpage_t *d_pg,
                               const sid_t *d_vals, int col,
                               bool fuse, sid_t fcval, const seg_t *fseg) {
    const uint64_t *tbm = fuse ? type_bitmap(e, fcval) : nullptr;
    // atomic-free pipeline: 1:1 gather of resolved objects (+0/1
    // counts), deterministic positions via the chunked scan, then a
    // barrier-free scatter.  A per-tile cursor atomic costs ~23 us per
    // 2048-block round (single-word ~88 atomics/us) and held every
    // in-kernel-aggregation variant of this step at a flat ~107 us.
    const int G = scan_grid(e->bound);
    launch_gather_scan(e, G, /*timed*/ false, [&] {
        hipLaunchKernelGGL(k_fn_gather, dim3(grid_for(e->bound)), dim3(BLOCK),
                           0, e->stream, cur_tbl, e->ncols, d_pg, d_vals,
                           e->st->fn_base, e->st->fn_n, col, fuse ? 1 : 0,
                           fcval, e->d_type_of, tbm, e->st->type_base,
                           e->st->type_n, e->d_verts, e->d_edges,
                           fseg ? fseg->bucket_start : 0,
                           fseg ? fseg->num_buckets : 0, e->d_state,
                           e->d_stats, (sid_t *)e->ovf.p,
                           (uint32_t *)e->cnt.p);
    });
    hipLaunchKernelGGL(k_fn_scatter<NC>, dim3(grid_for(e->bound)), dim3(BLOCK),
                       0, e->stream, cur_tbl, (const sid_t *)e->ovf.p,
                       (const uint32_t *)e->cnt.p, (const uint64_t *)e->prefix.p,
                       (const uint64_t *)e->bsums.p, G, e->d_state, e->d_stats,
                       out_tbl);
}

template <int NC>
static void launch_expand_fn_map_t(wk_engine *e, const sid_t *cur_tbl,
                                   sid_t *out_tbl, const fnpage_t *d_pg,
                                   const sid_t *d_vals,
                                   int col, bool fuse, sid_t fcval) {
    const uint64_t *tbm = fuse ? type_bitmap(e, fcval) : nullptr;
    hipLaunchKernelGGL(k_expand_fn_map<NC>, dim3(grid_for(e->bound)),
                       dim3(BLOCK), 0, e->stream, cur_tbl, d_pg, d_vals,
                       e->st->fn_base, e->st->fn_n, col, fuse ? 1 : 0, tbm,
                       e->d_type_of, e->st->type_base, e->st->type_n, fcval,
                       e->d_state, e->d_stats, out_tbl);
}

static void launch_expand_fn_map(wk_engine *e, const sid_t *cur_tbl,
                                 sid_t *out_tbl, const fnpage_t *d_pg,
                                 const sid_t *d_vals, int col,
                                 bool fuse, sid_t fcval) {
    with_ncols(e->ncols, [&](auto nc) {
        launch_expand_fn_map_t<decltype(nc)::value>(e, cur_tbl, out_tbl, d_pg, d_vals, col, fuse, fcval);
    });
}

static void launch_expand_fn(wk_engine *e, const sid_t *cur_tbl,
                             sid_t *out_tbl, const fnpage_t *d_pg,
                             const sid_t *d_vals, int col,
                             bool fuse, sid_t fcval, const seg_t *fseg) {
    with_ncols(e->ncols, [&](auto nc) {
        launch_expand_fn_t<decltype(nc)::value>(e, cur_tbl, out_tbl, d_pg, d_vals, col, fuse, fcval, fseg);
    });
}

template <int NC>
static void launch_expand_tf_t(wk_engine *e, const sid_t *cur_tbl,
                               sid_t *out_tbl, int G, const uint64_t *tbm) {
    hipLaunchKernelGGL(k_expand_tf<NC>, dim3(grid_for(e->bound)), dim3(BLOCK),
                       0, e->stream, cur_tbl, e->ncols, e->d_edges,
                       (uint64_t *)e->eoff.p, (uint32_t *)e->cnt.p,
                       (uint64_t *)e->prefix.p, (uint64_t *)e->bsums.p, G,
                       tbm, e->st->type_base, e->st->type_n, e->d_state,
                       (uint64_t)e->cap_rows, e->d_stats,
                       (uint32_t *)e->ovf.p, out_tbl);
    hipLaunchKernelGGL(k_expand_tf_big<NC>, dim3(512), dim3(BLOCK), 0,
                       e->stream, cur_tbl, e->ncols, e->d_edges,
                       (uint64_t *)e->eoff.p, (uint32_t *)e->cnt.p,
                       (uint64_t *)e->prefix.p, (uint64_t *)e->bsums.p, G,
                       tbm, e->st->type_base, e->st->type_n, e->d_state,
                       (uint64_t)e->cap_rows, (uint32_t *)e->ovf.p, out_tbl);
}

static void launch_expand_tf(wk_engine *e, const sid_t *cur_tbl,
                             sid_t *out_tbl, int G, const uint64_t *tbm) {
    with_ncols(e->ncols, [&](auto nc) {
        launch_expand_tf_t<decltype(nc)::value>(e, cur_tbl, out_tbl, G, tbm);
    });
}

static void launch_expand(wk_engine *e, const sid_t *cur_tbl, sid_t *out_tbl,
                          int G, const expand_verify &vf) {
    with_ncols(e->ncols, [&](auto nc) {
        launch_expand_t<decltype(nc)::value>(e, cur_tbl, out_tbl, G, vf);
    });
}

// Remote (xGMI peer-probe) variant of one pattern: small tables probe
// the owner rank's store in place instead of exchanging rows (the
// reference's sub-threshold one-sided read, sparql.hpp:802-814 +
// gstore.hpp:260-338).  Routed via e->remote_step_idx so the overflow
// re-run stays on the remote path.
static int32_t exec_pattern_remote(wk_engine *e) {
    wk_gpu_store *g = e->gs;
    if (!g || !g->d_peers || g->peer_nseg.empty()) return WK_ERR_STATE;
    const wk_pattern_t pat = e->pats[e->step];
    const ssid_t s = pat.subject, p = pat.predicate, o = pat.object;
    const int dir = pat.direction;
    if (s >= 0) return WK_ERR_PLAN;  // const/index starts stay local
    // [0|tid|IN] per-row index expansion fans out over ALL partitions —
    // not a per-owner read; callers must exchange for this shape
    if ((sid_t)p == TYPE_ID && dir == DIR_IN) return WK_ERR_PLAN;
    // predicate variables / VERSATILE [v|PREDICATE_ID|dir] lists live in
    // the dense vp CSR, not the peer-mapped cluster hash
    if (p < 1) return WK_ERR_PLAN;
    int col = e->var2col(s);
    if (col < 0) return WK_ERR_PLAN;
    const int nsrv = (int)g->peers.size();
    if (nsrv < 1 || nsrv > 8) return WK_ERR_STATE;
    segtab8 seg{};
    const size_t w = (size_t)p * 2 + dir;
    for (int r = 0; r < nsrv; r++) {
        if (w < g->peer_nseg[r].size()) {
            seg.bs[r] = g->peer_nseg[r][w].bucket_start;
            seg.nb[r] = g->peer_nseg[r][w].num_buckets;
        }
    }
    const int ostat = (o >= 0) ? 2 : (e->var2col(o) >= 0 ? 1 : 0);
    const int pmode = ostat == 0 ? PM_SIZE : (ostat == 2 ? PM_CONST : PM_COL);
    if (pmode == PM_SIZE && e->ncols + 1 > e->cap_cols) return WK_ERR_STATE;
    const sid_t *cur_tbl = cur_table(e);
    sid_t *out_tbl = (sid_t *)e->tbl[e->cur ^ 1].p;
    TIME_BEGIN(e);
    hipLaunchKernelGGL(k_peer_step, dim3(1), dim3(SCAN_T), 0, e->stream,
                       g->d_peers, nsrv, seg, cur_tbl, e->ncols, col,
                       (uint32_t)p, dir, pmode,
                       ostat == 1 ? e->var2col(o) : 0,
                       ostat == 2 ? (sid_t)o : 0, (uint64_t)e->cap_rows,
                       e->d_state, e->d_stats, out_tbl);
    TIME_END(e, CAT_PROBE);
    // commit inlined in k_peer_step (single block)
    if (pmode == PM_SIZE)
        finish_step(e, o, e->ncols + 1, e->cap_rows, 1);
    else
        finish_step(e, 0, e->ncols, e->bound, 1);
    return WK_OK;
}

// ---------------------------------------------------------------------
// One step_* function per operator; exec_pattern (below) validates,
// picks the operator and calls it.  step_ctx carries the pattern and
// the two table buffers; col/key_mode/seg are filled for known-start
// steps only.
// ---------------------------------------------------------------------
struct step_ctx {
    ssid_t s, p, o;
    int dir;
    const sid_t *cur_tbl;  // current table (may be a zero-copy view)
    sid_t *out_tbl;        // the other buffer
    int col = -1;          // column of the known subject
    int key_mode = PK_NORMAL;
    const seg_t *seg = nullptr;  // segment of the fixed (pid,dir)
};

// ---- OPTIONAL-mode dispatch (sparql.hpp:100-170,316-375) ----
static int32_t step_optional(wk_engine *e, const step_ctx &c) {
    const wk_store *st = e->st;
    const ssid_t s = c.s, p = c.p, o = c.o;
    const int dir = c.dir;
    if (p < 0) return WK_ERR_PLAN;  // BGP-only, like the reference
    const bool cstart = s >= 0;
    if (cstart && is_tpid(s)) return WK_ERR_PLAN;  // no index starts
    int ocol = cstart ? e->var2col(o) : e->var2col(s);
    if (ocol < 0 && cstart) return WK_ERR_PLAN;  // c2u inside OPTIONAL
    if (!cstart && e->var2col(s) < 0) return WK_ERR_PLAN;
    const int ostat = e->var_stat(o);
    const seg_t *oseg = st->seg_of((uint64_t)1 << NBITS_IDX, (uint64_t)p, dir);
    int okey_mode = PK_NORMAL;
    if (!cstart && ostat == 0 && (sid_t)p == TYPE_ID && dir == DIR_IN) {
        okey_mode = PK_INDEX;
        oseg = &st->iseg[DIR_IN];
    }
    uint64_t bs = oseg ? oseg->bucket_start : 0;
    uint64_t nb = oseg ? oseg->num_buckets : 0;
    if (cstart || ostat != 0) {
        // filter-style: in place, flags transition, no compaction
        uint64_t loff = 0, lsz = 0;
        int pm;
        int fcol, fcol2 = 0;
        sid_t fcval = 0;
        if (cstart) {  // const_to_known (sparql.hpp:138-186, OPTIONAL)
            const sid_t *ptr =
                store_get(*st, (uint64_t)s, (uint64_t)p, dir, &lsz);
            loff = ptr ? (uint64_t)(ptr - st->edges.data()) : 0;
            pm = PM_LIST;
            fcol = ocol;
        } else {
            pm = (ostat == 2) ? PM_CONST : PM_COL;
            fcol = e->var2col(s);
            fcol2 = (ostat == 1) ? e->var2col(o) : 0;
            fcval = (ostat == 2) ? (sid_t)o : 0;
        }
        TIME_BEGIN(e);
        // exec_pattern materialised any view: the owned buffer IS current
        hipLaunchKernelGGL(k_filter_opt, dim3(grid_for(e->bound)),
                           dim3(BLOCK), 0, e->stream, e->d_verts,
                           e->d_edges, bs, nb,
                           (sid_t *)e->tbl[e->cur].p, e->ncols, fcol,
                           (uint32_t)p, dir, pm, fcol2, fcval, loff, lsz,
                           e->opt_mask, (uint8_t *)e->oflag[e->ocur].p,
                           e->d_state, e->d_stats);
        TIME_END(e, CAT_FILTER);
        // nrows unchanged; no commit (S_NROWS stays), no table flip
        finish_step_in_place(e, 0, e->ncols, e->bound, 1);
        return WK_OK;
    }
    // known_to_unknown inside OPTIONAL: append column, keep rows
    const int oc = e->ncols + 1;
    if (oc > e->cap_cols) return WK_ERR_STATE;
    TIME_BEGIN(e);
    hipLaunchKernelGGL(k_expand_opt, dim3(grid_for(e->bound)),
                       dim3(BLOCK), 0, e->stream, e->d_verts, e->d_edges,
                       c.cur_tbl, e->ncols, e->var2col(s), (uint32_t)p, dir,
                       okey_mode, bs, nb,
                       (const uint8_t *)e->oflag[e->ocur].p,
                       (uint8_t *)e->oflag[e->ocur ^ 1].p, c.out_tbl,
                       (uint64_t)e->cap_rows, e->d_state, e->d_stats);
    TIME_END(e, CAT_EXPAND);
    launch_commit(e);
    e->opt_mask |= 1u << e->ncols;
    e->ocur ^= 1;
    finish_step(e, o, oc, e->cap_rows, 1);
    return WK_OK;
}

// ---- VERSATILE: predicate variable (sparql.hpp:556-744) ----
static int32_t step_versatile(wk_engine *e, const step_ctx &c) {
    const wk_store *st = e->st;
    const ssid_t s = c.s, p = c.p, o = c.o;
    const int dir = c.dir;
    if (!st->vp_n || !e->gs || !e->gs->d_segtab) return WK_ERR_PLAN;
    int pvar = -(p + 1);
    if (pvar >= e->nvars || e->v2c[pvar] >= 0) return WK_ERR_PLAN;
    const bool cstart = s >= 0;
    int col = -1;
    if (cstart) {
        // const_unknown_* must be the first pattern (sparql.hpp:719)
        if (e->ncols != 0 || is_tpid(s)) return WK_ERR_PLAN;
    } else {
        col = e->var2col(s);
        if (col < 0) return WK_ERR_PLAN;
    }
    const int ostat = e->var_stat(o);
    if (ostat == 1) return WK_ERR_PLAN;  // known_unknown_known: absent
                                         // in the reference too
    const int end_mode = (ostat == 2) ? VU_END_CONST : VU_END_NEW;
    const int oc = e->ncols + (end_mode == VU_END_CONST ? 1 : 2);
    if (oc > e->cap_cols) return WK_ERR_STATE;
    int G = (int)std::min<int64_t>(std::max<int64_t>(e->bound, 1), 4096);
    if (cstart) G = 1;
    TIME_BEGIN(e);
    hipLaunchKernelGGL(k_vu, dim3(G), dim3(64), 0, e->stream,
                       e->d_verts, e->d_edges, c.cur_tbl, e->ncols, col,
                       cstart ? (sid_t)s : 0,
                       e->gs->d_vp_off[dir], e->gs->d_vp_edges[dir],
                       st->vp_base, st->vp_n, e->gs->d_segtab,
                       st->max_pid, dir, end_mode,
                       ostat == 2 ? (sid_t)o : 0, c.out_tbl, oc,
                       (uint64_t)e->cap_rows, e->d_state, e->d_stats);
    TIME_END(e, CAT_EXPAND);
    launch_commit(e);
    // two appended columns: the predicate, then (VU_END_NEW) the object
    e->v2c[pvar] = e->ncols;
    if (end_mode == VU_END_NEW) e->v2c[-(o + 1)] = e->ncols + 1;
    finish_step(e, 0, oc, e->cap_rows, 1);
    return WK_OK;
}

// ---- step 0: index start (query.hpp:660-682) / const start ----
// index_to_unknown (sparql.hpp:194-231) or const_to_unknown (:238-285):
// a host-probed list becomes a 1-col table
static int32_t step_start(wk_engine *e, const step_ctx &c, bool index_start) {
    const wk_store *st = e->st;
    if (!index_start && e->ncols != 0) return WK_ERR_PLAN;
    uint64_t sz = 0;
    const sid_t *ptr =
        index_start ? store_get(*st, 0, (uint64_t)c.s, c.dir, &sz)
                    : store_get(*st, (uint64_t)c.s, (uint64_t)c.p, c.dir, &sz);
    uint64_t off = ptr ? (uint64_t)(ptr - st->edges.data()) : 0;
    int32_t rc = grow_caps(e, (int64_t)sz, e->nvars);
    if (rc) return rc;
    launch_set_rows(e, sz);
    // the new table REPLACES whatever was current: ?o is column 0
    e->v2c[-(c.o + 1)] = 0;
    finish_step(e, 0, 1, (int64_t)sz, 1);
    // zero-copy: the 1-col table IS the stored edge list (immutable)
    e->tbl_view = sz ? e->d_edges + off : nullptr;
    e->nrows = (int64_t)sz;
    return WK_OK;
}

// ---- const_to_known (sparql.hpp:138-186): fixed-list membership ----
static int32_t step_const_to_known(wk_engine *e, const step_ctx &c) {
    const wk_store *st = e->st;
    int col = e->var2col(c.o);
    if (col < 0) return WK_ERR_PLAN;
    uint64_t sz = 0;
    const sid_t *ptr =
        store_get(*st, (uint64_t)c.s, (uint64_t)c.p, c.dir, &sz);
    uint64_t off = ptr ? (uint64_t)(ptr - st->edges.data()) : 0;
    TIME_BEGIN(e);
    launch_filter_tpr(e, fparams_list(e, e->d_edges, c.cur_tbl, col, c.dir,
                                      off, sz), 0, c.out_tbl);
    TIME_END(e, CAT_FILTER);
    launch_commit(e);
    finish_step(e, 0, e->ncols, e->bound, 1);
    return WK_OK;
}

// known start, segment absent: every probe misses -> empty table, left
// in place (no kernel wrote the other buffer)
static int32_t step_absent_segment(wk_engine *e, const step_ctx &c,
                                   int ostat) {
    hipLaunchKernelGGL(k_set_state, dim3(1), dim3(1), 0, e->stream, e->d_state, 0);
    e->nrows = 0;
    if (ostat == 0)
        finish_step_in_place(e, c.o, e->ncols + 1, 0, 1);
    else
        finish_step_in_place(e, 0, e->ncols, 0, 1);
    return WK_OK;
}

// ---- known_to_const / known_to_known filter (sparql.hpp:416-476) ----
static int32_t step_filter(wk_engine *e, const step_ctx &c, int ostat) {
    const wk_store *st = e->st;
    const ssid_t p = c.p, o = c.o;
    const int dir = c.dir;
    int pmode = (ostat == 2) ? PM_CONST : PM_COL;
    int col2 = (ostat == 1) ? e->var2col(o) : 0;
    sid_t cval = (ostat == 2) ? (sid_t)o : 0;
    // identity-verified filter: the graph build's warm pass saw this
    // step keep every row, so the captured graph runs a read-only
    // verification (typeof/membership checks on every row, misses ->
    // sticky S_DONE -> S_ERR at the publish -> replay discarded + safe
    // fallback) with no compaction write, no table flip and no commit
    // launch (q7's COURSE filter: 86us -> ~40us)
    const bool verify_only = hint_nodrop(e, e->step);
    TIME_BEGIN(e);
    int use_typeof = (pmode == PM_CONST && (sid_t)p == TYPE_ID &&
                      dir == DIR_OUT && c.key_mode == PK_NORMAL &&
                      e->d_type_of != nullptr)
                         ? 1 : 0;
    const uint64_t *d_tbm = use_typeof ? type_bitmap(e, cval) : nullptr;
    // functional predicate: row's single object replaces the probe.
    // If only the REVERSED direction is functional, k2k checks
    // fn[other col] == col (fn_swap); k2c resolves the single edge
    // endpoint HOST-side and becomes a pure equality compare (PM_EQ).
    const fnpage_t *d_pg = nullptr;
    const sid_t *d_vals = nullptr;
    int fn_swap = 0;
    if (!use_typeof && c.key_mode == PK_NORMAL && e->gs &&
        !e->gs->d_fn_pages.empty() && wk_fn_dispatch()) {
        d_pg = e->gs->d_fn_pages[(size_t)p * 2 + dir];
        d_vals = e->gs->d_fn_vals[(size_t)p * 2 + dir];
        // the REVERSED map keys the non-routed endpoint, which is
        // only complete on a single-partition store (the forward map
        // is partitioned on the same axis as the probe routing)
        if (!d_pg && st->nsrv == 1) {
            const fnpage_t *rpg = e->gs->d_fn_pages[(size_t)p * 2 + (dir ^ 1)];
            if (rpg && pmode == PM_COL) {
                d_pg = rpg;
                d_vals = e->gs->d_fn_vals[(size_t)p * 2 + (dir ^ 1)];
                fn_swap = 1;
            } else if (rpg && pmode == PM_CONST) {
                // host lookup: the const's single neighbour
                sid_t tv = st->fn_get((size_t)p * 2 + (dir ^ 1), cval);
                pmode = PM_EQ;
                cval = tv;  // 0 never matches a vid -> empty result
            }
        }
    }
    fparams P{e->d_verts, e->d_edges, c.seg->bucket_start,
              c.seg->num_buckets, c.cur_tbl, e->ncols, c.col, (uint32_t)p,
              dir, c.key_mode, pmode, col2, cval, 0, 0, e->d_type_of,
              st->type_base, st->type_n, use_typeof, d_tbm,
              d_pg, d_vals, st->fn_base, st->fn_n, fn_swap};
    // one-pass ballot filter: measured FASTER than the
    // flags+scan+scatter pipeline at suite keep-rates (graph-q1
    // 205 -> 264 us with the pipeline: the extra passes cost more
    // than the per-tile cursor atomics they remove)
    launch_filter_tpr(e, P, verify_only ? 1 : 0, c.out_tbl);
    TIME_END(e, CAT_FILTER);
    if (verify_only) {
        // no rows written, S_NROWS/S_TOTAL untouched: the table stays
        // where it is
        finish_step_in_place(e, 0, e->ncols, e->bound, 1);
        return WK_OK;
    }
    launch_commit(e);
    finish_step(e, 0, e->ncols, e->bound, 1);
    return WK_OK;
}

// known_to_unknown over a FUNCTIONAL predicate (deg==1 rank-compressed
// map): probe+scan+expand collapse to a page+value gather pair +
// compacted append, with an optional fused typeof filter on the new
// column.  Output rows <= input rows, so no capacity risk; e->bound is
// unchanged.
static int32_t step_k2u_fn(wk_engine *e, const step_ctx &c,
                           const fnpage_t *d_pg, const sid_t *d_vals) {
    // this look-ahead needs the dense type_of and the [v|TYPE|OUT]
    // segment (k_fn_gather's multi-type probe); unlike step_k2u's
    // it is NOT disabled while hinting
    sid_t fcval = (e->d_type_of && e->st->nsrv == 1) ? typeof_lookahead(e, c.o)
                                                     : 0;
    const seg_t *fseg =
        fcval ? e->st->seg_of((uint64_t)1 << NBITS_IDX, TYPE_ID, DIR_OUT)
              : nullptr;
    if (!(fseg && fseg->num_buckets)) fcval = 0;
    const bool fuse = fcval != 0;
    // optimistic 1:1 map: only while capturing a graph, and only
    // when the build's warm pass saw this step drop no rows
    const bool opt = hint_nodrop(e, e->step);
    TIME_BEGIN(e);
    if (opt)
        launch_expand_fn_map(e, c.cur_tbl, c.out_tbl, d_pg, d_vals, c.col,
                             fuse, fcval);
    else
        launch_expand_fn(e, c.cur_tbl, c.out_tbl, d_pg, d_vals, c.col,
                         fuse, fcval, fseg);
    TIME_END(e, CAT_EXPAND);
    // the scan pipeline committed in k_scan_mid; the 1:1 map keeps the
    // row count and needs no commit
    finish_step(e, c.o, e->ncols + 1, e->bound, fuse ? 2 : 1);
    return WK_OK;
}

// EXACT fused `k2u + ?v rdf:type CONST` compaction over the CSR index
// (nothing optimistic: output == expansion-then-filter output): the CSR
// walk counts type-bitmap-passing values, the scan yields exact
// positions, the writer re-walks and emits only those.
static int32_t step_k2u_tf(wk_engine *e, const step_ctx &c,
                           const fnpage_t *c_pg, const uint64_t *tf_tbm) {
    const wk_store *st = e->st;
    const int G = scan_grid(e->bound);
    launch_gather_scan(e, G, /*timed*/ true, [&] {
        hipLaunchKernelGGL(k_csr_gather_tf, dim3(grid_for(e->bound)),
                           dim3(BLOCK), 0, e->stream, c.cur_tbl, e->ncols,
                           c.col, c_pg,
                           e->gs->d_csr_entries[(size_t)c.p * 2 + c.dir],
                           st->fn_base, st->fn_n, e->d_edges, tf_tbm,
                           st->type_base, st->type_n, e->d_state, e->d_stats,
                           (uint64_t *)e->eoff.p, (uint32_t *)e->cnt.p);
    });
    {
        TIME_BEGIN(e);
        launch_expand_tf(e, c.cur_tbl, c.out_tbl, G, tf_tbm);
        TIME_END(e, CAT_EXPAND);
    }
    // consumed the typeof filter pattern too
    finish_step(e, c.o, e->ncols + 1, e->cap_rows, 2);
    return WK_OK;
}

// classic known_to_unknown: CSR gather (24-B probes) or fused cluster-
// hash probe+scan -> cross-block scan -> input-centric expansion (+
// big-row wave pass)
static int32_t step_k2u_classic(wk_engine *e, const step_ctx &c,
                                const fnpage_t *c_pg) {
    const wk_store *st = e->st;
    const int G = scan_grid(e->bound);
    if (c_pg) {
        launch_gather_scan(e, G, /*timed*/ true, [&] {
            hipLaunchKernelGGL(k_csr_gather, dim3(grid_for(e->bound)),
                               dim3(BLOCK), 0, e->stream, c.cur_tbl, e->ncols,
                               c.col, c_pg,
                               e->gs->d_csr_entries[(size_t)c.p * 2 + c.dir],
                               st->fn_base, st->fn_n, e->d_state, e->d_stats,
                               (uint64_t *)e->eoff.p, (uint32_t *)e->cnt.p);
        });
    } else {
        {
            TIME_BEGIN(e);
            hipLaunchKernelGGL(k_probe_scan, dim3(G), dim3(SCAN_T), 0,
                               e->stream, e->d_verts, c.cur_tbl, e->ncols,
                               c.col, (uint32_t)c.p, c.dir, c.key_mode,
                               c.seg->bucket_start, c.seg->num_buckets,
                               e->d_state, e->d_stats, (uint64_t *)e->eoff.p,
                               (uint32_t *)e->cnt.p, (uint64_t *)e->prefix.p,
                               (uint64_t *)e->bsums.p);
            TIME_END(e, CAT_PROBE);
        }
        {
            TIME_BEGIN(e);
            launch_scan_mid(e, G);
            TIME_END(e, CAT_SCAN);
        }
    }
    // verify-fused no-drop typeof on the NEW column (captured graphs
    // only, warm-pass hint — same guard scheme as fn_map): the
    // separate full-table verify pass collapses into the expansion's
    // write loop + a 1-thread epilogue.  Unlike the other two
    // look-aheads this one accepts the dense type_of OR the bitmap.
    expand_verify vf;
    if (hint_nodrop(e, e->step + 1) && st->nsrv == 1)
        vf.cval = typeof_lookahead(e, c.o);
    if (vf.cval) {
        vf.base = st->type_base;
        vf.n = st->type_n;
        vf.tbm = type_bitmap(e, vf.cval);
        vf.type_of = e->d_type_of;
        if (vf.tbm || vf.type_of) vf.on = 1;
    }
    {
        TIME_BEGIN(e);
        launch_expand(e, c.cur_tbl, c.out_tbl, G, vf);
        TIME_END(e, CAT_EXPAND);
    }
    // fan-out unknown until a sync point; a fused verify consumed the
    // filter pattern too
    finish_step(e, c.o, e->ncols + 1, e->cap_rows, vf.on ? 2 : 1);
    return WK_OK;
}

// The same exact pipeline with a per-row op chain as the per-edge
// predicate: consumes the k2u and the chain's patterns.
// NC input columns, candidates W wide (chain_narrow picks the bucket).
template <int NC, int W>
static void launch_k2u_chain(wk_engine *e, const step_ctx &c,
                             const fnpage_t *c_pg, const chain_plan &cp,
                             int G) {
    const wk_store *st = e->st;
    launch_gather_scan(e, G, /*timed*/ true, [&] {
        hipLaunchKernelGGL(
            (k_csr_gather_chain<NC, W>),
            dim3(chain_grid<k_csr_gather_chain<NC, W>>(e->bound)),
            dim3(BLOCK), 0, e->stream, c.cur_tbl, c.col, c_pg,
            e->gs->d_csr_entries[(size_t)c.p * 2 + c.dir], st->fn_base,
            st->fn_n, e->d_edges, cp.C, e->d_state, e->d_stats,
            (uint64_t *)e->eoff.p, (uint32_t *)e->cnt.p,
            (uint32_t *)e->pmask.p);
    });
    TIME_BEGIN(e);
    hipLaunchKernelGGL(
        (k_expand_chain<NC, W>),
        dim3(chain_grid<k_expand_chain<NC, W>>(e->bound)), dim3(BLOCK), 0,
        e->stream, c.cur_tbl, e->d_edges, (uint64_t *)e->eoff.p,
        (uint32_t *)e->cnt.p, (uint32_t *)e->pmask.p,
        (uint64_t *)e->prefix.p,
        (uint64_t *)e->bsums.p, G, cp.C, cp.out_cols, e->d_state,
        (uint64_t)e->cap_rows, e->d_stats, (uint32_t *)e->ovf.p,
        c.out_tbl);
    hipLaunchKernelGGL(
        k_expand_chain_big<NC>, dim3(512), dim3(BLOCK), 0, e->stream,
        c.cur_tbl, e->d_edges, (uint64_t *)e->eoff.p,
        (uint64_t *)e->prefix.p, (uint64_t *)e->bsums.p, G, cp.C,
        cp.out_cols, e->d_state, (uint64_t)e->cap_rows,
        (uint32_t *)e->ovf.p, c.out_tbl);
    TIME_END(e, CAT_EXPAND);
}
static int32_t step_k2u_chain(wk_engine *e, const step_ctx &c,
                              const fnpage_t *c_pg, const chain_plan &cp) {
    const int G = scan_grid(e->bound);
    const int nc_in = e->ncols;
    // the edge value needs a column of its own (step_k2u checked cap_cols)
    if (nc_in + 1 > ROW_MAX) return WK_ERR_STATE;
    const bool narrow = chain_narrow(cp.out_cols);
    with_ncols(nc_in, [&](auto nc) {
        constexpr int NC = decltype(nc)::value;
        if constexpr (NC < ROW_NARROW) {
            if (narrow) {
                launch_k2u_chain<NC, ROW_NARROW>(e, c, c_pg, cp, G);
                return;
            }
        }
        if constexpr (NC < ROW_MAX)
            launch_k2u_chain<NC, ROW_MAX>(e, c, c_pg, cp, G);
    });
    bind_chain_vars(e, cp, nc_in + 1);
    finish_step(e, c.o, cp.out_cols, e->cap_rows, 1 + cp.npat);
    return WK_OK;
}

// Stand-alone row pass: a run of >= 2 chain-eligible
// patterns over the current table (no expansion in front) as one
// compacting kernel + commit.  Exact: no hint is consulted for the
// consumed patterns and nothing counts into S_DONE, so inside a capture
// it replaces the optimistic 1:1 maps and verify-only filters it covers.
// Output rows <= input rows; e->bound is unchanged.
template <int NC, int W>
static void launch_row_chain(wk_engine *e, const step_ctx &c,
                             const chain_plan &cp) {
    hipLaunchKernelGGL((k_row_chain<NC, W>),
                       dim3(chain_grid<k_row_chain<NC, W>>(e->bound)),
                       dim3(BLOCK), 0, e->stream, c.cur_tbl, cp.C,
                       cp.out_cols, e->d_state, (uint64_t)e->cap_rows,
                       e->d_stats, c.out_tbl);
}
static int32_t step_row_chain(wk_engine *e, const step_ctx &c,
                              const chain_plan &cp) {
    const int nc_in = e->ncols;
    const bool narrow = chain_narrow(cp.out_cols);
    TIME_BEGIN(e);
    with_ncols(nc_in, [&](auto nc) {
        constexpr int NC = decltype(nc)::value;
        if constexpr (NC <= ROW_NARROW) {
            if (narrow) {
                launch_row_chain<NC, ROW_NARROW>(e, c, cp);
                return;
            }
        }
        launch_row_chain<NC, ROW_MAX>(e, c, cp);
    });
    TIME_END(e, CAT_FILTER);
    launch_commit(e);
    bind_chain_vars(e, cp, nc_in);
    finish_step(e, 0, cp.out_cols, e->bound, cp.npat);
    return WK_OK;
}

// known_to_unknown: pick the pipeline (fn map, exact typeof-fused CSR,
// classic)
static int32_t step_k2u(wk_engine *e, const step_ctx &c) {
    const wk_store *st = e->st;
    if (e->ncols + 1 > e->cap_cols) return WK_ERR_STATE;  // begin_query sizes cap_cols
    const size_t w_seg = (size_t)c.p * 2 + c.dir;
    // side indexes key [vid|pid|dir] only; WK_FN_DISPATCH=0 routes
    // around both (diagnostic / roofline probe of the classic pipeline)
    const bool side = c.key_mode == PK_NORMAL && e->gs && wk_fn_dispatch();
    if (side && !e->gs->d_fn_pages.empty() && e->gs->d_fn_pages[w_seg])
        return step_k2u_fn(e, c, e->gs->d_fn_pages[w_seg],
                           e->gs->d_fn_vals[w_seg]);
    // CSR side index (rank-compressed, non-functional segments); the
    // cluster-hash probe remains the fallback
    const fnpage_t *c_pg = (side && !e->gs->d_csr_pages.empty())
                               ? e->gs->d_csr_pages[w_seg]
                               : nullptr;
    // The typeof-fused CSR pipeline is skipped when the capture hint
    // says the filter drops nothing (the verify-fused classic expansion
    // is cheaper there), while hinting (per-pattern counts needed), and
    // on hub-heavy segments: its count pass walks a row's whole edge
    // list in one thread, so a 10^5-edge hub key would serialize (fine
    // for LUBM/WatDiv leaf predicates, avg deg <= ~8)
    const bool tf_deg_ok =
        w_seg < st->seg_keys.size() && st->seg_keys[w_seg] &&
        st->seg_edges[w_seg] / st->seg_keys[w_seg] <= 32;
    // a trailing chain that does more than the lone typeof filter (whose
    // two paths below are both measured) rides on the exact pipeline
    if (c_pg && tf_deg_ok && st->nsrv == 1 && chain_enabled(e)) {
        chain_plan cp;
        std::vector<int32_t> v2c = e->v2c;
        v2c[-(c.o + 1)] = e->ncols;
        collect_chain(e, e->step + 1, v2c, e->ncols + 1, cp);
        if (cp.nfilter && !cp.lone_typeof(e->ncols))
            return step_k2u_chain(e, c, c_pg, cp);
    }
    if (c_pg && tf_deg_ok && st->nsrv == 1 && !e->hinting &&
        !hint_nodrop(e, e->step + 1)) {
        const sid_t t = typeof_lookahead(e, c.o);
        const uint64_t *tf_tbm = t ? type_bitmap(e, t) : nullptr;
        if (tf_tbm) return step_k2u_tf(e, c, c_pg, tf_tbm);
    }
    return step_k2u_classic(e, c, c_pg);
}

// Run one pattern — dispatch per sparql.hpp:1016-1058.  Fully async: row
// counts live on device; a non-NULL nrows_out forces a sync (step API).
static int32_t exec_pattern(wk_engine *e) {
    if (!e || e->step >= (int)e->pats.size()) return WK_ERR_STATE;
    const wk_store *st = e->st;
    const wk_pattern_t pat = e->pats[e->step];
    // a start step's state write doubles as the query's begin kernel
    // (launch_set_rows); every other operator reads d_state, so a
    // pending begin zeroing goes first
    const bool index_start =
        (e->step == 0 && pat.subject >= 0 && is_tpid(pat.subject));
    const bool start =
        e->step != e->remote_step_idx && !e->opt_mode && pat.predicate >= 0 &&
        (index_start || (pat.subject >= 0 && pat.object < 0 &&
                         e->var2col(pat.object) < 0));
    if (!start) flush_begin(e);
    if (e->step == e->remote_step_idx) return exec_pattern_remote(e);
    // OPT-group kernels write the current table IN PLACE (BLANK fill):
    // a zero-copy i2u view must be materialised first
    if (e->opt_mode && e->tbl_view) {
        int32_t rcm = materialize_view(e);
        if (rcm) return rcm;
    }
    step_ctx c{pat.subject, pat.predicate, pat.object, pat.direction,
               cur_table(e), (sid_t *)e->tbl[e->cur ^ 1].p};
    if (e->opt_mode) return step_optional(e, c);
    if (c.p < 0) return step_versatile(e, c);

    if (start) return step_start(e, c, index_start);
    if (c.s >= 0) return step_const_to_known(e, c);

    // ---- known start ----
    c.col = e->var2col(c.s);
    if (c.col < 0) return WK_ERR_PLAN;  // UNKNOWN start: invalid plan (sparql.hpp:1044-1049)
    // segment of the fixed (pid,dir); known_to_unknown's TYPE_ID/IN case
    // probes the index segment with per-row type keys (sparql.hpp:340-343)
    if ((sid_t)c.p == TYPE_ID && c.dir == DIR_IN) {
        c.key_mode = PK_INDEX;
        c.seg = &st->iseg[DIR_IN];
    } else {
        c.seg = st->seg_of((uint64_t)1 << NBITS_IDX, (uint64_t)c.p, c.dir);
    }
    const int ostat = e->var_stat(c.o);
    if (!c.seg || c.seg->num_buckets == 0)
        return step_absent_segment(e, c, ostat);
    // a run of >= 2 per-row patterns from here on: one row pass
    if (c.key_mode == PK_NORMAL && st->nsrv == 1 && chain_enabled(e) &&
        wk_row_chain()) {
        chain_plan cp;
        collect_chain(e, e->step, e->v2c, e->ncols, cp);
        if (cp.npat >= 2) return step_row_chain(e, c, cp);
    }
    if (ostat != 0) return step_filter(e, c, ostat);
    return step_k2u(e, c);
}

extern "C" int32_t wk_engine_execute_one_pattern(wk_engine_t *e, int64_t *nrows_out) {
    double t0 = wk_verbose_lvl() >= 2 ? now_us() : 0;
    if (!e) return WK_ERR_STATE;
    if (e->step >= (int)e->pats.size()) {
        // already done (a fused step may consume two patterns): no-op
        if (nrows_out) {
            int32_t rc0 = sync_state(e);
            if (rc0) return rc0;
            *nrows_out = e->nrows;
        }
        return WK_OK;
    }
    // snapshot for the overflow re-run (step mode syncs per step, so
    // e->nrows/ncols/v2c are the pattern's INPUT state here)
    const int64_t in_rows = e->nrows;
    const int in_cur = e->cur;
    const int in_ncols = e->ncols;
    const int in_step = e->step;  // a fused step consumes TWO patterns
    // a zero-copy i2u/c2u input lives in the (immutable) store, not in
    // tbl[in_cur]: the step drops the view, the re-run must see it again
    const sid_t *const in_view = e->tbl_view;
    const std::vector<int32_t> in_v2c = e->v2c;
    int32_t rc = exec_pattern(e);
    if (rc == WK_OK && nrows_out) {
        for (int attempt = 0; attempt < 6; attempt++) {
            rc = sync_state(e);
            if (rc != WK_ERR_CAP) break;
            // restore the input state; grow (preserving the INPUT table,
            // now current again); re-run this pattern
            int64_t need = (int64_t)e->h_pin[S_REQ];
            e->cur = in_cur;
            e->tbl_view = in_view;
            e->nrows = in_rows;
            e->ncols = in_ncols;
            e->v2c = in_v2c;
            e->step = in_step;
            e->bound = in_rows;
            int32_t rc2 = grow_caps(e, need + need / 4, e->cap_cols);
            if (rc2) return rc2;
            e->zero_pending = true;  // clear the flags with the row reset
            launch_set_rows(e, (uint64_t)in_rows);
            rc = exec_pattern(e);
            if (rc) return rc;
        }
        if (rc == WK_OK && nrows_out) *nrows_out = e->nrows;
    }
    if (wk_verbose_lvl() >= 2)
        fprintf(stderr, "[pat] step=%d rows_out=%lld host_us=%.0f\n",
                e ? e->step - 1 : -1, (long long)(e ? e->nrows : -1),
                now_us() - t0);
    return rc;
}

extern "C" int32_t wk_engine_pattern_step(const wk_engine_t *e) { return e->step; }
extern "C" int32_t wk_engine_col_num(const wk_engine_t *e) { return e->ncols; }

// Sync the stream and return the current row count — pairs with
// async pattern execution (nrows_out = NULL): the distributed driver
// launches filter steps (outputs <= inputs, no overflow possible)
// without a host round-trip and resolves counts lazily at the next
// exchange point.
extern "C" int32_t wk_engine_row_count(wk_engine_t *e, int64_t *nrows_out) {
    if (!e || !nrows_out) return WK_ERR_STATE;
    int32_t rc = sync_state(e);
    if (rc == WK_OK) *nrows_out = e->nrows;
    return rc;
}

// Run the CURRENT pattern via the xGMI peer-probe path (small tables:
// in-place remote reads instead of an exchange — sparql.hpp:802-814).
// Requires wk_gpu_store_import_peers.  The overflow re-run inherits the
// remote routing through e->remote_step_idx.
extern "C" int32_t wk_engine_execute_one_pattern_remote(wk_engine_t *e,
                                                        int64_t *nrows_out) {
    if (!e) return WK_ERR_STATE;
    e->remote_step_idx = e->step;
    int32_t rc = wk_engine_execute_one_pattern(e, nrows_out);
    e->remote_step_idx = -1;
    return rc;
}

// Execute the CURRENT pattern (const- or index-start membership filter,
// sparql.hpp:80-186) against a CALLER-SUPPLIED sorted edge list instead
// of the local store.  The distributed driver broadcasts the owner
// rank's list first (the reference reads it in place over one-sided
// RDMA, gstore.hpp:260-338): a mid-plan constant's edge list lives only
// on rank `const % nsrv`, so filtering against the local store would
// drop every row on the other ranks.
extern "C" int32_t wk_engine_execute_filter_list(wk_engine_t *e,
                                                 const sid_t *host_list,
                                                 uint64_t n,
                                                 int64_t *nrows_out) {
    if (!e || e->step >= (int)e->pats.size()) return WK_ERR_STATE;
    const wk_pattern_t pat = e->pats[e->step];
    if (pat.subject < 0) return WK_ERR_PLAN;
    int col = e->var2col(pat.object);
    if (col < 0) return WK_ERR_PLAN;
    int32_t rc0 = sync_state(e);  // misc scratch may be in use upstream
    if (rc0) return rc0;
    if (e->misc.ensure(std::max<uint64_t>(n * sizeof(sid_t), 4)))
        return WK_ERR_HIP;
    if (n && hipMemcpyAsync(e->misc.p, host_list, n * sizeof(sid_t),
                            hipMemcpyHostToDevice, e->stream) != hipSuccess)
        return WK_ERR_HIP;
    const sid_t *cur_tbl = cur_table(e);
    sid_t *out_tbl = (sid_t *)e->tbl[e->cur ^ 1].p;
    TIME_BEGIN(e);
    launch_filter_tpr(e, fparams_list(e, (const sid_t *)e->misc.p, cur_tbl,
                                      col, pat.direction, 0, n), 0, out_tbl);
    TIME_END(e, CAT_FILTER);
    launch_commit(e);
    finish_step(e, 0, e->ncols, e->bound, 1);
    int32_t rc = sync_state(e);
    if (rc == WK_OK && nrows_out) *nrows_out = e->nrows;
    return rc;
}

extern "C" int32_t wk_engine_generate_sub_query(wk_engine_t *e, int32_t ndst,
                                                sid_t *dev_out, int64_t cap_rows,
                                                int64_t *rows_per_dst) {
    if (!e || ndst <= 0 || ndst > 64 || e->step >= (int)e->pats.size())
        return WK_ERR_STATE;
    const wk_pattern_t pat = e->pats[e->step];
    int col = e->var2col(pat.subject);
    if (col < 0) return WK_ERR_PLAN;
    int32_t rc = sync_state(e);
    if (rc) return rc;
    int64_t R = e->nrows;
    if (R > cap_rows) return WK_ERR_CAP;
    if (e->misc.ensure(128 * sizeof(unsigned long long))) return WK_ERR_HIP;
    unsigned long long *d_hist = (unsigned long long *)e->misc.p;
    hipLaunchKernelGGL(k_zero_words, dim3(1), dim3(128), 0, e->stream,
                       (uint64_t *)e->misc.p, 128);
    const sid_t *cur_tbl = cur_table(e);
    // per-(block,dst) bases live in the prefix scratch: G2*ndst <=
    // (R/BLOCK+1)*64 entries fit its (cap_rows+1) u64s unless the
    // capacity is tiny (cap_rows < 84 with ndst = 64), so size it here;
    // the stream is idle after sync_state and the scratch holds nothing
    const int G2 = (int)std::max<int64_t>(
        1, std::min<int64_t>(1024, (R + BLOCK - 1) / BLOCK));
    if (e->prefix.ensure((size_t)G2 * ndst * sizeof(unsigned long long)))
        return WK_ERR_HIP;
    unsigned long long *bh = (unsigned long long *)e->prefix.p;
    if (R) {
        TIME_BEGIN(e);
        hipLaunchKernelGGL(k_dst_count, dim3(G2), dim3(BLOCK), 0, e->stream,
                           cur_tbl, R, e->ncols, col, ndst, bh);
        hipLaunchKernelGGL(k_dst_scan2, dim3(1), dim3(64), 0, e->stream, bh,
                           G2, ndst, d_hist);
        TIME_END(e, CAT_SPLIT);
    }
    unsigned long long h_hist[64];
    HIP_CHECK(hipMemcpyAsync(h_hist, d_hist, ndst * sizeof(unsigned long long),
                             hipMemcpyDeviceToHost, e->stream));
    HIP_CHECK(stream_sync(e->stream));
    for (int i = 0; i < ndst; i++) rows_per_dst[i] = (int64_t)h_hist[i];
    if (R) {
        TIME_BEGIN(e);
        hipLaunchKernelGGL(k_dst_scatter2, dim3(G2), dim3(BLOCK), 0,
                           e->stream, cur_tbl, R, e->ncols, col, ndst, bh,
                           dev_out);
        TIME_END(e, CAT_SPLIT);
    }
    HIP_CHECK(stream_sync(e->stream));
    return WK_OK;
}

// download the current device table via a persistent PINNED staging
// buffer: a pageable-destination hipMemcpyAsync makes the NEXT queries'
// kernels stall ~25 ms (driver pin/unpin behind a large result copy,
// measured with tools/qloop.py)
static int32_t download_table(wk_engine *e, sid_t *dst, size_t n) {
    if (!n) return WK_OK;
    size_t bytes = n * 4;
    if (bytes > e->h_stage_cap) {
        if (e->h_stage) (void)hipHostFree(e->h_stage);
        e->h_stage = nullptr;
        e->h_stage_cap = 0;
        size_t want = bytes + bytes / 2;
        if (hipHostMalloc(&e->h_stage, want) != hipSuccess) return WK_ERR_HIP;
        e->h_stage_cap = want;
    }
    HIP_CHECK(hipMemcpyAsync(e->h_stage, cur_table(e), bytes,
                             hipMemcpyDeviceToHost, e->stream));
    HIP_CHECK(stream_sync(e->stream));
    memcpy(dst, e->h_stage, bytes);
    return WK_OK;
}

// ---- host-side final ops (final_process, sparql.hpp:1424-1551) ----
static int32_t finalize_result(wk_engine *e, const wk_plan_t *plan,
                               std::vector<sid_t> &tbl, wk_result_t *out) {
    int C = e->ncols;
    int64_t Rn = e->nrows;
    // DISTINCT: full-row sort, then drop ADJACENT rows equal on required
    // vars (exactly the reference's algorithm, sparql.hpp:1443-1472)
    if (plan->distinct && Rn > 0) {
        std::vector<int64_t> idx(Rn);
        for (int64_t i = 0; i < Rn; i++) idx[i] = i;
        std::sort(idx.begin(), idx.end(), [&](int64_t a, int64_t b) {
            for (int c = 0; c < C; c++) {
                sid_t x = tbl[a * C + c], y = tbl[b * C + c];
                if (x != y) return x < y;
            }
            return false;
        });
        std::vector<int> rcols;
        // a required var with no column compares equal on every row
        // (indexing with its -1 would read the neighbouring row)
        for (int i = 0; i < plan->nrequired; i++) {
            int c = e->var2col(plan->required_vars[i]);
            if (c >= 0) rcols.push_back(c);
        }
        std::vector<sid_t> kept;
        kept.reserve(tbl.size());
        auto eq_req = [&](int64_t a, int64_t b) {
            for (int c : rcols)
                if (tbl[a * C + c] != tbl[b * C + c]) return false;
            return true;
        };
        for (int64_t i = 0; i < Rn; i++) {
            if (i > 0 && eq_req(idx[i - 1], idx[i])) continue;
            for (int c = 0; c < C; c++) kept.push_back(tbl[idx[i] * C + c]);
        }
        tbl.swap(kept);
        Rn = (int64_t)tbl.size() / C;
    }
    // OFFSET / LIMIT (sparql.hpp:1494-1508)
    if (plan->offset > 0) {
        int64_t drop = std::min<int64_t>(plan->offset, Rn);
        tbl.erase(tbl.begin(), tbl.begin() + drop * C);
        Rn -= drop;
    }
    if (plan->limit >= 0 && Rn > plan->limit) {
        tbl.resize((size_t)plan->limit * C);
        Rn = plan->limit;
    }
    // projection to required vars (sparql.hpp:1510-1536)
    int RC = plan->nrequired;
    wk_sid_t *res = (wk_sid_t *)malloc(std::max<size_t>((size_t)Rn * RC * 4, 4));
    for (int64_t i = 0; i < Rn; i++)
        for (int j = 0; j < RC; j++) {
            int c = e->var2col(plan->required_vars[j]);
            res[i * RC + j] = (c >= 0) ? tbl[i * C + c] : BLANK_ID;
        }
    out->col_num = RC;
    out->row_num = Rn;
    out->table = res;
    out->status_code = 0;
    e->fin_count = Rn;
    return WK_OK;
}

// ---- device final ops -------------------------------
// WK_DEV_FINAL=0: DISTINCT/OFFSET/LIMIT on the host (finalize_result) and
// no final-op plans in graphs.  Read per call, like WK_CHAIN.
static bool wk_dev_final() {
    const char *v = getenv("WK_DEV_FINAL");
    return !(v && !atoi(v));
}
// WK_FINAL_HOST_ROWS (default 8192, read per call): a non-captured fetch
// of fewer rows keeps the host final ops — below that the ~30-launch
// device chain costs more than the host sort.  0 = always
// the device.  Captured graphs always end with the device pass.
static int64_t wk_final_host_rows() {
    const char *v = getenv("WK_FINAL_HOST_ROWS");
    return v ? atoll(v) : 8192;
}
static bool plan_has_final(const wk_plan_t *plan) {
    return plan->distinct || plan->limit >= 0 || plan->offset > 0;
}
// The device pass writes final_rows x nrequired words into the other
// table buffer (cap_rows x cap_cols) and indexes rows with u32.
static bool dev_final_ok(const wk_engine *e, const wk_plan_t *plan) {
    return plan->nrequired > 0 && plan->nrequired <= 8 &&
           plan->nrequired <= e->cap_cols && e->ncols >= 1 && e->ncols <= 8 &&
           e->cap_rows < ((int64_t)1 << 32);
}
static wk_engine::fin_sig_t fin_sig_of(const wk_plan_t *plan) {
    wk_engine::fin_sig_t s;
    s.distinct = plan->distinct ? 1 : 0;
    s.nrequired = plan->nrequired;
    s.limit = plan->limit >= 0 ? plan->limit : -1;
    s.offset = plan->offset > 0 ? plan->offset : 0;
    for (int j = 0; j < plan->nrequired && j < 8; j++)
        s.req[j] = plan->required_vars[j];
    return s;
}

// Enqueue the final pass over the current table (no sync, capturable: all
// scratch is sized by cap_rows in grow_caps, row counts come from
// d_state).  The finalized, projected table goes to tbl[cur ^ 1]; the
// current table — possibly a store view — is only read, and stays current.
static void launch_final(wk_engine *e, const wk_plan_t *plan) {
    flush_begin(e);
    fin_tbl T{cur_table(e), e->ncols, e->d_state, (uint64_t)e->cap_rows,
              e->d_fin, {(uint32_t *)e->cnt.p, (uint32_t *)e->pmask.p}};
    fin_emit E{};
    for (int j = 0; j < 8; j++)
        E.cols.c[j] = j < plan->nrequired ? e->var2col(plan->required_vars[j]) : -1;
    E.rc = plan->nrequired;
    E.offset = plan->offset > 0 ? (uint64_t)plan->offset : 0;
    E.limit = plan->limit >= 0 ? (uint64_t)plan->limit : ~(uint64_t)0;
    E.out = (sid_t *)e->tbl[e->cur ^ 1].p;
    TIME_BEGIN(e);
    if (plan->distinct) {
        const int G = fin_grid(e->cap_rows);
        uint32_t *hist = (uint32_t *)e->fhist.p;
        hipLaunchKernelGGL(k_zero_words, dim3(1), dim3(64), 0, e->stream,
                           e->d_fin, F_WORDS);
        hipLaunchKernelGGL(k_fin_live, dim3(grid_for(e->cap_rows)), dim3(BLOCK),
                           0, e->stream, T);
        for (int p = 0; p < 4 * e->ncols; p++) {
            hipLaunchKernelGGL(k_fin_hist, dim3(G), dim3(BLOCK), 0, e->stream,
                               T, p, hist);
            hipLaunchKernelGGL(k_fin_scan, dim3(1), dim3(FIN_SCAN_T), 0,
                               e->stream, T, p, hist, G);
            hipLaunchKernelGGL(k_fin_scatter, dim3(G), dim3(BLOCK), 0,
                               e->stream, T, p, hist);
        }
        // the block x digit matrix is done with: its head holds the
        // per-block kept counts
        hipLaunchKernelGGL(k_fin_flag, dim3(G), dim3(BLOCK), 0, e->stream, T, E,
                           (uint32_t *)e->ovf.p, hist);
        hipLaunchKernelGGL(k_fin_emit, dim3(G), dim3(BLOCK), 0, e->stream, T, E,
                           (const uint32_t *)e->ovf.p, hist);
    } else {
        hipLaunchKernelGGL(k_fin_window, dim3(grid_for(e->cap_rows)),
                           dim3(BLOCK), 0, e->stream, T, E);
    }
    hipLaunchKernelGGL(k_fin_publish, dim3(1), dim3(1), 0, e->stream, e->d_fin,
                       e->h_pin);
    TIME_END(e, CAT_OTHER);
}

extern "C" int32_t wk_engine_final_count(wk_engine_t *e, int64_t *n) {
    if (!e || !n || e->fin_count < 0) return WK_ERR_STATE;
    *n = e->fin_count;
    return WK_OK;
}

// Digit passes of the last device DISTINCT: how many ran, out of how many
// (4 per column); 0/0 when the last final pass sorted nothing.
extern "C" int32_t wk_engine_final_passes(wk_engine_t *e, int32_t *live,
                                          int32_t *total) {
    if (!e || !live || !total || !e->fin_table) return WK_ERR_STATE;
    *live = *total = 0;
    if (!e->fin_sig.distinct) return WK_OK;
    for (int c = 0; c < e->ncols && c < 8; c++)
        for (int k = 0; k < 4; k++)
            *live += ((e->h_pin[HP_FIN_LIVE + c] >> (8 * k)) & 0xFF) != 0;
    *total = 4 * e->ncols;
    return WK_OK;
}

extern "C" int32_t wk_engine_fetch_result(wk_engine_t *e, const wk_plan_t *plan,
                                          wk_result_t *out) {
    if (!e || !plan || !out) return WK_ERR_STATE;
    bool synced = false;  // the row-count cutoff below already synced
    if (!plan->blind && plan_has_final(plan) && wk_dev_final() &&
        dev_final_ok(e, plan)) {
        // final ops on DEVICE; after a replay of a graph that ends with
        // this very final pass the table is already there
        const wk_engine::fin_sig_t sig = fin_sig_of(plan);
        bool device = true;
        if (!(e->fin_table && e->fin_sig == sig)) {
            fin_invalidate(e);
            const int64_t cut = wk_final_host_rows();
            if (cut > 0) {  // the row count decides: one sync ahead
                int32_t rc = sync_state_grow(e);
                if (rc) return rc;
                synced = true;
                device = e->nrows >= cut;
            }
            if (device) {
                launch_final(e, plan);
                int32_t rc = sync_state_grow(e);
                if (rc) return rc;
                e->fin_count = (int64_t)e->h_pin[HP_FIN_COUNT];
                e->fin_table = true;
                e->fin_sig = sig;
            }
        }
        if (device) {
            double t0 = now_us();
            const int64_t rows = e->fin_count;
            size_t n = (size_t)rows * plan->nrequired;
            wk_sid_t *res = (wk_sid_t *)malloc(n ? n * 4 : 4);
            const sid_t *view = e->tbl_view;
            e->cur ^= 1;
            e->tbl_view = nullptr;  // the finalized table, for the download only
            int32_t rc = download_table(e, res, n);
            e->cur ^= 1;
            e->tbl_view = view;     // the pre-final table stays current
            if (rc) { free(res); return rc; }
            out->col_num = plan->nrequired;
            out->row_num = rows;
            out->table = res;
            out->status_code = 0;
            if (wk_verbose_lvl() >= 2)
                fprintf(stderr, "[fetch] rows=%lld final_rows=%lld d2h_us=%.0f\n",
                        (long long)e->nrows, (long long)rows, now_us() - t0);
            return WK_OK;
        }
    }
    // the device projection writes nrows x nrequired words into the other
    // table buffer, which holds cap_rows x cap_cols: repeated required
    // vars can make nrequired exceed cap_cols (nvars 1, nrequired 8), so
    // those plans project on the host
    const bool simple = !plan->distinct && plan->offset <= 0 && plan->limit < 0 &&
                        plan->nrequired <= 8 && plan->nrequired <= e->cap_cols;
    if (!plan->blind && simple && plan->nrequired > 0) {
        // project on DEVICE (sparql.hpp:1510-1536 semantics) and download
        // the projected table directly
        cols8 cols{};
        for (int j = 0; j < plan->nrequired; j++)
            cols.c[j] = e->var2col(plan->required_vars[j]);
        sid_t *out_tbl = (sid_t *)e->tbl[e->cur ^ 1].p;
        fin_invalidate(e);  // a finalized table in that buffer is overwritten
        flush_begin(e);
        TIME_BEGIN(e);
        hipLaunchKernelGGL(k_project, dim3(grid_for(e->cap_rows)), dim3(BLOCK), 0,
                           e->stream, cur_table(e), e->ncols,
                           e->d_state, cols, plan->nrequired, out_tbl);
        TIME_END(e, CAT_OTHER);
        int32_t rc = sync_state_grow(e);
        if (rc) return rc;
        double t0 = now_us();
        size_t n = (size_t)e->nrows * plan->nrequired;
        wk_sid_t *res = (wk_sid_t *)malloc(n ? n * 4 : 4);
        e->cur ^= 1;
        e->tbl_view = nullptr;  // projected table is current for the download
        rc = download_table(e, res, n);
        e->cur ^= 1;
        e->tbl_view = nullptr;
        if (rc) { free(res); return rc; }
        out->col_num = plan->nrequired;
        out->row_num = e->nrows;
        out->table = res;
        out->status_code = 0;
        if (wk_verbose_lvl() >= 2)
            fprintf(stderr, "[fetch] rows=%lld proj+d2h_us=%.0f\n",
                    (long long)e->nrows, now_us() - t0);
        return WK_OK;
    }
    int32_t rc = synced ? WK_OK : sync_state_grow(e);
    if (rc) return rc;  // WK_ERR_CAP -> caller re-runs (run_query does)
    if (plan->blind) {
        // Result::blind (query.hpp:321): row count only, no table
        out->col_num = plan->nrequired;
        out->row_num = e->nrows;
        out->table = nullptr;
        out->status_code = 0;
        return WK_OK;
    }
    double t0 = now_us();
    std::vector<sid_t> tbl((size_t)e->nrows * e->ncols);
    rc = download_table(e, tbl.data(), tbl.size());
    if (rc) return rc;
    double t1 = now_us();
    rc = finalize_result(e, plan, tbl, out);
    if (wk_verbose_lvl() >= 2)
        fprintf(stderr, "[fetch] rows=%lld d2h_us=%.0f final_us=%.0f\n",
                (long long)e->nrows, t1 - t0, now_us() - t1);
    return rc;
}

// raw current table (no final ops) — for the gloo-path exchange in tests
extern "C" int32_t wk_engine_fetch_raw(wk_engine_t *e, wk_result_t *out) {
    if (!e || !out) return WK_ERR_STATE;
    int32_t rc = sync_state_grow(e);
    if (rc) return rc;
    size_t n = (size_t)e->nrows * e->ncols;
    wk_sid_t *res = (wk_sid_t *)malloc(n ? n * 4 : 4);
    rc = download_table(e, res, n);
    if (rc) { free(res); return rc; }
    out->col_num = e->ncols;
    out->row_num = e->nrows;
    out->table = res;
    out->status_code = 0;
    return WK_OK;
}

// ---- FILTER expressions -----------------------------
// One k_filter_expr launch of a validated postfix program over the
// current table (which may be a zero-copy view into the store): the kept
// rows go to the other owned buffer, k_commit publishes the count, the
// buffers flip.  Always the compacting kernel, inside captures too.
// WK_ERR_PLAN: a referenced variable has no column yet.
static int32_t launch_filter_prog(wk_engine *e, const wk_fnode_t *prog, int n) {
    if (n <= 0 || n > WK_FILTER_MAX || e->ncols <= 0) return WK_ERR_PLAN;
    fprog_t P{};
    uint32_t used = 0;  // distinct operand columns
    auto operand = [&](int32_t x, int32_t &col, sid_t &val) {
        col = -1;
        val = 0;
        if (x > 0) { val = (sid_t)x; return true; }
        if (x == 0 || -(x + 1) >= (int)e->v2c.size()) return false;
        col = e->v2c[-(x + 1)];
        if (col < 0 || col >= e->ncols) return false;
        used |= 1u << col;
        return true;
    };
    for (int i = 0; i < n; i++) {
        fnode_d &d = P.node[i];
        d.op = prog[i].op;
        d.ca = d.cb = -1;
        if (d.op > WK_F_BOUND) continue;
        if (!operand(prog[i].a, d.ca, d.va)) return WK_ERR_PLAN;
        if (d.op != WK_F_BOUND && !operand(prog[i].b, d.cb, d.vb))
            return WK_ERR_PLAN;
    }
    P.tbl = cur_table(e);
    P.n = n;
    P.ncols = e->ncols;
    P.bytes_per_row = 4u * (uint32_t)__builtin_popcount(used) + 8u * e->ncols;
    flush_begin(e);
    TIME_BEGIN(e);
    hipLaunchKernelGGL(k_filter_expr, dim3(grid_for(e->bound)), dim3(BLOCK), 0,
                       e->stream, P, e->d_state, e->d_stats,
                       (sid_t *)e->tbl[e->cur ^ 1].p);
    TIME_END(e, CAT_FILTER);
    launch_commit(e);
    e->cur ^= 1;
    e->tbl_view = nullptr;
    fin_invalidate(e);
    return WK_OK;
}

// The conjuncts placed behind main-BGP patterns [from, to] — or, with
// from = to = -1, the ones waiting for the reference position — as ONE
// launch (their programs ANDed back together).  The one hook shared by
// run_whole_plan and the hint pass of graph_warm_hints, so submit,
// run_query, both graph builders and the hints all see the same tables.
static int32_t apply_filters(wk_engine *e, int from, int to, bool *ran) {
    if (ran) *ran = false;
    std::vector<wk_fnode_t> prog;
    int k = 0;
    for (const wk_engine::fconj &cj : e->conj) {
        if (cj.after < from || cj.after > to) continue;
        prog.insert(prog.end(), cj.prog.begin(), cj.prog.end());
        if (k++) prog.push_back(wk_fnode_t{WK_F_AND, 0, 0});
    }
    if (!k) return WK_OK;
    if (ran) *ran = true;
    return launch_filter_prog(e, prog.data(), (int)prog.size());
}

extern "C" int32_t wk_engine_execute_filter(wk_engine_t *e, int64_t *nrows_out) {
    if (!e) return WK_ERR_STATE;
    if (!e->filt.empty()) {
        int32_t rc = launch_filter_prog(e, e->filt.data(), (int)e->filt.size());
        if (rc) return rc;
    }
    if (nrows_out) {
        int32_t rc = sync_state(e);
        if (rc) return rc;
        *nrows_out = e->nrows;
    }
    return WK_OK;
}

// ---- empty-tail truncation of captured plans -------------------------
// Host bookkeeping of one pattern that runs on an EMPTY table: bind the
// variable a full run would bind, launch nothing.  false = a shape whose
// effect is not "append at most one column to the same table" (a
// const/index start REPLACES the table, a predicate variable appends
// two columns, an unbound subject is an invalid plan): such a tail is
// executed, not skipped.
static bool skip_empty_pattern(const wk_pattern_t &pat,
                               std::vector<int32_t> &v2c, int &ncols) {
    auto col = [&](ssid_t v) { return v < 0 ? v2c[-(v + 1)] : -1; };
    if (pat.predicate < 0) return false;
    if (pat.subject >= 0)  // const_to_known keeps the layout
        return pat.object < 0 && col(pat.object) >= 0;
    if (col(pat.subject) < 0) return false;
    if (pat.object < 0 && col(pat.object) < 0) v2c[-(pat.object + 1)] = ncols++;
    return true;
}

// The rest of the plan on an empty table: the engine's host state ends
// up exactly where a full run leaves it (v2c, ncols, step; bound 0).
// The in-capture publish guards the assumption (expect_empty).
static int32_t skip_empty_tail(wk_engine *e) {
    while (e->step < (int)e->pats.size()) {
        if (!skip_empty_pattern(e->pats[e->step], e->v2c, e->ncols))
            return WK_ERR_PLAN;  // graph_warm_hints validated the tail
        e->step++;
    }
    e->bound = 0;
    e->nrows = 0;
    return WK_OK;
}

// The main pattern list from the current step to its end, as a WHOLE
// plan: op chains may span patterns (whole_plan is set for exactly this
// scope, whatever path leaves it).
static int32_t run_whole_plan(wk_engine *e) {
    struct scope {
        wk_engine *e;
        explicit scope(wk_engine *e_) : e(e_) { e->whole_plan = true; }
        ~scope() { e->whole_plan = false; }
    } guard(e);
    while (e->step < (int)e->pats.size()) {
        // captured plan with an empty tail: nothing is launched for the
        // patterns the warm pass saw run on zero rows
        if (e->capturing && e->capture_empty_after >= 0 &&
            e->step > e->capture_empty_after)
            return skip_empty_tail(e);  // its filters launch nothing
        const int from = e->step;
        int32_t rc = exec_pattern(e);
        if (rc) return rc;
        // FILTER conjuncts due behind the patterns this step consumed
        if (!e->conj.empty()) {
            rc = apply_filters(e, from, e->step - 1, nullptr);
            if (rc) return rc;
        }
    }
    return WK_OK;
}

// asynchronous whole-plan submission: enqueue the full launch chain and
// return without any sync (pipelined multi-engine execution — the
// reference proxy's in-flight window, proxy.hpp:477-525)
// true when the whole plan is [c2u, typeof-filter] and the store has a
// complete single-type index (no 0xFFFF fallbacks anywhere)
static bool light2_eligible(wk_engine *e, const wk_plan_t *plan) {
    if (plan->npatterns != 2 || !e->d_type_of || e->st->type_multi) return false;
    if (plan->nfilter > 0) return false;  // k_light2 evaluates no FILTER
    const wk_pattern_t &p0 = plan->patterns[0];
    const wk_pattern_t &p1 = plan->patterns[1];
    if (p0.subject < 0 || is_tpid(p0.subject) || p0.object >= 0) return false;
    if (p1.subject != p0.object) return false;
    if (p1.predicate != (ssid_t)TYPE_ID || p1.direction != DIR_OUT ||
        p1.object <= 0)
        return false;
    return true;
}

extern "C" int32_t wk_engine_submit(wk_engine_t *e, const wk_plan_t *plan) {
    if (!e || !plan) return WK_ERR_STATE;
    if (plan->nopt > 0 || plan->nunion > 0)
        return WK_ERR_PLAN;  // UNION/OPTIONAL need the sync run_query path
    const bool light = light2_eligible(e, plan);
    int32_t rc = light ? begin_light(e, plan) : wk_engine_begin_query(e, plan);
    if (rc) return rc;
    if (light) {
        const wk_pattern_t &p0 = plan->patterns[0];
        uint64_t sz = 0;
        const sid_t *ptr = store_get(*e->st, (uint64_t)p0.subject,
                                     (uint64_t)p0.predicate, p0.direction, &sz);
        uint64_t off = ptr ? (uint64_t)(ptr - e->st->edges.data()) : 0;
        rc = grow_caps(e, (int64_t)sz, e->nvars);
        if (rc) return rc;
        flush_publish(e);
        TIME_BEGIN(e);
        hipLaunchKernelGGL(k_light2, dim3(1), dim3(BLOCK), 0, e->stream,
                           e->d_edges, off, sz, (sid_t)plan->patterns[1].object,
                           e->d_type_of, e->st->type_base, e->st->type_n,
                           e->d_state, e->d_stats, (sid_t *)e->tbl[1].p, e->h_pin);
        TIME_END(e, CAT_FILTER);
        e->cur = 1;
        e->ncols = 1;
        e->bound = (int64_t)sz;
        e->v2c[-(p0.object + 1)] = 0;
        e->step = 2;
        return WK_OK;
    }
    return run_whole_plan(e);
}

// WK_FORCE_EMPTY_HINT=<k> (test-only, read at graph build): assume the
// table is empty after pattern k whatever the warm pass saw, so the
// expect_empty guard's failing branch can be exercised
static int force_empty_hint() {
    const char *v = getenv("WK_FORCE_EMPTY_HINT");
    return v ? atoi(v) : -1;
}

// Warm + hint passes shared by both graph builders.  The warm pass
// settles scratch capacities so the capture never allocates.  The
// step-wise pass then records (a) which pattern steps dropped no rows
// and (b) the last pattern after which the table is empty through the
// end of the plan (*empty_after, -1 = none or nothing to skip).  The
// store is immutable, so both observations hold for every replay; the
// replay still guards them (sticky S_DONE misses, expect_empty) and
// raises S_ERR when one fails.
static int32_t graph_warm_hints(wk_engine *e, const wk_plan_t *plan,
                                std::vector<uint8_t> &hint,
                                int *empty_after) {
    *empty_after = -1;
    for (int attempt = 0; attempt < 4; attempt++) {
        int32_t rc = wk_engine_submit(e, plan);
        if (rc) return rc;
        rc = sync_state_grow(e);
        if (rc == WK_OK) break;
        if (rc != WK_ERR_CAP) return rc;
    }
    const int np = std::max(plan->npatterns, 0);
    hint.assign((size_t)np, 0);
    int32_t rc = wk_engine_begin_query(e, plan);
    if (rc) return rc;
    // host layout after each step, keyed by the last pattern it consumed
    // (the skipped tail's bookkeeping starts from one of these)
    struct layout { int last; std::vector<int32_t> v2c; int ncols; };
    std::vector<layout> seen;
    e->hinting = true;  // per-pattern counts: no multi-step fusions
    int64_t prev = -1;
    int empty_at = -1;
    bool filtered = false;  // a FILTER ran right behind the last pattern
    while (e->step < (int)e->pats.size()) {
        const int at = e->step;
        int64_t n = 0;
        rc = wk_engine_execute_one_pattern(e, &n);
        if (rc) { e->hinting = false; return rc; }
        // the hint is about the pattern itself; the filters behind it
        // then set the count the next pattern starts from.  A pattern
        // that starts from a freshly filtered table gets no hint: the
        // capture may fuse it into its predecessor (verify-fused
        // expansion), which tests it BEFORE that filter.
        if (n == prev && at < np && !filtered) hint[at] = 1;
        filtered = false;
        if (!e->conj.empty()) {
            rc = apply_filters(e, at, e->step - 1, &filtered);
            if (rc == WK_OK && filtered) {
                rc = sync_state(e);
                n = e->nrows;
            }
            if (rc) { e->hinting = false; return rc; }
        }
        prev = n;
        seen.push_back({e->step - 1, e->v2c, e->ncols});
        if (n != 0) empty_at = -1;
        else if (empty_at < 0) empty_at = e->step - 1;
    }
    e->hinting = false;
    const int forced = force_empty_hint();
    if (forced >= 0) empty_at = forced;
    if (empty_at < 0 || empty_at >= np - 1) return WK_OK;  // nothing to skip
    for (const layout &l : seen) {
        if (l.last < empty_at) continue;
        // the tail must be pure bookkeeping (skip_empty_pattern)
        std::vector<int32_t> v2c = l.v2c;
        int ncols = l.ncols;
        for (int i = l.last + 1; i < np; i++)
            if (!skip_empty_pattern(plan->patterns[i], v2c, ncols))
                return WK_OK;
        if (l.last < np - 1) *empty_after = l.last;
        break;
    }
    return WK_OK;
}

// WK_FUSE_PAIR=0: suite captures keep k_publish_state + k_begin_state
// as two launches between queries.  Read per call, like WK_CHAIN.
static bool wk_fuse_pair() {
    const char *v = getenv("WK_FUSE_PAIR");
    return !(v && !atoi(v));
}
// True when the plan's first launch in a capture is the begin-aware state
// write of step_start (exec_pattern's `start` at step 0): an index or
// constant start whose row count the host knows.  k_light2 plans begin
// and publish inside their one kernel.
static bool opens_with_begin_state(wk_engine *e, const wk_plan_t *plan) {
    if (plan->npatterns <= 0 || light2_eligible(e, plan)) return false;
    if (e->remote_step_idx == 0) return false;
    const wk_pattern_t &p = plan->patterns[0];
    return p.predicate >= 0 && p.subject >= 0 &&
           (is_tpid(p.subject) || p.object < 0);
}

static void end_capture_state(wk_engine *e) {
    e->capturing = 0;
    e->publish_pending = -1;
    e->capture_hint.clear();
    e->capture_empty_after = -1;
}

// ---------------------------------------------------------------------
// hipGraph replay of a whole fixed plan: the benchmark suite re-runs
// the same 7 queries every step, so each plan's launch chain (3 to 12
// dispatches, with its per-launch dispatch gaps) collapses into ONE
// hipGraphLaunch.  Build captures the submit chain (after a warm pass
// settles capacities — growth is illegal mid-capture); run replays it
// and returns the blind row count.  S_ERR on replay = capacity
// overflow: caller falls back to the plain submit path.
// ---------------------------------------------------------------------
extern "C" int32_t wk_engine_graph_build(wk_engine_t *e,
                                         const wk_plan_t *plan,
                                         int32_t *gid) {
    if (!e || !plan || !gid) return WK_ERR_STATE;
    if (plan->nopt > 0 || plan->nunion > 0) return WK_ERR_PLAN;
    // replay returns the BLIND row count (pre-DISTINCT/LIMIT); a plan
    // with final ops ends its chain with the device final pass, whose
    // count wk_engine_final_count reads.  Without the device pass such a
    // plan is refused: its caller would misread the count.
    const bool fin = plan_has_final(plan) && !plan->blind;
    if (plan_has_final(plan) && (plan->blind || !wk_dev_final()))
        return WK_ERR_PLAN;
    {
        int32_t rc = graph_warm_hints(e, plan, e->capture_hint,
                                      &e->capture_empty_after);
        if (rc) return rc;
    }
    e->capturing = 1;
    hipGraph_t g = nullptr;
    if (hipStreamBeginCapture(e->stream, hipStreamCaptureModeThreadLocal) !=
        hipSuccess) {
        end_capture_state(e);
        return WK_ERR_HIP;
    }
    int32_t rc = wk_engine_submit(e, plan);
    if (rc == WK_OK && fin) {
        if (dev_final_ok(e, plan)) launch_final(e, plan);
        else rc = WK_ERR_PLAN;  // host-only final ops: not replayable
    }
    if (rc == WK_OK && !e->light)
        launch_publish(e, e->capture_empty_after >= 0);
    hipError_t ce = hipStreamEndCapture(e->stream, &g);
    end_capture_state(e);
    if (rc != WK_OK || ce != hipSuccess || !g) {
        if (g) (void)hipGraphDestroy(g);
        // the capture aborted mid-chain: resynchronise engine state
        (void)stream_sync(e->stream);
        return rc != WK_OK ? rc : WK_ERR_HIP;
    }
    hipGraphExec_t ex = nullptr;
    if (hipGraphInstantiate(&ex, g, nullptr, nullptr, 0) != hipSuccess) {
        (void)hipGraphDestroy(g);
        return WK_ERR_HIP;
    }
    (void)hipGraphDestroy(g);
    wk_engine::wk_graph wg;
    wg.exec = ex;
    wg.v2c = e->v2c;
    wg.ncols = e->ncols;
    wg.cur = e->cur;
    wg.nvars = e->nvars;
    wg.bound = e->bound;
    wg.light = e->light;
    wg.view = e->tbl_view;
    wg.fin = fin;
    if (fin) wg.fin_sig = fin_sig_of(plan);
    e->graphs.push_back(std::move(wg));
    *gid = (int32_t)e->graphs.size() - 1;
    return WK_OK;
}

// Whole-SUITE capture: N plans recorded back-to-back into ONE
// instantiated graph, so a full benchmark pass pays the ~10-16 us
// graph-replay floor once instead of once per query (microarch row
// `graph-replay-floor`).  Each query keeps its own in-capture publish,
// so the sticky S_ERR overflow guard still sees every query.  Replay
// with wk_engine_graph_launch + wk_engine_sync; counts come from the
// per-query graphs / latency passes.
extern "C" int32_t wk_engine_graph_build_suite(wk_engine_t *e,
                                               const wk_plan_t *plans,
                                               int32_t nplans,
                                               int32_t *gid) {
    if (!e || !plans || nplans <= 0 || !gid) return WK_ERR_STATE;
    std::vector<std::vector<uint8_t>> hints((size_t)nplans);
    std::vector<int> empty_after((size_t)nplans, -1);
    for (int i = 0; i < nplans; i++) {
        const wk_plan_t *plan = &plans[i];
        if (plan->nopt > 0 || plan->nunion > 0) return WK_ERR_PLAN;
        // final-op plans end with the device final pass (graph_build)
        if (plan_has_final(plan) && (plan->blind || !wk_dev_final()))
            return WK_ERR_PLAN;
        int32_t rc = graph_warm_hints(e, plan, hints[i], &empty_after[i]);
        if (rc) return rc;
    }
    e->capturing = 1;
    hipGraph_t g = nullptr;
    if (hipStreamBeginCapture(e->stream, hipStreamCaptureModeThreadLocal) !=
        hipSuccess) {
        end_capture_state(e);
        return WK_ERR_HIP;
    }
    int32_t rc = WK_OK;
    for (int i = 0; i < nplans && rc == WK_OK; i++) {
        e->capture_hint = hints[i];
        e->capture_empty_after = empty_after[i];
        rc = wk_engine_submit(e, &plans[i]);
        if (rc == WK_OK && plan_has_final(&plans[i])) {
            if (dev_final_ok(e, &plans[i])) launch_final(e, &plans[i]);
            else rc = WK_ERR_PLAN;
        }
        if (rc == WK_OK && !e->light) {
            // the next query opens with k_begin_state(host-known rows):
            // hold this publish back for it (k_publish_begin)
            if (i + 1 < nplans && wk_fuse_pair() &&
                opens_with_begin_state(e, &plans[i + 1])) {
                flush_begin(e);
                e->publish_pending = empty_after[i] >= 0;
            } else {
                launch_publish(e, empty_after[i] >= 0);
            }
        }
    }
    if (rc == WK_OK) flush_publish(e);  // never left pending: see above
    hipError_t ce = hipStreamEndCapture(e->stream, &g);
    end_capture_state(e);
    if (rc != WK_OK || ce != hipSuccess || !g) {
        if (g) (void)hipGraphDestroy(g);
        (void)stream_sync(e->stream);
        return rc != WK_OK ? rc : WK_ERR_HIP;
    }
    hipGraphExec_t ex = nullptr;
    if (hipGraphInstantiate(&ex, g, nullptr, nullptr, 0) != hipSuccess) {
        (void)hipGraphDestroy(g);
        return WK_ERR_HIP;
    }
    (void)hipGraphDestroy(g);
    wk_engine::wk_graph wg;
    wg.exec = ex;
    wg.v2c = e->v2c;
    wg.ncols = e->ncols;
    wg.cur = e->cur;
    wg.nvars = e->nvars;
    wg.bound = e->bound;
    wg.light = e->light;
    wg.view = e->tbl_view;
    e->graphs.push_back(std::move(wg));
    *gid = (int32_t)e->graphs.size() - 1;
    return WK_OK;
}

// Asynchronous replay: enqueue the graph with NO sync — back-to-back
// graphs on one stream serialize safely (each begins with its own
// state-reset kernel), so a whole suite pass costs ONE host sync
// (wk_engine_sync).  Counts are not read back (throughput loops).
extern "C" int32_t wk_engine_graph_launch(wk_engine_t *e, int32_t gid) {
    if (!e || gid < 0 || gid >= (int32_t)e->graphs.size())
        return WK_ERR_STATE;
    if (hipGraphLaunch(e->graphs[gid].exec, e->stream) != hipSuccess)
        return WK_ERR_HIP;
    e->zero_pending = false;  // the replay began with its own begin kernel
    fin_invalidate(e);
    return WK_OK;
}

extern "C" int32_t wk_engine_sync(wk_engine_t *e) {
    if (!e) return WK_ERR_STATE;
    HIP_CHECK(stream_sync(e->stream));
    resolve_timing(e);
    if (e->h_pin[7]) {  // sticky S_ERR from ANY replay in the window
        e->h_pin[7] = 0;
        return WK_ERR_CAP;
    }
    return e->h_pin[S_ERR] ? WK_ERR_CAP : WK_OK;
}

extern "C" int32_t wk_engine_graph_run(wk_engine_t *e, int32_t gid,
                                       int64_t *nrows) {
    if (!e || gid < 0 || gid >= (int32_t)e->graphs.size())
        return WK_ERR_STATE;
    wk_engine::wk_graph &g = e->graphs[gid];
    resolve_timing(e);
    fin_invalidate(e);
    if (hipGraphLaunch(g.exec, e->stream) != hipSuccess) return WK_ERR_HIP;
    e->zero_pending = false;  // the replay began with its own begin kernel
    HIP_CHECK(stream_sync(e->stream));
    e->v2c = g.v2c;
    e->ncols = g.ncols;
    e->cur = g.cur;
    e->nvars = g.nvars;
    e->bound = g.bound;
    e->light = g.light;
    e->tbl_view = g.view;
    if (e->h_pin[S_ERR]) {
        e->h_pin[7] = 0;  // reported here, not to a later wk_engine_sync
        return WK_ERR_CAP;
    }
    e->nrows = (int64_t)e->h_pin[S_NROWS];
    if (nrows) *nrows = e->nrows;
    if (g.fin) {  // the replay left the finalized table in tbl[cur ^ 1]
        e->fin_count = (int64_t)e->h_pin[HP_FIN_COUNT];
        e->fin_table = true;
        e->fin_sig = g.fin_sig;
    }
    return WK_OK;
}

// Batched light-query window: n queries of the light2 shape
// (subject=constant, predicate, direction → ?x; rdf:type ?x == cval),
// SoA arrays so the host hands numpy buffers straight through.  One
// async launch for the whole window; harvest with
// wk_engine_light_batch_wait.  Returns WK_ERR_PLAN when the store
// cannot take the fast path (no single-type index) — callers fall back
// to per-query wk_engine_submit.
extern "C" int32_t wk_engine_submit_light_batch(wk_engine_t *e,
                                                const int64_t *subj,
                                                const int32_t *pred,
                                                const int32_t *dirs,
                                                const uint32_t *cval,
                                                int32_t n) {
    if (!e || !subj || !pred || !dirs || !cval || n <= 0 || n > (1 << 20))
        return WK_ERR_STATE;
    if (!e->d_type_of || e->st->type_multi) return WK_ERR_PLAN;
    if (e->lb_n >= 0) return WK_ERR_STATE;  // previous batch not harvested
    resolve_timing(e);

    size_t need = (size_t)n * (sizeof(light_desc) + 8);
    if (e->h_lb_cap < need) {
        if (e->h_lb) (void)hipHostFree(e->h_lb);
        e->h_lb = nullptr; e->h_lb_cap = 0;
        if (hipHostMalloc(&e->h_lb, need) != hipSuccess) return WK_ERR_HIP;
        e->h_lb_cap = need;
    }
    if (e->lbd.ensure((size_t)n * sizeof(light_desc))) return WK_ERR_HIP;
    if (e->lbcnt.ensure((size_t)n * 8)) return WK_ERR_HIP;

    light_desc *descs = (light_desc *)e->h_lb;
    uint64_t total = 0;
    for (int i = 0; i < n; i++) {
        uint64_t sz = 0;
        const sid_t *ptr = store_get(*e->st, (uint64_t)subj[i],
                                     (uint64_t)pred[i], (int)dirs[i], &sz);
        descs[i].off = ptr ? (uint64_t)(ptr - e->st->edges.data()) : 0;
        descs[i].sz = sz;
        descs[i].out_off = total;
        descs[i].cval = cval[i];
        descs[i].pad = 0;
        total += sz;
    }
    int32_t rc = grow_caps(e, (int64_t)total, 1);
    if (rc) return rc;
    HIP_CHECK(hipMemcpyAsync(e->lbd.p, descs, (size_t)n * sizeof(light_desc),
                             hipMemcpyHostToDevice, e->stream));
    TIME_BEGIN(e);
    hipLaunchKernelGGL(k_light_batch, dim3(n), dim3(LBLOCK), 0, e->stream,
                       e->d_edges, (const light_desc *)e->lbd.p,
                       e->d_type_of, e->st->type_base, e->st->type_n,
                       (sid_t *)e->tbl[1].p, (uint64_t *)e->lbcnt.p,
                       e->d_stats);
    TIME_END(e, CAT_FILTER);
    uint64_t *h_counts = (uint64_t *)(descs + n);
    HIP_CHECK(hipMemcpyAsync(h_counts, e->lbcnt.p, (size_t)n * 8,
                             hipMemcpyDeviceToHost, e->stream));
    e->lb_coff = (size_t)n * sizeof(light_desc);
    e->lb_n = n;
    e->cur = 1;
    e->ncols = 1;
    e->light = false;
    return WK_OK;
}

// Compile a light whole-plan template for the LDS interpreter; the
// per-query constant replaces patterns[0].subject.  WK_ERR_PLAN = shape
// not interpretable (caller uses the per-pattern path instead).
static int32_t compile_light_plan(const wk_engine *e, const wk_plan_t *plan,
                                  lplan_t *lp) {
    if (!plan || plan->npatterns < 1 || plan->npatterns > 8) return WK_ERR_PLAN;
    if (plan->nvars < 1 || plan->nvars > 8) return WK_ERR_PLAN;
    if (plan->distinct || plan->limit >= 0) return WK_ERR_PLAN;
    const wk_store *st = e->st;
    int32_t v2c[8];
    for (int i = 0; i < 8; i++) v2c[i] = -1;

    const wk_pattern_t &p0 = plan->patterns[0];
    if (p0.subject < 0 || is_tpid(p0.subject) || p0.object >= 0 ||
        p0.predicate < 0)
        return WK_ERR_PLAN;  // must be const_to_unknown, fixed predicate
    const wk::seg_t *seg = st->seg_of(1ull << NBITS_IDX,
                                      (uint64_t)p0.predicate, p0.direction);
    lp->ops[0] = {LOP_C2U, 0, 0, p0.direction, 0, (uint32_t)p0.predicate,
                  seg ? seg->bucket_start : 0, seg ? seg->num_buckets : 0};
    v2c[-(p0.object + 1)] = 0;
    int nc = 1, no = 1;

    for (int i = 1; i < plan->npatterns; i++) {
        const wk_pattern_t &p = plan->patterns[i];
        if (p.subject >= 0) return WK_ERR_PLAN;  // const-start mid-plan
        if (p.predicate < 0) return WK_ERR_PLAN;  // predicate variable
        int sidx = -(p.subject + 1);
        if (sidx >= plan->nvars || v2c[sidx] < 0) return WK_ERR_PLAN;
        int scol = v2c[sidx];
        lop_t op = {};
        op.col = scol;
        op.dir = p.direction;
        op.pid = (uint32_t)p.predicate;
        if (p.object >= 0) {  // constant object
            if ((sid_t)p.predicate == TYPE_ID && p.direction == DIR_OUT &&
                st->type_n && !st->type_multi) {
                op.op = LOP_TYPEOF;
                op.cval = (uint32_t)p.object;
            } else {
                const wk::seg_t *s2 = st->seg_of(
                    1ull << NBITS_IDX, (uint64_t)p.predicate, p.direction);
                op.op = LOP_K2C;
                op.cval = (uint32_t)p.object;
                op.bucket_start = s2 ? s2->bucket_start : 0;
                op.num_buckets = s2 ? s2->num_buckets : 0;
            }
        } else {
            int oidx = -(p.object + 1);
            if (oidx >= plan->nvars) return WK_ERR_PLAN;
            const wk::seg_t *s2 = st->seg_of(
                1ull << NBITS_IDX, (uint64_t)p.predicate, p.direction);
            op.bucket_start = s2 ? s2->bucket_start : 0;
            op.num_buckets = s2 ? s2->num_buckets : 0;
            if (v2c[oidx] >= 0) {
                op.op = LOP_K2K;
                op.col2 = v2c[oidx];
            } else {
                op.op = LOP_K2U;
                if (nc >= 8) return WK_ERR_PLAN;
                v2c[oidx] = nc++;
            }
        }
        lp->ops[no++] = op;
    }
    lp->nops = no;
    return WK_OK;
}

// Batched whole-plan light queries: n same-template queries, ONE launch,
// one wavefront workgroup interpreting the compiled plan per query with
// the binding table in LDS.  Blind replies only (counts); a query whose
// table outgrows LDS reports WK_LP_OVERFLOW_COUNT and must be re-run on
// the per-pattern path.  Harvest with wk_engine_light_batch_wait.
extern "C" int32_t wk_engine_submit_plan_batch(wk_engine_t *e,
                                               const wk_plan_t *tmpl,
                                               const int64_t *consts,
                                               int32_t n) {
    if (!e || !tmpl || !consts || n <= 0 || n > (1 << 20)) return WK_ERR_STATE;
    if (e->lb_n >= 0) return WK_ERR_STATE;
    if (tmpl->nfilter > 0) return WK_ERR_PLAN;  // the interpreter has no FILTER
    lplan_t lp = {};
    int32_t rc = compile_light_plan(e, tmpl, &lp);
    if (rc) return rc;
    resolve_timing(e);

    size_t need = (size_t)n * 16;  // consts then counts
    if (e->h_lb_cap < need) {
        if (e->h_lb) (void)hipHostFree(e->h_lb);
        e->h_lb = nullptr; e->h_lb_cap = 0;
        if (hipHostMalloc(&e->h_lb, need) != hipSuccess) return WK_ERR_HIP;
        e->h_lb_cap = need;
    }
    if (e->lbd.ensure((size_t)n * 8)) return WK_ERR_HIP;
    if (e->lbcnt.ensure((size_t)n * 8)) return WK_ERR_HIP;
    memcpy(e->h_lb, consts, (size_t)n * 8);
    HIP_CHECK(hipMemcpyAsync(e->lbd.p, e->h_lb, (size_t)n * 8,
                             hipMemcpyHostToDevice, e->stream));
    TIME_BEGIN(e);
    hipLaunchKernelGGL(k_plan_batch, dim3(n), dim3(64), 0, e->stream,
                       e->d_verts, e->d_edges, lp,
                       (const int64_t *)e->lbd.p, e->d_type_of,
                       e->st->type_base, e->st->type_n,
                       (uint64_t *)e->lbcnt.p, e->d_stats);
    TIME_END(e, CAT_FILTER);
    uint64_t *h_counts = (uint64_t *)((char *)e->h_lb + (size_t)n * 8);
    HIP_CHECK(hipMemcpyAsync(h_counts, e->lbcnt.p, (size_t)n * 8,
                             hipMemcpyDeviceToHost, e->stream));
    e->lb_coff = (size_t)n * 8;
    e->lb_n = n;
    return WK_OK;
}

// Blocks until the window completes; writes the n per-query row counts
// (blind replies, Result::blind — proxy.hpp:491).
extern "C" int32_t wk_engine_light_batch_wait(wk_engine_t *e,
                                              uint64_t *counts, int32_t n) {
    if (!e || e->lb_n < 0 || !counts || n != e->lb_n) return WK_ERR_STATE;
    HIP_CHECK(stream_sync(e->stream));
    const uint64_t *h_counts =
        (const uint64_t *)((const char *)e->h_lb + e->lb_coff);
    memcpy(counts, h_counts, (size_t)n * 8);
    e->lb_n = -1;
    resolve_timing(e);
    return WK_OK;
}

// UNION branches (sparql.hpp:1593-1614 + rmap.hpp:57-87): each branch
// continues from the main group's result table; the final table is the
// row-concat of the branch results.  All branches must end with the
// same variable->column layout.
static int32_t run_union(wk_engine *e, const wk_plan_t *plan) {
    int32_t rc = sync_state(e);
    if (rc) return rc;
    const int64_t pr = e->nrows;
    const int pc = e->ncols;
    const std::vector<int32_t> pv2c = e->v2c;
    const int pcur = e->cur;
    devbuf snap;
    size_t bytes = (size_t)pr * std::max(pc, 1) * 4;
    if (bytes && pc) {
        if (snap.ensure(bytes)) return WK_ERR_HIP;
        // cur_table: the parent may be a zero-copy i2u view; the
        // restore below rematerialises it into the owned buffer
        HIP_CHECK(hipMemcpyAsync(snap.p, cur_table(e), bytes,
                                 hipMemcpyDeviceToDevice, e->stream));
    }
    std::vector<sid_t> merged;
    std::vector<int32_t> bv2c;
    int bc = -1;
    const wk_pattern_t *bp = plan->union_pats;
    for (int b = 0; b < plan->nunion; b++) {
        if (b) {  // restore the parent state for the next branch
            e->v2c = pv2c;
            e->ncols = pc;
            e->cur = pcur;
            e->tbl_view = nullptr;  // snap restore materialises the view
            if (bytes && pc)
                HIP_CHECK(hipMemcpyAsync(e->tbl[pcur].p, snap.p, bytes,
                                         hipMemcpyDeviceToDevice, e->stream));
            hipLaunchKernelGGL(k_set_state, dim3(1), dim3(1), 0, e->stream,
                               e->d_state, (uint64_t)pr);
            e->nrows = pr;
            e->bound = pr;
        }
        e->pats.assign(bp, bp + plan->union_sizes[b]);
        e->step = 0;
        bp += plan->union_sizes[b];
        while (e->step < (int)e->pats.size()) {
            rc = exec_pattern(e);
            if (rc) { snap.release(); return rc; }
        }
        rc = sync_state_grow(e);
        if (rc) { snap.release(); return rc; }
        if (bc < 0) {
            bc = e->ncols;
            bv2c = e->v2c;
        } else if (bc != e->ncols || bv2c != e->v2c) {
            snap.release();
            return WK_ERR_PLAN;
        }
        size_t off = merged.size();
        merged.resize(off + (size_t)e->nrows * bc);
        if (e->nrows)
            HIP_CHECK(hipMemcpy(merged.data() + off, cur_table(e),
                                (size_t)e->nrows * bc * 4,
                                hipMemcpyDeviceToHost));
    }
    snap.release();
    int64_t mrows = bc > 0 ? (int64_t)(merged.size() / bc) : 0;
    rc = wk_engine_load_rbuf(e, merged.empty() ? nullptr : merged.data(),
                             mrows, bc, bv2c.data(), 0);
    if (rc) return rc;
    HIP_CHECK(stream_sync(e->stream));  // merged[] is about to go away
    return WK_OK;
}

// OPTIONAL pattern group (sparql.hpp:1616-1649, BGP-only): rows are
// kept; unmatched rows carry BLANK_ID in the columns first bound inside
// the group.
static int32_t run_optional(wk_engine *e, const wk_plan_t *plan) {
    int32_t rc = sync_state(e);
    if (rc) return rc;
    if (e->oflag[0].ensure((size_t)e->cap_rows) ||
        e->oflag[1].ensure((size_t)e->cap_rows))
        return WK_ERR_HIP;
    HIP_CHECK(hipMemsetAsync(e->oflag[0].p, 1, (size_t)e->cap_rows,
                             e->stream));
    HIP_CHECK(hipMemsetAsync(e->oflag[1].p, 1, (size_t)e->cap_rows,
                             e->stream));
    e->opt_mode = 1;
    e->ocur = 0;
    e->opt_mask = 0;
    e->pats.assign(plan->opt_patterns, plan->opt_patterns + plan->nopt);
    e->step = 0;
    while (e->step < (int)e->pats.size()) {
        rc = exec_pattern(e);
        if (!rc) rc = sync_state_grow(e);
        if (rc) {
            e->opt_mode = 0;
            return rc;
        }
    }
    e->opt_mode = 0;
    return WK_OK;
}

extern "C" int32_t wk_engine_run_query(wk_engine_t *e, const wk_plan_t *plan,
                                       wk_result_t *out) {
    for (int attempt = 0; attempt < 6; attempt++) {
        int32_t rc = wk_engine_begin_query(e, plan);
        if (rc) return rc;
        rc = run_whole_plan(e);
        if (rc) return rc;
        // UNION then OPTIONAL, the reference's order
        // (execute_sparql_query, sparql.hpp:1564-1662)
        if (plan->nunion > 0 && plan->union_pats && plan->union_sizes) {
            rc = run_union(e, plan);
            if (rc == WK_ERR_CAP) continue;
            if (rc) return rc;
        }
        if (plan->nopt > 0 && plan->opt_patterns) {
            rc = run_optional(e, plan);
            if (rc == WK_ERR_CAP) continue;
            if (rc) return rc;
        }
        // FILTER conjuncts on UNION-/OPTIONAL-born variables: the
        // reference's stage 4 (sparql.hpp:1651-1655)
        if (!e->conj.empty()) {
            rc = apply_filters(e, -1, -1, nullptr);
            if (rc) return rc;
        }
        rc = wk_engine_fetch_result(e, plan, out);
        if (rc != WK_ERR_CAP) return rc;
        // overflow: fetch grew the caps; re-run the whole query
    }
    return WK_ERR_CAP;
}

extern "C" void wk_result_free(wk_result_t *r) {
    if (r && r->table) { free(r->table); r->table = nullptr; }
}


extern "C" int32_t wk_engine_kernel_stats(wk_engine_t *e, double *usec7,
                                          double *bytes7, int64_t *launches7) {
    if (!e) return WK_ERR_STATE;
    for (int i = 0; i < CAT_COUNT; i++) {
        if (usec7) usec7[i] = e->cat_usec[i];
        if (bytes7) bytes7[i] = e->cat_bytes[i];
        if (launches7) launches7[i] = e->cat_n[i];
    }
    return WK_OK;
}

// layout pinning against tests/golden/hash_golden.csv (ref_dump.cpp)
extern "C" uint64_t wk_hash_u64(uint64_t x) { return hash_u64(x); }
extern "C" uint64_t wk_key_pack(uint64_t vid, uint64_t pid, uint64_t dir) {
    return key_pack(vid, pid, dir);
}
extern "C" uint64_t wk_ptr_pack(uint64_t size, uint64_t off, uint64_t type) {
    return ptr_pack(size, off, type);
}

// raw device allocation helpers (tests / exchange buffers without torch)
extern "C" void *wk_dev_alloc(uint64_t bytes) {
    void *p = nullptr;
    if (hipMalloc(&p, bytes ? bytes : 4) != hipSuccess) return nullptr;
    return p;
}
extern "C" void wk_dev_free(void *p) { if (p) (void)hipFree(p); }
extern "C" int32_t wk_dev_download(const void *dev, void *host, uint64_t bytes) {
    HIP_CHECK(hipMemcpy(host, dev, bytes, hipMemcpyDeviceToHost));
    return 0;
}

extern "C" const char *wk_build_arch(void) {
#if defined(__HIP_PLATFORM_AMD__)
    return "gfx950";
#else
    return "unknown";
#endif
}

extern "C" int32_t wk_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}
