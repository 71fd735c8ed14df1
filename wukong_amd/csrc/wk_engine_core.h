// wk_engine_core.h — error codes, the store and engine structs, knobs, timing,
// capacities, begin / publish / sync of the device state.
// Included by gpu_engine.hip only (one translation unit).
#pragma once

static double now_us() {
    return std::chrono::duration<double, std::micro>(
               std::chrono::steady_clock::now().time_since_epoch()).count();
}
static int wk_verbose_lvl() {
    static int v = -1;
    if (v < 0) { const char *e = getenv("WK_VERBOSE"); v = e ? atoi(e) : 0; }
    return v;
}

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
    ~devbuf() { release(); }  // locals (e.g. run_union_host's snapshot)
                              // free on every early-return path
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

// Where the current table is and how it is laid out: the engine fields
// cur, tbl_view, ncols, bound and v2c as one value (save_pos /
// restore_pos).  nrows, step, nvars and light are not part of it: the
// sites that need one of them say so next to the call.
struct table_pos {
    int cur = 0;
    const sid_t *view = nullptr;  // zero-copy view into the store, or null
    int ncols = 0;
    int64_t bound = 0;
    std::vector<int32_t> v2c;
};

// Set a field for a scope; the old value comes back on every way out.
template <class T>
struct scoped_set {
    T &ref;
    T old;
    scoped_set(T &r, T v) : ref(r), old(r) { ref = v; }
    ~scoped_set() { ref = old; }
    scoped_set(const scoped_set &) = delete;
    scoped_set &operator=(const scoped_set &) = delete;
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
    uint64_t *d_grp = nullptr;    // G_WORDS words (UNION group state)
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

    // UNION on the device: the parent-table snapshot the
    // branches restart from and the merged table they append to.  Sized
    // like tbl[] (cap_rows x cap_cols words), grow-only, allocated by the
    // first UNION plan (ensure_group_bufs) and grown with tbl[] from then
    // on (grow_caps), so no capture ever allocates.
    devbuf gsnap, gmerge;
    bool grp_bufs = false;
    // inside a UNION branch or the OPTIONAL group: e->pats is the group's
    // pattern list and e->step indexes it, so the per-main-pattern capture
    // hints do not apply (hint_nodrop)
    bool in_group = false;

    // OPTIONAL group execution state (every whole-plan entry point)
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
        table_pos pos;  // where the chain leaves its table
        int nvars = 0;
        bool light = false;
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
    // sized by the host bound: exact for a view into the store (step_start
    // sets it to the list length) and never more than the buffer holds;
    // e->nrows is valid only after a sync, which this path does not have
    size_t bytes = (size_t)std::max<int64_t>(e->bound, 0) *
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
static table_pos save_pos(const wk_engine *e) {
    return table_pos{e->cur, e->tbl_view, e->ncols, e->bound, e->v2c};
}
static void restore_pos(wk_engine *e, const table_pos &p) {
    e->cur = p.cur;
    e->tbl_view = p.view;
    e->ncols = p.ncols;
    e->bound = p.bound;
    e->v2c = p.v2c;
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

// ---- environment knobs ------------------------------------------------
// knob_on: true unless the variable is set and parses to 0.  knob_num:
// the variable's number, or dflt when unset.  Everything in this block is
// read PER CALL: the tests and bench.py flip these inside one process.
// (Cached instead: WK_VERBOSE, WK_SPIN_SYNC; WK_KERNEL_TIMING is read
// once per engine, at creation.)  README "Environment knobs" is the
// user-facing table of the same names.
static bool knob_on(const char *name) {
    const char *v = getenv(name);
    return !(v && !atoi(v));
}
static int64_t knob_num(const char *name, int64_t dflt) {
    const char *v = getenv(name);
    return v ? atoll(v) : dflt;
}
// 0 = route around the functional-predicate maps at dispatch (diagnostic /
// roofline probe of the classic pipeline)
static bool wk_fn_dispatch() { return knob_on("WK_FN_DISPATCH"); }
// 0 = no per-row op chains at all: every pattern runs as a step of its
// own
static bool wk_chain() { return knob_on("WK_CHAIN"); }
// 0 = no stand-alone row pass (k_row_chain); chains fused into CSR
// expansions stay on
static bool wk_row_chain() { return knob_on("WK_ROW_CHAIN"); }
// 0 = one chain op per round in plan order and no wave early-out: the
// plain op loop through the same kernels
static bool wk_chain_sched() { return knob_on("WK_CHAIN_SCHED"); }
// 0 = k_filter_tpr evaluates its rows one after another (filter_keep) on
// every path
static bool wk_filter_batch() { return knob_on("WK_FILTER_BATCH"); }
// 0 = the barrier-ladder k_scan_local/k_scan_mid in
// place of the wave-scan ones
static bool wk_wave_scan() { return knob_on("WK_SCAN"); }
// 0 = every FILTER conjunct runs at the reference's position (after the
// whole plan), not right behind the pattern that binds its last variable
static bool wk_filter_pushdown() { return knob_on("WK_FILTER_PUSHDOWN"); }
// 0 = DISTINCT/OFFSET/LIMIT on the host (finalize_result), and the graph
// builders refuse plans that have them
static bool wk_dev_final() { return knob_on("WK_DEV_FINAL"); }
// 0 = suite captures keep k_publish_state + k_begin_state as two launches
// between queries
static bool wk_fuse_pair() { return knob_on("WK_FUSE_PAIR"); }
// 0 = UNION / OPTIONAL plans only through wk_engine_run_query, with the
// host merge of the branches and a sync per group pattern; submit and the
// graph builders refuse them
static bool wk_dev_groups() { return knob_on("WK_DEV_GROUPS"); }
// default 8192: a non-captured fetch of fewer rows keeps the host final
// ops — below that the ~30-launch device chain costs more than the host
// sort.  0 = always the device.  Captured graphs always end
// with the device pass.
static int64_t wk_final_host_rows() {
    return knob_num("WK_FINAL_HOST_ROWS", 8192);
}
// scratch floor in rows (default 2^20): tests force tiny caps to exercise
// the overflow re-run
static int64_t min_cap_rows() { return knob_num("WK_MIN_CAP", 1 << 20); }
// <k> (test-only, consulted at graph build): assume the table is empty
// after pattern k whatever the warm pass saw, so the expect_empty guard's
// failing branch can be exercised
static int force_empty_hint() {
    return (int)knob_num("WK_FORCE_EMPTY_HINT", -1);
}
// Width bucket of the batched chain kernels: candidate
// rows are carried as sid_t[ROW_NARROW] when the plan's widened row fits,
// else as sid_t[ROW_MAX].  WK_CHAIN_WIDTH=8 forces the wide instantiation
// (A/B arm and fallback).
static bool chain_narrow(int out_cols) {
    return out_cols <= ROW_NARROW && knob_num("WK_CHAIN_WIDTH", 0) != ROW_MAX;
}
// Grid of the three batched chain kernels: grid_for's, but never more
// blocks than are resident at once at the kernel's compiled occupancy
// (queried once per instantiation), so that the grid-stride loops run as
// one batch; every instantiation at 8 waves per SIMD keeps 2048.
// WK_CHAIN_GRID=<n> caps it further, so that a test table of a few
// thousand rows makes one block walk several tiles / iterations.
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
    const int cap = (int)knob_num("WK_CHAIN_GRID", 0);
    return cap > 0 && cap < g ? cap : g;
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
    if (e->grp_bufs && (e->gsnap.ensure((size_t)rows * cols * 4) ||
                        e->gmerge.ensure((size_t)rows * cols * 4)))
        return WK_ERR_HIP;
    e->cap_rows = rows;
    e->cap_cols = cols;
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
    for (int i = 0; i < CAT_COUNT; i++) e->cat_bytes[i] = (double)e->h_pin[HP_STATS + i];
    if (e->h_pin[S_ERR]) {
        // reported here: the sticky slot belongs to the pipelined
        // graph_launch window and must not fail a later wk_engine_sync
        e->h_pin[HP_STICKY_ERR] = 0;
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
