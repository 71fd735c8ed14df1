// wk_engine_graph.h — hipGraph capture and replay of whole plans: empty-tail
// truncation, warm and hint pass, capture_plans, build / launch / run.
// Included by gpu_engine.hip only (one translation unit).
#pragma once

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
    struct layout { int last; table_pos pos; };
    std::vector<layout> seen;
    // per-pattern counts: no multi-step fusions
    scoped_set<bool> hinting(e->hinting, true);
    int64_t prev = -1;
    int empty_at = -1;
    bool filtered = false;  // a FILTER ran right behind the last pattern
    while (e->step < (int)e->pats.size()) {
        const int at = e->step;
        int64_t n = 0;
        rc = wk_engine_execute_one_pattern(e, &n);
        if (rc) return rc;
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
            if (rc) return rc;
        }
        prev = n;
        seen.push_back({e->step - 1, save_pos(e)});
        if (n != 0) empty_at = -1;
        else if (empty_at < 0) empty_at = e->step - 1;
    }
    const int forced = force_empty_hint();
    if (forced >= 0) empty_at = forced;
    if (empty_at < 0 || empty_at >= np - 1) return WK_OK;  // nothing to skip
    for (const layout &l : seen) {
        if (l.last < empty_at) continue;
        // the tail must be pure bookkeeping (skip_empty_pattern)
        table_pos p = l.pos;
        for (int i = l.last + 1; i < np; i++)
            if (!skip_empty_pattern(plan->patterns[i], p.v2c, p.ncols))
                return WK_OK;
        if (l.last < np - 1) *empty_after = l.last;
        break;
    }
    return WK_OK;
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

// Everything a capture sets on the engine, dropped again on every way
// out of the scope that began it.
struct capture_scope {
    wk_engine *e;
    explicit capture_scope(wk_engine *e_) : e(e_) { e->capturing = 1; }
    ~capture_scope() {
        e->capturing = 0;
        e->publish_pending = -1;
        e->capture_hint.clear();
        e->capture_empty_after = -1;
    }
    capture_scope(const capture_scope &) = delete;
    capture_scope &operator=(const capture_scope &) = delete;
};

// ---------------------------------------------------------------------
// hipGraph replay of whole fixed plans: the benchmark suite re-runs the
// same 7 queries every step, so each plan's launch chain (3 to 12
// dispatches, with its per-launch dispatch gaps) collapses into ONE
// hipGraphLaunch.  capture_plans records the submit chains of n plans
// back-to-back into one instantiated graph, after the warm pass of EVERY
// plan has settled capacities — growth is illegal mid-capture.  Each
// plan keeps its own in-capture publish, so the sticky S_ERR overflow
// guard still sees every query; S_ERR on replay = capacity overflow or a
// failed hint: the caller falls back to the plain submit path.
//
// A plan with a UNION or an OPTIONAL group is one chain like any other
// (run_plan; refused under WK_DEV_GROUPS=0).  Its main BGP is never
// truncated, and inside the groups no warm-pass hint applies: the hints
// are indexed by main-BGP pattern (hint_nodrop).
//
// A plan with final ops ends its chain with the device final pass.
// Replay returns the BLIND row count (pre-DISTINCT/LIMIT) and
// wk_engine_final_count reads the final one, so without the device pass
// such a plan is refused: its caller would misread the count.
//
// single: the graph is one plan's, replayed with wk_engine_graph_run,
// which restores the host state the chain ends in — `fin`/`fin_sig`
// included, so that a following fetch finds the finalized table.  A suite
// graph records neither: it is replayed with wk_engine_graph_launch,
// which restores no host state at all (fin_invalidate only), and its
// counts come from the per-query graphs / latency passes.
// ---------------------------------------------------------------------
static int32_t capture_plans(wk_engine *e, const wk_plan_t *plans, int n,
                             bool single, int32_t *gid) {
    std::vector<std::vector<uint8_t>> hints((size_t)n);
    std::vector<int> empty_after((size_t)n, -1);
    for (int i = 0; i < n; i++) {
        const wk_plan_t *plan = &plans[i];
        const bool groups = plan->nopt > 0 || plan->nunion > 0;
        if (groups && !wk_dev_groups()) return WK_ERR_PLAN;
        if (plan_has_final(plan) && (plan->blind || !wk_dev_final()))
            return WK_ERR_PLAN;
        int32_t rc = graph_warm_hints(e, plan, hints[i], &empty_after[i]);
        if (rc) return rc;
        // A group plan keeps its whole main BGP: the publish guards a
        // truncated tail by expecting an EMPTY final table, and a UNION
        // branch that opens with a constant or index start replaces the
        // empty parent with rows of its own.
        if (groups) empty_after[i] = -1;
    }
    hipGraph_t g = nullptr;
    int32_t rc = WK_OK;
    hipError_t ce;
    {
        capture_scope capturing(e);
        if (hipStreamBeginCapture(e->stream, hipStreamCaptureModeThreadLocal) !=
            hipSuccess)
            return WK_ERR_HIP;
        for (int i = 0; i < n && rc == WK_OK; i++) {
            e->capture_hint = hints[i];
            e->capture_empty_after = empty_after[i];
            rc = wk_engine_submit(e, &plans[i]);
            if (rc == WK_OK && plan_has_final(&plans[i])) {
                if (dev_final_ok(e, &plans[i])) launch_final(e, &plans[i]);
                else rc = WK_ERR_PLAN;  // host-only final ops: not replayable
            }
            if (rc == WK_OK && !e->light) {
                // the next query opens with k_begin_state(host-known rows):
                // hold this publish back for it (k_publish_begin)
                if (i + 1 < n && wk_fuse_pair() &&
                    opens_with_begin_state(e, &plans[i + 1])) {
                    flush_begin(e);
                    e->publish_pending = empty_after[i] >= 0;
                } else {
                    launch_publish(e, empty_after[i] >= 0);
                }
            }
        }
        if (rc == WK_OK) flush_publish(e);  // never left pending: see above
        ce = hipStreamEndCapture(e->stream, &g);
    }
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
    wg.pos = save_pos(e);
    wg.nvars = e->nvars;
    wg.light = e->light;
    if (single && plan_has_final(&plans[0])) {
        wg.fin = true;
        wg.fin_sig = fin_sig_of(&plans[0]);
    }
    e->graphs.push_back(std::move(wg));
    *gid = (int32_t)e->graphs.size() - 1;
    return WK_OK;
}

extern "C" int32_t wk_engine_graph_build(wk_engine_t *e,
                                         const wk_plan_t *plan,
                                         int32_t *gid) {
    if (!e || !plan || !gid) return WK_ERR_STATE;
    return capture_plans(e, plan, 1, /*single*/ true, gid);
}

// Whole-SUITE capture: a full benchmark pass pays the ~10-16 us
// graph-replay floor once instead of once per query (microarch row
// `graph-replay-floor`).  Replay with wk_engine_graph_launch +
// wk_engine_sync.
extern "C" int32_t wk_engine_graph_build_suite(wk_engine_t *e,
                                               const wk_plan_t *plans,
                                               int32_t nplans,
                                               int32_t *gid) {
    if (!e || !plans || nplans <= 0 || !gid) return WK_ERR_STATE;
    return capture_plans(e, plans, nplans, /*single*/ false, gid);
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
    if (e->h_pin[HP_STICKY_ERR]) {  // sticky S_ERR from ANY replay in the window
        e->h_pin[HP_STICKY_ERR] = 0;
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
    restore_pos(e, g.pos);
    e->nvars = g.nvars;
    e->light = g.light;
    if (e->h_pin[S_ERR]) {
        e->h_pin[HP_STICKY_ERR] = 0;  // reported here, not to a later wk_engine_sync
        return WK_ERR_CAP;
    }
    e->nrows = (int64_t)e->h_pin[S_NROWS];  // the replay's own count
    if (nrows) *nrows = e->nrows;
    if (g.fin) {  // the replay left the finalized table in tbl[cur ^ 1]
        e->fin_count = (int64_t)e->h_pin[HP_FIN_COUNT];
        e->fin_table = true;
        e->fin_sig = g.fin_sig;
    }
    return WK_OK;
}
