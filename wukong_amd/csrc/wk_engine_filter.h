// wk_engine_filter.h — FILTER expressions: validation and placement (plan_filter),
// the launch, the hook shared by whole-plan runs and the hint pass.
// Included by gpu_engine.hip only (one translation unit).
#pragma once

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
