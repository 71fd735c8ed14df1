// wk_engine_launch.h — what the step operators share: column-count dispatch,
// hints and maps, op-chain collection, end-of-step bookkeeping and the
// launch helpers of the scan / expand / filter pipelines.
// Included by gpu_engine.hip only (one translation unit).
#pragma once

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
// capturing a graph).  The hints are indexed by MAIN-BGP pattern: inside a
// UNION branch or the OPTIONAL group e->step counts the group's patterns
// and no hint applies.
static bool hint_nodrop(const wk_engine *e, int step) {
    return e->capturing && !e->in_group &&
           step < (int)e->capture_hint.size() &&
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

// (each launch_* below picks the kernels' compile-time column count with
// with_ncols, whose lambda launches them directly)
static void launch_expand(wk_engine *e, const sid_t *cur_tbl, sid_t *out_tbl,
                          int G, const expand_verify &vf) {
    with_ncols(e->ncols, [&](auto nc) {
        constexpr int NC = decltype(nc)::value;
        hipLaunchKernelGGL(k_expand_in<NC>, dim3(grid_for(e->bound)),
                           dim3(BLOCK), 0, e->stream, cur_tbl, e->ncols,
                           e->d_edges, (uint64_t *)e->eoff.p,
                           (uint32_t *)e->cnt.p, (uint64_t *)e->prefix.p,
                           (uint64_t *)e->bsums.p, G, e->d_state,
                           (uint64_t)e->cap_rows, e->d_stats,
                           (uint32_t *)e->ovf.p, vf.tbm, vf.type_of, vf.base,
                           vf.n, vf.cval, vf.on, out_tbl);
        hipLaunchKernelGGL(k_expand_big<NC>, dim3(512), dim3(BLOCK), 0,
                           e->stream, cur_tbl, e->ncols, e->d_edges,
                           (uint64_t *)e->eoff.p, (uint32_t *)e->cnt.p,
                           (uint64_t *)e->prefix.p, (uint64_t *)e->bsums.p, G,
                           e->d_state, (uint64_t)e->cap_rows,
                           (uint32_t *)e->ovf.p, vf.tbm, vf.type_of, vf.base,
                           vf.n, vf.cval, vf.on, out_tbl);
    });
    // a fused verify's misses sit in the sticky S_DONE word until the
    // publish: no epilogue launch
}

static void launch_expand_fn(wk_engine *e, const sid_t *cur_tbl,
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
    with_ncols(e->ncols, [&](auto nc) {
        hipLaunchKernelGGL(k_fn_scatter<decltype(nc)::value>,
                           dim3(grid_for(e->bound)), dim3(BLOCK), 0, e->stream,
                           cur_tbl, (const sid_t *)e->ovf.p,
                           (const uint32_t *)e->cnt.p,
                           (const uint64_t *)e->prefix.p,
                           (const uint64_t *)e->bsums.p, G, e->d_state,
                           e->d_stats, out_tbl);
    });
}

static void launch_expand_fn_map(wk_engine *e, const sid_t *cur_tbl,
                                 sid_t *out_tbl, const fnpage_t *d_pg,
                                 const sid_t *d_vals, int col,
                                 bool fuse, sid_t fcval) {
    const uint64_t *tbm = fuse ? type_bitmap(e, fcval) : nullptr;
    with_ncols(e->ncols, [&](auto nc) {
        hipLaunchKernelGGL(k_expand_fn_map<decltype(nc)::value>,
                           dim3(grid_for(e->bound)), dim3(BLOCK), 0, e->stream,
                           cur_tbl, d_pg, d_vals, e->st->fn_base, e->st->fn_n,
                           col, fuse ? 1 : 0, tbm, e->d_type_of,
                           e->st->type_base, e->st->type_n, fcval, e->d_state,
                           e->d_stats, out_tbl);
    });
}

static void launch_expand_tf(wk_engine *e, const sid_t *cur_tbl,
                             sid_t *out_tbl, int G, const uint64_t *tbm) {
    with_ncols(e->ncols, [&](auto nc) {
        constexpr int NC = decltype(nc)::value;
        hipLaunchKernelGGL(k_expand_tf<NC>, dim3(grid_for(e->bound)),
                           dim3(BLOCK), 0, e->stream, cur_tbl, e->ncols,
                           e->d_edges, (uint64_t *)e->eoff.p,
                           (uint32_t *)e->cnt.p, (uint64_t *)e->prefix.p,
                           (uint64_t *)e->bsums.p, G, tbm, e->st->type_base,
                           e->st->type_n, e->d_state, (uint64_t)e->cap_rows,
                           e->d_stats, (uint32_t *)e->ovf.p, out_tbl);
        hipLaunchKernelGGL(k_expand_tf_big<NC>, dim3(512), dim3(BLOCK), 0,
                           e->stream, cur_tbl, e->ncols, e->d_edges,
                           (uint64_t *)e->eoff.p, (uint32_t *)e->cnt.p,
                           (uint64_t *)e->prefix.p, (uint64_t *)e->bsums.p, G,
                           tbm, e->st->type_base, e->st->type_n, e->d_state,
                           (uint64_t)e->cap_rows, (uint32_t *)e->ovf.p,
                           out_tbl);
    });
}
