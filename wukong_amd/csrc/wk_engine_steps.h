// wk_engine_steps.h — one step_* function per operator, exec_pattern, and the
// step API entry points.
// Included by gpu_engine.hip only (one translation unit).
#pragma once

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
    const int in_step = e->step;  // a fused step consumes TWO patterns
    // a zero-copy i2u/c2u input lives in the (immutable) store, not in
    // tbl[cur]: the step drops the view, the re-run must see it again
    const table_pos in_pos = save_pos(e);
    int32_t rc = exec_pattern(e);
    if (rc == WK_OK && nrows_out) {
        for (int attempt = 0; attempt < 6; attempt++) {
            rc = sync_state(e);
            if (rc != WK_ERR_CAP) break;
            // restore the input state; grow (preserving the INPUT table,
            // now current again); re-run this pattern
            int64_t need = (int64_t)e->h_pin[S_REQ];
            restore_pos(e, in_pos);
            e->nrows = in_rows;
            e->bound = in_rows;  // the synced count, not the input's bound
            e->step = in_step;
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
    scoped_set<int> remote(e->remote_step_idx, e->step);
    return wk_engine_execute_one_pattern(e, nrows_out);
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
