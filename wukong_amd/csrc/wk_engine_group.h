// wk_engine_group.h — UNION branches and the OPTIONAL group: as part of the
// asynchronous launch chain (run_union_dev, run_optional)
// and, under WK_DEV_GROUPS=0, with the host merge and the per-pattern syncs
// of wk_engine_run_query (run_union_host).
// Included by gpu_engine.hip only (one translation unit).
#pragma once

static bool plan_has_groups(const wk_plan_t *plan) {
    return (plan->nunion > 0 && plan->union_pats && plan->union_sizes) ||
           (plan->nopt > 0 && plan->opt_patterns);
}

// Before the first launch of a group plan: everything the groups need that
// could allocate.  Nothing here runs mid-chain, where grow_caps would have
// to save a table whose row count the host does not know, and a grown
// snapshot buffer would lose the parent; inside a capture all of it is a
// no-op, because the warm pass ran the same code (WK_ERR_STATE otherwise).
//  - a UNION branch may open with a constant or index start, whose
//    step_start sizes the capacity to its list: do that now
//  - the snapshot and merged buffers of the UNION
//  - the matched flags of the OPTIONAL group
static int32_t prepare_groups(wk_engine *e, const wk_plan_t *plan) {
    if (plan->nunion > 0 && plan->union_pats && plan->union_sizes) {
        uint64_t need = 0;
        const wk_pattern_t *bp = plan->union_pats;
        for (int b = 0; b < plan->nunion; b++) {
            for (int k = 0; k < plan->union_sizes[b]; k++) {
                const wk_pattern_t &pt = bp[k];
                if (pt.subject < 0 || pt.predicate < 0 || pt.object >= 0)
                    continue;
                uint64_t sz = 0;
                if (k == 0 && is_tpid(pt.subject))
                    (void)store_get(*e->st, 0, (uint64_t)pt.subject,
                                    pt.direction, &sz);
                else
                    (void)store_get(*e->st, (uint64_t)pt.subject,
                                    (uint64_t)pt.predicate, pt.direction, &sz);
                need = std::max(need, sz);
            }
            bp += plan->union_sizes[b];
        }
        int32_t rc = grow_caps(e, (int64_t)need, e->nvars);
        if (rc) return rc;
        const size_t bytes = (size_t)e->cap_rows * e->cap_cols * 4;
        if (e->capturing && (e->gsnap.cap < bytes || e->gmerge.cap < bytes))
            return WK_ERR_STATE;
        if (e->gsnap.ensure(bytes) || e->gmerge.ensure(bytes))
            return WK_ERR_HIP;
        e->grp_bufs = true;
    }
    if (plan->nopt > 0 && plan->opt_patterns) {
        const size_t bytes = (size_t)e->cap_rows;
        if (e->capturing && (e->oflag[0].cap < bytes || e->oflag[1].cap < bytes))
            return WK_ERR_STATE;
        if (e->oflag[0].ensure(bytes) || e->oflag[1].ensure(bytes))
            return WK_ERR_HIP;
    }
    return WK_OK;
}

// Grid of the group copies: one lane per GRP_UNROLL 16-B chunks of the
// host-known bound, never a value read back.
static int grp_grid(int64_t rows, int ncols) {
    return grid_for((rows * std::max(ncols, 1) + 4 * GRP_UNROLL - 1) /
                    (4 * GRP_UNROLL));
}

// UNION branches (sparql.hpp:1593-1614 + rmap.hpp:57-87) on the device:
// each branch continues from the main group's result table and the final
// table is the row-concat of the branch results, in branch order.  All
// branches must end with the same variable->column layout.
//
// No host round trip: k_grp_copy snapshots the parent (the first branch's
// ping-pong overwrites its buffer) and records its row count; a later
// branch restarts from the snapshot, which it reads IN PLACE as a table
// view (every reader goes through cur_table and every in-place writer
// materialises a view first), or from the store when the parent itself was
// a view into it; k_grp_append adds a finished branch to the merged buffer
// and the 1-thread k_grp_restart moves the device counts.  The merged
// table ends in tbl[0] by a last k_grp_copy: captured graphs bake buffer
// addresses and restore only `cur`, so the engine never swaps buffers.
static int32_t run_union_dev(wk_engine *e, const wk_plan_t *plan) {
    const size_t bytes = (size_t)e->cap_rows * e->cap_cols * 4;
    if (e->gsnap.cap < bytes || e->gmerge.cap < bytes)
        return WK_ERR_STATE;  // prepare_groups sized them for this capacity
    flush_begin(e);
    const table_pos parent = save_pos(e);
    const int pc = parent.ncols;
    const int64_t cap0 = e->cap_rows;
    const sid_t *restart_from =
        parent.view ? parent.view : (const sid_t *)e->gsnap.p;
    {
        TIME_BEGIN(e);
        // a parent that is a view into the (immutable) store needs no copy
        hipLaunchKernelGGL(k_grp_copy, dim3(grp_grid(parent.bound, pc)),
                           dim3(BLOCK), 0, e->stream, cur_table(e),
                           parent.view ? nullptr : (sid_t *)e->gsnap.p, pc,
                           (uint64_t)e->cap_rows, 1, e->d_state, e->d_grp,
                           e->d_stats);
        TIME_END(e, CAT_COPY);
    }
    scoped_set<bool> in_group(e->in_group, true);
    std::vector<int32_t> bv2c;
    int bc = -1;
    int64_t mbound = 0;
    const wk_pattern_t *bp = plan->union_pats;
    for (int b = 0; b < plan->nunion; b++) {
        if (b) {  // the parent again; k_grp_restart set its row count
            restore_pos(e, parent);
            e->tbl_view = (pc && parent.bound) ? restart_from : nullptr;
            fin_invalidate(e);
        }
        e->pats.assign(bp, bp + plan->union_sizes[b]);
        e->step = 0;
        bp += plan->union_sizes[b];
        while (e->step < (int)e->pats.size()) {
            int32_t rc = exec_pattern(e);
            if (rc) return rc;
        }
        // a start step that outgrew the capacity mid-chain would have
        // moved the buffers under the snapshot
        if (e->cap_rows != cap0) return WK_ERR_STATE;
        if (bc < 0) {
            bc = e->ncols;
            bv2c = e->v2c;
        } else if (bc != e->ncols || bv2c != e->v2c) {
            return WK_ERR_PLAN;
        }
        mbound = std::min<int64_t>(e->cap_rows, mbound + e->bound);
        TIME_BEGIN(e);
        hipLaunchKernelGGL(k_grp_append, dim3(grp_grid(e->bound, bc)),
                           dim3(BLOCK), 0, e->stream, cur_table(e),
                           (sid_t *)e->gmerge.p, bc, (uint64_t)e->cap_rows,
                           e->d_state, e->d_grp, e->d_stats);
        hipLaunchKernelGGL(k_grp_restart, dim3(1), dim3(1), 0, e->stream,
                           e->d_state, e->d_grp, (uint64_t)e->cap_rows,
                           b + 1 == plan->nunion ? 1 : 0);
        TIME_END(e, CAT_COPY);
    }
    // the merged table becomes the current one, in tbl[0]
    e->cur = 0;
    e->tbl_view = nullptr;
    e->bound = mbound;
    e->nrows = 0;  // unknown until the next sync
    fin_invalidate(e);
    TIME_BEGIN(e);
    hipLaunchKernelGGL(k_grp_copy, dim3(grp_grid(mbound, bc)), dim3(BLOCK), 0,
                       e->stream, (const sid_t *)e->gmerge.p,
                       (sid_t *)e->tbl[0].p, bc, (uint64_t)e->cap_rows, 0,
                       e->d_state, e->d_grp, e->d_stats);
    TIME_END(e, CAT_COPY);
    return WK_OK;
}

// The same UNION with the host merge (WK_DEV_GROUPS=0): a sync and a
// download per branch, the concatenation in host memory, one upload.
static int32_t run_union_host(wk_engine *e, const wk_plan_t *plan) {
    int32_t rc = sync_state(e);
    if (rc) return rc;
    const int64_t pr = e->nrows;  // == bound: sync_state just set both
    const table_pos parent = save_pos(e);
    const int pc = parent.ncols;
    devbuf snap;  // freed by its destructor on every way out
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
            restore_pos(e, parent);
            e->tbl_view = nullptr;  // snap restore materialises the view
            if (bytes && pc)
                HIP_CHECK(hipMemcpyAsync(e->tbl[parent.cur].p, snap.p, bytes,
                                         hipMemcpyDeviceToDevice, e->stream));
            hipLaunchKernelGGL(k_set_state, dim3(1), dim3(1), 0, e->stream,
                               e->d_state, (uint64_t)pr);
            e->nrows = pr;
        }
        e->pats.assign(bp, bp + plan->union_sizes[b]);
        e->step = 0;
        bp += plan->union_sizes[b];
        while (e->step < (int)e->pats.size()) {
            rc = exec_pattern(e);
            if (rc) return rc;
        }
        rc = sync_state_grow(e);
        if (rc) return rc;
        if (bc < 0) {
            bc = e->ncols;
            bv2c = e->v2c;
        } else if (bc != e->ncols || bv2c != e->v2c) {
            return WK_ERR_PLAN;
        }
        size_t off = merged.size();
        merged.resize(off + (size_t)e->nrows * bc);
        if (e->nrows)
            HIP_CHECK(hipMemcpy(merged.data() + off, cur_table(e),
                                (size_t)e->nrows * bc * 4,
                                hipMemcpyDeviceToHost));
    }
    int64_t mrows = bc > 0 ? (int64_t)(merged.size() / bc) : 0;
    rc = wk_engine_load_rbuf(e, merged.empty() ? nullptr : merged.data(),
                             mrows, bc, bv2c.data(), 0);
    if (rc) return rc;
    HIP_CHECK(stream_sync(e->stream));  // merged[] is about to go away
    return WK_OK;
}

// OPTIONAL pattern group (sparql.hpp:1616-1649, BGP-only): rows are
// kept; unmatched rows carry BLANK_ID in the columns first bound inside
// the group.  k_expand_opt and k_filter_opt take their row counts from
// d_state and clamp to cap_rows, so the group is a plain stretch of the
// launch chain; host_sync (WK_DEV_GROUPS=0) keeps a sync ahead of the
// group and behind every pattern.
static int32_t run_optional(wk_engine *e, const wk_plan_t *plan,
                            bool host_sync) {
    int32_t rc = WK_OK;
    if (host_sync) {
        rc = sync_state(e);
        if (rc) return rc;
    } else {
        flush_begin(e);
        if (e->capturing && (e->oflag[0].cap < (size_t)e->cap_rows ||
                             e->oflag[1].cap < (size_t)e->cap_rows))
            return WK_ERR_STATE;  // no allocation inside a capture
    }
    if (e->oflag[0].ensure((size_t)e->cap_rows) ||
        e->oflag[1].ensure((size_t)e->cap_rows))
        return WK_ERR_HIP;
    HIP_CHECK(hipMemsetAsync(e->oflag[0].p, 1, (size_t)e->cap_rows,
                             e->stream));
    HIP_CHECK(hipMemsetAsync(e->oflag[1].p, 1, (size_t)e->cap_rows,
                             e->stream));
    scoped_set<int> opt_mode(e->opt_mode, 1);
    scoped_set<bool> in_group(e->in_group, true);
    e->ocur = 0;
    e->opt_mask = 0;
    e->pats.assign(plan->opt_patterns, plan->opt_patterns + plan->nopt);
    e->step = 0;
    while (e->step < (int)e->pats.size()) {
        rc = exec_pattern(e);
        if (!rc && host_sync) rc = sync_state_grow(e);
        if (rc) return rc;
    }
    return WK_OK;
}
