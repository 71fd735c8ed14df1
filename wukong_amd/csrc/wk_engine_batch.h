// wk_engine_batch.h — the light-query paths: k_light2 eligibility, the batched
// light window and the LDS plan batch.
// Included by gpu_engine.hip only (one translation unit).
#pragma once

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
// not interpretable (caller uses the per-pattern path instead).  The
// interpreter runs the main patterns and nothing else, so whatever else
// a plan can carry is refused here, never dropped: DISTINCT, LIMIT,
// OFFSET, an OPTIONAL group, UNION branches (FILTER: the entry point).
static int32_t compile_light_plan(const wk_engine *e, const wk_plan_t *plan,
                                  lplan_t *lp) {
    if (!plan || plan->npatterns < 1 || plan->npatterns > 8) return WK_ERR_PLAN;
    if (plan->nvars < 1 || plan->nvars > 8) return WK_ERR_PLAN;
    if (plan->distinct || plan->limit >= 0 || plan->offset > 0)
        return WK_ERR_PLAN;
    if (plan->nopt > 0 || plan->nunion > 0) return WK_ERR_PLAN;
    const wk_store *st = e->st;
    int32_t v2c[8];
    for (int i = 0; i < 8; i++) v2c[i] = -1;

    const wk_pattern_t &p0 = plan->patterns[0];
    if (p0.subject < 0 || is_tpid(p0.subject) || p0.object >= 0 ||
        p0.predicate < 0)
        return WK_ERR_PLAN;  // must be const_to_unknown, fixed predicate
    if (-(p0.object + 1) >= plan->nvars) return WK_ERR_PLAN;
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
