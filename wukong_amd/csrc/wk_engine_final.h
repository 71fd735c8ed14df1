// wk_engine_final.h — result download, host and device final ops (DISTINCT,
// OFFSET, LIMIT, projection) and the fetch entry points.
// Included by gpu_engine.hip only (one translation unit).
#pragma once

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
