// wk_engine_store.h — device store image: upload, destroy, xGMI peer export / import.
// Included by gpu_engine.hip only (one translation unit).
#pragma once

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
