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
 * Inventory.  Device code lives in the wk_kernels_*.h headers and host
 * code in the wk_engine_*.h headers, all included below in a fixed order:
 * still one translation unit, so `static` linkage and the build line are
 * those of a single file:
 *  wk_kernels_common.h
 *   probe_one/probe_chain, bsearch_u32, tbm_has, csr_entry,
 *   type_of_dense, typeof_check, typeof_nodrop_ok — lookup helpers;
 *   d_state words and categories, commit_rows and begin_state — what one
 *   thread writes at a step's end / a query's begin; tile_compact — the
 *   ballot-rank compaction of the one-pass filters and k_row_chain;
 *   chain_eval (row-major, early exit) and chain_eval_batch (op-major,
 *   K candidates of compile-time width W, no early exit) — the per-row
 *   op chain evaluators
 *  wk_kernels_state.h
 *   k_commit, k_set_state, k_begin_state, k_zero_words,
 *   k_publish_state, k_publish_begin, k_project — 1-thread state
 *                       kernels, projection.
 *                       A query's begin zeroing rides on its first state
 *                       write (k_begin_state); the optimistic kernels
 *                       count guard misses into the sticky S_DONE word,
 *                       which k_publish_state alone turns into S_ERR —
 *                       no per-step commit for steps that keep the row
 *                       count
 *  wk_kernels_scan.h
 *   wave_incl_scan, block_excl_scan, block_ladder_scan — scan helpers;
 *   scan_pos, ovf_push, wave_emit_rows — what the writers behind the
 *   scan share
 *   k_scan_local/mid  — chunked exclusive scan with DEVICE-side length
 *                       (replaces the thrust scans, gpu_hash.cu:587-596):
 *                       several elements per thread, wave scan, one
 *                       barrier per tile; k_scan_mid also commits the
 *                       step (S_INROWS snapshot for the scatter side);
 *                       k_scan_*_ladder are their WK_SCAN=0 siblings
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
 *   k_expand_in/big   — input-centric expansion + wave-per-big-row pass
 *                       (replaces gpu_hash.cu:762-834; no 20-col cap),
 *                       optional inline no-drop typeof verify in graphs
 *   k_fn_gather/k_fn_scatter — functional-predicate rank-compressed
 *                       map k2u (deg==1 segments; page+value gathers);
 *                       k_expand_fn_map = optimistic 1:1 inside graphs
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
 *  wk_kernels_group.h
 *   k_grp_copy/append/restart — UNION on the device: parent snapshot,
 *                       branch append (16 B per lane, clamped to the
 *                       capacity) and the 1-thread restart between
 *                       branches (replaces the host merge of the branch
 *                       tables, rmap.hpp:57-87)
 *  host side (the wk_engine_*.h headers, included below in dependency
 *  order; the first lines of each say what it holds: core, store, launch,
 *  steps, filter, final, batch, graph, group).  This file keeps engine
 *  create / destroy, begin_query, run_plan (main BGP, UNION, OPTIONAL,
 *  trailing FILTER: one chain), wk_engine_submit, wk_engine_run_query and
 *  the small utility exports.
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

using namespace wk;

#include "wk_kernels_common.h"
#include "wk_kernels_state.h"
#include "wk_kernels_scan.h"
#include "wk_kernels_expand.h"
#include "wk_kernels_filter.h"
#include "wk_kernels_batch.h"
#include "wk_kernels_final.h"
#include "wk_kernels_group.h"

#include "wk_engine_core.h"
#include "wk_engine_store.h"
#include "wk_engine_launch.h"
#include "wk_engine_steps.h"
#include "wk_engine_filter.h"
#include "wk_engine_final.h"
#include "wk_engine_batch.h"
#include "wk_engine_graph.h"
#include "wk_engine_group.h"

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
    const size_t state_bytes = (S_WORDS + CAT_COUNT + 2 + G_WORDS) * 8;
    if (hipMalloc(&e->d_state, state_bytes) != hipSuccess ||
        hipHostMalloc(&e->h_pin, 64 * sizeof(uint64_t)) != hipSuccess) {
        wk_engine_destroy(e);
        return nullptr;
    }
    e->d_stats = e->d_state + S_WORDS;
    e->d_grp = e->d_state + S_WORDS + CAT_COUNT + 2;
    if (hipMalloc(&e->d_fin, F_WORDS * 8) != hipSuccess ||
        hipMemset(e->d_fin, 0, F_WORDS * 8) != hipSuccess ||
        hipMemset(e->d_state, 0, state_bytes) != hipSuccess) {
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
    e->gsnap.release(); e->gmerge.release();
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

// The main pattern list from the current step to its end, as a WHOLE
// plan: op chains may span patterns (whole_plan is set for exactly this
// scope, whatever path leaves it).
static int32_t run_whole_plan(wk_engine *e) {
    scoped_set<bool> whole_plan(e->whole_plan, true);
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

// The whole plan as one launch chain, with no host sync anywhere: main BGP,
// then UNION, then OPTIONAL (the reference's order, execute_sparql_query,
// sparql.hpp:1564-1662), then the FILTER conjuncts on UNION-/OPTIONAL-born
// variables (its stage 4, sparql.hpp:1651-1655).  Shared by
// wk_engine_submit (captures included) and wk_engine_run_query.
static int32_t run_plan(wk_engine *e, const wk_plan_t *plan) {
    int32_t rc = plan_has_groups(plan) ? prepare_groups(e, plan) : WK_OK;
    if (rc) return rc;
    rc = run_whole_plan(e);
    if (rc) return rc;
    if (plan->nunion > 0 && plan->union_pats && plan->union_sizes) {
        rc = run_union_dev(e, plan);
        if (rc) return rc;
    }
    if (plan->nopt > 0 && plan->opt_patterns) {
        rc = run_optional(e, plan, /*host_sync*/ false);
        if (rc) return rc;
    }
    if (!e->conj.empty()) rc = apply_filters(e, -1, -1, nullptr);
    return rc;
}

// WK_DEV_GROUPS=0: the groups with their host round trips (run_query only)
static int32_t run_plan_host_groups(wk_engine *e, const wk_plan_t *plan) {
    int32_t rc = run_whole_plan(e);
    if (rc) return rc;
    if (plan->nunion > 0 && plan->union_pats && plan->union_sizes) {
        rc = run_union_host(e, plan);
        if (rc) return rc;
    }
    if (plan->nopt > 0 && plan->opt_patterns) {
        rc = run_optional(e, plan, /*host_sync*/ true);
        if (rc) return rc;
    }
    if (!e->conj.empty()) rc = apply_filters(e, -1, -1, nullptr);
    return rc;
}

// asynchronous whole-plan submission: enqueue the full launch chain and
// return without any sync (pipelined multi-engine execution — the
// reference proxy's in-flight window, proxy.hpp:477-525)
extern "C" int32_t wk_engine_submit(wk_engine_t *e, const wk_plan_t *plan) {
    if (!e || !plan) return WK_ERR_STATE;
    const bool groups = plan->nopt > 0 || plan->nunion > 0;
    if (groups && !wk_dev_groups())
        return WK_ERR_PLAN;  // the host-merge path is run_query's alone
    const bool light = !groups && light2_eligible(e, plan);
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
    return run_plan(e, plan);
}

extern "C" int32_t wk_engine_run_query(wk_engine_t *e, const wk_plan_t *plan,
                                       wk_result_t *out) {
    for (int attempt = 0; attempt < 6; attempt++) {
        int32_t rc = wk_engine_begin_query(e, plan);
        if (rc) return rc;
        rc = wk_dev_groups() ? run_plan(e, plan) : run_plan_host_groups(e, plan);
        if (rc == WK_ERR_CAP) continue;  // a host-merge sync saw the overflow
        if (rc) return rc;
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
