// wk_kernels_batch.h — fork-join split, light-query batch and xGMI peer-step kernels.
// Included by gpu_engine.hip only (one translation unit).
#pragma once

// fork-join split (generate_sub_query sparql.hpp:772-796): dst = vid % ndst
// Fork-join split as a radix partition (replaces the per-row
// global-cursor scatter: 6.4M rows over <=8 cursor words serialize at
// ~88 atomics/us per word ~= 9 ms; reference analog
// gpu_hash.cu:600-760).  Phase 1: per-block LDS histograms over
// contiguous chunks; phase 2: ONE block turns them into per-
// (block,dst) bases + per-dst totals; phase 3: scatter with LDS
// cursors only — no global atomics anywhere.
__global__ void k_dst_count(const sid_t *__restrict__ tbl, int64_t nrows,
                            int ncols, int col, int ndst,
                            unsigned long long *__restrict__ bh)
{
    __shared__ unsigned int lh[64];
    const int G = gridDim.x;
    const int64_t chunk = (nrows + G - 1) / G;
    const int64_t start = (int64_t)blockIdx.x * chunk;
    const int64_t end = min(start + chunk, nrows);
    if (threadIdx.x < 64) lh[threadIdx.x] = 0;
    __syncthreads();
    for (int64_t r = start + threadIdx.x; r < end; r += blockDim.x)
        atomicAdd(&lh[tbl[r * ncols + col] % (sid_t)ndst], 1u);
    __syncthreads();
    if (threadIdx.x < (unsigned)ndst)
        bh[(size_t)blockIdx.x * ndst + threadIdx.x] = lh[threadIdx.x];
}

__global__ void k_dst_scan2(unsigned long long *__restrict__ bh, int G,
                            int ndst, unsigned long long *__restrict__ hist)
{
    __shared__ unsigned long long tot[64];
    const int d = threadIdx.x;
    if (d < ndst) {
        unsigned long long run = 0;
        for (int b = 0; b < G; b++) {
            unsigned long long t = bh[(size_t)b * ndst + d];
            bh[(size_t)b * ndst + d] = run;
            run += t;
        }
        tot[d] = run;
        hist[d] = run;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long acc = 0;
        for (int i = 0; i < ndst; i++) {
            unsigned long long t = tot[i];
            tot[i] = acc;
            acc += t;
        }
    }
    __syncthreads();
    if (d < ndst)
        for (int b = 0; b < G; b++) bh[(size_t)b * ndst + d] += tot[d];
}

__global__ void k_dst_scatter2(const sid_t *__restrict__ tbl, int64_t nrows,
                               int ncols, int col, int ndst,
                               const unsigned long long *__restrict__ bh,
                               sid_t *__restrict__ out)
{
    __shared__ unsigned int lc[64];
    const int G = gridDim.x;
    const int64_t chunk = (nrows + G - 1) / G;
    const int64_t start = (int64_t)blockIdx.x * chunk;
    const int64_t end = min(start + chunk, nrows);
    if (threadIdx.x < 64) lc[threadIdx.x] = 0;
    __syncthreads();
    for (int64_t r = start + threadIdx.x; r < end; r += blockDim.x) {
        int d = (int)(tbl[r * ncols + col] % (sid_t)ndst);
        unsigned long long pos = bh[(size_t)blockIdx.x * ndst + d] +
                                 atomicAdd(&lc[d], 1u);
        sid_t *dst = out + pos * ncols;
        const sid_t *src = tbl + r * ncols;
        for (int c = 0; c < ncols; c++) dst[c] = src[c];
    }
}

// whole-query fast path for the dominant light-template shape
// (const_to_unknown + rdf:type constant filter — emulator A1/A2/A3/A5,
// proxy.hpp:391-545): ONE single-block kernel executes both patterns and
// publishes the row count straight to pinned memory.  Cuts ~20 dispatches
// to 1 (the launch rate, not the kernels, bounds light-query throughput).
__global__ void k_light2(const sid_t *__restrict__ edges, uint64_t list_off,
                         uint64_t sz, sid_t cval,
                         const uint16_t *__restrict__ type_of,
                         uint64_t type_base, uint64_t type_n,
                         uint64_t *__restrict__ d_state,
                         uint64_t *__restrict__ d_stats,
                         sid_t *__restrict__ out,
                         uint64_t *__restrict__ h_pin)
{
    __shared__ unsigned int cnt;
    if (threadIdx.x == 0) cnt = 0;
    __syncthreads();
    for (uint64_t i = threadIdx.x; i < sz; i += blockDim.x) {
        sid_t v = edges[list_off + i];
        const uint16_t t = type_of_dense(type_of, type_base, type_n, v);
        if ((sid_t)t == cval) {
            unsigned p = atomicAdd(&cnt, 1u);
            out[p] = v;
        }
        // multi-type entities (t==0xFFFF) would need the probe path; the
        // host only routes here when the store has no such entities
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        d_state[S_NROWS] = cnt;
        d_state[S_ERR] = 0;
        for (int i = 0; i < S_WORDS; i++) h_pin[i] = d_state[i];
        for (int i = 0; i < CAT_COUNT; i++) h_pin[HP_STATS + i] = d_stats[i];
        atomicAdd((unsigned long long *)&d_stats[CAT_FILTER],
                  (unsigned long long)(sz * 6 + cnt * 4));
    }
}

// batched light queries: ONE launch executes a whole window of
// light2-shaped queries (const_to_unknown + rdf:type filter), one
// wavefront-sized workgroup per query.  This is the engine-side answer
// to the reference proxy's in-flight window (proxy.hpp:477-525): at
// 1024 in-flight light queries the bottleneck is kernel DISPATCH rate
// (~10us/launch), so the scheduler packs the window into one grid.
struct light_desc {
    uint64_t off;      // edge-list offset of the c2u constant
    uint64_t sz;       // edge-list length
    uint64_t out_off;  // this query's region in the shared out buffer
    uint32_t cval;     // rdf:type filter constant
    uint32_t pad;
};

static const int LBLOCK = 64;  // one wavefront per query

__global__ void k_light_batch(const sid_t *__restrict__ edges,
                              const light_desc *__restrict__ descs,
                              const uint16_t *__restrict__ type_of,
                              uint64_t type_base, uint64_t type_n,
                              sid_t *__restrict__ out,
                              uint64_t *__restrict__ d_counts,
                              uint64_t *__restrict__ d_stats)
{
    const light_desc d = descs[blockIdx.x];
    __shared__ unsigned int cnt;
    if (threadIdx.x == 0) cnt = 0;
    __syncthreads();
    sid_t *qout = out + d.out_off;
    for (uint64_t i = threadIdx.x; i < d.sz; i += blockDim.x) {
        sid_t v = edges[d.off + i];
        const uint16_t t = type_of_dense(type_of, type_base, type_n, v);
        if ((sid_t)t == d.cval) {
            unsigned p = atomicAdd(&cnt, 1u);
            qout[p] = v;
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        d_counts[blockIdx.x] = cnt;
        atomicAdd((unsigned long long *)&d_stats[CAT_FILTER],
                  (unsigned long long)(d.sz * 6 + cnt * 4));
    }
}

// ---------------------------------------------------------------------
// batched whole-plan light queries: the LDS plan interpreter.
//
// The emulator's heavy templates (A4: 5 patterns, A6: 4 patterns,
// proxy.hpp:391-545) have tiny intermediate tables (tens-hundreds of
// rows) — per-pattern global kernels waste ~20 dispatches/query.  Here
// ONE launch runs a window of same-template queries; each wavefront-
// sized workgroup interprets the whole compiled plan with its binding
// table staged in LDS (ping-pong buffers), probing the cluster hash in
// global memory (64 independent probes in flight per wave).  A query
// whose table outgrows LDS publishes WK_LP_OVERFLOW and the host
// re-runs it on the general per-pattern path — results identical.
// ---------------------------------------------------------------------
enum { LOP_C2U = 0, LOP_TYPEOF, LOP_K2U, LOP_K2C, LOP_K2K };
struct lop_t {
    int32_t op, col, col2, dir;
    uint32_t cval, pid;
    uint64_t bucket_start, num_buckets;  // segment of (pid,dir)
};
struct lplan_t {
    lop_t ops[8];
    int32_t nops;
};
static const int LP_CAP = 6144;            // u32 slots per LDS buffer
static const uint64_t WK_LP_OVERFLOW = ~0ull;

__global__ void
__launch_bounds__(64)
k_plan_batch(const vertex_t *__restrict__ verts,
             const sid_t *__restrict__ edges, const lplan_t lp,
             const int64_t *__restrict__ consts,
             const uint16_t *__restrict__ type_of, uint64_t type_base,
             uint64_t type_n, uint64_t *__restrict__ d_counts,
             uint64_t *__restrict__ d_stats)
{
    __shared__ sid_t bufA[LP_CAP], bufB[LP_CAP];
    __shared__ unsigned s_n, s_cur, s_err;
    __shared__ uint64_t s_eoff, s_esz, s_bytes;
    sid_t *cur = bufA, *nxt = bufB;
    int nc = 0;
    uint64_t my_bytes = 0;
    if (threadIdx.x == 0) { s_n = 0; s_err = 0; s_bytes = 0; }
    __syncthreads();

    for (int o = 0; o < lp.nops && !s_err; o++) {
        const lop_t op = lp.ops[o];
        if (op.op == LOP_C2U) {
            if (threadIdx.x == 0) {
                uint64_t key = key_pack((uint64_t)consts[blockIdx.x],
                                        (uint64_t)op.pid, (uint64_t)op.dir);
                s_eoff = 0; s_esz = 0;
                if (op.num_buckets)
                    probe_one(verts, op.bucket_start, op.num_buckets, key,
                              s_eoff, s_esz);
                if (s_esz > (uint64_t)LP_CAP) s_err = 1;
                s_n = (unsigned)s_esz;
                my_bytes += 148;
            }
            __syncthreads();
            if (s_err) break;
            for (unsigned i = threadIdx.x; i < s_n; i += blockDim.x)
                cur[i] = edges[s_eoff + i];
            if (threadIdx.x == 0) my_bytes += (uint64_t)s_n * 8;
            nc = 1;
            __syncthreads();
        } else if (op.op == LOP_TYPEOF) {
            if (threadIdx.x == 0) s_cur = 0;
            __syncthreads();
            for (unsigned r = threadIdx.x; r < s_n; r += blockDim.x) {
                sid_t v = cur[r * nc + op.col];
                uint64_t idx = (uint64_t)v - type_base;
                uint16_t t = (idx < type_n) ? type_of[idx] : 0;
                my_bytes += 6;
                if ((sid_t)t == (sid_t)op.cval) {
                    unsigned p = atomicAdd(&s_cur, 1u);
                    for (int c = 0; c < nc; c++)
                        nxt[p * nc + c] = cur[r * nc + c];
                    my_bytes += (uint64_t)nc * 4;
                }
            }
            __syncthreads();
            if (threadIdx.x == 0) s_n = s_cur;
            sid_t *t_ = cur; cur = nxt; nxt = t_;
            __syncthreads();
        } else if (op.op == LOP_K2C || op.op == LOP_K2K) {
            if (threadIdx.x == 0) s_cur = 0;
            __syncthreads();
            for (unsigned r = threadIdx.x; r < s_n; r += blockDim.x) {
                sid_t v = cur[r * nc + op.col];
                uint64_t eoff = 0, esz = 0;
                uint64_t key = key_pack((uint64_t)v, (uint64_t)op.pid,
                                        (uint64_t)op.dir);
                if (op.num_buckets)
                    probe_one(verts, op.bucket_start, op.num_buckets, key,
                              eoff, esz);
                sid_t tgt = (op.op == LOP_K2C) ? (sid_t)op.cval
                                               : cur[r * nc + op.col2];
                my_bytes += 148 + 32;  // probe + ~log2 bsearch lines
                if (esz && bsearch_u32(edges + eoff, esz, tgt)) {
                    unsigned p = atomicAdd(&s_cur, 1u);
                    for (int c = 0; c < nc; c++)
                        nxt[p * nc + c] = cur[r * nc + c];
                    my_bytes += (uint64_t)nc * 4;
                }
            }
            __syncthreads();
            if (threadIdx.x == 0) s_n = s_cur;
            sid_t *t_ = cur; cur = nxt; nxt = t_;
            __syncthreads();
        } else {  // LOP_K2U
            if (threadIdx.x == 0) s_cur = 0;
            __syncthreads();
            for (unsigned r = threadIdx.x; r < s_n; r += blockDim.x) {
                sid_t v = cur[r * nc + op.col];
                uint64_t eoff = 0, esz = 0;
                uint64_t key = key_pack((uint64_t)v, (uint64_t)op.pid,
                                        (uint64_t)op.dir);
                if (op.num_buckets)
                    probe_one(verts, op.bucket_start, op.num_buckets, key,
                              eoff, esz);
                my_bytes += 148;
                unsigned base = atomicAdd(&s_cur, (unsigned)esz);
                if (((uint64_t)base + esz) * (nc + 1) > (uint64_t)LP_CAP) {
                    s_err = 1;
                    continue;
                }
                for (uint64_t e = 0; e < esz; e++) {
                    sid_t *dst = nxt + (base + e) * (nc + 1);
                    for (int c = 0; c < nc; c++) dst[c] = cur[r * nc + c];
                    dst[nc] = edges[eoff + e];
                }
                my_bytes += esz * (uint64_t)(nc + 1) * 4 + esz * 4;
            }
            __syncthreads();
            if (threadIdx.x == 0) s_n = s_cur;
            sid_t *t_ = cur; cur = nxt; nxt = t_;
            nc++;
            __syncthreads();
        }
    }
    __syncthreads();
    atomicAdd((unsigned long long *)&s_bytes, (unsigned long long)my_bytes);
    __syncthreads();
    if (threadIdx.x == 0) {
        d_counts[blockIdx.x] = s_err ? WK_LP_OVERFLOW : (uint64_t)s_n;
        atomicAdd((unsigned long long *)&d_stats[CAT_FILTER],
                  (unsigned long long)s_bytes);
    }
}

// ---------------------------------------------------------------------
// xGMI peer-probe small-table step — the reference's one-sided in-place
// remote read (gstore.hpp:260-338), gated by the fork-join threshold
// (need_fork_join, sparql.hpp:802-814, Global::rdma_threshold=300): a
// binding table below the threshold probes the OWNER rank's HBM store
// directly through HIP-IPC peer mappings over xGMI instead of shipping
// rows with an all-to-allv.  ONE workgroup — tables are tiny, so the
// block-local scan keeps compaction exact with zero global atomics.
struct wk_peer_desc {
    const vertex_t *verts;
    const sid_t *edges;
    const uint16_t *type_of;
    uint64_t type_base, type_n;
};
struct segtab8 { uint64_t bs[8]; uint64_t nb[8]; };  // per-rank (pid,dir) segment

__global__ void k_peer_step(const wk_peer_desc *__restrict__ peers, int nsrv,
                            segtab8 seg,
                            const sid_t *__restrict__ tbl, int ncols, int col,
                            uint32_t pid, int dir, int pmode, int col2,
                            sid_t cval, uint64_t cap,
                            uint64_t *__restrict__ d_state,
                            uint64_t *__restrict__ d_stats,
                            sid_t *__restrict__ out)
{
    const int64_t nrows = (int64_t)d_state[S_NROWS];
    count_bytes(d_stats, CAT_PROBE, (uint64_t)nrows * (4 + 128 + 8));
    const int oc = pmode == PM_SIZE ? ncols + 1 : ncols;
    uint64_t carry = 0;
    for (int64_t base = 0; base < nrows; base += SCAN_T) {
        const int64_t r = base + threadIdx.x;
        uint64_t deg = 0;  // rows to emit (expand: fanout; filter: 0/1)
        const sid_t *el = nullptr;
        if (r < nrows) {
            sid_t v = tbl[r * ncols + col];
            int owner = (int)(v % (sid_t)nsrv);
            const wk_peer_desc P = peers[owner];
            bool resolved = false;
            // `?v rdf:type CONST` via the owner's dense side index;
            // multi-type (0xFFFF) falls through to the owner probe of
            // the same [v|TYPE|OUT] segment
            if (pmode == PM_CONST && pid == TYPE_ID && dir == DIR_OUT &&
                P.type_of) {
                const int tc = typeof_check(nullptr, P.type_of, P.type_base,
                                            P.type_n, cval, v);
                deg = tc == TC_YES ? 1 : 0;
                resolved = tc != TC_MULTI;
            }
            if (!resolved && seg.nb[owner]) {
                uint64_t eoff = 0, esz = 0;
                probe_one(P.verts, seg.bs[owner], seg.nb[owner],
                          key_pack(v, pid, (uint64_t)dir), eoff, esz);
                if (pmode == PM_SIZE) {
                    deg = esz;
                    el = P.edges + eoff;
                } else if (esz) {
                    sid_t tgt = pmode == PM_CONST ? cval
                                                  : tbl[r * ncols + col2];
                    deg = bsearch_u32(P.edges + eoff, esz, tgt) ? 1 : 0;
                }
            }
        }
        uint64_t total;
        const uint64_t pos = carry + block_ladder_scan(deg, &total) - deg;
        carry += total;
        if (r < nrows && deg) {
            if (pmode == PM_SIZE) {
                for (uint64_t k = 0; k < deg; k++) {
                    uint64_t dst = pos + k;
                    if (dst >= cap) break;
                    sid_t *d = out + dst * oc;
                    for (int c = 0; c < ncols; c++) d[c] = tbl[r * ncols + c];
                    d[ncols] = el[k];
                }
            } else if (pos < cap) {
                sid_t *d = out + pos * oc;
                for (int c = 0; c < ncols; c++) d[c] = tbl[r * ncols + c];
            }
        }
        __syncthreads();
    }
    if (threadIdx.x == 0)  // single block: commit inline, as k_commit would
        commit_rows(d_state, carry, cap, /*snapshot_inrows*/ false);
}
