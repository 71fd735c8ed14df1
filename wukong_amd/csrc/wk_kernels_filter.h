// wk_kernels_filter.h — filter, VERSATILE and OPTIONAL kernels.
// Included by gpu_engine.hip only (one translation unit).
#pragma once

// Filter predicate (k2c/k2k/c2k/i2k keep-row decision of the one-pass
// filter k_filter_tpr below).
struct fparams {
    const vertex_t *verts;
    const sid_t *edges;
    uint64_t bucket_start, num_buckets;
    const sid_t *tbl;
    int ncols, col;
    uint32_t pid;
    int dir, key_mode, probe_mode, col2;
    sid_t cval;
    uint64_t list_off, list_sz;
    const uint16_t *type_of;
    uint64_t type_base, type_n;
    int use_typeof;
    const uint64_t *tbm;
    const fnpage_t *fn_pg;
    const sid_t *fn_vals;
    uint64_t fn_base, fn_n;
    int fn_swap;
};

__device__ __forceinline__ bool filter_keep(const fparams &P, int64_t r) {
    sid_t v = P.tbl[r * P.ncols + P.col];
    if (P.use_typeof) {
        // per-type bitmap (1 bit/vid, whole map LLC-resident, exact) or
        // the dense index; multi-type falls through to the probe
        const int tc = typeof_check(P.tbm, P.type_of, P.type_base, P.type_n,
                                    P.cval, v);
        if (tc != TC_MULTI) return tc == TC_YES;
    }
    if (P.probe_mode == PM_EQ) {
        // reversed functional map resolved host-side: the edge exists
        // iff the row value IS the precomputed vertex
        return v == P.cval;
    }
    if (P.probe_mode == PM_LIST && !P.use_typeof)
        return bsearch_u32(P.edges + P.list_off, P.list_sz, v);
    if (P.fn_pg) {
        // functional predicate: the row's single object replaces the
        // probe + edge-list search (rank-compressed map: 16-B page +
        // 4-B value vs 148 bytes of hash traffic).  fn_swap: the
        // REVERSED direction is functional — check fn[other col] == col.
        sid_t a = v, b;
        if (P.probe_mode == PM_CONST) b = P.cval;
        else b = P.tbl[r * P.ncols + P.col2];
        if (P.fn_swap) { sid_t t_ = a; a = b; b = t_; }
        sid_t tv = fn_lookup(P.fn_pg, P.fn_vals, P.fn_base, P.fn_n, a);
        return tv && tv == b;
    }
    uint64_t key = (P.key_mode == PK_NORMAL)
                       ? key_pack(v, P.pid, (uint64_t)P.dir)
                       : key_pack(0, v, (uint64_t)P.dir);
    uint64_t eoff = 0, esz = 0;
    probe_one(P.verts, P.bucket_start, P.num_buckets, key, eoff, esz);
    sid_t tgt = (P.probe_mode == PM_CONST) ? P.cval
                                           : P.tbl[r * P.ncols + P.col2];
    return esz && bsearch_u32(P.edges + eoff, esz, tgt);
}

// The keep paths of filter_keep that are plain gathers, which
// filter_keep_batch evaluates op-major; FB_NONE = per-row filter_keep
// (dense type_of with its 0xFFFF probe fallback, PM_LIST, the cluster-hash
// probe, and any map or bitmap with an empty span, where index 0 may not
// exist).  Same order of tests as filter_keep.
enum { FB_NONE = 0, FB_TBM = 1, FB_EQ = 2, FB_FN = 3 };
__device__ __forceinline__ int filter_batch_mode(const fparams &P) {
    if (P.use_typeof) return (P.tbm && P.type_n) ? FB_TBM : FB_NONE;
    if (P.probe_mode == PM_EQ) return FB_EQ;
    if (P.probe_mode == PM_LIST) return FB_NONE;
    return (P.fn_pg && P.fn_vals && P.fn_n) ? FB_FN : FB_NONE;
}

// filter_keep on the tile's K rows at once, op-major like chain_eval_batch
// (DESIGN.md §3 item 3): all row values (and col2 values), then all bitmap
// words or map pages, then all map values, each level's K loads issued
// before any is consumed.  rr[] are VALID rows (a row past the end is
// clamped by the caller and has its bit clear in `in`); a row whose value
// is outside the span reads index 0 and is dropped.  Bit k of the result =
// filter_keep(P, rr[k]) for the rows of `in`.  `mode` is wave-uniform.
template <int K>
__device__ __forceinline__ uint32_t filter_keep_batch(const fparams &P,
                                                      int mode,
                                                      const int64_t (&rr)[K],
                                                      uint32_t in) {
    uint32_t keep = in;
    sid_t v[K];
#pragma unroll
    for (int j = 0; j < K; j++) v[j] = P.tbl[rr[j] * P.ncols + P.col];
    if (mode == FB_TBM) {
        uint64_t ix[K], w[K];
#pragma unroll
        for (int j = 0; j < K; j++) {
            const uint64_t x = (uint64_t)v[j] - P.type_base;
            const bool ok = x < P.type_n;
            keep = ok ? keep : keep & ~(1u << j);
            ix[j] = ok ? x : 0;
        }
#pragma unroll
        for (int j = 0; j < K; j++) w[j] = P.tbm[ix[j] >> 6];
#pragma unroll
        for (int j = 0; j < K; j++)
            keep = ((w[j] >> (ix[j] & 63)) & 1) ? keep : keep & ~(1u << j);
    } else if (mode == FB_EQ) {
#pragma unroll
        for (int j = 0; j < K; j++)
            keep = (v[j] == P.cval) ? keep : keep & ~(1u << j);
    } else {  // FB_FN: fn[a] != 0 && fn[a] == b
        sid_t b[K];
        if (P.probe_mode == PM_CONST) {
#pragma unroll
            for (int j = 0; j < K; j++) b[j] = P.cval;
        } else {
#pragma unroll
            for (int j = 0; j < K; j++)
                b[j] = P.tbl[rr[j] * P.ncols + P.col2];
        }
        uint64_t ix[K], bits[K];
        uint32_t rk[K];
        sid_t tv[K];
#pragma unroll
        for (int j = 0; j < K; j++) {
            // fn_swap: the REVERSED direction is functional
            const sid_t a = P.fn_swap ? b[j] : v[j];
            b[j] = P.fn_swap ? v[j] : b[j];
            const uint64_t x = (uint64_t)a - P.fn_base;
            const bool ok = x < P.fn_n;
            keep = ok ? keep : keep & ~(1u << j);
            ix[j] = ok ? x : 0;
        }
#pragma unroll
        for (int j = 0; j < K; j++) {  // one 16-B load per page
            const uint4 q =
                *reinterpret_cast<const uint4 *>(&P.fn_pg[ix[j] >> 6]);
            bits[j] = (uint64_t)q.x | ((uint64_t)q.y << 32);
            rk[j] = q.z;
        }
#pragma unroll
        for (int j = 0; j < K; j++) {
            const uint64_t bit = 1ull << (ix[j] & 63);
            const bool hit = ((keep >> j) & 1) && (bits[j] & bit);
            keep = hit ? keep : keep & ~(1u << j);
            // AND mask, not a select: a select lets the optimiser sink the
            // rank word's load into the `hit` branch, behind its own wait
            rk[j] = (rk[j] + (uint32_t)__popcll(bits[j] & (bit - 1))) &
                    (0u - (uint32_t)hit);
        }
#pragma unroll
        for (int j = 0; j < K; j++) tv[j] = P.fn_vals[rk[j]];
#pragma unroll
        for (int j = 0; j < K; j++)
            keep = (tv[j] && tv[j] == b[j]) ? keep : keep & ~(1u << j);
    }
    return keep;
}

__device__ __forceinline__ uint64_t filter_bytes_per_row(const fparams &P) {
    return (P.use_typeof ? 6
            : P.fn_pg ? 24
            : P.probe_mode == PM_LIST ? 12
                                      : (4 + 128 + 8 + 64)) +
           8 * P.ncols;
}

// One-pass filter: keep + wavefront-ballot compaction.  Each tile
// costs ONE global cursor atomic per block — a single word saturates
// at ~88 atomics/us (microarch row `dequeue`), so ~2048 in-flight
// blocks serialize ~23 us per tile ROUND; fine up to ~1-2M rows.
// (A flags+scan+scatter pipeline was tried for larger tables and
// measured SLOWER at suite keep-rates — extra passes cost more than
// the atomics they save.)  Row order is engine-internal; parity is
// set-level (sparql.hpp:455-476 semantics).
// `batch`: evaluate the tile's K rows op-major (filter_keep_batch) on the
// paths that are plain gathers; 0 (WK_FILTER_BATCH=0) or any other path:
// row after row through filter_keep.
__global__ void k_filter_tpr(fparams P, int verify_only, int batch,
                             uint64_t *__restrict__ d_state,
                             uint64_t *__restrict__ d_stats,
                             sid_t *__restrict__ out_tbl)
{
    const int64_t nrows = (int64_t)d_state[S_NROWS];
    count_bytes(d_stats, CAT_FILTER, (uint64_t)nrows * filter_bytes_per_row(P));
    constexpr int K = 4;
    const int lane = threadIdx.x & 63;
    const int ncols = P.ncols;
    const sid_t *__restrict__ tbl = P.tbl;
    const int64_t tile = (int64_t)blockDim.x * K;
    const int64_t stride = (int64_t)gridDim.x * tile;
    const int mode = batch ? filter_batch_mode(P) : FB_NONE;  // wave-uniform

    for (int64_t base = (int64_t)blockIdx.x * tile; base < nrows; base += stride) {
        uint32_t keep = 0;  // bit k: the thread's k-th row survives
        int64_t rr[K];
        if (mode != FB_NONE) {
            uint32_t in = 0;
#pragma unroll
            for (int k = 0; k < K; k++) {
                const int64_t r = base + k * SCAN_T + threadIdx.x;
                in |= r < nrows ? 1u << k : 0u;
                rr[k] = r < nrows ? r : base;  // base < nrows: a valid row
            }
            keep = filter_keep_batch<K>(P, mode, rr, in);
            // a clamped row is never kept; past nrows for verify_only
#pragma unroll
            for (int k = 0; k < K; k++)
                rr[k] = ((in >> k) & 1) ? rr[k] : nrows;
        } else {
#pragma unroll
            for (int k = 0; k < K; k++) {
                const int64_t r = base + k * SCAN_T + threadIdx.x;
                rr[k] = r;
                keep |= (r < nrows && filter_keep(P, r)) ? 1u << k : 0u;
            }
        }
        if (verify_only) {
            // identity-verified filter (captured graphs): the warm pass
            // saw zero drops; every replay still checks every row and
            // counts misses into the sticky S_DONE word (-> S_ERR at
            // the publish; no writes, no table flip, no commit)
            uint32_t miss = 0;
#pragma unroll
            for (int k = 0; k < K; k++)
                miss += (rr[k] < nrows && !((keep >> k) & 1)) ? 1u : 0u;
            if (miss)
                atomicAdd((unsigned long long *)&d_state[S_DONE],
                          (unsigned long long)miss);
            continue;
        }
        // output <= input rows: no position can pass the capacity
        uint64_t mask[K];
        uint64_t wpos = tile_compact<K>(keep, d_state, mask);
#pragma unroll
        for (int k = 0; k < K; k++) {
            if ((keep >> k) & 1) {
                const uint64_t pos = wpos + lanes_below(mask[k], lane);
                sid_t *dst = out_tbl + (int64_t)pos * ncols;
                const sid_t *srow = tbl + rr[k] * ncols;
                for (int c = 0; c < ncols; c++) dst[c] = srow[c];
            }
            wpos += (uint32_t)__popcll(mask[k]);
        }
    }
}

// ---------------------------------------------------------------------
// FILTER expressions (execute_filter, sparql.hpp:
// 1362-1382): the ID-exact subset =, !=, bound, &&, ||, ! as a postfix
// program over the row's columns.  The host (gpu_engine.hip) has
// validated the program and resolved every variable to its column: an
// operand is a column (ca/cb >= 0) or a constant (va/vb).  Ids compare
// verbatim, BLANK_ID included.
// ---------------------------------------------------------------------
struct fnode_d {
    int32_t op;      // WK_F_*
    int32_t ca, cb;  // operand columns, -1 = constant
    sid_t va, vb;    // constant operands
};
struct fprog_t {
    fnode_d node[WK_FILTER_MAX];
    const sid_t *tbl;
    int32_t n, ncols;
    uint32_t bytes_per_row;  // 4 * distinct operand columns + 8 * ncols
};

// The tile and compaction of k_filter_tpr (tile_compact, 5g(ii)); the
// keep decision is the program.  The program sits in the kernel-argument
// segment and is walked with a wave-uniform index; the evaluation stack
// of each of the thread's K rows is a bit-stack in one 32-bit register
// (a valid program of <= 32 nodes never holds more than 16 values), and
// operands come straight from the table — no runtime-indexed local
// array, no scratch.
__global__ void k_filter_expr(fprog_t P, uint64_t *__restrict__ d_state,
                              uint64_t *__restrict__ d_stats,
                              sid_t *__restrict__ out_tbl)
{
    const int64_t nrows = (int64_t)d_state[S_NROWS];
    count_bytes(d_stats, CAT_FILTER, (uint64_t)nrows * P.bytes_per_row);
    constexpr int K = 4;
    const int lane = threadIdx.x & 63;
    const int ncols = P.ncols;
    const sid_t *__restrict__ tbl = P.tbl;
    const int64_t tile = (int64_t)blockDim.x * K;
    const int64_t stride = (int64_t)gridDim.x * tile;

    // (every [K] array below is indexed by fully unrolled loops only)
    for (int64_t base = (int64_t)blockIdx.x * tile; base < nrows; base += stride) {
        bool in[K];
        const sid_t *row[K];
        uint32_t st[K];
#pragma unroll
        for (int k = 0; k < K; k++) {
            const int64_t r = base + k * SCAN_T + threadIdx.x;
            in[k] = r < nrows;
            row[k] = tbl + r * ncols;
            st[k] = 0;
        }
        for (int i = 0; i < P.n; i++) {
            const int op = P.node[i].op;
            if (op <= WK_F_BOUND) {
                const int ca = P.node[i].ca, cb = P.node[i].cb;
                const sid_t va = P.node[i].va;
                const sid_t vb = (op == WK_F_BOUND) ? BLANK_ID : P.node[i].vb;
                // rows past the end read nothing and are dropped below
                sid_t a[K], b[K];
#pragma unroll
                for (int k = 0; k < K; k++)
                    a[k] = (ca >= 0 && in[k]) ? row[k][ca] : va;
#pragma unroll
                for (int k = 0; k < K; k++)
                    b[k] = (cb >= 0 && in[k]) ? row[k][cb] : vb;
                // EQ pushes a == b; NE and BOUND (b = BLANK_ID) push a != b
                const uint32_t inv = (op == WK_F_EQ) ? 0u : 1u;
#pragma unroll
                for (int k = 0; k < K; k++)
                    st[k] = (st[k] << 1) | ((uint32_t)(a[k] == b[k]) ^ inv);
            } else if (op == WK_F_AND) {
#pragma unroll
                for (int k = 0; k < K; k++)
                    st[k] = (st[k] >> 1) & (st[k] | ~1u);
            } else if (op == WK_F_OR) {
#pragma unroll
                for (int k = 0; k < K; k++)
                    st[k] = (st[k] >> 1) | (st[k] & 1u);
            } else {  // WK_F_NOT
#pragma unroll
                for (int k = 0; k < K; k++) st[k] ^= 1u;
            }
        }
        uint32_t keep = 0;
#pragma unroll
        for (int k = 0; k < K; k++)
            keep |= (in[k] && (st[k] & 1u)) ? 1u << k : 0u;
        // output <= input rows: no position can pass the capacity
        uint64_t mask[K];
        uint64_t wpos = tile_compact<K>(keep, d_state, mask);
#pragma unroll
        for (int k = 0; k < K; k++) {
            if ((keep >> k) & 1) {
                const uint64_t pos = wpos + lanes_below(mask[k], lane);
                sid_t *dst = out_tbl + (int64_t)pos * ncols;
                for (int c = 0; c < ncols; c++) dst[c] = row[k][c];
            }
            wpos += (uint32_t)__popcll(mask[k]);
        }
    }
}

// ---------------------------------------------------------------------
// VERSATILE predicate-variable ops (sparql.hpp:556-744): one kernel
// covers known/const_unknown_unknown (append p [, y] columns) and
// known/const_unknown_const (keep one row per matching p).  Block per
// input row; the row vid's predicate list comes from the dense vp CSR;
// each predicate probes its own (pid,dir) segment via the device
// segment table.  Appends use the global S_TOTAL cursor (k_commit
// finalises; overflow -> S_ERR/S_REQ re-run like every other op).
// ---------------------------------------------------------------------
enum { VU_END_NEW = 0, VU_END_CONST = 1 };
__global__ void k_vu(const vertex_t *__restrict__ verts,
                     const sid_t *__restrict__ edges,
                     const sid_t *__restrict__ in_tbl, int ncols, int col,
                     sid_t const_start,
                     const uint32_t *__restrict__ vp_off,
                     const sid_t *__restrict__ vp_edges,
                     uint64_t vp_base, uint64_t vp_n,
                     const seg_t *__restrict__ segtab, uint32_t max_pid,
                     int dir, int end_mode, sid_t cval,
                     sid_t *__restrict__ out, int out_cols, uint64_t cap_rows,
                     uint64_t *__restrict__ d_state,
                     uint64_t *__restrict__ d_stats)
{
    const uint64_t nrows = (col >= 0) ? d_state[S_NROWS] : 1;
    uint64_t bytes = 0;
    for (uint64_t r = blockIdx.x; r < nrows; r += gridDim.x) {
        sid_t vid = (col >= 0) ? in_tbl[r * ncols + col] : const_start;
        uint64_t idx = (uint64_t)vid - vp_base;
        if (idx >= vp_n) continue;
        uint64_t plo = vp_off[idx], phi = vp_off[idx + 1];
        bytes += 8;
        for (uint64_t pi = plo + threadIdx.x; pi < phi; pi += blockDim.x) {
            sid_t p = vp_edges[pi];
            uint64_t eoff = 0, esz = 0;
            if (p <= max_pid) {
                const seg_t sg = segtab[p * 2 + dir];
                if (sg.num_buckets)
                    probe_one(verts, sg.bucket_start, sg.num_buckets,
                              key_pack((uint64_t)vid, (uint64_t)p,
                                       (uint64_t)dir),
                              eoff, esz);
            }
            bytes += 4 + 148;
            if (end_mode == VU_END_CONST) {
                if (esz && bsearch_u32(edges + eoff, esz, cval)) {
                    uint64_t pos = atomicAdd(
                        (unsigned long long *)&d_state[S_TOTAL], 1ull);
                    if (pos < cap_rows) {
                        sid_t *dst = out + pos * out_cols;
                        for (int c = 0; c < ncols; c++)
                            dst[c] = in_tbl[r * ncols + c];
                        dst[ncols] = p;
                        bytes += (uint64_t)out_cols * 4;
                    }
                }
            } else {
                uint64_t pos = atomicAdd(
                    (unsigned long long *)&d_state[S_TOTAL],
                    (unsigned long long)esz);
                for (uint64_t k = 0; k < esz && pos + k < cap_rows; k++) {
                    sid_t *dst = out + (pos + k) * out_cols;
                    for (int c = 0; c < ncols; c++)
                        dst[c] = in_tbl[r * ncols + c];
                    dst[ncols] = p;
                    dst[ncols + 1] = edges[eoff + k];
                }
                bytes += esz * ((uint64_t)out_cols * 4 + 4);
            }
        }
    }
    if (bytes)
        atomicAdd((unsigned long long *)&d_stats[CAT_EXPAND],
                  (unsigned long long)bytes);
}

// ---------------------------------------------------------------------
// OPTIONAL-mode operators (sparql.hpp:100-170, 316-375; BGP-only like
// the reference, query.hpp:722-733): rows are never dropped — a row
// whose pattern fails keeps BLANK_ID in every column first bound inside
// the OPTIONAL group (blank_mask) and clears its matched flag.  This is
// a correctness/coverage path (no LUBM/WatDiv benchmark uses OPTIONAL),
// so the expansion uses a plain global append cursor.
// ---------------------------------------------------------------------
__global__ void k_filter_opt(const vertex_t *__restrict__ verts,
                             const sid_t *__restrict__ edges,
                             uint64_t bucket_start, uint64_t num_buckets,
                             sid_t *__restrict__ tbl, int ncols, int col,
                             uint32_t pid, int dir, int probe_mode, int col2,
                             sid_t cval, uint64_t list_off, uint64_t list_sz,
                             uint32_t blank_mask, uint8_t *__restrict__ flags,
                             uint64_t *__restrict__ d_state,
                             uint64_t *__restrict__ d_stats)
{
    const int64_t nrows = (int64_t)d_state[S_NROWS];
    count_bytes(d_stats, CAT_FILTER, (uint64_t)nrows * (4 + 128 + 8 + 64));
    for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
         r < nrows; r += (int64_t)gridDim.x * blockDim.x) {
        sid_t v = tbl[r * ncols + col];
        bool ok;
        if (probe_mode == PM_LIST) {
            ok = bsearch_u32(edges + list_off, list_sz, v);
        } else {
            uint64_t eoff = 0, esz = 0;
            if (v != BLANK_ID && num_buckets)
                probe_one(verts, bucket_start, num_buckets,
                          key_pack((uint64_t)v, (uint64_t)pid, (uint64_t)dir),
                          eoff, esz);
            sid_t tgt = (probe_mode == PM_CONST) ? cval
                                                 : tbl[r * ncols + col2];
            ok = esz && tgt != BLANK_ID && bsearch_u32(edges + eoff, esz, tgt);
        }
        if (!ok) {
            if (flags[r]) {
                for (int c = 0; c < ncols; c++)
                    if ((blank_mask >> c) & 1)
                        tbl[r * ncols + c] = BLANK_ID;
            }
            flags[r] = 0;
        }
    }
}

__global__ void k_expand_opt(const vertex_t *__restrict__ verts,
                             const sid_t *__restrict__ edges,
                             const sid_t *__restrict__ tbl, int ncols,
                             int col, uint32_t pid, int dir, int key_mode,
                             uint64_t bucket_start, uint64_t num_buckets,
                             const uint8_t *__restrict__ flags_in,
                             uint8_t *__restrict__ flags_out,
                             sid_t *__restrict__ out, uint64_t cap,
                             uint64_t *__restrict__ d_state,
                             uint64_t *__restrict__ d_stats)
{
    const int64_t nrows = (int64_t)d_state[S_NROWS];
    const int oc = ncols + 1;
    count_bytes(d_stats, CAT_EXPAND, (uint64_t)nrows * (4 + 128 + 8));
    // block-aggregated append (one global atomic per 256-row tile)
    // replaces the round-1 per-row cursors — a single cursor word
    // saturates at ~88 atomics/us (microarch row `dequeue`)
    __shared__ unsigned long long s_base;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t base = (int64_t)blockIdx.x * blockDim.x; base < nrows;
         base += stride) {
        const int64_t r = base + threadIdx.x;
        uint64_t eoff = 0, esz = 0, emit = 0;
        uint8_t m = 0;
        sid_t v = 0;
        if (r < nrows) {
            v = tbl[r * ncols + col];
            m = flags_in[r];
            if (m && v != BLANK_ID && num_buckets) {
                uint64_t key = (key_mode == PK_NORMAL)
                                   ? key_pack((uint64_t)v, (uint64_t)pid,
                                              (uint64_t)dir)
                                   : key_pack(0, (uint64_t)v, (uint64_t)dir);
                probe_one(verts, bucket_start, num_buckets, key, eoff, esz);
            }
            // unmatched / blank / no edges: keep the row, BLANK new
            // col; the matched flag survives unchanged
            // (sparql.hpp:328-334, 352-356)
            emit = (!m || v == BLANK_ID || esz == 0) ? 1 : esz;
        }
        // (the scan's barriers also separate the previous tile's reads of
        // s_base from this tile's write: no barrier at the loop's end)
        uint64_t block_total;
        const uint64_t my_end = block_ladder_scan(emit, &block_total);
        if (threadIdx.x == SCAN_T - 1)
            s_base = block_total
                         ? atomicAdd((unsigned long long *)&d_state[S_TOTAL],
                                     (unsigned long long)block_total)
                         : 0;
        __syncthreads();
        if (r < nrows) {
            uint64_t pos = s_base + my_end - emit;
            if (!m || v == BLANK_ID || esz == 0) {
                if (pos < cap) {
                    sid_t *dst = out + pos * oc;
                    for (int c = 0; c < ncols; c++) dst[c] = tbl[r * ncols + c];
                    dst[ncols] = BLANK_ID;
                    flags_out[pos] = m;
                }
            } else {
                for (uint64_t k = 0; k < esz && pos + k < cap; k++) {
                    sid_t *dst = out + (pos + k) * oc;
                    for (int c = 0; c < ncols; c++) dst[c] = tbl[r * ncols + c];
                    dst[ncols] = edges[eoff + k];
                    flags_out[pos + k] = 1;
                }
            }
        }
    }
}
