// wk_kernels_common.h — device-side state words, probe and membership helpers shared by every kernel family.
// Included by gpu_engine.hip only (one translation unit).
#pragma once

// ---------------------------------------------------------------------
// device kernels
// ---------------------------------------------------------------------

// probe modes
enum { PK_NORMAL = 0, PK_INDEX = 1 };   // key = [vid|pid|dir] vs [0|val|dir]
enum { PM_SIZE = 0,    // k2u: write edge count per row
       PM_CONST = 1,   // k2c: flag = (const in edge list)
       PM_COL = 2,     // k2k: flag = (row's other col in edge list)
       PM_LIST = 3,    // c2k/i2k: flag = (row col value in a FIXED list)
       PM_EQ = 4 };    // k2c via reversed functional map: flag = (col == cval)

// device query state (see engine): [0]=nrows [1]=scan total [2]=overflow
// flag [3]=required rows [4]=big-row queue length / scratch cursor
// [5]=sticky guard-miss count of the optimistic (captured-graph)
// kernels: zeroed only at query begin, turned into S_ERR by
// k_publish_state [6]=input rows snapshot; stats[0..6] = algorithmic
// bytes per category
enum { S_NROWS = 0, S_TOTAL = 1, S_ERR = 2, S_REQ = 3, S_OVF = 4,
       S_DONE = 5, S_INROWS = 6, S_WORDS = 7 };
enum { CAT_PROBE = 0, CAT_SCAN, CAT_EXPAND, CAT_FILTER, CAT_COPY, CAT_SPLIT,
       CAT_OTHER, CAT_COUNT };

constexpr int SCAN_T = 256;  // scan tile = block size of the fused kernels

__device__ __forceinline__ void count_bytes(uint64_t *stats, int cat,
                                            uint64_t bytes) {
    if (blockIdx.x == 0 && threadIdx.x == 0 && stats)
        atomicAdd((unsigned long long *)&stats[cat], (unsigned long long)bytes);
}

// sorted-membership test: edge lists are ascending (loader sort,
// base_loader.hpp:367-377) so binary search replaces the reference's
// linear scan (sparql.hpp:430-470) with identical keep-row semantics.
__device__ __forceinline__ bool bsearch_u32(const sid_t *a, uint64_t n, sid_t x) {
    uint64_t lo = 0, hi = n;
    while (lo < hi) {
        uint64_t mid = (lo + hi) >> 1;
        sid_t v = a[mid];
        if (v < x) lo = mid + 1;
        else if (v > x) hi = mid;
        else return true;
    }
    return false;
}

// per-type membership bitmap: 1 bit per vid of [base, base+n)
__device__ __forceinline__ bool tbm_has(const uint64_t *__restrict__ tbm,
                                        uint64_t base, uint64_t n, sid_t v) {
    const uint64_t ix = (uint64_t)v - base;
    return ix < n && ((tbm[ix >> 6] >> (ix & 63)) & 1);
}

// CSR side-index entry of key v ({off:40|len:24}, wk_types.h), 0 = absent
__device__ __forceinline__ uint64_t csr_entry(const fnpage_t *__restrict__ pg,
                                              const uint64_t *__restrict__ entries,
                                              uint64_t base, uint64_t n,
                                              sid_t v) {
    const uint32_t rk = rank_lookup(pg, base, n, v);
    return rk == RANK_MISS ? 0 : entries[rk];
}

// No-drop verify of `v rdf:type cval` inside the verify-fused expansions
// (k_expand_in / k_expand_big): bitmap when present, else dense type_of.
// The engine treats multi-type entities (type_of == 0xFFFF) in three
// DELIBERATELY different ways — keep them apart:
//   - here: a miss (-> S_DONE -> k_publish_state -> S_ERR -> safe re-run)
//   - filter_keep: falls through to the hash probe
//   - k_fn_gather: probes [v|TYPE|OUT]
__device__ __forceinline__ bool typeof_nodrop_ok(
    const uint64_t *__restrict__ tbm, const uint16_t *__restrict__ type_of,
    uint64_t base, uint64_t n, sid_t cval, sid_t v) {
    if (tbm) return tbm_has(tbm, base, n, v);
    const uint64_t tix = (uint64_t)v - base;
    const uint16_t t = (tix < n) ? type_of[tix] : 0;
    return t != 0xFFFF && (sid_t)t == cval;
}

// ---------------------------------------------------------------------
// Per-row op chain: a run of consecutive 1:1 patterns
// (functional-map lookups, bitmap type tests, equality tests) evaluated
// on ONE register-resident row.  Passed by value like fparams; the host
// collector (collect_chain, gpu_engine.hip) has already resolved every
// map, bitmap, column and constant, and normalised a reversed-map k2k to
// (key col, value col).
// ---------------------------------------------------------------------
enum { CH_FN_APPEND = 0,  // v = fn[row[a]]; 0 drops, else append v
       CH_TYPE = 1,       // bitmap bit of row[a] (exact, multi-type incl.)
       CH_FN_EQ = 2,      // fn[row[a]] != 0 && == row[b]   (k2k)
       CH_EQ = 3 };       // row[a] == cval                 (PM_EQ k2c)
constexpr int CHAIN_MAX = 8;  // ops per chain
constexpr int ROW_MAX = 8;    // wk_engine_begin_query rejects nvars > 8
// narrow width bucket of the batched chain kernels: candidates of a plan
// whose out_cols <= ROW_NARROW are carried as sid_t[ROW_NARROW]
constexpr int ROW_NARROW = 4;
// batched chain evaluation in the fused expansion: edges of one row per
// round (LUBM takesCourse degrees are 2-4) x rows walked side by side
constexpr int CHAIN_EK = 4;
constexpr int CHAIN_RPT = 2;

struct chain_op {
    const fnpage_t *pg;  // FN_*: map pages
    const void *data;    // FN_*: packed values; TYPE: membership bitmap
    int32_t kind, a, b;
    sid_t cval;
};
struct chain_t {
    chain_op op[CHAIN_MAX];
    uint64_t fn_base, fn_n, t_base, t_n;
    int32_t nops;
};

// Column access by a (wave-uniform) runtime index as select chains: a
// runtime-indexed local array would spill to scratch (HIP guide rule 20)
__device__ __forceinline__ sid_t row_get(const sid_t (&row)[ROW_MAX], int c) {
    sid_t v = row[0];
#pragma unroll
    for (int i = 1; i < ROW_MAX; i++) v = (c == i) ? row[i] : v;
    return v;
}
// (W: the row's compile-time width, ROW_MAX or the plan's width bucket)
template <int W>
__device__ __forceinline__ void row_set(sid_t (&row)[W], int c, sid_t v) {
#pragma unroll
    for (int i = 0; i < W; i++) row[i] = (c == i) ? v : row[i];
}

// Evaluate the chain on a row whose first NC columns are valid; appended
// columns land at NC, NC+1, ...  Returns keep/drop, stops at the first
// failing op.
template <int NC>
__device__ __forceinline__ bool chain_eval(const chain_t &C,
                                           sid_t (&row)[ROW_MAX]) {
    int nc = NC;
#pragma unroll
    for (int i = 0; i < CHAIN_MAX; i++) {
        if (i >= C.nops) break;
        const chain_op &o = C.op[i];
        const sid_t v = row_get(row, o.a);
        if (o.kind == CH_TYPE) {
            if (!tbm_has((const uint64_t *)o.data, C.t_base, C.t_n, v))
                return false;
        } else if (o.kind == CH_EQ) {
            if (v != o.cval) return false;
        } else {
            const sid_t tv = fn_lookup(o.pg, (const sid_t *)o.data, C.fn_base,
                                       C.fn_n, v);
            if (!tv) return false;
            if (o.kind == CH_FN_EQ) {
                if (tv != row_get(row, o.b)) return false;
            } else {
                row_set(row, nc++, tv);
            }
        }
    }
    return true;
}

// Column pick for the batched evaluator.  Same contract as row_get, but
// built from AND/OR masks: a chain of selects between two loaded columns
// can be rewritten by the optimiser into ONE load at a selected address
// while the K x W candidate array still lives in memory, which then
// never becomes registers (observed: 144-400 B of scratch per lane).
template <int W>
__device__ __forceinline__ sid_t row_pick(const sid_t (&row)[W], int c) {
    sid_t v = 0;
#pragma unroll
    for (int i = 0; i < W; i++) v |= row[i] & (0u - (sid_t)(c == i));
    return v;
}

// Op-major evaluation of the chain on K candidate rows at once (DESIGN.md
// §3 5i): for every op the K loads of one level (bitmap words; map pages;
// map values) are issued before any of them is consumed, so a thread keeps
// K independent lookups in flight where chain_eval has one.  Nothing exits
// early: bit j of the returned mask says whether candidate j is kept (only
// bits set in `active` can stay set), and a candidate that is inactive or
// has failed sends its remaining loads to index 0 of the page / value /
// bitmap array, which exists whenever the op does — the loads are
// unconditional and the results of dropped candidates are ignored.  An op
// whose array is null or whose span is empty reads nothing and drops every
// candidate.  Keep/drop and the appended columns are exactly chain_eval's.
// APPEND_ONLY: the candidates are known to pass (the count pass said so);
// only the FN_APPEND lookups are repeated, the filter ops are skipped.
// W is the candidates' compile-time width: the host picks the bucket that
// holds the plan's out_cols (chain_width), so every column an op reads or
// appends is below W, and the picks and sets cost W selects, not ROW_MAX.
template <int NC, int K, bool APPEND_ONLY = false, int W = ROW_MAX>
__device__ __forceinline__ uint32_t chain_eval_batch(
    const chain_t &C, sid_t (&rows)[K][W], uint32_t active) {
    static_assert(K >= 1 && K <= 32, "keep mask is 32 bits");
    static_assert(NC <= W && W <= ROW_MAX, "the input columns must fit");
    uint32_t keep = active;
    int nc = NC;
    // the op loop stays rolled: one op's parameters are read from the
    // kernel arguments by a wave-uniform index (scalar loads), which keeps
    // the K-wide body within the register budget
#pragma unroll 1
    for (int i = 0; i < C.nops; i++) {
        const chain_op &o = C.op[i];
        if (o.kind == CH_TYPE) {
            if (APPEND_ONLY) continue;
            const uint64_t *tbm = (const uint64_t *)o.data;
            if (!tbm || !C.t_n) { keep = 0; continue; }
            uint64_t ix[K], w[K];
#pragma unroll
            for (int j = 0; j < K; j++) {
                const uint64_t x = (uint64_t)row_pick(rows[j], o.a) - C.t_base;
                const bool ok = ((keep >> j) & 1) && x < C.t_n;
                keep = ok ? keep : keep & ~(1u << j);
                ix[j] = ok ? x : 0;
            }
#pragma unroll
            for (int j = 0; j < K; j++) w[j] = tbm[ix[j] >> 6];
#pragma unroll
            for (int j = 0; j < K; j++)
                keep = ((w[j] >> (ix[j] & 63)) & 1) ? keep : keep & ~(1u << j);
        } else if (o.kind == CH_EQ) {
            if (APPEND_ONLY) continue;
#pragma unroll
            for (int j = 0; j < K; j++)
                keep = (row_pick(rows[j], o.a) == o.cval) ? keep
                                                          : keep & ~(1u << j);
        } else {
            if (APPEND_ONLY && o.kind != CH_FN_APPEND) continue;
            const sid_t *vals = (const sid_t *)o.data;
            if (!o.pg || !vals || !C.fn_n) {
                keep = 0;
                if (o.kind == CH_FN_APPEND) nc++;
                continue;
            }
            uint64_t ix[K], bits[K];
            uint32_t rk[K];
            sid_t tv[K];
#pragma unroll
            for (int j = 0; j < K; j++) {
                const uint64_t x = (uint64_t)row_pick(rows[j], o.a) - C.fn_base;
                const bool ok = ((keep >> j) & 1) && x < C.fn_n;
                keep = ok ? keep : keep & ~(1u << j);
                ix[j] = ok ? x : 0;
            }
#pragma unroll
            for (int j = 0; j < K; j++) {  // one 16-B load per page
                const uint4 q =
                    *reinterpret_cast<const uint4 *>(&o.pg[ix[j] >> 6]);
                bits[j] = (uint64_t)q.x | ((uint64_t)q.y << 32);
                rk[j] = q.z;
            }
#pragma unroll
            for (int j = 0; j < K; j++) {
                const uint64_t bit = 1ull << (ix[j] & 63);
                const bool hit = ((keep >> j) & 1) && (bits[j] & bit);
                keep = hit ? keep : keep & ~(1u << j);
                rk[j] = hit ? rk[j] + (uint32_t)__popcll(bits[j] & (bit - 1))
                            : 0u;
            }
#pragma unroll
            for (int j = 0; j < K; j++) tv[j] = vals[rk[j]];
            if (o.kind == CH_FN_EQ) {
#pragma unroll
                for (int j = 0; j < K; j++)
                    keep = (tv[j] && tv[j] == row_pick(rows[j], o.b))
                               ? keep
                               : keep & ~(1u << j);
            } else {
#pragma unroll
                for (int j = 0; j < K; j++) {
                    keep = tv[j] ? keep : keep & ~(1u << j);
                    row_set(rows[j], nc, tv[j]);
                }
                nc++;
            }
        }
    }
    return keep;
}

// one cluster-hash lookup: walk the bucket chain, 7 slot compares per
// 128-B bucket (gstore.hpp:341-361 semantics)
__device__ __forceinline__ void probe_one(const vertex_t *__restrict__ verts,
                                          uint64_t bucket_start,
                                          uint64_t num_buckets, uint64_t key,
                                          uint64_t &eoff, uint64_t &esz) {
    uint64_t bucket = bucket_start + hash_u64(key) % num_buckets;
    while (true) {
        const vertex_t *b = &verts[bucket * ASSOC];
        uint64_t k0 = b[0].key, k1 = b[1].key, k2 = b[2].key, k3 = b[3].key;
        uint64_t k4 = b[4].key, k5 = b[5].key, k6 = b[6].key, k7 = b[7].key;
        int hit = -1;
        if (k0 == key) hit = 0;
        else if (k1 == key) hit = 1;
        else if (k2 == key) hit = 2;
        else if (k3 == key) hit = 3;
        else if (k4 == key) hit = 4;
        else if (k5 == key) hit = 5;
        else if (k6 == key) hit = 6;
        if (hit >= 0) {
            uint64_t pp = b[hit].ptr;
            eoff = ptr_off(pp);
            esz = ptr_size(pp);
            return;
        }
        if (k7 == KEY_EMPTY) { eoff = 0; esz = 0; return; }
        bucket = key_vid(k7);
    }
}

// continue a probe from a chained bucket (absolute bucket id)
__device__ __forceinline__ void probe_chain(const vertex_t *__restrict__ verts,
                                            uint64_t bucket, uint64_t key,
                                            uint64_t &eoff, uint64_t &esz) {
    while (true) {
        const vertex_t *b = &verts[bucket * ASSOC];
        int hit = -1;
#pragma unroll
        for (int i = 0; i < ASSOC - 1; i++)
            if (b[i].key == key && hit < 0) hit = i;
        if (hit >= 0) {
            eoff = ptr_off(b[hit].ptr);
            esz = ptr_size(b[hit].ptr);
            return;
        }
        if (b[ASSOC - 1].key == KEY_EMPTY) { eoff = 0; esz = 0; return; }
        bucket = key_vid(b[ASSOC - 1].key);
    }
}
