// wk_kernels_common.h — device-side state words with the step commit and
// query begin, probe / membership / type lookups, the tile compaction and
// the op-chain evaluators: what every kernel family shares.
// Included by gpu_engine.hip only (one translation unit).
#pragma once
#include "wk_chain_sched.h"

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
// pinned block (h_pin) slots: [0..S_WORDS) the published d_state words,
// then the sticky error of the pipelined replay window (set by every
// publish that saw S_ERR, cleared by the host alone), the CAT_COUNT byte
// counters, and what the final publish writes (k_fin_publish)
enum { HP_STICKY_ERR = 7, HP_STATS = 8, HP_FIN_COUNT = 16, HP_FIN_LIVE = 24 };
static_assert(HP_STICKY_ERR >= S_WORDS, "sticky slot overlaps the state words");
static_assert(HP_STATS + CAT_COUNT <= HP_FIN_COUNT,
              "byte counters overlap the final-ops slots");

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

// Dense side index: the single type id of v, 0 = untyped or outside
// [base, base+n), TYPE_MULTI = several types (only a probe can tell)
constexpr uint16_t TYPE_MULTI = 0xFFFF;
__device__ __forceinline__ uint16_t type_of_dense(
    const uint16_t *__restrict__ type_of, uint64_t base, uint64_t n, sid_t v) {
    const uint64_t tix = (uint64_t)v - base;
    return tix < n ? type_of[tix] : 0;
}

// `v rdf:type cval` without a probe: the per-type bitmap when it is built
// (exact, multi-type included), else the dense index, which answers
// TC_MULTI for a multi-type v.  What TC_MULTI means is each caller's own,
// DELIBERATELY different — keep them apart:
//   - typeof_nodrop_ok, k_expand_fn_map: a miss (-> S_DONE ->
//     k_publish_state -> S_ERR -> safe re-run)
//   - filter_keep: falls through to the hash probe
//   - k_fn_gather, k_peer_step: probe [v|TYPE|OUT]
enum { TC_NO = 0, TC_YES = 1, TC_MULTI = 2 };
__device__ __forceinline__ int typeof_check(
    const uint64_t *__restrict__ tbm, const uint16_t *__restrict__ type_of,
    uint64_t base, uint64_t n, sid_t cval, sid_t v) {
    if (tbm) return tbm_has(tbm, base, n, v) ? TC_YES : TC_NO;
    const uint16_t t = type_of_dense(type_of, base, n, v);
    if (t == TYPE_MULTI) return TC_MULTI;
    return (sid_t)t == cval ? TC_YES : TC_NO;
}

// No-drop verify of `v rdf:type cval` inside the optimistic kernels of a
// captured plan (k_expand_in / k_expand_big / k_expand_fn_map)
__device__ __forceinline__ bool typeof_nodrop_ok(
    const uint64_t *__restrict__ tbm, const uint16_t *__restrict__ type_of,
    uint64_t base, uint64_t n, sid_t cval, sid_t v) {
    return typeof_check(tbm, type_of, base, n, cval, v) == TC_YES;
}

// Step commit: nrows = min(total, cap); an overflow raises S_ERR and the
// required capacity for the host re-run (replaces the reference's
// rbuf-overflow assert, gpu_engine_cuda.hpp:185).  S_TOTAL and S_OVF are
// zeroed for the next step (saves a k_zero_words launch per step).  One
// thread calls it.  snapshot_inrows: the commit sits BETWEEN a step's scan
// and its writers (k_scan_mid*), which read the input row count from
// S_INROWS; a commit behind the writers (k_commit, k_peer_step) leaves
// S_INROWS alone.
__device__ __forceinline__ void commit_rows(uint64_t *__restrict__ d_state,
                                            uint64_t total, uint64_t cap,
                                            bool snapshot_inrows) {
    if (snapshot_inrows) d_state[S_INROWS] = d_state[S_NROWS];
    if (total > cap) {
        d_state[S_ERR] = 1;
        d_state[S_REQ] = max(d_state[S_REQ], total);
        total = cap;
    }
    d_state[S_NROWS] = total;
    d_state[S_TOTAL] = 0;
    d_state[S_OVF] = 0;
}

// query begin: zero every state word (S_ERR/S_REQ and the sticky S_DONE
// miss word included), then set the start row count
__device__ __forceinline__ void begin_state(uint64_t *__restrict__ d_state,
                                            uint64_t nrows) {
#pragma unroll
    for (int i = 0; i < S_WORDS; i++) d_state[i] = 0;
    d_state[S_NROWS] = nrows;
}

// lanes below `lane` whose bit is set in a ballot mask: the lane's rank
__device__ __forceinline__ uint32_t lanes_below(uint64_t mask, int lane) {
    return (uint32_t)__popcll(mask & ((1ull << lane) - 1));
}

// Ballot-rank compaction of one tile of SCAN_T * K rows (thread t holds
// rows t, t + SCAN_T, ...; bit k of `keep` = its k-th row survives): K
// ballots per thread, one LDS atomic per wave, ONE S_TOTAL atomic per
// tile, three barriers.  Owns its three LDS words; every thread of the
// SCAN_T-thread block calls it once per tile.  Fills mask[k] with the
// wave's ballot of slot k and returns the output position of the wave's
// first survivor: the survivor of slot k in lane l goes to
//   returned base + popcount(mask[0..k-1]) + lanes_below(mask[k], l)
// Positions are not clamped: a caller whose output can outgrow its input
// tests pos < cap itself (k_commit flags the overflow).
template <int K>
__device__ __forceinline__ uint64_t tile_compact(
    uint32_t keep, uint64_t *__restrict__ d_state, uint64_t (&mask)[K]) {
    __shared__ unsigned long long s_base;
    __shared__ unsigned int s_cnt;
    __shared__ unsigned int s_wbase[SCAN_T / 64];
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    if (threadIdx.x == 0) s_cnt = 0;
    __syncthreads();
    uint32_t wtot = 0;
#pragma unroll
    for (int k = 0; k < K; k++) {
        mask[k] = __ballot((keep >> k) & 1);
        wtot += (uint32_t)__popcll(mask[k]);
    }
    if (lane == 0) s_wbase[wid] = atomicAdd(&s_cnt, wtot);
    __syncthreads();
    if (threadIdx.x == 0)
        s_base = s_cnt ? atomicAdd((unsigned long long *)&d_state[S_TOTAL],
                                   (unsigned long long)s_cnt)
                       : 0;
    __syncthreads();
    return s_base + s_wbase[wid];
}

// ---------------------------------------------------------------------
// Per-row op chain: a run of consecutive 1:1 patterns
// (functional-map lookups, bitmap type tests, equality tests) evaluated
// on ONE register-resident row.  Passed by value like fparams; the host
// collector (collect_chain, gpu_engine.hip) has already resolved every
// map, bitmap, column and constant, and normalised a reversed-map k2k to
// (key col, value col).
// ---------------------------------------------------------------------
// (the op kinds, CHAIN_MAX and CHAIN_SLOTS live in wk_chain_sched.h)
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
    int32_t dst;         // FN_APPEND: the column it writes (plan order)
};
// op[] is in plan order (chain_eval walks it as it is); slot[r][s] is the
// op of slot s of dependency round r, -1 = empty (chain_schedule,
// wk_chain_sched.h), which is what chain_eval_batch walks.
struct chain_t {
    chain_op op[CHAIN_MAX];
    uint64_t fn_base, fn_n, t_base, t_n;
    int32_t nops, nrounds;
    int32_t early_out;   // batch: a wave with no live candidate stops
    int32_t slot[CHAIN_MAX][CHAIN_SLOTS];
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

// Evaluation of the chain on K candidate rows at once, in dependency
// rounds.  The host schedule (chain_schedule) packs ops
// that do not read each other's appended column into rounds of up to
// CHAIN_SLOTS = 2 slots.  A slot is, by what it loads, SL_NONE (empty, EQ,
// or skipped: no load), SL_BITS (TYPE: a bitmap word) or SL_MAP (FN_*: a
// 16-B map page, then a value).  chain_round<M0, M1> is ONE round as
// straight-line code for one pair of slot classes, in three phases over
// both slots:
//   A  pick the K keys, issue the K first-level loads of each slot
//   B  BITS: test the bits.  MAP: test the page bits, rank, issue the K
//      value loads
//   C  MAP: FN_EQ compares, FN_APPEND writes column dst
// so every first-level load of a round is issued before any is consumed,
// and so is every value load: a thread has up to 2 x K independent lookups
// in flight and a chain costs two dependent load rounds per ROUND, not per
// op.  There is no branch between a round's loads and their use (a branch
// there makes the compiler copy loaded registers where the arms meet, and
// wait for the loads to do it); chain_eval_batch picks the body with one
// wave-uniform switch per round, slots ordered by class.  The round loop
// stays rolled, slot parameters are scalar loads from the kernel arguments
// by a wave-uniform index.
// Bit j of the returned mask says whether candidate j is kept (only bits
// set in `active` can stay set).  A candidate that is inactive or has
// failed (in an earlier round, phase or slot) sends its remaining loads to
// index 0 of the page / value / bitmap array, which exists whenever the op
// does — the loads are unconditional per lane and the results of dropped
// candidates are ignored.  An op whose array is null or whose span is
// empty reads nothing and drops every candidate.  Keep/drop and the
// appended columns of kept candidates are exactly chain_eval's.  With
// C.early_out a wave in which no lane has a live candidate leaves the
// round loop (wave-uniform; the caller's barriers are outside).
// APPEND_ONLY: the candidates are known to pass (the count pass said so);
// only the FN_APPEND lookups are repeated: filter slots are skipped, the
// rounds are kept, nothing exits early.
// W is the candidates' compile-time width: the host picks the bucket that
// holds the plan's out_cols (chain_width), so every column an op reads or
// appends is below W, and the picks and sets cost W selects, not ROW_MAX.
enum { SL_NONE = 0, SL_BITS = 1, SL_MAP = 2 };

// phase A of one slot: keys (0 for a dead candidate) and first-level loads
template <int M, int K, int W>
__device__ __forceinline__ void chain_slot_load(
    const chain_t &C, const chain_op &o, const sid_t (&rows)[K][W],
    uint32_t &keep, uint32_t (&ix)[K], uint64_t (&bits)[K],
    uint32_t (&rk)[K]) {
    if constexpr (M != SL_NONE) {
        const uint64_t base = M == SL_BITS ? C.t_base : C.fn_base;
        const uint64_t n = M == SL_BITS ? C.t_n : C.fn_n;
#pragma unroll
        for (int j = 0; j < K; j++) {
            const uint64_t x = (uint64_t)row_pick(rows[j], o.a) - base;
            const bool ok = ((keep >> j) & 1) && x < n;
            keep = ok ? keep : keep & ~(1u << j);
            ix[j] = ok ? (uint32_t)x : 0u;  // x < n: fits 32 bits
        }
        if constexpr (M == SL_BITS) {
            const uint64_t *tbm = (const uint64_t *)o.data;
#pragma unroll
            for (int j = 0; j < K; j++) bits[j] = tbm[ix[j] >> 6];
        } else {
#pragma unroll
            for (int j = 0; j < K; j++) {  // one 16-B page, 12 B of it used
                const uint4 q =
                    *reinterpret_cast<const uint4 *>(&o.pg[ix[j] >> 6]);
                bits[j] = (uint64_t)q.x | ((uint64_t)q.y << 32);
                rk[j] = q.z;
            }
        }
    }
}
// phase B: bit tests; a map slot ranks and issues its value loads (the
// value replaces the rank in rk)
template <int M, int K>
__device__ __forceinline__ void chain_slot_mid(
    const chain_op &o, uint32_t &keep, const uint32_t (&ix)[K],
    const uint64_t (&bits)[K], uint32_t (&rk)[K]) {
    if constexpr (M == SL_BITS) {
#pragma unroll
        for (int j = 0; j < K; j++)
            keep = ((bits[j] >> (ix[j] & 63)) & 1) ? keep : keep & ~(1u << j);
    } else if constexpr (M == SL_MAP) {
        const sid_t *vals = (const sid_t *)o.data;
#pragma unroll
        for (int j = 0; j < K; j++) {
            const uint64_t bit = 1ull << (ix[j] & 63);
            const bool hit = ((keep >> j) & 1) && (bits[j] & bit);
            keep = hit ? keep : keep & ~(1u << j);
            rk[j] = hit ? rk[j] + (uint32_t)__popcll(bits[j] & (bit - 1)) : 0u;
        }
#pragma unroll
        for (int j = 0; j < K; j++) rk[j] = vals[rk[j]];
    }
}
// phase C of a map slot, without a branch: FN_EQ compares with column b
// and sets no column (-1), FN_APPEND sets column dst
template <int M, int K, int W>
__device__ __forceinline__ void chain_slot_end(const chain_op &o,
                                               sid_t (&rows)[K][W],
                                               uint32_t &keep,
                                               const uint32_t (&tv)[K]) {
    if constexpr (M == SL_MAP) {
        const bool eq = o.kind == CH_FN_EQ;
        const int dst = eq ? -1 : o.dst;
#pragma unroll
        for (int j = 0; j < K; j++) {
            const bool ok = tv[j] && (!eq || tv[j] == row_pick(rows[j], o.b));
            keep = ok ? keep : keep & ~(1u << j);
            row_set(rows[j], dst, tv[j]);
        }
    }
}
template <int M0, int M1, int K, int W>
__device__ __forceinline__ uint32_t chain_round(const chain_t &C,
                                                const chain_op &o0,
                                                const chain_op &o1,
                                                sid_t (&rows)[K][W],
                                                uint32_t keep) {
    uint32_t ix0[K], ix1[K], rk0[K], rk1[K];
    uint64_t b0[K], b1[K];
    chain_slot_load<M0>(C, o0, rows, keep, ix0, b0, rk0);
    chain_slot_load<M1>(C, o1, rows, keep, ix1, b1, rk1);
    chain_slot_mid<M0>(o0, keep, ix0, b0, rk0);
    chain_slot_mid<M1>(o1, keep, ix1, b1, rk1);
    chain_slot_end<M0>(o0, rows, keep, rk0);
    chain_slot_end<M1>(o1, rows, keep, rk1);
    return keep;
}

template <int NC, int K, bool APPEND_ONLY = false, int W = ROW_MAX>
__device__ __forceinline__ uint32_t chain_eval_batch(
    const chain_t &C, sid_t (&rows)[K][W], uint32_t active) {
    static_assert(K >= 1 && K <= 32, "keep mask is 32 bits");
    static_assert(NC <= W && W <= ROW_MAX, "the input columns must fit");
    static_assert(CHAIN_SLOTS == 2, "chain_round takes two slots");
    uint32_t keep = active;
#pragma unroll 1
    for (int r = 0; r < C.nrounds; r++) {
        // the slots' load classes (wave-uniform scalars); an EQ is decided
        // here, an op without its array drops everything
        int idx[2], cls[2];
#pragma unroll
        for (int s = 0; s < 2; s++) {
            const int i = C.slot[r][s];
            idx[s] = i < 0 ? 0 : i;
            const chain_op &o = C.op[idx[s]];
            cls[s] = SL_NONE;
            if (i < 0 || (APPEND_ONLY && o.kind != CH_FN_APPEND)) continue;
            if (o.kind == CH_EQ) {
#pragma unroll
                for (int j = 0; j < K; j++)
                    keep = (row_pick(rows[j], o.a) == o.cval)
                               ? keep
                               : keep & ~(1u << j);
            } else if (o.kind == CH_TYPE) {
                if (o.data && C.t_n) cls[s] = SL_BITS;
                else keep = 0;
            } else {
                if (o.pg && o.data && C.fn_n) cls[s] = SL_MAP;
                else keep = 0;
            }
        }
        const bool sw = cls[0] < cls[1];  // the heavier class first
        const chain_op &o0 = C.op[sw ? idx[1] : idx[0]];
        const chain_op &o1 = C.op[sw ? idx[0] : idx[1]];
        switch ((sw ? cls[1] : cls[0]) * 3 + (sw ? cls[0] : cls[1])) {
        case SL_MAP * 3 + SL_MAP:
            keep = chain_round<SL_MAP, SL_MAP>(C, o0, o1, rows, keep);
            break;
        case SL_MAP * 3 + SL_BITS:
            keep = chain_round<SL_MAP, SL_BITS>(C, o0, o1, rows, keep);
            break;
        case SL_MAP * 3 + SL_NONE:
            keep = chain_round<SL_MAP, SL_NONE>(C, o0, o1, rows, keep);
            break;
        case SL_BITS * 3 + SL_BITS:
            keep = chain_round<SL_BITS, SL_BITS>(C, o0, o1, rows, keep);
            break;
        case SL_BITS * 3 + SL_NONE:
            keep = chain_round<SL_BITS, SL_NONE>(C, o0, o1, rows, keep);
            break;
        default:
            break;
        }
        if (!APPEND_ONLY && C.early_out && __ballot(keep != 0) == 0) break;
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
