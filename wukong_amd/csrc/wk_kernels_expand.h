// wk_kernels_expand.h — probe and gather kernels (the front half of a
// known_to_unknown step), the writers behind the scan with their big-row
// passes, and the stand-alone row pass k_row_chain.
// Included by gpu_engine.hip only (one translation unit).
#pragma once

// Fused known_to_unknown front half: contiguous-chunk thread-per-row
// probe + in-kernel exclusive prefix of the edge counts (local prefix +
// per-block sums; k_scan_mid finishes across blocks).  64 rows in
// flight per wave between scan barriers — MLP for DRAM-random probes
// (gstore.hpp:341-361; replaces gpu_hash.cu:94-324 + the thrust scan).
__global__ void k_probe_scan(const vertex_t *__restrict__ verts,
                             const sid_t *__restrict__ tbl, int ncols,
                             int col, uint32_t pid, int dir, int key_mode,
                             uint64_t bucket_start, uint64_t num_buckets,
                             uint64_t *__restrict__ d_state,
                             uint64_t *__restrict__ d_stats,
                             uint64_t *__restrict__ d_eoff,
                             uint32_t *__restrict__ d_cnt,
                             uint64_t *__restrict__ d_pre,
                             uint64_t *__restrict__ bsums)
{
    const int64_t nrows = (int64_t)d_state[S_NROWS];
    count_bytes(d_stats, CAT_PROBE, (uint64_t)nrows * (4 + 128 + 8 + 12));
    const int64_t chunk = (nrows + gridDim.x - 1) / gridDim.x;
    const int64_t start = (int64_t)blockIdx.x * chunk;
    const int64_t end = min(start + chunk, nrows);
    uint64_t carry = 0;

    // 2-deep pipeline: the NEXT tile row's first bucket is issued before
    // this tile's scan phase, so its ~900-cycle HBM latency hides under
    // the LDS scan + barriers (loads to registers stay in flight across
    // s_barrier; hipcc waits at first use)
    auto key_of = [&](int64_t r) {
        sid_t v = tbl[r * ncols + col];
        return (key_mode == PK_NORMAL) ? key_pack(v, pid, (uint64_t)dir)
                                       : key_pack(0, v, (uint64_t)dir);
    };
    uint64_t nkey = 0, nbucket = 0;
    uint64_t pk[ASSOC];
    uint64_t pp[ASSOC - 1];
    bool have_pref = false;
    if (start + threadIdx.x < end) {
        nkey = key_of(start + threadIdx.x);
        nbucket = bucket_start + hash_u64(nkey) % num_buckets;
        const vertex_t *b = &verts[nbucket * ASSOC];
#pragma unroll
        for (int i = 0; i < ASSOC; i++) pk[i] = b[i].key;
#pragma unroll
        for (int i = 0; i < ASSOC - 1; i++) pp[i] = b[i].ptr;
        have_pref = true;
    }
    for (int64_t base = start; base < end; base += SCAN_T) {
        const int64_t r = base + threadIdx.x;
        uint64_t eoff = 0, esz = 0;
        uint64_t key = nkey;
        uint64_t ck[ASSOC], cp[ASSOC - 1];
        bool have = have_pref;
        if (have) {
#pragma unroll
            for (int i = 0; i < ASSOC; i++) ck[i] = pk[i];
#pragma unroll
            for (int i = 0; i < ASSOC - 1; i++) cp[i] = pp[i];
        }
        // issue next tile's first bucket
        const int64_t rn = base + SCAN_T + threadIdx.x;
        have_pref = false;
        if (rn < end) {
            nkey = key_of(rn);
            nbucket = bucket_start + hash_u64(nkey) % num_buckets;
            const vertex_t *b = &verts[nbucket * ASSOC];
#pragma unroll
            for (int i = 0; i < ASSOC; i++) pk[i] = b[i].key;
#pragma unroll
            for (int i = 0; i < ASSOC - 1; i++) pp[i] = b[i].ptr;
            have_pref = true;
        }
        if (have) {
            // resolve the prefetched bucket; rare chains fall back to the walk
            int hit = -1;
#pragma unroll
            for (int i = 0; i < ASSOC - 1; i++)
                if (ck[i] == key && hit < 0) hit = i;
            if (hit >= 0) {
                eoff = ptr_off(cp[hit]);
                esz = ptr_size(cp[hit]);
            } else if (ck[ASSOC - 1] != KEY_EMPTY) {
                // rare (~13% of buckets): continue down the chain
                probe_chain(verts, key_vid(ck[ASSOC - 1]), key, eoff, esz);
            }
            d_eoff[r] = eoff;
            d_cnt[r] = (uint32_t)esz;
        }
        uint64_t total;
        const uint64_t incl = block_ladder_scan(esz, &total);
        if (r < end) d_pre[r] = carry + incl - esz;
        carry += total;
    }
    if (threadIdx.x == 0) bsums[blockIdx.x] = (start < end) ? carry : 0;
}

// CSR-indexed known_to_unknown front half (non-functional segments):
// the 128-B cluster-hash bucket walk becomes a 16-B page + 8-B entry
// lookup ({edge_off:40|len:24}, rank-compressed like the fn maps).
// Two phases, following the two-phase fn lesson: a barrier-free 1:1
// gather writes (eoff, cnt); k_scan_local then runs the chunked
// prefix exactly as k_probe_scan produced it, so the expansion
// kernels consume the identical layout.
__global__ void k_csr_gather(const sid_t *__restrict__ tbl, int ncols,
                             int col,
                             const fnpage_t *__restrict__ pg,
                             const uint64_t *__restrict__ entries,
                             uint64_t base, uint64_t n,
                             const uint64_t *__restrict__ d_state,
                             uint64_t *__restrict__ d_stats,
                             uint64_t *__restrict__ d_eoff,
                             uint32_t *__restrict__ d_cnt)
{
    const int64_t nrows = (int64_t)d_state[S_NROWS];
    count_bytes(d_stats, CAT_PROBE, (uint64_t)nrows * (4 + 16 + 8 + 12));
    for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
         r < nrows; r += (int64_t)gridDim.x * blockDim.x) {
        const uint64_t e =
            csr_entry(pg, entries, base, n, tbl[r * ncols + col]);
        d_eoff[r] = csr_off(e);
        d_cnt[r] = csr_len(e);
    }
}

// Counting variant for the EXACT fused `k2u + ?v rdf:type CONST`
// compaction (nothing optimistic: output == expansion+filter output):
// per row, CSR entry lookup, then ONE walk of the edge list counting
// values whose type-bitmap bit is set.  d_cnt gets the FILTERED count
// (the scan then yields exact output positions); d_eoff packs
// {edge_off:40 | full_len:24} so the writer can re-walk the list.
__global__ void k_csr_gather_tf(const sid_t *__restrict__ tbl, int ncols,
                                int col,
                                const fnpage_t *__restrict__ pg,
                                const uint64_t *__restrict__ entries,
                                uint64_t base, uint64_t n,
                                const sid_t *__restrict__ edges,
                                const uint64_t *__restrict__ tbm,
                                uint64_t t_base, uint64_t t_n,
                                const uint64_t *__restrict__ d_state,
                                uint64_t *__restrict__ d_stats,
                                uint64_t *__restrict__ d_eoff,
                                uint32_t *__restrict__ d_cnt)
{
    const int64_t nrows = (int64_t)d_state[S_NROWS];
    count_bytes(d_stats, CAT_PROBE, (uint64_t)nrows * (4 + 16 + 8 + 12));
    for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
         r < nrows; r += (int64_t)gridDim.x * blockDim.x) {
        const uint64_t e =
            csr_entry(pg, entries, base, n, tbl[r * ncols + col]);
        const uint64_t off = csr_off(e);
        const uint32_t len = csr_len(e);
        uint32_t keep = 0;
        for (uint32_t k = 0; k < len; k++)
            keep += tbm_has(tbm, t_base, t_n, edges[off + k]) ? 1u : 0u;
        d_eoff[r] = e;  // {off:40|len:24} for the writer's re-walk
        d_cnt[r] = keep;
    }
}

// writer for the fused compaction: re-walk the edge list, emit only
// passing values at the exact scanned positions (wave-ballot ranks for
// the big-row pass below)
template <int NC>
__global__ void k_expand_tf(const sid_t *__restrict__ tbl, int ncols,
                            const sid_t *__restrict__ edges,
                            const uint64_t *__restrict__ d_eoff,
                            const uint32_t *__restrict__ d_cnt,
                            const uint64_t *__restrict__ d_pre,
                            const uint64_t *__restrict__ bsums, int G,
                            const uint64_t *__restrict__ tbm,
                            uint64_t t_base, uint64_t t_n,
                            uint64_t *__restrict__ d_state, uint64_t cap,
                            uint64_t *__restrict__ d_stats,
                            uint32_t *__restrict__ ovf,
                            sid_t *__restrict__ out)
{
    const int64_t nrows = (int64_t)d_state[S_INROWS];
    const int64_t chunk = (nrows + G - 1) / G;
    constexpr int oc = NC + 1;
    (void)ncols;
    for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < nrows;
         r += (int64_t)gridDim.x * blockDim.x) {
        const uint32_t keep = d_cnt[r];
        if (!keep) continue;
        const uint64_t basep = scan_pos(d_pre, bsums, chunk, r);
        if (basep >= cap) continue;
        const uint64_t e = d_eoff[r];
        const uint64_t off = csr_off(e);
        const uint32_t len = csr_len(e);
        if (len > 32) {
            ovf_push(d_state, ovf, r);
            continue;
        }
        sid_t row[NC];
#pragma unroll
        for (int c = 0; c < NC; c++) row[c] = tbl[r * NC + c];
        sid_t *dst = out + (int64_t)basep * oc;
        uint32_t w = 0;
        for (uint32_t k = 0; k < len && w < keep; k++) {
            sid_t v = edges[off + k];
            if (!tbm_has(tbm, t_base, t_n, v)) continue;
            if (basep + w >= cap) break;
#pragma unroll
            for (int c = 0; c < NC; c++) dst[c] = row[c];
            dst[NC] = v;
            dst += oc;
            w++;
        }
    }
}

template <int NC>
__global__ void k_expand_tf_big(const sid_t *__restrict__ tbl, int ncols,
                                const sid_t *__restrict__ edges,
                                const uint64_t *__restrict__ d_eoff,
                                const uint32_t *__restrict__ d_cnt,
                                const uint64_t *__restrict__ d_pre,
                                const uint64_t *__restrict__ bsums, int G,
                                const uint64_t *__restrict__ tbm,
                                uint64_t t_base, uint64_t t_n,
                                uint64_t *__restrict__ d_state, uint64_t cap,
                                const uint32_t *__restrict__ ovf,
                                sid_t *__restrict__ out)
{
    const int64_t nq = (int64_t)d_state[S_OVF];
    const int64_t nrows = (int64_t)d_state[S_INROWS];
    const int64_t chunk = (nrows + G - 1) / G;
    constexpr int oc = NC + 1;
    (void)ncols;
    const int64_t w0 = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const int64_t nw = ((int64_t)gridDim.x * blockDim.x) >> 6;
    for (int64_t q = w0; q < nq; q += nw) {
        const int64_t r = ovf[q];
        const uint64_t e = d_eoff[r];
        const uint64_t basep = scan_pos(d_pre, bsums, chunk, r);
        if (basep >= cap) continue;
        sid_t row[oc];
#pragma unroll
        for (int c = 0; c < NC; c++) row[c] = tbl[r * NC + c];
        wave_emit_rows<NC>(row, edges + csr_off(e), csr_len(e), basep, cap, oc,
                           out, [&](const sid_t (&cand)[oc]) {
                               return tbm_has(tbm, t_base, t_n, cand[NC]);
                           });
    }
}

// The same exact count -> scan -> emit pipeline with a per-row op chain
// (wk_kernels_common.h chain_t) as the per-edge
// predicate: the candidate row is the NC-column input row plus the edge
// value, the chain tests it (and may append further columns), d_cnt gets
// the number of PASSING edges.  Siblings of the typeof-only kernels
// above, which stay as they are (both of their paths are measured).
// The count pass evaluates the chain op-major (chain_eval_batch) and
// leaves a 32-bit pass mask per row (bit k = edge k passes) in d_pmask,
// so the writer of a <= 32-edge row takes the passing edges from the
// mask and repeats only the chain's FN_APPEND lookups.
// W (here and in k_expand_chain, k_row_chain) is the candidate rows'
// compile-time width, the bucket that holds the plan's out_cols: the
// candidate array and every column pick / set scale with it.
template <int NC, int W>
__global__ void __launch_bounds__(SCAN_T)
k_csr_gather_chain(const sid_t *__restrict__ tbl, int col,
                                   const fnpage_t *__restrict__ pg,
                                   const uint64_t *__restrict__ entries,
                                   uint64_t base, uint64_t n,
                                   const sid_t *__restrict__ edges,
                                   chain_t C,
                                   const uint64_t *__restrict__ d_state,
                                   uint64_t *__restrict__ d_stats,
                                   uint64_t *__restrict__ d_eoff,
                                   uint32_t *__restrict__ d_cnt,
                                   uint32_t *__restrict__ d_pmask)
{
    static_assert(NC < W && W <= ROW_MAX, "the edge value needs a column");
    static_assert(32 % CHAIN_EK == 0, "pass-mask groups must tile 32 bits");
    constexpr int RPT = CHAIN_RPT, EK = CHAIN_EK, K = RPT * EK;
    const int64_t nrows = (int64_t)d_state[S_NROWS];
    count_bytes(d_stats, CAT_PROBE,
                (uint64_t)nrows * (4 * NC + 16 + 8 + 12 + 4));
    // a thread takes RPT rows H apart and walks their edge lists side by
    // side, EK edges of each per round: K candidates per chain_eval_batch
    // call.  H is the grid stride T, or ceil(nrows / RPT) for a table of
    // fewer than RPT * T rows (one round, threads below H), so that small
    // tables pair rows too.  A row past the end or out of edges is
    // inactive (its loads go to edges[0], which always exists).
    const int64_t T = (int64_t)gridDim.x * blockDim.x;
    const int64_t H = min(T, (nrows + RPT - 1) / RPT);
    const int64_t lim = H < T ? H : nrows;
    for (int64_t r0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
         r0 < lim; r0 += T * RPT) {
        sid_t in[RPT][NC];
        uint64_t e[RPT];
        uint32_t len[RPT], keep[RPT], pmask[RPT];
#pragma unroll
        for (int q = 0; q < RPT; q++) {
            const int64_t r = r0 + q * H;
            const int64_t rr = r < nrows ? r : r0;
#pragma unroll
            for (int c = 0; c < NC; c++) in[q][c] = tbl[rr * NC + c];
        }
        uint32_t maxlen = 0;
#pragma unroll
        for (int q = 0; q < RPT; q++) {
            sid_t key = in[q][0];
#pragma unroll
            for (int c = 1; c < NC; c++) key = (col == c) ? in[q][c] : key;
            e[q] = csr_entry(pg, entries, base, n, key);
            len[q] = (r0 + q * H < nrows) ? csr_len(e[q]) : 0u;
            keep[q] = 0;
            pmask[q] = 0;
            maxlen = max(maxlen, len[q]);
        }
        for (uint32_t k0 = 0; k0 < maxlen; k0 += EK) {
            sid_t cand[K][W];
            uint32_t active = 0;
#pragma unroll
            for (int q = 0; q < RPT; q++) {
                const uint64_t off = csr_off(e[q]);
#pragma unroll
                for (int j = 0; j < EK; j++) {
                    const bool on = k0 + j < len[q];
                    active |= on ? 1u << (q * EK + j) : 0u;
#pragma unroll
                    for (int c = 0; c < W; c++) cand[q * EK + j][c] = 0;
#pragma unroll
                    for (int c = 0; c < NC; c++)
                        cand[q * EK + j][c] = in[q][c];
                    cand[q * EK + j][NC] = edges[on ? off + k0 + j : 0];
                }
            }
            const uint32_t m = chain_eval_batch<NC + 1, K>(C, cand, active);
#pragma unroll
            for (int q = 0; q < RPT; q++) {
                const uint32_t mq = (m >> (q * EK)) & ((1u << EK) - 1);
                keep[q] += (uint32_t)__popc(mq);
                // bit k of the pass mask = edge k passes (rows of <= 32
                // edges; the writer sends longer rows to the wave pass)
                pmask[q] |= k0 < 32 ? mq << k0 : 0u;
            }
        }
#pragma unroll
        for (int q = 0; q < RPT; q++) {
            const int64_t r = r0 + q * H;
            if (r < nrows) {
                d_eoff[r] = e[q];  // {off:40|len:24} for the writer
                d_cnt[r] = keep[q];
                d_pmask[r] = pmask[q];
            }
        }
    }
}

// writer: emit the passing (widened) rows at the exact scanned positions,
// taking the passing edges from the count pass's mask; rows with > 32
// edges go to the wave pass, which re-evaluates the chain
template <int NC, int W>
__global__ void __launch_bounds__(SCAN_T)
k_expand_chain(const sid_t *__restrict__ tbl,
                               const sid_t *__restrict__ edges,
                               const uint64_t *__restrict__ d_eoff,
                               const uint32_t *__restrict__ d_cnt,
                               const uint32_t *__restrict__ d_pmask,
                               const uint64_t *__restrict__ d_pre,
                               const uint64_t *__restrict__ bsums, int G,
                               chain_t C, int oc,
                               uint64_t *__restrict__ d_state, uint64_t cap,
                               uint64_t *__restrict__ d_stats,
                               uint32_t *__restrict__ ovf,
                               sid_t *__restrict__ out)
{
    static_assert(NC < W && W <= ROW_MAX, "the edge value needs a column");
    constexpr int EK = CHAIN_EK;
    const int64_t nrows = (int64_t)d_state[S_INROWS];
    const int64_t chunk = (nrows + G - 1) / G;
    for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < nrows;
         r += (int64_t)gridDim.x * blockDim.x) {
        const uint32_t keep = d_cnt[r];
        if (!keep) continue;
        const uint64_t basep = scan_pos(d_pre, bsums, chunk, r);
        if (basep >= cap) continue;
        const uint64_t e = d_eoff[r];
        const uint64_t off = csr_off(e);
        const uint32_t len = csr_len(e);
        if (len > 32) {
            ovf_push(d_state, ovf, r);
            continue;
        }
        sid_t in[NC];
#pragma unroll
        for (int c = 0; c < NC; c++) in[c] = tbl[r * NC + c];
        sid_t *dst = out + (int64_t)basep * oc;
        uint32_t w = 0;
        // the passing edges, lowest first, EK at a time: their values are
        // loaded together, and so are the FN_APPEND lookups of a chain
        // that widens the row (off is valid: keep > 0 means len > 0)
        for (uint32_t m = d_pmask[r]; m;) {
            sid_t cand[EK][W];
            uint32_t act = 0;
#pragma unroll
            for (int j = 0; j < EK; j++) {
                const bool on = m != 0;
                const uint32_t p = on ? (uint32_t)__ffs((int)m) - 1u : 0u;
                m &= m - 1;
                act |= on ? 1u << j : 0u;
#pragma unroll
                for (int c = 0; c < W; c++) cand[j][c] = 0;
#pragma unroll
                for (int c = 0; c < NC; c++) cand[j][c] = in[c];
                cand[j][NC] = edges[off + p];
            }
            if (oc > NC + 1)
                act = chain_eval_batch<NC + 1, EK, true>(C, cand, act);
#pragma unroll
            for (int j = 0; j < EK; j++) {
                if (((act >> j) & 1) && basep + w < cap) {
#pragma unroll
                    for (int c = 0; c < W; c++)
                        if (c < oc) dst[c] = cand[j][c];
                    dst += oc;
                    w++;
                }
            }
        }
    }
    // written rows + per-input-row scan words and pass mask (the walk
    // itself is counted by the gather)
    if (blockIdx.x == 0 && threadIdx.x == 0)
        atomicAdd((unsigned long long *)&d_stats[CAT_EXPAND],
                  (unsigned long long)(d_state[S_NROWS] * (4 * oc) +
                                       (uint64_t)nrows * 24));
}

template <int NC>
__global__ void k_expand_chain_big(const sid_t *__restrict__ tbl,
                                   const sid_t *__restrict__ edges,
                                   const uint64_t *__restrict__ d_eoff,
                                   const uint64_t *__restrict__ d_pre,
                                   const uint64_t *__restrict__ bsums, int G,
                                   chain_t C, int oc,
                                   const uint64_t *__restrict__ d_state,
                                   uint64_t cap,
                                   const uint32_t *__restrict__ ovf,
                                   sid_t *__restrict__ out)
{
    static_assert(NC < ROW_MAX, "the edge value needs a column");
    const int64_t nq = (int64_t)d_state[S_OVF];
    const int64_t nrows = (int64_t)d_state[S_INROWS];
    const int64_t chunk = (nrows + G - 1) / G;
    const int64_t w0 = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const int64_t nw = ((int64_t)gridDim.x * blockDim.x) >> 6;
    for (int64_t q = w0; q < nq; q += nw) {
        const int64_t r = ovf[q];
        const uint64_t e = d_eoff[r];
        const uint64_t basep = scan_pos(d_pre, bsums, chunk, r);
        if (basep >= cap) continue;
        sid_t row[ROW_MAX];
#pragma unroll
        for (int c = 0; c < ROW_MAX; c++) row[c] = 0;
#pragma unroll
        for (int c = 0; c < NC; c++) row[c] = tbl[r * NC + c];
        wave_emit_rows<NC>(row, edges + csr_off(e), csr_len(e), basep, cap, oc,
                           out, [&](sid_t (&cand)[ROW_MAX]) {
                               return chain_eval<NC + 1>(C, cand);
                           });
    }
}

// Stand-alone row pass: a run of >= 2 per-row patterns
// that does not follow a CSR expansion, as ONE kernel over the table
// (possibly a zero-copy view): each thread evaluates the chain op-major
// on the 4 rows of its tile slots (chain_eval_batch), survivors are
// compacted at the widened width with tile_compact, whose positions can
// pass the capacity here (FN_APPEND widens the rows): pos < cap is tested
// per row; k_commit follows.  Exact; nothing counts into S_DONE.
// (1- and 2-column tables of the narrow bucket are held to the 64 VGPRs of
// 8 waves per SIMD, at which the 2048-block grid is resident at once: the
// two-slot round body comes out at 66 without the bound, at 64 and no
// scratch with it; wider inputs would spill VGPRs under it and stay at 7)
template <int NC, int W>
__global__ void
__launch_bounds__(SCAN_T, W == ROW_NARROW && NC <= 2 ? 8 : 1)
k_row_chain(const sid_t *__restrict__ tbl, chain_t C, int oc,
            uint64_t *__restrict__ d_state, uint64_t cap,
            uint64_t *__restrict__ d_stats, sid_t *__restrict__ out)
{
    static_assert(NC <= W && W <= ROW_MAX, "the input columns must fit");
    constexpr int K = 4;
    const int64_t nrows = (int64_t)d_state[S_NROWS];
    count_bytes(d_stats, CAT_FILTER, (uint64_t)nrows * (4 * NC + 4 * oc));
    const int lane = threadIdx.x & 63;
    const int64_t tile = (int64_t)SCAN_T * K;
    const int64_t stride = (int64_t)gridDim.x * tile;
    for (int64_t base = (int64_t)blockIdx.x * tile; base < nrows;
         base += stride) {
        sid_t rows[K][W];
        uint32_t active = 0;
#pragma unroll
        for (int k = 0; k < K; k++) {
            const int64_t r = base + k * SCAN_T + threadIdx.x;
            const bool in = r < nrows;
            const int64_t rr = in ? r : base;  // base < nrows: a valid row
            active |= in ? 1u << k : 0u;
#pragma unroll
            for (int c = 0; c < W; c++) rows[k][c] = 0;
#pragma unroll
            for (int c = 0; c < NC; c++) rows[k][c] = tbl[rr * NC + c];
        }
        const uint32_t keep = chain_eval_batch<NC, K>(C, rows, active);
        uint64_t mask[K];
        uint64_t wpos = tile_compact<K>(keep, d_state, mask);
#pragma unroll
        for (int k = 0; k < K; k++) {
            const uint64_t pos = wpos + lanes_below(mask[k], lane);
            if (((keep >> k) & 1) && pos < cap) {  // past cap: k_commit flags
                sid_t *dst = out + (int64_t)pos * oc;
#pragma unroll
                for (int c = 0; c < W; c++)
                    if (c < oc) dst[c] = rows[k][c];
            }
            wpos += (uint32_t)__popcll(mask[k]);
        }
    }
}

// fn-expansion scatter (phase 4 of gather -> scan_local -> scan_mid ->
// scatter): deterministic positions, no atomics, barrier-free.
template <int NC>
__global__ void k_fn_scatter(const sid_t *__restrict__ tbl,
                             const sid_t *__restrict__ d_val,
                             const uint32_t *__restrict__ d_cnt,
                             const uint64_t *__restrict__ d_pre,
                             const uint64_t *__restrict__ bsums, int G,
                             const uint64_t *__restrict__ d_state,
                             uint64_t *__restrict__ d_stats,
                             sid_t *__restrict__ out)
{
    const int64_t nrows = (int64_t)d_state[S_INROWS];  // scan_mid committed
    constexpr int oc = NC + 1;
    count_bytes(d_stats, CAT_EXPAND, (uint64_t)nrows * (4 + 4 * NC + 4 * oc));
    const int64_t chunk = (nrows + G - 1) / G;
    for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
         r < nrows; r += (int64_t)gridDim.x * blockDim.x) {
        if (!d_cnt[r]) continue;
        const uint64_t pos = scan_pos(d_pre, bsums, chunk, r);
        sid_t *dst = out + (int64_t)pos * oc;
        const sid_t *srow = tbl + r * NC;
#pragma unroll
        for (int c = 0; c < NC; c++) dst[c] = srow[c];
        dst[NC] = d_val[r];
    }
}

// Input-centric expansion (known_to_unknown back half,
// sparql.hpp:325-367): thread r writes its deg outputs at
// pre[r]+bsums[chunk(r)] — no per-output binary search (the
// output-centric version paid 2-3 DRAM lines of prefix walk per output
// row).  Rows with deg > 32 go to an overflow queue handled by
// k_expand_big with one WAVE per row (lanes stride the edge list).
// verify-fused expansion (captured graphs only): when the NEXT pattern
// is a no-drop `?v rdf:type CONST` filter on the NEW column (warm-pass
// hint), each written value is checked inline (bitmap or dense type_of;
// misses count into S_DONE -> k_publish_state -> S_ERR -> safe re-run)
// and the separate full-table verify pass disappears.
template <int NC>
__global__ void k_expand_in(const sid_t *__restrict__ tbl, int ncols,
                            const sid_t *__restrict__ edges,
                            const uint64_t *__restrict__ d_eoff,
                            const uint32_t *__restrict__ d_cnt,
                            const uint64_t *__restrict__ d_pre,
                            const uint64_t *__restrict__ bsums, int G,
                            uint64_t *__restrict__ d_state, uint64_t cap,
                            uint64_t *__restrict__ d_stats,
                            uint32_t *__restrict__ ovf,
                            const uint64_t *__restrict__ vtbm,
                            const uint16_t *__restrict__ v_type_of,
                            uint64_t v_type_base, uint64_t v_type_n,
                            sid_t v_cval, int verify,
                            sid_t *__restrict__ out)
{
    // k_scan_mid already committed: S_INROWS = the input row count,
    // S_NROWS = the (capped) output total
    const int64_t nrows = (int64_t)d_state[S_INROWS];
    const int64_t chunk = (nrows + G - 1) / G;
    constexpr int oc = NC + 1;
    (void)ncols;
    for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < nrows;
         r += (int64_t)gridDim.x * blockDim.x) {
        uint32_t deg = d_cnt[r];
        if (!deg) continue;
        const uint64_t basep = scan_pos(d_pre, bsums, chunk, r);
        if (basep >= cap) continue;  // overflow: flagged by k_scan_mid
        if (deg > 32) {
            ovf_push(d_state, ovf, r);
            continue;
        }
        if (basep + deg > cap) deg = (uint32_t)(cap - basep);
        sid_t row[NC];
#pragma unroll
        for (int c = 0; c < NC; c++) row[c] = tbl[r * NC + c];
        const sid_t *el = edges + d_eoff[r];
        sid_t *dst = out + (int64_t)basep * oc;
        uint32_t miss = 0;
        for (uint32_t k = 0; k < deg; k++) {
#pragma unroll
            for (int c = 0; c < NC; c++) dst[c] = row[c];
            sid_t v = el[k];
            dst[NC] = v;
            dst += oc;
            if (verify)
                miss += typeof_nodrop_ok(vtbm, v_type_of, v_type_base,
                                         v_type_n, v_cval, v) ? 0u : 1u;
        }
        if (miss)
            atomicAdd((unsigned long long *)&d_state[S_DONE],
                      (unsigned long long)miss);
    }
    // algorithmic bytes for the whole expansion (counted once; includes
    // the big-row pass): total*(edge 4 + write 4*oc) + nrows*(row 4*ncols
    // + cnt/pre/eoff 20)
    if (blockIdx.x == 0 && threadIdx.x == 0)
        atomicAdd((unsigned long long *)&d_stats[CAT_EXPAND],
                  (unsigned long long)(d_state[S_NROWS] * (4 + 4 * oc) +
                                       (uint64_t)nrows * (4 * ncols + 20)));
}

// big-fanout rows: one wave per queued row, lanes stride the edge list
// (coalesced writes: adjacent lanes write adjacent output rows)
template <int NC>
__global__ void k_expand_big(const sid_t *__restrict__ tbl, int ncols,
                             const sid_t *__restrict__ edges,
                             const uint64_t *__restrict__ d_eoff,
                             const uint32_t *__restrict__ d_cnt,
                             const uint64_t *__restrict__ d_pre,
                             const uint64_t *__restrict__ bsums, int G,
                             uint64_t *__restrict__ d_state, uint64_t cap,
                             const uint32_t *__restrict__ ovf,
                             const uint64_t *__restrict__ vtbm,
                             const uint16_t *__restrict__ v_type_of,
                             uint64_t v_type_base, uint64_t v_type_n,
                             sid_t v_cval, int verify,
                             sid_t *__restrict__ out)
{
    const int64_t nq = (int64_t)d_state[S_OVF];
    const int64_t nrows = (int64_t)d_state[S_INROWS];
    const int64_t chunk = (nrows + G - 1) / G;
    constexpr int oc = NC + 1;
    (void)ncols;
    const int lane = threadIdx.x & 63;
    const int64_t w0 = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const int64_t nw = ((int64_t)gridDim.x * blockDim.x) >> 6;
    for (int64_t q = w0; q < nq; q += nw) {
        const int64_t r = ovf[q];
        uint64_t deg = d_cnt[r];
        const uint64_t basep = scan_pos(d_pre, bsums, chunk, r);
        if (basep >= cap) continue;
        if (basep + deg > cap) deg = cap - basep;
        sid_t row[NC];
#pragma unroll
        for (int c = 0; c < NC; c++) row[c] = tbl[r * NC + c];
        const sid_t *el = edges + d_eoff[r];
        uint32_t miss = 0;
        for (uint64_t k = lane; k < deg; k += 64) {
            sid_t *dst = out + (int64_t)(basep + k) * oc;
#pragma unroll
            for (int c = 0; c < NC; c++) dst[c] = row[c];
            sid_t v = el[k];
            dst[NC] = v;
            if (verify)
                miss += typeof_nodrop_ok(vtbm, v_type_of, v_type_base,
                                         v_type_n, v_cval, v) ? 0u : 1u;
        }
        if (miss)
            atomicAdd((unsigned long long *)&d_state[S_DONE],
                      (unsigned long long)miss);
    }
}

// known_to_unknown over a FUNCTIONAL predicate (every key deg==1,
// rank-compressed map): the probe+scan+expand pipeline collapses into
// a page+value gather pair + compacted append, with an optional fused
// `?v rdf:type CONST` filter on the NEW column (plan pairs like Q1's
// ugDegreeFrom -> University).  Two phases: a 1:1 grid-stride GATHER
// (the measured-fast k_expand_fn_map shape — no barriers between the
// dependent page/value loads) writes each row's resolved object (0 =
// miss/filtered) to a scratch stream; the COMPACT phase then reads it
// SEQUENTIALLY with the block-aggregated scan.  The round-1 single-pass
// form interleaved the gathers with 16 scan barriers per tile and ran
// 4-5x slower than its own gather cost (169 vs 36 us on Q1's 6.4M-row
// step).  Multi-type (0xFFFF) falls back to a probe of [val|TYPE|OUT].
// Output rows <= input rows, so capacity can never overflow.
__global__ void k_fn_gather(const sid_t *__restrict__ tbl, int ncols,
                            const fnpage_t *__restrict__ fn_pg,
                            const sid_t *__restrict__ fn_vals,
                            uint64_t fn_base, uint64_t fn_n, int col,
                            int use_typeof, sid_t fcval,
                            const uint16_t *__restrict__ type_of,
                            const uint64_t *__restrict__ tbm,
                            uint64_t type_base, uint64_t type_n,
                            const vertex_t *__restrict__ verts,
                            const sid_t *__restrict__ edges,
                            uint64_t f_bstart, uint64_t f_nbuckets,
                            const uint64_t *__restrict__ d_state,
                            uint64_t *__restrict__ d_stats,
                            sid_t *__restrict__ d_val,
                            uint32_t *__restrict__ d_cnt)
{
    const int64_t nrows = (int64_t)d_state[S_NROWS];
    count_bytes(d_stats, CAT_EXPAND,
                (uint64_t)nrows * (24 + 4 + (use_typeof ? 2 : 0)));
    for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
         r < nrows; r += (int64_t)gridDim.x * blockDim.x) {
        sid_t v = tbl[r * ncols + col];
        sid_t tv = fn_lookup(fn_pg, fn_vals, fn_base, fn_n, v);
        if (tv && use_typeof) {
            const int tc =
                typeof_check(tbm, type_of, type_base, type_n, fcval, tv);
            if (tc == TC_MULTI) {
                uint64_t eo = 0, es = 0;
                probe_one(verts, f_bstart, f_nbuckets,
                          key_pack(tv, TYPE_ID, (uint64_t)DIR_OUT), eo, es);
                if (!(es && bsearch_u32(edges + eo, es, fcval))) tv = 0;
            } else if (tc == TC_NO) {
                tv = 0;
            }
        }
        d_val[r] = tv;
        d_cnt[r] = tv ? 1u : 0u;
    }
}

// OPTIMISTIC functional k2u: used ONLY inside captured graphs for
// steps whose warm pass dropped no rows (store is immutable, so the
// observation holds for replays; a miss at runtime counts into the
// sticky S_DONE word, k_publish_state turns it into S_ERR and the
// caller falls back to the safe path).  The row count is unchanged, so
// the step needs no commit; the 1:1 write needs no scan/compaction and
// coalesces perfectly.
template <int NC>
__global__ void k_expand_fn_map(const sid_t *__restrict__ tbl,
                                const fnpage_t *__restrict__ fn_pg,
                                const sid_t *__restrict__ fn_vals,
                                uint64_t fn_base, uint64_t fn_n, int col,
                                int use_typeof,
                                const uint64_t *__restrict__ tbm,
                                const uint16_t *__restrict__ type_of,
                                uint64_t type_base, uint64_t type_n,
                                sid_t fcval,
                                uint64_t *__restrict__ d_state,
                                uint64_t *__restrict__ d_stats,
                                sid_t *__restrict__ out)
{
    const int64_t nrows = (int64_t)d_state[S_NROWS];
    constexpr int oc = NC + 1;
    count_bytes(d_stats, CAT_EXPAND,
                (uint64_t)nrows * (24 + (use_typeof ? 1 : 0) + oc * 4));
    uint32_t miss = 0;
    for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
         r < nrows; r += (int64_t)gridDim.x * blockDim.x) {
        sid_t v = tbl[r * NC + col];
        sid_t tv = fn_lookup(fn_pg, fn_vals, fn_base, fn_n, v);
        bool ok = tv != 0;
        if (ok && use_typeof)  // multi-type counts as a miss -> fallback
            ok = typeof_nodrop_ok(tbm, type_of, type_base, type_n, fcval, tv);
        miss += ok ? 0u : 1u;
        sid_t *dst = out + r * oc;
#pragma unroll
        for (int c = 0; c < NC; c++) dst[c] = tbl[r * NC + c];
        dst[NC] = tv;
    }
    if (miss)
        atomicAdd((unsigned long long *)&d_state[S_DONE],
                  (unsigned long long)miss);
}
