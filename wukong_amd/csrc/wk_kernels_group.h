// wk_kernels_group.h — UNION / OPTIONAL groups as part of the launch chain:
// the parent-table snapshot, the branch restart and the branch append
// (DESIGN.md §3 5l).
// Included by gpu_engine.hip only (one translation unit).
#pragma once

// Group state, the words behind the byte counters of the d_state block:
// the row count of the table the UNION started from, and the rows the
// branches appended so far.  G_MERGED is NOT clamped to the capacity, so
// that S_REQ ends up as the whole union's demand in one overflowing run;
// every use as an offset clamps it.
enum { G_PARENT = 0, G_MERGED = 1, G_WORDS = 2 };

constexpr int GRP_UNROLL = 4;  // independent 16-B loads in flight per lane

// Streaming copy of `nw` 4-byte words, the whole grid: a scalar head up to
// the destination's 16-B boundary, 16 B per lane from there (GRP_UNROLL
// loads issued before the first store), a scalar tail.  When source and
// destination differ in their offset within 16 B (a table view into the
// store's edge array starts on any word, an append on any row), the body
// keeps the aligned 16-B store and reads its four words one by one.  No
// LDS, no atomics; nw == 0 touches no memory.
__device__ __forceinline__ void grp_copy_words(const sid_t *__restrict__ src,
                                               sid_t *__restrict__ dst,
                                               uint64_t nw) {
    const uint64_t tid = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t nthr = (uint64_t)gridDim.x * blockDim.x;
    uint64_t head = ((16 - ((uintptr_t)dst & 15)) & 15) >> 2;
    if (head > nw) head = nw;
    const uint64_t nvec = (nw - head) >> 2;
    const uint64_t tail0 = head + (nvec << 2);
    if (tid < head) dst[tid] = src[tid];
    if (tid < nw - tail0) dst[tail0 + tid] = src[tail0 + tid];
    const sid_t *s = src + head;
    uint4 *d4 = reinterpret_cast<uint4 *>(dst + head);
    if ((((uintptr_t)s) & 15) == 0) {
        const uint4 *s4 = reinterpret_cast<const uint4 *>(s);
        uint64_t i = tid;
        for (; i + (GRP_UNROLL - 1) * nthr < nvec; i += GRP_UNROLL * nthr) {
            uint4 v[GRP_UNROLL];
#pragma unroll
            for (int k = 0; k < GRP_UNROLL; k++) v[k] = s4[i + k * nthr];
#pragma unroll
            for (int k = 0; k < GRP_UNROLL; k++) d4[i + k * nthr] = v[k];
        }
        for (; i < nvec; i += nthr) d4[i] = s4[i];
    } else {
        for (uint64_t i = tid; i < nvec; i += nthr) {
            const sid_t *p = s + (i << 2);
            d4[i] = make_uint4(p[0], p[1], p[2], p[3]);
        }
    }
}

// Copy the current table (S_NROWS x ncols words at src, possibly a view
// into the store) to dst.  record = 1, the UNION's snapshot: also note the
// parent row count and open an empty merged table.  record = 0: the copy
// alone (the merged table on its way into a table buffer).  S_NROWS is
// only read here, so the one thread that records races with nobody.
__global__ void __launch_bounds__(SCAN_T)
k_grp_copy(const sid_t *__restrict__ src, sid_t *__restrict__ dst, int ncols,
           uint64_t cap, int record, const uint64_t *__restrict__ d_state,
           uint64_t *__restrict__ d_grp, uint64_t *__restrict__ d_stats)
{
    const uint64_t n = min(d_state[S_NROWS], cap);
    const uint64_t nw = dst ? n * (uint64_t)ncols : 0;
    count_bytes(d_stats, CAT_COPY, nw * 8);
    if (record && blockIdx.x == 0 && threadIdx.x == 0) {
        d_grp[G_PARENT] = n;
        d_grp[G_MERGED] = 0;
    }
    grp_copy_words(src, dst, nw);
}

// Append the current table (a finished branch) to the merged table at row
// G_MERGED.  Rows past the capacity are dropped and flagged (S_ERR, S_REQ
// = the rows the union needs so far); nothing is written past cap rows.
// G_MERGED itself moves in the 1-thread k_grp_restart that follows: every
// block of this launch reads the same value.
__global__ void __launch_bounds__(SCAN_T)
k_grp_append(const sid_t *__restrict__ src, sid_t *__restrict__ merged,
             int ncols, uint64_t cap, uint64_t *__restrict__ d_state,
             const uint64_t *__restrict__ d_grp,
             uint64_t *__restrict__ d_stats)
{
    const uint64_t n = min(d_state[S_NROWS], cap);
    const uint64_t at = d_grp[G_MERGED];
    const uint64_t off = min(at, cap);
    const uint64_t fit = min(n, cap - off);
    if (at + n > cap && blockIdx.x == 0 && threadIdx.x == 0) {
        // S_ERR / S_REQ are read by no block of this launch
        d_state[S_ERR] = 1;
        d_state[S_REQ] = max(d_state[S_REQ], at + n);
    }
    count_bytes(d_stats, CAT_COPY, fit * (uint64_t)ncols * 8);
    grp_copy_words(src, merged + off * (uint64_t)ncols, fit * (uint64_t)ncols);
}

// One thread, between two branches (last = 0) or behind the last one
// (last = 1): commit the rows the append just copied, then make the
// parent (last = 0) or the merged table (last = 1) the current row count.
// S_TOTAL and S_OVF go to 0 and S_ERR, S_REQ and S_DONE stay, as in
// k_set_state.
__global__ void k_grp_restart(uint64_t *__restrict__ d_state,
                              uint64_t *__restrict__ d_grp, uint64_t cap,
                              int last) {
    const uint64_t m = d_grp[G_MERGED] + min(d_state[S_NROWS], cap);
    d_grp[G_MERGED] = m;
    d_state[S_NROWS] = last ? min(m, cap) : d_grp[G_PARENT];
    d_state[S_TOTAL] = 0;
    d_state[S_OVF] = 0;
}
