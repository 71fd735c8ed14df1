// wk_kernels_final.h — device final ops: DISTINCT (stable LSD radix sort of a row-index permutation + adjacent dedup), OFFSET/LIMIT window, projection.
// Included by gpu_engine.hip only (one translation unit).
#pragma once

// Final ops on the device (final_process, sparql.hpp:1424-1551; the host
// restatement is finalize_result in gpu_engine.hip and stays the A/B arm).
//
// DISTINCT = full-row lexicographic sort, unsigned, column 0 most
// significant, then drop every row equal to its sorted predecessor on the
// required columns.  Only whole rows move, so any STABLE multi-key sort
// gives the host's output bit for bit.  The sort is an LSD radix sort of a
// u32 row-index permutation: last column first, four 8-bit digits per
// column, each digit pass = k_fin_hist (per-block LDS histogram over a
// contiguous row range) -> k_fin_scan (ONE block: digit-major exclusive
// scan of the block x digit matrix) -> k_fin_scatter (stable: equal digits
// are ranked by position with wave ballots, waves are ordered through
// per-wave digit counts in LDS, tiles through running bases in LDS — no
// atomics hand out slots).  The table itself is never moved or written:
// keys are read through the permutation, and the last pass (k_fin_emit)
// reads the kept rows through it and writes the projected window.
//
// Every kernel is launched over a grid fixed by the row CAPACITY and reads
// the row count from d_state, so the same chain runs inside a captured
// graph.  Pass skipping is decided on the device: k_fin_live ORs
// x ^ x[0] per column into d_fin[F_LIVE + c]; a digit pass whose 8 bits
// are constant over the table returns at once in all three kernels, and
// the ping-pong parity of a pass is the number of live passes before it.
// Correctness does not depend on the skip (a constant digit permutes
// nothing under a stable sort).

// d_fin words: [0..7] per-column live-bit masks, [8] post-final row count
enum { F_LIVE = 0, F_COUNT = 8, F_WORDS = 16 };
// (the pinned slots the final publish writes, HP_FIN_COUNT and
// HP_FIN_LIVE, are named with the others in wk_kernels_common.h)
constexpr int FIN_MAXB = 1024;   // blocks of the histogram/scatter grid
constexpr int FIN_SCAN_T = 1024; // threads of the one scan block

struct fin_tbl {
    const sid_t *tbl;          // current table (may be a store view)
    int ncols;
    const uint64_t *d_state;   // S_NROWS
    uint64_t cap_rows;
    uint64_t *d_fin;
    uint32_t *idx[2];          // ping-pong row-index permutation
};

__device__ __forceinline__ uint64_t fin_rows(const fin_tbl &T) {
    const uint64_t n = T.d_state[S_NROWS];
    return n < T.cap_rows ? n : T.cap_rows;
}
// rows per block: contiguous ranges, a multiple of the 256-row tile
__device__ __forceinline__ uint64_t fin_per(uint64_t n, int G) {
    const uint64_t per = (n + G - 1) / G;
    return (per + SCAN_T - 1) / SCAN_T * SCAN_T;
}
// bit q of the result = digit pass q is live (pass q: column
// C-1-q/4, bits [8*(q%4), +8)) — LSD order
__device__ __forceinline__ uint32_t fin_live_passes(const fin_tbl &T) {
    uint32_t lv = 0;
    for (int c = 0; c < T.ncols && c < 8; c++) {
        const uint32_t m = (uint32_t)T.d_fin[F_LIVE + c];
        const int q0 = 4 * (T.ncols - 1 - c);
#pragma unroll
        for (int k = 0; k < 4; k++)
            if ((m >> (8 * k)) & 0xFFu) lv |= 1u << (q0 + k);
    }
    return lv;
}
struct fin_pass {
    bool live, first;  // first live pass reads the identity permutation
    int src;           // idx[src] -> idx[src ^ 1]
    int col, shift;
};
__device__ __forceinline__ fin_pass fin_decode(const fin_tbl &T, int p) {
    const uint32_t lv = fin_live_passes(T);
    const int before = __popc(lv & ((1u << p) - 1u));
    fin_pass d;
    d.live = (lv >> p) & 1u;
    d.first = before == 0;
    d.src = before & 1;
    d.col = T.ncols - 1 - (p >> 2);
    d.shift = 8 * (p & 3);
    return d;
}

// per-column OR of x ^ x[0]: which key bits vary over the table
__global__ __launch_bounds__(SCAN_T)
void k_fin_live(fin_tbl T)
{
    const uint64_t n = fin_rows(T);
    if (n == 0) return;
    const int C = T.ncols;
    uint32_t acc[8];
    uint32_t x0[8];
#pragma unroll
    for (int c = 0; c < 8; c++) {
        acc[c] = 0;
        x0[c] = c < C ? T.tbl[c] : 0;
    }
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
         i += (uint64_t)gridDim.x * blockDim.x) {
        const sid_t *r = T.tbl + i * C;
#pragma unroll
        for (int c = 0; c < 8; c++)
            if (c < C) acc[c] |= r[c] ^ x0[c];
    }
#pragma unroll
    for (int c = 0; c < 8; c++) {
        uint32_t v = acc[c];
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) v |= __shfl_xor(v, off);
        if ((threadIdx.x & 63) == 0 && v)
            atomicOr((unsigned long long *)&T.d_fin[F_LIVE + c],
                     (unsigned long long)v);
    }
}

// digit pass p, phase 1: per-block digit histogram of its row range
__global__ __launch_bounds__(SCAN_T)
void k_fin_hist(fin_tbl T, int p, uint32_t *__restrict__ hist)
{
    __shared__ unsigned int s_h[256];
    const fin_pass d = fin_decode(T, p);
    if (!d.live) return;
    const uint64_t n = fin_rows(T);
    const uint64_t per = fin_per(n, gridDim.x);
    const uint64_t lo = (uint64_t)blockIdx.x * per;
    if (lo >= n) return;
    const uint64_t hi = min(n, lo + per);
    s_h[threadIdx.x] = 0;
    __syncthreads();
    const uint32_t *src = T.idx[d.src];
    for (uint64_t i = lo + threadIdx.x; i < hi; i += SCAN_T) {
        const uint64_t row = d.first ? i : (uint64_t)src[i];
        const sid_t key = T.tbl[row * T.ncols + d.col];
        atomicAdd(&s_h[(key >> d.shift) & 255u], 1u);
    }
    __syncthreads();
    hist[(size_t)blockIdx.x * 256 + threadIdx.x] = s_h[threadIdx.x];
}

// phase 2: ONE block of 1024 threads; exclusive scan of the
// (block x digit) matrix in digit-major order, in place.  Thread
// (g, d) owns a quarter of the blocks of digit d.
__global__ __launch_bounds__(FIN_SCAN_T)
void k_fin_scan(fin_tbl T, int p, uint32_t *__restrict__ hist, int G)
{
    __shared__ unsigned int s_part[4][256];
    __shared__ unsigned int s_dig[256];
    const fin_pass dp = fin_decode(T, p);
    if (!dp.live) return;
    const uint64_t n = fin_rows(T);
    const uint64_t per = fin_per(n, G);
    const int nact = per ? (int)((n + per - 1) / per) : 0;  // blocks with rows
    const int d = threadIdx.x & 255, g = threadIdx.x >> 8;
    const int q = (nact + 3) / 4;
    const int b0 = min(g * q, nact), b1 = min(b0 + q, nact);
    unsigned int sum = 0;
    for (int b = b0; b < b1; b++) sum += hist[(size_t)b * 256 + d];
    s_part[g][d] = sum;
    __syncthreads();
    unsigned int tot = 0;
    if (g == 0) {
        tot = s_part[0][d] + s_part[1][d] + s_part[2][d] + s_part[3][d];
        s_dig[d] = tot;
    }
    __syncthreads();
    for (int off = 1; off < 256; off <<= 1) {  // inclusive scan over digits
        unsigned int v = 0;
        if (g == 0 && d >= off) v = s_dig[d - off];
        __syncthreads();
        if (g == 0) s_dig[d] += v;
        __syncthreads();
    }
    if (g == 0) s_dig[d] -= tot;  // exclusive
    __syncthreads();
    unsigned int run = s_dig[d];
    for (int gg = 0; gg < g; gg++) run += s_part[gg][d];
    for (int b = b0; b < b1; b++) {
        const unsigned int v = hist[(size_t)b * 256 + d];
        hist[(size_t)b * 256 + d] = run;
        run += v;
    }
}

// phase 3: STABLE scatter.  Per 256-row tile: a lane's rank among the
// equal digits of its wave comes from 8 ballots, the waves before it from
// s_w, the tiles before it from the running s_base.
__global__ __launch_bounds__(SCAN_T)
void k_fin_scatter(fin_tbl T, int p, const uint32_t *__restrict__ hist)
{
    __shared__ unsigned int s_base[256];
    __shared__ unsigned int s_w[4][256];
    const fin_pass d = fin_decode(T, p);
    if (!d.live) return;
    const uint64_t n = fin_rows(T);
    const uint64_t per = fin_per(n, gridDim.x);
    const uint64_t lo = (uint64_t)blockIdx.x * per;
    if (lo >= n) return;
    const uint64_t hi = min(n, lo + per);
    const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
    s_base[tid] = hist[(size_t)blockIdx.x * 256 + tid];
#pragma unroll
    for (int k = 0; k < 4; k++) s_w[k][tid] = 0;
    __syncthreads();
    const uint32_t *src = T.idx[d.src];
    uint32_t *dst = T.idx[d.src ^ 1];
    for (uint64_t t0 = lo; t0 < hi; t0 += SCAN_T) {
        const uint64_t i = t0 + tid;
        const bool valid = i < hi;
        uint32_t row = 0;
        uint32_t dig = 0;
        if (valid) {
            row = d.first ? (uint32_t)i : src[i];
            dig = (T.tbl[(uint64_t)row * T.ncols + d.col] >> d.shift) & 255u;
        }
        unsigned long long m = __ballot(valid);
#pragma unroll
        for (int k = 0; k < 8; k++) {
            const bool bit = (dig >> k) & 1u;
            const unsigned long long b = __ballot(bit);
            m &= bit ? b : ~b;
        }
        const int rank = __popcll(m & ((1ull << lane) - 1ull));
        if (valid && rank == 0) s_w[w][dig] = (unsigned int)__popcll(m);
        __syncthreads();
        if (valid) {
            unsigned int pos = s_base[dig] + (unsigned int)rank;
            for (int k = 0; k < w; k++) pos += s_w[k][dig];
            if (pos < n) dst[pos] = row;
        }
        __syncthreads();
        s_base[tid] += s_w[0][tid] + s_w[1][tid] + s_w[2][tid] + s_w[3][tid];
#pragma unroll
        for (int k = 0; k < 4; k++) s_w[k][tid] = 0;
        __syncthreads();
    }
}

// required columns of the dedup / projection (-1 = the var has no column)
struct fin_emit {
    cols8 cols;
    int rc;            // nrequired (<= 8)
    uint64_t offset;   // rows dropped in front
    uint64_t limit;    // ~0 = none
    sid_t *out;        // owned buffer, cap_rows x cap_cols words
};

// sorted position i -> table row (identity when no digit pass was live)
__device__ __forceinline__ const uint32_t *fin_perm(const fin_tbl &T) {
    const uint32_t lv = fin_live_passes(T);
    return lv ? T.idx[__popc(lv) & 1] : nullptr;
}

// DISTINCT flags: keep[i] = row i differs from its sorted predecessor on
// a required column; per-block kept counts for the emit pass
__global__ __launch_bounds__(SCAN_T)
void k_fin_flag(fin_tbl T, fin_emit E, uint32_t *__restrict__ keep,
                uint32_t *__restrict__ bcnt)
{
    __shared__ unsigned int s_cnt;
    const uint64_t n = fin_rows(T);
    const uint64_t per = fin_per(n, gridDim.x);
    const uint64_t lo = (uint64_t)blockIdx.x * per;
    const uint64_t hi = min(n, lo + per);
    if (threadIdx.x == 0) s_cnt = 0;
    __syncthreads();
    const uint32_t *perm = fin_perm(T);
    unsigned int mine = 0;
    for (uint64_t i = lo + threadIdx.x; i < hi; i += SCAN_T) {
        uint32_t k = 1;
        if (i > 0) {
            const uint64_t r1 = perm ? perm[i] : i;
            const uint64_t r0 = perm ? perm[i - 1] : i - 1;
            const sid_t *a = T.tbl + r1 * T.ncols;
            const sid_t *b = T.tbl + r0 * T.ncols;
            k = 0;
#pragma unroll
            for (int j = 0; j < 8; j++) {
                const int c = E.cols.c[j];
                if (j < E.rc && c >= 0 && a[c] != b[c]) k = 1;
            }
        }
        keep[i] = k;
        mine += k;
    }
    if (mine) atomicAdd(&s_cnt, mine);
    __syncthreads();
    if (threadIdx.x == 0) bcnt[blockIdx.x] = s_cnt;
}

// order-preserving compaction of the kept rows, cut to the OFFSET/LIMIT
// window and projected in the same pass; block 0 writes the final count
__global__ __launch_bounds__(SCAN_T)
void k_fin_emit(fin_tbl T, fin_emit E, const uint32_t *__restrict__ keep,
                const uint32_t *__restrict__ bcnt)
{
    __shared__ unsigned long long s_acc[2];
    __shared__ unsigned int s_wv[4];
    const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
    if (tid < 2) s_acc[tid] = 0;
    __syncthreads();
    {
        unsigned long long before = 0, all = 0;
        for (int b = tid; b < (int)gridDim.x; b += SCAN_T) {
            const unsigned int v = bcnt[b];
            all += v;
            if (b < (int)blockIdx.x) before += v;
        }
        if (before) atomicAdd(&s_acc[0], before);
        if (all) atomicAdd(&s_acc[1], all);
    }
    __syncthreads();
    uint64_t run = s_acc[0];
    if (blockIdx.x == 0 && tid == 0) {
        const uint64_t tot = s_acc[1];
        const uint64_t left = tot > E.offset ? tot - E.offset : 0;
        T.d_fin[F_COUNT] = left < E.limit ? left : E.limit;
    }
    const uint64_t n = fin_rows(T);
    const uint64_t per = fin_per(n, gridDim.x);
    const uint64_t lo = (uint64_t)blockIdx.x * per;
    if (lo >= n) return;
    const uint64_t hi = min(n, lo + per);
    const uint32_t *perm = fin_perm(T);
    for (uint64_t t0 = lo; t0 < hi; t0 += SCAN_T) {
        const uint64_t i = t0 + tid;
        const bool k = i < hi && keep[i];
        const unsigned long long m = __ballot(k);
        if (lane == 0) s_wv[w] = (unsigned int)__popcll(m);
        __syncthreads();
        uint64_t pos = run + __popcll(m & ((1ull << lane) - 1ull));
        for (int j = 0; j < w; j++) pos += s_wv[j];
        const unsigned int tile = s_wv[0] + s_wv[1] + s_wv[2] + s_wv[3];
        if (k && pos >= E.offset && pos - E.offset < E.limit) {
            const uint64_t row = perm ? perm[i] : i;
            const sid_t *r = T.tbl + row * T.ncols;
            sid_t *o = E.out + (pos - E.offset) * E.rc;
#pragma unroll
            for (int j = 0; j < 8; j++) {
                const int c = E.cols.c[j];
                if (j < E.rc) o[j] = c >= 0 ? r[c] : (sid_t)0xFFFFFFFFu;
            }
        }
        run += tile;
        __syncthreads();
    }
}

// OFFSET/LIMIT without DISTINCT: the window of the table in its current
// order, projected (k_project with a row window)
__global__ __launch_bounds__(SCAN_T)
void k_fin_window(fin_tbl T, fin_emit E)
{
    const uint64_t n = fin_rows(T);
    const uint64_t left = n > E.offset ? n - E.offset : 0;
    const uint64_t cnt = left < E.limit ? left : E.limit;
    if (blockIdx.x == 0 && threadIdx.x == 0) T.d_fin[F_COUNT] = cnt;
    const uint64_t words = cnt * E.rc;
    for (uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; t < words;
         t += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t i = t / E.rc;
        const int j = (int)(t - i * E.rc);
        const int c = E.cols.c[j];
        E.out[t] = c >= 0 ? T.tbl[(E.offset + i) * T.ncols + c]
                          : (sid_t)0xFFFFFFFFu;
    }
}

// sibling of k_publish_state: the post-final row count and the live-bit
// masks go to pinned memory
__global__ void k_fin_publish(const uint64_t *__restrict__ d_fin,
                              uint64_t *__restrict__ h_pin)
{
    h_pin[HP_FIN_COUNT] = d_fin[F_COUNT];
#pragma unroll
    for (int c = 0; c < 8; c++) h_pin[HP_FIN_LIVE + c] = d_fin[F_LIVE + c];
}
