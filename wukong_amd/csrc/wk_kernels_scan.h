// wk_kernels_scan.h — wave / block scan helpers, the chunked scan kernels
// (k_scan_local, k_scan_mid and their WK_SCAN=0 ladder siblings) and what
// the writers behind them share: scan_pos and the big-row queue push.
// Included by gpu_engine.hip only (one translation unit).
#pragma once

// inclusive scan of one u64 per lane across the 64-lane wave (6 cross-
// lane steps, no LDS, no barrier)
__device__ __forceinline__ uint64_t wave_incl_scan(uint64_t v, int lane) {
#pragma unroll
    for (int ofs = 1; ofs < 64; ofs <<= 1) {
        const uint64_t t = __shfl_up((unsigned long long)v, ofs);
        if (lane >= ofs) v += t;
    }
    return v;
}

// Block-wide exclusive offset of this thread's `tsum` among the SCAN_T
// threads, plus the block total: wave scan in registers, the SCAN_T/64
// wave totals through LDS, ONE barrier.  s_wtot is the caller's
// [2][SCAN_T/64] ping-pong (`par` = tile parity), which is what makes a
// single barrier per tile enough: a wave can only reach the tile that
// rewrites a slot after passing the barrier of the tile in between,
// i.e. after every wave has read that slot.
__device__ __forceinline__ uint64_t block_excl_scan(uint64_t tsum,
                                                    uint64_t (*s_wtot)[SCAN_T / 64],
                                                    int par, uint64_t *total) {
    static_assert(SCAN_T == 256, "four wave totals");
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const uint64_t incl = wave_incl_scan(tsum, lane);
    if (lane == 63) s_wtot[par][wid] = incl;
    __syncthreads();
    const uint64_t w0 = s_wtot[par][0], w1 = s_wtot[par][1],
                   w2 = s_wtot[par][2], w3 = s_wtot[par][3];
    const uint64_t wbase = (wid > 0 ? w0 : 0) + (wid > 1 ? w1 : 0) +
                           (wid > 2 ? w2 : 0);
    *total = w0 + w1 + w2 + w3;
    return wbase + incl - tsum;
}

// The Hillis-Steele ladder: inclusive scan of one value per thread of the
// SCAN_T-thread block through LDS (owns its sh[SCAN_T]; ~18 barriers).
// Returns the thread's inclusive value, *total = the block's sum; the
// closing barrier lets the next call rewrite sh.  Used by the kernels that
// scan once per 256-row tile next to far heavier probes (k_probe_scan,
// k_expand_opt, k_peer_step) and by the WK_SCAN=0 scan kernels.
__device__ __forceinline__ uint64_t block_ladder_scan(uint64_t v,
                                                      uint64_t *total) {
    __shared__ uint64_t sh[SCAN_T];
    sh[threadIdx.x] = v;
    __syncthreads();
    for (int ofs = 1; ofs < SCAN_T; ofs <<= 1) {
        uint64_t x = (threadIdx.x >= (unsigned)ofs) ? sh[threadIdx.x - ofs] : 0;
        __syncthreads();
        sh[threadIdx.x] += x;
        __syncthreads();
    }
    const uint64_t incl = sh[threadIdx.x];
    *total = sh[SCAN_T - 1];
    __syncthreads();
    return incl;
}

// What the scan pipeline leaves for its writers: d_pre[r] is row r's
// exclusive prefix inside its chunk (chunk = ceil(nrows / G) consecutive
// rows per scan block), bsums[] the exclusive prefix of the chunk sums.
__device__ __forceinline__ uint64_t scan_pos(const uint64_t *__restrict__ d_pre,
                                             const uint64_t *__restrict__ bsums,
                                             int64_t chunk, int64_t r) {
    return d_pre[r] + bsums[r / chunk];
}

// queue input row r (more than 32 edges) for the one-wave-per-row pass
// that follows the thread-per-row writer; S_OVF is the queue length
__device__ __forceinline__ void ovf_push(uint64_t *__restrict__ d_state,
                                         uint32_t *__restrict__ ovf, int64_t r) {
    const unsigned long long i =
        atomicAdd((unsigned long long *)&d_state[S_OVF], 1ull);
    ovf[i] = (uint32_t)r;
}

// One wave emits one queued row: its `len` edges el[0..len) in chunks of
// 64, lane l takes edge k0 + l into row[NC] and asks pred(row) (which may
// append further columns); a passing lane's rank among the chunk's passing
// lanes (ballot) plus the passing count of the earlier chunks is its
// offset from basep.  Writes the first oc columns of row; never at or
// past cap.  All 64 lanes call it with the same arguments but row.
template <int NC, int W, class Pred>
__device__ __forceinline__ void wave_emit_rows(sid_t (&row)[W],
                                               const sid_t *__restrict__ el,
                                               uint32_t len, uint64_t basep,
                                               uint64_t cap, int oc,
                                               sid_t *__restrict__ out,
                                               Pred pred) {
    static_assert(NC < W, "the edge value needs a column");
    const int lane = threadIdx.x & 63;
    uint64_t wbase = 0;  // passing-rank base across 64-edge chunks
    for (uint32_t k0 = 0; k0 < len; k0 += 64) {
        const uint32_t k = k0 + lane;
        bool pass = false;
        if (k < len) {
            row[NC] = el[k];
            pass = pred(row);
        }
        const uint64_t mask = __ballot(pass);
        if (pass) {
            const uint64_t pos = basep + wbase + lanes_below(mask, lane);
            if (pos < cap) {
                sid_t *dst = out + (int64_t)pos * oc;
#pragma unroll
                for (int c = 0; c < W; c++)
                    if (c < oc) dst[c] = row[c];
            }
        }
        wbase += (uint64_t)__popcll(mask);
    }
}

// chunked exclusive prefix of d_cnt -> d_pre + per-chunk sums (same
// chunk math as k_probe_scan so the expansion kernels are unchanged).
// Each thread owns SCAN_PER consecutive rows and sums them in registers;
// one barrier per SCAN_T*SCAN_PER-row tile (block_excl_scan).
constexpr int SCAN_PER = 4;
__global__ void __launch_bounds__(SCAN_T)
k_scan_local(const uint32_t *__restrict__ d_cnt,
             const uint64_t *__restrict__ d_state,
             uint64_t *__restrict__ d_pre, uint64_t *__restrict__ bsums)
{
    const int64_t nrows = (int64_t)d_state[S_NROWS];
    const int G = gridDim.x;
    const int64_t chunk = (nrows + G - 1) / G;
    const int64_t start = (int64_t)blockIdx.x * chunk;
    const int64_t end = min(start + chunk, (int64_t)nrows);
    __shared__ uint64_t s_wtot[2][SCAN_T / 64];
    uint64_t carry = 0;
    int par = 0;
    for (int64_t base = start; base < end;
         base += SCAN_T * SCAN_PER, par ^= 1) {
        const int64_t r0 = base + (int64_t)threadIdx.x * SCAN_PER;
        const uint32_t c0 = (r0 < end) ? d_cnt[r0] : 0u;
        const uint32_t c1 = (r0 + 1 < end) ? d_cnt[r0 + 1] : 0u;
        const uint32_t c2 = (r0 + 2 < end) ? d_cnt[r0 + 2] : 0u;
        const uint32_t c3 = (r0 + 3 < end) ? d_cnt[r0 + 3] : 0u;
        uint64_t total;
        uint64_t pre = carry + block_excl_scan((uint64_t)c0 + c1 + c2 + c3,
                                               s_wtot, par, &total);
        if (r0 < end) d_pre[r0] = pre;
        pre += c0;
        if (r0 + 1 < end) d_pre[r0 + 1] = pre;
        pre += c1;
        if (r0 + 2 < end) d_pre[r0 + 2] = pre;
        pre += c2;
        if (r0 + 3 < end) d_pre[r0 + 3] = pre;
        carry += total;
    }
    if (threadIdx.x == 0) bsums[blockIdx.x] = (start < end) ? carry : 0;
}

// WK_SCAN=0: the previous Hillis-Steele ladders (one element per thread
// in LDS, block_ladder_scan), kept so the rewrite can be timed alone.
// Same arguments, launch shape and outputs.
__global__ void k_scan_local_ladder(const uint32_t *__restrict__ d_cnt,
                                    const uint64_t *__restrict__ d_state,
                                    uint64_t *__restrict__ d_pre,
                                    uint64_t *__restrict__ bsums)
{
    const int64_t nrows = (int64_t)d_state[S_NROWS];
    const int G = gridDim.x;
    const int64_t chunk = (nrows + G - 1) / G;
    const int64_t start = (int64_t)blockIdx.x * chunk;
    const int64_t end = min(start + chunk, (int64_t)nrows);
    uint64_t carry = 0;
    for (int64_t base = start; base < end; base += SCAN_T) {
        const int64_t r = base + threadIdx.x;
        const uint64_t esz = (r < end) ? d_cnt[r] : 0;
        uint64_t total;
        const uint64_t incl = block_ladder_scan(esz, &total);
        if (r < end) d_pre[r] = carry + incl - esz;
        carry += total;
    }
    if (threadIdx.x == 0) bsums[blockIdx.x] = (start < end) ? carry : 0;
}

// finish the scan across blocks: exclusive over the G block sums
// (single block), then the step commit with the S_INROWS snapshot
// (commit_rows): the pipeline total is known here, the writers that
// follow read the INPUT row count from S_INROWS, and S_OVF (the big-row
// queue they are about to fill) starts clean — no separate 1-thread
// commit launch per k2u/fn step.
// Each thread owns per = ceil(G/SCAN_T) (at most SCAN_MID_PER)
// consecutive sums in registers; one barrier per tile (block_excl_scan).
// scan_grid caps G at SCAN_T*SCAN_MID_PER, so the tile loop runs once.
constexpr int SCAN_MID_PER = 8;
__global__ void __launch_bounds__(SCAN_T)
k_scan_mid(uint64_t *__restrict__ bsums, int G, uint64_t cap,
           uint64_t *__restrict__ d_state)
{
    __shared__ uint64_t s_wtot[2][SCAN_T / 64];
    const int per = min((G + SCAN_T - 1) / SCAN_T, SCAN_MID_PER);
    uint64_t carry = 0;
    int par = 0;
    for (int base = 0; base < G; base += SCAN_T * per, par ^= 1) {
        const int i0 = base + (int)threadIdx.x * per;
        uint64_t v[SCAN_MID_PER];  // fully unrolled: stays in registers
        uint64_t tsum = 0;
#pragma unroll
        for (int k = 0; k < SCAN_MID_PER; k++) {
            v[k] = (k < per && i0 + k < G) ? bsums[i0 + k] : 0;
            tsum += v[k];
        }
        uint64_t total;
        uint64_t pre = carry + block_excl_scan(tsum, s_wtot, par, &total);
#pragma unroll
        for (int k = 0; k < SCAN_MID_PER; k++) {
            if (k < per && i0 + k < G) bsums[i0 + k] = pre;
            pre += v[k];
        }
        carry += total;
    }
    if (threadIdx.x == 0)
        commit_rows(d_state, carry, cap, /*snapshot_inrows*/ true);
}

// WK_SCAN=0 sibling of k_scan_mid (see k_scan_local_ladder): the same
// sums and the same commit
__global__ void k_scan_mid_ladder(uint64_t *__restrict__ bsums, int G,
                                  uint64_t cap, uint64_t *__restrict__ d_state)
{
    uint64_t carry = 0;
    for (int base = 0; base < G; base += SCAN_T) {
        const int i = base + threadIdx.x;
        const uint64_t x = (i < G) ? bsums[i] : 0;
        uint64_t total;
        const uint64_t incl = block_ladder_scan(x, &total);
        if (i < G) bsums[i] = carry + incl - x;
        carry += total;
    }
    if (threadIdx.x == 0)
        commit_rows(d_state, carry, cap, /*snapshot_inrows*/ true);
}
