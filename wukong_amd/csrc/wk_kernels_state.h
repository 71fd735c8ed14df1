// wk_kernels_state.h — the 1-thread d_state kernels (commit, set, begin,
// publish), the projection and k_zero_words.  commit_rows and begin_state
// themselves live in wk_kernels_common.h.
// Included by gpu_engine.hip only (one translation unit).
#pragma once

// advance: commit S_TOTAL, the cursor the step's kernels appended at
// (commit_rows).  Stays a 1-thread kernel: a commit fused into the last
// finishing block of a wide producer bumps one done-word per block, which
// serializes at ~88 atomics/us and costs more than this launch
// (k_peer_step, a single block, commits inline; so does k_scan_mid).
__global__ void k_commit(uint64_t *__restrict__ d_state, uint64_t cap) {
    commit_rows(d_state, d_state[S_TOTAL], cap, /*snapshot_inrows*/ false);
}

__global__ void k_set_state(uint64_t *__restrict__ d_state, uint64_t nrows) {
    d_state[S_NROWS] = nrows;
    d_state[S_TOTAL] = 0;
    d_state[S_OVF] = 0;
}

// query begin fused with the first state write — one launch instead of
// k_zero_words + k_set_state
__global__ void k_begin_state(uint64_t *__restrict__ d_state, uint64_t nrows) {
    begin_state(d_state, nrows);
}

// device projection to required-var columns (sparql.hpp:1510-1536)
struct cols8 { int32_t c[8]; };
__global__ void k_project(const sid_t *__restrict__ tbl, int ncols,
                          const uint64_t *__restrict__ d_state, cols8 cols,
                          int rc, sid_t *__restrict__ out)
{
    const int64_t n = (int64_t)d_state[S_NROWS];
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < n * rc;
         t += (int64_t)gridDim.x * blockDim.x) {
        int64_t i = t / rc;
        int j = (int)(t - i * rc);
        int c = cols.c[j];
        out[t] = (c >= 0) ? tbl[i * ncols + c] : (sid_t)0xFFFFFFFFu;
    }
}

// The optimistic kernels of a captured plan (k_expand_fn_map, the
// verify-only k_filter_tpr, the verify-fused k_expand_in/_big) count
// their guard misses into S_DONE, which nothing clears during a query;
// the conversion to S_ERR happens ONCE, here, before the words are
// copied out.  expect_empty (captured plans with a truncated empty
// tail): the skipped patterns are only valid on an empty table, so any
// row left raises S_ERR the same way.
__device__ __forceinline__ void publish_state(uint64_t *__restrict__ d_state,
                                              const uint64_t *__restrict__ d_stats,
                                              uint64_t *__restrict__ h_pin,
                                              int expect_empty) {
    if (d_state[S_DONE] || (expect_empty && d_state[S_NROWS])) {
        d_state[S_ERR] = 1;
        d_state[S_REQ] = max(d_state[S_REQ], d_state[S_NROWS]);
    }
    for (int i = 0; i < S_WORDS; i++) h_pin[i] = d_state[i];
    for (int i = 0; i < CAT_COUNT; i++) h_pin[HP_STATS + i] = d_stats[i];
    // sticky error flag: survives across back-to-back graph replays
    // whose own begin kernels clear d_state — the one-sync-per-pass path
    // checks and clears it host-side
    if (d_state[S_ERR]) h_pin[HP_STICKY_ERR] = 1;
}
__global__ void k_publish_state(uint64_t *__restrict__ d_state,
                                const uint64_t *__restrict__ d_stats,
                                uint64_t *__restrict__ h_pin,
                                int expect_empty) {
    publish_state(d_state, d_stats, h_pin, expect_empty);
}

// Suite captures: query i's publish followed by query i+1's begin, the
// same writes in the same order from one thread — one launch for two
// 
__global__ void k_publish_begin(uint64_t *__restrict__ d_state,
                                const uint64_t *__restrict__ d_stats,
                                uint64_t *__restrict__ h_pin,
                                int expect_empty, uint64_t nrows) {
    publish_state(d_state, d_stats, h_pin, expect_empty);
    begin_state(d_state, nrows);
}

__global__ void k_zero_words(uint64_t *p, int n) {
    for (int i = threadIdx.x; i < n; i += blockDim.x) p[i] = 0;
}
