// wk_chain_sched.h — round schedule of a per-row op chain.
// Plain C++ with no HIP dependency: the engine (gpu_engine.hip) and a
// host-only test program include the same code.
#pragma once
#include <cstdint>

enum { CH_FN_APPEND = 0,  // v = fn[row[a]]; 0 drops, else append v
       CH_TYPE = 1,       // bitmap bit of row[a] (exact, multi-type incl.)
       CH_FN_EQ = 2,      // fn[row[a]] != 0 && == row[b]   (k2k)
       CH_EQ = 3 };       // row[a] == cval                 (PM_EQ k2c)
constexpr int CHAIN_MAX = 8;  // ops per chain
// ops of one dependency round, evaluated side by side by chain_eval_batch.
// 2: Q1's rounds are {append, append}, {TYPE, FN_EQ}, {TYPE} and Q7's one
// round is {TYPE, FN_EQ}; a third slot would add K x 4 live VGPRs to every
// round for a round that the early-out skips on almost every wave.
constexpr int CHAIN_SLOTS = 2;

struct chain_sched_op {
    int32_t kind, a, b;  // b is read by CH_FN_EQ only
};
struct chain_sched {
    int32_t nrounds;
    int32_t slot[CHAIN_MAX][CHAIN_SLOTS];  // op index, -1 = empty
    int32_t dst[CHAIN_MAX];  // CH_FN_APPEND: destination column, else -1
    int32_t round_of[CHAIN_MAX];
    int32_t early_out;  // a wave without a live candidate leaves the loop
};

// Greedy list scheduling in plan order.  An op depends on an earlier op
// only if it reads (as `a`, or as `b` of an FN_EQ) the column that op
// appends: keep/drop is a pure conjunction and nothing exits early, so no
// other ordering exists.  Op i goes to the first round after all of its
// producers that has a free slot; round i is still empty when op i is
// placed, so nrounds <= nops.  The k-th FN_APPEND in plan order writes
// column nc_in + k whatever round it lands in, which keeps the widened
// row's layout.  packed = false: one op per round in plan order, no
// early-out (the evaluation order of a plain op loop).
inline void chain_schedule(const chain_sched_op *ops, int nops, int nc_in,
                           bool packed, chain_sched &S) {
    S.nrounds = 0;
    S.early_out = packed ? 1 : 0;
    int fill[CHAIN_MAX];
    for (int r = 0; r < CHAIN_MAX; r++) {
        fill[r] = 0;
        S.dst[r] = S.round_of[r] = -1;
        for (int s = 0; s < CHAIN_SLOTS; s++) S.slot[r][s] = -1;
    }
    int nc = nc_in;
    for (int i = 0; i < nops && i < CHAIN_MAX; i++) {
        int r = 0;
        if (!packed) {
            r = i;
        } else {
            for (int j = 0; j < i; j++) {
                if (ops[j].kind != CH_FN_APPEND) continue;
                const bool reads =
                    ops[i].a == S.dst[j] ||
                    (ops[i].kind == CH_FN_EQ && ops[i].b == S.dst[j]);
                if (reads && S.round_of[j] + 1 > r) r = S.round_of[j] + 1;
            }
            while (fill[r] == CHAIN_SLOTS) r++;
        }
        S.slot[r][fill[r]++] = i;
        S.round_of[i] = r;
        if (ops[i].kind == CH_FN_APPEND) S.dst[i] = nc++;
        if (r + 1 > S.nrounds) S.nrounds = r + 1;
    }
}
