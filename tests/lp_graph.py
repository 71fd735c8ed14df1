"""Synthetic graph for the LDS plan interpreter's edge tests (a helper
module, not a test).

`lp_graph(multi)` builds one small deterministic graph whose templates
put `k_plan_batch` on every edge of its micro-ops: first lists of 0, 1,
63, 64, 65 and 129 entries around the 64-lane loops, expansions from an
inner column and against the IN direction, binary searches that end on
the first and the last entry of lists of 1, 2, 32, 33 and 65, probes
that walk a collided bucket chain, segments without a bucket, a table
that is emptied mid-plan, and tables of exactly LP_CAP slots at three
and four columns.  `multi=False` leaves every entity with at most one
type (rdf:type compiles to LOP_TYPEOF); `multi=True` is the same graph
plus a second type on one entity (rdf:type compiles to LOP_K2C).

The interpreter returns counts only, so every template is built so that
a wrong column, a swapped pair of columns or a wrong row stride changes
the count; `WRONG` names those variants and `lp_ref` evaluates them like
the right ones.  `lp_ref` folds synth_graph.step_ref over a plan and
shares no code with the engine or the oracle.
"""
import numpy as np

from tests import synth_graph as sg
from tests.synth_graph import B, IN, OUT, TYPE, LP_CAP, step_ref

# predicates.  P_H is synth_graph's P_CHAIN so that its collision
# search (_chain_keys) serves this graph too.
P_A, P_B, P_C, P_D, P_U = 2, 3, 4, 5, 7
P_H = sg.P_CHAIN
P_K, P_N, P_E, P_F, P_G = 8, 9, 10, 11, 13
P_NONE = 12        # below the largest predicate id, no triple at all
P_PAST = 14        # above the largest predicate id
T_X, T_Y, T_M = 20, 21, 22

SIZES = [1, 63, 64, 65, 129]          # first-list lengths, plus two zeros
N_MID, N_LEAF = 129, 200
K_LENS = [1, 2, 32, 33, 65]           # P_K list lengths
K_MODES = ["first", "last", "absent"]
K_NOLIST = 17                         # mid[i], i % 17 == 16: no P_K list
ROWS3, ROWS4 = LP_CAP // 3, LP_CAP // 4

_NONE = np.empty(0, dtype=np.uint32)


def k_len(i):
    return K_LENS[i % 5]


def k_mode(i):
    return K_MODES[(i // 5) % 3]


def lp_graph(multi=False):
    """(triples, meta) of the single-typed or the multi-typed variant."""
    import wukong_amd as wk

    nxt = [B + 1024]          # [B+192, B+1024) is the chain-key zone

    def take(n):
        a = np.arange(nxt[0], nxt[0] + n, dtype=np.uint32)
        nxt[0] += n
        return a

    trip = []

    def add(s, p, o):
        s, o = np.broadcast_arrays(np.asarray(s, np.uint32),
                                   np.asarray(o, np.uint32))
        trip.append(np.stack([s.ravel(), np.full(s.size, p, np.uint32),
                              o.ravel()], axis=1))

    # vid order matters to the binary searches: fl < leaf < fh and
    # nl < nconst < nh.  mid[i] - leaf[i] is a multiple of 3, so that on
    # three partitions one rank owns both ends of a P_U edge.
    fl = take(70)
    leaf = take(N_LEAF)
    fh = take(71)
    nl, nconst, nh = take(5), int(take(1)[0]), take(5)
    mid = take(N_MID)
    src = take(8)
    multi_v = int(take(1)[0])
    absent = int(take(1)[0])           # in range, in no triple
    low_v = B - 1                      # below type_base: an index-range id

    j = np.arange(N_LEAF)
    add(leaf[j % 3 == 0], TYPE, T_X)
    add(leaf[j % 3 == 1], TYPE, T_Y)   # j % 3 == 2: untyped
    add(mid[::2], TYPE, T_M)
    add(multi_v, TYPE, T_Y)
    if multi:
        add(multi_v, TYPE, T_X)
    # leaves with a P_C list of their own: expanding from the wrong
    # column finds something, and something else
    add(leaf[::4], P_C, leaf[(np.arange(0, N_LEAF, 4) + 1) % N_LEAF])

    for i in range(N_MID):
        m = mid[i]
        add(m, P_B, leaf[(7 * i + np.arange(1 + i % 3)) % N_LEAF])
        add(m, P_C, leaf[(13 * i + np.arange(1 + 2 * (i % 2))) % N_LEAF])
        add(m, P_U, leaf[i])                       # functional
        if i % 4 != 3:                             # i % 4 == 3: no IN list
            add(src[i % 7], P_D, m)
        if i % 8 == 0:
            add(src[7], P_D, m)                    # IN list of two
        if i % K_NOLIST != K_NOLIST - 1:
            L, u = k_len(i), leaf[i]
            lst = {"first": [u] + list(fh[:L - 1]),
                   "last": list(fl[:L - 1]) + [u],
                   "absent": list(fl[:L // 2]) + list(fh[:L - L // 2])}
            add(m, P_K, lst[k_mode(i)])
        nlst = [[nconst] + list(nh), list(nl) + [nconst], list(nh), list(nl),
                list(nl) + list(nh), None][i % 6]
        if nlst is not None:
            add(m, P_N, nlst)

    # first lists of 1 .. 129 mids; SIZES[0] = 1 holds mid[0] only
    roots = take(len(SIZES))
    for r, n in zip(roots, SIZES):
        add(r, P_A, mid[:n])

    # collided P_H keys (22 in one bucket of 8: three hops, 16 in another:
    # two hops) and one vid of the long bucket that is no key: its probe
    # walks the whole chain and misses
    chain, b_long, b_mid = sg._chain_keys(wk.hash_u64, wk.key_pack)
    chain_miss = next(
        v for v in range(B + 192, B + 1024) if v not in chain and
        wk.hash_u64(wk.key_pack(v, P_H, OUT)) % sg.CHAIN_BUCKETS == b_long)
    for k, s in enumerate(chain):
        add(s, P_H, leaf[k:k + 1 + k % 3])
        add(s, P_B, leaf[k + 1])
    r_chain = int(take(1)[0])
    add(r_chain, P_A, list(chain) + [chain_miss])
    # k2c constant: first entry of the list of a key r_chain's owner owns
    chain_c = int(leaf[next(k for k, s in enumerate(chain)
                            if s % 3 == r_chain % 3)])

    # capacity: 32 (24) starts x 8 x 8 paths = 2048 (1536) rows of three
    # (four) columns = LP_CAP slots; ca[32] adds exactly one path
    ca, cb, cc = take(33), take(8), take(8)
    cb1, cd = int(take(1)[0]), int(take(1)[0])
    add(np.repeat(ca[:32], 8), P_E, np.tile(cb, 32))
    add(np.repeat(cb, 8), P_F, np.tile(cc, 8))
    add(ca[32], P_E, cb1)
    add(cb1, P_F, cc[0])
    add(cc, P_G, cd)
    add(cc, TYPE, T_X)
    cap = take(4)                      # 3-fit, 3-overflow, 4-fit, 4-overflow
    add(cap[0], P_A, ca[:32])
    add(cap[1], P_A, ca[:33])
    add(cap[2], P_A, ca[:24])
    add(cap[3], P_A, list(ca[:24]) + [ca[32]])

    # one path of the 8-op template whose every probed key shares the
    # owner (vid % 3) of the 65-entry root: a partition keeps it whole
    rho = int(roots[3]) % 3
    i8 = next(i for i in range(3, N_MID) if mid[i] % 3 == rho and
              i % 6 < 2 and i % 4 != 3 and i % 8 != 0)
    add(mid[i8], P_B, next(v for v in cc if v % 3 == rho))   # typed T_X
    add(mid[i8], P_C, next(v for v in leaf[::4] if v % 3 == rho))
    add(next(v for v in src if v % 3 == rho), P_D, mid[i8])

    # values of the rdf:type column: the last vid of the graph, a vid
    # below type_base and the entity with two types
    last_v = int(take(1)[0])
    add(last_v, TYPE, T_X)
    add(mid[0], P_B, last_v)
    add(mid[1], P_B, low_v)
    add(mid[2], P_B, multi_v)

    triples = np.unique(np.concatenate(trip).astype(np.uint32), axis=0)
    meta = dict(
        multi=bool(multi), max_id=last_v, last_v=last_v, low_v=low_v,
        multi_v=multi_v, absent=absent, leaf=leaf, mid=mid, fl=fl, fh=fh,
        nl=nl, nh=nh, nconst=nconst, src=src, roots=roots,
        nokey=int(leaf[0]),            # in the graph, no (P_A, OUT) key
        chain=np.array(chain, dtype=np.uint32), chain_miss=int(chain_miss),
        chain_long_bucket=b_long, chain_mid_bucket=b_mid, r_chain=r_chain,
        chain_c=chain_c,
        ca=ca, cb=cb, cc=cc, cb1=cb1, cd=cd, cap=cap)
    return triples, meta


def rc_consts(meta):
    """Constants whose first (P_A, OUT) list has 0, 0, 1, 63, 64, 65 and
    129 entries."""
    return [meta["nokey"], meta["absent"]] + [int(r) for r in meta["roots"]]


X, Y, Z, W_, V = -1, -2, -3, -4, -5


def templates(meta):
    """name -> (patterns, nvars, consts).  The first pattern's subject is
    replaced by each constant."""
    rc = rc_consts(meta)
    nc = meta["nconst"]
    r65, r1 = int(meta["roots"][3]), int(meta["roots"][0])
    r129 = int(meta["roots"][4])
    cap = [int(c) for c in meta["cap"]]
    rch = [meta["r_chain"]]
    a = (0, P_A, OUT, X)
    cap3 = [a, (X, P_E, OUT, Y), (Y, P_F, OUT, Z)]
    return {
        # ---- every op entered with 0 .. 129 rows
        "c2u": ([a], 1, rc),
        "k2u-last": ([a, (X, P_B, OUT, Y)], 2, rc),
        "k2u-col0": ([a, (X, P_B, OUT, Y), (X, P_C, OUT, Z)], 3, rc),
        "k2u-in": ([a, (X, P_U, OUT, Y), (X, P_D, IN, Z)], 3, rc),
        "k2k-lr": ([a, (X, P_U, OUT, Y), (X, P_K, OUT, Y)], 2, rc),
        "k2k-rl": ([a, (X, P_U, OUT, Y), (Y, P_K, IN, X)], 2, rc),
        "k2c-1col": ([a, (X, P_N, OUT, nc)], 1, rc),
        "k2c-3col": ([a, (X, P_B, OUT, Y), (X, P_C, OUT, Z),
                      (X, P_N, OUT, nc)], 3, rc),
        "type-1col": ([a, (X, TYPE, OUT, T_M)], 1, rc),
        "type-inner": ([a, (X, P_B, OUT, Y), (X, P_C, OUT, Z),
                        (Y, TYPE, OUT, T_X)], 3, rc),
        # ---- collided probes mid-plan
        "chain-k2u": ([a, (X, P_H, OUT, Y)], 2, rch),
        "chain-k2k": ([a, (X, P_B, OUT, Y), (X, P_H, OUT, Y)], 2, rch),
        "chain-k2c": ([a, (X, P_H, OUT, meta["chain_c"])], 1, rch),
        # ---- segments without a bucket
        "tin-c2u": ([(0, TYPE, IN, X)], 1, [int(meta["mid"][0]), r65]),
        "tin-k2u": ([a, (X, TYPE, IN, Y)], 2, [r65]),
        "tin-k2k": ([a, (X, P_U, OUT, Y), (X, TYPE, IN, Y)], 2, [r65]),
        "tin-k2c": ([a, (X, TYPE, IN, int(meta["leaf"][0]))], 1, [r65]),
        "none-c2u": ([(0, P_NONE, OUT, X)], 1, [r65]),
        "none-k2u": ([a, (X, P_NONE, OUT, Y)], 2, [r65]),
        "none-k2k": ([a, (X, P_U, OUT, Y), (X, P_NONE, OUT, Y)], 2, [r65]),
        "none-k2c": ([a, (X, P_NONE, OUT, int(meta["leaf"][0]))], 1, [r65]),
        "past-c2u": ([(0, P_PAST, OUT, X)], 1, [r65]),
        "past-k2u": ([a, (X, P_PAST, IN, Y)], 2, [r65]),
        # ---- a filter empties the table; a k2u and a k2k follow
        "emptied": ([a, (X, P_N, OUT, meta["absent"]), (X, P_U, OUT, Y),
                     (X, P_K, OUT, Y)], 2, [r65, r1]),
        # ---- capacity at three and four columns
        "cap3": (cap3, 3, cap[:2]),
        "cap4": (cap3 + [(Z, P_G, OUT, W_)], 4, cap[2:]),
        "cap3-k2k": (cap3 + [(Y, P_F, OUT, Z)], 3, cap[:2]),
        "cap3-k2c": (cap3 + [(Y, P_F, OUT, int(meta["cc"][0]))], 3, cap[:2]),
        "cap3-type": (cap3 + [(Z, TYPE, OUT, T_X)], 3, cap[:2]),
        # keeps the one row of ca[32]: far below the cap again
        "cap3-shrink": (cap3 + [(X, P_E, OUT, meta["cb1"])], 3, cap[:2]),
        # ---- 8 ops, 5 columns
        "eight": ([a, (X, P_B, OUT, Y), (Y, TYPE, OUT, T_X),
                   (X, P_C, OUT, Z), (X, P_D, IN, W_), (Z, P_C, OUT, V),
                   (W_, P_D, OUT, X), (X, P_N, OUT, nc)], 5,
                  [r129, r65, r1, meta["absent"]]),
    }


# (template, index of the constant) the interpreter must report as
# overflowing; nothing else may
OVERFLOWS = {("cap3", 1), ("cap4", 1), ("cap3-k2k", 1), ("cap3-k2c", 1),
             ("cap3-type", 1), ("cap3-shrink", 1)}

# deliberately wrong variants: template -> [(what, pattern index,
# replacement pattern)]; "stride" entries are evaluated by lp_ref's
# `restride` instead
WRONG = {
    "k2u-col0": [("subject column", 2, (Y, P_C, OUT, Z))],
    "k2u-in": [("subject column", 2, (Y, P_D, IN, Z))],
    "k2k-lr": [("swapped columns", 2, (Y, P_K, OUT, X))],
    "k2k-rl": [("swapped columns", 2, (X, P_K, IN, Y))],
    "k2c-3col": [("subject column", 3, (Y, P_N, OUT, None))],
    "type-inner": [("subject column", 3, (Z, TYPE, OUT, T_X)),
                   ("subject column", 3, (X, TYPE, OUT, T_X))],
    "chain-k2k": [("swapped columns", 2, (Y, P_H, OUT, X))],
}
# template -> index of the op that reads the table with a stride one
# column short
STRIDE = {"k2u-col0": 2, "k2u-in": 2, "k2k-lr": 2, "k2k-rl": 2,
          "k2c-3col": 3, "type-inner": 3}


def wrong_patterns(patterns, idx, repl):
    pats = list(patterns)
    s, p, d, o = repl
    pats[idx] = (s, p, d, patterns[idx][3] if o is None else o)
    return pats


def lp_ref(adj, patterns, const, restride=None):
    """(count, overflows) of a plan whose first subject is `const`, by
    folding step_ref over `adj` (c2u = the adjacency list itself).  The
    overflow rule is the interpreter's: the first list holds more than
    LP_CAP entries, or the table right after some k2u holds more than
    LP_CAP values (rows * columns), whatever later filters remove.

    `restride=i` models an op i that reads its input with a stride one
    column short: value (r, c) comes from flat[r * (ncols - 1) + c]."""
    _, p, d, o = patterns[0]
    first = adj.get((int(const), p, d), _NONE)
    ovf = len(first) > LP_CAP
    table = first.reshape(-1, 1).astype(np.uint32)
    cols = {o: 0}
    for i, (s, p, d, o) in enumerate(patterns[1:], start=1):
        col = cols[s]
        if restride == i:
            n, nc = table.shape
            flat = table.ravel()
            idx = np.arange(n)[:, None] * (nc - 1) + np.arange(nc)[None, :]
            table = flat[idx] if n else table
        if o >= 0:
            table = step_ref(table, col, adj, "k2c", p, d, const=o)
        elif o in cols:
            table = step_ref(table, col, adj, "k2k", p, d, col2=cols[o])
        else:
            table = step_ref(table, col, adj, "k2u", p, d)
            cols[o] = table.shape[1] - 1
            if table.shape[0] * table.shape[1] > LP_CAP:
                ovf = True
    return int(table.shape[0]), ovf


def owned(adj, rank, W):
    """The adjacency partition `rank` of W holds: the lists of the keys
    whose vertex it owns (vid % W)."""
    return {k: v for k, v in adj.items() if k[0] % W == rank}
