"""Synthetic edge-case graph for the operator-level tests (a helper
module, not a test).

`edge_graph()` builds one small deterministic graph that puts a row on
every hard threshold of the engine's kernels: the 32/64-edge row
classes of the expansion kernels, both sides of the `edges / keys <= 32`
type-fused CSR gate, rank-page edges of the functional maps, 2- and
3-hop cluster-hash chains, single/multi/untyped entities and the LDS
plan interpreter's capacity.  `step_ref()` is a plain numpy/dict
reference of one operator that shares no code with the engine or the
oracle, and `env()` sets WK_* variables for a block.
"""
import contextlib
import os

import numpy as np

B = 1 << 17          # first vertex id
IN, OUT = 0, 1
TYPE = 1
P_DEG, P_HUB, P_FN, P_RFN, P_CHAIN, P_LP = 2, 3, 4, 5, 6, 7
# entity types; T_N1.. only select the start sets of the whole plans
T_A, T_B, T_C = 10, 11, 12
T_N1, T_N2, T_OD = 13, 14, 15     # no-drop / no-drop+multi-typed / one-drop
T_F1, T_F2, T_F3 = 16, 17, 18     # P_FN: no-drop / dropping / no-drop+multi

LADDER = [1, 2, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1000]
HUB_DEG = 5000
FN_IDX = [0, 62, 63, 64, 65, 127, 128]   # span indexes of the P_FN keys
LP_CAP = 6144                            # LDS plan interpreter slots
N_CHAIN, CHAIN_BUCKETS = 40, 8           # (40 + 4) / 5 == 8 buckets
CHAIN_LONG, CHAIN_MID = 22, 16           # keys per collided bucket


@contextlib.contextmanager
def env(**kv):
    """Set environment variables (values are str()-ed) for a block and
    restore the previous state afterwards."""
    old = {k: os.environ.get(k) for k in kv}
    os.environ.update({k: str(v) for k, v in kv.items()})
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _chain_keys(hash_u64, key_pack):
    """40 subject vids for P_CHAIN: 22 hashing to one bucket of 8, 16 to
    a second, 2 elsewhere — found by scanning candidate vids."""
    by_bucket = {}
    for v in range(B + 192, B + 1024):
        b = hash_u64(key_pack(v, P_CHAIN, OUT)) % CHAIN_BUCKETS
        by_bucket.setdefault(b, []).append(v)
    keys = by_bucket[0][:CHAIN_LONG] + by_bucket[1][:CHAIN_MID]
    keys += by_bucket[2][:1] + by_bucket[3][:1]
    assert len(keys) == N_CHAIN
    return sorted(keys), 0, 1


def edge_graph():
    """(triples, meta): the uint32 (n,3) graph and the names of its
    vertices, predicates and types."""
    import wukong_amd as wk

    nxt = [B + 1024]   # [B, B+192): P_FN zone; [B+192, B+1024): chain zone

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

    # object pools.  pool: mixed types by index (0: T_A, 1: T_A+T_B,
    # 2: untyped, 3..6: T_B); nb: single-typed T_B; multi/bad: one
    # T_A+T_B entity and one T_A-only entity for the no-drop variants
    pool = take(HUB_DEG)
    nb = take(256)
    multi, bad = int(take(1)[0]), int(take(1)[0])
    i = np.arange(HUB_DEG)
    add(pool[(i % 7 == 0) | (i % 7 == 1)], TYPE, T_A)
    add(pool[(i % 7 == 1) | (i % 7 >= 3)], TYPE, T_B)
    add(nb, TYPE, T_B)
    add([multi, multi, bad], TYPE, [T_A, T_B, T_A])

    # P_DEG / P_HUB ladder (type T_A): degree d -> the first d pool
    # vertices for P_DEG, the last d for P_HUB
    ladder = take(len(LADDER) + 1)
    degs = LADDER + [HUB_DEG]
    for s, d in zip(ladder, degs):
        add(s, P_DEG, pool[:d])
        add(s, P_HUB, pool[HUB_DEG - d:])
    add(ladder, TYPE, T_A)

    # start sets of the whole plans: (type, degrees, extra object)
    groups = {}
    for t, gd, extra in ((T_N1, [1, 33, 65, 200], None),
                         (T_N2, [2, 40, 70], multi),
                         (T_OD, [3, 34, 66], bad)):
        subj = take(len(gd))
        for k, (s, d) in enumerate(zip(subj, gd)):
            objs = nb[k:k + d]
            if extra is not None and k == 1:   # lands in the deg > 32 row
                objs = np.append(objs[:-1], np.uint32(extra))
            add(s, P_DEG, objs)
            add(s, P_HUB, objs)
        add(subj, TYPE, t)
        groups[t] = subj

    # P_DEG filler (type T_C): degree 1/2 subjects so that P_DEG stays
    # eligible for the type-fused CSR path (edges / keys <= 32)
    filler = take(6000)
    add(filler, P_DEG, pool[np.arange(6000) % HUB_DEG])
    add(filler[1::2], P_DEG, pool[(2 * np.arange(3000) + 2) % HUB_DEG])
    add(filler, TYPE, T_C)

    # P_CHAIN: collided subject keys, 1..3 objects each
    chain, b_long, b_mid = _chain_keys(wk.hash_u64, wk.key_pack)
    for k, s in enumerate(chain):
        add(s, P_CHAIN, nb[k:k + 1 + k % 3])

    # P_RFN: functional in the IN direction only
    rfn_s, rfn_o = take(3), take(6)
    add(rfn_s[[0, 0, 0, 1, 2, 2]], P_RFN, rfn_o)

    # P_LP: constants with LP_CAP-1 / LP_CAP / LP_CAP+1 edges, and two
    # c2u->k2u roots whose second-level tables hold LP_CAP/2 and
    # LP_CAP/2+1 rows
    lpo = take(LP_CAP + 1)
    j = np.arange(LP_CAP + 1)
    add(lpo[(j % 5 == 0) | (j % 5 == 1)], TYPE, T_A)
    add(lpo[(j % 5 == 1) | (j % 5 >= 3)], TYPE, T_B)
    lp_c = take(3)
    for c, n in zip(lp_c, (LP_CAP - 1, LP_CAP, LP_CAP + 1)):
        add(c, P_LP, lpo[:n])
    lp_m = take(3)
    for m, n in zip(lp_m, (3000, LP_CAP // 2 - 3000, LP_CAP // 2 - 2999)):
        add(m, P_LP, lpo[100:100 + n])
    lp_d = take(2)
    add(lp_d[0], P_LP, lp_m[[0, 1]])
    add(lp_d[1], P_LP, lp_m[[0, 2]])

    # P_FN: strictly functional OUT; keys on the rank-page edges plus
    # the last vid of the graph.  fn[2] and fn[3] share an object, so
    # (P_FN, IN) is not functional.
    max_id = nxt[0]
    fn = np.array([B + k for k in FN_IDX] + [max_id], dtype=np.uint32)
    fn_o = np.array([nb[0], nb[1], nb[2], nb[2], bad, multi, nb[3], nb[4]],
                    dtype=np.uint32)
    add(fn, P_FN, fn_o)
    add(fn[:4], TYPE, T_F1)                       # objects all T_B
    add(np.append(fn[4:], np.uint32(B + 1)), TYPE, T_F2)   # B+1: no P_FN
    add(fn[[1, 5]], TYPE, T_F3)                   # fn[5] -> multi-typed

    triples = np.concatenate(trip).astype(np.uint32)
    meta = dict(
        max_id=int(max_id), pool=pool, nb=nb, multi=multi, bad=bad,
        ladder=ladder, ladder_degs=degs, groups=groups, filler=filler,
        chain=np.array(chain, dtype=np.uint32), chain_long_bucket=b_long,
        chain_mid_bucket=b_mid, rfn_s=rfn_s, rfn_o=rfn_o, lpo=lpo,
        lp_c=lp_c, lp_m=lp_m, lp_d=lp_d, fn=fn, fn_o=fn_o,
        fn_gaps=np.array([B + 1, B + 61, B + 66, B + 126, B + 129],
                         dtype=np.uint32),
        absent=B + 191,                 # in range, no triple at all
        sub_base=[5, B - 1], past_max=int(max_id) + 1)
    return triples, meta


GATE_W, GATE_RANK, N_GATE = 8, 2, 8


def gate_graph():
    """edge_graph() plus N_GATE subjects (type T_A) with one P_HUB edge
    each, all owned by rank GATE_RANK of GATE_W partitions.  On that
    partition (P_HUB, OUT) drops to `edges / keys <= 32` while the full
    store and the other partitions stay above: the gate of the
    type-fused CSR path decides differently on one rank."""
    triples, meta = edge_graph()
    first = meta["past_max"]
    first += (GATE_RANK - first) % GATE_W
    subj = (first + GATE_W * np.arange(N_GATE)).astype(np.uint32)
    obj = meta["pool"][HUB_DEG - 1]
    extra = np.array([[s, P_HUB, obj] for s in subj] +
                     [[s, TYPE, T_A] for s in subj], dtype=np.uint32)
    meta = dict(meta, gate_s=subj, max_id=int(subj[-1]),
                past_max=int(subj[-1]) + 1)
    return np.concatenate([triples, extra]), meta


def adjacency(triples):
    """{(vid, pid, dir): sorted uint32 array of neighbours}, straight
    from the triples (type triples have no IN lists: types are index
    ids, not vertices)."""
    adj = {}
    for s, p, o in np.unique(triples, axis=0).tolist():
        adj.setdefault((s, p, OUT), []).append(o)
        if p != TYPE:
            adj.setdefault((o, p, IN), []).append(s)
    return {k: np.array(sorted(v), dtype=np.uint32) for k, v in adj.items()}


_NONE = np.empty(0, dtype=np.uint32)


def step_ref(table, col, adj, mode, pid, d, col2=None, const=None):
    """One operator over an in-memory table.  mode 'k2u' appends every
    (pid, d) neighbour of table[:, col]; 'k2k' keeps the rows whose
    table[:, col2] is such a neighbour; 'k2c' keeps the rows that have
    `const` as one (the rdf:type const filter is k2c with pid=TYPE)."""
    table = np.asarray(table, dtype=np.uint32)
    # the start values repeat: look each distinct one up once
    uniq, inv = np.unique(table[:, col], return_inverse=True)
    lists = [adj.get((int(v), pid, d), _NONE) for v in uniq]
    inv = inv.ravel().tolist()
    if mode == "k2u":
        cnt = np.array([len(x) for x in lists], dtype=np.int64)[inv]
        new = np.concatenate([lists[j] for j in inv] + [_NONE])
        return np.column_stack([np.repeat(table, cnt, axis=0),
                                new.astype(np.uint32)])
    if mode == "k2k":
        tgt = table[:, col2].tolist()
    else:
        assert mode == "k2c"
        tgt = [int(const)] * len(table)
    sets = [set(x.tolist()) for x in lists]
    keep = np.array([t in sets[j] for t, j in zip(tgt, inv)], dtype=bool)
    return table[keep] if len(table) else table
