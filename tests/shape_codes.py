"""Generated codes for the kernel shapes and row structures no committed
matrix plans (tests/test_shape_plans.py pins the plan of each on the CPU,
tests/test_gpu_shapes.py decodes them against the oracle).

One deterministic builder per case; nothing here reads a file.  The regular
codes come from Q.regular_code, the irregular ones from a seeded generator
through Q.HMatrix.from_check_nodes.  A builder's result is cached: the
matrices are read-only.
"""
import functools

import numpy as np

import qkd_ldpc_v_amd as Q


def with_rows(H, extra_rows, at=None):
    """H with extra_rows (lists of bit ids, [] = an empty check) inserted
    before row `at`, or appended."""
    rows = H.check_nodes
    at = len(rows) if at is None else at
    return Q.HMatrix.from_check_nodes(H.n, rows[:at] + [sorted(r) for r in extra_rows] + rows[at:])


def random_code(n, m, dvs, seed):
    """Every bit draws its degree from dvs and that many distinct rows; row
    degrees fall where they fall (checked: 2..31 edges, so a row a case adds
    is the longest and the shortest)."""
    rng = np.random.default_rng(seed)
    rows = [[] for _ in range(m)]
    for b in range(n):
        for r in rng.choice(m, size=int(rng.choice(dvs)), replace=False):
            rows[int(r)].append(b)
    assert min(len(r) for r in rows) >= 2 and max(len(r) for r in rows) <= 31
    return Q.HMatrix.from_check_nodes(n, rows)


def without_bits(H, fraction, seed):
    """H with a random `fraction` of its bits isolated: taken out of every row
    that keeps at least two edges (so a few of them keep an edge)."""
    rng = np.random.default_rng(seed)
    drop = set(rng.choice(H.n, size=int(round(H.n * fraction)), replace=False).tolist())
    rows = []
    for r in H.check_nodes:
        keep = list(r)
        for b in r:
            if b in drop and len(keep) > 2:
                keep.remove(b)
        rows.append(keep)
    return Q.HMatrix.from_check_nodes(H.n, rows)


@functools.lru_cache(maxsize=None)
def reg44():  # C2's size, other edges: 44 register slots, epl 41
    return Q.regular_code(10240, 2201, 4, 1)


@functools.lru_cache(maxsize=None)
def reg44_full():  # the same shape with every slot of the fullest lane used (epl 44)
    return Q.regular_code(11000, 2400, 4, 1)


@functools.lru_cache(maxsize=None)
def hybrid_dv4_lds():  # 44 + 20 slots, dv_max 4: no high-degree stage, rows in LDS
    return Q.regular_code(11264, 2400, 4, 1)


@functools.lru_cache(maxsize=None)
def hybrid_dv4_global():  # the same with part of the min-sum row aggregates in global scratch
    return Q.regular_code(14000, 3000, 4, 1)


@functools.lru_cache(maxsize=None)
def split_k4():  # 4 parts of 8 waves, no scratch slots
    return Q.regular_code(20480, 4096, 3, 1)


@functools.lru_cache(maxsize=None)
def split_k2_w8():  # 2 parts of 8 waves, 12 scratch slots
    return Q.regular_code(14000, 7000, 3, 1)


@functools.lru_cache(maxsize=None)
def split_k2_w16():  # 2 parts of 16 waves, 12 scratch slots
    return Q.regular_code(30000, 6000, 3, 1)


@functools.lru_cache(maxsize=None)
def long_split():
    """2 parts of 16 waves at an odd n >= 32768: the smallest split shape whose
    one-workgroup-per-frame kernels (parties, blind, select, estimate) launch
    1024 threads, with a partial last key word, wave ballot and code byte
    (row degrees 15..16)."""
    return Q.regular_code(33001, 6600, 3, 1)


@functools.lru_cache(maxsize=None)
def base_2000x400():
    return random_code(2000, 400, [2, 3], 3)


@functools.lru_cache(maxsize=None)
def base_2000x300():
    return random_code(2000, 300, [2, 3], 5)


@functools.lru_cache(maxsize=None)
def degree1_rows():  # two checks of a single bit each
    return with_rows(base_2000x400(), [[5], [77]])


@functools.lru_cache(maxsize=None)
def short_rows(n=4096, m=4000, seed=6):
    """Every bit of degree 2, rows of 1..8 edges (socket model: the row
    sockets are shuffled and dealt two per bit; a bit that drew one row twice
    swaps a socket with another bit)."""
    rng = np.random.default_rng(seed)
    deg = np.ones(m, np.int64)
    while deg.sum() < 2 * n:
        j = int(rng.integers(m))
        if deg[j] < 8:
            deg[j] += 1
    sockets = rng.permutation(np.repeat(np.arange(m, dtype=np.int64), deg)).reshape(n, 2)
    for b in np.nonzero(sockets[:, 0] == sockets[:, 1])[0]:
        while True:
            c = int(rng.integers(n))
            if c != b and sockets[b, 0] not in sockets[c]:
                sockets[b, 1], sockets[c, 1] = sockets[c, 1], sockets[b, 1]
                break
    rows = [[] for _ in range(m)]
    for b in range(n):
        for r in sockets[b]:
            rows[int(r)].append(b)
    assert all(1 <= len(r) <= 8 and len(set(r)) == len(r) for r in rows)
    return Q.HMatrix.from_check_nodes(n, rows)


@functools.lru_cache(maxsize=None)
def row_starts_32():
    """Lanes that start 32 rows, the most a lane's 32-bit syndrome mask holds:
    a 32-edge row sets 32 slots per lane, and 400 consecutive one-edge rows
    (after a chain of 1500 two-edge rows) fill eleven lanes of the second
    wave with 32 row starts each."""
    return Q.HMatrix.from_check_nodes(2048, [list(range(32))] + [[i, i + 1] for i in range(1500)] +
                                      [[b] for b in range(1500, 1900)])


@functools.lru_cache(maxsize=None)
def long_row(dc):  # one row of dc edges: 32 is the V2 limit, beyond it v1 decodes
    return with_rows(base_2000x300(), [list(range(dc))])


@functools.lru_cache(maxsize=None)
def degree300_bit():  # bit 0 in 300 two-edge rows; bits 301..399 isolated
    return Q.HMatrix.from_check_nodes(400, [[0, i + 1] for i in range(300)])


@functools.lru_cache(maxsize=None)
def degree510_bit():  # the largest bit degree accepted, beside a chain of two-edge rows
    return Q.HMatrix.from_check_nodes(1200, [[0, i + 1] for i in range(510)] +
                                      [[600 + i, 601 + i] for i in range(500)])


@functools.lru_cache(maxsize=None)
def empty_row(at):  # base_2000x400 with one empty check before row `at` (400: appended)
    return with_rows(base_2000x400(), [[]], at=at)


@functools.lru_cache(maxsize=None)
def reg44_isolated():  # (reg44_full: 1 % fewer edges of reg44 fit 40 slots)
    return without_bits(reg44_full(), 0.01, 7)


@functools.lru_cache(maxsize=None)
def split_k4_isolated():
    return without_bits(split_k4(), 0.01, 8)


def _plan(variant, lanes, epl, split, debug=None):
    """The plan a case is meant to reach: Graph.plan()'s variant, lanes and
    edges_per_lane, Graph.split_plan(), and (V2 only) the fields of the
    {"plan": ...} diagnostic line: waves, slots_reg, slots_scratch,
    rows_global_ms, split_k."""
    keys = ("waves", "slots_reg", "slots_scratch", "rows_global_ms", "split_k")
    return {"variant": variant, "lanes": lanes, "edges_per_lane": epl,
            "split": dict(zip(("parts", "part_lanes", "scratch_slots"), split)),
            "debug": None if debug is None else dict(zip(keys, debug))}


# case -> builder (the c1 / c2 fixture cases with a forced wave count are built by the tests)
CODES = {
    "reg44": reg44, "reg44_full": reg44_full, "hybrid_dv4_lds": hybrid_dv4_lds,
    "hybrid_dv4_global": hybrid_dv4_global, "split_k4": split_k4, "split_k2_w8": split_k2_w8,
    "split_k2_w16": split_k2_w16, "long_split": long_split, "degree1_rows": degree1_rows, "short_rows": short_rows,
    "row_starts_32": row_starts_32,
    "long_row32": lambda: long_row(32), "long_row33": lambda: long_row(33), "long_row40": lambda: long_row(40),
    "long_row41": lambda: long_row(41), "degree300_bit": degree300_bit, "degree510_bit": degree510_bit,
    "empty_row_first": lambda: empty_row(0), "empty_row_last": lambda: empty_row(400),
    "reg44_isolated": reg44_isolated, "split_k4_isolated": split_k4_isolated,
}

# Recorded from the planner as it stood when these tests were written.  A
# planner change that moves a case re-records it here only together with a new
# case that reaches the shape the old one covered.
PLANS = {
    "reg44": _plan("v2", 1024, 41, (1, 1024, 0), (16, 44, 0, 0, 1)),
    "reg44_full": _plan("v2", 1024, 44, (1, 1024, 0), (16, 44, 0, 0, 1)),
    "hybrid_dv4_lds": _plan("v2_hybrid", 1024, 45, (1, 1024, 20), (16, 44, 20, 0, 1)),
    "hybrid_dv4_global": _plan("v2_hybrid", 1024, 60, (1, 1024, 20), (16, 44, 20, 1, 1)),
    "split_k4": _plan("v2_split", 2048, 30, (4, 512, 0), (64, 40, 0, 0, 4)),
    "split_k2_w8": _plan("v2_split", 1024, 42, (2, 512, 12), (32, 40, 12, 0, 2)),
    "split_k2_w16": _plan("v2_split", 2048, 45, (2, 1024, 12), (32, 40, 12, 0, 2)),
    "long_split": _plan("v2_split", 2048, 49, (2, 1024, 12), (32, 40, 12, 0, 2)),
    "degree1_rows": _plan("v2", 256, 24, (1, 256, 0), (4, 40, 0, 0, 1)),
    "short_rows": _plan("v2", 1024, 8, (1, 1024, 0), (16, 40, 0, 0, 1)),
    "row_starts_32": _plan("v2", 128, 32, (1, 128, 0), (2, 40, 0, 0, 1)),
    "long_row32": _plan("v2", 192, 32, (1, 192, 0), (3, 40, 0, 0, 1)),
    "long_row33": _plan("reg_lds", 128, 40, (1, 128, 0)),
    "long_row40": _plan("reg_lds", 128, 40, (1, 128, 0)),
    "long_row41": _plan("glb_lds", 640, 41, (1, 640, 0)),
    "degree300_bit": _plan("v2", 320, 2, (1, 320, 0), (5, 40, 0, 0, 1)),
    "degree510_bit": _plan("v2", 1024, 2, (1, 1024, 0), (16, 40, 0, 0, 1)),
    "empty_row_first": _plan("reg_lds", 128, 40, (1, 128, 0)),
    "empty_row_last": _plan("reg_lds", 128, 40, (1, 128, 0)),
    "reg44_isolated": _plan("v2", 1024, 43, (1, 1024, 0), (16, 44, 0, 0, 1)),
    "split_k4_isolated": _plan("v2_split", 1536, 40, (3, 512, 0), (48, 40, 0, 0, 3)),
    # committed fixtures under QLDPC_V2_WAVES (read when the graph is created)
    "c2_w12": _plan("v2", 768, 54, (1, 768, 0), (12, 56, 0, 0, 1)),
    "c1_w2": _plan("v2", 128, 40, (1, 128, 0), (2, 40, 0, 0, 1)),
    "c1_w3": _plan("v2", 192, 27, (1, 192, 0), (3, 40, 0, 0, 1)),
}
KNOBS = {"c2_w12": {"QLDPC_V2_WAVES": "12"}, "c1_w2": {"QLDPC_V2_WAVES": "2"}, "c1_w3": {"QLDPC_V2_WAVES": "3"}}


def assert_plan(g, case, algorithm=0):
    """The part of PLANS[case] a graph reports itself (device graphs too)."""
    want = PLANS[case]
    plan = g.plan(0, algorithm)
    got = {k: plan[k] for k in ("variant", "lanes", "edges_per_lane")}
    assert got == {k: want[k] for k in got}, (case, plan)
    assert g.split_plan() == want["split"], (case, g.split_plan())
