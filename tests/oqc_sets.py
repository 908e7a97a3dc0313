"""The directed inputs of the post-filter tests, shared by the CPU tier (tests/test_oqc_model.py: model == oqc_core.h, coverage reachable) and the GPU tier
(tests/test_gpu_oqc_edges.py: device == model): the same calls and seeds, imported by both.  A set is a list of (label, clumps) -- one entry per read of the batch, in
batch order; `qlens` are the lengths of the reads the lists are injected for (the golden r1k.fa: 1 kbp reads), `seqs` the sequence table."""
import numpy as np

import oqc_model as om

# the filter's parameter sets (command-line arguments of the session) and, per set, the environment hooks of the device stage
PARAM_SETS = {
    "defaults": [],
    "fbs_loose": ["-FBS", "Y", "-PSS", "0.1", "-PRL", "0.1"],
    "fbs_tight": ["-FBS", "Y", "-PSS", "0.99", "-PRL", "0.99"],
    "mno1": ["-MNO", "1", "-FBS", "Y"],
    "mno120": ["-MNO", "120"],
    "bp40": ["-BP", "40", "-MGDP", "9"],                  # 360 threshold steps: longer than YQ_THR_LDS, the table stays in HBM
    "bp1": ["-BP", "1", "-MGDP", "2"],
}


def session_inputs(s):
    """(model parameters, sequence table) of a yaha_amd.Session: what ygpu_set_postfilter gets, and the scores of the session's alignment parameters"""
    import ctypes as C
    import yaha_amd as ya
    p = ya.PostfilterParams()
    assert ya.lib().yaha_session_postfilter_params(s._h, C.byref(p)) == 0
    st, ln = C.cast(p.seq_start, C.POINTER(C.c_uint32)), C.cast(p.seq_length, C.POINTER(C.c_uint32))
    seqs = [(int(st[i]), int(ln[i])) for i in range(p.n_seqs)]
    a = s.params
    return om.Params(a.GOCost, a.GECost, a.RCost, a.MScore, p.minNonOverlap, p.BPCost, p.maxBPLog, p.FBS, np.float32(p.FBS_PSLength), np.float32(p.FBS_PSScore)), seqs


def batch_codes(b):
    """the forward codes of every read of a ReadBatch, as bytes"""
    import ctypes as C
    offs = C.cast(b.offsets, C.POINTER(C.c_uint64))
    return [C.string_at(b.codes + int(offs[i]), int(offs[i + 1] - offs[i])) for i in range(b.n_reads)]


def result_clumps(r):
    """per read, the clumps of a ResultBatch as model records"""
    out = []
    for i in range(r.n_reads):
        mine = []
        for k in range(r.clump_start[i], r.clump_start[i + 1]):
            c = r.clumps[k]
            mine.append(om.Clump(c.sro, c.sqo, c.eqo, c.refLen, c.totScore, c.totLength, c.status, tuple((r.ops[c.op_start + j] & 0xFFFF, chr((r.ops[c.op_start + j] >> 16) & 0xFF)) for j in range(c.n_ops))))
        out.append(mine)
    return out


def as_result(lists):
    """a ResultBatch (and the arrays it points into) of per-read clump lists, for ygpu_inject_results"""
    import ctypes as C
    import yaha_amd as ya
    starts, recs, ops = [0], [], []
    for clumps in lists:
        for c in clumps:
            recs.append((c.sro, c.sqo, c.eqo, c.refLen, c.totScore, c.totLength, sum(l for l, k in c.ops if k == "M"), sum(l for l, k in c.ops if k == "R"),
                         sum(l for l, k in c.ops if k in "ID"), c.status, 0, len(ops), len(c.ops)))
            ops.extend(l | (ord(k) << 16) for l, k in c.ops)
        starts.append(len(recs))
    cs = (C.c_uint32 * len(starts))(*starts); cl = (ya.Clump * max(1, len(recs)))(*[ya.Clump(*x) for x in recs]); op = (C.c_uint32 * max(1, len(ops)))(*ops)
    r = ya.ResultBatch(); r.n_reads = len(lists); r.clump_start = cs; r.clumps = cl; r.ops = op; r.n_clumps = len(recs); r.n_ops = len(ops)
    return r, (cs, cl, op)


def mixed(B, n):
    """n clumps: tie families (copies of a repeat) at different places and strands, exact duplicates, nests under the score/8 rule, single spans of a handful of scores;
    shuffled."""
    out, rng, q = [], B.rng, B.qlen
    while len(out) < n:
        kind, room = int(rng.integers(0, 6)), n - len(out)
        sqo = int(rng.integers(0, q - 80)); eqo = int(min(q - 1, sqo + rng.integers(30, 300)))
        score = int(rng.choice([30, 60, 60, 100, 200, 400]))
        if kind == 0:
            out += B.family(int(min(room, rng.integers(2, 9))), sqo, eqo, score)
        elif kind == 1:
            out += B.family(int(min(room, rng.integers(2, 5))), sqo, eqo, score, same_place=True)
        elif kind == 2 and room >= 3:
            out += B.nest(sqo, eqo, 800, int(min(room - 1, rng.integers(1, 6))))
        else:
            out.append(B.clump(sqo, eqo, score, bool(rng.random() < 0.5)))
    return B.shuffled(out[:n])


def steps_of(P, limit=4000):
    """distances d in 12 .. limit where the break-point penalty changes: f(d) != f(d - 1)"""
    return [d for d in range(12, limit) if om.break_point_penalty(P, d) != om.break_point_penalty(P, d - 1)]


def bpp_read(B, P):
    """One left clump and, further right on the query, clumps on the same sequence at reference distances just below, at and just above the first steps of the
    break-point penalty (and 5, 10, 11: the constant part and its end); one on another sequence.  (Needs BPCost >= 1: one clump's score is the cost itself, and a
    score of 0 has no mapping quality.)"""
    left = B.clump(0, 99, 300, False, B.place(0), ops=((100, "M"),))
    end = left.sro + left.refLen - 1
    dist = [5, 10, 11]
    for s in steps_of(P)[:4]:
        dist += [s - 1, s, s + 1]
    out = [left]
    for k, d in enumerate(sorted(set(dist))):
        out.append(B.clump(200 + 3 * k, 400 + 5 * k, 200 + k, False, end + d, ops=((201 + 2 * k, "M"),)))
    # a first node whose score is exactly the penalty of the step to its nearest successor (3 bases on): the new score ties with the successor's own and there is no
    # predecessor to compare path lengths with -- no update
    out.append(B.clump(0, 120, P.BPCost, False, out[1].sro - 123, ops=((121, "M"),)))
    out.append(B.clump(450, 700, 250, True, seq=1))
    return B.shuffled(out)


def scan_read(B, group, tail):
    """`group` clumps of one SQO and descending EQO (no two alike, one score: nothing dies), then `tail` clumps one base further right that reach further: the scan
    behind the node at sorted position i < group runs over the rest of the group and ends at position `group` exactly."""
    out = [B.clump(10, 700 - t, 100, bool(t % 2), ops=((691 - t, "M"),)) for t in range(group)]
    out += [B.clump(11, 900 - t, 100, False, ops=((890 - t, "M"),)) for t in range(tail)]
    return B.shuffled(out)


def kills_across_blocks(B, inner):
    """an outer clump first in the sorted order, `inner` (> 64) victims of the score/8 rule behind it -- killed inside its block and beyond -- and, after them, a
    family of exact duplicates longer than a block, its first member killing the rest on both sides of the next block edge"""
    out = B.nest(0, B.qlen - 1, 4000, inner)
    out += B.family(70, 300, 600, 700, False, same_place=True)
    out += B.family(3, 650, 900, 650)
    return B.shuffled(out)


def pivot_extreme(B, n, largest):
    """no two keys equal; the middle element of the list holds the smallest (nL == 0) or the largest (nL == m) key of all"""
    cl = B.by_key(B.distinct(n, 5, 10, 300, 100))
    mid = (n - 1) // 2
    pick = cl.pop(-1 if largest else 0)
    rest = B.shuffled(cl)
    return rest[:mid] + [pick] + rest[mid:]


def straddle(B, n=130):
    """a family of ten equal keys at list positions 59 .. 68 -- the pivot of the first partition (position 64) among them, its ties in scan positions 59 .. 63 and 65 .. 68:
    on both sides of the first 64-chunk's end -- between clumps of other keys"""
    others = B.shuffled(B.distinct(n - 10, 5, 10, 300, 100))
    fam = B.family(10, 8, 500, 100)
    return others[:59] + fam + others[59:]


def ladder_read(B, steps, width, stride, extra=0, score=200, near=False, seq_of=None):
    out = B.ladder(steps, 2, width, stride, score, seq_of=seq_of, near=near)
    if extra:
        out += B.distinct(extra, 0, 10, B.qlen - 40 - extra // 10, 90)
    return B.shuffled(out)


def tiny_batch(qlens, seqs):
    """About 130 reads of 0 .. 5 clumps: k_oqc_classify's lists hold one, two and more than 64 reads of a class, across wave boundaries of its blocks of 256 (with
    YGPU_OQC_MAX = 4 the reads of five clumps are the hand-over class)."""
    out = []
    for i, q in enumerate(qlens):
        B = om.Builder(q, seqs, 5000 + i)
        n = 113 if i == 70 else 230 if i in (3, 99) else (0, 1, 2, 3, 4, 5, 2, 4)[i % 8]
        out.append(("tiny_%d_of_%d" % (i, n), mixed(B, n)))
    return out


def edges(qlens, seqs, P):
    """The directed reads of one batch of at most 48 (class edges, first partitions of 63 .. 129 scanned elements, tie sets, scan and placement edges, ladders)."""
    assert len(qlens) >= 48 and min(qlens[:48]) >= 950
    reads = []

    def add(label, make):
        B = om.Builder(qlens[len(reads)], seqs, 1000 + len(reads))
        reads.append((label, make(B)))
    for n in (0, 1, 2, 112, 113, 224, 225, 448, 449):
        add("class_edge_%d" % n, lambda B, n=n: mixed(B, n))
    for n in (64, 65, 66, 128, 129, 130):
        add("first_partition_%d" % (n - 1), lambda B, n=n: mixed(B, n))
    for n in (2, 64, 65, 130):
        add("all_equal_%d" % n, lambda B, n=n: B.family(n, 100, 600, 100))
    # ONE clump set (a builder of its own seed makes it: the same plus-strand spans, places and strands whatever read it is injected for) in three orders
    one_set = lambda B: om.Builder(B.qlen, seqs, 777).distinct(100, 5, 10, 300, 100)
    add("none_equal_100", lambda B: B.shuffled(one_set(B)))
    add("none_equal_ascending", lambda B: B.by_key(one_set(B)))
    add("none_equal_descending", lambda B: B.by_key(one_set(B), descending=True))
    add("straddle_130", straddle)
    add("pivot_smallest_100", lambda B: pivot_extreme(B, 100, False))
    add("pivot_largest_100", lambda B: pivot_extreme(B, 100, True))
    for fam, n in ((63, 64), (64, 66), (65, 70), (130, 140)):
        # (the family, then clumps far to the right: the first far node of node 0 lies more than 64 places behind startj)
        add("family_%d" % fam, lambda B, fam=fam, n=n: B.shuffled(B.family(fam, 20, 400, 100) + B.distinct(n - fam, 500, 2, 800, 120)))
    add("duplicates_70", lambda B: B.shuffled(B.family(70, 50, 450, 300, True, same_place=True) + B.family(2, 500, 900, 310)))
    add("scan_ends_at_lane_63", lambda B: scan_read(B, 63, 5))
    add("scan_ends_at_lane_64", lambda B: scan_read(B, 64, 5))
    add("scan_ends_two_blocks_on", lambda B: scan_read(B, 150, 5))
    add("kills_across_blocks", lambda B: kills_across_blocks(B, 100))
    add("bpp_steps", lambda B: bpp_read(B, P))
    add("tables_overrun_112", lambda B: ladder_read(B, 112, 50, 8))
    add("ladder_overlaps", lambda B: ladder_read(B, 30, 70, 26))
    add("ladder_near", lambda B: ladder_read(B, 20, 40, 45, near=True))
    add("ladder_two_sequences", lambda B: ladder_read(B, 12, 60, 70, seq_of=lambda k: k // 3))
    add("primaries_70_in_hbm", lambda B: ladder_read(B, 70, 13, 13, extra=30))
    add("primaries_70_in_lds", lambda B: ladder_read(B, 70, 13, 13, extra=50))
    add("scores_wrap", lambda B: ladder_read(B, 30, 30, 32, score=2000))
    add("two_primaries", lambda B: B.shuffled(B.ladder(2, 10, 300, 400, 500) + B.family(3, 10, 309, 480) + B.family(2, 420, 700, 100)))
    while len(reads) < 48:
        add("mixed_%d" % (20 + 7 * len(reads)), lambda B: mixed(B, 20 + 7 * len(reads)))
    return reads


def large(qlens, seqs):
    """The reads of the last device class that only size reaches: 1 792 clumps in the anti-quicksort order (the sort's stack runs over its 128 ints of LDS into HBM;
    nearly all of them nested under one outer clump, so that the graph stays small), 1 793 (handed back unfiltered), 1 349 survivors (the last count whose nodes
    fit the LDS: 48 * 1349 <= 64 768, with four ints of table pool) and 1 350 and more (oqcGraph<false> without the environment hook), 500 equal keys."""
    reads = []

    def add(label, make):
        B = om.Builder(qlens[len(reads)], seqs, 3000 + len(reads))
        reads.append((label, make(B)))

    def nested(B, n):
        """n clumps of n distinct keys: one outer clump and n - 1 - 12 nested victims with distinct (SQO, EQO), twelve survivors beside"""
        inner = n - 13
        out = [B.clump(0, B.qlen - 1, 8000, False, ops=((B.qlen, "M"),))]
        for k in range(inner):
            s, e = 1 + k % 40, 100 + k // 40
            out.append(B.clump(s, e, 50 + k % 7, bool(k % 2), ops=((e - s + 1, "M"),)))
        out += B.ladder(12, 50, 60, 70, 1500)
        return out
    add("adversarial_1792", lambda B: B.adversarial(nested(B, 1792)))
    add("handed_back_1793", lambda B: B.shuffled(nested(B, 1793)))
    def with_copies(B, n, copies):                                     # (identical records: one of each pair dies)
        base = B.distinct(n, 0, 20, 400, 100)
        return B.shuffled(base + base[:copies])
    add("survivors_1349", lambda B: with_copies(B, 1349, 30))
    add("survivors_1400", lambda B: B.shuffled(B.distinct(1400, 0, 20, 400, 100) + B.ladder(6, 500, 60, 70, 150)))
    add("family_500", lambda B: B.shuffled(B.family(500, 20, 400, 100) + B.distinct(20, 500, 2, 800, 120)))
    add("class_edge_1792", lambda B: mixed(B, 1792))
    return reads
