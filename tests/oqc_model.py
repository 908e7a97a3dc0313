"""A plain model of the post-filter of ONE read (Optimal Query Coverage, duplicate removal, filter by similarity, mapping quality), stated from the reference's rules
and written for clarity: every intermediate is kept.  It is the independent referee of csrc/oqc_core.h (one thread) and device/oqc_stage.h (a wave a read).

What it follows, by line of the reference:
  GraphPath.cpp:897-1086  postFilterBySimilarity: zero and one clump (:903-916), nodes made in list order (:929-934, initcGraphNode :342-363), the sort
                          (myQuickSort :427-459 on getCompareKey :377-380, ties by graphNodeLessThan :382-388), deleteSubsumedDups :488-517, the graph loop
                          :973-1063 with the break-point penalty as the log10 expression :1015-1024, cacheQlenInOQCPath :841-867 (the recursion itself),
                          calcAccurateOverlapScore :744-800, cacehQlenInOQCPathReverse :802-826, cacheQlenInRightNode :873-878, calcScoreForLength :705-732 as the
                          literal walk over the edit list, filterBySimilarity :571-692, calcMQfromPAs :559-569.
  Math.c:274-284          getRandBits, the per-read generator;  QueryState.c:172-187 generateRandomSeed, its seed.
  BaseSeq.c:81-90         findBaseSequenceNum (-1 stored in a UBYTE: 255).
Types: SINT fields (bestScore, pathLength, nodeLength, nodeScore) and `SINT newScore` wrap at 16 bits, QOFF / SUINT fields (SQO, EQO, qLenInOQC) at 16 bits unsigned,
ROFF at 32; FBS_PSLength / FBS_PSScore are floats (numpy.float32 here) widened to double where the reference widens them; everything else in the similarity and
mapping-quality arithmetic is a Python float: IEEE double, one rounding per operation.

`Coverage` is something else: statements about the DEVICE's layout (device/oqc_stage.h) -- which class a read falls in, what its LDS holds, which partitions its sort
makes in the device's formulation, where a duplicate scan crosses a block of 64 -- never what the result should be.  The tests use it to show that an input reaches
the edge it was built for before anything is compared."""
import math
import sys
from collections import Counter, namedtuple

import numpy as np

ST_REVERSED, ST_PRIMARY = 0x01, 0x20
WORST_SCORE = -(0x7fffff00)

# One clump as the hot path returns it (include/yaha_hip.h ygpu_clump): sqo / eqo strand-local, ops = ((length, code), ...) with code in "MRID"
Clump = namedtuple("Clump", "sro sqo eqo refLen totScore totLength status ops")
Params = namedtuple("Params", "GOCost GECost RCost MScore minNonOverlap BPCost maxBPLog FBS PSLength PSScore")      # PSLength, PSScore: numpy.float32
Out = namedtuple("Out", "clump status mapQuality numSecondaries matchedPrimary")                                   # yoqc::OutRec / ygpu_out_clump


def s16(v):
    v &= 0xFFFF
    return v - 0x10000 if v & 0x8000 else v


def u16(v):
    return v & 0xFFFF


def u32(v):
    return v & 0xFFFFFFFF


class Rand:
    """Math.c:274-284, five words of state."""

    def __init__(self, state):
        self.s = [u32(w) for w in state]
        self.draws = 0

    def bits(self):
        s = self.s
        t = s[0] ^ (s[0] >> 7)
        s[0] = s[1]; s[1] = s[2]; s[2] = s[3]; s[3] = s[4]
        s[4] = u32((s[4] ^ u32(s[4] << 6)) ^ (t ^ u32(t << 13)))
        self.draws += 1
        return u32((s[1] + s[1] + 1) * s[4])


class ShortDrawRand(Rand):
    """What a wrong draw COUNT looks like (quick_sort reads `one_short_per_chunk`): of the ties in every 64 scanned elements of a partition the last gets no coin of
    its own and counts as not less -- a wave that draws one bit fewer than its ballot has ties -- so every later comparison meets another coin."""
    one_short_per_chunk = True


class FlippedRand(Rand):
    """The same generator with every coin turned over: what a wrong draw sequence looks like (the tests' proof that a tie set is sensitive to the draws)."""

    def bits(self):
        return Rand.bits(self) ^ 1


def seed_words(codes, qlen):
    """QueryState.c:172-187: two low bits of sixteen codes a word, the position running on from word to word and wrapping at the read's end."""
    q, out = 0, []
    for _ in range(5):
        w = 0
        for _ in range(16):
            w = u32(w << 2) | (codes[q] & 3)
            q += 1
            if q >= qlen:
                q = 0
        out.append(w)
    return out


class Node:
    """cGraphNode, GraphPath.cpp:299-324; bestPrev is a Node or None, clump an index into the read's list or None (dead)."""
    __slots__ = ("bestPrev", "clump", "bestScore", "pathLength", "SRO", "ERO", "SQO", "EQO", "nodeLength", "nodeScore", "qLenInOQC", "reversed", "seqNum", "key", "pos")


def find_seq(seqs, off):
    for i, (start, length) in enumerate(seqs):
        if start <= off < start + length:
            return i
    return -1


def init_node(i, c, qlen, seqs):                                      # :342-363
    nd = Node()
    nd.bestPrev = None; nd.pathLength = 1; nd.clump = i
    nd.bestScore = nd.nodeScore = s16(c.totScore)
    nd.nodeLength = s16(c.totLength)
    rev = bool(c.status & ST_REVERSED)
    nd.SQO = u16((qlen - 1) - c.eqo) if rev else c.sqo                 # clumpPlusSQO / clumpPlusEQO, FragsClumps.inl:355-365
    nd.EQO = u16((qlen - 1) - c.sqo) if rev else c.eqo
    nd.SRO = c.sro; nd.ERO = u32(c.sro + c.refLen - 1)
    nd.reversed = rev
    nd.qLenInOQC = u16(1 + c.eqo - c.sqo)
    nd.seqNum = find_seq(seqs, nd.SRO) & 0xFF
    nd.key = (((nd.SQO << 16) + u16(-s16(nd.EQO))) << 16) + u16(-nd.nodeScore)      # getCompareKey :377-380
    nd.pos = -1
    return nd


def quick_sort(arr, left, right, rng, parts, waiting=0):
    """myQuickSortHelper :427-453, the recursion as it stands.  `parts` collects, for Coverage, one record a partition in the device's terms: m = right - left scanned
    elements, the scan positions of the ties, nL, and how many right parts wait while this partition's left part is sorted (the device stacks a right part of two or
    more elements and nothing else; `waiting` counts those of the enclosing calls)."""
    if left >= right:
        return
    pivot = (left + right) // 2
    arr[pivot], arr[right] = arr[right], arr[pivot]
    pk, store, ties = arr[right].key, left, []
    no_coin = set()
    if getattr(rng, "one_short_per_chunk", False):                     # (ShortDrawRand only; the scan moves nothing that it has not yet looked at)
        no_coin = set({(i - left) // 64: i for i in range(left, right) if arr[i].key == pk}.values())
    for i in range(left, right):
        k = arr[i].key
        if k == pk:
            less = bool(rng.bits() & 1) if i not in no_coin else False
            ties.append(i - left)
        else:
            less = k < pk
        if less:
            arr[i], arr[store] = arr[store], arr[i]
            store += 1
    arr[store], arr[right] = arr[right], arr[store]
    mine = waiting + (1 if store + 1 < right else 0)
    parts.append({"left": left, "m": right - left, "ties": len(ties), "tie_chunks": len({t // 64 for t in ties}), "nL": store - left, "waiting": mine})
    quick_sort(arr, left, store - 1, rng, parts, mine)
    quick_sort(arr, store + 1, right, rng, parts, waiting)


def op_score(P, op, ln):
    if op == "M":
        return P.MScore * ln
    if op == "R":
        return -(P.RCost * ln)
    if op == "I":
        return -(P.GOCost + P.GECost * ln)
    return 0


def score_for_length(P, ops, length, forward):                         # calcScoreForLength :705-732
    qlen = ags = 0
    for ln, op in (ops if forward else reversed(ops)):
        if not qlen < length:
            break
        if op == "D":
            ags -= P.GOCost + P.GECost * ln
        else:
            if qlen + ln > length:
                ln = length - qlen
            qlen += ln
            ags += op_score(P, op, ln)
    return ags


def break_point_penalty(P, distance):                                  # :1015-1021, the expression itself
    if distance <= 10:
        return P.BPCost
    lg = math.log10(float(distance))
    if lg > P.maxBPLog:
        lg = float(P.maxBPLog)
    return int(lg * P.BPCost + 0.5)


def map_quality(tot, second, third):                                   # calcMQfromPAs :559-569, with the branch taken
    if second == 0:
        return 250, "mq_no_second"
    ts = float(tot)
    a = max(ts - second, 0.0)
    b = max(ts - third, 0.0)
    ratio = a / ts
    ratio = ratio * (1.0 + b / tot) / 2.0
    q = 250.0 * ratio + 0.5
    # (third <= second: b is clamped only where a is, and there the product is 0 whatever b is -- the clamp of the third term never changes a result; the event is
    # recorded so that the tests can show inputs in which a secondary scores at least what its primary does, twice)
    how = "mq_second_and_third_at_least_total" if b == 0.0 else "mq_second_at_least_total" if a == 0.0 else "mq_third_zero" if third == 0 else "mq_both"
    return int(q) & 0xFF, how


class Model:
    """One read's run.  After run(): sorted_order (clump indices after the sort), survivors (after the duplicate removal), nodes (the survivors' Node objects, in order),
    best (index of the best node), primaries (node indices, left to right), out (print order), primary_count, events (a Counter of the branches taken) and
    partitions / scans (the sort's and the duplicate scan's records for Coverage)."""

    def __init__(self, P, seqs, rand=Rand):
        self.P, self.seqs, self.rand = P, list(seqs), rand

    def run(self, codes, qlen, clumps):
        self.events = ev = Counter(); self.partitions = []; self.scans = []
        self.sorted_order = []; self.survivors = []; self.nodes = []; self.best = None; self.primaries = []
        n = len(clumps)
        if n < 1:                                                      # :903-904
            self.out, self.primary_count = [], 0
            return self.out, 0
        if n == 1:                                                     # :907-916
            self.out, self.primary_count = [Out(0, clumps[0].status | ST_PRIMARY, 250, 0, 1)], 1
            return self.out, 1
        P = self.P
        arr = [init_node(i, c, qlen, self.seqs) for i, c in enumerate(clumps)]
        if any(c.status & ST_REVERSED for c in clumps):
            ev["reversed_clump"] += 1
        rng = self.rand(seed_words(codes, qlen))
        limit = sys.getrecursionlimit()
        sys.setrecursionlimit(max(limit, 3 * n + 1000))
        try:
            quick_sort(arr, 0, n - 1, rng, self.partitions)
        finally:
            sys.setrecursionlimit(limit)
        self.draws = rng.draws
        self.sorted_order = [nd.clump for nd in arr]
        nodes = self.dedup(arr, clumps)
        self.survivors = [nd.clump for nd in nodes]
        self.nodes = nodes
        for p, nd in enumerate(nodes):
            nd.pos = p
        cnt = len(nodes)
        best_score, best, startj = WORST_SCORE, None, 1
        for i in range(cnt):                                           # :973-1063
            left = nodes[i]
            self.cache_path(left, clumps)
            found = False
            if startj >= cnt:
                ev["startj_at_cnt"] += 1
            first_j = startj
            for j in range(startj, cnt):
                right = nodes[j]
                if (right.SQO - left.SQO) >= P.minNonOverlap:
                    if not found:
                        startj, found = j, True
                        if (j - first_j) >= 64:                        # (the device looks at startj .. startj + 63 first)
                            ev["startj_first_far_in_later_chunk"] += 1
                    self.relax(left, right, clumps)
                if not found:
                    startj = cnt
            if not found and first_j < cnt:
                ev["startj_none_far"] += 1
            if left.bestScore < best_score:
                ev["best_lower"] += 1
                continue
            if left.bestScore > best_score:
                ev["best_higher"] += 1; best, best_score = left, left.bestScore
            elif best is not None and left.pathLength < best.pathLength:
                ev["best_tie_shorter_path"] += 1; best, best_score = left, left.bestScore
            else:
                ev["best_tie_not_shorter"] += 1
        self.best = best.pos
        self.best_prev = [nd.bestPrev.pos if nd.bestPrev is not None else -1 for nd in nodes]
        self.best_scores = [nd.bestScore for nd in nodes]
        return self.finish(nodes, best, clumps)

    # ---- deleteSubsumedDups :488-517 ---------------------------------------------------------------------------------------------------------------------------
    def dedup(self, arr, clumps):
        ev, n, keep = self.events, len(arr), []
        for i in range(n):
            cur = arr[i]
            if cur.clump is None:
                ev["dup_dead_at_its_turn"] += 1
                continue
            keep.append(cur)
            threshold = int(cur.nodeScore / 8)                         # C division truncates towards zero
            end = None
            for j in range(i + 1, n):
                nxt = arr[j]
                if nxt.clump is None:
                    continue
                if nxt.EQO > cur.EQO:
                    end = j
                    break
                where = "in_block" if j // 64 == i // 64 else "out_of_block"
                if cur.EQO > nxt.EQO and nxt.nodeScore < threshold:
                    ev["dup_kill_score8_" + where] += 1; nxt.clump = None
                elif (cur.SRO == nxt.SRO and cur.ERO == nxt.ERO and cur.reversed == nxt.reversed and cur.SQO == nxt.SQO and cur.EQO == nxt.EQO):
                    ev["dup_kill_same_place_" + where] += 1; nxt.clump = None
            self.scans.append((i, end))
        return keep

    # ---- the accurate overlap score and the two caches ------------------------------------------------------------------------------------------------------------
    def overlap_score(self, left, right, overlap, clumps):             # :744-800
        P = self.P
        right_score = score_for_length(P, clumps[right.clump].ops, overlap, not right.reversed)
        path_score, remaining, cur, walked = 0, overlap, left, 1
        while True:
            take = min(remaining, cur.qLenInOQC)
            remaining -= take
            path_score += score_for_length(P, clumps[cur.clump].ops, take, cur.reversed)
            if remaining <= 0:
                break
            cur = cur.bestPrev; walked += 1
            if cur is None:
                raise AssertionError("the best path ends before the overlap is covered: the reference would follow a NULL bestPrev")
        if walked > 1:
            self.events["overlap_walk_through_several_nodes"] += 1
        if path_score > right_score:
            return right_score, False
        return path_score, True

    def cache_path(self, right, clumps):                               # cacheQlenInOQCPath :841-867
        qlen = 1 + right.EQO - right.SQO
        if right.bestPrev is None:
            right.qLenInOQC = u16(qlen)
            return right
        left = self.cache_path(right.bestPrev, clumps)
        overlap = (left.EQO - right.SQO) + 1 if left.EQO >= right.SQO else 0
        if overlap > 0:
            _score, right_best = self.overlap_score(left, right, overlap, clumps)
            if right_best:                                             # cacehQlenInOQCPathReverse :802-826
                right.qLenInOQC = u16(qlen)
                remaining, cur = overlap, left
                while True:
                    take = min(remaining, cur.qLenInOQC)
                    cur.qLenInOQC = u16(cur.qLenInOQC - take); remaining -= take
                    if remaining <= 0:
                        break
                    cur = cur.bestPrev
            else:
                right.qLenInOQC = u16(qlen - overlap)
        else:
            right.qLenInOQC = u16(qlen)
        return right

    # ---- one pair of the graph loop, :996-1047 --------------------------------------------------------------------------------------------------------------------
    def relax(self, left, right, clumps):
        P, ev = self.P, self.events
        if (right.EQO - left.EQO) < P.minNonOverlap:
            ev["relax_eqo_too_close"] += 1
            return
        new = s16(left.bestScore + right.nodeScore)
        if right.bestScore > new:
            ev["relax_lost_before_penalty"] += 1
            return
        if left.seqNum == right.seqNum:
            if left.SRO > right.ERO:
                distance = u32(left.SRO - right.ERO)
            elif right.SRO > left.ERO:
                distance = u32(right.SRO - left.ERO)
            else:
                distance = 0
            bpp = break_point_penalty(P, distance)
            if distance <= 10:
                ev["bpp_near"] += 1
            else:
                ev["bpp_far"] += 1
                f = lambda d: break_point_penalty(P, d)
                if distance > 11 and f(distance) != f(distance - 1):
                    ev["bpp_at_a_step"] += 1
                if f(distance + 1) != f(distance):
                    ev["bpp_one_below_a_step"] += 1
                if distance > 12 and f(distance - 1) != f(distance - 2):
                    ev["bpp_one_above_a_step"] += 1
        else:
            bpp = P.maxBPLog * P.BPCost
            ev["bpp_other_sequence"] += 1
        new = s16(new - bpp)
        if right.bestScore > new:
            ev["relax_lost_after_penalty"] += 1
            return
        overlap = (left.EQO - right.SQO) + 1 if left.EQO >= right.SQO else 0
        right_best = False
        if overlap > 0:
            sc, right_best = self.overlap_score(left, right, overlap, clumps)
            ev["overlap_right_best" if right_best else "overlap_path_best"] += 1
            new = s16(new - sc)
            if right.bestScore > new:
                ev["relax_lost_after_overlap"] += 1
                return
        if right.bestScore < new:
            ev["relax_better"] += 1
        elif right.bestPrev is not None and left.pathLength < right.bestPrev.pathLength:
            ev["relax_tie_shorter_path"] += 1
        else:
            ev["relax_tie_no_prev" if right.bestPrev is None else "relax_tie_not_shorter"] += 1
            return
        if overlap > 0:                                                # cacheQlenInRightNode :873-878
            qlen = 1 + right.EQO - right.SQO
            right.qLenInOQC = u16(qlen if right_best else qlen - overlap)
        right.bestScore = new; right.bestPrev = left; right.pathLength = s16(left.pathLength + 1)

    # ---- filterBySimilarity :571-692 ------------------------------------------------------------------------------------------------------------------------------
    def finish(self, nodes, best, clumps):
        P, ev = self.P, self.events
        prime_count = best.pathLength
        primaries = [None] * prime_count
        attrs = [None] * prime_count
        pushed = []                                                    # pushClump puts a clump at the HEAD of the new list: the list is the pushes reversed
        matched = {}
        k, nd = prime_count - 1, best
        while nd is not None:
            primaries[k] = nd
            attrs[k] = {"len": 1 + nd.EQO - nd.SQO, "second": 0, "third": 0, "out": 0}
            matched[nd.clump] = k + 1
            pushed.append(nd.clump)
            nd = nd.bestPrev; k -= 1
        prime_clumps = set(matched)
        self.primaries = [p.pos for p in primaries]
        ev["primaries_1" if prime_count == 1 else "primaries_2" if prime_count == 2 else "primaries_more_than_64" if prime_count > 64 else "primaries_3_to_64"] += 1
        target = float(P.PSLength)
        for cur in nodes:
            if cur.clump in prime_clumps:
                continue
            cur_len = 1 + cur.EQO - cur.SQO
            max_overlap = max_index = 0
            for i, pn in enumerate(primaries):
                overlap = 1 + min(cur.EQO, pn.EQO) - max(cur.SQO, pn.SQO)
                if overlap > max_overlap:
                    max_overlap, max_index = overlap, i
            if max_overlap <= 0:
                ev["node_overlaps_no_primary"] += 1
                continue
            a, pn = attrs[max_index], primaries[max_index]
            if cur.nodeScore > a["second"]:                            # memoPAsFromOverlappingNode :545-557
                a["third"], a["second"] = a["second"], cur.nodeScore; ev["second_score_updated"] += 1
            elif cur.nodeScore > a["third"]:
                a["third"] = cur.nodeScore; ev["third_score_updated"] += 1
            else:
                ev["second_and_third_kept"] += 1
            if float(cur.nodeScore) / pn.nodeScore >= float(P.PSScore):
                overlap = float(1 + min(cur.EQO, pn.EQO) - max(cur.SQO, pn.SQO))
                if overlap / cur_len >= target and overlap / a["len"] >= target:
                    a["out"] += 1
                    if P.FBS:
                        matched[cur.clump] = max_index + 1
                        pushed.append(cur.clump); ev["secondary_pushed"] += 1
                        continue
                    ev["secondary_counted_not_pushed"] += 1
                    continue
            if P.FBS:
                ev["secondary_failed_with_FBS_on"] += 1
        out = []
        for c in reversed(pushed):
            if c in prime_clumps:
                a = attrs[matched[c] - 1]
                mq, how = map_quality(clumps[c].totScore, a["second"], a["third"]); ev[how] += 1
                out.append(Out(c, clumps[c].status | ST_PRIMARY, mq, a["out"] & 0xFFFF, matched[c]))
            else:
                out.append(Out(c, clumps[c].status, 255, 0, matched[c]))    # a secondary keeps what allocClump gave it (FragsClumps.c:131)
        self.out, self.primary_count = out, prime_count
        return out, prime_count


# ---- what an input reaches on the DEVICE (device/oqc_stage.h): statements about its layout, never about the result -----------------------------------------------
OQC_CAP_N = (112, 224, 448, 1792)                                      # kOqcCapN
YQ_DEVICE_MAX, YQ_STACK_LDS, YQ_THR_LDS, YQ_LDS_MAX, YQ_SORT_LDS = 1792, 128, 64, 65536, 36
NODE_BYTES, ATTR_BYTES = 32, 12                                        # sizeof(yoqc::CNode), sizeof(yoqc::PAttr)


def lds_main_bytes(cls):
    """oqcLdsBytes(cap) clamped to 64 KB, less the sort stack and the threshold table in front."""
    return min(YQ_LDS_MAX, 64 * OQC_CAP_N[cls] + 4 * (YQ_STACK_LDS + YQ_THR_LDS) + 64) - 4 * (YQ_STACK_LDS + YQ_THR_LDS)


def device_class(n, dev_max=YQ_DEVICE_MAX):
    """where k_oqc_classify sends a read of n clumps: it settles reads of none and one itself, hands reads of more than dev_max (YGPU_OQC_MAX, at most 1 792) back
    unfiltered, and lists the others by the first capacity of kOqcCapN that holds them"""
    return "settled_by_classify" if n < 2 else "host" if n > min(dev_max, YQ_DEVICE_MAX) else next(c for c in range(4) if n <= OQC_CAP_N[c])


class Coverage:
    """What one read reaches in device/oqc_stage.h, from the model's run of it (m = a Model after run(); dev_max = YGPU_OQC_MAX or 1 792; hbm = YGPU_OQC_HBM)."""

    def __init__(self, m, clumps, dev_max=YQ_DEVICE_MAX, hbm=False):
        n = len(clumps)
        self.n, self.events = n, Counter(m.events)
        self.cls = device_class(n, dev_max)
        self.partitions, self.scans = m.partitions, m.scans
        self.stack_spills, self.scan_ends = False, Counter()
        if not isinstance(self.cls, int):                              # not a read k_oqc_wave sees
            return
        mb = self.main_bytes = lds_main_bytes(self.cls)
        self.keys_in_lds = 16 * n <= mb
        self.sort_on_wave = self.keys_in_lds and YQ_SORT_LDS * n <= mb
        cnt = self.cnt = len(m.survivors)
        self.graph_in_lds = (not hbm) and self.keys_in_lds and 48 * cnt <= mb
        self.graph_at_lds_limit = self.graph_in_lds and 48 * (cnt + 1) > mb
        cap = (mb - 48 * cnt) // 4 if self.graph_in_lds else 0
        used, self.tables_lds, self.tables_hbm = 0, 0, 0
        for c in m.survivors:                                          # the bump allocator of assignTable, in node order
            need = 2 * len(clumps[c].ops) + 3
            if used + need <= cap:
                used += need; self.tables_lds += 1
            else:
                self.tables_hbm += 1
        pc = m.primary_count
        at = (48 * cnt + 15) & ~15
        self.primaries_in_lds = self.graph_in_lds and at + (NODE_BYTES + ATTR_BYTES) * pc <= mb
        self.max_waiting = max([p["waiting"] for p in m.partitions] or [0])
        self.stack_spills = 2 * self.max_waiting > YQ_STACK_LDS
        # where the scan behind the survivor at sorted position i ended, in blocks of 64 of the sorted list
        self.scan_ends = Counter()
        for i, end in m.scans:
            if end is None:
                self.scan_ends["list_end" if (n - 1) // 64 > i // 64 else "list_end_in_own_block"] += 1
            else:
                d = end // 64 - i // 64
                self.scan_ends["own_block" if d == 0 else "next_block" if d == 1 else "two_or_more_blocks_on"] += 1
                if d == 0 and end % 64 == 63:
                    self.scan_ends["at_lane_63"] += 1
                if d == 1 and end % 64 == 0:
                    self.scan_ends["at_lane_0_of_the_next_block"] += 1


def run_read(P, seqs, codes, qlen, clumps, rand=Rand):
    m = Model(P, seqs, rand)
    m.run(codes, qlen, clumps)
    return m


# ---- input builders: seeded, deterministic; spans are given on the PLUS strand and turned into the strand-local offsets of the clump record ------------------------
class Builder:
    """Clump lists for a read of `qlen` bases; places are drawn inside the sequences of `seqs` ((start, length), ...).
    What no list can reach on the device, and why: the one-lane sort of k_oqc_wave (`sortOnWave` false) and keys outside LDS (`keysInLds` false).  The last device class
    has 64 768 bytes of LDS behind the stack and the thresholds; the wave's sort needs 36 bytes a clump and the keys 16, so they fit up to 1 799 and 4 048 clumps, and
    k_oqc_classify hands every read of more than YQ_DEVICE_MAX = 1 792 clumps back unfiltered; in the smaller classes 64 bytes a clump are reserved.  Both branches are
    dead for every input; Coverage records the two flags and the tests assert that they are always true."""

    def __init__(self, qlen, seqs, seed):
        self.qlen, self.seqs, self.rng = qlen, list(seqs), np.random.default_rng(seed)

    def place(self, seq=None):
        k = int(self.rng.integers(0, len(self.seqs))) if seq is None else seq % len(self.seqs)
        start, length = self.seqs[k]
        return int(start + self.rng.integers(100, max(101, length - 5000)))

    def ops_for(self, span, plain=False):
        """An edit list that covers `span` query bases: all four ops, adjacent ops of one kind merged, no D at either end."""
        if plain or span < 6:
            return ((span, "M"),)
        out, q = [], 0
        while q < span:
            kind = "MMMMMRID"[int(self.rng.integers(0, 8))]
            ln = int(min(span - q, self.rng.integers(1, 30))) if kind != "D" else int(self.rng.integers(1, 5))
            if kind == "D" and (not out or span - q < 2):
                kind, ln = "M", int(min(span - q, self.rng.integers(1, 30)))
            if out and out[-1][1] == kind:
                out[-1] = (out[-1][0] + ln, kind)
            else:
                out.append((ln, kind))
            q += ln if kind != "D" else 0
        if out[-1][1] == "D":
            out.pop()
        return tuple(out)

    def clump(self, sqo, eqo, score, rev=False, sro=None, ops=None, seq=None):
        """plus-strand span [sqo, eqo]"""
        assert 0 <= sqo <= eqo < self.qlen
        ops = ops if ops is not None else self.ops_for(eqo - sqo + 1)
        assert sum(l for l, c in ops if c != "D") == eqo - sqo + 1
        ref_len = sum(l for l, c in ops if c in "MRD")
        lo, hi = ((self.qlen - 1) - eqo, (self.qlen - 1) - sqo) if rev else (sqo, eqo)
        return Clump(self.place(seq) if sro is None else sro, lo, hi, ref_len, score, eqo - sqo + 1, 0x0C | (ST_REVERSED if rev else 0), ops)

    def family(self, count, sqo, eqo, score, rev=None, same_place=False):
        """`count` clumps of ONE key.  same_place: exact duplicates (one place, one strand -- all but the first to be sorted die) whose edit lists differ, so that the
        survivor shows in the copied ops; otherwise copies of a repeat (other places, either strand), which all survive in the order the draws give them."""
        out, sro = [], self.place()
        r0 = bool(self.rng.random() < 0.5) if rev is None else rev
        span = eqo - sqo + 1
        for k in range(count):
            if same_place:
                cut = 1 + k % max(1, span - 1)
                ops = ((span, "M"),) if span < 2 else ((cut, "M"), (span - cut, "R")) if k % 2 else ((cut, "R"), (span - cut, "M"))
                out.append(self.clump(sqo, eqo, score, r0, sro, ops))
            else:
                out.append(self.clump(sqo, eqo, score, bool(self.rng.random() < 0.5) if rev is None else rev, ops=((span, "M"),)))
        return out

    def nest(self, sqo, eqo, score, inner):
        """An outer clump and `inner` clumps strictly inside its query span with less than an eighth of its score: the score/8 rule kills them."""
        out = [self.clump(sqo, eqo, score)]
        for _ in range(inner):
            a = int(self.rng.integers(sqo, eqo - 3)); b = int(self.rng.integers(a, eqo))
            out.append(self.clump(a, b, int(self.rng.integers(1, max(2, score // 8)))))
        return out

    def ladder(self, steps, first, width, stride, score, seq_of=None, near=False):
        """`steps` spans of `width` bases, each `stride` further right: stride < width makes them overlap (the accurate overlap score), stride >= minNonOverlap lets
        each follow the one before -- a best path of `steps` primaries.  near: consecutive steps a few bases apart on one sequence (small break-point penalties)."""
        out, sro = [], self.place(0)
        for k in range(steps):
            s = first + k * stride
            if near:
                sro += width + int(self.rng.integers(0, 30))
                out.append(self.clump(s, s + width - 1, score, False, sro))
            else:
                out.append(self.clump(s, s + width - 1, score, bool(k % 2), seq=None if seq_of is None else seq_of(k)))
        return out

    def distinct(self, count, sqo_lo, sqo_n, eqo_lo, score, rev=None):
        """`count` clumps no two of which share a key or die: distinct (SQO, EQO) pairs, SQO within [sqo_lo, sqo_lo + sqo_n), one score (the score/8 rule needs a
        smaller score)."""
        out, per = [], -(-count // sqo_n)
        assert eqo_lo + per <= self.qlen
        for k in range(count):
            out.append(self.clump(sqo_lo + k % sqo_n, eqo_lo + k // sqo_n, score, bool(k % 3 == 0) if rev is None else rev, ops=((eqo_lo + k // sqo_n - (sqo_lo + k % sqo_n) + 1, "M"),)))
        return out

    def shuffled(self, clumps):
        return [clumps[k] for k in self.rng.permutation(len(clumps))]

    def by_key(self, clumps, descending=False):
        nodes = [init_node(i, c, self.qlen, self.seqs) for i, c in enumerate(clumps)]
        return [clumps[nd.clump] for nd in sorted(nodes, key=lambda nd: nd.key, reverse=descending)]

    def adversarial(self, clumps):
        """The anti-quicksort ordering against a middle pivot, found by playing the sort on slots without values: at every level the middle slot gets the third largest
        key still to be given and the two larger ones go to the two slots the scan meets last, so every partition leaves a right part of two elements waiting while
        all the rest goes left: about n / 3 right parts wait at once.  `clumps` must have distinct keys (ties would leave the order to the draws)."""
        n = len(clumps)
        ranked = self.by_key(clumps)
        nodes = [init_node(i, c, self.qlen, self.seqs) for i, c in enumerate(ranked)]
        assert len({nd.key for nd in nodes}) == n
        a, rank = list(range(n)), [None] * n
        left, right, hi = 0, n - 1, n - 1
        while right - left >= 3:
            p = (left + right) // 2
            a[p], a[right] = a[right], a[p]
            rank[a[right]] = hi - 2; rank[a[right - 1]] = hi - 1; rank[a[right - 2]] = hi
            a[right - 2], a[right] = a[right], a[right - 2]
            right -= 3; hi -= 3
        for k in range(left, right + 1):
            rank[a[k]] = k - left
        assert sorted(rank) == list(range(n))
        return [ranked[rank[i]] for i in range(n)]
