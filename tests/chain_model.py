"""A plain-Python model of the chain stage (A3 + A4) that says which rules it used.

An event recorder first: it is there to say, region by region, which rules of the stage an input exercised.  It is written from SURVEY.md 3.2 and the
reference's QueryMatch.c:146-303 (regions, eliminateFragments, checkStartEndCoverage), GraphPath.cpp:57-292 (the best-chain DP and the repeated extraction) and
AlignHelpers.c:48-193 (insertFragment, cleanUpClump), and it follows those functions step by step -- as oracle/hotpath.cpp does, so the two share the reference's
loop shapes, early-outs and order of checks, and their agreement (test_chain_model.py) is a weak check of either.  What anchors the oracle are the golden files
and the reference binary.  Where the model does differ from the oracle is in how it keeps the data, which is the reference's way:

  * the fragment array is edited in place by the back chop of insertFragment (subLenFromBack on the array's element), the clump holds COPIES, so the front
    chop (subLenFromFront on the list's head) stays in the clump;
  * the coverage is an array of one flag per query base, set by memset(coverage + clumpSQO, TRUE, clumpQueryLen) -- clipped here at the read's length -- and
    read base by base by checkQueryRegion; no interval list;
  * scores and node lengths are int16_t (SINT), query offsets, refLen, matchedBases and clumpQueryLen uint16_t (QOFF / SUINT), diagonals and reference offsets
    uint32_t (ROFF); every store into one of them truncates, and says so below.  A comparison uses the untruncated int where the reference's does
    (`rightNode->bestScore > newScore` with `int newScore`).

Input: the oracle's seed_join tuples (sro, sqo, eqo, refLen, read_strand), the params and the reads' lengths.  Output: the clumps in oracle.chain's format
[(read_strand, ((sro, sqo, eqo, refLen), ...))] in creation order, and one Region per region with its size, the fragment index range it spans and the names of
the events raised while chaining it (EVENTS)."""

EVENTS = (
    # DP pair rejected
    "same_sqo", "over_maxgap", "ref_order", "desert", "no_new_bases",
    # DP accepted
    "gap_cost", "improve",
    # DP tie (equal scores)
    "tie_no_prev", "tie_diag_lose", "tie_diag_win", "tie_gap_lose", "tie_gap_win", "tie_psqo_lose", "tie_psqo_win",
    # best node
    "best_tie_eqo", "best_tie_psqo",
    # insert
    "chop_new", "chop_head", "chop_equal_single", "chop_equal_more", "overlap_ref_only",
    # clean-up
    "mid_removed_between", "mid_removed_band", "mid_kept", "mid_anchor_too_far", "head_removed", "tail_removed",
    # extraction
    "second_clump", "third_clump", "stop_minmatch", "stop_empty", "trim_reused",
    # elimination (of fragments that are not on the path just extracted: those are covered by construction)
    "elim_short", "elim_covered", "kept_start_free", "kept_end_free",
    # arithmetic
    "score_wraps",
)
BIT = {name: 1 << k for k, name in enumerate(EVENTS)}
WORST = -0x7fffff00
U32 = 0xFFFFFFFF


def s16(v):
    v &= 0xFFFF
    return v - 0x10000 if v & 0x8000 else v


def s32(v):
    v &= U32
    return v - 0x100000000 if v & 0x80000000 else v


def u16(v):
    return v & 0xFFFF


def absdiff(a, b):
    return a - b if a > b else b - a


def calc_gap(low, high):
    """calcGap, FragsClumps.inl:158: the bases strictly between two offsets"""
    return high - low - 1 if high > low else 0


def calc_overlap(low, high):
    """calcOverlap, FragsClumps.inl:159"""
    return low - high + 1 if low >= high else 0


class Region:
    __slots__ = ("rs", "start", "end", "size", "events", "clumps", "frags")

    def __init__(self, rs, start, end, frags):
        self.rs, self.start, self.end, self.size, self.events, self.clumps, self.frags = rs, start, end, end - start, set(), [], frags

    @property
    def body(self):
        return size_class(self.size)

    def describe(self):
        return "read %d strand %d: region of %d fragments [%d, %d), class %s, %d clumps, events %s" % (
            self.rs >> 1, self.rs & 1, self.size, self.start, self.end, self.body, len(self.clumps), " ".join(e for e in EVENTS if e in self.events))


def size_class(n):
    """the copy of the algorithm a region of n fragments gets (k_region_classify, regions.h)"""
    if n == 1:
        return "1"
    for top, name in ((4, "2-4"), (8, "5-8"), (16, "9-16"), (64, "17-64"), (512, "65-512")):
        if n <= top:
            return name
    return ">512"


def split_regions(frags, max_gap):
    """runs of consecutive fragments of one (read, strand) whose diagonals differ by at most maxGap from one to the next (findAlignableFragsForw, QueryMatch.c:146-158)"""
    out, start = [], 0
    for k in range(1, len(frags) + 1):
        if k < len(frags):
            a, b = frags[k - 1], frags[k]
            if a[4] == b[4] and absdiff((a[0] - a[1]) & U32, (b[0] - b[1]) & U32) <= max_gap:
                continue
        out.append((start, k))
        start = k
    return out if frags else []


class _Node:
    __slots__ = ("fi", "diag", "len", "best", "prev", "psqo", "sqo", "eqo")


def _frag_qlen(f):
    return 1 + f[2] - f[1]                                                   # fragQueryLen: ints


def _frag_diag(f):
    return (f[0] - f[1]) & U32


def _frag_ero(f):
    return (f[0] + f[3] - 1) & U32


def _best_chain(P, fr, used, ev):
    """buildBestClumpFromFragmentRange, GraphPath.cpp:161-270, up to the best node: returns (nodes in path order from the best node backwards, event bits)"""
    MS, GO, GE, max_gap, max_desert = P.MScore, P.GOCost, P.GECost, P.maxGap, P.maxDesert
    nodes = []
    for fi, f in enumerate(fr):
        if used[fi]:
            continue
        n = _Node()
        n.fi, n.diag, n.sqo, n.eqo, n.prev, n.psqo = fi, _frag_diag(f), f[1], f[2], None, f[1]
        n.len = s16(f[3])                                                    # SINT nodeLength = fragMatchCount
        own = n.len * MS
        if not -32768 <= own <= 32767:
            ev |= BIT["score_wraps"]
        n.best = s16(own)                                                    # SINT bestScore
        nodes.append(n)
    if not nodes:
        return None, ev
    nodes.sort(key=lambda n: (n.sqo, n.diag))                                # compareFragsByQueryOffsets (the keys are unique)
    B_SAME, B_GAP, B_ORDER, B_DESERT, B_NONEW, B_COST, B_IMPROVE = (BIT[k] for k in ("same_sqo", "over_maxgap", "ref_order", "desert", "no_new_bases", "gap_cost", "improve"))
    cnt = len(nodes)
    best_score, best_node = WORST, None
    for i in range(cnt):
        left = nodes[i]
        l_sqo, l_eqo, l_diag, l_best, l_psqo = left.sqo, left.eqo, left.diag, left.best, left.psqo
        l_sro, l_ero = (l_diag + l_sqo) & U32, (l_diag + l_eqo) & U32
        for j in range(cnt - 1, i, -1):
            right = nodes[j]
            r_sqo = right.sqo
            if r_sqo == l_sqo:
                ev |= B_SAME
                break
            r_diag = right.diag
            diag_gap = l_diag - r_diag if l_diag > r_diag else r_diag - l_diag
            if diag_gap > max_gap:
                ev |= B_GAP
                continue
            r_sro = (r_diag + r_sqo) & U32
            if l_sro >= r_sro:
                ev |= B_ORDER
                continue
            if min(calc_gap(l_eqo, r_sqo), calc_gap(l_ero, r_sro)) > max_desert:
                ev |= B_DESERT
                continue
            newbases = right.len - max(calc_overlap(l_eqo, r_sqo), calc_overlap(l_ero, r_sro))
            if newbases < 1:
                ev |= B_NONEW
                continue
            new_score = l_best + newbases * MS                               # int
            if diag_gap > 0:
                new_score -= GO + diag_gap * GE
                ev |= B_COST
            r_best = right.best
            if r_best > new_score:
                continue
            if r_best == new_score:
                prev = right.prev
                if prev is None:
                    ev |= BIT["tie_no_prev"]
                    continue
                dc = s32(diag_gap - absdiff(prev.diag, r_diag))
                if dc > 0:
                    ev |= BIT["tie_diag_lose"]
                    continue
                if dc == 0:
                    gc = s32(calc_gap(l_eqo, r_sqo) - calc_gap(prev.eqo, r_sqo))
                    if gc > 0:
                        ev |= BIT["tie_gap_lose"]
                        continue
                    if gc == 0:
                        if l_psqo <= prev.psqo:
                            ev |= BIT["tie_psqo_lose"]
                            continue
                        ev |= BIT["tie_psqo_win"]
                    else:
                        ev |= BIT["tie_gap_win"]
                else:
                    ev |= BIT["tie_diag_win"]
            else:
                ev |= B_IMPROVE
            if not -32768 <= new_score <= 32767:
                ev |= BIT["score_wraps"]
            right.best, right.prev, right.psqo = s16(new_score), left, l_psqo
        if l_best < best_score:
            continue
        take = l_best > best_score
        if not take:                                                         # differentiateEqualFragNodesDuringBacktrack, GraphPath.cpp:88-94
            if l_eqo != best_node.eqo:
                ev |= BIT["best_tie_eqo"]
                take = l_eqo < best_node.eqo
            else:
                ev |= BIT["best_tie_psqo"]
                take = l_psqo > best_node.psqo
        if take:
            best_node, best_score = left, l_best
    path, n = [], best_node
    while n is not None:
        path.append(n)
        n = n.prev
    return path, ev


def _insert_path(fr, path, ev):
    """insertFragment for every node of the path, back to front (GraphPath.cpp:136-139, AlignHelpers.c:48-90): returns (the clump's list, matchedBases, bits, the
    array fragments that were trimmed)"""
    clump, matched, trimmed = [], 0, []
    for node in path:
        f1 = fr[node.fi]                                                     # the array's element: a chop of it persists
        if clump:
            f2 = clump[0]                                                    # the clump's copy
            o_q, o_r = calc_overlap(f1[2], f2[1]), calc_overlap(_frag_ero(f1), f2[0])
            mo = max(o_q, o_r)
            if mo > 0:
                if o_r > o_q:
                    ev |= BIT["overlap_ref_only"]
                l1, l2 = _frag_qlen(f1), _frag_qlen(f2)
                if l1 != l2:
                    chop1 = l1 < l2
                    ev |= BIT["chop_new"] if chop1 else BIT["chop_head"]
                else:
                    chop1 = len(clump) == 1
                    ev |= BIT["chop_equal_single"] if chop1 else BIT["chop_equal_more"]
                if chop1:                                                    # subLenFromBack
                    f1[2], f1[3] = u16(f1[2] - mo), u16(f1[3] - mo)
                    trimmed.append(node.fi)
                else:                                                        # subLenFromFront
                    f2[1], f2[0], f2[3] = u16(f2[1] + mo), (f2[0] + mo) & U32, u16(f2[3] - mo)
        matched = u16(matched + f1[3])                                       # QOFF matchedBases += fragMatchCount
        clump.insert(0, list(f1))
    return clump, matched, ev, trimmed


def _clean_up(P, clump, ev):
    """cleanUpClump, AlignHelpers.c:92-193, on a Python list (removal by identity)"""
    word, max_gap, bw = P.wordLen, P.maxGap, P.bandWidth

    def nxt(f):
        k = next(i for i, g in enumerate(clump) if g is f)
        return clump[k + 1] if k + 1 < len(clump) else None

    def remove(f):
        del clump[next(i for i, g in enumerate(clump) if g is f)]
    s1 = clump[0]
    s2 = nxt(s1)
    s3 = nxt(s2) if s2 is not None else None
    while s2 is not None and s3 is not None:
        if _frag_qlen(s2) < word:
            anchor = s3
            while _frag_qlen(anchor) < word and nxt(anchor) is not None:
                anchor = nxt(anchor)
            d1, da = _frag_diag(s1), _frag_diag(anchor)
            after = nxt(anchor)
            if absdiff(d1, da) <= max_gap:
                k = next(i for i, g in enumerate(clump) if g is s2)
                for dl in clump[k:next(i for i, g in enumerate(clump) if g is anchor)]:
                    dd = _frag_diag(dl)
                    if not ((dd < d1 and dd < da) or (dd > d1 and dd > da)):
                        ev |= BIT["mid_removed_between"]
                        remove(dl)
                    elif min(absdiff(d1, dd), absdiff(dd, da)) <= bw:
                        ev |= BIT["mid_removed_band"]
                        remove(dl)
                    else:
                        ev |= BIT["mid_kept"]
            else:
                ev |= BIT["mid_anchor_too_far"]
            s1, s2 = anchor, after
        else:
            s1, s2 = s2, s3
        if s2 is not None:
            s3 = nxt(s2)

    def beside(a, b):
        q_gap, r_gap = calc_gap(a[2], b[1]), calc_gap(_frag_ero(a), b[0])
        return (q_gap == 0 and r_gap <= 2 * bw) or (r_gap == 0 and q_gap <= 2 * bw)
    first = clump[0]
    if _frag_qlen(first) < word and len(clump) > 1 and beside(first, clump[1]):
        ev |= BIT["head_removed"]
        del clump[0]
    last = clump[-1]
    if _frag_qlen(last) < word and len(clump) > 1 and beside(clump[-2], last):
        ev |= BIT["tail_removed"]
        del clump[-1]
    return ev


def _eliminate(P, fr, used, coverage, on_path, ev):
    """eliminateFragments / checkStartEndCoverage, QueryMatch.c:170-215"""
    min_left = P.minNonOverlap - 1
    for fi, f in enumerate(fr):
        if used[fi]:
            continue
        sqo, eqo = f[1], f[2]
        mine = fi in on_path
        if eqo - sqo < min_left:
            used[fi] = True
            if not mine:
                ev |= BIT["elim_short"]
            continue
        start_free = not any(coverage[sqo:sqo + min_left + 1])
        end_free = start_free or not any(coverage[eqo - min_left:eqo + 1])
        if start_free:
            ev |= 0 if mine else BIT["kept_start_free"]
        elif end_free:
            ev |= 0 if mine else BIT["kept_end_free"]
        else:
            used[fi] = True
            if not mine:
                ev |= BIT["elim_covered"]
    return ev


def chain_region(P, frags, qlen):
    """processFragmentRangeUsingGraph, GraphPath.cpp:272-292, for one region of two fragments or more: (clumps as lists of (sro, sqo, eqo, refLen), event names)"""
    fr = [[f[0], f[1], f[2], u16(1 + f[2] - f[1])] for f in frags]           # setRefLen
    used = [False] * len(fr)
    coverage = bytearray(qlen)
    ev, clumps, was_trimmed = 0, [], set()
    while True:
        if was_trimmed and any(not used[fi] for fi in was_trimmed):
            ev |= BIT["trim_reused"]
        path, ev = _best_chain(P, fr, used, ev)
        if path is None:
            ev |= BIT["stop_empty"]
            break
        clump, matched, ev, trimmed = _insert_path(fr, path, ev)
        was_trimmed.update(trimmed)
        if matched < P.minMatch:                                             # resetClump: the region is finished
            ev |= BIT["stop_minmatch"]
            break
        ev = _clean_up(P, clump, ev)
        c_sqo = clump[0][1]
        c_len = u16(1 + clump[-1][2] - c_sqo)                                # QOFF clumpQueryLen
        for q in range(c_sqo, min(c_sqo + c_len, qlen)):                     # memset(coverage + start, TRUE, len)
            coverage[q] = 1
        ev = _eliminate(P, fr, used, coverage, {n.fi for n in path}, ev)
        clumps.append(tuple(tuple(f) for f in clump))
        if len(clumps) == 2:
            ev |= BIT["second_clump"]
        elif len(clumps) == 3:
            ev |= BIT["third_clump"]
    return clumps, {name for name in EVENTS if ev & BIT[name]}


def chain(P, frags, read_lengths):
    """the whole stage over one batch's fragments: (clumps in oracle.chain's format, [Region])"""
    out, regions = [], []
    for start, end in split_regions(frags, P.maxGap):
        rs = frags[start][4]
        reg = Region(rs, start, end, [tuple(f[:4]) for f in frags[start:end]])
        if end - start == 1:                                                 # QueryMatch.c:281-290
            f = frags[start]
            ref_len = u16(1 + f[2] - f[1])
            if ref_len >= P.minMatch:
                reg.clumps = [((f[0], f[1], f[2], ref_len),)]
        else:
            reg.clumps, reg.events = chain_region(P, frags[start:end], read_lengths[rs >> 1])
        out.extend((rs, c) for c in reg.clumps)
        regions.append(reg)
    return out, regions


def region_of_clump(regions, clump):
    """the region a clump (read_strand, fragments) came from: its fragments keep their diagonal and lie inside a fragment of the region"""
    rs, cf = clump

    def inside(c, regs):
        return any((c[0] - c[1]) & U32 == (f[0] - f[1]) & U32 and f[1] <= c[1] and c[2] <= f[2] for f in regs)
    for reg in regions:
        if reg.rs == rs and all(inside(c, reg.frags) for c in cf):
            return reg
    return None
