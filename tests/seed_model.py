"""A plain model of the seed stage (A1 + A2) that says which edges of the device's layout an input reaches.

Integer-only and written for clarity.  It is stated from the reference's rules -- Query.c:341-412 (which k-mers enter the join), QueryMatch.c:52-121 (the
hit lists with the wrapping diagonals pre-loaded, the merge in ascending (diagonal, query offset), the coalescing into fragments) and QueryMatch.c:146-158
(what "within maxGap diagonals" means) -- not from the kernels, and it keeps every intermediate: per (read, strand) the kept k-mers, their effective hit
lists, the sorted (diag, qo) multiset and the fragments with their hit counts.  oracle/hotpath.cpp restates the same lines in C++ with one sort and no
intermediates; test_seed_model.py asserts that the two give the same fragments.

Two things here are NOT the reference's:

  * `dead`: a fragment of one hit with no neighbouring fragment of its (read, strand) within maxGap diagonals.  The reference never reports it; the device
    does not write such fragments (seed.h) while wordLen < minMatch.  That dropping them changes no clump is asserted by test_seed_model.py through
    chain_model.py, which is what lets the GPU tests trust this flag.
  * `cut_plan`, `frag_room_after` and the boundary events of `Coverage`: statements about the DEVICE's layout (segsort.h: k_seg_split, k_seg_split_range;
    seed.h: rows of 64, waves of 512 and tiles of 8 192 hits in k_frag_scan_build; stage_seed.hip: the room of the fragment array).  They say which sizes
    an input reaches, never what the result should be.

Input: the index arrays behind a ygpu_index_view (Index), the params, a batch's codes and offsets."""
import ctypes as C

import numpy as np

U32 = 0xFFFFFFFF
COMP4 = (2, 3, 0, 1, 4, 12, 7, 6, 9, 8, 15, 11, 5, 13, 14, 10)                # fourBitCompCodes, Math.c:156
ROW, WAVE, TILE = 64, 512, 8192                                             # k_frag_scan_build: a row of lanes, a wave's eight rows, a workgroup's tile
CLASS_HI = (1024, 2048, 3072, 4096, 5120, 6144, 7168, 8192, 10240, 12288, 14336, 15872)   # the workgroup sort's twelve shapes (stage_seed.hip: kShape)
SEGSORT_MAX = CLASS_HI[-1]
SPLIT_NB, SPLIT_PER_BUCKET = 16, 6144                                       # k_seg_split
BOUNDARY_EVENTS = ("frag_across", "dead_before", "dead_behind", "rs_change", "near_not_joined")


class Index:
    """the arrays of a ygpu_index_view: SO (4^wordLen + 1 list starts), ROA (the reference offsets, list after list), totalMatches, wordLen, maxROff"""

    def __init__(self, view):
        self.word, self.total, self.max_roff = int(view.wordLen), int(view.totalMatches), int(view.maxROff)
        self.SO = np.ctypeslib.as_array(C.cast(view.startingOffs, C.POINTER(C.c_uint32)), shape=((1 << (2 * self.word)) + 1,))
        self.ROA = np.ctypeslib.as_array(C.cast(view.ROA, C.POINTER(C.c_uint32)), shape=(max(self.total, 1),))


def strand_codes(codes, strand):
    """the codes a strand is looked up with: the read, or its reverse complement (Query.c:161-167)"""
    return list(codes) if strand == 0 else [COMP4[c & 15] for c in reversed(codes)]


def window_lists(ix, codes):
    """every window of wordLen codes of an array: (its list's start in ROA, the list's length -- 0 where the window holds a code above 3 --, that flag)"""
    L = ix.word
    n = max(len(codes) - L + 1, 0)
    c = np.asarray(codes, dtype=np.int64)
    h, bad = np.zeros(n, dtype=np.int64), np.zeros(n, dtype=bool)
    for k in range(L):                                                      # the hash: two bits a base, the first base highest
        w = c[k:k + n]
        h, bad = (h << 2) | (w & 3), bad | (w > 3)
    start = ix.SO[h].astype(np.int64)
    count = ix.SO[h + 1].astype(np.int64) - start
    count[bad] = 0
    return start, count, bad


class KmerTable:
    """Query.c:341-412 over a whole array of codes at once: which windows' lists enter the join.  A k-mer is dropped when its window holds a code above 3 (no
    lookup) or its list is longer than maxHits; an empty list enters nothing.  The array may hold many reads one behind the other (a batch of 65 536 is then
    one pass, not 131 072): a read asks for its own windows only, so a window across two reads is never looked at."""

    def __init__(self, ix, P, codes):
        start, count, bad = window_lists(ix, codes)
        kept = (count > 0) & (count <= P.maxHits)
        at = np.nonzero(kept)[0]
        self.at, self.start, self.count = at.tolist(), start[at].tolist(), count[at].tolist()
        self.edges = (P.maxHits, P.maxHits + 1)
        self.sums = {"kept": _running(kept), "bad": _running(bad)}                          # how many such windows lie before each window
        self.sums.update((m, _running(count == m)) for m in self.edges)

    def windows(self, a, n):
        """of the n windows from a on: ([(query offset, list start, count)] of the kept ones, table lookups made, {count: k-mers} around maxHits)"""
        if n <= 0:
            return [], 0, {}
        lo, hi = int(self.sums["kept"][a]), int(self.sums["kept"][a + n])
        kmers = [(p - a, s, c) for p, s, c in zip(self.at[lo:hi], self.start[lo:hi], self.count[lo:hi])]
        return kmers, n - self._in("bad", a, n), {m: self._in(m, a, n) for m in self.edges}

    def _in(self, what, a, n):
        return int(self.sums[what][a + n] - self.sums[what][a])


def _running(flags):
    return np.concatenate(([0], np.cumsum(flags, dtype=np.int64)))


def kept_kmers(ix, P, codes):
    """the kept k-mers of one strand (KmerTable.windows over its own codes)"""
    return KmerTable(ix, P, codes).windows(0, len(codes) - ix.word + 1)


def effective_list(ix, i, s, cnt):
    """QueryMatch.c:56-69: the entries of ROA that k-mer i brings into the merge: (how many from s on, how many of them wrap, whether the end of ROA cut it).
    Hits with a reference offset below the query offset (their diagonal wraps below zero) are pre-loaded one by one until the first that does not wrap, which
    the merge then continues from: all cnt entries when fewer than cnt wrap, else the w wrapping ones and the one behind them -- entries of the NEXT lists
    when the whole list wraps.  The reference reads past the end of ROA there; here (as in the oracle and on the device) the array's end stops it."""
    w = 0
    while s + w < ix.total and int(ix.ROA[s + w]) < i:
        w += 1
    eff = cnt if w < cnt else w + 1
    clamped = s + eff > ix.total
    if clamped:
        eff = ix.total - s
    return eff, w, clamped


class Strand:
    """one (read, strand): its hits in the order the k-mers give them, sorted, and as fragments"""
    __slots__ = ("rs", "kmers", "lookups", "edge", "hits", "sorted", "frags", "nhits", "hit_frag", "dead", "wrapped", "all_wrap", "foreign", "clamped")


def strand_model(ix, P, codes, rs, kmers=None):
    """one (read, strand) from its codes, or from what kept_kmers gives for them"""
    S = Strand()
    S.rs = rs
    S.kmers, S.lookups, S.edge = kmers if kmers is not None else kept_kmers(ix, P, codes)
    S.hits, S.wrapped, S.all_wrap, S.foreign, S.clamped = [], 0, 0, 0, 0
    for i, s, cnt in S.kmers:
        eff, w, clamped = effective_list(ix, i, s, cnt)
        S.wrapped += w
        S.all_wrap += w >= cnt
        S.foreign += max(eff - cnt, 0)
        S.clamped += clamped
        for ro in ix.ROA[s:s + eff].tolist():
            S.hits.append(((ro - i) & U32, i))                               # (diagonal as ROFF: wraps, query offset)
    S.sorted = sorted(S.hits)                                               # the heap pops ascending (diag << 32) + qo, QueryHeap.inl:70-73
    # QueryMatch.c:76-119: a hit goes on with the current fragment when it is on its diagonal and its k-mer overlaps or abuts the last one's
    L = ix.word
    S.frags, S.nhits, S.hit_frag = [], [], []
    cur_diag = cur_sqo = cur_end = None
    for d, q in S.sorted:
        if cur_diag is None or d != cur_diag or q > cur_end:
            if cur_diag is not None:
                S.frags.append(((cur_diag + cur_sqo) & U32, cur_sqo, cur_end - 1, cur_end - cur_sqo, rs))
            cur_diag, cur_sqo = d, q
            S.nhits.append(0)
        cur_end = q + L
        S.nhits[-1] += 1
        S.hit_frag.append(len(S.nhits) - 1)
    if cur_diag is not None:
        S.frags.append(((cur_diag + cur_sqo) & U32, cur_sqo, cur_end - 1, cur_end - cur_sqo, rs))
    # dead: one hit, and no neighbouring fragment of this (read, strand) within maxGap diagonals (absDiagDiff of QueryMatch.c:146-158 on ascending diagonals)
    diag = [(f[0] - f[1]) & U32 for f in S.frags]
    can_die = P.wordLen < P.minMatch
    S.dead = [can_die and S.nhits[k] == 1 and (k == 0 or diag[k] - diag[k - 1] > P.maxGap) and (k + 1 == len(diag) or diag[k + 1] - diag[k] > P.maxGap)
              for k in range(len(diag))]
    return S


class Batch:
    """a batch through the model: .strands in (read, strand) order, .frags (the oracle's seed_join format), .dead (a flag per fragment), .kept"""

    def __init__(self, ix, P, codes, offs):
        self.P, self.strands = P, []
        offs = [int(o) for o in offs]
        fwd = np.asarray(codes)[offs[0]:offs[-1]]
        rev = np.asarray(COMP4)[fwd[::-1] & 15]                              # the whole batch reverse-complemented: the last read comes first
        tables, end = (KmerTable(ix, P, fwd), KmerTable(ix, P, rev)), offs[-1]
        for r in range(len(offs) - 1):
            n = offs[r + 1] - offs[r] - ix.word + 1
            self.strands.append(strand_model(ix, P, None, 2 * r, tables[0].windows(offs[r] - offs[0], n)))
            self.strands.append(strand_model(ix, P, None, 2 * r + 1, tables[1].windows(end - offs[r + 1], n)))
        self.frags = [f for S in self.strands for f in S.frags]
        self.dead = [d for S in self.strands for d in S.dead]
        self.kept = [f for f, d in zip(self.frags, self.dead) if not d]
        self.n_hits = sum(len(S.hits) for S in self.strands)
        self.lookups = sum(S.lookups for S in self.strands)


# ---- the device's layout: which cuts a long segment gets ----------------------------------------------------------------------------------------------------
def cut_plan(diags, seg_max, max_roff):
    """A statement about the DEVICE (segsort.h), not the reference: how a segment of more than seg_max hits is cut.  k_seg_split: 1 << lg buckets of about
    6 144 hits by the diagonal's top bits (of the bits maxROff has), diagonals beyond them -- the wrapped ones -- clamped into the last bucket.  A bucket
    still above seg_max goes to k_seg_split_range, level by level: sixteen buckets over the piece's own range of diagonals, a piece of ONE diagonal copied as
    it stands.  Returns dict(nb, clamped, first_single: first-cut pieces above seg_max that hold one diagonal, levels: [(pieces cut again, of their buckets still
    too long)] per level of k_seg_split_range, copies: the levels at which a one-diagonal piece was met)."""
    n = len(diags)
    lg = 0
    while lg < 4 and (n + SPLIT_PER_BUCKET - 1) // SPLIT_PER_BUCKET > (1 << lg):
        lg += 1
    nb = 1 << lg
    diag_bits = 1
    while diag_bits < 32 and (max_roff >> diag_bits):
        diag_bits += 1
    sh = max(diag_bits - lg, 0)
    buckets = [[] for _ in range(nb)]
    clamped = 0
    for d in diags:
        clamped += (d >> sh) > nb - 1
        buckets[min(d >> sh, nb - 1)].append(d)
    over = [b for b in buckets if len(b) > seg_max]
    plan = dict(nb=nb, clamped=clamped, first_single=sum(1 for b in over if min(b) == max(b)), levels=[], copies=[])
    while over:
        nxt = []
        for piece in over:
            mn, mx = min(piece), max(piece)
            if mn == mx:
                plan["copies"].append(len(plan["levels"]))
                continue
            sub = [[] for _ in range(SPLIT_NB)]
            for d in piece:
                sub[(d - mn) * SPLIT_NB // (mx - mn + 1)].append(d)
            nxt.extend(s for s in sub if len(s) > seg_max)
        plan["levels"].append((len(over), len(nxt)))
        over = nxt
    return plan


def frag_room_after(n_frags):
    """A statement about the DEVICE (stage_seed.hip: buildFrags; ctx.h: DevBuf::ensure): the fragments a context's array holds once a batch of n_frags
    fragments has made it grow from nothing.  buildFrags asks for 16 bytes each of n + n / 8 + 4 096 records, ensure adds a quarter and 256 bytes, and one
    record stays free.  A later batch with more fragments than this is written as far as the room goes, counted, and run again in a larger array."""
    asked = 16 * (n_frags + n_frags // 8 + 4096)
    return (asked + asked // 4 + 256) // 16 - 1


class Coverage:
    """What a batch reaches, for a given segSortMax.  The reference's side: .seg_hits {rs: hits}, .max_on_diag {rs: most hits on one diagonal}, the lookup
    counts (.wrapped hits, .all_wrap k-mers whose whole list wraps, .foreign entries taken from the lists behind, .clamped walks stopped by the end of ROA,
    .at_max / .over_max k-mers with exactly maxHits / maxHits + 1 hits), .max_qo, .max_eqo, .max_rs.  The device's side: .seg_base {rs: index of its first hit
    in the batch-wide order}, .plans {rs: cut_plan} of the segments above seg_max, .cut_levels (the batch's totals per level, as the library's trace prints
    them), .events {(64 | 512 | 8192, name): [hit index]} -- BOUNDARY_EVENTS at the multiples of a row that are no multiple of a wave, of a wave that are no
    multiple of a tile, and of a tile."""

    def __init__(self, ix, batch, seg_max=SEGSORT_MAX):
        P = batch.P
        self.n_hits, self.seg_hits, self.seg_base, self.max_on_diag, self.plans = batch.n_hits, {}, {}, {}, {}
        self.wrapped = sum(S.wrapped for S in batch.strands)
        self.all_wrap = sum(S.all_wrap for S in batch.strands)
        self.foreign = sum(S.foreign for S in batch.strands)
        self.clamped = sum(S.clamped for S in batch.strands)
        self.at_max = sum(S.edge.get(P.maxHits, 0) for S in batch.strands)
        self.over_max = sum(S.edge.get(P.maxHits + 1, 0) for S in batch.strands)
        self.max_qo = max([q for S in batch.strands for _d, q in S.hits] + [-1])
        self.max_eqo = max([f[2] for f in batch.frags] + [-1])
        self.max_rs = max([S.rs for S in batch.strands if S.hits] + [-1])
        hit_rs, hit_diag, hit_frag, frag_dead = [], [], [], []
        for S in batch.strands:
            n = len(S.sorted)
            if not n:
                continue
            self.seg_hits[S.rs], self.seg_base[S.rs] = n, len(hit_rs)
            run = best = 0
            for k, (d, _q) in enumerate(S.sorted):
                run = run + 1 if k and d == S.sorted[k - 1][0] else 1
                best = max(best, run)
            self.max_on_diag[S.rs] = best
            if n > seg_max:
                self.plans[S.rs] = cut_plan([d for d, _q in S.hits], seg_max, ix.max_roff)
            base = len(frag_dead)
            hit_rs.extend([S.rs] * n)
            hit_diag.extend(d for d, _q in S.sorted)
            hit_frag.extend(base + k for k in S.hit_frag)
            frag_dead.extend(S.dead)
        depth = max([len(p["levels"]) for p in self.plans.values()] + [0])
        self.cut_levels = [tuple(sum(p["levels"][lv][k] for p in self.plans.values() if lv < len(p["levels"])) for k in (0, 1)) for lv in range(depth)]
        self.events = {}
        for B in range(ROW, len(hit_rs), ROW):
            level = TILE if B % TILE == 0 else (WAVE if B % WAVE == 0 else ROW)
            a, b = B - 1, B
            found = (hit_frag[a] == hit_frag[b], frag_dead[hit_frag[a]], frag_dead[hit_frag[b]], hit_rs[a] != hit_rs[b],
                     hit_rs[a] == hit_rs[b] and hit_frag[a] != hit_frag[b] and hit_diag[b] - hit_diag[a] <= P.maxGap)
            for name, yes in zip(BOUNDARY_EVENTS, found):
                if yes:
                    self.events.setdefault((level, name), []).append(B)
