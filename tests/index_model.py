"""A plain model of the hash-index file, stated from the reference's own loops: the sequential scan of Index.c:98-128 / 201-242 (count pass and fill pass run the
same loop), the sampling pass of Index.c:271-315, and Math.c's default-seeded Marsaglia generator with the modified Floyd sample (Math.c:257-343).  It is what the
device build (device/index_build.hip) is held against, and on purpose it is NOT stated from that file's walkKmers or from host/formats.cpp: the device restates the
`-S` scan in closed form (`(s - segStart) % S` before the sequence's first bad code, `s % S` after it) and this file keeps the loop, with its `baseOff`, its
`badOffset` and its re-phasing to `((badOffset + S-1) / S) * S` behind a run of codes above 3.

Input: the bytes of a `.nib2` as the command line writes it (version 2 header, 4-bit codes, high nibble first, every sequence on a byte boundary), wordLen, skipDist,
maxHits.  Output: the complete image {-1, wordLen, maxHits, total} + startingOffs[4^k + 1] + ROA as bytes, and a Coverage that says what the input reaches.

Two things the reference leaves open are fixed here the way the project fixes them.  A sequence shorter than wordLen holds no k-mer (the reference's unsigned
`endingOffset` wraps there and it reads whatever follows; tests leave such genomes out of the comparison with the reference binary).  The skip over a run of bad
codes stops at the end of the base array (the reference reads on into the bytes behind its mapping).

Only what the loop READS is tabulated ahead with numpy -- the next bad code at or behind an offset, the next good one, the 2-bit value of every window of wordLen and
of skipDist codes -- so that generateMatches4to2Fast is one look-up; which offsets are visited, in which order, is decided by the loop alone."""
import struct
from collections import Counter

import numpy as np

IX_PER_THREAD = 16
IX_WG = 256 * IX_PER_THREAD            # offsets a workgroup of the walk covers
IX_SMALL = 32
IX_BLOCK = 8192


class Genome:
    def __init__(self, codes, seqs):
        self.codes = codes                                                   # one uint8 per offset, padding included
        self.seqs = seqs                                                     # (start offset, length, name), ascending


def parse_nib2(buf):
    magic, version, base_off, n = struct.unpack_from("<4I", buf, 0)
    assert magic == 0x01020304 and version == 2
    names_at = 16 + 16 * n + 4
    seqs = []
    for i in range(n):
        start_byte, length, name_off, name_len = struct.unpack_from("<4I", buf, 16 + 16 * i)
        seqs.append((2 * start_byte, length, buf[names_at + name_off:names_at + name_off + name_len].decode()))
    b = np.frombuffer(buf, dtype=np.uint8, offset=base_off)
    codes = np.empty(2 * len(b), dtype=np.uint8)
    codes[0::2] = b >> 4; codes[1::2] = b & 15
    return Genome(codes, seqs)


# ---- Math.c:257-343 ------------------------------------------------------------------------------------------------------------------------------------------
class Rand:
    def __init__(self):
        self.s = [123456789, 362436069, 521288629, 88675123, 886756453]

    def bits(self):
        s = self.s
        t = s[0] ^ (s[0] >> 7)
        s[0], s[1], s[2], s[3] = s[1], s[2], s[3], s[4]
        s[4] = ((s[4] ^ (s[4] << 6)) ^ (t ^ (t << 13))) & 0xFFFFFFFF
        return ((s[1] + s[1] + 1) * s[4]) & 0xFFFFFFFF

    def uint(self, start, end):
        return start + int((self.bits() / 4294967296.0) * float(end - start))


def rand_sample(rs, inp, out_len):
    """getRandSample: out_len of inp without replacement, in inp's order"""
    in_len = len(inp)
    marked = [False] * in_len
    keep_marked, select = True, out_len
    if out_len > in_len // 2:
        keep_marked, select = False, in_len - out_len
    for i in range(in_len - select, in_len):
        pos = rs.uint(0, i + 1)
        if marked[pos]:
            marked[i] = True
        else:
            marked[pos] = True
    return [inp[i] for i in range(in_len) if marked[i] == keep_marked]


# ---- Index.c:98-128 ------------------------------------------------------------------------------------------------------------------------------------------
class Scan:
    """what the loop visited: (hash, offset) in visiting order, and per sequence (index, first bad code or None, [(run end, new baseOff, visited anything after)])"""
    def __init__(self):
        self.hashes = []; self.offsets = []; self.per_seq = []


def _tables(G, k, S):
    c = G.codes; n = len(c)
    bad = c > 3
    idx = np.arange(n, dtype=np.int64)
    next_bad = np.full(n + k + 1, n, dtype=np.int64)
    nb = np.where(bad, idx, n)
    next_bad[:n] = np.minimum.accumulate(nb[::-1])[::-1] if n else nb
    next_good = np.full(n + k + 1, n, dtype=np.int64)
    ng = np.where(~bad, idx, n)
    next_good[:n] = np.minimum.accumulate(ng[::-1])[::-1] if n else ng
    v = np.zeros(n + k, dtype=np.uint64); v[:n] = c & 3

    def windows(w):
        h = np.zeros(n, dtype=np.uint64)
        for i in range(w):
            h = (h << np.uint64(2)) + v[i:i + n]
        return h
    return next_bad, next_good, windows(k), windows(S)


def scan(G, k, S):
    next_bad, next_good, hk, hs = _tables(G, k, S)
    next_bad = next_bad.tolist(); next_good = next_good.tolist(); hk = hk.tolist(); hs = hs.tolist()
    mask = 0xFFFFFFFF >> (32 - 2 * k)
    save = k - S
    out = Scan(); H = out.hashes; O = out.offsets

    def gen(off, length):                                                    # generateMatches4to2Fast: (0, hash) or (1 past the offending offset, None)
        b = next_bad[off]
        if b < off + length:
            return b + 1, None
        return 0, (hk[off] if length == k else hs[off])

    hash_code = 0
    for si, (start, length, _name) in enumerate(G.seqs):
        if length < k:
            continue
        base = start; ending = start + length - k
        fb = next_bad[start]; fb = fb if fb < start + length else None
        runs = []
        bad_off, h = gen(base, k)
        if h is not None:
            hash_code = h
        while True:
            if bad_off != 0:
                bad_off = next_good[bad_off]                                 # get rid of all the bad ones in a row
                base = ((bad_off + (S - 1)) // S) * S                        # renormalize to a multiple of skipDist
                runs.append([bad_off, base, False])
                if base > ending:
                    break
                bad_off, h = gen(base, k)
                if h is not None:
                    hash_code = h
                continue
            H.append(hash_code); O.append(base)
            if runs:
                runs[-1][2] = True
            base += S
            if base > ending:
                break
            bad_off, partial = gen(base + save, S)
            if partial is not None:
                hash_code = ((hash_code << (2 * S)) | partial) & mask
        out.per_seq.append((si, fb, runs))
    return out


class Index:
    def __init__(self, k, max_hits, counts, so, roa, so2, roa2, n_over):
        self.k = k; self.max_hits = max_hits
        self.counts = counts                                                 # before sampling
        self.so = so; self.roa = roa                                         # before sampling
        self.so2 = so2; self.roa2 = roa2                                     # the file's
        self.n_over = n_over

    def image(self):
        head = np.array([0xFFFFFFFF, self.k, self.max_hits, len(self.roa2)], dtype="<u4")
        return head.tobytes() + self.so2.astype("<u4").tobytes() + self.roa2.astype("<u4").tobytes()


def build(G, k, S, max_hits, sc=None):
    sc = sc or scan(G, k, S)
    HT = 4 ** k
    h = np.array(sc.hashes, dtype=np.int64); o = np.array(sc.offsets, dtype=np.uint32)
    counts = np.bincount(h, minlength=HT).astype(np.int64)
    so = np.zeros(HT + 1, dtype=np.int64); np.cumsum(counts, out=so[1:])
    roa = o[np.argsort(h, kind="stable")]                                    # the fill pass: every list in visiting order
    # third pass: the over-represented k-mers in ascending order, one generator for all of them
    over = np.nonzero(counts > max_hits)[0]
    c2 = np.minimum(counts, max_hits)
    so2 = np.zeros(HT + 1, dtype=np.int64); np.cumsum(c2, out=so2[1:])
    keep = np.ones(len(roa), dtype=bool)
    rs = Rand()
    for i in over.tolist():
        b, e = int(so[i]), int(so[i + 1])
        lst = list(range(b, e))
        kept = rand_sample(rs, lst, max_hits)
        keep[b:e] = False; keep[kept] = True
    roa2 = roa[keep]
    assert len(roa2) == so2[HT]
    return Index(k, max_hits, counts, so, roa, so2, roa2, len(over))


def list_class(n, huge_min=IX_BLOCK):
    """which kernel of index_build.hip orders a list of n entries"""
    if n < 2:
        return "none"
    if n <= IX_SMALL:
        return "one thread (k_ix_order_small)"
    if n <= huge_min:
        return "workgroup in LDS (k_ix_order_block)"
    return "bitonic network over a padded copy (k_ix_bitonic_*)"


def padded_size(n):
    m = 64
    while m < n:
        m <<= 1
    return m


def first_difference(model_bytes, file_bytes, k, counts, huge_min=IX_BLOCK):
    """None when equal; else a sentence that names the first differing k-mer, its list length and its class"""
    if model_bytes == file_bytes:
        return None
    HT = 4 ** k
    a = np.frombuffer(model_bytes, dtype="<u4"); b = np.frombuffer(file_bytes[:len(file_bytes) // 4 * 4], dtype="<u4")
    if len(a) != len(b):
        return "file of %d words, model of %d (header: file %s, model %s)" % (len(b), len(a), b[:4].tolist(), a[:4].tolist())
    w = int(np.nonzero(a != b)[0][0])
    if w < 4:
        return "header word %d: file %d, model %d" % (w, b[w], a[w])
    if w < 4 + HT + 1:
        h = w - 4
        return "startingOffs[%d]: file %d, model %d (k-mer %d has %d entries before sampling)" % (h, b[w], a[w], max(h - 1, 0), counts[max(h - 1, 0)])
    r = w - (4 + HT + 1)
    so2 = a[4:4 + HT + 1]
    h = int(np.searchsorted(so2, r, side="right")) - 1
    n = int(counts[h])
    lo = int(so2[h]); hi = int(so2[h + 1])
    return "ROA[%d], entry %d of k-mer %d (%d entries before sampling, %d in the file; ordered by: %s): file %d, model %d; the list in the file %s, in the model %s" % (
        r, r - lo, h, n, hi - lo, list_class(n, huge_min), b[w], a[w], b[4 + HT + 1 + lo:4 + HT + 1 + hi][:12].tolist(), a[4 + HT + 1 + lo:4 + HT + 1 + hi][:12].tolist())


# ---- what an input reaches --------------------------------------------------------------------------------------------------------------------------------
class Coverage:
    """Facts about one genome under one (wordLen, skipDist, maxHits), in the terms of index_build.hip: spans of 16 offsets a thread, 4 096 a workgroup."""
    def __init__(self, G, k, S, max_hits, sc, ix):
        c = G.codes; n = len(c)
        self.k, self.S, self.max_hits = k, S, max_hits
        self.n_offsets = n
        self.end_of_bases = max((s + l for s, l, _ in G.seqs), default=0)
        # -- the walk
        self.len_minus_k = {l - k for _s, l, _n in G.seqs}
        spans = Counter()
        for s, l, _ in G.seqs:
            if l:
                for sp in range(s // IX_PER_THREAD, (s + l - 1) // IX_PER_THREAD + 1):
                    spans[sp] += 1
        self.max_seqs_in_a_span = max(spans.values(), default=0)
        self.seqs_in_a_span = set(spans.values())
        kept = [(s, l) for s, l, _ in G.seqs if l >= k]
        kspans = Counter()
        for s, l in kept:
            for sp in range(s // IX_PER_THREAD, (s + l - 1) // IX_PER_THREAD + 1):
                kspans[sp] += 1
        self.kept_seqs_in_a_span = set(kspans.values())
        self.start_mod_16 = {s % 16 for s, l, _ in G.seqs if l}
        self.last_base_mod_16 = {(s + l - 1) % 16 for s, l, _ in G.seqs if l}
        self.odd_lengths = sum(1 for _s, l, _ in G.seqs if l & 1)
        self.last_is_odd = bool(G.seqs and G.seqs[-1][1] & 1)
        self.bad_places = {}                                                # place -> kinds of code seen there ("N", "iupac")
        self.all_n_seqs = 0; self.no_clean_window_seqs = 0; self.clean_seqs = 0
        self.run_end_vs_S = set()                                           # where the first good code behind a run lies: "multiple", "one_before", "one_after"
        self.fb_in_first_window = 0; self.fb_far = 0
        fb_spans = Counter()
        for s, l, _ in G.seqs:
            if not l:
                continue
            seg = c[s:s + l]; bad = seg > 3
            if not bad.any():
                self.clean_seqs += 1
                continue
            if (seg == 4).all():
                self.all_n_seqs += 1
            good_run = 0; best = 0
            for g in (~bad).tolist():
                good_run = good_run + 1 if g else 0
                best = max(best, good_run)
            if l >= k and best < k and (~bad).any():
                self.no_clean_window_seqs += 1
            pos = np.nonzero(bad)[0]
            fb = s + int(pos[0])
            if l >= k:
                fb_spans[fb // IX_PER_THREAD] += 1
                if fb < s + k:
                    self.fb_in_first_window += 1
                if fb - s > IX_WG:
                    self.fb_far += 1
            # maximal runs
            brk = np.nonzero(np.diff(pos) > 1)[0]
            r0 = np.concatenate(([0], brk + 1)); r1 = np.concatenate((brk, [len(pos) - 1]))
            for a, b in zip(pos[r0].tolist(), pos[r1].tolist()):
                a += s; b += s                                               # the run is [a, b]
                kinds = {"N" if x == 4 else "iupac" for x in c[a:b + 1].tolist()}
                places = []
                if a == s: places.append("first_base")
                if b == s + l - 1: places.append("last_base")
                if any(p % 16 == 0 for p in range(a, min(b, a + 16) + 1)): places.append("span_offset_0")
                if any(p % 16 == 15 for p in range(a, min(b, a + 16) + 1)): places.append("span_offset_15")
                if a // 16 != b // 16: places.append("crosses_a_span")
                if a // IX_WG != b // IX_WG: places.append("crosses_a_workgroup")
                for p in places:
                    self.bad_places.setdefault(p, set()).update(kinds)
                e = b + 1
                if b < s + l - 1 and S > 1:
                    self.run_end_vs_S.update(w for w, r in (("multiple", 0), ("one_before", S - 1), ("one_after", 1)) if e % S == r)      # (S = 2: the last two are one)
        self.max_first_bads_in_a_span = max(fb_spans.values(), default=0)
        # -- the scan
        starts = {G.seqs[si][0] for si, _fb, _r in sc.per_seq}
        self.start_mod_S = {s % S for s in starts}
        self.window_ends_at_first_bad = 0; self.rephase_changes_residue = 0; self.max_runs_with_visits = 0
        visited = np.array(sc.offsets, dtype=np.int64)
        for si, fb, runs in sc.per_seq:
            s, l, _ = G.seqs[si]
            if fb is not None:
                lo = np.searchsorted(visited, s); hi = np.searchsorted(visited, s + l)
                mine = visited[lo:hi]
                if ((mine + k) == fb).any():
                    self.window_ends_at_first_bad += 1
                if s % S != 0 and (mine > fb).any() and (mine < fb).any():
                    self.rephase_changes_residue += 1
            self.max_runs_with_visits = max(self.max_runs_with_visits, sum(1 for r in runs if r[2]))
        # -- the lists
        cnt = ix.counts
        self.list_lengths = set(np.unique(cnt).tolist())
        self.len_hash_0 = int(cnt[0]); self.len_hash_max = int(cnt[-1])
        long_ = np.nonzero(cnt > IX_SMALL)[0]
        self.workgroups_of_long_lists = {int(cnt[h]): len(set((ix.roa[int(ix.so[h]):int(ix.so[h + 1])] // IX_WG).tolist())) for h in long_.tolist()}
        self._lengths = Counter(cnt[cnt > 1].tolist())
        self.n_long = int((cnt > IX_SMALL).sum())                            # entries of the device's bigList
        # -- sampling and compaction
        self.n_over = ix.n_over
        self.sampled_lengths = set(np.unique(cnt[cnt > max_hits]).tolist())
        self.hash_0_sampled = self.len_hash_0 > max_hits; self.hash_max_sampled = self.len_hash_max > max_hits
        wave_copied = np.nonzero((cnt > IX_SMALL) & (cnt <= max_hits))[0]     # k_ix_compact: copied by the whole wave (only runs when something is sampled)
        self.wave_copy_lanes = {int(h) & 63 for h in wave_copied.tolist()} if ix.n_over else set()
        per_wave = Counter(int(h) >> 6 for h in wave_copied.tolist())
        self.max_wave_copies_in_a_wave = max(per_wave.values(), default=0) if ix.n_over else 0
        self.unsampled_lengths = set(np.unique(cnt[cnt <= max_hits]).tolist())
        self.over_lengths = cnt[cnt > max_hits].tolist()                     # in k-mer order: the order of the generator and of the transfer groups

    def classes(self, huge_min=IX_BLOCK):
        out = Counter()
        for n, times in self._lengths.items():
            out[list_class(n, huge_min)] += times
        return out

    def network_sizes(self, huge_min=IX_BLOCK):
        """padded sizes m of the lists that take the multi-launch network"""
        return {padded_size(n) for n in self._lengths if n > huge_min}

    def transfer_groups(self, group_cap):
        """the over-represented lists as the device's host loop groups them: at most group_cap entries and group_cap samples a group, a list alone if it is larger"""
        groups = []; cur = []; tot = 0
        for n in self.over_lengths:
            if cur and (tot + n > group_cap or (len(cur) + 1) * self.max_hits > group_cap):
                groups.append(cur); cur = []; tot = 0
            cur.append(n); tot += n
        if cur:
            groups.append(cur)
        return groups


def model(nib2_bytes, k, S, max_hits):
    """(image bytes, Coverage, Index) of one genome under one option list"""
    G = parse_nib2(nib2_bytes)
    sc = scan(G, k, S)
    ix = build(G, k, S, max_hits, sc)
    return ix.image(), Coverage(G, k, S, max_hits, sc, ix), ix
