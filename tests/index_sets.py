"""Directed genomes for the index build (device/index_build.hip), each at most a few hundred kbp, from a seeded generator, with the option lists (wordLen, skipDist,
maxHits) each is meant for.  What each reaches is not claimed here but measured by index_model.Coverage and asserted in tests/test_index_model.py.

Two kinds of file.  FASTA, which the command line compresses itself: there every sequence starts on a multiple of 8 offsets (the `.nib2` writer pads every sequence
to four bytes), so a sequence start can only be 0 or 8 mod 16.  And `.nib2` files written here with the sequences on consecutive BYTE boundaries, which the format
allows and both loaders take: starts at every even residue, two and three whole sequences inside one thread's span of 16 offsets.  (An odd start cannot be written:
the header counts bytes.)"""
import os
import struct

import numpy as np

import index_model

LETTERS = "TCAGNBDHKMRSVWXY"                                                 # 4-bit code -> letter (Math.c)
T, Cc, A, Gg, N = 0, 1, 2, 3, 4
DEFAULT_H = 65525


class GenomeSet:
    def __init__(self, name, seqs, options, tight=False):
        self.name = name; self.seqs = [np.asarray(s, dtype=np.uint8) for s in seqs]; self.options = options; self.tight = tight
        self.ext = ".nib2" if tight else ".fa"

    def data(self):
        return tight_nib2(self.seqs) if self.tight else fasta(self.seqs)

    def write(self, directory):
        p = os.path.join(directory, self.name + self.ext)
        with open(p, "wb") as f:
            f.write(self.data())
        return p


def fasta(seqs):
    out = []
    for i, s in enumerate(seqs):
        out.append(">s%d set" % i)
        text = "".join(LETTERS[c] for c in s.tolist())
        out.extend(text[j:j + 60] for j in range(0, len(text), 60))
    return ("\n".join(out) + "\n").encode()


def tight_nib2(seqs):
    """version 2 `.nib2`, the sequences one behind the other on byte boundaries (an odd one ends with the pad nibble 14), the base array padded to four bytes with 0xEE"""
    names = [("s%d" % i).encode() for i in range(len(seqs))]
    body = bytearray(); ent = []; name_off = 0
    for s, nm in zip(seqs, names):
        c = s.tolist()
        ent.append((len(body), len(c), name_off, len(nm))); name_off += len(nm)
        if len(c) & 1:
            c = c + [14]
        body.extend((c[j] << 4) | c[j + 1] for j in range(0, len(c), 2))
    while len(body) & 3:
        body.append(0xEE)
    name_block = b"".join(names); name_block += b"\0" * (-len(name_block) & 3)
    pre = 20 + 16 * len(seqs) + len(name_block)
    return struct.pack("<4I", 0x01020304, 2, pre, len(seqs)) + b"".join(struct.pack("<4I", *e) for e in ent) + struct.pack("<I", 0) + name_block + bytes(body)


def background(rnd, n):
    """random T/C/A/G without four equal bases in a row (no accidental homopolymer word)"""
    b = rnd.integers(0, 4, size=n).astype(np.uint8)
    for i in range(3, n):
        if b[i] == b[i - 1] == b[i - 2] == b[i - 3]:
            b[i] = (b[i] + 1 + rnd.integers(0, 3)) & 3
    return b


def word(h, k):
    return np.array([(h >> (2 * (k - 1 - i))) & 3 for i in range(k)], dtype=np.uint8)


def _fa_offset(lengths):
    """start offset of the next FASTA sequence behind sequences of these lengths (each padded to four bytes)"""
    return sum((l + 7) // 8 * 8 for l in lengths)


# ---- the walk: thread, span and grid edges ---------------------------------------------------------------------------------------------------------------------
def walk_fa():
    rnd = np.random.default_rng(101)
    seqs = []
    for l in (7, 8, 9, 10, 11, 12):                                          # k-1, k, k+1 for k = 8, 10, 11
        seqs.append(background(rnd, l))
    for l in range(17, 33):                                                  # a last base at every residue mod 16 from starts at 0 and at 8 mod 16
        seqs.append(background(rnd, l)); seqs.append(background(rnd, l + 8))
    other = [5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15]
    for j, code in enumerate((N, other[0], N, other[1])):                    # first base, last base
        s = background(rnd, 40 + j); s[0 if j < 2 else -1] = code; seqs.append(s)
    for j, code in enumerate((N, other[2])):                                 # span offsets 0 and 15, a run that crosses a span
        start = _fa_offset([len(s) for s in seqs])
        s = background(rnd, 150 + j)
        rel = (-start) % 16                                                  # start + rel is a span's offset 0
        s[rel + 32] = code; s[rel + 63] = code; s[rel + 94:rel + 99] = code
        seqs.append(s)
    for code in (N, other[3]):                                               # a run that crosses a workgroup boundary
        start = _fa_offset([len(s) for s in seqs])
        s = background(rnd, 4501)
        rel = (-start) % 4096
        s[rel - 3:rel + 4] = code
        seqs.append(s)
    seqs.append(np.full(23, N, dtype=np.uint8))                              # N only
    s = background(rnd, 61); s[5::6] = N; s[2] = other[4]; seqs.append(s)    # no clean window
    s = background(rnd, 45); s[7::7] = other[5]; seqs.append(s)
    seqs.append(background(rnd, 333))                                        # the last sequence is odd as well
    return GenomeSet("walk_fa", seqs, [(8, 1, DEFAULT_H), (11, 1, DEFAULT_H)])


def walk_tight():
    rnd = np.random.default_rng(102)
    seqs = [background(rnd, 18), background(rnd, 8), background(rnd, 9), background(rnd, 8), background(rnd, 8), background(rnd, 2), background(rnd, 8)]
    for i in range(400):
        l = int(rnd.integers(1, 41))
        s = background(rnd, l)
        if rnd.random() < 0.3:
            a = int(rnd.integers(0, l)); s[a:a + int(rnd.integers(1, 4))] = N if rnd.random() < 0.5 else int(rnd.integers(5, 16))
        seqs.append(s)
    return GenomeSet("walk_tight", seqs, [(8, 1, DEFAULT_H)], tight=True)


def grid_edge(delta):
    """the last base ends a multiple of 4 096 offsets (delta 0), one short of it (-1), one past it (+1)"""
    rnd = np.random.default_rng(103)
    a = background(rnd, 4000); b = background(rnd, 4192 + delta)
    a[100:103] = N; b[-20] = N
    return GenomeSet("grid_edge_%s" % {-1: "short", 0: "exact", 1: "past"}[delta], [a, b], [(8, 1, DEFAULT_H)])


# ---- the skip distance ---------------------------------------------------------------------------------------------------------------------------------------------
SKIP_OPTIONS = [(8, 2, DEFAULT_H), (10, 3, DEFAULT_H), (11, 7, DEFAULT_H), (8, 8, DEFAULT_H)]


def skip():
    rnd = np.random.default_rng(104)
    seqs = []
    for _ in range(2):                                                       # several sequences with their own first bad code inside one thread's span
        s = background(rnd, 12); s[11] = N; seqs.append(s)
        s = background(rnd, 12); s[0] = N; seqs.append(s)
    seqs.append(background(rnd, 97))                                         # no bad code
    for k in (8, 10, 11):
        s = background(rnd, 120); s[3] = N; seqs.append(s)                   # a first bad code inside the very first window
        s = background(rnd, 171); s[42 + k] = N; seqs.append(s)              # a window that ends one base before the first bad code, S = 2, 3, 7
        s = background(rnd, 90); s[2 * k] = N; seqs.append(s)                # the same, S = k
    s = background(rnd, 6001); s[5000:5003] = N; s[5400:5409] = 10; s[5800] = N; seqs.append(s)     # a first bad code more than 4 096 offsets in, three runs
    for i in range(500):
        l = int(rnd.integers(30, 121))
        s = background(rnd, l)
        for _r in range(int(rnd.integers(0, 4))):
            a = int(rnd.integers(0, l)); s[a:a + int(rnd.integers(1, 10))] = N if rnd.random() < 0.6 else int(rnd.integers(5, 16))
        seqs.append(s)
    return GenomeSet("skip", seqs, SKIP_OPTIONS, tight=True)


# ---- list lengths --------------------------------------------------------------------------------------------------------------------------------------------------
LIST_K = 10
LIST_LENGTHS = (0, 1, 2, 32, 33, 64, 65, 128, 129, 8191, 8192, 8193, 16384, 16385)
LIST_WAVE = 0x5A5C0 >> 6                                                     # the wave of k_ix_compact that owns the planted lists of 33, 65 and 129 entries


def _run(unit, windows, k):
    """windows k-mer starts of the repeat `unit`, flanked so that it makes no further ones"""
    n = windows + k - 1
    body = np.resize(np.array(unit, dtype=np.uint8), n)
    flank = Gg if Gg not in unit else T
    return np.concatenate(([flank], body, [flank])).astype(np.uint8)


def _split(n, parts):
    q = n // parts
    return [q] * (parts - 1) + [n - q * (parts - 1)]


def _planted(rnd, k, plan):
    """every (hash, count) of plan planted count times, shuffled, random gaps between"""
    occ = [h for h, n in plan for _ in range(n)]
    rnd.shuffle(occ)
    parts = []
    for h in occ:
        parts.append(word(int(h), k)); parts.append(background(rnd, int(rnd.integers(4, 20))))
    return np.concatenate(parts) if parts else np.zeros(0, dtype=np.uint8)


def lists():
    """hash 0: 16 385, hash 4^k - 1: 16 384, the other two homopolymers 8 193 and 8 192, (TC)n 8 191 -- each in three pieces in different workgroups of the walk; 1 .. 129 planted"""
    k = LIST_K; rnd = np.random.default_rng(105)
    big = [((T,), 16385), ((Gg,), 16384), ((Cc,), 8193), ((A,), 8192)]
    pieces = [[_run(u, w, k) for w in _split(n, 3)] for u, n in big]
    # (TC)n: a piece of 2a - 1 windows holds a starts of TCTC.. and a - 1 of CTCT..
    pieces.append([_run((T, Cc), 2 * a - 1, k) for a in _split(8191, 3)])
    seqs = []
    for r in range(3):
        parts = []
        for p in pieces:
            parts.append(p[r]); parts.append(background(rnd, 701 + 2 * r))
        seqs.append(np.concatenate(parts))
    base = LIST_WAVE << 6
    plan = [(base + 3, 33), (base + 4, 65), (base + 17, 129), (0x12345, 1), (0x2B3C1, 2), (0x31F07, 32), (0x0C0DE, 64), (0x3D00D, 128)]
    seqs.append(np.concatenate((background(rnd, 501), _planted(rnd, k, plan))))
    return GenomeSet("lists", seqs, [(k, 1, 8192), (k, 1, DEFAULT_H)])


# ---- sampling ------------------------------------------------------------------------------------------------------------------------------------------------------
SAMPLING_H = (1, 20, 32, 33, 64, 100)
SAMPLING_WAVE = 0x77740 >> 6


def sampling():
    """lists of H-1, H, H+1 entries for every H; 40 entries at hash 0 and 70 at hash 4^k - 1; the lists of 33, 34 and 65 entries in one wave of k_ix_compact"""
    k = LIST_K; rnd = np.random.default_rng(106)
    base = SAMPLING_WAVE << 6
    plan = [(base + 1, 33), (base + 2, 34), (base + 40, 65), (0x01234, 19), (0x0ABCD, 20), (0x1BEE5, 21), (0x2F00D, 31), (0x3A1B2, 32), (0x15A5A, 63), (0x29C71, 64),
            (0x0F1E2, 99), (0x3C3C3 ^ 0x101, 100), (0x24680, 101)]
    seqs = [np.concatenate((background(rnd, 3001), _run((T,), 20, k), background(rnd, 4500), _run((Gg,), 35, k), background(rnd, 2000))),
            np.concatenate((background(rnd, 777), _planted(rnd, k, plan))),
            np.concatenate((background(rnd, 5000), _run((T,), 20, k), background(rnd, 4097), _run((Gg,), 35, k), background(rnd, 1001)))]
    return GenomeSet("sampling", seqs, [(k, 1, h) for h in SAMPLING_H])


def many_over():
    """several thousand over-represented k-mers: the generator's k-mer order matters"""
    rnd = np.random.default_rng(107)
    return GenomeSet("many_over", [rnd.integers(0, 4, size=60001).astype(np.uint8)], [(8, 1, 2)])


def all_sets():
    return [walk_fa(), walk_tight(), grid_edge(-1), grid_edge(0), grid_edge(1), skip(), lists(), sampling(), many_over()]


SHORTER_THAN_K = ("walk_fa", "walk_tight")      # sets with a sequence shorter than wordLen: the reference's unsigned endingOffset wraps there; not compared with its binary


# ---- shared by tests/test_index_model.py and tests/test_gpu_index_edges.py: every set is built, compressed and modelled once ----------------------------------
_MODELS = {}
_SETS = {}


def the_sets():
    if not _SETS:
        for gs in all_sets():
            _SETS[gs.name] = gs
    return _SETS


def nib2_of(gs, directory):
    """the set's `.nib2` as the command line writes it (FASTA sets are compressed by the command line itself); returns its path"""
    p = gs.write(directory)
    if not gs.tight:
        import subprocess
        import yaha_amd as ya
        subprocess.run([ya.CLI_PATH, "-g", p, "-c"], stderr=subprocess.PIPE, check=True)
    return os.path.splitext(p)[0] + ".nib2"


def modelled(gs, opt, nib2_path):
    """(image bytes, Coverage, Index), computed once per set and option list and shared by every test that needs it"""
    key = (gs.name, opt)
    if key not in _MODELS:
        _MODELS[key] = index_model.model(open(nib2_path, "rb").read(), *opt)
    return _MODELS[key]


def index_name(root, opt):
    return "%s.X%02d_%02d_%05dS" % ((root,) + tuple(opt))
