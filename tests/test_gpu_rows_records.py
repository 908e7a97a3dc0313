"""GPU tier: the trace records of k_ext_rows_pk (ext_lanes_pk.h), bit by bit, through the only thing that reads them -- the traceback.

A record holds four decision bits (notT, notU, notContE, notContF) and a mismatch bit for each of the strip's 21 columns: pair k of the kernel's eleven
register pairs serves column k in its low half and column k + 11 in its high half, and its bits sit at fixed places of the record's four dwords.  A bit
that lands in the wrong place, byte or dword only shows when a traceback walks through that column, so the problems here are made to: X-drop
extensions in both directions whose query is shifted against the reference by d = -10 ... +10 bases -- the best path leaves the origin (column 10)
through a gap of |d| and runs down column 10 + d -- with a substitution, a short insertion and a short deletion behind the shift, so that every kind
of decision is read in that column and its neighbour.  Around them extensions of 1, 2, 7, 8, 9, 16, 17 and 60 rows (a record block holds 8 records, a
chunk 16 blocks of a lane): lanes finish early and take their next problem in the middle of a block.  Two calls: 40 problems (one wave's pool, filled
once) and all of them (more than the 256 the call's four waves take at their first fill: the rest goes to lanes that refill).

Score, lengths and edit list of every problem equal the oracle's (ygpu_dp_batch, lane kernels and their careful instantiation), as in
test_gpu_parity.py::test_dp_batch_bit_exact.  Before anything is compared the ORACLE's results are checked for the coverage the test is about."""
import os
import random

import numpy as np
import pytest

import oracle
import yaha_amd as ya
from problems import batch_arrays

pytestmark = pytest.mark.gpu

LETTERS = "TCAG"                      # the index's base codes 0..3 (codes of 4 and above: N and the like, avoided)
CENTRE = 10                           # the strip's column of the origin: cell (row i, column j) is query base i - 1 against reference base i - 1 + j - CENTRE
# inside the packed kernel's limits (MS * longest read <= 15 000, RC + X + GO + 21 GE <= 4 000); gaps cheap enough that a gap of ten at the origin
# (13) stays inside the X-drop and beats any run of substitutions, dear enough that a substitution (4) is no insertion + deletion (8)
SCORING = ["-MS", "3", "-RC", "4", "-GOC", "3", "-GEC", "1", "-X", "40"]
ROW_COUNTS = (1, 2, 7, 8, 9, 16, 17, 60)
VARIANTS = 6


def _other(rng, base):
    return rng.choice([c for c in LETTERS if c != base])


def shifted_extension(rng, ref, d, variant):
    """The query of an extension over `ref` (both in the order the extension consumes them) whose best path starts with a gap of |d| -- d > 0: d reference
    bases skipped, d < 0: -d query bases of its own -- and then carries a substitution and two short gaps, ordered so that the path stays inside columns 0..20."""
    seg = [rng.randint(9, 14) + variant for _ in range(4)]
    r, q = max(d, 0), [_other(rng, ref[k]) for k in range(max(-d, 0))]

    def copy(n):
        nonlocal r
        q.extend(ref[r:r + n]); r += n

    def insertion(n):
        q.extend(_other(rng, ref[r]) for _ in range(n))

    def deletion(n):
        nonlocal r
        r += n
    copy(seg[0])
    q.append(_other(rng, ref[r])); r += 1
    copy(seg[1])
    n = 1 + variant % 2                                                      # (both of one length: the path comes back to its column)
    (deletion if d <= 0 else insertion)(n)
    copy(seg[2])
    (insertion if d <= 0 else deletion)(n)
    copy(seg[3])
    return "".join(q)


def build_problems(nib, max_roff):
    """reads (one per problem: the query in read order, padded) and [(DPProblem fields, kind)]; the reference pieces are taken 400 bases apart."""
    rng = random.Random(20)
    reads, probs = [], []
    place = [3000]

    def ref_piece(rev, n):
        while True:
            at = place[0]; place[0] += 400
            assert at + 200 < max_roff
            piece = nib[at:at + 200]
            if (piece < 4).all():
                break
        codes = piece[::-1] if rev else piece                                # consumption order: a reverse extension walks down from its first base
        return (at + 199 if rev else at), "".join(LETTERS[c] for c in codes[:n])

    def add(rev, r_off, query, kind):
        pad = "".join(rng.choice(LETTERS) for _ in range(max(0, 45 - len(query)) + 5))
        read = (query[::-1] + pad) if rev else (query + pad)                 # a reverse extension starts at the query's last base of the piece and walks down
        q_off = len(query) - 1 if rev else 0
        probs.append(((len(reads), 0, ya.DP_EXT_REV if rev else ya.DP_EXT_FWD, q_off, len(query), 0, r_off), kind))
        reads.append(read)
    for variant in range(VARIANTS):
        for rev in (False, True):
            for d in range(-CENTRE, CENTRE + 1):
                r_off, ref = ref_piece(rev, 160)
                add(rev, r_off, shifted_extension(rng, ref, d, variant), ("column", CENTRE + d))
        for rev in (False, True):
            for n in ROW_COUNTS:
                r_off, ref = ref_piece(rev, n)
                q = list(ref)
                if variant % 2 and n >= 7:
                    q[n // 2] = _other(rng, q[n // 2])
                add(rev, r_off, "".join(q), ("rows", n))
    # shuffled: short and long problems next to each other, so that lanes free up (and refill) while others still run
    order = list(range(len(probs)))
    random.Random(21).shuffle(order)
    return [reads[k] for k in order], [((new,) + probs[k][0][1:], probs[k][1]) for new, k in enumerate(order)]


def check_coverage(probs, exp):
    """What the oracle's own results have to show, or the comparison below proves nothing about the records' columns."""
    kinds = {c: set() for c in range(2 * CENTRE + 1)}
    rows_seen = set()
    for (fields, kind), (score, aq, ar, ops) in zip(probs, exp):
        assert score > 0, ("a problem without a positive score walks no record", fields, kind)
        maxj = CENTRE + ar - aq                                              # the column of the maximum: aq rows down, ar - aq columns off the origin's
        assert 0 <= maxj <= 2 * CENTRE
        if kind[0] == "column":
            assert maxj == kind[1], ("the oracle's path does not end in the column it was built for", fields, kind, (score, aq, ar, ops))
            kinds[maxj].update(c for _n, c in ops)
        else:
            assert aq == kind[1] and maxj == CENTRE, (fields, kind, (score, aq, ar))
            rows_seen.add(aq)
        assert fields[2] in (ya.DP_EXT_FWD, ya.DP_EXT_REV)
    for c, seen in kinds.items():
        assert seen >= set("MRID"), "column %d: edit lists hold only %r" % (c, sorted(seen))
    assert rows_seen == set(ROW_COUNTS)
    for rev in (ya.DP_EXT_FWD, ya.DP_EXT_REV):
        assert {k[1] for (f, k) in probs if k[0] == "column" and f[2] == rev} == set(range(2 * CENTRE + 1))


def _compare(ctx, probs, exp, kernels):
    res, ops, _nops = ctx.dp_batch([ya.DPProblem(*f) for f, _k in probs], kernels)
    bad = []
    for k, e in enumerate(exp):
        r = res[k]
        got = (r.score, r.addedQLen, r.addedRLen, tuple((ops[r.op_start + j] & 0xFFFF, chr((ops[r.op_start + j] >> 16) & 0xFF)) for j in range(r.n_ops)))
        if got != e:
            bad.append((probs[k], got, e))
    for b in bad[:4]:
        print("MISMATCH kernels %d: %r\n got %r\n exp %r" % ((kernels,) + b))
    assert not bad, "%d of %d extensions differ from the oracle (kernel family %d)" % (len(bad), len(probs), kernels)


@pytest.fixture(scope="module")
def cases(work, index11, tmp_path_factory):
    """(session arguments, problems, the oracle's results): made once for the module."""
    with ya.Session(["-x", index11, "-q", os.path.join(work, "r1k.fa")]) as s0:
        bases, _offs, _codes = batch_arrays(s0, s0.next_batch(1))
        nib = np.empty(2 * len(bases), np.uint8); nib[0::2] = bases >> 4; nib[1::2] = bases & 15
        reads, probs = build_problems(nib, int(s0.index.maxROff))
    path = str(tmp_path_factory.mktemp("rows") / "reads.fa")
    with open(path, "w") as f:
        for k, r in enumerate(reads):
            f.write(">q%d\n%s\n" % (k, r))
    args = ["-x", index11, "-q", path] + SCORING
    with ya.Session(args) as s:
        b = s.next_batch(len(reads) + 1)
        assert b.n_reads == len(reads)
        exp = oracle.dp_batch(s.index, s.params, b, [ya.DPProblem(*f) for f, _k in probs])
    return args, probs, exp


def test_the_oracle_walks_every_column_with_every_kind_of_step(cases):
    _args, probs, exp = cases
    assert len(probs) > 256 + 64
    check_coverage(probs, exp)


@pytest.mark.parametrize("kernels", [ya.DP_KERNELS_LANES, ya.DP_KERNELS_LANES_CAREFUL])
def test_rows_records_bit_exact_in_every_column(cases, kernels):
    args, probs, exp = cases
    check_coverage(probs, exp)
    with ya.Session(args) as s:
        b = s.next_batch(len(probs) + 1)
        assert s.params.bandWidth == 5 and s.params.maxGap >= 21 and s.params.maxIntron >= 21      # (the packed kernel's conditions)
        with ya.Context(s.index, s.params) as ctx:
            ctx.upload(b)
            _compare(ctx, probs[:40], exp[:40], kernels)                     # one wave's pool, filled once
            _compare(ctx, probs, exp, kernels)                               # four waves' first fills, and refills
            _compare(ctx, probs[40:90], exp[40:90], kernels)                 # and a small call again on the same context
