// depth_core.h -- read depth along the reference (-ocov): what one printed record adds to the binned coverage array, as ONE routine compiled for the host
// (host/depth.cpp: the records the device did not count) and for the device (device/depth_stage.h: a wave per clump behind the post-filter), so that the two
// sides cannot drift apart.  No allocation, no library calls.
//
// The contract (every layer and every test shares it): each reference sequence is cut into bins of `bin` bases; bins never straddle two sequences, the last
// bin of a sequence may be shorter; bins are numbered sequence by sequence in index order (binBase[s] = first bin of sequence s, binBase[nSeqs] = n_bins).
// cov[b] (uint32) = number of (record, reference base) pairs with the base in bin b over all printed records: a record covers the reference bases under its
// M and R ops (the M of the printed CIGAR); bases under D are not covered, I and clips consume no reference; a clump printClump drops (it spans two
// sequences, host/sam.cpp) covers nothing; records with mapQuality < minMapq cover nothing.  Overflow of a bin's uint32 is not handled.
#pragma once
#include <stdint.h>
#include "../../include/yaha_hip.h"

#if defined(__HIPCC__)
#define YDP_FN __host__ __device__ inline
#else
#define YDP_FN inline
#endif

namespace ydepth {

struct Layout {
    const uint32_t *seqStart, *seqLength;      // reference sequences in bases, ascending (Genome::seqs)
    const uint32_t *binBase;                   // nSeqs + 1 entries
    uint32_t nSeqs, bin, minMapq;
};
enum { COUNTED = 0, SKIPPED_MAPQ = 1, DROPPED = 2 };      // what became of a record (the first three words of the statistics)

// n_bins and binBase[] of a sequence table; false when the bins do not fit 32 bits or bin < 1.  binBase may be null (size only).
inline bool layoutBins(const uint32_t *seqLength, uint32_t nSeqs, uint32_t bin, uint32_t *binBase, uint64_t *nBins)
{
    if (bin < 1) return false;
    uint64_t n = 0;
    for (uint32_t s = 0; s < nSeqs; s++) { if (binBase) binBase[s] = (uint32_t)n; n += ((uint64_t)seqLength[s] + bin - 1) / bin; if (n > 0xFFFFFFFFull) return false; }
    if (binBase) binBase[nSeqs] = (uint32_t)n;
    *nBins = n; return true;
}

// the gate of a record: COUNTED and its sequence, or why it covers nothing.  The two-sequence drop is printClump's own test (sam.cpp:24-26) and comes first:
// such a clump is never printed, whatever its mapping quality.
YDP_FN int gate(const Layout &L, const ygpu_clump &c, uint32_t mapQuality, int *seq)
{
    const uint32_t s0 = c.sro, s1 = c.sro + c.refLen - 1; int si = -1;
    for (uint32_t i = 0; i < L.nSeqs; i++) if (s0 >= L.seqStart[i] && s0 < L.seqStart[i] + L.seqLength[i]) { si = (int)i; break; }
    if (si < 0 || s1 >= L.seqStart[si] + L.seqLength[si]) return DROPPED;
    *seq = si;
    return mapQuality < L.minMapq ? SKIPPED_MAPQ : COUNTED;
}
// reference bases an op consumes; *covered: they count (M, R) or not (D)
YDP_FN uint32_t opRef(uint32_t op, bool *covered)
{
    const char code = YGPU_OP_CODE(op);
    *covered = code == 'M' || code == 'R';
    return (*covered || code == 'D') ? YGPU_OP_LEN(op) : 0u;
}
// One covered run [off, off + len) of sequence seq (off: absolute reference offset) -> add(bin, bases of the run in that bin), one call per (run, bin).  The run's
// bins are dealt to `nLanes` callers: caller `lane` takes every nLanes-th of them, so that neighbouring lanes hit neighbouring words (bin == 1: neighbouring bases).
// A run never leaves its sequence (gate), so the last, short bin needs no clamp of its own.
template <class Add> YDP_FN void addRun(const Layout &L, int seq, uint32_t off, uint32_t len, uint32_t lane, uint32_t nLanes, Add add)
{
    if (!len) return;
    const uint32_t rel32 = off - L.seqStart[seq];                       // (offsets fit 32 bits: the divisions stay 32-bit ones on the device)
    const uint64_t rel = rel32, end = rel + len, B = L.bin;
    const uint64_t b0 = rel32 / L.bin, b1 = (uint32_t)(end - 1) / L.bin;
    for (uint64_t b = b0 + lane; b <= b1; b += nLanes) {
        const uint64_t lo = b * B > rel ? b * B : rel, hi = (b + 1) * B < end ? (b + 1) * B : end;
        add(L.binBase[seq] + (uint32_t)b, (uint32_t)(hi - lo));
    }
}
// The whole walk of one record on one thread: gate, then its ops -> covered runs (neighbouring M and R ops are one run; a D ends it) -> adds.
// Returns COUNTED / SKIPPED_MAPQ / DROPPED; *bases: reference bases the record covered.
template <class Add> YDP_FN int walkClump(const Layout &L, const ygpu_clump &c, const uint32_t *ops, uint32_t mapQuality, Add add, uint64_t *bases)
{
    int seq = -1; const int g = gate(L, c, mapQuality, &seq);
    if (g != COUNTED) return g;
    uint32_t cur = c.sro, runStart = c.sro; uint64_t tot = 0;
    for (uint32_t k = 0; k < c.n_ops; k++) {
        bool covered; const uint32_t n = opRef(ops[k], &covered);
        if (!covered && n) { addRun(L, seq, runStart, cur - runStart, 0u, 1u, add); runStart = cur + n; } else tot += n;
        cur += n;
    }
    addRun(L, seq, runStart, cur - runStart, 0u, 1u, add);
    if (bases) *bases = tot;
    return COUNTED;
}
}  // namespace ydepth
