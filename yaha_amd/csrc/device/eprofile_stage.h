// eprofile_stage.h -- the error profile (-oep) counted on the device, right behind the post-filter: the substitution spectrum, the indel lengths, the identity of
// every record and the error rate along the read, of the clumps that will be printed -- 1556 counters for a whole run.  What one record adds is
// ../eprofile_core.h, the very source the host compiles for the records the device does not see (host/eprofile.cpp).
//
// The other stages scatter sparse atomics over an array as large as the genome; this one funnels every aligned base of a batch into a table of 12 KB, where
// plain global atomics would queue up on a handful of addresses.  So k_eprofile_clumps is a PERSISTENT grid: a fixed number of workgroups, each with the table
// as uint32 words in LDS (6.2 KB, the four gate counters behind it), whose waves stride over the batch's clumps; a workgroup adds its non-zero words to the
// context's uint64 table with global atomics once, when it has run out of clumps.
// A clump gets a WAVE, which opens like the other tracks (track_stage.h: the ops 64 at a time with the scan of their reference lengths) and deals the chunk's
// aligned bases across the lanes in strips of 64 as k_pileup_clumps does (the two further scans, the binary search in the inclusive sums).  A lane then holds a
// PAIR: the reference's channel from the packed image, the read's from the snapshot's forward codes.  Nearly all pairs of a strip are matches in a few
// neighbouring POS bins, and same-address LDS atomics take their turns one by one -- so the strip is combined in the wave first: a ballot per diagonal SUB cell and
// one add of its population count; query offsets rise with the lane, so equal POS bins lie side by side, the first lane of each run adds the run's length (and
// its errors') from the ballots of the run heads.  Only what is rare -- substitutions, N, the D and I ops (a lane each) -- goes to LDS a lane at a time.
// matches and columns are summed over the wave at the record's end for its IDENT word.
//
// No LDS word can wrap within one launch.  A word of SUB or of POS channels 0 / 1 takes at most 1 per pair, and a record has at most qEnd <= 65 536 pairs (eqo
// has 16 bits, and q, which every pair advances, stays below qEnd); the host sizes the grid so that a workgroup's waves together take at most 65 535 records
// (eprofileGrid below): 65 535 x 65 536 < 2^32.  A word of INS, DEL or of POS channels 2 / 3 takes at most 1 per op, and a batch has fewer than 2^31 ops
// (ygpu_inject_results and the align stage both refuse more); IDENT and the gate counters take at most 1 per record.
#pragma once
#include "track_stage.h"
#include "../eprofile_core.h"

#define YE_GRID 256u                              // workgroups of a launch: one per CU of an MI355X (fewer for a batch with fewer clumps than their waves)
#define YE_WAVES 4u                               // waves a workgroup
#define YE_LDS_WORDS ((uint32_t)yeprofile::WORDS + 4u)      // the table, then records counted / skipped (MAPQ) / dropped (two sequences) / reads left to the host
struct EProfileArgs {
    ydepth::Layout L;                          // (binBase unused: the profile has no slots)
    unsigned long long *table;                 // the context's table: yeprofile::WORDS words, then the four statistics words
    const uint8_t *bases; uint64_t nBaseBytes; // the image's packed reference
    const uint8_t *fwd; const uint32_t *readOff;      // the snapshot's forward codes and the reads' offsets into them (n + 1 words)
};
// workgroups for nClumps clumps: YE_GRID, fewer when that leaves waves without a clump, more when a workgroup would pass 65 535 records (see above)
static inline uint32_t eprofileGrid(uint32_t nClumps)
{
    const uint32_t forWork = (nClumps + YE_WAVES - 1u) / YE_WAVES, forWrap = nClumps / (65535u - YE_WAVES) + 1u;
    const uint32_t g = forWork < YE_GRID ? forWork : YE_GRID;
    return g > forWrap ? g : forWrap;
}

__device__ __forceinline__ unsigned long long waveTotalSumU64(unsigned long long v)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += (unsigned long long)__shfl_xor((long long)v, d, 64);
    return v;
}

// one clump on one wave (every lane of the wave calls it with the same w)
__device__ __forceinline__ void eprofileClump(const EProfileArgs &P, uint32_t *tab, const ygpu_out_clump *fClumps, const uint32_t *fOps, const uint32_t *outStart,
                                              uint32_t nReads, uint32_t w, uint32_t lane)
{
    const ygpu_out_clump f = fClumps[w];
    // the read of clump w: the last r with outStart[r] <= w (reads without output repeat their neighbour's word)
    uint32_t lo = 0, hi = nReads - 1;
    while (lo < hi) { const uint32_t mid = (lo + hi + 1) >> 1; if (outStart[mid] <= w) lo = mid; else hi = mid - 1; }
    if (f.primaryCount == 0xFFFFu) {                                        // a read handed back unfiltered: the host filters it and counts what it prints
        if (lane == 0 && outStart[lo] == w) atomicAdd(tab + yeprofile::WORDS + 3, 1u);
        return;
    }
    int seq = -1; const int g = ydepth::gate(P.L, f.c, f.mapQuality, &seq);
    if (lane == 0) atomicAdd(tab + yeprofile::WORDS + g, 1u);
    if (g != ydepth::COUNTED) return;
    const uint32_t r0 = P.readOff[lo], qlen = P.readOff[lo + 1] - r0; const uint8_t *const fwd = P.fwd + r0;
    const bool reversed = (f.status & 1u) != 0;
    const uint32_t *ops = fOps + f.c.op_start; const uint32_t nOps = f.c.n_ops;
    const uint32_t qe = ypileup::qEnd(f.c, qlen);
    uint32_t cur = f.c.sro, q = f.c.sqo < qe ? f.c.sqo : qe, matches = 0;   // (cur and q: the same on every lane)
    unsigned long long cols = 0;
    for (uint32_t k0 = 0; k0 < nOps; k0 += 64) {
        const OpChunk c = loadOpChunk(ops, nOps, k0, lane);
        const uint32_t qn = c.k < nOps ? ypileup::opQuery(c.op) : 0u, qIncl = waveInclSumU(qn), qTotal = (uint32_t)__shfl((int)qIncl, 63, 64);
        const uint32_t bn = c.covered ? c.n : 0u, bIncl = waveInclSumU(bn), bTotal = (uint32_t)__shfl((int)bIncl, 63, 64);
        // D and I: the lane's own op
        uint32_t section, posCh;
        if (c.k < nOps && !c.covered && yeprofile::gapOp(f.c, c.op, cur + c.excl, &section, &posCh)) {
            const uint32_t qx = qIncl - qn, qOp = qx < qe - q ? q + qx : qe, len = YGPU_OP_LEN(c.op);
            atomicAdd(tab + yeprofile::lenWord(section, len), 1u);
            if (qOp < qe) { cols += len; atomicAdd(tab + yeprofile::posWord(yeprofile::posBin(qOp < qe - 1u ? qOp : qe - 1u, qlen, reversed), posCh), 1u); }
        }
        // M and R: the chunk's aligned bases in strips of 64, a pair a lane (every lane takes part in the shuffles and ballots; a lane past the last base adds nothing)
        for (uint32_t b0 = 0; b0 < bTotal; b0 += 64) {
            const uint32_t b = b0 + lane;
            uint32_t jl = 0, jh = 63;                                        // the first lane whose inclusive sum is above b
            for (int step = 0; step < 6; step++) {
                const uint32_t mid = (jl + jh) >> 1, v = (uint32_t)__shfl((int)bIncl, (int)mid, 64);
                if (v > b) jh = mid; else jl = mid + 1;
            }
            const uint32_t j = jl < 63u ? jl : 63u;
            const uint32_t i = b - (uint32_t)__shfl((int)(bIncl - bn), (int)j, 64);
            const uint32_t ro = cur + (uint32_t)__shfl((int)c.excl, (int)j, 64) + i, qo = q + (uint32_t)__shfl((int)(qIncl - qn), (int)j, 64) + i;
            const bool valid = b < bTotal && qo < qe;
            uint32_t rc = (uint32_t)ypileup::N, bc = (uint32_t)ypileup::N, bin = 0xFFFFFFFFu;
            if (valid) { rc = yeprofile::refCh(P.bases, P.nBaseBytes, ro); bc = ypileup::chOfRead(fwd, qlen, qo, reversed); bin = yeprofile::posBin(qo, qlen, reversed); }
            const bool match = valid && yeprofile::isMatch(rc, bc);
            // SUB: the four diagonal cells by ballot, everything else a lane at a time
#pragma unroll
            for (uint32_t ch = 0; ch < 4; ch++) {
                const unsigned long long mk = __ballot(match && rc == ch);
                if (lane == 0 && mk) atomicAdd(tab + yeprofile::subWord(ch, ch), (uint32_t)__popcll(mk));
            }
            if (valid && !match) atomicAdd(tab + yeprofile::subWord(rc, bc), 1u);
            // POS: runs of equal bins (query offsets rise with the lane, so a bin's pairs lie side by side): the first lane of a run adds its length and its errors
            const unsigned long long vm = __ballot(valid), em = __ballot(valid && !match);
            const uint32_t prev = (uint32_t)laneUp1((int)bin, -1);
            const unsigned long long heads = __ballot(valid && (lane == 0 || prev != bin));
            if (valid && (lane == 0 || prev != bin)) {
                const unsigned long long above = lane < 63u ? heads & ~((2ull << lane) - 1ull) : 0ull;
                const uint32_t end = above ? (uint32_t)__builtin_ctzll(above) : 64u;
                const unsigned long long run = (end < 64u ? (1ull << end) - 1ull : ~0ull) & ~((1ull << lane) - 1ull) & vm;
                atomicAdd(tab + yeprofile::posWord(bin, yeprofile::POS_PAIRS), (uint32_t)__popcll(run));
                if (run & em) atomicAdd(tab + yeprofile::posWord(bin, yeprofile::POS_ERRORS), (uint32_t)__popcll(run & em));
            }
            matches += match ? 1u : 0u; cols += valid ? 1u : 0u;
        }
        cur += c.total; q = qTotal < qe - q ? q + qTotal : qe;               // (past the end nothing is added any more: q stays there, as in the one-thread walk)
    }
    const uint32_t m = waveTotalSumU(matches); const unsigned long long n = waveTotalSumU64(cols);
    if (lane == 0 && n) atomicAdd(tab + yeprofile::identWord(m, n), 1u);
}

__global__ void __launch_bounds__(256) k_eprofile_clumps(EProfileArgs P, const ygpu_out_clump *fClumps, const uint32_t *fOps, const uint32_t *outStart, uint32_t nReads,
                                                         uint32_t nClumps)
{
    __shared__ uint32_t tab[YE_LDS_WORDS];
    for (uint32_t i = threadIdx.x; i < YE_LDS_WORDS; i += blockDim.x) tab[i] = 0u;
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63u, stride = gridDim.x * YE_WAVES;
    if (nReads) for (uint32_t w = blockIdx.x * YE_WAVES + (threadIdx.x >> 6); w < nClumps; w += stride) eprofileClump(P, tab, fClumps, fOps, outStart, nReads, w, lane);
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < YE_LDS_WORDS; i += blockDim.x) { const uint32_t v = tab[i]; if (v) atomicAdd(P.table + i, (unsigned long long)v); }
}
