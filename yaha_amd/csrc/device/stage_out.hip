// stage_out.hip -- what leaves the device: the batch's results as ygpu_run left them (ygpu_collect*), and the post-filter stage (postFilterBySimilarity,
// GraphPath.cpp:897-1086, Query.c:450) on a snapshot of them -- oqc_stage.h -- with its own stream, wait slot and look-back words (PfSide); behind it, when
// ygpu_depth_enable asked for it, the read-depth track of the printed clumps (depth_stage.h), and when ygpu_events_enable did, their evidence track
// (events_stage.h), and when ygpu_pileup_enable did, their allele pileup (pileup_stage.h: the one track that reads the reads' bases, which the snapshot then copies
// as well), and when ygpu_indels_enable did, their indel alleles in the context's own hash table (indel_stage.h); and when ygpu_junctions_enable did, the
// batch's split-read junctions (junction_stage.h), which leave with the filtered batch; and when ygpu_eprofile_enable did, their error profile in the context's
// own table of counters (eprofile_stage.h).  At the end of a run the pileup array also gives the SNV calls (snv_stage.h: folds into it, the selection over it) and,
// with the run's raw indel alleles, the indel calls (indelcall_stage.h: the left shift, the merge, the selection at the anchors).
#include "ctx.h"
#include "oqc_stage.h"
#include "depth_stage.h"
#include "events_stage.h"
#include "pileup_stage.h"
#include "snv_stage.h"
#include "indel_stage.h"
#include "indelcall_stage.h"
#include "eprofile_stage.h"
#include "junction_stage.h"
#include <algorithm>
#include <map>
#include <tuple>

extern "C" {
int ygpu_collect(ygpu_ctx *ctx, ygpu_result_batch *out)                      // into the context's own vectors
{
    if (!ctx || !out || ctx->stageDone < 3) return YGPU_EINVAL;
    ctx->hClumpStart.assign(ctx->nReads + 1, 0); ctx->hClumps.resize(ctx->nOut); ctx->hOps.resize(ctx->nOutOps);
    return ygpu_collect_into(ctx, ctx->hClumpStart.data(), ctx->hClumps.data(), ctx->hOps.data(), out);
}

int ygpu_result_size(ygpu_ctx *ctx, uint64_t *n_clumps, uint64_t *n_ops)
{
    if (!ctx || ctx->stageDone < 3) return YGPU_EINVAL;
    if (n_clumps) *n_clumps = ctx->nOut; if (n_ops) *n_ops = ctx->nOutOps;
    return 0;
}
int ygpu_collect_into(ygpu_ctx *ctx, uint32_t *clump_start, ygpu_clump *clumps, uint32_t *ops, ygpu_result_batch *out)
{
    if (!ctx || !out || !clump_start || ctx->stageDone < 3 || (ctx->nOut && !clumps) || (ctx->nOutOps && !ops)) return YGPU_EINVAL;
    HIPCHK(hipSetDevice(ctx->device));
    const uint32_t n = ctx->nReads;
    HIPCHK(hipMemcpyAsync(clump_start, ctx->readStart.p, 4ull * (n + 1), hipMemcpyDeviceToHost, ctx->stream));
    if (ctx->nOut) HIPCHK(hipMemcpyAsync(clumps, ctx->outClumps2.p, sizeof(ygpu_clump) * (uint64_t)ctx->nOut, hipMemcpyDeviceToHost, ctx->stream));
    if (ctx->nOutOps) HIPCHK(hipMemcpyAsync(ops, ctx->outOps.p, 4ull * ctx->nOutOps, hipMemcpyDeviceToHost, ctx->stream));
    DevCounters dc; HIPCHK(hipMemcpyAsync(&dc, ctx->ctr.p, sizeof dc, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(streamSync(ctx));
    { const unsigned long long dropped = dc.v[C_FRAGS];                      // dead single-hit fragments (each one a region of its own) that were counted, not written
      dc.v[C_HITS] = ctx->nHits; dc.v[C_FRAGS] = ctx->nFrags + dropped; dc.v[C_REGIONS] = ctx->nRegions + dropped; }
    memcpy(&ctx->hCounters, dc.v, sizeof(ygpu_counters));
    out->n_reads = n; out->clump_start = clump_start; out->clumps = clumps; out->ops = ops;
    out->n_clumps = ctx->nOut; out->n_ops = ctx->nOutOps; out->counters = ctx->hCounters;
    return 0;
}

// ---- post-filter on the device (oqc_stage.h; reference GraphPath.cpp:897-1086) ----------------------------------------------------------------------
int ygpu_set_postfilter(ygpu_ctx *ctx, const ygpu_postfilter_params *p)
{
    if (!ctx || !ctx->stream || !p) return YGPU_EINVAL;
    if (p->bppN < 0 || p->bppN > 65536 || (p->bppN && !p->bppThr) || (p->n_seqs && (!p->seq_start || !p->seq_length))) {
        ctx->err = "ygpu_set_postfilter: bad break point table or sequence table"; return YGPU_EINVAL; }
    // (the wave's successor relaxation writes node j > i only while it reads node i: with a non-overlap requirement below one base a node could be its own successor, oqc_stage.h)
    if (p->minNonOverlap < 1) { ctx->err = "ygpu_set_postfilter: minNonOverlap (-MNO) must be at least 1 for the device stage; use the host filter"; return YGPU_EINVAL; }
    HIPCHK(hipSetDevice(ctx->device));
    ENSURE(ctx->oqThr, 4ull * (p->bppN + 1)); ENSURE(ctx->oqSeqStart, 4ull * (p->n_seqs + 1)); ENSURE(ctx->oqSeqLen, 4ull * (p->n_seqs + 1));
    if (p->bppN) HIPCHK(hipMemcpyAsync(ctx->oqThr.p, p->bppThr, 4ull * p->bppN, hipMemcpyHostToDevice, ctx->stream));
    if (p->n_seqs) { HIPCHK(hipMemcpyAsync(ctx->oqSeqStart.p, p->seq_start, 4ull * p->n_seqs, hipMemcpyHostToDevice, ctx->stream));
        HIPCHK(hipMemcpyAsync(ctx->oqSeqLen.p, p->seq_length, 4ull * p->n_seqs, hipMemcpyHostToDevice, ctx->stream)); }
    HIPCHK(streamSync(ctx));
    yoqc::Params &P = ctx->oqP;
    P.GOCost = ctx->P.GO; P.GECost = ctx->P.GE; P.RCost = ctx->P.RC; P.MScore = ctx->P.MS;
    P.minNonOverlap = p->minNonOverlap; P.BPCost = p->BPCost; P.maxBPLog = p->maxBPLog; P.FBS = p->FBS; P.FBS_PSLength = p->FBS_PSLength; P.FBS_PSScore = p->FBS_PSScore;
    P.bppVmin = p->bppVmin; P.bppN = p->bppN; P.bppThr = ctx->oqThr.as<uint32_t>();
    ctx->oqG.start = ctx->oqSeqStart.as<uint32_t>(); ctx->oqG.length = ctx->oqSeqLen.as<uint32_t>(); ctx->oqG.n = p->n_seqs;
    ctx->oqSet = true; return 0;
}
/* The stage works on a SNAPSHOT of the batch's results -- clump lists, edit ops, the reads' lengths and generator seeds, the work counters: 150 MB copied inside
 * the device in ~0.1 ms -- so that the context can take its next batch (ygpu_upload, ygpu_run) while another thread filters this one: ygpu_postfilter_snapshot on
 * the context's thread after ygpu_run, then ygpu_postfilter / ygpu_filtered_size / ygpu_collect_filtered on any thread.  (A ygpu_postfilter without a snapshot
 * takes one itself: the sequential use.)  One snapshot at a time: the next may be taken once the filtered results of this one have been collected. */
int ygpu_postfilter_snapshot(ygpu_ctx *ctx)
{
    if (!ctx || !ctx->stream || ctx->stageDone < 3) return YGPU_EINVAL;
    if (!ctx->oqSet) { ctx->err = "ygpu_postfilter_snapshot: ygpu_set_postfilter has not been called on this context"; return YGPU_EINVAL; }
    if (ctx->pfSnap.load()) { ctx->err = "ygpu_postfilter_snapshot: the previous snapshot has not been filtered yet"; return YGPU_EINVAL; }
    HIPCHK(hipSetDevice(ctx->device));
    const uint32_t n = ctx->nReads, C = ctx->nOut, O = ctx->nOutOps;
    ENSURE(ctx->oqCs, 4ull * (n + 2)); ENSURE(ctx->oqCl, sizeof(ygpu_clump) * ((uint64_t)C + 1)); ENSURE(ctx->oqOpsIn, 4ull * ((uint64_t)O + 1));
        ENSURE(ctx->oqSeeds, 20ull * (n + 1)); ENSURE(ctx->oqQlen, 4ull * (n + 1));
    HIPCHK(hipMemcpyAsync(ctx->oqCs.p, ctx->readStart.p, 4ull * (n + 1), hipMemcpyDeviceToDevice, ctx->stream));
    if (C) HIPCHK(hipMemcpyAsync(ctx->oqCl.p, ctx->outClumps2.p, sizeof(ygpu_clump) * (uint64_t)C, hipMemcpyDeviceToDevice, ctx->stream));
    if (O) HIPCHK(hipMemcpyAsync(ctx->oqOpsIn.p, ctx->outOps.p, 4ull * O, hipMemcpyDeviceToDevice, ctx->stream));
    if (n) KL(k_oqc_seeds, dim3(gridFor(n, 256)), dim3(256), 0, ctx->stream, ctx->dFwd.as<uint8_t>(), ctx->dReadOff.as<uint32_t>(), n, ctx->oqSeeds.as<uint32_t>(),
        ctx->oqQlen.as<uint32_t>());
    // the allele pileup reads the reads' bases behind the filter, when the next upload may have overwritten them: the forward codes (the reverse strand's channel
    // follows from them, pileup_core.h) and the reads' offsets join the snapshot -- only on a context that enabled the pileup, the indel alleles, which read
    // the inserted bases there, or the error profile, which reads every aligned base
    ctx->snapBases = ctx->totalBases;
    if ((ctx->track[TRACK_PILEUP] || ctx->idSet || ctx->epSet) && n) {
        ENSURE(ctx->puFwd, ctx->totalBases + 1); ENSURE(ctx->puReadOff, 4ull * (n + 1));
        if (ctx->totalBases) HIPCHK(hipMemcpyAsync(ctx->puFwd.p, ctx->dFwd.p, ctx->totalBases, hipMemcpyDeviceToDevice, ctx->stream));
        HIPCHK(hipMemcpyAsync(ctx->puReadOff.p, ctx->dReadOff.p, 4ull * (n + 1), hipMemcpyDeviceToDevice, ctx->stream));
    }
    // (no wait here: the context's thread goes straight on to its next batch -- whatever it queues on this stream follows the copies -- and the work counters land
    // in a pinned slot the filter's side reads after its own first wait; without the slot, a wait it is)
    if (ctx->snapCtr) HIPCHK(hipMemcpyAsync(ctx->snapCtr, ctx->ctr.p, sizeof(DevCounters), hipMemcpyDeviceToHost, ctx->stream));
    else { DevCounters dc; HIPCHK(hipMemcpyAsync(&dc, ctx->ctr.p, sizeof dc, hipMemcpyDeviceToHost, ctx->stream)); HIPCHK(streamSync(ctx));
        memcpy(&ctx->snapCtrPlain, &dc, sizeof dc); }
    HIPCHK(hipEventRecord(ctx->evSnap, ctx->stream));
    { static const bool waitHere = getenv("YGPU_SNAPSHOT_WAIT") != nullptr; if (waitHere) HIPCHK(streamSync(ctx)); }
    ctx->snapHits = ctx->nHits; ctx->snapFrags = ctx->nFrags; ctx->snapRegions = ctx->nRegions;
    ctx->snapN = n; ctx->snapC = C; ctx->snapOps = O; ctx->oqDone = false;
    ctx->pfSnap.store(true);
    return 0;
}
// A look-back of an exclusive sum on the post-filter's side gave up (CNT_SCANFAIL).  Not sticky: the flag and the look-back words -- stale tickets and statuses --
// are made clean again for the next batch, as runTo does on its side; the call fails with `what`'s message.
static int scanGaveUp(PfSide *ctx, const char *what)
{
    HIPCHK(hipMemsetAsync(ctx->counters.as<uint32_t>() + CNT_SCANFAIL, 0, 4, ctx->stream));
    if (ctx->scanState.p) HIPCHK(hipMemsetAsync(ctx->scanState.p, 0, ctx->scanState.cap, ctx->stream));
    HIPCHK(streamSync(ctx));
    ctx->err = std::string(what) + ": a look-back of an exclusive sum gave up"; return YGPU_EINTERNAL;
}
// ---- the filter side of an entry point ---------------------------------------------------------------------------------------------------------------------------
// ygpu_last_error answers with the filter side's message (full->pf.err) while tlsPfFailed names the context on this thread, and with full->err otherwise.  The
// rule, stated here and nowhere else: pfEnter names the context before the first step that may fail on the filter's side -- HIPCHK, ENSURE, KL and the helpers
// below write that side's message and return with the name standing; pfLeave takes it back on success; pfArgError takes it back for an argument error, whose
// message is the context's own.
static PfSide *pfEnter(ygpu_ctx *full) { tlsPfFailed = full; return &full->pf; }
static int pfLeave() { tlsPfFailed = nullptr; return 0; }
static int pfArgError(ygpu_ctx *full, const std::string &what) { tlsPfFailed = nullptr; full->err = what; return YGPU_EINVAL; }
// the last word of a run of exclusive sums -- the total -- with the flag of a look-back that gave up and the caller's own words, in ONE wait
static int fetchTotal(PfSide *ctx, const uint32_t *last, const char *noun, uint32_t *tot, FetchPiece extra = {nullptr, nullptr, 0})
{
    uint32_t scanFail = 0;
    const FetchPiece pc[3] = {{last, tot, 1}, {ctx->counters.as<uint32_t>() + CNT_SCANFAIL, &scanFail, 1}, extra};
    const int rc = fetchMany(ctx, pc, extra.n ? 3 : 2); if (rc) return rc;
    return scanFail ? scanGaveUp(ctx, noun) : 0;
}
static ydepth::Layout trackLayout(const TrackImage &T)
{
    return ydepth::Layout{T.seqStart.as<uint32_t>(), T.seqLength.as<uint32_t>(), T.binBase.as<uint32_t>(), (uint32_t)T.hSeqStart.size(), T.bin, T.minMapq};
}
static ydepth::Layout indelLayout(const ygpu_ctx *full)
{
    return ydepth::Layout{full->idSeqStart.as<uint32_t>(), full->idSeqLen.as<uint32_t>(), full->idBinBase.as<uint32_t>(), full->idNSeqs, 1u, full->idMinMapq};
}
// the indel table made (or made again, larger) and zeroed with its statistics, on the post-filter side's stream
static int indelTable(ygpu_ctx *full, uint64_t capacity)
{
    PfSide *ctx = &full->pf;
    if (full->idTable.ensureExact(sizeof(ygpu_indel_entry) * capacity)) {
        (void)hipGetLastError(); size_t fb = 0, tb = 0; if (hipMemGetInfo(&fb, &tb) != hipSuccess) { fb = 0; (void)hipGetLastError(); }
        char m[256]; snprintf(m, sizeof m, "ygpu_indels_enable: no room on device %d for the indel table (-oid): %.2f GB for %llu entries, %.2f GB free", full->device,
            sizeof(ygpu_indel_entry) * capacity / 1e9, (unsigned long long)capacity, fb / 1e9);
        ctx->err = m; full->err = m; full->idCap = 0; return YGPU_ENOMEM;
    }
    full->idCap = capacity; full->idUsed = 0;
    HIPCHK(hipMemsetAsync(full->idTable.p, 0, sizeof(ygpu_indel_entry) * capacity, ctx->stream));
    HIPCHK(hipMemsetAsync(full->idStats.p, 0, 128, ctx->stream));
    return 0;
}
// The binned tracks of the nClumps clumps just gathered -- the ones that get printed -- on the post-filter's stream, a wave a clump: the evidence track (the wave
// finds its clump's read -- the query length of the right clip -- in oqOutStart; YGPU_EVENTS_DIRECT: every op's atomics without the combining in the wave, for
// measurements; read at every call), then read depth and its count of the reads handed back, then the allele pileup (the wave finds its clump's read the same
// way, and the read's bases in the snapshot's copy of the forward codes).
static int launchTracks(ygpu_ctx *full, uint32_t n, uint32_t nClumps)
{
    PfSide *ctx = &full->pf;
    if (!nClumps) return 0;
    const ygpu_out_clump *fClumps = full->oqFClumps.as<ygpu_out_clump>(); const uint32_t *fOps = full->oqFOps.as<uint32_t>();
    const dim3 grid(gridFor((uint64_t)nClumps * 64, 256)), block(256);
    if (const TrackImage *T = full->track[TRACK_EVENTS].get()) {
        EventsArgs E; E.L = trackLayout(*T); E.minClip = T->minClip; E.ev = T->data.as<uint32_t>(); E.nBins = (uint32_t)T->nBins; E.stats = T->stats.as<unsigned long long>();
        if (T->bin > 1 && getenv("YGPU_EVENTS_DIRECT") == nullptr)
            KL(k_event_clumps<true>, grid, block, 0, ctx->stream, E, fClumps, fOps, full->oqOutStart.as<uint32_t>(), full->oqQlen.as<uint32_t>(), n, nClumps);
        else
            KL(k_event_clumps<false>, grid, block, 0, ctx->stream, E, fClumps, fOps, full->oqOutStart.as<uint32_t>(), full->oqQlen.as<uint32_t>(), n, nClumps);
    }
    if (const TrackImage *T = full->track[TRACK_DEPTH].get()) {
        DepthArgs D; D.L = trackLayout(*T); D.cov = T->data.as<uint32_t>(); D.nBins = (uint32_t)T->nBins; D.stats = T->stats.as<unsigned long long>();
        KL(k_depth_clumps, grid, block, 0, ctx->stream, D, fClumps, fOps, nClumps);
        KL(k_depth_handed_back, dim3(gridFor(n, 256)), block, 0, ctx->stream, full->oqOutCnt.as<uint32_t>(), full->oqPrimCnt.as<uint32_t>(), n, D.stats);
    }
    if (const TrackImage *T = full->track[TRACK_PILEUP].get()) {
        PileupArgs P; P.L = trackLayout(*T); P.pu = T->data.as<uint32_t>(); P.nSlots = (uint32_t)T->nBins; P.stats = T->stats.as<unsigned long long>();
        P.fwd = full->puFwd.as<uint8_t>(); P.readOff = full->puReadOff.as<uint32_t>();
        KL(k_pileup_clumps, grid, block, 0, ctx->stream, P, fClumps, fOps, full->oqOutStart.as<uint32_t>(), n, nClumps);
    }
    // the indel alleles, behind the pileup's kernel: into the context's own table
    if (full->idSet && full->idTable.p) {
        IndelArgs A; A.L = indelLayout(full); A.minLen = full->idMinLen; A.table = full->idTable.as<ygpu_indel_entry>(); A.mask = (uint32_t)(full->idCap - 1);
        A.probeLimit = (uint32_t)std::min<uint64_t>(full->idCap, YI_PROBE_LIMIT);
        A.stats = full->idStats.as<unsigned long long>(); A.used = full->idStats.as<uint32_t>() + 16; A.lost = A.used + 1;
        A.fwd = full->puFwd.as<uint8_t>(); A.readOff = full->puReadOff.as<uint32_t>();
        KL(k_indel_clumps, grid, block, 0, ctx->stream, A, fClumps, fOps, full->oqOutStart.as<uint32_t>(), n, nClumps);
    }
    // the error profile, last: a persistent grid, the table in LDS, into the context's own table (eprofile_stage.h)
    if (full->epSet && full->epTable.p) {
        EProfileArgs E; E.L = ydepth::Layout{full->epSeqs.as<uint32_t>(), full->epSeqs.as<uint32_t>() + full->epNSeqs, nullptr, full->epNSeqs, 1u, full->epMinMapq};
        E.table = full->epTable.as<unsigned long long>(); E.bases = full->dBases.as<uint8_t>(); E.nBaseBytes = full->dBases.cap;
        E.fwd = full->puFwd.as<uint8_t>(); E.readOff = full->puReadOff.as<uint32_t>();
        KL(k_eprofile_clumps, dim3(eprofileGrid(nClumps)), dim3(64u * YE_WAVES), 0, ctx->stream, E, fClumps, fOps, full->oqOutStart.as<uint32_t>(), n, nClumps);
    }
    return 0;
}
static int postfilterBody(ygpu_ctx *full);
int ygpu_postfilter(ygpu_ctx *full)
{
    if (!full || !full->stream) return YGPU_EINVAL;
    if (!full->pfSnap.load()) { const int rc = ygpu_postfilter_snapshot(full); if (rc) { pfLeave(); return rc; } }      // (the snapshot's message is the context's own)
    int rc = postfilterBody(full);
    if (rc == 0 && ydCheckStateOn()) {                                       // (debug switch: the post-filter side's own look-back words)
        const DevBuf *const bufs[1] = {&full->pf.scanState}; static const char *const names[1] = {"the post-filter side's look-back state"};
        if (full->oqClsCnt.ensure(64)) { full->pf.err = "hipMalloc failed"; rc = YGPU_ENOMEM; }
        else rc = ydCheckZero(full->pf.stream, full->pf.err, (unsigned int *)full->oqClsCnt.p + 8, bufs, names, 1, "after ygpu_postfilter");
        if (rc) full->oqDone = false;
    }
    full->pfSnap.store(false);
    if (rc) { pfEnter(full); return rc; }
    return pfLeave();
}
static int postfilterBody(ygpu_ctx *full)
{
    PfSide *ctx = &full->pf;                                                 // (every macro and helper below: the post-filter's side)
    HIPCHK(hipSetDevice(full->device));
    HIPCHK(hipStreamWaitEvent(ctx->stream, full->evSnap, 0));
    const uint32_t n = full->snapN, C = full->snapC; full->pfN = n; full->nFOut = full->nFOps = 0; full->oqDone = false;
    full->jnDone = full->jnHaveTotal = false; full->jnReads = 0; full->jnTotal = 0;
    auto takeCounters = [&]() {                                              // (after a wait of this side's stream: the snapshot's copies are done)
        DevCounters dc = full->snapCtr ? *full->snapCtr : full->snapCtrPlain;
        const unsigned long long dropped = dc.v[C_FRAGS]; dc.v[C_HITS] = full->snapHits; dc.v[C_FRAGS] = full->snapFrags + dropped; dc.v[C_REGIONS] = full->snapRegions + dropped;
        memcpy(&full->pfCounters, dc.v, sizeof(ygpu_counters));
    };
    ENSURE(full->oqOutStart, 4ull * (n + 2)); ENSURE(full->oqOpsStart, 4ull * (n + 2));
    if (n == 0 || C == 0) { HIPCHK(hipMemsetAsync(full->oqOutStart.p, 0, 4ull * (n + 2), ctx->stream)); HIPCHK(streamSync(ctx)); takeCounters(); full->oqDone = true;
        full->jnDone = full->jnSet; return 0; }
    ENSURE(full->oqNeed, 8ull * (n + 2)); ENSURE(full->oqPoolOff, 8ull * (n + 2)); ENSURE(full->oqLists, 4ull * YQ_NCLASS * (uint64_t)n + 64); ENSURE(full->oqClsCnt, 64);
    ENSURE(full->oqPrim, sizeof(yoqc::CNode) * (uint64_t)C); ENSURE(full->oqPA, sizeof(yoqc::PAttr) * (uint64_t)C); ENSURE(full->oqPush, sizeof(yoqc::OutRec) * (uint64_t)C);
        ENSURE(full->oqOut, sizeof(yoqc::OutRec) * (uint64_t)C);
    ENSURE(full->oqOutCnt, 4ull * (n + 2)); ENSURE(full->oqOutOps, 4ull * (n + 2)); ENSURE(full->oqPrimCnt, 4ull * (n + 2));
    HIPCHK(hipMemsetAsync((uint32_t *)full->oqOutCnt.p + n, 0, 8, ctx->stream)); HIPCHK(hipMemsetAsync((uint32_t *)full->oqOutOps.p + n, 0, 8, ctx->stream));
        HIPCHK(hipMemsetAsync(full->oqClsCnt.p, 0, 64, ctx->stream));
    OqcArgs A; A.P = full->oqP; A.G = full->oqG; A.cs = full->oqCs.as<uint32_t>(); A.cl = full->oqCl.as<ygpu_clump>(); A.ops = full->oqOpsIn.as<uint32_t>();
        A.seeds = full->oqSeeds.as<uint32_t>(); A.qlen = full->oqQlen.as<uint32_t>(); A.nReads = n;
    A.poolOff = full->oqPoolOff.as<unsigned long long>(); A.prim = full->oqPrim.as<yoqc::CNode>(); A.pa = full->oqPA.as<yoqc::PAttr>(); A.push = full->oqPush.as<yoqc::OutRec>();
        A.out = full->oqOut.as<yoqc::OutRec>();
    A.outCnt = full->oqOutCnt.as<uint32_t>(); A.outOpsCnt = full->oqOutOps.as<uint32_t>(); A.primCnt = full->oqPrimCnt.as<uint32_t>();
    A.keys = nullptr; A.stack = nullptr; A.nodes = nullptr; A.pfxOff = nullptr; A.path = nullptr; A.pool = nullptr; A.prof = nullptr;
    // (read at every call: tests lower it to send small reads down the hand-over path)
    { const char *e = getenv("YGPU_OQC_MAX"); const int v = e ? atoi(e) : YQ_DEVICE_MAX; A.devMax = v >= 1 && v < YQ_DEVICE_MAX ? v : YQ_DEVICE_MAX; }
    { const char *e = getenv("YGPU_OQC_HBM"); A.graphInHbm = e && atoi(e) ? 1 : 0; }      // (read at every call, as YGPU_OQC_MAX)
    static const bool oqProf = getenv("YGPU_OQC_PROF") != nullptr;
    if (oqProf) { ENSURE(full->oqProf, 8ull * 32 * YQ_NCLASS); HIPCHK(hipMemsetAsync(full->oqProf.p, 0, 8ull * 32 * YQ_NCLASS, ctx->stream));
        A.prof = full->oqProf.as<unsigned long long>(); }
    uint32_t *lists = full->oqLists.as<uint32_t>();
    KL(k_oqc_classify, dim3(gridFor(n + 1, 256)), dim3(256), 0, ctx->stream, A, full->oqNeed.as<unsigned long long>(), lists, full->oqClsCnt.as<unsigned int>());
    int rc = cubScan64(ctx, full->oqNeed.as<unsigned long long>(), full->oqPoolOff.as<unsigned long long>(), n + 1); if (rc) return rc;
    unsigned long long poolInts = 0; uint32_t nCls[YQ_NCLASS] = {0, 0, 0, 0, 0};
    { uint32_t w[2] = {0, 0}; const FetchPiece pc[2] = {{full->oqPoolOff.as<unsigned long long>() + n, w, 2}, {full->oqClsCnt.p, nCls, YQ_NCLASS}};
      rc = fetchMany(ctx, pc, 2); if (rc) return rc; poolInts = (unsigned long long)w[0] | ((unsigned long long)w[1] << 32); }
    takeCounters();
    ENSURE(full->oqPool, 4ull * (poolInts + 16)); A.pool = full->oqPool.as<int>();
    // work space of the reads in HBM: what a wave's LDS does not hold (the survivors' keys while the nodes are made; everything for the reads of the last class)
    ENSURE(full->oqKeys, sizeof(yoqc::SortKey) * (uint64_t)C); ENSURE(full->oqStack, 4ull * (4ull * C + 8ull * n + 16)); ENSURE(full->oqNodes, sizeof(yoqc::CNode) * (uint64_t)C);
        ENSURE(full->oqPfx, 4ull * C); ENSURE(full->oqPath, 4ull * C);
    A.keys = full->oqKeys.as<yoqc::SortKey>(); A.stack = full->oqStack.as<int>(); A.nodes = full->oqNodes.as<yoqc::CNode>(); A.pfxOff = full->oqPfx.as<int>();
        A.path = full->oqPath.as<int>();
    // the classes: clumps a read may have -> LDS of its workgroup; ints of LDS pool (the first tables; later ones go to the read's slice of the HBM pool)
    static const int capN[YQ_NCLASS] = {112, 224, 448, YQ_DEVICE_MAX, 0};
    // A wave a read, every read of a class resident at once: a launch lasts as long as its slowest read (one of 400 clumps with 280 survivors: 3 ms), and the classes
    // follow one another on the post-filter's one stream.  That latency is off the context's path -- the next batch is running meanwhile -- and a stream of its own for
    // every class is not worth having: streams share four hardware queues, and more than two a context put all contexts' main streams on one (profiles/r05_hw_queues.txt).
    // left to the host, marked
    if (nCls[YQ_NCLASS - 1]) KL(k_oqc_raw, dim3(gridFor(nCls[YQ_NCLASS - 1], 64)), dim3(64), 0, ctx->stream, A, lists + (size_t)(YQ_NCLASS - 1) * n, nCls[YQ_NCLASS - 1]);
    for (int c = YQ_NCLASS - 2; c >= 0; c--) if (nCls[c]) {
        const unsigned lds = std::min(YQ_LDS_MAX, oqcLdsBytes(capN[c]));
        KL(k_oqc_wave, dim3(nCls[c]), dim3(64), lds, ctx->stream, A, lists + (size_t)c * n, nCls[c], lds);
    }
    if (kTrace) fprintf(stderr,
        "[ygpu] post-filter: %u reads with two or more clumps in classes of <= 112 / 224 / 448 / %d clumps: %u / %u / %u / %u, left to the host %u; pool %.1f MB\n",
        nCls[0] + nCls[1] + nCls[2] + nCls[3] + nCls[4], YQ_DEVICE_MAX, nCls[0], nCls[1], nCls[2], nCls[3], nCls[4], poolInts * 4.0 / 1e6);
    rc = cubScan(ctx, full->oqOutCnt.as<uint32_t>(), full->oqOutStart.as<uint32_t>(), n + 1); if (rc) return rc;
    rc = cubScan(ctx, full->oqOutOps.as<uint32_t>(), full->oqOpsStart.as<uint32_t>(), n + 1); if (rc) return rc;
    uint32_t tot[2] = {0, 0}, scanFail = 0;
    { const FetchPiece pc[3] = {{full->oqOutStart.as<uint32_t>() + n, &tot[0], 1}, {full->oqOpsStart.as<uint32_t>() + n, &tot[1], 1}, {ctx->counters.as<uint32_t>() + CNT_SCANFAIL,
        &scanFail, 1}}; rc = fetchMany(ctx, pc, 3); if (rc) return rc; }
    if (scanFail) return scanGaveUp(ctx, "post-filter");
    full->nFOut = tot[0]; full->nFOps = tot[1];
    ENSURE(full->oqFClumps, sizeof(ygpu_out_clump) * ((uint64_t)tot[0] + 1)); ENSURE(full->oqFOps, 4ull * ((uint64_t)tot[1] + 1));
    KL(k_oqc_gather, dim3(gridFor((uint64_t)n * 64, 256)), dim3(256), 0, ctx->stream, A, full->oqOutStart.as<uint32_t>(), full->oqOpsStart.as<uint32_t>(),
        full->oqFClumps.as<ygpu_out_clump>(), full->oqFOps.as<uint32_t>());
    // split-read junctions (-obp): the gathered clumps are in print order, so a wave a read counts its eligible records, the exclusive sum places the reads'
    // junctions, and a second pass ranks the records and writes them -- ordered by (read, ordinal); nothing is waited for here: ygpu_junctions_size fetches the total
    if (full->jnSet) {
        ENSURE(full->jnCnt, 4ull * (n + 2)); ENSURE(full->jnStart, 4ull * (n + 2)); ENSURE(full->jnOut, sizeof(ygpu_junction) * ((uint64_t)tot[0] + 1)); ENSURE(full->jnStats, 64);
        HIPCHK(hipMemsetAsync(full->jnCnt.p, 0, 4ull * (n + 2), ctx->stream)); HIPCHK(hipMemsetAsync(full->jnStats.p, 0, 64, ctx->stream));
        JunctionArgs J; J.L = yjunc::layout(full->jnSeqStart.as<uint32_t>(), full->jnSeqLen.as<uint32_t>(), full->jnNSeqs, full->jnMinMapq);
        J.fClumps = full->oqFClumps.as<ygpu_out_clump>(); J.outStart = full->oqOutStart.as<uint32_t>(); J.qlens = full->oqQlen.as<uint32_t>(); J.nReads = n;
        J.cnt = full->jnCnt.as<uint32_t>(); J.start = full->jnStart.as<uint32_t>(); J.out = full->jnOut.as<ygpu_junction>(); J.cap = tot[0] + 1;
        J.stats = full->jnStats.as<unsigned long long>();
        const dim3 grid(gridFor((uint64_t)n * 64, 256));
        KL(k_junction_count, grid, dim3(256), 0, ctx->stream, J);
        rc = cubScan(ctx, full->jnCnt.as<uint32_t>(), full->jnStart.as<uint32_t>(), n + 1); if (rc) return rc;
        KL(k_junction_emit, grid, dim3(256), 0, ctx->stream, J);
        full->jnReads = n; full->jnDone = true;
    }
    // the indel table by the rule: a batch larger than any before it gets a larger table while the table is empty (a table with entries stays as it is)
    if (full->idSet && full->idAuto && full->idUsed == 0 && full->idTable.p && yindel::tableCapacity(full->snapBases) > full->idCap) {
        rc = indelTable(full, yindel::tableCapacity(full->snapBases)); if (rc) return rc; }
    // the binned tracks that are enabled (-oev, -ocov, -opu), the indel alleles (-oid) and the error profile (-oep), behind the junctions on this stage's stream
    rc = launchTracks(full, n, tot[0]); if (rc) return rc;
    // the indel table's used and lost words: one more small wait, behind the kernel.  An event that found no entry is an error of this call, not a fault.
    if (full->idSet && full->idTable.p && tot[0]) {
        uint32_t ul[2] = {0, 0}; rc = fetchU32(ctx, full->idStats.as<uint32_t>() + 16, ul, 2); if (rc) return rc;
        full->idUsed = ul[0];
        if (ul[1]) { char m[256]; snprintf(m, sizeof m, "ygpu_postfilter: %u indel events found no entry in the table of %llu entries, %u of them in use (-oid): "
            "call ygpu_indels_collect more often or enable a larger capacity", ul[1], (unsigned long long)full->idCap, ul[0]); ctx->err = m; return YGPU_EOVERFLOW; }
    }
    if (oqProf) {
        unsigned long long h[32 * YQ_NCLASS]; HIPCHK(hipMemcpyAsync(h, full->oqProf.p, sizeof h, hipMemcpyDeviceToHost, ctx->stream)); HIPCHK(streamSync(ctx));
        static const char *nm[7] = {"keys", "sort", "dup scan", "nodes+tables", "path walk", "successors", "finish"};
        for (int c = 0; c < YQ_NCLASS; c++) if (h[32 * c + 7]) {
            const unsigned long long *q = h + 32 * c;
                fprintf(stderr, "[ygpu] post-filter class %d: %llu reads, %.0f clumps, %.0f survivors a read; us a read (largest of any read):", c, q[7], (double)q[8] / q[7],
                (double)q[9] / q[7]);
            for (int k = 0; k < 7; k++) fprintf(stderr, " %s %.1f (%.0f)", nm[k], q[k] / 100.0 / q[7], q[16 + k] / 100.0);
            fprintf(stderr, "; slowest read %.0f us: %llu clumps, %llu survivors\n", (q[10] >> 24) / 100.0, (q[10] >> 12) & 4095ull, q[10] & 4095ull);
        }
    }
    full->oqDone = true;
    return 0;
}
// ---- the binned tracks: read depth, the evidence track and the allele pileup (depth_stage.h, events_stage.h, pileup_stage.h; the contracts are in
// ../depth_core.h, ../events_core.h and ../pileup_core.h) -----------------------------------------------------------------------------------------------------
// What tells the kinds apart outside their kernels: the entry points' names and the array's noun for messages, the option that makes the array smaller (none:
// the bin is fixed), the words a bin takes, whether a clip length belongs to the parameters, and the statistics words the stage keeps.
struct TrackKind { int kind; const char *enable, *size, *collect, *noun, *counted, *binOpt; uint32_t channels; bool hasClip; uint32_t nStats; };
static const TrackKind kDepthKind = {TRACK_DEPTH, "ygpu_depth_enable", "ygpu_depth_size", "ygpu_depth_collect", "coverage", "depth is", "-covbin", 1, false, 4};
static const TrackKind kEventsKind = {TRACK_EVENTS, "ygpu_events_enable", "ygpu_events_size", "ygpu_events_collect", "evidence", "the events are", "-evbin",
    (uint32_t)yevents::NCH, true, 4};
static const TrackKind kPileupKind = {TRACK_PILEUP, "ygpu_pileup_enable", "ygpu_pileup_size", "ygpu_pileup_collect", "pileup", "the pileup is", nullptr,
    (uint32_t)ypileup::NCH, false, 5};
// the arrays of this process, by kind and by the image they belong to (the address of its bases on the device: what the contexts of an image share)
static std::mutex gTrackMu;
static std::map<std::tuple<int, int, const void *>, std::weak_ptr<TrackImage>> gTrackImages;

static int trackEnable(ygpu_ctx *ctx, const TrackKind &K, uint32_t bin, uint32_t minMapq, uint32_t minClip, uint32_t nSeqs, const uint32_t *seqStart, const uint32_t *seqLength)
{
    if (!ctx || !ctx->stream) return YGPU_EINVAL;
    const std::string who = std::string(K.enable) + ": ";
    if (!ctx->oqSet) { ctx->err = who + "ygpu_set_postfilter has not been called on this context (" + K.counted + " counted behind the post-filter)"; return YGPU_EINVAL; }
    if (bin < 1 || (K.hasClip && minClip < 1) || !nSeqs || !seqStart || !seqLength) {
        ctx->err = who + (K.hasClip ? "bad bin size, clip length or sequence table" : "bad bin size or sequence table"); return YGPU_EINVAL; }
    HIPCHK(hipSetDevice(ctx->device));
    std::lock_guard<std::mutex> lk(gTrackMu);
    const std::tuple<int, int, const void *> key(K.kind, ctx->device, ctx->dBases.p);
    if (std::shared_ptr<TrackImage> have = gTrackImages[key].lock()) {      // a sibling enabled it: the same array, if the same track is asked for
        if (have->bin != bin || have->minMapq != minMapq || have->minClip != minClip || have->hSeqStart.size() != nSeqs
            || memcmp(have->hSeqStart.data(), seqStart, 4ull * nSeqs) != 0 || memcmp(have->hSeqLength.data(), seqLength, 4ull * nSeqs) != 0) {
            ctx->err = who + "the image's " + K.noun + " array was enabled with other parameters"; return YGPU_EINVAL; }
        ctx->track[K.kind] = have; return 0;
    }
    std::shared_ptr<TrackImage> T(new TrackImage); T->device = ctx->device; T->channels = K.channels; T->bin = bin; T->minMapq = minMapq; T->minClip = minClip;
    T->hSeqStart.assign(seqStart, seqStart + nSeqs); T->hSeqLength.assign(seqLength, seqLength + nSeqs);
    std::vector<uint32_t> binBase(nSeqs + 1);
    if (!ydepth::layoutBins(seqLength, nSeqs, bin, binBase.data(), &T->nBins) || T->nBins == 0) { ctx->err = who + "the bins do not fit 32 bits"; return YGPU_EINVAL; }
    const uint64_t bytes = 4ull * K.channels * T->nBins;
    if (T->data.ensureExact(bytes)) {                                       // (exact: a growth margin on 12 GB is 3 GB)
        (void)hipGetLastError(); size_t fb = 0, tb = 0; if (hipMemGetInfo(&fb, &tb) != hipSuccess) { fb = 0; (void)hipGetLastError(); }
        char perBin[32] = ""; if (K.channels > 1) snprintf(perBin, sizeof perBin, " (%u bytes a bin)", 4u * K.channels);
        const std::string wayOut = K.binOpt ? std::string("a larger ") + K.binOpt + " needs less" : std::string("the bin is fixed: a smaller -ctx leaves more");
        char m[320]; snprintf(m, sizeof m, "%sno room on device %d for the %s array: %.2f GB for %llu bins of %u bases%s, %.2f GB free (%s)", who.c_str(),
            ctx->device, K.noun, bytes / 1e9, (unsigned long long)T->nBins, bin, perBin, fb / 1e9, wayOut.c_str());
        ctx->err = m; return YGPU_ENOMEM;
    }
    if (T->stats.ensure(64) || T->seqStart.ensure(4ull * nSeqs) || T->seqLength.ensure(4ull * nSeqs) || T->binBase.ensure(4ull * (nSeqs + 1))) {
        (void)hipGetLastError(); ctx->err = who + "hipMalloc failed"; return YGPU_ENOMEM; }
    HIPCHK(hipMemsetAsync(T->data.p, 0, bytes, ctx->stream)); HIPCHK(hipMemsetAsync(T->stats.p, 0, 64, ctx->stream));
    HIPCHK(hipMemcpyAsync(T->seqStart.p, seqStart, 4ull * nSeqs, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(hipMemcpyAsync(T->seqLength.p, seqLength, 4ull * nSeqs, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(hipMemcpyAsync(T->binBase.p, binBase.data(), 4ull * (nSeqs + 1), hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(streamSync(ctx));
    gTrackImages[key] = T; ctx->track[K.kind] = T;
    return 0;
}
static int trackSize(ygpu_ctx *ctx, const TrackKind &K, uint64_t *n_bins)
{
    if (!ctx || !n_bins) return YGPU_EINVAL;
    if (!ctx->track[K.kind]) { ctx->err = std::string(K.size) + ": " + K.enable + " has not been called on this context"; return YGPU_EINVAL; }
    *n_bins = ctx->track[K.kind]->nBins; return 0;
}
// The image's array as it stands: every filter stage queued on the device so far -- this context's and its siblings' -- has finished when the copy is taken.
static int trackCollect(ygpu_ctx *ctx, const TrackKind &K, uint32_t *words, uint64_t *stats /* K.nStats words */)
{
    if (!ctx || !ctx->stream) return YGPU_EINVAL;
    if (!ctx->track[K.kind]) { ctx->err = std::string(K.collect) + ": " + K.enable + " has not been called on this context"; return YGPU_EINVAL; }
    HIPCHK(hipSetDevice(ctx->device));
    HIPCHK(hipDeviceSynchronize());
    const TrackImage &T = *ctx->track[K.kind];
    if (words) HIPCHK(hipMemcpy(words, T.data.p, 4ull * T.channels * T.nBins, hipMemcpyDeviceToHost));
    if (stats) { unsigned long long h[8]; HIPCHK(hipMemcpy(h, T.stats.p, sizeof h, hipMemcpyDeviceToHost)); for (uint32_t k = 0; k < K.nStats; k++) stats[k] = h[k]; }
    return 0;
}
int ygpu_depth_enable(ygpu_ctx *ctx, const ygpu_depth_params *p)
{
    return p ? trackEnable(ctx, kDepthKind, p->bin, p->min_mapq, 0, p->n_seqs, p->seq_start, p->seq_length) : YGPU_EINVAL;
}
int ygpu_depth_size(ygpu_ctx *ctx, uint64_t *n_bins) { return trackSize(ctx, kDepthKind, n_bins); }
int ygpu_depth_collect(ygpu_ctx *ctx, uint32_t *bins, uint64_t stats[4]) { return trackCollect(ctx, kDepthKind, bins, stats); }
int ygpu_events_enable(ygpu_ctx *ctx, const ygpu_events_params *p)
{
    return p ? trackEnable(ctx, kEventsKind, p->bin, p->min_mapq, p->min_clip, p->n_seqs, p->seq_start, p->seq_length) : YGPU_EINVAL;
}
int ygpu_events_size(ygpu_ctx *ctx, uint64_t *n_bins) { return trackSize(ctx, kEventsKind, n_bins); }
int ygpu_events_collect(ygpu_ctx *ctx, uint32_t *counts, uint64_t stats[4]) { return trackCollect(ctx, kEventsKind, counts, stats); }
int ygpu_pileup_enable(ygpu_ctx *ctx, const ygpu_pileup_params *p)
{
    return p ? trackEnable(ctx, kPileupKind, 1, p->min_mapq, 0, p->n_seqs, p->seq_start, p->seq_length) : YGPU_EINVAL;
}
int ygpu_pileup_size(ygpu_ctx *ctx, uint64_t *n_slots) { return trackSize(ctx, kPileupKind, n_slots); }
int ygpu_pileup_collect(ygpu_ctx *ctx, uint32_t *counts, uint64_t stats[5]) { return trackCollect(ctx, kPileupKind, counts, stats); }
// The candidates of the image's array as it stands -- the slots with nonref >= 1, ascending -- selected on the device (pileup_stage.h): count a tile, exclusive
// sums of the tiles' counts, emit; on the post-filter's side of the context (its stream and look-back words), once everything queued on the device has finished.
// A PARKED context may be asked as well (the command line's feeder of an image has always run a batch, but a caller may hold any sibling): ygpu_park released
// that side's counter words with the arenas, so they are made again here -- the look-back words come back by themselves (prims.hip).
static int pileupSide(ygpu_ctx *full)
{
    PfSide *ctx = &full->pf;
    if (ctx->counters.p) return 0;
    ENSURE(ctx->counters, 4 * CNT_N);
    HIPCHK(hipMemsetAsync(ctx->counters.p, 0, 4 * CNT_N, ctx->stream));
    return 0;
}
// The count half of a tile selection (select.h) on the filter's side: the tiles' two buffers sized, the two words behind the counts zeroed, the count pass, the
// exclusive sums, and ONE wait for the total (with the caller's own words, if it has any).  The buffers are the pileup's (the candidates, the SNV calls) or the
// indel stage's (both drains, the indel calls).  The emit half is the caller's: sel.out sized from *tot, t->cap set, one launch of k_select_emit<S>.
enum TileBufs { TILES_PILEUP, TILES_INDEL };
static dim3 selectGrid(const TileSel &t) { return dim3(gridFor((uint64_t)t.nTiles * 64, 256)); }
extern "C++" template <class S> static int selectCount(ygpu_ctx *full, TileBufs which, const S &sel, uint64_t nItems, const char *noun, TileSel *t, uint32_t *tot,
                                          FetchPiece extra = {nullptr, nullptr, 0})
{
    PfSide *ctx = &full->pf;
    const uint32_t nTiles = (uint32_t)((nItems + 64u * S::ROWS - 1) / (64u * S::ROWS));
    if (which == TILES_PILEUP) { ENSURE(full->puTileCnt, 4ull * (nTiles + 2)); ENSURE(full->puTileStart, 4ull * (nTiles + 2)); }
    else { ENSURE(full->idTileCnt, 4ull * (nTiles + 2)); ENSURE(full->idTileStart, 4ull * (nTiles + 2)); }
    uint32_t *const cnt = (which == TILES_PILEUP ? full->puTileCnt : full->idTileCnt).as<uint32_t>();
    uint32_t *const start = (which == TILES_PILEUP ? full->puTileStart : full->idTileStart).as<uint32_t>();
    HIPCHK(hipMemsetAsync(cnt + nTiles, 0, 8, ctx->stream));
    *t = TileSel{nTiles, cnt, start, 0};
    KL(k_select_count<S>, selectGrid(*t), dim3(256), 0, ctx->stream, sel, *t);
    const int rc = cubScan(ctx, cnt, start, nTiles + 1); if (rc) return rc;
    return fetchTotal(ctx, start + nTiles, noun, tot, extra);
}
// A selection's records to the caller, on the filter side's stream (no wait for the rest of the device: the selection waited)
static int collectRecords(ygpu_ctx *full, bool have, const char *notYet, uint64_t n, void *out, const DevBuf &src, size_t recBytes)
{
    if (!have) return pfArgError(full, notYet);
    if (!n) return 0;
    if (!out || !src.p) return YGPU_EINVAL;
    PfSide *ctx = pfEnter(full);
    HIPCHK(hipSetDevice(full->device));
    HIPCHK(hipMemcpyAsync(out, src.p, recBytes * n, hipMemcpyDeviceToHost, ctx->stream)); HIPCHK(streamSync(ctx));
    return pfLeave();
}
int ygpu_pileup_candidates_size(ygpu_ctx *full, uint64_t *n)
{
    if (!full || !full->stream || !n) return YGPU_EINVAL;
    if (!full->track[TRACK_PILEUP]) return pfArgError(full, "ygpu_pileup_candidates_size: ygpu_pileup_enable has not been called on this context");
    PfSide *ctx = pfEnter(full);
    HIPCHK(hipSetDevice(full->device));
    HIPCHK(hipDeviceSynchronize());
    const TrackImage &T = *full->track[TRACK_PILEUP];
    full->puHaveCand = false; full->puNCand = 0;
    int rc = pileupSide(full); if (rc) return rc;
    CandidateSel A; A.L = trackLayout(T); A.pu = T.data.as<uint32_t>(); A.nSlots = (uint32_t)T.nBins; A.bases = full->dBases.as<uint8_t>(); A.nBaseBytes = full->dBases.cap;
    A.out = nullptr;
    TileSel t; uint32_t tot = 0;
    rc = selectCount(full, TILES_PILEUP, A, T.nBins, "pileup candidates", &t, &tot); if (rc) return rc;
    ENSURE(full->puCand, 4ull * ((uint64_t)tot + 1));
    A.out = full->puCand.as<uint32_t>(); t.cap = tot;
    if (tot) KL(k_select_emit<CandidateSel>, selectGrid(t), dim3(256), 0, ctx->stream, A, t);
    HIPCHK(streamSync(ctx));
    full->puNCand = tot; full->puHaveCand = true; *n = tot;
    return pfLeave();
}
int ygpu_pileup_candidates_collect(ygpu_ctx *full, uint32_t *slots)
{
    if (!full || !full->stream) return YGPU_EINVAL;
    return collectRecords(full, full->puHaveCand, "ygpu_pileup_candidates_collect: ygpu_pileup_candidates_size has not been called on this context", full->puNCand, slots,
        full->puCand, 4);
}
// Rows of the image's array for a caller's slots, a piece of the list at a time (the list and its rows pass through buffers of the context): read into rows[i][ch]
// (the gather), or -- a source folded into the array: the host's blocks, another image's rows -- added from them with global atomics (snv_stage.h k_pileup_add).
static int pileupRows(ygpu_ctx *full, const char *who, const uint32_t *slots, uint32_t *rows, uint64_t n, bool add)
{
    if (!full || !full->stream || (n && (!slots || !rows))) return YGPU_EINVAL;
    if (!full->track[TRACK_PILEUP]) return pfArgError(full, std::string(who) + ": ygpu_pileup_enable has not been called on this context");
    PfSide *ctx = pfEnter(full);
    HIPCHK(hipSetDevice(full->device));
    HIPCHK(hipDeviceSynchronize());
    const TrackImage &T = *full->track[TRACK_PILEUP];
    const uint64_t piece = 1ull << 22;
    for (uint64_t at = 0; at < n; at += piece) {
        const uint32_t m = (uint32_t)std::min<uint64_t>(piece, n - at); const dim3 grid(gridFor((uint64_t)m * ypileup::NCH, 256));
        ENSURE(full->puSlots, 4ull * m); ENSURE(full->puRows, 4ull * ypileup::NCH * m);
        HIPCHK(hipMemcpyAsync(full->puSlots.p, slots + at, 4ull * m, hipMemcpyHostToDevice, ctx->stream));
        if (add) {
            HIPCHK(hipMemcpyAsync(full->puRows.p, rows + at * ypileup::NCH, 4ull * ypileup::NCH * m, hipMemcpyHostToDevice, ctx->stream));
            KL(k_pileup_add, grid, dim3(256), 0, ctx->stream, T.data.as<uint32_t>(), (uint32_t)T.nBins, full->puSlots.as<uint32_t>(), full->puRows.as<uint32_t>(), m);
        } else {
            KL(k_pileup_gather, grid, dim3(256), 0, ctx->stream, T.data.as<uint32_t>(), (uint32_t)T.nBins, full->puSlots.as<uint32_t>(), m, full->puRows.as<uint32_t>());
            HIPCHK(hipMemcpyAsync(rows + at * ypileup::NCH, full->puRows.p, 4ull * ypileup::NCH * m, hipMemcpyDeviceToHost, ctx->stream));
        }
        HIPCHK(streamSync(ctx));                                               // (the caller's memory is pageable: the next piece may overwrite the buffers only now)
    }
    return pfLeave();
}
int ygpu_pileup_gather(ygpu_ctx *full, const uint32_t *slots, uint64_t n, uint32_t *rows) { return pileupRows(full, "ygpu_pileup_gather", slots, rows, n, false); }
// ---- SNV calls from the pileup array (snv_stage.h; the contract is in ../snv_core.h) -----------------------------------------------------------------------------
int ygpu_pileup_add(ygpu_ctx *full, const uint32_t *slots, const uint32_t *rows, uint64_t n)
{
    return pileupRows(full, "ygpu_pileup_add", slots, const_cast<uint32_t *>(rows), n, true);
}
// The calls of the image's array as it stands, ascending -- the candidates' steps with the verdict of snv_core.h in the place of the site test; the tiles'
// counts and sums live in the candidates' buffers (a selection of either kind leaves the other's RESULT alone).
int ygpu_snv_call_size(ygpu_ctx *full, const ygpu_snv_params *p, uint64_t *n)
{
    if (!full || !full->stream || !p || !n) return YGPU_EINVAL;
    if (!full->track[TRACK_PILEUP]) return pfArgError(full, "ygpu_snv_call_size: ygpu_pileup_enable has not been called on this context");
    if (p->min_alt < 1 || p->min_depth < 1) return pfArgError(full, "ygpu_snv_call_size: min_alt and min_depth must be at least 1");
    PfSide *ctx = pfEnter(full);
    HIPCHK(hipSetDevice(full->device));
    HIPCHK(hipDeviceSynchronize());
    const TrackImage &T = *full->track[TRACK_PILEUP];
    full->snvHave = false; full->snvN = 0;
    int rc = pileupSide(full); if (rc) return rc;
    SnvSel A; A.L = trackLayout(T); A.pu = T.data.as<uint32_t>(); A.nSlots = (uint32_t)T.nBins; A.bases = full->dBases.as<uint8_t>(); A.nBaseBytes = full->dBases.cap;
    A.P = *p; A.out = nullptr;
    TileSel t; uint32_t tot = 0;
    rc = selectCount(full, TILES_PILEUP, A, T.nBins, "SNV calls", &t, &tot); if (rc) return rc;
    ENSURE(full->snvOut, sizeof(ygpu_snv_call) * ((uint64_t)tot + 1));
    A.out = full->snvOut.as<ygpu_snv_call>(); t.cap = tot;
    if (tot) KL(k_select_emit<SnvSel>, selectGrid(t), dim3(256), 0, ctx->stream, A, t);
    HIPCHK(streamSync(ctx));
    full->snvN = tot; full->snvHave = true; *n = tot;
    return pfLeave();
}
int ygpu_snv_collect(ygpu_ctx *full, ygpu_snv_call *calls)
{
    if (!full || !full->stream) return YGPU_EINVAL;
    return collectRecords(full, full->snvHave && full->snvOut.p, "ygpu_snv_collect: ygpu_snv_call_size has not been called on this context", full->snvN, calls,
        full->snvOut, sizeof(ygpu_snv_call));
}
// ---- indel alleles (indel_stage.h; the contract is in ../indel_core.h) -------------------------------------------------------------------------------------------
// Per context, as the junctions are: a hash table of the context's own, fed by every ygpu_postfilter, drained by ygpu_indels_collect.
int ygpu_indels_enable(ygpu_ctx *full, const ygpu_indel_params *p)
{
    if (!full || !full->stream || !p) return YGPU_EINVAL;
    if (!full->oqSet) return pfArgError(full, "ygpu_indels_enable: ygpu_set_postfilter has not been called on this context (the alleles are counted behind the post-filter)");
    if (!p->n_seqs || !p->seq_start || !p->seq_length || p->min_mapq > 255 || p->min_length < 1)
        return pfArgError(full, "ygpu_indels_enable: bad mapping quality, minimum length or sequence table");
    if (p->capacity && ((p->capacity & (p->capacity - 1)) != 0 || p->capacity > (1ull << 31)))
        return pfArgError(full, "ygpu_indels_enable: the capacity must be a power of two of at most 2^31 entries (0: twice the batch capacity in bases)");
    if (full->parked) return pfArgError(full, "ygpu_indels_enable: the context was parked (ygpu_park)");
    std::vector<uint32_t> binBase(p->n_seqs + 1); uint64_t nSlots = 0;
    if (!ydepth::layoutBins(p->seq_length, p->n_seqs, 1, binBase.data(), &nSlots) || nSlots == 0) return pfArgError(full, "ygpu_indels_enable: the slots do not fit 32 bits");
    PfSide *ctx = pfEnter(full);
    HIPCHK(hipSetDevice(full->device));
    HIPCHK(streamSync(ctx));                                                   // (a second enable: nothing of this side may still be using the table)
    ENSURE(full->idSeqStart, 4ull * p->n_seqs); ENSURE(full->idSeqLen, 4ull * p->n_seqs); ENSURE(full->idBinBase, 4ull * (p->n_seqs + 1)); ENSURE(full->idStats, 128);
    // the rule: twice the bases of the largest batch the context has held -- what its buffer of forward codes holds -- and at least 2^20 of them
    const uint64_t capacity = p->capacity ? p->capacity : yindel::tableCapacity(std::max<uint64_t>(1ull << 20, std::max<uint64_t>(full->totalBases, full->snapBases)));
    full->idSet = false;
    int rc = indelTable(full, capacity); if (rc) return rc;
    HIPCHK(hipMemcpyAsync(full->idSeqStart.p, p->seq_start, 4ull * p->n_seqs, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(hipMemcpyAsync(full->idSeqLen.p, p->seq_length, 4ull * p->n_seqs, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(hipMemcpyAsync(full->idBinBase.p, binBase.data(), 4ull * (p->n_seqs + 1), hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(streamSync(ctx));
    full->idMinMapq = p->min_mapq; full->idMinLen = p->min_length; full->idNSeqs = p->n_seqs; full->idAuto = p->capacity == 0; full->idSet = true;
    return pfLeave();
}
int ygpu_indels_size(ygpu_ctx *ctx, uint64_t *used)
{
    if (!ctx || !ctx->stream || !used) return YGPU_EINVAL;
    if (!ctx->idSet) { ctx->err = "ygpu_indels_size: ygpu_indels_enable has not been called on this context"; return YGPU_EINVAL; }
    *used = ctx->idTable.p ? ctx->idUsed : 0; return 0;
}
int ygpu_indels_collect(ygpu_ctx *full, ygpu_indel_entry *out, uint64_t stats[6])
{
    if (!full || !full->stream) return YGPU_EINVAL;
    if (!full->idSet) return pfArgError(full, "ygpu_indels_collect: ygpu_indels_enable has not been called on this context");
    pfLeave();                                                                 // (an earlier call's failure is not this call's: the returns below leave no name behind)
    if (stats) for (int k = 0; k < 6; k++) stats[k] = 0;
    if (!full->idTable.p) return 0;                                            // (parked: the table went with the arenas)
    if (full->idUsed && !out) return YGPU_EINVAL;
    PfSide *ctx = pfEnter(full);
    HIPCHK(hipSetDevice(full->device));
    int rc = pileupSide(full); if (rc) return rc;
    IndelDrainSel A; A.table = full->idTable.as<ygpu_indel_entry>(); A.capacity = full->idCap; A.out = nullptr;
    TileSel t; uint32_t tot = 0; unsigned long long h[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    rc = selectCount(full, TILES_INDEL, A, full->idCap, "indel alleles", &t, &tot, {full->idStats.p, (uint32_t *)h, 18}); if (rc) return rc;
    // (the caller sized `out` by ygpu_indels_size: after a ygpu_postfilter that failed half-way the two may differ -- the size is put right, the call fails)
    if (tot != full->idUsed) { char m[200]; snprintf(m, sizeof m, "ygpu_indels_collect: %u occupied entries, ygpu_indels_size said %u (it now says %u: collect again)", tot,
        full->idUsed, tot); ctx->err = m; full->idUsed = tot; return YGPU_EINTERNAL; }
    if (tot) {
        ENSURE(full->idOut, sizeof(ygpu_indel_entry) * (uint64_t)tot);
        A.out = full->idOut.as<ygpu_indel_entry>(); t.cap = tot;
        KL(k_select_emit<IndelDrainSel>, selectGrid(t), dim3(256), 0, ctx->stream, A, t);
        HIPCHK(hipMemcpyAsync(out, full->idOut.p, sizeof(ygpu_indel_entry) * (uint64_t)tot, hipMemcpyDeviceToHost, ctx->stream));
    }
    // ... and the table, its statistics and the two words are clean for the next batch
    HIPCHK(hipMemsetAsync(full->idTable.p, 0, sizeof(ygpu_indel_entry) * full->idCap, ctx->stream));
    HIPCHK(hipMemsetAsync(full->idStats.p, 0, 128, ctx->stream));
    HIPCHK(streamSync(ctx));
    full->idUsed = 0;
    if (stats) { for (int k = 0; k < 5; k++) stats[k] = h[k]; stats[5] = (uint32_t)(h[8] >> 32); }
    return pfLeave();
}
// ---- indel calls (indelcall_stage.h; the contract is in ../indelcall_core.h) --------------------------------------------------------------------------------------
// The raw alleles normalised against the image's reference and merged in a table of the context's own, made (and cleared) for the call; the layout is the
// pileup's.  On the post-filter's side of the context, once everything queued on the device has finished; serves a parked context as the SNV calls do.
static const auto indelKeyLess = [](const auto &a, const auto &b) { return yindel::keyLess(yindel::Key{a.w0, a.w1, a.w2}, yindel::Key{b.w0, b.w1, b.w2}); };
int ygpu_indelcall_normalize(ygpu_ctx *full, const ygpu_indel_entry *raw, uint64_t n, uint32_t max_shift, uint64_t *n_out, uint64_t stats[4])
{
    if (!full || !full->stream || !n_out || (n && !raw)) return YGPU_EINVAL;
    if (!full->track[TRACK_PILEUP]) return pfArgError(full, "ygpu_indelcall_normalize: ygpu_pileup_enable has not been called on this context (the layout is the pileup's)");
    if (max_shift > (uint32_t)yindelcall::MAX_SHIFT || n > (1ull << 30)) return pfArgError(full, "ygpu_indelcall_normalize: max_shift must be at most 65535, n at most 2^30");
    PfSide *ctx = pfEnter(full);
    HIPCHK(hipSetDevice(full->device));
    HIPCHK(hipDeviceSynchronize());
    const TrackImage &T = *full->track[TRACK_PILEUP];
    full->icHave = full->icHaveCalls = false; full->icN = full->icCalls = 0;
    if (stats) { stats[0] = n; stats[1] = stats[2] = stats[3] = 0; }
    *n_out = 0;
    if (n == 0) { full->icHave = true; return pfLeave(); }
    int rc = pileupSide(full); if (rc) return rc;
    uint64_t capacity = 1024; while (capacity < 2 * n) capacity <<= 1;
    ENSURE(full->icRaw, sizeof(ygpu_indel_entry) * n); ENSURE(full->icTable, sizeof(ygpu_indel_entry) * capacity); ENSURE(full->icStats, 64);
    full->icCap = capacity;
    HIPCHK(hipMemcpyAsync(full->icRaw.p, raw, sizeof(ygpu_indel_entry) * n, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(hipMemsetAsync(full->icTable.p, 0, sizeof(ygpu_indel_entry) * capacity, ctx->stream));
    HIPCHK(hipMemsetAsync(full->icStats.p, 0, 64, ctx->stream));
    IndelNormArgs N; N.L = trackLayout(T); N.nSlots = T.nBins; N.bases = full->dBases.as<uint8_t>(); N.nBaseBytes = full->dBases.cap;
    N.raw = full->icRaw.as<ygpu_indel_entry>(); N.n = (uint32_t)n; N.maxShift = max_shift; N.table = full->icTable.as<ygpu_indel_entry>(); N.mask = (uint32_t)(capacity - 1);
    N.stats = full->icStats.as<unsigned long long>(); N.used = full->icStats.as<uint32_t>() + 8;
    KL(k_indel_norm, dim3(gridFor(n * 64, 256)), dim3(256), 0, ctx->stream, N);
    // the table's occupied entries, compacted: the indel table's pick, the store that saturates
    IndelMergeDrainSel A; A.table = full->icTable.as<ygpu_indel_entry>(); A.capacity = capacity; A.out = nullptr;
    TileSel t; uint32_t tot = 0; unsigned long long h[4] = {0, 0, 0, 0};
    rc = selectCount<IndelDrainSel>(full, TILES_INDEL, A, capacity, "indel calls", &t, &tot, {full->icStats.p, (uint32_t *)h, 8}); if (rc) return rc;      // (the pick is shared)
    if (h[2]) { ctx->err = "ygpu_indelcall_normalize: a normalised allele found no entry in the merge table"; return YGPU_EINTERNAL; }
    if (tot) {
        ENSURE(full->icAlleles, sizeof(ygpu_indel_entry) * (uint64_t)tot);
        A.out = full->icAlleles.as<ygpu_indel_entry>(); t.cap = tot;
        KL(k_select_emit<IndelMergeDrainSel>, selectGrid(t), dim3(256), 0, ctx->stream, A, t);
    }
    HIPCHK(streamSync(ctx));
    full->icN = tot; full->icHave = true; *n_out = tot;
    if (stats) { stats[1] = h[0]; stats[3] = h[1]; stats[2] = n - h[1] - tot; }
    return pfLeave();
}
int ygpu_indelcall_alleles(ygpu_ctx *full, ygpu_indel_entry *out)
{
    if (!full || !full->stream) return YGPU_EINVAL;
    const int rc = collectRecords(full, full->icHave, "ygpu_indelcall_alleles: ygpu_indelcall_normalize has not been called on this context", full->icN, out,
        full->icAlleles, sizeof(ygpu_indel_entry));
    if (rc == 0 && full->icN) std::sort(out, out + full->icN, indelKeyLess);      // (the table keeps no order: see the header)
    return rc;
}
// The calls among the merged alleles against the image's array as it stands: the SNV calls' steps, a lane an allele.
int ygpu_indelcall_size(ygpu_ctx *full, const ygpu_indelcall_params *p, uint64_t *n)
{
    if (!full || !full->stream || !p || !n) return YGPU_EINVAL;
    if (!full->track[TRACK_PILEUP]) return pfArgError(full, "ygpu_indelcall_size: ygpu_pileup_enable has not been called on this context");
    if (!full->icHave) return pfArgError(full, "ygpu_indelcall_size: ygpu_indelcall_normalize has not been called on this context");
    if (p->min_alt < 1 || p->min_depth < 1) return pfArgError(full, "ygpu_indelcall_size: min_alt and min_depth must be at least 1");
    PfSide *ctx = pfEnter(full);
    HIPCHK(hipSetDevice(full->device));
    HIPCHK(hipDeviceSynchronize());
    full->icHaveCalls = false; full->icCalls = 0; *n = 0;
    if (!full->icN || !full->icAlleles.p) { full->icHaveCalls = true; return pfLeave(); }
    const TrackImage &T = *full->track[TRACK_PILEUP];
    int rc = pileupSide(full); if (rc) return rc;
    IndelCallSel A; A.L = trackLayout(T); A.pu = T.data.as<uint32_t>(); A.nSlots = (uint32_t)T.nBins; A.bases = full->dBases.as<uint8_t>(); A.nBaseBytes = full->dBases.cap;
    A.alleles = full->icAlleles.as<ygpu_indel_entry>(); A.n = (uint32_t)full->icN; A.P = *p; A.out = nullptr;
    TileSel t; uint32_t tot = 0;
    rc = selectCount(full, TILES_INDEL, A, A.n, "indel calls", &t, &tot); if (rc) return rc;
    ENSURE(full->icOut, sizeof(ygpu_indel_call) * ((uint64_t)tot + 1));
    A.out = full->icOut.as<ygpu_indel_call>(); t.cap = tot;
    if (tot) KL(k_select_emit<IndelCallSel>, selectGrid(t), dim3(256), 0, ctx->stream, A, t);
    HIPCHK(streamSync(ctx));
    full->icCalls = tot; full->icHaveCalls = true; *n = tot;
    return pfLeave();
}
int ygpu_indelcall_collect(ygpu_ctx *full, ygpu_indel_call *calls)
{
    if (!full || !full->stream) return YGPU_EINVAL;
    const int rc = collectRecords(full, full->icHaveCalls, "ygpu_indelcall_collect: ygpu_indelcall_size has not been called on this context", full->icCalls, calls,
        full->icOut, sizeof(ygpu_indel_call));
    if (rc == 0 && full->icCalls) std::sort(calls, calls + full->icCalls, indelKeyLess);
    return rc;
}
// ---- the error profile (eprofile_stage.h; the contract is in ../eprofile_core.h) ------------------------------------------------------------------------------
// Per context, as the indel alleles are: a table of the context's own, fed by every ygpu_postfilter, read (not cleared) by ygpu_eprofile_collect.
int ygpu_eprofile_enable(ygpu_ctx *full, const ygpu_eprofile_params *p)
{
    if (!full || !full->stream || !p) return YGPU_EINVAL;
    if (!full->oqSet) return pfArgError(full, "ygpu_eprofile_enable: ygpu_set_postfilter has not been called on this context (the profile is counted behind the post-filter)");
    if (!p->n_seqs || !p->seq_start || !p->seq_length || p->min_mapq > 255) return pfArgError(full, "ygpu_eprofile_enable: bad mapping quality or sequence table");
    if (full->parked) return pfArgError(full, "ygpu_eprofile_enable: the context was parked (ygpu_park)");
    PfSide *ctx = pfEnter(full);
    HIPCHK(hipSetDevice(full->device));
    HIPCHK(streamSync(ctx));                                                   // (a second enable: nothing of this side may still be using the table)
    full->epSet = false;
    ENSURE(full->epTable, 8ull * YE_LDS_WORDS); ENSURE(full->epSeqs, 8ull * p->n_seqs);
    HIPCHK(hipMemsetAsync(full->epTable.p, 0, 8ull * YE_LDS_WORDS, ctx->stream));
    HIPCHK(hipMemcpyAsync(full->epSeqs.p, p->seq_start, 4ull * p->n_seqs, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(hipMemcpyAsync(full->epSeqs.as<uint32_t>() + p->n_seqs, p->seq_length, 4ull * p->n_seqs, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(streamSync(ctx));
    full->epMinMapq = p->min_mapq; full->epNSeqs = p->n_seqs; full->epSet = true;
    return pfLeave();
}
int ygpu_eprofile_size(ygpu_ctx *ctx, uint64_t *n_words)
{
    if (!ctx || !n_words) return YGPU_EINVAL;
    if (!ctx->epSet) { ctx->err = "ygpu_eprofile_size: ygpu_eprofile_enable has not been called on this context"; return YGPU_EINVAL; }
    *n_words = YGPU_EPROFILE_WORDS; return 0;
}
// The context's table as it stands: every filter stage queued on this context's post-filter side so far has finished when the copy is taken.
int ygpu_eprofile_collect(ygpu_ctx *full, uint64_t *words, uint64_t stats[4])
{
    if (!full || !full->stream) return YGPU_EINVAL;
    if (!full->epSet) return pfArgError(full, "ygpu_eprofile_collect: ygpu_eprofile_enable has not been called on this context");
    unsigned long long h[YE_LDS_WORDS]; memset(h, 0, sizeof h);
    if (full->epTable.p) {                                                     // (parked: the table went with the arenas -- a parked context never ran a batch)
        PfSide *ctx = pfEnter(full);
        HIPCHK(hipSetDevice(full->device));
        HIPCHK(hipMemcpyAsync(h, full->epTable.p, sizeof h, hipMemcpyDeviceToHost, ctx->stream)); HIPCHK(streamSync(ctx));
    }
    if (words) for (uint32_t k = 0; k < (uint32_t)yeprofile::WORDS; k++) words[k] = h[k];
    if (stats) for (uint32_t k = 0; k < 4; k++) stats[k] = h[yeprofile::WORDS + k];
    return pfLeave();
}
// ---- split-read junctions (junction_stage.h; the contract is in ../junction_core.h) --------------------------------------------------------------------------
// Per batch and per context, unlike the binned tracks above: the junctions of the batch the context's last ygpu_postfilter filtered.
int ygpu_junctions_enable(ygpu_ctx *ctx, const ygpu_junction_params *p)
{
    if (!ctx || !ctx->stream || !p) return YGPU_EINVAL;
    if (!ctx->oqSet) { ctx->err = "ygpu_junctions_enable: ygpu_set_postfilter has not been called on this context (the junctions are made behind the post-filter)";
        return YGPU_EINVAL; }
    if (!p->n_seqs || !p->seq_start || !p->seq_length || p->min_mapq > 255) { ctx->err = "ygpu_junctions_enable: bad mapping quality or sequence table"; return YGPU_EINVAL; }
    HIPCHK(hipSetDevice(ctx->device));
    ENSURE(ctx->jnSeqStart, 4ull * p->n_seqs); ENSURE(ctx->jnSeqLen, 4ull * p->n_seqs); ENSURE(ctx->jnStats, 64);
    HIPCHK(hipMemcpyAsync(ctx->jnSeqStart.p, p->seq_start, 4ull * p->n_seqs, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(hipMemcpyAsync(ctx->jnSeqLen.p, p->seq_length, 4ull * p->n_seqs, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(streamSync(ctx));
    ctx->jnMinMapq = p->min_mapq; ctx->jnNSeqs = p->n_seqs; ctx->jnSet = true; ctx->jnDone = false;
    return 0;
}
// the number of junctions of the filtered batch: the last word of the exclusive sums, fetched once (with the flag of a look-back that gave up)
static int junctionsTotal(ygpu_ctx *full, const char *who)
{
    if (!full->jnSet) return pfArgError(full, std::string(who) + ": ygpu_junctions_enable has not been called on this context");
    if (!full->jnDone) return pfArgError(full, std::string(who) + ": no ygpu_postfilter has run on this context since ygpu_junctions_enable");
    if (full->jnHaveTotal) return 0;
    if (full->jnReads == 0) { full->jnTotal = 0; full->jnHaveTotal = true; return 0; }
    PfSide *ctx = pfEnter(full);
    HIPCHK(hipSetDevice(full->device));
    uint32_t tot = 0;
    const int rc = fetchTotal(ctx, full->jnStart.as<uint32_t>() + full->jnReads, "junctions", &tot); if (rc) return rc;
    pfLeave();
    if ((uint64_t)tot * sizeof(ygpu_junction) > full->jnOut.cap) { full->err = std::string(who) + ": more junctions than the batch has clumps"; return YGPU_EINTERNAL; }
    full->jnTotal = tot; full->jnHaveTotal = true;
    return 0;
}
int ygpu_junctions_size(ygpu_ctx *ctx, uint64_t *n)
{
    if (!ctx || !ctx->stream || !n) return YGPU_EINVAL;
    const int rc = junctionsTotal(ctx, "ygpu_junctions_size"); if (rc) return rc;
    *n = ctx->jnTotal; return 0;
}
int ygpu_junctions_collect(ygpu_ctx *full, ygpu_junction *out, uint64_t stats[4])
{
    if (!full || !full->stream) return YGPU_EINVAL;
    const int rc = junctionsTotal(full, "ygpu_junctions_collect"); if (rc) return rc;
    if (stats) for (int k = 0; k < 4; k++) stats[k] = 0;
    if (full->jnReads == 0) return 0;
    PfSide *ctx = pfEnter(full);
    HIPCHK(hipSetDevice(full->device));
    unsigned long long h[4] = {0, 0, 0, 0};
    if (out && full->jnTotal) HIPCHK(hipMemcpyAsync(out, full->jnOut.p, sizeof(ygpu_junction) * (uint64_t)full->jnTotal, hipMemcpyDeviceToHost, ctx->stream));
    if (stats) HIPCHK(hipMemcpyAsync(h, full->jnStats.p, sizeof h, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(streamSync(ctx));
    if (stats) for (int k = 0; k < 4; k++) stats[k] = h[k];
    return pfLeave();
}
int ygpu_inject_results(ygpu_ctx *ctx, const ygpu_result_batch *r)
{
    if (!ctx || !ctx->stream || !r || r->n_reads != ctx->nReads || !r->clump_start || (r->n_clumps && !r->clumps) || (r->n_ops && !r->ops) || r->n_clumps > 0x7FFFFFF0ull
        || r->n_ops > 0x7FFFFFF0ull) return YGPU_EINVAL;
    HIPCHK(hipSetDevice(ctx->device));
    const uint32_t n = ctx->nReads;
    ENSURE(ctx->readStart, 4ull * (n + 1)); ENSURE(ctx->outClumps2, sizeof(ygpu_clump) * (r->n_clumps + 1)); ENSURE(ctx->outOps, 4ull * (r->n_ops + 1));
        ENSURE(ctx->ctr, sizeof(DevCounters));
    HIPCHK(hipMemcpyAsync(ctx->readStart.p, r->clump_start, 4ull * (n + 1), hipMemcpyHostToDevice, ctx->stream));
    if (r->n_clumps) HIPCHK(hipMemcpyAsync(ctx->outClumps2.p, r->clumps, sizeof(ygpu_clump) * r->n_clumps, hipMemcpyHostToDevice, ctx->stream));
    if (r->n_ops) HIPCHK(hipMemcpyAsync(ctx->outOps.p, r->ops, 4ull * r->n_ops, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(streamSync(ctx));
    ctx->nOut = (uint32_t)r->n_clumps; ctx->nOutOps = (uint32_t)r->n_ops; ctx->stageDone = 3;
    return 0;
}
int ygpu_postfilter_drop(ygpu_ctx *ctx)
{
    if (!ctx || !ctx->stream) return YGPU_EINVAL;
    ctx->pfSnap.store(false); ctx->oqDone = false; ctx->nFOut = ctx->nFOps = 0; ctx->jnDone = false;
    return 0;
}
int ygpu_filtered_size(ygpu_ctx *ctx, uint64_t *n_clumps, uint64_t *n_ops)
{
    if (!ctx || !ctx->oqDone) return YGPU_EINVAL;
    if (n_clumps) *n_clumps = ctx->nFOut; if (n_ops) *n_ops = ctx->nFOps;
    return 0;
}
int ygpu_collect_filtered(ygpu_ctx *full, uint32_t *clump_start, ygpu_out_clump *clumps, uint32_t *ops, ygpu_filtered_batch *out)
{
    if (!full || !out || !clump_start || !full->oqDone || (full->nFOut && !clumps) || (full->nFOps && !ops)) return YGPU_EINVAL;
    PfSide *ctx = pfEnter(full);
    HIPCHK(hipSetDevice(full->device));
    const uint32_t n = full->pfN;
    HIPCHK(hipMemcpyAsync(clump_start, full->oqOutStart.p, 4ull * (n + 1), hipMemcpyDeviceToHost, ctx->stream));
    if (full->nFOut) HIPCHK(hipMemcpyAsync(clumps, full->oqFClumps.p, sizeof(ygpu_out_clump) * (uint64_t)full->nFOut, hipMemcpyDeviceToHost, ctx->stream));
    if (full->nFOps) HIPCHK(hipMemcpyAsync(ops, full->oqFOps.p, 4ull * full->nFOps, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(streamSync(ctx));
    // (collected: a later ygpu_filtered_size without a new ygpu_postfilter is an error, not the previous batch once more)
    full->oqDone = false;
    out->n_reads = n; out->clump_start = clump_start; out->clumps = clumps; out->ops = ops; out->n_clumps = full->nFOut; out->n_ops = full->nFOps; out->counters = full->pfCounters;
    return pfLeave();
}
}  // extern "C"

// the post-filter's sort on the wave (oqc_stage.h waveSort) against the one-thread routine it stands for (oqc_core.h sortRange, the reference's quicksort with its
// random tie breaks): arrays of 2 .. YQ_DEVICE_MAX entries around the 64-lane edges, keys from 2 to 4 096 distinct values (ties by the hundred down to none), random,
// ascending and descending; every entry must land where the routine puts it
int ydSelftestWaveSort(ygpu_ctx *ctx, uint32_t seed, uint64_t &x)
{
    auto rnd = [&]() { x ^= x << 13; x ^= x >> 7; x ^= x << 17; return x; };
    DevBuf a; struct Rel { DevBuf &a; ~Rel() { a.release(); } } rel{a};
    {
        static const int fixedLen[] = {2, 3, 4, 5, 9, 17, 33, 63, 64, 65, 66, 100, 127, 128, 129, 130, 191, 192, 193, 300, 448, 449, 700, 1000, 1500, YQ_DEVICE_MAX};
        const uint32_t nArr = 56; std::vector<uint32_t> off(nArr + 1, 0), seeds(5 * nArr); std::vector<uint64_t> ent;
        for (uint32_t t = 0; t < nArr; t++) {
            const int len = t < sizeof fixedLen / sizeof fixedLen[0] ? fixedLen[t] : 2 + (int)(rnd() % (YQ_DEVICE_MAX - 1));
            const uint64_t span = 1ull << (1 + (seed * 7u + t) % 12u); const int shape = (int)(rnd() % 5);
            for (int i = 0; i < len; i++) { uint64_t k = rnd() % span; if (shape == 3) k = (uint64_t)i * span / len; if (shape == 4) k = (uint64_t)(len - 1 - i) * span / len;
                ent.push_back((k << 16) | (uint64_t)i); }
            for (int k = 0; k < 5; k++) seeds[5 * t + k] = (uint32_t)rnd();
            off[t + 1] = off[t] + (uint32_t)len;
        }
        std::vector<uint64_t> want(ent.size()), got(ent.size());
        for (uint32_t t = 0; t < nArr; t++) {
            const int len = (int)(off[t + 1] - off[t]); std::vector<yoqc::SortKey> sk(len); std::vector<int> stk(4 * len + 16);
            for (int i = 0; i < len; i++) { sk[i].key = ent[off[t] + i] >> 16; sk[i].clump = i; sk[i].pad = 0; }
            yoqc::Rand rs; for (int k = 0; k < 5; k++) rs.s[k] = seeds[5 * t + k];
            yoqc::Run::sortRange(sk.data(), len, stk.data(), (int)stk.size(), stk.data(), rs);
            for (int i = 0; i < len; i++) want[off[t] + i] = (sk[i].key << 16) | (uint64_t)(uint32_t)sk[i].clump;
        }
        DevBuf dOff, dSeeds, dStack; struct Rel2 { DevBuf &a, &b, &c; ~Rel2() { a.release(); b.release(); c.release(); } } rel2{dOff, dSeeds, dStack};
        if (a.ensure(8ull * ent.size()) || dOff.ensure(4ull * off.size()) || dSeeds.ensure(4ull * seeds.size()) || dStack.ensure(4ull * (2ull * ent.size() + 8ull * nArr + 16))) {
            ctx->err = "hipMalloc failed"; return YGPU_ENOMEM; }
        HIPCHK(hipMemcpyAsync(a.p, ent.data(), 8ull * ent.size(), hipMemcpyHostToDevice, ctx->stream));
            HIPCHK(hipMemcpyAsync(dOff.p, off.data(), 4ull * off.size(), hipMemcpyHostToDevice, ctx->stream));
        HIPCHK(hipMemcpyAsync(dSeeds.p, seeds.data(), 4ull * seeds.size(), hipMemcpyHostToDevice, ctx->stream));
        KL(k_oqc_sort_test, dim3(nArr), dim3(64), 4u * YQ_STACK_LDS + 20u * YQ_DEVICE_MAX, ctx->stream, a.as<uint64_t>(), dOff.as<uint32_t>(), dSeeds.as<uint32_t>(),
            dStack.as<int>(), nArr);
        HIPCHK(hipMemcpyAsync(got.data(), a.p, 8ull * ent.size(), hipMemcpyDeviceToHost, ctx->stream)); HIPCHK(streamSync(ctx));
        for (uint32_t t = 0; t < nArr; t++) for (uint32_t i = off[t]; i < off[t + 1]; i++) if (got[i] != want[i]) {
            char m[200]; snprintf(m, sizeof m, "selftest: the sort on the wave differs from the one-thread routine: array %u (%u entries), position %u", t, off[t + 1] - off[t],
                i - off[t]); ctx->err = m; return YGPU_EINTERNAL; }
    }
    return 0;
}
