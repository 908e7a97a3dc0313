/* yaha_hip.h -- C-ABI of the MI355X-native hot path of YAHA (seed join -> clumps -> banded affine-gap DP ->
 * score/split).  Plain pointers and sizes only; no torch, no C++ types.
 *
 * The reference (GregoryFaust/yaha v0.1.83) has no plugin/FFI seam: its hot path is the body of the per-read
 * loop in src/Query.c:306-497, which calls (all declared in src/Math.h)
 *     findFragmentsSort        Math.h:554   (QueryMatch.c:52)     -> ygpu stage A1+A2
 *     processFragmentsGapped   Math.h:555   (QueryMatch.c:224)    -> ygpu stage A3+A4
 *     postProcessClumps        Math.h:539   (QueryMatch.c:306)    -> ygpu stage A5..A8
 *       alignClump/scoreClump  Math.h:537-538, findAGS* Math.h:401-410, extendClump* Math.h:535-536
 * on one QueryState_t (Math.h:587-666) per thread.  This header is the *batched* replacement of that loop
 * body: a whole batch of reads is handed over, and for every read the clump list that postProcessClumps
 * leaves in QS->clumps (head -> tail order, QueryMatch.c:309-330) comes back, ready for the host's
 * postFilterBySimilarity / printClump stages.
 *
 * Conventions: every function returns 0 on success or a negative YGPU_E* code; nothing ever calls exit().
 * The caller owns inputs until the call returns.  Results are owned by the context and stay valid until the
 * next ygpu_run on that context.  One context per device, one host thread per context (mirrors one
 * QueryState_t per thread, Query.c:642-684).
 */
#ifndef YAHA_HIP_H
#define YAHA_HIP_H
#include <stdint.h>
#include <stddef.h>
#ifdef __cplusplus
extern "C" {
#endif

#define YGPU_OK            0
#define YGPU_EINVAL      (-1)   /* bad argument / unsupported parameter range            */
#define YGPU_ENODEV      (-2)   /* no HIP device / HIP runtime error                     */
#define YGPU_ENOMEM      (-3)   /* device or host allocation failed                      */
#define YGPU_EOVERFLOW   (-4)   /* a device arena overflowed even after regrowth         */
#define YGPU_EINTERNAL   (-5)
#define YGPU_EBUSY       (-6)   /* ygpu_submit while the context's previous ticket is still open */

/* Alignment parameters: the subset of AlignmentArgs_t (Math.h:257-334) the hot path reads, after
 * postProcessAlignmentArgs (AlignArgs.c:108-169) has filled the derived ones. */
typedef struct ygpu_params {
    int32_t wordLen;        /* -L, from the index header (Query.c:603)                         */
    int32_t maxHits;        /* min(-H, index header maxHits) (Query.c:604-610)                 */
    int32_t bandWidth;      /* -BW                                                             */
    int32_t maxGap;         /* -G                                                              */
    int32_t maxIntron;      /* -I, default = maxGap (AlignArgs.c:111)                          */
    int32_t minMatch;       /* -M                                                              */
    int32_t maxDesert;      /* -MD                                                             */
    int32_t minNonOverlap;  /* = OQCMinNonOverlap = -MNO, default minMatch (AlignArgs.c:115-125) */
    int32_t minRawScore;    /* -R, default = minMatch (AlignArgs.c:113)                        */
    int32_t minExtLength;   /* derived (AlignArgs.c:141-149); 5 at defaults                    */
    int32_t GOCost, GECost, RCost, MScore, XCutoff;
    float   minIdentity;    /* -P, kept as float on purpose (Math.h:292, AlignHelpers.c:359)   */
} ygpu_params;

/* Borrowed, read-only view of the loaded .nib2 bases and index (Query.c:565-626). */
typedef struct ygpu_index_view {
    const uint8_t  *bases;        /* AAs->basePtr: 4-bit codes, two per byte, high nibble first */
    uint64_t        n_base_bytes;
    uint32_t        maxROff;      /* AAs->maxROff (BaseSeq.c:121-125)                           */
    const uint32_t *startingOffs; /* 4^wordLen + 1 entries                                      */
    const uint32_t *ROA;          /* totalMatches entries                                       */
    uint32_t        totalMatches;
    int32_t         wordLen;
} ygpu_index_view;

/* A batch of reads: forward-strand 4-bit codes, one per byte (QS->forwardCodeBuf, Query.c:161-163);
 * read i occupies codes[offsets[i] .. offsets[i+1]).  The reverse complement (Query.c:164-167) is derived
 * on the device. */
typedef struct ygpu_read_batch {
    uint32_t        n_reads;
    const uint8_t  *codes;
    const uint64_t *offsets;      /* n_reads + 1 */
} ygpu_read_batch;

/* Edit operations are packed (len | opcode << 16), opcode one of 'M','R','I','D' (Math.h:353-360). */
#define YGPU_OP_LEN(x)  ((uint32_t)(x) & 0xFFFFu)
#define YGPU_OP_CODE(x) ((char)(((uint32_t)(x) >> 16) & 0xFFu))
#define YGPU_OP_MAKE(code, len) (((uint32_t)(uint8_t)(code) << 16) | ((uint32_t)(len) & 0xFFFFu))

/* One scored clump = the single SFragment + EditOpList + Clump_t fields (Math.h:448-456,512-527).
 * Offsets are strand-local exactly as in the reference (FragsClumps.inl:355-365 converts later). */
typedef struct ygpu_clump {
    uint32_t sro;          /* frag.startRefOff                       */
    uint16_t sqo, eqo;     /* frag.startQueryOff / endQueryOff       */
    uint16_t refLen;       /* frag.refLen (SUINT)                    */
    uint16_t totScore;     /* Clump_t::totScore (QOFF!)              */
    uint16_t totLength, matchedBases, mismatchedBases, gapBases;
    uint8_t  status;       /* clumpReversed 0x01 | Aligned 0x04 | Scored 0x08 | Split 0x10 */
    uint8_t  reserved;
    uint32_t op_start;     /* first op of this clump in ygpu_result_batch::ops */
    uint32_t n_ops;
} ygpu_clump;

/* Work counters (per batch) used for the algorithmic-bytes figure of SURVEY.md 8(d). */
typedef struct ygpu_counters {
    uint64_t kmer_lookups, hits, fragments, regions, clumps_formed, clumps_scored;
    uint64_t dp_ext_calls, dp_ext_rows, dp_ext_cells;
    uint64_t dp_gap_calls, dp_gap_rows, dp_gap_cells;
    uint64_t perfect_ext_bases, ref_bases_touched, ops_out, splits;
} ygpu_counters;

typedef struct ygpu_result_batch {
    uint32_t          n_reads;
    const uint32_t   *clump_start;   /* n_reads + 1; clumps of read i = [clump_start[i], clump_start[i+1]) in
                                        QS->clumps head->tail order after postProcessClumps */
    const ygpu_clump *clumps;
    const uint32_t   *ops;
    uint64_t          n_clumps, n_ops;
    ygpu_counters     counters;
} ygpu_result_batch;

typedef struct ygpu_ctx ygpu_ctx;

/* HIP devices visible to the process (0 when there is none or no runtime): what `-gpus N` may ask for. */
int  ygpu_device_count(void);
/* Create a context on HIP device `device`: copies the index view into HBM (replicated per GPU; reads shard
 * across GPUs, no collective).  Replaces the per-thread makeQueryState/initializeQueries (QueryState.c:36-104). */
int  ygpu_init(int device, const ygpu_index_view *index, const ygpu_params *params, ygpu_ctx **out);
/* The same for n devices at once, ctx_per_device contexts each -- the reference maps its index ONCE for all its threads (Query.c:565-626, 642-690); here every
 * device needs the image in its own HBM, and it crosses the host's memory and PCIe only once: devices[0] takes it from the host in pieces, every further device
 * takes each piece from the device before it as soon as that one has it (hipMemcpyPeerAsync over xGMI, a chain pipelined by piece).  A device that cannot reach
 * its neighbour (hipDeviceCanAccessPeer) uploads from the host itself.  The contexts of a device share its image (as ygpu_clone's do); their streams and events
 * are made while the image travels.  out[k * ctx_per_device + j] = context j of devices[k]; all are filled (also on failure, for ygpu_last_error; destroy them
 * all, a device's first context last); rc_each[0..n), when given, receives every device's own result code, the return value is the first that is not 0.  The
 * same device may be listed twice (two images on one device: what the 1-GPU tests use to drive the chain). */
int  ygpu_init_multi(const int *devices, int n, int ctx_per_device, const ygpu_index_view *index, const ygpu_params *params, ygpu_ctx **out, int *rc_each);
/* A further context on the same device sharing the parent's index image (no second upload; the parent must outlive it).  Two
 * contexts per GPU, one host thread and one stream of batches each, overlap one context's latency-bound stages and host work
 * with the other's compute -- the counterpart of running the reference with more threads than one per core is not needed:
 * there is no shared mutable state between contexts (as between the reference's per-thread QueryStates, Query.c:642-684). */
int  ygpu_clone(const ygpu_ctx *parent, ygpu_ctx **out);
void ygpu_destroy(ygpu_ctx *ctx);
const char *ygpu_last_error(const ygpu_ctx *ctx);
/* Device memory as the context sees it: free and total bytes of its device, and the bytes its own buffers hold (arenas grow with the first batches; the
 * reference's per-thread QueryState grows the same way, Query.c:81-100, 313).  A batching host uses it to decide how many contexts a device can carry. */
int  ygpu_memory(ygpu_ctx *ctx, uint64_t *free_bytes, uint64_t *total_bytes, uint64_t *ctx_bytes);
/* A context the batching host leaves out (its device has no room for another set of arenas): releases the context's own buffers and takes it out of the count of
 * contexts that share the device's memory budget, so that the contexts that do run are not held to a share sized for it.  The reference has no counterpart -- a
 * thread of Query.c:642-690 that cannot allocate its QueryState is fatal (FragsClumps.c:74).  The context can only be destroyed afterwards. */
int  ygpu_park(ygpu_ctx *ctx);
/* The capacities of a context's arenas and the estimates it carries from batch to batch (trace rows per bound row, clump slots ...), as they stand after a batch;
 * ygpu_presize gives another context of the same build the same capacities in one go and seeds its estimates, so that its first batch runs like any later one
 * instead of growing a hundred buffers one by one (each growth frees a buffer, and a free waits for every kernel on the device: first batches used to run one
 * at a time with the device's other contexts held back).  The reference's per-thread QueryState grows lazily as well (Query.c:81-100, 313); its threads do not
 * share an allocator that stalls the others. */
typedef struct ygpu_arena_profile {
    uint32_t n; uint32_t last_clump_slots; uint64_t cap[224]; double trace_ratio, ops_ratio; int64_t last_fall; uint64_t bases;
} ygpu_arena_profile;
int  ygpu_get_arena_profile(ygpu_ctx *ctx, ygpu_arena_profile *out);
int  ygpu_presize(ygpu_ctx *ctx, const ygpu_arena_profile *profile);

/* Stage reads into HBM (H2D).  Separate from ygpu_run so that a benchmark can time the hot path with inputs
 * already resident. */
int  ygpu_upload(ygpu_ctx *ctx, const ygpu_read_batch *batch);
/* The same without the wait at its end: returns once the copies are queued (the reads' bytes may still be on their way).  The batch's memory must stay
 * unchanged until the ygpu_run that follows has returned.  (The command line's context threads: their batches live until they are printed.) */
int  ygpu_upload_nowait(ygpu_ctx *ctx, const ygpu_read_batch *batch);
/* Run the whole hot path (A1..A10) on the resident batch; results stay in HBM. */
int  ygpu_run(ygpu_ctx *ctx);
/* Copy results of the last ygpu_run to host memory owned by the context. */
int  ygpu_collect(ygpu_ctx *ctx, ygpu_result_batch *out);
/* The same into memory of the caller's: ygpu_result_size gives the element counts of the last ygpu_run; ygpu_collect_into copies clump_start[n_reads + 1],
 * clumps[n_clumps] and ops[n_ops] there and points `out` at them.  With buffers from ygpu_host_alloc (page-locked host memory) the copy is a DMA straight
 * into them -- no staging copy by the calling thread, none afterwards to get the results out of the context: a batching host keeps a result buffer per batch
 * in flight and hands it to its formatter threads while the context already runs the next batch (the reference's QueryState owns its clump list the same
 * way, QueryState.c:156-161).  Any memory works; pageable memory is staged by the runtime. */
int  ygpu_result_size(ygpu_ctx *ctx, uint64_t *n_clumps, uint64_t *n_ops);
int  ygpu_collect_into(ygpu_ctx *ctx, uint32_t *clump_start, ygpu_clump *clumps, uint32_t *ops, ygpu_result_batch *out);
void *ygpu_host_alloc(size_t bytes);           /* NULL when no device runtime is there or the memory cannot be locked */
void  ygpu_host_free(void *p);
/* ---- post-filter on the device (optional stage behind ygpu_run) ------------------------------------------------------------------------------------------
 * The reference's loop goes on, after the hot path, with postFilterBySimilarity (Query.c:450, GraphPath.cpp:897-1086: Optimal Query Coverage, filter by
 * similarity, mapping quality) and prints what is left -- for a 1 kbp read one or two of the ~75 clumps the hot path returns.  ygpu_postfilter runs that step
 * for the whole batch on the device (same routine as the host's, yaha_amd/csrc/oqc_core.h) and ygpu_collect_filtered returns, per read and in PRINT order,
 * only the clumps printClumps would see (QS->clumps after the filter) with the fields the filter sets (Math.h Clump_t: status, mapQuality, numSecondaries,
 * matchedPrimary; QS->primaryCount), and only their edit ops.  Bit-identical to filtering ygpu_collect's output on the host; -OQC N runs keep the host filter.
 * A read with more clumps than the device stage takes (1 792: what its sort holds in a workgroup's 64 KB of LDS) comes back UNFILTERED -- all its clumps in
 * ygpu_collect's order, primaryCount == 0xFFFF in each -- for the caller to filter (yaha_session_emit_filtered does).
 * The stage works on a SNAPSHOT of the batch's results, so a context can run its next batch while another thread filters this one (the reference's threads
 * each finish a read before they take the next, Query.c:430-470; here the two halves of a batch's life overlap):
 *   context's thread:  ygpu_upload, ygpu_run, ygpu_postfilter_snapshot  -> hand the batch to the filter thread -> ygpu_upload, ygpu_run of the next batch ...
 *   filter thread:     ygpu_postfilter, ygpu_filtered_size, ygpu_collect_filtered
 * One snapshot at a time: the next ygpu_postfilter_snapshot may be called once the filtered results of the previous one have been collected.  ygpu_postfilter
 * without a snapshot takes one itself (the sequential use: ygpu_run, ygpu_postfilter, ygpu_collect_filtered on one thread).  The filtered results are handed out
 * ONCE: after ygpu_collect_filtered, ygpu_filtered_size answers YGPU_EINVAL until the next ygpu_postfilter (it used to answer with the previous batch).  A snapshot
 * that will not be filtered after all (an error between the two calls) is dropped with ygpu_postfilter_drop -- otherwise the next ygpu_postfilter would filter IT. */
typedef struct ygpu_postfilter_params {
    int32_t  minNonOverlap, BPCost, maxBPLog, FBS;     /* AlignArgs: OQCMinNonOverlap, BPCost, maxBPLog, FBS (0/1) */
    float    FBS_PSLength, FBS_PSScore;
    int32_t  bppVmin, bppN;                            /* break point penalty (int)(min(log10(d), maxBPLog) * BPCost + 0.5) as a step function of the distance d > 10: */
    const uint32_t *bppThr;                            /*   bppVmin + number of thresholds <= d; bppN thresholds, ascending (host memory; copied) */
    uint32_t n_seqs; const uint32_t *seq_start, *seq_length;   /* reference sequences in bases, ascending (findBaseSequenceNum, BaseSeq.c:81-90; host memory; copied) */
} ygpu_postfilter_params;
typedef struct ygpu_out_clump {                        /* 40 bytes */
    ygpu_clump c;                                      /* op_start indexes the filtered batch's ops */
    uint8_t  status, mapQuality; uint16_t numSecondaries, matchedPrimary, primaryCount;
} ygpu_out_clump;
typedef struct ygpu_filtered_batch {
    uint32_t              n_reads;
    const uint32_t       *clump_start;   /* n_reads + 1 */
    const ygpu_out_clump *clumps;
    const uint32_t       *ops;
    uint64_t              n_clumps, n_ops;
    ygpu_counters         counters;
} ygpu_filtered_batch;
int  ygpu_set_postfilter(ygpu_ctx *ctx, const ygpu_postfilter_params *p);     /* once per context */
int  ygpu_postfilter_snapshot(ygpu_ctx *ctx);                                  /* after ygpu_run, on the context's thread */
int  ygpu_postfilter(ygpu_ctx *ctx);                                           /* after ygpu_run or ygpu_postfilter_snapshot */
int  ygpu_postfilter_drop(ygpu_ctx *ctx);                                      /* forget an unfiltered snapshot and uncollected results */
int  ygpu_filtered_size(ygpu_ctx *ctx, uint64_t *n_clumps, uint64_t *n_ops);
int  ygpu_collect_filtered(ygpu_ctx *ctx, uint32_t *clump_start, ygpu_out_clump *clumps, uint32_t *ops, ygpu_filtered_batch *out);

/* ---- read depth along the reference (optional, behind ygpu_postfilter) ------------------------------------------------------------------------------------
 * Structural-variant callers combine split reads -- the SAM -- with read depth.  After the post-filter the clumps that will be printed, their edit ops and the
 * sequence table are all on the device, so depth is accumulated there: with ygpu_depth_enable, every ygpu_postfilter of the context also adds the clumps it
 * returns to a binned coverage array (uint32 per bin; the reference has no counterpart, its users run a second tool over the sorted SAM).
 * The contract (yaha_amd/csrc/depth_core.h -- one routine for host and device): every sequence is cut into bins of `bin` bases, never across two sequences, the
 * last bin of a sequence may be shorter, bins are numbered sequence by sequence in index order: n_bins = sum of ceil(length / bin).  cov[b] = number of
 * (record, reference base) pairs in bin b over the records yaha_session_emit_filtered prints: the bases under M and R ops (the M of the printed CIGAR), not those
 * under D; a clump that spans two sequences is not printed and covers nothing; records with mapQuality < min_mapq cover nothing.  A bin that passes 2^32 - 1
 * wraps (not handled).  Reads that come back UNFILTERED (more than 1 792 clumps, primaryCount == 0xFFFF) are NOT counted: the caller filters them and counts
 * what it prints.
 * ONE array per index image, 4 * n_bins bytes of device memory: the contexts that share an image (ygpu_clone, ctx_per_device of ygpu_init_multi) add into the
 * same array (global atomics) once each of them has called ygpu_depth_enable with the same parameters -- the first call makes and zeroes it, the others join.
 * When it does not fit: YGPU_ENOMEM, the sizes in ygpu_last_error (bin 1 on a 3.1 Gbp genome is 12.4 GB).  It lives until the last of those contexts is destroyed;
 * ygpu_park of one of them does not touch it.  Order: ygpu_set_postfilter, ygpu_depth_enable, then batches (ygpu_run, ygpu_postfilter ...), ygpu_depth_collect. */
typedef struct ygpu_depth_params {
    uint32_t bin, min_mapq, n_seqs;
    const uint32_t *seq_start, *seq_length;            /* reference sequences in bases, ascending (host memory; copied) */
} ygpu_depth_params;
int  ygpu_depth_enable(ygpu_ctx *ctx, const ygpu_depth_params *p);             /* after ygpu_set_postfilter */
int  ygpu_depth_size(ygpu_ctx *ctx, uint64_t *n_bins);
/* The image's array as it stands, into bins[n_bins] (may be NULL): waits for every filter stage queued so far on the device, its sibling contexts' included.
 * stats (may be NULL): records counted, records skipped (MAPQ), records dropped (two sequences), reads left to the caller (handed back unfiltered). */
int  ygpu_depth_collect(ygpu_ctx *ctx, uint32_t *bins, uint64_t stats[4]);

/* ---- the evidence track: mismatches, indels and clipped ends along the reference (optional, behind ygpu_postfilter) -------------------------------------------
 * The third signal of a structural-variant caller beside the split alignments and read depth: where the printed alignments disagree with the reference or stop.
 * With ygpu_events_enable, every ygpu_postfilter of the context also adds the clumps it returns to ev[bin][channel] (uint32, bin-major, five channels), on the
 * bin layout of the depth track above, so that a caller can divide by depth.  The contract (yaha_amd/csrc/events_core.h -- one routine for host and device):
 * channel 0 mismatch: 1 per reference base under an R op; 1 deleted: 1 per reference base under a D op; 2 insertion: 1 per I op, whatever its length, in the bin
 * of the next reference base the walk reaches (kept inside the record); 3 clip_left: 1 in the bin of the record's first reference base when the printed CIGAR
 * starts with a clip of at least min_clip bases; 4 clip_right: 1 in the bin of its last reference base when it ends with one.  Hard and soft clips count alike.
 * As for depth: a clump that spans two sequences is not printed and adds nothing, records with mapQuality < min_mapq add nothing, a count that passes 2^32 - 1
 * wraps, and reads that come back UNFILTERED (primaryCount == 0xFFFF) are NOT counted: the caller filters them and counts what it prints.
 * ONE array per index image, 20 * n_bins bytes of device memory (bin 1 on a 3.1 Gbp genome is 62 GB), shared by the image's contexts once each of them has
 * called ygpu_events_enable with the same parameters -- the first call makes and zeroes it, the others join; other parameters are refused.  When it does not
 * fit: YGPU_ENOMEM, the sizes in ygpu_last_error.  It lives until the last of those contexts is destroyed; ygpu_park does not touch it.  It does not need the
 * depth track.  Order: ygpu_set_postfilter, ygpu_events_enable, then batches (ygpu_run, ygpu_postfilter ...), ygpu_events_collect. */
#define YGPU_EVENTS_CHANNELS 5
typedef struct ygpu_events_params {
    uint32_t bin, min_mapq, min_clip, n_seqs;
    const uint32_t *seq_start, *seq_length;            /* reference sequences in bases, ascending (host memory; copied) */
} ygpu_events_params;
int  ygpu_events_enable(ygpu_ctx *ctx, const ygpu_events_params *p);           /* after ygpu_set_postfilter */
int  ygpu_events_size(ygpu_ctx *ctx, uint64_t *n_bins);
/* The image's array as it stands, into counts[n_bins * 5], bin-major (may be NULL): waits for every filter stage queued so far on the device, its sibling
 * contexts' included.  stats (may be NULL): records counted, records skipped (MAPQ), records dropped (two sequences), reads left to the caller. */
int  ygpu_events_collect(ygpu_ctx *ctx, uint32_t *counts, uint64_t stats[4]);

/* ---- the allele pileup: which base the printed alignments carry at every reference base (optional, behind ygpu_postfilter) ------------------------------------
 * The allele-resolved member of the family: the tracks above say that a bin holds mismatches, this one says which base the reads carry there and how many of
 * them agree.  With ygpu_pileup_enable, every ygpu_postfilter of the context also adds the clumps it returns to pu[slot][channel] (uint32, slot-major, seven
 * channels A C G T N DEL INS) on the bin layout of the depth track with a bin of ONE base: a slot per reference base, sequence by sequence.  The contract
 * (yaha_amd/csrc/pileup_core.h -- one set of routines for host and device): every reference base under an M or R op adds 1 to the channel of the read's base
 * there (the reverse-complement base for a reversed clump, i.e. what SEQ shows: reference orientation; codes other than A C G T: N), every reference base under a
 * D op adds 1 to DEL, every I op adds 1 to INS at the next reference base the walk reaches (kept inside the record); a base whose query offset lies past the
 * clump's eqo adds nothing, whatever the ops add up to.  Base qualities are not used.  As for depth: a clump that spans two sequences is not printed and adds
 * nothing, records with mapQuality < min_mapq add nothing, a count that passes 2^32 - 1 wraps, and reads that come back UNFILTERED (primaryCount == 0xFFFF) are
 * NOT counted: the caller filters them and counts what it prints.  While the pileup is enabled ygpu_postfilter_snapshot also copies the batch's forward codes
 * and read offsets (device to device, into buffers of the snapshot's own): the stage reads the bases when the context may already hold its next batch.
 * ONE array per index image, 28 * n_slots bytes of device memory (a 3.1 Gbp genome is 86.8 GB), shared by the image's contexts once each of them has called
 * ygpu_pileup_enable with the same parameters -- the first call makes and zeroes it, the others join; other parameters are refused.  When it does not fit:
 * YGPU_ENOMEM, the sizes in ygpu_last_error.  It lives until the last of those contexts is destroyed; ygpu_park does not touch it.
 * An array of that size does not travel: a SITE is a slot with nonref = A + C + G + T + N + DEL - pu[slot][channel of the reference's own base] + INS >= some
 * threshold >= 1, and the device selects the CANDIDATES -- the slots with nonref >= 1, ascending -- itself (ygpu_pileup_candidates_size runs the selection over
 * the array as it stands, ygpu_pileup_candidates_collect copies the slot numbers); ygpu_pileup_gather returns the seven counts of every slot of a caller's
 * list.  With several images: candidates of each, the sorted union, a gather on each, the sums, the threshold -- nothing is lost, since a slot whose summed
 * nonref is at least 1 has nonref >= 1 in some image.  These three calls wait for everything queued on the device and use the post-filter's side of the
 * context: call them between batches or at the end of the run, not while a ygpu_postfilter of the context is running.  They, and ygpu_pileup_collect, also
 * work on a context that has been parked (ygpu_park): the array is the image's, and the few work buffers they need are made again.
 * This is the first track whose kernel reads the SNAPSHOT after the stage's last wait of the host (the forward codes, for the bases): ygpu_postfilter returns
 * with that kernel still queued, so the rule of ygpu_postfilter_snapshot holds in earnest here -- the next snapshot of the context may be taken only once the
 * filtered results of this one have been collected (ygpu_collect_filtered waits behind the kernel), not as soon as ygpu_postfilter has returned.
 * Order: ygpu_set_postfilter, ygpu_pileup_enable, then batches (ygpu_run, ygpu_postfilter ...), then the candidates and gathers (or ygpu_pileup_collect). */
#define YGPU_PILEUP_CHANNELS 7
typedef struct ygpu_pileup_params {
    uint32_t min_mapq, n_seqs;
    const uint32_t *seq_start, *seq_length;            /* reference sequences in bases, ascending (host memory; copied) */
} ygpu_pileup_params;
int  ygpu_pileup_enable(ygpu_ctx *ctx, const ygpu_pileup_params *p);           /* after ygpu_set_postfilter */
int  ygpu_pileup_size(ygpu_ctx *ctx, uint64_t *n_slots);
/* The image's whole array as it stands, into counts[n_slots * 7], slot-major (may be NULL) -- for tests and small genomes: waits for every filter stage queued so
 * far on the device.  stats (may be NULL): records counted, records skipped (MAPQ), records dropped (two sequences), reads left to the caller, counts added
 * (the sum over the array while nothing has wrapped). */
int  ygpu_pileup_collect(ygpu_ctx *ctx, uint32_t *counts, uint64_t stats[5]);
int  ygpu_pileup_candidates_size(ygpu_ctx *ctx, uint64_t *n);                  /* selects; *n = candidates of the array as it stands */
int  ygpu_pileup_candidates_collect(ygpu_ctx *ctx, uint32_t *slots);           /* slots[n] of the last ygpu_pileup_candidates_size, ascending */
/* rows[n * 7]: the seven counts of slots[0 .. n) (host memory; ascending for locality, not checked; a slot past the array reads as zeros). */
int  ygpu_pileup_gather(ygpu_ctx *ctx, const uint32_t *slots, uint64_t n, uint32_t *rows);

/* ---- SNV calls with genotypes from the pileup array (optional; needs ygpu_pileup_enable) -----------------------------------------------------------------------
 * The step behind the pileup: which allele the reads carry at a slot, how sure that is, and whether the sample is heterozygous there -- judged on the device,
 * one selection pass over the image's array, so that only the calls cross PCIe.  The contract (yaha_amd/csrc/snv_core.h -- one set of routines for host and
 * device): r = the count of the reference's own base, a = the greatest count among the other three of A C G T (ties to the lowest channel), D = A + C + G + T,
 * other = N + DEL; PL0 = r cost_match + a cost_error, PL1 = (r + a) cost_het, PL2 = r cost_error + a cost_match in 1/100 phred, GT the smallest (ties to the
 * lower index), QUAL = min(PL0 - least, 999 900) / 100, GQ = min(second smallest - least, 9 900) / 100; a slot is a call when GT != 0, a >= min_alt,
 * D >= min_depth and QUAL >= min_qual.  A slot whose reference base is not one of A C G T is never a call.  The three costs come from the caller: the device
 * takes no logarithm (yaha_session_snv_params derives them from -snverr; 46, 1477 and 331 at the default of 100 per mille).
 * One call needs the SUM of all sources before it is judged -- the counts the caller made itself (reads handed back unfiltered, runs filtered on the host), the
 * other index images of a run over several devices.  ygpu_pileup_add folds such a source into ONE image's array: rows[i * 7 + channel] is added to slot
 * slots[i] with global atomics; a slot at or past n_slots adds nothing; slots need not be distinct or ordered.  An array folded into is no longer the image's
 * own counts: nothing may read it as such afterwards.
 * ygpu_snv_call_size runs the selection over the array as it stands (a wave per tile of 2 048 slots, the tiles' counts through the exclusive sum, the records
 * written by ballot and population count in ascending slot order, no atomics) and returns the number of calls; ygpu_snv_collect copies the records of the last
 * selection.  A second ygpu_snv_call_size, with other parameters, selects again over the same array.  Like the candidates, these calls wait for everything
 * queued on the device, use the post-filter's side of the context and serve a parked context. */
typedef struct ygpu_snv_params {
    uint32_t cost_match, cost_error, cost_het;          /* 1/100 phred: a read that shows the genotype's base / another base / one of a heterozygote's two */
    uint32_t min_alt, min_depth, min_qual;              /* at least 1, at least 1, whole phred */
    uint32_t reserved[2];                               /* zero */
} ygpu_snv_params;
/* 48 bytes.  info = channel of the reference's base | channel of alt << 4 | GT << 8 | the reference's 4-bit code << 12 (channels: A0 C1 G2 T3); depth and
 * other saturate at 2^32 - 1; pl[3]: the three normalised likelihoods in 1/100 phred, each saturated at 2^32 - 1 */
typedef struct ygpu_snv_call {
    uint32_t slot, info, ref_count, alt_count, depth, other, qual, gq;
    uint32_t pl[3], zero;
} ygpu_snv_call;
int  ygpu_pileup_add(ygpu_ctx *ctx, const uint32_t *slots, const uint32_t *rows, uint64_t n);      /* after ygpu_pileup_enable */
int  ygpu_snv_call_size(ygpu_ctx *ctx, const ygpu_snv_params *p, uint64_t *n);                     /* selects; *n = calls of the array as it stands */
int  ygpu_snv_collect(ygpu_ctx *ctx, ygpu_snv_call *calls);                                        /* calls[n] of the last ygpu_snv_call_size, ascending */

/* ---- indel alleles: which insertions and deletions the printed alignments carry (optional, behind ygpu_postfilter) -----------------------------------------------
 * What the pileup's INS and DEL channels leave out: how long an indel is and what was inserted.  With ygpu_indels_enable, every ygpu_postfilter of the context
 * also counts the indel ALLELES of the clumps it returns in a hash table on the device.  The contract (yaha_amd/csrc/indel_core.h -- one set of routines for
 * host and device): slots, gates and the two-sequence drop are the pileup's; a D op of at least min_length bases is the allele (slot of its first base, DEL,
 * length), an I op of at least min_length bases the allele (slot of the next reference base the walk reaches, kept inside the record; INS; length; the first
 * min(length, 42) inserted bases as channels A0 C1 G2 T3 N4 in reference orientation); an insertion whose bases would lie past the clump's eqo, or a deletion
 * past its last reference base, is no event; two insertions of more than 42 bases that agree in slot, length and first 42 bases are one allele; a record adds 1
 * per event.  The key: w0 = slot | type << 32 | length << 33 | 1 << 63, w1 / w2 = 21 bases each at 3 bits, the first lowest, bit 63 set (a deletion: that bit alone).
 * Reads that come back UNFILTERED (primaryCount == 0xFFFF) are NOT counted: the caller filters them and counts what it prints.
 * The table is the CONTEXT's own (as the junctions' buffers are, unlike the binned arrays): open addressing, linear probing, `capacity` entries of 32 bytes, a
 * power of two.  capacity == 0 asks for the rule: the smallest power of two >= 2 x the context's batch capacity in bases -- the bases of the largest batch it
 * has held, at least 2^20; made at enable and made larger before a larger batch is counted while it is EMPTY (a batch has at most one event per two bases: a
 * caller that collects whenever ygpu_indels_size says more than capacity / 4 keeps the load at or below one half).  A capacity that is no power of two is
 * refused.  An event that finds no entry within the probe limit is counted as LOST and ygpu_postfilter answers YGPU_EOVERFLOW, naming -oid in
 * ygpu_last_error: the filtered batch is lost, the table holds a part of it; after ygpu_indels_collect the context serves its next batch.
 * While the stage is enabled ygpu_postfilter_snapshot also copies the batch's forward codes and read offsets (as for the pileup), and ygpu_postfilter ends with
 * one more small wait (the used and lost words).  ygpu_indels_size: entries in use after the context's last ygpu_postfilter.  ygpu_indels_collect: the occupied
 * entries compacted on the device in ascending table index (count a tile, exclusive sums, emit by ballot), copied to out[ygpu_indels_size] (may be NULL when
 * that is 0), then the table, the statistics and both words are CLEARED: every entry is returned once.  stats (may be NULL), since the previous collect:
 * records counted, records skipped (MAPQ), records dropped (two sequences), events, reads left to the caller, events lost.  Both calls use the post-filter's
 * side of the context: between batches, not while a ygpu_postfilter of the context is running.  A parked context (ygpu_park) has given its table up: 0 entries.
 * Order: ygpu_set_postfilter, ygpu_indels_enable, then batches (ygpu_run, ygpu_postfilter, now and then ygpu_indels_collect), a last ygpu_indels_collect. */
#define YGPU_INDEL_KEPT_BASES 42
typedef struct ygpu_indel_params {
    uint32_t min_mapq, min_length, n_seqs, reserved;
    const uint32_t *seq_start, *seq_length;            /* reference sequences in bases, ascending (host memory; copied) */
    uint64_t capacity;                                 /* entries, a power of two; 0: the rule above */
} ygpu_indel_params;
typedef struct ygpu_indel_entry { uint64_t w0, w1, w2; uint32_t count, zero; } ygpu_indel_entry;      /* 32 bytes */
int  ygpu_indels_enable(ygpu_ctx *ctx, const ygpu_indel_params *p);            /* after ygpu_set_postfilter */
int  ygpu_indels_size(ygpu_ctx *ctx, uint64_t *used);
int  ygpu_indels_collect(ygpu_ctx *ctx, ygpu_indel_entry *out, uint64_t stats[6]);

/* ---- indel calls with genotypes: the raw alleles left-normalised, merged and judged at their anchor base (optional; needs ygpu_pileup_enable) -----------------
 * The step behind the indel alleles and the pileup: a raw allele sits where the aligner happened to put the gap, so one indel of a homopolymer or tandem repeat
 * can be spread over several keys.  The contract (yaha_amd/csrc/indelcall_core.h -- one set of routines for host and device): p = the key's slot, the anchor is
 * p - 1; an insertion of more than 42 bases and an allele at the first slot of its sequence are `skipped` (so are keys that are no event of the layout: a slot
 * past it, length 0, a deletion past the end of its sequence); the shift s is the first i < min(max_shift, p - 1 - first slot of the sequence) at which
 * ref[p-1-i] differs from ref[p+L-1-i] (deletion) or from I[L-1-(i mod L)] (insertion), or either is not one of A C G T; the normalised allele has slot p - s
 * and, an insertion, its bases rotated right by s mod L; equal normalised keys are ONE allele whose counts add, saturated at 2^32 - 1.  An allele is judged with
 * d = A + C + G + T + N + DEL of the pileup row at its anchor, a = its count, r = max(d - a, 0): PL0 = r cost_match + a cost_error, PL1 = (r + a) cost_het,
 * PL2 = r cost_error + a cost_match, GT / QUAL / GQ as for the SNV calls; a call needs GT != 0, a >= min_alt, d >= min_depth, QUAL >= min_qual.
 * ygpu_indelcall_normalize takes the run's raw alleles (host memory; counted with min_length 1 and the pileup's gate), normalises them on the device -- a wave per
 * allele reads the image's reference 64 bases a step, the first mismatch comes from one ballot -- and merges them in a table of the context's own (compare-and-
 * swap on the key's words, a 64-bit atomic add of the count: sums of integers, the same whatever order the atomics are served in).  *n_out = merged alleles;
 * stats (may be NULL) = raw alleles, alleles that moved, alleles merged away, alleles skipped.  The layout is the pileup's: ygpu_pileup_enable first.
 * ygpu_indelcall_alleles copies the merged alleles of the last normalize, ygpu_indelcall_size judges every one of them against the image's pileup array AS IT
 * STANDS (fold the other sources with ygpu_pileup_add first) and returns the number of calls, ygpu_indelcall_collect copies the records of the last selection.
 * Both lists leave in the order of indel_core.h's keyLess: the table keeps no order, so the records selected on the device -- the calls alone -- are put into it
 * by the host side of the call.  A second ygpu_indelcall_size, with other parameters, selects again.  Like the SNV calls these wait for everything queued on the
 * device, use the post-filter's side of the context and serve a parked context. */
typedef struct ygpu_indelcall_params {
    uint32_t cost_match, cost_error, cost_het;          /* 1/100 phred: a read that agrees with the genotype / disagrees / one of a heterozygote's two */
    uint32_t min_alt, min_depth, min_qual;              /* reads that carry the allele, reads that cover the anchor, whole phred */
    uint32_t reserved[2];                               /* zero */
} ygpu_indelcall_params;
/* 64 bytes.  w0 .. w2: the normalised key (indel_core.h); info = GT | the 4-bit reference code of the anchor << 4; counts and PLs saturate at 2^32 - 1 */
typedef struct ygpu_indel_call {
    uint64_t w0, w1, w2;
    uint32_t alt_count, ref_count, depth, qual, gq, pl[3], info, zero;
} ygpu_indel_call;
int  ygpu_indelcall_normalize(ygpu_ctx *ctx, const ygpu_indel_entry *raw, uint64_t n, uint32_t max_shift, uint64_t *n_out, uint64_t stats[4]);
int  ygpu_indelcall_alleles(ygpu_ctx *ctx, ygpu_indel_entry *out);                                  /* out[n_out] of the last normalize, keyLess order */
int  ygpu_indelcall_size(ygpu_ctx *ctx, const ygpu_indelcall_params *p, uint64_t *n);              /* selects; *n = calls over the array as it stands */
int  ygpu_indelcall_collect(ygpu_ctx *ctx, ygpu_indel_call *calls);                                 /* calls[n] of the last ygpu_indelcall_size, keyLess order */

/* ---- the error profile: how good the printed alignments are (optional, behind ygpu_postfilter) -----------------------------------------------------------------
 * What the other outputs leave out: the substitution spectrum, the lengths of insertions and deletions, the identity the records reach and the error rate
 * along the read.  With ygpu_eprofile_enable, every ygpu_postfilter of the context also adds the clumps it returns to ONE table of YGPU_EPROFILE_WORDS = 1556
 * uint64 words on the device.  The contract (yaha_amd/csrc/eprofile_core.h -- one set of routines for host and device): gates, the two-sequence drop and the
 * walk are the pileup's; a PAIR is a reference base under an M or R op with the read base over it, both as channels A C G T N (the reference's from the packed
 * image, past the image N), a MATCH a pair of equal channels that are not N.  The words, in this order:
 *   SUB    25         [ref channel][read channel], 1 per pair
 *   INS    65         1 per I op of n >= 1 bases at index min(n, 65) - 1
 *   DEL    65         the same per D op
 *   IDENT  1001       1 per record with cols > 0 at floor(1000 * matches / cols), cols = pairs + inserted + deleted bases
 *   POS    100 x 4    by the pair's place in the read as sequenced, bin = forward offset * 100 / read length: pairs, pairs that are no match, I ops, D ops
 * The reads the stage hands back unfiltered (primaryCount 0xFFFF) are NOT counted: the caller filters them and counts what it prints.  While the stage is
 * enabled ygpu_postfilter_snapshot also copies the batch's forward codes and read offsets (as for the pileup).
 * The table is the CONTEXT's own (a caller with several contexts adds their tables up): the kernel keeps it in LDS for a workgroup's whole share of a batch
 * and reaches memory once per workgroup.  ygpu_eprofile_size: the number of words, YGPU_EPROFILE_WORDS.  ygpu_eprofile_collect: the table as it stands --
 * nothing is cleared -- after waiting for the filter stages queued on the context so far; words and stats may each be NULL.  stats: records counted, records
 * skipped (MAPQ), records dropped (two sequences), reads left to the caller.  A parked context (ygpu_park) has given its table up: all zero.
 * Order: ygpu_set_postfilter, ygpu_eprofile_enable, then batches (ygpu_run, ygpu_postfilter ...), then ygpu_eprofile_collect. */
#define YGPU_EPROFILE_WORDS 1556
typedef struct ygpu_eprofile_params {
    uint32_t min_mapq, n_seqs;
    const uint32_t *seq_start, *seq_length;            /* reference sequences in bases, ascending (host memory; copied) */
} ygpu_eprofile_params;
int  ygpu_eprofile_enable(ygpu_ctx *ctx, const ygpu_eprofile_params *p);        /* after ygpu_set_postfilter */
int  ygpu_eprofile_size(ygpu_ctx *ctx, uint64_t *n_words);
int  ygpu_eprofile_collect(ygpu_ctx *ctx, uint64_t *words, uint64_t stats[4]);

/* ---- split-read breakpoint calls: where the printed alignments of a read join (optional, behind ygpu_postfilter) ----------------------------------------------
 * The primary signal of a structural-variant caller.  With ygpu_junctions_enable, every ygpu_postfilter of the context also makes the JUNCTIONS of its batch on
 * the device.  The contract (yaha_amd/csrc/junction_core.h -- one set of routines for host and device): the eligible records of a read are the printed ones (a
 * clump that spans two sequences is not) that are primary (status & 0x20) with mapQuality >= min_mapq; their read-forward query interval is (qs, qe) =
 * status & 1 ? (qlen - 1 - eqo, qlen - 1 - sqo) : (sqo, eqo); ordered by (qs, qe, print order), every consecutive pair (a, b) is one junction with side A =
 * (sequence of a, its last reference base -- its first when a is reversed --, '+' or '-' when reversed), side B = (sequence of b, its first reference base -- its
 * last when reversed --, strand) and qgap = qs_b - qe_a - 1 (negative: overlap on the read, positive: unaligned bases between the pieces).  Positions are 0-based
 * within their sequence.  Canonical form: when (seqB, posB) < (seqA, posA) the sides are swapped and both strands flipped (equal positions: no swap).  Type: TRA
 * when the sequences differ, else INV when the strands differ, else DEL for +/+ and DUP for -/-.
 * The junctions of a batch are ordered by (read, ordinal) -- always the same for the same batch -- live in a buffer of the context sized from the batch's filtered
 * clump count, and are handed out by ygpu_junctions_size / ygpu_junctions_collect, valid after ygpu_postfilter until the context's next ygpu_postfilter (any
 * number of times, before or after ygpu_collect_filtered).  Reads that come back UNFILTERED (primaryCount == 0xFFFF) get none: the caller filters them and makes
 * the junctions of what it prints.  Order: ygpu_set_postfilter, ygpu_junctions_enable, then batches.  The table of sequences is copied; a second call replaces
 * the parameters. */
enum { YGPU_JUNCTION_DEL = 0, YGPU_JUNCTION_DUP = 1, YGPU_JUNCTION_INV = 2, YGPU_JUNCTION_TRA = 3 };
typedef struct ygpu_junction {                         /* 32 bytes */
    uint32_t read;                                     /* index of the read in the batch                          */
    uint32_t ordinal;                                  /* 0 .. junctions of the read - 1, along the read          */
    uint32_t seqA, posA, seqB, posB;                   /* canonical: (seqA, posA) <= (seqB, posB)                 */
    uint8_t  strandA, strandB;                         /* '+' or '-'                                              */
    uint8_t  type, reserved;                           /* YGPU_JUNCTION_*; 0                                      */
    int32_t  qgap;
} ygpu_junction;
typedef struct ygpu_junction_params {
    uint32_t min_mapq, n_seqs;
    const uint32_t *seq_start, *seq_length;            /* reference sequences in bases, ascending (host memory; copied) */
} ygpu_junction_params;
int  ygpu_junctions_enable(ygpu_ctx *ctx, const ygpu_junction_params *p);      /* after ygpu_set_postfilter, else YGPU_EINVAL */
int  ygpu_junctions_size(ygpu_ctx *ctx, uint64_t *n);
/* out[n] (may be NULL).  stats (may be NULL): reads with junctions, junctions, records skipped by MAPQ, reads left to the caller (handed back unfiltered) --
 * of this batch. */
int  ygpu_junctions_collect(ygpu_ctx *ctx, ygpu_junction *out, uint64_t stats[4]);

/* Stage-level entry for tests of the post-filter (as ygpu_dp_batch is for the DP kernels): place a result batch on the device as if ygpu_run had produced it
 * for the reads uploaded last (r->n_reads must equal the uploaded batch's; clump_start / clumps / ops as ygpu_collect returns them).  ygpu_postfilter,
 * ygpu_collect and their siblings then work on it -- so that the device filter can be driven with clump lists no real read produces (hundreds of exact ties,
 * chains of overlaps) and compared with the host's on the same data. */
int  ygpu_inject_results(ygpu_ctx *ctx, const ygpu_result_batch *r);
/* Stage-level test entry for the exclusive sums and orderings the hot path lays its variable-size outputs out with (device/scan.h: single-pass look-back sums of
 * u32 / u64, orderings by a small key) and for the post-filter's sort on the wave (device/oqc_stage.h waveSort, against oqc_core.h sortRange): runs them on n
 * pseudo-random elements (the sort: on arrays of 2 .. 1 792 entries with ties) and compares with the plain host loops; and for A2's workgroup sort (device/wgsort.h: five
 * shapes, both rankings -- LDS atomics and ballots -- over segments of every fill whose diagonals are made to tie, against std::stable_sort; its own order check must
 * stay silent).  0, or YGPU_EINTERNAL with the first difference in ygpu_last_error.  (The reference needs none of them: it handles one read at a time and merges
 * sorted k-mer lists, Query.c:306-497, QueryMatch.c:52-121.) */
int  ygpu_selftest_primitives(ygpu_ctx *ctx, uint32_t n, uint32_t seed, int key_bits);
/* The trace stream of the last ygpu_run -- the largest HBM stream of the path, an implementation choice and not algorithmic traffic: the X-drop rows kernel writes
 * a record per DP row it computes, the traceback (SW.cpp:1138-1195) comes back for those of rows 0 .. maxi of the calls that end above zero (SW.cpp:1091-1111 returns
 * before any traceback otherwise).  out[0] = records written, out[1] = records a traceback can visit, out[2] = extension calls run, out[3] = calls that walk,
 * out[4] = bytes a record, out[5] = bytes of the trace arena.  After ygpu_run, before the next upload. */
int  ygpu_trace_volume(ygpu_ctx *ctx, uint64_t out[6]);

/* Asynchronous form: ygpu_submit hands the batch to the context and returns at once; the context's own worker thread does
 * upload + run + collect; ygpu_wait blocks until the ticket is complete and returns the results (ygpu_poll: 1 = complete, 0 = still running).
 * One host thread can so keep several contexts (devices) busy -- the reference needs one thread per QueryState for that (Query.c:642-684).
 * One open ticket per context: the caller keeps the batch alive until ygpu_wait returns, results stay valid until the next ygpu_submit /
 * ygpu_run on the context; a second ygpu_submit before ygpu_wait returns YGPU_EBUSY, a ygpu_wait for a ticket that is not open (or that another
 * thread is already waiting for) YGPU_EINVAL.  ygpu_last_error describes the ticket's failure once ygpu_wait has returned it; while a ticket is open
 * the text belongs to the worker and must not be read. */
typedef uint64_t ygpu_ticket;
int  ygpu_submit(ygpu_ctx *ctx, const ygpu_read_batch *batch, ygpu_ticket *ticket);
int  ygpu_poll(ygpu_ctx *ctx, ygpu_ticket ticket);
int  ygpu_wait(ygpu_ctx *ctx, ygpu_ticket ticket, ygpu_result_batch *out);
/* Elapsed device time of the last ygpu_run in milliseconds, total and per kernel family (HIP events on the
 * context's stream). names/ms arrays are owned by the context. */
int  ygpu_last_timing(ygpu_ctx *ctx, float *total_ms, int *n_stages, const char *const **names, const float **ms);

/* ---- stage-level entry points (what golden vectors are replayed against) ------------------------------ */

/* Fragment_t (Math.h:448-456) as produced by findFragmentsSort, plus the owning read/strand. */
typedef struct ygpu_fragment {
    uint32_t startRefOff;
    uint16_t startQueryOff, endQueryOff;
    uint16_t refLen;
    uint16_t reserved;
    uint32_t read_strand;    /* read * 2 + strand */
} ygpu_fragment;

/* A1+A2 for the resident batch: fragments sorted by (read, strand, diag, SQO). Output owned by ctx. */
int  ygpu_seed_join(ygpu_ctx *ctx, const ygpu_fragment **frags, uint64_t *n_frags);

/* The same, but the fragment array as ygpu_run builds it: a fragment of ONE hit whose neighbouring fragments of its
 * (read, strand) are both more than maxGap diagonals away is not written (it cannot become a clump while
 * wordLen < minMatch; with wordLen >= minMatch every fragment is kept).  refLen is set.  Output owned by ctx. */
int  ygpu_seed_join_kept(ygpu_ctx *ctx, const ygpu_fragment **frags, uint64_t *n_frags);

/* A3+A4 on the fragments of the last ygpu_seed_join: per clump (in creation order per read/strand) the
 * ordered fragment list before alignClump. clump_frag_start has n_clumps+1 entries. */
int  ygpu_chain(ygpu_ctx *ctx, const ygpu_fragment **clump_frags, const uint32_t **clump_frag_start,
                const uint32_t **clump_read_strand, uint64_t *n_clumps);

/* One DP call of findAffineGapScore (SW.cpp:798-1208) through its wrappers (SW.cpp:462-547). */
enum { YGPU_DP_FULL = 0, YGPU_DP_BANDED = 1, YGPU_DP_EXT_FWD = 2, YGPU_DP_EXT_REV = 3 };
typedef struct ygpu_dp_problem {
    uint32_t read;      /* index into the resident batch              */
    uint8_t  strand;    /* 0 forward codes, 1 reverse-complement      */
    uint8_t  mode;      /* YGPU_DP_*                                   */
    uint16_t qOff;      /* as passed to the reference wrapper          */
    uint16_t qLen;
    uint16_t rLen;      /* FULL/BANDED only                            */
    uint32_t rOff;
} ygpu_dp_problem;
typedef struct ygpu_dp_result {
    int32_t  score;
    uint16_t addedQLen, addedRLen;  /* extensions only */
    uint32_t op_start, n_ops;       /* ops in list order (head..tail) as the wrapper would merge them */
} ygpu_dp_result;
int  ygpu_dp_batch(ygpu_ctx *ctx, const ygpu_dp_problem *problems, uint32_t n,
                   const ygpu_dp_result **results, const uint32_t **ops, uint64_t *n_ops);
/* The same with the kernel family chosen explicitly.  AUTO = the kernels ygpu_run would use for these parameters: at the default band (-BW 5, -G >= 10)
 * the lane kernels -- k_ext_rows + k_ext_trace for extensions (findAGSForward/BackwardExtension, SW.cpp:479-533), the pure-diagonal shortcut and
 * k_gap_lanes / k_gap_wave for gap fills (findAGSAlignment[Banded], SW.cpp:462-475) -- otherwise the wave-per-problem DP.  WAVE = always the
 * wave-per-problem DP (dp_wave.h).  LANES_CAREFUL = the lane kernels with the k_ext_rows instantiation that serves splitClump's careful extensions
 * (SW.cpp:553-788 call the same findAGSExtension).  ygpu_dp_batch = AUTO. */
enum { YGPU_DP_KERNELS_AUTO = 0, YGPU_DP_KERNELS_WAVE = 1, YGPU_DP_KERNELS_LANES = 2, YGPU_DP_KERNELS_LANES_CAREFUL = 3 };
int  ygpu_dp_batch_ex(ygpu_ctx *ctx, const ygpu_dp_problem *problems, uint32_t n, int kernels,
                      const ygpu_dp_result **results, const uint32_t **ops, uint64_t *n_ops);

/* ---- host stages around the hot path (SURVEY.md 8(f) rows restated on the host) ------------------------
 * A session owns what processQueryFile (Query.c:551-709) sets up: parsed arguments, the mmap'ed .nib2 and
 * index, the query reader.  argv is the reference's own command line (`-x index -q reads -osh out ...`). */
typedef struct yaha_session yaha_session;
int  yaha_session_open(int argc, const char *const *argv, yaha_session **out);
void yaha_session_close(yaha_session *s);
const char *yaha_session_error(const yaha_session *s);
int  yaha_session_params(const yaha_session *s, ygpu_params *p);
int  yaha_session_index_view(const yaha_session *s, ygpu_index_view *v);
/* SAM header (@HD/@SQ/@PG, AlignOutput.c:30-111); text owned by the session. */
int  yaha_session_header(yaha_session *s, const char **text, size_t *len);
/* Read up to max_reads queries (readNextQuery, Query.c:102-228); b->n_reads == 0 at end of input.
 * The batch stays valid until the next call. */
int  yaha_session_next_batch(yaha_session *s, uint32_t max_reads, ygpu_read_batch *b);
/* Post-filter (OQC/FBS/dedup/MAPQ, GraphPath.cpp:897-1174) and format (printClump, AlignOutput.c:115-321)
 * the hot-path results of the current batch; text owned by the session until the next call. */
int  yaha_session_emit(yaha_session *s, const ygpu_result_batch *r, const char **text, size_t *len);
/* The same for a batch whose post-filter ran on the device: set a context up with the session's filter parameters (pointers into the session, valid until it is
 * closed; returns YGPU_EINVAL for runs the device stage does not take: -OQC N, break point costs that are no step function), then format what
 * ygpu_collect_filtered returned.  yaha_session_emit(ygpu_collect(...)) and yaha_session_emit_filtered(ygpu_collect_filtered(...)) give the same text. */
int  yaha_session_postfilter_params(yaha_session *s, ygpu_postfilter_params *p);
int  yaha_session_emit_filtered(yaha_session *s, const ygpu_filtered_batch *r, const char **text, size_t *len);
/* Bin size (-covbin, default 100), least mapping quality (-covq, default 0) and the sequence table for ygpu_depth_enable, from the session's arguments
 * (pointers into the session, valid until it is closed). */
int  yaha_session_depth_params(yaha_session *s, ygpu_depth_params *p);
/* The same for ygpu_events_enable: -evbin (default 100), -evq (default 0), -evclip (default 1) and the sequence table (pointers of their own into the session). */
int  yaha_session_events_params(yaha_session *s, ygpu_events_params *p);
/* The same for ygpu_pileup_enable: -puq (default 0) and the sequence table (pointers of their own into the session). */
int  yaha_session_pileup_params(yaha_session *s, ygpu_pileup_params *p);
/* For ygpu_snv_call_size: the three costs derived from -snverr (default 100 per mille), -snvmin (2), -snvdp (4) and -snvqual (20). */
int  yaha_session_snv_params(yaha_session *s, ygpu_snv_params *p);
/* For ygpu_indelcall_size: the three costs derived from -inderr (default 50 per mille: 22, 1301, 301), -indmin (2), -inddp (4) and -indqual (20). */
int  yaha_session_indelcall_params(yaha_session *s, ygpu_indelcall_params *p);
/* The same for ygpu_indels_enable: -idq (default 0), -idlen (default 1), capacity 0 and the sequence table (pointers of their own into the session). */
int  yaha_session_indel_params(yaha_session *s, ygpu_indel_params *p);
/* The same for ygpu_eprofile_enable: -epq (default 0) and the sequence table (pointers of their own into the session). */
int  yaha_session_eprofile_params(yaha_session *s, ygpu_eprofile_params *p);
/* The same for ygpu_junctions_enable: -bpq (default 0) and the sequence table (pointers of their own into the session). */
int  yaha_session_junction_params(yaha_session *s, ygpu_junction_params *p);
/* ---- BGZF compression on the device (-obh / -obs: BAM output; device/bgzf.hip, csrc/bgzf_core.h) ---------------------------------------------------------
 * A primitive of its own: a handle has its own stream, device buffers and page-locked staging for inputs of up to max_in_bytes; it touches no ygpu_ctx.
 * Handles are independent: two threads with two handles may compress at the same time; one handle serves one thread at a time.
 * compress cuts in[0 .. n_in) into payloads of 65 280 bytes (the last one shorter), deflates every payload into one BGZF block on the device (one workgroup
 * a block, fixed Huffman codes, the stored form wherever that is not larger; CRC-32 on the device as well) and writes the blocks one after the other, in
 * order, to out; *n_out = their bytes.  n_in == 0 gives *n_out == 0: no end-of-file block is added, the writer of a file owns that.  out_cap must be at least
 * bound(n_in) = ceil(n_in / 65280) * 65536.  An input over max_in_bytes or a smaller out_cap is YGPU_EINVAL, and the handle stays usable.  The same input
 * gives the same bytes every time. */
typedef struct ygpu_bgzf ygpu_bgzf;
int  ygpu_bgzf_open(int device, uint64_t max_in_bytes, ygpu_bgzf **h);
uint64_t ygpu_bgzf_bound(uint64_t n_in);
int  ygpu_bgzf_compress(ygpu_bgzf *h, const void *in, uint64_t n_in, void *out, uint64_t out_cap, uint64_t *n_out);
const char *ygpu_bgzf_last_error(ygpu_bgzf *h);
int  ygpu_bgzf_close(ygpu_bgzf *h);

/* ---- Coordinate order of a run's BAM records on the device (-obsort; device/bgzf.hip, device/bamsort_stage.h) ------------------------------------------------
 * A primitive of its own, like ygpu_bgzf: its own stream, device buffers and page-locked staging; it touches no ygpu_ctx.  One handle serves one thread.
 * open    max_store_bytes caps the device memory of the record store (segments and the per-record arrays); segment_bytes (0: 256 MB) is the size of a
 *         hipMalloc'd segment of record bytes, window_bytes (0: 1024 payloads of 65 280 bytes) that of a window of the sorted stream, rounded down to a
 *         multiple of 65 280 and at least 65 280.
 * append  a batch: n_records whole records in bytes[0 .. n_bytes), record i with keys[i] and lens[i] bytes (their sum is n_bytes).  A record never straddles
 *         two segments; a batch larger than what is left of the current segment opens a new one, a batch larger than a segment gets one of its own size.
 *         Passing max_store_bytes (or a refusal of the device) is YGPU_ENOMEM with a message; more than 2^32 - 1 records and an append after sort YGPU_EINVAL.
 * sort    a stable least-significant-digit radix sort of the keys, 8 bits a pass, the passes whose digit is the same in every key skipped; perm (may be
 *         null) receives the record number at every sorted place.  Equal keys keep the order they were appended in.
 * next    window w = bytes [w W, (w + 1) W) of the sorted stream (the records one behind the other in sorted order): gathered on the device, deflated by the
 *         kernels of ygpu_bgzf_compress, returned as whole BGZF blocks with *n_raw = the window's uncompressed bytes; *n_out == 0: the end.  out_cap must be
 *         at least ygpu_bgzf_bound(window_bytes).  The blocks of all windows together are the device encoder's blocks of the consecutive payloads of the
 *         sorted stream, whatever the window size, the segment size and the batches were.  Before sort: YGPU_EINVAL.
 * info    what = one of YGPU_BAMSORT_*: counters of the handle and the constants a caller needs. */
typedef struct ygpu_bamsort ygpu_bamsort;
enum { YGPU_BAMSORT_PASSES = 0,        /* radix passes the last sort ran */
       YGPU_BAMSORT_SEGMENTS = 1,      /* segments allocated */
       YGPU_BAMSORT_WINDOWS = 2,       /* windows returned so far */
       YGPU_BAMSORT_WINDOW_BYTES = 3,  /* W */
       YGPU_BAMSORT_TILE_KEYS = 4,     /* keys a scatter tile ranks (a workgroup) */
       YGPU_BAMSORT_STORE_BYTES = 5,   /* device memory of the store now */
       YGPU_BAMSORT_RECORDS = 6 };
int  ygpu_bamsort_open(int device, uint64_t max_store_bytes, uint64_t segment_bytes, uint64_t window_bytes, ygpu_bamsort **h);
int  ygpu_bamsort_append(ygpu_bamsort *h, const void *bytes, uint64_t n_bytes, const uint64_t *keys, const uint32_t *lens, uint32_t n_records);
int  ygpu_bamsort_sort(ygpu_bamsort *h, uint32_t *perm /* n entries, may be null */);
int  ygpu_bamsort_next(ygpu_bamsort *h, void *out, uint64_t out_cap, uint64_t *n_out, uint64_t *n_raw);
uint64_t ygpu_bamsort_info(ygpu_bamsort *h, int what);
const char *ygpu_bamsort_last_error(ygpu_bamsort *h);
int  ygpu_bamsort_close(ygpu_bamsort *h);

/* `yaha -g genome.fa [-L k] [-S s] [-H h]`: writes genome.nib2 and genome.X<LL>_<SS>_<HHHHH>S (Main.c:554-628). */
int  yaha_build_index(int argc, const char *const *argv);
/* The complete command-line program (index creation or query alignment on the GPU). */
int  yaha_main(int argc, char **argv);

#ifdef __cplusplus
}
#endif
#endif
