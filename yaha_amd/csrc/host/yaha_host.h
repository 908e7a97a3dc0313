// yaha_host.h -- host side of the MI355X-native YAHA hot path: everything the reference does *around* the
// per-read hot loop (file formats, argument handling, FASTA/FASTQ reading, OQC/FBS post-filter, SAM/Blast8
// output).  These stages are SURVEY.md 8(f) "next" rows restated on the host so that `yaha -x .. -q ..` keeps
// producing bit-identical output; the hot path itself (8(a) A1..A10) lives in ../device and is reached only
// through include/yaha_hip.h.
#pragma once
#include <cstdint>
#include <cstdio>
#include <string>
#include <map>
#include <mutex>
#include <atomic>
#include <algorithm>
#include <vector>
#include <memory>
#include <cstdlib>
#include <cstring>
#include <new>
#include "../../../include/yaha_hip.h"
#include "../depth_core.h"

namespace yaha {

// ---- 4-bit code tables (data contract, reference Math.c:141-157) -----------------------------------------
extern const uint8_t kFourBitCodes[128];
extern const char    kFourBitChars[16];
extern const uint8_t kFourBitCompCodes[16];
inline uint8_t map8to4(int c) { return kFourBitCodes[c & 127]; }
inline uint8_t get4(const uint8_t *bases, uint32_t off) { uint8_t b = bases[off >> 1]; return (off & 1) ? (b & 0xF) : (uint8_t)(b >> 4); }

// ---- Marsaglia xorshift RNG (reference Math.c:238-343) ----------------------------------------------------
struct RandState { uint32_t s[5]; };
void     randInitDefault(RandState &r);
uint32_t randBits(RandState &r);
void     randSample(RandState &r, const uint32_t *in, int inLen, uint32_t *out, int outLen);

// ---- memory-mapped read-only file -----------------------------------------------------------------------
struct MMap { void *ptr = nullptr; size_t size = 0; int fd = -1; bool open(const char *path, std::string &err); void close(); ~MMap() { close(); } };

// ---- .nib2 genome (reference Compress.c, BaseSeq.c) -----------------------------------------------------
struct BaseSeq { std::string name; uint32_t start; uint32_t length; };      // start in BASES (already normalised)
struct Genome {
    MMap map; std::vector<uint8_t> owned;              // either mapped file or in-memory image
    const uint8_t *bases = nullptr; uint64_t nBaseBytes = 0;
    std::vector<BaseSeq> seqs; uint32_t maxROff = 0;
    int findSeq(uint32_t off) const;                   // findBaseSequenceNum, BaseSeq.c:81-90
};
bool compressFasta(const char *fastaPath, std::vector<uint8_t> &nib2Image, std::string &err);   // Compress.c:220-329
bool parseNib2(const uint8_t *img, size_t size, Genome &g, std::string &err);                   // Compress.c:76-134
bool loadNib2(const char *path, Genome &g, std::string &err);
bool writeFile(const char *path, const void *data, size_t size, std::string &err);             // mode 0744, FileHelpers.c:279

// ---- index (reference Index.c:49-335, Query.c:596-626) --------------------------------------------------
struct IndexFile {
    MMap map; std::vector<uint32_t> owned;
    int wordLen = 0; int maxHits = 0; uint32_t totalMatches = 0; const uint32_t *SO = nullptr; const uint32_t *ROA = nullptr;
};
// builds the complete file image {-1, wordLen, maxHits, total} + SO[4^L+1] + ROA[total] (huge-page backed: 4.3 GB at L=15)
struct IndexImage { uint32_t *p = nullptr; size_t words = 0, bytes = 0; bool alloc(size_t n); void release(); uint32_t &operator[](size_t i) { return p[i];
    } ~IndexImage() { release(); } };
bool buildIndex(const Genome &g, int wordLen, int skipDist, int maxHits, IndexImage &image, FILE *log);
// the same image built on HIP device `device` (device/index_build.hip)
bool buildIndexDevice(int device, const Genome &g, int wordLen, int skipDist, int maxHits, IndexImage &image, FILE *log, std::string &err);
int  visibleDevices();                                  // HIP devices this process can use (0 on a machine without a GPU)
bool parseIndex(const uint32_t *img, size_t bytes, IndexFile &ix, std::string &err);
bool loadIndex(const char *path, IndexFile &ix, std::string &err);

// ---- arguments (reference AlignArgs.c, Main.c) -----------------------------------------------------------
struct Args {
    std::string gfileName, xfileName, qfileName = "stdin", ofileName; bool haveG = false, haveX = false, haveO = false;
    int numThreads = 1; bool fastq = false;
    int wordLen = 15, skipDist = 1, maxHits = -1;
    int maxGap = 50, maxIntron = -1, minMatch = 25; float minIdentity = 0.9f; int bandWidth = 5, maxDesert = 50, minRawScore = -1, minNonOverlap = -1;
    bool affineGapScoring = true; int GOCost = 5, GECost = 2, RCost = 3, MScore = 1, XCutoff = 25; int minExtLength = 0;
    bool OQC = true; int OQCMinNonOverlap = -1, BPCost = 5, maxBPLog = 5; bool FBS = false; float FBS_PSLength = 0.90f, FBS_PSScore = 0.90f;
    int maxQueryLength = 32000; bool verbose = false, outputBlast8 = false, outputSAM = true, hardClip = true;
    bool outputBAM = false;                              // -obh / -obs: the SAM writer's records in BAM's layout, BGZF-compressed (bam.cpp); outputSAM stays set
    // -obsort: the BAM in coordinate order with FILE.bai beside it, both written after the last alignment; -sortmem GB caps the record store (bam.cpp BamSorter)
    bool bamSort = false, haveSortMem = false; int sortMemGB = 32;
    // extensions of this implementation (not in the reference CLI)
    int batchReads = 0; int device = 0; int gpus = 1; int ctxPerGpu = 3; bool cpuIndex = false; bool devicePostFilter = true;      // batchReads 0: batches of ~16 M bases
    // read-depth track: -ocov FILE (bedGraph), -covbin B (bases a bin), -covq Q (records below this mapping quality cover nothing)
    bool haveCov = false, haveCovBin = false, haveCovQ = false; std::string covFileName; int covBin = 100, covMinQ = 0;
    // evidence track: -oev FILE (mismatch / deleted / insertion / clipped-end counts per bin), -evbin B, -evq Q, -evclip N (a clip counts from N bases on)
    bool haveEv = false, haveEvBin = false, haveEvQ = false, haveEvClip = false; std::string evFileName; int evBin = 100, evMinQ = 0, evMinClip = 1;
    // breakpoint calls: -obp FILE (BEDPE, one line a cluster of split-read junctions), -bpq Q (records below this mapping quality join nothing), -bpw W (cluster window)
    bool haveBp = false, haveBpQ = false, haveBpW = false; std::string bpFileName; int bpMinQ = 0, bpWindow = 10;
    // allele pileup: -opu FILE (the sites where at least -pumin reads disagree with the reference, with the counts of A C G T N del ins), -puq Q
    bool havePu = false, havePuMin = false, havePuQ = false; std::string puFileName; int puMinAlt = 2, puMinQ = 0;
    // indel alleles: -oid FILE (one line per insertion / deletion allele that at least -idmin printed records carry), -idlen L (shortest op counted), -idq Q
    bool haveId = false, haveIdMin = false, haveIdLen = false, haveIdQ = false; std::string idFileName; int idMin = 2, idLen = 1, idMinQ = 0;
    // error profile: -oep FILE (substitution spectrum, indel lengths, identity of the records, errors by position in the read, of the printed records), -epq Q
    bool haveEp = false, haveEpQ = false; std::string epFileName; int epMinQ = 0;
    // SNV calls: -osnv FILE (VCF 4.2: the sites the pileup genotypes as 0/1 or 1/1), -snverr E (sequencing error in per mille), -snvmin N (reads that carry the
    // allele), -snvdp D (depth), -snvqual Q (QUAL in phred); the mapping-quality gate is the pileup's -puq
    bool haveSnv = false, haveSnvErr = false, haveSnvMin = false, haveSnvDp = false, haveSnvQual = false; std::string snvFileName;
    int snvErr = 100, snvMin = 2, snvDp = 4, snvQual = 20;
    // indel calls: -oindel FILE (VCF 4.2: the run's indel alleles left-normalised, merged and genotyped at their anchor base), -inderr E (per mille), -indmin N
    // (reads that carry the allele), -inddp D (reads that cover the anchor), -indqual Q, -indshift S (bases an allele may move; 0: as the aligner put it); gate -puq
    bool haveIndel = false, haveIndErr = false, haveIndMin = false, haveIndDp = false, haveIndQual = false, haveIndShift = false; std::string indFileName;
    int indErr = 50, indMin = 2, indDp = 4, indQual = 20, indShift = 256;
    bool query = false, index = true, compress = false, uncompress = false;   // -c / -u: .fa -> .nib2 / .nib2 -> .fasta only (Main.c:284-293, non-user builds of the reference)
};
void postProcessArgs(Args &a, bool query);                                  // AlignArgs.c:108-169
// returns 0 to continue, >0 exit code+1 to stop (usage / error)
int  parseArgs(int argc, char **argv, Args &a);                            // Main.c:187-565
void paramsFromArgs(const Args &a, ygpu_params &p);
void snvParamsFromArgs(const Args &a, ygpu_snv_params &p);                  // snv.cpp: the three costs from -snverr, the three thresholds
void indelcallParamsFromArgs(const Args &a, ygpu_indelcall_params &p);      // indelcalls.cpp: the three costs from -inderr, the three thresholds
std::string samHeader(const Args &a, const Genome &g);                      // AlignOutput.c:30-111

// ---- reads (reference Query.c:63-228, QueryState.c:172-187) ---------------------------------------------
struct Read {
    std::string id; std::string fwd, rev; std::vector<uint8_t> fwdCodes; std::string qual;
    int len() const { return (int)fwd.size(); }
};
// One record of the input as byte ranges (offsets from base): produced serially by ReadSplitter, parsed by any thread.
struct Span { std::shared_ptr<std::vector<char>> hold; const char *base = nullptr; size_t idLen = 0, seq0 = 0, seqEnd = 0, qual0 = 0, qualEnd = 0; };
// Record boundaries of a FASTA/FASTQ stream (memory-mapped file, or stdin/pipe read in blocks); see reader.cpp for the rules.
struct ReadSplitter {
    size_t blockBytes = 32u << 20;                       // streaming sources are read in blocks of this size
    int fd = -1; bool ownFd = false; const char *mapPtr = nullptr; size_t mapLen = 0;
    std::shared_ptr<std::vector<char>> chunk; const char *cur = nullptr, *end = nullptr; bool atEof = true, done = true, fastq = false;
    bool open(const char *path, std::string &err);       // peeks '>' / '@' (Query.c:63-74)
    void close();
    bool nextSpan(Span &s);                              // false at the end of input (an empty sequence ends it, Query.c:216-217)
    size_t nextSpans(size_t maxSpans, std::vector<Span> &out) { return nextSpans(maxSpans, ~(size_t)0, out); }
    size_t nextSpans(size_t maxSpans, size_t maxBases, std::vector<Span> &out);   // up to maxSpans records, stopping once their sequences reach maxBases bytes
    ~ReadSplitter() { close(); }
  private:
    void fill(); bool seek(char c, size_t *pos); bool seekNlAt(size_t *pos);
};
// id / sequence / quality / codes of one record; false = the record is skipped (with the reference's warning on stderr)
bool parseSpan(const Span &s, bool fastq, int maxQueryLength, int wordLen, Read &r);
void finishRead(Read &r);                                // 4-bit codes + reverse-complement text from r.fwd
struct ReadReader {                                      // sequential reader: one accepted read per call
    ReadSplitter split; bool fastq = false; int maxQueryLength = 32000; int wordLen = 15;
    bool open(const char *path, std::string &err);
    bool next(Read &r);                                  // readNextQuery; false at EOF
    void close();
};
void seedFromRead(const Read &r, RandState &rs);          // generateRandomSeed

// ---- post filter + output (reference GraphPath.cpp:294-1175, AlignOutput.c:115-321) ---------------------
struct OutClump {                                        // one clump as it reaches printClump
    ygpu_clump c; const uint32_t *ops;                   // ops[0..c.n_ops)
    uint8_t status; uint8_t mapQuality = 255; uint16_t numSecondaries = 0, matchedPrimary = 0;
};
// clumps: QS->clumps head->tail after postProcessClumps.  Result: print order.  primaryCount = QS->primaryCount.
void postFilter(const Args &a, const Genome &g, const Read &r, const ygpu_clump *clumps, uint32_t n, const uint32_t *ops,
                std::vector<OutClump> &out, int &primaryCount);
// Output text of a batch: a plain growable byte buffer that is reused from batch to batch (no zero-fill on growth, no per-record allocation; a formatter
// thread keeps its buffers, so that the steady state touches no allocator and maps no new pages).
struct Text {
    char *p = nullptr; size_t len = 0, cap = 0;
    Text() {} Text(const Text &) = delete; Text &operator=(const Text &) = delete;
    Text(Text &&o) noexcept : p(o.p), len(o.len), cap(o.cap) { o.p = nullptr; o.len = o.cap = 0; }
    Text &operator=(Text &&o) noexcept { if (this != &o) { free(p); p = o.p; len = o.len; cap = o.cap; o.p = nullptr; o.len = o.cap = 0; } return *this; }
    ~Text() { free(p); }
    void clear() { len = 0; }
    char *room(size_t n) { if (len + n > cap) grow(len + n); return p + len; }      // at least n writable bytes at the end
    void append(const char *s, size_t n) { memcpy(room(n), s, n); len += n; }
  private:
    void grow(size_t need) { size_t c = cap ? cap : (1u << 16); while (c < need) c += c / 2; char *q = (char *)realloc(p, c); if (!q) throw std::bad_alloc(); p = q; cap = c; }
};
void printClump(const Args &a, const Genome &g, const Read &r, const OutClump &oc, int primaryCount, Text &out);

// ---- BAM output (-obh / -obs; bam.cpp, ../bgzf_core.h) ----------------------------------------------------------------------------------------------------------
// The uncompressed header: "BAM\1", samHeader's text, the genome's sequences.  A record: printClump's record in BAM's layout, appended to out (false: the
// clump spans two sequences and is dropped, as printClump drops it).
std::string bamHeader(const Args &a, const Genome &g);
// entry (may be null): what the sort and the index need of the record -- sequence, position, bytes (block_size's four included), end (exclusive), bin
struct BamEntry { uint32_t ref, pos, len, end, bin; };
bool bamRecord(const Args &a, const Genome &g, const Read &r, const OutClump &oc, int primaryCount, Text &out, BamEntry *entry = nullptr);
struct BamStats { std::atomic<uint64_t> records{0}, bytesRaw{0}, bytesWritten{0}, blocks{0}, blocksStored{0}, deviceBatches{0}, hostBatches{0}; };
// What a formatter thread compresses its batches with: a device handle of its own (ygpu_bgzf_*, looked up weakly as the tracks' entry points are), opened
// when first needed and reopened when a batch outgrows it, or the host's encoder -- without the entry points, when no handle can be opened, with
// YAHA_HOST_BGZF=1.  No end-of-file block is written here (bgzfEof: the writer's, once).
struct BgzfPacker {
    BgzfPacker(); ~BgzfPacker(); BgzfPacker(const BgzfPacker &) = delete; BgzfPacker &operator=(const BgzfPacker &) = delete;
    static bool deviceEntryPoints();                                      // does this build have ygpu_bgzf_*?
    // in[0 .. n) as whole BGZF blocks into out (cleared first); 0, or the device's error code with err = the handle's message
    int  pack(int device, const char *in, size_t n, Text &out, BamStats &st, std::string &err);
    void packHost(const char *in, size_t n, Text &out, BamStats &st);     // the host's encoder, whatever the build has
  private:
    struct Impl; Impl *impl;
};
void bgzfEof(Text &out);                                                  // appends the 28-byte end-of-file block
// -obsort: the run's records, put into coordinate order and written with their index at the end of the run.  The writer thread appends every batch in ticket
// order; finish() sorts -- stable, so equal keys keep print order --, writes the header's blocks (the host's encoder), the sorted stream's blocks window by
// window, the end-of-file block, and FILE.bai (bai.cpp).  The store is a device handle (ygpu_bamsort_*, weak references) on device `device`; without the entry
// points, with YAHA_HOST_BAMSORT=1 or when the handle cannot be opened it is host memory, ordered with std::stable_sort and compressed through BgzfPacker.  Both
// are capped by capBytes.  A failure of an opened handle is an error of the run.
struct BamSortStats { uint64_t records = 0, segments = 0, windows = 0, passes = 0, baiBytes = 0; bool device = false; };
struct BamSorter {
    BamSorter(int device, uint64_t capBytes); ~BamSorter(); BamSorter(const BamSorter &) = delete; BamSorter &operator=(const BamSorter &) = delete;
    // 0, or an error code with err = a message (passing the cap: it names -sortmem)
    int append(const char *bytes, size_t n, const BamEntry *entries, size_t nEntries, std::string &err);
    int finish(FILE *out, const std::string &baiPath, const std::string &rawHeader, size_t nRefs, BamStats &st, std::string &err);
    BamSortStats stats; double msAppend = 0;
  private:
    struct Impl; Impl *impl;
};
// The BAI of a sorted file (../bai_core.h): the entries in file order, the file offsets of the record blocks (coffs[nBlocks] = the end-of-file block's).
void bamSortOrder(const BamEntry *entries, size_t n, uint32_t *perm);      // the host's ordering (stable): perm[j] = the record at sorted place j
std::string baiBuild(const BamEntry *sorted, size_t n, size_t nRefs, const uint64_t *coffs, size_t nBlocks);

// ---- the genome's sequence table, as every device stage's parameter block takes it ---------------------------------------------------------------------------
struct SeqTable {
    std::vector<uint32_t> start, length;
    void set(const Genome &g) { start.clear(); length.clear(); for (auto &sq : g.seqs) { start.push_back(sq.start); length.push_back(sq.length); } }
    template <class P> void into(P &p) const { p.n_seqs = (uint32_t)start.size(); p.seq_start = start.data(); p.seq_length = length.data(); }
};

// ---- a side output of a query run: a file beside the alignments, made of the records that are printed (the kinds follow) -------------------------------------
// The run driver (pipeline.cpp) knows the outputs by this interface alone, as a list: output k is bit k of a batch's onDevice mask -- the device stage behind
// the post-filter did the batch's share of it, all but the reads it handed back unfiltered -- and owns slot k of every batch object.  Every hook defaults to
// "nothing to do".  The device entry points of a kind are weak references: host code links and runs without them (the CPU tier's test doubles).
struct CtxAt { ygpu_ctx *ctx; int index, image, device; };                // a context of the run: its number, the index image it shares, the HIP device
struct SideOutput {
    struct Slot { virtual ~Slot() {} };                                   // what a kind keeps with a batch; made once per batch object, reused with it
    virtual ~SideOutput() {}
    virtual const char *name() const = 0;                                 // the option of its file: how messages speak of it
    // set-up: the kind's own options; nImages index images (-gpus), nContexts contexts in all
    virtual bool setup(const Args &a, const Genome &g, int nImages, int nContexts, std::string &err) = 0;
    // per context, by its thread, before its first batch: 0 = the device does this context's batches; YGPU_ENOMEM = no room on the device, the run stops with
    // ygpu_last_error; anything else (no entry points in this build, the kind's YAHA_HOST_* switch, a refusal) = the formatters do them
    virtual int  enable(const CtxAt &) { return YGPU_ENODEV; }
    // per batch of such a context, by the thread that runs its post-filter: before ygpu_postfilter (list order) and after it (reverse order)
    virtual int  beforeFilter(const CtxAt &, size_t /*batchBases*/) { return 0; }
    virtual int  afterFilter(const CtxAt &, Slot *) { return 0; }
    // per batch by the formatter thread that has it: beginBatch (onDevice: the slot holds what afterFilter put there), then add for every printed record and
    // endRead (wantsReads) for every read with its printed records -- those the device did not do --, then endBatch
    virtual Slot *newSlot() const { return nullptr; }
    virtual void beginBatch(Slot *, bool /*onDevice*/) const {}
    virtual void add(const OutClump &, const Read &, Slot *) {}
    virtual bool wantsReads() const { return false; }
    virtual void endRead(const OutClump *, uint32_t /*n*/, const Read &, uint32_t /*read*/, Slot *) const {}
    virtual void endBatch(Slot *) {}
    virtual void written(Slot *) {}                                       // per batch by the writer thread, in ticket order
    // the end of a run that got there: what the devices hold joins the host's, mainOut is flushed, the file is written; false: failed, with a line in log
    virtual bool finish(FILE *mainOut, FILE *log, bool timing) = 0;
    virtual void stats(std::string &line) const = 0;                      // its keys of the stats line, each with its leading ", "
};

// ---- the binned tracks: read depth (-ocov), the evidence track (-oev) and the allele pileup (-opu) (depth.cpp, events.cpp, pileup.cpp; ../*_core.h) --------
// The host's array of a track, in the layout the device uses (one routine a kind, *_core.h): `channels` uint32 a bin, bin-major.  The formatter threads add the
// records the device did NOT count -- runs whose post-filter stays on the host (-dpf N, -OQC N, YAHA_HOST_OQC=1), the reads the device stage hands back
// unfiltered, and everything when the library has no device entry points for the track or refuses to enable them -- with relaxed atomics.  The device stage
// feeds an array of its own per index image, enabled by every context of the image (the first makes it): at the end of the run the arrays are added -- each
// through its feeder, the first context of the image to post-filter a batch (such a context is never left out afterwards) -- and the file is written after the
// last alignment.  A kind adds what differs: its options, what a record adds, the parameters of its device stage, its entry points and its lines.
struct BinnedTrack : SideOutput {
    // the words a kind is spoken of with: the options of the bin size and of the file, the array's noun, the file's, the switch that keeps it on the host, its keys
    // of the stats line (bins, device records, host records, sum)
    struct Names { const char *binOpt, *fileOpt, *array, *file, *hostSwitch, *statsFmt; };
    typedef int (*SizeFn)(ygpu_ctx *, uint64_t *);
    typedef int (*CollectFn)(ygpu_ctx *, uint32_t *, uint64_t[4]);
    // what the kind is: how it is spoken of, its words a bin, its device entry points (null in a build without them)
    const Names names; const uint32_t channels;
  private:
    const bool haveEnable; const SizeFn devSize; const CollectFn devCollect;
    const Genome *genome = nullptr; std::string file; std::vector<CtxAt> ctxs; std::vector<std::atomic<int>> feeder;      // feeder[k]: 1 + the context that feeds image k
  public:
    SeqTable seqs; std::vector<uint32_t> binBase; uint64_t nBins = 0; uint32_t bin = 100, minMapq = 0;
    uint32_t *data = nullptr;                                             // nBins * channels words, zeroed; relaxed atomic adds
    uint64_t hostRecords = 0, hostSkipped = 0, hostDropped = 0;           // (atomic adds as well) records the host counted / gated by MAPQ / dropped
    uint64_t devRecords = 0, devSkipped = 0, devDropped = 0, devHandedBack = 0;
    BinnedTrack(const BinnedTrack &) = delete; BinnedTrack &operator=(const BinnedTrack &) = delete;
    ~BinnedTrack() override { free(data); }
    const char *quietFor = nullptr;                                       // set: the track serves that option alone -- no file, no keys of the stats line, no merge
    const char *name() const override { return quietFor ? quietFor : names.fileOpt; }
    int  enable(const CtxAt &at) override;
    int  beforeFilter(const CtxAt &at, size_t) override;                  // (the image's feeder)
    bool finish(FILE *mainOut, FILE *log, bool timing) override;
    void stats(std::string &line) const override;
    bool deviceEntryPoints() const { return haveEnable && devSize && devCollect; }      // does this build have the kind's ygpu_*_enable / _size / _collect?
    virtual int deviceEnable(ygpu_ctx *ctx) const = 0;                    // YGPU_ENODEV without the entry points
    int  deviceCollect(ygpu_ctx *ctx, std::string &err);                  // adds the image's array and statistics to this track
    void feeders(std::vector<ygpu_ctx *> &ctx, std::vector<int> &dev) const;      // a feeding context per image that has one, image by image, with its HIP device
    // The end of the run: what the devices counted joins what the host counted.  feeders[k]: a context of index image k that fed the image's array (n may be 0).
    // Returns 0, or the device's error code with *failed = the image it came from.  Here: deviceCollect of every image; a kind whose array does not travel
    // (the pileup) has its own way.
    virtual int mergeDevices(ygpu_ctx *const *feeders, int n, const Genome &g, int *failed, std::string &err);
    virtual uint64_t sum() const;                                         // over all bins and channels
    virtual std::string extraStats() const { return std::string(); }      // more keys of the stats line, each with its leading ", "
    virtual std::string mergeNote() const { return std::string(); }       // where mergeDevices' time went, for the YAHA_TIMING line
    bool write(const char *path, const Genome &g, std::string &err) const;      // path "stdout" = standard output
  protected:
    BinnedTrack(const Names &nm, uint32_t ch, bool enable, SizeFn sz, CollectFn co) : names(nm), channels(ch), haveEnable(enable), devSize(sz), devCollect(co) {}
    // (a kind's setup: its file, the layout, then its host storage -- allocate)
    bool init(const Genome &g, const std::string &path, int binBases, int minQ, int nImages, int nContexts, std::string &err);
    ydepth::Layout layout() const { return ydepth::Layout{seqs.start.data(), seqs.length.data(), binBase.data(), (uint32_t)seqs.start.size(), bin, minMapq}; }
    void countRecord(int gate);                                           // what became of a record the host walked (ydepth::COUNTED ...)
    virtual bool allocate(std::string &err);                              // the host's storage for nBins bins: here the dense, zeroed `data`
    virtual bool writeLines(FILE *f, const Genome &g) const = 0;          // the kind's lines; false: a write failed
};
struct DepthTrack : BinnedTrack {                                         // bedGraph of the covered bases (-covbin, -covq)
    DepthTrack();
    bool setup(const Args &a, const Genome &g, int nImages, int nContexts, std::string &err) override;
    void add(const OutClump &oc, const Read &r, Slot *) override;
    int  deviceEnable(ygpu_ctx *ctx) const override;
  protected:
    bool writeLines(FILE *f, const Genome &g) const override;
};
struct EventsTrack : BinnedTrack {                                        // mismatched bases, deleted bases, insertions, clipped ends left and right (-evbin, -evq, -evclip)
    uint32_t minClip = 1;
    EventsTrack();
    bool setup(const Args &a, const Genome &g, int nImages, int nContexts, std::string &err) override;
    void add(const OutClump &oc, const Read &r, Slot *) override;
    int  deviceEnable(ygpu_ctx *ctx) const override;
  protected:
    bool writeLines(FILE *f, const Genome &g) const override;
};
// The allele pileup: A C G T N del ins per reference base (../pileup_core.h), written as the table of the sites where at least minAlt reads disagree with the
// reference.  Its device array (28 bytes a reference base) never travels: at the end of the run every source -- each index image, the host's own counts --
// lists its candidates (nonref >= 1), every image gathers its counts at the sorted union, the host adds its own and applies minAlt (mergeDevices).  Nothing
// dense on the host either: its counts live in blocks of kBlock slots, made when a formatter thread first adds to one (`data` stays null) -- a pointer per
// block, 6 MB of them at 3.1 Gbp, and 112 KB for every block the host's share of the records touches.
struct PileupTrack : BinnedTrack {                                        // (a bin of one base, seven channels; -pumin, -puq)
    enum : uint32_t { kBlock = 4096 };
    uint32_t minAlt = 2;
    std::vector<uint32_t *> blocks;                                       // blocks[slot / kBlock]: kBlock * 7 zeroed words, or null (atomic loads, made by compare-and-swap)
    uint64_t hostCounted = 0, devCounted = 0, nCandidates = 0;            // counts added by the formatters / on the devices; slots of the union
    struct Site { uint32_t slot, ref; uint32_t n[7]; };                   // ref: the reference's 4-bit code
    std::vector<Site> sites;                                              // what writeLines prints, ascending (made by mergeDevices)
    PileupTrack();
    ~PileupTrack() override;
    bool setup(const Args &a, const Genome &g, int nImages, int nContexts, std::string &err) override;
    void add(const OutClump &oc, const Read &r, Slot *) override;
    int  deviceEnable(ygpu_ctx *ctx) const override;
    int  mergeDevices(ygpu_ctx *const *feeders, int n, const Genome &g, int *failed, std::string &err) override;
    // what mergeDevices stands on, for the SNV calls as well (snv.cpp): the sorted union of the sources' candidates -- the host's blocks if withHost, every
    // feeder's selection -- and the sources' summed rows there (all.size() * 7 words); account: the feeders' statistics join this track's
    int  unionRows(ygpu_ctx *const *feeders, int n, bool withHost, bool account, const Genome &g, std::vector<uint32_t> &all, std::vector<uint32_t> &rows, int *failed,
                   std::string &err);
    int  candidatesUnion(ygpu_ctx *const *feeders, int n, bool withHost, const Genome &g, std::vector<uint32_t> &all, int *failed, std::string &err);      // the union alone
    // the host's counts as a list for ygpu_pileup_add: the slots of its blocks that hold something, ascending, and their rows
    void hostRows(std::vector<uint32_t> &slots, std::vector<uint32_t> &rows) const;
    // Folds into feeders[0]'s array (ygpu_pileup_add) what the callers -- the SNV calls, the indel calls -- need summed there, each thing ONCE a run whoever asks
    // first: the host's rows (withHost) unless they have been folded, and every other image's rows at those of `at` (ascending, distinct; may be null) that
    // have not been.  *folded += list entries added; *anyAdded: the array is no longer the image's own.  0, or the device's code with *bad = the context.
    int  foldOnce(ygpu_ctx *const *feeders, int n, bool withHost, const std::vector<uint32_t> *at, uint64_t *folded, bool *anyAdded, ygpu_ctx **bad);
    // the sources' summed rows at `slots` for a caller on the host, after whatever has been folded: feeders[0]'s array, the others' where they have not been
    // folded into it, the host's unless they have been
    int  rowsAt(ygpu_ctx *const *feeders, int n, const std::vector<uint32_t> &slots, std::vector<uint32_t> &rows, ygpu_ctx **bad);
    bool hostFolded = false; std::vector<uint32_t> othersFolded;          // what foldOnce has done: the host's rows; the slots of the other images (ascending)
    uint64_t sum() const override { return hostCounted + devCounted; }    // (the counts added: the sum over the arrays without reading 28 bytes a base)
    std::string extraStats() const override;
    std::string mergeNote() const override;
    double msCandidates = 0, msGather = 0;                                // mergeDevices: the selections and their copies / the gathers
  protected:
    bool allocate(std::string &err) override;                             // the table of blocks, all null (the bin must be 1)
    bool writeLines(FILE *f, const Genome &g) const override;
    const uint32_t *row(uint32_t slot) const { const uint32_t *b = blocks[slot / kBlock]; return b ? b + (size_t)(slot % kBlock) * 7 : nullptr; }
  private:
    uint32_t *block(uint32_t slot);                                       // the block of a slot, made if it is not there yet
};

// ---- split-read breakpoint calls (-obp; junctions.cpp, ../junction_core.h) ---------------------------------------------------------------------------------
// The junctions of the whole run, their clustering and the BEDPE writer.  The junctions of a batch are made on the device behind its post-filter
// (ygpu_junctions_*), per context and per batch, nothing shared, and travel with the batch in its slot; the formatter threads make the ones the device did not
// -- the reads it handed back unfiltered, runs whose post-filter stays on the host, builds without the entry points, YAHA_HOST_JUNCTIONS -- with the same
// routine (junction_core.h), from a read's printed records.  The writer thread adds every batch's junctions in ticket order, merged by read: the list is in
// read order whatever -ctx and -batch are.
struct JunctionTrack : SideOutput {
    SeqTable seqs; uint32_t minMapq = 0, window = 10;
    std::vector<ygpu_junction> all;                                       // (read: the index within its batch; not used after the merge)
    uint64_t devReads = 0, hostReads = 0, devSkipped = 0, hostSkipped = 0, devHandedBack = 0, nClusters = 0, nJunctions = 0;      // reads with junctions by who made them ...
    // a batch's: the junctions the device made and its statistics; the ones the formatter made, and its counts
    struct Batch : Slot { std::vector<ygpu_junction> dev, host; uint64_t devStats[4] = {0, 0, 0, 0}, hostReads = 0, hostSkipped = 0; };
    const char *name() const override { return "-obp"; }
    bool setup(const Args &a, const Genome &g, int nImages, int nContexts, std::string &err) override;      // -bpq, -bpw
    int  enable(const CtxAt &at) override;                                // (no room for a context's lists: the formatters make its junctions)
    int  afterFilter(const CtxAt &at, Slot *s) override;                  // the junctions of the context's last ygpu_postfilter: few, and on their way while the clumps are sized
    Slot *newSlot() const override { return new Batch; }
    void beginBatch(Slot *s, bool onDevice) const override;
    bool wantsReads() const override { return true; }
    // the junctions of one read's printed records on the host, appended to the batch's (ordinal order)
    void endRead(const OutClump *recs, uint32_t n, const Read &r, uint32_t read, Slot *s) const override;
    // one batch, in output order: the device's junctions (read order) and the formatter's (read order) merged by read
    void written(Slot *s) override;
    bool finish(FILE *mainOut, FILE *log, bool timing) override;
    void stats(std::string &line) const override;
    static bool deviceEntryPoints();                                      // does this build have ygpu_junctions_*?
    bool write(const char *path, const Genome &g, std::string &err);      // clusters and writes; path "stdout" = standard output
  private:
    const Genome *genome = nullptr; std::string file;
};

// ---- indel alleles (-oid; indels.cpp, ../indel_core.h) --------------------------------------------------------------------------------------------------------
// The run's alleles -- (slot, type, length, inserted bases) -> records that carry it -- and their writer.  The device counts them in a hash table per context
// behind its post-filter (ygpu_indels_*): a context's table is drained BEFORE a batch that could take it past one half (a batch has at most one event per two
// bases), whenever more than a quarter of it is in use after one, and once more at the end.  The table has two entries per base of the largest batch the
// splitter cuts (indel_core.h tableCapacity), as far as that is known before the reads are: -batch N gives a read count, and N reads of the greatest length
// would ask for more than a batch ever holds -- the table then stops at that of the default batch, and the drain before a batch keeps the load where the rule
// wants it.  The formatter threads count what the device did not -- runs whose post-filter stays on the host, the reads it hands back unfiltered, builds
// without the entry points, YAHA_HOST_INDELS -- with the same walk (indel_core.h) into the batch's slot, merged here under a lock once per batch.
struct IndelKey { uint64_t w0, w1, w2; };
struct IndelKeyLess { bool operator()(const IndelKey &a, const IndelKey &b) const; };      // the order of the file (indel_core.h keyLess)
struct IndelTrack : SideOutput {
    SeqTable seqs; std::vector<uint32_t> binBase; uint64_t nSlots = 0, capacity = 0; uint32_t minMapq = 0, minLen = 1, minCount = 2;
    std::mutex mu; std::map<IndelKey, uint64_t, IndelKeyLess> alleles;
    uint64_t hostRecords = 0, hostSkipped = 0, hostDropped = 0, hostEvents = 0;           // (under mu, by merge)
    uint64_t devRecords = 0, devSkipped = 0, devDropped = 0, devEvents = 0, devHandedBack = 0, devLost = 0, drains = 0, nLines = 0;
    // what a formatter thread gathers of one batch before it merges: the events' keys and what became of the records it walked
    struct Local : Slot { std::vector<IndelKey> keys; uint64_t records = 0, skipped = 0, dropped = 0; };
    const char *quietFor = nullptr;                                       // set: the track serves that option alone (-oindel) -- -puq and length 1, no file, no keys
    const char *name() const override { return quietFor ? quietFor : "-oid"; }
    bool setup(const Args &a, const Genome &g, int nImages, int nContexts, std::string &err) override;      // -idq, -idlen, -idmin; the table's capacity
    int  enable(const CtxAt &at) override;                                // (remembers the context for the end of the run)
    int  beforeFilter(const CtxAt &at, size_t batchBases) override;
    int  afterFilter(const CtxAt &at, Slot *) override;
    Slot *newSlot() const override { return new Local; }
    void add(const OutClump &oc, const Read &r, Slot *s) override;        // one record printClump was called for
    void endBatch(Slot *s) override;                                      // ... and the batch's share into the run's alleles; clears the slot
    bool finish(FILE *mainOut, FILE *log, bool timing) override;          // what every context's table still holds, then the file
    void stats(std::string &line) const override;
    static bool deviceEntryPoints();                                      // does this build have ygpu_indels_*?
    int  deviceDrain(ygpu_ctx *ctx, bool duringRun, std::string &err);    // collects and clears the context's table into the run's alleles
    bool write(const char *path, const Genome &g, std::string &err);      // applies minCount; path "stdout" = standard output
  private:
    int drainAbove(ygpu_ctx *ctx, uint64_t more, uint64_t limit);         // drains the table if it holds entries and they, with `more`, pass limit
    const Genome *genome = nullptr; std::string file; std::vector<CtxAt> enabled;
};

// ---- the error profile (-oep; eprofile.cpp, ../eprofile_core.h) -----------------------------------------------------------------------------------------------
// The run's table of 1556 counters -- substitutions by reference and read base, insertion and deletion lengths, the records' identity, pairs / errors /
// insertions / deletions by position in the read -- and its writer.  The device keeps a table per context behind its post-filter (ygpu_eprofile_*: in LDS for a
// workgroup's whole share of a batch), read once at the end of the run; the formatter threads count what the device did not -- runs whose post-filter stays on
// the host, the reads it hands back unfiltered, builds without the entry points, YAHA_HOST_EPROFILE -- with the same walk (eprofile_core.h) into the batch's
// slot, added here under a lock once per batch.
struct EProfileTrack : SideOutput {
    SeqTable seqs; uint32_t minMapq = 0;
    std::mutex mu; std::vector<uint64_t> table;                           // the host's share while the run lasts (under mu), the whole run's after finish
    uint64_t hostRecords = 0, hostSkipped = 0, hostDropped = 0;           // (under mu, by endBatch)
    uint64_t devRecords = 0, devSkipped = 0, devDropped = 0, devHandedBack = 0;
    // what a formatter thread gathers of one batch before it merges: a table of its own and what became of the records it walked
    struct Local : Slot { std::vector<uint64_t> words; uint64_t records = 0, skipped = 0, dropped = 0; };
    const char *name() const override { return "-oep"; }
    bool setup(const Args &a, const Genome &g, int nImages, int nContexts, std::string &err) override;      // -epq
    int  enable(const CtxAt &at) override;                                // (remembers the context for the end of the run)
    Slot *newSlot() const override;
    void add(const OutClump &oc, const Read &r, Slot *s) override;        // one record printClump was called for
    void endBatch(Slot *s) override;                                      // ... and the batch's share into the run's table; clears the slot
    bool finish(FILE *mainOut, FILE *log, bool timing) override;          // every enabled context's table, then the file
    void stats(std::string &line) const override;
    static bool deviceEntryPoints();                                      // does this build have ygpu_eprofile_*?
    bool write(const char *path, std::string &err) const;                 // path "stdout" = standard output
  private:
    const Genome *genome = nullptr; std::string file; std::vector<CtxAt> enabled;
};

// ---- SNV calls with genotypes (-osnv; snv.cpp, ../snv_core.h) ---------------------------------------------------------------------------------------------------
// The seventh side output counts nothing itself: it judges the run's pileup -- the -opu track's when that option is given (`shared`: this kind's hooks then do
// nothing, and the pileup's table has been written when finish runs), otherwise a PileupTrack of its own that writes no file and that every hook is handed on
// to.  One device array per image, the host's blocks counted once.  finish folds every source into ONE image's array -- the first image with a feeder: the
// host's blocks, then every other image's rows at the union of all sources' candidates (ygpu_pileup_add) --, selects the calls there (ygpu_snv_call_size /
// ygpu_snv_collect) and writes the VCF.  A run over N images so moves roughly what -opu moves.  Without the entry points (the CPU tier's test doubles), without a
// feeder, with YAHA_HOST_SNV=1 or when the selection fails before anything was folded, ysnv's routine runs on the host over the union of the sources
// (PileupTrack::unionRows); when it fails after every fold was done, over the one image's candidates.  A fold that fails half-way leaves an array nobody can
// read any more: the run fails.
struct SnvTrack : SideOutput {
    explicit SnvTrack(PileupTrack *sharedPileup) : shared(sharedPileup) {}
    const char *name() const override { return "-osnv"; }
    bool setup(const Args &a, const Genome &g, int nImages, int nContexts, std::string &err) override;
    int  enable(const CtxAt &at) override { return own ? own->enable(at) : YGPU_ENODEV; }
    int  beforeFilter(const CtxAt &at, size_t n) override { return own ? own->beforeFilter(at, n) : 0; }
    void add(const OutClump &oc, const Read &r, Slot *s) override { if (own) own->add(oc, r, s); }
    bool finish(FILE *mainOut, FILE *log, bool timing) override;
    void stats(std::string &line) const override;
    static bool deviceEntryPoints();                                      // does this build have ygpu_pileup_add and ygpu_snv_*?
    PileupTrack *pileup() const { return shared ? shared : own.get(); }   // the array it judges (after setup)
    std::vector<ygpu_snv_call> calls;                                     // what the writer prints, ascending (made by finish)
    uint64_t nHet = 0, nHom = 0, foldedSlots = 0; bool onDevice = false;
    bool write(const char *path, std::string &err) const;                 // path "stdout" = standard output
  private:
    int  callOnDevice(PileupTrack &pu, ygpu_ctx *const *feeders, int n, int *folded, std::string &err);      // *folded: 0 nothing, 1 every source, 2 half-way
    int  callOnHost(PileupTrack &pu, ygpu_ctx *const *feeders, int n, bool withHost, std::string &err);
    PileupTrack *shared; std::unique_ptr<PileupTrack> own; const Genome *genome = nullptr; std::string file, options; ygpu_snv_params P{};
    double msFold = 0, msSelect = 0, msWrite = 0;
};

// ---- indel calls with genotypes (-oindel; indelcalls.cpp, ../indelcall_core.h) ---------------------------------------------------------------------------------
// The eighth side output counts nothing itself either: it takes the run's raw indel alleles -- the -oid track's when that runs with -idlen 1 and -idq = -puq,
// otherwise a quiet IndelTrack the run driver lists before it -- and the run's pileup -- the -opu track's, failing that the one -osnv made, failing that a quiet
// PileupTrack listed before it.  finish runs after theirs.  On the home image, the first with a feeder: the alleles are normalised and merged
// (ygpu_indelcall_normalize); what the array lacks is folded in (PileupTrack::foldOnce: the host's rows, and with several images the others' rows at the anchor
// slots, which the merged alleles are fetched for); the calls are selected and collected (ygpu_indelcall_size / _collect).  Without the entry points (the CPU
// tier's test doubles), without a feeder, with YAHA_HOST_INDELCALL=1 or when the device step fails before any fold the same core runs on the host over
// PileupTrack::rowsAt; a fold that failed half-way fails the run.
struct IndelCallTrack : SideOutput {
    IndelCallTrack(PileupTrack *pileupTrack, SnvTrack *snvTrack, IndelTrack *indelTrack) : puGiven(pileupTrack), snv(snvTrack), id(indelTrack) {}
    const char *name() const override { return "-oindel"; }
    bool setup(const Args &a, const Genome &g, int nImages, int nContexts, std::string &err) override;
    bool finish(FILE *mainOut, FILE *log, bool timing) override;
    void stats(std::string &line) const override;
    static bool deviceEntryPoints();                                      // does this build have ygpu_indelcall_* and the folds?
    std::vector<ygpu_indel_call> calls;                                   // what the writer prints, in keyLess order (made by finish)
    uint64_t nHet = 0, nHom = 0, nRaw = 0, nShifted = 0, nMerged = 0, nSkipped = 0, foldedSlots = 0; bool onDevice = false;
    bool write(const char *path, std::string &err) const;                 // path "stdout" = standard output
  private:
    int  callOnDevice(ygpu_ctx *const *feeders, int n, const std::vector<ygpu_indel_entry> &raw, bool *anyAdded, std::string &err);
    int  callOnHost(ygpu_ctx *const *feeders, int n, const std::vector<ygpu_indel_entry> &raw, std::string &err);
    PileupTrack *puGiven; SnvTrack *snv; IndelTrack *id; PileupTrack *pu = nullptr; const Genome *genome = nullptr; std::string file, options;
    ygpu_indelcall_params P{}; uint32_t maxShift = 256; bool foldBroke = false;      // (a fold that failed after it had added something)
    double msNorm = 0, msFold = 0, msSelect = 0, msWrite = 0;
};

// ---- the main output of a query run: where the formatted records of the batches go (sam.cpp: SAM / Blast8 text; bam.cpp: BAM, sorted BAM) -----------------
// What of a batch belongs to the main output: the device it ran on, its records as the formatter wrote them, as BGZF blocks (-obh / -obs) with the time their
// compression took, one entry per record in the order of the text (-obsort), the records written into the text
struct SinkBatch { int dev = 0; Text text, packed; double tPack = 0; std::vector<BamEntry> entries; uint64_t records = 0; };
// This one writes text: the header at the start, every batch's text with one call.  bam.cpp has the two others.
struct RecordSink {
    FILE *out = nullptr; std::string path;
    virtual ~RecordSink() {}
    bool open(const std::string &file, FILE *log);                        // "stdout" = standard output; unbuffered: whole batches are written with one call each
    virtual bool begin(const Args &a, const Genome &g, const std::string &samHeader, int nFormatters, FILE *log);      // the header; false: failed, with a line in log
    virtual std::vector<BamEntry> *entries(SinkBatch &) const { return nullptr; }      // where the formatter lists the batch's records, if the sink wants that
    virtual bool pack(SinkBatch &, int /*formatter*/, bool /*stopped*/, std::string &) { return true; }      // per batch by formatter thread 0 .. nFormatters - 1
    virtual bool write(SinkBatch &b, std::string &err);                   // per batch by the writer thread, in ticket order
    virtual void timingLine(const SinkBatch &, uint64_t /*ticket*/) const {}      // the sink's own YAHA_TIMING line of a batch written
    virtual bool finish(FILE *) { return true; }                          // after the last batch of a run that got there
    virtual void abandon() {}                                             // a run that failed: a sink that writes nothing before the end leaves no file behind
    bool close(bool stopped, FILE *log);                                  // flushes and closes; false: failed, with a line in log unless the run had stopped
    virtual void stats(std::string &) const {}                            // its keys of the stats line, each with its leading ", "
  protected:
    bool writeBytes(const Text &t, std::string &err);
};
std::unique_ptr<RecordSink> makeRecordSink(const Args &a);                // by -obh / -obs / -obsort

// ---- what the formatting of a batch works with (pipeline.cpp): filled by a formatter thread of the command line and by yaha_session_emit[_filtered] ---------
struct FormatCtx {
    const Args &args; const Genome &genome; const Read *reads;            // the batch's reads
    const std::vector<std::unique_ptr<SideOutput>> *outputs = nullptr; SideOutput::Slot *const *slots = nullptr; unsigned wantReads = 0;      // (mask: outputs with endRead)
    std::vector<BamEntry> *bamEntries = nullptr; uint64_t bamRecords = 0; // -obsort: the batch's list; -obh / -obs: records written into the text
};
// OQC/FBS filter + output text of one batch.  nt > 1: the reads of the batch are cut into nt contiguous ranges, one thread each (the ctypes/Session path, one
// batch at a time); the command line formats whole batches on a pool of threads instead and passes nt = 1.
void formatBatch(FormatCtx &f, const ygpu_result_batch *r, Text &text, int nt);
// ... of a batch whose post-filter ran on the device (ygpu_postfilter): the clumps arrive in print order with the filter's fields set.  onDevice: the side
// outputs the device stage did for the batch -- all but the reads it handed back unfiltered
void formatFiltered(FormatCtx &f, const ygpu_filtered_batch *r, Text &text, unsigned onDevice = 0);
}  // namespace yaha
namespace yoqc { struct Params; }
namespace yaha {
// the post-filter's parameters in the form oqc_core.h takes them (host and device stage); thr receives the break point table P points into
void oqcParamsFromArgs(const Args &a, yoqc::Params &P, std::vector<uint32_t> &thr);
// ... and in the form ygpu_set_postfilter takes them (p points into thr and seqs).  false: the run is not one the device stage takes -- OQC runs with break
// point costs that are a step function and -MNO of at least 1 only.  (-MNO below 1: the graph's successor test then also lets a node relax itself and nodes
// before it, which the device stage's one-successor-per-lane step does not order the way the sequential loop does, GraphPath.cpp:633-700)
bool postfilterParams(const Args &a, const SeqTable &seqs, std::vector<uint32_t> &thr, ygpu_postfilter_params *p);

// ---- whole-run driver (replacement of processQueryFile, Query.c:551-709) --------------------------------
int effectiveCpus();                                    // affinity mask and control-group CPU quota
int runQueries(Args &a, FILE *log);
int runIndex(Args &a, FILE *log);
int runCompress(Args &a, FILE *log);                     // -c: compressFile only (Main.c:572-577)
int runUncompress(Args &a, FILE *log);                   // -u: uncompressFile, Compress.c:337-397 (50 bases a line)
}  // namespace yaha

// ---- the session behind the C-ABI's yaha_session_* (session.cpp); a command-line run loads one as well ------------------------------------------------------
struct yaha_session {
    yaha::Args args; yaha::Genome genome; yaha::IndexFile index; yaha::ReadReader reader; std::string err, header; yaha::Text text;
    yaha::SeqTable seqs;                                                  // the genome's sequence table (load): what every yaha_session_*_params points into
    std::vector<uint32_t> pfThr;                                          // the break point table yaha_session_postfilter_params points into
    std::vector<yaha::Read> reads; std::vector<uint8_t> codes; std::vector<uint64_t> offsets;
    bool readerOpen = false;
    bool load();                                                          // genome, index, input, header; false with err
};
