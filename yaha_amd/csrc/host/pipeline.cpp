// pipeline.cpp -- the batching host that replaces the reference's per-read loop (Query.c:255-543) and its
// run driver (Query.c:551-709): read a batch of queries, hand it to the device hot path through the C-ABI
// (ygpu_upload / ygpu_run / ygpu_collect), post-filter and format on host threads, write in input order.
// With -gpus N one context per device is driven by its own host thread; batches are dealt round-robin and the
// output is re-ordered by batch ticket, so the text equals a `-t 1` run of the reference.
//
// The shape of the file: what a run writes is two lists made at the top -- the side outputs (SideOutput, yaha_host.h: one file each beside the alignments) and
// the main output (RecordSink) -- and nothing below that point knows a particular one.  Then the formatting of a batch (FormatCtx), the small types the stages
// share (StageQueue, ResBuf, Batch and its Pool, Warm: a device's start-up protocol, FilterSide: a context's post-filter thread), Context (one context's
// thread), Run (what the stages share, the stages as member functions) and runQueries, which is the list of a run's steps.
#include "yaha_host.h"
#include <cstring>
#include <cstdlib>
#include <thread>
#include <chrono>
#include <atomic>
#include <mutex>
#include <condition_variable>
#include <map>
#include <deque>
#include <memory>
#include <sys/stat.h>
#include <sched.h>

using namespace yaha;

namespace yaha {

// ---- what a run writes ------------------------------------------------------------------------------------------------------------------------------------------
// The side outputs the options ask for, in the order their files are written in and their keys stand in the stats line: the binned tracks (depth.cpp,
// events.cpp, pileup.cpp), the breakpoint calls (junctions.cpp), the indel alleles (indels.cpp), the error profile (eprofile.cpp), the SNV calls (snv.cpp: they
// judge the run's pileup -- the -opu track's if there is one, which has then written its table before them), the indel calls (indelcalls.cpp).  A new kind is
// one line here.
static std::vector<std::unique_ptr<SideOutput>> makeSideOutputs(const Args &a)
{
    std::vector<std::unique_ptr<SideOutput>> o;
    if (a.haveCov) o.emplace_back(new DepthTrack);
    if (a.haveEv) o.emplace_back(new EventsTrack);
    PileupTrack *pu = nullptr;
    if (a.havePu) o.emplace_back(pu = new PileupTrack);
    if (a.haveBp) o.emplace_back(new JunctionTrack);
    IndelTrack *id = nullptr;
    if (a.haveId) o.emplace_back(id = new IndelTrack);
    if (a.haveEp) o.emplace_back(new EProfileTrack);
    SnvTrack *snv = nullptr;
    if (a.haveSnv) o.emplace_back(snv = new SnvTrack(pu));
    // the indel calls stand on a pileup and on the run's indel alleles: the tracks above where the options gave them, otherwise quiet ones of their own, listed
    // before them so that their finish has run
    if (a.haveIndel) {
        PileupTrack *ipu = pu;
        if (!ipu && !snv) { o.emplace_back(ipu = new PileupTrack); ipu->quietFor = "-oindel"; }
        if (!id) { o.emplace_back(id = new IndelTrack); id->quietFor = "-oindel"; }
        o.emplace_back(new IndelCallTrack(ipu, snv, id));
    }
    return o;
}
// (the main output -- SAM / Blast8 text, BAM, sorted BAM -- is makeRecordSink's choice, bam.cpp)

// ---- the formatting of a batch ----------------------------------------------------------------------------------------------------------------------------------
// one record of read i: its text, and its share of every side output the device did not do it for
static inline void emitRecord(FormatCtx &f, uint32_t i, const OutClump &o, int primaryCount, Text &text, unsigned onDevice = 0)
{
    const Read &rd = f.reads[i];
    // (per record and hot: the choice of the record's layout stays a branch on the options)
    if (f.args.outputBAM) { BamEntry e; if (bamRecord(f.args, f.genome, rd, o, primaryCount, text, f.bamEntries ? &e : nullptr)) { f.bamRecords++;
        if (f.bamEntries) f.bamEntries->push_back(e); } }
    else printClump(f.args, f.genome, rd, o, primaryCount, text);
    if (f.outputs) for (size_t k = 0; k < f.outputs->size(); k++) if (!(onDevice >> k & 1u)) (*f.outputs)[k]->add(o, rd, f.slots[k]);
}
// ... and the records printed for read i as a whole, for the outputs that are made of those (mask: which of them)
static inline void endRead(FormatCtx &f, uint32_t i, const std::vector<OutClump> &oc, unsigned mask)
{
    if (mask) for (size_t k = 0; k < f.outputs->size(); k++) if (mask >> k & 1u) (*f.outputs)[k]->endRead(oc.data(), (uint32_t)oc.size(), f.reads[i], i, f.slots[k]);
}
static void formatRange(FormatCtx &f, const ygpu_result_batch *r, uint32_t i0, uint32_t i1, Text &text, std::vector<OutClump> &oc)
{
    for (uint32_t i = i0; i < i1; i++) {
        uint32_t c0 = r->clump_start[i], c1 = r->clump_start[i + 1]; int primaryCount = 0;
        postFilter(f.args, f.genome, f.reads[i], r->clumps + c0, c1 - c0, r->ops, oc, primaryCount);
        for (auto &o : oc) emitRecord(f, i, o, primaryCount, text);
        endRead(f, i, oc, f.wantReads);
    }
}
void formatFiltered(FormatCtx &f, const ygpu_filtered_batch *r, Text &text, unsigned onDevice)
{
    text.clear();
    const unsigned readsTo = f.wantReads & ~onDevice;                        // the outputs that want a read's records and did not get them on the device
    std::vector<ygpu_clump> raw; std::vector<OutClump> oc;
    for (uint32_t i = 0; i < r->n_reads; i++) {
        const uint32_t k0 = r->clump_start[i], k1 = r->clump_start[i + 1];
        if (k1 > k0 && r->clumps[k0].primaryCount == 0xFFFFu) {
            // a read the device left unfiltered (more clumps than its stage takes, device/oqc_stage.h): all its clumps in the hot path's order -- the host's filter, same routine
            raw.resize(k1 - k0); for (uint32_t k = k0; k < k1; k++) raw[k - k0] = r->clumps[k].c;
            int primaryCount = 0;
            postFilter(f.args, f.genome, f.reads[i], raw.data(), k1 - k0, r->ops, oc, primaryCount);
            for (auto &o : oc) emitRecord(f, i, o, primaryCount, text);
            endRead(f, i, oc, f.wantReads);
            continue;
        }
        if (readsTo) oc.clear();
        for (uint32_t k = k0; k < k1; k++) {
            const ygpu_out_clump &c = r->clumps[k];
            OutClump o; o.c = c.c; o.ops = r->ops + c.c.op_start; o.status = c.status; o.mapQuality = c.mapQuality; o.numSecondaries = c.numSecondaries;
                o.matchedPrimary = c.matchedPrimary;
            emitRecord(f, i, o, (int)c.primaryCount, text, onDevice);
            if (readsTo) oc.push_back(o);
        }
        endRead(f, i, oc, readsTo);
    }
}
void formatBatch(FormatCtx &f, const ygpu_result_batch *r, Text &text, int nt)
{
    const uint32_t n = r->n_reads;
    text.clear();
    // straight into the batch's text (its buffer is reused from batch to batch)
    if (nt <= 1 || n < 2 * (uint32_t)nt) { std::vector<OutClump> oc; formatRange(f, r, 0, n, text, oc); return; }
    std::vector<Text> parts(nt);
    auto work = [&](int t) { std::vector<OutClump> oc; formatRange(f, r, (uint32_t)((uint64_t)n * t / nt), (uint32_t)((uint64_t)n * (t + 1) / nt), parts[t], oc); };
    std::vector<std::thread> th;
    for (int t = 1; t < nt; t++) th.emplace_back(work, t);
    work(0); for (auto &x : th) x.join();
    size_t tot = 0; for (auto &p : parts) tot += p.len;
    text.room(tot); for (auto &p : parts) text.append(p.p, p.len);
}

namespace {
double now() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

// a bounded hand-over queue between pipeline stages
template <class T> struct StageQueue {
    std::mutex mu; std::condition_variable cvPush, cvPop; std::deque<T> q; size_t cap = 0; int producers = 0;
    void open(size_t c, int np) { cap = c; producers = np; }
    void push(T &&v) { std::unique_lock<std::mutex> lk(mu); cvPush.wait(lk, [&] { return q.size() < cap; }); q.push_back(std::move(v)); cvPop.notify_one(); }
    bool pop(T &v) { std::unique_lock<std::mutex> lk(mu); cvPop.wait(lk, [&] { return !q.empty() || producers == 0; }); if (q.empty()) return false; v = std::move(q.front());
        q.pop_front(); cvPush.notify_one(); return true; }
    void producerDone() { std::lock_guard<std::mutex> lk(mu); if (--producers == 0) cvPop.notify_all(); }
};

// Result storage of a batch: page-locked host memory (ygpu_host_alloc) the device copies into directly (ygpu_collect_into) -- no staging copy by the context
// thread, no copy out of the context afterwards (two passes over ~9 KB a read otherwise); plain memory when it cannot be locked.  Grows, never shrinks.
struct ResBuf {
    void *p = nullptr; size_t cap = 0; bool pinned = false;
    ~ResBuf() { drop(); }
    void drop() { if (p) { if (pinned) ygpu_host_free(p); else free(p); } p = nullptr; cap = 0; }
    bool ensure(size_t bytes)
    {
        if (bytes <= cap) return true;
        drop();
        const size_t c = bytes + bytes / 4 + 4096;
        p = ygpu_host_alloc(c); pinned = p != nullptr;
        if (!p) p = malloc(c);
        cap = p ? c : 0; return p != nullptr;
    }
};
// The batch object -- reads, codes, results, text, what the main output and every side output keep with it (slot k is output k's), all with their capacity --
// goes back to the pool the splitter takes from once it is written, so that the steady state allocates nothing and maps no new pages.
struct Batch { uint64_t ticket = 0; std::vector<Span> spans; std::vector<Read> reads; size_t nReads = 0; std::vector<uint8_t> codes; std::vector<uint64_t> offsets;
               ResBuf clumpStart, ops, clumps; uint64_t nClumps = 0, nOps = 0; bool filtered = false; unsigned onDevice = 0;
               SinkBatch main; std::vector<SideOutput::Slot *> slots;
               double tRead = 0, tDev = 0, tFmt = 0;
               ~Batch() { for (SideOutput::Slot *s : slots) delete s; } };
typedef std::unique_ptr<Batch> BatchP;
struct Pool {
    std::mutex mu; std::vector<BatchP> free; const std::vector<std::unique_ptr<SideOutput>> *outputs = nullptr;
    BatchP get()
    {
        { std::lock_guard<std::mutex> lk(mu); if (!free.empty()) { BatchP b = std::move(free.back()); free.pop_back(); return b; } }
        BatchP b(new Batch); for (auto &o : *outputs) b->slots.push_back(o->newSlot());
        return b;
    }
    void put(BatchP &&b) { std::lock_guard<std::mutex> lk(mu); free.push_back(std::move(b)); }
};

// The start-up protocol of one device's contexts.  ready: 0 = image not there yet, 1 = there, -1 = failed.
// A context's FIRST batch allocates its device buffers (a hundred hipMalloc calls, each of which waits for the device to go idle): first batches run one at a
// time (`first`) and hold back the other contexts' new batches meanwhile (firstRunning), instead of fighting their kernels for every allocation (0.6 s per
// context otherwise, measured).  The first context of a device to get to its first batch leads (claim): its first batch allocates its arenas, and what it then
// holds is the measure of what a context needs (footprint, profile).  The others wait for that measure BEFORE they take a batch, then go one at a time: a
// context that would start with less free memory than 0.9 of the measure is left out -- parked without ever holding a batch (round 4 took the batch first and
// pushed it back: a queue whose other consumers had already seen it empty and finished never delivered it, and the output ended early with exit code 0).  Its
// share of the device's memory budget goes back to the contexts that run (ygpu_park).
struct Warm {
    std::mutex mu, first; std::condition_variable cv; int firstRunning = 0; int ready = 0; uint64_t footprint = 0;
    bool claimed = false, measured = false, haveProfile = false; ygpu_arena_profile profile;
    void setReady(bool ok) { { std::lock_guard<std::mutex> lk(mu); ready = ok ? 1 : -1; } cv.notify_all(); }
    bool waitReady() { std::unique_lock<std::mutex> lk(mu); cv.wait(lk, [&] { return ready != 0; }); return ready == 1; }
    // true: the caller leads
    bool claimOrWait() { std::unique_lock<std::mutex> lk(mu); if (!claimed) { claimed = true; return true; } cv.wait(lk, [&] { return measured; }); return false; }
    void setMeasured() { { std::lock_guard<std::mutex> lk(mu); measured = true; } cv.notify_all(); }
    void holdOthers() { std::lock_guard<std::mutex> lk(mu); firstRunning++; }
    void releaseOthers() { { std::lock_guard<std::mutex> lk(mu); firstRunning--; } cv.notify_all(); }
    void waitForFirsts() { std::unique_lock<std::mutex> lk(mu); cv.wait(lk, [&] { return firstRunning == 0; }); }
};

// The post-filter of batch n runs on a thread of its own, on the SNAPSHOT the context's thread takes of the batch's results (ygpu_postfilter_snapshot), while
// that thread is already uploading and running batch n + 1: the stage is a chain of waits for a few slow reads -- 5 to 9 ms in which the device is nearly idle
// -- and behind the hot path it made every batch of the context that much longer (the command line's steady rate 0.85 of the hot path's, round 4).  A
// context's first batch keeps the sequential order (its arenas are measured after it).  YAHA_SERIAL_FILTER=1: every batch in the sequential order.
// This is the hand-over between the two threads: one batch at a time (busy), the thread made when the first batch is handed over.
struct FilterSide {
    std::mutex mu; std::condition_variable cv; BatchP b; double t0 = 0; bool busy = false, quit = false; std::thread th;
    template <class Loop> void hand(BatchP &&fb, double t, Loop loop)
    {
        { std::lock_guard<std::mutex> lk(mu); b = std::move(fb); t0 = t; busy = true; if (!th.joinable()) th = std::thread(loop); }
        cv.notify_all();
    }
    bool take(BatchP &fb, double &t) { std::unique_lock<std::mutex> lk(mu); cv.wait(lk, [&] { return quit || b; }); if (!b) return false; fb = std::move(b); t = t0; return true; }
    void done() { { std::lock_guard<std::mutex> lk(mu); busy = false; } cv.notify_all(); }
    void idle() { std::unique_lock<std::mutex> lk(mu); cv.wait(lk, [&] { return !busy; }); }
    void finish() { if (!th.joinable()) return; idle(); { std::lock_guard<std::mutex> lk(mu); quit = true; } cv.notify_all(); th.join(); }
};

// What the stages of a run share, and the stages.  Six of them, batches handed over through bounded queues, a ticket ordering the output (= the reference's
// -t 1 order):
//   splitter   (1 thread)          record boundaries of the memory-mapped / block-read input (memchr; reader.cpp) -- the only serial part;
//   parsers    (a few threads)     id, sequence, quality, codes and the skip rules of one batch of records;
//   contexts   (1 thread each)     upload, run the hot path, results by DMA into the batch's page-locked buffers (asleep while the device works): Context, below;
//   formatters                     OQC/FBS filter and output text of one whole batch each, into the batch's own text buffer;
//   writer     (1 thread)          batches in ticket order, one write each; the batch object then goes back to the pool the splitter takes from.
// The device never waits for parsing or formatting unless those stages as a whole are slower than it.  The first failure (a device error, a write
// error) stops the run: nothing after the last complete batch before it is written, and the exit code is 1.
struct Run {
    yaha_session &S; Args &A; FILE *const log; const bool timing, stats; const double tEnter;
    std::vector<std::unique_ptr<SideOutput>> outputs; unsigned wantReads = 0; std::unique_ptr<RecordSink> sink;
    // -gpus N devices x -ctx M contexts per device (default 3 -- four contexts of ~60 GB beside the image leave a later, heavier batch no memory to grow into: measured slower;
    // while one context's batch is in a latency-bound device stage the others' batches compute).  Contexts of one device share its index image.
    const int perDev, nDev, ngpu; int cpus = 0, nParse = 0, nFmt = 0; size_t maxReads = 0, maxBases = 0;
    ygpu_params P; ygpu_index_view V; std::vector<ygpu_ctx *> ctx; std::vector<int> devs, leadRc; bool deviceFilter = false; ygpu_postfilter_params PF; std::vector<uint32_t> pfThr;
    std::vector<std::unique_ptr<Warm>> warm; std::atomic<int> ctxUp{0}, parked{0}; double tCtxUp = 0;
    Pool pool; StageQueue<BatchP> parseQ, inQ, fmtQ, outQ;
    std::atomic<bool> stop{false}; std::atomic<int> rcAll{0}; std::atomic<uint64_t> ticketsIssued{0}, ticketsWritten{0};
    std::vector<std::atomic<uint64_t>> devReads;                            // reads each device took (the stats line: do all devices pull their weight?)
    // where a context thread's time goes, batches after a context's first (the stats line; microseconds): upload, run, waiting for the filter thread, snapshot; and the filter
    // thread's post-filter + collect
    std::atomic<uint64_t> usUpload{0}, usRun{0}, usWaitFilter{0}, usSnapshot{0}, usFilter{0}, usIdle{0}, nLater{0};
    uint64_t nWritten = 0, nFirst = 0; double tFirstOut = 0, tLastOut = 0, tDone = 0;      // (the writer's)

    Run(yaha_session &s, FILE *l) : S(s), A(s.args), log(l), timing(getenv("YAHA_TIMING") != nullptr), stats(timing || getenv("YAHA_STATS") != nullptr), tEnter(now()),
        perDev(std::max(1, s.args.ctxPerGpu)), nDev(std::max(1, s.args.gpus)), ngpu(nDev * perDev) {}
    void fail(const char *what) { if (!stop.exchange(true)) fprintf(log, "%s -- stopping; the output ends with the last batch completed before this one.\n", what); rcAll = 1; }
    void failInit(int device, int rc, const char *why) { char m[512]; snprintf(m, sizeof m, "ygpu_init(device %d) failed: %d %s", device, rc, why); fail(m); }
    bool load(); void sizePools(); bool buildOutputs(); void planDevices();
    void bringUpDevices(); void splitter(); void parser(); void formatter(int me); void writer();
    void runThreads(); void checkTickets(); void finishOutputs(); void tearDown(); void printStats();
};

// One context's thread.  Contexts are made by the threads that use them, all devices at once (an index image of 16.7 GB takes 0.65 s to reach a device; eight
// in a row would be five seconds), while the splitter and the parsers already work on the first batches.  The first context of a device uploads the image, the
// others share it.
// The post-filter (OQC, filter by similarity, mapping quality) runs on the device behind the hot path (ygpu_postfilter; the same routine as the host's,
// oqc_core.h): the results that cross PCIe and reach the formatters are the clumps that get printed.  The host filter remains for -OQC N (duplicate
// removal only), for break point costs that are no step function, and on request (-dpf N, YAHA_HOST_OQC=1).
struct Context {
    Run &R; const int d, image, dev, leadCtx; Warm &W; int rc0 = 0; bool first = true, lead = false; const bool overlapFilter; FilterSide F;
    unsigned onDevice = 0;                                                   // what the device stage does for this context's batches (Batch::onDevice)
    Context(Run &r, int d_) : R(r), d(d_), image(d_ / r.perDev), dev(r.devs[d_ / r.perDev]), leadCtx(d_ - d_ % r.perDev), W(*r.warm[d_ / r.perDev]),
        overlapFilter(r.deviceFilter && getenv("YAHA_SERIAL_FILTER") == nullptr) {}
    ygpu_ctx *c() const { return R.ctx[d]; }
    CtxAt at() const { return CtxAt{R.ctx[d], d, image, dev}; }
    void run();
  private:
    void bringUp(); bool startUp(std::unique_lock<std::mutex> &one); void park() { (void)ygpu_park(c()); R.parked++; }
    int hotPath(BatchP &b, ygpu_result_batch &res, double t0, bool &handedOver); int collectFiltered(Batch &fb, ygpu_result_batch &res);
    void deliver(BatchP &fb, int rc, const ygpu_result_batch &res, double t0); void filterLoop();
};

// the image (thread 0 brings the devices up for all), the post-filter's parameters, and every side output's stage on this context
void Context::bringUp()
{
    if (d == 0) { R.bringUpDevices(); for (int k = 0; k < R.nDev; k++) R.warm[k]->setReady(R.leadRc[k] == 0); }
    rc0 = W.waitReady() ? 0 : (R.leadRc[image] ? R.leadRc[image] : YGPU_ENODEV);
    if (rc0 == 0 && R.deviceFilter) rc0 = ygpu_set_postfilter(c(), &R.PF);
    // (the stages sit behind the device's post-filter: a run whose filter stays on the host leaves every output to the formatters)
    if (rc0 == 0 && R.deviceFilter) for (size_t k = 0; k < R.outputs.size(); k++) {
        const int rc = R.outputs[k]->enable(at());
        // the run stops here, before its first batch
        if (rc == YGPU_ENOMEM) { char m[640]; snprintf(m, sizeof m, "%s: %s", R.outputs[k]->name(), ygpu_last_error(c())); R.fail(m); }
        else if (rc == 0) onDevice |= 1u << k;
    }
    if (rc0 != 0) R.failInit(dev, rc0, c() ? ygpu_last_error(c()) : (d == leadCtx ? "" : "(the device's first context failed)"));
    if (++R.ctxUp == R.ngpu) { R.tCtxUp = now();
        if (R.timing) fprintf(stderr, "[yaha] %d device contexts up (index image on %d device%s) %.1f ms after start\n", R.ngpu, R.nDev, R.nDev > 1 ? "s" : "",
            R.tCtxUp - R.tEnter); }
}

// Before a context's first batch, with the device's `first` lock held from here on (Warm has the protocol).  false: the context is left out.
bool Context::startUp(std::unique_lock<std::mutex> &one)
{
    if (!lead) lead = W.claimOrWait();
    one.lock();
    // Does the device still have room for this context's arenas?  (~55 GB a context for 16 M bases of 1 kbp reads, ~75 GB for 10 kbp reads; squeezed into
    // what is left, a first batch of 10 kbp reads at -ctx 3 took 1.8 s, cut into ranges, with every other context waiting behind it.)
    bool roomy = false;                                                      // twice a context's arenas free: room to take them in one go AND for the others to grow theirs later
    if (!lead && W.footprint > 0 && rc0 == 0) {
        uint64_t fb = 0, tb = 0, mine = 0;
        const bool known = ygpu_memory(c(), &fb, &tb, &mine) == 0;
        roomy = known && (double)fb >= 2.0 * (double)W.footprint;
        if (known && (double)fb < 0.9 * (double)W.footprint) {
            if (R.timing || R.stats) fprintf(stderr, "[yaha] context %d left out: %.1f GB free on device %d, the first context's arenas hold %.1f GB\n", d, fb / 1e9, dev,
                W.footprint / 1e9);
            park(); return false;
        }
    }
    // The other contexts of the device get the leader's arenas in ONE go (ygpu_presize: its capacities after its first batch, its estimates) while the
    // device's running contexts are held back for those few milliseconds; their own first batch then runs like any later batch, beside the others'.
    // (Before: every context grew its hundred buffers during a first batch of its own, first batches ran one at a time and held the others back --
    // 64 + 106 + 158 ms for the first three batches of a run, a fourth context cost more at the start than it gained later.)
    // (Only while the device is roomy: presized to the brim -- four contexts of 60 GB beside a 17 GB image, three of 90 GB on 10 kbp reads -- a later batch
    // that needs a larger arena finds no memory and is cut into ranges: 319 k -> 290 k reads/s steady, 27.6 k -> 12.4 k on 10 kbp reads, measured.  A
    // context that starts in a tighter device grows its arenas during a first batch of its own, one at a time, as before.)
    if (!lead && rc0 == 0 && W.haveProfile && roomy && getenv("YAHA_NO_PRESIZE") == nullptr) {
        W.holdOthers();
        const double p0 = now(); const int prc = ygpu_presize(c(), &W.profile);
        W.releaseOthers();
        if (R.timing) fprintf(stderr, "[yaha] context %d: arenas presized from the device's first context in %.1f ms (rc %d)\n", d, now() - p0, prc);
        if (prc == YGPU_ENOMEM) { if (R.timing || R.stats) fprintf(stderr, "[yaha] context %d left out: no room for its arenas on device %d\n", d, dev);
            park(); return false; }
        if (prc == 0) { first = false; one.unlock(); }
    }
    return true;
}

// post-filter (of the snapshot, or of the context's last run) and its results into the batch's own buffers; the side outputs' hooks around the filter, for the
// outputs the device does for this batch
int Context::collectFiltered(Batch &fb, ygpu_result_batch &res)
{
    uint64_t nc = 0, no = 0; int rc = 0; const CtxAt me = at(); const size_t nOut = R.outputs.size();
    for (size_t k = 0; k < nOut && rc == 0; k++) if (fb.onDevice >> k & 1u) rc = R.outputs[k]->beforeFilter(me, fb.codes.size());
    if (rc == 0) rc = ygpu_postfilter(c());
    if (rc == 0) rc = ygpu_filtered_size(c(), &nc, &no);
    for (size_t k = nOut; k-- > 0 && rc == 0;) if (fb.onDevice >> k & 1u) rc = R.outputs[k]->afterFilter(me, fb.slots[k]);
    if (rc != 0) return rc;
    if (!fb.clumpStart.ensure(4 * (fb.nReads + 1)) || !fb.clumps.ensure(sizeof(ygpu_out_clump) * nc) || !fb.ops.ensure(4 * no)) return YGPU_ENOMEM;
    ygpu_filtered_batch fr; rc = ygpu_collect_filtered(c(), (uint32_t *)fb.clumpStart.p, (ygpu_out_clump *)fb.clumps.p, (uint32_t *)fb.ops.p, &fr);
    res.n_clumps = fr.n_clumps; res.n_ops = fr.n_ops; return rc;
}

void Context::deliver(BatchP &fb, int rc, const ygpu_result_batch &res, double t0)
{
    if (rc != 0) { char m[512];
        snprintf(m, sizeof m, "context %d: hot path failed (%d): %s", d, rc, rc == YGPU_ENOMEM && !fb->ops.p ? "host memory for the results" : ygpu_last_error(c()));
        R.fail(m); fb->nReads = 0; R.fmtQ.push(std::move(fb)); return; }
    fb->nClumps = res.n_clumps; fb->nOps = res.n_ops;
    fb->tDev = now() - t0; R.devReads[image] += fb->nReads;
    R.fmtQ.push(std::move(fb));
}

void Context::filterLoop()
{
    BatchP fb; double t0;
    while (F.take(fb, t0)) {
        ygpu_result_batch res; memset(&res, 0, sizeof res);
        const double f0 = now();
        const int rc = R.stop ? 0 : collectFiltered(*fb, res);
        R.usFilter += (uint64_t)((now() - f0) * 1e3);
        if (R.stop && rc == 0) { fb->nReads = 0; R.fmtQ.push(std::move(fb)); } else deliver(fb, rc, res, t0);
        F.done();
    }
}

// upload, run (+ post-filter), results straight into the batch's own buffers
int Context::hotPath(BatchP &b, ygpu_result_batch &res, double t0, bool &handedOver)
{
    ygpu_read_batch rb{(uint32_t)b->nReads, b->codes.data(), b->offsets.data()};
    const double h0 = now();
    // (the batch lives until it is printed: no wait for its bytes here)
    int rc = ygpu_upload_nowait(c(), &rb); const double h1 = now(); if (rc == 0) rc = ygpu_run(c()); if (rc != 0) return rc;
    const double h2 = now();
    uint64_t nc = 0, no = 0; b->filtered = R.deviceFilter; b->onDevice = R.deviceFilter ? onDevice : 0u;
    if (!first) { R.usUpload += (uint64_t)((h1 - h0) * 1e3); R.usRun += (uint64_t)((h2 - h1) * 1e3); R.nLater++; }
    if (R.deviceFilter && overlapFilter && !first) {                         // the filter thread takes it from here; this thread goes on with the next batch
        F.idle();
        const double h3 = now();
        if (R.stop) return 0;
        rc = ygpu_postfilter_snapshot(c()); if (rc != 0) return rc;
        R.usWaitFilter += (uint64_t)((h3 - h2) * 1e3); R.usSnapshot += (uint64_t)((now() - h3) * 1e3);
        F.hand(std::move(b), t0, [this] { filterLoop(); }); handedOver = true; return 0;
    }
    if (R.deviceFilter) {
        rc = collectFiltered(*b, res);
        if (R.timing && first) fprintf(stderr, "[yaha] context %d, first batch: upload %.1f  run %.1f  post-filter and collect %.1f ms\n", d, h1 - h0, h2 - h1, now() - h2);
        return rc;
    }
    rc = ygpu_result_size(c(), &nc, &no); if (rc != 0) return rc;
    if (!b->clumpStart.ensure(4 * (b->nReads + 1)) || !b->clumps.ensure(sizeof(ygpu_clump) * nc) || !b->ops.ensure(4 * no)) return YGPU_ENOMEM;
    return ygpu_collect_into(c(), (uint32_t *)b->clumpStart.p, (ygpu_clump *)b->clumps.p, (uint32_t *)b->ops.p, &res);
}

void Context::run()
{
    bringUp();
    BatchP b;
    for (;;) {
        std::unique_lock<std::mutex> one(W.first, std::defer_lock);
        if (first && !startUp(one)) break;                                   // (left out: before it takes a batch)
        const double w0 = now();
        if (!R.inQ.pop(b)) break;
        if (R.stop) { b->nReads = 0; R.fmtQ.push(std::move(b)); continue; }
        b->main.dev = dev;
        const double t0 = now(); if (!first) R.usIdle += (uint64_t)((t0 - w0) * 1e3);
        ygpu_result_batch res; memset(&res, 0, sizeof res); bool handedOver = false; int rc;
        if (first) {
            W.holdOthers();
            rc = hotPath(b, res, t0, handedOver); first = false;
            if (lead) {                                                      // the measure: what this context holds after its first batch (without the index image)
                uint64_t fb = 0, tb = 0, mine = 0; const ygpu_index_view &V = R.V;
                const uint64_t img = (uint64_t)V.n_base_bytes + 4ull * V.totalMatches + 4ull * ((1ull << (2 * V.wordLen)) + 1);
                if (rc == 0 && ygpu_memory(c(), &fb, &tb, &mine) == 0) W.footprint = std::max<uint64_t>(1, d == leadCtx && mine > img ? mine - img : mine);
                if (rc == 0 && ygpu_get_arena_profile(c(), &W.profile) == 0) W.haveProfile = true;
            }
            W.releaseOthers();
            one.unlock();
            if (lead) W.setMeasured();
        } else {
            W.waitForFirsts();
            rc = hotPath(b, res, t0, handedOver);
        }
        if (!handedOver) deliver(b, rc, res, t0);
    }
    if (lead) W.setMeasured();                                               // (a leader that never saw a batch: the others must not wait for its measure)
    F.finish();
    R.fmtQ.producerDone();
}

// ---- the steps of a run ---------------------------------------------------------------------------------------------------------------------------------------
bool Run::load()
{
    if (!S.load()) { fprintf(log, "%s\n", S.err.c_str()); return false; }
    if (timing) fprintf(stderr, "[yaha] index and input opened in %.1f ms\n", now() - tEnter);
    return true;
}

// Thread counts follow the CPUs the process may use (effectiveCpus: affinity and the control group's quota).  -t is the reference's thread count and is
// echoed in @PG; given explicitly (> 1) it is the number of formatter threads, otherwise every CPU that is not a parser, the splitter or the writer is one.
void Run::sizePools()
{
    cpus = effectiveCpus();
    // (a parser thread does 1.4 M reads/s, a formatter 0.1 M with the host's post-filter and 0.65 M when the filter ran on the device: with several devices
    // behind a small CPU quota the parsers are what must not run short -- one for every two devices)
    nParse = std::max(1, std::min(8, std::min(std::max((cpus + 7) / 10, (nDev + 1) / 2), std::max(1, cpus / 3))));
    nFmt = A.numThreads > 1 ? A.numThreads : std::max(1, cpus - nParse - 2);
    parseQ.open((size_t)nParse + 2, 1); inQ.open((size_t)ngpu + 2, nParse); fmtQ.open((size_t)nFmt + (size_t)ngpu, ngpu + nParse); outQ.open((size_t)nFmt + 4, nFmt);
    // batches follow the read length: about 16 M bases each (16 384 reads of 1 kbp, 1 600 of 10 kbp, 65 536 of 100 bp), unless -batch gives a read count
    maxReads = A.batchReads > 0 ? (size_t)A.batchReads : 65536; maxBases = A.batchReads > 0 ? ~(size_t)0 : ((size_t)16 << 20);
}

bool Run::buildOutputs()
{
    sink = makeRecordSink(A);
    if (!sink->open(A.ofileName, log)) return false;
    outputs = makeSideOutputs(A); pool.outputs = &outputs;
    for (size_t k = 0; k < outputs.size(); k++) {
        if (!outputs[k]->setup(A, S.genome, nDev, ngpu, S.err)) { fprintf(log, "%s\n", S.err.c_str()); return false; }
        if (outputs[k]->wantsReads()) wantReads |= 1u << k;
    }
    return sink->begin(A, S.genome, S.header, nFmt, log);
}

void Run::planDevices()
{
    paramsFromArgs(A, P); yaha_session_index_view(&S, &V);
    ctx.assign((size_t)ngpu, nullptr); leadRc.assign((size_t)nDev, 0);
    deviceFilter = postfilterParams(A, S.seqs, pfThr, &PF) && A.devicePostFilter && getenv("YAHA_HOST_OQC") == nullptr;
    for (int k = 0; k < nDev; k++) warm.emplace_back(new Warm);
    devReads = std::vector<std::atomic<uint64_t>>((size_t)nDev); for (auto &x : devReads) x = 0;
    // logical GPU k of -gpus N is HIP device -device + k, or the k-th entry of YAHA_DEVICES (a comma-separated list; the same device may appear twice: two
    // images on one device, which is how the multi-device path is exercised on a box with one GPU)
    devs.resize((size_t)nDev); for (int k = 0; k < nDev; k++) devs[k] = A.device + k;
    if (const char *e = getenv("YAHA_DEVICES")) { int k = 0; for (const char *q = e; *q && k < nDev; k++) { devs[k] = atoi(q); while (*q && *q != ',') q++; if (*q == ',') q++; } }
}

// The index image reaches the devices through ONE call (ygpu_init_multi): the first device takes it from the host, the others from their neighbour over xGMI,
// piece by piece -- the reference maps its index once for all threads (Query.c:565-626); N uploads of 16.7 GB at once would share the host's memory instead.
void Run::bringUpDevices()
{
    const int rc = ygpu_init_multi(devs.data(), nDev, perDev, &V, &P, ctx.data(), leadRc.data());      // ctx[k * perDev + j] = context j of device k
    for (int k = 0; k < nDev; k++) if (rc != 0 && !ctx[k * perDev]) leadRc[k] = rc;
    // (the device that failed is reported before the ones that were merely not started because of it)
    if (rc != 0) for (int k = 0; k < nDev; k++) { ygpu_ctx *c = ctx[k * perDev];
        if (leadRc[k] != 0 && c && strncmp(ygpu_last_error(c), "not started", 11) != 0) { failInit(devs[k], leadRc[k], ygpu_last_error(c)); break; } }
}

void Run::splitter()
{
    uint64_t ticket = 0;
    while (!stop) {
        BatchP b = pool.get();
        if (S.reader.split.nextSpans(maxReads, maxBases, b->spans) == 0) break;
        b->ticket = ticket++; ticketsIssued = ticket;
        parseQ.push(std::move(b));
    }
    parseQ.producerDone();
}

void Run::parser()
{
    BatchP b;
    while (parseQ.pop(b)) {
        b->nReads = 0;
        if (!stop) {
            const double t0 = now();
            if (b->reads.size() < b->spans.size()) b->reads.resize(b->spans.size());      // Read objects keep their strings' capacity from batch to batch
            b->offsets.assign(1, 0); size_t bases = 0, k = 0;
            for (auto &sp : b->spans) if (parseSpan(sp, S.reader.fastq, S.reader.maxQueryLength, S.reader.wordLen, b->reads[k])) { bases += b->reads[k].fwdCodes.size(); k++; }
            b->nReads = k; b->codes.resize(bases); size_t o = 0;
            for (size_t i = 0; i < k; i++) { const Read &rd = b->reads[i]; memcpy(b->codes.data() + o, rd.fwdCodes.data(), rd.fwdCodes.size()); o += rd.fwdCodes.size();
                b->offsets.push_back(o); }
            b->tRead = now() - t0;
        }
        b->spans.clear();                                                  // lets go of the input chunk
        // a batch whose records were all skipped still takes its place in the output order
        if (b->nReads == 0) { b->nClumps = b->nOps = 0; fmtQ.push(std::move(b)); } else inQ.push(std::move(b));
    }
    inQ.producerDone(); fmtQ.producerDone();
}

void Run::formatter(int me)
{
    BatchP b;
    while (fmtQ.pop(b)) {
        const double t0 = now(); SinkBatch &m = b->main; m.text.clear(); m.entries.clear();
        if (!(b->nReads && b->filtered)) b->onDevice = 0;                    // (a batch that failed, or without reads: what its slots hold of the device's is a former batch's)
        for (size_t k = 0; k < outputs.size(); k++) outputs[k]->beginBatch(b->slots[k], (b->onDevice >> k & 1u) != 0);
        FormatCtx f{A, S.genome, b->reads.data(), &outputs, b->slots.data(), wantReads, sink->entries(m)};
        if (!stop && b->nReads && b->filtered) {
            ygpu_filtered_batch fr; memset(&fr, 0, sizeof fr);
            fr.n_reads = (uint32_t)b->nReads; fr.clump_start = (const uint32_t *)b->clumpStart.p; fr.clumps = (const ygpu_out_clump *)b->clumps.p;
                fr.ops = (const uint32_t *)b->ops.p; fr.n_clumps = b->nClumps; fr.n_ops = b->nOps;
            formatFiltered(f, &fr, m.text, b->onDevice);
        } else if (!stop && b->nReads) {
            ygpu_result_batch res; memset(&res, 0, sizeof res);
            res.n_reads = (uint32_t)b->nReads; res.clump_start = (const uint32_t *)b->clumpStart.p; res.clumps = (const ygpu_clump *)b->clumps.p;
                res.ops = (const uint32_t *)b->ops.p; res.n_clumps = b->nClumps; res.n_ops = b->nOps;
            formatBatch(f, &res, m.text, 1);
        }
        for (size_t k = 0; k < outputs.size(); k++) outputs[k]->endBatch(b->slots[k]);
        m.records = f.bamRecords; b->tFmt = now() - t0;
        std::string err; if (!sink->pack(m, me, stop, err)) fail(err.c_str());
        m.tPack = now() - t0 - b->tFmt;
        outQ.push(std::move(b));
    }
    outQ.producerDone();
}

void Run::writer()
{
    std::map<uint64_t, BatchP> done; uint64_t nextOut = 0; BatchP b;
    while (outQ.pop(b)) {
        done[b->ticket] = std::move(b);
        while (!done.empty() && done.begin()->first == nextOut) {
            BatchP w = std::move(done.begin()->second); done.erase(done.begin()); nextOut++; ticketsWritten = nextOut;
            if (!stop) {
                std::string err;
                if (!sink->write(w->main, err)) fail(err.c_str());
                else { const double t = now(); if (nWritten == 0) { tFirstOut = t; nFirst = w->nReads; } tLastOut = t; nWritten += w->nReads; }
                if (w->nReads) for (size_t k = 0; k < outputs.size(); k++) outputs[k]->written(w->slots[k]);
                if (timing) { fprintf(stderr, "[yaha] ticket %llu: %zu reads  parse %.1f  device (upload, run, collect) %.1f  format %.1f ms  written at %.1f\n",
                    (unsigned long long)w->ticket, w->nReads, w->tRead, w->tDev, w->tFmt, now() - tEnter); sink->timingLine(w->main, w->ticket); }
            }
            pool.put(std::move(w));
        }
    }
}

void Run::runThreads()
{
    if (timing) fprintf(stderr, "[yaha] %d usable CPUs: %d parser, %d formatter threads, %d contexts\n", cpus, nParse, nFmt, ngpu);
    std::vector<std::unique_ptr<Context>> contexts; for (int d = 0; d < ngpu; d++) contexts.emplace_back(new Context(*this, d));
    std::vector<std::thread> th;
    for (auto &c : contexts) th.emplace_back([&c] { c->run(); });           // the index image starts towards the devices first
    th.emplace_back([this] { splitter(); });
    for (int i = 0; i < nParse; i++) th.emplace_back([this] { parser(); });
    for (int i = 0; i < nFmt; i++) th.emplace_back([this, i] { formatter(i); });
    th.emplace_back([this] { writer(); });
    for (auto &x : th) x.join();
    tDone = now();
}

// every batch the splitter cut must have reached the writer, in order: a batch lost between two stages would otherwise be a shorter output with exit code 0
void Run::checkTickets()
{
    if (!stop && ticketsWritten.load() != ticketsIssued.load()) {
        fprintf(log, "internal error: %llu of %llu batches were written -- the output is incomplete.\n", (unsigned long long)ticketsWritten.load(),
        (unsigned long long)ticketsIssued.load()); rcAll = 1; }
}

// the end of a run that got there: the main output's, then every side output's file in the list's order, each after the last alignment
void Run::finishOutputs()
{
    if (!stop && rcAll == 0 && !sink->finish(log)) rcAll = 1;
    for (auto &o : outputs) if (!stop && rcAll == 0 && !o->finish(sink->out, log, timing)) rcAll = 1;
}

// The command line (csrc/main.cpp) leaves right after runQueries: it sets YAHA_FAST_EXIT and lets the process exit release the device memory and the
// page-locked buffers in one go, instead of a hipFree per buffer (a second of waiting at the end of every run, measured).  Library users get the orderly path.
void Run::tearDown()
{
    const bool fastExit = getenv("YAHA_FAST_EXIT") != nullptr;
    if (!fastExit) for (int d = ngpu - 1; d >= 0; d--) if (ctx[d]) ygpu_destroy(ctx[d]);     // clones before their parents
    // (the batches -- a million small strings, the page-locked buffers -- go with the process as well: freeing them one by one was 0.3 s)
    if (fastExit) (void)new std::vector<BatchP>(std::move(pool.free));
    if (rcAll != 0) sink->abandon();
    if (!sink->close(stop, log)) rcAll = 1;
    if (timing) fprintf(stderr, "[yaha] batches done %.1f ms after start, teardown %.1f ms\n", tDone - tEnter, now() - tDone);
}

// one line for scripts (bench.py): steady = reads written after the first batch / time from the first batch's write to the last one's
void Run::printStats()
{
    const double steady = (nWritten > nFirst && tLastOut > tFirstOut) ? (nWritten - nFirst) / ((tLastOut - tFirstOut) * 1e-3) : 0.0;
    std::string per = "[", more;
    for (int k = 0; k < nDev; k++) { char t[32]; snprintf(t, sizeof t, "%s%llu", k ? ", " : "", (unsigned long long)devReads[k].load()); per += t; }
    per += "]";
    for (auto &o : outputs) o->stats(more);
    sink->stats(more);
    const double n = (double)std::max<uint64_t>(1, nLater);
    fprintf(stderr, "[yaha] stats {\"reads\": %llu, \"contexts_up_ms\": %.1f, \"first_batch_written_ms\": %.1f, \"last_batch_written_ms\": %.1f, \"total_ms\": %.1f, "
        "\"steady_reads_per_s\": %.0f, \"cpus\": %d, \"formatters\": %d, \"parsers\": %d, \"gpus\": %d, \"ctx_per_gpu\": %d, \"ctx_left_out\": %d, "
        "\"reads_per_device\": %s, \"context_thread_ms_per_batch\": {\"wait_for_a_batch\": %.2f, \"upload\": %.2f, \"run\": %.2f, \"wait_for_filter_thread\": %.2f, "
        "\"snapshot\": %.2f}, \"filter_thread_ms_per_batch\": %.2f%s}\n",
            (unsigned long long)nWritten, tCtxUp - tEnter, tFirstOut - tEnter, tLastOut - tEnter, now() - tEnter, steady, cpus, nFmt, nParse, nDev, perDev, parked.load(),
                per.c_str(),
            usIdle / 1e3 / n, usUpload / 1e3 / n, usRun / 1e3 / n, usWaitFilter / 1e3 / n, usSnapshot / 1e3 / n, usFilter / 1e3 / n, more.c_str());
}
}  // namespace

int runQueries(Args &a, FILE *log)
{
    std::unique_ptr<yaha_session> S(new yaha_session); S->args = a;
    Run R(*S, log);
    if (!R.load()) return 1;
    R.sizePools();                                                           // (before the outputs: the main output is told the number of formatter threads)
    if (!R.buildOutputs()) return 1;
    R.planDevices();
    R.runThreads();                                                          // started, and joined
    R.checkTickets();
    R.finishOutputs();
    R.tearDown();
    if (R.stats) R.printStats();
    return R.rcAll;
}

// CPUs this process may really use: the smaller of the affinity mask and the control group's CPU quota (cpu.max; v1: cfs_quota/cfs_period).  A container that
// shows 256 hardware threads and has a quota of 16 CPUs is throttled -- every thread of it, the ones that feed the GPUs included, stopped for the rest of each
// 100 ms period -- as soon as more than 16 threads are busy: the pools below are sized from this number, not from hardware_concurrency().
int effectiveCpus()
{
    int n = (int)std::thread::hardware_concurrency(); if (n < 1) n = 1;
    cpu_set_t set; if (sched_getaffinity(0, sizeof set, &set) == 0) { const int c = CPU_COUNT(&set); if (c >= 1 && c < n) n = c; }
    long long quota = -1, period = -1;
    if (FILE *f = fopen("/sys/fs/cgroup/cpu.max", "r")) { char q[64] = ""; if (fscanf(f, "%63s %lld", q, &period) == 2 && strcmp(q, "max") != 0) quota = atoll(q); fclose(f); }
    else {
        if (FILE *f1 = fopen("/sys/fs/cgroup/cpu/cpu.cfs_quota_us", "r")) { if (fscanf(f1, "%lld", &quota) != 1) quota = -1; fclose(f1); }
        if (FILE *f2 = fopen("/sys/fs/cgroup/cpu/cpu.cfs_period_us", "r")) { if (fscanf(f2, "%lld", &period) != 1) period = -1; fclose(f2); }
    }
    if (quota > 0 && period > 0) { const int c = (int)((quota + period - 1) / period); if (c >= 1 && c < n) n = c; }
    if (const char *e = getenv("YAHA_CPUS")) { const int c = atoi(e); if (c >= 1) n = c; }
    return n;
}

// ---- the other runs of the command line: index creation, -c, -u --------------------------------------------------------------------------------------------
static bool fileNewerThan(const std::string &f1, const std::string &f2)      // FileHelpers.c:127-146
{
    struct stat s1, s2;
    if (stat(f1.c_str(), &s1) != 0) return false;
    if (stat(f2.c_str(), &s2) != 0) return true;
    return s1.st_mtime > s2.st_mtime;
}

int runIndex(Args &a, FILE *log)                                              // Main.c:587-628
{
    auto now = []() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
    const bool timing = getenv("YAHA_TIMING") != nullptr; double t0 = now();
    if (a.wordLen > 15) { fprintf(log, "Word Length (-L) for index creation is currently restricted to < 16.\n"); return 1; }
    if (a.skipDist < 1 || a.skipDist > a.wordLen) { fprintf(log, "Skip Distance (-S) for index creation must be between 1 and WordLength (inclusive).\n"); return 1; }
    size_t dot = a.gfileName.rfind('.'); std::string ext = dot == std::string::npos ? "" : a.gfileName.substr(dot);
    bool fasta = (ext == ".fna" || ext == ".fa" || ext == ".fasta");
    if (!fasta && ext != ".nib2") { fprintf(log, "Expecting a \".fa\", \".fna\", \".fasta\", or \".nib2\" genome file.\n"); return 1; }
    char oext[32]; snprintf(oext, sizeof oext, ".X%02d_%02d_%05dS", a.wordLen, a.skipDist, a.maxHits);
    std::string root = a.gfileName.substr(0, dot), nib2 = fasta ? root + ".nib2" : a.gfileName, xfile = root + oext, err;
    if (fasta) {
        if (fileNewerThan(a.gfileName, nib2)) {
            fprintf(log, "Compressing %s into %s.\n", a.gfileName.c_str(), nib2.c_str());
            std::vector<uint8_t> img;
            if (!compressFasta(a.gfileName.c_str(), img, err) || !writeFile(nib2.c_str(), img.data(), img.size(), err)) { fprintf(log, "%s\n", err.c_str()); return 1; }
            fprintf(log, "Finished compressing %s, now forming index.\n", nib2.c_str());
            if (timing) { fprintf(log, "[yaha] compress %.1f s\n", now() - t0); t0 = now(); }
        } else fprintf(log, "%s already exists.  Creating the index file.\n", nib2.c_str());
    }
    fprintf(log, "Creating index file %s.\n", xfile.c_str());
    Genome g; if (!loadNib2(nib2.c_str(), g, err)) { fprintf(log, "%s\n", err.c_str()); return 1; }
    IndexImage image;
    // count -> scan -> fill -> order -> sample on the GPU (device/index_build.hip) when there is one; the host
    // builder (the reference's three passes, formats.cpp) otherwise.  Both produce the reference's file byte for byte.
    bool onDevice = !a.cpuIndex && a.device >= 0 && getenv("YAHA_CPU_INDEX") == nullptr && visibleDevices() > a.device;
    if (onDevice) {
        fprintf(log, "Building the index on GPU %d.\n", a.device);
        if (!buildIndexDevice(a.device, g, a.wordLen, a.skipDist, a.maxHits, image, log, err)) {
            // (a shared or smaller device may lack the ~40 GB an hg18-scale build keeps resident: the host builder writes the same file, slower)
            fprintf(log, "Index build on the GPU failed (%s): building on the host instead.\n", err.c_str());
            image.release(); onDevice = false;
        }
    }
    if (!onDevice && !buildIndex(g, a.wordLen, a.skipDist, a.maxHits, image, log)) { fprintf(log, "Insufficient memory to build the index.\n"); return 1; }
    if (timing) { fprintf(log, "[yaha] index image (%.2f GB) built in %.1f s %s\n", image.words * 4 / 1e9, now() - t0, onDevice ? "on the GPU" : "on the host"); t0 = now(); }
    if (!writeFile(xfile.c_str(), image.p, image.words * 4, err)) { fprintf(log, "%s\n", err.c_str()); return 1; }
    if (timing) fprintf(log, "[yaha] index file written in %.1f s\n", now() - t0);
    fprintf(log, "Index %s created.\n", xfile.c_str());
    return 0;
}

int runCompress(Args &a, FILE *log)                                           // Main.c:572-577 -> compressFile
{
    std::string err; std::vector<uint8_t> img;
    if (!compressFasta(a.gfileName.c_str(), img, err) || !writeFile(a.ofileName.c_str(), img.data(), img.size(), err)) { fprintf(log, "%s\n", err.c_str()); return 1; }
    return 0;
}
int runUncompress(Args &a, FILE *log)                                         // uncompressFile, Compress.c:337-397
{
    std::string err; Genome g;
    if (!loadNib2(a.gfileName.c_str(), g, err)) { fprintf(log, "%s\n", err.c_str()); return 1; }
    if (a.verbose) fprintf(log, "Read in %zu reference sequences from %s.\n", g.seqs.size(), a.gfileName.c_str());
    std::string out; size_t tot = 0; for (auto &s : g.seqs) tot += s.name.size() + 2 + s.length + s.length / 50 + 1; out.reserve(tot + 16);
    for (auto &s : g.seqs) {
        out += '>'; out += s.name; out += '\n';
        int col = 0;
        for (uint32_t j = 0; j < s.length; j++) { if (col == 50) { out += '\n'; col = 0; } out += kFourBitChars[get4(g.bases, s.start + j)]; col++; }
        if (col != 0) out += '\n';
    }
    if (!writeFile(a.ofileName.c_str(), out.data(), out.size(), err)) { fprintf(log, "%s\n", err.c_str()); return 1; }
    return 0;
}
}  // namespace yaha
