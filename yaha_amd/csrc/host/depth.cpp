// depth.cpp -- the host's side of the binned tracks (BinnedTrack: the array the formatter threads feed with the records the device did not count, the merge with
// the device's arrays at the end of the run, the shell of the writer) and of the first of them, the read-depth track (-ocov) with its bedGraph lines.  The walk
// of a record -- ops -> covered runs -> (bin, count) adds, the two-sequence drop, the MAPQ gate -- is ../depth_core.h, the source the device stage compiles as
// well (device/depth_stage.h).
//
// The device entry points are WEAK references here: the host stages are also linked against test doubles that do not have them (the CPU tier), and then --
// as when the library refuses to enable the stage -- the host counts every record itself.
#include "yaha_host.h"
#include <algorithm>
#include <chrono>

extern "C" {
__attribute__((weak)) int ygpu_depth_enable(ygpu_ctx *ctx, const ygpu_depth_params *p);
__attribute__((weak)) int ygpu_depth_size(ygpu_ctx *ctx, uint64_t *n_bins);
__attribute__((weak)) int ygpu_depth_collect(ygpu_ctx *ctx, uint32_t *bins, uint64_t stats[4]);
}

namespace yaha {

// ---- what the tracks share ------------------------------------------------------------------------------------------------------------------------------
bool BinnedTrack::init(const Genome &g, const std::string &path, int binBases, int minQ, int nImages, int nContexts, std::string &err)
{
    genome = &g; file = path; bin = (uint32_t)binBases; minMapq = (uint32_t)minQ;
    ctxs.assign((size_t)nContexts, CtxAt{nullptr, 0, 0, 0}); feeder = std::vector<std::atomic<int>>((size_t)nImages); for (auto &x : feeder) x = 0;
    seqs.set(g); binBase.assign(seqs.start.size() + 1, 0);
    if (binBases < 1 || !ydepth::layoutBins(seqs.length.data(), (uint32_t)seqs.length.size(), bin, binBase.data(), &nBins)) {
        err = std::string(names.binOpt) + ": the bins do not fit 32 bits"; return false; }
    return allocate(err);
}

int BinnedTrack::enable(const CtxAt &at)
{
    if (getenv(names.hostSwitch) != nullptr) return YGPU_ENODEV;
    // (no room for the array beside the image and the arenas stops the run, with the sizes: a host array would hide that the device is full; larger bins are the way out)
    const int rc = deviceEnable(at.ctx); if (rc == 0) ctxs[at.index] = at;
    return rc;
}

int BinnedTrack::beforeFilter(const CtxAt &at, size_t)
{
    if (feeder[at.image].load(std::memory_order_relaxed) == 0) { int none = 0; feeder[at.image].compare_exchange_strong(none, at.index + 1); }
    return 0;
}

void BinnedTrack::feeders(std::vector<ygpu_ctx *> &ctx, std::vector<int> &dev) const
{
    ctx.clear(); dev.clear();
    for (auto &x : feeder) if (const int c1 = x.load()) { ctx.push_back(ctxs[c1 - 1].ctx); dev.push_back(ctxs[c1 - 1].device); }
}

// every image's array added to the host's, the file written after the last alignment
bool BinnedTrack::finish(FILE *mainOut, FILE *log, bool timing)
{
    auto now = []() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
    if (quietFor) return true;                                               // (its array is read where it lies, by the output it serves)
    std::string terr; bool ok = true; std::vector<ygpu_ctx *> feedCtx; std::vector<int> feedDev;
    feeders(feedCtx, feedDev);
    const double m0 = now();
    int failed = -1; const int rc = mergeDevices(feedCtx.data(), (int)feedCtx.size(), *genome, &failed, terr);
    const double m1 = now();
    if (rc != 0) { fprintf(log, "%s: collecting the %s array of device %d failed (%d): %s\n", names.fileOpt, names.array, failed >= 0 ? feedDev[failed] : -1, rc, terr.c_str());
        ok = false; }
    if (fflush(mainOut) != 0) ok = false;
    if (ok && !write(file.c_str(), *genome, terr)) { fprintf(log, "%s\n", terr.c_str()); ok = false; }
    if (timing) fprintf(stderr, "[yaha] %s: devices merged in %.1f ms%s, file written in %.1f ms\n", names.fileOpt, m1 - m0, mergeNote().c_str(), now() - m1);
    return ok;
}

void BinnedTrack::stats(std::string &line) const
{
    if (quietFor) return;
    char t[512]; snprintf(t, sizeof t, names.statsFmt, (unsigned long long)nBins, (unsigned long long)devRecords, (unsigned long long)hostRecords, (unsigned long long)sum());
    line += t; line += extraStats();
}

bool BinnedTrack::allocate(std::string &err)
{
    free(data); data = (uint32_t *)calloc((nBins ? nBins : 1) * channels, sizeof(uint32_t));      // (untouched pages stay unmapped: a sparse track costs what it holds)
    if (!data) { char m[160]; snprintf(m, sizeof m, "%s: no host memory for %llu bins (%.2f GB)", names.fileOpt, (unsigned long long)nBins, 4.0 * channels * nBins / 1e9);
        err = m; return false; }
    return true;
}

void BinnedTrack::countRecord(int gate)
{
    __atomic_fetch_add(gate == ydepth::COUNTED ? &hostRecords : gate == ydepth::SKIPPED_MAPQ ? &hostSkipped : &hostDropped, (uint64_t)1, __ATOMIC_RELAXED);
}

int BinnedTrack::deviceCollect(ygpu_ctx *ctx, std::string &err)
{
    if (!deviceEntryPoints()) return YGPU_ENODEV;
    uint64_t n = 0; int rc = devSize(ctx, &n);
    if (rc == 0 && n != nBins) { err = std::string("the device's ") + names.array + " array has another size than the host's"; return YGPU_EINTERNAL; }
    const uint64_t words = n * channels;
    uint32_t *tmp = rc == 0 ? (uint32_t *)malloc((size_t)(words ? words : 1) * sizeof(uint32_t)) : nullptr;
    if (rc == 0 && !tmp) { err = std::string("no host memory for the device's ") + names.array + " array"; return YGPU_ENOMEM; }
    uint64_t st[4] = {0, 0, 0, 0};
    if (rc == 0) rc = devCollect(ctx, tmp, st);
    if (rc != 0) { err = ygpu_last_error(ctx); free(tmp); return rc; }
    for (uint64_t w = 0; w < words; w++) if (tmp[w]) data[w] += tmp[w];     // (the run is over: no other thread adds any more)
    free(tmp);
    devRecords += st[0]; devSkipped += st[1]; devDropped += st[2]; devHandedBack += st[3];
    return 0;
}

int BinnedTrack::mergeDevices(ygpu_ctx *const *feeders, int n, const Genome &, int *failed, std::string &err)
{
    for (int k = 0; k < n; k++) { const int rc = deviceCollect(feeders[k], err); if (rc != 0) { *failed = k; return rc; } }
    return 0;
}

uint64_t BinnedTrack::sum() const { uint64_t t = 0; for (uint64_t w = 0; w < nBins * channels; w++) t += data[w]; return t; }

bool BinnedTrack::write(const char *path, const Genome &g, std::string &err) const
{
    FILE *f = strcmp(path, "stdout") == 0 ? stdout : fopen(path, "w");
    if (!f) { err = std::string("Failure to open the ") + names.file + " file: " + path + "."; return false; }
    bool ok = writeLines(f, g);
    if (fflush(f) != 0 || ferror(f)) ok = false;
    if (f != stdout && fclose(f) != 0) ok = false;
    if (!ok) err = std::string("Failure writing the ") + names.file + " file: " + path + ".";
    return ok;
}

// ---- read depth -----------------------------------------------------------------------------------------------------------------------------------------
DepthTrack::DepthTrack() : BinnedTrack({"-covbin", "-ocov", "coverage", "depth", "YAHA_HOST_DEPTH",
    ", \"depth_bins\": %llu, \"depth_device_records\": %llu, \"depth_host_records\": %llu, \"depth_covered_bases\": %llu"}, 1, ygpu_depth_enable != nullptr, ygpu_depth_size,
    ygpu_depth_collect) {}

bool DepthTrack::setup(const Args &a, const Genome &g, int nImages, int nContexts, std::string &err) { return init(g, a.covFileName, a.covBin, a.covMinQ, nImages, nContexts, err);
    }

void DepthTrack::add(const OutClump &oc, const Read &, Slot *)
{
    uint32_t *const c = data; const uint64_t n = nBins;
    countRecord(ydepth::walkClump(layout(), oc.c, oc.ops, oc.mapQuality, [c, n](uint32_t b, uint32_t k) { if (b < n) __atomic_fetch_add(c + b, k, __ATOMIC_RELAXED); }, nullptr));
}

int DepthTrack::deviceEnable(ygpu_ctx *ctx) const
{
    if (!deviceEntryPoints()) return YGPU_ENODEV;
    ygpu_depth_params p; p.bin = bin; p.min_mapq = minMapq; seqs.into(p);
    return ygpu_depth_enable(ctx, &p);
}

// bedGraph: name, start (0-based), end (exclusive), value; sequences in index order, empty bins left out.  A bin of one base: the integer depth, neighbouring
// bases of equal depth in one line.  Wider bins: one line a bin, covered bases / bases of the bin ("%.4f"; the last bin of a sequence may be shorter).
bool DepthTrack::writeLines(FILE *f, const Genome &g) const
{
    bool ok = true;
    for (size_t s = 0; s < g.seqs.size() && ok; s++) {
        const char *name = g.seqs[s].name.c_str(); const uint32_t len = seqs.length[s]; const uint32_t *c = data + binBase[s];
        if (bin == 1) {
            for (uint32_t i = 0; i < len && ok;) {
                if (!c[i]) { i++; continue; }
                uint32_t j = i + 1; while (j < len && c[j] == c[i]) j++;
                ok = fprintf(f, "%s\t%u\t%u\t%u\n", name, i, j, c[i]) > 0; i = j;
            }
        } else {
            const uint32_t nb = binBase[s + 1] - binBase[s];
            for (uint32_t b = 0; b < nb && ok; b++) if (c[b]) {
                const uint64_t lo = (uint64_t)b * bin, hi = std::min<uint64_t>(lo + bin, len);
                ok = fprintf(f, "%s\t%llu\t%llu\t%.4f\n", name, (unsigned long long)lo, (unsigned long long)hi, (double)c[b] / (double)(hi - lo)) > 0;
            }
        }
    }
    return ok;
}
}  // namespace yaha
