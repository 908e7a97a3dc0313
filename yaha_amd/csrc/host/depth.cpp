// depth.cpp -- the host's side of the binned tracks (BinnedTrack: the array the formatter threads feed with the records the device did not count, the merge with
// the device's arrays at the end of the run, the shell of the writer) and of the first of them, the read-depth track (-ocov) with its bedGraph lines.  The walk
// of a record -- ops -> covered runs -> (bin, count) adds, the two-sequence drop, the MAPQ gate -- is ../depth_core.h, the source the device stage compiles as
// well (device/depth_stage.h).
//
// The device entry points are WEAK references here: the host stages are also linked against test doubles that do not have them (the CPU tier), and then --
// as when the library refuses to enable the stage -- the host counts every record itself.
#include "yaha_host.h"
#include <algorithm>

extern "C" {
__attribute__((weak)) int ygpu_depth_enable(ygpu_ctx *ctx, const ygpu_depth_params *p);
__attribute__((weak)) int ygpu_depth_size(ygpu_ctx *ctx, uint64_t *n_bins);
__attribute__((weak)) int ygpu_depth_collect(ygpu_ctx *ctx, uint32_t *bins, uint64_t stats[4]);
}

namespace yaha {

// ---- what the tracks share ------------------------------------------------------------------------------------------------------------------------------
bool BinnedTrack::init(const Genome &g, int binBases, int minQ, std::string &err)
{
    bin = (uint32_t)binBases; minMapq = (uint32_t)minQ;
    seqStart.clear(); seqLength.clear(); for (auto &sq : g.seqs) { seqStart.push_back(sq.start); seqLength.push_back(sq.length); }
    binBase.assign(seqStart.size() + 1, 0);
    if (binBases < 1 || !ydepth::layoutBins(seqLength.data(), (uint32_t)seqLength.size(), bin, binBase.data(), &nBins)) {
        err = std::string(names.binOpt) + ": the bins do not fit 32 bits"; return false; }
    return allocate(err);
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
DepthTrack::DepthTrack() : BinnedTrack({"-covbin", "-ocov", "coverage", "depth"}, 1, ygpu_depth_enable != nullptr, ygpu_depth_size, ygpu_depth_collect) {}

void DepthTrack::add(const OutClump &oc, const Read &)
{
    uint32_t *const c = data; const uint64_t n = nBins;
    countRecord(ydepth::walkClump(layout(), oc.c, oc.ops, oc.mapQuality, [c, n](uint32_t b, uint32_t k) { if (b < n) __atomic_fetch_add(c + b, k, __ATOMIC_RELAXED); }, nullptr));
}

int DepthTrack::deviceEnable(ygpu_ctx *ctx) const
{
    if (!deviceEntryPoints()) return YGPU_ENODEV;
    ygpu_depth_params p; p.bin = bin; p.min_mapq = minMapq; p.n_seqs = (uint32_t)seqStart.size(); p.seq_start = seqStart.data(); p.seq_length = seqLength.data();
    return ygpu_depth_enable(ctx, &p);
}

// bedGraph: name, start (0-based), end (exclusive), value; sequences in index order, empty bins left out.  A bin of one base: the integer depth, neighbouring
// bases of equal depth in one line.  Wider bins: one line a bin, covered bases / bases of the bin ("%.4f"; the last bin of a sequence may be shorter).
bool DepthTrack::writeLines(FILE *f, const Genome &g) const
{
    bool ok = true;
    for (size_t s = 0; s < g.seqs.size() && ok; s++) {
        const char *name = g.seqs[s].name.c_str(); const uint32_t len = seqLength[s]; const uint32_t *c = data + binBase[s];
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
