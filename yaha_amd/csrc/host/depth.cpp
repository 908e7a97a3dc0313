// depth.cpp -- the host's side of the read-depth track (-ocov): the coverage array the formatter threads feed with the records the device did not count, the
// merge with the device's arrays at the end of the run, and the bedGraph writer.  The walk of a record -- ops -> covered runs -> (bin, count) adds, the
// two-sequence drop, the MAPQ gate -- is ../depth_core.h, the source the device stage compiles as well (device/depth_stage.h).
//
// The device entry points are WEAK references here: the host stages are also linked against test doubles that do not have them (the CPU tier), and then --
// as when the library refuses to enable the stage -- the host counts every record itself.
#include "yaha_host.h"
#include "../depth_core.h"
#include <algorithm>

extern "C" {
__attribute__((weak)) int ygpu_depth_enable(ygpu_ctx *ctx, const ygpu_depth_params *p);
__attribute__((weak)) int ygpu_depth_size(ygpu_ctx *ctx, uint64_t *n_bins);
__attribute__((weak)) int ygpu_depth_collect(ygpu_ctx *ctx, uint32_t *bins, uint64_t stats[4]);
}

namespace yaha {

bool DepthTrack::init(const Genome &g, int binBases, int minQ, std::string &err)
{
    bin = (uint32_t)binBases; minMapq = (uint32_t)minQ;
    seqStart.clear(); seqLength.clear(); for (auto &sq : g.seqs) { seqStart.push_back(sq.start); seqLength.push_back(sq.length); }
    binBase.assign(seqStart.size() + 1, 0);
    if (binBases < 1 || !ydepth::layoutBins(seqLength.data(), (uint32_t)seqLength.size(), bin, binBase.data(), &nBins)) { err = "-covbin: the bins do not fit 32 bits";
        return false; }
    free(cov); cov = (uint32_t *)calloc(nBins ? nBins : 1, sizeof(uint32_t));      // (untouched pages stay unmapped: a sparse track costs what it covers)
    if (!cov) { char m[160]; snprintf(m, sizeof m, "-ocov: no host memory for %llu bins (%.2f GB)", (unsigned long long)nBins, 4.0 * nBins / 1e9); err = m; return false; }
    return true;
}

void DepthTrack::add(const OutClump &oc)
{
    const ydepth::Layout L{seqStart.data(), seqLength.data(), binBase.data(), (uint32_t)seqStart.size(), bin, minMapq};
    uint32_t *const c = cov; const uint64_t n = nBins;
    const int g = ydepth::walkClump(L, oc.c, oc.ops, oc.mapQuality, [c, n](uint32_t b, uint32_t k) { if (b < n) __atomic_fetch_add(c + b, k, __ATOMIC_RELAXED); }, nullptr);
    __atomic_fetch_add(g == ydepth::COUNTED ? &hostRecords : g == ydepth::SKIPPED_MAPQ ? &hostSkipped : &hostDropped, (uint64_t)1, __ATOMIC_RELAXED);
}

bool DepthTrack::deviceEntryPoints() { return ygpu_depth_enable != nullptr && ygpu_depth_size != nullptr && ygpu_depth_collect != nullptr; }

int DepthTrack::deviceEnable(ygpu_ctx *ctx) const
{
    if (!deviceEntryPoints()) return YGPU_ENODEV;
    ygpu_depth_params p; p.bin = bin; p.min_mapq = minMapq; p.n_seqs = (uint32_t)seqStart.size(); p.seq_start = seqStart.data(); p.seq_length = seqLength.data();
    return ygpu_depth_enable(ctx, &p);
}

int DepthTrack::deviceCollect(ygpu_ctx *ctx, std::string &err)
{
    if (!deviceEntryPoints()) return YGPU_ENODEV;
    uint64_t n = 0; int rc = ygpu_depth_size(ctx, &n);
    if (rc == 0 && n != nBins) { err = "the device's coverage array has another size than the host's"; return YGPU_EINTERNAL; }
    uint32_t *tmp = rc == 0 ? (uint32_t *)malloc((size_t)(n ? n : 1) * sizeof(uint32_t)) : nullptr;
    if (rc == 0 && !tmp) { err = "no host memory for the device's coverage array"; return YGPU_ENOMEM; }
    uint64_t st[4] = {0, 0, 0, 0};
    if (rc == 0) rc = ygpu_depth_collect(ctx, tmp, st);
    if (rc != 0) { err = ygpu_last_error(ctx); free(tmp); return rc; }
    for (uint64_t b = 0; b < n; b++) if (tmp[b]) cov[b] += tmp[b];          // (the run is over: no other thread adds any more)
    free(tmp);
    devRecords += st[0]; devSkipped += st[1]; devDropped += st[2]; devHandedBack += st[3];
    return 0;
}

uint64_t DepthTrack::coveredBases() const { uint64_t t = 0; for (uint64_t b = 0; b < nBins; b++) t += cov[b]; return t; }

// bedGraph: name, start (0-based), end (exclusive), value; sequences in index order, empty bins left out.  A bin of one base: the integer depth, neighbouring
// bases of equal depth in one line.  Wider bins: one line a bin, covered bases / bases of the bin ("%.4f"; the last bin of a sequence may be shorter).
bool DepthTrack::write(const char *path, const Genome &g, std::string &err) const
{
    FILE *f = strcmp(path, "stdout") == 0 ? stdout : fopen(path, "w");
    if (!f) { err = std::string("Failure to open the depth file: ") + path + "."; return false; }
    bool ok = true;
    for (size_t s = 0; s < g.seqs.size() && ok; s++) {
        const char *name = g.seqs[s].name.c_str(); const uint32_t len = seqLength[s]; const uint32_t *c = cov + binBase[s];
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
    if (fflush(f) != 0 || ferror(f)) ok = false;
    if (f != stdout && fclose(f) != 0) ok = false;
    if (!ok) err = std::string("Failure writing the depth file: ") + path + ".";
    return ok;
}
}  // namespace yaha
