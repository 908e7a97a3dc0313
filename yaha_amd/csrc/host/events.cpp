// events.cpp -- the host's side of the evidence track (-oev): the array the formatter threads feed with the records the device did not count, the merge with
// the device's arrays at the end of the run, and the writer.  What a record adds -- a mismatch or deleted base per reference base under R / D, one insertion per
// I, the two clipped ends, the two-sequence drop, the MAPQ gate -- is ../events_core.h, the source the device stage compiles as well (device/events_stage.h).
//
// The device entry points are WEAK references here, as depth.cpp's are: the host stages are also linked against test doubles that do not have them (the CPU
// tier), and then -- as when the library refuses to enable the stage -- the host counts every record itself.
#include "yaha_host.h"
#include "../events_core.h"
#include <algorithm>

extern "C" {
__attribute__((weak)) int ygpu_events_enable(ygpu_ctx *ctx, const ygpu_events_params *p);
__attribute__((weak)) int ygpu_events_size(ygpu_ctx *ctx, uint64_t *n_bins);
__attribute__((weak)) int ygpu_events_collect(ygpu_ctx *ctx, uint32_t *counts, uint64_t stats[4]);
}

namespace yaha {

bool EventsTrack::init(const Genome &g, int binBases, int minQ, int minClipBases, std::string &err)
{
    bin = (uint32_t)binBases; minMapq = (uint32_t)minQ; minClip = (uint32_t)minClipBases;
    seqStart.clear(); seqLength.clear(); for (auto &sq : g.seqs) { seqStart.push_back(sq.start); seqLength.push_back(sq.length); }
    binBase.assign(seqStart.size() + 1, 0);
    if (binBases < 1 || !ydepth::layoutBins(seqLength.data(), (uint32_t)seqLength.size(), bin, binBase.data(), &nBins)) { err = "-evbin: the bins do not fit 32 bits";
        return false; }
    free(ev); ev = (uint32_t *)calloc((nBins ? nBins : 1) * yevents::NCH, sizeof(uint32_t));      // (untouched pages stay unmapped: a sparse track costs what it holds)
    if (!ev) { char m[160]; snprintf(m, sizeof m, "-oev: no host memory for %llu bins (%.2f GB)", (unsigned long long)nBins, 4.0 * yevents::NCH * nBins / 1e9); err = m;
        return false; }
    return true;
}

void EventsTrack::add(const OutClump &oc, int qlen)
{
    const ydepth::Layout L{seqStart.data(), seqLength.data(), binBase.data(), (uint32_t)seqStart.size(), bin, minMapq};
    uint32_t *const e = ev; const uint64_t n = nBins;
    const int g = yevents::walkClump(L, minClip, oc.c, oc.ops, (uint32_t)qlen, oc.mapQuality,
        [e, n](uint32_t b, uint32_t ch, uint32_t k) { if (b < n && ch < (uint32_t)yevents::NCH) __atomic_fetch_add(e + (size_t)b * yevents::NCH + ch, k, __ATOMIC_RELAXED); });
    __atomic_fetch_add(g == ydepth::COUNTED ? &hostRecords : g == ydepth::SKIPPED_MAPQ ? &hostSkipped : &hostDropped, (uint64_t)1, __ATOMIC_RELAXED);
}

bool EventsTrack::deviceEntryPoints() { return ygpu_events_enable != nullptr && ygpu_events_size != nullptr && ygpu_events_collect != nullptr; }

int EventsTrack::deviceEnable(ygpu_ctx *ctx) const
{
    if (!deviceEntryPoints()) return YGPU_ENODEV;
    ygpu_events_params p; p.bin = bin; p.min_mapq = minMapq; p.min_clip = minClip; p.n_seqs = (uint32_t)seqStart.size(); p.seq_start = seqStart.data();
        p.seq_length = seqLength.data();
    return ygpu_events_enable(ctx, &p);
}

int EventsTrack::deviceCollect(ygpu_ctx *ctx, std::string &err)
{
    if (!deviceEntryPoints()) return YGPU_ENODEV;
    uint64_t n = 0; int rc = ygpu_events_size(ctx, &n);
    if (rc == 0 && n != nBins) { err = "the device's evidence array has another size than the host's"; return YGPU_EINTERNAL; }
    const uint64_t words = n * yevents::NCH;
    uint32_t *tmp = rc == 0 ? (uint32_t *)malloc((size_t)(words ? words : 1) * sizeof(uint32_t)) : nullptr;
    if (rc == 0 && !tmp) { err = "no host memory for the device's evidence array"; return YGPU_ENOMEM; }
    uint64_t st[4] = {0, 0, 0, 0};
    if (rc == 0) rc = ygpu_events_collect(ctx, tmp, st);
    if (rc != 0) { err = ygpu_last_error(ctx); free(tmp); return rc; }
    for (uint64_t w = 0; w < words; w++) if (tmp[w]) ev[w] += tmp[w];       // (the run is over: no other thread adds any more)
    free(tmp);
    devRecords += st[0]; devSkipped += st[1]; devDropped += st[2]; devHandedBack += st[3];
    return 0;
}

uint64_t EventsTrack::counted() const { uint64_t t = 0; for (uint64_t w = 0; w < nBins * yevents::NCH; w++) t += ev[w]; return t; }

// A header line, then one line per bin in which any channel is non-zero: name, start (0-based), end (exclusive), the five counts; sequences and bins in index
// order, neighbouring bins are never merged (at a bin of one base either).
bool EventsTrack::write(const char *path, const Genome &g, std::string &err) const
{
    FILE *f = strcmp(path, "stdout") == 0 ? stdout : fopen(path, "w");
    if (!f) { err = std::string("Failure to open the events file: ") + path + "."; return false; }
    bool ok = fputs("#chrom\tstart\tend\tmismatch\tdeleted\tinsertion\tclip_left\tclip_right\n", f) >= 0;
    for (size_t s = 0; s < g.seqs.size() && ok; s++) {
        const char *name = g.seqs[s].name.c_str(); const uint32_t len = seqLength[s], nb = binBase[s + 1] - binBase[s];
        const uint32_t *c = ev + (size_t)binBase[s] * yevents::NCH;
        for (uint32_t b = 0; b < nb && ok; b++, c += yevents::NCH) if (c[0] | c[1] | c[2] | c[3] | c[4]) {
            const uint64_t lo = (uint64_t)b * bin, hi = std::min<uint64_t>(lo + bin, len);
            ok = fprintf(f, "%s\t%llu\t%llu\t%u\t%u\t%u\t%u\t%u\n", name, (unsigned long long)lo, (unsigned long long)hi, c[0], c[1], c[2], c[3], c[4]) > 0;
        }
    }
    if (fflush(f) != 0 || ferror(f)) ok = false;
    if (f != stdout && fclose(f) != 0) ok = false;
    if (!ok) err = std::string("Failure writing the events file: ") + path + ".";
    return ok;
}
}  // namespace yaha
