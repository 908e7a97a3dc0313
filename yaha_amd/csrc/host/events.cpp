// events.cpp -- the host's side of the evidence track (-oev), a BinnedTrack (depth.cpp has what the tracks share: the array the formatter threads feed with
// the records the device did not count, the merge with the device's arrays at the end of the run, the shell of the writer).  What a record adds -- a mismatch
// or deleted base per reference base under R / D, one insertion per I, the two clipped ends, the two-sequence drop, the MAPQ gate -- is ../events_core.h, the
// source the device stage compiles as well (device/events_stage.h).
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

EventsTrack::EventsTrack() : BinnedTrack({"-evbin", "-oev", "evidence", "events", "YAHA_HOST_EVENTS",
    ", \"events_bins\": %llu, \"events_device_records\": %llu, \"events_host_records\": %llu, \"events_counted\": %llu"}, (uint32_t)yevents::NCH, ygpu_events_enable != nullptr,
    ygpu_events_size, ygpu_events_collect) {}

bool EventsTrack::setup(const Args &a, const Genome &g, int nImages, int nContexts, std::string &err)
{
    minClip = (uint32_t)a.evMinClip; return init(g, a.evFileName, a.evBin, a.evMinQ, nImages, nContexts, err);
}

void EventsTrack::add(const OutClump &oc, const Read &r, Slot *)
{
    uint32_t *const e = data; const uint64_t n = nBins;
    countRecord(yevents::walkClump(layout(), minClip, oc.c, oc.ops, (uint32_t)r.len(), oc.mapQuality,
        [e, n](uint32_t b, uint32_t ch, uint32_t k) { if (b < n && ch < (uint32_t)yevents::NCH) __atomic_fetch_add(e + (size_t)b * yevents::NCH + ch, k, __ATOMIC_RELAXED); }));
}

int EventsTrack::deviceEnable(ygpu_ctx *ctx) const
{
    if (!deviceEntryPoints()) return YGPU_ENODEV;
    ygpu_events_params p; p.bin = bin; p.min_mapq = minMapq; p.min_clip = minClip; seqs.into(p);
    return ygpu_events_enable(ctx, &p);
}

// A header line, then one line per bin in which any channel is non-zero: name, start (0-based), end (exclusive), the five counts; sequences and bins in index
// order, neighbouring bins are never merged (at a bin of one base either).
bool EventsTrack::writeLines(FILE *f, const Genome &g) const
{
    bool ok = fputs("#chrom\tstart\tend\tmismatch\tdeleted\tinsertion\tclip_left\tclip_right\n", f) >= 0;
    for (size_t s = 0; s < g.seqs.size() && ok; s++) {
        const char *name = g.seqs[s].name.c_str(); const uint32_t len = seqs.length[s], nb = binBase[s + 1] - binBase[s];
        const uint32_t *c = data + (size_t)binBase[s] * yevents::NCH;
        for (uint32_t b = 0; b < nb && ok; b++, c += yevents::NCH) if (c[0] | c[1] | c[2] | c[3] | c[4]) {
            const uint64_t lo = (uint64_t)b * bin, hi = std::min<uint64_t>(lo + bin, len);
            ok = fprintf(f, "%s\t%llu\t%llu\t%u\t%u\t%u\t%u\t%u\n", name, (unsigned long long)lo, (unsigned long long)hi, c[0], c[1], c[2], c[3], c[4]) > 0;
        }
    }
    return ok;
}
}  // namespace yaha
