// junctions.cpp -- the host's side of the split-read breakpoint calls (-obp): the junctions of the reads the device did not see, the run's list of junctions in
// read order, the clustering and the BEDPE writer.  What a junction is -- the eligible records of a read, their read-forward order, the two sides, the canonical
// form, the type -- is ../junction_core.h, the source the device stage compiles as well (device/junction_stage.h).
//
// The device entry points are WEAK references here, as depth.cpp's and events.cpp's are: the host stages are also linked against test doubles that do not have
// them (the CPU tier), and then -- as when the library refuses to enable the stage -- the host makes every junction itself.
#include "yaha_host.h"
#include "../junction_core.h"
#include <algorithm>
#include <tuple>

extern "C" {
__attribute__((weak)) int ygpu_junctions_enable(ygpu_ctx *ctx, const ygpu_junction_params *p);
__attribute__((weak)) int ygpu_junctions_size(ygpu_ctx *ctx, uint64_t *n);
__attribute__((weak)) int ygpu_junctions_collect(ygpu_ctx *ctx, ygpu_junction *out, uint64_t stats[4]);
}

namespace yaha {

bool JunctionTrack::setup(const Args &a, const Genome &g, int, int, std::string &)
{
    genome = &g; file = a.bpFileName; minMapq = (uint32_t)a.bpMinQ; window = (uint32_t)a.bpWindow; seqs.set(g); return true;
}

void JunctionTrack::beginBatch(Slot *s, bool onDevice) const
{
    Batch &b = *static_cast<Batch *>(s); b.host.clear(); b.hostReads = b.hostSkipped = 0;
    if (!onDevice) { b.dev.clear(); memset(b.devStats, 0, sizeof b.devStats); }
}

void JunctionTrack::endRead(const OutClump *recs, uint32_t n, const Read &r, uint32_t read, Slot *s) const
{
    if (n == 0) return;
    Batch &b = *static_cast<Batch *>(s); std::vector<ygpu_junction> &out = b.host; uint32_t skipped = 0;      // (skipped: records gated by MAPQ alone)
    const ydepth::Layout L = yjunc::layout(seqs.start.data(), seqs.length.data(), (uint32_t)seqs.start.size(), minMapq);
    if (yjunc::readJunctions(L, n, (uint32_t)r.len(), read,
        [recs](uint32_t k, const ygpu_clump **c, uint32_t *status, uint32_t *mq) { *c = &recs[k].c; *status = recs[k].status; *mq = recs[k].mapQuality; },
        [&out](const ygpu_junction &j) { out.push_back(j); }, &skipped)) b.hostReads++;
    b.hostSkipped += skipped;
}

void JunctionTrack::written(Slot *s)
{
    // (a read's junctions come from one side only, in ordinal order: merging by read keeps them together)
    const Batch &b = *static_cast<Batch *>(s); const size_t at = all.size(); all.resize(at + b.dev.size() + b.host.size());
    std::merge(b.dev.begin(), b.dev.end(), b.host.begin(), b.host.end(), all.begin() + at, [](const ygpu_junction &x, const ygpu_junction &y) { return x.read < y.read; });
    devReads += b.devStats[0]; devSkipped += b.devStats[2]; devHandedBack += b.devStats[3];
    hostReads += b.hostReads; hostSkipped += b.hostSkipped;
}

bool JunctionTrack::deviceEntryPoints() { return ygpu_junctions_enable != nullptr && ygpu_junctions_size != nullptr && ygpu_junctions_collect != nullptr; }

int JunctionTrack::enable(const CtxAt &at)
{
    if (!deviceEntryPoints() || getenv("YAHA_HOST_JUNCTIONS") != nullptr) return YGPU_ENODEV;
    ygpu_junction_params p; p.min_mapq = minMapq; seqs.into(p);
    const int rc = ygpu_junctions_enable(at.ctx, &p); return rc == YGPU_ENOMEM ? YGPU_ENODEV : rc;
}

int JunctionTrack::afterFilter(const CtxAt &at, Slot *s)
{
    Batch &b = *static_cast<Batch *>(s); b.dev.clear();
    uint64_t n = 0; int rc = ygpu_junctions_size(at.ctx, &n); if (rc != 0) return rc;
    b.dev.resize((size_t)n);
    return ygpu_junctions_collect(at.ctx, b.dev.data(), b.devStats);
}

// the run's junctions clustered and written
bool JunctionTrack::finish(FILE *mainOut, FILE *log, bool)
{
    std::string jerr; nJunctions = all.size();
    if (fflush(mainOut) != 0) return false;
    if (!write(file.c_str(), *genome, jerr)) { fprintf(log, "%s\n", jerr.c_str()); return false; }
    return true;
}

void JunctionTrack::stats(std::string &line) const
{
    char t[256]; snprintf(t, sizeof t, ", \"bp_device_reads\": %llu, \"bp_host_reads\": %llu, \"bp_junctions\": %llu, \"bp_clusters\": %llu", (unsigned long long)devReads,
        (unsigned long long)hostReads, (unsigned long long)nJunctions, (unsigned long long)nClusters);
    line += t;
}

// Clusters: the junctions sorted by (seqA, strandA, seqB, strandB, posA, posB, qgap); in that order a junction joins the FIRST cluster, in creation order, of its
// (seqA, strandA, seqB, strandB) whose first member is within the window on both sides -- posA - first.posA <= W (positions ascend within a group) and
// |posB - first.posB| <= W -- or opens a new one.  Clusters whose first member lies more than W before the current posA can take no further member, so the
// search starts behind them: what is searched is a handful of clusters.  One line per cluster in creation order:
// chromA, least posA, largest posA + 1, chromB, least posB, largest posB + 1, type, members, strandA, strandB, least and largest qgap.
bool JunctionTrack::write(const char *path, const Genome &g, std::string &err)
{
    std::sort(all.begin(), all.end(), [](const ygpu_junction &a, const ygpu_junction &b) {                 // ('+' sorts before '-')
        return std::tie(a.seqA, a.strandA, a.seqB, a.strandB, a.posA, a.posB, a.qgap) < std::tie(b.seqA, b.strandA, b.seqB, b.strandB, b.posA, b.posB, b.qgap); });
    struct Cluster { ygpu_junction first; uint32_t minA, maxA, minB, maxB, n; int32_t minGap, maxGap; };
    std::vector<Cluster> cl; size_t group0 = 0, live0 = 0;                  // first cluster of the current group; first of them that can still take a member
    const int64_t W = window;
    for (const ygpu_junction &j : all) {
        if (group0 < cl.size()) { const ygpu_junction &f = cl[group0].first;
            if (f.seqA != j.seqA || f.strandA != j.strandA || f.seqB != j.seqB || f.strandB != j.strandB) group0 = live0 = cl.size(); }
        while (live0 < cl.size() && (int64_t)j.posA - (int64_t)cl[live0].first.posA > W) live0++;
        size_t k = live0;
        for (; k < cl.size(); k++) { const ygpu_junction &f = cl[k].first; const int64_t dB = (int64_t)j.posB - (int64_t)f.posB;
            if ((int64_t)j.posA - (int64_t)f.posA <= W && dB <= W && -dB <= W) break; }
        if (k == cl.size()) { cl.push_back(Cluster{j, j.posA, j.posA, j.posB, j.posB, 1u, j.qgap, j.qgap}); continue; }
        Cluster &c = cl[k]; c.n++;
        c.minA = std::min(c.minA, j.posA); c.maxA = std::max(c.maxA, j.posA); c.minB = std::min(c.minB, j.posB); c.maxB = std::max(c.maxB, j.posB);
        c.minGap = std::min(c.minGap, j.qgap); c.maxGap = std::max(c.maxGap, j.qgap);
    }
    nClusters = cl.size();
    FILE *f = strcmp(path, "stdout") == 0 ? stdout : fopen(path, "w");
    if (!f) { err = std::string("Failure to open the breakpoint file: ") + path + "."; return false; }
    static const char *const typeName[4] = {"DEL", "DUP", "INV", "TRA"};
    bool ok = true;
    for (size_t k = 0; k < cl.size() && ok; k++) {
        const Cluster &c = cl[k]; const ygpu_junction &j = c.first;
        if (j.seqA >= g.seqs.size() || j.seqB >= g.seqs.size() || j.type > 3) { err = "a junction names a sequence or a type that does not exist"; ok = false; break; }
        ok = fprintf(f, "%s\t%u\t%u\t%s\t%u\t%u\t%s\t%u\t%c\t%c\t%d\t%d\n", g.seqs[j.seqA].name.c_str(), c.minA, c.maxA + 1, g.seqs[j.seqB].name.c_str(), c.minB, c.maxB + 1,
            typeName[j.type], c.n, (char)j.strandA, (char)j.strandB, c.minGap, c.maxGap) > 0;
    }
    if (fflush(f) != 0 || ferror(f)) ok = false;
    if (f != stdout && fclose(f) != 0) ok = false;
    if (!ok && err.empty()) err = std::string("Failure writing the breakpoint file: ") + path + ".";
    return ok;
}
}  // namespace yaha
