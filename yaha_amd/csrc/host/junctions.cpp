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

void JunctionTrack::init(const Genome &g, int minQ, int w)
{
    minMapq = (uint32_t)minQ; window = (uint32_t)w;
    seqStart.clear(); seqLength.clear(); for (auto &sq : g.seqs) { seqStart.push_back(sq.start); seqLength.push_back(sq.length); }
}

uint32_t JunctionTrack::addRead(const OutClump *recs, uint32_t n, int qlen, uint32_t read, std::vector<ygpu_junction> &out, uint32_t *skipped) const
{
    if (skipped) *skipped = 0;
    if (n == 0) return 0;
    const ydepth::Layout L = yjunc::layout(seqStart.data(), seqLength.data(), (uint32_t)seqStart.size(), minMapq);
    return yjunc::readJunctions(L, n, (uint32_t)qlen, read,
        [recs](uint32_t k, const ygpu_clump **c, uint32_t *status, uint32_t *mq) { *c = &recs[k].c; *status = recs[k].status; *mq = recs[k].mapQuality; },
        [&out](const ygpu_junction &j) { out.push_back(j); }, skipped);
}

void JunctionTrack::addBatch(const ygpu_junction *dev, size_t nDev, const uint64_t devStats[4], const std::vector<ygpu_junction> &host, uint64_t hostReadsB, uint64_t hostSkippedB)
{
    // (a read's junctions come from one side only, in ordinal order: merging by read keeps them together)
    const size_t at = all.size(); all.resize(at + nDev + host.size());
    std::merge(dev, dev + nDev, host.begin(), host.end(), all.begin() + at, [](const ygpu_junction &a, const ygpu_junction &b) { return a.read < b.read; });
    if (devStats) { devReads += devStats[0]; devSkipped += devStats[2]; devHandedBack += devStats[3]; }
    hostReads += hostReadsB; hostSkipped += hostSkippedB;
}

bool JunctionTrack::deviceEntryPoints() { return ygpu_junctions_enable != nullptr && ygpu_junctions_size != nullptr && ygpu_junctions_collect != nullptr; }

int JunctionTrack::deviceEnable(ygpu_ctx *ctx) const
{
    if (!deviceEntryPoints()) return YGPU_ENODEV;
    ygpu_junction_params p; p.min_mapq = minMapq; p.n_seqs = (uint32_t)seqStart.size(); p.seq_start = seqStart.data(); p.seq_length = seqLength.data();
    return ygpu_junctions_enable(ctx, &p);
}

int JunctionTrack::deviceCollect(ygpu_ctx *ctx, std::vector<ygpu_junction> &out, uint64_t stats[4]) const
{
    out.clear();
    if (!deviceEntryPoints()) return YGPU_ENODEV;
    uint64_t n = 0; int rc = ygpu_junctions_size(ctx, &n); if (rc != 0) return rc;
    out.resize((size_t)n);
    return ygpu_junctions_collect(ctx, out.data(), stats);
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
