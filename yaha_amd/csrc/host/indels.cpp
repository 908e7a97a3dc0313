// indels.cpp -- the host's side of the indel alleles (-oid): the run's alleles, what the formatter threads count of them, and the writer.  What an event is --
// a D or I op of at least -idlen bases of a printed record, its slot, the kept bases of an insertion, the two-sequence drop, the MAPQ gate, the walk that never
// leaves [sqo, eqo] -- and what its key looks like are ../indel_core.h, the source the device stage compiles as well (device/indel_stage.h).
//
// The run's alleles are ONE map keyed by the three words, in the file's order.  It is fed by every drain of a context's table during the run, by a last
// collect per context, and by the formatter threads, which walk the records the device did not count into a list of their own per batch and merge it here
// under the lock: the map is touched once per batch and per drain, not once per event.
//
// The device entry points are WEAK references here, as depth.cpp's are: the host stages are also linked against test doubles that do not have them (the CPU
// tier), and then -- as when the library refuses to enable the stage -- the host counts every record itself.
#include "yaha_host.h"
#include "../indel_core.h"
#include <algorithm>

extern "C" {
__attribute__((weak)) int ygpu_indels_enable(ygpu_ctx *ctx, const ygpu_indel_params *p);
__attribute__((weak)) int ygpu_indels_size(ygpu_ctx *ctx, uint64_t *used);
__attribute__((weak)) int ygpu_indels_collect(ygpu_ctx *ctx, ygpu_indel_entry *out, uint64_t stats[6]);
}

namespace yaha {

static inline yindel::Key coreKey(const IndelKey &k) { yindel::Key c; c.w0 = k.w0; c.w1 = k.w1; c.w2 = k.w2; return c; }
bool IndelKeyLess::operator()(const IndelKey &a, const IndelKey &b) const { return yindel::keyLess(coreKey(a), coreKey(b)); }

bool IndelTrack::setup(const Args &a, const Genome &g, int, int nContexts, std::string &err)
{
    genome = &g; file = a.idFileName; minMapq = (uint32_t)a.idMinQ; minLen = (uint32_t)a.idLen; minCount = (uint32_t)a.idMin;
    if (quietFor) { minMapq = (uint32_t)a.puMinQ; minLen = 1; }             // (what the indel calls take: every length, the pileup's gate)
    enabled.assign((size_t)nContexts, CtxAt{nullptr, 0, 0, 0});
    capacity = yindel::tableCapacity(a.batchReads > 0 ? std::min<uint64_t>((uint64_t)a.batchReads * (uint64_t)std::max(1, a.maxQueryLength), (uint64_t)16 << 20)
        : (uint64_t)16 << 20);
    seqs.set(g); binBase.assign(seqs.start.size() + 1, 0);
    if (!ydepth::layoutBins(seqs.length.data(), (uint32_t)seqs.length.size(), 1, binBase.data(), &nSlots)) { err = "-oid: the reference bases do not fit 32 bits"; return false; }
    return true;
}

void IndelTrack::add(const OutClump &oc, const Read &r, Slot *s)
{
    const ydepth::Layout L{seqs.start.data(), seqs.length.data(), binBase.data(), (uint32_t)seqs.start.size(), 1u, minMapq};
    Local &local = *static_cast<Local *>(s); std::vector<IndelKey> &keys = local.keys;
    const int g = yindel::walkClump(L, oc.c, oc.ops, r.fwdCodes.data(), (uint32_t)r.fwdCodes.size(), (oc.status & 0x01) != 0, oc.mapQuality, minLen,
        [&keys](const yindel::Key &k) { keys.push_back(IndelKey{k.w0, k.w1, k.w2}); });
    if (g == ydepth::COUNTED) local.records++; else if (g == ydepth::SKIPPED_MAPQ) local.skipped++; else local.dropped++;
}

void IndelTrack::endBatch(Slot *s)
{
    Local &local = *static_cast<Local *>(s);
    if (local.keys.empty() && !local.records && !local.skipped && !local.dropped) return;
    std::sort(local.keys.begin(), local.keys.end(), IndelKeyLess());       // (equal keys side by side: one look-up each)
    {
        std::lock_guard<std::mutex> lk(mu);
        for (size_t i = 0; i < local.keys.size();) {
            size_t j = i + 1; while (j < local.keys.size() && yindel::sameKey(coreKey(local.keys[i]), coreKey(local.keys[j]))) j++;
            alleles[local.keys[i]] += j - i; i = j;
        }
        hostEvents += local.keys.size(); hostRecords += local.records; hostSkipped += local.skipped; hostDropped += local.dropped;
    }
    local.keys.clear(); local.records = local.skipped = local.dropped = 0;
}

bool IndelTrack::deviceEntryPoints() { return ygpu_indels_enable != nullptr && ygpu_indels_size != nullptr && ygpu_indels_collect != nullptr; }

int IndelTrack::enable(const CtxAt &at)
{
    if (!deviceEntryPoints() || getenv("YAHA_HOST_INDELS") != nullptr) return YGPU_ENODEV;
    ygpu_indel_params p; memset(&p, 0, sizeof p);
    p.min_mapq = minMapq; p.min_length = minLen; seqs.into(p); p.capacity = capacity;
    const int rc = ygpu_indels_enable(at.ctx, &p); if (rc == 0) enabled[at.index] = at;
    return rc;
}

int IndelTrack::drainAbove(ygpu_ctx *ctx, uint64_t more, uint64_t limit)
{
    uint64_t used = 0; std::string err; const int rc = ygpu_indels_size(ctx, &used);
    return rc == 0 && used && used + more > limit ? deviceDrain(ctx, true, err) : rc;
}
int IndelTrack::beforeFilter(const CtxAt &at, size_t batchBases) { return drainAbove(at.ctx, batchBases / 2, capacity / 2); }
int IndelTrack::afterFilter(const CtxAt &at, Slot *) { return drainAbove(at.ctx, 0, capacity / 4); }

int IndelTrack::deviceDrain(ygpu_ctx *ctx, bool duringRun, std::string &err)
{
    if (!deviceEntryPoints()) return YGPU_ENODEV;
    uint64_t n = 0, st[6] = {0, 0, 0, 0, 0, 0};
    int rc = ygpu_indels_size(ctx, &n);
    std::vector<ygpu_indel_entry> got((size_t)n);
    if (rc == 0) rc = ygpu_indels_collect(ctx, got.data(), st);
    if (rc != 0) { err = ygpu_last_error(ctx); return rc; }
    std::lock_guard<std::mutex> lk(mu);
    for (const ygpu_indel_entry &e : got) alleles[IndelKey{e.w0, e.w1, e.w2}] += e.count;
    devRecords += st[0]; devSkipped += st[1]; devDropped += st[2]; devEvents += st[3]; devHandedBack += st[4]; devLost += st[5];
    if (duringRun) drains++;
    return 0;
}

// the end of the run: what every enabled context's table still holds, then the file
bool IndelTrack::finish(FILE *mainOut, FILE *log, bool)
{
    std::string ierr; bool ok = true;
    for (const CtxAt &at : enabled) if (at.ctx && ok) {
        const int rc = deviceDrain(at.ctx, false, ierr);
        if (rc != 0) { fprintf(log, "%s: collecting the indel table of context %d failed (%d): %s\n", name(), at.index, rc, ierr.c_str()); ok = false; }
    }
    if (devLost) { fprintf(log, "%s: %llu indel events found no entry in a device table -- the file would be incomplete.\n", name(), (unsigned long long)devLost); ok = false; }
    if (quietFor) return ok;
    if (fflush(mainOut) != 0) ok = false;
    if (ok && !write(file.c_str(), *genome, ierr)) { fprintf(log, "%s\n", ierr.c_str()); ok = false; }
    return ok;
}

void IndelTrack::stats(std::string &line) const
{
    if (quietFor) return;
    char t[512]; snprintf(t, sizeof t, ", \"indel_device_records\": %llu, \"indel_host_records\": %llu, \"indel_events\": %llu, \"indel_alleles\": %llu, "
        "\"indel_lines\": %llu, \"indel_drains\": %llu, \"indel_lost\": %llu", (unsigned long long)devRecords, (unsigned long long)hostRecords,
        (unsigned long long)(devEvents + hostEvents), (unsigned long long)alleles.size(), (unsigned long long)nLines, (unsigned long long)drains, (unsigned long long)devLost);
    line += t;
}

// One line per allele at least minCount records carry, in the map's order: name, position (1-based within the sequence: a deletion's first deleted base, an
// insertion's slot), DEL / INS, length, the kept bases of an insertion ('+' behind them when it is longer) or '*', the count.
bool IndelTrack::write(const char *path, const Genome &g, std::string &err)
{
    FILE *f = !strcmp(path, "stdout") ? stdout : fopen(path, "w");
    if (!f) { err = std::string("Failure to open the indel allele file: ") + path + "."; return false; }
    bool ok = true; size_t s = 0; nLines = 0; char bases[yindel::KEPT + 2];
    for (auto it = alleles.begin(); it != alleles.end() && ok; ++it) {
        if (it->second < minCount) continue;
        const yindel::Key k = coreKey(it->first); const uint32_t slot = yindel::slotOfKey(k);
        if (slot >= nSlots) continue;
        while (s + 1 < g.seqs.size() && slot >= binBase[s + 1]) s++;
        const bool ins = yindel::typeOfKey(k) == (uint32_t)yindel::INS; const uint32_t kept = yindel::keptOfKey(k); uint32_t n = 0;
        for (; n < kept; n++) bases[n] = "ACGTN"[std::min(yindel::baseOfKey(k, n), 4u)];
        if (ins && yindel::lenOfKey(k) > (uint32_t)yindel::KEPT) bases[n++] = '+';
        if (!ins) bases[n++] = '*';
        bases[n] = 0;
        ok = fprintf(f, "%s\t%u\t%s\t%u\t%s\t%llu\n", g.seqs[s].name.c_str(), slot - binBase[s] + 1, ins ? "INS" : "DEL", yindel::lenOfKey(k), bases,
            (unsigned long long)it->second) > 0;
        nLines++;
    }
    if (f == stdout) ok = fflush(f) == 0 && ok; else ok = fclose(f) == 0 && ok;
    if (!ok) err = std::string("Failure writing the indel allele file: ") + path + ".";
    return ok;
}
}  // namespace yaha
