// eprofile.cpp -- the host's side of the error profile (-oep): the run's table, what the formatter threads add to it, and the writer.  What one record adds -- a
// pair per aligned base by the channels of reference and read, the lengths of its I and D ops, its identity, its errors by position in the read, the
// two-sequence drop, the MAPQ gate, the walk that never leaves [sqo, eqo] -- is ../eprofile_core.h, the source the device stage compiles as well
// (device/eprofile_stage.h).
//
// The run's table is 1556 words.  The device keeps one per context behind its post-filter (ygpu_eprofile_*), read once at the end of the run; the formatter
// threads walk the records the device did not count -- runs whose post-filter stays on the host, the reads it hands back unfiltered, builds without the entry
// points, YAHA_HOST_EPROFILE -- into the batch's slot, which is added here under the lock once per batch.
//
// The device entry points are WEAK references here, as depth.cpp's are: the host stages are also linked against test doubles that do not have them (the CPU
// tier), and then -- as when the library refuses to enable the stage -- the host counts every record itself.
#include "yaha_host.h"
#include "../eprofile_core.h"

extern "C" {
__attribute__((weak)) int ygpu_eprofile_enable(ygpu_ctx *ctx, const ygpu_eprofile_params *p);
__attribute__((weak)) int ygpu_eprofile_size(ygpu_ctx *ctx, uint64_t *n_words);
__attribute__((weak)) int ygpu_eprofile_collect(ygpu_ctx *ctx, uint64_t *words, uint64_t stats[4]);
}

namespace yaha {

bool EProfileTrack::setup(const Args &a, const Genome &g, int, int nContexts, std::string &)
{
    genome = &g; file = a.epFileName; minMapq = (uint32_t)a.epMinQ;
    enabled.assign((size_t)nContexts, CtxAt{nullptr, 0, 0, 0});
    seqs.set(g); table.assign((size_t)yeprofile::WORDS, 0);
    return true;
}

SideOutput::Slot *EProfileTrack::newSlot() const { Local *l = new Local; l->words.assign((size_t)yeprofile::WORDS, 0); return l; }

void EProfileTrack::add(const OutClump &oc, const Read &r, Slot *s)
{
    const ydepth::Layout L{seqs.start.data(), seqs.length.data(), nullptr, (uint32_t)seqs.start.size(), 1u, minMapq};
    Local &local = *static_cast<Local *>(s); uint64_t *const words = local.words.data();
    const int g = yeprofile::walkClump(L, oc.c, oc.ops, r.fwdCodes.data(), (uint32_t)r.fwdCodes.size(), (oc.status & 0x01) != 0, oc.mapQuality, genome->bases,
        genome->nBaseBytes, [words](uint32_t w, uint32_t n) { if (w < (uint32_t)yeprofile::WORDS) words[w] += n; });
    if (g == ydepth::COUNTED) local.records++; else if (g == ydepth::SKIPPED_MAPQ) local.skipped++; else local.dropped++;
}

void EProfileTrack::endBatch(Slot *s)
{
    Local &local = *static_cast<Local *>(s);
    if (!local.records && !local.skipped && !local.dropped) return;
    {
        std::lock_guard<std::mutex> lk(mu);
        if (local.records) for (size_t w = 0; w < table.size(); w++) table[w] += local.words[w];
        hostRecords += local.records; hostSkipped += local.skipped; hostDropped += local.dropped;
    }
    if (local.records) std::fill(local.words.begin(), local.words.end(), 0);
    local.records = local.skipped = local.dropped = 0;
}

bool EProfileTrack::deviceEntryPoints() { return ygpu_eprofile_enable != nullptr && ygpu_eprofile_size != nullptr && ygpu_eprofile_collect != nullptr; }

int EProfileTrack::enable(const CtxAt &at)
{
    if (!deviceEntryPoints() || getenv("YAHA_HOST_EPROFILE") != nullptr) return YGPU_ENODEV;
    ygpu_eprofile_params p; memset(&p, 0, sizeof p);
    p.min_mapq = minMapq; seqs.into(p);
    const int rc = ygpu_eprofile_enable(at.ctx, &p); if (rc == 0) enabled[at.index] = at;
    return rc;
}

// the end of the run: every enabled context's table joins the host's share, then the file
bool EProfileTrack::finish(FILE *mainOut, FILE *log, bool)
{
    bool ok = true; std::vector<uint64_t> part((size_t)yeprofile::WORDS);
    for (const CtxAt &at : enabled) if (at.ctx && ok) {
        uint64_t n = 0, st[4] = {0, 0, 0, 0}; int rc = ygpu_eprofile_size(at.ctx, &n);
        if (rc == 0 && n != (uint64_t)yeprofile::WORDS) { fprintf(log, "-oep: the device's table has another size than the host's\n"); ok = false; break; }
        if (rc == 0) rc = ygpu_eprofile_collect(at.ctx, part.data(), st);
        if (rc != 0) { fprintf(log, "-oep: collecting the error profile of context %d failed (%d): %s\n", at.index, rc, ygpu_last_error(at.ctx)); ok = false; break; }
        for (size_t w = 0; w < table.size(); w++) table[w] += part[w];
        devRecords += st[0]; devSkipped += st[1]; devDropped += st[2]; devHandedBack += st[3];
    }
    if (fflush(mainOut) != 0) ok = false;
    std::string err;
    if (ok && !write(file.c_str(), err)) { fprintf(log, "%s\n", err.c_str()); ok = false; }
    return ok;
}

void EProfileTrack::stats(std::string &line) const
{
    uint64_t pairs = 0, indels = 0;
    for (int w = 0; w < yeprofile::NCH * yeprofile::NCH; w++) pairs += table[(size_t)yeprofile::SUB + w];
    for (int w = 0; w < 2 * yeprofile::NLEN; w++) indels += table[(size_t)yeprofile::INS + w];
    char t[256]; snprintf(t, sizeof t, ", \"eprofile_device_records\": %llu, \"eprofile_host_records\": %llu, \"eprofile_pairs\": %llu, \"eprofile_indels\": %llu",
        (unsigned long long)devRecords, (unsigned long long)hostRecords, (unsigned long long)pairs, (unsigned long long)indels);
    line += t;
}

// Fixed text, tab-separated.  A first line with the record counts, then every line starts with its section's name: SUB -- a header row, then a row per reference
// channel with the five read channels --, INS and DEL -- all 65 lengths, the last one "65+" --, IDENT -- the per-mille values that records reached, with their
// count --, POS -- all 100 bins: pairs, pairs that are no match, insertions, deletions.
bool EProfileTrack::write(const char *path, std::string &err) const
{
    FILE *f = !strcmp(path, "stdout") ? stdout : fopen(path, "w");
    if (!f) { err = std::string("Failure to open the error profile file: ") + path + "."; return false; }
    auto u = [](uint64_t v) { return (unsigned long long)v; };
    static const char *const chName[yeprofile::NCH] = {"A", "C", "G", "T", "N"};
    bool ok = fprintf(f, "#yaha error profile\trecords\t%llu\tskipped_mapq\t%llu\tdropped\t%llu\n", u(devRecords + hostRecords), u(devSkipped + hostSkipped),
        u(devDropped + hostDropped)) > 0;
    ok = ok && fputs("SUB\tref\tA\tC\tG\tT\tN\n", f) >= 0;
    for (int r = 0; r < yeprofile::NCH && ok; r++) {
        const uint64_t *row = table.data() + yeprofile::SUB + r * yeprofile::NCH;
        ok = fprintf(f, "SUB\t%s\t%llu\t%llu\t%llu\t%llu\t%llu\n", chName[r], u(row[0]), u(row[1]), u(row[2]), u(row[3]), u(row[4])) > 0;
    }
    for (int sec = 0; sec < 2 && ok; sec++) for (int n = 1; n <= yeprofile::NLEN && ok; n++)
        ok = fprintf(f, "%s\t%d%s\t%llu\n", sec ? "DEL" : "INS", n, n == yeprofile::NLEN ? "+" : "", u(table[(size_t)(sec ? yeprofile::DEL : yeprofile::INS) + n - 1])) > 0;
    for (int i = 0; i < yeprofile::NIDENT && ok; i++) if (table[(size_t)yeprofile::IDENT + i]) ok = fprintf(f, "IDENT\t%d\t%llu\n", i, u(table[(size_t)yeprofile::IDENT + i])) > 0;
    for (int b = 0; b < yeprofile::NBINS && ok; b++) {
        const uint64_t *row = table.data() + yeprofile::POS + b * yeprofile::NPOS;
        ok = fprintf(f, "POS\t%d\t%llu\t%llu\t%llu\t%llu\n", b, u(row[0]), u(row[1]), u(row[2]), u(row[3])) > 0;
    }
    if (f == stdout) ok = fflush(f) == 0 && ok; else ok = fclose(f) == 0 && ok;
    if (!ok) err = std::string("Failure writing the error profile file: ") + path + ".";
    return ok;
}
}  // namespace yaha
