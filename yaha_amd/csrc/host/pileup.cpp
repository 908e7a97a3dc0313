// pileup.cpp -- the host's side of the allele pileup (-opu), a BinnedTrack with a bin of one base and seven channels (depth.cpp has what the tracks share).
// What a record adds -- the read's base under every M / R reference base, DEL under D, INS per I, the two-sequence drop, the MAPQ gate, the walk that never
// leaves [sqo, eqo] -- and what a site is are ../pileup_core.h, the source the device stage compiles as well (device/pileup_stage.h).
//
// The end of the run is this kind's own (mergeDevices): the device's array is 28 bytes a reference base per index image and stays where it is.  Every source
// lists its candidates, the slots with nonref >= 1 -- each image on the device (ygpu_pileup_candidates_*), the host from the blocks of counts its formatter
// threads made (nothing dense on the host either: a block of 4 096 slots exists once a record the host counts touches it); the sorted union goes back to
// every image, which gathers its seven counts there (ygpu_pileup_gather); the host adds its own and applies -pumin with the core's routine.
// A site with summed nonref >= minAlt >= 1 has nonref >= 1 in at least one source, so it is in the union: the table is exact for any number of images and any share of the host.
//
// The device entry points are WEAK references here, as depth.cpp's are: the host stages are also linked against test doubles that do not have them (the CPU
// tier), and then -- as when the library refuses to enable the stage -- the host counts every record itself.
#include "yaha_host.h"
#include "../pileup_core.h"
#include <algorithm>
#include <new>
#include <chrono>

extern "C" {
__attribute__((weak)) int ygpu_pileup_enable(ygpu_ctx *ctx, const ygpu_pileup_params *p);
__attribute__((weak)) int ygpu_pileup_size(ygpu_ctx *ctx, uint64_t *n_slots);
__attribute__((weak)) int ygpu_pileup_collect(ygpu_ctx *ctx, uint32_t *counts, uint64_t stats[5]);
__attribute__((weak)) int ygpu_pileup_candidates_size(ygpu_ctx *ctx, uint64_t *n);
__attribute__((weak)) int ygpu_pileup_candidates_collect(ygpu_ctx *ctx, uint32_t *slots);
__attribute__((weak)) int ygpu_pileup_gather(ygpu_ctx *ctx, const uint32_t *slots, uint64_t n, uint32_t *rows);
__attribute__((weak)) int ygpu_pileup_add(ygpu_ctx *ctx, const uint32_t *slots, const uint32_t *rows, uint64_t n);
}

namespace yaha {

PileupTrack::PileupTrack()
    : BinnedTrack({"-opu", "-opu", "pileup", "pileup", "YAHA_HOST_PILEUP",
                   ", \"pileup_bases\": %llu, \"pileup_device_records\": %llu, \"pileup_host_records\": %llu, \"pileup_counted\": %llu"}, (uint32_t)ypileup::NCH,
                  ygpu_pileup_enable != nullptr && ygpu_pileup_candidates_size != nullptr && ygpu_pileup_candidates_collect != nullptr && ygpu_pileup_gather != nullptr,
                  ygpu_pileup_size, ygpu_pileup_collect) {}

bool PileupTrack::setup(const Args &a, const Genome &g, int nImages, int nContexts, std::string &err)
{
    minAlt = (uint32_t)a.puMinAlt; return init(g, a.puFileName, 1, a.puMinQ, nImages, nContexts, err);
}

PileupTrack::~PileupTrack() { for (uint32_t *b : blocks) free(b); }

bool PileupTrack::allocate(std::string &err)
{
    if (bin != 1) { err = "-opu: the pileup has one slot per reference base"; return false; }
    for (uint32_t *b : blocks) free(b);
    blocks.assign((size_t)(nBins / kBlock + 1), nullptr);
    return true;
}

// (several formatter threads may meet at a block that is not there yet: each makes one, the first compare-and-swap wins, the others free theirs)
uint32_t *PileupTrack::block(uint32_t slot)
{
    uint32_t **const at = &blocks[slot / kBlock];
    uint32_t *b = __atomic_load_n(at, __ATOMIC_ACQUIRE);
    if (b) return b;
    uint32_t *fresh = (uint32_t *)calloc((size_t)kBlock * ypileup::NCH, sizeof(uint32_t));
    if (!fresh) throw std::bad_alloc();
    if (__atomic_compare_exchange_n(at, &b, fresh, false, __ATOMIC_ACQ_REL, __ATOMIC_ACQUIRE)) return fresh;
    free(fresh); return b;
}

void PileupTrack::add(const OutClump &oc, const Read &r, Slot *)
{
    const uint64_t n = nBins; uint64_t added = 0;
    countRecord(ypileup::walkClump(layout(), oc.c, oc.ops, r.fwdCodes.data(), (uint32_t)r.fwdCodes.size(), (oc.status & 0x01) != 0, oc.mapQuality,
        [this, n, &added](uint32_t s, uint32_t ch) {
            if (s >= n || ch >= (uint32_t)ypileup::NCH) return;
            __atomic_fetch_add(block(s) + (size_t)(s % kBlock) * ypileup::NCH + ch, 1u, __ATOMIC_RELAXED); added++;
        }));
    if (added) __atomic_fetch_add(&hostCounted, added, __ATOMIC_RELAXED);
}

int PileupTrack::deviceEnable(ygpu_ctx *ctx) const
{
    if (!deviceEntryPoints()) return YGPU_ENODEV;
    ygpu_pileup_params p; p.min_mapq = minMapq; seqs.into(p);
    return ygpu_pileup_enable(ctx, &p);
}

int PileupTrack::candidatesUnion(ygpu_ctx *const *feeders, int n, bool withHost, const Genome &g, std::vector<uint32_t> &all, int *failed, std::string &err)
{
    const ydepth::Layout L = layout();
    // 1. every source's candidates: the host's blocks, then each image's selection
    all.clear();
    if (withHost) for (size_t b = 0; b < blocks.size(); b++) if (blocks[b]) {
        const uint64_t s0 = (uint64_t)b * kBlock, s1 = std::min<uint64_t>(s0 + kBlock, nBins);
        for (uint64_t s = s0; s < s1; s++) if (ypileup::isSiteAt(L, g.bases, g.nBaseBytes, (uint32_t)s, row((uint32_t)s), 1u)) all.push_back((uint32_t)s);
    }
    std::vector<uint32_t> mine, merged;
    for (int k = 0; k < n; k++) {
        uint64_t slots = 0, nc = 0; int rc = ygpu_pileup_size(feeders[k], &slots);
        if (rc == 0 && slots != nBins) { err = "the device's pileup array has another size than the host's"; *failed = k; return YGPU_EINTERNAL; }
        if (rc == 0) rc = ygpu_pileup_candidates_size(feeders[k], &nc);
        if (rc == 0) { mine.resize((size_t)nc); rc = ygpu_pileup_candidates_collect(feeders[k], mine.data()); }
        if (rc != 0) { err = ygpu_last_error(feeders[k]); *failed = k; return rc; }
        // 2. the sorted union (every list is ascending and has no slot twice)
        merged.resize(all.size() + mine.size());
        merged.resize((size_t)(std::set_union(all.begin(), all.end(), mine.begin(), mine.end(), merged.begin()) - merged.begin()));
        all.swap(merged);
    }
    return 0;
}

int PileupTrack::unionRows(ygpu_ctx *const *feeders, int n, bool withHost, bool account, const Genome &g, std::vector<uint32_t> &all, std::vector<uint32_t> &rows,
                           int *failed, std::string &err)
{
    auto now = []() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
    const double t0 = now();
    { const int rc = candidatesUnion(feeders, n, withHost, g, all, failed, err); if (rc != 0) return rc; }
    const double t1 = now(); msCandidates = t1 - t0;
    // 3. every image's counts at the union, 4. the host's own on top
    rows.assign(all.size() * ypileup::NCH + 1, 0); std::vector<uint32_t> part;
    if (withHost) for (size_t i = 0; i < all.size(); i++) if (const uint32_t *own = row(all[i])) memcpy(rows.data() + i * ypileup::NCH, own, sizeof(uint32_t) * ypileup::NCH);
    for (int k = 0; k < n; k++) {
        part.assign(all.size() * ypileup::NCH + 1, 0); uint64_t st[5] = {0, 0, 0, 0, 0};
        int rc = ygpu_pileup_gather(feeders[k], all.data(), all.size(), part.data());
        if (rc == 0 && account) rc = ygpu_pileup_collect(feeders[k], nullptr, st);
        if (rc != 0) { err = ygpu_last_error(feeders[k]); *failed = k; return rc; }
        for (size_t w = 0; w < all.size() * ypileup::NCH; w++) rows[w] += part[w];
        devRecords += st[0]; devSkipped += st[1]; devDropped += st[2]; devHandedBack += st[3]; devCounted += st[4];
    }
    msGather = now() - t1;
    return 0;
}

int PileupTrack::mergeDevices(ygpu_ctx *const *feeders, int n, const Genome &g, int *failed, std::string &err)
{
    const ydepth::Layout L = layout();
    std::vector<uint32_t> all, rows;
    const int rc = unionRows(feeders, n, true, true, g, all, rows, failed, err); if (rc != 0) return rc;
    nCandidates = all.size();
    // ... and -pumin, with the routine the candidates were selected with
    sites.clear();
    for (size_t i = 0; i < all.size(); i++) {
        const uint32_t *sum = rows.data() + i * ypileup::NCH; const uint32_t code = ypileup::refCode(L, g.bases, g.nBaseBytes, all[i]);
        if (!ypileup::isSite(sum, ypileup::chOfCode(code), minAlt)) continue;
        Site s; s.slot = all[i]; s.ref = code; memcpy(s.n, sum, sizeof s.n); sites.push_back(s);
    }
    return 0;
}

void PileupTrack::hostRows(std::vector<uint32_t> &slots, std::vector<uint32_t> &rows) const
{
    slots.clear(); rows.clear();
    for (size_t b = 0; b < blocks.size(); b++) if (const uint32_t *blk = blocks[b]) {
        const uint64_t s0 = (uint64_t)b * kBlock, s1 = std::min<uint64_t>(s0 + kBlock, nBins);
        for (uint64_t s = s0; s < s1; s++) {
            const uint32_t *r = blk + (size_t)(s - s0) * ypileup::NCH;
            if (r[0] | r[1] | r[2] | r[3] | r[4] | r[5] | r[6]) { slots.push_back((uint32_t)s); rows.insert(rows.end(), r, r + ypileup::NCH); }
        }
    }
}

int PileupTrack::foldOnce(ygpu_ctx *const *feeders, int n, bool withHost, const std::vector<uint32_t> *at, uint64_t *folded, bool *anyAdded, ygpu_ctx **bad)
{
    if (n < 1 || ygpu_pileup_add == nullptr) return YGPU_ENODEV;
    ygpu_ctx *const home = feeders[0]; std::vector<uint32_t> slots, rows;
    if (withHost && !hostFolded) {
        hostRows(slots, rows);
        if (!slots.empty()) { *anyAdded = true; const int rc = ygpu_pileup_add(home, slots.data(), rows.data(), slots.size()); if (rc != 0) { *bad = home; return rc; } }
        hostFolded = true; *folded += slots.size();
    }
    if (n > 1 && at) {
        std::vector<uint32_t> want(at->size());
        want.resize((size_t)(std::set_difference(at->begin(), at->end(), othersFolded.begin(), othersFolded.end(), want.begin()) - want.begin()));
        for (int k = 1; k < n && !want.empty(); k++) {
            rows.assign(want.size() * ypileup::NCH + 1, 0);
            int rc = ygpu_pileup_gather(feeders[k], want.data(), want.size(), rows.data()); if (rc != 0) { *bad = feeders[k]; return rc; }
            *anyAdded = true; rc = ygpu_pileup_add(home, want.data(), rows.data(), want.size()); if (rc != 0) { *bad = home; return rc; }
            *folded += want.size();
        }
        std::vector<uint32_t> merged(othersFolded.size() + want.size());
        merged.resize((size_t)(std::set_union(othersFolded.begin(), othersFolded.end(), want.begin(), want.end(), merged.begin()) - merged.begin()));
        othersFolded.swap(merged);
    }
    return 0;
}

int PileupTrack::rowsAt(ygpu_ctx *const *feeders, int n, const std::vector<uint32_t> &slots, std::vector<uint32_t> &rows, ygpu_ctx **bad)
{
    rows.assign(slots.size() * ypileup::NCH + 1, 0); std::vector<uint32_t> part;
    if (!hostFolded) for (size_t i = 0; i < slots.size(); i++) if (slots[i] < nBins) if (const uint32_t *own = row(slots[i]))
        for (int ch = 0; ch < ypileup::NCH; ch++) rows[i * ypileup::NCH + ch] += own[ch];
    for (int k = 0; k < n && !slots.empty(); k++) {
        part.assign(slots.size() * ypileup::NCH + 1, 0);
        const int rc = ygpu_pileup_gather(feeders[k], slots.data(), slots.size(), part.data()); if (rc != 0) { *bad = feeders[k]; return rc; }
        for (size_t i = 0; i < slots.size(); i++) {
            if (k > 0 && std::binary_search(othersFolded.begin(), othersFolded.end(), slots[i])) continue;      // (already in the home image's row)
            for (int ch = 0; ch < ypileup::NCH; ch++) rows[i * ypileup::NCH + ch] += part[i * ypileup::NCH + ch];
        }
    }
    return 0;
}

std::string PileupTrack::mergeNote() const
{
    char t[96]; snprintf(t, sizeof t, " (candidates and their union %.1f ms, gathers %.1f ms)", msCandidates, msGather);
    return t;
}

std::string PileupTrack::extraStats() const
{
    char t[96]; snprintf(t, sizeof t, ", \"pileup_candidates\": %llu, \"pileup_sites\": %llu", (unsigned long long)nCandidates, (unsigned long long)sites.size());
    return t;
}

// A header line, then one line per site in index order: name, start (0-based), end = start + 1 -- a line joins with the bins of -oev and -ocov --, the
// reference letter as the .nib2 decodes it, the seven counts.
bool PileupTrack::writeLines(FILE *f, const Genome &g) const
{
    bool ok = fputs("#chrom\tstart\tend\tref\tA\tC\tG\tT\tN\tdel\tins\n", f) >= 0;
    size_t s = 0;
    for (size_t i = 0; i < sites.size() && ok; i++) {
        const Site &x = sites[i];
        while (s + 1 < g.seqs.size() && x.slot >= binBase[s + 1]) s++;
        const uint32_t pos = x.slot - binBase[s];
        ok = fprintf(f, "%s\t%u\t%u\t%c\t%u\t%u\t%u\t%u\t%u\t%u\t%u\n", g.seqs[s].name.c_str(), pos, pos + 1, kFourBitChars[x.ref & 15u], x.n[0], x.n[1], x.n[2], x.n[3], x.n[4],
            x.n[5], x.n[6]) > 0;
    }
    return ok;
}
}  // namespace yaha
