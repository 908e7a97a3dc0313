// indelcalls.cpp -- the host's side of the indel calls (-oindel), the eighth side output: it counts nothing itself but takes the run's raw indel alleles
// (indels.cpp) and the run's allele pileup (pileup.cpp) at the end of the run, left-normalises and merges the alleles, judges each at its anchor base and writes
// the calls as VCF 4.2.  What the shift is, when two alleles are one, the counts r and a, the three costs, GT, QUAL, GQ, the thresholds and the record a call
// leaves are ../indelcall_core.h, the source the device stage compiles as well (device/indelcall_stage.h).
//
// The end of the run (finish, after the pileup's, the SNVs' and the indel alleles' own): ONE image is picked, the first with a feeder.  There the alleles are
// normalised and merged (ygpu_indelcall_normalize: the reference lives in HBM beside the array); what the array lacks is folded in -- the host's rows, and in a
// run over several images the other images' rows at the anchor slots, for which alone the merged alleles travel back (PileupTrack::foldOnce: nothing is added
// twice, whichever of -osnv and -oindel got there first); the calls are selected (ygpu_indelcall_size) and collected.  In a run over one image only the raw
// alleles go up and only the calls come down.
// The host's routine: without the entry points (the CPU tier's test doubles), without a feeder (the host counted everything), with YAHA_HOST_INDELCALL=1, or
// when the device's part fails before anything was folded, the same core runs here over the rows PileupTrack::rowsAt sums at the anchors; a fold that failed
// half-way leaves nothing to stand on and fails the run, as -osnv's does.
//
// The three costs are derived here, once, from -inderr: the device never takes a logarithm.  The device entry points are WEAK references, as pileup.cpp's are.
#include "yaha_host.h"
#include "../indelcall_core.h"
#include <algorithm>
#include <chrono>
#include <cmath>

extern "C" {
__attribute__((weak)) int ygpu_pileup_add(ygpu_ctx *ctx, const uint32_t *slots, const uint32_t *rows, uint64_t n);
__attribute__((weak)) int ygpu_pileup_gather(ygpu_ctx *ctx, const uint32_t *slots, uint64_t n, uint32_t *rows);
__attribute__((weak)) int ygpu_indelcall_normalize(ygpu_ctx *ctx, const ygpu_indel_entry *raw, uint64_t n, uint32_t max_shift, uint64_t *n_out, uint64_t stats[4]);
__attribute__((weak)) int ygpu_indelcall_alleles(ygpu_ctx *ctx, ygpu_indel_entry *out);
__attribute__((weak)) int ygpu_indelcall_size(ygpu_ctx *ctx, const ygpu_indelcall_params *p, uint64_t *n);
__attribute__((weak)) int ygpu_indelcall_collect(ygpu_ctx *ctx, ygpu_indel_call *calls);
}

namespace yaha {

static double nowMs() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
static inline yindel::Key keyOf(const ygpu_indel_entry &e) { yindel::Key k; k.w0 = e.w0; k.w1 = e.w1; k.w2 = e.w2; return k; }

// cM = round(-1000 log10(1 - e)), cE = round(-1000 log10 e), cH = round(1000 log10 2) with e = -inderr / 1000: (22, 1301, 301) at 50
void indelcallParamsFromArgs(const Args &a, ygpu_indelcall_params &p)
{
    memset(&p, 0, sizeof p);
    const double e = a.indErr / 1000.0;
    p.cost_match = (uint32_t)std::llround(-1000.0 * std::log10(1.0 - e)); p.cost_error = (uint32_t)std::llround(-1000.0 * std::log10(e));
    p.cost_het = (uint32_t)std::llround(1000.0 * std::log10(2.0));
    p.min_alt = (uint32_t)a.indMin; p.min_depth = (uint32_t)a.indDp; p.min_qual = (uint32_t)a.indQual;
}

bool IndelCallTrack::deviceEntryPoints()
{
    return ygpu_pileup_add != nullptr && ygpu_pileup_gather != nullptr && ygpu_indelcall_normalize != nullptr && ygpu_indelcall_alleles != nullptr
        && ygpu_indelcall_size != nullptr && ygpu_indelcall_collect != nullptr;
}

bool IndelCallTrack::setup(const Args &a, const Genome &g, int, int, std::string &err)
{
    genome = &g; file = a.indFileName; indelcallParamsFromArgs(a, P); maxShift = (uint32_t)a.indShift;
    char t[200]; snprintf(t, sizeof t, "-inderr %d -indmin %d -inddp %d -indqual %d -indshift %d -puq %d", a.indErr, a.indMin, a.indDp, a.indQual, a.indShift, a.puMinQ);
    options = t;
    pu = puGiven ? puGiven : snv ? snv->pileup() : nullptr;                  // (the tracks before this one in the list have been set up)
    if (!pu || !id) { err = "-oindel: no pileup or no indel alleles to stand on"; return false; }
    return true;
}

int IndelCallTrack::callOnDevice(ygpu_ctx *const *feeders, int n, const std::vector<ygpu_indel_entry> &raw, bool *anyAdded, std::string &err)
{
    ygpu_ctx *const home = feeders[0]; ygpu_ctx *bad = home;
    const double t0 = nowMs();
    uint64_t nOut = 0, st[4] = {0, 0, 0, 0};
    int rc = ygpu_indelcall_normalize(home, raw.data(), raw.size(), maxShift, &nOut, st);
    if (rc != 0) { err = ygpu_last_error(home); return rc; }
    const double t1 = nowMs(); msNorm = t1 - t0;
    // the other images' rows at the anchors: the one step the merged alleles leave the device for
    std::vector<uint32_t> anchors;
    if (n > 1 && nOut) {
        std::vector<ygpu_indel_entry> al((size_t)nOut);
        rc = ygpu_indelcall_alleles(home, al.data()); if (rc != 0) { err = ygpu_last_error(home); return rc; }
        for (const ygpu_indel_entry &e : al) anchors.push_back(yindel::slotOfKey(keyOf(e)) - 1u);
        std::sort(anchors.begin(), anchors.end()); anchors.erase(std::unique(anchors.begin(), anchors.end()), anchors.end());
    }
    rc = pu->foldOnce(feeders, n, true, n > 1 ? &anchors : nullptr, &foldedSlots, anyAdded, &bad);
    if (rc != 0) { err = ygpu_last_error(bad); foldBroke = *anyAdded; return rc; }
    const double t2 = nowMs(); msFold = t2 - t1;
    uint64_t nCalls = 0; rc = ygpu_indelcall_size(home, &P, &nCalls);
    if (rc == 0) { calls.assign((size_t)nCalls, ygpu_indel_call{}); rc = ygpu_indelcall_collect(home, calls.data()); }
    if (rc != 0) { err = ygpu_last_error(home); calls.clear(); return rc; }
    msSelect = nowMs() - t2;
    nRaw = st[0]; nShifted = st[1]; nMerged = st[2]; nSkipped = st[3];
    return 0;
}

int IndelCallTrack::callOnHost(ygpu_ctx *const *feeders, int n, const std::vector<ygpu_indel_entry> &raw, std::string &err)
{
    const double t0 = nowMs();
    const ydepth::Layout L{pu->seqs.start.data(), pu->seqs.length.data(), pu->binBase.data(), (uint32_t)pu->seqs.start.size(), 1u, pu->minMapq};
    std::map<IndelKey, uint64_t, IndelKeyLess> merged;
    nRaw = raw.size(); nShifted = nSkipped = 0;
    for (const ygpu_indel_entry &e : raw) {
        const yindel::Key k = keyOf(e); uint32_t seq = 0, cap = 0;
        if (!yindelcall::callable(L, pu->nBins, k, maxShift, &seq, &cap)) { nSkipped++; continue; }
        const uint32_t s = yindelcall::shiftOf(L, genome->bases, genome->nBaseBytes, seq, k, cap);
        if (s) nShifted++;
        const yindel::Key o = yindelcall::shifted(k, s);
        merged[IndelKey{o.w0, o.w1, o.w2}] += e.count;
    }
    nMerged = nRaw - nSkipped - merged.size();
    const double t1 = nowMs(); msNorm = t1 - t0;
    std::vector<uint32_t> anchors, rows;
    for (const auto &m : merged) anchors.push_back((uint32_t)m.first.w0 - 1u);
    std::sort(anchors.begin(), anchors.end()); anchors.erase(std::unique(anchors.begin(), anchors.end()), anchors.end());
    ygpu_ctx *bad = nullptr;
    const int rc = pu->rowsAt(feeders, n, anchors, rows, &bad); if (rc != 0) { err = bad ? ygpu_last_error(bad) : "no device"; return rc; }
    const double t2 = nowMs(); msFold = t2 - t1;
    calls.clear();
    for (const auto &m : merged) {
        const yindel::Key k{m.first.w0, m.first.w1, m.first.w2}; const uint32_t anchor = yindel::slotOfKey(k) - 1u;
        const size_t at = (size_t)(std::lower_bound(anchors.begin(), anchors.end(), anchor) - anchors.begin());
        ygpu_indel_call c;
        if (yindelcall::judgeAt(L, genome->bases, genome->nBaseBytes, k, ysnv::sat32(m.second), rows.data() + at * ypileup::NCH, P, &c)) calls.push_back(c);
    }
    msSelect = nowMs() - t2;
    return 0;
}

bool IndelCallTrack::finish(FILE *mainOut, FILE *log, bool timing)
{
    std::vector<ygpu_ctx *> feedCtx; std::vector<int> feedDev; pu->feeders(feedCtx, feedDev);
    // the run's raw alleles, as the device takes them (a count saturates at 32 bits)
    std::vector<ygpu_indel_entry> raw; raw.reserve(id->alleles.size());
    for (const auto &m : id->alleles) raw.push_back(ygpu_indel_entry{m.first.w0, m.first.w1, m.first.w2, ysnv::sat32(m.second), 0u});
    bool ok = true; std::string err;
    if (deviceEntryPoints() && getenv("YAHA_HOST_INDELCALL") == nullptr && !feedCtx.empty()) {
        bool anyAdded = false;
        const int rc = callOnDevice(feedCtx.data(), (int)feedCtx.size(), raw, &anyAdded, err);
        if (rc == 0) onDevice = true;
        else {
            // (what foldOnce finished is remembered by the pileup track and the host's routine reads around it; a fold that broke off is not)
            const bool halfWay = foldBroke;
            fprintf(log, "-oindel: calling on device %d failed (%d): %s%s\n", feedDev[0], rc, err.c_str(),
                halfWay ? " -- its array holds a part of the other sources: no calls" : "; the host calls instead");
            if (halfWay) ok = false;
        }
    }
    if (ok && !onDevice) {
        const int rc = callOnHost(feedCtx.data(), (int)feedCtx.size(), raw, err);
        if (rc != 0) { fprintf(log, "-oindel: collecting the pileup rows for the calls failed (%d): %s\n", rc, err.c_str()); ok = false; }
    }
    nHet = nHom = 0;
    for (const ygpu_indel_call &c : calls) (yindelcall::infoGt(c.info) == 1u ? nHet : nHom)++;
    if (fflush(mainOut) != 0) ok = false;
    const double w0 = nowMs();
    if (ok && !write(file.c_str(), err)) { fprintf(log, "%s\n", err.c_str()); ok = false; }
    msWrite = nowMs() - w0;
    if (timing) fprintf(stderr, "[yaha] -oindel: %llu raw alleles normalised in %.1f ms, %llu slots folded in %.1f ms, %llu calls selected on the %s in %.1f ms, "
        "file written in %.1f ms\n", (unsigned long long)nRaw, msNorm, (unsigned long long)foldedSlots, msFold, (unsigned long long)calls.size(), onDevice ? "device" : "host",
        msSelect, msWrite);
    return ok;
}

void IndelCallTrack::stats(std::string &line) const
{
    char t[384]; snprintf(t, sizeof t, ", \"indel_calls\": %llu, \"indel_call_het\": %llu, \"indel_call_hom\": %llu, \"indel_call_on_device\": %d, \"indel_call_raw\": %llu, "
        "\"indel_call_shifted\": %llu, \"indel_call_merged\": %llu, \"indel_call_skipped\": %llu", (unsigned long long)calls.size(), (unsigned long long)nHet,
        (unsigned long long)nHom, onDevice ? 1 : 0, (unsigned long long)nRaw, (unsigned long long)nShifted, (unsigned long long)nMerged, (unsigned long long)nSkipped);
    line += t;
}

// VCF 4.2: the header -- the options, the costs, one contig line per sequence in index order, the fields -- then one line per call in the alleles' order: POS is
// the anchor, 1-based; a deletion has REF = the anchor and the deleted bases, ALT = the anchor; an insertion REF = the anchor, ALT = the anchor and the inserted
// bases; ID is '.', FILTER is PASS, INFO has DP (reads that cover the anchor), TYPE and LEN; the one sample `yaha` has GT (0/1 or 1/1), GQ, AD (reads that do
// not carry the allele, reads that do) and PL.  One line per allele, no multi-allelic lines.
bool IndelCallTrack::write(const char *path, std::string &err) const
{
    FILE *f = !strcmp(path, "stdout") ? stdout : fopen(path, "w");
    if (!f) { err = std::string("Failure to open the indel calls file: ") + path + "."; return false; }
    const Genome &g = *genome;
    const ydepth::Layout L{pu->seqs.start.data(), pu->seqs.length.data(), pu->binBase.data(), (uint32_t)pu->seqs.start.size(), 1u, pu->minMapq};
    bool ok = fprintf(f, "##fileformat=VCFv4.2\n##source=yaha_amd %s\n", options.c_str()) > 0;
    ok = ok && fprintf(f, "##yaha_costs=<match=%u,error=%u,het=%u>\n", P.cost_match, P.cost_error, P.cost_het) > 0;
    ok = ok && fputs("##yaha_note=insertions and deletions only, left-normalised, one line per allele (-osnv holds the single-nucleotide variants)\n", f) >= 0;
    for (size_t s = 0; s < g.seqs.size() && ok; s++) ok = fprintf(f, "##contig=<ID=%s,length=%u>\n", g.seqs[s].name.c_str(), g.seqs[s].length) > 0;
    ok = ok && fputs("##INFO=<ID=DP,Number=1,Type=Integer,Description=\"Reads that cover the anchor base\">\n"
                     "##INFO=<ID=TYPE,Number=1,Type=String,Description=\"INS or DEL\">\n"
                     "##INFO=<ID=LEN,Number=1,Type=Integer,Description=\"Inserted or deleted bases\">\n"
                     "##FORMAT=<ID=GT,Number=1,Type=String,Description=\"Genotype\">\n"
                     "##FORMAT=<ID=GQ,Number=1,Type=Integer,Description=\"Genotype quality: the second smallest PL, at most 99\">\n"
                     "##FORMAT=<ID=AD,Number=R,Type=Integer,Description=\"Reads that cover the anchor without the allele, reads that carry it\">\n"
                     "##FORMAT=<ID=PL,Number=G,Type=Integer,Description=\"Normalised phred-scaled genotype likelihoods\">\n"
                     "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tyaha\n", f) >= 0;
    size_t s = 0; std::string ref, alt;
    for (size_t i = 0; i < calls.size() && ok; i++) {
        const ygpu_indel_call &c = calls[i]; const yindel::Key k{c.w0, c.w1, c.w2};
        const uint32_t slot = yindel::slotOfKey(k), len = yindel::lenOfKey(k), anchor = slot - 1u; const bool ins = yindel::typeOfKey(k) == (uint32_t)yindel::INS;
        while (s + 1 < g.seqs.size() && anchor >= pu->binBase[s + 1]) s++;
        ref.assign(1, kFourBitChars[yindelcall::infoRefCode(c.info)]); alt = ref;
        if (ins) for (uint32_t j = 0; j < yindel::keptOfKey(k); j++) alt += "ACGTN"[std::min(yindel::baseOfKey(k, j), 4u)];
        else for (uint32_t j = 0; j < len; j++) ref += kFourBitChars[yindelcall::codeIn(L, g.bases, g.nBaseBytes, (uint32_t)s, slot + j) & 15u];
        const uint32_t gt = yindelcall::infoGt(c.info);
        ok = fprintf(f, "%s\t%u\t.\t%s\t%s\t%u\tPASS\tDP=%u;TYPE=%s;LEN=%u\tGT:GQ:AD:PL\t%s:%u:%u,%u:%u,%u,%u\n", g.seqs[s].name.c_str(), anchor - pu->binBase[s] + 1u,
            ref.c_str(), alt.c_str(), c.qual, c.depth, ins ? "INS" : "DEL", len, gt == 1u ? "0/1" : "1/1", c.gq, c.ref_count, c.alt_count, c.pl[0] / 100u, c.pl[1] / 100u,
            c.pl[2] / 100u) > 0;
    }
    if (f == stdout) ok = fflush(f) == 0 && ok; else ok = fclose(f) == 0 && ok;
    if (!ok) err = std::string("Failure writing the indel calls file: ") + path + ".";
    return ok;
}
}  // namespace yaha
