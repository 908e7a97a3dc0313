// snv.cpp -- the host's side of the SNV calls (-osnv), the seventh side output: it counts nothing itself but judges the run's allele pileup (pileup.cpp) at the
// end of the run and writes the calls as VCF 4.2.  What a call is -- the reference's count r, the greatest other count a, three likelihoods from three integer
// costs, GT, QUAL, GQ, the four thresholds -- and the record it leaves are ../snv_core.h, the source the device stage compiles as well (device/snv_stage.h).
//
// The end of the run (finish, after the pileup's own): ONE image is picked, the first with a feeder; the host's non-empty slots are folded into its array, then
// every other image's rows at the union of all sources' candidates (ygpu_pileup_add: a call needs the sum of all sources before it is judged, the reads that
// agree with the reference included -- an image's own candidates alone would leave those out where all its reads agree); ONE selection runs there
// (ygpu_snv_call_size / ygpu_snv_collect) and only the calls cross PCIe.  A run over N images so moves roughly what -opu moves: the candidates of every image
// and the other images' rows travel to the host and on to the one image.  The array folded into is no longer that image's own counts -- the pileup's table
// has been written by then, and nothing reads the array afterwards.
// The host's routine: without the entry points (the CPU tier's test doubles), without a feeder (the host counted everything), with YAHA_HOST_SNV=1, or when the
// device's part fails, ysnv::judgeAt runs here over the union PileupTrack::unionRows makes -- of all sources while nothing has been folded, of the one image
// alone once everything has; a fold that failed half-way leaves nothing to stand on and fails the run.
//
// The three costs are derived here, once, from -snverr: the device never takes a logarithm.  The device entry points are WEAK references, as pileup.cpp's are.
#include "yaha_host.h"
#include "../snv_core.h"
#include <chrono>
#include <cmath>

extern "C" {
__attribute__((weak)) int ygpu_pileup_add(ygpu_ctx *ctx, const uint32_t *slots, const uint32_t *rows, uint64_t n);
__attribute__((weak)) int ygpu_snv_call_size(ygpu_ctx *ctx, const ygpu_snv_params *p, uint64_t *n);
__attribute__((weak)) int ygpu_snv_collect(ygpu_ctx *ctx, ygpu_snv_call *calls);
__attribute__((weak)) int ygpu_pileup_gather(ygpu_ctx *ctx, const uint32_t *slots, uint64_t n, uint32_t *rows);
}

namespace yaha {

static double nowMs() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

// cM = round(-1000 log10(1 - e)), cE = round(-1000 log10(e / 3)), cH = round(-1000 log10(1/2 - e / 3)) with e = -snverr / 1000: (46, 1477, 331) at 100
void snvParamsFromArgs(const Args &a, ygpu_snv_params &p)
{
    memset(&p, 0, sizeof p);
    const double e = a.snvErr / 1000.0;
    p.cost_match = (uint32_t)std::llround(-1000.0 * std::log10(1.0 - e)); p.cost_error = (uint32_t)std::llround(-1000.0 * std::log10(e / 3.0));
    p.cost_het = (uint32_t)std::llround(-1000.0 * std::log10(0.5 - e / 3.0));
    p.min_alt = (uint32_t)a.snvMin; p.min_depth = (uint32_t)a.snvDp; p.min_qual = (uint32_t)a.snvQual;
}

bool SnvTrack::deviceEntryPoints()
{
    return ygpu_pileup_add != nullptr && ygpu_snv_call_size != nullptr && ygpu_snv_collect != nullptr && ygpu_pileup_gather != nullptr;
}

bool SnvTrack::setup(const Args &a, const Genome &g, int nImages, int nContexts, std::string &err)
{
    genome = &g; file = a.snvFileName; snvParamsFromArgs(a, P);
    char t[160]; snprintf(t, sizeof t, "-snverr %d -snvmin %d -snvdp %d -snvqual %d -puq %d", a.snvErr, a.snvMin, a.snvDp, a.snvQual, a.puMinQ); options = t;
    if (shared) return true;
    own.reset(new PileupTrack);                                              // (it writes no file: its finish is never called)
    return own->setup(a, g, nImages, nContexts, err);
}

int SnvTrack::callOnDevice(PileupTrack &pu, ygpu_ctx *const *feeders, int n, int *folded, std::string &err)
{
    ygpu_ctx *const home = feeders[0]; bool anyAdded = false; int rc = 0;
    auto failed = [&](ygpu_ctx *c) { err = ygpu_last_error(c); *folded = anyAdded ? 2 : 0; return rc; };
    const double t0 = nowMs();
    // (through the pileup track, which remembers what has been folded: the indel calls read the same array after this and must add nothing twice)
    ygpu_ctx *bad = home; foldedSlots = 0;
    rc = pu.foldOnce(feeders, n, true, nullptr, &foldedSlots, &anyAdded, &bad); if (rc != 0) return failed(bad);
    // The other images: a call's counts must be the sum over ALL sources, the reference's count included -- and an image whose reads all agree with the reference
    // at a slot does not list it.  So the slots are the union of every source's candidates (the home image's and the host's too), and every other image's rows
    // THERE are folded.  A slot outside the union has no disagreeing read in any source: a = 0 in the sum, GT = 0, never a call, whatever part of r it holds.
    if (n > 1) {
        std::vector<uint32_t> all; int badImage = -1;
        rc = pu.candidatesUnion(feeders, n, true, *genome, all, &badImage, err); if (rc != 0) { *folded = anyAdded ? 2 : 0; return rc; }
        rc = pu.foldOnce(feeders, n, false, &all, &foldedSlots, &anyAdded, &bad); if (rc != 0) return failed(bad);
    }
    *folded = 1;
    const double t1 = nowMs(); msFold = t1 - t0;
    uint64_t nCalls = 0; rc = ygpu_snv_call_size(home, &P, &nCalls);
    if (rc == 0) { calls.assign((size_t)nCalls, ygpu_snv_call{}); rc = ygpu_snv_collect(home, calls.data()); }
    if (rc != 0) { err = ygpu_last_error(home); calls.clear(); return rc; }
    msSelect = nowMs() - t1;
    return 0;
}

int SnvTrack::callOnHost(PileupTrack &pu, ygpu_ctx *const *feeders, int n, bool withHost, std::string &err)
{
    const double t0 = nowMs();
    std::vector<uint32_t> all, rows; int failed = -1;
    const int rc = pu.unionRows(feeders, n, withHost, false, *genome, all, rows, &failed, err); if (rc != 0) return rc;
    const ydepth::Layout L{pu.seqs.start.data(), pu.seqs.length.data(), pu.binBase.data(), (uint32_t)pu.seqs.start.size(), 1u, pu.minMapq};
    calls.clear();
    for (size_t i = 0; i < all.size(); i++) {
        ygpu_snv_call c;
        if (ysnv::judgeAt(L, genome->bases, genome->nBaseBytes, all[i], rows.data() + i * ypileup::NCH, P, &c)) calls.push_back(c);
    }
    msSelect = nowMs() - t0;
    return 0;
}

bool SnvTrack::finish(FILE *mainOut, FILE *log, bool timing)
{
    PileupTrack &pu = shared ? *shared : *own;
    std::vector<ygpu_ctx *> feedCtx; std::vector<int> feedDev; pu.feeders(feedCtx, feedDev);
    bool ok = true; std::string err; int folded = 0;
    if (deviceEntryPoints() && getenv("YAHA_HOST_SNV") == nullptr && !feedCtx.empty()) {
        const int rc = callOnDevice(pu, feedCtx.data(), (int)feedCtx.size(), &folded, err);
        if (rc == 0) onDevice = true;
        else {
            fprintf(log, "-osnv: calling on device %d failed (%d): %s%s\n", feedDev[0], rc, err.c_str(),
                folded == 2 ? " -- its array holds a part of the other sources: no calls" : "; the host calls instead");
            if (folded == 2) ok = false;
        }
    }
    if (ok && !onDevice) {
        const bool oneImage = folded == 1;                                  // everything was folded: the one image's array is the sum
        const int rc = callOnHost(pu, feedCtx.data(), oneImage ? 1 : (int)feedCtx.size(), !oneImage, err);
        if (rc != 0) { fprintf(log, "-osnv: collecting the pileup for the calls failed (%d): %s\n", rc, err.c_str()); ok = false; }
    }
    nHet = nHom = 0;
    for (const ygpu_snv_call &c : calls) (ysnv::infoGt(c.info) == 1u ? nHet : nHom)++;
    if (fflush(mainOut) != 0) ok = false;
    const double w0 = nowMs();
    if (ok && !write(file.c_str(), err)) { fprintf(log, "%s\n", err.c_str()); ok = false; }
    msWrite = nowMs() - w0;
    if (timing) fprintf(stderr, "[yaha] -osnv: %llu slots folded in %.1f ms, %llu calls selected on the %s in %.1f ms, file written in %.1f ms\n",
        (unsigned long long)foldedSlots, msFold, (unsigned long long)calls.size(), onDevice ? "device" : "host", msSelect, msWrite);
    return ok;
}

void SnvTrack::stats(std::string &line) const
{
    char t[256]; snprintf(t, sizeof t, ", \"snv_calls\": %llu, \"snv_het\": %llu, \"snv_hom\": %llu, \"snv_on_device\": %d, \"snv_folded_slots\": %llu",
        (unsigned long long)calls.size(), (unsigned long long)nHet, (unsigned long long)nHom, onDevice ? 1 : 0, (unsigned long long)foldedSlots);
    line += t;
}

// VCF 4.2: the header -- the options, one contig line per sequence in index order, the fields -- then one line per call, ascending by slot: POS is 1-based, ID
// is '.', FILTER is PASS, INFO has DP (reads that show A, C, G or T) and OT (reads that show N or a deletion), the one sample `yaha` has GT (0/1 or 1/1), GQ,
// DP, AD (reference, alt) and PL (the three normalised likelihoods in whole phred).  The letters come from the record's info word alone.
bool SnvTrack::write(const char *path, std::string &err) const
{
    FILE *f = !strcmp(path, "stdout") ? stdout : fopen(path, "w");
    if (!f) { err = std::string("Failure to open the SNV calls file: ") + path + "."; return false; }
    const Genome &g = *genome; const PileupTrack &pu = shared ? *shared : *own;
    bool ok = fprintf(f, "##fileformat=VCFv4.2\n##source=yaha_amd %s\n", options.c_str()) > 0;
    ok = ok && fprintf(f, "##yaha_costs=<match=%u,error=%u,het=%u>\n", P.cost_match, P.cost_error, P.cost_het) > 0;
    ok = ok && fputs("##yaha_note=single-nucleotide variants only: insertions and deletions are not called here (-oid holds them)\n", f) >= 0;
    for (size_t s = 0; s < g.seqs.size() && ok; s++) ok = fprintf(f, "##contig=<ID=%s,length=%u>\n", g.seqs[s].name.c_str(), g.seqs[s].length) > 0;
    ok = ok && fputs("##INFO=<ID=DP,Number=1,Type=Integer,Description=\"Reads that show A, C, G or T at the site\">\n"
                     "##INFO=<ID=OT,Number=1,Type=Integer,Description=\"Reads that show N or a deletion at the site (not modelled)\">\n"
                     "##FORMAT=<ID=GT,Number=1,Type=String,Description=\"Genotype\">\n"
                     "##FORMAT=<ID=GQ,Number=1,Type=Integer,Description=\"Genotype quality: the second smallest PL, at most 99\">\n"
                     "##FORMAT=<ID=DP,Number=1,Type=Integer,Description=\"Reads that show A, C, G or T at the site\">\n"
                     "##FORMAT=<ID=AD,Number=R,Type=Integer,Description=\"Reads that show the reference base and the alternate base\">\n"
                     "##FORMAT=<ID=PL,Number=G,Type=Integer,Description=\"Normalised phred-scaled genotype likelihoods\">\n"
                     "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tyaha\n", f) >= 0;
    size_t s = 0;
    for (size_t i = 0; i < calls.size() && ok; i++) {
        const ygpu_snv_call &c = calls[i];
        while (s + 1 < g.seqs.size() && c.slot >= pu.binBase[s + 1]) s++;
        const uint32_t gt = ysnv::infoGt(c.info);
        ok = fprintf(f, "%s\t%u\t.\t%c\t%c\t%u\tPASS\tDP=%u;OT=%u\tGT:GQ:DP:AD:PL\t%s:%u:%u:%u,%u:%u,%u,%u\n", g.seqs[s].name.c_str(), c.slot - pu.binBase[s] + 1u,
            kFourBitChars[ysnv::infoRefCode(c.info)], "ACGT"[ysnv::infoAlt(c.info) & 3u], c.qual, c.depth, c.other, gt == 1u ? "0/1" : "1/1", c.gq, c.depth, c.ref_count,
            c.alt_count, c.pl[0] / 100u, c.pl[1] / 100u, c.pl[2] / 100u) > 0;
    }
    if (f == stdout) ok = fflush(f) == 0 && ok; else ok = fclose(f) == 0 && ok;
    if (!ok) err = std::string("Failure writing the SNV calls file: ") + path + ".";
    return ok;
}
}  // namespace yaha
