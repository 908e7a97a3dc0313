// args.cpp -- command line, defaults and derived parameters.  Same option names, defaults, value checks and
// file-name derivation as the reference CLI (Main.c:187-565, AlignArgs.c:27-169) so that
// `yaha -g genome.fa` / `yaha -x index -q reads ...` keep working unchanged.  Extra options of this
// implementation: -gpus N (shard batches over N devices), -ctx M (contexts per device), -device D, -batch N (reads per device batch),
// -ocov FILE / -covbin B / -covq Q (read depth of the printed records as bedGraph), -oev FILE / -evbin B / -evq Q / -evclip N (their mismatches, indels and
// clipped ends per bin), -obp FILE / -bpq Q / -bpw W (split-read breakpoint calls as BEDPE), -opu FILE / -pumin N / -puq Q (the allele pileup: the sites where
// at least N reads disagree with the reference, with the counts of A C G T N del ins), -oid FILE / -idmin N / -idlen L / -idq Q (indel alleles: position,
// length and inserted bases of the insertions and deletions at least N printed records carry), -oep FILE / -epq Q (the error profile of the printed records:
// substitution spectrum, indel lengths, identity, errors by position in the read), -osnv FILE / -snverr E / -snvmin N / -snvdp D / -snvqual Q (SNV calls with
// genotypes as VCF 4.2, judged on the device from the pileup array; their mapping-quality gate is -puq).
#include "yaha_host.h"
#include <cstring>
#include <cstdlib>
#include <algorithm>

namespace yaha {

static void usage(FILE *o)
{
    fputs("Usage (defaults in parentheses):\n\n"
          "Index creation:\n"
          "  yaha -g genome.{fa|fna|fasta|nib2} [-H maxHits (65525)] [-L wordLen (15)] [-S skipDist (1)] [-device D (0)] [-cpuindex]\n"
          "  yaha -g genome.{fa|fna|fasta} -c   (compress to genome.nib2 only)      yaha -g genome.nib2 -u   (back to genome.fasta)\n"
          "       (built on the GPU when one is visible, for any -S; -cpuindex forces the host builder; the files are identical)\n\n"
          "Query alignment (hot path on MI355X):\n"
          "  yaha -x indexFile [-q queryFile|(stdin)] [-o8|(-osh)|-oss|-obh|-obs outFile|(stdout)] [-obsort [-sortmem GB (32)]] [-t hostThreads (1)]\n"
          "       [-gpus N (1)] [-ctx contextsPerGpu (3)] [-device D (0)] [-batch readsPerBatch (about 16 M bases)] [-dpf Y|N (Y: post-filter on the device)]\n"
          "  general : [-BW 5] [-G 50] [-H 650] [-M 25] [-MD 50] [-P 0.9] [-X 25]\n"
          "  scoring : [-AGS Y|N] [-GEC 2] [-GOC 5] [-MS 1] [-RC 3]\n"
          "  OQC     : [-OQC Y|N] [-BP 5] [-MGDP 5] [-MNO minMatch]   FBS: [-FBS Y|N] [-PRL 0.9] [-PSS 0.9]\n"
          "  -o8 modified Blast8, -osh SAM hard clipping, -oss SAM soft clipping.\n"
          "  -obh BAM hard clipping, -obs BAM soft clipping: the records of -osh / -oss in BAM's layout, unsorted, in BGZF blocks deflated on the device\n"
          "       (fixed Huffman codes; YAHA_HOST_BGZF=1: on the host).  The blocks' boundaries follow -batch and -ctx, the decompressed stream does not.\n"
          "  -obsort (with -obh / -obs FILE) [-sortmem GB (32)]: the BAM in coordinate order -- sequence, position, equal keys in print order -- and its index\n"
          "       FILE.bai, both written after the last alignment; the decompressed stream does not depend on -batch, -ctx, -gpus or -t.  The whole run's records\n"
          "       stay in the memory of device -device until then (about 1.7 KB per 1 kbp read with qualities; -sortmem caps it), are ordered there by a radix\n"
          "       sort and go from there into the deflate kernels.  There is NO spill: sorted runs are not written to disk and merged -- when the store would pass\n"
          "       -sortmem the run stops, says so and leaves no file behind.  A sequence over 2^29 bases cannot be indexed by BAI: the run stops before the\n"
          "       first batch.  YAHA_HOST_BAMSORT=1: store and order on the host; YAHA_SORTMEM_BYTES=N: the cap in bytes (for tests).  Errors in these two\n"
          "       options leave with exit code 2.\n"
          "  depth   : [-ocov depthFile|stdout] [-covbin basesPerBin (100)] [-covq minMapQ (0)]\n"
          "       read depth of the printed records along the reference (bases under M of the CIGAR) as bedGraph, written after the last alignment;\n"
          "       accumulated on the device behind its post-filter: 4 bytes a bin of device memory per GPU -- -covbin 1 on a 3.1 Gbp genome is 12.4 GB beside the\n"
          "       contexts' arenas; when that does not fit the run stops before the first batch and says so (use a larger bin or a smaller -ctx).\n"
          "  events  : [-oev eventsFile|stdout] [-evbin basesPerBin (100)] [-evq minMapQ (0)] [-evclip minClippedBases (1)]\n"
          "       where the printed records disagree with the reference or stop, per bin (the bins of -ocov): mismatched bases, deleted bases, insertions,\n"
          "       records clipped by at least -evclip bases at their left / right end; tab-separated with a header line, bins without events left out, written\n"
          "       after the last alignment.  Accumulated on the device like the depth: 20 bytes a bin of device memory per GPU -- -evbin 1 on a 3.1 Gbp genome\n"
          "       is 62 GB; when that does not fit the run stops before the first batch and says so (use a larger bin).\n"
          "  breakpoints : [-obp bedpeFile|stdout] [-bpq minMapQ (0)] [-bpw clusterWindow (10)]\n"
          "       where the printed primary alignments of a read join: its records with mapping quality of at least -bpq, ordered along the read, give one\n"
          "       junction per neighbouring pair (made on the device behind its post-filter); junctions of the same sequences and strands within -bpw bases\n"
          "       of a cluster's first member on both sides are one cluster.  One BEDPE line per cluster, written after the last alignment: chromA, startA,\n"
          "       endA, chromB, startB, endB, type (DEL, DUP, INV, TRA), supporting junctions, strandA, strandB, least and largest gap on the read (negative:\n"
          "       the pieces overlap).\n"
          "  pileup  : [-opu sitesFile|stdout] [-pumin minDisagreeingReads (2)] [-puq minMapQ (0)]\n"
          "       which base the printed records carry at every reference base (A C G T N, deleted, an insertion before it), and the sites where at least -pumin\n"
          "       of them disagree with the reference: tab-separated with a header line -- chrom, start (0-based), end = start + 1, ref, A, C, G, T, N, del, ins --\n"
          "       in index order, written after the last alignment.  Accumulated on the device like the depth, per reference base: 28 bytes of device memory per\n"
          "       reference base per GPU, which is 86.8 GB at 3.1 Gbp; the sites are selected on the device and only they leave it.  When the array does not fit\n"
          "       the run stops before the first batch and says so (use a smaller -ctx).  The host keeps counts only for the records it counts itself, in blocks\n"
          "       of 4096 reference bases (112 KB each) made when first touched.  Errors in these three options leave with exit code 3 (the other tracks': 2).\n"
          "  indels  : [-oid allelesFile|stdout] [-idmin minRecords (2)] [-idlen minBases (1)] [-idq minMapQ (0)]\n"
          "       the insertions and deletions of at least -idlen bases that at least -idmin printed records carry, as alleles: tab-separated, no header line --\n"
          "       chrom, position (1-based: a deletion's first deleted base, an insertion's next reference base), DEL or INS, length, the inserted bases as the\n"
          "       reference strand shows them (the first 42, then '+'; '*' for a deletion), records -- in index order, written after the last alignment.  Counted\n"
          "       on the device behind its post-filter in a hash table per context (32 bytes an entry, two entries per base of a batch: 1 GB at the default\n"
          "       batch), which the host drains whenever a quarter of it is in use.  Errors in these four options leave with exit code 2.\n"
          "  errors  : [-oep profileFile|stdout] [-epq minMapQ (0)]\n"
          "       how good the printed records are, tab-separated, every line with its section's name first, written after the last alignment: SUB -- aligned\n"
          "       bases by reference base (rows) and read base (columns), A C G T N --, INS and DEL -- insertions and deletions by length, 1 to 65+ --, IDENT --\n"
          "       records by identity in per mille: matching bases / (aligned + inserted + deleted bases) --, POS -- aligned bases, those that differ, insertions\n"
          "       and deletions by position in the read as sequenced, in hundredths of its length.  The first line has the records counted, left out by -epq\n"
          "       and dropped.  Counted on the device behind its post-filter, in a table of 12 KB per context.  Errors in these two options leave with exit\n"
          "       code 3.\n"
          "  SNVs    : [-osnv callsFile|stdout] [-snverr errorPerMille (100)] [-snvmin minAltReads (2)] [-snvdp minDepth (4)] [-snvqual minQual (20)] [-puq minMapQ (0)]\n"
          "       the sites where the pileup of the printed records says the sample differs from the reference, as VCF 4.2 with one sample, written after the last\n"
          "       alignment: r reads show the reference's base, a the most frequent other base of A C G T; the genotypes 0/0, 0/1 and 1/1 cost r cM + a cE,\n"
          "       (r + a) cH and r cE + a cM in 1/100 phred, the three costs derived from -snverr (46, 1477, 331 at 100); GT is the cheapest, QUAL what 0/0 costs\n"
          "       more (at most 9999), GQ what the second cheapest costs more (at most 99).  A line needs GT 0/1 or 1/1, a >= -snvmin, A + C + G + T >= -snvdp and\n"
          "       QUAL >= -snvqual.  Indels are not called (-oid holds them).  The counts are the pileup's (-opu; 28 bytes of device memory per reference base per\n"
          "       GPU, made for -osnv alone as well, with -puq as its gate); the sites are judged on the device and only the calls leave it.  With -gpus N the\n"
          "       other devices' candidate sites are added to the first one's array before that, which moves what -opu moves.  YAHA_HOST_SNV=1: judged on the\n"
          "       host.  Errors in these five options leave with exit code 3.\n"
          "  indels  : [-oindel callsFile|stdout] [-inderr errorPerMille (50)] [-indmin minAltReads (2)] [-inddp minDepth (4)] [-indqual minQual (20)]\n"
          "            [-indshift maxShift (256)] [-puq minMapQ (0)]\n"
          "       the insertions and deletions of the printed records as genotyped calls, VCF 4.2 with one sample, written after the last alignment.  Every\n"
          "       allele -oid would list (any length, gate -puq) is moved left along the reference while its last base equals the base before it, at most\n"
          "       -indshift bases (0: not at all) and never out of its sequence or across an N; alleles that become equal are one, their records add up.  POS is\n"
          "       the base before the event (the anchor).  d reads cover the anchor (A C G T N del of the pileup there), a carry the allele, r = d - a do not:\n"
          "       0/0, 0/1 and 1/1 cost r cM + a cE, (r + a) cH and r cE + a cM in 1/100 phred, the costs derived from -inderr (22, 1301, 301 at 50); GT, QUAL\n"
          "       and GQ as for -osnv.  A line needs GT 0/1 or 1/1, a >= -indmin, d >= -inddp and QUAL >= -indqual.  Insertions of more than 42 bases are\n"
          "       not called.  Shares the arrays of -opu / -osnv and the table of -oid (which must then run with -idlen 1 and -idq equal to -puq); normalised,\n"
          "       merged and judged on the device, only the calls leave it.  YAHA_HOST_INDELCALL=1: on the host.  Errors in these options leave with exit code 3.\n", o);
}

static bool parseBool(const char *s, const char *key, bool &out)
{
    if (strlen(s) == 1) { if (strchr("YyTt", s[0])) { out = true; return true; } if (strchr("NnFf", s[0])) { out = false; return true; } }
    fprintf(stderr, "%s is not a valid value for parameter %s.\nUse one of 'YyTt' for Yes and 'NnFf' for No.\n\n", s, key); usage(stderr); return false;
}
static bool parseInt(const char *s, const char *key, int &out)
{
    out = atoi(s);
    if (out < 0) { fprintf(stderr, "%s is not a valid value for parameter %s.\nValue must be a positive integer.\n\n", s, key); usage(stderr); return false; }
    return true;
}
static bool parseFloat(const char *s, const char *key, float &out)
{
    out = (float)atof(s);                                           // float on purpose: Main.c:161-171
    if (out <= 0.0 || out > 1.0) { fprintf(stderr, "%s is not a valid value for parameter %s.\nValue must be in the range 0<value<=1.0.\n\n", s, key); usage(stderr); return false;
        }
    return true;
}

// (parseArgs returns the exit code + 1: the pileup's argument errors leave with 3 -- as its specification asks, and as the usage text says; the older tracks'
// leave with 2; the error profile's with 3 as well)
static const int kPileupError = 4;

int parseArgs(int argc, char **argv, Args &a)
{
    if (argc <= 1) { usage(stderr); return 1; }
    bool query = false, index = true;
    for (int x = 1; x < argc; x++) {
        const char *k = argv[x]; auto is = [&](const char *s) { return strcmp(k, s) == 0; };
        auto val = [&]() -> const char * { x++; return x < argc ? argv[x] : ""; };
        if (is("-h") || is("-?") || is("-xh")) { usage(stderr); return 1; }
        else if (is("-g")) { a.gfileName = val(); a.haveG = true; }
        // deliberate fix of Main.c:173-178, which turns these into "stdout" and then fails to open it
        else if (is("-q")) { const char *v = val(); a.qfileName = (!strcmp(v, "-") || !strcmp(v, "-stdin") || !strcmp(v, "stdin")) ? "stdin" : v; query = true; index = false; }
        else if (is("-o8")) { a.outputBlast8 = true; a.outputSAM = false; a.outputBAM = false; const char *v = val(); a.ofileName = (!strcmp(v, "-stdout")) ? "stdout" : v;
            a.haveO = true; }
        else if (is("-osh")) { a.outputBlast8 = false; a.outputSAM = true; a.outputBAM = false; a.hardClip = true; const char *v = val();
            a.ofileName = (!strcmp(v, "-stdout")) ? "stdout" : v;
            a.haveO = true; }
        else if (is("-oss")) { a.outputBlast8 = false; a.outputSAM = true; a.outputBAM = false; a.hardClip = false; const char *v = val();
            a.ofileName = (!strcmp(v, "-stdout")) ? "stdout" : v; a.haveO = true; }
        // BAM: the SAM writer's records in binary, hard (-obh) or soft (-obs) clipped; an output selector like the three above -- the last one given wins
        else if (is("-obh") || is("-obs")) { a.outputBlast8 = false; a.outputSAM = true; a.outputBAM = true; a.hardClip = is("-obh"); const char *v = val();
            a.ofileName = (!strcmp(v, "-stdout")) ? "stdout" : v; a.haveO = true; }
        // -obsort: the BAM of -obh / -obs in coordinate order with its index; -sortmem: the cap of the record store in GB
        else if (is("-obsort")) a.bamSort = true;
        else if (is("-sortmem")) { if (!parseInt(val(), "-sortmem", a.sortMemGB)) return 3; a.haveSortMem = true;
            if (a.sortMemGB < 1) { fprintf(stderr, "-sortmem must be at least 1 (GB).\n\n"); usage(stderr); return 3; } }
        else if (is("-t")) { if (!parseInt(val(), "-t", a.numThreads)) return 2; }
        else if (is("-v")) a.verbose = true;
        else if (is("-x")) { a.xfileName = val(); a.haveX = true; query = true; index = false; }
        else if (is("-H")) { if (!parseInt(val(), "-H", a.maxHits)) return 2; }
        else if (is("-L")) { if (!parseInt(val(), "-L", a.wordLen)) return 2; }
        else if (is("-S")) { if (!parseInt(val(), "-S", a.skipDist)) return 2; }
        else if (is("-BW")) { if (!parseInt(val(), "-BW", a.bandWidth)) return 2; }
        else if (is("-G")) { if (!parseInt(val(), "-G", a.maxGap)) return 2; }
        else if (is("-M")) { if (!parseInt(val(), "-M", a.minMatch)) return 2; }
        else if (is("-MD")) { if (!parseInt(val(), "-MD", a.maxDesert)) return 2; }
        else if (is("-P")) { if (!parseFloat(val(), "-P", a.minIdentity)) return 2; }
        else if (is("-X")) { if (!parseInt(val(), "-X", a.XCutoff)) return 2; }
        else if (is("-AGS")) { if (!parseBool(val(), "-AGS", a.affineGapScoring)) return 2; }
        else if (is("-GEC")) { if (!parseInt(val(), "-GEC", a.GECost)) return 2; }
        else if (is("-GOC")) { if (!parseInt(val(), "-GOC", a.GOCost)) return 2; }
        else if (is("-MS")) { if (!parseInt(val(), "-MS", a.MScore)) return 2; }
        else if (is("-RC")) { if (!parseInt(val(), "-RC", a.RCost)) return 2; }
        else if (is("-OQC")) { if (!parseBool(val(), "-OQC", a.OQC)) return 2; }
        else if (is("-BP")) { if (!parseInt(val(), "-BP", a.BPCost)) return 2; }
        else if (is("-MGDP")) { if (!parseInt(val(), "-MGDP", a.maxBPLog)) return 2; }
        else if (is("-MNO")) { if (!parseInt(val(), "-MNO", a.OQCMinNonOverlap)) return 2; }
        else if (is("-FBS")) { if (!parseBool(val(), "-FBS", a.FBS)) return 2; }
        else if (is("-PRL")) { if (!parseFloat(val(), "-PRL", a.FBS_PSLength)) return 2; }
        else if (is("-PSS")) { if (!parseFloat(val(), "-PSS", a.FBS_PSScore)) return 2; }
        else if (is("-I")) { if (!parseInt(val(), "-I", a.maxIntron)) return 2; }          // experimental builds of the reference, Main.c:418-435
        else if (is("-R")) { if (!parseInt(val(), "-R", a.minRawScore)) return 2; }
        else if (is("-c")) { a.compress = true; index = false; }                                // the two below: Main.c:284-293 (builds of the reference without COMPILE_USER_MODE)
        else if (is("-u")) { a.uncompress = true; index = false; }
        else if (is("-gpus")) { if (!parseInt(val(), "-gpus", a.gpus)) return 2; if (a.gpus < 1) { fprintf(stderr, "-gpus must be at least 1.\n\n"); usage(stderr); return 2; } }
        else if (is("-ctx")) { if (!parseInt(val(), "-ctx", a.ctxPerGpu)) return 2; if (a.ctxPerGpu < 1 || a.ctxPerGpu > 8) { fprintf(stderr, "-ctx must be between 1 and 8.\n\n");
            usage(stderr); return 2; } }
        else if (is("-device")) { if (!parseInt(val(), "-device", a.device)) return 2; }
        else if (is("-cpuindex")) a.cpuIndex = true;
        else if (is("-dpf")) { if (!parseBool(val(), "-dpf", a.devicePostFilter)) return 2; }        // post-filter (OQC / FBS / MAPQ) on the device (default) or on the host
        else if (is("-batch")) { if (!parseInt(val(), "-batch", a.batchReads)) return 2;
                                 if (a.batchReads < 1 || a.batchReads > 65536) { fprintf(stderr, "-batch must be between 1 and 65536 (reads per device batch).\n\n"); usage(stderr);
                                     return 2; } }
        else if (is("-ocov")) { const char *v = val(); a.covFileName = (!strcmp(v, "-stdout")) ? "stdout" : v; a.haveCov = true;
            if (a.covFileName.empty()) { fprintf(stderr, "-ocov needs a file name.\n\n"); usage(stderr); return 3; } }
        else if (is("-covbin")) { if (!parseInt(val(), "-covbin", a.covBin)) return 3; a.haveCovBin = true;
            if (a.covBin < 1) { fprintf(stderr, "-covbin must be at least 1 (bases per bin).\n\n"); usage(stderr); return 3; } }
        else if (is("-covq")) { if (!parseInt(val(), "-covq", a.covMinQ)) return 3; a.haveCovQ = true; }
        else if (is("-oev")) { const char *v = val(); a.evFileName = (!strcmp(v, "-stdout")) ? "stdout" : v; a.haveEv = true;
            if (a.evFileName.empty()) { fprintf(stderr, "-oev needs a file name.\n\n"); usage(stderr); return 3; } }
        else if (is("-evbin")) { if (!parseInt(val(), "-evbin", a.evBin)) return 3; a.haveEvBin = true;
            if (a.evBin < 1) { fprintf(stderr, "-evbin must be at least 1 (bases per bin).\n\n"); usage(stderr); return 3; } }
        else if (is("-evq")) { if (!parseInt(val(), "-evq", a.evMinQ)) return 3; a.haveEvQ = true; }
        else if (is("-evclip")) { if (!parseInt(val(), "-evclip", a.evMinClip)) return 3; a.haveEvClip = true;
            if (a.evMinClip < 1) { fprintf(stderr, "-evclip must be at least 1 (clipped bases).\n\n"); usage(stderr); return 3; } }
        else if (is("-obp")) { const char *v = val(); a.bpFileName = (!strcmp(v, "-stdout")) ? "stdout" : v; a.haveBp = true;
            if (a.bpFileName.empty()) { fprintf(stderr, "-obp needs a file name.\n\n"); usage(stderr); return 3; } }
        else if (is("-bpq")) { if (!parseInt(val(), "-bpq", a.bpMinQ)) return 3; a.haveBpQ = true;
            if (a.bpMinQ < 0 || a.bpMinQ > 255) { fprintf(stderr, "-bpq must be a mapping quality (0 to 255).\n\n"); usage(stderr); return 3; } }
        else if (is("-bpw")) { if (!parseInt(val(), "-bpw", a.bpWindow)) return 3; a.haveBpW = true;
            if (a.bpWindow < 0) { fprintf(stderr, "-bpw must not be negative (bases).\n\n"); usage(stderr); return 3; } }
        else if (is("-opu")) { const char *v = val(); a.puFileName = (!strcmp(v, "-stdout")) ? "stdout" : v; a.havePu = true;
            if (a.puFileName.empty()) { fprintf(stderr, "-opu needs a file name.\n\n"); usage(stderr); return kPileupError; } }
        else if (is("-pumin")) { if (!parseInt(val(), "-pumin", a.puMinAlt)) return kPileupError; a.havePuMin = true;
            if (a.puMinAlt < 1) { fprintf(stderr, "-pumin must be at least 1 (reads that disagree with the reference).\n\n"); usage(stderr); return kPileupError; } }
        else if (is("-puq")) { if (!parseInt(val(), "-puq", a.puMinQ)) return kPileupError; a.havePuQ = true; }
        else if (is("-oid")) { const char *v = val(); a.idFileName = (!strcmp(v, "-stdout")) ? "stdout" : v; a.haveId = true;
            if (a.idFileName.empty()) { fprintf(stderr, "-oid needs a file name.\n\n"); usage(stderr); return 3; } }
        else if (is("-idmin")) { if (!parseInt(val(), "-idmin", a.idMin)) return 3; a.haveIdMin = true;
            if (a.idMin < 1) { fprintf(stderr, "-idmin must be at least 1 (records that carry the allele).\n\n"); usage(stderr); return 3; } }
        else if (is("-idlen")) { if (!parseInt(val(), "-idlen", a.idLen)) return 3; a.haveIdLen = true;
            if (a.idLen < 1) { fprintf(stderr, "-idlen must be at least 1 (inserted or deleted bases).\n\n"); usage(stderr); return 3; } }
        else if (is("-idq")) { if (!parseInt(val(), "-idq", a.idMinQ)) return 3; a.haveIdQ = true;
            if (a.idMinQ < 0 || a.idMinQ > 255) { fprintf(stderr, "-idq must be a mapping quality (0 to 255).\n\n"); usage(stderr); return 3; } }
        else if (is("-oep")) { const char *v = val(); a.epFileName = (!strcmp(v, "-stdout")) ? "stdout" : v; a.haveEp = true;
            if (a.epFileName.empty()) { fprintf(stderr, "-oep needs a file name.\n\n"); usage(stderr); return kPileupError; } }
        else if (is("-epq")) { if (!parseInt(val(), "-epq", a.epMinQ)) return kPileupError; a.haveEpQ = true;
            if (a.epMinQ < 0 || a.epMinQ > 255) { fprintf(stderr, "-epq must be a mapping quality (0 to 255).\n\n"); usage(stderr); return kPileupError; } }
        else if (is("-osnv")) { const char *v = val(); a.snvFileName = (!strcmp(v, "-stdout")) ? "stdout" : v; a.haveSnv = true;
            if (a.snvFileName.empty()) { fprintf(stderr, "-osnv needs a file name.\n\n"); usage(stderr); return kPileupError; } }
        else if (is("-snverr")) { if (!parseInt(val(), "-snverr", a.snvErr)) return kPileupError; a.haveSnvErr = true;
            if (a.snvErr < 1 || a.snvErr > 500) { fprintf(stderr, "-snverr must be between 1 and 500 (sequencing error in per mille).\n\n"); usage(stderr); return kPileupError; } }
        else if (is("-snvmin")) { if (!parseInt(val(), "-snvmin", a.snvMin)) return kPileupError; a.haveSnvMin = true;
            if (a.snvMin < 1) { fprintf(stderr, "-snvmin must be at least 1 (reads that carry the allele).\n\n"); usage(stderr); return kPileupError; } }
        else if (is("-snvdp")) { if (!parseInt(val(), "-snvdp", a.snvDp)) return kPileupError; a.haveSnvDp = true;
            if (a.snvDp < 1) { fprintf(stderr, "-snvdp must be at least 1 (reads that show A, C, G or T).\n\n"); usage(stderr); return kPileupError; } }
        else if (is("-snvqual")) { if (!parseInt(val(), "-snvqual", a.snvQual)) return kPileupError; a.haveSnvQual = true; }
        else if (is("-oindel")) { const char *v = val(); a.indFileName = (!strcmp(v, "-stdout")) ? "stdout" : v; a.haveIndel = true;
            if (a.indFileName.empty()) { fprintf(stderr, "-oindel needs a file name.\n\n"); usage(stderr); return kPileupError; } }
        else if (is("-inderr")) { if (!parseInt(val(), "-inderr", a.indErr)) return kPileupError; a.haveIndErr = true;
            if (a.indErr < 1 || a.indErr > 500) { fprintf(stderr, "-inderr must be between 1 and 500 (error in per mille).\n\n"); usage(stderr); return kPileupError; } }
        else if (is("-indmin")) { if (!parseInt(val(), "-indmin", a.indMin)) return kPileupError; a.haveIndMin = true;
            if (a.indMin < 1) { fprintf(stderr, "-indmin must be at least 1 (reads that carry the allele).\n\n"); usage(stderr); return kPileupError; } }
        else if (is("-inddp")) { if (!parseInt(val(), "-inddp", a.indDp)) return kPileupError; a.haveIndDp = true;
            if (a.indDp < 1) { fprintf(stderr, "-inddp must be at least 1 (reads that cover the anchor base).\n\n"); usage(stderr); return kPileupError; } }
        else if (is("-indqual")) { if (!parseInt(val(), "-indqual", a.indQual)) return kPileupError; a.haveIndQual = true; }
        else if (is("-indshift")) { if (!parseInt(val(), "-indshift", a.indShift)) return kPileupError; a.haveIndShift = true;
            if (a.indShift > 65535) { fprintf(stderr, "-indshift must be between 0 and 65535 (bases an allele may move).\n\n"); usage(stderr); return kPileupError; } }
        else { fprintf(stderr, "%s is not a valid option.\n\n", k); usage(stderr); return 2; }
    }
    a.query = query; a.index = index && !query;
    // the read-depth track (exit code 2 for its errors): a query run's output only, its options need it, and it cannot share standard output with the alignments
    if (!a.haveCov && (a.haveCovBin || a.haveCovQ)) { fprintf(stderr, "-covbin and -covq need -ocov.\n\n"); usage(stderr); return 3; }
    if (a.haveCov && !query) { fprintf(stderr, "-ocov is an output of query alignment; it is not allowed during index creation.\n\n"); usage(stderr); return 3; }
    if (a.haveCov && a.covFileName == "stdout" && (!a.haveO || a.ofileName == "stdout")) {
        fprintf(stderr, "-ocov stdout: the alignments already go to standard output; give one of them a file.\n\n"); usage(stderr); return 3; }
    // the evidence track: the same rules, and the two tracks cannot share standard output either
    if (!a.haveEv && (a.haveEvBin || a.haveEvQ || a.haveEvClip)) { fprintf(stderr, "-evbin, -evq and -evclip need -oev.\n\n"); usage(stderr); return 3; }
    if (a.haveEv && !query) { fprintf(stderr, "-oev is an output of query alignment; it is not allowed during index creation.\n\n"); usage(stderr); return 3; }
    if (a.haveEv && a.evFileName == "stdout" && (!a.haveO || a.ofileName == "stdout")) {
        fprintf(stderr, "-oev stdout: the alignments already go to standard output; give one of them a file.\n\n"); usage(stderr); return 3; }
    if (a.haveEv && a.haveCov && a.evFileName == "stdout" && a.covFileName == "stdout") {
        fprintf(stderr, "-oev stdout: the depth track (-ocov) already goes to standard output; give one of them a file.\n\n"); usage(stderr); return 3; }
    // the breakpoint calls: the same rules once more
    if (!a.haveBp && (a.haveBpQ || a.haveBpW)) { fprintf(stderr, "-bpq and -bpw need -obp.\n\n"); usage(stderr); return 3; }
    if (a.haveBp && !query) { fprintf(stderr, "-obp is an output of query alignment; it is not allowed during index creation.\n\n"); usage(stderr); return 3; }
    if (a.haveBp && a.bpFileName == "stdout" && (!a.haveO || a.ofileName == "stdout")) {
        fprintf(stderr, "-obp stdout: the alignments already go to standard output; give one of them a file.\n\n"); usage(stderr); return 3; }
    if (a.haveBp && a.bpFileName == "stdout" && ((a.haveCov && a.covFileName == "stdout") || (a.haveEv && a.evFileName == "stdout"))) {
        fprintf(stderr, "-obp stdout: another track already goes to standard output; give one of them a file.\n\n"); usage(stderr); return 3; }
    // the allele pileup: the same rules, its errors with an exit code of their own (3)
    if (!a.havePu && (a.havePuMin || (a.havePuQ && !a.haveSnv && !a.haveIndel))) { fprintf(stderr, "-pumin needs -opu, -puq needs -opu, -osnv or -oindel.\n\n"); usage(stderr);
        return kPileupError; }
    if (a.havePu && !query) { fprintf(stderr, "-opu is an output of query alignment; it is not allowed during index creation.\n\n"); usage(stderr); return kPileupError; }
    if (a.havePu && a.puFileName == "stdout" && (!a.haveO || a.ofileName == "stdout")) {
        fprintf(stderr, "-opu stdout: the alignments already go to standard output; give one of them a file.\n\n"); usage(stderr); return kPileupError; }
    if (a.havePu && a.puFileName == "stdout" && ((a.haveCov && a.covFileName == "stdout") || (a.haveEv && a.evFileName == "stdout") || (a.haveBp && a.bpFileName == "stdout"))) {
        fprintf(stderr, "-opu stdout: another track already goes to standard output; give one of them a file.\n\n"); usage(stderr); return kPileupError; }
    // the indel alleles: the same rules, with the older tracks' exit code (2)
    if (!a.haveId && (a.haveIdMin || a.haveIdLen || a.haveIdQ)) { fprintf(stderr, "-idmin, -idlen and -idq need -oid.\n\n"); usage(stderr); return 3; }
    if (a.haveId && !query) { fprintf(stderr, "-oid is an output of query alignment; it is not allowed during index creation.\n\n"); usage(stderr); return 3; }
    if (a.haveId && a.idFileName == "stdout" && (!a.haveO || a.ofileName == "stdout")) {
        fprintf(stderr, "-oid stdout: the alignments already go to standard output; give one of them a file.\n\n"); usage(stderr); return 3; }
    if (a.haveId && a.idFileName == "stdout" && ((a.haveCov && a.covFileName == "stdout") || (a.haveEv && a.evFileName == "stdout") || (a.haveBp && a.bpFileName == "stdout")
        || (a.havePu && a.puFileName == "stdout"))) {
        fprintf(stderr, "-oid stdout: another track already goes to standard output; give one of them a file.\n\n"); usage(stderr); return 3; }
    // the error profile: the same rules, with the pileup's exit code (3)
    if (!a.haveEp && a.haveEpQ) { fprintf(stderr, "-epq needs -oep.\n\n"); usage(stderr); return kPileupError; }
    if (a.haveEp && !query) { fprintf(stderr, "-oep is an output of query alignment; it is not allowed during index creation.\n\n"); usage(stderr); return kPileupError; }
    if (a.haveEp && a.epFileName == "stdout" && (!a.haveO || a.ofileName == "stdout")) {
        fprintf(stderr, "-oep stdout: the alignments already go to standard output; give one of them a file.\n\n"); usage(stderr); return kPileupError; }
    if (a.haveEp && a.epFileName == "stdout" && ((a.haveCov && a.covFileName == "stdout") || (a.haveEv && a.evFileName == "stdout") || (a.haveBp && a.bpFileName == "stdout")
        || (a.havePu && a.puFileName == "stdout") || (a.haveId && a.idFileName == "stdout"))) {
        fprintf(stderr, "-oep stdout: another track already goes to standard output; give one of them a file.\n\n"); usage(stderr); return kPileupError; }
    // the SNV calls: the same rules, with the pileup's exit code (3); their mapping-quality gate is the pileup's -puq
    if (!a.haveSnv && (a.haveSnvErr || a.haveSnvMin || a.haveSnvDp || a.haveSnvQual)) { fprintf(stderr, "-snverr, -snvmin, -snvdp and -snvqual need -osnv.\n\n"); usage(stderr);
        return kPileupError; }
    if (a.haveSnv && !query) { fprintf(stderr, "-osnv is an output of query alignment; it is not allowed during index creation.\n\n"); usage(stderr); return kPileupError; }
    if (a.haveSnv && a.snvFileName == "stdout" && (!a.haveO || a.ofileName == "stdout")) {
        fprintf(stderr, "-osnv stdout: the alignments already go to standard output; give one of them a file.\n\n"); usage(stderr); return kPileupError; }
    if (a.haveSnv && a.snvFileName == "stdout" && ((a.haveCov && a.covFileName == "stdout") || (a.haveEv && a.evFileName == "stdout") || (a.haveBp && a.bpFileName == "stdout")
        || (a.havePu && a.puFileName == "stdout") || (a.haveId && a.idFileName == "stdout") || (a.haveEp && a.epFileName == "stdout"))) {
        fprintf(stderr, "-osnv stdout: another track already goes to standard output; give one of them a file.\n\n"); usage(stderr); return kPileupError; }
    // the indel calls: the same rules once more (exit code 3); they stand on the pileup's gate -puq and on alleles of every length counted with that gate
    if (!a.haveIndel && (a.haveIndErr || a.haveIndMin || a.haveIndDp || a.haveIndQual || a.haveIndShift)) {
        fprintf(stderr, "-inderr, -indmin, -inddp, -indqual and -indshift need -oindel.\n\n"); usage(stderr); return kPileupError; }
    if (a.haveIndel && !query) { fprintf(stderr, "-oindel is an output of query alignment; it is not allowed during index creation.\n\n"); usage(stderr); return kPileupError; }
    if (a.haveIndel && a.haveId && (a.idLen != 1 || a.idMinQ != a.puMinQ)) {
        fprintf(stderr, "-oindel shares the alleles of -oid: beside it -oid must run with -idlen 1 and -idq equal to -puq (%d).\n\n", a.puMinQ); usage(stderr); return kPileupError;
            }
    if (a.haveIndel && a.indFileName == "stdout" && (!a.haveO || a.ofileName == "stdout")) {
        fprintf(stderr, "-oindel stdout: the alignments already go to standard output; give one of them a file.\n\n"); usage(stderr); return kPileupError; }
    if (a.haveIndel && a.indFileName == "stdout" && ((a.haveCov && a.covFileName == "stdout") || (a.haveEv && a.evFileName == "stdout") || (a.haveBp && a.bpFileName == "stdout")
        || (a.havePu && a.puFileName == "stdout") || (a.haveId && a.idFileName == "stdout") || (a.haveEp && a.epFileName == "stdout")
        || (a.haveSnv && a.snvFileName == "stdout"))) {
        fprintf(stderr, "-oindel stdout: another track already goes to standard output; give one of them a file.\n\n"); usage(stderr); return kPileupError; }
    // the sorted BAM: an option of -obh / -obs with a file of its own beside theirs
    if (a.haveSortMem && !a.bamSort) { fprintf(stderr, "-sortmem needs -obsort.\n\n"); usage(stderr); return 3; }
    if (a.bamSort && !query) { fprintf(stderr, "-obsort is an option of query alignment; it is not allowed during index creation.\n\n"); usage(stderr); return 3; }
    if (a.bamSort && !a.outputBAM) { fprintf(stderr, "-obsort needs -obh or -obs as the output selector (the last one given wins).\n\n"); usage(stderr); return 3; }
    if (a.bamSort && a.ofileName == "stdout") { fprintf(stderr, "-obsort writes FILE and FILE.bai: the BAM cannot go to standard output.\n\n"); usage(stderr); return 3; }
    if ((a.compress || a.uncompress) && !query) {                                                  // Main.c:472-533: -c wants a FASTA genome, -u a .nib2
        if (!a.haveG) { fprintf(stderr, "Genome file specification (-g) is required for index creation.\n\n"); usage(stderr); return 2; }
        size_t dot = a.gfileName.rfind('.'); const std::string ext = dot == std::string::npos ? "" : a.gfileName.substr(dot);
        const bool fasta = ext == ".fna" || ext == ".fa" || ext == ".fasta";
        if (!fasta && ext != ".nib2") { fprintf(stderr, "Expecting a \".fa\", \".fna\", \".fasta\", or \".nib2\" genome file.\n"); return 2; }
        if (a.compress && !fasta) { fprintf(stderr, "Expecting a \".fa\", \".fna\", or \".fasta\" genome file.\n"); return 2; }
        if (a.uncompress && !a.compress && fasta) { fprintf(stderr, "Expecting a \".nib2\" genome file.\n"); return 2; }
        a.ofileName = a.gfileName.substr(0, dot) + (a.compress ? ".nib2" : ".fasta");
        postProcessArgs(a, false);
        return 0;
    }
    if (a.index) {
        if (!a.haveG) { fprintf(stderr, "Genome file specification (-g) is required for index creation.\n\n"); usage(stderr); return 2; }
        if (a.haveO) { fprintf(stderr, "Output file specification is not allowed during index creation.\n\n"); usage(stderr); return 2; }
    }
    if (query) {
        if (a.haveG) { fprintf(stderr, "Genome file specification (-g) is not allowed for query alignment.\n"); usage(stderr); return 2; }
        if (!a.haveX) { fprintf(stderr, "Index file specification (-x) is required for query alignment.\n"); usage(stderr); return 2; }
        size_t dot = a.xfileName.rfind('.');                             // Main.c:493-501
        if (dot == std::string::npos) { fprintf(stderr, "Specified index filename has improper or missing file extension.  Is it an index file?\n"); return 2; }
        a.gfileName = a.xfileName.substr(0, dot) + ".nib2";
        if (!a.haveO) { a.outputBlast8 = false; a.outputSAM = true; a.hardClip = true; a.ofileName = "stdout"; }
    }
    postProcessArgs(a, query);
    return 0;
}

void postProcessArgs(Args &a, bool query)
{
    if (a.maxIntron == -1) a.maxIntron = a.maxGap;
    if (a.minRawScore == -1) a.minRawScore = a.minMatch;
    if (a.OQCMinNonOverlap == -1) a.OQCMinNonOverlap = a.minMatch;
    if (a.OQCMinNonOverlap <= 0) { fprintf(stderr, "MNO parameter must be >=1.  MNO=1 will be used.\n"); a.OQCMinNonOverlap = 1; }
    if (a.minNonOverlap == -1) a.minNonOverlap = a.OQCMinNonOverlap;
    if (!a.affineGapScoring) { a.MScore = 1; a.RCost = a.GECost = 1; a.GOCost = 0; }
    int len = 1, score = 0, target = std::min(a.RCost, a.GOCost + a.GECost);
    while (score <= target) { score += a.MScore; len += 1; if (a.MScore <= 0) break; }
    a.minExtLength = (uint8_t)len;
    if (a.maxHits == -1) a.maxHits = query ? 650 : 0xFFFF - 10; else a.maxHits = std::min(a.maxHits, 0xFFFF - 10);
    if (a.maxBPLog < 1) { fprintf(stderr, "MGDP parameter must be between 1 and 9 (inclusive). MGDP=1 will be used.\n"); a.maxBPLog = 1; }
    if (a.maxBPLog > 9) { fprintf(stderr, "MGDP parameter must be between 1 and 9 (inclusive). MGDP=9 will be used.\n"); a.maxBPLog = 9; }
}

void paramsFromArgs(const Args &a, ygpu_params &p)
{
    p.wordLen = a.wordLen; p.maxHits = a.maxHits; p.bandWidth = a.bandWidth; p.maxGap = a.maxGap; p.maxIntron = a.maxIntron;
    p.minMatch = a.minMatch; p.maxDesert = a.maxDesert; p.minNonOverlap = a.minNonOverlap; p.minRawScore = a.minRawScore;
    p.minExtLength = a.minExtLength; p.GOCost = a.GOCost; p.GECost = a.GECost; p.RCost = a.RCost; p.MScore = a.MScore;
    p.XCutoff = a.XCutoff; p.minIdentity = a.minIdentity;
}

std::string samHeader(const Args &a, const Genome &g)                   // outputFileHeader, AlignOutput.c:30-111
{
    if (!a.outputSAM) return "";
    std::string h = a.bamSort ? "@HD\tVN:1.0\tSO:coordinate\n" : "@HD\tVN:1.0\n"; char buf[512];
    for (auto &s : g.seqs) { h += "@SQ\tSN:" + s.name; snprintf(buf, sizeof buf, "\tLN:%u\n", s.length); h += buf; }
    h += "@PG\tID:YAHA\tVN:0.1.83\tCL:yaha";
    h += " -q " + a.qfileName + " -x " + a.xfileName; h += a.outputBAM ? (a.hardClip ? " -obh " : " -obs ") : a.hardClip ? " -osh " : " -oss "; h += a.ofileName;
    if (a.bamSort) h += " -obsort";
    snprintf(buf, sizeof buf, " -t %d -BW %d -G %d -H %d -M %d -MD %d -P %4.2f -X %d", a.numThreads, a.bandWidth, a.maxGap, a.maxHits, a.minMatch, a.maxDesert, a.minIdentity,
        a.XCutoff); h += buf;
    if (a.affineGapScoring) { snprintf(buf, sizeof buf, " -AGS Y -GEC %d -GOC %d -MS %d -RC %d", a.GECost, a.GOCost, a.MScore, a.RCost); h += buf; } else h += " -AGS N";
    if (a.OQC) {
        snprintf(buf, sizeof buf, " -OQC Y -BP %d -MGDP %d -MNO %d", a.BPCost, a.maxBPLog, a.OQCMinNonOverlap); h += buf;
        if (a.FBS) { snprintf(buf, sizeof buf, " -FBS Y -PRL %4.2f -PSS %4.2f", a.FBS_PSLength, a.FBS_PSScore); h += buf; } else h += " -FBS N";
    } else h += " -OQC N";
    if (a.haveCov) { snprintf(buf, sizeof buf, " -covbin %d -covq %d", a.covBin, a.covMinQ); h += " -ocov " + a.covFileName + buf; }
    if (a.haveEv) { snprintf(buf, sizeof buf, " -evbin %d -evq %d -evclip %d", a.evBin, a.evMinQ, a.evMinClip); h += " -oev " + a.evFileName + buf; }
    if (a.haveBp) { snprintf(buf, sizeof buf, " -bpq %d -bpw %d", a.bpMinQ, a.bpWindow); h += " -obp " + a.bpFileName + buf; }
    if (a.havePu) { snprintf(buf, sizeof buf, " -pumin %d -puq %d", a.puMinAlt, a.puMinQ); h += " -opu " + a.puFileName + buf; }
    if (a.haveId) { snprintf(buf, sizeof buf, " -idmin %d -idlen %d -idq %d", a.idMin, a.idLen, a.idMinQ); h += " -oid " + a.idFileName + buf; }
    if (a.haveEp) { snprintf(buf, sizeof buf, " -epq %d", a.epMinQ); h += " -oep " + a.epFileName + buf; }
    if (a.haveSnv) { snprintf(buf, sizeof buf, " -snverr %d -snvmin %d -snvdp %d -snvqual %d", a.snvErr, a.snvMin, a.snvDp, a.snvQual); h += " -osnv " + a.snvFileName + buf; }
    if (a.haveIndel) { snprintf(buf, sizeof buf, " -inderr %d -indmin %d -inddp %d -indqual %d -indshift %d", a.indErr, a.indMin, a.indDp, a.indQual, a.indShift);
        h += " -oindel " + a.indFileName + buf; }
    h += "\n";
    return h;
}
}  // namespace yaha
