// bam.cpp -- BAM output (-obh / -obs): the header, the record writer and the compression of a batch's records into BGZF blocks.
//
// A record is printClump's record (sam.cpp, reference AlignOutput.c:115-321) in BAM's binary layout: every decision is taken in the same order from the same
// fields, so that the text a BAM reader makes of it is the line the SAM writer would have written -- but for the two things BAM cannot carry: the case of the
// read's letters (SEQ is four bits a base, =ACMGRSVTWYHKDBN) and a read name of more than 254 characters (cut off there).  Like printClump it writes straight
// into the batch's buffer (yaha::Text) after one bound on its size.
//
// The bytes of a batch are compressed on the device (device/bgzf.hip: a workgroup per block of 65 280 bytes, one handle per formatter thread) by the thread
// that formatted them.  The entry points are WEAK references here, as the tracks' are: the host stages are also linked against test doubles that do not have
// them (the CPU tier), and then -- as when a handle cannot be opened, or with YAHA_HOST_BGZF=1 -- the host's encoder (../bgzf_core.h, the source the device
// compiles as well) does the work.  A compression that FAILS on the device is an error of the run, not a reason to fall back.
#include "yaha_host.h"
#include "../bgzf_core.h"
#include "../bai_core.h"
#include <chrono>

extern "C" {
__attribute__((weak)) int ygpu_bgzf_open(int device, uint64_t max_in_bytes, ygpu_bgzf **h);
__attribute__((weak)) uint64_t ygpu_bgzf_bound(uint64_t n_in);
__attribute__((weak)) int ygpu_bgzf_compress(ygpu_bgzf *h, const void *in, uint64_t n_in, void *out, uint64_t out_cap, uint64_t *n_out);
__attribute__((weak)) const char *ygpu_bgzf_last_error(ygpu_bgzf *h);
__attribute__((weak)) int ygpu_bgzf_close(ygpu_bgzf *h);
__attribute__((weak)) int ygpu_bamsort_open(int device, uint64_t max_store_bytes, uint64_t segment_bytes, uint64_t window_bytes, ygpu_bamsort **h);
__attribute__((weak)) int ygpu_bamsort_append(ygpu_bamsort *h, const void *bytes, uint64_t n_bytes, const uint64_t *keys, const uint32_t *lens, uint32_t n_records);
__attribute__((weak)) int ygpu_bamsort_sort(ygpu_bamsort *h, uint32_t *perm);
__attribute__((weak)) int ygpu_bamsort_next(ygpu_bamsort *h, void *out, uint64_t out_cap, uint64_t *n_out, uint64_t *n_raw);
__attribute__((weak)) uint64_t ygpu_bamsort_info(ygpu_bamsort *h, int what);
__attribute__((weak)) const char *ygpu_bamsort_last_error(ygpu_bamsort *h);
__attribute__((weak)) int ygpu_bamsort_close(ygpu_bamsort *h);
}

namespace yaha {
namespace {
inline uint8_t *put8(uint8_t *w, uint32_t v) { *w++ = (uint8_t)v; return w; }
inline uint8_t *put16(uint8_t *w, uint32_t v) { ybgzf::put16(w, v); return w + 2; }
inline uint8_t *put32(uint8_t *w, uint32_t v) { ybgzf::put32(w, v); return w + 4; }
inline uint8_t *putU(uint8_t *w, uint32_t v)                             // decimal, no sign (the MD text)
{
    char t[12]; int n = 0;
    do { t[n++] = (char)('0' + v % 10); v /= 10; } while (v);
    while (n) *w++ = (uint8_t)t[--n];
    return w;
}
// an integer tag of the smallest unsigned type that holds the value
inline uint8_t *putTagU(uint8_t *w, const char *tag, uint32_t v)
{
    *w++ = (uint8_t)tag[0]; *w++ = (uint8_t)tag[1];
    if (v < 256u) { *w++ = 'C'; return put8(w, v); }
    if (v < 65536u) { *w++ = 'S'; return put16(w, v); }
    *w++ = 'I'; return put32(w, v);
}
inline uint32_t reg2bin(uint32_t beg, uint32_t end)                       // the SAM specification's, end exclusive
{
    --end;
    if (beg >> 14 == end >> 14) return ((1u << 15) - 1u) / 7u + (beg >> 14);
    if (beg >> 17 == end >> 17) return ((1u << 12) - 1u) / 7u + (beg >> 17);
    if (beg >> 20 == end >> 20) return ((1u << 9) - 1u) / 7u + (beg >> 20);
    if (beg >> 23 == end >> 23) return ((1u << 6) - 1u) / 7u + (beg >> 23);
    if (beg >> 26 == end >> 26) return ((1u << 3) - 1u) / 7u + (beg >> 26);
    return 0;
}
// a letter of the read as BAM's four bits: upper-cased, anything outside the table is N
inline uint32_t seqCode(char c)
{
    static const char table[] = "=ACMGRSVTWYHKDBN";
    if (c >= 'a' && c <= 'z') c = (char)(c - 'a' + 'A');
    for (uint32_t k = 0; k < 16; k++) if (table[k] == c) return k;
    return 15;
}
enum { CIG_M = 0, CIG_I = 1, CIG_D = 2, CIG_S = 4, CIG_H = 5 };
inline uint32_t cigarOp(char code) { return code == 'I' ? CIG_I : code == 'D' ? CIG_D : code == 'S' ? CIG_S : code == 'H' ? CIG_H : CIG_M; }
}  // namespace

std::string bamHeader(const Args &a, const Genome &g)
{
    const std::string text = samHeader(a, g);
    std::string h = "BAM\1"; uint8_t w[4];
    auto add32 = [&](uint32_t v) { ybgzf::put32(w, v); h.append((const char *)w, 4); };
    add32((uint32_t)text.size()); h += text;
    add32((uint32_t)g.seqs.size());
    for (auto &s : g.seqs) { add32((uint32_t)s.name.size() + 1u); h += s.name; h += '\0'; add32(s.length); }
    return h;
}

bool bamRecord(const Args &a, const Genome &g, const Read &r, const OutClump &oc, int primaryCount, Text &out, BamEntry *entry)
{
    const ygpu_clump &c = oc.c;
    uint32_t seqStart = c.sro, seqEnd = c.sro + c.refLen - 1;
    int si = g.findSeq(seqStart);
    if (si < 0 || seqEnd >= g.seqs[si].start + g.seqs[si].length) return false;      // spans two sequences: silently dropped, as printClump does
    const BaseSeq &bs = g.seqs[si];
    seqStart -= bs.start; seqEnd -= bs.start;
    const bool reversed = (oc.status & 0x01) != 0;
    const std::string &queryBuf = reversed ? r.rev : r.fwd;
    const int qlen = r.len();
    const size_t idLen = std::min<size_t>(r.id.size(), 254);                         // l_read_name is one byte and counts the NUL
    // bound: the fixed fields and tags < 160; CIGAR 4 bytes per op + two clips; SEQ and QUAL 1.5 bytes a base; MD <= 13 per op + one character per reference base
    uint8_t *const w0 = (uint8_t *)out.room(idLen + 2 * (size_t)qlen + 32 * (size_t)c.n_ops + (size_t)c.refLen + 256);
    uint8_t *w = w0 + 4;                                                              // (block_size: when the record's end is known)
    const char clipCode = a.hardClip ? 'H' : 'S';
    const int clipBack = qlen - 1 - c.eqo, clipFront = c.sqo;
    int qstart = 0, qend = qlen - 1;
    if (a.hardClip) { qstart = c.sqo; qend = c.eqo; }
    const uint32_t lseq = qend >= qstart ? (uint32_t)(qend - qstart + 1) : 0u;
    w = put32(w, (uint32_t)si); w = put32(w, seqStart); w = put8(w, (uint32_t)idLen + 1u); w = put8(w, oc.mapQuality);
    const uint32_t endExcl = std::max(seqStart, seqEnd) + 1u, bin = reg2bin(seqStart, endExcl);
    w = put16(w, bin);
    uint8_t *const nCigarAt = w; w += 2;
    w = put16(w, reversed ? 0x10 : 0); w = put32(w, lseq); w = put32(w, 0xFFFFFFFFu); w = put32(w, 0xFFFFFFFFu); w = put32(w, 0);
    memcpy(w, r.id.data(), idLen); w += idLen; *w++ = 0;
    // CIGAR (M and R merge into M), the SAM writer's walk
    uint8_t *const cigar0 = w; int matches = 0;
    auto cig = [&](int len, char code) { w = put32(w, (uint32_t)len << 4 | cigarOp(code)); };
    if (clipFront > 0) cig(clipFront, clipCode);
    for (uint32_t k = 0; k < c.n_ops; k++) {
        const char code = YGPU_OP_CODE(oc.ops[k]); const int len = (int)YGPU_OP_LEN(oc.ops[k]);
        if (code == 'M' || code == 'R') { matches += len; continue; }
        if (matches > 0) { cig(matches, 'M'); matches = 0; }
        cig(len, code);
    }
    if (clipBack > 0) { if (matches > 0) { cig(matches, 'M'); matches = 0; } cig(clipBack, clipCode); }
    if (matches > 0) cig(matches, 'M');
    ybgzf::put16(nCigarAt, (uint32_t)((w - cigar0) / 4));
    // SEQ, two bases a byte, the first in the high half
    for (uint32_t i = 0; i < lseq; i += 2) {
        const uint32_t hi = seqCode(queryBuf[(size_t)qstart + i]), lo = i + 1 < lseq ? seqCode(queryBuf[(size_t)qstart + i + 1]) : 0u;
        *w++ = (uint8_t)(hi << 4 | lo);
    }
    // QUAL: the SAM writer's order (sic, sam.cpp), less 33; 0xFF without qualities
    if (a.fastq) { if (reversed) for (int i = qend; i >= qstart; i--) *w++ = (uint8_t)(r.qual[i] - 33);
        else for (int i = qstart; i <= qend; i++) *w++ = (uint8_t)(r.qual[i] - 33); }
    else { memset(w, 0xFF, lseq); w += lseq; }
    w = putTagU(w, "AS", c.totScore); w = putTagU(w, "NM", (uint32_t)c.gapBases + c.mismatchedBases);
    *w++ = 'M'; *w++ = 'D'; *w++ = 'Z';
    // MD, the SAM writer's walk (the clip ops sit in the list as well: they only reset `previous`)
    matches = 0; char previous = clipFront > 0 ? clipCode : 'U'; uint32_t cur = c.sro;
    for (uint32_t k = 0; k < c.n_ops; k++) {
        const char code = YGPU_OP_CODE(oc.ops[k]); const int len = (int)YGPU_OP_LEN(oc.ops[k]);
        if (code == 'M') { matches += len; cur += len; }
        else if (code == 'R') {
            if (matches > 0) { w = putU(w, (uint32_t)matches); matches = 0; }
            if (previous == 'D') *w++ = '0';
            for (int i = 0; i < len; i++) *w++ = (uint8_t)kFourBitChars[get4(g.bases, cur + i)];
            cur += len;
        } else if (code == 'D') {
            if (matches > 0) { w = putU(w, (uint32_t)matches); matches = 0; }
            *w++ = '^';
            for (int i = 0; i < len; i++) *w++ = (uint8_t)kFourBitChars[get4(g.bases, cur + i)];
            cur += len;
        }
        previous = code;
    }
    if (matches > 0) w = putU(w, (uint32_t)matches);
    *w++ = 0;
    static const char H[] = "0123456789ABCDEF";
    *w++ = 'Y'; *w++ = 'F'; *w++ = 'H'; *w++ = (uint8_t)H[(oc.status >> 4) & 15]; *w++ = (uint8_t)H[oc.status & 15]; *w++ = 0;
    if (a.OQC) {
        w = putTagU(w, "YI", oc.matchedPrimary); w = putTagU(w, "YP", (uint32_t)primaryCount);
        if (oc.status & 0x20) w = putTagU(w, "YS", oc.numSecondaries);
    }
    ybgzf::put32(w0, (uint32_t)(w - w0) - 4u);
    out.len += (size_t)(w - w0);
    if (entry) *entry = BamEntry{(uint32_t)si, seqStart, (uint32_t)(w - w0), endExcl, bin};
    return true;
}

// ---- compression ----------------------------------------------------------------------------------------------------------------------------------------------------
struct BgzfPacker::Impl { ygpu_bgzf *h = nullptr; uint64_t cap = 0; int dev = -1; bool hostOnly = false; ybgzf::HostWork work; };

bool BgzfPacker::deviceEntryPoints()
{ return ygpu_bgzf_open != nullptr && ygpu_bgzf_bound != nullptr && ygpu_bgzf_compress != nullptr && ygpu_bgzf_last_error != nullptr && ygpu_bgzf_close != nullptr; }
BgzfPacker::BgzfPacker() : impl(new Impl) { impl->hostOnly = !deviceEntryPoints() || getenv("YAHA_HOST_BGZF") != nullptr; }
BgzfPacker::~BgzfPacker() { if (impl->h && getenv("YAHA_FAST_EXIT") == nullptr) ygpu_bgzf_close(impl->h); delete impl; }

void BgzfPacker::packHost(const char *in, size_t n, Text &out, BamStats &st)
{
    out.clear();
    uint64_t blocks = 0, stored = 0;
    out.len = (size_t)ybgzf::encodeStream((const uint8_t *)in, n, (uint8_t *)out.room((size_t)ybgzf::bound(n)), impl->work, &blocks, &stored);
    st.blocks += blocks; st.blocksStored += stored; st.bytesRaw += n; st.bytesWritten += out.len;
}

int BgzfPacker::pack(int device, const char *in, size_t n, Text &out, BamStats &st, std::string &err)
{
    if (n == 0) { out.clear(); return 0; }
    Impl &I = *impl;
    // the handle: opened when first needed, on the device the batch ran on, sized to the largest batch seen (a quarter more); a handle that cannot be opened
    // leaves this thread's batches to the host's encoder
    if (!I.hostOnly && (!I.h || n > I.cap || device != I.dev)) {
        if (I.h) { ygpu_bgzf_close(I.h); I.h = nullptr; }
        I.cap = std::max<uint64_t>(I.dev == device ? I.cap : 0, (uint64_t)n + n / 4); I.dev = device;
        if (ygpu_bgzf_open(device, I.cap, &I.h) != 0) {
            fprintf(stderr, "-ob: no BGZF handle on device %d (%s): this thread compresses on the host.\n", device, I.h ? ygpu_bgzf_last_error(I.h) : "no handle was made");
            if (I.h) { ygpu_bgzf_close(I.h); I.h = nullptr; }
            I.hostOnly = true;
        }
    }
    if (I.hostOnly) { packHost(in, n, out, st); st.hostBatches++; return 0; }
    out.clear();
    const uint64_t room = ygpu_bgzf_bound(n); uint64_t got = 0;
    const int rc = ygpu_bgzf_compress(I.h, in, n, out.room((size_t)room), room, &got);
    if (rc != 0) { err = ygpu_bgzf_last_error(I.h); return rc; }
    out.len = (size_t)got;
    // the blocks, counted from their headers (BSIZE; the stored form: BTYPE 00 in the first byte of the deflate data)
    uint64_t blocks = 0, stored = 0;
    for (size_t at = 0; at + ybgzf::HEADER < out.len;) {
        const uint8_t *b = (const uint8_t *)out.p + at;
        blocks++; if ((b[ybgzf::HEADER] & 6u) == 0) stored++;
        at += (size_t)(b[16] | b[17] << 8) + 1u;
    }
    st.blocks += blocks; st.blocksStored += stored; st.bytesRaw += n; st.bytesWritten += out.len; st.deviceBatches++;
    return 0;
}

// ---- -obsort ------------------------------------------------------------------------------------------------------------------------------------------------------
struct BamSorter::Impl {
    int device = 0; uint64_t cap = 0; ygpu_bamsort *h = nullptr; bool host = false;
    std::vector<BamEntry> entries;                                                    // every record of the run, in append (= print) order: 20 bytes a record
    Text store; std::vector<uint64_t> at;                                             // host store: the records' bytes and where each starts
    std::vector<uint64_t> keys; std::vector<uint32_t> lens;                           // (a batch's, reused)
};

static double msNow() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

BamSorter::BamSorter(int device, uint64_t capBytes) : impl(new Impl)
{
    Impl &I = *impl; I.device = device; I.cap = capBytes;
    const bool have = ygpu_bamsort_open != nullptr && ygpu_bamsort_append != nullptr && ygpu_bamsort_sort != nullptr && ygpu_bamsort_next != nullptr &&
        ygpu_bamsort_info != nullptr && ygpu_bamsort_last_error != nullptr && ygpu_bamsort_close != nullptr && ygpu_bgzf_bound != nullptr;
    I.host = !have || getenv("YAHA_HOST_BAMSORT") != nullptr;
    if (!I.host && ygpu_bamsort_open(device, capBytes, 0, 0, &I.h) != 0) {
        fprintf(stderr, "-obsort: no record store on device %d (%s): the records are kept and ordered on the host.\n", device, I.h ? ygpu_bamsort_last_error(I.h)
            : "no handle was made");
        if (I.h) { ygpu_bamsort_close(I.h); I.h = nullptr; }
        I.host = true;
    }
    stats.device = !I.host;
}
BamSorter::~BamSorter() { if (impl->h && getenv("YAHA_FAST_EXIT") == nullptr) ygpu_bamsort_close(impl->h); delete impl; }

int BamSorter::append(const char *bytes, size_t n, const BamEntry *e, size_t nEntries, std::string &err)
{
    Impl &I = *impl; const double t0 = msNow();
    if (nEntries == 0) return 0;
    if (I.entries.size() + nEntries > 0xFFFFFFFFull) { err = "-obsort: more than 2^32 - 1 records"; return YGPU_EINVAL; }
    if (I.host) {
        if ((uint64_t)I.store.len + n + 20ull * (I.entries.size() + nEntries) > I.cap) {
            err = "-obsort: the record store would pass -sortmem (" + std::to_string(I.cap) + " bytes) -- there is no spill: give a larger -sortmem or sort the unsorted output";
            return YGPU_ENOMEM; }
        uint64_t p = I.store.len;
        try { I.store.append(bytes, n); for (size_t i = 0; i < nEntries; i++) { I.at.push_back(p); p += e[i].len; } }
        catch (const std::bad_alloc &) { err = "-obsort: the host cannot give the memory for the record store (-sortmem " + std::to_string(I.cap) + " bytes)"; return YGPU_ENOMEM; }
    } else {
        I.keys.resize(nEntries); I.lens.resize(nEntries);
        for (size_t i = 0; i < nEntries; i++) { I.keys[i] = ybai::sortKey(e[i].ref, e[i].pos); I.lens[i] = e[i].len; }
        const int rc = ygpu_bamsort_append(I.h, bytes, n, I.keys.data(), I.lens.data(), (uint32_t)nEntries);
        if (rc != 0) { err = std::string("-obsort: the record store on device ") + std::to_string(I.device) + " (-sortmem " + std::to_string(I.cap) + " bytes): " +
            ygpu_bamsort_last_error(I.h); return rc; }
    }
    I.entries.insert(I.entries.end(), e, e + nEntries);
    stats.records = I.entries.size(); msAppend += msNow() - t0;
    return 0;
}

int BamSorter::finish(FILE *out, const std::string &baiPath, const std::string &rawHeader, size_t nRefs, BamStats &st, std::string &err)
{
    Impl &I = *impl; const bool timing = getenv("YAHA_TIMING") != nullptr; const double t0 = msNow();
    const size_t n = I.entries.size();
    // the order: perm[j] = the record at sorted place j
    std::vector<uint32_t> perm(n);
    if (I.host) {
        bamSortOrder(I.entries.data(), n, perm.data());
    } else {
        const int rc = ygpu_bamsort_sort(I.h, perm.data());
        if (rc != 0) { err = std::string("-obsort: the sort on device ") + std::to_string(I.device) + " failed: " + ygpu_bamsort_last_error(I.h); return rc; }
        stats.passes = ygpu_bamsort_info(I.h, YGPU_BAMSORT_PASSES); stats.segments = ygpu_bamsort_info(I.h, YGPU_BAMSORT_SEGMENTS);
    }
    std::vector<BamEntry> sorted(n);
    for (size_t j = 0; j < n; j++) { if (perm[j] >= n) { err = "-obsort: the permutation is out of range"; return YGPU_EINTERNAL; } sorted[j] = I.entries[perm[j]]; }
    for (size_t j = 1; j < n; j++) if (ybai::sortKey(sorted[j - 1].ref, sorted[j - 1].pos) > ybai::sortKey(sorted[j].ref, sorted[j].pos) ||
        (ybai::sortKey(sorted[j - 1].ref, sorted[j - 1].pos) == ybai::sortKey(sorted[j].ref, sorted[j].pos) && perm[j - 1] > perm[j])) {
        err = "-obsort: the records are not in stable coordinate order at place " + std::to_string(j); return YGPU_EINTERNAL; }
    const double t1 = msNow();
    if (timing) fprintf(stderr, "[yaha] -obsort: %zu records appended in %.1f ms (all batches), ordered %s in %.1f ms\n", n, msAppend, I.host ? "on the host" : "on the device",
        t1 - t0);
    // the header's blocks, from the host's encoder
    auto put = [&](const char *p, size_t len) { if (len && fwrite(p, 1, len, out) != len) { err = "Failure writing the output file."; return false; } return true; };
    Text packed; uint64_t fileAt = 0;
    { BgzfPacker hostPacker; hostPacker.packHost(rawHeader.data(), rawHeader.size(), packed, st); if (!put(packed.p, packed.len)) return YGPU_EINTERNAL; fileAt = packed.len; }
    // the sorted stream's blocks, window by window; the file offset of every block
    uint64_t total = 0; for (size_t j = 0; j < n; j++) total += sorted[j].len;
    std::vector<uint64_t> coffs((size_t)ybgzf::blocksOf(total) + 1); size_t nBlocks = 0;
    auto account = [&](const Text &blk) {
        const uint64_t end = ybai::blockOffsets((const uint8_t *)blk.p, blk.len, fileAt, coffs.data(), &nBlocks, coffs.size() - 1);
        if (end == 0) { err = "-obsort: a window's blocks do not add up"; return false; }
        fileAt = end; stats.windows++; return true; };
    if (I.host) {
        const uint64_t W = 1024ull * ybgzf::PAYLOAD_MAX; BgzfPacker packer; Text win; size_t j = 0; uint64_t inRec = 0;
        for (uint64_t w0 = 0; w0 < total; w0 += W) {
            const double tw = msNow(); const uint64_t wn = std::min<uint64_t>(W, total - w0); win.clear(); win.room((size_t)wn);
            while (win.len < wn) {                                                    // the records of the window, the first and the last possibly in part
                const BamEntry &e = sorted[j]; const uint64_t take = std::min<uint64_t>(e.len - inRec, wn - win.len);
                win.append(I.store.p + I.at[perm[j]] + inRec, (size_t)take); inRec += take;
                if (inRec == e.len) { j++; inRec = 0; }
            }
            std::string perr; const int rc = packer.pack(I.device, win.p, win.len, packed, st, perr);
            if (rc != 0) { err = "BGZF compression on device " + std::to_string(I.device) + " failed: " + perr; return rc; }
            if (!account(packed) || !put(packed.p, packed.len)) return YGPU_EINTERNAL;
            if (timing) fprintf(stderr, "[yaha] -obsort: window %llu: %llu bytes to %zu in %.1f ms (host store)\n", (unsigned long long)(w0 / W), (unsigned long long)wn,
                packed.len,
                msNow() - tw);
        }
    } else {
        const uint64_t room = ygpu_bgzf_bound(ygpu_bamsort_info(I.h, YGPU_BAMSORT_WINDOW_BYTES));
        for (uint64_t w = 0;; w++) {
            const double tw = msNow(); uint64_t got = 0, nRaw = 0; packed.clear();
            const int rc = ygpu_bamsort_next(I.h, packed.room((size_t)room), room, &got, &nRaw);
            if (rc != 0) { err = std::string("-obsort: window ") + std::to_string(w) + " on device " + std::to_string(I.device) + " failed: " + ygpu_bamsort_last_error(I.h);
                return rc; }
            if (got == 0) break;
            packed.len = (size_t)got;
            const size_t before = nBlocks;
            if (!account(packed) || !put(packed.p, packed.len)) return YGPU_EINTERNAL;
            uint64_t stored = 0;
            for (size_t b = before; b < nBlocks; b++) if ((((const uint8_t *)packed.p)[coffs[b] - coffs[before] + ybgzf::HEADER] & 6u) == 0) stored++;
            st.blocks += nBlocks - before; st.blocksStored += stored; st.bytesRaw += nRaw; st.bytesWritten += got; st.deviceBatches++;
            if (timing) fprintf(stderr, "[yaha] -obsort: window %llu: %llu bytes to %llu in %.1f ms (gather, deflate, download)\n", (unsigned long long)w, (unsigned long long)nRaw,
                (unsigned long long)got, msNow() - tw);
        }
    }
    if (nBlocks != ybgzf::blocksOf(total)) { err = "-obsort: " + std::to_string(nBlocks) + " blocks were written, the stream has " + std::to_string(ybgzf::blocksOf(total));
        return YGPU_EINTERNAL; }
    coffs[nBlocks] = fileAt;
    Text eof; bgzfEof(eof); st.bytesWritten += eof.len; if (!put(eof.p, eof.len)) return YGPU_EINTERNAL;
    if (fflush(out) != 0) { err = "Failure writing the output file."; return YGPU_EINTERNAL; }
    const double t2 = msNow();
    const std::string bai = baiBuild(sorted.data(), n, nRefs, coffs.data(), nBlocks);
    std::string werr; if (!writeFile(baiPath.c_str(), bai.data(), bai.size(), werr)) { err = werr; return YGPU_EINTERNAL; }
    stats.baiBytes = bai.size();
    if (timing) fprintf(stderr, "[yaha] -obsort: %llu windows written in %.1f ms, the index (%zu bytes) in %.1f ms\n", (unsigned long long)stats.windows, t2 - t1, bai.size(),
        msNow() - t2);
    return 0;
}

void bgzfEof(Text &out) { ybgzf::putEof((uint8_t *)out.room(ybgzf::EOF_BYTES)); out.len += ybgzf::EOF_BYTES; }

// ---- the main output as BAM (RecordSink, yaha_host.h) ---------------------------------------------------------------------------------------------------------
namespace {
// -obh / -obs: the header is BGZF blocks of its own from the host's encoder; every batch's records are compressed by the thread that formats them, with a packer
// of its own, and the end-of-file block follows the last batch of a run that got there
struct BamSink : RecordSink {
    BamStats bam; std::vector<std::unique_ptr<BgzfPacker>> packers;
    bool begin(const Args &a, const Genome &g, const std::string &, int nFormatters, FILE *log) override
    {
        for (int i = 0; i < nFormatters; i++) packers.emplace_back(new BgzfPacker);
        const std::string raw = bamHeader(a, g); Text packed; BgzfPacker hostPacker; hostPacker.packHost(raw.data(), raw.size(), packed, bam);
        if (fwrite(packed.p, 1, packed.len, out) != packed.len) { fprintf(log, "Failure writing the output file.\n"); return false; }
        return true;
    }
    bool pack(SinkBatch &b, int formatter, bool stopped, std::string &err) override
    {
        std::string perr; b.packed.clear();                                // (a batch without records is no block: an empty one would read as the end of the file)
        const int rc = stopped ? 0 : packers[formatter]->pack(b.dev, b.text.p, b.text.len, b.packed, bam, perr);
        bam.records += b.records;
        if (rc != 0) { char m[640]; snprintf(m, sizeof m, "BGZF compression on device %d failed (%d): %s", b.dev, rc, perr.c_str()); err = m; }
        return rc == 0;
    }
    bool write(SinkBatch &b, std::string &err) override { return writeBytes(b.packed, err); }
    void timingLine(const SinkBatch &b, uint64_t ticket) const override
    {
        fprintf(stderr, "[yaha] ticket %llu: %zu bytes of records compressed to %zu in %.1f ms (wait for the blocks included)\n", (unsigned long long)ticket, b.text.len,
            b.packed.len,
            b.tPack);
    }
    bool finish(FILE *log) override
    {
        Text eof; bgzfEof(eof); bam.bytesWritten += eof.len;
        if (fwrite(eof.p, 1, eof.len, out) != eof.len) { fprintf(log, "Failure writing the output file.\n"); return false; }
        return true;
    }
    void stats(std::string &line) const override
    {
        char t[512]; snprintf(t, sizeof t, ", \"bam_records\": %llu, \"bam_bytes_raw\": %llu, \"bam_bytes_written\": %llu, \"bam_blocks\": %llu, "
            "\"bam_blocks_stored\": %llu, \"bam_device_batches\": %llu, \"bam_host_batches\": %llu", (unsigned long long)bam.records.load(),
            (unsigned long long)bam.bytesRaw.load(), (unsigned long long)bam.bytesWritten.load(), (unsigned long long)bam.blocks.load(),
            (unsigned long long)bam.blocksStored.load(), (unsigned long long)bam.deviceBatches.load(), (unsigned long long)bam.hostBatches.load());
        line += t;
    }
};
// -obsort: nothing is written before the last alignment -- the raw records travel to the writer thread and into the sorter (a store on device -device, or the
// host's), appended in ticket order, which is what makes equal keys keep print order; the sorter writes the header's blocks, the sorted stream's and FILE.bai at
// the end.  A failed run leaves neither file behind.
struct SortedBamSink : BamSink {
    std::unique_ptr<BamSorter> sorter; const Args *args = nullptr; const Genome *genome = nullptr;
    bool begin(const Args &a, const Genome &g, const std::string &, int, FILE *log) override
    {
        args = &a; genome = &g;
        for (auto &sq : g.seqs) if (sq.length > (1u << 29)) {
            fprintf(log, "-obsort: sequence %s has %u bases; BAI indexes sequences of up to 2^29 = 536870912 bases.\n", sq.name.c_str(), sq.length); abandon(); return false; }
        uint64_t capBytes = (uint64_t)a.sortMemGB << 30;
        if (const char *e = getenv("YAHA_SORTMEM_BYTES")) { const long long v = atoll(e); if (v > 0) capBytes = (uint64_t)v; }      // (byte-granular, for tests)
        sorter.reset(new BamSorter(a.device, capBytes)); return true;
    }
    std::vector<BamEntry> *entries(SinkBatch &b) const override { return &b.entries; }
    bool pack(SinkBatch &b, int, bool, std::string &) override { bam.records += b.records; return true; }
    bool write(SinkBatch &b, std::string &err) override { return sorter->append(b.text.p, b.text.len, b.entries.data(), b.entries.size(), err) == 0; }
    void timingLine(const SinkBatch &b, uint64_t ticket) const override
    {
        fprintf(stderr, "[yaha] ticket %llu: %zu records (%zu bytes) appended to the sorter, %.1f ms so far\n", (unsigned long long)ticket, b.entries.size(), b.text.len,
            sorter->msAppend);
    }
    bool finish(FILE *log) override
    {
        std::string serr;
        if (sorter->finish(out, path + ".bai", bamHeader(*args, *genome), genome->seqs.size(), bam, serr) != 0) { fprintf(log, "%s\n", serr.c_str()); return false; }
        return true;
    }
    void abandon() override { if (out != stdout) { fclose(out); out = nullptr; } remove(path.c_str()); remove((path + ".bai").c_str()); }
    void stats(std::string &line) const override
    {
        BamSink::stats(line); const BamSortStats &bs = sorter->stats;
        char t[384]; snprintf(t, sizeof t, ", \"bam_sorted_records\": %llu, \"bam_sort_device\": %d, \"bam_sort_segments\": %llu, \"bam_sort_windows\": %llu, "
            "\"bam_sort_passes\": %llu, \"bai_bytes\": %llu", (unsigned long long)bs.records, bs.device ? 1 : 0, (unsigned long long)bs.segments,
            (unsigned long long)bs.windows, (unsigned long long)bs.passes, (unsigned long long)bs.baiBytes);
        line += t;
    }
};
}  // namespace

std::unique_ptr<RecordSink> makeRecordSink(const Args &a)
{
    return std::unique_ptr<RecordSink>(a.bamSort ? new SortedBamSink : a.outputBAM ? new BamSink : new RecordSink);
}
}  // namespace yaha
