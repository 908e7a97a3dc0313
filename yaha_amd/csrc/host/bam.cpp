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

extern "C" {
__attribute__((weak)) int ygpu_bgzf_open(int device, uint64_t max_in_bytes, ygpu_bgzf **h);
__attribute__((weak)) uint64_t ygpu_bgzf_bound(uint64_t n_in);
__attribute__((weak)) int ygpu_bgzf_compress(ygpu_bgzf *h, const void *in, uint64_t n_in, void *out, uint64_t out_cap, uint64_t *n_out);
__attribute__((weak)) const char *ygpu_bgzf_last_error(ygpu_bgzf *h);
__attribute__((weak)) int ygpu_bgzf_close(ygpu_bgzf *h);
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

bool bamRecord(const Args &a, const Genome &g, const Read &r, const OutClump &oc, int primaryCount, Text &out)
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
    w = put16(w, reg2bin(seqStart, std::max(seqStart, seqEnd) + 1u));
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

void bgzfEof(Text &out) { ybgzf::putEof((uint8_t *)out.room(ybgzf::EOF_BYTES)); out.len += ybgzf::EOF_BYTES; }
}  // namespace yaha
