// session.cpp -- the host side of the C-ABI (include/yaha_hip.h, second half): a session is a parsed command line with its genome, index and input open;
// yaha_session_next_batch reads, yaha_session_emit[_filtered] formats what the caller's ygpu_* calls computed (pipeline.cpp's formatting, one batch at a
// time), and the yaha_session_*_params fill the parameter blocks of the device stages from the session's options.  The command line's run loads one as well.
#include "yaha_host.h"

using namespace yaha;

bool yaha_session::load()
{
    Args &a = args;
    if (!loadNib2(a.gfileName.c_str(), genome, err)) return false;
    seqs.set(genome);
    if (!loadIndex(a.xfileName.c_str(), index, err)) return false;
    a.wordLen = index.wordLen;                                               // Query.c:603-610
    if (index.maxHits < a.maxHits) {
        fprintf(stderr, "WARNING: Index file made with maxHits of %d, while %d specified for this query run.\nMimimum of two (%d) will be used.\n", index.maxHits, a.maxHits,
            index.maxHits);
        a.maxHits = index.maxHits;
    }
    reader.maxQueryLength = a.maxQueryLength; reader.wordLen = a.wordLen;
    if (!reader.open(a.qfileName.c_str(), err)) return false;
    readerOpen = true; a.fastq = reader.fastq;
    header = samHeader(a, genome);
    return true;
}

// the part every yaha_session_*_params shares: the arguments checked, the sequence table in
template <class P> static int sessionParams(yaha_session *s, P *p) { if (!s || !p) return YGPU_EINVAL; s->seqs.into(*p); return 0; }

extern "C" {
int yaha_session_open(int argc, const char *const *argv, yaha_session **out)
{
    *out = nullptr; yaha_session *s = new yaha_session;
    std::vector<char *> av; av.push_back((char *)"yaha"); for (int i = 0; i < argc; i++) av.push_back((char *)argv[i]);
    int rc = parseArgs((int)av.size(), av.data(), s->args);
    if (rc != 0 || !s->args.query) { delete s; return YGPU_EINVAL; }
    *out = s;
    if (!s->load()) return YGPU_EINVAL;
    return 0;
}
void yaha_session_close(yaha_session *s) { if (!s) return; if (s->readerOpen) s->reader.close(); delete s; }
const char *yaha_session_error(const yaha_session *s) { return s ? s->err.c_str() : "null session"; }
int yaha_session_params(const yaha_session *s, ygpu_params *p) { paramsFromArgs(s->args, *p); return 0; }
int yaha_session_index_view(const yaha_session *s, ygpu_index_view *v)
{
    v->bases = s->genome.bases; v->n_base_bytes = s->genome.nBaseBytes; v->maxROff = s->genome.maxROff;
    v->startingOffs = s->index.SO; v->ROA = s->index.ROA; v->totalMatches = s->index.totalMatches; v->wordLen = s->index.wordLen; return 0;
}
int yaha_session_header(yaha_session *s, const char **text, size_t *len) { *text = s->header.c_str(); *len = s->header.size(); return 0; }
int yaha_session_next_batch(yaha_session *s, uint32_t max_reads, ygpu_read_batch *b)
{
    s->reads.clear(); s->codes.clear(); s->offsets.assign(1, 0);
    Read r;
    while (s->reads.size() < max_reads && s->reader.next(r)) { s->codes.insert(s->codes.end(), r.fwdCodes.begin(), r.fwdCodes.end()); s->offsets.push_back(s->codes.size());
        s->reads.push_back(std::move(r)); r = Read(); }
    b->n_reads = (uint32_t)s->reads.size(); b->codes = s->codes.data(); b->offsets = s->offsets.data(); return 0;
}
int yaha_session_emit(yaha_session *s, const ygpu_result_batch *r, const char **text, size_t *len)
{
    if (r->n_reads != s->reads.size()) { s->err = "result batch does not match the current read batch"; return YGPU_EINVAL; }
    FormatCtx f{s->args, s->genome, s->reads.data()};
    formatBatch(f, r, s->text, std::max(1, s->args.numThreads)); *s->text.room(1) = 0; *text = s->text.p; *len = s->text.len; return 0;
}
int yaha_session_emit_filtered(yaha_session *s, const ygpu_filtered_batch *r, const char **text, size_t *len)
{
    if (r->n_reads != s->reads.size()) { s->err = "result batch does not match the current read batch"; return YGPU_EINVAL; }
    FormatCtx f{s->args, s->genome, s->reads.data()};
    formatFiltered(f, r, s->text); *s->text.room(1) = 0; *text = s->text.p; *len = s->text.len; return 0;
}
int yaha_session_postfilter_params(yaha_session *s, ygpu_postfilter_params *p)
{
    if (postfilterParams(s->args, s->seqs, s->pfThr, p)) return 0;
    s->err = "the device post-filter takes OQC runs with non-negative break point costs and -MNO of at least 1 only"; return YGPU_EINVAL;
}
int yaha_session_depth_params(yaha_session *s, ygpu_depth_params *p)
{
    if (sessionParams(s, p) != 0) return YGPU_EINVAL;
    p->bin = (uint32_t)s->args.covBin; p->min_mapq = (uint32_t)s->args.covMinQ; return 0;
}
int yaha_session_events_params(yaha_session *s, ygpu_events_params *p)
{
    if (sessionParams(s, p) != 0) return YGPU_EINVAL;
    p->bin = (uint32_t)s->args.evBin; p->min_mapq = (uint32_t)s->args.evMinQ; p->min_clip = (uint32_t)s->args.evMinClip; return 0;
}
int yaha_session_pileup_params(yaha_session *s, ygpu_pileup_params *p)
{
    if (sessionParams(s, p) != 0) return YGPU_EINVAL;
    p->min_mapq = (uint32_t)s->args.puMinQ; return 0;
}
int yaha_session_snv_params(yaha_session *s, ygpu_snv_params *p)
{
    if (!s || !p) return YGPU_EINVAL;
    snvParamsFromArgs(s->args, *p); return 0;
}
int yaha_session_indelcall_params(yaha_session *s, ygpu_indelcall_params *p)
{
    if (!s || !p) return YGPU_EINVAL;
    indelcallParamsFromArgs(s->args, *p); return 0;
}
int yaha_session_indel_params(yaha_session *s, ygpu_indel_params *p)
{
    if (!s || !p) return YGPU_EINVAL;
    memset(p, 0, sizeof *p); sessionParams(s, p);
    p->min_mapq = (uint32_t)s->args.idMinQ; p->min_length = (uint32_t)s->args.idLen; return 0;
}
int yaha_session_eprofile_params(yaha_session *s, ygpu_eprofile_params *p)
{
    if (sessionParams(s, p) != 0) return YGPU_EINVAL;
    p->min_mapq = (uint32_t)s->args.epMinQ; return 0;
}
int yaha_session_junction_params(yaha_session *s, ygpu_junction_params *p)
{
    if (sessionParams(s, p) != 0) return YGPU_EINVAL;
    p->min_mapq = (uint32_t)s->args.bpMinQ; return 0;
}
int yaha_build_index(int argc, const char *const *argv)
{
    Args a; std::vector<char *> av; av.push_back((char *)"yaha"); for (int i = 0; i < argc; i++) av.push_back((char *)argv[i]);
    int rc = parseArgs((int)av.size(), av.data(), a); if (rc != 0 || !a.index) return YGPU_EINVAL;
    return runIndex(a, stderr) == 0 ? 0 : YGPU_EINVAL;
}
int yaha_main(int argc, char **argv)
{
    fprintf(stderr, "YAHA (MI355X hot path) compatible with version 0.1.83\n");
    Args a; int rc = parseArgs(argc, argv, a);
    if (rc != 0) return rc - 1;
    if (a.query) return runQueries(a, stderr);
    if (a.compress) return runCompress(a, stderr);
    if (a.uncompress) return runUncompress(a, stderr);
    return runIndex(a, stderr);
}
}
