// bgzf_driver.cpp -- the host's BGZF encoder (yaha_amd/csrc/bgzf_core.h) as a program of its own, for tests/test_bam_cpu.py: built plainly and under
// AddressSanitizer + UBSan, started as a process.  `bgzf_driver IN OUT`: the bytes of IN cut into payloads, their blocks and the end-of-file block written to OUT.
// Every input is encoded twice, into buffers of exactly the promised size; the two results must be the same bytes (exit code 3 otherwise).
#include "../../yaha_amd/csrc/bgzf_core.h"
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>

int main(int argc, char **argv)
{
    if (argc != 3) { fprintf(stderr, "usage: bgzf_driver IN OUT\n"); return 2; }
    FILE *f = fopen(argv[1], "rb"); if (!f) { perror(argv[1]); return 2; }
    std::vector<uint8_t> in; uint8_t buf[1 << 16]; size_t got;
    while ((got = fread(buf, 1, sizeof buf, f)) > 0) in.insert(in.end(), buf, buf + got);
    fclose(f);
    std::unique_ptr<ybgzf::HostWork> W(new ybgzf::HostWork);
    std::vector<uint8_t> a(ybgzf::bound(in.size())), b(ybgzf::bound(in.size()));      // (exact: a block written past its slot is a sanitizer report)
    uint64_t blocksA = 0, storedA = 0, blocksB = 0, storedB = 0;
    const uint64_t na = ybgzf::encodeStream(in.data(), in.size(), a.data(), *W, &blocksA, &storedA);
    const uint64_t nb = ybgzf::encodeStream(in.data(), in.size(), b.data(), *W, &blocksB, &storedB);
    if (na != nb || blocksA != blocksB || storedA != storedB || (na && memcmp(a.data(), b.data(), na) != 0)) { fprintf(stderr, "the two encodings differ\n"); return 3; }
    if (blocksA != ybgzf::blocksOf(in.size()) || na > ybgzf::bound(in.size())) { fprintf(stderr, "block count or size out of bounds\n"); return 4; }
    uint8_t eof[ybgzf::EOF_BYTES]; ybgzf::putEof(eof);
    FILE *o = fopen(argv[2], "wb"); if (!o) { perror(argv[2]); return 2; }
    if ((na && fwrite(a.data(), 1, na, o) != na) || fwrite(eof, 1, sizeof eof, o) != sizeof eof || fclose(o) != 0) { perror(argv[2]); return 2; }
    printf("{\"bytes_in\": %zu, \"bytes_out\": %llu, \"blocks\": %llu, \"stored\": %llu}\n", in.size(), (unsigned long long)(na + sizeof eof), (unsigned long long)blocksA,
           (unsigned long long)storedA);
    return 0;
}
