// bgzf_codes_driver.cpp -- the code tables and the checksum algebra of yaha_amd/csrc/bgzf_core.h printed for tests/test_bam_cpu.py, which compares every line
// with tests/bgzf_model.py (RFC 1951's tables) and zlib.
// `bgzf_codes_driver codes D ...` (D ...: the first and the last distance of every distance code, as the caller's tables have them): one line per entry,
//   L b v n            literalBits(b), b = 0 .. 255
//   M len dist v n     matchBits(len, dist): every len 3 .. 258 with every D; every dist 1 .. 32 768 with len 4, 258
// `bgzf_codes_driver crc FILE`: for |A|, |B| in {0, 1, 255, 256, 257, 65 279}, A = FILE[0, |A|), B = FILE[|A|, |A| + |B|), one line
//   C |A| |B| crc32(A) crc32(B) crcShift(crc32(A), |B|) ^ crc32(B)
#include "../../yaha_amd/csrc/bgzf_core.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

static void match(uint32_t len, uint32_t dist) { const ybgzf::Bits t = ybgzf::matchBits(len, dist); printf("M %u %u %u %u\n", len, dist, t.v, t.n); }

int main(int argc, char **argv)
{
    if (argc >= 2 && !strcmp(argv[1], "codes")) {
        for (uint32_t b = 0; b < 256; b++) { const ybgzf::Bits t = ybgzf::literalBits(b); if (t.n != ybgzf::literalLen(b)) return 3; printf("L %u %u %u\n", b, t.v, t.n); }
        std::vector<uint32_t> edges; for (int i = 2; i < argc; i++) edges.push_back((uint32_t)strtoul(argv[i], nullptr, 10));
        for (uint32_t len = 3; len <= ybgzf::MAX_MATCH; len++) for (uint32_t d : edges) match(len, d);
        for (uint32_t d = 1; d <= ybgzf::MAX_DIST; d++) { match(4, d); match(258, d); }
        return 0;
    }
    if (argc == 3 && !strcmp(argv[1], "crc")) {
        FILE *f = fopen(argv[2], "rb"); if (!f) { perror(argv[2]); return 2; }
        std::vector<uint8_t> in(2 * 65279); if (fread(in.data(), 1, in.size(), f) != in.size()) { fprintf(stderr, "%s: too short\n", argv[2]); return 2; }
        fclose(f);
        uint32_t tab[256]; for (uint32_t i = 0; i < 256; i++) tab[i] = ybgzf::crcEntry(i);
        const uint32_t sizes[] = {0, 1, 255, 256, 257, 65279};
        for (uint32_t a : sizes) for (uint32_t b : sizes) {
            const uint32_t ca = ybgzf::crc32(tab, in.data(), a), cb = ybgzf::crc32(tab, in.data() + a, b);
            printf("C %u %u %u %u %u\n", a, b, ca, cb, ybgzf::crcShift(ca, b) ^ cb);
        }
        return 0;
    }
    fprintf(stderr, "usage: bgzf_codes_driver codes D ... | crc FILE\n");
    return 2;
}
