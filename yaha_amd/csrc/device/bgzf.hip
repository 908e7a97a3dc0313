// bgzf.hip -- ygpu_bgzf_*: BGZF compression as a device primitive of its own (include/yaha_hip.h; the kernels are bgzf_stage.h, the format ../bgzf_core.h).
// A handle owns a stream, the device buffers -- the input, a slot of 65 536 bytes per block, the contiguous output, the blocks' sizes and offsets -- and
// page-locked staging for both directions; it shares nothing with a ygpu_ctx or another handle, so handles of different threads work side by side.
// One compress: the input through the staging buffer to the device, k_bgzf_deflate (a workgroup a block), k_bgzf_offsets, k_bgzf_gather, the total, then
// exactly the compressed bytes back -- two waits of the host, the second for the bytes.
// ygpu_bamsort_* (-obsort; the kernels are bamsort_stage.h): the run's records in segments of device memory, their order by a radix sort, and the sorted stream
// window by window through the same three kernels (bzDeflate: everything of a compress behind its upload) -- the uncompressed bytes never return to the host.
#include "bgzf_stage.h"
#include "bamsort_stage.h"
#include <string>
#include <cstring>
#include <vector>
#include <algorithm>

// what the deflate launches work in: a slot per block, the contiguous output, the blocks' sizes and offsets, page-locked memory for the result
struct BzWork {
    uint8_t *dSlots = nullptr, *dOut = nullptr; uint32_t *dSizes = nullptr; unsigned long long *dOffs = nullptr;
    uint8_t *hOut = nullptr; unsigned long long *hTotal = nullptr;
};
struct ygpu_bgzf {
    int device = 0; uint64_t maxIn = 0; hipStream_t stream = nullptr;
    uint8_t *dIn = nullptr; BzWork z; uint8_t *hIn = nullptr;
    std::string err;
};

#define BZCHK(call) do { hipError_t e_ = (call); \
    if (e_ != hipSuccess) { err_ = std::string(#call) + ": " + hipGetErrorString(e_); (void)hipGetLastError(); \
                            return e_ == hipErrorOutOfMemory ? YGPU_ENOMEM : YGPU_ENODEV; } } while (0)

static int bzWorkAlloc(BzWork &z, uint64_t maxIn, std::string &err_)
{
    const uint64_t room = ybgzf::bound(maxIn), nBlocks = ybgzf::blocksOf(maxIn);
    BZCHK(hipMalloc((void **)&z.dSlots, room));
    BZCHK(hipMalloc((void **)&z.dOut, room));
    BZCHK(hipMalloc((void **)&z.dSizes, 4 * nBlocks));
    BZCHK(hipMalloc((void **)&z.dOffs, 8 * (nBlocks + 1)));
    BZCHK(hipHostMalloc((void **)&z.hOut, room, hipHostMallocDefault));
    BZCHK(hipHostMalloc((void **)&z.hTotal, 8, hipHostMallocDefault));
    return 0;
}
static void bzWorkFree(BzWork &z)
{
    void *dev[] = {z.dSlots, z.dOut, z.dSizes, z.dOffs}; for (void *p : dev) if (p) (void)hipFree(p);
    void *host[] = {z.hOut, z.hTotal}; for (void *p : host) if (p) (void)hipHostFree(p);
    z = BzWork();
}
// dIn[0 .. n_in) (word-aligned, YBZ_PAD readable bytes behind it) as whole BGZF blocks into out: the three kernels, the total, the bytes -- two waits
static int bzDeflate(hipStream_t stream, const uint8_t *dIn, uint64_t n_in, BzWork &z, void *out, uint64_t *n_out, std::string &err_, const char *who)
{
    const uint32_t nBlocks = (uint32_t)ybgzf::blocksOf(n_in);
    hipLaunchKernelGGL(k_bgzf_deflate, dim3(nBlocks), dim3(YBZ_BS), 0, stream, (const uint32_t *)dIn, (unsigned long long)n_in, z.dSlots, z.dSizes);
    BZCHK(hipGetLastError());
    hipLaunchKernelGGL(k_bgzf_offsets, dim3(1), dim3(YBZ_BS), 0, stream, (const uint32_t *)z.dSizes, nBlocks, z.dOffs);
    BZCHK(hipGetLastError());
    hipLaunchKernelGGL(k_bgzf_gather, dim3(nBlocks), dim3(YBZ_BS), 0, stream, (const uint8_t *)z.dSlots, (const uint32_t *)z.dSizes, (const unsigned long long *)z.dOffs, z.dOut);
    BZCHK(hipGetLastError());
    BZCHK(hipMemcpyAsync(z.hTotal, z.dOffs + nBlocks, 8, hipMemcpyDeviceToHost, stream));
    BZCHK(hipStreamSynchronize(stream));
    const uint64_t total = *z.hTotal;
    if (total > ybgzf::bound(n_in) || total < 26ull * nBlocks) { err_ = std::string(who) + ": the blocks' sizes do not add up (" + std::to_string(total) + " bytes)";
        return YGPU_EINTERNAL; }
    BZCHK(hipMemcpyAsync(z.hOut, z.dOut, total, hipMemcpyDeviceToHost, stream));
    BZCHK(hipStreamSynchronize(stream));
    memcpy(out, z.hOut, total);
    *n_out = total;
    return 0;
}

extern "C" {

uint64_t ygpu_bgzf_bound(uint64_t n_in) { return ybgzf::bound(n_in); }

int ygpu_bgzf_open(int device, uint64_t max_in_bytes, ygpu_bgzf **out)
{
    if (!out) return YGPU_EINVAL;
    ygpu_bgzf *h = new ygpu_bgzf; *out = h; h->device = device; h->maxIn = max_in_bytes; std::string &err_ = h->err;
    int nDev = 0;
    if (hipGetDeviceCount(&nDev) != hipSuccess || device < 0 || device >= nDev) { (void)hipGetLastError(); h->err = "no such HIP device"; return YGPU_ENODEV; }
    if (max_in_bytes == 0 || ybgzf::blocksOf(max_in_bytes) > 0x7FFFFFFFull) { h->err = "max_in_bytes must be at least 1 and give fewer than 2^31 blocks"; return YGPU_EINVAL; }
    BZCHK(hipSetDevice(device));
    BZCHK(hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking));
    BZCHK(hipMalloc((void **)&h->dIn, max_in_bytes + YBZ_PAD + 4));
    BZCHK(hipMemsetAsync(h->dIn, 0, max_in_bytes + YBZ_PAD + 4, h->stream));
    { const int rc = bzWorkAlloc(h->z, max_in_bytes, h->err); if (rc != 0) return rc; }
    BZCHK(hipHostMalloc((void **)&h->hIn, max_in_bytes, hipHostMallocDefault));
    BZCHK(hipStreamSynchronize(h->stream));
    return 0;
}

int ygpu_bgzf_compress(ygpu_bgzf *h, const void *in, uint64_t n_in, void *out, uint64_t out_cap, uint64_t *n_out)
{
    if (!h) return YGPU_EINVAL;
    std::string &err_ = h->err;
    if (!n_out || (n_in && (!in || !out))) { h->err = "ygpu_bgzf_compress: null argument"; return YGPU_EINVAL; }
    *n_out = 0;
    if (!h->z.hTotal) { h->err = "ygpu_bgzf_compress: the handle was not opened"; return YGPU_EINVAL; }
    if (n_in > h->maxIn) { h->err = "ygpu_bgzf_compress: " + std::to_string(n_in) + " input bytes, the handle was opened for " + std::to_string(h->maxIn); return YGPU_EINVAL; }
    if (out_cap < ybgzf::bound(n_in)) { h->err = "ygpu_bgzf_compress: out_cap " + std::to_string(out_cap) + " is below ygpu_bgzf_bound = " + std::to_string(ybgzf::bound(n_in));
        return YGPU_EINVAL; }
    if (n_in == 0) return 0;
    BZCHK(hipSetDevice(h->device));
    memcpy(h->hIn, in, n_in);
    BZCHK(hipMemcpyAsync(h->dIn, h->hIn, n_in, hipMemcpyHostToDevice, h->stream));
    return bzDeflate(h->stream, h->dIn, n_in, h->z, out, n_out, h->err, "ygpu_bgzf_compress");
}

const char *ygpu_bgzf_last_error(ygpu_bgzf *h) { return h ? h->err.c_str() : "null handle"; }

int ygpu_bgzf_close(ygpu_bgzf *h)
{
    if (!h) return YGPU_EINVAL;
    if (h->stream || h->dIn || h->z.dSlots) (void)hipSetDevice(h->device);
    if (h->stream) { (void)hipStreamSynchronize(h->stream); (void)hipStreamDestroy(h->stream); }
    if (h->dIn) (void)hipFree(h->dIn);
    if (h->hIn) (void)hipHostFree(h->hIn);
    bzWorkFree(h->z);
    (void)hipGetLastError();
    delete h;
    return 0;
}

}  // extern "C"

// ---- ygpu_bamsort_* -------------------------------------------------------------------------------------------------------------------------------------------------
// Defaults: segments of 256 MB (a run of 1 M reads of 1 kbp is seven of them), windows of 1024 payloads (66.8 MB raw: 64 MB of slots, 64 MB of output and as
// much page-locked memory beside the window itself).  Staging: two page-locked buffers of 8 MB that an append fills in turn while the other one's copy runs.
enum : uint64_t { YBS_SEGMENT_DEFAULT = 256ull << 20, YBS_WINDOW_PAYLOADS = 1024, YBS_STAGE_BYTES = 8ull << 20, YBS_SEG_PAD = 8 };

struct ygpu_bamsort {
    int device = 0; uint64_t maxStore = 0, segBytes = 0, winBytes = 0; hipStream_t stream = nullptr;
    struct Segment { uint8_t *p; uint64_t cap, used; };
    std::vector<Segment> segs; uint64_t storeBytes = 0;                               // device memory of the store: the segments and the per-record arrays
    // per record, in append order (capacity recCap, grown by doubling): address, length, key; the sort's second key array and its two value arrays
    unsigned long long *dAddr = nullptr, *dKey = nullptr, *dKey2 = nullptr, *dOffs = nullptr; uint32_t *dLen = nullptr, *dValA = nullptr, *dValB = nullptr, *dTable = nullptr;
    uint32_t *dPerm = nullptr; uint64_t nRec = 0, recCap = 0;
    uint8_t *hStage[2] = {nullptr, nullptr}; hipEvent_t stageDone[2] = {nullptr, nullptr}; int stageAt = 0;
    uint64_t keyOr = 0, keyAnd = ~0ull;                                               // over every key appended: a digit that is the same in all keys needs no pass
    bool sorted = false; uint64_t total = 0, nextWin = 0, passes = 0, windows = 0;
    std::vector<unsigned long long> hOffs;                                            // the sorted records' stream offsets (n + 1), for the windows' binary search
    uint8_t *dWin = nullptr; BzWork z;
    std::vector<unsigned long long> tmpAddr;
    std::string err;
};

// n bytes from the host's src to the device's dst through the two staging buffers, asynchronously on the handle's stream
static int bsStage(ygpu_bamsort *h, void *dst, const void *src, uint64_t n)
{
    std::string &err_ = h->err;
    for (uint64_t at = 0; at < n;) {
        const uint64_t part = std::min<uint64_t>(YBS_STAGE_BYTES, n - at); const int b = h->stageAt; h->stageAt ^= 1;
        BZCHK(hipEventSynchronize(h->stageDone[b]));                                   // (the copy that last used this buffer)
        memcpy(h->hStage[b], (const uint8_t *)src + at, part);
        BZCHK(hipMemcpyAsync((uint8_t *)dst + at, h->hStage[b], part, hipMemcpyHostToDevice, h->stream));
        BZCHK(hipEventRecord(h->stageDone[b], h->stream));
        at += part;
    }
    return 0;
}
// room for `need` records in the per-record arrays (20 bytes a record count as the store's)
static int bsGrow(ygpu_bamsort *h, uint64_t need)
{
    std::string &err_ = h->err;
    if (need <= h->recCap) return 0;
    uint64_t cap = h->recCap ? h->recCap : 4096; while (cap < need) cap *= 2;
    if (cap > 0xFFFFFFFFull) cap = 0xFFFFFFFFull;
    if (h->storeBytes + 20 * (cap - h->recCap) > h->maxStore) cap = need;              // (doubling would pass the cap: exactly what is needed, if that fits)
    if (h->storeBytes + 20 * (cap - h->recCap) > h->maxStore) {
        h->err = "ygpu_bamsort_append: the arrays of " + std::to_string(need) + " records would pass max_store_bytes = " + std::to_string(h->maxStore); return YGPU_ENOMEM; }
    unsigned long long *a = nullptr, *k = nullptr; uint32_t *l = nullptr;
    BZCHK(hipMalloc((void **)&a, 8 * cap)); BZCHK(hipMalloc((void **)&k, 8 * cap)); BZCHK(hipMalloc((void **)&l, 4 * cap));
    if (h->nRec) {
        BZCHK(hipMemcpyAsync(a, h->dAddr, 8 * h->nRec, hipMemcpyDeviceToDevice, h->stream)); BZCHK(hipMemcpyAsync(k, h->dKey, 8 * h->nRec, hipMemcpyDeviceToDevice, h->stream));
        BZCHK(hipMemcpyAsync(l, h->dLen, 4 * h->nRec, hipMemcpyDeviceToDevice, h->stream));
        BZCHK(hipStreamSynchronize(h->stream));
    }
    void *old[] = {h->dAddr, h->dKey, h->dLen}; for (void *p : old) if (p) (void)hipFree(p);
    h->dAddr = a; h->dKey = k; h->dLen = l; h->storeBytes += 20 * (cap - h->recCap); h->recCap = cap;
    return 0;
}

extern "C" {

int ygpu_bamsort_open(int device, uint64_t max_store_bytes, uint64_t segment_bytes, uint64_t window_bytes, ygpu_bamsort **out)
{
    if (!out) return YGPU_EINVAL;
    ygpu_bamsort *h = new ygpu_bamsort; *out = h; h->device = device; h->maxStore = max_store_bytes; std::string &err_ = h->err;
    h->segBytes = segment_bytes ? segment_bytes : (uint64_t)YBS_SEGMENT_DEFAULT;
    h->winBytes = window_bytes ? std::max<uint64_t>(1, window_bytes / ybgzf::PAYLOAD_MAX) * ybgzf::PAYLOAD_MAX : (uint64_t)YBS_WINDOW_PAYLOADS * ybgzf::PAYLOAD_MAX;
    int nDev = 0;
    if (hipGetDeviceCount(&nDev) != hipSuccess || device < 0 || device >= nDev) { (void)hipGetLastError(); h->err = "no such HIP device"; return YGPU_ENODEV; }
    if (max_store_bytes == 0 || ybgzf::blocksOf(h->winBytes) > 0x7FFFFFFFull) { h->err = "max_store_bytes must be at least 1 and a window fewer than 2^31 blocks";
        return YGPU_EINVAL; }
    BZCHK(hipSetDevice(device));
    BZCHK(hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking));
    for (int b = 0; b < 2; b++) { BZCHK(hipHostMalloc((void **)&h->hStage[b], YBS_STAGE_BYTES, hipHostMallocDefault)); BZCHK(hipEventCreateWithFlags(&h->stageDone[b],
        hipEventDisableTiming)); }
    return 0;
}

int ygpu_bamsort_append(ygpu_bamsort *h, const void *bytes, uint64_t n_bytes, const uint64_t *keys, const uint32_t *lens, uint32_t n_records)
{
    if (!h) return YGPU_EINVAL;
    std::string &err_ = h->err;
    if (!h->stream) { h->err = "ygpu_bamsort_append: the handle was not opened"; return YGPU_EINVAL; }
    if (h->sorted) { h->err = "ygpu_bamsort_append: the store was sorted already"; return YGPU_EINVAL; }
    if (n_records == 0) { if (n_bytes) { h->err = "ygpu_bamsort_append: bytes without records"; return YGPU_EINVAL; } return 0; }
    if (!bytes || !keys || !lens) { h->err = "ygpu_bamsort_append: null argument"; return YGPU_EINVAL; }
    if (h->nRec + n_records > 0xFFFFFFFFull) { h->err = "ygpu_bamsort_append: more than 2^32 - 1 records"; return YGPU_EINVAL; }
    uint64_t sum = 0; for (uint32_t i = 0; i < n_records; i++) sum += lens[i];
    if (sum != n_bytes) { h->err = "ygpu_bamsort_append: the records' lengths add up to " + std::to_string(sum) + ", n_bytes is " + std::to_string(n_bytes); return YGPU_EINVAL; }
    BZCHK(hipSetDevice(h->device));
    // the segment: the current one where the whole batch fits, else a new one (a batch never straddles two, so no record does)
    if (h->segs.empty() || h->segs.back().cap - h->segs.back().used < n_bytes) {
        const uint64_t cap = std::max<uint64_t>(n_bytes, h->segBytes);
        if (h->storeBytes + cap + YBS_SEG_PAD > h->maxStore) {
            h->err = "ygpu_bamsort_append: a segment of " + std::to_string(cap) + " bytes beside the " + std::to_string(h->storeBytes) +
                " the store holds would pass max_store_bytes = " +
                std::to_string(h->maxStore); return YGPU_ENOMEM; }
        uint8_t *p = nullptr;
        if (hipMalloc((void **)&p, cap + YBS_SEG_PAD) != hipSuccess) { (void)hipGetLastError();
            h->err = "ygpu_bamsort_append: the device cannot give a segment of " + std::to_string(cap) + " bytes (the store holds " + std::to_string(h->storeBytes) + ")";
                return YGPU_ENOMEM; }
        BZCHK(hipMemsetAsync(p + cap, 0, YBS_SEG_PAD, h->stream));
        h->segs.push_back(ygpu_bamsort::Segment{p, cap, 0}); h->storeBytes += cap + YBS_SEG_PAD;
    }
    { const int rc = bsGrow(h, h->nRec + n_records); if (rc != 0) return rc; }
    ygpu_bamsort::Segment &sg = h->segs.back();
    h->tmpAddr.resize(n_records); uint64_t at = sg.used;
    for (uint32_t i = 0; i < n_records; i++) { h->tmpAddr[i] = (unsigned long long)(uintptr_t)(sg.p + at); at += lens[i]; h->keyOr |= keys[i]; h->keyAnd &= keys[i]; }
    int rc = bsStage(h, sg.p + sg.used, bytes, n_bytes);
    if (rc == 0) rc = bsStage(h, h->dAddr + h->nRec, h->tmpAddr.data(), 8ull * n_records);
    if (rc == 0) rc = bsStage(h, h->dKey + h->nRec, keys, 8ull * n_records);
    if (rc == 0) rc = bsStage(h, h->dLen + h->nRec, lens, 4ull * n_records);
    if (rc != 0) return rc;
    sg.used += n_bytes; h->nRec += n_records;
    return 0;
}

int ygpu_bamsort_sort(ygpu_bamsort *h, uint32_t *perm)
{
    if (!h) return YGPU_EINVAL;
    std::string &err_ = h->err;
    if (!h->stream) { h->err = "ygpu_bamsort_sort: the handle was not opened"; return YGPU_EINVAL; }
    if (h->sorted) { h->err = "ygpu_bamsort_sort: the store was sorted already"; return YGPU_EINVAL; }
    BZCHK(hipSetDevice(h->device));
    const uint32_t n = (uint32_t)h->nRec, nTiles = (n + YBS_TILE - 1) / YBS_TILE;
    h->passes = 0; h->total = 0; h->hOffs.assign((size_t)n + 1, 0);
    if (n) {
        BZCHK(hipMalloc((void **)&h->dKey2, 8ull * n)); BZCHK(hipMalloc((void **)&h->dValA, 4ull * n)); BZCHK(hipMalloc((void **)&h->dValB, 4ull * n));
        BZCHK(hipMalloc((void **)&h->dTable, 4 * (256ull * nTiles + 1))); BZCHK(hipMalloc((void **)&h->dOffs, 8 * ((uint64_t)n + 1)));
        unsigned long long *kIn = h->dKey, *kOut = h->dKey2; uint32_t *vIn = h->dValA, *vOut = h->dValB;
        hipLaunchKernelGGL(k_bamsort_iota, dim3(nTiles), dim3(YBS_BS), 0, h->stream, vIn, n);
        BZCHK(hipGetLastError());
        const uint64_t differs = h->keyOr ^ h->keyAnd;                                 // (a pass over a digit every key shares would move nothing: the sort is stable)
        for (uint32_t d = 0; d < 8; d++) {
            if (((differs >> (8 * d)) & 255u) == 0) continue;
            hipLaunchKernelGGL(k_bamsort_hist, dim3(nTiles), dim3(YBS_BS), 0, h->stream, (const unsigned long long *)kIn, n, 8 * d, nTiles, h->dTable);
            BZCHK(hipGetLastError());
            hipLaunchKernelGGL(k_bamsort_sum<uint32_t>, dim3(1), dim3(YBS_BS), 0, h->stream, (const uint32_t *)h->dTable, (const uint32_t *)nullptr, 256ull * nTiles, h->dTable);
            BZCHK(hipGetLastError());
            hipLaunchKernelGGL(k_bamsort_scatter, dim3(nTiles), dim3(YBS_BS), 0, h->stream, (const unsigned long long *)kIn, (const uint32_t *)vIn, kOut, vOut, n, 8 * d, nTiles,
                               (const uint32_t *)h->dTable);
            BZCHK(hipGetLastError());
            std::swap(kIn, kOut); std::swap(vIn, vOut); h->passes++;
        }
        h->dPerm = vIn;
        hipLaunchKernelGGL(k_bamsort_sum<unsigned long long>, dim3(1), dim3(YBS_BS), 0, h->stream, (const uint32_t *)h->dLen, (const uint32_t *)h->dPerm, (unsigned long long)n,
            h->dOffs);
        BZCHK(hipGetLastError());
        BZCHK(hipMemcpyAsync(h->hOffs.data(), h->dOffs, 8 * ((uint64_t)n + 1), hipMemcpyDeviceToHost, h->stream));
        if (perm) BZCHK(hipMemcpyAsync(perm, h->dPerm, 4ull * n, hipMemcpyDeviceToHost, h->stream));
        BZCHK(hipStreamSynchronize(h->stream));
        h->total = h->hOffs[n];
        uint64_t stored = 0; for (auto &sg : h->segs) stored += sg.used;
        if (h->total != stored) { h->err = "ygpu_bamsort_sort: the sorted lengths add up to " + std::to_string(h->total) + ", the store holds " + std::to_string(stored);
            return YGPU_EINTERNAL; }
        for (uint32_t j = 0; j < n; j++) if (h->hOffs[j] > h->hOffs[j + 1]) { h->err = "ygpu_bamsort_sort: the stream offsets do not ascend"; return YGPU_EINTERNAL; }
        // the windows' buffers: the window with the bytes a search may read behind it, zeroed once, and what the deflate launches work in
        const uint64_t win = std::min<uint64_t>(h->winBytes, std::max<uint64_t>(h->total, 1));
        BZCHK(hipMalloc((void **)&h->dWin, win + YBZ_PAD + 4));
        BZCHK(hipMemsetAsync(h->dWin, 0, win + YBZ_PAD + 4, h->stream));
        { const int rc = bzWorkAlloc(h->z, win, h->err); if (rc != 0) return rc; }
        BZCHK(hipStreamSynchronize(h->stream));
    }
    h->sorted = true; h->nextWin = 0;
    return 0;
}

int ygpu_bamsort_next(ygpu_bamsort *h, void *out, uint64_t out_cap, uint64_t *n_out, uint64_t *n_raw)
{
    if (!h) return YGPU_EINVAL;
    std::string &err_ = h->err;
    if (!n_out || !n_raw) { h->err = "ygpu_bamsort_next: null argument"; return YGPU_EINVAL; }
    *n_out = 0; *n_raw = 0;
    if (!h->sorted) { h->err = "ygpu_bamsort_next: the store has not been sorted"; return YGPU_EINVAL; }
    const uint64_t w0 = h->nextWin * h->winBytes;
    if (w0 >= h->total) return 0;
    const uint64_t w1 = std::min<uint64_t>(w0 + h->winBytes, h->total), nIn = w1 - w0;
    if (!out || out_cap < ybgzf::bound(nIn)) {
        h->err = "ygpu_bamsort_next: out_cap " + std::to_string(out_cap) + " is below ygpu_bgzf_bound = " + std::to_string(ybgzf::bound(nIn));
        return YGPU_EINVAL; }
    BZCHK(hipSetDevice(h->device));
    // the records that intersect [w0, w1): the last one that starts at or before w0 up to the first that starts at or behind w1
    const uint32_t n = (uint32_t)h->nRec;
    const uint32_t j0 = (uint32_t)(std::upper_bound(h->hOffs.begin(), h->hOffs.begin() + n, (unsigned long long)w0) - h->hOffs.begin()) - 1u;
    const uint32_t j1 = (uint32_t)(std::lower_bound(h->hOffs.begin(), h->hOffs.begin() + n, (unsigned long long)w1) - h->hOffs.begin());
    if (j0 >= j1 || j1 > n) { h->err = "ygpu_bamsort_next: no record in window " + std::to_string(h->nextWin); return YGPU_EINTERNAL; }
    const uint32_t nRecs = j1 - j0, wavesPerBlock = YBS_BS / 64;
    hipLaunchKernelGGL(k_bam_gather, dim3((nRecs + wavesPerBlock - 1) / wavesPerBlock), dim3(YBS_BS), 0, h->stream, (const uint32_t *)h->dPerm,
        (const unsigned long long *)h->dOffs,
                       (const unsigned long long *)h->dAddr, (const uint32_t *)h->dLen, j0, nRecs, (unsigned long long)w0, (unsigned long long)w1, h->dWin);
    BZCHK(hipGetLastError());
    const int rc = bzDeflate(h->stream, h->dWin, nIn, h->z, out, n_out, h->err, "ygpu_bamsort_next");
    if (rc != 0) return rc;
    *n_raw = nIn; h->nextWin++; h->windows++;
    return 0;
}

uint64_t ygpu_bamsort_info(ygpu_bamsort *h, int what)
{
    if (what == YGPU_BAMSORT_TILE_KEYS) return YBS_TILE;
    if (!h) return 0;
    switch (what) {
    case YGPU_BAMSORT_PASSES: return h->passes;
    case YGPU_BAMSORT_SEGMENTS: return h->segs.size();
    case YGPU_BAMSORT_WINDOWS: return h->windows;
    case YGPU_BAMSORT_WINDOW_BYTES: return h->winBytes;
    case YGPU_BAMSORT_STORE_BYTES: return h->storeBytes;
    case YGPU_BAMSORT_RECORDS: return h->nRec;
    }
    return 0;
}

const char *ygpu_bamsort_last_error(ygpu_bamsort *h) { return h ? h->err.c_str() : "null handle"; }

int ygpu_bamsort_close(ygpu_bamsort *h)
{
    if (!h) return YGPU_EINVAL;
    if (h->stream) (void)hipSetDevice(h->device);
    if (h->stream) { (void)hipStreamSynchronize(h->stream); (void)hipStreamDestroy(h->stream); }
    for (auto &sg : h->segs) (void)hipFree(sg.p);
    void *dev[] = {h->dAddr, h->dKey, h->dKey2, h->dOffs, h->dLen, h->dValA, h->dValB, h->dTable, h->dWin}; for (void *p : dev) if (p) (void)hipFree(p);
    for (int b = 0; b < 2; b++) { if (h->hStage[b]) (void)hipHostFree(h->hStage[b]); if (h->stageDone[b]) (void)hipEventDestroy(h->stageDone[b]); }
    bzWorkFree(h->z);
    (void)hipGetLastError();
    delete h;
    return 0;
}

}  // extern "C"
