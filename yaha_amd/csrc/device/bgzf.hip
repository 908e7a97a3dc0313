// bgzf.hip -- ygpu_bgzf_*: BGZF compression as a device primitive of its own (include/yaha_hip.h; the kernels are bgzf_stage.h, the format ../bgzf_core.h).
// A handle owns a stream, the device buffers -- the input, a slot of 65 536 bytes per block, the contiguous output, the blocks' sizes and offsets -- and
// page-locked staging for both directions; it shares nothing with a ygpu_ctx or another handle, so handles of different threads work side by side.
// One compress: the input through the staging buffer to the device, k_bgzf_deflate (a workgroup a block), k_bgzf_offsets, k_bgzf_gather, the total, then
// exactly the compressed bytes back -- two waits of the host, the second for the bytes.
#include "bgzf_stage.h"
#include <string>
#include <cstring>

struct ygpu_bgzf {
    int device = 0; uint64_t maxIn = 0; hipStream_t stream = nullptr;
    uint8_t *dIn = nullptr, *dSlots = nullptr, *dOut = nullptr; uint32_t *dSizes = nullptr; unsigned long long *dOffs = nullptr;
    uint8_t *hIn = nullptr, *hOut = nullptr; unsigned long long *hTotal = nullptr;
    std::string err;
};

#define BZCHK(call) do { hipError_t e_ = (call); \
    if (e_ != hipSuccess) { h->err = std::string(#call) + ": " + hipGetErrorString(e_); (void)hipGetLastError(); \
                            return e_ == hipErrorOutOfMemory ? YGPU_ENOMEM : YGPU_ENODEV; } } while (0)

extern "C" {

uint64_t ygpu_bgzf_bound(uint64_t n_in) { return ybgzf::bound(n_in); }

int ygpu_bgzf_open(int device, uint64_t max_in_bytes, ygpu_bgzf **out)
{
    if (!out) return YGPU_EINVAL;
    ygpu_bgzf *h = new ygpu_bgzf; *out = h; h->device = device; h->maxIn = max_in_bytes;
    int nDev = 0;
    if (hipGetDeviceCount(&nDev) != hipSuccess || device < 0 || device >= nDev) { (void)hipGetLastError(); h->err = "no such HIP device"; return YGPU_ENODEV; }
    if (max_in_bytes == 0 || ybgzf::blocksOf(max_in_bytes) > 0x7FFFFFFFull) { h->err = "max_in_bytes must be at least 1 and give fewer than 2^31 blocks"; return YGPU_EINVAL; }
    const uint64_t room = ybgzf::bound(max_in_bytes), nBlocks = ybgzf::blocksOf(max_in_bytes);
    BZCHK(hipSetDevice(device));
    BZCHK(hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking));
    BZCHK(hipMalloc((void **)&h->dIn, max_in_bytes + YBZ_PAD + 4));
    BZCHK(hipMemsetAsync(h->dIn, 0, max_in_bytes + YBZ_PAD + 4, h->stream));
    BZCHK(hipMalloc((void **)&h->dSlots, room));
    BZCHK(hipMalloc((void **)&h->dOut, room));
    BZCHK(hipMalloc((void **)&h->dSizes, 4 * nBlocks));
    BZCHK(hipMalloc((void **)&h->dOffs, 8 * (nBlocks + 1)));
    BZCHK(hipHostMalloc((void **)&h->hIn, max_in_bytes, hipHostMallocDefault));
    BZCHK(hipHostMalloc((void **)&h->hOut, room, hipHostMallocDefault));
    BZCHK(hipHostMalloc((void **)&h->hTotal, 8, hipHostMallocDefault));
    BZCHK(hipStreamSynchronize(h->stream));
    return 0;
}

int ygpu_bgzf_compress(ygpu_bgzf *h, const void *in, uint64_t n_in, void *out, uint64_t out_cap, uint64_t *n_out)
{
    if (!h) return YGPU_EINVAL;
    if (!n_out || (n_in && (!in || !out))) { h->err = "ygpu_bgzf_compress: null argument"; return YGPU_EINVAL; }
    *n_out = 0;
    if (!h->hTotal) { h->err = "ygpu_bgzf_compress: the handle was not opened"; return YGPU_EINVAL; }
    if (n_in > h->maxIn) { h->err = "ygpu_bgzf_compress: " + std::to_string(n_in) + " input bytes, the handle was opened for " + std::to_string(h->maxIn); return YGPU_EINVAL; }
    if (out_cap < ybgzf::bound(n_in)) { h->err = "ygpu_bgzf_compress: out_cap " + std::to_string(out_cap) + " is below ygpu_bgzf_bound = " + std::to_string(ybgzf::bound(n_in));
        return YGPU_EINVAL; }
    if (n_in == 0) return 0;
    const uint32_t nBlocks = (uint32_t)ybgzf::blocksOf(n_in);
    BZCHK(hipSetDevice(h->device));
    memcpy(h->hIn, in, n_in);
    BZCHK(hipMemcpyAsync(h->dIn, h->hIn, n_in, hipMemcpyHostToDevice, h->stream));
    hipLaunchKernelGGL(k_bgzf_deflate, dim3(nBlocks), dim3(YBZ_BS), 0, h->stream, (const uint32_t *)h->dIn, (unsigned long long)n_in, h->dSlots, h->dSizes);
    BZCHK(hipGetLastError());
    hipLaunchKernelGGL(k_bgzf_offsets, dim3(1), dim3(YBZ_BS), 0, h->stream, (const uint32_t *)h->dSizes, nBlocks, h->dOffs);
    BZCHK(hipGetLastError());
    hipLaunchKernelGGL(k_bgzf_gather, dim3(nBlocks), dim3(YBZ_BS), 0, h->stream, (const uint8_t *)h->dSlots, (const uint32_t *)h->dSizes, (const unsigned long long *)h->dOffs,
                       h->dOut);
    BZCHK(hipGetLastError());
    BZCHK(hipMemcpyAsync(h->hTotal, h->dOffs + nBlocks, 8, hipMemcpyDeviceToHost, h->stream));
    BZCHK(hipStreamSynchronize(h->stream));
    const uint64_t total = *h->hTotal;
    if (total > ybgzf::bound(n_in) || total < 26ull * nBlocks) { h->err = "ygpu_bgzf_compress: the blocks' sizes do not add up (" + std::to_string(total) + " bytes)";
        return YGPU_EINTERNAL; }
    BZCHK(hipMemcpyAsync(h->hOut, h->dOut, total, hipMemcpyDeviceToHost, h->stream));
    BZCHK(hipStreamSynchronize(h->stream));
    memcpy(out, h->hOut, total);
    *n_out = total;
    return 0;
}

const char *ygpu_bgzf_last_error(ygpu_bgzf *h) { return h ? h->err.c_str() : "null handle"; }

int ygpu_bgzf_close(ygpu_bgzf *h)
{
    if (!h) return YGPU_EINVAL;
    if (h->stream || h->dIn) (void)hipSetDevice(h->device);
    if (h->stream) { (void)hipStreamSynchronize(h->stream); (void)hipStreamDestroy(h->stream); }
    void *dev[] = {h->dIn, h->dSlots, h->dOut, h->dSizes, h->dOffs}; for (void *p : dev) if (p) (void)hipFree(p);
    void *host[] = {h->hIn, h->hOut, h->hTotal}; for (void *p : host) if (p) (void)hipHostFree(p);
    (void)hipGetLastError();
    delete h;
    return 0;
}

}  // extern "C"
