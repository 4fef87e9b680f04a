/* A plain-C caller of the filter's delta mode in include/glc_container.h (gcc, not hipcc): int64 timestamps through one COMPRESS
 * plan with the order-0 codec, shuffle 8 alone and with the delta on, a device round trip of the version-4 container by a plan
 * whose own delta is off, and glcDeltaShuffleDevice / glcUndeltaUnshuffleDevice on their own.  Prints the two container lengths,
 * the version, flags and element-size fields of the version-4 header, what the setters refused, and whether the decoded, the
 * filtered and the restored bytes are what they must be. */
#define __HIP_PLATFORM_AMD__ 1
#include <hip/hip_runtime_api.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "glc_container.h"

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "HIP error %d at line %d\n", (int)e_, __LINE__); return 2; } } while (0)
#define CR(x) do { CUDPPResult r_ = (x); if (r_ != CUDPP_SUCCESS) { fprintf(stderr, "CUDPPResult %d at line %d\n", (int)r_, __LINE__); return 3; } } while (0)

int main(void)
{
    const size_t n = 65536, count = 9 * n / 8 + 300, len = 8 * count + 5;     /* a ragged tail that is no whole element */
    unsigned char *h_in = (unsigned char *)malloc(len), *h_back = (unsigned char *)malloc(len), *h_filt = (unsigned char *)malloc(len);
    unsigned long long t = 1700000000000ull;
    srand(12);
    for (size_t i = 0; i < count; i++) {
        t += 900 + (unsigned long long)(rand() % 200);
        memcpy(h_in + 8 * i, &t, 8);
    }
    for (int i = 0; i < 5; i++) h_in[8 * count + i] = (unsigned char)(i + 1);
    const unsigned long long cap = glcContainerBound(len, n);
    unsigned char *d_in, *d_out, *d_back, *d_filt, hdr[32];
    unsigned long long *d_len, off_len = 0, on_len = 0, blen = 0;
    unsigned int on = 99;
    CK(hipMalloc((void **)&d_in, len)); CK(hipMalloc((void **)&d_out, cap)); CK(hipMalloc((void **)&d_back, len));
    CK(hipMalloc((void **)&d_filt, len)); CK(hipMalloc((void **)&d_len, 8));
    CK(hipMemcpy(d_in, h_in, len, hipMemcpyHostToDevice));
    CUDPPHandle lib, plan;
    CUDPPConfiguration cfg = {CUDPP_COMPRESS, CUDPP_ADD, CUDPP_UCHAR, 0, CUDPP_DEFAULT_BUCKET_MAPPER};
    CR(cudppCreate(&lib));
    CR(cudppPlan(lib, &plan, cfg, n, 8, 0));
    CR(glcPlanGetContainerDelta(plan, &on));
    if (on != 0) return 4;                                      /* off by default */
    int refused = glcPlanSetContainerDelta(plan, 1) == CUDPP_ERROR_ILLEGAL_CONFIGURATION;      /* the shuffle is off */
    CR(glcPlanSetContainerCodec(plan, GLC_CONTAINER_CODEC_HUFF0));
    CR(glcPlanSetContainerShuffle(plan, 8));
    refused &= glcPlanSetContainerDelta(plan, 2) == CUDPP_ERROR_ILLEGAL_CONFIGURATION;
    CR(glcContainerCompressDevice(plan, d_in, len, d_out, cap, d_len));
    CK(hipMemcpy(&off_len, d_len, 8, hipMemcpyDeviceToHost));
    CR(glcPlanSetContainerDelta(plan, 1));
    CR(glcPlanGetContainerDelta(plan, &on));
    CR(glcContainerCompressDevice(plan, d_in, len, d_out, cap, d_len));
    CK(hipMemcpy(&on_len, d_len, 8, hipMemcpyDeviceToHost));
    CK(hipMemcpy(hdr, d_out, 32, hipMemcpyDeviceToHost));
    CR(glcPlanSetContainerShuffle(plan, 0));                    /* clears the delta too; the decoder reads the stream header */
    unsigned int cleared = 99;
    CR(glcPlanGetContainerDelta(plan, &cleared));
    CR(glcContainerDecompressDevice(plan, d_out, on_len, d_back, len, d_len));
    CK(hipMemcpy(&blen, d_len, 8, hipMemcpyDeviceToHost));
    CK(hipMemcpy(h_back, d_back, len, hipMemcpyDeviceToHost));
    const int equal = blen == len && memcmp(h_in, h_back, len) == 0;
    CR(glcDeltaShuffleDevice(d_in, d_filt, len, 8, NULL));
    CR(glcUndeltaUnshuffleDevice(d_filt, d_back, len, 8, NULL));
    CK(hipDeviceSynchronize());
    CK(hipMemcpy(h_filt, d_filt, len, hipMemcpyDeviceToHost));
    CK(hipMemcpy(h_back, d_back, len, hipMemcpyDeviceToHost));
    int planes = 1;
    unsigned long long prev = 0;
    for (size_t i = 0; i < count && planes; i++) {
        unsigned long long x, d;
        memcpy(&x, h_in + 8 * i, 8);
        d = i % 2048 == 0 ? x : x - prev;
        prev = x;
        for (int j = 0; j < 8; j++) planes &= h_filt[(size_t)j * count + i] == (unsigned char)(d >> (8 * j));
    }
    planes &= memcmp(h_filt + 8 * count, h_in + 8 * count, 5) == 0;
    printf("off_len=%llu on_len=%llu version=%d flags=%d elem=%d delta_on=%u cleared=%u refused=%d decoded_len=%llu equal=%d planes=%d restored=%d\n",
           off_len, on_len, hdr[4] | (hdr[5] << 8), hdr[6] | (hdr[7] << 8), hdr[12], on, cleared, refused, blen, equal, planes,
           memcmp(h_in, h_back, len) == 0);
    CR(cudppDestroyPlan(plan));
    CR(cudppDestroy(lib));
    return 0;
}
