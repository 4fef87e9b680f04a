/* A plain-C caller of the container codec setting in include/glc_container.h (gcc, not hipcc): skewed i.i.d. bytes through one
 * COMPRESS plan with the default codec and with GLC_CONTAINER_CODEC_HUFF0, the version field of each header, a device round
 * trip of the order-0 container by a plan whose own codec is BWT again.  Prints the codec a plan starts with, the two container
 * lengths and versions, whether a bad codec is refused and whether the decoded bytes equal the input. */
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
    const size_t n = 65536, len = 9 * n + 1235;
    unsigned char *h_in = (unsigned char *)malloc(len), *h_back = (unsigned char *)malloc(len), hdr[32];
    srand(7);
    for (size_t i = 0; i < len; i++) {                          /* symbol k with probability about 2^-(k+1) */
        int r = rand(), k = 0;
        while ((r & 1) && k < 40) { r >>= 1; k++; }
        h_in[i] = (unsigned char)(3 * k);
    }
    const unsigned long long cap = glcContainerBound(len, n);
    unsigned char *d_in, *d_out, *d_back;
    unsigned long long *d_len, bwt_len = 0, huff0_len = 0, blen = 0;
    unsigned int codec = 99;
    CK(hipMalloc((void **)&d_in, len)); CK(hipMalloc((void **)&d_out, cap)); CK(hipMalloc((void **)&d_back, len));
    CK(hipMalloc((void **)&d_len, 8));
    CK(hipMemcpy(d_in, h_in, len, hipMemcpyHostToDevice));
    CUDPPHandle lib, plan;
    CUDPPConfiguration cfg = {CUDPP_COMPRESS, CUDPP_ADD, CUDPP_UCHAR, 0, CUDPP_DEFAULT_BUCKET_MAPPER};
    CR(cudppCreate(&lib));
    CR(cudppPlan(lib, &plan, cfg, n, 4, 0));
    CR(glcPlanGetContainerCodec(plan, &codec));
    const unsigned int default_codec = codec;
    CR(glcContainerCompressDevice(plan, d_in, len, d_out, cap, d_len));
    CK(hipMemcpy(&bwt_len, d_len, 8, hipMemcpyDeviceToHost));
    CK(hipMemcpy(hdr, d_out, 32, hipMemcpyDeviceToHost));
    const int bwt_version = hdr[4] | (hdr[5] << 8);
    const int refused = glcPlanSetContainerCodec(plan, 2) == CUDPP_ERROR_ILLEGAL_CONFIGURATION;
    CR(glcPlanSetContainerCodec(plan, GLC_CONTAINER_CODEC_HUFF0));
    CR(glcPlanGetContainerCodec(plan, &codec));
    if (codec != GLC_CONTAINER_CODEC_HUFF0) return 4;
    CR(glcContainerCompressDevice(plan, d_in, len, d_out, cap, d_len));
    CK(hipMemcpy(&huff0_len, d_len, 8, hipMemcpyDeviceToHost));
    CK(hipMemcpy(hdr, d_out, 32, hipMemcpyDeviceToHost));
    CR(glcPlanSetContainerCodec(plan, GLC_CONTAINER_CODEC_BWT));      /* the decoder reads what was done from the stream */
    CR(glcContainerDecompressDevice(plan, d_out, huff0_len, d_back, len, d_len));
    CK(hipMemcpy(&blen, d_len, 8, hipMemcpyDeviceToHost));
    CK(hipMemcpy(h_back, d_back, len, hipMemcpyDeviceToHost));
    printf("default_codec=%u bwt_len=%llu bwt_version=%d huff0_len=%llu huff0_version=%d bad_codec_refused=%d decoded_len=%llu equal=%d\n",
           default_codec, bwt_len, bwt_version, huff0_len, hdr[4] | (hdr[5] << 8), refused, blen,
           blen == len && memcmp(h_in, h_back, len) == 0);
    CR(cudppDestroyPlan(plan));
    CR(cudppDestroy(lib));
    return 0;
}
