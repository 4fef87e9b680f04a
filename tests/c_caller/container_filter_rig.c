/* A plain-C caller of the shuffle filter in include/glc_container.h (gcc, not hipcc): float32 samples of a smooth signal through
 * one COMPRESS plan with the filter off and with element size 4, a device round trip of the filtered container, and
 * glcShuffleDevice / glcUnshuffleDevice on their own.  Prints the two container lengths, the version and element-size fields of
 * the filtered header, and whether the decoded and the unshuffled bytes equal the input.  With a file name as its argument
 * the input is read from that file (the test writes it, so that it can hold the CPU model's containers of the same bytes beside
 * the rig's: sinf and float accumulation are not reproduced bit for bit elsewhere); without one the signal is made here.  The
 * CRC-32 of the input and the length and CRC-32 of both containers are printed BEFORE anything is decoded: a failed decode then
 * says whether the encoder wrote wrong bytes or the decoder misread right ones. */
#define __HIP_PLATFORM_AMD__ 1
#include <hip/hip_runtime_api.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "glc_container.h"

static unsigned crc32(const void *p, size_t n)
{
    const unsigned char *b = (const unsigned char *)p;
    unsigned c = 0xFFFFFFFFu;
    for (size_t i = 0; i < n; i++) { c ^= b[i]; for (int k = 0; k < 8; k++) c = (c >> 1) ^ (0xEDB88320u & (0u - (c & 1u))); }
    return c ^ 0xFFFFFFFFu;
}

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "HIP error %d at line %d\n", (int)e_, __LINE__); return 2; } } while (0)
/* a failing call also says what the container's last error was (what, frame, block) and HIP's, once there is a plan */
static CUDPPHandle plan = 0;
static int refused(CUDPPResult r, int line)
{
    unsigned long long e[3] = {0, 0, 0};
    fprintf(stderr, "CUDPPResult %d at line %d", (int)r, line);
    if (plan && glcContainerLastError(plan, e) == CUDPP_SUCCESS)
        fprintf(stderr, ", container last error (%llu, %lld, %lld), hip last error %d", e[0], (long long)e[1], (long long)e[2], (int)hipGetLastError());
    fprintf(stderr, "\n");
    return 3;
}
#define CR(x) do { CUDPPResult r_ = (x); if (r_ != CUDPP_SUCCESS) return refused(r_, __LINE__); } while (0)

int main(int argc, char **argv)
{
    const size_t n = 65536, count = 9 * n / 4 + 300, len = 4 * count + 3;     /* a ragged tail that is no whole element */
    unsigned char *h_in = (unsigned char *)malloc(len), *h_back = (unsigned char *)malloc(len), *h_shuf = (unsigned char *)malloc(len);
    if (argc > 1) {
        FILE *fin = fopen(argv[1], "rb");
        if (!fin || fread(h_in, 1, len, fin) != len || fgetc(fin) != EOF) { fprintf(stderr, "%s does not hold %zu bytes\n", argv[1], len); return 6; }
        fclose(fin);
    } else {
        float walk = 0.0f;
        srand(11);
        for (size_t i = 0; i < count; i++) {
            walk += 0.01f * (float)(rand() % 201 - 100) / 100.0f;
            const float v = 100.0f * sinf((float)i * 0.00125f) + walk;
            memcpy(h_in + 4 * i, &v, 4);
        }
        h_in[len - 3] = 1; h_in[len - 2] = 2; h_in[len - 1] = 3;
    }
    const unsigned long long cap = glcContainerBound(len, n);
    unsigned char *d_in, *d_out, *d_back, *d_shuf, hdr[32];
    unsigned long long *d_len, off_len = 0, on_len = 0, blen = 0;
    unsigned int elem = 99;
    CK(hipMalloc((void **)&d_in, len)); CK(hipMalloc((void **)&d_out, cap)); CK(hipMalloc((void **)&d_back, len));
    CK(hipMalloc((void **)&d_shuf, len)); CK(hipMalloc((void **)&d_len, 8));
    CK(hipMemcpy(d_in, h_in, len, hipMemcpyHostToDevice));
    CUDPPHandle lib;
    CUDPPConfiguration cfg = {CUDPP_COMPRESS, CUDPP_ADD, CUDPP_UCHAR, 0, CUDPP_DEFAULT_BUCKET_MAPPER};
    CR(cudppCreate(&lib));
    CR(cudppPlan(lib, &plan, cfg, n, 4, 0));
    CR(glcPlanGetContainerShuffle(plan, &elem));
    if (elem != 0) return 4;                                    /* off by default */
    CR(glcContainerCompressDevice(plan, d_in, len, d_out, cap, d_len));
    CK(hipMemcpy(&off_len, d_len, 8, hipMemcpyDeviceToHost));
    unsigned char *h_cont = (unsigned char *)malloc(cap);
    CK(hipMemcpy(h_cont, d_out, off_len, hipMemcpyDeviceToHost));
    const unsigned off_crc = crc32(h_cont, off_len);
    if (glcPlanSetContainerShuffle(plan, 3) != CUDPP_ERROR_ILLEGAL_CONFIGURATION) return 5;
    CR(glcPlanSetContainerShuffle(plan, 4));
    CR(glcContainerCompressDevice(plan, d_in, len, d_out, cap, d_len));
    CK(hipMemcpy(&on_len, d_len, 8, hipMemcpyDeviceToHost));
    CK(hipMemcpy(hdr, d_out, 32, hipMemcpyDeviceToHost));
    CK(hipMemcpy(h_cont, d_out, on_len, hipMemcpyDeviceToHost));
    printf("input_crc=%08x off_len=%llu off_crc=%08x on_len=%llu on_crc=%08x\n", crc32(h_in, len), off_len, off_crc, on_len,
           crc32(h_cont, on_len));
    fflush(stdout);
    free(h_cont);
    CR(glcPlanSetContainerShuffle(plan, 0));                    /* the decoder reads the element size from the stream */
    CR(glcContainerDecompressDevice(plan, d_out, on_len, d_back, len, d_len));
    CK(hipMemcpy(&blen, d_len, 8, hipMemcpyDeviceToHost));
    CK(hipMemcpy(h_back, d_back, len, hipMemcpyDeviceToHost));
    const int equal = blen == len && memcmp(h_in, h_back, len) == 0;
    CR(glcShuffleDevice(d_in, d_shuf, len, 4, NULL));
    CR(glcUnshuffleDevice(d_shuf, d_back, len, 4, NULL));
    CK(hipDeviceSynchronize());
    CK(hipMemcpy(h_shuf, d_shuf, len, hipMemcpyDeviceToHost));
    CK(hipMemcpy(h_back, d_back, len, hipMemcpyDeviceToHost));
    int planes = 1;
    for (size_t i = 0; i < count && planes; i++)
        for (int j = 0; j < 4; j++) planes &= h_shuf[(size_t)j * count + i] == h_in[4 * i + j];
    planes &= memcmp(h_shuf + 4 * count, h_in + 4 * count, 3) == 0;
    printf("off_len=%llu on_len=%llu version=%d elem=%d decoded_len=%llu equal=%d planes=%d unshuffled=%d\n", off_len, on_len,
           hdr[4] | (hdr[5] << 8), hdr[12], blen, equal, planes, memcmp(h_in, h_back, len) == 0);
    CR(cudppDestroyPlan(plan));
    CR(cudppDestroy(lib));
    return 0;
}
