/* A plain-C caller of include/glc_container.h (gcc, not hipcc): a device round trip of a ragged input through one
 * COMPRESS plan, printing the container length, its CRC-32, the CRC-32 glcCrc32Segments reports for the input and whether
 * the decoded bytes equal the input.  The container's length and CRC-32 are printed BEFORE it is decoded (the test compares
 * them with the CPU model's), so that a failed decode says whether the encoder wrote wrong bytes or the decoder misread right
 * ones. */
#define __HIP_PLATFORM_AMD__ 1
#include <hip/hip_runtime_api.h>
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

int main(void)
{
    const size_t n = 65536, len = 3 * n + 12345;
    unsigned char *h_in = (unsigned char *)malloc(len), *h_back = (unsigned char *)malloc(len);
    srand(7);
    for (size_t i = 0; i < len; i++) h_in[i] = (unsigned char)("abcabd, the cat sat on the mat. "[rand() % 32] ^ ((i % 977) == 0));
    const unsigned long long cap = glcContainerBound(len, n);
    unsigned char *d_in, *d_out, *d_back, *h_cont;
    unsigned long long *d_len, clen = 0, blen = 0, *d_off, *d_ln;
    unsigned *d_crc, gcrc = 0;
    CK(hipMalloc((void **)&d_in, len)); CK(hipMalloc((void **)&d_out, cap)); CK(hipMalloc((void **)&d_back, len));
    CK(hipMalloc((void **)&d_len, 8)); CK(hipMalloc((void **)&d_off, 8)); CK(hipMalloc((void **)&d_ln, 8)); CK(hipMalloc((void **)&d_crc, 4));
    CK(hipMemcpy(d_in, h_in, len, hipMemcpyHostToDevice));
    CUDPPHandle lib;
    CUDPPConfiguration cfg = {CUDPP_COMPRESS, CUDPP_ADD, CUDPP_UCHAR, 0, CUDPP_DEFAULT_BUCKET_MAPPER};
    CR(cudppCreate(&lib));
    CR(cudppPlan(lib, &plan, cfg, n, 2, 0));
    CR(glcContainerCompressDevice(plan, d_in, len, d_out, cap, d_len));
    CK(hipMemcpy(&clen, d_len, 8, hipMemcpyDeviceToHost));
    h_cont = (unsigned char *)malloc(clen);
    CK(hipMemcpy(h_cont, d_out, clen, hipMemcpyDeviceToHost));
    const unsigned ccrc = crc32(h_cont, clen);
    printf("container_len=%llu container_crc=%08x\n", clen, ccrc);
    fflush(stdout);
    CR(glcContainerDecompressDevice(plan, d_out, clen, d_back, len, d_len));
    CK(hipMemcpy(&blen, d_len, 8, hipMemcpyDeviceToHost));
    CK(hipMemcpy(h_back, d_back, len, hipMemcpyDeviceToHost));
    unsigned long long zero = 0, l = len;
    CK(hipMemcpy(d_off, &zero, 8, hipMemcpyHostToDevice)); CK(hipMemcpy(d_ln, &l, 8, hipMemcpyHostToDevice));
    CR(glcCrc32Segments(d_in, d_off, d_ln, 1, d_crc, NULL));
    CK(hipDeviceSynchronize());
    CK(hipMemcpy(&gcrc, d_crc, 4, hipMemcpyDeviceToHost));
    printf("container_len=%llu container_crc=%08x input_crc=%08x gpu_crc=%08x decoded_len=%llu equal=%d\n", clen,
           ccrc, crc32(h_in, len), gcrc, blen, blen == len && memcmp(h_in, h_back, len) == 0);
    CR(cudppDestroyPlan(plan));
    CR(cudppDestroy(lib));
    return 0;
}
