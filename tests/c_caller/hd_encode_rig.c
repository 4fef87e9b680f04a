/* A plain-C caller of include/glc_hd.h (gcc, not hipcc): the device-only round trip of a CUHD-shaped stream on one
 * stream -- histogram, table (with the reference's 2048-entry decoder table), encode, decode with that table in device
 * memory -- then checks the device's stream against glcHdEncodeHost on the host's own table. */
#define __HIP_PLATFORM_AMD__ 1
#include <hip/hip_runtime_api.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "glc_hd.h"

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "HIP error %d at line %d\n", (int)e_, __LINE__); return 2; } } while (0)
#define CG(x) do { if (!(x)) { fprintf(stderr, "call failed at line %d\n", __LINE__); return 3; } } while (0)

int main(void)
{
    const size_t n = (1u << 22) + 12345;
    unsigned char *h_in = (unsigned char *)malloc(n), *h_back = (unsigned char *)malloc(n);
    srand(11);
    for (size_t i = 0; i < n; i++) {                       /* ~ Binomial(32, 0.5) + 100: a skewed alphabet */
        unsigned r = (unsigned)rand() ^ ((unsigned)rand() << 15), s = 0;
        for (int k = 0; k < 30; k++) s += (r >> k) & 1u;
        h_in[i] = (unsigned char)(100 + s + (rand() & 3));
    }
    const size_t cap = glcHdEncodeBound(n);
    unsigned char *d_in, *d_lens, *d_table, *d_out, *d_work, *d_dwork;
    unsigned short *d_codes;
    unsigned int *d_units;
    unsigned long long *d_hist, *d_nunits, nunits = 0;
    hipStream_t st;
    CK(hipStreamCreate(&st));
    CK(hipMalloc((void **)&d_in, n + 1)); CK(hipMalloc((void **)&d_out, n)); CK(hipMalloc((void **)&d_units, cap * 4));
    CK(hipMalloc((void **)&d_hist, 256 * 8)); CK(hipMalloc((void **)&d_lens, 256)); CK(hipMalloc((void **)&d_codes, 512));
    CK(hipMalloc((void **)&d_table, 4096)); CK(hipMalloc((void **)&d_nunits, 8));
    CK(hipMalloc((void **)&d_work, glcHdEncodeWorkBytes(n)));
    CK(hipMemcpy(d_in + 1, h_in, n, hipMemcpyHostToDevice));               /* an unaligned input */
    CG(glcHdHistogramDevice(d_in + 1, n, d_hist, st));
    CG(glcHdBuildTableDevice(d_hist, d_lens, d_codes, d_table, st));
    CG(glcHdEncodeDevice(d_in + 1, n, d_lens, d_codes, d_units, cap, d_nunits, d_work, st));
    CK(hipMemcpyAsync(&nunits, d_nunits, 8, hipMemcpyDeviceToHost, st));  /* the one host read */
    CK(hipStreamSynchronize(st));
    CG(nunits > 0);
    CK(hipMalloc((void **)&d_dwork, glcHdWorkBytes(nunits)));
    CG(glcHdDecodeDeviceTableOnDevice(d_units, nunits, d_table, d_out, n, d_dwork, st));
    CK(hipStreamSynchronize(st));
    CK(hipMemcpy(h_back, d_out, n, hipMemcpyDeviceToHost));
    const int round_trip = memcmp(h_in, h_back, n) == 0;

    /* the host's own path on the same bytes */
    unsigned long long hist[256] = {0}, dhist[256];
    unsigned char lens[256], dlens[256];
    unsigned short codes[256], dcodes[256];
    for (size_t i = 0; i < n; i++) hist[h_in[i]]++;
    CG(glcHdBuildTable(hist, lens, codes));
    unsigned int *h_units = (unsigned int *)malloc(cap * 4), *g_units = (unsigned int *)malloc(nunits * 4);
    const size_t hn = glcHdEncodeHost(h_in, n, lens, codes, h_units, cap);
    CK(hipMemcpy(dhist, d_hist, sizeof dhist, hipMemcpyDeviceToHost));
    CK(hipMemcpy(dlens, d_lens, 256, hipMemcpyDeviceToHost));
    CK(hipMemcpy(dcodes, d_codes, 512, hipMemcpyDeviceToHost));
    CK(hipMemcpy(g_units, d_units, nunits * 4, hipMemcpyDeviceToHost));
    const int equal_host = hn == nunits && memcmp(hist, dhist, sizeof hist) == 0 && memcmp(lens, dlens, 256) == 0 &&
                           memcmp(codes, dcodes, 512) == 0 && memcmp(h_units, g_units, nunits * 4) == 0;
    printf("symbols=%zu units=%llu round_trip=%d equal_host=%d\n", n, nunits, round_trip, equal_host);
    CK(hipStreamDestroy(st));
    return round_trip && equal_host ? 0 : 1;
}
