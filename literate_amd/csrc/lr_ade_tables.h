// lr_ade_tables.h - what the profile (lr_ade.hip, --ade) and the joint sampler (lr_adej.hip, --ade_joint) both derive from
// lr_ade_classes' dead [A, A] and cens [A], and the pieces of the interval-censored Weibull likelihood they share.
//
// The tables: [hdr | death_bin | cls_cell | cls_n | cls_n32 | R | R32], each 256-byte aligned.
//   hdr                     long long [LR_ADE_HDR_*]
//   death_bin [A]           1 where a death was observed in the bin
//   cls_cell, cls_n, cls_n32  the cells (jb, a) with jb + a < A and a count > 0, in the order of the table (so every sum over
//                           them has one order): je | a << 16, and the count as a double and clamped to INT_MAX
//   R, R32                  R[jb][j] = max(cens[jb], 0) + sum_{a > j} dead[jb][a], the lineages of birth bin jb that live past
//                           age j, as a packed triangle (row jb holds A - jb numbers, at lr_ade_row)
// lr_ade_prepare_tables (lr_ade.hip, with its two kernels) writes all of it for any A <= LR_ADE_MAX_BINS.
#pragma once
#include "../../include/literate_hip_ade.h"
#include "lr_internal.h"

#define LR_ADE_HDR_CLASSES 0
#define LR_ADE_HDR_DEATHS 1
#define LR_ADE_HDR_FITS32 2      /* every class count and every number at risk is below 2^31 */

// what a kernel reads of the tables
struct lr_ade_data {
    const long long* hdr;
    const int* death_bin;
    const int* cls_cell;      // je | a << 16
    const double* cls_n;
    const int* cls_n32;
    const double* R;          // packed triangle
    const int* R32;
};

struct lr_ade_ws {
    size_t hdr, death_bin, cls_cell, cls_n, cls_n32, R, R32, total;
};

static inline lr_ade_ws lr_ade_layout(int A) {
    lr_ade_ws w;
    const long long tri = (long long)A * (A + 1) / 2;
    size_t o = 0;
    w.hdr = o, o += 256;
    w.death_bin = o, o += lr_align_up64((long long)A * sizeof(int), 256);
    w.cls_cell = o, o += lr_align_up64(tri * sizeof(int), 256);
    w.cls_n = o, o += lr_align_up64(tri * sizeof(double), 256);
    w.cls_n32 = o, o += lr_align_up64(tri * sizeof(int), 256);
    w.R = o, o += lr_align_up64(tri * sizeof(double), 256);
    w.R32 = o, o += lr_align_up64(tri * sizeof(int), 256);
    w.total = o;
    return w;
}

static inline lr_ade_data lr_ade_view(const void* tables, int A) {
    const lr_ade_ws w = lr_ade_layout(A);
    const char* base = (const char*)tables;
    lr_ade_data d;
    d.hdr = (const long long*)(base + w.hdr);
    d.death_bin = (const int*)(base + w.death_bin);
    d.cls_cell = (const int*)(base + w.cls_cell);
    d.cls_n = (const double*)(base + w.cls_n);
    d.cls_n32 = (const int*)(base + w.cls_n32);
    d.R = (const double*)(base + w.R);
    d.R32 = (const int*)(base + w.R32);
    return d;
}

// enqueue the two kernels that write the tables of (dead, cens) into the lr_ade_layout(A).total bytes at `tables`; the caller
// has checked the arguments.  -> 0 or a hipError_t
int lr_ade_prepare_tables(const int64_t* dead, const int64_t* cens, int A, void* tables, hipStream_t stream);

// where row jb of the packed triangle starts
__host__ __device__ __forceinline__ int lr_ade_row(int jb, int A) { return jb * A - (jb * (jb - 1)) / 2; }

// the number of classes, kept inside the list's room whatever the tables hold
__device__ __forceinline__ int lr_ade_class_count(const lr_ade_data& d, int A) {
    const long long n = d.hdr[LR_ADE_HDR_CLASSES];
    return (int)(n < 0 ? 0 : (n > (long long)A * (A + 1) / 2 ? (long long)A * (A + 1) / 2 : n));
}

// a rate no likelihood takes: not finite, negative, or zero in a bin that holds an observed death
__device__ __forceinline__ bool lr_ade_bad_rate(double m, const int* death_bin, int b) {
    return !(m >= 0.0) || !(m < __builtin_inf()) || (m == 0.0 && death_bin[b]);
}

// n log(1 - exp(-x)): accurate from the smallest x to the largest
__device__ __forceinline__ double lr_ade_term(double n, double x) {
    return n * (x < 0.6931471805599453 ? log(-expm1(-x)) : log1p(-exp(-x)));
}
