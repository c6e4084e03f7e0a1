/* libdlesm_lab.so -- measurement tooling that is loaded NEXT TO libdlesm_hip.so, never instead of it and never by it
 * (dl_esm_inf_amd/csrc/lab/).  No reference counterpart: the reference has no device code to hold a kernel against.
 * Shares no state with the product library: raw device pointers and a HIP stream in, 0 / -1 out. */
#ifndef DLESM_LAB_H
#define DLESM_LAB_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

/* text of the last failure of this thread */
const char *dlesm_lab_last_error(void);

/* The measured ceiling of a sweep with `nread` read and `nwrite` written arrays of n doubles each (n even; 16-byte aligned
 * bases): one 16-byte element per thread per array, workgroups front to back, nothing else.  Supported (nread + nwrite):
 * 1+1, 2+1, 3+1, 4+1, 6+3, 6+6 (dst[3..5] may be src[3..5]: the in-place pattern of the filtered step), 8+1.
 * nt bit 0: the second half of the read arrays loaded non-temporally; bit 1: non-temporal stores.
 * bench.py times it on the kernels' own arrays (`copy_ceiling`, `roofline.frac_of_copy_ceiling`). */
int dlesm_lab_stream_copy_f64(int nread, int nwrite, const double *const *src, double *const *dst, size_t n, int nt,
                              void *stream);

/* A competing load for the hand-over tests (tests/handover_load.py): `groups` workgroups of 256 threads, each read-modify-
 * writes its own slice of `slice` doubles of buf (n doubles; groups * slice <= n) `iters` times (1 .. 2^20) with plain
 * vector loads and stores.  Fixed trip counts, no flags, no waits between workgroups.  one_per_cu != 0: every workgroup
 * claims 96 KiB of LDS, so a CU holds one of them at a time. */
int dlesm_lab_load_rmw_f64(double *buf, size_t n, int groups, size_t slice, int iters, int one_per_cu, void *stream);

/* how many workgroups of that kernel one CU holds at a time (the runtime's occupancy figure): 1 with one_per_cu != 0 */
int dlesm_lab_load_rmw_occupancy(int one_per_cu, int *workgroups_per_cu);

#ifdef __cplusplus
}
#endif
#endif
