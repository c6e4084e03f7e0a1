// What the record reductions share around their per-cell arithmetic: a read-only sweep leaves one record per workgroup, a
// fixed tree of levels reduces the records to one, and that one goes to the caller, asynchronously or through a host copy.
//
// The two Courant checks (dlesm_courant.hip; dlesm_flow_courant.hip, section 6.15) take all of it: the
// three kernel bodies, the driver (its launch plan: dlesm_tile_plan.h) and the pointer checks.  Each supplies a policy type P:
//   Args, Acc, Record, Counts        the kernel's operands, what a thread / wave / workgroup has seen, the caller's record, and
//                                    the packed counts of a lane's cells of one wave tile
//   identity(), merge(a, b)          Acc's "nothing seen yet" and its combine
//   wave_pairs(a)                    the extremes and their lowest indices over the wave
//   wave_reduce(a)                   ... and the counts as 64-bit sums
//   wave_counts(c), add_counts(a, c) the packed counts over the wave; unpacked into an Acc
//   to_record(a), from_record(r)     Acc <-> Record; in the scratch records "none yet" reads as in the Acc
//   finish(a)                        the last level's rewrite of "none" for the caller
//   tile_row(f, ld, x0, x1, j, c0, lane, acc, cn)   one wave tile of a row
//   direct_cell(f, ld, o, acc)       the cell at linear offset o into acc, counts and all, if it is wet
// The kernels themselves stay in the two files, under their own names and launch bounds, as one-line wrappers of the bodies.
//
// dlesm_field_stats (dlesm_stats.hip, section 5.5) keeps its own sweep and its multi-field level loop -- every field's level in
// one launch -- and takes the copy-back tail from here.
#ifndef DLESM_RECORD_REDUCE_H
#define DLESM_RECORD_REDUCE_H

#include <climits>

#include "dlesm_nemolite.h"
#include "dlesm_wave_reduce.h"

namespace dlesm {

namespace recred {

constexpr int TILE_CHUNKS = CHUNKS_EAST;      // chunks (2 columns) a wave owns; lane 63 only loads
constexpr int LEVEL_CHUNK = 1024;     // records per workgroup of a level
constexpr double BIGGEST = 1.7976931348623157e308;
constexpr long long NO_INDEX = LLONG_MAX;

__device__ __forceinline__ bool valid(double x) { return x >= 0.0 && x <= BIGGEST; }   // false for a NaN

// the waves of a workgroup through LDS, in wave order; thread 0 returns with the workgroup's value in `a`.  Every thread of
// the workgroup calls it.
template <class P>
__device__ __forceinline__ void block_reduce(typename P::Acc &a, typename P::Acc *wv)
{
    const int nw = blockDim.x >> 6;
    if ((threadIdx.x & 63) == 0) wv[threadIdx.x >> 6] = a;
    __syncthreads();
    if (threadIdx.x == 0)
        for (int k = 1; k < nw; k++) P::merge(a, wv[k]);
}

// The wave-tile sweep: 64 lanes x 2 columns x 1 row in 16-byte lanes, waves step by TILE_CHUNKS chunks.  (x0:x1, y0:y1) = the
// box (0-based); nxw tiles per row, tile 0 begins at chunk c_first; rec[blockIdx.x] = the workgroup's record.  No thread
// leaves before the reductions: the DPP butterflies and the barrier want every lane.
template <class P>
__device__ __forceinline__ void tile_body(const typename P::Args &a, int ld, int x0, int x1, int y0, int y1, int c_first,
                                          int nxw, typename P::Record *__restrict__ rec)
{
    __shared__ typename P::Acc wv[4];
    const int lane = threadIdx.x & 63;
    const long long w = (long long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    const int xw = (int)(w % nxw);
    const long long j = y0 + w / nxw;
    const int c0 = c_first + xw * TILE_CHUNKS;
    typename P::Acc acc = P::identity();
    typename P::Counts cn{};
    if (j <= y1 && c0 <= x1 / 2) P::tile_row(a, ld, x0, x1, (int)j, c0, lane, acc, cn);   // (else: an idle padding tile)
    P::wave_pairs(acc);
    P::add_counts(acc, P::wave_counts(cn));
    block_reduce<P>(acc, wv);
    if (threadIdx.x == 0) rec[blockIdx.x] = P::to_record(acc);
}

// One cell per thread: odd leading dimensions, unaligned bases, the HOOK key of the check.  A thread walks its column i by rows
// y0 + blockIdx.y, + gridDim.y, ...; *rec = the workgroup's record.  The kernel says which column and which record those are
// (x0 + blockIdx.x * blockDim.x + threadIdx.x; rec[blockIdx.y * gridDim.x + blockIdx.x]): the compiler resolves blockDim.x to
// the dispatch's workgroup size only while the x geometry is read in the kernel function itself (LAB_NOTES.md section 5.29).
template <class P>
__device__ __forceinline__ void direct_body(const typename P::Args &f, int ld, int i, int x1, int y0, int y1,
                                            typename P::Record *__restrict__ rec)
{
    __shared__ typename P::Acc wv[4];
    typename P::Acc acc = P::identity();
    if (i <= x1) {
        for (long long j = (long long)y0 + blockIdx.y; j <= y1; j += gridDim.y) {
            const size_t o = (size_t)j * ld + i;
            P::direct_cell(f, ld, o, acc);
        }
    }
    P::wave_reduce(acc);
    block_reduce<P>(acc, wv);
    if (threadIdx.x == 0) *rec = P::to_record(acc);
}

// One level: workgroup b combines src[b * LEVEL_CHUNK .. (b + 1) * LEVEL_CHUNK) into dst[b] (n = 0: the identity).  `last`:
// dst is the caller's record, in which "none" reads as P::finish leaves it.  No atomics; plain vector stores only.
template <class P>
__device__ __forceinline__ void level_body(const typename P::Record *__restrict__ src, long long n,
                                           typename P::Record *__restrict__ dst, int last)
{
    __shared__ typename P::Acc wv[4];
    const long long lo = (long long)blockIdx.x * LEVEL_CHUNK, hi = lo + LEVEL_CHUNK < n ? lo + LEVEL_CHUNK : n;
    typename P::Acc acc = P::identity();
    for (long long k = lo + threadIdx.x; k < hi; k += 256) P::merge(acc, P::from_record(src[k]));
    P::wave_reduce(acc);
    block_reduce<P>(acc, wv);
    if (threadIdx.x == 0) {
        if (last) P::finish(acc);
        dst[blockIdx.x] = P::to_record(acc);
    }
}

// ---- the host side

// the mask and the n double arrays of a check: non-null and aligned for their element
inline int check_arrays(const char *who, const int *tmask, const double *const *ins, const char *const *name, int n)
{
    DLESM_REQUIRE(tmask != nullptr, "%s: null tmask", who);
    DLESM_REQUIRE((uintptr_t)tmask % 4 == 0, "%s: tmask is not 4-byte aligned", who);
    for (int k = 0; k < n; k++) {
        DLESM_REQUIRE(ins[k] != nullptr, "%s: null %s", who, name[k]);
        DLESM_REQUIRE((uintptr_t)ins[k] % 8 == 0, "%s: %s is not 8-byte aligned", who, name[k]);
    }
    return DLESM_OK;
}
// the `bytes` at result_dev (nullptr: nothing to check) lie inside none of these arrays of ld x ny
inline int check_result_apart(const char *who, const void *result_dev, size_t bytes, int ld, int ny, const int *tmask,
                              const double *const *ins, const char *const *name, int n)
{
    if (!result_dev) return DLESM_OK;
    const size_t nb = (size_t)ld * (size_t)ny * sizeof(double);
    DLESM_REQUIRE(!overlap(result_dev, bytes, tmask, nb / 2), "%s: result_dev lies inside tmask", who);
    for (int k = 0; k < n; k++)
        DLESM_REQUIRE(!overlap(result_dev, bytes, ins[k], nb), "%s: result_dev lies inside %s", who, name[k]);
    return DLESM_OK;
}

// The tail of a record reduction, behind its last launch: n records from result_dev back through a copy on `s` that the host
// waits for (result_host != nullptr; at most N of them), the scratch given back on every path, then the errors in the order
// launch / copy, free, synchronise.  result_host is written only when all of it went well.
template <class R, int N>
int copy_back(R *scratch, const R *result_dev, R *result_host, int n, hipStream_t s)
{
    hipError_t err = hipGetLastError();
    R host[N];
    if (result_host && err == hipSuccess)
        err = hipMemcpyAsync(host, result_dev, (size_t)n * sizeof(R), hipMemcpyDeviceToHost, s);
    DLESM_HIP_TRY(hipFreeAsync(scratch, s));
    DLESM_HIP_TRY(err);
    if (result_host) {
        DLESM_HIP_TRY(hipStreamSynchronize(s));
        for (int k = 0; k < n; k++) result_host[k] = host[k];
    }
    return DLESM_OK;
}

// the three kernels of a check
template <class P>
struct Kernels {
    void (*tile)(const typename P::Args, int, int, int, int, int, int, int, typename P::Record *);
    void (*direct)(const typename P::Args, int, int, int, int, int, typename P::Record *);
    void (*level)(const typename P::Record *, long long, typename P::Record *, int);
};

// Both forms of a check, behind its refusals.  The box is (x0:x1, y0:y1), 0-based, `empty` when it holds no cell; `tile`: the
// wave-tile kernel.  result_host == nullptr: the asynchronous form, *result_dev written when `s` gets there; otherwise the
// record lands behind the scratch records and comes back through copy_back.
template <class P>
int run(const char *who, const Kernels<P> &k, const typename P::Args &a, int ld, int x0, int x1, int y0, int y1, bool empty,
        bool tile, typename P::Record *result_dev, typename P::Record *result_host, hipStream_t s)
{
    using Record = typename P::Record;
    // the sweep's launch shape = its number of records; an empty box: no record
    TilePlan p{};
    DirectGrid g{};
    if (!empty && !tile) g = direct_grid(x0, x1, y0, y1);
    if (!empty && tile)
        if (int rc = tile_plan(who, ld, x0, x1, y0, y1, TILE_CHUNKS, 1, SHAPE_FOUR, 4, &p)) return rc;   // __launch_bounds__(256)
    unsigned nrec;
    if (int rc = sweep_grid(who, tile ? p.grid : (long long)g.x * g.y, &nrec)) return rc;
    const long long above = tree_records(nrec, LEVEL_CHUNK);

    Record *scratch = nullptr;
    DLESM_HIP_TRY(scratch_alloc_async((void **)&scratch, (size_t)(nrec + above + 1) * sizeof(Record), s));
    if (!result_dev) result_dev = scratch + nrec + above;
    if (nrec > 0) {
        if (tile)
            hipLaunchKernelGGL(k.tile, dim3(nrec), dim3(64 * p.tpb), 0, s, a, ld, x0, x1, y0, y1, p.c_first, p.nxw, scratch);
        else
            hipLaunchKernelGGL(k.direct, dim3(g.x, g.y), dim3(256), 0, s, a, ld, x0, x1, y0, y1, scratch);
    }
    // levels of LEVEL_CHUNK until one record is left, that one into *result_dev
    const Record *src = scratch;
    Record *next = scratch + nrec;
    for (long long n = nrec;;) {
        const long long groups = n > LEVEL_CHUNK ? (n + LEVEL_CHUNK - 1) / LEVEL_CHUNK : 1;
        const bool last = groups == 1;
        hipLaunchKernelGGL(k.level, dim3((unsigned)groups), dim3(256), 0, s, src, n, last ? result_dev : next, last ? 1 : 0);
        if (last) break;
        src = next, next += groups, n = groups;
    }
    return copy_back<Record, 1>(scratch, result_dev, result_host, 1, s);
}

} // namespace recred

} // namespace dlesm

#endif
