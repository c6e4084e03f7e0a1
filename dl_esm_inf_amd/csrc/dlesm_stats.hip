// What a time loop asks about its fields every few steps (NEMO's stp_ctl is the familiar example): minimum, maximum,
// SUM x, SUM x*x, the number of counted cells and how many of them are NaN or infinite -- of up to eight fields of one
// array shape, each over its own box and under its own optional land/sea mask (counted where mask > 0, the tmask
// convention of dlesm_stencil5_masked_f64), in ONE sweep launch that reads every cell once.
//
// The sweep is the row-segment form of the checksum (dlesm_device.h): one workgroup = one segment of one row of one
// field, four 16-byte non-temporal loads in flight per lane (and the four 8-byte mask loads), one 48-byte record per
// workgroup; a fixed tree of levels of 4096 then reduces each field's records into result_dev[k].  The split of a field
// into workgroups depends on (ld, box, base alignment) alone and every field has its own records and its own tree, so
// the bits of a field's sums do not depend on what else is in the call.  No floating-point atomics anywhere.
//
// The wave reductions are dlesm_wave_reduce.h's -- their fixed order is part of what makes a field's sums reproducible -- and
// the copy-back tail is dlesm_record_reduce.h's, both shared with the two Courant checks; the multi-field level loop, which
// puts every field's level into one launch, is this file's own.
#include <climits>

#include "dlesm_device.h"
#include "dlesm_record_reduce.h"

namespace dlesm {

namespace {

typedef double d2u __attribute__((ext_vector_type(2)));
typedef int i2u __attribute__((ext_vector_type(2), aligned(4)));   // a mask row starts on any int

using namespace wavered;

constexpr int SCALAR_SEG = 2048;      // elements per workgroup of the 8-byte form (eight per thread)
constexpr int TREE_CHUNK = 4096;      // records per workgroup of a tree level

struct SweepField {
    const double *f;
    const int *mask;                  // nullptr: every cell of the box counts
    long blk0;                        // first workgroup (= first record) of this field
    int x0, y0, nx, segs, segp;       // 0-based box corner, columns, segments per row; segp = 0: the 8-byte form
};
struct SweepJob {
    SweepField fd[DLESM_STATS_MAX_FIELDS];
    int n, ld;
    dlesm_field_stats *rec;           // one record per workgroup
};
struct TreeField {
    const dlesm_field_stats *src;
    dlesm_field_stats *dst;
    long n;
    int nb;                           // workgroups of this level; 0: the field is done
};
struct TreeJob { TreeField t[DLESM_STATS_MAX_FIELDS]; };

// what one thread, one wave or one workgroup has seen; cn = counted cells + (non-finite ones << 16), both <= 2048
struct Acc {
    double mn, mx, s, q;
    int cn;
};

__device__ __forceinline__ void acc_cell(Acc &a, double x, bool counted)
{
    const bool fin = counted && fabs(x) <= 1.7976931348623157e308;   // false for a NaN
    const double v = fin ? x : 0.0;
    a.s += v;
    a.q += v * v;
    a.mn = (fin && x < a.mn) ? x : a.mn;
    a.mx = (fin && x > a.mx) ? x : a.mx;
    a.cn += (int)counted + ((int)(counted && !fin) << 16);
}

// the segment's cells, 16-byte lanes: the pairs of rowseg_pair, all loads of a lane issued before the first use.  A
// pair that is not wholly inside the box may end outside the array: it reads the row's first whole pair instead (the box
// is at least ROWSEG_MIN_NX wide) and takes its one cell from a scalar load -- only the two ends of a row have such pairs.
template <bool MASK>
__device__ __forceinline__ void sweep_pairs(const SweepField &fd, int ld, int jr, int sg, Acc &a)
{
    const double *__restrict__ f = fd.f;
    const int *__restrict__ mask = fd.mask;
    const long row = (long)(fd.y0 + jr) * ld, e0 = row + fd.x0, e1 = e0 + fd.nx - 1;
    const long safe = (e0 + 1) & ~1L;
    RowPair pr[4];
    d2u v[4];
    i2u m[4];
#pragma unroll
    for (int k = 0; k < 4; k++) {
        pr[k] = rowseg_pair(e0, e1, sg, fd.segp, threadIdx.x, k);
        const long at = pr[k].full() ? pr[k].el : safe;
        v[k] = __builtin_nontemporal_load((const d2u *)(f + at));
        if constexpr (MASK) m[k] = __builtin_nontemporal_load((const i2u *)(mask + at));
        else m[k] = i2u{1, 1};
    }
#pragma unroll
    for (int k = 0; k < 4; k++) {
        if (pr[k].any() && !pr[k].full()) {
            const long e = pr[k].m0 ? pr[k].el : pr[k].el + 1;
            const double x = f[e];
            int mk = 1;
            if constexpr (MASK) mk = mask[e];
            if (pr[k].m0) v[k].x = x, m[k].x = mk;
            else v[k].y = x, m[k].y = mk;
        }
        acc_cell(a, v[k].x, pr[k].m0 && m[k].x > 0);
        acc_cell(a, v[k].y, pr[k].m1 && m[k].y > 0);
    }
}

// the same with 8-byte lanes (a base 8 bytes off 16, boxes narrower than ROWSEG_MIN_NX): cells tid, tid + 256, ...
template <bool MASK>
__device__ __forceinline__ void sweep_cells(const SweepField &fd, int ld, int jr, int sg, Acc &a)
{
    const double *__restrict__ f = fd.f;
    const int *__restrict__ mask = fd.mask;
    const long e0 = (long)(fd.y0 + jr) * ld + fd.x0, e1 = e0 + fd.nx - 1;
    const long first = e0 + (long)sg * SCALAR_SEG + threadIdx.x;
    double v[8];
    int m[8];
#pragma unroll
    for (int k = 0; k < 8; k++) {
        const long e = first + 256 * k;
        const long at = e <= e1 ? e : e0;
        v[k] = __builtin_nontemporal_load(f + at);
        if constexpr (MASK) m[k] = __builtin_nontemporal_load(mask + at);
        else m[k] = 1;
    }
#pragma unroll
    for (int k = 0; k < 8; k++) acc_cell(a, v[k], first + 256 * k <= e1 && m[k] > 0);
}

// One workgroup = one row segment of one field; its record goes to rec[blockIdx.x].  Per lane the cells in index order,
// then the lanes by the wave reduction (dlesm_wave_reduce.h), then the four waves as (0 . 1) . (2 . 3).
__global__ __launch_bounds__(256) void field_stats_sweep(const SweepJob job)
{
    __shared__ Acc wv[4];
    int k = 0;
    for (int q = 1; q < job.n; q++)
        if ((long)blockIdx.x >= job.fd[q].blk0) k = q;     // (an empty field shares its blk0 with the next one: skipped)
    const SweepField fd = job.fd[k];
    const int b = (int)((long)blockIdx.x - fd.blk0);
    const int jr = b / fd.segs, sg = b - jr * fd.segs;
    Acc a{__builtin_inf(), -__builtin_inf(), 0.0, 0.0, 0};
    if (fd.segp) {
        if (fd.mask) sweep_pairs<true>(fd, job.ld, jr, sg, a);
        else sweep_pairs<false>(fd, job.ld, jr, sg, a);
    } else {
        if (fd.mask) sweep_cells<true>(fd, job.ld, jr, sg, a);
        else sweep_cells<false>(fd, job.ld, jr, sg, a);
    }
    a.mn = wave_f64<OP_MIN>(a.mn);
    a.mx = wave_f64<OP_MAX>(a.mx);
    a.s = wave_f64<OP_ADD>(a.s);
    a.q = wave_f64<OP_ADD>(a.q);
    a.cn = wave_add_i32(a.cn);
    if ((threadIdx.x & 63) == 0) wv[threadIdx.x >> 6] = a;
    __syncthreads();
    if (threadIdx.x == 0) {
        dlesm_field_stats r;
        r.min = combine<OP_MIN>(combine<OP_MIN>(wv[0].mn, wv[1].mn), combine<OP_MIN>(wv[2].mn, wv[3].mn));
        r.max = combine<OP_MAX>(combine<OP_MAX>(wv[0].mx, wv[1].mx), combine<OP_MAX>(wv[2].mx, wv[3].mx));
        r.sum = (wv[0].s + wv[1].s) + (wv[2].s + wv[3].s);
        r.sumsq = (wv[0].q + wv[1].q) + (wv[2].q + wv[3].q);
        const int cn = (wv[0].cn + wv[1].cn) + (wv[2].cn + wv[3].cn);
        r.count = cn & 0xffff;
        r.nonfinite = cn >> 16;
        job.rec[blockIdx.x] = r;
    }
}

// One level of the tree, all fields in one launch (blockIdx.y = field): workgroup b of a field combines its records
// src[b*4096 .. (b+1)*4096) -- per lane in index order, then lanes and waves as in the sweep -- into dst[b].  A field
// with no record at all (an empty box) gets the empty result.
__global__ __launch_bounds__(256) void field_stats_level(const TreeJob job)
{
    __shared__ dlesm_field_stats wv[4];
    const TreeField t = job.t[blockIdx.y];
    if ((int)blockIdx.x >= t.nb) return;
    const long lo = (long)blockIdx.x * TREE_CHUNK, hi = lo + TREE_CHUNK < t.n ? lo + TREE_CHUNK : t.n;
    dlesm_field_stats a{__builtin_inf(), -__builtin_inf(), 0.0, 0.0, 0, 0};
    for (long i = lo + threadIdx.x; i < hi; i += 256) {
        const dlesm_field_stats r = t.src[i];
        a.min = combine<OP_MIN>(a.min, r.min);
        a.max = combine<OP_MAX>(a.max, r.max);
        a.sum += r.sum;
        a.sumsq += r.sumsq;
        a.count += r.count;
        a.nonfinite += r.nonfinite;
    }
    a.min = wave_f64<OP_MIN>(a.min);
    a.max = wave_f64<OP_MAX>(a.max);
    a.sum = wave_f64<OP_ADD>(a.sum);
    a.sumsq = wave_f64<OP_ADD>(a.sumsq);
    a.count = wave_i64<OP_ADD>(a.count);
    a.nonfinite = wave_i64<OP_ADD>(a.nonfinite);
    if ((threadIdx.x & 63) == 0) wv[threadIdx.x >> 6] = a;
    __syncthreads();
    if (threadIdx.x == 0) {
        dlesm_field_stats r;
        r.min = combine<OP_MIN>(combine<OP_MIN>(wv[0].min, wv[1].min), combine<OP_MIN>(wv[2].min, wv[3].min));
        r.max = combine<OP_MAX>(combine<OP_MAX>(wv[0].max, wv[1].max), combine<OP_MAX>(wv[2].max, wv[3].max));
        r.sum = (wv[0].sum + wv[1].sum) + (wv[2].sum + wv[3].sum);
        r.sumsq = (wv[0].sumsq + wv[1].sumsq) + (wv[2].sumsq + wv[3].sumsq);
        r.count = (wv[0].count + wv[1].count) + (wv[2].count + wv[3].count);
        r.nonfinite = (wv[0].nonfinite + wv[1].nonfinite) + (wv[2].nonfinite + wv[3].nonfinite);
        t.dst[blockIdx.x] = r;
    }
}

// the rare path: the lowest linear index of a counted cell that is not finite / that equals `value`, by an integer
// atomic minimum on one device word (one per thread that found something)
__global__ __launch_bounds__(256) void field_locate_k(const double *__restrict__ f, const int *__restrict__ mask, int ld, int x0,
                                                      int y0, int nx, int nyb, int what, double value,
                                                      unsigned long long *__restrict__ best)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= nx) return;
    unsigned long long mine = ~0ULL;
    for (int j = blockIdx.y; j < nyb; j += gridDim.y) {
        const size_t e = (size_t)(y0 + j) * ld + x0 + i;
        if (mask && mask[e] <= 0) continue;
        const double x = f[e];
        const bool hit = what == DLESM_LOCATE_NONFINITE ? !(fabs(x) <= 1.7976931348623157e308) : x == value;
        if (hit && e < mine) mine = e;
    }
    if (mine != ~0ULL) atomicMin(best, mine);
}

} // namespace

} // namespace dlesm

using namespace dlesm;

// Both forms of the entry.  result_host == nullptr: the asynchronous one, result_dev[k] written when `s` gets there;
// otherwise the results land behind the scratch records and come back by a copy on `s` that the host waits for.
static int field_stats_run(const char *who, const double *const *fields, const int *const *masks, const dlesm_region *boxes,
                           int nfields, int ld, int ny, dlesm_field_stats *result_dev, dlesm_field_stats *result_host,
                           hipStream_t s)
{
    static_assert(sizeof(dlesm_field_stats) == 48, "dlesm_field_stats has padding");
    if (int rc = ensure_device()) return rc;
    DLESM_REQUIRE(nfields >= 1 && nfields <= DLESM_STATS_MAX_FIELDS, "%s: %d fields (1 to %d)", who, nfields,
                  DLESM_STATS_MAX_FIELDS);
    DLESM_REQUIRE(fields != nullptr && boxes != nullptr && (result_dev != nullptr || result_host != nullptr),
                  "%s: null pointer", who);
    DLESM_REQUIRE(ld >= 1 && ny >= 1, "%s: array extents %dx%d", who, ld, ny);
    DLESM_REQUIRE(!capturing(s), "%s: not callable under stream capture", who);
    const size_t bytes = (size_t)ld * (size_t)ny * sizeof(double);
    const char *r0 = (const char *)result_dev, *r1 = r0 + (size_t)nfields * sizeof(dlesm_field_stats);
    SweepJob job{};
    long nrec[DLESM_STATS_MAX_FIELDS], total = 0, above = 0;
    for (int k = 0; k < nfields; k++) {
        const double *f = fields[k];
        const dlesm_region &b = boxes[k];
        DLESM_REQUIRE(f != nullptr, "%s: field %d is null", who, k);
        DLESM_REQUIRE((uintptr_t)f % 8 == 0, "%s: field %d is not 8-byte aligned", who, k);
        DLESM_REQUIRE(!result_dev || !(r1 > (const char *)f && r0 < (const char *)f + bytes),
                      "%s: result_dev lies inside field %d", who, k);
        const bool empty = b.xstop < b.xstart || b.ystop < b.ystart;
        if (!empty)
            if (int rc = check_box(who, ld, ny, b.xstart, b.xstop, b.ystart, b.ystop, 0)) return rc;
        SweepField &fd = job.fd[k];
        fd.f = f;
        fd.mask = masks ? masks[k] : nullptr;
        DLESM_REQUIRE((uintptr_t)fd.mask % 4 == 0, "%s: mask %d is not 4-byte aligned", who, k);
        fd.blk0 = total;
        fd.x0 = b.xstart - 1, fd.y0 = b.ystart - 1;
        fd.nx = empty ? 0 : b.xstop - b.xstart + 1;
        fd.segs = 1, fd.segp = 0;
        if (!empty) {
            if ((uintptr_t)f % 16 == 0 && fd.nx >= ROWSEG_MIN_NX) rowseg_split(fd.nx, SEG_PAIRS, &fd.segs, &fd.segp);
            else fd.segs = (fd.nx + SCALAR_SEG - 1) / SCALAR_SEG;
        }
        nrec[k] = empty ? 0 : (long)fd.segs * (b.ystop - b.ystart + 1);
        total += nrec[k];
        above += tree_records(nrec[k], TREE_CHUNK);
    }
    DLESM_REQUIRE(total <= INT_MAX, "%s: %ld row segments in one call (at most %d)", who, total, INT_MAX);
    job.n = nfields, job.ld = ld;

    dlesm_field_stats *scratch = nullptr;
    DLESM_HIP_TRY(scratch_alloc_async((void **)&scratch, (size_t)(total + above + nfields) * sizeof(dlesm_field_stats), s));
    if (!result_dev) result_dev = scratch + total + above;
    job.rec = scratch;
    if (total > 0) hipLaunchKernelGGL(field_stats_sweep, dim3((unsigned)total), dim3(256), 0, s, job);
    // each field's own tree: levels of 4096 until one record is left, that one into result_dev[k]
    TreeJob tj{};
    dlesm_field_stats *next = scratch + total;
    for (int k = 0; k < nfields; k++) tj.t[k] = TreeField{scratch + job.fd[k].blk0, nullptr, nrec[k], 0};
    for (bool more = true; more;) {
        more = false;
        int nbmax = 0;
        for (int k = 0; k < nfields; k++) {
            TreeField &t = tj.t[k];
            if (!t.src) { t.nb = 0; continue; }
            t.nb = t.n > TREE_CHUNK ? (int)((t.n + TREE_CHUNK - 1) / TREE_CHUNK) : 1;
            t.dst = t.nb == 1 ? result_dev + k : next;
            if (t.nb > 1) next += t.nb;
            if (t.nb > nbmax) nbmax = t.nb;
        }
        hipLaunchKernelGGL(field_stats_level, dim3((unsigned)nbmax, (unsigned)nfields), dim3(256), 0, s, tj);
        for (int k = 0; k < nfields; k++) {
            TreeField &t = tj.t[k];
            if (!t.src) continue;
            if (t.nb == 1) t.src = nullptr;
            else t.src = t.dst, t.n = t.nb, more = true;
        }
    }
    return recred::copy_back<dlesm_field_stats, DLESM_STATS_MAX_FIELDS>(scratch, result_dev, result_host, nfields, s);
}

extern "C" int dlesm_field_stats_async_f64(const double *const *fields, const int *const *masks, const dlesm_region *boxes,
                                           int nfields, int ld, int ny, dlesm_field_stats *result_dev, void *stream)
{
    DLESM_REQUIRE(result_dev != nullptr, "dlesm_field_stats_async_f64: null result_dev");
    return field_stats_run("dlesm_field_stats_async_f64", fields, masks, boxes, nfields, ld, ny, result_dev, nullptr,
                           (hipStream_t)stream);
}

extern "C" int dlesm_field_stats_f64(const double *const *fields, const int *const *masks, const dlesm_region *boxes,
                                     int nfields, int ld, int ny, dlesm_field_stats *result_host, void *stream)
{
    DLESM_REQUIRE(result_host != nullptr, "dlesm_field_stats_f64: null result");
    return field_stats_run("dlesm_field_stats_f64", fields, masks, boxes, nfields, ld, ny, nullptr, result_host,
                           (hipStream_t)stream);
}

extern "C" int dlesm_field_locate_f64(const double *f, const int *mask, int ld, int ny, int xstart, int xstop, int ystart,
                                      int ystop, int what, double value, int64_t *index_host, void *stream)
{
    if (int rc = ensure_device()) return rc;
    DLESM_REQUIRE(f != nullptr && index_host != nullptr, "dlesm_field_locate_f64: null pointer");
    DLESM_REQUIRE(what == DLESM_LOCATE_NONFINITE || what == DLESM_LOCATE_EQUAL, "dlesm_field_locate_f64: unknown search %d", what);
    hipStream_t s = (hipStream_t)stream;
    DLESM_REQUIRE(!capturing(s), "dlesm_field_locate_f64: not callable under stream capture");
    if (xstop < xstart || ystop < ystart) {
        *index_host = -1;
        return DLESM_OK;
    }
    if (int rc = check_box("dlesm_field_locate_f64", ld, ny, xstart, xstop, ystart, ystop, 0)) return rc;
    const int nx = xstop - xstart + 1, nyb = ystop - ystart + 1;
    unsigned long long *best = nullptr, got = 0;
    DLESM_HIP_TRY(scratch_alloc_async((void **)&best, sizeof *best, s));
    hipError_t err = hipMemsetAsync(best, 0xff, sizeof *best, s);
    if (err == hipSuccess) {
        hipLaunchKernelGGL(field_locate_k, dim3((unsigned)((nx + 255) / 256), (unsigned)(nyb < 4096 ? nyb : 4096)), dim3(256), 0, s,
                           f, mask, ld, xstart - 1, ystart - 1, nx, nyb, what, value, best);
        err = hipGetLastError();
    }
    if (err == hipSuccess) err = hipMemcpyAsync(&got, best, sizeof got, hipMemcpyDeviceToHost, s);
    const hipError_t ferr = hipFreeAsync(best, s);
    DLESM_HIP_TRY(err);
    DLESM_HIP_TRY(ferr);
    DLESM_HIP_TRY(hipStreamSynchronize(s));
    *index_host = got == ~0ULL ? -1 : (int64_t)got;
    return DLESM_OK;
}
