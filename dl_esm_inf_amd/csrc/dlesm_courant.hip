// The tracer schemes' Courant check: one read-only sweep over the level-n flow that evaluates, in
// every wet T cell of a box, the four face Courant numbers n1..n4 exactly as the Hancock step does (tracer_flow /
// tracer_weight / tracer_numbers, dlesm_nemolite.h) and the cell's outflow number o, and reduces them to one 64-byte record:
// the two maxima, the lowest linear index that attains each, how many cells reach the caller's two limits, how many hold a
// number that is not a finite non-negative one, and how many are wet.  Maxima, integers and lowest indices: every member is
// exact and independent of the order of the reduction, so the record does not depend on the kernel form or the launch shape.
//
// This file holds the check's own part: the per-cell rule, the record, the loads of the two sweep forms and the entry's
// refusals (the policy TracerCheck).  The kernel bodies around them, the launch shape, the levels and the copy-back are
// dlesm_record_reduce.h's, shared with dlesm_flow_courant.hip; the wave reductions are dlesm_wave_reduce.h's.
//
// courant_tile: tracer_tile's wave shape (dlesm_tracer.hip) -- 64 lanes x 2 columns x 1 row in 16-byte lanes, operands at
// i-1 / i+1 (the u-face operands, the mask and w) from the neighbouring lane by a DPP wave shift, lane 0 fetches the column
// west of the wave without a branch, lane 63 only loads, waves step by 63 chunks.  w of rows j-1 and j+1 comes from six more
// row pairs a lane, asked for first, as in the Hancock tile.  A wave that owns no wet cell of the box leaves after its mask
// row and contributes the identity.  Within the wave the reduction runs on the VALU, across the waves of a workgroup through
// LDS: one record per workgroup.
//
// courant_direct: one cell per thread -- odd leading dimensions, unaligned bases and the HOOK key tracer_courant_kernel = 1.
//
// courant_level: workgroup b combines records [b * 1024, (b + 1) * 1024) into one; launched until one record is left, and
// that launch writes the caller's record (the empty maxima as 0.0 / -1).  No atomics; plain vector stores only.
#include "dlesm_record_reduce.h"

namespace dlesm {

namespace {

typedef double d2 __attribute__((ext_vector_type(2)));
typedef int i2 __attribute__((ext_vector_type(2)));

using namespace nemo;
using namespace wavered;
using namespace recred;

struct CourantArgs {
    const int *tmask;
    const double *area_t, *un, *vn, *hu, *hv, *ht, *sshn_t, *sshn_u, *sshn_v;
    double rdt, face_limit, outflow_limit;
};

struct TracerCheck {
    using Args = CourantArgs;
    using Record = dlesm_tracer_courant;
    // the four counts of a cell or a wave tile, a byte each: wet | bad << 8 | (m >= face_limit) << 16 |
    // (o >= outflow_limit) << 24 (two cells a lane, 126 a wave: a byte holds each sum, so the four share one 32-bit reduction)
    using Counts = int;

    // what one thread, one wave or one workgroup has seen.  A maximum of -1.0 (with NO_INDEX) stands for "none yet": every
    // value that competes is >= 0.  In the scratch records the same convention holds; only the last level writes 0.0 / -1.
    struct Acc {
        double fm, om;
        long long fi, oi;
        long long over_f, over_o, bad, wet;
    };
    static __device__ __forceinline__ Acc identity() { return Acc{-1.0, -1.0, NO_INDEX, NO_INDEX, 0, 0, 0, 0}; }

    // one wet cell of the box (section 6.14); ix = its 0-based linear index.  The maxima go into a; what the cell adds to the
    // four counts comes back
    static __device__ __forceinline__ int acc_cell(Acc &a, bool wet, long long ix, const TracerFlow &f, const TracerNumbers &n,
                                                   double w, double face_limit, double outflow_limit)
    {
        double m = -1.0;
        m = (f.e && valid(n.n1) && n.n1 > m) ? n.n1 : m;
        m = (f.w && valid(n.n2) && n.n2 > m) ? n.n2 : m;
        m = (f.n && valid(n.n3) && n.n3 > m) ? n.n3 : m;
        m = (f.s && valid(n.n4) && n.n4 > m) ? n.n4 : m;
        const double o1 = (f.e && f.r1 > 0.0) ? f.r1 : 0.0, o2 = (f.w && f.r2 < 0.0) ? -f.r2 : 0.0;
        const double o3 = (f.n && f.r3 > 0.0) ? f.r3 : 0.0, o4 = (f.s && f.r4 < 0.0) ? -f.r4 : 0.0;
        const double o = (((o1 + o2) + o3) + o4) * w;
        const bool bad = !(w > 0.0 && w <= BIGGEST) || (f.e && !valid(n.n1)) || (f.w && !valid(n.n2)) ||
                         (f.n && !valid(n.n3)) || (f.s && !valid(n.n4)) || !valid(o);
        const bool has_m = wet && m >= 0.0, has_o = wet && valid(o);
        if (has_m) take(a.fm, a.fi, m, ix);
        if (has_o) take(a.om, a.oi, o, ix);
        return (int)wet | ((int)(wet && bad) << 8) | ((int)(has_m && m >= face_limit) << 16) |
               ((int)(has_o && o >= outflow_limit) << 24);
    }
    static __device__ __forceinline__ void add_counts(Acc &a, int c)
    {
        a.wet += c & 0xff, a.bad += (c >> 8) & 0xff, a.over_f += (c >> 16) & 0xff, a.over_o += (c >> 24) & 0xff;
    }
    static __device__ __forceinline__ int wave_counts(int c) { return wave_add_i32(c); }

    // the maxima and their lowest indices over the wave; every lane must be active
    static __device__ __forceinline__ void wave_pairs(Acc &a)
    {
        const double fm = wave_f64<OP_MAX>(a.fm), om = wave_f64<OP_MAX>(a.om);
        a.fi = wave_i64<OP_MIN>(a.fm == fm ? a.fi : NO_INDEX);
        a.oi = wave_i64<OP_MIN>(a.om == om ? a.oi : NO_INDEX);
        a.fm = fm, a.om = om;
    }
    // ... and the four counts as 64-bit sums (the one-cell-per-thread kernel, whose threads walk many rows, and the levels)
    static __device__ __forceinline__ void wave_reduce(Acc &a)
    {
        wave_pairs(a);
        a.wet = wave_i64<OP_ADD>(a.wet);
        a.bad = wave_i64<OP_ADD>(a.bad);
        a.over_f = wave_i64<OP_ADD>(a.over_f);
        a.over_o = wave_i64<OP_ADD>(a.over_o);
    }

    static __device__ __forceinline__ void merge(Acc &a, const Acc &b)
    {
        take(a.fm, a.fi, b.fm, b.fi);
        take(a.om, a.oi, b.om, b.oi);
        a.over_f += b.over_f, a.over_o += b.over_o, a.bad += b.bad, a.wet += b.wet;
    }

    static __device__ __forceinline__ Record to_record(const Acc &a)
    {
        return Record{a.fm, a.om, a.fi, a.oi, a.over_f, a.over_o, a.bad, a.wet};
    }
    static __device__ __forceinline__ Acc from_record(const Record &r)
    {
        return Acc{r.face_max, r.outflow_max, r.face_index, r.outflow_index, r.face_over, r.outflow_over, r.invalid, r.wet};
    }
    // the caller's record: "none" reads 0.0 / -1
    static __device__ __forceinline__ void finish(Acc &acc)
    {
        if (acc.fi == NO_INDEX) acc.fm = 0.0, acc.fi = -1;
        if (acc.oi == NO_INDEX) acc.om = 0.0, acc.oi = -1;
    }

    // one wave tile of row j (0-based); lane 0 of the tile holds chunk c0.  cn: the lane's counts
    static __device__ __forceinline__ void tile_row(const Args &f, int ld, int x0, int x1, int j, int c0, int lane, Acc &acc,
                                                    int &cn)
    {
        const int c = c0 + lane;                         // this lane's chunk (2 columns); lane 63 = the next wave's lane 0
        const int c_ld = ld / 2 - 1, cl = c < c_ld ? c : c_ld;
        const bool own = lane != 63;                     // lane 63 only loads: its chunk is the east column of lane 62
        const bool m0 = own && c * 2 >= x0 && c * 2 <= x1, m1 = own && c * 2 + 1 >= x0 && c * 2 + 1 <= x1;
        const size_t row = (size_t)j * ld, o = row + (size_t)cl * 2, os = o - ld, on = o + ld;

        // the land exit: the mask of the row first; a wave that owns no wet cell of the box contributes the identity
        const i2 t = *(const i2 *)(f.tmask + o);
        const bool wet0 = m0 && t.x > 0, wet1 = m1 && t.y > 0;
        if (__ballot(wet0 || wet1) == 0) return;

        // w of the lane's two columns on rows j-1 and j+1, asked for in front of everything else (the Hancock tile's order)
        const d2 ar_s = *(const d2 *)(f.area_t + os), ht_s = *(const d2 *)(f.ht + os), st_s = *(const d2 *)(f.sshn_t + os);
        const d2 ar_n = *(const d2 *)(f.area_t + on), ht_n = *(const d2 *)(f.ht + on), st_n = *(const d2 *)(f.sshn_t + on);
        const d2 ws = d2{tracer_weight(f.rdt, ar_s.x, ht_s.x, st_s.x), tracer_weight(f.rdt, ar_s.y, ht_s.y, st_s.y)};
        const d2 wn = d2{tracer_weight(f.rdt, ar_n.x, ht_n.x, st_n.x), tracer_weight(f.rdt, ar_n.y, ht_n.y, st_n.y)};

        // the west column this wave cannot get from a lane (no branch, LAB_NOTES.md section 5.10)
        const size_t ow = row + (size_t)((lane == 0 && m0) ? c * 2 - 1 : cl * 2);
        const i2 ts = *(const i2 *)(f.tmask + os), tn = *(const i2 *)(f.tmask + on);
        int tw = f.tmask[ow];
        const d2 su = *(const d2 *)(f.sshn_u + o), hu = *(const d2 *)(f.hu + o), un = *(const d2 *)(f.un + o);
        double su_w = f.sshn_u[ow], hu_w = f.hu[ow], un_w = f.un[ow];
        const d2 sv = *(const d2 *)(f.sshn_v + o), hv = *(const d2 *)(f.hv + o), vn = *(const d2 *)(f.vn + o);
        const d2 sv_s = *(const d2 *)(f.sshn_v + os), hv_s = *(const d2 *)(f.hv + os), vn_s = *(const d2 *)(f.vn + os);
        const d2 ht = *(const d2 *)(f.ht + o), st = *(const d2 *)(f.sshn_t + o), ar = *(const d2 *)(f.area_t + o);
        double w_w = tracer_weight(f.rdt, f.area_t[ow], f.ht[ow], f.sshn_t[ow]);

        const double w0 = tracer_weight(f.rdt, ar.x, ht.x, st.x), w1 = tracer_weight(f.rdt, ar.y, ht.y, st.y);
        {
            const double s1 = from_lower<true>(su.y), h1 = from_lower<true>(hu.y), u1 = from_lower<true>(un.y);
            const double wl = from_lower<true>(w1);
            const int t1 = __builtin_amdgcn_mov_dpp(t.y, 0x138, 0xf, 0xf, true);
            if (lane != 0) su_w = s1, hu_w = h1, un_w = u1, w_w = wl, tw = t1;
        }
        const int te = __builtin_amdgcn_mov_dpp(t.x, 0x130, 0xf, 0xf, true);      // (lane 63: 0, never used)
        const double w_e = from_upper<true>(w0);                                   // (the same)
        // tracer_flow's ssha operand only makes h_new, which nothing here reads: sshn_t stands in for it
        const TracerFlow f0 = tracer_flow(f.rdt, su.x, su_w, sv.x, sv_s.x, hu.x, hu_w, hv.x, hv_s.x, un.x, un_w, vn.x, vn_s.x,
                                          ar.x, ht.x, st.x, st.x, t.y, tw, tn.x, ts.x);
        const TracerFlow f1 = tracer_flow(f.rdt, su.y, su.x, sv.y, sv_s.y, hu.y, hu.x, hv.y, hv_s.y, un.y, un.x, vn.y, vn_s.y,
                                          ar.y, ht.y, st.y, st.y, te, t.x, tn.y, ts.y);
        const TracerNumbers n0 = tracer_numbers(f0, w0, w1, w_w, wn.x, ws.x);
        const TracerNumbers n1 = tracer_numbers(f1, w1, w_e, w0, wn.y, ws.y);
        const long long ix = (long long)row + (long long)c * 2;
        cn = acc_cell(acc, wet0, ix, f0, n0, w0, f.face_limit, f.outflow_limit) +
             acc_cell(acc, wet1, ix + 1, f1, n1, w1, f.face_limit, f.outflow_limit);
    }

    // the cell at linear offset o, one thread's
    static __device__ __forceinline__ void direct_cell(const Args &f, int ld, size_t o, Acc &acc)
    {
        if (f.tmask[o] <= 0) return;
        const TracerFlow fl = tracer_flow(f.rdt, f.sshn_u[o], f.sshn_u[o - 1], f.sshn_v[o], f.sshn_v[o - ld], f.hu[o],
                                          f.hu[o - 1], f.hv[o], f.hv[o - ld], f.un[o], f.un[o - 1], f.vn[o], f.vn[o - ld],
                                          f.area_t[o], f.ht[o], f.sshn_t[o], f.sshn_t[o], f.tmask[o + 1], f.tmask[o - 1],
                                          f.tmask[o + ld], f.tmask[o - ld]);
        auto W = [&](size_t p) { return tracer_weight(f.rdt, f.area_t[p], f.ht[p], f.sshn_t[p]); };
        const double w = W(o);
        const TracerNumbers n = tracer_numbers(fl, w, W(o + 1), W(o - 1), W(o + ld), W(o - ld));
        add_counts(acc, acc_cell(acc, true, (long long)o, fl, n, w, f.face_limit, f.outflow_limit));
    }
};

__global__ __launch_bounds__(256, 4) void courant_tile(const CourantArgs a, int ld, int x0, int x1, int y0, int y1, int c_first,
                                                    int nxw, dlesm_tracer_courant *__restrict__ rec)
{
    tile_body<TracerCheck>(a, ld, x0, x1, y0, y1, c_first, nxw, rec);
}
__global__ __launch_bounds__(256) void courant_direct(const CourantArgs f, int ld, int x0, int x1, int y0, int y1,
                                                      dlesm_tracer_courant *__restrict__ rec)
{
    direct_body<TracerCheck>(f, ld, x0 + blockIdx.x * blockDim.x + threadIdx.x, x1, y0, y1,
                             rec + ((size_t)blockIdx.y * gridDim.x + blockIdx.x));
}
__global__ __launch_bounds__(256) void courant_level(const dlesm_tracer_courant *__restrict__ src, long long n,
                                                     dlesm_tracer_courant *__restrict__ dst, int last)
{
    level_body<TracerCheck>(src, n, dst, last);
}

} // namespace

} // namespace dlesm

using namespace dlesm;

// Both forms of the entry (recred::run): the refusals, in their order, then the sweep
static int tracer_courant_run(const char *who, double rdt, int ld, int ny, int xstart, int xstop, int ystart, int ystop,
                              const int *tmask, const double *area_t, const double *un, const double *vn, const double *hu,
                              const double *hv, const double *ht, const double *sshn_t, const double *sshn_u,
                              const double *sshn_v, double face_limit, double outflow_limit,
                              dlesm_tracer_courant *result_dev, dlesm_tracer_courant *result_host, hipStream_t s)
{
    static_assert(sizeof(dlesm_tracer_courant) == 64, "dlesm_tracer_courant has padding");
    if (int rc = ensure_device()) return rc;
    const double *const ins[9] = {area_t, un, vn, hu, hv, ht, sshn_t, sshn_u, sshn_v};
    static const char *const in_name[9] = {"area_t", "un", "vn", "hu", "hv", "ht", "sshn_t", "sshn_u", "sshn_v"};
    DLESM_REQUIRE(result_dev != nullptr || result_host != nullptr, "%s: null result", who);
    if (int rc = check_arrays(who, tmask, ins, in_name, 9)) return rc;
    DLESM_REQUIRE(ld >= 1 && ny >= 1, "%s: array extents %dx%d", who, ld, ny);
    const bool empty = xstop < xstart || ystop < ystart;
    if (!empty)
        if (int rc = check_box(who, ld, ny, xstart, xstop, ystart, ystop, 1)) return rc;
    DLESM_REQUIRE(face_limit > 0.0, "%s: face_limit %g (a positive number)", who, face_limit);
    DLESM_REQUIRE(outflow_limit > 0.0, "%s: outflow_limit %g (a positive number)", who, outflow_limit);
    if (int rc = check_result_apart(who, result_dev, sizeof *result_dev, ld, ny, tmask, ins, in_name, 9)) return rc;
    DLESM_REQUIRE(!capturing(s), "%s: not callable under stream capture", who);

    const CourantArgs a{tmask, area_t, un, vn, hu, hv, ht, sshn_t, sshn_u, sshn_v, rdt, face_limit, outflow_limit};
    const bool tile = lanes16_fit(ld, tmask, ins, 9) && tuning("tracer_courant_kernel", 0) == 0;
    return run<TracerCheck>(who, {courant_tile, courant_direct, courant_level}, a, ld, xstart - 1, xstop - 1, ystart - 1, ystop - 1, empty,
                  tile, result_dev, result_host, s);
}

extern "C" int dlesm_tracer_courant_async_f64(double rdt, int ld, int ny, int xstart, int xstop, int ystart, int ystop,
                                              const int *tmask, const double *area_t, const double *un, const double *vn,
                                              const double *hu, const double *hv, const double *ht, const double *sshn_t,
                                              const double *sshn_u, const double *sshn_v, double face_limit,
                                              double outflow_limit, dlesm_tracer_courant *result_dev, void *stream)
{
    DLESM_REQUIRE(result_dev != nullptr, "dlesm_tracer_courant_async_f64: null result_dev");
    return tracer_courant_run("dlesm_tracer_courant_async_f64", rdt, ld, ny, xstart, xstop, ystart, ystop, tmask, area_t, un, vn,
                              hu, hv, ht, sshn_t, sshn_u, sshn_v, face_limit, outflow_limit, result_dev, nullptr,
                              (hipStream_t)stream);
}

extern "C" int dlesm_tracer_courant_f64(double rdt, int ld, int ny, int xstart, int xstop, int ystart, int ystop,
                                        const int *tmask, const double *area_t, const double *un, const double *vn,
                                        const double *hu, const double *hv, const double *ht, const double *sshn_t,
                                        const double *sshn_u, const double *sshn_v, double face_limit, double outflow_limit,
                                        dlesm_tracer_courant *result_host, void *stream)
{
    DLESM_REQUIRE(result_host != nullptr, "dlesm_tracer_courant_f64: null result");
    return tracer_courant_run("dlesm_tracer_courant_f64", rdt, ld, ny, xstart, xstop, ystart, ystop, tmask, area_t, un, vn, hu,
                              hv, ht, sshn_t, sshn_u, sshn_v, face_limit, outflow_limit, nullptr, result_host,
                              (hipStream_t)stream);
}
