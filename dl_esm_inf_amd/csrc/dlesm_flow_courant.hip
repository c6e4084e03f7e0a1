// The flow step's own stability check: one read-only sweep over the level-n flow that evaluates, in
// every wet T cell of a box, the water column d = ht + sshn_t, the gravity-wave number rdt * sqrt(g d) * sqrt(1/dx^2 + 1/dy^2),
// the advective number rdt * (max|u| / dx + max|v| / dy) over the cell's switched-on faces and the viscous number
// rdt * visc * (1/dx^2 + 1/dy^2), and reduces them to one 128-byte record: the three maxima and the smallest column, the
// lowest linear index that attains each, how many cells reach the caller's four limits, how many are `bad` and how many are
// wet.  Maxima, a minimum, integers and lowest indices: every member is exact and independent of the order of the reduction,
// so the record does not depend on the kernel form or the launch shape.  sqrt and the two divisions are the compiler's
// correctly rounded f64 ones, as in dlesm_open_bc.hip.
//
// This file holds the check's own part: the per-cell rule, the record, the loads of the two sweep forms and the entry's
// refusals (the policy FlowCheck).  The kernel bodies around them, the launch shape, the levels and the copy-back are
// dlesm_record_reduce.h's, shared with dlesm_courant.hip; the wave reductions are dlesm_wave_reduce.h's.
//
// flow_courant_tile: courant_tile's wave shape (dlesm_courant.hip) -- 64 lanes x 2 columns x 1 row in 16-byte lanes, un and
// the mask at i-1 / i+1 from the neighbouring lane by a DPP wave shift, lane 0 fetches the column west of the wave without a
// branch, lane 63 only loads, waves step by 63 chunks.  Of rows j-1 and j+1 only the mask and vn (row j-1) are read.  A wave
// that owns no wet cell of the box leaves after its mask row and contributes the identity.  Within the wave the reduction
// runs on the VALU, across the waves of a workgroup through LDS: one record per workgroup.
//
// flow_courant_direct: one cell per thread -- odd leading dimensions, unaligned bases and the HOOK key flow_courant_kernel = 1.
//
// flow_courant_level: workgroup b combines records [b * 1024, (b + 1) * 1024) into one; launched until one record is left,
// and that launch writes the caller's record (the empty extremes as 0.0 / +infinity / -1).  No atomics; plain vector stores.
#include <cmath>

#include "dlesm_record_reduce.h"

namespace dlesm {

namespace {

typedef double d2 __attribute__((ext_vector_type(2)));
typedef int i2 __attribute__((ext_vector_type(2)));

using namespace wavered;
using namespace recred;

struct FlowArgs {
    const int *tmask;
    const double *dx_t, *dy_t, *un, *vn, *ht, *sshn_t;
    double rdt, g, visc, gravity_limit, advective_limit, viscous_limit, depth_limit;
};

struct FlowCheck {
    using Args = FlowArgs;
    using Record = dlesm_flow_courant;
    // the six counts of a cell or a wave tile, a byte each (two cells a lane, 126 a wave):
    // a = wet | bad << 8 | gravity_over << 16 | advective_over << 24, b = viscous_over | shallow << 8
    struct Counts {
        int a, b;
    };

    // what one thread, one wave or one workgroup has seen.  A maximum of -1.0 (with NO_INDEX) stands for "none yet": every
    // value that competes is >= 0.  The smallest column is kept as the largest -d, -infinity for "none yet": every d that
    // competes is in (0, DBL_MAX], so one combine serves the four extremes.
    struct Acc {
        double gm, am, vm, nd;
        long long gi, ai, vi, di;
        long long over_g, over_a, over_v, shallow, bad, wet;
    };
    static __device__ __forceinline__ Acc identity()
    {
        return Acc{-1.0, -1.0, -1.0, -HUGE_VAL, NO_INDEX, NO_INDEX, NO_INDEX, NO_INDEX, 0, 0, 0, 0, 0, 0};
    }

    // one cell of section 6.15, line by line.  t_e, t_w, t_n, t_s: the mask at (i+1,j), (i-1,j), (i,j+1), (i,j-1);
    // u_w = un(i-1,j), v_s = vn(i,j-1); ix = the cell's 0-based linear index.  The extremes go into acc, the counts come back.
    static __device__ __forceinline__ Counts acc_cell(Acc &acc, const Args &f, bool wet, long long ix, double ht, double ssh,
                                                      double dx, double dy, double u, double u_w, double v, double v_s, int t_e,
                                                      int t_w, int t_n, int t_s)
    {
        const double d = ht + ssh;
        const double ivx = 1.0 / dx, ivy = 1.0 / dy;
        const double k2 = ivx * ivx + ivy * ivy;
        const double gw = (f.rdt * sqrt(f.g * d)) * sqrt(k2);
        const double a1 = t_e != 0 ? fabs(u) : 0.0, a2 = t_w != 0 ? fabs(u_w) : 0.0;
        const double a3 = t_n != 0 ? fabs(v) : 0.0, a4 = t_s != 0 ? fabs(v_s) : 0.0;
        const double um = a1 >= a2 ? a1 : a2, vm = a3 >= a4 ? a3 : a4;
        const double adv = (f.rdt * um) * ivx + (f.rdt * vm) * ivy;
        const double vis = (f.rdt * f.visc) * k2;
        const bool bad = !(d > 0.0 && d <= BIGGEST) || !valid(a1) || !valid(a2) || !valid(a3) || !valid(a4) || !valid(gw) ||
                         !valid(adv) || !valid(vis);
        const bool ok = wet && !bad;
        if (ok) {
            take(acc.gm, acc.gi, gw, ix);
            take(acc.am, acc.ai, adv, ix);
            take(acc.vm, acc.vi, vis, ix);
            take(acc.nd, acc.di, -d, ix);
        }
        return Counts{(int)wet | ((int)(wet && bad) << 8) | ((int)(ok && gw >= f.gravity_limit) << 16) |
                          ((int)(ok && adv >= f.advective_limit) << 24),
                      (int)(ok && vis >= f.viscous_limit) | ((int)(ok && d <= f.depth_limit) << 8)};
    }
    static __device__ __forceinline__ void add_counts(Acc &a, const Counts &c)
    {
        a.wet += c.a & 0xff, a.bad += (c.a >> 8) & 0xff, a.over_g += (c.a >> 16) & 0xff, a.over_a += (c.a >> 24) & 0xff;
        a.over_v += c.b & 0xff, a.shallow += (c.b >> 8) & 0xff;
    }
    static __device__ __forceinline__ Counts wave_counts(const Counts &c)
    {
        return Counts{wave_add_i32(c.a), wave_add_i32(c.b)};
    }

    // the four extremes and their lowest indices over the wave; every lane must be active
    static __device__ __forceinline__ void wave_pairs(Acc &a)
    {
        wave_pair(a.gm, a.gi, NO_INDEX);
        wave_pair(a.am, a.ai, NO_INDEX);
        wave_pair(a.vm, a.vi, NO_INDEX);
        wave_pair(a.nd, a.di, NO_INDEX);
    }
    // ... and the six counts as 64-bit sums (the one-cell-per-thread kernel, whose threads walk many rows, and the levels)
    static __device__ __forceinline__ void wave_reduce(Acc &a)
    {
        wave_pairs(a);
        a.over_g = wave_i64<OP_ADD>(a.over_g);
        a.over_a = wave_i64<OP_ADD>(a.over_a);
        a.over_v = wave_i64<OP_ADD>(a.over_v);
        a.shallow = wave_i64<OP_ADD>(a.shallow);
        a.bad = wave_i64<OP_ADD>(a.bad);
        a.wet = wave_i64<OP_ADD>(a.wet);
    }

    static __device__ __forceinline__ void merge(Acc &a, const Acc &b)
    {
        take(a.gm, a.gi, b.gm, b.gi);
        take(a.am, a.ai, b.am, b.ai);
        take(a.vm, a.vi, b.vm, b.vi);
        take(a.nd, a.di, b.nd, b.di);
        a.over_g += b.over_g, a.over_a += b.over_a, a.over_v += b.over_v, a.shallow += b.shallow, a.bad += b.bad,
            a.wet += b.wet;
    }

    // in the scratch records "none yet" reads -1.0 / +infinity with NO_INDEX; only the last level writes 0.0 / +infinity / -1
    static __device__ __forceinline__ Record to_record(const Acc &a)
    {
        return Record{a.gm, a.am, a.vm, -a.nd, a.gi, a.ai, a.vi, a.di, a.over_g, a.over_a, a.over_v, a.shallow,
                      a.bad, a.wet, {0, 0}};
    }
    static __device__ __forceinline__ Acc from_record(const Record &r)
    {
        return Acc{r.gravity_max, r.advective_max, r.viscous_max, -r.depth_min, r.gravity_index, r.advective_index,
                   r.viscous_index, r.depth_index, r.gravity_over, r.advective_over, r.viscous_over, r.shallow, r.invalid,
                   r.wet};
    }
    static __device__ __forceinline__ void finish(Acc &acc)
    {
        if (acc.gi == NO_INDEX) acc.gm = 0.0, acc.gi = -1;
        if (acc.ai == NO_INDEX) acc.am = 0.0, acc.ai = -1;
        if (acc.vi == NO_INDEX) acc.vm = 0.0, acc.vi = -1;
        if (acc.di == NO_INDEX) acc.nd = -HUGE_VAL, acc.di = -1;
    }

    // one wave tile of row j (0-based); lane 0 of the tile holds chunk c0.  cn: the lane's counts
    static __device__ __forceinline__ void tile_row(const Args &f, int ld, int x0, int x1, int j, int c0, int lane, Acc &acc,
                                                    Counts &cn)
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

        // the west column this wave cannot get from a lane (no branch, LAB_NOTES.md section 5.10)
        const size_t ow = row + (size_t)((lane == 0 && m0) ? c * 2 - 1 : cl * 2);
        const i2 ts = *(const i2 *)(f.tmask + os), tn = *(const i2 *)(f.tmask + on);
        int tw = f.tmask[ow];
        const d2 un = *(const d2 *)(f.un + o), vn = *(const d2 *)(f.vn + o), vn_s = *(const d2 *)(f.vn + os);
        double un_w = f.un[ow];
        const d2 ht = *(const d2 *)(f.ht + o), st = *(const d2 *)(f.sshn_t + o);
        const d2 dx = *(const d2 *)(f.dx_t + o), dy = *(const d2 *)(f.dy_t + o);
        {
            const double u1 = from_lower<true>(un.y);
            const int t1 = __builtin_amdgcn_mov_dpp(t.y, 0x138, 0xf, 0xf, true);
            if (lane != 0) un_w = u1, tw = t1;
        }
        const int te = __builtin_amdgcn_mov_dpp(t.x, 0x130, 0xf, 0xf, true);      // (lane 63: 0, never used)
        const long long ix = (long long)row + (long long)c * 2;
        const Counts k0 = acc_cell(acc, f, wet0, ix, ht.x, st.x, dx.x, dy.x, un.x, un_w, vn.x, vn_s.x, t.y, tw, tn.x, ts.x);
        const Counts k1 = acc_cell(acc, f, wet1, ix + 1, ht.y, st.y, dx.y, dy.y, un.y, un.x, vn.y, vn_s.y, te, t.x, tn.y, ts.y);
        cn = Counts{k0.a + k1.a, k0.b + k1.b};
    }

    // the cell at linear offset o, one thread's
    static __device__ __forceinline__ void direct_cell(const Args &f, int ld, size_t o, Acc &acc)
    {
        if (f.tmask[o] <= 0) return;
        add_counts(acc, acc_cell(acc, f, true, (long long)o, f.ht[o], f.sshn_t[o], f.dx_t[o], f.dy_t[o], f.un[o], f.un[o - 1],
                                 f.vn[o], f.vn[o - ld], f.tmask[o + 1], f.tmask[o - 1], f.tmask[o + ld], f.tmask[o - ld]));
    }
};

__global__ __launch_bounds__(256, 4) void flow_courant_tile(const FlowArgs a, int ld, int x0, int x1, int y0, int y1,
                                                            int c_first, int nxw, dlesm_flow_courant *__restrict__ rec)
{
    tile_body<FlowCheck>(a, ld, x0, x1, y0, y1, c_first, nxw, rec);
}
__global__ __launch_bounds__(256) void flow_courant_direct(const FlowArgs f, int ld, int x0, int x1, int y0, int y1,
                                                           dlesm_flow_courant *__restrict__ rec)
{
    direct_body<FlowCheck>(f, ld, x0 + blockIdx.x * blockDim.x + threadIdx.x, x1, y0, y1,
                           rec + ((size_t)blockIdx.y * gridDim.x + blockIdx.x));
}
__global__ __launch_bounds__(256) void flow_courant_level(const dlesm_flow_courant *__restrict__ src, long long n,
                                                          dlesm_flow_courant *__restrict__ dst, int last)
{
    level_body<FlowCheck>(src, n, dst, last);
}

} // namespace

} // namespace dlesm

using namespace dlesm;

// Both forms of the entry (recred::run): the refusals, in their order, then the sweep
static int flow_courant_run(const char *who, double rdt, double g, double visc, int ld, int ny, int xstart, int xstop,
                            int ystart, int ystop, const int *tmask, const double *dx_t, const double *dy_t, const double *un,
                            const double *vn, const double *ht, const double *sshn_t, double gravity_limit,
                            double advective_limit, double viscous_limit, double depth_limit, dlesm_flow_courant *result_dev,
                            dlesm_flow_courant *result_host, hipStream_t s)
{
    static_assert(sizeof(dlesm_flow_courant) == 128, "dlesm_flow_courant has padding");
    if (int rc = ensure_device()) return rc;
    const double *const ins[6] = {dx_t, dy_t, un, vn, ht, sshn_t};
    static const char *const in_name[6] = {"dx_t", "dy_t", "un", "vn", "ht", "sshn_t"};
    DLESM_REQUIRE(result_dev != nullptr || result_host != nullptr, "%s: null result", who);
    if (int rc = check_arrays(who, tmask, ins, in_name, 6)) return rc;
    DLESM_REQUIRE(ld >= 1 && ny >= 1, "%s: array extents %dx%d", who, ld, ny);
    const bool empty = xstop < xstart || ystop < ystart;
    if (!empty)
        if (int rc = check_box(who, ld, ny, xstart, xstop, ystart, ystop, 1)) return rc;
    DLESM_REQUIRE(rdt > 0.0, "%s: rdt %g (a positive number)", who, rdt);
    DLESM_REQUIRE(g > 0.0, "%s: g %g (a positive number)", who, g);
    DLESM_REQUIRE(visc >= 0.0, "%s: visc %g (not negative)", who, visc);
    DLESM_REQUIRE(gravity_limit > 0.0, "%s: gravity_limit %g (a positive number)", who, gravity_limit);
    DLESM_REQUIRE(advective_limit > 0.0, "%s: advective_limit %g (a positive number)", who, advective_limit);
    DLESM_REQUIRE(viscous_limit > 0.0, "%s: viscous_limit %g (a positive number)", who, viscous_limit);
    DLESM_REQUIRE(depth_limit >= 0.0, "%s: depth_limit %g (not negative)", who, depth_limit);
    if (int rc = check_result_apart(who, result_dev, sizeof *result_dev, ld, ny, tmask, ins, in_name, 6)) return rc;
    DLESM_REQUIRE(!capturing(s), "%s: not callable under stream capture", who);

    const FlowArgs a{tmask, dx_t, dy_t, un, vn, ht, sshn_t, rdt, g, visc, gravity_limit, advective_limit, viscous_limit,
                     depth_limit};
    const bool tile = lanes16_fit(ld, tmask, ins, 6) && tuning("flow_courant_kernel", 0) == 0;
    return run<FlowCheck>(who, {flow_courant_tile, flow_courant_direct, flow_courant_level}, a, ld, xstart - 1, xstop - 1,
                          ystart - 1, ystop - 1, empty, tile, result_dev, result_host, s);
}

extern "C" int dlesm_flow_courant_async_f64(double rdt, double g, double visc, int ld, int ny, int xstart, int xstop,
                                            int ystart, int ystop, const int *tmask, const double *dx_t, const double *dy_t,
                                            const double *un, const double *vn, const double *ht, const double *sshn_t,
                                            double gravity_limit, double advective_limit, double viscous_limit,
                                            double depth_limit, dlesm_flow_courant *result_dev, void *stream)
{
    DLESM_REQUIRE(result_dev != nullptr, "dlesm_flow_courant_async_f64: null result_dev");
    return flow_courant_run("dlesm_flow_courant_async_f64", rdt, g, visc, ld, ny, xstart, xstop, ystart, ystop, tmask, dx_t,
                            dy_t, un, vn, ht, sshn_t, gravity_limit, advective_limit, viscous_limit, depth_limit, result_dev,
                            nullptr, (hipStream_t)stream);
}

extern "C" int dlesm_flow_courant_f64(double rdt, double g, double visc, int ld, int ny, int xstart, int xstop, int ystart,
                                      int ystop, const int *tmask, const double *dx_t, const double *dy_t, const double *un,
                                      const double *vn, const double *ht, const double *sshn_t, double gravity_limit,
                                      double advective_limit, double viscous_limit, double depth_limit,
                                      dlesm_flow_courant *result_host, void *stream)
{
    DLESM_REQUIRE(result_host != nullptr, "dlesm_flow_courant_f64: null result");
    return flow_courant_run("dlesm_flow_courant_f64", rdt, g, visc, ld, ny, xstart, xstop, ystart, ystop, tmask, dx_t, dy_t, un,
                            vn, ht, sshn_t, gravity_limit, advective_limit, viscous_limit, depth_limit, nullptr, result_host,
                            (hipStream_t)stream);
}
