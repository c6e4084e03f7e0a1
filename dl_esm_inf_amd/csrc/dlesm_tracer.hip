// Tracer transport of a NEMOLite2D-class model: first-order upwind advection of up to
// DLESM_TRACER_MAX tracers with continuity's own face transports, in one sweep that loads the flow once.
//
// tracer_tile<NT>: the one-sweep step's wave tile (dlesm_nemolite_step.hip) -- 64 lanes x 2 columns x 1 row in 16-byte lanes,
// operands at i-1 / i+1 from the neighbouring lane by a DPP wave shift, lane 0 fetches the column west of the wave without a
// branch, lane 63 only loads (its chunk is the east column of lane 62 and the next wave's lane 0), waves step by 63 chunks.
// A wave first loads its row of the mask and returns if it owns no wet cell of the box (one ballot: only wet cells are
// written, so land costs a mask read).  Then the flow: un, hu, sshn_u on the row, vn, hv, sshn_v on the row and the one
// below, ht, sshn_t, ssha, area_t and the mask rows above and below; r1..r4, the four face switches, q, h_old and h_new of
// the lane's two cells stay in registers (TracerFlow, dlesm_nemolite.h) and the NT tracers are applied from them in an
// unrolled loop, tracer k+1's loads issued in front of tracer k's arithmetic.  NT is a template parameter, so the tracer
// pointers are kernel arguments indexed by constants (scalar registers, no scratch).  Instantiated for 1..4 tracers; a call
// with 5..8 is two launches (4, then the rest), each loading the flow once: 84 + 16 K B/cell up to 4 tracers, 168 + 16 K
// beyond, against 100 K for K single-tracer sweeps.
//
// tracer_direct<NT>: one cell per thread -- odd leading dimensions, unaligned bases and the HOOK key tracer_kernel = 1.
//
// Second-order limited transport (dlesm_tracer_step_muscl_f64): the same sweep with the value a face
// carries rebuilt from the upwind cell's monotonised-central slope (muscl_slope / tracer_point_muscl, dlesm_nemolite.h).  The
// stencil reaches two cells.  tracer_muscl_tile<NT> keeps the shape above and feeds the wave's two ends with two load-only
// lanes: lanes 1..62 own a chunk, lanes 0 and 63 load the chunk west / east of them, waves step by 62 chunks.  Every lane
// computes the x slopes of its own two columns from its neighbours' near columns (one DPP shift each way) and hands them on by
// a second shift, so both columns of lanes c-1 and c+1 reach lane c with four shifts of doubles per tracer and no lane
// evaluates a slope twice; the alternative, 63 owned chunks and extra edge loads, needs two scalar loads per row, array and
// tracer at each end and a second evaluation of the end slopes behind a lane test.  Rows j-2 .. j+2 of the lane's own columns
// are loaded for c and for the mask.  A chunk or a row outside the array is loaded clamped and its mask forced to 0 by a
// select, which zeroes every slope that would have read it.  tracer_muscl_direct<NT>: one cell per thread, HOOK key
// tracer_muscl_kernel = 1.
//
// Time-centred limited transport (dlesm_tracer_step_hancock_f64): the two kernels above with a second
// template parameter, <NT, true>; <NT, false> is section 6.11's sweep.  The constant 0.5 in front of a slope becomes a factor
// per face, 0.5 * (1 - n) with n the face's Courant number in its upwind cell (tracer_courant / tracer_point_hancock,
// dlesm_nemolite.h).  The factors depend on the flow only: every lane computes w = rdt / (area_t * (ht + sshn_t)) of its own
// two columns on rows j-1, j, j+1 (six divisions and six more 16-byte loads a lane and tile, re-reads), takes w of columns
// i-1 and i+1 from its neighbours by the DPP shifts of the flow stage -- the load-only lanes supply the tile's ends -- and
// keeps g1..g4 of its two cells in registers for the unrolled tracer loop.  HOOK key tracer_hancock_kernel = 1.
#include "dlesm_nemolite.h"

namespace dlesm {

namespace {

typedef double d2 __attribute__((ext_vector_type(2)));
typedef int i2 __attribute__((ext_vector_type(2)));

using namespace nemo;

constexpr int TILE_CHUNKS = CHUNKS_EAST;      // chunks (2 columns) a wave owns; lane 63 only loads
constexpr int NT_MAX = 4;             // tracers per launch

template <int NT> struct TracerArgs {
    TracerFields f;
    const double *c_in[NT];
    double *c_out[NT];
    double rdt;
};

// a column pair: both columns in one 16-byte store, a mixed pair per column (a cell not written is never stored)
__device__ __forceinline__ void store_pair(double *p, double x0, double x1, bool w0, bool w1)
{
    if (w0 && w1) *(d2 *)p = d2{x0, x1};
    else {
        if (w0) p[0] = x0;
        if (w1) p[1] = x1;
    }
}

// what one tracer's update reads: its row (and the column west of the wave), the rows below and above
struct TracerRows {
    d2 m, s, n;
    double w;
};
__device__ __forceinline__ TracerRows load_rows(const double *c, size_t o, size_t ow, int ld)
{
    return TracerRows{*(const d2 *)(c + o), *(const d2 *)(c + o - ld), *(const d2 *)(c + o + ld), c[ow]};
}

// (x0:x1, y0:y1) = the box (0-based); nxw tiles per row, tile 0 begins at chunk c_first
template <int NT>
__global__ __launch_bounds__(256) void tracer_tile(TracerArgs<NT> a, int ld, int x0, int x1, int y0, int y1, int c_first,
                                                   int nxw)
{
    const TracerFields &f = a.f;
    const int lane = threadIdx.x & 63;
    const int w = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    const int xw = w % nxw, j = y0 + w / nxw;
    if (j > y1) return;
    const int c = c_first + xw * TILE_CHUNKS + lane;     // this lane's chunk (2 columns); lane 63 = the next wave's lane 0
    if (c - lane > x1 / 2) return;                       // idle padding tile
    const int c_ld = ld / 2 - 1, cl = c < c_ld ? c : c_ld;
    const bool own = lane != 63;                         // lane 63 only loads: its chunk is the east column of lane 62
    const bool m0 = own && c * 2 >= x0 && c * 2 <= x1, m1 = own && c * 2 + 1 >= x0 && c * 2 + 1 <= x1;
    const size_t row = (size_t)j * ld, o = row + (size_t)cl * 2;

    // the land exit: the mask of the row first; a wave that owns no wet cell of the box stores nothing
    const i2 t = *(const i2 *)(f.tmask + o);
    const bool wet0 = m0 && t.x > 0, wet1 = m1 && t.y > 0;
    if (__ballot(wet0 || wet1) == 0) return;

    // the west column this wave cannot get from a lane (no branch, LAB_NOTES.md section 5.10)
    const size_t ow = row + (size_t)((lane == 0 && m0) ? c * 2 - 1 : cl * 2);
    TracerRows cur = load_rows(a.c_in[0], o, ow, ld);    // the first tracer's loads go out with the flow's

    const i2 ts = *(const i2 *)(f.tmask + o - ld), tn = *(const i2 *)(f.tmask + o + ld);
    int tw = f.tmask[ow];
    const d2 su = *(const d2 *)(f.sshn_u + o), hu = *(const d2 *)(f.hu + o), un = *(const d2 *)(f.un + o);
    double su_w = f.sshn_u[ow], hu_w = f.hu[ow], un_w = f.un[ow];
    const d2 sv = *(const d2 *)(f.sshn_v + o), hv = *(const d2 *)(f.hv + o), vn = *(const d2 *)(f.vn + o);
    const d2 sv_s = *(const d2 *)(f.sshn_v + o - ld), hv_s = *(const d2 *)(f.hv + o - ld), vn_s = *(const d2 *)(f.vn + o - ld);
    const d2 ht = *(const d2 *)(f.ht + o), st = *(const d2 *)(f.sshn_t + o), sa = *(const d2 *)(f.ssha + o);
    const d2 ar = *(const d2 *)(f.area_t + o);

    {
        const double s1 = from_lower<true>(su.y), h1 = from_lower<true>(hu.y), u1 = from_lower<true>(un.y);
        const int t1 = __builtin_amdgcn_mov_dpp(t.y, 0x138, 0xf, 0xf, true);
        if (lane != 0) su_w = s1, hu_w = h1, un_w = u1, tw = t1;
    }
    const int te = __builtin_amdgcn_mov_dpp(t.x, 0x130, 0xf, 0xf, true);      // (lane 63: 0, never used)
    const TracerFlow f0 = tracer_flow(a.rdt, su.x, su_w, sv.x, sv_s.x, hu.x, hu_w, hv.x, hv_s.x, un.x, un_w, vn.x, vn_s.x,
                                      ar.x, ht.x, st.x, sa.x, t.y, tw, tn.x, ts.x);
    const TracerFlow f1 = tracer_flow(a.rdt, su.y, su.x, sv.y, sv_s.y, hu.y, hu.x, hv.y, hv_s.y, un.y, un.x, vn.y, vn_s.y,
                                      ar.y, ht.y, st.y, sa.y, te, t.x, tn.y, ts.y);

    const size_t oc = row + (size_t)c * 2;
#pragma unroll
    for (int k = 0; k < NT; k++) {
        TracerRows nxt = cur;
        if (k + 1 < NT) nxt = load_rows(a.c_in[k + 1], o, ow, ld);
        const double wl = from_lower<true>(cur.m.y), c_e = from_upper<true>(cur.m.x);
        const double c_w = lane != 0 ? wl : cur.w;
        const double o0 = tracer_point(f0, cur.m.x, cur.m.y, c_w, cur.n.x, cur.s.x);
        const double o1 = tracer_point(f1, cur.m.y, c_e, cur.m.x, cur.n.y, cur.s.y);
        store_pair(a.c_out[k] + oc, o0, o1, wet0, wet1);
        cur = nxt;
    }
}

// one cell per thread: odd leading dimensions, unaligned bases, the HOOK key tracer_kernel
template <int NT>
__global__ __launch_bounds__(256) void tracer_direct(TracerArgs<NT> a, int ld, int x0, int x1, int y0, int y1)
{
    const TracerFields &f = a.f;
    const int i = x0 + blockIdx.x * blockDim.x + threadIdx.x;
    if (i > x1) return;
    for (int j = y0 + blockIdx.y; j <= y1; j += gridDim.y) {
        const size_t o = (size_t)j * ld + i;
        if (f.tmask[o] <= 0) continue;
        const TracerFlow fl = tracer_flow(a.rdt, f.sshn_u[o], f.sshn_u[o - 1], f.sshn_v[o], f.sshn_v[o - ld], f.hu[o],
                                          f.hu[o - 1], f.hv[o], f.hv[o - ld], f.un[o], f.un[o - 1], f.vn[o], f.vn[o - ld],
                                          f.area_t[o], f.ht[o], f.sshn_t[o], f.ssha[o], f.tmask[o + 1], f.tmask[o - 1],
                                          f.tmask[o + ld], f.tmask[o - ld]);
#pragma unroll
        for (int k = 0; k < NT; k++) {
            const double *c = a.c_in[k];
            a.c_out[k][o] = tracer_point(fl, c[o], c[o + 1], c[o - 1], c[o + ld], c[o - ld]);
        }
    }
}

// ---- second-order limited transport ----------------------------------------------------------

constexpr int MUSCL_CHUNKS = CHUNKS_BOTH;     // chunks a wave owns; lanes 0 and 63 only load

// what one tracer's update reads: rows j-2 .. j+2 of the lane's two columns
struct MusclRows {
    d2 ss, s, m, n, nn;
};
__device__ __forceinline__ MusclRows load_muscl_rows(const double *c, size_t oss, size_t os, size_t o, size_t on, size_t onn)
{
    return MusclRows{*(const d2 *)(c + oss), *(const d2 *)(c + os), *(const d2 *)(c + o), *(const d2 *)(c + on),
                     *(const d2 *)(c + onn)};
}

// (x0:x1, y0:y1) = the box (0-based); nxw tiles per row, lane 1 of tile 0 holds chunk c_first.  HANCOCK: section 6.12's
// face factors in the place of 0.5; <NT, false> compiles to the code the kernel had before it had the parameter
template <int NT, bool HANCOCK = false>
__global__ __launch_bounds__(256) void tracer_muscl_tile(TracerArgs<NT> a, int ld, int ny, int x0, int x1, int y0, int y1,
                                                         int c_first, int nxw)
{
    const TracerFields &f = a.f;
    const int lane = threadIdx.x & 63;
    const int w = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    const int xw = w % nxw, j = y0 + w / nxw;
    if (j > y1) return;
    const int c = c_first + xw * MUSCL_CHUNKS + lane - 1;  // this lane's chunk (2 columns); lane 0: the one west of the tile
    if (c - lane + 1 > x1 / 2) return;                     // idle padding tile
    const int c_ld = ld / 2 - 1, cl = c < 0 ? 0 : (c < c_ld ? c : c_ld);
    const bool in = c == cl;                               // the chunk lies in the array: otherwise loaded clamped, mask 0
    const bool own = lane != 0 && lane != 63;
    const bool m0 = own && c * 2 >= x0 && c * 2 <= x1, m1 = own && c * 2 + 1 >= x0 && c * 2 + 1 <= x1;
    const size_t col = (size_t)cl * 2, row = (size_t)j * ld, o = row + col;

    // the land exit: the mask of the row first; a wave that owns no wet cell of the box stores nothing
    i2 t = *(const i2 *)(f.tmask + o);
    const bool wet0 = m0 && t.x > 0, wet1 = m1 && t.y > 0;
    if (__ballot(wet0 || wet1) == 0) return;

    // rows j-1 and j+1 lie in the array (the box has its ring); rows j-2 and j+2 may not: clamped, mask 0
    const bool in_ss = j >= 2, in_nn = j + 2 < ny;
    const size_t os = o - ld, on = o + ld, oss = (size_t)(in_ss ? j - 2 : 0) * ld + col,
                 onn = (size_t)(in_nn ? j + 2 : ny - 1) * ld + col;
    // section 6.12: w of the lane's two columns on rows j-1 and j+1 (with row j's, six divisions a lane and tile, none per
    // tracer), asked for in front of everything else: the six row pairs are then dead before the tracers' rows arrive, and
    // every instantiation stays at four waves per SIMD (LAB_NOTES.md section 5.21)
    d2 ws{}, wn{};
    if constexpr (HANCOCK) {
        const d2 ar_s = *(const d2 *)(f.area_t + os), ht_s = *(const d2 *)(f.ht + os), st_s = *(const d2 *)(f.sshn_t + os);
        const d2 ar_n = *(const d2 *)(f.area_t + on), ht_n = *(const d2 *)(f.ht + on), st_n = *(const d2 *)(f.sshn_t + on);
        ws = d2{tracer_weight(a.rdt, ar_s.x, ht_s.x, st_s.x), tracer_weight(a.rdt, ar_s.y, ht_s.y, st_s.y)};
        wn = d2{tracer_weight(a.rdt, ar_n.x, ht_n.x, st_n.x), tracer_weight(a.rdt, ar_n.y, ht_n.y, st_n.y)};
    }
    MusclRows cur = load_muscl_rows(a.c_in[0], oss, os, o, on, onn);     // the first tracer's loads go out with the flow's

    i2 ts = *(const i2 *)(f.tmask + os), tn = *(const i2 *)(f.tmask + on);
    i2 tss = *(const i2 *)(f.tmask + oss), tnn = *(const i2 *)(f.tmask + onn);
    const d2 su = *(const d2 *)(f.sshn_u + o), hu = *(const d2 *)(f.hu + o), un = *(const d2 *)(f.un + o);
    const d2 sv = *(const d2 *)(f.sshn_v + o), hv = *(const d2 *)(f.hv + o), vn = *(const d2 *)(f.vn + o);
    const d2 sv_s = *(const d2 *)(f.sshn_v + os), hv_s = *(const d2 *)(f.hv + os), vn_s = *(const d2 *)(f.vn + os);
    const d2 ht = *(const d2 *)(f.ht + o), st = *(const d2 *)(f.sshn_t + o), sa = *(const d2 *)(f.ssha + o);
    const d2 ar = *(const d2 *)(f.area_t + o);

    if (!in) t = i2{0, 0}, ts = i2{0, 0}, tn = i2{0, 0};
    if (!in || !in_ss) tss = i2{0, 0};
    if (!in || !in_nn) tnn = i2{0, 0};

    const double su_w = from_lower<true>(su.y), hu_w = from_lower<true>(hu.y), un_w = from_lower<true>(un.y);
    const int tw = __builtin_amdgcn_mov_dpp(t.y, 0x138, 0xf, 0xf, true);      // (lane 0: 0, never used)
    const int te = __builtin_amdgcn_mov_dpp(t.x, 0x130, 0xf, 0xf, true);      // (lane 63: 0, never used)
    const TracerFlow f0 = tracer_flow(a.rdt, su.x, su_w, sv.x, sv_s.x, hu.x, hu_w, hv.x, hv_s.x, un.x, un_w, vn.x, vn_s.x,
                                      ar.x, ht.x, st.x, sa.x, t.y, tw, tn.x, ts.x);
    const TracerFlow f1 = tracer_flow(a.rdt, su.y, su.x, sv.y, sv_s.y, hu.y, hu.x, hv.y, hv_s.y, un.y, un.x, vn.y, vn_s.y,
                                      ar.y, ht.y, st.y, sa.y, te, t.x, tn.y, ts.y);
    // section 6.12: w of the lane's own row; w of columns i-1 and i+1 from the neighbouring lanes, the load-only lanes
    // supplying the tile's ends.  A clamped chunk's w belongs to another cell: it reaches only the factor of a face whose flux
    // the forced mask switches off.
    TracerCourant g0{}, g1{};
    if constexpr (HANCOCK) {
        const double w0 = tracer_weight(a.rdt, ar.x, ht.x, st.x), w1 = tracer_weight(a.rdt, ar.y, ht.y, st.y);
        const double w_w = from_lower<true>(w1), w_e = from_upper<true>(w0);
        g0 = tracer_courant(f0, w0, w1, w_w, wn.x, ws.x);
        g1 = tracer_courant(f1, w1, w_e, w0, wn.y, ws.y);
    }
    // where a slope is taken: a wet cell between two cells that are not land.  x: the lane's two columns (lane 0's west
    // column and lane 63's east column get none, and nothing asks for them); y: rows j-1, j, j+1 of both columns
    const bool x_0 = t.x > 0 && tw != 0 && t.y != 0, x_1 = t.y > 0 && t.x != 0 && te != 0;
    const bool ys_0 = ts.x > 0 && tss.x != 0 && t.x != 0, ys_1 = ts.y > 0 && tss.y != 0 && t.y != 0;
    const bool ym_0 = t.x > 0 && ts.x != 0 && tn.x != 0, ym_1 = t.y > 0 && ts.y != 0 && tn.y != 0;
    const bool yn_0 = tn.x > 0 && t.x != 0 && tnn.x != 0, yn_1 = tn.y > 0 && t.y != 0 && tnn.y != 0;

    const size_t oc = row + (size_t)c * 2;
#pragma unroll
    for (int k = 0; k < NT; k++) {
        MusclRows nxt = cur;
        if (k + 1 < NT) nxt = load_muscl_rows(a.c_in[k + 1], oss, os, o, on, onn);
        const double c_w = from_lower<true>(cur.m.y), c_e = from_upper<true>(cur.m.x);
        const double sx0 = muscl_slope(x_0, c_w, cur.m.x, cur.m.y), sx1 = muscl_slope(x_1, cur.m.x, cur.m.y, c_e);
        const double sx_w = from_lower<true>(sx1), sx_e = from_upper<true>(sx0);
        double o0, o1;
        if constexpr (HANCOCK) {
            o0 = tracer_point_hancock(f0, g0, cur.m.x, cur.m.y, c_w, cur.n.x, cur.s.x, sx0, sx1, sx_w,
                                      muscl_slope(ym_0, cur.s.x, cur.m.x, cur.n.x),
                                      muscl_slope(yn_0, cur.m.x, cur.n.x, cur.nn.x),
                                      muscl_slope(ys_0, cur.ss.x, cur.s.x, cur.m.x));
            o1 = tracer_point_hancock(f1, g1, cur.m.y, c_e, cur.m.x, cur.n.y, cur.s.y, sx1, sx_e, sx0,
                                      muscl_slope(ym_1, cur.s.y, cur.m.y, cur.n.y),
                                      muscl_slope(yn_1, cur.m.y, cur.n.y, cur.nn.y),
                                      muscl_slope(ys_1, cur.ss.y, cur.s.y, cur.m.y));
        } else {
            o0 = tracer_point_muscl(f0, cur.m.x, cur.m.y, c_w, cur.n.x, cur.s.x, sx0, sx1, sx_w,
                                    muscl_slope(ym_0, cur.s.x, cur.m.x, cur.n.x),
                                    muscl_slope(yn_0, cur.m.x, cur.n.x, cur.nn.x),
                                    muscl_slope(ys_0, cur.ss.x, cur.s.x, cur.m.x));
            o1 = tracer_point_muscl(f1, cur.m.y, c_e, cur.m.x, cur.n.y, cur.s.y, sx1, sx_e, sx0,
                                    muscl_slope(ym_1, cur.s.y, cur.m.y, cur.n.y),
                                    muscl_slope(yn_1, cur.m.y, cur.n.y, cur.nn.y),
                                    muscl_slope(ys_1, cur.ss.y, cur.s.y, cur.m.y));
        }
        store_pair(a.c_out[k] + oc, o0, o1, wet0, wet1);
        cur = nxt;
    }
}

// one cell per thread: odd leading dimensions, unaligned bases, the HOOK keys tracer_muscl_kernel / tracer_hancock_kernel
template <int NT, bool HANCOCK = false>
__global__ __launch_bounds__(256) void tracer_muscl_direct(TracerArgs<NT> a, int ld, int ny, int x0, int x1, int y0, int y1)
{
    const TracerFields &f = a.f;
    const int i = x0 + blockIdx.x * blockDim.x + threadIdx.x;
    if (i > x1) return;
    // columns i-1, i+1 and rows j-1, j+1 lie in the array (the box has its ring); i-2, i+2, j-2, j+2 may not: clamped, mask 0
    const bool in_ww = i >= 2, in_ee = i + 2 < ld;
    const int iww = in_ww ? i - 2 : 0, iee = in_ee ? i + 2 : ld - 1;
    for (int j = y0 + blockIdx.y; j <= y1; j += gridDim.y) {
        const size_t o = (size_t)j * ld + i;
        const int t = f.tmask[o];
        if (t <= 0) continue;
        const bool in_ss = j >= 2, in_nn = j + 2 < ny;
        const size_t oww = (size_t)j * ld + iww, oee = (size_t)j * ld + iee;
        const size_t oss = (size_t)(in_ss ? j - 2 : 0) * ld + i, onn = (size_t)(in_nn ? j + 2 : ny - 1) * ld + i;
        const int t_e = f.tmask[o + 1], t_w = f.tmask[o - 1], t_n = f.tmask[o + ld], t_s = f.tmask[o - ld];
        const int l_ee = f.tmask[oee], l_ww = f.tmask[oww], l_nn = f.tmask[onn], l_ss = f.tmask[oss];
        const int t_ee = in_ee ? l_ee : 0, t_ww = in_ww ? l_ww : 0, t_nn = in_nn ? l_nn : 0, t_ss = in_ss ? l_ss : 0;
        const TracerFlow fl = tracer_flow(a.rdt, f.sshn_u[o], f.sshn_u[o - 1], f.sshn_v[o], f.sshn_v[o - ld], f.hu[o],
                                          f.hu[o - 1], f.hv[o], f.hv[o - ld], f.un[o], f.un[o - 1], f.vn[o], f.vn[o - ld],
                                          f.area_t[o], f.ht[o], f.sshn_t[o], f.ssha[o], t_e, t_w, t_n, t_s);
        const bool x_m = t_e != 0 && t_w != 0, y_m = t_n != 0 && t_s != 0;           // (t > 0 here)
        const bool x_e = t_e > 0 && t_ee != 0, x_w = t_w > 0 && t_ww != 0;            // (t != 0 here)
        const bool y_n = t_n > 0 && t_nn != 0, y_s = t_s > 0 && t_ss != 0;
        TracerCourant g{};
        if constexpr (HANCOCK) {
            auto W = [&](size_t p) { return tracer_weight(a.rdt, f.area_t[p], f.ht[p], f.sshn_t[p]); };
            g = tracer_courant(fl, W(o), W(o + 1), W(o - 1), W(o + ld), W(o - ld));
        }
#pragma unroll
        for (int k = 0; k < NT; k++) {
            const double *c = a.c_in[k];
            const double cm = c[o], ce = c[o + 1], cw = c[o - 1], cn = c[o + ld], cs = c[o - ld];
            if constexpr (HANCOCK)
                a.c_out[k][o] = tracer_point_hancock(fl, g, cm, ce, cw, cn, cs, muscl_slope(x_m, cw, cm, ce),
                                                     muscl_slope(x_e, cm, ce, c[oee]), muscl_slope(x_w, c[oww], cw, cm),
                                                     muscl_slope(y_m, cs, cm, cn), muscl_slope(y_n, cm, cn, c[onn]),
                                                     muscl_slope(y_s, c[oss], cs, cm));
            else
                a.c_out[k][o] = tracer_point_muscl(fl, cm, ce, cw, cn, cs, muscl_slope(x_m, cw, cm, ce),
                                                   muscl_slope(x_e, cm, ce, c[oee]), muscl_slope(x_w, c[oww], cw, cm),
                                                   muscl_slope(y_m, cs, cm, cn), muscl_slope(y_n, cm, cn, c[onn]),
                                                   muscl_slope(y_s, c[oss], cs, cm));
        }
    }
}

enum Scheme { SCHEME_UPWIND = 0, SCHEME_MUSCL = 1, SCHEME_HANCOCK = 2 };    // sections 6.10, 6.11, 6.12

struct Launch {
    bool tile;
    Scheme scheme;
    int ld, ny, x0, x1, y0, y1;
    TilePlan p;               // tile: its plan
    hipStream_t st;
};

template <int NT>
void launch(const Launch &l, double rdt, const TracerFields &f, const double *const *c_in, double *const *c_out)
{
    TracerArgs<NT> a{};
    a.f = f, a.rdt = rdt;
    for (int k = 0; k < NT; k++) a.c_in[k] = c_in[k], a.c_out[k] = c_out[k];
    const DirectGrid g = direct_grid(l.x0, l.x1, l.y0, l.y1);
    if (l.scheme != SCHEME_UPWIND) {
        if (l.tile) {
            const auto tile = l.scheme == SCHEME_HANCOCK ? tracer_muscl_tile<NT, true> : tracer_muscl_tile<NT, false>;
            hipLaunchKernelGGL(tile, dim3(l.p.grid), dim3(64 * l.p.tpb), 0, l.st, a, l.ld, l.ny, l.x0, l.x1, l.y0, l.y1,
                               l.p.c_first, l.p.nxw);
        } else {
            const auto direct = l.scheme == SCHEME_HANCOCK ? tracer_muscl_direct<NT, true> : tracer_muscl_direct<NT, false>;
            hipLaunchKernelGGL(direct, dim3(g.x, g.y), dim3(256), 0, l.st, a, l.ld, l.ny, l.x0, l.x1, l.y0, l.y1);
        }
    } else if (l.tile) {
        hipLaunchKernelGGL(tracer_tile<NT>, dim3(l.p.grid), dim3(64 * l.p.tpb), 0, l.st, a, l.ld, l.x0, l.x1, l.y0, l.y1,
                           l.p.c_first, l.p.nxw);
    } else {
        hipLaunchKernelGGL(tracer_direct<NT>, dim3(g.x, g.y), dim3(256), 0, l.st, a, l.ld, l.x0, l.x1, l.y0, l.y1);
    }
}

} // namespace

// every refusal of DESIGN.md section 6.10, before anything is launched (the four tracer entries)
int nemo::tracer_check(const char *who, int ld, int ny, int xstart, int xstop, int ystart, int ystop, const TracerFields &f,
                       const double *const *c_in, double *const *c_out, int ntracers)
{
    DLESM_REQUIRE(ntracers >= 1 && ntracers <= DLESM_TRACER_MAX, "%s: %d tracers (1..%d)", who, ntracers, DLESM_TRACER_MAX);
    const double *const ins[10] = {f.area_t, f.un, f.vn, f.hu, f.hv, f.ht, f.sshn_t, f.sshn_u, f.sshn_v, f.ssha};
    static const char *const in_name[10] = {"area_t", "un", "vn", "hu", "hv", "ht", "sshn_t", "sshn_u", "sshn_v", "ssha"};
    DLESM_REQUIRE(f.tmask, "%s: null tmask", who);
    for (int k = 0; k < 10; k++) DLESM_REQUIRE(ins[k], "%s: null %s", who, in_name[k]);
    DLESM_REQUIRE(c_in && c_out, "%s: null tracer pointer array", who);
    for (int k = 0; k < ntracers; k++) DLESM_REQUIRE(c_in[k] && c_out[k], "%s: null pointer of tracer %d", who, k);
    if (!(xstop < xstart || ystop < ystart))
        if (int rc = check_box(who, ld, ny, xstart, xstop, ystart, ystop, 1)) return rc;
    DLESM_REQUIRE(ld >= 1 && ny >= 1, "%s: array extents %dx%d", who, ld, ny);
    const size_t nb = (size_t)ld * (size_t)ny * sizeof(double);
    for (int k = 0; k < ntracers; k++) {
        DLESM_REQUIRE(!overlap(c_out[k], nb, f.tmask, nb / 2), "%s: c_out[%d] overlaps tmask", who, k);
        for (int m = 0; m < 10; m++)
            DLESM_REQUIRE(!overlap(c_out[k], nb, ins[m], nb), "%s: c_out[%d] overlaps the input %s", who, k, in_name[m]);
        for (int m = 0; m < ntracers; m++)
            DLESM_REQUIRE(!overlap(c_out[k], nb, c_in[m], nb), "%s: c_out[%d] overlaps c_in[%d]", who, k, m);
        for (int m = k + 1; m < ntracers; m++)
            DLESM_REQUIRE(!overlap(c_out[k], nb, c_out[m], nb), "%s: c_out[%d] and c_out[%d] overlap", who, k, m);
    }
    return DLESM_OK;
}

} // namespace dlesm

using namespace dlesm;

namespace {

// the body of the three single-domain entries: the refusals, the path, at most NT_MAX tracers per launch
int tracer_step(const char *who, Scheme scheme, double rdt, int ld, int ny, int xstart, int xstop, int ystart, int ystop,
                const TracerFields &f, const double *const *c_in, double *const *c_out, int ntracers, void *stream)
{
    if (int rc = ensure_device()) return rc;
    if (int rc = tracer_check(who, ld, ny, xstart, xstop, ystart, ystop, f, c_in, c_out, ntracers)) return rc;
    if (xstop < xstart || ystop < ystart) return DLESM_OK;   // empty box: a zero-trip loop nest

    const bool aligned = lanes16_fit(ld, f.tmask, {f.area_t, f.un, f.vn, f.hu, f.hv, f.ht, f.sshn_t, f.sshn_u, f.sshn_v, f.ssha}) &&
                         lanes16_fit(ld, nullptr, c_in, ntracers) && lanes16_fit(ld, nullptr, c_out, ntracers);

    Launch l{};
    static const char *const hook[3] = {"tracer_kernel", "tracer_muscl_kernel", "tracer_hancock_kernel"};
    l.scheme = scheme;
    l.tile = aligned && tuning(hook[scheme], 0) == 0;
    l.ld = ld, l.ny = ny, l.x0 = xstart - 1, l.x1 = xstop - 1, l.y0 = ystart - 1, l.y1 = ystop - 1;
    l.st = (hipStream_t)stream;
    if (l.tile) {
        const int chunks = scheme != SCHEME_UPWIND ? MUSCL_CHUNKS : TILE_CHUNKS;
        if (int rc = tile_plan(who, ld, l.x0, l.x1, l.y0, l.y1, chunks, 1, SHAPE_FOUR, 4, &l.p)) return rc;   // __launch_bounds__(256)
    }
    // at most NT_MAX tracers per launch: 5..8 tracers are two launches, each loading the flow once
    for (int k = 0; k < ntracers; k += NT_MAX) {
        switch (ntracers - k < NT_MAX ? ntracers - k : NT_MAX) {
        case 1: launch<1>(l, rdt, f, c_in + k, c_out + k); break;
        case 2: launch<2>(l, rdt, f, c_in + k, c_out + k); break;
        case 3: launch<3>(l, rdt, f, c_in + k, c_out + k); break;
        default: launch<4>(l, rdt, f, c_in + k, c_out + k); break;
        }
        DLESM_HIP_TRY(hipGetLastError());
    }
    return DLESM_OK;
}

} // namespace

extern "C" int dlesm_tracer_step_f64(double rdt, int ld, int ny, int xstart, int xstop, int ystart, int ystop,
                                     const int *tmask, const double *area_t, const double *un, const double *vn,
                                     const double *hu, const double *hv, const double *ht, const double *sshn_t,
                                     const double *sshn_u, const double *sshn_v, const double *ssha,
                                     const double *const *c_in, double *const *c_out, int ntracers, void *stream)
{
    const TracerFields f{tmask, area_t, un, vn, hu, hv, ht, sshn_t, sshn_u, sshn_v, ssha};
    return tracer_step("dlesm_tracer_step_f64", SCHEME_UPWIND, rdt, ld, ny, xstart, xstop, ystart, ystop, f, c_in, c_out,
                       ntracers, stream);
}

extern "C" int dlesm_tracer_step_muscl_f64(double rdt, int ld, int ny, int xstart, int xstop, int ystart, int ystop,
                                           const int *tmask, const double *area_t, const double *un, const double *vn,
                                           const double *hu, const double *hv, const double *ht, const double *sshn_t,
                                           const double *sshn_u, const double *sshn_v, const double *ssha,
                                           const double *const *c_in, double *const *c_out, int ntracers, void *stream)
{
    const TracerFields f{tmask, area_t, un, vn, hu, hv, ht, sshn_t, sshn_u, sshn_v, ssha};
    return tracer_step("dlesm_tracer_step_muscl_f64", SCHEME_MUSCL, rdt, ld, ny, xstart, xstop, ystart, ystop, f, c_in, c_out,
                       ntracers, stream);
}

extern "C" int dlesm_tracer_step_hancock_f64(double rdt, int ld, int ny, int xstart, int xstop, int ystart, int ystop,
                                             const int *tmask, const double *area_t, const double *un, const double *vn,
                                             const double *hu, const double *hv, const double *ht, const double *sshn_t,
                                             const double *sshn_u, const double *sshn_v, const double *ssha,
                                             const double *const *c_in, double *const *c_out, int ntracers, void *stream)
{
    const TracerFields f{tmask, area_t, un, vn, hu, hv, ht, sshn_t, sshn_u, sshn_v, ssha};
    return tracer_step("dlesm_tracer_step_hancock_f64", SCHEME_HANCOCK, rdt, ld, ny, xstart, xstop, ystart, ystop, f, c_in, c_out,
                       ntracers, stream);
}
