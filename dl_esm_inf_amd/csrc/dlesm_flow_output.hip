// The model's output fields: one sweep over the level-n flow that writes, in every wet T cell of a
// box, up to six T-point fields -- the sea-surface height, the velocities brought to the T point through section 6.10's face
// switches, their speed, the kinetic energy of the column and the relative vorticity at the cell's NE corner (stored only
// where the three neighbours east, north and north-east are not land) -- either as they are (DLESM_OUT_SET) or added with a
// weight to what the arrays hold (DLESM_OUT_ADD, a time mean).  The point rule is flow_output_point (dlesm_nemolite.h); sqrt
// and the two divisions are the compiler's correctly rounded f64 ones, as in dlesm_flow_courant.hip.
//
// flow_output_tile<VORT, ADD>: tracer_tile's wave shape (dlesm_tracer.hip) -- 64 lanes x 2 columns x 1 row in 16-byte lanes,
// un and the mask at i-1 / i+1 (and, for VORT, vn, dx_v and the mask of row j+1 at i+1) from the neighbouring lane by a DPP
// wave shift, lane 0 fetches the column west of the wave without a branch, lane 63 only loads, waves step by 63 chunks.  A
// wave that owns no wet cell of the box leaves after its mask row (one ballot).  Which outputs are wanted is the same for the
// whole launch: the six pointers are kernel arguments, tested by scalar branches; an array that no wanted output reads is not
// loaded (ht: KE; sshn_t: SSH, KE).  Row j+1 of un and dy_u, dx_v and the north-east mask are read by the VORT instantiations
// alone, the outputs' old content by the ADD ones.  Stores are plain predicated vector stores.
//
// flow_output_direct<VORT, ADD>: one cell per thread -- odd leading dimensions, unaligned bases and the HOOK key
// flow_output_kernel = 1.
#include <cmath>

#include "dlesm_nemolite.h"

namespace dlesm {

namespace {

typedef double d2 __attribute__((ext_vector_type(2)));
typedef int i2 __attribute__((ext_vector_type(2)));

using namespace nemo;

constexpr int TILE_CHUNKS = CHUNKS_EAST;      // chunks (2 columns) a wave owns; lane 63 only loads
constexpr int NOUT = DLESM_OUT_COUNT;

struct OutArgs {
    const int *tmask;
    const double *dx_v, *dy_u, *un, *vn, *ht, *sshn_t;
    double *out[NOUT];                // null: not wanted
    double weight;
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

// (x0:x1, y0:y1) = the box (0-based); nxw tiles per row, tile 0 begins at chunk c_first
template <bool VORT, bool ADD>
__global__ __launch_bounds__(256) void flow_output_tile(const OutArgs a, int ld, int x0, int x1, int y0, int y1, int c_first,
                                                        int nxw)
{
    const int lane = threadIdx.x & 63;
    const long long w = (long long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    const int xw = (int)(w % nxw);
    const long long j = y0 + w / nxw;
    if (j > y1) return;
    const int c = c_first + xw * TILE_CHUNKS + lane;     // this lane's chunk (2 columns); lane 63 = the next wave's lane 0
    if (c - lane > x1 / 2) return;                       // idle padding tile
    const int c_ld = ld / 2 - 1, cl = c < c_ld ? c : c_ld;
    const bool own = lane != 63;                         // lane 63 only loads: its chunk is the east column of lane 62
    const bool m0 = own && c * 2 >= x0 && c * 2 <= x1, m1 = own && c * 2 + 1 >= x0 && c * 2 + 1 <= x1;
    const size_t row = (size_t)j * ld, o = row + (size_t)cl * 2, os = o - ld, on = o + ld;

    // the land exit: the mask of the row first; a wave that owns no wet cell of the box stores nothing
    const i2 t = *(const i2 *)(a.tmask + o);
    const bool wet0 = m0 && t.x > 0, wet1 = m1 && t.y > 0;
    if (__ballot(wet0 || wet1) == 0) return;

    // the west column this wave cannot get from a lane (no branch, LAB_NOTES.md section 5.10)
    const size_t ow = row + (size_t)((lane == 0 && m0) ? c * 2 - 1 : cl * 2);
    const i2 ts = *(const i2 *)(a.tmask + os), tn = *(const i2 *)(a.tmask + on);
    int tw = a.tmask[ow];
    const d2 un = *(const d2 *)(a.un + o), vn = *(const d2 *)(a.vn + o), vn_s = *(const d2 *)(a.vn + os);
    double un_w = a.un[ow];
    d2 st{0.0, 0.0}, ht{0.0, 0.0};
    if (a.out[DLESM_OUT_SSH] || a.out[DLESM_OUT_KE]) st = *(const d2 *)(a.sshn_t + o);
    if (a.out[DLESM_OUT_KE]) ht = *(const d2 *)(a.ht + o);
    d2 un_n{0.0, 0.0}, dxv{0.0, 0.0}, dyu{0.0, 0.0}, dyu_n{0.0, 0.0};
    if constexpr (VORT) {
        un_n = *(const d2 *)(a.un + on);
        dxv = *(const d2 *)(a.dx_v + o);
        dyu = *(const d2 *)(a.dy_u + o), dyu_n = *(const d2 *)(a.dy_u + on);
    }
    d2 old[NOUT];
#pragma unroll
    for (int k = 0; k < NOUT; k++) {
        old[k] = d2{0.0, 0.0};
        if constexpr (ADD)
            if ((VORT || k != DLESM_OUT_VORT) && a.out[k]) old[k] = *(const d2 *)(a.out[k] + o);
    }

    {
        const double u1 = from_lower<true>(un.y);
        const int t1 = __builtin_amdgcn_mov_dpp(t.y, 0x138, 0xf, 0xf, true);
        if (lane != 0) un_w = u1, tw = t1;
    }
    const int te = __builtin_amdgcn_mov_dpp(t.x, 0x130, 0xf, 0xf, true);      // (lane 63: 0, never used)
    double v_e = 0.0, dxv_e = 0.0;
    int tne = 0;
    if constexpr (VORT) {
        v_e = from_upper<true>(vn.x), dxv_e = from_upper<true>(dxv.x);
        tne = __builtin_amdgcn_mov_dpp(tn.x, 0x130, 0xf, 0xf, true);
    }
    const FlowOutput r0 = flow_output_point<VORT>(un.x, un_w, vn.x, vn_s.x, vn.y, un_n.x, ht.x, st.x, dxv.x, dxv.y, dyu.x,
                                                  dyu_n.x, t.y, tw, tn.x, ts.x, tn.y);
    const FlowOutput r1 = flow_output_point<VORT>(un.y, un.x, vn.y, vn_s.y, v_e, un_n.y, ht.y, st.y, dxv.y, dxv_e, dyu.y,
                                                  dyu_n.y, te, t.x, tn.y, ts.y, tne);

    const size_t oc = row + (size_t)c * 2;
#pragma unroll
    for (int k = 0; k < NOUT; k++) {
        if (!VORT && k == DLESM_OUT_VORT) continue;
        if (!a.out[k]) continue;
        const bool w0 = wet0 && (k != DLESM_OUT_VORT || r0.corner), w1 = wet1 && (k != DLESM_OUT_VORT || r1.corner);
        double y0v = r0.v[k], y1v = r1.v[k];
        if constexpr (ADD) y0v = old[k].x + a.weight * y0v, y1v = old[k].y + a.weight * y1v;
        store_pair(a.out[k] + oc, y0v, y1v, w0, w1);
    }
}

// one cell per thread: odd leading dimensions, unaligned bases, the HOOK key flow_output_kernel.  A thread walks its column
// by rows y0 + blockIdx.y, + gridDim.y, ...
template <bool VORT, bool ADD>
__global__ __launch_bounds__(256) void flow_output_direct(const OutArgs a, int ld, int x0, int x1, int y0, int y1)
{
    const int i = x0 + blockIdx.x * blockDim.x + threadIdx.x;
    if (i > x1) return;
    for (long long j = (long long)y0 + blockIdx.y; j <= y1; j += gridDim.y) {
        const size_t o = (size_t)j * ld + i;
        if (a.tmask[o] <= 0) continue;
        const double st = (a.out[DLESM_OUT_SSH] || a.out[DLESM_OUT_KE]) ? a.sshn_t[o] : 0.0;
        const double ht = a.out[DLESM_OUT_KE] ? a.ht[o] : 0.0;
        double v_e = 0.0, u_n = 0.0, dxv = 0.0, dxv_e = 0.0, dyu = 0.0, dyu_n = 0.0;
        int tne = 0;
        if constexpr (VORT) {
            v_e = a.vn[o + 1], u_n = a.un[o + ld];
            dxv = a.dx_v[o], dxv_e = a.dx_v[o + 1], dyu = a.dy_u[o], dyu_n = a.dy_u[o + ld];
            tne = a.tmask[o + ld + 1];
        }
        const FlowOutput r = flow_output_point<VORT>(a.un[o], a.un[o - 1], a.vn[o], a.vn[o - ld], v_e, u_n, ht, st, dxv,
                                                     dxv_e, dyu, dyu_n, a.tmask[o + 1], a.tmask[o - 1], a.tmask[o + ld],
                                                     a.tmask[o - ld], tne);
#pragma unroll
        for (int k = 0; k < NOUT; k++) {
            if (!VORT && k == DLESM_OUT_VORT) continue;
            if (!a.out[k] || (k == DLESM_OUT_VORT && !r.corner)) continue;
            if constexpr (ADD) a.out[k][o] = a.out[k][o] + a.weight * r.v[k];
            else a.out[k][o] = r.v[k];
        }
    }
}

template <bool VORT, bool ADD>
int launch(bool tile, const OutArgs &a, int ld, int x0, int x1, int y0, int y1, hipStream_t s)
{
    if (tile) {
        TilePlan p;                                      // (4 waves: __launch_bounds__(256))
        if (int rc = tile_plan("dlesm_flow_output_f64", ld, x0, x1, y0, y1, TILE_CHUNKS, 1, SHAPE_FOUR, 4, &p)) return rc;
        hipLaunchKernelGGL((flow_output_tile<VORT, ADD>), dim3(p.grid), dim3(64 * p.tpb), 0, s, a, ld, x0, x1, y0, y1, p.c_first, p.nxw);
    } else {
        const DirectGrid g = direct_grid(x0, x1, y0, y1);
        hipLaunchKernelGGL((flow_output_direct<VORT, ADD>), dim3(g.x, g.y), dim3(256), 0, s, a, ld, x0, x1, y0, y1);
    }
    return DLESM_OK;
}

} // namespace

} // namespace dlesm

using namespace dlesm;

extern "C" int dlesm_flow_output_f64(int mode, double weight, int ld, int ny, int xstart, int xstop, int ystart, int ystop,
                                     const int *tmask, const double *dx_v, const double *dy_u, const double *un,
                                     const double *vn, const double *ht, const double *sshn_t, double *const *out,
                                     void *stream)
{
    static const char *const who = "dlesm_flow_output_f64";
    static const char *const out_name[NOUT] = {"SSH", "UT", "VT", "SPEED", "KE", "VORT"};
    static const char *const in_name[6] = {"dx_v", "dy_u", "un", "vn", "ht", "sshn_t"};
    if (int rc = ensure_device()) return rc;
    DLESM_REQUIRE(mode == DLESM_OUT_SET || mode == DLESM_OUT_ADD, "%s: mode %d (DLESM_OUT_SET or DLESM_OUT_ADD)", who, mode);
    DLESM_REQUIRE(mode == DLESM_OUT_SET || std::isfinite(weight), "%s: weight %g (a finite number)", who, weight);
    DLESM_REQUIRE(out != nullptr, "%s: null out", who);
    bool any = false;
    for (int k = 0; k < NOUT; k++) any = any || out[k] != nullptr;
    DLESM_REQUIRE(any, "%s: every out entry is null", who);
    const bool vort = out[DLESM_OUT_VORT] != nullptr, ke = out[DLESM_OUT_KE] != nullptr;
    const bool ssh = out[DLESM_OUT_SSH] != nullptr;
    // an array that no wanted output reads is not read: it may be null (one that is given must still not hold an output)
    const bool need[6] = {vort, vort, true, true, ke, ssh || ke};
    const double *const ins[6] = {dx_v, dy_u, un, vn, ht, sshn_t};
    DLESM_REQUIRE(tmask != nullptr, "%s: null tmask", who);
    DLESM_REQUIRE((uintptr_t)tmask % 4 == 0, "%s: tmask is not 4-byte aligned", who);
    for (int m = 0; m < 6; m++) {
        if (!need[m]) continue;
        DLESM_REQUIRE(ins[m] != nullptr, "%s: null %s", who, in_name[m]);
        DLESM_REQUIRE((uintptr_t)ins[m] % 8 == 0, "%s: %s is not 8-byte aligned", who, in_name[m]);
    }
    for (int k = 0; k < NOUT; k++)
        DLESM_REQUIRE((uintptr_t)out[k] % 8 == 0, "%s: out[%s] is not 8-byte aligned", who, out_name[k]);
    DLESM_REQUIRE(ld >= 1 && ny >= 1, "%s: array extents %dx%d", who, ld, ny);
    const bool empty = xstop < xstart || ystop < ystart;
    if (!empty)
        if (int rc = check_box(who, ld, ny, xstart, xstop, ystart, ystop, 1)) return rc;
    const size_t nb = (size_t)ld * (size_t)ny * sizeof(double);
    for (int k = 0; k < NOUT; k++) {
        if (!out[k]) continue;
        DLESM_REQUIRE(!overlap(out[k], nb, tmask, nb / 2), "%s: out[%s] overlaps tmask", who, out_name[k]);
        for (int m = 0; m < 6; m++)
            DLESM_REQUIRE(!ins[m] || !overlap(out[k], nb, ins[m], nb), "%s: out[%s] overlaps the input %s", who, out_name[k],
                          in_name[m]);
        for (int m = k + 1; m < NOUT; m++)
            DLESM_REQUIRE(!out[m] || !overlap(out[k], nb, out[m], nb), "%s: out[%s] and out[%s] overlap", who, out_name[k],
                          out_name[m]);
    }
    if (empty) return DLESM_OK;                          // a zero-trip loop nest

    OutArgs a{tmask, need[0] ? dx_v : nullptr, need[1] ? dy_u : nullptr, un, vn, need[4] ? ht : nullptr,
              need[5] ? sshn_t : nullptr, {}, mode == DLESM_OUT_ADD ? weight : 0.0};
    for (int k = 0; k < NOUT; k++) a.out[k] = out[k];
    const bool tile = lanes16_fit(ld, tmask, {a.dx_v, a.dy_u, a.un, a.vn, a.ht, a.sshn_t}) && lanes16_fit(ld, nullptr, out, NOUT) &&
                      tuning("flow_output_kernel", 0) == 0;

    const int x0 = xstart - 1, x1 = xstop - 1, y0 = ystart - 1, y1 = ystop - 1;
    const hipStream_t s = (hipStream_t)stream;
    int rc;
    switch ((vort ? 2 : 0) | (mode == DLESM_OUT_ADD ? 1 : 0)) {
    case 0: rc = launch<false, false>(tile, a, ld, x0, x1, y0, y1, s); break;
    case 1: rc = launch<false, true>(tile, a, ld, x0, x1, y0, y1, s); break;
    case 2: rc = launch<true, false>(tile, a, ld, x0, x1, y0, y1, s); break;
    default: rc = launch<true, true>(tile, a, ld, x0, x1, y0, y1, s); break;
    }
    if (rc) return rc;
    DLESM_HIP_TRY(hipGetLastError());
    return DLESM_OK;
}
