// One NEMOLite2D-class time step in one call: continuity, next_sshu, next_sshv, the fused momentum
// update and, with an open-boundary plan, bc_open -- bit for bit the five entries run in that order.
//
// nemolite_step_tile: ONE wave-tile sweep for the first four, when the T, U and V boxes are one box B (every NE grid) and
// the arrays meet the 16-byte lane conditions.  momentum_tile's shape (dlesm_momentum.hip) -- 64 lanes x 2 columns x 1 row,
// operands at i-1 / i+1 from the neighbouring lane by a DPP wave shift, lane 0 fetches the column west of the wave without
// a branch, rows j-1 / j+1 loaded -- except at the east end: lane 63 only loads (its chunk is the next wave's lane 0), so
// lane 62 takes its east column from it by DPP and no lane loads an east edge column.  Waves step by 63 chunks.  The edge
// loads of the 64-lane form (lane 63 as in momentum_tile) held 256 VGPRs + 14 AGPRs, one wave per SIMD; this form holds 250
// VGPRs, two waves per SIMD, no scratch (LAB_NOTES.md section 5.14).  The tile evaluates ssha with continuity's expression
// on its row (columns c*2 .. c*2+2; c*2+2 from the next lane by DPP) and on the row above (c*2, c*2+1) --
// a cell another tile also stores, recomputed from the same operands with the same expression tree, so the bits are the
// stored ones -- then ssha_u and ssha_v with next_ssh's, then ua and va with
// momentum's, which read the ssha_u / ssha_v values the tile stores.  ssha of a cell outside B (the east column and the
// north row of the ring) is the caller's: loaded from memory, only there; inside B ssha is never read.  Mixed pairs store
// per column, as in momentum.  19 double streams and the mask read, five written: 196 B/cell against 324 B/cell for the
// five launches.
//
// Everything else -- boxes that differ, odd leading dimensions, unaligned bases, the HOOK key nemo_step_kernel -- runs the
// definition: the five entries in order on the caller's stream.  The open-boundary pass is always obc_apply's own launch
// behind the sweep (O(perimeter) cells).
//
// Land: a wet plan (dlesm_wet_plan) marks the wave tiles in which the sweep would store nothing but
// ssha on T == 0 cells; dlesm_nemolite_step_wet_f64 runs the same tile body on the others only -- one bit per tile read on a
// wave-uniform address in today's launch, trimmed to the rows that hold an active tile (the flag map), or a grid of the
// active tiles alone, each wave taking its tile from a row-major list (HOOK key nemo_wet_form = 1).  The plan and the
// launcher take the tile geometry from dlesm_tile_plan.h, the one place it is written.
#include <climits>
#include <vector>

#include "dlesm_nemolite.h"

// the wet plan: which wave tiles of the sweep over `box` store anything but land ssha
struct dlesm_wet_plan {
    int ld, ny;
    dlesm_region box;         // the box it was made for (1-based inclusive, as given)
    int c_first, chunks, nxt; // the tile geometry it was made for (tile_geometry)
    long long tiles, active;
    int row_lo, row_hi;       // the first and last row (0-based, relative to the box) that holds an active tile
    unsigned *bits;           // HBM: one bit per tile, row-major, tile t in word t / 32; NULL when tiles == 0
    int *list;                // HBM: the active tiles, row-major; NULL when active == 0
};


namespace dlesm {

namespace {

typedef double d2 __attribute__((ext_vector_type(2)));
typedef int i2 __attribute__((ext_vector_type(2)));

using namespace nemo;

// chunks (2 columns) a wave tile owns; the kernel, its launcher and the wet plan take the geometry from dlesm_tile_plan.h
constexpr int TILE_CHUNKS = CHUNKS_EAST;

// how a launch finds its tiles: FULL = every tile of the box (today's sweep), FLAGS = every tile of rows y0 .. that has its
// bit set, LIST = the tiles of a list
enum { FULL = 0, FLAGS = 1, LIST = 2 };
struct WetArgs {
    const unsigned *bits;     // FLAGS: the plan's bit map; bit0 = the number of the first tile of row y0
    const int *list;          // LIST: the plan's list of n tiles
    long long bit0;
    int nxt, n;
};

enum { AT = NF, NS };   // area_t: the one operand the step reads beyond momentum's

// the operands the tile loads: momentum's less ssha_u / ssha_v (evaluated in the tile), and area_t
__host__ __device__ constexpr bool loaded(int f) { return f != SAU && f != SAV; }

struct StepArgs {
    MomArgs m;                                // m.f[SAU] and m.f[SAV] are unused
    const double *area_t;
    double *ssha, *ssha_u, *ssha_v;
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

// (x0:x1, y0:y1) = the box B (0-based).  WET = FLAGS: y0 is the first row of the launch, a tile whose bit is clear returns;
// WET = LIST: wave w takes tile wa.list[w], rows counted from y0.  The tile's coordinates are wave-uniform, so the look-up is
// a scalar load.
template <int WET>
__global__ __launch_bounds__(256) void nemolite_step_tile(StepArgs s, int ld, int x0, int x1, int y0, int y1, int c_first,
                                                          int nxw, WetArgs wa)
{
    const MomArgs &a = s.m;
    const int lane = threadIdx.x & 63;
    int w;
    if constexpr (WET == FULL) w = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    else w = blockIdx.x * (blockDim.x >> 6) + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if constexpr (WET == LIST) {
        if (w >= wa.n) return;
        w = wa.list[w];
        nxw = wa.nxt;
    }
    const int xw = w % nxw, j = y0 + w / nxw;
    if (j > y1) return;
    const int c = c_first + xw * TILE_CHUNKS + lane;     // this lane's chunk (2 columns); lane 63 = the next wave's lane 0
    if (c - lane > x1 / 2) return;                       // idle padding tile
    if constexpr (WET == FLAGS) {
        const long long t = wa.bit0 + (long long)(w / nxw) * wa.nxt + xw;
        if (!((wa.bits[t >> 5] >> (t & 31)) & 1u)) return;   // nothing but land ssha would be stored here
    }
    const int c_ld = ld / 2 - 1, cl = c < c_ld ? c : c_ld;
    const bool own = lane != 63;                         // lane 63 only loads: its chunk is the east column of lane 62
    const bool m0 = own && c * 2 >= x0 && c * 2 <= x1, m1 = own && c * 2 + 1 >= x0 && c * 2 + 1 <= x1;
    // the west column this wave cannot get from a lane (no branch, LAB_NOTES.md section 5.10)
    const int wcol = (lane == 0 && m0) ? c * 2 - 1 : cl * 2;

    // rows j-1 .. j+1, columns c*2-1 .. c*2+2
    double v[NS][3][4];
    int t[3][4];
#pragma unroll
    for (int r = 0; r < 3; r++) {
        const size_t row = (size_t)(j - 1 + r) * ld, o = row + (size_t)cl * 2;
#pragma unroll
        for (int f = 0; f < NS; f++) {
            if (!loaded(f)) continue;
            const double *p = f == AT ? s.area_t : a.f[f];
            const d2 q = *(const d2 *)(p + o);
            v[f][r][0] = p[row + wcol];
            v[f][r][1] = q.x;
            v[f][r][2] = q.y;
        }
        const i2 q = *(const i2 *)(a.tmask + o);
        t[r][0] = a.tmask[row + wcol];
        t[r][1] = q.x;
        t[r][2] = q.y;
    }
#pragma unroll
    for (int r = 0; r < 3; r++) {
#pragma unroll
        for (int f = 0; f < NS; f++) {
            if (!loaded(f)) continue;
            const double wl = from_lower<true>(v[f][r][2]);
            if (lane != 0) v[f][r][0] = wl;
            v[f][r][3] = from_upper<true>(v[f][r][1]);   // (lane 63: 0.0, never used)
        }
        const int wl = __builtin_amdgcn_mov_dpp(t[r][2], 0x138, 0xf, 0xf, true);
        if (lane != 0) t[r][0] = wl;
        t[r][3] = __builtin_amdgcn_mov_dpp(t[r][1], 0x130, 0xf, 0xf, true);
    }

    // ssha: e[0][k] at (c*2+k, j), e[1][k] at (c*2+k, j+1).  Continuity's expression inside B; in the ring the caller's
    // value, loaded only where a face of B reads it.
    auto cont = [&](int r, int k) {
        return cont_point(a.rdt, v[SST][r][k], v[SSU][r][k], v[SSU][r][k - 1], v[SSV][r][k], v[SSV][r - 1][k], v[HU][r][k],
                          v[HU][r][k - 1], v[HV][r][k], v[HV][r - 1][k], v[UN][r][k], v[UN][r][k - 1], v[VN][r][k],
                          v[VN][r - 1][k], v[AT][r][k]);
    };
    const size_t oj = (size_t)j * ld + (size_t)c * 2, on = oj + ld;
    double e[2][3];
    e[0][0] = cont(1, 1);
    e[0][1] = cont(1, 2);
    e[0][2] = from_upper<true>(e[0][0]);                 // (c*2+2, j): the next lane's
    e[1][0] = cont(2, 1);
    e[1][1] = cont(2, 2);
    e[1][2] = 0.0;                                       // (never read)
    if (m0 && !m1) e[0][1] = s.ssha[oj + 1];             // c*2 = x1: its u face reads ssha(x1+1, j)
    if (m1 && c * 2 + 2 > x1) e[0][2] = s.ssha[oj + 2];  // c*2+1 = x1
    if (j == y1) {                                       // the v faces of the last row read ssha(i, y1+1)
        if (m0) e[1][0] = s.ssha[on];
        if (m1) e[1][1] = s.ssha[on + 1];
    }

    double su[2], sv[2], ou[2], ov[2];
    bool wsu[2], wsv[2], wu[2], wv[2];
#pragma unroll
    for (int q = 0; q < 2; q++) {
        const bool in = q ? m1 : m0;
        const long long t0 = t[1][q + 1], tu = t[1][q + 2], tv = t[2][q + 1];
        su[q] = ssh_point(t0, tu, v[AT][1][q + 1], v[AT][1][q + 2], e[0][q], e[0][q + 1], v[AU][1][q + 1]);
        sv[q] = ssh_point(t0, tv, v[AT][1][q + 1], v[AT][2][q + 1], e[0][q], e[1][q], v[AV][1][q + 1]);
        wsu[q] = in && t0 + tu > 0;
        wsv[q] = in && t0 + tv > 0;
        auto X = [&](int f, int di, int dj) { return f == SAU ? su[q] : f == SAV ? sv[q] : v[f][1 + dj][q + 1 + di]; };
        auto T = [&](int di, int dj) { return t[1 + dj][q + 1 + di]; };
        ou[q] = mom_u(a, X, T);
        ov[q] = mom_v(a, X, T);
        wu[q] = in && T(0, 0) > 0 && T(1, 0) > 0;
        wv[q] = in && T(0, 0) > 0 && T(0, 1) > 0;
    }
    store_pair(s.ssha + oj, e[0][0], e[0][1], m0, m1);
    store_pair(s.ssha_u + oj, su[0], su[1], wsu[0], wsu[1]);
    store_pair(s.ssha_v + oj, sv[0], sv[1], wsv[0], wsv[1]);
    store_pair(a.ua + oj, ou[0], ou[1], wu[0], wu[1]);
    store_pair(a.va + oj, ov[0], ov[1], wv[0], wv[1]);
}

} // namespace

// every refusal of DESIGN.md section 6.7, before anything is launched (dlesm_nemolite_step_f64, dlesm_nemolite_step_dm)
int nemo::step_check(const char *who, const dlesm_momentum_params *params, const dlesm_momentum_grid *grid,
                     const double *area_t, int ld, int ny, const dlesm_region *tbox, const dlesm_region *ubox,
                     const dlesm_region *vbox, const dlesm_obc *obc, const double *un, const double *vn, const double *ht,
                     const double *hu, const double *hv, const double *sshn_t, const double *sshn_u, const double *sshn_v,
                     double *ssha, double *ssha_u, double *ssha_v, double *ua, double *va)
{
    DLESM_REQUIRE(params && grid && tbox && ubox && vbox, "%s: null parameter, grid or region pointer", who);
    for (const dlesm_region *r : {tbox, ubox, vbox})
        if (!empty(r))
            if (int rc = check_box(who, ld, ny, r->xstart, r->xstop, r->ystart, r->ystop, 1)) return rc;

    // every input of the five entries, every output
    const double *const ins[19] = {un, vn, ht, hu, hv, sshn_t, sshn_u, sshn_v, area_t, grid->dx_t, grid->dy_t, grid->dx_u,
                                   grid->dy_u, grid->dx_v, grid->dy_v, grid->area_u, grid->area_v, grid->fcor_u,
                                   grid->fcor_v};
    static const char *const in_name[19] = {"un", "vn", "ht", "hu", "hv", "sshn_t", "sshn_u", "sshn_v", "area_t", "dx_t",
                                            "dy_t", "dx_u", "dy_u", "dx_v", "dy_v", "area_u", "area_v", "fcor_u", "fcor_v"};
    double *const outs[5] = {ssha, ssha_u, ssha_v, ua, va};
    static const char *const out_name[5] = {"ssha", "ssha_u", "ssha_v", "ua", "va"};
    DLESM_REQUIRE(grid->tmask, "%s: null tmask", who);
    for (int k = 0; k < 19; k++)
        DLESM_REQUIRE(ins[k], "%s: null %s%s", who, in_name[k],
                      k >= 17 ? ": the Coriolis parameter has not been set" : "");
    for (int k = 0; k < 5; k++) DLESM_REQUIRE(outs[k], "%s: null %s", who, out_name[k]);
    const size_t nb = (size_t)ld * (size_t)ny * sizeof(double);
    for (int k = 0; k < 5; k++) {
        DLESM_REQUIRE(!overlap(outs[k], nb, grid->tmask, nb / 2), "%s: %s overlaps tmask", who, out_name[k]);
        for (int m = 0; m < 19; m++)
            DLESM_REQUIRE(!overlap(outs[k], nb, ins[m], nb), "%s: %s overlaps the input %s", who, out_name[k], in_name[m]);
        for (int m = k + 1; m < 5; m++)
            DLESM_REQUIRE(!overlap(outs[k], nb, outs[m], nb), "%s: the outputs %s and %s overlap", who, out_name[k],
                          out_name[m]);
    }
    DLESM_REQUIRE(!obc || (obc->ld == ld && obc->ny == ny), "%s: the open-boundary plan was made for %dx%d arrays, not %dx%d",
                  who, obc ? obc->ld : 0, obc ? obc->ny : 0, ld, ny);
    return DLESM_OK;
}

// the refusals of a wet plan: made for other extents, for a box other than tbox, or for another
// tile geometry than the sweep's.  A null plan is no plan.
int nemo::wet_check(const char *who, const dlesm_wet_plan *wet, int ld, int ny, const dlesm_region *tbox)
{
    if (!wet) return DLESM_OK;
    DLESM_REQUIRE(tbox, "%s: null region pointer", who);
    DLESM_REQUIRE(wet->ld == ld && wet->ny == ny, "%s: the wet plan was made for %dx%d arrays, not %dx%d", who, wet->ld,
                  wet->ny, ld, ny);
    DLESM_REQUIRE(same_box(&wet->box, tbox), "%s: the wet plan was made for the box (%d:%d,%d:%d), not tbox (%d:%d,%d:%d)", who,
                  wet->box.xstart, wet->box.xstop, wet->box.ystart, wet->box.ystop, tbox->xstart, tbox->xstop, tbox->ystart,
                  tbox->ystop);
    if (!empty(tbox)) {
        const TilePlan g = tile_geometry(tbox->xstart - 1, tbox->xstop - 1, tbox->ystart - 1, tbox->ystop - 1, TILE_CHUNKS, 1);
        DLESM_REQUIRE(wet->c_first == g.c_first && wet->chunks == TILE_CHUNKS && wet->nxt == g.nxt && wet->tiles == g.tiles(),
                      "%s: the wet plan was made for another tile geometry", who);
    }
    return DLESM_OK;
}

} // namespace dlesm

using namespace dlesm;

namespace {

// dlesm_nemolite_step_f64 (wet == NULL) and dlesm_nemolite_step_wet_f64
int step_impl(const char *who, const dlesm_wet_plan *wet, const dlesm_momentum_params *params, const dlesm_momentum_grid *grid,
              const double *area_t, int ld, int ny, const dlesm_region *tbox, const dlesm_region *ubox,
              const dlesm_region *vbox, const dlesm_obc *obc, double ssh_bc, const double *un, const double *vn,
              const double *ht, const double *hu, const double *hv, const double *sshn_t, const double *sshn_u,
              const double *sshn_v, double *ssha, double *ssha_u, double *ssha_v, double *ua, double *va, void *stream)
{
    if (int rc = ensure_device()) return rc;
    if (int rc = step_check(who, params, grid, area_t, ld, ny, tbox, ubox, vbox, obc, un, vn, ht, hu, hv, sshn_t, sshn_u,
                            sshn_v, ssha, ssha_u, ssha_v, ua, va))
        return rc;
    if (int rc = wet_check(who, wet, ld, ny, tbox)) return rc;
    const double *const ins[19] = {un, vn, ht, hu, hv, sshn_t, sshn_u, sshn_v, area_t, grid->dx_t, grid->dy_t, grid->dx_u,
                                   grid->dy_u, grid->dx_v, grid->dy_v, grid->area_u, grid->area_v, grid->fcor_u,
                                   grid->fcor_v};
    double *const outs[5] = {ssha, ssha_u, ssha_v, ua, va};

    const bool aligned = lanes16_fit(ld, grid->tmask, ins, 19) && lanes16_fit(ld, nullptr, outs, 5);
    hipStream_t st = (hipStream_t)stream;
    if (same_box(tbox, ubox) && same_box(tbox, vbox) && aligned && tuning("nemo_step_kernel", 0) == 0) {
        if (!empty(tbox)) {
            StepArgs s{};
            const double *const fld[NF] = {un, vn, ht, sshn_t, hu, sshn_u, hv, sshn_v, nullptr, nullptr, grid->dx_t,
                                           grid->dy_t, grid->dx_u, grid->dy_u, grid->dx_v, grid->dy_v, grid->area_u,
                                           grid->area_v, grid->fcor_u, grid->fcor_v};
            for (int f = 0; f < NF; f++) s.m.f[f] = fld[f];
            s.m.tmask = grid->tmask;
            s.m.ua = ua, s.m.va = va;
            s.m.rdt = params->rdt, s.m.visc = params->visc, s.m.g = params->g;
            s.m.den = 1.0 + params->cbfr * params->rdt;
            s.area_t = area_t, s.ssha = ssha, s.ssha_u = ssha_u, s.ssha_v = ssha_v;
            const int x0 = tbox->xstart - 1, x1 = tbox->xstop - 1, y0 = tbox->ystart - 1, y1 = tbox->ystop - 1;
            TilePlan g;
            if (int rc = tile_plan(who, ld, x0, x1, y0, y1, TILE_CHUNKS, 1, SHAPE_FOUR, 4, &g)) return rc;   // __launch_bounds__(256)
            unsigned nblk;
            if (!wet || wet->active == wet->tiles) {            // every tile: today's kernel, today's launch shape
                hipLaunchKernelGGL(nemolite_step_tile<FULL>, dim3(g.grid), dim3(64 * g.tpb), 0, st, s, ld, x0, x1, y0, y1, g.c_first,
                                   g.nxw, WetArgs{});
            } else if (wet->active == 0) {                      // all land: nothing to sweep
            } else if (tuning("nemo_wet_form", 0) == 1) {       // the compacted list: one wave per active tile
                const WetArgs wa{nullptr, wet->list, 0, g.nxt, (int)wet->active};
                if (int rc = sweep_grid(who, (wet->active + 3) / 4, &nblk)) return rc;
                hipLaunchKernelGGL(nemolite_step_tile<LIST>, dim3(nblk), dim3(256), 0, st, s, ld, x0, x1, y0, y1, g.c_first,
                                   g.nxt, wa);
            } else {                                            // the flag map: today's shape over the rows row_lo .. row_hi
                const WetArgs wa{wet->bits, nullptr, (long long)wet->row_lo * g.nxt, g.nxt, 0};
                if (int rc = sweep_grid(who, g.groups_for(wet->row_hi - wet->row_lo + 1), &nblk)) return rc;
                hipLaunchKernelGGL(nemolite_step_tile<FLAGS>, dim3(nblk), dim3(64 * g.tpb), 0, st, s, ld, x0, x1, y0 + wet->row_lo,
                                   y1, g.c_first, g.nxw, wa);
            }
            DLESM_HIP_TRY(hipGetLastError());
        }
    } else {
        // the definition
        if (int rc = dlesm_continuity_f64(params->rdt, ld, ny, tbox->xstart, tbox->xstop, tbox->ystart, tbox->ystop, sshn_t,
                                          sshn_u, sshn_v, hu, hv, un, vn, area_t, ssha, stream))
            return rc;
        if (int rc = dlesm_next_sshu_f64(ld, ny, ubox->xstart, ubox->xstop, ubox->ystart, ubox->ystop, grid->tmask, area_t,
                                         grid->area_u, ssha, ssha_u, stream))
            return rc;
        if (int rc = dlesm_next_sshv_f64(ld, ny, vbox->xstart, vbox->xstop, vbox->ystart, vbox->ystop, grid->tmask, area_t,
                                         grid->area_v, ssha, ssha_v, stream))
            return rc;
        if (int rc = dlesm_momentum_f64(params, grid, ld, ny, ubox, vbox, un, vn, ht, sshn_t, hu, sshn_u, hv, sshn_v, ssha_u,
                                        ssha_v, ua, va, stream))
            return rc;
    }
    if (obc) return dlesm_bc_open_f64(obc, params, ssh_bc, hu, sshn_u, hv, sshn_v, sshn_t, ssha, ua, va, stream);
    return DLESM_OK;
}

} // namespace

extern "C" int dlesm_wet_plan_create(const int *tmask_host, int ld, int ny, const dlesm_region *box, dlesm_wet_plan **out)
{
    static const char *who = "dlesm_wet_plan_create";
    DLESM_REQUIRE(out, "%s: null output pointer", who);
    *out = nullptr;
    DLESM_REQUIRE(tmask_host && box, "%s: null mask or region", who);
    DLESM_REQUIRE(ld >= 1 && ny >= 1, "%s: array extents %dx%d", who, ld, ny);
    dlesm_wet_plan *p = new dlesm_wet_plan{ld, ny, *box, 0, TILE_CHUNKS, 0, 0, 0, 0, -1, nullptr, nullptr};
    std::vector<unsigned> bits;
    std::vector<int> list;
    if (!empty(box)) {
        // the step's own condition on its boxes: a one-cell ring, so that T(i+1, j) and T(i, j+1) are inside the array
        if (int rc = check_box(who, ld, ny, box->xstart, box->xstop, box->ystart, box->ystop, 1)) {
            delete p;
            return rc;
        }
        const int x0 = box->xstart - 1, x1 = box->xstop - 1, y0 = box->ystart - 1, y1 = box->ystop - 1;
        const TilePlan g = tile_geometry(x0, x1, y0, y1, TILE_CHUNKS, 1);
        if (g.tiles() > INT_MAX) {
            delete p;
            return fail(DLESM_EINVAL, "%s: %lld tiles do not fit the plan's int32 tile index", who, g.tiles());
        }
        p->c_first = g.c_first, p->nxt = g.nxt, p->tiles = g.tiles();
        bits.assign((size_t)((p->tiles + 31) / 32), 0u);
        // One pass over the mask per tile row.  A tile is inactive only if the sweep would store nothing but ssha on T == 0
        // cells in it: no owned cell of the box has T(i,j) != 0, T(i+1,j) > 0 (its ssha_u is written) or T(i,j+1) > 0 (its
        // ssha_v is written).
        for (int j = y0; j <= y1; j++) {
            const int *t = tmask_host + (size_t)j * ld, *tn = t + ld;
            for (int xw = 0; xw < g.nxt; xw++) {
                const int lo = (g.c_first + xw * TILE_CHUNKS) * 2, hi = lo + 2 * TILE_CHUNKS - 1;
                bool on = false;
                for (int i = lo < x0 ? x0 : lo; i <= (hi > x1 ? x1 : hi) && !on; i++)
                    on = t[i] != 0 || t[i + 1] > 0 || tn[i] > 0;
                if (!on) continue;
                const long long k = (long long)(j - y0) * g.nxt + xw;
                bits[(size_t)(k >> 5)] |= 1u << (k & 31);
                list.push_back((int)k);
                if (p->row_hi < 0) p->row_lo = j - y0;
                p->row_hi = j - y0;
            }
        }
        p->active = (long long)list.size();
    }
    if (!bits.empty()) {
        int rc = ensure_device();
        const size_t nb = bits.size() * sizeof(unsigned), nl = list.size() * sizeof(int);
        if (rc == DLESM_OK && hipMalloc((void **)&p->bits, nb) != hipSuccess) {
            p->bits = nullptr;
            rc = fail(DLESM_EHIP, "%s: hipMalloc of %zu bytes failed", who, nb);
        }
        if (rc == DLESM_OK && nl && hipMalloc((void **)&p->list, nl) != hipSuccess) {
            p->list = nullptr;
            rc = fail(DLESM_EHIP, "%s: hipMalloc of %zu bytes failed", who, nl);
        }
        if (rc == DLESM_OK && (hipMemcpy(p->bits, bits.data(), nb, hipMemcpyHostToDevice) != hipSuccess ||
                               (nl && hipMemcpy(p->list, list.data(), nl, hipMemcpyHostToDevice) != hipSuccess)))
            rc = fail(DLESM_EHIP, "%s: upload of the tile map failed", who);
        if (rc != DLESM_OK) {
            if (p->bits) (void)hipFree(p->bits);
            if (p->list) (void)hipFree(p->list);
            delete p;
            return rc;
        }
    }
    *out = p;
    return DLESM_OK;
}

extern "C" int dlesm_wet_plan_destroy(dlesm_wet_plan *plan)
{
    if (!plan) return DLESM_OK;
    if (plan->bits) DLESM_HIP_TRY(hipFree(plan->bits));
    if (plan->list) DLESM_HIP_TRY(hipFree(plan->list));
    delete plan;
    return DLESM_OK;
}

extern "C" int dlesm_wet_plan_counts(const dlesm_wet_plan *plan, long long *tiles, long long *active)
{
    DLESM_REQUIRE(plan && tiles && active, "dlesm_wet_plan_counts: null pointer");
    *tiles = plan->tiles, *active = plan->active;
    return DLESM_OK;
}

extern "C" int dlesm_nemolite_step_f64(const dlesm_momentum_params *params, const dlesm_momentum_grid *grid,
                                       const double *area_t, int ld, int ny, const dlesm_region *tbox,
                                       const dlesm_region *ubox, const dlesm_region *vbox, const dlesm_obc *obc,
                                       double ssh_bc, const double *un, const double *vn, const double *ht, const double *hu,
                                       const double *hv, const double *sshn_t, const double *sshn_u, const double *sshn_v,
                                       double *ssha, double *ssha_u, double *ssha_v, double *ua, double *va, void *stream)
{
    return step_impl("dlesm_nemolite_step_f64", nullptr, params, grid, area_t, ld, ny, tbox, ubox, vbox, obc, ssh_bc, un, vn,
                     ht, hu, hv, sshn_t, sshn_u, sshn_v, ssha, ssha_u, ssha_v, ua, va, stream);
}

extern "C" int dlesm_nemolite_step_wet_f64(const dlesm_wet_plan *wet, const dlesm_momentum_params *params,
                                           const dlesm_momentum_grid *grid, const double *area_t, int ld, int ny,
                                           const dlesm_region *tbox, const dlesm_region *ubox, const dlesm_region *vbox,
                                           const dlesm_obc *obc, double ssh_bc, const double *un, const double *vn,
                                           const double *ht, const double *hu, const double *hv, const double *sshn_t,
                                           const double *sshn_u, const double *sshn_v, double *ssha, double *ssha_u,
                                           double *ssha_v, double *ua, double *va, void *stream)
{
    return step_impl("dlesm_nemolite_step_wet_f64", wet, params, grid, area_t, ld, ny, tbox, ubox, vbox, obc, ssh_bc, un, vn,
                     ht, hu, hv, sshn_t, sshn_u, sshn_v, ssha, ssha_u, ssha_v, ua, va, stream);
}
