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
#include "dlesm_nemolite.h"

namespace dlesm {

namespace {

typedef double d2 __attribute__((ext_vector_type(2)));
typedef int i2 __attribute__((ext_vector_type(2)));

using namespace nemo;

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

// (x0:x1, y0:y1) = the box B (0-based)
__global__ __launch_bounds__(256) void nemolite_step_tile(StepArgs s, int ld, int x0, int x1, int y0, int y1, int c_first,
                                                          int nxw)
{
    const MomArgs &a = s.m;
    const int lane = threadIdx.x & 63;
    const int w = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    const int xw = w % nxw, j = y0 + w / nxw;
    if (j > y1) return;
    const int c = c_first + xw * 63 + lane;              // this lane's chunk (2 columns); lane 63 = the next wave's lane 0
    if (c - lane > x1 / 2) return;                       // idle padding tile
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

} // namespace dlesm

using namespace dlesm;

extern "C" int dlesm_nemolite_step_f64(const dlesm_momentum_params *params, const dlesm_momentum_grid *grid,
                                       const double *area_t, int ld, int ny, const dlesm_region *tbox,
                                       const dlesm_region *ubox, const dlesm_region *vbox, const dlesm_obc *obc,
                                       double ssh_bc, const double *un, const double *vn, const double *ht, const double *hu,
                                       const double *hv, const double *sshn_t, const double *sshn_u, const double *sshn_v,
                                       double *ssha, double *ssha_u, double *ssha_v, double *ua, double *va, void *stream)
{
    static const char *who = "dlesm_nemolite_step_f64";
    if (int rc = ensure_device()) return rc;
    if (int rc = step_check(who, params, grid, area_t, ld, ny, tbox, ubox, vbox, obc, un, vn, ht, hu, hv, sshn_t, sshn_u,
                            sshn_v, ssha, ssha_u, ssha_v, ua, va))
        return rc;
    const double *const ins[19] = {un, vn, ht, hu, hv, sshn_t, sshn_u, sshn_v, area_t, grid->dx_t, grid->dy_t, grid->dx_u,
                                   grid->dy_u, grid->dx_v, grid->dy_v, grid->area_u, grid->area_v, grid->fcor_u,
                                   grid->fcor_v};
    double *const outs[5] = {ssha, ssha_u, ssha_v, ua, va};

    bool aligned = ld % 2 == 0 && (uintptr_t)grid->tmask % 8 == 0;
    for (const double *p : ins) aligned = aligned && (uintptr_t)p % 16 == 0;
    for (const double *p : outs) aligned = aligned && (uintptr_t)p % 16 == 0;
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
            const int c_first = (x0 / 2) & ~7, c_last = x1 / 2;  // tiles anchored on 128-byte lines of the row
            int nxw = (c_last - c_first + 63) / 63, tpb = 4;   // 63 chunks per wave
            choose_block_shape(&nxw, &tpb, 4);
            if (tpb > 4) tpb = 4;                               // __launch_bounds__(256)
            const unsigned nblk = (unsigned)(((long)nxw * (y1 - y0 + 1) + tpb - 1) / tpb);
            hipLaunchKernelGGL(nemolite_step_tile, dim3(nblk), dim3(64 * tpb), 0, st, s, ld, x0, x1, y0, y1, c_first, nxw);
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
