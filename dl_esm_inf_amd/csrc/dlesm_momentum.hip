// The momentum update and the sea-surface-height interpolation onto u and v points of a NEMOLite2D-class model: the loop
// nests that consume the metric grid properties (GO_GRID_DX_U, GO_GRID_DY_U/V, GO_GRID_AREA_U/V, GO_GRID_LAT_U/V via the
// Coriolis parameter; argument_mod.f90:75-112).  The reference holds no such loop (SURVEY.md sections 0 and 2.1): the
// specification is frozen in DESIGN.md section 6.5 and the kernels below evaluate it as written there, every operation
// rounded in double precision in the order the parentheses give (built with -ffp-contract=off, no reciprocals).
//
// momentum_tile<WU, WV>: ONE wave-tile sweep for momentum_u (WU), momentum_v (WV) and both in one pass (the fused entry),
// so that the three entries cannot drift apart.  64 lanes x 2 columns x MR rows, swept linearly like the other sweeps:
// operands at i-1 / i+1 come from the neighbouring lane by a DPP wave shift, lane 0 and lane 63 fetch the column outside
// the wave; operands at j-1 / j+1 come from the rows loaded above and below the tile's own.  Mixed wet / dry column pairs
// store per column (8 bytes) -- an unwritten cell is never stored, and ua / va are never read.  Fused: 20 double streams
// and the mask read, two written, 180 B/cell against 2 x 140 B/cell for the separate loop nests.
// momentum_direct<WU, WV>: one cell per thread, for odd leading dimensions and bases the wave tile cannot take.
// next_ssh<DI, DJ>: the pointwise interpolation of the new surface height onto u (1,0) or v (0,1) points, 36 B/cell.
#include <algorithm>

#include "dlesm_nemolite.h"

namespace dlesm {

namespace {

typedef double d2 __attribute__((ext_vector_type(2)));
typedef int i2 __attribute__((ext_vector_type(2)));

using namespace nemo;   // the operands, MomArgs, Box and the point expressions mom_u / mom_v / ssh_point (dlesm_nemolite.h)

// which operands each loop nest reads
__host__ __device__ constexpr bool read_by_u(int f) { return f != SAV && f != DYV && f != AV && f != FV; }
__host__ __device__ constexpr bool read_by_v(int f) { return f != SAU && f != DXU && f != AU && f != FU; }
template <bool WU, bool WV> __host__ __device__ constexpr bool needed(int f) { return (WU && read_by_u(f)) || (WV && read_by_v(f)); }

constexpr int MR = 1;   // rows per wave tile: 2 rows need more than 256 VGPRs in every instantiation (one wave per SIMD)

// (x0:x1, y0:y1) = the bounding box of the boxes swept (0-based); ub / vb = the U-point and V-point boxes
template <bool WU, bool WV>
__global__ __launch_bounds__(256) void momentum_tile(MomArgs a, int ld, Box ub, Box vb, int x0, int x1, int y0, int y1,
                                                     int c_first, int nxw)
{
    const int lane = threadIdx.x & 63;
    const int w = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    const int xw = w % nxw, jb = y0 + (w / nxw) * MR;
    if (jb > y1) return;
    const int je = jb + MR - 1 > y1 ? y1 : jb + MR - 1;
    const int c = c_first + xw * 64 + lane;              // this lane's chunk (2 columns)
    if (c - lane > x1 / 2) return;                       // idle padding tile
    const int c_ld = ld / 2 - 1, cl = c < c_ld ? c : c_ld;
    const bool m0 = c * 2 >= x0 && c * 2 <= x1, m1 = c * 2 + 1 >= x0 && c * 2 + 1 <= x1;
    // the columns this wave cannot get from a lane; other lanes load a cell of their own chunk (no branch, see
    // LAB_NOTES.md section 5.10: an edge load behind a branch is one more dependent round trip)
    const int wcol = (lane == 0 && m0) ? c * 2 - 1 : cl * 2, ecol = (lane == 63 && m1) ? c * 2 + 2 : cl * 2 + 1;

    // rows jb-1 .. je+1 (clamped to je+1: loaded again, never used); columns c*2-1 .. c*2+2
    double v[NF][MR + 2][4];
    int t[MR + 2][4];
#pragma unroll
    for (int r = 0; r < MR + 2; r++) {
        int jj = jb - 1 + r;
        if (jj > je + 1) jj = je + 1;
        const size_t row = (size_t)jj * ld, o = row + (size_t)cl * 2;
#pragma unroll
        for (int f = 0; f < NF; f++) {
            if (!needed<WU, WV>(f)) continue;
            const d2 q = *(const d2 *)(a.f[f] + o);
            v[f][r][0] = a.f[f][row + wcol];
            v[f][r][1] = q.x;
            v[f][r][2] = q.y;
            v[f][r][3] = a.f[f][row + ecol];
        }
        const i2 q = *(const i2 *)(a.tmask + o);
        t[r][0] = a.tmask[row + wcol];
        t[r][1] = q.x;
        t[r][2] = q.y;
        t[r][3] = a.tmask[row + ecol];
    }
    // west / east neighbours from the neighbouring lanes (whatever is unused is dropped by the compiler)
#pragma unroll
    for (int r = 0; r < MR + 2; r++) {
#pragma unroll
        for (int f = 0; f < NF; f++) {
            if (!needed<WU, WV>(f)) continue;
            const double wl = from_lower<true>(v[f][r][2]), eu = from_upper<true>(v[f][r][1]);
            if (lane != 0) v[f][r][0] = wl;
            if (lane != 63) v[f][r][3] = eu;
        }
        const int wl = __builtin_amdgcn_mov_dpp(t[r][2], 0x138, 0xf, 0xf, true);
        const int eu = __builtin_amdgcn_mov_dpp(t[r][1], 0x130, 0xf, 0xf, true);
        if (lane != 0) t[r][0] = wl;
        if (lane != 63) t[r][3] = eu;
    }
#pragma unroll
    for (int k = 0; k < MR; k++) {
        const int jj = jb + k;
        if (jj > je) break;
        const size_t o = (size_t)jj * ld + (size_t)c * 2;
        double ou[2], ov[2];
        bool su[2], sv[2];
#pragma unroll
        for (int q = 0; q < 2; q++) {
            auto X = [&](int f, int di, int dj) { return v[f][k + 1 + dj][q + 1 + di]; };
            auto T = [&](int di, int dj) { return t[k + 1 + dj][q + 1 + di]; };
            const bool in = q ? m1 : m0;
            if constexpr (WU) {
                ou[q] = mom_u(a, X, T);
                su[q] = in && ub.has(c * 2 + q, jj) && T(0, 0) > 0 && T(1, 0) > 0;
            }
            if constexpr (WV) {
                ov[q] = mom_v(a, X, T);
                sv[q] = in && vb.has(c * 2 + q, jj) && T(0, 0) > 0 && T(0, 1) > 0;
            }
        }
        if constexpr (WU) {
            double *p = a.ua + o;
            if (su[0] && su[1]) *(d2 *)p = d2{ou[0], ou[1]};
            else {
                if (su[0]) p[0] = ou[0];
                if (su[1]) p[1] = ou[1];
            }
        }
        if constexpr (WV) {
            double *p = a.va + o;
            if (sv[0] && sv[1]) *(d2 *)p = d2{ov[0], ov[1]};
            else {
                if (sv[0]) p[0] = ov[0];
                if (sv[1]) p[1] = ov[1];
            }
        }
    }
}

// one cell per thread: odd leading dimensions and bases the wave tile cannot take
template <bool WU, bool WV>
__global__ __launch_bounds__(256) void momentum_direct(MomArgs a, int ld, Box ub, Box vb, int x0, int x1, int y0, int y1)
{
    const int i = x0 + blockIdx.x * blockDim.x + threadIdx.x;
    if (i > x1) return;
    for (int j = y0 + blockIdx.y; j <= y1; j += gridDim.y) {
        const long o = (long)j * ld + i;
        auto X = [&](int f, int di, int dj) { return a.f[f][o + di + (long)dj * ld]; };
        auto T = [&](int di, int dj) { return a.tmask[o + di + (long)dj * ld]; };
        if (WU && ub.has(i, j) && T(0, 0) > 0 && T(1, 0) > 0) a.ua[o] = mom_u(a, X, T);
        if (WV && vb.has(i, j) && T(0, 0) > 0 && T(0, 1) > 0) a.va[o] = mom_v(a, X, T);
    }
}

// next_sshu (DI, DJ) = (1, 0), next_sshv (0, 1); area_x = area_u / area_v
template <int DI, int DJ>
__global__ __launch_bounds__(256) void next_ssh(const int *__restrict__ tmask, const double *__restrict__ area_t,
                                                const double *__restrict__ area_x, const double *__restrict__ sshn_t,
                                                double *__restrict__ out, int ld, int x0, int x1, int y0, int y1)
{
    const int i = x0 + blockIdx.x * blockDim.x + threadIdx.x;
    if (i > x1) return;
    for (int j = y0 + blockIdx.y; j <= y1; j += gridDim.y) {
        const size_t o = (size_t)j * ld + i, on = o + DI + (size_t)DJ * ld;
        const long long t0 = tmask[o], t1 = tmask[on];
        const double a0 = area_t[o], a1 = area_t[on], s0 = sshn_t[o], s1 = sshn_t[on], ax = area_x[o];
        if (t0 + t1 <= 0) continue;
        out[o] = ssh_point(t0, t1, a0, a1, s0, s1, ax);
    }
}

// the momentum entries: boxes 1-based (an empty one: xstop < xstart or ystop < ystart)
template <bool WU, bool WV>
int momentum_launch(const char *who, const dlesm_momentum_params *p, const dlesm_momentum_grid *gr, int ld, int ny,
                    const dlesm_region *ubox, const dlesm_region *vbox, const double *const (&in)[10], double *ua, double *va,
                    void *stream)
{
    if (int rc = ensure_device()) return rc;
    DLESM_REQUIRE(p && gr, "%s: null parameter or grid pointer", who);
    Box ub{1, 0, 1, 0}, vb{1, 0, 1, 0};
    if (WU) {
        DLESM_REQUIRE(ubox, "%s: null region", who);
        if (ubox->xstop >= ubox->xstart && ubox->ystop >= ubox->ystart) {
            if (int rc = check_box(who, ld, ny, ubox->xstart, ubox->xstop, ubox->ystart, ubox->ystop, 1)) return rc;
            ub = Box{ubox->xstart - 1, ubox->xstop - 1, ubox->ystart - 1, ubox->ystop - 1};
        }
    }
    if (WV) {
        DLESM_REQUIRE(vbox, "%s: null region", who);
        if (vbox->xstop >= vbox->xstart && vbox->ystop >= vbox->ystart) {
            if (int rc = check_box(who, ld, ny, vbox->xstart, vbox->xstop, vbox->ystart, vbox->ystop, 1)) return rc;
            vb = Box{vbox->xstart - 1, vbox->xstop - 1, vbox->ystart - 1, vbox->ystop - 1};
        }
    }
    const bool eu = ub.x0 > ub.x1, ev = vb.x0 > vb.x1;
    if (eu && ev) return DLESM_OK;                       // empty boxes: zero-trip loop nests

    MomArgs a{};
    const double *const grid_of[NF] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                                       gr->dx_t, gr->dy_t, gr->dx_u, gr->dy_u, gr->dx_v, gr->dy_v, gr->area_u, gr->area_v,
                                       gr->fcor_u, gr->fcor_v};
    const size_t nb = (size_t)ld * (size_t)ny * sizeof(double);
    DLESM_REQUIRE(gr->tmask, "%s: null tmask", who);
    for (int f = 0; f < NF; f++) {
        if (!needed<WU, WV>(f)) continue;
        a.f[f] = f < 10 ? in[f] : grid_of[f];
        DLESM_REQUIRE(a.f[f], "%s: null pointer (operand %d)%s", who, f,
                      f == FU || f == FV ? ": the Coriolis parameter has not been set" : "");
    }
    double *const outs[2] = {WU ? ua : nullptr, WV ? va : nullptr};
    DLESM_REQUIRE(!(WU && !ua) && !(WV && !va), "%s: null output", who);
    for (double *o : outs) {
        if (!o) continue;
        DLESM_REQUIRE(!overlap(o, nb, gr->tmask, nb / 2), "%s: an output overlaps tmask", who);
        for (int f = 0; f < NF; f++)
            DLESM_REQUIRE(!a.f[f] || !overlap(o, nb, a.f[f], nb), "%s: an output overlaps an input (operand %d)", who, f);
    }
    DLESM_REQUIRE(!(WU && WV) || !overlap(ua, nb, va, nb), "%s: ua and va overlap", who);
    a.tmask = gr->tmask;
    a.ua = ua;
    a.va = va;
    a.rdt = p->rdt;
    a.visc = p->visc;
    a.g = p->g;
    a.den = 1.0 + p->cbfr * p->rdt;

    // the bounding box of the boxes swept
    const int x0 = eu ? vb.x0 : ev ? ub.x0 : std::min(ub.x0, vb.x0), x1 = eu ? vb.x1 : ev ? ub.x1 : std::max(ub.x1, vb.x1);
    const int y0 = eu ? vb.y0 : ev ? ub.y0 : std::min(ub.y0, vb.y0), y1 = eu ? vb.y1 : ev ? ub.y1 : std::max(ub.y1, vb.y1);
    hipStream_t s = (hipStream_t)stream;
    if (lanes16_fit(ld, gr->tmask, a.f, NF) && lanes16_fit(ld, nullptr, outs, 2) && tuning("mom_kernel", 0) == 0) {
        TilePlan t;
        if (int rc = tile_plan(who, ld, x0, x1, y0, y1, CHUNKS_ALL, MR, SHAPE_FOUR, 4, &t)) return rc;      // __launch_bounds__(256)
        hipLaunchKernelGGL((momentum_tile<WU, WV>), dim3(t.grid), dim3(64 * t.tpb), 0, s, a, ld, ub, vb, x0, x1, y0, y1, t.c_first, t.nxw);
    } else {
        const DirectGrid g = direct_grid(x0, x1, y0, y1);
        hipLaunchKernelGGL((momentum_direct<WU, WV>), dim3(g.x, g.y), dim3(256), 0, s, a, ld, ub, vb, x0, x1, y0, y1);
    }
    DLESM_HIP_TRY(hipGetLastError());
    return DLESM_OK;
}

template <int DI, int DJ>
int next_ssh_launch(const char *who, int ld, int ny, int xstart, int xstop, int ystart, int ystop, const int *tmask,
                    const double *area_t, const double *area_x, const double *sshn_t, double *out, void *stream)
{
    if (int rc = ensure_device()) return rc;
    if (xstop < xstart || ystop < ystart) return DLESM_OK;
    if (int rc = check_box(who, ld, ny, xstart, xstop, ystart, ystop, 1)) return rc;
    DLESM_REQUIRE(tmask && area_t && area_x && sshn_t && out, "%s: null pointer", who);
    const size_t nb = (size_t)ld * (size_t)ny * sizeof(double);
    DLESM_REQUIRE(!overlap(out, nb, tmask, nb / 2) && !overlap(out, nb, area_t, nb) && !overlap(out, nb, area_x, nb) &&
                      !overlap(out, nb, sshn_t, nb),
                  "%s: the output overlaps an input", who);
    const int x0 = xstart - 1, x1 = xstop - 1, y0 = ystart - 1, y1 = ystop - 1;
    const DirectGrid g = direct_grid(x0, x1, y0, y1);
    hipLaunchKernelGGL((next_ssh<DI, DJ>), dim3(g.x, g.y), dim3(256), 0, (hipStream_t)stream, tmask, area_t, area_x, sshn_t, out,
                       ld, x0, x1, y0, y1);
    DLESM_HIP_TRY(hipGetLastError());
    return DLESM_OK;
}

} // namespace

} // namespace dlesm

using namespace dlesm;

extern "C" int dlesm_momentum_u_f64(const dlesm_momentum_params *params, const dlesm_momentum_grid *grid, int ld, int ny,
                                    int xstart, int xstop, int ystart, int ystop, const double *un, const double *vn,
                                    const double *ht, const double *sshn_t, const double *hu, const double *sshn_u,
                                    const double *hv, const double *sshn_v, const double *ssha_u, double *ua, void *stream)
{
    const dlesm_region box{0, 0, xstart, xstop, ystart, ystop};
    const double *const in[10] = {un, vn, ht, sshn_t, hu, sshn_u, hv, sshn_v, ssha_u, nullptr};
    return momentum_launch<true, false>("dlesm_momentum_u_f64", params, grid, ld, ny, &box, nullptr, in, ua, nullptr, stream);
}

extern "C" int dlesm_momentum_v_f64(const dlesm_momentum_params *params, const dlesm_momentum_grid *grid, int ld, int ny,
                                    int xstart, int xstop, int ystart, int ystop, const double *un, const double *vn,
                                    const double *ht, const double *sshn_t, const double *hu, const double *sshn_u,
                                    const double *hv, const double *sshn_v, const double *ssha_v, double *va, void *stream)
{
    const dlesm_region box{0, 0, xstart, xstop, ystart, ystop};
    const double *const in[10] = {un, vn, ht, sshn_t, hu, sshn_u, hv, sshn_v, nullptr, ssha_v};
    return momentum_launch<false, true>("dlesm_momentum_v_f64", params, grid, ld, ny, nullptr, &box, in, nullptr, va, stream);
}

extern "C" int dlesm_momentum_f64(const dlesm_momentum_params *params, const dlesm_momentum_grid *grid, int ld, int ny,
                                  const dlesm_region *ubox, const dlesm_region *vbox, const double *un, const double *vn,
                                  const double *ht, const double *sshn_t, const double *hu, const double *sshn_u,
                                  const double *hv, const double *sshn_v, const double *ssha_u, const double *ssha_v,
                                  double *ua, double *va, void *stream)
{
    const double *const in[10] = {un, vn, ht, sshn_t, hu, sshn_u, hv, sshn_v, ssha_u, ssha_v};
    return momentum_launch<true, true>("dlesm_momentum_f64", params, grid, ld, ny, ubox, vbox, in, ua, va, stream);
}

extern "C" int dlesm_next_sshu_f64(int ld, int ny, int xstart, int xstop, int ystart, int ystop, const int *tmask,
                                   const double *area_t, const double *area_u, const double *sshn_t, double *sshn_u,
                                   void *stream)
{
    return next_ssh_launch<1, 0>("dlesm_next_sshu_f64", ld, ny, xstart, xstop, ystart, ystop, tmask, area_t, area_u, sshn_t,
                                 sshn_u, stream);
}

extern "C" int dlesm_next_sshv_f64(int ld, int ny, int xstart, int xstop, int ystart, int ystop, const int *tmask,
                                   const double *area_t, const double *area_v, const double *sshn_t, double *sshn_v,
                                   void *stream)
{
    return next_ssh_launch<0, 1>("dlesm_next_sshv_f64", ld, ny, xstart, xstop, ystart, ystop, tmask, area_t, area_v, sshn_t,
                                 sshn_v, stream);
}
