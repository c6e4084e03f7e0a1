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
#include "dlesm_nemolite.h"

namespace dlesm {

namespace {

typedef double d2 __attribute__((ext_vector_type(2)));
typedef int i2 __attribute__((ext_vector_type(2)));

using namespace nemo;

constexpr int TILE_CHUNKS = 63;       // chunks (2 columns) a wave owns; lane 63 only loads
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

struct Launch {
    bool tile;
    int ld, x0, x1, y0, y1, c_first, nxw, tpb;
    hipStream_t st;
};

template <int NT>
void launch(const Launch &l, double rdt, const TracerFields &f, const double *const *c_in, double *const *c_out)
{
    TracerArgs<NT> a{};
    a.f = f, a.rdt = rdt;
    for (int k = 0; k < NT; k++) a.c_in[k] = c_in[k], a.c_out[k] = c_out[k];
    const int h = l.y1 - l.y0 + 1;
    if (l.tile) {
        const unsigned nblk = (unsigned)(((long)l.nxw * h + l.tpb - 1) / l.tpb);
        hipLaunchKernelGGL(tracer_tile<NT>, dim3(nblk), dim3(64 * l.tpb), 0, l.st, a, l.ld, l.x0, l.x1, l.y0, l.y1, l.c_first,
                           l.nxw);
    } else {
        hipLaunchKernelGGL(tracer_direct<NT>, dim3((l.x1 - l.x0 + 256) / 256, h > 4096 ? 4096 : h), dim3(256), 0, l.st, a,
                           l.ld, l.x0, l.x1, l.y0, l.y1);
    }
}

} // namespace

// every refusal of DESIGN.md section 6.10, before anything is launched (dlesm_tracer_step_f64, dlesm_tracer_step_dm)
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

extern "C" int dlesm_tracer_step_f64(double rdt, int ld, int ny, int xstart, int xstop, int ystart, int ystop,
                                     const int *tmask, const double *area_t, const double *un, const double *vn,
                                     const double *hu, const double *hv, const double *ht, const double *sshn_t,
                                     const double *sshn_u, const double *sshn_v, const double *ssha,
                                     const double *const *c_in, double *const *c_out, int ntracers, void *stream)
{
    static const char *who = "dlesm_tracer_step_f64";
    if (int rc = ensure_device()) return rc;
    const TracerFields f{tmask, area_t, un, vn, hu, hv, ht, sshn_t, sshn_u, sshn_v, ssha};
    if (int rc = tracer_check(who, ld, ny, xstart, xstop, ystart, ystop, f, c_in, c_out, ntracers)) return rc;
    if (xstop < xstart || ystop < ystart) return DLESM_OK;   // empty box: a zero-trip loop nest

    bool aligned = ld % 2 == 0 && (uintptr_t)tmask % 8 == 0;
    for (const double *p : {area_t, un, vn, hu, hv, ht, sshn_t, sshn_u, sshn_v, ssha}) aligned = aligned && (uintptr_t)p % 16 == 0;
    for (int k = 0; k < ntracers; k++) aligned = aligned && (uintptr_t)c_in[k] % 16 == 0 && (uintptr_t)c_out[k] % 16 == 0;

    Launch l{};
    l.tile = aligned && tuning("tracer_kernel", 0) == 0;
    l.ld = ld, l.x0 = xstart - 1, l.x1 = xstop - 1, l.y0 = ystart - 1, l.y1 = ystop - 1;
    l.st = (hipStream_t)stream;
    if (l.tile) {
        l.c_first = (l.x0 / 2) & ~7;                     // tiles anchored on a 128-byte line of the row
        l.nxw = (l.x1 / 2 - l.c_first + TILE_CHUNKS) / TILE_CHUNKS, l.tpb = 4;
        choose_block_shape(&l.nxw, &l.tpb, 4);
        if (l.tpb > 4) l.tpb = 4;                        // __launch_bounds__(256)
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
