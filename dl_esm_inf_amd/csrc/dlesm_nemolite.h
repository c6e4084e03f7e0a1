// The point expressions of the NEMOLite2D-class kernels (DESIGN.md sections 5.10 and 6.5), shared by every entry that
// evaluates them -- continuity (dlesm_continuity.hip), momentum and next_ssh* (dlesm_momentum.hip), the one-sweep time
// step (dlesm_nemolite_step.hip), tracer transport (dlesm_tracer.hip) and the output fields (dlesm_flow_output.hip) -- so
// that the entries cannot drift apart.  The particles' point rules are in dlesm_particles.h.  Every
// operation is rounded in double precision in the order the parentheses give: the sources that include this header are
// built with -ffp-contract=off and no expression here replaces a division by a reciprocal.
#pragma once

#include "dlesm_internal.h"

namespace dlesm {

namespace nemo {

// the double-precision operands of the momentum loop nests, by number
enum { UN, VN, HT, SST, HU, SSU, HV, SSV, SAU, SAV, DXT, DYT, DXU, DYU, DXV, DYV, AU, AV, FU, FV, NF };

struct MomArgs {
    const double *f[NF];
    const int *tmask;
    double *ua, *va;
    double rdt, visc, g, den;                 // den = 1.0 + cbfr*rdt
};

struct Box {                                  // 0-based inclusive; empty: x0 > x1
    int x0, x1, y0, y1;
    __host__ __device__ bool has(int i, int j) const { return i >= x0 && i <= x1 && j >= y0 && j <= y1; }
};

__device__ __forceinline__ double sg(double x) { return copysign(0.5, x); }

// ssha(ji,jj) of the continuity kernel: _w operands at (ji-1, jj), _s operands at (ji, jj-1)
__device__ __forceinline__ double cont_point(double rdt, double st, double su, double su_w, double sv, double sv_s,
                                             double hu, double hu_w, double hv, double hv_s, double un, double un_w,
                                             double vn, double vn_s, double area)
{
    const double r1 = (su + hu) * un, r2 = (su_w + hu_w) * un_w;
    const double r3 = (sv + hv) * vn, r4 = (sv_s + hv_s) * vn_s;
    return st + (((r2 - r1) + r4) - r3) * rdt / area;
}

// Tracer transport.  What a T cell's update takes from the flow, the same for every tracer: the
// face transports r1..r4 with continuity's expression tree (east, west, north, south), whether each face's far cell is
// anything but land, q = rdt / area_t and the old and new water column.  _w operands at (i-1, j), _s operands at (i, j-1);
// t_e .. t_s = tmask at (i+1, j), (i-1, j), (i, j+1), (i, j-1).
struct TracerFlow {
    double r1, r2, r3, r4, q, h_old, h_new;
    bool e, w, n, s;
};
__device__ __forceinline__ TracerFlow tracer_flow(double rdt, double su, double su_w, double sv, double sv_s, double hu,
                                                  double hu_w, double hv, double hv_s, double un, double un_w, double vn,
                                                  double vn_s, double area, double ht, double st, double sa, int t_e,
                                                  int t_w, int t_n, int t_s)
{
    return TracerFlow{(su + hu) * un, (su_w + hu_w) * un_w, (sv + hv) * vn, (sv_s + hv_s) * vn_s, rdt / area, ht + st,
                      ht + sa, t_e != 0, t_w != 0, t_n != 0, t_s != 0};
}
// c_out(i,j) of a wet cell: first-order upwind fluxes through the four faces; c = the tracer at (i, j), c_e .. c_s at
// (i+1, j), (i-1, j), (i, j+1), (i, j-1).  The upwind choice and the land switch are selects, never blends: what a land
// cell or a face that touches land holds (a NaN included) does not reach the result.
__device__ __forceinline__ double tracer_point(const TracerFlow &f, double c, double c_e, double c_w, double c_n, double c_s)
{
    const double F1 = f.e ? f.r1 * (f.r1 >= 0.0 ? c : c_e) : 0.0;
    const double F2 = f.w ? f.r2 * (f.r2 >= 0.0 ? c_w : c) : 0.0;
    const double F3 = f.n ? f.r3 * (f.r3 >= 0.0 ? c : c_n) : 0.0;
    const double F4 = f.s ? f.r4 * (f.r4 >= 0.0 ? c_s : c) : 0.0;
    return (f.h_old * c + (((F2 - F1) + F4) - F3) * f.q) / f.h_new;
}

// Second-order limited tracer transport: the monotonised-central slope of c at a cell from the
// differences to its two neighbours along one axis (c_m, c, c_p), or 0.0 where `on` is false -- `on` is "the cell is wet and
// neither neighbour is land", T outside the array counting as land.  Compare-and-select, never fmin / fmax (a NaN difference
// gives 0.0), and no division.
__device__ __forceinline__ double muscl_slope(bool on, double c_m, double c, double c_p)
{
    const double a = c - c_m, b = c_p - c;
    const double a2 = 2.0 * fabs(a), b2 = 2.0 * fabs(b), m = 0.5 * fabs(a + b);
    double lo = a2 < b2 ? a2 : b2;
    lo = m < lo ? m : lo;
    const double mc = (a > 0.0 && b > 0.0) ? lo : ((a < 0.0 && b < 0.0) ? -lo : 0.0);
    return on ? mc : 0.0;
}
// c_out(i,j) of a wet cell with the face values reconstructed from the upwind cell's slope: sx, sy = the slopes at (i, j),
// sx_e, sx_w at (i+1, j), (i-1, j), sy_n, sy_s at (i, j+1), (i, j-1); everything else as tracer_point.  A zero slope gives
// tracer_point's face value (c + 0.0, c - 0.0), so coasts, open boundaries and a constant tracer fall back to section 6.10.
__device__ __forceinline__ double tracer_point_muscl(const TracerFlow &f, double c, double c_e, double c_w, double c_n,
                                                     double c_s, double sx, double sx_e, double sx_w, double sy, double sy_n,
                                                     double sy_s)
{
    const double ce = f.r1 >= 0.0 ? c + 0.5 * sx : c_e - 0.5 * sx_e;
    const double cw = f.r2 >= 0.0 ? c_w + 0.5 * sx_w : c - 0.5 * sx;
    const double cn = f.r3 >= 0.0 ? c + 0.5 * sy : c_n - 0.5 * sy_n;
    const double cs = f.r4 >= 0.0 ? c_s + 0.5 * sy_s : c - 0.5 * sy;
    const double F1 = f.e ? f.r1 * ce : 0.0;
    const double F2 = f.w ? f.r2 * cw : 0.0;
    const double F3 = f.n ? f.r3 * cn : 0.0;
    const double F4 = f.s ? f.r4 * cs : 0.0;
    return (f.h_old * c + (((F2 - F1) + F4) - F3) * f.q) / f.h_new;
}

// Time-centred (Hancock) limited tracer transport: the factor that replaces section 6.11's constant
// 0.5 on each face, the same for every tracer.  w = tracer_weight of the cell, w_e .. w_s of its four neighbours; a face's
// Courant number n is taken in the face's upwind cell, and g = 0.5 * (1 - n) for 0 <= n < 1, else 0.0 -- a NaN, an infinite
// or a negative n fails the two comparisons, so g is always finite and what land holds in area_t, ht, sshn_t reaches no
// written cell.
struct TracerCourant {
    double g1, g2, g3, g4;
};
__device__ __forceinline__ double tracer_weight(double rdt, double area, double ht, double st)
{
    return rdt / (area * (ht + st));
}
__device__ __forceinline__ double hancock_factor(double n)
{
    return (n >= 0.0 && n < 1.0) ? 0.5 * (1.0 - n) : 0.0;
}
__device__ __forceinline__ TracerCourant tracer_courant(const TracerFlow &f, double w, double w_e, double w_w, double w_n,
                                                        double w_s)
{
    return TracerCourant{hancock_factor(fabs(f.r1) * (f.r1 >= 0.0 ? w : w_e)),
                         hancock_factor(fabs(f.r2) * (f.r2 >= 0.0 ? w_w : w)),
                         hancock_factor(fabs(f.r3) * (f.r3 >= 0.0 ? w : w_n)),
                         hancock_factor(fabs(f.r4) * (f.r4 >= 0.0 ? w_s : w))};
}
// The four face Courant numbers n1..n4 themselves (east, west, north, south), the arguments of hancock_factor above, for the
// Courant check (dlesm_courant.hip).  tracer_courant keeps its own copy of the four products: routed
// through this function the Hancock kernels compile to other instructions, and their code is to stay as it was measured.  A
// change to one of the two is a change to both.
struct TracerNumbers {
    double n1, n2, n3, n4;
};
__device__ __forceinline__ TracerNumbers tracer_numbers(const TracerFlow &f, double w, double w_e, double w_w, double w_n,
                                                        double w_s)
{
    return TracerNumbers{fabs(f.r1) * (f.r1 >= 0.0 ? w : w_e), fabs(f.r2) * (f.r2 >= 0.0 ? w_w : w),
                         fabs(f.r3) * (f.r3 >= 0.0 ? w : w_n), fabs(f.r4) * (f.r4 >= 0.0 ? w_s : w)};
}
// tracer_point_muscl with the face factors g1..g4 in the place of 0.5.  g = 0.0 gives tracer_point's face value.
__device__ __forceinline__ double tracer_point_hancock(const TracerFlow &f, const TracerCourant &g, double c, double c_e,
                                                       double c_w, double c_n, double c_s, double sx, double sx_e, double sx_w,
                                                       double sy, double sy_n, double sy_s)
{
    const double ce = f.r1 >= 0.0 ? c + g.g1 * sx : c_e - g.g1 * sx_e;
    const double cw = f.r2 >= 0.0 ? c_w + g.g2 * sx_w : c - g.g2 * sx;
    const double cn = f.r3 >= 0.0 ? c + g.g3 * sy : c_n - g.g3 * sy_n;
    const double cs = f.r4 >= 0.0 ? c_s + g.g4 * sy_s : c - g.g4 * sy;
    const double F1 = f.e ? f.r1 * ce : 0.0;
    const double F2 = f.w ? f.r2 * cw : 0.0;
    const double F3 = f.n ? f.r3 * cn : 0.0;
    const double F4 = f.s ? f.r4 * cs : 0.0;
    return (f.h_old * c + (((F2 - F1) + F4) - F3) * f.q) / f.h_new;
}

// The model's output fields (dlesm_flow_output.hip) of a wet T cell, by DLESM_OUT_* number: the
// sea-surface height, the velocities brought to the T point through section 6.10's face switches, their speed, the kinetic
// energy of the column and the relative vorticity at the cell's NE corner.  u, v = un, vn at (i, j); _w, _e operands at
// (i-1, j), (i+1, j), _s, _n at (i, j-1), (i, j+1); t_e .. t_s = tmask at the four neighbours, t_ne at (i+1, j+1).  `corner`
// says whether v[5] may be stored: with the three neighbours non-land all four faces of the circulation are live.  VORT =
// false leaves v[5] at 0.0 and reads none of v_e, u_n, t_ne, dxv, dxv_e, dyu, dyu_n.  Selects, never blends.
struct FlowOutput {
    double v[6];
    bool corner;
};
template <bool VORT>
__device__ __forceinline__ FlowOutput flow_output_point(double u, double u_w, double v, double v_s, double v_e, double u_n,
                                                        double ht, double st, double dxv, double dxv_e, double dyu,
                                                        double dyu_n, int t_e, int t_w, int t_n, int t_s, int t_ne)
{
    const double e = t_e != 0 ? u : 0.0, w = t_w != 0 ? u_w : 0.0;
    const double n = t_n != 0 ? v : 0.0, s = t_s != 0 ? v_s : 0.0;
    const double ut = 0.5 * (w + e), vt = 0.5 * (s + n);
    const double q = ut * ut + vt * vt;
    const double d = ht + st;
    FlowOutput r{{st, ut, vt, sqrt(q), (0.5 * d) * q, 0.0}, false};
    if constexpr (VORT) {
        const double dvdx = (v_e - v) / (0.5 * (dxv + dxv_e));
        const double dudy = (u_n - u) / (0.5 * (dyu + dyu_n));
        r.v[5] = dvdx - dudy;
        r.corner = t_e != 0 && t_n != 0 && t_ne != 0;
    }
    return r;
}

// next_sshu / next_sshv at a face whose mask sum t0 + t1 is > 0: 0 = the face's own T cell,
// 1 = the one east (north) of it; ax = area_u (area_v) of the face
__device__ __forceinline__ double ssh_point(long long t0, long long t1, double a0, double a1, double s0, double s1, double ax)
{
    return t0 * t1 > 0 ? (0.5 * (a0 * s0 + a1 * s1)) / ax : (t0 <= 0 ? s1 : s0);
}

// ua(i,j) of DESIGN.md section 6.5.  X(f, di, dj) = operand f at (i+di, j+dj), T(di, dj) = tmask there.
template <class XF, class TF>
__device__ __forceinline__ double mom_u(const MomArgs &a, XF X, TF T)
{
    const bool sw = T(0, -1) > 0 && T(1, -1) > 0, nw = T(0, 1) > 0 && T(1, 1) > 0;
    const double un = X(UN, 0, 0), hsu = X(HU, 0, 0) + X(SSU, 0, 0);
    const double u_e = (0.5 * (un + X(UN, 1, 0))) * X(DYT, 1, 0);
    const double depe = X(HT, 1, 0) + X(SST, 1, 0);
    const double u_w = (0.5 * (un + X(UN, -1, 0))) * X(DYT, 0, 0);
    const double depw = X(HT, 0, 0) + X(SST, 0, 0);
    const double v_sc = 0.5 * (X(VN, 0, -1) + X(VN, 1, -1));
    const double v_s = (0.5 * v_sc) * (X(DXV, 0, -1) + X(DXV, 1, -1));
    const double deps = 0.5 * (((X(HV, 0, -1) + X(SSV, 0, -1)) + X(HV, 1, -1)) + X(SSV, 1, -1));
    const double v_nc = 0.5 * (X(VN, 0, 0) + X(VN, 1, 0));
    const double v_n = (0.5 * v_nc) * (X(DXV, 0, 0) + X(DXV, 1, 0));
    const double depn = 0.5 * (((X(HV, 0, 0) + X(SSV, 0, 0)) + X(HV, 1, 0)) + X(SSV, 1, 0));
    const double uu_w = (0.5 - sg(u_w)) * un + (0.5 + sg(u_w)) * X(UN, -1, 0);
    const double uu_e = (0.5 + sg(u_e)) * un + (0.5 - sg(u_e)) * X(UN, 1, 0);
    const double uu_s = sw ? (0.5 - sg(v_s)) * un + (0.5 + sg(v_s)) * X(UN, 0, -1) : (0.5 - sg(v_s)) * un;
    const double uu_n = nw ? (0.5 + sg(v_n)) * un + (0.5 - sg(v_n)) * X(UN, 0, 1) : (0.5 + sg(v_n)) * un;
    const double adv = (((uu_w * u_w) * depw - (uu_e * u_e) * depe) + (uu_s * v_s) * deps) - (uu_n * v_n) * depn;
    const double dudx_e = ((X(UN, 1, 0) - un) / X(DXT, 1, 0)) * (X(HT, 1, 0) + X(SST, 1, 0));
    const double dudx_w = ((un - X(UN, -1, 0)) / X(DXT, 0, 0)) * (X(HT, 0, 0) + X(SST, 0, 0));
    const double dudy_s = sw ? ((un - X(UN, 0, -1)) / (X(DYU, 0, 0) + X(DYU, 0, -1))) *
                                   ((hsu + X(HU, 0, -1)) + X(SSU, 0, -1))
                             : 0.0;
    const double dudy_n = nw ? ((X(UN, 0, 1) - un) / (X(DYU, 0, 0) + X(DYU, 0, 1))) *
                                   ((hsu + X(HU, 0, 1)) + X(SSU, 0, 1))
                             : 0.0;
    const double vis = a.visc * ((dudx_e - dudx_w) * X(DYU, 0, 0) + ((dudy_n - dudy_s) * X(DXU, 0, 0)) * 0.5);
    const double cor = ((0.5 * (X(FU, 0, 0) * (v_sc + v_nc))) * X(AU, 0, 0)) * hsu;
    const double hpg = -(((a.g * hsu) * X(DYU, 0, 0)) * (X(SST, 1, 0) - X(SST, 0, 0)));
    return ((un * hsu + (a.rdt * (((adv + vis) + cor) + hpg)) / X(AU, 0, 0)) / (X(HU, 0, 0) + X(SAU, 0, 0))) / a.den;
}

// va(i,j) of DESIGN.md section 6.5
template <class XF, class TF>
__device__ __forceinline__ double mom_v(const MomArgs &a, XF X, TF T)
{
    const bool ww = T(-1, 0) > 0 && T(-1, 1) > 0, ew = T(1, 0) > 0 && T(1, 1) > 0;
    const double vn = X(VN, 0, 0), hsv = X(HV, 0, 0) + X(SSV, 0, 0);
    const double v_n = (0.5 * (vn + X(VN, 0, 1))) * X(DXT, 0, 1);
    const double depn = X(HT, 0, 1) + X(SST, 0, 1);
    const double v_s = (0.5 * (vn + X(VN, 0, -1))) * X(DXT, 0, 0);
    const double deps = X(HT, 0, 0) + X(SST, 0, 0);
    const double u_wc = 0.5 * (X(UN, -1, 0) + X(UN, -1, 1));
    const double u_w = (0.5 * u_wc) * (X(DYU, -1, 0) + X(DYU, -1, 1));
    const double depw = 0.5 * (((X(HU, -1, 0) + X(SSU, -1, 0)) + X(HU, -1, 1)) + X(SSU, -1, 1));
    const double u_ec = 0.5 * (X(UN, 0, 0) + X(UN, 0, 1));
    const double u_e = (0.5 * u_ec) * (X(DYU, 0, 0) + X(DYU, 0, 1));
    const double depe = 0.5 * (((X(HU, 0, 0) + X(SSU, 0, 0)) + X(HU, 0, 1)) + X(SSU, 0, 1));
    const double vv_s = (0.5 - sg(v_s)) * vn + (0.5 + sg(v_s)) * X(VN, 0, -1);
    const double vv_n = (0.5 + sg(v_n)) * vn + (0.5 - sg(v_n)) * X(VN, 0, 1);
    const double vv_w = ww ? (0.5 - sg(u_w)) * vn + (0.5 + sg(u_w)) * X(VN, -1, 0) : (0.5 - sg(u_w)) * vn;
    const double vv_e = ew ? (0.5 + sg(u_e)) * vn + (0.5 - sg(u_e)) * X(VN, 1, 0) : (0.5 + sg(u_e)) * vn;
    const double adv = (((vv_w * u_w) * depw - (vv_e * u_e) * depe) + (vv_s * v_s) * deps) - (vv_n * v_n) * depn;
    const double dvdy_n = ((X(VN, 0, 1) - vn) / X(DYT, 0, 1)) * (X(HT, 0, 1) + X(SST, 0, 1));
    const double dvdy_s = ((vn - X(VN, 0, -1)) / X(DYT, 0, 0)) * (X(HT, 0, 0) + X(SST, 0, 0));
    const double dvdx_w = ww ? ((vn - X(VN, -1, 0)) / (X(DXV, 0, 0) + X(DXV, -1, 0))) *
                                   ((hsv + X(HV, -1, 0)) + X(SSV, -1, 0))
                             : 0.0;
    const double dvdx_e = ew ? ((X(VN, 1, 0) - vn) / (X(DXV, 0, 0) + X(DXV, 1, 0))) *
                                   ((hsv + X(HV, 1, 0)) + X(SSV, 1, 0))
                             : 0.0;
    const double vis = a.visc * ((dvdy_n - dvdy_s) * X(DXV, 0, 0) + ((dvdx_e - dvdx_w) * X(DYV, 0, 0)) * 0.5);
    const double cor = -(((0.5 * (X(FV, 0, 0) * (u_ec + u_wc))) * X(AV, 0, 0)) * hsv);
    const double hpg = -(((a.g * hsv) * X(DXV, 0, 0)) * (X(SST, 0, 1) - X(SST, 0, 0)));
    return ((vn * hsv + (a.rdt * (((adv + vis) + cor) + hpg)) / X(AV, 0, 0)) / (X(HV, 0, 0) + X(SAV, 0, 0))) / a.den;
}

inline bool empty(const dlesm_region *r) { return r->xstop < r->xstart || r->ystop < r->ystart; }

inline bool same_box(const dlesm_region *a, const dlesm_region *b)
{
    return (empty(a) && empty(b)) ||
           (a->xstart == b->xstart && a->xstop == b->xstop && a->ystart == b->ystart && a->ystop == b->ystop);
}

// every refusal of DESIGN.md section 6.7 (null pointers, boxes, overlaps, the Coriolis parameter, an open-boundary plan of
// other extents), messages prefixed with `who`; DLESM_OK or DLESM_EINVAL.  Launches nothing (dlesm_nemolite_step.hip).
int step_check(const char *who, const dlesm_momentum_params *params, const dlesm_momentum_grid *grid, const double *area_t,
               int ld, int ny, const dlesm_region *tbox, const dlesm_region *ubox, const dlesm_region *vbox,
               const dlesm_obc *obc, const double *un, const double *vn, const double *ht, const double *hu,
               const double *hv, const double *sshn_t, const double *sshn_u, const double *sshn_v, double *ssha,
               double *ssha_u, double *ssha_v, double *ua, double *va);
// every refusal of a wet plan: other extents, a box other than tbox; a null plan is accepted.
// Launches nothing (dlesm_nemolite_step.hip).
int wet_check(const char *who, const dlesm_wet_plan *wet, int ld, int ny, const dlesm_region *tbox);

// the flow a tracer step reads, in the order of the C entry's arguments
struct TracerFields {
    const int *tmask;
    const double *area_t, *un, *vn, *hu, *hv, *ht, *sshn_t, *sshn_u, *sshn_v, *ssha;
};
// every refusal of DESIGN.md section 6.10 (the tracer count, null pointers, a box without its ring, a c_out that overlaps
// an input, a c_in or another c_out), messages prefixed with `who`; DLESM_OK or DLESM_EINVAL.  Launches nothing
// (dlesm_tracer.hip).
int tracer_check(const char *who, int ld, int ny, int xstart, int xstop, int ystart, int ystop, const TracerFields &f,
                 const double *const *c_in, double *const *c_out, int ntracers);

} // namespace nemo

} // namespace dlesm
