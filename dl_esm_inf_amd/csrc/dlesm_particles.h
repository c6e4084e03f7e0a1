// The point rules of the Lagrangian particles (DESIGN.md sections 6.17 to 6.22), shared by every source that moves, keys or
// counts them: the steps (dlesm_particle_steps.hip), sampling and the owner of the arrays (dlesm_drifter.hip), the sort
// (dlesm_particle_sort.hip), the bins (dlesm_cell_bin.hip) and the migration (dlesm_particle_migrate.hip).  No flow rule is
// here and no particle rule is in dlesm_nemolite.h: a change on one side recompiles nothing on the other.  Every operation
// is rounded in double precision in the order the parentheses give: the sources that include this header are built with
// -ffp-contract=off and no expression here replaces a division by a reciprocal.
#pragma once

#include "dlesm_internal.h"

namespace dlesm {

namespace nemo {

// Drifters (dlesm_particle_steps.hip).  A particle's position (x, y) is in local index coordinates: T cell
// (i, j), 1-based, covers [i, i+1) x [j, j+1); un(i-1, j) and un(i, j) live on its west and east face, vn(i, j-1) and
// vn(i, j) on its south and north face.  DrifterBox holds the box's bounds as doubles: inbox is evaluated in double BEFORE
// any conversion to an integer, so a NaN or an infinity is "not in the box" and is never cast.
struct DrifterBox {
    double x_lo, x_hi, y_lo, y_hi;            // xstart, xstop + 1, ystart, ystop + 1
    __host__ __device__ bool has(double x, double y) const { return x >= x_lo && x < x_hi && y >= y_lo && y < y_hi; }
};
inline DrifterBox drifter_box(int xstart, int xstop, int ystart, int ystop)
{
    return DrifterBox{(double)xstart, (double)xstop + 1.0, (double)ystart, (double)ystop + 1.0};
}
// The key of a particle (dlesm_particle_sort.hip orders by it, dlesm_cell_bin.hip bins by it): the
// row-major number of its cell in the box while it is live -- ACTIVE and in the box --, ncells when it is not.  cell() is
// for a live particle alone: the cast stands behind inbox.
struct CellKey {
    DrifterBox box;
    unsigned xstart, ystart, nxb, ncells;
    __device__ __forceinline__ bool live(double x, double y, int status) const
    {
        return status == DLESM_DRIFTER_ACTIVE && box.has(x, y);
    }
    __device__ __forceinline__ unsigned cell(double x, double y) const
    {
        return ((unsigned)(int)floor(y) - ystart) * nxb + ((unsigned)(int)floor(x) - xstart);
    }
    __device__ __forceinline__ unsigned of(double x, double y, int status) const
    {
        unsigned key = ncells;
        if (live(x, y, status)) key = cell(x, y);
        return key;
    }
};
inline CellKey cell_key(int xstart, int xstop, int ystart, int ystop, long long ncells)
{
    return CellKey{drifter_box(xstart, xstop, ystart, ystop), (unsigned)xstart, (unsigned)ystart,
                   (unsigned)((long long)xstop - xstart + 1), (unsigned)ncells};
}
// what one velocity evaluation reads of cell (i, j): the four neighbour masks, the four faces, the two metrics
struct DrifterCell {
    int t_e, t_w, t_n, t_s;
    double u_e, u_w, v_n, v_s, dx, dy;
};
struct DrifterMove {
    double kx, ky;
};
// the arrays a particle step gathers from, and the one text of its 64-bit offsets: at(i, j) of a 1-based cell -- every cell
// asked for is a cell of the box or of its ring --, mask(i, j) = T there, cell(i, j) the DrifterCell, its ten loads
// unconditional and all issued before any is used
struct DrifterFlow {
    const int *tmask;
    const double *dx_t, *dy_t, *un, *vn;
    int ld;
    __device__ __forceinline__ size_t at(int i, int j) const { return (size_t)(j - 1) * (size_t)ld + (size_t)(i - 1); }
    __device__ __forceinline__ int mask(int i, int j) const { return tmask[at(i, j)]; }
    __device__ __forceinline__ DrifterCell cell(int i, int j) const
    {
        const size_t o = at(i, j);
        DrifterCell c;
        c.t_e = tmask[o + 1], c.t_w = tmask[o - 1], c.t_n = tmask[o + ld], c.t_s = tmask[o - ld];
        c.u_e = un[o], c.u_w = un[o - 1], c.v_n = vn[o], c.v_s = vn[o - ld];
        c.dx = dx_t[o], c.dy = dy_t[o];
        return c;
    }
};
// the displacement of one substep of h seconds, in cells, at (x, y) inside cell (i, j): section 6.10's face switches (the
// ones flow_output_point uses), linear between the faces.  Selects, never blends: a face that touches land carries nothing.
__device__ __forceinline__ DrifterMove drifter_vel(double h, double x, double y, int i, int j, const DrifterCell &c)
{
    const double ue = c.t_e != 0 ? c.u_e : 0.0, uw = c.t_w != 0 ? c.u_w : 0.0;
    const double vn = c.t_n != 0 ? c.v_n : 0.0, vs = c.t_s != 0 ? c.v_s : 0.0;
    const double a = x - (double)i, b = y - (double)j;
    const double up = uw + (ue - uw) * a, vp = vs + (vn - vs) * b;
    return DrifterMove{(h * up) / c.dx, (h * vp) / c.dy};
}
// One substep of a particle at (x, y) in the wet cell (i, j): the midpoint rule with an Euler fallback where the midpoint is
// outside the box or not on a wet cell.  cell(i, j) loads the DrifterCell of a cell of the box -- every load of it issued
// before any is used --, mask(i, j) loads T there.  On return status says what became of the particle; (x, y) and (i, j) are
// the new position and its cell unless the move ended on land (GROUNDED keeps the last wet position).  The destination's
// mask is the next substep's own-cell mask: ACTIVE on return means (i, j) is wet.
template <class CF, class TF>
__device__ __forceinline__ int drifter_substep(double h, const DrifterBox &box, double &x, double &y, int &i, int &j, CF cell,
                                               TF mask)
{
    const DrifterMove k1 = drifter_vel(h, x, y, i, j, cell(i, j));
    const double xm = x + 0.5 * k1.kx, ym = y + 0.5 * k1.ky;
    const bool in_m = box.has(xm, ym);
    // a midpoint outside the box is evaluated at the particle's own place (always a cell of the box) and then not used
    const double xe = in_m ? xm : x, ye = in_m ? ym : y;
    const int im = (int)floor(xe), jm = (int)floor(ye);
    const int tm = mask(im, jm);
    const DrifterMove km = drifter_vel(h, xe, ye, im, jm, cell(im, jm));
    const bool mid = in_m && tm > 0;
    const double k2x = mid ? km.kx : k1.kx, k2y = mid ? km.ky : k1.ky;
    const double xn = x + k2x, yn = y + k2y;
    if (!box.has(xn, yn)) {
        x = xn, y = yn;
        return DLESM_DRIFTER_LEFT;
    }
    const int in = (int)floor(xn), jn = (int)floor(yn);
    const int tn = mask(in, jn);
    if (tn == 0) return DLESM_DRIFTER_GROUNDED;
    x = xn, y = yn, i = in, j = jn;
    return tn < 0 ? DLESM_DRIFTER_OPEN : DLESM_DRIFTER_ACTIVE;
}

// Random-walk diffusion (dlesm_particle_steps.hip).  Philox4x32-10 as published (Salmon et al., "Parallel
// random numbers: as easy as 1, 2, 3", SC11): a counter-based generator, integer arithmetic alone, no state anywhere.
struct Philox4 {
    unsigned w[4];
};
__host__ __device__ __forceinline__ Philox4 philox4x32_10(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0,
                                                          unsigned k1)
{
#pragma unroll
    for (int r = 0; r < 10; r++) {
        const unsigned long long p0 = 0xD2511F53ull * c0, p1 = 0xCD9E8D57ull * c2;
        const unsigned n0 = (unsigned)(p1 >> 32) ^ c1 ^ k0, n2 = (unsigned)(p0 >> 32) ^ c3 ^ k1;
        c1 = (unsigned)p1, c3 = (unsigned)p0, c0 = n0, c2 = n2;
        k0 += 0x9E3779B9u, k1 += 0xBB67AE85u;
    }
    return Philox4{{c0, c1, c2, c3}};
}
// a word -> the centre of its bin of (-1, 1): exact, never 0, symmetric (w and ~w give opposite numbers)
__host__ __device__ __forceinline__ double philox_sym(unsigned w) { return ((double)w + 0.5) * 0x1p-31 - 1.0; }
// the kick of particle `id` at substep `tau`, before the metrics divide it: amp metres times two numbers of (-1, 1)
__device__ __forceinline__ DrifterMove dispersal_kick(double amp, unsigned id, unsigned long long tau, unsigned k0, unsigned k1)
{
    const Philox4 r = philox4x32_10(id, 0u, (unsigned)tau, (unsigned)(tau >> 32), k0, k1);
    return DrifterMove{amp * philox_sym(r.w[0]), amp * philox_sym(r.w[1])};
}
// pin_here (dlesm_internal.h) for an int: a load behind it cannot be sunk into a lane-varying branch
__device__ __forceinline__ int pin_here(int x) { return __builtin_amdgcn_mov_dpp(x, 0xE4, 0xf, 0xf, true); }
// The move of a substep with a kick, stage 1 done: k1 of the substep's own cell and the kick (gx, gy) in cells are given.
// The midpoint and k2 as drifter_substep, D = (x, y) + k2, A = D + (gx, gy).  A in the box and not on land is taken; a kick
// that ends on land is rejected -- the no-flux wall -- and D meets drifter_substep's destination rule.  T(cell(A)) and
// T(cell(D)) are loaded together and unconditionally, a point outside the box at the particle's own cell and then not used:
// three dependent round trips as drifter_substep, and whichever destination is taken supplies the next substep's own-cell
// mask.
template <class CF, class TF>
__device__ __forceinline__ int kicked_move(double h, const DrifterBox &box, double &x, double &y, int &i, int &j,
                                           const DrifterMove k1, double gx, double gy, CF cell, TF mask)
{
    const double xm = x + 0.5 * k1.kx, ym = y + 0.5 * k1.ky;
    const bool in_m = box.has(xm, ym);
    const double xe = in_m ? xm : x, ye = in_m ? ym : y;
    const int im = (int)floor(xe), jm = (int)floor(ye);
    const int tm = mask(im, jm);
    const DrifterMove km = drifter_vel(h, xe, ye, im, jm, cell(im, jm));
    const bool mid = in_m && tm > 0;
    const double k2x = mid ? km.kx : k1.kx, k2y = mid ? km.ky : k1.ky;
    const double xd = x + k2x, yd = y + k2y;
    const double xa = xd + gx, ya = yd + gy;
    const bool in_a = box.has(xa, ya), in_d = box.has(xd, yd);
    const int ia = (int)floor(in_a ? xa : x), ja = (int)floor(in_a ? ya : y);
    const int id = (int)floor(in_d ? xd : x), jd = (int)floor(in_d ? yd : y);
    // pinned: left alone, the compiler sinks each load into the branch that uses it, a fourth round trip for a rejected kick
    const int la = mask(ia, ja), ld = mask(id, jd);
    __builtin_amdgcn_sched_barrier(0);            // both issued before either is waited for, whatever the register budget
    const int ta = pin_here(la), td = pin_here(ld);
    if (!in_a) {
        x = xa, y = ya;
        return DLESM_DRIFTER_LEFT;
    }
    if (ta != 0) {
        x = xa, y = ya, i = ia, j = ja;
        return ta < 0 ? DLESM_DRIFTER_OPEN : DLESM_DRIFTER_ACTIVE;
    }
    if (!in_d) {
        x = xd, y = yd;
        return DLESM_DRIFTER_LEFT;
    }
    if (td == 0) return DLESM_DRIFTER_GROUNDED;
    x = xd, y = yd, i = id, j = jd;
    return td < 0 ? DLESM_DRIFTER_OPEN : DLESM_DRIFTER_ACTIVE;
}

// One substep with a kick of a constant amplitude: kick() / the metrics of the substep's own cell (stage 1's, already
// loaded), then kicked_move.  kick() is called behind the stage-1 loads and before their first use: its integer work sits
// under their latency.
template <class CF, class TF, class KF>
__device__ __forceinline__ int dispersal_substep(double h, const DrifterBox &box, double &x, double &y, int &i, int &j, CF cell,
                                                 TF mask, KF kick)
{
    const DrifterCell c1 = cell(i, j);
    const DrifterMove g = kick();
    __builtin_amdgcn_sched_barrier(0);            // the scheduler would otherwise put the generator behind the loads' first use
    const DrifterMove k1 = drifter_vel(h, x, y, i, j, c1);
    return kicked_move(h, box, x, y, i, j, k1, g.kx / c1.dx, g.ky / c1.dy, cell, mask);
}

// A random walk in a varying diffusivity (dlesm_particle_steps.hip).  WalkCell: what one substep reads of
// kh_t, the cell's own value and its four neighbours'.  A face between two cells that are not land carries the mean of the
// two, a coast face the cell's own value: K along x is linear between the cell's u-faces, along y between its v-faces.
struct WalkCell {
    double c, e, w, n, s;
};
// the kick along one axis, in cells: the drift ah * dK/dx (Visser 1997) plus r in (-1, 1) times the amplitude of K half a drift
// ahead of the particle; t_hi, k_hi: the east (north) neighbour's mask and value, frac: the particle's place in its cell
__device__ __forceinline__ double random_walk_kick(double ah, double d, double frac, int t_hi, int t_lo, double kc, double k_hi,
                                                   double k_lo, double r)
{
    const double f_hi = t_hi != 0 ? 0.5 * (kc + k_hi) : kc, f_lo = t_lo != 0 ? 0.5 * (kc + k_lo) : kc;
    const double dk = f_hi - f_lo;
    const double c = (ah * dk) / (d * d);
    double k = f_lo + dk * (frac + 0.5 * c);
    k = k > 0.0 ? k : 0.0;
    return c + (sqrt((6.0 * k) * ah) * r) / d;
}
// One substep of it: dispersal_substep with the kick made from kh_t.  kcell(i, j) loads the WalkCell, five unconditional
// loads issued with cell(i, j)'s ten before any is used; rng() gives the two numbers of (-1, 1) and stands, like kick()
// above, behind the loads and before their first use.
template <class CF, class WF, class TF, class RF>
__device__ __forceinline__ int random_walk_substep(double h, const DrifterBox &box, double &x, double &y, int &i, int &j, CF cell,
                                                   WF kcell, TF mask, RF rng)
{
    const DrifterCell c1 = cell(i, j);
    const WalkCell k = kcell(i, j);
    const DrifterMove r = rng();
    __builtin_amdgcn_sched_barrier(0);
    const DrifterMove k1 = drifter_vel(h, x, y, i, j, c1);
    const double ah = fabs(h);
    const double gx = random_walk_kick(ah, c1.dx, x - (double)i, c1.t_e, c1.t_w, k.c, k.e, k.w, r.kx);
    const double gy = random_walk_kick(ah, c1.dy, y - (double)j, c1.t_n, c1.t_s, k.c, k.n, k.s, r.ky);
    return kicked_move(h, box, x, y, i, j, k1, gx, gy, cell, mask);
}

// The three particle arrays of an entry, for its host checks: whether a range of bytes shares one with px, py or status,
// and with which.  Nothing overlaps the arrays of no particles.
struct ParticleArrays {
    const void *p[3];                         // px, py, status
    long long n;
    static const char *name(int k) { return k == 0 ? "px" : k == 1 ? "py" : "status"; }
    size_t bytes(int k) const { return (size_t)n * (k < 2 ? 8 : 4); }
    bool hits(int k, const void *a, size_t na) const { return n > 0 && overlap(p[k], bytes(k), a, na); }
    // the first of the three that [a, a+na) overlaps, or -1
    int which(const void *a, size_t na) const
    {
        for (int k = 0; k < 3; k++)
            if (hits(k, a, na)) return k;
        return -1;
    }
    // what every entry asks of them, of the extents and of the box with its one-cell ring; *empty: the box holds no cell
    int check(const char *who, int ld, int ny, int xstart, int xstop, int ystart, int ystop, bool *empty) const
    {
        DLESM_REQUIRE(p[0] != nullptr && p[1] != nullptr && p[2] != nullptr, "%s: null px, py or status", who);
        DLESM_REQUIRE((uintptr_t)p[0] % 8 == 0 && (uintptr_t)p[1] % 8 == 0, "%s: px or py is not 8-byte aligned", who);
        DLESM_REQUIRE((uintptr_t)p[2] % 4 == 0, "%s: status is not 4-byte aligned", who);
        DLESM_REQUIRE(n >= 0, "%s: %lld particles", who, n);
        DLESM_REQUIRE(ld >= 1 && ny >= 1, "%s: array extents %dx%d", who, ld, ny);
        *empty = xstop < xstart || ystop < ystart;
        if (!*empty)
            if (int rc = check_box(who, ld, ny, xstart, xstop, ystart, ystop, 1)) return rc;
        DLESM_REQUIRE((n + 255) / 256 <= 0x7fffffffLL, "%s: %lld particles in one call", who, n);
        return DLESM_OK;
    }
};

} // namespace nemo

} // namespace dlesm
