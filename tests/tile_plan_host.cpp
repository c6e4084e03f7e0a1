// CPU harness for the launch geometry of the wave-tile sweeps (dl_esm_inf_amd/csrc/dlesm_tile_plan.h): built by
// tests/test_tile_plan_host.py with g++ -fsanitize=address,undefined and run over a sweep of boxes.  For every launcher that
// takes its geometry from the header, the expressions that launcher held before the header existed are written out below as
// they stood, one function per site -- a FROZEN table: it is not to be tidied or shared -- and compared with the header's
// results: first chunk, tiles per row, launched tiles per row, waves per workgroup, workgroups, the one-cell-per-thread grid,
// and both fit rules over aligned and misaligned pointer values.
#include <climits>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "dlesm_tile_plan.h"

namespace dlesm {
static char g_err[512];
int fail(int code, const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof g_err, fmt, ap);
    va_end(ap);
    return code;
}
void clear_error() { g_err[0] = 0; }

// Deterministic stand-ins for the two shape rules of dlesm_kernels.hip: they pad the row and return every block size of
// 2, 4, 8 and 16 waves, so that the caps of 4, 8 and 16 all bite and all pass.
static const int WAVES[4] = {2, 4, 8, 16};
void choose_block_shape(int *nxw_io, int *tpb_out, int prefer)
{
    const int nxw = *nxw_io;
    *tpb_out = WAVES[(nxw + (prefer ? 1 : 0)) & 3];
    *nxw_io = nxw + (nxw * 7 + prefer) % 5;
}
void shape_for_tile_sweep(int ld, int x0, int x1, int y0, int y1, int *nxw_io, int *tpb_out)
{
    if ((ld % 3 + x0 % 3 + y0 % 3 + y1 % 3) % 3 == 0) {            // "a planned shape"
        *nxw_io += 3;
        *tpb_out = WAVES[(x1 + ld) & 3];
        return;
    }
    choose_block_shape(nxw_io, tpb_out);
}
} // namespace dlesm

using namespace dlesm;

static long checks = 0;
#define REQUIRE(c)                                                                                        \
    do {                                                                                                  \
        checks++;                                                                                         \
        if (!(c)) {                                                                                       \
            fprintf(stderr, "FAILED %s (line %d; ld %d box %d:%d,%d:%d): %s\n", #c, __LINE__, g_ld, g_x0, \
                    g_x1, g_y0, g_y1, dlesm::g_err);                                                      \
            return 1;                                                                                     \
        }                                                                                                 \
    } while (0)
static int g_ld, g_x0, g_x1, g_y0, g_y1;

// what a site launches: the tile kernel's arguments and grid, or the one-cell-per-thread grid
struct Was {
    int c_first, nxt, nxw, tpb;
    long long groups;         // the workgroup count before the site turned it into a grid extent
    unsigned grid;            // ... and after
    bool refused;             // (two sites refused more than INT_MAX workgroups; the others cast)
    unsigned gx, gy;
};

// ---- the frozen table: the launchers' own expressions, as they stood --------------------------------------------------

static Was was_launch_stencil9(int ld, int x0, int x1, int y0, int y1)             // dlesm_stencil9.hip; also the shape of
{                                                                                 // dlesm_masked.hip and dlesm_continuity.hip
    constexpr int R = 2;
    Was r{};
    const int c_first = (x0 / 2) & ~7, c_last = x1 / 2;
    int nxw = (c_last - c_first + 64) / 64, tpb = 4;
    r.nxt = nxw;
    shape_for_tile_sweep(ld, x0, x1, y0, y1, &nxw, &tpb);
    const int strips = (y1 - y0 + R) / R;
    const unsigned grid = (unsigned)(((long)nxw * strips + tpb - 1) / tpb);
    r.c_first = c_first, r.nxw = nxw, r.tpb = tpb, r.groups = ((long)nxw * strips + tpb - 1) / tpb, r.grid = grid;
    const int h = y1 - y0 + 1;
    r.gx = (x1 - x0 + 256) / 256, r.gy = h > 4096 ? 4096 : h;
    return r;
}
static Was was_dlesm_stencil5_masked_f64(int ld, int x0, int x1, int y0, int y1)   // dlesm_masked.hip
{
    constexpr int R = 2;
    Was r{};
    const int c_first = (x0 / 2) & ~7, c_last = x1 / 2;
    int nxw = (c_last - c_first + 64) / 64, tpb = 4;
    r.nxt = nxw;
    shape_for_tile_sweep(ld, x0, x1, y0, y1, &nxw, &tpb);
    const int strips = (y1 - y0 + R) / R;
    const unsigned grid = (unsigned)(((long)nxw * strips + tpb - 1) / tpb);
    r.c_first = c_first, r.nxw = nxw, r.tpb = tpb, r.groups = ((long)nxw * strips + tpb - 1) / tpb, r.grid = grid;
    const int h = y1 - y0 + 1;
    r.gx = (x1 - x0 + 256) / 256, r.gy = h > 4096 ? 4096 : h;
    return r;
}
static Was was_dlesm_continuity_f64(int ld, int x0, int x1, int y0, int y1)        // dlesm_continuity.hip
{
    constexpr int R = 2;
    Was r{};
    const int c_first = (x0 / 2) & ~7, c_last = x1 / 2;
    int nxw = (c_last - c_first + 64) / 64, tpb = 4;
    r.nxt = nxw;
    shape_for_tile_sweep(ld, x0, x1, y0, y1, &nxw, &tpb);
    const int strips = (y1 - y0 + R) / R;
    const unsigned grid = (unsigned)(((long)nxw * strips + tpb - 1) / tpb);
    r.c_first = c_first, r.nxw = nxw, r.tpb = tpb, r.groups = ((long)nxw * strips + tpb - 1) / tpb, r.grid = grid;
    const int h = y1 - y0 + 1;
    r.gx = (x1 - x0 + 256) / 256, r.gy = h > 4096 ? 4096 : h;
    return r;
}
static Was was_launch_stencil9_framed(int x0, int x1, int y0, int y1)              // dlesm_stencil9.hip: the interior
{
    constexpr int R = 2;
    Was r{};
    const int c_first = (x0 / 2) & ~7, c_last = x1 / 2;
    int nxw = (c_last - c_first + 64) / 64, tpb = 4;
    r.nxt = nxw;
    choose_block_shape(&nxw, &tpb);
    const int strips = (y1 - y0 + R) / R;
    const unsigned grid = (unsigned)(((long)nxw * strips + tpb - 1) / tpb);
    r.c_first = c_first, r.nxw = nxw, r.tpb = tpb, r.groups = ((long)nxw * strips + tpb - 1) / tpb, r.grid = grid;
    return r;
}
static Was was_momentum_launch(int x0, int x1, int y0, int y1)                     // dlesm_momentum.hip
{
    constexpr int MR = 1;
    Was r{};
    const int c_first = (x0 / 2) & ~7, c_last = x1 / 2;
    int nxw = (c_last - c_first + 64) / 64, tpb = 4;
    r.nxt = nxw;
    choose_block_shape(&nxw, &tpb, 4);
    if (tpb > 4) tpb = 4;
    const int strips = (y1 - y0 + MR) / MR;
    const unsigned grid = (unsigned)(((long)nxw * strips + tpb - 1) / tpb);
    r.c_first = c_first, r.nxw = nxw, r.tpb = tpb, r.groups = ((long)nxw * strips + tpb - 1) / tpb, r.grid = grid;
    const int h = y1 - y0 + 1;
    r.gx = (x1 - x0 + 256) / 256, r.gy = h > 4096 ? 4096 : h;
    return r;
}
static Was was_next_ssh_launch(int x0, int x1, int y0, int y1)                     // dlesm_momentum.hip: one cell per thread only
{
    Was r{};
    const int h = y1 - y0 + 1;
    r.gx = (x1 - x0 + 256) / 256, r.gy = h > 4096 ? 4096 : h;
    return r;
}
static Was was_launch_kernel(int x0, int x1, int y0, int y1)                       // dlesm_shallow_kernels.hip
{
    Was r{};
    const int nx = x1 - x0 + 1, h = y1 - y0 + 1;
    constexpr int R = 2;
    const int cb = (x0 / 2) & ~7, c_last = x1 / 2;
    int nxw = (c_last - cb + 64) / 64, tpb = 4;
    r.nxt = nxw;
    choose_block_shape(&nxw, &tpb, 4);
    if (tpb > 8) tpb = 8;
    const int strips = (h + R - 1) / R;
    const unsigned grid = (unsigned)(((long)nxw * strips + tpb - 1) / tpb);
    r.c_first = cb, r.nxw = nxw, r.tpb = tpb, r.groups = ((long)nxw * strips + tpb - 1) / tpb, r.grid = grid;
    r.gx = (nx + 255) / 256, r.gy = h > 4096 ? 4096 : h;
    return r;
}
struct WasStepTiles {                                                              // dlesm_nemolite_step.hip
    int x0, x1, y0, y1;
    int c_first, nxt;
    long long tiles() const { return (long long)nxt * (y1 - y0 + 1); }
};
static WasStepTiles was_step_tiles(int x0, int x1, int y0, int y1)
{
    constexpr int TILE_CHUNKS = 63;
    WasStepTiles g{x0, x1, y0, y1, 0, 0};
    g.c_first = (g.x0 / 2) & ~7;
    g.nxt = (g.x1 / 2 - g.c_first + TILE_CHUNKS) / TILE_CHUNKS;
    return g;
}
// row_lo < 0: the launch of every tile; otherwise the flag map's, over the rows row_lo .. row_hi of the box
static Was was_step_impl(int x0, int x1, int y0, int y1, int row_lo, int row_hi)   // dlesm_nemolite_step.hip
{
    Was r{};
    const WasStepTiles g = was_step_tiles(x0, x1, y0, y1);
    int nxw = g.nxt, tpb = 4;
    choose_block_shape(&nxw, &tpb, 4);
    if (tpb > 4) tpb = 4;
    r.c_first = g.c_first, r.nxt = g.nxt, r.nxw = nxw, r.tpb = tpb;
    if (row_lo < 0) {
        const unsigned nblk = (unsigned)(((long)nxw * (g.y1 - g.y0 + 1) + tpb - 1) / tpb);
        r.groups = ((long)nxw * (g.y1 - g.y0 + 1) + tpb - 1) / tpb, r.grid = nblk;
    } else {
        const unsigned nblk = (unsigned)(((long)nxw * (row_hi - row_lo + 1) + tpb - 1) / tpb);
        r.groups = ((long)nxw * (row_hi - row_lo + 1) + tpb - 1) / tpb, r.grid = nblk;
    }
    return r;
}
static Was was_tracer_step(bool muscl, int x0, int x1, int y0, int y1)             // dlesm_tracer.hip: tracer_step + launch<NT>
{
    constexpr int TILE_CHUNKS = 63, MUSCL_CHUNKS = 62;
    Was r{};
    struct { int x0, x1, y0, y1, c_first, nxw, tpb; } l{x0, x1, y0, y1, 0, 0, 0};
    const int chunks = muscl ? MUSCL_CHUNKS : TILE_CHUNKS;
    l.c_first = (l.x0 / 2) & ~7;
    l.nxw = (l.x1 / 2 - l.c_first + chunks) / chunks, l.tpb = 4;
    r.nxt = l.nxw;
    choose_block_shape(&l.nxw, &l.tpb, 4);
    if (l.tpb > 4) l.tpb = 4;
    const int h = l.y1 - l.y0 + 1;
    const unsigned nblk = (unsigned)(((long)l.nxw * h + l.tpb - 1) / l.tpb);
    r.c_first = l.c_first, r.nxw = l.nxw, r.tpb = l.tpb, r.groups = ((long)l.nxw * h + l.tpb - 1) / l.tpb, r.grid = nblk;
    r.gx = (l.x1 - l.x0 + 256) / 256, r.gy = h > 4096 ? 4096 : h;
    return r;
}
static Was was_flow_output_launch(int x0, int x1, int y0, int y1)                  // dlesm_flow_output.hip
{
    constexpr int TILE_CHUNKS = 63;
    Was r{};
    const long long h = (long long)y1 - y0 + 1;
    const int c_first = (x0 / 2) & ~7;
    int nxw = (x1 / 2 - c_first + TILE_CHUNKS) / TILE_CHUNKS, tpb = 4;
    r.nxt = nxw;
    choose_block_shape(&nxw, &tpb, 4);
    if (tpb > 4) tpb = 4;
    const long long nblk = ((long long)nxw * h + tpb - 1) / tpb;
    r.refused = !(nblk <= INT_MAX);
    r.c_first = c_first, r.nxw = nxw, r.tpb = tpb, r.groups = nblk, r.grid = (unsigned)nblk;
    r.gx = (unsigned)((x1 - x0 + 256) / 256), r.gy = (unsigned)(h > 4096 ? 4096 : h);
    return r;
}
struct WasSweepPlan {                                                              // dlesm_record_reduce.h
    int c_first, nxw, tpb;
    int gx, gy;
    long long nrec;
};
static WasSweepPlan was_plan_sweep(int x0, int x1, long long rows, bool tile)
{
    constexpr int TILE_CHUNKS = 63;
    WasSweepPlan p{0, 0, 4, 0, 0, 0};
    if (rows <= 0) return p;
    if (tile) {
        p.c_first = (x0 / 2) & ~7;
        p.nxw = (x1 / 2 - p.c_first + TILE_CHUNKS) / TILE_CHUNKS;
        choose_block_shape(&p.nxw, &p.tpb, 4);
        if (p.tpb > 4) p.tpb = 4;
        p.nrec = ((long long)p.nxw * rows + p.tpb - 1) / p.tpb;
    } else {
        p.gx = (x1 - x0 + 256) / 256, p.gy = (int)(rows > 4096 ? 4096 : rows);
        p.nrec = (long long)p.gx * p.gy;
    }
    return p;
}

// the fit tests as they stood; m = the mask, f = the arrays (an entry the site skipped is null here too)
static bool was_fit_stencil9(int ld, const double *in, const double *out)
{
    return ld % 2 == 0 && (uintptr_t)in % 16 == 0 && (uintptr_t)out % 16 == 0;
}
static bool was_fit_masked(int ld, const double *in, const double *out, const int *tmask)
{
    return ld % 2 == 0 && (uintptr_t)in % 16 == 0 && (uintptr_t)out % 16 == 0 && (uintptr_t)tmask % 8 == 0;
}
static bool was_fit_continuity(int ld, const double *const *nine)
{
    bool aligned = ld % 2 == 0;
    for (int k = 0; k < 9; k++) aligned = aligned && (uintptr_t)nine[k] % 16 == 0;
    return aligned;
}
static bool was_lanes16_fit(int ld, const int *tmask, const double *const *ins, int n)        // recred::lanes16_fit; the loops
{                                                                                            // of momentum, the step, tracers
    bool ok = ld % 2 == 0 && (uintptr_t)tmask % 8 == 0;
    for (int k = 0; k < n; k++) ok = ok && (uintptr_t)ins[k] % 16 == 0;
    return ok;
}
static bool was_fit_flow_output(int ld, const int *tmask, const bool *need, const double *const *ins, const double *const *out)
{
    bool tile = ld % 2 == 0 && (uintptr_t)tmask % 8 == 0;
    for (int m = 0; m < 6; m++) tile = tile && (!need[m] || (uintptr_t)ins[m] % 16 == 0);
    for (int k = 0; k < 6; k++) tile = tile && (uintptr_t)out[k] % 16 == 0;
    return tile;
}
static bool was_sw_lanes16_fit(int ld, int east0, const double *const *f, int n)             // dlesm_internal.h
{
    bool ok = ld % 2 == 0 || east0 + 1 <= 2 * (ld / 2) - 1;
    for (int k = 0; k < n; k++) ok = ok && ((uintptr_t)f[k] % 16 == 0);
    return ok;
}
static bool was_fit_launch_kernel(int ld, int x1, bool east, const double *out, const double *const *in, int nin)
{
    bool aligned = ld % 2 == 0 || x1 + (east ? 1 : 0) <= 2 * (ld / 2) - 1;
    aligned = aligned && (uintptr_t)out % 16 == 0;
    for (int n = 0; n < nin; n++) aligned = aligned && (uintptr_t)in[n] % 16 == 0;
    return aligned;
}

// ---- the comparison ------------------------------------------------------------------------------------------------------

// the header's plan against a site's tile launch.  A site that cast its count to unsigned launched that grid; the header
// refuses a count above INT_MAX, where the cast had dropped bits or the site refused as well.
static int same_tiles(const Was &w, const TilePlan &p, long long groups)
{
    REQUIRE(p.c_first == w.c_first && p.nxt == w.nxt && p.nxw == w.nxw && p.tpb == w.tpb);
    REQUIRE(groups == w.groups);
    unsigned grid = 0;
    const int rc = sweep_grid("site", groups, &grid);
    if (w.groups <= INT_MAX) REQUIRE(rc == DLESM_OK && grid == w.grid && !w.refused);
    else REQUIRE(rc == DLESM_EINVAL);
    if (groups == p.groups() && groups <= INT_MAX) REQUIRE(p.grid == w.grid);      // what tile_plan itself left
    return 0;
}
static int same_direct(const Was &w, const DirectGrid &g)
{
    REQUIRE(g.x == w.gx && g.y == w.gy);
    return 0;
}

// the plan whether or not its grid was refused: same_tiles() looks at the refusal
static TilePlan plan(int ld, int x0, int x1, int y0, int y1, int chunks, int rows_per_tile, TileShape shape, int max_waves)
{
    TilePlan p;
    const int rc = tile_plan("site", ld, x0, x1, y0, y1, chunks, rows_per_tile, shape, max_waves, &p);
    if (rc != (p.groups() > INT_MAX ? DLESM_EINVAL : DLESM_OK)) p.c_first = -1;      // (no box has that: a comparison fails)
    return p;
}

static int sweep_box(int ld, int x0, int x1, int y0, int y1)
{
    g_ld = ld, g_x0 = x0, g_x1 = x1, g_y0 = y0, g_y1 = y1;
    const long long h = (long long)y1 - y0 + 1;
    const DirectGrid d = direct_grid(x0, x1, y0, y1);
    TilePlan p = plan(ld, x0, x1, y0, y1, CHUNKS_ALL, 2, SHAPE_PLANNED, 16);
    if (same_tiles(was_launch_stencil9(ld, x0, x1, y0, y1), p, p.groups()) || same_direct(was_launch_stencil9(ld, x0, x1, y0, y1), d))
        return 1;
    if (same_tiles(was_dlesm_stencil5_masked_f64(ld, x0, x1, y0, y1), p, p.groups()) ||
        same_direct(was_dlesm_stencil5_masked_f64(ld, x0, x1, y0, y1), d))
        return 1;
    if (same_tiles(was_dlesm_continuity_f64(ld, x0, x1, y0, y1), p, p.groups()) ||
        same_direct(was_dlesm_continuity_f64(ld, x0, x1, y0, y1), d))
        return 1;
    p = plan(ld, x0, x1, y0, y1, CHUNKS_ALL, 2, SHAPE_RULE, 16);
    if (same_tiles(was_launch_stencil9_framed(x0, x1, y0, y1), p, p.groups())) return 1;
    p = plan(ld, x0, x1, y0, y1, CHUNKS_ALL, 1, SHAPE_FOUR, 4);
    if (same_tiles(was_momentum_launch(x0, x1, y0, y1), p, p.groups()) || same_direct(was_momentum_launch(x0, x1, y0, y1), d))
        return 1;
    if (same_direct(was_next_ssh_launch(x0, x1, y0, y1), d)) return 1;
    p = plan(ld, x0, x1, y0, y1, CHUNKS_ALL, 2, SHAPE_FOUR, 8);
    if (same_tiles(was_launch_kernel(x0, x1, y0, y1), p, p.groups()) || same_direct(was_launch_kernel(x0, x1, y0, y1), d)) return 1;

    // the one-call step: the geometry alone (the wet plan, its check), every tile, the rows of the flag map
    const WasStepTiles g = was_step_tiles(x0, x1, y0, y1);
    p = tile_geometry(x0, x1, y0, y1, CHUNKS_EAST, 1);
    REQUIRE(p.c_first == g.c_first && p.nxt == g.nxt && p.tiles() == g.tiles());
    p = plan(ld, x0, x1, y0, y1, CHUNKS_EAST, 1, SHAPE_FOUR, 4);
    REQUIRE(p.tiles() == g.tiles());
    if (same_tiles(was_step_impl(x0, x1, y0, y1, -1, -1), p, p.groups())) return 1;
    const int row_lo = (int)(h / 3), row_hi = (int)(h - 1 - h / 5);
    if (same_tiles(was_step_impl(x0, x1, y0, y1, row_lo, row_hi), p, p.groups_for(row_hi - row_lo + 1))) return 1;

    if (same_tiles(was_tracer_step(false, x0, x1, y0, y1), p, p.groups()) || same_direct(was_tracer_step(false, x0, x1, y0, y1), d))
        return 1;
    if (same_tiles(was_flow_output_launch(x0, x1, y0, y1), p, p.groups()) || same_direct(was_flow_output_launch(x0, x1, y0, y1), d))
        return 1;
    const WasSweepPlan st = was_plan_sweep(x0, x1, h, true), sd = was_plan_sweep(x0, x1, h, false);
    REQUIRE(p.c_first == st.c_first && p.nxw == st.nxw && p.tpb == st.tpb && p.groups() == st.nrec);
    REQUIRE((int)d.x == sd.gx && (int)d.y == sd.gy && (long long)d.x * d.y == sd.nrec);
    p = plan(ld, x0, x1, y0, y1, CHUNKS_BOTH, 1, SHAPE_FOUR, 4);
    if (same_tiles(was_tracer_step(true, x0, x1, y0, y1), p, p.groups())) return 1;
    return 0;
}

static int sweep_fits()
{
    // pointer VALUES only, never dereferenced: 16-byte aligned, 8 off, 4 off (a mask), null
    auto D = [](uintptr_t v) { return (const double *)v; };
    auto M = [](uintptr_t v) { return (const int *)v; };
    const uintptr_t base = 0x10000;
    for (int ld : {164, 165, 2, 3})
        for (uintptr_t moff : {(uintptr_t)0, (uintptr_t)4, (uintptr_t)8, (uintptr_t)12})
            for (int bad = -1; bad < 24; bad++)            // which array is 8 bytes off (-1: none)
                for (int nullmask = 0; nullmask < 2; nullmask++) {
                    g_ld = ld, g_x0 = (int)moff, g_x1 = bad, g_y0 = nullmask, g_y1 = 0;
                    const double *a[24];
                    for (int k = 0; k < 24; k++) a[k] = D(base + 0x1000 * k + (k == bad ? 8 : 0));
                    const int *m = nullmask ? nullptr : M(0x8000 + moff);
                    REQUIRE(lanes16_fit(ld, nullptr, {a[0], a[1]}) == was_fit_stencil9(ld, a[0], a[1]));
                    REQUIRE(lanes16_fit(ld, m, {a[0], a[1]}) == was_fit_masked(ld, a[0], a[1], m));
                    REQUIRE(lanes16_fit(ld, nullptr, a, 9) == was_fit_continuity(ld, a));
                    for (int n : {0, 1, 6, 9, 20, 24}) REQUIRE(lanes16_fit(ld, m, a, n) == was_lanes16_fit(ld, m, a, n));
                    // a mask, a list, then further lists without one: momentum, the step, the tracers
                    REQUIRE((lanes16_fit(ld, m, a, 19) && lanes16_fit(ld, nullptr, a + 19, 5)) == was_lanes16_fit(ld, m, a, 24));
                    // optional arrays: the output fields skip an input no wanted output reads, and pass it as null
                    for (int skip = 0; skip < 64; skip += 7) {
                        bool need[6];
                        const double *ins[6], *given[6];
                        for (int q = 0; q < 6; q++)
                            need[q] = !((skip >> q) & 1), ins[q] = a[q], given[q] = need[q] ? a[q] : nullptr;
                        REQUIRE((lanes16_fit(ld, m, given, 6) && lanes16_fit(ld, nullptr, a + 6, 6)) ==
                                was_fit_flow_output(ld, m, need, ins, a + 6));
                    }
                    // the shallow-water rule: the east column at, inside and past the last whole chunk of an odd row
                    for (int east0 = ld - 4; east0 <= ld - 1; east0++) {
                        if (east0 < 0) continue;
                        REQUIRE(sw_lanes16_fit(ld, east0, a, 9) == was_sw_lanes16_fit(ld, east0, a, 9));
                        REQUIRE(sw_lanes16_fit(ld, east0, a, 12) == was_sw_lanes16_fit(ld, east0, a, 12));
                        for (int east = 0; east < 2; east++) {
                            const int x1 = east0 - east;       // launch_kernel passes x1 - (K::E ? 0 : 1)
                            if (x1 < 0) continue;
                            for (int nin = 2; nin <= 4; nin++)
                                REQUIRE((sw_lanes16_fit(ld, x1 - (east ? 0 : 1), a + 1, nin) && all_16_byte(a, 1)) ==
                                        was_fit_launch_kernel(ld, x1, east != 0, a[0], a + 1, nin));
                        }
                    }
                }
    return 0;
}

int main()
{
    static_assert(CHUNKS_ALL == 64 && CHUNKS_EAST == 63 && CHUNKS_BOTH == 62, "the chunk constants");
    const int heights[9] = {1, 2, 3, 7, 8, 4095, 4096, 4097, INT_MAX - 1};      // 2^31 - 2
    for (int x0 = 0; x0 <= 300; x0++)
        for (int x1 = x0; x1 <= x0 + 600; x1++)
            for (int h : heights)
                for (int odd = 0; odd < 2; odd++) {
                    const int y0 = h == INT_MAX - 1 ? 0 : 1 + (x1 & 1);
                    const int ld = ((x1 + 3) & ~1) + odd;              // the box and its ring fit; even, then odd
                    if (sweep_box(ld, x0, x1, y0, y0 + h - 1)) return 1;
                }
    if (sweep_fits()) return 1;

    // the refusal: at INT_MAX + 1 workgroups, not at INT_MAX, with the text the two sites that refused had
    g_ld = g_x0 = g_x1 = g_y0 = g_y1 = 0;
    unsigned grid = 0;
    clear_error();
    REQUIRE(sweep_grid("who", INT_MAX, &grid) == DLESM_OK && grid == (unsigned)INT_MAX && g_err[0] == 0);
    grid = 7;
    REQUIRE(sweep_grid("who", (long long)INT_MAX + 1, &grid) == DLESM_EINVAL && grid == 7);
    char want[128];
    snprintf(want, sizeof want, "%s: %lld workgroups in one sweep (at most %d)", "who", (long long)INT_MAX + 1, INT_MAX);
    REQUIRE(strcmp(g_err, want) == 0);
    REQUIRE(sweep_grid("who", 0, &grid) == DLESM_OK && grid == 0);

    printf("checks passed: %ld comparisons\n", checks);
    return 0;
}
