// The host side of every wave-tile sweep: where the tiles of a box lie, how many workgroups sweep them, and whether the arrays
// may be read in 16-byte lanes at all.  Host arithmetic only (no HIP header, no dim3): the launchers include it through
// dlesm_internal.h, tests/tile_plan_host.cpp includes it alone and compares it with the expressions it replaced.
//
// THE TWO TILE GEOMETRIES.  A wave tile is 64 lanes x one chunk of 2 columns (a 16-byte lane) x R rows.  Tile 0 of every row
// begins at chunk c_first = (x0 / 2) & ~7, the 128-byte line that holds the box's west column x0, so that every wave loads
// whole lines; the last chunk that holds a cell of the box is x1 / 2.
//   two rows (R = 2):  the Jacobi sweep's geometry -- the 3 x 3, masked and continuity sweeps, the shallow-water kernel set.
//                      Every lane owns its chunk, lanes 0 and 63 load the one column outside the wave: waves step by
//                      CHUNKS_ALL = 64 chunks.  A box of h rows has (h + 1) / 2 strips of tiles; the last may hold one row.
//   one row (R = 1):   the NEMOLite2D-class sweeps.  Momentum steps by 64 as above.  In the one-call step, the upwind tracers,
//                      the Courant checks and the output fields lane 63 only loads (its chunk is the next wave's lane 0):
//                      CHUNKS_EAST = 63.  The two-cell stencils (MUSCL, Hancock) make lane 0 load-only too: CHUNKS_BOTH = 62.
// A row holds nxt = (x1 / 2 - c_first + chunks) / chunks tiles.  The launch pads that to nxw >= nxt (a padding tile leaves at
// once); wave w takes tile w % nxw of strip w / nxw, tpb waves to a workgroup: (nxw * strips + tpb - 1) / tpb workgroups.
//
// THE THREE SHAPE RULES pick nxw and tpb; each kernel keeps the one it was measured with.
//   SHAPE_RULE     choose_block_shape(&nxw, &tpb): the rule fitted to the Jacobi sweep (a row a quarter of a workgroup off a
//                  multiple of 8 workgroups, dlesm_kernels.hip).
//   SHAPE_FOUR     choose_block_shape(&nxw, &tpb, 4): the same padding rule at the caller's measured 4 waves per workgroup.
//   SHAPE_PLANNED  shape_for_tile_sweep(ld, box, ...): the shape dlesm_stencil5_autotune_f64 measured for this (ld, box) if
//                  there is one, else SHAPE_RULE.  Two-row geometry only: the plan is keyed on it.
// The tuning keys (j5_tpb, j5_autoshape, j5_pad_tiles) can make any rule return up to 16 waves; max_waves, the kernel's launch
// bound in waves (4, 8, or 16 for the 1024-thread kernels), caps what is launched.
#ifndef DLESM_TILE_PLAN_H
#define DLESM_TILE_PLAN_H

#include <climits>
#include <cstdint>
#include <initializer_list>

#include "dlesm_error.h"

namespace dlesm {

// block shape (waves per workgroup, padded tiles per row) of a linear tile sweep (dlesm_kernels.hip)
void choose_block_shape(int *nxw_io, int *tpb_out, int prefer = 0);
// the same for a sweep with the Jacobi tile geometry over the 0-based box: the planned Jacobi shape of that (ld, box) if there is one
void shape_for_tile_sweep(int ld, int x0, int x1, int y0, int y1, int *nxw_io, int *tpb_out);
constexpr int CHUNKS_ALL = 64, CHUNKS_EAST = 63, CHUNKS_BOTH = 62;
enum TileShape { SHAPE_RULE, SHAPE_FOUR, SHAPE_PLANNED };

// a workgroup count as a grid extent; more than INT_MAX: refused -- beyond arrays that fit a device (LAB_NOTES.md section 5.30)
inline int sweep_grid(const char *who, long long groups, unsigned *grid)
{
    if (groups > INT_MAX) return fail(DLESM_EINVAL, "%s: %lld workgroups in one sweep (at most %d)", who, groups, INT_MAX);
    *grid = (unsigned)groups;
    return DLESM_OK;
}
struct TilePlan {
    int c_first, nxt, nxw, tpb;               // the first chunk of tile 0; tiles per row, unpadded and as launched; waves per workgroup
    long long rows_per_tile, rows;            // (rows: of the box)
    unsigned grid;            // groups() as a grid extent (tile_plan)
    long long strips(long long h) const { return (h + rows_per_tile - 1) / rows_per_tile; }
    long long tiles() const { return nxt * strips(rows); }                          // unpadded: what a tile map indexes
    long long groups_for(long long h) const { return (nxw * strips(h) + tpb - 1) / tpb; }   // a sub-range of h rows
    long long groups() const { return groups_for(rows); }                           // the workgroups of the sweep
};
// the geometry alone, for the box (x0:x1, y0:y1), 0-based inclusive and not empty: nxw = nxt, 4 waves
inline TilePlan tile_geometry(int x0, int x1, int y0, int y1, int chunks, int rows_per_tile)
{
    const int c_first = (x0 / 2) & ~7, nxt = (x1 / 2 - c_first + chunks) / chunks;
    return TilePlan{c_first, nxt, nxt, 4, rows_per_tile, (long long)y1 - y0 + 1, 0};
}
// ... with the launch shape and the grid (ld: read by SHAPE_PLANNED alone); refuses as sweep_grid does, *p filled all the same
inline int tile_plan(const char *who, int ld, int x0, int x1, int y0, int y1, int chunks, int rows_per_tile, TileShape shape,
                     int max_waves, TilePlan *p)
{
    *p = tile_geometry(x0, x1, y0, y1, chunks, rows_per_tile);
    if (shape == SHAPE_PLANNED) shape_for_tile_sweep(ld, x0, x1, y0, y1, &p->nxw, &p->tpb);
    else choose_block_shape(&p->nxw, &p->tpb, shape == SHAPE_FOUR ? 4 : 0);
    if (p->tpb > max_waves) p->tpb = max_waves;
    return sweep_grid(who, p->groups(), &p->grid);
}
// the one-cell-per-thread kernels: 256 columns to a workgroup, a thread walks its column by rows y0 + blockIdx.y, + gridDim.y, ...
struct DirectGrid { unsigned x, y; };
inline DirectGrid direct_grid(int x0, int x1, int y0, int y1)
{
    const long long h = (long long)y1 - y0 + 1;
    return DirectGrid{(unsigned)((x1 - x0 + 256) / 256), (unsigned)(h > 4096 ? 4096 : h)};
}
// ---- may a sweep take 16-byte lanes (the wave-tile kernel)?  A null pointer (no mask, an optional array not given) passes.
inline bool all_16_byte(const double *const *a, int n)
{
    bool ok = true;
    for (int k = 0; k < n; k++) ok = ok && (uintptr_t)a[k] % 16 == 0;
    return ok;
}
// the even-ld rule: every row starts on 16 bytes; the mask (4-byte elements) is read in 8-byte lanes
inline bool lanes16_fit(int ld, const int *mask, const double *const *a, int n)
{
    return ld % 2 == 0 && (uintptr_t)mask % 8 == 0 && all_16_byte(a, n);
}
inline bool lanes16_fit(int ld, const int *mask, std::initializer_list<const double *> a)
{
    return lanes16_fit(ld, mask, a.begin(), (int)a.size());
}
// The shallow-water rule: ld is even, or column east0 + 1 (0-based) -- the east neighbour of the last column the launch
// computes, east0 -- lies inside the last whole two-column chunk of a row (an odd ld: rows alternately 8-byte aligned).  east0
// is the caller's to say: xstop - 1 for a box, xstop - 2 for the interior of the framed step, xstop - 1 + ge for the grown box
// of the two-step distributed form, x1 - 1 for a kernel of the set (dlesm_shallow_kernels.hip) that reads no east neighbour.
inline bool sw_lanes16_fit(int ld, int east0, const double *const *f, int n)
{
    return (ld % 2 == 0 || east0 + 1 <= 2 * (ld / 2) - 1) && all_16_byte(f, n);
}

} // namespace dlesm

#endif
