/*
 * dlesm_hip.h -- C ABI of the MI355X-native dl_esm_inf hot path.
 *
 * Everything a host language binds is declared here: plain C, plain pointers
 * and sizes, no C++ or torch types.  The Fortran side binds these through
 * ISO_C_BINDING (dl_esm_inf_amd/fortran/dlesm_hip_mod.f90), Python through
 * ctypes (dl_esm_inf_amd/_cabi.py).  INTEGRATION.md shows the stub a
 * maintainer of stfc/dl_esm_inf would add.
 *
 * Each entry cites the reference interface it replaces; paths are relative to
 * the reference's finite_difference/src/ directory.
 *
 * Conventions
 *   - all grid indices are 1-based and inclusive, exactly as in the Fortran;
 *   - a field is a column-major array data(1:ld, 1:ny) of doubles
 *     (field_mod.f90:350); element (ji,jj) lives at (jj-1)*ld + (ji-1);
 *   - functions return 0 on success, a negative DLESM_E* code otherwise;
 *     dlesm_last_error() gives the text.  Nothing falls back to the CPU:
 *     device entry points fail with DLESM_ENODEV when there is no GPU.
 *   - `stream` arguments are hipStream_t handles passed as void*; NULL is the
 *     HIP null stream.  Device entry points are asynchronous on that stream
 *     unless stated otherwise.
 *   - hipGraph capture: the kernel entries, the halo exchange and the distributed steps may be
 *     called on a stream that is being captured (hipStreamBeginCapture), so that a whole time loop
 *     replays as one graph launch.  Planning calls, checksums, gathers and anything documented as
 *     synchronising may not.  Under capture a distributed step forks to the library's side stream
 *     and joins back inside the graph (the *_pipelined form then equals the joined form); run the
 *     call once uncaptured first -- pack buffers are allocated on first use.  On a plan whose
 *     mailboxes are connected (peer transport, section 5) the captured operations are the ordinary
 *     single launches -- no RCCL call in the graph, *_pipelined stays the time-loop form -- and a
 *     graph has to hold an EVEN number of mailbox operations of a plan (see there).
 */
#ifndef DLESM_HIP_H
#define DLESM_HIP_H

#include <stdbool.h>
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DLESM_VERSION 310   /* round 3: entries added (the GOcean shallow kernels one by one, time_smooth, fused periodic step, plan description; 310: the peer transport, mailbox mode, the board); no signature changed */

/* error codes */
#define DLESM_OK 0
#define DLESM_EINVAL (-1)   /* bad argument / shape mismatch              */
#define DLESM_ENODEV (-2)   /* no usable HIP device                       */
#define DLESM_EHIP (-3)     /* a HIP runtime call failed                  */
#define DLESM_ERCCL (-4)    /* an RCCL call failed                        */
#define DLESM_EABORT (-5)   /* the reference aborts (gocean_stop) here    */
#define DLESM_ECOMMS (-12)  /* comm list overflow, parallel_comms_mod.f90:1223 */

/* enumerations shared with the Fortran API (values are the reference's) */
enum { DLESM_U_POINTS = 0, DLESM_V_POINTS = 1, DLESM_T_POINTS = 2,
       DLESM_F_POINTS = 3, DLESM_ALL_POINTS = 4 };            /* field_mod.f90:47-52 */
enum { DLESM_OFFSET_SW = 0, DLESM_OFFSET_SE = 1, DLESM_OFFSET_NW = 2,
       DLESM_OFFSET_NE = 3, DLESM_OFFSET_ANY = 4 };           /* grid_mod.f90:52-60  */
enum { DLESM_BC_PERIODIC = 0, DLESM_BC_EXTERNAL = 1, DLESM_BC_NONE = 2 }; /* grid_mod.f90:64-69 */
/* halo-exchange direction codes, parallel_comms_mod.f90:101-110 */
enum { DLESM_IPLUS = 1, DLESM_IMINUS = 2, DLESM_JPLUS = 3, DLESM_JMINUS = 4,
       DLESM_IPLUSJPLUS = 5, DLESM_IMINUSJMINUS = 6, DLESM_IPLUSJMINUS = 7,
       DLESM_IMINUSJPLUS = 8 };

/* region_mod.f90:7-12 -- member order matches the Fortran type so that
 * type(region_type) can be passed by reference. */
typedef struct dlesm_region {
    int nx, ny;
    int xstart, xstop;
    int ystart, ystop;
} dlesm_region;

/* decomposition_mod.f90:44-50 */
typedef struct dlesm_subdomain {
    dlesm_region global;   /* internal part in global coordinates; nx,ny = WHOLE extent */
    dlesm_region internal; /* internal part in local coordinates                        */
} dlesm_subdomain;

/* scalar part of decomposition_mod.f90:54-68 */
typedef struct dlesm_decomp {
    int global_nx, global_ny; /* size of the decomposed domain        */
    int nx, ny;               /* grid of subdomains                   */
    int ndomains;
    int max_width, max_height;
} dlesm_decomp;

#define DLESM_MAXCOMM 16 /* parallel_comms_mod.f90:70 */

/* One rank's message lists: the public tables of parallel_comms_mod.f90:71-83,156-161.
 * destination/source are 0-based ranks, coordinates are local 1-based. */
typedef struct dlesm_comm_tables {
    int nsend, nrecv;
    int dirsend[DLESM_MAXCOMM], destination[DLESM_MAXCOMM];
    int isrcsend[DLESM_MAXCOMM], jsrcsend[DLESM_MAXCOMM];
    int idessend[DLESM_MAXCOMM], jdessend[DLESM_MAXCOMM];
    int nxsend[DLESM_MAXCOMM], nysend[DLESM_MAXCOMM];
    int dirrecv[DLESM_MAXCOMM], source[DLESM_MAXCOMM];
    int isrcrecv[DLESM_MAXCOMM], jsrcrecv[DLESM_MAXCOMM];
    int idesrecv[DLESM_MAXCOMM], jdesrecv[DLESM_MAXCOMM];
    int nxrecv[DLESM_MAXCOMM], nyrecv[DLESM_MAXCOMM];
} dlesm_comm_tables;

/* ------------------------------------------------------------------------
 * 1. Host-side index maps (no GPU needed; bit-exact with the reference)
 * ---------------------------------------------------------------------- */

/* grid_init's DL_ESM_ALIGNMENT block, grid_mod.f90:349-363: parse the
 * environment variable.  *alignment = 1 when unset.  DLESM_EABORT when the
 * reference would gocean_stop (more than 3 characters, not a positive int). */
int dlesm_alignment_from_env(int *alignment);

/* grid_mod.f90:364-385: allocated extents of every field on a subdomain whose
 * whole size is sub_global_nx x sub_global_ny. */
int dlesm_grid_extents(int sub_global_nx, int sub_global_ny, int alignment, int *nx, int *ny);

/* set_field_bounds + c{u,v,t,f}_{sw,ne}_init + field_init, field_mod.f90:563-1122.
 * DLESM_EABORT for the combinations on which the reference stops. */
int dlesm_field_bounds(int grid_points, int offset, int bc_x, int bc_y,
                       const dlesm_region *subdomain_internal, int grid_nx, int grid_ny,
                       dlesm_region *internal, dlesm_region *whole);

/* init_periodic_bc_halos, field_mod.f90:1394-1464: the (source, destination) regions of the
 * periodic-boundary copies of a field with the given internal region, in the reference's order
 * (x pair first, then the y pair over the widened columns).  source/dest hold 4 entries;
 * *num_halos = 0, 2 or 4.  The region's nx, ny members are filled with the extents. */
int dlesm_periodic_halos(const dlesm_region *internal, int bc_x, int bc_y, dlesm_region *source,
                         dlesm_region *dest, int *num_halos);

/* go_decompose, parallel_mod.f90:70-332.  ntilex,ntiley <= 0 selects the
 * reference's automatic tiling.  subdomains must hold ndomains entries. */
int dlesm_decompose(int domainx, int domainy, int ndomains, int ntilex, int ntiley,
                    int halo_width, dlesm_decomp *decomp, dlesm_subdomain *subdomains);

/* iprocmap, parallel_comms_mod.f90:1365-1398 (1-based owner, 0 if none) */
int dlesm_iprocmap(const dlesm_decomp *decomp, const dlesm_subdomain *subdomains,
                   int nranks, int ia, int ja);

/* map_comms, parallel_comms_mod.f90:178-1172, for rank `rank1` (1-based, as
 * get_rank() returns it, parallel_utils_mod.f90:84). */
int dlesm_map_comms(const dlesm_decomp *decomp, const dlesm_subdomain *subdomains,
                    int nranks, int rank1, dlesm_comm_tables *tables);

/* Extension (the reference aborts beyond MAX_HALO_DEPTH = 1, parallel_comms_mod.f90:48,
 * 220-222): tables of a depth-`depth` exchange -- same neighbours, direction codes and order,
 * strips `depth` cells deep against the internal region, corners depth x depth.  Needs a
 * decomposition made with halo_width >= depth and tiles at least `depth` wide and high. */
int dlesm_map_comms_depth(const dlesm_decomp *decomp, const dlesm_subdomain *subdomains,
                          int nranks, int rank1, int depth, dlesm_comm_tables *tables);

/* ------------------------------------------------------------------------
 * 2. Runtime
 * ---------------------------------------------------------------------- */

const char *dlesm_last_error(void);
int dlesm_version(void);

/* number of visible HIP devices (0 when there is none; never an error) */
int dlesm_device_count(void);

/* Bind this process to a device -- the HIP counterpart of
 * acc_init(acc_device_nvidia) in gocean_initialise, gocean_mod.F90:31-33.
 * Creates the library's side stream and events.  Idempotent. */
int dlesm_init(int device);
int dlesm_finalize(void);

/* ------------------------------------------------------------------------
 * 3. Device-resident fields and the reference's device-sync callbacks
 * ---------------------------------------------------------------------- */

/* What r2d_field%device_ptr (field_mod.f90:153) points at: an opaque
 * descriptor that remembers the device buffer and its row stride, which the
 * C-flavour callbacks below are not told. */
typedef struct dlesm_field dlesm_field;

/* allocate ld*ny doubles on the device and zero them (field_mod.f90:350,375) */
int dlesm_field_create(int ld, int ny, dlesm_field **field);
/* describe device memory owned by the caller (e.g. a torch tensor) */
int dlesm_field_wrap(void *device_data, int ld, int ny, dlesm_field **field);
int dlesm_field_destroy(dlesm_field *field);
double *dlesm_field_data(const dlesm_field *field); /* raw device pointer */
int dlesm_field_ld(const dlesm_field *field);
int dlesm_field_ny(const dlesm_field *field);

/* read_from_device_c_interface / write_to_device_c_interface,
 * field_mod.f90:65-73 and 86-94, with exactly that argument list:
 *   read : from = device_ptr (dlesm_field*), to = C_LOC(host data)
 *   write: from = C_LOC(host data),          to = device_ptr (dlesm_field*)
 * startx,starty are 1-based, nx,ny the extent of the patch.  Assign them to
 * fld%read_from_device_c / fld%write_to_device_c.  Errors abort the process
 * (the reference's error model: gocean_stop, gocean_mod.F90:50-57). */
void dlesm_read_from_device(void *from, void *to, int startx, int starty, int nx, int ny,
                            bool blocking);
void dlesm_write_to_device(void *from, void *to, int startx, int starty, int nx, int ny,
                           bool blocking);
/* wait for non-blocking transfers issued by the two callbacks */
int dlesm_transfer_sync(void);

/* ------------------------------------------------------------------------
 * 4. Kernels over a 1-based inclusive index box (the PSy-layer loop nest
 *    `do jj = ystart,ystop ; do ji = xstart,xstop ; call kern_code(ji,jj,...)`,
 *    form: infrastructure_mod.f90:32-41, bounds: field_mod.f90:116-119).
 *    Raw device pointers; ld,ny describe every array passed.
 * ---------------------------------------------------------------------- */

/* out(ji,jj) = 0.25*((in(ji-1,jj)+in(ji+1,jj)) + (in(ji,jj-1)+in(ji,jj+1))) */
int dlesm_stencil5_f64(const double *in, double *out, int ld, int ny,
                       int xstart, int xstop, int ystart, int ystop, void *stream);

/* The same step, reporting how far it moved the field: with d = out - in over the box (xstart:xstop, ystart:ystop),
 *   norm = DLESM_NORM_MAX:   max |d|  -- exact; a NaN d gives NaN (as numpy.max; fmax would drop it), an infinite one inf;
 *   norm = DLESM_NORM_SUMSQ: SUM d*d  -- summed in an order fixed by (ld, box, lane width) alone: the launch shape, the
 *                            planning call and the padding do not change its bits (16- or 8-byte lanes may).
 * `out` is bit for bit what dlesm_stencil5_f64 writes, and no other cell changes.  *result_dev -- device memory, or host
 * memory the device can write (hipHostMalloc) -- receives the value when `stream` gets there, with no host
 * synchronisation; the scratch space is stream-ordered, as for dlesm_checksum_async_f64.  An empty box writes 0.0 and
 * launches no sweep.  DLESM_EINVAL, before anything is launched: a box that does not fit with its one-cell ring,
 * in == out, a null result_dev, a result_dev inside `in` or `out`, an unknown norm.  Combine across ranks with
 * dlesm_global_max_f64 / dlesm_global_sum_f64.  Not callable under stream capture. */
enum { DLESM_NORM_MAX = 0, DLESM_NORM_SUMSQ = 1 };
int dlesm_stencil5_resid_f64(const double *in, double *out, int ld, int ny,
                             int xstart, int xstop, int ystart, int ystop,
                             int norm, double *result_dev, void *stream);

/* Optional planning call for dlesm_stencil5_f64 (in the manner of an FFT plan): times about a dozen
 * launch shapes (waves per workgroup, tiles per row, rows per tile) on the caller's own arrays -- each
 * is the same valid step in -> out, the results do not depend on the shape -- and remembers the fastest
 * for later calls with this (ld, box).  Synchronises `stream`.  Without it a fitted rule picks the shape. */
int dlesm_stencil5_autotune_f64(const double *in, double *out, int ld, int ny,
                                int xstart, int xstop, int ystart, int ystop, void *stream);
/* What the planning call kept for this (ld, box): waves per workgroup, wave tiles per row, rows per
 * tile (all 0 when no planning call has been made for it), and whether `out` is stored non-temporally
 * (by size: on from 150 MB per array, when a ping-pong pair no longer fits the 256 MB Infinity Cache).  Host only; for logs and profiles. */
int dlesm_stencil5_planned_shape(int ld, int xstart, int xstop, int ystart, int ystop,
                                 int *waves_per_group, int *tiles_per_row, int *rows_per_tile,
                                 int *nt_stores);

/* TWO Jacobi steps in one sweep (temporal blocking; SURVEY section 8 f.4 -- an extension,
 * the reference stops at MAX_HALO_DEPTH = 1, parallel_comms_mod.f90:48):
 *   t   = J(in) on the intermediate box (exstart:exstop, eystart:eystop), in elsewhere
 *   out = J(t)  on the box (xstart:xstop, ystart:ystop)
 * bit-identical to two dlesm_stencil5_f64 calls through a buffer that equals `in` outside the
 * intermediate box.  One tile: intermediate box = box (fixed boundary ring).  Distributed:
 * the box grown by one cell towards each neighbouring tile, `in` holding depth-2 halos. */
int dlesm_stencil5_x2_f64(const double *in, double *out, int ld, int ny,
                          int xstart, int xstop, int ystart, int ystop,
                          int exstart, int exstop, int eystart, int eystop, void *stream);

/* nsteps (2..8) Jacobi steps in one sweep:
 *   t_0 = in;  t_s = J(t_{s-1}) on the stage box E_s, t_{s-1} elsewhere (s = 1..nsteps-1);
 *   out = J(t_{nsteps-1}) on the box.
 * (exstart:exstop, eystart:eystop) is the LAST stage box E_{nsteps-1}; E_s is that box grown by
 * (nsteps-1-s) cells on every side whose grow_* flag is 1 (W, E, S, N = towards lower i, higher
 * i, lower j, higher j).  One tile: stage box = box, flags 0.  A tile with neighbours: stage
 * box = box grown by 1 towards each neighbour, flag 1 there, `in` holding depth-nsteps halos.
 * Bit-identical to nsteps dlesm_stencil5_f64 calls. */
int dlesm_stencil5_multi_f64(const double *in, double *out, int ld, int ny, int nsteps,
                             int xstart, int xstop, int ystart, int ystop,
                             int exstart, int exstop, int eystart, int eystop,
                             int grow_w, int grow_e, int grow_s, int grow_n, void *stream);

/* A general 9-point (3 x 3) weighted stencil -- the loop nest of any kernel of the form
 *   out(ji,jj) = SUM_{dj,di = -1..1} coef(di,dj) * in(ji+di, jj+dj)
 * (go_arg(GO_READ, GO_CT, GO_STENCIL(111,111,111)) + nine real scalars, argument_mod.f90:39-112).
 * coef[(dj+1)*3 + (di+1)]: south-west, south, south-east, west, centre, east, north-west, north,
 * north-east -- the storage order of a Fortran coef(-1:1,-1:1).  Five-point kernels pass zero corners.
 * Evaluation order: out = ((c_sw*sw + c_s*s) + c_se*se  +  (c_w*w + c_c*c) + c_e*e)
 * + ((c_nw*nw + c_n*n) + c_ne*ne), each row left to right, rows south to north, no FMA contraction. */
int dlesm_stencil9_f64(const double *in, double *out, const double *coef, int ld, int ny,
                       int xstart, int xstop, int ystart, int ystop, void *stream);

/* The same loop nest for a kernel that requests a GRID PROPERTY: the T-point land/sea mask
 * (GO_GRID_MASK_T in the kernel metadata, argument_mod.f90:75-112; the PSy layer passes
 * grid%tmask, here its device mirror grid%tmask_device, grid_mod.f90:104-106).  tmask is a
 * default-integer array with the field layout, > 0 = wet.  Dry points carry their value over;
 * a dry neighbour of a wet point is mirrored (no-flux coast):
 *   out = tmask(ji,jj) > 0 ? 0.25*((w+e)+(s+n)) : in(ji,jj),  w = tmask(ji-1,jj) > 0 ? in(ji-1,jj) : in(ji,jj), ... */
int dlesm_stencil5_masked_f64(const double *in, double *out, const int *tmask, int ld, int ny,
                              int xstart, int xstop, int ystart, int ystop, void *stream);

/* A kernel on all three C-grid point types that also takes a double-precision GRID PROPERTY
 * (GO_GRID_AREA_T, argument_mod.f90:75-112; the PSy layer passes grid%area_t, on the device its mirror
 * grid%area_t_device, grid_mod.f90:104-150): the free-surface (continuity) update of a NEMOLite2D-class
 * model over the box,
 *   r1 = (sshn_u(ji,jj)+hu(ji,jj))*un(ji,jj)         r2 = the same at (ji-1,jj)
 *   r3 = (sshn_v(ji,jj)+hv(ji,jj))*vn(ji,jj)         r4 = the same at (ji,jj-1)
 *   ssha(ji,jj) = sshn_t(ji,jj) + (((r2 - r1) + r4) - r3) * rdt / area_t(ji,jj)
 * (specification frozen in DESIGN.md section 5.10; the reference holds no such loop).  72 B/cell.
 * ssha may alias sshn_t only. */
int dlesm_continuity_f64(double rdt, int ld, int ny, int xstart, int xstop, int ystart, int ystop,
                         const double *sshn_t, const double *sshn_u, const double *sshn_v,
                         const double *hu, const double *hv, const double *un, const double *vn,
                         const double *area_t, double *ssha, void *stream);

/* The momentum update and the interpolation of the sea-surface height onto u and v points of a NEMOLite2D-class model:
 * the kernels that read the metric grid properties (GO_GRID_DX_U, GO_GRID_DY_U/V, GO_GRID_AREA_U/V and, through the
 * Coriolis parameter, GO_GRID_LAT_U/V; argument_mod.f90:75-112).  Specification frozen in DESIGN.md section 6.5 (the
 * reference holds none of these loops): NE offset, every operation rounded in double precision in the order the
 * parentheses give.  Boxes are 1-based and inclusive and need a one-cell ring inside the array; a cell the rule does not
 * write keeps its content, nothing outside the box is written.  No output may overlap any input, and ua may not overlap
 * va (DLESM_EINVAL).  Constants of the time step: */
typedef struct dlesm_momentum_params {
    double rdt, cbfr, visc, g;
} dlesm_momentum_params;
/* Device copies of the grid properties the momentum kernels read, all with the field layout (tmask: int32).  fcor_u/v are
 * the Coriolis parameter at u / v points, (2*omega)*sin(gphiu/v*d2r), computed on the host once per grid (DESIGN.md
 * section 6.5).  A loop nest reads only the arrays its rule names; the others may be NULL. */
typedef struct dlesm_momentum_grid {
    const int *tmask;
    const double *dx_t, *dy_t, *dx_u, *dy_u, *dx_v, *dy_v, *area_u, *area_v, *fcor_u, *fcor_v;
} dlesm_momentum_grid;
/* momentum_u over the box: ua(i,j) where tmask(i,j) > 0 and tmask(i+1,j) > 0.  140 B/cell. */
int dlesm_momentum_u_f64(const dlesm_momentum_params *params, const dlesm_momentum_grid *grid, int ld, int ny,
                         int xstart, int xstop, int ystart, int ystop,
                         const double *un, const double *vn, const double *ht, const double *sshn_t,
                         const double *hu, const double *sshn_u, const double *hv, const double *sshn_v,
                         const double *ssha_u, double *ua, void *stream);
/* momentum_v over the box: va(i,j) where tmask(i,j) > 0 and tmask(i,j+1) > 0.  140 B/cell. */
int dlesm_momentum_v_f64(const dlesm_momentum_params *params, const dlesm_momentum_grid *grid, int ld, int ny,
                         int xstart, int xstop, int ystart, int ystop,
                         const double *un, const double *vn, const double *ht, const double *sshn_t,
                         const double *hu, const double *sshn_u, const double *hv, const double *sshn_v,
                         const double *ssha_v, double *va, void *stream);
/* Both loop nests in one sweep: bit for bit dlesm_momentum_u_f64 over ubox (the U-point internal
 * region) followed by dlesm_momentum_v_f64 over vbox (the V-point internal region).  180 B/cell instead of 2 x 140. */
int dlesm_momentum_f64(const dlesm_momentum_params *params, const dlesm_momentum_grid *grid, int ld, int ny,
                       const dlesm_region *ubox, const dlesm_region *vbox,
                       const double *un, const double *vn, const double *ht, const double *sshn_t,
                       const double *hu, const double *sshn_u, const double *hv, const double *sshn_v,
                       const double *ssha_u, const double *ssha_v, double *ua, double *va, void *stream);
/* next_sshu / next_sshv: the sea-surface height at u (v) points from sshn_t, area-weighted where
 * both T cells are wet, the wet side's value on a coast, unwritten between two dry cells. */
int dlesm_next_sshu_f64(int ld, int ny, int xstart, int xstop, int ystart, int ystop, const int *tmask,
                        const double *area_t, const double *area_u, const double *sshn_t, double *sshn_u, void *stream);
int dlesm_next_sshv_f64(int ld, int ny, int xstart, int xstop, int ystart, int ystop, const int *tmask,
                        const double *area_t, const double *area_v, const double *sshn_t, double *sshn_v, void *stream);

/* The open boundary of a NEMOLite2D-class model: bc_ssh, the tidal sea-surface height on open T cells,
 * and the Flather condition on u and v faces.  "Open" is tmask < 0, "wet" tmask > 0.  A plan holds three lists of linear
 * indices in HBM, made once per grid from the host mask: the open T cells of tbox, the open u faces of ubox and the open v
 * faces of vbox (a face is open when one of its two T cells is open and the other wet), each face with its inner face (across
 * the wet cell) and its open T cell.  Boxes are 1-based and inclusive; ubox and vbox need a one-cell ring inside the array,
 * an empty box gives an empty list.  Refused with DLESM_EINVAL: a box that does not fit, an open face whose inner face or
 * either of that face's T cells lies outside the array, and an open face whose inner face is itself open (a wet region one
 * cell wide between two open cells).  A mask with no open cell gives empty lists, and the entries below then launch nothing. */
typedef struct dlesm_obc dlesm_obc;
int dlesm_obc_create(const int *tmask_host, int ld, int ny, const dlesm_region *tbox, const dlesm_region *ubox,
                     const dlesm_region *vbox, dlesm_obc **plan);
int dlesm_obc_destroy(dlesm_obc *plan);
/* the lengths of the plan's three lists (host only) */
int dlesm_obc_counts(const dlesm_obc *plan, int *nt, int *nu, int *nv);
/* bc_ssh: ssha = ssh_bc on every open T cell of the plan.  ssh_bc is a host scalar (amp*sin(omega*t), computed by the
 * caller with the host's sin: the kernel evaluates no transcendental). */
int dlesm_bc_ssh_f64(const dlesm_obc *plan, double ssh_bc, double *ssha, void *stream);
/* Flather on the open u (v) faces of the plan, with c = sqrt(g/hu(i,j)) and g = params->g: open side west (south), inner face
 * iu = i+1: ua(i,j) = ua(iu,j) - c*(sshn_u(iu,j) - sshn_t(o)); open side east (north), iu = i-1: ua(iu,j) + c*(...).
 * ua is written in place; it may not overlap hu, sshn_u or sshn_t (DLESM_EINVAL). */
int dlesm_bc_flather_u_f64(const dlesm_obc *plan, const dlesm_momentum_params *params, const double *hu, const double *sshn_u,
                           const double *sshn_t, double *ua, void *stream);
int dlesm_bc_flather_v_f64(const dlesm_obc *plan, const dlesm_momentum_params *params, const double *hv, const double *sshn_v,
                           const double *sshn_t, double *va, void *stream);
/* All three lists in one launch: bit for bit dlesm_bc_ssh_f64, dlesm_bc_flather_u_f64 and dlesm_bc_flather_v_f64.  No output
 * may overlap an input, and ssha, ua and va may not overlap each other (DLESM_EINVAL). */
int dlesm_bc_open_f64(const dlesm_obc *plan, const dlesm_momentum_params *params, double ssh_bc, const double *hu,
                      const double *sshn_u, const double *hv, const double *sshn_v, const double *sshn_t, double *ssha,
                      double *ua, double *va, void *stream);

/* One NEMOLite2D-class time step in one call: bit for bit the sequence
 *   dlesm_continuity_f64 over tbox (rdt = params->rdt) -> dlesm_next_sshu_f64 over ubox and dlesm_next_sshv_f64 over vbox
 *   (reading ssha) -> dlesm_momentum_f64 over ubox / vbox (reading ssha_u / ssha_v) -> dlesm_bc_open_f64(obc, params, ssh_bc,
 *   ...) when obc is not NULL (NULL: a closed basin, no boundary pass).
 * Every cell of every array is written where that sequence writes it and keeps its content elsewhere.  ssha is in/out:
 * next_ssh* read ssha(xstop+1, j) and ssha(i, ystop+1) in the ring, which continuity does not write; the call reads them
 * from ssha.  tbox == ubox == vbox (every NE grid) with an even ld and 16-byte aligned arrays is one sweep, 196 B/cell
 * against 324 for the sequence; anything else runs the sequence itself.  No output may overlap an input (tmask, area_t,
 * the grid arrays and the ten fields), and ssha, ssha_u, ssha_v, ua and va may not overlap each other (DLESM_EINVAL,
 * refused before anything is launched); the plan must have been made for ld x ny arrays.  Single domain, rank-local: on a
 * decomposed grid the sequence needs an ssha halo exchange between continuity and next_ssh*, which one call cannot hold. */
int dlesm_nemolite_step_f64(const dlesm_momentum_params *params, const dlesm_momentum_grid *grid, const double *area_t,
                            int ld, int ny, const dlesm_region *tbox, const dlesm_region *ubox, const dlesm_region *vbox,
                            const dlesm_obc *obc, double ssh_bc, const double *un, const double *vn, const double *ht,
                            const double *hu, const double *hv, const double *sshn_t, const double *sshn_u,
                            const double *sshn_v, double *ssha, double *ssha_u, double *ssha_v, double *ua, double *va,
                            void *stream);

/* Land: a wet plan marks the wave tiles of the one-sweep step over `box` in which the sweep would
 * store nothing but ssha on T == 0 cells -- no cell (i,j) of the tile inside the box has T(i,j) != 0, T(i+1,j) > 0 or
 * T(i,j+1) > 0 -- and dlesm_nemolite_step_wet_f64 leaves those tiles out.  The plan is made once from the HOST mask, which must
 * be the mask grid->tmask holds on the device when the plan is used: that is the caller's responsibility, the library
 * cannot check it.  box is the T box the step will be called with (1-based, inclusive, a one-cell ring inside the array; an
 * empty box gives a plan of no tiles).  The tile geometry is internal; dlesm_wet_plan_counts shows the number of tiles of the
 * box and how many of them are active.  DLESM_EINVAL: null pointers, a box that does not fit, more tiles than an int32 holds. */
typedef struct dlesm_wet_plan dlesm_wet_plan;
int dlesm_wet_plan_create(const int *tmask_host, int ld, int ny, const dlesm_region *box, dlesm_wet_plan **plan);
int dlesm_wet_plan_destroy(dlesm_wet_plan *plan);
int dlesm_wet_plan_counts(const dlesm_wet_plan *plan, long long *tiles, long long *active);
/* dlesm_nemolite_step_f64 that skips land.  wet == NULL: dlesm_nemolite_step_f64, bit for bit in every cell.  Otherwise, after
 * the call ssha_u, ssha_v, ua and va hold in EVERY cell what dlesm_nemolite_step_f64 leaves; ssha does so in every cell with
 * T != 0 and in every cell outside tbox; a T == 0 cell of tbox holds either that value or its content from before the call.
 * Stale land values of ssha are never read by a written cell, in this step or after the caller rotates ssha into sshn_t
 * (section 6.9).  With every tile active the call launches exactly the kernel and shape of dlesm_nemolite_step_f64; with none,
 * nothing but bc_open.  The definition path (unequal boxes, an odd ld, unaligned bases, the HOOK key nemo_step_kernel) ignores
 * the plan.  DLESM_EINVAL before anything is launched: a plan made for other (ld, ny) or for a box other than tbox, and
 * every refusal of dlesm_nemolite_step_f64. */
int dlesm_nemolite_step_wet_f64(const dlesm_wet_plan *wet, const dlesm_momentum_params *params,
                                const dlesm_momentum_grid *grid, const double *area_t, int ld, int ny,
                                const dlesm_region *tbox, const dlesm_region *ubox, const dlesm_region *vbox,
                                const dlesm_obc *obc, double ssh_bc, const double *un, const double *vn, const double *ht,
                                const double *hu, const double *hv, const double *sshn_t, const double *sshn_u,
                                const double *sshn_v, double *ssha, double *ssha_u, double *ssha_v, double *ua, double *va,
                                void *stream);

/* Shallow-water u/v/h update: reads u,v,p (3x3 footprint)
 * and uold,vold,pold, writes unew,vnew,pnew on the box. */
typedef struct dlesm_sw_params {
    double fsdx, fsdy;            /* 4/dx, 4/dy            */
    double tdts8, tdtsdx, tdtsdy; /* tdt/8, tdt/dx, tdt/dy */
} dlesm_sw_params;
int dlesm_shallow_step_f64(const dlesm_sw_params *params, int ld, int ny,
                           int xstart, int xstop, int ystart, int ystop,
                           const double *u, const double *v, const double *p,
                           const double *uold, const double *vold, const double *pold,
                           double *unew, double *vnew, double *pnew, void *stream);

/* Optional planning call for dlesm_shallow_step_f64, like dlesm_stencil5_autotune_f64: times a
 * dozen launch shapes and the cache policies of the once-read / once-written arrays on the caller's
 * own arrays (each trial is the same valid step) and remembers the fastest for this (ld, box).
 * Synchronises `stream`. */
int dlesm_shallow_autotune_f64(const dlesm_sw_params *params, int ld, int ny,
                               int xstart, int xstop, int ystart, int ystop,
                               const double *u, const double *v, const double *p,
                               const double *uold, const double *vold, const double *pold,
                               double *unew, double *vnew, double *pnew, void *stream);

/* The SW-offset form of the same step -- the staggering of the GOcean `shallow` benchmark
 * (DESIGN.md section 6.2): u(i,j) on the WEST face of T(i,j), v on the south face, z on the SW
 * corner.  The only staggering the reference supports with periodic boundaries, and only serially
 * (field_mod.f90:675-751, grid_mod.f90:437-442); u, v, p must hold valid periodic halos
 * (dlesm_periodic_halos_apply_f64), the new fields get theirs from the caller the same way. */
int dlesm_shallow_step_sw_f64(const dlesm_sw_params *params, int ld, int ny,
                              int xstart, int xstop, int ystart, int ystop,
                              const double *u, const double *v, const double *p,
                              const double *uold, const double *vold, const double *pold,
                              double *unew, double *vnew, double *pnew, void *stream);

/* planning call for the SW-offset step (dlesm_shallow_step_sw_f64 and its periodic form), as
 * dlesm_shallow_autotune_f64 is for the NE one; the new fields receive one valid step (no periodic copies) */
int dlesm_shallow_autotune_sw_f64(const dlesm_sw_params *params, int ld, int ny,
                                  int xstart, int xstop, int ystart, int ystop,
                                  const double *u, const double *v, const double *p,
                                  const double *uold, const double *vold, const double *pold,
                                  double *unew, double *vnew, double *pnew, void *stream);

/* The same step over the INTERNAL region of periodic fields, with the periodic copies of the new level done by
 * the same launch: every cell stored on the first / last internal column or row is also stored into the halo cell
 * that init_periodic_bc_halos (field_mod.f90:1394-1464) would copy it to, corner halos included.  Leaves unew,
 * vnew, pnew exactly as dlesm_shallow_step_sw_f64 over `internal` followed by
 * dlesm_periodic_halos_apply_multi_f64 does -- one launch instead of three.  bc_x, bc_y: the grid's
 * boundary_conditions(1:2); a non-periodic direction gets no copies. */
int dlesm_shallow_step_sw_periodic_f64(const dlesm_sw_params *params, int ld, int ny,
                                       const dlesm_region *internal, int bc_x, int bc_y,
                                       const double *u, const double *v, const double *p,
                                       const double *uold, const double *vold, const double *pold,
                                       double *unew, double *vnew, double *pnew, void *stream);

/* TWO leapfrog steps per launch (NE offset, fixed boundary ring): level n+1 into unew / vnew / pnew and
 * level n+2 into unew2 / vnew2 / pnew2, bit for bit what
 *     dlesm_shallow_step_f64(..., u, v, p, uold, vold, pold, unew, vnew, pnew);
 *     dlesm_shallow_step_f64(..., unew, vnew, pnew, u, v, p, unew2, vnew2, pnew2);
 * leave behind -- six arrays read and six written per TWO steps, 48 B/cell/step instead of 72.  As for those two calls the ring of
 * unew, vnew, pnew outside the box (which no step writes) must hold the boundary values before the call.  Twelve distinct
 * arrays (level n+2 cannot overwrite level n-1 in place: the first stage reads it one cell around each tile).  The PSy-layer
 * loop nests it replaces: two passes of the un-fused GOcean kernel sequence (infrastructure_mod.f90:13-41 for the form).
 * Single domain only: on a decomposed grid use dlesm_shallow_step_x2_dm. */
int dlesm_shallow_step_x2_f64(const dlesm_sw_params *q, int ld, int ny, int xstart, int xstop, int ystart, int ystop,
                              const double *u, const double *v, const double *p, const double *uold, const double *vold,
                              const double *pold, double *unew, double *vnew, double *pnew, double *unew2, double *vnew2,
                              double *pnew2, void *stream);
/* ... and with the Asselin filter after EACH step: two whole time steps of the GOcean loop (update + time_smooth of the old level,
 * twice) in one launch.  In: level n (u, v, p) and the filtered level n-1 (uold, vold, pold), both untouched.  Out: level n+2 in
 * unew2 / vnew2 / pnew2 and the FILTERED level n+1 in uold2 / vold2 / pold2 -- the new current and old levels two calls of
 * dlesm_shallow_step_smooth_f64 with the usual rotation leave, bit for bit, provided the boundary ring is the same at every time
 * level (the ring of the unfiltered level n+1, which no array holds, is taken from u, v, p).  48 B/cell/step against 96 for the
 * one-launch filtered step.  Time loop: ping-pong (u.., uold..) <-> (unew2.., uold2..).
 * Cells written: the box of unew2 / vnew2 / pnew2 and of uold2 / vold2 / pold2, nothing else; every other cell of the six outputs
 * (ring, halos, padding columns) keeps the value it had before the call.  This holds on every path, the fall-back for arrays the
 * wave tiles cannot take included.
 * Single domain only: on a decomposed grid use dlesm_shallow_step_smooth_x2_dm. */
int dlesm_shallow_step_smooth_x2_f64(const dlesm_sw_params *q, double alpha, int ld, int ny, int xstart, int xstop, int ystart,
                                     int ystop, const double *u, const double *v, const double *p, const double *uold,
                                     const double *vold, const double *pold, double *unew2, double *vnew2, double *pnew2,
                                     double *uold2, double *vold2, double *pold2, void *stream);
/* The same two entries for the SW-offset, doubly periodic model -- the configuration of the GOcean `shallow` benchmark
 * (field_mod.f90:675-751, 1394-1464): == two calls of dlesm_shallow_step_sw_periodic_f64 / dlesm_shallow_step_sw_smooth_periodic_f64
 * with the loop's rotation, periodic images of every level that comes out included.  Level n+1 one cell outside the box is the
 * image of level n+1 inside, so the first stage reads level n TWO cells outside the box from where it is the image of.  Beyond
 * the single steps' preconditions: level n-1 carries valid periodic halos as well.  Cells written: the internal region of each
 * output and its periodic images (halo rows and columns, corners included), nothing else -- on every path, the fall-back
 * included; every other cell (padding columns and rows beyond the halos) keeps the value it had before the call. */
int dlesm_shallow_step_sw_x2_periodic_f64(const dlesm_sw_params *q, int ld, int ny, const dlesm_region *internal, int bc_x, int bc_y,
                                          const double *u, const double *v, const double *p, const double *uold, const double *vold,
                                          const double *pold, double *unew, double *vnew, double *pnew, double *unew2,
                                          double *vnew2, double *pnew2, void *stream);
int dlesm_shallow_step_sw_smooth_x2_periodic_f64(const dlesm_sw_params *q, double alpha, int ld, int ny, const dlesm_region *internal,
                                                 int bc_x, int bc_y, const double *u, const double *v, const double *p,
                                                 const double *uold, const double *vold, const double *pold, double *unew2,
                                                 double *vnew2, double *pnew2, double *uold2, double *vold2, double *pold2,
                                                 void *stream);

/* One WHOLE time step of the GOcean leapfrog in one launch: the u/v/h update AND the Asselin filter of the old level
 * (the benchmark's time_smooth kernel), from values the lanes already hold --
 *     unew, vnew, pnew <- step(u, v, p, uold, vold, pold);   uold <- u + alpha*(unew - 2*u + uold)   (likewise vold, pold; in place)
 * -- bit for bit what dlesm_shallow_step_f64 followed by three dlesm_time_smooth_f64 calls leave, at 96 B/cell
 * (six arrays read, six written) instead of 72 + 3 x 32 = 168.  After the call the host program rotates
 * u <- unew (uold already holds the filtered u; the former u buffers are free).  The nine arrays must be distinct. */
int dlesm_shallow_step_smooth_f64(const dlesm_sw_params *params, double alpha, int ld, int ny,
                                  int xstart, int xstop, int ystart, int ystop,
                                  const double *u, const double *v, const double *p,
                                  double *uold, double *vold, double *pold,
                                  double *unew, double *vnew, double *pnew, void *stream);
/* ... and the SW-offset form over the internal region of periodic fields, the periodic images of the new level AND of
 * the filtered old level written by the same launch: a whole time step of the GOcean `shallow` benchmark = ONE launch. */
int dlesm_shallow_step_sw_smooth_periodic_f64(const dlesm_sw_params *params, double alpha, int ld, int ny,
                                              const dlesm_region *internal, int bc_x, int bc_y,
                                              const double *u, const double *v, const double *p,
                                              double *uold, double *vold, double *pold,
                                              double *unew, double *vnew, double *pnew, void *stream);

/* The GOcean `shallow` kernel set as SEPARATE launch entries: one per PSy loop nest, which is what a
 * PSyclone-generated PSy layer has -- `do jj / do ji / call compute_cu_code(ji, jj, cu%data, p%data,
 * u%data)` becomes dlesm_compute_cu_f64 over the same index box (kernel form infrastructure_mod.f90:13-41,
 * metadata argument_mod.f90:39-112, kernel_mod.f90:28-50).  Array arguments in the kernels' own order
 * (the written field first).  `offset` is the kernel's index_offset, DLESM_OFFSET_NE or DLESM_OFFSET_SW;
 * formulas frozen in DESIGN.md section 6 (NE), 6.2 (SW), 6.3 (time_smooth) -- the expression trees of the
 * fused step, so that the seven launches
 *     cu, cv, z, h  (each over the box grown towards its consumers, or over the internal region followed by
 *     the periodic copies)  then  unew, vnew, pnew
 * give bit for bit what dlesm_shallow_step_f64 / dlesm_shallow_step_sw_f64 give, at 224 B/cell of HBM
 * traffic instead of 72.  The box plus the cells its stencil reads must lie inside the ld x ny arrays;
 * the output may not alias an input (time_smooth updates field_old in place).
 *   NE:  cu(i,j) = 0.5*(p(i+1,j)+p(i,j))*u(i,j)         SW:  cu(i,j) = 0.5*(p(i,j)+p(i-1,j))*u(i,j)   ... */
int dlesm_compute_cu_f64(int offset, int ld, int ny, int xstart, int xstop, int ystart, int ystop,
                         double *cu, const double *p, const double *u, void *stream);
int dlesm_compute_cv_f64(int offset, int ld, int ny, int xstart, int xstop, int ystart, int ystop,
                         double *cv, const double *p, const double *v, void *stream);
int dlesm_compute_z_f64(int offset, int ld, int ny, int xstart, int xstop, int ystart, int ystop,
                        double fsdx, double fsdy, double *z, const double *p, const double *u,
                        const double *v, void *stream);
int dlesm_compute_h_f64(int offset, int ld, int ny, int xstart, int xstop, int ystart, int ystop,
                        double *h, const double *p, const double *u, const double *v, void *stream);
int dlesm_compute_unew_f64(int offset, int ld, int ny, int xstart, int xstop, int ystart, int ystop,
                           double tdts8, double tdtsdx, double *unew, const double *uold,
                           const double *z, const double *cv, const double *h, void *stream);
int dlesm_compute_vnew_f64(int offset, int ld, int ny, int xstart, int xstop, int ystart, int ystop,
                           double tdts8, double tdtsdy, double *vnew, const double *vold,
                           const double *z, const double *cu, const double *h, void *stream);
int dlesm_compute_pnew_f64(int offset, int ld, int ny, int xstart, int xstop, int ystart, int ystop,
                           double tdtsdx, double tdtsdy, double *pnew, const double *pold,
                           const double *cu, const double *cv, void *stream);
/* time_smooth (the Asselin filter of the `shallow` leapfrog; any offset; pointwise):
 *   field_old(i,j) = field(i,j) + alpha*(field_new(i,j) - 2.0*field(i,j) + field_old(i,j)) */
int dlesm_time_smooth_f64(int ld, int ny, int xstart, int xstop, int ystart, int ystop, double alpha,
                          const double *field, const double *field_new, double *field_old, void *stream);

/* All periodic-boundary copies of one field (dlesm_periodic_halos' regions, applied in order with
 * the patch copy below), enqueued on `stream`: what the PSy layer of a periodic model does after
 * every kernel that writes the field. */
int dlesm_periodic_halos_apply_f64(double *field, int ld, int ny, const dlesm_region *internal,
                                   int bc_x, int bc_y, void *stream);
/* the same for up to 16 fields of one shape and internal region in two launches (all x copies, then
 * all y copies): what follows a step that writes unew, vnew and pnew */
int dlesm_periodic_halos_apply_multi_f64(double *const *fields, int nfields, int ld, int ny,
                                         const dlesm_region *internal, int bc_x, int bc_y, void *stream);

/* field_copy_code over a box (infrastructure_mod.f90:32-41) and the patch copy
 * used for periodic boundaries (copy_2dfield_patch, field_mod.f90:1179-1187):
 * dst(dx0.., dy0..) = src(sx0.., sy0..) for an nx x ny patch. */
int dlesm_copy_patch_f64(const double *src, double *dst, int ld, int ny_arr,
                         int sx0, int sy0, int dx0, int dy0, int nx, int ny, void *stream);
/* set_field, field_mod.f90:1191-1202, restricted to a box */
int dlesm_fill_f64(double *f, int ld, int ny, int xstart, int xstop, int ystart, int ystop,
                   double value, void *stream);
/* array_checksum's local part, SUM(ABS(f(xs:xe,ys:ye))), field_mod.f90:1298-1302.
 * Synchronous: returns the value in *result (host). Deterministic tree order. */
int dlesm_checksum_f64(const double *f, int ld, int ny, int xstart, int xstop,
                       int ystart, int ystop, double *result, void *stream);
/* The same sum with NO host synchronisation: *result_dev -- device memory, or host memory the device can write
 * (hipHostMalloc) -- receives the value when `stream` gets there; bit-identical to dlesm_checksum_f64.  For time
 * loops that record a checksum every few steps (field_checksum of field_mod.f90:1209-1219 costs the reference a
 * full device-to-host copy of the field per call, :538); combine across ranks afterwards (dlesm_global_sum_f64). */
int dlesm_checksum_async_f64(const double *f, int ld, int ny, int xstart, int xstop,
                             int ystart, int ystop, double *result_dev, void *stream);
/* What a time loop asks about its fields every few steps: of 1 to DLESM_STATS_MAX_FIELDS fields of
 * one array shape (ld, ny), each over its own 1-based inclusive box boxes[k] and, where masks != NULL and masks[k] != NULL,
 * only where the int mask masks[k] (field layout) is > 0 -- the tmask convention of dlesm_stencil5_masked_f64:
 *   min, max    over the counted FINITE cells, compared by value (the sign of a zero is unspecified); +inf / -inf when
 *               there is none
 *   sum, sumsq  SUM x and SUM x*x over the counted finite cells; IEEE overflow allowed
 *   count       counted cells: inside the box, and mask > 0 where a mask is given
 *   nonfinite   counted cells that are NaN or +-inf (left out of min, max, sum, sumsq)
 * All fields are swept in ONE launch, every cell read once.  min, max, count and nonfinite are exact.  The bits of sum and
 * sumsq of a field depend only on (ld, its box, whether its base is 16-byte aligned, whether it has a mask) and on the
 * data: not on how many fields the call has or where the field stands in the list, not on the stream, repeats or what lies
 * outside the box.  Any base (8-byte aligned) and pitch; boxes need no ring.
 * result_dev[k] -- device memory, or host memory the device can write (hipHostMalloc) -- receives field k's numbers when
 * `stream` gets there, with no host synchronisation; the scratch space is stream-ordered, as for
 * dlesm_checksum_async_f64.  Nothing but result_dev[0..nfields) is written.  An empty box gives {+inf, -inf, 0, 0, 0, 0}
 * and reads nothing.  DLESM_EINVAL, before anything is launched: nfields outside 1..DLESM_STATS_MAX_FIELDS, a null field,
 * a box that does not fit the array, a null result_dev, a result_dev range that overlaps a field, a stream that is being
 * captured.  Combine across ranks with dlesm_global_sum_f64 / dlesm_global_max_f64 (min as -max(-min)). */
typedef struct dlesm_field_stats {   /* 48 bytes, no padding */
    double min, max;
    double sum, sumsq;
    int64_t count;
    int64_t nonfinite;
} dlesm_field_stats;
enum { DLESM_STATS_MAX_FIELDS = 8 };
int dlesm_field_stats_async_f64(const double *const *fields, const int *const *masks, const dlesm_region *boxes,
                                int nfields, int ld, int ny, dlesm_field_stats *result_dev, void *stream);
/* The same, synchronous: result_host[0..nfields) (host memory) holds the numbers on return, bit for bit those of the
 * asynchronous entry. */
int dlesm_field_stats_f64(const double *const *fields, const int *const *masks, const dlesm_region *boxes,
                          int nfields, int ld, int ny, dlesm_field_stats *result_host, void *stream);
/* After a check has tripped: *index_host = the lowest 0-based linear index (j-1)*ld + (i-1) of a counted cell of the box
 * (mask NULL, or mask > 0) that is NaN or +-inf (what = DLESM_LOCATE_NONFINITE; `value` unused) or that compares == value
 * (DLESM_LOCATE_EQUAL; pass a min or max of dlesm_field_stats), -1 if there is none.  Synchronous; the rare path. */
enum { DLESM_LOCATE_NONFINITE = 0, DLESM_LOCATE_EQUAL = 1 };
int dlesm_field_locate_f64(const double *f, const int *mask, int ld, int ny, int xstart, int xstop, int ystart, int ystop,
                           int what, double value, int64_t *index_host, void *stream);
/* synthetic initial condition of BASELINE.md: f(i,j) = u01(splitmix64(seed ^ (gi + gj<<32)))
 * on the box, gi = gx0+i-1, gj = gy0+j-1; cells outside the box are left alone. */
int dlesm_hash_init_f64(double *f, int ld, int ny, int xstart, int xstop, int ystart, int ystop,
                        uint64_t seed, int64_t gx0, int64_t gy0, void *stream);

/* (The measured copy ceilings of bench.py live in their own library, include/dlesm_lab.h: measurement tooling.)
 *
 * Settings, by name; returns the previous value (0 if the key had none).  Three classes (dlesm_tuning_class):
 *   0  USER  what a host program may want to say ("Settings"): dm_safe, dm_wait_seconds, dm_peer,
 *            dm_peer_exchange, mailbox_fences, mailbox_fields, mailbox_gather_host, dm_acquire, j5_dm_corners,
 *            j5_nt_stores, j5_use_tuned, side_stream_priority, dm_graph_force.
 *   1  HOOK  forces a path the library takes BY ITSELF for some inputs (an unaligned base, a capture, a planned launch
 *            shape, DLESM_DM_SAFE ...) so that tests can reach it on any input; every setting computes the same bits.
 *   2  LAB   selects a comparison-only kernel or a diagnostic that skips work: compiled into libdlesm_hip_lab.so only
 *            (-DDLESM_LAB, the same sources); libdlesm_hip.so ignores such a key and says so once on stderr.
 * An unknown key is reported on stderr (once) and kept. */
int dlesm_set_tuning(const char *key, int value);
/* 0 USER, 1 HOOK, 2 LAB, -1 unknown */
int dlesm_tuning_class(const char *key);
/* 1 in libdlesm_hip_lab.so (built with -DDLESM_LAB), 0 in the product library */
int dlesm_is_lab_build(void);

/* ------------------------------------------------------------------------
 * 5. Device-resident halo exchange over RCCL
 *    (replaces r2d_field%halo_exchange -> exchange_generic,
 *     field_mod.f90:1231-1256, parallel_comms_mod.f90:1501-1855, and the
 *     MPI calls of parallel/parallel_utils_mod.f90:148-183)
 * ---------------------------------------------------------------------- */

#define DLESM_UNIQUE_ID_BYTES 128
/* rank 0 creates the id, the host program distributes it (file, MPI, torch store ...) */
int dlesm_comm_unique_id(void *id /* DLESM_UNIQUE_ID_BYTES */);
/* parallel_init, parallel_utils_mod.f90:77-90: rank0 is 0-based here */
int dlesm_comm_init(const void *id, int nranks, int rank0);
/* MAILBOX MODE -- the same job without a communication library: no RCCL communicator is created.  Every message plan
 * connects its mailboxes when it is created (dlesm_halo_plan_create becomes collective; room for mailbox_fields /
 * DLESM_MAILBOX_FIELDS fields, default 3), halo exchanges and the distributed Jacobi / shallow-water steps go through them
 * (stores over xGMI, see the peer transport below), dlesm_global_sum_f64 is eight bytes per rank over the host-side board
 * (summed in rank order, the same bits on every rank), dlesm_gather_f64 / dlesm_gather_inner_f64 copy every rank's
 * block straight into a gather buffer the library owns on the root (exported once, mapped once per job by each rank).  `id`: a session name all ranks share, made by rank 0 with
 * dlesm_board_nonce and handed round like an RCCL id (dlesm_rendezvous_publish / _fetch, a torch store ...).
 * Replaces MPI_Init + the MPI calls of parallel_utils_mod.f90:77-255 for a job of one process per GPU on one node. */
int dlesm_comm_init_mailbox(const void *id, int nranks, int rank0);
int dlesm_comm_is_mailbox(void);
/* How often, in this process, hipIpcOpenMemHandle had to be tried again (or a gather fell back to host memory).  Processes
 * of one node import in turns (flock on /dev/shm/dlesm-ipc-<uid>.lock), so anything but 0 is a finding: every occurrence is
 * also logged to stderr with the HIP error name.  IPC mappings need HSA_ENABLE_IPC_MODE_LEGACY=0 in the environment of every
 * process on this driver ("Environment"). */
int dlesm_ipc_open_retries(void);
int dlesm_comm_finalize(void);
int dlesm_comm_rank(void);   /* 0-based, -1 before init */
int dlesm_comm_size(void);

/* File rendezvous for the id (dl_esm_inf_amd/csrc/dlesm_rendezvous.cpp): what a job started by
 * a launcher that only exports RANK/WORLD_SIZE uses instead of MPI_Init
 * (parallel/parallel_utils_mod.f90:77-90).  Host only, no GPU needed.  Rank 0: remove(path),
 * dlesm_comm_unique_id, publish(path, id, token) -- atomic (rename).  Others: fetch waits up to
 * timeout_ms for a record whose job token matches and whose publisher started within
 * DLESM_RENDEZVOUS_SLACK_S (default 120) seconds of the caller; anything else is a stale file
 * of a dead job and is ignored.  token: at most 111 characters. */
int dlesm_rendezvous_remove(const char *path);
int dlesm_rendezvous_publish(const char *path, const void *id, const char *token);
int dlesm_rendezvous_fetch(const char *path, void *id, const char *token, int timeout_ms);
/* dry runs only (no communicator, hence no ncclCommInitRank to hold rank 0 until everybody has the
 * id): readers acknowledge, rank 0 waits for nranks-1 acknowledgements and removes them */
int dlesm_rendezvous_ack(const char *path, int rank0);
int dlesm_rendezvous_wait_acks(const char *path, int nranks, int timeout_ms);

/* The BOARD: a host-side all-gather between the processes of one job through files (/dev/shm, or DLESM_BOARD_DIR) -- the
 * control plane of mailbox mode.  Host only.  nonce: a session name (letters, digits, '-', '_') no other job has;
 * allgather: every rank contributes `bytes`, `all` receives nranks x bytes in rank order (may be null on ranks that only
 * contribute); every rank must make the same sequence of calls.  A rank that does not show up within
 * DLESM_BOARD_TIMEOUT_S (default 600) makes the call fail. */
int dlesm_board_nonce(void *id /* DLESM_UNIQUE_ID_BYTES */);
int dlesm_board_open(const void *id, int nranks, int rank0);
int dlesm_board_is_open(void);
int dlesm_board_allgather(const void *mine, size_t bytes, void *all);
int dlesm_board_close(void);
/* parallel_abort in mailbox mode: leaves a note; ranks waiting on the board for this rank fail with its text (DLESM_EABORT)
 * instead of sitting out the time-out.  The note stays (it names a dead job's session, which no other job shares). */
int dlesm_board_abort(const char *msg);

/* Message plan for fields of shape (ld, ny): device copy of the tables, pack
 * buffers for the strided (east/west) strips.  One plan serves every field of
 * that shape (all dl_esm_inf fields share the grid's extents, field_mod.f90:327-333). */
typedef struct dlesm_halo_plan dlesm_halo_plan;
int dlesm_halo_plan_create(const dlesm_comm_tables *tables, int ld, int ny,
                           dlesm_halo_plan **plan);
int dlesm_halo_plan_destroy(dlesm_halo_plan *plan);

/* One ncclRecv / ncclSend of an exchange, as dlesm_halo_plan_describe reports it. */
typedef struct dlesm_msg_desc {
    int is_recv;           /* 1 = ncclRecv, 0 = ncclSend                                                   */
    int peer;              /* 0-based rank                                                                 */
    int dir;               /* direction code of the strip (DLESM_IPLUS ...)                                */
    int field;             /* which of the nfields fields; -1 = the strips of ALL fields, field after field */
    int i0, j0, nx, ny;    /* the strip inside the field, 1-based origin                                   */
    long count;            /* doubles on the wire                                                          */
    long buffer_offset;    /* doubles from the start of the staging buffer (receive buffer for a receive,
                              send buffer for a send); -1 = the message travels in place                  */
} dlesm_msg_desc;

/* The calls ONE exchange of `nfields` fields under `dirs_mask` makes on a plan created from `tables` for fields of
 * ld x ny, in ISSUE ORDER -- the receives then the sends, each sorted by (peer, direction code); aggregated = 1: the
 * one-message-per-neighbour-and-direction form (dlesm_halo_exchange_multi_f64, dlesm_halo_exchange_f64 on its own,
 * the shallow-water step); 0: the Jacobi step's own form (rows in place, strided strips through the pack buffer;
 * field-major).  RCCL has no tags (the reference matches messages by tag_orig + dir, parallel_comms_mod.f90:1606,
 * 1647): between a pair of ranks the k-th send meets the k-th receive, so this order IS the protocol.  Host only (no
 * GPU, no communicator); built and walked by the very code the plan and its exchanges use.  *n_out = number of
 * calls; with max_out = 0 only the count is returned. */
int dlesm_halo_plan_describe(const dlesm_comm_tables *tables, int ld, int ny, int nfields,
                             unsigned dirs_mask, int aggregated, dlesm_msg_desc *out, int max_out,
                             int *n_out);

/* halo_exchange(depth=1) of one device field: pack -> grouped ncclSend/ncclRecv
 * -> unpack, all enqueued on `stream`.  dirs_mask selects the enabled edge
 * directions (bit d-1 for DLESM_IPLUS..DLESM_JMINUS: the comm1..comm4 arguments of
 * exchange_generic); diagonals are enabled when both their edges are,
 * parallel_comms_mod.f90:1557-1571.  DLESM_DIRS_ALL is what halo_exchange passes
 * (field_mod.f90:1247-1248); 0 exchanges nothing, as in the reference; halos of a
 * disabled direction are left untouched.  DLESM_DIRS_NO_DIAGONALS (an extension)
 * keeps the four corner messages off whatever the edges say: all a 5-point stencil needs.
 * One exchange per plan may be in flight at a time (the pack buffers are the plan's). */
#define DLESM_DIRS_ALL 0xFu
#define DLESM_DIRS_NO_DIAGONALS 0x10u
int dlesm_halo_exchange_f64(dlesm_halo_plan *plan, double *field, unsigned dirs_mask,
                            void *stream);

/* The same for several fields of the plan's shape at once: ONE grouped launch for all of them
 * (what a time step that updates u, v and p needs), ONE message per neighbour and direction that
 * carries the strips of all the fields, field after field (an RCCL send/recv pair costs microseconds
 * whatever its size: message count is the lever).  At most 16 fields. */
int dlesm_halo_exchange_multi_f64(dlesm_halo_plan *plan, double *const *fields, int nfields,
                                  unsigned dirs_mask, void *stream);

/* One distributed Jacobi time step with the exchange hidden behind the
 * interior: frame(out) on `stream` (its west/east columns written straight into the
 * send buffer too), then [exchange(out) on the library's side stream] ||
 * [interior(out) on `stream`], joined on `stream`.  On return (asynchronously)
 * `out` holds the new values AND valid depth-1 EDGE halos (west, east, south, north:
 * DLESM_DIRS_ALL | DLESM_DIRS_NO_DIAGONALS -- the 5-point stencil never reads a corner
 * halo cell, so the corner messages are not sent), i.e. it is ready to be the `in` of
 * the next step.  `in` must have valid edge halos. */
int dlesm_jacobi5_step_dm(dlesm_halo_plan *plan, const double *in, double *out,
                          int ld, int ny, int xstart, int xstop, int ystart, int ystop,
                          void *stream);

/* The same step for a TIME LOOP of such steps: it returns with the exchange of `out` still in flight
 * on the library's side stream -- the caller's stream carries one kernel launch per step and no
 * event wait.  The next pipelined step on the same plan and stream waits for that exchange on the
 * device (its frame workgroups, the only ones that read halos, sleep on a flag the side stream sets
 * once the messages have landed; bounded; the received west/east strips are read straight from the
 * receive buffer, not unpacked into the field); every other entry point that takes the plan joins it
 * first -- the join also runs the deferred unpack, so that `out` then holds valid edge halos (the
 * outputs of EARLIER steps of the loop keep whatever west/east halos they had: only the joined
 * output's are promised).  Before
 * anything ELSE reads the halo cells of `out` (a kernel of the host program, a copy on another
 * stream), call dlesm_halo_plan_join.  Same results as dlesm_jacobi5_step_dm, bit for bit. */
int dlesm_jacobi5_step_dm_pipelined(dlesm_halo_plan *plan, const double *in, double *out,
                                    int ld, int ny, int xstart, int xstop, int ystart, int ystop,
                                    void *stream);
/* order `stream` behind the exchange a pipelined step left in flight (no-op when there is none) */
int dlesm_halo_plan_join(dlesm_halo_plan *plan, void *stream);

/* ---- Peer transport of the distributed Jacobi step: the stencil kernel itself is the exchange. ----------------------
 * What the reference does with MPI_Isend / MPI_Irecv / MPI_Waitany per strip (parallel_comms_mod.f90:1601-1750,
 * parallel_utils_mod.f90:148-211) and the default path here with one RCCL group per step, a connected plan does with
 * stores: the frame workgroups of the step launch write every cell a neighbour needs straight into that neighbour's
 * receive MAILBOX (peer-mapped fine-grained memory: xGMI stores) and then raise the neighbour's arrival flag; they read
 * their own halo operands from the local mailbox once its arrival flags are up.  No RCCL kernel, no side stream, no
 * pack, no event.  Mailboxes are double-buffered on the step number, which therefore has to advance on every rank alike
 * (each rank takes the same sequence of distributed steps on its plan -- what a halo exchange asks for anyway).
 * Results are bit for bit those of the RCCL path.  dlesm_jacobi5_step_dm / _pipelined use the mailboxes (nfields >= 1), and
 * so do dlesm_shallow_step_dm / _pipelined / _smooth_dm* when the plan was connected with nfields >= 3 (plans of halo depth 1,
 * stepped over the internal region), and dlesm_halo_exchange_f64 / _multi_f64 themselves (any depth, nfields <= the
 * count the plan was connected for: one launch that copies the send strips into the neighbours' mailboxes and raises their
 * flags, one that waits for this rank's flags and unpacks; dm_peer_exchange = 0 keeps the RCCL group for them).  The
 * fused multi-step and 3x3 distributed steps keep their RCCL-side machinery.  The mailboxes of a plan are one resource:
 * operations on it issued on different streams are ordered one behind the other by the library (an event); ordering the
 * FIELDS between streams stays the caller's business, as with any other entry.  dm_peer = 0 (dlesm_set_tuning)
 * switches a connected plan back to RCCL -- on every rank or on none.
 * hipGraph capture: the number of a mailbox operation is kept in DEVICE memory (each operation's flag-raising workgroup
 * writes the next operation's number), the host only tracks its parity -- which mailbox half the operation's pointers
 * address.  Mailbox operations may therefore be captured, and replayed any number of times between un-captured ones,
 * provided (a) a graph holds an EVEN number of them per plan and ends joined (dlesm_halo_plan_join inside the capture
 * after *_pipelined steps), (b) every replay starts at the parity the capture started at (an even number of un-captured
 * operations in between), (c) the operation before the capture was issued on the capturing stream, and (d) every rank
 * replays alike.  A replay out of step is detected on the device (last number raised != this one - 1) and raises the
 * process-wide flag of dlesm_wait_timed_out: wrong halos cannot leave silently.
 *
 * Connecting is collective over the ranks that share neighbours:
 *   1. dlesm_halo_plan_peer_export(plan, my_rank, nfields = 1, blob): allocates this rank's mailbox and writes
 *      DLESM_PEER_BLOB_BYTES describing it (an IPC handle + the slot of each receive message);
 *   2. the host program all-gathers the blobs in rank order (MPI_Allgather, torch.distributed.all_gather, a file ...);
 *   3. dlesm_halo_plan_peer_connect(plan, my_rank, nranks, blobs): maps the neighbours' mailboxes
 *      (hipIpcOpenMemHandle; a rank that is its own neighbour uses the pointer) and matches every send with the receive
 *      it meets -- the k-th message to a neighbour is the k-th that neighbour receives from this rank.
 * dlesm_halo_plan_peer_connect_rccl does 1-3 with ncclAllGather on the library's communicator.
 * my_rank / the peers in the plan's tables are 0-based ranks, as everywhere in this header. */
#define DLESM_PEER_BLOB_BYTES 1024
int dlesm_halo_plan_peer_export(dlesm_halo_plan *plan, int my_rank, int nfields, void *blob);
int dlesm_halo_plan_peer_connect(dlesm_halo_plan *plan, int my_rank, int nranks, const void *blobs);
int dlesm_halo_plan_peer_connect_rccl(dlesm_halo_plan *plan, int nfields);
int dlesm_halo_plan_peer_connected(const dlesm_halo_plan *plan);   /* 1 / 0 */
/* HOST ONLY (no device, no communicator), for checking the matching on any mesh: the blob a plan made from `tables` would
 * export (without an IPC handle), and, given the blobs of all ranks, what every SEND of this rank is matched with -- the code
 * dlesm_halo_plan_peer_export / _connect run.  One record per send, in the plan's (peer, direction) order. */
typedef struct dlesm_peer_match_desc {
    int peer, dir;         /* the neighbour (0-based rank) and the direction code of the send                   */
    int i0, j0, nx, ny;    /* the strip it reads in this rank's field (1-based origin, extent)                 */
    long count;            /* cells per field                                                                  */
    int slot;              /* index of the matching receive in the NEIGHBOUR's (peer, direction)-sorted list   */
    long off;              /* its per-field offset in the neighbour's mailbox parity                           */
} dlesm_peer_match_desc;
int dlesm_peer_blob_describe(const dlesm_comm_tables *tables, int ld, int ny, int my_rank, int nfields, void *blob);
int dlesm_peer_match_describe(const dlesm_comm_tables *tables, int ld, int ny, int my_rank, int nranks, int nfields,
                              const void *blobs, dlesm_peer_match_desc *out, int max_out, int *n_out);

/* Device-side waits of the distributed steps are bounded: 30 s for this GPU's own frame workgroups, and
 * dm_wait_seconds (dlesm_set_tuning; default 600, 0 = no limit, as the reference waits in MPI_Waitany,
 * parallel_comms_mod.f90:1773-1798) wherever the wait is for an EXCHANGE, i.e. for the slowest neighbour.  A wait
 * that gives up raises ONE process-wide flag; the stream then runs on, so whatever was enqueued behind the wait may
 * have read halos that never arrived.  From that moment EVERY device entry point of this library (steps, checksum,
 * gather, field callbacks ...) fails with DLESM_EHIP: wrong numbers cannot leave silently.  Returns 1 if the flag is
 * up; clear != 0 acknowledges it (after the host program has destroyed its halo plans) and makes the library
 * re-measure whether streams still run side by side. */
int dlesm_wait_timed_out(int clear);

/* The one-launch and time-loop forms park a waiting kernel on the library's side stream while the kernel that
 * releases it runs on the caller's stream: that needs kernels of the two streams to execute side by side (not so
 * under tools that serialise kernels).  Measured once per caller's stream -- at dlesm_halo_plan_create for the null
 * stream, else at the first step on a stream: one device synchronisation, 64 bytes, at most 50 ms -- and remembered.
 * This call measures again NOW (after re-creating a stream, attaching a tool ...): 1 = side by side (one-launch
 * forms are used), 0 = not (the steps take their event-ordered form), < 0 on error.  Not inside a graph capture. */
int dlesm_probe_stream_concurrency(void *stream);

/* The distributed step of any 3 x 3 weighted kernel (dlesm_stencil9_f64's coefficients and
 * evaluation order): out = stencil9(in) on the box, then the halos of `out` valid as after
 * out%halo_exchange(1) -- all eight directions when a corner weight is non-zero (corner halos are
 * operands of the next step), the four edges when all four are zero (the diagonal halo cells are
 * then left untouched).  `in` must hold valid halos for the same directions.  The frame of `out` is
 * computed first (west/east columns straight into the send buffer), the exchange runs on the
 * library's side stream beside the interior sweep, the call returns with `stream` ordered behind
 * both.  Bit-identical to dlesm_stencil9_f64 + dlesm_halo_exchange_f64. */
int dlesm_stencil9_step_dm(dlesm_halo_plan *plan, const double *in, double *out, const double *coef,
                           int ld, int ny, int xstart, int xstop, int ystart, int ystop, void *stream);

/* nsteps (2..8) distributed Jacobi time steps per call, ONE depth-nsteps exchange per call
 * (temporal blocking across tiles; dlesm_stencil5_multi_f64 with stage boxes grown towards
 * every neighbouring tile).  `plan` must come from dlesm_map_comms_depth(depth = nsteps) tables
 * and `in` must hold valid depth-nsteps halos; `out` leaves with valid depth-nsteps halos.
 * Bit-identical to nsteps x (dlesm_stencil5_f64 + depth-nsteps exchange). */
int dlesm_jacobi5_multi_step_dm(dlesm_halo_plan *plan, const double *in, double *out,
                                int ld, int ny, int nsteps,
                                int xstart, int xstop, int ystart, int ystop, void *stream);

/* The distributed form of dlesm_shallow_step_f64: frame of unew/vnew/pnew, then one grouped
 * exchange of the three new fields on the side stream behind the interior.  u, v, p must have
 * valid halos; unew, vnew, pnew leave with valid halos (corners included). */
int dlesm_shallow_step_dm(dlesm_halo_plan *plan, const dlesm_sw_params *params, int ld, int ny,
                          int xstart, int xstop, int ystart, int ystop,
                          const double *u, const double *v, const double *p,
                          const double *uold, const double *vold, const double *pold,
                          double *unew, double *vnew, double *pnew, void *stream);

/* The same step for a TIME LOOP (the contract of dlesm_jacobi5_step_dm_pipelined): returns with the
 * exchange of unew/vnew/pnew in flight on the side stream; the next pipelined step on the same plan
 * and stream -- which reads them as u/v/p -- waits for it on the device, in its frame workgroups;
 * every other entry that takes the plan joins first; dlesm_halo_plan_join orders a stream behind it.
 * Between pipelined steps the caller only rotates the nine pointers.  Same results, bit for bit. */
int dlesm_shallow_step_dm_pipelined(dlesm_halo_plan *plan, const dlesm_sw_params *params, int ld, int ny,
                                    int xstart, int xstop, int ystart, int ystop,
                                    const double *u, const double *v, const double *p,
                                    const double *uold, const double *vold, const double *pold,
                                    double *unew, double *vnew, double *pnew, void *stream);

/* The two distributed forms of dlesm_shallow_step_smooth_f64 (the step with the Asselin filter of the old level folded
 * in): dlesm_shallow_step_dm[_pipelined]'s frame / exchange / interior, uold, vold, pold filtered in place.  The filtered
 * old level needs no exchange: the next step reads it at (i, j) only.  Same results as dlesm_shallow_step_dm[_pipelined]
 * followed by three dlesm_time_smooth_f64 calls over the box, bit for bit. */
int dlesm_shallow_step_smooth_dm(dlesm_halo_plan *plan, const dlesm_sw_params *params, double alpha, int ld, int ny,
                                 int xstart, int xstop, int ystart, int ystop,
                                 const double *u, const double *v, const double *p,
                                 double *uold, double *vold, double *pold,
                                 double *unew, double *vnew, double *pnew, void *stream);
int dlesm_shallow_step_smooth_dm_pipelined(dlesm_halo_plan *plan, const dlesm_sw_params *params, double alpha,
                                           int ld, int ny, int xstart, int xstop, int ystart, int ystop,
                                           const double *u, const double *v, const double *p,
                                           double *uold, double *vold, double *pold,
                                           double *unew, double *vnew, double *pnew, void *stream);

/* The distributed forms of dlesm_shallow_step_x2_f64 / dlesm_shallow_step_smooth_x2_f64: two leapfrog steps per launch and ONE
 * depth-2 exchange per two steps.  `plan` must come from dlesm_map_comms_depth(depth = 2) tables (a grid decomposed with
 * halo_width = 2); a plan of another depth is refused, a plan without messages is the single-domain entry, bit for bit.
 * Plain form.  In: u, v, p (level n) with valid depth-2 halos towards every neighbour, corners included; uold, vold, pold
 * (level n-1) with valid depth-1 halos; on sides without a neighbour the ring rules of dlesm_shallow_step_x2_f64.  Out:
 * unew2.. (level n+2) valid on the box and in its depth-2 halos (one exchange); unew.. (level n+1) valid on the box grown by
 * one cell towards every side that has a neighbour (corners where both sides have one) -- computed there, not exchanged, and
 * bit for bit the neighbour's interior cells -- other halo cells of unew.. keep what they held.  Both levels are what
 * step + depth-2 exchange, twice, leave in those cells.  Time loop: (cur, old, new1, new2) <- (new2, new1, old, cur).
 * Filtered form.  In: level n with depth-2 halos, the filtered level n-1 with depth-1 halos, both untouched.  Out: level n+2
 * (unew2..) and the filtered level n+1 (uold2..), both with valid depth-2 halos: what two calls of dlesm_shallow_step_smooth_dm
 * on a depth-2 plan leave as the new current and old levels.  The filtered level n+1 needs level n+2 at the cell, so it
 * is exchanged with it: six fields in one aggregated exchange (two turns of three in mailbox mode).
 * Twelve distinct arrays, as for the single-domain entries; plan dimensions ld x ny. */
int dlesm_shallow_step_x2_dm(dlesm_halo_plan *plan, const dlesm_sw_params *q, int ld, int ny,
                             int xstart, int xstop, int ystart, int ystop,
                             const double *u, const double *v, const double *p,
                             const double *uold, const double *vold, const double *pold,
                             double *unew, double *vnew, double *pnew,
                             double *unew2, double *vnew2, double *pnew2, void *stream);
int dlesm_shallow_step_smooth_x2_dm(dlesm_halo_plan *plan, const dlesm_sw_params *q, double alpha, int ld, int ny,
                                    int xstart, int xstop, int ystart, int ystop,
                                    const double *u, const double *v, const double *p,
                                    const double *uold, const double *vold, const double *pold,
                                    double *unew2, double *vnew2, double *pnew2,
                                    double *uold2, double *vold2, double *pold2, void *stream);

/* The distributed form of dlesm_nemolite_step_f64: one NEMOLite2D-class time step and ONE exchange of
 * its five outputs.  Bit for bit, in every cell of every array (halos and padding included), what this definition leaves:
 * dlesm_continuity_f64 over tbox; dlesm_halo_exchange_f64(plan, ssha, DLESM_DIRS_ALL); next_sshu / next_sshv, momentum and,
 * when obc is not NULL, bc_open, as dlesm_nemolite_step_f64 runs them; dlesm_halo_exchange_multi_f64 of {ssha, ssha_u,
 * ssha_v, ua, va} over DLESM_DIRS_ALL.
 * In: un, vn, sshn_t, sshn_u, sshn_v, ht, hu, hv with valid depth-1 halos towards every neighbour, corners included (the
 * ssha cells a neighbour would send are computed here by continuity, which reads e.g. vn(xe+1, ys-1)); on sides without a
 * neighbour the ring rules of dlesm_nemolite_step_f64 (ssha there is the caller's).  Out: ssha, ssha_u, ssha_v, ua, va with
 * valid depth-1 halos; a time loop only rotates the pointers.
 * A plan without messages: dlesm_nemolite_step_f64, bit for bit, for any boxes.  A plan with messages needs a depth-1 plan
 * (a grid decomposed with halo_width = 1) and tbox == ubox == vbox; another depth or unequal boxes give DLESM_EINVAL, as do
 * a null plan, a plan for other extents and every refusal of dlesm_nemolite_step_f64 -- all before anything is launched or
 * exchanged.  obc is rank-local (each rank's plan from its own mask, possibly empty).  Collective: every rank calls it, in
 * the same order. */
int dlesm_nemolite_step_dm(dlesm_halo_plan *plan, const dlesm_momentum_params *params, const dlesm_momentum_grid *grid,
                           const double *area_t, int ld, int ny, const dlesm_region *tbox, const dlesm_region *ubox,
                           const dlesm_region *vbox, const dlesm_obc *obc, double ssh_bc, const double *un, const double *vn,
                           const double *ht, const double *hu, const double *hv, const double *sshn_t, const double *sshn_u,
                           const double *sshn_v, double *ssha, double *ssha_u, double *ssha_v, double *ua, double *va,
                           void *stream);
/* dlesm_nemolite_step_dm that skips land: step 2 is dlesm_nemolite_step_wet_f64 with this rank's wet
 * plan (rank-local, as obc is; NULL: dlesm_nemolite_step_dm, bit for bit); the ring ssha and the exchange of the five outputs
 * are unchanged, every rank performs the same number of mailbox operations whatever its plan, and stale land ssha travels in
 * the exchange.  The contract of dlesm_nemolite_step_wet_f64 holds against dlesm_nemolite_step_dm, halos included.
 * DLESM_EINVAL before anything is launched or exchanged: the refusals of both entries. */
int dlesm_nemolite_step_wet_dm(dlesm_halo_plan *plan, const dlesm_wet_plan *wet, const dlesm_momentum_params *params,
                           const dlesm_momentum_grid *grid, const double *area_t, int ld, int ny, const dlesm_region *tbox, const dlesm_region *ubox,
                           const dlesm_region *vbox, const dlesm_obc *obc, double ssh_bc, const double *un, const double *vn,
                           const double *ht, const double *hu, const double *hv, const double *sshn_t, const double *sshn_u,
                           const double *sshn_v, double *ssha, double *ssha_u, double *ssha_v, double *ua, double *va,
                           void *stream);

/* Tracer transport: first-order upwind advection of ntracers (1..DLESM_TRACER_MAX) T-point tracers
 * with continuity's own face transports, in one sweep that loads the flow once.  For every T cell (i,j) of the box (1-based,
 * inclusive, a one-cell ring inside the array) with tmask(i,j) > 0 and every tracer c = c_in[k]:
 *     r1..r4 = continuity's (east, west, north, south face)
 *     F1 = tmask(i+1,j) != 0 ? r1 * (r1 >= 0 ? c(i,j)   : c(i+1,j)) : 0      F2 = tmask(i-1,j) != 0 ? r2 * (r2 >= 0 ? c(i-1,j) : c(i,j)) : 0
 *     F3 = tmask(i,j+1) != 0 ? r3 * (r3 >= 0 ? c(i,j)   : c(i,j+1)) : 0      F4 = tmask(i,j-1) != 0 ? r4 * (r4 >= 0 ? c(i,j-1) : c(i,j)) : 0
 *     c_out[k](i,j) = ((ht + sshn_t) * c + (((F2 - F1) + F4) - F3) * (rdt / area_t)) / (ht + ssha)
 * every operation rounded in double precision in that order.  Cells with tmask <= 0 (land, open) and cells outside the box
 * are not written; what land cells of c or faces that touch land hold never reaches a written cell.  ssha is the array the
 * time step produced from the same level-n inputs; an open cell's c is the boundary value, kept by the caller in both buffers.
 * c_in and c_out are HOST arrays of ntracers device pointers.  Asynchronous on `stream`, may be captured.  Any 8-byte-aligned
 * bases and any ld give the same bits (an even ld and 16-byte bases take the wave-tile sweep; the HOOK key tracer_kernel = 1
 * forces the general path).  An empty box launches nothing.  DLESM_EINVAL before anything is launched: ntracers outside
 * 1..DLESM_TRACER_MAX, a null pointer, a box that does not fit with its ring, a c_out[k] that overlaps an input, a c_in or
 * another c_out. */
enum { DLESM_TRACER_MAX = 8 };
int dlesm_tracer_step_f64(double rdt, int ld, int ny, int xstart, int xstop, int ystart, int ystop,
                          const int *tmask, const double *area_t, const double *un, const double *vn,
                          const double *hu, const double *hv, const double *ht,
                          const double *sshn_t, const double *sshn_u, const double *sshn_v, const double *ssha,
                          const double *const *c_in, double *const *c_out, int ntracers, void *stream);
/* The distributed form: bit for bit in every cell, dlesm_tracer_step_f64 followed by dlesm_halo_exchange_multi_f64(plan, c_out,
 * ntracers, DLESM_DIRS_ALL).  In: the flow arrays, tmask and c_in with valid depth-1 halos towards every neighbour.  Out: c_out
 * with valid depth-1 halos; a time loop only rotates the pointers.  A plan without messages: dlesm_tracer_step_f64.  A plan
 * with messages must be a depth-1 plan for ld x ny (DLESM_EINVAL otherwise, as for a null plan and every refusal above, before
 * anything is launched or exchanged).  Over connected mailboxes the exchange runs in ceil(ntracers / mailbox fields) turns on
 * every rank, whatever the box.  Collective: every rank calls it, in the same order. */
int dlesm_tracer_step_dm(dlesm_halo_plan *plan, double rdt, int ld, int ny, int xstart, int xstop, int ystart, int ystop,
                         const int *tmask, const double *area_t, const double *un, const double *vn,
                         const double *hu, const double *hv, const double *ht,
                         const double *sshn_t, const double *sshn_u, const double *sshn_v, const double *ssha,
                         const double *const *c_in, double *const *c_out, int ntracers, void *stream);

/* Second-order limited tracer transport: dlesm_tracer_step_f64 with the value a face carries rebuilt
 * from the upwind cell's monotonised-central slope.  T(i,j) = tmask(i,j) inside the array and 0 outside it:
 *     MC(a, b): a2 = 2*|a|; b2 = 2*|b|; m = 0.5*|a + b|; lo = a2 < b2 ? a2 : b2; lo = m < lo ? m : lo
 *               MC = (a > 0 && b > 0) ? lo : ((a < 0 && b < 0) ? -lo : 0)
 *     sx(i,j) = (T(i,j) > 0 && T(i-1,j) != 0 && T(i+1,j) != 0) ? MC(c(i,j) - c(i-1,j), c(i+1,j) - c(i,j)) : 0
 *     sy(i,j) = (T(i,j) > 0 && T(i,j-1) != 0 && T(i,j+1) != 0) ? MC(c(i,j) - c(i,j-1), c(i,j+1) - c(i,j)) : 0
 *     ce = r1 >= 0 ? c(i,j)   + 0.5*sx(i,j)   : c(i+1,j) - 0.5*sx(i+1,j)      cw = r2 >= 0 ? c(i-1,j) + 0.5*sx(i-1,j) : c(i,j) - 0.5*sx(i,j)
 *     cn = r3 >= 0 ? c(i,j)   + 0.5*sy(i,j)   : c(i,j+1) - 0.5*sy(i,j+1)      cs = r4 >= 0 ? c(i,j-1) + 0.5*sy(i,j-1) : c(i,j) - 0.5*sy(i,j)
 *     F1 = T(i+1,j) != 0 ? r1*ce : 0    F2 = T(i-1,j) != 0 ? r2*cw : 0    F3 = T(i,j+1) != 0 ? r3*cn : 0    F4 = T(i,j-1) != 0 ? r4*cs : 0
 * and c_out[k](i,j) as above.  Compare-and-select throughout, no division but the rule's own; land, open cells and cells next
 * to land have slope zero, so coasts and open boundaries carry the upwind value, a NaN on land (two cells away included) never
 * reaches a written cell, and a constant nonzero tracer gets dlesm_tracer_step_f64's bits.  Nothing outside the array is read:
 * the box needs only its one-cell ring.  Arguments, aliasing rules, refusals and the asynchronous contract are those of
 * dlesm_tracer_step_f64; the HOOK key tracer_muscl_kernel = 1 forces the general path.  Keeps a profile's range while
 * |r| * rdt / (area_t * (ht + ssha)) <= 1/2. */
int dlesm_tracer_step_muscl_f64(double rdt, int ld, int ny, int xstart, int xstop, int ystart, int ystop,
                                const int *tmask, const double *area_t, const double *un, const double *vn,
                                const double *hu, const double *hv, const double *ht,
                                const double *sshn_t, const double *sshn_u, const double *sshn_v, const double *ssha,
                                const double *const *c_in, double *const *c_out, int ntracers, void *stream);
/* The distributed form: bit for bit in every cell, dlesm_tracer_step_muscl_f64 followed by dlesm_halo_exchange_multi_f64(plan,
 * c_out, ntracers, DLESM_DIRS_ALL).  In: tmask and c_in with valid depth-2 halos towards every neighbour, the flow arrays with
 * depth-1 halos.  Out: c_out with valid depth-2 halos.  A plan without messages: dlesm_tracer_step_muscl_f64.  A plan with
 * messages must be a depth-2 plan for ld x ny, from a grid decomposed with halo_width = 2 (DLESM_EINVAL otherwise, as for a null
 * plan and every refusal above, before anything is launched or exchanged).  Guards, mailbox turns and the collective contract
 * are dlesm_tracer_step_dm's. */
int dlesm_tracer_step_muscl_dm(dlesm_halo_plan *plan, double rdt, int ld, int ny, int xstart, int xstop, int ystart, int ystop,
                               const int *tmask, const double *area_t, const double *un, const double *vn,
                               const double *hu, const double *hv, const double *ht,
                               const double *sshn_t, const double *sshn_u, const double *sshn_v, const double *ssha,
                               const double *const *c_in, double *const *c_out, int ntracers, void *stream);

/* Time-centred (Hancock) limited tracer transport: dlesm_tracer_step_muscl_f64 with the constant 0.5
 * in front of a slope replaced, face by face, by half of one minus the face's Courant number, taken in the face's upwind cell:
 *     w(i,j) = rdt / (area_t(i,j) * (ht(i,j) + sshn_t(i,j)))
 *     n1 = |r1| * (r1 >= 0 ? w(i,j)   : w(i+1,j))      n2 = |r2| * (r2 >= 0 ? w(i-1,j) : w(i,j))
 *     n3 = |r3| * (r3 >= 0 ? w(i,j)   : w(i,j+1))      n4 = |r4| * (r4 >= 0 ? w(i,j-1) : w(i,j))
 *     gk = (nk >= 0 && nk < 1) ? 0.5 * (1 - nk) : 0                                                          k = 1..4
 *     ce = r1 >= 0 ? c(i,j)   + g1*sx(i,j)   : c(i+1,j) - g1*sx(i+1,j)      cw = r2 >= 0 ? c(i-1,j) + g2*sx(i-1,j) : c(i,j) - g2*sx(i,j)
 *     cn = r3 >= 0 ? c(i,j)   + g3*sy(i,j)   : c(i,j+1) - g3*sy(i,j+1)      cs = r4 >= 0 ? c(i,j-1) + g4*sy(i,j-1) : c(i,j) - g4*sy(i,j)
 * with sx, sy, F1..F4 and c_out as above.  g is always finite: a NaN, an infinite or a negative n fails the two comparisons and
 * gives 0, so what land holds in area_t, ht and sshn_t never reaches a written cell, a face with n >= 1 carries the upwind
 * value, and coasts, open cells and a constant nonzero tracer keep dlesm_tracer_step_f64's bits.  A face carries one flux: the
 * upwind cell is the same from both sides.  w is read in the four neighbours, inside the box's ring: nothing is read further
 * out than by dlesm_tracer_step_muscl_f64.  Arguments, aliasing rules, refusals and the asynchronous contract are those of
 * dlesm_tracer_step_f64; the HOOK key tracer_hancock_kernel = 1 forces the general path.  In one dimension a profile's range is
 * kept while n <= 1/2. */
int dlesm_tracer_step_hancock_f64(double rdt, int ld, int ny, int xstart, int xstop, int ystart, int ystop,
                                  const int *tmask, const double *area_t, const double *un, const double *vn,
                                  const double *hu, const double *hv, const double *ht,
                                  const double *sshn_t, const double *sshn_u, const double *sshn_v, const double *ssha,
                                  const double *const *c_in, double *const *c_out, int ntracers, void *stream);
/* The distributed form: bit for bit in every cell, dlesm_tracer_step_hancock_f64 followed by dlesm_halo_exchange_multi_f64(plan,
 * c_out, ntracers, DLESM_DIRS_ALL).  Halos, the depth-2 plan, refusals, guards, mailbox turns and the collective contract are
 * dlesm_tracer_step_muscl_dm's; w of the cell beyond the box comes from the depth-1 halos of area_t, ht and sshn_t. */
int dlesm_tracer_step_hancock_dm(dlesm_halo_plan *plan, double rdt, int ld, int ny, int xstart, int xstop, int ystart, int ystop,
                                 const int *tmask, const double *area_t, const double *un, const double *vn,
                                 const double *hu, const double *hv, const double *ht,
                                 const double *sshn_t, const double *sshn_u, const double *sshn_v, const double *ssha,
                                 const double *const *c_in, double *const *c_out, int ntracers, void *stream);

/* The tracer schemes' Courant check: "may I take this step with this rdt".  One read-only sweep over
 * the level-n flow (no ssha: callable before the flow step) that evaluates, in every wet T cell (tmask > 0) of the 1-based
 * inclusive box, the four face Courant numbers n1..n4 of dlesm_tracer_step_hancock_f64 -- the same expression tree, bit for
 * bit -- and the cell's outflow number, with on1..on4 = tmask != 0 at (i+1,j), (i-1,j), (i,j+1), (i,j-1):
 *     valid(x) = x >= 0 && x <= DBL_MAX                               (a NaN, an infinity and a negative number fail it)
 *     o1 = (on1 && r1 > 0) ?  r1 : 0      o2 = (on2 && r2 < 0) ? -r2 : 0
 *     o3 = (on3 && r3 > 0) ?  r3 : 0      o4 = (on4 && r4 < 0) ? -r4 : 0
 *     o  = (((o1 + o2) + o3) + o4) * w(i,j)        the upwind step keeps c >= 0 while o <= 1
 *     m  = the largest valid n_k among the faces with on_k ("none" if there is no such face)
 *     bad = !(w(i,j) > 0 && w(i,j) <= DBL_MAX) || (some on_k face has !valid(n_k)) || !valid(o)
 * and reduces them to the record below.  Every member is exact: the record does not depend on the kernel form, the launch
 * shape, alignment, the stream or repeats, and what land holds (a NaN in area_t, ht, sshn_t of a land cell, in un / vn on a
 * face that touches land) changes no member.  An empty box and a box without a wet cell give {0, 0, -1, -1, 0, 0, 0, 0}. */
typedef struct dlesm_tracer_courant {   /* 64 bytes, no padding */
    double  face_max;       /* max of m over the wet cells of the box that have one; 0.0 if none (compare by value) */
    double  outflow_max;    /* max of the valid o over the wet cells of the box; 0.0 if none */
    int64_t face_index;     /* lowest 0-based linear index (j-1)*ld + (i-1) of a wet cell with m == face_max; -1 if none */
    int64_t outflow_index;  /* the same for o == outflow_max */
    int64_t face_over;      /* wet cells with an m >= face_limit */
    int64_t outflow_over;   /* wet cells with a valid o >= outflow_limit */
    int64_t invalid;        /* wet cells with bad */
    int64_t wet;            /* wet cells of the box */
} dlesm_tracer_courant;
/* The array arguments are dlesm_tracer_step_f64's without ssha and the tracers (device memory, ny x ld, the box with a
 * one-cell ring inside the array).  *result_dev (device memory) is written when `stream` gets there; the scratch is
 * stream-ordered, nothing else is written, there are no floating-point atomics and the host is not synchronised.
 * DLESM_EINVAL before anything is launched: a null pointer, a double array not 8-byte aligned or a mask not 4-byte aligned, a
 * box that does not fit with its ring, a limit that is NaN or <= 0, a result_dev inside an input array, a stream that is
 * being captured.  Even ld with 16-byte bases (8-byte for the mask) takes the wave-tile kernel, anything else -- and the HOOK
 * key tracer_courant_kernel = 1 -- the one-cell-per-thread kernel.  There is no plan argument: the sweep exchanges nothing; on
 * a decomposed grid the inputs need valid depth-1 halos and the caller combines the ranks' records. */
int dlesm_tracer_courant_async_f64(double rdt, int ld, int ny, int xstart, int xstop, int ystart, int ystop,
                                   const int *tmask, const double *area_t, const double *un, const double *vn,
                                   const double *hu, const double *hv, const double *ht,
                                   const double *sshn_t, const double *sshn_u, const double *sshn_v,
                                   double face_limit, double outflow_limit,
                                   dlesm_tracer_courant *result_dev, void *stream);
/* The synchronous twin: the same record in host memory; returns when it is there. */
int dlesm_tracer_courant_f64(double rdt, int ld, int ny, int xstart, int xstop, int ystart, int ystop,
                             const int *tmask, const double *area_t, const double *un, const double *vn,
                             const double *hu, const double *hv, const double *ht,
                             const double *sshn_t, const double *sshn_u, const double *sshn_v,
                             double face_limit, double outflow_limit,
                             dlesm_tracer_courant *result_host, void *stream);

/* The flow step's own stability check: "may the flow step take this rdt".  One read-only sweep over
 * the level-n flow that evaluates, in every wet T cell (T = tmask > 0) of the 1-based inclusive box, every operation rounded
 * in double in the order the parentheses give, sqrt and the two divisions correctly rounded, choices by select:
 *     valid(x) = x >= 0.0 && x <= DBL_MAX                             (a NaN, an infinity and a negative number fail it)
 *     d   = ht(i,j) + sshn_t(i,j)                                     the water column momentum and continuity use
 *     ix  = 1.0 / dx_t(i,j)          iy = 1.0 / dy_t(i,j)             k2 = ix*ix + iy*iy
 *     gw  = (rdt * sqrt(g * d)) * sqrt(k2)                            the gravity-wave number, both directions at once
 *     on1 = T(i+1,j) != 0   on2 = T(i-1,j) != 0   on3 = T(i,j+1) != 0   on4 = T(i,j-1) != 0       (open faces count)
 *     a1 = on1 ? fabs(un(i,j)) : 0.0      a2 = on2 ? fabs(un(i-1,j)) : 0.0
 *     a3 = on3 ? fabs(vn(i,j)) : 0.0      a4 = on4 ? fabs(vn(i,j-1)) : 0.0
 *     um = a1 >= a2 ? a1 : a2             vm = a3 >= a4 ? a3 : a4
 *     adv = (rdt * um) * ix + (rdt * vm) * iy                         the advective number of the cell
 *     vis = (rdt * visc) * k2                                         the viscous number (0.0 when visc == 0)
 *     bad = !(d > 0.0 && d <= DBL_MAX) || !valid(a1) || !valid(a2) || !valid(a3) || !valid(a4)
 *           || !valid(gw) || !valid(adv) || !valid(vis)
 * and reduces them to the record below.  A bad wet cell adds to invalid and wet only, every other wet cell to every member.
 * Every member is exact: the record does not depend on the kernel form, the launch shape, alignment, the stream or repeats,
 * and what land holds (a NaN in un / vn on a face that touches land, anything in ht, sshn_t, dx_t, dy_t of a land cell)
 * changes no member.  An empty box and a box without a wet cell give {0, 0, 0, +inf, -1, -1, -1, -1, 0, 0, 0, 0, 0, 0, 0, 0}
 * and read nothing. */
typedef struct dlesm_flow_courant {     /* 128 bytes, no padding */
    double  gravity_max, advective_max, viscous_max;    /* maxima over the wet, not-bad cells; 0.0 if none; compared by value */
    double  depth_min;                                  /* min of d over the same cells; +infinity if none */
    int64_t gravity_index, advective_index, viscous_index, depth_index;   /* lowest 0-based (j-1)*ld+(i-1) holding the extreme; -1 if none */
    int64_t gravity_over, advective_over, viscous_over; /* cells with the number >= its limit */
    int64_t shallow;                                    /* cells with d <= depth_limit */
    int64_t invalid, wet;
    int64_t reserved[2];                                /* written as 0 */
} dlesm_flow_courant;
/* The arrays are device memory, ny x ld, the box with a one-cell ring inside the array.  *result_dev (device memory) is
 * written when `stream` gets there; the scratch is stream-ordered, nothing else is written, there are no atomics of any kind
 * and the host is not synchronised.  DLESM_EINVAL before anything is launched: a null pointer, a double array not 8-byte
 * aligned or a mask not 4-byte aligned, a box that does not fit with its ring, rdt, g or one of the three number limits NaN or
 * <= 0, visc or depth_limit NaN or < 0, a result_dev inside an input array, a stream that is being captured.  Even ld with
 * 16-byte bases (8-byte for the mask) takes the wave-tile kernel, anything else -- and the HOOK key flow_courant_kernel = 1 --
 * the one-cell-per-thread kernel.  There is no plan argument: the sweep exchanges nothing; on a decomposed grid the inputs
 * need valid depth-1 halos and the caller combines the ranks' records. */
int dlesm_flow_courant_async_f64(double rdt, double g, double visc, int ld, int ny, int xstart, int xstop, int ystart,
                                 int ystop, const int *tmask, const double *dx_t, const double *dy_t,
                                 const double *un, const double *vn, const double *ht, const double *sshn_t,
                                 double gravity_limit, double advective_limit, double viscous_limit, double depth_limit,
                                 dlesm_flow_courant *result_dev, void *stream);
/* The synchronous twin: the same record in host memory; returns when it is there. */
int dlesm_flow_courant_f64(double rdt, double g, double visc, int ld, int ny, int xstart, int xstop, int ystart,
                           int ystop, const int *tmask, const double *dx_t, const double *dy_t,
                           const double *un, const double *vn, const double *ht, const double *sshn_t,
                           double gravity_limit, double advective_limit, double viscous_limit, double depth_limit,
                           dlesm_flow_courant *result_host, void *stream);

/* The model's output fields: what NEMOLite2D's model_write puts out -- the sea-surface height and
 * the velocities brought to the T points -- and what every user derives from them, in one sweep over the level-n flow.  In
 * every wet T cell (T = tmask > 0) of the 1-based inclusive box, every operation rounded in double in the order the
 * parentheses give, sqrt and the two divisions correctly rounded, choices by select:
 *     e = T(i+1,j) != 0 ? un(i,j)   : 0.0      w = T(i-1,j) != 0 ? un(i-1,j) : 0.0     (section 6.10's face switches)
 *     n = T(i,j+1) != 0 ? vn(i,j)   : 0.0      s = T(i,j-1) != 0 ? vn(i,j-1) : 0.0
 *     ut = 0.5 * (w + e)      vt = 0.5 * (s + n)      q = ut*ut + vt*vt      d = ht(i,j) + sshn_t(i,j)
 *     corner = T(i+1,j) != 0 && T(i,j+1) != 0 && T(i+1,j+1) != 0
 *     dvdx = (vn(i+1,j) - vn(i,j)) / (0.5 * (dx_v(i,j) + dx_v(i+1,j)))
 *     dudy = (un(i,j+1) - un(i,j)) / (0.5 * (dy_u(i,j) + dy_u(i,j+1)))
 *     SSH = sshn_t(i,j)   UT = ut   VT = vt   SPEED = sqrt(q)   KE = (0.5 * d) * q   VORT = dvdx - dudy  (only where corner)
 * DLESM_OUT_SET stores out[k](i,j) = value[k]; DLESM_OUT_ADD stores out[k](i,j) = out[k](i,j) + weight * value[k], two rounded
 * operations (a time mean: weight = 1/nsteps into a zeroed array).  Land and open cells are never written, VORT neither in a
 * wet cell with land to the east, north or north-east, and nothing outside the box: such a cell keeps its content.  A NaN in
 * un / vn on a face that touches land and anything in ht, sshn_t, dx_v, dy_u of a land cell reaches no written cell (VORT
 * reads dx_v(i+1,j) and dy_u(i,j+1), and stores, only under corner); a special value in a wet cell's own operands goes where
 * IEEE sends it; a face between two open cells is read as it is.
 * out: a HOST array of DLESM_OUT_COUNT device pointers, NULL = not wanted; passed to the kernel by value.  The arrays are
 * device memory, ny x ld, the box with a one-cell ring inside the array.  An array no wanted output reads is not read and may
 * be NULL: ht serves KE, sshn_t SSH and KE, dx_v and dy_u VORT; tmask, un and vn are always needed.  weight is ignored by SET.
 * Asynchronous on `stream`, no scratch, no host state: the call may be captured into a graph.  There is no plan argument: the
 * sweep exchanges nothing; on a decomposed grid the inputs and the mask need valid depth-1 halos, corners included.  An empty
 * box launches nothing and returns 0.  Any 8-byte-aligned bases and any ld give the same bits: even ld with 16-byte bases
 * (8-byte for the mask) takes the wave-tile kernel, anything else -- and the HOOK key flow_output_kernel = 1 -- the
 * one-cell-per-thread kernel.  DLESM_EINVAL before anything is launched: a mode other than the two, DLESM_OUT_ADD with a NaN
 * or infinite weight, a null out or every entry of it null, a needed input null, a double array not 8-byte aligned or a mask
 * not 4-byte aligned, a box that does not fit with its ring, an out[k] that overlaps the mask, an input that is not NULL or
 * another out entry. */
enum { DLESM_OUT_SSH = 0, DLESM_OUT_UT, DLESM_OUT_VT, DLESM_OUT_SPEED, DLESM_OUT_KE, DLESM_OUT_VORT, DLESM_OUT_COUNT };
enum { DLESM_OUT_SET = 0, DLESM_OUT_ADD = 1 };
int dlesm_flow_output_f64(int mode, double weight, int ld, int ny, int xstart, int xstop, int ystart, int ystop,
                          const int *tmask, const double *dx_v, const double *dy_u, const double *un, const double *vn,
                          const double *ht, const double *sshn_t, double *const *out, void *stream);

/* Drifters: Lagrangian particles carried through the level-n C-grid flow, on the device.  A particle
 * has a position (x, y) in local index coordinates, as doubles: T cell (i, j), 1-based as the box, covers [i, i+1) x
 * [j, j+1); its west face x = i carries un(i-1,j), its east face x = i+1 un(i,j), its south and north faces vn(i,j-1) and
 * vn(i,j).  cell(x, y) = (floor(x), floor(y)); inbox(x, y) = x >= xstart && x < xstop + 1 && y >= ystart && y < ystop + 1,
 * evaluated in double before any conversion to an integer (a NaN or an infinity is not in the box and is never cast).  With
 * T = tmask (wet > 0, land == 0, open < 0), h the seconds per substep, every operation rounded in double in the order the
 * parentheses give, both divisions correctly rounded, choices by select:
 *     ue = T(i+1,j) != 0 ? un(i,j) : 0.0     uw = T(i-1,j) != 0 ? un(i-1,j) : 0.0      (section 6.10's face switches)
 *     vn_ = T(i,j+1) != 0 ? vn(i,j) : 0.0    vs = T(i,j-1) != 0 ? vn(i,j-1) : 0.0
 *     a = x - (double)i      b = y - (double)j      up = uw + (ue - uw) * a      vp = vs + (vn_ - vs) * b
 *     kx = (h * up) / dx_t(i,j)              ky = (h * vp) / dy_t(i,j)
 * dlesm_drifter_step_f64, for every particle p < n whose status is DLESM_DRIFTER_ACTIVE (any other is neither read further
 * nor written), with (x, y) = (px[p], py[p]):
 *     entry:  !inbox(x,y) -> LEFT;  T(cell) < 0 -> OPEN;  T(cell) == 0 -> GROUNDED       (position unchanged, done)
 *     repeat nsub times:
 *         (k1x, k1y) = vel(cell(x,y), x, y);   xm = x + 0.5 * k1x;  ym = y + 0.5 * k1y
 *         (k2x, k2y) = inbox(xm,ym) && T(cell(xm,ym)) > 0 ? vel(cell(xm,ym), xm, ym) : (k1x, k1y)
 *         xn = x + k2x;  yn = y + k2y
 *         !inbox(xn,yn)       -> (x,y) = (xn,yn), LEFT, stop
 *         T(cell(xn,yn)) == 0 -> GROUNDED, stop                  (the last wet position is kept)
 *         (x,y) = (xn,yn);  T(cell(x,y)) < 0 -> OPEN, stop
 *     (px[p], py[p]) = (x, y)
 * One call with nsub = k equals k calls with nsub = 1 bit for bit.  A NaN on a face that touches land reaches no particle and
 * what land holds changes no bit.  LEFT and OPEN store where the particle went, GROUNDED does not store the rejected move.  A
 * step longer than one cell passes over cells without seeing them: the advective number of dlesm_flow_courant_f64 is the
 * check.  dlesm_drifter_sample_f64: for every ACTIVE particle with inbox(px, py), out[k][p] = fields[k](cell(px, py)) for
 * each of the nfields T-point arrays; every other out[k][p] keeps its content.
 * All arrays are device memory: the fields ny x ld with the box and its one-cell ring inside the array, px, py, status and
 * every out[k] of n elements.  fields and out are HOST arrays of nfields device pointers, passed to the kernel by value.
 * Asynchronous on `stream`, no plan, no scratch, no atomics: both calls may be captured into a graph.  On a decomposed grid
 * the flow and the mask need valid depth-1 halos; nothing is exchanged.  n == 0 or an empty box launches nothing and returns
 * 0 with every status unchanged.  DLESM_EINVAL before anything is launched: a null pointer, a double array not 8-byte
 * aligned or an int array not 4-byte aligned, n < 0, nsub outside 1..DLESM_DRIFTER_MAX_SUB, a non-finite h, nfields outside
 * 1..DLESM_DRIFTER_MAX_FIELDS, a box that does not fit with its ring, px, py or status overlapping each other or an input,
 * an out[k] overlapping an input, px, py, status or another out.  Read-only inputs may share arrays. */
enum { DLESM_DRIFTER_ACTIVE = 0, DLESM_DRIFTER_LEFT, DLESM_DRIFTER_OPEN, DLESM_DRIFTER_GROUNDED };
enum { DLESM_DRIFTER_MAX_SUB = 1024, DLESM_DRIFTER_MAX_FIELDS = 8 };
int dlesm_drifter_step_f64(double h, int nsub, int ld, int ny, int xstart, int xstop, int ystart, int ystop,
                           const int *tmask, const double *dx_t, const double *dy_t, const double *un, const double *vn,
                           long long n, double *px, double *py, int *status, void *stream);
int dlesm_drifter_sample_f64(int ld, int ny, int xstart, int xstop, int ystart, int ystop, long long n,
                             const double *px, const double *py, const int *status,
                             const double *const *fields, double *const *out, int nfields, void *stream);
/* An owner of the three particle arrays of section 6.17 on the device, for callers (Fortran, plain C) that have no device
 * arrays other than fields.  create: n >= 0 particles, status zeroed (all ACTIVE), positions not set.  put: host -> device,
 * status NULL = all ACTIVE.  get: device -> host after waiting for the device, NULL = skip that array.  arrays: the device
 * pointers, to hand to the two entries above (any of the four results may be NULL).  destroy(NULL) is accepted. */
typedef struct dlesm_drifters dlesm_drifters;
int dlesm_drifters_create(long long n, dlesm_drifters **set);
int dlesm_drifters_put(dlesm_drifters *set, const double *px, const double *py, const int *status);
int dlesm_drifters_get(dlesm_drifters *set, double *px, double *py, int *status);
int dlesm_drifters_arrays(dlesm_drifters *set, long long *n, double **px, double **py, int **status);
int dlesm_drifters_destroy(dlesm_drifters *set);

/* Particles in cell order: section 6.17's step is a gather, and particles that lie in memory in the
 * row-major order of their cells step several times faster than particles in random order.  With the box xstart..xstop x
 * ystart..ystop, nxb = xstop - xstart + 1, nyb = ystop - ystart + 1, ncells = nxb * nyb (an empty box: 0) and section 6.17's
 * inbox, evaluated in double before any conversion (a NaN or an infinity is never cast):
 *     live(p) = status[p] == DLESM_DRIFTER_ACTIVE && inbox(px[p], py[p])
 *     key(p)  = live(p) ? (floor(py[p]) - ystart) * nxb + (floor(px[p]) - xstart) : ncells            (unsigned 32-bit)
 * dlesm_particle_order_f64 writes perm[0..n), the STABLE ascending order of the keys -- key(perm[k]) does not decrease with k
 * and equal keys keep ascending p, so perm is unique -- and, where nlive is not NULL, one int on the device: the number of
 * live particles, which occupy the slots 0..nlive-1.  The dead (LEFT, OPEN, GROUNDED, any other status, outside the box)
 * follow in their old order, so later steps may pass n = nlive.  No mask and no flow array is read.  ncells == 0 gives the
 * identity and nlive = 0; n == 0 writes nlive = 0 and nothing else.  A least-significant-digit radix sort on 8-bit digits,
 * ceil(bit_length(ncells) / 8) passes (a 200 x 200 box: two), hand-written kernels, no global atomics.  scratch: device
 * memory, 16-byte aligned, of at least the bytes dlesm_particle_order_scratch gives for n (it needs no device); nothing is
 * written outside perm, nlive and those bytes.  Asynchronous on `stream`, no host synchronisation, no allocation: it may be
 * captured into a graph.
 * dlesm_particle_permute: dst[a][k] = src[a][perm[k]] for k < n and each of narrays (1..8) arrays of elem_bytes[a] (4 or 8)
 * bytes an element, in one launch that reads perm once.  An index outside 0..n-1 leaves that slot of every dst as it was: a
 * bad perm cannot fault.  src, dst and elem_bytes are HOST arrays, passed to the kernel by value.  Asynchronous, capturable.
 * DLESM_EINVAL before anything is launched: a null pointer (nlive may be NULL), n < 0 or n > 2^31-1, xstop < xstart - 1,
 * ystop < ystart - 1, ncells > 2^32-2, scratch_bytes too small, px or py not 8-byte aligned, status, perm or nlive not
 * 4-byte aligned, scratch not 16-byte aligned, a src or dst not aligned to its element, perm, nlive or scratch overlapping
 * each other or px, py or status, a dst overlapping perm, a src or another dst, narrays outside 1..8, an elem_bytes other
 * than 4 or 8.  DLESM_ENODEV without a device.
 * dlesm_particle_sort_set orders the owner's px, py and status and an int array origin: origin[k] is the index, at the last
 * dlesm_drifters_put, of the particle now in slot k (put resets it to the identity).  The pointers dlesm_drifters_arrays
 * gave stay valid and hold the sorted set.  Asynchronous on `stream`, but the first call on a set allocates its second
 * buffers and scratch (dlesm_drifters_destroy frees them), so capture only later calls.  dlesm_particle_set_origin: device
 * -> host after waiting for the device; origin (n ints) or nlive may be NULL; before the first sort since a put origin is the
 * identity and *nlive = -1 (not known). */
int dlesm_particle_order_scratch(long long n, long long *bytes);
int dlesm_particle_order_f64(int xstart, int xstop, int ystart, int ystop, long long n, const double *px, const double *py,
                             const int *status, int *perm, int *nlive, void *scratch, long long scratch_bytes, void *stream);
int dlesm_particle_permute(long long n, const int *perm, int narrays, const void *const *src, void *const *dst,
                           const int *elem_bytes, void *stream);
int dlesm_particle_sort_set(dlesm_drifters *set, int xstart, int xstop, int ystart, int ystop, void *stream);
int dlesm_particle_set_origin(dlesm_drifters *set, int *origin, long long *nlive);

/* Particles binned by cell: the Eulerian product of a particle set -- particles or mass per cell, a
 * time-integrated exposure -- as T-point fields, without atomics and with bits that can be pinned.  The box, inbox, live(p)
 * and key(p) are section 6.18's.  perm is a permutation in key order, as dlesm_particle_order_f64 gives for the same box and
 * arrays; perm == NULL is the identity, for arrays already sorted in place.  Slot k holds particle p = perm[k].  In key
 * order the particles of a live cell c are one run of slots.  For each of narrays (1..8) outputs, with w(p) = weights[a][p],
 * or 1.0 where weights[a] is NULL (the cell's count, exact as a double), the sum S_a(c) over the run has a fixed order:
 *     the chunks are the aligned groups of 64 consecutive slots, g = k >> 6;
 *     P_a(c, g) = the run's slots of chunk g added one by one in ascending k, beginning with the first of them (not with 0.0);
 *     S_a(c)    = the partials P_a(c, g) added one by one in ascending g, beginning with the first;
 * every addition rounded in double, nothing contracted.  A cell without live particle has S = +0.0.  The bits depend on the
 * inputs and on perm alone, not on the launch shape, the stream or the run.
 *     DLESM_OUT_SET: EVERY cell of the box gets out[a](c) = alpha * S_a(c), one rounding.
 *     DLESM_OUT_ADD: the cells with at least one live particle get out[a](c) = out[a](c) + alpha * S_a(c), two roundings
 *                    (alpha = dt or 1/nsteps into zeroed fields: an exposure, a time mean); every other cell keeps its bits.
 * Nothing outside the box is ever written.  The dead (key ncells) lie behind the live and add nothing.  A slot whose index is
 * outside 0..n-1 counts as dead.  unordered, where not NULL, is one int on the device: it ends as 1 if the key of some slot is
 * below that of the slot before it or an index was out of range, else as 0; equal keys being contiguous exactly when the keys
 * do not decrease, 0 means "the result is the one defined here".  With 1 the values inside the box are unspecified, and still
 * nothing but the box, the flag and the stated scratch bytes is written and no load leaves [0, n): a stale perm cannot
 * fault.  No mask and no flow array is read.
 * out[a]: device memory, ny x ld doubles, cell (i, j) at (size_t)(j-1)*ld + (i-1).  weights and out are HOST arrays of narrays
 * device pointers, passed to the kernels by value; px, py, status, perm and every weights[a] have n elements.  scratch: device
 * memory, 16-byte aligned, of at least the bytes dlesm_cell_bin_scratch gives for n and narrays (it needs no device).
 * Asynchronous on `stream`, no host synchronisation, no allocation, no global atomics: it may be captured into a graph.  n == 0
 * with DLESM_OUT_SET still fills the box; n == 0 or an empty box with DLESM_OUT_ADD touches no out.
 * DLESM_EINVAL before anything is launched: a null pointer other than perm, unordered and single weights[a], a mode other
 * than the two, a non-finite alpha, n < 0 or n > 2^31-1, narrays outside 1..8, xstop < xstart - 1, ystop < ystart - 1, a box
 * that does not fit in ld x ny, ncells > 2^32-2, a double array not 8-byte aligned, an int array not 4-byte aligned, scratch
 * not 16-byte aligned, scratch_bytes too small, an out[a], unordered or scratch overlapping each other or an input.
 * DLESM_ENODEV without a device.
 * dlesm_cell_bin_set, for callers without device arrays: the count of the owner's particles (weights NULL) into `count`.  The
 * order is computed into buffers of the owner and the particles are not moved.  Asynchronous on `stream`, but the first call
 * on a set allocates those buffers (dlesm_drifters_destroy frees them), so capture only later calls. */
int dlesm_cell_bin_scratch(long long n, int narrays, long long *bytes);
int dlesm_cell_bin_f64(int mode, double alpha, int ld, int ny, int xstart, int xstop, int ystart, int ystop, long long n,
                       const double *px, const double *py, const int *status, const int *perm, int narrays,
                       const double *const *weights, double *const *out, int *unordered, void *scratch,
                       long long scratch_bytes, void *stream);
int dlesm_cell_bin_set(dlesm_drifters *set, int mode, double alpha, int ld, int ny, int xstart, int xstop, int ystart,
                       int ystop, double *count, void *stream);

/* Drifters with random-walk diffusion: section 6.17's step plus one random kick per substep, for a
 * constant horizontal diffusivity kh in m2/s -- a cloud released at one place spreads.  The grid, the box, inbox, cell, vel,
 * the statuses and the arithmetic rules are section 6.17's.  The numbers come from Philox4x32-10 as published (Salmon et al.,
 * Random123: multipliers 0xD2511F53 and 0xCD9E8D57, key increments 0x9E3779B9 and 0xBB67AE85, ten rounds), a counter-based
 * generator: no state is stored anywhere.  For particle p and substep s = 0..nsub-1 of a call:
 *     tau = tick + (tick_dev ? *tick_dev : 0) + s                                                   (64-bit)
 *     w   = philox4x32_10(counter = (id_p, 0, lo32(tau), hi32(tau)), key = (lo32(seed), hi32(seed)))
 *     rx  = ((double)w[0] + 0.5) * 0x1p-31 - 1.0      ry = ((double)w[1] + 0.5) * 0x1p-31 - 1.0     (exact, in (-1, 1), never 0)
 *     amp = sqrt((6.0 * kh) * fabs(h))                                          (on the host, once per call; metres)
 *     gx  = (amp * rx) / dx_t(i,j)                    gy = (amp * ry) / dy_t(i,j)      ((i,j): the cell at the substep's start)
 * id_p = id[p] taken as 32 bits (any values, duplicates allowed), or (uint32)p when id is NULL.  The kick's variance is
 * 2 kh |h| per axis.  A substep computes k1, the midpoint and k2 as section 6.17 and, with D = (x + k2x, y + k2y):
 *     A = (D.x + gx, D.y + gy)
 *     !inbox(A)        -> (x,y) = A, LEFT, stop
 *     T(cell(A)) != 0  -> (x,y) = A; OPEN and stop if T < 0
 *     T(cell(A)) == 0  -> the kick is rejected and D meets section 6.17's rule: !inbox(D) -> (x,y) = D, LEFT, stop;
 *                         T(cell(D)) == 0 -> GROUNDED, stop (position kept); (x,y) = D; T(cell(D)) < 0 -> OPEN, stop
 * The entry test and the particles that are not ACTIVE are section 6.17's.  kh == 0 gives dlesm_drifter_step_f64's bits.  One
 * call with nsub = k at tick t equals k calls with nsub = 1 at ticks t .. t+k-1.  A particle's path depends on its id, not on
 * its slot: sorting between calls with the ids carried along changes no particle's bits.  In still water nobody is GROUNDED:
 * a kick onto land is rejected, the no-flux wall.  Same seed, ids and ticks give the same bytes on any stream and any run.
 * seed: any 64 bits.  tick >= 0 with tick + nsub representable: the caller's count of substeps so far.  tick_dev: NULL, or one
 * 8-byte-aligned long long on the device whose value the kernel adds to tick; behind the step a one-lane launch on the same
 * stream does *tick_dev += nsub, so that a captured time loop draws fresh numbers on every replay and equals eager calls with
 * tick advanced by hand.  A GRAPH CAPTURED WITHOUT tick_dev REPLAYS THE SAME KICKS: tick is baked into it.
 * Asynchronous on `stream`, no plan, no scratch, no atomics, no allocation, no host synchronisation.  n == 0 or an empty box
 * launches nothing and returns 0, *tick_dev unchanged.  DLESM_EINVAL before anything is launched: everything
 * dlesm_drifter_step_f64 refuses, kh negative or not finite, tick < 0 or tick + nsub overflowing, id not 4-byte aligned,
 * tick_dev not 8-byte aligned, id or tick_dev overlapping px, py or status, tick_dev overlapping an input.
 * dlesm_dispersal_step_set steps the owner's particles with the set's origin (section 6.18) as id -- before the first sort
 * since a put that is the identity, NULL --, so a set's particles keep their random streams through
 * dlesm_particle_sort_set. */
int dlesm_dispersal_step_f64(double h, int nsub, double kh, long long seed, long long tick, const long long *tick_dev,
                             int ld, int ny, int xstart, int xstop, int ystart, int ystop, const int *tmask,
                             const double *dx_t, const double *dy_t, const double *un, const double *vn, long long n,
                             const int *id, double *px, double *py, int *status, void *stream);
int dlesm_dispersal_step_set(dlesm_drifters *set, double h, int nsub, double kh, long long seed, long long tick,
                             const long long *tick_dev, int ld, int ny, int xstart, int xstop, int ystart, int ystop,
                             const int *tmask, const double *dx_t, const double *dy_t, const double *un, const double *vn,
                             void *stream);

/* Drifters in a varying diffusivity: section 6.20's step with the kick made from a T-point field
 * kh_t (m2/s; ld x ny doubles laid out like dx_t) instead of one number, with the drift correction of Visser (1997), so that
 * a well-mixed cloud stays well mixed where kh_t varies -- a walk without the drift collects particles where mixing is weak.
 * Everything of section 6.20 holds -- the generator, its counter and key, rx, ry, tau, k1, the midpoint and k2, D, A = D +
 * (gx, gy), the destination rule on A then D, the entry test, the statuses, tick, tick_dev and the ids -- except how the kick
 * is made.  With (i,j) the particle's cell at the substep's start, a = x - i, b = y - j there, t_e..t_s the four neighbours'
 * masks, dx = dx_t(i,j), dy = dy_t(i,j), every operation rounded in double in the order written:
 *     Kc  = kh_t(i,j)
 *     ke  = t_e != 0 ? 0.5*(Kc + kh_t(i+1,j)) : Kc      kw, kn, ks likewise        (face values; a coast face takes the cell's own)
 *     ah  = fabs(h)
 *     dkx = ke - kw                         dky = kn - ks
 *     cx  = (ah * dkx) / (dx * dx)          cy  = (ah * dky) / (dy * dy)           (the drift, in cells)
 *     kx  = kw + dkx * (a + 0.5*cx)         ky  = ks + dky * (b + 0.5*cy)          (K half a drift ahead, linear in the cell)
 *     kx  = kx > 0.0 ? kx : 0.0             ky likewise
 *     gx  = cx + (sqrt((6.0*kx) * ah) * rx) / dx
 *     gy  = cy + (sqrt((6.0*ky) * ah) * ry) / dy
 * The five values of kh_t are read whatever the masks say; a neighbour that is wet or open (T != 0) is used, ring cells outside
 * the box included, and what a land cell of kh_t holds changes no bit.  kh_t must be finite and >= 0 on the cells with T != 0:
 * the caller's responsibility, the host cannot see the field; any other value is carried through the arithmetic above and
 * cannot fault.  kh_t == kh on every cell with T != 0 gives dlesm_dispersal_step_f64(kh)'s bits, kh_t == 0 there
 * dlesm_drifter_step_f64's.  Keep |cx| + sqrt(6 K |h|) / dx below one cell, and h short where the gradients of neighbouring
 * faces differ strongly.  Asynchronous on `stream`, no plan, no scratch, no atomics, no allocation, no host synchronisation.
 * n == 0 or an empty box launches nothing and returns 0, *tick_dev unchanged.  DLESM_EINVAL before anything is launched:
 * everything dlesm_dispersal_step_f64 refuses of the arguments they share, kh_t NULL or not 8-byte aligned, kh_t overlapping
 * px, py, status or tick_dev.  dlesm_random_walk_set steps the owner's particles with the set's origin as id, like
 * dlesm_dispersal_step_set. */
int dlesm_random_walk_f64(double h, int nsub, const double *kh_t, long long seed, long long tick, const long long *tick_dev,
                          int ld, int ny, int xstart, int xstop, int ystart, int ystop, const int *tmask,
                          const double *dx_t, const double *dy_t, const double *un, const double *vn, long long n,
                          const int *id, double *px, double *py, int *status, void *stream);
int dlesm_random_walk_set(dlesm_drifters *set, double h, int nsub, const double *kh_t, long long seed, long long tick,
                          const long long *tick_dev, int ld, int ny, int xstart, int xstop, int ystart, int ystop,
                          const int *tmask, const double *dx_t, const double *dy_t, const double *un, const double *vn,
                          void *stream);

/* Particles that cross rank boundaries: on a decomposed grid a particle that leaves its tile is handed
 * to the neighbouring rank on the device, without a host copy of px, py or status.  A particle set is arrays of a fixed length n,
 * the capacity; a slot whose status is DLESM_DRIFTER_FREE holds no particle (every entry of sections 6.17-6.20 treats it as
 * dead, like any status other than ACTIVE).  A departure frees its slot, an arrival takes a FREE one.  With a particle travel
 * `long long id[n]` -- so that section 6.20's random streams follow it -- and npayload (0..DLESM_MIGRATE_MAX_PAYLOAD) further
 * arrays of one 8-byte word per slot, moved as raw bits.  The box and inbox are section 6.17's, evaluated in double before any
 * conversion.  Directions: W, E, S, N = 0..3; axis DLESM_MIGRATE_X serves W and E (d = 0, 1), DLESM_MIGRATE_Y S and N.
 * A MESSAGE of capacity cap is one contiguous device buffer, 16-byte aligned: `long long count`, 8 bytes of padding, then
 * x[cap] | y[cap] | id[cap] | payload_0[cap] | ...; dlesm_migrate_bytes gives its size, 16 + (3 + npayload) * 8 * cap.  Words past
 * count, and the padding, are never written by pack.
 * dlesm_migrate_pack_f64, axis X: slot p is a W departure if status[p] == LEFT, px[p] and py[p] are finite, px[p] < xstart and
 * has_neighbour[0] != 0; an E departure if instead px[p] >= xstop + 1 and has_neighbour[1] != 0.  Axis Y: xstart <= px[p] <
 * xstop + 1 is required too, then S if py[p] < ystart and has_neighbour[0], N if py[p] >= ystop + 1 and has_neighbour[1].  The
 * k-th departure of direction d in ascending slot order, k < cap: send[d] gets x = px[p] + (double)shift_x[d], y = py[p] +
 * (double)shift_y[d] (one rounded add each), id[p] and the payload words at index k, and status[p] becomes FREE.  k >= cap: the
 * particle is HELD, nothing changes, a later call retries it.  count = min(departures, cap).  Everything else stays as it is: a
 * LEFT particle at the edge of the global domain (no neighbour), one with a NaN or an infinite position, one outside in x on
 * a side without neighbour while outside in y.  px, py, id and the payload are only read.
 * dlesm_migrate_unpack_f64: the arrivals are the records 0..count-1 of recv[0] (from the low side: W or S), then those of
 * recv[1]; arrival j goes into the j-th FREE slot in ascending slot order: px, py, id and the payload are stored and status
 * becomes inbox(x, y) ? ACTIVE : LEFT (so phase Y forwards a corner crossing, a later call a jump longer than a tile; an
 * arrival on land or an open cell is classified by the next step's entry test).  Arrivals beyond the FREE slots are DROPPED
 * and counted.  A header count outside 0..cap counts as 0 and sets bit (1 << direction) of bad_message: a bad message cannot
 * fault.  Unpack after pack of the same axis reuses the slots that pack has freed.
 * The record, on the device: pack stores sent[] and held[] of its two directions; unpack stores arrived[] of its two (by the
 * side they came from), nfree (the FREE slots after it) and -- axis X: sets, axis Y: adds to / ors into -- dropped and
 * bad_message.  After pack X, unpack X, pack Y, unpack Y every word is defined.
 * scratch: device memory, 16-byte aligned, of at least the bytes dlesm_migrate_scratch gives for n (it needs no device, nor do
 * dlesm_migrate_bytes and dlesm_migrate_work).  payload, send, recv, has_neighbour, shift_x and shift_y are HOST arrays, passed
 * to the kernels by value.  Both calls are asynchronous on `stream`, allocate nothing, do not synchronise, use no global
 * atomics and may be captured into a graph: count, scan, scatter over 4096-slot tiles, hand-written kernels.
 * dlesm_migrate_exchange, the transport: send[d] travels to rank neighbour[d] (0-based), recv[d] receives what that rank sent
 * towards this one.  neighbour[d] < 0: recv[d]'s count becomes 0.  neighbour[d] == the caller's rank (0 without a
 * communicator): send[d] is copied into recv[1 - d] on the device -- one rank whose W and E neighbour is itself, with shifts
 * +nxb and -nxb, is a periodic channel.  Collective and synchronous, after waiting for `stream`; every rank passes the same
 * bytes.  Mailbox mode stages both messages through the host and the board, O(ranks x bytes) per rank; RCCL sends and receives
 * one grouped pair per neighbour.  The same other rank on both sides is refused.
 * dlesm_migrate_f64: pack X, exchange, unpack X, pack Y, exchange, unpack Y -- a particle that leaves through a corner makes
 * both hops in one call.  neighbour[4] (< 0: none), shift_x[4], shift_y[4] in the order W, E, S, N; work: device memory, 16-byte
 * aligned, of dlesm_migrate_work(n, cap, npayload) bytes, holding the eight messages and the scratch.  Collective, synchronous.
 * A particle that crosses loses the rest of the substeps of the step that made it LEFT: step with nsub = 1 for no lag.
 * DLESM_EINVAL before anything is launched: a null pointer, px, py, id or a payload not 8-byte aligned, status or counts not
 * 4-byte aligned, a message, scratch or work not 16-byte aligned, n outside 0..2^31-1, cap outside 1..2^31-1, npayload outside
 * 0..4, an axis other than 0 or 1, xstop < xstart - 1, ystop < ystart - 1, scratch_bytes or work_bytes too small, an array that
 * is written overlapping any other array.  DLESM_ENODEV without a device. */
enum { DLESM_DRIFTER_FREE = 4 };        /* follows DLESM_DRIFTER_GROUNDED */
enum { DLESM_MIGRATE_MAX_PAYLOAD = 4 };
enum { DLESM_MIGRATE_W = 0, DLESM_MIGRATE_E, DLESM_MIGRATE_S, DLESM_MIGRATE_N };
enum { DLESM_MIGRATE_X = 0, DLESM_MIGRATE_Y = 1 };
typedef struct dlesm_migrate_counts {
    int sent[4];
    int held[4];
    int arrived[4];
    int dropped;
    int nfree;
    int bad_message;
    int pad;
} dlesm_migrate_counts;                 /* 64 bytes, no holes */
int dlesm_migrate_bytes(long long cap, int npayload, long long *bytes);
int dlesm_migrate_scratch(long long n, long long *bytes);
int dlesm_migrate_work(long long n, long long cap, int npayload, long long *bytes);
int dlesm_migrate_pack_f64(int axis, int xstart, int xstop, int ystart, int ystop, long long n, const double *px,
                           const double *py, int *status, const long long *id, const void *const *payload, int npayload,
                           const int *has_neighbour, const int *shift_x, const int *shift_y, long long cap, void *const *send,
                           dlesm_migrate_counts *counts, void *scratch, long long scratch_bytes, void *stream);
int dlesm_migrate_unpack_f64(int axis, int xstart, int xstop, int ystart, int ystop, long long n, double *px, double *py,
                             int *status, long long *id, void *const *payload, int npayload, long long cap,
                             const void *const *recv, dlesm_migrate_counts *counts, void *scratch, long long scratch_bytes,
                             void *stream);
int dlesm_migrate_exchange(const int *neighbour, const void *const *send, void *const *recv, long long bytes, void *stream);
int dlesm_migrate_f64(int xstart, int xstop, int ystart, int ystop, long long n, double *px, double *py, int *status,
                      long long *id, void *const *payload, int npayload, const int *neighbour, const int *shift_x,
                      const int *shift_y, long long cap, dlesm_migrate_counts *counts, void *work, long long work_bytes,
                      void *stream);

/* Particle sources that fill FREE slots on the device: particles are created during the run, at a rate,
 * at places -- a spill, a spawning reef, an outfall -- without a copy of the set to the host, and a run on any decomposition
 * releases the particles of the undivided run.  `sources` is a DEVICE table of nsources records; every rank passes the same
 * table, seed and max_count and its own box, offx = global minus local x of its tile (0 on an undivided grid), offy likewise.
 * Every operation is rounded in double in the order written.
 * Source s is VALID iff x, y, rx, ry are finite, rx >= 0, ry >= 0 and count >= 0.  An invalid source gives c_s = 0, adds 1 to
 * bad_source and keeps its next_id; a valid one gives c_s = min(count, max_count), and clamped counts those with count >
 * max_count.  requested = sum of c_s.  Candidate (s, m), 0 <= m < c_s, with 64-bit wrapping id arithmetic:
 *     id = next_id_s + m
 *     w  = philox4x32_10(counter = (lo32(id), 1, hi32(id), 0), key = (lo32(seed), hi32(seed)))
 *     gx = x_s + rx_s * philox_sym(w[0])          gy = y_s + ry_s * philox_sym(w[1])
 * (section 6.20's generator and its rx expression; its kicks have 0 in the counter's second word, so no release number is a
 * kick number).  A position depends on the id and the seed alone.  The candidate is OWNED iff gx and gy are finite,
 * (double)((long long)xstart + offx) <= gx < (double)((long long)xstop + 1 + offx) and the same in y: the tiles of a
 * decomposition tile the global box, so exactly one rank owns a candidate inside the domain.  One that is not owned adds 1 to
 * `foreign` and nothing else.  An owned one has lx = gx - (double)offx, ly = gy - (double)offy.  !inbox(lx, ly) (section
 * 6.17's; only when the subtraction rounds up onto the upper edge): ACCEPTED with status LEFT, counted by `edge`, for section
 * 6.21 to hand over.  Otherwise T = tmask(cell(lx, ly)): T == 0 adds 1 to on_land and creates nothing, T != 0 is ACCEPTED as
 * ACTIVE (on an open cell the next step's entry test classifies it).  The accepted, ordered source-major with m ascending:
 * accepted k takes the k-th FREE slot p in ascending slot order and stores px[p] = lx, py[p] = ly, status[p], id[p] = id,
 * tag[p] = tag_s if tag is not NULL, born[p] = tick + (tick_dev ? *tick_dev : 0) if born is not NULL; those beyond the FREE
 * slots add to `dropped` and are lost.  released: the number stored; nfree: the FREE slots afterwards; edge counts every
 * accepted LEFT candidate, stored or not; requested == released + dropped + foreign + on_land.  No other slot and no other
 * word is written.  Then next_id_s += c_s for every valid source, on the stream, behind the fill: ids are consumed whether or
 * not a candidate was owned, wet or placed, so every rank's table advances alike and a captured graph releases fresh ids at
 * every replay.  tick_dev is only read.
 * Asynchronous on `stream`; no allocation, no host synchronisation, no global atomics, plain vector stores; capturable.
 * scratch: device memory, 16-byte aligned, of at least dlesm_release_scratch(n, nsources, max_count) bytes (tables of counts and
 * a staging area of min(n, nsources * max_count) records of 36 bytes).  n == 0, nsources == 0 or an empty box: counts is filled
 * as the rule gives, ids advance, 0 is returned.  DLESM_EINVAL before anything is launched: a null tmask, sources, px, py,
 * status, id, counts or scratch; sources, px, py, id, tag, born, tick_dev or counts not 8-byte aligned, tmask or status not
 * 4-byte aligned, scratch not 16-byte aligned; n outside 0..2^31-1; nsources outside 0..DLESM_RELEASE_MAX_SOURCES; max_count
 * < 1, nsources * max_count > 2^31-1 or nsources * ceil(max_count / 256) > 2^22; tick < 0; a box that does not fit ld x ny
 * with its one-cell ring; scratch_bytes too small; a written array (px, py, status, id, tag, born, sources, counts, scratch)
 * overlapping any other array.  DLESM_ENODEV without a device. */
typedef struct dlesm_release_source {   /* 64 bytes, no holes; a DEVICE table of nsources of them */
    double x, y;          /* centre of the patch, GLOBAL index coordinates (T cell (i,j) covers [i,i+1) x [j,j+1)) */
    double rx, ry;        /* half-widths in cells, >= 0; 0 = a point source */
    long long next_id;    /* id of this source's next particle; the call advances it */
    long long count;      /* particles wanted from this source at the next call; the call leaves it alone */
    long long tag;        /* any 8 bytes (a source number, a mass as double bits): stored per new particle */
    long long pad;
} dlesm_release_source;
typedef struct dlesm_release_counts {   /* 64 bytes, no holes, on the device */
    long long requested;
    int released, foreign, on_land, dropped, edge, nfree, clamped, bad_source;
    int pad[6];
} dlesm_release_counts;
enum { DLESM_RELEASE_MAX_SOURCES = 65536 };
int dlesm_release_scratch(long long n, int nsources, int max_count, long long *bytes);   /* needs no device */
int dlesm_release_f64(int ld, int ny, int xstart, int xstop, int ystart, int ystop, int offx, int offy, const int *tmask,
                      dlesm_release_source *sources, int nsources, int max_count, long long seed, long long tick,
                      const long long *tick_dev, long long n, double *px, double *py, int *status, long long *id,
                      long long *tag, long long *born, dlesm_release_counts *counts, void *scratch,
                      long long scratch_bytes, void *stream);

/* One coupled time step on a decomposed grid: the flow from level n to n+1 and ntracers
 * (0..DLESM_TRACER_MAX) tracers carried by the level-n transports into the new water column, on ONE plan of depth 1 or 2, with
 * ONE exchange of the 5 + ntracers outputs.  Bit for bit, in every cell of every array (halos and padding included), what this
 * definition leaves: dlesm_continuity_f64 over tbox with params->rdt; dlesm_halo_exchange_f64(plan, ssha, DLESM_DIRS_ALL);
 * next_sshu / next_sshv, momentum and, when obc is not NULL, bc_open, as dlesm_nemolite_step_f64 runs them (wet != NULL: the
 * contract of dlesm_nemolite_step_wet_f64 for land ssha); the single-domain tracer entry of `scheme` (dlesm_tracer_step_f64,
 * _muscl_f64 or _hancock_f64) with params->rdt over tbox, grid->tmask, area_t, the level-n flow arrays and the ssha just made,
 * c_in to c_out; dlesm_halo_exchange_multi_f64(plan, {ssha, ssha_u, ssha_v, ua, va, c_out[0..ntracers-1]}, 5 + ntracers,
 * DLESM_DIRS_ALL).  The tracer update reads ssha in its own wet cell only and everything else at level n, so one exchange
 * serves both.
 * In: the level-n flow arrays with valid depth-1 halos, corners included, as for dlesm_nemolite_step_dm; c_in with depth-1 halos
 * for DLESM_TRACER_UPWIND; c_in and grid->tmask with depth-2 halos for the two limited schemes (dlesm_halo_exchange_i32 fills
 * the mask's).  Out: all 5 + ntracers outputs with halos of the plan's depth; a time loop only rotates the pointers.
 * ntracers = 0 is the flow step alone, on a plan of either depth (c_in / c_out may be NULL; scheme is still checked).
 * A plan without messages: dlesm_nemolite_step_wet_f64, then the tracer entry over tbox, for any boxes.  A plan with messages
 * needs tbox == ubox == vbox, x and y receive messages all of depth 1 or all of depth 2, and depth 2 when ntracers > 0 and the
 * scheme is a limited one.  DLESM_EINVAL before anything is launched or exchanged: every refusal of dlesm_nemolite_step_wet_f64
 * and of the tracer entries, a scheme outside 0..2, ntracers outside 0..DLESM_TRACER_MAX, a c_out[k] that overlaps ssha_u,
 * ssha_v, ua, va or an array of grid, a null plan, a plan for other extents, another or a mixed depth, a limited scheme on a
 * depth-1 plan, and the guards of the other *_dm entries.  Over connected mailboxes the exchange runs in
 * ceil((5 + ntracers) / mailbox fields) turns on every rank, whatever the box, obc, the wet plan or the path the step takes;
 * over RCCL it is one aggregated group.  obc and wet are rank-local.  Collective: every rank calls it, in the same order. */
enum { DLESM_TRACER_UPWIND = 0, DLESM_TRACER_MUSCL = 1, DLESM_TRACER_HANCOCK = 2 };
int dlesm_nemolite_coupled_step_dm(dlesm_halo_plan *plan, const dlesm_wet_plan *wet, int scheme,
                                   const dlesm_momentum_params *params, const dlesm_momentum_grid *grid,
                                   const double *area_t, int ld, int ny, const dlesm_region *tbox, const dlesm_region *ubox,
                                   const dlesm_region *vbox, const dlesm_obc *obc, double ssh_bc, const double *un, const double *vn,
                                   const double *ht, const double *hu, const double *hv, const double *sshn_t, const double *sshn_u,
                                   const double *sshn_v, double *ssha, double *ssha_u, double *ssha_v, double *ua, double *va,
                                   const double *const *c_in, double *const *c_out, int ntracers, void *stream);
/* The halos of one int field of the plan's extents (ny x ld, device) from the neighbours: after the
 * call every cell a receive message of the plan covers holds the sending rank's value, and no other cell has changed.  All
 * directions, a plan of any depth; a plan without messages does nothing.  The values travel as doubles (exact for every int)
 * through a scratch of ld x ny doubles the plan owns, allocated by the first call and freed with the plan: one mailbox
 * operation per rank.  Asynchronous on `stream`.  DLESM_EINVAL: a null plan or field, an earlier wait that timed out, a stream
 * that is being captured (the first call allocates).  Collective: every rank calls it, in the same order. */
int dlesm_halo_exchange_i32(dlesm_halo_plan *plan, int *field, void *stream);

/* global_sum, parallel_utils_mod.f90:230-238: in-place sum of one host double
 * over all ranks (synchronous). */
int dlesm_global_sum_f64(double *value);
/* In-place max of one host double over all ranks (synchronous); a NaN on any rank gives NaN on every rank.  One rank: a
 * no-op.  Mailbox mode: gathered over the board; RCCL: one double per rank all-gathered; either way the max is taken on
 * the host in rank order (not ncclMax, whose NaN behaviour is unspecified). */
int dlesm_global_max_f64(double *value);
/* gather, parallel_utils_mod.f90:242-255: n doubles per rank (device memory)
 * -> n*nranks doubles on rank 0 (device memory). Synchronous. */
int dlesm_gather_f64(const double *send, double *recv, int n);

/* ------------------------------------------------------------------------
 * 6. Device-side gather / scatter of whole fields
 *    (gather_inner_data, field_mod.f90:1313-1390; the init_global_data scatter of the
 *     constructor, field_mod.f90:378-389)
 * ---------------------------------------------------------------------- */

/* Pack loop of gather_inner_data (field_mod.f90:1360-1368): the box of a device field, j outer /
 * i inner, into send[0 .. nx*ny); the rest of the slot (tiles are uneven, every rank sends the
 * size of the largest one, field_mod.f90:1348-1351) is zeroed.  slot >= nx*ny. */
int dlesm_pack_inner_f64(const double *field, int ld, int ny, int xstart, int xstop, int ystart,
                         int ystop, double *send, long slot, void *stream);

/* Unpack loop of gather_inner_data on rank 0 (field_mod.f90:1372-1386): slot r of `recv` (slot
 * doubles each) goes to rank r's box in the global array, `global` being a device array of
 * global_nx x global_ny doubles (column-major, like the Fortran result).  One launch for all ranks. */
int dlesm_unpack_gathered_f64(const double *recv, long slot, const dlesm_decomp *decomp,
                              const dlesm_subdomain *subdomains, int nranks, double *global,
                              void *stream);

/* gather_inner_data for a device-resident field: pack on the device, ncclSend/ncclRecv to rank 0
 * (MPI_Gather of parallel_utils_mod.f90:242-255), unpack on the device, ONE device-to-host copy of
 * the global array into global_host (global_nx x global_ny doubles; only read on rank 0, may be
 * NULL elsewhere).  internal: this rank's internal region (halo_x = xstart-1, halo_y = ystart-1,
 * field_mod.f90:1348-1349).  Synchronous.  With one rank: the copy-out of field_mod.f90:1332-1343. */
int dlesm_gather_inner_f64(const double *field, int ld, int ny, const dlesm_region *internal,
                           const dlesm_decomp *decomp, const dlesm_subdomain *subdomains,
                           int nranks, double *global_host);

/* The constructor's scatter (field_mod.f90:378-389): this rank's internal region of the device
 * field <- the matching patch of a HOST global array (global_nx x global_ny), one strided
 * host-to-device copy.  sub: this rank's subdomain (its global box gives the patch). Synchronous. */
int dlesm_scatter_inner_f64(const double *global_host, int global_nx, int global_ny,
                            const dlesm_subdomain *sub, double *field, int ld, int ny);

#ifdef __cplusplus
}
#endif
#endif /* DLESM_HIP_H */
