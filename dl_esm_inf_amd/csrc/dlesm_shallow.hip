// Shallow-water u/v/h update as a register-tiled linear sweep.
//
// 72 B/cell of algorithmic traffic: u, v, p (3x3 footprint), uold, vold, pold read once,
// unew, vnew, pnew written once; cu, cv, z, h never touch memory.
//
// Work unit: a wave tile of 56 output lanes x 2 doubles x R rows.  A wave loads 64 lanes
// (one 16-byte-aligned, 1 KiB-contiguous access per row): the outer lanes are halo lanes whose
// values only feed their neighbours through wave64 shuffles, so there are no scattered edge
// loads and every cross-lane value -- raw (p, v east; u west) or derived (cu, z west; cv, h
// east) -- is one shuffle away.  ONE halo lane per side is all the arithmetic needs; FOUR are
// given up (sw_halo_lanes) when rows start on lines, so that a tile's 112 output columns are seven WHOLE 128-byte lines
// of every array written: with 62 output lanes the tile edges fell inside a line (at 992-byte
// steps) and two of every 8.75 lines stored per row were partial.  Measured at 8192^2, same
// box, planned shapes (round 4): step 0.823 -> 0.808 ms, filtered step 1.18 -> 1.12 ms, the
// periodic forms alike, against 12.5 % more lanes loaded (L2 hits: the neighbouring tile's
// lines); eight halo lanes (loads on whole lines as well) 0.814 / 1.13.
// Tiles are numbered row-major and workgroups sweep memory
// linearly in dispatch order, exactly as jacobi5_tile does (see the notes there); the
// (R+2)-row overlap between vertically adjacent tiles is served by L2 / Infinity Cache.
//
// The expression trees are exactly those of the specification in DESIGN.md section 6 and the
// file is compiled with -ffp-contract=off, so results agree bit for bit with the CPU checker
// used by the tests.
#include <map>
#include <mutex>
#include <tuple>
#include <vector>

#include "dlesm_internal.h"
#include "dlesm_device.h"

namespace dlesm {

namespace {

typedef double d2 __attribute__((ext_vector_type(2)));

// lanes per side that only feed their neighbours: 4 (56 output chunks = 112 columns = 7 whole lines of 128 bytes) when every
// row of every array starts on a line -- an even pitch that is a multiple of 16 doubles, line-aligned bases: DL_ESM_ALIGNMENT a
// multiple of 16 --, else 1 (62 output chunks): on an odd pitch (the reference's default alignment) no tile covers whole lines
// whatever its width, and the wider halo only costs (8192^2, alignment 1, planned shapes, same box: step 0.836-0.845 ms with
// 56 lanes against 0.808-0.813 with 62).
static inline int sw_halo_lanes(int ld, const SwFields &f)
{
    bool lines = ld % 16 == 0;
    for (const double *a : {f.u, f.v, f.p, f.uold, f.vold, f.pold, (const double *)f.unew, (const double *)f.vnew, (const double *)f.pnew})
        lines = lines && ((uintptr_t)a % 128 == 0);
    return lines ? 4 : 1;
}

struct V2 {
    double x, y;
};

template <bool NT = false>
__device__ __forceinline__ V2 ld2(const double *p)
{
    d2 t = NT ? __builtin_nontemporal_load((const d2 *)p) : *(const d2 *)p;
    return V2{t.x, t.y};
}
template <bool NT>
__device__ __forceinline__ void st2(double *p, const V2 &v)
{
    if constexpr (NT) __builtin_nontemporal_store(d2{v.x, v.y}, (d2 *)p);
    else *(d2 *)p = d2{v.x, v.y};
}
// value of the column to the east / west of each of the lane's two columns
// (DPP: whole-wave shift on the VALU instead of ds_bpermute, see dlesm_internal.h)
template <bool DPP> __device__ __forceinline__ V2 east_of(const V2 &a) { return V2{a.y, from_upper<DPP>(a.x)}; }
template <bool DPP> __device__ __forceinline__ V2 west_of(const V2 &a) { return V2{from_lower<DPP>(a.y), a.x}; }

#define EW(expr_x, expr_y) V2{(expr_x), (expr_y)}
// the old level: read-only and restrict-qualified in the plain step; the filtered step (SM) also writes it, through
// SwSmooth's pointers, so there it must not promise no-alias
typedef const double *__restrict__ OldLevelRO;
typedef const double *OldLevelRW;
template <bool SM> struct OldLevel { typedef OldLevelRO ptr; };
template <> struct OldLevel<true> { typedef OldLevelRW ptr; };
// The Asselin filter of the GOcean leapfrog (time_smooth) folded into the step: with uo != nullptr
// the old level is ALSO updated in place, uold <- u + alpha*(unew - 2*u + uold) (likewise v, p), from values the lane
// already holds -- three more stores per cell instead of three more launches that re-read nine arrays: 96 B/cell for a
// whole filtered time step against 72 + 3 x 32 = 168.  uo, vo, po are the old arrays themselves (writable).
struct SwSmooth {
    double alpha;
    double *uo, *vo, *po;
};
[[maybe_unused]] __device__ __forceinline__ V2 pin_here(const V2 &a) { return V2{::dlesm::pin_here(a.x), ::dlesm::pin_here(a.y)}; }   // dlesm_internal.h
// new time level stored non-temporally by default: +1.2 % at 8192^2 (profiles/r02_shallow_variants.txt)
#define SW_NT_DEFAULT 2
// ... unless the nine arrays of the step fit the 256 MB Infinity Cache together: a store that bypasses it takes the next step's
// input away (the Jacobi sweep's finding at 4096^2, nt_stores_for).  Measured with the round-4 tile, rule shapes, time-loop
// rotation: 1024^2 (80 MB) 0.0153 ms cached against 0.0165; 1536^2 (177 MB) 0.0296 / 0.0301; 2048^2 (312 MB) 0.0537 / 0.0510.
static inline int sw_nt_default(int ld, int y0, int y1)
{
    return 9.0 * 8.0 * (double)ld * (double)(y1 - y0 + 3) <= 200.0e6 ? 0 : SW_NT_DEFAULT;
}

// NTM bit 0: the old time level (read exactly once, by one lane) is loaded non-temporally;
// bit 1: the new time level is stored non-temporally.  u, v, p keep the default policy: their
// rows are re-read by the tile below.
template <int R, bool DPP, int NTM, bool SM = false>
__device__ __forceinline__ void shallow_tile_body(
    const dlesm_sw_params &q, int ld, int x0, int x1, int y0, int y1, int cb, int nxw, int hl,
    const double *__restrict__ u, const double *__restrict__ v, const double *__restrict__ p,
    typename OldLevel<SM>::ptr uold, typename OldLevel<SM>::ptr vold, typename OldLevel<SM>::ptr pold,
    double *__restrict__ unew, double *__restrict__ vnew, double *__restrict__ pnew, unsigned block, int stack = 1,
    SwSmooth sm = SwSmooth{0.0, nullptr, nullptr, nullptr})
{
    auto east = [](const V2 &a) { return east_of<DPP>(a); };
    auto west = [](const V2 &a) { return west_of<DPP>(a); };
    const int lane = threadIdx.x & 63;
    int xw, strip;
    if (stack <= 1) {
        const int w = block * (blockDim.x >> 6) + (threadIdx.x >> 6);
        xw = w % nxw, strip = w / nxw;
    } else {
        // `stack` vertically adjacent tiles per workgroup (experiment, sw_stack): the halo rows two tiles of a
        // group share are then requested by one CU at about the same time
        const int wv = threadIdx.x >> 6, sx = (blockDim.x >> 6) / stack, nbx = (nxw + sx - 1) / sx;
        xw = (int)(block % nbx) * sx + wv % sx;
        strip = (int)(block / nbx) * stack + wv / sx;
        if (xw >= nxw) return;
    }
    const int jb = y0 + strip * R;
    if (jb > y1) return;
    int je = jb + R - 1;
    if (je > y1) je = y1;
    const int c = cb + xw * (64 - 2 * hl) - hl + lane;             // this lane's chunk (2 columns)
    if (c - lane + hl > x1 / 2) return;                 // idle padding tile
    const int c_ld = ld / 2 - 1;
    const int cl = c < 0 ? 0 : (c > c_ld ? c_ld : c);  // halo / trailing lanes: any valid chunk
    const bool out_lane = lane >= hl && lane < 64 - hl && c <= c_ld;
    const bool m0 = out_lane && 2 * c >= x0 && 2 * c <= x1;
    const bool m1 = out_lane && 2 * c + 1 >= x0 && 2 * c + 1 <= x1;

    const size_t col = (size_t)cl * 2;
    // rows jb-1 .. jb+R of u, v, p ; rows jb .. jb+R-1 of the old fields (clamped past je+1 / je)
    V2 U[R + 2], Vv[R + 2], P[R + 2], UO[R], VO[R], PO[R];
    if constexpr ((NTM & 4) != 0) {     // experiment: the once-read old level requested first
#pragma unroll
        for (int k = 0; k < R; k++) {
            int jj = jb + k;
            if (jj > je) jj = je;
            const size_t o = (size_t)jj * ld + col;
            UO[k] = ld2<(NTM & 1) != 0>(uold + o);
            VO[k] = ld2<(NTM & 1) != 0>(vold + o);
            PO[k] = ld2<(NTM & 1) != 0>(pold + o);
        }
    }
#pragma unroll
    for (int k = 0; k < R + 2; k++) {
        int jj = jb - 1 + k;
        if (jj > je + 1) jj = je + 1;
        const size_t o = (size_t)jj * ld + col;
        U[k] = ld2(u + o);
        Vv[k] = ld2(v + o);
        P[k] = ld2(p + o);
    }
    if constexpr ((NTM & 4) == 0) {
#pragma unroll
        for (int k = 0; k < R; k++) {
            int jj = jb + k;
            if (jj > je) jj = je;
            const size_t o = (size_t)jj * ld + col;
            UO[k] = ld2<(NTM & 1) != 0>(uold + o);
            VO[k] = ld2<(NTM & 1) != 0>(vold + o);
            PO[k] = ld2<(NTM & 1) != 0>(pold + o);
        }
    }

    // straight-line form: no instruction moves across this point, i.e. every load above is issued before the first use
    if constexpr ((NTM & 8) != 0) __builtin_amdgcn_sched_barrier(0);

    // raw neighbours
    V2 Pe[R + 2], Ve[R + 1], Uw[R + 2];
#pragma unroll
    for (int k = 0; k < R + 2; k++) Pe[k] = east(P[k]);
#pragma unroll
    for (int k = 0; k < R + 1; k++) Ve[k] = east(Vv[k]);
#pragma unroll
    for (int k = 1; k < R + 2; k++) Uw[k] = west(U[k]);

    // intermediates at the lane's own columns: index k = row jb-1+k
    V2 CU[R + 2], CV[R + 1], Z[R + 1], H[R + 2];
#pragma unroll
    for (int k = 1; k < R + 2; k++) {
        CU[k] = EW(0.5 * (Pe[k].x + P[k].x) * U[k].x, 0.5 * (Pe[k].y + P[k].y) * U[k].y);
        H[k] = EW(P[k].x + 0.25 * (U[k].x * U[k].x + Uw[k].x * Uw[k].x + Vv[k].x * Vv[k].x +
                                   Vv[k - 1].x * Vv[k - 1].x),
                  P[k].y + 0.25 * (U[k].y * U[k].y + Uw[k].y * Uw[k].y + Vv[k].y * Vv[k].y +
                                   Vv[k - 1].y * Vv[k - 1].y));
    }
#pragma unroll
    for (int k = 0; k < R + 1; k++) {
        CV[k] = EW(0.5 * (P[k + 1].x + P[k].x) * Vv[k].x, 0.5 * (P[k + 1].y + P[k].y) * Vv[k].y);
        Z[k] = EW((q.fsdx * (Ve[k].x - Vv[k].x) - q.fsdy * (U[k + 1].x - U[k].x)) /
                      (P[k].x + Pe[k].x + Pe[k + 1].x + P[k + 1].x),
                  (q.fsdx * (Ve[k].y - Vv[k].y) - q.fsdy * (U[k + 1].y - U[k].y)) /
                      (P[k].y + Pe[k].y + Pe[k + 1].y + P[k + 1].y));
    }
    // derived neighbours
    V2 CUw[R + 2], Zw[R + 1], CVe[R + 1], He[R + 1];
#pragma unroll
    for (int k = 1; k < R + 2; k++) CUw[k] = west(CU[k]);
#pragma unroll
    for (int k = 1; k < R + 1; k++) Zw[k] = west(Z[k]);
#pragma unroll
    for (int k = 0; k < R + 1; k++) CVe[k] = east(CV[k]);
#pragma unroll
    for (int k = 1; k < R + 1; k++) He[k] = east(H[k]);

#pragma unroll
    for (int k = 1; k <= R; k++) {
        const int jj = jb - 1 + k;
        constexpr bool STRAIGHT = (NTM & 8) != 0;
        if constexpr (!STRAIGHT) {
            if (jj > je) break;
        }
        V2 un = EW(UO[k - 1].x + q.tdts8 * (Z[k].x + Z[k - 1].x) *
                                           (CVe[k].x + CV[k].x + CV[k - 1].x + CVe[k - 1].x) -
                             q.tdtsdx * (He[k].x - H[k].x),
                         UO[k - 1].y + q.tdts8 * (Z[k].y + Z[k - 1].y) *
                                           (CVe[k].y + CV[k].y + CV[k - 1].y + CVe[k - 1].y) -
                             q.tdtsdx * (He[k].y - H[k].y));
        V2 vn = EW(VO[k - 1].x - q.tdts8 * (Z[k].x + Zw[k].x) *
                                           (CU[k + 1].x + CUw[k + 1].x + CUw[k].x + CU[k].x) -
                             q.tdtsdy * (H[k + 1].x - H[k].x),
                         VO[k - 1].y - q.tdts8 * (Z[k].y + Zw[k].y) *
                                           (CU[k + 1].y + CUw[k + 1].y + CUw[k].y + CU[k].y) -
                             q.tdtsdy * (H[k + 1].y - H[k].y));
        V2 pn = EW(PO[k - 1].x - q.tdtsdx * (CU[k].x - CUw[k].x) - q.tdtsdy * (CV[k].x - CV[k - 1].x),
                         PO[k - 1].y - q.tdtsdx * (CU[k].y - CUw[k].y) - q.tdtsdy * (CV[k].y - CV[k - 1].y));
        const size_t o = (size_t)jj * ld + (size_t)c * 2;
        if constexpr (STRAIGHT) {
            // Every value stored goes through a convergent identity first, so that neither the arithmetic nor the
            // loads of the old time level can be sunk into the (lane-dependent) store branches: all 18 row loads
            // of the wave tile are then in flight together instead of in two dependent groups.
            un = pin_here(un); vn = pin_here(vn); pn = pin_here(pn);
            if (jj > je) continue;
        }
        if (m0 && m1) {
            st2<(NTM & 2) != 0>(unew + o, un);
            st2<(NTM & 2) != 0>(vnew + o, vn);
            st2<(NTM & 2) != 0>(pnew + o, pn);
        } else {
            if (m0) { unew[o] = un.x; vnew[o] = vn.x; pnew[o] = pn.x; }
            if (m1) { unew[o + 1] = un.y; vnew[o + 1] = vn.y; pnew[o + 1] = pn.y; }
        }
        if constexpr (SM) {   // time_smooth of the old level, in place: field_old = field + alpha*(field_new - 2*field + field_old)
            const V2 us = EW(U[k].x + sm.alpha * (un.x - 2.0 * U[k].x + UO[k - 1].x), U[k].y + sm.alpha * (un.y - 2.0 * U[k].y + UO[k - 1].y));
            const V2 vs = EW(Vv[k].x + sm.alpha * (vn.x - 2.0 * Vv[k].x + VO[k - 1].x), Vv[k].y + sm.alpha * (vn.y - 2.0 * Vv[k].y + VO[k - 1].y));
            const V2 ps = EW(P[k].x + sm.alpha * (pn.x - 2.0 * P[k].x + PO[k - 1].x), P[k].y + sm.alpha * (pn.y - 2.0 * P[k].y + PO[k - 1].y));
            if (m0 && m1) {
                st2<(NTM & 2) != 0>(sm.uo + o, us);
                st2<(NTM & 2) != 0>(sm.vo + o, vs);
                st2<(NTM & 2) != 0>(sm.po + o, ps);
            } else {
                if (m0) { sm.uo[o] = us.x; sm.vo[o] = vs.x; sm.po[o] = ps.x; }
                if (m1) { sm.uo[o + 1] = us.y; sm.vo[o + 1] = vs.y; sm.po[o + 1] = ps.y; }
            }
        }
    }
}


template <int R, bool DPP, int NTM, bool SM = false>
__global__ __launch_bounds__(512) void shallow_tile(
    dlesm_sw_params q, int ld, int x0, int x1, int y0, int y1, int cb, int nxw, int hl,
    const double *__restrict__ u, const double *__restrict__ v, const double *__restrict__ p,
    typename OldLevel<SM>::ptr uold, typename OldLevel<SM>::ptr vold, typename OldLevel<SM>::ptr pold,
    double *__restrict__ unew, double *__restrict__ vnew, double *__restrict__ pnew, int stack, SwSmooth sm)
{
    shallow_tile_body<R, DPP, NTM, SM>(q, ld, x0, x1, y0, y1, cb, nxw, hl, u, v, p, uold, vold, pold, unew, vnew, pnew, blockIdx.x, stack, sm);
}

// The distributed shallow-water step in ONE launch on the caller's stream (as jacobi5_tile_framed): the
// first fj.nblocks workgroups compute the one-cell ring of the box (fx0:fx1, fy0:fy1), one cell per thread
// from memory, store it write-through at device scope -- the exchange reads it while this kernel is still
// running -- into the fields and, where a neighbour will receive it, into the aggregated send buffer; the last of them
// publishes `seq` in the flag the side stream's waiter sleeps on.  All other workgroups are the ordinary
// tile sweep over the interior.
template <int R, bool DPP, int NTM, bool SM = false>
__global__ __launch_bounds__(512) void shallow_tile_framed(
    dlesm_sw_params q, int ld, int x0, int x1, int y0, int y1, int cb, int nxw, int hl,
    const double *__restrict__ u, const double *__restrict__ v, const double *__restrict__ p,
    typename OldLevel<SM>::ptr uold, typename OldLevel<SM>::ptr vold, typename OldLevel<SM>::ptr pold,
    double *__restrict__ unew, double *__restrict__ vnew, double *__restrict__ pnew, SwFrameJob fj)
{
    if (blockIdx.x >= (unsigned)fj.nblocks && blockIdx.x < (unsigned)(fj.nblocks + fj.nunb)) {
        // the join inside the launch (peer transport): wait for this step's strips, copy the three fields into the halos
        const int b = blockIdx.x - fj.nblocks, k = b % fj.nun, part = b / fj.nun, parts = (fj.nunb - k + fj.nun - 1) / fj.nun;
        const PeerJob::In m = fj.un[k];
        if (threadIdx.x == 0) {
            const unsigned long long t0 = __builtin_amdgcn_s_memrealtime(), seq = peer_seq_load(fj.seqw, fj.seq);
            while (__hip_atomic_load(m.flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) < seq) {
                __builtin_amdgcn_s_sleep(32);
                if (fj.halo_wait_ticks && __builtin_amdgcn_s_memrealtime() - t0 > fj.halo_wait_ticks) {
                    __hip_atomic_store(fj.timed_out, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                    break;
                }
            }
            if (fj.fenced) handover_acquire<true>();      // (peer_wait_flags' form, dlesm_kernels.hip)
        }
        __syncthreads();
        const long n = (long)m.ni * m.nj;
        double *const dst[3] = {unew, vnew, pnew};
        for (long t = (long)part * blockDim.x + threadIdx.x; t < 3 * n; t += (long)parts * blockDim.x) {
            const int f = (int)(t / n);
            const long e = t - (long)f * n;
            const int jj = (int)(e / m.ni), ii = (int)(e - (long)jj * m.ni);
            dst[f][(size_t)(m.j0 + jj) * ld + (m.i0 + ii)] = __hip_atomic_load(m.src + t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        }
        return;
    }
    if (blockIdx.x >= (unsigned)fj.nblocks) {
        const SwSmooth sm = fj.smooth ? SwSmooth{fj.alpha, const_cast<double *>(uold), const_cast<double *>(vold), const_cast<double *>(pold)}
                                      : SwSmooth{0.0, nullptr, nullptr, nullptr};
        shallow_tile_body<R, DPP, NTM, SM>(q, ld, x0, x1, y0, y1, cb, nxw, hl, u, v, p, uold, vold, pold, unew, vnew, pnew,
                                           blockIdx.x - fj.nblocks - fj.nunb, 1, sm);
        return;
    }
    auto put = [](double *ptr, double val) { __hip_atomic_store(ptr, val, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); };
    long total = frame_cells(fj.fx1 - fj.fx0 + 1, fj.fy1 - fj.fy0 + 1);
    if (fj.diag & 1) total = 0;
    if (fj.diag & 2) total = 2L * (fj.fx1 - fj.fx0 + 1);
    const bool chained = fj.halo_seq != 0;
    if (chained) {
        // time-loop form: the halos of u, v, p (and the send buffers) belong to the previous step's exchange
        // until its completion flag is up -- in steady state long since.  Bounded, as in jacobi5_tile_framed.
        if (threadIdx.x == 0) {
            const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
            while (__hip_atomic_load(fj.halo_flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < fj.halo_seq) {
                __builtin_amdgcn_s_sleep(32);
                if (fj.halo_wait_ticks && __builtin_amdgcn_s_memrealtime() - t0 > fj.halo_wait_ticks) {   // dm_wait_seconds
                    __hip_atomic_store(fj.timed_out, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                    break;
                }
            }
            if (fj.acquire) handover_acquire<false>();    // the consumer form of jacobi5_tile_framed: acquire, waited for, barrier
        }
        __syncthreads();
    }
    for (long t = (long)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (long)fj.nblocks * blockDim.x) {
        int i, j;
        frame_index(t, fj.fx0, fj.fx1, fj.fy0, fj.fy1, i, j);
        const size_t o = (size_t)j * ld + i;
        // chained: the halo operands were unpacked by a kernel that ran beside this one, on whatever XCD
        const SwPoint r = chained ? shallow_values_ne<true>(q, ld, o, u, v, p, uold, vold, pold)
                                  : shallow_values_ne<false>(q, ld, o, u, v, p, uold, vold, pold);
        put(unew + o, r.un);
        put(vnew + o, r.vn);
        put(pnew + o, r.pn);
        // the filtered old level is read by nobody before the next launch: ordinary stores
        if constexpr (SM) smooth_old_level(fj.alpha, o, u, v, p, r, const_cast<double *>(uold), const_cast<double *>(vold), const_cast<double *>(pold));
        if (fj.npeer) {
            // A neighbour's mailbox: system scope (the bytes cross xGMI), 16 bytes per store where two cells are neighbours
            // in the strip too (round 4, as jacobi5_tile_peer's frame).  Consecutive lanes hold consecutive frame cells --
            // along a row, then up a column -- and a strip is contiguous in the mailbox in that same order, so a lane whose
            // slot starts a 16-byte granule takes the upper lane's values by a wave shift (DPP) and stores both; the
            // upper lane then stores nothing; odd ends, corners and granules split between two waves take 8-byte stores.
            const int lane = threadIdx.x & 63;
            const double upn = from_upper<true>(r.un), vpn = from_upper<true>(r.vn), ppn = from_upper<true>(r.pn);
            int i2 = 0, j2 = 0, i0 = 0, j0 = 0;
            const bool has_up = lane < 63 && t + 1 < total, has_lo = lane > 0 && t > 0;
            if (has_up) frame_index(t + 1, fj.fx0, fj.fx1, fj.fy0, fj.fy1, i2, j2);
            if (has_lo) frame_index(t - 1, fj.fx0, fj.fx1, fj.fy0, fj.fy1, i0, j0);
            const double mine[3] = {r.un, r.vn, r.pn}, upper[3] = {upn, vpn, ppn};
            for (int k = 0; k < fj.pk.n; k++) {
                if (!fj.pk.holds(k, i, j)) continue;
                double *b = fj.pk.at(k);
                const long s0 = fj.pk.slot(k, 0, i, j);
                const bool up_next = has_up && fj.pk.holds(k, i2, j2) && fj.pk.slot(k, 0, i2, j2) == s0 + 1;
                const bool lo_prev = has_lo && fj.pk.holds(k, i0, j0) && fj.pk.slot(k, 0, i0, j0) == s0 - 1;
#pragma unroll
                for (int f = 0; f < 3; f++) {
                    double *d = b + fj.pk.slot(k, f, i, j);
                    const bool starts_granule = ((uintptr_t)d & 15) == 0;
                    typedef double sw_pd2 __attribute__((ext_vector_type(2)));
                    if (starts_granule && up_next)
                        *(__attribute__((address_space(1))) volatile sw_pd2 *)d = sw_pd2{mine[f], upper[f]};   // global_store_dwordx4 sc0 sc1
                    else if (starts_granule || !lo_prev)
                        __hip_atomic_store(d, mine[f], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                    // else: the second half of the lower lane's granule -- that lane has stored it
                }
            }
        } else {
            for (int k = 0; k < fj.pk.n; k++)
                if (fj.pk.holds(k, i, j)) {
                    double *b = fj.pk.at(k);
                    put(b + fj.pk.slot(k, 0, i, j), r.un);
                    put(b + fj.pk.slot(k, 1, i, j), r.vn);
                    put(b + fj.pk.slot(k, 2, i, j), r.pn);
                }
        }
    }
    __builtin_amdgcn_s_waitcnt(0);        // this wave's stores have been acknowledged ...
    __syncthreads();                      // ... and those of every wave of the group ...
    if (threadIdx.x == 0) {               // ... before the group is counted as done
        const unsigned done = __hip_atomic_fetch_add(fj.counter, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (done == (unsigned)fj.nblocks - 1) {
            __hip_atomic_store(fj.counter, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (fj.npeer) {       // peer transport: the neighbours' arrival flags, then this plan's sequence words (peer_seq_load)
                const unsigned long long seq = peer_seq_load(fj.seqw, fj.seq);
                if (fj.fenced) handover_release<true>();      // (peer_publish's form, dlesm_kernels.hip)
                for (int k = 0; k < fj.npeer; k++)
                    __hip_atomic_store(fj.peer_flag[k], seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                peer_seq_advance(fj.seqw, seq, fj.timed_out);
            } else
                __hip_atomic_store(fj.flag, fj.seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}

// The SW-offset step in the same wave-tile form: the mirror image of
// shallow_tile -- cu, cv, z look WEST/SOUTH, h looks EAST/NORTH -- with its own expression trees
// (the four-term sums associate differently from the mirrored NE ones, so this is not the NE
// kernel run backwards).  Row index k = row jb-1+k, as above.
// wrap (bit 0: x, bit 1: y): the box is the internal region of periodic fields, and every cell stored on its
// first / last column or row is ALSO stored into the halo cell it is the periodic image of -- the copies of
// init_periodic_bc_halos (field_mod.f90:1394-1464: east halo column <- first internal column, west halo column <-
// last internal column over the internal rows; then north halo row <- first internal row, south halo row <- last
// internal row over the columns widened by the two halo columns, which is what makes the corner halos the doubly
// wrapped cells) without the two extra launches.
template <int R, bool DPP, int NTM, bool SM = false>
__global__ __launch_bounds__(512) void shallow_tile_sw(
    dlesm_sw_params q, int ld, int x0, int x1, int y0, int y1, int cb, int nxw, int hl,
    const double *__restrict__ u, const double *__restrict__ v, const double *__restrict__ p,
    typename OldLevel<SM>::ptr uold, typename OldLevel<SM>::ptr vold, typename OldLevel<SM>::ptr pold,
    double *__restrict__ unew, double *__restrict__ vnew, double *__restrict__ pnew, int wrap, SwSmooth sm)
{
    auto east = [](const V2 &a) { return east_of<DPP>(a); };
    auto west = [](const V2 &a) { return west_of<DPP>(a); };
    const int lane = threadIdx.x & 63;
    const int w = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    const int xw = w % nxw, strip = w / nxw;
    const int jb = y0 + strip * R;
    if (jb > y1) return;
    int je = jb + R - 1;
    if (je > y1) je = y1;
    const int c = cb + xw * (64 - 2 * hl) - hl + lane;             // this lane's chunk (2 columns)
    if (c - lane + hl > x1 / 2) return;                 // idle padding tile
    const int c_ld = ld / 2 - 1;
    const int cl = c < 0 ? 0 : (c > c_ld ? c_ld : c);  // halo / trailing lanes: any valid chunk
    const bool out_lane = lane >= hl && lane < 64 - hl && c <= c_ld;
    const bool m0 = out_lane && 2 * c >= x0 && 2 * c <= x1;
    const bool m1 = out_lane && 2 * c + 1 >= x0 && 2 * c + 1 <= x1;

    const size_t col = (size_t)cl * 2;
    V2 U[R + 2], Vv[R + 2], P[R + 2], UO[R], VO[R], PO[R];
#pragma unroll
    for (int k = 0; k < R + 2; k++) {
        int jj = jb - 1 + k;
        if (jj > je + 1) jj = je + 1;
        const size_t o = (size_t)jj * ld + col;
        U[k] = ld2(u + o);
        Vv[k] = ld2(v + o);
        P[k] = ld2(p + o);
    }
#pragma unroll
    for (int k = 0; k < R; k++) {
        int jj = jb + k;
        if (jj > je) jj = je;
        const size_t o = (size_t)jj * ld + col;
        UO[k] = ld2<(NTM & 1) != 0>(uold + o);
        VO[k] = ld2<(NTM & 1) != 0>(vold + o);
        PO[k] = ld2<(NTM & 1) != 0>(pold + o);
    }

    // raw neighbours
    V2 Pw[R + 2], Vw[R + 2], Ue[R + 1];
#pragma unroll
    for (int k = 0; k < R + 2; k++) Pw[k] = west(P[k]);
#pragma unroll
    for (int k = 1; k < R + 2; k++) Vw[k] = west(Vv[k]);
#pragma unroll
    for (int k = 0; k < R + 1; k++) Ue[k] = east(U[k]);

    // intermediates at the lane's own columns
    V2 CU[R + 1], H[R + 1], CV[R + 2], Z[R + 2];
#pragma unroll
    for (int k = 0; k < R + 1; k++) {   // rows jb-1 .. je: cu(i,j) = 0.5*(p(i,j)+p(i-1,j))*u(i,j); h looks east/north
        CU[k] = EW(0.5 * (P[k].x + Pw[k].x) * U[k].x, 0.5 * (P[k].y + Pw[k].y) * U[k].y);
        H[k] = EW(P[k].x + 0.25 * (Ue[k].x * Ue[k].x + U[k].x * U[k].x + Vv[k + 1].x * Vv[k + 1].x +
                                   Vv[k].x * Vv[k].x),
                  P[k].y + 0.25 * (Ue[k].y * Ue[k].y + U[k].y * U[k].y + Vv[k + 1].y * Vv[k + 1].y +
                                   Vv[k].y * Vv[k].y));
    }
#pragma unroll
    for (int k = 1; k < R + 2; k++) {   // rows jb .. je+1: cv and z look south
        CV[k] = EW(0.5 * (P[k].x + P[k - 1].x) * Vv[k].x, 0.5 * (P[k].y + P[k - 1].y) * Vv[k].y);
        Z[k] = EW((q.fsdx * (Vv[k].x - Vw[k].x) - q.fsdy * (U[k].x - U[k - 1].x)) /
                      (Pw[k - 1].x + P[k - 1].x + P[k].x + Pw[k].x),
                  (q.fsdx * (Vv[k].y - Vw[k].y) - q.fsdy * (U[k].y - U[k - 1].y)) /
                      (Pw[k - 1].y + P[k - 1].y + P[k].y + Pw[k].y));
    }
    // derived neighbours
    V2 CUe[R + 1], Ze[R + 1], CVw[R + 2], Hw[R + 1];
#pragma unroll
    for (int k = 0; k < R + 1; k++) CUe[k] = east(CU[k]);
#pragma unroll
    for (int k = 1; k < R + 1; k++) Ze[k] = east(Z[k]);
#pragma unroll
    for (int k = 1; k < R + 2; k++) CVw[k] = west(CV[k]);
#pragma unroll
    for (int k = 1; k < R + 1; k++) Hw[k] = west(H[k]);

    if constexpr ((NTM & 8) != 0) __builtin_amdgcn_sched_barrier(0);   // (see shallow_tile_body) nothing sinks below the loads
#pragma unroll
    for (int k = 1; k <= R; k++) {
        const int jj = jb - 1 + k;
        constexpr bool STRAIGHT = (NTM & 8) != 0;
        if constexpr (!STRAIGHT) {
            if (jj > je) break;
        }
        // unew = uold + tdts8*(z(i,j+1)+z(i,j))*(cv(i,j+1)+cv(i-1,j+1)+cv(i-1,j)+cv(i,j)) - tdtsdx*(h(i,j)-h(i-1,j))
        V2 un = EW(UO[k - 1].x + q.tdts8 * (Z[k + 1].x + Z[k].x) *
                                           (CV[k + 1].x + CVw[k + 1].x + CVw[k].x + CV[k].x) -
                             q.tdtsdx * (H[k].x - Hw[k].x),
                         UO[k - 1].y + q.tdts8 * (Z[k + 1].y + Z[k].y) *
                                           (CV[k + 1].y + CVw[k + 1].y + CVw[k].y + CV[k].y) -
                             q.tdtsdx * (H[k].y - Hw[k].y));
        // vnew = vold - tdts8*(z(i+1,j)+z(i,j))*(cu(i+1,j)+cu(i,j)+cu(i,j-1)+cu(i+1,j-1)) - tdtsdy*(h(i,j)-h(i,j-1))
        V2 vn = EW(VO[k - 1].x - q.tdts8 * (Ze[k].x + Z[k].x) *
                                           (CUe[k].x + CU[k].x + CU[k - 1].x + CUe[k - 1].x) -
                             q.tdtsdy * (H[k].x - H[k - 1].x),
                         VO[k - 1].y - q.tdts8 * (Ze[k].y + Z[k].y) *
                                           (CUe[k].y + CU[k].y + CU[k - 1].y + CUe[k - 1].y) -
                             q.tdtsdy * (H[k].y - H[k - 1].y));
        // pnew = pold - tdtsdx*(cu(i+1,j)-cu(i,j)) - tdtsdy*(cv(i,j+1)-cv(i,j))
        V2 pn = EW(PO[k - 1].x - q.tdtsdx * (CUe[k].x - CU[k].x) - q.tdtsdy * (CV[k + 1].x - CV[k].x),
                         PO[k - 1].y - q.tdtsdx * (CUe[k].y - CU[k].y) - q.tdtsdy * (CV[k + 1].y - CV[k].y));
        if constexpr (STRAIGHT) {
            un = pin_here(un); vn = pin_here(vn); pn = pin_here(pn);
            if (jj > je) continue;
        }
        // this row, and the halo row(s) it is the periodic image of.  (Scalars, not a small array: an array captured by
        // the lambda below survives until the compiler moves it into LDS, which costs the kernel 2-5 %.)
        const int image_n = ((wrap & 2) && jj == y0) ? y1 + 1 : -1;
        const int image_s = ((wrap & 2) && jj == y1) ? y0 - 1 : -1;
        // one time level (three arrays) into this row and its periodic images
        auto store3 = [&](double *fu, double *fv, double *fp, const V2 &a, const V2 &b, const V2 &d) {
#pragma unroll
            for (int r = 0; r < 3; r++) {
                const int jr = r == 0 ? jj : r == 1 ? image_n : image_s;
                if (jr < 0) continue;
                const size_t row = (size_t)jr * ld, o = row + (size_t)c * 2;
                if (m0 && m1) {
                    st2<(NTM & 2) != 0>(fu + o, a);
                    st2<(NTM & 2) != 0>(fv + o, b);
                    st2<(NTM & 2) != 0>(fp + o, d);
                } else {
                    if (m0) { fu[o] = a.x; fv[o] = b.x; fp[o] = d.x; }
                    if (m1) { fu[o + 1] = a.y; fv[o + 1] = b.y; fp[o + 1] = d.y; }
                }
                if (wrap & 1) {     // the first / last internal column also goes to the opposite halo column
                    const int i0 = 2 * c, i1 = 2 * c + 1;
                    if (m0 && i0 == x0) { fu[row + x1 + 1] = a.x; fv[row + x1 + 1] = b.x; fp[row + x1 + 1] = d.x; }
                    if (m1 && i1 == x0) { fu[row + x1 + 1] = a.y; fv[row + x1 + 1] = b.y; fp[row + x1 + 1] = d.y; }
                    if (m0 && i0 == x1) { fu[row + x0 - 1] = a.x; fv[row + x0 - 1] = b.x; fp[row + x0 - 1] = d.x; }
                    if (m1 && i1 == x1) { fu[row + x0 - 1] = a.y; fv[row + x0 - 1] = b.y; fp[row + x0 - 1] = d.y; }
                }
            }
        };
        store3(unew, vnew, pnew, un, vn, pn);
        if constexpr (SM) {   // time_smooth of the old level, in place (and its periodic images): see SwSmooth
            const V2 us = EW(U[k].x + sm.alpha * (un.x - 2.0 * U[k].x + UO[k - 1].x), U[k].y + sm.alpha * (un.y - 2.0 * U[k].y + UO[k - 1].y));
            const V2 vs = EW(Vv[k].x + sm.alpha * (vn.x - 2.0 * Vv[k].x + VO[k - 1].x), Vv[k].y + sm.alpha * (vn.y - 2.0 * Vv[k].y + VO[k - 1].y));
            const V2 ps = EW(P[k].x + sm.alpha * (pn.x - 2.0 * P[k].x + PO[k - 1].x), P[k].y + sm.alpha * (pn.y - 2.0 * P[k].y + PO[k - 1].y));
            store3(sm.uo, sm.vo, sm.po, us, vs, ps);
        }
    }
}

} // namespace

// Measured launch shapes (dlesm_shallow_autotune_f64), as for the Jacobi sweep: every shape and
// cache policy computes the same bits, so the fastest for a given (leading dimension, box) is
// simply timed once and remembered.
struct SwKey {
    int ld, x0, x1, y0, y1, sw;       // sw: 1 = the SW-offset kernel (its own landscape)
    bool operator<(const SwKey &o) const { return std::tie(ld, x0, x1, y0, y1, sw) < std::tie(o.ld, o.x0, o.x1, o.y0, o.y1, o.sw); }
};
struct SwShape { int tpb, nxw, ntm; };
static std::mutex g_sw_mu;
static std::map<SwKey, SwShape> g_sw_cache;
static SwShape g_sw_override = {0, 0, 0};

// First chunk of the first wave tile of a row: anchored on a 128-byte line of the row, not on the box --
// measured at 8192^2 (round 2): the same sweep over a box that starts one or two columns further east
// (the interior of the distributed step) ran 8 us (1 %) slower when its tiles started at the box.
// Lanes west of x0 are masked.
static inline int sw_first_chunk(int x0) { return (x0 / 2) & ~7; }

static void sw_rule_shape(int ld, int x0, int x1, int hl, int *nxw_out, int *tpb_out)
{
    const int cb = sw_first_chunk(x0), c_last = x1 / 2, out_lanes = 64 - 2 * hl;
    int nxw = (c_last - cb + out_lanes) / out_lanes, tpb = 4;          // output chunks per wave tile
    if (!tuning("j5_autoshape", 1) || tuning("j5_tpb", 0) || nxw < 16) {
        choose_block_shape(&nxw, &tpb);                  // experiments and thin boxes: the shared path
    } else if (hl == 4) {
        // Exhaustive (waves per group, tiles per row) searches with the 56-lane tile at 2048^2 .. 12288^2 (round 4,
        // scripts/shallow_shape_search.py, profiles/r04_shallow_shape_search.txt) show one pattern, the Jacobi sweep's: FOUR waves
        // per group and a row of a QUARTER GROUP SHORT OF OR PAST a multiple of 8 groups -- 31 / 33, 63 / 65, 95 / 97 tiles --
        // first or within 1 % of first at every size, idle padding tiles included (8192^2: 74 tiles padded to 95 = 23.75 groups
        // 0.808 ms, unpadded 0.89; 4096^2: 37 -> 63 tiles; exactly 8k groups per row is the worst shape: 1.11 ms).  So: the
        // smallest such row length that holds the box.
        tpb = 4;
        const int below = (nxw + 1 + 31) / 32 * 32 - 1;  // smallest 32k - 1 >= nxw
        const int above = (nxw - 1 + 31) / 32 * 32 + 1;  // smallest 32k + 1 >= nxw
        nxw = below < above ? below : above;
    } else {
        // The 62-lane tile (rounds 1-3; still the form of odd pitches): an exhaustive search at 8192^2 (67 tiles per row) found 8
        // waves per group JUST ABOVE a multiple of 8 groups best (67 tiles 0.844 ms, 68 0.846, 69 0.852), 4 waves at 23.75 groups
        // equal, 15.75 groups per row 25 % slower.  So: the group size whose 8-group multiple lies closest below the row, no
        // padding when the row is within 3/8 group past it, else padding up to the next multiple (+1 tile when on it exactly).
        double best = 1e9;
        int pad = 0;
        for (int cand : {8, 4, 2}) {
            const int period = 8 * cand, slack = 3 * cand / 8;
            if (nxw < period) continue;
            const int r = nxw % period, p = r <= slack ? 0 : period - r;
            const double cost = (double)p / nxw + (cand == 8 ? 0.0 : cand == 4 ? 0.01 : 0.03);
            if (cost < best) { best = cost; tpb = cand; pad = p; }
        }
        if (best > 0.25) { tpb = 4; pad = 0; }
        nxw += pad;
        if (nxw >= 128 && nxw % (8 * tpb) == 0) nxw += 1;
    }
    *nxw_out = nxw;
    *tpb_out = tpb;
}

// shallow-water step, register-tiled linear sweep; 0-based inclusive box
static void launch_shallow_tile(const dlesm_sw_params &q, int ld, int x0, int x1, int y0, int y1, const SwFields &f, hipStream_t s,
                                bool sw_offset = false, SwFrameJob *fj = nullptr, int wrap = 0,
                                const double *smooth_alpha = nullptr)   // non-null: also uold/vold/pold <- time_smooth, in place
{
    const double *u = f.u, *v = f.v, *p = f.p, *uold = f.uold, *vold = f.vold, *pold = f.pold;   // (as the launches below name them)
    double *unew = f.unew, *vnew = f.vnew, *pnew = f.pnew;
    const int cb = sw_first_chunk(x0);
    const int hl = sw_halo_lanes(ld, f);
    int nxw, tpb, ntm = tuning("sw_nt", sw_nt_default(ld, y0, y1)) & (kLab ? 15 : 3);      // (bits 4, 8: experiments, lab build only)
    SwSmooth sm{0.0, nullptr, nullptr, nullptr};
    if (smooth_alpha) sm = SwSmooth{*smooth_alpha, const_cast<double *>(uold), const_cast<double *>(vold), const_cast<double *>(pold)};
    {
        std::lock_guard<std::mutex> lk(g_sw_mu);
        auto it = g_sw_cache.find(SwKey{ld, x0, x1, y0, y1, (sw_offset ? 1 : 0) | (hl << 1)});
        if (g_sw_override.tpb) { tpb = g_sw_override.tpb; nxw = g_sw_override.nxw; ntm = g_sw_override.ntm; }
        else if (it != g_sw_cache.end() && tuning("j5_use_tuned", 1)) { tpb = it->second.tpb; nxw = it->second.nxw; ntm = it->second.ntm; }
        else sw_rule_shape(ld, x0, x1, hl, &nxw, &tpb);
    }
    {   // whatever chose the row length: it must hold the box
        const int need = (x1 / 2 - cb + (64 - 2 * hl)) / (64 - 2 * hl);
        if (nxw < need) nxw = need;
    }
    if (tpb > 8) tpb = 8;                                // the kernel is bounded to 512 threads
    // the old level updated in place: non-temporal stores want non-temporal loads of it too (the in-place finding of
    // time_smooth, dlesm_shallow_kernels.hip: a store into a line its own load has just left in L2 is the slow case)
    if (sm.uo && (ntm & 2) && tuning("sw_smooth_ntl", 1)) ntm |= 1;
    int R = tuning("sw_tile_rows", 2);
    if ((R != 1 && R != 3) || sm.uo) R = 2;               // (the filtered step exists for two-row tiles)
    const int h = y1 - y0 + 1, strips = (h + R - 1) / R;
    const long tiles = (long)nxw * strips;
    unsigned grid = (unsigned)((tiles + tpb - 1) / tpb);
    const bool dpp = tuning("sw_dpp", 1);
    // experiments (NE offset, R = 2, DPP): sw_stack = vertically adjacent tiles per workgroup; sw_nt bit 2 = the old
    // level requested before u, v, p
    int stack = (!fj && !sw_offset && R == 2 && dpp && !sm.uo) ? tuning("sw_stack", 1) : 1;
    if (stack != 2 && stack != 4) stack = 1;
    if (stack > tpb) stack = 1;
    if (stack > 1) grid = (unsigned)(((nxw + tpb / stack - 1) / (tpb / stack)) * (long)((strips + stack - 1) / stack));
    if ((ntm & 4) && (fj || sw_offset || R != 2 || !dpp)) ntm &= 11;      // old-level-first: NE only
    if ((ntm & 8) && (fj || R != 2 || !dpp)) ntm &= 3;                     // straight-line: both staggerings, R = 2, DPP
    if (fj) {   // NE offset, R = 2, the default wave shifts: the one form the distributed step uses
        fj->smooth = sm.uo ? 1 : 0;
        fj->alpha = sm.alpha;
        const long cells = 2L * (fj->fx1 - fj->fx0 + 1) + 2L * (fj->fy1 - fj->fy0 + 1);
        long nb = ((cells + 64 * tpb - 1) / (64 * tpb) + 7) & ~7L;    // a multiple of 8: tile groups keep their XCD
        fj->nblocks = (int)(nb < 8 ? 8 : nb > 512 ? 512 : nb);
        fj->nunb = fj->nun > 0 ? 16 : 0;                 // join workgroups of the peer transport (a multiple of 8)
        const unsigned g2 = grid + (unsigned)fj->nblocks + (unsigned)fj->nunb;
#define DLESM_SWF(NN, SS) hipLaunchKernelGGL((shallow_tile_framed<2, true, NN, SS>), dim3(g2), dim3(64 * tpb), 0, s, q, ld, x0, x1, y0, y1, cb, nxw, hl, u, v, p, uold, vold, pold, unew, vnew, pnew, *fj)
        if (sm.uo) {
            switch (ntm & 3) {
            case 1: DLESM_SWF(1, true); break;
            case 2: DLESM_SWF(2, true); break;
            case 3: DLESM_SWF(3, true); break;
            default: DLESM_SWF(0, true); break;
            }
        } else {
            switch (ntm & 3) {
            case 1: DLESM_SWF(1, false); break;
            case 2: DLESM_SWF(2, false); break;
            case 3: DLESM_SWF(3, false); break;
            default: DLESM_SWF(0, false); break;
            }
        }
#undef DLESM_SWF
        return;
    }
    if (sm.uo) {   // the filter folded in: the R = 2, DPP form with the plain / non-temporal policies
#define DLESM_SWS(NN)                                                                                          \
    do {                                                                                                       \
        if (sw_offset)                                                                                         \
            hipLaunchKernelGGL((shallow_tile_sw<2, true, NN, true>), dim3(grid), dim3(64 * tpb), 0, s, q, ld, x0, x1, y0, \
                               y1, cb, nxw, hl, u, v, p, uold, vold, pold, unew, vnew, pnew, wrap, sm);            \
        else                                                                                                   \
            hipLaunchKernelGGL((shallow_tile<2, true, NN, true>), dim3(grid), dim3(64 * tpb), 0, s, q, ld, x0, x1, y0, \
                               y1, cb, nxw, hl, u, v, p, uold, vold, pold, unew, vnew, pnew, 1, sm);               \
    } while (0)
        switch ((ntm == 10 || ntm == 11) ? ntm : (ntm & 3)) {
        case 1: DLESM_SWS(1); break;
        case 2: DLESM_SWS(2); break;
        case 3: DLESM_SWS(3); break;
#ifdef DLESM_LAB
        case 10: DLESM_SWS(10); break;
        case 11: DLESM_SWS(11); break;
#endif
        default: DLESM_SWS(0); break;
        }
#undef DLESM_SWS
        return;
    }
#define DLESM_SW3(RR, DD, NN)                                                                                  \
    do {                                                                                                       \
        if (sw_offset)                                                                                         \
            hipLaunchKernelGGL((shallow_tile_sw<RR, DD, NN>), dim3(grid), dim3(64 * tpb), 0, s, q, ld, x0, x1, y0, \
                               y1, cb, nxw, hl, u, v, p, uold, vold, pold, unew, vnew, pnew, wrap, sm);            \
        else                                                                                                   \
            hipLaunchKernelGGL((shallow_tile<RR, DD, NN>), dim3(grid), dim3(64 * tpb), 0, s, q, ld, x0, x1, y0, \
                               y1, cb, nxw, hl, u, v, p, uold, vold, pold, unew, vnew, pnew, stack, sm);           \
    } while (0)
#define DLESM_SW2(RR, DD)                                                                                      \
    do {                                                                                                       \
        switch (ntm) {                                                                                         \
        case 1: DLESM_SW3(RR, DD, 1); break;                                                                   \
        case 2: DLESM_SW3(RR, DD, 2); break;                                                                   \
        case 3: DLESM_SW3(RR, DD, 3); break;                                                                   \
        default: DLESM_SW3(RR, DD, 0); break;                                                                  \
        }                                                                                                      \
    } while (0)
#ifndef DLESM_LAB
    // the product's form: two-row tiles, DPP wave shifts, the four cache policies the planning call chooses from;
    // one- and three-row tiles, shuffles through LDS, stacked tiles, the straight-line and old-level-first forms were
    // comparison points and live in libdlesm_hip_lab.so
    (void)dpp;
    DLESM_SW2(2, true);
#else
#define DLESM_SW(RR)                                                                                           \
    do {                                                                                                       \
        if (dpp) DLESM_SW2(RR, true);                                                                          \
        else DLESM_SW2(RR, false);                                                                             \
    } while (0)
    if (ntm & 12) {     // only reached for the NE offset, R = 2, DPP
        switch (ntm) {
        case 5: DLESM_SW3(2, true, 5); break;
        case 6: DLESM_SW3(2, true, 6); break;
        case 7: DLESM_SW3(2, true, 7); break;
        case 8: DLESM_SW3(2, true, 8); break;
        case 9: DLESM_SW3(2, true, 9); break;
        case 10: DLESM_SW3(2, true, 10); break;
        case 11: DLESM_SW3(2, true, 11); break;
        case 14: DLESM_SW3(2, true, 14); break;
        case 15: DLESM_SW3(2, true, 15); break;
        default: DLESM_SW3(2, true, 4); break;
        }
    }
    else if (R == 1) DLESM_SW(1);
    else if (R == 3) DLESM_SW(3);
    else DLESM_SW(2);
#undef DLESM_SW
#endif // DLESM_LAB
#undef DLESM_SW2
#undef DLESM_SW3
}

// ===========================================================================
// Shallow-water u/v/h update, NE staggering, all intermediates (cu, cv, z, h)
// recomputed in registers from the 3x3 neighbourhood of u, v, p: 6 fields read,
// 3 written = 72 B/cell of algorithmic traffic.
// First, direct form: neighbours come from L1/L2.
// ===========================================================================
__global__ __launch_bounds__(256) void shallow_step_direct(
    dlesm_sw_params q, int ld, int x0, int x1, int y0, int y1, const double *__restrict__ u,
    const double *__restrict__ v, const double *__restrict__ p, const double *__restrict__ uold,
    const double *__restrict__ vold, const double *__restrict__ pold, double *__restrict__ unew,
    double *__restrict__ vnew, double *__restrict__ pnew)
{
    const int i = x0 + blockIdx.x * blockDim.x + threadIdx.x;
    if (i > x1) return;
    for (int j = y0 + blockIdx.y; j <= y1; j += gridDim.y)
        shallow_point_ne(q, ld, (size_t)j * ld + i, u, v, p, uold, vold, pold, unew, vnew, pnew);
}

// the same for boxes a few columns wide and many rows tall (frame columns): lanes run along j
__global__ __launch_bounds__(256) void shallow_step_direct_cols(
    dlesm_sw_params q, int ld, int x0, int x1, int y0, int y1, const double *__restrict__ u,
    const double *__restrict__ v, const double *__restrict__ p, const double *__restrict__ uold,
    const double *__restrict__ vold, const double *__restrict__ pold, double *__restrict__ unew,
    double *__restrict__ vnew, double *__restrict__ pnew)
{
    const int j = y0 + blockIdx.x * blockDim.x + threadIdx.x;
    if (j > y1) return;
    for (int i = x0; i <= x1; i++)
        shallow_point_ne(q, ld, (size_t)j * ld + i, u, v, p, uold, vold, pold, unew, vnew, pnew);
}

// the one-cell frame of the box (the cells a neighbour needs first in the distributed step): one cell
// per thread, all four sides in ONE launch; cells a neighbour will receive also go into the aggregated
// send buffer of the three new fields (FramePack3)
__global__ __launch_bounds__(256) void shallow_frame_k(
    dlesm_sw_params q, int ld, int x0, int x1, int y0, int y1, const double *__restrict__ u,
    const double *__restrict__ v, const double *__restrict__ p, const double *uold,
    const double *vold, const double *pold, double *__restrict__ unew,
    double *__restrict__ vnew, double *__restrict__ pnew, FramePack3 pk, int smooth, double alpha)
{
    const long total = frame_cells(x1 - x0 + 1, y1 - y0 + 1);
    for (long t = (long)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (long)gridDim.x * blockDim.x) {
        int i, j;
        frame_index(t, x0, x1, y0, y1, i, j);
        const size_t o = (size_t)j * ld + i;
        const SwPoint r = shallow_values_ne(q, ld, o, u, v, p, uold, vold, pold);
        unew[o] = r.un;
        vnew[o] = r.vn;
        pnew[o] = r.pn;
        if (smooth) smooth_old_level(alpha, o, u, v, p, r, const_cast<double *>(uold), const_cast<double *>(vold), const_cast<double *>(pold));
        for (int k = 0; k < pk.n; k++)
            if (pk.holds(k, i, j)) {
                double *b = pk.at(k);          // (a neighbour's mailbox with the peer transport: uncached memory, the
                b[pk.slot(k, 0, i, j)] = r.un; //  stores have left by the end of the kernel; its flags are raised by a
                b[pk.slot(k, 1, i, j)] = r.vn; //  launch behind this one)
                b[pk.slot(k, 2, i, j)] = r.pn;
            }
    }
}

int launch_shallow_frame(const dlesm_sw_params &q, int ld, int ny, int xstart, int xstop, int ystart, int ystop,
                         const SwFields &f, const FramePack3 *pack, hipStream_t s, const double *smooth_alpha)
{
    if (xstop < xstart || ystop < ystart) return DLESM_OK;
    if (int rc = check_box("shallow frame", ld, ny, xstart, xstop, ystart, ystop, 1)) return rc;
    const long cells = 2L * (xstop - xstart + 1) + 2L * (ystop - ystart + 1);
    int blocks = (int)((cells + 255) / 256);
    if (blocks > 2048) blocks = 2048;
    FramePack3 pk{};
    if (pack) pk = *pack;
    hipLaunchKernelGGL(shallow_frame_k, dim3(blocks), dim3(256), 0, s, q, ld, xstart - 1, xstop - 1, ystart - 1,
                       ystop - 1, f.u, f.v, f.p, f.uold, f.vold, f.pold, f.unew, f.vnew, f.pnew, pk, smooth_alpha ? 1 : 0,
                       smooth_alpha ? *smooth_alpha : 0.0);
    DLESM_HIP_TRY(hipGetLastError());
    return DLESM_OK;
}

} // namespace dlesm

int dlesm::launch_shallow_framed(const dlesm_sw_params &q, int ld, int ny, int xstart, int xstop, int ystart, int ystop,
                                 const SwFields &f, SwFrameJob job, hipStream_t s, bool *fused, const double *smooth_alpha)
{
    *fused = false;
    if (xstop - xstart < 2 || ystop - ystart < 2) return DLESM_OK;          // no interior: two-launch path
    if (int rc = check_box("dlesm_shallow_step_dm", ld, ny, xstart, xstop, ystart, ystop, 1)) return rc;
    // (the interior's east column: the frame takes column xstop - 1)
    if (!sw_lanes16_fit(ld, xstop - 2, f) || tuning("sw_kernel", 0) != 0 || tuning("sw_tile_rows", 2) != 2 || !tuning("sw_dpp", 1)) return DLESM_OK;
    job.fx0 = xstart - 1, job.fx1 = xstop - 1, job.fy0 = ystart - 1, job.fy1 = ystop - 1;
    job.diag = tuning("sw_dm_diag", 0);
    launch_shallow_tile(q, ld, xstart, xstop - 2, ystart, ystop - 2, f, s, false, &job, 0, smooth_alpha);
    DLESM_HIP_TRY(hipGetLastError());
    *fused = true;
    return DLESM_OK;
}

using namespace dlesm;

extern "C" int dlesm_shallow_step_f64(const dlesm_sw_params *q, int ld, int ny, int xstart, int xstop,
                                      int ystart, int ystop, const double *u, const double *v,
                                      const double *p, const double *uold, const double *vold,
                                      const double *pold, double *unew, double *vnew, double *pnew,
                                      void *stream)
{
    if (int rc = ensure_device()) return rc;
    DLESM_REQUIRE(q && u && v && p && uold && vold && pold && unew && vnew && pnew, "null pointer");
    if (xstop < xstart || ystop < ystart) return DLESM_OK;
    if (int rc = check_box("dlesm_shallow_step_f64", ld, ny, xstart, xstop, ystart, ystop, 1)) return rc;
    DLESM_REQUIRE(unew != u && unew != v && unew != p && vnew != u && vnew != v && vnew != p &&
                      pnew != u && pnew != v && pnew != p,
                  "shallow step: outputs alias the 3x3-read inputs");
    const int nx = xstop - xstart + 1, nyb = ystop - ystart + 1;
    const SwFields f{u, v, p, uold, vold, pold, unew, vnew, pnew};
    // sw_kernel: 0 (default) = register-tiled sweep of dlesm_shallow.hip, 73.7 % of HBM peak at
    // 8192^2; 1 = direct form, 62 % (scripts/shallow_probe.py, profiles/r01_shallow_*.txt)
    // boxes a few columns wide (the west/east frame columns of the distributed step): a wave tile would load
    // 128 columns x 4 rows of three arrays for two useful cells -- one cell per thread moves 6 x less
    const bool thin = nx <= SW_THIN_BOX && nyb > 8;
    if (sw_lanes16_fit(ld, xstop - 1, f) && tuning("sw_kernel", 0) == 0 && !thin) {
        launch_shallow_tile(*q, ld, xstart - 1, xstop - 1, ystart - 1, ystop - 1, f, (hipStream_t)stream);
        DLESM_HIP_TRY(hipGetLastError());
        return DLESM_OK;
    }
    // odd leading dimension / thin boxes: direct form, neighbours through L1/L2
    if (thin)
        hipLaunchKernelGGL(shallow_step_direct_cols, dim3((nyb + 255) / 256), dim3(256), 0, (hipStream_t)stream, *q, ld,
                           xstart - 1, xstop - 1, ystart - 1, ystop - 1, u, v, p, uold, vold, pold, unew, vnew, pnew);
    else
        hipLaunchKernelGGL(shallow_step_direct, dim3((nx + 255) / 256, nyb > 4096 ? 4096 : nyb), dim3(256), 0,
                           (hipStream_t)stream, *q, ld, xstart - 1, xstop - 1, ystart - 1, ystop - 1, u, v, p, uold,
                           vold, pold, unew, vnew, pnew);
    DLESM_HIP_TRY(hipGetLastError());
    return DLESM_OK;
}

// SW staggering, one cell per thread, neighbours through L1/L2: the
// configuration is serial-only in the reference (periodic boundaries), small next to the NE step.
// Expression trees exactly as specified (oracle: compute_*_sw_code).
__global__ __launch_bounds__(256) void shallow_step_sw_direct(
    dlesm_sw_params q, int ld, int x0, int x1, int y0, int y1, const double *__restrict__ u,
    const double *__restrict__ v, const double *__restrict__ p, const double *__restrict__ uold,
    const double *__restrict__ vold, const double *__restrict__ pold, double *__restrict__ unew,
    double *__restrict__ vnew, double *__restrict__ pnew)
{
    const int i = x0 + blockIdx.x * blockDim.x + threadIdx.x;
    if (i > x1) return;
    for (int j = y0 + blockIdx.y; j <= y1; j += gridDim.y) {
        const size_t o = (size_t)j * ld + i;
#define U_(di, dj) u[o + (di) + (long)(dj) * ld]
#define V_(di, dj) v[o + (di) + (long)(dj) * ld]
#define P_(di, dj) p[o + (di) + (long)(dj) * ld]
#define CU(di, dj) (0.5 * (P_(di, dj) + P_((di)-1, dj)) * U_(di, dj))
#define CV(di, dj) (0.5 * (P_(di, dj) + P_(di, (dj)-1)) * V_(di, dj))
#define Z(di, dj)                                                                                   \
    ((q.fsdx * (V_(di, dj) - V_((di)-1, dj)) - q.fsdy * (U_(di, dj) - U_(di, (dj)-1))) /             \
     (P_((di)-1, (dj)-1) + P_(di, (dj)-1) + P_(di, dj) + P_((di)-1, dj)))
#define H(di, dj)                                                                                   \
    (P_(di, dj) + 0.25 * (U_((di) + 1, dj) * U_((di) + 1, dj) + U_(di, dj) * U_(di, dj) +            \
                          V_(di, (dj) + 1) * V_(di, (dj) + 1) + V_(di, dj) * V_(di, dj)))
        const double z00 = Z(0, 0), z0p = Z(0, 1), zp0 = Z(1, 0);
        const double h00 = H(0, 0), hm0 = H(-1, 0), h0m = H(0, -1);
        const double cu00 = CU(0, 0), cup0 = CU(1, 0), cu0m = CU(0, -1), cupm = CU(1, -1);
        const double cv00 = CV(0, 0), cv0p = CV(0, 1), cvmp = CV(-1, 1), cvm0 = CV(-1, 0);
        unew[o] = uold[o] + q.tdts8 * (z0p + z00) * (cv0p + cvmp + cvm0 + cv00) - q.tdtsdx * (h00 - hm0);
        vnew[o] = vold[o] - q.tdts8 * (zp0 + z00) * (cup0 + cu00 + cu0m + cupm) - q.tdtsdy * (h00 - h0m);
        pnew[o] = pold[o] - q.tdtsdx * (cup0 - cu00) - q.tdtsdy * (cv0p - cv00);
#undef U_
#undef V_
#undef P_
#undef CU
#undef CV
#undef Z
#undef H
    }
}

extern "C" int dlesm_shallow_step_sw_f64(const dlesm_sw_params *q, int ld, int ny, int xstart, int xstop,
                                         int ystart, int ystop, const double *u, const double *v,
                                         const double *p, const double *uold, const double *vold,
                                         const double *pold, double *unew, double *vnew, double *pnew,
                                         void *stream)
{
    if (int rc = ensure_device()) return rc;
    DLESM_REQUIRE(q && u && v && p && uold && vold && pold && unew && vnew && pnew, "null pointer");
    if (xstop < xstart || ystop < ystart) return DLESM_OK;
    if (int rc = check_box("dlesm_shallow_step_sw_f64", ld, ny, xstart, xstop, ystart, ystop, 1)) return rc;
    DLESM_REQUIRE(unew != u && unew != v && unew != p && vnew != u && vnew != v && vnew != p &&
                      pnew != u && pnew != v && pnew != p,
                  "shallow step: outputs alias the 3x3-read inputs");
    const int nx = xstop - xstart + 1, h = ystop - ystart + 1;
    const SwFields f{u, v, p, uold, vold, pold, unew, vnew, pnew};
    // 16-byte lanes under the same conditions as the NE step (dlesm_shallow_step_f64)
    if (sw_lanes16_fit(ld, xstop - 1, f) && tuning("sw_kernel", 0) == 0) {
        launch_shallow_tile(*q, ld, xstart - 1, xstop - 1, ystart - 1, ystop - 1, f, (hipStream_t)stream, true);
        DLESM_HIP_TRY(hipGetLastError());
        return DLESM_OK;
    }
    hipLaunchKernelGGL(shallow_step_sw_direct, dim3((nx + 255) / 256, h > 4096 ? 4096 : h), dim3(256), 0,
                       (hipStream_t)stream, *q, ld, xstart - 1, xstop - 1, ystart - 1, ystop - 1, u, v, p, uold, vold,
                       pold, unew, vnew, pnew);
    DLESM_HIP_TRY(hipGetLastError());
    return DLESM_OK;
}

// The SW-offset step over the internal region of periodic fields WITH the periodic copies of the new level inside
// the launch (shallow_tile_sw's `wrap`): what dlesm_shallow_step_sw_f64 + dlesm_periodic_halos_apply_multi_f64 leave
// behind, in one launch instead of three.  Arrays that do not qualify for the wave-tile kernel take those three.
extern "C" int dlesm_shallow_step_sw_periodic_f64(const dlesm_sw_params *q, int ld, int ny, const dlesm_region *internal,
                                                  int bc_x, int bc_y, const double *u, const double *v, const double *p,
                                                  const double *uold, const double *vold, const double *pold, double *unew,
                                                  double *vnew, double *pnew, void *stream)
{
    if (int rc = ensure_device()) return rc;
    DLESM_REQUIRE(q && internal && u && v && p && uold && vold && pold && unew && vnew && pnew, "null pointer");
    const int xstart = internal->xstart, xstop = internal->xstop, ystart = internal->ystart, ystop = internal->ystop;
    if (xstop < xstart || ystop < ystart) return DLESM_OK;
    if (int rc = check_box("dlesm_shallow_step_sw_periodic_f64", ld, ny, xstart, xstop, ystart, ystop, 1)) return rc;
    DLESM_REQUIRE(unew != u && unew != v && unew != p && vnew != u && vnew != v && vnew != p &&
                      pnew != u && pnew != v && pnew != p && unew != vnew && unew != pnew && vnew != pnew,
                  "shallow step: outputs alias the 3x3-read inputs or each other");
    const int wrap = (bc_x == DLESM_BC_PERIODIC ? 1 : 0) | (bc_y == DLESM_BC_PERIODIC ? 2 : 0);
    const SwFields f{u, v, p, uold, vold, pold, unew, vnew, pnew};
    if (sw_lanes16_fit(ld, xstop - 1, f) && tuning("sw_kernel", 0) == 0 && tuning("sw_wrap_fused", 1)) {
        launch_shallow_tile(*q, ld, xstart - 1, xstop - 1, ystart - 1, ystop - 1, f, (hipStream_t)stream, true, nullptr, wrap);
        DLESM_HIP_TRY(hipGetLastError());
        return DLESM_OK;
    }
    if (int rc = dlesm_shallow_step_sw_f64(q, ld, ny, xstart, xstop, ystart, ystop, u, v, p, uold, vold, pold, unew, vnew,
                                           pnew, stream))
        return rc;
    if (!wrap) return DLESM_OK;
    double *fields[3] = {unew, vnew, pnew};
    return dlesm_periodic_halos_apply_multi_f64(fields, 3, ld, ny, internal, bc_x, bc_y, stream);
}

// ---- the step WITH the Asselin filter of the old level (time_smooth) folded in: one launch = one whole time step of
// the GOcean leapfrog, 96 B/cell (six arrays read, six written) instead of 72 + 3 x 32 = 168 for step + three filters.
static int nine_distinct(const char *who, const SwFields &f)
{
    const double *a[9] = {f.u, f.v, f.p, f.uold, f.vold, f.pold, f.unew, f.vnew, f.pnew};
    for (int i = 0; i < 9; i++)
        for (int j = i + 1; j < 9; j++)
            if (a[i] == a[j]) return fail(DLESM_EINVAL, "%s: the nine fields must be nine different arrays", who);
    return DLESM_OK;
}

extern "C" int dlesm_shallow_step_smooth_f64(const dlesm_sw_params *q, double alpha, int ld, int ny, int xstart, int xstop,
                                             int ystart, int ystop, const double *u, const double *v, const double *p,
                                             double *uold, double *vold, double *pold, double *unew, double *vnew,
                                             double *pnew, void *stream)
{
    if (int rc = ensure_device()) return rc;
    DLESM_REQUIRE(q && u && v && p && uold && vold && pold && unew && vnew && pnew, "null pointer");
    if (xstop < xstart || ystop < ystart) return DLESM_OK;
    if (int rc = check_box("dlesm_shallow_step_smooth_f64", ld, ny, xstart, xstop, ystart, ystop, 1)) return rc;
    const SwFields f{u, v, p, uold, vold, pold, unew, vnew, pnew};
    if (int rc = nine_distinct("dlesm_shallow_step_smooth_f64", f)) return rc;
    const int nx = xstop - xstart + 1, nyb = ystop - ystart + 1;
    const bool thin = nx <= SW_THIN_BOX && nyb > 8;
    if (sw_lanes16_fit(ld, xstop - 1, f) && tuning("sw_kernel", 0) == 0 && !thin && tuning("sw_smooth_fused", 1)) {
        launch_shallow_tile(*q, ld, xstart - 1, xstop - 1, ystart - 1, ystop - 1, f, (hipStream_t)stream, false, nullptr, 0, &alpha);
        DLESM_HIP_TRY(hipGetLastError());
        return DLESM_OK;
    }
    // the definition: the step, then time_smooth of each prognostic field
    if (int rc = dlesm_shallow_step_f64(q, ld, ny, xstart, xstop, ystart, ystop, u, v, p, uold, vold, pold, unew, vnew, pnew, stream))
        return rc;
    if (int rc = dlesm_time_smooth_f64(ld, ny, xstart, xstop, ystart, ystop, alpha, u, unew, uold, stream)) return rc;
    if (int rc = dlesm_time_smooth_f64(ld, ny, xstart, xstop, ystart, ystop, alpha, v, vnew, vold, stream)) return rc;
    return dlesm_time_smooth_f64(ld, ny, xstart, xstop, ystart, ystop, alpha, p, pnew, pold, stream);
}

int dlesm::sw_step_box(const dlesm_sw_params *q, const double *smooth_alpha, int ld, int ny, int xs, int xe, int ys, int ye,
                       const SwFields &f, hipStream_t s)
{
    if (smooth_alpha)
        return dlesm_shallow_step_smooth_f64(q, *smooth_alpha, ld, ny, xs, xe, ys, ye, f.u, f.v, f.p, const_cast<double *>(f.uold),
                                             const_cast<double *>(f.vold), const_cast<double *>(f.pold), f.unew, f.vnew, f.pnew, s);
    return dlesm_shallow_step_f64(q, ld, ny, xs, xe, ys, ye, f.u, f.v, f.p, f.uold, f.vold, f.pold, f.unew, f.vnew, f.pnew, s);
}

extern "C" int dlesm_shallow_step_sw_smooth_periodic_f64(const dlesm_sw_params *q, double alpha, int ld, int ny,
                                                         const dlesm_region *internal, int bc_x, int bc_y, const double *u,
                                                         const double *v, const double *p, double *uold, double *vold,
                                                         double *pold, double *unew, double *vnew, double *pnew, void *stream)
{
    if (int rc = ensure_device()) return rc;
    DLESM_REQUIRE(q && internal && u && v && p && uold && vold && pold && unew && vnew && pnew, "null pointer");
    const int xstart = internal->xstart, xstop = internal->xstop, ystart = internal->ystart, ystop = internal->ystop;
    if (xstop < xstart || ystop < ystart) return DLESM_OK;
    if (int rc = check_box("dlesm_shallow_step_sw_smooth_periodic_f64", ld, ny, xstart, xstop, ystart, ystop, 1)) return rc;
    const SwFields f{u, v, p, uold, vold, pold, unew, vnew, pnew};
    if (int rc = nine_distinct("dlesm_shallow_step_sw_smooth_periodic_f64", f)) return rc;
    const int wrap = (bc_x == DLESM_BC_PERIODIC ? 1 : 0) | (bc_y == DLESM_BC_PERIODIC ? 2 : 0);
    if (sw_lanes16_fit(ld, xstop - 1, f) && tuning("sw_kernel", 0) == 0 && tuning("sw_wrap_fused", 1) && tuning("sw_smooth_fused", 1)) {
        launch_shallow_tile(*q, ld, xstart - 1, xstop - 1, ystart - 1, ystop - 1, f, (hipStream_t)stream, true, nullptr, wrap, &alpha);
        DLESM_HIP_TRY(hipGetLastError());
        return DLESM_OK;
    }
    if (int rc = dlesm_shallow_step_sw_f64(q, ld, ny, xstart, xstop, ystart, ystop, u, v, p, uold, vold, pold, unew, vnew, pnew, stream))
        return rc;
    if (int rc = dlesm_time_smooth_f64(ld, ny, xstart, xstop, ystart, ystop, alpha, u, unew, uold, stream)) return rc;
    if (int rc = dlesm_time_smooth_f64(ld, ny, xstart, xstop, ystart, ystop, alpha, v, vnew, vold, stream)) return rc;
    if (int rc = dlesm_time_smooth_f64(ld, ny, xstart, xstop, ystart, ystop, alpha, p, pnew, pold, stream)) return rc;
    if (!wrap) return DLESM_OK;
    double *fields[6] = {unew, vnew, pnew, uold, vold, pold};
    return dlesm_periodic_halos_apply_multi_f64(fields, 6, ld, ny, internal, bc_x, bc_y, stream);
}

// Up to 16 fields x 2 independent patch copies in one launch: grid.y = field * 2 + copy.
struct HaloPair { int sx[2], sy[2], dx[2], dy[2], nx[2], ny[2]; };
struct FieldList { double *f[16]; };
__global__ void periodic_pair_k(FieldList fl, int ld, HaloPair h)
{
    double *f = fl.f[blockIdx.y >> 1];
    const int c = blockIdx.y & 1;
    const long n = (long)h.nx[c] * h.ny[c];
    for (long t = (long)blockIdx.x * blockDim.x + threadIdx.x; t < n; t += (long)gridDim.x * blockDim.x) {
        const int j = (int)(t / h.nx[c]), i = (int)(t % h.nx[c]);
        f[(size_t)(h.dy[c] + j) * ld + h.dx[c] + i] = f[(size_t)(h.sy[c] + j) * ld + h.sx[c] + i];
    }
}

// The periodic copies of `nfields` fields of one shape: the x pair of every field in one launch, then
// the y pair of every field in a second one (the y copies carry the corners the x copies made, so
// the two phases stay ordered; the two copies of a phase never overlap).
extern "C" int dlesm_periodic_halos_apply_multi_f64(double *const *fields, int nfields, int ld, int ny,
                                                    const dlesm_region *internal, int bc_x, int bc_y, void *stream)
{
    DLESM_REQUIRE(fields != nullptr && internal != nullptr && nfields >= 1 && nfields <= 16, "bad arguments");
    if (int rc = ensure_device()) return rc;
    FieldList fl{};
    for (int k = 0; k < nfields; k++) {
        DLESM_REQUIRE(fields[k] != nullptr, "null field %d", k);
        fl.f[k] = fields[k];
    }
    dlesm_region src[4], dst[4];
    int n = 0;
    if (int rc = dlesm_periodic_halos(internal, bc_x, bc_y, src, dst, &n)) return rc;
    for (int k = 0; k < n; k++)
        DLESM_REQUIRE(src[k].xstart >= 1 && src[k].ystart >= 1 && dst[k].xstart >= 1 && dst[k].ystart >= 1 &&
                          src[k].xstop <= ld && dst[k].xstop <= ld && src[k].ystop <= ny && dst[k].ystop <= ny,
                      "periodic halo %d lies outside the %dx%d field", k, ld, ny);
    for (int k0 = 0; k0 < n; k0 += 2) {
        HaloPair h{};
        long widest = 0;
        for (int c = 0; c < 2; c++) {
            h.sx[c] = src[k0 + c].xstart - 1; h.sy[c] = src[k0 + c].ystart - 1;
            h.dx[c] = dst[k0 + c].xstart - 1; h.dy[c] = dst[k0 + c].ystart - 1;
            h.nx[c] = src[k0 + c].nx;         h.ny[c] = src[k0 + c].ny;
            if ((long)h.nx[c] * h.ny[c] > widest) widest = (long)h.nx[c] * h.ny[c];
        }
        if (widest <= 0) continue;
        long gx = (widest + 255) / 256;
        if (gx > 256) gx = 256;
        hipLaunchKernelGGL(periodic_pair_k, dim3((unsigned)gx, (unsigned)(2 * nfields)), dim3(256), 0,
                           (hipStream_t)stream, fl, ld, h);
    }
    DLESM_HIP_TRY(hipGetLastError());
    return DLESM_OK;
}

extern "C" int dlesm_periodic_halos_apply_f64(double *field, int ld, int ny, const dlesm_region *internal,
                                              int bc_x, int bc_y, void *stream)
{
    DLESM_REQUIRE(field != nullptr, "null pointer");
    double *one[1] = {field};
    return dlesm_periodic_halos_apply_multi_f64(one, 1, ld, ny, internal, bc_x, bc_y, stream);
}

static int shallow_autotune(bool sw_offset, const dlesm_sw_params *q, int ld, int ny, int xstart, int xstop, int ystart, int ystop,
                            const SwFields &f, void *stream)
{
    // the step itself validates the arguments, warms the clocks, and tells whether the tile kernel applies
    if (int rc = (sw_offset ? dlesm_shallow_step_sw_f64 : dlesm_shallow_step_f64)(q, ld, ny, xstart, xstop, ystart, ystop, f.u, f.v, f.p,
                                                                                  f.uold, f.vold, f.pold, f.unew, f.vnew, f.pnew, stream))
        return rc;
    // arrays the step sent to the one-cell-per-thread form have no shapes to choose from
    if (!sw_lanes16_fit(ld, xstop - 1, f)) return DLESM_OK;
    if (xstop < xstart || ystop < ystart || tuning("sw_kernel", 0) != 0) return DLESM_OK;
    const int x0 = xstart - 1, x1 = xstop - 1, y0 = ystart - 1, y1 = ystop - 1;
    const int hl = sw_halo_lanes(ld, f);
    const int nxw0 = (x1 / 2 - sw_first_chunk(x0) + (64 - 2 * hl)) / (64 - 2 * hl);
    if (nxw0 < 16 || tuning("sw_tile_rows", 2) != 2) return DLESM_OK;      // thin boxes: nothing to choose
    hipStream_t s = (hipStream_t)stream;
    std::vector<SwShape> cand;
    auto add = [&](int tpb, int t, int ntm) {
        for (const SwShape &c : cand)
            if (c.tpb == tpb && c.nxw == t && c.ntm == ntm) return;
        cand.push_back(SwShape{tpb, t, ntm});
    };
    int rn, rt;
    sw_rule_shape(ld, x0, x1, hl, &rn, &rt);
    if (rt > 8) rt = 8;
    const int nt0 = tuning("sw_nt", sw_nt_default(ld, y0, y1)) & 3;
    add(rt, rn, nt0);                                                      // the rule's own choice first
    for (int tpb : {8, 4}) {
        add(tpb, nxw0, nt0);
        const int period = 8 * tpb, dmax = tpb == 8 ? 3 : 1;
        for (int k = 0; k < 2; k++) {
            const int base = (nxw0 / period + k) * period;
            for (int d = 0; d <= dmax; d++) {
                if (base - d >= nxw0) add(tpb, base - d, nt0);
                if (base + d >= nxw0) add(tpb, base + d, nt0);
            }
        }
    }
    hipEvent_t e0, e1;
    DLESM_HIP_TRY(hipEventCreate(&e0));
    DLESM_HIP_TRY(hipEventCreate(&e1));
    int rc = DLESM_OK;
    auto measure = [&](std::vector<float> &best_of) {
        // three interleaved passes (clock drift hits all candidates alike); a trial is 3 back-to-back
        // launches between two events; the first trial of a pass is a warm-up
        for (int pass = 0; pass < 3 && !rc; pass++)
            for (size_t k = 0; k <= cand.size() && !rc; k++) {
                const SwShape c = cand[k ? k - 1 : 0];
                { std::lock_guard<std::mutex> lk(g_sw_mu); g_sw_override = c; }
                (void)hipEventRecord(e0, s);
                for (int rep = 0; rep < 3; rep++)
                    launch_shallow_tile(*q, ld, x0, x1, y0, y1, f, s, sw_offset);
                (void)hipEventRecord(e1, s);
                { std::lock_guard<std::mutex> lk(g_sw_mu); g_sw_override = SwShape{0, 0, 0}; }
                if (hipGetLastError() != hipSuccess || hipEventSynchronize(e1) != hipSuccess)
                    rc = fail(DLESM_EHIP, "shallow autotune: launch or synchronisation failed");
                float ms = 0.f;
                if (!rc && k > 0 && hipEventElapsedTime(&ms, e0, e1) == hipSuccess && ms < best_of[k - 1]) best_of[k - 1] = ms;
            }
    };
    std::vector<float> t1(cand.size(), 1e30f);
    measure(t1);
    SwShape best = cand[0];
    float best_ms = t1[0] * 0.995f;                       // the rule's choice stays unless beaten by 0.5 %
    if (!rc) {
        for (size_t k = 1; k < cand.size(); k++)
            if (t1[k] < best_ms) { best_ms = t1[k]; best = cand[k]; }
        // second round: the cache policies on the chosen shape
        cand.clear();
        for (int ntm : {best.ntm, 0, 2, 3, 1}) add(best.tpb, best.nxw, ntm);
        std::vector<float> t2(cand.size(), 1e30f);
        measure(t2);
        if (!rc) {
            best_ms = t2[0] * 0.995f;
            for (size_t k = 1; k < cand.size(); k++)
                if (t2[k] < best_ms) { best_ms = t2[k]; best = cand[k]; }
        }
    }
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    if (rc) return rc;
    std::lock_guard<std::mutex> lk(g_sw_mu);
    g_sw_cache[SwKey{ld, x0, x1, y0, y1, (sw_offset ? 1 : 0) | (hl << 1)}] = best;
    return DLESM_OK;
}

extern "C" int dlesm_shallow_autotune_f64(const dlesm_sw_params *q, int ld, int ny, int xstart, int xstop, int ystart,
                                          int ystop, const double *u, const double *v, const double *p, const double *uold,
                                          const double *vold, const double *pold, double *unew, double *vnew, double *pnew,
                                          void *stream)
{
    return shallow_autotune(false, q, ld, ny, xstart, xstop, ystart, ystop, {u, v, p, uold, vold, pold, unew, vnew, pnew}, stream);
}

extern "C" int dlesm_shallow_autotune_sw_f64(const dlesm_sw_params *q, int ld, int ny, int xstart, int xstop, int ystart,
                                             int ystop, const double *u, const double *v, const double *p, const double *uold,
                                             const double *vold, const double *pold, double *unew, double *vnew, double *pnew,
                                             void *stream)
{
    return shallow_autotune(true, q, ld, ny, xstart, xstop, ystart, ystop, {u, v, p, uold, vold, pold, unew, vnew, pnew}, stream);
}
