// Drifters in a varying diffusivity: section 6.20's step with the kick made from a T-point field kh_t
// -- per axis the drift |h| dK/dx of Visser (1997) plus a uniform kick sized by K half a drift ahead --, so that a well-mixed
// cloud stays well mixed where kh_t varies.  The generator, the ids, the ticks, the rejection wall and the statuses are section
// 6.20's; the point rule is random_walk_substep (dlesm_nemolite.h), beside dispersal_substep, over the same tail (kicked_move).
//
// random_walk_k: one particle per lane, the nsub loop inside, as dispersal_step_k.  The five kh_t loads of a substep are
// unconditional and issued with the ten stage-1 loads, before any is used, and Philox stands between them and their first
// use: a substep stays at three dependent round trips.  Plain vector loads and stores, no scratch, no LDS, no atomics.
#include <climits>
#include <cmath>

#include "dlesm_nemolite.h"

namespace dlesm {

namespace {

using namespace nemo;

struct RandomWalkArgs {
    DrifterFlow flow;
    const double *kh_t;
    const int *id;
    const long long *tick_dev;
    double *px, *py;
    int *status;
    long long n;
    DrifterBox box;
    double h;
    unsigned long long tick;
    unsigned key0, key1;
    int nsub;
};

// five doubles and two square roots more than dispersal_step_k, and still within the 64 VGPRs of eight waves per SIMD without
// scratch (DESIGN.md section 6.22 has the compiler's report)
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(8, 8))) void random_walk_k(const RandomWalkArgs a)
{
    const long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const bool mine = p < a.n;
    const bool active = mine && a.status[p] == DLESM_DRIFTER_ACTIVE;
    if (__ballot(active) == 0) return;
    if (!active) return;

    double x = a.px[p], y = a.py[p];
    const unsigned id = a.id ? (unsigned)a.id[p] : (unsigned)p;
    const unsigned long long tick = a.tick + (a.tick_dev ? (unsigned long long)*a.tick_dev : 0ull);
    const auto mask = [&](int i, int j) { return a.flow.mask(i, j); };
    const auto cell = [&](int i, int j) { return a.flow.cell(i, j); };
    const auto kcell = [&](int i, int j) {
        const size_t o = a.flow.at(i, j);
        const size_t ld = (size_t)a.flow.ld;
        return WalkCell{a.kh_t[o], a.kh_t[o + 1], a.kh_t[o - 1], a.kh_t[o + ld], a.kh_t[o - ld]};
    };

    int st;
    if (!a.box.has(x, y)) {
        st = DLESM_DRIFTER_LEFT;
    } else {
        int i = (int)floor(x), j = (int)floor(y);
        const int t = mask(i, j);
        st = t < 0 ? DLESM_DRIFTER_OPEN : t == 0 ? DLESM_DRIFTER_GROUNDED : DLESM_DRIFTER_ACTIVE;
        for (int s = 0; s < a.nsub && st == DLESM_DRIFTER_ACTIVE; s++)
            st = random_walk_substep(a.h, a.box, x, y, i, j, cell, kcell, mask,
                                     [&] { return dispersal_kick(1.0, id, tick + (unsigned)s, a.key0, a.key1); });
    }
    a.px[p] = x;
    a.py[p] = y;
    if (st != DLESM_DRIFTER_ACTIVE) a.status[p] = st;
}

} // namespace

} // namespace dlesm

using namespace dlesm;

extern "C" int dlesm_random_walk_f64(double h, int nsub, const double *kh_t, long long seed, long long tick,
                                     const long long *tick_dev, int ld, int ny, int xstart, int xstop, int ystart, int ystop,
                                     const int *tmask, const double *dx_t, const double *dy_t, const double *un, const double *vn,
                                     long long n, const int *id, double *px, double *py, int *status, void *stream)
{
    static const char *const who = "dlesm_random_walk_f64";
    static const char *const p_name[3] = {"px", "py", "status"};
    if (int rc = ensure_device()) return rc;
    bool nothing;
    if (int rc = lagrangian_step_checks(who, h, nsub, ld, ny, xstart, xstop, ystart, ystop, tmask, dx_t, dy_t, un, vn, n, px, py,
                                        status, &nothing))
        return rc;
    if (int rc = random_stream_checks(who, nsub, tick, tick_dev, ld, ny, tmask, dx_t, dy_t, un, vn, n, id, px, py, status)) return rc;
    DLESM_REQUIRE(kh_t != nullptr, "%s: null kh_t", who);
    DLESM_REQUIRE((uintptr_t)kh_t % 8 == 0, "%s: kh_t is not 8-byte aligned", who);
    const size_t nb = (size_t)ld * (size_t)ny * sizeof(double);
    const void *const parts[3] = {px, py, status};
    const size_t pb[3] = {(size_t)n * 8, (size_t)n * 8, (size_t)n * 4};
    for (int k = 0; k < 3 && n > 0; k++)
        DLESM_REQUIRE(!overlap(parts[k], pb[k], kh_t, nb), "%s: %s overlaps the input kh_t", who, p_name[k]);
    DLESM_REQUIRE(!tick_dev || !overlap(tick_dev, 8, kh_t, nb), "%s: tick_dev overlaps the input kh_t", who);
    if (nothing) return DLESM_OK;

    const RandomWalkArgs a{DrifterFlow{tmask, dx_t, dy_t, un, vn, ld}, kh_t, id, tick_dev, px, py, status, n,
                           DrifterBox{(double)xstart, (double)xstop + 1.0, (double)ystart, (double)ystop + 1.0}, h,
                           (unsigned long long)tick, (unsigned)((unsigned long long)seed & 0xffffffffull),
                           (unsigned)((unsigned long long)seed >> 32), nsub};
    hipLaunchKernelGGL(random_walk_k, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a);
    DLESM_HIP_TRY(hipGetLastError());
    return tick_dev ? launch_tick_bump(tick_dev, nsub, (hipStream_t)stream) : DLESM_OK;
}

extern "C" int dlesm_random_walk_set(dlesm_drifters *set, double h, int nsub, const double *kh_t, long long seed, long long tick,
                                     const long long *tick_dev, int ld, int ny, int xstart, int xstop, int ystart, int ystop,
                                     const int *tmask, const double *dx_t, const double *dy_t, const double *un, const double *vn,
                                     void *stream)
{
    static const char *const who = "dlesm_random_walk_set";
    if (int rc = ensure_device()) return rc;
    DLESM_REQUIRE(set != nullptr && set->magic == DLESM_DRIFTERS_MAGIC, "%s: not a drifter set", who);
    if (set->n == 0) return DLESM_OK;
    // origin (section 6.18) is the particle's identity, as for dlesm_dispersal_step_set
    return dlesm_random_walk_f64(h, nsub, kh_t, seed, tick, tick_dev, ld, ny, xstart, xstop, ystart, ystop, tmask, dx_t, dy_t, un, vn,
                                 set->n, set->sorted ? set->origin : nullptr, set->px, set->py, set->status, stream);
}
