// Drifters with random-walk diffusion: section 6.17's midpoint step plus one random kick per
// substep, uniform in a square of half-width sqrt(6 kh |h|) metres (variance 2 kh |h| per axis).  The numbers come from
// Philox4x32-10 keyed by the seed, with the particle's identity and the substep's tick as the counter: no generator state is
// stored anywhere, so a particle's path depends on its id and not on its slot, the stream or the run.  The point rule is
// dispersal_substep (dlesm_nemolite.h), beside drifter_substep, over the same loads (DrifterFlow).
//
// dispersal_step_k: one particle per lane, the nsub loop inside the kernel, as drifter_step_k.  A substep stays at three
// dependent round trips: the kick is divided by the stage-1 cell's metrics, the masks of the kicked and of the unkicked
// destination are loaded together, and the one taken is the next substep's own-cell mask.  Philox -- twenty 32 x 32 -> 64
// bit multiplications and some xors, no memory -- stands between the stage-1 loads and their first use.  Held at eight waves
// per SIMD; plain vector loads and stores, no scratch, no LDS, no atomics.
//
// tick_bump_k: one lane, *tick_dev += nsub behind the step on the same stream, so that a captured time loop draws fresh
// numbers on every replay.
#include <climits>
#include <cmath>

#include "dlesm_nemolite.h"

namespace dlesm {

namespace {

using namespace nemo;

struct DispersalArgs {
    DrifterFlow flow;
    const int *id;
    const long long *tick_dev;
    double *px, *py;
    int *status;
    long long n;
    DrifterBox box;
    double h, amp;
    unsigned long long tick;
    unsigned key0, key1;
    int nsub;
};

__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(8, 8))) void dispersal_step_k(const DispersalArgs a)
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

    int st;
    if (!a.box.has(x, y)) {
        st = DLESM_DRIFTER_LEFT;
    } else {
        int i = (int)floor(x), j = (int)floor(y);
        const int t = mask(i, j);
        st = t < 0 ? DLESM_DRIFTER_OPEN : t == 0 ? DLESM_DRIFTER_GROUNDED : DLESM_DRIFTER_ACTIVE;
        for (int s = 0; s < a.nsub && st == DLESM_DRIFTER_ACTIVE; s++)
            st = dispersal_substep(a.h, a.box, x, y, i, j, cell, mask,
                                   [&] { return dispersal_kick(a.amp, id, tick + (unsigned)s, a.key0, a.key1); });
    }
    a.px[p] = x;
    a.py[p] = y;
    if (st != DLESM_DRIFTER_ACTIVE) a.status[p] = st;
}

__global__ __launch_bounds__(64) void tick_bump_k(long long *tick_dev, int nsub)
{
    if (threadIdx.x == 0 && blockIdx.x == 0) *tick_dev = (long long)((unsigned long long)*tick_dev + (unsigned)nsub);
}

} // namespace

// what a step that draws random numbers refuses beyond lagrangian_step_checks (dlesm_random_walk.hip makes these checks too):
// the rules of tick, id and tick_dev
int random_stream_checks(const char *who, int nsub, long long tick, const long long *tick_dev, int ld, int ny, const int *tmask,
                         const double *dx_t, const double *dy_t, const double *un, const double *vn, long long n, const int *id,
                         const double *px, const double *py, const int *status)
{
    static const char *const p_name[3] = {"px", "py", "status"};
    static const char *const in_name[5] = {"tmask", "dx_t", "dy_t", "un", "vn"};
    DLESM_REQUIRE(tick >= 0 && tick <= LLONG_MAX - nsub, "%s: tick = %lld (>= 0, tick + nsub representable)", who, tick);
    DLESM_REQUIRE((uintptr_t)id % 4 == 0, "%s: id is not 4-byte aligned", who);
    DLESM_REQUIRE((uintptr_t)tick_dev % 8 == 0, "%s: tick_dev is not 8-byte aligned", who);
    const size_t nb = (size_t)ld * (size_t)ny * sizeof(double);
    const void *const parts[3] = {px, py, status};
    const size_t pb[3] = {(size_t)n * 8, (size_t)n * 8, (size_t)n * 4};
    for (int k = 0; k < 3 && n > 0; k++) {
        DLESM_REQUIRE(!id || !overlap(id, (size_t)n * 4, parts[k], pb[k]), "%s: id overlaps %s", who, p_name[k]);
        DLESM_REQUIRE(!tick_dev || !overlap(tick_dev, 8, parts[k], pb[k]), "%s: tick_dev overlaps %s", who, p_name[k]);
    }
    if (tick_dev) {
        const void *const ins[5] = {tmask, dx_t, dy_t, un, vn};
        for (int m = 0; m < 5; m++)
            DLESM_REQUIRE(!overlap(tick_dev, 8, ins[m], m == 0 ? nb / 2 : nb), "%s: tick_dev overlaps the input %s", who,
                          in_name[m]);
        DLESM_REQUIRE(!id || !overlap(tick_dev, 8, id, (size_t)n * 4), "%s: tick_dev overlaps the input id", who);
    }
    return DLESM_OK;
}

// *tick_dev += nsub behind whatever stands on the stream
int launch_tick_bump(const long long *tick_dev, int nsub, hipStream_t stream)
{
    hipLaunchKernelGGL(tick_bump_k, dim3(1), dim3(64), 0, stream, const_cast<long long *>(tick_dev), nsub);
    DLESM_HIP_TRY(hipGetLastError());
    return DLESM_OK;
}

} // namespace dlesm

using namespace dlesm;

extern "C" int dlesm_dispersal_step_f64(double h, int nsub, double kh, long long seed, long long tick, const long long *tick_dev,
                                        int ld, int ny, int xstart, int xstop, int ystart, int ystop, const int *tmask,
                                        const double *dx_t, const double *dy_t, const double *un, const double *vn, long long n,
                                        const int *id, double *px, double *py, int *status, void *stream)
{
    static const char *const who = "dlesm_dispersal_step_f64";
    if (int rc = ensure_device()) return rc;
    bool nothing;
    if (int rc = lagrangian_step_checks(who, h, nsub, ld, ny, xstart, xstop, ystart, ystop, tmask, dx_t, dy_t, un, vn, n, px, py,
                                        status, &nothing))
        return rc;
    DLESM_REQUIRE(std::isfinite(kh) && kh >= 0.0, "%s: kh = %g (a finite diffusivity >= 0 in m2/s)", who, kh);
    if (int rc = random_stream_checks(who, nsub, tick, tick_dev, ld, ny, tmask, dx_t, dy_t, un, vn, n, id, px, py, status)) return rc;
    if (nothing) return DLESM_OK;

    const DispersalArgs a{DrifterFlow{tmask, dx_t, dy_t, un, vn, ld}, id, tick_dev, px, py, status, n,
                          DrifterBox{(double)xstart, (double)xstop + 1.0, (double)ystart, (double)ystop + 1.0}, h,
                          sqrt((6.0 * kh) * fabs(h)), (unsigned long long)tick, (unsigned)((unsigned long long)seed & 0xffffffffull),
                          (unsigned)((unsigned long long)seed >> 32), nsub};
    hipLaunchKernelGGL(dispersal_step_k, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a);
    DLESM_HIP_TRY(hipGetLastError());
    return tick_dev ? launch_tick_bump(tick_dev, nsub, (hipStream_t)stream) : DLESM_OK;
}

extern "C" int dlesm_dispersal_step_set(dlesm_drifters *set, double h, int nsub, double kh, long long seed, long long tick,
                                        const long long *tick_dev, int ld, int ny, int xstart, int xstop, int ystart, int ystop,
                                        const int *tmask, const double *dx_t, const double *dy_t, const double *un,
                                        const double *vn, void *stream)
{
    static const char *const who = "dlesm_dispersal_step_set";
    if (int rc = ensure_device()) return rc;
    DLESM_REQUIRE(set != nullptr && set->magic == DLESM_DRIFTERS_MAGIC, "%s: not a drifter set", who);
    if (set->n == 0) return DLESM_OK;
    // origin (section 6.18) is the particle's identity; before the first sort since a put it is the identity: NULL
    return dlesm_dispersal_step_f64(h, nsub, kh, seed, tick, tick_dev, ld, ny, xstart, xstop, ystart, ystop, tmask, dx_t, dy_t, un,
                                    vn, set->n, set->sorted ? set->origin : nullptr, set->px, set->py, set->status, stream);
}
