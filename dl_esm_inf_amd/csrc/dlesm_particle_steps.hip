// The three particle steps (DESIGN.md sections 6.17, 6.20 and 6.22): Lagrangian particles carried through the level-n C-grid
// flow by the midpoint rule (dlesm_drifter_step_f64), with one random kick of a constant diffusivity per substep
// (dlesm_dispersal_step_f64), and with the kick made from a T-point field kh_t (dlesm_random_walk_f64).  The point rules are
// drifter_substep, dispersal_substep and random_walk_substep (dlesm_particles.h); the divisions and square roots are the
// compiler's correctly rounded f64 ones.  The random numbers come from Philox4x32-10 keyed by the seed, with the particle's
// identity and the substep's tick as the counter: no generator state is stored anywhere, so a particle's path depends on its
// id and not on its slot, the stream or the run.
//
// particle_step_k<Rule>: the one frame of the three kernels, one particle per lane, the nsub loop inside the kernel.  The
// status is loaded first, coalesced; a wave with no ACTIVE lane leaves after one ballot.  px and py are loaded coalesced and
// stored once, after the loop, by the lanes that were ACTIVE on entry.  A rule adds what a lane needs before the loop -- nothing
// (AdvectRule), or its id and the tick (RandomStream, for DispersalRule and WalkRule) -- and the one substep call.  This is a
// gather: every stage reads the four neighbour masks, the four faces and the two metrics of one cell (and WalkRule five values
// of kh_t), scattered 4- and 8-byte loads, all unconditional (the box's one-cell ring makes them safe) and all issued before
// any is used; the selects come after.  A substep is three dependent round trips -- stage 1, stage 2 with the midpoint
// cell's own mask, the destination's mask (with a kick: the masks of the kicked and of the unkicked destination together)
// -- and the destination's mask serves as the next substep's own-cell mask.  Philox -- twenty 32 x 32 -> 64 bit
// multiplications and some xors, no memory -- stands between the stage-1 loads and their first use.  Memory latency and
// occupancy set the time, so the kernels are held at eight waves per SIMD: 44, 61 and 59 VGPRs, no scratch (LAB_NOTES.md has
// the compiler's report beside that of the three kernels this frame replaced).  Offsets are 64-bit, stores plain vector
// stores, no LDS, no atomics.
//
// tick_bump_k: one lane, *tick_dev += nsub behind the step on the same stream, so that a captured time loop draws fresh
// numbers on every replay.
#include <climits>
#include <cmath>

#include "dlesm_particles.h"

namespace dlesm {

namespace {

using namespace nemo;

// what every step takes
struct StepArgs {
    DrifterFlow flow;
    double *px, *py;
    int *status;
    long long n;
    DrifterBox box;
    double h;
    int nsub;
};

// A rule: lane(p), what particle p needs before its first substep, and substep(), substep s of it.
struct AdvectRule {
    struct Lane {};
    __device__ __forceinline__ Lane lane(long long) const { return Lane{}; }
    template <class CF, class TF>
    __device__ __forceinline__ int substep(const StepArgs &a, const Lane &, int, double &x, double &y, int &i, int &j, CF cell,
                                           TF mask) const
    {
        return drifter_substep(a.h, a.box, x, y, i, j, cell, mask);
    }
};

// the prologue and the generator of the two rules that draw numbers
struct RandomStream {
    const int *id;
    const long long *tick_dev;
    unsigned long long tick;
    unsigned key0, key1;
    struct Lane {
        unsigned id;
        unsigned long long tick;
    };
    __device__ __forceinline__ Lane lane(long long p) const
    {
        const unsigned i = id ? (unsigned)id[p] : (unsigned)p;
        return Lane{i, tick + (tick_dev ? (unsigned long long)*tick_dev : 0ull)};
    }
    __device__ __forceinline__ DrifterMove kick(double amp, const Lane &l, int s) const
    {
        return dispersal_kick(amp, l.id, l.tick + (unsigned)s, key0, key1);
    }
};

struct DispersalRule : RandomStream {
    double amp;
    template <class CF, class TF>
    __device__ __forceinline__ int substep(const StepArgs &a, const Lane &l, int s, double &x, double &y, int &i, int &j, CF cell,
                                           TF mask) const
    {
        return dispersal_substep(a.h, a.box, x, y, i, j, cell, mask, [&] { return kick(amp, l, s); });
    }
};

// five doubles and two square roots more than DispersalRule, and still within the 64 VGPRs of eight waves per SIMD without
// scratch
struct WalkRule : RandomStream {
    const double *kh_t;
    template <class CF, class TF>
    __device__ __forceinline__ int substep(const StepArgs &a, const Lane &l, int s, double &x, double &y, int &i, int &j, CF cell,
                                           TF mask) const
    {
        const auto kcell = [&](int ci, int cj) {
            const size_t o = a.flow.at(ci, cj);
            const size_t ld = (size_t)a.flow.ld;
            return WalkCell{kh_t[o], kh_t[o + 1], kh_t[o - 1], kh_t[o + ld], kh_t[o - ld]};
        };
        return random_walk_substep(a.h, a.box, x, y, i, j, cell, kcell, mask, [&] { return kick(1.0, l, s); });
    }
};

template <class Rule>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(8, 8))) void particle_step_k(const StepArgs a, const Rule r)
{
    const long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const bool mine = p < a.n;
    const bool active = mine && a.status[p] == DLESM_DRIFTER_ACTIVE;
    if (__ballot(active) == 0) return;
    if (!active) return;

    double x = a.px[p], y = a.py[p];
    const auto lane = r.lane(p);
    const auto mask = [&](int i, int j) { return a.flow.mask(i, j); };
    const auto cell = [&](int i, int j) { return a.flow.cell(i, j); };

    int st;
    if (!a.box.has(x, y)) {
        st = DLESM_DRIFTER_LEFT;
    } else {
        int i = (int)floor(x), j = (int)floor(y);
        const int t = mask(i, j);
        st = t < 0 ? DLESM_DRIFTER_OPEN : t == 0 ? DLESM_DRIFTER_GROUNDED : DLESM_DRIFTER_ACTIVE;
        for (int s = 0; s < a.nsub && st == DLESM_DRIFTER_ACTIVE; s++) st = r.substep(a, lane, s, x, y, i, j, cell, mask);
    }
    a.px[p] = x;
    a.py[p] = y;
    if (st != DLESM_DRIFTER_ACTIVE) a.status[p] = st;
}

__global__ __launch_bounds__(64) void tick_bump_k(long long *tick_dev, int nsub)
{
    if (threadIdx.x == 0 && blockIdx.x == 0) *tick_dev = (long long)((unsigned long long)*tick_dev + (unsigned)nsub);
}

// everything dlesm_drifter_step_f64 refuses, for every entry that steps particles; *nothing = n == 0 or an empty box: return
// DLESM_OK without a launch
int lagrangian_step_checks(const char *who, double h, int nsub, const DrifterFlow &f, int ny, int xstart, int xstop, int ystart,
                           int ystop, const ParticleArrays &P, bool *nothing)
{
    static const char *const in_name[4] = {"dx_t", "dy_t", "un", "vn"};
    DLESM_REQUIRE(std::isfinite(h), "%s: h = %g (a finite number of seconds)", who, h);
    DLESM_REQUIRE(nsub >= 1 && nsub <= DLESM_DRIFTER_MAX_SUB, "%s: nsub = %d (1..%d)", who, nsub, DLESM_DRIFTER_MAX_SUB);
    const double *const ins[4] = {f.dx_t, f.dy_t, f.un, f.vn};
    DLESM_REQUIRE(f.tmask != nullptr, "%s: null tmask", who);
    DLESM_REQUIRE((uintptr_t)f.tmask % 4 == 0, "%s: tmask is not 4-byte aligned", who);
    for (int m = 0; m < 4; m++) {
        DLESM_REQUIRE(ins[m] != nullptr, "%s: null %s", who, in_name[m]);
        DLESM_REQUIRE((uintptr_t)ins[m] % 8 == 0, "%s: %s is not 8-byte aligned", who, in_name[m]);
    }
    bool empty;
    if (int rc = P.check(who, f.ld, ny, xstart, xstop, ystart, ystop, &empty)) return rc;
    const size_t nb = (size_t)f.ld * (size_t)ny * sizeof(double);
    for (int k = 0; k < 3; k++) {
        DLESM_REQUIRE(!P.hits(k, f.tmask, nb / 2), "%s: %s overlaps tmask", who, P.name(k));
        for (int m = 0; m < 4; m++)
            DLESM_REQUIRE(!P.hits(k, ins[m], nb), "%s: %s overlaps the input %s", who, P.name(k), in_name[m]);
        for (int m = k + 1; m < 3; m++)
            DLESM_REQUIRE(!P.hits(k, P.p[m], P.bytes(m)), "%s: %s and %s overlap", who, P.name(k), P.name(m));
    }
    *nothing = P.n == 0 || empty;
    return DLESM_OK;
}

// what a step that draws random numbers refuses beyond lagrangian_step_checks: the rules of tick, id and tick_dev
int random_stream_checks(const char *who, int nsub, long long tick, const long long *tick_dev, const DrifterFlow &f, int ny,
                         const int *id, const ParticleArrays &P)
{
    static const char *const in_name[5] = {"tmask", "dx_t", "dy_t", "un", "vn"};
    DLESM_REQUIRE(tick >= 0 && tick <= LLONG_MAX - nsub, "%s: tick = %lld (>= 0, tick + nsub representable)", who, tick);
    DLESM_REQUIRE((uintptr_t)id % 4 == 0, "%s: id is not 4-byte aligned", who);
    DLESM_REQUIRE((uintptr_t)tick_dev % 8 == 0, "%s: tick_dev is not 8-byte aligned", who);
    const size_t nb = (size_t)f.ld * (size_t)ny * sizeof(double);
    for (int k = 0; k < 3; k++) {
        DLESM_REQUIRE(!id || !P.hits(k, id, (size_t)P.n * 4), "%s: id overlaps %s", who, P.name(k));
        DLESM_REQUIRE(!tick_dev || !P.hits(k, tick_dev, 8), "%s: tick_dev overlaps %s", who, P.name(k));
    }
    if (tick_dev) {
        const void *const ins[5] = {f.tmask, f.dx_t, f.dy_t, f.un, f.vn};
        for (int m = 0; m < 5; m++)
            DLESM_REQUIRE(!overlap(tick_dev, 8, ins[m], m == 0 ? nb / 2 : nb), "%s: tick_dev overlaps the input %s", who,
                          in_name[m]);
        DLESM_REQUIRE(!id || !overlap(tick_dev, 8, id, (size_t)P.n * 4), "%s: tick_dev overlaps the input id", who);
    }
    return DLESM_OK;
}

RandomStream random_stream(const int *id, const long long *tick_dev, long long tick, long long seed)
{
    return RandomStream{id, tick_dev, (unsigned long long)tick, (unsigned)((unsigned long long)seed & 0xffffffffull),
                        (unsigned)((unsigned long long)seed >> 32)};
}

// the step, and behind it on the stream *tick_dev += nsub where the rule's numbers count from it
template <class Rule>
int launch_step(const StepArgs &a, const Rule &r, const long long *tick_dev, hipStream_t stream)
{
    hipLaunchKernelGGL(particle_step_k<Rule>, dim3((unsigned)((a.n + 255) / 256)), dim3(256), 0, stream, a, r);
    DLESM_HIP_TRY(hipGetLastError());
    if (!tick_dev) return DLESM_OK;
    hipLaunchKernelGGL(tick_bump_k, dim3(1), dim3(64), 0, stream, const_cast<long long *>(tick_dev), a.nsub);
    DLESM_HIP_TRY(hipGetLastError());
    return DLESM_OK;
}

} // namespace

} // namespace dlesm

using namespace dlesm;

extern "C" int dlesm_drifter_step_f64(double h, int nsub, int ld, int ny, int xstart, int xstop, int ystart, int ystop,
                                      const int *tmask, const double *dx_t, const double *dy_t, const double *un,
                                      const double *vn, long long n, double *px, double *py, int *status, void *stream)
{
    static const char *const who = "dlesm_drifter_step_f64";
    if (int rc = ensure_device()) return rc;
    const DrifterFlow f{tmask, dx_t, dy_t, un, vn, ld};
    const ParticleArrays P{{px, py, status}, n};
    bool nothing;
    if (int rc = lagrangian_step_checks(who, h, nsub, f, ny, xstart, xstop, ystart, ystop, P, &nothing)) return rc;
    if (nothing) return DLESM_OK;
    const StepArgs a{f, px, py, status, n, drifter_box(xstart, xstop, ystart, ystop), h, nsub};
    return launch_step(a, AdvectRule{}, nullptr, (hipStream_t)stream);
}

extern "C" int dlesm_dispersal_step_f64(double h, int nsub, double kh, long long seed, long long tick, const long long *tick_dev,
                                        int ld, int ny, int xstart, int xstop, int ystart, int ystop, const int *tmask,
                                        const double *dx_t, const double *dy_t, const double *un, const double *vn, long long n,
                                        const int *id, double *px, double *py, int *status, void *stream)
{
    static const char *const who = "dlesm_dispersal_step_f64";
    if (int rc = ensure_device()) return rc;
    const DrifterFlow f{tmask, dx_t, dy_t, un, vn, ld};
    const ParticleArrays P{{px, py, status}, n};
    bool nothing;
    if (int rc = lagrangian_step_checks(who, h, nsub, f, ny, xstart, xstop, ystart, ystop, P, &nothing)) return rc;
    DLESM_REQUIRE(std::isfinite(kh) && kh >= 0.0, "%s: kh = %g (a finite diffusivity >= 0 in m2/s)", who, kh);
    if (int rc = random_stream_checks(who, nsub, tick, tick_dev, f, ny, id, P)) return rc;
    if (nothing) return DLESM_OK;
    const StepArgs a{f, px, py, status, n, drifter_box(xstart, xstop, ystart, ystop), h, nsub};
    const DispersalRule r{random_stream(id, tick_dev, tick, seed), sqrt((6.0 * kh) * fabs(h))};
    return launch_step(a, r, tick_dev, (hipStream_t)stream);
}

extern "C" int dlesm_dispersal_step_set(dlesm_drifters *set, double h, int nsub, double kh, long long seed, long long tick,
                                        const long long *tick_dev, int ld, int ny, int xstart, int xstop, int ystart, int ystop,
                                        const int *tmask, const double *dx_t, const double *dy_t, const double *un,
                                        const double *vn, void *stream)
{
    if (int rc = ensure_device()) return rc;
    if (int rc = drifters_ok("dlesm_dispersal_step_set", set)) return rc;
    if (set->n == 0) return DLESM_OK;
    // origin (section 6.18) is the particle's identity; before the first sort since a put it is the identity: NULL
    return dlesm_dispersal_step_f64(h, nsub, kh, seed, tick, tick_dev, ld, ny, xstart, xstop, ystart, ystop, tmask, dx_t, dy_t, un,
                                    vn, set->n, set->sorted ? set->origin : nullptr, set->px, set->py, set->status, stream);
}

extern "C" int dlesm_random_walk_f64(double h, int nsub, const double *kh_t, long long seed, long long tick,
                                     const long long *tick_dev, int ld, int ny, int xstart, int xstop, int ystart, int ystop,
                                     const int *tmask, const double *dx_t, const double *dy_t, const double *un, const double *vn,
                                     long long n, const int *id, double *px, double *py, int *status, void *stream)
{
    static const char *const who = "dlesm_random_walk_f64";
    if (int rc = ensure_device()) return rc;
    const DrifterFlow f{tmask, dx_t, dy_t, un, vn, ld};
    const ParticleArrays P{{px, py, status}, n};
    bool nothing;
    if (int rc = lagrangian_step_checks(who, h, nsub, f, ny, xstart, xstop, ystart, ystop, P, &nothing)) return rc;
    if (int rc = random_stream_checks(who, nsub, tick, tick_dev, f, ny, id, P)) return rc;
    DLESM_REQUIRE(kh_t != nullptr, "%s: null kh_t", who);
    DLESM_REQUIRE((uintptr_t)kh_t % 8 == 0, "%s: kh_t is not 8-byte aligned", who);
    const size_t nb = (size_t)ld * (size_t)ny * sizeof(double);
    const int k = P.which(kh_t, nb);
    DLESM_REQUIRE(k < 0, "%s: %s overlaps the input kh_t", who, P.name(k));
    DLESM_REQUIRE(!tick_dev || !overlap(tick_dev, 8, kh_t, nb), "%s: tick_dev overlaps the input kh_t", who);
    if (nothing) return DLESM_OK;
    const StepArgs a{f, px, py, status, n, drifter_box(xstart, xstop, ystart, ystop), h, nsub};
    const WalkRule r{random_stream(id, tick_dev, tick, seed), kh_t};
    return launch_step(a, r, tick_dev, (hipStream_t)stream);
}

extern "C" int dlesm_random_walk_set(dlesm_drifters *set, double h, int nsub, const double *kh_t, long long seed, long long tick,
                                     const long long *tick_dev, int ld, int ny, int xstart, int xstop, int ystart, int ystop,
                                     const int *tmask, const double *dx_t, const double *dy_t, const double *un, const double *vn,
                                     void *stream)
{
    if (int rc = ensure_device()) return rc;
    if (int rc = drifters_ok("dlesm_random_walk_set", set)) return rc;
    if (set->n == 0) return DLESM_OK;
    // origin (section 6.18) is the particle's identity, as for dlesm_dispersal_step_set
    return dlesm_random_walk_f64(h, nsub, kh_t, seed, tick, tick_dev, ld, ny, xstart, xstop, ystart, ystop, tmask, dx_t, dy_t, un, vn,
                                 set->n, set->sorted ? set->origin : nullptr, set->px, set->py, set->status, stream);
}
