// Drifters: Lagrangian particles carried through the level-n C-grid flow by the midpoint rule, and
// T-point fields sampled at them.  The point rule is drifter_vel / drifter_substep (dlesm_nemolite.h); the two divisions are
// the compiler's correctly rounded f64 ones.
//
// drifter_step_k: one particle per lane, the nsub loop inside the kernel.  The status is loaded first, coalesced; a wave with
// no ACTIVE lane leaves after one ballot.  px and py are loaded coalesced and stored once, after the loop, by the lanes that
// were ACTIVE on entry.  This is a gather: every stage reads the four neighbour masks, the four faces and the two metrics of
// one cell, ten scattered 4- and 8-byte loads, all unconditional (the box's one-cell ring makes them safe) and all issued
// before any is used; the selects come after.  A substep is three dependent round trips -- stage 1, stage 2 with the
// midpoint cell's own mask, the destination's mask -- and the destination's mask serves as the next substep's own-cell mask.
// Memory latency and occupancy set the time, so the kernel is held at eight waves per SIMD.  Offsets are 64-bit, stores
// plain vector stores, no scratch, no atomics.
//
// drifter_sample_k: one particle per lane, a loop over the fields.
//
// dlesm_drifters: an owner of the three particle arrays on the device, for callers whose language has no device arrays
// other than fields.
#include <cmath>
#include <new>

#include "dlesm_nemolite.h"

namespace dlesm {

namespace {

using namespace nemo;

struct DrifterArgs {
    const int *tmask;
    const double *dx_t, *dy_t, *un, *vn;
    double *px, *py;
    int *status;
    long long n;
    DrifterBox box;
    double h;
    int nsub, ld;
};

struct SampleArgs {
    const double *px, *py;
    const int *status;
    const double *fields[DLESM_DRIFTER_MAX_FIELDS];
    double *out[DLESM_DRIFTER_MAX_FIELDS];
    long long n;
    DrifterBox box;
    int nfields, ld;
};

__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(8, 8))) void drifter_step_k(const DrifterArgs a)
{
    const long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const bool mine = p < a.n;
    const bool active = mine && a.status[p] == DLESM_DRIFTER_ACTIVE;
    if (__ballot(active) == 0) return;
    if (!active) return;

    double x = a.px[p], y = a.py[p];
    const DrifterFlow f{a.tmask, a.dx_t, a.dy_t, a.un, a.vn, a.ld};
    const auto mask = [&](int i, int j) { return f.mask(i, j); };
    const auto cell = [&](int i, int j) { return f.cell(i, j); };

    int st;
    if (!a.box.has(x, y)) {
        st = DLESM_DRIFTER_LEFT;
    } else {
        int i = (int)floor(x), j = (int)floor(y);
        const int t = mask(i, j);
        st = t < 0 ? DLESM_DRIFTER_OPEN : t == 0 ? DLESM_DRIFTER_GROUNDED : DLESM_DRIFTER_ACTIVE;
        for (int s = 0; s < a.nsub && st == DLESM_DRIFTER_ACTIVE; s++) st = drifter_substep(a.h, a.box, x, y, i, j, cell, mask);
    }
    a.px[p] = x;
    a.py[p] = y;
    if (st != DLESM_DRIFTER_ACTIVE) a.status[p] = st;
}

__global__ __launch_bounds__(256) void drifter_sample_k(const SampleArgs a)
{
    const long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= a.n || a.status[p] != DLESM_DRIFTER_ACTIVE) return;
    const double x = a.px[p], y = a.py[p];
    if (!a.box.has(x, y)) return;
    const size_t o = (size_t)((int)floor(y) - 1) * (size_t)a.ld + (size_t)((int)floor(x) - 1);
    for (int k = 0; k < a.nfields; k++) a.out[k][p] = a.fields[k][o];
}

// the checks the two entries share: extents, the box, the particle count, the three particle arrays
int check_particles(const char *who, int ld, int ny, int xstart, int xstop, int ystart, int ystop, long long n, const void *px,
                    const void *py, const void *status, bool *empty)
{
    DLESM_REQUIRE(px != nullptr && py != nullptr && status != nullptr, "%s: null px, py or status", who);
    DLESM_REQUIRE((uintptr_t)px % 8 == 0 && (uintptr_t)py % 8 == 0, "%s: px or py is not 8-byte aligned", who);
    DLESM_REQUIRE((uintptr_t)status % 4 == 0, "%s: status is not 4-byte aligned", who);
    DLESM_REQUIRE(n >= 0, "%s: %lld particles", who, n);
    DLESM_REQUIRE(ld >= 1 && ny >= 1, "%s: array extents %dx%d", who, ld, ny);
    *empty = xstop < xstart || ystop < ystart;
    if (!*empty)
        if (int rc = check_box(who, ld, ny, xstart, xstop, ystart, ystop, 1)) return rc;
    DLESM_REQUIRE((n + 255) / 256 <= 0x7fffffffLL, "%s: %lld particles in one call", who, n);
    return DLESM_OK;
}

} // namespace

// the checks every particle step shares (dlesm_dispersal.hip makes them too): what dlesm_drifter_step_f64 refuses.
// *nothing: n == 0 or an empty box
int lagrangian_step_checks(const char *who, double h, int nsub, int ld, int ny, int xstart, int xstop, int ystart, int ystop,
                           const int *tmask, const double *dx_t, const double *dy_t, const double *un, const double *vn,
                           long long n, const double *px, const double *py, const int *status, bool *nothing)
{
    static const char *const in_name[4] = {"dx_t", "dy_t", "un", "vn"};
    static const char *const p_name[3] = {"px", "py", "status"};
    DLESM_REQUIRE(std::isfinite(h), "%s: h = %g (a finite number of seconds)", who, h);
    DLESM_REQUIRE(nsub >= 1 && nsub <= DLESM_DRIFTER_MAX_SUB, "%s: nsub = %d (1..%d)", who, nsub, DLESM_DRIFTER_MAX_SUB);
    const double *const ins[4] = {dx_t, dy_t, un, vn};
    DLESM_REQUIRE(tmask != nullptr, "%s: null tmask", who);
    DLESM_REQUIRE((uintptr_t)tmask % 4 == 0, "%s: tmask is not 4-byte aligned", who);
    for (int m = 0; m < 4; m++) {
        DLESM_REQUIRE(ins[m] != nullptr, "%s: null %s", who, in_name[m]);
        DLESM_REQUIRE((uintptr_t)ins[m] % 8 == 0, "%s: %s is not 8-byte aligned", who, in_name[m]);
    }
    bool empty;
    if (int rc = check_particles(who, ld, ny, xstart, xstop, ystart, ystop, n, px, py, status, &empty)) return rc;
    const size_t nb = (size_t)ld * (size_t)ny * sizeof(double);
    const void *const parts[3] = {px, py, status};
    const size_t pb[3] = {(size_t)n * 8, (size_t)n * 8, (size_t)n * 4};
    for (int k = 0; k < 3 && n > 0; k++) {
        DLESM_REQUIRE(!overlap(parts[k], pb[k], tmask, nb / 2), "%s: %s overlaps tmask", who, p_name[k]);
        for (int m = 0; m < 4; m++)
            DLESM_REQUIRE(!overlap(parts[k], pb[k], ins[m], nb), "%s: %s overlaps the input %s", who, p_name[k], in_name[m]);
        for (int m = k + 1; m < 3; m++)
            DLESM_REQUIRE(!overlap(parts[k], pb[k], parts[m], pb[m]), "%s: %s and %s overlap", who, p_name[k], p_name[m]);
    }
    *nothing = n == 0 || empty;
    return DLESM_OK;
}

} // namespace dlesm

using namespace dlesm;

extern "C" int dlesm_drifter_step_f64(double h, int nsub, int ld, int ny, int xstart, int xstop, int ystart, int ystop,
                                      const int *tmask, const double *dx_t, const double *dy_t, const double *un,
                                      const double *vn, long long n, double *px, double *py, int *status, void *stream)
{
    static const char *const who = "dlesm_drifter_step_f64";
    if (int rc = ensure_device()) return rc;
    bool nothing;
    if (int rc = lagrangian_step_checks(who, h, nsub, ld, ny, xstart, xstop, ystart, ystop, tmask, dx_t, dy_t, un, vn, n, px, py,
                                        status, &nothing))
        return rc;
    if (nothing) return DLESM_OK;

    const DrifterArgs a{tmask, dx_t, dy_t, un, vn, px, py, status, n,
                        DrifterBox{(double)xstart, (double)xstop + 1.0, (double)ystart, (double)ystop + 1.0}, h, nsub, ld};
    hipLaunchKernelGGL(drifter_step_k, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a);
    DLESM_HIP_TRY(hipGetLastError());
    return DLESM_OK;
}

extern "C" int dlesm_drifter_sample_f64(int ld, int ny, int xstart, int xstop, int ystart, int ystop, long long n,
                                        const double *px, const double *py, const int *status, const double *const *fields,
                                        double *const *out, int nfields, void *stream)
{
    static const char *const who = "dlesm_drifter_sample_f64";
    static const char *const p_name[3] = {"px", "py", "status"};
    if (int rc = ensure_device()) return rc;
    DLESM_REQUIRE(nfields >= 1 && nfields <= DLESM_DRIFTER_MAX_FIELDS, "%s: nfields = %d (1..%d)", who, nfields,
                  DLESM_DRIFTER_MAX_FIELDS);
    DLESM_REQUIRE(fields != nullptr && out != nullptr, "%s: null fields or out", who);
    for (int k = 0; k < nfields; k++) {
        DLESM_REQUIRE(fields[k] != nullptr && out[k] != nullptr, "%s: null fields[%d] or out[%d]", who, k, k);
        DLESM_REQUIRE((uintptr_t)fields[k] % 8 == 0 && (uintptr_t)out[k] % 8 == 0,
                      "%s: fields[%d] or out[%d] is not 8-byte aligned", who, k, k);
    }
    bool empty;
    if (int rc = check_particles(who, ld, ny, xstart, xstop, ystart, ystop, n, px, py, status, &empty)) return rc;
    const size_t nb = (size_t)ld * (size_t)ny * sizeof(double);
    const void *const parts[3] = {px, py, status};
    const size_t pb[3] = {(size_t)n * 8, (size_t)n * 8, (size_t)n * 4};
    for (int k = 0; k < nfields && n > 0; k++) {
        for (int m = 0; m < 3; m++)
            DLESM_REQUIRE(!overlap(out[k], pb[0], parts[m], pb[m]), "%s: out[%d] overlaps %s", who, k, p_name[m]);
        for (int m = 0; m < nfields; m++)
            DLESM_REQUIRE(!overlap(out[k], pb[0], fields[m], nb), "%s: out[%d] overlaps fields[%d]", who, k, m);
        for (int m = k + 1; m < nfields; m++)
            DLESM_REQUIRE(!overlap(out[k], pb[0], out[m], pb[0]), "%s: out[%d] and out[%d] overlap", who, k, m);
    }
    if (n == 0 || empty) return DLESM_OK;

    SampleArgs a{px, py, status, {}, {}, n,
                 DrifterBox{(double)xstart, (double)xstop + 1.0, (double)ystart, (double)ystop + 1.0}, nfields, ld};
    for (int k = 0; k < nfields; k++) a.fields[k] = fields[k], a.out[k] = out[k];
    hipLaunchKernelGGL(drifter_sample_k, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a);
    DLESM_HIP_TRY(hipGetLastError());
    return DLESM_OK;
}

// ---- the owner of the three arrays (the struct: dlesm_internal.h)
static int drifters_ok(const char *who, const dlesm_drifters *set)
{
    DLESM_REQUIRE(set != nullptr && set->magic == DLESM_DRIFTERS_MAGIC, "%s: not a drifter set", who);
    return DLESM_OK;
}

extern "C" int dlesm_drifters_create(long long n, dlesm_drifters **set)
{
    static const char *const who = "dlesm_drifters_create";
    if (int rc = ensure_device()) return rc;
    DLESM_REQUIRE(set != nullptr, "%s: null set", who);
    *set = nullptr;
    DLESM_REQUIRE(n >= 0, "%s: %lld particles", who, n);
    dlesm_drifters *d = new (std::nothrow) dlesm_drifters{};
    if (!d) return fail(DLESM_EHIP, "%s: out of host memory", who);
    d->magic = DLESM_DRIFTERS_MAGIC, d->n = n;
    if (n > 0) {
        // one allocation: px | py | status (each 8-byte aligned)
        void *base = nullptr;
        if (hipMalloc(&base, (size_t)n * 20) != hipSuccess) {
            delete d;
            return fail(DLESM_EHIP, "%s: no device memory for %lld particles", who, n);
        }
        d->px = (double *)base, d->py = d->px + n, d->status = (int *)(d->py + n);
        if (hipMemset(d->status, 0, (size_t)n * 4) != hipSuccess) {
            (void)hipFree(base);
            delete d;
            return fail(DLESM_EHIP, "%s: hipMemset failed", who);
        }
    }
    *set = d;
    return DLESM_OK;
}

extern "C" int dlesm_drifters_put(dlesm_drifters *set, const double *px, const double *py, const int *status)
{
    static const char *const who = "dlesm_drifters_put";
    if (int rc = drifters_ok(who, set)) return rc;
    DLESM_REQUIRE(px != nullptr && py != nullptr, "%s: null px or py", who);
    if (set->n == 0) return DLESM_OK;
    const size_t n = (size_t)set->n;
    set->sorted = false;                                 // origin is the identity again (section 6.18)
    DLESM_HIP_TRY(hipMemcpy(set->px, px, n * 8, hipMemcpyHostToDevice));
    DLESM_HIP_TRY(hipMemcpy(set->py, py, n * 8, hipMemcpyHostToDevice));
    if (status) DLESM_HIP_TRY(hipMemcpy(set->status, status, n * 4, hipMemcpyHostToDevice));
    else DLESM_HIP_TRY(hipMemset(set->status, 0, n * 4));
    return DLESM_OK;
}

extern "C" int dlesm_drifters_get(dlesm_drifters *set, double *px, double *py, int *status)
{
    static const char *const who = "dlesm_drifters_get";
    if (int rc = drifters_ok(who, set)) return rc;
    if (set->n == 0) return DLESM_OK;
    const size_t n = (size_t)set->n;
    DLESM_HIP_TRY(hipDeviceSynchronize());               // steps on any stream have landed
    if (px) DLESM_HIP_TRY(hipMemcpy(px, set->px, n * 8, hipMemcpyDeviceToHost));
    if (py) DLESM_HIP_TRY(hipMemcpy(py, set->py, n * 8, hipMemcpyDeviceToHost));
    if (status) DLESM_HIP_TRY(hipMemcpy(status, set->status, n * 4, hipMemcpyDeviceToHost));
    return DLESM_OK;
}

extern "C" int dlesm_drifters_arrays(dlesm_drifters *set, long long *n, double **px, double **py, int **status)
{
    if (int rc = drifters_ok("dlesm_drifters_arrays", set)) return rc;
    if (n) *n = set->n;
    if (px) *px = set->px;
    if (py) *py = set->py;
    if (status) *status = set->status;
    return DLESM_OK;
}

extern "C" int dlesm_drifters_destroy(dlesm_drifters *set)
{
    if (!set) return DLESM_OK;
    if (int rc = drifters_ok("dlesm_drifters_destroy", set)) return rc;
    set->magic = 0;
    if (set->px) (void)hipFree(set->px);
    if (set->sort_mem) (void)hipFree(set->sort_mem);
    if (set->bin_mem) (void)hipFree(set->bin_mem);
    delete set;
    return DLESM_OK;
}
