// Drifters: T-point fields sampled at Lagrangian particles, and the owner of their arrays.  The steps
// that move them are in dlesm_particle_steps.hip, the point rules in dlesm_particles.h.
//
// drifter_sample_k: one particle per lane, a loop over the fields.
//
// dlesm_drifters: an owner of the three particle arrays on the device, for callers whose language has no device arrays
// other than fields.
#include <cmath>
#include <new>

#include "dlesm_particles.h"

namespace dlesm {

namespace {

using namespace nemo;

struct SampleArgs {
    const double *px, *py;
    const int *status;
    const double *fields[DLESM_DRIFTER_MAX_FIELDS];
    double *out[DLESM_DRIFTER_MAX_FIELDS];
    long long n;
    DrifterBox box;
    int nfields, ld;
};

__global__ __launch_bounds__(256) void drifter_sample_k(const SampleArgs a)
{
    const long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= a.n || a.status[p] != DLESM_DRIFTER_ACTIVE) return;
    const double x = a.px[p], y = a.py[p];
    if (!a.box.has(x, y)) return;
    const size_t o = (size_t)((int)floor(y) - 1) * (size_t)a.ld + (size_t)((int)floor(x) - 1);
    for (int k = 0; k < a.nfields; k++) a.out[k][p] = a.fields[k][o];
}

} // namespace

} // namespace dlesm

using namespace dlesm;

extern "C" int dlesm_drifter_sample_f64(int ld, int ny, int xstart, int xstop, int ystart, int ystop, long long n,
                                        const double *px, const double *py, const int *status, const double *const *fields,
                                        double *const *out, int nfields, void *stream)
{
    static const char *const who = "dlesm_drifter_sample_f64";
    if (int rc = ensure_device()) return rc;
    DLESM_REQUIRE(nfields >= 1 && nfields <= DLESM_DRIFTER_MAX_FIELDS, "%s: nfields = %d (1..%d)", who, nfields,
                  DLESM_DRIFTER_MAX_FIELDS);
    DLESM_REQUIRE(fields != nullptr && out != nullptr, "%s: null fields or out", who);
    for (int k = 0; k < nfields; k++) {
        DLESM_REQUIRE(fields[k] != nullptr && out[k] != nullptr, "%s: null fields[%d] or out[%d]", who, k, k);
        DLESM_REQUIRE((uintptr_t)fields[k] % 8 == 0 && (uintptr_t)out[k] % 8 == 0,
                      "%s: fields[%d] or out[%d] is not 8-byte aligned", who, k, k);
    }
    const ParticleArrays P{{px, py, status}, n};
    bool empty;
    if (int rc = P.check(who, ld, ny, xstart, xstop, ystart, ystop, &empty)) return rc;
    const size_t nb = (size_t)ld * (size_t)ny * sizeof(double), ob = P.bytes(0);
    for (int k = 0; k < nfields && n > 0; k++) {
        const int m = P.which(out[k], ob);
        DLESM_REQUIRE(m < 0, "%s: out[%d] overlaps %s", who, k, P.name(m));
        for (int f = 0; f < nfields; f++)
            DLESM_REQUIRE(!overlap(out[k], ob, fields[f], nb), "%s: out[%d] overlaps fields[%d]", who, k, f);
        for (int f = k + 1; f < nfields; f++)
            DLESM_REQUIRE(!overlap(out[k], ob, out[f], ob), "%s: out[%d] and out[%d] overlap", who, k, f);
    }
    if (n == 0 || empty) return DLESM_OK;

    SampleArgs a{px, py, status, {}, {}, n, drifter_box(xstart, xstop, ystart, ystop), nfields, ld};
    for (int k = 0; k < nfields; k++) a.fields[k] = fields[k], a.out[k] = out[k];
    hipLaunchKernelGGL(drifter_sample_k, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a);
    DLESM_HIP_TRY(hipGetLastError());
    return DLESM_OK;
}

// ---- the owner of the three arrays (the struct: dlesm_internal.h)
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
