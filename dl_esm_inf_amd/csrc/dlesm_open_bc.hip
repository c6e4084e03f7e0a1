// The open-boundary kernels of a NEMOLite2D-class model: bc_ssh (the tidal sea-surface height on open T cells) and the
// Flather condition on u and v faces.  The reference holds no such loop: the specification is frozen in DESIGN.md
// section 6.6 and the kernel below evaluates it as written there, every operation rounded in double precision in the order
// the parentheses give (built with -ffp-contract=off).  sqrt and the division are the compiler's correctly rounded f64
// expansions (v_div_scale / v_div_fmas / v_div_fixup; v_rsq_f64 with two refinement steps and scaling), never the
// approximate instructions alone.
//
// Open cells lie along the edge of the basin, O(perimeter) of them: instead of a masked sweep over the whole array (4 B/cell
// of tmask for a few thousand writes), dlesm_obc_create scans the host mask once and keeps three lists of linear indices in
// HBM.  obc_apply walks one, two or all three lists in a single launch, one entry per thread; the separate entries and the
// fused one launch the same kernel, so they cannot drift apart.
#include <vector>

#include "dlesm_internal.h"

namespace dlesm {

namespace {

struct ObcArgs {
    const int *t, *uf, *ui, *uo, *vf, *vi, *vo;
    int nt, nu, nv;                  // entries of each list this launch walks (0: the list is skipped)
    double ssh_bc, g;
    const double *hu, *sshn_u, *hv, *sshn_v, *sshn_t;
    double *ssha, *ua, *va;
};

// Flather on one face f: in = the inner face across the wet cell, o = the open T cell.  The open side
// lies on the far side of f from `in`: in > f is an open side to the west / south (minus), in < f to the east / north (plus).
__device__ __forceinline__ void flather(double *x, const double *h, const double *sshn_x, const double *sshn_t, double g, int f,
                                        int in, int o)
{
    const double c = sqrt(g / h[f]);
    const double cd = c * (sshn_x[in] - sshn_t[o]);
    x[f] = in > f ? x[in] - cd : x[in] + cd;
}

__global__ __launch_bounds__(256) void obc_apply(ObcArgs a)
{
    int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k < a.nt) {
        a.ssha[a.t[k]] = a.ssh_bc;
        return;
    }
    k -= a.nt;
    if (k < a.nu) {
        flather(a.ua, a.hu, a.sshn_u, a.sshn_t, a.g, a.uf[k], a.ui[k], a.uo[k]);
        return;
    }
    k -= a.nu;
    if (k < a.nv) flather(a.va, a.hv, a.sshn_v, a.sshn_t, a.g, a.vf[k], a.vi[k], a.vo[k]);
}

// the open faces of one box: (di, dj) = (1, 0) for u faces, (0, 1) for v faces; indices 0-based linear
int scan_faces(const char *who, const char *kind, const int *tm, int ld, int ny, const dlesm_region *box, int di, int dj,
               std::vector<int> &f, std::vector<int> &in, std::vector<int> &o)
{
    if (box->xstop < box->xstart || box->ystop < box->ystart) return DLESM_OK;
    if (int rc = check_box(who, ld, ny, box->xstart, box->xstop, box->ystart, box->ystop, 1)) return rc;
    const long step = di + (long)dj * ld;
    for (int j = box->ystart - 1; j <= box->ystop - 1; j++)
        for (int i = box->xstart - 1; i <= box->xstop - 1; i++) {
            const long c = (long)j * ld + i;
            const int t0 = tm[c], t1 = tm[c + step];
            if (!((t0 < 0 && t1 > 0) || (t0 > 0 && t1 < 0))) continue;
            // the inner face lies across the wet cell; it and both its T cells must be in the array
            const int ii = t0 < 0 ? i + di : i - di, jj = t0 < 0 ? j + dj : j - dj;
            DLESM_REQUIRE(ii >= 0 && jj >= 0 && ii + di < ld && jj + dj < ny,
                          "%s: the open %s face (%d,%d) has its inner face (%d,%d) at the edge of the array", who, kind,
                          i + 1, j + 1, ii + 1, jj + 1);
            const long ci = (long)jj * ld + ii;
            const int s0 = tm[ci], s1 = tm[ci + step];
            DLESM_REQUIRE(!((s0 < 0 && s1 > 0) || (s0 > 0 && s1 < 0)),
                          "%s: the open %s face (%d,%d) has an open inner face (%d,%d): the wet region between two open "
                          "cells is one cell wide", who, kind, i + 1, j + 1, ii + 1, jj + 1);
            f.push_back((int)c);
            in.push_back((int)ci);
            o.push_back((int)(t0 < 0 ? c : c + step));
        }
    return DLESM_OK;
}

enum { W_SSH = 1, W_U = 2, W_V = 4 };

int obc_launch(const char *who, int which, const dlesm_obc *p, const dlesm_momentum_params *prm, double ssh_bc,
               const double *hu, const double *sshn_u, const double *hv, const double *sshn_v, const double *sshn_t,
               double *ssha, double *ua, double *va, void *stream)
{
    DLESM_REQUIRE(p, "%s: null plan", who);
    DLESM_REQUIRE(!(which & (W_U | W_V)) || prm, "%s: null parameter pointer", who);
    const double *ins[5] = {hu, sshn_u, hv, sshn_v, sshn_t};
    double *outs[3] = {which & W_SSH ? ssha : nullptr, which & W_U ? ua : nullptr, which & W_V ? va : nullptr};
    const bool need[5] = {(which & W_U) != 0, (which & W_U) != 0, (which & W_V) != 0, (which & W_V) != 0,
                          (which & (W_U | W_V)) != 0};
    for (int k = 0; k < 5; k++) DLESM_REQUIRE(!need[k] || ins[k], "%s: null input pointer", who);
    for (int k = 0; k < 3; k++) DLESM_REQUIRE(!(which & (1 << k)) || outs[k], "%s: null output pointer", who);
    const size_t nb = (size_t)p->ld * (size_t)p->ny * sizeof(double);
    for (int k = 0; k < 3; k++) {
        if (!outs[k]) continue;
        for (int m = 0; m < 5; m++)
            DLESM_REQUIRE(!need[m] || !overlap(outs[k], nb, ins[m], nb), "%s: an output overlaps an input", who);
        for (int m = k + 1; m < 3; m++)
            DLESM_REQUIRE(!outs[m] || !overlap(outs[k], nb, outs[m], nb), "%s: two outputs overlap", who);
    }
    ObcArgs a{};
    a.nt = which & W_SSH ? p->nt : 0;
    a.nu = which & W_U ? p->nu : 0;
    a.nv = which & W_V ? p->nv : 0;
    const long n = (long)a.nt + a.nu + a.nv;
    if (n == 0) return DLESM_OK;                         // no open cell in the lists this entry walks
    if (int rc = ensure_device()) return rc;
    int *d = p->dev;
    a.t = d;
    a.uf = d + p->nt, a.ui = a.uf + p->nu, a.uo = a.ui + p->nu;
    a.vf = a.uo + p->nu, a.vi = a.vf + p->nv, a.vo = a.vi + p->nv;
    a.ssh_bc = ssh_bc;
    a.g = prm ? prm->g : 0.0;
    a.hu = hu, a.sshn_u = sshn_u, a.hv = hv, a.sshn_v = sshn_v, a.sshn_t = sshn_t;
    a.ssha = ssha, a.ua = ua, a.va = va;
    hipLaunchKernelGGL(obc_apply, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a);
    DLESM_HIP_TRY(hipGetLastError());
    return DLESM_OK;
}

} // namespace

} // namespace dlesm

using namespace dlesm;

extern "C" int dlesm_obc_create(const int *tmask_host, int ld, int ny, const dlesm_region *tbox, const dlesm_region *ubox,
                                const dlesm_region *vbox, dlesm_obc **out)
{
    static const char *who = "dlesm_obc_create";
    DLESM_REQUIRE(out, "%s: null output pointer", who);
    *out = nullptr;
    DLESM_REQUIRE(tmask_host && tbox && ubox && vbox, "%s: null mask or region", who);
    DLESM_REQUIRE(ld >= 1 && ny >= 1, "%s: array extents %dx%d", who, ld, ny);
    DLESM_REQUIRE((long)ld * ny < (1L << 31), "%s: %dx%d cells do not fit an int32 index", who, ld, ny);
    std::vector<int> t, uf, ui, uo, vf, vi, vo;
    if (tbox->xstop >= tbox->xstart && tbox->ystop >= tbox->ystart) {
        if (int rc = check_box(who, ld, ny, tbox->xstart, tbox->xstop, tbox->ystart, tbox->ystop, 0)) return rc;
        for (int j = tbox->ystart - 1; j <= tbox->ystop - 1; j++)
            for (int i = tbox->xstart - 1; i <= tbox->xstop - 1; i++)
                if (tmask_host[(long)j * ld + i] < 0) t.push_back(j * ld + i);
    }
    if (int rc = scan_faces(who, "u", tmask_host, ld, ny, ubox, 1, 0, uf, ui, uo)) return rc;
    if (int rc = scan_faces(who, "v", tmask_host, ld, ny, vbox, 0, 1, vf, vi, vo)) return rc;

    dlesm_obc *p = new dlesm_obc{ld, ny, (int)t.size(), (int)uf.size(), (int)vf.size(), nullptr};
    std::vector<int> all;
    all.reserve(t.size() + 3 * uf.size() + 3 * vf.size());
    for (const std::vector<int> *v : {&t, &uf, &ui, &uo, &vf, &vi, &vo}) all.insert(all.end(), v->begin(), v->end());
    if (!all.empty()) {
        int rc = ensure_device();
        if (rc == DLESM_OK && hipMalloc((void **)&p->dev, all.size() * sizeof(int)) != hipSuccess) {
            p->dev = nullptr;
            rc = fail(DLESM_EHIP, "%s: hipMalloc of %zu bytes failed", who, all.size() * sizeof(int));
        }
        if (rc == DLESM_OK && hipMemcpy(p->dev, all.data(), all.size() * sizeof(int), hipMemcpyHostToDevice) != hipSuccess)
            rc = fail(DLESM_EHIP, "%s: upload of the lists failed", who);
        if (rc != DLESM_OK) {
            if (p->dev) (void)hipFree(p->dev);
            delete p;
            return rc;
        }
    }
    *out = p;
    return DLESM_OK;
}

extern "C" int dlesm_obc_destroy(dlesm_obc *plan)
{
    if (!plan) return DLESM_OK;
    if (plan->dev) DLESM_HIP_TRY(hipFree(plan->dev));
    delete plan;
    return DLESM_OK;
}

extern "C" int dlesm_obc_counts(const dlesm_obc *plan, int *nt, int *nu, int *nv)
{
    DLESM_REQUIRE(plan && nt && nu && nv, "dlesm_obc_counts: null pointer");
    *nt = plan->nt, *nu = plan->nu, *nv = plan->nv;
    return DLESM_OK;
}

extern "C" int dlesm_bc_ssh_f64(const dlesm_obc *plan, double ssh_bc, double *ssha, void *stream)
{
    return obc_launch("dlesm_bc_ssh_f64", W_SSH, plan, nullptr, ssh_bc, nullptr, nullptr, nullptr, nullptr, nullptr, ssha,
                      nullptr, nullptr, stream);
}

extern "C" int dlesm_bc_flather_u_f64(const dlesm_obc *plan, const dlesm_momentum_params *params, const double *hu,
                                      const double *sshn_u, const double *sshn_t, double *ua, void *stream)
{
    return obc_launch("dlesm_bc_flather_u_f64", W_U, plan, params, 0.0, hu, sshn_u, nullptr, nullptr, sshn_t, nullptr, ua,
                      nullptr, stream);
}

extern "C" int dlesm_bc_flather_v_f64(const dlesm_obc *plan, const dlesm_momentum_params *params, const double *hv,
                                      const double *sshn_v, const double *sshn_t, double *va, void *stream)
{
    return obc_launch("dlesm_bc_flather_v_f64", W_V, plan, params, 0.0, nullptr, nullptr, hv, sshn_v, sshn_t, nullptr,
                      nullptr, va, stream);
}

extern "C" int dlesm_bc_open_f64(const dlesm_obc *plan, const dlesm_momentum_params *params, double ssh_bc, const double *hu,
                                 const double *sshn_u, const double *hv, const double *sshn_v, const double *sshn_t,
                                 double *ssha, double *ua, double *va, void *stream)
{
    return obc_launch("dlesm_bc_open_f64", W_SSH | W_U | W_V, plan, params, ssh_bc, hu, sshn_u, hv, sshn_v, sshn_t, ssha,
                      ua, va, stream);
}
