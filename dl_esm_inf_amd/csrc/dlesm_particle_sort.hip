// Particles in cell order: the stable ascending order of the particles' cell keys as a permutation,
// the gather that applies it, and both for the owner of dlesm_drifter.hip.  The key rule is section 6.17's inbox and cell.
//
// A least-significant-digit radix sort on 8-bit digits, passes = ceil(bit_length(ncells) / 8), known on the host.  A block
// owns SORT_TILE consecutive keys in every kernel, so one table of 256 x nblocks counts, digit-major, serves a pass:
//   sort_key_k      px, py, status (20 B a particle) -> the key, the block's live count and its histogram of digit 0
//   sort_hist_k     the block's histogram of a later digit
//   scan_*_k        one exclusive scan of the table: entry (d, b) becomes the first slot of block b's keys of digit d
//   sort_scatter_k  the stable scatter: the block walks its keys in index order, 256 at a time; a lane's rank among its
//                   wave's lanes of equal digit comes from eight ballots over the digit's bits; the four waves leave their
//                   counts in LDS and add those of the waves before them; a running base per digit carries to the next 256
// The value carried is the particle's index; the first pass takes it from the slot, the last writes perm and no keys.  perm
// is one of the two value buffers, chosen so that the last pass lands in it.
// Counts are exact integers: LDS integer adds in the histograms, no global atomics anywhere, plain vector stores, no scratch
// memory.  Every kernel is latency bound and small, so all are held at eight waves per SIMD.
//
// permute_k: one slot per lane, perm read once, a loop over the arrays; an index outside 0..n-1 stores nothing.
#include <cmath>

#include "dlesm_particles.h"

namespace dlesm {

namespace {

using namespace nemo;

#include "dlesm_scan.h"                      // SORT_BLOCK, SORT_KERNEL, block_scan and the three scan kernels

constexpr int SORT_TILE = 4096;            // keys of one block, in every kernel of a pass
constexpr long long SORT_MAX_N = 0x7fffffffLL;
constexpr int PERMUTE_MAX = 8;

// ---- pieces

// add the digits of a wave's valid lanes to the block's histogram; valid lanes are a prefix of the wave.  A wave whose
// digits are all one (sorted input, the high digits of a small box) adds once
__device__ __forceinline__ void hist_add(unsigned *hist, unsigned d, bool valid)
{
    const unsigned long long v = __ballot(valid);
    if (v == 0) return;
    const unsigned d0 = __builtin_amdgcn_readfirstlane(d);
    if (__ballot(valid && d != d0) == 0) {
        if ((threadIdx.x & 63) == 0) atomicAdd(&hist[d0], (unsigned)__popcll(v));
    } else if (valid) {
        atomicAdd(&hist[d], 1u);
    }
}

// ---- keys

struct KeyArgs {
    const double *px, *py;
    const int *status;
    unsigned *keys, *table, *live_part;
    long long n;
    CellKey cell;
    unsigned nblocks;
};

SORT_KERNEL sort_key_k(const KeyArgs a)
{
    __shared__ unsigned hist[256];
    __shared__ unsigned wlive[SORT_BLOCK / 64];
    const unsigned t = threadIdx.x;
    hist[t] = 0;
    __syncthreads();
    const long long first = (long long)blockIdx.x * SORT_TILE;
    unsigned live_here = 0;                                         // of this wave, the same on every lane
    for (int c = 0; c < SORT_TILE / SORT_BLOCK && first + c * SORT_BLOCK < a.n; c++) {
        const long long p = first + c * SORT_BLOCK + t;
        const bool valid = p < a.n;
        unsigned key = a.cell.ncells;
        bool live = false;
        if (valid) {
            const double x = a.px[p], y = a.py[p];
            live = a.cell.live(x, y, a.status[p]);
            if (live) key = a.cell.cell(x, y);
            a.keys[p] = key;
        }
        live_here += (unsigned)__popcll(__ballot(live));
        hist_add(hist, key & 255u, valid);
    }
    if ((t & 63) == 0) wlive[t >> 6] = live_here;
    __syncthreads();
    a.table[(size_t)t * a.nblocks + blockIdx.x] = hist[t];
    if (t == 0) {
        unsigned s = 0;
        for (int w = 0; w < SORT_BLOCK / 64; w++) s += wlive[w];
        a.live_part[blockIdx.x] = s;
    }
}

// one block: nlive = the sum of the blocks' live counts
SORT_KERNEL sort_nlive_k(const unsigned *live_part, unsigned nblocks, int *nlive)
{
    __shared__ unsigned wtot[SORT_BLOCK / 64];
    unsigned s = 0, total;
    for (unsigned b = threadIdx.x; b < nblocks; b += SORT_BLOCK) s += live_part[b];
    (void)block_scan(s, wtot, total);
    if (threadIdx.x == 0) *nlive = (int)total;
}

// perm = the identity, nlive = 0: an empty box (and n == 0, where only nlive is stored)
SORT_KERNEL sort_identity_k(int *perm, long long n, int *nlive)
{
    const long long p = (long long)blockIdx.x * SORT_BLOCK + threadIdx.x;
    if (p < n) perm[p] = (int)p;
    if (p == 0 && nlive) *nlive = 0;
}

// ---- one pass

SORT_KERNEL sort_hist_k(const unsigned *keys, unsigned *table, long long n, unsigned nblocks, int shift)
{
    __shared__ unsigned hist[256];
    const unsigned t = threadIdx.x;
    hist[t] = 0;
    __syncthreads();
    const long long first = (long long)blockIdx.x * SORT_TILE;
    for (int c = 0; c < SORT_TILE / SORT_BLOCK && first + c * SORT_BLOCK < n; c++) {
        const long long p = first + c * SORT_BLOCK + t;
        const bool valid = p < n;
        const unsigned key = valid ? keys[p] : 0u;
        hist_add(hist, (key >> shift) & 255u, valid);
    }
    __syncthreads();
    table[(size_t)t * nblocks + blockIdx.x] = hist[t];
}

struct ScatterArgs {
    const unsigned *keys_in, *vals_in;      // vals_in == nullptr: the value is the slot (the first pass)
    unsigned *keys_out, *vals_out;          // keys_out == nullptr: the last pass
    const unsigned *table;
    long long n;
    unsigned nblocks;
    int shift;
};

SORT_KERNEL sort_scatter_k(const ScatterArgs a)
{
    __shared__ unsigned base[256];                       // the next slot of each digit's keys of this block
    __shared__ unsigned wcount[SORT_BLOCK / 64][256];    // each wave's count of each digit among the current 256 keys
    const unsigned t = threadIdx.x, lane = t & 63, wave = t >> 6;
    base[t] = a.table[(size_t)t * a.nblocks + blockIdx.x];
    for (unsigned w = 0; w < SORT_BLOCK / 64; w++) wcount[w][t] = 0;
    __syncthreads();
    const long long first = (long long)blockIdx.x * SORT_TILE;
    for (int c = 0; c < SORT_TILE / SORT_BLOCK && first + c * SORT_BLOCK < a.n; c++) {
        const long long p = first + c * SORT_BLOCK + t;
        const bool valid = p < a.n;
        const unsigned key = valid ? a.keys_in[p] : 0u;
        const unsigned val = a.vals_in ? (valid ? a.vals_in[p] : 0u) : (unsigned)p;
        const unsigned d = (key >> a.shift) & 255u;
        // the valid lanes of this wave with this lane's digit
        unsigned long long same = __ballot(valid);
        for (int b = 0; b < 8; b++) {
            const bool bit = (d >> b) & 1u;
            const unsigned long long m = __ballot(valid && bit);
            same &= bit ? m : ~m;
        }
        const unsigned rank = (unsigned)__popcll(same & ((1ull << lane) - 1ull));
        if (valid && rank == 0) wcount[wave][d] = (unsigned)__popcll(same);
        __syncthreads();
        if (valid) {
            unsigned slot = base[d] + rank;
            for (unsigned w = 0; w < wave; w++) slot += wcount[w][d];
            if ((long long)slot < a.n) {                 // always, when the table is this pass's own
                if (a.keys_out) a.keys_out[slot] = key;
                a.vals_out[slot] = val;
            }
        }
        __syncthreads();
        unsigned sum = 0;
        for (unsigned w = 0; w < SORT_BLOCK / 64; w++) sum += wcount[w][t], wcount[w][t] = 0;
        base[t] += sum;
        __syncthreads();
    }
}

// ---- the gather

struct PermuteArgs {
    const int *perm;
    long long n;
    const void *src[PERMUTE_MAX];
    void *dst[PERMUTE_MAX];
    int elem_bytes[PERMUTE_MAX];
    int narrays;
};

SORT_KERNEL permute_k(const PermuteArgs a)
{
    const long long k = (long long)blockIdx.x * SORT_BLOCK + threadIdx.x;
    if (k >= a.n) return;
    const long long from = a.perm[k];
    if (from < 0 || from >= a.n) return;
    for (int m = 0; m < a.narrays; m++) {
        if (a.elem_bytes[m] == 8) ((uint64_t *)a.dst[m])[k] = ((const uint64_t *)a.src[m])[from];
        else ((uint32_t *)a.dst[m])[k] = ((const uint32_t *)a.src[m])[from];
    }
}

// ---- the host side

// where the pieces of the scratch lie, for n particles (every piece 16-byte aligned)
struct SortPlan {
    unsigned nblocks, m, nscan;
    size_t keys[2], vals, table, sums, live, bytes;
};

SortPlan sort_plan(long long n)
{
    SortPlan s{};
    const auto up16 = [](size_t b) { return (b + 15) / 16 * 16; };
    s.nblocks = (unsigned)((n + SORT_TILE - 1) / SORT_TILE);
    s.m = 256u * s.nblocks;
    s.nscan = (s.m + SCAN_TILE - 1) / SCAN_TILE;
    size_t at = 0;
    const auto piece = [&](size_t b) {
        const size_t here = at;
        at += up16(b);
        return here;
    };
    s.keys[0] = piece((size_t)n * 4), s.keys[1] = piece((size_t)n * 4), s.vals = piece((size_t)n * 4);
    s.table = piece((size_t)s.m * 4), s.sums = piece((size_t)s.nscan * 4), s.live = piece((size_t)s.nblocks * 4);
    s.bytes = at;
    return s;
}

int bit_length(unsigned long long v)
{
    int b = 0;
    for (; v; v >>= 1) b++;
    return b;
}

// every refusal of dlesm_particle_order_f64; *ncells = the box's cells
int check_order(const char *who, int xstart, int xstop, int ystart, int ystop, long long n, const void *px, const void *py,
                const void *status, const void *perm, const void *nlive, const void *scratch, long long scratch_bytes,
                long long *ncells)
{
    static const char *const in_name[3] = {"px", "py", "status"};
    static const char *const out_name[3] = {"perm", "nlive", "scratch"};
    DLESM_REQUIRE(px != nullptr && py != nullptr && status != nullptr, "%s: null px, py or status", who);
    DLESM_REQUIRE(perm != nullptr && scratch != nullptr, "%s: null perm or scratch", who);
    DLESM_REQUIRE((uintptr_t)px % 8 == 0 && (uintptr_t)py % 8 == 0, "%s: px or py is not 8-byte aligned", who);
    DLESM_REQUIRE((uintptr_t)status % 4 == 0 && (uintptr_t)perm % 4 == 0 && (uintptr_t)nlive % 4 == 0,
                  "%s: status, perm or nlive is not 4-byte aligned", who);
    DLESM_REQUIRE((uintptr_t)scratch % 16 == 0, "%s: scratch is not 16-byte aligned", who);
    DLESM_REQUIRE(n >= 0 && n <= SORT_MAX_N, "%s: %lld particles (0..2^31-1)", who, n);
    DLESM_REQUIRE((long long)xstop >= (long long)xstart - 1 && (long long)ystop >= (long long)ystart - 1,
                  "%s: box %d..%d x %d..%d", who, xstart, xstop, ystart, ystop);
    const unsigned long long nxb = (unsigned long long)((long long)xstop - xstart + 1),
                             nyb = (unsigned long long)((long long)ystop - ystart + 1);
    DLESM_REQUIRE(nxb == 0 || nyb <= 0xfffffffeULL / nxb, "%s: a box of %llu x %llu cells (at most 2^32-2)", who, nxb, nyb);
    *ncells = (long long)(nxb * nyb);
    const size_t need = sort_plan(n).bytes;
    DLESM_REQUIRE(scratch_bytes >= 0 && (unsigned long long)scratch_bytes >= need,
                  "%s: %lld bytes of scratch, %zu needed (dlesm_particle_order_scratch)", who, scratch_bytes, need);
    const void *const ins[3] = {px, py, status};
    const size_t ib[3] = {(size_t)n * 8, (size_t)n * 8, (size_t)n * 4};
    const void *const outs[3] = {perm, nlive, scratch};
    const size_t ob[3] = {(size_t)n * 4, nlive ? (size_t)4 : 0, need};
    for (int k = 0; k < 3; k++) {
        if (!outs[k] || ob[k] == 0) continue;
        for (int m = 0; m < 3; m++)
            DLESM_REQUIRE(ib[m] == 0 || !overlap(outs[k], ob[k], ins[m], ib[m]), "%s: %s overlaps %s", who, out_name[k],
                          in_name[m]);
        for (int m = k + 1; m < 3; m++)
            DLESM_REQUIRE(!outs[m] || ob[m] == 0 || !overlap(outs[k], ob[k], outs[m], ob[m]), "%s: %s and %s overlap", who,
                          out_name[k], out_name[m]);
    }
    return DLESM_OK;
}

// the launches of dlesm_particle_order_f64, after check_order
int launch_order(int xstart, int xstop, int ystart, int ystop, long long n, long long ncells, const double *px, const double *py,
                 const int *status, int *perm, int *nlive, void *scratch, hipStream_t s)
{
    const dim3 block(SORT_BLOCK);
    if (n == 0 || ncells == 0) {
        if (n == 0 && !nlive) return DLESM_OK;
        const unsigned grid = n == 0 ? 1u : (unsigned)((n + SORT_BLOCK - 1) / SORT_BLOCK);
        hipLaunchKernelGGL(sort_identity_k, dim3(grid), block, 0, s, perm, n, nlive);
        DLESM_HIP_TRY(hipGetLastError());
        return DLESM_OK;
    }
    const SortPlan plan = sort_plan(n);
    char *const base = (char *)scratch;
    unsigned *const keys[2] = {(unsigned *)(base + plan.keys[0]), (unsigned *)(base + plan.keys[1])};
    unsigned *const vals[2] = {(unsigned *)perm, (unsigned *)(base + plan.vals)};
    unsigned *const table = (unsigned *)(base + plan.table), *const sums = (unsigned *)(base + plan.sums),
                   *const live = (unsigned *)(base + plan.live);
    const dim3 grid(plan.nblocks);
    const int passes = (bit_length((unsigned long long)ncells) + 7) / 8;       // 1..4: the dead key is ncells itself

    const KeyArgs ka{px, py, status, keys[0], table, live, n, cell_key(xstart, xstop, ystart, ystop, ncells), plan.nblocks};
    hipLaunchKernelGGL(sort_key_k, grid, block, 0, s, ka);
    if (nlive) hipLaunchKernelGGL(sort_nlive_k, dim3(1), block, 0, s, (const unsigned *)live, plan.nblocks, nlive);
    for (int pass = 0; pass < passes; pass++) {
        const bool last = pass == passes - 1;
        const unsigned *const kin = keys[pass & 1];
        if (pass > 0) hipLaunchKernelGGL(sort_hist_k, grid, block, 0, s, kin, table, n, plan.nblocks, 8 * pass);
        launch_scan(table, plan.m, plan.nscan, sums, s);
        // pass k writes perm when an even number of passes follow it, so that the last one does
        const int out = (passes - 1 - pass) & 1;
        const ScatterArgs sa{kin, pass == 0 ? nullptr : vals[out ^ 1], last ? nullptr : keys[(pass & 1) ^ 1], vals[out],
                             table, n, plan.nblocks, 8 * pass};
        hipLaunchKernelGGL(sort_scatter_k, grid, block, 0, s, sa);
    }
    DLESM_HIP_TRY(hipGetLastError());
    return DLESM_OK;
}

// every refusal of dlesm_particle_permute
int check_permute(const char *who, long long n, const int *perm, int narrays, const void *const *src, void *const *dst,
                  const int *elem_bytes)
{
    DLESM_REQUIRE(perm != nullptr && src != nullptr && dst != nullptr && elem_bytes != nullptr,
                  "%s: null perm, src, dst or elem_bytes", who);
    DLESM_REQUIRE((uintptr_t)perm % 4 == 0, "%s: perm is not 4-byte aligned", who);
    DLESM_REQUIRE(n >= 0 && n <= SORT_MAX_N, "%s: %lld particles (0..2^31-1)", who, n);
    DLESM_REQUIRE(narrays >= 1 && narrays <= PERMUTE_MAX, "%s: narrays = %d (1..%d)", who, narrays, PERMUTE_MAX);
    for (int k = 0; k < narrays; k++) {
        DLESM_REQUIRE(elem_bytes[k] == 4 || elem_bytes[k] == 8, "%s: elem_bytes[%d] = %d (4 or 8)", who, k, elem_bytes[k]);
        DLESM_REQUIRE(src[k] != nullptr && dst[k] != nullptr, "%s: null src[%d] or dst[%d]", who, k, k);
        DLESM_REQUIRE((uintptr_t)src[k] % (unsigned)elem_bytes[k] == 0 && (uintptr_t)dst[k] % (unsigned)elem_bytes[k] == 0,
                      "%s: src[%d] or dst[%d] is not %d-byte aligned", who, k, k, elem_bytes[k]);
    }
    for (int k = 0; k < narrays && n > 0; k++) {
        const size_t kb = (size_t)n * (size_t)elem_bytes[k];
        DLESM_REQUIRE(!overlap(dst[k], kb, perm, (size_t)n * 4), "%s: dst[%d] overlaps perm", who, k);
        for (int m = 0; m < narrays; m++) {
            const size_t mb = (size_t)n * (size_t)elem_bytes[m];
            DLESM_REQUIRE(!overlap(dst[k], kb, src[m], mb), "%s: dst[%d] overlaps src[%d]", who, k, m);
            DLESM_REQUIRE(m <= k || !overlap(dst[k], kb, dst[m], mb), "%s: dst[%d] and dst[%d] overlap", who, k, m);
        }
    }
    return DLESM_OK;
}

int launch_permute(long long n, const int *perm, int narrays, const void *const *src, void *const *dst, const int *elem_bytes,
                   hipStream_t s)
{
    if (n == 0) return DLESM_OK;
    PermuteArgs a{perm, n, {}, {}, {}, narrays};
    for (int k = 0; k < narrays; k++) a.src[k] = src[k], a.dst[k] = dst[k], a.elem_bytes[k] = elem_bytes[k];
    hipLaunchKernelGGL(permute_k, dim3((unsigned)((n + SORT_BLOCK - 1) / SORT_BLOCK)), dim3(SORT_BLOCK), 0, s, a);
    DLESM_HIP_TRY(hipGetLastError());
    return DLESM_OK;
}

} // namespace

} // namespace dlesm

using namespace dlesm;

extern "C" int dlesm_particle_order_scratch(long long n, long long *bytes)
{
    static const char *const who = "dlesm_particle_order_scratch";
    clear_error();
    DLESM_REQUIRE(bytes != nullptr, "%s: null bytes", who);
    DLESM_REQUIRE(n >= 0 && n <= SORT_MAX_N, "%s: %lld particles (0..2^31-1)", who, n);
    *bytes = (long long)sort_plan(n).bytes;
    return DLESM_OK;
}

extern "C" int dlesm_particle_order_f64(int xstart, int xstop, int ystart, int ystop, long long n, const double *px,
                                        const double *py, const int *status, int *perm, int *nlive, void *scratch,
                                        long long scratch_bytes, void *stream)
{
    static const char *const who = "dlesm_particle_order_f64";
    if (int rc = ensure_device()) return rc;
    long long ncells;
    if (int rc = check_order(who, xstart, xstop, ystart, ystop, n, px, py, status, perm, nlive, scratch, scratch_bytes, &ncells))
        return rc;
    return launch_order(xstart, xstop, ystart, ystop, n, ncells, px, py, status, perm, nlive, scratch, (hipStream_t)stream);
}

extern "C" int dlesm_particle_permute(long long n, const int *perm, int narrays, const void *const *src, void *const *dst,
                                      const int *elem_bytes, void *stream)
{
    if (int rc = ensure_device()) return rc;
    if (int rc = check_permute("dlesm_particle_permute", n, perm, narrays, src, dst, elem_bytes)) return rc;
    return launch_permute(n, perm, narrays, src, dst, elem_bytes, (hipStream_t)stream);
}

extern "C" int dlesm_particle_sort_set(dlesm_drifters *set, int xstart, int xstop, int ystart, int ystop, void *stream)
{
    static const char *const who = "dlesm_particle_sort_set";
    if (int rc = ensure_device()) return rc;
    if (int rc = drifters_ok(who, set)) return rc;
    const long long n = set->n;
    DLESM_REQUIRE(n <= SORT_MAX_N, "%s: %lld particles (0..2^31-1)", who, n);
    DLESM_REQUIRE((long long)xstop >= (long long)xstart - 1 && (long long)ystop >= (long long)ystart - 1,
                  "%s: box %d..%d x %d..%d", who, xstart, xstop, ystart, ystop);
    if (n == 0) return DLESM_OK;
    const size_t seconds = (size_t)n * 24, fours = ((size_t)n * 4 + 15) / 16 * 16;
    if (!set->sort_mem) {
        // px2 | py2 | status2 | origin2 (24 n bytes, 8-byte aligned pieces) | origin | perm | nlive | scratch
        const size_t need = sort_plan(n).bytes, head = (seconds + 15) / 16 * 16;
        void *mem = nullptr;
        if (hipMalloc(&mem, head + 2 * fours + 16 + need) != hipSuccess)
            return fail(DLESM_EHIP, "%s: no device memory to sort %lld particles", who, n);
        char *const at = (char *)mem;
        set->sort_mem = mem;
        set->origin = (int *)(at + head), set->perm = (int *)(at + head + fours), set->nlive = (int *)(at + head + 2 * fours);
        set->scratch = at + head + 2 * fours + 16, set->scratch_bytes = (long long)need;
    }
    double *const px2 = (double *)set->sort_mem, *const py2 = px2 + n;
    int *const st2 = (int *)(py2 + n), *const origin2 = st2 + n;
    hipStream_t s = (hipStream_t)stream;
    long long ncells;
    if (int rc = check_order(who, xstart, xstop, ystart, ystop, n, set->px, set->py, set->status, set->perm, set->nlive,
                             set->scratch, set->scratch_bytes, &ncells))
        return rc;
    if (int rc = launch_order(xstart, xstop, ystart, ystop, n, ncells, set->px, set->py, set->status, set->perm, set->nlive,
                              set->scratch, s))
        return rc;
    // an origin that is still the identity becomes perm itself
    const void *const src[4] = {set->px, set->py, set->status, set->origin};
    void *const dst[4] = {px2, py2, st2, origin2};
    const int eb[4] = {8, 8, 4, 4};
    if (int rc = launch_permute(n, set->perm, set->sorted ? 4 : 3, src, dst, eb, s)) return rc;
    DLESM_HIP_TRY(hipMemcpyAsync(set->px, px2, (size_t)n * 20, hipMemcpyDeviceToDevice, s));
    DLESM_HIP_TRY(hipMemcpyAsync(set->origin, set->sorted ? origin2 : set->perm, (size_t)n * 4, hipMemcpyDeviceToDevice, s));
    set->sorted = true;
    return DLESM_OK;
}

extern "C" int dlesm_particle_set_origin(dlesm_drifters *set, int *origin, long long *nlive)
{
    static const char *const who = "dlesm_particle_set_origin";
    if (int rc = ensure_device()) return rc;
    if (int rc = drifters_ok(who, set)) return rc;
    if (nlive) *nlive = set->n == 0 ? 0 : -1;
    if (!set->sorted) {                                  // no sort since the last put: the identity, nlive not known
        for (long long k = 0; origin && k < set->n; k++) origin[k] = (int)k;
        return DLESM_OK;
    }
    DLESM_HIP_TRY(hipDeviceSynchronize());               // sorts on any stream have landed
    if (origin) DLESM_HIP_TRY(hipMemcpy(origin, set->origin, (size_t)set->n * 4, hipMemcpyDeviceToHost));
    if (nlive) {
        int live = 0;
        DLESM_HIP_TRY(hipMemcpy(&live, set->nlive, 4, hipMemcpyDeviceToHost));
        *nlive = live;
    }
    return DLESM_OK;
}
