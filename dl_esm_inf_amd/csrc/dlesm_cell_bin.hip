// Particles binned by cell: per-cell sums of up to eight per-particle weights -- a null weight
// array counts -- over the slots of a permutation in key order, stored (DLESM_OUT_SET) or added with a factor
// (DLESM_OUT_ADD) into T-point fields, and the count for the owner of dlesm_drifter.hip.  The key rule is section 6.18's
// (CellKey, dlesm_particles.h).  In key order a cell's particles are one run of slots, so no cell is added to from two places.
//
// The sum of a run has a fixed order: the aligned groups of 64 slots are chunks; inside a chunk the run's slots are added one
// by one in slot order, beginning with the first; the chunks' partials are added one by one in chunk order, beginning with the
// first.  A chunk is a wave:
//   bin_fill_k   SET: alpha * 0.0 into every cell of the box, one cell per lane; it also zeroes the flag
//   bin_key_k    one slot per lane: the key of perm[k], stored to scratch; a lane whose predecessor's key is larger, or whose
//                index is outside 0..n-1 (key ncells: dead), raises the flag.  The predecessor's key comes by a wave shift;
//                lane 0 makes its own
//   bin_chunk_k  one chunk per wave, once per array: a lane that is not the head of its run adds its weight to the partial
//                of the lane before it, the lanes taking their turn in slot order (the partial comes over by v_readlane,
//                only the lanes that add take a turn).  A run that begins and ends in the chunk is written to its cell; the
//                partial of a run that came in from the chunk before goes to open[g], that of one that goes on into the next
//                chunk to close[g]; ckey[g] is the chunk's first key
//   bin_join_k   one chunk and one array per wave: where the chunk's last run began in it and goes on, close[g] + open[g+1]
//                + ... for as long as ckey says the run goes on, 64 chunks to a load -- the next load on its way --, added in
//                order by the wave as one; the cell
// A live key is below ncells and a cell offset is made of a live key alone, so whatever the order of the keys nothing is
// stored outside the box; every slot and chunk index is compared with n or nchunks before it is used.  Plain vector stores, no
// atomics, no LDS, no scratch memory; latency bound and small, so held at eight waves per SIMD.
#include <cmath>

#include "dlesm_particles.h"

namespace dlesm {

namespace {

using namespace nemo;

constexpr int BIN_BLOCK = 256;             // four waves
constexpr int BIN_WAVES = BIN_BLOCK / 64;
constexpr int BIN_MAX = 8;
constexpr long long BIN_MAX_N = 0x7fffffffLL;

#define BIN_KERNEL __global__ __launch_bounds__(BIN_BLOCK) __attribute__((amdgpu_waves_per_eu(8, 8))) void

struct BinArgs {
    const double *px, *py;
    const int *status, *perm;              // perm == nullptr: the identity
    const double *weights[BIN_MAX];        // nullptr: 1.0
    double *out[BIN_MAX];
    int *unordered;                        // may be nullptr
    unsigned *keys, *ckey;                 // scratch: n keys in slot order, the first key of each chunk
    double *open, *close;                  // scratch: [m * nchunks + g]
    long long n;
    CellKey cell;
    double alpha;
    unsigned nchunks;
    int narrays, add, ld, x0, y0;          // (x0, y0): the box's first cell, 0-based
};

// where the cell of a live key lies in a field
__device__ __forceinline__ size_t cell_offset(const BinArgs &a, unsigned key)
{
    return ((size_t)a.y0 + key / a.cell.nxb) * (size_t)a.ld + ((size_t)a.x0 + key % a.cell.nxb);
}

__device__ __forceinline__ void store_cell(const BinArgs &a, double *at, double sum)
{
    if (a.add) *at = *at + a.alpha * sum;
    else *at = a.alpha * sum;
}

// x of lane `from`, the same for the whole wave
__device__ __forceinline__ double from_lane(double x, int from)
{
    return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(x), from),
                            __builtin_amdgcn_readlane(__double2loint(x), from));
}

BIN_KERNEL bin_fill_k(const BinArgs a, int fill)
{
    const long long c = (long long)blockIdx.x * BIN_BLOCK + threadIdx.x;
    if (c == 0 && a.unordered) *a.unordered = 0;
    if (!fill || c >= (long long)a.cell.ncells) return;
    const size_t at = cell_offset(a, (unsigned)c);
    const double zero = a.alpha * 0.0;
    for (int m = 0; m < a.narrays; m++) a.out[m][at] = zero;
}

// the key of slot k < n; an index outside 0..n-1 is dead and bad
__device__ __forceinline__ unsigned slot_key(const BinArgs &a, long long k, bool &bad)
{
    const long long p = a.perm ? (long long)a.perm[k] : k;
    if (p < 0 || p >= a.n) {
        bad = true;
        return a.cell.ncells;
    }
    return a.cell.of(a.px[p], a.py[p], a.status[p]);
}

BIN_KERNEL bin_key_k(const BinArgs a)
{
    const long long k = (long long)blockIdx.x * BIN_BLOCK + threadIdx.x;
    const bool valid = k < a.n;
    bool bad = false;
    unsigned key = a.cell.ncells;
    if (valid) key = slot_key(a, k, bad);
    unsigned before = __shfl_up(key, 1);
    if ((threadIdx.x & 63) == 0) before = valid && k > 0 ? slot_key(a, k - 1, bad) : 0u;
    if (!valid) return;
    a.keys[k] = key;
    if (a.unordered && (bad || before > key)) *a.unordered = 1;
}

BIN_KERNEL bin_chunk_k(const BinArgs a)
{
    const int lane = threadIdx.x & 63;
    const long long g = (long long)blockIdx.x * BIN_WAVES + (threadIdx.x >> 6);
    if (g >= (long long)a.nchunks) return;
    const long long k = g * 64 + lane;
    const bool valid = k < a.n;                          // (lane 0 always is)
    const unsigned dead = a.cell.ncells;
    const unsigned key = valid ? a.keys[k] : dead;
    unsigned before = __shfl_up(key, 1), after = __shfl_down(key, 1);
    if (lane == 0) before = k > 0 ? a.keys[k - 1] : dead;
    if (lane == 63) after = k + 1 < a.n ? a.keys[k + 1] : dead;
    if (lane == 0) a.ckey[g] = key;

    const bool live = key < dead, head = before != key, tail = after != key;
    const unsigned long long heads = __ballot(live && head);
    if (__ballot(live) == 0) return;
    // the run of this lane came in from the chunk before: no head at or below the lane
    const bool came_in = (heads & ((2ull << lane) - 1ull)) == 0;
    // the lanes that add to the lane before them; lane 0 begins the chunk's partial whatever came before it
    const unsigned long long adders = __ballot(live && !head) & ~1ull;
    long long p = k;
    if (live && a.perm) p = a.perm[k];
    const bool mine = live && p >= 0 && p < a.n;
    const size_t at = live ? cell_offset(a, key) : 0;
    const bool ends = live && (tail || lane == 63);

    for (int m = 0; m < a.narrays; m++) {
        const double *const w = a.weights[m];
        double v = 1.0;
        if (w && mine) v = w[p];
        double sum = v;
        for (unsigned long long f = adders; f; f &= f - 1) {
            const int turn = __builtin_ctzll(f);
            const double lower = from_lane(sum, turn - 1);
            if (lane == turn) sum = lower + v;
        }
        if (!ends) continue;
        if (came_in) a.open[(size_t)m * a.nchunks + (size_t)g] = sum;
        else if (tail) store_cell(a, a.out[m] + at, sum);
        else a.close[(size_t)m * a.nchunks + (size_t)g] = sum;
    }
}

BIN_KERNEL bin_join_k(const BinArgs a)
{
    const int lane = threadIdx.x & 63, m = blockIdx.y;
    const long long g = (long long)blockIdx.x * BIN_WAVES + (threadIdx.x >> 6);
    if (g >= (long long)a.nchunks) return;
    const long long last = g * 64 + 63;
    if (last + 1 >= a.n) return;                         // no slot behind this chunk
    const unsigned c = a.keys[last];
    if (c >= a.cell.ncells || a.keys[last + 1] != c) return;          // the last run is the dead, or ends here
    if (g > 0 && a.ckey[g] == c && a.keys[last - 64] == c) return;    // it came in from the chunk before: that one's work
    const double *const open = a.open + (size_t)m * a.nchunks;
    double sum = a.close[(size_t)m * a.nchunks + (size_t)g];
    // this lane's chunk of the 64 that begin at `first`: does the run go on through it, and its opening partial (whatever
    // the scratch holds where it does not: never added)
    const auto load = [&](long long first, bool &on, double &part) {
        const long long h = first + lane;
        const bool there = h < (long long)a.nchunks;
        on = there && a.ckey[h] == c;
        part = there ? open[h] : 0.0;
    };
    bool on, on_next = false;
    double part, part_next = 0.0;
    load(g + 1, on, part);
    for (long long first = g + 1;; first += 64) {
        const bool more = first + 64 < (long long)a.nchunks;
        if (more) load(first + 64, on_next, part_next);  // on its way while this load's partials are added
        const unsigned long long stop = ~__ballot(on);
        if (stop == 0) {
#pragma unroll
            for (int i = 0; i < 64; i++) sum = sum + from_lane(part, i);
        } else {
            const int count = __builtin_ctzll(stop);     // the chunks of this load the run goes on through
            for (int i = 0; i < count; i++) sum = sum + from_lane(part, i);
        }
        if (stop != 0 || !more) break;
        on = on_next, part = part_next;
    }
    if (lane == 0) store_cell(a, a.out[m] + cell_offset(a, c), sum);
}

// ---- the host side

// where the pieces of the scratch lie (every piece 16-byte aligned)
struct BinPlan {
    unsigned nchunks;
    size_t keys, ckey, open, close, bytes;
};

BinPlan bin_plan(long long n, int narrays)
{
    BinPlan b{};
    b.nchunks = (unsigned)((n + 63) / 64);
    size_t at = 0;
    const auto piece = [&](size_t bytes) {
        const size_t here = at;
        at += (bytes + 15) / 16 * 16;
        return here;
    };
    b.keys = piece((size_t)n * 4), b.ckey = piece((size_t)b.nchunks * 4);
    b.open = piece((size_t)b.nchunks * 8 * (size_t)narrays), b.close = piece((size_t)b.nchunks * 8 * (size_t)narrays);
    b.bytes = at;
    return b;
}

// the refusals that concern the fields; *ncells = the box's cells
int check_fields(const char *who, int mode, double alpha, int ld, int ny, int xstart, int xstop, int ystart, int ystop,
                 int narrays, double *const *out, long long *ncells)
{
    DLESM_REQUIRE(mode == DLESM_OUT_SET || mode == DLESM_OUT_ADD, "%s: mode %d (DLESM_OUT_SET or DLESM_OUT_ADD)", who, mode);
    DLESM_REQUIRE(std::isfinite(alpha), "%s: alpha %g (a finite number)", who, alpha);
    DLESM_REQUIRE(narrays >= 1 && narrays <= BIN_MAX, "%s: narrays = %d (1..%d)", who, narrays, BIN_MAX);
    DLESM_REQUIRE(out != nullptr, "%s: null out", who);
    for (int m = 0; m < narrays; m++) {
        DLESM_REQUIRE(out[m] != nullptr, "%s: null out[%d]", who, m);
        DLESM_REQUIRE((uintptr_t)out[m] % 8 == 0, "%s: out[%d] is not 8-byte aligned", who, m);
    }
    DLESM_REQUIRE(ld >= 1 && ny >= 1, "%s: array extents %dx%d", who, ld, ny);
    DLESM_REQUIRE((long long)xstop >= (long long)xstart - 1 && (long long)ystop >= (long long)ystart - 1,
                  "%s: box %d..%d x %d..%d", who, xstart, xstop, ystart, ystop);
    const unsigned long long nxb = (unsigned long long)((long long)xstop - xstart + 1),
                             nyb = (unsigned long long)((long long)ystop - ystart + 1);
    if (nxb > 0 && nyb > 0)
        if (int rc = check_box(who, ld, ny, xstart, xstop, ystart, ystop, 0)) return rc;
    DLESM_REQUIRE(nxb == 0 || nyb <= 0xfffffffeULL / nxb, "%s: a box of %llu x %llu cells (at most 2^32-2)", who, nxb, nyb);
    *ncells = (long long)(nxb * nyb);
    const size_t fb = (size_t)ld * (size_t)ny * sizeof(double);
    for (int m = 0; m < narrays; m++)
        for (int q = m + 1; q < narrays; q++)
            DLESM_REQUIRE(!overlap(out[m], fb, out[q], fb), "%s: out[%d] and out[%d] overlap", who, m, q);
    return DLESM_OK;
}

// the refusals that concern the particles, the flag and the scratch, after check_fields
int check_particles(const char *who, int ld, int ny, long long n, const double *px, const double *py, const int *status,
                    const int *perm, int narrays, const double *const *weights, double *const *out, const int *unordered,
                    const void *scratch, long long scratch_bytes)
{
    DLESM_REQUIRE(px != nullptr && py != nullptr && status != nullptr, "%s: null px, py or status", who);
    DLESM_REQUIRE(weights != nullptr && scratch != nullptr, "%s: null weights or scratch", who);
    DLESM_REQUIRE(n >= 0 && n <= BIN_MAX_N, "%s: %lld particles (0..2^31-1)", who, n);
    DLESM_REQUIRE((uintptr_t)px % 8 == 0 && (uintptr_t)py % 8 == 0, "%s: px or py is not 8-byte aligned", who);
    DLESM_REQUIRE((uintptr_t)status % 4 == 0 && (uintptr_t)perm % 4 == 0 && (uintptr_t)unordered % 4 == 0,
                  "%s: status, perm or unordered is not 4-byte aligned", who);
    DLESM_REQUIRE((uintptr_t)scratch % 16 == 0, "%s: scratch is not 16-byte aligned", who);
    for (int m = 0; m < narrays; m++)
        DLESM_REQUIRE((uintptr_t)weights[m] % 8 == 0, "%s: weights[%d] is not 8-byte aligned", who, m);
    const size_t need = bin_plan(n, narrays).bytes;
    DLESM_REQUIRE(scratch_bytes >= 0 && (unsigned long long)scratch_bytes >= need,
                  "%s: %lld bytes of scratch, %zu needed (dlesm_cell_bin_scratch)", who, scratch_bytes, need);
    // what is written: the fields, the flag, the scratch; what is read: the particle arrays
    const size_t fb = (size_t)ld * (size_t)ny * sizeof(double);
    const void *wr[BIN_MAX + 2];
    size_t wb[BIN_MAX + 2];
    for (int m = 0; m < narrays; m++) wr[m] = out[m], wb[m] = fb;
    wr[narrays] = unordered, wb[narrays] = unordered ? 4 : 0;
    wr[narrays + 1] = scratch, wb[narrays + 1] = need;
    const void *rd[BIN_MAX + 4] = {px, py, status, perm};
    size_t rb[BIN_MAX + 4] = {(size_t)n * 8, (size_t)n * 8, (size_t)n * 4, perm ? (size_t)n * 4 : 0};
    for (int m = 0; m < narrays; m++) rd[4 + m] = weights[m], rb[4 + m] = weights[m] ? (size_t)n * 8 : 0;
    for (int k = 0; k < narrays + 2; k++) {
        if (wb[k] == 0) continue;
        for (int q = 0; q < narrays + 4; q++)
            DLESM_REQUIRE(rb[q] == 0 || !overlap(wr[k], wb[k], rd[q], rb[q]), "%s: %s overlaps an input", who,
                          k < narrays ? "an out array" : k == narrays ? "unordered" : "scratch");
        for (int q = narrays > k + 1 ? narrays : k + 1; q < narrays + 2; q++)
            DLESM_REQUIRE(wb[q] == 0 || !overlap(wr[k], wb[k], wr[q], wb[q]), "%s: %s overlaps %s", who,
                          k < narrays ? "an out array" : "unordered", q == narrays ? "unordered" : "scratch");
    }
    return DLESM_OK;
}

// the launches, after the checks; with n == 0 no particle array and no scratch is touched
int launch_bin(int mode, double alpha, int ld, int xstart, int xstop, int ystart, int ystop, long long ncells, long long n,
               const double *px, const double *py, const int *status, const int *perm, int narrays,
               const double *const *weights, double *const *out, int *unordered, void *scratch, hipStream_t s)
{
    const BinPlan plan = bin_plan(n, narrays);
    char *const base = (char *)scratch;
    BinArgs a{px, py, status, perm, {}, {}, unordered, (unsigned *)(base + plan.keys), (unsigned *)(base + plan.ckey),
              (double *)(base + plan.open), (double *)(base + plan.close), n, cell_key(xstart, xstop, ystart, ystop, ncells),
              alpha, plan.nchunks, narrays, mode == DLESM_OUT_ADD ? 1 : 0, ld, xstart - 1, ystart - 1};
    for (int m = 0; m < narrays; m++) a.weights[m] = weights ? weights[m] : nullptr, a.out[m] = out[m];
    const dim3 block(BIN_BLOCK);
    const auto blocks = [](long long items, long long each) { return dim3((unsigned)((items + each - 1) / each)); };
    const bool fill = mode == DLESM_OUT_SET && ncells > 0;
    if (fill || unordered) hipLaunchKernelGGL(bin_fill_k, blocks(fill ? ncells : 1, BIN_BLOCK), block, 0, s, a, fill ? 1 : 0);
    if (n > 0) {
        hipLaunchKernelGGL(bin_key_k, blocks(n, BIN_BLOCK), block, 0, s, a);
        if (ncells > 0) {
            hipLaunchKernelGGL(bin_chunk_k, blocks(plan.nchunks, BIN_WAVES), block, 0, s, a);
            if (plan.nchunks > 1) {
                const dim3 grid(blocks(plan.nchunks - 1, BIN_WAVES).x, (unsigned)narrays);
                hipLaunchKernelGGL(bin_join_k, grid, block, 0, s, a);
            }
        }
    }
    DLESM_HIP_TRY(hipGetLastError());
    return DLESM_OK;
}

} // namespace

} // namespace dlesm

using namespace dlesm;

extern "C" int dlesm_cell_bin_scratch(long long n, int narrays, long long *bytes)
{
    static const char *const who = "dlesm_cell_bin_scratch";
    clear_error();
    DLESM_REQUIRE(bytes != nullptr, "%s: null bytes", who);
    DLESM_REQUIRE(n >= 0 && n <= BIN_MAX_N, "%s: %lld particles (0..2^31-1)", who, n);
    DLESM_REQUIRE(narrays >= 1 && narrays <= BIN_MAX, "%s: narrays = %d (1..%d)", who, narrays, BIN_MAX);
    *bytes = (long long)bin_plan(n, narrays).bytes;
    return DLESM_OK;
}

extern "C" int dlesm_cell_bin_f64(int mode, double alpha, int ld, int ny, int xstart, int xstop, int ystart, int ystop,
                                  long long n, const double *px, const double *py, const int *status, const int *perm,
                                  int narrays, const double *const *weights, double *const *out, int *unordered,
                                  void *scratch, long long scratch_bytes, void *stream)
{
    static const char *const who = "dlesm_cell_bin_f64";
    if (int rc = ensure_device()) return rc;
    long long ncells;
    if (int rc = check_fields(who, mode, alpha, ld, ny, xstart, xstop, ystart, ystop, narrays, out, &ncells)) return rc;
    if (int rc = check_particles(who, ld, ny, n, px, py, status, perm, narrays, weights, out, unordered, scratch, scratch_bytes))
        return rc;
    return launch_bin(mode, alpha, ld, xstart, xstop, ystart, ystop, ncells, n, px, py, status, perm, narrays, weights, out,
                      unordered, scratch, (hipStream_t)stream);
}

extern "C" int dlesm_cell_bin_set(dlesm_drifters *set, int mode, double alpha, int ld, int ny, int xstart, int xstop,
                                  int ystart, int ystop, double *count, void *stream)
{
    static const char *const who = "dlesm_cell_bin_set";
    if (int rc = ensure_device()) return rc;
    if (int rc = drifters_ok(who, set)) return rc;
    const long long n = set->n;
    DLESM_REQUIRE(n <= BIN_MAX_N, "%s: %lld particles (0..2^31-1)", who, n);
    long long ncells;
    double *const out[1] = {count};
    if (int rc = check_fields(who, mode, alpha, ld, ny, xstart, xstop, ystart, ystop, 1, out, &ncells)) return rc;
    hipStream_t s = (hipStream_t)stream;
    if (n == 0)
        return launch_bin(mode, alpha, ld, xstart, xstop, ystart, ystop, ncells, 0, nullptr, nullptr, nullptr, nullptr, 1,
                          nullptr, out, nullptr, nullptr, s);
    long long order_bytes = 0;
    if (int rc = dlesm_particle_order_scratch(n, &order_bytes)) return rc;
    const size_t fours = ((size_t)n * 4 + 15) / 16 * 16, bin_bytes = bin_plan(n, 1).bytes;
    if (!set->bin_mem) {
        // perm | the order's scratch | the bin's scratch
        void *mem = nullptr;
        if (hipMalloc(&mem, fours + (size_t)order_bytes + bin_bytes) != hipSuccess)
            return fail(DLESM_EHIP, "%s: no device memory to bin %lld particles", who, n);
        set->bin_mem = mem;
    }
    char *const at = (char *)set->bin_mem;
    int *const perm = (int *)at;
    void *const bin_scratch = at + fours + (size_t)order_bytes;
    static const double *const no_weights[1] = {nullptr};
    if (int rc = check_particles(who, ld, ny, n, set->px, set->py, set->status, perm, 1, no_weights, out, nullptr, bin_scratch,
                                 (long long)bin_bytes))
        return rc;
    DLESM_REQUIRE(!overlap(count, (size_t)ld * (size_t)ny * 8, at, fours + (size_t)order_bytes),
                  "%s: count overlaps the set's buffers", who);
    if (int rc = dlesm_particle_order_f64(xstart, xstop, ystart, ystop, n, set->px, set->py, set->status, perm, nullptr,
                                          at + fours, order_bytes, stream))
        return rc;
    return launch_bin(mode, alpha, ld, xstart, xstop, ystart, ystop, ncells, n, set->px, set->py, set->status, perm, 1,
                      no_weights, out, nullptr, bin_scratch, s);
}
