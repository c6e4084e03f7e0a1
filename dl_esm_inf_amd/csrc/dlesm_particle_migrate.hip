// Particles that cross rank boundaries: the departures of one axis compacted into one message per
// direction, and the arrivals of one axis filled into the FREE slots, both stable and without atomics.  inbox is section
// 6.17's, the statuses are its numbers plus DLESM_DRIFTER_FREE.
//
// A block owns MIG_TILE consecutive slots in both kernels of a phase, a wave MIG_TILE / 4 consecutive ones of them, walked 64
// at a time in ascending order:
//   pack_count_k     status (4 B a slot; px and py only where a lane is LEFT) -> each wave's count of the two classes (the
//                    two directions of the axis) from ballots, left in wave_part; the block's two sums in the table
//   scan_*_k         one exclusive scan of the table, class-major, 2 x nblocks + 1 entries: entry (c, b) becomes the number
//                    of departures of class c in the blocks before b plus ALL of the classes before c, the last entry the
//                    total (dlesm_scan.h, shared with the sort)
//   pack_scatter_k   a lane's rank = popcount(ballot & lanes below) + the wave's earlier chunks + the waves before it
//                    (wave_part) + the block's base (table); rank < cap: the record is stored and the slot becomes FREE
//   unpack_count_k, unpack_fill_k   the same over one class, status == FREE: the j-th FREE slot takes arrival j
// A wave without a candidate (the common case: few particles leave per step) reads its two counts in the second kernel and
// leaves.  The headers and the counts record are written by thread 0 of block 0 of the second kernel.  Counts are exact
// integers, no global atomics, plain vector stores, no scratch memory; every kernel is latency bound and small, so all are held
// at eight waves per SIMD, as the sort's.
#include <cmath>

#include "dlesm_particles.h"

namespace dlesm {

namespace {

using namespace nemo;

#include "dlesm_scan.h"

constexpr int MIG_TILE = 4096;                     // slots of one block
constexpr int MIG_WAVES = SORT_BLOCK / 64;
constexpr int MIG_WAVE_TILE = MIG_TILE / MIG_WAVES; // consecutive slots of one wave
constexpr long long MIG_MAX_N = 0x7fffffffLL;
constexpr size_t MIG_HEADER = 16;                  // long long count + padding
constexpr int MAXP = DLESM_MIGRATE_MAX_PAYLOAD;

static_assert(sizeof(dlesm_migrate_counts) == 64, "dlesm_migrate_counts is 64 bytes");

// word k of array w (x, y, id, payload_0 ...) of a message of capacity cap
__device__ __forceinline__ uint64_t *msg_word(uint64_t *msg, long long cap, int w, long long k)
{
    return msg + MIG_HEADER / 8 + (size_t)w * (size_t)cap + (size_t)k;
}

struct PackArgs {
    const double *px, *py;
    int *status;
    const uint64_t *id;
    const uint64_t *payload[MAXP];
    int npayload;
    long long n;
    DrifterBox box;
    int axis;
    int has[2];                 // a neighbour on the low (W, S) and on the high (E, N) side
    double sx[2], sy[2];        // what a record's x and y gain on its way there
    long long cap;
    uint64_t *msg[2];
    unsigned *table, *wave_part;
    unsigned nblocks, m;
    dlesm_migrate_counts *counts;
};

// 0: stays; 1: leaves on the low side of the axis; 2: on the high side.  For a LEFT particle alone
__device__ __forceinline__ int pack_class(const PackArgs &a, double x, double y)
{
    if (!(fabs(x) < HUGE_VAL && fabs(y) < HUGE_VAL)) return 0;        // a NaN or an infinity
    int c = 0;
    if (a.axis == 0) {
        if (x < a.box.x_lo) c = a.has[0] ? 1 : 0;
        else if (x >= a.box.x_hi) c = a.has[1] ? 2 : 0;
    } else if (x >= a.box.x_lo && x < a.box.x_hi) {
        if (y < a.box.y_lo) c = a.has[0] ? 1 : 0;
        else if (y >= a.box.y_hi) c = a.has[1] ? 2 : 0;
    }
    return c;
}

SORT_KERNEL pack_count_k(const PackArgs a)
{
    __shared__ unsigned wlo[MIG_WAVES], whi[MIG_WAVES];
    const unsigned t = threadIdx.x, lane = t & 63, wave = t >> 6, b = blockIdx.x;
    const long long wfirst = (long long)b * MIG_TILE + (long long)wave * MIG_WAVE_TILE;
    unsigned nlo = 0, nhi = 0;                                         // of this wave, the same on every lane
    for (int c = 0; c < MIG_WAVE_TILE / 64 && wfirst + c * 64 < a.n; c++) {
        const long long p = wfirst + c * 64 + lane;
        const bool cand = p < a.n && a.status[p] == DLESM_DRIFTER_LEFT;
        if (__ballot(cand) == 0) continue;
        int cls = 0;
        if (cand) cls = pack_class(a, a.px[p], a.py[p]);
        nlo += (unsigned)__popcll(__ballot(cls == 1));
        nhi += (unsigned)__popcll(__ballot(cls == 2));
    }
    if (lane == 0) wlo[wave] = nlo, whi[wave] = nhi;
    if (b < a.nblocks && lane == 0) {
        a.wave_part[((size_t)b * MIG_WAVES + wave) * 2] = nlo;
        a.wave_part[((size_t)b * MIG_WAVES + wave) * 2 + 1] = nhi;
    }
    __syncthreads();
    if (b < a.nblocks && t == 0) {
        unsigned lo = 0, hi = 0;
        for (int w = 0; w < MIG_WAVES; w++) lo += wlo[w], hi += whi[w];
        a.table[b] = lo;
        a.table[(size_t)a.nblocks + b] = hi;
    }
    if (b == 0 && 2 * a.nblocks + t < a.m) a.table[2 * a.nblocks + t] = 0;        // the total's entry and the padding
}

SORT_KERNEL pack_scatter_k(const PackArgs a)
{
    const unsigned t = threadIdx.x, lane = t & 63, wave = t >> 6, b = blockIdx.x;
    const unsigned tot_lo = a.table[a.nblocks], tot_all = a.table[2 * a.nblocks];
    if (b < a.nblocks) {
        unsigned base_lo = a.table[b], base_hi = a.table[(size_t)a.nblocks + b] - tot_lo;
        const unsigned *const part = a.wave_part + (size_t)b * MIG_WAVES * 2;
        for (unsigned w = 0; w < wave; w++) base_lo += part[2 * w], base_hi += part[2 * w + 1];
        const long long wfirst = (long long)b * MIG_TILE + (long long)wave * MIG_WAVE_TILE;
        const bool any = part[2 * wave] + part[2 * wave + 1] != 0;
        for (int c = 0; any && c < MIG_WAVE_TILE / 64 && wfirst + c * 64 < a.n; c++) {
            const long long p = wfirst + c * 64 + lane;
            const bool cand = p < a.n && a.status[p] == DLESM_DRIFTER_LEFT;
            if (__ballot(cand) == 0) continue;
            int cls = 0;
            double x = 0.0, y = 0.0;
            if (cand) {
                x = a.px[p], y = a.py[p];
                cls = pack_class(a, x, y);
            }
            const unsigned long long blo = __ballot(cls == 1), bhi = __ballot(cls == 2);
            if (cls != 0) {
                const int d = cls - 1;
                const unsigned long long below = (1ull << lane) - 1ull;
                const long long k = (long long)(d ? base_hi : base_lo) + __popcll((d ? bhi : blo) & below);
                if (k < a.cap) {                                     // else held: nothing changes
                    uint64_t *const msg = a.msg[d];
                    *(double *)msg_word(msg, a.cap, 0, k) = x + a.sx[d];
                    *(double *)msg_word(msg, a.cap, 1, k) = y + a.sy[d];
                    *msg_word(msg, a.cap, 2, k) = a.id[p];
#pragma unroll
                    for (int q = 0; q < MAXP; q++)
                        if (q < a.npayload) *msg_word(msg, a.cap, 3 + q, k) = a.payload[q][p];
                    a.status[p] = DLESM_DRIFTER_FREE;
                }
            }
            base_lo += (unsigned)__popcll(blo), base_hi += (unsigned)__popcll(bhi);
        }
    }
    if (b == 0 && t == 0) {
        const long long dep[2] = {(long long)tot_lo, (long long)(tot_all - tot_lo)};
        for (int d = 0; d < 2; d++) {
            const long long sent = dep[d] < a.cap ? dep[d] : a.cap;
            *(long long *)a.msg[d] = sent;
            a.counts->sent[2 * a.axis + d] = (int)sent;
            a.counts->held[2 * a.axis + d] = (int)(dep[d] - sent);
        }
    }
}

struct UnpackArgs {
    double *px, *py;
    int *status;
    uint64_t *id;
    uint64_t *payload[MAXP];
    int npayload;
    long long n;
    DrifterBox box;
    int axis;
    long long cap;
    const uint64_t *msg[2];
    unsigned *table, *wave_part;
    unsigned nblocks, m;
    dlesm_migrate_counts *counts;
};

// the two headers' counts; one outside 0..cap counts as 0 and sets its direction's bit of *bad
__device__ __forceinline__ void arrivals(const UnpackArgs &a, long long (&c)[2], int &bad)
{
    bad = 0;
    for (int d = 0; d < 2; d++) {
        c[d] = *(const long long *)a.msg[d];
        if (c[d] < 0 || c[d] > a.cap) c[d] = 0, bad |= 1 << (2 * a.axis + d);
    }
}

SORT_KERNEL unpack_count_k(const UnpackArgs a)
{
    __shared__ unsigned wfree[MIG_WAVES];
    const unsigned t = threadIdx.x, lane = t & 63, wave = t >> 6, b = blockIdx.x;
    const long long wfirst = (long long)b * MIG_TILE + (long long)wave * MIG_WAVE_TILE;
    unsigned nfree = 0;
    for (int c = 0; c < MIG_WAVE_TILE / 64 && wfirst + c * 64 < a.n; c++) {
        const long long p = wfirst + c * 64 + lane;
        nfree += (unsigned)__popcll(__ballot(p < a.n && a.status[p] == DLESM_DRIFTER_FREE));
    }
    if (lane == 0) wfree[wave] = nfree;
    if (b < a.nblocks && lane == 0) a.wave_part[(size_t)b * MIG_WAVES + wave] = nfree;
    __syncthreads();
    if (b < a.nblocks && t == 0) {
        unsigned s = 0;
        for (int w = 0; w < MIG_WAVES; w++) s += wfree[w];
        a.table[b] = s;
    }
    if (b == 0 && a.nblocks + t < a.m) a.table[a.nblocks + t] = 0;
}

SORT_KERNEL unpack_fill_k(const UnpackArgs a)
{
    const unsigned t = threadIdx.x, lane = t & 63, wave = t >> 6, b = blockIdx.x;
    long long cnt[2];
    int bad;
    arrivals(a, cnt, bad);
    const long long all = cnt[0] + cnt[1];
    if (b < a.nblocks) {
        long long base = a.table[b];
        const unsigned *const part = a.wave_part + (size_t)b * MIG_WAVES;
        for (unsigned w = 0; w < wave; w++) base += part[w];
        const long long wfirst = (long long)b * MIG_TILE + (long long)wave * MIG_WAVE_TILE;
        const bool any = part[wave] != 0;
        for (int c = 0; any && base < all && c < MIG_WAVE_TILE / 64 && wfirst + c * 64 < a.n; c++) {
            const long long p = wfirst + c * 64 + lane;
            const bool fr = p < a.n && a.status[p] == DLESM_DRIFTER_FREE;
            const unsigned long long bal = __ballot(fr);
            if (bal == 0) continue;
            const long long j = base + __popcll(bal & ((1ull << lane) - 1ull));
            if (fr && j < all) {
                const int d = j >= cnt[0];
                const long long k = d ? j - cnt[0] : j;              // 0 <= k < cnt[d] <= cap
                uint64_t *const msg = const_cast<uint64_t *>(a.msg[d]);
                const double x = *(const double *)msg_word(msg, a.cap, 0, k), y = *(const double *)msg_word(msg, a.cap, 1, k);
                a.px[p] = x, a.py[p] = y;
                a.id[p] = *msg_word(msg, a.cap, 2, k);
#pragma unroll
                for (int q = 0; q < MAXP; q++)
                    if (q < a.npayload) a.payload[q][p] = *msg_word(msg, a.cap, 3 + q, k);
                a.status[p] = a.box.has(x, y) ? DLESM_DRIFTER_ACTIVE : DLESM_DRIFTER_LEFT;
            }
            base += __popcll(bal);
        }
    }
    if (b == 0 && t == 0) {
        const long long nfree = a.table[a.nblocks];                  // scanned: all FREE slots
        const long long a0 = cnt[0] < nfree ? cnt[0] : nfree, a1 = cnt[1] < nfree - a0 ? cnt[1] : nfree - a0;
        const int dropped = (int)(all - a0 - a1);
        a.counts->arrived[2 * a.axis] = (int)a0;
        a.counts->arrived[2 * a.axis + 1] = (int)a1;
        if (a.axis == 0) {
            a.counts->dropped = dropped, a.counts->bad_message = bad, a.counts->pad = 0;
        } else {
            a.counts->dropped += dropped, a.counts->bad_message |= bad;
        }
        a.counts->nfree = (int)(nfree - a0 - a1);
    }
}

// ---- the host side

// where the pieces of the scratch lie, for n slots (every piece 16-byte aligned); the table is sized for the pack's two classes
struct MigPlan {
    unsigned nblocks, m[2], nscan[2];          // [0]: the pack's table, [1]: the unpack's
    size_t table, sums, wave_part, bytes;
};

MigPlan mig_plan(long long n)
{
    MigPlan s{};
    const auto up16 = [](size_t b) { return (b + 15) / 16 * 16; };
    s.nblocks = (unsigned)((n + MIG_TILE - 1) / MIG_TILE);
    for (int k = 0; k < 2; k++) {
        s.m[k] = ((2 - k) * s.nblocks + 1 + SCAN_ITEMS - 1) / SCAN_ITEMS * SCAN_ITEMS;
        s.nscan[k] = (s.m[k] + SCAN_TILE - 1) / SCAN_TILE;
    }
    size_t at = 0;
    const auto piece = [&](size_t b) {
        const size_t here = at;
        at += up16(b);
        return here;
    };
    s.table = piece((size_t)s.m[0] * 4), s.sums = piece((size_t)s.nscan[0] * 4);
    s.wave_part = piece((size_t)s.nblocks * MIG_WAVES * 2 * 4);
    s.bytes = at;
    return s;
}

size_t message_bytes(long long cap, int npayload) { return MIG_HEADER + (size_t)(3 + npayload) * 8 * (size_t)cap; }

struct Span {
    const void *p;
    size_t bytes;
    bool out;
    const char *name;
};

// no output may share a byte with any other array
int disjoint(const char *who, const Span *s, int ns)
{
    for (int k = 0; k < ns; k++)
        for (int m = 0; m < k; m++)
            DLESM_REQUIRE(!(s[k].out || s[m].out) || s[k].bytes == 0 || s[m].bytes == 0 ||
                              !overlap(s[k].p, s[k].bytes, s[m].p, s[m].bytes),
                          "%s: %s and %s overlap", who, s[m].name, s[k].name);
    return DLESM_OK;
}

const char *const payload_name[MAXP] = {"payload[0]", "payload[1]", "payload[2]", "payload[3]"};

// what pack, unpack and the whole migration refuse alike; *nspans spans of the particle arrays and the record are left in s
int check_particles(const char *who, int xstart, int xstop, int ystart, int ystop, long long n, const void *px, const void *py,
                    const void *status, const void *id, const void *const *payload, int npayload, long long cap,
                    const void *counts, bool arrays_out, Span *s, int *nspans)
{
    DLESM_REQUIRE(px != nullptr && py != nullptr && status != nullptr && id != nullptr, "%s: null px, py, status or id", who);
    DLESM_REQUIRE(counts != nullptr, "%s: null counts", who);
    DLESM_REQUIRE(npayload >= 0 && npayload <= MAXP, "%s: npayload = %d (0..%d)", who, npayload, MAXP);
    DLESM_REQUIRE(npayload == 0 || payload != nullptr, "%s: null payload", who);
    DLESM_REQUIRE((uintptr_t)px % 8 == 0 && (uintptr_t)py % 8 == 0 && (uintptr_t)id % 8 == 0,
                  "%s: px, py or id is not 8-byte aligned", who);
    DLESM_REQUIRE((uintptr_t)status % 4 == 0 && (uintptr_t)counts % 4 == 0, "%s: status or counts is not 4-byte aligned", who);
    for (int k = 0; k < npayload; k++)
        DLESM_REQUIRE(payload[k] != nullptr && (uintptr_t)payload[k] % 8 == 0, "%s: payload[%d] is null or not 8-byte aligned",
                      who, k);
    DLESM_REQUIRE(n >= 0 && n <= MIG_MAX_N, "%s: %lld slots (0..2^31-1)", who, n);
    DLESM_REQUIRE(cap >= 1 && cap <= MIG_MAX_N, "%s: cap = %lld (1..2^31-1)", who, cap);
    DLESM_REQUIRE((long long)xstop >= (long long)xstart - 1 && (long long)ystop >= (long long)ystart - 1,
                  "%s: box %d..%d x %d..%d", who, xstart, xstop, ystart, ystop);
    int k = 0;
    s[k++] = Span{px, (size_t)n * 8, arrays_out, "px"};
    s[k++] = Span{py, (size_t)n * 8, arrays_out, "py"};
    s[k++] = Span{status, (size_t)n * 4, true, "status"};
    s[k++] = Span{id, (size_t)n * 8, arrays_out, "id"};
    for (int q = 0; q < npayload; q++) s[k++] = Span{payload[q], (size_t)n * 8, arrays_out, payload_name[q]};
    s[k++] = Span{counts, sizeof(dlesm_migrate_counts), true, "counts"};
    *nspans = k;
    return DLESM_OK;
}

constexpr int MAX_SPANS = 5 + MAXP + 3;

// ... and the messages and the scratch of one phase
int check_phase(const char *who, int axis, const void *const *msg, bool msg_out, const char *const (&msg_name)[2], long long cap,
                int npayload, long long n, const void *scratch, long long scratch_bytes, Span *s, int ns)
{
    DLESM_REQUIRE(axis == DLESM_MIGRATE_X || axis == DLESM_MIGRATE_Y, "%s: axis = %d (0 or 1)", who, axis);
    DLESM_REQUIRE(msg != nullptr && msg[0] != nullptr && msg[1] != nullptr, "%s: null %s or %s", who, msg_name[0], msg_name[1]);
    DLESM_REQUIRE((uintptr_t)msg[0] % 16 == 0 && (uintptr_t)msg[1] % 16 == 0, "%s: %s or %s is not 16-byte aligned", who,
                  msg_name[0], msg_name[1]);
    DLESM_REQUIRE(scratch != nullptr && (uintptr_t)scratch % 16 == 0, "%s: scratch is null or not 16-byte aligned", who);
    const size_t need = mig_plan(n).bytes;
    DLESM_REQUIRE(scratch_bytes >= 0 && (unsigned long long)scratch_bytes >= need,
                  "%s: %lld bytes of scratch, %zu needed (dlesm_migrate_scratch)", who, scratch_bytes, need);
    const size_t mb = message_bytes(cap, npayload);
    s[ns++] = Span{msg[0], mb, msg_out, msg_name[0]};
    s[ns++] = Span{msg[1], mb, msg_out, msg_name[1]};
    s[ns++] = Span{scratch, need, true, "scratch"};
    return disjoint(who, s, ns);
}

int launch_pack(int axis, int xstart, int xstop, int ystart, int ystop, long long n, const double *px, const double *py,
                int *status, const long long *id, const void *const *payload, int npayload, const int *has_neighbour,
                const int *shift_x, const int *shift_y, long long cap, void *const *send, dlesm_migrate_counts *counts,
                void *scratch, hipStream_t s)
{
    const MigPlan plan = mig_plan(n);
    char *const base = (char *)scratch;
    PackArgs a{};
    a.px = px, a.py = py, a.status = status, a.id = (const uint64_t *)id, a.npayload = npayload, a.n = n;
    for (int q = 0; q < npayload; q++) a.payload[q] = (const uint64_t *)payload[q];
    a.box = drifter_box(xstart, xstop, ystart, ystop), a.axis = axis, a.cap = cap;
    for (int d = 0; d < 2; d++) {
        a.has[d] = has_neighbour[d] != 0, a.sx[d] = (double)shift_x[d], a.sy[d] = (double)shift_y[d];
        a.msg[d] = (uint64_t *)send[d];
    }
    a.table = (unsigned *)(base + plan.table), a.wave_part = (unsigned *)(base + plan.wave_part);
    a.nblocks = plan.nblocks, a.m = plan.m[0], a.counts = counts;
    const dim3 grid(plan.nblocks ? plan.nblocks : 1u), block(SORT_BLOCK);
    hipLaunchKernelGGL(pack_count_k, grid, block, 0, s, a);
    launch_scan(a.table, a.m, plan.nscan[0], (unsigned *)(base + plan.sums), s);
    hipLaunchKernelGGL(pack_scatter_k, grid, block, 0, s, a);
    DLESM_HIP_TRY(hipGetLastError());
    return DLESM_OK;
}

int launch_unpack(int axis, int xstart, int xstop, int ystart, int ystop, long long n, double *px, double *py, int *status,
                  long long *id, void *const *payload, int npayload, long long cap, const void *const *recv,
                  dlesm_migrate_counts *counts, void *scratch, hipStream_t s)
{
    const MigPlan plan = mig_plan(n);
    char *const base = (char *)scratch;
    UnpackArgs a{};
    a.px = px, a.py = py, a.status = status, a.id = (uint64_t *)id, a.npayload = npayload, a.n = n;
    for (int q = 0; q < npayload; q++) a.payload[q] = (uint64_t *)payload[q];
    a.box = drifter_box(xstart, xstop, ystart, ystop), a.axis = axis, a.cap = cap;
    for (int d = 0; d < 2; d++) a.msg[d] = (const uint64_t *)recv[d];
    a.table = (unsigned *)(base + plan.table), a.wave_part = (unsigned *)(base + plan.wave_part);
    a.nblocks = plan.nblocks, a.m = plan.m[1], a.counts = counts;
    const dim3 grid(plan.nblocks ? plan.nblocks : 1u), block(SORT_BLOCK);
    hipLaunchKernelGGL(unpack_count_k, grid, block, 0, s, a);
    launch_scan(a.table, a.m, plan.nscan[1], (unsigned *)(base + plan.sums), s);
    hipLaunchKernelGGL(unpack_fill_k, grid, block, 0, s, a);
    DLESM_HIP_TRY(hipGetLastError());
    return DLESM_OK;
}

const char *const send_name[2] = {"send[0]", "send[1]"};
const char *const recv_name[2] = {"recv[0]", "recv[1]"};

// the work area of dlesm_migrate_f64: send W, E, S, N | recv W, E, S, N | scratch, every piece 16-byte aligned
struct WorkPlan {
    size_t msg, scratch, scratch_bytes, bytes;         // msg: the bytes from one message to the next
};

WorkPlan work_plan(long long n, long long cap, int npayload)
{
    WorkPlan w{};
    w.msg = (message_bytes(cap, npayload) + 15) / 16 * 16;
    w.scratch = 8 * w.msg;
    w.scratch_bytes = mig_plan(n).bytes;
    w.bytes = w.scratch + w.scratch_bytes;
    return w;
}

} // namespace

} // namespace dlesm

using namespace dlesm;

extern "C" int dlesm_migrate_bytes(long long cap, int npayload, long long *bytes)
{
    static const char *const who = "dlesm_migrate_bytes";
    clear_error();
    DLESM_REQUIRE(bytes != nullptr, "%s: null bytes", who);
    DLESM_REQUIRE(cap >= 1 && cap <= MIG_MAX_N, "%s: cap = %lld (1..2^31-1)", who, cap);
    DLESM_REQUIRE(npayload >= 0 && npayload <= MAXP, "%s: npayload = %d (0..%d)", who, npayload, MAXP);
    *bytes = (long long)message_bytes(cap, npayload);
    return DLESM_OK;
}

extern "C" int dlesm_migrate_scratch(long long n, long long *bytes)
{
    static const char *const who = "dlesm_migrate_scratch";
    clear_error();
    DLESM_REQUIRE(bytes != nullptr, "%s: null bytes", who);
    DLESM_REQUIRE(n >= 0 && n <= MIG_MAX_N, "%s: %lld slots (0..2^31-1)", who, n);
    *bytes = (long long)mig_plan(n).bytes;
    return DLESM_OK;
}

extern "C" int dlesm_migrate_work(long long n, long long cap, int npayload, long long *bytes)
{
    static const char *const who = "dlesm_migrate_work";
    clear_error();
    DLESM_REQUIRE(bytes != nullptr, "%s: null bytes", who);
    DLESM_REQUIRE(n >= 0 && n <= MIG_MAX_N, "%s: %lld slots (0..2^31-1)", who, n);
    DLESM_REQUIRE(cap >= 1 && cap <= MIG_MAX_N, "%s: cap = %lld (1..2^31-1)", who, cap);
    DLESM_REQUIRE(npayload >= 0 && npayload <= MAXP, "%s: npayload = %d (0..%d)", who, npayload, MAXP);
    *bytes = (long long)work_plan(n, cap, npayload).bytes;
    return DLESM_OK;
}

extern "C" int dlesm_migrate_pack_f64(int axis, int xstart, int xstop, int ystart, int ystop, long long n, const double *px,
                                      const double *py, int *status, const long long *id, const void *const *payload,
                                      int npayload, const int *has_neighbour, const int *shift_x, const int *shift_y,
                                      long long cap, void *const *send, dlesm_migrate_counts *counts, void *scratch,
                                      long long scratch_bytes, void *stream)
{
    static const char *const who = "dlesm_migrate_pack_f64";
    if (int rc = ensure_device()) return rc;
    Span spans[MAX_SPANS];
    int ns;
    if (int rc = check_particles(who, xstart, xstop, ystart, ystop, n, px, py, status, id, payload, npayload, cap, counts, false,
                                 spans, &ns))
        return rc;
    DLESM_REQUIRE(has_neighbour != nullptr && shift_x != nullptr && shift_y != nullptr,
                  "%s: null has_neighbour, shift_x or shift_y", who);
    if (int rc = check_phase(who, axis, send, true, send_name, cap, npayload, n, scratch, scratch_bytes, spans, ns)) return rc;
    return launch_pack(axis, xstart, xstop, ystart, ystop, n, px, py, status, id, payload, npayload, has_neighbour, shift_x,
                       shift_y, cap, send, counts, scratch, (hipStream_t)stream);
}

extern "C" int dlesm_migrate_unpack_f64(int axis, int xstart, int xstop, int ystart, int ystop, long long n, double *px,
                                        double *py, int *status, long long *id, void *const *payload, int npayload,
                                        long long cap, const void *const *recv, dlesm_migrate_counts *counts, void *scratch,
                                        long long scratch_bytes, void *stream)
{
    static const char *const who = "dlesm_migrate_unpack_f64";
    if (int rc = ensure_device()) return rc;
    Span spans[MAX_SPANS];
    int ns;
    if (int rc = check_particles(who, xstart, xstop, ystart, ystop, n, px, py, status, id, payload, npayload, cap, counts, true,
                                 spans, &ns))
        return rc;
    if (int rc = check_phase(who, axis, recv, false, recv_name, cap, npayload, n, scratch, scratch_bytes, spans, ns)) return rc;
    return launch_unpack(axis, xstart, xstop, ystart, ystop, n, px, py, status, id, payload, npayload, cap, recv, counts, scratch,
                         (hipStream_t)stream);
}

extern "C" int dlesm_migrate_f64(int xstart, int xstop, int ystart, int ystop, long long n, double *px, double *py, int *status,
                                 long long *id, void *const *payload, int npayload, const int *neighbour, const int *shift_x,
                                 const int *shift_y, long long cap, dlesm_migrate_counts *counts, void *work,
                                 long long work_bytes, void *stream)
{
    static const char *const who = "dlesm_migrate_f64";
    if (int rc = ensure_device()) return rc;
    Span spans[MAX_SPANS];
    int ns;
    if (int rc = check_particles(who, xstart, xstop, ystart, ystop, n, px, py, status, id, payload, npayload, cap, counts, true,
                                 spans, &ns))
        return rc;
    DLESM_REQUIRE(neighbour != nullptr && shift_x != nullptr && shift_y != nullptr, "%s: null neighbour, shift_x or shift_y",
                  who);
    DLESM_REQUIRE(work != nullptr && (uintptr_t)work % 16 == 0, "%s: work is null or not 16-byte aligned", who);
    const WorkPlan w = work_plan(n, cap, npayload);
    DLESM_REQUIRE(work_bytes >= 0 && (unsigned long long)work_bytes >= w.bytes,
                  "%s: %lld bytes of work area, %zu needed (dlesm_migrate_work)", who, work_bytes, w.bytes);
    spans[ns++] = Span{work, w.bytes, true, "work"};
    if (int rc = disjoint(who, spans, ns)) return rc;
    hipStream_t s = (hipStream_t)stream;
    char *const base = (char *)work;
    const long long bytes = (long long)message_bytes(cap, npayload);
    for (int axis = 0; axis < 2; axis++) {
        void *const send[2] = {base + (2 * axis) * w.msg, base + (2 * axis + 1) * w.msg};
        void *const recv[2] = {base + (4 + 2 * axis) * w.msg, base + (4 + 2 * axis + 1) * w.msg};
        const int has[2] = {neighbour[2 * axis] >= 0, neighbour[2 * axis + 1] >= 0};
        if (int rc = launch_pack(axis, xstart, xstop, ystart, ystop, n, px, py, status, id, payload, npayload, has,
                                 shift_x + 2 * axis, shift_y + 2 * axis, cap, send, counts, base + w.scratch, s))
            return rc;
        if (int rc = dlesm_migrate_exchange(neighbour + 2 * axis, send, recv, bytes, stream)) return rc;
        if (int rc = launch_unpack(axis, xstart, xstop, ystart, ystop, n, px, py, status, id, payload, npayload, cap, recv, counts,
                                   base + w.scratch, s))
            return rc;
    }
    return DLESM_OK;
}
