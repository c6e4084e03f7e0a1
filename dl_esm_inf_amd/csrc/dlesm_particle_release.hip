// Particle sources that fill FREE slots: two stable, atomic-free compactions that meet.  The
// candidates of every source -- positions from Philox by id and seed alone, the exact owner test, one mask gather -- are
// compacted source-major into a staging area; the FREE slots are counted as section 6.21's unpack counts them; the j-th FREE
// slot takes staged record j.  inbox, the statuses and DrifterBox are section 6.17's, the generator and philox_sym section
// 6.20's, the scan dlesm_scan.h's.
//
// A candidate block owns REL_CHUNK consecutive m of one source, a wave 64 of them; a slot block REL_TILE consecutive slots, a
// wave REL_TILE / 4 of them walked 64 at a time in ascending order:
//   count_k        one launch for both sides, the candidate blocks first.  A candidate block: a lane's class (accepted ACTIVE,
//                  accepted LEFT, foreign, on land) from the rule; each wave's accepted count from a ballot, left in cand_part;
//                  the block's four sums -- accepted, foreign, on land, edge -- in the table; a block whose source wants
//                  nothing of its chunk stores zeros after one load of the source.  A slot block: status == FREE per wave in
//                  slot_part, per block in the table; the first clears the total's entry and the padding
//   scan_*_k       one exclusive scan of the ONE table, class-major: accepted x ncand | foreign x ncand | on land x ncand |
//                  edge x ncand | FREE x nblocks | total.  The entry at the head of a class is the sum of all classes before it,
//                  so the five totals are differences of five entries.  The sums may pass 2^32 (n FREE slots beside 2^31
//                  candidates); every difference taken is below 2^32 and unsigned arithmetic gives it exactly
//   stage_k        the class again (one Philox is cheaper than five words of traffic), a lane's rank = the block's base + the
//                  waves before it + popcount(ballot & lanes below); rank < the number of FREE slots: the record is staged
//   fill_k         section 6.21's unpack_fill_k over the staging area: the j-th FREE slot takes record j.  Its last block fills
//                  nothing: next_id += c_s, behind stage_k, the last reader of it; requested, clamped, bad_source reduced
//                  over the sources; thread 0 stores the whole record
// Four launches, six where the table is more than one scan block.  Counts are exact integers, no global atomics, plain vector stores, no scratch memory; every kernel is latency bound and
// small, so all are held at eight waves per SIMD, as the sort's and the migration's.
#include <cmath>

#include "dlesm_particles.h"

namespace dlesm {

namespace {

using namespace nemo;

#include "dlesm_scan.h"

constexpr int REL_CHUNK = SORT_BLOCK;               // candidates of one block: one a lane
constexpr int REL_TILE = 4096;                      // slots of one block
constexpr int REL_WAVES = SORT_BLOCK / 64;
constexpr int REL_WAVE_TILE = REL_TILE / REL_WAVES; // consecutive slots of one wave
constexpr long long REL_MAX_N = 0x7fffffffLL;
constexpr long long REL_MAX_BLOCKS = 1LL << 22;     // candidate blocks of one call
constexpr int REL_CLASSES = 4;                      // accepted, foreign, on land, edge

static_assert(sizeof(dlesm_release_source) == 64, "dlesm_release_source is 64 bytes");
static_assert(sizeof(dlesm_release_counts) == 64, "dlesm_release_counts is 64 bytes");

enum { CAND_IDLE = 0, CAND_ACTIVE, CAND_LEFT, CAND_FOREIGN, CAND_LAND };

// the staging area: x[cap] | y[cap] | id[cap] | tag[cap] | status[cap], cap = min(n, nsources * max_count) records
struct Stage {
    double *x, *y;
    uint64_t *id, *tag;
    int *status;
};

struct ReleaseArgs {
    const int *tmask;
    dlesm_release_source *sources;
    int ld, nsources, max_count;
    unsigned nchunks, ncand, nblocks, m;      // chunks of a source, candidate blocks, slot blocks, table entries
    DrifterBox box;                           // local
    double gx_lo, gx_hi, gy_lo, gy_hi;        // the box in global coordinates
    double offx, offy;
    unsigned k0, k1;
    long long tick;
    const long long *tick_dev;
    long long n;
    double *px, *py;
    int *status;
    uint64_t *id, *tag, *born;
    dlesm_release_counts *counts;
    unsigned *table, *cand_part, *slot_part;
    Stage stage;
    __device__ __forceinline__ unsigned head(int cls) const { return table[(size_t)cls * ncand]; }
    __device__ __forceinline__ unsigned free_head() const { return table[(size_t)REL_CLASSES * ncand]; }
    __device__ __forceinline__ unsigned all_free() const { return table[(size_t)REL_CLASSES * ncand + nblocks] - free_head(); }
    __device__ __forceinline__ unsigned accepted() const { return head(1) - head(0); }
};

__device__ __forceinline__ bool finite(double v) { return fabs(v) < HUGE_VAL; }

// c_s: what source s gives at this call; *bad: the source is invalid, *clamped: it wanted more than max_count
__device__ __forceinline__ long long source_count(const dlesm_release_source &s, int max_count, bool *bad, bool *clamped)
{
    const bool valid = finite(s.x) && finite(s.y) && finite(s.rx) && finite(s.ry) && s.rx >= 0.0 && s.ry >= 0.0 && s.count >= 0;
    *bad = !valid;
    *clamped = valid && s.count > (long long)max_count;
    return !valid ? 0 : *clamped ? (long long)max_count : s.count;
}

struct Candidate {
    double lx, ly;
    uint64_t id;
    int cls;
};

// candidate m of source s, m < c_s: the rule of section 6.23 in the order it is written
__device__ __forceinline__ Candidate candidate(const ReleaseArgs &a, const dlesm_release_source &s, unsigned m)
{
    Candidate c;
    c.id = (uint64_t)s.next_id + (uint64_t)m;
    const Philox4 w = philox4x32_10((unsigned)c.id, 1u, (unsigned)(c.id >> 32), 0u, a.k0, a.k1);
    const double gx = s.x + s.rx * philox_sym(w.w[0]), gy = s.y + s.ry * philox_sym(w.w[1]);
    c.lx = gx - a.offx, c.ly = gy - a.offy;
    c.cls = CAND_FOREIGN;
    if (finite(gx) && finite(gy) && gx >= a.gx_lo && gx < a.gx_hi && gy >= a.gy_lo && gy < a.gy_hi) {
        c.cls = CAND_LEFT;
        if (a.box.has(c.lx, c.ly)) {          // the cast and the gather stand behind inbox: a cell of the box
            const int i = (int)floor(c.lx), j = (int)floor(c.ly);
            const int t = a.tmask[(size_t)(j - 1) * (size_t)a.ld + (size_t)(i - 1)];
            c.cls = t != 0 ? CAND_ACTIVE : CAND_LAND;
        }
    }
    return c;
}

// the candidate side of the count: block b of ncand
__device__ __forceinline__ void cand_count(const ReleaseArgs &a, unsigned b)
{
    __shared__ unsigned part[REL_WAVES][REL_CLASSES];
    const unsigned t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const unsigned s = b / a.nchunks, m = (b % a.nchunks) * REL_CHUNK + t;
    const dlesm_release_source src = a.sources[s];
    bool bad, clamped;
    const long long cs = source_count(src, a.max_count, &bad, &clamped);
    unsigned cnt[REL_CLASSES] = {0, 0, 0, 0};
    if ((long long)(m - t) < cs) {                                     // else: nothing of this chunk is wanted
        int cls = CAND_IDLE;
        if ((long long)m < cs) cls = candidate(a, src, m).cls;
        cnt[0] = (unsigned)__popcll(__ballot(cls == CAND_ACTIVE || cls == CAND_LEFT));
        cnt[1] = (unsigned)__popcll(__ballot(cls == CAND_FOREIGN));
        cnt[2] = (unsigned)__popcll(__ballot(cls == CAND_LAND));
        cnt[3] = (unsigned)__popcll(__ballot(cls == CAND_LEFT));
    }
    if (lane == 0) {
        for (int c = 0; c < REL_CLASSES; c++) part[wave][c] = cnt[c];
        a.cand_part[(size_t)b * REL_WAVES + wave] = cnt[0];
    }
    __syncthreads();
    if (t < REL_CLASSES) {
        unsigned sum = 0;
        for (int w = 0; w < REL_WAVES; w++) sum += part[w][t];
        a.table[(size_t)t * a.ncand + b] = sum;
    }
}

// the slot side: block b of max(nblocks, 1)
__device__ __forceinline__ void slot_count(const ReleaseArgs &a, unsigned b)
{
    __shared__ unsigned wfree[REL_WAVES];
    const unsigned t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const long long wfirst = (long long)b * REL_TILE + (long long)wave * REL_WAVE_TILE;
    unsigned nfree = 0;
    for (int c = 0; c < REL_WAVE_TILE / 64 && wfirst + c * 64 < a.n; c++) {
        const long long p = wfirst + c * 64 + lane;
        nfree += (unsigned)__popcll(__ballot(p < a.n && a.status[p] == DLESM_DRIFTER_FREE));
    }
    if (lane == 0) wfree[wave] = nfree;
    if (b < a.nblocks && lane == 0) a.slot_part[(size_t)b * REL_WAVES + wave] = nfree;
    __syncthreads();
    const size_t first = (size_t)REL_CLASSES * a.ncand;
    if (b < a.nblocks && t == 0) {
        unsigned s = 0;
        for (int w = 0; w < REL_WAVES; w++) s += wfree[w];
        a.table[first + b] = s;
    }
    if (b == 0 && first + a.nblocks + t < a.m) a.table[first + a.nblocks + t] = 0;      // the total's entry and the padding
}

// one launch for both sides: the first ncand blocks count candidates, the others slots
SORT_KERNEL count_k(const ReleaseArgs a)
{
    if (blockIdx.x < a.ncand)
        cand_count(a, blockIdx.x);
    else
        slot_count(a, blockIdx.x - a.ncand);
}

SORT_KERNEL stage_k(const ReleaseArgs a)
{
    const unsigned t = threadIdx.x, lane = t & 63, wave = t >> 6, b = blockIdx.x;
    if (b >= a.ncand) return;
    const unsigned *const part = a.cand_part + (size_t)b * REL_WAVES;
    if (part[wave] == 0) return;                                       // no barrier below: a wave may leave
    unsigned base = a.table[b] - a.head(0);
    for (unsigned w = 0; w < wave; w++) base += part[w];
    const unsigned nfree = a.all_free();
    if (base >= nfree) return;
    const unsigned s = b / a.nchunks, m = (b % a.nchunks) * REL_CHUNK + t;
    const dlesm_release_source src = a.sources[s];
    bool bad, clamped;
    const long long cs = source_count(src, a.max_count, &bad, &clamped);
    Candidate c;
    c.cls = CAND_IDLE;
    if ((long long)m < cs) c = candidate(a, src, m);
    const bool acc = c.cls == CAND_ACTIVE || c.cls == CAND_LEFT;
    const unsigned k = base + (unsigned)__popcll(__ballot(acc) & ((1ull << lane) - 1ull));
    if (acc && k < nfree) {                                            // k < nfree <= n and k < nsources * max_count
        a.stage.x[k] = c.lx, a.stage.y[k] = c.ly;
        a.stage.id[k] = c.id, a.stage.tag[k] = (uint64_t)src.tag;
        a.stage.status[k] = c.cls == CAND_ACTIVE ? DLESM_DRIFTER_ACTIVE : DLESM_DRIFTER_LEFT;
    }
}

__device__ __forceinline__ void fill(const ReleaseArgs &a, unsigned b)
{
    const unsigned t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const unsigned *const part = a.slot_part + (size_t)b * REL_WAVES;
    if (part[wave] == 0) return;
    const long long all = a.accepted();
    long long base = a.table[(size_t)REL_CLASSES * a.ncand + b] - a.free_head();
    for (unsigned w = 0; w < wave; w++) base += part[w];
    if (base >= all) return;
    const uint64_t born = (uint64_t)a.tick + (a.tick_dev ? (uint64_t)*a.tick_dev : 0ull);
    const long long wfirst = (long long)b * REL_TILE + (long long)wave * REL_WAVE_TILE;
    for (int c = 0; base < all && c < REL_WAVE_TILE / 64 && wfirst + c * 64 < a.n; c++) {
        const long long p = wfirst + c * 64 + lane;
        const bool fr = p < a.n && a.status[p] == DLESM_DRIFTER_FREE;
        const unsigned long long bal = __ballot(fr);
        if (bal == 0) continue;
        const long long j = base + __popcll(bal & ((1ull << lane) - 1ull));
        if (fr && j < all) {                                           // j < the FREE slots too: slot p is the j-th of them
            a.px[p] = a.stage.x[j], a.py[p] = a.stage.y[j];
            a.id[p] = a.stage.id[j];
            if (a.tag) a.tag[p] = a.stage.tag[j];
            if (a.born) a.born[p] = born;
            a.status[p] = a.stage.status[j];
        }
        base += __popcll(bal);
    }
}

// one block: the ids advance and the record is stored.  Behind stage_k, the last reader of next_id; the fill beside it
// reads neither the table of sources nor the record
__device__ __forceinline__ void advance(const ReleaseArgs &a)
{
    __shared__ unsigned long long wreq[REL_WAVES];
    __shared__ unsigned wcl[REL_WAVES], wbad[REL_WAVES];
    const unsigned t = threadIdx.x, lane = t & 63, wave = t >> 6;
    unsigned long long req = 0;
    unsigned ncl = 0, nbad = 0;
    for (unsigned s0 = 0; s0 < (unsigned)a.nsources; s0 += SORT_BLOCK) {
        const unsigned s = s0 + t;
        long long cs = 0;
        bool bad = false, clamped = false;
        if (s < (unsigned)a.nsources) {
            const dlesm_release_source src = a.sources[s];
            cs = source_count(src, a.max_count, &bad, &clamped);
            if (cs != 0) a.sources[s].next_id = (long long)((uint64_t)src.next_id + (uint64_t)cs);
        }
        req += (unsigned long long)cs;
        ncl += (unsigned)__popcll(__ballot(clamped)), nbad += (unsigned)__popcll(__ballot(bad));
    }
    for (int o = 32; o > 0; o >>= 1) req += __shfl_xor(req, o);
    if (lane == 0) wreq[wave] = req, wcl[wave] = ncl, wbad[wave] = nbad;
    __syncthreads();
    if (t == 0) {
        unsigned long long requested = 0;
        unsigned clamped = 0, bad = 0;
        for (int w = 0; w < REL_WAVES; w++) requested += wreq[w], clamped += wcl[w], bad += wbad[w];
        // without a source the five heads are one entry and every difference is 0
        const unsigned h1 = a.head(1), h2 = a.head(2), h3 = a.head(3);
        const unsigned acc = h1 - a.head(0), foreign = h2 - h1, land = h3 - h2, edge = a.free_head() - h3;
        const unsigned nfree = a.all_free();
        const unsigned released = acc < nfree ? acc : nfree;
        dlesm_release_counts r;
        r.requested = (long long)requested;
        r.released = (int)released, r.foreign = (int)foreign, r.on_land = (int)land, r.dropped = (int)(acc - released);
        r.edge = (int)edge, r.nfree = (int)(nfree - released), r.clamped = (int)clamped, r.bad_source = (int)bad;
        for (int k = 0; k < 6; k++) r.pad[k] = 0;
        *a.counts = r;
    }
}

// one launch for both: the first nblocks blocks fill their tiles, the last one advances the ids and stores the record
SORT_KERNEL fill_k(const ReleaseArgs a)
{
    if (blockIdx.x < a.nblocks)
        fill(a, blockIdx.x);
    else
        advance(a);
}

// ---- the host side

// where the pieces of the scratch lie (every piece 16-byte aligned)
struct ReleasePlan {
    unsigned nchunks, ncand, nblocks, m, nscan;
    long long cap;                             // records of the staging area
    size_t table, sums, cand_part, slot_part, stage, bytes;
};

ReleasePlan release_plan(long long n, int nsources, int max_count)
{
    ReleasePlan p{};
    const auto up16 = [](size_t b) { return (b + 15) / 16 * 16; };
    p.nchunks = (unsigned)(((long long)max_count + REL_CHUNK - 1) / REL_CHUNK);
    p.ncand = (unsigned)nsources * p.nchunks;
    p.nblocks = (unsigned)((n + REL_TILE - 1) / REL_TILE);
    p.m = (REL_CLASSES * p.ncand + p.nblocks + 1 + SCAN_ITEMS - 1) / SCAN_ITEMS * SCAN_ITEMS;
    p.nscan = (p.m + SCAN_TILE - 1) / SCAN_TILE;
    const long long wanted = (long long)nsources * max_count;
    p.cap = n < wanted ? n : wanted;
    size_t at = 0;
    const auto piece = [&](size_t b) {
        const size_t here = at;
        at += up16(b);
        return here;
    };
    p.table = piece((size_t)p.m * 4), p.sums = piece((size_t)p.nscan * 4);
    p.cand_part = piece((size_t)p.ncand * REL_WAVES * 4), p.slot_part = piece((size_t)p.nblocks * REL_WAVES * 4);
    p.stage = piece((size_t)p.cap * 8 * 4 + (size_t)p.cap * 4);
    p.bytes = at;
    return p;
}

// what the scratch-size function and the entry refuse alike
int check_sizes(const char *who, long long n, int nsources, int max_count)
{
    DLESM_REQUIRE(n >= 0 && n <= REL_MAX_N, "%s: %lld slots (0..2^31-1)", who, n);
    DLESM_REQUIRE(nsources >= 0 && nsources <= DLESM_RELEASE_MAX_SOURCES, "%s: nsources = %d (0..%d)", who, nsources,
                  (int)DLESM_RELEASE_MAX_SOURCES);
    DLESM_REQUIRE(max_count >= 1, "%s: max_count = %d (at least 1)", who, max_count);
    DLESM_REQUIRE((long long)nsources * max_count <= REL_MAX_N, "%s: %d sources x %d candidates (at most 2^31-1)", who, nsources,
                  max_count);
    DLESM_REQUIRE((long long)nsources * (((long long)max_count + REL_CHUNK - 1) / REL_CHUNK) <= REL_MAX_BLOCKS,
                  "%s: %d sources x %d candidates are more than 2^22 blocks of %d", who, nsources, max_count, REL_CHUNK);
    return DLESM_OK;
}

struct Span {
    const void *p;
    size_t bytes;
    bool out;
    const char *name;
};

} // namespace

} // namespace dlesm

using namespace dlesm;

extern "C" int dlesm_release_scratch(long long n, int nsources, int max_count, long long *bytes)
{
    static const char *const who = "dlesm_release_scratch";
    clear_error();
    DLESM_REQUIRE(bytes != nullptr, "%s: null bytes", who);
    if (int rc = check_sizes(who, n, nsources, max_count)) return rc;
    *bytes = (long long)release_plan(n, nsources, max_count).bytes;
    return DLESM_OK;
}

extern "C" int dlesm_release_f64(int ld, int ny, int xstart, int xstop, int ystart, int ystop, int offx, int offy,
                                 const int *tmask, dlesm_release_source *sources, int nsources, int max_count, long long seed,
                                 long long tick, const long long *tick_dev, long long n, double *px, double *py, int *status,
                                 long long *id, long long *tag, long long *born, dlesm_release_counts *counts, void *scratch,
                                 long long scratch_bytes, void *stream)
{
    static const char *const who = "dlesm_release_f64";
    if (int rc = ensure_device()) return rc;
    DLESM_REQUIRE(tmask != nullptr && sources != nullptr, "%s: null tmask or sources", who);
    DLESM_REQUIRE(id != nullptr && counts != nullptr, "%s: null id or counts", who);
    const ParticleArrays arr{{px, py, status}, n};
    bool empty;
    if (int rc = arr.check(who, ld, ny, xstart, xstop, ystart, ystop, &empty)) return rc;
    if (int rc = check_sizes(who, n, nsources, max_count)) return rc;
    DLESM_REQUIRE((uintptr_t)sources % 8 == 0 && (uintptr_t)id % 8 == 0 && (uintptr_t)counts % 8 == 0,
                  "%s: sources, id or counts is not 8-byte aligned", who);
    DLESM_REQUIRE((uintptr_t)tag % 8 == 0 && (uintptr_t)born % 8 == 0 && (uintptr_t)tick_dev % 8 == 0,
                  "%s: tag, born or tick_dev is not 8-byte aligned", who);
    DLESM_REQUIRE((uintptr_t)tmask % 4 == 0, "%s: tmask is not 4-byte aligned", who);
    DLESM_REQUIRE(tick >= 0, "%s: tick = %lld", who, tick);
    DLESM_REQUIRE(scratch != nullptr && (uintptr_t)scratch % 16 == 0, "%s: scratch is null or not 16-byte aligned", who);
    const ReleasePlan plan = release_plan(n, nsources, max_count);
    DLESM_REQUIRE(scratch_bytes >= 0 && (unsigned long long)scratch_bytes >= plan.bytes,
                  "%s: %lld bytes of scratch, %zu needed (dlesm_release_scratch)", who, scratch_bytes, plan.bytes);
    const Span spans[] = {
        {px, (size_t)n * 8, true, "px"},
        {py, (size_t)n * 8, true, "py"},
        {status, (size_t)n * 4, true, "status"},
        {id, (size_t)n * 8, true, "id"},
        {tag, tag ? (size_t)n * 8 : 0, true, "tag"},
        {born, born ? (size_t)n * 8 : 0, true, "born"},
        {sources, (size_t)nsources * sizeof(dlesm_release_source), true, "sources"},
        {counts, sizeof(dlesm_release_counts), true, "counts"},
        {scratch, plan.bytes, true, "scratch"},
        {tmask, (size_t)ld * (size_t)ny * 4, false, "tmask"},
        {tick_dev, tick_dev ? (size_t)8 : 0, false, "tick_dev"},
    };
    const int ns = (int)(sizeof(spans) / sizeof(spans[0]));
    for (int k = 0; k < ns; k++)
        for (int q = 0; q < k; q++)
            DLESM_REQUIRE(!(spans[k].out || spans[q].out) || spans[k].bytes == 0 || spans[q].bytes == 0 ||
                              !overlap(spans[k].p, spans[k].bytes, spans[q].p, spans[q].bytes),
                          "%s: %s and %s overlap", who, spans[q].name, spans[k].name);

    hipStream_t s = (hipStream_t)stream;
    char *const base = (char *)scratch;
    ReleaseArgs a{};
    a.tmask = tmask, a.sources = sources, a.ld = ld, a.nsources = nsources, a.max_count = max_count;
    a.nchunks = plan.nchunks, a.ncand = plan.ncand, a.nblocks = plan.nblocks, a.m = plan.m;
    a.box = drifter_box(xstart, xstop, ystart, ystop);
    a.gx_lo = (double)((long long)xstart + offx), a.gx_hi = (double)((long long)xstop + 1 + offx);
    a.gy_lo = (double)((long long)ystart + offy), a.gy_hi = (double)((long long)ystop + 1 + offy);
    a.offx = (double)offx, a.offy = (double)offy;
    a.k0 = (unsigned)(unsigned long long)seed, a.k1 = (unsigned)((unsigned long long)seed >> 32);
    a.tick = tick, a.tick_dev = tick_dev, a.n = n;
    a.px = px, a.py = py, a.status = status;
    a.id = (uint64_t *)id, a.tag = (uint64_t *)tag, a.born = (uint64_t *)born, a.counts = counts;
    a.table = (unsigned *)(base + plan.table);
    a.cand_part = (unsigned *)(base + plan.cand_part), a.slot_part = (unsigned *)(base + plan.slot_part);
    char *const st = base + plan.stage;
    const size_t col = (size_t)plan.cap * 8;
    a.stage = Stage{(double *)st, (double *)(st + col), (uint64_t *)(st + 2 * col), (uint64_t *)(st + 3 * col),
                    (int *)(st + 4 * col)};
    const dim3 block(SORT_BLOCK);
    hipLaunchKernelGGL(count_k, dim3(plan.ncand + (plan.nblocks ? plan.nblocks : 1u)), block, 0, s, a);
    launch_scan(a.table, a.m, plan.nscan, (unsigned *)(base + plan.sums), s);
    if (plan.ncand && plan.nblocks) hipLaunchKernelGGL(stage_k, dim3(plan.ncand), block, 0, s, a);
    hipLaunchKernelGGL(fill_k, dim3(plan.nblocks + 1u), block, 0, s, a);
    DLESM_HIP_TRY(hipGetLastError());
    return DLESM_OK;
}
