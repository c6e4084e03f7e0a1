// The exclusive scan of a table of 32-bit counts on the device, shared by the particle sort (dlesm_particle_sort.hip, DESIGN.md
// section 6.18) and the particle migration (dlesm_particle_migrate.hip, section 6.21).  A table of m entries, m a multiple of
// SCAN_ITEMS and the table 16-byte aligned, is scanned in place by
//   scan_reduce_k   the sum of each scan block's SCAN_TILE entries                 (only when the table is more than one block)
//   scan_top_k      one block: the exclusive scan of those sums, in place         (only then)
//   scan_down_k     every entry becomes the sum of all entries before it
// Integer adds only, no atomics, plain vector stores.  Included inside namespace dlesm { namespace { ... } } of a .hip file:
// every translation unit holds its own copy of the three kernels.
#ifndef DLESM_SCAN_H
#define DLESM_SCAN_H

constexpr int SORT_BLOCK = 256;            // four waves
constexpr int SCAN_ITEMS = 8;              // table entries of one lane of the scan
constexpr int SCAN_TILE = SORT_BLOCK * SCAN_ITEMS;

#define SORT_KERNEL __global__ __launch_bounds__(SORT_BLOCK) __attribute__((amdgpu_waves_per_eu(8, 8))) void

// exclusive scan of one value per thread over the block; wtot: four words of LDS, free again on return
__device__ __forceinline__ unsigned block_scan(unsigned v, unsigned *wtot, unsigned &total)
{
    const unsigned lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned inc = v;
    for (int o = 1; o < 64; o <<= 1) {
        const unsigned up = __shfl_up(inc, o);
        if (lane >= (unsigned)o) inc += up;
    }
    if (lane == 63) wtot[wave] = inc;
    __syncthreads();
    unsigned before = 0;
    total = 0;
    for (unsigned w = 0; w < SORT_BLOCK / 64; w++) {
        const unsigned c = wtot[w];
        before += w < wave ? c : 0;
        total += c;
    }
    __syncthreads();
    return before + inc - v;
}

// the table has m entries, a multiple of SCAN_ITEMS, and starts 16-byte aligned: a lane's eight entries are all there or
// none is
__device__ __forceinline__ bool scan_load(const unsigned *table, unsigned m, unsigned (&v)[SCAN_ITEMS], unsigned &at)
{
    at = (blockIdx.x * SORT_BLOCK + threadIdx.x) * SCAN_ITEMS;
    const bool mine = at < m;
    for (int k = 0; k < SCAN_ITEMS; k += 4) {
        const uint4 q = mine ? *(const uint4 *)(table + at + k) : make_uint4(0, 0, 0, 0);
        v[k] = q.x, v[k + 1] = q.y, v[k + 2] = q.z, v[k + 3] = q.w;
    }
    return mine;
}

SORT_KERNEL scan_reduce_k(const unsigned *table, unsigned m, unsigned *sums)
{
    __shared__ unsigned wtot[SORT_BLOCK / 64];
    unsigned v[SCAN_ITEMS], at, s = 0, total;
    (void)scan_load(table, m, v, at);
    for (int k = 0; k < SCAN_ITEMS; k++) s += v[k];
    (void)block_scan(s, wtot, total);
    if (threadIdx.x == 0) sums[blockIdx.x] = total;
}

// one block: the exclusive scan of the scan blocks' sums, in place
SORT_KERNEL scan_top_k(unsigned *sums, unsigned nscan)
{
    __shared__ unsigned wtot[SORT_BLOCK / 64];
    unsigned carry = 0;
    for (unsigned b0 = 0; b0 < nscan; b0 += SORT_BLOCK) {
        const unsigned b = b0 + threadIdx.x;
        const unsigned v = b < nscan ? sums[b] : 0u;
        unsigned total;
        const unsigned ex = block_scan(v, wtot, total);
        if (b < nscan) sums[b] = carry + ex;
        carry += total;
    }
}

// sums == nullptr: the table is one scan block
SORT_KERNEL scan_down_k(unsigned *table, unsigned m, const unsigned *sums)
{
    __shared__ unsigned wtot[SORT_BLOCK / 64];
    unsigned v[SCAN_ITEMS], at, s = 0, total;
    const bool mine = scan_load(table, m, v, at);
    for (int k = 0; k < SCAN_ITEMS; k++) s += v[k];
    unsigned run = block_scan(s, wtot, total) + (sums ? sums[blockIdx.x] : 0u);
    if (!mine) return;
    for (int k = 0; k < SCAN_ITEMS; k++) {
        const unsigned c = v[k];
        v[k] = run;
        run += c;
    }
    for (int k = 0; k < SCAN_ITEMS; k += 4) *(uint4 *)(table + at + k) = make_uint4(v[k], v[k + 1], v[k + 2], v[k + 3]);
}

// the launches of one scan of table[0..m) on s; sums: nscan = ceil(m / SCAN_TILE) words, used when nscan > 1
inline void launch_scan(unsigned *table, unsigned m, unsigned nscan, unsigned *sums, hipStream_t s)
{
    const dim3 block(SORT_BLOCK);
    if (nscan > 1) {
        hipLaunchKernelGGL(scan_reduce_k, dim3(nscan), block, 0, s, (const unsigned *)table, m, sums);
        hipLaunchKernelGGL(scan_top_k, dim3(1), block, 0, s, sums, nscan);
    }
    hipLaunchKernelGGL(scan_down_k, dim3(nscan), block, 0, s, table, m,
                       nscan > 1 ? (const unsigned *)sums : (const unsigned *)nullptr);
}

#endif
