// The reductions over the 64 lanes of a wave on the VALU, for the record reductions (dlesm_stats.hip, DESIGN.md section 5.5;
// dlesm_courant.hip, section 6.14; dlesm_flow_courant.hip, section 6.15), and the (value, index) pairs of the two Courant
// checks under "the larger value, then the lower index".
//
// One fixed scheme: within each row of 16 lanes a butterfly by DPP -- xor 1, xor 2, the half-row and row mirrors: every lane
// of a row ends with the same bits, as a + b == b + a -- then the four rows' values read into scalars and combined as
// (row 0 . row 1) . (row 2 . row 3).  The result is the same in every lane; every lane of the wave must be active.  Minima,
// maxima and integer sums are exact, so the order plays no part in them; the f64 sums of the field statistics depend on
// exactly this order.
#ifndef DLESM_WAVE_REDUCE_H
#define DLESM_WAVE_REDUCE_H

#include <hip/hip_runtime.h>

namespace dlesm {

namespace wavered {

enum { OP_MIN, OP_MAX, OP_ADD };
template <int OP, class T>
__device__ __forceinline__ T combine(T a, T b)
{
    if constexpr (OP == OP_MIN) return b < a ? b : a;      // no NaN gets here
    else if constexpr (OP == OP_MAX) return b > a ? b : a;
    else return a + b;
}

// (value, index) pairs under "the larger value, then the lower index"
__device__ __forceinline__ void take(double &m, long long &at, double x, long long ix)
{
    const bool better = x > m || (x == m && ix < at);
    m = better ? x : m;
    at = better ? ix : at;
}

template <int CTRL>
__device__ __forceinline__ double dpp_f64(double v)
{
    return __hiloint2double(__builtin_amdgcn_mov_dpp(__double2hiint(v), CTRL, 0xf, 0xf, false),
                            __builtin_amdgcn_mov_dpp(__double2loint(v), CTRL, 0xf, 0xf, false));
}
template <int CTRL>
__device__ __forceinline__ long long dpp_i64(long long v)
{
    const unsigned lo = (unsigned)__builtin_amdgcn_mov_dpp((int)(v & 0xffffffffLL), CTRL, 0xf, 0xf, false);
    const int hi = __builtin_amdgcn_mov_dpp((int)(v >> 32), CTRL, 0xf, 0xf, false);
    return ((long long)hi << 32) | lo;
}

template <int OP>
__device__ __forceinline__ double wave_f64(double v)
{
    v = combine<OP>(v, dpp_f64<0xB1>(v));                  // quad_perm [1,0,3,2]
    v = combine<OP>(v, dpp_f64<0x4E>(v));                  // quad_perm [2,3,0,1]
    v = combine<OP>(v, dpp_f64<0x141>(v));                 // row_half_mirror
    v = combine<OP>(v, dpp_f64<0x140>(v));                 // row_mirror
    const int lo = __double2loint(v), hi = __double2hiint(v);
    auto row = [&](int l) { return __hiloint2double(__builtin_amdgcn_readlane(hi, l), __builtin_amdgcn_readlane(lo, l)); };
    return combine<OP>(combine<OP>(row(0), row(16)), combine<OP>(row(32), row(48)));
}
template <int OP>
__device__ __forceinline__ long long wave_i64(long long v)
{
    v = combine<OP>(v, dpp_i64<0xB1>(v));
    v = combine<OP>(v, dpp_i64<0x4E>(v));
    v = combine<OP>(v, dpp_i64<0x141>(v));
    v = combine<OP>(v, dpp_i64<0x140>(v));
    const int lo = (int)(v & 0xffffffffLL), hi = (int)(v >> 32);
    auto row = [&](int l) {
        return ((long long)__builtin_amdgcn_readlane(hi, l) << 32) | (unsigned)__builtin_amdgcn_readlane(lo, l);
    };
    return combine<OP>(combine<OP>(row(0), row(16)), combine<OP>(row(32), row(48)));
}
// the 32-bit sum: a word of packed counts whose fields cannot carry into each other (a wave tile of the Courant checks owns
// at most 126 cells, a byte each; a workgroup of the field statistics at most 2048, 16 bits each)
__device__ __forceinline__ int wave_add_i32(int v)
{
    v += __builtin_amdgcn_mov_dpp(v, 0xB1, 0xf, 0xf, false);
    v += __builtin_amdgcn_mov_dpp(v, 0x4E, 0xf, 0xf, false);
    v += __builtin_amdgcn_mov_dpp(v, 0x141, 0xf, 0xf, false);
    v += __builtin_amdgcn_mov_dpp(v, 0x140, 0xf, 0xf, false);
    return (__builtin_amdgcn_readlane(v, 0) + __builtin_amdgcn_readlane(v, 16)) +
           (__builtin_amdgcn_readlane(v, 32) + __builtin_amdgcn_readlane(v, 48));
}

// a (maximum, lowest index) pair over the wave: `none` is the index of a lane that does not hold the maximum
__device__ __forceinline__ void wave_pair(double &m, long long &at, long long none)
{
    const double top = wave_f64<OP_MAX>(m);
    at = wave_i64<OP_MIN>(m == top ? at : none);
    m = top;
}

} // namespace wavered

} // namespace dlesm

#endif
