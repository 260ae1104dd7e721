// The wide-limb accumulators of the dBFV plaintext products, shared by dbfv_plain.hip (a streaming product)
// and dbfv_hoist.hip (the same sums fed by hoisted rotations): the reduction of a lazily accumulated
// 128-bit sum, the test for a wide limb that is formed at all, and the fold of the high limbs.  The bound
// the lazy sums rely on is stated at the head of dbfv_plain.hip.
#pragma once
#include "exacto_internal.hpp"

namespace exacto {

// 2^64 mod q
__device__ __forceinline__ u64 pl_r64(const PrimeConst& P) { return add_mod(reduce64(~(u64)0, P.q, P.mu64), 1, P.q); }

// hi:lo (any 128-bit value) mod q; r64 = 2^64 mod q
__device__ __forceinline__ u64 pl_red(u128 v, const PrimeConst& P, u64 r64) {
    const u64 h = reduce64((u64)(v >> 64), P.q, P.mu64);
    const u64 l = reduce64((u64)v, P.q, P.mu64);
    return add_mod(mul_mod(h, r64, P), l, P.q);
}

// wide limb m of a d = D product is formed: every low limb, a high limb only with a non-zero representative
template <int D>
__device__ __forceinline__ bool pl_live(unsigned live, int m) {
    return m < D || (live >> (m - D) & 1);
}

// Every one of the W sums reduced in place (between two runs of lazy products); `lane` picks the 128-bit
// sum inside an accumulator (dbfv_plain.hip keeps two positions per accumulator).
template <int W, class Acc, class Lane>
__device__ __forceinline__ void pl_red_all(Acc (&acc)[W], const PrimeConst& P, u64 r64, Lane lane) {
#pragma unroll
    for (int m = 0; m < W; ++m) lane(acc[m]) = pl_red(lane(acc[m]), P, r64);
}

// The fold of the high limbs m in [D, 2D - 1) into the low ones: all sums reduced to canonical residues,
// then acc[i] += rep[m - D][i] acc[m] with f = fold + l (D - 1) D the digits mod q_l (at most D - 1
// products join one residue; the caller reduces acc[i] once more when it stores).
template <int D, class Acc, class Lane>
__device__ __forceinline__ void pl_fold(Acc (&acc)[2 * D - 1], unsigned live, const u64* __restrict__ f,
                                        const PrimeConst& P, u64 r64, Lane lane) {
    pl_red_all<2 * D - 1>(acc, P, r64, lane);
#pragma unroll
    for (int m = D; m < 2 * D - 1; ++m)
        if (live >> (m - D) & 1) {
#pragma unroll
            for (int i = 0; i < D; ++i) lane(acc[i]) += (u128)f[(m - D) * D + i] * (u64)lane(acc[m]);
        }
}

}  // namespace exacto
