// Slot linear transforms on dBFV ciphertexts with wide public diagonals, the limb-wise key-switch path
// ("dBFV linear transforms"):
//
//   out[b] = reduce( sum_r W_r * rot_r(x_b) ),   x_b a dBFV ciphertext of D limbs, W_r a lifted digit vector,
//
// limb for limb exacto_dbfv_plain_mul_sum over the rotations exacto_bfv_rotate_hoisted makes of the B D limbs.
// The kernel joins hoist_mac_kernel<true> (hoist.hip) with the accumulators of dbfv_plain_mul_kernel
// (dbfv_plain.hip, shared through dbfv_acc.hpp): after the one decomposition and digit transform of the B D
// limbs a thread owns one position of one (item, prime) and, rotation by rotation and ciphertext digit by
// ciphertext digit, forms the rotated pair (a0, a1) exactly as hoist_mac_kernel does (c0 and the digit rows
// gathered through perm_r, the key words coalesced, Shoup MAC in [0, 2q), canonical residues; the identity
// reads no key) and adds W[r][i] a0, W[r][i] a1 into the 128-bit sums of wide limb i + j.  No rotated limb
// is ever stored.
//
// The bound: a0, a1 and the lifted W are canonical, so the sums obey the bound at the head of dbfv_plain.hip
// with a rotation in the place of a term: a sum takes at most D products per rotation and every sum is
// reduced in place after flush / D rotations.
//
// NC = 2: a thread keeps the sums of both components (2 W 128-bit sums).  NC = 1: a thread owns one
// component (blocks of component 1 follow those of component 0), which halves the sums in registers and
// doubles the digit gathers; the instantiations that would not fit the register file otherwise use it.
#include "dbfv_acc.hpp"

namespace exacto {

static constexpr int DH_TPB = 256;

template <int D, bool HI, int NC>
__global__ void __launch_bounds__(DH_TPB)
dbfv_hoist_lt_kernel(const u64* __restrict__ ct, const u64* __restrict__ Dg, const u64* __restrict__ keys,
                     const u64* __restrict__ keys_s, const uint32_t* __restrict__ perm,
                     const unsigned char* __restrict__ ident, const u64* __restrict__ pl, u64* __restrict__ out, int R,
                     int guse, int items, int nblk, int flush_rots, int accum, unsigned live,
                     const u64* __restrict__ fold, int n, int L, const PrimeConst* __restrict__ primes) {
    constexpr int W = HI ? 2 * D - 1 : D;
    const long Ln = (long)L * n;
    const unsigned it = blockIdx.x % (unsigned)items;
    const unsigned rest = blockIdx.x / (unsigned)items;
    const unsigned blk = rest % (unsigned)nblk;
    const int c_lo = NC == 1 ? (int)(rest / (unsigned)nblk) : 0;   // block-uniform
    const long coef = (long)blk * DH_TPB + threadIdx.x;
    if (coef >= Ln) return;
    const int l = (int)(coef / n);
    const int p = (int)(coef - (long)l * n);
    const PrimeConst& P = primes[l];
    const u64 q = P.q, q2 = P.two_q, nq = (u64)0 - q;
    const u64 r64 = pl_r64(P);
    const auto self = [](u128& v) -> u128& { return v; };
    u128 acc[NC][W];
#pragma unroll
    for (int c = 0; c < NC; ++c)
#pragma unroll
        for (int m = 0; m < W; ++m) acc[c][m] = 0;
    int since = 0;
    for (int r = 0; r < R; ++r) {
        u64 w[D];
#pragma unroll
        for (int i = 0; i < D; ++i) w[i] = pl[((long)r * D + i) * Ln + coef];
        const bool idn = ident[r] != 0;
        const long src = (long)l * n + perm[(long)r * n + p];
        const u64* kp = keys + (long)r * guse * 2 * Ln + coef;
        const u64* ksp = keys_s + (long)r * guse * 2 * Ln + coef;
#pragma unroll
        for (int j = 0; j < D; ++j) {
            const long limb = (long)it * D + j;
            const u64* c0 = ct + limb * 2 * Ln;
            u64 a[NC];
            if (idn) {
#pragma unroll
                for (int c = 0; c < NC; ++c) a[c] = c0[(long)(c_lo + c) * Ln + coef];
            } else {
                const u64* dp = Dg + limb * guse * Ln + src;
#pragma unroll
                for (int c = 0; c < NC; ++c) a[c] = (c_lo + c) == 0 ? c0[src] : 0;
                constexpr int U = 4;
                for (int g0 = 0; g0 < guse; g0 += U) {
                    u64 d[U], kw[NC][U], kh[NC][U];
#pragma unroll
                    for (int t = 0; t < U; ++t) {
                        const int g = min(g0 + t, guse - 1);  // clamped (re-read) tail, masked below
                        d[t] = dp[(long)g * Ln];
#pragma unroll
                        for (int c = 0; c < NC; ++c) {
                            kw[c][t] = kp[(2L * g + c_lo + c) * Ln];
                            kh[c][t] = ksp[(2L * g + c_lo + c) * Ln];
                        }
                    }
#pragma unroll
                    for (int t = 0; t < U; ++t) {
                        if (g0 + t < guse) {
#pragma unroll
                            for (int c = 0; c < NC; ++c) {
                                const u64 v = a[c] + shoup_mul_nq(d[t], kw[c][t], kh[c][t], nq);
                                a[c] = v >= q2 ? v - q2 : v;
                            }
                        }
                    }
                }
#pragma unroll
                for (int c = 0; c < NC; ++c) a[c] = a[c] >= q ? a[c] - q : a[c];
            }
#pragma unroll
            for (int i = 0; i < D; ++i) {
                const int m = i + j;
                if (m < W && pl_live<D>(live, m)) {
#pragma unroll
                    for (int c = 0; c < NC; ++c) acc[c][m] += (u128)w[i] * a[c];
                }
            }
        }
        if (++since == flush_rots && r + 1 < R) {
            since = 0;
#pragma unroll
            for (int c = 0; c < NC; ++c) pl_red_all<W>(acc[c], P, r64, self);
        }
    }
    if constexpr (HI) {
        const u64* f = fold + (long)l * (D - 1) * D;
#pragma unroll
        for (int c = 0; c < NC; ++c) pl_fold<D>(acc[c], live, f, P, r64, self);
    }
    u64* dst = out + (long)it * D * 2 * Ln + coef;
#pragma unroll
    for (int i = 0; i < D; ++i)
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            u64* o = dst + ((long)i * 2 + c_lo + c) * Ln;
            u64 v = pl_red(acc[c][i], P, r64);
            if (accum) v = add_mod(v, *o, q);
            *o = v;
        }
}

// the instantiations that keep one component per thread (the resource table)
template <int D, bool HI>
static constexpr int dh_nc() {
    return (HI ? 2 * D - 1 : D) > DH_NC2_MAX_W ? 1 : 2;
}

template <int D, bool HI>
static void dh_launch(const DbfvHoistArgs& a, hipStream_t s) {
    constexpr int NC = dh_nc<D, HI>();
    const long Ln = (long)a.L * a.n;
    const int nblk = (int)((Ln + DH_TPB - 1) / DH_TPB);
    const long blocks = a.items * nblk * (NC == 1 ? 2 : 1);
    EXACTO_LAUNCH((dbfv_hoist_lt_kernel<D, HI, NC>), dim3((unsigned)blocks), dim3(DH_TPB), 0, s, a.ct, a.D, a.keys,
                  a.keys_s, a.perm, a.ident, a.pl, a.out, a.R, a.guse, (int)a.items, nblk, a.flush / D, a.accum, a.live,
                  a.fold, a.n, a.L, a.primes);
}

// d <= DP_MAX_D, guse >= 0 (0: every element is the identity and neither D nor the keys are read)
void launch_dbfv_hoist_lt(const DbfvHoistArgs& a, hipStream_t s) {
    if (a.items <= 0 || a.R <= 0) return;
#define DH_CASE(D_) case D_: return a.live ? dh_launch<D_, true>(a, s) : dh_launch<D_, false>(a, s)
    switch (a.d) {
    DH_CASE(1); DH_CASE(2); DH_CASE(3); DH_CASE(4); DH_CASE(5); DH_CASE(6); DH_CASE(7); DH_CASE(8);
    default: break;
    }
#undef DH_CASE
}

}  // namespace exacto
