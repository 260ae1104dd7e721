// Hoisted rotations on a prepared Galois key set ("Hoisted rotations").
//
// sigma_k is a ring homomorphism, so sigma_k(c1) == sum_g sigma_k(d_g) B^g with d_g the gadget digits of c1
// itself, and in the NTT domain sigma_k is a permutation of evaluations without signs, the same for every
// prime: NTT(sigma_k(a))[p] = NTT(a)[perm_k[p]] (exacto_galois_ntt_permutation).  One ciphertext is therefore
// decomposed and its digits transformed once; each rotation is then only a MAC whose digit (and c0) reads go
// through perm_r, while the key is read position by position.
//
//   hoist_mac_kernel<false> : out[it][r] = (c0 o perm_r + sum_g (D_g o perm_r) (.) k_{r,g,0},
//                                           sum_g (D_g o perm_r) (.) k_{r,g,1}), every r in one launch
//   hoist_mac_lds_kernel    : the same rotations with key slice r staged in LDS (guse <= 32, L n a multiple of 64)
//   hoist_mac_kernel<true>  : out[it] = sum_r pt_r (.) (that), accumulated in registers (no [B][R] intermediate)
//   hoist_c0_kernel         : the 31-bit path's last step, H[it][r] += (c0 o perm_r, 0) in the NTT domain
//   hoist_ptsum_kernel      : the 31-bit path's linear transform, out[it] = sum_r pt_r (.) H[it][r]
// A rotation by the identity element (ident[r] != 0) reads no key: its output is the input ciphertext.
// The rotation kernels place output (item, r) at hoist_out_index(item, r, R, gs): gs = 1 is [item][R]; gs = d
// makes the d limbs of a dBFV ciphertext one group, [item / d][R][item % d] (items a multiple of d).
#include "exacto_internal.hpp"

namespace exacto {

static constexpr int HO_TPB = 256;

// One thread per (item, limb l, position j).  Blocks are numbered item-fastest (as relin_mac_kernel), so the
// blocks resident together share a few key slices.  The gathered reads (c0 and the guse digit rows at
// l n + perm_r[j]) are 8-byte reads scattered inside one n-word row; the key, the plaintexts and the output
// are coalesced.  Accumulators stay in [0, 2q); D and the ciphertext are canonical.
template <bool LT>
__global__ void __launch_bounds__(HO_TPB)
hoist_mac_kernel(const u64* __restrict__ ct, const u64* __restrict__ D, const u64* __restrict__ keys,
                 const u64* __restrict__ keys_s, const uint32_t* __restrict__ perm,
                 const unsigned char* __restrict__ ident, const u64* __restrict__ pts, u64* __restrict__ out, int R,
                 int guse, int items, int nblk, int n, int L, const PrimeConst* __restrict__ primes, int gs) {
    const long Ln = (long)L * n;
    const unsigned it = blockIdx.x % (unsigned)items;
    const unsigned rest = blockIdx.x / (unsigned)items;
    const unsigned blk = rest % (unsigned)nblk;
    const long coef = (long)blk * HO_TPB + threadIdx.x;
    if (coef >= Ln) return;
    const int l = (int)(coef / n);
    const int j = (int)(coef - (long)l * n);
    const PrimeConst& P = primes[l];
    const u64 q = P.q, q2 = P.two_q, nq = (u64)0 - q;
    const u64* c0 = ct + (long)it * 2 * Ln;
    const u64* dp = D + (long)it * guse * Ln;
    const int r_lo = LT ? 0 : (int)(rest / (unsigned)nblk), r_hi = LT ? R : r_lo + 1;
    u64 s0 = 0, s1 = 0;
    for (int r = r_lo; r < r_hi; ++r) {
        u64 a0, a1;
        if (ident[r]) {
            a0 = c0[coef];
            a1 = c0[Ln + coef];
        } else {
            const long src = (long)l * n + perm[(long)r * n + j];
            a0 = c0[src];
            a1 = 0;
            const u64* kp = keys + (long)r * guse * 2 * Ln + coef;
            const u64* ksp = keys_s + (long)r * guse * 2 * Ln + coef;
            constexpr int U = 4;
            for (int g0 = 0; g0 < guse; g0 += U) {
                u64 d[U], w0[U], h0[U], w1[U], h1[U];
#pragma unroll
                for (int t = 0; t < U; ++t) {
                    const int g = min(g0 + t, guse - 1);  // clamped (re-read) tail, masked below
                    d[t] = dp[(long)g * Ln + src];
                    w0[t] = kp[2L * g * Ln];
                    h0[t] = ksp[2L * g * Ln];
                    w1[t] = kp[2L * g * Ln + Ln];
                    h1[t] = ksp[2L * g * Ln + Ln];
                }
#pragma unroll
                for (int t = 0; t < U; ++t) {
                    if (g0 + t < guse) {
                        u64 v = a0 + shoup_mul_nq(d[t], w0[t], h0[t], nq);
                        a0 = v >= q2 ? v - q2 : v;
                        v = a1 + shoup_mul_nq(d[t], w1[t], h1[t], nq);
                        a1 = v >= q2 ? v - q2 : v;
                    }
                }
            }
            a0 = a0 >= q ? a0 - q : a0;
            a1 = a1 >= q ? a1 - q : a1;
        }
        if constexpr (LT) {
            const u64 m = pts[(long)r * Ln + coef];
            s0 = add_mod(s0, mul_mod(a0, m, P), q);
            s1 = add_mod(s1, mul_mod(a1, m, P), q);
        } else {
            u64* op = out + hoist_out_index(it, r, R, gs) * 2 * Ln;
            op[coef] = a0;
            op[Ln + coef] = a1;
        }
    }
    if constexpr (LT) {
        u64* op = out + (long)it * 2 * Ln;
        op[coef] = s0;
        op[Ln + coef] = s1;
    }
}

// The rotations (not the linear transform) with rotation r's key slice staged in LDS, after
// relin_mac_lds_kernel: a block owns 64 consecutive positions of one rotation and HO_IG items; the key words
// and Shoup companions of every digit (guse * 2 KiB) come from global memory once per block and the items'
// traffic is the gathered digits, c0 and the output.  Wave w handles items it0 + w, it0 + w + 4, ...
constexpr int HO_LS = 64;    // positions per block
constexpr int HO_IG = 64;    // items per block
constexpr int HO_GMAX = 32;  // digits staged (LDS = 2 KiB per digit)

__global__ void __launch_bounds__(HO_TPB)
hoist_mac_lds_kernel(const u64* __restrict__ ct, const u64* __restrict__ D, const u64* __restrict__ keys,
                     const u64* __restrict__ keys_s, const uint32_t* __restrict__ perm,
                     const unsigned char* __restrict__ ident, u64* __restrict__ out, int R, int guse, int items, int n,
                     int L, const PrimeConst* __restrict__ primes, int gs) {
    extern __shared__ u64 kst[];  // [guse][4][HO_LS]: w0, ws0, w1, ws1
    const long Ln = (long)L * n;
    const long c0 = (long)blockIdx.x * HO_LS;  // first position (flat limb * n + j)
    const int r = blockIdx.z;
    const int lane = threadIdx.x & (HO_LS - 1), wave = threadIdx.x / HO_LS;
    const long coef = c0 + lane;
    const int it_end = min(items, (int)(blockIdx.y + 1) * HO_IG);
    if (ident[r]) {   // block-uniform
        for (int it = blockIdx.y * HO_IG + wave; it < it_end; it += HO_TPB / HO_LS) {
            const u64* cp = ct + (long)it * 2 * Ln;
            u64* op = out + hoist_out_index(it, r, R, gs) * 2 * Ln;
            op[coef] = cp[coef];
            op[Ln + coef] = cp[Ln + coef];
        }
        return;
    }
    const u64* kp = keys + (long)r * guse * 2 * Ln;
    const u64* ksp = keys_s + (long)r * guse * 2 * Ln;
    for (int e = threadIdx.x; e < guse * 4 * HO_LS; e += HO_TPB) {
        const int g = e / (4 * HO_LS), w = (e / HO_LS) & 3, l = e & (HO_LS - 1);
        const long kk = (2L * g + (w >> 1)) * Ln + c0 + l;
        kst[e] = (w & 1) ? ksp[kk] : kp[kk];
    }
    __syncthreads();
    const int i = (int)(coef / n);
    const PrimeConst& P = primes[i];
    const u64 q = P.q, q2 = P.two_q, nq = (u64)0 - q;
    const long src = (long)i * n + perm[(long)r * n + (coef - (long)i * n)];
    for (int it = blockIdx.y * HO_IG + wave; it < it_end; it += HO_TPB / HO_LS) {
        u64 a0 = ct[(long)it * 2 * Ln + src], a1 = 0;
        const u64* dp = D + (long)it * guse * Ln + src;
        constexpr int U = 4;
        for (int g0 = 0; g0 < guse; g0 += U) {
            u64 d[U];
#pragma unroll
            for (int t = 0; t < U; ++t) d[t] = dp[(long)min(g0 + t, guse - 1) * Ln];
#pragma unroll
            for (int t = 0; t < U; ++t) {
                if (g0 + t < guse) {
                    const u64* kg = kst + (g0 + t) * 4 * HO_LS + lane;
                    u64 v = a0 + shoup_mul_nq(d[t], kg[0], kg[HO_LS], nq);
                    a0 = v >= q2 ? v - q2 : v;
                    v = a1 + shoup_mul_nq(d[t], kg[2 * HO_LS], kg[3 * HO_LS], nq);
                    a1 = v >= q2 ? v - q2 : v;
                }
            }
        }
        u64* op = out + hoist_out_index(it, r, R, gs) * 2 * Ln;
        op[coef] = a0 >= q ? a0 - q : a0;
        op[Ln + coef] = a1 >= q ? a1 - q : a1;
    }
}

void launch_hoist_mac(bool lt, const u64* ct, const u64* D, const u64* keys, const u64* keys_s, const uint32_t* perm,
                      const unsigned char* ident, const u64* pts, u64* out, int R, int guse, int items, int n, int L,
                      const PrimeConst* primes, hipStream_t s, int gs) {
    if (items <= 0 || R <= 0) return;
    const long Ln = (long)L * n;
    if (!lt && guse > 0 && guse <= HO_GMAX && Ln % HO_LS == 0 && R <= 65535) {
        const dim3 grid((unsigned)(Ln / HO_LS), (unsigned)((items + HO_IG - 1) / HO_IG), (unsigned)R);
        EXACTO_LAUNCH(hoist_mac_lds_kernel, grid, dim3(HO_TPB), (size_t)guse * 4 * HO_LS * sizeof(u64), s, ct, D, keys,
                      keys_s, perm, ident, out, R, guse, items, n, L, primes, gs);
        return;
    }
    const int nblk = (int)((Ln + HO_TPB - 1) / HO_TPB);
    const long blocks = (long)items * nblk * (lt ? 1 : R);
    if (lt)
        EXACTO_LAUNCH(hoist_mac_kernel<true>, dim3((unsigned)blocks), dim3(HO_TPB), 0, s, ct, D, keys, keys_s, perm,
                      ident, pts, out, R, guse, items, nblk, n, L, primes, gs);
    else
        EXACTO_LAUNCH(hoist_mac_kernel<false>, dim3((unsigned)blocks), dim3(HO_TPB), 0, s, ct, D, keys, keys_s, perm,
                      ident, pts, out, R, guse, items, nblk, n, L, primes, gs);
}

// H [items][R][2][L][n] (the key-switched sums, NTT domain) += (c0 o perm_r, 0); the identity element's
// sums are zero and it takes both components of the input as they are.
__global__ void __launch_bounds__(HO_TPB)
hoist_c0_kernel(const u64* __restrict__ ct, const uint32_t* __restrict__ perm, const unsigned char* __restrict__ ident,
                u64* __restrict__ H, int R, int nblk, int n, int L, const PrimeConst* __restrict__ primes,
                int gs) {
    const long Ln = (long)L * n;
    const unsigned ir = blockIdx.x / (unsigned)nblk;          // H's index: hoist_out_index(item, r, R, gs)
    const long coef = (long)(blockIdx.x - ir * (unsigned)nblk) * HO_TPB + threadIdx.x;
    if (coef >= Ln) return;
    const unsigned grp = ir / ((unsigned)R * gs), in_grp = ir - grp * ((unsigned)R * gs);
    const int r = (int)(in_grp / (unsigned)gs);
    const unsigned it = grp * gs + (in_grp - (unsigned)r * gs);
    const int l = (int)(coef / n);
    const int j = (int)(coef - (long)l * n);
    const u64 q = primes[l].q;
    const u64* c0 = ct + (long)it * 2 * Ln;
    u64* hp = H + (long)ir * 2 * Ln;
    if (ident[r]) {
        hp[coef] = add_mod(hp[coef], c0[coef], q);
        hp[Ln + coef] = add_mod(hp[Ln + coef], c0[Ln + coef], q);
    } else {
        hp[coef] = add_mod(hp[coef], c0[(long)l * n + perm[(long)r * n + j]], q);
    }
}

void launch_hoist_c0(const u64* ct, const uint32_t* perm, const unsigned char* ident, u64* H, int R, int items, int n,
                     int L, const PrimeConst* primes, hipStream_t s, int gs) {
    if (items <= 0 || R <= 0) return;
    const int nblk = (int)(((long)L * n + HO_TPB - 1) / HO_TPB);
    EXACTO_LAUNCH(hoist_c0_kernel, dim3((unsigned)((long)items * R * nblk)), dim3(HO_TPB), 0, s, ct, perm, ident, H, R,
                  nblk, n, L, primes, gs);
}

// out[it][c][l][j] = sum_r pts[r][l][j] H[it][r][c][l][j] mod q_l: one streaming pass over H
__global__ void __launch_bounds__(HO_TPB)
hoist_ptsum_kernel(const u64* __restrict__ H, const u64* __restrict__ pts, u64* __restrict__ out, int R, int nblk,
                   int n, int L, const PrimeConst* __restrict__ primes) {
    const long Ln = (long)L * n;
    const unsigned it = blockIdx.x / (unsigned)nblk;
    const long coef = (long)(blockIdx.x - it * (unsigned)nblk) * HO_TPB + threadIdx.x;
    if (coef >= Ln) return;
    const PrimeConst& P = primes[(int)(coef / n)];
    const u64* hp = H + (long)it * R * 2 * Ln + coef;
    u64 s0 = 0, s1 = 0;
    for (int r = 0; r < R; ++r) {
        const u64 m = pts[(long)r * Ln + coef];
        s0 = add_mod(s0, mul_mod(hp[(long)r * 2 * Ln], m, P), P.q);
        s1 = add_mod(s1, mul_mod(hp[(long)r * 2 * Ln + Ln], m, P), P.q);
    }
    out[(long)it * 2 * Ln + coef] = s0;
    out[(long)it * 2 * Ln + Ln + coef] = s1;
}

void launch_hoist_ptsum(const u64* H, const u64* pts, u64* out, int R, int items, int n, int L,
                        const PrimeConst* primes, hipStream_t s) {
    if (items <= 0 || R <= 0) return;
    const int nblk = (int)(((long)L * n + HO_TPB - 1) / HO_TPB);
    EXACTO_LAUNCH(hoist_ptsum_kernel, dim3((unsigned)((long)items * nblk)), dim3(HO_TPB), 0, s, H, pts, out, R, nblk, n,
                  L, primes);
}

}  // namespace exacto
