// Noise measurement (paper_repro.rs:238-281 max_limb_noise / bfv_noise_inf), exact for every L.
//
// For one ciphertext with phase x_j = CRT(INTT(sum_k c_k s^k))_j in [0, Q) (the decryption's dec_buf):
//   m_j   = the decrypted coefficient floor((x_j p + floor(Q/2)) / Q) mod p, or expected[j] mod p,
//   e_j   = (x_j - m_j Delta) mod Q,  Delta = floor(Q / p),
//   noise = max_j min(e_j, Q - e_j).
// L = 1 is bfv_noise_inf literally, in u64.  L >= 2 is the same formula over the full Q (the
// extension semantics of SURVEY §8(c); the reference looks at moduli[0] only).
//
// noise_kernel: a workgroup owns NOISE_CHUNK consecutive coefficients of one item; a thread strides
// over NOISE_CPT of them and keeps its running maximum as L mixed-radix digits in registers
// (digit i < q_i, so comparing digits from the top one down compares the values).  e's digits come
// from one Garner pass over its residues e_i = x_i - m Delta_i; above floor(Q/2) the digits of
// Q - e are the complement q_i - 1 - v_i plus one with carry (Q - 1 has the digits q_i - 1), not
// another Garner pass.  The workgroup's maximum (64 lanes by shuffles, 4 waves through LDS) goes to
// part[item][chunk][L].
// noise_final_kernel: one wave per output takes the maximum of its cnt partials (the chunks of a BFV
// item, or the chunks of all d limbs of a dBFV ciphertext), and lane 0 turns the winning digits into
// L little-endian binary words by Horner's rule.
// A maximum does not depend on the order of its operands, so the words are the same for every launch
// shape and from run to run.  Lanes past n contribute 0.
#include "exacto_internal.hpp"
#include "crt_dev.hpp"

namespace exacto {

static constexpr int NOISE_TPB = 256;
static constexpr int NOISE_CPT = 2;                      // coefficients per thread
static constexpr int NOISE_CHUNK = NOISE_TPB * NOISE_CPT;  // coefficients per workgroup

// a > b, most significant digit first
template <int LT>
__device__ __forceinline__ bool dig_greater(const u64 (&a)[EXACTO_MAX_L], const u64 (&b)[EXACTO_MAX_L]) {
    bool gt = false, open = true;
#pragma unroll
    for (int k = LT - 1; k >= 0; --k) {
        if (open && a[k] != b[k]) {
            gt = a[k] > b[k];
            open = false;
        }
    }
    return gt;
}

template <int LT>
__device__ __forceinline__ void dig_max(u64 (&best)[EXACTO_MAX_L], const u64 (&v)[EXACTO_MAX_L]) {
    if (dig_greater<LT>(v, best)) {
#pragma unroll
        for (int k = 0; k < LT; ++k) best[k] = v[k];
    }
}

// the maximum over the 64 lanes of a wave, left in every lane
template <int LT>
__device__ __forceinline__ void wave_max(u64 (&best)[EXACTO_MAX_L]) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        u64 o[EXACTO_MAX_L];
#pragma unroll
        for (int k = 0; k < LT; ++k) o[k] = (u64)__shfl_xor((unsigned long long)best[k], off, 64);
        dig_max<LT>(best, o);
    }
}

// X [items][L][n] (coefficient domain, canonical), expected / plain_out [items][n] or null,
// part [items][nchunk][L]; nchunk = max(1, n / NOISE_CHUNK) is a power of two; delta: Delta mod q_i at [i],
// its Shoup companion at [EXACTO_MAX_L + i].
// round: compute the decrypted coefficient (needed unless expected is given and plain_out is not).
template <int LT>
__global__ void __launch_bounds__(NOISE_TPB)
noise_kernel(const u64* __restrict__ X, const u64* __restrict__ expected, u64* __restrict__ plain_out,
             u64* __restrict__ part, int n, int nchunk, const CrtTables* __restrict__ C,
             const PrimeConst* __restrict__ primes, const u64* __restrict__ delta, u64 plain, int round) {
    const int csh = __builtin_ctz((unsigned)nchunk);
    const long item = (long)(blockIdx.x >> csh);
    const int j0 = (int)(blockIdx.x & (unsigned)(nchunk - 1)) * NOISE_CHUNK + (int)threadIdx.x;
    u64 best[EXACTO_MAX_L];
#pragma unroll
    for (int k = 0; k < EXACTO_MAX_L; ++k) best[k] = 0;

#pragma unroll
    for (int c = 0; c < NOISE_CPT; ++c) {
        const int j = j0 + c * NOISE_TPB;
        if (j >= n) continue;
        u64 v[EXACTO_MAX_L];
        if (LT == 1) {
            // bfv_noise_inf (paper_repro.rs:249-281) in u64: one 128-by-64 division for the rounding
            const u64 q = primes[0].q;
            const u64 x = X[item * n + j];
            u64 m = 0;
            if (round) {
                const u128 y = (u128)x * plain + (q >> 1);
                const u64 r = (u64)(y / q);
                m = r >= plain ? r - plain : r;  // r <= p
                if (plain_out) plain_out[item * n + j] = m;
            }
            if (expected) m = expected[item * n + j] % plain;
            const u64 target = m * delta[0];  // m < p: below q, no reduction needed
            const u64 raw = x >= target ? x - target : x + q - target;
            v[0] = raw < q - raw ? raw : q - raw;
        } else {
            u64 x[EXACTO_MAX_L], e[EXACTO_MAX_L];
#pragma unroll
            for (int i = 0; i < LT; ++i) x[i] = X[(item * LT + i) * n + j];
            u64 m = 0;
            if (round) {
                // decrypt_round_kernel's r (kernels.hip): exact in the first auxiliary prime P0 > p
                u64 s[EXACTO_MAX_L], vx[EXACTO_MAX_L], vs[EXACTO_MAX_L];
#pragma unroll
                for (int i = 0; i < LT; ++i) {
                    const u64 qi = primes[i].q;
                    s[i] = add_mod(shoup_mul_red(x[i], C->pmod_w[i], C->pmod_ws[i], qi), C->hq[i], qi);
                }
                garner_q<false>(vx, x, LT, C, primes);
                garner_q<false>(vs, s, LT, C, primes);
                const PrimeConst& P0 = primes[LT];
                const u64 p0 = P0.q;
                const u64 xP = mr_eval<EXACTO_MAX_L, EXACTO_MAX_PRIMES, false>(vx, LT, false, &C->qpref_w[0][0],
                                                                               &C->qpref_ws[0][0], LT, P0);
                const u64 sP = mr_eval<EXACTO_MAX_L, EXACTO_MAX_PRIMES, false>(vs, LT, false, &C->qpref_w[0][0],
                                                                               &C->qpref_ws[0][0], LT, P0);
                const u64 a = shoup_mul_red(xP, C->pq_w[0], C->pq_ws[0], p0);
                const u64 b = shoup_mul_red(sub_mod(C->hq[LT], sP, p0), C->qinvp_w[0], C->qinvp_ws[0], p0);
                const u64 r = add_mod(a, b, p0);
                m = r >= plain ? r - plain : r;  // r <= p
                if (plain_out) plain_out[item * n + j] = m;
            }
            if (expected) m = expected[item * n + j] % plain;
#pragma unroll
            for (int i = 0; i < LT; ++i) {
                const u64 qi = primes[i].q;   // a Shoup product takes any 64-bit m
                e[i] = sub_mod(x[i], shoup_mul_red(m, delta[i], delta[EXACTO_MAX_L + i], qi), qi);
            }
            garner_q<false>(v, e, LT, C, primes);
            if (mr_greater(v, C->halfQ_mr, LT)) {
                // Q - e: complement every digit (Q - 1 - e), then add one with carry
                u64 carry = 1;
#pragma unroll
                for (int i = 0; i < LT; ++i) {
                    const u64 qi = primes[i].q;
                    u64 w = qi - 1 - v[i] + carry;
                    carry = w == qi ? 1 : 0;
                    v[i] = carry ? 0 : w;
                }
            }
        }
        dig_max<LT>(best, v);
    }

    wave_max<LT>(best);
    __shared__ u64 sm[NOISE_TPB / 64][EXACTO_MAX_L];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < LT; ++k) sm[wave][k] = best[k];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int w = 1; w < NOISE_TPB / 64; ++w) {
            u64 o[EXACTO_MAX_L];
#pragma unroll
            for (int k = 0; k < LT; ++k) o[k] = sm[w][k];
            dig_max<LT>(best, o);
        }
#pragma unroll
        for (int k = 0; k < LT; ++k) part[(long)blockIdx.x * LT + k] = best[k];
    }
}

// part [outs][cnt][L] mixed-radix digits -> out [outs][L] little-endian binary words of the maximum
template <int LT>
__global__ void __launch_bounds__(64)
noise_final_kernel(const u64* __restrict__ part, int cnt, u64* __restrict__ out,
                   const PrimeConst* __restrict__ primes) {
    const long o = blockIdx.x;
    u64 best[EXACTO_MAX_L];
#pragma unroll
    for (int k = 0; k < EXACTO_MAX_L; ++k) best[k] = 0;
    for (int t = threadIdx.x; t < cnt; t += 64) {
        u64 v[EXACTO_MAX_L];
#pragma unroll
        for (int k = 0; k < LT; ++k) v[k] = part[(o * cnt + t) * LT + k];
        dig_max<LT>(best, v);
    }
    wave_max<LT>(best);
    if (threadIdx.x != 0) return;
    // Horner: ((v_{L-1} q_{L-2} + v_{L-2}) q_{L-3} + ...) q_0 + v_0 < Q < 2^(64 L)
    u64 w[EXACTO_MAX_L];
#pragma unroll
    for (int k = 0; k < LT; ++k) w[k] = 0;
    w[0] = best[LT - 1];
#pragma unroll
    for (int i = LT - 2; i >= 0; --i) {
        const u64 qi = primes[i].q;
        u64 carry = best[i];
#pragma unroll
        for (int k = 0; k < LT; ++k) {
            const u128 t = (u128)w[k] * qi + carry;
            w[k] = (u64)t;
            carry = (u64)(t >> 64);
        }
    }
#pragma unroll
    for (int k = 0; k < LT; ++k) out[o * LT + k] = w[k];
}

int noise_chunks(int n) { return n > NOISE_CHUNK ? n / NOISE_CHUNK : 1; }

template <int LT>
static void launch_noise_t(const u64* X, const u64* expected, u64* plain_out, u64* part, u64* out, long items,
                           int group, int n, const CrtTables* ct, const PrimeConst* primes, const u64* delta,
                           u64 plain, bool round, hipStream_t s) {
    const int nchunk = noise_chunks(n);
    EXACTO_LAUNCH((noise_kernel<LT>), dim3(items * nchunk), dim3(NOISE_TPB), 0, s, X, expected, plain_out, part, n,
                  nchunk, ct, primes, delta, plain, round ? 1 : 0);
    EXACTO_LAUNCH((noise_final_kernel<LT>), dim3(items / group), dim3(64), 0, s, part, group * nchunk, out, primes);
}

void launch_noise(const u64* X, const u64* expected, u64* plain_out, u64* part, u64* out, long items, int group,
                  int n, int L, const CrtTables* ct, const PrimeConst* primes, const u64* delta, u64 plain,
                  bool round, hipStream_t s) {
    if (items == 0) return;
#define NOISE_CASE(LT_) \
    case LT_: launch_noise_t<LT_>(X, expected, plain_out, part, out, items, group, n, ct, primes, delta, plain, round, s); break
    switch (L) {
        NOISE_CASE(1); NOISE_CASE(2); NOISE_CASE(3); NOISE_CASE(4);
        NOISE_CASE(5); NOISE_CASE(6); NOISE_CASE(7); NOISE_CASE(8);
        default: break;
    }
#undef NOISE_CASE
}

}  // namespace exacto
