// SIMD batching: slot encode / decode modulo the plaintext prime t < 2^32 (t == 1 mod 2n).
//
// With zeta = find_psi(n, t), e_i = 3^i mod 2n and the slot vector seen as a 2 x n/2 matrix, the
// plaintext m(X) of `values` has m(zeta^e_i) = values[i] and m(zeta^(2n - e_i)) = values[n/2 + i].
// In the library's evaluation numbering (evaluation k = a(psi^(2 brv(k) + 1)), stored at position
// (k mod 16) n/16 + k / 16) slot exponent e is evaluation brv((e - 1) / 2), so
//   encode = place the values by a fixed permutation, inverse negacyclic transform mod t, n^-1;
//   decode = forward transform, read through the same permutation.
// The permutation table perm[slot] is that storage position, which is also the conflict-free LDS word
// the transform's threads read their evaluations from (thread tid holds evaluations 16 tid + k at
// words k n/16 + tid), so it is applied on the way into LDS (encode) or out of it (decode): the
// global loads and stores are the contiguous u64 rows of the ABI, 8n bytes each way per polynomial.
//
// One workgroup per polynomial.  n >= 1024: n/16 threads x 16 values in registers, the radix-16
// rounds and LDS transposes of ks32_dev.hpp (4n bytes of LDS).  Arithmetic by template parameter:
//   F32_LAZY  t < 2^30   lazy [0, 4t) / [0, 2t) butterflies,
//   F32_WIDE  t < 2^31   values below 2t, operands reduced,
//   BF_STRICT t < 2^32   canonical values throughout, the Shoup remainder (below 2t: 33 bits)
//                        carried in 64 bits.
// n < 1024 (tests and the reference's small presets): an LDS-resident radix-2 kernel, canonical
// values, the same two remainder widths.
#include "exacto_internal.hpp"
#include "ks32_dev.hpp"

namespace exacto {

// ---------------------------------------------------------------- arithmetic mod t

// any u64 -> [0, t): Barrett with mu = floor((2^64 - 1) / t) (quotient at most 2 short)
__device__ __forceinline__ uint32_t batch_reduce(u64 v, uint32_t t, u64 mu) {
    if (v < t) return (uint32_t)v;
    u64 r = v - __umul64hi(v, mu) * t;
    r = r >= t ? r - t : r;
    r = r >= t ? r - t : r;
    return (uint32_t)r;
}

// canonical operands and results; WIDE64: t may reach 2^32 - 1
template <bool WIDE64>
__device__ __forceinline__ uint32_t bmul(uint32_t x, uint32_t w, uint32_t ws, uint32_t p) {
    if constexpr (WIDE64) {
        const u64 r = (u64)x * w - (u64)__umulhi(x, ws) * p;   // in [0, 2p)
        return (uint32_t)(r >= p ? r - p : r);
    } else {
        return red32(shoup32(x, w, ws, p), p);
    }
}
template <bool WIDE64>
__device__ __forceinline__ uint32_t badd(uint32_t a, uint32_t b, uint32_t p) {
    if constexpr (WIDE64) {
        const u64 s = (u64)a + b;
        return (uint32_t)(s >= p ? s - p : s);
    } else {
        return red32(a + b, p);
    }
}
template <bool WIDE64>
__device__ __forceinline__ uint32_t bsub(uint32_t a, uint32_t b, uint32_t p) {
    return a >= b ? a - b : a - b + p;   // the wrapped a - b + p is the residue for any p < 2^32
}

// ---------------------------------------------------------------- strict radix-16 rounds (t < 2^32)

// the round structure of fwd32_round / inv32_round with canonical values between stages
template <int LOGN, int LO, int BHI>
__device__ __forceinline__ void sfwd_round(uint32_t (&x)[16], int tid, Tw32 tw, uint32_t p) {
    constexpr int N = 1 << LOGN;
    const int thigh = (LO + 4 >= LOGN) ? 0 : (tid >> LO);
#pragma unroll
    for (int b = BHI; b >= LO; --b) {
        const int lb = b - LO, half = 1 << lb;
        const int base = (N >> (b + 1)) + (thigh << (LO + 3 - b));
#pragma unroll
        for (int g = 0; g < (8 >> lb); ++g) {
            const uint2 t = make_uint2(tw[base + g].x, tw[base + g].y);
#pragma unroll
            for (int m = 0; m < half; ++m) {
                const int k0 = g * 2 * half + m, k1 = k0 + half;
                const uint32_t X = x[k0], T = bmul<true>(x[k1], t.x, t.y, p);
                x[k0] = badd<true>(X, T, p);
                x[k1] = bsub<true>(X, T, p);
            }
        }
    }
}

template <int LOGN, int R>
__device__ __forceinline__ void sfwd_rounds(uint32_t (&x)[16], uint32_t* lds, int tid, Tw32 tw, uint32_t p) {
    constexpr int LO = (LOGN - 4 * (R + 1)) > 0 ? (LOGN - 4 * (R + 1)) : 0;
    constexpr int BHI = LOGN - 1 - 4 * R;
    if constexpr (R > 0) {
        constexpr int PLO = (LOGN - 4 * R) > 0 ? (LOGN - 4 * R) : 0;
        lds_sync();
        lds32_store<PLO>(lds, x, tid);
        lds_sync();
        lds32_load<LO>(lds, x, tid);
    }
    sfwd_round<LOGN, LO, BHI>(x, tid, tw, p);
    if constexpr (LO > 0) sfwd_rounds<LOGN, R + 1>(x, lds, tid, tw, p);
}

template <int LOGN, int LO, int BLO, int BHI>
__device__ __forceinline__ void sinv_round(uint32_t (&x)[16], int tid, const Prime32& P) {
    constexpr int N = 1 << LOGN;
    const uint32_t p = P.p;
    const Tw32 twi = tw32(P.tw_inv);
    const int thigh = (LO + 4 >= LOGN) ? 0 : (tid >> LO);
#pragma unroll
    for (int b = BLO; b <= BHI; ++b) {
        const int lb = b - LO, half = 1 << lb;
        const int base = (N >> (b + 1)) + (thigh << (LO + 3 - b));
#pragma unroll
        for (int g = 0; g < (8 >> lb); ++g) {
            uint2 t = make_uint2(0, 0);
            if (b != LOGN - 1) t = make_uint2(twi[base + g].x, twi[base + g].y);
#pragma unroll
            for (int m = 0; m < half; ++m) {
                const int k0 = g * 2 * half + m, k1 = k0 + half;
                const uint32_t U = x[k0], V = x[k1];
                const uint32_t s = badd<true>(U, V, p), d = bsub<true>(U, V, p);
                if (b == LOGN - 1) {   // n^-1 folded into the last stage
                    x[k0] = bmul<true>(s, P.n_inv, P.n_inv_s, p);
                    x[k1] = bmul<true>(d, P.last_w, P.last_ws, p);
                } else {
                    x[k0] = s;
                    x[k1] = bmul<true>(d, t.x, t.y, p);
                }
            }
        }
    }
}

template <int LOGN, int R>
__device__ __forceinline__ void sinv_rounds(uint32_t (&x)[16], uint32_t* lds, int tid, const Prime32& P) {
    constexpr int LO = (4 * R) < (LOGN - 4) ? 4 * R : LOGN - 4;
    constexpr int BLO = 4 * R;
    constexpr int BHI = (4 * R + 3) < (LOGN - 1) ? 4 * R + 3 : LOGN - 1;
    if constexpr (R > 0) {
        constexpr int PLO = (4 * (R - 1)) < (LOGN - 4) ? 4 * (R - 1) : LOGN - 4;
        lds_sync();
        lds32_store<PLO>(lds, x, tid);
        lds_sync();
        lds32_load<LO>(lds, x, tid);
    }
    sinv_round<LOGN, LO, BLO, BHI>(x, tid, P);
    if constexpr (BHI < LOGN - 1) sinv_rounds<LOGN, R + 1>(x, lds, tid, P);
}

// ---------------------------------------------------------------- n >= 1024

typedef const uint32_t __attribute__((address_space(1)))* Perm32;

// values [B][n] (any u64, reduced mod t here) -> plaintext coefficients [B][n] in [0, t); out == in allowed
template <int LOGN, int FORM>
__global__ void __launch_bounds__((1 << LOGN) / 16)
batch_encode_kernel(const u64* __restrict__ in, u64* __restrict__ out, BatchTab tab) {
    constexpr int N = 1 << LOGN, T = N / 16;
    __shared__ uint32_t lds[N];
    const int tid = threadIdx.x;
    const long b = blockIdx.x;
    const Prime32& P = tab.P;
    const __amdgpu_buffer_rsrc_t ri = poly_rsrc(in + b * N, N * 8);
    const __amdgpu_buffer_rsrc_t ro = poly_rsrc(out + b * N, N * 8);
    const Perm32 perm = (Perm32)tab.perm;
    uint32_t x[16];
    // slot tid + k T -> its evaluation's LDS word
#pragma unroll
    for (int k = 0; k < 16; ++k) x[k] = batch_reduce(buf_ld64(ri, tid * 8, k * T * 8), P.p, tab.mu);
#pragma unroll
    for (int k = 0; k < 16; ++k) lds[perm[tid + k * T]] = x[k];
    lds_sync();
#pragma unroll
    for (int k = 0; k < 16; ++k) x[k] = lds[k * T + tid];   // evaluation 16 tid + k
    if constexpr (FORM == BF_STRICT) sinv_rounds<LOGN, 0>(x, lds, tid, P);
    else inv32_rounds<LOGN, 0, FORM == F32_LAZY>(x, lds, tid, P);
    // coefficient k T + tid, canonical
#pragma unroll
    for (int k = 0; k < 16; ++k) buf_st64(ro, (u64)x[k], tid * 8, k * T * 8);
}

// plaintext coefficients [B][n] (any u64, reduced mod t here) -> values [B][n]; out == in allowed
template <int LOGN, int FORM>
__global__ void __launch_bounds__((1 << LOGN) / 16)
batch_decode_kernel(const u64* __restrict__ in, u64* __restrict__ out, BatchTab tab) {
    constexpr int N = 1 << LOGN, T = N / 16;
    __shared__ uint32_t lds[N];
    const int tid = threadIdx.x;
    const long b = blockIdx.x;
    const Prime32& P = tab.P;
    const uint32_t p = P.p;
    const __amdgpu_buffer_rsrc_t ri = poly_rsrc(in + b * N, N * 8);
    const __amdgpu_buffer_rsrc_t ro = poly_rsrc(out + b * N, N * 8);
    const Perm32 perm = (Perm32)tab.perm;
    uint32_t x[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) x[k] = batch_reduce(buf_ld64(ri, tid * 8, k * T * 8), p, tab.mu);
    if constexpr (FORM == BF_STRICT) {
        sfwd_rounds<LOGN, 0>(x, lds, tid, tw32(P.tw_fwd), p);
    } else {
        fwd32_rounds<LOGN, 0, FORM>(x, lds, tid, tw32(P.tw_fwd), p);
#pragma unroll
        for (int k = 0; k < 16; ++k)   // lazy [0, 4t) / wide [0, 2t) -> [0, t)
            x[k] = FORM == F32_WIDE ? red32(x[k], p) : red32(min(x[k], x[k] - 2 * p), p);
    }
    // evaluation 16 tid + k to its storage position, then slot by slot through the permutation
    lds_sync();
#pragma unroll
    for (int k = 0; k < 16; ++k) lds[k * T + tid] = x[k];
    lds_sync();
#pragma unroll
    for (int k = 0; k < 16; ++k) x[k] = lds[perm[tid + k * T]];
#pragma unroll
    for (int k = 0; k < 16; ++k) buf_st64(ro, (u64)x[k], tid * 8, k * T * 8);
}

// ---------------------------------------------------------------- n < 1024

// n / 2 threads, one butterfly per thread and stage (oracle/ring.py NttPlan.fwd / inv literally); the
// LDS image is in evaluation order k, perm's storage position p is evaluation ((p mod n/16) << 4) | p / (n/16)
template <bool ENCODE, bool WIDE64>
__global__ void __launch_bounds__(256)
batch_small_kernel(const u64* __restrict__ in, u64* __restrict__ out, int n, BatchTab tab) {
    __shared__ uint32_t a[512];
    const int tid = threadIdx.x, nt = n >> 1, T = n >> 4;
    const long b = blockIdx.x;
    const Prime32& P = tab.P;
    const uint32_t p = P.p;
    const u64* src = in + b * n;
    u64* dst = out + b * n;
    for (int j = tid; j < n; j += nt) {
        const uint32_t v = batch_reduce(src[j], p, tab.mu);
        if constexpr (ENCODE) {
            const int pos = (int)tab.perm[j];
            a[((pos % T) << 4) | (pos / T)] = v;
        } else {
            a[j] = v;
        }
    }
    __syncthreads();
    if constexpr (ENCODE) {
        int t = 1;
        for (int m = n; m > 1; m >>= 1) {
            const int h = m >> 1, i = tid / t, j = 2 * i * t + tid % t;
            const uint2 s = P.tw_inv[h + i];
            const uint32_t u = a[j], v = a[j + t];
            a[j] = badd<WIDE64>(u, v, p);
            a[j + t] = bmul<WIDE64>(bsub<WIDE64>(u, v, p), s.x, s.y, p);
            __syncthreads();
            t <<= 1;
        }
        for (int j = tid; j < n; j += nt) dst[j] = (u64)bmul<WIDE64>(a[j], P.n_inv, P.n_inv_s, p);
    } else {
        int t = n;
        for (int m = 1; m < n; m <<= 1) {
            t >>= 1;
            const int i = tid / t, j = 2 * i * t + tid % t;
            const uint2 s = P.tw_fwd[m + i];
            const uint32_t u = a[j], v = bmul<WIDE64>(a[j + t], s.x, s.y, p);
            a[j] = badd<WIDE64>(u, v, p);
            a[j + t] = bsub<WIDE64>(u, v, p);
            __syncthreads();
        }
        for (int j = tid; j < n; j += nt) {
            const int pos = (int)tab.perm[j];
            dst[j] = (u64)a[((pos % T) << 4) | (pos / T)];
        }
    }
}

// ---------------------------------------------------------------- slot-packed dBFV
//
// n wide integers mod p per dBFV ciphertext: digit k of every slot value, slot-encoded, is the plaintext
// of limb k.  One workgroup per item loops over the d digits, so the [d][n] digit vectors never exist in
// memory: the encode reads the item's n values once and writes d rows, the decode reads d rows and
// writes n values once.  The transforms, the LDS image (4n bytes) and the three arithmetic forms are
// those of batch_encode_kernel / batch_decode_kernel.
//
// The recomposition is dbfv_recompose_kernel's rule (sum of centred digit times b^k in i128 with
// wrapping, then mod p; p = 0: truncation to 64 bits) in the cheapest accumulator that gives its bits:
//   DB_U64   p = 0: truncation commutes with wrapping add and multiply, so the sum is kept in 64 bits;
//   DB_I64   floor(t / 2) (1 + b + ... + b^(d-1)) < 2^63: nothing wraps and the sum fits a signed
//            64-bit word, reduced by Barrett with mu = floor((2^64 - 1) / p);
//   DB_I128  everything else: the rule literally.
enum { DB_U64 = 0, DB_I64 = 1, DB_I128 = 2 };

struct DbfvBatchArgs {
    int d, shift;   // digits; log2(b) when b is a power of two, else -1
    u64 base, p;    // p = 0: 2^64
    u64 pmu;        // floor((2^64 - 1) / p), 0 for p = 0
};

// The tables are the same for every digit, and the compiler would otherwise keep a whole transform's
// twiddles in registers across the digit loop (about 30 more VGPRs, and scratch in every n = 16384 form):
// the pointer is made opaque once per digit, so each pass loads what it needs as the one-polynomial
// kernels do.
template <class T>
__device__ __forceinline__ T db_fresh(T ptr) {
    asm volatile("" : "+s"(ptr));
    return ptr;
}

template <int MODE> struct DbAcc { typedef u64 type; };
template <> struct DbAcc<DB_I128> { typedef u128 type; };

// acc += centred(x) b^k with power = b^k (wrapping in the accumulator's width)
template <int MODE>
__device__ __forceinline__ void db_accumulate(typename DbAcc<MODE>::type& acc, uint32_t x, uint32_t t, uint32_t half_t,
                                              typename DbAcc<MODE>::type power) {
    typedef typename DbAcc<MODE>::type A;
    const A centred = x > half_t ? (A)x - (A)t : (A)x;   // wraps to the two's-complement negative
    acc += centred * power;
}

template <int MODE>
__device__ __forceinline__ u64 db_finish(typename DbAcc<MODE>::type acc, const DbfvBatchArgs& a) {
    if constexpr (MODE == DB_U64) {
        return acc;
    } else if constexpr (MODE == DB_I64) {
        return signed_mod((i64)acc, a.p, a.pmu);
    } else {
        if ((i128)acc >= 0) return (u64)(acc % a.p);
        const u64 m = (u64)((~acc + 1) % a.p);   // |sum| mod p
        return m == 0 ? 0 : a.p - m;
    }
}

// values [B][n] (reduced mod p; as they are for p = 0) -> pt [B][d][n], row k the slot encoding of the k-th digits
template <int LOGN, int FORM>
__global__ void __launch_bounds__((1 << LOGN) / 16)
dbfv_batch_encode_kernel(const u64* __restrict__ in, u64* __restrict__ out, BatchTab tab, DbfvBatchArgs a) {
    constexpr int N = 1 << LOGN, T = N / 16;
    __shared__ uint32_t lds[N];
    const int tid = threadIdx.x;
    const long b = blockIdx.x;
    const Prime32& P = tab.P;
    const __amdgpu_buffer_rsrc_t ri = poly_rsrc(in + b * N, N * 8);
    const Perm32 perm = (Perm32)tab.perm;
    u64 v[16];   // what is left of slot tid + k T after the digits peeled so far
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        v[k] = buf_ld64(ri, tid * 8, k * T * 8);
        if (a.p) v[k] = reduce64(v[k], a.p, a.pmu);
    }
    Prime32 Pk = P;
    for (int dk = 0; dk < a.d; ++dk) {
        const __amdgpu_buffer_rsrc_t ro = poly_rsrc(out + (b * a.d + dk) * N, N * 8);
        const Perm32 pm = db_fresh(perm);
        Pk.tw_inv = db_fresh(P.tw_inv);
        uint32_t x[16];
        lds_sync();   // the previous digit's transposes are read
        // digits are below b <= t: canonical as they are
#pragma unroll
        for (int k = 0; k < 16; ++k) lds[pm[tid + k * T]] = (uint32_t)dbfv_digit_next(v[k], a.base, a.shift);
        lds_sync();
#pragma unroll
        for (int k = 0; k < 16; ++k) x[k] = lds[k * T + tid];   // evaluation 16 tid + k
        if constexpr (FORM == BF_STRICT) sinv_rounds<LOGN, 0>(x, lds, tid, Pk);
        else inv32_rounds<LOGN, 0, FORM == F32_LAZY>(x, lds, tid, Pk);
#pragma unroll
        for (int k = 0; k < 16; ++k) buf_st64(ro, (u64)x[k], tid * 8, k * T * 8);
    }
}

// pt [B][d][n] (any u64, reduced mod t here) -> values [B][n] = sum_k centred(decode(pt[k])) b^k mod p
template <int LOGN, int FORM, int MODE>
__global__ void __launch_bounds__((1 << LOGN) / 16)
dbfv_batch_decode_kernel(const u64* __restrict__ in, u64* __restrict__ out, BatchTab tab, DbfvBatchArgs a) {
    typedef typename DbAcc<MODE>::type A;
    constexpr int N = 1 << LOGN, T = N / 16;
    __shared__ uint32_t lds[N];
    const int tid = threadIdx.x;
    const long b = blockIdx.x;
    const Prime32& P = tab.P;
    const uint32_t p = P.p, half_t = p / 2;
    const Perm32 perm = (Perm32)tab.perm;
    // 16 sums per thread, except where 16 u128 sums (64 registers) cannot sit next to the transform in the 128
    // registers of a 1024-thread group: there the digits are walked four times, for 4 slots per thread each time.
    constexpr int PASSES = (LOGN == 14 && MODE == DB_I128) ? 4 : 1, W = 16 / PASSES;
    // The next row is loaded while this one is transformed wherever 32 more registers fit: with one workgroup
    // per item and few items a compute unit holds too few waves to hide the loads behind each other's arithmetic.
    constexpr bool AHEAD = LOGN <= 13 && MODE != DB_I128;
    const __amdgpu_buffer_rsrc_t ro = poly_rsrc(out + b * N, N * 8);
#pragma unroll 1
    for (int h = 0; h < PASSES; ++h) {
        A acc[W], power = 1;
#pragma unroll
        for (int k = 0; k < W; ++k) acc[k] = 0;
        u64 nx[16];
        if constexpr (AHEAD) {
            const __amdgpu_buffer_rsrc_t r0 = poly_rsrc(in + b * a.d * N, N * 8);
#pragma unroll
            for (int k = 0; k < 16; ++k) nx[k] = buf_ld64(r0, tid * 8, k * T * 8);
        }
        for (int dk = 0; dk < a.d; ++dk) {
            const Perm32 pm = db_fresh(perm);
            const Tw32 tw = db_fresh(tw32(P.tw_fwd));
            uint32_t x[16];
            if constexpr (AHEAD) {
#pragma unroll
                for (int k = 0; k < 16; ++k) x[k] = batch_reduce(nx[k], p, tab.mu);
                if (dk + 1 < a.d) {
                    const __amdgpu_buffer_rsrc_t rn = poly_rsrc(in + (b * a.d + dk + 1) * N, N * 8);
#pragma unroll
                    for (int k = 0; k < 16; ++k) nx[k] = buf_ld64(rn, tid * 8, k * T * 8);
                }
            } else {
                const __amdgpu_buffer_rsrc_t ri = poly_rsrc(in + (b * a.d + dk) * N, N * 8);
#pragma unroll
                for (int k = 0; k < 16; ++k) x[k] = batch_reduce(buf_ld64(ri, tid * 8, k * T * 8), p, tab.mu);
            }
            lds_sync();   // the previous digit's slots are read
            if constexpr (FORM == BF_STRICT) {
                sfwd_rounds<LOGN, 0>(x, lds, tid, tw, p);
            } else {
                fwd32_rounds<LOGN, 0, FORM>(x, lds, tid, tw, p);
#pragma unroll
                for (int k = 0; k < 16; ++k)   // lazy [0, 4t) / wide [0, 2t) -> [0, t)
                    x[k] = FORM == F32_WIDE ? red32(x[k], p) : red32(min(x[k], x[k] - 2 * p), p);
            }
            lds_sync();
#pragma unroll
            for (int k = 0; k < 16; ++k) lds[k * T + tid] = x[k];
            lds_sync();
#pragma unroll
            for (int k = 0; k < W; ++k)
                db_accumulate<MODE>(acc[k], lds[pm[tid + (h * W + k) * T]], p, half_t, power);
            power *= (A)a.base;
        }
#pragma unroll
        for (int k = 0; k < W; ++k) buf_st64(ro, db_finish<MODE>(acc[k], a), tid * 8, (h * W + k) * T * 8);
    }
}

// n < 1024: batch_small_kernel's LDS image and butterflies, n / 2 threads with slots tid and tid + n / 2
template <bool WIDE64>
__global__ void __launch_bounds__(256)
dbfv_batch_encode_small_kernel(const u64* __restrict__ in, u64* __restrict__ out, int n, BatchTab tab,
                               DbfvBatchArgs a) {
    __shared__ uint32_t lds[512];
    const int tid = threadIdx.x, nt = n >> 1, T = n >> 4;
    const long b = blockIdx.x;
    const Prime32& P = tab.P;
    const uint32_t p = P.p;
    u64 v[2];
    int at[2];
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        const int j = tid + r * nt, pos = (int)tab.perm[j];
        v[r] = in[b * n + j];
        if (a.p) v[r] = reduce64(v[r], a.p, a.pmu);
        at[r] = ((pos % T) << 4) | (pos / T);
    }
    for (int dk = 0; dk < a.d; ++dk) {
        u64* dst = out + (b * a.d + dk) * n;
        __syncthreads();   // the previous digit's row is read
#pragma unroll
        for (int r = 0; r < 2; ++r) lds[at[r]] = (uint32_t)dbfv_digit_next(v[r], a.base, a.shift);
        __syncthreads();
        int t = 1;
        for (int m = n; m > 1; m >>= 1) {
            const int h = m >> 1, i = tid / t, j = 2 * i * t + tid % t;
            const uint2 s = P.tw_inv[h + i];
            const uint32_t u = lds[j], w = lds[j + t];
            lds[j] = badd<WIDE64>(u, w, p);
            lds[j + t] = bmul<WIDE64>(bsub<WIDE64>(u, w, p), s.x, s.y, p);
            __syncthreads();
            t <<= 1;
        }
#pragma unroll
        for (int r = 0; r < 2; ++r) dst[tid + r * nt] = (u64)bmul<WIDE64>(lds[tid + r * nt], P.n_inv, P.n_inv_s, p);
    }
}

template <bool WIDE64, int MODE>
__global__ void __launch_bounds__(256)
dbfv_batch_decode_small_kernel(const u64* __restrict__ in, u64* __restrict__ out, int n, BatchTab tab,
                               DbfvBatchArgs a) {
    typedef typename DbAcc<MODE>::type A;
    __shared__ uint32_t lds[512];
    const int tid = threadIdx.x, nt = n >> 1, T = n >> 4;
    const long b = blockIdx.x;
    const Prime32& P = tab.P;
    const uint32_t p = P.p, half_t = p / 2;
    int at[2];
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        const int pos = (int)tab.perm[tid + r * nt];
        at[r] = ((pos % T) << 4) | (pos / T);
    }
    A acc[2] = {0, 0}, power = 1;
    for (int dk = 0; dk < a.d; ++dk) {
        const u64* src = in + (b * a.d + dk) * n;
        __syncthreads();   // the previous digit's slots are read
#pragma unroll
        for (int r = 0; r < 2; ++r) lds[tid + r * nt] = batch_reduce(src[tid + r * nt], p, tab.mu);
        __syncthreads();
        int t = n;
        for (int m = 1; m < n; m <<= 1) {
            t >>= 1;
            const int i = tid / t, j = 2 * i * t + tid % t;
            const uint2 s = P.tw_fwd[m + i];
            const uint32_t u = lds[j], w = bmul<WIDE64>(lds[j + t], s.x, s.y, p);
            lds[j] = badd<WIDE64>(u, w, p);
            lds[j + t] = bsub<WIDE64>(u, w, p);
            __syncthreads();
        }
#pragma unroll
        for (int r = 0; r < 2; ++r) db_accumulate<MODE>(acc[r], lds[at[r]], p, half_t, power);
        power *= (A)a.base;
    }
#pragma unroll
    for (int r = 0; r < 2; ++r) out[b * n + tid + r * nt] = db_finish<MODE>(acc[r], a);
}

// ---------------------------------------------------------------- launcher

template <int LOGN>
static void dbfv_batch_launch_big(bool encode, const u64* in, u64* out, long count, const BatchTab& tab, int form,
                                  int mode, const DbfvBatchArgs& a, hipStream_t s) {
    const dim3 grid((unsigned)count), block((1 << LOGN) / 16);
#define DD_(F_, M_) EXACTO_LAUNCH((dbfv_batch_decode_kernel<LOGN, F_, M_>), grid, block, 0, s, in, out, tab, a)
#define DB_(F_)                                                                                              \
    do {                                                                                                     \
        if (encode) EXACTO_LAUNCH((dbfv_batch_encode_kernel<LOGN, F_>), grid, block, 0, s, in, out, tab, a); \
        else if (mode == DB_U64) DD_(F_, DB_U64);                                                            \
        else if (mode == DB_I64) DD_(F_, DB_I64);                                                            \
        else DD_(F_, DB_I128);                                                                               \
    } while (0)
    if (form == F32_LAZY) DB_(F32_LAZY);
    else if (form == F32_WIDE) DB_(F32_WIDE);
    else DB_(BF_STRICT);
#undef DB_
#undef DD_
}

template <bool WIDE64>
static void dbfv_batch_launch_small(bool encode, const u64* in, u64* out, long count, int n, const BatchTab& tab,
                                    int mode, const DbfvBatchArgs& a, hipStream_t s) {
    const dim3 grid((unsigned)count), block((unsigned)n / 2);
    if (encode) EXACTO_LAUNCH((dbfv_batch_encode_small_kernel<WIDE64>), grid, block, 0, s, in, out, n, tab, a);
    else if (mode == DB_U64)
        EXACTO_LAUNCH((dbfv_batch_decode_small_kernel<WIDE64, DB_U64>), grid, block, 0, s, in, out, n, tab, a);
    else if (mode == DB_I64)
        EXACTO_LAUNCH((dbfv_batch_decode_small_kernel<WIDE64, DB_I64>), grid, block, 0, s, in, out, n, tab, a);
    else EXACTO_LAUNCH((dbfv_batch_decode_small_kernel<WIDE64, DB_I128>), grid, block, 0, s, in, out, n, tab, a);
}

void launch_dbfv_batch(bool encode, const u64* in, u64* out, long count, int d, u64 base, u64 p, int logn,
                       const BatchTab& tab, int form, hipStream_t s) {
    if (count <= 0 || d <= 0) return;
    DbfvBatchArgs a;
    a.d = d;
    a.shift = (base & (base - 1)) == 0 ? __builtin_ctzll(base) : -1;
    a.base = base;
    a.p = p;
    a.pmu = p ? ~0ull / p : 0;
    // the largest |sum of centred digit times b^k|, saturating
    const u128 lim = (u128)1 << 63;
    u128 bound = 0, power = 1;
    for (int k = 0; k < d && bound < lim; ++k) {
        bound += (u128)(tab.P.p / 2) * power;
        power = power > lim / base ? lim : power * base;
    }
    const int mode = p == 0 ? DB_U64 : bound < lim ? DB_I64 : DB_I128;
    if (logn < 10) {
        if (form == BF_STRICT) dbfv_batch_launch_small<true>(encode, in, out, count, 1 << logn, tab, mode, a, s);
        else dbfv_batch_launch_small<false>(encode, in, out, count, 1 << logn, tab, mode, a, s);
        return;
    }
    switch (logn) {
        case 10: dbfv_batch_launch_big<10>(encode, in, out, count, tab, form, mode, a, s); break;
        case 11: dbfv_batch_launch_big<11>(encode, in, out, count, tab, form, mode, a, s); break;
        case 12: dbfv_batch_launch_big<12>(encode, in, out, count, tab, form, mode, a, s); break;
        case 13: dbfv_batch_launch_big<13>(encode, in, out, count, tab, form, mode, a, s); break;
        case 14: dbfv_batch_launch_big<14>(encode, in, out, count, tab, form, mode, a, s); break;
        default: break;
    }
}

template <int LOGN>
static void batch_launch_big(bool encode, const u64* in, u64* out, long count, const BatchTab& tab, int form,
                             hipStream_t s) {
    const dim3 grid((unsigned)count), block((1 << LOGN) / 16);
#define BT_(F_)                                                                                          \
    do {                                                                                                 \
        if (encode) EXACTO_LAUNCH((batch_encode_kernel<LOGN, F_>), grid, block, 0, s, in, out, tab);    \
        else EXACTO_LAUNCH((batch_decode_kernel<LOGN, F_>), grid, block, 0, s, in, out, tab);           \
    } while (0)
    if (form == F32_LAZY) BT_(F32_LAZY);
    else if (form == F32_WIDE) BT_(F32_WIDE);
    else BT_(BF_STRICT);
#undef BT_
}

void launch_batch_transform(bool encode, const u64* in, u64* out, long count, int logn, const BatchTab& tab, int form,
                            hipStream_t s) {
    if (count <= 0) return;
    if (logn < 10) {
        const dim3 grid((unsigned)count), block((1u << logn) / 2);
        const int n = 1 << logn;
        const bool wide = form == BF_STRICT;
        if (encode) {
            if (wide) EXACTO_LAUNCH((batch_small_kernel<true, true>), grid, block, 0, s, in, out, n, tab);
            else EXACTO_LAUNCH((batch_small_kernel<true, false>), grid, block, 0, s, in, out, n, tab);
        } else {
            if (wide) EXACTO_LAUNCH((batch_small_kernel<false, true>), grid, block, 0, s, in, out, n, tab);
            else EXACTO_LAUNCH((batch_small_kernel<false, false>), grid, block, 0, s, in, out, n, tab);
        }
        return;
    }
    switch (logn) {
        case 10: batch_launch_big<10>(encode, in, out, count, tab, form, s); break;
        case 11: batch_launch_big<11>(encode, in, out, count, tab, form, s); break;
        case 12: batch_launch_big<12>(encode, in, out, count, tab, form, s); break;
        case 13: batch_launch_big<13>(encode, in, out, count, tab, form, s); break;
        case 14: batch_launch_big<14>(encode, in, out, count, tab, form, s); break;
        default: break;
    }
}

}  // namespace exacto
