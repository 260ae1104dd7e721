// Linear maps between dBFV digit vectors (dbfv/advanced.rs:36-160): dbfv_div_by_base and
// dbfv_change_base are both out_j = sum_i s_ji * in_i over the limbs of one ciphertext, which the
// reference composes from bfv_scalar_plain_mul (advanced.rs:162-171), bfv_add and bfv_sub, one
// ciphertext-sized pass per step.  Here the whole map is one streaming kernel over the non-zero
// entries of the matrix, listed row by row on the host: a thread owns two adjacent slots of one
// (item, component, limb) row, and for each output limb in turn sums that row's terms in registers
// and stores the limb once.  An input limb is fetched once per non-zero entry of its column: once
// per call for the maps this exists for (a base change between powers of one base and phi_b have one
// or two entries per column), and again from cache, by the same thread a few instructions later, for
// a denser column.  The next term's input is requested before the current one is used.
// Every term is reduced (Shoup, the scalar's companion precomputed on the host) and added modulo
// q_l, so the stored residues are the canonical ones the reference's sequence produces.  An entry 1
// costs no multiplication; a row of zeros is stored without reading anything.
#include "exacto_internal.hpp"

namespace exacto {

static constexpr int LM_TPB = 256;
static constexpr int LM_SLOTS = 2 * LM_TPB;  // slots per block: 16-byte accesses per lane

__device__ __forceinline__ ulonglong2 lm_load(const u64* p) { return *reinterpret_cast<const ulonglong2*>(p); }

// in [B][d_in][rpi][n], out [B][d_out][rpi][n] with rpi = polys * L rows per limb; terms [E][L]
// (LinTerm, exacto_internal.hpp), E >= 1, every output limb ending in a term with `last` set.
// WIDE (n a multiple of LM_SLOTS): a block stays inside one row, so the row, its prime and the terms
// are wave-uniform (scalar loads and branches); otherwise the rows are packed and each thread finds
// its own (the tail for n < 512, down to n = 16).
template <bool WIDE>
__global__ void __launch_bounds__(LM_TPB)
dbfv_linmap_kernel(const u64* __restrict__ in, u64* __restrict__ out, const LinTerm* __restrict__ terms, int E,
                   int d_in, int d_out, int rpi, int L, int n, long rows, const PrimeConst* __restrict__ primes) {
    long row;
    int j;
    if (WIDE) {
        const int bpr = n / LM_SLOTS;
        row = blockIdx.x / bpr;
        j = (int)(blockIdx.x - row * bpr) * LM_SLOTS + 2 * (int)threadIdx.x;
    } else {
        const long g = ((long)blockIdx.x * LM_TPB + threadIdx.x) * 2;
        row = g / n;
        j = (int)(g - row * n);
    }
    if (row >= rows) return;
    const long item = row / rpi;
    const int r = (int)(row - item * rpi);
    const int l = r % L;
    const u64 q = primes[l].q;
    const long limb_stride = (long)rpi * n;
    const u64* src = in + (item * d_in * rpi + r) * n + j;
    u64* dst = out + (item * d_out * rpi + r) * n + j;
    LinTerm t = terms[l];
    ulonglong2 x = make_ulonglong2(0, 0);
    if (t.s) x = lm_load(src + t.col * limb_stride);
    ulonglong2 acc = make_ulonglong2(0, 0);
    for (int e = 0; e < E; ++e) {
        LinTerm tn = t;
        ulonglong2 xn = x;
        if (e + 1 < E) {
            tn = terms[(long)(e + 1) * L + l];
            if (tn.s) xn = lm_load(src + tn.col * limb_stride);
        }
        if (t.s == 1) {
            acc.x = add_mod(acc.x, x.x, q);
            acc.y = add_mod(acc.y, x.y, q);
        } else if (t.s) {
            acc.x = add_mod(acc.x, shoup_mul_red(x.x, t.s, t.ss, q), q);
            acc.y = add_mod(acc.y, shoup_mul_red(x.y, t.s, t.ss, q), q);
        }
        if (t.last) {
            *reinterpret_cast<ulonglong2*>(dst) = acc;
            dst += limb_stride;
            acc = make_ulonglong2(0, 0);
        }
        t = tn;
        x = xn;
    }
}

// n even (ring degrees are powers of two >= 16), rows = items * polys * L, rows * n / 2 threads
void launch_dbfv_linmap(const u64* in, u64* out, const LinTerm* terms, int E, int d_in, int d_out, long items,
                        int polys, int n, int L, const PrimeConst* primes, hipStream_t s) {
    const int rpi = polys * L;
    const long rows = items * rpi;
    if (rows == 0 || E == 0) return;
    if (n % LM_SLOTS == 0) {
        const long blocks = rows * (n / LM_SLOTS);
        EXACTO_LAUNCH(dbfv_linmap_kernel<true>, dim3((unsigned)blocks), dim3(LM_TPB), 0, s, in, out, terms, E, d_in,
                      d_out, rpi, L, n, rows, primes);
    } else {
        const long blocks = (rows * n / 2 + LM_TPB - 1) / LM_TPB;
        EXACTO_LAUNCH(dbfv_linmap_kernel<false>, dim3((unsigned)blocks), dim3(LM_TPB), 0, s, in, out, terms, E, d_in,
                      d_out, rpi, L, n, rows, primes);
    }
}

}  // namespace exacto
