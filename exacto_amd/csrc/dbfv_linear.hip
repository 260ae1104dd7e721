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

// bfv_mul_sum's group sum: an output slot whose products exceed what one key switch lifts is computed
// as several groups (each one summed scale and one summed key switch); this adds a slot's groups
// modulo q_l before the slot's forward transform.  in [B][groups][rpi][n] with rpi = 2 L, out
// [B][nslots][rpi][n], slot s = groups [slot_start[s], slot_start[s + 1]) (at least one each).  Same
// shape as the linear map above: a thread owns two adjacent coefficients of one (item, slot,
// component, limb) row, 16-byte accesses, the next group's load issued before the current add; every
// input is read once and every output written once.
template <bool WIDE>
__global__ void __launch_bounds__(LM_TPB)
group_sum_kernel(const u64* __restrict__ in, u64* __restrict__ out, const int* __restrict__ slot_start, int groups,
                 int nslots, int rpi, int L, int n, long rows, const PrimeConst* __restrict__ primes) {
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
    // row = (item * nslots + slot) * rpi + r
    const long is = row / rpi;
    const int r = (int)(row - is * rpi);
    const long item = is / nslots;
    const int slot = (int)(is - item * nslots);
    const u64 q = primes[r % L].q;
    const int g0 = slot_start[slot], g1 = slot_start[slot + 1];
    const long group_stride = (long)rpi * n;
    const u64* src = in + ((item * groups + g0) * rpi + r) * n + j;
    ulonglong2 acc = lm_load(src);
    if (g0 + 1 < g1) {
        ulonglong2 x = lm_load(src + group_stride);
        for (int g = g0 + 1; g < g1; ++g) {
            ulonglong2 xn = x;
            if (g + 1 < g1) xn = lm_load(src + (long)(g + 1 - g0) * group_stride);
            acc.x = add_mod(acc.x, x.x, q);
            acc.y = add_mod(acc.y, x.y, q);
            x = xn;
        }
    }
    *reinterpret_cast<ulonglong2*>(out + row * n + j) = acc;
}

// n even, rows = items * nslots * 2 L, rows * n / 2 threads; in and out 16-byte aligned, disjoint
void launch_group_sum(const u64* in, u64* out, const int* slot_start, int groups, int nslots, long items, int n, int L,
                      const PrimeConst* primes, hipStream_t s) {
    const int rpi = 2 * L;
    const long rows = items * nslots * rpi;
    if (rows == 0) return;
    if (n % LM_SLOTS == 0) {
        const long blocks = rows * (n / LM_SLOTS);
        EXACTO_LAUNCH(group_sum_kernel<true>, dim3((unsigned)blocks), dim3(LM_TPB), 0, s, in, out, slot_start, groups,
                      nslots, rpi, L, n, rows, primes);
    } else {
        const long blocks = (rows * n / 2 + LM_TPB - 1) / LM_TPB;
        EXACTO_LAUNCH(group_sum_kernel<false>, dim3((unsigned)blocks), dim3(LM_TPB), 0, s, in, out, slot_start, groups,
                      nslots, rpi, L, n, rows, primes);
    }
}

}  // namespace exacto
