// Products of dBFV ciphertexts with public wide operands: out = reduce(sum_k pt_k * ct_k), the
// polynomial product of the two digit vectors, limb for limb what the reference would compose from
// bfv_plain_mul per digit pair (bfv/eval.rs:468-486), bfv_add by i + j and over k, and reduce
// (reduction.rs:15-93).  Every step of that composition is linear modulo q_l, so the stored canonical
// residues do not depend on the order of summation, and the whole of it is one streaming kernel shaped
// like dbfv_linmap_kernel: a thread owns two adjacent positions of one (item, component, prime) row,
// every access is 16 bytes, and per term it reads the d ciphertext values and the d lifted plaintext
// values of its positions once into registers, forms the surviving digit pairs and keeps the wide limbs
// as lazily accumulated 128-bit sums.  The next term's loads are issued before the current term's
// products (except where the second set of operand registers costs a wave, see PF), which are formed wide limb by wide limb, so that limb m waits for the first m + 1 digits of
// either operand only.  Each of the d output limbs is stored once; neither the 2d - 1 wide limbs nor
// the per-pair products ever exist in memory.  No LDS.
//
// The bound the lazy sums rely on.  Operands are canonical, so one product is at most (q - 1)^2 <
// 2^(2s) with s = bitlen(q) (PrimeConst::bar_s), and a partially reduced sum (pl_red: a residue below
// q) counts for less than one product.  A 128-bit accumulator therefore holds N = 2^(128 - 2s)
// products; the host (dbfv_plain_flush_products, context.hip) hands the kernels `flush` <= N - 2
// products of the largest prime between two reductions: the registers form reduces every accumulator
// in place after `flush / d` terms (an accumulator takes at most d products per term), the list form
// after `flush` products.  s <= 62 for every prime a context accepts, so N >= 16.
// barrett128 takes x < 2^(2s) only, so a sum is reduced as (hi mod q) (2^64 mod q) + (lo mod q): two
// reduce64 and one product of canonical residues.
// The fold of the high limbs (rep[m - d][i] wide[m], m >= d) uses the digits rep mod q_l from the
// host: the high sums are reduced to canonical residues first, the low sums too, and the at most d - 1
// products of the fold join one low residue in the accumulator (d <= N), reduced once more.
#include "dbfv_acc.hpp"

namespace exacto {

static constexpr int DP_TPB = 256;
static constexpr int DP_SLOTS = 2 * DP_TPB;  // positions per block: 16-byte accesses per lane

__device__ __forceinline__ ulonglong2 dp_load(const u64* p) { return *reinterpret_cast<const ulonglong2*>(p); }

struct DpAcc {   // the two positions' 128-bit sums
    u128 x, y;
};

__device__ __forceinline__ u128& dp_x(DpAcc& a) { return a.x; }
__device__ __forceinline__ u128& dp_y(DpAcc& a) { return a.y; }

struct DpRow {   // a thread's row and position
    long item;
    int r, l, j;
    bool ok;
};

template <bool WIDE>
__device__ __forceinline__ DpRow dp_row(int rpi, int L, int n, long rows) {
    DpRow w;
    long row;
    if (WIDE) {
        const int bpr = n / DP_SLOTS;
        row = blockIdx.x / bpr;
        w.j = (int)(blockIdx.x - row * bpr) * DP_SLOTS + 2 * (int)threadIdx.x;
    } else {
        const long g = ((long)blockIdx.x * DP_TPB + threadIdx.x) * 2;
        row = g / n;
        w.j = (int)(g - row * n);
    }
    w.ok = row < rows;
    w.item = row / rpi;
    w.r = (int)(row - w.item * rpi);
    w.l = w.r % L;
    return w;
}

// The registers form, d = D <= DP_MAX_D.  cts [items][K][D][rpi][n] (rpi = polys * L rows per limb; item
// and term strides in words), pl [pt items][K][D][L][n] lifted plaintexts (item stride 0: one plaintext
// for every item), out [items][D][rpi][n].  HI: some wide limb m >= D has a non-zero representative:
// bit m - D of `live` says which, fold [L][D - 1][D] holds rep[m - D][i] mod q_l.  accum: the sums join
// what out holds (a later term chunk).  flush_terms >= 1: terms between two in-place reductions.
template <bool WIDE, int D, bool HI>
__global__ void __launch_bounds__(DP_TPB)
dbfv_plain_mul_kernel(const u64* __restrict__ cts, long ct_item_stride, long ct_term_stride,
                      const u64* __restrict__ pl, long pl_item_stride, long pl_term_stride, u64* __restrict__ out,
                      int K, int flush_terms, int accum, unsigned live, const u64* __restrict__ fold, int rpi, int L,
                      int n, long rows, const PrimeConst* __restrict__ primes) {
    const DpRow w = dp_row<WIDE>(rpi, L, n, rows);
    if (!w.ok) return;
    const PrimeConst& P = primes[w.l];
    const u64 q = P.q;
    const u64 r64 = pl_r64(P);
    const long limb_stride = (long)rpi * n, Ln = (long)L * n;
    const u64* cp = cts + w.item * ct_item_stride + (long)w.r * n + w.j;
    const u64* pp = pl + w.item * pl_item_stride + (long)w.l * n + w.j;
    constexpr int W = HI ? 2 * D - 1 : D;
    // the next term's operands are requested before the current term's products, except with 15 wide limbs,
    // where the second set of operand registers would leave one wave per SIMD (measured: 1.5 x slower)
    constexpr bool PF = W < 15;
    DpAcc acc[W];
#pragma unroll
    for (int m = 0; m < W; ++m) acc[m].x = acc[m].y = 0;
    ulonglong2 c[D], p[D];
    if (PF) {
#pragma unroll
        for (int i = 0; i < D; ++i) {
            c[i] = dp_load(cp + i * limb_stride);
            p[i] = dp_load(pp + i * Ln);
        }
    }
    int since = 0;
    for (int k = 0; k < K; ++k) {
        ulonglong2 cn[D], pn[D];
        if (PF) {
#pragma unroll
            for (int i = 0; i < D; ++i) {
                cn[i] = c[i];
                pn[i] = p[i];
            }
            if (k + 1 < K) {
                cp += ct_term_stride;
                pp += pl_term_stride;
#pragma unroll
                for (int i = 0; i < D; ++i) {
                    cn[i] = dp_load(cp + i * limb_stride);
                    pn[i] = dp_load(pp + i * Ln);
                }
            }
        } else {
#pragma unroll
            for (int i = 0; i < D; ++i) {
                c[i] = dp_load(cp + i * limb_stride);
                p[i] = dp_load(pp + i * Ln);
            }
            cp += ct_term_stride;
            pp += pl_term_stride;
        }
        // by wide limb, so that limb m waits for the first m + 1 digits of either operand only
#pragma unroll
        for (int m = 0; m < W; ++m) {
            if (pl_live<D>(live, m)) {
#pragma unroll
                for (int i = 0; i < D; ++i) {
                    const int j = m - i;
                    if (j >= 0 && j < D) {
                        acc[m].x += (u128)p[i].x * c[j].x;
                        acc[m].y += (u128)p[i].y * c[j].y;
                    }
                }
            }
        }
        if (++since == flush_terms && k + 1 < K) {
            since = 0;
            pl_red_all<W>(acc, P, r64, dp_x);
            pl_red_all<W>(acc, P, r64, dp_y);
        }
        if (PF) {
#pragma unroll
            for (int i = 0; i < D; ++i) {
                c[i] = cn[i];
                p[i] = pn[i];
            }
        }
    }
    if constexpr (HI) {
        const u64* f = fold + (long)w.l * (D - 1) * D;
        pl_fold<D>(acc, live, f, P, r64, dp_x);
        pl_fold<D>(acc, live, f, P, r64, dp_y);
    }
    u64* dst = out + (w.item * D * rpi + w.r) * n + w.j;
#pragma unroll
    for (int i = 0; i < D; ++i) {
        ulonglong2 v = make_ulonglong2(pl_red(acc[i].x, P, r64), pl_red(acc[i].y, P, r64));
        if (accum) {
            const ulonglong2 o = dp_load(dst + i * limb_stride);
            v.x = add_mod(v.x, o.x, q);
            v.y = add_mod(v.y, o.y, q);
        }
        *reinterpret_cast<ulonglong2*>(dst + i * limb_stride) = v;
    }
}

// The list form, any d: output limb by output limb over the host's pair list (DpPair [E][L], rows in
// order, every output limb ending in a pair with `last` set; a limb without pairs is one pair with
// s = 0).  The operands of a pair are re-read through the cache instead of held in registers, and a
// folded pair (s != 1) costs a reduced product before its coefficient; flush: products between two
// in-place reductions.
template <bool WIDE>
__global__ void __launch_bounds__(DP_TPB)
dbfv_plain_mul_list_kernel(const u64* __restrict__ cts, long ct_item_stride, long ct_term_stride,
                           const u64* __restrict__ pl, long pl_item_stride, long pl_term_stride,
                           u64* __restrict__ out, int K, int flush, int accum, const DpPair* __restrict__ pairs, int E,
                           int d, int rpi, int L, int n, long rows, const PrimeConst* __restrict__ primes) {
    const DpRow w = dp_row<WIDE>(rpi, L, n, rows);
    if (!w.ok) return;
    const PrimeConst& P = primes[w.l];
    const u64 q = P.q;
    const u64 r64 = pl_r64(P);
    const long limb_stride = (long)rpi * n, Ln = (long)L * n;
    const u64* cp = cts + w.item * ct_item_stride + (long)w.r * n + w.j;
    const u64* pp = pl + w.item * pl_item_stride + (long)w.l * n + w.j;
    u64* dst = out + (w.item * d * rpi + w.r) * n + w.j;
    DpAcc acc;
    acc.x = acc.y = 0;
    int cnt = 0;
    for (int e = 0; e < E; ++e) {
        const DpPair t = pairs[(long)e * L + w.l];
        if (t.s) {
            const u64* ce = cp + t.ci * limb_stride;
            const u64* pe = pp + t.pi * Ln;
            ulonglong2 x = dp_load(ce), y = dp_load(pe);
            for (int k = 0; k < K; ++k) {
                ulonglong2 xn = x, yn = y;
                if (k + 1 < K) {
                    xn = dp_load(ce + (long)(k + 1) * ct_term_stride);
                    yn = dp_load(pe + (long)(k + 1) * pl_term_stride);
                }
                if (t.s == 1) {
                    acc.x += (u128)x.x * y.x;
                    acc.y += (u128)x.y * y.y;
                } else {
                    acc.x += (u128)mul_mod(x.x, y.x, P) * t.s;
                    acc.y += (u128)mul_mod(x.y, y.y, P) * t.s;
                }
                if (++cnt == flush) {
                    cnt = 0;
                    acc.x = pl_red(acc.x, P, r64);
                    acc.y = pl_red(acc.y, P, r64);
                }
                x = xn;
                y = yn;
            }
        }
        if (t.last) {
            ulonglong2 v = make_ulonglong2(pl_red(acc.x, P, r64), pl_red(acc.y, P, r64));
            if (accum) {
                const ulonglong2 o = dp_load(dst);
                v.x = add_mod(v.x, o.x, q);
                v.y = add_mod(v.y, o.y, q);
            }
            *reinterpret_cast<ulonglong2*>(dst) = v;
            dst += limb_stride;
            acc.x = acc.y = 0;
            cnt = 0;
        }
    }
}

template <bool WIDE, int D>
static void dp_launch(const DbfvPlainArgs& a, long blocks, hipStream_t s) {
    const int rpi = a.polys * a.L;
    const long rows = a.items * rpi;
    const int ft = a.flush / D;   // >= 1: flush >= 14 >= D
    if (a.live)
        EXACTO_LAUNCH((dbfv_plain_mul_kernel<WIDE, D, true>), dim3((unsigned)blocks), dim3(DP_TPB), 0, s, a.cts,
                      a.ct_item_stride, a.ct_term_stride, a.pl, a.pl_item_stride, a.pl_term_stride, a.out, a.K, ft,
                      a.accum, a.live, a.fold, rpi, a.L, a.n, rows, a.primes);
    else
        EXACTO_LAUNCH((dbfv_plain_mul_kernel<WIDE, D, false>), dim3((unsigned)blocks), dim3(DP_TPB), 0, s, a.cts,
                      a.ct_item_stride, a.ct_term_stride, a.pl, a.pl_item_stride, a.pl_term_stride, a.out, a.K, ft,
                      a.accum, a.live, a.fold, rpi, a.L, a.n, rows, a.primes);
}

template <bool WIDE>
static void dp_dispatch(const DbfvPlainArgs& a, long blocks, hipStream_t s) {
    const int rpi = a.polys * a.L;
    switch (a.d <= DP_MAX_D ? a.d : 0) {
    case 1: return dp_launch<WIDE, 1>(a, blocks, s);
    case 2: return dp_launch<WIDE, 2>(a, blocks, s);
    case 3: return dp_launch<WIDE, 3>(a, blocks, s);
    case 4: return dp_launch<WIDE, 4>(a, blocks, s);
    case 5: return dp_launch<WIDE, 5>(a, blocks, s);
    case 6: return dp_launch<WIDE, 6>(a, blocks, s);
    case 7: return dp_launch<WIDE, 7>(a, blocks, s);
    case 8: return dp_launch<WIDE, 8>(a, blocks, s);
    default:
        EXACTO_LAUNCH(dbfv_plain_mul_list_kernel<WIDE>, dim3((unsigned)blocks), dim3(DP_TPB), 0, s, a.cts,
                      a.ct_item_stride, a.ct_term_stride, a.pl, a.pl_item_stride, a.pl_term_stride, a.out, a.K,
                      a.flush, a.accum, a.pairs, a.E, a.d, rpi, a.L, a.n, a.items * rpi, a.primes);
    }
}

// n even (ring degrees are powers of two >= 16), rows = items * polys * L, rows * n / 2 threads
void launch_dbfv_plain_mul(const DbfvPlainArgs& a, hipStream_t s) {
    const long rows = a.items * a.polys * a.L;
    if (rows == 0 || a.K == 0) return;
    if (a.n % DP_SLOTS == 0) dp_dispatch<true>(a, rows * (a.n / DP_SLOTS), s);
    else dp_dispatch<false>(a, (rows * a.n / 2 + DP_TPB - 1) / DP_TPB, s);
}

}  // namespace exacto
