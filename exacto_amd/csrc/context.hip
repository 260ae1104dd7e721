// Host runtime and C ABI of libexacto_hip.so (see include/exacto_hip.h).
//
// Owns, per context: the prime set (ciphertext primes, then the auxiliary primes of
// the selected multiplication path), per-prime NTT twiddle tables and constants in
// HBM, the exact-CRT tables, the resident relinearisation key and a chunked
// workspace.  Every `_dev` entry point only enqueues kernels on the context stream.

#include "runtime.hpp"

using namespace exacto;

thread_local const void* exacto::g_last_kernel = nullptr;

// ============================================================== errors

static thread_local std::string g_last_error;

int exacto::fail(int code, const std::string& msg) {
    g_last_error = msg;
    return code;
}
int exacto::invalid_param(const std::string& s) { return fail(EXACTO_ERR_INVALID_PARAM, "invalid parameter: " + s); }

// ============================================================== host integer helpers

static u64 mulmod_h(u64 a, u64 b, u64 m) { return (u64)((u128)a * b % m); }

static u64 powmod_h(u64 b, u64 e, u64 m) {
    u64 r = 1 % m;
    b %= m;
    while (e) {
        if (e & 1) r = mulmod_h(r, b, m);
        b = mulmod_h(b, b, m);
        e >>= 1;
    }
    return r;
}

static bool is_prime_h(u64 n) {
    if (n < 2) return false;
    static const u64 small[] = {2, 3, 5, 7, 11, 13, 17, 19, 23, 29, 31, 37};
    for (u64 p : small)
        if (n % p == 0) return n == p;
    u64 d = n - 1;
    int s = 0;
    while ((d & 1) == 0) { d >>= 1; ++s; }
    for (u64 a : small) {
        u64 x = powmod_h(a, d, n);
        if (x == 1 || x == n - 1) continue;
        bool comp = true;
        for (int r = 1; r < s; ++r) {
            x = mulmod_h(x, x, n);
            if (x == n - 1) { comp = false; break; }
        }
        if (comp) return false;
    }
    return true;
}

// modular inverse via extended Euclid (returns 0 if not invertible)
u64 exacto::invmod_h(u64 a, u64 m) {
    i128 t = 0, nt = 1, r = m, nr = a % m;
    while (nr != 0) {
        i128 q = r / nr;
        i128 tmp = t - q * nt; t = nt; nt = tmp;
        tmp = r - q * nr; r = nr; nr = tmp;
    }
    if (r != 1) return 0;
    if (t < 0) t += m;
    return (u64)t;
}

u64 exacto::shoup_h(u64 w, u64 q) { return (u64)(((u128)w << 64) / q); }
static int bitlen(u64 x) { return x ? 64 - __builtin_clzll(x) : 0; }

static int bitrev(int x, int bits) {
    int r = 0;
    for (int i = 0; i < bits; ++i) { r = (r << 1) | (x & 1); x >>= 1; }
    return r;
}

// psi: smallest x >= 2 with (x^((q-1)/2n))^n == -1 (oracle/ring.py find_psi)
static u64 find_psi(u64 n, u64 q) {
    const u64 e = (q - 1) / (2 * n);
    for (u64 x = 2;; ++x) {
        const u64 psi = powmod_h(x, e, q);
        if (powmod_h(psi, n, q) == q - 1) return psi;
    }
}

// mixed-radix digits of X (given as residues mod primes[0..cnt)) — host Garner
static std::vector<u64> mixed_radix(const std::vector<u64>& res, const std::vector<u64>& pr) {
    std::vector<u64> v(pr.size());
    for (size_t i = 0; i < pr.size(); ++i) {
        u64 t = res[i];
        for (size_t k = 0; k < i; ++k) {
            const u64 vk = v[k] % pr[i];
            t = (t + pr[i] - vk) % pr[i];
            t = mulmod_h(t, invmod_h(pr[k] % pr[i], pr[i]), pr[i]);
        }
        v[i] = t;
    }
    return v;
}

// EXACTO_DEBUG_ALLOC=1: every device allocation and release of the library is logged
// to stderr with its pointer, size, pool and stream; =2 adds the allocation range the runtime reports
// for it (hipMemGetAddressRange), so that the failing bootstrap call's blocks can be checked for
// overlap with any other live block.  (Round 5: with the range lookups the failure no longer showed.)
static int dbg_alloc_on() {
    static const int on = [] { const char* e = getenv("EXACTO_DEBUG_ALLOC"); return e ? atoi(e) : 0; }();
    return on;
}
static void dbg_alloc_log(const char* what, const void* p, size_t bytes, const void* pool, const void* stream,
                          bool range) {
    if (!dbg_alloc_on()) return;
    hipDeviceptr_t base = nullptr;
    size_t sz = 0;
    if (range && p && dbg_alloc_on() > 1) {
        if (hipMemGetAddressRange(&base, &sz, (hipDeviceptr_t)p) != hipSuccess) base = nullptr;
        (void)hipGetLastError();   // a failed lookup must not reach the next CHECK_LAUNCH
    }
    std::fprintf(stderr, "alloc-dbg %s p=%p bytes=%zu pool=%p stream=%p range=%p+%zu\n", what, p, bytes, pool, stream,
                 (void*)base, sz);
}

void exacto::free_dev(void* p) {
    if (p) {
        dbg_alloc_log("hipFree", p, 0, nullptr, nullptr, false);
        (void)hipFree(p);
    }
}

// Per-call scratch from the context's own stream-ordered pool (hipMallocFromPoolAsync / hipFreeAsync
// on the stream that uses it; no device-wide synchronisation).  The pool belongs to the context
// (hipMemPoolCreate), so its release threshold -- freed blocks stay mapped for the next call -- does
// not change the device's default pool that other libraries in the process use.
// EXACTO_DEBUG_SCRATCH=1 (read when a context is created) fills every block with 0xFF when it is
// handed out, so a kernel that reads scratch it never wrote gives wrong results at once instead of
// whatever the previous owner of the block left there.
struct Scratch {
    void* p = nullptr;
    hipStream_t s = nullptr;
    Scratch() = default;
    Scratch(const Scratch&) = delete;
    Scratch& operator=(const Scratch&) = delete;
    hipMemPool_t from = nullptr;
    ~Scratch() {
        if (p) {
            dbg_alloc_log("hipFreeAsync", p, 0, from, s, false);
            (void)hipFreeAsync(p, s);
        }
    }
    hipError_t alloc(size_t bytes, hipStream_t st, hipMemPool_t pool, bool debug) {
        s = st;
        from = pool;
        hipError_t e = pool ? hipMallocFromPoolAsync(&p, std::max<size_t>(bytes, 8), pool, st)
                            : hipMallocAsync(&p, std::max<size_t>(bytes, 8), st);
        if (e == hipSuccess) dbg_alloc_log(pool ? "hipMallocFromPoolAsync" : "hipMallocAsync", p, bytes, pool, st, true);
        if (e == hipSuccess && debug) e = hipMemsetAsync(p, 0xFF, std::max<size_t>(bytes, 8), st);
        return e;
    }
    template <class T> T* as() const { return static_cast<T*>(p); }
};

// Every device allocation of the library.  EXACTO_DEBUG_FILL=1 (read once): new blocks are filled
// with 0xA5 bytes, so that a kernel reading memory nothing wrote sees garbage at once instead of the
// zeros of fresh pages (a read of that kind passed in a fresh process and failed after other work
// had freed and re-used the memory).
hipError_t exacto::dev_alloc(void** p, size_t bytes) {
    static const bool fill = [] { const char* e = getenv("EXACTO_DEBUG_FILL"); return e && e[0] == '1'; }();
    hipError_t e = hipMalloc(p, bytes);
    if (e == hipSuccess) dbg_alloc_log("hipMalloc", *p, bytes, nullptr, nullptr, true);
    if (e == hipSuccess && fill && bytes) {
        e = hipMemset(*p, 0xA5, bytes);
        if (e == hipSuccess) e = hipDeviceSynchronize();
    }
    return e;
}

// Device -> device copies of the library, as a kernel (every size here is whole u64 words); device
// fills likewise (launch_fill_u32).  Round 3 replaced hipMemcpyAsync / hipMemsetAsync with these
// while chasing an intermittent stale bootstrap result; round 4 measured that the runtime's own
// device-to-device copy is a blit kernel on the same queue (__amd_rocclr_copyBuffer) and never read
// stale in 180k replays of the bootstrap's sequence (tools/d2d_repro.cpp), so the change is not a
// fix of a runtime fault.  It stays: every device-side operation of the library is a
// kernel of its own, one code path, visible by name in kernel traces.
static hipError_t dev_copy(void* dst, const void* src, size_t bytes, hipStream_t s) {
    launch_copy_u64(static_cast<u64*>(dst), static_cast<const u64*>(src), (long)(bytes / 8), s);
    return hipGetLastError();
}

// Host -> device copy ordered on the context stream.  The stream is non-blocking, so it does not
// wait for the legacy null stream that a plain hipMemcpy runs on: a kernel enqueued on it right
// after such a copy may read the destination before the copy has landed.  Returns once the copy
// is complete, so `src` may be reused at once.
static int upload(exacto_ctx* c, void* dst, const void* src, size_t bytes) {
    if (!bytes) return 0;
    HIP_TRY(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return 0;
}

static int plan_check(size_t n, u64 q) {
    // make_plan (ntt.rs:19-29) via concrete-ntt Plan::try_new: prime q == 1 mod 2n, n >= 16.
    // This library additionally needs q < 2^62 (lazy butterflies keep 4q < 2^64).
    if (n < 16 || q < 2 || q >= (1ull << 62) || (q - 1) % (2 * n) != 0 || !is_prime_h(q))
        return invalid_param("cannot create NTT plan for n=" + std::to_string(n) + ", q=" + std::to_string(q) +
                             " (need prime q ≡ 1 mod " + std::to_string(2 * n));
    return 0;
}

static PrimeConst make_prime_const(u64 q, int n, int logn, TwPair* h_fwd, TwPair* h_inv) {
    PrimeConst P{};
    P.q = q;
    P.two_q = 2 * q;
    P.mu64 = (u64)((((u128)1) << 64) / q);
    P.bar_s = bitlen(q);
    P.bar_mu = (u64)((((u128)1) << (2 * P.bar_s)) / q);
    const u64 psi = find_psi(n, q);
    const u64 psi_inv = invmod_h(psi, q);
    for (int i = 0; i < n; ++i) {
        const int e = bitrev(i, logn);
        const u64 w = powmod_h(psi, e, q), wi = powmod_h(psi_inv, e, q);
        h_fwd[i] = {w, shoup_h(w, q)};
        h_inv[i] = {wi, shoup_h(wi, q)};
    }
    P.n_inv = invmod_h((u64)n % q, q);
    P.n_inv_s = shoup_h(P.n_inv, q);
    P.last_w = mulmod_h(h_inv[1].w, P.n_inv, q);
    P.last_ws = shoup_h(P.last_w, q);
    u64 qi = q;                                   // q^-1 mod 2^64 by Newton (q odd): 6 doublings
    for (int it = 0; it < 6; ++it) qi *= 2 - q * qi;
    P.qinv_neg = (u64)0 - qi;
    const u64 r = (u64)((((u128)1) << 64) % q);   // R = 2^64 mod q
    P.n_inv_r = mulmod_h(P.n_inv, r, q);
    P.n_inv_rs = shoup_h(P.n_inv_r, q);
    P.last_wr = mulmod_h(P.last_w, r, q);
    P.last_wrs = shoup_h(P.last_wr, q);
    return P;
}

static void set_shoup(u64& w, u64& ws, u64 v, u64 q) {
    w = v;
    ws = shoup_h(v, q);
}

// The largest magnitude of a balanced gadget digit (keyswitch.rs:24-44: a remainder >= floor(B/2)
// becomes rem - B): ceil(B/2).  An odd base reaches -(B+1)/2, from a positive remainder equal to
// floor(B/2); for an even base this is B/2.  (Written so that B = 2^64 - 1 does not wrap.)
static inline u64 digit_max(u64 gbase) { return gbase / 2 + (gbase & 1); }

// The largest m <= 64 with prod p > 2 m `one` + 1: the centred lift of a sum of m terms, each at most
// `one` in magnitude, is exact.  fpc: with the float-CRT lift's margin, prod p 2^20 > (2 m one + 1)
// (2^20 + 1), so |u| / P < 1/2 - 2^-21 against the float sum's error below 2^-48 (ks32_fpc_one).
static int sums_lifted(const Big& P, const Big& one, bool fpc) {
    Big pf = P;
    if (fpc) pf.mul(1ull << 20);
    int r = 0;
    for (u64 m = 1; m <= 64; ++m) {
        Big bm = one;
        bm.mul(2 * m);
        bm.add(1);
        if (fpc) bm.mul((1ull << 20) + 1);
        if (pf.cmp(bm) <= 0) break;
        r = (int)m;
    }
    return r;
}

// ks32.hip's auxiliary basis: the fewest primes p == 1 mod 2n in (2^30, 2^31), largest first, with
// prod p > 2 G n ceil(B/2) floor(q_max/2) (the magnitude bound of sum_g d_g * r_g, digits balanced
// in [-ceil(B/2), B/2), key coefficients balanced).  Eligible: exact path, gadget base <= 2^16 (int16
// digits), every ciphertext prime 2^60 - d with d < 2^24 (ks32_crt reduces with reduce_near60),
// 1024 <= n <= 16384; S <= 4.
// One 31-bit basis for ks32: the fewest primes p == 1 mod 2n below pmax (largest first, all above
// 2^30) with prod p > `bound`, its twiddles, constants and Garner tables on the device.  sum_max:
// how many key-switch sums (dBFV products of one output limb) the basis lifts exactly when they
// are added first.  S = 0 when no basis of at most EXACTO_KS32_MAXS primes exists.
// fixedS > 0 (the lazy basis): exactly fixedS primes in (7 pmax / 8, pmax), no bound check here (the
// bound is the resident key's, checked when the key is converted: ensure_rs; ks32.hip's red_s64_lz
// needs p > 0.8 * 2^30).
static int build_ks32_basis_impl(exacto_ctx* c, u64 pmax, u64 qmax, const Big& bound, Ks32Basis* b,
                                 int fixedS = 0) {
    b->S = 0;
    std::vector<u64> ps;
    Big P(1);
    const u64 step = 2 * (u64)c->n;
    const u64 pmin = fixedS ? pmax - pmax / 8 : (1ull << 30);
    for (u64 p = (pmax - 1) / step * step + 1; p > pmin && ps.size() < EXACTO_KS32_MAXS; p -= step) {
        if (!is_prime_h(p)) continue;
        ps.push_back(p);
        P.mul(p);
        if (fixedS ? (int)ps.size() == fixedS : P.cmp(bound) > 0) break;
    }
    if (fixedS ? (int)ps.size() != fixedS : (P.cmp(bound) <= 0 || ps.size() < 2)) return 0;
    bool lazy = true, narrow = true;
    for (u64 p : ps) {
        lazy &= p < (1ull << 30);
        narrow &= p < (1ull << 32) / 3;
    }
    b->mac_form = lazy ? 2 : narrow ? 1 : 0;
    b->P = P;
    b->sum_max = b->fpc_max = 0;
    if (!fixedS) {   // the lazy basis' limits come from the resident key (ks32_select_basis)
        Big one((u64)c->G);
        one.mul((u64)c->n);
        one.mul(digit_max(c->gbase));
        one.mul(qmax / 2);
        b->sum_max = std::max(1, sums_lifted(P, one, false));   // P > bound was checked above
        b->fpc_max = ps.size() <= 3 || narrow ? sums_lifted(P, one, true) : 0;   // ks32_crt's condition
    }
    const int S = (int)ps.size(), n = c->n;
    std::vector<uint2> tw((size_t)S * 2 * n);
    std::vector<Prime32> pc(S);
    auto sh32 = [](u64 w, u64 p) { return (uint32_t)((w << 32) / p); };
    for (int s = 0; s < S; ++s) {
        const u64 p = ps[s];
        const u64 psi = find_psi(n, p), psi_inv = invmod_h(psi, p);
        for (int i = 0; i < n; ++i) {
            const int e = bitrev(i, c->logn);
            const u64 w = powmod_h(psi, e, p), wi = powmod_h(psi_inv, e, p);
            tw[(size_t)s * 2 * n + i] = make_uint2((uint32_t)w, sh32(w, p));
            tw[(size_t)s * 2 * n + n + i] = make_uint2((uint32_t)wi, sh32(wi, p));
        }
        Prime32& Q = pc[s];
        Q.p = (uint32_t)p;
        const u64 ninv = invmod_h((u64)n % p, p);
        Q.n_inv = (uint32_t)ninv;
        Q.n_inv_s = sh32(ninv, p);
        const u64 lw = mulmod_h(tw[(size_t)s * 2 * n + n + 1].x, ninv, p);
        Q.last_w = (uint32_t)lw;
        Q.last_ws = sh32(lw, p);
        const u64 c32 = (1ull << 32) % p;
        Q.c32 = (uint32_t)c32;
        Q.c32s = sh32(c32, p);
        const u64 m63 = (1ull << 63) % p;
        Q.k63 = (uint32_t)(m63 == 0 ? 0 : p - m63);
        // the float-CRT lift's factor pi = (P / p)^-1 mod p folded into the last inverse stage
        u64 pi = 1;
        for (int k = 0; k < (int)ps.size(); ++k)
            if (k != s) pi = mulmod_h(pi, ps[k] % p, p);
        pi = invmod_h(pi, p);
        const u64 fni = mulmod_h(ninv, pi, p), flw = mulmod_h(lw, pi, p);
        Q.fn_inv = (uint32_t)fni;
        Q.fn_inv_s = sh32(fni, p);
        Q.flast_w = (uint32_t)flw;
        Q.flast_ws = sh32(flw, p);
        Q.inv_p = 1.0 / (double)p;
    }
    if (int e_ = b->d_tw32.alloc(tw.size() * sizeof(uint2))) return e_;
    if (int e_ = upload(c, b->d_tw32, tw.data(), tw.size() * sizeof(uint2))) return e_;
    for (int s = 0; s < S; ++s) {
        pc[s].tw_fwd = b->d_tw32 + (size_t)s * 2 * n;
        pc[s].tw_inv = b->d_tw32 + (size_t)s * 2 * n + n;
    }
    if (int e_ = b->d_p32.alloc(S * sizeof(Prime32))) return e_;
    if (int e_ = upload(c, b->d_p32, pc.data(), S * sizeof(Prime32))) return e_;
    Ks32Tables T;
    std::memset(&T, 0, sizeof(T));
    for (int s = 0; s < S; ++s)
        for (int k = 0; k < s; ++k) {
            const u64 v = invmod_h(ps[k] % ps[s], ps[s]);
            T.ginv[s][k] = (uint32_t)v;
            T.ginv_s[s][k] = sh32(v, ps[s]);
        }
    Big H = P;
    H.shr1();
    {
        std::vector<u64> hr(S);
        for (int s = 0; s < S; ++s) hr[s] = H.mod(ps[s]);
        auto mr = mixed_radix(hr, ps);
        for (int s = 0; s < S; ++s) T.halfP[s] = (uint32_t)mr[s];
    }
    for (int l = 0; l < c->L; ++l) {
        const u64 q = c->ctq[l];
        u64 pref = 1;
        for (int s = 0; s < S; ++s) {
            T.pref_w[l][s] = pref;
            T.pref_ws[l][s] = shoup_h(pref, q);
            pref = mulmod_h(pref, ps[s] % q, q);
        }
        const u64 pm = P.mod(q);
        T.negP[l] = pm == 0 ? 0 : q - pm;
        constexpr u64 M30 = (1ull << 30) - 1;
        for (int s = 0; s < S; ++s) {
            u64 cs = 1;   // (P / p_s) mod q
            for (int k = 0; k < S; ++k)
                if (k != s) cs = mulmod_h(cs, ps[k] % q, q);
            T.fpc_c[l][s][0] = (uint32_t)(cs & M30);
            T.fpc_c[l][s][1] = (uint32_t)(cs >> 30);
        }
        T.fpc_n[l][0] = (uint32_t)(T.negP[l] & M30);
        T.fpc_n[l][1] = (uint32_t)(T.negP[l] >> 30);
    }
    if (int e_ = b->d_kst.alloc(sizeof(Ks32Tables))) return e_;
    if (int e_ = upload(c, b->d_kst, &T, sizeof(Ks32Tables))) return e_;
    b->S = S;
    return 0;
}

// the active primary basis (run_mul, dbfv_mul_group, bfv_apply_automorphism read these fields)
static void use_ks32_basis(exacto_ctx* c, const Ks32Basis& b) {
    c->S32 = b.S;
    c->d_p32 = b.d_p32;
    c->d_tw32 = b.d_tw32;
    c->d_kst = b.d_kst;
    c->ks32_sum_max = b.sum_max;
    c->ks32_fpc_max = b.fpc_max;
    c->ks32_mac_form = b.mac_form;
    c->ks32_lazy_active = &b == &c->kz;
}

// build_ks32_basis_impl, releasing whatever it allocated when a later step fails (no half-built basis)
static int build_ks32_basis(exacto_ctx* c, u64 pmax, u64 qmax, const Big& bound, Ks32Basis* b, int fixedS = 0) {
    const int e = build_ks32_basis_impl(c, pmax, qmax, bound, b, fixedS);
    if (e) *b = Ks32Basis{};
    return e;
}

// ks32.hip's auxiliary bases, bounding |sum_g d_g * r_g| <= G n ceil(B/2) floor(q_max/2) (digits
// balanced in [-ceil(B/2), B/2), key coefficients balanced).  Eligible: exact path, gadget base <= 2^16
// (int16 digits), every ciphertext prime 2^60 - d with d < 2^24 (ks32_crt reduces with
// reduce_near60), 1024 <= n <= 16384; S <= 4.
//   primary: primes below 2^32 / 3, so that sums of three residues fit 32 bits and the MAC adds
//            twelve balanced products (< 2^58.9) per reduction;
//   wide:    primes up to 2^31 (seven products per reduction), kept only when it holds more
//            dBFV digit sums than the primary (cfg4: two products per limb).
// EXACTO_KS32_WIDE=0: no wide basis; =2: the wide basis as the primary too (A/B switch).
static int setup_ks32(exacto_ctx* c) {
    c->S32 = 0;
    if (c->path != EXACTO_PATH_EXACT_RNS || c->gbase > 65536 || c->logn < 10 || c->logn > 14 || c->L > 4)
        return 0;
    u64 qmax = 0;
    for (u64 q : c->ctq) {
        if (q >= (1ull << 60) || q <= (1ull << 60) - (1ull << 24)) return 0;
        qmax = std::max(qmax, q);
    }
    Big bound((u64)c->G);
    bound.mul((u64)c->n);
    bound.mul(digit_max(c->gbase));
    bound.mul(qmax / 2);
    bound.mul(2);
    bound.add(1);
    const char* wide_env = getenv("EXACTO_KS32_WIDE");
    const int wide_mode = wide_env ? atoi(wide_env) : 1;
    Ks32Basis prim;
    if (int e = build_ks32_basis(c, wide_mode == 2 ? (1ull << 31) : (1ull << 32) / 3, qmax, bound, &prim)) return e;
    if (wide_mode == 1) {
        if (int e = build_ks32_basis(c, 1ull << 31, qmax, bound, &c->kw)) return e;
        if (prim.S == 0 && c->kw.S > 0) {   // only the wide range holds the bound: it is the primary
            prim = std::move(c->kw);
            c->kw = Ks32Basis{};
        } else if (c->kw.S > 0 && c->kw.sum_max <= prim.sum_max) {
            c->kw = Ks32Basis{};
        }
    }
    if (prim.S == 0) return 0;
    c->kn = std::move(prim);
    // the lazy basis: as many primes below 2^30 as the primary has (the workspaces are sized by S)
    const char* lz = getenv("EXACTO_KS32_LAZY");
    if (!(lz && lz[0] == '0') && wide_mode != 2)
        if (int e = build_ks32_basis(c, 1ull << 30, qmax, bound, &c->kz, c->kn.S)) return e;
    use_ks32_basis(c, c->kn);
    return 0;
}

static int build_tables(exacto_ctx* c) {
    const int NP = (int)c->primes.size();
    std::vector<TwPair> tw((size_t)NP * 2 * c->n);
    std::vector<PrimeConst> pc(NP);
    for (int t = 0; t < NP; ++t)
        pc[t] = make_prime_const(c->primes[t], c->n, c->logn, &tw[(size_t)t * 2 * c->n],
                                 &tw[(size_t)t * 2 * c->n + c->n]);
    if (int e_ = c->d_tw.alloc(tw.size() * sizeof(TwPair))) return e_;
    if (int e_ = upload(c, c->d_tw, tw.data(), tw.size() * sizeof(TwPair))) return e_;
    for (int t = 0; t < NP; ++t) {
        pc[t].tw_fwd = c->d_tw + (size_t)t * 2 * c->n;
        pc[t].tw_inv = c->d_tw + (size_t)t * 2 * c->n + c->n;
    }
    if (int e_ = c->d_primes.alloc(NP * sizeof(PrimeConst))) return e_;   // (uploaded below, with the CRT folds)

    // ---- CRT tables
    CrtTables& C = c->h_crt;
    std::memset(&C, 0, sizeof(C));
    const int L = c->L, K = c->K;
    C.L = L;
    C.K = K;
    C.G = c->G;
    C.gbase = c->gbase;
    C.gshift = (c->gbase & (c->gbase - 1)) == 0 ? bitlen(c->gbase) - 1 : -1;
    C.plain = c->plain;
    const std::vector<u64> qv(c->primes.begin(), c->primes.begin() + L);
    const std::vector<u64> pv(c->primes.begin() + L, c->primes.end());
    for (int i = 0; i < L; ++i)
        for (int k = 0; k < i; ++k) set_shoup(C.gq_w[i][k], C.gq_ws[i][k], invmod_h(qv[k] % qv[i], qv[i]), qv[i]);
    Big Q(1);
    for (u64 q : qv) Q.mul(q);
    Big H = Q;
    H.shr1();
    {
        std::vector<u64> hr(L);
        for (int i = 0; i < L; ++i) hr[i] = H.mod(qv[i]);
        auto mr = mixed_radix(hr, qv);
        for (int i = 0; i < L; ++i) C.halfQ_mr[i] = mr[i];
    }
    for (int t = 0; t < NP; ++t) {
        const u64 pt = c->primes[t];
        u64 pref = 1 % pt;
        for (int k = 0; k <= L; ++k) {
            set_shoup(C.qpref_w[k][t], C.qpref_ws[k][t], pref, pt);
            if (k < L) pref = mulmod_h(pref, qv[k] % pt, pt);
        }
        set_shoup(C.pmod_w[t], C.pmod_ws[t], c->plain % pt, pt);
    }
    for (int i = 0; i < L && i < (int)Q.w.size(); ++i) C.Qwords[i] = Q.w[i];
    for (int t = 0; t < NP; ++t) C.hq[t] = H.mod(c->primes[t]);
    if (c->path == EXACTO_PATH_HPS) {
        const u64 q = qv[0];
        for (int a = 0; a < K && a < 2; ++a) {
            C.hps_qinv[a] = invmod_h(q % pv[a], pv[a]);
            C.hps_qinv_s[a] = shoup_h(C.hps_qinv[a], pv[a]);
        }
        if (c->plain < q) C.hps_pc = (u64)(((u128)c->plain << 64) / q);
        if (K == 2) {
            C.hps_p1_inv_p0 = invmod_h(pv[1] % pv[0], pv[0]);
            C.hps_p0_inv_p1 = invmod_h(pv[0] % pv[1], pv[1]);
            set_shoup(C.hps_t_w[0], C.hps_t_ws[0], mulmod_h(C.hps_qinv[0], C.hps_p1_inv_p0, pv[0]), pv[0]);
            set_shoup(C.hps_t_w[1], C.hps_t_ws[1], mulmod_h(C.hps_qinv[1], C.hps_p0_inv_p1, pv[1]), pv[1]);
            set_shoup(C.hps_pq_w[0], C.hps_pq_ws[0], pv[1] % q, q);
            set_shoup(C.hps_pq_w[1], C.hps_pq_ws[1], pv[0] % q, q);
            const u128 P = (u128)pv[0] * pv[1];
            const u64 Pq = (u64)(P % q);
            C.hps_kPq[0] = 0;
            C.hps_kPq[1] = Pq;
            C.hps_kPq[2] = (u64)(((u128)Pq * 2) % q);
            C.hps_P[0] = (u64)P; C.hps_P[1] = (u64)(P >> 64);
            C.hps_halfP[0] = (u64)(P >> 1); C.hps_halfP[1] = (u64)(P >> 65);
        }
    } else {
        for (int a = 0; a < K; ++a)
            for (int k = 0; k < a; ++k) set_shoup(C.gp_w[a][k], C.gp_ws[a][k], invmod_h(pv[k] % pv[a], pv[a]), pv[a]);
        Big P(1);
        for (u64 p : pv) P.mul(p);
        Big HP = P;
        HP.shr1();
        std::vector<u64> hr(K);
        for (int a = 0; a < K; ++a) hr[a] = HP.mod(pv[a]);
        auto mr = mixed_radix(hr, pv);
        for (int a = 0; a < K; ++a) C.halfP_mr[a] = mr[a];
        for (int i = 0; i < L; ++i) {
            u64 pref = 1 % qv[i];
            for (int k = 0; k <= K; ++k) {
                set_shoup(C.ppref_w[k][i], C.ppref_ws[k][i], pref, qv[i]);
                if (k < K) pref = mulmod_h(pref, pv[k] % qv[i], qv[i]);
            }
        }
        for (int a = 0; a < K; ++a) {
            const u64 pa = pv[a];
            const u64 qinv = invmod_h(Q.mod(pa), pa);
            set_shoup(C.qinvp_w[a], C.qinvp_ws[a], qinv, pa);
            set_shoup(C.pq_w[a], C.pq_ws[a], mulmod_h(c->plain % pa, qinv, pa), pa);
            for (int k = 0; k <= L; ++k)
                set_shoup(C.qpq_w[k][a], C.qpq_ws[k][a], mulmod_h(C.qpref_w[k][L + a], qinv, pa), pa);
        }
        for (int a = 0; a < K; ++a) {   // the FPC constants (see CrtTables)
            const u64 pa = pv[a];
            u64 others = 1;   // (P / p_a) mod p_a
            for (int b = 0; b < K; ++b)
                if (b != a) others = mulmod_h(others, pv[b] % pa, pa);
            const u64 pi = invmod_h(others, pa);
            C.fpc_pq[a] = mulmod_h(C.pq_w[a], pi, pa);
            for (int k = 0; k < L; ++k) C.fpc_qpq[k][a] = mulmod_h((pa - C.qpq_w[k][a]) % pa, pi, pa);
            C.fpc_neg[a] = pi;
            C.fpc_inv[a] = 1.0 / (double)pa;
            for (int i = 0; i < L; ++i) {
                u64 pm = 1 % qv[i];
                for (int b = 0; b < K; ++b)
                    if (b != a) pm = mulmod_h(pm, pv[b] % qv[i], qv[i]);
                C.fpc_pm[a][i] = pm;
            }
        }
        for (int i = 0; i < L; ++i) {
            const u64 pm = P.mod(qv[i]);
            C.fpc_negP[i] = pm == 0 ? 0 : qv[i] - pm;
        }
        for (int i = 0; i < L; ++i) {   // the FPQ constants (see CrtTables)
            const u64 q = qv[i];
            u64 qo = 1 % q;   // (Q / q_i) mod q_i
            for (int k = 0; k < L; ++k)
                if (k != i) qo = mulmod_h(qo, qv[k] % q, q);
            set_shoup(C.fpq_pz_w[i], C.fpq_pz_ws[i], mulmod_h(c->plain % q, invmod_h(qo, q), q), q);
            set_shoup(C.fpq_qo_w[i], C.fpq_qo_ws[i], qo, q);
            C.fpq_inv0[i] = 1.0 / (double)q;
            C.fpq_inv1[i] = (double)(1ull << 30) / (double)q;
            for (int a = 0; a < K; ++a) {
                const u64 pa = pv[a], qi = invmod_h(q % pa, pa);
                C.fpq_c[i][a] = mulmod_h((pa - qi) % pa, C.fpc_neg[a], pa);
            }
        }
        // the last inverse stage's constants times the prime's CRT factor (PrimeConst::fold_*)
        auto fold = [&](PrimeConst& P, u64 f) {
            set_shoup(P.fold_n, P.fold_ns, mulmod_h(P.n_inv, f, P.q), P.q);
            set_shoup(P.fold_w, P.fold_ws, mulmod_h(P.last_w, f, P.q), P.q);
        };
        for (int i = 0; i < L; ++i) fold(pc[i], C.fpq_pz_w[i]);
        for (int a = 0; a < K; ++a) fold(pc[L + a], C.fpc_pq[a]);
    }
    if (int e_ = upload(c, c->d_primes, pc.data(), NP * sizeof(PrimeConst))) return e_;
    {
        const u64 mx = *std::max_element(c->primes.begin(), c->primes.end());
        const u64 mn = *std::min_element(c->primes.begin(), c->primes.end());
        C.near = (u128)mx < 2 * (u128)mn;
        C.fast = C.near && mx < (1ull << 60);
        C.special = C.fast && mn > (1ull << 60) - (1ull << 24);
        C.digit_small = c->gbase <= *std::min_element(qv.begin(), qv.end());
    }
    if (int e_ = c->d_scal.alloc(EXACTO_MAX_L * sizeof(u64))) return e_;
    if (int e_ = c->d_crt.alloc(sizeof(CrtTables))) return e_;
    if (int e_ = upload(c, c->d_crt, &C, sizeof(CrtTables))) return e_;
    return 0;
}

extern "C" int exacto_ctx_create(exacto_ctx** out, size_t n, const uint64_t* ct_moduli, size_t L,
                                 const uint64_t* aux_moduli, size_t num_aux, uint64_t plain,
                                 uint64_t gadget_base, int device) {
    if (!out) return invalid_param("null context pointer");
    *out = nullptr;
    // BfvParamsBuilder::build order (params/mod.rs:81-98)
    if (n < 2 || (n & (n - 1)) != 0)
        return fail(EXACTO_ERR_INVALID_RING_DEGREE, "ring degree must be a power of 2, got " + std::to_string(n));
    if (L == 0 || !ct_moduli) return invalid_param("must specify at least one ciphertext modulus");
    if (plain < 2) return invalid_param("plaintext modulus must be >= 2");
    if (n > 16384) return invalid_param("ring degree " + std::to_string(n) + " exceeds the HIP NTT limit of 16384");
    if (L > EXACTO_MAX_L) return invalid_param("at most " + std::to_string(EXACTO_MAX_L) + " ciphertext moduli are supported");
    for (size_t i = 0; i < L; ++i)
        if (int e = plan_check(n, ct_moduli[i])) return e;
    for (size_t i = 0; i < L; ++i)
        for (size_t k = 0; k < i; ++k)
            if (ct_moduli[i] == ct_moduli[k]) return invalid_param("RNS moduli must be coprime");
    for (size_t i = 0; i < num_aux; ++i)
        if (int e = plan_check(n, aux_moduli[i])) return e;

    exacto_ctx* c = new exacto_ctx();
    c->device = device;
    c->n = (int)n;
    c->logn = bitlen(n) - 1;
    c->L = (int)L;
    c->ctq.assign(ct_moduli, ct_moduli + L);
    if (num_aux) c->user_aux.assign(aux_moduli, aux_moduli + num_aux);
    c->plain = plain;
    c->gbase = gadget_base == 0 ? (1ull << 16) : gadget_base;
    if (c->gbase < 2) { delete c; return invalid_param("gadget base must be >= 2"); }
    // compute_gadget_digits (params/mod.rs:126-140)
    {
        Big Q(1);
        for (u64 q : c->ctq) Q.mul(q);
        Big pw(1);
        int g = 0;
        while (pw.cmp(Q) < 0) { pw.mul(c->gbase); ++g; }
        c->G = std::max(g, 1);
    }
    if (c->G > EXACTO_MAX_G) { delete c; return invalid_param("gadget digit count exceeds " + std::to_string(EXACTO_MAX_G)); }
    // dispatcher (eval.rs:99-107)
    if (L > 1) {
        c->path = EXACTO_PATH_EXACT_RNS;
    } else if (num_aux > 0) {
        c->path = EXACTO_PATH_HPS;
        const u64 q = c->ctq[0];
        if (num_aux == 1) {
            const u128 min_required = ((u128)n * q) / 2;
            if ((u128)c->user_aux[0] <= min_required) {
                c->deferred_code = EXACTO_ERR_INVALID_PARAM;
                c->deferred_msg = "invalid parameter: single aux prime too small for HPS centering: P=" +
                                  std::to_string(c->user_aux[0]) + " <= n*Q/2=" + std::to_string((u64)min_required);
            }
        } else if (num_aux > 2) {
            c->deferred_code = EXACTO_ERR_INVALID_PARAM;
            c->deferred_msg = "invalid parameter: HPS scaling supports 1 or 2 aux primes, got " + std::to_string(num_aux);
        }
    } else {
        c->path = EXACTO_PATH_SCHOOLBOOK;
        // schoolbook_overflow_risk (eval.rs:457-464), u128 saturating
        const u128 maxc = c->ctq[0] / 2;
        const u128 sat = ~(u128)0;
        const u128 i128max = sat >> 1;
        auto smul = [&](u128 a, u128 b) -> u128 { return (b != 0 && a > sat / b) ? sat : a * b; };
        const u128 max_tensor = smul(smul((u128)n, maxc), maxc);
        const u128 max_scaled = smul(max_tensor, (u128)plain);
        if (max_tensor > i128max || max_scaled > i128max) {
            c->deferred_code = EXACTO_ERR_NOT_IMPLEMENTED;
            c->deferred_msg = "not yet implemented: schoolbook BFV multiplication can overflow i128 for these "
                              "parameters; use HPS auxiliary basis";
        }
    }
    c->primes = c->ctq;
    if (c->path == EXACTO_PATH_HPS) {
        if (num_aux <= 2) {
            c->K = (int)num_aux;
            for (u64 p : c->user_aux) c->primes.push_back(p);
        }
    } else {
        // internal auxiliary basis P > 4 * p * n * Q (exact tensor and exact rounding fit)
        Big need(4);
        need.mul(plain);
        need.mul(n);
        for (u64 q : c->ctq) need.mul(q);
        Big P(1);
        const u64 step = 2 * n;
        // below 2^60 so every prime of the exact path takes the lazy forward NTT (16q <= 2^64)
        u64 cand = ((1ull << 60) - 1) / step * step + 1;
        while (P.cmp(need) <= 0) {
            while (cand > step) {
                cand -= step;
                const bool used = std::find(c->ctq.begin(), c->ctq.end(), cand) != c->ctq.end();
                if (!used && is_prime_h(cand)) break;
            }
            c->int_aux.push_back(cand);
            P.mul(cand);
            if ((int)c->int_aux.size() > EXACTO_MAX_K) {
                delete c;
                return invalid_param("too many auxiliary primes required for exact multiplication");
            }
        }
        c->K = (int)c->int_aux.size();
        for (u64 p : c->int_aux) c->primes.push_back(p);
        // |r| <= p n Q / 2 + 1 for every scaled tensor component (|T| <= n Q^2 / 2), so a sum of m of
        // them is liftable from P (centred) when m (p n Q + 2) < P
        Big X(plain);
        X.mul(n);
        for (u64 q : c->ctq) X.mul(q);
        X.add(2);
        for (u64 m = 1; m <= 64; ++m) {
            Big Y = X;
            Y.mul(m);
            if (Y.cmp(P) >= 0) break;
            c->psum_max = (int)m;
        }
        // m (p n Q + 2) <= P / 2, i.e. |R| <= m (p n Q / 2 + 1) <= P / 4: the float CRT is exact
        for (u64 m = 1; m <= 64; ++m) {
            Big Y = X;
            Y.mul(2 * m);
            if (Y.cmp(P) >= 0) break;
            c->psum_fp_max = (int)m;
        }
    }
    hipError_t e = hipSetDevice(device);
    if (e != hipSuccess) { delete c; return fail(EXACTO_ERR_HIP, std::string("HIP error: ") + hipGetErrorString(e)); }
    e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking);
    if (e != hipSuccess) { delete c; return fail(EXACTO_ERR_HIP, std::string("HIP error: ") + hipGetErrorString(e)); }
    c->own_stream = true;
    {
        // Per-call scratch (Scratch) comes from a stream-ordered pool created by the library, one per
        // device and shared by every context on it.  Its freed blocks stay mapped for reuse instead of
        // going back to the driver at every synchronisation (release threshold 0 is the default), and
        // the device's default pool keeps its settings for everything else in the process.
        // One pool per context instead (rounds 1-4; EXACTO_SCRATCH_POOL=own until round 5) made the
        // bootstrap's n = 16 scratch read back zeros written by no kernel of the library in 4 of 20 runs
        // of the C++ API test, 13 of 20 with destroyed contexts' pools kept alive, and 0 of 20 with one
        // pool for all contexts (tools/archive/r4_bootab.sh).  Round 6 removed that mode
        // ("own" now means the shared pool) and moved the bootstrap's intermediates off the pool.
        // The release threshold is read back after it is set: a pool that does not keep it is not used.
        // EXACTO_SCRATCH_POOL=default: the device's default pool (threshold raised there), for A/B
        const char* pe = getenv("EXACTO_SCRATCH_POOL");
        const std::string mode = pe ? pe : "shared";
        uint64_t thr = ~0ull;
        auto make_pool = [&](hipMemPool_t* p) {
            hipMemPoolProps props{};
            props.allocType = hipMemAllocationTypePinned;
            props.location.type = hipMemLocationTypeDevice;
            props.location.id = device;
            if (hipMemPoolCreate(p, &props) != hipSuccess) return (*p = nullptr, false);
            dbg_alloc_log("hipMemPoolCreate", nullptr, 0, *p, nullptr, false);
            uint64_t back = 0;
            const bool set = hipMemPoolSetAttribute(*p, hipMemPoolAttrReleaseThreshold, &thr) == hipSuccess &&
                             hipMemPoolGetAttribute(*p, hipMemPoolAttrReleaseThreshold, &back) == hipSuccess;
            if (dbg_alloc_on())
                std::fprintf(stderr, "exacto-alloc pool %p device %d release threshold set %s, read back 0x%llx\n",
                             (void*)*p, device, set ? "ok" : "FAILED", (unsigned long long)back);
            if (set && back == thr) return true;
            (void)hipMemPoolDestroy(*p);
            return (*p = nullptr, false);
        };
        if (mode != "default") {
            static std::mutex mu;
            static std::map<int, hipMemPool_t> shared;   // never destroyed: lives as long as the process
            std::lock_guard<std::mutex> g(mu);
            auto it = shared.find(device);
            if (it == shared.end()) {
                hipMemPool_t p = nullptr;
                if (make_pool(&p)) it = shared.emplace(device, p).first;
            }
            if (it != shared.end()) c->pool = it->second;
        }
        if (!c->pool) {   // Scratch uses the device's default pool, kept mapped the same way
            hipMemPool_t dp;
            if (hipDeviceGetDefaultMemPool(&dp, device) == hipSuccess)
                (void)hipMemPoolSetAttribute(dp, hipMemPoolAttrReleaseThreshold, &thr);
        }
    }
    if (const char* e = getenv("EXACTO_DEBUG_SCRATCH")) c->debug_scratch = atoi(e) != 0;
    if (const char* e = getenv("EXACTO_DBFV_GROUP_MB")) c->dbfv_group_bytes = (size_t)std::max(1, atoi(e)) << 20;
    if (const char* e = getenv("EXACTO_NTT_ASM")) c->ntt_asm = atoi(e) != 0;
    if (const char* e = getenv("EXACTO_NTT_ASM_INV")) c->ntt_asm_inv = atoi(e) != 0;
    // products per pipeline chunk: 512 at cfg3's n (L + K) = 4096 x 7, more where a product is smaller,
    // so that every chunk's launches (and workspace, ~1.4 GB) stay about the same size (compact_bfv,
    // n = 1024 with L + K = 2: 7168 products per chunk instead of launches of a few blocks per CU)
    c->chunk = (size_t)std::min<long>(8192, std::max<long>(512, 512L * 4096 * 7 / ((long)n * (c->L + c->K)) / 64 * 64));
    if (const char* e = getenv("EXACTO_DUAL_STREAM")) c->dual = atoi(e) != 0;
    if (const char* e = getenv("EXACTO_LANES")) c->lanes = std::max(1, std::min(EXACTO_MAX_LANES, atoi(e)));
    if (const char* e = getenv("EXACTO_SHARE_EXT")) c->share_ext = atoi(e) != 0;
    if (const char* e = getenv("EXACTO_DIGIT16")) c->digit16 = atoi(e) != 0;
    if (const char* e = getenv("EXACTO_KS32")) c->ks32 = atoi(e) != 0;
    if (const char* e = getenv("EXACTO_PSUM")) c->psum_env = atoi(e) != 0;
    if (const char* e = getenv("EXACTO_CHAIN_SPLIT")) c->batch_split = atoi(e) != 0;
    if (const char* e = getenv("EXACTO_FP_CRT")) c->fp_crt = atoi(e) != 0;
    if (const char* e = getenv("EXACTO_FPQ")) c->fpq_lim = atoi(e) == 0 ? 0.0 : atoi(e) == 2 ? 0.25 : c->fpq_lim;
    if (const char* e = getenv("EXACTO_KS_FPC")) c->ks_fpc = atoi(e) != 0;
    if (const char* e = getenv("EXACTO_DIGIT8")) c->digit8_env = atoi(e) != 0;
    if (const char* e = getenv("EXACTO_HPS_SUM")) c->hps_sum_env = atoi(e) != 0;
    c->hps_fast = c->path == EXACTO_PATH_HPS && c->ctq[0] > (1ull << 32) && c->plain < c->ctq[0] &&
                  c->plain < (1ull << 32);
    if (const char* e = getenv("EXACTO_HPS_LITERAL")) c->hps_fast &= atoi(e) == 0;
    if (int rc = build_tables(c)) { exacto_ctx_destroy(c); return rc; }
    if (int rc = setup_ks32(c)) { exacto_ctx_destroy(c); return rc; }
    *out = c;
    return 0;
}

extern "C" void exacto_ctx_destroy(exacto_ctx* c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    for (LaneSet& l : c->xl)
        if (l.stream) (void)hipStreamSynchronize(l.stream);
    // EXACTO_LEAK_CTX=1 (diagnostic of DESIGN.md §3): keep every allocation of a destroyed context
    static const bool leak = [] { const char* e = getenv("EXACTO_LEAK_CTX"); return e && e[0] == '1'; }();
    if (leak) return;
    for (auto& r : c->recs) { (void)hipEventDestroy(r.a); (void)hipEventDestroy(r.b); }
    for (LaneSet& l : c->xl) {
        if (l.stream) (void)hipStreamDestroy(l.stream);
        if (l.join) (void)hipEventDestroy(l.join);
    }
    if (c->ev_fork) (void)hipEventDestroy(c->ev_fork);
    for (int i = 0; i < exacto_ctx::MAX_TWINS; ++i) {
        if (c->twin[i]) exacto_ctx_destroy(c->twin[i]);
        if (c->ev_twin_out[i]) (void)hipEventDestroy(c->ev_twin_out[i]);
    }
    if (c->ev_twin_in) (void)hipEventDestroy(c->ev_twin_in);
    if (c->own_stream && c->stream) (void)hipStreamDestroy(c->stream);
    delete c;   // every device buffer is a DevBuf member: released here
}

extern "C" int exacto_ctx_get_info(const exacto_ctx* c, exacto_ctx_info* info) {
    if (!c || !info) return invalid_param("null argument");
    info->ring_degree = c->n;
    info->num_ct_moduli = c->L;
    info->num_aux_moduli = c->user_aux.size();
    info->num_internal_aux = c->int_aux.size();
    info->gadget_digits = c->G;
    info->gadget_base = c->gbase;
    info->plain_modulus = c->plain;
    info->mul_path = c->path;
    info->device = c->device;
    info->ks32_primes = c->ks32 ? c->S32 : 0;
    info->psum_max = c->psum_env ? c->psum_max : 0;
    info->ks32_lazy = c->ks32 && c->ks32_lazy_active ? 1 : 0;
    info->ntt_order = EXACTO_NTT_ORDER;
    info->dbfv_key_switch = c->last_dbfv_ks;
    return 0;
}

extern "C" int exacto_ctx_set_stream(exacto_ctx* c, void* s) {
    // The handle is used as given; NULL is the device's default (null) stream, which is what
    // torch.cuda.current_stream().cuda_stream returns for the default torch stream.
    if (!c) return invalid_param("null context");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (c->own_stream && c->stream) HIP_TRY(hipStreamDestroy(c->stream));
    c->stream = (hipStream_t)s;
    c->own_stream = false;
    return 0;
}

extern "C" int exacto_ctx_set_chunk(exacto_ctx* c, size_t chunk) {
    if (!c) return invalid_param("null context");
    c->chunk = chunk == 0 ? 128 : chunk;
    return 0;
}

extern "C" int exacto_ctx_set_plain_terms(exacto_ctx* c, size_t terms) {
    if (!c) return invalid_param("null context");
    c->plain_terms = terms == 0 ? 64 : terms;
    return 0;
}

extern "C" int exacto_ctx_set_square_hook(exacto_ctx* c, int on) {
    if (!c) return invalid_param("null context");
    c->square_hook = on != 0;
    return 0;
}

extern "C" int exacto_synchronize(exacto_ctx* c) {
    if (!c) return invalid_param("null context");
    HIP_TRY(hipStreamSynchronize(c->stream));
    return 0;
}

size_t exacto::poly_bytes(const exacto_ctx* c) { return (size_t)c->n * sizeof(u64); }

extern "C" uint64_t* exacto_ctx_relin_key_buffer(exacto_ctx* c, size_t num_keys) {
    if (!c) return nullptr;
    const size_t bytes = num_keys * 2 * c->L * poly_bytes(c);
    if (hipSetDevice(c->device) != hipSuccess) return nullptr;
    if (c->d_rlk.grow(bytes)) return nullptr;
    c->rlk_keys = num_keys;
    c->rlk_loaded = true;
    c->rlk_s_valid = false;  // contents change: companions recomputed before first use
    c->rs_valid = false; c->kw.rs_valid = false;     // and the auxiliary-basis key
    ++c->rlk_version;
    return c->d_rlk;
}

extern "C" int exacto_ctx_load_relin_key_dev(exacto_ctx* c, const uint64_t* rlk, size_t num_keys) {
    if (!c) return invalid_param("null context");
    if (num_keys && !rlk) return invalid_param("null relinearization key");
    u64* dst = exacto_ctx_relin_key_buffer(c, num_keys);
    if (!dst) return fail(EXACTO_ERR_HIP, "HIP error: relinearization key allocation failed");
    if (num_keys)
        HIP_TRY(dev_copy(dst, rlk, num_keys * 2 * c->L * poly_bytes(c), c->stream));
    return 0;
}

extern "C" int exacto_ctx_load_relin_key(exacto_ctx* c, const uint64_t* rlk, size_t num_keys) {
    if (!c) return invalid_param("null context");
    if (num_keys && !rlk) return invalid_param("null relinearization key");
    u64* dst = exacto_ctx_relin_key_buffer(c, num_keys);
    if (!dst) return fail(EXACTO_ERR_HIP, "HIP error: relinearization key allocation failed");
    if (num_keys) if (int e_ = upload(c, dst, rlk, num_keys * 2 * c->L * poly_bytes(c))) return e_;
    return 0;
}

// ============================================================== NTT helper (+ profiling)

int exacto::run_ntt(exacto_ctx* c, const NttBatch& nb, long count, bool inverse) {
    if (count <= 0) return 0;
    // algorithmic bytes: one read of the source (int16 digits: 2 B per coefficient) + one 8 B write
    ProfScope ps(c, inverse ? PK_INV : PK_FWD, (u64)count, ((nb.src16 ? 2.0 : 8.0) + 8.0) * c->n * (double)count);
    bool lazy = true, near60 = c->ntt_asm;
    int qbits = 0;   // bit length of the batch's largest prime
    for (int t = nb.prime_base; t < nb.prime_base + nb.period; ++t) {
        lazy &= c->primes[t] < (1ull << 60);
        near60 &= c->primes[t] < (1ull << 60) && c->primes[t] > (1ull << 60) - (1ull << 32);
        qbits = std::max(qbits, 64 - __builtin_clzll(c->primes[t]));
    }
    launch_ntt(nb, (int)count, c->logn, inverse, lazy, c->d_primes, c->stream, near60, near60 && c->ntt_asm_inv, qbits);
    CHECK_LAUNCH();
    return 0;
}

// two forward batches in one launch where both take the pinned rounds (every prime 2^60 - d, n = 4096
// / 8192), else two launches
static int run_ntt_fwd2(exacto_ctx* c, const NttBatch& nb1, long count1, const NttBatch& nb2, long count2) {
    bool near60 = c->ntt_asm && !nb1.src16 && !nb2.src16;
    for (u64 q : c->primes) near60 &= q < (1ull << 60) && q > (1ull << 60) - (1ull << 32);
    if (near60 && count1 > 0 && count2 > 0) {
        ProfScope ps(c, PK_FWD, (u64)(count1 + count2), 16.0 * c->n * (double)(count1 + count2));
        if (launch_ntt_fwd2(nb1, (int)count1, nb2, (int)count2, c->logn, c->d_primes, c->stream)) {
            CHECK_LAUNCH();
            return 0;
        }
    }
    if (int e = run_ntt(c, nb1, count1, false)) return e;
    return run_ntt(c, nb2, count2, false);
}

// the tensor runs the asm kernels (products by MulNear60*Asm, special-prime inverse rounds)
static bool tensor_asm(const exacto_ctx* c) {
    bool near60 = c->ntt_asm && c->ntt_asm_inv;
    for (int t = 0; t < c->L + c->K; ++t)   // the fused product needs d = 2^60 - q < 2^24
        near60 &= c->primes[t] < (1ull << 60) && c->primes[t] > (1ull << 60) - (1ull << 24);
    return near60;
}

// The folded scale (EXACTO_CRT_FOLD): the tensor's last inverse stage multiplies by the constants the
// float-sum scale would apply first, and the scale reads that form.  One decision for both launches of
// run_mul: the asm special-prime tensor at n = 4096 with lazy outputs, and exact_scale_sp's FPQ form.
static int crt_mode(const exacto_ctx* c);
static bool scale_fold(const exacto_ctx* c) {
    return c->path != EXACTO_PATH_HPS && crt_fold_tensor_ok(c->logn, tensor_asm(c), true) &&
           exact_scale_fold_ok(c->L, c->K, crt_mode(c), c->fp_crt, c->fpq_lim);
}

static int run_inv_tensor(exacto_ctx* c, const Operands& o, int cnt, bool p2only = false, bool fold = false,
                          bool square = false) {
    const int NP = c->L + c->K;
    bool lazy = true;
    const bool near60 = tensor_asm(c);
    int qbits = 0;
    for (int t = 0; t < NP; ++t) {
        qbits = std::max(qbits, 64 - __builtin_clzll(c->primes[t]));
        lazy &= c->primes[t] < (1ull << 60);
    }
    // algorithmic bytes per (item, prime): the four operands a0, a1, b0, b1 in and the three
    // components out (7 polys); psum's auxiliary primes only c2 = a1 b1 (2 in, 1 out).  dBFV with
    // shared extensions (tensor_share_d > 0): the d^2 products of an item read only its 2d distinct
    // ciphertexts, so the inputs count once per ciphertext (the chunk's ceil(cnt / npairs) items),
    // not once per product (which overcounted: u64_dbfv's measured traffic was 0.95 of it)
    const double pb = 8.0 * c->n;
    double bytes;
    if (c->tensor_share_d > 0 && c->tensor_share_npairs > 0) {
        const double items = (double)((cnt + c->tensor_share_npairs - 1) / c->tensor_share_npairs);
        const double cts = items * 2.0 * c->tensor_share_d;
        bytes = pb * (c->L * (2.0 * cts + 3.0 * cnt) +
                      c->K * (p2only ? cts + (double)cnt : 2.0 * cts + 3.0 * cnt));
    } else {
        // (a square reads its one operand's two polynomials: 5 polys)
        bytes = cnt * (p2only ? pb * (7.0 * c->L + 3.0 * c->K) : pb * (square ? 5.0 : 7.0) * NP);
    }
    ProfScope ps(c, PK_TENSOR, (u64)cnt * (p2only ? 3 * c->L + c->K : 3 * NP), bytes);
    // the exact path's scale kernels take T in [0, 2q) (shoup products, 30-bit-limb dot products with
    // headroom); the HPS scale subtracts residues as canonical
    launch_inv_tensor(o, c->ws.extP, c->ws.T, cnt, c->logn, c->L, c->K, lazy, c->d_primes, c->stream, near60, p2only,
                      qbits, c->tensor_share_npairs, near60 && c->path != EXACTO_PATH_HPS, fold, square);
    CHECK_LAUNCH();
    return 0;
}

NttBatch exacto::contiguous(u64* data, long count_items, long poly_per_item, int prime_base, int period,
                            int n) {
    (void)count_items;
    NttBatch nb{};
    nb.src = data;
    nb.src_off = nullptr;
    nb.src_item_stride = poly_per_item * n;
    nb.dst = data;
    nb.dst_item_stride = poly_per_item * n;
    nb.ppi = (int)poly_per_item;
    nb.prime_base = prime_base;
    nb.period = period;
    return nb;
}

// ============================================================== workspace

// The one copy of the workspace sizes.  Every buffer is released before the first is allocated; a
// failed allocation leaves items at 0, so the next call allocates again.
int Workspace::ensure(const exacto_ctx* c, size_t want) {
    if (items >= want) return 0;
    items = 0;
    coefQ.reset(); extP.reset(); T.reset(); D.reset(); D16.reset(); DS.reset(); U.reset();
    const size_t pb = poly_bytes(c);
    const int NP = c->L + c->K;
    if (int e = coefQ.alloc(want * 4 * c->L * pb)) return e;
    if (int e = extP.alloc(want * 4 * std::max(c->K, 1) * pb)) return e;
    if (int e = T.alloc(want * 3 * NP * pb)) return e;
    if (int e = D.alloc(want * std::max(c->G, 1) * c->L * pb)) return e;
    if (int e = D16.alloc(want * std::max(c->G, 1) * c->n * sizeof(int16_t))) return e;
    if (c->S32) {
        if (int e = DS.alloc(want * std::max(c->G, 1) * c->S32 * c->n * sizeof(uint32_t))) return e;
        if (int e = U.alloc(want * 2 * c->L * c->S32 * c->n * sizeof(uint32_t))) return e;
    }
    items = want;
    return 0;
}

// Extra pipeline lane `idx` (1 ..): its stream, join event and workspace (allocated on first use).
static int ensure_lane(exacto_ctx* c, int idx, size_t items) {
    if (!c->ev_fork) HIP_TRY(hipEventCreateWithFlags(&c->ev_fork, hipEventDisableTiming));
    LaneSet& l = c->xl[idx - 1];
    if (!l.stream) HIP_TRY(hipStreamCreateWithFlags(&l.stream, hipStreamNonBlocking));
    if (!l.join) HIP_TRY(hipEventCreateWithFlags(&l.join, hipEventDisableTiming));
    return l.ws.ensure(c, items);
}

// Points the context's stream and workspace at lane idx (> 0) for the lifetime of the guard.
struct LaneGuard {
    exacto_ctx* c;
    int idx;
    LaneGuard(exacto_ctx* c_, int idx_) : c(c_), idx(idx_) { if (idx > 0) flip(); }
    LaneGuard(const LaneGuard&) = delete;
    LaneGuard& operator=(const LaneGuard&) = delete;
    ~LaneGuard() { if (idx > 0) flip(); }
    void flip() {
        LaneSet& l = c->xl[idx - 1];
        std::swap(c->stream, l.stream);
        std::swap(c->ws, l.ws);
    }
};

// One pass of nchunks chunks of C items over the lanes.  begin() sizes lane 0's workspace and forks
// the extra lanes off c->stream (their streams wait for everything enqueued so far, so whatever
// their kernels read -- converted keys, per-lane scratch -- is made before it); chunk i runs under
// chunk(i), on lane i % lanes(); the destructor makes c->stream wait for the extra lanes again, also
// on an error return from inside the chunk loop (the chunk's guard has flipped back by then).
// Profiling keeps one lane, so that its per-kernel events time each kernel alone.
struct LanePass {
    exacto_ctx* c = nullptr;
    int nl = 1;
    LanePass() = default;
    LanePass(const LanePass&) = delete;
    LanePass& operator=(const LanePass&) = delete;
    static int count(const exacto_ctx* c, long nchunks) {
        return (c->dual && !c->prof) ? (int)std::min<long>(c->lanes, nchunks) : 1;
    }
    int begin(exacto_ctx* c_, long nchunks, size_t C) {
        c = c_;
        if (int e = c->ws.ensure(c, C)) return e;
        const int want = count(c, nchunks);
        if (want <= 1) return 0;
        for (int i = 1; i < want; ++i)
            if (int e = ensure_lane(c, i, C)) return e;
        HIP_TRY(hipEventRecord(c->ev_fork, c->stream));
        for (int i = 1; i < want; ++i) HIP_TRY(hipStreamWaitEvent(c->xl[i - 1].stream, c->ev_fork, 0));
        nl = want;   // (a failed fork joins nothing)
        return 0;
    }
    ~LanePass() {
        for (int i = 1; i < nl; ++i)
            if (hipEventRecord(c->xl[i - 1].join, c->xl[i - 1].stream) == hipSuccess)
                (void)hipStreamWaitEvent(c->stream, c->xl[i - 1].join, 0);
    }
    int lanes() const { return nl; }
    LaneGuard chunk(long i) const { return LaneGuard(c, (int)(i % nl)); }
};

static int ensure_rlk_companions(exacto_ctx* c) {
    if (c->rlk_s_valid) return 0;
    const size_t count = c->rlk_keys * 2 * c->L * (size_t)c->n;
    if (c->d_rlk_s.grow(count * sizeof(u64))) return EXACTO_ERR_HIP;
    launch_shoup_companions(c->d_rlk, c->d_rlk_s, (long)count, c->n, c->L, c->d_primes, c->stream);
    CHECK_LAUNCH();
    c->rlk_s_valid = true;
    return 0;
}

// CRT kernel variant: 3 special-prime reductions, 2 lazy (fast), 1 near primes, 0 generic
static int crt_mode(const exacto_ctx* c) {
    return c->h_crt.special ? 3 : c->h_crt.fast ? 2 : c->h_crt.near ? 1 : 0;
}

// A key [keys][2][L][n] (NTT domain mod q_l) in ks32's auxiliary basis: INTT mod q_l
// (coefficient domain), balanced, reduced mod each p_s, forward NTT mod p_s -> dst [keys][2L][S][n]
// (grown as needed).
static int ks32_convert_key(exacto_ctx* c, const u64* key, size_t keys, DevBuf<uint32_t>& dst, int S = 0,
                            const Prime32* p32 = nullptr, int form = 0) {
    if (!S) { S = c->S32; p32 = c->d_p32; form = c->ks32_mac_form; }
    const long rows = (long)keys * 2 * c->L;
    if (dst.grow((size_t)rows * S * c->n * sizeof(uint32_t))) return EXACTO_ERR_HIP;
    Scratch ks;
    HIP_TRY(ks.alloc((size_t)rows * c->n * sizeof(u64), c->stream, c->pool, c->debug_scratch));
    NttBatch nb{};
    nb.src = key; nb.src_item_stride = 2L * c->L * c->n;
    nb.dst = ks.as<u64>(); nb.dst_item_stride = 2L * c->L * c->n;
    nb.ppi = 2 * c->L; nb.prime_base = 0; nb.period = c->L;
    if (int e = run_ntt(c, nb, rows, true)) return e;
    ks32_key(ks.as<u64>(), dst, rows, c->L, S, c->logn, p32, c->d_primes, form, c->stream);
    CHECK_LAUNCH();
    return 0;
}

#ifndef EXACTO_KN_NORM
#define EXACTO_KN_NORM 1   // the narrow basis' digit-sum limit from the key's norms too (A/B build switch)
#endif
// The primary basis for the resident key: the lazy one (kz) when the key's own norms bound the key
// switch, |u_{c,l}| <= ceil(B/2) sum_g ||r_{g,c,l}||_1 with ||r||_1 <= (sum floor(|r_j|/2^20) + n) 2^20
// (ks32_key_norm_kernel), for every (c, l): prod p > 2 m bound for m = 1 (and sum_max = the largest
// such m <= 64 for dBFV digit sums); otherwise the narrow one (kn), whose bound holds for any key.
static int ks32_select_basis(exacto_ctx* c) {
    use_ks32_basis(c, c->kn);
    if (c->kz.S == 0 || c->rlk_keys == 0) return 0;
    const long rows = (long)c->rlk_keys * 2 * c->L, CL = 2L * c->L;
    Scratch ks, nr;
    HIP_TRY(ks.alloc((size_t)rows * c->n * sizeof(u64), c->stream, c->pool, c->debug_scratch));
    HIP_TRY(nr.alloc((size_t)rows * sizeof(u64), c->stream, c->pool, c->debug_scratch));
    NttBatch nb{};
    nb.src = c->d_rlk; nb.src_item_stride = CL * c->n;
    nb.dst = ks.as<u64>(); nb.dst_item_stride = CL * c->n;
    nb.ppi = (int)CL; nb.prime_base = 0; nb.period = c->L;
    if (int e = run_ntt(c, nb, rows, true)) return e;
    ks32_key_norms(ks.as<u64>(), nr.as<u64>(), rows, c->L, c->n, c->d_primes, c->stream);
    CHECK_LAUNCH();
    std::vector<u64> h((size_t)rows);
    HIP_TRY(hipMemcpyAsync(h.data(), nr.as<u64>(), h.size() * sizeof(u64), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    Big worst(0);
    for (long cl = 0; cl < CL; ++cl) {
        Big acc(0);
        for (size_t g = 0; g < c->rlk_keys; ++g) {
            Big t(h[(size_t)g * CL + cl] + (u64)c->n);
            t.mul(1ull << 20);
            acc.add(t);
        }
        if (acc.cmp(worst) > 0) worst = acc;
    }
    worst.mul(digit_max(c->gbase));
    // sums the lazy / the narrow basis lift for this key (its norms, not the analytic bound), by the
    // Garner and by the float-CRT lift
    const int sm = sums_lifted(c->kz.P, worst, false);
    const int snm = EXACTO_KN_NORM ? sums_lifted(c->kn.P, worst, false) : 0;
    const int fsm = sums_lifted(c->kz.P, worst, true);   // lazy and narrow primes: any S (ks32_crt)
    const int fsnm = EXACTO_KN_NORM && (c->kn.S <= 3 || c->kn.mac_form != 0) ? sums_lifted(c->kn.P, worst, true) : 0;
    // the narrow basis with the key's own bound: cfg4's two-product digit sums (2^90.6) fit its 2^91.2,
    // which the analytic bound (2^91.6) refused -- they then take the narrow form instead of the wide one
    c->ks32_sum_max = std::max(c->kn.sum_max, snm);
    c->ks32_fpc_max = std::max(c->kn.fpc_max, fsnm);
    const int kn_sum = c->ks32_sum_max;
    // never a basis that lifts fewer sums than the narrow one where those sums are needed (a dBFV digit
    // sum the lazy basis cannot hold would otherwise drop to the per-product key switch)
    if (sm >= 1 && sm >= std::min(kn_sum, std::max(1, c->ks32_need_m))) {
        c->kz.sum_max = sm;
        c->kz.fpc_max = fsm;
        use_ks32_basis(c, c->kz);
    }
    return 0;
}

// The resident relinearisation key in ks32's basis (d_rs), the basis chosen for it first.  Once per key.
static int ensure_rs(exacto_ctx* c) {
    if (c->rs_valid) return 0;
    if (int e = ks32_select_basis(c)) return e;
    if (int e = ks32_convert_key(c, c->d_rlk, c->rlk_keys, c->d_rs)) return e;
    c->rs_valid = true;
    return 0;
}

// ... and in the wide basis (dBFV digit sums), on first use after each key load
static int ensure_rs_wide(exacto_ctx* c) {
    if (c->kw.rs_valid) return 0;
    if (int e = ks32_convert_key(c, c->d_rlk, c->rlk_keys, c->kw.d_rs, c->kw.S, c->kw.d_p32, c->kw.mac_form)) return e;
    c->kw.rs_valid = true;
    return 0;
}

// ============================================================== multiplication pipeline

// products [0, P): ct1 = op.a + off_a(p), ct2 = op.b + off_b(p) (each [2][L][n], NTT domain).
// relin: out[p] = [2][L][n] = relinearize(mul_no_relin); else out[p] = [3][L][n].
// coef (optional): when the key switch runs over the integers (ks32), the last forward NTT is left
// to the caller and *coef is set: out then holds the coefficient domain (a caller that first sums
// products, as dbfv_mul does, transforms the sums instead of every product).
// square: product p is op.a's ciphertext times itself (op.b is never read): steps 1-3 run over its two
// polynomials only, coefQ[item] = [c0, c1] and extP[item] = [a0, a1] at a two-polynomial stride, and the
// tensor takes its square form; from the scale on nothing differs.
static int run_mul(exacto_ctx* c, const Operands& op, long P, u64* out, long out_stride, bool relin,
                   bool* coef = nullptr, bool square = false) {
    if (coef) *coef = false;
    if (c->deferred_code) return fail(c->deferred_code, c->deferred_msg);
    if (relin && !c->rlk_loaded) return fail(EXACTO_ERR_MISSING_KEY, "key not available: relinearization key not loaded");
    if (P <= 0) return 0;
    const int n = c->n, L = c->L, K = c->K;
    const long Ln = (long)L * n;
    const int guse = relin ? (int)std::min<size_t>(c->G, c->rlk_keys) : 0;
    const exacto_ctx::PsumPlan& ps = c->psum;
    // psum: chunks hold whole dBFV items (their products are summed inside the chunk)
    size_t C = ps.on ? std::max<size_t>(ps.npairs, std::min<size_t>(c->chunk, (size_t)P) / ps.npairs * ps.npairs)
                     : std::min<size_t>(c->chunk, (size_t)P);
    // a batch that fits one chunk still takes two lanes when each half has work enough (>= 64
    // products): the halves fill each other's launch tails (cfg5, 288 products per dbfv_mul: 1837 ->
    // 1889 chains/s with two chunks of 144; four chunks of 72 measured 1800)
    if (c->dual && !c->prof && c->lanes > 1 && (size_t)P <= C && P >= 128) {
        size_t half = ((size_t)P + 1) / 2;
        if (ps.on) half = (half + ps.npairs - 1) / ps.npairs * ps.npairs;
        if (half < (size_t)P) C = half;
    }
    // int16 gadget digits (base <= 2^16, exact path): the scale kernel writes each digit once
    const bool d16 = relin && guse > 0 && c->digit16 && c->path != EXACTO_PATH_HPS &&
                     c->gbase <= 65536;
    // ... and then the key switch runs over the integers in the 31-bit basis (ks32.hip)
    const bool k32 = d16 && c->ks32 && c->S32 > 0;
    // HPS in dbfv_mul (dbfv_mul_group): the scale writes each product's signed digits to ks_defer,
    // c0 / c1 stay in the coefficient domain; the caller sums both per output limb, then transforms
    // and relinearises once per limb
    const bool hps_defer = c->path == EXACTO_PATH_HPS && relin && guse > 0 && c->ks_defer && coef;
    const bool skip_fwd = coef && (k32 || hps_defer);
    if (skip_fwd) *coef = true;
    if (relin && guse > 0) {
        // both before the second lane forks: its kernels read these too
        // (a deferred key switch -- dbfv_mul_core's digit sums -- has already made the key for the basis
        // it uses, which may be the wide one: the primary form would be built and never read)
        if (int e = k32 ? (c->ks_defer ? 0 : ensure_rs(c)) : ensure_rlk_companions(c)) return e;
    }
    // two chunks or more: odd chunks on the second lane
    LanePass pass;
    if (int e = pass.begin(c, (P + (long)C - 1) / (long)C, C)) return e;
    for (long s = 0; s < P; s += (long)C) {
        const int cnt = (int)std::min<long>((long)C, P - s);
        LaneGuard lane = pass.chunk(s / (long)C);
        Operands o = op;
        if (o.a_off) o.a_off += s; else o.a += s * o.a_stride;
        if (square) { o.b = nullptr; o.b_off = nullptr; }
        else if (o.b_off) o.b_off += s; else o.b += s * o.b_stride;
        if (!o.ea) {
            // 1. inputs -> coefficient domain (INTT), coefQ[item] = [c0, c1, d0, d1][L][n]
            // (square: [c0, c1][L][n])
            const long ip = square ? 2 : 4;   // input polynomials per product
            NttBatch nb{};
            nb.src = o.a; nb.src_off = o.a_off; nb.src_item_stride = o.a_stride;
            nb.dst = c->ws.coefQ; nb.dst_item_stride = ip * Ln;
            nb.ppi = 2 * L; nb.prime_base = 0; nb.period = L;
            if (int e = run_ntt(c, nb, (long)cnt * 2 * L, true)) return e;
            if (!square) {
                nb.src = o.b; nb.src_off = o.b_off; nb.src_item_stride = o.b_stride;
                nb.dst = c->ws.coefQ + 2 * Ln;
                if (int e = run_ntt(c, nb, (long)cnt * 2 * L, true)) return e;
            }
            // 2. extension to the auxiliary primes
            if (c->path == EXACTO_PATH_HPS) {
                // per input poly: the q residues in, K auxiliary residues out
                ProfScope pl(c, PK_HPS_EXT, (u64)ip * cnt, 8.0 * (1 + K) * n * (double)ip * cnt);
                launch_hps_extend(c->ws.coefQ, c->ws.extP, ip * cnt, n, c->d_primes, K, c->stream);
            } else {
                ProfScope pl(c, PK_LIFT, (u64)ip * cnt, 8.0 * (L + K) * n * (double)ip * cnt);
                launch_exact_lift(c->ws.coefQ, c->ws.extP, ip * cnt, n, c->d_crt, c->d_primes, L, K,
                                  crt_mode(c), c->stream);
            }
            CHECK_LAUNCH();
            // 3. forward NTT of the extended polynomials (exact path with the asm tensor, its only
            // reader: outputs left in [0, 2q), which its products take)
            NttBatch eb = contiguous(c->ws.extP, cnt, ip * K, L, K, n);
            eb.lazy_out = c->path != EXACTO_PATH_HPS && tensor_asm(c);
            if (int e = run_ntt(c, eb, (long)cnt * ip * K, false)) return e;
        } else {
            o.ea_off += s;
            o.eb_off += s;
        }
        // 4+5. tensor product in every prime, fused into the inverse NTT of its components
        // (psum's readers of T, fpq_acc, sum up to 15 canonical z_i: they keep the unfolded form)
        const bool tfold = !ps.on && scale_fold(c);
        if (int e = run_inv_tensor(c, o, cnt, ps.on, tfold, square)) return e;
        if (ps.on) {
            // the output limbs' c0 / c1 auxiliary residues, summed over their products, then inverse-
            // transformed: [ib][k][c][a][n] in extP (unused: the extensions are shared, steps 1-3 skipped)
            const int ib_cnt = cnt / ps.npairs;
            {   // per (item, prime): the 2d input ciphertexts' two polys in, 2 sums per output limb out
                ProfScope pp(c, PK_PAIRSUM, (u64)ib_cnt * K * ps.d, 8.0 * n * K * ib_cnt * (4.0 * ps.d + 2.0 * ps.d));
                launch_dbfv_pairsum(o, c->ws.extP, ib_cnt, ps.d, ps.npairs, ps.term_start, ps.terms, L, K, n,
                                    c->d_primes, c->stream);
            }
            CHECK_LAUNCH();
            if (int e = run_ntt(c, contiguous(c->ws.extP, (long)ib_cnt * ps.d, 2L * K, L, K, n),
                                (long)ib_cnt * ps.d * 2 * K, true))
                return e;
        }
        // 6. scale-and-round (+ gadget digits of the third component)
        u64* R = out + s * out_stride;
        const int ncomp = relin ? 2 : 3;
        u64* D = relin ? c->ws.D : nullptr;
        // scale bytes per item: the three components' L+K residues in; c0, c1 (L residues each) out
        // (psum: c2 only), and the third component's digits (int16 / int8) or its L residues
        const double dig_b = (d16 || hps_defer) ? (c->ks_defer && c->ks_defer8 ? 1.0 : 2.0) * guse
                                                : 8.0 * L * (relin ? guse : 1);
        {   // (scoped: the events bracket the scale launch alone)
        ProfScope psc(c, c->path == EXACTO_PATH_HPS ? PK_HPS_SCALE : PK_SCALE, (u64)cnt, (double)n * cnt *
                      ((ps.on ? 1.0 : 3.0) * 8.0 * (L + K) + (ps.on ? 0.0 : 16.0 * L) + (relin ? dig_b : 8.0 * L)));
        if (c->path == EXACTO_PATH_HPS) {
            void* d16p = hps_defer ? (c->ks_defer8 ? (void*)((int8_t*)c->ks_defer + s * (long)guse * n)
                                                   : (void*)(c->ks_defer + s * (long)guse * n))
                                   : nullptr;
            launch_hps_scale(c->ws.T, R, out_stride, ncomp, hps_defer ? nullptr : D, d16p,
                             hps_defer && c->ks_defer8, guse, cnt, n, c->d_crt, c->d_primes, K, c->hps_fast,
                             c->stream);
        } else
            launch_exact_scale(c->ws.T, R, out_stride, ncomp, d16 ? nullptr : D,
                               d16 ? (c->ks_defer ? (c->ks_defer8
                                                         ? (int16_t*)((int8_t*)c->ks_defer + s * (long)guse * n)
                                                         : c->ks_defer + s * (long)guse * n)
                                                  : c->ws.D16)
                                   : nullptr,
                               guse, cnt, n, c->d_crt, c->d_primes, L, K, crt_mode(c),
                               c->stream, c->h_crt.gshift, ps.on, c->ks_defer && c->ks_defer8, c->fp_crt, c->fpq_lim,
                               tfold);
        CHECK_LAUNCH();
        }
        if (ps.on) {   // ... and their scale: the output limbs' c0 / c1, coefficient domain
            const long item0 = s / ps.npairs;
            const double ib = (double)(cnt / ps.npairs);
            // per item: each limb's summed auxiliary residues (K) and its products' ciphertext-prime
            // residues (L each) in, the limb's L residues out, for c0 and c1
            ProfScope pq(c, PK_PSUM_SCALE, (u64)(cnt / ps.npairs) * ps.d,
                         ib * 2.0 * n * 8.0 * (ps.d * (double)(K + L) + (double)ps.npairs * L));
            if (!launch_psum_scale(c->ws.T, c->ws.extP, ps.out + item0 * ps.d * 2 * Ln, cnt / ps.npairs, ps.d, ps.npairs,
                                   ps.term_start, ps.terms, n, c->d_crt, c->d_primes, L, c->stream, ps.fpc,
                                   c->fpq_lim))
                return fail(EXACTO_ERR_HIP, "internal: psum scale not available for these limbs");
            CHECK_LAUNCH();
        }
        // 7. forward NTT of the results (and digits)
        NttBatch rb{};
        rb.src = R; rb.src_off = nullptr; rb.src_item_stride = out_stride;
        rb.dst = R; rb.dst_item_stride = out_stride;
        rb.ppi = ncomp * L; rb.prime_base = 0; rb.period = L;
        if (k32) {
            // 7'+8'. the key switch over the integers (ks32.hip): digits -> NTT mod p_s, MAC with the
            // key in the same basis, inverse NTT + centred lift, added to R mod q_l in the
            // coefficient domain; the forward NTT of R below then yields the relinearised result
            if (!c->ks_defer) {   // (deferred: the caller sums the digits of products first, dbfv_mul_core)
                {   // int16 digit in (2 B), 31-bit residue out (4 B) per coefficient and prime
                    ProfScope pd(c, PK_KS_DIGITS, (u64)cnt * guse * c->S32, 6.0 * n * cnt * guse * c->S32);
                    ks32_digits(c->ws.D16, c->ws.DS, cnt, guse, c->S32, c->logn, c->d_p32, c->ks32_mac_form, c->stream);
                }
                {   // per (item, prime, coefficient): G digit residues in, 2L sums out (the key slice from LDS)
                    ProfScope pm(c, PK_KS_MAC, (u64)cnt * c->S32, 4.0 * n * cnt * c->S32 * (guse + 2.0 * L));
                    ks32_mac(c->ws.DS, c->d_rs, c->ws.U, cnt, guse, L, c->S32, n, c->d_p32, c->ks32_mac_form, c->stream);
                }
                {   // per (item, component, limb): S 31-bit sums in, R in and out
                    ProfScope pc(c, PK_KS_CRT, (u64)cnt * 2 * L, (double)n * cnt * 2 * L * (4.0 * c->S32 + 16.0));
                    ks32_crt(c->ws.U, R, out_stride, cnt, L, c->S32, c->logn, c->d_kst, c->d_p32, c->d_primes, c->ks32_mac_form,
                             c->stream, c->ks_fpc && c->ks32_fpc_max >= 1);
                }
                CHECK_LAUNCH();
            }
        }
        if (skip_fwd) continue;   // (hps_defer: digits and c0 / c1 are the caller's now)
        if (int e = run_ntt(c, rb, (long)cnt * ncomp * L, false)) return e;
        if (relin && guse > 0 && !k32) {
            NttBatch db = contiguous(c->ws.D, cnt, (long)guse * L, 0, L, n);
            if (d16) {  // int16 digits [item][g][n] -> NTT residues [item][g][L][n]
                db.src16 = c->ws.D16;
                db.src16_item_stride = (long)guse * n;
            }
            if (int e = run_ntt(c, db, (long)cnt * guse * L, false)) return e;
            // 8. relinearisation MAC, in place on the output
            if (int e = ensure_rlk_companions(c)) return e;
            {   // per item: c0, c1 and the G digit residues in, c0, c1 out (the key from LDS)
                ProfScope pm(c, PK_RELIN_MAC, (u64)cnt, 8.0 * n * L * cnt * (4.0 + guse));
                launch_relin_mac(R, out_stride, c->ws.D, c->d_rlk, c->d_rlk_s, guse, R, out_stride, cnt, n, L,
                                 c->d_primes, c->stream);
            }
            CHECK_LAUNCH();
        }
    }
    return 0;
}

// ============================================================== C ABI: NTT / RNS

int exacto::check_ctx(exacto_ctx* c) {
    if (!c) return invalid_param("null context");
    HIP_TRY(hipSetDevice(c->device));
    return 0;
}

static int ntt_dev(exacto_ctx* c, uint64_t* polys, size_t count, size_t limb, bool inverse) {
    if (int e = check_ctx(c)) return e;
    if (limb >= (size_t)c->L)
        // the reference's Display text ("expected {expected}, got {got}", error.rs:8-9): the context's
        // limb count and the limb index asked for
        return fail(EXACTO_ERR_DIMENSION_MISMATCH, "dimension mismatch: expected " + std::to_string(c->L) + ", got " +
                                                       std::to_string(limb));
    return run_ntt(c, contiguous(polys, count, 1, (int)limb, 1, c->n), (long)count, inverse);
}

extern "C" int exacto_ntt_fwd_dev(exacto_ctx* c, uint64_t* p, size_t count, size_t limb) { return ntt_dev(c, p, count, limb, false); }
extern "C" int exacto_ntt_inv_dev(exacto_ctx* c, uint64_t* p, size_t count, size_t limb) { return ntt_dev(c, p, count, limb, true); }

extern "C" int exacto_rns_fwd_dev(exacto_ctx* c, uint64_t* p, size_t count) {
    if (int e = check_ctx(c)) return e;
    return run_ntt(c, contiguous(p, count, c->L, 0, c->L, c->n), (long)count * c->L, false);
}
extern "C" int exacto_rns_inv_dev(exacto_ctx* c, uint64_t* p, size_t count) {
    if (int e = check_ctx(c)) return e;
    return run_ntt(c, contiguous(p, count, c->L, 0, c->L, c->n), (long)count * c->L, true);
}

static int stage(exacto_ctx* c, size_t bytes) {
    if (c->io.grow(bytes)) return EXACTO_ERR_HIP;
    return 0;
}

static int ntt_host(exacto_ctx* c, uint64_t* polys, size_t count, size_t limb, bool inverse) {
    if (int e = check_ctx(c)) return e;
    const size_t bytes = count * poly_bytes(c);
    if (int e = stage(c, bytes)) return e;
    if (int e_ = upload(c, c->io, polys, bytes)) return e_;
    if (int e = ntt_dev(c, c->io, count, limb, inverse)) return e;
    HIP_TRY(hipMemcpyAsync(polys, c->io, bytes, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return 0;
}
extern "C" int exacto_ntt_fwd(exacto_ctx* c, uint64_t* p, size_t count, size_t limb) { return ntt_host(c, p, count, limb, false); }
extern "C" int exacto_ntt_inv(exacto_ctx* c, uint64_t* p, size_t count, size_t limb) { return ntt_host(c, p, count, limb, true); }

static int pw(exacto_ctx* c, PwOp op, const u64* a, const u64* b, u64* out, long polys, const u64* scal) {
    if (int e = check_ctx(c)) return e;
    launch_pointwise(op, a, b, out, polys, c->n, c->L, scal, c->d_primes, c->stream);
    CHECK_LAUNCH();
    return 0;
}

extern "C" int exacto_rns_add_dev(exacto_ctx* c, const uint64_t* a, const uint64_t* b, uint64_t* o, size_t n) {
    return pw(c, PwOp::Add, a, b, o, (long)n * (c ? c->L : 0), nullptr);
}
extern "C" int exacto_rns_sub_dev(exacto_ctx* c, const uint64_t* a, const uint64_t* b, uint64_t* o, size_t n) {
    return pw(c, PwOp::Sub, a, b, o, (long)n * (c ? c->L : 0), nullptr);
}
extern "C" int exacto_rns_neg_dev(exacto_ctx* c, const uint64_t* a, uint64_t* o, size_t n) {
    return pw(c, PwOp::Neg, a, nullptr, o, (long)n * (c ? c->L : 0), nullptr);
}
extern "C" int exacto_rns_mul_dev(exacto_ctx* c, const uint64_t* a, const uint64_t* b, uint64_t* o, size_t n) {
    return pw(c, PwOp::Mul, a, b, o, (long)n * (c ? c->L : 0), nullptr);
}
// INTT(a (.) b): RnsPoly::mul then to_coeff_poly per limb, fused (one pass instead of a
// pointwise pass and an inverse transform); [count][L][n], out may alias a or b.
extern "C" int exacto_rns_mul_inv_dev(exacto_ctx* c, const uint64_t* a, const uint64_t* b, uint64_t* o, size_t count) {
    if (int e = check_ctx(c)) return e;
    if (count == 0) return 0;
    if (!a || !b || !o) return invalid_param("null buffer");
    bool lazy = true, near60 = c->ntt_asm && c->ntt_asm_inv;
    for (int t = 0; t < c->L; ++t) {
        lazy &= c->ctq[t] < (1ull << 60);
        near60 &= c->ctq[t] < (1ull << 60) && c->ctq[t] > (1ull << 60) - (1ull << 24);
    }
    launch_mul_inv(a, b, o, (long)count * c->L, c->L, c->logn, lazy, near60, c->d_primes, c->stream);
    CHECK_LAUNCH();
    return 0;
}
// Negacyclic products of coefficient-domain RnsPolys: to_coeff_poly(from_coeff_poly(a) (.)
// from_coeff_poly(b)) per limb (ntt.rs:181-195 composed).  n = 4096 / 8192 with special primes:
// one fused kernel; otherwise the forward transforms into scratch and the fused product + inverse.
// [count][L][n]; out may alias a or b.
extern "C" int exacto_rns_polymul_dev(exacto_ctx* c, const uint64_t* a, const uint64_t* b, uint64_t* o, size_t count) {
    if (int e = check_ctx(c)) return e;
    if (count == 0) return 0;
    if (!a || !b || !o) return invalid_param("null buffer");
    bool near60 = c->ntt_asm && c->ntt_asm_inv, lazy = true;
    for (int t = 0; t < c->L; ++t) {
        lazy &= c->ctq[t] < (1ull << 60);
        near60 &= c->ctq[t] < (1ull << 60) && c->ctq[t] > (1ull << 60) - (1ull << 24);
    }
    const long rows = (long)count * c->L;
    if (near60 && (c->logn == 12 || c->logn == 13)) {
        // fused product: 3 transforms, algorithmic bytes a + b in, product out
        ProfScope pp(c, PK_POLYMUL, (u64)rows, 24.0 * c->n * (double)rows);
        launch_polymul(a, b, o, rows, c->L, c->logn, c->d_primes, c->stream);
        CHECK_LAUNCH();
        return 0;
    }
    Scratch sa, sb;
    HIP_TRY(sa.alloc((size_t)rows * poly_bytes(c), c->stream, c->pool, c->debug_scratch));
    HIP_TRY(sb.alloc((size_t)rows * poly_bytes(c), c->stream, c->pool, c->debug_scratch));
    NttBatch nb = contiguous(sa.as<u64>(), count, c->L, 0, c->L, c->n);
    nb.src = a;
    if (int e = run_ntt(c, nb, rows, false)) return e;
    nb = contiguous(sb.as<u64>(), count, c->L, 0, c->L, c->n);
    nb.src = b;
    if (int e = run_ntt(c, nb, rows, false)) return e;
    launch_mul_inv(sa.as<u64>(), sb.as<u64>(), o, rows, c->L, c->logn, lazy, false, c->d_primes, c->stream);
    CHECK_LAUNCH();
    return 0;
}

extern "C" int exacto_rns_scalar_mul_dev(exacto_ctx* c, const uint64_t* a, uint64_t scalar, uint64_t* o, size_t n) {
    if (int e = check_ctx(c)) return e;
    // s = scalar % q_i per limb (ntt.rs:136); tiny synchronous upload into the context's table
    u64 sm[EXACTO_MAX_L];
    for (int i = 0; i < c->L; ++i) sm[i] = scalar % c->ctq[i];
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (int e_ = upload(c, c->d_scal, sm, c->L * sizeof(u64))) return e_;
    return pw(c, PwOp::ScalarMul, a, nullptr, o, (long)n * c->L, c->d_scal);
}

// bfv_add / bfv_sub / bfv_neg (eval.rs:14-60), batched: ct1 [B][p1][L][n], ct2 [B][p2][L][n] ->
// out [B][max(p1, p2)][L][n].  Components beyond the shorter operand pass through from the longer
// one, negated when they are ct2's under subtraction (eval.rs:21-22, 41-42).
static int bfv_addsub(exacto_ctx* c, bool sub, const u64* x, size_t p1, const u64* y, size_t p2, u64* o, size_t B) {
    if (int e = check_ctx(c)) return e;
    const size_t pm = std::max(p1, p2);
    if (!B || !pm) return 0;
    if ((p1 && !x) || (p2 && !y) || !o) return invalid_param("null ciphertext pointer");
    // in place only over an operand laid out like the output; any other overlap is rejected
    const size_t pw = (size_t)c->L * c->n;
    auto overlaps = [&](const u64* in, size_t polys) {
        return in && polys && in < o + B * pm * pw && o < in + B * polys * pw;
    };
    if ((overlaps(x, p1) && (o != x || p1 != pm)) || (overlaps(y, p2) && (o != y || p2 != pm)))
        return invalid_param("output may alias an input only when it has as many components as the output");
    launch_bfv_addsub(sub, x, (int)p1, y, (int)p2, o, (long)B, c->n, c->L, c->d_primes, c->stream);
    CHECK_LAUNCH();
    return 0;
}
extern "C" int exacto_bfv_add_dev(exacto_ctx* c, const uint64_t* x, size_t p1, const uint64_t* y, size_t p2, uint64_t* o,
                                  size_t B) {
    return bfv_addsub(c, false, x, p1, y, p2, o, B);
}
extern "C" int exacto_bfv_sub_dev(exacto_ctx* c, const uint64_t* x, size_t p1, const uint64_t* y, size_t p2, uint64_t* o,
                                  size_t B) {
    return bfv_addsub(c, true, x, p1, y, p2, o, B);
}
extern "C" int exacto_bfv_neg_dev(exacto_ctx* c, const uint64_t* x, size_t polys, uint64_t* o, size_t B) {
    if (int e = check_ctx(c)) return e;
    if (!B || !polys) return 0;
    if (!x || !o) return invalid_param("null ciphertext pointer");
    return pw(c, PwOp::Neg, x, nullptr, o, (long)B * polys * c->L, nullptr);
}

// ============================================================== C ABI: BFV

static Operands plain_operands(const exacto_ctx* c, const u64* a, const u64* b) {
    Operands op{};
    op.a = a; op.a_off = nullptr; op.a_stride = 2L * c->L * c->n;
    op.b = b; op.b_off = nullptr; op.b_stride = 2L * c->L * c->n;
    return op;
}

extern "C" int exacto_bfv_mul_no_relin_dev(exacto_ctx* c, const uint64_t* ct1, size_t polys1,
                                           const uint64_t* ct2, size_t polys2, uint64_t* out, size_t B) {
    if (int e = check_ctx(c)) return e;
    if (polys1 != 2 || polys2 != 2) return invalid_param("multiplication requires degree-1 ciphertexts");
    return run_mul(c, plain_operands(c, ct1, ct2), (long)B, out, 3L * c->L * c->n, false);
}

extern "C" int exacto_bfv_mul_and_relin_dev(exacto_ctx* c, const uint64_t* ct1, const uint64_t* ct2,
                                            uint64_t* out, size_t B) {
    if (int e = check_ctx(c)) return e;
    return run_mul(c, plain_operands(c, ct1, ct2), (long)B, out, 2L * c->L * c->n, true);
}

// ct (.) ct on the one-operand pipeline (run_mul square): bit for bit bfv_mul_*(ct, ct).  The checks and
// their order are the two-operand call's; out must not overlap ct (the tensor reads ct after the first
// chunks' results are written).
static int bfv_square_dev(exacto_ctx* c, const u64* ct, u64* out, size_t B, bool relin) {
    if (c->deferred_code) return fail(c->deferred_code, c->deferred_msg);
    if (relin && !c->rlk_loaded) return fail(EXACTO_ERR_MISSING_KEY, "key not available: relinearization key not loaded");
    if (B == 0) return 0;
    if (!ct || !out) return invalid_param("null ciphertext pointer");
    const size_t pw = (size_t)c->L * c->n;
    if (ct < out + B * (relin ? 2 : 3) * pw && out < ct + B * 2 * pw)
        return invalid_param("the output of a square must not overlap its input");
    Operands op = plain_operands(c, ct, nullptr);
    return run_mul(c, op, (long)B, out, (relin ? 2L : 3L) * c->L * c->n, relin, nullptr, true);
}

extern "C" int exacto_bfv_square_no_relin_dev(exacto_ctx* c, const uint64_t* ct, size_t polys, uint64_t* out, size_t B) {
    if (int e = check_ctx(c)) return e;
    if (polys != 2) return invalid_param("multiplication requires degree-1 ciphertexts");
    return bfv_square_dev(c, ct, out, B, false);
}

extern "C" int exacto_bfv_square_and_relin_dev(exacto_ctx* c, const uint64_t* ct, uint64_t* out, size_t B) {
    if (int e = check_ctx(c)) return e;
    return bfv_square_dev(c, ct, out, B, true);
}

extern "C" int exacto_relinearize_dev(exacto_ctx* c, const uint64_t* ct, size_t polys, uint64_t* out, size_t B) {
    if (int e = check_ctx(c)) return e;
    const long Ln = (long)c->L * c->n;
    if (polys < 3) {  // keyswitch.rs:63-65: already degree-1, cloned: out = [B][polys][L][n]
        if (B * polys)
            HIP_TRY(dev_copy(out, ct, B * polys * Ln * sizeof(u64), c->stream));
        return 0;
    }
    if (polys > 3) return invalid_param("relinearization only supports degree-2 ciphertexts");
    if (!c->rlk_loaded) return fail(EXACTO_ERR_MISSING_KEY, "key not available: relinearization key not loaded");
    const int guse = (int)std::min<size_t>(c->G, c->rlk_keys);
    const size_t C = std::min<size_t>(c->chunk, std::max<size_t>(B, 1));
    if (int e = c->ws.ensure(c, C)) return e;
    for (size_t s = 0; s < B; s += C) {
        const int cnt = (int)std::min(C, B - s);
        const u64* src = ct + s * 3 * Ln;
        u64* dst = out + s * 2 * Ln;
        // c0, c1 copied, then accumulated in place
        launch_rows(dst, 2 * Ln, src, 3 * Ln, 2 * Ln, cnt, c->stream);
        CHECK_LAUNCH();
        if (guse == 0) continue;
        NttBatch nb{};
        nb.src = src + 2 * Ln; nb.src_off = nullptr; nb.src_item_stride = 3 * Ln;
        nb.dst = c->ws.coefQ; nb.dst_item_stride = Ln;
        nb.ppi = c->L; nb.prime_base = 0; nb.period = c->L;
        if (int e = run_ntt(c, nb, (long)cnt * c->L, true)) return e;
        const bool d16 = c->digit16 && c->gbase <= 65536;  // int16 digits, as in run_mul
        launch_decompose(c->ws.coefQ, Ln, c->ws.D, guse, cnt, c->n, c->d_crt, c->d_primes, c->L, c->stream,
                         d16 ? c->ws.D16 : nullptr);
        CHECK_LAUNCH();
        NttBatch db = contiguous(c->ws.D, cnt, (long)guse * c->L, 0, c->L, c->n);
        if (d16) {
            db.src16 = c->ws.D16;
            db.src16_item_stride = (long)guse * c->n;
        }
        if (int e = run_ntt(c, db, (long)cnt * guse * c->L, false)) return e;
        if (int e = ensure_rlk_companions(c)) return e;
        launch_relin_mac(dst, 2 * Ln, c->ws.D, c->d_rlk, c->d_rlk_s, guse, dst, 2 * Ln, cnt, c->n, c->L,
                         c->d_primes, c->stream);
        CHECK_LAUNCH();
    }
    return 0;
}

extern "C" int exacto_gadget_decompose_dev(exacto_ctx* c, const uint64_t* coeffs, uint64_t* digits, size_t B,
                                           size_t num_digits) {
    if (int e = check_ctx(c)) return e;
    const int guse = (int)std::min<size_t>(c->G, num_digits);
    launch_decompose(coeffs, (long)c->L * c->n, digits, guse, (int)B, c->n, c->d_crt, c->d_primes, c->L, c->stream);
    CHECK_LAUNCH();
    return 0;
}

// host-pointer wrappers: stage inputs in the context's io buffer, run the _dev entry, copy back
int exacto::host_call(exacto_ctx* c, const std::vector<std::pair<const void*, size_t>>& ins, size_t out_bytes,
                      void* host_out, const std::function<int(std::vector<u64*>&, u64*)>& fn) {
    if (int e = check_ctx(c)) return e;
    size_t total = out_bytes;
    for (auto& in : ins) total += (in.second + 255) / 256 * 256;
    if (int e = stage(c, total)) return e;
    std::vector<u64*> dins;
    char* p = (char*)c->io.get();
    for (auto& in : ins) {
        // stream-ordered on the context stream (see upload)
        if (in.second) HIP_TRY(hipMemcpyAsync(p, in.first, in.second, hipMemcpyHostToDevice, c->stream));
        dins.push_back((u64*)p);
        p += (in.second + 255) / 256 * 256;
    }
    // landed before fn runs: fn may read the inputs on another context's stream (bootstrap)
    HIP_TRY(hipStreamSynchronize(c->stream));
    u64* dout = (u64*)p;
    if (int e = fn(dins, dout)) return e;
    HIP_TRY(hipMemcpyAsync(host_out, dout, out_bytes, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    static const bool dbg = [] { const char* e = getenv("EXACTO_DEBUG_BOOT"); return e && e[0] == '1'; }();
    if (dbg && host_out && out_bytes >= 8 && out_bytes <= 64 * 8) {   // (the bootstrap diagnostic: what the host received)
        u64 hsh = 1469598103934665603ull;
        const u64* ho = static_cast<const u64*>(host_out);
        for (size_t k = 0; k < out_bytes / 8; ++k) hsh = (hsh ^ ho[k]) * 1099511628211ull;
        std::fprintf(stderr, "boot-dbg host_out       %016llx [%llu %llu %llu %llu]\n", (unsigned long long)hsh,
                     (unsigned long long)ho[0], (unsigned long long)(out_bytes > 8 ? ho[1] : 0),
                     (unsigned long long)(out_bytes > 16 ? ho[2] : 0), (unsigned long long)(out_bytes > 24 ? ho[3] : 0));
    }
    return 0;
}

extern "C" int exacto_bfv_mul_no_relin(exacto_ctx* c, const uint64_t* ct1, size_t p1, const uint64_t* ct2, size_t p2,
                                       uint64_t* out, size_t B) {
    if (!c) return invalid_param("null context");
    const size_t ctb = B * 2 * c->L * poly_bytes(c);
    return host_call(c, {{ct1, ctb}, {ct2, ctb}}, B * 3 * c->L * poly_bytes(c), out,
                     [&](std::vector<u64*>& d, u64* o) { return exacto_bfv_mul_no_relin_dev(c, d[0], p1, d[1], p2, o, B); });
}

extern "C" int exacto_bfv_mul_and_relin(exacto_ctx* c, const uint64_t* ct1, const uint64_t* ct2, uint64_t* out,
                                        size_t B) {
    if (!c) return invalid_param("null context");
    const size_t ctb = B * 2 * c->L * poly_bytes(c);
    return host_call(c, {{ct1, ctb}, {ct2, ctb}}, ctb, out,
                     [&](std::vector<u64*>& d, u64* o) { return exacto_bfv_mul_and_relin_dev(c, d[0], d[1], o, B); });
}

extern "C" int exacto_bfv_square_no_relin(exacto_ctx* c, const uint64_t* ct, size_t polys, uint64_t* out, size_t B) {
    if (!c) return invalid_param("null context");
    const size_t ctb = B * 2 * c->L * poly_bytes(c);
    return host_call(c, {{ct, ctb}}, B * 3 * c->L * poly_bytes(c), out,
                     [&](std::vector<u64*>& d, u64* o) { return exacto_bfv_square_no_relin_dev(c, d[0], polys, o, B); });
}

extern "C" int exacto_bfv_square_and_relin(exacto_ctx* c, const uint64_t* ct, uint64_t* out, size_t B) {
    if (!c) return invalid_param("null context");
    const size_t ctb = B * 2 * c->L * poly_bytes(c);
    return host_call(c, {{ct, ctb}}, ctb, out,
                     [&](std::vector<u64*>& d, u64* o) { return exacto_bfv_square_and_relin_dev(c, d[0], o, B); });
}

extern "C" int exacto_relinearize(exacto_ctx* c, const uint64_t* ct, size_t polys, uint64_t* out, size_t B) {
    if (!c) return invalid_param("null context");
    const size_t inb = B * polys * c->L * poly_bytes(c);
    const size_t outp = polys < 3 ? polys : 2;
    return host_call(c, {{ct, inb}}, B * outp * c->L * poly_bytes(c), out,
                     [&](std::vector<u64*>& d, u64* o) { return exacto_relinearize_dev(c, d[0], polys, o, B); });
}

// ============================================================== C ABI: dBFV

// lattice.rs:104-122 compute_simple + decomposition.rs:8-16 digit_decompose
extern "C" int exacto_bfv_add(exacto_ctx* c, const uint64_t* ct1, size_t p1, const uint64_t* ct2, size_t p2,
                              uint64_t* out, size_t B) {
    if (!c) return invalid_param("null context");
    const size_t pb = c->L * poly_bytes(c);
    return host_call(c, {{ct1, B * p1 * pb}, {ct2, B * p2 * pb}}, B * std::max(p1, p2) * pb, out,
                     [&](std::vector<u64*>& in, u64* o) { return exacto_bfv_add_dev(c, in[0], p1, in[1], p2, o, B); });
}
extern "C" int exacto_bfv_sub(exacto_ctx* c, const uint64_t* ct1, size_t p1, const uint64_t* ct2, size_t p2,
                              uint64_t* out, size_t B) {
    if (!c) return invalid_param("null context");
    const size_t pb = c->L * poly_bytes(c);
    return host_call(c, {{ct1, B * p1 * pb}, {ct2, B * p2 * pb}}, B * std::max(p1, p2) * pb, out,
                     [&](std::vector<u64*>& in, u64* o) { return exacto_bfv_sub_dev(c, in[0], p1, in[1], p2, o, B); });
}
extern "C" int exacto_bfv_neg(exacto_ctx* c, const uint64_t* ct, size_t polys, uint64_t* out, size_t B) {
    if (!c) return invalid_param("null context");
    const size_t bytes = B * polys * c->L * poly_bytes(c);
    return host_call(c, {{ct, bytes}}, bytes, out,
                     [&](std::vector<u64*>& in, u64* o) { return exacto_bfv_neg_dev(c, in[0], polys, o, B); });
}

static std::vector<std::vector<i64>> small_reps(u64 base, size_t d, u64 p) {
    std::vector<std::vector<i64>> reps;
    for (size_t j = d; j + 1 < 2 * d; ++j) {
        u64 val;
        if (p == 0) {
            val = 1;
            for (size_t e = 0; e < j; ++e) val *= base;  // wrapping_pow
        } else {
            val = powmod_h(base, j, p);
        }
        std::vector<i64> dg;
        u64 rem = val;
        for (size_t k = 0; k < d; ++k) { dg.push_back((i64)(rem % base)); rem /= base; }
        reps.push_back(dg);
    }
    return reps;
}

// Uploads a product-sum plan: `pairs` = the (left, right) operand indices of the npairs products of one
// item (left in [0, na), right in [0, nb)), and for each of the dout outputs the products it sums
// (terms [start[s], start[s + 1]), CombineTerm::pair indexing `pairs`).  dbfv_mul's index rule
// (dbfv_plan) and bfv_mul_sum's term lists (mul_sum_plan) are its two producers; the caller sets the
// cache key.  d_off: [0, BP): a offsets, [BP, 2BP): b offsets (ciphertexts), [2BP, 4BP): the same
// into the per-ciphertext extension buffers (ext_a = [B na], ext_b = [B nb] ciphertexts).
static int plan_upload(exacto_ctx* c, size_t B, size_t na, size_t nb, const std::vector<std::pair<int, int>>& pairs,
                       const std::vector<int>& start, const std::vector<CombineTerm>& terms) {
    c->cached_kind = -1;   // (a failed upload leaves no plan)
    const int npairs = (int)pairs.size();
    const size_t dout = start.size() - 1;
    // ks32 sums before the lift: every combine term a plain sum (zero reps), at most this many per limb
    int sum_m = 0;
    for (const CombineTerm& t : terms) if (t.coef != 1) sum_m = -1;
    for (size_t so = 0; so < dout && sum_m >= 0; ++so) sum_m = std::max(sum_m, start[so + 1] - start[so]);
    const long Ln2 = 2L * c->L * c->n, Kn2 = 2L * c->K * c->n;
    const size_t BP = B * npairs;
    std::vector<u64> off(4 * BP);
    for (size_t b = 0; b < B; ++b)
        for (int pi = 0; pi < npairs; ++pi) {
            off[b * npairs + pi] = (u64)((b * na + pairs[pi].first) * Ln2);
            off[BP + b * npairs + pi] = (u64)((b * nb + pairs[pi].second) * Ln2);
            off[2 * BP + b * npairs + pi] = (u64)((b * na + pairs[pi].first) * Kn2);
            off[3 * BP + b * npairs + pi] = (u64)((b * nb + pairs[pi].second) * Kn2);
        }
    if (c->d_off.grow(off.size() * sizeof(u64) + 8)) return EXACTO_ERR_HIP;
    if (int e_ = upload(c, c->d_off, off.data(), off.size() * sizeof(u64))) return e_;
    c->d_term_start.reset();
    c->d_terms.reset();
    if (int e_ = c->d_term_start.alloc(start.size() * sizeof(int))) return e_;
    if (int e_ = upload(c, c->d_term_start, start.data(), start.size() * sizeof(int))) return e_;
    if (int e_ = c->d_terms.alloc(std::max<size_t>(terms.size(), 1) * sizeof(CombineTerm))) return e_;
    if (!terms.empty())
        if (int e_ = upload(c, c->d_terms, terms.data(), terms.size() * sizeof(CombineTerm))) return e_;
    c->cached_B = B;
    c->cached_npairs = npairs;
    c->cached_sum_m = sum_m;
    return 0;
}

// The product list and combine terms of a dbfv_mul batch (dbfv/eval.rs:109-132 + reduce,
// reduction.rs:34-52) for the output limbs `limbs` (all of 0..d-1, or the subset one GPU computes
// when the limbs of one dbfv_mul are split across GPUs): output slot s = limb limbs[s] gets the sum
// over pairs (i, j) with i + j == limbs[s] plus the reps folding of the high limbs i + j >= d.  Only
// the pairs some listed limb uses are multiplied.
// sym (dbfv_square: both operands are the same d ciphertexts, so products (i, j) and (j, i) are one
// ciphertext): only the pairs i <= j are multiplied, and every limb's term list is the one above with
// (j, i) replaced by the index of (i, j) -- a product shared by two ordered pairs is listed twice, term for
// term in the same order and with the same coefficients, so the terms per limb (cached_sum_m, the
// psum / ks32 bounds) and with them the key-switch mode are those of dbfv_mul(a, a).
static void dbfv_plan_build(size_t d, u64 base, u64 plain, const std::vector<int>& limbs, bool sym,
                            std::vector<std::pair<int, int>>& pairs, std::vector<int>& start,
                            std::vector<CombineTerm>& terms) {
    const auto reps = small_reps(base, d, plain);
    const size_t dout = limbs.size();
    auto coef_of = [&](size_t i, size_t j, size_t ko) -> i64 {
        const size_t k = i + j;
        return k == ko ? 1 : k >= d ? reps[k - d][ko] : 0;
    };
    // the ordered pairs some listed limb needs, and the product each reads
    std::vector<std::pair<int, int>> ordered;
    std::vector<int> index;
    std::vector<int> of(d * d, -1);
    pairs.clear();
    for (size_t i = 0; i < d; ++i)
        for (size_t j = 0; j < d; ++j) {
            bool needed = false;
            for (int ko : limbs) needed |= coef_of(i, j, (size_t)ko) != 0;
            if (!needed) continue;
            const size_t lo = sym ? std::min(i, j) : i, hi = sym ? std::max(i, j) : j;
            if (of[lo * d + hi] < 0) {   // (sym: (lo, hi) comes first in this order, lo <= hi)
                of[lo * d + hi] = (int)pairs.size();
                pairs.push_back({(int)lo, (int)hi});
            }
            ordered.push_back({(int)i, (int)j});
            index.push_back(of[lo * d + hi]);
        }
    start.assign(dout + 1, 0);
    terms.clear();
    for (size_t so = 0; so < dout; ++so) {
        start[so] = (int)terms.size();
        for (size_t oi = 0; oi < ordered.size(); ++oi) {
            const i64 coef = coef_of(ordered[oi].first, ordered[oi].second, (size_t)limbs[so]);
            if (coef != 0) terms.push_back({index[oi], 0, coef});
        }
    }
    start[dout] = (int)terms.size();
}

static int dbfv_plan(exacto_ctx* c, size_t B, size_t d, u64 base, u64 plain, const std::vector<int>& limbs,
                     bool sym = false) {
    if (c->cached_kind == (sym ? 2 : 0) && c->cached_B == B && c->cached_d == d && c->cached_base == base && c->cached_p == plain &&
        c->d_off && c->cached_limbs == limbs)
        return 0;
    std::vector<std::pair<int, int>> pairs;
    std::vector<int> start;
    std::vector<CombineTerm> terms;
    dbfv_plan_build(d, base, plain, limbs, sym, pairs, start, terms);
    if (int e = plan_upload(c, B, d, d, pairs, start, terms)) return e;
    c->cached_kind = sym ? 2 : 0;
    c->cached_d = d; c->cached_base = base; c->cached_p = plain;
    c->cached_limbs = limbs;
    return 0;
}

// The plan of a bfv_mul_sum: product t = (ia[t], ib[t]) (a pair listed twice is two products: it counts
// twice), the terms of each output slot in groups of at most `gcap` products (0: one group per slot),
// groups ordered by slot.  Each group is one "output limb" of the pass; slot_start (uploaded when a
// slot has several groups) lists each slot's groups for the group sum.
static int mul_sum_plan(exacto_ctx* c, size_t B, size_t na, size_t nb, const uint32_t* ia, const uint32_t* ib,
                        const uint32_t* slot, size_t nterms, size_t nslots, size_t gcap) {
    std::vector<uint32_t> key;
    key.reserve(3 * nterms + 4);
    key.insert(key.end(), ia, ia + nterms);
    key.insert(key.end(), ib, ib + nterms);
    key.insert(key.end(), slot, slot + nterms);
    for (size_t v : {na, nb, nslots, gcap}) key.push_back((uint32_t)std::min<size_t>(v, 0xffffffffu));
    if (c->cached_kind == 1 && c->cached_B == B && c->d_off && c->cached_ms == key) return 0;
    std::vector<std::pair<int, int>> pairs(nterms);
    for (size_t t = 0; t < nterms; ++t) pairs[t] = {(int)ia[t], (int)ib[t]};
    std::vector<int> start{0}, slot_start{0};
    std::vector<CombineTerm> terms;
    for (size_t s = 0; s < nslots; ++s) {
        size_t in_group = 0;
        for (size_t t = 0; t < nterms; ++t) {
            if (slot[t] != s) continue;
            if (gcap && in_group == gcap) {
                start.push_back((int)terms.size());
                in_group = 0;
            }
            terms.push_back({(int)t, 0, 1});
            ++in_group;
        }
        start.push_back((int)terms.size());
        slot_start.push_back((int)start.size() - 1);
    }
    if (int e = plan_upload(c, B, na, nb, pairs, start, terms)) return e;
    const size_t ngroups = start.size() - 1;
    if (ngroups > nslots) {
        if (int e_ = c->d_slot_start.alloc(slot_start.size() * sizeof(int))) return e_;
        if (int e_ = upload(c, c->d_slot_start, slot_start.data(), slot_start.size() * sizeof(int))) return e_;
    }
    c->cached_kind = 1;
    c->cached_ms = key;
    c->cached_ngroups = (int)ngroups;
    return 0;
}

// DbfvParams::new checks (params/mod.rs:168-184)
int exacto::dbfv_params_check(size_t d, uint64_t base, uint64_t plain) {
    if (base < 2) return invalid_param("base must be >= 2");
    if (d < 1) return invalid_param("num_digits must be >= 1");
    u128 bd = 1;
    const u128 sat = ~(u128)0;
    for (size_t i = 0; i < d; ++i) bd = (bd > sat / base) ? sat : bd * base;
    const u128 p128 = plain == 0 ? ((u128)1 << 64) : (u128)plain;
    if (bd < p128) {
        auto u128s = [](u128 v) { std::string s; do { s.insert(s.begin(), char('0' + (int)(v % 10))); v /= 10; } while (v); return s; };
        return invalid_param("base^digits = " + u128s(bd) + " < plain_modulus = " + u128s(p128));
    }
    return 0;
}

// The plan dbfv_mul (symmetric = 0) or dbfv_square (1) runs for all d output limbs, pure host code.
extern "C" int exacto_dbfv_mul_plan(size_t d, uint64_t base, uint64_t plain, int symmetric, int32_t* pairs,
                                    size_t pair_cap, size_t* npairs, int32_t* term_start, int64_t* terms,
                                    size_t term_cap, size_t* nterms) {
    if (int e = dbfv_params_check(d, base, plain)) return e;
    if (!npairs || !nterms) return invalid_param("null count pointer");
    std::vector<int> limbs;
    for (size_t k = 0; k < d; ++k) limbs.push_back((int)k);
    std::vector<std::pair<int, int>> pr;
    std::vector<int> start;
    std::vector<CombineTerm> tm;
    dbfv_plan_build(d, base, plain, limbs, symmetric != 0, pr, start, tm);
    *npairs = pr.size();
    *nterms = tm.size();
    if (pairs && pair_cap >= pr.size())
        for (size_t i = 0; i < pr.size(); ++i) { pairs[2 * i] = pr[i].first; pairs[2 * i + 1] = pr[i].second; }
    if (term_start)
        for (size_t k = 0; k <= d; ++k) term_start[k] = start[k];
    if (terms && term_cap >= tm.size())
        for (size_t i = 0; i < tm.size(); ++i) { terms[2 * i] = tm[i].pair; terms[2 * i + 1] = tm[i].coef; }
    return 0;
}

// Every input ciphertext of a dBFV product batch enters d products (dbfv/eval.rs:109-122): its
// inverse NTT, its exact (or HPS) extension to the auxiliary primes and their forward NTT
// (pipeline steps 1-3) are computed here once per ciphertext, ext = [ct][2][K][n], instead of
// once per product.  The results are identical: steps 1-3 depend on the ciphertext alone.
// coef: the same ciphertexts already in the coefficient domain (a dBFV chain's previous step,
// [ct][2][L][n]), or nullptr: the inverse NTT is skipped and the lift reads them directly.
static int extend_cts(exacto_ctx* c, const u64* cts, size_t ncts, u64* ext, const u64* coef = nullptr) {
    const int n = c->n, L = c->L, K = c->K;
    const long Ln2 = 2L * L * n, Kn2 = 2L * K * n;
    if (int e = c->ws.ensure(c, std::min<size_t>(c->chunk, (ncts + 1) / 2))) return e;
    const size_t G = coef ? ncts : 2 * c->ws.items;  // ciphertexts per pass: coefQ holds 4 polys x L per item
    for (size_t g0 = 0; g0 < ncts; g0 += G) {
        const long cnt = (long)std::min(G, ncts - g0);
        const u64* cq = coef ? coef + g0 * Ln2 : c->ws.coefQ;
        if (!coef) {
            NttBatch nb{};
            nb.src = cts + g0 * Ln2; nb.src_off = nullptr; nb.src_item_stride = Ln2;
            nb.dst = c->ws.coefQ; nb.dst_item_stride = Ln2;
            nb.ppi = 2 * L; nb.prime_base = 0; nb.period = L;
            if (int e = run_ntt(c, nb, cnt * 2 * L, true)) return e;
        }
        u64* eo = ext + g0 * Kn2;
        if (c->path == EXACTO_PATH_HPS) {
            ProfScope pl(c, PK_HPS_EXT, 2ull * cnt, 8.0 * (1 + K) * n * 2.0 * cnt);
            launch_hps_extend(cq, eo, 2 * cnt, n, c->d_primes, K, c->stream);
        } else {
            ProfScope pl(c, PK_LIFT, 2ull * cnt, 8.0 * (L + K) * n * 2.0 * cnt);
            launch_exact_lift(cq, eo, 2 * cnt, n, c->d_crt, c->d_primes, L, K,
                              crt_mode(c), c->stream);
        }
        CHECK_LAUNCH();
        if (int e = run_ntt(c, contiguous(eo, cnt, 2L * K, L, K, n), cnt * 2 * K, false)) return e;
    }
    return 0;
}

// One pass over the resident plan (plan_upload): a = [B][na][2][L][n], b = [B][nb][2][L][n], the plan's
// dout outputs per item, each the sum of its products, relinearised.
// b_extended: c->ext_b already holds the extensions of b (a chain's constant right operand)
// nslots == dout (dbfv_mul: the outputs are the limbs): out = [B][dout][2][L][n].  nslots < dout
// (bfv_mul_sum with more products per slot than one key switch lifts): the dout outputs are groups,
// formed in gsum_buf and added per slot (mul_sum_plan's slot_start) before the forward transform of
// out = [B][nslots][2][L][n].  *mode: the key switch taken, exacto_ctx_info.dbfv_key_switch's codes.
// same_ab (the symmetric plan, b == a and nb == na): the extensions are made once, ext_b is ext_a.
static int mul_group_run(exacto_ctx* c, size_t na, size_t nb, const uint64_t* a, const uint64_t* b, uint64_t* out,
                         size_t B, bool b_extended, size_t dout, size_t nslots, int* mode, bool same_ab = false) {
    const int npairs = c->cached_npairs;
    const bool grouped = nslots < dout;
    const long Ln2 = 2L * c->L * c->n;
    const long P = (long)B * npairs;
    if (c->prod.grow((size_t)P * Ln2 * sizeof(u64))) return EXACTO_ERR_HIP;
    Operands op{};
    const size_t BP = (size_t)B * npairs;
    op.a = a; op.a_off = c->d_off; op.a_stride = 0;
    op.b = b; op.b_off = c->d_off + BP; op.b_stride = 0;
    if (c->share_ext && c->K > 0 && !c->deferred_code) {
        const size_t bytes_a = B * na * 2 * c->K * poly_bytes(c), bytes_b = B * nb * 2 * c->K * poly_bytes(c);
        if (c->ext_a_ready) {   // made by the previous chain step (same ciphertexts, same buffer size)
            if (c->ext_a.bytes() < bytes_a) return fail(EXACTO_ERR_HIP, "internal: pre-extended operand buffer too small");
        } else {
            if (c->ext_a.grow(bytes_a)) return EXACTO_ERR_HIP;
            if (int e = extend_cts(c, a, B * na, c->ext_a, c->coef_in)) return e;
        }
        c->ext_a_ready = false;
        if (!b_extended && !same_ab) {
            if (c->ext_b.grow(bytes_b)) return EXACTO_ERR_HIP;
            if (int e = extend_cts(c, b, B * nb, c->ext_b)) return e;
        }
        op.ea = c->ext_a; op.ea_off = c->d_off + 2 * BP;
        op.eb = same_ab ? c->ext_a : c->ext_b; op.eb_off = c->d_off + 3 * BP;
    }
    // the per-limb sums (dbfv/eval.rs:124-132) and the degree reduction are linear, so with ks32 they
    // run on the products' coefficient-domain results and only the d output limbs are transformed
    // (B d 2L forward NTTs instead of B npairs 2L)
    // ... and when the 31-bit basis holds the sum of a limb's key switches, the key switch is
    // linear in the digits, so the products' int16 digits are summed per output limb (still int16)
    // and transformed, multiplied with the key and lifted once per limb instead of once per product
    // (cfg5: 8 instead of 36 products' worth of digit NTTs, MACs and lifts per dbfv_mul)
    // The primary 31-bit basis when it holds the sums, else the wide one (primes up to 2^31).
    const size_t gu = std::min<size_t>(c->G, c->rlk_keys);
    const int m = c->cached_sum_m;
    // the primary basis (narrow or lazy) and its sum_max depend on the resident key: decide first
    if (m > c->ks32_need_m) {
        c->ks32_need_m = m;
        // a key already on the lazy basis that cannot lift these sums while the narrow one can: re-select
        if (c->rs_valid && c->ks32_lazy_active && m > c->ks32_sum_max) c->rs_valid = false;
    }
    if (c->S32 > 0 && c->ks32 && c->rlk_loaded && gu > 0)
        if (int e = ensure_rs(c)) return e;
    const bool on = c->S32 > 0 && c->ks32 && m > 0 && c->digit16 && c->gbase <= 65536 &&
                    c->rlk_loaded && gu > 0;
    const bool use_prim = on && m <= c->ks32_sum_max;
    const bool use_wide = on && !use_prim && c->kw.S > 0 && m <= c->kw.sum_max;
    const bool sum_ks = use_prim || use_wide;
    *mode = use_prim ? 1 : use_wide ? 2 : 0;
    const int S = use_wide ? c->kw.S : c->S32;
    const Prime32* p32 = use_wide ? c->kw.d_p32 : c->d_p32;
    const Ks32Tables* kst = use_wide ? c->kw.d_kst : c->d_kst;
    const int mac_form = use_wide ? c->kw.mac_form : c->ks32_mac_form;
    const bool wide = (u64)m * digit_max(c->gbase) > 32767;   // digit sums beyond int16
    const size_t Bd = B * dout, Sn = (size_t)S * c->n;
    // HPS (u64_dbfv): with the products' c0 / c1 kept in the coefficient domain, relinearize is linear
    // mod q in the gadget digits and so are the per-limb sums and the NTT: limb k = NTT(sum c0) +
    // sum_g NTT(sum_p d_pg) (.) rlk_g.  The scale writes every product's signed digits (int8 when the
    // base is at most 2^8), ks32_digit_sum adds them per output limb as int16 (|sum| <= m ceil(B/2)), and
    // the forward NTTs and the MAC run once per output limb instead of once per product (u64_dbfv:
    // 8 instead of 36 products' worth of 10 forward NTTs and one MAC per dbfv_mul).
    const bool hps_sum = c->path == EXACTO_PATH_HPS && c->hps_sum_env && m > 0 && c->gbase <= 65536 &&
                         (u64)m * digit_max(c->gbase) <= 32767 && c->rlk_loaded && gu > 0 && c->n >= 1024 &&
                         !c->deferred_code;
    if (grouped) {
        // (the HPS sum multiplies with the key after the forward transform, once per output: never grouped)
        if (hps_sum) return fail(EXACTO_ERR_HIP, "internal: grouped product sums on the HPS digit-sum path");
        if (c->gsum_buf.grow(B * dout * (size_t)Ln2 * sizeof(u64))) return EXACTO_ERR_HIP;
    }
    if (hps_sum) {
        if (c->d_dall.grow((size_t)P * gu * c->n * sizeof(int16_t)) || c->d_dk.grow(Bd * gu * c->n * 2) ||
            c->d_hdig.grow(Bd * gu * c->L * c->n * sizeof(u64)))
            return EXACTO_ERR_HIP;
        if (int e = ensure_rlk_companions(c)) return e;
        c->ks_defer = c->d_dall;
        c->ks_defer8 = c->digit8_env && c->gbase <= 256;
    }
    if (sum_ks) {
        if (c->d_dall.grow((size_t)P * gu * c->n * sizeof(int16_t)) || c->d_dk.grow(Bd * gu * c->n * (wide ? 4 : 2)) ||
            c->d_dsk.grow(Bd * gu * Sn * sizeof(uint32_t)) || c->d_uk.grow(Bd * 2 * c->L * Sn * sizeof(uint32_t)))
            return EXACTO_ERR_HIP;
        if (int e = use_wide ? ensure_rs_wide(c) : ensure_rs(c)) return e;
        c->ks_defer = c->d_dall;
        // base <= 2^8: every balanced digit fits int8 (half the digit bytes written and summed)
        const int sh = c->h_crt.gshift;
        c->ks_defer8 = c->digit8_env && sh > 0 && sh <= 8 && 32 % sh == 0 &&
                       exact_scale_sp_ok(c->L, c->K, crt_mode(c));
    }
    // psum: each output limb's c0 / c1 from one scale of its products' summed tensors (the
    // auxiliary-prime residues summed in the NTT domain and inverse-transformed once per limb, the
    // per-product corrections from the ciphertext-prime residues; exact_psum_sp_kernel), written
    // straight to out: no per-product c0 / c1 and no dbfv_combine pass.  Needs the summed digits
    // (so the third component is per product only for its digits), shared extensions, special
    // primes with K = L + 1 (30-bit-limb scale) and the asm tensor kernels.
    bool near60 = c->ntt_asm && c->ntt_asm_inv;
    for (u64 q : c->primes) near60 &= q < (1ull << 60) && q > (1ull << 60) - (1ull << 24);
    const bool psum = sum_ks && c->psum_env && m <= c->psum_max && op.ea != nullptr && near60 &&
                      (c->logn == 12 || c->logn == 13) && exact_scale_sp_ok(c->L, c->K, crt_mode(c));
    // chain (psum): the limbs are formed in the coefficient domain in coef_out and forward-transformed
    // from there into out, so coef_out keeps them for the next step's extension.  The buffer is grown
    // only here, where psum is known to be on (HPS or non-psum chains never allocate it).
    c->coef_out = nullptr;
    if (psum && c->coef_slot >= 0) {
        if (c->chain_coef.grow(2 * c->coef_slot_words * sizeof(u64))) return EXACTO_ERR_HIP;
        c->coef_out = c->chain_coef + (size_t)c->coef_slot * c->coef_slot_words;
    }
    const bool chain_cf = psum && c->coef_out;
    u64* cf = chain_cf ? c->coef_out : grouped ? c->gsum_buf : out;
    c->coef_written = false;
    if (psum) {
        c->psum.on = true;
        c->psum.d = (int)dout;
        c->psum.npairs = npairs;
        c->psum.term_start = c->d_term_start;
        c->psum.terms = c->d_terms;
        c->psum.out = cf;
        c->psum.fpc = c->fp_crt && m <= c->psum_fp_max;
    }
    bool coef = false;
    if (op.ea) {
        // (distinct ciphertexts per item / 2; a square's d count as 2 ceil(d / 2) in the byte estimate)
        c->tensor_share_d = (int)(((same_ab ? na : na + nb) + 1) / 2);
        c->tensor_share_npairs = npairs;
    }
    const int rc = run_mul(c, op, P, c->prod, Ln2, true, &coef);
    c->tensor_share_d = c->tensor_share_npairs = 0;
    c->ks_defer = nullptr;
    const bool in8 = c->ks_defer8;
    c->ks_defer8 = false;
    c->psum.on = false;
    if (rc) return rc;
    if ((sum_ks || hps_sum) && !coef) return fail(EXACTO_ERR_HIP, "internal: digit sums without a deferred key switch");
    if (!psum) {
        ProfScope pk(c, PK_COMBINE, (u64)B * dout, 8.0 * c->n * B * 2 * c->L * (double)(npairs + dout));
        launch_dbfv_combine(c->prod, npairs, c->d_term_start, c->d_terms, cf, (int)B, (int)dout, c->n, c->L,
                            c->d_primes, c->stream);
        CHECK_LAUNCH();
    }
    if (sum_ks) {
        const double nn = c->n, ds = wide ? 4.0 : 2.0;
        {   // every product's digits in (1 or 2 B), one sum per (limb, digit) out
            ProfScope pd(c, PK_DIGIT_SUM, (u64)Bd, nn * gu * ((double)B * npairs * (in8 ? 1.0 : 2.0) + (double)Bd * ds));
            ks32_digit_sum(c->d_dall, in8, npairs, c->d_term_start, c->d_terms, c->d_dk, wide, (int)B, (int)dout, (int)gu,
                           c->n, c->stream);
        }
        {
            ProfScope pn(c, PK_KS_DIGITS, (u64)Bd * gu * S, nn * Bd * gu * S * (ds + 4.0));
            if (wide) ks32_digits32((const int32_t*)c->d_dk.get(), c->d_dsk, (int)Bd, (int)gu, S, c->logn, p32, mac_form, c->stream);
            else ks32_digits((const int16_t*)c->d_dk.get(), c->d_dsk, (int)Bd, (int)gu, S, c->logn, p32, mac_form, c->stream);
        }
        {
            ProfScope pm(c, PK_KS_MAC, (u64)Bd * S, 4.0 * nn * Bd * S * (gu + 2.0 * c->L));
            ks32_mac(c->d_dsk, use_wide ? c->kw.d_rs : c->d_rs, c->d_uk, (int)Bd, (int)gu, c->L, S, c->n, p32,
                     mac_form, c->stream);
        }
        {
            ProfScope pc(c, PK_KS_CRT, (u64)Bd * 2 * c->L, nn * Bd * 2 * c->L * (4.0 * S + 16.0));
            const bool fpc = c->ks_fpc && m <= (use_wide ? c->kw.fpc_max : c->ks32_fpc_max);
            ks32_crt(c->d_uk, cf, 2L * c->L * c->n, (int)Bd, c->L, S, c->logn, kst, p32, c->d_primes, mac_form, c->stream,
                     fpc);
        }
        CHECK_LAUNCH();
    }
    if (hps_sum) {
        const double nn = c->n;
        {   // every product's digits in (1 or 2 B), one int16 sum per (limb, digit) out
            ProfScope pd(c, PK_DIGIT_SUM, (u64)Bd, nn * gu * ((double)B * npairs * (in8 ? 1.0 : 2.0) + 2.0 * Bd));
            ks32_digit_sum(c->d_dall, in8, npairs, c->d_term_start, c->d_terms, c->d_dk, false, (int)B, (int)dout,
                           (int)gu, c->n, c->stream);
        }
        CHECK_LAUNCH();
        NttBatch db = contiguous(c->d_hdig, (long)Bd, (long)gu * c->L, 0, c->L, c->n);
        db.src16 = (const int16_t*)c->d_dk.get();
        db.src16_item_stride = (long)gu * c->n;
        if (int e = run_ntt(c, db, (long)Bd * gu * c->L, false)) return e;
    }
    if (grouped) {
        // each slot's groups added mod q_l (relinearised already, coefficient domain when `coef`): the
        // forward transform below then runs once per slot, not once per group
        ProfScope pg(c, PK_GROUP_SUM, (u64)B * nslots, 8.0 * c->n * B * 2 * c->L * (double)(dout + nslots));
        launch_group_sum(cf, out, c->d_slot_start, (int)dout, (int)nslots, (long)B, c->n, c->L, c->d_primes, c->stream);
        CHECK_LAUNCH();
        cf = out;
    }
    if (coef) {
        NttBatch ob = contiguous(out, (long)B * nslots, 2L * c->L, 0, c->L, c->n);
        ob.src = cf;   // (== out unless a chain keeps the coefficient form)
        // a chain step whose limbs stay in the coefficient domain (cf) for the next step: that step's
        // extension of its left operand (exact lift of cf to the auxiliary primes, then their forward
        // transform: extend_cts with coef = cf) is made here, and the two forward batches go in one
        // launch (cfg5: 512 + 640 polynomials instead of two launches that each fill about one
        // generation of the 512 resident workgroups)
        const bool pre = chain_cf && op.ea != nullptr && dout == na && na == nb && !c->deferred_code &&
                         c->path != EXACTO_PATH_HPS && c->ext_a.bytes() >= (size_t)B * na * 2 * c->K * poly_bytes(c);
        if (pre) {
            const long cts = (long)B * na;
            {
                ProfScope pl(c, PK_LIFT, 2ull * cts, 8.0 * (c->L + c->K) * c->n * 2.0 * cts);
                launch_exact_lift(cf, c->ext_a, 2 * cts, c->n, c->d_crt, c->d_primes, c->L, c->K, crt_mode(c),
                                  c->stream);
                CHECK_LAUNCH();
            }
            const NttBatch eb = contiguous(c->ext_a, cts, 2L * c->K, c->L, c->K, c->n);
            if (int e = run_ntt_fwd2(c, ob, cts * 2 * c->L, eb, cts * 2 * c->K)) return e;
            c->ext_a_ready = true;
        } else {
            if (int e = run_ntt(c, ob, (long)B * nslots * 2 * c->L, false)) return e;
        }
        c->coef_written = chain_cf;
    }
    if (hps_sum) {
        ProfScope pm(c, PK_RELIN_MAC, (u64)Bd, 8.0 * c->n * c->L * Bd * (4.0 + gu));
        launch_relin_mac(out, 2L * c->L * c->n, c->d_hdig, c->d_rlk, c->d_rlk_s, (int)gu, out, 2L * c->L * c->n,
                         (int)Bd, c->n, c->L, c->d_primes, c->stream);
        CHECK_LAUNCH();
    }
    return 0;
}

// out = [B][dout][2][L][n] for the output limbs `limbs` (dout = limbs.size()), one group of items
static int dbfv_mul_group(exacto_ctx* c, size_t d, uint64_t base, uint64_t plain, const uint64_t* a,
                          const uint64_t* b, uint64_t* out, size_t B, bool b_extended,
                          const std::vector<int>* limbs, bool square = false) {
    if (int e = dbfv_plan(c, B, d, base, plain, *limbs, square)) return e;
    return mul_group_run(c, d, d, a, b, out, B, b_extended, limbs->size(), limbs->size(), &c->last_dbfv_ks, square);
}

// Every buffer of a dbfv_mul pass grows with its item count (the products' results and digits, their
// per-limb digit sums and 31-bit residues, the shared extensions: per_item below, 4.4 MB at cfg4 and
// 113 MB at cfg5), so a batch runs in groups of whole items whose buffers stay within
// EXACTO_DBFV_GROUP_MB (default 16 GiB of the 288 GB HBM: the BASELINE batches, 4.5 GB at cfg4 and
// 0.9 GB at cfg5, are one group -- a 4 GiB default split cfg4's 1024 items into 932 + 92 and cost 5 %).
// Items are independent: the groups give the same results as one pass.  out = [B][dout][2][L][n] for
// the output limbs `limbs` (nullptr: all d).
static int dbfv_mul_core(exacto_ctx* c, size_t d, uint64_t base, uint64_t plain, const uint64_t* a,
                         const uint64_t* b, uint64_t* out, size_t B, bool b_extended,
                         const std::vector<int>* limbs = nullptr, bool square = false) {
    std::vector<int> all;
    if (!limbs) {
        for (size_t k = 0; k < d; ++k) all.push_back((int)k);
        limbs = &all;
    }
    const size_t dout = limbs->size();
    const size_t budget = c->dbfv_group_bytes;
    const size_t n = c->n, L = c->L, K = c->K, G = c->G, S = std::max(c->S32, c->kw.S);
    const size_t per_item = 8 * n * (d * d * 2 * L + 2 * d * 2 * K) +       // products, both extensions
                            n * G * (d * d * 2 + d * (4 + 4 * S)) +         // digits, sums, residues
                            4 * n * d * 2 * L * S;                          // key-switch sums
    const size_t Bg = std::max<size_t>(1, budget / std::max<size_t>(per_item, 1));
    if (B <= Bg) return dbfv_mul_group(c, d, base, plain, a, b, out, B, b_extended, limbs, square);
    // several groups: no coefficient-form carry between chain steps (its buffers are whole-batch)
    c->coef_in = nullptr;
    c->coef_slot = -1;
    const size_t ctw = 2 * L * n;
    for (size_t g0 = 0; g0 < B; g0 += Bg) {
        const size_t cnt = std::min(Bg, B - g0);
        // b's extensions are per group here (a chain recomputes them for each group)
        if (int e = dbfv_mul_group(c, d, base, plain, a + g0 * d * ctw, b + g0 * d * ctw, out + g0 * dout * ctw, cnt,
                                   false, limbs, square))
            return e;
    }
    return 0;
}

static int ensure_twin(exacto_ctx* c, int i);

// A batch of independent items in `parts` near-equal parts on the context and its twins (each on its own
// stream, overlapping), or whole on the context: f(ctx, first item, items) per part.  The context's
// stream waits for every twin's part.  Parts measured: a depth-4 cfg5 chain batch 2 /
// 3 / 4 parts 2558 / 2575 / 2586 chains/s; dbfv_mul batches: cfg4 188.7k / 187.0k / 186.7k/s,
// u64_dbfv 57.5k / 56.2k / 55.1k/s -- so four parts for chains, two for single dbfv_mul batches.
template <class F>
static int split_run(exacto_ctx* c, size_t B, int want, F f) {
    const int parts = c->batch_split ? (int)std::min<size_t>(B, (size_t)std::min(want, exacto_ctx::MAX_TWINS + 1)) : 1;
    if (parts < 2 || !c->dual || c->prof || !c->rlk_loaded || c->deferred_code) return f(c, 0, B);
    const size_t per = (B + parts - 1) / parts;
    int rc = 0;
    for (int i = 1; i < parts; ++i) {
        const size_t i0 = per * i;
        if (i0 >= B) break;
        if (int e = ensure_twin(c, i - 1)) return e;
        const int r = f(c->twin[i - 1], i0, std::min(per, B - i0));
        if (!rc) rc = r;
    }
    const int r0 = f(c, 0, std::min(per, B));
    for (int i = 1; i < parts && per * i < B; ++i) {
        HIP_TRY(hipEventRecord(c->ev_twin_out[i - 1], c->twin[i - 1]->stream));
        HIP_TRY(hipStreamWaitEvent(c->stream, c->ev_twin_out[i - 1], 0));
    }
    return r0 ? r0 : rc;   // (the last error message is the failing call's)
}

extern "C" int exacto_dbfv_mul_dev(exacto_ctx* c, size_t d, uint64_t base, uint64_t plain, const uint64_t* a,
                                   const uint64_t* b, uint64_t* out, size_t B, const uint32_t* depth_a,
                                   const uint32_t* depth_b, uint32_t* depth_out) {
    if (int e = check_ctx(c)) return e;
    if (int e = dbfv_params_check(d, base, plain)) return e;
    // depth guard (dbfv/eval.rs:96-102)
    for (size_t i = 0; i < B; ++i) {
        const uint32_t da = depth_a ? depth_a[i] : 0, db = depth_b ? depth_b[i] : 0;
        if (std::max(da, db) + 1 > 1)
            return fail(EXACTO_ERR_NOT_IMPLEMENTED, "not yet implemented: chained dBFV multiplication requires "
                                                    "ciphertext-level lattice reduction (paper §4.6.2)");
    }
    if (B == 0) return 0;
    const size_t w = d * 2 * c->L * (size_t)c->n;
    if (int e = split_run(c, B, 2, [&](exacto_ctx* x, size_t i0, size_t cnt) {
            return dbfv_mul_core(x, d, base, plain, a + i0 * w, b + i0 * w, out + i0 * w, cnt, false);
        }))
        return e;
    if (depth_out)
        for (size_t i = 0; i < B; ++i) depth_out[i] = 1;
    return 0;
}

// dbfv_mul(a, a) with the symmetric plan (dbfv_plan sym): d (d + 1) / 2 of the d^2 products, the operand's
// extensions made once.  The checks and the depth guard are exacto_dbfv_mul_dev's with depth_b = depth_a.
extern "C" int exacto_dbfv_square_dev(exacto_ctx* c, size_t d, uint64_t base, uint64_t plain, const uint64_t* a,
                                      uint64_t* out, size_t B, const uint32_t* depth_a, uint32_t* depth_out) {
    if (int e = check_ctx(c)) return e;
    if (int e = dbfv_params_check(d, base, plain)) return e;
    for (size_t i = 0; i < B; ++i)
        if ((depth_a ? depth_a[i] : 0) + 1 > 1)
            return fail(EXACTO_ERR_NOT_IMPLEMENTED, "not yet implemented: chained dBFV multiplication requires "
                                                    "ciphertext-level lattice reduction (paper §4.6.2)");
    if (B == 0) return 0;
    const size_t w = d * 2 * c->L * (size_t)c->n;
    if (!a || !out) return invalid_param("null ciphertext pointer");
    if (a < out + B * w && out < a + B * w) return invalid_param("the output of a square must not overlap its input");
    if (int e = split_run(c, B, 2, [&](exacto_ctx* x, size_t i0, size_t cnt) {
            return dbfv_mul_core(x, d, base, plain, a + i0 * w, a + i0 * w, out + i0 * w, cnt, false, nullptr, true);
        }))
        return e;
    if (depth_out)
        for (size_t i = 0; i < B; ++i) depth_out[i] = 1;
    return 0;
}

// One GPU's share of a dbfv_mul whose output limbs are split across GPUs (dbfv/eval.rs:109-132): the
// output limbs limbs[0..nlimbs) only, out = [B][nlimbs][2][L][n] (slot s = limb limbs[s]), each exactly
// as exacto_dbfv_mul computes it (its pairs i + j = k, relinearised and summed, and the reduce
// folding of the high limbs).  Distinct limbs need no cross-GPU sum: the caller gathers the slots.
extern "C" int exacto_dbfv_mul_limbs_dev(exacto_ctx* c, size_t d, uint64_t base, uint64_t plain, const uint64_t* a,
                                         const uint64_t* b, uint64_t* out, size_t B, const uint32_t* limbs,
                                         size_t nlimbs) {
    if (int e = check_ctx(c)) return e;
    if (int e = dbfv_params_check(d, base, plain)) return e;
    if (nlimbs && !limbs) return invalid_param("null limb list");
    std::vector<int> ls;
    for (size_t s = 0; s < nlimbs; ++s) {
        if (limbs[s] >= d) return invalid_param("output limb " + std::to_string(limbs[s]) + " >= d = " + std::to_string(d));
        if (std::find(ls.begin(), ls.end(), (int)limbs[s]) != ls.end()) return invalid_param("repeated output limb");
        ls.push_back((int)limbs[s]);
    }
    if (B == 0 || ls.empty()) return 0;
    return dbfv_mul_core(c, d, base, plain, a, b, out, B, false, &ls);
}

extern "C" int exacto_dbfv_mul_limbs(exacto_ctx* c, size_t d, uint64_t base, uint64_t plain, const uint64_t* a,
                                     const uint64_t* b, uint64_t* out, size_t B, const uint32_t* limbs, size_t nlimbs) {
    if (!c) return invalid_param("null context");
    const size_t ctb = B * d * 2 * c->L * poly_bytes(c);
    return host_call(c, {{a, ctb}, {b, ctb}}, B * nlimbs * 2 * c->L * poly_bytes(c), out,
                     [&](std::vector<u64*>& in, u64* o) {
                         return exacto_dbfv_mul_limbs_dev(c, d, base, plain, in[0], in[1], o, B, limbs, nlimbs);
                     });
}

// ============================================================== sums of ciphertext products

// How many products of one output bfv_mul_sum key-switches as one sum on this context: what the
// resident key's 31-bit basis (or the wide one) lifts, what the summed scale takes where it runs
// (psum_max), and the caller's limit `cap` (0: none).  0: this context has no summed key switch (no
// 31-bit basis, gadget base above 2^16, small n, EXACTO_KS32=0, HPS, schoolbook): one per product.
// want > 0 (a bfv_mul_sum about to run sums of `want`): the primary basis is chosen for them first,
// as dbfv_mul does for its limbs.
static int mul_sum_group_max(exacto_ctx* c, int want, size_t cap, int* gmax) {
    *gmax = 0;
    const size_t gu = std::min<size_t>(c->G, c->rlk_keys);
    if (want > c->ks32_need_m) {
        c->ks32_need_m = want;
        if (c->rs_valid && c->ks32_lazy_active && want > c->ks32_sum_max) c->rs_valid = false;
    }
    const bool on = c->S32 > 0 && c->ks32 && c->digit16 && c->gbase <= 65536 && c->rlk_loaded && gu > 0 &&
                    !c->deferred_code;
    if (!on) return 0;
    if (int e = ensure_rs(c)) return e;
    int g = std::max(c->ks32_sum_max, c->kw.S > 0 ? c->kw.sum_max : 0);
    bool near60 = c->ntt_asm && c->ntt_asm_inv;
    for (u64 q : c->primes) near60 &= q < (1ull << 60) && q > (1ull << 60) - (1ull << 24);
    const bool psum = c->psum_env && c->psum_max >= 1 && c->share_ext && c->K > 0 && near60 &&
                      (c->logn == 12 || c->logn == 13) && exact_scale_sp_ok(c->L, c->K, crt_mode(c));
    if (psum) g = std::min(g, c->psum_max);
    if (cap) g = (int)std::min<size_t>((size_t)g, cap);
    *gmax = std::max(g, 0);
    return 0;
}

// One context's share of a bfv_mul_sum batch: items in passes of whole items within
// EXACTO_DBFV_GROUP_MB (as dbfv_mul_core), each pass one plan and one mul_group_run.  mmax: the most
// terms of one slot; cap: the caller's group limit (the parent context's when this is a twin).
static int mul_sum_core(exacto_ctx* c, const u64* a, size_t na, const u64* b, size_t nb, const uint32_t* ia,
                        const uint32_t* ib, const uint32_t* slot, size_t nterms, size_t nslots, size_t mmax, size_t cap,
                        u64* out, size_t B) {
    // chain state belongs to chains: this call neither reads a previous step's carry nor leaves one
    c->coef_in = nullptr;
    c->coef_slot = -1;
    c->ext_a_ready = false;
    int gmax = 0;
    if (int e = mul_sum_group_max(c, (int)std::min<size_t>(cap ? std::min(cap, mmax) : mmax, 64), cap, &gmax)) return e;
    // every slot within one group: one group per slot and no extra pass; no summed key switch: the
    // per-product path sums any number of products (launch_dbfv_combine)
    const size_t gcap = gmax >= 1 && mmax > (size_t)gmax ? (size_t)gmax : 0;
    size_t ngroups = nslots;
    if (gcap) {
        std::vector<size_t> cnt(nslots, 0);
        for (size_t t = 0; t < nterms; ++t) ++cnt[slot[t]];
        ngroups = 0;
        for (size_t s = 0; s < nslots; ++s) ngroups += (cnt[s] + gcap - 1) / gcap;
    }
    const size_t n = c->n, L = c->L, K = c->K, G = c->G, S = std::max(c->S32, c->kw.S);
    const size_t per_item = 8 * n * (nterms * 2 * L + (na + nb) * 2 * K) +              // products, both extensions
                            n * G * (nterms * 2 + ngroups * (4 + 4 * S)) +              // digits, sums, residues
                            4 * n * ngroups * 2 * L * S +                               // key-switch sums
                            (ngroups > nslots ? 8 * n * ngroups * 2 * L : 0);           // the groups' results
    const size_t Bg = std::max<size_t>(1, c->dbfv_group_bytes / std::max<size_t>(per_item, 1));
    const size_t ctw = 2 * L * n;
    for (size_t g0 = 0; g0 < B; g0 += Bg) {
        const size_t cnt = std::min(Bg, B - g0);
        if (int e = mul_sum_plan(c, cnt, na, nb, ia, ib, slot, nterms, nslots, gcap)) return e;
        if (int e = mul_group_run(c, na, nb, a + g0 * na * ctw, b + g0 * nb * ctw, out + g0 * nslots * ctw, cnt, false,
                                  (size_t)c->cached_ngroups, nslots, &c->last_mul_sum_mode))
            return e;
    }
    return 0;
}

// out[b][s] = sum over the terms t with slot[t] == s of bfv_mul_and_relin(a[b][ia[t]], b[b][ib[t]])
// (eval.rs:73-82 per product, bfv_add eval.rs:14-32 over the terms): the sums move in front of the key
// switch and the forward transform (mul_group_run), in groups of what one key switch lifts.
extern "C" int exacto_bfv_mul_sum_dev(exacto_ctx* c, const uint64_t* a, size_t na, const uint64_t* b, size_t nb,
                                      const uint32_t* ia, const uint32_t* ib, const uint32_t* slot, size_t nterms,
                                      size_t nslots, uint64_t* out, size_t B) {
    if (int e = check_ctx(c)) return e;
    if (nterms == 0) return invalid_param("bfv_mul_sum: nterms = 0 (no products to sum)");
    if (!ia || !ib || !slot) return invalid_param("bfv_mul_sum: null term list");
    if (nterms > 0x7fffffffu / 4) return invalid_param("bfv_mul_sum: nterms = " + std::to_string(nterms) + " is too large");
    std::vector<size_t> per_slot(nslots, 0);
    for (size_t t = 0; t < nterms; ++t) {
        if (ia[t] >= na)
            return invalid_param("bfv_mul_sum: term " + std::to_string(t) + " left index " + std::to_string(ia[t]) +
                                 " >= na = " + std::to_string(na));
        if (ib[t] >= nb)
            return invalid_param("bfv_mul_sum: term " + std::to_string(t) + " right index " + std::to_string(ib[t]) +
                                 " >= nb = " + std::to_string(nb));
        if (slot[t] >= nslots)
            return invalid_param("bfv_mul_sum: term " + std::to_string(t) + " slot " + std::to_string(slot[t]) +
                                 " >= nslots = " + std::to_string(nslots));
        ++per_slot[slot[t]];
    }
    size_t mmax = 0;
    for (size_t s = 0; s < nslots; ++s) {
        if (per_slot[s] == 0) return invalid_param("bfv_mul_sum: output slot " + std::to_string(s) + " has no term");
        mmax = std::max(mmax, per_slot[s]);
    }
    if (B == 0) return 0;
    if (!a || !b || !out) return invalid_param("bfv_mul_sum: null ciphertext buffer");
    if ((uintptr_t)out & 15) return invalid_param("bfv_mul_sum: out must be 16-byte aligned");
    const size_t ctw = 2 * c->L * (size_t)c->n;
    auto overlaps = [&](const u64* p, size_t cts) { return out < p + B * cts * ctw && p < out + B * nslots * ctw; };
    if (overlaps(a, na) || overlaps(b, nb)) return invalid_param("bfv_mul_sum: out overlaps an input");
    if (c->deferred_code) return fail(c->deferred_code, c->deferred_msg);
    if (!c->rlk_loaded) return fail(EXACTO_ERR_MISSING_KEY, "key not available: relinearization key not loaded");
    const size_t cap = c->mul_sum_cap;
    // two parts on two streams, as exacto_dbfv_mul_dev (split_run's measurements)
    return split_run(c, B, 2, [&](exacto_ctx* x, size_t i0, size_t cnt) {
        return mul_sum_core(x, a + i0 * na * ctw, na, b + i0 * nb * ctw, nb, ia, ib, slot, nterms, nslots, mmax, cap,
                            out + i0 * nslots * ctw, cnt);
    });
}

extern "C" int exacto_bfv_mul_sum(exacto_ctx* c, const uint64_t* a, size_t na, const uint64_t* b, size_t nb,
                                  const uint32_t* ia, const uint32_t* ib, const uint32_t* slot, size_t nterms,
                                  size_t nslots, uint64_t* out, size_t B) {
    if (!c) return invalid_param("null context");
    const size_t ctb = 2 * c->L * poly_bytes(c);
    return host_call(c, {{a, B * na * ctb}, {b, B * nb * ctb}}, B * nslots * ctb, out,
                     [&](std::vector<u64*>& in, u64* o) {
                         return exacto_bfv_mul_sum_dev(c, in[0], na, in[1], nb, ia, ib, slot, nterms, nslots, o, B);
                     });
}

extern "C" int exacto_ctx_set_mul_sum_group(exacto_ctx* c, size_t max_products) {
    if (!c) return invalid_param("null context");
    c->mul_sum_cap = max_products;
    return 0;
}

extern "C" int exacto_bfv_mul_sum_info(exacto_ctx* c, size_t* group_max, int* last_mode) {
    if (int e = check_ctx(c)) return e;
    int gmax = 0;
    if (int e = mul_sum_group_max(c, 0, c->mul_sum_cap, &gmax)) return e;
    if (group_max) *group_max = (size_t)std::max(gmax, 1);   // (no summed key switch: one product each)
    if (last_mode) *last_mode = c->last_mul_sum_mode;
    return 0;
}

// dBFV multiplication chain with the guard-bypass semantics of paper_repro.rs:203-236 (and the
// chain of bfv_host.rs:258-288 without its bootstrap): acc <- dbfv_mul(acc, y) `depth` times,
// both mul_depth reset to 0 before every step; intermediates ping-pong between two
// context-owned device buffers and never leave HBM.
// The twin of a context (its second chain stream): created on first use with the same parameters
// and chunking, its own stream, workspaces and scratch; the relinearisation key is copied from the
// context whenever it changed since (rlk_version), ordered after everything on the context's stream.
static int ensure_twin(exacto_ctx* c, int i) {
    if (!c->twin[i]) {
        exacto_ctx* t = nullptr;
        if (int e = exacto_ctx_create(&t, c->n, c->ctq.data(), c->L, c->user_aux.empty() ? nullptr : c->user_aux.data(),
                                      c->user_aux.size(), c->plain, c->gbase, c->device))
            return e;
        t->batch_split = false;
        c->twin[i] = t;
        if (!c->ev_twin_in) HIP_TRY(hipEventCreateWithFlags(&c->ev_twin_in, hipEventDisableTiming));
        HIP_TRY(hipEventCreateWithFlags(&c->ev_twin_out[i], hipEventDisableTiming));
    }
    exacto_ctx* t = c->twin[i];
    t->chunk = c->chunk;
    HIP_TRY(hipEventRecord(c->ev_twin_in, c->stream));
    HIP_TRY(hipStreamWaitEvent(t->stream, c->ev_twin_in, 0));
    if (c->twin_rlk_version[i] != c->rlk_version) {
        if (int e = exacto_ctx_load_relin_key_dev(t, c->d_rlk, c->rlk_keys)) return e;
        c->twin_rlk_version[i] = c->rlk_version;
    }
    return 0;
}

static int dbfv_chain_one(exacto_ctx* c, size_t d, uint64_t base, uint64_t plain, const uint64_t* x,
                          const uint64_t* y, uint64_t* out, size_t B, size_t depth);

extern "C" int exacto_dbfv_mul_chain_dev(exacto_ctx* c, size_t d, uint64_t base, uint64_t plain,
                                         const uint64_t* x, const uint64_t* y, uint64_t* out, size_t B,
                                         size_t depth) {
    if (int e = check_ctx(c)) return e;
    // two halves on two streams: items are independent, so each half's chain is the chain of those
    // items (bit-identical: tests/test_gpu_chain.py against EXACTO_CHAIN_SPLIT=0)
    if (depth >= 1)
        if (int e = dbfv_params_check(d, base, plain)) return e;
    const size_t w = d * 2 * c->L * (size_t)c->n;
    if (depth == 0) return dbfv_chain_one(c, d, base, plain, x, y, out, B, depth);
    return split_run(c, B, 4, [&](exacto_ctx* t, size_t i0, size_t cnt) {
        return dbfv_chain_one(t, d, base, plain, x + i0 * w, y + i0 * w, out + i0 * w, cnt, depth);
    });
}

static int dbfv_chain_one(exacto_ctx* c, size_t d, uint64_t base, uint64_t plain, const uint64_t* x,
                          const uint64_t* y, uint64_t* out, size_t B, size_t depth) {
    const size_t bytes = B * d * 2 * c->L * poly_bytes(c);
    if (depth == 0) {
        if (B && out != x) HIP_TRY(dev_copy(out, x, bytes, c->stream));
        return 0;
    }
    if (depth > 1 && B) {
        if (c->chain_buf.grow(2 * bytes)) return EXACTO_ERR_HIP;
    }
    if (int e = dbfv_params_check(d, base, plain)) return e;
    if (B == 0) return 0;
    // the coefficient form of each step's result (psum path, one item group) goes to chain_coef, and
    // the next step lifts it directly: one batched inverse NTT of its input less per step
    // (dbfv_mul_group allocates chain_coef, two halves of `bytes`, only when the step runs psum)
    const bool carry = depth > 1 && c->share_ext && c->K > 0;
    c->ext_a_ready = false;
    const uint64_t* src = x;
    const u64* src_coef = nullptr;
    int rc = 0;
    for (size_t k = 0; k < depth && rc == 0; ++k) {
        uint64_t* dst = (k + 1 == depth) ? out : c->chain_buf + (k % 2) * (bytes / sizeof(u64));
        c->coef_in = src_coef;
        c->coef_slot = carry && k + 1 < depth ? (int)(k % 2) : -1;
        c->coef_slot_words = bytes / sizeof(u64);
        c->coef_out = nullptr;
        c->coef_written = false;
        // y's extensions are computed by the first step and reused by the others
        rc = dbfv_mul_core(c, d, base, plain, src, y, dst, B, k > 0);
        src_coef = c->coef_out && c->coef_written ? c->coef_out : nullptr;
        src = dst;
    }
    c->coef_in = nullptr;
    c->coef_out = nullptr;
    c->coef_slot = -1;
    c->coef_written = false;
    c->ext_a_ready = false;
    return rc;
}

extern "C" int exacto_dbfv_mul_chain(exacto_ctx* c, size_t d, uint64_t base, uint64_t plain, const uint64_t* x,
                                     const uint64_t* y, uint64_t* out, size_t B, size_t depth) {
    if (!c) return invalid_param("null context");
    const size_t bytes = B * d * 2 * c->L * poly_bytes(c);
    return host_call(c, {{x, bytes}, {y, bytes}}, bytes, out, [&](std::vector<u64*>& dv, u64* o) {
        return exacto_dbfv_mul_chain_dev(c, d, base, plain, dv[0], dv[1], o, B, depth);
    });
}

extern "C" int exacto_dbfv_square(exacto_ctx* c, size_t d, uint64_t base, uint64_t plain, const uint64_t* a,
                                  uint64_t* out, size_t B, const uint32_t* depth_a, uint32_t* depth_out) {
    if (!c) return invalid_param("null context");
    const size_t bytes = B * d * 2 * c->L * poly_bytes(c);
    return host_call(c, {{a, bytes}}, bytes, out, [&](std::vector<u64*>& dv, u64* o) {
        return exacto_dbfv_square_dev(c, d, base, plain, dv[0], o, B, depth_a, depth_out);
    });
}

extern "C" int exacto_dbfv_mul(exacto_ctx* c, size_t d, uint64_t base, uint64_t plain, const uint64_t* a,
                               const uint64_t* b, uint64_t* out, size_t B, const uint32_t* depth_a,
                               const uint32_t* depth_b, uint32_t* depth_out) {
    if (!c) return invalid_param("null context");
    const size_t bytes = B * d * 2 * c->L * poly_bytes(c);
    return host_call(c, {{a, bytes}, {b, bytes}}, bytes, out, [&](std::vector<u64*>& dv, u64* o) {
        return exacto_dbfv_mul_dev(c, d, base, plain, dv[0], dv[1], o, B, depth_a, depth_b, depth_out);
    });
}

// ============================================================== keygen / encryption

// Gaussian CDT of sampling/gaussian.rs:18-33 (unnormalised cumulative weights over
// [-ceil(6 sigma), ceil(6 sigma)]), cached on the device per sigma.
static int gaussian_table(exacto_ctx* c, double sigma, int* tail, int* len, double* total) {
    if (!(sigma > 0.0) || sigma > 1e6) return invalid_param("sigma must be positive");
    const int t = (int)std::ceil(6.0 * sigma);
    std::vector<double> cdf;
    double cum = 0.0;
    const double two_s2 = 2.0 * sigma * sigma;
    for (long x = -t; x <= t; ++x) {
        cum += std::exp(-(double)(x * x) / two_s2);
        cdf.push_back(cum);
    }
    if (c->cdt_sigma != sigma || !c->d_cdt) {
        if (c->d_cdt.grow(cdf.size() * sizeof(double))) return EXACTO_ERR_HIP;
        HIP_TRY(hipStreamSynchronize(c->stream));  // in-flight samplers may still read the old table
        if (int e_ = upload(c, c->d_cdt, cdf.data(), cdf.size() * sizeof(double))) return e_;
        c->cdt_sigma = sigma;
    }
    *tail = t;
    *len = (int)cdf.size();
    *total = cum;
    return 0;
}

static ChaChaKey chacha_key(const uint64_t* key) {
    ChaChaKey k{};
    for (int i = 0; i < 4; ++i) k.w[i] = key ? key[i] : 0;
    return k;
}

// Sample `polys` polynomials ([L][n] residues each, at out + p * stride) with indices base + p * step.
static int sample_polys(exacto_ctx* c, int kind, const ChaChaKey& key, u64 stream, u64* out, long stride, u64 base,
                        u64 step, long polys, double sigma) {
    int tail = 0, len = 0;
    double total = 0.0;
    if (kind == KG_GAUSSIAN)
        if (int e = gaussian_table(c, sigma, &tail, &len, &total)) return e;
    launch_sample(kind, key, stream, out, stride, base, step, polys, c->n, c->L, c->d_primes, c->d_cdt, len, tail,
                  total, c->stream);
    CHECK_LAUNCH();
    return 0;
}

// Forward NTT of `items` groups of `polys_per_item` [L][n] blocks spaced `stride` words apart.
static int ntt_items(exacto_ctx* c, u64* data, long items, long stride, long polys_per_item) {
    NttBatch nb{};
    nb.src = data; nb.src_item_stride = stride;
    nb.dst = data; nb.dst_item_stride = stride;
    nb.ppi = (int)polys_per_item; nb.prime_base = 0; nb.period = c->L;
    return run_ntt(c, nb, items * polys_per_item, false);
}

extern "C" int exacto_gen_secret_key_dev(exacto_ctx* c, const uint64_t* key, uint64_t stream, uint64_t* sk) {
    if (int e = check_ctx(c)) return e;
    if (!key || !sk) return invalid_param("null argument");
    // keygen.rs:69-79: ternary s mod q0 -> RnsPoly::from_coeff_poly
    if (int e = sample_polys(c, KG_TERNARY, chacha_key(key), stream, sk, 0, 0, 1, 1, 0.0)) return e;
    return ntt_items(c, sk, 1, 0, c->L);
}

extern "C" int exacto_gen_public_key_dev(exacto_ctx* c, const uint64_t* sk, double sigma, const uint64_t* key,
                                         uint64_t stream, uint64_t* pk) {
    if (int e = check_ctx(c)) return e;
    if (!key || !sk || !pk) return invalid_param("null argument");
    const long Ln = (long)c->L * c->n;
    const ChaChaKey k = chacha_key(key);
    // keygen.rs:90-110: a (-> pk1), e (-> pk0 slot), pk0 = -(a s + e)
    if (int e = sample_polys(c, KG_UNIFORM, k, stream, pk + Ln, 0, 0, 1, 1, sigma)) return e;
    if (int e = sample_polys(c, KG_GAUSSIAN, k, stream, pk, 0, 1, 1, 1, sigma)) return e;
    if (int e = ntt_items(c, pk, 1, 0, 2L * c->L)) return e;
    launch_combine(KG_PK, pk, 1, 0, Ln, sk, nullptr, nullptr, nullptr, nullptr, c->n, c->L, c->d_primes, c->stream);
    CHECK_LAUNCH();
    return 0;
}

extern "C" int exacto_gen_relin_key_dev(exacto_ctx* c, const uint64_t* sk, double sigma, const uint64_t* key,
                                        uint64_t stream, size_t num_keys, uint64_t* rlk) {
    if (int e = check_ctx(c)) return e;
    if (!key || !sk) return invalid_param("null argument");
    const long Ln = (long)c->L * c->n;
    const bool resident = rlk == nullptr;
    if (resident) {  // generate straight into the context's resident key (no host build, no upload)
        rlk = exacto_ctx_relin_key_buffer(c, num_keys);
        if (!rlk && num_keys) return fail(EXACTO_ERR_HIP, "HIP error: relinearization key allocation failed");
    }
    if (num_keys == 0) return 0;
    // g_i = base^i mod q_l (keygen.rs:133-158: gadget_s_sq scaled by base after every key)
    std::vector<u64> gpow(num_keys * c->L);
    for (int l = 0; l < c->L; ++l) {
        const u64 q = c->primes[l];
        u64 g = 1 % q;
        const u64 b = c->gbase % q;
        for (size_t i = 0; i < num_keys; ++i) {
            gpow[i * c->L + l] = g;
            g = (u64)((u128)g * b % q);
        }
    }
    if (c->d_gpow.grow(gpow.size() * sizeof(u64))) return EXACTO_ERR_HIP;
    // the table is host-pageable and d_gpow may still be read by a previous call's kernels
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (int e_ = upload(c, c->d_gpow, gpow.data(), gpow.size() * sizeof(u64))) return e_;
    const ChaChaKey k = chacha_key(key);
    // key i: a_i (index 2i) into the rlk1 slot, e_i (index 2i+1) into the rlk0 slot
    if (int e = sample_polys(c, KG_UNIFORM, k, stream, rlk + Ln, 2 * Ln, 0, 2, (long)num_keys, sigma)) return e;
    if (int e = sample_polys(c, KG_GAUSSIAN, k, stream, rlk, 2 * Ln, 1, 2, (long)num_keys, sigma)) return e;
    if (int e = ntt_items(c, rlk, (long)num_keys, 2 * Ln, 2L * c->L)) return e;
    launch_combine(KG_RLK, rlk, (long)num_keys, 2 * Ln, Ln, sk, nullptr, nullptr, nullptr, c->d_gpow, c->n, c->L,
                   c->d_primes, c->stream);
    CHECK_LAUNCH();
    if (resident) {
        HIP_TRY(hipStreamSynchronize(c->stream));  // the key must be complete before it is marked loaded
        c->rlk_keys = num_keys;
        c->rlk_loaded = true;
        c->rlk_s_valid = false;
        c->rs_valid = false; c->kw.rs_valid = false;
        ++c->rlk_version;
    }
    return 0;
}

// Delta_i = floor(Q / p) mod q_i (encrypt.rs:205-229), device copy in c->d_delta (with Shoup companions).
int exacto::delta_residues(exacto_ctx* c) {
    if (c->delta_ok) return 0;
    // Q as little-endian 64-bit words, then floor(Q / p) by long division, then mod each q_i
    std::vector<u64> Qw(1, 1);
    for (int i = 0; i < c->L; ++i) {
        u128 carry = 0;
        for (auto& w : Qw) {
            const u128 t = (u128)w * c->primes[i] + carry;
            w = (u64)t;
            carry = t >> 64;
        }
        if (carry) Qw.push_back((u64)carry);
    }
    std::vector<u64> D(Qw.size());
    u128 rem = 0;
    for (size_t w = Qw.size(); w-- > 0;) {
        const u128 cur = (rem << 64) | Qw[w];
        D[w] = (u64)(cur / c->plain);
        rem = cur % c->plain;
    }
    bool zero = true;
    for (u64 w : D) zero &= (w == 0);
    if (zero) return invalid_param("ciphertext modulus product Q must be >= plaintext modulus p");
    // [0, L): the residues; [EXACTO_MAX_L, EXACTO_MAX_L + L): their Shoup companions (noise.hip)
    std::vector<u64> dr(2 * EXACTO_MAX_L, 0);
    for (int i = 0; i < c->L; ++i) {
        u128 r = 0;
        for (size_t w = D.size(); w-- > 0;) r = ((r << 64) | D[w]) % c->primes[i];
        dr[i] = (u64)r;
        dr[EXACTO_MAX_L + i] = shoup_h((u64)r, c->primes[i]);
    }
    if (!c->d_delta)
        if (int e_ = c->d_delta.alloc(2 * EXACTO_MAX_L * sizeof(u64))) return e_;
    if (int e_ = upload(c, c->d_delta, dr.data(), dr.size() * sizeof(u64))) return e_;
    c->delta_ok = true;
    return 0;
}

// The plaintexts of a dBFV encryption (dbfv/encrypt.rs:105-141): B scalars, or (poly) B polynomials
// [B][n], each encrypted as its d base-`base` digit polynomials.
struct DbfvPlain {
    size_t d;
    u64 base, plain;
    bool poly;
};

// encrypt.rs:29-106 for a batch: pt = [B][n] plaintext coefficients, ct = [B][2][L][n] (NTT domain).
// pk == nullptr: secret-key encryption with sk; otherwise public-key encryption with pk [2][L][n].
// dp != nullptr: pt holds B dBFV plaintexts and the batch is their B * d digit encryptions, ct =
// [B][d][2][L][n]: item b * d + k is what this function gives for digit plaintext k of item b; only
// Delta*m is produced differently (straight from pt, and already in the NTT domain for scalars).
// item0: the batch is items item0 .. item0 + B - 1 of a larger call (their sample indices; the batch
// compositions' chunks)
static int encrypt_batch(exacto_ctx* c, const u64* pt, const u64* sk, const u64* pk, double sigma,
                         const uint64_t* key, u64 stream, u64* ct, size_t B, const DbfvPlain* dp = nullptr,
                         size_t item0 = 0) {
    if (!key || !pt || !ct || (!sk && !pk)) return invalid_param("null argument");
    const size_t items = dp ? B * dp->d : B;
    if (items == 0) return 0;
    if (int e = delta_residues(c)) return e;
    const long Ln = (long)c->L * c->n;
    const ChaChaKey k = chacha_key(key);
    // scratch: Delta m [items][L][n], and u [items][L][n] for pk-encryption
    if (c->enc_buf.grow(items * (pk ? 2 : 1) * Ln * sizeof(u64))) return EXACTO_ERR_HIP;
    u64* dm = c->enc_buf;
    u64* u = c->enc_buf + items * Ln;
    if (dp)
        launch_dbfv_digits(pt, dp->poly, c->d_delta, dm, (long)B, (int)dp->d, dp->base, dp->plain, c->n, c->L,
                           c->d_primes, c->stream);
    else
        launch_scale_plain(pt, c->d_delta, dm, (long)B, c->n, c->L, c->d_primes, c->stream);
    CHECK_LAUNCH();
    if (!dp || dp->poly)
        if (int e = ntt_items(c, dm, (long)items, Ln, c->L)) return e;
    if (!pk) {
        // encrypt.rs:79-106, item b: a (index 2b) -> c1, e (index 2b+1) -> c0 slot
        if (int e = sample_polys(c, KG_UNIFORM, k, stream, ct + Ln, 2 * Ln, 2 * item0, 2, (long)items, sigma)) return e;
        if (int e = sample_polys(c, KG_GAUSSIAN, k, stream, ct, 2 * Ln, 2 * item0 + 1, 2, (long)items, sigma)) return e;
        if (int e = ntt_items(c, ct, (long)items, 2 * Ln, 2L * c->L)) return e;
        launch_combine(KG_ENC_SK, ct, (long)items, 2 * Ln, Ln, sk, dm, nullptr, nullptr, nullptr, c->n, c->L,
                       c->d_primes, c->stream);
    } else {
        // encrypt.rs:29-69, item b: u binary (3b), e1 (3b+1) -> c0 slot, e2 (3b+2) -> c1 slot
        if (int e = sample_polys(c, KG_BINARY, k, stream, u, Ln, 3 * item0, 3, (long)items, sigma)) return e;
        if (int e = sample_polys(c, KG_GAUSSIAN, k, stream, ct, 2 * Ln, 3 * item0 + 1, 3, (long)items, sigma)) return e;
        if (int e = sample_polys(c, KG_GAUSSIAN, k, stream, ct + Ln, 2 * Ln, 3 * item0 + 2, 3, (long)items, sigma)) return e;
        if (int e = ntt_items(c, u, (long)items, Ln, c->L)) return e;
        if (int e = ntt_items(c, ct, (long)items, 2 * Ln, 2L * c->L)) return e;
        launch_combine(KG_ENC_PK, ct, (long)items, 2 * Ln, Ln, nullptr, u, dm, pk, nullptr, c->n, c->L, c->d_primes,
                       c->stream);
    }
    CHECK_LAUNCH();
    return 0;
}

extern "C" int exacto_encrypt_sk_dev(exacto_ctx* c, const uint64_t* pt, const uint64_t* sk, double sigma,
                                     const uint64_t* key, uint64_t stream, uint64_t* ct, size_t B) {
    if (int e = check_ctx(c)) return e;
    if (!sk) return invalid_param("null argument");
    return encrypt_batch(c, pt, sk, nullptr, sigma, key, stream, ct, B);
}

extern "C" int exacto_encrypt_pk_dev(exacto_ctx* c, const uint64_t* pt, const uint64_t* pk, double sigma,
                                     const uint64_t* key, uint64_t stream, uint64_t* ct, size_t B) {
    if (int e = check_ctx(c)) return e;
    if (!pk) return invalid_param("null argument");
    return encrypt_batch(c, pt, nullptr, pk, sigma, key, stream, ct, B);
}

// ---- Galois automorphisms (eval.rs:512-561, keygen.rs:171-262)

// gen_galois_key_with_rng (keygen.rs:171-209).  s(X^k) is formed as the reference does: limb 0 of s
// in the coefficient domain (mod q0), sigma_k mod q0, then reduced modulo every q_i (keygen.rs:179-182).
extern "C" int exacto_gen_galois_key_dev(exacto_ctx* c, const uint64_t* sk, uint64_t element, double sigma,
                                         const uint64_t* key, uint64_t stream, size_t num_keys, uint64_t* gk) {
    if (int e = check_ctx(c)) return e;
    if (!key || !sk || !gk) return invalid_param("null argument");
    if (num_keys == 0) return 0;
    const int n = c->n, L = c->L;
    const long Ln = (long)L * n;
    if (c->enc_buf.grow((size_t)(2 * n + Ln) * sizeof(u64))) return EXACTO_ERR_HIP;
    u64 *t0 = c->enc_buf, *t1 = t0 + n, *s_auto = t1 + n;
    HIP_TRY(dev_copy(t0, sk, n * sizeof(u64), c->stream));
    if (int e = run_ntt(c, contiguous(t0, 1, 1, 0, 1, n), 1, true)) return e;
    launch_automorph(t0, n, t1, n, 1, 1, n, 1, element, c->d_primes, 0, c->stream);
    launch_lift_q0(t1, s_auto, 1, n, L, c->d_primes, c->stream);
    CHECK_LAUNCH();
    if (int e = ntt_items(c, s_auto, 1, 0, L)) return e;
    std::vector<u64> gpow(num_keys * L);
    for (int l = 0; l < L; ++l) {
        const u64 q = c->primes[l];
        u64 g = 1 % q;
        const u64 b = c->gbase % q;
        for (size_t i = 0; i < num_keys; ++i) {
            gpow[i * L + l] = g;
            g = (u64)((u128)g * b % q);
        }
    }
    if (c->d_gpow.grow(gpow.size() * sizeof(u64))) return EXACTO_ERR_HIP;
    // the table is host-pageable and d_gpow may still be read by a previous call's kernels
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (int e_ = upload(c, c->d_gpow, gpow.data(), gpow.size() * sizeof(u64))) return e_;
    const ChaChaKey k = chacha_key(key);
    if (int e = sample_polys(c, KG_UNIFORM, k, stream, gk + Ln, 2 * Ln, 0, 2, (long)num_keys, sigma)) return e;
    if (int e = sample_polys(c, KG_GAUSSIAN, k, stream, gk, 2 * Ln, 1, 2, (long)num_keys, sigma)) return e;
    if (int e = ntt_items(c, gk, (long)num_keys, 2 * Ln, 2L * L)) return e;
    launch_combine(KG_GALOIS, gk, (long)num_keys, 2 * Ln, Ln, sk, s_auto, nullptr, nullptr, c->d_gpow, n, L,
                   c->d_primes, c->stream);
    CHECK_LAUNCH();
    // gpow / s_auto scratch is reused by the next call: finish this one first
    HIP_TRY(hipStreamSynchronize(c->stream));
    return 0;
}

// bfv_apply_automorphism (eval.rs:512-561), batched: sigma_k(c0) + sum_i d_i (.) gk_i0, sum_i d_i (.) gk_i1
// with d = gadget digits of sigma_k(c1) (exact CRT: extension semantics for Q >= 2^64, as relinearize).
extern "C" int exacto_bfv_apply_automorphism_dev(exacto_ctx* c, const uint64_t* ct, size_t polys, uint64_t element,
                                                 const uint64_t* gk, size_t num_keys, uint64_t* out, size_t B) {
    if (int e = check_ctx(c)) return e;
    if (polys != 2) return invalid_param("automorphism requires degree-1 ciphertext");
    if (num_keys == 0 || !gk) return invalid_param("galois key is empty");
    if (B == 0) return 0;
    const int n = c->n, L = c->L;
    const long Ln = (long)L * n;
    const int guse = (int)std::min<size_t>(c->G, num_keys);
    const size_t count = (size_t)guse * 2 * Ln;
    const bool d16 = c->digit16 && c->gbase <= 65536;  // int16 digits, as in run_mul
    // ks32 key switch (as run_mul): the key converted to the 31-bit basis on every call (the
    // caller may pass a different key in the same buffer), G L (2L) 60-bit (32-bit) transforms
    // The narrow basis (kn) always: its bound holds for any key, and this key's norms are not
    // examined (the lazy basis is chosen per resident relinearisation key only).
    const Ks32Basis& kb = c->kn;
    const bool k32 = d16 && c->ks32 && kb.S > 0 && c->path == EXACTO_PATH_EXACT_RNS;
    if (k32) {
        if (int e = ks32_convert_key(c, gk, (size_t)guse, c->d_gk_rs, kb.S, kb.d_p32, kb.mac_form)) return e;
    } else {
        if (c->gk_s.grow(count * sizeof(u64))) return EXACTO_ERR_HIP;
        launch_shoup_companions(gk, c->gk_s, (long)count, n, L, c->d_primes, c->stream);
        CHECK_LAUNCH();
    }
    const size_t C = std::min<size_t>(c->chunk, B);
    // chunks alternate over the pipeline lanes as in run_mul (the key tables above are made on
    // the main stream before the fork)
    LanePass pass;
    if (int e = pass.begin(c, (long)((B + C - 1) / C), C)) return e;
    for (size_t s0 = 0; s0 < B; s0 += C) {
        const int cnt = (int)std::min(C, B - s0);
        LaneGuard lane = pass.chunk((long)(s0 / C));
        const u64* src = ct + s0 * 2 * Ln;
        u64* dst = out + s0 * 2 * Ln;
        NttBatch nb{};
        nb.src = src; nb.src_item_stride = 2 * Ln;
        nb.dst = c->ws.coefQ; nb.dst_item_stride = 2 * Ln;
        nb.ppi = 2 * L; nb.prime_base = 0; nb.period = L;
        if (int e = run_ntt(c, nb, (long)cnt * 2 * L, true)) return e;
        launch_automorph(c->ws.coefQ, 2 * Ln, c->ws.T, 2 * Ln, cnt, 2, n, L, element, c->d_primes, -1, c->stream);
        CHECK_LAUNCH();
        if (k32) {
            // digits of sigma(c1); sum_g d_g * r_g over the integers added to (sigma(c0), 0) in the
            // coefficient domain; then both components forward
            launch_decompose(c->ws.T + Ln, 2 * Ln, c->ws.D, guse, cnt, n, c->d_crt, c->d_primes, L, c->stream,
                             c->ws.D16);
            CHECK_LAUNCH();
            launch_rows(c->ws.T + Ln, 2 * Ln, nullptr, 0, Ln, cnt, c->stream);
            CHECK_LAUNCH();
            ks32_digits(c->ws.D16, c->ws.DS, cnt, guse, kb.S, c->logn, kb.d_p32, kb.mac_form, c->stream);
            ks32_mac(c->ws.DS, c->d_gk_rs, c->ws.U, cnt, guse, L, kb.S, n, kb.d_p32, kb.mac_form, c->stream);
            ks32_crt(c->ws.U, c->ws.T, 2 * Ln, cnt, L, kb.S, c->logn, kb.d_kst, kb.d_p32, c->d_primes, kb.mac_form, c->stream,
                     c->ks_fpc && kb.fpc_max >= 1);
            CHECK_LAUNCH();
            NttBatch rb{};
            rb.src = c->ws.T; rb.src_item_stride = 2 * Ln;
            rb.dst = dst; rb.dst_item_stride = 2 * Ln;
            rb.ppi = 2 * L; rb.prime_base = 0; rb.period = L;
            if (int e = run_ntt(c, rb, (long)cnt * 2 * L, false)) return e;
            continue;
        }
        NttBatch c0{};
        c0.src = c->ws.T; c0.src_item_stride = 2 * Ln;
        c0.dst = dst; c0.dst_item_stride = 2 * Ln;
        c0.ppi = L; c0.prime_base = 0; c0.period = L;
        if (int e = run_ntt(c, c0, (long)cnt * L, false)) return e;
        launch_rows(dst + Ln, 2 * Ln, nullptr, 0, Ln, cnt, c->stream);
        launch_decompose(c->ws.T + Ln, 2 * Ln, c->ws.D, guse, cnt, n, c->d_crt, c->d_primes, L, c->stream,
                         d16 ? c->ws.D16 : nullptr);
        CHECK_LAUNCH();
        NttBatch db = contiguous(c->ws.D, cnt, (long)guse * L, 0, L, n);
        if (d16) {
            db.src16 = c->ws.D16;
            db.src16_item_stride = (long)guse * n;
        }
        if (int e = run_ntt(c, db, (long)cnt * guse * L, false)) return e;
        launch_relin_mac(dst, 2 * Ln, c->ws.D, gk, c->gk_s, guse, dst, 2 * Ln, cnt, n, L, c->d_primes, c->stream);
        CHECK_LAUNCH();
    }
    return 0;
}

extern "C" int exacto_gen_galois_key(exacto_ctx* c, const uint64_t* sk, uint64_t element, double sigma,
                                     const uint64_t* key, uint64_t stream, size_t num_keys, uint64_t* gk) {
    if (!c) return invalid_param("null context");
    return host_call(c, {{sk, c->L * poly_bytes(c)}}, num_keys * 2 * c->L * poly_bytes(c), gk,
                     [&](std::vector<u64*>& d, u64* o) {
                         return exacto_gen_galois_key_dev(c, d[0], element, sigma, key, stream, num_keys, o);
                     });
}

extern "C" int exacto_bfv_apply_automorphism(exacto_ctx* c, const uint64_t* ct, size_t polys, uint64_t element,
                                             const uint64_t* gk, size_t num_keys, uint64_t* out, size_t B) {
    if (!c) return invalid_param("null context");
    if (polys != 2) return invalid_param("automorphism requires degree-1 ciphertext");
    return host_call(c, {{ct, B * 2 * c->L * poly_bytes(c)}, {gk, num_keys * 2 * c->L * poly_bytes(c)}},
                     B * 2 * c->L * poly_bytes(c), out, [&](std::vector<u64*>& d, u64* o) {
                         return exacto_bfv_apply_automorphism_dev(c, d[0], polys, element, d[1], num_keys, o, B);
                     });
}

// ---- plaintext-ciphertext operations and the trace (bfv/eval.rs:468-503, 572-652) ----

static int pl_scratch(exacto_ctx* c, size_t words) {
    if (c->pl_buf.grow(words * sizeof(u64))) return EXACTO_ERR_HIP;
    return 0;
}

// pt [items][n] (any u64) -> NTT(pt mod q_i [* Delta_i]) as [items][L][n] in c->pl_buf
static int lift_plain(exacto_ctx* c, const u64* pt, long items, bool delta) {
    const long Ln = (long)c->L * c->n;
    if (delta)
        if (int e = delta_residues(c)) return e;
    if (int e = pl_scratch(c, (size_t)items * Ln)) return e;
    launch_scale_plain(pt, delta ? c->d_delta : nullptr, c->pl_buf, items, c->n, c->L, c->d_primes, c->stream);
    CHECK_LAUNCH();
    return ntt_items(c, c->pl_buf, items, Ln, c->L);
}

extern "C" int exacto_bfv_plain_mul_dev(exacto_ctx* c, const uint64_t* ct, size_t polys, const uint64_t* pt,
                                        uint64_t* out, size_t B) {
    if (int e = check_ctx(c)) return e;
    if (!ct || !pt || !out) return invalid_param("null argument");
    if (polys == 0) return invalid_param("ciphertext has no components");
    if (B == 0) return 0;
    if (int e = lift_plain(c, pt, (long)B, false)) return e;
    const long Ln = (long)c->L * c->n;
    launch_plain_apply(PLAIN_MUL, ct, (long)polys * Ln, out, (long)B, (int)polys, c->pl_buf, Ln, c->n, c->L, c->d_primes,
                       c->stream);
    CHECK_LAUNCH();
    return 0;
}

extern "C" int exacto_bfv_plain_add_dev(exacto_ctx* c, const uint64_t* ct, size_t polys, const uint64_t* pt,
                                        uint64_t* out, size_t B) {
    if (int e = check_ctx(c)) return e;
    if (!ct || !pt || !out) return invalid_param("null argument");
    if (polys == 0) return invalid_param("ciphertext has no components");
    if (B == 0) return 0;
    if (int e = lift_plain(c, pt, (long)B, true)) return e;
    const long Ln = (long)c->L * c->n;
    launch_plain_apply(PLAIN_ADD, ct, (long)polys * Ln, out, (long)B, (int)polys, c->pl_buf, Ln, c->n, c->L, c->d_primes,
                       c->stream);
    CHECK_LAUNCH();
    return 0;
}

extern "C" int exacto_bfv_inner_product_dev(exacto_ctx* c, const uint64_t* cts, const uint64_t* pts, size_t K,
                                            size_t polys, uint64_t* out) {
    if (int e = check_ctx(c)) return e;
    if (K == 0) return invalid_param("mismatched ct/pt lengths");
    if (!cts || !pts || !out) return invalid_param("null argument");
    if (polys == 0) return invalid_param("ciphertext has no components");
    if (int e = lift_plain(c, pts, (long)K, false)) return e;
    launch_inner_product(cts, c->pl_buf, out, (int)K, (int)polys, c->n, c->L, c->d_primes, c->stream);
    CHECK_LAUNCH();
    return 0;
}

extern "C" int exacto_bfv_monomial_mul_dev(exacto_ctx* c, const uint64_t* ct, size_t polys, uint64_t j,
                                           uint64_t* out, size_t B) {
    if (int e = check_ctx(c)) return e;
    if (!ct || !out) return invalid_param("null argument");
    if (B == 0 || polys == 0) return 0;
    const long Ln = (long)c->L * c->n;
    j %= 2 * (u64)c->n;
    if (j == 0) {  // eval.rs:619-621: a clone
        if (out != ct)
            HIP_TRY(dev_copy(out, ct, B * polys * Ln * sizeof(u64), c->stream));
        return 0;
    }
    if (int e = pl_scratch(c, (size_t)Ln)) return e;
    launch_monomials(c->pl_buf, 1, j, false, c->n, c->L, c->d_primes, c->stream);
    CHECK_LAUNCH();
    if (int e = ntt_items(c, c->pl_buf, 1, 0, c->L)) return e;
    launch_plain_apply(PLAIN_MUL, ct, polys * Ln, out, (long)B, (int)polys, c->pl_buf, 0, c->n, c->L, c->d_primes,
                       c->stream);
    CHECK_LAUNCH();
    return 0;
}

// Trace accumulation over [B][2][L][n] in r: chain (src == nullptr): r += sigma_k(r) for each k in
// order (eval.rs:572-586, coeffs_to_slots.rs:65-75); naive: r += sigma_k(src) (coeffs_to_slots.rs:79-95).
// key e of ks lives at gks + kidx[e] * num_keys * 2Ln.
static int trace_core(exacto_ctx* c, const u64* src, u64* r, const std::vector<u64>& ks,
                      const std::vector<size_t>& kidx, const u64* gks, size_t num_keys, size_t B) {
    if (ks.empty()) return 0;
    const long Ln = (long)c->L * c->n;
    Scratch rs;
    HIP_TRY(rs.alloc(B * 2 * Ln * sizeof(u64), c->stream, c->pool, c->debug_scratch));
    u64* rot = rs.as<u64>();
    int rc = 0;
    for (size_t e = 0; e < ks.size() && rc == 0; ++e) {
        rc = exacto_bfv_apply_automorphism_dev(c, src ? src : r, 2, ks[e], gks + kidx[e] * num_keys * 2 * Ln,
                                               num_keys, rot, B);
        if (rc == 0) {
            launch_pointwise(PwOp::Add, r, rot, r, (long)B * 2 * c->L, c->n, c->L, nullptr, c->d_primes, c->stream);
            if (hipGetLastError() != hipSuccess) rc = fail(EXACTO_ERR_HIP, "HIP error: trace add launch");
        }
    }
    return rc;
}

// eval.rs:572-586 batched: result = ct; for k in elements: result += sigma_k(result).
// elements is a host array [E]; gks = [E][num_keys][2][L][n], the key of elements[e] at index e.
extern "C" int exacto_bfv_trace_dev(exacto_ctx* c, const uint64_t* ct, size_t polys, const uint64_t* elements,
                                    size_t E, const uint64_t* gks, size_t num_keys, uint64_t* out, size_t B) {
    if (int e = check_ctx(c)) return e;
    if (!ct || !out || (E && (!elements || !gks))) return invalid_param("null argument");
    if (B == 0) return 0;
    const long Ln = (long)c->L * c->n;
    if (out != ct) HIP_TRY(dev_copy(out, ct, B * polys * Ln * sizeof(u64), c->stream));
    if (E == 0) return 0;
    if (polys != 2) return invalid_param("automorphism requires degree-1 ciphertext");
    std::vector<u64> ks(elements, elements + E);
    std::vector<size_t> kidx(E);
    for (size_t e = 0; e < E; ++e) kidx[e] = e;
    return trace_core(c, nullptr, out, ks, kidx, gks, num_keys, B);
}

// coeffs_to_slots.rs:168-183
extern "C" size_t exacto_required_trace_elements(size_t n, uint64_t* out, size_t cap) {
    std::vector<u64> v;
    if (n <= 32 || (n & (n - 1))) {
        for (u64 k = 3; k < 2 * (u64)n; k += 2) v.push_back(k);
    } else {
        for (u64 step = n; step >= 2; step >>= 1) v.push_back(step + 1);
    }
    for (size_t i = 0; i < v.size() && i < cap && out; ++i) out[i] = v[i];
    return v.size();
}

// coeffs_to_slots.rs:21-49 for the coefficients j0 .. j0+J-1 of one ciphertext at once:
// out[t] = n^-1 * Tr(X^(2n-j) ct), j = j0 + t; the J shifted copies share every trace step.
extern "C" int exacto_extract_coefficients_dev(exacto_ctx* c, const uint64_t* ct, uint64_t j0, size_t J,
                                               const uint64_t* elements, size_t E, const uint64_t* gks,
                                               size_t num_keys, uint64_t* out) {
    if (int e = check_ctx(c)) return e;
    if (!ct || !out || (E && (!elements || !gks))) return invalid_param("null argument");
    if (J == 0) return 0;
    const int n = c->n;
    if (j0 + J - 1 > 2 * (u64)n) return invalid_param("coefficient index out of range");
    // resolve every key the trace needs first (HashMap lookups, coeffs_to_slots.rs:67-69, 87-89)
    std::vector<u64> ks(exacto_required_trace_elements(n, nullptr, 0));
    exacto_required_trace_elements(n, ks.data(), ks.size());
    std::vector<size_t> kidx(ks.size());
    for (size_t e = 0; e < ks.size(); ++e) {
        size_t f = 0;
        while (f < E && elements[f] != ks[e]) ++f;
        if (f == E) return invalid_param("missing Galois key for element " + std::to_string(ks[e]));
        kidx[e] = f;
    }
    // n^-1 mod t (coeffs_to_slots.rs:40-42)
    const u64 n_inv = invmod_h((u64)n % c->plain, c->plain);
    if (!n_inv) return invalid_param("n not invertible mod t");
    const long Ln = (long)c->L * n;
    const bool naive = n <= 32 || (n & (n - 1));
    // shifted copies X^(2n-j) ct: the monomial table [J][L][n] in the NTT domain, one broadcast product
    if (int e = pl_scratch(c, J * Ln)) return e;
    launch_monomials(c->pl_buf, (long)J, j0, true, n, c->L, c->d_primes, c->stream);
    CHECK_LAUNCH();
    if (int e = ntt_items(c, c->pl_buf, (long)J, Ln, c->L)) return e;
    Scratch ss;
    if (naive) HIP_TRY(ss.alloc(J * 2 * Ln * sizeof(u64), c->stream, c->pool, c->debug_scratch));
    u64* shifted = naive ? ss.as<u64>() : out;
    launch_plain_apply(PLAIN_MUL, ct, 0, shifted, (long)J, 2, c->pl_buf, Ln, n, c->L, c->d_primes, c->stream);
    int rc = hipGetLastError() == hipSuccess ? 0 : fail(EXACTO_ERR_HIP, "HIP error: monomial launch");
    if (rc == 0 && naive)
        rc = dev_copy(out, shifted, J * 2 * Ln * sizeof(u64), c->stream) == hipSuccess
                 ? 0 : fail(EXACTO_ERR_HIP, "HIP error: copy");
    if (rc == 0) rc = trace_core(c, naive ? shifted : nullptr, out, ks, kidx, gks, num_keys, J);
    if (rc) return rc;
    // times the constant plaintext n^-1: NTT(constant) is that constant in every slot
    return exacto_rns_scalar_mul_dev(c, out, n_inv, out, J * 2);
}

// coeffs_to_slots.rs:121-145: sum_j X^j slots[j], as one inner product against the monomial table
extern "C" int exacto_slots_to_coeffs_dev(exacto_ctx* c, const uint64_t* slots, size_t S, size_t polys,
                                          uint64_t* out) {
    if (int e = check_ctx(c)) return e;
    if (S == 0) return invalid_param("empty slots");
    if (S != (size_t)c->n)
        return invalid_param("expected " + std::to_string(c->n) + " slots, got " + std::to_string(S));
    if (!slots || !out) return invalid_param("null argument");
    if (polys == 0) return invalid_param("ciphertext has no components");
    const long Ln = (long)c->L * c->n;
    if (int e = pl_scratch(c, S * Ln)) return e;
    launch_monomials(c->pl_buf, (long)S, 0, false, c->n, c->L, c->d_primes, c->stream);
    CHECK_LAUNCH();
    if (int e = ntt_items(c, c->pl_buf, (long)S, Ln, c->L)) return e;
    launch_inner_product(slots, c->pl_buf, out, (int)S, (int)polys, c->n, c->L, c->d_primes, c->stream);
    CHECK_LAUNCH();
    return 0;
}

extern "C" int exacto_extract_coefficients(exacto_ctx* c, const uint64_t* ct, uint64_t j0, size_t J,
                                           const uint64_t* elements, size_t E, const uint64_t* gks, size_t num_keys,
                                           uint64_t* out) {
    if (!c) return invalid_param("null context");
    const size_t ctb = 2 * c->L * poly_bytes(c);
    return host_call(c, {{ct, ctb}, {gks, E * num_keys * ctb}}, J * ctb, out, [&](std::vector<u64*>& d, u64* o) {
        return exacto_extract_coefficients_dev(c, d[0], j0, J, elements, E, d[1], num_keys, o);
    });
}

extern "C" int exacto_slots_to_coeffs(exacto_ctx* c, const uint64_t* slots, size_t S, size_t polys, uint64_t* out) {
    if (!c) return invalid_param("null context");
    const size_t ctb = polys * c->L * poly_bytes(c);
    return host_call(c, {{slots, S * ctb}}, ctb, out, [&](std::vector<u64*>& d, u64* o) {
        return exacto_slots_to_coeffs_dev(c, d[0], S, polys, o);
    });
}

extern "C" int exacto_bfv_plain_mul(exacto_ctx* c, const uint64_t* ct, size_t polys, const uint64_t* pt,
                                    uint64_t* out, size_t B) {
    if (!c) return invalid_param("null context");
    const size_t ctb = B * polys * c->L * poly_bytes(c);
    return host_call(c, {{ct, ctb}, {pt, B * poly_bytes(c)}}, ctb, out, [&](std::vector<u64*>& d, u64* o) {
        return exacto_bfv_plain_mul_dev(c, d[0], polys, d[1], o, B);
    });
}

extern "C" int exacto_bfv_plain_add(exacto_ctx* c, const uint64_t* ct, size_t polys, const uint64_t* pt,
                                    uint64_t* out, size_t B) {
    if (!c) return invalid_param("null context");
    const size_t ctb = B * polys * c->L * poly_bytes(c);
    return host_call(c, {{ct, ctb}, {pt, B * poly_bytes(c)}}, ctb, out, [&](std::vector<u64*>& d, u64* o) {
        return exacto_bfv_plain_add_dev(c, d[0], polys, d[1], o, B);
    });
}

extern "C" int exacto_bfv_inner_product(exacto_ctx* c, const uint64_t* cts, const uint64_t* pts, size_t K,
                                        size_t polys, uint64_t* out) {
    if (!c) return invalid_param("null context");
    if (K == 0) return invalid_param("mismatched ct/pt lengths");
    const size_t ctb = polys * c->L * poly_bytes(c);
    return host_call(c, {{cts, K * ctb}, {pts, K * poly_bytes(c)}}, ctb, out, [&](std::vector<u64*>& d, u64* o) {
        return exacto_bfv_inner_product_dev(c, d[0], d[1], K, polys, o);
    });
}

extern "C" int exacto_bfv_monomial_mul(exacto_ctx* c, const uint64_t* ct, size_t polys, uint64_t j, uint64_t* out,
                                       size_t B) {
    if (!c) return invalid_param("null context");
    const size_t ctb = B * polys * c->L * poly_bytes(c);
    return host_call(c, {{ct, ctb}}, ctb, out, [&](std::vector<u64*>& d, u64* o) {
        return exacto_bfv_monomial_mul_dev(c, d[0], polys, j, o, B);
    });
}

extern "C" int exacto_bfv_trace(exacto_ctx* c, const uint64_t* ct, size_t polys, const uint64_t* elements, size_t E,
                                const uint64_t* gks, size_t num_keys, uint64_t* out, size_t B) {
    if (!c) return invalid_param("null context");
    const size_t ctb = B * polys * c->L * poly_bytes(c);
    return host_call(c, {{ct, ctb}, {gks, E * num_keys * 2 * c->L * poly_bytes(c)}}, ctb, out,
                     [&](std::vector<u64*>& d, u64* o) {
                         return exacto_bfv_trace_dev(c, d[0], polys, elements, E, d[1], num_keys, o, B);
                     });
}

// ---- digit extraction pieces (bootstrap/digit_extract.rs) ----

// lagrange_interpolate (digit_extract.rs:37-90): the Lagrange formula at the points 0..n-1 over Z_p.
// The numerator prod_{k != j} (x - k) is the master polynomial prod_k (x - k) divided by the monic
// (x - j) -- exact over Z, so reducing mod p commutes -- which makes it O(n^2) instead of O(n^3)
// with the same coefficients; the denominators prod_{k != j} (j - k) are the reference's.
extern "C" int exacto_lagrange_interpolate(const uint64_t* values, size_t n, uint64_t p, uint64_t* out) {
    if (n == 0) return 0;
    if (!values || !out) return invalid_param("null argument");
    if (p == 0) return invalid_param("modulus must be nonzero");
    if (n == 1) { out[0] = values[0] % p; return 0; }
    auto mulm = [p](u64 a, u64 b) { return (u64)((u128)a * b % p); };
    auto addm = [p](u64 a, u64 b) { return (u64)(((u128)a + b) % p); };
    // master[d], degree n: prod_{k=0}^{n-1} (x - k)
    std::vector<u64> master(n + 1, 0), num(n), res(n, 0);
    master[0] = 1 % p;
    for (size_t k = 0; k < n; ++k) {
        const u64 neg_k = (p - (u64)k % p) % p;
        for (size_t d = k + 2; d-- > 0;) {  // d = k+1 .. 0
            const u64 lower = d ? master[d - 1] : 0;
            master[d] = addm(lower, mulm(master[d], neg_k));
        }
    }
    for (size_t j = 0; j < n; ++j) {
        if (values[j] % p == 0) continue;
        // synthetic division of master by (x - j): num[n-1] = master[n], num[d-1] = master[d] + j num[d]
        const u64 jm = (u64)j % p;
        num[n - 1] = master[n];
        for (size_t d = n - 1; d >= 1; --d) num[d - 1] = addm(master[d], mulm(jm, num[d]));
        u64 denom = 1 % p;
        for (size_t k = 0; k < n; ++k) {
            if (k == j) continue;
            const u64 diff = j >= k ? (u64)(j - k) % p : (p - (u64)(k - j) % p) % p;
            denom = mulm(denom, diff);
        }
        const u64 dinv = invmod_h(denom, p);
        if (!dinv) return invalid_param("points must be distinct mod p");
        const u64 scale = mulm(values[j] % p, dinv);
        for (size_t d = 0; d < n; ++d) res[d] = addm(res[d], mulm(num[d], scale));
    }
    std::copy(res.begin(), res.end(), out);
    return 0;
}

// compute_rounding_poly (digit_extract.rs:19-30): g(x) = round(t_orig (x mod q') / q') mod t_orig
// on x in [0, t_boot), interpolated over Z_{t_boot}; out has t_boot coefficients.
extern "C" int exacto_compute_rounding_poly(uint64_t t_orig, uint64_t q_prime, uint64_t t_boot, uint64_t* out) {
    if (!out) return invalid_param("null argument");
    if (q_prime == 0 || t_orig == 0) return invalid_param("moduli must be nonzero");
    std::vector<u64> v(t_boot);
    for (u64 x = 0; x < t_boot; ++x) {
        const u128 reduced = x % q_prime;
        v[x] = (u64)(((u128)t_orig * reduced + q_prime / 2) / q_prime % t_orig);
    }
    return exacto_lagrange_interpolate(v.data(), t_boot, t_boot, out);
}

// trivial_encrypt_poly (digit_extract.rs:179-189): (Delta m, 0), m = pt [B][n] as given
extern "C" int exacto_trivial_encrypt_dev(exacto_ctx* c, const uint64_t* pt, uint64_t* out, size_t B) {
    if (int e = check_ctx(c)) return e;
    if (!pt || !out) return invalid_param("null argument");
    if (B == 0) return 0;
    const long Ln = (long)c->L * c->n;
    if (int e = lift_plain(c, pt, (long)B, true)) return e;
    launch_rows(out, 2 * Ln, c->pl_buf, Ln, Ln, (long)B, c->stream);
    launch_rows(out + Ln, 2 * Ln, nullptr, 0, Ln, (long)B, c->stream);
    CHECK_LAUNCH();
    return 0;
}

// eval_poly_homomorphic (digit_extract.rs:101-157), batched: the same polynomial on B ciphertexts.
// Paterson-Stockmeyer with the reference's schedule: baby steps x^i = x^(i/2) * x^(i - i/2) for
// i = 2..k (even i on the one-operand square pipeline), k = max(2, ceil(sqrt(d + 1))); groups g_i = sum_j a_{ik+j} x^j (trivial(0) + scalar
// multiples, coefficients reduced mod t as bfv_scalar_mul does); Horner in x^k.  Uses the context's
// resident relinearisation key for every bfv_mul_and_relin.
extern "C" int exacto_eval_poly_dev(exacto_ctx* c, const uint64_t* ct, const uint64_t* coeffs, size_t m,
                                    uint64_t* out, size_t B) {
    if (int e = check_ctx(c)) return e;
    if (m == 0) return invalid_param("empty polynomial");
    if (!ct || !out || !coeffs) return invalid_param("null argument");
    if (B == 0) return 0;
    if (int e = delta_residues(c)) return e;
    const long Ln = (long)c->L * c->n;
    const size_t words = B * 2 * Ln;
    const size_t d = m - 1;
    const u64 t = c->plain;
    if (d == 0) {  // digit_extract.rs:109-111: trivial_encrypt(a_0)
        launch_trivial_const(out, (long)B, coeffs[0] % t, c->d_delta, c->n, c->L, c->d_primes, c->stream);
        CHECK_LAUNCH();
        return 0;
    }
    if (!c->rlk_loaded) return fail(EXACTO_ERR_MISSING_KEY, "key not available: relinearization key not loaded");
    const size_t k = std::max<size_t>(2, (size_t)std::ceil(std::sqrt((double)d + 1.0)));
    const size_t groups = (d + k) / k;
    // workspace: baby[0], baby[2..k] (baby[1] is ct), one group accumulator, a Horner ping buffer
    const size_t nbuf = k + 3;
    Scratch wss;
    HIP_TRY(wss.alloc(nbuf * words * sizeof(u64), c->stream, c->pool, c->debug_scratch));
    u64* ws = wss.as<u64>();
    std::vector<const u64*> baby(k + 1);
    auto slot = [&](size_t i) { return ws + i * words; };
    baby[0] = slot(0);
    baby[1] = ct;
    u64* acc = slot(k + 1);
    u64* ping = slot(k + 2);
    int rc = 0;
    launch_trivial_const(slot(0), (long)B, 1 % t, c->d_delta, c->n, c->L, c->d_primes, c->stream);
    if (hipGetLastError() != hipSuccess) rc = fail(EXACTO_ERR_HIP, "HIP error: trivial launch");
    for (size_t i = 2; i <= k && rc == 0; ++i) {
        const size_t half = i / 2;
        // (even i: a square, bit for bit the product of baby[half] with itself)
        rc = (i - half == half && c->square_hook)
                 ? exacto_bfv_square_and_relin_dev(c, baby[half], slot(i), B)
                 : exacto_bfv_mul_and_relin_dev(c, baby[half], baby[i - half], slot(i), B);
        baby[i] = slot(i);
    }
    // group g_i into `dst`: trivial(0) + sum_j (a mod t) x^j
    auto group = [&](size_t gi, u64* dst) -> int {
        launch_fill_u32(reinterpret_cast<uint32_t*>(dst), 0, (long)(2 * words), c->stream);   // (see dev_copy)
        HIP_TRY(hipGetLastError());
        for (size_t j = 0; j < k; ++j) {
            const size_t idx = gi * k + j;
            if (idx >= m) break;
            if (coeffs[idx] == 0) continue;
            launch_axpy(dst, baby[j], coeffs[idx] % t, (long)B * 2 * c->L, c->n, c->L, c->d_primes, c->stream);
            CHECK_LAUNCH();
        }
        return 0;
    };
    // Horner from the last group; the running result alternates between out and ping
    u64* res = ((groups - 1) % 2 == 0) ? out : ping;  // so that the final result lands in out
    u64* other = res == out ? ping : out;
    if (rc == 0) rc = group(groups - 1, res);
    for (size_t gi = groups - 1; gi-- > 0 && rc == 0;) {
        rc = exacto_bfv_mul_and_relin_dev(c, res, baby[k], other, B);
        if (rc == 0) rc = group(gi, acc);
        if (rc == 0) {
            launch_pointwise(PwOp::Add, other, acc, other, (long)B * 2 * c->L, c->n, c->L, nullptr, c->d_primes,
                             c->stream);
            if (hipGetLastError() != hipSuccess) rc = fail(EXACTO_ERR_HIP, "HIP error: add launch");
        }
        std::swap(res, other);
    }
    return rc;
}

// ---- bootstrap composition (bootstrap/bfv_host.rs) ----

static int boot_pair_check(exacto_ctx* o, exacto_ctx* b) {
    if (int e = check_ctx(o)) return e;
    if (int e = check_ctx(b)) return e;
    if (o->n != b->n) return invalid_param("boot params must have same ring degree");
    if (o->device != b->device) return invalid_param("both contexts must be on one device");
    // the reference switches from q = moduli[0] after to_coeff_poly, which only holds one residue
    // system when L = 1 (bfv_host.rs:149-157): multi-prime originals are not supported
    if (o->L != 1) return invalid_param("bootstrap requires a single-prime ciphertext modulus");
    return 0;
}

// The bootstrap functions work on two contexts.  They run every step of both on ONE stream (the
// boot context's): o's stream is rebound to b's for the call, so that every hand-off between the
// contexts (the inputs uploaded on b's stream and copied on o's, the modulus-switched rows written on
// o's and read on b's) is ordered by the runtime instead of by host-side synchronisation alone.
// (Made while chasing an intermittent failure of the C++ test's bootstrap case)
struct StreamRebind {
    exacto_ctx* c;
    hipStream_t saved;
    StreamRebind(exacto_ctx* c_, hipStream_t s) : c(c_), saved(c_->stream) {
        if (saved != s) (void)hipStreamSynchronize(saved);
        c->stream = s;
    }
    ~StreamRebind() {
        if (c->stream != saved) (void)hipStreamSynchronize(c->stream);
        c->stream = saved;
    }
};

// gen_bootstrap_key's key material (bfv_host.rs:57-100, 289-330): the boot scheme's secret key
// boot_sk [Lb][n] (NTT domain, create_boot_sk) and the plaintext s_pt [n] that bsk encrypts.
extern "C" int exacto_bootstrap_key_material_dev(exacto_ctx* o, exacto_ctx* b, const uint64_t* sk, uint64_t* boot_sk,
                                                 uint64_t* s_pt) {
    if (int e = boot_pair_check(o, b)) return e;
    if (!sk || !boot_sk || !s_pt) return invalid_param("null argument");
    const int n = o->n;
    StreamRebind one(o, b->stream);   // before the scratch: its block is freed on b's stream
    Scratch ts;
    HIP_TRY(ts.alloc(2 * n * sizeof(u64), o->stream, o->pool, o->debug_scratch));
    u64* tmp = ts.as<u64>();
    HIP_TRY(dev_copy(tmp, sk, n * sizeof(u64), o->stream));
    int rc = run_ntt(o, contiguous(tmp, 1, 1, 0, 1, n), 1, true);  // sk.poly.components[0].to_coeff_poly()
    if (rc == 0) {
        launch_boot_key_map(tmp, tmp + n, s_pt, n, o->primes[0], b->primes[0], b->plain, o->stream);
        rc = hipGetLastError() == hipSuccess ? 0 : fail(EXACTO_ERR_HIP, "HIP error: key map launch");
    }
    if (rc == 0) rc = hipStreamSynchronize(o->stream) == hipSuccess ? 0 : fail(EXACTO_ERR_HIP, "HIP error: sync");
    if (rc == 0) {  // RnsPoly::from_coeff_poly over the boot basis, then its NTT
        launch_scale_plain(tmp + n, nullptr, boot_sk, 1, n, b->L, b->d_primes, b->stream);
        rc = hipGetLastError() == hipSuccess ? 0 : fail(EXACTO_ERR_HIP, "HIP error: lift launch");
    }
    if (rc == 0) rc = ntt_items(b, boot_sk, 1, 0, b->L);
    // tmp + n was read on b's stream: both streams drain before the block returns to o's pool
    const hipError_t sb = hipStreamSynchronize(b->stream), so = hipStreamSynchronize(o->stream);
    if (rc == 0 && (sb != hipSuccess || so != hipSuccess)) rc = fail(EXACTO_ERR_HIP, "HIP error: sync");
    return rc;
}

// EXACTO_DEBUG_BOOT=1: the diagnostic of DESIGN.md §3's intermittent bootstrap result.  snap()
// copies the first words of an intermediate into a debug buffer on the stream as the call runs;
// xsnap() reads a block from 16 workgroups spread over the XCDs, each recording its XCD; dump()
// prints both to stderr after the call's final synchronisation.  Off: every call is a no-op.
struct BootDebug {
    static constexpr int DW = 64, DN = 16, XB = 16, XN = 4;
    hipStream_t s;
    bool on;
    u64* dbuf = nullptr;
    u64* xbuf = nullptr;
    uint32_t* xcc = nullptr;
    uint32_t* whit = nullptr;   // write-watch flags (kernels.hip DbgWatch)
    std::vector<std::pair<std::string, size_t>> names;
    std::vector<std::string> xnames;
    explicit BootDebug(hipStream_t st) : s(st) {
        static const bool env = [] { const char* e = getenv("EXACTO_DEBUG_BOOT"); return e && e[0] == '1'; }();
        on = env && hipMalloc((void**)&dbuf, DN * DW * sizeof(u64)) == hipSuccess &&
             hipMalloc((void**)&xbuf, XN * XB * 4 * sizeof(u64)) == hipSuccess &&
             hipMalloc((void**)&xcc, XN * XB * sizeof(uint32_t)) == hipSuccess &&
             hipMalloc((void**)&whit, 8 * sizeof(uint32_t)) == hipSuccess;
        if (on) launch_fill_u32(whit, 0, 8, s);
    }
    ~BootDebug() {
        if (dbuf || xbuf || xcc || whit) (void)hipStreamSynchronize(s);
        // (raw, like the hipMalloc above: the diagnostic's own blocks stay out of the allocation log)
        (void)hipFree(dbuf); (void)hipFree(xbuf); (void)hipFree(xcc); (void)hipFree(whit);
    }
    // null source (an earlier allocation failed; the call's rc carries the real error): skipped, so the
    // diagnostic never faults the GPU and hides that error
    void snap(const std::string& name, const u64* p, size_t words) {
        if (!on || !p || names.size() >= (size_t)DN) return;
        const size_t w = std::min<size_t>(words, DW);
        launch_copy_u64(dbuf + names.size() * DW, p, (long)w, s);
        names.emplace_back(name, w);
    }
    void xsnap(const std::string& name, const u64* p) {
        if (!on || !p || xnames.size() >= (size_t)XN) return;
        launch_xcd_probe(p, xbuf + xnames.size() * XB * 4, 4, xcc + xnames.size() * XB, XB, s);
        xnames.push_back(name);
    }
    void dump() {
        if (!on) return;
        std::vector<u64> h(DN * DW), hx(XN * XB * 4);
        std::vector<uint32_t> hc(XN * XB);
        (void)hipMemcpyAsync(h.data(), dbuf, h.size() * sizeof(u64), hipMemcpyDeviceToHost, s);
        (void)hipMemcpyAsync(hx.data(), xbuf, hx.size() * sizeof(u64), hipMemcpyDeviceToHost, s);
        (void)hipMemcpyAsync(hc.data(), xcc, hc.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, s);
        (void)hipStreamSynchronize(s);
        for (size_t i = 0; i < xnames.size(); ++i) {
            std::string line = "boot-dbg xcd " + xnames[i] + ":";
            for (int k = 0; k < XB; ++k)
                line += " x" + std::to_string(hc[i * XB + k]) + "=" + std::to_string(hx[(i * XB + k) * 4]);
            std::fprintf(stderr, "%s\n", line.c_str());
        }
        for (size_t i = 0; i < names.size(); ++i) {
            u64 hsh = 1469598103934665603ull;   // FNV-1a of the snapshot
            for (size_t k = 0; k < names[i].second; ++k) hsh = (hsh ^ h[i * DW + k]) * 1099511628211ull;
            std::fprintf(stderr, "boot-dbg %-14s %016llx [%llu %llu %llu %llu]\n", names[i].first.c_str(),
                         (unsigned long long)hsh, (unsigned long long)h[i * DW], (unsigned long long)h[i * DW + 1],
                         (unsigned long long)h[i * DW + 2], (unsigned long long)h[i * DW + 3]);
        }
    }
};

// bfv_bootstrap (bfv_host.rs:131-205) on B ciphertexts of the original scheme (ct [B][2][1][n] on
// o) -> out [B][2][Lb][n] on b.  bsk [2][Lb][n] is the encryption of s under b; the boot
// relinearisation key must be resident in b; (elements, gks) are the trace keys as in
// exacto_extract_coefficients; rpoly [m] (host) the rounding polynomial.  Items whose c1 is zero
// take the reference's trivial fast path, the others the full ring path.
extern "C" int exacto_bfv_bootstrap_dev(exacto_ctx* o, exacto_ctx* b, const uint64_t* ct, size_t polys,
                                        const uint64_t* bsk, const uint64_t* rpoly, size_t m, uint64_t q_prime,
                                        const uint64_t* elements, size_t E, const uint64_t* gks, size_t num_keys,
                                        uint64_t* out, size_t B) {
    if (int e = boot_pair_check(o, b)) return e;
    if (polys != 2) return invalid_param("bootstrap requires degree-1 ciphertext");
    if (!ct || !bsk || !out || !rpoly) return invalid_param("null argument");
    if (q_prime == 0) return invalid_param("q_prime must be nonzero");
    if (B == 0) return 0;
    const int n = o->n;
    const long Lbn = (long)b->L * n;
    StreamRebind one(o, b->stream);
    // The call's intermediates live in b's persistent buffers (boot_buf: coefficients, flags, the
    // c0'/c1' rows, phase; boot_slots: the ring path's slots), grown like the workspaces and never
    // taken from the stream-ordered pool (round 4-5's zeros appeared in pool blocks).
    // Both streams drain before the call returns (`drain`, on every return path; the normal path calls
    // finish() to fold a failed synchronisation, e.g. a kernel fault, into the return code).
    const size_t ctw = 2 * Lbn;
    const size_t w_coef = 2 * B * 2 * n, w_flags = (B + 1) / 2, w_c0pt = 2 * B * n;
    if (b->boot_buf.grow((w_coef + w_flags + w_c0pt + ctw) * sizeof(u64))) return EXACTO_ERR_HIP;
    int rc = 0;
    struct Drain {
        exacto_ctx *o, *b;
        bool done = false;
        int finish(int code) {
            done = true;
            const hipError_t sb = hipStreamSynchronize(b->stream), so = hipStreamSynchronize(o->stream);
            if (code == 0 && (sb != hipSuccess || so != hipSuccess)) return fail(EXACTO_ERR_HIP, "HIP error: sync");
            return code;
        }
        ~Drain() {
            if (!done) finish(1);
        }
    } drain{o, b};
    auto ok = [&](hipError_t e, const char* what) {
        if (rc == 0 && e != hipSuccess) rc = fail(EXACTO_ERR_HIP, std::string("HIP error: ") + what);
    };
    BootDebug dbg(b->stream);
    // 1. to coefficients (o), modulus switch to q' and reduce mod t_boot; c1 == 0 flags
    u64* coef = b->boot_buf;
    int* flags = reinterpret_cast<int*>(coef + w_coef);
    u64* small = coef + B * 2 * n;
    dbg.snap("ct", ct, B * 2 * n);
    ok(dev_copy(coef, ct, B * 2 * n * sizeof(u64), o->stream), "copy");
    launch_fill_u32(reinterpret_cast<uint32_t*>(flags), 0, (long)B, o->stream);   // (see dev_copy)
    ok(hipGetLastError(), "flags fill");
    dbg.snap("coef", coef, B * 2 * n);
    if (rc == 0) rc = exacto_rns_inv_dev(o, coef, B * 2);
    dbg.snap("coef_inv", coef, B * 2 * n);
    if (rc == 0) {
        launch_modswitch(coef, small, flags, (long)B, n, o->primes[0], q_prime, b->plain, o->stream);
        ok(hipGetLastError(), "modswitch launch");
    }
    dbg.snap("small", small, B * 2 * n);
    std::vector<int> hflags(B);
    if (rc == 0) ok(hipMemcpyAsync(hflags.data(), flags, B * sizeof(int), hipMemcpyDeviceToHost, o->stream), "flags");
    if (rc == 0) ok(hipStreamSynchronize(o->stream), "sync");
    // 2. phase = TrivialEnc(c0') + bsk * c1' (b), written into out
    // [B][n] copies of c0' and c1' rows in the plaintext layout
    u64* c0pt = coef + w_coef + w_flags;
    u64* c1pt = c0pt + B * n;
    // debug: the library's generic writers (rows / copy / fill kernels) report writes into c0pt and
    // c1pt from here to the end of the call (the rows copies below are the expected ones, kind 0)
    // EXACTO_DEBUG_WATCH=1: the watch alone, its flag buffer allocated once per process (the least
    // perturbing diagnostic: the snapshots' per-call allocations made the failure disappear in round 5)
    static uint32_t* watch_hit = [] {
        uint32_t* p = nullptr;
        const char* e = getenv("EXACTO_DEBUG_WATCH");
        if (e && e[0] == '1' && hipMalloc((void**)&p, 8 * sizeof(uint32_t)) == hipSuccess &&
            hipMemset(p, 0, 8 * sizeof(uint32_t)) == hipSuccess && hipDeviceSynchronize() == hipSuccess)
            return p;
        return (uint32_t*)nullptr;
    }();
    uint32_t* whit = dbg.on ? dbg.whit : watch_hit;
    if (whit && rc == 0) debug_watch_set(c0pt, c0pt + 2 * B * n, whit, b->stream);
    dbg.snap("small_again", small, B * 2 * n);
    dbg.xsnap("small", small);
    dbg.xsnap("c0pt_before", c0pt);
    if (rc == 0) {
        launch_rows(c0pt, n, small, 2 * n, n, (long)B, b->stream);
        launch_rows(c1pt, n, small + n, 2 * n, n, (long)B, b->stream);
        ok(hipGetLastError(), "copy c0/c1");
    }
    dbg.snap("c0pt_copied", c0pt, B * n);
    dbg.xsnap("c0pt_after", c0pt);
    if (rc == 0) rc = lift_plain(b, c1pt, (long)B, false);
    dbg.snap("c0pt_lift1", c0pt, B * n);
    if (rc == 0) {
        launch_plain_apply(PLAIN_MUL, bsk, 0, out, (long)B, 2, b->pl_buf, Lbn, n, b->L, b->d_primes, b->stream);
        ok(hipGetLastError(), "plain_mul launch");
    }
    if (rc == 0) rc = lift_plain(b, c0pt, (long)B, true);
    if (rc == 0) {
        launch_plain_apply(PLAIN_ADD, out, 2 * Lbn, out, (long)B, 2, b->pl_buf, Lbn, n, b->L, b->d_primes,
                           b->stream);
        ok(hipGetLastError(), "plain_add launch");
    }
    dbg.snap("c0pt", c0pt, B * n);
    dbg.snap("phase_out", out, B * 2 * Lbn);
    // 3. per item: rounding polynomial directly (trivial) or CoeffsToSlots -> g -> SlotsToCoeffs
    u64* phase = c0pt + w_c0pt;
    u64 *slots = nullptr, *rounded = nullptr;
    for (size_t i = 0; i < B && rc == 0; ++i) {
        u64* oi = out + i * ctw;
        ok(dev_copy(phase, oi, ctw * sizeof(u64), b->stream), "copy");
        if (rc) break;
        dbg.snap("phase" + std::to_string(i), phase, ctw);
        if (!hflags[i]) {  // bfv_host.rs:180-186
            rc = exacto_eval_poly_dev(b, phase, rpoly, m, oi, 1);
            dbg.snap("result" + std::to_string(i), oi, ctw);
            continue;
        }
        if (!slots) {  // once per call, on the first item that takes the ring path
            if (b->boot_slots.bytes() < 2 * (size_t)n * ctw * sizeof(u64)) ok(hipStreamSynchronize(b->stream), "sync");
            if (rc == 0 && b->boot_slots.grow(2 * (size_t)n * ctw * sizeof(u64))) rc = EXACTO_ERR_HIP;
            if (rc) break;
            slots = b->boot_slots;
            rounded = slots + (size_t)n * ctw;
        }
        rc = exacto_extract_coefficients_dev(b, phase, 0, n, elements, E, gks, num_keys, slots);
        if (rc == 0) rc = exacto_eval_poly_dev(b, slots, rpoly, m, rounded, n);
        if (rc == 0) rc = exacto_slots_to_coeffs_dev(b, rounded, n, 2, oi);
    }
    rc = drain.finish(rc);
    dbg.dump();
    if (whit) {
        debug_watch_set(nullptr, nullptr, nullptr);
        uint32_t hh[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        (void)hipMemcpy(hh, whit, sizeof(hh), hipMemcpyDeviceToHost);
        (void)hipMemset(whit, 0, sizeof(hh));
        uint32_t hits = 0;
        for (int k = 0; k < 8; ++k) hits |= hh[k] ? (1u << k) : 0;
        std::fprintf(stderr, "boot-dbg watch c0pt=%p..%p hits=0x%x (bit k: 0 rows copy, 1 rows zero, 2 copy_u64, "
                     "3 fill 0, 4 fill other)\n", (void*)c0pt, (void*)(c0pt + 2 * B * n), hits);
    }
    if (dbg.on) {
        std::fprintf(stderr, "boot-dbg ptrs coef=%p small=%p flags=%p c0pt=%p out=%p o.pool=%p b.pool=%p o.stream=%p "
                     "b.stream=%p\n", (void*)coef, (void*)small, (void*)flags, (void*)c0pt, (void*)out, (void*)o->pool,
                     (void*)b->pool, (void*)o->stream, (void*)b->stream);
    }
    return rc;
}

extern "C" int exacto_bootstrap_key_material(exacto_ctx* o, exacto_ctx* b, const uint64_t* sk, uint64_t* boot_sk,
                                             uint64_t* s_pt) {
    if (!o || !b) return invalid_param("null context");
    if (int e = boot_pair_check(o, b)) return e;
    const size_t n = o->n;
    DevBuf<u64> d;
    if (int e = d.alloc((n + b->L * n + n) * sizeof(u64))) return e;
    int rc = upload(o, d, sk, n * sizeof(u64));
    if (rc == 0) rc = exacto_bootstrap_key_material_dev(o, b, d, d + n, d + n + b->L * n);
    if (rc == 0 && (hipMemcpyAsync(boot_sk, d + n, b->L * n * sizeof(u64), hipMemcpyDeviceToHost, o->stream) != hipSuccess ||
                    hipMemcpyAsync(s_pt, d + n + b->L * n, n * sizeof(u64), hipMemcpyDeviceToHost, o->stream) != hipSuccess ||
                    hipStreamSynchronize(o->stream) != hipSuccess))
        rc = fail(EXACTO_ERR_HIP, "HIP error: copy back");
    return rc;
}

extern "C" int exacto_bfv_bootstrap(exacto_ctx* o, exacto_ctx* b, const uint64_t* ct, size_t polys,
                                    const uint64_t* bsk, const uint64_t* rpoly, size_t m, uint64_t q_prime,
                                    const uint64_t* elements, size_t E, const uint64_t* gks, size_t num_keys,
                                    uint64_t* out, size_t B) {
    if (!o || !b) return invalid_param("null context");
    if (int e = boot_pair_check(o, b)) return e;
    if (polys != 2) return invalid_param("bootstrap requires degree-1 ciphertext");
    const size_t ctb = 2 * b->L * poly_bytes(b);
    return host_call(b, {{ct, B * 2 * o->L * poly_bytes(o)}, {bsk, ctb}, {gks, E * num_keys * ctb}}, B * ctb, out,
                     [&](std::vector<u64*>& d, u64* dout) {
                         return exacto_bfv_bootstrap_dev(o, b, d[0], polys, d[1], rpoly, m, q_prime, elements, E,
                                                         d[2], num_keys, dout, B);
                     });
}

extern "C" int exacto_trivial_encrypt(exacto_ctx* c, const uint64_t* pt, uint64_t* out, size_t B) {
    if (!c) return invalid_param("null context");
    return host_call(c, {{pt, B * poly_bytes(c)}}, B * 2 * c->L * poly_bytes(c), out,
                     [&](std::vector<u64*>& d, u64* o) { return exacto_trivial_encrypt_dev(c, d[0], o, B); });
}

extern "C" int exacto_eval_poly(exacto_ctx* c, const uint64_t* ct, const uint64_t* coeffs, size_t m, uint64_t* out,
                                size_t B) {
    if (!c) return invalid_param("null context");
    const size_t ctb = B * 2 * c->L * poly_bytes(c);
    return host_call(c, {{ct, ctb}}, ctb, out,
                     [&](std::vector<u64*>& d, u64* o) { return exacto_eval_poly_dev(c, d[0], coeffs, m, o, B); });
}

// Host-pointer variants (synchronous); `key` is always a host pointer to 4 words.
extern "C" int exacto_gen_secret_key(exacto_ctx* c, const uint64_t* key, uint64_t stream, uint64_t* sk) {
    if (!c) return invalid_param("null context");
    return host_call(c, {}, c->L * poly_bytes(c), sk,
                     [&](std::vector<u64*>&, u64* o) { return exacto_gen_secret_key_dev(c, key, stream, o); });
}

extern "C" int exacto_gen_public_key(exacto_ctx* c, const uint64_t* sk, double sigma, const uint64_t* key,
                                     uint64_t stream, uint64_t* pk) {
    if (!c) return invalid_param("null context");
    return host_call(c, {{sk, c->L * poly_bytes(c)}}, 2 * c->L * poly_bytes(c), pk, [&](std::vector<u64*>& d, u64* o) {
        return exacto_gen_public_key_dev(c, d[0], sigma, key, stream, o);
    });
}

extern "C" int exacto_gen_relin_key(exacto_ctx* c, const uint64_t* sk, double sigma, const uint64_t* key,
                                    uint64_t stream, size_t num_keys, uint64_t* rlk) {
    if (!c) return invalid_param("null context");
    if (!rlk) {  // resident key only: stage the secret key, generate in place
        return host_call(c, {{sk, c->L * poly_bytes(c)}}, 0, nullptr, [&](std::vector<u64*>& d, u64*) {
            return exacto_gen_relin_key_dev(c, d[0], sigma, key, stream, num_keys, nullptr);
        });
    }
    return host_call(c, {{sk, c->L * poly_bytes(c)}}, num_keys * 2 * c->L * poly_bytes(c), rlk,
                     [&](std::vector<u64*>& d, u64* o) {
                         return exacto_gen_relin_key_dev(c, d[0], sigma, key, stream, num_keys, o);
                     });
}

extern "C" int exacto_encrypt_sk(exacto_ctx* c, const uint64_t* pt, const uint64_t* sk, double sigma,
                                 const uint64_t* key, uint64_t stream, uint64_t* ct, size_t B) {
    if (!c) return invalid_param("null context");
    return host_call(c, {{pt, B * poly_bytes(c)}, {sk, c->L * poly_bytes(c)}}, B * 2 * c->L * poly_bytes(c), ct,
                     [&](std::vector<u64*>& d, u64* o) {
                         return exacto_encrypt_sk_dev(c, d[0], d[1], sigma, key, stream, o, B);
                     });
}

extern "C" int exacto_encrypt_pk(exacto_ctx* c, const uint64_t* pt, const uint64_t* pk, double sigma,
                                 const uint64_t* key, uint64_t stream, uint64_t* ct, size_t B) {
    if (!c) return invalid_param("null context");
    return host_call(c, {{pt, B * poly_bytes(c)}, {pk, 2 * c->L * poly_bytes(c)}}, B * 2 * c->L * poly_bytes(c), ct,
                     [&](std::vector<u64*>& d, u64* o) {
                         return exacto_encrypt_pk_dev(c, d[0], d[1], sigma, key, stream, o, B);
                     });
}

// ============================================================== SIMD batching (replaces bfv/encoding.rs)
// Slot encode / decode mod t (batch.hip), row rotations and the encode + encrypt / decrypt + decode
// compositions.  The convention is in include/exacto_hip.h.

// The first batching call of a context validates (n, t) and builds the tables; a context that cannot
// batch gives the same error at every batching call and is otherwise untouched.
static int batch_ready(exacto_ctx* c) {
    if (c->batch_state == 1) return 0;
    if (c->batch_state < 0) return fail(c->batch_code, c->batch_msg);
    const u64 t = c->plain;
    const int n = c->n, logn = c->logn;
    auto cannot = [&](int code, const std::string& msg) {
        c->batch_state = -1;
        c->batch_code = code;
        c->batch_msg = msg;
        return fail(code, msg);
    };
    if (n < 16 || n > 16384 || t < 2 || (t - 1) % (2 * (u64)n) != 0 || !is_prime_h(t))
        return cannot(EXACTO_ERR_INVALID_PARAM,
                      "invalid parameter: batching requires a prime plaintext modulus t ≡ 1 (mod 2n), got t=" +
                          std::to_string(t) + ", n=" + std::to_string(n));
    if (t >= (1ull << 32))
        return cannot(EXACTO_ERR_NOT_IMPLEMENTED, "not yet implemented: batching for plaintext moduli >= 2^32");
    const u64 zeta = find_psi((u64)n, t), zeta_inv = invmod_h(zeta, t);
    auto sh32 = [](u64 w, u64 p) { return (uint32_t)((w << 32) / p); };
    std::vector<uint2> tw((size_t)2 * n);
    for (int i = 0; i < n; ++i) {
        const int e = bitrev(i, logn);
        const u64 w = powmod_h(zeta, e, t), wi = powmod_h(zeta_inv, e, t);
        tw[i] = make_uint2((uint32_t)w, sh32(w, t));
        tw[(size_t)n + i] = make_uint2((uint32_t)wi, sh32(wi, t));
    }
    // slot i of row 0 is exponent 3^i, of row 1 exponent 2n - 3^i; exponent e is evaluation brv((e - 1) / 2)
    std::vector<uint32_t> perm(n);
    const int T = n / 16;
    u64 e = 1;
    for (int i = 0; i < n / 2; ++i) {
        const int k0 = bitrev((int)((e - 1) / 2), logn), k1 = bitrev((int)((2 * (u64)n - e - 1) / 2), logn);
        perm[i] = (uint32_t)((k0 % 16) * T + k0 / 16);
        perm[n / 2 + i] = (uint32_t)((k1 % 16) * T + k1 / 16);
        e = e * 3 % (2 * (u64)n);
    }
    if (!c->d_btw)
        if (int e_ = c->d_btw.alloc(tw.size() * sizeof(uint2))) return e_;
    if (!c->d_bperm)
        if (int e_ = c->d_bperm.alloc(perm.size() * sizeof(uint32_t))) return e_;
    if (int e_ = upload(c, c->d_btw, tw.data(), tw.size() * sizeof(uint2))) return e_;
    if (int e_ = upload(c, c->d_bperm, perm.data(), perm.size() * sizeof(uint32_t))) return e_;
    BatchTab& B = c->batch_tab;
    std::memset(&B, 0, sizeof(B));
    const u64 ninv = invmod_h((u64)n % t, t), lw = mulmod_h(tw[(size_t)n + 1].x, ninv, t);
    B.P.p = (uint32_t)t;
    B.P.n_inv = (uint32_t)ninv;
    B.P.n_inv_s = sh32(ninv, t);
    B.P.last_w = (uint32_t)lw;
    B.P.last_ws = sh32(lw, t);
    B.P.tw_fwd = c->d_btw;
    B.P.tw_inv = c->d_btw + n;
    B.mu = ~0ull / t;
    B.perm = c->d_bperm;
    // ks32_dev.hpp's forms: lazy butterflies below 2^30 (2), reduced operands below 2^31 (0); beyond, 64-bit carries
    c->batch_form = t < (1ull << 30) ? 2 : t < (1ull << 31) ? 0 : BF_STRICT;
    c->batch_root = zeta;
    c->batch_state = 1;
    return 0;
}

extern "C" int exacto_batch_info(exacto_ctx* c, uint64_t* root) {
    if (int e = check_ctx(c)) return e;
    if (int e = batch_ready(c)) return e;
    if (root) *root = c->batch_root;
    return 0;
}

// in / out [B][n]: equal or disjoint
static int batch_overlap_check(const uint64_t* in, const uint64_t* out, size_t words) {
    if (!in || !out) return invalid_param("batch: null buffer");
    if (in != out && out < in + words && in < out + words)
        return invalid_param("batch: out overlaps in (only out == in is allowed)");
    return 0;
}

static int batch_transform_dev(exacto_ctx* c, bool encode, const uint64_t* in, uint64_t* out, size_t B) {
    if (int e = check_ctx(c)) return e;
    if (int e = batch_ready(c)) return e;
    if (B == 0) return 0;
    if (int e = batch_overlap_check(in, out, B * (size_t)c->n)) return e;
    if (((uintptr_t)in | (uintptr_t)out) & 15) return invalid_param("batch: buffers must be 16-byte aligned");
    // one grid dimension: 2^31 - 1 polynomials per launch
    const size_t step = (size_t)1 << 30;
    for (size_t i0 = 0; i0 < B; i0 += step) {
        launch_batch_transform(encode, in + i0 * c->n, out + i0 * c->n, (long)std::min(step, B - i0), c->logn,
                               c->batch_tab, c->batch_form, c->stream);
        CHECK_LAUNCH();
    }
    return 0;
}

extern "C" int exacto_batch_encode_dev(exacto_ctx* c, const uint64_t* values, uint64_t* pt, size_t B) {
    return batch_transform_dev(c, true, values, pt, B);
}
extern "C" int exacto_batch_decode_dev(exacto_ctx* c, const uint64_t* pt, uint64_t* values, size_t B) {
    return batch_transform_dev(c, false, pt, values, B);
}

// encode_simd's range check (encoding.rs:40-46): the first value >= t
static int batch_values_check(const exacto_ctx* c, const uint64_t* values, size_t B) {
    for (size_t i = 0; i < B * (size_t)c->n; ++i)
        if (values[i] >= c->plain)
            return invalid_param("plaintext " + std::to_string(values[i]) + " >= plain_modulus " +
                                 std::to_string(c->plain));
    return 0;
}

static int batch_transform_host(exacto_ctx* c, bool encode, const uint64_t* in, uint64_t* out, size_t B) {
    if (int e = check_ctx(c)) return e;
    if (int e = batch_ready(c)) return e;
    if (B == 0) return 0;
    if (int e = batch_overlap_check(in, out, B * (size_t)c->n)) return e;
    if (encode)
        if (int e = batch_values_check(c, in, B)) return e;
    const size_t bytes = B * poly_bytes(c);
    return host_call(c, {{in, bytes}}, bytes, out,
                     [&](std::vector<u64*>& d, u64* o) { return batch_transform_dev(c, encode, d[0], o, B); });
}

extern "C" int exacto_batch_encode(exacto_ctx* c, const uint64_t* values, uint64_t* pt, size_t B) {
    return batch_transform_host(c, true, values, pt, B);
}
extern "C" int exacto_batch_decode(exacto_ctx* c, const uint64_t* pt, uint64_t* values, size_t B) {
    return batch_transform_host(c, false, pt, values, B);
}

// 3^(steps mod n/2) mod 2n (negative steps rotate right) and 2n - 1; host only
extern "C" int exacto_galois_element_rotate_rows(size_t n, int64_t steps, uint64_t* element) {
    if (!element) return invalid_param("null argument");
    if (n < 4 || (n & (n - 1)) != 0) return fail(EXACTO_ERR_INVALID_RING_DEGREE,
                                                 "ring degree must be a power of 2, got " + std::to_string(n));
    const int64_t h = (int64_t)(n / 2);
    const uint64_t k = (uint64_t)(((steps % h) + h) % h);
    *element = powmod_h(3, k, 2 * (u64)n);
    return 0;
}
extern "C" int exacto_galois_element_swap_rows(size_t n, uint64_t* element) {
    if (!element) return invalid_param("null argument");
    if (n < 4 || (n & (n - 1)) != 0) return fail(EXACTO_ERR_INVALID_RING_DEGREE,
                                                 "ring degree must be a power of 2, got " + std::to_string(n));
    *element = 2 * (u64)n - 1;
    return 0;
}

extern "C" int exacto_bfv_rotate_rows_dev(exacto_ctx* c, const uint64_t* ct, size_t polys, int64_t steps,
                                          const uint64_t* gk, size_t num_keys, uint64_t* out, size_t B) {
    if (int e = check_ctx(c)) return e;
    uint64_t element = 1;
    if (int e = exacto_galois_element_rotate_rows((size_t)c->n, steps, &element)) return e;
    if (element != 1) return exacto_bfv_apply_automorphism_dev(c, ct, polys, element, gk, num_keys, out, B);
    // the identity: a copy, no key
    if (polys != 2) return invalid_param("automorphism requires degree-1 ciphertext");
    if (B == 0) return 0;
    if (!ct || !out) return invalid_param("null argument");
    if (out != ct) HIP_TRY(dev_copy(out, ct, B * 2 * c->L * poly_bytes(c), c->stream));
    return 0;
}
extern "C" int exacto_bfv_swap_rows_dev(exacto_ctx* c, const uint64_t* ct, size_t polys, const uint64_t* gk,
                                        size_t num_keys, uint64_t* out, size_t B) {
    if (int e = check_ctx(c)) return e;
    return exacto_bfv_apply_automorphism_dev(c, ct, polys, 2 * (u64)c->n - 1, gk, num_keys, out, B);
}
extern "C" int exacto_bfv_rotate_rows(exacto_ctx* c, const uint64_t* ct, size_t polys, int64_t steps,
                                      const uint64_t* gk, size_t num_keys, uint64_t* out, size_t B) {
    if (!c) return invalid_param("null context");
    uint64_t element = 1;
    if (int e = exacto_galois_element_rotate_rows((size_t)c->n, steps, &element)) return e;
    if (element != 1) return exacto_bfv_apply_automorphism(c, ct, polys, element, gk, num_keys, out, B);
    if (polys != 2) return invalid_param("automorphism requires degree-1 ciphertext");
    if (B == 0) return 0;
    if (!ct || !out) return invalid_param("null argument");
    if (out != ct) std::memmove(out, ct, B * 2 * c->L * poly_bytes(c));
    return 0;
}
extern "C" int exacto_bfv_swap_rows(exacto_ctx* c, const uint64_t* ct, size_t polys, const uint64_t* gk,
                                    size_t num_keys, uint64_t* out, size_t B) {
    if (!c) return invalid_param("null context");
    return exacto_bfv_apply_automorphism(c, ct, polys, 2 * (u64)c->n - 1, gk, num_keys, out, B);
}

// ---- hoisted rotations and slot linear transforms on a prepared Galois key set (hoist.hip)

// perm[p] = the storage position whose value lands at storage position p under sigma_element:
// NTT(sigma(a))[p] = NTT(a)[perm[p]].  Storage position p holds evaluation j = (p mod n/16) 16 + p / (n/16)
// (evaluation j at (j mod 16) n/16 + j / 16), evaluation j is the value at psi^(2 brv(j) + 1), and
// sigma_k(a)(x) = a(x^k): evaluation j of sigma_k(a) is evaluation j' of a with
// 2 brv(j') + 1 = (2 brv(j) + 1) k mod 2n.  The same table for every prime.  Host only.
extern "C" int exacto_galois_ntt_permutation(size_t n, uint64_t element, uint32_t* perm) {
    if (!perm) return invalid_param("null argument");
    if (n < 16 || n > 16384 || (n & (n - 1)) != 0)
        return fail(EXACTO_ERR_INVALID_RING_DEGREE,
                    "ring degree must be a power of 2 in 16..16384, got " + std::to_string(n));
    const u64 k = element % (2 * (u64)n);
    if ((k & 1) == 0) return invalid_param("hoisted automorphisms require odd Galois elements");
    int logn = 0;
    while (((size_t)1 << logn) < n) ++logn;
    const size_t m = n / 16;
    for (size_t p = 0; p < n; ++p) {
        const int j = (int)((p % m) * 16 + p / m);
        const u64 e = ((2 * (u64)bitrev(j, logn) + 1) * k) % (2 * (u64)n);
        const size_t j2 = (size_t)bitrev((int)((e - 1) / 2), logn);
        perm[p] = (uint32_t)((j2 % 16) * m + j2 / 16);
    }
    return 0;
}

struct exacto_galois_keyset {
    int device = 0, n = 0, L = 0;
    std::vector<u64> primes;      // the ciphertext primes of the context it was prepared on
    u64 gbase = 0;
    size_t R = 0;
    int guse = 0;                 // min(G, num_keys); 0: every element is the identity
    bool k32 = false;             // keys as ks32_convert_key's rows in the narrow 31-bit basis
    int S = 0, mac_form = 0;
    DevBuf<uint32_t> d_perm;      // [R][n]
    DevBuf<unsigned char> d_ident;     // [R]
    DevBuf<u64> d_keys, d_keys_s;      // limb-wise: [R][guse][2][L][n] and Shoup companions
    DevBuf<uint32_t> d_rs;        // 31-bit path: [R][guse][2L][S][n]
};

extern "C" void exacto_galois_keyset_destroy(exacto_galois_keyset* ks) {
    if (!ks) return;
    (void)hipSetDevice(ks->device);
    delete ks;
}

extern "C" int exacto_galois_keyset_info(const exacto_galois_keyset* ks, size_t* R, size_t* num_keys_used,
                                         int* ks32_primes) {
    if (!ks) return invalid_param("null key set");
    if (R) *R = ks->R;
    if (num_keys_used) *num_keys_used = (size_t)ks->guse;
    if (ks32_primes) *ks32_primes = ks->k32 ? ks->S : 0;
    return 0;
}

// the single automorphism's choice of key switch (exacto_bfv_apply_automorphism_dev)
static bool hoist_k32(const exacto_ctx* c) {
    const bool d16 = c->digit16 && c->gbase <= 65536;
    return d16 && c->ks32 && c->kn.S > 0 && c->path == EXACTO_PATH_EXACT_RNS;
}

extern "C" int exacto_galois_keyset_create_dev(exacto_ctx* c, const uint64_t* elements, size_t R, const uint64_t* gks,
                                               size_t num_keys, exacto_galois_keyset** out) {
    if (int e = check_ctx(c)) return e;
    if (!out || !elements) return invalid_param("null argument");
    *out = nullptr;
    if (R == 0) return invalid_param("galois key set needs at least one element");
    if (R > 65535) return invalid_param("galois key set holds at most 65535 elements");
    const int n = c->n, L = c->L;
    const long Ln = (long)L * n;
    std::vector<unsigned char> ident(R);
    std::vector<uint32_t> perm(R * (size_t)n);
    bool keyed = false;
    for (size_t r = 0; r < R; ++r) {
        if (int e = exacto_galois_ntt_permutation((size_t)n, elements[r], perm.data() + r * n)) return e;
        ident[r] = elements[r] % (2 * (u64)n) == 1;
        keyed |= !ident[r];
    }
    if (keyed && num_keys == 0) return invalid_param("galois key is empty");
    if (keyed && !gks) return invalid_param("null argument");
    std::unique_ptr<exacto_galois_keyset, void (*)(exacto_galois_keyset*)> ks(new exacto_galois_keyset,
                                                                             exacto_galois_keyset_destroy);
    ks->device = c->device; ks->n = n; ks->L = L;
    ks->primes.assign(c->primes.begin(), c->primes.begin() + L);
    ks->gbase = c->gbase;
    ks->R = R;
    ks->guse = keyed ? (int)std::min<size_t>(c->G, num_keys) : 0;
    ks->k32 = keyed && hoist_k32(c);
    if (int e = ks->d_perm.alloc(perm.size() * sizeof(uint32_t))) return e;
    if (int e = ks->d_ident.alloc((R + 7) / 8 * 8)) return e;
    if (int e = upload(c, ks->d_perm, perm.data(), perm.size() * sizeof(uint32_t))) return e;
    if (int e = upload(c, ks->d_ident, ident.data(), R)) return e;
    const size_t guse = (size_t)ks->guse;
    if (ks->k32) {
        const Ks32Basis& kb = c->kn;   // the narrow basis: its bound holds for any key (as the single call)
        ks->S = kb.S; ks->mac_form = kb.mac_form;
        const long rows = (long)guse * 2 * L;
        if (int e = ks->d_rs.alloc(R * (size_t)rows * kb.S * n * sizeof(uint32_t))) return e;
        Scratch kc;
        HIP_TRY(kc.alloc((size_t)rows * n * sizeof(u64), c->stream, c->pool, c->debug_scratch));
        for (size_t r = 0; r < R; ++r) {
            if (ident[r]) continue;   // its slot is never read
            NttBatch nb{};
            nb.src = gks + r * num_keys * 2 * Ln; nb.src_item_stride = 2 * Ln;
            nb.dst = kc.as<u64>(); nb.dst_item_stride = 2 * Ln;
            nb.ppi = 2 * L; nb.prime_base = 0; nb.period = L;
            if (int e = run_ntt(c, nb, rows, true)) return e;
            ks32_key(kc.as<u64>(), ks->d_rs + r * (size_t)rows * kb.S * n, rows, L, kb.S, c->logn, kb.d_p32, c->d_primes,
                     kb.mac_form, c->stream);
            CHECK_LAUNCH();
        }
    } else if (keyed) {
        const size_t per = guse * 2 * (size_t)Ln;
        if (int e = ks->d_keys.alloc(R * per * sizeof(u64))) return e;
        if (int e = ks->d_keys_s.alloc(R * per * sizeof(u64))) return e;
        for (size_t r = 0; r < R; ++r) {
            if (ident[r])
                launch_rows(ks->d_keys + r * per, 0, nullptr, 0, (long)per, 1, c->stream);
            else
                HIP_TRY(dev_copy(ks->d_keys + r * per, gks + r * num_keys * 2 * Ln, per * sizeof(u64), c->stream));
            CHECK_LAUNCH();
        }
        launch_shoup_companions(ks->d_keys, ks->d_keys_s, (long)(R * per), n, L, c->d_primes, c->stream);
        CHECK_LAUNCH();
    }
    // the caller's gks may go once this returns
    HIP_TRY(hipStreamSynchronize(c->stream));
    *out = ks.release();
    return 0;
}

extern "C" int exacto_galois_keyset_create(exacto_ctx* c, const uint64_t* elements, size_t R, const uint64_t* gks,
                                           size_t num_keys, exacto_galois_keyset** out) {
    if (int e = check_ctx(c)) return e;
    if (!gks || num_keys == 0 || R == 0 || !elements || !out)   // nothing to stage: the device form's checks
        return exacto_galois_keyset_create_dev(c, elements, R, nullptr, num_keys, out);
    const size_t bytes = R * num_keys * 2 * c->L * poly_bytes(c);
    DevBuf<u64> d;
    if (int e = d.alloc(bytes)) return e;
    if (int e = upload(c, d, gks, bytes)) return e;
    return exacto_galois_keyset_create_dev(c, elements, R, d, num_keys, out);
}

static int hoist_check(exacto_ctx* c, const exacto_galois_keyset* ks) {
    if (!ks) return invalid_param("null key set");
    if (ks->n != c->n || ks->L != c->L || ks->gbase != c->gbase || ks->device != c->device ||
        !std::equal(ks->primes.begin(), ks->primes.end(), c->primes.begin()))
        return invalid_param("galois key set was prepared on a context with other parameters");
    if (ks->guse > 0 && (ks->k32 != hoist_k32(c) || (ks->k32 && (ks->S != c->kn.S || ks->mac_form != c->kn.mac_form))))
        return invalid_param("galois key set was prepared for another key-switch path");
    return 0;
}

// What the dBFV entry points add to a hoisted pass: the B limbs are B / d whole dBFV ciphertexts
struct HoistDbfv {
    int d = 1;                  // group size: output (limb, r) goes to hoist_out_index(limb, r, R, d)
    size_t r0 = 0, rc = 0;      // the key set's rotations [r0, r0 + rc) only (rc = 0: all of them)
    // linear transform: the product's tables, its pl the lifted diagonals [rc][d][L][n] of those rotations;
    // out [B / d][d][2][L][n] = (accum ? out : 0) + reduce(sum_r pl_r * rotation r)
    const DbfvPlainArgs* prod = nullptr;
    bool fused = false;         // limb-wise key switch only: dbfv_hoist.hip instead of rotations + product
};

// out[b][r] = (sigma_r(c0) + sum_g sigma_r(d_g) k_{r,g,0}, sum_g sigma_r(d_g) k_{r,g,1}), d_g the digits of c1
// itself; pts != nullptr: out[b] = sum_r pt_r out[b][r] instead (pts [R][n] plaintext coefficients).
static int hoist_core(exacto_ctx* c, const exacto_galois_keyset* ks, const u64* ct, const u64* pts, bool lt, u64* out,
                      size_t B, const HoistDbfv* dv = nullptr) {
    if (int e = check_ctx(c)) return e;
    if (int e = hoist_check(c, ks)) return e;
    if (B == 0) return 0;
    if (!ct || !out || (lt && !pts)) return invalid_param("null argument");
    const int gs = dv ? dv->d : 1;
    const size_t r0 = dv ? dv->r0 : 0, Rz = dv && dv->rc ? dv->rc : ks->R;
    const bool prod = dv && dv->prod;
    const int n = c->n, L = c->L, R = (int)Rz, guse = ks->guse;
    const long Ln = (long)L * n;
    const size_t in_words = B * 2 * (size_t)Ln, out_words = in_words * (lt || prod ? 1 : Rz);
    if (out < ct + in_words && ct < out + out_words) return invalid_param("out must not overlap ct");
    const bool d16 = c->digit16 && c->gbase <= 65536;
    const bool k32 = ks->k32;
    const bool fused = prod && dv->fused && !k32;
    const Ks32Basis& kb = c->kn;
    if (lt)
        if (int e = lift_plain(c, pts, R, false)) return e;   // pl_buf [R][L][n], made before the fork
    // the rotations' slice of the set
    const uint32_t* perm = ks->d_perm + r0 * (size_t)n;
    const unsigned char* ident = ks->d_ident + r0;
    const size_t key_off = r0 * (size_t)guse * 2 * (size_t)Ln;
    // chunk: the 31-bit path's sums (S / 2 outputs per rotation) and, for the linear transforms, its
    // rotations stay within R outputs per chunk item of c->chunk; one launch's blocks within 2^30; whole
    // dBFV ciphertexts (max(1, chunk / d) of them)
    size_t C = std::min<size_t>(c->chunk, B);
    if (k32) C = std::max<size_t>(1, C * 2 / (size_t)(kb.S + (lt || prod ? 2 : 0)));
    const size_t nblk = (size_t)((Ln + 255) / 256);
    if (nblk * Rz * (size_t)gs > ((size_t)1 << 30)) return invalid_param("batch too large");
    C = std::max<size_t>(1, std::min<size_t>(C, ((size_t)1 << 30) / (nblk * Rz)));
    C = std::max<size_t>(1, C / (size_t)gs) * (size_t)gs;
    const long nchunks = (long)((B + C - 1) / C);
    const int nl_max = LanePass::count(c, nchunks);
    // per-lane scratch, declared before the LanePass: allocated before the fork, released after the join
    const size_t u_words = k32 ? C * Rz * 2 * L * (size_t)kb.S * n : 0;               // uint32
    const size_t h_words = ((k32 && lt) || (prod && !fused)) ? C * Rz * 2 * (size_t)Ln : 0;   // u64
    Scratch us, hs;
    if (u_words) HIP_TRY(us.alloc(u_words * nl_max * sizeof(uint32_t), c->stream, c->pool, c->debug_scratch));
    if (h_words) HIP_TRY(hs.alloc(h_words * nl_max * sizeof(u64), c->stream, c->pool, c->debug_scratch));
    LanePass pass;
    if (int e = pass.begin(c, nchunks, C)) return e;
    for (size_t s0 = 0; s0 < B; s0 += C) {
        const int cnt = (int)std::min(C, B - s0);
        const int li = (int)((s0 / C) % (size_t)pass.lanes());
        LaneGuard lane = pass.chunk((long)(s0 / C));
        const u64* src = ct + s0 * 2 * Ln;
        u64* dst = out + s0 * 2 * Ln * (lt || prod ? 1 : Rz);
        // the staged dBFV product: H [cnt / d][R][d][2][L][n] is the term-major operand of dbfv_plain.hip as it is
        auto product = [&](const u64* H) {
            DbfvPlainArgs a = *dv->prod;
            a.cts = H;
            a.ct_term_stride = (long)gs * 2 * Ln; a.ct_item_stride = (long)R * a.ct_term_stride;
            a.K = R; a.polys = 2;
            a.out = dst; a.items = cnt / gs;
            launch_dbfv_plain_mul(a, c->stream);
        };
        if (guse > 0) {
            // c1 alone back to coefficients, its exact CRT and gadget digits, one digit transform
            NttBatch nb{};
            nb.src = src + Ln; nb.src_item_stride = 2 * Ln;
            nb.dst = c->ws.coefQ; nb.dst_item_stride = Ln;
            nb.ppi = L; nb.prime_base = 0; nb.period = L;
            if (int e = run_ntt(c, nb, (long)cnt * L, true)) return e;
            launch_decompose(c->ws.coefQ, Ln, c->ws.D, guse, cnt, n, c->d_crt, c->d_primes, L, c->stream,
                             d16 ? c->ws.D16 : nullptr);
            CHECK_LAUNCH();
        }
        if (k32) {
            uint32_t* U = us.as<uint32_t>() + (size_t)li * u_words;
            u64* H = h_words ? hs.as<u64>() + (size_t)li * h_words : dst;
            {
                ProfScope pd(c, PK_KS_DIGITS, (u64)cnt * guse * kb.S, (2.0 + 4.0 * kb.S) * n * (double)cnt * guse);
                ks32_digits(c->ws.D16, c->ws.DS, cnt, guse, kb.S, c->logn, kb.d_p32, kb.mac_form, c->stream);
            }
            // The basis bound of setup_ks32 covers sigma(d) unchanged: sigma permutes a digit's coefficients
            // up to sign, so the digit magnitudes, and with them |sum_g sigma(d_g) * r_g|, are the same.
            {
                ProfScope pm(c, PK_KS_MAC, (u64)cnt * R * 2 * L * kb.S,
                             4.0 * n * kb.S * ((double)cnt * R * (guse + 2 * L) + (double)R * guse * 2 * L));
                ks32_mac_hoist(c->ws.DS, ks->d_rs + key_off * (size_t)kb.S, U, perm, ident, cnt, R, guse, L, kb.S, n,
                               kb.d_p32, kb.mac_form, c->stream, gs);
            }
            CHECK_LAUNCH();
            // the lift adds into a zeroed coefficient buffer; both components forward; c0 o perm_r joins
            // in the NTT domain
            launch_rows(H, 0, nullptr, 0, (long)cnt * R * 2 * Ln, 1, c->stream);
            {
                ProfScope pc(c, PK_KS_CRT, (u64)cnt * R * 2 * L, (4.0 * kb.S + 16.0) * n * (double)cnt * R * 2 * L);
                ks32_crt(U, H, 2 * Ln, cnt * R, L, kb.S, c->logn, kb.d_kst, kb.d_p32, c->d_primes, kb.mac_form,
                         c->stream, c->ks_fpc && kb.fpc_max >= 1);
            }
            CHECK_LAUNCH();
            NttBatch rb{};
            rb.src = H; rb.src_item_stride = 2 * Ln;
            rb.dst = H; rb.dst_item_stride = 2 * Ln;
            rb.ppi = 2 * L; rb.prime_base = 0; rb.period = L;
            if (int e = run_ntt(c, rb, (long)cnt * R * 2 * L, false)) return e;
            launch_hoist_c0(src, perm, ident, H, R, cnt, n, L, c->d_primes, c->stream, gs);
            if (lt) launch_hoist_ptsum(H, c->pl_buf, dst, R, cnt, n, L, c->d_primes, c->stream);
            if (prod) product(H);
            CHECK_LAUNCH();
            continue;
        }
        if (guse > 0) {
            NttBatch db = contiguous(c->ws.D, cnt, (long)guse * L, 0, L, n);
            if (d16) {
                db.src16 = c->ws.D16;
                db.src16_item_stride = (long)guse * n;
            }
            if (int e = run_ntt(c, db, (long)cnt * guse * L, false)) return e;
        }
        {
            ProfScope pm(c, PK_RELIN_MAC, (u64)cnt * R * 2 * L,
                         8.0 * Ln * ((double)cnt * R * (guse + 1 + (lt ? 0 : 2)) + (double)R * guse * 4));
            const u64* keys = guse > 0 ? ks->d_keys + key_off : nullptr;
            const u64* keys_s = guse > 0 ? ks->d_keys_s + key_off : nullptr;
            if (fused) {
                const DbfvPlainArgs& p = *dv->prod;
                DbfvHoistArgs a{};
                a.ct = src; a.D = c->ws.D; a.keys = keys; a.keys_s = keys_s; a.perm = perm; a.ident = ident;
                a.pl = p.pl; a.out = dst; a.items = cnt / gs;
                a.R = R; a.guse = guse; a.d = gs; a.n = n; a.L = L;
                a.flush = p.flush; a.accum = p.accum; a.live = p.live; a.fold = p.fold; a.primes = c->d_primes;
                launch_dbfv_hoist_lt(a, c->stream);
            } else {
                u64* H = prod ? hs.as<u64>() + (size_t)li * h_words : dst;
                launch_hoist_mac(lt, src, c->ws.D, keys, keys_s, perm, ident, lt ? c->pl_buf : nullptr, H, R, guse, cnt,
                                 n, L, c->d_primes, c->stream, gs);
                if (prod) product(H);
            }
        }
        CHECK_LAUNCH();
    }
    return 0;
}

extern "C" int exacto_bfv_rotate_hoisted_dev(exacto_ctx* c, const exacto_galois_keyset* ks, const uint64_t* ct,
                                             uint64_t* out, size_t B) {
    return hoist_core(c, ks, ct, nullptr, false, out, B);
}

extern "C" int exacto_bfv_linear_transform_dev(exacto_ctx* c, const exacto_galois_keyset* ks, const uint64_t* ct,
                                               const uint64_t* pts, uint64_t* out, size_t B) {
    return hoist_core(c, ks, ct, pts, true, out, B);
}

extern "C" int exacto_bfv_rotate_hoisted(exacto_ctx* c, const exacto_galois_keyset* ks, const uint64_t* ct,
                                         uint64_t* out, size_t B) {
    if (int e = check_ctx(c)) return e;
    if (int e = hoist_check(c, ks)) return e;
    if (B == 0) return 0;
    if (!ct || !out) return invalid_param("null argument");
    const size_t ctb = B * 2 * c->L * poly_bytes(c);
    return host_call(c, {{ct, ctb}}, ctb * ks->R, out,
                     [&](std::vector<u64*>& d, u64* o) { return hoist_core(c, ks, d[0], nullptr, false, o, B); });
}

extern "C" int exacto_bfv_linear_transform(exacto_ctx* c, const exacto_galois_keyset* ks, const uint64_t* ct,
                                           const uint64_t* pts, uint64_t* out, size_t B) {
    if (int e = check_ctx(c)) return e;
    if (int e = hoist_check(c, ks)) return e;
    if (B == 0) return 0;
    if (!ct || !out || !pts) return invalid_param("null argument");
    const size_t ctb = B * 2 * c->L * poly_bytes(c);
    return host_call(c, {{ct, ctb}, {pts, ks->R * poly_bytes(c)}}, ctb, out,
                     [&](std::vector<u64*>& d, u64* o) { return hoist_core(c, ks, d[0], d[1], true, o, B); });
}

// encode + encrypt chunk by chunk through batch_buf: the chunk's items keep the sample indices they
// have in one exacto_encrypt_* call over the whole batch, so the ciphertexts are that call's bit for bit
static int batch_encrypt_dev(exacto_ctx* c, const uint64_t* values, const uint64_t* sk, const uint64_t* pk,
                             double sigma, const uint64_t* key, uint64_t stream, uint64_t* ct, size_t B) {
    if (int e = check_ctx(c)) return e;
    if (int e = batch_ready(c)) return e;
    if (!key || !values || !ct || (!sk && !pk)) return invalid_param("null argument");
    if (B == 0) return 0;
    if ((uintptr_t)values & 15) return invalid_param("batch: buffers must be 16-byte aligned");
    const size_t C = std::min<size_t>(c->chunk, B), n = (size_t)c->n;
    if (c->batch_buf.grow(C * poly_bytes(c))) return EXACTO_ERR_HIP;
    for (size_t i0 = 0; i0 < B; i0 += C) {
        const size_t cnt = std::min(C, B - i0);
        launch_batch_transform(true, values + i0 * n, c->batch_buf, (long)cnt, c->logn, c->batch_tab, c->batch_form,
                               c->stream);
        CHECK_LAUNCH();
        if (int e = encrypt_batch(c, c->batch_buf, sk, pk, sigma, key, stream, ct + i0 * 2 * c->L * n, cnt, nullptr, i0))
            return e;
    }
    return 0;
}

extern "C" int exacto_batch_encrypt_sk_dev(exacto_ctx* c, const uint64_t* values, const uint64_t* sk, double sigma,
                                           const uint64_t* key, uint64_t stream, uint64_t* ct, size_t B) {
    if (c && !sk) return invalid_param("null argument");
    return batch_encrypt_dev(c, values, sk, nullptr, sigma, key, stream, ct, B);
}
extern "C" int exacto_batch_encrypt_pk_dev(exacto_ctx* c, const uint64_t* values, const uint64_t* pk, double sigma,
                                           const uint64_t* key, uint64_t stream, uint64_t* ct, size_t B) {
    if (c && !pk) return invalid_param("null argument");
    return batch_encrypt_dev(c, values, nullptr, pk, sigma, key, stream, ct, B);
}

extern "C" int exacto_batch_decrypt_dev(exacto_ctx* c, const uint64_t* ct, size_t polys, const uint64_t* sk,
                                        uint64_t* values, size_t B) {
    if (int e = check_ctx(c)) return e;
    if (int e = batch_ready(c)) return e;
    if (polys < 1) return invalid_param("ciphertext has no polynomials");
    if (B == 0) return 0;
    if (!ct || !sk || !values) return invalid_param("null argument");
    if ((uintptr_t)values & 15) return invalid_param("batch: buffers must be 16-byte aligned");
    const size_t C = std::min<size_t>(c->chunk, B), n = (size_t)c->n;
    const long stride = (long)polys * c->L * c->n;
    if (c->batch_buf.grow(C * poly_bytes(c))) return EXACTO_ERR_HIP;
    for (size_t i0 = 0; i0 < B; i0 += C) {
        const size_t cnt = std::min(C, B - i0);
        if (int e = decrypt_batch(c, ct + i0 * (size_t)stride, polys, stride, sk, c->batch_buf, cnt)) return e;
        launch_batch_transform(false, c->batch_buf, values + i0 * n, (long)cnt, c->logn, c->batch_tab, c->batch_form,
                               c->stream);
        CHECK_LAUNCH();
    }
    return 0;
}

extern "C" int exacto_batch_encrypt_sk(exacto_ctx* c, const uint64_t* values, const uint64_t* sk, double sigma,
                                       const uint64_t* key, uint64_t stream, uint64_t* ct, size_t B) {
    if (int e = check_ctx(c)) return e;
    if (int e = batch_ready(c)) return e;
    if (!values || !sk || !ct) return invalid_param("null argument");
    if (int e = batch_values_check(c, values, B)) return e;
    return host_call(c, {{values, B * poly_bytes(c)}, {sk, c->L * poly_bytes(c)}}, B * 2 * c->L * poly_bytes(c), ct,
                     [&](std::vector<u64*>& d, u64* o) {
                         return exacto_batch_encrypt_sk_dev(c, d[0], d[1], sigma, key, stream, o, B);
                     });
}
extern "C" int exacto_batch_encrypt_pk(exacto_ctx* c, const uint64_t* values, const uint64_t* pk, double sigma,
                                       const uint64_t* key, uint64_t stream, uint64_t* ct, size_t B) {
    if (int e = check_ctx(c)) return e;
    if (int e = batch_ready(c)) return e;
    if (!values || !pk || !ct) return invalid_param("null argument");
    if (int e = batch_values_check(c, values, B)) return e;
    return host_call(c, {{values, B * poly_bytes(c)}, {pk, 2 * c->L * poly_bytes(c)}}, B * 2 * c->L * poly_bytes(c), ct,
                     [&](std::vector<u64*>& d, u64* o) {
                         return exacto_batch_encrypt_pk_dev(c, d[0], d[1], sigma, key, stream, o, B);
                     });
}
extern "C" int exacto_batch_decrypt(exacto_ctx* c, const uint64_t* ct, size_t polys, const uint64_t* sk,
                                    uint64_t* values, size_t B) {
    if (int e = check_ctx(c)) return e;
    if (int e = batch_ready(c)) return e;
    if (polys < 1) return invalid_param("ciphertext has no polynomials");
    if (B == 0) return 0;
    if (!ct || !sk || !values) return invalid_param("null argument");
    return host_call(c, {{ct, B * polys * c->L * poly_bytes(c)}, {sk, c->L * poly_bytes(c)}}, B * poly_bytes(c), values,
                     [&](std::vector<u64*>& dv, u64* o) { return exacto_batch_decrypt_dev(c, dv[0], polys, dv[1], o, B); });
}

// ============================================================== slot-packed dBFV (no reference function)
// n integers mod p per dBFV ciphertext: limb k carries the slot encoding of every slot's k-th digit.  The
// fused transforms are batch.hip's dbfv_batch_*_kernel; the convention is in include/exacto_hip.h.

// batch_ready's errors, then DbfvParams::new's, then the digit range (dbfv/encrypt.rs:152-159)
static int dbfv_batch_check(exacto_ctx* c, size_t d, uint64_t base, uint64_t plain) {
    if (int e = check_ctx(c)) return e;
    if (int e = batch_ready(c)) return e;
    if (int e = dbfv_params_check(d, base, plain)) return e;
    if (base > c->plain)
        return invalid_param("dBFV base " + std::to_string(base) + " must be <= BFV plaintext modulus " +
                             std::to_string(c->plain));
    if (d > (size_t)INT32_MAX / 2) return invalid_param("batch * num_digits too large");
    return 0;
}

// values [B][n] and pt [B][d][n]: sizes differ, so any overlap is an error
static int dbfv_batch_buffers_check(const uint64_t* values, const uint64_t* pt, size_t vwords, size_t d, bool dev) {
    if (!values || !pt) return invalid_param("dbfv batch: null buffer");
    if (dev && (((uintptr_t)values | (uintptr_t)pt) & 15))
        return invalid_param("dbfv batch: buffers must be 16-byte aligned");
    if (pt < values + vwords && values < pt + vwords * d)
        return invalid_param("dbfv batch: values and pt overlap (no in-place form)");
    return 0;
}

static void dbfv_batch_launch(exacto_ctx* c, bool encode, const u64* in, u64* out, size_t items, size_t d,
                              uint64_t base, uint64_t plain) {
    // one grid dimension: 2^31 - 1 items per launch
    const size_t step = (size_t)1 << 30, n = (size_t)c->n;
    for (size_t i0 = 0; i0 < items; i0 += step) {
        const size_t vo = i0 * n, po = i0 * d * n;
        launch_dbfv_batch(encode, in + (encode ? vo : po), out + (encode ? po : vo), (long)std::min(step, items - i0),
                          (int)d, base, plain, c->logn, c->batch_tab, c->batch_form, c->stream);
    }
}

static int dbfv_batch_transform_dev(exacto_ctx* c, bool encode, size_t d, uint64_t base, uint64_t plain,
                                    const uint64_t* values, const uint64_t* pt, size_t B) {
    if (int e = dbfv_batch_check(c, d, base, plain)) return e;
    if (B == 0) return 0;
    if (int e = dbfv_batch_buffers_check(values, pt, B * (size_t)c->n, d, true)) return e;
    dbfv_batch_launch(c, encode, encode ? values : pt, const_cast<u64*>(encode ? pt : values), B, d, base, plain);
    CHECK_LAUNCH();
    return 0;
}

extern "C" int exacto_dbfv_batch_encode_dev(exacto_ctx* c, size_t d, uint64_t base, uint64_t plain,
                                            const uint64_t* values, uint64_t* pt, size_t B) {
    return dbfv_batch_transform_dev(c, true, d, base, plain, values, pt, B);
}
extern "C" int exacto_dbfv_batch_decode_dev(exacto_ctx* c, size_t d, uint64_t base, uint64_t plain,
                                            const uint64_t* pt, uint64_t* values, size_t B) {
    return dbfv_batch_transform_dev(c, false, d, base, plain, values, pt, B);
}

static int dbfv_batch_transform_host(exacto_ctx* c, bool encode, size_t d, uint64_t base, uint64_t plain,
                                     const uint64_t* values, const uint64_t* pt, size_t B) {
    if (int e = dbfv_batch_check(c, d, base, plain)) return e;
    if (B == 0) return 0;
    if (int e = dbfv_batch_buffers_check(values, pt, B * (size_t)c->n, d, false)) return e;
    const size_t vb = B * poly_bytes(c), pb = vb * d;
    return host_call(c, {{encode ? values : pt, encode ? vb : pb}}, encode ? pb : vb,
                     const_cast<uint64_t*>(encode ? pt : values), [&](std::vector<u64*>& in, u64* o) {
                         return dbfv_batch_transform_dev(c, encode, d, base, plain, encode ? in[0] : o,
                                                         encode ? o : in[0], B);
                     });
}

extern "C" int exacto_dbfv_batch_encode(exacto_ctx* c, size_t d, uint64_t base, uint64_t plain, const uint64_t* values,
                                        uint64_t* pt, size_t B) {
    return dbfv_batch_transform_host(c, true, d, base, plain, values, pt, B);
}
extern "C" int exacto_dbfv_batch_decode(exacto_ctx* c, size_t d, uint64_t base, uint64_t plain, const uint64_t* pt,
                                        uint64_t* values, size_t B) {
    return dbfv_batch_transform_host(c, false, d, base, plain, values, pt, B);
}

// encode + encrypt chunk by chunk through batch_buf (d plaintexts per item): limb k of item b keeps the
// sample indices of item b * d + k of one exacto_encrypt_* call over the [B * d][n] plaintexts
static int dbfv_batch_encrypt_dev(exacto_ctx* c, size_t d, uint64_t base, uint64_t plain, const uint64_t* values,
                                  const uint64_t* sk, const uint64_t* pk, double sigma, const uint64_t* key,
                                  uint64_t stream, uint64_t* ct, size_t B) {
    if (int e = dbfv_batch_check(c, d, base, plain)) return e;
    if (!key || !values || !ct || (!sk && !pk)) return invalid_param("null argument");
    if (B > (size_t)INT32_MAX / d) return invalid_param("batch * num_digits too large");
    if (B == 0) return 0;
    if ((uintptr_t)values & 15) return invalid_param("dbfv batch: buffers must be 16-byte aligned");
    const size_t C = std::min<size_t>(c->chunk, B), n = (size_t)c->n;
    if (c->batch_buf.grow(C * d * poly_bytes(c))) return EXACTO_ERR_HIP;
    for (size_t i0 = 0; i0 < B; i0 += C) {
        const size_t cnt = std::min(C, B - i0);
        dbfv_batch_launch(c, true, values + i0 * n, c->batch_buf, cnt, d, base, plain);
        CHECK_LAUNCH();
        if (int e = encrypt_batch(c, c->batch_buf, sk, pk, sigma, key, stream, ct + i0 * d * 2 * c->L * n, cnt * d,
                                  nullptr, i0 * d))
            return e;
    }
    return 0;
}

extern "C" int exacto_dbfv_batch_encrypt_sk_dev(exacto_ctx* c, size_t d, uint64_t base, uint64_t plain,
                                                const uint64_t* values, const uint64_t* sk, double sigma,
                                                const uint64_t* key, uint64_t stream, uint64_t* ct, size_t B) {
    if (int e = dbfv_batch_check(c, d, base, plain)) return e;
    if (!sk) return invalid_param("null argument");
    return dbfv_batch_encrypt_dev(c, d, base, plain, values, sk, nullptr, sigma, key, stream, ct, B);
}
extern "C" int exacto_dbfv_batch_encrypt_pk_dev(exacto_ctx* c, size_t d, uint64_t base, uint64_t plain,
                                                const uint64_t* values, const uint64_t* pk, double sigma,
                                                const uint64_t* key, uint64_t stream, uint64_t* ct, size_t B) {
    if (int e = dbfv_batch_check(c, d, base, plain)) return e;
    if (!pk) return invalid_param("null argument");
    return dbfv_batch_encrypt_dev(c, d, base, plain, values, nullptr, pk, sigma, key, stream, ct, B);
}

// decrypt_batch over the chunk's limbs into dig_buf, then the fused decode
extern "C" int exacto_dbfv_batch_decrypt_dev(exacto_ctx* c, size_t d, uint64_t base, uint64_t plain,
                                             const uint64_t* ct, const uint64_t* sk, uint64_t* values, size_t B) {
    if (int e = dbfv_batch_check(c, d, base, plain)) return e;
    if (!ct || !sk || !values) return invalid_param("null argument");
    if (B > (size_t)INT32_MAX / d) return invalid_param("batch * num_digits too large");
    if (B == 0) return 0;
    if ((uintptr_t)values & 15) return invalid_param("dbfv batch: buffers must be 16-byte aligned");
    const size_t C = std::min<size_t>(c->chunk, B), n = (size_t)c->n;
    const long stride = 2L * c->L * c->n;
    if (c->dig_buf.grow(C * d * poly_bytes(c))) return EXACTO_ERR_HIP;
    for (size_t i0 = 0; i0 < B; i0 += C) {
        const size_t cnt = std::min(C, B - i0);
        if (int e = decrypt_batch(c, ct + i0 * d * (size_t)stride, 2, stride, sk, c->dig_buf, cnt * d)) return e;
        dbfv_batch_launch(c, false, c->dig_buf, values + i0 * n, cnt, d, base, plain);
        CHECK_LAUNCH();
    }
    return 0;
}

static int dbfv_batch_encrypt_host(exacto_ctx* c, size_t d, uint64_t base, uint64_t plain, const uint64_t* values,
                                   const uint64_t* sk, const uint64_t* pk, double sigma, const uint64_t* key,
                                   uint64_t stream, uint64_t* ct, size_t B) {
    if (int e = dbfv_batch_check(c, d, base, plain)) return e;
    if (!values || !ct || !key || (!sk && !pk)) return invalid_param("null argument");
    const size_t keyb = (pk ? 2 : 1) * c->L * poly_bytes(c);
    return host_call(c, {{values, B * poly_bytes(c)}, {pk ? pk : sk, keyb}}, B * d * 2 * c->L * poly_bytes(c), ct,
                     [&](std::vector<u64*>& in, u64* o) {
                         return dbfv_batch_encrypt_dev(c, d, base, plain, in[0], pk ? nullptr : in[1],
                                                       pk ? in[1] : nullptr, sigma, key, stream, o, B);
                     });
}

extern "C" int exacto_dbfv_batch_encrypt_sk(exacto_ctx* c, size_t d, uint64_t base, uint64_t plain,
                                            const uint64_t* values, const uint64_t* sk, double sigma,
                                            const uint64_t* key, uint64_t stream, uint64_t* ct, size_t B) {
    return dbfv_batch_encrypt_host(c, d, base, plain, values, sk, nullptr, sigma, key, stream, ct, B);
}
extern "C" int exacto_dbfv_batch_encrypt_pk(exacto_ctx* c, size_t d, uint64_t base, uint64_t plain,
                                            const uint64_t* values, const uint64_t* pk, double sigma,
                                            const uint64_t* key, uint64_t stream, uint64_t* ct, size_t B) {
    return dbfv_batch_encrypt_host(c, d, base, plain, values, nullptr, pk, sigma, key, stream, ct, B);
}
extern "C" int exacto_dbfv_batch_decrypt(exacto_ctx* c, size_t d, uint64_t base, uint64_t plain, const uint64_t* ct,
                                         const uint64_t* sk, uint64_t* values, size_t B) {
    if (int e = dbfv_batch_check(c, d, base, plain)) return e;
    if (!ct || !sk || !values) return invalid_param("null argument");
    if (B == 0) return 0;
    return host_call(c, {{ct, B * d * 2 * c->L * poly_bytes(c)}, {sk, c->L * poly_bytes(c)}}, B * poly_bytes(c), values,
                     [&](std::vector<u64*>& in, u64* o) {
                         return exacto_dbfv_batch_decrypt_dev(c, d, base, plain, in[0], in[1], o, B);
                     });
}

// ============================================================== dBFV beyond the product
// encryption (dbfv/encrypt.rs), limb-wise operations (dbfv/eval.rs:11-71, dbfv/keyswitch.rs,
// dbfv/advanced.rs:15-29) and the maps between digit vectors (dbfv/advanced.rs:36-160)

static std::string u128_str(u128 v) {
    std::string s;
    do { s.insert(s.begin(), char('0' + (int)(v % 10))); v /= 10; } while (v);
    return s;
}

// DbfvParams::new, then validate_digit_polys' base check (dbfv/encrypt.rs:152-159; its coefficient
// check cannot fail: digits are below base <= t), then normalize_poly_plaintext's (encrypt.rs:121-126)
static int dbfv_encrypt_dev(exacto_ctx* c, size_t d, uint64_t base, uint64_t plain, const uint64_t* src, bool poly,
                            const uint64_t* sk, const uint64_t* pk, double sigma, const uint64_t* key,
                            uint64_t stream, uint64_t* ct, size_t B) {
    if (int e = check_ctx(c)) return e;
    if (int e = dbfv_params_check(d, base, plain)) return e;
    if (poly && plain == 0)
        return invalid_param("polynomial dBFV plaintext requires finite plain_modulus (plain_modulus=0 is scalar-only)");
    if (base > c->plain)
        return invalid_param("dBFV base " + std::to_string(base) + " must be <= BFV plaintext modulus " +
                             std::to_string(c->plain));
    if (!sk && !pk) return invalid_param("null argument");
    if (d > (size_t)INT32_MAX / 2 || B > (size_t)INT32_MAX / d) return invalid_param("batch * num_digits too large");
    const DbfvPlain dp{d, base, plain, poly};
    return encrypt_batch(c, src, sk, pk, sigma, key, stream, ct, B, &dp);
}

static int dbfv_encrypt_host(exacto_ctx* c, size_t d, uint64_t base, uint64_t plain, const uint64_t* src, bool poly,
                             const uint64_t* sk, const uint64_t* pk, double sigma, const uint64_t* key,
                             uint64_t stream, uint64_t* ct, size_t B) {
    if (!c) return invalid_param("null context");
    const size_t keyb = (pk ? 2 : 1) * c->L * poly_bytes(c);
    return host_call(c, {{src, poly ? B * poly_bytes(c) : B * sizeof(u64)}, {pk ? pk : sk, keyb}},
                     B * d * 2 * c->L * poly_bytes(c), ct, [&](std::vector<u64*>& in, u64* o) {
                         return dbfv_encrypt_dev(c, d, base, plain, in[0], poly, pk ? nullptr : in[1],
                                                 pk ? in[1] : nullptr, sigma, key, stream, o, B);
                     });
}

extern "C" int exacto_dbfv_encrypt_sk_dev(exacto_ctx* c, size_t d, uint64_t base, uint64_t plain,
                                          const uint64_t* values, const uint64_t* sk, double sigma,
                                          const uint64_t* key, uint64_t stream, uint64_t* ct, size_t B) {
    if (!sk) return invalid_param("null argument");
    return dbfv_encrypt_dev(c, d, base, plain, values, false, sk, nullptr, sigma, key, stream, ct, B);
}
extern "C" int exacto_dbfv_encrypt_pk_dev(exacto_ctx* c, size_t d, uint64_t base, uint64_t plain,
                                          const uint64_t* values, const uint64_t* pk, double sigma,
                                          const uint64_t* key, uint64_t stream, uint64_t* ct, size_t B) {
    if (!pk) return invalid_param("null argument");
    return dbfv_encrypt_dev(c, d, base, plain, values, false, nullptr, pk, sigma, key, stream, ct, B);
}
extern "C" int exacto_dbfv_encrypt_poly_sk_dev(exacto_ctx* c, size_t d, uint64_t base, uint64_t plain,
                                               const uint64_t* pt, const uint64_t* sk, double sigma,
                                               const uint64_t* key, uint64_t stream, uint64_t* ct, size_t B) {
    if (!sk) return invalid_param("null argument");
    return dbfv_encrypt_dev(c, d, base, plain, pt, true, sk, nullptr, sigma, key, stream, ct, B);
}
extern "C" int exacto_dbfv_encrypt_poly_pk_dev(exacto_ctx* c, size_t d, uint64_t base, uint64_t plain,
                                               const uint64_t* pt, const uint64_t* pk, double sigma,
                                               const uint64_t* key, uint64_t stream, uint64_t* ct, size_t B) {
    if (!pk) return invalid_param("null argument");
    return dbfv_encrypt_dev(c, d, base, plain, pt, true, nullptr, pk, sigma, key, stream, ct, B);
}
extern "C" int exacto_dbfv_encrypt_sk(exacto_ctx* c, size_t d, uint64_t base, uint64_t plain, const uint64_t* values,
                                      const uint64_t* sk, double sigma, const uint64_t* key, uint64_t stream,
                                      uint64_t* ct, size_t B) {
    if (!sk) return invalid_param("null argument");
    return dbfv_encrypt_host(c, d, base, plain, values, false, sk, nullptr, sigma, key, stream, ct, B);
}
extern "C" int exacto_dbfv_encrypt_pk(exacto_ctx* c, size_t d, uint64_t base, uint64_t plain, const uint64_t* values,
                                      const uint64_t* pk, double sigma, const uint64_t* key, uint64_t stream,
                                      uint64_t* ct, size_t B) {
    if (!pk) return invalid_param("null argument");
    return dbfv_encrypt_host(c, d, base, plain, values, false, nullptr, pk, sigma, key, stream, ct, B);
}
extern "C" int exacto_dbfv_encrypt_poly_sk(exacto_ctx* c, size_t d, uint64_t base, uint64_t plain, const uint64_t* pt,
                                           const uint64_t* sk, double sigma, const uint64_t* key, uint64_t stream,
                                           uint64_t* ct, size_t B) {
    if (!sk) return invalid_param("null argument");
    return dbfv_encrypt_host(c, d, base, plain, pt, true, sk, nullptr, sigma, key, stream, ct, B);
}
extern "C" int exacto_dbfv_encrypt_poly_pk(exacto_ctx* c, size_t d, uint64_t base, uint64_t plain, const uint64_t* pt,
                                           const uint64_t* pk, double sigma, const uint64_t* key, uint64_t stream,
                                           uint64_t* ct, size_t B) {
    if (!pk) return invalid_param("null argument");
    return dbfv_encrypt_host(c, d, base, plain, pt, true, nullptr, pk, sigma, key, stream, ct, B);
}

// dbfv_add / dbfv_sub (dbfv/eval.rs:11-58): the limbs are B * d independent BFV ciphertexts
static int dbfv_addsub_dev(exacto_ctx* c, bool sub, const uint64_t* a, size_t d1, size_t p1, const uint64_t* b,
                           size_t d2, size_t p2, uint64_t* out, size_t B, const uint32_t* da, const uint32_t* db,
                           uint32_t* dout) {
    if (int e = check_ctx(c)) return e;
    if (d1 != d2)
        return fail(EXACTO_ERR_DIMENSION_MISMATCH,
                    "dimension mismatch: expected " + std::to_string(d1) + ", got " + std::to_string(d2));
    if (int e = bfv_addsub(c, sub, a, p1, b, p2, out, B * d1)) return e;
    if (dout)
        for (size_t i = 0; i < B; ++i) dout[i] = std::max(da ? da[i] : 0u, db ? db[i] : 0u);
    return 0;
}
static int dbfv_addsub_host(exacto_ctx* c, bool sub, const uint64_t* a, size_t d1, size_t p1, const uint64_t* b,
                            size_t d2, size_t p2, uint64_t* out, size_t B, const uint32_t* da, const uint32_t* db,
                            uint32_t* dout) {
    if (!c) return invalid_param("null context");
    if (d1 != d2) return dbfv_addsub_dev(c, sub, a, d1, p1, b, d2, p2, out, B, da, db, dout);
    const size_t pb = c->L * poly_bytes(c);
    return host_call(c, {{a, B * d1 * p1 * pb}, {b, B * d2 * p2 * pb}}, B * d1 * std::max(p1, p2) * pb, out,
                     [&](std::vector<u64*>& in, u64* o) {
                         return dbfv_addsub_dev(c, sub, in[0], d1, p1, in[1], d2, p2, o, B, da, db, dout);
                     });
}
extern "C" int exacto_dbfv_add_dev(exacto_ctx* c, const uint64_t* a, size_t d1, size_t p1, const uint64_t* b, size_t d2,
                                   size_t p2, uint64_t* out, size_t B, const uint32_t* da, const uint32_t* db,
                                   uint32_t* dout) {
    return dbfv_addsub_dev(c, false, a, d1, p1, b, d2, p2, out, B, da, db, dout);
}
extern "C" int exacto_dbfv_sub_dev(exacto_ctx* c, const uint64_t* a, size_t d1, size_t p1, const uint64_t* b, size_t d2,
                                   size_t p2, uint64_t* out, size_t B, const uint32_t* da, const uint32_t* db,
                                   uint32_t* dout) {
    return dbfv_addsub_dev(c, true, a, d1, p1, b, d2, p2, out, B, da, db, dout);
}
extern "C" int exacto_dbfv_add(exacto_ctx* c, const uint64_t* a, size_t d1, size_t p1, const uint64_t* b, size_t d2,
                               size_t p2, uint64_t* out, size_t B, const uint32_t* da, const uint32_t* db,
                               uint32_t* dout) {
    return dbfv_addsub_host(c, false, a, d1, p1, b, d2, p2, out, B, da, db, dout);
}
extern "C" int exacto_dbfv_sub(exacto_ctx* c, const uint64_t* a, size_t d1, size_t p1, const uint64_t* b, size_t d2,
                               size_t p2, uint64_t* out, size_t B, const uint32_t* da, const uint32_t* db,
                               uint32_t* dout) {
    return dbfv_addsub_host(c, true, a, d1, p1, b, d2, p2, out, B, da, db, dout);
}

// dbfv_neg (eval.rs:61-71), dbfv_relinearize (keyswitch.rs:9-23), dbfv_apply_automorphism
// (advanced.rs:15-29): the BFV entry point over the B * d limbs
extern "C" int exacto_dbfv_neg_dev(exacto_ctx* c, const uint64_t* ct, size_t d, size_t polys, uint64_t* out, size_t B) {
    return exacto_bfv_neg_dev(c, ct, polys, out, B * d);
}
extern "C" int exacto_dbfv_neg(exacto_ctx* c, const uint64_t* ct, size_t d, size_t polys, uint64_t* out, size_t B) {
    return exacto_bfv_neg(c, ct, polys, out, B * d);
}
extern "C" int exacto_dbfv_relinearize_dev(exacto_ctx* c, const uint64_t* ct, size_t d, size_t polys, uint64_t* out,
                                           size_t B) {
    return exacto_relinearize_dev(c, ct, polys, out, B * d);
}
extern "C" int exacto_dbfv_relinearize(exacto_ctx* c, const uint64_t* ct, size_t d, size_t polys, uint64_t* out,
                                       size_t B) {
    return exacto_relinearize(c, ct, polys, out, B * d);
}
extern "C" int exacto_dbfv_apply_automorphism_dev(exacto_ctx* c, const uint64_t* ct, size_t d, size_t polys,
                                                  uint64_t element, const uint64_t* gk, size_t num_keys, uint64_t* out,
                                                  size_t B) {
    return exacto_bfv_apply_automorphism_dev(c, ct, polys, element, gk, num_keys, out, B * d);
}
extern "C" int exacto_dbfv_apply_automorphism(exacto_ctx* c, const uint64_t* ct, size_t d, size_t polys,
                                              uint64_t element, const uint64_t* gk, size_t num_keys, uint64_t* out,
                                              size_t B) {
    return exacto_bfv_apply_automorphism(c, ct, polys, element, gk, num_keys, out, B * d);
}

// out[b][j] = sum_i ((matrix[j][i] mod t) mod q_l) * in[b][i]: bfv_scalar_plain_mul (advanced.rs:162-171:
// the scalar mod t as a constant plaintext, whose lift is the same residue in every slot) and bfv_add.
extern "C" int exacto_dbfv_linear_map_dev(exacto_ctx* c, size_t d_in, size_t d_out, size_t polys,
                                          const uint64_t* matrix, const uint64_t* in, uint64_t* out, size_t B) {
    if (int e = check_ctx(c)) return e;
    if (d_in < 1 || d_out < 1) return invalid_param("num_digits must be >= 1");
    if (d_in > 4096 || d_out > 4096) return invalid_param("linear map larger than 4096 digits");
    if (!matrix) return invalid_param("null matrix");
    if (B == 0 || polys == 0) return 0;
    if (!in || !out) return invalid_param("null ciphertext pointer");
    const size_t limb = polys * c->L * (size_t)c->n;
    if (in < out + B * d_out * limb && out < in + B * d_in * limb)
        return invalid_param("linear map output must not overlap its input");
    if (((uintptr_t)in | (uintptr_t)out) & 15) return invalid_param("linear map buffers must be 16-byte aligned");
    if (B * polys * c->L > ((size_t)1 << 31) / c->n * 256) return invalid_param("batch too large");
    // the non-zero entries row by row (the reference skips a zero coefficient, advanced.rs:138-140),
    // reduced per limb; a row without any is one empty term, so that every output limb is written
    const int L = c->L;
    std::vector<u64> tab;
    size_t E = 0;
    auto term = [&](u64 m, size_t col, bool last) {
        for (int l = 0; l < L; ++l) {
            const u64 q = c->primes[l], s = m % q;
            const u64 w[4] = {s, shoup_h(s, q), (u64)col | ((u64)(last ? 1 : 0) << 32), 0};
            tab.insert(tab.end(), w, w + 4);
        }
        ++E;
    };
    for (size_t j = 0; j < d_out; ++j) {
        size_t last_nz = d_in;
        for (size_t i = 0; i < d_in; ++i)
            if (matrix[j * d_in + i] % c->plain) last_nz = i;
        if (last_nz == d_in) term(0, 0, true);
        for (size_t i = 0; i <= last_nz && last_nz < d_in; ++i)
            if (const u64 m = matrix[j * d_in + i] % c->plain) term(m, i, i == last_nz);
    }
    static_assert(sizeof(LinTerm) == 4 * sizeof(u64), "LinTerm is four words: s, ss, {col, last}, pad");
    if (tab != c->lin_host) {  // the same map again (a circuit's repeated step): the resident table stands
        // the table is host-pageable and d_lin may still be read by a previous call's kernel
        HIP_TRY(hipStreamSynchronize(c->stream));
        c->lin_host.clear();
        if (c->d_lin.grow(tab.size() * sizeof(u64))) return EXACTO_ERR_HIP;
        if (int e_ = upload(c, c->d_lin, tab.data(), tab.size() * sizeof(u64))) return e_;
        c->lin_host = tab;
    }
    launch_dbfv_linmap(in, out, reinterpret_cast<const LinTerm*>(c->d_lin.get()), (int)E, (int)d_in, (int)d_out, (long)B,
                       (int)polys, c->n, L, c->d_primes, c->stream);
    CHECK_LAUNCH();
    return 0;
}

extern "C" int exacto_dbfv_linear_map(exacto_ctx* c, size_t d_in, size_t d_out, size_t polys, const uint64_t* matrix,
                                      const uint64_t* in, uint64_t* out, size_t B) {
    if (!c) return invalid_param("null context");
    const size_t lb = polys * c->L * poly_bytes(c);
    return host_call(c, {{in, B * d_in * lb}}, B * d_out * lb, out, [&](std::vector<u64*>& dv, u64* o) {
        return exacto_dbfv_linear_map_dev(c, d_in, d_out, polys, matrix, dv[0], o, B);
    });
}

// advanced.rs:104-130, 147-152: M[j][i] = digit j of (base^i mod p) in base new_base
static int change_base_matrix(size_t d, uint64_t base, uint64_t plain, uint64_t new_base, size_t new_d,
                              std::vector<u64>* M) {
    if (int e = dbfv_params_check(d, base, plain)) return e;
    if (new_base < 2) return invalid_param("new base must be >= 2");
    if (new_d == 0) return invalid_param("new_num_digits must be >= 1");
    if (int e = dbfv_params_check(new_d, new_base, plain)) return e;
    if (d > 4096 || new_d > 4096) return invalid_param("linear map larger than 4096 digits");
    M->assign(new_d * d, 0);
    u128 b_pow = 1;  // p = 2^64: the reduction is the truncation to 64 bits
    for (size_t i = 0; i < d; ++i) {
        u64 rem = plain ? (u64)(b_pow % plain) : (u64)b_pow;
        for (size_t j = 0; j < new_d; ++j) {
            (*M)[j * d + i] = rem % new_base;
            rem /= new_base;
        }
        b_pow = plain ? (b_pow * base) % plain : (u128)(u64)((u64)b_pow * base);
    }
    return 0;
}

extern "C" int exacto_dbfv_change_base_matrix(size_t d, uint64_t base, uint64_t plain, uint64_t new_base, size_t new_d,
                                              uint64_t* out) {
    std::vector<u64> M;
    if (int e = change_base_matrix(d, base, plain, new_base, new_d, &M)) return e;
    if (!out) return invalid_param("null matrix");
    std::memcpy(out, M.data(), M.size() * sizeof(u64));
    return 0;
}

extern "C" int exacto_dbfv_change_base_dev(exacto_ctx* c, size_t d, uint64_t base, uint64_t plain, uint64_t new_base,
                                           size_t new_d, const uint64_t* in, uint64_t* out, size_t B) {
    if (int e = check_ctx(c)) return e;
    std::vector<u64> M;
    if (int e = change_base_matrix(d, base, plain, new_base, new_d, &M)) return e;
    return exacto_dbfv_linear_map_dev(c, d, new_d, 2, M.data(), in, out, B);
}

extern "C" int exacto_dbfv_change_base(exacto_ctx* c, size_t d, uint64_t base, uint64_t plain, uint64_t new_base,
                                       size_t new_d, const uint64_t* in, uint64_t* out, size_t B) {
    if (!c) return invalid_param("null context");
    const size_t lb = 2 * c->L * poly_bytes(c);
    return host_call(c, {{in, B * d * lb}}, B * new_d * lb, out, [&](std::vector<u64*>& dv, u64* o) {
        return exacto_dbfv_change_base_dev(c, d, base, plain, new_base, new_d, dv[0], o, B);
    });
}

// advanced.rs:36-93: phi_b as a matrix: row 0 = (base^-1 mod t, 1, 0, ...), row i = e_{i+1}, last row 0
extern "C" int exacto_dbfv_div_by_base_dev(exacto_ctx* c, size_t d, uint64_t base, uint64_t plain, const uint64_t* in,
                                           uint64_t* out, size_t B, uint64_t* new_plain) {
    if (int e = check_ctx(c)) return e;
    if (int e = dbfv_params_check(d, base, plain)) return e;
    if (d > 4096) return invalid_param("linear map larger than 4096 digits");
    const u64 inv = invmod_h(base % c->plain, c->plain);
    if (inv == 0) return invalid_param("base not invertible modulo BFV plaintext modulus");
    const u128 old_p = plain == 0 ? ((u128)1 << 64) : (u128)plain;
    if (old_p % base != 0)
        return invalid_param("plaintext modulus " + u128_str(old_p) + " is not divisible by base " +
                             std::to_string(base));
    const u64 np = (u64)(old_p / base);  // base >= 2: below 2^64
    if (int e = dbfv_params_check(d, base, np)) return e;
    std::vector<u64> M(d * d, 0);
    M[0] = inv;
    for (size_t i = 0; i + 1 < d; ++i) M[i * d + i + 1] = 1;
    if (int e = exacto_dbfv_linear_map_dev(c, d, d, 2, M.data(), in, out, B)) return e;
    if (new_plain) *new_plain = np;
    return 0;
}

extern "C" int exacto_dbfv_div_by_base(exacto_ctx* c, size_t d, uint64_t base, uint64_t plain, const uint64_t* in,
                                       uint64_t* out, size_t B, uint64_t* new_plain) {
    if (!c) return invalid_param("null context");
    const size_t bytes = B * d * 2 * c->L * poly_bytes(c);
    return host_call(c, {{in, bytes}}, bytes, out, [&](std::vector<u64*>& dv, u64* o) {
        return exacto_dbfv_div_by_base_dev(c, d, base, plain, dv[0], o, B, new_plain);
    });
}

// ============================================================== dBFV plaintext products
// out = reduce(sum_k pt_k * ct_k) over digit vectors (dbfv_plain.hip): bfv_plain_mul per digit pair
// (bfv/eval.rs:468-486), bfv_add by i + j and over k, reduce (reduction.rs:15-93), in one kernel.

// Products a 128-bit accumulator of dbfv_plain.hip takes between two reductions: 2^(128 - 2s) - 2 for the
// largest prime's bit length s <= 62 (one slot for the carried residue, one to spare), at most 2^20.
static int dbfv_plain_flush_products(const exacto_ctx* c) {
    int s = 1;
    for (int l = 0; l < c->L; ++l) s = std::max(s, 64 - __builtin_clzll(c->primes[l]));
    const int e = 128 - 2 * s;
    return e >= 20 ? (1 << 20) : (1 << e) - 2;
}

extern "C" int exacto_ctx_set_dbfv_lt_fused(exacto_ctx* c, int on) {
    if (!c) return invalid_param("null context");
    c->dbfv_lt_fused = on != 0;
    return 0;
}

extern "C" int exacto_dbfv_plain_limits(exacto_ctx* c, size_t* flush_products, size_t* chunk_terms) {
    if (!c) return invalid_param("null context");
    if (flush_products) *flush_products = (size_t)dbfv_plain_flush_products(c);
    if (chunk_terms) *chunk_terms = c->plain_terms;
    return 0;
}

// The kernel's host tables in d_dp behind a two-word header {d, form}: d <= DP_MAX_D: rep[m - d][i] mod
// q_l as [L][d - 1][d]; above, the list form's pairs [E][L].  *live: the high limbs with a non-zero
// representative (a pair whose wide limb has none is never formed).
static int dbfv_plain_tables(exacto_ctx* c, size_t d, u64 base, u64 plain, unsigned* live, int* E) {
    const auto reps = small_reps(base, d, plain);
    const int L = c->L;
    const bool regs = d <= DP_MAX_D;
    std::vector<u64> tab{(u64)d, regs ? 0u : 1u};
    *live = 0;
    *E = 0;
    if (regs) {
        for (size_t m = 0; m + 1 < d; ++m)
            for (size_t i = 0; i < d; ++i)
                if (reps[m][i]) *live |= 1u << m;
        for (int l = 0; l < L; ++l)
            for (size_t m = 0; m + 1 < d; ++m)
                for (size_t i = 0; i < d; ++i) tab.push_back((u64)reps[m][i] % c->primes[l]);
    } else {
        static_assert(sizeof(DpPair) == 3 * sizeof(u64), "DpPair is three words: s, {ci, pi}, {last, pad}");
        auto pair = [&](u64 coef, size_t ci, size_t pi, bool last) {
            for (int l = 0; l < L; ++l) {
                const u64 w[3] = {coef % c->primes[l], (u64)ci | ((u64)pi << 32), last ? 1u : 0u};
                tab.insert(tab.end(), w, w + 3);
            }
            ++*E;
        };
        for (size_t i = 0; i < d; ++i) {
            std::vector<std::array<u64, 3>> row;
            for (size_t pi = 0; pi < d; ++pi)
                for (size_t ci = 0; ci < d; ++ci) {
                    const size_t m = pi + ci;
                    const u64 coef = m == i ? 1 : m >= d ? (u64)reps[m - d][i] : 0;
                    if (coef) row.push_back({coef, (u64)ci, (u64)pi});
                }
            if (row.empty()) pair(0, 0, 0, true);
            for (size_t e = 0; e < row.size(); ++e) pair(row[e][0], row[e][1], row[e][2], e + 1 == row.size());
        }
    }
    if (tab != c->dp_host) {
        // the table is host-pageable and d_dp may still be read by a previous call's kernel
        HIP_TRY(hipStreamSynchronize(c->stream));
        c->dp_host.clear();
        if (c->d_dp.grow(tab.size() * sizeof(u64))) return EXACTO_ERR_HIP;
        if (int e_ = upload(c, c->d_dp, tab.data(), tab.size() * sizeof(u64))) return e_;
        c->dp_host = tab;
    }
    return 0;
}

static bool ranges_overlap(const u64* a, size_t aw, const u64* b, size_t bw) { return a < b + bw && b < a + aw; }

// The checks of exacto_dbfv_plain_mul_sum[_dev], in the header's order
static int dbfv_plain_mul_check(exacto_ctx* c, size_t d, uint64_t base, uint64_t plain, const uint64_t* cts, size_t K,
                                size_t polys, const uint64_t* pts, size_t pt_batch, const uint64_t* out, size_t B,
                                const uint32_t* depth_ct, bool dev) {
    if (int e = check_ctx(c)) return e;
    if (!cts || !pts || !out) return invalid_param("null argument");
    if (K == 0) return invalid_param("mismatched ct/pt lengths");
    if (polys == 0) return invalid_param("ciphertext has no components");
    if (pt_batch != 1 && pt_batch != B) return invalid_param("plaintext batch must be 1 or the batch");
    if (int e = dbfv_params_check(d, base, plain)) return e;
    if (d > 64) return invalid_param("plaintext product larger than 64 digits");
    for (size_t i = 0; depth_ct && i < B * K; ++i)
        if (depth_ct[i] + 1 > 1)
            return fail(EXACTO_ERR_NOT_IMPLEMENTED, "not yet implemented: chained dBFV multiplication requires "
                                                    "ciphertext-level lattice reduction (paper §4.6.2)");
    if (dev && (((uintptr_t)cts | (uintptr_t)pts | (uintptr_t)out) & 15))
        return invalid_param("dbfv plain: buffers must be 16-byte aligned");
    const size_t n = (size_t)c->n, limb = polys * c->L * n;
    if (ranges_overlap(out, B * d * limb, cts, B * K * d * limb) || ranges_overlap(out, B * d * limb, pts, pt_batch * K * d * n))
        return invalid_param("dbfv plain: the output must not overlap an input");
    if (std::min<size_t>(c->chunk, B) * polys * c->L > ((size_t)1 << 31) / n * 256) return invalid_param("batch too large");
    return 0;
}

// pt rows [rows][n] (any u64) -> NTT(pt mod q_l) as [rows][L][n] at dst (inside pl_buf)
static int lift_plain_rows(exacto_ctx* c, const u64* pt, long rows, u64* dst) {
    launch_scale_plain(pt, nullptr, dst, rows, c->n, c->L, c->d_primes, c->stream);
    CHECK_LAUNCH();
    return ntt_items(c, dst, rows, (long)c->L * c->n, c->L);
}

extern "C" int exacto_dbfv_plain_mul_sum_dev(exacto_ctx* c, size_t d, uint64_t base, uint64_t plain,
                                             const uint64_t* cts, size_t K, size_t polys, const uint64_t* pts,
                                             size_t pt_batch, uint64_t* out, size_t B, const uint32_t* depth_ct,
                                             uint32_t* depth_out) {
    if (int e = dbfv_plain_mul_check(c, d, base, plain, cts, K, polys, pts, pt_batch, out, B, depth_ct, true)) return e;
    if (B == 0) return 0;
    unsigned live = 0;
    int E = 0;
    if (int e = dbfv_plain_tables(c, d, base, plain, &live, &E)) return e;
    const size_t n = (size_t)c->n, Ln = (size_t)c->L * n;
    const size_t ct_term = d * polys * Ln, ct_item = K * ct_term;
    const bool shared = pt_batch == 1;
    // term chunks of at most plain_terms terms (a later chunk adds into out), items in chunks of the
    // context's chunk; a shared plaintext is lifted once per term chunk, a per-item one per item chunk
    const size_t Kc = std::min(K, c->plain_terms), C = std::min<size_t>(c->chunk, B);
    if (int e = pl_scratch(c, (shared ? 1 : C) * Kc * d * Ln)) return e;
    DbfvPlainArgs a{};
    a.ct_item_stride = (long)ct_item; a.ct_term_stride = (long)ct_term;
    a.d = (int)d; a.polys = (int)polys; a.n = c->n; a.L = c->L;
    a.flush = dbfv_plain_flush_products(c);
    a.live = live;
    a.fold = c->d_dp.get() + 2;
    a.pairs = reinterpret_cast<const DpPair*>(c->d_dp.get() + 2);
    a.E = E;
    a.primes = c->d_primes;
    a.pl = c->pl_buf;
    for (size_t k0 = 0; k0 < K; k0 += Kc) {
        const size_t kc = std::min(Kc, K - k0);
        a.K = (int)kc;
        a.accum = k0 != 0;
        a.pl_term_stride = (long)(d * Ln);
        a.pl_item_stride = shared ? 0 : (long)(kc * d * Ln);
        for (size_t i0 = 0; i0 < B; i0 += C) {
            const size_t cnt = std::min(C, B - i0);
            if (shared) {
                if (i0 == 0)
                    if (int e = lift_plain_rows(c, pts + k0 * d * n, (long)(kc * d), c->pl_buf)) return e;
            } else if (kc == K) {
                if (int e = lift_plain_rows(c, pts + i0 * K * d * n, (long)(cnt * K * d), c->pl_buf)) return e;
            } else {
                for (size_t i = 0; i < cnt; ++i)
                    if (int e = lift_plain_rows(c, pts + ((i0 + i) * K + k0) * d * n, (long)(kc * d),
                                                c->pl_buf + i * kc * d * Ln))
                        return e;
            }
            a.cts = cts + i0 * ct_item + k0 * ct_term;
            a.out = out + i0 * d * polys * Ln;
            a.items = (long)cnt;
            launch_dbfv_plain_mul(a, c->stream);
            CHECK_LAUNCH();
        }
    }
    if (depth_out)
        for (size_t i = 0; i < B; ++i) depth_out[i] = 1;
    return 0;
}

extern "C" int exacto_dbfv_plain_mul_sum(exacto_ctx* c, size_t d, uint64_t base, uint64_t plain, const uint64_t* cts,
                                         size_t K, size_t polys, const uint64_t* pts, size_t pt_batch, uint64_t* out,
                                         size_t B, const uint32_t* depth_ct, uint32_t* depth_out) {
    if (int e = dbfv_plain_mul_check(c, d, base, plain, cts, K, polys, pts, pt_batch, out, B, depth_ct, false)) return e;
    if (B == 0) return 0;
    const size_t lb = polys * c->L * poly_bytes(c);
    return host_call(c, {{cts, B * K * d * lb}, {pts, pt_batch * K * d * poly_bytes(c)}}, B * d * lb, out,
                     [&](std::vector<u64*>& in, u64* o) {
                         return exacto_dbfv_plain_mul_sum_dev(c, d, base, plain, in[0], K, polys, in[1], pt_batch, o, B,
                                                              depth_ct, depth_out);
                     });
}

extern "C" int exacto_dbfv_plain_mul_dev(exacto_ctx* c, size_t d, uint64_t base, uint64_t plain, const uint64_t* ct,
                                         size_t polys, const uint64_t* pt, size_t pt_batch, uint64_t* out, size_t B,
                                         const uint32_t* depth_ct, uint32_t* depth_out) {
    return exacto_dbfv_plain_mul_sum_dev(c, d, base, plain, ct, 1, polys, pt, pt_batch, out, B, depth_ct, depth_out);
}
extern "C" int exacto_dbfv_plain_mul(exacto_ctx* c, size_t d, uint64_t base, uint64_t plain, const uint64_t* ct,
                                     size_t polys, const uint64_t* pt, size_t pt_batch, uint64_t* out, size_t B,
                                     const uint32_t* depth_ct, uint32_t* depth_out) {
    return exacto_dbfv_plain_mul_sum(c, d, base, plain, ct, 1, polys, pt, pt_batch, out, B, depth_ct, depth_out);
}

// Limb k of the output is bfv_plain_add (eval.rs:489-503) of limb k and plaintext digit k: c0 +- NTT(Delta m)
static int dbfv_plain_addsub_check(exacto_ctx* c, size_t d, const uint64_t* ct, size_t polys, const uint64_t* pt,
                                   size_t pt_batch, const uint64_t* out, size_t B) {
    if (int e = check_ctx(c)) return e;
    if (!ct || !pt || !out) return invalid_param("null argument");
    if (polys == 0) return invalid_param("ciphertext has no components");
    if (pt_batch != 1 && pt_batch != B) return invalid_param("plaintext batch must be 1 or the batch");
    if (d < 1) return invalid_param("num_digits must be >= 1");
    if (B > (size_t)INT32_MAX / d) return invalid_param("batch * num_digits too large");
    return 0;
}
static int dbfv_plain_addsub_dev(exacto_ctx* c, bool sub, size_t d, const uint64_t* ct, size_t polys,
                                 const uint64_t* pt, size_t pt_batch, uint64_t* out, size_t B) {
    if (int e = dbfv_plain_addsub_check(c, d, ct, polys, pt, pt_batch, out, B)) return e;
    if (B == 0) return 0;
    if (int e = lift_plain(c, pt, (long)(pt_batch * d), true)) return e;
    const long Ln = (long)c->L * c->n;
    launch_plain_apply(sub ? PLAIN_SUB : PLAIN_ADD, ct, (long)polys * Ln, out, (long)(B * d), (int)polys, c->pl_buf, Ln,
                       c->n, c->L, c->d_primes, c->stream, pt_batch == B ? 0 : (long)d);
    CHECK_LAUNCH();
    return 0;
}
static int dbfv_plain_addsub_host(exacto_ctx* c, bool sub, size_t d, const uint64_t* ct, size_t polys,
                                  const uint64_t* pt, size_t pt_batch, uint64_t* out, size_t B) {
    if (int e = dbfv_plain_addsub_check(c, d, ct, polys, pt, pt_batch, out, B)) return e;
    if (B == 0) return 0;
    const size_t bytes = B * d * polys * c->L * poly_bytes(c);
    return host_call(c, {{ct, bytes}, {pt, pt_batch * d * poly_bytes(c)}}, bytes, out,
                     [&](std::vector<u64*>& in, u64* o) {
                         return dbfv_plain_addsub_dev(c, sub, d, in[0], polys, in[1], pt_batch, o, B);
                     });
}
extern "C" int exacto_dbfv_plain_add_dev(exacto_ctx* c, size_t d, const uint64_t* ct, size_t polys, const uint64_t* pt,
                                         size_t pt_batch, uint64_t* out, size_t B) {
    return dbfv_plain_addsub_dev(c, false, d, ct, polys, pt, pt_batch, out, B);
}
extern "C" int exacto_dbfv_plain_sub_dev(exacto_ctx* c, size_t d, const uint64_t* ct, size_t polys, const uint64_t* pt,
                                         size_t pt_batch, uint64_t* out, size_t B) {
    return dbfv_plain_addsub_dev(c, true, d, ct, polys, pt, pt_batch, out, B);
}
extern "C" int exacto_dbfv_plain_add(exacto_ctx* c, size_t d, const uint64_t* ct, size_t polys, const uint64_t* pt,
                                     size_t pt_batch, uint64_t* out, size_t B) {
    return dbfv_plain_addsub_host(c, false, d, ct, polys, pt, pt_batch, out, B);
}
extern "C" int exacto_dbfv_plain_sub(exacto_ctx* c, size_t d, const uint64_t* ct, size_t polys, const uint64_t* pt,
                                     size_t pt_batch, uint64_t* out, size_t B) {
    return dbfv_plain_addsub_host(c, true, d, ct, polys, pt, pt_batch, out, B);
}

// ============================================================== dBFV hoisted rotations and linear transforms
// The join of the hoisted rotations with the plaintext products ("dBFV linear transforms"):
// out = reduce(sum_r W_r * rot_r(x)), bit for bit exacto_dbfv_plain_mul_sum over exacto_bfv_rotate_hoisted's
// rotations of the limbs.  hoist_core runs it with the limbs of a ciphertext as one group.

static int dbfv_hoist_rotate_check(exacto_ctx* c, const exacto_galois_keyset* ks, size_t d, const uint64_t* ct,
                                   const uint64_t* out, size_t B) {
    if (int e = check_ctx(c)) return e;
    if (int e = hoist_check(c, ks)) return e;
    if (d < 1) return invalid_param("num_digits must be >= 1");
    if (d > 4096) return invalid_param("more than 4096 digits");
    if (B == 0) return 0;
    if (!ct || !out) return invalid_param("null argument");
    return 0;
}

extern "C" int exacto_dbfv_rotate_hoisted_dev(exacto_ctx* c, const exacto_galois_keyset* ks, size_t d,
                                              const uint64_t* ct, uint64_t* out, size_t B) {
    if (int e = dbfv_hoist_rotate_check(c, ks, d, ct, out, B)) return e;
    HoistDbfv dv;
    dv.d = (int)d;
    return hoist_core(c, ks, ct, nullptr, false, out, B * d, &dv);
}

extern "C" int exacto_dbfv_rotate_hoisted(exacto_ctx* c, const exacto_galois_keyset* ks, size_t d, const uint64_t* ct,
                                          uint64_t* out, size_t B) {
    if (int e = dbfv_hoist_rotate_check(c, ks, d, ct, out, B)) return e;
    if (B == 0) return 0;
    const size_t ctb = B * d * 2 * c->L * poly_bytes(c);
    return host_call(c, {{ct, ctb}}, ctb * ks->R, out, [&](std::vector<u64*>& in, u64* o) {
        return exacto_dbfv_rotate_hoisted_dev(c, ks, d, in[0], o, B);
    });
}

// Lifted diagonals [R][d][L][n], resident on the device
struct exacto_dbfv_diagonals {
    int device = 0, n = 0, L = 0;
    std::vector<u64> primes;
    size_t R = 0, d = 0;
    bool fused = false;      // dbfv_lt_fused_route of the context it was made on, when it was made
    DevBuf<u64> d_pl;
};

// The route of a dBFV linear transform on this context: the fused kernel on the limb-wise key switch with
// at most DP_MAX_D digits, else rotations into scratch and the plaintext-product kernel
static bool dbfv_lt_fused_route(const exacto_ctx* c, size_t d) {
    return c->dbfv_lt_fused && !hoist_k32(c) && d <= DP_MAX_D;
}

extern "C" void exacto_dbfv_diagonals_destroy(exacto_dbfv_diagonals* dg) {
    if (!dg) return;
    (void)hipSetDevice(dg->device);
    delete dg;
}

extern "C" int exacto_dbfv_diagonals_info(const exacto_dbfv_diagonals* dg, size_t* R, size_t* d, int* fused) {
    if (!dg) return invalid_param("null diagonals");
    if (R) *R = dg->R;
    if (d) *d = dg->d;
    if (fused) *fused = dg->fused ? 1 : 0;
    return 0;
}

extern "C" int exacto_dbfv_diagonals_create_dev(exacto_ctx* c, size_t d, size_t R, const uint64_t* pts,
                                                exacto_dbfv_diagonals** out) {
    if (int e = check_ctx(c)) return e;
    if (!out || !pts) return invalid_param("null argument");
    *out = nullptr;
    if (d < 1) return invalid_param("num_digits must be >= 1");
    if (d > 64) return invalid_param("plaintext product larger than 64 digits");
    if (R == 0) return invalid_param("diagonals need at least one rotation");
    if (R > 65535) return invalid_param("at most 65535 diagonals");
    std::unique_ptr<exacto_dbfv_diagonals, void (*)(exacto_dbfv_diagonals*)> dg(new exacto_dbfv_diagonals,
                                                                                exacto_dbfv_diagonals_destroy);
    dg->device = c->device; dg->n = c->n; dg->L = c->L;
    dg->primes.assign(c->primes.begin(), c->primes.begin() + c->L);
    dg->R = R; dg->d = d;
    dg->fused = dbfv_lt_fused_route(c, d);
    if (int e = dg->d_pl.alloc(R * d * c->L * poly_bytes(c))) return e;
    if (int e = lift_plain_rows(c, pts, (long)(R * d), dg->d_pl)) return e;
    // the caller's pts may go once this returns
    HIP_TRY(hipStreamSynchronize(c->stream));
    *out = dg.release();
    return 0;
}

extern "C" int exacto_dbfv_diagonals_create(exacto_ctx* c, size_t d, size_t R, const uint64_t* pts,
                                            exacto_dbfv_diagonals** out) {
    if (int e = check_ctx(c)) return e;
    if (!out || !pts || d < 1 || d > 64 || R == 0 || R > 65535)   // nothing to stage: the device form's checks
        return exacto_dbfv_diagonals_create_dev(c, d, R, pts, out);
    const size_t bytes = R * d * poly_bytes(c);
    DevBuf<u64> dp;
    if (int e = dp.alloc(bytes)) return e;
    if (int e = upload(c, dp, pts, bytes)) return e;
    return exacto_dbfv_diagonals_create_dev(c, d, R, dp, out);
}

// The checks of exacto_dbfv_linear_transform[_prepared][_dev], in the header's order; exactly one of pts, dg
static int dbfv_lt_check(exacto_ctx* c, const exacto_galois_keyset* ks, size_t d, uint64_t base, uint64_t plain,
                         const uint64_t* ct, const uint64_t* pts, const exacto_dbfv_diagonals* dg, bool prepared,
                         const uint64_t* out, size_t B, const uint32_t* depth_ct, bool dev) {
    if (int e = check_ctx(c)) return e;
    if (!ks) return invalid_param("null key set");
    if (!ct || !out || (prepared ? !dg : !pts)) return invalid_param("null argument");
    if (int e = hoist_check(c, ks)) return e;
    if (int e = dbfv_params_check(d, base, plain)) return e;
    if (d > 64) return invalid_param("plaintext product larger than 64 digits");
    if (prepared) {
        if (dg->n != c->n || dg->L != c->L || dg->device != c->device ||
            !std::equal(dg->primes.begin(), dg->primes.end(), c->primes.begin()))
            return invalid_param("diagonals were prepared on a context with other parameters");
        if (dg->R != ks->R || dg->d != d)
            return invalid_param("diagonals were prepared for " + std::to_string(dg->R) + " rotations of " +
                                 std::to_string(dg->d) + " digits, not " + std::to_string(ks->R) + " of " +
                                 std::to_string(d));
    }
    for (size_t i = 0; depth_ct && i < B; ++i)
        if (depth_ct[i] + 1 > 1)
            return fail(EXACTO_ERR_NOT_IMPLEMENTED, "not yet implemented: chained dBFV multiplication requires "
                                                    "ciphertext-level lattice reduction (paper §4.6.2)");
    if (dev && (((uintptr_t)ct | (uintptr_t)pts | (uintptr_t)out) & 15))
        return invalid_param("dbfv linear transform: buffers must be 16-byte aligned");
    const size_t n = (size_t)c->n, ctw = B * d * 2 * c->L * n;
    if (ranges_overlap(out, ctw, ct, ctw) || (pts && ranges_overlap(out, ctw, pts, ks->R * d * n)))
        return invalid_param("dbfv linear transform: the output must not overlap an input");
    return 0;
}

static int dbfv_lt_dev(exacto_ctx* c, const exacto_galois_keyset* ks, size_t d, uint64_t base, uint64_t plain,
                       const uint64_t* ct, const uint64_t* pts, const exacto_dbfv_diagonals* dg, bool prepared,
                       uint64_t* out, size_t B, const uint32_t* depth_ct, uint32_t* depth_out) {
    if (int e = dbfv_lt_check(c, ks, d, base, plain, ct, pts, dg, prepared, out, B, depth_ct, true)) return e;
    if (B == 0) return 0;
    unsigned live = 0;
    int E = 0;
    if (int e = dbfv_plain_tables(c, d, base, plain, &live, &E)) return e;
    const size_t n = (size_t)c->n, Ln = (size_t)c->L * n, R = ks->R;
    DbfvPlainArgs a{};
    a.d = (int)d; a.polys = 2; a.n = c->n; a.L = c->L;
    a.flush = dbfv_plain_flush_products(c);
    a.live = live;
    a.fold = c->d_dp.get() + 2;
    a.pairs = reinterpret_cast<const DpPair*>(c->d_dp.get() + 2);
    a.E = E;
    a.primes = c->d_primes;
    a.pl_term_stride = (long)(d * Ln);
    a.pl_item_stride = 0;
    HoistDbfv dv;
    dv.d = (int)d;
    dv.prod = &a;
    dv.fused = dbfv_lt_fused_route(c, d);
    // raw diagonals: plain_terms rotations at a time through pl_buf, a later group adding into out
    const size_t Rc = prepared ? R : std::min(R, c->plain_terms);
    if (!prepared)
        if (int e = pl_scratch(c, Rc * d * Ln)) return e;
    for (size_t r0 = 0; r0 < R; r0 += Rc) {
        const size_t rc = std::min(Rc, R - r0);
        if (!prepared)
            if (int e = lift_plain_rows(c, pts + r0 * d * n, (long)(rc * d), c->pl_buf)) return e;
        a.pl = prepared ? dg->d_pl.get() : c->pl_buf.get();
        a.accum = r0 != 0;
        dv.r0 = r0; dv.rc = rc;
        if (int e = hoist_core(c, ks, ct, nullptr, false, out, B * d, &dv)) return e;
    }
    if (depth_out)
        for (size_t i = 0; i < B; ++i) depth_out[i] = 1;
    return 0;
}

extern "C" int exacto_dbfv_linear_transform_dev(exacto_ctx* c, const exacto_galois_keyset* ks, size_t d, uint64_t base,
                                                uint64_t plain, const uint64_t* ct, const uint64_t* pts, uint64_t* out,
                                                size_t B, const uint32_t* depth_ct, uint32_t* depth_out) {
    return dbfv_lt_dev(c, ks, d, base, plain, ct, pts, nullptr, false, out, B, depth_ct, depth_out);
}

extern "C" int exacto_dbfv_linear_transform_prepared_dev(exacto_ctx* c, const exacto_galois_keyset* ks, size_t d,
                                                         uint64_t base, uint64_t plain, const uint64_t* ct,
                                                         const exacto_dbfv_diagonals* dg, uint64_t* out, size_t B,
                                                         const uint32_t* depth_ct, uint32_t* depth_out) {
    return dbfv_lt_dev(c, ks, d, base, plain, ct, nullptr, dg, true, out, B, depth_ct, depth_out);
}

extern "C" int exacto_dbfv_linear_transform(exacto_ctx* c, const exacto_galois_keyset* ks, size_t d, uint64_t base,
                                            uint64_t plain, const uint64_t* ct, const uint64_t* pts, uint64_t* out,
                                            size_t B, const uint32_t* depth_ct, uint32_t* depth_out) {
    if (int e = dbfv_lt_check(c, ks, d, base, plain, ct, pts, nullptr, false, out, B, depth_ct, false)) return e;
    if (B == 0) return 0;
    const size_t ctb = B * d * 2 * c->L * poly_bytes(c);
    return host_call(c, {{ct, ctb}, {pts, ks->R * d * poly_bytes(c)}}, ctb, out, [&](std::vector<u64*>& in, u64* o) {
        return exacto_dbfv_linear_transform_dev(c, ks, d, base, plain, in[0], in[1], o, B, depth_ct, depth_out);
    });
}

extern "C" int exacto_dbfv_linear_transform_prepared(exacto_ctx* c, const exacto_galois_keyset* ks, size_t d,
                                                     uint64_t base, uint64_t plain, const uint64_t* ct,
                                                     const exacto_dbfv_diagonals* dg, uint64_t* out, size_t B,
                                                     const uint32_t* depth_ct, uint32_t* depth_out) {
    if (int e = dbfv_lt_check(c, ks, d, base, plain, ct, nullptr, dg, true, out, B, depth_ct, false)) return e;
    if (B == 0) return 0;
    const size_t ctb = B * d * 2 * c->L * poly_bytes(c);
    return host_call(c, {{ct, ctb}}, ctb, out, [&](std::vector<u64*>& in, u64* o) {
        return exacto_dbfv_linear_transform_prepared_dev(c, ks, d, base, plain, in[0], dg, o, B, depth_ct, depth_out);
    });
}

// ============================================================== diagnostics

extern "C" size_t exacto_last_error(char* buf, size_t len) {
    if (buf && len) {
        const size_t m = std::min(len - 1, g_last_error.size());
        std::memcpy(buf, g_last_error.data(), m);
        buf[m] = 0;
    }
    return g_last_error.size();
}

extern "C" int exacto_prof_enable(exacto_ctx* c, int enable) {
    if (!c) return invalid_param("null context");
    c->prof = enable != 0;
    return 0;
}

extern "C" int exacto_prof_read(exacto_ctx* c, int kind, uint64_t* launches, double* total_ms, double* total_bytes,
                                uint64_t* polys) {
    if (!c) return invalid_param("null context");
    HIP_TRY(hipStreamSynchronize(c->stream));
    u64 nl = 0, np = 0;
    double ms = 0, by = 0;
    std::vector<ProfRec> keep;
    std::vector<double> rate;   // bytes per ms of each launch
    for (auto& r : c->recs) {
        if (r.kind != kind) { keep.push_back(r); continue; }
        float t = 0;
        HIP_TRY(hipEventElapsedTime(&t, r.a, r.b));
        ms += t; by += r.bytes; np += r.polys; ++nl;
        if (t > 0) rate.push_back(r.bytes / t);
        if (r.kern) {
            auto& k = c->prof_kern[kind][r.kern];
            k.first += 1;
            k.second += t;
        }
        (void)hipEventDestroy(r.a);
        (void)hipEventDestroy(r.b);
    }
    c->recs.swap(keep);
    // Robust total: the family's bytes at the MEDIAN per-launch rate.  An event pair can also span a
    // host-side gap before its launch reaches an idle stream (seen once: a cfg5 inverse family at 3x
    // its rocprofv3 durations in one run); the median ignores such a launch.  EXACTO_PROF_RAW=1 sums
    // the raw intervals.
    static const bool raw = [] { const char* e = getenv("EXACTO_PROF_RAW"); return e && atoi(e) != 0; }();
    if (!raw && !rate.empty()) {
        std::sort(rate.begin(), rate.end());
        const size_t m = rate.size();
        const double med = m % 2 ? rate[m / 2] : 0.5 * (rate[m / 2 - 1] + rate[m / 2]);
        if (med > 0) ms = by / med;
    }
    if (launches) *launches = nl;
    if (total_ms) *total_ms = ms;
    if (total_bytes) *total_bytes = by;
    if (polys) *polys = np;
    return 0;
}

// The kernels behind one profiled family in the records exacto_prof_read consumed since the last
// exacto_prof_kernels call for it, as rocprofv3 names them (the demangled kernel symbol without its
// "void " and parameter list), by descending event time: "name (launches, ms); name (...)".  Returns
// the length of the full text (like snprintf); buf may be NULL (a size query).  A call with a buffer
// clears the list.
static std::string kernel_symbol_name(const void* handle) {
    Dl_info info{};
    if (!dladdr(handle, &info) || !info.dli_sname) return "?";
    int st = 0;
    char* dm = abi::__cxa_demangle(info.dli_sname, nullptr, nullptr, &st);
    std::string nm = (st == 0 && dm) ? dm : info.dli_sname;
    free(dm);
    if (nm.rfind("void ", 0) == 0) nm = nm.substr(5);
    int depth = 0;   // cut the parameter list: the first '(' outside template brackets
    for (size_t i = 0; i < nm.size(); ++i) {
        if (nm[i] == '<') ++depth;
        else if (nm[i] == '>') --depth;
        else if (nm[i] == '(' && depth == 0) { nm.resize(i); break; }
    }
    return nm;
}

extern "C" size_t exacto_prof_kernels(exacto_ctx* c, int kind, char* buf, size_t len) {
    if (!c) return 0;
    std::vector<std::pair<double, std::string>> v;
    for (auto& kv : c->prof_kern[kind]) {
        char tail[64];
        snprintf(tail, sizeof tail, " (%llu, %.3f ms)", (unsigned long long)kv.second.first, kv.second.second);
        v.emplace_back(kv.second.second, kernel_symbol_name(kv.first) + tail);
    }
    if (buf && len) c->prof_kern.erase(kind);   // a size query (buf NULL) keeps the list
    std::sort(v.begin(), v.end(), [](const auto& a, const auto& b) { return a.first > b.first; });
    std::string out;
    for (auto& e : v) out += (out.empty() ? "" : "; ") + e.second;
    if (buf && len) {
        const size_t k = std::min(len - 1, out.size());
        std::memcpy(buf, out.data(), k);
        buf[k] = 0;
    }
    return out.size();
}

extern "C" const char* exacto_version(void) { return "exacto-hip 0.4.0 (gfx950)"; }
