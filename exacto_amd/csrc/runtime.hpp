// Internal header of the host runtime of libexacto_hip.so: what more than one host module uses.
// The types that own a context's state, the error and launch macros, and the declarations of the
// helpers shared between context.hip and the api_*.hip / rccl.hip modules (each is defined once,
// in the file named above its declaration).  Everything is in namespace exacto, except exacto_ctx,
// which is the C ABI's opaque type.
#pragma once

#include <algorithm>
#include <array>
#include <cxxabi.h>
#include <dlfcn.h>
#include <chrono>
#include <condition_variable>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <map>
#include <memory>
#include <mutex>
#include <set>
#include <string>
#include <thread>
#include <type_traits>
#include <vector>

#include "../../include/exacto_hip.h"
#include "exacto_internal.hpp"

namespace exacto {

// ============================================================== errors

// (context.hip) the one error state of the library: exacto_last_error reads what fail() stored
int fail(int code, const std::string& msg);
int invalid_param(const std::string& s);

#define HIP_TRY(x)                                                                              \
    do {                                                                                        \
        hipError_t e_ = (x);                                                                    \
        if (e_ != hipSuccess)                                                                   \
            return fail(EXACTO_ERR_HIP, std::string("HIP error: ") + hipGetErrorString(e_) +    \
                                            " (" #x ")");                                       \
    } while (0)

#define CHECK_LAUNCH()                                                                          \
    do {                                                                                        \
        hipError_t e_ = hipGetLastError();                                                      \
        if (e_ != hipSuccess)                                                                   \
            return fail(EXACTO_ERR_HIP, std::string("HIP launch error: ") + hipGetErrorString(e_)); \
    } while (0)

// (context.hip) every device allocation and release, as the owning types below make them
void free_dev(void* p);
hipError_t dev_alloc(void** p, size_t bytes);

// --- minimal unsigned big integer (little-endian 64-bit words) ---
struct Big {
    std::vector<u64> w;
    Big(u64 v = 0) { w.push_back(v); trim(); }
    void trim() { while (w.size() > 1 && w.back() == 0) w.pop_back(); }
    void mul(u64 m) {
        u64 c = 0;
        for (auto& x : w) { u128 t = (u128)x * m + c; x = (u64)t; c = (u64)(t >> 64); }
        if (c) w.push_back(c);
        trim();
    }
    void add(u64 a) {
        for (size_t i = 0; i < w.size() && a; ++i) { u64 s = w[i] + a; a = s < a; w[i] = s; }
        if (a) w.push_back(a);
    }
    void add(const Big& o) {
        u64 carry = 0;
        for (size_t i = 0; i < std::max(w.size(), o.w.size()) || carry; ++i) {
            if (i == w.size()) w.push_back(0);
            const u128 t = (u128)w[i] + (i < o.w.size() ? o.w[i] : 0) + carry;
            w[i] = (u64)t;
            carry = (u64)(t >> 64);
        }
        trim();
    }
    void shr1() {
        for (size_t i = 0; i < w.size(); ++i) w[i] = (w[i] >> 1) | (i + 1 < w.size() ? w[i + 1] << 63 : 0);
        trim();
    }
    u64 mod(u64 m) const {
        u128 r = 0;
        for (size_t i = w.size(); i-- > 0;) r = ((r << 64) | w[i]) % m;
        return (u64)r;
    }
    int cmp(const Big& o) const {
        if (w.size() != o.w.size()) return w.size() < o.w.size() ? -1 : 1;
        for (size_t i = w.size(); i-- > 0;)
            if (w[i] != o.w[i]) return w[i] < o.w[i] ? -1 : 1;
        return 0;
    }
};

// ============================================================== context

struct ProfRec {
    int kind;
    hipEvent_t a, b;
    u64 polys;
    double bytes;
    const void* kern;   // host handle of the last kernel launched inside the scope (EXACTO_LAUNCH)
};

// A device buffer that owns its memory.  Move-only; released through free_dev when its owner goes, so
// every release reaches the EXACTO_DEBUG_ALLOC log.  It converts to its pointer, so the launchers take
// it as they took the raw pointer; nothing outside the type assigns the pointer or the capacity.
template <class T>
class DevBuf {
    T* p_ = nullptr;
    size_t cap_ = 0;   // bytes
public:
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    DevBuf(DevBuf&& o) noexcept : p_(o.p_), cap_(o.cap_) { o.p_ = nullptr; o.cap_ = 0; }
    DevBuf& operator=(DevBuf&& o) noexcept {
        if (this != &o) {
            reset();
            p_ = o.p_; cap_ = o.cap_;
            o.p_ = nullptr; o.cap_ = 0;
        }
        return *this;
    }
    ~DevBuf() { reset(); }
    operator T*() const { return p_; }
    T* get() const { return p_; }
    size_t bytes() const { return cap_; }
    void reset() {
        free_dev(p_);
        p_ = nullptr;
        cap_ = 0;
    }
    // exactly `bytes` (the tables allocated once, the workspaces): what it held is released first
    int alloc(size_t bytes) {
        reset();
        HIP_TRY(dev_alloc((void**)&p_, bytes));
        cap_ = bytes;
        return 0;
    }
    // at least max(bytes, 8): nothing when the capacity suffices, else free first, then allocate (the
    // old and the new block are never live together).  A failure leaves the buffer empty.
    int grow(size_t bytes) {
        bytes = std::max<size_t>(bytes, 8);
        return cap_ >= bytes ? 0 : alloc(bytes);
    }
};
static_assert(!std::is_copy_constructible<DevBuf<u64>>::value && !std::is_copy_assignable<DevBuf<u64>>::value,
              "a device buffer has one owner");

// A 31-bit auxiliary basis of the ks32 key switch (ks32.hip) with its device tables and the
// relinearisation key converted to it.
struct Ks32Basis {
    int S = 0;
    int sum_max = 0;              // dBFV key-switch sums the basis lifts exactly
    int fpc_max = 0;              // ... and by the float-CRT lift (ks32_fpc_one's margin; S <= 3 or p < 2^32 / 3)
    int mac_form = 0;             // ks32_mac: 0 primes up to 2^31 (7 products per reduction),
                                  // 1 below 2^32 / 3 (12), 2 below 2^30 (12, lazy transforms)
    Big P;                        // product of the primes
    DevBuf<Prime32> d_p32;
    DevBuf<uint2> d_tw32;
    DevBuf<Ks32Tables> d_kst;
    DevBuf<uint32_t> d_rs;        // the relinearisation key in this basis
    bool rs_valid = false;
};
static_assert(!std::is_copy_constructible<Ks32Basis>::value && !std::is_copy_assignable<Ks32Basis>::value,
              "a basis owns its tables");

// The per-chunk workspace of one pipeline lane, sized in items (products) by ensure().
struct Workspace {
    size_t items = 0;
    DevBuf<u64> coefQ, extP, T, D;
    // exact path with gadget base <= 2^16: the scale kernel writes each digit once as int16 and
    // the digit NTT converts it per limb on load (EXACTO_DIGIT16=0: u64 digits per limb)
    DevBuf<int16_t> D16;
    DevBuf<uint32_t> DS, U;   // ks32: digit residues [item][G][S][n] and accumulators [item][2L][S][n]
    int ensure(const exacto_ctx* c, size_t want);
};

// Stream and per-chunk workspace of one extra pipeline lane (lane 0 is the context's own).
constexpr int EXACTO_MAX_LANES = 4;
struct LaneSet {
    hipStream_t stream = nullptr;
    hipEvent_t join = nullptr;
    Workspace ws;
};

}  // namespace exacto

// exacto_ctx is the C ABI's opaque type (include/exacto_hip.h), so it is defined at global scope, between
// the two halves of the namespace: after the types it owns and before ProfScope, which needs it complete.
// The using-directive at file scope is deliberate: the struct names its field types unqualified, as it
// always has, and every host module that includes this header says the same on its first lines.
using namespace exacto;

struct exacto_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    int n = 0, logn = 0, L = 0, K = 0;
    std::vector<u64> ctq, user_aux, int_aux, primes;  // primes = ctq ++ (path aux)
    u64 plain = 0, gbase = 0;
    int G = 0;
    int path = EXACTO_PATH_EXACT_RNS;
    int deferred_code = 0;  // error raised at multiplication time (reference semantics)
    std::string deferred_msg;
    DevBuf<PrimeConst> d_primes;
    DevBuf<TwPair> d_tw;
    DevBuf<CrtTables> d_crt;
    CrtTables h_crt{};
    DevBuf<u64> d_scal;
    DevBuf<u64> d_rlk;
    DevBuf<u64> d_rlk_s;  // Shoup companions of the key (limb-wise relinearisation MAC)
    size_t rlk_keys = 0;
    bool rlk_s_valid = false;
    // EXACTO_NTT_ASM=0: no special-prime (2^60 - d) asm rounds; those batches then take the generated
    // generic-prime asm rounds where their size has them (n = 1024 / 4096 / 8192, lazy primes), and the
    // compiler-scheduled C++ rounds only with EXACTO_NTT_GEN=0 as well (A/B switches)
    bool ntt_asm = true;
    bool ntt_asm_inv = true;  // EXACTO_NTT_ASM_INV=0: compiler-scheduled inverse NTT (A/B)
    // relinearisation MAC in an auxiliary basis of S 31-bit primes (ks32.hip; EXACTO_KS32=0: the
    // limb-wise 60-bit digit NTTs + relin_mac)
    bool ks32 = true;
    int S32 = 0;                 // 0: not eligible for these parameters
    int ks32_sum_max = 0;        // key-switch sums that may be added before one lift (prod p bound)
    int ks32_fpc_max = 0;        // ... that the active basis' float-CRT lift takes (Ks32Basis::fpc_max)
    bool ks_fpc = true;          // EXACTO_KS_FPC=0: the Garner lift in ks32_crt always (A/B)
    int ks32_mac_form = 0;       // ks32_mac's reduction form for the active basis (Ks32Basis::mac_form)
    Ks32Basis kw;                // wide basis (primes up to 2^31) for dBFV digit sums the primary cannot hold
    // The primary basis is one of two, chosen per relinearisation key (ensure_rs):
    //   kn: narrow primes below 2^32 / 3 bounding |sum_g d_g * r_g| by G n ceil(B/2) (q/2) for ANY key;
    //   kz: lazy primes below 2^30 (cheaper 32-bit butterflies, ks32_dev.hpp), used when the resident
    //       key's own L1 norms bound the sum: |u_{c,l}| <= ceil(B/2) sum_g ||r_{g,c,l}||_1 < prod p / 2
    //       (a uniform key has ||r||_1 ~ n q / 4: half the generic bound).  EXACTO_KS32_LAZY=0: kn only.
    // S32 / d_p32 / d_tw32 / d_kst / ks32_sum_max / ks32_mac_form describe the active one.
    Ks32Basis kn, kz;
    bool ks32_lazy_active = false;
    int ks32_need_m = 1;          // the most key-switch sums per output limb a dbfv_mul of this context asked for
    int last_dbfv_ks = -1;        // exacto_ctx_info.dbfv_key_switch
    int last_mul_sum_mode = -1;   // exacto_bfv_mul_sum_info: the same codes for the last bfv_mul_sum
    size_t mul_sum_cap = 0;       // exacto_ctx_set_mul_sum_group (0: the context's own limit)
    // a dBFV pass with shared extensions: d and its products per item (0: plain BFV products), for
    // run_inv_tensor's algorithmic bytes and the tensor kernels' prime-major block order
    int tensor_share_d = 0, tensor_share_npairs = 0;
    // dBFV chain: the step that formed the output limbs in the coefficient domain also lifted them to
    // the auxiliary primes into ext_a and transformed both in one launch; the next step's extension of
    // its left operand is then already in ext_a (measured A/B: DESIGN.md §6.4)
    bool ext_a_ready = false;
    // (a view of d_dall, not owned) run_mul: int16 digits of product p to ks_defer + p G n, no key switch
    int16_t* ks_defer = nullptr;
    bool ks_defer8 = false;       // ... int8 digits instead (base <= 2^8; EXACTO_DIGIT8=0: int16)
    bool digit8_env = true;
    // dBFV psum (EXACTO_PSUM=0: off): an output limb's c0 / c1 scaled once from the sum of its
    // products' tensors in the auxiliary primes (run_mul, dbfv_mul_core); psum_max = the largest
    // product count m with m (p n Q + 2) < P, so that the summed rounding stays liftable from P
    bool psum_env = true;
    // dBFV linear transforms on the limb-wise key switch: the staged route (rotations into scratch, then the
    // plaintext-product kernel) unless exacto_ctx_set_dbfv_lt_fused(ctx, 1) selects dbfv_hoist.hip's fused
    // kernel, which measured half as fast; the switch is for tests and measurements
    bool dbfv_lt_fused = false;
    bool square_hook = true;     // eval_poly's baby steps x^(i/2) x^(i/2) on the square path (exacto_ctx_set_square_hook)
    int psum_max = 0;
    int psum_fp_max = 0;         // ... and with |sum| < P / 4, the rounded-float CRT over P (kernels.hip fpc_lift)
    bool fp_crt = true;          // EXACTO_FP_CRT=0: Garner over P in the SP scale kernels (A/B)
    // the scale kernels' s = [p T]_Q by a rounded float sum (with fp_crt; kernels.hip fpq_y) wherever
    // |f - round(f)| <= fpq_lim.  EXACTO_FPQ=0: Garner over Q always; =2: a 1/4 band (half the
    // coefficients take Garner: the fallback's bit-exact variant)
    double fpq_lim = 0.5 - 0x1p-40;
    // HPS: the division-free scale (q > 2^32, p < min(q, 2^32); EXACTO_HPS_LITERAL=1: the literal i128
    // form, kept for the equivalence test) and, in dbfv_mul, the products' c0 / c1 and signed gadget
    // digits summed per output limb before ONE forward NTT + relinearisation MAC per limb
    // (EXACTO_HPS_SUM=0: per product)
    bool hps_fast = false;
    bool hps_sum_env = true;
    struct PsumPlan {
        bool on = false;
        int d = 0, npairs = 0;
        const int* term_start = nullptr;
        const CombineTerm* terms = nullptr;
        u64* out = nullptr;       // [B][d][2][L][n], coefficient domain (a view: the caller's buffer)
        bool fpc = false;         // its scale may take the rounded-float CRT over P (m <= psum_fp_max)
    } psum;
    DevBuf<u64> d_hdig;          // dBFV over HPS: the summed digits' NTT residues [B][d][G][L][n]
    DevBuf<int16_t> d_dall;      // dBFV: per-product digits
    DevBuf<void> d_dk;           // ... and their per-limb sums (int16, or int32 when m ceil(B/2) > 2^15 - 1)
    DevBuf<uint32_t> d_dsk, d_uk;   // their residues and key-switch sums in the 31-bit basis
    // views of the active basis' tables (use_ks32_basis): kn / kz own them
    Prime32* d_p32 = nullptr;
    uint2* d_tw32 = nullptr;
    Ks32Tables* d_kst = nullptr;
    DevBuf<uint32_t> d_rs;       // key in the auxiliary basis [keys][2L][S][n], NTT domain mod p_s
    bool rs_valid = false;
    bool rlk_loaded = false;
    // workspace (per chunk) of lane 0
    size_t chunk = 512;  // products per pipeline pass; throughput plateaus from ~512 (r1 sweep)
    Workspace ws;
    bool digit16 = true;   // EXACTO_DIGIT16=0: u64 digits per limb instead of Workspace::D16
    // further pipeline lanes: chunk i runs on lane i % lanes, each lane a stream with its own
    // workspace, so the kernels of consecutive chunks overlap (EXACTO_DUAL_STREAM=0: one lane;
    // EXACTO_LANES: lane count, 2 by default)
    bool dual = true;
    int lanes = 2;
    hipEvent_t ev_fork = nullptr;
    // dBFV chains of two or more items run as two halves on two streams (exacto_dbfv_mul_chain_dev):
    // the second half on a twin context (same parameters, its own stream and workspaces, a copy of
    // the relinearisation key), so each half's whole chain overlaps the other's
    static constexpr int MAX_TWINS = 3;
    exacto_ctx* twin[MAX_TWINS] = {};
    bool batch_split = true;         // EXACTO_CHAIN_SPLIT=0: one stream for the whole batch
    unsigned rlk_version = 0, twin_rlk_version[MAX_TWINS] = {~0u, ~0u, ~0u};
    hipEvent_t ev_twin_in = nullptr, ev_twin_out[MAX_TWINS] = {};
    LaneSet xl[EXACTO_MAX_LANES - 1];   // lanes 1 .. lanes-1
    // dBFV: per-ciphertext extensions shared by the products that use the ciphertext
    // (EXACTO_SHARE_EXT=0 recomputes them per product)
    bool share_ext = true;
    // keygen / encryption
    DevBuf<double> d_cdt;
    double cdt_sigma = 0.0;
    DevBuf<u64> d_gpow;
    DevBuf<u64> d_delta;
    bool delta_ok = false;
    DevBuf<u64> enc_buf;
    DevBuf<u64> d_lin;  // terms of the last dBFV linear map, LinTerm [E][L]
    std::vector<u64> lin_host;  // what d_lin holds
    DevBuf<u64> d_dp;   // fold digits or pair list of the last dBFV plaintext product (dbfv_plain_tables)
    std::vector<u64> dp_host;   // what d_dp holds
    size_t plain_terms = 64;    // dBFV plaintext products: terms lifted into pl_buf at a time
    DevBuf<u64> gk_s;  // Shoup companions of the Galois key of the last automorphism call
    DevBuf<uint32_t> d_gk_rs;  // ks32: Galois key of the last automorphism call in the 31-bit basis
    DevBuf<u64> pl_buf;  // lifted plaintexts / monomial scratch
    DevBuf<u64> ext_a, ext_b;
    DevBuf<u64> chain_buf;  // dBFV chain ping-pong buffers
    // dBFV chain, psum path: each step's relinearised limbs also in the coefficient domain (they are
    // there before the final forward NTT), so the next step's extension lifts them directly instead
    // of inverse-transforming its NTT-domain input (dbfv_mul_group, exacto_dbfv_mul_chain_dev)
    DevBuf<u64> chain_coef;
    // (coef_out and coef_in are views into chain_coef halves, not owned)
    u64* coef_out = nullptr;        // where this step's coefficient form went (psum steps of a chain)
    int coef_slot = -1;             // set by the chain: chain_coef half for this step's coefficient form
    size_t coef_slot_words = 0;     // ... and the size of one half
    const u64* coef_in = nullptr;   // set by the chain: the coefficient form of this step's `a`
    bool coef_written = false;      // reported back: coef_out holds this step's results
    DevBuf<u64> dec_buf;    // decryption phase [B][L][n]
    DevBuf<u64> dig_buf;    // dBFV decrypted digits [B][d][n]
    // staging for host-pointer API and dBFV products
    DevBuf<u64> io;
    DevBuf<u64> prod;
    // product-sum plan cache (dbfv_mul's index rule, or bfv_mul_sum's term lists: cached_kind)
    DevBuf<u64> d_off;
    int cached_kind = -1;            // 0: dbfv_plan, 1: mul_sum_plan, 2: dbfv_plan's symmetric form; -1: none
    std::vector<uint32_t> cached_ms; // mul_sum_plan: ia, ib, slot lists, then na, nb, nslots, group limit
    int cached_ngroups = 0;          // mul_sum_plan: groups of the cached plan (its "output limbs")
    DevBuf<int> d_slot_start;        // ... and, when a slot has several, slot s = groups [start[s], start[s+1])
    DevBuf<u64> gsum_buf;            // bfv_mul_sum: the groups' coefficient-domain results [B][groups][2][L][n]
    // modulus switch: q_j^-1 mod q_i (j > i) at [j * L + i] with their Shoup companions, built on first use;
    // the intermediate levels of a call that drops several primes (two halves, one chunk each)
    std::vector<u64> msw_w, msw_ws;
    DevBuf<u64> msw_buf;
    // SIMD batching (batch.hip): validated and built at the context's first batching call (batch_ready)
    int batch_state = 0;             // 0: not tried, 1: tables resident, -1: this context cannot batch
    int batch_code = 0;              // ... and why
    std::string batch_msg;
    u64 batch_root = 0;              // zeta = find_psi(n, t)
    int batch_form = 0;              // the transforms' arithmetic (F32_LAZY / F32_WIDE / BF_STRICT)
    BatchTab batch_tab{};
    DevBuf<uint2> d_btw;             // [2][n] forward, inverse twiddles mod t
    DevBuf<uint32_t> d_bperm;        // [n] slot -> storage position
    DevBuf<u64> batch_buf;           // the compositions' plaintexts, one chunk
    size_t cached_B = 0, cached_d = 0;
    u64 cached_base = 0, cached_p = 0;
    int cached_npairs = 0;
    std::vector<int> cached_limbs;   // output limbs of the cached plan (all d, or a subset: exacto_dbfv_mul_limbs)
    int cached_sum_m = 0;        // max products per dBFV output limb when all combine terms are sums, else -1
    DevBuf<int> d_term_start;
    DevBuf<CombineTerm> d_terms;
    // per-call scratch: the context's own stream-ordered pool (Scratch)
    hipMemPool_t pool = nullptr;
    // the bootstrap's intermediates (coefficients, flags, the c0'/c1' rows, phase, slots): a persistent
    // buffer of the boot context, grown like the workspaces, never from the stream-ordered pool
    DevBuf<u64> boot_buf;
    DevBuf<u64> boot_slots;      // ... and the slots of the ring path, grown when an item takes it
    bool debug_scratch = false;
    size_t dbfv_group_bytes = (size_t)16384 << 20;  // dbfv_mul item groups (EXACTO_DBFV_GROUP_MB)
    // profiling
    bool prof = false;
    std::vector<ProfRec> recs;
    std::map<int, std::map<const void*, std::pair<u64, double>>> prof_kern;   // kind -> kernel -> (launches, ms)
};

namespace exacto {

// Kernel families timed by exacto_prof_enable (HIP events around each launch on the launching
// stream; the bench's roofline takes the family with the largest share of a profiled step).
// Bytes are ALGORITHMIC: each operand read once and each result written once.
enum ProfKind : int {
    PK_FWD = 0, PK_INV = 1, PK_TENSOR = 2, PK_POLYMUL = 3, PK_LIFT = 4, PK_SCALE = 5, PK_KS_DIGITS = 6,
    PK_KS_MAC = 7, PK_KS_CRT = 8, PK_PAIRSUM = 9, PK_PSUM_SCALE = 10, PK_TENSOR_C2 = 11, PK_DIGIT_SUM = 12,
    PK_COMBINE = 13, PK_HPS_EXT = 14, PK_RELIN_MAC = 15, PK_HPS_SCALE = 16, PK_GROUP_SUM = 17, PK_MODSWITCH = 18,
    PK_COUNT = 19
};

struct ProfScope {
    exacto_ctx* c;
    ProfRec rec{};
    bool on;
    ProfScope(exacto_ctx* c_, int kind, u64 units, double bytes) : c(c_), on(c_->prof) {
        if (!on) return;
        rec.kind = kind; rec.polys = units; rec.bytes = bytes;
        g_last_kernel = nullptr;
        if (hipEventCreate(&rec.a) != hipSuccess || hipEventCreate(&rec.b) != hipSuccess ||
            hipEventRecord(rec.a, c->stream) != hipSuccess)
            on = false;
    }
    ~ProfScope() {
        if (!on) return;
        rec.kern = g_last_kernel;
        if (hipEventRecord(rec.b, c->stream) == hipSuccess) c->recs.push_back(rec);
    }
};

// ============================================================== shared helpers, by the file that defines them

// context.hip
u64 invmod_h(u64 a, u64 m);
u64 shoup_h(u64 w, u64 q);
size_t poly_bytes(const exacto_ctx* c);
int run_ntt(exacto_ctx* c, const NttBatch& nb, long count, bool inverse);
NttBatch contiguous(u64* data, long count_items, long poly_per_item, int prime_base, int period,
                    int n);
int check_ctx(exacto_ctx* c);
int host_call(exacto_ctx* c, const std::vector<std::pair<const void*, size_t>>& ins, size_t out_bytes,
              void* host_out, const std::function<int(std::vector<u64*>&, u64*)>& fn);
int dbfv_params_check(size_t d, uint64_t base, uint64_t plain);
int delta_residues(exacto_ctx* c);

// api_decrypt.hip
int decrypt_batch(exacto_ctx* c, const u64* ct, size_t polys, long ct_stride, const u64* sk, u64* out,
                  size_t B);

}  // namespace exacto
