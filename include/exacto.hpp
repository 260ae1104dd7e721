// exacto.hpp — C++ host API mirroring the reference's Rust API on the multiplication path,
// layered on the C ABI (exacto_hip.h).  Same names and argument meaning as
//   exacto::params::{BfvParams, BfvParamsBuilder, DbfvParams}   (src/params/mod.rs:12-193)
//   exacto::bfv::{BfvCiphertext, RelinKey}                       (src/bfv/mod.rs:19-24, keygen.rs:39-45)
//   exacto::bfv::eval::{bfv_mul_and_relin, bfv_mul_no_relin, bfv_add, bfv_sub, bfv_neg}
//   exacto::bfv::keyswitch::relinearize
//   exacto::dbfv::{DbfvCiphertext, eval::dbfv_mul}
//   exacto::bfv::keygen / encrypt (device samplers), eval::{bfv_plain_mul, bfv_plain_add,
//     bfv_inner_product, bfv_monomial_mul, bfv_trace, bfv_apply_automorphism}
//   exacto::bootstrap::{coeffs_to_slots, digit_extract, bfv_host}  (src/bootstrap/*.rs)
// Errors: Rust's Result<T, ExactoError> becomes a thrown exacto::ExactoError carrying the
// variant (src/error.rs:4-31) and the reference's Display text.
// Ciphertexts are host-resident here (one H2D/D2H per call); the batched overloads amortise it.
#pragma once

#include <algorithm>
#include <cstdint>
#include <map>
#include <memory>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "exacto_hip.h"

namespace exacto {

class ExactoError : public std::runtime_error {
  public:
    ExactoError(int code, const std::string& msg) : std::runtime_error(msg), code_(code) {}
    int code() const { return code_; }
    const char* variant() const {
        static const char* names[] = {"InvalidParam", "DimensionMismatch", "ModulusMismatch",
                                      "InvalidRingDegree", "DecryptionError", "DecompositionError",
                                      "LatticeError", "MissingKey", "NotImplemented"};
        return (code_ >= 1 && code_ <= 9) ? names[code_ - 1] : "HipError";
    }

  private:
    int code_;
};

namespace detail {
inline void check(int rc) {
    if (rc == 0) return;
    char buf[1024];
    exacto_last_error(buf, sizeof buf);
    throw ExactoError(rc, buf);
}
}  // namespace detail

// RnsPoly (src/ring/rns.rs:14-17): L limbs of n NTT-domain evaluations, stored [L][n].
struct RnsPoly {
    size_t ring_degree = 0;
    size_t num_limbs = 0;
    std::vector<uint64_t> data;  // [limb][n]
    uint64_t* limb(size_t i) { return data.data() + i * ring_degree; }
    const uint64_t* limb(size_t i) const { return data.data() + i * ring_degree; }
};

class BfvParams {
  public:
    size_t ring_degree;
    uint64_t plain_modulus;
    std::vector<uint64_t> ct_moduli, aux_moduli;
    double sigma;
    uint64_t gadget_base;
    size_t gadget_digits;
    ~BfvParams() { exacto_ctx_destroy(ctx_); }
    exacto_ctx* ctx() const { return ctx_; }
    size_t num_limbs() const { return ct_moduli.size(); }
    // the key last uploaded to the context (identity, not contents)
    mutable const void* loaded_key = nullptr;

  private:
    friend class BfvParamsBuilder;
    exacto_ctx* ctx_ = nullptr;
};
using BfvParamsPtr = std::shared_ptr<const BfvParams>;

// BfvParamsBuilder (src/params/mod.rs:30-124); build() also creates the device context.
class BfvParamsBuilder {
  public:
    BfvParamsBuilder& ring_degree(size_t n) { n_ = n; return *this; }
    BfvParamsBuilder& plain_modulus(uint64_t p) { p_ = p; return *this; }
    BfvParamsBuilder& ct_moduli(std::vector<uint64_t> m) { ct_ = std::move(m); return *this; }
    BfvParamsBuilder& aux_moduli(std::vector<uint64_t> m) { aux_ = std::move(m); return *this; }
    BfvParamsBuilder& sigma(double s) { sigma_ = s; return *this; }
    BfvParamsBuilder& gadget_base(uint64_t b) { base_ = b; return *this; }
    BfvParamsBuilder& device(int d) { device_ = d; return *this; }
    BfvParamsPtr build() const {
        auto p = std::shared_ptr<BfvParams>(new BfvParams());
        detail::check(exacto_ctx_create(&p->ctx_, n_, ct_.data(), ct_.size(),
                                        aux_.empty() ? nullptr : aux_.data(), aux_.size(), p_, base_,
                                        device_));
        exacto_ctx_info info{};
        detail::check(exacto_ctx_get_info(p->ctx_, &info));
        // NTT-domain data (keys, ciphertexts) is laid out in the library's storage order: refuse a
        // library whose order differs from the one this header was written for
        if (info.ntt_order != EXACTO_NTT_ORDER)
            throw ExactoError(EXACTO_ERR_INVALID_PARAM, "libexacto_hip NTT-domain order differs from exacto.hpp's");
        p->ring_degree = n_;
        p->plain_modulus = p_;
        p->ct_moduli = ct_;
        p->aux_moduli = aux_;
        p->sigma = sigma_;
        p->gadget_base = info.gadget_base;
        p->gadget_digits = info.gadget_digits;
        return p;
    }

  private:
    size_t n_ = 4096;        // params/mod.rs:42
    uint64_t p_ = 65537;     // params/mod.rs:43
    std::vector<uint64_t> ct_, aux_;
    double sigma_ = 3.2;
    uint64_t base_ = 0;      // auto: 2^16 (params/mod.rs:102-108)
    int device_ = 0;
};

struct BfvCiphertext {
    std::vector<RnsPoly> c;
    BfvParamsPtr params;
    size_t degree() const { return c.size() - 1; }
};

struct RelinKey {
    std::vector<std::pair<RnsPoly, RnsPoly>> keys;
    BfvParamsPtr params;
};

// SecretKey (src/bfv/keygen.rs): the secret polynomial s in the NTT domain, [L][n].
struct SecretKey {
    RnsPoly poly;
    BfvParamsPtr params;
};

// CoeffPoly (src/ring/poly.rs:6-9): plaintext coefficients mod `modulus`.
struct CoeffPoly {
    std::vector<uint64_t> coeffs;
    uint64_t modulus = 0;
};

namespace detail {
inline std::vector<uint64_t> flatten(const std::vector<BfvCiphertext>& cts, size_t polys) {
    std::vector<uint64_t> out;
    for (auto& ct : cts) {
        if (ct.c.size() != polys) throw ExactoError(1, "invalid parameter: mixed ciphertext degrees in a batch");
        for (auto& p : ct.c) out.insert(out.end(), p.data.begin(), p.data.end());
    }
    return out;
}
inline std::vector<BfvCiphertext> unflatten(const std::vector<uint64_t>& flat, size_t batch, size_t polys,
                                            const BfvParamsPtr& prm) {
    const size_t L = prm->num_limbs(), n = prm->ring_degree;
    std::vector<BfvCiphertext> out(batch);
    for (size_t b = 0; b < batch; ++b) {
        out[b].params = prm;
        out[b].c.resize(polys);
        for (size_t k = 0; k < polys; ++k) {
            RnsPoly& p = out[b].c[k];
            p.ring_degree = n;
            p.num_limbs = L;
            auto it = flat.begin() + (long)((b * polys + k) * L * n);
            p.data.assign(it, it + (long)(L * n));
        }
    }
    return out;
}
inline void load_key(const RelinKey& rlk) {
    const BfvParams& prm = *rlk.params;
    if (prm.loaded_key == &rlk) return;
    std::vector<uint64_t> flat;
    for (auto& kp : rlk.keys) {
        flat.insert(flat.end(), kp.first.data.begin(), kp.first.data.end());
        flat.insert(flat.end(), kp.second.data.begin(), kp.second.data.end());
    }
    check(exacto_ctx_load_relin_key(prm.ctx(), flat.empty() ? nullptr : flat.data(), rlk.keys.size()));
    prm.loaded_key = &rlk;
}
}  // namespace detail

// ---- exacto::bfv::eval (batched forms; the single-ciphertext forms below wrap them)
inline std::vector<BfvCiphertext> bfv_mul_no_relin(const std::vector<BfvCiphertext>& a,
                                                   const std::vector<BfvCiphertext>& b) {
    if (a.empty()) return {};
    const BfvParamsPtr& prm = a[0].params;
    const size_t p1 = a[0].c.size(), p2 = b[0].c.size();
    auto fa = detail::flatten(a, p1), fb = detail::flatten(b, p2);
    std::vector<uint64_t> out(a.size() * 3 * prm->num_limbs() * prm->ring_degree);
    detail::check(exacto_bfv_mul_no_relin(prm->ctx(), fa.data(), p1, fb.data(), p2, out.data(), a.size()));
    return detail::unflatten(out, a.size(), 3, prm);
}

inline std::vector<BfvCiphertext> relinearize(const std::vector<BfvCiphertext>& cts, const RelinKey& rlk) {
    if (cts.empty()) return {};
    const BfvParamsPtr& prm = cts[0].params;
    const size_t polys = cts[0].c.size();
    detail::load_key(rlk);
    auto f = detail::flatten(cts, polys);
    const size_t outp = polys < 3 ? polys : 2;
    std::vector<uint64_t> out(cts.size() * outp * prm->num_limbs() * prm->ring_degree);
    detail::check(exacto_relinearize(prm->ctx(), f.data(), polys, out.data(), cts.size()));
    return detail::unflatten(out, cts.size(), outp, prm);
}

inline std::vector<BfvCiphertext> bfv_mul_and_relin(const std::vector<BfvCiphertext>& a,
                                                    const std::vector<BfvCiphertext>& b, const RelinKey& rlk) {
    if (a.empty()) return {};
    const BfvParamsPtr& prm = a[0].params;
    if (a[0].c.size() != 2 || b[0].c.size() != 2)
        throw ExactoError(1, "invalid parameter: multiplication requires degree-1 ciphertexts");
    detail::load_key(rlk);
    auto fa = detail::flatten(a, 2), fb = detail::flatten(b, 2);
    std::vector<uint64_t> out(fa.size());
    detail::check(exacto_bfv_mul_and_relin(prm->ctx(), fa.data(), fb.data(), out.data(), a.size()));
    return detail::unflatten(out, a.size(), 2, prm);
}

// Squares (exacto_bfv_square_*): bit for bit bfv_mul_no_relin(a, a) / bfv_mul_and_relin(a, a, rlk), the
// operand's input work done once.
inline std::vector<BfvCiphertext> bfv_square_no_relin(const std::vector<BfvCiphertext>& a) {
    if (a.empty()) return {};
    const BfvParamsPtr& prm = a[0].params;
    const size_t p1 = a[0].c.size();
    auto fa = detail::flatten(a, p1);
    std::vector<uint64_t> out(a.size() * 3 * prm->num_limbs() * prm->ring_degree);
    detail::check(exacto_bfv_square_no_relin(prm->ctx(), fa.data(), p1, out.data(), a.size()));
    return detail::unflatten(out, a.size(), 3, prm);
}

inline std::vector<BfvCiphertext> bfv_square_and_relin(const std::vector<BfvCiphertext>& a, const RelinKey& rlk) {
    if (a.empty()) return {};
    const BfvParamsPtr& prm = a[0].params;
    if (a[0].c.size() != 2) throw ExactoError(1, "invalid parameter: multiplication requires degree-1 ciphertexts");
    detail::load_key(rlk);
    auto fa = detail::flatten(a, 2);
    std::vector<uint64_t> out(fa.size());
    detail::check(exacto_bfv_square_and_relin(prm->ctx(), fa.data(), out.data(), a.size()));
    return detail::unflatten(out, a.size(), 2, prm);
}

inline BfvCiphertext bfv_square_no_relin(const BfvCiphertext& a) {
    return bfv_square_no_relin(std::vector<BfvCiphertext>{a})[0];
}
inline BfvCiphertext bfv_square_and_relin(const BfvCiphertext& a, const RelinKey& rlk) {
    return bfv_square_and_relin(std::vector<BfvCiphertext>{a}, rlk)[0];
}

inline BfvCiphertext bfv_mul_no_relin(const BfvCiphertext& a, const BfvCiphertext& b) {
    return bfv_mul_no_relin(std::vector<BfvCiphertext>{a}, std::vector<BfvCiphertext>{b})[0];
}
inline BfvCiphertext relinearize(const BfvCiphertext& ct, const RelinKey& rlk) {
    return relinearize(std::vector<BfvCiphertext>{ct}, rlk)[0];
}
inline BfvCiphertext bfv_mul_and_relin(const BfvCiphertext& a, const BfvCiphertext& b, const RelinKey& rlk) {
    return bfv_mul_and_relin(std::vector<BfvCiphertext>{a}, std::vector<BfvCiphertext>{b}, rlk)[0];
}

// Sums of ciphertext products with one key switch per sum (exacto_bfv_mul_sum; the ciphertext x
// ciphertext counterpart of bfv_inner_product): out[s] = sum over the terms {ia, ib, s} of
// bfv_mul_and_relin(a[ia], b[ib], rlk), bit for bit the composition with bfv_add.  One item; a and b
// may be the same vector, a pair listed twice counts twice.
struct MulSumTerm {
    uint32_t ia, ib, slot;
};
inline std::vector<BfvCiphertext> bfv_mul_sum(const std::vector<BfvCiphertext>& a, const std::vector<BfvCiphertext>& b,
                                              const std::vector<MulSumTerm>& terms, size_t nslots,
                                              const RelinKey& rlk) {
    if (a.empty() || b.empty()) throw ExactoError(1, "invalid parameter: bfv_mul_sum needs ciphertexts on both sides");
    const BfvParamsPtr& prm = a[0].params;
    if (a[0].c.size() != 2 || b[0].c.size() != 2)
        throw ExactoError(1, "invalid parameter: multiplication requires degree-1 ciphertexts");
    detail::load_key(rlk);
    auto fa = detail::flatten(a, 2), fb = detail::flatten(b, 2);
    std::vector<uint32_t> ia, ib, sl;
    for (auto& t : terms) { ia.push_back(t.ia); ib.push_back(t.ib); sl.push_back(t.slot); }
    std::vector<uint64_t> out(nslots * 2 * prm->num_limbs() * prm->ring_degree);
    detail::check(exacto_bfv_mul_sum(prm->ctx(), fa.data(), a.size(), fb.data(), b.size(), ia.data(), ib.data(),
                                     sl.data(), terms.size(), nslots, out.data(), 1));
    return detail::unflatten(out, nslots, 2, prm);
}

// bfv_add / bfv_sub (eval.rs:14-51): each batch has one component count; the two counts may differ
// (the longer operand's extra components pass through, ct2's negated under subtraction)
namespace detail {
inline std::vector<BfvCiphertext> addsub(bool sub, const std::vector<BfvCiphertext>& a,
                                         const std::vector<BfvCiphertext>& b) {
    if (a.empty()) return {};
    if (a.size() != b.size()) throw ExactoError(1, "invalid parameter: batch sizes differ");
    const BfvParamsPtr& prm = a[0].params;
    const size_t p1 = a[0].c.size(), p2 = b[0].c.size(), pm = p1 > p2 ? p1 : p2;
    auto fa = flatten(a, p1), fb = flatten(b, p2);
    std::vector<uint64_t> out(a.size() * pm * prm->num_limbs() * prm->ring_degree);
    check((sub ? exacto_bfv_sub : exacto_bfv_add)(prm->ctx(), fa.data(), p1, fb.data(), p2, out.data(), a.size()));
    return unflatten(out, a.size(), pm, prm);
}
}  // namespace detail
inline std::vector<BfvCiphertext> bfv_add(const std::vector<BfvCiphertext>& a, const std::vector<BfvCiphertext>& b) {
    return detail::addsub(false, a, b);
}
inline std::vector<BfvCiphertext> bfv_sub(const std::vector<BfvCiphertext>& a, const std::vector<BfvCiphertext>& b) {
    return detail::addsub(true, a, b);
}
inline std::vector<BfvCiphertext> bfv_neg(const std::vector<BfvCiphertext>& cts) {
    if (cts.empty()) return {};
    const BfvParamsPtr& prm = cts[0].params;
    const size_t polys = cts[0].c.size();
    auto f = detail::flatten(cts, polys);
    std::vector<uint64_t> out(f.size());
    detail::check(exacto_bfv_neg(prm->ctx(), f.data(), polys, out.data(), cts.size()));
    return detail::unflatten(out, cts.size(), polys, prm);
}
inline BfvCiphertext bfv_add(const BfvCiphertext& a, const BfvCiphertext& b) {
    return bfv_add(std::vector<BfvCiphertext>{a}, std::vector<BfvCiphertext>{b})[0];
}
inline BfvCiphertext bfv_sub(const BfvCiphertext& a, const BfvCiphertext& b) {
    return bfv_sub(std::vector<BfvCiphertext>{a}, std::vector<BfvCiphertext>{b})[0];
}
inline BfvCiphertext bfv_neg(const BfvCiphertext& ct) { return bfv_neg(std::vector<BfvCiphertext>{ct})[0]; }

// decrypt (src/bfv/encrypt.rs:111-178), batched over ciphertexts of one degree.
inline std::vector<CoeffPoly> decrypt(const std::vector<BfvCiphertext>& cts, const SecretKey& sk) {
    if (cts.empty()) return {};
    const BfvParams& prm = *cts[0].params;
    const size_t polys = cts[0].c.size(), n = prm.ring_degree;
    auto flat = detail::flatten(cts, polys);
    std::vector<uint64_t> out(cts.size() * n);
    detail::check(exacto_bfv_decrypt(prm.ctx(), flat.data(), polys, sk.poly.data.data(), out.data(), cts.size()));
    std::vector<CoeffPoly> res(cts.size());
    for (size_t b = 0; b < cts.size(); ++b) {
        res[b].coeffs.assign(out.begin() + (long)(b * n), out.begin() + (long)((b + 1) * n));
        res[b].modulus = prm.plain_modulus;
    }
    return res;
}
inline CoeffPoly decrypt(const BfvCiphertext& ct, const SecretKey& sk) {
    return decrypt(std::vector<BfvCiphertext>{ct}, sk)[0];
}

// ---- key generation / encryption on the device (src/bfv/keygen.rs, src/bfv/encrypt.rs:29-106)
// ChaChaRng stands in for the reference's `R: Rng` argument (ChaCha20Rng): a 256-bit key and a
// stream counter; every call consumes one stream id, as a call consumes words of the reference's
// RNG.  The word stream is this library's own (see include/exacto_hip.h).
struct ChaChaRng {
    uint64_t key[4];
    uint64_t stream = 0;
    explicit ChaChaRng(uint64_t seed) {  // SplitMix64 expansion of a 64-bit seed
        uint64_t z = seed;
        for (auto& k : key) {
            z += 0x9E3779B97F4A7C15ull;
            uint64_t x = z;
            x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
            x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
            k = x ^ (x >> 31);
        }
    }
    uint64_t next() { return stream++; }
};

// PublicKey (keygen.rs:28-34): pk0 = -(a s + e), pk1 = a.
struct PublicKey {
    RnsPoly pk0, pk1;
    BfvParamsPtr params;
};

namespace detail {
inline RnsPoly make_poly(const BfvParams& prm, const uint64_t* src) {
    RnsPoly p;
    p.ring_degree = prm.ring_degree;
    p.num_limbs = prm.num_limbs();
    p.data.assign(src, src + p.ring_degree * p.num_limbs);
    return p;
}
}  // namespace detail

// gen_secret_key_with_rng (keygen.rs:64-79)
inline SecretKey gen_secret_key_with_rng(const BfvParamsPtr& prm, ChaChaRng& rng) {
    std::vector<uint64_t> sk(prm->num_limbs() * prm->ring_degree);
    detail::check(exacto_gen_secret_key(prm->ctx(), rng.key, rng.next(), sk.data()));
    return SecretKey{detail::make_poly(*prm, sk.data()), prm};
}

// gen_public_key_with_rng (keygen.rs:87-110)
inline PublicKey gen_public_key_with_rng(const SecretKey& sk, ChaChaRng& rng) {
    const BfvParams& prm = *sk.params;
    const size_t Ln = prm.num_limbs() * prm.ring_degree;
    std::vector<uint64_t> pk(2 * Ln);
    detail::check(exacto_gen_public_key(prm.ctx(), sk.poly.data.data(), prm.sigma, rng.key, rng.next(), pk.data()));
    return PublicKey{detail::make_poly(prm, pk.data()), detail::make_poly(prm, pk.data() + Ln), sk.params};
}

// gen_relin_key_with_rng (keygen.rs:123-162): gadget_digits keys
inline RelinKey gen_relin_key_with_rng(const SecretKey& sk, ChaChaRng& rng) {
    const BfvParams& prm = *sk.params;
    const size_t Ln = prm.num_limbs() * prm.ring_degree, G = prm.gadget_digits;
    std::vector<uint64_t> flat(G * 2 * Ln);
    detail::check(exacto_gen_relin_key(prm.ctx(), sk.poly.data.data(), prm.sigma, rng.key, rng.next(), G,
                                       flat.data()));
    RelinKey rlk;
    rlk.params = sk.params;
    for (size_t g = 0; g < G; ++g)
        rlk.keys.emplace_back(detail::make_poly(prm, flat.data() + 2 * g * Ln),
                              detail::make_poly(prm, flat.data() + (2 * g + 1) * Ln));
    return rlk;
}

// encrypt_sk_with_rng / encrypt_pk_with_rng (encrypt.rs:29-106), batched over plaintexts
inline std::vector<BfvCiphertext> encrypt_batch(const std::vector<CoeffPoly>& pts, const SecretKey* sk,
                                                const PublicKey* pk, const BfvParamsPtr& prm, ChaChaRng& rng) {
    const size_t n = prm->ring_degree, Ln = prm->num_limbs() * n;
    std::vector<uint64_t> pt;
    for (auto& p : pts) {
        if (p.coeffs.size() != n) throw ExactoError(2, "dimension mismatch: expected " + std::to_string(n) +
                                                           ", got " + std::to_string(p.coeffs.size()));
        pt.insert(pt.end(), p.coeffs.begin(), p.coeffs.end());
    }
    std::vector<uint64_t> ct(pts.size() * 2 * Ln);
    if (sk) {
        detail::check(exacto_encrypt_sk(prm->ctx(), pt.data(), sk->poly.data.data(), prm->sigma, rng.key,
                                        rng.next(), ct.data(), pts.size()));
    } else {
        std::vector<uint64_t> pkf(pk->pk0.data);
        pkf.insert(pkf.end(), pk->pk1.data.begin(), pk->pk1.data.end());
        detail::check(exacto_encrypt_pk(prm->ctx(), pt.data(), pkf.data(), prm->sigma, rng.key, rng.next(),
                                        ct.data(), pts.size()));
    }
    return detail::unflatten(ct, pts.size(), 2, prm);
}
inline BfvCiphertext encrypt_sk_with_rng(const CoeffPoly& pt, const SecretKey& sk, const BfvParamsPtr& prm,
                                         ChaChaRng& rng) {
    return encrypt_batch({pt}, &sk, nullptr, prm, rng)[0];
}
inline BfvCiphertext encrypt_pk_with_rng(const CoeffPoly& pt, const PublicKey& pk, const BfvParamsPtr& prm,
                                         ChaChaRng& rng) {
    return encrypt_batch({pt}, nullptr, &pk, prm, rng)[0];
}

// GaloisKey (keygen.rs:49-56) and bfv_apply_automorphism (eval.rs:512-561)
struct GaloisKey {
    std::vector<std::pair<RnsPoly, RnsPoly>> keys;
    size_t element = 0;
    BfvParamsPtr params;
};

inline GaloisKey gen_galois_key_with_rng(const SecretKey& sk, size_t element, ChaChaRng& rng) {
    const BfvParams& prm = *sk.params;
    const size_t Ln = prm.num_limbs() * prm.ring_degree, G = prm.gadget_digits;
    std::vector<uint64_t> flat(G * 2 * Ln);
    detail::check(exacto_gen_galois_key(prm.ctx(), sk.poly.data.data(), element, prm.sigma, rng.key, rng.next(), G,
                                        flat.data()));
    GaloisKey gk;
    gk.element = element;
    gk.params = sk.params;
    for (size_t g = 0; g < G; ++g)
        gk.keys.emplace_back(detail::make_poly(prm, flat.data() + 2 * g * Ln),
                             detail::make_poly(prm, flat.data() + (2 * g + 1) * Ln));
    return gk;
}

inline std::vector<BfvCiphertext> bfv_apply_automorphism(const std::vector<BfvCiphertext>& cts, const GaloisKey& gk) {
    if (cts.empty()) return {};
    const BfvParams& prm = *cts[0].params;
    const size_t polys = cts[0].c.size();
    if (polys != 2) throw ExactoError(1, "invalid parameter: automorphism requires degree-1 ciphertext");
    auto flat = detail::flatten(cts, polys);
    std::vector<uint64_t> key;
    for (auto& k : gk.keys) {
        key.insert(key.end(), k.first.data.begin(), k.first.data.end());
        key.insert(key.end(), k.second.data.begin(), k.second.data.end());
    }
    std::vector<uint64_t> out(flat.size());
    detail::check(exacto_bfv_apply_automorphism(prm.ctx(), flat.data(), polys, gk.element, key.data(),
                                                gk.keys.size(), out.data(), cts.size()));
    return detail::unflatten(out, cts.size(), 2, cts[0].params);
}
inline BfvCiphertext bfv_apply_automorphism(const BfvCiphertext& ct, const GaloisKey& gk) {
    return bfv_apply_automorphism(std::vector<BfvCiphertext>{ct}, gk)[0];
}

// encode_scalar / decode_scalar (src/bfv/encoding.rs:7-20)
inline CoeffPoly encode_scalar(uint64_t m, const BfvParamsPtr& prm) {
    if (m >= prm->plain_modulus)
        throw ExactoError(1, "invalid parameter: plaintext " + std::to_string(m) + " >= plain_modulus " +
                                 std::to_string(prm->plain_modulus));
    CoeffPoly p;
    p.coeffs.assign(prm->ring_degree, 0);
    p.coeffs[0] = m;
    p.modulus = prm->plain_modulus;
    return p;
}
inline uint64_t decode_scalar(const CoeffPoly& p) { return p.coeffs.empty() ? 0 : p.coeffs[0]; }

// ---- SIMD batching (replaces src/bfv/encoding.rs encode_simd / decode_simd, which pack coefficients):
// slot vectors of n values as 2 x n/2 matrices, the convention of include/exacto_hip.h.  Needs a prime
// plain_modulus == 1 (mod 2n) below 2^32; a context that cannot batch throws at its first batching call.
using SlotVector = std::vector<uint64_t>;

// zeta of the slot encoding (exacto_batch_info)
inline uint64_t batch_root(const BfvParamsPtr& prm) {
    uint64_t root = 0;
    detail::check(exacto_batch_info(prm->ctx(), &root));
    return root;
}
namespace detail {
inline std::vector<uint64_t> flatten_slots(const std::vector<SlotVector>& values, size_t n) {
    std::vector<uint64_t> out;
    for (auto& v : values) {
        if (v.size() != n) throw ExactoError(2, "dimension mismatch: expected " + std::to_string(n) + ", got " +
                                                    std::to_string(v.size()));
        out.insert(out.end(), v.begin(), v.end());
    }
    return out;
}
inline std::vector<SlotVector> split_slots(const std::vector<uint64_t>& flat, size_t batch, size_t n) {
    std::vector<SlotVector> out(batch);
    for (size_t b = 0; b < batch; ++b) out[b].assign(flat.begin() + (long)(b * n), flat.begin() + (long)((b + 1) * n));
    return out;
}
inline std::vector<uint64_t> flatten_key(const std::vector<std::pair<RnsPoly, RnsPoly>>& keys) {
    std::vector<uint64_t> key;
    for (auto& k : keys) {
        key.insert(key.end(), k.first.data.begin(), k.first.data.end());
        key.insert(key.end(), k.second.data.begin(), k.second.data.end());
    }
    return key;
}
}  // namespace detail

// values (each below t: InvalidParam "plaintext {v} >= plain_modulus {t}" otherwise) -> plaintexts
inline std::vector<CoeffPoly> batch_encode(const std::vector<SlotVector>& values, const BfvParamsPtr& prm) {
    const size_t n = prm->ring_degree;
    auto flat = detail::flatten_slots(values, n);
    std::vector<uint64_t> out(flat.size());
    detail::check(exacto_batch_encode(prm->ctx(), flat.data(), out.data(), values.size()));
    std::vector<CoeffPoly> res(values.size());
    for (size_t b = 0; b < values.size(); ++b) {
        res[b].coeffs.assign(out.begin() + (long)(b * n), out.begin() + (long)((b + 1) * n));
        res[b].modulus = prm->plain_modulus;
    }
    return res;
}
inline CoeffPoly batch_encode(const SlotVector& values, const BfvParamsPtr& prm) {
    return batch_encode(std::vector<SlotVector>{values}, prm)[0];
}
inline std::vector<SlotVector> batch_decode(const std::vector<CoeffPoly>& pts, const BfvParamsPtr& prm) {
    const size_t n = prm->ring_degree;
    std::vector<uint64_t> flat;
    for (auto& p : pts) {
        if (p.coeffs.size() != n) throw ExactoError(2, "dimension mismatch: expected " + std::to_string(n) +
                                                           ", got " + std::to_string(p.coeffs.size()));
        flat.insert(flat.end(), p.coeffs.begin(), p.coeffs.end());
    }
    std::vector<uint64_t> out(flat.size());
    detail::check(exacto_batch_decode(prm->ctx(), flat.data(), out.data(), pts.size()));
    return detail::split_slots(out, pts.size(), n);
}
inline SlotVector batch_decode(const CoeffPoly& pt, const BfvParamsPtr& prm) {
    return batch_decode(std::vector<CoeffPoly>{pt}, prm)[0];
}

// 3^(steps mod n/2) mod 2n (negative steps rotate right) and 2n - 1: the keys to generate
inline size_t galois_element_rotate_rows(size_t n, int64_t steps) {
    uint64_t el = 0;
    detail::check(exacto_galois_element_rotate_rows(n, steps, &el));
    return (size_t)el;
}
inline size_t galois_element_swap_rows(size_t n) {
    uint64_t el = 0;
    detail::check(exacto_galois_element_swap_rows(n, &el));
    return (size_t)el;
}

// both slot rows left by `steps`; gk is the key of galois_element_rotate_rows(n, steps), or nullptr
// when steps == 0 (mod n/2), which copies
inline std::vector<BfvCiphertext> bfv_rotate_rows(const std::vector<BfvCiphertext>& cts, int64_t steps,
                                                  const GaloisKey* gk) {
    if (cts.empty()) return {};
    const BfvParams& prm = *cts[0].params;
    const size_t polys = cts[0].c.size();
    auto flat = detail::flatten(cts, polys);
    std::vector<uint64_t> key;
    if (gk) key = detail::flatten_key(gk->keys);
    std::vector<uint64_t> out(flat.size());
    detail::check(exacto_bfv_rotate_rows(prm.ctx(), flat.data(), polys, steps, key.empty() ? nullptr : key.data(),
                                         gk ? gk->keys.size() : 0, out.data(), cts.size()));
    return detail::unflatten(out, cts.size(), polys, cts[0].params);
}
inline BfvCiphertext bfv_rotate_rows(const BfvCiphertext& ct, int64_t steps, const GaloisKey& gk) {
    return bfv_rotate_rows(std::vector<BfvCiphertext>{ct}, steps, &gk)[0];
}
inline std::vector<BfvCiphertext> bfv_swap_rows(const std::vector<BfvCiphertext>& cts, const GaloisKey& gk) {
    if (cts.empty()) return {};
    const BfvParams& prm = *cts[0].params;
    const size_t polys = cts[0].c.size();
    auto flat = detail::flatten(cts, polys);
    auto key = detail::flatten_key(gk.keys);
    std::vector<uint64_t> out(flat.size());
    detail::check(exacto_bfv_swap_rows(prm.ctx(), flat.data(), polys, key.empty() ? nullptr : key.data(),
                                       gk.keys.size(), out.data(), cts.size()));
    return detail::unflatten(out, cts.size(), polys, cts[0].params);
}
inline BfvCiphertext bfv_swap_rows(const BfvCiphertext& ct, const GaloisKey& gk) {
    return bfv_swap_rows(std::vector<BfvCiphertext>{ct}, gk)[0];
}

// ---- hoisted rotations and slot linear transforms (exacto_hip.h, "Hoisted rotations ...")
// perm[p]: NTT(sigma_element(a))[p] = NTT(a)[perm[p]] in the library's NTT-domain order; element odd
inline std::vector<uint32_t> galois_ntt_permutation(size_t n, uint64_t element) {
    std::vector<uint32_t> perm(n ? n : 1);
    detail::check(exacto_galois_ntt_permutation(n, element, perm.data()));
    perm.resize(n);
    return perm;
}

// Galois keys prepared once for hoisted rotations.  keys[r] is the key of elements()[r]; an identity
// element (1 mod 2n) takes no key: pass a default-constructed GaloisKey with that element.  The set keeps its
// parameters (and with them the context) alive and releases its device memory first.
class GaloisKeySet {
public:
    GaloisKeySet(const BfvParamsPtr& prm, const std::vector<GaloisKey>& keys) : params_(prm) {
        const size_t Ln = prm->num_limbs() * prm->ring_degree;
        size_t nk = 0;
        for (const auto& k : keys) {
            elements_.push_back(k.element);
            nk = std::max(nk, k.keys.size());
        }
        std::vector<uint64_t> flat(keys.size() * nk * 2 * Ln, 0);
        for (size_t r = 0; r < keys.size(); ++r) {
            if (keys[r].keys.empty()) continue;   // identity: the slot is never read
            if (keys[r].keys.size() != nk) throw ExactoError(EXACTO_ERR_INVALID_PARAM, "invalid parameter: galois keys of one set need the same number of digits");
            const auto f = detail::flatten_key(keys[r].keys);
            std::copy(f.begin(), f.end(), flat.begin() + r * nk * 2 * Ln);
        }
        detail::check(exacto_galois_keyset_create(prm->ctx(), elements_.data(), elements_.size(),
                                                  flat.empty() ? nullptr : flat.data(), nk, &h_));
    }
    GaloisKeySet(const GaloisKeySet&) = delete;
    GaloisKeySet& operator=(const GaloisKeySet&) = delete;
    GaloisKeySet(GaloisKeySet&& o) noexcept : params_(std::move(o.params_)), elements_(std::move(o.elements_)), h_(o.h_) {
        o.h_ = nullptr;
    }
    ~GaloisKeySet() { exacto_galois_keyset_destroy(h_); }
    const exacto_galois_keyset* handle() const { return h_; }
    const std::vector<uint64_t>& elements() const { return elements_; }
    size_t size() const { return elements_.size(); }
    const BfvParamsPtr& params() const { return params_; }
    // the 31-bit primes of the set's key switch (0: the limb-wise multiply-accumulate)
    int ks32_primes() const {
        int s = 0;
        detail::check(exacto_galois_keyset_info(h_, nullptr, nullptr, &s));
        return s;
    }

private:
    BfvParamsPtr params_;
    std::vector<uint64_t> elements_;
    exacto_galois_keyset* h_ = nullptr;
};

// out[b][r] = the set's automorphism r of cts[b] on the shared gadget digits of its c1: the same plaintexts
// and noise bound as bfv_apply_automorphism, not its bits
inline std::vector<std::vector<BfvCiphertext>> bfv_rotate_hoisted(const std::vector<BfvCiphertext>& cts,
                                                                  const GaloisKeySet& ks) {
    if (cts.empty()) return {};
    const BfvParams& prm = *cts[0].params;
    if (cts[0].c.size() != 2) throw ExactoError(EXACTO_ERR_INVALID_PARAM, "invalid parameter: automorphism requires degree-1 ciphertext");
    auto flat = detail::flatten(cts, 2);
    std::vector<uint64_t> out(flat.size() * ks.size());
    detail::check(exacto_bfv_rotate_hoisted(prm.ctx(), ks.handle(), flat.data(), out.data(), cts.size()));
    auto all = detail::unflatten(out, cts.size() * ks.size(), 2, cts[0].params);
    std::vector<std::vector<BfvCiphertext>> res(cts.size());
    for (size_t b = 0; b < cts.size(); ++b)
        res[b].assign(all.begin() + b * ks.size(), all.begin() + (b + 1) * ks.size());
    return res;
}
inline std::vector<BfvCiphertext> bfv_rotate_hoisted(const BfvCiphertext& ct, const GaloisKeySet& ks) {
    return bfv_rotate_hoisted(std::vector<BfvCiphertext>{ct}, ks)[0];
}

// out[b] = sum_r pts[r] * (automorphism r of cts[b]); pts[r] plaintext coefficients, lifted as bfv_plain_mul's
inline std::vector<BfvCiphertext> bfv_linear_transform(const std::vector<BfvCiphertext>& cts, const GaloisKeySet& ks,
                                                       const std::vector<CoeffPoly>& pts) {
    if (cts.empty()) return {};
    const BfvParams& prm = *cts[0].params;
    if (cts[0].c.size() != 2) throw ExactoError(EXACTO_ERR_INVALID_PARAM, "invalid parameter: automorphism requires degree-1 ciphertext");
    if (pts.size() != ks.size()) throw ExactoError(EXACTO_ERR_INVALID_PARAM, "invalid parameter: one plaintext per element of the key set");
    auto flat = detail::flatten(cts, 2);
    std::vector<uint64_t> p(pts.size() * prm.ring_degree), out(flat.size());
    for (size_t r = 0; r < pts.size(); ++r) {
        if (pts[r].coeffs.size() != prm.ring_degree) throw ExactoError(EXACTO_ERR_INVALID_PARAM, "invalid parameter: plaintext length");
        std::copy(pts[r].coeffs.begin(), pts[r].coeffs.end(), p.begin() + r * prm.ring_degree);
    }
    detail::check(exacto_bfv_linear_transform(prm.ctx(), ks.handle(), flat.data(), p.data(), out.data(), cts.size()));
    return detail::unflatten(out, cts.size(), 2, cts[0].params);
}

// batch_encode + encrypt_sk / encrypt_pk, and decrypt + batch_decode, composed on the device
inline std::vector<BfvCiphertext> batch_encrypt(const std::vector<SlotVector>& values, const SecretKey* sk,
                                                const PublicKey* pk, const BfvParamsPtr& prm, ChaChaRng& rng) {
    const size_t Ln = prm->num_limbs() * prm->ring_degree;
    auto flat = detail::flatten_slots(values, prm->ring_degree);
    std::vector<uint64_t> ct(values.size() * 2 * Ln);
    if (sk) {
        detail::check(exacto_batch_encrypt_sk(prm->ctx(), flat.data(), sk->poly.data.data(), prm->sigma, rng.key,
                                              rng.next(), ct.data(), values.size()));
    } else {
        std::vector<uint64_t> pkf(pk->pk0.data);
        pkf.insert(pkf.end(), pk->pk1.data.begin(), pk->pk1.data.end());
        detail::check(exacto_batch_encrypt_pk(prm->ctx(), flat.data(), pkf.data(), prm->sigma, rng.key, rng.next(),
                                              ct.data(), values.size()));
    }
    return detail::unflatten(ct, values.size(), 2, prm);
}
inline BfvCiphertext batch_encrypt_sk(const SlotVector& values, const SecretKey& sk, const BfvParamsPtr& prm,
                                      ChaChaRng& rng) {
    return batch_encrypt({values}, &sk, nullptr, prm, rng)[0];
}
inline BfvCiphertext batch_encrypt_pk(const SlotVector& values, const PublicKey& pk, const BfvParamsPtr& prm,
                                      ChaChaRng& rng) {
    return batch_encrypt({values}, nullptr, &pk, prm, rng)[0];
}
inline std::vector<SlotVector> batch_decrypt(const std::vector<BfvCiphertext>& cts, const SecretKey& sk) {
    if (cts.empty()) return {};
    const BfvParams& prm = *cts[0].params;
    const size_t polys = cts[0].c.size(), n = prm.ring_degree;
    auto flat = detail::flatten(cts, polys);
    std::vector<uint64_t> out(cts.size() * n);
    detail::check(exacto_batch_decrypt(prm.ctx(), flat.data(), polys, sk.poly.data.data(), out.data(), cts.size()));
    return detail::split_slots(out, cts.size(), n);
}
inline SlotVector batch_decrypt(const BfvCiphertext& ct, const SecretKey& sk) {
    return batch_decrypt(std::vector<BfvCiphertext>{ct}, sk)[0];
}

// ---- plaintext operations and the trace (src/bfv/eval.rs:468-652)
namespace detail {
inline std::vector<uint64_t> flatten_pts(const std::vector<CoeffPoly>& pts, size_t n) {
    std::vector<uint64_t> out;
    for (auto& p : pts) {
        if (p.coeffs.size() != n) throw ExactoError(2, "dimension mismatch: expected " + std::to_string(n) +
                                                           ", got " + std::to_string(p.coeffs.size()));
        out.insert(out.end(), p.coeffs.begin(), p.coeffs.end());
    }
    return out;
}
inline BfvCiphertext one_ct(const std::vector<uint64_t>& flat, size_t polys, const BfvParamsPtr& prm) {
    return unflatten(flat, 1, polys, prm)[0];
}
}  // namespace detail

inline BfvCiphertext bfv_plain_mul(const BfvCiphertext& ct, const CoeffPoly& pt) {
    const BfvParams& prm = *ct.params;
    auto flat = detail::flatten({ct}, ct.c.size());
    auto p = detail::flatten_pts({pt}, prm.ring_degree);
    std::vector<uint64_t> out(flat.size());
    detail::check(exacto_bfv_plain_mul(prm.ctx(), flat.data(), ct.c.size(), p.data(), out.data(), 1));
    return detail::one_ct(out, ct.c.size(), ct.params);
}
inline BfvCiphertext bfv_plain_add(const BfvCiphertext& ct, const CoeffPoly& pt) {
    const BfvParams& prm = *ct.params;
    auto flat = detail::flatten({ct}, ct.c.size());
    auto p = detail::flatten_pts({pt}, prm.ring_degree);
    std::vector<uint64_t> out(flat.size());
    detail::check(exacto_bfv_plain_add(prm.ctx(), flat.data(), ct.c.size(), p.data(), out.data(), 1));
    return detail::one_ct(out, ct.c.size(), ct.params);
}
inline BfvCiphertext bfv_monomial_mul(const BfvCiphertext& ct, size_t j) {
    const BfvParams& prm = *ct.params;
    auto flat = detail::flatten({ct}, ct.c.size());
    std::vector<uint64_t> out(flat.size());
    detail::check(exacto_bfv_monomial_mul(prm.ctx(), flat.data(), ct.c.size(), j, out.data(), 1));
    return detail::one_ct(out, ct.c.size(), ct.params);
}
inline BfvCiphertext bfv_inner_product(const std::vector<BfvCiphertext>& cts, const std::vector<CoeffPoly>& pts) {
    if (cts.empty() || cts.size() != pts.size()) throw ExactoError(1, "invalid parameter: mismatched ct/pt lengths");
    const BfvParams& prm = *cts[0].params;
    const size_t polys = cts[0].c.size();
    auto flat = detail::flatten(cts, polys);
    auto p = detail::flatten_pts(pts, prm.ring_degree);
    std::vector<uint64_t> out(polys * prm.num_limbs() * prm.ring_degree);
    detail::check(exacto_bfv_inner_product(prm.ctx(), flat.data(), p.data(), cts.size(), polys, out.data()));
    return detail::one_ct(out, polys, cts[0].params);
}

// HashMap<usize, GaloisKey> of the reference
using GaloisKeys = std::map<size_t, GaloisKey>;
namespace detail {
// the map as (elements, keys stacked in that order); every key must carry the same digit count
inline size_t pack_keys(const GaloisKeys& keys, std::vector<uint64_t>& els, std::vector<uint64_t>& flat) {
    size_t nk = 0;
    for (auto& kv : keys) {
        if (nk == 0) nk = kv.second.keys.size();
        if (kv.second.keys.size() != nk) throw ExactoError(1, "invalid parameter: Galois keys differ in digit count");
        els.push_back(kv.first);
        for (auto& k : kv.second.keys) {
            flat.insert(flat.end(), k.first.data.begin(), k.first.data.end());
            flat.insert(flat.end(), k.second.data.begin(), k.second.data.end());
        }
    }
    return nk;
}
}  // namespace detail

// bfv_trace (eval.rs:572-586)
inline BfvCiphertext bfv_trace(const BfvCiphertext& ct, const std::vector<size_t>& elements, const GaloisKeys& keys) {
    const BfvParams& prm = *ct.params;
    std::vector<uint64_t> els, flat;
    size_t nk = 0;
    for (size_t k : elements) {
        auto it = keys.find(k);
        if (it == keys.end()) throw ExactoError(1, "invalid parameter: missing Galois key for element " + std::to_string(k));
        if (nk == 0) nk = it->second.keys.size();
        els.push_back(k);
        for (auto& kp : it->second.keys) {
            flat.insert(flat.end(), kp.first.data.begin(), kp.first.data.end());
            flat.insert(flat.end(), kp.second.data.begin(), kp.second.data.end());
        }
    }
    auto c = detail::flatten({ct}, ct.c.size());
    std::vector<uint64_t> out(c.size());
    detail::check(exacto_bfv_trace(prm.ctx(), c.data(), ct.c.size(), els.data(), els.size(),
                                   flat.empty() ? nullptr : flat.data(), nk, out.data(), 1));
    return detail::one_ct(out, ct.c.size(), ct.params);
}

// ---- exacto::bootstrap::coeffs_to_slots (src/bootstrap/coeffs_to_slots.rs)
inline std::vector<size_t> required_trace_elements(size_t n) {
    std::vector<uint64_t> v(exacto_required_trace_elements(n, nullptr, 0));
    exacto_required_trace_elements(n, v.data(), v.size());
    return std::vector<size_t>(v.begin(), v.end());
}
inline GaloisKeys gen_trace_galois_keys(const SecretKey& sk, ChaChaRng& rng) {
    GaloisKeys keys;
    for (size_t k : required_trace_elements(sk.params->ring_degree)) keys[k] = gen_galois_key_with_rng(sk, k, rng);
    return keys;
}
inline GaloisKeys gen_all_galois_keys(const SecretKey& sk, ChaChaRng& rng) {
    GaloisKeys keys;
    for (size_t k = 3; k < 2 * sk.params->ring_degree; k += 2) keys[k] = gen_galois_key_with_rng(sk, k, rng);
    return keys;
}
namespace detail {
inline std::vector<BfvCiphertext> extract_range(const BfvCiphertext& ct, size_t j0, size_t count,
                                                const GaloisKeys& keys) {
    const BfvParams& prm = *ct.params;
    if (ct.c.size() != 2) throw ExactoError(1, "invalid parameter: automorphism requires degree-1 ciphertext");
    std::vector<uint64_t> els, flat;
    const size_t nk = pack_keys(keys, els, flat);
    auto c = flatten({ct}, 2);
    std::vector<uint64_t> out(count * c.size());
    check(exacto_extract_coefficients(prm.ctx(), c.data(), j0, count, els.data(), els.size(),
                                      flat.empty() ? nullptr : flat.data(), nk, out.data()));
    return unflatten(out, count, 2, ct.params);
}
}  // namespace detail
inline BfvCiphertext extract_coefficient(const BfvCiphertext& ct, size_t j, const GaloisKeys& keys) {
    return detail::extract_range(ct, j, 1, keys)[0];
}
inline std::vector<BfvCiphertext> coeffs_to_slots(const BfvCiphertext& ct, const GaloisKeys& keys) {
    return detail::extract_range(ct, 0, ct.params->ring_degree, keys);
}
inline BfvCiphertext slots_to_coeffs(const std::vector<BfvCiphertext>& slots) {
    if (slots.empty()) throw ExactoError(1, "invalid parameter: empty slots");
    const BfvParams& prm = *slots[0].params;
    const size_t polys = slots[0].c.size();
    auto flat = detail::flatten(slots, polys);
    std::vector<uint64_t> out(polys * prm.num_limbs() * prm.ring_degree);
    detail::check(exacto_slots_to_coeffs(prm.ctx(), flat.data(), slots.size(), polys, out.data()));
    return detail::one_ct(out, polys, slots[0].params);
}

// ---- exacto::bootstrap::digit_extract (src/bootstrap/digit_extract.rs)
inline std::vector<uint64_t> lagrange_interpolate(const std::vector<uint64_t>& values, uint64_t p) {
    std::vector<uint64_t> out(values.size());
    if (!values.empty()) detail::check(exacto_lagrange_interpolate(values.data(), values.size(), p, out.data()));
    return out;
}
inline std::vector<uint64_t> compute_rounding_poly(uint64_t t_orig, uint64_t q_prime, uint64_t t_boot) {
    std::vector<uint64_t> out(t_boot);
    detail::check(exacto_compute_rounding_poly(t_orig, q_prime, t_boot, out.data()));
    return out;
}
inline BfvCiphertext trivial_encrypt_poly(const CoeffPoly& pt, const BfvParamsPtr& prm) {
    auto p = detail::flatten_pts({pt}, prm->ring_degree);
    std::vector<uint64_t> out(2 * prm->num_limbs() * prm->ring_degree);
    detail::check(exacto_trivial_encrypt(prm->ctx(), p.data(), out.data(), 1));
    return detail::one_ct(out, 2, prm);
}
inline BfvCiphertext trivial_encrypt(uint64_t m, const BfvParamsPtr& prm) {
    CoeffPoly p;
    p.coeffs.assign(prm->ring_degree, 0);
    p.coeffs[0] = m % prm->plain_modulus;
    p.modulus = prm->plain_modulus;
    return trivial_encrypt_poly(p, prm);
}
inline BfvCiphertext eval_poly_homomorphic(const BfvCiphertext& ct, const std::vector<uint64_t>& coeffs,
                                           const RelinKey& rlk) {
    const BfvParams& prm = *ct.params;
    if (coeffs.size() > 1) detail::load_key(rlk);
    auto c = detail::flatten({ct}, 2);
    std::vector<uint64_t> out(c.size());
    detail::check(exacto_eval_poly(prm.ctx(), c.data(), coeffs.data(), coeffs.size(), out.data(), 1));
    return detail::one_ct(out, 2, ct.params);
}

// ---- exacto::bootstrap::bfv_host (src/bootstrap/bfv_host.rs)
struct BootstrapKey {
    BfvCiphertext bsk;
    BfvParamsPtr boot_params;
    RelinKey boot_rlk;
    GaloisKeys galois_keys;
    std::vector<uint64_t> rounding_poly;
    uint64_t t_orig = 0, q_prime = 0;
    SecretKey boot_sk;  // create_boot_sk's key (the reference recomputes it in its tests)
};

inline BootstrapKey gen_bootstrap_key(const SecretKey& sk, const BfvParamsPtr& boot_params, uint64_t q_prime,
                                      uint64_t t_orig, ChaChaRng& rng) {
    const BfvParams& o = *sk.params;
    const size_t n = o.ring_degree;
    std::vector<uint64_t> boot_sk(boot_params->num_limbs() * n), s_pt(n);
    detail::check(exacto_bootstrap_key_material(o.ctx(), boot_params->ctx(), sk.poly.data.data(), boot_sk.data(),
                                                s_pt.data()));
    BootstrapKey k;
    k.boot_params = boot_params;
    k.boot_sk = SecretKey{detail::make_poly(*boot_params, boot_sk.data()), boot_params};
    CoeffPoly spt{s_pt, boot_params->plain_modulus};
    k.bsk = encrypt_sk_with_rng(spt, k.boot_sk, boot_params, rng);
    k.boot_rlk = gen_relin_key_with_rng(k.boot_sk, rng);
    k.galois_keys = gen_trace_galois_keys(k.boot_sk, rng);
    k.rounding_poly = compute_rounding_poly(t_orig, q_prime, boot_params->plain_modulus);
    k.t_orig = t_orig;
    k.q_prime = q_prime;
    return k;
}

inline std::vector<BfvCiphertext> bfv_bootstrap(const std::vector<BfvCiphertext>& cts, const BootstrapKey& bsk) {
    if (cts.empty()) return {};
    const BfvParams& o = *cts[0].params;
    const BfvParams& b = *bsk.boot_params;
    if (cts[0].c.size() != 2) throw ExactoError(1, "invalid parameter: bootstrap requires degree-1 ciphertext");
    detail::load_key(bsk.boot_rlk);
    auto flat = detail::flatten(cts, 2);
    auto key = detail::flatten({bsk.bsk}, 2);
    std::vector<uint64_t> els, gks;
    const size_t nk = detail::pack_keys(bsk.galois_keys, els, gks);
    std::vector<uint64_t> out(cts.size() * 2 * b.num_limbs() * b.ring_degree);
    detail::check(exacto_bfv_bootstrap(o.ctx(), b.ctx(), flat.data(), 2, key.data(), bsk.rounding_poly.data(),
                                       bsk.rounding_poly.size(), bsk.q_prime, els.data(), els.size(),
                                       gks.empty() ? nullptr : gks.data(), nk, out.data(), cts.size()));
    return detail::unflatten(out, cts.size(), 2, bsk.boot_params);
}
inline BfvCiphertext bfv_bootstrap(const BfvCiphertext& ct, const BootstrapKey& bsk) {
    return bfv_bootstrap(std::vector<BfvCiphertext>{ct}, bsk)[0];
}

// ---- exacto::dbfv
struct DbfvParams {
    BfvParamsPtr bfv_params;
    uint64_t base;
    size_t num_digits;
    uint64_t plain_modulus;  // 0 == 2^64
};

struct DbfvCiphertext {
    std::vector<BfvCiphertext> limbs;
    size_t degree = 0;
    size_t mul_depth = 0;
    std::shared_ptr<const DbfvParams> params;
    size_t num_limbs() const { return limbs.size(); }
};

// dbfv_mul (src/dbfv/eval.rs:82-149), batched over independent products.
inline std::vector<DbfvCiphertext> dbfv_mul(const std::vector<DbfvCiphertext>& a,
                                            const std::vector<DbfvCiphertext>& b, const RelinKey& rlk) {
    if (a.empty()) return {};
    const auto& dp = *a[0].params;
    const size_t d = dp.num_digits;
    for (size_t i = 0; i < a.size(); ++i)
        if (a[i].num_limbs() != d || b[i].num_limbs() != d)
            throw ExactoError(1, "invalid parameter: multiplication requires d-limb ciphertexts");
    detail::load_key(rlk);
    std::vector<uint64_t> fa, fb;
    std::vector<uint32_t> da, db, dout(a.size());
    for (size_t i = 0; i < a.size(); ++i) {
        auto x = detail::flatten(a[i].limbs, 2), y = detail::flatten(b[i].limbs, 2);
        fa.insert(fa.end(), x.begin(), x.end());
        fb.insert(fb.end(), y.begin(), y.end());
        da.push_back((uint32_t)a[i].mul_depth);
        db.push_back((uint32_t)b[i].mul_depth);
    }
    std::vector<uint64_t> out(fa.size());
    detail::check(exacto_dbfv_mul(dp.bfv_params->ctx(), d, dp.base, dp.plain_modulus, fa.data(), fb.data(),
                                  out.data(), a.size(), da.data(), db.data(), dout.data()));
    std::vector<DbfvCiphertext> res(a.size());
    const size_t per = d * 2 * dp.bfv_params->num_limbs() * dp.bfv_params->ring_degree;
    for (size_t i = 0; i < a.size(); ++i) {
        std::vector<uint64_t> slice(out.begin() + (long)(i * per), out.begin() + (long)((i + 1) * per));
        res[i].limbs = detail::unflatten(slice, d, 2, dp.bfv_params);
        res[i].degree = d;
        res[i].mul_depth = dout[i];
        res[i].params = a[0].params;
    }
    return res;
}

inline DbfvCiphertext dbfv_mul(const DbfvCiphertext& a, const DbfvCiphertext& b, const RelinKey& rlk) {
    return dbfv_mul(std::vector<DbfvCiphertext>{a}, std::vector<DbfvCiphertext>{b}, rlk)[0];
}

// dbfv_mul(a, a, rlk) (exacto_dbfv_square): d (d + 1) / 2 of the d^2 digit-pair products, bit for bit.
inline std::vector<DbfvCiphertext> dbfv_square(const std::vector<DbfvCiphertext>& a, const RelinKey& rlk) {
    if (a.empty()) return {};
    const auto& dp = *a[0].params;
    const size_t d = dp.num_digits;
    for (size_t i = 0; i < a.size(); ++i)
        if (a[i].num_limbs() != d) throw ExactoError(1, "invalid parameter: multiplication requires d-limb ciphertexts");
    detail::load_key(rlk);
    std::vector<uint64_t> fa;
    std::vector<uint32_t> da, dout(a.size());
    for (size_t i = 0; i < a.size(); ++i) {
        auto x = detail::flatten(a[i].limbs, 2);
        fa.insert(fa.end(), x.begin(), x.end());
        da.push_back((uint32_t)a[i].mul_depth);
    }
    std::vector<uint64_t> out(fa.size());
    detail::check(exacto_dbfv_square(dp.bfv_params->ctx(), d, dp.base, dp.plain_modulus, fa.data(), out.data(), a.size(),
                                     da.data(), dout.data()));
    std::vector<DbfvCiphertext> res(a.size());
    const size_t per = d * 2 * dp.bfv_params->num_limbs() * dp.bfv_params->ring_degree;
    for (size_t i = 0; i < a.size(); ++i) {
        std::vector<uint64_t> slice(out.begin() + (long)(i * per), out.begin() + (long)((i + 1) * per));
        res[i].limbs = detail::unflatten(slice, d, 2, dp.bfv_params);
        res[i].degree = d;
        res[i].mul_depth = dout[i];
        res[i].params = a[0].params;
    }
    return res;
}

inline DbfvCiphertext dbfv_square(const DbfvCiphertext& a, const RelinKey& rlk) {
    return dbfv_square(std::vector<DbfvCiphertext>{a}, rlk)[0];
}

namespace detail {
inline std::vector<uint64_t> flatten_dbfv(const DbfvCiphertext& ct) {
    if (ct.num_limbs() != ct.params->num_digits)
        throw ExactoError(1, "invalid parameter: expected d-limb dBFV ciphertext");
    return flatten(ct.limbs, 2);
}
}  // namespace detail

// dbfv_decrypt (src/dbfv/decrypt.rs:20-43): scalar plaintext (coefficient 0).
inline uint64_t dbfv_decrypt(const DbfvCiphertext& ct, const SecretKey& sk) {
    const auto& dp = *ct.params;
    auto flat = detail::flatten_dbfv(ct);
    uint64_t out = 0;
    detail::check(exacto_dbfv_decrypt(dp.bfv_params->ctx(), dp.num_digits, dp.base, dp.plain_modulus, flat.data(),
                                      sk.poly.data.data(), &out, 1));
    return out;
}

// dbfv_decrypt_poly (src/dbfv/decrypt.rs:48-79).
inline CoeffPoly dbfv_decrypt_poly(const DbfvCiphertext& ct, const SecretKey& sk) {
    const auto& dp = *ct.params;
    auto flat = detail::flatten_dbfv(ct);
    CoeffPoly res;
    res.coeffs.resize(dp.bfv_params->ring_degree);
    res.modulus = dp.plain_modulus;
    detail::check(exacto_dbfv_decrypt_poly(dp.bfv_params->ctx(), dp.num_digits, dp.base, dp.plain_modulus,
                                           flat.data(), sk.poly.data.data(), res.coeffs.data(), 1));
    return res;
}

// ---- noise (src/bin/paper_repro.rs:238-281: max_limb_noise, bfv_noise_inf), exact over the full Q
// A noise value: little-endian 64-bit words, one per ciphertext prime (Q < 2^(64 L)).
struct Noise {
    std::vector<uint64_t> words;
    size_t bit_length() const {
        for (size_t k = words.size(); k-- > 0;)
            if (words[k]) return 64 * k + (64 - (size_t)__builtin_clzll(words[k]));
        return 0;
    }
    bool fits_u64() const { return bit_length() <= 64; }
    // the reference's u64 (paper_repro.rs returns one); throws when the value needs more words
    uint64_t to_u64() const {
        if (!fits_u64()) throw ExactoError(1, "invalid parameter: noise value does not fit 64 bits");
        return words.empty() ? 0 : words[0];
    }
};

namespace detail {
// bitlen(floor(floor(Q / p) / 2)) for Q = prod moduli (host only)
inline size_t half_delta_bits(const std::vector<uint64_t>& moduli, uint64_t plain) {
    if (plain == 0) throw ExactoError(1, "invalid parameter: plain_modulus must be non-zero");
    std::vector<uint64_t> q(1, 1);
    for (uint64_t m : moduli) {
        unsigned __int128 carry = 0;
        for (auto& w : q) {
            const unsigned __int128 t = (unsigned __int128)w * m + carry;
            w = (uint64_t)t;
            carry = t >> 64;
        }
        if (carry) q.push_back((uint64_t)carry);
    }
    Noise delta;
    delta.words.resize(q.size());
    unsigned __int128 rem = 0;
    for (size_t k = q.size(); k-- > 0;) {
        const unsigned __int128 cur = (rem << 64) | q[k];
        delta.words[k] = (uint64_t)(cur / plain);
        rem = cur % plain;
    }
    const size_t bits = delta.bit_length();
    return bits ? bits - 1 : 0;
}
}  // namespace detail

// max(0, bitlen(floor(Delta / 2)) - bitlen(noise)), Delta = floor(Q / p): the bits left before
// decryption can fail.
inline size_t noise_budget_bits(const Noise& noise, const std::vector<uint64_t>& moduli, uint64_t plain) {
    const size_t have = detail::half_delta_bits(moduli, plain), used = noise.bit_length();
    return have > used ? have - used : 0;
}
inline size_t noise_budget_bits(const Noise& noise, const BfvParams& prm) {
    return noise_budget_bits(noise, prm.ct_moduli, prm.plain_modulus);
}

// bfv_noise_inf (paper_repro.rs:249-281), batched over ciphertexts of one degree: max |phase - Delta m|
// centred mod Q against the decrypted m.  At L = 1 the reference's value; for L >= 2 the same formula
// over the full Q.
inline std::vector<Noise> bfv_noise_inf(const std::vector<BfvCiphertext>& cts, const SecretKey& sk) {
    if (cts.empty()) return {};
    const BfvParams& prm = *cts[0].params;
    const size_t polys = cts[0].c.size(), L = prm.num_limbs();
    auto flat = detail::flatten(cts, polys);
    std::vector<uint64_t> out(cts.size() * L);
    detail::check(exacto_bfv_noise(prm.ctx(), flat.data(), polys, sk.poly.data.data(), nullptr, nullptr, out.data(),
                                   cts.size()));
    std::vector<Noise> res(cts.size());
    for (size_t b = 0; b < cts.size(); ++b)
        res[b].words.assign(out.begin() + (long)(b * L), out.begin() + (long)((b + 1) * L));
    return res;
}
inline Noise bfv_noise_inf(const BfvCiphertext& ct, const SecretKey& sk) {
    return bfv_noise_inf(std::vector<BfvCiphertext>{ct}, sk)[0];
}

// max_limb_noise (paper_repro.rs:238-247): the maximum of bfv_noise_inf over the limbs.
inline Noise max_limb_noise(const DbfvCiphertext& ct, const SecretKey& sk) {
    const auto& dp = *ct.params;
    auto flat = detail::flatten_dbfv(ct);
    Noise res;
    res.words.resize(dp.bfv_params->num_limbs());
    detail::check(exacto_dbfv_noise(dp.bfv_params->ctx(), dp.num_digits, flat.data(), sk.poly.data.data(),
                                    res.words.data(), 1));
    return res;
}

// ---- exacto::bfv::modswitch (src/bfv/modswitch.rs) and its exact form
namespace detail {
// `lower` continues `upper`: same n and p, ct_moduli a proper prefix of upper's
inline bool is_lower_level(const BfvParams& upper, const BfvParams& lower) {
    return lower.ring_degree == upper.ring_degree && lower.plain_modulus == upper.plain_modulus &&
           !lower.ct_moduli.empty() && lower.ct_moduli.size() < upper.ct_moduli.size() &&
           std::equal(lower.ct_moduli.begin(), lower.ct_moduli.end(), upper.ct_moduli.begin());
}
inline BfvCiphertext mod_switch_to(const BfvCiphertext& ct, size_t limbs_out, int mode, const BfvParamsPtr& carry) {
    const BfvParams& prm = *ct.params;
    const size_t polys = ct.c.size(), n = prm.ring_degree, lin = polys ? ct.c[0].num_limbs : 0;
    auto flat = flatten({ct}, polys);
    std::vector<uint64_t> out(polys * limbs_out * n);
    check(exacto_bfv_mod_switch(prm.ctx(), flat.data(), polys, lin, limbs_out, mode, out.data(), 1));
    BfvCiphertext res;
    res.params = carry;
    res.c.resize(polys);
    for (size_t k = 0; k < polys; ++k) {
        res.c[k].ring_degree = n;
        res.c[k].num_limbs = limbs_out;
        res.c[k].data.assign(out.begin() + (long)(k * limbs_out * n), out.begin() + (long)((k + 1) * limbs_out * n));
    }
    return res;
}
}  // namespace detail

// mod_switch_drop_prime (modswitch.rs:13-34), literally: the last RNS component dropped with the
// reference's "simplified" correction (unscaled, uncentred), the same `params` kept; the polys have
// L - 1 limbs.  Its output does not decrypt under the smaller modulus: use mod_switch for that.
inline BfvCiphertext mod_switch_drop_prime(const BfvCiphertext& ct) {
    const size_t lin = ct.c.empty() ? ct.params->num_limbs() : ct.c[0].num_limbs;
    return detail::mod_switch_to(ct, lin > 0 ? lin - 1 : 0, EXACTO_MODSWITCH_REFERENCE, ct.params);
}

// The exact modulus switch down to `lower` (ct_moduli a proper prefix of the input's, same n and p, else
// ModulusMismatch): one rounding division per dropped prime.  The result carries `lower`, under which it
// decrypts (with the secret key's first limbs) and multiplies (with a relinearisation key of its own:
// gadget digits depend on Q).
inline BfvCiphertext mod_switch(const BfvCiphertext& ct, BfvParamsPtr lower) {
    if (!lower || !detail::is_lower_level(*ct.params, *lower))
        throw ExactoError(EXACTO_ERR_MODULUS_MISMATCH, "modulus mismatch");
    return detail::mod_switch_to(ct, lower->num_limbs(), EXACTO_MODSWITCH_ROUND, lower);
}

// The secret key under a lower level's parameters: its first limbs (per-prime tables depend only on (n, q_i)).
inline SecretKey lower_secret_key(const SecretKey& sk, BfvParamsPtr lower) {
    if (!lower || !detail::is_lower_level(*sk.params, *lower))
        throw ExactoError(EXACTO_ERR_MODULUS_MISMATCH, "modulus mismatch");
    SecretKey res;
    res.params = lower;
    res.poly.ring_degree = sk.poly.ring_degree;
    res.poly.num_limbs = lower->num_limbs();
    res.poly.data.assign(sk.poly.data.begin(), sk.poly.data.begin() + (long)(lower->num_limbs() * sk.poly.ring_degree));
    return res;
}

// ---- exacto::dbfv beyond the product: keygen, encrypt, eval, keyswitch, advanced
using DbfvParamsPtr = std::shared_ptr<const DbfvParams>;

// dbfv_keygen / dbfv_keygen_full (src/dbfv/keygen.rs:9-30) with the caller's RNG, as every
// generator of this header takes it.
struct DbfvKeys {
    SecretKey sk;
    PublicKey pk;
    RelinKey rlk;
    std::vector<GaloisKey> gks;
};
inline DbfvKeys dbfv_keygen_full(const DbfvParamsPtr& params, const std::vector<size_t>& galois_elements,
                                 ChaChaRng& rng) {
    DbfvKeys k;
    k.sk = gen_secret_key_with_rng(params->bfv_params, rng);
    k.pk = gen_public_key_with_rng(k.sk, rng);
    k.rlk = gen_relin_key_with_rng(k.sk, rng);
    for (size_t e : galois_elements) k.gks.push_back(gen_galois_key_with_rng(k.sk, e, rng));
    return k;
}
inline DbfvKeys dbfv_keygen(const DbfvParamsPtr& params, ChaChaRng& rng) { return dbfv_keygen_full(params, {}, rng); }

namespace detail {
inline DbfvCiphertext make_dbfv(const std::vector<uint64_t>& flat, size_t d, size_t polys, size_t degree,
                                size_t mul_depth, const DbfvParamsPtr& params) {
    DbfvCiphertext res;
    res.limbs = unflatten(flat, d, polys, params->bfv_params);
    res.degree = degree;
    res.mul_depth = mul_depth;
    res.params = params;
    return res;
}
inline size_t dbfv_polys(const DbfvCiphertext& ct) {
    if (ct.limbs.empty()) throw ExactoError(1, "invalid parameter: empty dBFV ciphertext");
    return ct.limbs[0].c.size();
}
inline size_t limb_words(const DbfvParams& dp) { return dp.bfv_params->num_limbs() * dp.bfv_params->ring_degree; }
inline DbfvCiphertext dbfv_encrypt_any(const uint64_t* src, bool poly, const SecretKey* sk, const PublicKey* pk,
                                       const DbfvParamsPtr& params, ChaChaRng& rng) {
    const DbfvParams& dp = *params;
    const BfvParams& prm = *dp.bfv_params;
    const size_t d = dp.num_digits;
    std::vector<uint64_t> ct(d * 2 * limb_words(dp));
    std::vector<uint64_t> pkf;
    if (pk) {
        pkf = pk->pk0.data;
        pkf.insert(pkf.end(), pk->pk1.data.begin(), pk->pk1.data.end());
    }
    auto fn = sk ? (poly ? exacto_dbfv_encrypt_poly_sk : exacto_dbfv_encrypt_sk)
                 : (poly ? exacto_dbfv_encrypt_poly_pk : exacto_dbfv_encrypt_pk);
    check(fn(prm.ctx(), d, dp.base, dp.plain_modulus, src, sk ? sk->poly.data.data() : pkf.data(), prm.sigma,
             rng.key, rng.next(), ct.data(), 1));
    return make_dbfv(ct, d, 2, d, 0, params);  // degree = num_digits, mul_depth = 0 (encrypt.rs:196-201)
}
inline const uint64_t* poly_plain(const CoeffPoly& pt, const DbfvParams& dp) {
    // normalize_poly_plaintext (dbfv/encrypt.rs:120-141); the p = 2^64 error is the library's
    if (dp.plain_modulus != 0) {
        const size_t n = dp.bfv_params->ring_degree;
        if (pt.coeffs.size() != n)
            throw ExactoError(2, "dimension mismatch: expected " + std::to_string(n) + ", got " +
                                     std::to_string(pt.coeffs.size()));
        if (pt.modulus != dp.plain_modulus) throw ExactoError(3, "modulus mismatch");
    }
    return pt.coeffs.data();
}
}  // namespace detail

// dbfv_encrypt_with_rng / dbfv_encrypt_sk_with_rng (src/dbfv/encrypt.rs:27-35, 73-81)
inline DbfvCiphertext dbfv_encrypt_with_rng(uint64_t plaintext, const PublicKey& pk, const DbfvParamsPtr& params,
                                            ChaChaRng& rng) {
    return detail::dbfv_encrypt_any(&plaintext, false, nullptr, &pk, params, rng);
}
inline DbfvCiphertext dbfv_encrypt_sk_with_rng(uint64_t plaintext, const SecretKey& sk, const DbfvParamsPtr& params,
                                               ChaChaRng& rng) {
    return detail::dbfv_encrypt_any(&plaintext, false, &sk, nullptr, params, rng);
}
// dbfv_encrypt_poly_with_rng / dbfv_encrypt_poly_sk_with_rng (src/dbfv/encrypt.rs:51-60, 94-103)
inline DbfvCiphertext dbfv_encrypt_poly_with_rng(const CoeffPoly& pt, const PublicKey& pk, const DbfvParamsPtr& params,
                                                 ChaChaRng& rng) {
    return detail::dbfv_encrypt_any(detail::poly_plain(pt, *params), true, nullptr, &pk, params, rng);
}
inline DbfvCiphertext dbfv_encrypt_poly_sk_with_rng(const CoeffPoly& pt, const SecretKey& sk,
                                                    const DbfvParamsPtr& params, ChaChaRng& rng) {
    return detail::dbfv_encrypt_any(detail::poly_plain(pt, *params), true, &sk, nullptr, params, rng);
}
// the reference's names without `_with_rng` draw from the OS; here the RNG is always the caller's
inline DbfvCiphertext dbfv_encrypt_pk(uint64_t m, const PublicKey& pk, const DbfvParamsPtr& p, ChaChaRng& rng) {
    return dbfv_encrypt_with_rng(m, pk, p, rng);
}
inline DbfvCiphertext dbfv_encrypt_sk(uint64_t m, const SecretKey& sk, const DbfvParamsPtr& p, ChaChaRng& rng) {
    return dbfv_encrypt_sk_with_rng(m, sk, p, rng);
}
inline DbfvCiphertext dbfv_encrypt_poly_pk(const CoeffPoly& pt, const PublicKey& pk, const DbfvParamsPtr& p,
                                           ChaChaRng& rng) {
    return dbfv_encrypt_poly_with_rng(pt, pk, p, rng);
}
inline DbfvCiphertext dbfv_encrypt_poly_sk(const CoeffPoly& pt, const SecretKey& sk, const DbfvParamsPtr& p,
                                           ChaChaRng& rng) {
    return dbfv_encrypt_poly_sk_with_rng(pt, sk, p, rng);
}

namespace detail {
inline DbfvCiphertext dbfv_addsub(bool sub, const DbfvCiphertext& a, const DbfvCiphertext& b) {
    const DbfvParams& dp = *a.params;
    const size_t d1 = a.num_limbs(), d2 = b.num_limbs();
    const size_t p1 = d1 ? a.limbs[0].c.size() : 0, p2 = d2 ? b.limbs[0].c.size() : 0, pm = std::max(p1, p2);
    auto fa = flatten(a.limbs, p1), fb = flatten(b.limbs, p2);
    std::vector<uint64_t> out(d1 * pm * limb_words(dp));
    const uint32_t da = (uint32_t)a.mul_depth, db = (uint32_t)b.mul_depth;
    uint32_t dout = 0;
    check((sub ? exacto_dbfv_sub : exacto_dbfv_add)(dp.bfv_params->ctx(), fa.data(), d1, p1, fb.data(), d2, p2,
                                                    out.data(), 1, &da, &db, &dout));
    return make_dbfv(out, d1, pm, std::max(a.degree, b.degree), dout, a.params);  // eval.rs:27-32
}
}  // namespace detail

// dbfv_add / dbfv_sub / dbfv_neg (src/dbfv/eval.rs:11-71)
inline DbfvCiphertext dbfv_add(const DbfvCiphertext& a, const DbfvCiphertext& b) {
    return detail::dbfv_addsub(false, a, b);
}
inline DbfvCiphertext dbfv_sub(const DbfvCiphertext& a, const DbfvCiphertext& b) {
    return detail::dbfv_addsub(true, a, b);
}
inline DbfvCiphertext dbfv_neg(const DbfvCiphertext& ct) {
    const DbfvParams& dp = *ct.params;
    const size_t d = ct.num_limbs(), polys = detail::dbfv_polys(ct);
    auto f = detail::flatten(ct.limbs, polys);
    std::vector<uint64_t> out(f.size());
    detail::check(exacto_dbfv_neg(dp.bfv_params->ctx(), f.data(), d, polys, out.data(), 1));
    return detail::make_dbfv(out, d, polys, ct.degree, ct.mul_depth, ct.params);
}

// dbfv_relinearize (src/dbfv/keyswitch.rs:9-23)
inline DbfvCiphertext dbfv_relinearize(const DbfvCiphertext& ct, const RelinKey& rlk) {
    const DbfvParams& dp = *ct.params;
    const size_t d = ct.num_limbs(), polys = detail::dbfv_polys(ct), outp = polys < 3 ? polys : 2;
    if (polys == 3) detail::load_key(rlk);
    auto f = detail::flatten(ct.limbs, polys);
    std::vector<uint64_t> out(d * outp * detail::limb_words(dp));
    detail::check(exacto_dbfv_relinearize(dp.bfv_params->ctx(), f.data(), d, polys, out.data(), 1));
    return detail::make_dbfv(out, d, outp, ct.degree, ct.mul_depth, ct.params);
}

// dbfv_apply_automorphism (src/dbfv/advanced.rs:15-29)
inline DbfvCiphertext dbfv_apply_automorphism(const DbfvCiphertext& ct, const GaloisKey& gk) {
    const DbfvParams& dp = *ct.params;
    const size_t d = ct.num_limbs(), polys = detail::dbfv_polys(ct);
    if (polys != 2) throw ExactoError(1, "invalid parameter: automorphism requires degree-1 ciphertext");
    auto f = detail::flatten(ct.limbs, polys);
    std::vector<uint64_t> key;
    for (auto& k : gk.keys) {
        key.insert(key.end(), k.first.data.begin(), k.first.data.end());
        key.insert(key.end(), k.second.data.begin(), k.second.data.end());
    }
    std::vector<uint64_t> out(f.size());
    detail::check(exacto_dbfv_apply_automorphism(dp.bfv_params->ctx(), f.data(), d, polys, gk.element,
                                                 key.empty() ? nullptr : key.data(), gk.keys.size(), out.data(), 1));
    return detail::make_dbfv(out, d, 2, ct.degree, ct.mul_depth, ct.params);
}

// ---- slot-packed dBFV (exacto_dbfv_batch_*, no reference function): n integers mod p per ciphertext, limb k
// carrying the slot encoding of the k-th digits; plain_modulus = 0 (2^64) is allowed.  Needs a batching prime t.
// A dBFV plaintext of the slot form: d polynomials mod t.
using DbfvSlotPlain = std::vector<CoeffPoly>;

inline DbfvSlotPlain dbfv_batch_encode(const SlotVector& values, const DbfvParamsPtr& params) {
    const DbfvParams& dp = *params;
    const BfvParams& prm = *dp.bfv_params;
    const size_t n = prm.ring_degree, d = dp.num_digits;
    if (values.size() != n)
        throw ExactoError(2, "dimension mismatch: expected " + std::to_string(n) + ", got " + std::to_string(values.size()));
    std::vector<uint64_t> out(d * n);
    detail::check(exacto_dbfv_batch_encode(prm.ctx(), d, dp.base, dp.plain_modulus, values.data(), out.data(), 1));
    DbfvSlotPlain res(d);
    for (size_t k = 0; k < d; ++k) {
        res[k].coeffs.assign(out.begin() + (long)(k * n), out.begin() + (long)((k + 1) * n));
        res[k].modulus = prm.plain_modulus;
    }
    return res;
}
inline SlotVector dbfv_batch_decode(const DbfvSlotPlain& pt, const DbfvParamsPtr& params) {
    const DbfvParams& dp = *params;
    const BfvParams& prm = *dp.bfv_params;
    const size_t n = prm.ring_degree, d = dp.num_digits;
    if (pt.size() != d) throw ExactoError(1, "invalid parameter: expected d digit plaintexts");
    std::vector<uint64_t> flat;
    for (auto& p : pt) {
        if (p.coeffs.size() != n)
            throw ExactoError(2, "dimension mismatch: expected " + std::to_string(n) + ", got " +
                                     std::to_string(p.coeffs.size()));
        flat.insert(flat.end(), p.coeffs.begin(), p.coeffs.end());
    }
    SlotVector out(n);
    detail::check(exacto_dbfv_batch_decode(prm.ctx(), d, dp.base, dp.plain_modulus, flat.data(), out.data(), 1));
    return out;
}
namespace detail {
inline DbfvCiphertext dbfv_batch_encrypt_any(const SlotVector& values, const SecretKey* sk, const PublicKey* pk,
                                             const DbfvParamsPtr& params, ChaChaRng& rng) {
    const DbfvParams& dp = *params;
    const BfvParams& prm = *dp.bfv_params;
    const size_t d = dp.num_digits;
    if (values.size() != prm.ring_degree)
        throw ExactoError(2, "dimension mismatch: expected " + std::to_string(prm.ring_degree) + ", got " +
                                 std::to_string(values.size()));
    std::vector<uint64_t> ct(d * 2 * limb_words(dp));
    std::vector<uint64_t> pkf;
    if (pk) {
        pkf = pk->pk0.data;
        pkf.insert(pkf.end(), pk->pk1.data.begin(), pk->pk1.data.end());
    }
    check((sk ? exacto_dbfv_batch_encrypt_sk : exacto_dbfv_batch_encrypt_pk)(
        prm.ctx(), d, dp.base, dp.plain_modulus, values.data(), sk ? sk->poly.data.data() : pkf.data(), prm.sigma,
        rng.key, rng.next(), ct.data(), 1));
    return make_dbfv(ct, d, 2, d, 0, params);
}
}  // namespace detail
inline DbfvCiphertext dbfv_batch_encrypt_sk(const SlotVector& values, const SecretKey& sk, const DbfvParamsPtr& params,
                                            ChaChaRng& rng) {
    return detail::dbfv_batch_encrypt_any(values, &sk, nullptr, params, rng);
}
inline DbfvCiphertext dbfv_batch_encrypt_pk(const SlotVector& values, const PublicKey& pk, const DbfvParamsPtr& params,
                                            ChaChaRng& rng) {
    return detail::dbfv_batch_encrypt_any(values, nullptr, &pk, params, rng);
}
inline SlotVector dbfv_batch_decrypt(const DbfvCiphertext& ct, const SecretKey& sk) {
    const DbfvParams& dp = *ct.params;
    auto flat = detail::flatten_dbfv(ct);
    SlotVector out(dp.bfv_params->ring_degree);
    detail::check(exacto_dbfv_batch_decrypt(dp.bfv_params->ctx(), dp.num_digits, dp.base, dp.plain_modulus, flat.data(),
                                            sk.poly.data.data(), out.data(), 1));
    return out;
}
// Both rows of the wide slots left by `steps` (gk: the key of galois_element_rotate_rows(n, steps)) / exchanged
// (gk: the key of galois_element_swap_rows(n)): dbfv_apply_automorphism with that element.
inline DbfvCiphertext dbfv_rotate_rows(const DbfvCiphertext& ct, int64_t steps, const GaloisKey& gk) {
    if (gk.element != galois_element_rotate_rows(ct.params->bfv_params->ring_degree, steps))
        throw ExactoError(1, "invalid parameter: the Galois key is not that of this rotation");
    return dbfv_apply_automorphism(ct, gk);
}
inline DbfvCiphertext dbfv_swap_rows(const DbfvCiphertext& ct, const GaloisKey& gk) {
    if (gk.element != galois_element_swap_rows(ct.params->bfv_params->ring_degree))
        throw ExactoError(1, "invalid parameter: the Galois key is not that of the row swap");
    return dbfv_apply_automorphism(ct, gk);
}

// ---- dBFV plaintext products (exacto_dbfv_plain_*, no reference function): a public digit vector (d plaintext
// polynomials, e.g. dbfv_batch_encode's) applied to dBFV ciphertexts: bfv_plain_mul per digit pair, bfv_add by
// i + j and over the terms, reduce, in one kernel.  A product raises mul_depth as dbfv_mul does.
namespace detail {
inline void append_plain(std::vector<uint64_t>& flat, const DbfvSlotPlain& pt, const DbfvParams& dp) {
    const size_t n = dp.bfv_params->ring_degree;
    if (pt.size() != dp.num_digits) throw ExactoError(1, "invalid parameter: expected d digit plaintexts");
    for (auto& p : pt) {
        if (p.coeffs.size() != n)
            throw ExactoError(2, "dimension mismatch: expected " + std::to_string(n) + ", got " +
                                     std::to_string(p.coeffs.size()));
        flat.insert(flat.end(), p.coeffs.begin(), p.coeffs.end());
    }
}
}  // namespace detail
// sum_k pts[k] * cts[k]
inline DbfvCiphertext dbfv_plain_mul_sum(const std::vector<DbfvCiphertext>& cts, const std::vector<DbfvSlotPlain>& pts) {
    if (cts.empty() || cts.size() != pts.size()) throw ExactoError(1, "invalid parameter: mismatched ct/pt lengths");
    const DbfvParams& dp = *cts[0].params;
    const size_t d = dp.num_digits, polys = detail::dbfv_polys(cts[0]);
    std::vector<uint64_t> fc, fp;
    std::vector<uint32_t> depth;
    for (size_t k = 0; k < cts.size(); ++k) {
        if (cts[k].num_limbs() != d) throw ExactoError(1, "invalid parameter: multiplication requires d-limb ciphertexts");
        auto x = detail::flatten(cts[k].limbs, polys);
        fc.insert(fc.end(), x.begin(), x.end());
        detail::append_plain(fp, pts[k], dp);
        depth.push_back((uint32_t)cts[k].mul_depth);
    }
    std::vector<uint64_t> out(d * polys * detail::limb_words(dp));
    uint32_t dout = 0;
    detail::check(exacto_dbfv_plain_mul_sum(dp.bfv_params->ctx(), d, dp.base, dp.plain_modulus, fc.data(), cts.size(),
                                            polys, fp.data(), 1, out.data(), 1, depth.data(), &dout));
    return detail::make_dbfv(out, d, polys, d, dout, cts[0].params);
}
inline DbfvCiphertext dbfv_plain_mul(const DbfvCiphertext& ct, const DbfvSlotPlain& pt) {
    return dbfv_plain_mul_sum(std::vector<DbfvCiphertext>{ct}, std::vector<DbfvSlotPlain>{pt});
}
namespace detail {
inline DbfvCiphertext dbfv_plain_addsub(bool sub, const DbfvCiphertext& ct, const DbfvSlotPlain& pt) {
    const DbfvParams& dp = *ct.params;
    const size_t d = ct.num_limbs(), polys = dbfv_polys(ct);
    if (d != dp.num_digits) throw ExactoError(1, "invalid parameter: expected d-limb dBFV ciphertext");
    auto f = flatten(ct.limbs, polys);
    std::vector<uint64_t> fp, out(f.size());
    append_plain(fp, pt, dp);
    check((sub ? exacto_dbfv_plain_sub : exacto_dbfv_plain_add)(dp.bfv_params->ctx(), d, f.data(), polys, fp.data(), 1,
                                                                 out.data(), 1));
    return make_dbfv(out, d, polys, ct.degree, ct.mul_depth, ct.params);
}
}  // namespace detail
inline DbfvCiphertext dbfv_plain_add(const DbfvCiphertext& ct, const DbfvSlotPlain& pt) {
    return detail::dbfv_plain_addsub(false, ct, pt);
}
inline DbfvCiphertext dbfv_plain_sub(const DbfvCiphertext& ct, const DbfvSlotPlain& pt) {
    return detail::dbfv_plain_addsub(true, ct, pt);
}
// Slot-wise ct * values mod p: dbfv_batch_encode, then dbfv_plain_mul.
inline DbfvCiphertext dbfv_batch_plain_mul(const DbfvCiphertext& ct, const SlotVector& values) {
    return dbfv_plain_mul(ct, dbfv_batch_encode(values, ct.params));
}

// ---- dBFV hoisted rotations and slot linear transforms with wide public diagonals (exacto_dbfv_linear_transform*,
// no reference function): reduce(sum_r W_r * rot_r(x)), bit for bit dbfv_plain_mul_sum over the rotations
// bfv_rotate_hoisted makes of the limbs.
// out[r] = the set's automorphism r of ct, limb by limb on the shared gadget digits of each limb's c1
inline std::vector<DbfvCiphertext> dbfv_rotate_hoisted(const DbfvCiphertext& ct, const GaloisKeySet& ks) {
    const DbfvParams& dp = *ct.params;
    const size_t d = ct.num_limbs(), R = ks.size(), per = d * 2 * detail::limb_words(dp);
    if (detail::dbfv_polys(ct) != 2) throw ExactoError(EXACTO_ERR_INVALID_PARAM, "invalid parameter: automorphism requires degree-1 ciphertext");
    auto flat = detail::flatten_dbfv(ct);
    std::vector<uint64_t> out(R * per);
    detail::check(exacto_dbfv_rotate_hoisted(dp.bfv_params->ctx(), ks.handle(), d, flat.data(), out.data(), 1));
    std::vector<DbfvCiphertext> res;
    for (size_t r = 0; r < R; ++r) {
        std::vector<uint64_t> one(out.begin() + (long)(r * per), out.begin() + (long)((r + 1) * per));
        res.push_back(detail::make_dbfv(one, d, 2, ct.degree, ct.mul_depth, ct.params));
    }
    return res;
}
// Both rows of the wide slots left by every steps[r] at once; ks holds the elements
// galois_element_rotate_rows(n, steps[r]) in this order
inline std::vector<DbfvCiphertext> dbfv_rotate_rows_many(const DbfvCiphertext& ct, const std::vector<int64_t>& steps,
                                                         const GaloisKeySet& ks) {
    const size_t n = ct.params->bfv_params->ring_degree;
    bool same = steps.size() == ks.size();
    for (size_t r = 0; same && r < steps.size(); ++r)
        same = ks.elements()[r] % (2 * n) == galois_element_rotate_rows(n, steps[r]);
    if (!same) throw ExactoError(1, "invalid parameter: the key set does not hold the elements of these steps in this order");
    return dbfv_rotate_hoisted(ct, ks);
}

// Wide public diagonals lifted once (exacto_dbfv_diagonals_create): one DbfvSlotPlain per element of the key
// set they will be used with.  Keeps its parameters (and with them the context) alive.
class DbfvDiagonals {
public:
    DbfvDiagonals(const DbfvParamsPtr& params, const std::vector<DbfvSlotPlain>& pts) : params_(params), R_(pts.size()) {
        std::vector<uint64_t> flat;
        for (auto& p : pts) detail::append_plain(flat, p, *params);
        detail::check(exacto_dbfv_diagonals_create(params->bfv_params->ctx(), params->num_digits, pts.size(),
                                                   flat.empty() ? nullptr : flat.data(), &h_));
    }
    DbfvDiagonals(const DbfvDiagonals&) = delete;
    DbfvDiagonals& operator=(const DbfvDiagonals&) = delete;
    DbfvDiagonals(DbfvDiagonals&& o) noexcept : params_(std::move(o.params_)), R_(o.R_), h_(o.h_) { o.h_ = nullptr; }
    ~DbfvDiagonals() { exacto_dbfv_diagonals_destroy(h_); }
    const exacto_dbfv_diagonals* handle() const { return h_; }
    size_t size() const { return R_; }
    const DbfvParamsPtr& params() const { return params_; }
    // the route a transform takes on this context: the fused kernel, or rotations staged for the product kernel
    bool fused() const {
        int f = 0;
        detail::check(exacto_dbfv_diagonals_info(h_, nullptr, nullptr, &f));
        return f != 0;
    }

private:
    DbfvParamsPtr params_;
    size_t R_ = 0;
    exacto_dbfv_diagonals* h_ = nullptr;
};

// reduce(sum_r pts[r] * (automorphism r of ct)): raw diagonals (lifted on every call) or prepared ones
inline DbfvCiphertext dbfv_linear_transform(const DbfvCiphertext& ct, const GaloisKeySet& ks,
                                            const std::vector<DbfvSlotPlain>& pts) {
    const DbfvParams& dp = *ct.params;
    const size_t d = dp.num_digits;
    if (ct.num_limbs() != d) throw ExactoError(1, "invalid parameter: multiplication requires d-limb ciphertexts");
    if (detail::dbfv_polys(ct) != 2) throw ExactoError(EXACTO_ERR_INVALID_PARAM, "invalid parameter: automorphism requires degree-1 ciphertext");
    if (pts.size() != ks.size()) throw ExactoError(EXACTO_ERR_INVALID_PARAM, "invalid parameter: one plaintext per element of the key set");
    auto flat = detail::flatten_dbfv(ct);
    std::vector<uint64_t> fp, out(flat.size());
    for (auto& p : pts) detail::append_plain(fp, p, dp);
    const uint32_t depth = (uint32_t)ct.mul_depth;
    uint32_t dout = 0;
    detail::check(exacto_dbfv_linear_transform(dp.bfv_params->ctx(), ks.handle(), d, dp.base, dp.plain_modulus,
                                               flat.data(), fp.data(), out.data(), 1, &depth, &dout));
    return detail::make_dbfv(out, d, 2, d, dout, ct.params);
}
inline DbfvCiphertext dbfv_linear_transform(const DbfvCiphertext& ct, const GaloisKeySet& ks, const DbfvDiagonals& dg) {
    const DbfvParams& dp = *ct.params;
    const size_t d = dp.num_digits;
    if (ct.num_limbs() != d) throw ExactoError(1, "invalid parameter: multiplication requires d-limb ciphertexts");
    if (detail::dbfv_polys(ct) != 2) throw ExactoError(EXACTO_ERR_INVALID_PARAM, "invalid parameter: automorphism requires degree-1 ciphertext");
    auto flat = detail::flatten_dbfv(ct);
    std::vector<uint64_t> out(flat.size());
    const uint32_t depth = (uint32_t)ct.mul_depth;
    uint32_t dout = 0;
    detail::check(exacto_dbfv_linear_transform_prepared(dp.bfv_params->ctx(), ks.handle(), d, dp.base, dp.plain_modulus,
                                                        flat.data(), dg.handle(), out.data(), 1, &depth, &dout));
    return detail::make_dbfv(out, d, 2, d, dout, ct.params);
}

// dbfv_div_by_base (src/dbfv/advanced.rs:36-93): the result carries new DbfvParams with p / base.
inline DbfvCiphertext dbfv_div_by_base(const DbfvCiphertext& ct) {
    const DbfvParams& dp = *ct.params;
    auto f = detail::flatten_dbfv(ct);
    std::vector<uint64_t> out(f.size());
    uint64_t new_plain = 0;
    detail::check(exacto_dbfv_div_by_base(dp.bfv_params->ctx(), dp.num_digits, dp.base, dp.plain_modulus, f.data(),
                                          out.data(), 1, &new_plain));
    auto np = std::make_shared<DbfvParams>(DbfvParams{dp.bfv_params, dp.base, dp.num_digits, new_plain});
    const size_t degree = std::max<size_t>(ct.degree ? ct.degree - 1 : 0, 1);  // saturating_sub(1).max(1)
    return detail::make_dbfv(out, dp.num_digits, 2, degree, ct.mul_depth, np);
}

// dbfv_change_base (src/dbfv/advanced.rs:99-160): new DbfvParams (new_base, new_num_digits, p).
inline DbfvCiphertext dbfv_change_base(const DbfvCiphertext& ct, uint64_t new_base, size_t new_num_digits) {
    const DbfvParams& dp = *ct.params;
    auto f = detail::flatten_dbfv(ct);
    std::vector<uint64_t> out(std::max<size_t>(new_num_digits, 1) * 2 * detail::limb_words(dp));
    detail::check(exacto_dbfv_change_base(dp.bfv_params->ctx(), dp.num_digits, dp.base, dp.plain_modulus, new_base,
                                          new_num_digits, f.data(), out.data(), 1));
    auto np = std::make_shared<DbfvParams>(DbfvParams{dp.bfv_params, new_base, new_num_digits, dp.plain_modulus});
    return detail::make_dbfv(out, new_num_digits, 2, new_num_digits, ct.mul_depth, np);
}

// The benchmark chain of src/bin/paper_repro.rs:203-236: x * y^depth with mul_depth reset before
// every dbfv_mul (guard bypass), run device-resident in one call.
inline DbfvCiphertext dbfv_mul_chain(const DbfvCiphertext& x, const DbfvCiphertext& y, const RelinKey& rlk,
                                     size_t depth) {
    const auto& dp = *x.params;
    detail::load_key(rlk);
    auto fx = detail::flatten_dbfv(x), fy = detail::flatten_dbfv(y);
    std::vector<uint64_t> out(fx.size());
    detail::check(exacto_dbfv_mul_chain(dp.bfv_params->ctx(), dp.num_digits, dp.base, dp.plain_modulus, fx.data(),
                                        fy.data(), out.data(), 1, depth));
    DbfvCiphertext res;
    res.limbs = detail::unflatten(out, dp.num_digits, 2, dp.bfv_params);
    res.degree = dp.num_digits;
    res.mul_depth = depth ? 1 : x.mul_depth;
    res.params = x.params;
    return res;
}


// One GPU's share of a dbfv_mul split by output limb (dbfv/eval.rs:109-132): the limbs `limbs` of each
// product a[i] * b[i] (mul_depth 0 inputs), as BfvCiphertexts [item][slot] (exacto_dbfv_mul_limbs).
inline std::vector<std::vector<BfvCiphertext>> dbfv_mul_limbs(const std::vector<DbfvCiphertext>& a,
                                                             const std::vector<DbfvCiphertext>& b,
                                                             const RelinKey& rlk, const std::vector<uint32_t>& limbs) {
    if (a.empty()) return {};
    const auto& dp = *a[0].params;
    detail::load_key(rlk);
    std::vector<uint64_t> fa, fb;
    for (size_t i = 0; i < a.size(); ++i) {
        auto x = detail::flatten_dbfv(a[i]), y = detail::flatten_dbfv(b[i]);
        fa.insert(fa.end(), x.begin(), x.end());
        fb.insert(fb.end(), y.begin(), y.end());
    }
    const size_t per = 2 * dp.bfv_params->num_limbs() * dp.bfv_params->ring_degree;
    std::vector<uint64_t> out(a.size() * limbs.size() * per);
    detail::check(exacto_dbfv_mul_limbs(dp.bfv_params->ctx(), dp.num_digits, dp.base, dp.plain_modulus, fa.data(),
                                        fb.data(), out.data(), a.size(), limbs.data(), limbs.size()));
    std::vector<std::vector<BfvCiphertext>> res(a.size());
    for (size_t i = 0; i < a.size(); ++i)
        res[i] = detail::unflatten(std::vector<uint64_t>(out.begin() + (long)(i * limbs.size() * per),
                                                         out.begin() + (long)((i + 1) * limbs.size() * per)),
                                   limbs.size(), 2, dp.bfv_params);
    return res;
}

// ---- RCCL over xGMI (exacto_hip.h): one communicator per GPU, keys broadcast from one root
class RcclComm {
  public:
    // ncclGetUniqueId on the root; every rank passes the same 128 bytes
    static std::vector<uint8_t> unique_id() {
        std::vector<uint8_t> id(128);
        detail::check(exacto_rccl_unique_id(id.data()));
        return id;
    }
    RcclComm(int nranks, const std::vector<uint8_t>& id, int rank, int device) {
        detail::check(exacto_rccl_comm_init(&h_, nranks, id.data(), rank, device));
    }
    ~RcclComm() { exacto_rccl_comm_destroy(h_); }
    RcclComm(const RcclComm&) = delete;
    RcclComm& operator=(const RcclComm&) = delete;
    void* handle() const { return h_; }

  private:
    void* h_ = nullptr;
};

// The root's relinearisation key (loaded with load_relin_key / generated on its device) becomes the
// resident key of every rank's context (ncclBroadcast in place): keys are made once, keygen.rs:123-162.
inline void broadcast_relin_key(const BfvParams& prm, const RcclComm& comm, int root, size_t num_keys) {
    detail::check(exacto_ctx_broadcast_relin_key(prm.ctx(), comm.handle(), root, num_keys));
    prm.loaded_key = nullptr;   // resident contents now come from the root
}

}  // namespace exacto
