// C++ host-API test of modulus switching (include/exacto.hpp: mod_switch, mod_switch_drop_prime,
// lower_secret_key) at cfg3's primes, n = 1024: encrypt -> (multiply) -> mod_switch -> decrypt and noise
// under the lower parameters; the reference-mode function keeps the params and has L - 1 limbs; the
// ModulusMismatch and InvalidParam cases.  Run with the argument "host" it checks only the level
// predicate, which needs no device.  Prints "PASS <name>" per step and "ALL OK" at the end.
#include <cstdio>
#include <iostream>
#include <memory>
#include <string>
#include <vector>

#include "exacto.hpp"

using namespace exacto;

static int failures = 0;

static void expect(bool ok, const std::string& name) {
    std::cout << (ok ? "PASS " : "FAIL ") << name << "\n";
    if (!ok) ++failures;
}

static const std::vector<uint64_t> Q3 = {1152921504606830593ull, 1152921504606748673ull, 1152921504606683137ull};

template <class F>
static bool throws(F f, const char* variant, const std::string& text) {
    try {
        f();
    } catch (const ExactoError& e) {
        return std::string(e.variant()) == variant && std::string(e.what()).find(text) != std::string::npos;
    }
    return false;
}

static void host_helpers() {
    // is_lower_level reads the plain fields only: parameter objects without a device context
    auto plain = [](size_t n, uint64_t p, std::vector<uint64_t> m) {
        auto prm = std::make_shared<BfvParams>();
        prm->ring_degree = n;
        prm->plain_modulus = p;
        prm->ct_moduli = std::move(m);
        return prm;
    };
    auto top = plain(1024, 65537, Q3);
    expect(detail::is_lower_level(*top, *plain(1024, 65537, {Q3[0], Q3[1]})) &&
               detail::is_lower_level(*top, *plain(1024, 65537, {Q3[0]})),
           "a proper prefix is a lower level");
    expect(!detail::is_lower_level(*top, *top) && !detail::is_lower_level(*top, *plain(1024, 65537, {})) &&
               !detail::is_lower_level(*top, *plain(1024, 65537, {Q3[1]})) &&
               !detail::is_lower_level(*top, *plain(1024, 65537, {Q3[0], Q3[2]})) &&
               !detail::is_lower_level(*top, *plain(2048, 65537, {Q3[0]})) &&
               !detail::is_lower_level(*top, *plain(1024, 257, {Q3[0]})) &&
               !detail::is_lower_level(*plain(1024, 65537, {Q3[0]}), *top),
           "the same level, no prime, another prime, another n or p, a higher level are not");
    expect(EXACTO_MODSWITCH_ROUND == 0 && EXACTO_MODSWITCH_REFERENCE == 1, "mode values");
}

// A ternary secret (coefficients -1, 0, 1 reduced per prime: small mod Q, which the noise bound of a drop
// assumes; gen_secret_key_with_rng samples as the reference does, where a "-1" is q_0 - 1 in every limb).
static SecretKey ternary_key(const BfvParamsPtr& prm, uint64_t seed) {
    const size_t n = prm->ring_degree, L = prm->num_limbs();
    std::vector<uint64_t> s(L * n);
    uint64_t z = seed;
    for (size_t j = 0; j < n; ++j) {
        z = z * 6364136223846793005ull + 1442695040888963407ull;
        const int v = (int)((z >> 33) % 3) - 1;
        for (size_t i = 0; i < L; ++i) s[i * n + j] = v < 0 ? prm->ct_moduli[i] - 1 : (uint64_t)v;
    }
    for (size_t i = 0; i < L; ++i) detail::check(exacto_ntt_fwd(prm->ctx(), s.data() + i * n, 1, i));
    return SecretKey{detail::make_poly(*prm, s.data()), prm};
}

// floor(noise / q) for a noise below 2^128
static unsigned __int128 div_q(const Noise& v, uint64_t q) {
    unsigned __int128 x = 0;
    for (size_t i = v.words.size(); i-- > 0;) {
        if (i >= 2 && v.words[i]) return ~(unsigned __int128)0;
        if (i < 2) x |= (unsigned __int128)v.words[i] << (64 * i);
    }
    return x / q;
}

int main(int argc, char** argv) {
    try {
        host_helpers();
        if (argc > 1 && std::string(argv[1]) == "host") {
            if (failures) return 1;
            std::cout << "ALL OK\n";
            return 0;
        }
        const size_t n = 1024;
        const uint64_t p = 65537;
        auto top = BfvParamsBuilder().ring_degree(n).plain_modulus(p).ct_moduli(Q3).build();
        auto mid = BfvParamsBuilder().ring_degree(n).plain_modulus(p).ct_moduli({Q3[0], Q3[1]}).build();
        auto low = BfvParamsBuilder().ring_degree(n).plain_modulus(p).ct_moduli({Q3[0]}).build();
        ChaChaRng rng(7);
        SecretKey sk = ternary_key(top, 99);
        RelinKey rlk = gen_relin_key_with_rng(sk, rng);
        SecretKey sk_mid = lower_secret_key(sk, mid), sk_low = lower_secret_key(sk, low);

        CoeffPoly m1{std::vector<uint64_t>(n, 0), p}, m2 = m1;
        for (size_t j = 0; j < n; ++j) m1.coeffs[j] = (j * 2654435761ull) % p;
        m2.coeffs[0] = 3;
        BfvCiphertext a = encrypt_sk_with_rng(m1, sk, top, rng), b = encrypt_sk_with_rng(m2, sk, top, rng);

        BfvCiphertext a_mid = mod_switch(a, mid);
        expect(a_mid.params == mid && a_mid.c.size() == 2 && a_mid.c[0].num_limbs == 2 &&
                   a_mid.c[0].data.size() == 2 * n,
               "mod_switch carries the lower params and has their limbs");
        expect(decrypt(a_mid, sk_mid).coeffs == m1.coeffs, "a fresh encryption decrypts one level down");
        BfvCiphertext a_low = mod_switch(a, low);
        expect(a_low.c[0].num_limbs == 1 && decrypt(a_low, sk_low).coeffs == m1.coeffs,
               "... and two levels down in one call");
        expect(mod_switch(a_mid, low).c[0].data == a_low.c[0].data && mod_switch(a_mid, low).c[1].data == a_low.c[1].data,
               "two drops are two single drops");

        const Noise before = bfv_noise_inf(a, sk), after = bfv_noise_inf(a_mid, sk_mid);
        std::printf("noise %zu bits -> %zu bits (budget %zu -> %zu bits)\n", before.bit_length(), after.bit_length(),
                    noise_budget_bits(before, *top), noise_budget_bits(after, *mid));
        expect(after.fits_u64() && after.to_u64() <= div_q(before, Q3[2]) + p + n / 2 + 2,
               "noise after the drop within floor(noise / q) + p + n / 2 + 2");

        BfvCiphertext prod = bfv_mul_and_relin(a, b, rlk);
        std::vector<uint64_t> want(n);
        for (size_t j = 0; j < n; ++j) want[j] = m1.coeffs[j] * 3 % p;
        BfvCiphertext prod_mid = mod_switch(prod, mid);
        expect(decrypt(prod_mid, sk_mid).coeffs == want, "a product decrypts one level down");
        const Noise pb = bfv_noise_inf(prod, sk), pa = bfv_noise_inf(prod_mid, sk_mid);
        expect(pa.fits_u64() && pa.to_u64() <= div_q(pb, Q3[2]) + p + n / 2 + 2, "the product's noise is divided by q");
        // the library's own key generator (the reference's sampling): the plaintext survives the drop too
        SecretKey skd = gen_secret_key_with_rng(top, rng);
        BfvCiphertext d_mid = mod_switch(encrypt_sk_with_rng(m1, skd, top, rng), mid);
        expect(decrypt(d_mid, lower_secret_key(skd, mid)).coeffs == m1.coeffs, "with a generated key as well");

        // degree 2: switched like any other
        BfvCiphertext t = bfv_mul_no_relin(a, b);
        BfvCiphertext t_mid = mod_switch(t, mid);
        expect(t_mid.c.size() == 3 && decrypt(t_mid, sk_mid).coeffs == want, "a degree-2 ciphertext is switched too");

        // the reference's function: same params, L - 1 limbs, not a ciphertext of the smaller modulus
        BfvCiphertext r = mod_switch_drop_prime(a);
        expect(r.params == top && r.c.size() == 2 && r.c[0].num_limbs == 2 && r.c[0].data.size() == 2 * n,
               "mod_switch_drop_prime keeps the params and drops one limb");
        expect(r.c[0].data != a_mid.c[0].data, "... and is not the exact switch");
        BfvCiphertext r2 = mod_switch_drop_prime(r);
        expect(r2.c[0].num_limbs == 1, "... applied twice");
        expect(throws([&] { (void)mod_switch_drop_prime(r2); }, "InvalidParam",
                      "cannot drop prime: only one modulus remaining"),
               "one limb left: the reference's InvalidParam");

        auto other_p = BfvParamsBuilder().ring_degree(n).plain_modulus(257).ct_moduli({Q3[0], Q3[1]}).build();
        auto other_q = BfvParamsBuilder().ring_degree(n).plain_modulus(p).ct_moduli({Q3[1], Q3[0]}).build();
        auto other_n = BfvParamsBuilder().ring_degree(2 * n).plain_modulus(p).ct_moduli({Q3[0], Q3[1]}).build();
        expect(throws([&] { (void)mod_switch(a, top); }, "ModulusMismatch", "modulus mismatch") &&
                   throws([&] { (void)mod_switch(a, other_p); }, "ModulusMismatch", "modulus mismatch") &&
                   throws([&] { (void)mod_switch(a, other_q); }, "ModulusMismatch", "modulus mismatch") &&
                   throws([&] { (void)mod_switch(a, other_n); }, "ModulusMismatch", "modulus mismatch") &&
                   throws([&] { (void)mod_switch(a_mid, top); }, "ModulusMismatch", "modulus mismatch") &&
                   throws([&] { (void)mod_switch(a, nullptr); }, "ModulusMismatch", "modulus mismatch"),
               "anything but a proper prefix with equal n and p: ModulusMismatch");
    } catch (const std::exception& e) {
        std::cout << "FAIL exception: " << e.what() << "\n";
        return 1;
    }
    if (failures) return 1;
    std::cout << "ALL OK\n";
    return 0;
}
