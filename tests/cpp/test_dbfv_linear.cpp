// C++ host-API test of the dBFV surface beyond the product (include/exacto.hpp), following the
// reference's own tests (src/dbfv/advanced.rs:183-221, src/dbfv/encrypt.rs:240-273) at compact_dbfv:
// keygen -> encrypt -> change_base -> div_by_base -> decrypt, checking the values, degree, mul_depth
// and the DbfvParams every step returns.  Prints "PASS <name>" per step and "ALL OK" at the end.
#include <cstdio>
#include <iostream>
#include <string>
#include <vector>

#include "exacto.hpp"

using namespace exacto;

static int failures = 0;

static void expect(bool ok, const std::string& name) {
    std::cout << (ok ? "PASS " : "FAIL ") << name << "\n";
    if (!ok) ++failures;
}

template <class F>
static void expect_error(F f, const char* variant, const std::string& text, const std::string& name) {
    try {
        f();
        expect(false, name + " (no error)");
    } catch (const ExactoError& e) {
        expect(std::string(e.variant()) == variant && std::string(e.what()).find(text) != std::string::npos,
               name + " [" + e.what() + "]");
    }
}

int main() {
    try {
        // presets.rs:86-98 compact_dbfv
        auto bfv = BfvParamsBuilder().ring_degree(1024).plain_modulus(929).ct_moduli({1099509805057ull})
                       .aux_moduli({562949953443841ull}).sigma(3.2).build();
        DbfvParamsPtr params = std::make_shared<DbfvParams>(DbfvParams{bfv, 16, 2, 256});
        ChaChaRng rng(42);
        DbfvKeys keys = dbfv_keygen_full(params, {3}, rng);
        expect(keys.gks.size() == 1 && keys.gks[0].element == 3 && keys.rlk.keys.size() == bfv->gadget_digits,
               "dbfv_keygen_full");

        // encrypt -> decrypt, secret and public key
        DbfvCiphertext ct = dbfv_encrypt_sk(48, keys.sk, params, rng);
        expect(ct.num_limbs() == 2 && ct.degree == 2 && ct.mul_depth == 0 && dbfv_decrypt(ct, keys.sk) == 48,
               "dbfv_encrypt_sk");
        expect(dbfv_decrypt(dbfv_encrypt_pk(300, keys.pk, params, rng), keys.sk) == 300 % 256, "dbfv_encrypt_pk");
        CoeffPoly pt;
        pt.modulus = 256;
        pt.coeffs.assign(1024, 0);
        pt.coeffs[0] = 42;
        pt.coeffs[1] = 100;
        pt.coeffs[2] = 255;
        CoeffPoly back = dbfv_decrypt_poly(dbfv_encrypt_poly_sk(pt, keys.sk, params, rng), keys.sk);
        expect(back.coeffs == pt.coeffs, "dbfv_encrypt_poly_sk");
        back = dbfv_decrypt_poly(dbfv_encrypt_poly_pk(pt, keys.pk, params, rng), keys.sk);
        expect(back.coeffs == pt.coeffs, "dbfv_encrypt_poly_pk");

        // change_base: (16, 2) -> (4, 4), values and the returned DbfvParams
        DbfvCiphertext b4 = dbfv_change_base(ct, 4, 4);
        expect(b4.num_limbs() == 4 && b4.degree == 4 && b4.mul_depth == 0 && b4.params->base == 4 &&
                   b4.params->num_digits == 4 && b4.params->plain_modulus == 256 &&
                   b4.params->bfv_params.get() == bfv.get(),
               "dbfv_change_base params");
        expect(dbfv_decrypt(b4, keys.sk) == 48, "dbfv_change_base value");
        for (uint64_t v : {0ull, 1ull, 15ull, 42ull, 127ull, 255ull})
            expect(dbfv_decrypt(dbfv_change_base(dbfv_encrypt_sk(v, keys.sk, params, rng), 4, 4), keys.sk) == v,
                   "dbfv_change_base preserves " + std::to_string(v));

        // div_by_base on the base-4 form: 48 / 4 = 12 mod 64, then on the original: 48 / 16 = 3 mod 16
        DbfvCiphertext q4 = dbfv_div_by_base(b4);
        expect(q4.params->plain_modulus == 64 && q4.params->base == 4 && q4.params->num_digits == 4 &&
                   q4.degree == 3 && q4.num_limbs() == 4,
               "dbfv_div_by_base params (base 4)");
        expect(dbfv_decrypt(q4, keys.sk) == 12, "dbfv_div_by_base value (base 4)");
        DbfvCiphertext q16 = dbfv_div_by_base(ct);
        expect(q16.params->plain_modulus == 16 && q16.degree == 1 && dbfv_decrypt(q16, keys.sk) == 3,
               "dbfv_div_by_base (advanced.rs:196-207)");

        // add / sub / neg and the automorphism
        DbfvCiphertext a = dbfv_encrypt_sk(100, keys.sk, params, rng), b = dbfv_encrypt_sk(27, keys.sk, params, rng);
        a.mul_depth = 1;
        DbfvCiphertext s = dbfv_add(a, b);
        expect(dbfv_decrypt(s, keys.sk) == 127 && s.mul_depth == 1 && s.degree == 2, "dbfv_add");
        expect(dbfv_decrypt(dbfv_sub(a, b), keys.sk) == 73, "dbfv_sub");
        expect(dbfv_decrypt(dbfv_neg(b), keys.sk) == 256 - 27, "dbfv_neg");
        expect(dbfv_decrypt(dbfv_apply_automorphism(dbfv_encrypt_sk(42, keys.sk, params, rng), keys.gks[0]),
                            keys.sk) == 42,
               "dbfv_apply_automorphism (advanced.rs:183-194)");
        DbfvCiphertext r = dbfv_relinearize(b, keys.rlk);  // degree-1 limbs: cloned
        expect(dbfv_decrypt(r, keys.sk) == 27 && r.limbs[0].c.size() == 2, "dbfv_relinearize (clone)");

        // errors, worded as the reference words them
        expect_error([&] { dbfv_change_base(ct, 1, 4); }, "InvalidParam", "new base must be >= 2", "new base");
        expect_error([&] { dbfv_change_base(ct, 4, 0); }, "InvalidParam", "new_num_digits must be >= 1", "new digits");
        expect_error([&] { dbfv_change_base(ct, 4, 3); }, "InvalidParam", "base^digits = 64 < plain_modulus = 256",
                     "new params");
        DbfvCiphertext three = ct;
        three.limbs.push_back(ct.limbs[0]);
        expect_error([&] { dbfv_add(ct, three); }, "DimensionMismatch", "dimension mismatch: expected 2, got 3",
                     "dbfv_add limbs");
        auto odd = std::make_shared<DbfvParams>(DbfvParams{bfv, 16, 2, 250});
        DbfvCiphertext c250 = ct;
        c250.params = odd;
        expect_error([&] { dbfv_div_by_base(c250); }, "InvalidParam",
                     "plaintext modulus 250 is not divisible by base 16", "dbfv_div_by_base divisibility");
    } catch (const std::exception& e) {
        std::cout << "FAIL exception: " << e.what() << "\n";
        return 1;
    }
    if (failures) return 1;
    std::cout << "ALL OK\n";
    return 0;
}
