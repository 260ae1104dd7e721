// C++ host-API test of bfv_mul_sum (include/exacto.hpp): sums of ciphertext products with one key switch
// per sum, at compact_bfv (presets.rs:24-35): keygen -> encrypt three pairs of scalars -> bfv_mul_sum ->
// decrypt, checking sum_k x_k y_k mod t and a second output slot with a single product.  Run with the
// argument "host" it only checks that the header's declarations are usable (no device needed).
// Prints "PASS <name>" per step and "ALL OK" at the end.
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

int main(int argc, char** argv) {
    try {
        const std::vector<MulSumTerm> terms = {{0, 0, 0}, {1, 1, 0}, {2, 2, 0}, {0, 2, 1}};
        expect(terms.size() == 4 && terms[3].ia == 0 && terms[3].ib == 2 && terms[3].slot == 1, "MulSumTerm");
        if (argc > 1 && std::string(argv[1]) == "host") {
            if (failures) return 1;
            std::cout << "ALL OK\n";
            return 0;
        }
        auto prm = BfvParamsBuilder().ring_degree(1024).plain_modulus(257).ct_moduli({1099509805057ull})
                       .aux_moduli({562949953443841ull}).sigma(3.2).build();
        ChaChaRng rng(7);
        const SecretKey sk = gen_secret_key_with_rng(prm, rng);
        const RelinKey rlk = gen_relin_key_with_rng(sk, rng);
        const uint64_t x[3] = {3, 5, 200}, y[3] = {11, 13, 2}, t = prm->plain_modulus;
        std::vector<BfvCiphertext> a, b;
        for (int k = 0; k < 3; ++k) {
            a.push_back(encrypt_sk_with_rng(encode_scalar(x[k], prm), sk, prm, rng));
            b.push_back(encrypt_sk_with_rng(encode_scalar(y[k], prm), sk, prm, rng));
        }
        const std::vector<BfvCiphertext> out = bfv_mul_sum(a, b, terms, 2, rlk);
        expect(out.size() == 2 && out[0].c.size() == 2, "two degree-1 outputs");
        const uint64_t dot = (x[0] * y[0] + x[1] * y[1] + x[2] * y[2]) % t;
        expect(decode_scalar(decrypt(out[0], sk)) == dot, "dot product decrypts to sum x_k y_k mod t");
        expect(decode_scalar(decrypt(out[1], sk)) == (x[0] * y[2]) % t, "single-product slot");
        // the composition it replaces, bit for bit
        BfvCiphertext want = bfv_mul_and_relin(a[0], b[0], rlk);
        for (int k = 1; k < 3; ++k) want = bfv_add(want, bfv_mul_and_relin(a[k], b[k], rlk));
        expect(want.c[0].data == out[0].c[0].data && want.c[1].data == out[0].c[1].data,
               "equals bfv_mul_and_relin + bfv_add bit for bit");
        // sum of squares: both operands the same vector
        const std::vector<BfvCiphertext> sq = bfv_mul_sum(a, a, {{0, 0, 0}, {1, 1, 0}, {2, 2, 0}}, 1, rlk);
        expect(decode_scalar(decrypt(sq[0], sk)) == (x[0] * x[0] + x[1] * x[1] + x[2] * x[2]) % t, "sum of squares");
        bool threw = false;
        try {
            (void)bfv_mul_sum(a, b, {{0, 3, 0}}, 1, rlk);
        } catch (const ExactoError& e) {
            threw = std::string(e.variant()) == "InvalidParam" && std::string(e.what()).find("nb = 3") != std::string::npos;
        }
        expect(threw, "index out of range is InvalidParam");
    } catch (const std::exception& e) {
        std::cout << "FAIL exception: " << e.what() << "\n";
        return 1;
    }
    if (failures) return 1;
    std::cout << "ALL OK\n";
    return 0;
}
