// C++ host-API test of SIMD batching (include/exacto.hpp): at cfg3's basis with n = 1024, keygen -> batch_encode
// (1, 2, ..., n) -> encrypt -> bfv_square_and_relin -> bfv_rotate_rows by 1 -> decrypt -> batch_decode gives
// the squares mod t with both rows rotated left by one; the composed batch_encrypt_sk / batch_decrypt agree.
// Run with the argument "host" it checks the two Galois-element helpers and that the header's declarations
// link (no device needed).  Prints "PASS <name>" per step and "ALL OK" at the end.
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

static uint64_t pow3(uint64_t e, uint64_t m) {
    uint64_t r = 1;
    for (uint64_t i = 0; i < e; ++i) r = r * 3 % m;
    return r;
}

int main(int argc, char** argv) {
    try {
        std::vector<CoeffPoly> (*f1)(const std::vector<SlotVector>&, const BfvParamsPtr&) = &batch_encode;
        std::vector<SlotVector> (*f2)(const std::vector<CoeffPoly>&, const BfvParamsPtr&) = &batch_decode;
        std::vector<BfvCiphertext> (*f3)(const std::vector<BfvCiphertext>&, int64_t, const GaloisKey*) = &bfv_rotate_rows;
        std::vector<BfvCiphertext> (*f4)(const std::vector<BfvCiphertext>&, const GaloisKey&) = &bfv_swap_rows;
        std::vector<SlotVector> (*f5)(const std::vector<BfvCiphertext>&, const SecretKey&) = &batch_decrypt;
        BfvCiphertext (*f6)(const SlotVector&, const SecretKey&, const BfvParamsPtr&, ChaChaRng&) = &batch_encrypt_sk;
        BfvCiphertext (*f7)(const SlotVector&, const PublicKey&, const BfvParamsPtr&, ChaChaRng&) = &batch_encrypt_pk;
        uint64_t (*f8)(const BfvParamsPtr&) = &batch_root;
        expect(f1 && f2 && f3 && f4 && f5 && f6 && f7 && f8, "declarations");
        expect(f3(std::vector<BfvCiphertext>{}, 1, nullptr).empty(), "empty batch");
        bool ok = true;
        for (size_t n : {16u, 64u, 4096u}) {
            const int64_t h = (int64_t)(n / 2);
            for (int64_t k : {(int64_t)0, (int64_t)1, (int64_t)-1, h, h + 3, -h - 1}) {
                const uint64_t e = (uint64_t)(((k % h) + h) % h);
                ok = ok && galois_element_rotate_rows(n, k) == pow3(e, 2 * n);
            }
            ok = ok && galois_element_swap_rows(n) == 2 * n - 1;
        }
        expect(ok, "galois_element_rotate_rows / galois_element_swap_rows");
        bool threw = false;
        try {
            (void)galois_element_rotate_rows(48, 1);
        } catch (const ExactoError& e) {
            threw = std::string(e.variant()) == "InvalidRingDegree";
        }
        expect(threw, "n = 48 is InvalidRingDegree");
        if (argc > 1 && std::string(argv[1]) == "host") {
            if (failures) return 1;
            std::cout << "ALL OK\n";
            return 0;
        }
        const size_t n = 1024;
        auto prm = BfvParamsBuilder().ring_degree(n).plain_modulus(65537)
                       .ct_moduli({1152921504606830593ull, 1152921504606748673ull, 1152921504606683137ull}).build();
        const uint64_t t = prm->plain_modulus;
        expect(batch_root(prm) != 0, "the context batches");
        ChaChaRng rng(5);
        const SecretKey sk = gen_secret_key_with_rng(prm, rng);
        const RelinKey rlk = gen_relin_key_with_rng(sk, rng);
        const GaloisKey gk = gen_galois_key_with_rng(sk, galois_element_rotate_rows(n, 1), rng);
        SlotVector v(n);
        for (size_t i = 0; i < n; ++i) v[i] = i + 1;
        const CoeffPoly pt = batch_encode(v, prm);
        expect(batch_decode(pt, prm) == v, "decode(encode(v)) == v");
        const BfvCiphertext ct = encrypt_sk_with_rng(pt, sk, prm, rng);
        const BfvCiphertext sq = bfv_square_and_relin(ct, rlk);
        const BfvCiphertext rot = bfv_rotate_rows(sq, 1, gk);
        SlotVector want(n);
        for (size_t i = 0; i < n / 2; ++i) {
            const uint64_t a = v[(i + 1) % (n / 2)], b = v[n / 2 + (i + 1) % (n / 2)];
            want[i] = a * a % t;
            want[n / 2 + i] = b * b % t;
        }
        expect(batch_decode(decrypt(rot, sk), prm) == want, "squares mod t, rows rotated left by one");
        expect(batch_decrypt(rot, sk) == want, "batch_decrypt is decrypt then decode");
        // the same rng stream: batch_encrypt_sk is encode then encrypt bit for bit
        ChaChaRng r1(9), r2(9);
        const BfvCiphertext c1 = encrypt_sk_with_rng(pt, sk, prm, r1), c2 = batch_encrypt_sk(v, sk, prm, r2);
        expect(c1.c[0].data == c2.c[0].data && c1.c[1].data == c2.c[1].data, "batch_encrypt_sk is encode then encrypt");
        const BfvCiphertext same = bfv_rotate_rows(std::vector<BfvCiphertext>{sq}, (int64_t)(n / 2), nullptr)[0];
        expect(same.c[0].data == sq.c[0].data && same.c[1].data == sq.c[1].data, "n/2 steps copy without a key");
        threw = false;
        try {
            SlotVector bad(n, 0);
            bad[3] = t;
            (void)batch_encode(bad, prm);
        } catch (const ExactoError& e) {
            threw = std::string(e.variant()) == "InvalidParam" &&
                    std::string(e.what()).find("plaintext 65537 >= plain_modulus 65537") != std::string::npos;
        }
        expect(threw, "a value >= t is InvalidParam");
    } catch (const std::exception& e) {
        std::cout << "FAIL exception: " << e.what() << "\n";
        return 1;
    }
    if (failures) return 1;
    std::cout << "ALL OK\n";
    return 0;
}
