// C++ host-API test of the squares (include/exacto.hpp): bfv_square_and_relin / bfv_square_no_relin at
// compact_bfv (presets.rs:24-35) and dbfv_square at u64_dbfv (presets.rs:61-75): keygen -> encrypt 3 and 5 ->
// square -> decrypt, checking x^2 mod t (mod p for dBFV) and the two-operand call bit for bit.  Run with
// the argument "host" it only checks that the header's declarations are usable (no device needed).
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

static bool same(const BfvCiphertext& a, const BfvCiphertext& b) {
    if (a.c.size() != b.c.size()) return false;
    for (size_t i = 0; i < a.c.size(); ++i)
        if (a.c[i].data != b.c[i].data) return false;
    return true;
}

int main(int argc, char** argv) {
    try {
        // the declarations: batched and single forms
        std::vector<BfvCiphertext> (*f1)(const std::vector<BfvCiphertext>&) = &bfv_square_no_relin;
        std::vector<BfvCiphertext> (*f2)(const std::vector<BfvCiphertext>&, const RelinKey&) = &bfv_square_and_relin;
        BfvCiphertext (*f3)(const BfvCiphertext&) = &bfv_square_no_relin;
        BfvCiphertext (*f4)(const BfvCiphertext&, const RelinKey&) = &bfv_square_and_relin;
        std::vector<DbfvCiphertext> (*f5)(const std::vector<DbfvCiphertext>&, const RelinKey&) = &dbfv_square;
        DbfvCiphertext (*f6)(const DbfvCiphertext&, const RelinKey&) = &dbfv_square;
        expect(f1 && f2 && f3 && f4 && f5 && f6, "declarations");
        expect(f1(std::vector<BfvCiphertext>{}).empty(), "empty batch");
        if (argc > 1 && std::string(argv[1]) == "host") {
            if (failures) return 1;
            std::cout << "ALL OK\n";
            return 0;
        }
        {
            auto prm = BfvParamsBuilder().ring_degree(1024).plain_modulus(257).ct_moduli({1099509805057ull})
                           .aux_moduli({562949953443841ull}).sigma(3.2).build();
            ChaChaRng rng(7);
            const SecretKey sk = gen_secret_key_with_rng(prm, rng);
            const RelinKey rlk = gen_relin_key_with_rng(sk, rng);
            const uint64_t x[2] = {3, 5}, t = prm->plain_modulus;
            std::vector<BfvCiphertext> a;
            for (int k = 0; k < 2; ++k) a.push_back(encrypt_sk_with_rng(encode_scalar(x[k], prm), sk, prm, rng));
            const std::vector<BfvCiphertext> sq = bfv_square_and_relin(a, rlk);
            expect(sq.size() == 2 && sq[0].c.size() == 2, "two degree-1 outputs");
            expect(decode_scalar(decrypt(sq[0], sk)) == 9 % t, "3^2 decrypts to 9 mod t");
            expect(decode_scalar(decrypt(sq[1], sk)) == 25 % t, "5^2 decrypts to 25 mod t");
            expect(same(sq[0], bfv_mul_and_relin(a[0], a[0], rlk)) && same(sq[1], bfv_mul_and_relin(a[1], a[1], rlk)),
                   "equals bfv_mul_and_relin(x, x) bit for bit");
            const BfvCiphertext s3 = bfv_square_no_relin(a[1]);
            expect(s3.c.size() == 3 && same(s3, bfv_mul_no_relin(a[1], a[1])), "bfv_square_no_relin equals bfv_mul_no_relin(x, x)");
            expect(same(relinearize(s3, rlk), sq[1]), "relinearize(bfv_square_no_relin) equals bfv_square_and_relin");
            expect(same(bfv_square_and_relin(a[0], rlk), sq[0]), "single form");
        }
        {
            auto bfv = BfvParamsBuilder().ring_degree(4096).plain_modulus(1040407).ct_moduli({1152921504606830593ull})
                           .aux_moduli({18014398509998081ull, 36028797018972161ull}).gadget_base(256).sigma(3.2).build();
            DbfvParamsPtr dp = std::make_shared<DbfvParams>(DbfvParams{bfv, 256, 8, 0});
            ChaChaRng rng(11);
            const SecretKey sk = gen_secret_key_with_rng(bfv, rng);
            const RelinKey rlk = gen_relin_key_with_rng(sk, rng);
            const uint64_t x[2] = {3, 0xFFFFFFFF00000005ull};
            std::vector<DbfvCiphertext> a;
            for (int k = 0; k < 2; ++k) a.push_back(dbfv_encrypt_sk_with_rng(x[k], sk, dp, rng));
            const std::vector<DbfvCiphertext> sq = dbfv_square(a, rlk);
            expect(sq.size() == 2 && sq[0].num_limbs() == 8 && sq[0].mul_depth == 1, "dbfv outputs");
            expect(dbfv_decrypt(sq[0], sk) == 9, "dBFV 3^2 decrypts to 9");
            expect(dbfv_decrypt(sq[1], sk) == x[1] * x[1], "dBFV x^2 decrypts to x^2 mod 2^64");
            const DbfvCiphertext want = dbfv_mul(a[1], a[1], rlk);
            bool eq = want.num_limbs() == sq[1].num_limbs() && want.mul_depth == sq[1].mul_depth;
            for (size_t k = 0; eq && k < want.num_limbs(); ++k) eq = same(want.limbs[k], sq[1].limbs[k]);
            expect(eq, "equals dbfv_mul(x, x) bit for bit");
            bool threw = false;
            try {
                (void)dbfv_square(sq[0], rlk);
            } catch (const ExactoError& e) {
                threw = std::string(e.variant()) == "NotImplemented";
            }
            expect(threw, "depth 1 in is NotImplemented");
        }
    } catch (const std::exception& e) {
        std::cout << "FAIL exception: " << e.what() << "\n";
        return 1;
    }
    if (failures) return 1;
    std::cout << "ALL OK\n";
    return 0;
}
