// C++ host-API test of slot-packed dBFV (include/exacto.hpp): at the u64 profile (b = 256, d = 8, p = 2^64) over
// three 60-bit primes with n = 4096 and the batching prime t = 1073153, keygen -> dbfv_batch_encrypt_sk of n
// 64-bit values per ciphertext -> dbfv_mul -> dbfv_batch_decrypt gives a[i] * b[i] in wrapping uint64_t in every
// slot, and dbfv_rotate_rows moves the wide slots.  Run with the argument "host" it only checks that the
// header's declarations link (no device needed).  Prints "PASS <name>" per step and "ALL OK" at the end.
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
        DbfvSlotPlain (*f1)(const SlotVector&, const DbfvParamsPtr&) = &dbfv_batch_encode;
        SlotVector (*f2)(const DbfvSlotPlain&, const DbfvParamsPtr&) = &dbfv_batch_decode;
        DbfvCiphertext (*f3)(const SlotVector&, const SecretKey&, const DbfvParamsPtr&, ChaChaRng&) = &dbfv_batch_encrypt_sk;
        DbfvCiphertext (*f4)(const SlotVector&, const PublicKey&, const DbfvParamsPtr&, ChaChaRng&) = &dbfv_batch_encrypt_pk;
        SlotVector (*f5)(const DbfvCiphertext&, const SecretKey&) = &dbfv_batch_decrypt;
        DbfvCiphertext (*f6)(const DbfvCiphertext&, int64_t, const GaloisKey&) = &dbfv_rotate_rows;
        DbfvCiphertext (*f7)(const DbfvCiphertext&, const GaloisKey&) = &dbfv_swap_rows;
        expect(f1 && f2 && f3 && f4 && f5 && f6 && f7, "declarations");
        if (argc > 1 && std::string(argv[1]) == "host") {
            if (failures) return 1;
            std::cout << "ALL OK\n";
            return 0;
        }
        const size_t n = 4096;
        auto bfv = BfvParamsBuilder().ring_degree(n).plain_modulus(1073153)
                       .ct_moduli({1152921504606830593ull, 1152921504606748673ull, 1152921504606683137ull}).build();
        DbfvParamsPtr dp = std::make_shared<DbfvParams>(DbfvParams{bfv, 256, 8, 0});
        expect(batch_root(bfv) != 0, "the context batches");
        ChaChaRng rng(5);
        const SecretKey sk = gen_secret_key_with_rng(bfv, rng);
        const RelinKey rlk = gen_relin_key_with_rng(sk, rng);
        SlotVector a(n), b(n), want(n);
        uint64_t x = 0x9E3779B97F4A7C15ull;
        for (size_t i = 0; i < n; ++i) {
            x = x * 6364136223846793005ull + 1442695040888963407ull;
            a[i] = x;
            x = x * 6364136223846793005ull + 1442695040888963407ull;
            b[i] = x;
        }
        a[0] = b[0] = ~0ull;   // (2^64 - 1)^2 = 1
        a[1] = ~0ull;
        b[2] = 0;
        for (size_t i = 0; i < n; ++i) want[i] = a[i] * b[i];
        expect(dbfv_batch_decode(dbfv_batch_encode(a, dp), dp) == a, "decode(encode(a)) == a");
        const DbfvCiphertext ca = dbfv_batch_encrypt_sk(a, sk, dp, rng), cb = dbfv_batch_encrypt_sk(b, sk, dp, rng);
        expect(ca.num_limbs() == 8 && dbfv_batch_decrypt(ca, sk) == a, "encrypt / decrypt round trip");
        const DbfvCiphertext prod = dbfv_mul(ca, cb, rlk);
        expect(dbfv_batch_decrypt(prod, sk) == want, "n products a[i] * b[i] mod 2^64 in one dbfv_mul");
        const GaloisKey gk = gen_galois_key_with_rng(sk, galois_element_rotate_rows(n, 1), rng);
        SlotVector rot(n);
        for (size_t i = 0; i < n / 2; ++i) {
            rot[i] = a[(i + 1) % (n / 2)];
            rot[n / 2 + i] = a[n / 2 + (i + 1) % (n / 2)];
        }
        expect(dbfv_batch_decrypt(dbfv_rotate_rows(ca, 1, gk), sk) == rot, "rows rotated left by one");
        bool threw = false;
        try {
            (void)dbfv_swap_rows(ca, gk);
        } catch (const ExactoError& e) {
            threw = std::string(e.variant()) == "InvalidParam";
        }
        expect(threw, "a rotation key is not the row swap's");
    } catch (const std::exception& e) {
        std::cout << "FAIL exception: " << e.what() << "\n";
        return 1;
    }
    if (failures) return 1;
    std::cout << "ALL OK\n";
    return 0;
}
