// C++ host-API test of the dBFV plaintext products (include/exacto.hpp): at n = 16 over three 60-bit primes,
// with (b = 16, d = 2, p = 256, t = 12289) and at the u64 shape (b = 256, d = 8, p = 2^64, t = 1040449),
// keygen -> dbfv_batch_encrypt_sk -> dbfv_batch_plain_mul by public values -> dbfv_batch_decrypt gives
// a[i] * w[i] mod p in every slot; dbfv_plain_mul_sum, dbfv_plain_add and dbfv_plain_sub likewise; then the
// error strings.  Run with the argument "host" it only checks that the header's declarations link (no device
// needed).  Prints "PASS <name>" per step and "ALL OK" at the end.
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
static void expect_error(F f, const std::string& variant, const std::string& text, const std::string& name) {
    bool ok = false;
    try {
        f();
    } catch (const ExactoError& e) {
        ok = std::string(e.variant()) == variant && std::string(e.what()).find(text) != std::string::npos;
        if (!ok) std::cout << "     got: " << e.variant() << ": " << e.what() << "\n";
    }
    expect(ok, name);
}

static void run_shape(uint64_t t, uint64_t base, size_t d, uint64_t p, const std::string& tag) {
    const size_t n = 16;
    auto bfv = BfvParamsBuilder().ring_degree(n).plain_modulus(t)
                   .ct_moduli({1152921504606830593ull, 1152921504606748673ull, 1152921504606683137ull}).build();
    DbfvParamsPtr dp = std::make_shared<DbfvParams>(DbfvParams{bfv, base, d, p});
    ChaChaRng rng(9);
    const SecretKey sk = gen_secret_key_with_rng(bfv, rng);
    auto mod = [&](unsigned __int128 v) { return p ? (uint64_t)(v % p) : (uint64_t)v; };
    SlotVector a(n), w(n), mul(n), add(n), sub(n), dot(n);
    uint64_t x = 0x9E3779B97F4A7C15ull;
    for (size_t i = 0; i < n; ++i) {
        x = x * 6364136223846793005ull + 1442695040888963407ull;
        a[i] = mod(x);
        x = x * 6364136223846793005ull + 1442695040888963407ull;
        w[i] = mod(x);
    }
    const uint64_t top = p ? p - 1 : ~0ull;
    a[0] = 0; a[1] = 1; a[2] = a[3] = top;
    w[0] = w[1] = w[2] = top; w[3] = top - 1;
    for (size_t i = 0; i < n; ++i) {
        mul[i] = mod((unsigned __int128)a[i] * w[i]);
        add[i] = mod((unsigned __int128)a[i] + w[i]);
        sub[i] = mod((unsigned __int128)a[i] + (p ? p : 0) - w[i]);
        dot[i] = mod((unsigned __int128)a[i] * w[i] + (unsigned __int128)w[i] * a[i]);
    }
    const DbfvCiphertext ca = dbfv_batch_encrypt_sk(a, sk, dp, rng), cw = dbfv_batch_encrypt_sk(w, sk, dp, rng);
    const DbfvSlotPlain pw = dbfv_batch_encode(w, dp), pa = dbfv_batch_encode(a, dp);
    const DbfvCiphertext prod = dbfv_batch_plain_mul(ca, w);
    expect(prod.num_limbs() == d && prod.mul_depth == 1, tag + ": d limbs at depth 1");
    expect(dbfv_batch_decrypt(prod, sk) == mul, tag + ": a[i] * w[i] mod p in every slot");
    expect(dbfv_batch_decrypt(dbfv_plain_mul(ca, pw), sk) == mul, tag + ": dbfv_plain_mul of the encoded values");
    if (d == 2)   // t = 12289 holds the digits of a sum of two products; t = 1040449 at d = 8 holds one
        expect(dbfv_batch_decrypt(dbfv_plain_mul_sum({ca, cw}, {pw, pa}), sk) == dot, tag + ": a w + w a");
    const DbfvCiphertext sum = dbfv_plain_add(ca, pw);
    expect(sum.mul_depth == 0 && dbfv_batch_decrypt(sum, sk) == add, tag + ": a[i] + w[i]");
    expect(dbfv_batch_decrypt(dbfv_plain_sub(ca, pw), sk) == sub, tag + ": a[i] - w[i]");
    expect(dbfv_batch_decrypt(dbfv_plain_sub(sum, pw), sk) == a, tag + ": add then sub");
    if (d == 2) {
        expect_error([&] { (void)dbfv_plain_mul(prod, pw); }, "NotImplemented",
                     "chained dBFV multiplication requires ciphertext-level lattice reduction", "a product of a product");
        expect_error([&] { (void)dbfv_plain_mul_sum({ca, cw}, {pw}); }, "InvalidParam", "mismatched ct/pt lengths",
                     "two ciphertexts, one plaintext");
        expect_error([&] { (void)dbfv_plain_mul_sum({}, {}); }, "InvalidParam", "mismatched ct/pt lengths", "no terms");
        DbfvSlotPlain shortpt(pw.begin(), pw.begin() + 1);
        expect_error([&] { (void)dbfv_plain_mul(ca, shortpt); }, "InvalidParam", "expected d digit plaintexts",
                     "a plaintext of d - 1 digits");
        expect_error([&] { (void)dbfv_plain_add(ca, shortpt); }, "InvalidParam", "expected d digit plaintexts",
                     "plain_add of d - 1 digits");
        SlotVector few(n - 1);
        expect_error([&] { (void)dbfv_batch_plain_mul(ca, few); }, "DimensionMismatch", "expected 16, got 15",
                     "n - 1 values");
    }
}

int main(int argc, char** argv) {
    try {
        DbfvCiphertext (*f1)(const DbfvCiphertext&, const DbfvSlotPlain&) = &dbfv_plain_mul;
        DbfvCiphertext (*f2)(const std::vector<DbfvCiphertext>&, const std::vector<DbfvSlotPlain>&) = &dbfv_plain_mul_sum;
        DbfvCiphertext (*f3)(const DbfvCiphertext&, const DbfvSlotPlain&) = &dbfv_plain_add;
        DbfvCiphertext (*f4)(const DbfvCiphertext&, const DbfvSlotPlain&) = &dbfv_plain_sub;
        DbfvCiphertext (*f5)(const DbfvCiphertext&, const SlotVector&) = &dbfv_batch_plain_mul;
        expect(f1 && f2 && f3 && f4 && f5, "declarations");
        if (argc > 1 && std::string(argv[1]) == "host") {
            if (failures) return 1;
            std::cout << "ALL OK\n";
            return 0;
        }
        run_shape(12289, 16, 2, 256, "d = 2");
        run_shape(1040449, 256, 8, 0, "d = 8, p = 2^64");
    } catch (const std::exception& e) {
        std::cout << "FAIL exception: " << e.what() << "\n";
        return 1;
    }
    if (failures) return 1;
    std::cout << "ALL OK\n";
    return 0;
}
