// C++ host-API test of the noise measurement (include/exacto.hpp: bfv_noise_inf, max_limb_noise,
// noise_budget_bits), following the reference's own evaluation (src/bin/paper_repro.rs:166-201, 238-281) at
// compact_dbfv: keygen -> dbfv_encrypt_sk -> max_limb_noise -> dbfv_mul -> max_limb_noise, asserting
// growth and a positive budget before.  Run with the argument "host" it checks only the word and budget
// helpers, which need no device.  Prints "PASS <name>" per step and "ALL OK" at the end.
#include <algorithm>
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

static void host_helpers() {
    Noise z{{0, 0, 0}}, one{{1, 0, 0}}, w64{{~0ull, 0, 0}}, w65{{0, 1, 0}}, top{{5, 0, 1ull << 63}}, none{{}};
    expect(z.bit_length() == 0 && one.bit_length() == 1 && w64.bit_length() == 64 && w65.bit_length() == 65 &&
               top.bit_length() == 192 && none.bit_length() == 0,
           "Noise::bit_length");
    expect(z.fits_u64() && w64.fits_u64() && !w65.fits_u64() && !top.fits_u64() && none.fits_u64(), "Noise::fits_u64");
    expect(z.to_u64() == 0 && w64.to_u64() == ~0ull && none.to_u64() == 0, "Noise::to_u64");
    bool threw = false;
    try {
        (void)w65.to_u64();
    } catch (const ExactoError& e) {
        threw = std::string(e.what()).find("does not fit 64 bits") != std::string::npos;
    }
    expect(threw, "Noise::to_u64 throws past 64 bits");
    // compact_dbfv: q = 1099509805057, t = 929: Delta = 1183541232, floor(Delta / 2) = 591770616 (30 bits)
    const std::vector<uint64_t> q1 = {1099509805057ull};
    expect(detail::half_delta_bits(q1, 929) == 30, "half_delta_bits (one prime)");
    expect(noise_budget_bits(Noise{{0}}, q1, 929) == 30 && noise_budget_bits(Noise{{19}}, q1, 929) == 25 &&
               noise_budget_bits(Noise{{591770616ull}}, q1, 929) == 0 &&
               noise_budget_bits(Noise{{1ull << 40}}, q1, 929) == 0,
           "noise_budget_bits (one prime)");
    // cfg3: three 60-bit primes, p = 65537: Q has 180 bits, floor(Q / p) 164 (Q / 2^180 > p / 2^17), half of it 163
    const std::vector<uint64_t> q3 = {1152921504606830593ull, 1152921504606748673ull, 1152921504606683137ull};
    expect(detail::half_delta_bits(q3, 65537) == 163, "half_delta_bits (three primes)");
    expect(noise_budget_bits(Noise{{0, 0, 1}}, q3, 65537) == 163 - 129 && noise_budget_bits(top, q3, 65537) == 0,
           "noise_budget_bits (three primes)");
}

int main(int argc, char** argv) {
    try {
        host_helpers();
        if (argc > 1 && std::string(argv[1]) == "host") {
            if (failures) return 1;
            std::cout << "ALL OK\n";
            return 0;
        }
        // presets.rs:86-98 compact_dbfv
        auto bfv = BfvParamsBuilder().ring_degree(1024).plain_modulus(929).ct_moduli({1099509805057ull})
                       .aux_moduli({562949953443841ull}).sigma(3.2).build();
        DbfvParamsPtr params = std::make_shared<DbfvParams>(DbfvParams{bfv, 16, 2, 256});
        ChaChaRng rng(42);
        DbfvKeys keys = dbfv_keygen_full(params, {}, rng);

        DbfvCiphertext a = dbfv_encrypt_sk(200, keys.sk, params, rng), b = dbfv_encrypt_sk(3, keys.sk, params, rng);
        const Noise na = max_limb_noise(a, keys.sk), nb = max_limb_noise(b, keys.sk);
        expect(na.words.size() == 1 && na.to_u64() > 0 && na.to_u64() < 64 && nb.to_u64() > 0 && nb.to_u64() < 64,
               "max_limb_noise of fresh encryptions (a few sigma)");
        expect(noise_budget_bits(na, *bfv) > 0 && noise_budget_bits(nb, *bfv) > 0, "positive budget before");
        // the maximum over the limbs is the maximum of the per-limb values
        const std::vector<Noise> per = bfv_noise_inf(a.limbs, keys.sk);
        expect(per.size() == 2 && std::max(per[0].to_u64(), per[1].to_u64()) == na.to_u64() &&
                   bfv_noise_inf(a.limbs[1], keys.sk).to_u64() == per[1].to_u64(),
               "bfv_noise_inf per limb");

        DbfvCiphertext prod = dbfv_mul(a, b, keys.rlk);
        expect(dbfv_decrypt(prod, keys.sk) == (200 * 3) % 256, "dbfv_mul value");
        const Noise np = max_limb_noise(prod, keys.sk);
        const uint64_t in = std::max(na.to_u64(), nb.to_u64());
        std::printf("noise in %llu, out %llu, growth %.1f, budget %zu -> %zu bits\n", (unsigned long long)in,
                    (unsigned long long)np.to_u64(), (double)np.to_u64() / (double)in, noise_budget_bits(na, *bfv),
                    noise_budget_bits(np, *bfv));
        expect(np.to_u64() > in, "noise grows through dbfv_mul");
        expect(noise_budget_bits(np, *bfv) < noise_budget_bits(na, *bfv), "budget shrinks through dbfv_mul");
        expect(max_limb_noise(prod, keys.sk).words == np.words, "two calls agree");
    } catch (const std::exception& e) {
        std::cout << "FAIL exception: " << e.what() << "\n";
        return 1;
    }
    if (failures) return 1;
    std::cout << "ALL OK\n";
    return 0;
}
