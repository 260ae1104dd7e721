// C++ host-API test of the hoisted rotations (include/exacto.hpp).  Run with the argument "host" it checks
// galois_ntt_permutation on the CPU: a permutation, composing as the elements multiply (the table of k k' is
// perm_k o perm_k'), the errors, and that the header's declarations link.  Without it, at cfg3's basis with
// n = 1024: keygen -> batch_encode (1 .. n) -> encrypt -> bfv_rotate_hoisted by (1, 0, -1) and the row swap ->
// decrypt gives the rotated rows, and bfv_linear_transform the weighted sum of them.
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

static SlotVector rolled(const SlotVector& v, int64_t s, bool swap) {
    const size_t n = v.size(), h = n / 2;
    SlotVector w(n);
    for (size_t i = 0; i < h; ++i) {
        const size_t j = (size_t)((((int64_t)i + s) % (int64_t)h + (int64_t)h) % (int64_t)h);
        w[i] = v[(swap ? h : 0) + j];
        w[h + i] = v[(swap ? 0 : h) + j];
    }
    return w;
}

int main(int argc, char** argv) {
    try {
        std::vector<std::vector<BfvCiphertext>> (*f1)(const std::vector<BfvCiphertext>&, const GaloisKeySet&) =
            &bfv_rotate_hoisted;
        std::vector<BfvCiphertext> (*f2)(const std::vector<BfvCiphertext>&, const GaloisKeySet&,
                                         const std::vector<CoeffPoly>&) = &bfv_linear_transform;
        expect(f1 && f2, "declarations");
        bool ok = true;
        for (size_t n : {16u, 64u, 1024u, 16384u}) {
            const uint64_t ks[] = {3, 5, 2 * n - 1, 1, 4 * n + 3};
            for (uint64_t k : ks) {
                const auto p = galois_ntt_permutation(n, k);
                std::vector<char> seen(n, 0);
                for (uint32_t x : p) {
                    ok = ok && x < n && !seen[x];
                    if (x < n) seen[x] = 1;
                }
                for (uint64_t k2 : ks) {
                    // NTT(sigma_k(sigma_k2(a)))[p] = NTT(sigma_k2(a))[perm_k[p]] = NTT(a)[perm_k2[perm_k[p]]]
                    const auto p2 = galois_ntt_permutation(n, k2), pk = galois_ntt_permutation(n, k * k2);
                    for (size_t i = 0; i < n; ++i) ok = ok && pk[i] == p2[p[i]];
                }
            }
            const auto id = galois_ntt_permutation(n, 1);
            for (size_t i = 0; i < n; ++i) ok = ok && id[i] == i;
        }
        expect(ok, "galois_ntt_permutation: permutations that compose");
        bool threw = false;
        try {
            (void)galois_ntt_permutation(64, 10);
        } catch (const ExactoError& e) {
            threw = std::string(e.variant()) == "InvalidParam" &&
                    std::string(e.what()).find("hoisted automorphisms require odd Galois elements") != std::string::npos;
        }
        expect(threw, "an even element is InvalidParam");
        threw = false;
        try {
            (void)galois_ntt_permutation(48, 3);
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
        ChaChaRng rng(5);
        const SecretKey sk = gen_secret_key_with_rng(prm, rng);
        std::vector<GaloisKey> keys;
        const int64_t steps[] = {1, 0, -1};
        for (int64_t s : steps) {
            const size_t el = galois_element_rotate_rows(n, s);
            if (el == 1) {
                GaloisKey id;
                id.element = 1;
                id.params = prm;
                keys.push_back(id);
            } else {
                keys.push_back(gen_galois_key_with_rng(sk, el, rng));
            }
        }
        keys.push_back(gen_galois_key_with_rng(sk, galois_element_swap_rows(n), rng));
        const GaloisKeySet ks(prm, keys);
        expect(ks.size() == 4 && ks.ks32_primes() > 0, "a set of four on the 31-bit key switch");
        SlotVector v(n);
        for (size_t i = 0; i < n; ++i) v[i] = i + 1;
        const BfvCiphertext ct = batch_encrypt_sk(v, sk, prm, rng);
        const auto rot = bfv_rotate_hoisted(ct, ks);
        expect(rot.size() == 4, "four rotations");
        for (size_t r = 0; r < 3; ++r)
            expect(batch_decrypt(rot[r], sk) == rolled(v, steps[r], false), "rows rotated by " + std::to_string(steps[r]));
        expect(batch_decrypt(rot[3], sk) == rolled(v, 0, true), "rows swapped");
        expect(rot[1].c[0].data == ct.c[0].data && rot[1].c[1].data == ct.c[1].data, "the identity copies");
        std::vector<SlotVector> w(4, SlotVector(n));
        for (size_t r = 0; r < 4; ++r)
            for (size_t i = 0; i < n; ++i) w[r][i] = (7 * r + 3 * i + 1) % t;
        const auto lt = bfv_linear_transform(std::vector<BfvCiphertext>{ct}, ks, batch_encode(w, prm));
        SlotVector want(n, 0);
        for (size_t r = 0; r < 4; ++r) {
            const SlotVector x = r < 3 ? rolled(v, steps[r], false) : rolled(v, 0, true);
            for (size_t i = 0; i < n; ++i) want[i] = (want[i] + w[r][i] * x[i]) % t;
        }
        expect(batch_decrypt(lt[0], sk) == want, "linear transform: the weighted sum of the rotations");
    } catch (const std::exception& e) {
        std::cout << "FAIL exception: " << e.what() << "\n";
        return 1;
    }
    if (failures) return 1;
    std::cout << "ALL OK\n";
    return 0;
}
