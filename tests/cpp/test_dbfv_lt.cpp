// C++ host-API test of the dBFV hoisted rotations and linear transforms (include/exacto.hpp): DbfvDiagonals,
// dbfv_rotate_hoisted, dbfv_rotate_rows_many and dbfv_linear_transform in its raw and prepared overloads.  Run
// with the argument "host" it only checks that the header's declarations link (no device needed).  Otherwise
// it runs one shape on the fused route (n = 64, switched on) and one on the staged route (n = 1024, the 31-bit key switch)
// over cfg3's primes at (b = 16, d = 2, p = 251) on residues from a fixed generator, checks the raw form
// against the prepared one and the rotations against the identity element, and prints
// "DIGEST <shape> <FNV-1a of the output words>", which tests/test_cpp_dbfv_lt.py holds against the ctypes
// result on the same inputs.  Prints "PASS <name>" per step and "ALL OK" at the end.
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

static uint64_t lcg_state = 0x9E3779B97F4A7C15ull;
static uint64_t next_word() {
    lcg_state = lcg_state * 6364136223846793005ull + 1442695040888963407ull;
    return lcg_state;
}

static const std::vector<uint64_t> Q3 = {1152921504606830593ull, 1152921504606748673ull, 1152921504606683137ull};

// [rows][L][n] residues in the generator's order
static std::vector<uint64_t> residues(size_t rows, size_t n) {
    std::vector<uint64_t> out(rows * Q3.size() * n);
    for (size_t r = 0; r < rows; ++r)
        for (size_t l = 0; l < Q3.size(); ++l)
            for (size_t i = 0; i < n; ++i) out[(r * Q3.size() + l) * n + i] = next_word() % Q3[l];
    return out;
}

static uint64_t fnv(const DbfvCiphertext& ct) {
    uint64_t h = 1469598103934665603ull;
    for (auto& limb : ct.limbs)
        for (auto& c : limb.c)
            for (uint64_t w : c.data)
                for (int b = 0; b < 8; ++b) {
                    h ^= (w >> (8 * b)) & 0xff;
                    h *= 1099511628211ull;
                }
    return h;
}

static bool same(const DbfvCiphertext& a, const DbfvCiphertext& b) {
    if (a.num_limbs() != b.num_limbs()) return false;
    for (size_t k = 0; k < a.num_limbs(); ++k)
        for (size_t c = 0; c < 2; ++c)
            if (a.limbs[k].c[c].data != b.limbs[k].c[c].data) return false;
    return true;
}

static void run_shape(size_t n, bool want_fused, const std::string& tag) {
    lcg_state = 0x9E3779B97F4A7C15ull + n;
    const uint64_t base = 16, p = 251;
    const size_t d = 2, L = Q3.size();
    auto bfv = BfvParamsBuilder().ring_degree(n).plain_modulus(12289).ct_moduli(Q3).build();
    DbfvParamsPtr dp = std::make_shared<DbfvParams>(DbfvParams{bfv, base, d, p});
    const DbfvCiphertext ct = detail::make_dbfv(residues(d * 2, n), d, 2, d, 0, dp);
    const std::vector<size_t> elements = {3, 1, 2 * n - 1};
    std::vector<GaloisKey> keys;
    for (size_t el : elements) {
        GaloisKey gk;
        gk.element = el;
        gk.params = bfv;
        if (el != 1)
            for (size_t g = 0; g < bfv->gadget_digits; ++g) {
                RnsPoly k0{n, L, residues(1, n)}, k1{n, L, residues(1, n)};
                gk.keys.emplace_back(k0, k1);
            }
        keys.push_back(gk);
    }
    const GaloisKeySet ks(bfv, keys);
    std::vector<DbfvSlotPlain> pts(elements.size(), DbfvSlotPlain(d));
    for (auto& pt : pts)
        for (auto& row : pt) {
            row.coeffs.resize(n);
            row.modulus = 12289;
            for (auto& c : row.coeffs) c = next_word();
        }
    if (want_fused) detail::check(exacto_ctx_set_dbfv_lt_fused(bfv->ctx(), 1));   // the default is the staged route
    const DbfvDiagonals dg(dp, pts);
    expect(dg.size() == elements.size() && dg.fused() == want_fused, tag + ": the route");
    expect((ks.ks32_primes() > 0) == !want_fused, tag + ": the key switch");
    const auto rot = dbfv_rotate_hoisted(ct, ks);
    expect(rot.size() == elements.size() && same(rot[1], ct), tag + ": the identity's rotation is the input");
    const DbfvCiphertext raw = dbfv_linear_transform(ct, ks, pts), prep = dbfv_linear_transform(ct, ks, dg);
    expect(raw.num_limbs() == d && raw.mul_depth == 1, tag + ": d limbs at depth 1");
    expect(same(raw, prep), tag + ": raw and prepared diagonals agree");
    // the composition of the calls that existed before: the product over the rotations
    expect(same(raw, dbfv_plain_mul_sum(rot, pts)), tag + ": dbfv_plain_mul_sum over the rotations");
    std::printf("DIGEST %s %016llx\n", tag.c_str(), (unsigned long long)fnv(raw));
    bool threw = false;
    try {
        (void)dbfv_linear_transform(raw, ks, dg);
    } catch (const ExactoError& e) {
        threw = std::string(e.variant()) == "NotImplemented";
    }
    expect(threw, tag + ": a transform of a product is NotImplemented");
    threw = false;
    try {
        (void)dbfv_rotate_rows_many(ct, {1, 0}, ks);
    } catch (const ExactoError& e) {
        threw = std::string(e.variant()) == "InvalidParam";
    }
    expect(threw, tag + ": steps that are not the set's");
}

int main(int argc, char** argv) {
    try {
        std::vector<DbfvCiphertext> (*f1)(const DbfvCiphertext&, const GaloisKeySet&) = &dbfv_rotate_hoisted;
        std::vector<DbfvCiphertext> (*f2)(const DbfvCiphertext&, const std::vector<int64_t>&, const GaloisKeySet&) =
            &dbfv_rotate_rows_many;
        DbfvCiphertext (*f3)(const DbfvCiphertext&, const GaloisKeySet&, const std::vector<DbfvSlotPlain>&) =
            &dbfv_linear_transform;
        DbfvCiphertext (*f4)(const DbfvCiphertext&, const GaloisKeySet&, const DbfvDiagonals&) = &dbfv_linear_transform;
        expect(f1 && f2 && f3 && f4 && sizeof(DbfvDiagonals) > 0, "declarations");
        if (argc > 1 && std::string(argv[1]) == "host") {
            if (failures) return 1;
            std::cout << "ALL OK\n";
            return 0;
        }
        run_shape(64, true, "fused_n64");
        run_shape(1024, false, "staged_n1024");
    } catch (const std::exception& e) {
        std::cout << "FAIL exception: " << e.what() << "\n";
        return 1;
    }
    if (failures) return 1;
    std::cout << "ALL OK\n";
    return 0;
}
