// C ABI: decryption, modulus switch and noise measurement.
// Part of the host runtime of libexacto_hip.so; the shared types and helpers are in runtime.hpp.
#include "runtime.hpp"

using namespace exacto;

// ============================================================== decryption

// bfv/encrypt.rs:111-178 for a batch: phase = sum_k c_k s^k (NTT domain), INTT, exact rounding.
// ct = [B][polys][L][n] (stride ct_stride words per ciphertext), sk = [L][n] NTT domain.
int exacto::decrypt_batch(exacto_ctx* c, const u64* ct, size_t polys, long ct_stride, const u64* sk, u64* out,
                          size_t B) {
    if (polys < 1) return invalid_param("ciphertext has no polynomials");
    if (B == 0) return 0;
    const int L = c->L, n = c->n;
    if (L >= 2 && (c->K < 1 || c->plain >= c->primes[L]))
        return fail(EXACTO_ERR_NOT_IMPLEMENTED, "not yet implemented: GPU decryption needs plain_modulus below the "
                                                "first internal auxiliary prime");
    if (c->dec_buf.grow(B * L * poly_bytes(c))) return EXACTO_ERR_HIP;
    launch_phase(ct, (int)polys, ct_stride, sk, c->dec_buf, (int)B, n, L, c->d_primes, c->stream);
    CHECK_LAUNCH();
    if (int e = run_ntt(c, contiguous(c->dec_buf, (long)B, L, 0, L, n), (long)B * L, true)) return e;
    launch_decrypt_round(c->dec_buf, out, (int)B, n, L, c->d_crt, c->d_primes, c->plain, c->stream);
    CHECK_LAUNCH();
    return 0;
}

extern "C" int exacto_bfv_decrypt_dev(exacto_ctx* c, const uint64_t* ct, size_t polys, const uint64_t* sk,
                                      uint64_t* out, size_t B) {
    if (int e = check_ctx(c)) return e;
    return decrypt_batch(c, ct, polys, (long)polys * c->L * c->n, sk, out, B);
}

extern "C" int exacto_bfv_decrypt(exacto_ctx* c, const uint64_t* ct, size_t polys, const uint64_t* sk,
                                  uint64_t* out, size_t B) {
    if (!c) return invalid_param("null context");
    return host_call(c, {{ct, B * polys * c->L * poly_bytes(c)}, {sk, c->L * poly_bytes(c)}}, B * poly_bytes(c), out,
                     [&](std::vector<u64*>& dv, u64* o) { return exacto_bfv_decrypt_dev(c, dv[0], polys, dv[1], o, B); });
}

// dbfv/decrypt.rs:20-79: every limb decrypted with the BFV plaintext modulus t, then signed
// recomposition mod p coefficient-wise (poly) or of coefficient 0 (scalar).
static int dbfv_decrypt_common(exacto_ctx* c, size_t d, uint64_t base, uint64_t plain, const uint64_t* ct,
                               const uint64_t* sk, uint64_t* out, size_t B, bool scalar) {
    if (int e = check_ctx(c)) return e;
    if (int e = dbfv_params_check(d, base, plain)) return e;
    if (!scalar && plain == 0)
        return invalid_param("polynomial dBFV decrypt requires finite plain_modulus (plain_modulus=0 is scalar-only)");
    if (B == 0) return 0;
    const size_t nd = B * d;
    if (c->dig_buf.grow(nd * poly_bytes(c))) return EXACTO_ERR_HIP;
    if (int e = decrypt_batch(c, ct, 2, 2L * c->L * c->n, sk, c->dig_buf, nd)) return e;
    launch_dbfv_recompose(c->dig_buf, out, (int)B, c->n, (int)d, base, plain, c->plain, scalar, c->stream);
    CHECK_LAUNCH();
    return 0;
}

extern "C" int exacto_dbfv_decrypt_dev(exacto_ctx* c, size_t d, uint64_t base, uint64_t plain, const uint64_t* ct,
                                       const uint64_t* sk, uint64_t* out, size_t B) {
    return dbfv_decrypt_common(c, d, base, plain, ct, sk, out, B, true);
}

extern "C" int exacto_dbfv_decrypt_poly_dev(exacto_ctx* c, size_t d, uint64_t base, uint64_t plain,
                                            const uint64_t* ct, const uint64_t* sk, uint64_t* out, size_t B) {
    return dbfv_decrypt_common(c, d, base, plain, ct, sk, out, B, false);
}

extern "C" int exacto_dbfv_decrypt(exacto_ctx* c, size_t d, uint64_t base, uint64_t plain, const uint64_t* ct,
                                   const uint64_t* sk, uint64_t* out, size_t B) {
    if (!c) return invalid_param("null context");
    return host_call(c, {{ct, B * d * 2 * c->L * poly_bytes(c)}, {sk, c->L * poly_bytes(c)}}, B * sizeof(u64), out,
                     [&](std::vector<u64*>& dv, u64* o) {
                         return exacto_dbfv_decrypt_dev(c, d, base, plain, dv[0], dv[1], o, B);
                     });
}

extern "C" int exacto_dbfv_decrypt_poly(exacto_ctx* c, size_t d, uint64_t base, uint64_t plain,
                                        const uint64_t* ct, const uint64_t* sk, uint64_t* out, size_t B) {
    if (!c) return invalid_param("null context");
    return host_call(c, {{ct, B * d * 2 * c->L * poly_bytes(c)}, {sk, c->L * poly_bytes(c)}}, B * poly_bytes(c), out,
                     [&](std::vector<u64*>& dv, u64* o) {
                         return exacto_dbfv_decrypt_poly_dev(c, d, base, plain, dv[0], dv[1], o, B);
                     });
}

// ============================================================== modulus switch (bfv/modswitch.rs)

// Argument checks shared by both forms, before anything is launched or copied.
static int mod_switch_check(const exacto_ctx* c, size_t polys, size_t lin, size_t lout, int mode) {
    if (lin <= 1) return invalid_param("cannot drop prime: only one modulus remaining");
    if (lin > (size_t)c->L)
        return invalid_param("mod_switch: limbs_in = " + std::to_string(lin) + " exceeds the context's " +
                             std::to_string(c->L) + " ciphertext primes");
    if (lout == 0) return invalid_param("mod_switch: limbs_out = 0 (at least one prime must remain)");
    if (lout >= lin)
        return invalid_param("mod_switch: limbs_out = " + std::to_string(lout) + " must be below limbs_in = " +
                             std::to_string(lin));
    if (polys == 0) return invalid_param("mod_switch: ciphertext has no polynomials");
    if (mode != EXACTO_MODSWITCH_ROUND && mode != EXACTO_MODSWITCH_REFERENCE)
        return invalid_param("mod_switch: unknown mode " + std::to_string(mode));
    return 0;
}

// One drop l -> l - 1 of `rows` polynomials; the kernel path is chosen from the primes involved
// (0 .. l-1), as run_ntt chooses the transforms'.
static int run_drop_prime(exacto_ctx* c, const u64* in, u64* out, size_t rows, int l, bool round) {
    const int L = c->L;
    if (c->msw_w.empty()) {
        c->msw_w.assign((size_t)L * L, 0);
        c->msw_ws.assign((size_t)L * L, 0);
        for (int j = 1; j < L; ++j)
            for (int i = 0; i < j; ++i) {
                const u64 qi = c->ctq[i], w = invmod_h(c->ctq[j] % qi, qi);
                c->msw_w[(size_t)j * L + i] = w;
                c->msw_ws[(size_t)j * L + i] = shoup_h(w, qi);
            }
    }
    DropPrimeK K{};
    for (int i = 0; i < l - 1; ++i) {
        K.w[i] = c->msw_w[(size_t)(l - 1) * L + i];
        K.ws[i] = c->msw_ws[(size_t)(l - 1) * L + i];
    }
    bool lazy = true, near60 = c->ntt_asm && c->ntt_asm_inv;
    for (int t = 0; t < l; ++t) {
        lazy &= c->primes[t] < (1ull << 60);
        near60 &= c->primes[t] < (1ull << 60) && c->primes[t] > (1ull << 60) - (1ull << 32);
    }
    // algorithmic bytes: l rows read, l - 1 written
    ProfScope ps(c, PK_MODSWITCH, (u64)rows, 8.0 * c->n * (double)rows * (2 * l - 1));
    launch_drop_prime(in, out, (long)rows, l, round, K, c->logn, lazy, near60, c->d_primes, c->stream);
    CHECK_LAUNCH();
    return 0;
}

extern "C" int exacto_bfv_mod_switch_dev(exacto_ctx* c, const uint64_t* ct, size_t polys, size_t lin, size_t lout,
                                         int mode, uint64_t* out, size_t B) {
    if (int e = check_ctx(c)) return e;
    if (int e = mod_switch_check(c, polys, lin, lout, mode)) return e;
    if (B == 0) return 0;
    if (!ct || !out) return invalid_param("mod_switch: null ciphertext buffer");
    if (((uintptr_t)ct | (uintptr_t)out) & 15) return invalid_param("mod_switch: ct and out must be 16-byte aligned");
    const size_t n = (size_t)c->n, iw = polys * lin * n, ow = polys * lout * n;
    if (out < ct + B * iw && ct < out + B * ow) return invalid_param("mod_switch: out overlaps ct");
    const bool round = mode == EXACTO_MODSWITCH_ROUND;
    if (lin - lout == 1) return run_drop_prime(c, ct, out, B * polys, (int)lin, round);
    // several drops: chunk by chunk through two halves of the workspace, the last drop into out
    const size_t C = std::min(c->chunk, B), half = C * polys * (lin - 1) * n;
    if (c->msw_buf.grow(2 * half * sizeof(u64))) return EXACTO_ERR_HIP;
    for (size_t i0 = 0; i0 < B; i0 += C) {
        const size_t cnt = std::min(C, B - i0);
        const u64* src = ct + i0 * iw;
        int h = 0;
        for (size_t l = lin; l > lout; --l) {
            u64* dst = l - 1 == lout ? out + i0 * ow : c->msw_buf + h * half;
            if (int e = run_drop_prime(c, src, dst, cnt * polys, (int)l, round)) return e;
            src = dst;
            h ^= 1;
        }
    }
    return 0;
}

extern "C" int exacto_bfv_mod_switch(exacto_ctx* c, const uint64_t* ct, size_t polys, size_t lin, size_t lout, int mode,
                                     uint64_t* out, size_t B) {
    if (!c) return invalid_param("null context");
    if (int e = mod_switch_check(c, polys, lin, lout, mode)) return e;
    if (B == 0) return 0;
    if (!ct || !out) return invalid_param("mod_switch: null ciphertext buffer");
    const size_t iw = polys * lin * (size_t)c->n, ow = polys * lout * (size_t)c->n;
    if (out < ct + B * iw && ct < out + B * ow) return invalid_param("mod_switch: out overlaps ct");
    return host_call(c, {{ct, B * iw * sizeof(u64)}}, B * ow * sizeof(u64), out, [&](std::vector<u64*>& in, u64* o) {
        return exacto_bfv_mod_switch_dev(c, in[0], polys, lin, lout, mode, o, B);
    });
}

// ============================================================== noise (paper_repro.rs:238-281)

// The decryption's phase and inverse NTT into dec_buf, then noise.hip: the maximum of the centred
// residual |x - m Delta| over each group of `group` consecutive ciphertexts, L binary words each.
// The per-workgroup partial maxima live behind the phase in dec_buf.  Delta's residues are uploaded
// on the context's first use of them (as for encryption); nothing else waits for the device.
static int noise_batch(exacto_ctx* c, const u64* ct, size_t polys, long ct_stride, const u64* sk, const u64* expected,
                       u64* plain_out, u64* noise_out, size_t items, size_t group) {
    if (polys < 1) return invalid_param("ciphertext has no polynomials");
    if (items == 0) return 0;
    const int L = c->L, n = c->n;
    const bool round = !expected || plain_out;
    if (round && L >= 2 && (c->K < 1 || c->plain >= c->primes[L]))
        return fail(EXACTO_ERR_NOT_IMPLEMENTED, "not yet implemented: GPU decryption needs plain_modulus below the "
                                                "first internal auxiliary prime");
    if (int e = delta_residues(c)) return e;
    const size_t phase_words = items * L * (size_t)n;
    if (c->dec_buf.grow((phase_words + items * noise_chunks(n) * L) * sizeof(u64))) return EXACTO_ERR_HIP;
    launch_phase(ct, (int)polys, ct_stride, sk, c->dec_buf, (int)items, n, L, c->d_primes, c->stream);
    CHECK_LAUNCH();
    if (int e = run_ntt(c, contiguous(c->dec_buf, (long)items, L, 0, L, n), (long)items * L, true)) return e;
    launch_noise(c->dec_buf, expected, plain_out, c->dec_buf + phase_words, noise_out, (long)items, (int)group, n, L,
                 c->d_crt, c->d_primes, c->d_delta, c->plain, round, c->stream);
    CHECK_LAUNCH();
    return 0;
}

extern "C" int exacto_bfv_noise_dev(exacto_ctx* c, const uint64_t* ct, size_t polys, const uint64_t* sk,
                                    const uint64_t* expected, uint64_t* plain_out, uint64_t* noise_out, size_t B) {
    if (int e = check_ctx(c)) return e;
    return noise_batch(c, ct, polys, (long)polys * c->L * c->n, sk, expected, plain_out, noise_out, B, 1);
}

extern "C" int exacto_bfv_noise(exacto_ctx* c, const uint64_t* ct, size_t polys, const uint64_t* sk,
                                const uint64_t* expected, uint64_t* plain_out, uint64_t* noise_out, size_t B) {
    if (!c) return invalid_param("null context");
    // one staged output: [the plaintexts, if asked for][the noise words]
    const size_t pw = plain_out ? B * (size_t)c->n : 0, nw = B * (size_t)c->L;
    std::vector<u64> host(pw + nw);
    std::vector<std::pair<const void*, size_t>> ins = {{ct, B * polys * c->L * poly_bytes(c)}, {sk, c->L * poly_bytes(c)}};
    if (expected) ins.push_back({expected, B * poly_bytes(c)});
    if (int e = host_call(c, ins, host.size() * sizeof(u64), host.data(), [&](std::vector<u64*>& dv, u64* o) {
            return exacto_bfv_noise_dev(c, dv[0], polys, dv[1], expected ? dv[2] : nullptr, plain_out ? o : nullptr,
                                        o + pw, B);
        }))
        return e;
    if (pw) std::memcpy(plain_out, host.data(), pw * sizeof(u64));
    if (nw) std::memcpy(noise_out, host.data() + pw, nw * sizeof(u64));
    return 0;
}

extern "C" int exacto_dbfv_noise_dev(exacto_ctx* c, size_t d, const uint64_t* ct, const uint64_t* sk,
                                     uint64_t* noise_out, size_t B) {
    if (int e = check_ctx(c)) return e;
    if (d < 1) return invalid_param("num_digits must be >= 1");
    return noise_batch(c, ct, 2, 2L * c->L * c->n, sk, nullptr, nullptr, noise_out, B * d, d);
}

extern "C" int exacto_dbfv_noise(exacto_ctx* c, size_t d, const uint64_t* ct, const uint64_t* sk, uint64_t* noise_out,
                                 size_t B) {
    if (!c) return invalid_param("null context");
    return host_call(c, {{ct, B * d * 2 * c->L * poly_bytes(c)}, {sk, c->L * poly_bytes(c)}}, B * c->L * sizeof(u64),
                     noise_out, [&](std::vector<u64*>& dv, u64* o) { return exacto_dbfv_noise_dev(c, d, dv[0], dv[1], o, B); });
}
