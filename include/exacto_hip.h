/* exacto_hip.h — C ABI of the MI355X (gfx950) ciphertext-multiplication path.
 *
 * Drop-in boundary for the hot path of RajeshRk18/exacto (Rust).  Each entry point
 * names the reference interface it replaces (paths relative to the reference repo).
 * A Rust caller binds these with an `extern "C"` block.
 *
 * Conventions
 *   - Return value: 0 = Ok; 1..9 = ExactoError variants in declaration order
 *     (src/error.rs:4-31): 1 InvalidParam, 2 DimensionMismatch, 3 ModulusMismatch,
 *     4 InvalidRingDegree, 5 DecryptionError, 6 DecompositionError, 7 LatticeError,
 *     8 MissingKey, 9 NotImplemented; 100 = HIP runtime failure.  The Display text
 *     of the error (same wording as the reference's #[error(...)] strings) is
 *     available from exacto_last_error() on the calling thread.
 *   - Layout: little-endian uint64, ciphertext batches are [batch][poly][limb][coeff]
 *     (BfvCiphertext.c: Vec<RnsPoly>, src/bfv/mod.rs:19-24; RnsPoly.components:
 *     Vec<NttPoly>, src/ring/rns.rs:14-17).  dBFV batches are
 *     [batch][digit][poly][limb][coeff] (DbfvCiphertext.limbs, src/dbfv/ciphertext.rs:10-22).
 *     Relinearisation keys are [key][2][limb][coeff] (RelinKey.keys,
 *     src/bfv/keygen.rs:39-45).  Residues are canonical, in [0, q_i).
 *   - NTT domain: ciphertexts are stored as NttPoly evaluations (src/ring/ntt.rs:11-15)
 *     in THIS library's documented convention (DESIGN.md "NTT convention"): negacyclic
 *     Cooley-Tukey, evaluation k = a(psi^(2*brv(k)+1)), psi = smallest-generator
 *     primitive 2n-th root, stored at position (k mod 16)*(n/16) + k/16 (the order
 *     the device threads hold the values in: contiguous loads and stores).
 *     concrete-ntt's own order is not observable from the reference's tests; all
 *     parity is checked after the inverse transform.
 *   - Functions without suffix take HOST pointers and are synchronous.  The `_dev`
 *     variants take DEVICE pointers (hipMalloc'd on the context's device) and are
 *     asynchronous on the context's stream (exacto_ctx_set_stream); call
 *     exacto_synchronize() before reading results.
 *   - Inputs are read-only (the reference borrows &BfvCiphertext); outputs never alias
 *     inputs unless stated.
 *   - A context is not thread-safe; use one context per host thread (the reference's
 *     types are Send+Sync because they are immutable; here the stream is shared state).
 */
#ifndef EXACTO_HIP_H
#define EXACTO_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct exacto_ctx exacto_ctx;

enum exacto_status {
    EXACTO_OK = 0,
    EXACTO_ERR_INVALID_PARAM = 1,
    EXACTO_ERR_DIMENSION_MISMATCH = 2,
    EXACTO_ERR_MODULUS_MISMATCH = 3,
    EXACTO_ERR_INVALID_RING_DEGREE = 4,
    EXACTO_ERR_DECRYPTION = 5,
    EXACTO_ERR_DECOMPOSITION = 6,
    EXACTO_ERR_LATTICE = 7,
    EXACTO_ERR_MISSING_KEY = 8,
    EXACTO_ERR_NOT_IMPLEMENTED = 9,
    EXACTO_ERR_HIP = 100
};

/* Multiplication algorithm selected for the context (mirrors the dispatcher
 * bfv_mul_no_relin, src/bfv/eval.rs:89-108). */
enum exacto_mul_path {
    EXACTO_PATH_EXACT_RNS = 0,   /* L > 1: exact CRT + exact rounding (eval.rs:113-147) */
    EXACTO_PATH_HPS = 1,         /* L = 1 with aux basis: literal HPS (eval.rs:157-413)  */
    EXACTO_PATH_SCHOOLBOOK = 2   /* L = 1, no aux: exact i128 semantics (eval.rs:416-454) */
};

typedef struct exacto_ctx_info {
    size_t ring_degree;       /* n */
    size_t num_ct_moduli;     /* L */
    size_t num_aux_moduli;    /* user aux basis size */
    size_t num_internal_aux;  /* primes the exact path adds internally (0 for HPS) */
    size_t gadget_digits;     /* G (params/mod.rs:126-140) */
    uint64_t gadget_base;
    uint64_t plain_modulus;
    int mul_path;             /* enum exacto_mul_path */
    int device;
    int ks32_primes;          /* primes of the 31-bit key-switch basis in use (0: limb-wise MAC) */
    int psum_max;             /* dbfv_mul: products per output limb scaled as one sum (0: per product) */
    int ks32_lazy;            /* 1: the resident relinearisation key runs in the lazy 31-bit basis (primes
                                 below 2^30, chosen from the key's own norms at its first use) */
    int ntt_order;            /* storage order of every NTT-domain buffer (keys, ciphertexts): 1 = evaluation k
                                 at position (k mod 16)*n/16 + floor(k/16) (library 0.5 and later); 0 would be
                                 the plain bit-reversed order of 0.4 and earlier, which this library no longer
                                 reads or writes.  Bindings check it (INTEGRATION.md "Format versions") */
    int dbfv_key_switch;      /* the last dbfv_mul's key switch: 1 = the products' digits summed per output
                                 limb in the primary 31-bit basis, 2 = the same in the wide basis, 0 = one key
                                 switch per product, -1 = no dbfv_mul yet */
} exacto_ctx_info;

#define EXACTO_NTT_ORDER 1

/* ---- context: replaces BfvParamsBuilder::build + RnsBasis::new + make_plan ----
 * params/mod.rs:81-124, ring/rns.rs:35-63, ring/ntt.rs:19-29.
 * gadget_base = 0 selects the reference default 2^16 (params/mod.rs:102-108).
 * aux_moduli may be NULL when num_aux == 0.  Errors as the builder: InvalidRingDegree,
 * InvalidParam ("must specify at least one ciphertext modulus", "plaintext modulus must
 * be >= 2", "cannot create NTT plan for n=.., q=.. ..."). */
int exacto_ctx_create(exacto_ctx** out, size_t ring_degree, const uint64_t* ct_moduli,
                      size_t num_ct_moduli, const uint64_t* aux_moduli, size_t num_aux,
                      uint64_t plain_modulus, uint64_t gadget_base, int device);
void exacto_ctx_destroy(exacto_ctx* ctx);
int exacto_ctx_get_info(const exacto_ctx* ctx, exacto_ctx_info* info);
/* Enqueue on an external hipStream_t (e.g. torch.cuda.current_stream().cuda_stream), used as
 * given: NULL is the device's default stream.  A new context starts on a stream of its own. */
int exacto_ctx_set_stream(exacto_ctx* ctx, void* hip_stream);
/* Products per pipeline chunk (workspace = chunk * ~3 MB at n=4096, L=3). 0 = default. */
int exacto_ctx_set_chunk(exacto_ctx* ctx, size_t products_per_chunk);
int exacto_synchronize(exacto_ctx* ctx);

/* ---- relinearisation key: RelinKey (bfv/keygen.rs:39-45, made by gen_relin_key_with_rng
 * keygen.rs:123-162).  rlk = [num_keys][2][L][n], NTT domain.  relinearize uses
 * min(G, num_keys) digits (keyswitch.rs:86-89). */
int exacto_ctx_load_relin_key(exacto_ctx* ctx, const uint64_t* rlk, size_t num_keys);
int exacto_ctx_load_relin_key_dev(exacto_ctx* ctx, const uint64_t* rlk_dev, size_t num_keys);
/* Device pointer of the resident key (for an RCCL broadcast into it), or NULL. */
uint64_t* exacto_ctx_relin_key_buffer(exacto_ctx* ctx, size_t num_keys);

/* ---- NTT engine: concrete_ntt::prime64::Plan::{fwd, inv + normalize} ----
 * NttPoly::from_coeff_poly / to_coeff_poly (ntt.rs:42-67).  polys = [count][n], all mod
 * ct prime `limb`, transformed in place. */
int exacto_ntt_fwd(exacto_ctx* ctx, uint64_t* polys, size_t count, size_t limb);
int exacto_ntt_inv(exacto_ctx* ctx, uint64_t* polys, size_t count, size_t limb);
int exacto_ntt_fwd_dev(exacto_ctx* ctx, uint64_t* polys, size_t count, size_t limb);
int exacto_ntt_inv_dev(exacto_ctx* ctx, uint64_t* polys, size_t count, size_t limb);
/* RnsPoly batches [count][L][n]: RnsPoly::from_coeff_poly per limb (rns.rs:84-105,
 * coefficients already reduced mod q_i) and the per-limb inverse. */
int exacto_rns_fwd_dev(exacto_ctx* ctx, uint64_t* polys, size_t count);
int exacto_rns_inv_dev(exacto_ctx* ctx, uint64_t* polys, size_t count);

/* ---- RNS pointwise ops: RnsPoly::{add,sub,neg,mul,scalar_mul} (rns.rs:159-217 ->
 * NttPoly ops ntt.rs:75-139).  a, b, out = [count][L][n]; out may alias a or b. */
int exacto_rns_add_dev(exacto_ctx* ctx, const uint64_t* a, const uint64_t* b, uint64_t* out, size_t count);
int exacto_rns_sub_dev(exacto_ctx* ctx, const uint64_t* a, const uint64_t* b, uint64_t* out, size_t count);
int exacto_rns_neg_dev(exacto_ctx* ctx, const uint64_t* a, uint64_t* out, size_t count);
int exacto_rns_mul_dev(exacto_ctx* ctx, const uint64_t* a, const uint64_t* b, uint64_t* out, size_t count);
int exacto_rns_scalar_mul_dev(exacto_ctx* ctx, const uint64_t* a, uint64_t scalar, uint64_t* out, size_t count);
/* INTT(a (.) b): RnsPoly::mul followed by the per-limb inverse (to_coeff_poly, ntt.rs:58-67,
 * 119-129) fused into one pass, as the reference's own negacyclic-product test composes them
 * (ntt.rs:181-195).  a, b NTT domain, out coefficient domain; out may alias a or b. */
int exacto_rns_mul_inv_dev(exacto_ctx* ctx, const uint64_t* a, const uint64_t* b, uint64_t* out, size_t count);
/* Negacyclic products of coefficient-domain RnsPolys: to_coeff_poly(from_coeff_poly(a) (.)
 * from_coeff_poly(b)) per limb, the reference's NTT multiplication (ntt.rs:181-195), fused into
 * one kernel at n = 4096 / 8192 (neither operand's evaluations are stored).  out may alias a or b. */
int exacto_rns_polymul_dev(exacto_ctx* ctx, const uint64_t* a, const uint64_t* b, uint64_t* out, size_t count);

/* ---- BFV ciphertext ops (bfv/eval.rs).  Degree-1 ct batches [B][2][L][n]. ---- */
/* bfv_add / bfv_sub / bfv_neg (eval.rs:14-60), batched.  ct1 = [B][polys1][L][n], ct2 =
 * [B][polys2][L][n] -> out = [B][max(polys1, polys2)][L][n]: component i < min is the pointwise
 * sum / difference; the longer operand's further components pass through (eval.rs:21-22), negated
 * when they are ct2's under subtraction (eval.rs:41-42).  out may alias an input only when that
 * input has max(polys1, polys2) components. */
int exacto_bfv_add(exacto_ctx* ctx, const uint64_t* ct1, size_t polys1, const uint64_t* ct2, size_t polys2,
                   uint64_t* out, size_t batch);
int exacto_bfv_add_dev(exacto_ctx* ctx, const uint64_t* ct1, size_t polys1, const uint64_t* ct2, size_t polys2,
                       uint64_t* out, size_t batch);
int exacto_bfv_sub(exacto_ctx* ctx, const uint64_t* ct1, size_t polys1, const uint64_t* ct2, size_t polys2,
                   uint64_t* out, size_t batch);
int exacto_bfv_sub_dev(exacto_ctx* ctx, const uint64_t* ct1, size_t polys1, const uint64_t* ct2, size_t polys2,
                       uint64_t* out, size_t batch);
int exacto_bfv_neg(exacto_ctx* ctx, const uint64_t* ct, size_t polys, uint64_t* out, size_t batch);
int exacto_bfv_neg_dev(exacto_ctx* ctx, const uint64_t* ct, size_t polys, uint64_t* out, size_t batch);

/* bfv_mul_no_relin (eval.rs:89-108): out = [B][3][L][n].  `polys1`/`polys2` are the
 * input ciphertexts' component counts (must be 2: "multiplication requires degree-1
 * ciphertexts"). */
int exacto_bfv_mul_no_relin(exacto_ctx* ctx, const uint64_t* ct1, size_t polys1, const uint64_t* ct2,
                            size_t polys2, uint64_t* out, size_t batch);
int exacto_bfv_mul_no_relin_dev(exacto_ctx* ctx, const uint64_t* ct1, size_t polys1, const uint64_t* ct2,
                                size_t polys2, uint64_t* out, size_t batch);

/* relinearize (bfv/keyswitch.rs:59-101): ct = [B][3][L][n] -> out = [B][2][L][n].
 * polys < 3: cloned, out = [B][polys][L][n] (keyswitch.rs:63-65); polys > 3: InvalidParam
 * "relinearization only supports degree-2 ciphertexts". */
int exacto_relinearize(exacto_ctx* ctx, const uint64_t* ct, size_t polys, uint64_t* out, size_t batch);
int exacto_relinearize_dev(exacto_ctx* ctx, const uint64_t* ct, size_t polys, uint64_t* out, size_t batch);

/* bfv_mul_and_relin (eval.rs:73-82): ct1, ct2 = [B][2][L][n] -> out = [B][2][L][n]. */
int exacto_bfv_mul_and_relin(exacto_ctx* ctx, const uint64_t* ct1, const uint64_t* ct2, uint64_t* out,
                             size_t batch);
int exacto_bfv_mul_and_relin_dev(exacto_ctx* ctx, const uint64_t* ct1, const uint64_t* ct2,
                                 uint64_t* out, size_t batch);

/* Squares: a ciphertext times itself on a one-operand pipeline (the input transformed, lifted and
 * forward-transformed once instead of twice; the tensor loads each polynomial once and forms c1 as one
 * doubled product).  Bit for bit exacto_bfv_mul_no_relin(ct, polys, ct, polys) and
 * exacto_bfv_mul_and_relin(ct, ct), on every multiplication path, with the same error codes and
 * messages (polys != 2, no key, a deferred parameter error).  ct = [B][2][L][n]; out = [B][3][L][n]
 * (no_relin) or [B][2][L][n]; out must not overlap ct (InvalidParam); batch == 0 returns 0. */
int exacto_bfv_square_no_relin(exacto_ctx* ctx, const uint64_t* ct, size_t polys, uint64_t* out, size_t batch);
int exacto_bfv_square_no_relin_dev(exacto_ctx* ctx, const uint64_t* ct, size_t polys, uint64_t* out, size_t batch);
int exacto_bfv_square_and_relin(exacto_ctx* ctx, const uint64_t* ct, uint64_t* out, size_t batch);
int exacto_bfv_square_and_relin_dev(exacto_ctx* ctx, const uint64_t* ct, uint64_t* out, size_t batch);
/* exacto_eval_poly's baby steps x^i = x^(i/2) x^(i/2) (even i) run exacto_bfv_square_and_relin_dev (the
 * default, on != 0) or the two-operand call (on == 0: for A/B timing; the results are the same bits). */
int exacto_ctx_set_square_hook(exacto_ctx* ctx, int on);

/* gadget_decompose (keyswitch.rs:11-52) of coefficient-domain RNS polynomials [B][L][n]
 * (CRT value mod Q, extension semantics when Q >= 2^64) -> digits [B][G'][L][n] as
 * residues mod q_i, G' = min(G, num_digits). */
int exacto_gadget_decompose_dev(exacto_ctx* ctx, const uint64_t* coeffs, uint64_t* digits,
                                size_t batch, size_t num_digits);

/* ---- dBFV: dbfv_mul (dbfv/eval.rs:82-149) + reduce (dbfv/reduction.rs:15-60) ----
 * a, b, out = [B][d][2][L][n]; base/plain as DbfvParams (params/mod.rs:144-193,
 * plain_modulus 0 == 2^64).  depth_a/depth_b = mul_depth of each input (NULL = 0);
 * depth_out receives mul_depth of each output (NULL allowed).  Errors:
 * "multiplication requires d-limb ciphertexts" is not reachable through fixed shapes;
 * depth > 1 -> NotImplemented "chained dBFV multiplication requires ciphertext-level
 * lattice reduction (paper §4.6.2)". */
int exacto_dbfv_mul(exacto_ctx* ctx, size_t d, uint64_t base, uint64_t dbfv_plain_modulus,
                    const uint64_t* a, const uint64_t* b, uint64_t* out, size_t batch,
                    const uint32_t* depth_a, const uint32_t* depth_b, uint32_t* depth_out);
int exacto_dbfv_mul_dev(exacto_ctx* ctx, size_t d, uint64_t base, uint64_t dbfv_plain_modulus,
                        const uint64_t* a, const uint64_t* b, uint64_t* out, size_t batch,
                        const uint32_t* depth_a, const uint32_t* depth_b, uint32_t* depth_out);

/* dbfv_mul(a, a): a, out = [B][d][2][L][n], bit for bit exacto_dbfv_mul(a, a, depth_a, depth_a) with the
 * same errors and depth_out.  The digit-pair products (i, j) and (j, i) are one ciphertext, so
 * d (d + 1) / 2 of the d^2 products are formed and the operand is extended once; every output limb sums
 * the same terms (a shared product counted for both of its ordered pairs), so the key switch taken
 * (exacto_ctx_info.dbfv_key_switch) is the two-operand call's.  out must not overlap a. */
int exacto_dbfv_square(exacto_ctx* ctx, size_t d, uint64_t base, uint64_t dbfv_plain_modulus, const uint64_t* a,
                       uint64_t* out, size_t batch, const uint32_t* depth_a, uint32_t* depth_out);
int exacto_dbfv_square_dev(exacto_ctx* ctx, size_t d, uint64_t base, uint64_t dbfv_plain_modulus, const uint64_t* a,
                           uint64_t* out, size_t batch, const uint32_t* depth_a, uint32_t* depth_out);

/* The products and per-limb sums exacto_dbfv_mul (symmetric = 0) or exacto_dbfv_square (symmetric != 0)
 * forms for the d output limbs, pure host code (no context): pairs = [npairs][2] digit indices (i, j) (the
 * symmetric plan: i <= j only), term_start = [d + 1], terms = [nterms][2] = (index into pairs, coefficient),
 * limb k summing terms term_start[k] .. term_start[k + 1] - 1.  *npairs / *nterms receive the counts; a
 * NULL or too small pairs / terms buffer (capacities in entries) is left unwritten, term_start may be NULL.
 * Errors: those of DbfvParams::new. */
int exacto_dbfv_mul_plan(size_t d, uint64_t base, uint64_t dbfv_plain_modulus, int symmetric, int32_t* pairs,
                         size_t pair_cap, size_t* npairs, int32_t* term_start, int64_t* terms, size_t term_cap,
                         size_t* nterms);

/* One GPU's share of a dbfv_mul whose d output limbs are split across GPUs (the d^2 digit-pair
 * products of dbfv/eval.rs:109-122 partitioned by output limb k = i + j, so no cross-GPU sum is
 * needed): only the output limbs limbs[0..nlimbs) (host array, distinct, < d) are computed, out =
 * [B][nlimbs][2][L][n] with slot s holding limb limbs[s] exactly as exacto_dbfv_mul computes it
 * (including the reduce folding of limbs >= d, reduction.rs:34-52).  The caller gathers the slots of
 * all GPUs (exacto_rccl_allgather_u64) into [B][d][2][L][n].  Inputs at mul_depth 0. */
int exacto_dbfv_mul_limbs(exacto_ctx* ctx, size_t d, uint64_t base, uint64_t dbfv_plain_modulus,
                          const uint64_t* a, const uint64_t* b, uint64_t* out, size_t batch, const uint32_t* limbs,
                          size_t nlimbs);
int exacto_dbfv_mul_limbs_dev(exacto_ctx* ctx, size_t d, uint64_t base, uint64_t dbfv_plain_modulus,
                              const uint64_t* a, const uint64_t* b, uint64_t* out, size_t batch, const uint32_t* limbs,
                              size_t nlimbs);

/* Sums of ciphertext products with one key switch per sum (the ciphertext x ciphertext counterpart of
 * exacto_bfv_inner_product: dot products, matrix-vector products, convolutions).  For every batch
 * item and output slot s,
 *     out[item][s] = sum over the terms t with slot[t] == s of
 *                    bfv_mul_and_relin(a[item][ia[t]], b[item][ib[t]], rlk)      (eval.rs:73-82)
 * added with bfv_add (eval.rs:14-32): bit for bit what exacto_bfv_mul_and_relin per product and
 * exacto_bfv_add per term give, but the sums are taken before the key switch and the forward
 * transform, so each output pays them once (relinearisation is linear mod q in the gadget digits).
 * a = [B][na][2][L][n], b = [B][nb][2][L][n], out = [B][nslots][2][L][n], NTT domain.  ia, ib, slot:
 * HOST arrays of nterms entries, for the _dev form too.  a and b may be the same buffer (sums of
 * squares); a pair listed twice counts twice.  out must not overlap an input and is 16-byte aligned.
 * The resident relinearisation key and min(G, num_keys) digits are used as by
 * exacto_bfv_mul_and_relin; with no key, and on a context with a deferred parameter error, the error
 * is that function's.  InvalidParam: nterms == 0, an index >= na or >= nb, a slot >= nslots, an
 * output slot with no term.  batch == 0 returns 0.
 * A slot with more products than one key switch lifts (exacto_bfv_mul_sum_info) is computed in groups
 * whose coefficient-domain results are added before the slot's forward transform.  Contexts without
 * the summed key switch (no 31-bit basis, gadget base above 2^16, small n, HPS, schoolbook) take one
 * key switch per product and sum the results.
 * The _dev form is asynchronous on the context's stream; a call whose term lists and shape differ
 * from the previous call's may wait for the stream once before it uploads its tables. */
int exacto_bfv_mul_sum(exacto_ctx* ctx, const uint64_t* a, size_t na, const uint64_t* b, size_t nb,
                       const uint32_t* ia, const uint32_t* ib, const uint32_t* slot, size_t nterms, size_t nslots,
                       uint64_t* out, size_t batch);
int exacto_bfv_mul_sum_dev(exacto_ctx* ctx, const uint64_t* a, size_t na, const uint64_t* b, size_t nb,
                           const uint32_t* ia, const uint32_t* ib, const uint32_t* slot, size_t nterms, size_t nslots,
                           uint64_t* out, size_t batch);
/* At most max_products products of one output are key-switched as one sum (0: the context's own
 * limit).  Results do not depend on it. */
int exacto_ctx_set_mul_sum_group(exacto_ctx* ctx, size_t max_products);
/* group_max: how many products of one output a bfv_mul_sum key-switches as one sum, with the resident
 * key, the basis in use and the limit set above (1 where the context has no summed key switch).
 * last_mode: the last bfv_mul_sum's key switch in the codes of exacto_ctx_info's dbfv_key_switch (1 =
 * summed in the primary 31-bit basis, 2 = summed in the wide basis, 0 = one per product), -1 = none
 * yet.  Either pointer may be null. */
int exacto_bfv_mul_sum_info(exacto_ctx* ctx, size_t* group_max, int* last_mode);

/* dBFV multiplication chain, device-resident (paper_repro.rs:203-236 guard-bypass semantics;
 * bfv_host.rs:258-288 without the bootstrap): out = (((x*y)*y)...*y), `depth` dbfv_mul steps,
 * each with both inputs' mul_depth reset to 0, intermediates kept in context-owned HBM buffers.
 * x, y, out = [B][d][2][L][n]; depth 0 copies x.  Errors as exacto_dbfv_mul. */
int exacto_dbfv_mul_chain(exacto_ctx* ctx, size_t d, uint64_t base, uint64_t dbfv_plain_modulus,
                          const uint64_t* x, const uint64_t* y, uint64_t* out, size_t batch, size_t depth);
int exacto_dbfv_mul_chain_dev(exacto_ctx* ctx, size_t d, uint64_t base, uint64_t dbfv_plain_modulus,
                              const uint64_t* x, const uint64_t* y, uint64_t* out, size_t batch, size_t depth);

/* ---- decryption ----
 * BFV decrypt (bfv/encrypt.rs:111-178), batched: phase = sum_k c_k * s^k in the NTT domain,
 * INTT, x = CRT(phase) in [0, Q), m = floor((x*p + floor(Q/2)) / Q) mod p, exact for any Q.
 * ct = [B][polys][L][n] (polys >= 1), sk = secret key [L][n] (NTT domain), out = [B][n] mod p.
 * L >= 2 needs p below the first internal auxiliary prime (~2^60), else NotImplemented. */
int exacto_bfv_decrypt(exacto_ctx* ctx, const uint64_t* ct, size_t polys, const uint64_t* sk, uint64_t* out,
                       size_t batch);
int exacto_bfv_decrypt_dev(exacto_ctx* ctx, const uint64_t* ct, size_t polys, const uint64_t* sk,
                           uint64_t* out, size_t batch);
/* dBFV decrypt (dbfv/decrypt.rs:20-43): each limb decrypted mod t (the context's plain modulus),
 * coefficient 0 of every limb centred and recomposed: sum centred(mu_i) * base^i mod p (i128,
 * p = 0 -> mod 2^64).  ct = [B][d][2][L][n], out = [B]. */
int exacto_dbfv_decrypt(exacto_ctx* ctx, size_t d, uint64_t base, uint64_t dbfv_plain_modulus,
                        const uint64_t* ct, const uint64_t* sk, uint64_t* out, size_t batch);
int exacto_dbfv_decrypt_dev(exacto_ctx* ctx, size_t d, uint64_t base, uint64_t dbfv_plain_modulus,
                            const uint64_t* ct, const uint64_t* sk, uint64_t* out, size_t batch);
/* dbfv_decrypt_poly (dbfv/decrypt.rs:48-79): the same recomposition for every coefficient,
 * out = [B][n]; plain modulus 0 -> InvalidParam "polynomial dBFV decrypt requires finite
 * plain_modulus (plain_modulus=0 is scalar-only)". */
int exacto_dbfv_decrypt_poly(exacto_ctx* ctx, size_t d, uint64_t base, uint64_t dbfv_plain_modulus,
                             const uint64_t* ct, const uint64_t* sk, uint64_t* out, size_t batch);
int exacto_dbfv_decrypt_poly_dev(exacto_ctx* ctx, size_t d, uint64_t base, uint64_t dbfv_plain_modulus,
                                 const uint64_t* ct, const uint64_t* sk, uint64_t* out, size_t batch);

/* ---- noise measurement (paper_repro.rs:238-281 bfv_noise_inf, max_limb_noise) ----
 * With Q = prod q_i, p the context's plain modulus, Delta = floor(Q / p) and x_j in [0, Q) the phase
 * exacto_bfv_decrypt rounds:  e_j = (x_j - m_j Delta) mod Q,  noise = max_j min(e_j, Q - e_j),
 * where m_j is the decrypted coefficient (expected == NULL) or expected[j] mod p.  Noise against the
 * decrypted value never exceeds about Delta / 2 + p; to see it past the point where decryption
 * fails, say in `expected` what the plaintext should be.
 * At L = 1 this is bfv_noise_inf literally.  For L >= 2 it is the same formula over the full Q (the
 * extension semantics of the multi-prime configurations; the reference looks at moduli[0] only).
 * The result is exact: noise_out = [B][L] little-endian 64-bit words (Q < 2^(64 L)), the same from
 * run to run.  ct = [B][polys][L][n], sk = [L][n] (NTT domain), expected = [B][n] or NULL,
 * plain_out = [B][n] or NULL: the decrypted m of exacto_bfv_decrypt, a free by-product.
 * polys < 1 -> InvalidParam as exacto_bfv_decrypt; batch = 0 returns 0.  L >= 2 with p not below the
 * first internal auxiliary prime is NotImplemented only when the rounding is computed (expected ==
 * NULL or plain_out != NULL).  The _dev form enqueues on the context's stream and does not wait (but
 * for the upload of Delta's residues on a context's first use of them, as in exacto_encrypt_sk_dev). */
int exacto_bfv_noise(exacto_ctx* ctx, const uint64_t* ct, size_t polys, const uint64_t* sk,
                     const uint64_t* expected, uint64_t* plain_out, uint64_t* noise_out, size_t batch);
int exacto_bfv_noise_dev(exacto_ctx* ctx, const uint64_t* ct, size_t polys, const uint64_t* sk,
                         const uint64_t* expected, uint64_t* plain_out, uint64_t* noise_out, size_t batch);
/* max_limb_noise: the maximum over the d limbs of each dBFV ciphertext, against each limb's decrypted
 * value.  ct = [B][d][2][L][n], noise_out = [B][L].  The per-limb values are exacto_bfv_noise with
 * polys = 2 and batch B * d on the same memory.  d = 0 -> InvalidParam as exacto_dbfv_decrypt. */
int exacto_dbfv_noise(exacto_ctx* ctx, size_t d, const uint64_t* ct, const uint64_t* sk, uint64_t* noise_out,
                      size_t batch);
int exacto_dbfv_noise_dev(exacto_ctx* ctx, size_t d, const uint64_t* ct, const uint64_t* sk, uint64_t* noise_out,
                          size_t batch);

/* ---- modulus switching: drop ciphertext primes (bfv/modswitch.rs mod_switch_drop_prime) ----
 * A ciphertext "at level l" (1 <= l <= L) is [B][polys][l][n] over the context's first l primes, NTT
 * domain, the library's storage order.  The per-prime tables depend only on (n, q_i), so a level-l
 * ciphertext is also, bit for bit, a ciphertext of a context created with moduli[:l]: decryption, noise
 * measurement and further products happen there (with a relinearisation key generated from sk[:l]: the
 * gadget digits depend on Q).
 * One drop l -> l - 1, with q = q_{l-1}, Q' = q_0 ... q_{l-2} and x_j in [0, Q' q) a coefficient's CRT value:
 *   EXACTO_MODSWITCH_ROUND      y_j = floor((2 x_j + q) / (2 q)) mod Q' = round(x_j / q) (q is odd: no ties);
 *                               limb i = (c_i - delta) q^-1 mod q_i with delta the centred residue of
 *                               x_j mod q.  The noise is divided by q (plus at most p + n / 2 + 2 for a
 *                               ternary secret).
 *   EXACTO_MODSWITCH_REFERENCE  drop_last_rns_prime literally (modswitch.rs:37-87): limb i =
 *                               c_i - NTT_{q_i}(u mod q_i) with u = INTT_q(c_{l-1}) in [0, q), uncentred and
 *                               unscaled.  The reference calls this "simplified"; its output does not
 *                               decrypt under the smaller modulus.  Kept for the bit-exact seam.
 * limbs_in -> limbs_out is limbs_in - limbs_out single drops from the top, each as above (not one
 * rounding by the product of the dropped primes).  ct = [B][polys][limbs_in][n], out =
 * [B][polys][limbs_out][n], polys >= 1 (a degree-2 ciphertext is switched like any other).  A dBFV
 * ciphertext [B][d][polys][l][n] is this call with batch B * d.
 * InvalidParam, before any launch: limbs_in <= 1 ("cannot drop prime: only one modulus remaining"),
 * limbs_in > L, limbs_out == 0, limbs_out >= limbs_in, polys == 0, an unknown mode, out overlapping
 * ct, a _dev buffer that is not 16-byte aligned.  batch = 0 returns 0.  The _dev form is asynchronous
 * on the context's stream (intermediate levels of several drops live in a context-owned workspace,
 * chunked by exacto_ctx_set_chunk). */
enum exacto_mod_switch_mode {
    EXACTO_MODSWITCH_ROUND = 0,
    EXACTO_MODSWITCH_REFERENCE = 1
};
int exacto_bfv_mod_switch(exacto_ctx* ctx, const uint64_t* ct, size_t polys, size_t limbs_in, size_t limbs_out,
                          int mode, uint64_t* out, size_t batch);
int exacto_bfv_mod_switch_dev(exacto_ctx* ctx, const uint64_t* ct, size_t polys, size_t limbs_in, size_t limbs_out,
                              int mode, uint64_t* out, size_t batch);

/* ---- dBFV beyond the product: encryption, limb-wise operations, maps between digit vectors ----
 * All on the dBFV layout [B][d][polys][L][n].  DbfvCiphertext.degree is not carried over this
 * ABI; a binding keeps it (INTEGRATION.md gives the rule of each function).  Depth arrays as in
 * exacto_dbfv_mul: host uint32_t[B], NULL = 0, depth_out may be NULL. */

/* dbfv_encrypt_sk_with_rng / dbfv_encrypt_with_rng (dbfv/encrypt.rs:27-35, 73-81, 105-118):
 * values [B] scalars (DEVICE pointer for _dev), each reduced mod p (taken as is for p = 2^64),
 * decomposed into d base-b digits (decomposition.rs:8-16, excess digits dropped); limb k of item b
 * encrypts the constant polynomial of digit k.  ct = [B][d][2][L][n].  sk / pk / sigma / key /
 * stream as exacto_encrypt_sk / exacto_encrypt_pk, and the randomness is theirs: limb k of item b
 * is bit for bit item b*d + k of exacto_encrypt_sk/pk called with the same (key, stream, sigma) on
 * the [B*d][n] digit plaintexts.  Errors: those of DbfvParams::new, then InvalidParam "dBFV base
 * {b} must be <= BFV plaintext modulus {t}" (encrypt.rs:152-159). */
int exacto_dbfv_encrypt_sk(exacto_ctx* ctx, size_t d, uint64_t base, uint64_t dbfv_plain_modulus,
                           const uint64_t* values, const uint64_t* sk, double sigma, const uint64_t* key,
                           uint64_t stream, uint64_t* ct, size_t batch);
int exacto_dbfv_encrypt_sk_dev(exacto_ctx* ctx, size_t d, uint64_t base, uint64_t dbfv_plain_modulus,
                               const uint64_t* values, const uint64_t* sk, double sigma, const uint64_t* key,
                               uint64_t stream, uint64_t* ct, size_t batch);
int exacto_dbfv_encrypt_pk(exacto_ctx* ctx, size_t d, uint64_t base, uint64_t dbfv_plain_modulus,
                           const uint64_t* values, const uint64_t* pk, double sigma, const uint64_t* key,
                           uint64_t stream, uint64_t* ct, size_t batch);
int exacto_dbfv_encrypt_pk_dev(exacto_ctx* ctx, size_t d, uint64_t base, uint64_t dbfv_plain_modulus,
                               const uint64_t* values, const uint64_t* pk, double sigma, const uint64_t* key,
                               uint64_t stream, uint64_t* ct, size_t batch);
/* dbfv_encrypt_poly_sk_with_rng / dbfv_encrypt_poly_with_rng (dbfv/encrypt.rs:51-60, 94-103,
 * 120-141): pt [B][n] coefficients, each reduced mod p; limb k encrypts the polynomial of the k-th
 * digits.  p = 2^64 is InvalidParam "polynomial dBFV plaintext requires finite plain_modulus
 * (plain_modulus=0 is scalar-only)". */
int exacto_dbfv_encrypt_poly_sk(exacto_ctx* ctx, size_t d, uint64_t base, uint64_t dbfv_plain_modulus,
                                const uint64_t* pt, const uint64_t* sk, double sigma, const uint64_t* key,
                                uint64_t stream, uint64_t* ct, size_t batch);
int exacto_dbfv_encrypt_poly_sk_dev(exacto_ctx* ctx, size_t d, uint64_t base, uint64_t dbfv_plain_modulus,
                                    const uint64_t* pt, const uint64_t* sk, double sigma, const uint64_t* key,
                                    uint64_t stream, uint64_t* ct, size_t batch);
int exacto_dbfv_encrypt_poly_pk(exacto_ctx* ctx, size_t d, uint64_t base, uint64_t dbfv_plain_modulus,
                                const uint64_t* pt, const uint64_t* pk, double sigma, const uint64_t* key,
                                uint64_t stream, uint64_t* ct, size_t batch);
int exacto_dbfv_encrypt_poly_pk_dev(exacto_ctx* ctx, size_t d, uint64_t base, uint64_t dbfv_plain_modulus,
                                    const uint64_t* pt, const uint64_t* pk, double sigma, const uint64_t* key,
                                    uint64_t stream, uint64_t* ct, size_t batch);

/* dbfv_add / dbfv_sub (dbfv/eval.rs:11-58): a = [B][d1][polys1][L][n], b = [B][d2][polys2][L][n] ->
 * out = [B][d1][max(polys1, polys2)][L][n], every limb by the rule of exacto_bfv_add / exacto_bfv_sub
 * (aliasing included).  d1 != d2 is DimensionMismatch {expected d1, got d2} (eval.rs:15-20);
 * depth_out = max(depth_a, depth_b).
 * dbfv_neg (eval.rs:61-71): ct, out = [B][d][polys][L][n].
 * dbfv_relinearize (dbfv/keyswitch.rs:9-23): exacto_relinearize on every limb with the resident key:
 * [B][d][3][L][n] -> [B][d][2][L][n]; polys < 3 cloned; polys > 3 the reference's error.
 * dbfv_apply_automorphism (dbfv/advanced.rs:15-29): exacto_bfv_apply_automorphism on every limb. */
int exacto_dbfv_add(exacto_ctx* ctx, const uint64_t* a, size_t d1, size_t polys1, const uint64_t* b, size_t d2,
                    size_t polys2, uint64_t* out, size_t batch, const uint32_t* depth_a, const uint32_t* depth_b,
                    uint32_t* depth_out);
int exacto_dbfv_add_dev(exacto_ctx* ctx, const uint64_t* a, size_t d1, size_t polys1, const uint64_t* b, size_t d2,
                        size_t polys2, uint64_t* out, size_t batch, const uint32_t* depth_a,
                        const uint32_t* depth_b, uint32_t* depth_out);
int exacto_dbfv_sub(exacto_ctx* ctx, const uint64_t* a, size_t d1, size_t polys1, const uint64_t* b, size_t d2,
                    size_t polys2, uint64_t* out, size_t batch, const uint32_t* depth_a, const uint32_t* depth_b,
                    uint32_t* depth_out);
int exacto_dbfv_sub_dev(exacto_ctx* ctx, const uint64_t* a, size_t d1, size_t polys1, const uint64_t* b, size_t d2,
                        size_t polys2, uint64_t* out, size_t batch, const uint32_t* depth_a,
                        const uint32_t* depth_b, uint32_t* depth_out);
int exacto_dbfv_neg(exacto_ctx* ctx, const uint64_t* ct, size_t d, size_t polys, uint64_t* out, size_t batch);
int exacto_dbfv_neg_dev(exacto_ctx* ctx, const uint64_t* ct, size_t d, size_t polys, uint64_t* out, size_t batch);
int exacto_dbfv_relinearize(exacto_ctx* ctx, const uint64_t* ct, size_t d, size_t polys, uint64_t* out,
                            size_t batch);
int exacto_dbfv_relinearize_dev(exacto_ctx* ctx, const uint64_t* ct, size_t d, size_t polys, uint64_t* out,
                                size_t batch);
int exacto_dbfv_apply_automorphism(exacto_ctx* ctx, const uint64_t* ct, size_t d, size_t polys, uint64_t element,
                                   const uint64_t* gk, size_t num_keys, uint64_t* out, size_t batch);
int exacto_dbfv_apply_automorphism_dev(exacto_ctx* ctx, const uint64_t* ct, size_t d, size_t polys,
                                       uint64_t element, const uint64_t* gk, size_t num_keys, uint64_t* out,
                                       size_t batch);

/* Linear maps between digit vectors, the common core of dbfv_div_by_base and dbfv_change_base
 * (dbfv/advanced.rs:36-160): out[b][j] = sum_i s_ji * in[b][i] per component, limb and slot, with
 * s_ji = (matrix[j][i] mod t) mod q_l: the reference's bfv_scalar_plain_mul (advanced.rs:162-171)
 * followed by bfv_add, in canonical residues.  matrix = [d_out][d_in] HOST u64 (also for _dev);
 * in = [B][d_in][polys][L][n], out = [B][d_out][polys][L][n]; a row of zeros gives the zero
 * ciphertext (the reference's bfv_sub(x, x)).  One kernel launch, no intermediate ciphertexts.
 * out must not overlap in, and _dev buffers are 16-byte aligned (InvalidParam otherwise).  A call
 * with the matrix of the previous call reuses the resident scalar table and stays asynchronous; a
 * new matrix waits for the context's stream once before it is uploaded. */
int exacto_dbfv_linear_map(exacto_ctx* ctx, size_t d_in, size_t d_out, size_t polys, const uint64_t* matrix,
                           const uint64_t* in, uint64_t* out, size_t batch);
int exacto_dbfv_linear_map_dev(exacto_ctx* ctx, size_t d_in, size_t d_out, size_t polys, const uint64_t* matrix,
                               const uint64_t* in, uint64_t* out, size_t batch);
/* dbfv_change_base (advanced.rs:99-160): in = [B][d][2][L][n] -> out = [B][new_d][2][L][n] in base
 * new_base.  exacto_dbfv_change_base_matrix is the transform alone (advanced.rs:119-130), pure host
 * code: out[j][i] = digit j of (base^i mod p) in base new_base, out = [new_d][d].  Errors (both):
 * those of DbfvParams::new(base, d, plain), "new base must be >= 2", "new_num_digits must be >= 1",
 * then those of DbfvParams::new(new_base, new_d, plain). */
int exacto_dbfv_change_base_matrix(size_t d, uint64_t base, uint64_t dbfv_plain_modulus, uint64_t new_base,
                                   size_t new_d, uint64_t* out);
int exacto_dbfv_change_base(exacto_ctx* ctx, size_t d, uint64_t base, uint64_t dbfv_plain_modulus,
                            uint64_t new_base, size_t new_d, const uint64_t* in, uint64_t* out, size_t batch);
int exacto_dbfv_change_base_dev(exacto_ctx* ctx, size_t d, uint64_t base, uint64_t dbfv_plain_modulus,
                                uint64_t new_base, size_t new_d, const uint64_t* in, uint64_t* out, size_t batch);
/* dbfv_div_by_base (advanced.rs:36-93): in, out = [B][d][2][L][n]; limb 0 = base^-1 (mod t) * in_0 +
 * in_1, limb i = in_{i+1}, last limb zero; *new_plain = p / base (new_plain may be NULL).  Errors:
 * "base not invertible modulo BFV plaintext modulus", "plaintext modulus {p} is not divisible by
 * base {b}" (p printed as 18446744073709551616 for 2^64). */
int exacto_dbfv_div_by_base(exacto_ctx* ctx, size_t d, uint64_t base, uint64_t dbfv_plain_modulus,
                            const uint64_t* in, uint64_t* out, size_t batch, uint64_t* new_plain);
int exacto_dbfv_div_by_base_dev(exacto_ctx* ctx, size_t d, uint64_t base, uint64_t dbfv_plain_modulus,
                                const uint64_t* in, uint64_t* out, size_t batch, uint64_t* new_plain);

/* ---- diagnostics ---- */
/* Copies the last error message of this thread (NUL-terminated); returns its length. */
/* ---- key generation and encryption on the device ----
 * keygen.rs:64-162 and encrypt.rs:29-106, 181-229.  Polynomials are sampled exactly as the
 * reference's samplers define them (sampling/uniform.rs, sampling/gaussian.rs: values of a CoeffPoly
 * modulo the FIRST ciphertext prime, then reduced modulo every q_i), from a ChaCha20 stream in
 * counter mode (the reference's ChaCha20Rng primitive; the word stream is this library's own):
 * `key` = 4 words (256 bits, HOST pointer, also for _dev), `stream` = 64-bit nonce.  Equal
 * (key, stream) reproduce the same output.  sigma: Gaussian width (BfvParams.sigma, 3.2 default).
 * sk [L][n], pk [2][L][n], rlk [num_keys][2][L][n], ct [B][2][L][n]: NTT domain.  pt [B][n]:
 * plaintext coefficients (CoeffPoly mod p). */
int exacto_gen_secret_key(exacto_ctx* ctx, const uint64_t* key, uint64_t stream, uint64_t* sk);
int exacto_gen_secret_key_dev(exacto_ctx* ctx, const uint64_t* key, uint64_t stream, uint64_t* sk);
int exacto_gen_public_key(exacto_ctx* ctx, const uint64_t* sk, double sigma, const uint64_t* key,
                          uint64_t stream, uint64_t* pk);
int exacto_gen_public_key_dev(exacto_ctx* ctx, const uint64_t* sk, double sigma, const uint64_t* key,
                              uint64_t stream, uint64_t* pk);
/* rlk == NULL: the key is generated straight into the context's resident relinearisation key
 * (replaces exacto_ctx_load_relin_key: no host build, no upload). */
int exacto_gen_relin_key(exacto_ctx* ctx, const uint64_t* sk, double sigma, const uint64_t* key,
                         uint64_t stream, size_t num_keys, uint64_t* rlk);
int exacto_gen_relin_key_dev(exacto_ctx* ctx, const uint64_t* sk, double sigma, const uint64_t* key,
                             uint64_t stream, size_t num_keys, uint64_t* rlk);
int exacto_encrypt_sk(exacto_ctx* ctx, const uint64_t* pt, const uint64_t* sk, double sigma, const uint64_t* key,
                      uint64_t stream, uint64_t* ct, size_t batch);
int exacto_encrypt_sk_dev(exacto_ctx* ctx, const uint64_t* pt, const uint64_t* sk, double sigma,
                          const uint64_t* key, uint64_t stream, uint64_t* ct, size_t batch);
int exacto_encrypt_pk(exacto_ctx* ctx, const uint64_t* pt, const uint64_t* pk, double sigma, const uint64_t* key,
                      uint64_t stream, uint64_t* ct, size_t batch);
int exacto_encrypt_pk_dev(exacto_ctx* ctx, const uint64_t* pt, const uint64_t* pk, double sigma,
                          const uint64_t* key, uint64_t stream, uint64_t* ct, size_t batch);

/* ---- Galois automorphisms ----
 * gen_galois_key_with_rng (keygen.rs:171-209): key-switch key from s(X^element) to s(X), gk =
 * [num_keys][2][L][n]; s(X^element) is formed from limb 0 of s as the reference does
 * (keygen.rs:179-182).  bfv_apply_automorphism (eval.rs:512-561), batched: ct/out [B][2][L][n],
 * polys must be 2 ("automorphism requires degree-1 ciphertext"); min(G, num_keys) digits are
 * used; an empty key is InvalidParam (the reference panics on it). */
int exacto_gen_galois_key(exacto_ctx* ctx, const uint64_t* sk, uint64_t element, double sigma,
                          const uint64_t* key, uint64_t stream, size_t num_keys, uint64_t* gk);
int exacto_gen_galois_key_dev(exacto_ctx* ctx, const uint64_t* sk, uint64_t element, double sigma,
                              const uint64_t* key, uint64_t stream, size_t num_keys, uint64_t* gk);
int exacto_bfv_apply_automorphism(exacto_ctx* ctx, const uint64_t* ct, size_t polys, uint64_t element,
                                  const uint64_t* gk, size_t num_keys, uint64_t* out, size_t batch);
int exacto_bfv_apply_automorphism_dev(exacto_ctx* ctx, const uint64_t* ct, size_t polys, uint64_t element,
                                      const uint64_t* gk, size_t num_keys, uint64_t* out, size_t batch);

/* ---- SIMD batching: slot encoding mod t, row rotations (replaces bfv/encoding.rs) ----
 * The reference's encode_simd is coefficient packing ("not true SIMD", encoding.rs:30-31); this is the
 * CRT batching it names.  It needs a prime plaintext modulus t == 1 (mod 2n) with 16 <= n <= 16384 and
 * t < 2^32.  zeta = x^((t-1)/2n) for the smallest x >= 2 for which it has order 2n (the library's root
 * rule applied to t).  A slot vector values[n] is a 2 x n/2 matrix, row 0 = values[0 .. n/2), row 1 =
 * values[n/2 .. n).  With e_i = 3^i mod 2n, the plaintext m(X) mod t that encodes `values` satisfies
 *     m(zeta^e_i) = values[i],   m(zeta^(2n - e_i)) = values[n/2 + i]     (0 <= i < n/2).
 * So: the negacyclic product of plaintexts is the slot-wise product; sigma_{3^k} rotates both rows left
 * by k; sigma_{2n-1} swaps the rows; the trace over exacto_required_trace_elements(n) leaves the sum
 * of all slots in every slot.
 * pt = [B][n] is exactly what exacto_encrypt_sk / exacto_bfv_plain_mul / exacto_bfv_plain_add take and
 * what exacto_bfv_decrypt returns.  The transforms are one 32-bit kernel per direction (batch.hip).
 * Errors come from a context's first batching call, never from exacto_ctx_create, and the same error
 * is returned by every later batching call; every other entry point of such a context works as before:
 *   InvalidParam    "batching requires a prime plaintext modulus t ≡ 1 (mod 2n), got t={t}, n={n}"
 *   NotImplemented  "batching for plaintext moduli >= 2^32"   (a valid t >= 2^32)
 * The tables (twiddles mod t, n^-1, the slot permutation) are built on the host and uploaded at that
 * first call, which waits for the context's stream once; later calls do not.
 *
 * exacto_batch_info: 0 when the context batches (building the tables if need be), else the error;
 *   *root (may be NULL) receives zeta.
 * exacto_batch_encode: values [B][n] -> pt [B][n].  The host form rejects the first value >= t as
 *   encode_simd does (encoding.rs:40-46): InvalidParam "plaintext {v} >= plain_modulus {t}".  The _dev
 *   form cannot look at the values without waiting: it REDUCES every value mod t in the kernel.
 * exacto_batch_decode: pt [B][n] -> values [B][n]; coefficients are reduced mod t in both forms.
 * Both: out == in (in place) is allowed, any other overlap is InvalidParam; _dev buffers must be 16-byte
 * aligned (InvalidParam); batch == 0 returns 0. */
int exacto_batch_info(exacto_ctx* ctx, uint64_t* root);
int exacto_batch_encode(exacto_ctx* ctx, const uint64_t* values, uint64_t* pt, size_t batch);
int exacto_batch_encode_dev(exacto_ctx* ctx, const uint64_t* values, uint64_t* pt, size_t batch);
int exacto_batch_decode(exacto_ctx* ctx, const uint64_t* pt, uint64_t* values, size_t batch);
int exacto_batch_decode_dev(exacto_ctx* ctx, const uint64_t* pt, uint64_t* values, size_t batch);
/* Galois elements of the slot matrix, host only, no context: 3^(steps mod n/2) mod 2n (negative steps
 * rotate right) and 2n - 1.  n must be a power of two >= 4 (InvalidRingDegree). */
int exacto_galois_element_rotate_rows(size_t n, int64_t steps, uint64_t* element);
int exacto_galois_element_swap_rows(size_t n, uint64_t* element);
/* Row rotation / row swap of ciphertexts: bit for bit exacto_bfv_apply_automorphism with the element
 * above and gk that element's key, with the same errors.  steps == 0 (mod n/2) copies ct (out == ct
 * allowed) and needs no key: gk may be NULL.  Well defined, and working, on a context that cannot
 * batch (the automorphism does not depend on t). */
int exacto_bfv_rotate_rows(exacto_ctx* ctx, const uint64_t* ct, size_t polys, int64_t steps, const uint64_t* gk,
                           size_t num_keys, uint64_t* out, size_t batch);
int exacto_bfv_rotate_rows_dev(exacto_ctx* ctx, const uint64_t* ct, size_t polys, int64_t steps, const uint64_t* gk,
                               size_t num_keys, uint64_t* out, size_t batch);
int exacto_bfv_swap_rows(exacto_ctx* ctx, const uint64_t* ct, size_t polys, const uint64_t* gk, size_t num_keys,
                         uint64_t* out, size_t batch);
int exacto_bfv_swap_rows_dev(exacto_ctx* ctx, const uint64_t* ct, size_t polys, const uint64_t* gk, size_t num_keys,
                             uint64_t* out, size_t batch);
/* ---- Hoisted rotations and slot linear transforms on a prepared Galois key set ----
 * R automorphisms of ONE ciphertext share everything that depends on the ciphertext alone: sigma_k is a
 * ring homomorphism, so sigma_k(c1) == sum_g sigma_k(d_g) B^g with d_g the balanced gadget digits of c1
 * itself, and in the NTT domain sigma_k only permutes evaluations.  c1 is inverse-transformed, decomposed
 * and its digits transformed once; each rotation is a multiply-accumulate whose reads go through a table.
 *
 * exacto_galois_ntt_permutation (host only, no context): perm[p] = the storage position whose value lands
 *   at storage position p under sigma_element, NTT(sigma(a))[p] = NTT(a)[perm[p]], in the library's
 *   NTT-domain order (EXACTO_NTT_ORDER); the same table for every prime.  n: a power of two in 16..16384
 *   (else InvalidRingDegree); element is taken mod 2n and must be odd: InvalidParam "hoisted automorphisms
 *   require odd Galois elements" (exacto_bfv_apply_automorphism keeps accepting even ones).
 *
 * exacto_galois_keyset_create: elements [R] (host memory in both forms), gks [R][num_keys][2][L][n] (NTT
 *   domain; host memory, _dev: device memory), key r that of elements[r].  The set keeps on the device the R
 *   permutation tables and the keys in the form the context's key switch consumes (rows in the 31-bit
 *   basis, or the keys with their Shoup companions), truncated to min(gadget_digits, num_keys) as the
 *   single call does; gks may be released when the call returns.  Element 1 is allowed: its key slot is
 *   never read and its output is a copy of the input; duplicates are allowed.  InvalidParam: R == 0 (or
 *   above 65535), a null pointer, num_keys == 0 unless every element is 1, an even element.
 *   The caller owns the set and destroys every set BEFORE destroying the context it was created on.
 * exacto_galois_keyset_destroy: NULL is a no-op.
 * exacto_galois_keyset_info: R, the keys used per element, and the 31-bit primes of its key switch (0: the
 *   limb-wise multiply-accumulate); any out pointer may be NULL.
 *
 * exacto_bfv_rotate_hoisted: ct [B][2][L][n] -> out [B][R][2][L][n],
 *     out[b][r] = (sigma_r(c0) + sum_g sigma_r(d_g) k_{r,g,0}, sum_g sigma_r(d_g) k_{r,g,1})  per limb,
 *   d_g the digits of the exact CRT of c1 (the decomposition of relinearize; extension semantics for
 *   Q >= 2^64).  This is NOT bit-identical to exacto_bfv_apply_automorphism, which decomposes sigma(c1):
 *   the digits of -x are not minus the digits of x where a digit sits at -B/2.  It decrypts to the same
 *   plaintext under the same noise bound (||sigma(d_g)|| = ||d_g||).
 * exacto_bfv_linear_transform: pts [R][n] plaintext coefficients shared by the batch (lifted as
 *   exacto_bfv_plain_mul lifts them), out [B][2][L][n] = sum_r pts[r] * out_hoisted[b][r]: bit for bit the
 *   composition of exacto_bfv_rotate_hoisted, exacto_bfv_plain_mul and exacto_bfv_add.
 * Both: out must not overlap ct (InvalidParam); a key set prepared on a context with another n, L, primes or
 * gadget base (or another key-switch path) is InvalidParam; batch == 0 returns 0.  They run chunk by chunk
 * (exacto_ctx_set_chunk) with at most R outputs of scratch per chunk item, and leave the state of
 * exacto_bfv_apply_automorphism untouched. */
typedef struct exacto_galois_keyset exacto_galois_keyset;
int exacto_galois_ntt_permutation(size_t n, uint64_t element, uint32_t* perm);
int exacto_galois_keyset_create(exacto_ctx* ctx, const uint64_t* elements, size_t num_elements, const uint64_t* gks,
                                size_t num_keys, exacto_galois_keyset** out);
int exacto_galois_keyset_create_dev(exacto_ctx* ctx, const uint64_t* elements, size_t num_elements, const uint64_t* gks,
                                    size_t num_keys, exacto_galois_keyset** out);
void exacto_galois_keyset_destroy(exacto_galois_keyset* ks);
int exacto_galois_keyset_info(const exacto_galois_keyset* ks, size_t* num_elements, size_t* num_keys_used, int* ks32_primes);
int exacto_bfv_rotate_hoisted(exacto_ctx* ctx, const exacto_galois_keyset* ks, const uint64_t* ct, uint64_t* out,
                              size_t batch);
int exacto_bfv_rotate_hoisted_dev(exacto_ctx* ctx, const exacto_galois_keyset* ks, const uint64_t* ct, uint64_t* out,
                                  size_t batch);
int exacto_bfv_linear_transform(exacto_ctx* ctx, const exacto_galois_keyset* ks, const uint64_t* ct,
                                const uint64_t* pts, uint64_t* out, size_t batch);
int exacto_bfv_linear_transform_dev(exacto_ctx* ctx, const exacto_galois_keyset* ks, const uint64_t* ct,
                                    const uint64_t* pts, uint64_t* out, size_t batch);
/* Compositions on the context's stream, no host round trip: bit for bit exacto_batch_encode followed by
 * exacto_encrypt_sk / exacto_encrypt_pk on the whole batch (values [B][n] instead of pt, the other
 * arguments theirs), and exacto_bfv_decrypt followed by exacto_batch_decode (values_out [B][n]).  The
 * plaintexts live in a context-owned buffer of one chunk (exacto_ctx_set_chunk).  Value range as in
 * exacto_batch_encode: the host forms reject, the _dev forms reduce. */
int exacto_batch_encrypt_sk(exacto_ctx* ctx, const uint64_t* values, const uint64_t* sk, double sigma,
                            const uint64_t* key, uint64_t stream, uint64_t* ct, size_t batch);
int exacto_batch_encrypt_sk_dev(exacto_ctx* ctx, const uint64_t* values, const uint64_t* sk, double sigma,
                                const uint64_t* key, uint64_t stream, uint64_t* ct, size_t batch);
int exacto_batch_encrypt_pk(exacto_ctx* ctx, const uint64_t* values, const uint64_t* pk, double sigma,
                            const uint64_t* key, uint64_t stream, uint64_t* ct, size_t batch);
int exacto_batch_encrypt_pk_dev(exacto_ctx* ctx, const uint64_t* values, const uint64_t* pk, double sigma,
                                const uint64_t* key, uint64_t stream, uint64_t* ct, size_t batch);
int exacto_batch_decrypt(exacto_ctx* ctx, const uint64_t* ct, size_t polys, const uint64_t* sk, uint64_t* values_out,
                         size_t batch);
int exacto_batch_decrypt_dev(exacto_ctx* ctx, const uint64_t* ct, size_t polys, const uint64_t* sk,
                             uint64_t* values_out, size_t batch);

/* ---- Slot-packed dBFV: n integers mod p per dBFV ciphertext (no reference function) ----
 * Slot encoding is a ring isomorphism R_t = Z_t^n, and dbfv_mul / dbfv_square / dbfv_add / dbfv_sub /
 * dbfv_neg / dbfv_relinearize, the reduction with the small representatives, dbfv_div_by_base and
 * dbfv_change_base are Z-linear combinations of BFV products of limbs, so each acts on every slot
 * independently: a dBFV ciphertext [d][2][L][n] whose limb k encrypts the slot encoding of the k-th digits
 * of n values carries n independent integers mod p through all of them, and exacto_dbfv_apply_automorphism
 * with exacto_galois_element_rotate_rows / _swap_rows moves them as it moves BFV slots.  A constant
 * polynomial is "all slots equal", so the digit growth per slot is that of the SCALAR dBFV case, not the
 * n times larger growth of the polynomial case: the scalar bound on t is enough (one product at the u64
 * profile, b = 256, d = 8: t > 2 d (b - 1)^2 = 1040400), and t must be a batching prime, t == 1 (mod 2n),
 * t < 2^32 (the smallest for the u64 profile: 1073153 at n = 4096, 1097729 at n = 8192).
 * dbfv_plain_modulus = 0 (p = 2^64) is ALLOWED in all of these calls: the polynomial entry points reject it
 * as "scalar-only" because a polynomial product mixes coefficients, whereas here every slot is a scalar
 * of its own and wrapping 64-bit arithmetic per slot is exactly dBFV's scalar case.
 *
 * exacto_dbfv_batch_encode: values [B][n] -> pt [B][d][n].  values[b][s] is reduced mod p (taken as is for
 *   p = 2^64, as exacto_dbfv_encrypt_sk does; the host form does not reject, it reduces like the _dev form),
 *   decomposed into d base-b digits (decomposition.rs:8-16, excess digits dropped), and pt[b][k] is the slot
 *   encoding (exacto_batch_encode's: the same zeta, the same slot matrix) of the vector of k-th digits.
 * exacto_dbfv_batch_decode: pt [B][d][n] -> values [B][n].  Every pt[b][k] (any u64, reduced mod t) is slot
 *   decoded, centred at floor(t / 2) and recomposed as sum_k centred_k b^k in i128 with wrapping, then mod p
 *   (p = 2^64: truncation): the arithmetic of exacto_dbfv_decrypt_poly, slot by slot.
 * exacto_dbfv_batch_encrypt_sk / _pk: ct [B][d][2][L][n]; limb k of item b is bit for bit item b*d + k of
 *   exacto_encrypt_sk / exacto_encrypt_pk called with the same (key, stream, sigma) on the [B*d][n]
 *   plaintexts of exacto_dbfv_batch_encode (the guarantee of exacto_dbfv_encrypt_*).  Chunk by chunk
 *   (exacto_ctx_set_chunk) through a context-owned plaintext buffer of d polynomials per chunk item.
 * exacto_dbfv_batch_decrypt: ct [B][d][2][L][n] -> values_out [B][n]: exacto_bfv_decrypt of the B*d limbs,
 *   then exacto_dbfv_batch_decode, chunk by chunk.
 * One fused kernel per direction (batch.hip): one workgroup per item loops over the d digits, so the digit
 * vectors [B][d][n] never exist in memory.
 * Errors, all before any launch and in this order: the context's batching error (above); those of
 * DbfvParams::new ("base must be >= 2", "num_digits must be >= 1", "base^digits = {b^d} < plain_modulus =
 * {p}"); InvalidParam "dBFV base {b} must be <= BFV plaintext modulus {t}".  Also InvalidParam: a null
 * pointer, a _dev values / pt buffer that is not 16-byte aligned, any overlap of values and pt (their
 * sizes differ: there is no in-place form).  batch == 0 returns 0.  The _dev forms are asynchronous on the
 * context's stream, apart from the one wait of a context's first batching call. */
int exacto_dbfv_batch_encode(exacto_ctx* ctx, size_t d, uint64_t base, uint64_t dbfv_plain_modulus,
                             const uint64_t* values, uint64_t* pt, size_t batch);
int exacto_dbfv_batch_encode_dev(exacto_ctx* ctx, size_t d, uint64_t base, uint64_t dbfv_plain_modulus,
                                 const uint64_t* values, uint64_t* pt, size_t batch);
int exacto_dbfv_batch_decode(exacto_ctx* ctx, size_t d, uint64_t base, uint64_t dbfv_plain_modulus,
                             const uint64_t* pt, uint64_t* values, size_t batch);
int exacto_dbfv_batch_decode_dev(exacto_ctx* ctx, size_t d, uint64_t base, uint64_t dbfv_plain_modulus,
                                 const uint64_t* pt, uint64_t* values, size_t batch);
int exacto_dbfv_batch_encrypt_sk(exacto_ctx* ctx, size_t d, uint64_t base, uint64_t dbfv_plain_modulus,
                                 const uint64_t* values, const uint64_t* sk, double sigma, const uint64_t* key,
                                 uint64_t stream, uint64_t* ct, size_t batch);
int exacto_dbfv_batch_encrypt_sk_dev(exacto_ctx* ctx, size_t d, uint64_t base, uint64_t dbfv_plain_modulus,
                                     const uint64_t* values, const uint64_t* sk, double sigma, const uint64_t* key,
                                     uint64_t stream, uint64_t* ct, size_t batch);
int exacto_dbfv_batch_encrypt_pk(exacto_ctx* ctx, size_t d, uint64_t base, uint64_t dbfv_plain_modulus,
                                 const uint64_t* values, const uint64_t* pk, double sigma, const uint64_t* key,
                                 uint64_t stream, uint64_t* ct, size_t batch);
int exacto_dbfv_batch_encrypt_pk_dev(exacto_ctx* ctx, size_t d, uint64_t base, uint64_t dbfv_plain_modulus,
                                     const uint64_t* values, const uint64_t* pk, double sigma, const uint64_t* key,
                                     uint64_t stream, uint64_t* ct, size_t batch);
int exacto_dbfv_batch_decrypt(exacto_ctx* ctx, size_t d, uint64_t base, uint64_t dbfv_plain_modulus,
                              const uint64_t* ct, const uint64_t* sk, uint64_t* values_out, size_t batch);
int exacto_dbfv_batch_decrypt_dev(exacto_ctx* ctx, size_t d, uint64_t base, uint64_t dbfv_plain_modulus,
                                  const uint64_t* ct, const uint64_t* sk, uint64_t* values_out, size_t batch);

/* dBFV plaintext products: public wide operands (weights, a matrix row, a constant vector) applied to dBFV
 * ciphertexts.  No reference function (dbfv/advanced.rs stops at bfv_scalar_plain_mul); the definition is the
 * composition of bfv_plain_mul (bfv/eval.rs:468-486) per digit pair, bfv_add by i + j and over k, and reduce
 * (dbfv/reduction.rs:15-93), bit for bit, in one fused kernel (dbfv_plain.hip).
 *   cts [B][K][d][polys][L][n] (NTT domain, polys >= 1), pts [pt_batch][K][d][n] plaintext coefficients (any
 *   u64, reduced mod each q_l as exacto_bfv_plain_mul lifts them: what exacto_dbfv_batch_encode writes),
 *   pt_batch = B or 1 (1: one plaintext for every item), out [B][d][polys][L][n].
 * With P[k][i] = NTT(pts[k][i] mod q_l) and wide[m] = sum over k and over i + j = m of P[k][i] (.) cts[k][j]
 * (m = 0 .. 2d-2): out[i] = wide[i] + sum_{m >= d} rep[m-d][i] wide[m], rep = SmallReps::compute_simple(base,
 * d, p) (lattice.rs:104-122), canonical residues mod q_l.  Pairs whose wide limb has an all-zero
 * representative are not formed (p = 2^64, b = 256, d = 8: only i + j < d, as in exacto_dbfv_mul_plan).
 * exacto_dbfv_plain_mul is K = 1.  depth_ct: host [B][K] (NULL = 0); depth_out[b] = max_k depth + 1 (NULL
 * allowed).  A plaintext product grows the digits as a ciphertext product does: an input depth >= 1 is
 * exacto_dbfv_mul's NotImplemented error.  The plaintexts are lifted into a context-owned buffer of at
 * most exacto_ctx_set_plain_terms terms (default 64; 0 restores it) for one plaintext, or for one chunk of
 * items (exacto_ctx_set_chunk) with plaintexts of their own; a later term chunk adds into out.  Neither
 * setting changes a result.  A batching context is NOT required: the product is defined for any plaintext
 * polynomials, and slot semantics is the caller's encoding.
 * exacto_dbfv_plain_add / _sub: ct [B][d][polys][L][n], pt [pt_batch][d][n] -> out likewise; limb k of the
 *   output is exacto_bfv_plain_add of limb k and digit k, c0 + NTT(Delta m) (sub: c0 - NTT(Delta m)), the other
 *   components copied; depth unchanged; out may be ct.
 * Errors, all before any launch and in this order: the context's; InvalidParam for a null pointer; K == 0
 * ("mismatched ct/pt lengths"); polys == 0; pt_batch not in {1, B}; those of DbfvParams::new (_add / _sub:
 * d == 0 only); more than 64 digits; the depth error; a _dev buffer that is not 16-byte aligned (products
 * only); out overlapping cts or pts (products only).  batch == 0 returns 0.  The _dev forms are asynchronous
 * on the context's stream.
 * exacto_dbfv_plain_limits: what a test needs to cross both chunkings: the products one 128-bit accumulator of
 * the kernel takes between two reductions (2^(128 - 2 s) - 2 for the largest prime's bit length s, at most
 * 2^20; the registers form, d <= 8, reduces every flush_products / d terms) and the term chunk. */
int exacto_dbfv_plain_mul_sum(exacto_ctx* ctx, size_t d, uint64_t base, uint64_t dbfv_plain_modulus,
                              const uint64_t* cts, size_t K, size_t polys, const uint64_t* pts, size_t pt_batch,
                              uint64_t* out, size_t batch, const uint32_t* depth_ct, uint32_t* depth_out);
int exacto_dbfv_plain_mul_sum_dev(exacto_ctx* ctx, size_t d, uint64_t base, uint64_t dbfv_plain_modulus,
                                  const uint64_t* cts, size_t K, size_t polys, const uint64_t* pts, size_t pt_batch,
                                  uint64_t* out, size_t batch, const uint32_t* depth_ct, uint32_t* depth_out);
int exacto_dbfv_plain_mul(exacto_ctx* ctx, size_t d, uint64_t base, uint64_t dbfv_plain_modulus, const uint64_t* ct,
                          size_t polys, const uint64_t* pt, size_t pt_batch, uint64_t* out, size_t batch,
                          const uint32_t* depth_ct, uint32_t* depth_out);
int exacto_dbfv_plain_mul_dev(exacto_ctx* ctx, size_t d, uint64_t base, uint64_t dbfv_plain_modulus,
                              const uint64_t* ct, size_t polys, const uint64_t* pt, size_t pt_batch, uint64_t* out,
                              size_t batch, const uint32_t* depth_ct, uint32_t* depth_out);
int exacto_dbfv_plain_add(exacto_ctx* ctx, size_t d, const uint64_t* ct, size_t polys, const uint64_t* pt,
                          size_t pt_batch, uint64_t* out, size_t batch);
int exacto_dbfv_plain_add_dev(exacto_ctx* ctx, size_t d, const uint64_t* ct, size_t polys, const uint64_t* pt,
                              size_t pt_batch, uint64_t* out, size_t batch);
int exacto_dbfv_plain_sub(exacto_ctx* ctx, size_t d, const uint64_t* ct, size_t polys, const uint64_t* pt,
                          size_t pt_batch, uint64_t* out, size_t batch);
int exacto_dbfv_plain_sub_dev(exacto_ctx* ctx, size_t d, const uint64_t* ct, size_t polys, const uint64_t* pt,
                              size_t pt_batch, uint64_t* out, size_t batch);
int exacto_ctx_set_plain_terms(exacto_ctx* ctx, size_t terms);
int exacto_dbfv_plain_limits(exacto_ctx* ctx, size_t* flush_products, size_t* chunk_terms);

/* ---- Slot linear transforms on dBFV ciphertexts with public wide diagonals ----
 * The join of the hoisted rotations with the dBFV plaintext products: a public matrix over Z_p (p up to 2^64)
 * applied to an encrypted vector of wide slots by the diagonal method, out = reduce(sum_r W_r * rot_{k_r}(x)).
 * No reference function.  The definition, bit for bit: with ct [B][d][2][L][n] (NTT domain), a key set of R
 * elements and H [B*d][R][2][L][n] = exacto_bfv_rotate_hoisted of the B*d limbs taken as BFV ciphertexts,
 *     out [B][d][2][L][n] = exacto_dbfv_plain_mul_sum(cts[b][r][j] = H[b*d + j][r], K = R, polys = 2,
 *                                                     pts [R][d][n] with pt_batch = 1),
 * canonical residues: the same SmallReps::compute_simple fold and the same skipped pairs, the same depth rule
 * (an input depth >= 1 is NotImplemented, depth_out[b] = depth_ct[b] + 1; depth_ct host [B], NULL = 0;
 * depth_out NULL allowed), and the same bits on both key-switch paths.  pts are plaintext coefficients (any
 * u64); in the slot case what exacto_dbfv_batch_encode writes for R value vectors.
 *
 * exacto_dbfv_rotate_hoisted: ct [B][d][2][L][n] -> out [B][R][d][2][L][n]: every out[b][r] is a dBFV
 *   ciphertext, limb j of it bit for bit exacto_bfv_rotate_hoisted's out[b*d + j][r]; written in place by the
 *   rotation kernels, no copy.  out must not overlap ct; d == 0 is InvalidParam.  exacto_ctx_set_chunk counts
 *   BFV limbs: a chunk is max(1, chunk / d) dBFV ciphertexts.
 * exacto_dbfv_diagonals_create: pts [R][d][n] (host memory, _dev: device memory) lifted once (reduced mod each
 *   q_l and transformed, as the products lift them) into a device buffer [R][d][L][n] owned by the handle; pts
 *   may be released when the call returns.  InvalidParam: a null pointer, d == 0 or d > 64, R == 0 or above
 *   65535.  The caller owns the handle and destroys it BEFORE destroying the context it was created on.
 * exacto_dbfv_diagonals_destroy: NULL is a no-op.
 * exacto_dbfv_diagonals_info: R, d, and the route a transform of d digits takes on the context the handle was
 *   made on (0: the staged route, rotations into per-chunk scratch read in place by the plaintext-product
 *   kernel: the default; 1: the fused kernel, dbfv_hoist.hip, after exacto_ctx_set_dbfv_lt_fused(ctx, 1) on the
 *   limb-wise key switch with d <= 8), as it was when the handle was made; any out pointer may be NULL.
 * exacto_ctx_set_dbfv_lt_fused: on != 0 sends the limb-wise key switch with d <= 8 through the fused kernel, on
 *   = 0 (the default: the staged route measured twice as fast) restores the staged route.  For tests and
 *   measurements, not a tuning knob: no result depends on it.
 * exacto_dbfv_linear_transform: the raw diagonals pts [R][d][n], lifted on every call into the context-owned
 *   buffer exacto_ctx_set_plain_terms rotations at a time, a later group of rotations adding into out.
 * exacto_dbfv_linear_transform_prepared: the handle instead of pts: no lift and no term chunking.
 * Neither exacto_ctx_set_chunk nor exacto_ctx_set_plain_terms changes a result.  The scratch of the staged
 * route stays within R outputs per chunk limb; on the fused route no rotated limb is ever stored.
 * Errors of the two transforms, all before any launch and in this order: the context's; InvalidParam for a
 * null pointer; a key set prepared on a context with other parameters, or for another key-switch path; those
 * of DbfvParams::new; more than 64 digits; a handle from a context with another n, L or primes, then a handle
 * whose R or d differs from the key set's R or from d; the depth error; a _dev buffer that is not 16-byte
 * aligned; out overlapping ct or pts.  batch == 0 returns 0.  The _dev forms are asynchronous on the context's
 * stream.  The state of exacto_bfv_apply_automorphism and of the BFV hoisted calls stays untouched. */
typedef struct exacto_dbfv_diagonals exacto_dbfv_diagonals;
int exacto_dbfv_rotate_hoisted(exacto_ctx* ctx, const exacto_galois_keyset* ks, size_t d, const uint64_t* ct,
                               uint64_t* out, size_t batch);
int exacto_dbfv_rotate_hoisted_dev(exacto_ctx* ctx, const exacto_galois_keyset* ks, size_t d, const uint64_t* ct,
                                   uint64_t* out, size_t batch);
int exacto_dbfv_diagonals_create(exacto_ctx* ctx, size_t d, size_t num_elements, const uint64_t* pts,
                                 exacto_dbfv_diagonals** out);
int exacto_dbfv_diagonals_create_dev(exacto_ctx* ctx, size_t d, size_t num_elements, const uint64_t* pts,
                                     exacto_dbfv_diagonals** out);
void exacto_dbfv_diagonals_destroy(exacto_dbfv_diagonals* dg);
int exacto_dbfv_diagonals_info(const exacto_dbfv_diagonals* dg, size_t* num_elements, size_t* d, int* fused);
int exacto_ctx_set_dbfv_lt_fused(exacto_ctx* ctx, int on);
int exacto_dbfv_linear_transform(exacto_ctx* ctx, const exacto_galois_keyset* ks, size_t d, uint64_t base,
                                 uint64_t dbfv_plain_modulus, const uint64_t* ct, const uint64_t* pts, uint64_t* out,
                                 size_t batch, const uint32_t* depth_ct, uint32_t* depth_out);
int exacto_dbfv_linear_transform_dev(exacto_ctx* ctx, const exacto_galois_keyset* ks, size_t d, uint64_t base,
                                     uint64_t dbfv_plain_modulus, const uint64_t* ct, const uint64_t* pts,
                                     uint64_t* out, size_t batch, const uint32_t* depth_ct, uint32_t* depth_out);
int exacto_dbfv_linear_transform_prepared(exacto_ctx* ctx, const exacto_galois_keyset* ks, size_t d, uint64_t base,
                                          uint64_t dbfv_plain_modulus, const uint64_t* ct,
                                          const exacto_dbfv_diagonals* dg, uint64_t* out, size_t batch,
                                          const uint32_t* depth_ct, uint32_t* depth_out);
int exacto_dbfv_linear_transform_prepared_dev(exacto_ctx* ctx, const exacto_galois_keyset* ks, size_t d,
                                              uint64_t base, uint64_t dbfv_plain_modulus, const uint64_t* ct,
                                              const exacto_dbfv_diagonals* dg, uint64_t* out, size_t batch,
                                              const uint32_t* depth_ct, uint32_t* depth_out);

/* Plaintext-ciphertext operations (CoeffsToSlots' linear layer), all in the NTT domain.
 * ct/out [B][polys][L][n]; pt [B][n] plaintext coefficients (any u64, reduced mod each q_i).
 *   bfv_plain_mul     replaces bfv::eval::bfv_plain_mul      (src/bfv/eval.rs:468-486)
 *   bfv_plain_add     replaces bfv::eval::bfv_plain_add      (src/bfv/eval.rs:489-503), c0 + Delta m
 *   bfv_inner_product replaces bfv::eval::bfv_inner_product  (src/bfv/eval.rs:588-606):
 *                     cts [K][polys][L][n], pts [K][n] -> out [polys][L][n]; K == 0 is InvalidParam
 *   bfv_monomial_mul  replaces bfv::eval::bfv_monomial_mul   (src/bfv/eval.rs:613-652), X^j, j mod 2n
 *   bfv_trace         replaces bfv::eval::bfv_trace          (src/bfv/eval.rs:572-586): elements is a
 *                     HOST array [E]; gks [E][num_keys][2][L][n] holds the key of elements[e] at e. */
int exacto_bfv_plain_mul(exacto_ctx* ctx, const uint64_t* ct, size_t polys, const uint64_t* pt, uint64_t* out,
                         size_t batch);
int exacto_bfv_plain_mul_dev(exacto_ctx* ctx, const uint64_t* ct, size_t polys, const uint64_t* pt, uint64_t* out,
                             size_t batch);
int exacto_bfv_plain_add(exacto_ctx* ctx, const uint64_t* ct, size_t polys, const uint64_t* pt, uint64_t* out,
                         size_t batch);
int exacto_bfv_plain_add_dev(exacto_ctx* ctx, const uint64_t* ct, size_t polys, const uint64_t* pt, uint64_t* out,
                             size_t batch);
int exacto_bfv_inner_product(exacto_ctx* ctx, const uint64_t* cts, const uint64_t* pts, size_t K, size_t polys,
                             uint64_t* out);
int exacto_bfv_inner_product_dev(exacto_ctx* ctx, const uint64_t* cts, const uint64_t* pts, size_t K, size_t polys,
                                 uint64_t* out);
int exacto_bfv_monomial_mul(exacto_ctx* ctx, const uint64_t* ct, size_t polys, uint64_t j, uint64_t* out,
                            size_t batch);
int exacto_bfv_monomial_mul_dev(exacto_ctx* ctx, const uint64_t* ct, size_t polys, uint64_t j, uint64_t* out,
                                size_t batch);
int exacto_bfv_trace(exacto_ctx* ctx, const uint64_t* ct, size_t polys, const uint64_t* elements, size_t E,
                     const uint64_t* gks, size_t num_keys, uint64_t* out, size_t batch);
int exacto_bfv_trace_dev(exacto_ctx* ctx, const uint64_t* ct, size_t polys, const uint64_t* elements, size_t E,
                         const uint64_t* gks, size_t num_keys, uint64_t* out, size_t batch);

/* CoeffsToSlots / SlotsToCoeffs (src/bootstrap/coeffs_to_slots.rs).
 *   exacto_required_trace_elements replaces required_trace_elements (coeffs_to_slots.rs:168-183):
 *     pure host function, writes up to cap elements and returns how many there are.
 *   exacto_extract_coefficients replaces extract_coefficient (coeffs_to_slots.rs:21-49) for the J
 *     indices j0 .. j0+J-1 of one ciphertext ct [2][L][n] -> out [J][2][L][n] (coeffs_to_slots,
 *     coeffs_to_slots.rs:103-115, is j0 = 0, J = n).  (elements [E] host, gks [E][num_keys][2][L][n])
 *     is the reference's HashMap<element, GaloisKey>; a required element missing from it is
 *     InvalidParam "missing Galois key for element k"; n not invertible mod t is InvalidParam.
 *   exacto_slots_to_coeffs replaces slots_to_coeffs (coeffs_to_slots.rs:121-145): slots
 *     [S][polys][L][n] -> out [polys][L][n]; S == 0 "empty slots", S != n "expected n slots, got S". */
size_t exacto_required_trace_elements(size_t n, uint64_t* out, size_t cap);
int exacto_extract_coefficients(exacto_ctx* ctx, const uint64_t* ct, uint64_t j0, size_t J, const uint64_t* elements,
                                size_t E, const uint64_t* gks, size_t num_keys, uint64_t* out);
int exacto_extract_coefficients_dev(exacto_ctx* ctx, const uint64_t* ct, uint64_t j0, size_t J,
                                    const uint64_t* elements, size_t E, const uint64_t* gks, size_t num_keys,
                                    uint64_t* out);
int exacto_slots_to_coeffs(exacto_ctx* ctx, const uint64_t* slots, size_t S, size_t polys, uint64_t* out);
int exacto_slots_to_coeffs_dev(exacto_ctx* ctx, const uint64_t* slots, size_t S, size_t polys, uint64_t* out);

/* Digit extraction (src/bootstrap/digit_extract.rs).
 *   exacto_lagrange_interpolate replaces lagrange_interpolate (digit_extract.rs:37-90): host only,
 *     out [n]; a zero denominator (points not distinct mod p) is InvalidParam (the reference panics).
 *   exacto_compute_rounding_poly replaces compute_rounding_poly (digit_extract.rs:19-30): host only,
 *     out [t_boot].
 *   exacto_trivial_encrypt replaces trivial_encrypt_poly (digit_extract.rs:179-189): pt [B][n] ->
 *     (Delta m, 0) [B][2][L][n]; trivial_encrypt(m) is pt = (m mod t, 0, ..., 0).
 *   exacto_eval_poly replaces eval_poly_homomorphic (digit_extract.rs:101-157) on B ciphertexts at
 *     once with the reference's Paterson-Stockmeyer schedule; coeffs is a HOST array [m], m >= 1;
 *     the relinearisation key is the context's resident one (MissingKey if none). */
int exacto_lagrange_interpolate(const uint64_t* values, size_t n, uint64_t p, uint64_t* out);
int exacto_compute_rounding_poly(uint64_t t_orig, uint64_t q_prime, uint64_t t_boot, uint64_t* out);
int exacto_trivial_encrypt(exacto_ctx* ctx, const uint64_t* pt, uint64_t* out, size_t batch);
int exacto_trivial_encrypt_dev(exacto_ctx* ctx, const uint64_t* pt, uint64_t* out, size_t batch);
int exacto_eval_poly(exacto_ctx* ctx, const uint64_t* ct, const uint64_t* coeffs, size_t m, uint64_t* out,
                     size_t batch);
int exacto_eval_poly_dev(exacto_ctx* ctx, const uint64_t* ct, const uint64_t* coeffs, size_t m, uint64_t* out,
                         size_t batch);

/* Bootstrapping (src/bootstrap/bfv_host.rs), over two contexts on one device: `orig` (the scheme
 * being refreshed; ONE ciphertext prime, because the reference switches from moduli[0] after
 * to_coeff_poly, bfv_host.rs:149-157) and `boot` (same n).
 *   exacto_bootstrap_key_material replaces the key-material half of gen_bootstrap_key and
 *     create_boot_sk (bfv_host.rs:57-100, 289-330): sk [1][n] (NTT) -> boot_sk [Lb][n] (NTT) and the
 *     plaintext s_pt [n] that bsk encrypts.  bsk, boot_rlk and the trace keys are then made with
 *     exacto_encrypt_sk / exacto_gen_relin_key / exacto_gen_galois_key on `boot`.
 *   exacto_bfv_bootstrap replaces bfv_bootstrap (bfv_host.rs:131-205) for B ciphertexts:
 *     ct [B][2][1][n] -> out [B][2][Lb][n]; bsk [2][Lb][n]; rpoly [m] HOST (compute_rounding_poly);
 *     (elements [E] HOST, gks [E][num_keys][2][Lb][n]) the trace keys; boot's resident relin key is
 *     boot_rlk.  Items with c1 = 0 take the trivial path (bfv_host.rs:180-186), the rest the full
 *     ring path (CoeffsToSlots -> rounding polynomial on the n slots at once -> SlotsToCoeffs). */
int exacto_bootstrap_key_material(exacto_ctx* orig, exacto_ctx* boot, const uint64_t* sk, uint64_t* boot_sk,
                                  uint64_t* s_pt);
int exacto_bootstrap_key_material_dev(exacto_ctx* orig, exacto_ctx* boot, const uint64_t* sk, uint64_t* boot_sk,
                                      uint64_t* s_pt);
int exacto_bfv_bootstrap(exacto_ctx* orig, exacto_ctx* boot, const uint64_t* ct, size_t polys, const uint64_t* bsk,
                         const uint64_t* rpoly, size_t m, uint64_t q_prime, const uint64_t* elements, size_t E,
                         const uint64_t* gks, size_t num_keys, uint64_t* out, size_t batch);
int exacto_bfv_bootstrap_dev(exacto_ctx* orig, exacto_ctx* boot, const uint64_t* ct, size_t polys,
                             const uint64_t* bsk, const uint64_t* rpoly, size_t m, uint64_t q_prime,
                             const uint64_t* elements, size_t E, const uint64_t* gks, size_t num_keys, uint64_t* out,
                             size_t batch);

/* ---- RCCL collectives over xGMI ----
 * Replace the host-side key distribution of the reference (keys built once, keygen.rs:123-209, and
 * shared by every rayon worker) with one broadcast per key to every GPU, and gather the output limbs
 * of a split dbfv_mul.  `comm` is an ncclComm_t (RCCL), as void*: made by exacto_rccl_comm_init or by
 * the caller's own RCCL.  RCCL is opened at first use (librccl.so.1, or $EXACTO_RCCL_LIB); failures
 * return EXACTO_ERR_HIP with an "RCCL error: ..." message.  All collectives are enqueued on the
 * context's stream.
 *   exacto_rccl_unique_id      ncclGetUniqueId -> id[128] (rank 0; share it out of band)
 *   exacto_rccl_comm_init      ncclCommInitRank on `device`
 *   exacto_rccl_comm_count     ncclCommCount: the ranks the communicator spans (bench lines record it)
 *   exacto_ctx_broadcast_relin_key   root's resident relinearisation key -> every rank's resident key
 *                              (in place; non-root ranks need no prior load), num_keys = [G] rows.
 *                              Collective agreement first: every rank all-gathers {num_keys, verdict},
 *                              so a root without a key of that size, or ranks passing different
 *                              num_keys, fail with InvalidParam on EVERY rank, keys untouched
 *   exacto_broadcast_galois_key      a device Galois key buffer [num_keys][2][L][n], in place
 *   exacto_rccl_allgather_u64  recv = [nranks][count] u64 (never a reduction: residues are not summable
 *                              by RCCL)
 *   exacto_rccl_sync           waits for the context stream (the collectives enqueued on it) with a deadline
 * Deadlines: communicator init, the agreement all-gather and exacto_rccl_sync wait at most
 * $EXACTO_RCCL_TIMEOUT_S seconds (default 300, 0 = forever) for the other ranks; on expiry they return
 * EXACTO_ERR_HIP "RCCL error: ... timed out" (a collective's communicator is aborted with ncclCommAbort,
 * after which exacto_rccl_comm_destroy on it is a no-op), so a rank that never joins cannot block the
 * others for good. */
int exacto_rccl_unique_id(uint8_t* id);
int exacto_rccl_comm_init(void** comm, int nranks, const uint8_t* id, int rank, int device);
int exacto_rccl_comm_destroy(void* comm);
int exacto_rccl_comm_count(void* comm, int* nranks);
int exacto_ctx_broadcast_relin_key(exacto_ctx* ctx, void* comm, int root, size_t num_keys);
int exacto_broadcast_galois_key(exacto_ctx* ctx, void* comm, int root, uint64_t* gk_dev, size_t num_keys);
int exacto_rccl_allgather_u64(exacto_ctx* ctx, void* comm, const uint64_t* send, uint64_t* recv, size_t count);
int exacto_rccl_sync(exacto_ctx* ctx, void* comm);

size_t exacto_last_error(char* buf, size_t len);
/* Per-kernel-family timing of the last profiled calls: enable, then read
 * (kind 0 = forward NTT, 1 = inverse NTT): launches, summed device ms, summed algorithmic
 * bytes (16*n per polynomial). */
int exacto_prof_enable(exacto_ctx* ctx, int enable);
int exacto_prof_read(exacto_ctx* ctx, int kind, uint64_t* launches, double* total_ms,
                     double* total_bytes, uint64_t* polys);
/* The kernels that ran for one family in the records exacto_prof_read consumed (since the last call for
 * that kind), named as rocprofv3 names them ("exacto::ntt_fwd_pin_kernel<12, 0, false>"), by descending
 * event time: "name (launches, ms); ...".  Returns the full length (snprintf-like); buf may be NULL (a
 * size query, which keeps the list; a call with a buffer clears it). */
size_t exacto_prof_kernels(exacto_ctx* ctx, int kind, char* buf, size_t len);
const char* exacto_version(void);

#ifdef __cplusplus
}
#endif
#endif /* EXACTO_HIP_H */
